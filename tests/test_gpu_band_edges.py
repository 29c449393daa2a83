"""The banded sweep (dp_fill_band16, smoothxg_amd/csrc/poa_band16.hip.h) at the edges of its own machinery, every block against
the live scalar oracle -- graph, paths, scores, consensus and the band cells of every sequence -- and with the class that ran
read from the SXG_POA_DEBUG variant line: strip width, band cell bytes, gap model.  The inputs and what the oracle says about
them (which window states they reach) are in tests/band_edges.py; tests/test_band_edges_inputs.py asserts the same facts
without a GPU.

  (a) both sides of each change of the strip width (decree B2): 2 266 | 2 267 and 6 466 | 6 467 letters; a block whose first
      sequence alone sets W = 11
  (b) the last strip: sequences of k W - 1, k W, k W + 1 letters (column L alone in its strip; the adaptive band's best-cell
      search must ignore the columns beyond L), local and global; one-letter sequences, an empty block
  (c) rows without a band (static band, a short sequence on a long backbone)
  (d) a full window that moves: every band move a re-centre, stored predecessors from earlier window origins, the 2-byte path's
      read of the strip left of the window, four predecessors
  (e) ties for the end cell, across a window re-centre and inside one strip (decree S4)
  (f) the key fold at 65 536 rows

Which line of poa_band16.hip.h each of (c) - (f) stands on:
  (c) `if (bh >= bl) cells += ...` and the re-centre's `bh >= bl &&` guard (an empty band neither counts nor moves the window),
      `in_lo` / `in_hi` (nothing stored: P16_SLOT_OOB; nothing in the keys: `rowmax & m2`), and BAND_FETCH's `a_` / `b_` /
      `la_` / `lb_` for the rows of the third sequence that read an empty-band row's strips as NEGCELL
  (d) the re-centre block (`s0 = max(0, bl - (BAND_WIN - (bh - bl + 1)) / 2)`, `regs_ok = false`, the letters, `so_lo` / `so_hi`),
      BAND_FETCH / BAND_FETCH2's fetch by absolute strip (`% BS`), BAND_FETCH2's `if (s0 >= 1 && s0 - 1 >= fl_ && s0 - 1 <= fh_
      && bl == s0)` read of the strip left of the window, and the `for (int x = 2; x < np; ++x)` / `g_preds[pb + x]` paths
  (e) `fold_keys` at a re-centre (`if (SW && s0 > -1000000) fold_keys(i, s0)`) and its `ku > ekey` (first strictly greatest
      row, then smallest strip); inside a strip `key_lo = max(key_lo, ...)` with the row in the low half
  (f) `if ((i & 0xffff) == 0) fold_keys(i, s0)` and the epoch `ep` of fold_keys"""
import re
import time

import pytest

import band_edges as B
from helpers import assert_block_equal
from oracle import oracle_py as O
from smoothxg_amd import Params

pytestmark = pytest.mark.gpu

VARIANT_LINE = re.compile(r"^\[sxg\] variant T=(\d+) W=(\d+) cvx=(\d+) rowmode=(\d+) attempt=(\d+) .* tmax=(\d+) cb=(\d+) ds=(\d+) w2=(\d+)$", re.M)
LOCAL_BOTH = ((0, 1), (0, 2))              # (alignment mode, band mode): the static and the adaptive band
ALL_MODES = LOCAL_BOTH + ((1, 2),)         # ... and global alignment, adaptive band


def run(engine, monkeypatch, capfd, blocks, scores, modes, want_w, label, knob4=False, oracle_results=None, arena_retries=False):
    """Every block under every (alignment mode, band mode) of `modes` in ONE batch (per-block parameters: blocks of one strip
    width, gap model and alignment mode share a launch), against the oracle.  want_w: the strip widths the variant lines must
    name, as a set -- every line must say row mode 3, 64 threads, tmax 64, ds 0, w2 0, the gap model and the cell bytes.
    arena_retries: the block may outgrow its arena and run again in a larger one (a graph of unrelated sequences grows by a
    node per letter) -- on the same class: later attempts must name it too.
    Returns the oracle's results, which a re-run with other band cells passes back in (they do not depend on the format)."""
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    if knob4:
        monkeypatch.setenv("SXG_POA_BAND_CELL_BYTES", "4")
    else:
        monkeypatch.delenv("SXG_POA_BAND_CELL_BYTES", raising=False)
    batch = [(blk, md, bnd) for blk in blocks for md, bnd in modes]
    t0 = time.perf_counter()
    if oracle_results is None:
        oracle_results = [O.block_run(blk, None, O.mkparams(*scores, mode=md, banded=bnd)) for blk, md, bnd in batch]
    t1 = time.perf_counter()
    capfd.readouterr()
    res = engine.run_blocks([x[0] for x in batch], [Params(*scores, md, bnd) for _, md, bnd in batch], want_consensus=True)
    t2 = time.perf_counter()
    st = engine.stats()
    err = capfd.readouterr().err
    print("%s%s: oracle %.2f s, engine %.2f s" % (label, " cb4" if knob4 else "", t1 - t0, t2 - t1))
    for k, ((blk, md, bnd), (g, sc, cells)) in enumerate(zip(batch, oracle_results)):
        what = "%s/block%d/%s/banded=%d%s" % (label, k // len(modes), "global" if md else "local", bnd, "/cb4" if knob4 else "")
        assert_block_equal(res[k], g, sc, cells, label=what)
        assert (res[k].consensus == g.consensus()).all(), what
    lines = [tuple(map(int, x)) for x in VARIANT_LINE.findall(err)]
    print(label, "cb4" if knob4 else "", lines)
    cvx = int(scores[2] < scores[3] and scores[2] > scores[4] and scores[3] < scores[5])
    for T, W, lcvx, rm, attempt, tmax, cb, ds, w2 in lines:
        sw_cb = 2 if not knob4 and tuple(scores) != B.CB4 else 4
        assert (T, rm, tmax, ds, w2, lcvx) == (64, 3, 64, 0, 0, cvx) and (attempt == 0 or arena_retries), (label, lines)
        assert cb in ((sw_cb,) if all(md == 0 for md, _ in modes) else (sw_cb, 4)), (label, lines)
    assert {x[1] for x in lines} == set(want_w), (label, lines)
    assert st["dom_row_mode"] == 3 and st["dom_threads"] == 64 and (st["retries"] == 0 or arena_retries), (label, st)
    return oracle_results


def both_cell_formats(engine, monkeypatch, capfd, blocks, scores, modes, want_w, label):
    ref = run(engine, monkeypatch, capfd, blocks, scores, modes, want_w, label)
    run(engine, monkeypatch, capfd, blocks, scores, modes, want_w, label, knob4=True, oracle_results=ref)
    return ref


# ---- (a) both sides of each strip-width change

@pytest.mark.parametrize("top,W", [(2266, 6), (2267, 8), (6466, 8), (6467, 11)])
def test_both_sides_of_a_strip_width_change(engine, monkeypatch, capfd, top, W):
    """The longest sequence one letter before and one letter behind the change (three sequences at 2 266 | 2 267, a pair at
    6 466 | 6 467): the variant line names W, with 2-byte cells, with 4-byte cells under the knob and with 4-byte cells by the
    scores (cb4_convex).  This holds the product's band_strip_width (a HIP header) equal to the oracle's at its two changes."""
    assert B.strip_width(top) == W and B.strip_width(top + (1 if W == 6 or top == 6466 else -1)) != W
    blk = B.width_change_block(top, 3 if top < 3000 else 2)
    assert max(len(s) for s in blk) == top == len(blk[0])
    both_cell_formats(engine, monkeypatch, capfd, [blk], B.DEFAULT, LOCAL_BOTH, {W}, "width-change/%d" % top)
    run(engine, monkeypatch, capfd, [blk], B.CB4, LOCAL_BOTH, {W}, "width-change/%d/cb4_convex" % top)


def test_the_first_sequence_alone_sets_the_strip_width(engine, monkeypatch, capfd):
    """6 500 letters first (W = 11), then sequences of 300 - 900 letters: band_w from each sequence's own length, the strip width
    from the block's; the last strip of the short ones lies far left of where the window of a 6 500-letter sequence would be."""
    blk = B.long_first_block()
    assert B.strip_width(len(blk[0])) == 11 and all(300 <= len(s) <= 900 and B.strip_width(len(s)) == 6 for s in blk[1:])
    both_cell_formats(engine, monkeypatch, capfd, [blk], B.DEFAULT, LOCAL_BOTH, {11}, "long-first")


# ---- (b) the last strip

def test_the_last_strip(engine, monkeypatch, capfd):
    """k W - 1, k W, k W + 1 letters at W = 6 for k = 5 (one lane's worth), k = 127 (column L in the LAST strip of the window at
    origin 0: lane 63's high half) and k = 128 (one strip more: the window must move for the strip of column L alone), in local
    mode with both bands and in global mode, where the end cell is column L of a sink row; one-letter sequences, a block of one
    one-letter sequence, an empty block."""
    blocks = [B.last_strip_block(k) for k in (5, 127, 128)]
    for k, blk in zip((5, 127, 128), blocks):
        assert sorted({len(s) for s in blk}) == [6 * k - 1, 6 * k, 6 * k + 1] and {len(s) // 6 for s in blk} == {k - 1, k}
    both_cell_formats(engine, monkeypatch, capfd, blocks + B.tiny_blocks(), B.DEFAULT, ALL_MODES, {6}, "last-strip")
    run(engine, monkeypatch, capfd, blocks, B.AFFINE, ALL_MODES, {6}, "last-strip/affine")


# ---- (c) rows without a band

@pytest.mark.parametrize("at_end", [False, True], ids=["start", "end"])
def test_rows_without_a_band(engine, monkeypatch, capfd, at_end):
    """Static band.  A 100-letter sequence on a 2 000-letter backbone: every row beyond backbone coordinate L + w has no band --
    nothing swept, nothing stored, nothing in the keys -- then a full-length sequence that reads rows of both.  at_end: the
    short sequence matches the backbone's END only, finds nothing inside its band and is added as a new chain."""
    blk = B.empty_band_block(int(at_end))
    facts = B.check_empty_bands(O, blk)     # (more than half of the rows have no band; cells = the sum of the others)
    ref = both_cell_formats(engine, monkeypatch, capfd, [blk], B.DEFAULT, ((0, 1),), {6}, "empty-bands/%d" % at_end)
    assert int(ref[0][2][1]) == facts[0]["cells"]
    if at_end:
        assert int(ref[0][1][1]) < 20 and ref[0][0].n_nodes > len(blk[0]) + 80


# ---- (d) a full window that moves

@pytest.mark.parametrize("ins", [300, 420])
def test_a_full_window_that_moves(engine, monkeypatch, capfd, ins):
    """The bars, asserted on the oracle's graphs (band_edges.check_moving_window): in the sweep of the last, 2 266-letter sequence
    at least ten re-centres, a stored predecessor swept under an earlier window origin, a stored predecessor whose band holds
    the strip left of the window while the row's band begins at the window's origin, a row with three or more predecessors."""
    blk = B.moving_window_block(ins)
    B.check_moving_window(O, blk)
    ref = both_cell_formats(engine, monkeypatch, capfd, [blk], B.DEFAULT, LOCAL_BOTH, {6}, "moving-window/%d" % ins)
    full = O.block_run(blk, None, O.mkparams(*B.DEFAULT, mode=0, banded=0))[1]
    static, adaptive = ref[0][1], ref[1][1]
    if ins == 300:     # inside w = 378: kept by both bands
        assert (static == full).all() and (adaptive == full).all()
    else:              # beyond: the static band loses the second sequence's alignment, the adaptive band keeps it
        assert static[1] < full[1] == adaptive[1]


# ---- (e) ties for the end cell

def test_ties_for_the_end_cell(engine, monkeypatch, capfd):
    """Two end cells of the same score (checked on the oracle by aligning each alone): in different strips with a hundred window
    re-centres between them, and in the same column of one window that never moves.  First strictly greatest row, then smallest
    column (decree S4) must pick the oracle's cell; the blocks with one of the two windows spoiled show that either is found."""
    for bnd in (1, 2):
        B.check_ties(O, bnd)
    a, q, q1, q2 = B.tie_far_block()
    both_cell_formats(engine, monkeypatch, capfd, [[a, q], [a, q1], [a, q2]] + [list(x) for x in B.tie_same_strip_block()], B.DEFAULT,
                      LOCAL_BOTH, {6}, "ties")


# ---- (f) the key fold at 65 536 rows

def test_the_key_fold_at_65536_rows(engine, monkeypatch, capfd):
    """Four unrelated sequences of ~18 kbp (the fewest that pass 65 536 rows), then 1 200 letters: 600 of the last long sequence's
    start and 600 of the first one's, both worth 600.  Static band, default scores.  The last sweep runs over 71 361 rows: its
    keys are folded at row 65 536 and at the end, in two row epochs.  (The bands of a 1 200-letter sequence end where the backbone
    coordinates pass L + w: its cells lie in the first 21 000 rows, so the fold at 65 536 must carry the end cell found before
    it through rows without a band, and the final fold must not take the second epoch's empty keys for rows.)  The one case here
    that is not small: ~10 s of oracle."""
    blk = B.epoch_block()
    ref = run(engine, monkeypatch, capfd, [blk], B.DEFAULT, ((0, 1),), {11}, "epochs", arena_retries=True)
    g, sc, _ = ref[0]
    assert len(g.nodes()[0]) > 66000 and int(sc[-1]) == 600
    assert g.n_nodes - len(blk[-1]) > 65536          # (rows in front of the last sweep: it adds at most a node per letter)

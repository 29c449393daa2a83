"""Inputs of tests/test_gpu_band_edges.py and what the ORACLE says about them: the states of the banded sweep
(smoothxg_amd/csrc/poa_band16.hip.h) each input is built to reach, derived from the oracle's graphs alone -- the rows' CSR and
backbone coordinates (Graph.rows(), Graph.row_hints()) after every sequence -- with the band rule (decrees B1, B2 of
oracle/poa_oracle.c) and the kernel's window rule written down here a second time.  tests/test_band_edges_inputs.py asserts
these facts without a GPU; the GPU test compares the kernel with the live oracle on the same inputs.

Nothing here is random at run time: every generator is seeded."""
import numpy as np

WIN = 128                      # strips of the kernel's one-wave window (BAND_WIN)
DEFAULT = (1, -4, -6, -2, -26, -1)            # 2-byte band cells in local mode
CB4 = (1, -19, -39, -3, -81, -1)              # 4-byte band cells by the scores alone (20 code bits)
AFFINE = (1, -4, -6, -2, -6, -2)


def half_width(L):
    return min(311 + int(0.03 * L), 693)


def strip_width(maxlen):
    w = half_width(maxlen)
    return 6 if 2 * w <= 756 else (8 if 2 * w <= 1008 else 11)


def static_band(x, L, W):
    """(first, last strip) of the static band of a row with backbone coordinate x for a sequence of L letters: empty if first > last"""
    w = half_width(L)
    return max(x - w, 0) // W, min((x + w) // W, L // W)


def sweep_facts(rows, hints, L, W):
    """One static-band sweep of a sequence of L letters over a graph (rows = Graph.rows(), hints = Graph.row_hints()), as the
    kernel runs it: per row the band, and the window origin under which the row is swept -- the window re-centres when a
    non-empty band leaves it, origin max(0, first - (128 - width) / 2).  Returns counts:
      recentres     window moves after the first placement
      empty         rows without a band;  cells: the sum of the non-empty bands' columns (min(L, last * W + W - 1) - first * W + 1)
      stored_moved  rows with a STORED predecessor (not the previous row, not the virtual row, its band not empty) that was swept
                    under another window origin
      left_read     rows with such a predecessor whose band begins at the window's origin s0 >= 1 while strip s0 - 1 lies in the
                    predecessor's band: the 2-byte path's separate read of the strip left of the window
      np3           rows with three or more predecessors"""
    _, off, pred, _, _ = rows
    N = len(hints)
    s0 = None
    origin = np.zeros(N + 1, np.int64)
    band = np.zeros((N + 1, 2), np.int64)
    band[0] = (0, -1)
    f = dict(recentres=0, empty=0, cells=0, stored_moved=0, left_read=0, np3=0, rows=N)
    for i in range(1, N + 1):
        bl, bh = static_band(int(hints[i - 1]), L, W)
        band[i] = (bl, bh)
        if bh >= bl:
            f["cells"] += min(L, bh * W + W - 1) - bl * W + 1
            if s0 is None or bl < s0 or bh >= s0 + WIN:
                f["recentres"] += s0 is not None
                s0 = max(0, bl - (WIN - (bh - bl + 1)) // 2)
        else:
            f["empty"] += 1
        origin[i] = -1 if s0 is None else s0
        ps = pred[off[i - 1]:off[i]]
        f["np3"] += len(ps) >= 3
        if bh < bl:
            continue
        stored = [int(p) for p in ps if p >= 1 and p != i - 1 and band[p][1] >= band[p][0]]
        f["stored_moved"] += any(origin[p] != s0 for p in stored)
        f["left_read"] += any(bl == s0 and s0 >= 1 and band[p][0] <= s0 - 1 <= band[p][1] for p in stored)
    return f


def block_facts(O, seqs, scores, banded=1):
    """sweep_facts of every alignment of a block (sequence k against the oracle's graph of the first k), static band"""
    W = strip_width(max(len(s) for s in seqs))
    p = O.mkparams(*scores, mode=0, banded=banded)
    out = []
    for k in range(1, len(seqs)):
        g = O.block_run(seqs[:k], None, p)[0]
        out.append(sweep_facts(g.rows(), g.row_hints(), len(seqs[k]), W))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def with_snps(a, first, every=50, shift=1):
    """a copy of `a` with letter + shift (mod 4) at first, first + every, ..."""
    b = a.copy()
    b[first::every] = (b[first::every] + shift) & 3
    return b


def width_change_block(top, n_seqs=3, seed=0):
    """(a) near-identical sequences, the longest of exactly `top` letters: SNPs every 50 letters, one 40-base deletion"""
    a = _rng(810000 + top + seed).integers(0, 4, top, dtype=np.uint8)
    b = with_snps(a, 17)
    b = np.concatenate([b[:top // 2], b[top // 2 + 40:]])
    return [a, b, with_snps(a, 33, shift=2)][:n_seqs]


def long_first_block():
    """(a) the first sequence sets W = 11 (6 500 letters), the others are 300 - 900 letters from its start, middle and end: their
    band_w comes from their own length, the strip width from the block's"""
    a = _rng(810011).integers(0, 4, 6500, dtype=np.uint8)
    return [a, with_snps(a[:900], 20), with_snps(a[3000:3300], 9), with_snps(a[-600:], 31), with_snps(a[:450], 5, shift=3)]


def last_strip_block(k, W=6):
    """(b) sequences of k W + 1, k W, k W - 1, k W + 1, k W letters: every length is aligned at least once; the shorter ones lose
    letters at the END, where the strip of column L is"""
    a = _rng(820000 + k).integers(0, 4, k * W + 1, dtype=np.uint8)
    snp = lambda s, at: with_snps(s, at, every=37) if len(s) > 40 else s.copy()
    return [a, snp(a[:k * W], 11), snp(a[:k * W - 1], 23), snp(a, 5), with_snps(a[:k * W], k * W - 1, shift=2)]


def tiny_blocks():
    """(b) a one-letter sequence inside a block, a block of one-letter sequences, a block of one sequence of one letter, an empty block"""
    a = _rng(820999).integers(0, 4, 30, dtype=np.uint8)
    one = np.array([int(a[12])], np.uint8)
    return [[a, one, with_snps(a, 7, every=11)], [one, one.copy(), np.array([(int(one[0]) + 1) & 3], np.uint8)], [one], []]


def empty_band_block(at_end):
    """(c) a backbone of 2 000 letters, a sequence of 100 letters taken from its start (at_end: from its END -- nothing inside its
    band matches, it becomes a new chain), then a full-length sequence whose rows read predecessors from both"""
    a = _rng(830000 + at_end).integers(0, 4, 2000, dtype=np.uint8)
    short = with_snps(a[-100:] if at_end else a[:100], 30, every=45)
    third = with_snps(a, 19)
    if at_end:
        third = np.concatenate([short[:60], third[60:]])   # (begins on the short sequence's chain)
    return [a, short, third]


def moving_window_block(ins):
    """(d) W = 6, the longest sequence 2 266 letters, and it is the LAST: its band fills the window while the graph holds every
    other sequence's nodes.  All but the backbone have SNPs every 50 letters, and three of them differ from the backbone and
    from each other at column 500 (four sibling nodes: the next row has four predecessors).
    ins = 300: [backbone, - 40 letters, + 40 letters, - 300 letters, + 300 letters]: 300 is inside w = 378, both bands keep it.
    ins = 420: the backbone carries 420 letters at column 804 that the second, third and fourth sequence lack (the second lacks
    40 more, the third has 40 of its own): behind them these run 420 columns off the backbone coordinates, where the static band
    loses the alignment and the adaptive band, which follows the best cells, does not; the last sequence is the backbone with
    SNPs."""
    r = _rng(840000 + ins)
    core = r.integers(0, 4, 2266 - ins, dtype=np.uint8)
    b, c, e = with_snps(core, 13), with_snps(core, 27, shift=2), with_snps(core, 41, shift=3)
    for k, s in enumerate((b, c, e)):
        s[500] = (core[500] + 1 + k) & 3
    b = np.concatenate([b[:600], b[640:]])
    c = np.concatenate([c[:402], r.integers(0, 4, 40, dtype=np.uint8), c[402:]])
    payload = r.integers(0, 4, ins, dtype=np.uint8)
    if ins == 300:
        e = np.concatenate([e[:1300], e[1600:]])
        return [core, b, c, e, np.concatenate([with_snps(core, 7)[:804], payload, with_snps(core, 7)[804:]])]
    a = np.concatenate([core[:804], payload, core[804:]])
    return [a, b, c, e, with_snps(a, 7)]


# ---------------------------------------------------------------------------------------------------------------------------
# what the inputs must reach, asserted on the oracle alone (an input that misses a bar is changed, never the bar)

def check_empty_bands(O, seqs):
    """(c) more than half of the short sequence's rows have no band; its cells are the sum of the non-empty bands"""
    facts = block_facts(O, seqs, DEFAULT)
    cells = O.block_run(seqs, None, O.mkparams(*DEFAULT, mode=0, banded=1))[2]
    assert facts[0]["empty"] > facts[0]["rows"] // 2 and facts[0]["rows"] == len(seqs[0]), facts[0]
    assert [int(x) for x in cells[1:]] == [f["cells"] for f in facts], (cells, facts)
    assert facts[1]["empty"] == 0 and facts[1]["recentres"] >= 10, facts[1]
    return facts


def check_moving_window(O, seqs):
    """(d) the bars of a full window that moves, on the sweep of the last sequence"""
    assert strip_width(max(len(s) for s in seqs)) == 6 and max(len(s) for s in seqs) == 2266 == len(seqs[-1])
    facts = block_facts(O, seqs, DEFAULT)
    last = facts[-1]
    assert last["recentres"] >= 10 and last["stored_moved"] >= 1 and last["left_read"] >= 1 and last["np3"] >= 1, last
    assert all(f["recentres"] >= 10 for f in facts), facts
    return facts


def check_ties(O, banded):
    """(e) the two windows score the same alone and together, and the oracle's alignment takes the FIRST row's (decree S4)"""
    p = O.mkparams(*DEFAULT, mode=0, banded=banded)
    a, q, q1, q2 = tie_far_block()
    assert [int(O.block_run([a, x], None, p)[1][1]) for x in (q, q1, q2)] == [60, 60, 60]
    g = O.block_run([a, q], None, p)[0]
    assert (g.seq_path(1)[900:960] == g.seq_path(0)[900:960]).all() and not (g.seq_path(1)[1500:1560] == g.seq_path(0)[1500:1560]).any()
    # ... on either side of a window re-centre: the band of the 2 266-letter query is 127 - 128 strips, the window moves between
    assert sweep_facts(O.block_run([a], None, p)[0].rows(), np.arange(1, len(a) + 1), len(q), 6)["recentres"] >= 10
    both, no_first, no_second = tie_same_strip_block()
    assert [int(O.block_run(x, None, p)[1][1]) for x in (both, no_first, no_second)] == [40, 40, 40]
    g = O.block_run(both, None, p)[0]
    assert (g.seq_path(1)[310:350] == g.seq_path(0)[200:240]).all()
    assert (len(both[0]) + 1 + 5) // 6 <= WIN      # (one window holds every strip: the keys of both rows meet in one lane)


def tie_far_block():
    """(e) [backbone, query, the query with its first window only, with its second only]: the query equals the 2 266-letter backbone
    in columns 900 .. 959 and 1 500 .. 1 559 and differs from it everywhere else -- two end cells of score 60 in different strips,
    a hundred window re-centres apart"""
    a = _rng(850001).integers(0, 4, 2266, dtype=np.uint8)
    junk = (a + 1 + np.arange(len(a)) % 3).astype(np.uint8) & 3
    q, q1, q2 = junk.copy(), junk.copy(), junk.copy()
    for lo in (900, 1500):
        q[lo:lo + 60] = a[lo:lo + 60]
    q1[900:960] = a[900:960]
    q2[1500:1560] = a[1500:1560]
    return [a, q, q1, q2]


def tie_same_strip_block():
    """(e) [backbone, query, backbone without its first copy, without its second]: the 700-letter backbone holds the same 40 letters
    at 200 and at 420, the query holds them at column 310 and otherwise a letter that differs from the backbone's at the same
    column and 110 to either side: two end cells of score 40 in ONE column, rows 220 apart, the window never moves (700 letters
    are 117 strips)"""
    r = _rng(850002)
    a = r.integers(0, 4, 700, dtype=np.uint8)
    s = r.integers(0, 4, 40, dtype=np.uint8)
    a[200:240] = s
    a[420:460] = s
    q = np.empty(700, np.uint8)
    for j in range(700):
        bad = {int(a[j]), int(a[min(j + 110, 699)]), int(a[max(j - 110, 0)])}
        q[j] = min(x for x in range(4) if x not in bad) if len(bad) < 4 else (int(a[j]) + 1) & 3
    q[310:350] = s
    a1, a2 = a.copy(), a.copy()
    a1[200:240] = (s + 1) & 3
    a2[420:460] = (s + 2) & 3
    return [a, q], [a1, q], [a2, q]


def epoch_block(n_long=4):
    """(f) unrelated sequences of ~18 kbp until the graph passes 65 536 rows, then a last sequence of 1 200 letters: 600 of the
    LAST long sequence's start, whose rows come late in the graph, then 600 of the first one's"""
    r = _rng(865536)
    seqs = [r.integers(0, 4, n, dtype=np.uint8) for n in (18000, 17900, 17800, 17700, 17600)[:n_long]]
    return seqs + [np.concatenate([seqs[-1][40:640], seqs[0][700:1300]])]

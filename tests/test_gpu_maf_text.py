"""GPU: the MAF text of the resident trimmed rows (want_msa = SXG_MSA_TRIMMED_RESIDENT, sxg_poa_msa_row_letters, sxg_poa_maf_text:
maf_text_kernel + msa_row_letters_kernel of poa_maf_text.hip.h) against numpy on the rows the same batch downloads with
SXG_MSA_TRIMMED -- the hand-sized blocks of tests/test_gpu_msa_rows.py in ONE batch -- and the MAF iteration that uses it
(Smoother.smooth_maf_gfa(..., device_text=gpu_maf_texter(engine))) against device_rows=True and the legacy call on the same engine."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import smooth_oracle as SO
import smoothxg_amd as S
from smoothxg_amd import poa as P
from smoothxg_amd import smooth as SM

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_msa_rows import drb1_discovered, flat, make_batch  # noqa: E402
from test_maf_device_rows_host import HEADER, last_path_first  # noqa: E402
from test_smooth_host import inversion_gfa, synthetic_gfa  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALID = -1
COMP = np.full(256, ord("N"), np.uint8)   # revcomp_gapped's table
for _a, _b in ("AT", "TA", "CG", "GC", "--"):
    COMP[ord(_a)] = ord(_b)


@pytest.fixture(scope="module")
def batch(engine):
    return make_batch(engine.msa_geometry()[1])


def run(engine, batch, msa, cons=True):
    bases, seq_off, blk_off, params, trims = flat(batch)
    res = engine.run_flat(bases, seq_off, blk_off, None, params, want_consensus=cons, want_msa=msa, check=False, block_graph=3, bg_trim=trims)
    return res, engine.msa_layout


@pytest.fixture(scope="module")
def ref(engine, batch):
    """The batch with SXG_MSA_TRIMMED, computed once: (results, (msa_off, msa_cols), the rows in global row order as uint8 arrays,
    the first global row of every block)."""
    res, layout = run(engine, batch, P.MSA_TRIMMED)
    rows, first = [], []
    for b, (name, seqs, trim, mode, banded) in enumerate(batch):
        first.append(len(rows))
        if res[b].status == 0 and seqs:
            assert len(res[b].msa) == len(seqs) + 1, name
            rows += [np.frombuffer(r.encode(), np.uint8) for r in res[b].msa]
    return res, layout, rows, first


@pytest.fixture()
def resident(engine, batch):
    """The batch with SXG_MSA_TRIMMED_RESIDENT, executed anew for every test that needs the rows on the handle."""
    return run(engine, batch, P.MSA_TRIMMED_RESIDENT)


def same_block(a, z):
    assert a.status == z.status and (a.scores == z.scores).all() and (a.cells == z.cells).all()
    assert a.paths is None and z.paths is None and a.node_code is None and z.node_code is None and a.consensus is None and z.consensus is None
    assert (a.bg is None) == (z.bg is None)
    if a.bg is not None:
        assert a.bg.node_seq == z.bg.node_seq and a.bg.edges == z.bg.edges and (a.bg.node_indeg == z.bg.node_indeg).all()
        assert len(a.bg.paths) == len(z.bg.paths) and all((x == y).all() for x, y in zip(a.bg.paths, z.bg.paths))
        assert (a.bg.consensus == z.bg.consensus).all()


def test_the_download_leaves_the_rows_behind(engine, batch, ref, resident):
    res, layout, rows, first = ref
    got, got_layout = resident
    assert all(r.msa is None or all(x == "" for x in r.msa) for r in got)            # msa == NULL: no row came down
    assert any(r.msa for r in res)
    assert (got_layout[0] == layout[0]).all() and (got_layout[1] == layout[1]).all()   # msa_off, msa_cols
    assert got_layout[0][-1] == sum(len(r) for r in rows) > 0
    for a, z in zip(got, res):
        same_block(a, z)
    letters = engine.msa_row_letters()
    assert len(letters) == len(rows)
    assert (letters == np.asarray([int((r != ord("-")).sum()) for r in rows], np.int32)).all()
    assert engine.msa_stats()[2] == layout[0][-1]


def expected(segs, literal, rows):
    lit = np.frombuffer(literal, np.uint8)
    parts = [lit[s:s + n] if k == 0 else rows[s] if k == 1 else COMP[rows[s][::-1]] for s, n, k in segs]
    return np.concatenate(parts).tobytes() if parts else b""


def check_text(engine, segs, literal, rows):
    """maf_text into a buffer between guard bytes, against numpy"""
    want = expected(segs, literal, rows)
    buf = np.full(len(want) + 128, 0xA5, np.uint8)
    before = engine.maf_text_stats()[1]
    engine.maf_text(segs, literal, out=buf[64:64 + len(want)])
    assert buf[64:64 + len(want)].tobytes() == want
    assert (buf[:64] == 0xA5).all() and (buf[64 + len(want):] == 0xA5).all()
    assert engine.maf_text_stats()[1] - before == len(want)
    return len(want)


def test_segment_lists_against_numpy(engine, batch, ref, resident):
    res, layout, rows, first = ref
    rng = np.random.default_rng(7)
    literal = bytes(rng.integers(33, 127, 400, dtype=np.uint8))
    lits = (0, 1, 15, 16, 17, 33)
    widths = {len(r) for r in rows}
    assert {0, 1, 15, 16, 17, 255, 257} <= widths
    # (i) every row forward, literals of 0, 1, 15, 16, 17 and 33 bytes between them
    segs, at = [], 0
    for r in range(len(rows)):
        n = lits[r % len(lits)]
        segs += [(at, n, 0), (r, len(rows[r]), 1)]
        at = (at + n) % 300
    check_text(engine, segs, literal, rows)
    # (ii) every row reversed and complemented
    check_text(engine, [(r, len(rows[r]), 2) for r in range(len(rows))], literal, rows)
    # (iii) kinds mixed, one row used three times, the rows of a block without columns
    zero = [r for r in range(len(rows)) if len(rows[r]) == 0]
    wide = max(range(len(rows)), key=lambda r: len(rows[r]))
    segs = [(0, 3, 0), (wide, len(rows[wide]), 1), (wide, len(rows[wide]), 2), (5, 0, 0), (wide, len(rows[wide]), 1)]
    segs += [(z, 0, 1 + z % 2) for z in zero] + [(7, 40, 0)]
    for r in range(0, len(rows), 3):
        segs += [(r, len(rows[r]), 1 + (r // 3) % 2), (r % 50, r % 7, 0)]
    check_text(engine, segs, literal, rows)
    # the empty list
    assert engine.maf_text([], b"") == b""


@pytest.mark.parametrize("residue", [1, 15, 0])
def test_more_than_two_chunks_and_every_alignment(engine, batch, ref, resident, residue):
    """(iv) the rows of the block one byte wider than the rows kernel's window, repeated until the text passes two chunks; the
    literals in front of them make the rows start on every destination alignment; the total is `residue` modulo 16."""
    res, layout, rows, first = ref
    tile = engine.msa_geometry()[1]
    chunk = engine.maf_text_geometry()
    mine = [r for r in range(len(rows)) if len(rows[r]) == tile + 1]
    assert len(mine) >= 3
    literal = bytes(np.random.default_rng(residue).integers(33, 127, 64, dtype=np.uint8))
    segs, total, k, starts = [], 0, 0, set()
    while total <= 2 * chunk + 100 or len(starts) < 16:
        pre = (k % 16 - total) % 16 or (16 if k % 5 == 0 else 0)      # the row starts at k modulo 16
        r = mine[k % 3]
        segs += [(k % 7, pre, 0), (r, len(rows[r]), 1 + k % 2)]
        total += pre
        starts.add(total % 16)
        total += len(rows[r])
        k += 1
    tail = (residue - total) % 16
    segs.append((1, tail, 0))
    assert (total + tail) % 16 == residue and starts == set(range(16))
    assert check_text(engine, segs, literal, rows) > 2 * chunk


def invalid(engine, segs, literal=b"", out_bytes=None):
    """the raw call: (return code, whether `out` was left alone)"""
    sa = np.array([tuple(x) for x in segs], P.MAF_SEG_DTYPE).reshape(-1)
    lit = np.frombuffer(literal, np.uint8)
    n = int(sa["len"].astype(np.int64).clip(0).sum()) if out_bytes is None else out_bytes
    buf = np.full(max(n, 0) + 64, 0x5A, np.uint8)
    ti = P.MafTextIn(len(sa), C.cast(sa.ctypes.data, C.POINTER(P.MafSeg)), lit.ctypes.data_as(C.POINTER(C.c_uint8)) if len(lit) else None, len(lit))
    rc = engine.lib.sxg_poa_maf_text(engine.h, C.byref(ti), buf.ctypes.data, n)
    return rc, bool((buf == 0x5A).all())


def test_bad_calls_are_refused_before_anything_runs(engine, batch, ref, resident):
    res, layout, rows, first = ref
    n = len(rows)
    w0 = len(rows[0])
    lit = b"0123456789"
    assert invalid(engine, [(0, w0, 1), (0, 10, 0)], lit) == (0, False)          # the good call, for contrast
    for what, segs, kw in (("len != msa_cols", [(0, w0 + 1, 1)], {}), ("len != msa_cols, shorter", [(0, w0 - 1, 2)], {}),
                           ("row -1", [(-1, w0, 1)], {}), ("row n", [(n, w0, 1)], {}), ("row n, kind 2", [(n, 0, 2)], {}),
                           ("a literal past the blob", [(0, w0, 1), (5, 6, 0)], {}), ("a literal that starts past the blob", [(11, 0, 0)], {}),
                           ("a negative literal offset", [(-1, 2, 0)], {}), ("a negative length", [(0, -1, 0)], {}),
                           ("out_bytes too small", [(0, w0, 1)], dict(out_bytes=w0 - 1)), ("out_bytes too large", [(0, w0, 1)], dict(out_bytes=w0 + 1)),
                           ("kind 3", [(0, w0, 3)], {}), ("kind -1", [(0, w0, -1)], {})):
        assert invalid(engine, [(0, 4, 0)] + segs, lit, **kw) == (E_INVALID, True), what
    with pytest.raises(P.PoaError, match="maf_text"):
        engine.maf_text([(0, w0, 3)], lit)
    # after a further upload the rows are gone
    bases, seq_off, blk_off, params, trims = flat(batch[:3])
    engine.upload(bases, seq_off, blk_off, None, params, want_consensus=True, want_msa=P.MSA_TRIMMED_RESIDENT, block_graph=3, bg_trim=trims)
    assert invalid(engine, [(0, w0, 1)]) == (E_INVALID, True)
    with pytest.raises(P.PoaError, match="resident"):
        engine.msa_row_letters()
    engine.execute()
    assert invalid(engine, [(0, w0, 1)]) == (0, False)
    # after batches that built no trimmed rows
    for msa in (0, P.MSA_FULL):
        engine.run_flat(bases, seq_off, blk_off, None, params, want_consensus=True, want_msa=msa, block_graph=1, bg_trim=trims)
        assert invalid(engine, [(0, w0, 1)]) == (E_INVALID, True)
        assert invalid(engine, [(0, 4, 0)], lit) == (E_INVALID, True)


def test_a_fresh_handle_has_no_rows():
    eng = S.PoaEngine(0)
    try:
        assert invalid(eng, [(0, 4, 0)], b"0123") == (E_INVALID, True)
        with pytest.raises(P.PoaError, match="resident"):
            eng.msa_row_letters()
    finally:
        eng.close()


def test_the_text_of_a_plain_trimmed_batch(engine, batch, ref):
    """maf_text and msa_row_letters also work on the rows a SXG_MSA_TRIMMED batch leaves on the handle, and that batch's download
    is what it was."""
    res, layout, rows, first = ref
    again, again_layout = run(engine, batch, P.MSA_TRIMMED)
    assert [r.msa for r in again] == [r.msa for r in res] and (again_layout[0] == layout[0]).all()
    check_text(engine, [(r, len(rows[r]), 1 + r % 2) for r in range(len(rows))], b"", rows)
    assert (engine.msa_row_letters() == np.asarray([int((r != ord("-")).sum()) for r in rows], np.int32)).all()


def test_a_group_and_the_sharded_entry_refuse_resident_rows(engine, batch):
    bases, seq_off, blk_off, params, trims = flat(batch[:3])
    for ranks in (0, 2):
        with pytest.raises(P.PoaError, match="SXG_MSA_TRIMMED"):
            engine.run_flat_sharded(bases, seq_off, blk_off, None, params, want_msa=P.MSA_TRIMMED_RESIDENT, simulate_ranks=ranks, block_graph=3, bg_trim=trims)
    group = P.PoaGroup([0, 0])
    try:
        with pytest.raises(P.PoaError, match="SXG_MSA_TRIMMED_RESIDENT"):
            group.run_flat(bases, seq_off, blk_off, None, params, want_msa=P.MSA_TRIMMED_RESIDENT, block_graph=3, bg_trim=trims)
        assert group.run_flat(bases, seq_off, blk_off, None, params, want_msa=P.MSA_TRIMMED, block_graph=3, bg_trim=trims)[1].msa
        with pytest.raises(ValueError):
            SM.gpu_maf_texter(group)
    finally:
        group.close()


# ---- end to end: the MAF iteration over device text
def iteration_case(engine, text, sm, pkw, identity=False):
    g = SO.Graph(text)
    p = SM.default_params(**pkw)
    kw = dict(identity=SM.gpu_range_identifier(engine)) if identity else {}
    before = engine.maf_text_stats()[1]
    new = sm.smooth_maf_gfa(p, SM.gpu_provider(engine), header=HEADER, device_text=SM.gpu_maf_texter(engine), **kw)
    assert engine.maf_text_stats()[1] - before == len(new[1].encode())
    rows = sm.smooth_maf_gfa(p, SM.gpu_provider(engine), header=HEADER, device_rows=True, **kw)
    old = sm.smooth_maf_gfa(p, SM.gpu_provider(engine), header=HEADER, **kw)
    assert new[1] == rows[1] == old[1], "MAF"
    assert new[0] == rows[0] == old[0], "GFA"
    assert new[2] == rows[2] == old[2] == 0
    out = SO.Graph(new[0])
    for q, nm in enumerate(g.pname):          # every input path is spelt by the output (the invariants of conftest.py ran as well)
        assert out.path_sequence(out.pname.index(nm)) == g.path_sequence(q)
    return new


@pytest.mark.parametrize("chunks", [1, 3])
def test_iteration_with_groomed_blocks(engine, monkeypatch, chunks):
    text = last_path_first(synthetic_gfa(0))
    sm = SM.Smoother(text, 90)
    if chunks > 1:
        monkeypatch.setenv("SXG_SMOOTH_CHUNK_BLOCKS", str(max(1, sm.n_blocks // chunks)))
    iteration_case(engine, text, sm, dict(add_consensus=1))
    sm.close()


@pytest.mark.parametrize("adaptive", [0, 1])
def test_iteration_with_a_block_collected_in_reverse(engine, adaptive):
    text = inversion_gfa(3, length=2400, lo=800, hi=1600)
    sm = SM.Smoother(text, 800)
    iteration_case(engine, text, sm, dict(add_consensus=1, adaptive_poa_params=adaptive), identity=bool(adaptive))
    sm.close()


def test_iteration_on_drb1_discovered_blocks(engine):
    """2161 blocks, most of one sequence; 8 have a consensus row of fewer than 2 * 311 letters, which is all gaps."""
    text, g, blocks, sm = drb1_discovered()
    new = iteration_case(engine, text, sm, dict(add_consensus=1))
    assert new[1].count("\na ") + new[1].startswith("a ") >= 2000
    sm.close()

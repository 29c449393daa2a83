"""The 32-bit sweep in column tiles (smoothxg_amd/csrc/poa_tiles.h, dp_fill in poa_dp.hip.h), switched on per engine with
set_long_blocks(True): every block is compared bit for bit with the live oracle through assert_block_equal.

Small tiles are forced with SXG_POA_TILE_COLS=512 (honoured with the switch on only) on SXG_POA_NO_PACKED=1, so that two to five
tiles are reached at 510 .. 2 100 letters: lengths whose L + 1 columns end on, just below and just above a tile edge; local and
global; the convex default, an affine and a linear score set; int16 and int32 row words (the latter reached the way
test_gpu_class_matrix.py reaches them: through a score set whose m * L leaves int16 -- here a convex, an affine and a linear set
with m = 64, as large as the one-byte scores of sxg_poa_params allow next to their penalties).  Then what crosses an edge
(insertions in the query across column 512, a deletion between columns 511 and 512, a bubble at columns 510 - 514), the end cell
of a local alignment whose equal maxima lie in different tiles, the real tile width (two sequences of 14 600 letters, global:
status 5 with the switch off, as today), the data-dependent case (two independent sequences of 13 000 letters, global) and a
device group.

2 100 letters (five tiles) is beyond the lengths the issue lists: it is the shortest case in which a boundary buffer that was
read is written again and read again (tile 2 rewrites the buffer tile 1 read, tile 3 reads it)."""
import numpy as np
import pytest

from helpers import PARAM_SETS, assert_block_equal, assert_same, random_block
from oracle import oracle_py as O
from smoothxg_amd import Params

pytestmark = pytest.mark.gpu

TILE = 512
SETS = ("convex_default", "affine_4param", "linear")
LENGTHS = (510, 511, 512, 1023, 1024, 1300, 2100)


# m = 64: m * L >= 30 000 from 469 letters on, so every length here runs int32 row words (convex: q < g < e < c)
WIDE_SETS = {"convex_default": (64, -127, -96, -32, -127, -16), "affine_4param": (64, -127, -96, -32, -96, -32), "linear": (64, -96, -80, -80, -80, -80)}


def scores_of(name, wide):
    return WIDE_SETS[name] if wide else PARAM_SETS[name]


def block_of(rng, n, length, div):
    """n related sequences, the longest of exactly `length` letters"""
    seqs = [s[:length] for s in random_block(rng, n, length, div)]
    if len(seqs[0]) < length:
        seqs[0] = np.concatenate([seqs[0], rng.integers(0, 4, length - len(seqs[0])).astype(np.uint8)])
    assert max(len(s) for s in seqs) == length == len(seqs[0])
    return seqs


@pytest.fixture
def tiled(engine, monkeypatch):
    """the session's engine with the switch on and small tiles forced; the switch is off again afterwards"""
    monkeypatch.setenv("SXG_POA_NO_PACKED", "1")
    monkeypatch.setenv("SXG_POA_TILE_COLS", str(TILE))
    engine.set_long_blocks(True)
    yield engine
    engine.set_long_blocks(False)


@pytest.fixture
def long_engine(engine):
    """the session's engine with the switch on and no other knob"""
    engine.set_long_blocks(True)
    yield engine
    engine.set_long_blocks(False)


def run_against_oracle(eng, blocks, scores, mode, label):
    """blocks[k] with scores[k] (six numbers): one batch on the engine, every block against the oracle"""
    res = eng.run_blocks(blocks, [Params(*s, mode, 0) for s in scores])
    for k, (seqs, s) in enumerate(zip(blocks, scores)):
        g, sc, cells = O.block_run(seqs, None, O.mkparams(*s, mode=mode))
        assert_block_equal(res[k], g, sc, cells, label="%s[%d] L=%d %r" % (label, k, len(seqs[0]), s))
    return res


@pytest.mark.parametrize("wide", [False, True], ids=["int16-words", "int32-words"])
@pytest.mark.parametrize("mode", [0, 1], ids=["local", "global"])
def test_forced_small_tiles(tiled, mode, wide):
    rng = np.random.default_rng(5120 + 2 * mode + int(wide))
    blocks, scores = [], []
    for k, L in enumerate(LENGTHS):
        for j, name in enumerate(SETS):
            blocks.append(block_of(rng, 4 + (k + j) % 5, L, 0.02 + 0.01 * ((k + 2 * j) % 4)))
            scores.append(scores_of(name, wide))
    run_against_oracle(tiled, blocks, scores, mode, "tiles")
    st, ts = tiled.stats(), tiled.tile_stats()
    print(st["dom_row_mode"], st["dp_launches"], st["retries"], ts)
    assert st["dom_row_mode"] == (1 if wide else 0)
    # 510 and 511 letters fill one tile (a launch of one tile is no tiled launch); the others are tiled, every sweep of their
    # longest sequence over more than one tile
    n_tiled = sum(1 for b in blocks if len(b[0]) + 1 > TILE)
    assert ts["blocks"] == n_tiled and ts["sweeps"] == sum(len(b) - 1 for b in blocks if len(b[0]) + 1 > TILE)
    assert ts["tiles"] > ts["sweeps"]
    want_tiles = sum(-(-(len(s) + 1) // TILE) for b in blocks if len(b[0]) + 1 > TILE for s in b[1:])
    assert ts["tiles"] == want_tiles


@pytest.mark.parametrize("mode", [0, 1], ids=["local", "global"])
def test_what_crosses_a_tile_edge(tiled, mode):
    rng = np.random.default_rng(5121 + mode)
    base = rng.integers(0, 4, 1000).astype(np.uint8)

    def noisy(s):   # a third sequence: the second one with a few substitutions, so that later rows have several predecessors
        s = s.copy()
        for p in rng.integers(0, len(s), 12):
            s[p] = (s[p] + 1) % 4
        return s

    def ins(start_col, n):   # n letters inserted into the query, the first of them at column start_col
        return np.concatenate([base[:start_col - 1], rng.integers(0, 4, n).astype(np.uint8), base[start_col - 1:]])

    ins40, ins3 = ins(TILE - 20, 40), ins(TILE - 2, 3)      # E and Q carried across column 512
    dele = np.concatenate([base[:TILE - 1], base[TILE - 1 + 30:]])   # columns 511 and 512 are neighbours of a 30-letter deletion
    snp = base.copy()
    snp[TILE - 3:TILE + 2] = (snp[TILE - 3:TILE + 2] + 2) % 4        # columns 510 .. 514
    bubble = [base, snp, base.copy(), snp.copy(), base.copy(), snp.copy(), base.copy(), snp.copy()]
    blocks, scores = [], []
    for name in ("convex_default", "affine_4param"):
        for blk in ([base, ins40, noisy(ins40)], [base, ins3, noisy(ins3)], [base, dele, noisy(dele)], [ins40, base, noisy(base)], bubble):
            blocks.append(blk)
            scores.append(PARAM_SETS[name])
    run_against_oracle(tiled, blocks, scores, mode, "edge")
    ts = tiled.tile_stats()
    assert ts["blocks"] == len(blocks) and ts["tiles"] > ts["sweeps"]


def test_end_cell_is_merged_by_row_then_column_not_by_tile(tiled):
    """Two maxima of equal H in different tiles: S4 takes the smaller row, whichever tile holds it."""
    rng = np.random.default_rng(5123)
    U, V, X = (rng.integers(0, 4, n).astype(np.uint8) for n in (400, 400, 500))
    s = PARAM_SETS["convex_default"]
    # graph U+V, query V+U: H = 400 at (row 800, column 400), tile 0, and at (row 400, column 800), tile 1 -- the later tile wins
    later = [np.concatenate([U, V]), np.concatenate([V, U])]
    # mirrored -- graph U+V, query U, a 500-letter spacer, V: H = 400 at (row 400, column 400), tile 0, and at (row 800, column
    # 1 300), tile 2 (joining the two through the spacer costs 525: 275 in all) -- the earlier tile keeps it
    earlier = [np.concatenate([U, V]), np.concatenate([U, X, V])]
    res = run_against_oracle(tiled, [later, earlier], [s, s], 0, "end cell")
    assert [int(r.scores[1]) for r in res] == [400, 400]
    # (the query's aligned letters: V+U's second half, columns 401 .. 800; U+X+V's first 400)
    assert (np.asarray(res[0].paths[1][:400]) != np.asarray(res[0].paths[0][400:800])).any()
    assert (np.asarray(res[0].paths[1][400:]) == np.asarray(res[0].paths[0][:400])).all()
    assert (np.asarray(res[1].paths[1][:400]) == np.asarray(res[1].paths[0][:400])).all()


@pytest.fixture(scope="module")
def real_width_case():
    """two sequences of 14 600 letters at 2 % divergence, global, convex default: ~2e8 cells, 32-bit, two tiles of 12 288 columns"""
    rng = np.random.default_rng(14600)
    seqs = block_of(rng, 2, 14600, 0.02)
    g, sc, cells = O.block_run(seqs, None, O.mkparams(*PARAM_SETS["convex_default"], mode=1))
    return seqs, g, sc, cells


def test_real_tile_width(engine, real_width_case):
    seqs, g, sc, cells = real_width_case
    par = Params(*PARAM_SETS["convex_default"], 1, 0)
    off = engine.run_blocks([seqs], par, check=False)
    assert off[0].status == 5   # the switch is off: today's answer
    assert engine.tile_stats() == {"blocks": 0, "sweeps": 0, "tiles": 0}
    engine.set_long_blocks(True)
    try:
        on = engine.run_blocks([seqs], par)
        st, ts = engine.stats(), engine.tile_stats()
    finally:
        engine.set_long_blocks(False)
    assert_block_equal(on[0], g, sc, cells, label="14600 global")
    assert (st["dom_threads"], st["dom_cols_per_lane"]) == (1024, 12) and st["dom_row_mode"] in (0, 1)
    assert ts == {"blocks": 1, "sweeps": 1, "tiles": 2}
    assert engine.run_blocks([seqs], par, check=False)[0].status == 5   # ... and off again


def test_data_dependent_global_block_completes(long_engine):
    """Two independent sequences of 13 000 letters, global: the packed sweep takes them (m L + m < 14 500) and its walk may meet a
    clamped cell, which sends the block to a 32-bit sweep that no single geometry covers.  With the switch on it completes
    whatever route the ladder took."""
    rng = np.random.default_rng(13000)
    seqs = [rng.integers(0, 4, 13000).astype(np.uint8) for _ in range(2)]
    s = PARAM_SETS["convex_default"]
    run_against_oracle(long_engine, [seqs], [s], 1, "independent 13000")
    print(long_engine.stats()["retries"], long_engine.tile_stats())


def test_local_block_beyond_the_packed_geometries(engine):
    """Local, default scores, a sequence of 27 000 letters: m L < 30 000, so the scores are the packed sweep's, whose widest geometry
    ends at 26 623 letters -- status 5 with the switch off.  With it on the block takes the 32-bit sweep in three tiles of 12 288
    columns and equals the oracle.  (The graph is founded by a 2 000-letter sequence and the long one holds a diverged copy of it
    across column 12 288, so the oracle sweeps 2 000 x 27 000 cells, not 27 000 squared; a third, short sequence is then aligned
    to the graph of ~29 000 nodes in one tile of the same launch.)"""
    rng = np.random.default_rng(27000)
    short, copy, third = random_block(rng, 3, 2000, 0.04)
    long_ = rng.integers(0, 4, 27000).astype(np.uint8)
    at = 12288 - len(copy) // 2
    long_[at:at + len(copy)] = copy
    seqs = [short, long_, third[:1500]]
    s = PARAM_SETS["convex_default"]
    par = Params(*s, 0, 0)
    assert engine.run_blocks([seqs], par, check=False)[0].status == 5
    engine.set_long_blocks(True)
    try:
        res = engine.run_blocks([seqs], par)
        st, ts = engine.stats(), engine.tile_stats()
    finally:
        engine.set_long_blocks(False)
    g, sc, cells = O.block_run(seqs, None, O.mkparams(*s, mode=0))
    assert_block_equal(res[0], g, sc, cells, label="local 27000")
    assert int(sc[1]) > 500   # (the copy was found: the alignment crosses the edge between tiles 0 and 1)
    assert st["dom_row_mode"] == 0 and (st["dom_threads"], st["dom_cols_per_lane"]) == (1024, 12)
    assert ts == {"blocks": 1, "sweeps": 2, "tiles": 4}


def test_group_runs_tiled_blocks(engine, real_width_case):
    import smoothxg_amd as S
    seqs, g, sc, cells = real_width_case
    par = Params(*PARAM_SETS["convex_default"], 1, 0)
    engine.set_long_blocks(True)
    try:
        want = engine.run_blocks([seqs], par)
    finally:
        engine.set_long_blocks(False)
    grp = S.PoaGroup([0, 0])
    try:
        assert grp.run_blocks([seqs], par, check=False)[0].status == 5
        grp.set_long_blocks(True)
        got = grp.run_blocks([seqs], par)
        assert grp.tile_stats() == {"blocks": 1, "sweeps": 1, "tiles": 2}
    finally:
        grp.close()
    assert_block_equal(got[0], g, sc, cells, label="group 14600 global")
    assert_same(got, want, "group against one engine")

"""GPU: the identity estimate of the adaptive scores on the device (sxg_poa_block_identity_batch, decree Q of DESIGN.md section
9) against the exact restatement in tests/identity_ref.py.  n_used and status must be equal; the returned pair must have the
Jaccard index of the ref's pair, compared by cross-multiplication: there is no tolerance anywhere."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_ref as IR  # noqa: E402
import split_ref as R  # noqa: E402
import split_synth as Y  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402
from test_identity_host import smooth_gfa_with  # noqa: E402
from test_smooth_host import DRB1, haplotype_gfa  # noqa: E402

pytestmark = pytest.mark.gpu
MIN_LEN = 100            # one min_len for every k, so that the same sequences take part at k = 5, 17 and 32
KS = (17, 32, 5)


def family(rng, n, length, muts):
    anc = rng.integers(0, 4, length).astype(np.uint8)
    return [anc] + [Y.mutate(rng, anc, muts * (1 + q % 4)) for q in range(n - 1)]


@functools.lru_cache(maxsize=None)
def batch():
    """ONE batch of small blocks with every case in which the kernels can go wrong (the comments name them)."""
    rng = np.random.default_rng(2026)
    short = lambda: rng.integers(0, 4, 60).astype(np.uint8)             # below min_len
    a = rng.integers(0, 4, 150).astype(np.uint8)
    n_run = rng.integers(0, 4, 1100).astype(np.uint8)
    n_run[400:470] = 4                                                    # a run of N
    big = family(rng, 2, 2500, 40)                                        # sets several times the sort tile
    mid = family(rng, 2, 1100, 15)                                        # just above the tile (1100 - k + 1 windows)
    three = family(rng, 3, 150, 3)
    blocks = [
        [short(), short()],                                               # n_used 0
        [rng.integers(0, 4, 150).astype(np.uint8), short()],              # n_used 1
        family(rng, 2, 150, 4),                                           # n_used 2: P = 1
        [three[0], short(), three[1], three[2]],                          # n_used 3: idx = 0, a short sequence in the middle
        family(rng, 12, 150, 2),                                          # n_used 12: P = 66
        family(rng, 40, 150, 1),                                          # n_used 40: P = 780
        [big[0], mid[0], a, n_run, big[1], mid[1], Y.mutate(rng, n_run, 10), np.full(150, 4, np.uint8), np.full(160, 4, np.uint8)],
        [a, a.copy(), R.revcomp(a), rng.integers(0, 4, 150).astype(np.uint8)],   # identical, reverse complement (J = 1), unrelated (J = 0)
        [],                                                               # an empty block
        [np.full(150, 4, np.uint8), np.full(101, 4, np.uint8)],           # two empty sets: uni = 0
        [big[0], R.revcomp(big[0])],                                      # P = 1 at J = 1: the largest key there is
        [mid[0], mid[1], mid[0][:100]],                                   # a sequence of exactly min_len
    ]
    return blocks


@functools.lru_cache(maxsize=None)
def want(k):
    return IR.identify_blocks(batch(), k, MIN_LEN)


def check(got, ref):
    used, inter, uni, status = got
    assert [(int(u), int(s)) for u, s in zip(used, status)] == [(r[0], r[3]) for r in ref]
    for b, r in enumerate(ref):
        assert int(inter[b]) * r[2] == r[1] * int(uni[b]), (b, int(inter[b]), int(uni[b]), r)
        assert (int(uni[b]) == 0) == (r[2] == 0) and 0 <= int(inter[b]) <= int(uni[b]), (b, int(inter[b]), int(uni[b]), r)


def test_the_batch_holds_what_it_says():
    ref = want(17)
    assert [r[0] for r in ref] == [0, 1, 2, 3, 12, 40, 9, 4, 0, 2, 2, 3]
    assert ref[9][1:3] == (0, 0) and ref[10][1] == ref[10][2] > 2 * P.MASH_SORT_TILE and ref[2][1] > 0
    assert 1100 - 32 + 1 > P.MASH_SORT_TILE > 150


@pytest.mark.parametrize("k", KS)
def test_every_case_in_one_batch(engine, k):
    got = engine.block_identity(batch(), k, MIN_LEN)
    check(got, want(k))
    st = engine.stats()
    assert st["kernel_ms"] > 0 and st["device_bytes"] > 0 and st["dp_launches"] == 3 and st["n_slots"] > 0


def test_rounds_under_a_small_budget_give_the_same_bytes(engine):
    k = 17
    one = engine.block_identity(batch(), k, MIN_LEN)
    ref = want(k)
    sent = [[s for s in blk if len(s) >= MIN_LEN] for blk, r in zip(batch(), ref) if r[0] > 1]
    sets_bytes = sum(8 * len(s) + 4 for blk in sent for s in blk)
    deepest = max(r[0] * (r[0] - 1) // 2 for r in ref)
    assert sum(r[0] * (r[0] - 1) // 2 for r in ref) > deepest + 20
    try:
        engine.set_memory_budget(sets_bytes + 8 * (deepest + 20))        # the words of the deepest block and twenty more
        two = engine.block_identity(batch(), k, MIN_LEN)
        st = engine.stats()
        engine.set_memory_budget(sets_bytes + 8 * (deepest - 1))
        with pytest.raises(P.PoaError, match="memory budget too small"):
            engine.block_identity(batch(), k, MIN_LEN)
    finally:
        engine.set_memory_budget(0)
    assert (st["dp_launches"] - 1) // 2 > 1                               # the sketch + (pairs, select) per round
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    check(two, ref)


def test_too_long_sequence_fails_its_block_only(engine):
    rng = np.random.default_rng(5)
    long_blk = [rng.integers(0, 4, 300).astype(np.uint8), rng.integers(0, 4, P.MAX_SEQ_LEN + 1).astype(np.uint8)]
    assert len(long_blk[1]) == 26624
    blocks = [batch()[4], long_blk, batch()[7]]
    used, inter, uni, status = engine.block_identity(blocks, 17, MIN_LEN, check=False)
    ref = IR.identify_blocks(blocks, 17, MIN_LEN)
    assert [r[3] for r in ref] == [0, P.ST_TOO_LONG, 0] and (int(inter[1]), int(uni[1])) == (0, 0)
    check((used, inter, uni, status), ref)
    with pytest.raises(P.PoaError, match="longer than"):
        engine.block_identity(blocks, 17, MIN_LEN)


def test_bad_parameters(engine):
    blk = [batch()[2]]
    for k in (0, 33):
        with pytest.raises(P.PoaError, match="kmer_size"):
            engine.block_identity(blk, k, 200)
    with pytest.raises(P.PoaError, match="min_len"):
        engine.block_identity(blk, 17, 16)
    for pc in (-0.1, 1.5, float("nan")):
        with pytest.raises(P.PoaError, match="percentile"):
            engine.block_identity(blk, 17, MIN_LEN, pc)
    for pc, pick in ((0.0, min), (1.0, max)):                              # the ends of the range are ranks 0 and P - 1
        used, inter, uni, _ = engine.block_identity([batch()[4]], 17, MIN_LEN, pc)
        js = [IR.jaccard(*p) for p in IR.pair_counts(batch()[4], 17)]
        assert IR.jaccard(int(inter[0]), int(uni[0])) == pick(js)


def test_same_batch_twice_gives_the_same_bytes(engine):
    one, two = engine.block_identity(batch(), 17, MIN_LEN), engine.block_identity(batch(), 17, MIN_LEN)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    assert engine.stats()["kernel_ms"] > 0


def test_device_thresholds_are_the_host_estimators(engine):
    sm = S.Smoother(open(DRB1).read(), 700)
    host_thr, host_used = sm.identity_thresholds(17)
    thr, used = sm.identity_thresholds(17, S.gpu_identifier(engine))
    assert thr.tobytes() == host_thr.tobytes() and used.tolist() == host_used.tolist() and (used > 1).sum() >= 10


@pytest.mark.parametrize("sub", [0.0005, 0.004, 0.012, 0.02])
def test_adaptive_iteration_with_the_device_estimate_is_byte_equal_on_haplotypes(engine, sub):
    sm = S.Smoother(haplotype_gfa(int(sub * 1e5), sub=sub), 450)
    p = S.default_params(adaptive_poa_params=1, kmer_size=15)
    without = sm.smooth_gfa(p, S.gpu_provider(engine))
    assert smooth_gfa_with(sm, p, S.gpu_provider(engine), S.gpu_identifier(engine)) == without


def test_adaptive_iteration_with_the_device_estimate_is_byte_equal_on_drb1(engine):
    sm = S.Smoother(open(DRB1).read(), 700)
    p = S.default_params(adaptive_poa_params=1)
    without = sm.smooth_gfa(p, S.gpu_provider(engine))
    assert smooth_gfa_with(sm, p, S.gpu_provider(engine), S.gpu_identifier(engine)) == without
    got = sm.smooth_maf_gfa(p, S.gpu_provider(engine), identity=S.gpu_identifier(engine))
    assert got == sm.smooth_maf_gfa(p, S.gpu_provider(engine))

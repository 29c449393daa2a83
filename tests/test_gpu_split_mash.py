"""GPU: the mash-based branch of the identity split (src/breaks.cpp:388-471; decrees M1-M5 of DESIGN.md section 9) --
sxg_poa_kmer_jaccard_batch and sxg_poa_split_mash_batch against the restatement in tests/split_mash_ref.py.  Sets are compared
key by key, intersections and counters as integers, groups id by id: there is no tolerance anywhere."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_mash_ref as M  # noqa: E402
import split_ref as R  # noqa: E402
import split_synth as Y  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = P.MASH_SORT_TILE
K, MIN_LEN = 17, 200


def check_sets(engine, seqs, pairs, k):
    """One batch on the GPU: every set against np.unique, every intersection against Python sets."""
    size, inter, sets = engine.kmer_jaccard(seqs, pairs, k, want_sets=True)
    want = [M.kmer_set(s, k) for s in seqs]
    for q, (w, g) in enumerate(zip(want, sets)):
        assert int(size[q]) == len(w) and g.dtype == np.uint64 and np.array_equal(g, w), (q, len(seqs[q]), k)
    as_set = [set(w.tolist()) for w in want]
    assert [int(x) for x in inter] == [len(as_set[a] & as_set[b]) for a, b in pairs]
    size2, inter2 = engine.kmer_jaccard(seqs, pairs, k)
    assert size2.tolist() == size.tolist() and inter2.tolist() == inter.tolist()
    return size, inter


def with_keys(rng, n, k):
    """A random sequence with n windows (distinct k-mers: n at the k used here, but for a chance repeat np.unique sees too)."""
    return rng.integers(0, 4, n + k - 1).astype(np.uint8)


@pytest.mark.parametrize("k", [11, 17, 32])
def test_sets_around_the_wave_and_the_tile(engine, k):
    rng = np.random.default_rng(100 + k)
    counts = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
    seqs = [np.full(250, 4, np.uint8)] + [with_keys(rng, n, k) for n in counts]
    seqs += [Y.mutate(rng, s, max(1, len(s) // 50)) for s in seqs[1:]]
    unit = rng.integers(0, 4, 20).astype(np.uint8)
    seqs += [np.tile(unit, 15)[:299], np.tile(unit, 200)[:3 * TILE + 77], np.zeros(k - 1, np.uint8), np.zeros(0, np.uint8)]
    nn = rng.integers(0, 4, TILE + 300).astype(np.uint8)
    nn[rng.choice(len(nn), 25, replace=False)] = 4                       # windows with an N, on both sides of a tile edge
    seqs.append(nn)
    n = len(seqs)
    pairs = [(q, q + len(counts)) for q in range(1, 1 + len(counts))]     # a sequence and its mutated copy
    pairs += [(0, 0), (0, 5), (5, 0), (n - 2, 3), (4, 4), (8, 8), (1, 2), (6, 7), (n - 5, n - 4), (n - 1, n - 1), (n - 1, 8)]
    size, inter = check_sets(engine, seqs, pairs, k)
    assert int(size[0]) == 0 and int(size[1]) == 1 and int(size[n - 3]) == 0 and int(size[n - 2]) == 0
    assert int(size[n - 5]) == int(size[n - 4]) == 20 == int(inter[len(counts) + 8])   # a tandem repeat of a 20-mer: duplicates collapse
    if k >= 17:
        assert [int(x) for x in size[1:1 + len(counts)]] == list(counts)
        assert int(inter[len(counts) + 6]) == 0 and int(inter[len(counts) + 7]) == 0      # unrelated: disjoint
    assert int(inter[len(counts) + 4]) == int(size[4]) and int(inter[len(counts) + 5]) == int(size[8])   # identical sets


def test_largest_sequence_and_its_mutated_copy(engine):
    rng = np.random.default_rng(7)
    a = rng.integers(0, 4, P.MAX_SEQ_LEN).astype(np.uint8)
    b = Y.mutate(rng, a, 300, (5, -5))
    size, inter = check_sets(engine, [a, b, R.revcomp(a)], [(0, 1), (1, 0), (0, 2), (0, 0)], K)
    assert int(size[0]) > 26000 and 0 < int(inter[0]) < int(size[0]) and int(inter[2]) == int(size[0]) == int(inter[3])


def test_reverse_complement_has_the_same_set(engine):
    rng = np.random.default_rng(8)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in (40, 300, TILE + 50)]
    seqs += [R.revcomp(s) for s in seqs]
    size, inter = check_sets(engine, seqs, [(0, 3), (1, 4), (2, 5)], K)
    assert inter.tolist() == size[:3].tolist() == size[3:].tolist()


def test_bad_arguments_of_the_set_call(engine):
    a = np.zeros(50, np.uint8)
    for k in (0, 33):
        with pytest.raises(P.PoaError, match="kmer_size"):
            engine.kmer_jaccard([a], [], k)
    with pytest.raises(P.PoaError, match="no such sequence"):
        engine.kmer_jaccard([a], [(0, 1)], K)
    with pytest.raises(P.PoaError, match="longer than"):
        engine.kmer_jaccard([np.zeros(P.MAX_SEQ_LEN + 1, np.uint8)], [], K)


# ------------------------------------------------------------------------------------------------------------------
def fam_block(seed, per_fam, length, within, across, n_fam=2, rc_second=False, indel_every=3):
    rng = np.random.default_rng(seed)
    fam = Y.families(rng, n_fam, per_fam, length, within, across, indel_every)
    seqs = [R.revcomp(s) if rc_second and f == 1 else s for f, s in fam]
    srt, _ = R.dedup_sort(seqs)
    return srt


@functools.lru_cache(maxsize=None)
def block(key):
    if key == "families":
        return fam_block(21, 6, 300, 3, 60)
    if key == "rc":
        return fam_block(22, 6, 300, 3, 60, rc_second=True)
    if key == "alternating":
        fam = fam_block(27, 6, 300, 2, 0, n_fam=1)
        return R.dedup_sort([R.revcomp(s) if k % 2 else s for k, s in enumerate(fam)])[0]
    if key == "both_rules":
        rng = np.random.default_rng(40)
        seqs = [s for _, s in Y.families(rng, 2, 4, 150, 2, 40, 3)] + [s for _, s in Y.families(rng, 2, 5, 320, 3, 70, 3)]
        return R.dedup_sort(seqs)[0]
    if key == "size_break":
        rng = np.random.default_rng(41)
        unit = rng.integers(0, 4, 20).astype(np.uint8)
        return R.dedup_sort([np.tile(unit, 15)[:299]] + [s for _, s in Y.families(rng, 2, 5, 300, 3, 60, 0)])[0]
    if key == "all_n":
        return [np.full(250, 4, np.uint8), np.full(260, 4, np.uint8)]
    if key == "deep":
        return fam_block(50, 20, 400, 4, 90, n_fam=3)
    if key == "one":
        return fam_block(23, 1, 80, 0, 0, n_fam=1)
    if key == "two":
        return fam_block(24, 1, 250, 2, 40)
    if key == "short":
        return fam_block(25, 6, 100, 2, 30)
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def want(key, t, k=K, min_len=MIN_LEN, e=None):
    """M4's answer for a block, computed once: (groups, n_groups, n_pairs, n_mash)."""
    return M.greedy_mash(block(key), t, 0.0, k, min_len, e)


def check(engine, keys, t, k=K, min_len=MIN_LEN, e=None):
    got = engine.split_mash([block(key) for key in keys], t, 0.0, k, min_len, e)
    for key, (grp, ng, npairs, nmash, st) in zip(keys, got):
        w = want(key, t, k, min_len, e)
        assert st == 0 and (list(grp), ng, npairs, nmash) == (list(w[0]), w[1], w[2], w[3]), key
    return got


def test_two_families(engine):
    assert len(block("families")) == 12 and want("families", 0.95)[1:] == (2, 0, 36)
    check(engine, ["families"], 0.95)
    assert want("families", 0.95, e=0.99)[1:] == (12, 0, 66)               # a stricter estimate keeps nobody together
    check(engine, ["families"], 0.95, e=0.99)
    for k in (11, 32):
        assert want("families", 0.95, k=k)[1:] == (2, 0, 36) and want("families", 0.95, k=k)[0] == want("families", 0.95)[0]
        check(engine, ["families"], 0.95, k=k)


def test_strand_is_in_the_canonical_kmer(engine):
    assert want("rc", 0.95)[1:] == (2, 0, 20)
    assert want("alternating", 0.95)[1:] == (1, 0, 5)                     # the reverse pass does nothing
    check(engine, ["rc", "alternating"], 0.95)


def test_both_rules_in_one_block(engine):
    assert want("both_rules", 0.9)[1:] == (4, 52, 25)
    check(engine, ["both_rules"], 0.9)
    assert engine.stats()["cells"] > 0


def test_size_break_of_the_member_loop(engine):
    assert want("size_break", 0.95)[1:] == (3, 0, 13)
    assert M.greedy_mash(block("size_break"), 0.95, 0.0, K, MIN_LEN, size_break=False)[1:] == (3, 0, 15)
    check(engine, ["size_break"], 0.95)


def test_empty_sets_are_compared_and_never_joined(engine):
    assert want("all_n", 0.95) == ([0, 1], 2, 0, 1)
    check(engine, ["all_n"], 0.95)


def test_depths_in_one_batch_and_a_block_without_the_branch(engine):
    assert len(block("deep")) == 60 and want("deep", 0.95)[1:] == (3, 0, 564)
    keys = ["deep", "one", "two", "short", "families"]
    min_len = [MIN_LEN, MIN_LEN, MIN_LEN, MIN_LEN, 0]
    got = engine.split_mash([block(key) for key in keys], 0.95, 0.0, K, min_len)
    st = engine.stats()
    for key, ml, (grp, ng, npairs, nmash, status) in zip(keys, min_len, got):
        w = want(key, 0.95, K, ml)
        assert status == 0 and (list(grp), ng, npairs, nmash) == (list(w[0]), w[1], w[2], w[3]), key
    plain = engine.split([block("families")], 0.95, 0.0)[0]
    assert (list(got[4][0]), got[4][1], got[4][2], got[4][3]) == (list(plain[0]), plain[1], plain[2], 0)
    assert want("short", 0.95)[3] == 0 and want("short", 0.95)[2] > 0      # below min_len: the edit path
    assert st["kernel_ms"] > 0 and st["cells"] > 0 and st["device_bytes"] > 0


def test_too_long_sequence_fails_its_block_only(engine):
    long_blk = [np.zeros(300, np.uint8), np.zeros(P.MAX_SEQ_LEN + 1, np.uint8)]
    got = engine.split_mash([long_blk, block("families")], 0.95, 0.0, K, MIN_LEN, check=False)
    w = want("families", 0.95)
    assert got[0][4] == P.ST_TOO_LONG and got[0][1] == 0 and got[0][3] == 0
    assert got[1][4] == 0 and (list(got[1][0]),) + got[1][1:4] == (list(w[0]),) + tuple(w[1:])
    with pytest.raises(P.PoaError):
        engine.split_mash([long_blk], 0.95, 0.0, K, MIN_LEN)


def test_bad_parameters(engine):
    blk = [block("families")]
    with pytest.raises(P.PoaError, match="min_len"):
        engine.split_mash(blk, 0.95, 0.0, K, K - 1)
    for e in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(P.PoaError, match="est_identity"):
            engine.split_mash(blk, 0.95, 0.0, K, MIN_LEN, e)
    with pytest.raises(P.PoaError, match="kmer_size"):
        engine.split_mash(blk, 0.95, 0.0, 33, MIN_LEN)
    with pytest.raises(P.PoaError, match="identity"):
        engine.split_mash(blk, 0.0, 0.0, K, MIN_LEN)


def test_same_batch_twice_gives_the_same_bytes(engine):
    blocks = [block(key) for key in ("deep", "both_rules", "rc", "one")]
    one, two = engine.split_mash(blocks, 0.9, 0.0, K, MIN_LEN), engine.split_mash(blocks, 0.9, 0.0, K, MIN_LEN)
    for (g1, *r1), (g2, *r2) in zip(one, two):
        assert g1.tobytes() == g2.tobytes() and r1 == r2
    assert engine.stats()["kernel_ms"] > 0


def test_discover_split_mash_smooth_end_to_end(engine):
    """synthetic two-family graph with ranges of more than 200 bases -> block discovery -> mash split on the GPU -> one
    smoothing iteration on the GPU; the blockset is the one the Python callback provider gives."""
    import gfa_invariants as GI
    from test_split_mash_host import RefMashSplitter
    text = Y.two_family_gfa(31, backbone=30, node_bp=20, flank=40)
    disc = dict(target_poa_length=1000, n_haps=8)
    sm = S.Smoother(text, discover=disc)
    before = sm.n_blocks
    ranges = sorted(r for k in range(before) for r in sm.block_ranges(k))
    assert max(r[3] for r in ranges) >= MIN_LEN
    n_split, n_long = sm.split_blocks_mash(S.gpu_mash_splitter(engine), 0.9, 0.0, 1, MIN_LEN, 0, 0.0, K)
    assert n_split >= 1 and n_long == 0 and sm.n_blocks == before + n_split
    assert sorted(r for k in range(sm.n_blocks) for r in sm.block_ranges(k)) == ranges
    ref = S.Smoother(text, discover=disc)
    prov = RefMashSplitter()
    ref.split_blocks_mash(prov.splitter(), 0.9, 0.0, 1, MIN_LEN, 0, 0.0, K)
    assert any(s[2] == MIN_LEN for s in prov.seen)
    assert [sm.block_ranges(k) for k in range(sm.n_blocks)] == [ref.block_ranges(k) for k in range(ref.n_blocks)]
    out = sm.smooth_gfa(S.default_params(), S.gpu_provider(engine))
    GI.check_laced(out, text)

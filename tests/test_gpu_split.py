"""GPU: the identity split of break_blocks (src/breaks.cpp:335-586; decrees P1-P4 of DESIGN.md section 9) --
sxg_poa_pair_identity_batch and sxg_poa_split_batch against the restatement in tests/split_ref.py.  Triples are compared,
not floats; for blocks the group ids AND the number of pair sweeps must be P3's (the device runs the same comparisons)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R  # noqa: E402
import split_synth as Y  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402

pytestmark = pytest.mark.gpu
PANEL = P.SPLIT_PANEL


def check_pairs(engine, seqs, pairs, caps=None, rev=None):
    """One batch on the GPU; every pair against split_ref (cap = len(a) unless given)."""
    caps = [len(seqs[a]) for a, _ in pairs] if caps is None else caps
    pen, cols, mat = engine.pair_identity(seqs, pairs, caps, rev)
    for k, (a, b) in enumerate(pairs):
        sb = R.revcomp(seqs[b]) if rev is not None and rev[k] else seqs[b]
        want = R.pair_identity(seqs[a], sb, caps[k])
        assert (int(pen[k]), int(cols[k]), int(mat[k])) == want, (k, len(seqs[a]), len(seqs[b]), caps[k])
    return pen, cols, mat


def related(rng, length, other_length=None):
    a = rng.integers(0, 4, length).astype(np.uint8)
    b = Y.mutate(rng, a, max(1, length // 40))
    if other_length is not None and other_length != length:
        d = other_length - length
        b = Y.mutate(rng, b, 0, (d,))
    return a, b


def test_pairs_of_lengths_around_the_wave(engine):
    rng = np.random.default_rng(1)
    lens = (1, 2, 63, 64, 65)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in lens]
    seqs += [Y.mutate(rng, s, 1) for s in seqs]
    pairs = [(a, b) for a in range(len(seqs)) for b in range(len(seqs))]
    check_pairs(engine, seqs, pairs, caps=[1 << 20] * len(pairs))     # every triple, identity or not


@pytest.mark.parametrize("width", [PANEL - 1, PANEL, PANEL + 1, 2 * PANEL + 1])
def test_pairs_around_the_panel_width(engine, width):
    rng = np.random.default_rng(width)
    a, b = related(rng, width)
    c, d = related(rng, width, width - 37)                 # the columns end before the panel does / in an earlier panel
    short = Y.mutate(rng, a[:100], 2)
    seqs = [a, b, c, d, short]
    # columns run over the second sequence: both as rows and as columns, len(a) < len(b) and the reverse
    check_pairs(engine, seqs, [(0, 1), (1, 0), (2, 3), (3, 2), (4, 0), (0, 4)], caps=[1 << 20] * 6)


def test_orientation_flag(engine):
    rng = np.random.default_rng(3)
    a, b = related(rng, 300)
    n4 = np.array([0, 4, 1, 4, 4, 2, 3] * 20, np.uint8)     # N complements to N
    seqs = [a, R.revcomp(b), b, n4, R.revcomp(Y.mutate(rng, n4, 3)), related(rng, 600)[0]]
    seqs.append(R.revcomp(Y.mutate(rng, seqs[5], 5, (4, -7))))
    pairs = [(0, 1), (0, 1), (0, 2), (3, 4), (5, 6), (6, 5)]
    rev = [1, 0, 1, 1, 1, 1]
    pen, cols, mat = check_pairs(engine, seqs, pairs, rev=rev)
    assert cols[0] > 0 and cols[1] == 0 and cols[3] > 0 and cols[4] > 0      # related only in the right orientation


def test_all_n(engine):
    n = [np.full(k, 4, np.uint8) for k in (1, 70, 75, 600)]
    pen, cols, mat = check_pairs(engine, n, [(1, 1), (1, 2), (2, 1), (0, 3), (3, 3)], caps=[1 << 20] * 5)
    assert (int(pen[0]), int(cols[0]), int(mat[0])) == (0, 70, 70)           # N = N matches
    assert (int(pen[1]), int(cols[1]), int(mat[1])) == (16, 71, 70)


def test_anchor_pairs(engine):
    from test_split_ref import anchors
    seqs, pairs, want = [], [], []
    for name, a, b, triple in anchors():
        seqs += [np.asarray(a, np.uint8), np.asarray(b, np.uint8)]
        pairs.append((len(seqs) - 2, len(seqs) - 1))
        want.append(triple)
    pen, cols, mat = check_pairs(engine, seqs, pairs)
    for k, t in enumerate(want):
        if t is not None:
            assert (int(pen[k]), int(cols[k]), int(cols[k] - mat[k])) == t
        else:
            assert pen[k] >= 700 and cols[k] == 0 and mat[k] == 0           # unrelated: no identity below the cap


def test_cap_is_a_strict_bound(engine):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, 200).astype(np.uint8)
    b = a.copy()
    b[[20, 90, 150]] = (b[[20, 90, 150]] + 1) % 4                            # penalty 21
    pen, cols, mat = check_pairs(engine, [a, b], [(0, 1)] * 3, caps=[22, 21, 20])
    assert list(pen) == [21, 21, 21] and list(cols) == [200, 0, 0] and list(mat) == [197, 0, 0]


def test_mutated_random_pairs(engine):
    rng = np.random.default_rng(6)
    seqs, pairs = [], []
    for k in range(100):
        n = int(rng.integers(5, 700)) if k % 4 else int(rng.integers(400, 700))
        a = rng.integers(0, 4 + (k % 7 == 0), n).astype(np.uint8)
        indels = tuple(int(x) for x in rng.integers(-6, 7, int(rng.integers(0, 4))) if x)
        if k % 10 == 3:
            indels += (int(rng.integers(20, 60)) * (1 if k % 20 == 3 else -1),)      # a long one
        b = Y.mutate(rng, a, int(rng.integers(0, max(2, n // 25))), indels)
        if len(b) > 700:
            b = b[:700]
        seqs += [a, b]
        pairs.append((2 * k, 2 * k + 1) if k % 2 else (2 * k + 1, 2 * k))
    rev = [int(k % 5 == 0) for k in range(100)]
    pen, cols, mat = check_pairs(engine, seqs, pairs, rev=rev)
    assert 20 < int((cols > 0).sum()) < 100                                  # both sides of the bound are in play


# ------------------------------------------------------------------------------------------------------------------
def fam_block(seed, per_fam, length, within, across, n_fam=2, rc_second=False, indel_every=3):
    rng = np.random.default_rng(seed)
    fam = Y.families(rng, n_fam, per_fam, length, within, across, indel_every)
    seqs = [R.revcomp(s) if rc_second and f == 1 else s for f, s in fam]
    srt, _ = R.dedup_sort(seqs)
    return srt


@functools.lru_cache(maxsize=None)
def ref_blocks(key):
    """Blocks (dedup'd, sorted) with P3's answer, computed once: -> (blocks, t, ratio, [(groups, n_groups, n_pairs)])."""
    if key == "families":
        blocks, t, ratio = [fam_block(21, 6, 300, 3, 60)], 0.95, 0.0
    elif key == "rc":
        blocks, t, ratio = [fam_block(22, 6, 300, 3, 60, rc_second=True)], 0.95, 0.0
    elif key == "mixed":       # depth 1, 2 and 40 in one batch, one block longer than the panel
        blocks = [fam_block(23, 1, 80, 0, 0, n_fam=1), fam_block(24, 1, 150, 2, 40), fam_block(25, 20, 100, 2, 30),
                  fam_block(26, 2, PANEL + 90, 4, 150)]
        t, ratio = 0.9, 0.0
    else:
        raise KeyError(key)
    return blocks, t, ratio, [R.greedy(b, t, ratio) for b in blocks]


def check_blocks(engine, blocks, t, ratio, want):
    got = engine.split(blocks, t, ratio)
    for b, ((grp, ng, npairs, st), (wg, wng, wnp)) in enumerate(zip(got, want)):
        assert st == 0
        assert (list(grp), ng, npairs) == (list(wg), wng, wnp), b
    return got


def test_two_families_split_in_two(engine):
    blocks, t, ratio, want = ref_blocks("families")
    assert len(blocks[0]) == 12 and want[0][1] == 2
    check_blocks(engine, blocks, t, ratio, want)


def test_second_family_stored_reverse_complemented(engine):
    blocks, t, ratio, want = ref_blocks("rc")
    assert want[0][1] == 2
    check_blocks(engine, blocks, t, ratio, want)
    # ... and a family whose members alternate in orientation is ONE group: the reverse complement is tried second
    fam = fam_block(27, 6, 200, 2, 0, n_fam=1)
    alt, _ = R.dedup_sort([R.revcomp(s) if k % 2 else s for k, s in enumerate(fam)])
    w = R.greedy(alt, 0.95, 0.0)
    assert w[1] == 1
    check_blocks(engine, [alt], 0.95, 0.0, [w])


def test_identity_exactly_on_the_threshold_joins(engine):
    a = np.array([0, 1, 2, 3] * 5, np.uint8)
    one, two = a.copy(), a.copy()
    one[7] = (one[7] + 1) % 4                    # 19 matches of 20 columns: 0.95 >= 0.95
    two[3], two[12] = (two[3] + 2) % 4, (two[12] + 2) % 4
    for blk in ([a, one], [a, two]):
        srt, _ = R.dedup_sort(blk)
        w = R.greedy(srt, 0.95, 0.0)
        check_blocks(engine, [srt], 0.95, 0.0, [w])
    assert R.greedy(R.dedup_sort([a, one])[0], 0.95, 0.0)[1] == 1
    assert R.greedy(R.dedup_sort([a, two])[0], 0.95, 0.0)[1] == 2


def test_both_early_exits_of_the_member_loop(engine):
    rng = np.random.default_rng(28)
    base = rng.integers(0, 4, 100).astype(np.uint8)
    by_ratio, _ = R.dedup_sort([base[:50], base, Y.mutate(rng, base, 1)])                 # 50 / 100 < 0.8: never aligned
    by_len, _ = R.dedup_sort([base[:10], base[:30], Y.mutate(rng, base[:30], 1)])         # 10 < 0.95 / 0.05 = 18: never aligned
    want = [R.greedy(by_ratio, 0.9, 0.8), R.greedy(by_len, 0.95, 0.0), R.greedy(by_len, 1.0, 0.0)]
    assert want[0][1:] == (2, 1) and want[1][1:] == (2, 1) and want[2][1:] == (3, 2)      # (t = 1: "always", only equal lengths are aligned)
    got = engine.split([by_ratio, by_len, by_len], [0.9, 0.95, 1.0], [0.8, 0.0, 0.0])
    assert [(list(g), n, p) for g, n, p, s in got] == [(list(g), n, p) for g, n, p in want]


def test_mixed_depths_and_a_block_longer_than_the_panel(engine):
    blocks, t, ratio, want = ref_blocks("mixed")
    assert [len(b) for b in blocks] == [1, 2, 40, 4] and want[0] == ([0], 1, 0) and want[2][1] == 2 and want[3][1] == 2
    check_blocks(engine, blocks, t, ratio, want)
    st = engine.stats()
    assert st["cells"] == sum(cells_of(b, t, ratio) for b in blocks) and st["kernel_ms"] > 0


def cells_of(block, t, ratio):
    """Cells of the pair alignments P3 runs on a block."""
    seen = []

    def spy(a, b, cap):
        seen.append(len(a) * len(b))
        return R.pair_identity(a, b, cap)

    R.greedy(block, t, ratio, pair=spy)
    return sum(seen)


def test_too_long_sequence_fails_its_block_only(engine):
    blocks, t, ratio, want = ref_blocks("families")
    long_blk = [np.zeros(100, np.uint8), np.zeros(P.MAX_SEQ_LEN + 1, np.uint8)]
    got = engine.split([long_blk, blocks[0]], t, ratio, check=False)
    assert got[0][3] == P.ST_TOO_LONG and got[0][1] == 0
    assert got[1][3] == 0 and (list(got[1][0]), got[1][1], got[1][2]) == (list(want[0][0]), want[0][1], want[0][2])
    with pytest.raises(P.PoaError):
        engine.split([long_blk], t, ratio)
    with pytest.raises(P.PoaError, match="no bases"):
        engine.split([[np.zeros(0, np.uint8), np.zeros(5, np.uint8)]], t, ratio)


def test_same_batch_twice_gives_the_same_bytes(engine):
    blocks, t, ratio, _ = ref_blocks("mixed")
    one, two = engine.split(blocks, t, ratio), engine.split(blocks, t, ratio)
    for (g1, n1, p1, s1), (g2, n2, p2, s2) in zip(one, two):
        assert g1.tobytes() == g2.tobytes() and (n1, p1, s1) == (n2, p2, s2)


def test_discover_split_smooth_end_to_end(engine):
    """synthetic two-family graph -> block discovery -> split on the GPU -> one smoothing iteration on the GPU: every path
    spells its sequence (tests/gfa_invariants.py, applied by the conftest to every smooth_gfa) and the block count grew."""
    import gfa_invariants as GI
    text = Y.two_family_gfa(31)
    sm = S.Smoother(text, discover=dict(target_poa_length=1000, n_haps=8))
    before = sm.n_blocks
    ranges = sorted(r for k in range(before) for r in sm.block_ranges(k))
    n_split, n_long = sm.split_blocks(S.gpu_splitter(engine), 0.9, 0.0, 1)
    assert n_split >= 1 and n_long == 0 and sm.n_blocks == before + n_split
    assert sorted(r for k in range(sm.n_blocks) for r in sm.block_ranges(k)) == ranges
    out = sm.smooth_gfa(S.default_params(), S.gpu_provider(engine))
    GI.check_laced(out, text)
    # the same split as P3 in Python gives
    from test_split_host import RefSplitter
    ref = S.Smoother(text, discover=dict(target_poa_length=1000, n_haps=8))
    ref.split_blocks(RefSplitter().splitter(), 0.9, 0.0, 1)
    assert [sm.block_ranges(k) for k in range(sm.n_blocks)] == [ref.block_ranges(k) for k in range(ref.n_blocks)]

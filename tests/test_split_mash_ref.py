"""CPU: the restatement of the mash-based branch of the identity split (tests/split_mash_ref.py; decrees M1-M5 of DESIGN.md
section 9) against properties of M1, a brute force, the product's canonical_kmers (reached through the A14 estimator) and the
walks the issue of this feature worked out by hand."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_mash_ref as M  # noqa: E402
import split_ref as R  # noqa: E402
import split_synth as Y  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402


def brute_set(s, k):
    """M1 on strings: every window and its reverse complement as text, the smaller one kept."""
    text = "".join("ACGTN"[c] for c in s)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    out = set()
    for p in range(len(text) - k + 1):
        w = text[p:p + k]
        if "N" in w:
            continue
        r = "".join(comp[c] for c in reversed(w))
        out.add(int("".join(str("ACGT".index(c)) for c in min(w, r)), 4))      # A < C < G < T: text order = value order
    return sorted(out)


@pytest.mark.parametrize("k", [1, 5, 11, 17, 31, 32])
def test_sets_against_brute_force_and_strand_symmetry(k):
    rng = np.random.default_rng(k)
    for n in (k - 1, k, k + 1, 90):
        s = rng.integers(0, 4, max(n, 0)).astype(np.uint8)
        if n == 90:
            s[[13, 60]] = 4
        got = M.kmer_set(s, k)
        assert got.dtype == np.uint64 and got.tolist() == brute_set(s, k)
        assert M.kmer_set(R.revcomp(s), k).tolist() == got.tolist()


def test_window_with_an_n_is_skipped():
    rng = np.random.default_rng(2)
    s = rng.integers(0, 4, 60).astype(np.uint8)
    t = s.copy()
    t[30] = 4
    clean = [M.kmer_set(s[p:p + 17], 17)[0] for p in range(44) if not (p <= 30 < p + 17)]
    assert M.kmer_set(t, 17).tolist() == sorted(set(int(x) for x in clean))
    assert len(M.kmer_set(np.full(250, 4, np.uint8), 17)) == 0 and len(M.kmer_set(s[:16], 17)) == 0


def test_tandem_repeat_collapses():
    unit = np.random.default_rng(3).integers(0, 4, 20).astype(np.uint8)
    assert len(M.kmer_set(np.tile(unit, 15)[:299], 17)) == 20


@pytest.mark.parametrize("k", [11, 17, 32])
def test_sets_agree_with_the_product_estimator(k):
    """sxg_block_identity_threshold of a block of two sequences is max(0.7, (float)(1 - dist)) of canonical_kmers' sets."""
    rng = np.random.default_rng(10 + k)
    a = rng.integers(0, 4, 400).astype(np.uint8)
    b = Y.mutate(rng, a, 6, (3, -2))
    a[100] = 4
    text, ranges, _ = Y.blocks_gfa([[a, R.revcomp(b)]])
    sm = S.Smoother(text, blocks=ranges)
    thr, used = sm.identity_threshold(0, k)
    ka, kb = set(M.kmer_set(a, k).tolist()), set(M.kmer_set(b, k).tolist())
    inter = len(ka & kb)
    j = inter / (len(ka) + len(kb) - inter)
    want = np.float32(1.0 - (-math.log(2.0 * j / (1.0 + j)) / k))
    assert used == 2 and want > 0.7 and np.float32(thr) == want


def test_thresholds_restate_the_distance_test():
    for t, k in ((0.95, 17), (0.9, 11), (0.99, 32), (1.0, 17)):
        f, jmin = M.thresholds(t, t, k)
        assert f == jmin
        if t < 1:
            assert abs((1 - (-math.log(2 * jmin / (1 + jmin)) / k)) - t) < 1e-12      # J = jmin is identity t
    assert M.thresholds(1.0, 1.0, 17) == (1.0, 1.0)


def fam_block(seed, per_fam, length, within, across, n_fam=2, rc_second=False, indel_every=3):
    rng = np.random.default_rng(seed)
    fam = Y.families(rng, n_fam, per_fam, length, within, across, indel_every)
    return R.dedup_sort([R.revcomp(s) if rc_second and f == 1 else s for f, s in fam])[0]


def no_sweep(a, b, cap):
    raise AssertionError("an eligible pair was aligned")


def test_walks_worked_out_by_hand():
    b = fam_block(21, 6, 300, 3, 60)
    assert M.greedy_mash(b, 0.95, 0.0, 17, 200, pair=no_sweep)[1:] == (2, 0, 36)
    assert M.greedy_mash(b, 0.95, 0.0, 17, 200, e=0.99, pair=no_sweep)[1:] == (12, 0, 66)
    assert M.greedy_mash(fam_block(22, 6, 300, 3, 60, rc_second=True), 0.95, 0.0, 17, 200, pair=no_sweep)[1:] == (2, 0, 20)
    assert M.greedy_mash(b, 0.95, 0.0, 17, 0)[:3] == R.greedy(b, 0.95, 0.0)          # min_len 0 is P3


def test_size_break_and_empty_sets():
    rng = np.random.default_rng(41)
    unit = rng.integers(0, 4, 20).astype(np.uint8)
    b, _ = R.dedup_sort([np.tile(unit, 15)[:299]] + [s for _, s in Y.families(rng, 2, 5, 300, 3, 60, 0)])
    assert M.greedy_mash(b, 0.95, 0.0, 17, 200)[1:] == (3, 0, 13)
    assert M.greedy_mash(b, 0.95, 0.0, 17, 200, size_break=False)[1:] == (3, 0, 15)
    n = [np.full(250, 4, np.uint8), np.full(260, 4, np.uint8)]
    assert M.greedy_mash(n, 0.95, 0.0, 17, 200) == ([0, 1], 2, 0, 1)                 # uni == 0: compared, never joined

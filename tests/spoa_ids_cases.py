"""The blocks the tests of decree S6' (SXG_IDS_SPOA) share: tests/test_spoa_ids_ref.py anchors the reference on them,
tests/test_graph_emul_ids.py and tests/test_gpu_spoa_ids.py compare the product with the reference on them."""
import numpy as np

from helpers import random_block

SCORE_SETS = ("convex_default", "affine_4param", "linear")

# 20 random blocks: 4-10 sequences of 40-160 bp, 5-25 % divergence; the seeds are fixed (test_spoa_ids_ref.py checks that the
# two id rules differ on them in ranks and in paths: the comparison is not vacuous)
RANDOM_SEEDS = tuple(range(9100, 9120))
INSERTION_SEEDS = (9200, 9201, 9202)


def random_case(seed):
    rng = np.random.default_rng(seed)
    n_seqs = int(rng.integers(4, 11))
    length = int(rng.integers(40, 161))
    div = float(rng.uniform(0.05, 0.25))
    seqs = random_block(rng, n_seqs, length, div=div)
    return seqs, rng.integers(1, 4, len(seqs)).astype(np.int64)


def insertion_case(seed):
    """A block one of whose sequences carries a 30-base insertion."""
    rng = np.random.default_rng(seed)
    seqs = random_block(rng, 6, int(rng.integers(80, 141)), div=0.1)
    k = int(rng.integers(1, len(seqs)))
    at = int(rng.integers(10, len(seqs[k]) - 10))
    seqs[k] = np.concatenate([seqs[k][:at], rng.integers(0, 4, 30, dtype=np.uint8), seqs[k][at:]])
    return seqs, np.ones(len(seqs), np.int64)


def case_set():
    """[(name, seqs, weights)]"""
    out = [("random%d" % s,) + random_case(s) for s in RANDOM_SEEDS]
    out += [("insertion%d" % s,) + insertion_case(s) for s in INSERTION_SEEDS]
    return out


# ---- the hand-written anchor (local mode, convex_default: m 1, n -4, a one-base gap -6)
# Sequence 0: 40 letters over ACGT.  Sequence 1: the same, its first 3 and last 3 letters replaced by N (code 4: aligns to nothing
# in a graph over ACGT), one mismatch at position 15 and one letter inserted behind position 25.  The local alignment runs over
# positions 3 .. 37 of sequence 1: 12 matches (12), the mismatch (8), 10 matches (18), the insertion (12), 11 matches (23 -- the
# strictly greatest cell, so the walk ends there and begins at the first match).
ANCHOR_LEN = 40


def anchor(prefix=True, suffix=True):
    rng = np.random.default_rng(424242)
    s0 = rng.integers(0, 4, ANCHOR_LEN, dtype=np.uint8)
    # (no letter repeats its neighbour: the inserted letter, equal to none of its neighbours, cannot slide)
    for i in range(1, ANCHOR_LEN):
        while s0[i] == s0[i - 1]:
            s0[i] = (s0[i] + 1) % 4
    s1 = s0.copy()
    if prefix:
        s1[:3] = 4
    if suffix:
        s1[-3:] = 4
    s1[15] = (s0[15] + 2) % 4
    ins = [c for c in range(4) if c != s1[25] and c != s1[26]][0]
    s1 = np.concatenate([s1[:26], np.asarray([ins], np.uint8), s1[26:]])
    return [s0, s1], np.ones(2, np.int64)


def unrelated():
    """The anchor without its N tips (the graph holds ACGT only), then a run of seven N: it aligns to nothing -- an empty walk."""
    seqs, _ = anchor(False, False)
    return seqs + [np.full(7, 4, np.uint8)], np.ones(3, np.int64)

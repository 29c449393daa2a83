"""CPU: the restatement of the pair identity (decree P1 / P2 of DESIGN.md section 9) in tests/split_ref.py against a
brute-force enumeration of all alignments, against a plain Gotoh, and on the anchor pairs the decree quotes."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_ref as R  # noqa: E402


def test_recurrence_equals_brute_force_optimum():
    rng = np.random.default_rng(11)
    n = 0
    for _ in range(320):
        a = rng.integers(0, 2, int(rng.integers(1, 7)))
        b = rng.integers(0, 2, int(rng.integers(1, 7)))
        assert R.pair_triple(a, b) == R.brute_triple(a, b), (a, b)
        n += 1
    assert n >= 300


def test_penalty_equals_plain_gotoh():
    rng = np.random.default_rng(12)
    for _ in range(60):
        a = rng.integers(0, 4, int(rng.integers(1, 60)))
        b = a.copy() if rng.random() < 0.7 else rng.integers(0, 4, int(rng.integers(1, 60)))
        for _ in range(int(rng.integers(0, 5))):           # a few substitutions / indels
            p = int(rng.integers(0, len(b)))
            if rng.random() < 0.5:
                b[p] = (b[p] + 1) % 4
            elif len(b) > 3:
                b = np.delete(b, slice(p, p + int(rng.integers(1, 4))))
        if len(b) == 0:
            b = a[:1]
        assert R.pair_triple(a, b)[0] == R.gotoh_penalty(list(a), list(b))
        assert R.pair_triple(a, b) == R.pair_triple(b, a)
        assert R.pair_triple(R.revcomp(a), b) == R.pair_triple(a, R.revcomp(b))


def anchors():
    rng = np.random.default_rng(2024)
    A20 = [0] * 20
    s = rng.integers(0, 4, 700)
    t = s.copy()
    pos = np.arange(10, 700, 38)[:18]
    t[pos] = (t[pos] + 1) % 4
    u = np.random.default_rng(77).integers(0, 4, 700)
    return [("five", A20 + [1] * 5 + A20, A20 + [2] * 5 + A20, (32, 41, 1)),
            ("four", A20 + [1] * 4 + A20, A20 + [2] * 4 + A20, (28, 44, 4)),
            ("subst", s, t, (126, 700, 18)),
            ("unrelated", s, u, None)]


def test_anchor_pairs():
    for name, a, b, want in anchors():
        got = R.pair_triple(a, b)
        if want is not None:
            assert got == want, name
            assert R.pair_identity(a, b, len(a)) == (want[0], want[1], want[1] - want[2])
        else:
            assert got[0] >= 700, got                        # no identity below the cap of P2
            assert R.pair_identity(a, b, 700)[1:] == (0, 0)


def test_bound_is_strict():
    a, b = [0] * 10 + [1] + [0] * 10, [0] * 10 + [2] + [0] * 10     # one mismatch: penalty 7
    assert R.pair_identity(a, b, 8) == (7, 21, 20)
    assert R.pair_identity(a, b, 7) == (7, 0, 0)


def test_greedy_and_dedup_small():
    rng = np.random.default_rng(5)
    fam = [rng.integers(0, 4, 120) for _ in range(2)]
    seqs = []
    for k in range(6):
        s = fam[k % 2].copy()
        s[10 + k] = (s[10 + k] + 1) % 4
        seqs.append(s)
    seqs.append(seqs[0].copy())              # a duplicate
    seqs.append(R.revcomp(seqs[1]))          # a reverse-complement duplicate
    srt, ranks = R.dedup_sort(seqs)
    assert len(srt) == 6 and sorted(sum(ranks, [])) == list(range(8))
    assert [0, 6] in ranks and [1, 7] in ranks
    blocks, n_pairs = R.split_block(seqs, 0.9, 0.0, 1)
    assert len(blocks) == 2 and sorted(sum(blocks, [])) == list(range(8)) and n_pairs > 0
    assert {r % 2 for r in blocks[0] if r < 6} != {r % 2 for r in blocks[1] if r < 6}
    assert R.split_block(seqs, 0.9, 0.0, 0) == ([list(range(8))], 0)        # the CLI default: never split
    assert R.split_block(seqs, 0.9, 0.0, 7) == ([list(range(8))], 0)        # depth below the minimum

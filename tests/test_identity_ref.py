"""CPU: decree Q against the oracle.  tests/identity_ref.py picks ONE pair per block in exact integers
(Fractions); max(0.7f, f(J)) of that pair must be oracle/smooth_oracle.py's identity_threshold -- the sorted-float rule of
src/smooth.cpp:2026 -- as float32, bit for bit: Q4's claim, also where pair identities are zero or negative."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import identity_ref as IR  # noqa: E402
from oracle import smooth_oracle as SO  # noqa: E402
from test_smooth_host import DRB1, haplotype_gfa, synthetic_gfa  # noqa: E402

CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
HAP_SUBS = (0.0005, 0.004, 0.012, 0.02)          # test_adaptive_iteration_high_identity_tiers


def codes(text):
    return np.asarray([CODE.get(ch, 4) for ch in text], np.uint8)


def range_seqs(g, ranges):
    return ["".join(g.sequence(h) for h in g.steps[p][b:e]) for (p, b, e, _) in ranges]


def cases():
    """(name, oracle graph, blocks as lists of ranges, k) of every graph the estimate is pinned on."""
    out = []
    for seed, k in ((4, 5), (5, 7), (6, 11)):      # test_identity_threshold_matches_oracle
        g = SO.Graph(synthetic_gfa(seed, n_paths=6, n_nodes=80))
        out.append(("synthetic%d" % seed, g, SO.blockset_by_path_windows(g, 150), k))
    for sub in HAP_SUBS:
        g = SO.Graph(haplotype_gfa(int(sub * 1e5), sub=sub))
        out.append(("haplotype%g" % sub, g, SO.blockset_by_path_windows(g, 450), 15))
    g = SO.Graph(open(DRB1).read())
    blocks = SO.blockset_by_path_windows(g, 700)
    out.append(("drb1", g, [blocks[b] for b in (0, 3, 7, 11)], 17))
    return out


@pytest.fixture(scope="module")
def graphs():
    return cases()


def check_block(seqs, k, thr, used):
    n_used, inter, uni, status = IR.block([codes(s) for s in seqs], k, 8 * k)
    assert (n_used, status) == (used, IR.ST_OK)
    if used > 1:
        got = IR.threshold(inter, uni, k)
        assert got.dtype == np.float32 and thr.dtype == np.float32 and got.tobytes() == thr.tobytes(), (inter, uni, got, thr)
    else:
        assert (inter, uni) == (0, 0) and thr is None


def test_ref_threshold_is_the_oracles_bit_for_bit(graphs):
    tiers, n_checked = set(), 0
    for name, g, blocks, k in graphs:
        for ranges in blocks:
            thr, used = SO.identity_threshold(g, ranges, k)
            check_block(range_seqs(g, ranges), k, thr, used)
            if used > 1:
                tiers.add(SO.adaptive_scores(thr))
                n_checked += 1
    assert n_checked >= 30
    assert len(tiers) >= 3, tiers                  # (from the oracle alone)


# Q4's case.  Two sequences whose canonical 4-mer sets share exactly ONE of 129 k-mers -- J = 1/129, identity below 0 --,
# one that shares nothing with a third (J = 0, identity 0), and near copies (identities close to 1).
A4 = "TTAGTTGTGCCGCATGTTTCGATAGCAGTCCTTGAACGAGGCTGTACTCACTTAACCAGGGGTATTGGATGGCGA"
B4 = "CCACGCGCTCCGTCTCTTTTGCAAATTATGACACCGGGCCCACCTACGTGGGAAGCTCCCGACCTAGAATGATCTAA"
POLY_A, POLY_C = "A" * 40, "AC" * 20
A4_COPY = A4[:30] + "T" + A4[31:]


class ListGraph:
    """Just enough of the oracle's graph for identity_threshold: one single-node path per sequence."""

    def __init__(self, seqs):
        self.seqs, self.steps = seqs, [[q] for q in range(len(seqs))]

    def sequence(self, h):
        return self.seqs[h]

    def ranges(self):
        return [(q, 0, 1, len(s)) for q, s in enumerate(self.seqs)]


@pytest.mark.parametrize("seqs", [[A4, B4, POLY_A, POLY_C], [A4, B4, POLY_A, POLY_C, A4_COPY], [A4, B4, A4_COPY, A4, B4, A4_COPY],
                                  [A4, B4], [POLY_A, POLY_C], [A4.lower(), B4, "N" * 40, A4_COPY]],
                         ids=["lower_set", "rank_at_the_edge", "rank_above", "negative_alone", "zero_alone", "lower_case_and_n"])
def test_zero_and_negative_pair_identities_end_at_the_floor(seqs):
    k = 4
    sets = [SO.canonical_kmers(s, k) for s in seqs]
    ids = [SO.mash_identity(sets[i], sets[j], k) for i in range(len(seqs)) for j in range(i + 1, len(seqs))]
    if A4 in seqs or A4.lower() in seqs:
        assert any(x < 0 for x in ids), ids        # the oracle alone shows a pair identity below 0 ...
        inter = len(SO.canonical_kmers(A4, k) & SO.canonical_kmers(B4, k))
        assert inter == 1 and len(SO.canonical_kmers(A4, k) | SO.canonical_kmers(B4, k)) == 129
    if POLY_A in seqs or "N" * 40 in seqs:
        assert any(x == 0 for x in ids), ids       # ... and one of exactly 0 (J = 0)
    g = ListGraph(seqs)
    thr, used = SO.identity_threshold(g, g.ranges(), k)
    assert used == len(seqs)
    check_block(seqs, k, thr, used)


def test_the_lower_set_is_a_lower_set_in_both_orders():
    """Q4 directly: over every (inter, uni) a block can show at k = 4 and k = 5, the pairs with identity <= 0 are exactly an
    initial stretch of the J order, and the identity never decreases with J once J > 0 (at J = 0 it is 0 by definition,
    ABOVE the negative ones: the two orders differ only inside the stretch that the floor flattens)."""
    for k, top in ((4, 140), (5, 530)):
        pairs = sorted(((i, u) for u in range(1, top, 7) for i in sorted({0, 1, 2} | set(range(0, u + 1, max(1, u // 40)))) if i <= u),
                       key=lambda p: IR.jaccard(*p))
        vals = [float(IR.identity(i, u, k)) for i, u in pairs]
        positive = [v for (i, u), v in zip(pairs, vals) if i > 0]
        assert all(a <= b for a, b in zip(positive, positive[1:])) and any(v < 0 for v in positive)
        n_low = sum(v <= 0 for v in vals)
        assert 0 < n_low < len(vals) and all(v <= 0 for v in vals[:n_low])

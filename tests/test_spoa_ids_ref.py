"""CPU: the plain-Python reference of decree S6' (tests/spoa_ids_ref.py) is anchored before anything is compared with it:
under sequence-order ids it must be the oracle, bit for bit; a hand-written block spells the expected ids out; in global mode
the two id rules coincide; in local mode they differ -- in the names of the nodes, and in nothing else."""
import numpy as np
import pytest

import spoa_ids_cases as K
import spoa_ids_ref as R
from helpers import oparams


def params(oracle, pname, mode):
    p = oparams(pname, mode)
    p.mode = mode | 0x10
    return p


def same(a, b):
    return (len(a.node_code) == len(b.node_code) and (a.node_code == b.node_code).all() and (a.node_rank == b.node_rank).all()
            and (a.node_group == b.node_group).all() and len(a.edge_tail) == len(b.edge_tail) and (a.edge_tail == b.edge_tail).all()
            and (a.edge_head == b.edge_head).all() and (a.edge_weight == b.edge_weight).all()
            and all((x == y).all() for x, y in zip(a.paths, b.paths)) and (a.scores == b.scores).all())


@pytest.fixture(scope="module")
def runs(oracle):
    """Both id rules on the whole case set, once: {(pname, mode, name): (sequence-order result, spoa-order result)}"""
    out = {}
    for pname in K.SCORE_SETS:
        for mode in (0, 1):
            p = params(oracle, pname, mode)
            for name, seqs, w in K.case_set():
                out[pname, mode, name] = (R.run_block(seqs, w, p, ids="sequence"), R.run_block(seqs, w, p, ids="spoa"))
    return out


def test_sequence_order_ids_are_the_oracle(oracle, runs):
    for pname in K.SCORE_SETS:
        for mode in (0, 1):
            p = params(oracle, pname, mode)
            for name, seqs, w in K.case_set():
                g, sc, _ = oracle.block_run(seqs, w, p)
                r = runs[pname, mode, name][0]
                code, rank, grp = g.nodes()
                t, h, ww = g.edges()
                label = (pname, mode, name)
                assert (r.node_code == code).all() and (r.node_rank == rank).all() and (r.node_group == grp).all(), label
                assert (r.edge_tail == t).all() and (r.edge_head == h).all() and (r.edge_weight == ww).all(), label
                for s in range(g.n_seqs):
                    assert (r.paths[s] == g.seq_path(s)).all(), label
                assert (r.scores == sc).all(), label


def test_hand_written_anchor(oracle):
    """Sequence 0: 40 letters.  Sequence 1: the same with its first 3 and last 3 letters replaced by letters that cannot align,
    one mismatch (position 15) and one inserted letter (position 26); local mode, convex_default.  (The issue asked for 24
    letters: with m = 1, n = -4 and a one-letter gap of -6 no local alignment of 18 middle letters gets over both the
    mismatch and the insertion -- the score behind them, 17 - 10 = 7, is not above the peak before them.  40 letters:
    12 -> 8 -> 18 -> 12 -> 23.)"""
    seqs, w = K.anchor()
    p = params(oracle, "convex_default", 0)
    n0 = K.ANCHOR_LEN
    assert len(seqs[0]) == n0 and len(seqs[1]) == n0 + 1
    spoa = R.run_block(seqs, w, p, ids="spoa")
    seq = R.run_block(seqs, w, p, ids="sequence")
    assert spoa.spans == [None, (3, n0 - 3)] and spoa.scores.tolist() == [0, 23]
    backbone = list(range(n0))
    want_spoa = [n0, n0 + 1, n0 + 2] + backbone[3:n0 - 3] + [n0 + 3, n0 + 4, n0 + 5]     # prefix 40 41 42, suffix 43 44 45
    want_spoa[15] = n0 + 6                                                               # the mismatch: the first middle node
    want_spoa.insert(26, n0 + 7)                                                         # the insertion: the second
    want_seq = [n0, n0 + 1, n0 + 2] + backbone[3:n0 - 3] + [n0 + 5, n0 + 6, n0 + 7]       # position order
    want_seq[15] = n0 + 3
    want_seq.insert(26, n0 + 4)
    assert spoa.paths[0].tolist() == backbone and seq.paths[0].tolist() == backbone
    assert spoa.paths[1].tolist() == want_spoa
    assert seq.paths[1].tolist() == want_seq
    # the same graph up to the names of its nodes
    ren = dict(zip(seq.paths[1].tolist(), spoa.paths[1].tolist()))
    ren.update({v: v for v in backbone})
    assert [(ren[t], ren[h]) for t, h in zip(seq.edge_tail.tolist(), seq.edge_head.tolist())] == list(zip(spoa.edge_tail.tolist(), spoa.edge_head.tolist()))
    assert (seq.edge_weight == spoa.edge_weight).all()
    assert spoa.node_group[n0 + 6] == 15 and seq.node_group[n0 + 3] == 15


def test_prefix_only_suffix_only_neither(oracle):
    p = params(oracle, "convex_default", 0)
    n0 = K.ANCHOR_LEN
    for prefix, suffix in ((True, False), (False, True), (False, False)):
        seqs, w = K.anchor(prefix, suffix)
        a, b = R.run_block(seqs, w, p, ids="spoa"), R.run_block(seqs, w, p, ids="sequence")
        assert a.spans[1] == (3 if prefix else 0, n0 - 3 if suffix else n0)
        # without a suffix nothing overtakes the middle: the rules coincide
        assert same(a, b) == (not suffix), (prefix, suffix)


def test_empty_walk_is_one_chain(oracle):
    seqs, w = K.unrelated()
    p = params(oracle, "convex_default", 0)
    r = R.run_block(seqs, w, p, ids="spoa")
    assert r.spans[2] is None and r.scores[2] == 0
    n = len(r.node_code)
    assert r.paths[2].tolist() == list(range(n - 7, n))


def test_global_mode_both_rules_agree(runs):
    for (pname, mode, name), (a, b) in runs.items():
        if mode == 1:
            assert same(a, b), (pname, name)


def renaming(a, b):
    """The map from a's node names to b's that the paths spell out, sequence by sequence; None when there is none (some later
    alignment took another way through the graph)."""
    ren = {}
    if len(a.node_code) != len(b.node_code):
        return None
    for pa, pb in zip(a.paths, b.paths):
        if len(pa) != len(pb):
            return None
        for x, y in zip(pa.tolist(), pb.tolist()):
            if ren.setdefault(x, y) != y:
                return None
    return ren if len(set(ren.values())) == len(ren) == len(a.node_code) else None


def test_local_mode_rules_differ(runs):
    """Not vacuous: on the local-mode case set the two rules differ in some node's rank on at least one block and in a path on at
    least one block -- the arrays a caller receives are not the same."""
    rank_differs, path_differs = 0, 0
    for (pname, mode, name), (a, b) in runs.items():
        if mode != 0:
            continue
        assert len(a.node_code) == len(b.node_code)
        rank_differs += int((a.node_rank != b.node_rank).any())
        path_differs += int(any((x != y).any() for x, y in zip(a.paths, b.paths)))
    assert rank_differs > 0 and path_differs > 0, (rank_differs, path_differs)


def test_local_mode_rules_differ_by_a_renaming_only(runs):
    """What the difference amounts to (DESIGN.md section 2, S6'): under the re-sort S7' the two rules give the same graph under
    other node names -- same rank for every node, same scores, same edges and weights.  A walk of the re-sort starts at a node
    none of whose descendants has a smaller id; a new node inside the span always leads to an old node (the walk's last aligned
    node), so it never starts a walk, and the rules only swap such nodes with the suffix chain.  Pinned here so that a change that
    breaks it is seen."""
    checked = 0
    for (pname, mode, name), (a, b) in runs.items():
        if mode != 0:
            continue
        ren = renaming(a, b)
        assert ren is not None, (pname, name)
        assert (a.scores == b.scores).all()
        assert all(a.node_rank[x] == b.node_rank[y] and a.node_code[x] == b.node_code[y] for x, y in ren.items()), (pname, name)
        assert [(ren[t], ren[h]) for t, h in zip(a.edge_tail.tolist(), a.edge_head.tolist())] == list(zip(b.edge_tail.tolist(), b.edge_head.tolist()))
        assert (a.edge_weight == b.edge_weight).all()
        checked += int(any(x != y for x, y in ren.items()))
    assert checked >= 10    # (blocks on which the renaming is not the identity)

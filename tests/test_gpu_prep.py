"""GPU: the path-guided SGD node order of prep (sxg_poa_path_sgd_order, decree Y of DESIGN.md section 9) against its
restatement in tests/prep_ref.py -- order AND coordinates, bit for bit, on both device paths -- and prep end to end on DRB1:
sort on the GPU, chop, real block discovery, one batched GPU POA call, lacing, against the oracle stack."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prep_ref as R  # noqa: E402
from oracle import smooth_oracle as SO  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402

pytestmark = pytest.mark.gpu
DRB1 = os.path.join(HERE, "golden", "DRB1-3123.seqwish.gfa")
LDS, GLOBAL = 1, 2


def graph(node_len, paths):
    """paths: lists of node ranks -> (node_len, path_off, step_node, step_pos)."""
    path_off, step_node, step_pos = [0], [], []
    for p in paths:
        bp = 0
        for r in p:
            step_node.append(r)
            step_pos.append(bp)
            bp += node_len[r]
        path_off.append(len(step_node))
    return np.array(node_len, np.int32), np.array(path_off, np.int64), np.array(step_node, np.int32), np.array(step_pos, np.int64)


def check(engine, g, modes=(LDS, GLOBAL), iter_max=10, term_updates=1.0, seed=R.DEFAULT_SEED):
    """Both device paths against the restatement; returns (order, x, stats per mode)."""
    node_len, path_off, step_node, step_pos = g
    eta, cs, terms = R.schedule(path_off, iter_max=iter_max, term_updates=term_updates)
    want_order, want_x = R.sgd_order(node_len, path_off, step_node, step_pos, eta, cs, terms, seed)
    stats = {}
    for mode in modes:
        order, x = engine.path_sgd_order(node_len, path_off, step_node, step_pos, eta, cs, terms, seed, mode=mode)
        assert x.dtype == np.int64 and x.tobytes() == want_x.tobytes(), (mode, int((x != want_x).sum()))
        assert order.tobytes() == want_order.tobytes(), mode
        stats[mode] = engine.stats()
        n_batches = -(-terms // max(1, len(node_len) // 8)) if int(path_off[-1]) else 0
        if n_batches:
            which = mode if mode else (LDS if len(node_len) <= P.SGD_LDS_NODES else GLOBAL)
            assert stats[mode]["n_slots"] == (1 if which == LDS else 2 * iter_max * n_batches)    # the number of launches
            assert stats[mode]["kernel_ms"] > 0 and stats[mode]["device_bytes"] >= 16 * len(node_len)
    return want_order, want_x, stats


@pytest.mark.parametrize("n", [1, 7, 9])
def test_degenerate_sizes(engine, n):
    """N = 1; N = 7: a batch of one term; N = 9: the first size with 8 | N false and B = 1 still."""
    rng = np.random.default_rng(n)
    lens = rng.integers(1, 9, n).tolist()
    paths = [rng.permutation(n).tolist(), rng.permutation(n)[: max(1, n // 2)].tolist()]
    _, x, _ = check(engine, graph(lens, paths), term_updates=3)
    if n > 1:
        assert x.tolist() != (np.cumsum([0] + lens)[:n] << 20).tolist()


def test_one_path_of_one_step(engine):
    order, x, _ = check(engine, graph([3, 4, 5], [[1]]))
    assert order.tolist() == [0, 1, 2] and x.tolist() == [0, 3 << 20, 7 << 20]


def test_graph_without_steps(engine):
    order, x, _ = check(engine, graph([3, 0, 0, 5], []))
    assert order.tolist() == [0, 1, 2, 3] and x.tolist() == [0, 3 << 20, 3 << 20, 3 << 20]


def test_star_colliding_atomic_adds_on_one_word(engine):
    """One hub shared by 64 paths of 3 steps, 520 nodes in all so that a batch holds 65 terms: nearly every term of a batch
    moves the hub, and the sums must not depend on the order the adds arrive in."""
    n = 520
    lens = np.random.default_rng(1).integers(1, 30, n).tolist()
    paths = [[1 + 2 * p, 0, 2 + 2 * p] for p in range(64)]
    g = graph(lens, paths)
    assert n // 8 >= 64
    a = check(engine, g, term_updates=2, iter_max=20)
    b = check(engine, g, term_updates=2, iter_max=20)                           # and again: the same bits
    assert a[1].tobytes() == b[1].tobytes()


def test_revisited_nodes_and_zero_distance_pairs(engine):
    """Y4's skips: a pair on one node (the path comes back to it) and a pair of node ends at the same offset (the end of a
    step is the start of the next; nodes of no bases)."""
    lens = [4, 0, 6, 1, 0, 3, 2, 5, 1, 7, 2, 2]
    paths = [[0, 1, 0, 2, 2, 3, 4, 4, 0, 5, 1, 6], [7, 8, 7, 8, 9, 9, 9, 10], [11, 11, 11]]
    check(engine, graph(lens, paths), term_updates=6, iter_max=30)


def test_shuffled_linear_graph_with_a_partial_last_batch(engine):
    g = R.shuffled_linear(2000, 8, 11)
    terms = int(g[1][-1])
    assert terms % (2000 // 8) != 0                                             # the last batch of an iteration is partial
    check(engine, g, iter_max=10)


@pytest.mark.parametrize("n", [P.SGD_LDS_NODES, P.SGD_LDS_NODES + 1])
def test_lds_path_boundary(engine, n):
    g = R.shuffled_linear(n, 2, n)
    _, _, stats = check(engine, g, modes=(0,), iter_max=2)
    assert (stats[0]["n_slots"] == 1) == (n <= P.SGD_LDS_NODES)
    if n > P.SGD_LDS_NODES:
        eta, cs, terms = R.schedule(g[1], iter_max=2)
        with pytest.raises(P.PoaError):
            engine.path_sgd_order(*g, eta, cs, terms, 1, mode=LDS)


def test_limits_are_checked_before_anything_is_launched(engine):
    g = graph([1 << 30] * 1024, [[0, 1, 2]])                                    # 2^40 bases
    eta, cs, terms = R.schedule(g[1], iter_max=2)
    with pytest.raises(P.PoaError):
        engine.path_sgd_order(*g, eta, cs, terms, 1)
    g = graph([3, 4, 5], [[0, 1, 2]])
    with pytest.raises(P.PoaError):
        engine.path_sgd_order(*g, None, cs, terms, 1)                           # eta == NULL
    with pytest.raises(P.PoaError):
        engine.path_sgd_order(g[0], g[1], np.array([0, 3, 1], np.int32), g[3], eta, cs, terms, 1)   # a step names no node
    engine.path_sgd_order(*g, eta, cs, terms, 1)                                # the handle still works


@functools.lru_cache(maxsize=None)
def drb1_reference():
    text = open(DRB1).read()
    seqs, paths, edges = R.parse_gfa(text)
    g = R.flatten(seqs, paths)
    eta, cs, terms = R.schedule(g[1])
    return text, g, (eta, cs, terms), R.sgd_order(*g, eta, cs, terms, R.DEFAULT_SEED)


def test_drb1_at_full_settings(engine):
    """100 iterations, 2.58 M terms, 3 585 nodes: the LDS path's home.  Both paths give the reference's order and coordinates;
    the prepped GFA -- sxg_graph_prep with the GPU as its sort provider -- has the digest the CPU suite pinned."""
    text, g, (eta, cs, terms), (want_order, want_x) = drb1_reference()
    for mode in (0, LDS, GLOBAL):
        order, x = engine.path_sgd_order(*g, eta, cs, terms, R.DEFAULT_SEED, mode=mode)
        st = engine.stats()
        print("DRB1 sort mode %d: kernel_ms %.3f launches %d device_bytes %d" % (mode, st["kernel_ms"], st["n_slots"], st["device_bytes"]))
        assert x.tobytes() == want_x.tobytes() and order.tobytes() == want_order.tobytes(), mode
    gold = json.load(open(os.path.join(HERE, "golden", "prep_drb1.json")))
    for mode in (0, GLOBAL):
        got = S.prep_gfa(text, S.gpu_sorter(engine), mode=mode)
        assert hashlib.sha256(got.encode()).hexdigest() == gold["prepped_gfa_sha256"], mode


def test_drb1_prepped_iteration_end_to_end(engine):
    """prep on the GPU, then the iteration the reference's ctest runs (-l 700 -j 5k -e 5k -r 12) on the prepped graph: real
    block discovery, ONE batched GPU POA call, lacing.  The GFA equals the oracle stack's over the same blocks and every
    input path still spells its sequence (tests/gfa_invariants.py runs on the output through conftest.py)."""
    text = open(DRB1).read()
    prepped = S.prep_gfa(text, S.gpu_sorter(engine))
    g0, g = SO.Graph(text), SO.Graph(prepped)
    blocks = SO.break_blocks(g, SO.smoothable_blocks(g, 700 * 12, 700, 5000, 5000), 1400)
    assert len(blocks) <= 216
    sm = S.Smoother(prepped, discover=dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000))
    assert [sm.block_ranges(k) for k in range(sm.n_blocks)] == [[tuple(r) for r in blk] for blk in blocks]
    got = sm.smooth_gfa(S.default_params(add_consensus=1), S.gpu_provider(engine))
    st = engine.stats()
    print("prepped DRB1: %d blocks, kernel_ms %.3f (%.3f ms per block)" % (len(blocks), st["kernel_ms"], st["kernel_ms"] / len(blocks)))
    assert got == SO.smooth(g, blocks, add_consensus=True)
    out = SO.Graph(got)
    for q, nm in enumerate(g0.pname):
        assert out.path_sequence(out.pname.index(nm)) == g0.path_sequence(q)
    sm.close()

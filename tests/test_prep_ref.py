"""CPU: the restatement of decree Y (tests/prep_ref.py) on hand-made graphs, and against a scalar restatement of the same
decree written with Python integers and floats, one term at a time."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prep_ref as R  # noqa: E402

M64 = (1 << 64) - 1


def mix1(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def scalar_order(node_len, path_off, step_node, step_pos, eta, cooling_start, terms, seed):
    """Decree Y, Y1-Y7, term by term."""
    node_len, path_off = [int(v) for v in node_len], [int(v) for v in path_off]
    step_node, step_pos = [int(v) for v in step_node], [int(v) for v in step_pos]
    N, S = len(node_len), path_off[-1]
    X, acc = [], 0
    for v in node_len:
        X.append(acc << 20)
        acc += v
    counts = [path_off[p + 1] - path_off[p] for p in range(len(path_off) - 1)]
    maxsteps = max(counts) if counts else 0
    nb = max(1, (maxsteps - 1).bit_length()) if maxsteps else 1
    B = max(1, N // 8)
    if S == 0:
        terms = 0
    for it in range(len(eta)):
        for k0 in range(0, terms, B):
            D = [0] * N
            for k in range(k0, min(k0 + B, terms)):
                r1 = mix1(mix1(seed ^ (it << 40) ^ k))
                r2 = mix1(r1)
                r3 = mix1(r2)
                a = r1 % S
                p = max(q for q in range(len(counts)) if path_off[q] <= a)
                n, ia = counts[p], a - path_off[p]
                if (r2 & 1) or it >= cooling_start:
                    bits = (r2 >> 1) % nb
                    j = (1 << bits) + ((r2 >> 8) & ((1 << bits) - 1))
                    ib = ia + j if (r2 >> 7) & 1 else ia - j
                    if not 0 <= ib < n:
                        ib = ia - j if (r2 >> 7) & 1 else ia + j
                    ib = min(max(ib, 0), n - 1)
                else:
                    ib = r3 % n
                b = path_off[p] + ib
                i, jn = step_node[a], step_node[b]
                pa = step_pos[a] + (node_len[i] if (r3 >> 62) & 1 else 0)
                pb = step_pos[b] + (node_len[jn] if (r3 >> 63) & 1 else 0)
                d = abs(pa - pb)
                if d == 0 or i == jn:
                    continue
                dx = float(X[i] - X[jn]) / 1048576.0
                mag = abs(dx)
                sgn = 1.0 if dx > 0 else (-1.0 if dx < 0 else (-1.0 if i < jn else 1.0))
                mu = min(float(eta[it]) / float(d), 1.0)
                delta = mu * (mag - float(d)) / 2.0
                q = round(delta * sgn * 1048576.0)          # Python rounds halves to even
                D[i] -= q
                D[jn] += q
            X = [x + dd for x, dd in zip(X, D)]
    return sorted(range(N), key=lambda n: (X[n], n)), X


def run(g, iter_max=10, term_updates=1.0, seed=R.DEFAULT_SEED, fn=R.sgd_order):
    node_len, path_off, step_node, step_pos = g
    eta, cs, terms = R.schedule(path_off, iter_max=iter_max, term_updates=term_updates)
    return fn(node_len, path_off, step_node, step_pos, eta, cs, terms, seed)


def graph(node_len, paths):
    """paths: lists of node ranks."""
    path_off, step_node, step_pos = [0], [], []
    for p in paths:
        bp = 0
        for r in p:
            step_node.append(r)
            step_pos.append(bp)
            bp += node_len[r]
        path_off.append(len(step_node))
    return np.array(node_len, np.int32), np.array(path_off, np.int64), np.array(step_node, np.int32), np.array(step_pos, np.int64)


def test_mix_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 and with 1234567 (published test vectors of the generator)
    assert mix1(0) == 0xE220A8397B1DCDAF
    assert int(R.mix(np.array([0], np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert mix1(1234567) == 6457827717110365317
    x = np.array([0, 1, 2 ** 63, M64], np.uint64)
    assert [int(v) for v in R.mix(x)] == [mix1(int(v)) for v in x]


def test_schedule():
    eta, cs, terms = R.schedule([0, 10, 40, 45])
    assert len(eta) == 100 and cs == 50 and terms == 45
    assert eta[0] == 900.0 and math.isclose(eta[-1], 0.01, rel_tol=1e-12)
    assert all(a > b for a, b in zip(eta, eta[1:]))
    assert R.schedule([0, 10], iter_max=1)[0].tolist() == [100.0]
    assert R.schedule([0, 7], term_updates=2.5)[2] == 17


def test_one_node_graph():
    order, X = run(graph([5], [[0]]))
    assert order.tolist() == [0] and X.tolist() == [0]


def test_a_path_of_one_step_moves_nothing():
    g = graph([3, 4, 5], [[1]])
    order, X = run(g)
    assert order.tolist() == [0, 1, 2] and X.tolist() == [0, 3 << 20, 7 << 20]


def test_a_path_that_visits_a_node_twice():
    g = graph([3, 4, 5, 2], [[0, 1, 0, 2, 3, 1]])
    order, X = run(g, term_updates=4)
    want_order, want_X = run(g, term_updates=4, fn=scalar_order)
    assert order.tolist() == want_order and X.tolist() == want_X
    assert sorted(order.tolist()) == [0, 1, 2, 3]
    assert X.tolist() != [0, 3 << 20, 7 << 20, 12 << 20]                        # something moved
    assert int(X.sum()) == (0 + 3 + 7 + 12) << 20                               # what one node loses the other gains


def test_nodes_on_no_path_keep_their_coordinate():
    g = graph([3, 4, 5, 2, 6, 1], [[4, 0, 2], [2, 0]])
    order, X = run(g, term_updates=3)
    start = (np.cumsum([0, 3, 4, 5, 2, 6])[:6] << 20).tolist()
    assert [X[n] for n in (1, 3, 5)] == [start[n] for n in (1, 3, 5)]
    assert [X[n] for n in (0, 2, 4)] != [start[n] for n in (0, 2, 4)]


def test_equal_coordinates_fall_back_to_the_old_rank():
    order, X = run(graph([0, 0, 0, 4, 0], []))
    assert X.tolist() == [0, 0, 0, 0, 4 << 20] and order.tolist() == [0, 1, 2, 3, 4]
    order, X = run(graph([0, 0, 5, 0], [[2]]))                                   # terms are drawn and all skipped
    assert order.tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("n,paths,seed", [(7, 2, 1), (9, 3, 2), (40, 4, 3)])
def test_the_vectorised_restatement_equals_the_scalar_one(n, paths, seed):
    g = R.shuffled_linear(n, paths, seed)
    order, X = run(g, iter_max=6, term_updates=1.3, seed=seed)
    want_order, want_X = run(g, iter_max=6, term_updates=1.3, seed=seed, fn=scalar_order)
    assert X.tolist() == want_X and order.tolist() == want_order


def test_two_runs_give_equal_bits_and_a_seed_matters():
    g = R.shuffled_linear(300, 4, 5)
    a, xa = run(g, iter_max=20)
    b, xb = run(g, iter_max=20)
    assert a.tobytes() == b.tobytes() and xa.tobytes() == xb.tobytes()
    c, xc = run(g, iter_max=20, seed=R.DEFAULT_SEED + 1)
    assert c.tolist() != a.tolist()


def test_the_sort_brings_path_neighbours_together():
    node_len, path_off, step_node, step_pos = g = R.shuffled_linear(400, 4, 7)
    order, _ = run(g, iter_max=100)
    rank = np.empty(400, np.int64)
    rank[order] = np.arange(400)

    def mean_jump(rk):
        return np.mean(np.concatenate([np.abs(np.diff(rk[step_node[path_off[p]:path_off[p + 1]]])) for p in range(4)]))
    assert mean_jump(np.arange(400)) > 100                                       # shuffled: a third of the graph per step
    assert mean_jump(rank) < 10


def test_limits():
    big = np.full(1024, 1 << 30, np.int32)
    with pytest.raises(ValueError):
        R.sgd_order(big, [0], [], [], np.ones(1), 0, 0)

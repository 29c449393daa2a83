"""GPU: engine handles come and go (sxg_poa_create / sxg_poa_destroy, the group's) at every stage of their life -- nothing run,
uploaded only, after every kind of call, two alive at once, a group that never executed -- and a short-lived handle computes what
a long-lived one does.  Every device resource of a handle frees itself when the handle is deleted (smoothxg_amd/csrc/poa_devres.h);
whether anything leaks is checked on the host (tests/test_devres.py), not here: other work shares the device's memory.

Every call goes through the PoaEngine / PoaGroup wrappers, which raise unless the library answered SXG_OK.  The library's error
text is per thread and is never cleared, so "no error" is asserted as: the text after the test is the text before it (empty when
nothing failed earlier in the process, as when this file runs alone)."""
import os
import sys

import numpy as np
import pytest

import smoothxg_amd as S
from smoothxg_amd import poa as P
from smoothxg_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prep_ref as R  # noqa: E402
from helpers import assert_same  # noqa: E402

pytestmark = pytest.mark.gpu

SCORES = (1, -4, -6, -2, -26, -1)   # convex defaults
PARAMS = S.Params(*SCORES, 0, 0)
RUN = dict(want_consensus=True, want_msa=P.MSA_TRIMMED, block_graph=1, bg_trim=np.full(4, 6, np.int32))


@pytest.fixture(scope="module")
def batch():
    return synth.make_batch(4, 8, 300)   # 4 blocks, 8 sequences, 300 bp


@pytest.fixture(scope="module")
def toy_graph():
    """20 nodes, 2 paths: one through all of them in a shuffled order, one through every other node."""
    rng = np.random.default_rng(20)
    node_len = rng.integers(1, 9, 20).astype(np.int32)
    paths = [rng.permutation(20).tolist(), list(range(0, 20, 2))]
    path_off, step_node, step_pos = [0], [], []
    for p in paths:
        bp = 0
        for r in p:
            step_node.append(r)
            step_pos.append(bp)
            bp += int(node_len[r])
        path_off.append(len(step_node))
    path_off = np.array(path_off, np.int64)
    eta, cooling_start, terms = R.schedule(path_off, iter_max=10, term_updates=3)
    return node_len, path_off, np.array(step_node, np.int32), np.array(step_pos, np.int64), eta, cooling_start, terms, R.DEFAULT_SEED


@pytest.fixture(scope="module")
def first_block(batch, oracle):
    """The first block's sequences, the graph of all but the last of them as the rows of an align problem, and its pairs."""
    bases, seq_off, blk_off = batch
    seqs = [np.asarray(bases[seq_off[s]:seq_off[s + 1]], np.uint8) for s in range(blk_off[0], blk_off[1])]
    g, _, _ = oracle.block_run(seqs[:-1], None, oracle.mkparams(*SCORES, mode=0))
    codes, off, pred, sink, _ = g.rows()
    pairs = [(i, j) for i in range(len(seqs)) for j in range(i + 1, len(seqs))]
    return seqs, (codes, off, pred, sink, seqs[-1]), pairs


def every_call(eng, batch, first_block, toy_graph):
    """A whole batch with consensus, block graphs and the trimmed MSA, then the calls that bring buffers of their own."""
    seqs, problem, pairs = first_block
    res = eng.run_flat(*batch, None, PARAMS, **RUN)
    aligned = eng.align([problem], PARAMS)
    identity = eng.pair_identity(seqs, pairs, [2 * 300] * len(pairs))
    order = eng.path_sgd_order(*toy_graph)
    return res, aligned, identity, order


@pytest.fixture(scope="module")
def long_lived(batch, first_block, toy_graph):
    """An engine that lives as long as the module, and its results (computed once, shared, never changed)."""
    eng = S.PoaEngine(0)
    yield eng, every_call(eng, batch, first_block, toy_graph)
    eng.close()


@pytest.fixture()
def error_text_unchanged():
    lib = S.load_library()
    before = lib.sxg_poa_last_error()
    yield
    assert lib.sxg_poa_last_error() == before
    if not before:
        assert lib.sxg_poa_last_error() == b""


def test_create_destroy(error_text_unchanged):
    eng = S.PoaEngine(0)
    assert eng.compute_units() > 0
    eng.close()
    assert eng.h is None


def test_upload_only(batch, error_text_unchanged):
    eng = S.PoaEngine(0)
    eng.upload(*batch, None, PARAMS, **RUN)
    eng.close()


def test_every_call_then_destroy(batch, first_block, toy_graph, long_lived, error_text_unchanged):
    _, (want_res, want_aligned, want_identity, want_order) = long_lived
    eng = S.PoaEngine(0)
    res, aligned, identity, order = every_call(eng, batch, first_block, toy_graph)
    eng.close()
    assert all(r.status == 0 and r.bg is not None and r.msa and r.consensus is not None for r in res)
    assert_same(res, want_res, "short-lived engine")
    (rows, pos, score, status), (want_rows, want_pos, want_score, want_status) = aligned[0], want_aligned[0]
    assert status == want_status == 0 and score == want_score and len(rows) > 0
    assert rows.tobytes() == want_rows.tobytes() and pos.tobytes() == want_pos.tobytes()
    for got, want in zip(identity, want_identity):
        assert len(got) == 28 and got.tobytes() == want.tobytes()
    assert sorted(order[0].tolist()) == list(range(20))
    assert order[0].tobytes() == want_order[0].tobytes() and order[1].tobytes() == want_order[1].tobytes()


def test_two_handles_alive_at_once(batch, long_lived, error_text_unchanged):
    _, (want_res, _, _, _) = long_lived
    a, b = S.PoaEngine(0), S.PoaEngine(0)
    res_a = a.run_flat(*batch, None, PARAMS, **RUN)
    res_b = b.run_flat(*batch, None, PARAMS, **RUN)
    a.close()   # in creation order: b's buffers, streams and events outlive a's
    assert_same(b.run_flat(*batch, None, PARAMS, **RUN), want_res, "second handle after the first is gone")
    b.close()
    assert_same(res_a, want_res, "first handle")
    assert_same(res_b, want_res, "second handle")


def test_group_uploaded_but_never_executed(batch, error_text_unchanged):
    g = S.PoaGroup([0, 0])
    assert len(g) == 2
    g.upload(*batch, None, PARAMS, **RUN)
    g.close()
    assert g.h is None

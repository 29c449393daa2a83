"""GPU: the result of a sharded run (sxg_poa_batch_run_sharded and its stages) equals the single engine's, field for field.  The
ranks' blobs are their results serialised in the order of the table of result arrays (smoothxg_amd/csrc/poa_results.h) and the
root puts them together with the reassembly the device group uses; here the deal (longest block first onto the least loaded
rank: interleaved, ascending lists) is played with 1, 2, 3 and 5 simulated ranks on one GPU and through a real communicator of
one rank, on the base batch of test_gpu_group.py: 24 blocks of four launch geometries, one block of a single sequence, one without
sequences.  What the sharded entry does not carry -- block_cycles, the trimmed MSA -- stays absent and refused."""
import os
import sys

import numpy as np
import pytest

import smoothxg_amd as S
from smoothxg_amd import poa as P

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from helpers import PARAM_SETS, assert_same, gparams, rerun_in_own_process  # noqa: E402
from test_gpu_group import BUDGET, EMPTY, SCORES, SINGLE, base, base_blocks, trims  # noqa: E402,F401  (the last three are fixtures)

pytestmark = pytest.mark.gpu

RANKS = (1, 2, 3, 5)
PLAIN = S.Params(*SCORES, 0, 0)


@pytest.fixture(scope="module")
def budgeted(engine):
    engine.set_memory_budget(BUDGET)
    yield engine
    engine.set_memory_budget(0)


def raw_request(base_blocks, base):
    """Consensus and the full MSA with per-sequence weights and per-block params (every score set, local and global in turn)."""
    names = list(PARAM_SETS)
    params = [gparams(names[b % len(names)], b % 2) for b in range(len(base_blocks))]
    weights = np.random.default_rng(1602).integers(1, 4, len(base[1]) - 1).astype(np.uint32)
    return weights, params, dict(want_consensus=True, want_msa=P.MSA_FULL)


def assert_sharded(got, want, label):
    assert_same(got, want, label)
    assert all(r.device_cycles is None for r in got), label      # (block_cycles do not travel with the ranks' blobs)
    assert got[SINGLE].status == 0 and got[EMPTY].status == 0 and len(got[EMPTY].scores) == 0


def test_raw_results_with_weights_and_per_block_params(budgeted, base, base_blocks):
    weights, params, req = raw_request(base_blocks, base)
    want = budgeted.run_flat(*base, weights, params, **req)
    assert all(r.status == 0 and r.device_cycles is not None for r in want) and len(want[SINGLE].msa) == 2
    for n in RANKS:
        assert_sharded(budgeted.run_flat_sharded(*base, weights, params, simulate_ranks=n, **req), want, "%d ranks" % n)


@pytest.mark.parametrize("mode", [1, 2])
def test_block_graphs_with_trims(budgeted, base, trims, mode):
    req = dict(want_consensus=True, block_graph=mode, bg_trim=trims)
    want = budgeted.run_flat(*base, None, PLAIN, **req)
    assert all(r.bg is not None and (r.paths is None) == (mode == 2) and r.node_code is not None for r in want)
    for n in RANKS:
        assert_sharded(budgeted.run_flat_sharded(*base, None, PLAIN, simulate_ranks=n, **req), want, "mode %d, %d ranks" % (mode, n))


def test_mode_3_is_answered_as_mode_2(budgeted, base, trims):
    """A sharded run always carries the raw POA graphs to the root."""
    want = budgeted.run_flat(*base, None, PLAIN, want_consensus=True, block_graph=2, bg_trim=trims)
    for n in RANKS:
        got = budgeted.run_flat_sharded(*base, None, PLAIN, want_consensus=True, block_graph=3, bg_trim=trims, simulate_ranks=n)
        assert_sharded(got, want, "mode 3, %d ranks" % n)
        assert all(r.node_code is not None and r.paths is None for r in got)


def test_mode_3_with_the_full_msa_is_answered_as_mode_1(budgeted, base, trims):
    req = dict(want_consensus=True, want_msa=P.MSA_FULL, bg_trim=trims)
    want = budgeted.run_flat(*base, None, PLAIN, block_graph=1, **req)
    for n in RANKS:
        got = budgeted.run_flat_sharded(*base, None, PLAIN, block_graph=3, simulate_ranks=n, **req)
        assert_sharded(got, want, "mode 3 + MSA, %d ranks" % n)
        assert all(r.paths is not None and r.msa is not None for k, r in enumerate(got) if k != EMPTY)


def test_through_a_communicator_of_one_rank(request):
    """The same through RCCL: the one-shot call and the staged form (the collective stage twice).  (In a process of its own:
    see helpers.rerun_in_own_process.)"""
    if rerun_in_own_process(request):
        return
    engine = request.getfixturevalue("budgeted")
    base, base_blocks = request.getfixturevalue("base"), request.getfixturevalue("base_blocks")
    weights, params, req = raw_request(base_blocks, base)
    want = engine.run_flat(*base, weights, params, **req)
    engine.comm_init(engine.comm_unique_id(), 1, 0)
    try:
        assert_sharded(engine.run_flat_sharded(*base, weights, params, **req), want, "communicator")
        engine.upload_sharded(*base, weights, params, **req)
        for _ in range(2):
            engine.execute_sharded()
            info = engine.sharded_info()
            assert (info["ranks_seen"], info["bytes_received"]) == (1, 0)
        assert_sharded(engine.download_sharded(), want, "communicator, staged")
    finally:
        engine.lib.sxg_poa_comm_destroy(engine.h)

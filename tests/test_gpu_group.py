"""GPU: the device group (sxg_poa_group, smoothxg_amd.PoaGroup) -- one process, one engine handle per entry of a device list, a
batch dealt over them in contiguous slices of equal cost, one host thread per member -- returns what ONE engine returns for the
same batch, array for array: raw POA results, the full MSA, block graphs at want_block_graph = 3 with the trimmed MSA built on
the device, per-block params, a batch with a refused block, the staged form, and whole smoothing iterations through
smooth.gpu_provider(group).  The same device may appear more than once in a group, so everything but the last test runs on
one GPU; what it shows there is that the members coexist and that the reassembly is right, not a speed-up."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import smoothxg_amd as S
from smoothxg_amd import poa as P
from smoothxg_amd import smooth as SM

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from helpers import assert_same, random_block  # noqa: E402
from test_identity_host import smooth_gfa_with  # noqa: E402
from test_maf_device_rows_host import HEADER  # noqa: E402
from test_smooth_host import DRB1, synthetic_gfa  # noqa: E402

pytestmark = pytest.mark.gpu

SCORES = (1, -4, -6, -2, -26, -1)   # convex defaults
BUDGET = 1 << 30                    # arena cap of every member
SINGLE, EMPTY = 5, 17               # the block with one sequence, the block without sequences


def make_group(devices):
    g = S.PoaGroup(devices)
    g.set_memory_budget(BUDGET)
    return g


@pytest.fixture(scope="module")
def group():
    g = make_group([0, 0])
    yield g
    g.close()


def flatten(blocks):
    seqs = [s for blk in blocks for s in blk]
    bases = np.concatenate(seqs).astype(np.uint8) if seqs else np.zeros(0, np.uint8)
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    blk_off = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.int32)
    return bases, seq_off, blk_off


@pytest.fixture(scope="module")
def base_blocks():
    """24 blocks of 3-6 sequences at 2 % divergence, lengths from {60, 300, 700, 1500} (every slice of the deal holds more than
    one launch geometry); one block of a single sequence and one without sequences."""
    rng = np.random.default_rng(1601)
    lengths = [60, 300, 700, 1500] * 6
    rng.shuffle(lengths)
    blocks = [random_block(rng, int(rng.integers(3, 7)), int(L), div=0.02) for L in lengths]
    blocks[SINGLE] = blocks[SINGLE][:1]
    blocks[EMPTY] = []
    return blocks


@pytest.fixture(scope="module")
def base(base_blocks):
    return flatten(base_blocks)


@pytest.fixture(scope="module")
def trims(base_blocks):
    """bg_trim as the iteration sets it: the block's padding, here 1/50 of its longest sequence (1, 6, 14 and 30 letters)."""
    return np.asarray([max((len(s) for s in blk), default=0) // 50 for blk in base_blocks], np.int32)


RAW = dict(want_consensus=True, want_msa=P.MSA_FULL)


def compact(trims):
    return dict(want_consensus=True, want_msa=P.MSA_TRIMMED, block_graph=3, bg_trim=trims)


@pytest.fixture(scope="module")
def want_raw(engine, base):
    """The single-engine results of the base batch with consensus and the full MSA (computed once, shared, never changed)."""
    return engine.run_flat(*base, None, S.Params(*SCORES, 0, 0), **RAW)


@pytest.fixture(scope="module")
def want_compact(engine, base, trims):
    return engine.run_flat(*base, None, S.Params(*SCORES, 0, 0), **compact(trims))


# ---- 1
@pytest.mark.parametrize("serial", [0, 1])
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_raw_results_equal_one_engine(engine, base, base_blocks, want_raw, devices, serial, monkeypatch):
    if serial:
        monkeypatch.setenv("SXG_POA_GROUP_SERIAL", "1")
    prm = S.Params(*SCORES, 0, 0)
    g = make_group(devices)
    try:
        assert len(g) == len(devices)
        got = g.run_flat(*base, None, prm, **RAW)
        assert_same(got, want_raw, "devices %r" % (devices,))
        assert got[SINGLE].status == 0 and len(got[SINGLE].msa) == 2 and got[EMPTY].status == 0 and len(got[EMPTY].node_code) == 0
        assert all(r.paths is not None and r.msa is not None for k, r in enumerate(got) if k != EMPTY)
        t = g.timing()
        assert len(t["member_ms"]) == len(devices) and all(ms > 0 for ms in t["member_ms"]) and t["pack_ms"] > 0 and t["assemble_ms"] >= 0
        assert g.stats(len(devices) - 1)["dp_launches"] >= 1 and g.member(0).compute_units() == engine.compute_units()
        # fewer blocks than members, and no blocks at all
        two = flatten(base_blocks[2:4])
        assert_same(g.run_flat(*two, None, prm, **RAW), engine.run_flat(*two, None, prm, **RAW), "two blocks")
        none = flatten([])
        assert g.run_flat(*none, None, prm, **RAW) == engine.run_flat(*none, None, prm, **RAW) == []
    finally:
        g.close()


# ---- 2
def check_compact(g, base, trims, want_compact):
    got = g.run_flat(*base, None, S.Params(*SCORES, 0, 0), **compact(trims))
    assert_same(got, want_compact, "compact")
    assert all(r.node_code is None and r.paths is None and r.bg is not None for r in got)
    assert sum(r.msa is not None and len(r.msa) > 0 and len(r.msa[0]) > 0 for r in got) >= 22
    assert len(got) == len(want_compact) == 24
    for k, r in enumerate(got):      # block_cycles: one entry per block, a positive time for every block that ran
        assert r.device_cycles is not None
        if r.status == 0 and k != EMPTY:
            assert r.device_cycles > 0, k


def test_compact_results_equal_one_engine(group, base, trims, want_compact):
    """Block graphs only (want_block_graph = 3) and the rows of the MAF built on the device: what the sharded entry refuses."""
    check_compact(group, base, trims, want_compact)


# ---- 3
def test_per_block_params(engine, group, base, base_blocks, trims):
    """Tiers of the adaptive scores, global alignment on some blocks and the adaptive band on others."""
    tiers = [SM.adaptive_poa_scores(t) for t in (0.995, 0.985, 0.96, 0.7)]
    assert len(set(tiers)) == 4
    params = []
    for b in range(len(base_blocks)):
        m, n, gp, e, q, c = tiers[b % 4]
        params.append(S.Params(m, -n, -gp, -e, -q, -c, 0x10 | (1 if b % 5 == 1 else 0), 2 if b % 3 == 2 else 0))
    for req in (RAW, compact(trims)):
        assert_same(group.run_flat(*base, None, params, **req), engine.run_flat(*base, None, params, **req), "per-block params")


# ---- 4
def test_a_refused_block_leaves_the_others_complete(engine, group, base_blocks):
    rng = np.random.default_rng(4)
    blocks = [list(b) for b in base_blocks[:12]]
    blocks[7] = [rng.integers(0, 4, P.MAX_SEQ_LEN + 1, dtype=np.uint8), blocks[7][0]]
    flat = flatten(blocks)
    prm = S.Params(*SCORES, 0, 0)
    want = engine.run_flat(*flat, None, prm, check=False, **RAW)
    assert [r.status for r in want] == [0] * 7 + [P.ST_TOO_LONG] + [0] * 4
    got = group.run_flat(*flat, None, prm, check=False, **RAW)
    assert group.last_rc == -4      # SXG_E_BLOCK
    assert_same(got, want, "refused block", refused=(7,))
    with pytest.raises(P.PoaError, match="block 7 failed with status 5"):
        group.run_flat(*flat, None, prm, **RAW)
    group.upload(*flat, None, prm, **RAW)
    assert group.execute(check=False) == -4
    assert_same(group.download(), want, "refused block, staged", refused=(7,))


# ---- 5
def test_staged_run_executes_twice(group, base, trims, want_raw, want_compact):
    prm = S.Params(*SCORES, 0, 0)
    group.upload(*base, None, prm, **RAW)
    assert group.execute() == 0 and group.execute() == 0
    assert_same(group.download(), want_raw, "staged")
    group.upload(*base, None, prm, **compact(trims))
    assert group.execute() == 0 and group.execute() == 0
    assert_same(group.download(), want_compact, "staged, compact")


# ---- 6
def iteration_equals(engine, group, sm, cons_gfa):
    pe, pg = SM.gpu_provider(engine), SM.gpu_provider(group)
    p = SM.default_params(add_consensus=cons_gfa)
    gfa = sm.smooth_gfa(p, pg)
    assert gfa == sm.smooth_gfa(p, pe)
    p = SM.default_params(add_consensus=1)
    new = sm.smooth_maf_gfa(p, pg, header=HEADER, device_rows=True)
    old = sm.smooth_maf_gfa(p, pe, header=HEADER, device_rows=True)
    assert new[0] == old[0] and new[1] == old[1] and new[2] == old[2]
    assert new[1].startswith(HEADER)
    # -a: the identity estimates come from a member engine, the POA calls spread over the group
    p = SM.default_params(add_consensus=1, adaptive_poa_params=1)
    member = group.member(0)
    assert smooth_gfa_with(sm, p, pg, SM.gpu_identifier(member)) == smooth_gfa_with(sm, p, pe, SM.gpu_identifier(engine))
    mafs = [sm.smooth_maf_gfa(p, prov, header=HEADER, device_rows=True, identity=SM.gpu_identifier(e)) for prov, e in ((pg, member), (pe, engine))]
    assert mafs[0] == mafs[1]
    return gfa


def test_iteration_on_the_synthetic_graph(engine, group):
    sm = SM.Smoother(synthetic_gfa(6, n_paths=6, n_nodes=80), 90)
    assert sm.n_blocks >= 4
    iteration_equals(engine, group, sm, 1)
    sm.close()


def test_first_drb1_iteration(engine, group):
    """The first iteration of the reference's own test (-l 700 -j 5k -e 5k -r 12) over the group: the GFA pinned by
    tests/golden/drb1_chain.json, the MAF iteration on device rows equal to the single engine's."""
    gold = json.load(open(os.path.join(HERE, "golden", "drb1_chain.json")))["iterations"][0]
    sm = SM.Smoother(open(DRB1).read(), discover=dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000))
    assert sm.n_blocks == gold["blocks"]
    gfa = iteration_equals(engine, group, sm, 0)
    assert len(gfa) == gold["gfa_bytes"] and hashlib.sha256(gfa.encode()).hexdigest() == gold["sha256"]
    sm.close()


# ---- 7
def test_two_real_devices(base, trims, want_compact):
    if S.load_library().sxg_poa_device_count() < 2:
        pytest.skip("needs a second GPU")
    g = make_group([0, 1])
    try:
        check_compact(g, base, trims, want_compact)
    finally:
        g.close()


def test_bad_arguments_are_refused():
    for devices in ([], [0] * 17, [-1], [0, 4096]):
        with pytest.raises(P.PoaError, match="group"):
            S.PoaGroup(devices)

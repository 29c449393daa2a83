"""GPU, through the C ABI: decree S6' (mode | SXG_IDS_SPOA, 0x20, with SXG_ORDER_SPOA, 0x10) -- the new nodes of a sequence numbered
prefix chain, suffix chain, span -- against the plain-Python reference tests/spoa_ids_ref.py (anchored on the CPU by
tests/test_spoa_ids_ref.py): node codes, ranks, groups, edges, weights, paths and scores bit for bit, the consensus against
helpers.heaviest_bundle_independent run on the reference's arrays.  Every workgroup size the class list builds, the 32-bit and
the banded kernels, global mode, per-block params, the device group, and one DRB1 iteration of the host library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import smoothxg_amd as S
from smoothxg_amd import poa as P
from smoothxg_amd import smooth as SM

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import gfa_invariants as GI  # noqa: E402
import make_class_matrix as M  # noqa: E402
import spoa_ids_cases as K  # noqa: E402
import spoa_ids_ref as R  # noqa: E402
from helpers import PARAM_SETS, gparams, heaviest_bundle_independent  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("node_code", "node_rank", "node_group", "edge_tail", "edge_head", "edge_weight", "scores", "consensus")


def reference(seqs, w, pname, mode, _cache={}):
    """(computed once per block, shared, never changed)"""
    scores = PARAM_SETS[pname] if isinstance(pname, str) else tuple(pname)      # a name of helpers.PARAM_SETS or (m, n, g, e, q, c)
    key = (scores, mode, tuple(s.tobytes() for s in seqs), tuple(int(x) for x in w))
    if key not in _cache:
        p = O.mkparams(*scores, mode=mode)
        _cache[key] = R.run_block(seqs, w, p, ids="spoa" if mode & 0x20 else "sequence")
    return _cache[key]


def assert_equals_reference(res, want, label):
    assert res.status == 0, label
    assert len(res.node_code) == len(want.node_code) and len(res.edge_tail) == len(want.edge_tail), label
    assert (res.scores == want.scores).all(), (label, res.scores, want.scores)
    assert (res.node_code == want.node_code).all() and (res.node_rank == want.node_rank).all() and (res.node_group == want.node_group).all(), label
    assert (res.edge_tail == want.edge_tail).all() and (res.edge_head == want.edge_head).all() and (res.edge_weight == want.edge_weight).all(), label
    assert len(res.paths) == len(want.paths) and all((a == b).all() for a, b in zip(res.paths, want.paths)), label
    if res.consensus is not None:
        cons = heaviest_bundle_independent(want.node_code, want.node_rank, want.edge_tail, want.edge_head, want.edge_weight)
        assert (res.consensus == cons).all(), label


def assert_same(x, y, label):
    """two device results, byte for byte"""
    assert x.status == y.status == 0, label
    for f in FIELDS:
        a, b = getattr(x, f), getattr(y, f)
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (label, f)
    assert len(x.paths) == len(y.paths) and all((a == b).all() for a, b in zip(x.paths, y.paths)), label


HAND = [("anchor",) + K.anchor(), ("prefix",) + K.anchor(True, False), ("suffix",) + K.anchor(False, True),
        ("neither",) + K.anchor(False, False), ("unrelated",) + K.unrelated()]
SEEDED = K.case_set()[:7] + K.case_set()[-1:]      # eight blocks of the CPU case set, one of them with the 30-base insertion


def run(engine, blocks, params, **kw):
    return engine.run_blocks([b[1] for b in blocks], params, weights=[b[2] for b in blocks], want_consensus=True, **kw)


# ---- 1
@pytest.mark.parametrize("pname", K.SCORE_SETS)
def test_device_equals_reference(engine, pname):
    blocks = HAND + SEEDED
    got = run(engine, blocks, gparams(pname, 0x30))
    plain = run(engine, blocks, gparams(pname, 0x10))
    differ = 0
    for (name, seqs, w), res, res10 in zip(blocks, got, plain):
        want = reference(seqs, w, pname, 0x30)
        assert_equals_reference(res, want, (pname, name))
        assert_equals_reference(res10, reference(seqs, w, pname, 0x10), (pname, name, "0x10"))
        differ += int(any((a != b).any() for a, b in zip(res.paths, res10.paths)))
        if name in ("neither", "prefix"):          # nothing behind the span: the flag changes nothing
            assert_same(res, res10, (pname, name))
        if name == "unrelated":                    # an empty walk: one chain in position order
            n = len(res.node_code)
            assert res.scores[2] == 0 and res.paths[2].tolist() == list(range(n - 7, n))
        if name == "anchor" and pname == "convex_default":
            n0 = K.ANCHOR_LEN
            assert res.paths[1][:3].tolist() == [n0, n0 + 1, n0 + 2] and res.paths[1][-3:].tolist() == [n0 + 3, n0 + 4, n0 + 5]
            assert (res.paths[1][15], res.paths[1][26]) == (n0 + 6, n0 + 7)
    assert differ >= 3                             # (the anchor, the suffix block and seeded blocks: not a comparison of equals)


# ---- 2
def class_case(waves):
    """The smallest local-mode block case of tests/golden/class_matrix.json that lands on a workgroup of `waves` wavefronts -- on
    one wave the smallest whose longest sequence exceeds GB x threads = 16 x 64 positions, so that add_alignment's position loops
    wrap there too (4 x 256 and 4 x 512 are below every case of those sizes) -- plus a copy of its last sequence with N tips and a
    mismatch: a walk with a prefix, a suffix and a new node inside the span."""
    import json
    with open(M.FIXTURE) as f:
        cases = [c for c in json.load(f)["cases"] if c["kind"] == "block" and c["mode"] == 0 and c["NW"] == waves]
    if waves == 1:
        cases = [c for c in cases if max(c["seq_lens"]) > 16 * 64]
    case = min(cases, key=lambda c: (sum(c["seq_lens"]), M.case_id(c)))
    seqs = [np.asarray(s, np.uint8) for s in M.case_inputs(case)][:8]
    extra = seqs[-1].copy()
    extra[:5] = 4
    extra[-5:] = 4
    mid = len(extra) // 2
    extra[mid] = (extra[mid] + 1) % 4
    return case, seqs + [extra]


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
def test_every_workgroup_size_runs_the_phase(engine, monkeypatch, waves):
    case, seqs = class_case(waves)
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    for name, on, value in (("SXG_POA_NO_PACKED", case["rm"] != 2 or case.get("no_packed", False), "1"),
                            ("SXG_POA_FORCE_P16", case["force"], "%d,%d" % (case["W"], case["NW"]))):
        if on:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)
    monkeypatch.delenv("SXG_POA_CELL_BYTES", raising=False)
    gb = 16 if waves == 1 else (8 if waves == 2 else 4)      # poa_classes.h: graph_batch of the class
    if waves != 2:
        assert max(len(s) for s in seqs) > gb * 64 * waves      # the position loops wrap
    w = np.ones(len(seqs), np.int64)
    res = engine.run_blocks([seqs], S.Params(*case["params"], 0x30, 0), want_consensus=True)[0]
    st = engine.stats()
    assert st["dom_threads"] == 64 * waves and st["dom_row_mode"] == case["rm"], (M.case_id(case), st)
    want = reference(seqs, w, case["params"], 0x30)
    assert want.spans[-1] == (5, len(seqs[-1]) - 6)
    assert_equals_reference(res, want, M.case_id(case))
    n_old = len(want.node_code) - 11
    assert res.paths[-1][:5].tolist() == list(range(n_old, n_old + 5)) and res.paths[-1][-5:].tolist() == list(range(n_old + 5, n_old + 10))
    assert res.paths[-1][len(seqs[-1]) // 2] == n_old + 10


def test_adaptive_band_path(engine, oracle):
    """banded = 2 (decree B4) under 0x30.  The reference sweeps the full matrix; on these blocks the band does not bind (the oracle's
    banded and full runs agree under 0x10), so the full-matrix reference is the banded one's."""
    blocks = SEEDED[:3] + HAND[:1]
    for name, seqs, w in blocks:
        a = oracle.block_run(seqs, w, oracle.mkparams(*PARAM_SETS["convex_default"], mode=0x10, banded=2))
        b = oracle.block_run(seqs, w, oracle.mkparams(*PARAM_SETS["convex_default"], mode=0x10, banded=0))
        assert (a[1] == b[1]).all() and all((a[0].seq_path(s) == b[0].seq_path(s)).all() for s in range(len(seqs))), name
    m, n, g, e, q, c = PARAM_SETS["convex_default"]
    got = run(engine, blocks, S.Params(m, n, g, e, q, c, 0x30, 2))
    assert engine.stats()["dom_row_mode"] == 3
    for (name, seqs, w), res in zip(blocks, got):
        assert_equals_reference(res, reference(seqs, w, "convex_default", 0x30), ("banded", name))


# ---- 3
def test_global_mode_is_unchanged(engine):
    blocks = HAND + SEEDED
    for x, y, (name, _, _) in zip(run(engine, blocks, gparams("convex_default", 0x31)), run(engine, blocks, gparams("convex_default", 0x11)), blocks):
        assert_same(x, y, name)


def test_ids_without_the_order_are_refused(engine):
    name, seqs, w = HAND[0]
    for mode in (0x20, 0x21):
        with pytest.raises(P.PoaError, match="SXG_IDS_SPOA"):
            engine.run_blocks([seqs], gparams("convex_default", mode))
        bases = np.concatenate(seqs).astype(np.uint8)
        seq_off = np.asarray([0, len(seqs[0]), len(bases)], np.int64)
        bi = engine._mk_in(bases, seq_off, np.asarray([0, 2], np.int32), None, gparams("convex_default", mode), False, False)
        assert engine.lib.sxg_poa_batch_upload(engine.h, C.byref(bi)) == -1      # SXG_E_INVALID
    # per-block params: the check is per block
    with pytest.raises(P.PoaError, match="SXG_IDS_SPOA"):
        engine.run_blocks([seqs, seqs], [gparams("convex_default", 0x30), gparams("convex_default", 0x20)])


def test_per_block_params_mix_flagged_and_unflagged_blocks(engine):
    blocks = HAND[:3] + SEEDED
    modes = [0x30 if b % 2 == 0 else 0x10 for b in range(len(blocks))]
    modes[-1] = 0x31
    got = run(engine, blocks, [gparams("convex_default", m) for m in modes])
    for (name, seqs, w), m, res in zip(blocks, modes, got):
        assert_equals_reference(res, reference(seqs, w, "convex_default", m), (name, hex(m)))


# ---- 4
def test_group_passes_the_flag_through(engine):
    blocks = HAND[:2] + SEEDED[:4]
    g = S.PoaGroup([0, 0])
    try:
        g.set_memory_budget(1 << 30)
        flat = [s for b in blocks for s in b[1]]
        bases = np.concatenate(flat).astype(np.uint8)
        seq_off = np.concatenate([[0], np.cumsum([len(s) for s in flat])]).astype(np.int64)
        blk_off = np.concatenate([[0], np.cumsum([len(b[1]) for b in blocks])]).astype(np.int32)
        w = np.concatenate([b[2] for b in blocks]).astype(np.uint32)
        prm = gparams("convex_default", 0x30)
        got = g.run_flat(bases, seq_off, blk_off, w, prm, want_consensus=True)
        want = engine.run_flat(bases, seq_off, blk_off, w, prm, want_consensus=True)
        assert len(got) == len(want) == 6
        for x, y, b in zip(got, want, blocks):
            assert_same(x, y, b[0])
        assert_equals_reference(got[0], reference(blocks[0][1], blocks[0][2], "convex_default", 0x30), "group, anchor")
    finally:
        g.close()


# ---- 5
class _PoaOf:
    """A device result as test_graph_emul.run_block_graph_emul reads an oracle graph."""

    def __init__(self, res):
        self.res, self.n_seqs = res, len(res.paths)

    def nodes(self):
        return self.res.node_code, self.res.node_rank, self.res.node_group

    def edges(self):
        return self.res.edge_tail, self.res.edge_head, self.res.edge_weight

    def seq_path(self, s):
        return self.res.paths[s]

    def consensus(self):
        return self.res.consensus if self.res.consensus is not None else np.zeros(0, np.int32)


def test_host_chain_with_spoa_ids(engine):
    """One DRB1 iteration (-l 700 -j 5k -e 5k -r 12) with poa_spoa_order = 2: the GFA passes every check of tests/gfa_invariants.py,
    and every block graph the device built equals the block-graph phase's one-thread emulation (poa_bgraph_dev.h through
    tests/csrc/graph_emul.cpp) run on that block's own POA result -- node codes, edges and paths: independent of the id rule."""
    import subprocess
    from test_graph_emul import run_block_graph_emul
    from test_smooth_host import DRB1
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc"), "-s"])
    emul = C.CDLL(os.path.join(HERE, "csrc", "libgraph_emul.so"))
    L = engine.lib
    seen = []

    def run_cb(ctx, pin, pout):
        rc = L.sxg_poa_batch_run(engine.h, pin, pout)
        i = pin.contents
        nb = i.n_blocks
        blk = np.ctypeslib.as_array(i.blk_off, (nb + 1,)).copy()
        ns = int(blk[-1])
        so = np.ctypeslib.as_array(i.seq_off, (ns + 1,)).copy()
        rec = dict(blk=blk, so=so, bases=np.ctypeslib.as_array(i.bases, (int(so[-1]),)).copy(),
                   w=np.ctypeslib.as_array(i.weights, (ns,)).copy() if i.weights else None,
                   params=[S.Params.from_buffer_copy(i.params[b if i.per_block_params else 0]) for b in range(nb)],
                   cons=int(i.want_consensus), visited=int(i.bg_consensus_visited_only), want_bg=int(i.want_block_graph),
                   trim=np.ctypeslib.as_array(i.bg_trim, (nb,)).copy() if i.bg_trim else None)
        if rc == 0:
            rec["own"] = engine._unpack(pout.contents, (blk, so, int(i.want_msa)))
        seen.append(rec)
        return rc

    run_fn, free_fn = SM.RUN_FN(run_cb), SM.FREE_FN(lambda pout: L.sxg_poa_batch_free(pout))
    text = open(DRB1).read()
    sm = SM.Smoother(text, discover=dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000))
    gfa = sm.smooth_gfa(SM.default_params(add_consensus=1, poa_spoa_order=2), (C.cast(run_fn, C.c_void_p), C.cast(free_fn, C.c_void_p), None))
    sm.close()
    GI.check_laced(gfa, text)
    assert seen and all(p.mode == 0x30 for rec in seen for p in rec["params"])
    checked = 0
    for rec in seen:
        assert rec["want_bg"] >= 1 and "own" in rec
        res = engine.run_flat(rec["bases"], rec["so"], rec["blk"], rec["w"], rec["params"], want_consensus=bool(rec["cons"]), block_graph=1,
                              bg_trim=rec["trim"], bg_cons_visited_only=bool(rec["visited"]))
        for b, (r, own) in enumerate(zip(res, rec["own"])):
            assert r.status == 0 and own.status == 0
            seqs = [rec["bases"][rec["so"][s]:rec["so"][s + 1]] for s in range(rec["blk"][b], rec["blk"][b + 1])]
            cons_mode = 0 if not rec["cons"] else (2 if rec["visited"] else 1)
            B = run_block_graph_emul(emul, _PoaOf(r), seqs, int(rec["trim"][b]) if rec["trim"] is not None else 0, cons_mode)
            for dev in (r.bg, own.bg):      # the graph of the re-run and the one the iteration laced
                assert dev.node_seq == B.node_seq and dev.edges == B.edges, b
                assert len(dev.paths) == len(B.paths) and all((x == y).all() for x, y in zip(dev.paths, B.paths)), b
                if cons_mode:
                    assert (np.asarray(dev.consensus) == np.asarray(B.consensus)).all(), b
            checked += 1
    assert checked >= 4

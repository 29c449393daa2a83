"""CPU: the row flags of the packed sweep's twin step (round 13).  prep_rows (smoothxg_amd/csrc/poa_graph_dev.h) is compiled for the
host with a one-thread context -- with the classes' `twin` trait (prep_rows_twin) and without it (prep_rows) -- and run on the
graphs after every sequence of the two small blocks of tests/twin_ref.py (those of tests/test_gpu_twin_rows.py), local and global, in spoa's node order.
Its ROW_TWIN / ROW_JOIN / ROW_STORE and slots are compared with the plain restatement in tests/twin_ref.py on the oracle's
Graph.rows().  A row's last reader lives only inside prep_rows (finish_rows turns it into the slot): it is checked through the
slots, at two on-chip depths (2 and 8 copies), which tell the stored rows between a row and its last reader at two distances.
The product's look-back bound and its join test are also driven directly, on hand-made and random row CSRs (twin_flags_csr).  Without the trait, and with the trait but the knob off, the flags are the old rule's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import twin_ref as T
from twin_ref import block

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
POOL, LDS_ROWS = 64, 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    so = str(tmp_path_factory.mktemp("twin_rows") / "libtwin_rows_check.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-w", "-o", so, os.path.join(HERE, "csrc", "twin_rows_check.cpp"),
                           "-x", "c", os.path.join(ROOT, "oracle", "poa_oracle.c"), os.path.join(ROOT, "oracle", "poa_simd.c")])
    return C.CDLL(so)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def product_rows(lib, seqs, params, trait, twin_on, lds_rows=LDS_ROWS):
    """[(flags, slots, off, pred)] of the graphs after 1 .. len(seqs) - 1 sequences"""
    bases = np.concatenate(seqs).astype(np.uint8)
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    cap = int(off[-1]) * len(seqs) + 64
    n_rows = np.zeros(len(seqs), np.int32)
    rb, pb = np.zeros(len(seqs), np.int64), np.zeros(len(seqs), np.int64)
    fl, sl, po, pr = np.zeros(cap, np.uint8), np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(2 * cap, np.int32)
    st = lib.twin_rows_run(_p(bases, C.c_uint8), _p(off, C.c_int32), len(seqs), C.byref(params), POOL, lds_rows, trait, twin_on,
                           _p(n_rows, C.c_int32), _p(rb, C.c_int64), _p(pb, C.c_int64), _p(fl, C.c_uint8), _p(sl, C.c_int32),
                           _p(po, C.c_int32), _p(pr, C.c_int32))
    assert st == 0
    out = []
    for s in range(1, len(seqs)):
        n = int(n_rows[s])
        o = po[rb[s] + s:rb[s] + s + n + 1]
        out.append((fl[rb[s]:rb[s] + n], sl[rb[s]:rb[s] + n], o, pr[pb[s]:pb[s] + o[n]]))
    return out


_oracle_rows = {}


def oracle_rows(oracle, name, mode):
    """Graph.rows() after every sequence, computed once per (block, mode)."""
    if (name, mode) not in _oracle_rows:
        p = oracle.mkparams(1, -4, -6, -2, -26, -1, mode=mode | 0x10)
        seqs = block(name)
        impl = oracle.IMPL_AVX2 if oracle.simd_available() else oracle.IMPL_SCALAR
        _oracle_rows[(name, mode)] = [oracle.block_run(seqs[:k], None, p, impl=impl)[0].rows() for k in range(1, len(seqs))]
    return _oracle_rows[(name, mode)]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["L", "S"])
def test_flags_and_slots_equal_the_restatement(harness, oracle, name, mode):
    p = oracle.mkparams(1, -4, -6, -2, -26, -1, mode=mode | 0x10)
    got = product_rows(harness, block(name), p, 1, 1)
    n_twin = n_join = n_dropped = 0
    for k, ((flags, slot, off, pred), (_, ooff, opred, osink, _)) in enumerate(zip(got, oracle_rows(oracle, name, mode))):
        assert (off == ooff).all() and (pred == opred).all(), "graph %d: the product's rows are not the oracle's" % k
        f = T.row_flags(ooff, opred)
        assert ((flags & T.ROW_TWIN) != 0).tolist() == f["twin"].tolist(), "graph %d: ROW_TWIN" % k
        assert ((flags & T.ROW_JOIN) != 0).tolist() == f["join"].tolist(), "graph %d: ROW_JOIN" % k
        assert ((flags & T.ROW_STORE) != 0).tolist() == f["stored"].tolist(), "graph %d: ROW_STORE" % k
        assert ((flags & T.ROW_SINK) != 0).tolist() == (osink != 0).tolist() and not (flags & 0xE0).any(), "graph %d: other bits" % k
        assert slot.tolist() == T.slots(f["stored"], f["last"], POOL, LDS_ROWS).tolist(), "graph %d: slots" % k
        # every non-adjacent read: one of the three served cases, or of a stored row
        old = T.row_flags(ooff, opred, new_rule=False)
        assert sorted(f["reads"]) == sorted(old["unserved"])
        for h, x in f["reads"]:
            if (h, x) in set(f["unserved"]):
                assert flags[x] & T.ROW_STORE
            else:
                assert h == x + 2 and ((flags[x + 1] & T.ROW_TWIN) or ((flags[x] & T.ROW_TWIN) and (flags[h] & T.ROW_JOIN)))
        # pairs are disjoint, both rows have the same single predecessor, a join row reads both
        tw = np.flatnonzero(flags & T.ROW_TWIN)
        assert not (np.diff(tw) < 2).any()
        for r in tw:
            assert f["preds"][r] == f["preds"][r + 1] and len(f["preds"][r]) == 1
        n_twin += len(tw)
        n_join += int(f["join"].sum())
        n_dropped += int(old["stored"].sum() - f["stored"].sum())
    assert n_twin > 0 and n_join > 0 and n_dropped > 0


@pytest.mark.parametrize("trait,twin_on", [(0, 0), (1, 0)])
def test_without_the_trait_or_with_the_knob_off_the_old_rule(harness, oracle, trait, twin_on):
    p = oracle.mkparams(1, -4, -6, -2, -26, -1, mode=0x10)
    # (8 on-chip copies here, 2 above: the slots tell a row's last reader by two different distances)
    for (flags, slot, off, pred), (_, ooff, opred, osink, _) in zip(product_rows(harness, block("S"), p, trait, twin_on, lds_rows=8), oracle_rows(oracle, "S", 0)):
        f = T.row_flags(ooff, opred, new_rule=False)
        regpred = np.array([r + 0 in ps for r, ps in enumerate(f["preds"])])   # (row r - 1 is the row number r)
        want = f["stored"] * T.ROW_STORE + (osink != 0) * T.ROW_SINK + regpred * T.ROW_REGPRED
        assert flags.tolist() == want.tolist()
        assert slot.tolist() == T.slots(f["stored"], f["last"], POOL, 8).tolist()


def product_flags_of_csr(lib, preds):
    """twin_flags of the product on a hand-made row CSR (the plain rule's bits set by the harness): the flags per row."""
    off = np.zeros(len(preds) + 1, np.int32)
    off[1:] = np.cumsum([len(p) for p in preds])
    pred = np.array([x for p in preds for x in p] + [0], np.int32)
    flags = np.zeros(len(preds), np.uint8)
    lib.twin_flags_csr(len(preds), _p(off, C.c_int32), _p(pred, C.c_int32), _p(flags, C.c_uint8))
    return flags, off, pred[:off[-1]]


def check_csr(lib, preds):
    flags, off, pred = product_flags_of_csr(lib, preds)
    f = T.row_flags(off, pred)
    assert ((flags & T.ROW_TWIN) != 0).tolist() == f["twin"].tolist(), preds
    assert ((flags & T.ROW_JOIN) != 0).tolist() == f["join"].tolist(), preds
    assert ((flags & T.ROW_STORE) != 0).tolist() == f["stored"].tolist(), preds
    assert not (flags & 0xE0).any()
    return f


@pytest.mark.parametrize("run", [2, 3, 8, 9, 10, 11, 12, 17])
def test_a_long_run_is_paired_up_to_the_bound(harness, run):
    """`run` rows with the same predecessor, then a row that reads the last two of them and the run's predecessor: the product
    pairs rows 1 + 2 .. 7 + 8 of the run and leaves the rows beyond its look-back bound alone, as the restatement does; the
    closing row joins only a pair that exists."""
    preds = [[]] + [[1]] * run + [[run, run + 1, 1]] + [[run + 2]]
    f = check_csr(harness, preds)
    assert np.flatnonzero(f["twin"]).tolist() == [r for r in range(1, run, 2) if r < T.LOOKBACK]
    assert bool(f["join"][run + 1]) == (run % 2 == 0 and run <= T.LOOKBACK)
    # two runs back to back with different predecessors: the second is paired from its own start
    check_csr(harness, [[]] + [[1]] * run + [[2]] * run + [[run + 1]])


def test_random_row_graphs(harness):
    """Row CSRs with many short runs, joins and far readers, drawn at random: product against restatement."""
    rng = np.random.default_rng(1303)
    for _ in range(200):
        n = int(rng.integers(3, 60))
        preds = [[]]
        for r in range(1, n):
            k = rng.random()
            if k < 0.45:
                ps = [r]
            elif k < 0.75 and preds[r - 1] and len(preds[r - 1]) == 1:
                ps = list(preds[r - 1])                       # a sibling of the previous row
            else:
                ps = sorted(set(int(x) for x in rng.integers(max(1, r - 4), r + 1, int(rng.integers(1, 4)))))
            preds.append(ps)
        check_csr(harness, preds)

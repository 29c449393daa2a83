"""CPU: the product's graph code (poa_graph_dev.h: add_alignment under decree S6', mode | SXG_IDS_SPOA, followed by spoa_resort)
compiled for the host with a one-thread context (tests/csrc/graph_emul_ids.cpp) against the plain-Python reference
(tests/spoa_ids_ref.py), in every storage mode of the re-sort the existing harness distinguishes.  The existing harness must
still build from its untouched source."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spoa_ids_cases as K
import spoa_ids_ref as R
from helpers import oparams

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emul_ids(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("graph_emul_ids") / "libgraph_emul_ids.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-fopenmp", "-w", "-o", so,
                           os.path.join(HERE, "csrc", "graph_emul_ids.cpp"), "-x", "c", os.path.join(ROOT, "oracle", "poa_oracle.c"),
                           os.path.join(ROOT, "oracle", "poa_simd.c")])
    return C.CDLL(so)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def run_emul_ids(L, seqs, weights, params, storage, ids_spoa=1):
    bases = np.concatenate(seqs).astype(np.uint8)
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    cap = int(off[-1]) + 8
    cnt = np.zeros(2, np.int32)
    code = np.zeros(cap, np.uint8)
    rank, ld, et, eh, paths = (np.zeros(cap, np.int32) for _ in range(5))
    ew = np.zeros(cap, np.uint32)
    sc = np.zeros(len(seqs), np.int32)
    w = np.asarray(weights, np.uint32)
    st = L.emul_ids_block_run(_p(bases, C.c_uint8), _p(off, C.c_int32), len(seqs), _p(w, C.c_uint32), C.byref(params), storage, ids_spoa,
                              _p(cnt, C.c_int32), _p(code, C.c_uint8), _p(rank, C.c_int32), _p(ld, C.c_int32), _p(et, C.c_int32),
                              _p(eh, C.c_int32), _p(ew, C.c_uint32), _p(paths, C.c_int32), _p(sc, C.c_int32))
    assert st == 0
    n, e = cnt
    return code[:n], rank[:n], ld[:n], et[:e], eh[:e], ew[:e], paths[:off[-1]], sc


def assert_equals_reference(got, want, label):
    code, rank, grp, t, h, w, paths, sc = got
    assert len(code) == len(want.node_code) and len(t) == len(want.edge_tail), label
    assert (code == want.node_code).all() and (rank == want.node_rank).all() and (grp == want.node_group).all(), label
    assert (t == want.edge_tail).all() and (h == want.edge_head).all() and (w == want.edge_weight).all(), label
    assert (paths == np.concatenate(want.paths)).all() and (sc == want.scores).all(), label


@pytest.fixture(scope="module")
def wanted():
    """The reference on every block, score set and mode, computed once and shared by the storage modes."""
    blocks = K.case_set() + [("anchor",) + K.anchor(), ("prefix",) + K.anchor(True, False), ("suffix",) + K.anchor(False, True),
                             ("neither",) + K.anchor(False, False), ("unrelated",) + K.unrelated()]
    out = []
    for pname in K.SCORE_SETS:
        for mode in (0, 1):
            p = oparams(pname, mode)
            p.mode = mode | 0x30
            out += [((pname, mode, name), seqs, w, p, R.run_block(seqs, w, p, ids="spoa")) for name, seqs, w in blocks]
    return out


@pytest.mark.parametrize("storage", [1, 2, 4])
def test_graph_code_under_spoa_ids_matches_the_reference(emul_ids, oracle, wanted, storage):
    """Storage modes of the re-sort (graph_emul.cpp's spoa_order values): 1 = per-node words in scratch once the graph has 16 nodes,
    no static chain named; 2 = words on the chip, the first sequence named as the static chain, pieces kept; 4 = as 2, everything
    rebuilt at every re-sort."""
    for label, seqs, w, p, want in wanted:
        assert_equals_reference(run_emul_ids(emul_ids, seqs, w, p, storage), want, label + (storage,))


def test_flag_off_is_the_oracle(emul_ids, oracle):
    """The same harness without the flag: sequence-order ids, i.e. the oracle under mode | 0x10."""
    p = oparams("convex_default", 0)
    p.mode = 0x10
    for name, seqs, w in K.case_set()[:6]:
        g, sc, _ = oracle.block_run(seqs, w, p)
        got = run_emul_ids(emul_ids, seqs, w, p, 2, ids_spoa=0)
        assert (got[1] == g.nodes()[1]).all() and (got[6] == np.concatenate([g.seq_path(s) for s in range(g.n_seqs)])).all() and (got[7] == sc).all()


def test_existing_harness_still_builds():
    """tests/csrc/graph_emul.cpp calls add_alignment with seven arguments and fills GraphView by position: it must keep compiling
    (the new argument is defaulted and last)."""
    subprocess.check_call(["make", "-C", os.path.join(HERE, "csrc"), "-s"])
    assert os.path.exists(os.path.join(HERE, "csrc", "libgraph_emul.so"))
    # (make skips an up-to-date library: compile the source against the current headers as well, without writing anything)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-fopenmp", "-w", "-fsyntax-only", os.path.join(HERE, "csrc", "graph_emul.cpp")])

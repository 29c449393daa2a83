"""The edge score sets of tests/score_edges.py without a GPU: (a) the reference itself is right on them -- the scalar oracle
equals its own derived-traceback restatement and the independent DAG DP of tests/test_oracle.py; (b) every case names the
sweep the model of the host's choice computes for it, on a built kernel class, and its input REACHES the limit it is said to
sit on -- asserted on the oracle and the model alone, so that tests/test_gpu_score_edges.py cannot pass on an input that
misses its edge; (c) the model agrees with the product's own headers (tests/csrc/score_edges_check.cpp)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import score_edges as E
from helpers import random_block
from score_edges import M
from test_oracle import _dag_dp_score

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK_CASES = E.block_cases()
ALIGN_CASES = E.align_cases()


def _compile(tmp_path_factory, name):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(HERE, "csrc", name + ".cpp")])
    return exe


@pytest.fixture(scope="module")
def built_classes(tmp_path_factory):
    """(kind, rm, cb, tmax, W, sw, ds) of every built kernel class: poa_classes.h's list, printed by tests/csrc/class_list.cpp"""
    out = subprocess.run([_compile(tmp_path_factory, "class_list")], capture_output=True, text=True, check=True)
    return {tuple(map(int, line.split())) for line in out.stdout.splitlines()}


@pytest.fixture(scope="module")
def runs(oracle):
    """the oracle's run of every block case, computed once: id -> (seqs, graph, scores, cells, expected sweep)"""
    out = {}
    for c in BLOCK_CASES:
        seqs = E.case_seqs(c)
        x = E.case_expected(c, seqs)
        key = (c["set"], c["mode"], c["builder"], c["L"], c["seed"], c["tail"], E.oracle_banded(c, x))
        if key not in out:
            g, sc, cells = oracle.block_run(seqs, None, oracle.mkparams(*c["scores"], mode=c["mode"], banded=key[-1]))
            out[key] = (g, sc, cells)
        out[c["id"]] = (seqs,) + out[key] + (x,)
    return out


nodes_before = E.nodes_before


# ---------------------------------------------------------------------------------------------------------------------------
# (a) the reference at the edges

@pytest.mark.parametrize("mode", [0, 1], ids=["local", "global"])
@pytest.mark.parametrize("name", list(E.ALL_SETS))
def test_oracle_equals_the_independent_dag_dp_on_the_edge_sets(oracle, name, mode):
    scores = E.ALL_SETS[name]
    rng = np.random.default_rng(4100 + 2 * list(E.ALL_SETS).index(name) + mode)
    p = oracle.mkparams(*scores, mode=mode)
    for trial in range(4):
        seqs = random_block(rng, int(rng.integers(2, 6)), int(rng.integers(5, 31)), div=0.15)
        g, _, _ = oracle.block_run(seqs[:-1], None, p)
        codes, off, pred, sink, _ = g.rows()
        an, ap, sc = oracle.align_csr(codes, off, pred, sink, seqs[-1], p)
        bn, bp, sc2 = oracle.align_csr(codes, off, pred, sink, seqs[-1], p, vtb=True)
        assert sc == sc2 and (an == bn).all() and (ap == bp).all(), (name, mode, trial)
        assert sc == _dag_dp_score(codes, off, pred, sink, seqs[-1], scores, mode == 0), (name, mode, trial)


def test_the_sets_are_what_the_table_says():
    assert E.model_name(E.EDGE_SETS["top4"]) == "convex" and M.code_bits(E.EDGE_SETS["top4"]) > 16
    assert E.model_name(E.EDGE_SETS["top4a"]) == "affine" and E.model_name(E.EDGE_SETS["lin120"]) == "linear"
    assert E.model_name(E.EDGE_SETS["top2"]) == "convex" and M.code_bits(E.EDGE_SETS["top2"]) <= 16 and E.EDGE_SETS["top2"] != E.DEFAULT
    for name in ("q120", "q121", "g121"):
        # convex: the short piece decides short gaps, the long piece the 40-letter ones (q120 / q121: from 11 columns on)
        s = E.EDGE_SETS[name]
        assert E.model_name(s) == "convex" and M.gap_cost(s, 40) == s[4] + 39 * s[5] and M.gap_cost(s, 2) == s[2] + s[3], name
    q120 = E.EDGE_SETS["q120"]
    assert M.gap_cost(q120, 10) == q120[2] + 9 * q120[3] and M.gap_cost(q120, 12) == q120[4] + 11 * q120[5]
    assert max(abs(v) for v in E.EDGE_SETS["q120"][2:]) == E.BYTE_LIMIT and abs(E.EDGE_SETS["q121"][4]) == E.BYTE_LIMIT + 1
    assert abs(E.EDGE_SETS["g121"][2]) == E.BYTE_LIMIT + 1 and E.EDGE_SETS["g121"][4] == -128
    assert {k: E.model_name(v) for k, v in E.BORDER_SETS.items()} == E.BORDER_MODELS
    # each field of the default set moved by one, both ways, except where the sign convention ends (c = -1 + 1 = 0 is valid)
    assert len(E.NEAR_DEFAULT_SETS) == 12 and E.DEFAULT not in E.NEAR_DEFAULT_SETS.values()
    assert all(sum(abs(a - b) for a, b in zip(s, E.DEFAULT)) == 1 for s in E.NEAR_DEFAULT_SETS.values())
    # no near-default set is the DS class's (expected_block: ds needs the default set itself)
    assert E.expected_block(E.DEFAULT, 0, 300)["ds"] == 1
    assert all(E.expected_block(s, mode, 300)["ds"] == 0 for s in E.NEAR_DEFAULT_SETS.values() for mode in (0, 1))
    assert all(E.expected_block(s, mode, 345)["rm"] == 2 for s in list(E.NEAR_DEFAULT_SETS.values()) + list(E.BORDER_SETS.values()) for mode in (0, 1))


# ---------------------------------------------------------------------------------------------------------------------------
# (b) the cases name the model's sweep and reach their limits

@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c["id"] for c in BLOCK_CASES])
def test_block_case_names_its_sweep_and_reaches_its_limit(oracle, runs, built_classes, case):
    seqs, g, sc, cells, x = runs[case["id"]]
    m = case["scores"][0]
    maxlen = max(len(s) for s in seqs)
    sw = case["mode"] == 0
    assert (x["rm"], x["cb"], (x["W"], x["NW"])) == (case["rm"], case["cb"], case["geometry"]), x
    assert (0, x["rm"], x["cb"], x["tmax"], x["W"], int(sw), x["ds"]) in built_classes, x
    assert x["ds"] == 0 and any(4 in s for s in seqs) and (maxlen == case["L"] or case["builder"] == "indel")
    edge = case["edge"]
    if edge == "local_at":
        assert m * maxlen < E.LOCAL_LIMIT and int(sc.max()) >= E.LOCAL_LIMIT - m, (maxlen, sc)
    elif edge == "local_past":
        assert m * maxlen >= E.LOCAL_LIMIT and int(sc.max()) > E.LOCAL_LIMIT, (maxlen, sc)
        if case["L"] == 511:
            assert int(sc.max()) > 60000        # beyond 16 bits with room to spare: a word that still holds 16 shows
        else:
            assert m * (maxlen - 1) < E.LOCAL_LIMIT, "one letter past, no more"
    elif edge == "byte":
        top = max(abs(case["scores"][2]), abs(case["scores"][4]))
        assert top == E.BYTE_LIMIT if case["set"] == "q120" else top > E.BYTE_LIMIT
        assert m * maxlen + m < E.CLAMP_LIMIT and E.global_floor(case["scores"], maxlen, 2 * maxlen) < E.LOCAL_LIMIT   # nothing else decides
    elif edge in ("clamp", "clamp_rerun"):
        top = m * maxlen + m
        assert (E.CLAMP_LIMIT - m <= top < E.CLAMP_LIMIT) if case["rm"] == 2 else (E.CLAMP_LIMIT <= top < E.CLAMP_LIMIT + m), top
        thr = [-16000 + m * len(s) + m for s in seqs]      # poa_dp16.hip.h: a walk through a cell at or below it is re-run
        if case["builder"] == "clean":
            # the walk of the second sequence stays above -5 (m - n) >= thr, the short one's above its all-gap path
            assert -5 * (m - case["scores"][1]) > thr[1] and -E.global_floor(case["scores"], 10, g.n_nodes) - 10 * m > thr[-1]
            assert all(int(sc[k]) > thr[k] for k in range(1, len(seqs)))
        if edge == "clamp_rerun":
            assert int(sc[2]) <= thr[2], "the unrelated sequence ends at or below the clamp threshold: a re-run is certain"
            assert E.next_step(case["scores"], 1, maxlen, 2) == 0
    elif edge in ("recheck_fires", "recheck_quiet", "strict_recheck"):
        limit = E.STRICT_LIMIT if edge == "strict_recheck" else E.LOCAL_LIMIT
        before = nodes_before(oracle, case, seqs)
        floors = [E.global_floor(case["scores"], len(s), n) for s, n in zip(seqs, before)]
        assert E.global_floor(case["scores"], maxlen, maxlen) < limit, "the host, on its own row count, admits the block"
        if edge == "recheck_quiet":
            assert max(before) < 128 and max(floors[1:]) < limit, (before, floors)
        else:
            # ... and the true row count does not: in front of the third sequence
            assert floors[1] < limit <= floors[2] and (edge != "recheck_fires" or before[2] >= 128), (before, floors)
    elif edge == "h16_past":
        assert E.LOCAL_LIMIT <= E.global_floor(case["scores"], maxlen, maxlen) < E.LOCAL_LIMIT + 128 and m * maxlen < E.LOCAL_LIMIT
    else:
        raise AssertionError("a case without an edge: " + case["id"])


def test_the_ladders_of_the_cases(oracle, runs):
    """what the GPU test expects of the re-runs, from the oracle's row counts alone"""
    want = {"e/lin121/divergent/L120": [0, 1], "e/lin121/near/L120": [0], "e/lin121/near/L124": [1], "f/lin120/global/L65/band2": [3, 0],
            "d/lin120/disjoint/L113": [2, 0], "d/top4/clean/L113": [2], "d/top4/clean/L114": [0], "d/top4/divergent/L113": [(2, None)],
            "d/top4/divergent/L114": [0]}
    for c in BLOCK_CASES:
        seqs = runs[c["id"]][0]
        ladder = E.expected_ladder(c, seqs, nodes_before(oracle, c, seqs))
        assert ladder == want.get(c["id"], [c["rm"]]), (c["id"], ladder)


def test_every_section_has_its_cases():
    ids = [c["id"] for c in BLOCK_CASES]
    assert [sum(1 for i in ids if i.startswith(s + "/")) for s in "abcdef"] == [19, 5, 16, 5, 3, 9]
    assert {c["env"].get("SXG_POA_FORCE_P16") for c in BLOCK_CASES if c["id"].startswith("a/")} == {None} | set(E.FORCED)
    assert all(not c["env"] for c in BLOCK_CASES if c["id"][0] in "bdef"), "one past, thresholds, re-check, band: no knob"
    assert all(not c["env"] for c in BLOCK_CASES if c["set"] in ("q121", "g121"))


@pytest.mark.parametrize("case", ALIGN_CASES, ids=[c["id"] for c in ALIGN_CASES])
def test_align_case_names_its_sweep_and_reaches_its_limit(oracle, built_classes, case):
    scores = E.EDGE_SETS[case["set"]]
    m = scores[0]
    codes, off, pred, sink, q = E.align_problem(case, oracle)
    x = E.expected_align(scores, case["mode"], len(q), len(codes))
    assert x["rm"] == case["rm"] and (1, x["rm"], 4, x["tmax"], x["W"], 1 - case["mode"], 0) in built_classes, x
    _, _, sc = oracle.align_csr(codes, off, pred, sink, q, oracle.mkparams(*scores, mode=case["mode"]))
    floor = E.global_floor(scores, len(q), len(codes))
    edge = case["edge"]
    if edge == "local_at":
        assert m * len(q) < E.LOCAL_LIMIT and sc == m * len(q) >= E.LOCAL_LIMIT - m
    elif edge == "local_past":
        assert m * (len(q) - 1) < E.LOCAL_LIMIT <= m * len(q) == sc
    elif edge == "strict_at":
        assert m * len(q) < E.STRICT_LIMIT and floor < E.STRICT_LIMIT
        assert m * (len(q) + 1) >= E.STRICT_LIMIT or E.global_floor(scores, len(q) + 1, len(codes)) >= E.STRICT_LIMIT
    elif edge == "strict_past":
        assert (m * len(q) >= E.STRICT_LIMIT) != (floor >= E.STRICT_LIMIT), "exactly one half of the rule fails"
        assert m * (len(q) - 1) < E.STRICT_LIMIT and E.global_floor(scores, len(q) - 1, len(codes)) < E.STRICT_LIMIT
    else:
        assert edge == "byte" and (max(abs(scores[2]), abs(scores[4])) == E.BYTE_LIMIT) == (case["rm"] == 2)
        assert m * len(q) < E.STRICT_LIMIT and floor < E.STRICT_LIMIT


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the model agrees with the code

def test_the_model_agrees_with_the_product_headers(oracle, tmp_path_factory):
    exe = _compile(tmp_path_factory, "score_edges_check")
    asked = []      # (label, normalised scores + convex, sw, maxlen, rm, cb, force, expected (fits16, def, W, NW, tmax))

    def ask(label, scores, sw, maxlen, rm, cb, force, x):
        norm = M.normalise(scores)
        fits = int(M.code_bits(scores) <= 16)
        asked.append((label, norm, sw, maxlen, rm, cb, force, (fits, int(tuple(scores) == E.DEFAULT), x["W"], x["NW"], x["tmax"])))

    for c in BLOCK_CASES:
        seqs = E.case_seqs(c)
        x = E.case_expected(c, seqs)
        force = tuple(int(v) for v in c["env"].get("SXG_POA_FORCE_P16", "0,0").split(","))
        ask(c["id"], c["scores"], c["mode"] == 0, max(len(s) for s in seqs), x["rm"], x["cb"], (x["W"], 1) if x["rm"] == 3 else force, x)
    for c in ALIGN_CASES:
        codes, _, _, _, q = E.align_problem(c, oracle)
        x = E.expected_align(E.EDGE_SETS[c["set"]], c["mode"], len(q), len(codes))
        ask(c["id"], E.EDGE_SETS[c["set"]], c["mode"] == 0, len(q), x["rm"], 4, (0, 0), x)
    for name, scores in list(E.ALL_SETS.items()) + [("default", E.DEFAULT)]:
        for mode in (0, 1):
            for L in (236, 237, 345, 1034, 1035):
                x = E.expected_block(scores, mode, L)
                ask("%s/%d/%d" % (name, mode, L), scores, mode == 0, L, x["rm"], x["cb"], (0, 0), x)
    text = "".join("%d %d %d %d %d %d %d %d %d %d %d %d %d\n" % (n[:6] + (int(n[6]), int(sw), L, rm, cb) + tuple(f)) for _, n, sw, L, rm, cb, f, _ in asked)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    # the constants the model writes down a second time
    assert out[0].split() == ["consts", str(E.LOCAL_LIMIT), "1024", "13", str(1024 + E.LOCAL_LIMIT - 1 + 12 * 120)], out[0]
    assert 1024 + E.LOCAL_LIMIT - 1 + 12 * 120 <= 32767, "lin120 on the widest strip: the top field stays a positive int16"
    assert len(out) == len(asked) + 1
    for (label, *_, want), line in zip(asked, out[1:]):
        assert tuple(map(int, line.split())) == want, (label, line, want)
    assert sum(1 for a in asked if a[-1][1]) == 10 and {a[-1][0] for a in asked} == {0, 1}

"""MI355X: score sets at the edge of every sweep's admitted range (tests/score_edges.py has the cases and says which rule each
sits on; tests/test_score_edges.py holds, without a GPU, that every input reaches its limit).  The kernels rest on the host's
admission rules with no run-time check, so a kernel that is wrong at an edge returns wrong scores with status OK: every block
and every align-only problem here is compared with the LIVE scalar oracle, bit for bit, and every test NAMES the sweep it ran
on -- row mode, threads, columns per lane, retries and launches from the statistics, class (tmax, cb, ds) from the
SXG_POA_DEBUG variant line -- so that a case that quietly ran on another class fails."""
import os

import numpy as np
import pytest

import score_edges as E
from helpers import assert_block_equal, random_block
from smoothxg_amd import Params
from test_gpu_class_matrix import VARIANT_LINE

pytestmark = pytest.mark.gpu

BLOCK_CASES = E.block_cases()
ALIGN_CASES = E.align_cases()
KNOBS = ("SXG_POA_NO_PACKED", "SXG_POA_CELL_BYTES", "SXG_POA_FORCE_P16")
_oracle_runs = {}


def set_env(monkeypatch, env):
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    for k in KNOBS:
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)


def launches(err):
    """one dict per variant line of the engine's debug output, in launch order"""
    keys = ("T", "W", "cvx", "rm", "attempt", "tmax", "cb", "ds", "w2")
    return [dict(zip(keys, map(int, g))) for g in VARIANT_LINE.findall(err)]


def oracle_block(oracle, seqs, scores, mode, banded, key, weights=None):
    """the live scalar oracle, once per distinct (input, scores, mode, band)"""
    if key not in _oracle_runs:
        _oracle_runs[key] = oracle.block_run(seqs, weights, oracle.mkparams(*scores, mode=mode, banded=banded), impl=oracle.IMPL_SCALAR)
    return _oracle_runs[key]


# ---------------------------------------------------------------------------------------------------------------------------
# a .. f: one block per case

@pytest.mark.parametrize("case", BLOCK_CASES, ids=[c["id"] for c in BLOCK_CASES])
def test_block_at_the_edge(engine, oracle, monkeypatch, capfd, case):
    seqs = E.case_seqs(case)
    x = E.case_expected(case, seqs)
    assert (x["rm"], x["cb"], (x["W"], x["NW"])) == (case["rm"], case["cb"], case["geometry"])
    # the knobbed re-runs in the incrementally kept node order, everything else in spoa's (the product's default)
    mode = case["mode"] | (0 if case["env"] else 0x10)
    ob = E.oracle_banded(case, x)
    g, sc, cells = oracle_block(oracle, seqs, case["scores"], mode, ob, (case["set"], mode, case["builder"], case["L"], case["seed"], case["tail"], ob))
    ladder = E.expected_ladder(case, seqs, E.nodes_before(oracle, case, seqs))
    set_env(monkeypatch, case["env"])
    capfd.readouterr()
    res = engine.run_blocks([seqs], Params(*case["scores"], mode, case["banded"]), want_consensus=True)[0]
    st = engine.stats()
    ran = launches(capfd.readouterr().err)
    print(case["id"], "scores", res.scores.tolist(), "oracle", sc.tolist(), "launches", ran, "retries", st["retries"])
    assert_block_equal(res, g, sc, cells, label=case["id"])
    assert (res.consensus == g.consensus()).all(), case["id"]
    # the first launch: the class the case names
    assert ran, "no variant line"
    first = ran[0]
    assert (first["rm"], first["T"], first["W"], first["attempt"]) == (x["rm"], x["threads"], x["W"], 0), (case["id"], ran)
    assert (first["tmax"], first["cb"], first["ds"]) == (x["tmax"], x["cb"], 0), (case["id"], ran)
    assert first["cvx"] == int(E.M.normalise(case["scores"])[6]), (case["id"], ran)
    # the re-runs: the ladder the model computes from the oracle's row counts
    if ladder[-1] == (2, None):      # a packed global walk that may or may not visit a clamped cell: both are right, each is named
        ladder = [2] if len(ran) == 1 else [2] + E.expected_ladder(dict(case, env={"SXG_POA_NO_PACKED": "1"}), seqs, E.nodes_before(oracle, case, seqs))
    assert [r["rm"] for r in ran] == ladder and [r["attempt"] for r in ran] == list(range(len(ladder))), (case["id"], ran, ladder)
    assert st["retries"] == len(ladder) - 1 and st["dp_launches"] == len(ladder), (case["id"], st)
    if case["edge"] in ("recheck_fires", "strict_recheck", "clamp_rerun"):
        assert st["retries"] >= 1, case["id"]
    last = (x["threads"], x["cols_per_lane"]) if len(ladder) == 1 else E.final_geometry(case, seqs, ladder[-1])
    assert (st["dom_row_mode"], st["dom_threads"], st["dom_cols_per_lane"]) == (ladder[-1],) + last, (case["id"], st)


# ---------------------------------------------------------------------------------------------------------------------------
# g: gap-model borders and near-default sets, one batch with per_block_params

def _border_batch(names):
    blocks, prm, tags = [], [], []
    for k, name in enumerate(names):
        for mode in (0, 1):
            seqs = E.indel_block(300, 5200 + k % 4)
            blocks.append(seqs)
            prm.append((E.ALL_SETS.get(name, E.DEFAULT), mode | 0x10))
            tags.append(("g", name, mode, k % 4))
    return blocks, prm, tags


def _run_batch(engine, oracle, monkeypatch, capfd, blocks, prm, tags, env, rm, ds):
    set_env(monkeypatch, env)
    capfd.readouterr()
    res = engine.run_blocks(blocks, [Params(*s, mode, 0) for s, mode in prm], want_consensus=True)
    st = engine.stats()
    ran = launches(capfd.readouterr().err)
    for b, (seqs, (scores, mode), tag) in enumerate(zip(blocks, prm, tags)):
        g, sc, cells = oracle_block(oracle, seqs, scores, mode, 0, tag)
        assert_block_equal(res[b], g, sc, cells, label="%s %s" % (tag, env))
        assert (res[b].consensus == g.consensus()).all(), tag
    assert ran and all((r["rm"], r["attempt"], r["ds"]) == (rm, 0, ds) for r in ran), ran
    assert st["retries"] == 0 and st["dp_launches"] == len(ran) and st["dom_row_mode"] == rm and st["dom_threads"] == 64, st
    # 341-odd letters: one wave of 4 packed columns (8 per lane) or of 8 columns of a 32-bit sweep
    assert all((r["T"], r["W"]) == (64, 4 if rm == 2 else 8) for r in ran) and st["dom_cols_per_lane"] == 8, (ran, st)
    return ran


@pytest.mark.parametrize("sweep", ["packed", "no_packed"])
def test_gap_model_borders_and_near_default_sets(engine, oracle, monkeypatch, capfd, sweep):
    blocks, prm, tags = _border_batch(list(E.BORDER_SETS) + list(E.NEAR_DEFAULT_SETS))
    assert len(blocks) == 32 and all(E.expected_block(s, m & 1, max(len(x) for x in b))["rm"] == 2 for b, (s, m) in zip(blocks, prm))
    env = {} if sweep == "packed" else {"SXG_POA_NO_PACKED": "1"}
    ran = _run_batch(engine, oracle, monkeypatch, capfd, blocks, prm, tags, env, 2 if sweep == "packed" else 0, 0)
    # linear, affine and convex sets are in the batch: both gap models of the class ran
    assert {r["cvx"] for r in ran} == {0, 1}


def test_near_default_sets_run_the_generic_class_and_the_default_set_its_own(engine, oracle, monkeypatch, capfd):
    blocks, prm, tags = _border_batch(list(E.NEAR_DEFAULT_SETS))
    ran = _run_batch(engine, oracle, monkeypatch, capfd, blocks, prm, tags, {}, 2, 0)
    assert all(r["cb"] == 2 for r in ran)                     # (every near-default set takes the 2-byte cells the DS class has)
    blocks, prm, tags = _border_batch(["default"])
    assert [s for s, _ in prm] == [E.DEFAULT, E.DEFAULT]
    ran = _run_batch(engine, oracle, monkeypatch, capfd, blocks, prm, tags, {}, 2, 1)
    assert all((r["cb"], r["cvx"]) == (2, 1) for r in ran)


# ---------------------------------------------------------------------------------------------------------------------------
# h: the align-only API

@pytest.mark.parametrize("case", ALIGN_CASES, ids=[c["id"] for c in ALIGN_CASES])
def test_align_only_at_the_edge(engine, oracle, monkeypatch, capfd, case):
    scores = E.EDGE_SETS[case["set"]]
    codes, off, pred, sink, q = E.align_problem(case, oracle)
    x = E.expected_align(scores, case["mode"], len(q), len(codes))
    assert x["rm"] == case["rm"]
    an, ap, sc = oracle.align_csr(codes, off, pred, sink, q, oracle.mkparams(*scores, mode=case["mode"]))
    set_env(monkeypatch, {})
    capfd.readouterr()
    (rows, pos, score, status), = engine.align([(codes, off, pred, sink, q)], Params(*scores, case["mode"], 0))
    st = engine.stats()
    ran = launches(capfd.readouterr().err)
    print(case["id"], status, score, sc, len(rows), len(an), ran)
    assert status == 0 and score == sc, (case["id"], status, score, sc)
    assert len(rows) == len(an) and (np.asarray(rows) == an).all() and (np.asarray(pos) == ap).all(), case["id"]
    assert len(ran) == 1 and st["retries"] == 0 and st["dp_launches"] == 1, (case["id"], ran, st)
    assert (st["dom_row_mode"], st["dom_threads"], st["dom_cols_per_lane"]) == (x["rm"], x["threads"], x["cols_per_lane"]), (case["id"], st)
    r = ran[0]
    assert (r["rm"], r["T"], r["W"], r["attempt"], r["tmax"], r["cb"], r["ds"]) == (x["rm"], x["threads"], x["W"], 0, x["tmax"], 4, 0), (case["id"], ran)


# ---------------------------------------------------------------------------------------------------------------------------
# i: a campaign over the whole int8 domain

# SXG_FUZZ_WIDE=<n>: more seeds (the default four cost a few seconds each)
@pytest.mark.parametrize("seed", [9701 + k for k in range(int(os.environ.get("SXG_FUZZ_WIDE", "4")))])
def test_random_blocks_full_score_domain(engine, seed):
    """The shape of test_gpu_fuzz.py's campaign -- 36 blocks per seed, per_block_params, weights, every fourth block with Ns, the
    node order drawn per block -- with scores from the whole valid domain (score_edges.random_scores_full) and lengths around
    the limits a large m brings down to a few hundred letters.  No assertion on the sweep: equality with the oracle."""
    from oracle import oracle_py as O
    rng = np.random.default_rng(seed)
    blocks, weights, gp, op = [], [], [], []
    for trial in range(36):
        L = int(rng.choice([1, 3, 17, 60, 120, 236, 237, 400, 600]))
        L = max(1, L + int(rng.integers(-(L // 4), L // 4 + 1)))
        seqs = random_block(rng, int(rng.integers(1, 9)), L, div=float(rng.choice([0.01, 0.05, 0.15])), alphabet=5 if trial % 4 == 0 else 4)
        if trial % 6 == 0 and L > 40:   # a structural variant: one sequence loses a piece, one gains one
            seqs.append(np.concatenate([seqs[0][:L // 3], seqs[0][L // 3 + L // 8:]]))
            seqs.append(np.concatenate([seqs[0][:L // 2], rng.integers(0, 4, L // 10 + 1, dtype=np.uint8), seqs[0][L // 2:]]))
        m, n, g, e, q, c = E.random_scores_full(rng)
        mode = int(rng.integers(0, 2))
        banded = int(rng.integers(0, 3)) if mode == 0 else 0
        if mode == 1 and L <= 300 and trial % 2 == 1:
            banded = 2   # abPOA's band in global mode: here a score set may well leave the packed range, and the band with it
        mode |= 0x10 if int(rng.integers(0, 3)) else 0
        blocks.append(seqs)
        weights.append(rng.integers(1, 6, len(seqs)).astype(np.uint32))
        gp.append(Params(m, n, g, e, q, c, mode, banded))
        op.append((m, n, g, e, q, c, mode, banded))
    res = engine.run_blocks(blocks, gp, weights=weights, want_consensus=True)
    for b, (seqs, w) in enumerate(zip(blocks, weights)):
        m, n, g, e, q, c, mode, banded = op[b]
        label = f"wide{seed}/block{b} L={len(seqs[0])} S={len(seqs)} scores=({m},{n},{g},{e},{q},{c}) mode={mode} banded={banded}"
        # The band flag counts where the engine runs the banded kernel: a local alignment, or the adaptive band,
        # inside the packed range under the strict rule.  Anywhere else the full matrix runs, and a global block that leaves
        # the range while its graph grows is re-run on the full matrix.  Decided by the model, before the result is looked at.
        scores = (m, n, g, e, q, c)
        if banded and E.expected_block(scores, mode & 1, max(len(s) for s in seqs), banded)["rm"] != 3:
            banded = 0
        if banded and mode & 1:
            before = E.nodes_before(O, dict(scores=scores, mode=1), seqs)
            if any(E.global_floor(scores, len(s), k) >= E.STRICT_LIMIT for s, k in zip(seqs[1:], before[1:])):
                banded = 0
        g_, sc, cells = O.block_run(seqs, w, O.mkparams(m, n, g, e, q, c, mode=mode, banded=banded))
        assert_block_equal(res[b], g_, sc, cells, label=label)
        assert (res[b].consensus == g_.consensus()).all(), label


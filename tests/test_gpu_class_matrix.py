"""Every built kernel class against committed oracle output (tests/golden/class_matrix.json, class_matrix_wide.json and class_matrix_banded.json, made by
tests/golden/make_class_matrix.py -- see its docstring for the inputs and the families): one block, or one align-only problem,
per class, with sequences that fill the class's geometry to within three letters, so that the carry scans across strips, the
wave-to-wave hand-over, the stored-row read-back, the compiled-in thread count, the T < TMAX launch of the 4-byte classes and
the plane's strip bookkeeping all run with every wave at work.  No oracle runs here.

Per case: scores, cells, node / edge counts and digests equal the fixture; the engine's statistics name the expected geometry
(threads, columns per lane, row mode); the SXG_POA_DEBUG variant line names the expected class (tmax, cb, ds, w2); there is
exactly one variant line and no retry, so no step of a ladder quietly repaired a wrong sweep on another class.

Re-runs at no fixture cost (results do not depend on the geometry):
  * W = 9 .. 12 at 4 and 8 waves: the (W - 1, NW) block under SXG_POA_FORCE_P16=W,NW -- every sweep at the second width W2 = W - 1;
    the natural (W, NW) case of such a class sweeps its longest sequence at W (both from the width counters);
  * the (12,8) blocks under SXG_POA_FORCE_P16=8,12: the 768-thread launch of the 1 024-thread class, which the chooser never picks;
  * gen2_affine's blocks under SXG_POA_CELL_BYTES=4 (family cb4_affine): the affine 4-byte classes;
  * the longest packed global align-only query under the wider forced geometries (make_class_matrix.ALIGN_GLOBAL_FORCED);
  * the banded sweep's local 2-byte cases under SXG_POA_BAND_CELL_BYTES=4: the 4-byte local kernels, of which the affine ones
    are reachable through the knob only (the argument of cb4_affine).

The banded sweep (kind "band", row mode 3): one block per strip width W = 6, 8, 11 whose band fills the one-wave window, per band
mode, alignment mode and gap model -- the variant line must name W (which holds the product's band_strip_width, a HIP header's,
equal to the model's and the oracle's at the lengths where it changes), tmax 64, the band cell bytes, ds 0 and the gap model,
which is what tells the two kernels of a class line apart."""
import os
import re
import sys

import numpy as np
import pytest

from smoothxg_amd import Params

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_class_matrix as M  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = M.load_cases()
VARIANT_LINE = re.compile(r"^\[sxg\] variant T=(\d+) W=(\d+) cvx=(\d+) rowmode=(\d+) attempt=(\d+) .* tmax=(\d+) cb=(\d+) ds=(\d+) w2=(\d+)$", re.M)
PACKED_FAMILIES = M.BLOCK_FAMILIES + ("cb4_affine",)


def cases_of(kind, family, mode, **where):
    family = "gen2_affine" if family == "cb4_affine" else family
    return [c for c in CASES if c["kind"] == kind and c["family"] == family and c["mode"] == mode and all(c[k] == v for k, v in where.items())]


def set_env(monkeypatch, case, knob4=False, force=None):
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    # (a 32-bit case takes the knob unless it says that its scores reach the sweep by themselves: no_packed = False)
    for name, on, value in (("SXG_POA_NO_PACKED", case.get("no_packed", case["rm"] != 2), "1"), ("SXG_POA_CELL_BYTES", knob4, "4"),
                            ("SXG_POA_FORCE_P16", force or case["force"], "%d,%d" % (force or (case["W"], case["NW"])))):
        if on:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)


def check_launch(st, err, case, cls, geometry, w2, label):
    """the statistics' geometry, the one variant line's class, no retry"""
    W, NW = geometry
    _, rm, cb, tmax, _, _, ds = cls
    assert (st["dom_threads"], st["dom_cols_per_lane"], st["dom_row_mode"]) == (64 * NW, W * (2 if rm == 2 else 1), rm), (label, st)
    lines = VARIANT_LINE.findall(err)
    assert len(lines) == 1, (label, lines, [x for x in err.splitlines() if "round" in x])
    T, lw, cvx, lrm, attempt, ltmax, lcb, lds, lw2 = map(int, lines[0])
    assert (T, lw, lrm, attempt) == (64 * NW, W, rm, 0), (label, lines)
    assert cvx == int(M.normalise(tuple(case["params"]))[6]), (label, lines)
    assert (ltmax, lcb, lds, lw2) == (tmax, cb, ds, w2), (label, lines)
    assert st["retries"] == 0 and st["dp_launches"] == 1, (label, st)


def run_block(engine, monkeypatch, capfd, case, knob4=False, force=None):
    """One run_blocks call of a case's block (force: re-run on that packed geometry); returns the statistics."""
    label = M.case_id(case) + ("+cb4" if knob4 else "") + ("+force%d,%d" % force if force else "")
    set_env(monkeypatch, case, knob4, force)
    seqs = M.case_inputs(case)
    assert [len(s) for s in seqs] == case["seq_lens"], label
    capfd.readouterr()
    res = engine.run_blocks([seqs], Params(*case["params"], case["mode"] | 0x10, 0))[0]
    st = engine.stats()
    err = capfd.readouterr().err
    assert res.status == 0, (label, res.status)
    got = {"scores": [int(x) for x in res.scores], "cells": int(res.cells.sum()), "n_nodes": int(len(res.node_code)), "n_edges": int(len(res.edge_tail)),
           "digests": M.digest_block(res.node_code, res.node_rank, res.node_group, res.edge_tail, res.edge_head, res.edge_weight, res.paths)}
    print(label, got["scores"], got["cells"], got["n_nodes"], got["n_edges"], st["width_sweeps"], st["hint_shift_repeats"], st["retries"])
    for k, v in got.items():
        assert v == case[k], (label, k, v, case[k])
    cls = M.case_class(case, knob4, force)
    geometry = force or (case["W"], case["NW"])
    w2 = M.second_width(geometry[0], geometry[1], cls[2]) if case["rm"] == 2 else 0
    check_launch(st, err, case, cls, geometry, w2, label)
    if case["rm"] == 2:
        # every alignment (the first sequence founds the graph) is one sweep, at the narrowest of W2 and W that covers it
        T = 64 * geometry[1]
        narrow = sum(1 for n in case["seq_lens"][1:] if w2 and n + 1 <= T * 2 * w2)
        wide = len(case["seq_lens"]) - 1 - narrow
        assert st["hint_shift_repeats"] == 0 and (st["dom_width"], st["dom_width2"]) == (geometry[0], w2), (label, st)
        assert tuple(st["width_sweeps"]) == (wide, narrow), (label, st)
        assert tuple(st["width_swept_cols"]) == (wide * T * 2 * geometry[0], narrow * T * 2 * w2), (label, st)
        if force and w2 and not knob4 and force[1] == case["NW"]:
            assert (wide, narrow) == (0, 2), label          # the (W - 1, NW) block: every sweep at W2
        elif w2 and not force and int(np.argmax(case["seq_lens"])) > 0:
            assert wide >= 1, label                          # the natural case: the longest sequence at W
    return st


# (no packed global class of 16 waves is reachable with a full geometry: a global block stays packed up to 14 498 letters)
PACKED_CASES = [(f, m, w) for f in PACKED_FAMILIES for m in (0, 1) for w in (1, 2, 3, 4, 8, 16) if (m, w) != (1, 16)]


@pytest.mark.parametrize("family,mode,waves", PACKED_CASES, ids=["%s-%s-%dw" % (f, ("local", "global")[m], w) for f, m, w in PACKED_CASES])
def test_packed_block_classes(engine, monkeypatch, capfd, family, mode, waves):
    knob4 = family == "cb4_affine"
    cases = cases_of("block", family, mode, rm=2, NW=waves)
    widths = {c["W"]: c for c in cases}
    assert sorted(widths) == list({1: range(4, 13), 2: range(4, 13), 3: range(4, 13), 4: range(4, 13), 8: range(8, 13), 16: (8, 10, 12, 13)}[waves])
    for c in cases:
        run_block(engine, monkeypatch, capfd, c, knob4)
    if waves in (4, 8) and family not in ("cb4_convex", "cb4_affine"):
        for W in (9, 10, 11, 12):
            run_block(engine, monkeypatch, capfd, widths[W - 1], force=(W, waves))
    if waves == 8 and family in M.FORCED_768_FAMILIES:
        st = run_block(engine, monkeypatch, capfd, widths[12], force=(8, 12))
        assert st["dom_threads"] == 768


# (wide_match: int32 row words with no knob set, every geometry; split by wave count to keep each function short)
WIDE_WAVES = {"few": (1, 2, 3, 4), "many": (8, 12, 16)}
BLOCK32 = [("ds", 0, None), ("ds", 1, None), ("convex_heavy", 0, None)] + [("wide_match", m, w) for m in (0, 1) for w in WIDE_WAVES]
BLOCK32_IDS = ["int16-local", "int16-global", "int32-local"] + ["int32-wide-%s-%s-waves" % (("local", "global")[m], w) for m in (0, 1) for w in WIDE_WAVES]


@pytest.mark.parametrize("family,mode,waves", BLOCK32, ids=BLOCK32_IDS)
def test_32_bit_block_classes(engine, monkeypatch, capfd, family, mode, waves):
    cases = [c for c in cases_of("block", family, mode) if c["rm"] != 2 and (waves is None or c["NW"] in WIDE_WAVES[waves])]
    if family == "wide_match":
        assert sorted((c["W"], c["NW"]) for c in cases) == sorted(g for g in M.natural_geometries(1, mode == 0, 12287) if g[1] in WIDE_WAVES[waves])
        assert len(cases) == (8 if waves == "few" else 4) and all(c["no_packed"] is False for c in cases)
    assert len(cases) == ({"ds": 12, "convex_heavy": 1}.get(family, len(cases))) and {c["rm"] for c in cases} == {0 if family == "ds" else 1}
    for c in cases:
        run_block(engine, monkeypatch, capfd, c)


@pytest.mark.parametrize("tier", range(5))
def test_adaptive_tiers_at_the_headline_geometries(engine, monkeypatch, capfd, tier):
    cases = cases_of("tier", "tier%d" % tier, 0)
    assert sorted((c["W"], c["NW"]) for c in cases) == [(10, 4), (11, 4)] and all(tuple(c["params"]) == M.TIERS[tier] for c in cases)
    for c in cases:
        assert M.case_class(c)[2] == M.TIER_CELL_BYTES[tier]
        run_block(engine, monkeypatch, capfd, c)


def run_align(engine, monkeypatch, capfd, case, force=None):
    label = M.case_id(case) + ("+force%d,%d" % force if force else "")
    set_env(monkeypatch, case, force=force)
    codes, off, pred, sink, q = M.align_problem(case)
    assert len(codes) == case["rows"] and len(q) == case["seq_lens"][2], label
    capfd.readouterr()
    (rows, pos, score, status), = engine.align([(codes, off, pred, sink, q)], Params(*case["params"], case["mode"], 0))
    st = engine.stats()
    err = capfd.readouterr().err
    print(label, status, score, len(rows))
    assert status == 0, (label, status)
    assert (score, len(rows), M.digest_pairs(rows, pos)) == (case["score"], case["n_pairs"], case["digest"]), (label, score, len(rows))
    check_launch(st, err, case, M.case_class(case, force=force), force or (case["W"], case["NW"]), 0, label)


ALIGN_CASES = [(f, m, s) for s in ("packed", "32-bit") for m in (0, 1) for f in M.ALIGN_FAMILIES] + [("wide_match", m, "int32-wide") for m in (0, 1)]


@pytest.mark.parametrize("family,mode,sweep", ALIGN_CASES, ids=["%s-%s-%s" % (f, ("local", "global")[m], s) for f, m, s in ALIGN_CASES])
def test_align_only_classes(engine, monkeypatch, capfd, family, mode, sweep):
    cases = cases_of("align", family, mode, no_packed=sweep == "32-bit")
    if sweep == "int32-wide":      # int32 row words by the scores alone: no knob, every geometry of the 32-bit sweep
        assert [(c["W"], c["NW"]) for c in cases] == M.natural_geometries(1, mode == 0, 12287) and {c["rm"] for c in cases} == {1}
    assert len(cases) >= (12 if sweep != "packed" else 21) and all((c["rm"] == 2) == (sweep == "packed") for c in cases)
    for c in cases:
        run_align(engine, monkeypatch, capfd, c)
        if "top" in c and (c["W"], c["NW"]) == (8, 8):
            for f in M.ALIGN_GLOBAL_FORCED:
                run_align(engine, monkeypatch, capfd, c, force=f)


# ---- the banded sweep: nine class lines, 18 kernels (tests/test_class_matrix_fixture.py: covered_band_kernels)

def run_band(engine, monkeypatch, capfd, case, knob4=False):
    label = M.case_id(case) + ("+bcb4" if knob4 else "")
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    for name in ("SXG_POA_NO_PACKED", "SXG_POA_CELL_BYTES", "SXG_POA_FORCE_P16", "SXG_POA_BAND_CELL_BYTES"):
        monkeypatch.delenv(name, raising=False)
    if knob4:
        monkeypatch.setenv("SXG_POA_BAND_CELL_BYTES", "4")
    seqs = M.case_inputs(case)
    assert [len(s) for s in seqs] == case["seq_lens"], label
    capfd.readouterr()
    res = engine.run_blocks([seqs], Params(*case["params"], case["mode"] | 0x10, case["banded"]))[0]
    st = engine.stats()
    err = capfd.readouterr().err
    assert res.status == 0, (label, res.status)          # (never ST_INTERNAL, never a refused sweep)
    got = {"scores": [int(x) for x in res.scores], "cells": int(res.cells.sum()), "n_nodes": int(len(res.node_code)), "n_edges": int(len(res.edge_tail)),
           "digests": M.digest_block(res.node_code, res.node_rank, res.node_group, res.edge_tail, res.edge_head, res.edge_weight, res.paths)}
    print(label, got["scores"], got["cells"], got["n_nodes"], got["n_edges"], st["retries"])
    for k, v in got.items():
        assert v == case[k], (label, k, v, case[k])
    kind, rm, cb, tmax, W, sw, ds = M.case_class(case, knob4)
    assert (kind, rm, tmax, W, sw, ds) == (0, 3, 64, case["W"], 1 - case["mode"], 0) and cb == (2 if not knob4 and sw and M.code_bits(tuple(case["params"])) <= 16 else 4), label
    assert (st["dom_row_mode"], st["dom_threads"], st["dom_cols_per_lane"]) == (3, 64, 2 * W), (label, st)
    lines = VARIANT_LINE.findall(err)
    assert len(lines) == 1, (label, lines, [x for x in err.splitlines() if "round" in x])
    T, lw, cvx, lrm, attempt, ltmax, lcb, lds, lw2 = map(int, lines[0])
    assert (T, lw, lrm, attempt, ltmax, lcb, lds, lw2) == (64, W, 3, 0, 64, cb, 0, 0), (label, lines)
    assert cvx == int(M.normalise(tuple(case["params"]))[6]), (label, lines)
    assert st["retries"] == 0 and st["dp_launches"] == 1, (label, st)
    return W, cb, sw, cvx


BAND_CASES = [(W, 0, f) for W in (6, 8, 11) for f in M.BAND_LOCAL_FAMILIES] + [(W, 1, None) for W in (6, 8, 11)]


@pytest.mark.parametrize("W,mode,family", BAND_CASES, ids=["W%d-%s" % (W, "local-" + f if f else "global") for W, m, f in BAND_CASES])
def test_banded_classes(engine, monkeypatch, capfd, W, mode, family):
    cases = [c for c in CASES if c["kind"] == "band" and c["W"] == W and c["mode"] == mode and (family is None or c["family"] == family)]
    ran = set()
    if mode == 0:     # the static and the adaptive band; the 2-byte families again with 4-byte band cells
        assert sorted(c["banded"] for c in cases) == [1, 2]
        for c in cases:
            ran.add(run_band(engine, monkeypatch, capfd, c))
            if family != "cb4_convex":
                ran.add(run_band(engine, monkeypatch, capfd, c, knob4=True))
        cvx = int(family != "gen2_affine")
        assert ran == ({(W, 4, 1, 1)} if family == "cb4_convex" else {(W, 2, 1, cvx), (W, 4, 1, cvx)})
    else:             # global: the adaptive band only, 4-byte cells by rule, a convex and an affine set
        assert [c["banded"] for c in cases] == [2, 2] and sorted(c["family"] for c in cases) == sorted(M.BAND_GLOBAL_FAMILIES[W])
        for c in cases:
            ran.add(run_band(engine, monkeypatch, capfd, c))
        assert ran == {(W, 4, 0, 0), (W, 4, 0, 1)}

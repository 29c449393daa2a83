"""Adaptive band of the packed sweep (round 8): after a block's first alignments, every alignment keeps only the strips of
the traceback plane that the drift of the block's earlier walks asks for (|path column - backbone hint|, plus a margin);
a hint-shift repeat doubles the width for the rest of the block.  The width changes speed, never results: a walk that
leaves the band is repaired exactly (hint shift and repeat, then a re-run with a plane that keeps every strip).

SXG_POA_BAND_ADAPT = "floor,margin,full" sets the band's parameters, "0" keeps the layout's width for every alignment (the
fixed band of rounds 1-7); SXG_POA_DEBUG prints the mean width the sweeps kept and the hint-shift repeats of a launch."""
import json
import os
import re

import numpy as np
import pytest

from helpers import assert_block_equal, gparams, oparams, random_block
from smoothxg_amd import Params, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
BAND_LINE = re.compile(r"band: (\d+) sweeps, mean width ([0-9.]+) strips of (\d+) \(\d+ columns\), (\d+) hint-shift repeats")


def _cases(name):
    with open(os.path.join(HERE, "golden", "fullshape_oracle.json")) as f:
        return [c for c in json.load(f)["cases"] if c["name"] == name and c.get("order", "s7") == "spoa"]


def _band_stats(text):
    """(sweeps, mean width, layout width of the first launch, repeats) of the packed launches that SXG_POA_DEBUG reported,
    summed over the launches (a block re-run with a plane that keeps every strip adds a launch of its own)."""
    rows = [tuple(float(x) for x in m.groups()) for m in BAND_LINE.finditer(text)]
    assert rows, "no band line in the engine's debug output"
    sweeps = sum(r[0] for r in rows)
    return sweeps, sum(r[0] * r[1] for r in rows) / max(sweeps, 1), rows[0][2], sum(r[3] for r in rows)


def _same(a, b, label):
    assert a.status == 0 and b.status == 0, label
    for k in ("scores", "cells", "node_code", "node_rank", "node_group", "edge_tail", "edge_head", "edge_weight", "consensus"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), "%s: %s differs between the adaptive and the fixed band" % (label, k)
    # (paths: one node path per sequence)
    assert len(a.paths) == len(b.paths), label
    for s, (pa, pb) in enumerate(zip(a.paths, b.paths)):
        assert np.array_equal(pa, pb), "%s: path of sequence %d differs between the adaptive and the fixed band" % (label, s)


@pytest.mark.parametrize("name", ["ns_sw", "ns_nw", "c3"])
def test_adaptive_band_matches_the_fixed_band_on_the_fixture_blocks(engine, monkeypatch, capfd, name):
    """The committed full-shape blocks (64 x 5 kbp, spoa's order): byte-identical outputs with the adaptive band and with
    the fixed 1 100-column band, and the adaptive band really kept fewer strips."""
    cases = _cases(name)
    assert cases
    blocks = [synth.make_block(c["block_id"], c["n_seqs"], c["length"]) for c in cases]
    prm = Params(*cases[0]["params"], cases[0]["mode"] | 0x10, 0)
    monkeypatch.setenv("SXG_POA_BAND_ADAPT", "0")
    fixed = engine.run_blocks(blocks, prm, want_consensus=True)
    monkeypatch.delenv("SXG_POA_BAND_ADAPT")
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    capfd.readouterr()
    adaptive = engine.run_blocks(blocks, prm, want_consensus=True)
    err = capfd.readouterr().err
    monkeypatch.delenv("SXG_POA_DEBUG")
    for c, a, f in zip(cases, adaptive, fixed):
        _same(a, f, "%s block %d" % (name, c["block_id"]))
        assert a.scores.tolist() == c["scores"]
    sweeps, mean_w, layout_w, _ = _band_stats(err)
    assert sweeps >= len(blocks) * 60 and mean_w < layout_w, (sweeps, mean_w, layout_w)


def test_drifting_block_with_a_capped_band_repairs_itself(engine, oracle, monkeypatch, capfd):
    """A block built to drift: a 420 bp insertion that half of the sequences carry, sequences without it first, so that the
    block's early walks see little drift and the band narrows before the first carrier arrives.  With the width capped at
    352 columns (SXG_POA_BAND_COLS) and an adaptive band allowed to shrink to 8 strips without margin, the walks leave the
    band, the sweeps are repeated with shifted hints and a doubled width -- and the block still matches the oracle."""
    rng = np.random.default_rng(808)
    base = random_block(rng, 1, 5000, div=0.0)[0]
    ins = rng.integers(0, 4, 420).astype(np.uint8)
    seqs = []
    for k in range(10):
        s = base.copy()
        pos = rng.integers(0, len(s), 40)
        s[pos] = (s[pos] + 1) & 3
        if k >= 5:
            s = np.concatenate([s[:2500], ins, s[2500:]])
        seqs.append(s)
    g, sc, cells = oracle.block_run(seqs, None, oparams("convex_default", 0))
    monkeypatch.setenv("SXG_POA_BAND_COLS", "352")
    monkeypatch.setenv("SXG_POA_BAND_ADAPT", "8,0,1")
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    capfd.readouterr()
    res = engine.run_blocks([seqs], gparams("convex_default", 0))
    err = capfd.readouterr().err
    assert_block_equal(res[0], g, sc, cells, label="drift-capped")
    sweeps, mean_w, layout_w, repeats = _band_stats(err)
    assert layout_w <= 36 and repeats >= 1, (sweeps, mean_w, layout_w, repeats)

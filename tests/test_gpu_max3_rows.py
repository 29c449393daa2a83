"""The local classes compiled for the default scores take the three-way maxima of a row -- max(diag + s, F, O) and
max(Hc, E, Q), and the nodes of the row-maximum tree -- as one binary16 instruction on their biased fields
(pk_max3, smoothxg_amd/csrc/poa_fields.h).  Every case here runs that code on another range of fields or another wave
count, equals the oracle exactly, and equals the run through the generic classes (SXG_POA_NO_DEFAULT_CLASS: unchanged code)."""
import numpy as np
import pytest

from helpers import assert_block_equal, gparams, oparams, random_block

pytestmark = pytest.mark.gpu


def _unrelated(rng, n, length):
    return [rng.integers(0, 4, length, dtype=np.uint8) for _ in range(n)]


# name: (seed, block builder, (threads, columns per lane) the one-block batch runs at, least top score or None, twin rows expected)
CASES = {
    # scores run beyond 0x6000 - 1 024 = 23 552: fields above 0x6000, the 16-wave class of 13 columns per strip (W >= 12: the
    # pinned pass 2)
    "high_fields_16_waves": (2601, lambda rng: random_block(rng, 3, 26000, div=0.01), (1024, 26), 0x6000 - 1024, False),
    # a one-block batch of 3 kbp is spread over four waves: twin steps and join rows
    "twin_rows_4_waves": (2602, lambda rng: random_block(rng, 6, 3000, div=0.03), (256, 12), None, True),
    "one_wave": (2603, lambda rng: random_block(rng, 4, 700, div=0.03), (64, 12), None, False),
    "two_waves": (2604, lambda rng: random_block(rng, 4, 1200, div=0.03), (128, 10), None, False),
    # nothing in common: almost every cell sits at the bias, every gap state below 1 024 (binary16 denormals)
    "low_fields": (2605, lambda rng: _unrelated(rng, 4, 2500), (256, 10), None, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_three_way_maxima_equal_the_oracle_and_the_generic_class(engine, oracle, monkeypatch, name):
    seed, build, geometry, top, twin = CASES[name]
    seqs = build(np.random.default_rng(seed))
    g, sc, cells = oracle.block_run(seqs, None, oparams("convex_default", 0))
    if top is not None:
        assert int(max(sc)) >= top, sc
    if name == "low_fields":
        assert int(max(sc)) < 60, sc
    monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
    res = engine.run_blocks([seqs], gparams("convex_default", 0))
    st = engine.stats()
    print(f"{name}: scores {list(sc)}, {st['dom_threads']} threads, {st['dom_cols_per_lane']} columns per lane, "
          f"twin steps {st['twin_steps']}, join rows {st['join_rows']}, retries {st['retries']}")
    assert st["dom_row_mode"] == 2 and (st["dom_threads"], st["dom_cols_per_lane"]) == geometry, st
    if name != "low_fields":            # (unrelated sequences: nearly every base a new node, the graph may outgrow its first tier)
        assert st["retries"] == 0, st   # (a wrong sweep that the widening ladder repairs would still equal the oracle)
    if twin:
        assert st["twin_steps"] > 0 and st["join_rows"] > 0, st
    assert_block_equal(res[0], g, sc, cells, label=f"{name}/default-score class")
    monkeypatch.setenv("SXG_POA_NO_DEFAULT_CLASS", "1")
    gen = engine.run_blocks([seqs], gparams("convex_default", 0))
    stg = engine.stats()
    monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
    assert stg["dom_row_mode"] == 2 and (stg["dom_threads"], stg["dom_cols_per_lane"]) == geometry, stg
    assert_block_equal(gen[0], g, sc, cells, label=f"{name}/generic class")


def test_global_block_of_the_default_scores_is_unchanged(engine, oracle, monkeypatch):
    """The global classes hold signed fields and keep their two-input integer maxima: still the oracle's result."""
    monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
    seqs = random_block(np.random.default_rng(2606), 5, 3000, div=0.03)
    g, sc, cells = oracle.block_run(seqs, None, oparams("convex_default", 1))
    res = engine.run_blocks([seqs], gparams("convex_default", 1))
    st = engine.stats()
    assert st["dom_row_mode"] == 2 and st["dom_threads"] == 256 and st["retries"] == 0, st
    assert_block_equal(res[0], g, sc, cells, label="global")

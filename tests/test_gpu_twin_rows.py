"""Packed sweep, twin step (round 13): the classes of three waves and more with 2-byte cells sweep two consecutive rows with the
same single predecessor in one step (ROW_TWIN) and the row that joins them takes their maxima out of the registers (ROW_JOIN).
Every case runs one block against the oracle bit for bit, in spoa's node order (where a substitution bubble lies A, B, B', C),
on a forced geometry with SXG_POA_NO_SPREAD=1, and compares the engine's counters with the plain restatement of the row flags
(tests/twin_ref.py) summed over the block's alignments; the same case with SXG_POA_TWIN=0 has both counters 0 and the same results.

Block S: an ancestor of 1 500 letters, 8 sequences with 4 % substitutions, every third with a deletion of 1 or 2 letters.  On
SXG_POA_FORCE_P16=4,4 -- four waves of 512 columns -- its bubbles fall in three waves and across their mailbox edges.
Block L: an ancestor of 5 200 letters, 6 sequences with 3 % substitutions: unforced it runs the W = 11 sweep of the four-wave
default-score class (5 200 letters do not fit its second width).
test_blocks_hold_every_case derives from the restatement how often each case the step has to get right occurs in S, and
requires every count to be positive: a change of the generator cannot quietly drop one."""
import numpy as np
import pytest

import twin_ref as T
from helpers import assert_block_equal
from smoothxg_amd import Params

pytestmark = pytest.mark.gpu

SCORES = {
    "default": (1, -4, -6, -2, -26, -1),   # the default-score class
    "asm10": (1, -9, -16, -2, -41, -1),    # another convex set: the general class
    "affine": (1, -4, -6, -2, -6, -2),
}
ORDER_SPOA = 0x10

_expected, _counts = {}, {}
BLOCKS, block = T.BLOCKS, T.block


def _impl(oracle):
    return oracle.IMPL_AVX2 if oracle.simd_available() else oracle.IMPL_SCALAR


def expected(oracle, name, scores, mode):
    """The oracle's run of the block, once per (block, scores, mode)."""
    k = (name, scores, mode)
    if k not in _expected:
        _expected[k] = oracle.block_run(block(name), None, oracle.mkparams(*SCORES[scores], mode=mode | ORDER_SPOA), impl=_impl(oracle))
    return _expected[k]


def counts(oracle, name, scores, mode):
    """The restatement's census summed over the graphs the block's alignments sweep (after 1 .. n - 1 sequences)."""
    k = (name, scores, mode)
    if k not in _counts:
        p = oracle.mkparams(*SCORES[scores], mode=mode | ORDER_SPOA)
        total = {}
        for n in range(1, len(block(name))):
            _, off, pred, _, _ = oracle.block_run(block(name)[:n], None, p, impl=_impl(oracle))[0].rows()
            for key, v in T.census(off, pred).items():
                total[key] = total.get(key, 0) + v
        _counts[k] = total
    return _counts[k]


def run(engine, oracle, monkeypatch, name, geometry, scores, mode, env, label, twin=True):
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    if geometry:
        monkeypatch.setenv("SXG_POA_FORCE_P16", "%d,%d" % geometry)
    monkeypatch.setenv("SXG_POA_TWIN", "1" if twin else "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g, sc, cells = expected(oracle, name, scores, mode)
    res = engine.run_blocks([block(name)], Params(*SCORES[scores], mode | ORDER_SPOA, 0))
    st = engine.stats()
    print(f"{label}/twin={twin}: {st['dom_threads']} threads x {st['dom_cols_per_lane']} columns per lane, row mode {st['dom_row_mode']}, widths "
          f"{st['dom_width']}/{st['dom_width2']}, sweeps {st['width_sweeps']}, twin steps {st['twin_steps']}, join rows {st['join_rows']}, "
          f"hint-shift repeats {st['hint_shift_repeats']}, retries {st['retries']}")
    assert st["dom_row_mode"] == 2, st
    if geometry:
        assert (st["dom_threads"], st["dom_cols_per_lane"]) == (64 * geometry[1], 2 * geometry[0]), st
    assert_block_equal(res[0], g, sc, cells, label=label)
    return st


def both(engine, oracle, monkeypatch, name, geometry, scores="default", mode=0, env={}, label=""):
    """The case with the step and with the knob off; the counters against the restatement."""
    st = run(engine, oracle, monkeypatch, name, geometry, scores, mode, env, label)
    want = counts(oracle, name, scores, mode)
    assert st["hint_shift_repeats"] == 0 and st["retries"] == 0, st
    assert (st["twin_steps"], st["join_rows"]) == (want["twin_steps"], want["joins"]), (st, want)
    assert want["twin_steps"] > 0 and want["joins"] > 0
    off = run(engine, oracle, monkeypatch, name, geometry, scores, mode, env, label, twin=False)
    assert (off["twin_steps"], off["join_rows"]) == (0, 0), off
    return st


def test_blocks_hold_every_case(oracle):
    """Twin steps with a stored predecessor, joins with further predecessors, pairs whose next row reads only the first row or
    neither, runs of three siblings, a pair directly after a pair, twin rows with a far reader: all occur in S."""
    c = counts(oracle, "S", "default", 0)
    print("block S:", c)
    for key, v in c.items():
        assert v > 0, key
    big = counts(oracle, "L", "default", 0)
    print("block L:", big)
    assert big["twin_steps"] > 1000 and big["joins"] > 1000


@pytest.mark.parametrize("scores,mode", [("default", 0), ("asm10", 0), ("affine", 1)])
def test_four_waves_of_512_columns(engine, oracle, monkeypatch, scores, mode):
    both(engine, oracle, monkeypatch, "S", (4, 4), scores, mode, label=f"S/4,4/{scores}/{mode}")


@pytest.mark.parametrize("geometry", [(4, 3), (8, 8)])
def test_three_and_eight_waves(engine, oracle, monkeypatch, geometry):
    both(engine, oracle, monkeypatch, "S", geometry, label="S/%d,%d" % geometry)


def test_headline_class_at_its_own_width(engine, oracle, monkeypatch):
    """L, unforced: four waves, strips of 11 columns, every alignment at W."""
    st = both(engine, oracle, monkeypatch, "L", None, label="L/unforced")
    assert (st["dom_threads"], st["dom_width"], st["dom_width2"]) == (256, 11, 10) and st["width_sweeps"][1] == 0, st


def test_headline_class_at_its_second_width(engine, oracle, monkeypatch):
    """S on 11,4: 1 500 letters fit the second width, every alignment runs at W2 = 10."""
    st = both(engine, oracle, monkeypatch, "S", (11, 4), label="S/11,4")
    assert st["dom_width2"] == 10 and st["width_sweeps"][0] == 0 and st["width_sweeps"][1] == len(block("S")) - 1, st


@pytest.mark.parametrize("lds_rows", ["0", "1"])
def test_on_chip_row_copies(engine, oracle, monkeypatch, lds_rows):
    """Every stored row in the ring, and one on-chip copy."""
    both(engine, oracle, monkeypatch, "S", (4, 4), env={"SXG_POA_LDS_ROWS": lds_rows}, label=f"S/4,4/lds_rows={lds_rows}")


@pytest.mark.parametrize("name", ["S", "SD"])
def test_hint_shift_repeats_over_twin_rows(engine, oracle, monkeypatch, name):
    """A plane of 480 columns keeps 232 columns on either side of a row's hint.  S itself never leaves it (its deletions are 1 or 2
    letters: measured, 0 repeats) and only has to stay exact; SD, the same recipe with deletions of 250 letters, does: its walks
    miss the band and their sweeps are repeated with shifted hints, twin rows included -- repeats or retries > 0."""
    env = {"SXG_POA_BAND_COLS": "480"}
    st = run(engine, oracle, monkeypatch, name, (4, 4), "default", 0, env, f"{name}/4,4/band 480")
    if name == "SD":
        assert st["hint_shift_repeats"] + st["retries"] > 0, st
    assert st["twin_steps"] > 0 and st["join_rows"] > 0, st
    off = run(engine, oracle, monkeypatch, name, (4, 4), "default", 0, env, f"{name}/4,4/band 480", twin=False)
    assert (off["twin_steps"], off["join_rows"]) == (0, 0), off


def test_a_class_without_the_step(engine, oracle, monkeypatch):
    """4-byte plane cells: no twin step, both counters 0, the same results."""
    st = run(engine, oracle, monkeypatch, "S", (4, 4), "default", 0, {"SXG_POA_CELL_BYTES": "4"}, "S/4,4/4-byte cells")
    assert (st["twin_steps"], st["join_rows"]) == (0, 0), st

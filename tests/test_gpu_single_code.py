"""One cell code for the packed sweep's 2-byte classes (round 11): the traceback plane holds the stored-row code, a row that is
stored AND inside its band is encoded once, and every reader of the plane -- the traceback, the one- and two-wave classes'
read-back of stored rows -- decodes row codes.  Every case compares scores, graph and per-base paths with the oracle.

Short blocks (8-12 sequences of 600-1 500 letters from synth.make_block) on the geometry each path needs: SXG_POA_FORCE_P16
puts a block on a wider packed geometry than its length asks for, SXG_POA_BAND_COLS narrows the plane so that a row's band
leaves waves out (and, narrowed far enough, so that a walk leaves it), and the engine's statistics say which class ran:

  * one wave, W <= 11: a plane that keeps every strip, stored rows are read back from it (rp = 2);
  * two waves, narrowed plane: row ring in HBM, on-chip row copies, a band that leaves a wave out;
  * four waves (T = 256, exact thread count, no read-back), band narrower than one wave: a row is stored and in band on one
    wave, stored but out of band on the others -- local and global; default scores (the default-score class), asm10 (general
    class, all 16 bits of the code) and affine 1,4,6,2; one case with a band so narrow that a walk misses it and is repeated;
  * the banded sweep (-A) at W = 6, whose plane keeps its delta code but is read through the same decoder;
  * 4-byte cells (SXG_POA_CELL_BYTES=4), which the change leaves alone."""
import re

import pytest

from helpers import assert_block_equal
from smoothxg_amd import Params, synth

pytestmark = pytest.mark.gpu

SCORES = {
    "default": (1, -4, -6, -2, -26, -1),
    "asm10": (1, -9, -16, -2, -41, -1),
    "affine": (1, -4, -6, -2, -6, -2),
}
# (block id, sequences, ancestor length) of synth.make_block: 1 154 / 1 299 letters in the longest sequence, a structural
# variant that three / five of the ten sequences carry
BLOCK_1K = (9001, 10, 1000)
BLOCK_12 = (9005, 10, 1200)
BAND_LINE = re.compile(r"band: (\d+) sweeps, mean width ([0-9.]+) strips of (\d+) \(\d+ columns\), (\d+) hint-shift repeats")

_blocks, _expected = {}, {}


def block(key):
    if key not in _blocks:
        _blocks[key] = synth.make_block(*key)
    return _blocks[key]


def expected(oracle, key, scores, mode, banded=0):
    """The oracle's run of a block, computed once per (block, scores, mode)."""
    k = (key, scores, mode, banded)
    if k not in _expected:
        _expected[k] = oracle.block_run(block(key), None, oracle.mkparams(*SCORES[scores], mode=mode, banded=banded))
    return _expected[k]


def run(engine, oracle, monkeypatch, key, scores, mode, env, geometry, banded=0, label=""):
    """geometry: (threads, columns per lane or None, row mode) the launch must have run at."""
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    g, sc, cells = expected(oracle, key, scores, mode, banded)
    res = engine.run_blocks([block(key)], Params(*SCORES[scores], mode, banded))
    st = engine.stats()
    print(f"{label}: ran {st['dom_threads']} threads x {st['dom_cols_per_lane']} columns per lane, row mode {st['dom_row_mode']}, "
          f"retries {st['retries']}, scores {sc.tolist()}")
    threads, cols, rm = geometry
    assert st["dom_row_mode"] == rm and st["dom_threads"] == threads, st
    if cols is not None:
        assert st["dom_cols_per_lane"] == cols, st
    assert_block_equal(res[0], g, sc, cells, label=label)
    return st


@pytest.mark.parametrize("scores,mode", [("default", 0), ("affine", 1)])
def test_one_wave_reads_stored_rows_back_from_a_plane_of_row_codes(engine, oracle, monkeypatch, scores, mode):
    st = run(engine, oracle, monkeypatch, BLOCK_1K, scores, mode, {}, (64, None, 2), label=f"one-wave/{scores}/{mode}")
    assert st["dom_cols_per_lane"] <= 22, st   # W <= 11: the class compiled for a plane that keeps every strip


@pytest.mark.parametrize("scores,mode", [("default", 0), ("default", 1)])
def test_two_waves_with_a_narrowed_plane(engine, oracle, monkeypatch, scores, mode):
    # 2 x 128 strips of 6 columns; the plane keeps 64 strips (384 columns) of a row: ring and on-chip copies, not the plane, feed
    # the stored predecessors, and most rows' bands lie inside one wave
    run(engine, oracle, monkeypatch, BLOCK_12, scores, mode, {"SXG_POA_FORCE_P16": "6,2", "SXG_POA_BAND_COLS": "384"},
        (128, 12, 2), label=f"two-wave/{scores}/{mode}")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scores", list(SCORES))
def test_four_waves_with_a_band_narrower_than_a_wave(engine, oracle, monkeypatch, scores, mode):
    # 4 x 128 strips of 4 columns; the plane keeps 64 strips (256 columns) of a row
    run(engine, oracle, monkeypatch, BLOCK_12, scores, mode, {"SXG_POA_FORCE_P16": "4,4", "SXG_POA_BAND_COLS": "256"},
        (256, 8, 2), label=f"four-wave/{scores}/{mode}")


def test_four_waves_band_miss_is_repeated_and_matches_the_oracle(engine, oracle, monkeypatch, capfd):
    """A plane of 8 strips (32 columns, 12 on either side of the hint) cannot hold the walk of a sequence that carries the
    block's structural variant against a graph built without it: the walk misses the band, the sweep is repeated with shifted
    hints (or, failing that, the block is re-run with a plane that keeps every strip) -- and the result is the oracle's."""
    monkeypatch.setenv("SXG_POA_DEBUG", "1")
    capfd.readouterr()
    st = run(engine, oracle, monkeypatch, BLOCK_12, "default", 0, {"SXG_POA_FORCE_P16": "4,4", "SXG_POA_BAND_COLS": "32"},
             (256, 8, 2), label="four-wave/band-miss")
    err = capfd.readouterr().err
    repeats = sum(int(m.group(4)) for m in BAND_LINE.finditer(err))
    print(f"hint-shift repeats {repeats}, re-runs {st['retries']}")
    assert repeats + st["retries"] >= 1, (repeats, st)


def test_banded_sweep_keeps_its_delta_code(engine, oracle, monkeypatch):
    run(engine, oracle, monkeypatch, BLOCK_12, "default", 0, {}, (64, 12, 3), banded=2, label="banded-A/W6")


def test_four_byte_cells_are_unchanged(engine, oracle, monkeypatch):
    run(engine, oracle, monkeypatch, BLOCK_12, "default", 0, {"SXG_POA_FORCE_P16": "4,4", "SXG_POA_BAND_COLS": "256", "SXG_POA_CELL_BYTES": "4"},
        (256, 8, 2), label="four-wave/4-byte")

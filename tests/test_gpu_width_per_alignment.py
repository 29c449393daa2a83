"""Packed sweep, strip width per alignment (round 12): a class with a second width W2 = W - 1 sweeps every alignment whose
sequence fits T * 2 * W2 columns in strips of W2 columns, sweep and traceback alike.  Every case runs one block against the
oracle bit for bit and asserts from the engine's width counters which sweeps ran at which width, and from its statistics
which class ran.

The smallest geometry with a dual-width class and four waves (the mailbox path) is forced: SXG_POA_FORCE_P16=9,4.  Its 256
lanes hold two strips each: 256 * 2 * 9 = 4 608 columns, of which W2 = 8 covers 4 096 -- sequences of up to 4 095 letters run at
W2, 4 096 letters at W.  One case runs eight waves (9,8: 9 216 columns, W2 = 8 up to 8 191 letters).
The block: an ancestor of 4 300 letters, every sequence with 2 % substitutions, the short ones with a 250-letter deletion, in
the order long, short, long, 4 095 letters, 4 096 letters, short, long, short -- handed over unsorted, so that the width changes
in both directions between alignments (band state, LDS layout, mailbox reset) and both sides of the boundary are in it.
One case runs two blocks on their own geometries, W = 11 and W = 10 at four waves (the headline's pair), apart and -- with
SXG_POA_MERGE_WIDTH2=1 -- in ONE launch of the W = 11 class, where every alignment of the W = 10 block runs at W2."""
import numpy as np
import pytest

from helpers import assert_block_equal
from smoothxg_amd import Params

pytestmark = pytest.mark.gpu

SCORES = {
    "default": (1, -4, -6, -2, -26, -1),   # the default-score class
    "asm10": (1, -9, -16, -2, -41, -1),    # another convex set: the general class
    "affine": (1, -4, -6, -2, -6, -2),
}
W, W2 = 9, 8
DELETION = 250
# waves -> (ancestor length, deletions of the block's sequences in alignment order; "cap" / "cap+1": down to exactly that length)
SHAPES = {
    4: (4300, (0, DELETION, 0, "cap", "cap+1", DELETION, 0, DELETION)),
    8: (8400, (0, DELETION, 0, "cap", "cap+1", DELETION)),
    # unforced, four waves: 5 200 letters choose W = 11 (W2 = 10 up to 5 119 letters), 5 000 letters W = 10
    "w11": (5200, (0, DELETION, 0, "cap", "cap+1", DELETION)),
    "w10": (5000, (0, DELETION, 0, DELETION)),
}

_blocks, _expected = {}, {}


def cap(waves):
    """The longest sequence that runs at W2."""
    if waves in ("w11", "w10"):
        return 256 * 2 * 10 - 1
    return 64 * waves * 2 * W2 - 1


def block(waves):
    if waves not in _blocks:
        n, dels = SHAPES[waves]
        rng = np.random.default_rng(1200 + (waves if isinstance(waves, int) else int(waves[1:])))
        anc = rng.integers(0, 4, n, dtype=np.uint8)
        pos = n // 3
        seqs = []
        for d in dels:
            d = n - cap(waves) if d == "cap" else (n - cap(waves) - 1 if d == "cap+1" else d)
            s = anc.copy()
            m = rng.random(n) < 0.02
            s[m] = (s[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
            seqs.append(np.concatenate([s[:pos], s[pos + d:]]))
        assert "cap" not in dels or [len(s) for s in seqs][3:5] == [cap(waves), cap(waves) + 1]
        _blocks[waves] = seqs
    return _blocks[waves]


def expected(oracle, waves, scores, mode):
    """The oracle's run of the block, computed once per (block, scores, mode) -- with its vector implementation, which
    test_oracle.py holds equal to the scalar one (these blocks take it 0.5-1.5 s instead of 4-10 s)."""
    k = (waves, scores, mode)
    if k not in _expected:
        _expected[k] = oracle.block_run(block(waves), None, oracle.mkparams(*SCORES[scores], mode=mode), impl=oracle.IMPL_AVX2)
    return _expected[k]


def run(engine, oracle, monkeypatch, waves, scores, mode, env, label):
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.setenv("SXG_POA_FORCE_P16", "%d,%d" % (W, waves))
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    g, sc, cells = expected(oracle, waves, scores, mode)
    res = engine.run_blocks([block(waves)], Params(*SCORES[scores], mode, 0))
    st = engine.stats()
    print(f"{label}: {st['dom_threads']} threads x {st['dom_cols_per_lane']} columns per lane, row mode {st['dom_row_mode']}, widths "
          f"{st['dom_width']}/{st['dom_width2']}, sweeps {st['width_sweeps']}, swept columns {st['width_swept_cols']}, "
          f"hint-shift repeats {st['hint_shift_repeats']}, retries {st['retries']}")
    # the class that ran: the forced geometry's, packed sweep; dom_cols_per_lane keeps reporting the class's W
    assert (st["dom_row_mode"], st["dom_threads"], st["dom_cols_per_lane"], st["dom_width"]) == (2, 64 * waves, 2 * W, W), st
    assert_block_equal(res[0], g, sc, cells, label=label)
    return st


def widths_of(waves):
    """(sweeps at W, sweeps at W2) of the block's alignments: the first sequence founds the graph and is not swept."""
    narrow = sum(1 for s in block(waves)[1:] if len(s) <= cap(waves))
    return len(block(waves)) - 1 - narrow, narrow


def assert_widths(st, waves, dual):
    """Without repeats every alignment is one sweep, at the narrowest width that covers it."""
    t = 64 * waves
    wide, narrow = widths_of(waves) if dual else (len(block(waves)) - 1, 0)
    assert st["hint_shift_repeats"] == 0 and st["retries"] == 0, st
    assert st["dom_width2"] == (W2 if dual else 0), st
    assert tuple(st["width_sweeps"]) == (wide, narrow), st
    assert tuple(st["width_swept_cols"]) == (wide * t * 2 * W, narrow * t * 2 * W2), st


@pytest.mark.parametrize("waves", [4, 8])
def test_alternating_widths_and_both_sides_of_the_boundary(engine, oracle, monkeypatch, waves):
    """cap letters run at W2, cap + 1 at W; the width changes in both directions between alignments."""
    assert widths_of(waves) == ((3, 4) if waves == 4 else (2, 3))
    st = run(engine, oracle, monkeypatch, waves, "default", 0, {}, f"alternating/{waves} waves")
    assert_widths(st, waves, dual=True)


@pytest.mark.parametrize("adapt", [None, "0"])
def test_repeats_at_the_narrow_width(engine, oracle, monkeypatch, adapt):
    """A plane of 480 columns keeps at most 232 columns on either side of a row's hint: the walk of a short sequence, 250 columns
    off the backbone behind its deletion, misses it and its sweep is repeated at the same width with shifted hints -- with the
    adaptive band at its defaults (the least width after a repeat is carried from a narrow to a wide alignment, in columns) and
    with the fixed band."""
    env = {"SXG_POA_BAND_COLS": "480"}
    if adapt is not None:
        env["SXG_POA_BAND_ADAPT"] = adapt
    st = run(engine, oracle, monkeypatch, 4, "default", 0, env, f"repeats/adapt={adapt}")
    wide, narrow = widths_of(4)
    assert st["hint_shift_repeats"] + st["retries"] > 0, st
    assert st["dom_width2"] == W2 and st["width_sweeps"][0] >= wide and st["width_sweeps"][1] > narrow, st
    assert st["width_swept_cols"] == (st["width_sweeps"][0] * 256 * 2 * W, st["width_sweeps"][1] * 256 * 2 * W2), st


@pytest.mark.parametrize("scores,mode", [("asm10", 0), ("affine", 1)])
def test_score_sets(engine, oracle, monkeypatch, scores, mode):
    """The general class (another convex local set) and global affine 1,4,6,2; the default scores run in every other case."""
    st = run(engine, oracle, monkeypatch, 4, scores, mode, {}, f"scores/{scores}/{mode}")
    assert_widths(st, 4, dual=True)


def test_a_class_without_a_second_width(engine, oracle, monkeypatch):
    """4-byte plane cells: the same block, no sweep at a narrow width, the same results."""
    st = run(engine, oracle, monkeypatch, 4, "default", 0, {"SXG_POA_CELL_BYTES": "4"}, "4-byte cells")
    assert_widths(st, 4, dual=False)


def test_knob_switches_the_second_width_off(engine, oracle, monkeypatch):
    """SXG_POA_WIDTH2=0: every alignment at W, the same block results as the default (both equal the oracle's)."""
    st = run(engine, oracle, monkeypatch, 4, "default", 0, {"SXG_POA_WIDTH2": "0"}, "knob off")
    assert_widths(st, 4, dual=False)


@pytest.mark.parametrize("merged", [False, True])
def test_neighbouring_widths_apart_and_in_one_launch(engine, oracle, monkeypatch, merged):
    """A W = 11 block and a W = 10 block, four waves each, on the geometries their lengths choose.  Apart: two launches, the W = 10
    launch's class has W2 = 9, which 5 kbp never fits.  SXG_POA_MERGE_WIDTH2=1: one launch of the W = 11 class, the W = 10 block's
    alignments all at its W2."""
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    if merged:
        monkeypatch.setenv("SXG_POA_MERGE_WIDTH2", "1")
    res = engine.run_blocks([block("w11"), block("w10")], Params(*SCORES["default"], 0, 0))
    st = engine.stats()
    print(f"merged={merged}: launches {st['dp_launches']}, widths {st['dom_width']}/{st['dom_width2']}, sweeps {st['width_sweeps']}, "
          f"hint-shift repeats {st['hint_shift_repeats']}, retries {st['retries']}")
    for key, r in zip(("w11", "w10"), res):
        g, sc, cells = expected(oracle, key, "default", 0)
        assert_block_equal(r, g, sc, cells, label=f"{key}/merged={merged}")
    assert st["hint_shift_repeats"] == 0 and st["retries"] == 0 and st["dom_threads"] == 256, st
    wide, narrow = widths_of("w11")
    assert (wide, narrow) == (2, 3)
    n10 = len(block("w10")) - 1
    if merged:
        assert st["dp_launches"] == 1 and (st["dom_width"], st["dom_width2"]) == (11, 10), st
        assert tuple(st["width_sweeps"]) == (wide, narrow + n10), st
        assert tuple(st["width_swept_cols"]) == (wide * 512 * 11, (narrow + n10) * 512 * 10), st
    else:
        assert st["dp_launches"] == 2, st
        assert tuple(st["width_sweeps"]) == (wide + n10, narrow), st
        assert tuple(st["width_swept_cols"]) == (wide * 512 * 11 + n10 * 512 * 10, narrow * 512 * 10), st

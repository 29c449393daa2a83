"""Neighbouring widths in one launch by default (round 14): a round whose packed launches together ask for at least one workgroup
per CU runs a geometry whose strip width is the second width of a wider one's class INSIDE that class's launch -- the headline's
W = 10 blocks beside its W = 11 blocks -- with every block priced, sorted and dealt over the CUs by the columns its alignments
sweep there (smoothxg_amd/csrc/poa_cost.h).  Below that size the launches stay apart; SXG_POA_MERGE_WIDTH2=0 keeps them apart at
any size.  The plan changes where and when a block runs, never what it computes: every block of every case equals the oracle's
run of its recipe bit for bit, and the engine's width counters say which sweeps ran at which width.

Blocks of 3 sequences on the recipes of test_gpu_width_per_alignment.py (an ancestor, 2 % substitutions per sequence, a deletion
a third of the way in), four waves each on the geometries their lengths choose:
    w11: 5 200, 5 119 and 5 120 letters -- W = 11 (5 632 columns); its class's W2 = 10 covers 5 119 letters (+ column 0 = 5 120
         columns) and not 5 120: one sweep on either side of the boundary;
    w10: 5 000, 4 750 and 5 000 letters -- W = 10 (5 120 columns); on its own class (W2 = 9: 4 608 columns) both sweeps run at
         W = 10, merged into the W = 11 class both run at that class's W2 = 10.
No case asserts a time."""
import numpy as np
import pytest

from helpers import assert_block_equal
from smoothxg_amd import Params

pytestmark = pytest.mark.gpu

DEFAULT = (1, -4, -6, -2, -26, -1)
CAP = 256 * 2 * 10 - 1   # the longest sequence the W = 11 class sweeps at W2 = 10
# recipe -> (ancestor length, lengths of the block's sequences)
SHAPES = {"w11": (5200, (5200, CAP, CAP + 1)), "w10": (5000, (5000, 4750, 5000))}

_blocks, _expected = {}, {}


def block(key):
    if key not in _blocks:
        n, lens = SHAPES[key]
        rng = np.random.default_rng(1500 + int(key[1:]))
        anc = rng.integers(0, 4, n, dtype=np.uint8)
        pos = n // 3
        seqs = []
        for length in lens:
            s = anc.copy()
            m = rng.random(n) < 0.02
            s[m] = (s[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
            seqs.append(np.concatenate([s[:pos], s[pos + n - length:]]))
        assert tuple(len(s) for s in seqs) == lens
        _blocks[key] = seqs
    return _blocks[key]


def expected(oracle, key):
    """The oracle's run of a recipe's block, once per distinct block (its vector implementation: test_oracle.py holds it equal to
    the scalar one)."""
    if key not in _expected:
        _expected[key] = oracle.block_run(block(key), None, oracle.mkparams(*DEFAULT, mode=0), impl=oracle.IMPL_AVX2)
    return _expected[key]


def run(engine, oracle, monkeypatch, keys, env, label):
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.delenv("SXG_POA_MERGE_WIDTH2", raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    res = engine.run_blocks([block(k) for k in keys], Params(*DEFAULT, 0, 0))
    st = engine.stats()
    print(f"{label}: {len(keys)} blocks, launches {st['dp_launches']}, slots {st['n_slots']}, widths {st['dom_width']}/{st['dom_width2']}, "
          f"sweeps {st['width_sweeps']}, swept columns {st['width_swept_cols']}, hint-shift repeats {st['hint_shift_repeats']}, retries {st['retries']}")
    for i, (k, r) in enumerate(zip(keys, res)):
        g, sc, cells = expected(oracle, k)
        assert_block_equal(r, g, sc, cells, label=f"{label}/block {i} ({k})")
    assert st["hint_shift_repeats"] == 0 and st["retries"] == 0 and st["dom_threads"] == 256 and st["dom_row_mode"] == 2, st
    return st


def assert_sweeps(st, keys, merged):
    """Without repeats every alignment is one sweep.  Counters: (at the launch's W, at its class's W2), summed over the launches."""
    n11, n10 = keys.count("w11"), keys.count("w10")
    if merged:   # one launch of the W = 11 class: a w11 block one sweep at either width, a w10 block both at W2 = 10
        assert st["dp_launches"] == 1 and (st["dom_width"], st["dom_width2"]) == (11, 10), st
        assert tuple(st["width_sweeps"]) == (n11, n11 + 2 * n10), st
        assert tuple(st["width_swept_cols"]) == (n11 * 512 * 11, (n11 + 2 * n10) * 512 * 10), st
    else:        # apart: the W = 10 launch's class has W2 = 9, which 4 750 letters do not fit
        assert st["dp_launches"] == 2, st
        assert tuple(st["width_sweeps"]) == (n11 + 2 * n10, n11), st
        assert tuple(st["width_swept_cols"]) == (n11 * 512 * 11 + 2 * n10 * 512 * 10, n11 * 512 * 10), st


def alternating(n):
    return ["w11" if i % 2 == 0 else "w10" for i in range(n)]


def test_one_workgroup_per_cu_merges_by_default(engine, oracle, monkeypatch):
    """(a) as many blocks as the device has CUs, the recipes alternating, nothing set: ONE launch of the W = 11 class."""
    keys = alternating(engine.compute_units())
    st = run(engine, oracle, monkeypatch, keys, {}, "default")
    assert st["n_slots"] == len(keys), st
    assert_sweeps(st, keys, merged=True)


def test_knob_keeps_the_launches_apart(engine, oracle, monkeypatch):
    """(b) the same batch with SXG_POA_MERGE_WIDTH2=0: two launches, the same results."""
    keys = alternating(engine.compute_units())
    st = run(engine, oracle, monkeypatch, keys, {"SXG_POA_MERGE_WIDTH2": "0"}, "knob off")
    assert_sweeps(st, keys, merged=False)


def test_two_blocks_stay_apart(engine, oracle, monkeypatch):
    """(c) two blocks, nothing set: nothing shares a CU, nothing to deal -- two launches, as
    test_gpu_width_per_alignment.py::test_neighbouring_widths_apart_and_in_one_launch[False] expects."""
    keys = ["w11", "w10"]
    st = run(engine, oracle, monkeypatch, keys, {}, "two blocks")
    assert_sweeps(st, keys, merged=False)


def test_every_slot_of_the_merged_launch_ran(engine, oracle, monkeypatch, tmp_path):
    """(d) the merged batch with the per-slot record (SXG_POA_SLOT_CSV: slot, start, end, one word smid << 32 | HW_ID per wave):
    every slot ran, and no CU holds more than the four workgroups of this class that fit one."""
    csv = tmp_path / "slots.csv"
    keys = alternating(engine.compute_units())
    st = run(engine, oracle, monkeypatch, keys, {"SXG_POA_DEBUG": "1", "SXG_POA_SLOT_CSV": str(csv)}, "slot record")
    assert_sweeps(st, keys, merged=True)
    rows = [line.split(",") for line in csv.read_text().splitlines() if line.strip()]
    assert [int(r[0]) for r in rows] == list(range(len(keys))), "one record per slot of the one launch"
    per_cu = {}
    for r in rows:
        start, end, waves = int(r[1]), int(r[2]), [int(x, 16) for x in r[3:]]
        assert start > 0 and end > start, r
        assert len(waves) == 4 and len({w >> 32 for w in waves}) == 1, r   # four waves, on one CU
        per_cu[waves[0] >> 32] = per_cu.get(waves[0] >> 32, 0) + 1
    print(f"slot record: {len(rows)} slots on {len(per_cu)} CUs, at most {max(per_cu.values())} per CU")
    assert max(per_cu.values()) <= 4, per_cu

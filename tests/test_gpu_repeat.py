"""GPU: the tandem-repeat scan on the device (sxg_poa_repeat_scan_batch, decree R of DESIGN.md section 9) against the restatement
in tests/repeat_ref.py and the oracle.  The counts must equal numpy's, (best, dev, v) the restatement's bit patterns, the decided
lengths oracle.smooth_oracle.repeat_length's; through the host library the blocks with the scanner must be the blocks without it.
There is no tolerance anywhere."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import repeat_ref as RR  # noqa: E402
from oracle import smooth_oracle as SO  # noqa: E402
from smoothxg_amd import poa as P  # noqa: E402
from smoothxg_amd import smooth as S  # noqa: E402
from test_repeat_host import shared_chain_gfa  # noqa: E402
from test_smooth_host import DRB1  # noqa: E402

pytestmark = pytest.mark.gpu
SMALL, TILE, REAL = (8, 64), (8, 1000), (1000, 20000)


def tandem(rng, n, period, sub=0.0, letters=b"ACGT"):
    unit = rng.integers(0, len(letters), period)
    s = np.frombuffer(letters, np.uint8)[unit[np.arange(n) % period]].copy()
    hit = rng.random(n) < sub
    s[hit] = np.frombuffer(letters, np.uint8)[rng.integers(0, len(letters), int(hit.sum()))]
    return s.tobytes()


@functools.lru_cache(maxsize=None)
def batch():
    """Every case in which the kernels can go wrong (the comments name them), as {(min_copy, max_copy, stride): [sequences]}:
    one engine call per parameter set, made once for the module."""
    rng = np.random.default_rng(2027)
    rnd = lambda n: tandem(rng, n, n)                                      # random letters: no repeat
    mixed_case = bytearray(tandem(rng, 600, 40, 0.05))
    mixed_case[100:180] = bytes(mixed_case[100:180]).lower()               # lower case is another letter (R1)
    mixed_case[300:340] = b"N" * 40                                        # N == N
    small = [rnd(16),                                                      # one lag: sd = 0
             rnd(17), rnd(72), rnd(73), rnd(333), rnd(600),                # 2 lags; the last lag is max_copy exactly; beyond it
             tandem(rng, 600, 40),                                         # exact period 40: equal greatest r at 40 and at nothing before it
             tandem(rng, 333, 10),                                         # exact period 10: r = 1 at lags 10, 20, ... -- the first wins
             tandem(rng, 600, 40, 0.05), tandem(rng, 600, 20, 0.05),       # the issue's shapes: 40 at z 5; 20 only at z 3 (three peaks)
             tandem(rng, 600, 40, 0.05), tandem(rng, 333, 25, 0.03),
             bytes(mixed_case), b"A" * 600, b"N" * 100,                    # poly-A, a run of N: every r is 1, sd = 0
             rnd(15), b"",                                                 # shorter than 2 min_copy; empty
             tandem(rng, 73, 9, 0.02)]
    tile = [rnd(270), rnd(271), rnd(272),                                  # 255, 256 and 257 lags: one below, equal to, one above the lag tile
            tandem(rng, 600, 150, 0.05), rnd(600), tandem(rng, 523, 60)]   # three tiles, the last one partial
    real = [rnd(2000), rnd(2001),                                          # one lag, two lags
            tandem(rng, 2600, 1200, 0.05), rnd(6000),
            tandem(rng, 21049, 7000, 0.05), tandem(rng, 45000, 3000, 0.05),   # 19 050 and 19 001 lags: 75 tiles, the last one short
            tandem(rng, 6000, 1300, 0.02, b"ACGTacgtN"), rnd(1999)]
    out = {SMALL + (stride,): small for stride in (1, 3, 7, 50)}           # stride 50 > n - L: cnt = 1
    out[TILE + (3,)] = tile
    out[REAL + (50,)] = real
    return out


@functools.lru_cache(maxsize=None)
def want():
    """The restatement's answer, computed once: {params: [(n_lags, counts, best, dev, v) per sequence]}."""
    out = {}
    for (lo, hi, stride), seqs in batch().items():
        rows = []
        for s in seqs:
            m = RR.counts(s, lo, hi, stride)
            rows.append((len(m), m) + (RR.stats(m, len(s), lo, stride) if len(m) else (0, 0.0, 0.0)))
        out[(lo, hi, stride)] = rows
    return out


@pytest.fixture(scope="module")
def got(engine):
    return {key: engine.repeat_scan(seqs, *key, want_match=True) for key, seqs in batch().items()}


def lengths(rows, lo, min_z):
    return [RR.decide(lo, r[2], r[3], r[4], min_z) if r[0] else 0.0 for r in rows]


def test_the_batch_holds_what_it_says():
    """On the oracle alone: both outcomes, the tile's neighbours, equal greatest r, cnt = 1, sd = 0."""
    found = none = 0
    for (lo, hi, stride), seqs in batch().items():
        for s, row in zip(seqs, want()[(lo, hi, stride)]):
            for z in (5.0, 3.0):
                rl = SO.repeat_length(s.decode(), lo, hi, z, stride)
                assert rl == (RR.decide(lo, row[2], row[3], row[4], z) if row[0] else 0.0), (lo, hi, stride, len(s), z)
            found += SO.repeat_length(s.decode(), lo, hi, 5.0, stride) > 0
            none += SO.repeat_length(s.decode(), lo, hi, 5.0, stride) == 0 and len(s) >= 2 * lo
    assert found >= 5 and none >= 5, (found, none)
    w = want()
    assert [r[0] for r in w[TILE + (3,)][:3]] == [RR.TILE_LAGS - 1, RR.TILE_LAGS, RR.TILE_LAGS + 1]
    assert [r[0] for r in w[SMALL + (1,)][:6]] == [1, 2, 57, 57, 57, 57] and [r[0] for r in w[REAL + (50,)][:2]] == [1, 2]
    assert [r[0] for r in w[REAL + (50,)][4:6]] == [19001, 19001] and w[REAL + (50,)][7][0] == 0
    exact = w[SMALL + (1,)][7]                                              # period 10: r = 1 at 10, 20, 30, ...; the first wins
    assert exact[2] == 2 and exact[1][2] == 333 - 10 and exact[1][12] == 333 - 20
    assert lengths(w[SMALL + (3,)], 8, 5.0)[8] == 40.0                      # the issue's examples
    assert lengths(w[SMALL + (1,)], 8, 5.0)[9] == 0.0 and lengths(w[SMALL + (1,)], 8, 3.0)[9] == 20.0   # (three peaks: 20, 40, 60)
    assert lengths(w[REAL + (50,)], 1000, 5.0)[2] == 1200.0 and lengths(w[REAL + (50,)], 1000, 5.0)[5] % 3000 == 0 < lengths(w[REAL + (50,)], 1000, 5.0)[5]
    assert w[SMALL + (50,)][0][1].tolist() == [int(batch()[SMALL + (50,)][0][0] == batch()[SMALL + (50,)][0][8])]   # cnt = 1
    assert w[SMALL + (1,)][13][4] == 0.0 and w[SMALL + (1,)][0][4] == 0.0   # poly-A and the single lag: sd = 0


def test_counts_equal_numpy(got):
    for key, rows in want().items():
        lags, best, dev, v, status, match = got[key]
        assert status.tolist() == [0] * len(rows) and lags.tolist() == [r[0] for r in rows], key
        for s, r in enumerate(rows):
            assert match[s].dtype == np.int32 and match[s].tolist() == r[1].tolist(), (key, s)


def test_statistics_bit_for_bit(got):
    for key, rows in want().items():
        lags, best, dev, v, status, match = got[key]
        for s, r in enumerate(rows):
            assert int(best[s]) == r[2] and RR.bits(dev[s]) == RR.bits(r[3]) and RR.bits(v[s]) == RR.bits(r[4]), (key, s, best[s], dev[s], v[s], r[2:])


def test_decided_lengths_are_the_oracles(got):
    for (lo, hi, stride), seqs in batch().items():
        lags, best, dev, v, status, match = got[(lo, hi, stride)]
        for z in (5.0, 3.0):
            mine = [RR.decide(lo, int(best[s]), float(dev[s]), float(v[s]), z) if lags[s] else 0.0 for s in range(len(seqs))]
            assert mine == [SO.repeat_length(s.decode(), lo, hi, z, stride) for s in seqs], (lo, hi, stride, z)


def test_stats_and_an_empty_batch(engine):
    key = TILE + (3,)
    engine.repeat_scan(batch()[key], *key)
    st = engine.stats()
    assert st["kernel_ms"] > 0 and st["device_bytes"] > 0 and st["dp_launches"] == 2 and st["n_slots"] == sum(-(-r[0] // RR.TILE_LAGS) for r in want()[key]) == 12
    res = engine.repeat_scan([], 8, 64, 3, want_match=True)
    assert [len(x) for x in res] == [0] * 6 and engine.stats()["dp_launches"] == 0
    res = engine.repeat_scan([b"ACGT", b""], 8, 64, 3)
    assert res[0].tolist() == [0, 0] and res[4].tolist() == [0, 0] and engine.stats()["dp_launches"] == 0


def test_rounds_under_a_small_budget_give_the_same_bytes(engine, got):
    key = REAL + (50,)
    seqs, rows = batch()[key], want()[key]
    ns, n_work = len(seqs), sum(r[0] > 0 for r in rows)
    items = sum(-(-r[0] // RR.TILE_LAGS) for r in rows)
    fixed = sum(len(s) for s in seqs) + 16 * (ns + 1) + 8 * items + 4 * n_work + 20 * ns
    most = max(r[0] for r in rows)
    assert sum(r[0] for r in rows) > most + 100
    try:
        engine.set_memory_budget(fixed + 4 * (most + 100))               # the counts of the longest sequence and a hundred more
        two = engine.repeat_scan(seqs, *key, want_match=True)
        st = engine.stats()
        engine.set_memory_budget(fixed + 4 * (most - 1))
        with pytest.raises(P.PoaError, match="memory budget too small"):
            engine.repeat_scan(seqs, *key)
    finally:
        engine.set_memory_budget(0)
    assert st["dp_launches"] // 2 >= 2                                     # (count, statistics) per round
    one = got[key]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one[:5], two[:5]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one[5], two[5]))


def test_same_batch_twice_gives_the_same_bytes(engine, got):
    key = SMALL + (7,)
    again = engine.repeat_scan(batch()[key], *key, want_match=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[key][:5], again[:5]))


def test_too_long_sequence_is_declined_alone(engine):
    rng = np.random.default_rng(9)
    seqs = [tandem(rng, 600, 40, 0.05), tandem(rng, P.REPEAT_MAX_LEN + 1, 977), tandem(rng, 333, 25, 0.03)]
    lags, best, dev, v, status, match = engine.repeat_scan(seqs, 8, 64, 3, want_match=True, check=False)
    assert status.tolist() == [0, P.ST_TOO_LONG, 0] and lags.tolist() == [57, 0, 57] and len(match[1]) == 0
    for s in (0, 2):
        m = RR.counts(seqs[s], 8, 64, 3)
        assert match[s].tolist() == m.tolist()
        ref = RR.stats(m, len(seqs[s]), 8, 3)
        assert (int(best[s]), RR.bits(dev[s]), RR.bits(v[s])) == (ref[0], RR.bits(ref[1]), RR.bits(ref[2]))
    with pytest.raises(P.PoaError, match="longer than"):
        engine.repeat_scan(seqs, 8, 64, 3)


def test_bad_parameters(engine):
    for lo, hi, stride in ((0, 64, 3), (8, 64, 0), (8, 7, 3)):
        with pytest.raises(P.PoaError, match="min_copy and stride"):
            engine.repeat_scan([b"ACGT" * 50], lo, hi, stride)


DISCOVER = [("chain", lambda: shared_chain_gfa(5), dict(target_poa_length=4000, n_haps=3, max_poa_length=2000)),
            ("chain-scaled", lambda: shared_chain_gfa(6, n_paths=4, unit=600, copies=8), dict(target_poa_length=3000, n_haps=4, max_poa_length=1500, repeats=(400, 3000, 4.0, 25))),
            ("drb1-scaled", lambda: open(DRB1).read(), dict(target_poa_length=700, n_haps=12, max_path_jump=5000, max_edge_jump=5000,
                                                            max_poa_length=300, repeats=(40, 300, 3.0, 3)))]


def blocks_of(text, conf):
    sm = S.Smoother(text, discover=conf)
    try:
        return [sm.block_ranges(k) for k in range(sm.n_blocks)], getattr(sm, "break_counts", None)
    finally:
        sm.close()


@pytest.fixture(scope="module")
def discovered():
    return {name: (text(), conf, blocks_of(text(), conf)[0]) for name, text, conf in DISCOVER}


@pytest.mark.parametrize("name", [d[0] for d in DISCOVER])
def test_discovery_with_the_scanner_gives_the_same_blocks(engine, discovered, name):
    text, conf, host = discovered[name]
    got, counts = blocks_of(text, dict(conf, scanner=S.gpu_repeat_scanner(engine)))
    assert got == host
    assert counts[0] >= 1 and counts[1] >= 1 and counts[2] == 0, counts
    assert engine.stats()["dp_launches"] == 2                              # ONE provider call, one round


def test_discovery_through_a_group_member(discovered):
    group = P.PoaGroup([0, 0])
    try:
        for name in ("chain", "drb1-scaled"):
            text, conf, host = discovered[name]
            assert blocks_of(text, dict(conf, scanner=S.gpu_repeat_scanner(group.member(1))))[0] == host
    finally:
        group.close()

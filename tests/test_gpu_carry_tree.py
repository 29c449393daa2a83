"""Pass 1 of the packed sweep builds the strips' carries a and b as trees of three-input maxima in the local classes compiled
for the default scores: smoothxg_amd/csrc/poa_dp16_row.inc.h (part 1), argument in smoothxg_amd/csrc/poa_fields.h
(p16_carry_leaf_bottom).  The carries decide when an in-row gap leaves the strip it opened in.

Every case is ONE batch of three-sequence blocks on a forced geometry, as in tests/test_gpu_strip_gap.py: `base`; `base` with a
substitution every 41st letter; `base` with ONE random insertion of n letters whose first letter stands in column `col` of the
sweep (column j holds letter j - 1).  The third sequence -- the carrier -- then scores L - min(6 + 2 (n - 1), 26 + (n - 1)) and
the block has L + #substitutions + n nodes.  The gap opens behind the H of column col - 1, so that column's leaf has to hold the
winner of its strip's tree:
  * n = W + 2 at every phase of one strip: the SHORT piece decides (n <= 15 < 21) and the gap always leaves its strip -- each of
    the W leaves of a in turn;
  * n = 30 at every phase: the LONG piece decides -- the same for b;
  * n = 1 and 2 opening in the last column of a strip and in the first column of the next: with more than one wave that
    boundary is a wave's edge, columns 128 W k - 1 and 128 W k.
The closed form is asserted on the ORACLE's output first, then the engine's result equals the oracle's on the default-score
class and on the generic class (SXG_POA_NO_DEFAULT_CLASS: the running form of the carries), the geometry is asserted from
engine.stats() and retries == 0 (a wrong sweep that the widening ladder repairs would still equal the oracle).

Geometries: one wave at every W = 4 .. 12 -- every leaf count and so every tree shape --, (8,2), (10,4) and (11,4) with twin and
join rows, (12,8), (13,16), the last two forced at a short L.  The classes of (10,4), (11,4) and (12,8) have a second width W - 1,
which would take every sequence short enough for a quick test: those cases run under SXG_POA_WIDTH2=0 (every alignment at the
geometry's width) and every case asserts that all its sweeps ran at W."""
import numpy as np
import pytest

from helpers import assert_block_equal, gparams, oparams

pytestmark = pytest.mark.gpu

G, E, Q, C = 6, 2, 26, 1


def gap_cost(n):
    return min(G + E * (n - 1), Q + C * (n - 1))


def make_block(rng, L, col, n):
    """(base, base with substitutions, carrier); the insertion can stand nowhere else: its ends differ from the letters beside it."""
    base = rng.integers(0, 4, L, dtype=np.uint8)
    subs = base.copy()
    subs[40::41] = (subs[40::41] + 1) % 4
    ins = rng.integers(0, 4, n, dtype=np.uint8)
    a = col - 1                        # letters of base in front of the insertion
    assert 60 < a < L - 60
    if n == 1:
        ins[0] = next(x for x in range(4) if x != base[a] and x != base[a - 1])
    else:
        if ins[0] == base[a]:
            ins[0] = (ins[0] + 1) % 4      # (else the gap could open a column later)
        if ins[-1] == base[a - 1]:
            ins[-1] = (ins[-1] + 1) % 4    # (else it could open a column earlier)
    return [base, subs, np.concatenate([base[:a], ins, base[a:]])]


def placements(W, boundary, phase_strip):
    """(col, n): n = W + 2 and n = 30 at every phase of strip `phase_strip`; n = 1, 2 in the last column in front of the strip
    boundary `boundary` (a column, a multiple of W) and in the first column behind it."""
    out = [(phase_strip * W + p, W + 2) for p in range(W)]
    out += [(phase_strip * W + p, 30) for p in range(W)]
    out += [(boundary - 1, n) for n in (1, 2)] + [(boundary, n) for n in (1, 2)]
    return out


# name: (seed, L, (W, waves), the class has a second width, strip boundary that takes n = 1, 2, strip whose phases take the rest,
#        twin rows expected)
# (L: more than four letters behind the last substitution, or the local alignment of the second sequence drops its end)
CASES = {"one_wave_w%d" % W: (3200 + W, 100 * W + (10 if W == 7 else 0), (W, 1), False, 30 * W, 50, False) for W in range(4, 13)}
CASES.update({
    "two_waves": (3221, 1610, (8, 2), False, 1024, 150, False),
    # (the first two waves hold letters: the boundary is the edge between them, the phases' strip lies in the second)
    "four_waves_w10": (3222, 2000, (10, 4), True, 1280, 150, True),
    "four_waves_w11": (3223, 2200, (11, 4), True, 1408, 150, True),
    "eight_waves_w12": (3224, 2310, (12, 8), True, 1536, 150, False),
    "sixteen_waves_w13": (3225, 2310, (13, 16), False, 1664, 150, False),
})

_cache = {}


def case_blocks(oracle, name):
    """The case's blocks with the oracle's result of each, computed once."""
    if name not in _cache:
        seed, L, (W, waves), _, boundary, strip, _ = CASES[name]
        rng = np.random.default_rng(seed)
        impl = oracle.IMPL_AVX2 if oracle.simd_available() else oracle.IMPL_SCALAR
        out = []
        for col, n in placements(W, boundary, strip):
            seqs = make_block(rng, L, col, n)
            out.append((col, n, seqs, oracle.block_run(seqs, None, oparams("convex_default", 0), impl=impl)))
        _cache[name] = out
    return _cache[name]


def check_closed_form(name, L, blocks):
    nsubs = len(range(40, L, 41))
    for col, n, seqs, (g, sc, cells) in blocks:
        label = f"{name}: insertion of {n} at column {col}"
        assert int(sc[2]) == L - gap_cost(n), (label, list(sc))
        assert len(g.nodes()[0]) == L + nsubs + n, label


def run_both_classes(engine, monkeypatch, name, batch, expect, geometry, dual, twin):
    """twin: True -- twin and join rows expected; False -- not asserted; None -- retries are not held at 0 either."""
    W, waves = geometry
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.setenv("SXG_POA_FORCE_P16", "%d,%d" % (W, waves))
    if dual:
        monkeypatch.setenv("SXG_POA_WIDTH2", "0")
    else:
        monkeypatch.delenv("SXG_POA_WIDTH2", raising=False)
    for env, label in ((None, "default-score class"), ("1", "generic class")):
        if env is None:
            monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
        else:
            monkeypatch.setenv("SXG_POA_NO_DEFAULT_CLASS", env)
        res = engine.run_blocks(batch, gparams("convex_default", 0))
        st = engine.stats()
        monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
        print(f"{name}/{label}: {st['dom_threads']} threads x {st['dom_cols_per_lane']} columns per lane, row mode {st['dom_row_mode']}, "
              f"widths {st['dom_width']}/{st['dom_width2']}, sweeps {st['width_sweeps']}, twin steps {st['twin_steps']}, "
              f"join rows {st['join_rows']}, retries {st['retries']}")
        assert (st["dom_row_mode"], st["dom_threads"], st["dom_cols_per_lane"], st["dom_width"], st["dom_width2"]) == (2, 64 * waves, 2 * W, W, 0), st
        # every sweep at W, none at the second width: two per block, more only where a block is run again
        assert st["width_sweeps"][0] >= 2 * len(batch) and st["width_sweeps"][1] == 0, st
        if twin is not None:
            assert st["retries"] == 0 and st["width_sweeps"][0] == 2 * len(batch), st
        if twin:
            assert st["twin_steps"] > 0 and st["join_rows"] > 0, st
        for b, (g, sc, cells) in enumerate(expect):
            assert_block_equal(res[b], g, sc, cells, label=f"{name}/{label}/block {b}")


@pytest.mark.parametrize("name", list(CASES))
def test_every_leaf_of_both_carry_trees_decides(engine, oracle, monkeypatch, name):
    seed, L, geometry, dual, boundary, strip, twin = CASES[name]
    W, waves = geometry
    blocks = case_blocks(oracle, name)
    assert W + 2 < 21 <= 30   # the short piece decides the first family, the long piece the second
    for n in (W + 2, 30):
        assert {col % W for col, m, _, _ in blocks if m == n} == set(range(W))   # every phase of a strip
    assert boundary % W == 0 and {(boundary - 1, 1), (boundary - 1, 2), (boundary, 1), (boundary, 2)} <= {(col, n) for col, n, _, _ in blocks}
    if waves > 1:
        assert boundary % (128 * W) == 0 and 0 < boundary < 128 * W * waves   # a wave's edge
    assert (L - 41) % 41 > 4 and L + 30 + 1 <= 128 * W * waves
    check_closed_form(name, L, blocks)
    run_both_classes(engine, monkeypatch, name, [seqs for _, _, seqs, _ in blocks], [r for _, _, _, r in blocks], geometry, dual, twin)


def test_unrelated_sequences_sit_at_the_clamp_leaf(engine, oracle, monkeypatch):
    """Nothing in common: almost every H is at or below the bias, so nearly every carry is the clamp leaf of its tree."""
    rng = np.random.default_rng(3226)
    batch = [[rng.integers(0, 4, 2500, dtype=np.uint8) for _ in range(3)] for _ in range(2)]
    impl = oracle.IMPL_AVX2 if oracle.simd_available() else oracle.IMPL_SCALAR
    expect = [oracle.block_run(seqs, None, oparams("convex_default", 0), impl=impl) for seqs in batch]
    assert max(int(max(sc)) for _, sc, _ in expect) < 60
    # (nearly every base a new node: the graph may outgrow its first tier -- retries are not held at 0 here)
    run_both_classes(engine, monkeypatch, "unrelated", batch, expect, (11, 4), True, None)

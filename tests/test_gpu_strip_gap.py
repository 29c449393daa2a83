"""Pass 2 of the packed sweep without the in-strip state of the long gap piece (classes compiled for the default scores), the
local clamp carried in E: smoothxg_amd/csrc/poa_dp16_row.inc.h, argument in smoothxg_amd/csrc/poa_fields.h.

Every case is ONE batch of three-sequence blocks on a forced geometry: `base`; `base` with a substitution every 41st letter
(bubbles: the third alignment meets twin and join rows); `base` with ONE random insertion of n letters whose first letter stands
in column `col` of the sweep (column j holds letter j - 1).  The third sequence -- the carrier -- then scores
L - min(6 + 2 (n - 1), 26 + (n - 1)) and the block has L + #substitutions + n nodes: from n = 22 on the LONG piece decides, and it
has to be carried over n columns -- two to nineteen strips, a wave's edge where the case puts one -- by the strips' carries
alone.  The closed form is asserted on the ORACLE's output first (the long piece decided, the alignment bridged the insertion),
then the engine's result equals the oracle's on the default-score class and on the generic class
(SXG_POA_NO_DEFAULT_CLASS: unchanged code, per-column Q).

Insertions stand relative to the geometry the case asserts from engine.stats(): in the last column of a wave (128 W k - 1), in
the first column of the next, at every phase of one strip (W consecutive columns), with n in {21, 22, 23, 30, 150}."""
import numpy as np
import pytest

from helpers import assert_block_equal, gparams, oparams

pytestmark = pytest.mark.gpu

G, E, Q, C = 6, 2, 26, 1
NS = (21, 22, 23, 30, 150)


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
    if ins[0] == base[a]:
        ins[0] = (ins[0] + 1) % 4      # (else the gap could open a column later)
    if ins[-1] == base[a - 1]:
        ins[-1] = (ins[-1] + 1) % 4    # (else it could open a column earlier)
    return [base, subs, np.concatenate([base[:a], ins, base[a:]])]


def placements(W, edges, phase_strip):
    """(col, n): every n at the last column of the first wave edge and at the first column behind it, two n at the further
    edges, n = 30 at every phase of strip `phase_strip`."""
    out = []
    for x, edge in enumerate(edges):
        for n in (NS if x == 0 else (22, 150)):
            out += [(edge - 1, n), (edge, n)]
    out += [(phase_strip * W + p, 30) for p in range(W)]
    if not edges:
        out += [(phase_strip * W + W - 1, n) for n in NS if n != 30] + [(phase_strip * W, n) for n in NS if n != 30]
    return out


# name: (seed, L, mode, (W, waves), wave edges with an insertion, strip whose W phases take one, twin rows expected)
CASES = {
    "one_wave": (3101, 710, 0, (10, 1), (), 33, False),
    "two_waves": (3102, 1300, 0, (8, 2), (1024,), 70, False),
    "four_waves_twin": (3103, 3000, 0, (8, 4), (1024, 2048), 200, True),
    "four_waves_global": (3104, 3000, 1, (8, 4), (1024, 2048), 131, True),
}

_cache = {}


def case_blocks(oracle, name):
    """The case's blocks with the oracle's result of each, computed once."""
    if name not in _cache:
        seed, L, mode, (W, waves), edges, strip, _ = CASES[name]
        rng = np.random.default_rng(seed)
        impl = oracle.IMPL_AVX2 if oracle.simd_available() else oracle.IMPL_SCALAR
        out = []
        for col, n in placements(W, edges, strip):
            seqs = make_block(rng, L, col, n)
            out.append((col, n, seqs, oracle.block_run(seqs, None, oparams("convex_default", mode), impl=impl)))
        _cache[name] = out
    return _cache[name]


def check_closed_form(name, L, blocks):
    nsubs = len(range(40, L, 41))
    for col, n, seqs, (g, sc, cells) in blocks:
        label = f"{name}: insertion of {n} at column {col}"
        assert int(sc[2]) == L - gap_cost(n), (label, list(sc))
        assert len(g.nodes()[0]) == L + nsubs + n, label


def run_both_classes(engine, monkeypatch, name, batch, expect, mode, geometry, twin):
    W, waves = geometry
    monkeypatch.setenv("SXG_POA_NO_SPREAD", "1")
    monkeypatch.setenv("SXG_POA_FORCE_P16", "%d,%d" % (W, waves))
    for env, label in ((None, "default-score class"), ("1", "generic class")):
        if env is None:
            monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
        else:
            monkeypatch.setenv("SXG_POA_NO_DEFAULT_CLASS", env)
        res = engine.run_blocks(batch, gparams("convex_default", mode))
        st = engine.stats()
        monkeypatch.delenv("SXG_POA_NO_DEFAULT_CLASS", raising=False)
        print(f"{name}/{label}: {st['dom_threads']} threads x {st['dom_cols_per_lane']} columns per lane, row mode {st['dom_row_mode']}, "
              f"widths {st['dom_width']}/{st['dom_width2']}, twin steps {st['twin_steps']}, join rows {st['join_rows']}, retries {st['retries']}")
        assert (st["dom_row_mode"], st["dom_threads"], st["dom_cols_per_lane"], st["dom_width"], st["dom_width2"]) == (2, 64 * waves, 2 * W, W, 0), st
        if twin is not None:
            assert st["retries"] == 0, st   # (a wrong sweep that the widening ladder repairs would still equal the oracle)
        if twin:
            assert st["twin_steps"] > 0 and st["join_rows"] > 0, st
        for b, (g, sc, cells) in enumerate(expect):
            assert_block_equal(res[b], g, sc, cells, label=f"{name}/{label}/block {b}")


@pytest.mark.parametrize("name", list(CASES))
def test_long_piece_crosses_strips_and_wave_edges(engine, oracle, monkeypatch, name):
    seed, L, mode, geometry, edges, strip, twin = CASES[name]
    blocks = case_blocks(oracle, name)
    assert {n for _, n, _, _ in blocks} == set(NS)
    assert {col % geometry[0] for col, n, _, _ in blocks if n == 30} == set(range(geometry[0]))   # every phase of a strip
    for edge in edges:
        assert edge % (128 * geometry[0]) == 0 and {edge - 1, edge} <= {col for col, _, _, _ in blocks}
    check_closed_form(name, L, blocks)
    run_both_classes(engine, monkeypatch, name, [seqs for _, _, seqs, _ in blocks], [r for _, _, _, r in blocks], mode, geometry, twin)


def test_unrelated_sequences_sit_at_the_bias(engine, oracle, monkeypatch):
    """Nothing in common: almost every H is the bias, so E enters nearly every strip at its floor and the words that cross the
    wave edges are floored ones."""
    rng = np.random.default_rng(3105)
    batch = [[rng.integers(0, 4, 2500, dtype=np.uint8) for _ in range(3)] for _ in range(2)]
    impl = oracle.IMPL_AVX2 if oracle.simd_available() else oracle.IMPL_SCALAR
    expect = [oracle.block_run(seqs, None, oparams("convex_default", 0), impl=impl) for seqs in batch]
    assert max(int(max(sc)) for _, sc, _ in expect) < 60
    # (nearly every base a new node: the graph may outgrow its first tier -- retries are not held at 0 here)
    run_both_classes(engine, monkeypatch, "unrelated", batch, expect, 0, (8, 4), None)

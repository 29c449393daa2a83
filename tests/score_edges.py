"""Score sets at the edge of every sweep's admitted range: the cases of tests/test_score_edges.py (CPU: the oracle and the
model of the host's choice alone) and tests/test_gpu_score_edges.py (GPU: every case against the live scalar oracle), stated
once.  A plain module, no test.

The host chooses a sweep per block from the score set and the longest sequence (sxg_poa.hip: p16_safe, h16_safe, row_mode,
plane_cell_bytes, band_cell_bytes, classify_block) and the kernels rest on those admission rules with no run-time check
(poa_fields.h).  Every case here sits ON one of the rules: the last input a sweep admits, or the first it does not.

The EXPECTED sweep of a case is written down as a literal (`rm`, `cb`, `geometry`) and, independently, computed by the second
statement of the host's choice, tests/golden/make_class_matrix.py (row_mode, cell_bytes, variant_for_len, class_tmax,
normalise); tests/test_score_edges.py holds the two equal and holds the inputs to the limits they are said to reach.  Nothing
here is read back from the engine."""
import os
import sys

import numpy as np

from helpers import random_block

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_class_matrix as M  # noqa: E402

DEFAULT = (1, -4, -6, -2, -26, -1)
LOCAL_LIMIT = 30000          # poa_fields.h: P16_LOCAL_LIMIT; sxg_poa.hip: h16_safe
CLAMP_LIMIT = 14500          # sxg_poa.hip: p16_safe with clamp_ok (whole blocks, global, no band)
STRICT_LIMIT = 15800         # sxg_poa.hip: p16_safe, the strict rule (align-only, banded)
BYTE_LIMIT = 120             # sxg_poa.hip: p16_safe -- the one-byte gap distances of stored rows

# (m, n, g, e, q, c) in spoa's sign convention
EDGE_SETS = {
    "top4": (127, -128, -119, -60, -120, -1),        # int8 extremes, convex: 22 code bits, 4-byte cells
    "top4a": (127, -128, -120, -60, -120, -1),       # ... with g = q: affine to the kernels, 15 code bits, 2-byte cells
    "lin120": (127, -128, -120, -120, -120, -120),   # linear: the largest (W - 1) |e| above H in a biased field; 9 code bits
    "top2": (29, -4, -6, -2, -26, -1),               # 2-byte cells, the generic class (not DS)
    "q120": (3, -5, -100, -3, -120, -1),             # the last set the packed sweep takes, convex
    "q121": (3, -5, -100, -3, -121, -1),             # the first on int16 row words
    "g121": (3, -5, -121, -3, -128, -1),             # both openings beyond a byte, q at the int8 end
    "lin121": (1, -4, -121, -121, -121, -121),       # the kernel's own range re-check (int16 -> int32 row words)
}
# the borders of the gap-model choice (S1): linear from g = e, affine from g = q or e = c
BORDER_SETS = {
    "g_eq_e": (2, -4, -5, -5, -30, -1),
    "g_eq_q": (2, -4, -10, -3, -10, -1),
    "e_eq_c": (2, -4, -6, -2, -20, -2),
    "g_lt_q": (2, -4, -30, -1, -6, -2),
}
BORDER_MODELS = {"g_eq_e": "linear", "g_eq_q": "affine", "e_eq_c": "affine", "g_lt_q": "affine"}


def near_default_sets():
    """the default set with each field moved by one, in each direction that leaves a valid set (m >= 0, the others <= 0)"""
    out = {}
    for i, name in enumerate("mngeqc"):
        for d in (-1, 1):
            s = list(DEFAULT)
            s[i] += d
            if s[0] >= 0 and all(v <= 0 for v in s[1:]):
                out["%s%+d" % (name, d)] = tuple(s)
    return out


NEAR_DEFAULT_SETS = near_default_sets()
ALL_SETS = dict(EDGE_SETS, **BORDER_SETS, **NEAR_DEFAULT_SETS)


def model_name(scores):
    m, n, g, e, q, c, convex = M.normalise(scores)
    return "convex" if convex else ("linear" if g == e else "affine")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: random over four letters, an N (code 4) every ~50 letters in ONE sequence of each block (never the first two, so that
# the second sequence of a near-identical block still matches the first letter for letter)

def _sprinkle_n(s, rng):
    s = s.copy()
    s[int(rng.integers(10, 40))::50] = 4
    return s


def near_identical_block(L, seed):
    """[a, a, a without 10 letters (and with the Ns), a with 6 letters inserted and three substituted]; len(a) = L and no
    sequence is longer: the fourth is built on a's first L - 6 letters."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, L, dtype=np.uint8)
    cut = L // 3
    c = _sprinkle_n(np.concatenate([a[:cut], a[cut + 10:]]), rng) if L > 30 else a.copy()
    at = 2 * L // 3
    d = np.concatenate([a[:at], rng.integers(0, 4, 6, dtype=np.uint8), a[at:L - 6]])
    for p in rng.choice(L, 3, replace=False):
        d[p] = (d[p] + 1) & 3
    assert len(d) == L
    return [a, a.copy(), c, d]


def clean_pair_block(L, seed):
    """[a, a with five substitutions]: a global walk of the second sequence never falls below -5 * (m - n)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, L, dtype=np.uint8)
    b = a.copy()
    for p in rng.choice(L, 5, replace=False):
        b[p] = (b[p] + 1) & 3
    return [a, b]


def divergent_block(L, seed):
    """[a, a with 12 % substitutions (and the Ns), an unrelated sequence], all of L letters"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 4, L, dtype=np.uint8)
    b = a.copy()
    for p in rng.choice(L, max(1, (12 * L + 99) // 100), replace=False):
        b[p] = (b[p] + 1 + int(rng.integers(0, 3))) & 3
    return [a, _sprinkle_n(b, rng), rng.integers(0, 4, L, dtype=np.uint8)]


def disjoint_block(L, seed):
    """[a, a with 12 % substitutions (and the Ns), a sequence that shares no letter with them]: a and b over {A, C}, the third
    over {G, T}, all of L letters -- the third sequence's global alignment holds no match at all"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, L, dtype=np.uint8)
    b = a.copy()
    for p in rng.choice(L, max(1, (12 * L + 99) // 100), replace=False):
        b[p] ^= 1
    return [a, _sprinkle_n(b, rng), rng.integers(2, 4, L, dtype=np.uint8)]


def short_tail(seqs, seed):
    """... with one sequence of 10 letters added (an N among them)"""
    t = np.random.default_rng(seed + 77).integers(0, 4, 10, dtype=np.uint8)
    t[5] = 4
    return seqs + [t]


def indel_block(L, seed):
    """random_block(3 sequences, 4 % divergence) plus its first sequence without 40 letters (and with the Ns) and with 40
    letters inserted: gaps long enough for the second gap piece to decide cells"""
    rng = np.random.default_rng(seed)
    seqs = random_block(rng, 3, L, div=0.04)
    a = seqs[0]
    n = len(a)
    seqs.append(_sprinkle_n(np.concatenate([a[:n // 3], a[n // 3 + 40:]]), rng))
    seqs.append(np.concatenate([a[:2 * n // 3], rng.integers(0, 4, 40, dtype=np.uint8), a[2 * n // 3:]]))
    return seqs


BUILDERS = {"near": near_identical_block, "clean": clean_pair_block, "divergent": divergent_block, "disjoint": disjoint_block, "indel": indel_block}


# ---------------------------------------------------------------------------------------------------------------------------
# the model of the host's choice (make_class_matrix.py), extended by the band (sxg_poa.hip: sxg_poa_batch_upload; decree B2)

def band_strip_width(maxlen):
    w = min(311 + int(0.03 * maxlen), 693)
    return 6 if 2 * w <= 756 else (8 if 2 * w <= 1008 else 11)


def expected_block(scores, mode, maxlen, banded=0, env=None):
    """dict(rm, cb, W, NW, tmax, ds, threads, cols_per_lane) of the FIRST launch of a block: mode 0 = local, 1 = global"""
    env = env or {}
    sw = mode == 0
    rm = M.row_mode(scores, sw, maxlen, maxlen, no_packed="SXG_POA_NO_PACKED" in env, clamp_ok=banded == 0)
    knob4 = env.get("SXG_POA_CELL_BYTES") == "4"
    cb = M.cell_bytes(scores, knob4) if rm == 2 else 4
    if banded and (sw or banded == 2) and rm == 2:
        W, NW, rm = band_strip_width(maxlen), 1, 3
        cb = cb if sw else 4
        tmax = 64
    else:
        force = tuple(int(x) for x in env["SXG_POA_FORCE_P16"].split(",")) if "SXG_POA_FORCE_P16" in env else None
        W, NW = M.variant_for_len(maxlen, rm, sw, force=force)
        tmax = M.class_tmax(NW, rm, cb)
    ds = int(rm == 2 and cb == 2 and tuple(scores) == DEFAULT)
    return dict(rm=rm, cb=cb, W=W, NW=NW, tmax=tmax, ds=ds, threads=64 * NW, cols_per_lane=W * (2 if rm >= 2 else 1))


def next_step(scores, mode, maxlen, rm):
    """the row mode of the re-run after ST_RANGE_OVERFLOW on row mode rm (sxg_poa.hip: advance_ladders)"""
    if rm == 0:
        return 1
    return M.row_mode(scores, mode == 0, maxlen, maxlen, no_packed=True)


def nodes_before(oracle, case, seqs):
    """graph rows in front of every sequence of a global block, from the oracle's own graph (None: a local block, no re-check)"""
    if case["mode"] == 0:
        return None
    p = oracle.mkparams(*case["scores"], mode=case["mode"])
    return [0] + [oracle.block_run(seqs[:k], None, p)[0].n_nodes for k in range(1, len(seqs))]


def expected_ladder(case, seqs, before):
    """The row modes of a block's launches, first to last (sxg_poa.hip: advance_ladders), from the oracle's row counts `before`
    every sequence.  Int16 row words and the band re-check the all-gap floor in front of every sequence, with the true row count
    (poa_kernels.hip.h: ST_RANGE_OVERFLOW), exactly as global_floor does.  A packed global sweep without a band is re-run when
    its walk visits a cell at or below -16 000 + m L + m, which no row count tells: the case says it (edge "clamp_rerun": the
    walk ends there; builder "clean": it cannot get there), and where it does not, the entry is the pair (2, None) and the
    caller takes what it sees."""
    scores, mode = case["scores"], case["mode"]
    maxlen = max(len(s) for s in seqs)
    rm = case_expected(case, seqs)["rm"]
    out = []
    while True:
        out.append(rm)
        if rm == 1 or mode == 0:
            return out
        if rm == 2:
            if case["edge"] == "clamp_rerun":
                again = True
            elif case["builder"] in ("clean", "near", "indel"):
                again = False
            else:
                out[-1] = (2, None)
                return out
        else:
            limit = STRICT_LIMIT if rm == 3 else LOCAL_LIMIT
            again = any(global_floor(scores, len(s), n) >= limit for s, n in zip(seqs[1:], before[1:]))
        if not again:
            return out
        rm = next_step(scores, mode, maxlen, rm)


def final_geometry(case, seqs, rm):
    """(threads, columns per lane) of a re-run on row mode rm: no forced geometry, no band"""
    W, NW = M.variant_for_len(max(len(s) for s in seqs), rm, case["mode"] == 0)
    return 64 * NW, W * (2 if rm >= 2 else 1)


def expected_align(scores, mode, qlen, rows):
    """the align-only API: the strict rule on the graph's real row count, 4-byte cells, no DS class"""
    sw = mode == 0
    rm = M.row_mode(scores, sw, qlen, rows)
    W, NW = M.variant_for_len(qlen, rm, sw)
    return dict(rm=rm, cb=4, W=W, NW=NW, tmax=M.class_tmax(NW, rm, 4), ds=0, threads=64 * NW, cols_per_lane=W * (2 if rm >= 2 else 1))


def global_floor(scores, qlen, rows):
    """-(the all-gap path): what h16_safe / p16_safe and the kernel's re-check compare with 30 000 / 15 800"""
    return -(M.gap_cost(scores, rows) + M.gap_cost(scores, qlen))


# ---------------------------------------------------------------------------------------------------------------------------
# the block cases of section 3 (a .. f): what is run, and the sweep each case NAMES (literals: rm, cb, geometry = (W, NW))

def _case(cid, sets, mode, builder, L, rm, cb, geometry, banded=0, env=None, tail=False, edge=None, seed=0):
    return dict(id=cid, set=sets, scores=EDGE_SETS[sets], mode=mode, builder=builder, L=L, rm=rm, cb=cb, geometry=geometry, banded=banded,
                env=dict(env or {}), tail=tail, edge=edge, seed=seed or (1000 * L + 7 * len(cid)))


FORCED = ("9,4", "8,8", "13,16")
NATURAL_LOCAL = {"top4": (4, 1), "top4a": (4, 1), "lin120": (4, 1), "top2": (9, 1)}
LOCAL_CB = {"top4": 4, "top4a": 2, "lin120": 2, "top2": 2}
LOCAL_AT = {"top4": 236, "top4a": 236, "lin120": 236, "top2": 1034}


def block_cases():
    cases = []
    # a. local, at the admission limit: m L < 30 000 holds by less than one m
    for name, L in LOCAL_AT.items():
        cases.append(_case("a/%s/L%d" % (name, L), name, 0, "near", L, 2, LOCAL_CB[name], NATURAL_LOCAL[name], edge="local_at"))
        for f in FORCED:
            g = tuple(int(x) for x in f.split(","))
            cases.append(_case("a/%s/L%d/force%s" % (name, L, f), name, 0, "near", L, 2, LOCAL_CB[name], g, env={"SXG_POA_FORCE_P16": f}, edge="local_at"))
    # (no linear set needs more than 9 code bits: lin120 reaches the 4-byte classes through the knob, like top2)
    cases.append(_case("a/top2/L1034/cb4", "top2", 0, "near", 1034, 2, 4, (9, 1), env={"SXG_POA_CELL_BYTES": "4"}, edge="local_at"))
    cases.append(_case("a/lin120/L236/cb4", "lin120", 0, "near", 236, 2, 4, (4, 1), env={"SXG_POA_CELL_BYTES": "4"}, edge="local_at"))
    cases.append(_case("a/lin120/L236/cb4/force13,16", "lin120", 0, "near", 236, 2, 4, (13, 16), env={"SXG_POA_CELL_BYTES": "4", "SXG_POA_FORCE_P16": "13,16"}, edge="local_at"))
    # b. one letter past it: int32 row words, no knob
    for name, L, g in (("top4", 237, (8, 1)), ("top4a", 237, (8, 1)), ("lin120", 237, (8, 1)), ("top2", 1035, (12, 2)), ("top4", 511, (8, 1))):
        cases.append(_case("b/%s/L%d" % (name, L), name, 0, "near", L, 1, 4, g, edge="local_past"))
    # c. byte-wide gap distances: |g|, |q| of 120 against 121
    for L in (300, 900):
        for mode in (0, 1):
            packed_g = {(300, 0): (4, 1), (300, 1): (4, 1), (900, 0): (8, 1), (900, 1): (8, 1)}[(L, mode)]
            wide_g = {300: (8, 1), 900: (16, 1)}[L]
            tag = "local" if mode == 0 else "global"
            cases.append(_case("c/q120/%s/L%d" % (tag, L), "q120", mode, "indel", L, 2, 4, packed_g, edge="byte"))
            cases.append(_case("c/q120/%s/L%d/no_packed" % (tag, L), "q120", mode, "indel", L, 0, 4, wide_g, env={"SXG_POA_NO_PACKED": "1"}, edge="byte"))
            cases.append(_case("c/q121/%s/L%d" % (tag, L), "q121", mode, "indel", L, 0, 4, wide_g, edge="byte"))
            cases.append(_case("c/g121/%s/L%d" % (tag, L), "g121", mode, "indel", L, 0, 4, wide_g, edge="byte"))
    # d. global thresholds of whole blocks (banded = 0): m L + m < 14 500
    for L, rm, g in ((113, 2, (4, 1)), (114, 0, (8, 1))):
        cases.append(_case("d/top4/clean/L%d" % L, "top4", 1, "clean", L, rm, 4, g, tail=True, edge="clamp"))
        cases.append(_case("d/top4/divergent/L%d" % L, "top4", 1, "divergent", L, rm, 4, g, tail=True, edge="clamp"))
    # ... and a block whose walk certainly ends below -16 000 + m L + m, where cells may be clamped ones: the third sequence
    # shares no letter with the graph.  The packed sweep says so and the block is re-run on int16 row words.
    cases.append(_case("d/lin120/disjoint/L113", "lin120", 1, "disjoint", 113, 2, 2, (4, 1), tail=True, edge="clamp_rerun"))
    # e. the kernel's own re-check, int16 -> int32 row words: 121 (N + len) >= 30 000 from N = 128 on at len = 120
    cases.append(_case("e/lin121/divergent/L120", "lin121", 1, "divergent", 120, 0, 4, (8, 1), edge="recheck_fires"))
    cases.append(_case("e/lin121/near/L120", "lin121", 1, "near", 120, 0, 4, (8, 1), edge="recheck_quiet"))
    cases.append(_case("e/lin121/near/L124", "lin121", 1, "near", 124, 1, 4, (8, 1), edge="h16_past"))      # 121 * 248 = 30 008: the host's own step
    # f. banded kernel
    for banded in (1, 2):
        for name, L in (("top4", 236), ("top2", 1034)):
            cases.append(_case("f/%s/L%d/band%d" % (name, L, banded), name, 0, "near", L, 3, LOCAL_CB[name], (6, 1), banded=banded, edge="local_at"))
        for name, L, g in (("top4", 237, (8, 1)), ("top2", 1035, (12, 2))):
            cases.append(_case("f/%s/L%d/band%d" % (name, L, banded), name, 0, "near", L, 1, 4, g, banded=banded, edge="local_past"))
    # ... global with the adaptive band: the strict rule holds on the host's row count (120 * 130 = 15 600) and fails on the true one
    cases.append(_case("f/lin120/global/L65/band2", "lin120", 1, "divergent", 65, 3, 4, (6, 1), banded=2, edge="strict_recheck"))
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


def case_seqs(case):
    seqs = BUILDERS[case["builder"]](case["L"], case["seed"])
    return short_tail(seqs, case["seed"]) if case["tail"] else seqs


def case_expected(case, seqs):
    return expected_block(case["scores"], case["mode"], max(len(s) for s in seqs), case["banded"], case["env"])


def oracle_banded(case, expected):
    """the band flag the oracle is asked for: the engine ignores it where the block does not run the banded kernel"""
    return case["banded"] if expected["rm"] == 3 and case["edge"] != "strict_recheck" else 0


# ---------------------------------------------------------------------------------------------------------------------------
# the align-only cases of section 3h: the graph of a block's first sequences, a query at (or cut to) the length the rule turns at

def align_cases():
    """(id, set, mode, builder, L, query length or None = the problem's own query, rm literal, edge).  The strict global rule has
    two halves.  m L < 15 800 turns between 124 and 125 letters for top4 and between 544 and 545 for top2, whose all-gap floor
    stays far away at these sizes.  floor < 15 800 is 120 (L + N) < 15 800 for lin120: the query is cut to a length chosen from
    the graph's real row count N (qlen = "sum131" / "sum132": L + N = 131 holds it, 132 breaks it).  q120 / q121 stay packed, or
    not, by |q| alone at any length a test can afford."""
    return [
        dict(id="h/top4/local/L236", set="top4", mode=0, builder="near", L=236, qlen=None, rm=2, edge="local_at"),
        dict(id="h/top4/local/L237", set="top4", mode=0, builder="near", L=237, qlen=None, rm=1, edge="local_past"),
        dict(id="h/top2/local/L1034", set="top2", mode=0, builder="near", L=1034, qlen=None, rm=2, edge="local_at"),
        dict(id="h/top2/local/L1035", set="top2", mode=0, builder="near", L=1035, qlen=None, rm=1, edge="local_past"),
        dict(id="h/top4/global/L124", set="top4", mode=1, builder="near", L=124, qlen=None, rm=2, edge="strict_at"),
        dict(id="h/top4/global/L125", set="top4", mode=1, builder="near", L=125, qlen=None, rm=0, edge="strict_past"),
        dict(id="h/lin120/global/sum131", set="lin120", mode=1, builder="near", L=70, qlen="sum131", rm=2, edge="strict_at"),
        dict(id="h/lin120/global/sum132", set="lin120", mode=1, builder="near", L=70, qlen="sum132", rm=0, edge="strict_past"),
        dict(id="h/top2/global/L544", set="top2", mode=1, builder="near", L=544, qlen=None, rm=2, edge="strict_at"),
        dict(id="h/top2/global/L545", set="top2", mode=1, builder="near", L=545, qlen=None, rm=0, edge="strict_past"),
        dict(id="h/q120/local/L300", set="q120", mode=0, builder="indel", L=300, qlen=None, rm=2, edge="byte"),
        dict(id="h/q121/local/L300", set="q121", mode=0, builder="indel", L=300, qlen=None, rm=0, edge="byte"),
        dict(id="h/q120/global/L300", set="q120", mode=1, builder="indel", L=300, qlen=None, rm=2, edge="byte"),
        dict(id="h/q121/global/L300", set="q121", mode=1, builder="indel", L=300, qlen=None, rm=0, edge="byte"),
    ]


def align_problem(case, oracle):
    """(codes, off, pred, sink, query) -- the graph is the oracle's.  An indel block: of every sequence but the last, the query.
    A near-identical block: of the first, third and fourth sequence, and the query is the second, the first's copy -- a local
    query then scores m L, the most its length can."""
    seqs = BUILDERS[case["builder"]](case["L"], 31 * case["L"] + len(case["set"]))
    scores = EDGE_SETS[case["set"]]
    first, q = ([seqs[0]] + seqs[2:], seqs[1]) if case["builder"] == "near" else (seqs[:-1], seqs[-1])
    g, _, _ = oracle.block_run(first, None, oracle.mkparams(*scores, mode=case["mode"]))
    codes, off, pred, sink, _ = g.rows()
    if case["qlen"] is not None:
        q = q[:int(case["qlen"][3:]) - len(codes)]
    return codes, off, pred, sink, q


# ---------------------------------------------------------------------------------------------------------------------------
# the campaign over the whole int8 domain (section 3i)

def random_scores_full(rng):
    """A valid score set anywhere in the int8 domain: m 1 .. 127, n -128 .. -1, gap scores down to -128, in the three gap models;
    the convex draws land on the borders g = e, g = q and e = c (a zero difference) about one time in eight each."""
    m = int(rng.integers(1, 128))
    n = -int(rng.integers(1, 129))
    kind = int(rng.integers(0, 3))
    step = lambda top: 0 if int(rng.integers(0, 8)) == 0 else int(rng.integers(1, top))
    if kind == 0:       # linear
        g = -int(rng.integers(1, 129)); e = q = c = g
    elif kind == 1:     # affine
        e = -int(rng.integers(1, 129)); g = max(-128, e - step(100)); q, c = g, e
    else:               # convex where every difference is positive
        c = -int(rng.integers(1, 65)); e = max(-128, c - step(48))
        g = max(-128, e - step(40)); q = max(-128, g - step(80))
    return m, n, g, e, q, c

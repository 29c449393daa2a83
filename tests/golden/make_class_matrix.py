"""Generates tests/golden/class_matrix.json, class_matrix_wide.json (family wide_match) and class_matrix_banded.json (kind "band"):
oracle results for one block (or one align-only problem) per built kernel class, each with sequences that FILL the class's geometry.

SELF-ORACLE fixtures (oracle/poa_oracle.c and its AVX2 twin, which tests/test_oracle.py holds equal to it; NOT reference-derived --
see the header of tests/golden/make_golden.py).  tests/test_gpu_class_matrix.py runs every case on the GPU and compares with the
committed values, tests/test_class_matrix_fixture.py checks without a GPU that the cases cover the built classes
(smoothxg_amd/csrc/poa_classes.h), that the inputs regenerate, and re-runs the small cases through the scalar oracle.  Both import
this module for the case list, the inputs and the model of the host's choice of a class.

Inputs.  synth.make_block(block_id, 3, length, sv_frac=0): three sequences with 1 % substitutions and small indels, no structural
variant (the traceback band is not the question here).  One 40-base deletion is spliced into the second sequence and one 40-base
insertion into the third, each straddling a wave boundary of the geometry -- column 128 * W * k of a packed sweep, 64 * W * k of
a 32-bit sweep, k >= 1 -- or, on one wave, a strip boundary (a multiple of W columns).  40 bases is past the crossover of the two
convex pieces (20 for the default scores), so an in-row gap in its second piece crosses the hand-over.  (length, block_id) are
searched until the longest sequence is capacity - 3 .. capacity - 1 letters long: the query spans every wave of the workgroup.
A geometry the chooser never picks by itself (another one with the same columns and a wider strip wins the tie) is marked
"force": the GPU test pins it with SXG_POA_FORCE_P16.  Sequences are handed over in the order drawn, not re-sorted.

Families (scores in spoa's sign convention):
  ds           1,4,6,2,26,1               the default-score class, 2-byte plane cells
  gen2_convex  1,9,16,2,41,1 (asm10)      the general class, all 16 code bits
  gen2_affine  1,4,6,2,6,2                the general class, affine
  cb4_convex   1,19,39,3,81,1 (asm5)      4-byte plane cells (20 code bits)
  cb4_affine   gen2_affine's cases run with SXG_POA_CELL_BYTES=4: with |g| <= 120 no affine set needs more than 15 code bits
               (H 8 + F 7), so the 4-byte affine classes are reachable through the knob only.  Results do not depend on the cell
               format: the cases share gen2_affine's expectations and have no entries of their own.
  wide_match   64,127,96,32,127,16        int32 row words by the scores alone (64 L >= 30 000 from 469 letters on, no knob): every
               geometry of the 32-bit sweep as a block and as an align-only problem, local and global
  banded       kind "band": the one-wave banded sweep (row mode 3), one block per strip width W = 6, 8, 11 (decree B2 of
               oracle/poa_oracle.c), its longest sequence within three letters of the LAST length on W = 6 (2 266) and on W = 8
               (6 466) and at the FIRST lengths with the capped half-width 693 (12 734 .. 12 740): there the band of a row spans
               127 - 128 of the window's 128 strips, so the window has no slack and re-centres at every second band move at the
               latest.  Local mode with the static (banded = 1) and the adaptive band (banded = 2) for gen2_convex, gen2_affine
               (2-byte band cells) and cb4_convex (4-byte); global mode, adaptive band (4-byte cells by rule), for ds (convex),
               gen2_affine and affine_e1 1,4,6,1,6,1 (affine).  The strict range rule bounds a global block (m L < 15 800 and
               the all-gap floor < 15 800 on the true row count): ds fills W = 6 and W = 8 and reaches W = 11 up to ~7 600
               letters, gen2_affine (e = -2) fills W = 6 and reaches W = 8 up to ~3 800, affine_e1 reaches W = 11 -- partial
               fills, the most a global block of these scores can do; such a case takes the longest length the model admits
               with 4 % more rows than letters, and records the oracle's row counts in front of every sequence ("rows_before"),
               on which the model says that no sweep is refused and re-run.  Expectations come from the scalar oracle (the AVX2
               twin is not held equal to it in banded mode); cells = band cells.
Expectations are in spoa's node order (mode | 0x10, the product default: the re-sort is a graph phase whose batch size differs
by class): scores, summed cells, node and edge counts, digests of nodes / edges / paths (make_fullshape.digest_block's arrays,
folded into three to keep the file small), no consensus.

    python tests/golden/make_class_matrix.py      (from the repository root; ~10 min of CPU over up to 16 processes; cases the
                                                   fixtures hold already are kept, the banded file alone takes ~10 s)
"""
import hashlib
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(HERE, "class_matrix.json")
FIXTURE_WIDE = os.path.join(HERE, "class_matrix_wide.json")   # the families added later (WIDE_FAMILIES): the first file keeps its bytes
WIDE_FAMILIES = ("wide_match",)
FIXTURE_BANDED = os.path.join(HERE, "class_matrix_banded.json")   # kind "band": the banded sweep's cases, one per line

SCORES = {
    "ds": (1, -4, -6, -2, -26, -1),
    "gen2_convex": (1, -9, -16, -2, -41, -1),
    "gen2_affine": (1, -4, -6, -2, -6, -2),
    "cb4_convex": (1, -19, -39, -3, -81, -1),
    "convex_heavy": (3, -5, -9, -3, -30, -1),
    "wide_match": (64, -127, -96, -32, -127, -16),
    "affine_e1": (1, -4, -6, -1, -6, -1),
}
BLOCK_FAMILIES = ("ds", "gen2_convex", "gen2_affine", "cb4_convex")
ALIGN_FAMILIES = ("cb4_convex", "gen2_affine")
# The strict range rule ends packed global align-only queries inside 8 waves x 8 columns (asm5: ~7 700 letters).  The wider
# global classes of the align-only kernel run that query again under SXG_POA_FORCE_P16: it reaches the seventh of eight waves at
# W = 9 and the fifth at W = 12 -- a partial fill, the most a global query of these scores can do.
ALIGN_GLOBAL_FORCED = ((9, 8), (10, 8), (11, 8), (12, 8), (8, 16))
FORCED_768_FAMILIES = ("ds", "gen2_convex", "cb4_convex")   # their (12,8) blocks are re-run on 12 waves x 8 columns (768 threads)
# the five tiers of adaptive_scores() (sxg_smooth.cpp), top identity first, and the plane cell bytes each must come out with
TIERS = ((1, -19, -39, -3, -81, -1), (1, -13, -31, -3, -51, -1), (1, -9, -16, -2, -41, -1), (1, -7, -11, -2, -33, -1), (1, -4, -6, -2, -26, -1))
TIER_CELL_BYTES = (4, 4, 2, 2, 2)
SPLICE = 40
# the banded sweep (kind "band"): (longest sequence from, to) per strip width -- to = the last length on W = 6 and on W = 8, from
# = the first length with the capped half-width at W = 11; and the score families of each (mode, gap model)
BAND_LENGTHS = {6: (2264, 2266), 8: (6464, 6466), 11: (12734, 12740)}
BAND_LOCAL_FAMILIES = ("gen2_convex", "gen2_affine", "cb4_convex")
BAND_GLOBAL_FAMILIES = {6: ("ds", "gen2_affine"), 8: ("ds", "gen2_affine"), 11: ("ds", "affine_e1")}
BAND_ROWS_MARGIN = 1.04   # rows per letter a partial global case is sized for (the oracle's count is recorded and asserted on)
MAX_SEQ_LEN = 26623       # SXG_POA_MAX_SEQ_LEN (include/sxg_poa.h)

# ---------------------------------------------------------------------------------------------------------------------------
# The host's choice of a class, written down a second time (sxg_poa.hip: p16_safe / h16_safe / row_mode / plane_cell_bytes,
# poa_classes.h: variant_for_len / class_tmax).  tests/test_class_matrix_fixture.py holds variant_for_len() equal to the
# recorded choice of tests/golden/geometry_choice.json.


def normalise(scores):
    """(m, n, g, e, q, c, convex) as the kernels see them"""
    m, n, g, e, q, c = scores
    if g >= e:
        return m, n, g, g, g, g, False
    if g <= q or e >= c:
        return m, n, g, e, g, e, False
    return m, n, g, e, q, c, True


def gap_cost(scores, k):
    _, _, g, e, q, c, _ = normalise(scores)
    return 0 if k <= 0 else max(g + (k - 1) * e, q + (k - 1) * c)


def code_bits(scores):
    """p16_delta_fits' arithmetic: the bits of a stored cell's three fields"""
    m, _, g, e, q, c, convex = normalise(scores)
    bits = lambda n: max(0, (n - 1).bit_length())
    return bits(m - 2 * g + 1) + bits(e - g + 1) + (bits(c - q + 1) if convex else 0)


def cell_bytes(scores, knob4=False):
    return 4 if knob4 or code_bits(scores) > 16 else 2


def row_mode(scores, sw, maxlen, rows, no_packed=False, clamp_ok=False):
    m, _, g, _, q, _, _ = normalise(scores)
    floor = 0 if sw else -(gap_cost(scores, rows) + gap_cost(scores, maxlen))
    packed = not no_packed and abs(g) <= 120 and abs(q) <= 120
    if packed and sw:
        packed = abs(m) * maxlen < 30000
    elif packed:
        packed = abs(m) * maxlen < 15800 and (abs(m) * maxlen + abs(m) < 14500 if clamp_ok else floor < 15800)
    if packed:
        return 2
    return 0 if abs(m) * maxlen < 30000 and floor < 30000 else 1


def variant_for_len(maxlen, rm, sw, force=None):
    """(W, NW) or None"""
    if rm == 2 and force and 128 * force[0] * force[1] >= maxlen + 1:
        return tuple(force)
    best = None
    for W in ((13, 12, 11, 10, 9, 8, 7, 6, 5, 4) if rm == 2 else (16, 12, 8)):
        for NW in (1, 2, 3, 4, 8, 12, 16):
            cols = 64 * NW * W * (2 if rm == 2 else 1)
            if cols < maxlen + 1:
                continue
            wide = W > 8 if rm == 2 else W > 12
            long_class = rm == 2 and sw and NW == 16 and W in (10, 12, 13)
            if (W == 13 and not long_class) or (rm == 2 and W < 8 and NW > 4) or (wide and NW > 8 and not long_class):
                continue
            if best is None or cols < best[0]:
                best = (cols, W, NW)
            break
    return best[1:] if best else None


def class_tmax(NW, rm, cb):
    """class_tmax of a plane that keeps every strip"""
    if rm == 2 and cb == 2 and NW <= 4:
        return 64 * NW
    return 256 if NW <= 4 else (512 if NW <= 8 else 1024)


def capacity(W, NW, rm):
    return 64 * NW * W * (2 if rm == 2 else 1)


def second_width(W, NW, cb):
    """class_w2: the 2-byte classes of 4 and 8 waves, W = 9 .. 12"""
    return W - 1 if cb == 2 and NW in (4, 8) and 9 <= W <= 12 else 0


# Row mode 3, the banded sweep (sxg_poa.hip, upload: the `bnd && (sw || bnd == 2) && rm == 2` branch; decrees B1, B2 of
# oracle/poa_oracle.c).  tests/test_class_matrix_fixture.py holds band_strip_width() equal to the oracle's
# poa_band_strip_width for every length; the product's own copy lives in a HIP header, and the GPU test holds it through the
# variant line of every banded case.

def band_half_width(L):
    return min(311 + int(0.03 * L), 693)


def band_strip_width(maxlen):
    w = band_half_width(maxlen)
    return 6 if 2 * w <= 756 else (8 if 2 * w <= 1008 else 11)


def band_cell_bytes(scores, sw, knob4=False):
    """2 only for local alignments whose delta code fits; knob4: SXG_POA_BAND_CELL_BYTES=4"""
    return 4 if knob4 or not sw else cell_bytes(scores)


def block_sweep(scores, mode, maxlen, banded, knob4=False):
    """(rm, W, NW, cb, tmax, ds) of a block's first launch; a banded block runs row mode 3 when its alignments are local or its
    band adaptive, and the STRICT range rule keeps it packed (a banded block has no clamp and no re-run of its own)"""
    sw = mode == 0
    rm = row_mode(scores, sw, maxlen, maxlen, clamp_ok=banded == 0)
    if banded and (sw or banded == 2) and rm == 2 and maxlen <= MAX_SEQ_LEN:
        return 3, band_strip_width(maxlen), 1, band_cell_bytes(scores, sw, knob4), 64, 0
    cb = cell_bytes(scores) if rm == 2 else 4
    W, NW = variant_for_len(maxlen, rm, sw)
    return rm, W, NW, cb, class_tmax(NW, rm, cb), int(rm == 2 and cb == 2 and tuple(scores) == SCORES["ds"])


def band_no_rerun(scores, mode, seq_lens, rows_before):
    """The banded kernel re-checks a global alignment's all-gap floor with the true row count in front of every sequence
    (poa_kernels.hip.h: ST_RANGE_OVERFLOW at 15 800); True when no sequence is refused"""
    if mode == 0:
        return True
    return all(-(gap_cost(scores, n) + gap_cost(scores, L)) < 15800 for L, n in zip(seq_lens, rows_before))


def band_global_top(scores, W):
    """the longest sequence of a global banded case at strip width W: the last length on W if the strict rule admits it with
    BAND_ROWS_MARGIN rows per letter, else the longest length it admits -- None if that is not on W"""
    ok = lambda L: abs(scores[0]) * L < 15800 and band_no_rerun(scores, 1, [L, L], [L, int(L * BAND_ROWS_MARGIN) + 1])
    full = BAND_LENGTHS[W][1]
    if ok(full) and W != 11:
        return full
    top = max(L for L in range(1, BAND_LENGTHS[11][1] + 1) if ok(L))
    return top if band_strip_width(top) == W and band_strip_width(top - 2) == W else None


def band_splices(W, top):
    """(column of the deletion, of the insertion): two strip boundaries a third and two thirds along the sequence"""
    strips = (top + 1) // W
    return W * (strips // 3), W * (2 * strips // 3)


def case_class(case, knob4=False, force=None):
    """(kind, rm, cb, tmax, W, sw, ds) of the class a case runs on -- the line tests/csrc/class_list.cpp prints for it"""
    W, NW = force or (case["W"], case["NW"])
    sw = 1 - case["mode"]
    scores = tuple(case["params"])
    if case["kind"] == "band":
        rm, bw, _, cb, tmax, ds = block_sweep(scores, case["mode"], max(case["seq_lens"]) if "seq_lens" in case else case["top"], case["banded"], knob4)
        assert (rm, bw) == (3, W), case
        return (0, 3, cb, tmax, W, sw, ds)
    if case["kind"] == "align":
        return (1, case["rm"], 4, class_tmax(NW, case["rm"], 4), W, sw, 0)
    cb = cell_bytes(scores, knob4) if case["rm"] == 2 else 4
    return (0, case["rm"], cb, class_tmax(NW, case["rm"], cb), W, sw, int(case["rm"] == 2 and cb == 2 and scores == SCORES["ds"]))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs

def splice_columns(W, NW, rm):
    """(column of the deletion, column of the insertion): the first and the last wave boundary, on one wave two strip boundaries"""
    if NW > 1:
        wave = capacity(W, NW, rm) // NW
        return wave, wave * (NW - 1)
    strips = capacity(W, 1, rm) // W
    return W * (strips // 3), W * (2 * strips // 3)


def make_inputs(block_id, length, del_at, ins_at):
    from smoothxg_amd import synth
    a, b, c = synth.make_block(block_id, 3, length, sv_frac=0)
    h = SPLICE // 2
    b = np.concatenate([b[:del_at - h], b[del_at + h:]])
    payload = np.random.Generator(np.random.PCG64(synth.SEED0 + 7 * int(block_id) + 1)).integers(0, 4, SPLICE, dtype=np.uint8)
    c = np.concatenate([c[:ins_at - h], payload, c[ins_at - h:]])
    return [a, b, c]


def search_inputs(seed, W, NW, rm, lo=3, hi=1, top=None, splices=None):
    """(block_id, length, del_at, ins_at, seqs) whose longest sequence has capacity - lo .. capacity - hi letters (top: that many
    letters at most in place of capacity - 1; splices: their columns in place of splice_columns')"""
    cap = capacity(W, NW, rm) if top is None else top + 1
    del_at, ins_at = splices or splice_columns(W, NW, rm)
    for k in range(400):
        block_id = seed + k
        length = cap - 2 - SPLICE
        for _ in range(6):
            seqs = make_inputs(block_id, length, del_at, ins_at)
            top = max(len(s) for s in seqs)
            if cap - lo <= top <= cap - hi:
                return block_id, length, del_at, ins_at, seqs
            length += cap - 2 - top
    raise RuntimeError("no input found for W=%d NW=%d rm=%d" % (W, NW, rm))


def snp_graph(backbone, marks):
    """A chain of `backbone` with a one-node SNP bubble every ~50 nodes and at every position of `marks`, as the CSR of
    oracle_py.Graph.rows(): codes, off, pred (1-based row index), sink.  Rows are in topological order: ..., c[p-1], c[p],
    alt[p], c[p+1], ... with alt[p] = the next letter, sharing c[p]'s predecessor and successor."""
    n = len(backbone)
    bub = np.zeros(n, bool)
    bub[25:n - 1:50] = True
    for p in marks:
        if 0 < p < n - 1:
            bub[p] = True
    bub[1:] &= ~bub[:-1]                                   # (no two bubbles in a row: every alt has one plain successor)
    nb = np.concatenate([[0], np.cumsum(bub)])             # bubbles before chain position p
    row = np.arange(n) + nb[:n]                            # row of chain node p
    N = n + int(bub.sum())
    codes = np.empty(N, np.uint8)
    codes[row] = backbone
    codes[row[bub] + 1] = (backbone[bub] + 1) & 3
    npred = np.ones(N, np.int64)
    npred[0] = 0
    after = np.flatnonzero(bub) + 1                        # chain positions behind a bubble: two predecessors
    npred[row[after]] = 2
    off = np.concatenate([[0], np.cumsum(npred)]).astype(np.int32)
    pred = np.empty(int(off[-1]), np.int32)
    chain = np.arange(1, n)
    pred[off[row[chain]]] = row[chain - 1] + 1             # c[p] <- c[p-1]
    pred[off[row[after]] + 1] = row[after - 1] + 2         # c[p+1] <- alt[p]
    alt = row[bub] + 1
    pred[off[alt]] = row[np.flatnonzero(bub) - 1] + 1      # alt[p] <- c[p-1]
    sink = np.zeros(N, np.uint8)
    sink[N - 1] = 1
    return codes, off, pred, sink


def align_problem(case):
    """(codes, off, pred, sink, query) of an align case: the graph of the block's first sequence, the third as the query"""
    seqs = make_inputs(case["block_id"], case["length"], case["del_at"], case["ins_at"])
    W, NW, rm = case["W"], case["NW"], case["rm"]
    wave = capacity(W, NW, rm) // NW
    marks = [wave * k + d for k in range(1, NW) for d in (-1, 0, 2)] if NW > 1 else [case["del_at"], case["ins_at"]]
    return snp_graph(seqs[0], marks) + (seqs[2],)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases

def packed_geometries(sw):
    g = [(W, NW) for NW in (1, 2, 3, 4) for W in range(4, 13)] + [(W, 8) for W in range(8, 13)] + [(8, 16)]
    return g + ([(10, 16), (12, 16), (13, 16)] if sw else [])


def natural_geometries(rm, sw, max_len):
    """every (W, NW) variant_for_len returns by itself for a sequence of up to max_len letters, in order of capacity"""
    out = []
    for L in range(1, max_len + 1):
        v = variant_for_len(L, rm, sw)
        if v and v not in out:
            out.append(v)
    return out


def case_id(c):
    return "%s/%s/%s/rm%d/W%dx%d" % (c["kind"], c["family"], "global" if c["mode"] else "local", c["rm"], c["W"], c["NW"]) + ("/b%d" % c["banded"] if c["kind"] == "band" else "")


def list_cases():
    """Every case without inputs and expectations: kind, family, params, mode, rm, W, NW, force, seed."""
    cases = []

    def add(kind, family, params, mode, rm, W, NW, seed, force=False, **kw):
        cases.append(dict(kind=kind, family=family, params=list(params), mode=mode, rm=rm, W=W, NW=NW, force=force, seed=seed, **kw))

    for fi, fam in enumerate(BLOCK_FAMILIES):
        for mode in (0, 1):
            for W, NW in packed_geometries(mode == 0):
                top = capacity(W, NW, 2) - 1
                if mode == 1 and not top + 1 < 14500:          # the host would not keep a global block packed
                    continue
                assert row_mode(SCORES[fam], mode == 0, top, top, clamp_ok=True) == 2
                add("block", fam, SCORES[fam], mode, 2, W, NW, 1000000 + 100000 * fi + 1000 * W + 10 * NW,
                    force=variant_for_len(top, 2, mode == 0) != (W, NW))
    # 32-bit sweeps (SXG_POA_NO_PACKED=1): int16 row words with the default scores, int32 row words where 3 * L >= 30 000
    for mode in (0, 1):
        for W, NW in natural_geometries(0, mode == 0, 12287):
            top = capacity(W, NW, 0) - 1
            assert row_mode(SCORES["ds"], mode == 0, top, top, no_packed=True) == 0
            add("block", "ds", SCORES["ds"], mode, 0, W, NW, 2000000 + 1000 * W + 10 * NW)
    for W, NW in natural_geometries(1, True, 12287):
        top = capacity(W, NW, 1) - 1
        if row_mode(SCORES["convex_heavy"], True, top - 2, top - 2, no_packed=True) == 1:
            add("block", "convex_heavy", SCORES["convex_heavy"], 0, 1, W, NW, 2500000 + 1000 * W + 10 * NW)
    # align-only: the strict range rule, no clamp -- global alignments leave the packed sweep (and int16 row words) earlier
    for fi, fam in enumerate(ALIGN_FAMILIES):
        for mode in (0, 1):
            for no_packed in (False, True):
                for W, NW in natural_geometries(0 if no_packed else 2, mode == 0, 26623 if not no_packed else 12287):
                    top = capacity(W, NW, 0 if no_packed else 2) - 1
                    # rows of the SNP graph: ~2 % more than letters; the mode must hold for the whole target range
                    rms = {row_mode(SCORES[fam], mode == 0, L, int(L * 1.03), no_packed=no_packed) for L in (top - 42, top)}
                    rm = rms.pop()
                    if rms or (rm == 2) == no_packed:
                        continue
                    if variant_for_len(top, rm, mode == 0) != (W, NW):
                        continue
                    add("align", fam, SCORES[fam], mode, rm, W, NW, 3000000 + 100000 * fi + 1000 * W + 10 * NW + 5 * no_packed, no_packed=no_packed)
            if mode == 1:
                # the last packed geometry of a global alignment is left before it is full: one case at the longest query the
                # strict rule admits, if that still reaches into the geometry's last wave
                packed = lambda L: row_mode(SCORES[fam], False, L, int(L * 1.03)) == 2
                top = max(L for L in range(1, 26624) if packed(L)) - 8
                W, NW = variant_for_len(top, 2, False)
                have = [c for c in cases if c["kind"] == "align" and c["family"] == fam and c["mode"] == 1 and (c["rm"], c["W"], c["NW"]) == (2, W, NW)]
                if not have and top > capacity(W, NW, 2) * (NW - 1) // NW + 64:
                    add("align", fam, SCORES[fam], mode, 2, W, NW, 3500000 + 100000 * fi, no_packed=False, top=top)
    # the adaptive tiers at the headline geometries: 3 x ~5.0 kbp on (10,4), 3 x ~5.2 kbp on (11,4)
    for ti, prm in enumerate(TIERS):
        assert cell_bytes(prm) == TIER_CELL_BYTES[ti], (prm, code_bits(prm))
        for W, length in ((10, 5000), (11, 5200)):
            add("tier", "tier%d" % ti, prm, 0, 2, W, 4, 4000000 + 1000 * W + ti, length=length)
    # int32 row words WITHOUT a knob: m = 64 leaves the packed sweep and int16 row words at 469 letters, before the smallest
    # geometry's target range begins (512 - 42), so every geometry of the 32-bit sweep is the host's own choice.  (Listed last,
    # and kept in class_matrix_wide.json: class_matrix.json is one line and keeps its bytes.)
    for kind in ("block", "align"):
        for mode in (0, 1):
            for W, NW in natural_geometries(1, mode == 0, 12287):
                top = capacity(W, NW, 1) - 1
                for L in (top - 42, top):
                    assert row_mode(SCORES["wide_match"], mode == 0, L, L, clamp_ok=kind == "block") == 1
                    assert row_mode(SCORES["wide_match"], mode == 0, L, int(L * 1.03)) == 1
                add(kind, "wide_match", SCORES["wide_match"], mode, 1, W, NW, 5000000 + 100000 * (kind == "align") + 1000 * W + 10 * NW, no_packed=False)
    # the banded sweep (listed last, kept in class_matrix_banded.json): "top" = the longest sequence aimed at, "lo" = how far below
    # it the search may end
    for W in (6, 8, 11):
        lo_len, hi_len = BAND_LENGTHS[W]
        for fi, fam in enumerate(BAND_LOCAL_FAMILIES):
            for banded in (1, 2):
                for L in (lo_len, hi_len):
                    assert block_sweep(SCORES[fam], 0, L, banded)[:3] == (3, W, 1)
                add("band", fam, SCORES[fam], 0, 3, W, 1, 6000000 + 100000 * fi + 1000 * W + banded, banded=banded, top=hi_len, lo=hi_len - lo_len)
        for fi, fam in enumerate(BAND_GLOBAL_FAMILIES[W]):
            top = band_global_top(SCORES[fam], W)
            assert top is not None and block_sweep(SCORES[fam], 1, top, 2)[:4] == (3, W, 1, 4), (fam, W, top)
            assert block_sweep(SCORES[fam], 1, top, 1)[0] == 2       # (the static band is for local mode only)
            add("band", fam, SCORES[fam], 1, 3, W, 1, 6500000 + 100000 * fi + 1000 * W, banded=2, top=top, lo=2)
    assert len({case_id(c) for c in cases}) == len(cases)
    return cases


def case_inputs(case):
    """the sequences of a case with recorded inputs"""
    return make_inputs(case["block_id"], case["length"], case["del_at"], case["ins_at"])


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digest_block(code, rank, group, tail, head, weight, paths):
    """make_fullshape.digest_block's arrays and types, folded into three digests; both sides compute them"""
    return {"nodes": sha(np.asarray(code, np.uint8), np.asarray(rank, np.int32), np.asarray(group, np.int32)),
            "edges": sha(np.asarray(tail, np.int32), np.asarray(head, np.int32), np.asarray(weight, np.uint32)),
            "paths": sha(np.concatenate([np.asarray(p, np.int32) for p in paths]))}


def digest_pairs(rows, pos):
    return sha(np.asarray(rows, np.int32), np.asarray(pos, np.int32))


def expectations(case, impl=None):
    """What the oracle computes for a case with inputs: the fixture's result fields."""
    from oracle import oracle_py as O
    p = O.mkparams(*case["params"], mode=case["mode"] | (0 if case["kind"] == "align" else 0x10), banded=case.get("banded", 0))
    if case["kind"] == "align":
        codes, off, pred, sink, q = align_problem(case)
        an, ap, sc = O.align_csr(codes, off, pred, sink, q, p)
        return {"rows": int(len(codes)), "score": int(sc), "n_pairs": int(len(an)), "digest": digest_pairs(an, ap)}
    seqs = case_inputs(case)
    if impl is None:   # (banded: the scalar oracle at every length -- the AVX2 twin is not held equal to it there)
        impl = O.IMPL_AVX2 if max(case["seq_lens"]) > 2100 and case["kind"] != "band" else O.IMPL_SCALAR
    g, sc, cells = O.block_run(seqs, None, p, impl=impl)
    code, rank, grp = g.nodes()
    t, h, w = g.edges()
    extra = {}
    if case["kind"] == "band":   # graph rows in front of every sequence: what the kernel's range re-check sees
        extra["rows_before"] = [0] + [int(O.block_run(seqs[:k], None, p, impl=impl)[0].n_nodes) for k in range(1, len(seqs))]
    return {**extra, "scores": [int(x) for x in sc], "cells": int(cells.sum()), "n_nodes": int(g.n_nodes), "n_edges": int(g.n_edges),
            "digests": digest_block(code, rank, grp, t, h, w, [g.seq_path(s) for s in range(g.n_seqs)])}


def run_case(case):
    t0 = time.time()
    case = dict(case)
    if case["kind"] == "tier":
        W, NW = case["W"], 4
        del_at, ins_at = splice_columns(W, NW, 2)
        for k in range(400):
            seqs = make_inputs(case["seed"] + k, case["length"], del_at, ins_at)
            if variant_for_len(max(len(s) for s in seqs), 2, True) == (W, NW):
                break
        block_id, length = case["seed"] + k, case["length"]
    elif case["kind"] == "band":
        block_id, length, del_at, ins_at, seqs = search_inputs(case["seed"], case["W"], 1, 3, lo=case["lo"] + 1, top=case["top"],
                                                               splices=band_splices(case["W"], case["top"]))
    else:
        lo = 42 if case["kind"] == "align" else 3            # (an align case's query is the third sequence, the longest or nearly)
        block_id, length, del_at, ins_at, seqs = search_inputs(case["seed"], case["W"], case["NW"], case["rm"], lo=lo, top=case.get("top"))
    case.update(block_id=block_id, length=length, del_at=del_at, ins_at=ins_at, seq_lens=[int(len(s)) for s in seqs])
    del case["seed"]
    if case["kind"] == "align":
        assert variant_for_len(len(seqs[2]), case["rm"], case["mode"] == 0) == (case["W"], case["NW"]), case
    case.update(expectations(case))
    if case["kind"] == "align":
        assert row_mode(tuple(case["params"]), case["mode"] == 0, len(seqs[2]), case["rows"], no_packed=case["no_packed"]) == case["rm"], case
    if case["kind"] == "band":
        assert band_no_rerun(tuple(case["params"]), case["mode"], case["seq_lens"], case["rows_before"]), case
    print("done %-44s %6.1f s" % (case_id(case), time.time() - t0), flush=True)
    return case


PROVENANCE = ("self-oracle (oracle/poa_oracle.c; AVX2 twin beyond 2 100 letters), generated by tests/golden/make_class_matrix.py; "
              "NOT reference-derived")
PROVENANCE_BANDED = ("self-oracle (oracle/poa_oracle.c, the scalar oracle's banded modes), generated by tests/golden/make_class_matrix.py; "
                     "NOT reference-derived")


def load_cases():
    """every case of the three fixture files, in list_cases' order: class_matrix.json, class_matrix_wide.json, class_matrix_banded.json"""
    cases = []
    for path in (FIXTURE, FIXTURE_WIDE, FIXTURE_BANDED):
        with open(path) as f:
            cases += json.load(f)["cases"]
    return cases


def main():
    """Cases the fixtures already hold are kept as they stand (the files are re-written from their parsed values, which
    round-trip byte for byte); only cases they lack are computed.  Delete a fixture to regenerate its cases."""
    from oracle import oracle_py as O
    O.build()
    have = {}
    for path in (FIXTURE, FIXTURE_WIDE, FIXTURE_BANDED):   # (a fixture that is not there: its cases are computed)
        if os.path.exists(path):
            with open(path) as f:
                have.update({case_id(c): c for c in json.load(f)["cases"]})
    listed = list_cases()
    cases = [c for c in listed if case_id(c) not in have]
    # the long ones first, so that the pool does not end on one of them
    order = sorted(range(len(cases)), key=lambda i: -cases[i].get("top", capacity(cases[i]["W"], cases[i]["NW"], cases[i]["rm"])))
    with mp.Pool(min(16, max(1, os.cpu_count() or 1))) as pool:
        done = pool.map(run_case, [cases[i] for i in order], chunksize=1)
    have.update({case_id(c): c for c in done})
    res = [have[case_id(c)] for c in listed]
    dump = lambda c: json.dumps(c, indent=None, separators=(",", ":"))
    with open(FIXTURE, "w") as f:       # (one line, as it was first written)
        f.write(dump({"provenance": PROVENANCE, "cases": [c for c in res if c["family"] not in WIDE_FAMILIES and c["kind"] != "band"]}) + "\n")
    with open(FIXTURE_WIDE, "w") as f:  # (one case per line: a later family shows in a diff as the lines it adds)
        f.write('{"provenance":%s,"cases":[\n%s\n]}\n' % (json.dumps(PROVENANCE), ",\n".join(dump(c) for c in res if c["family"] in WIDE_FAMILIES)))
    with open(FIXTURE_BANDED, "w") as f:
        f.write('{"provenance":%s,"cases":[\n%s\n]}\n' % (json.dumps(PROVENANCE_BANDED), ",\n".join(dump(c) for c in res if c["kind"] == "band")))
    print("wrote", len(res), "cases,", os.path.getsize(FIXTURE), "+", os.path.getsize(FIXTURE_WIDE), "+", os.path.getsize(FIXTURE_BANDED), "bytes")


if __name__ == "__main__":
    main()

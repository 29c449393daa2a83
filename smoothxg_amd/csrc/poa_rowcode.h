// poa_rowcode.h -- the 16-bit cell codes of the packed sweep's 2-byte classes (CB = 2).  Since round 11 the full-matrix sweep
// has ONE code: the stored-row code (P16RowCode) is what the row ring, its on-chip copies AND the traceback plane hold, so a
// row that is both stored and inside its band is encoded once.  The delta code (P16Delta / p16_plane_code, round 5) remains
// the plane format of the banded sweep (poa_band16.hip.h) and the value the unbiased (global) row code is derived from; both
// codes share the field widths of P16Delta.  p16_code_step / p16_strip_decode are what every reader of a plane strip -- the
// traceback, the sweep's read-back of stored rows -- decodes with.  Host-compilable (tests/test_rowcode.py and
// tests/test_planecode.py round-trip every representable cell of a score set on the CPU); the device forms are the same functions.
#pragma once
#include "poa_types.h"

namespace sxg {

// ---- 2-byte plane cells (CB = 2, round 5) --------------------------------------------------------------------------
// The band stores of the traceback plane were the largest single cost of the packed sweep (cost map of round 4: 24 % of the
// headline launch; 45 % of the sweep of 8000 blocks of 16 x 1 kbp, where the launch sits at the HBM write roof).  A plane cell
// held H (16 bits) and the two distances H - oF, H - oO (8 bits each).  H need not be stored in full: along a row it moves in
// small steps --
//     g <= H[i][j] - H[i][j-1] <= m - g        (g = the cheapest gap opening, normalised scores; proof in DESIGN.md section 3.1:
//     the lower bound is the in-row gap E >= H[j-1] + g, the upper one follows by induction over the ranks from
//     H[i][j-1] >= H[p][j-1] + g for the predecessor p a diagonal step into (i, j) came from)
// -- and the distances lie in [-e, -g] and [-c, -q].  A cell is therefore the 16-bit code
//     (H[j] - H[j-1] - g)  |  (H - oF + e) << bH  |  (H - oO + c) << (bH + bF),      bH + bF + bO <= 16,
// and a strip of a row is W + 1 halfwords: the H of the column LEFT of the strip (the value the sweep hands from lane to
// lane anyway; strip 0: H of column 0, whose own step is written as 0), then the W codes.  12 bits for the default scores
// 1,4,6,2,26,1; 16 for pggb's asm10 set; a score set that needs more (asm5: 1,19,39,3,81,1 -- 20 bits) takes the 4-byte
// cells (CB = 4: the round-4 format, every kernel class exists in both).  The traceback rebuilds H by summing the steps of
// a strip from its left end -- at most W additions for a cell it visits.
struct P16Delta {
    int bH, bF, bO;      // field widths
    int g, eabs, cabs;   // what the fields are offset by: dH - g, dF - |e|, dO - |c| are >= 0
};
SXG_HD int p16_bits_for(int n_values) { int b = 0; while ((1 << b) < n_values) ++b; return b; }
SXG_HD P16Delta p16_delta_of(const Scoring& S) {
    P16Delta D;
    D.g = S.g; D.eabs = -S.e; D.cabs = -S.c;
    D.bH = p16_bits_for(S.m - 2 * S.g + 1);
    D.bF = p16_bits_for(S.e - S.g + 1);
    D.bO = S.convex ? p16_bits_for(S.c - S.q + 1) : 0;
    return D;
}
SXG_HD bool p16_delta_fits(const Scoring& S) { const P16Delta D = p16_delta_of(S); return D.bH + D.bF + D.bO <= 16; }

// Two 16-bit fields in one 32-bit word, each modulo 2^16 (v_pk_add_u16 / v_pk_sub_u16 / v_pk_mad_u16 on the device).
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short p16w_u16x2 __attribute__((ext_vector_type(2)));
SXG_HD int p16w_add(int a, int b) { return __builtin_bit_cast(int, (p16w_u16x2)(__builtin_bit_cast(p16w_u16x2, a) + __builtin_bit_cast(p16w_u16x2, b))); }
SXG_HD int p16w_sub(int a, int b) { return __builtin_bit_cast(int, (p16w_u16x2)(__builtin_bit_cast(p16w_u16x2, a) - __builtin_bit_cast(p16w_u16x2, b))); }
SXG_HD int p16w_mad(int a, int b, int c) {
    return __builtin_bit_cast(int, (p16w_u16x2)(__builtin_bit_cast(p16w_u16x2, a) * __builtin_bit_cast(p16w_u16x2, b) + __builtin_bit_cast(p16w_u16x2, c)));
}
#else
SXG_HD int p16w_join(unsigned lo, unsigned hi) { return (int)((lo & 0xffffu) | (hi << 16)); }
SXG_HD int p16w_add(int a, int b) { return p16w_join((unsigned)a + (unsigned)b, ((unsigned)a >> 16) + ((unsigned)b >> 16)); }
SXG_HD int p16w_sub(int a, int b) { return p16w_join((unsigned)a - (unsigned)b, ((unsigned)a >> 16) - ((unsigned)b >> 16)); }
SXG_HD int p16w_mad(int a, int b, int c) {
    return p16w_join((unsigned)a * (unsigned)(b & 0xffff) + (unsigned)c, ((unsigned)a >> 16) * ((unsigned)b >> 16) + ((unsigned)c >> 16));
}
#endif

// Plane code of a cell, both halves of a word at once: h, of, oo = the cell's H and outgoing candidates, prev = H of the column
// to its left.  The fields are NOT yet offset by g, |e|, |c| (the decode subtracts that constant): step + (h - of) << bH + ...
// modulo 2^16.  BIASED: the sweep's biased fields (P16_BIAS), where h >= of, oo field by field makes the distances plain
// 32-bit subtractions.
template <bool CVX, bool BIASED>
SXG_HD int p16_plane_code(const int h, const int prev, const int of, const int oo, const P16Delta& D) {
    const int kf = (1 << D.bH) * 0x10001, ko = (1 << (D.bH + D.bF)) * 0x10001;
    const int df = BIASED ? (int)((unsigned)h - (unsigned)of) : p16w_sub(h, of);
    int cd = p16w_mad(df, kf, p16w_sub(h, prev));
    if (CVX) cd = p16w_mad(BIASED ? (int)((unsigned)h - (unsigned)oo) : p16w_sub(h, oo), ko, cd);
    return cd;
}

// ---- stored rows of the 2-byte classes -----------------------------------------------------------------------------
// A stored row (one that a successor other than the next rank reads: the row ring in HBM, or one of the workgroup's on-chip
// copies) holds the same facts as a plane cell in 2 bytes: per lane, dword k = the codes of column k of the lane's low and high
// strip as the two halves (the halves the sweep computes on: no permute), then one dword with the packed H of the column left
// of the two strips (lane 0 of strip 0: H of column 0 itself, its step 0).  Half the bytes of the round-2..6 row word (packed H
// + two 8-bit distances), so a four-wave workgroup's share of the CU's LDS holds two row copies instead of one.
// Fields, low bits first, each >= 0 and inside its P16Delta width:
//     s = step - g   |   f = MF - (H - oF - |e|)   |   o = MO - (H - oO - |c|)          (MF, MO = all ones of the field)
// so that decoding is one AND and one ADD3 per field: H = Hleft + s - |g|, oF = H + f - (|e| + MF), oO = H + o - (|c| + MO).
// With the sweep's biased fields these are plain 32-bit operations on both halves at once (no half ever leaves [0, 65535]).
struct P16RowCode {
    int mh, mf, mo;     // field masks after the shift, both halves
    int shf, sho;       // shifts of the F and O fields
    int kh, kf, ko;     // decode offsets |g|, |e| + MF, |c| + MO, both halves
    int kc;             // encode offset |g| + (|e| + MF) << shf + (|c| + MO) << sho, both halves
};
// (cvx: the code has the O field -- of width D.bO, which is 0 for a convex set with q = c)
SXG_HD P16RowCode p16_row_code_of(const P16Delta& D, const bool cvx) {
    P16RowCode R;
    const int MF = (1 << D.bF) - 1, MO = (1 << D.bO) - 1;
    R.mh = ((1 << D.bH) - 1) * 0x10001; R.mf = MF * 0x10001; R.mo = MO * 0x10001;
    R.shf = D.bH; R.sho = D.bH + D.bF;
    R.kh = -D.g * 0x10001; R.kf = (D.eabs + MF) * 0x10001; R.ko = (D.cabs + MO) * 0x10001;
    const int kc = (-D.g + ((D.eabs + MF) << R.shf) + (cvx ? (D.cabs + MO) << R.sho : 0)) & 0xffff;
    R.kc = kc * 0x10001;
    return R;
}
// BIASED: every field straight from its definition in plain 32-bit arithmetic (h + |g| - prev, of + |e| + MF - h, ... are >= 0
// and inside their fields on both halves: no borrow, no carry crosses bit 16) -- 8 instructions of the 2-cycle kind per column.
// Otherwise (global alignments: unbiased, negative fields) from the cell's plane code, which the band stores compute anyway:
// code = 2 (h - prev) + kc - plane code, modulo 2^16 on each half.
template <bool CVX, bool BIASED>
SXG_HD int p16_row_encode(const int h, const int prev, const int of, const int oo, const P16Delta& D, const P16RowCode& R) {
    if (BIASED) {
        unsigned cd = (unsigned)h + (unsigned)R.kh - (unsigned)prev;
        cd += ((unsigned)of + (unsigned)R.kf - (unsigned)h) << R.shf;
        if (CVX) cd += ((unsigned)oo + (unsigned)R.ko - (unsigned)h) << R.sho;
        return (int)cd;
    }
    return p16w_mad(p16w_sub(h, prev), 0x20002, p16w_sub(R.kc, p16_plane_code<CVX, BIASED>(h, prev, of, oo, D)));
}
// One column: h enters as the H of the column to the left and leaves as this column's; of, oo receive its outgoing candidates.
template <bool CVX, bool BIASED>
SXG_HD void p16_row_decode(const unsigned w, int& h, int& of, int& oo, const P16RowCode& R) {
    const int s = (int)w & R.mh, f = (int)(w >> R.shf) & R.mf;
    h = BIASED ? (int)((unsigned)h + (unsigned)s - (unsigned)R.kh) : p16w_sub(p16w_add(h, s), R.kh);
    of = BIASED ? (int)((unsigned)h + (unsigned)f - (unsigned)R.kf) : p16w_sub(p16w_add(h, f), R.kf);
    if (CVX) {
        const int o = (int)(w >> R.sho) & R.mo;
        oo = BIASED ? (int)((unsigned)h + (unsigned)o - (unsigned)R.ko) : p16w_sub(p16w_add(h, o), R.ko);
    }
}

// ---- a strip of a plane row, one cell at a time (the traceback; round 11) ------------------------------------------
// A strip is W + 1 halfwords: the H left of the strip (strip 0, and every strip of the banded sweep: its own first H, whose
// step is then 0), then the W codes -- row codes in the full-matrix sweep's plane, delta codes (DELTA) in the banded sweep's.
// These are the scalar forms, one 16-bit code at a time in ordinary int arithmetic; H comes back sign-extended, biased as stored.
// halfword hw of a strip whose dwords are d[]
SXG_HD unsigned p16_strip_half(const unsigned* const d, const int hw) { return (hw & 1) ? d[hw >> 1] >> 16 : d[hw >> 1] & 0xffffu; }
// One column: h enters as the H of the column to the left and leaves as this column's; df, dq receive the distances H - oF,
// H - oO to its outgoing candidates (dq = 0 without the second gap piece).
template <bool CVX, bool DELTA = false>
SXG_HD void p16_code_step(unsigned code, int& h, int& df, int& dq, const P16Delta& D) {
    const unsigned mH = (1u << D.bH) - 1u, mF = (1u << D.bF) - 1u, mO = (1u << D.bO) - 1u;
    if (DELTA) {
        // the sweep adds the raw step and distances into the code; taking their least values off first (mod 2^16) leaves
        // three non-negative fields side by side
        code = (code - (unsigned)(D.g + (D.eabs << D.bH) + ((CVX ? D.cabs : 0) << (D.bH + D.bF)))) & 0xffffu;
        h += (int)(code & mH) + D.g;
        df = (int)((code >> D.bH) & mF) + D.eabs;
        dq = (int)(code >> (D.bH + D.bF)) + (CVX ? D.cabs : 0);
    } else {
        code &= 0xffffu;
        h += (int)(code & mH) + D.g;
        df = D.eabs + (int)(mF - ((code >> D.bH) & mF));
        dq = CVX ? D.cabs + (int)(mO - ((code >> (D.bH + D.bF)) & mO)) : 0;
    }
}
// Column k of a strip (0 <= k < W): sums the steps from the strip's left end; `half(hw)` returns halfword hw of the strip.
// W > 0: unrolled over a strip of W columns (strips held in registers); W = 0: a plain loop up to k.
template <bool CVX, bool DELTA = false, int W = 0, class HALF>
SXG_HD void p16_strip_decode(HALF half, const int k, int& h, int& of, int& oo, const P16Delta& D) {
    int df = 0, dq = 0;
    h = (int)(short)(half(0) & 0xffffu);
    if (W > 0) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int t = 0; t < W; ++t) if (t <= k) p16_code_step<CVX, DELTA>(half(1 + t), h, df, dq, D);
    } else {
        for (int t = 0; t <= k; ++t) p16_code_step<CVX, DELTA>(half(1 + t), h, df, dq, D);
    }
    of = h - df; oo = h - dq;
}

}  // namespace sxg

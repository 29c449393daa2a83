// poa_fields.h -- the 16-bit fields of the packed sweep's LOCAL classes: the bias, what the host admits, and the range the
// fields therefore stay in.  Plain C++17, constexpr, no HIP: included by the sweep (poa_dp16.hip.h), by the host's admission
// test (sxg_poa.hip: p16_safe) and by the host-only checks of the range (tests/csrc/field_range_check.cpp) and of the strip
// form of the long gap piece (tests/csrc/strip_gap_check.cpp).
//
// Nothing here is checked at run time: the static_asserts below ARE the argument.
#pragma once

namespace sxg {

// smoothxg's default scores in the engine's (spoa's) sign convention: the score set the DS kernel classes are compiled for
constexpr int P16_DEF_M = 1, P16_DEF_N = -4, P16_DEF_G = -6, P16_DEF_E = -2, P16_DEF_Q = -26, P16_DEF_C = -1;

// LOCAL alignments run the packed sweep on BIASED fields: a register half holds score + P16_BIAS, always inside
// [P16_FLOOR, 32767].  Every reachable value of a local alignment is >= min(g, q) >= -120 (H >= 0, every gap state is
// some H plus at most one opening) and the few "minus infinity" inputs (the column left of column 0, a carry that enters
// strip 0) are replaced by P16_FLOOR - P16_BIAS = -512, which never wins a maximum.  Fields that never leave
// [0, 65535] make a PLAIN 32-bit add/subtract of a constant -- or of any register whose fields do not underflow --
// correct on both halves at once (no borrow ever crosses bit 16), and on gfx950 v_add_u32 / v_sub_u32 issue every 2
// cycles per wave where every VOP3P instruction (v_pk_add_i16, v_pk_max_i16, ...) takes 4
// (profiles/r03/op_rate.txt): 37 % of the row loop's VALU instructions were packed adds and subtracts.
constexpr int P16_BIAS = 1024, P16_FLOOR = 512;

// What the host admits to the packed sweep as a local alignment: m * L < P16_LOCAL_LIMIT (L = the longest sequence), so that
// every score is at most P16_LOCAL_LIMIT - 1.
constexpr int P16_LOCAL_LIMIT = 30000;
// The widest strip a packed class has (poa_classes.h: the 16-wave local classes; field_range_check.cpp holds the class list
// against it).
constexpr int P16_W_MAX = 13;

// ---- the biased fields as binary16 patterns ------------------------------------------------------------------------
// A field in [0x0000, 0x7BFF] read as an IEEE binary16 number is +0, a positive denormal or a positive finite normal, and on
// those patterns the binary16 order IS the unsigned integer order (sign 0; exponent, then mantissa, from the top bit down).
// maximum(a, b) returns one of its operands bit for bit (denormals preserved: the kernels run with FP16 denormals on), so
// on such fields a three-input binary16 maximum equals pk_max(pk_max(a, b), c), the signed 16-bit maximum, exactly.
// 0x7C00 is +infinity and everything above it up to 0x7FFF a NaN: the first pattern the argument does not cover.
constexpr int P16_F16_TOP = 0x7BFF;
constexpr int p16_abs(int v) { return v < 0 ? -v : v; }
// The greatest field a local row of strip width W can hold under gap extensions e, c: a score at the admission limit, biased,
// plus the offset the strip-local carries of pass 1 ride on ((W - 1) extensions above the H they start from).
constexpr int p16_top_field(int e, int c, int W) {
    return P16_BIAS + P16_LOCAL_LIMIT - 1 + (W - 1) * (p16_abs(e) > p16_abs(c) ? p16_abs(e) : p16_abs(c));
}
// The least: "minus infinity" plus one mismatch or one opening (the diagonal / a gap state out of a floor cell) -- or, in the
// classes that read the long piece inside a strip straight off its carry (p16_strip_q_dominated below), a carry at the floor
// run to the strip's last column: Qin - (W - 1) |c| >= P16_FLOOR - (W - 1) |c|.
constexpr int p16_bottom_field(int n, int g, int q, int c = 0, int W = 1) {
    const int open_ = p16_abs(n) > p16_abs(g) ? (p16_abs(n) > p16_abs(q) ? p16_abs(n) : p16_abs(q)) : (p16_abs(g) > p16_abs(q) ? p16_abs(g) : p16_abs(q));
    const int run_ = (W - 1) * p16_abs(c);
    return P16_FLOOR - (open_ > run_ ? open_ : run_);
}
constexpr bool p16_fields_are_f16_ordered(int n, int g, int e, int q, int c, int W) {
    return p16_bottom_field(n, g, q, c, W) >= 0 && p16_top_field(e, c, W) <= P16_F16_TOP;
}
// The default scores, every strip width up to the widest: the classes compiled for them (DS) may take three-input maxima.
static_assert(p16_top_field(P16_DEF_E, P16_DEF_C, P16_W_MAX) == 31047, "1024 + 29 999 + 12 * 2");
static_assert(p16_fields_are_f16_ordered(P16_DEF_N, P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, P16_W_MAX), "default scores: fields within 0 .. 0x7BFF");
// Not so for every score set the generic local classes admit (|g|, |q| <= 120, |e| <= |g|): (W - 1) * |e| may exceed the
// 0x7BFF - 31 023 = 720 of headroom there -- they keep the two-input integer maxima.
static_assert(!p16_fields_are_f16_ordered(-4, -120, -120, -120, -120, P16_W_MAX), "generic score sets are not covered");
static_assert(p16_bottom_field(P16_DEF_N, P16_DEF_G, P16_DEF_Q, P16_DEF_C, P16_W_MAX) == P16_FLOOR - 26, "the opening (26) is still the deepest: a floor carry run over a strip is 512 - 12");

// ---- pass 1's strip carries as maximum trees ------------------------------------------------------------------------
// The carries a strip hands to the scans are plain maxima over its columns: a = max_k (Hc[k] - (W-1-k) |e|), b the same with
// |c| (Hc: H before the in-row gaps).  The classes with ordered fields build them as trees of three-input maxima whose leaves
// are Hc[k] run down to the strip's last column, (W - 1 - k) extensions: the least operand of a node is a pass-1 H at the
// bottom bound, W - 1 extensions of the dearer piece down.  (Nothing rides ABOVE H in this form; p16_top_field keeps its
// (W - 1) extensions for the classes that still carry a and b column by column.)
// The leaf is ONE 32-bit subtraction of (W-1-k) |e| * 0x10001 on both halves: with every half at least this bound before and
// at least 0 after, the low half never borrows from bit 16 -- the same bound is the range argument and the borrow argument.
constexpr int p16_carry_leaf_bottom(int n, int g, int e, int q, int c, int W) {
    return p16_bottom_field(n, g, q, c, W) - (W - 1) * (p16_abs(e) > p16_abs(c) ? p16_abs(e) : p16_abs(c));
}
static_assert(p16_carry_leaf_bottom(P16_DEF_N, P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, P16_W_MAX) == 462, "512 - 26 - 12 * 2");
static_assert(p16_carry_leaf_bottom(P16_DEF_N, P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, P16_W_MAX) >= 0, "default scores: no leaf below 0, no borrow");
// Not so for every score set the generic local classes admit -- they keep the running form.
static_assert(p16_carry_leaf_bottom(-4, -120, -120, -120, -120, P16_W_MAX) < 0, "generic score sets are not covered");
static_assert(p16_carry_leaf_bottom(-4, -120, -60, -120, -1, P16_W_MAX) < 0, "... nor with a cheap long piece: 512 - 120 - 12 * 60");

// ---- the long gap piece inside a strip ------------------------------------------------------------------------------
// Two-piece gap cost: a gap opened at column j' and read at column j, d = j - j' - 1 columns between them, scores
// H[j'] + g + d e by the first piece and H[j'] + q + d c by the second.  The first is at least the second while
// g - q >= d (c - e); inside a strip of W columns d <= W - 2.  Where that holds for every such d, the second piece opened
// INSIDE a strip never decides a cell of that strip: H[j] = max(Hc[j], E[j], Qin - (j - j_s) |c|) with Qin the carry that
// entered the strip at its first column j_s, and the per-column update Q = max(h + q, Q + c) is dead inside the strip.
// What leaves a strip does not come from that update either: the strips' carries are scanned from pass 1's b (H before the
// in-row gaps), and the word for the next wave is max(Qin - W |c|, b) of the wave's last strip.
constexpr bool p16_strip_q_dominated(int g, int e, int q, int c, int W) {
    for (int d = 0; d <= W - 2; ++d)
        if (g + d * e < q + d * c) return false;
    return true;
}
static_assert(p16_strip_q_dominated(P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, P16_W_MAX), "default scores: 20 >= d for d <= 11");
static_assert(!p16_strip_q_dominated(P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, 23), "... and no further than d = 20");
// Not so for every score set the generic classes admit (g = q: the second piece wins from d = 1 on) -- they keep the update.
static_assert(!p16_strip_q_dominated(-6, -2, -6, -1, 4), "generic score sets are not covered");

}  // namespace sxg

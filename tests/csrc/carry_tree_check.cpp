// TEST HARNESS: pass 1's strip carries as trees of three-input binary16 maxima (smoothxg_amd/csrc/poa_fields.h:
// p16_carry_leaf_bottom; smoothxg_amd/csrc/poa_dp16_row.inc.h, part 1).  One strip of a local row, both halves of the packed
// registers, restated on the host in two forms from the same H-before-the-in-row-gaps (pass 1's Hc):
//   RUNNING  the sweep as it was: a = pk_max(a + |e|, Hc[k]) from the strip's last column to its first, then - (W-1) |e|, the
//            clamp at the bias, the opening; b the same with |c| and q -- 32-bit adds on both halves, signed 16-bit maxima;
//   TREE     the sweep as it is: leaves Hc[k] - (W-1-k) |e| by ONE 32-bit subtraction on both halves, the bias as one more
//            leaf, nodes of three (a last one of two) that pick by binary16 VALUE -- decoded here with integers only --, the opening.
// Checks: both halves of a and b are equal in the two forms; every operand of a node is a pattern in 0 .. 0x7BFF; no half of a
// leaf subtraction borrows (the 32-bit result is the two 16-bit results side by side); the constexpr bound holds at every
// strip width a default-score class is built for.  A control shows the borrow check firing for a generic score set.
// Prints "<checks> <failures>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../smoothxg_amd/csrc/poa_classes.h"
#include "../../smoothxg_amd/csrc/poa_fields.h"

using namespace sxg;

static long n_checks = 0, n_bad = 0;
#define CHECK(cond) do { ++n_checks; if (!(cond) && ++n_bad <= 5) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } while (0)

constexpr int W_MAX = P16_W_MAX;
static_assert(CLASS_W_MIN == 4 && P16_W_MAX == 13, "the widths this check walks");

static uint32_t pk2(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }
static int lo_of(uint32_t x) { return (int)(int16_t)(x & 0xffffu); }
static int hi_of(uint32_t x) { return (int)(int16_t)(x >> 16); }
// v_pk_max_i16: the signed maximum of each half
static uint32_t pk_max(uint32_t a, uint32_t b) { return pk2(std::max(lo_of(a), lo_of(b)), std::max(hi_of(a), hi_of(b))); }

// binary16 -> (finite?, value * 2^24): 1 sign, 5 exponent, 10 mantissa bits; exponent 0: denormal m * 2^-24; 31: infinity / NaN
static bool f16_decode(unsigned p, int64_t* scaled) {
    const unsigned ex = (p >> 10) & 31u, m = p & 1023u;
    if (ex == 31u) return false;
    const int64_t mag = ex == 0 ? (int64_t)m : (int64_t)(1024u + m) << (ex - 1);
    *scaled = (p & 0x8000u) ? -mag : mag;
    return true;
}
static long n_out_of_range = 0;
static unsigned f16_max(unsigned a, unsigned b) {   // by VALUE; an operand outside 0 .. 0x7BFF is counted
    int64_t va = 0, vb = 0;
    if (a > (unsigned)P16_F16_TOP || b > (unsigned)P16_F16_TOP) ++n_out_of_range;
    const bool fa = f16_decode(a, &va), fb = f16_decode(b, &vb);
    if (!fa || !fb) return 0xffffu;   // (never a result of ordered fields: the comparison with RUNNING fails)
    return vb > va ? b : a;
}
// v_pk_maximum3_f16 / v_pk_max_f16 on the patterns of both halves
static uint32_t pk_max3_f16(uint32_t a, uint32_t b, uint32_t c) {
    return (f16_max(f16_max(a & 0xffffu, b & 0xffffu), c & 0xffffu)) | (f16_max(f16_max(a >> 16, b >> 16), c >> 16) << 16);
}
static uint32_t pk_max_f16(uint32_t a, uint32_t b) { return f16_max(a & 0xffffu, b & 0xffffu) | (f16_max(a >> 16, b >> 16) << 16); }

struct Scores { int g, e, q, c; };
constexpr Scores DEF{P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C};

// RUNNING: the parent's pass 1 and what follows its column loop, token by token (SW: P16_INC / P16_DEC are 32-bit adds / subtracts)
static void carries_running(const Scores& s, int W, const uint32_t* Hc, uint32_t* a_out, uint32_t* b_out) {
    const uint32_t Gm = (uint32_t)(-s.g) * 0x10001u, Em = (uint32_t)(-s.e) * 0x10001u, Qm = (uint32_t)(-s.q) * 0x10001u, Cm = (uint32_t)(-s.c) * 0x10001u;
    const uint32_t NEG2 = pk2(P16_FLOOR, P16_FLOOR), B2 = pk2(P16_BIAS, P16_BIAS);
    uint32_t a = NEG2, b = NEG2;
    for (int k = W - 1; k >= 0; --k) {
        a = pk_max(a + Em, Hc[k]);
        b = pk_max(b + Cm, Hc[k]);
    }
    a = a - (uint32_t)(W - 1) * Em;
    b = b - (uint32_t)(W - 1) * Cm;
    a = pk_max(a, B2); b = pk_max(b, B2);
    *a_out = a - Gm;
    *b_out = b - Qm;
}

// one leaf: the 32-bit subtraction, checked against the two halves done on their own
static long n_borrows = 0;
static uint32_t leaf(uint32_t h, int down) {
    const uint32_t y = h - (uint32_t)down * 0x10001u;
    const int lo = (int)(h & 0xffffu) - down, hi = (int)(h >> 16) - down;
    if (lo < 0 || hi < 0 || y != (((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16))) ++n_borrows;
    return y;
}

// TREE: the kernel's part 1 behind its column loop
static void carries_tree(const Scores& s, int W, const uint32_t* Hc, uint32_t* a_out, uint32_t* b_out) {
    const uint32_t Gm = (uint32_t)(-s.g) * 0x10001u, Qm = (uint32_t)(-s.q) * 0x10001u;
    uint32_t ta[W_MAX + 1], tb[W_MAX + 1];
    for (int k = 0; k < W - 1; ++k) {
        ta[k] = leaf(Hc[k], (W - 1 - k) * -s.e);
        tb[k] = leaf(Hc[k], (W - 1 - k) * -s.c);
    }
    ta[W - 1] = tb[W - 1] = Hc[W - 1];
    ta[W] = tb[W] = pk2(P16_BIAS, P16_BIAS);
    for (int n = W + 1; n > 1; n = n / 3 + (n % 3 ? 1 : 0)) {
        for (int k = 0; k < n / 3; ++k) {
            ta[k] = pk_max3_f16(ta[3 * k], ta[3 * k + 1], ta[3 * k + 2]);
            tb[k] = pk_max3_f16(tb[3 * k], tb[3 * k + 1], tb[3 * k + 2]);
        }
        if (n % 3 == 1) { ta[n / 3] = ta[n - 1]; tb[n / 3] = tb[n - 1]; }
        if (n % 3 == 2) { ta[n / 3] = pk_max_f16(ta[n - 2], ta[n - 1]); tb[n / 3] = pk_max_f16(tb[n - 2], tb[n - 1]); }
    }
    *a_out = ta[0] - Gm;
    *b_out = tb[0] - Qm;
}

// the carries written out with plain integers, one half: what both forms must give
static int carry_plain(int W, const int* h, int ext, int open_) {
    int v = P16_BIAS;
    for (int k = 0; k < W; ++k) v = std::max(v, h[k] + (W - 1 - k) * ext);
    return v + open_;
}

static void check_strip(int W, const int* lo, const int* hi) {
    uint32_t Hc[W_MAX];
    for (int k = 0; k < W; ++k) Hc[k] = pk2(lo[k], hi[k]);
    uint32_t ar, br, at, bt;
    const long oor = n_out_of_range, bor = n_borrows;
    carries_running(DEF, W, Hc, &ar, &br);
    carries_tree(DEF, W, Hc, &at, &bt);
    CHECK((at & 0xffffu) == (ar & 0xffffu));
    CHECK((at >> 16) == (ar >> 16));
    CHECK((bt & 0xffffu) == (br & 0xffffu));
    CHECK((bt >> 16) == (br >> 16));
    CHECK(lo_of(at) == carry_plain(W, lo, DEF.e, DEF.g) && hi_of(at) == carry_plain(W, hi, DEF.e, DEF.g));
    CHECK(lo_of(bt) == carry_plain(W, lo, DEF.c, DEF.q) && hi_of(bt) == carry_plain(W, hi, DEF.c, DEF.q));
    CHECK(n_out_of_range == oor);   // every operand of a node within 0 .. 0x7BFF
    CHECK(n_borrows == bor);        // no half of a leaf subtraction borrowed
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (unsigned)(rng_state >> 32); }
static int rnd_in(int lo, int hi) { return lo + (int)(rnd() % (unsigned)(hi - lo + 1)); }

int main() {
    // the bound, at every strip width a class compiled for the default scores has (the second width W - 1 included)
    int widths = 0;
    for (const ClassRow& c : kClasses) {
        if (!(c.rms & RM2) || !(c.modes & CLS_DS) || !(c.modes & CLS_LOCAL)) continue;
        for (int w = CLASS_W_MIN; w <= CLASS_W_MAX; ++w) {
            if (!(c.widths & cw(w))) continue;
            ++widths;
            CHECK(w <= P16_W_MAX && p16_carry_leaf_bottom(P16_DEF_N, DEF.g, DEF.e, DEF.q, DEF.c, w) >= 0);
            if (c.widths2 & cw(w)) CHECK(p16_carry_leaf_bottom(P16_DEF_N, DEF.g, DEF.e, DEF.q, DEF.c, w - 1) >= 0);
        }
    }
    CHECK(widths > 0);
    CHECK(p16_carry_leaf_bottom(P16_DEF_N, DEF.g, DEF.e, DEF.q, DEF.c, P16_W_MAX) == 512 - 26 - 12 * 2);
    CHECK(p16_carry_leaf_bottom(-4, -120, -120, -120, -120, P16_W_MAX) < 0);

    for (int W = CLASS_W_MIN; W <= P16_W_MAX; ++W) {
        // what pass 1 can hold: from the bottom bound to a score at the admission limit (nothing rides above H before the carries)
        const int BOT = p16_bottom_field(P16_DEF_N, DEF.g, DEF.q, DEF.c, W), TOP = P16_BIAS + P16_LOCAL_LIMIT - 1;
        int lo[W_MAX], hi[W_MAX];
        // all fields at the bottom bound, all at the top bound, one half each way
        for (int v = 0; v < 4; ++v) {
            for (int k = 0; k < W; ++k) { lo[k] = (v & 1) ? TOP : BOT; hi[k] = (v & 2) ? TOP : BOT; }
            check_strip(W, lo, hi);
        }
        // the winning column at every k, on a floor of every kind: the bottom bound, just under the bias, at it, mid-range, near the top
        const int floors[] = {BOT, P16_BIAS - 1, P16_BIAS, P16_BIAS + 1, 5000, TOP - 40};
        for (int f : floors)
            for (int k0 = 0; k0 < W; ++k0)
                for (int k1 = 0; k1 < W; ++k1)
                    for (int up : {1, 2, 3, 25, 40}) {
                        for (int k = 0; k < W; ++k) { lo[k] = f; hi[k] = f; }
                        lo[k0] = std::min(TOP, f + up + (W - 1 - k0) * 2);   // (just enough, or not quite, to beat the last column)
                        hi[k1] = std::min(TOP, f + up + (W - 1 - k1));
                        check_strip(W, lo, hi);
                    }
        // ties: every leaf of a equal (slope |e|), every leaf of b equal (slope |c|), flat rows, a tie with the clamp leaf
        for (int base : {BOT, P16_BIAS - 24, P16_BIAS, 2000, TOP - 24}) {
            for (int k = 0; k < W; ++k) { lo[k] = base + (W - 1 - k) * 2; hi[k] = base + (W - 1 - k); }
            check_strip(W, lo, hi);
            for (int k = 0; k < W; ++k) { lo[k] = base + (W - 1 - k); hi[k] = base + (W - 1 - k) * 2; }
            check_strip(W, lo, hi);
            for (int k = 0; k < W; ++k) { lo[k] = base; hi[k] = base + (k & 1); }
            check_strip(W, lo, hi);
        }
        for (int k0 = 0; k0 < W; ++k0) {   // column k0's leaf equals the bias exactly, one below, one above; the rest below it
            for (int d = -1; d <= 1; ++d) {
                for (int k = 0; k < W; ++k) { lo[k] = BOT; hi[k] = P16_BIAS - 30; }
                lo[k0] = P16_BIAS + d + (W - 1 - k0) * 2;
                hi[k0] = P16_BIAS + d + (W - 1 - k0);
                check_strip(W, lo, hi);
            }
        }
        // the clamp leaf winning: every field below the bias
        for (int r = 0; r < 400; ++r) {
            for (int k = 0; k < W; ++k) { lo[k] = rnd_in(BOT, P16_BIAS - 1); hi[k] = rnd_in(BOT, P16_BIAS - 1); }
            check_strip(W, lo, hi);
        }
        // random rows: the whole range, walks near the bias, walks near the top, halves of different kinds
        for (int r = 0; r < 6000; ++r) {
            const int kl = r % 3, kh = (r / 3) % 3;
            int vl = kl == 1 ? rnd_in(P16_BIAS - 20, P16_BIAS + 60) : TOP - rnd_in(0, 80), vh = kh == 1 ? rnd_in(P16_BIAS - 20, P16_BIAS + 60) : TOP - rnd_in(0, 80);
            for (int k = 0; k < W; ++k) {
                vl = std::min(TOP, std::max(BOT, vl + rnd_in(-6, 5)));
                vh = std::min(TOP, std::max(BOT, vh + rnd_in(-6, 5)));
                lo[k] = kl == 0 ? rnd_in(BOT, TOP) : vl;
                hi[k] = kh == 0 ? rnd_in(BOT, TOP) : vh;
            }
            check_strip(W, lo, hi);
        }
    }
    // a control: the borrow check must be able to fire -- a generic score set (|e| = 120), a strip at the bottom bound
    {
        const Scores gen{-120, -120, -120, -120};
        uint32_t Hc[W_MAX], at, bt;
        for (int k = 0; k < W_MAX; ++k) Hc[k] = pk2(P16_FLOOR - 120, P16_BIAS);
        const long bor = n_borrows;
        carries_tree(gen, W_MAX, Hc, &at, &bt);
        CHECK(n_borrows > bor);
        n_out_of_range = 0;   // (the control's own)
    }
    printf("%ld %ld\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}

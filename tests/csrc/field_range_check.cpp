// TEST HARNESS: the range argument behind the packed sweep's three-input binary16 maxima (smoothxg_amd/csrc/poa_fields.h,
// compiled for the host).  Checks that
//   * the fields of a local row stay within the patterns 0 .. 0x7BFF for the default scores at every packed strip width, and the
//     widest strip the class list has is the width the header names;
//   * read as IEEE binary16 -- decoded here with integers only, value * 2^24 -- the patterns 0 .. 0x7BFF are strictly increasing,
//     0x7BFF is the last finite one and 0x7C00 is not finite;
//   * hence a maximum picked by binary16 value is the maximum picked by the integers, three inputs at a time, at the edges.
// Prints "<checks> <failures>".
#include <cstdint>
#include <cstdio>
#include "../../smoothxg_amd/csrc/poa_classes.h"
#include "../../smoothxg_amd/csrc/poa_fields.h"

using namespace sxg;

// binary16 -> (finite?, value * 2^24): 1 sign, 5 exponent, 10 mantissa bits; exponent 0: denormal m * 2^-24; 31: infinity / NaN
static bool f16_decode(unsigned p, int64_t* scaled) {
    const unsigned ex = (p >> 10) & 31u, m = p & 1023u;
    if (ex == 31u) return false;
    const int64_t mag = ex == 0 ? (int64_t)m : (int64_t)(1024u + m) << (ex - 1);
    *scaled = (p & 0x8000u) ? -mag : mag;
    return true;
}
static unsigned f16_max3(unsigned a, unsigned b, unsigned c) {   // by VALUE
    int64_t va, vb, vc;
    f16_decode(a, &va); f16_decode(b, &vb); f16_decode(c, &vc);
    unsigned r = a; int64_t vr = va;
    if (vb > vr) { r = b; vr = vb; }
    if (vc > vr) { r = c; vr = vc; }
    return r;
}

int main() {
    long n = 0, bad = 0;
#define CHECK(cond) do { ++n; if (!(cond) && ++bad <= 5) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } while (0)
    // the bound, width by width
    int wmax = 0;
    for (const ClassRow& c : kClasses)
        if (c.rms & RM2)
            for (int w = CLASS_W_MIN; w <= CLASS_W_MAX; ++w) if ((c.widths & cw(w)) && w > wmax) wmax = w;
    CHECK(wmax == P16_W_MAX);
    for (int w = CLASS_W_MIN; w <= P16_W_MAX; ++w) {
        CHECK(p16_fields_are_f16_ordered(P16_DEF_N, P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, w));
        const int top = P16_BIAS + (P16_LOCAL_LIMIT - 1) + (w - 1) * 2;   // written out: m L <= 29 999, |e| = 2 > |c| = 1
        CHECK(p16_top_field(P16_DEF_E, P16_DEF_C, w) == top && top <= 0x7BFF);
    }
    CHECK(p16_bottom_field(P16_DEF_N, P16_DEF_G, P16_DEF_Q) == 512 - 26);
    CHECK(P16_F16_TOP == 0x7BFF && P16_FLOOR < P16_BIAS);
    // the order of the patterns
    int64_t prev = -1, v = 0;
    for (unsigned p = 0; p <= 0x7BFFu; ++p) {
        const bool fin = f16_decode(p, &v);
        CHECK(fin && v > prev);
        prev = v;
    }
    CHECK(v == (int64_t)65504 << 24);          // the greatest finite binary16
    CHECK(!f16_decode(0x7C00u, &v));           // +infinity: the first pattern that is not finite
    CHECK(f16_decode(P16_FLOOR, &v) && v == P16_FLOOR && f16_decode(1023u, &v) && v == 1023);   // denormals: pattern == value * 2^24
    // three inputs at the edges of the range, the floor, the bias, the denormal / normal border
    const unsigned e[] = {0, 1, (unsigned)P16_FLOOR - 26, (unsigned)P16_FLOOR, 1023, (unsigned)P16_BIAS, 1025, 0x3BFF, 0x3C00, 0x5FFF, 0x6000,
                          (unsigned)p16_top_field(P16_DEF_E, P16_DEF_C, P16_W_MAX), 0x7BFE, 0x7BFF};
    for (unsigned a : e) for (unsigned b : e) for (unsigned c : e) {
        const unsigned want = a > b ? (a > c ? a : c) : (b > c ? b : c);
        CHECK(f16_max3(a, b, c) == want);
    }
    printf("%ld %ld\n", n, bad);
    return 0;
}

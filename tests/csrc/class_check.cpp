// TEST HARNESS: the host-side choice of a kernel class (smoothxg_amd/csrc/poa_classes.h) for every sequence length.  Never shipped.
//
//   class_check          prints one line per case: kind rm sw cb full_plane spread maxlen W NW TMAX   (W = -1: no geometry)
//                        and fails (exit status 1, reasons on stderr) when a chosen geometry has no built class, a class compiled
//                        for a fixed thread count is chosen at another one, a class compiled for a plane that keeps every strip is
//                        chosen for a narrowed one, or the columns do not cover the sequence.
// The choice follows what sxg_poa.hip does with the header: variant_for_len at classification (the plane is assumed to keep
// every strip), one halving step of the spread where it applies, class_tmax once the launch knows its plane.
#include <cstdio>

#include "../../smoothxg_amd/csrc/poa_classes.h"

// a compile-time sample: the header is constexpr all the way
static_assert(class_tmax(11, 1, 2, 2, true) == 64 && class_tmax(11, 1, 2, 2, false) == 128 && class_tmax(12, 1, 2, 2, false) == 64, "class_tmax");
static_assert(class_traits(64, 11, 2, 2).rp == 2 && class_traits(64, 12, 2, 2).rp == 1 && class_traits(256, 8, 2, 2).rp == 0, "rp");
static_assert(class_built(Variant{11, 4, 256, 2, 2, true}, true, true) && !class_built(Variant{13, 16, 1024, 2, 2}, true, false), "class_built");
static_assert(!class_built(Variant{7, 1, 64, 3, 2}, true, true), "a banded width without a class");

static int bad = 0;
static void fault(const char* what, int kind, int rm, int sw, int cb, int full, int spread, int maxlen, const Variant& v) {
    if (++bad <= 20)
        fprintf(stderr, "%s: kind=%d rm=%d sw=%d cb=%d full=%d spread=%d maxlen=%d -> W=%d NW=%d TMAX=%d\n", what, kind, rm, sw, cb, full, spread, maxlen, v.W, v.NW, v.TMAX);
}

int main() {
    const int kMaxLen = 26623;   // the widest class: 16 waves x 13 columns x 128
    for (int kind = 0; kind < 2; ++kind)
    for (int rm = 0; rm < 3; ++rm) for (int sw = 0; sw < 2; ++sw) for (int cb = 2; cb <= 4; cb += 2) for (int full = 1; full >= 0; --full) for (int spread = 0; spread < 2; ++spread) {
        if (kind == CLASS_ALIGN && (cb != 4 || !full || spread)) continue;   // the align-only path: 4-byte cells, every strip kept, no spread
        for (int maxlen = 0; maxlen <= kMaxLen; ++maxlen) {
            Variant v{-1, -1, -1, rm};
            bool fits = variant_for_len(maxlen, rm, &v, sw != 0, rm == 2 ? cb : 4);
            if (fits && spread) {
                if (v.RM == 2 && v.NW <= 2 && v.W % 2 == 0 && v.W / 2 >= 4) v = Variant{v.W / 2, 2 * v.NW, class_tmax(v.W / 2, 2 * v.NW, 2, v.CB, true), 2, v.CB, v.DS};
                else fits = false;   // (the step does not apply)
            }
            if (fits) v.TMAX = class_tmax(v.W, v.NW, v.RM, v.CB, full != 0);
            if (!fits) { printf("%d %d %d %d %d %d %d -1 -1 -1\n", kind, rm, sw, cb, full, spread, maxlen); continue; }
            printf("%d %d %d %d %d %d %d %d %d %d\n", kind, rm, sw, cb, full, spread, maxlen, v.W, v.NW, v.TMAX);
            for (int cvx = 0; cvx < 2; ++cvx) for (int ds = 0; ds < 2; ++ds) {
                Variant u = v;
                u.DS = ds != 0;
                if (ds && !(rm == 2 && v.CB == 2 && cvx)) continue;   // (the host asks for the default-score class of those only)
                if (!class_built(u, cvx != 0, sw != 0, (ClassKind)kind)) fault("no class built", kind, rm, sw, cb, full, spread, maxlen, v);
            }
            const ClassTraits ct = class_traits(v.TMAX, v.W, v.RM, v.CB);
            if (ct.tfix && ct.tfix != v.T()) fault("fixed thread count", kind, rm, sw, cb, full, spread, maxlen, v);
            if (ct.rp == 2 && !full) fault("full-plane class on a narrowed plane", kind, rm, sw, cb, full, spread, maxlen, v);
            if (v.Lpad() < maxlen + 1) fault("columns do not cover the sequence", kind, rm, sw, cb, full, spread, maxlen, v);
            if (v.T() > v.TMAX) fault("more threads than the class's bound", kind, rm, sw, cb, full, spread, maxlen, v);
        }
    }
    if (bad) fprintf(stderr, "%d faults\n", bad);
    return bad ? 1 : 0;
}

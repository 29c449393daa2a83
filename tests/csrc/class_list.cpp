// TEST HARNESS: every kernel class that is built (smoothxg_amd/csrc/poa_classes.h: kClasses), one line per instantiation.  Never shipped.
//
//   class_list           prints: kind rm cb tmax W sw ds      (kind 0 = block kernel, 1 = align-only; sw 1 = local, 0 = global;
//                        ds 1 = the instantiation for the default scores).  Every line exists for the convex and the affine gap model.
// tests/test_class_matrix_fixture.py compares the list with the classes the cases of tests/golden/class_matrix.json run on.
#include <cstdio>

#include "../../smoothxg_amd/csrc/poa_classes.h"

int main() {
    int n = 0;
    for (int r = 0; r < kNumClasses; ++r) {
        const ClassRow& c = kClasses[r];
        for (int rm = 0; rm <= CLASS_RM_MAX; ++rm) {
            if (!(c.rms & cw(rm))) continue;
            for (int w = CLASS_W_MIN; w <= CLASS_W_MAX; ++w) {
                if (!(c.widths & cw(w))) continue;
                for (int sw = 1; sw >= 0; --sw) {
                    if (!(c.modes & (sw ? CLS_LOCAL : CLS_GLOBAL))) continue;
                    // the row must be the one the host finds for this geometry (no two rows build the same class)
                    if (class_row(c.kind, Variant{w, 1, c.tmax, rm, c.cb}, sw != 0) != r) { fprintf(stderr, "row %d: class listed twice\n", r); return 1; }
                    for (int ds = 0; ds <= ((c.modes & CLS_DS) ? 1 : 0); ++ds, ++n) printf("%d %d %d %d %d %d %d\n", (int)c.kind, rm, c.cb, c.tmax, w, sw, ds);
                }
            }
        }
    }
    return n ? 0 : 1;
}

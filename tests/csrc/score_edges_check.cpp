// TEST HARNESS: what the product's own host-side headers say about the edge score sets of tests/score_edges.py.  Never shipped.
//
//   score_edges_check    reads lines "m n g e q c convex sw maxlen rm cb force_w force_nw" (scores as the kernels see them:
//                        normalised) and prints for each "fits def W NW TMAX":
//     fits   p16_delta_fits (poa_rowcode.h): the three fields of a stored cell's code fit 16 bits -> 2-byte plane cells
//     def    the score set is the one the DS classes are compiled for: p16_default_scores' comparison (poa_dp16.hip.h, a HIP
//            header) restated on the P16_DEF_* constants of poa_fields.h
//     W NW TMAX   variant_for_len and class_tmax (poa_classes.h) for a plane that keeps every strip; -1 -1 -1: no geometry
//                 (rm 3, the banded sweep: one wave of strip width force_w, as sxg_poa_batch_upload sets it)
// The first line is "consts P16_LOCAL_LIMIT P16_BIAS P16_W_MAX p16_top_field(-120, -120, P16_W_MAX)" (poa_fields.h).
// tests/test_score_edges.py compares every line with the Python model of tests/golden/make_class_matrix.py.
#include <cstdio>

#include "../../smoothxg_amd/csrc/poa_classes.h"
#include "../../smoothxg_amd/csrc/poa_fields.h"
#include "../../smoothxg_amd/csrc/poa_rowcode.h"

using namespace sxg;

int main() {
    int m, n, g, e, q, c, convex, sw, maxlen, rm, cb, fw, fnw;
    printf("consts %d %d %d %d\n", P16_LOCAL_LIMIT, P16_BIAS, P16_W_MAX, p16_top_field(-120, -120, P16_W_MAX));
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &m, &n, &g, &e, &q, &c, &convex, &sw, &maxlen, &rm, &cb, &fw, &fnw) == 13) {
        const Scoring S{m, n, g, e, q, c, sw, convex};
        const bool def = convex && m == P16_DEF_M && n == P16_DEF_N && g == P16_DEF_G && e == P16_DEF_E && q == P16_DEF_Q && c == P16_DEF_C;
        Variant v{-1, -1, -1, rm};
        bool fits = true;
        if (rm == 3) v = Variant{fw, 1, -1, 3, cb};
        else fits = variant_for_len(maxlen, rm, &v, sw != 0, cb, fw, fnw);
        if (fits) v.TMAX = class_tmax(v.W, v.NW, rm, cb, true);
        printf("%d %d %d %d %d\n", (int)p16_delta_fits(S), (int)def, fits ? v.W : -1, fits ? v.NW : -1, fits ? v.TMAX : -1);
    }
    return 0;
}

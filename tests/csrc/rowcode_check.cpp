// TEST HARNESS: round-trips the packed sweep's stored-row code (smoothxg_amd/csrc/poa_rowcode.h, compiled for the host) over
// every representable (step, H - oF, H - oO) of a score set, with H at the edges of the sweep's ranges, both halves of a word
// at once.  Usage: rowcode_check m n g e q c; prints "<cells checked> <failures>".
#include <cstdio>
#include <cstdlib>
#include "../../smoothxg_amd/csrc/poa_rowcode.h"

using namespace sxg;

static int pk(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }
static int lo16(int v) { return (short)(v & 0xffff); }
static int hi16(int v) { return (short)((unsigned)v >> 16); }

template <bool CVX, bool BIASED>
static void run(const Scoring& S, long& n, long& bad) {
    const P16Delta D = p16_delta_of(S);
    const P16RowCode R = p16_row_code_of(D, CVX);
    // H of a column and of the one left of it: local alignments hold H + 1024 in [1024, 32767] (P16_BIAS), global ones
    // [-16000, 15800] (P16_NWFLOOR and the range check of the packed sweep)
    const int hmin = BIASED ? 1024 : -16000, hmax = BIASED ? 32767 : 15800;
    for (int step = S.g; step <= S.m - S.g; ++step)
        for (int df = -S.e; df <= -S.g; ++df)
            for (int dq = CVX ? -S.c : 0; dq <= (CVX ? -S.q : 0); ++dq) {
                const int hs[3] = {hmin + (df > dq ? df : dq) + (step > 0 ? step : 0), (hmin + hmax) / 2, hmax + (step < 0 ? step : 0)};
                for (int a = 0; a < 3; ++a) {
                    // the high half walks the same cell backwards through the field ranges: two different cells per word
                    const int step2 = S.m - S.g - (step - S.g), df2 = -S.g - (df + S.e), dq2 = CVX ? -S.q - (dq + S.c) : 0;
                    int h2 = hs[2 - a];
                    if (h2 - step2 < hmin) h2 = hmin + step2;
                    if (h2 - step2 > hmax) h2 = hmax + step2;
                    if (h2 - (df2 > dq2 ? df2 : dq2) < hmin) continue;
                    const int h = pk(hs[a], h2), prev = pk(hs[a] - step, h2 - step2);
                    const int of = pk(hs[a] - df, h2 - df2), oo = CVX ? pk(hs[a] - dq, h2 - dq2) : 0;
                    const unsigned w = (unsigned)p16_row_encode<CVX, BIASED>(h, prev, of, oo, D, R);
                    int hh = prev, gf = 0, go = 0;
                    p16_row_decode<CVX, BIASED>(w, hh, gf, go, R);
                    const bool fits = (w & 0xffffu) < (1u << (D.bH + D.bF + D.bO)) && (w >> 16) < (1u << (D.bH + D.bF + D.bO));
                    const bool ok = fits && lo16(hh) == hs[a] && hi16(hh) == h2 && lo16(gf) == hs[a] - df && hi16(gf) == h2 - df2 &&
                                    (!CVX || (lo16(go) == hs[a] - dq && hi16(go) == h2 - dq2));
                    ++n;
                    if (!ok && ++bad <= 5)
                        fprintf(stderr, "cvx %d biased %d: step %d dF %d dO %d H %d / %d -> code %08x\n", CVX, BIASED, step, df, dq, hs[a], h2, w);
                }
            }
}

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    Scoring S{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), 0, 1};
    long n = 0, bad = 0;
    if (p16_delta_fits(S)) { run<true, true>(S, n, bad); run<true, false>(S, n, bad); }
    S.convex = 0;
    if (p16_delta_fits(S)) { run<false, true>(S, n, bad); run<false, false>(S, n, bad); }
    printf("%ld %ld\n", n, bad);
    return 0;
}

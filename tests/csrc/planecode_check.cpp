// TEST HARNESS: the traceback plane of the packed sweep's 2-byte classes holds stored-row codes (round 11).  Builds strips of
// W cells out of every representable (step, H - oF, H - oO) of a score set, encodes them two strips to a word with the sweep's
// p16_row_encode, lays each strip out as a plane row does -- the H left of the strip, then the codes, as halfwords -- and
// decodes every column with the strip decoder the traceback calls (smoothxg_amd/csrc/poa_rowcode.h, compiled for the host).
// Also the banded sweep's strips (delta codes, p16_plane_code) through the same decoder's DELTA form.
// Usage: planecode_check m n g e q c; prints "<cells checked> <failures>".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../smoothxg_amd/csrc/poa_rowcode.h"

using namespace sxg;

struct Triple { int step, df, dq; };

static int pk(int lo, int hi) { return (int)(((unsigned)lo & 0xffffu) | ((unsigned)hi << 16)); }

// one strip's halfwords (left H, code 0 .. code W-1) -> dwords, as plane_store_strip writes them
template <int W>
static void lay_out(const int left, const unsigned (&code)[W], unsigned (&d)[(W + 2) / 2]) {
    unsigned hw[2 * ((W + 2) / 2)] = {0};
    hw[0] = (unsigned)left & 0xffffu;
    for (int k = 0; k < W; ++k) hw[1 + k] = code[k] & 0xffffu;
    for (int x = 0; x < (W + 2) / 2; ++x) d[x] = hw[2 * x] | (hw[2 * x + 1] << 16);
}

template <int W, bool CVX, bool BIASED>
static void run(const Scoring& S, const std::vector<Triple>& cells, long& n, long& bad) {
    const P16Delta D = p16_delta_of(S);
    const P16RowCode R = p16_row_code_of(D, CVX);
    // H as the sweep holds it: local alignments H + 1024 in [1024, 32767] (P16_BIAS), global ones [-16000, 15800]
    const int hmin = BIASED ? 1024 : -16000, hmax = BIASED ? 32767 : 15800;
    const int maxd = -S.g > -S.q ? -S.g : -S.q;
    const int bases[3] = {hmin + W * -S.g + maxd, (hmin + hmax) / 2, hmax - W * (S.m - S.g)};
    const size_t NC = cells.size();
    for (size_t at = 0; at < NC; at += W)
        for (int a = 0; a < 3; ++a)
            for (int own = 0; own < 2; ++own) {   // own: "strip 0" -- the left word is the strip's own first H, its step 0
                // the low halves walk the list forwards from `at`, the high halves backwards: two different strips per word
                Triple c[2][W];
                int H[2][W], left[2];
                for (int k = 0; k < W; ++k) { c[0][k] = cells[(at + k) % NC]; c[1][k] = cells[(NC - 1 - ((at + k) % NC))]; }
                for (int hf = 0; hf < 2; ++hf) {
                    left[hf] = bases[hf ? 2 - a : a];
                    if (own) c[hf][0].step = 0;
                    int h = left[hf];
                    for (int k = 0; k < W; ++k) { h += c[hf][k].step; H[hf][k] = h; }
                }
                unsigned rc[2][W], dc[2][W];
                int prev = pk(left[0], left[1]);
                for (int k = 0; k < W; ++k) {
                    const int h = pk(H[0][k], H[1][k]);
                    const int of = pk(H[0][k] - c[0][k].df, H[1][k] - c[1][k].df);
                    const int oo = CVX ? pk(H[0][k] - c[0][k].dq, H[1][k] - c[1][k].dq) : 0;
                    const unsigned w = (unsigned)p16_row_encode<CVX, BIASED>(h, prev, of, oo, D, R);
                    const unsigned p = (unsigned)p16_plane_code<CVX, BIASED>(h, prev, of, oo, D);
                    rc[0][k] = w & 0xffffu; rc[1][k] = w >> 16;
                    dc[0][k] = p & 0xffffu; dc[1][k] = p >> 16;
                    prev = h;
                }
                for (int hf = 0; hf < 2; ++hf) {
                    unsigned dr[(W + 2) / 2], dd[(W + 2) / 2];
                    lay_out<W>(left[hf], rc[hf], dr);
                    lay_out<W>(left[hf], dc[hf], dd);
                    auto half_r = [&](const int hw) -> unsigned { return p16_strip_half(dr, hw); };
                    auto half_d = [&](const int hw) -> unsigned { return p16_strip_half(dd, hw); };
                    for (int k = 0; k < W; ++k) {
                        const int eh = H[hf][k], ef = eh - c[hf][k].df, eo = CVX ? eh - c[hf][k].dq : eh;
                        int h[3], f[3], o[3];
                        p16_strip_decode<CVX, false, W>(half_r, k, h[0], f[0], o[0], D);   // unrolled form (strips in registers)
                        p16_strip_decode<CVX, false, 0>(half_r, k, h[1], f[1], o[1], D);   // loop form
                        p16_strip_decode<CVX, true, 0>(half_d, k, h[2], f[2], o[2], D);    // banded sweep: delta codes
                        for (int v = 0; v < 3; ++v) {
                            ++n;
                            if (h[v] == eh && f[v] == ef && o[v] == eo) continue;
                            if (++bad <= 5)
                                fprintf(stderr, "W %d cvx %d biased %d own %d form %d: column %d step %d dF %d dO %d H %d -> H %d oF %d oO %d (want %d %d %d)\n",
                                        W, CVX, BIASED, own, v, k, c[hf][k].step, c[hf][k].df, c[hf][k].dq, eh, h[v], f[v], o[v], eh, ef, eo);
                        }
                    }
                }
            }
}

template <bool CVX>
static void run_set(const Scoring& S, long& n, long& bad) {
    std::vector<Triple> cells;
    for (int step = S.g; step <= S.m - S.g; ++step)
        for (int df = -S.e; df <= -S.g; ++df)
            for (int dq = CVX ? -S.c : 0; dq <= (CVX ? -S.q : 0); ++dq) cells.push_back(Triple{step, df, dq});
    run<4, CVX, true>(S, cells, n, bad);  run<4, CVX, false>(S, cells, n, bad);
    run<11, CVX, true>(S, cells, n, bad); run<11, CVX, false>(S, cells, n, bad);
    run<13, CVX, true>(S, cells, n, bad); run<13, CVX, false>(S, cells, n, bad);
}

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    Scoring S{atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), 0, 1};
    long n = 0, bad = 0;
    if (p16_delta_fits(S)) run_set<true>(S, n, bad);
    S.convex = 0;
    if (p16_delta_fits(S)) run_set<false>(S, n, bad);
    printf("%ld %ld\n", n, bad);
    return 0;
}

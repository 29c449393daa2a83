// TEST HARNESS: the second strip width of the packed block classes (smoothxg_amd/csrc/poa_classes.h: ClassRow::widths2, class_w2,
// width_for_len) against the slot layout and the LDS sizes the host gives a dual-width launch (poa_kernels.hip.h::make_layout,
// p16_launch_sizes -- what sxg_poa.hip::prepare_plan calls, SXG_POA_BAND_COLS and SXG_POA_LDS_ROWS included).  Host code only, no
// GPU: compile with `hipcc -x hip --offload-host-only`.  Never shipped.
//
//   width2_check     prints one line per built class with a second width: tmax W W2 cb band_strips band_strips2 plane_bytes
//                    pool_bytes lds_bytes lds_rows (defaults), and fails (exit status 1, reasons on stderr) when
//                      * the plane, the pool, row 0 or the launch's LDS do not hold a sweep at either width,
//                      * width_for_len is not the narrowest of W2, W that covers a length,
//                      * a class outside the packed 2-byte block classes of four and eight waves has a second width.
#include <cstdio>
#include <cstdlib>

#include "../../smoothxg_amd/csrc/poa_kernels.hip.h"

static int bad = 0;
static void fault(const char* what, int tmax, int W, int W2, long a, long b) {
    if (++bad <= 20) fprintf(stderr, "%s: tmax=%d W=%d W2=%d (%ld against %ld)\n", what, tmax, W, W2, a, b);
}

int main() {
    int seen = 0;
    for (int r = 0; r < kNumClasses; ++r) {
        const ClassRow& c = kClasses[r];
        for (int W = CLASS_W_MIN; W <= CLASS_W_MAX; ++W) {
            if (!(c.widths & cw(W))) { if (c.widths2 & cw(W)) fault("second width of a width that is not built", c.tmax, W, W - 1, 0, 0); continue; }
            for (int sw = 0; sw < 2; ++sw) {
                if (!(c.modes & (sw ? CLS_LOCAL : CLS_GLOBAL)) || !(c.rms & RM2)) continue;
                const Variant v{W, c.tmax / 64, c.tmax, 2, c.cb};
                const int W2 = class_w2(c.kind, v, sw != 0);
                const bool may = c.kind == CLASS_BLOCK && c.cb == 2 && (c.tmax == 256 || c.tmax == 512) && W >= 9 && W <= 12;
                if ((W2 != 0) != may) fault("second width where none is meant, or none where one is", c.tmax, W, W2, W2, may);
                if (!W2 || sw) continue;   // (the layout does not depend on the alignment mode: once per class)
                ++seen;
                if (W2 != W - 1) fault("second width is not W - 1", c.tmax, W, W2, W2, W - 1);
                if (class_row(c.kind, Variant{W2, v.NW, c.tmax, 2, c.cb}, false) != r) fault("no class of its own at the second width", c.tmax, W, W2, 0, 0);
                const int T = v.T(), CB = c.cb;
                // the choice: the narrowest covering width, for every length the geometry takes
                // (expected independently of the function: the first of the ascending candidate widths whose 2 T strips hold the
                //  letters and the column in front of them)
                for (int len = 0; len + 1 <= T * 2 * W; ++len) {
                    const int wk = width_for_len(W, W2, T, len);
                    int want = -1;
                    for (int cand = 1; cand <= W && want < 0; ++cand)
                        if ((cand == W2 || cand == W) && (long)cand * 2 * T > len) want = cand;
                    if (wk != want) { fault("width_for_len", c.tmax, W, W2, wk, want); break; }
                    if (width_for_len(W, 0, T, len) != W) { fault("width_for_len without a second width", c.tmax, W, W2, len, W); break; }
                }
                // the launch as the host sizes it (p16_launch_sizes): banded plane at its default and narrowed by SXG_POA_BAND_COLS,
                // the every-strip plane of a band-miss re-run, on-chip rows at their default and forced by SXG_POA_LDS_ROWS
                static const char* const band_cols[] = {nullptr, "480", "32", "100000"};
                static const char* const lds_rows_env[] = {nullptr, "0", "8"};
                for (const char* bc : band_cols) for (const char* lr : lds_rows_env) for (int wide = 0; wide < 2; ++wide) {
                    if (bc) setenv("SXG_POA_BAND_COLS", bc, 1); else unsetenv("SXG_POA_BAND_COLS");
                    if (lr) setenv("SXG_POA_LDS_ROWS", lr, 1); else unsetenv("SXG_POA_LDS_ROWS");
                    const int rows_cap = 3000, pool_slots = 768;
                    const P16LaunchSizes S = p16_launch_sizes(T, W, W2, CB, wide != 0);
                    const P16LaunchSizes S1 = p16_launch_sizes(T, W, 0, CB, wide != 0);
                    const SlotLayout L = make_layout(8000, rows_cap, pool_slots, rows_cap, T, v.Lpad(), 4, false, S.strips, CB, false, W2, S.strips2);
                    const SlotLayout L1 = make_layout(8000, rows_cap, pool_slots, rows_cap, T, v.Lpad(), 4, false, S1.strips, CB, false);
                    if (L.W2 != W2 || L.band_strips != S.strips || L.band_strips2 != S.strips2) fault("layout does not carry the widths", c.tmax, W, W2, L.W2, L.band_strips2);
                    if (S1.strips2 != 0 || S1.strips != S.strips || S1.lds_rows != S.lds_rows || S1.smem > S.smem) fault("single-width launch", c.tmax, W, W2, S1.smem, S.smem);
                    if (L1.W2 != 0 || L1.band_strips2 != 0 || L1.total > L.total) fault("single-width layout", c.tmax, W, W2, (long)L1.total, (long)L.total);
                    const long plane = (long)(L.steps - L.tb), pool = (long)(L.row0 - L.pool), row0 = (long)(L.park - L.row0);
                    const int wk[2] = {W, W2}, bs[2] = {S.strips, S.strips2};
                    for (int k = 0; k < 2; ++k) {
                        // the band a sweep at this width asks for: every strip (wide), or the columns of the knob / ~1 100, in strips of
                        // ITS width, a multiple of 4, at most the geometry's 2 T strips
                        const int cols = bc ? std::max(atoi(bc), wk[k]) : 1100;
                        const int want_bs = wide ? 2 * T : std::min(((cols + wk[k] - 1) / wk[k] + 3) / 4 * 4, 2 * T);
                        if (bs[k] != want_bs) fault("strips per plane row", c.tmax, W, wk[k], bs[k], want_bs);
                        const long need_plane = ((long)rows_cap + 1) * bs[k] * p16_slot_dwords(wk[k], CB) * 4;
                        const long row = dp16_row_bytes(T, wk[k], CB);
                        if (plane < need_plane) fault("plane too small", c.tmax, W, wk[k], plane, need_plane);
                        if (pool < pool_slots * row) fault("pool too small", c.tmax, W, wk[k], pool, pool_slots * row);
                        if (row0 < row) fault("row 0 too small", c.tmax, W, wk[k], row0, row);
                        // LDS of a sweep at this width with the launch's on-chip rows: control words, mailbox / window area, row copies, letters
                        const long need_lds = LDS_CTL_BYTES + dp16_meta_bytes(T) + (long)S.lds_rows * row + (long)T * dp16_let_words(wk[k]) * 4;
                        if (S.smem < need_lds) fault("LDS too small", c.tmax, W, wk[k], S.smem, need_lds);
                    }
                    if (lr && S.lds_rows != atoi(lr)) fault("on-chip rows do not follow the knob", c.tmax, W, W2, S.lds_rows, atoi(lr));
                    // by default four workgroups of four waves (two of eight) share a CU's 160 KB
                    if (!lr && (long)S.smem * (16 / (T / 64)) > 160 * 1024) fault("LDS beyond the workgroup's share of a CU", c.tmax, W, W2, S.smem, 0);
                    if (!bc && !lr && !wide)
                        printf("%d %d %d %d %d %d %ld %ld %d %d\n", c.tmax, W, W2, CB, S.strips, S.strips2, plane, pool, S.smem, S.lds_rows);
                }
            }
        }
    }
    if (seen != 8) { fprintf(stderr, "%d classes with a second width, 8 expected (four and eight waves, W = 9 .. 12)\n", seen); ++bad; }
    if (bad) fprintf(stderr, "%d faults\n", bad);
    return bad ? 1 : 0;
}

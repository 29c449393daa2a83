// poa_classes.h -- the engine's kernel classes: which exist, what each is compiled for, which one a geometry runs on.
//
// Plain C++17, constexpr, no HIP: included by the kernels (poa_kernels.hip.h reads class_traits), by the translation units that
// instantiate the classes (poa_kern_tables.hip.h walks kClasses), by the host (sxg_poa.hip: variant_for_len, class_tmax,
// class_built) and by the host-only check of the choice (tests/csrc/class_check.cpp).
//
// Adding a class: one row in kClasses; if it is compiled for something new, one line in class_traits.
#pragma once

// A launch geometry: W columns per strip, NW waves (T = 64*NW), kernel class TMAX, row mode RM
// (2 = packed sweep: two strips per lane; 3 = banded), CB = bytes per plane cell of the packed sweep (poa_dp16.hip.h).
struct Variant {
    int W, NW, TMAX, RM;
    int CB = 4;
    bool DS = false;   // the class compiled for smoothxg's default scores (packed sweep, 2-byte cells, convex)
    // second strip width of the launch's class (class_w2; 0 = none): an alignment whose sequence fits T * 2 * W2 columns sweeps
    // strips of W2 columns.  Follows from the class (prepare_plan sets it); not part of a geometry's identity (operator==).
    int W2 = 0;
    constexpr int T() const { return 64 * NW; }
    constexpr int Lpad() const { return 64 * NW * W * (RM >= 2 ? 2 : 1); }
    constexpr bool operator==(const Variant& o) const { return W == o.W && NW == o.NW && TMAX == o.TMAX && RM == o.RM && CB == o.CB && DS == o.DS; }
    constexpr bool operator!=(const Variant& o) const { return !(*this == o); }
};
// the same kind of class: everything but the size (launches of the same kind may merge)
constexpr bool same_kind(const Variant& a, const Variant& b) { return a.RM == b.RM && a.CB == b.CB && a.DS == b.DS; }

// What a class <TMAX, W, RM, CB> is compiled for.
struct ClassTraits {
    int rp;           // packed sweep reads stored rows back from the plane: 0 = no, 1 = yes, 2 = yes, from a plane that keeps EVERY strip
    int tfix;         // the thread count the sweep is compiled for (the launch must run at exactly that), 0 = read at run time
    int min_waves;    // second launch bound: waves per SIMD the register allocator leaves room for
    int graph_batch;  // elements per thread and step of the graph phases (WgCtxT<>): 16, 8 or 4; a class of 8 run on one wave takes 16
    int twin;         // packed sweep: sibling rows are swept in one step and joined from registers (ROW_TWIN / ROW_JOIN, poa_types.h)
};
constexpr ClassTraits class_traits(int TMAX, int W, int RM, int CB) {
    const bool p2 = RM == 2 && CB == 2;   // packed sweep, 2-byte delta plane cells
    ClassTraits t{};
    // one and two waves read stored rows back from the plane; one wave up to W = 11 covers at most 1 408 columns, whose plane keeps
    // every strip by construction (p16_band_strips), and is compiled for that alone
    t.rp = (p2 && TMAX <= 128) ? ((TMAX == 64 && W <= 11) ? 2 : 1) : 0;
    // up to eight waves: compiled for exactly TMAX threads (1.6 % on the headline; the two-wave class measured 1 % slower that way)
#ifdef SXG_DEV_TFIX128
    t.tfix = (p2 && TMAX <= 512) ? TMAX : 0;
#else
    t.tfix = (p2 && TMAX <= 512 && TMAX != 128) ? TMAX : 0;
#endif
    // 8 columns per lane need ~100 VGPRs (4 waves), 16 need ~165 (3 waves); a 1024-thread workgroup is 4 waves per SIMD by itself
    // (packed sweep: 128 VGPRs hold up to 13 columns per strip since round 2 -- two 8-wave workgroups share a CU)
#ifdef SXG_DEV_WAVES
    t.min_waves = SXG_DEV_WAVES;
#else
    t.min_waves = TMAX > 512 ? 4 : (RM == 2 ? 4 : (W <= 12 ? 4 : 3));
#endif
    t.graph_batch = TMAX == 64 ? 16 : (TMAX <= 128 ? 8 : 4);
    // the packed classes of three waves and more (2-byte cells, stored rows never read back from the plane)
    t.twin = (p2 && t.rp == 0) ? 1 : 0;
    return t;
}

// ---------------------------------------------------------------------------------------
// The classes that are built.  One row: the translation unit ("part", smoothxg_amd/build.py compiles kern_part.hip once per
// part) that holds them, block or align-only kernel, row modes, plane cell bytes, TMAX, the strip widths, and which alignment
// modes exist (every class exists for the convex and the affine gap model; CLS_DS: also compiled for the default scores, convex).
// The assignment to parts balances the build; a part's classes are instantiated row by row, width by width, row mode by row mode.
enum ClassKind { CLASS_BLOCK = 0, CLASS_ALIGN = 1 };
enum : unsigned { CLS_LOCAL = 1, CLS_GLOBAL = 2, CLS_BOTH = 3, CLS_DS = 4 };
// widths2: the widths W of the row whose classes are also compiled for strips of W - 1 columns (the second width, picked per
// alignment inside the block kernel -- poa_kernels.hip.h)
struct ClassRow { int part; ClassKind kind; unsigned rms; int cb, tmax; unsigned widths, modes; unsigned widths2 = 0; };
constexpr unsigned cw(int w) { return 1u << w; }   // a strip width / a row mode as a bit of ClassRow::widths / rms
constexpr unsigned RM0 = cw(0), RM1 = cw(1), RM2 = cw(2), RM3 = cw(3), RM01 = RM0 | RM1;
constexpr unsigned cw_range(int lo, int hi) { unsigned m = 0; for (int w = lo; w <= hi; ++w) m |= cw(w); return m; }
constexpr int CLASS_W_MIN = 4, CLASS_W_MAX = 16, CLASS_RM_MAX = 3, CLASS_PARTS = 9;
constexpr ClassRow kClasses[] = {
    // part 1: the banded one-wave sweep (2-byte band cells: local alignment only), the 32-bit sweeps (int16 and int32 row words)
    {1, CLASS_BLOCK, RM3, 2, 64, cw(6) | cw(8) | cw(11), CLS_LOCAL},
    {1, CLASS_BLOCK, RM3, 4, 64, cw(6) | cw(8) | cw(11), CLS_BOTH},
    // (no 8-column class of 8 or 16 waves: 8 x 8, 12 x 8 and 16 x 8 waves-by-columns tie with 4 x 16, 8 x 12 and 8 x 16, and the
    //  wider strip wins -- variant_for_len never returns them for a 32-bit sweep, which has no forced geometry either)
    {1, CLASS_BLOCK, RM01, 4, 256, cw(8) | cw(12) | cw(16), CLS_BOTH},
    {1, CLASS_BLOCK, RM01, 4, 512, cw(12) | cw(16), CLS_BOTH},
    {1, CLASS_BLOCK, RM01, 4, 1024, cw(12), CLS_BOTH},
    {1, CLASS_ALIGN, RM01, 4, 256, cw(8) | cw(12) | cw(16), CLS_BOTH},
    {1, CLASS_ALIGN, RM01, 4, 512, cw(12) | cw(16), CLS_BOTH},
    {1, CLASS_ALIGN, RM01, 4, 1024, cw(12), CLS_BOTH},
    // parts 2, 3: packed sweep, block kernels, 2-byte delta plane cells, 4 / 8 and 16 waves
    // (the long classes, 16 waves of 10, 12, 13 columns, exist for local alignment only: a global score of such lengths does not fit int16)
    // (W = 9 .. 12 with the second width W - 1: sequences of 4.6-6.1 kbp and 9.2-12.3 kbp, whose blocks mix lengths on either side
    //  of a width's columns)
    {2, CLASS_BLOCK, RM2, 2, 256, cw_range(4, 12), CLS_BOTH | CLS_DS, cw_range(9, 12)},
    {3, CLASS_BLOCK, RM2, 2, 512, cw_range(8, 12), CLS_BOTH | CLS_DS, cw_range(9, 12)},
    {3, CLASS_BLOCK, RM2, 2, 1024, cw(8), CLS_BOTH | CLS_DS},
    {3, CLASS_BLOCK, RM2, 2, 1024, cw(10) | cw(12) | cw(13), CLS_LOCAL | CLS_DS},
    // parts 4, 5: ... 4-byte plane cells (score sets whose deltas do not fit 16 bits); no class of its own for one to three waves
    {4, CLASS_BLOCK, RM2, 4, 256, cw_range(4, 12), CLS_BOTH},
    {5, CLASS_BLOCK, RM2, 4, 512, cw_range(8, 12), CLS_BOTH},
    {5, CLASS_BLOCK, RM2, 4, 1024, cw(8), CLS_BOTH},
    {5, CLASS_BLOCK, RM2, 4, 1024, cw(10) | cw(12) | cw(13), CLS_LOCAL},
    // part 6: packed sweep, align-only kernels (4-byte cells)
    {6, CLASS_ALIGN, RM2, 4, 256, cw_range(4, 12), CLS_BOTH},
    {6, CLASS_ALIGN, RM2, 4, 512, cw_range(8, 12), CLS_BOTH},
    {6, CLASS_ALIGN, RM2, 4, 1024, cw(8), CLS_BOTH},
    {6, CLASS_ALIGN, RM2, 4, 1024, cw(10) | cw(12) | cw(13), CLS_LOCAL},
    // parts 7, 8, 9: packed sweep, block kernels, 2-byte cells, two-, one- and three-wave workgroups
    {7, CLASS_BLOCK, RM2, 2, 128, cw_range(4, 12), CLS_BOTH | CLS_DS},
    {8, CLASS_BLOCK, RM2, 2, 64, cw_range(4, 12), CLS_BOTH | CLS_DS},
    {9, CLASS_BLOCK, RM2, 2, 192, cw_range(4, 12), CLS_BOTH | CLS_DS},
};
constexpr int kNumClasses = (int)(sizeof(kClasses) / sizeof(kClasses[0]));

// the row of kClasses that holds the class of geometry v for local (sw) or global alignment, -1: none built
constexpr int class_row(ClassKind kind, const Variant& v, bool sw) {
    if (v.W < CLASS_W_MIN || v.W > CLASS_W_MAX || v.RM < 0 || v.RM > CLASS_RM_MAX) return -1;
    for (int r = 0; r < kNumClasses; ++r) {
        const ClassRow& c = kClasses[r];
        if (c.kind == kind && (c.rms & cw(v.RM)) && c.cb == v.CB && c.tmax == v.TMAX && (c.widths & cw(v.W)) && (c.modes & (sw ? CLS_LOCAL : CLS_GLOBAL)))
            return r;
    }
    return -1;
}
// The second strip width of the class of geometry v (0: the class has none), and the width an alignment of `len` letters runs
// at on T threads: the narrowest of W2 and W that covers it (a sequence beyond W's columns is ST_TOO_LONG, tested against W).
constexpr int class_w2(ClassKind kind, const Variant& v, bool sw) {
    const int r = class_row(kind, v, sw);
    return r >= 0 && (kClasses[r].widths2 & cw(v.W)) ? v.W - 1 : 0;
}
constexpr int width_for_len(int W, int W2, int T, int len) { return W2 != 0 && len + 1 <= T * 2 * W2 ? W2 : W; }
// (cvx: both gap models of a row are built; a geometry that asks for the default-score class of a row without one runs the general class)
constexpr bool class_built(const Variant& v, bool /*cvx*/, bool sw, ClassKind kind = CLASS_BLOCK) { return class_row(kind, v, sw) >= 0; }

// ---------------------------------------------------------------------------------------
// Which class a geometry runs on.  32-bit sweeps: classes of 4, 8 and 16 waves.  Packed sweep: 2-byte cells have classes of their
// own for one, two and three waves; the one-wave class that is compiled for a plane that keeps every strip (rp == 2) gives way to
// the two-wave class, run at 64 threads, when the launch's plane was narrowed (full_plane == false: SXG_POA_BAND_COLS).
constexpr int class_tmax(int W, int NW, int RM, int CB, bool full_plane) {
    if (RM == 3) return 64;
    int t = NW <= 4 ? 256 : (NW <= 8 ? 512 : 1024);
    if (RM == 2 && CB == 2 && NW <= 4) t = 64 * NW;
    if (class_traits(t, W, RM, CB).rp == 2 && !full_plane) t = 128;
    return t;
}

// Geometry choice.  Inside a workgroup all waves meet at two barriers per row, so the wave
// count should load the four SIMDs of a CU evenly: 1, 2, 3, 4, 8, 12 or 16 waves.  Among the
// (W, NW) pairs that cover the sequence pick the one with the fewest padded columns, then the
// wider strip (less per-row overhead).  Strip widths are bounded by VGPRs: 32-bit sweep 16
// columns (~165 VGPRs, <= 512 threads) / 12 (128 VGPRs); packed sweep 12 (~152) / 8 (124).
// Long local alignments (sequences of 12-26 kbp: smoothxg runs with -l 13k cut at 2 * 13k) get 16-wave workgroups of the
// packed sweep with 10, 12 or 13 columns per strip (128 VGPRs, a handful of spill slots): 20 480 / 24 576 / 26 624 columns.
// cb: plane cell bytes of the packed sweep (4 for the other row modes and for the align-only kernels); force_w, force_nw:
// a packed geometry the caller insists on if it covers the sequence (development knob SXG_POA_FORCE_P16), 0 = none.
// The class is the one of a plane that keeps every strip; the launch settles that (prepare_plan).
constexpr bool variant_for_len(int maxlen, int rm, Variant* v, bool sw = false, int cb = 4, int force_w = 0, int force_nw = 0) {
    constexpr int kNW[] = {1, 2, 3, 4, 8, 12, 16};
    if (rm == 2 && force_w > 0 && 128L * force_nw * force_w >= maxlen + 1 && (force_nw <= 4 || force_nw == 8 || force_nw == 12 || force_nw == 16)) {
        *v = Variant{force_w, force_nw, class_tmax(force_w, force_nw, rm, cb, true), rm, cb};
        return true;
    }
    // (narrow strips, 4-7 columns, for sequences below 1 kbp -- pggb's -l 700 ... 1100 -- in workgroups of up to 4 waves)
    constexpr int kW32[] = {16, 12, 8}, kW16[] = {13, 12, 11, 10, 9, 8, 7, 6, 5, 4};
    const int* ws = rm == 2 ? kW16 : kW32;
    const int nws = rm == 2 ? 10 : 3;
    const int need = maxlen + 1;
    long best_cols = -1;
    for (int wi = 0; wi < nws; ++wi)
        for (int NW : kNW) {
            const int W = ws[wi];
            const long cols = 64L * NW * W * (rm == 2 ? 2 : 1);
            if (cols < need) continue;
            const bool wide = rm == 2 ? W > 8 : W > 12;   // needs > 128 VGPRs unless squeezed
            const bool long_class = rm == 2 && sw && NW == 16 && (W == 10 || W == 12 || W == 13);
            if (W == 13 && !long_class) continue;
            if (rm == 2 && W < 8 && NW > 4) continue;
            if (wide && NW > 8 && !long_class) continue;
            if (best_cols < 0 || cols < best_cols) {
                best_cols = cols;
                *v = Variant{W, NW, class_tmax(W, NW, rm, cb, true), rm, cb};
            }
            break;  // larger NW for this W only adds padding
        }
    return best_cols >= 0;
}

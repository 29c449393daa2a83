// poa_repeat.h -- the arithmetic of the tandem-repeat scan (decree R of DESIGN.md section 9 / include/sxg_poa.h), HIP-free: the
// lag range of a sequence, the samples of a lag, the tiling of the lags into work items, what ONE LANE of the counting kernel
// reads and counts (repeat_count_kernel of poa_repeat.hip.h calls sxg_repeat_lane_counts and nothing else touches the letters),
// and the double-precision pass over a sequence's counts (repeat_stats_kernel calls sxg_repeat_stats).  tests/csrc/
// repeat_check.cpp walks the same functions lane by lane over heap buffers of exactly n bytes, under AddressSanitizer.
//
// A work item is (sequence, tile): SXG_REPEAT_TILE_LAGS consecutive lags, one wavefront.  Lane l of the item owns the
// SXG_REPEAT_LANE_LAGS consecutive lags k0 = tile * TILE + l * LANE_LAGS ... (lag index k stands for the lag L = min_copy + k),
// so for the sample at position i the wavefront reads the 256 consecutive bytes s[i + L(tile)] ..., four per lane, and compares
// them with the ONE letter s[i] all at once: XOR against the replicated letter, a 1 in every byte that came out zero, added to
// four 8-bit counters packed in a word, which are unpacked into 32-bit counts every 255 samples (R2: nothing is approximate).
// The 4-byte read is taken only where all four bytes lie inside the sequence; the few samples that only the smaller lags of a
// lane still have (and every sample of a lane at the sequence's very end) are compared byte by byte, each behind its own guard.
#ifndef SXG_POA_REPEAT_H
#define SXG_POA_REPEAT_H
#include <stdint.h>
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define SXG_RHD __host__ __device__ __forceinline__
#else
#define SXG_RHD inline
#endif

#define SXG_REPEAT_LANE_LAGS 4
#define SXG_REPEAT_WAVE 64
#define SXG_REPEAT_TILE_LAGS (SXG_REPEAT_WAVE * SXG_REPEAT_LANE_LAGS)
#define SXG_REPEAT_FLUSH 255   // samples a packed 8-bit counter takes before it is unpacked
// R4: the longest sequence whose first lag of greatest r is provably the first lag of greatest z (= SXG_POA_REPEAT_MAX_LEN)
#define SXG_REPEAT_MAX_LEN (1 << 20)

// R2: the number of lags of a sequence of n letters, L = min_copy ... min(max_copy, n - min_copy); 0 below 2 min_copy letters
SXG_RHD int64_t sxg_repeat_n_lags(int64_t n, int64_t min_copy, int64_t max_copy) {
    if (min_copy <= 0 || max_copy < min_copy || n < 2 * min_copy) return 0;
    const int64_t hi = max_copy < n - min_copy ? max_copy : n - min_copy;
    return hi - min_copy + 1;
}
// (from here on 32-bit: the device sees sequences of at most SXG_REPEAT_MAX_LEN letters, and a stride or a max_copy beyond that
// limit clamped to it, which changes no count)
// R2: the samples i = 0, stride, 2 stride, ... < n - L of lag L; 0 where L >= n
SXG_RHD int32_t sxg_repeat_cnt(int32_t n, int32_t L, int32_t stride) { return L < n ? (n - L + stride - 1) / stride : 0; }
// the work items of a sequence
SXG_RHD int32_t sxg_repeat_n_tiles(int32_t n_lags) { return (n_lags + SXG_REPEAT_TILE_LAGS - 1) / SXG_REPEAT_TILE_LAGS; }
// the first lag index of a lane of an item
SXG_RHD int32_t sxg_repeat_lane_first(int32_t tile, int lane) { return tile * SXG_REPEAT_TILE_LAGS + lane * SXG_REPEAT_LANE_LAGS; }
// the samples of a lane whose LANE_LAGS bytes s[i + L0] ... s[i + L0 + LANE_LAGS - 1] all lie inside the sequence
SXG_RHD int32_t sxg_repeat_full_samples(int32_t n, int32_t L0, int32_t stride) { return sxg_repeat_cnt(n, L0 + SXG_REPEAT_LANE_LAGS - 1, stride); }
// the counts of a batch: sequence s's n_lags 32-bit counts stand at match + match_off[s] (match_off[0] = 0, [n_seqs + 1]); a
// sequence beyond the length limit is declined and has none
inline void sxg_repeat_match_offsets(int64_t n_seqs, const int64_t* seq_off, int64_t min_copy, int64_t max_copy, int64_t* match_off) {
    match_off[0] = 0;
    for (int64_t s = 0; s < n_seqs; ++s) {
        const int64_t n = seq_off[s + 1] - seq_off[s];
        match_off[s + 1] = match_off[s] + (n > SXG_REPEAT_MAX_LEN ? 0 : sxg_repeat_n_lags(n, min_copy, max_copy));
    }
}

SXG_RHD uint32_t sxg_repeat_load4(const uint8_t* p) { uint32_t w; memcpy(&w, p, 4); return w; }   // (any alignment; byte q is p[q])
// 1 in every byte of w that equals the letter c
SXG_RHD uint32_t sxg_repeat_eq4(uint32_t w, uint8_t c) {
    const uint32_t x = w ^ ((uint32_t)c * 0x01010101u);
    return (~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u) >> 7;
}

// ONE LANE of item (sequence s of n letters, tile): out[q] = match(min_copy + k0 + q) for its m = min(LANE_LAGS, n_lags - k0) lags
// (R2); returns m, 0 for a lane beyond the sequence's lags.  Reads s[0 .. n) and nothing else.
SXG_RHD int sxg_repeat_lane_counts(const uint8_t* s, int32_t n, int32_t min_copy, int32_t n_lags, int32_t stride, int32_t tile, int lane,
                                   int32_t out[SXG_REPEAT_LANE_LAGS]) {
    const int32_t k0 = sxg_repeat_lane_first(tile, lane);
    if (k0 >= n_lags) return 0;
    const int m = n_lags - k0 < SXG_REPEAT_LANE_LAGS ? (int)(n_lags - k0) : SXG_REPEAT_LANE_LAGS;
    const int32_t L0 = min_copy + k0;
    const int32_t full = sxg_repeat_full_samples(n, L0, stride);
    uint32_t c[SXG_REPEAT_LANE_LAGS];
    for (int q = 0; q < SXG_REPEAT_LANE_LAGS; ++q) c[q] = 0;
    for (int32_t j0 = 0; j0 < full; j0 += SXG_REPEAT_FLUSH) {
        const int32_t j1 = full - j0 < SXG_REPEAT_FLUSH ? full : j0 + SXG_REPEAT_FLUSH;
        uint32_t acc = 0;
#pragma GCC unroll 4
        for (int32_t j = j0; j < j1; ++j) acc += sxg_repeat_eq4(sxg_repeat_load4(s + j * stride + L0), s[j * stride]);   // the sample against the four letters L0 ... L0 + 3 later
        for (int q = 0; q < SXG_REPEAT_LANE_LAGS; ++q) c[q] += (acc >> (8 * q)) & 0xffu;
    }
    // the samples past `full`: lag L0 + q still has those with i + L0 + q < n
    for (int32_t i = full * stride; i + L0 < n; i += stride)
        for (int q = 0; q < m; ++q)
            if (i + L0 + q < n) c[q] += s[i] == s[i + L0 + q] ? 1u : 0u;
    for (int q = 0; q < SXG_REPEAT_LANE_LAGS; ++q) out[q] = (int32_t)c[q];
    return m;
}

// R3: the double-precision pass over the n_lags (>= 1) counts of a sequence of n letters, sums in lag order, every operation
// rounded once (the translation unit is built without contraction): best = the first k of the greatest r[k], dev = r[best] - mean,
// v = var / n_lags.
SXG_RHD void sxg_repeat_stats(const int32_t* match, int32_t n, int32_t min_copy, int32_t n_lags, int32_t stride, int32_t* best, double* dev, double* v) {
    double mean = 0.0, top = 0.0;
    int32_t at = 0;
    for (int32_t k = 0; k < n_lags; ++k) {
        const double r = (double)match[k] / (double)sxg_repeat_cnt(n, min_copy + k, stride);
        mean += r;
        if (k == 0 || r > top) { top = r; at = k; }
    }
    mean /= (double)n_lags;
    double var = 0.0;
    for (int32_t k = 0; k < n_lags; ++k) {
        const double r = (double)match[k] / (double)sxg_repeat_cnt(n, min_copy + k, stride);
        var += (r - mean) * (r - mean);
    }
    *best = (int32_t)at;
    *dev = top - mean;
    *v = var / (double)n_lags;
}

// The host's three operations on what sxg_repeat_stats returns (R3): the repeat's length, 0 when there is none.
inline double sxg_repeat_decide(int64_t min_copy, int64_t best, double dev, double v, double min_z) {
    const double sd = sqrt(v);
    if (sd == 0.0) return 0.0;
    return dev / sd >= min_z ? (double)(min_copy + best) : 0.0;
}
#endif

// poa_repeat.hip.h -- the tandem-repeat scan of the cutting half of break_blocks (src/breaks.cpp:224-272) on the device, decree R
// of DESIGN.md section 9: for every sequence the match count of every lag (repeat_count_kernel) and the double-precision pass
// over them (repeat_stats_kernel).  All index arithmetic, the compare and the sums are poa_repeat.h's, which the CPU checks run.
//
// Included by sxg_poa.hip for the argument structs and the launchers' prototypes; kern_repeat.hip defines SXG_REPEAT_IMPL and is
// built without floating-point contraction (R3: one rounding per operation).
//
// Counting.  One wavefront per workgroup; the work items (sequence, tile of SXG_REPEAT_TILE_LAGS lags) of a round stand in a
// list the host sorted largest first, and workgroup g takes items g, g + G, g + 2G, ...: the list is the queue, no counter, no
// atomic.  A lane owns SXG_REPEAT_LANE_LAGS consecutive lags, so the wavefront reads 256 consecutive letters per sample and the
// sampled letter is one address for all of it.  The counts leave as plain 32-bit stores, each written by exactly one lane.
//
// Statistics.  One THREAD per sequence of the round: R3's sums are a chain in lag order, so a sequence has no parallelism to
// give, and the sequences of a round are independent.
#ifndef SXG_POA_REPEAT_HIP_H
#define SXG_POA_REPEAT_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "poa_repeat.h"

#define SXG_REPEAT_STATS_THREADS 64

struct RepeatArgs {
    const uint8_t* bases;       // the batch's letters
    const int64_t* seq_off;     // [n_seqs + 1]
    const int64_t* match_off;   // [n_seqs + 1] (sxg_repeat_match_offsets)
    int64_t match_base;         // match_off of the round's first sequence: the round's counts start at `match`
    int32_t* match;             // the round's counts
    const int32_t* items;       // [2 * n_items] (sequence, tile), largest first
    int32_t n_items;
    const int32_t* work;        // [n_work] the round's sequences that have lags
    int32_t n_work;
    int32_t min_copy, max_copy, stride;
    int32_t* best;              // [n_seqs]
    double* dev;                // [n_seqs]
    double* v;                  // [n_seqs]
};

void sxg_repeat_launch_count(const RepeatArgs& A, int n_groups, hipStream_t stream);
void sxg_repeat_launch_stats(const RepeatArgs& A, hipStream_t stream);
int sxg_repeat_occupancy(int* count_waves_per_cu);

#ifdef SXG_REPEAT_IMPL
__global__ __launch_bounds__(SXG_REPEAT_WAVE) void repeat_count_kernel(const RepeatArgs A) {
    const int lane = (int)threadIdx.x;
    for (int it = (int)blockIdx.x; it < A.n_items; it += (int)gridDim.x) {
        const int s = __builtin_amdgcn_readfirstlane(A.items[2 * it]), tile = __builtin_amdgcn_readfirstlane(A.items[2 * it + 1]);
        const int64_t o = A.seq_off[s];
        const int32_t n = (int32_t)(A.seq_off[s + 1] - o);
        const int32_t n_lags = (int32_t)sxg_repeat_n_lags(n, A.min_copy, A.max_copy);
        int32_t c[SXG_REPEAT_LANE_LAGS];
        const int m = sxg_repeat_lane_counts(A.bases + o, n, A.min_copy, n_lags, A.stride, tile, lane, c);
        int32_t* out = A.match + (A.match_off[s] - A.match_base) + sxg_repeat_lane_first(tile, lane);
#pragma unroll
        for (int q = 0; q < SXG_REPEAT_LANE_LAGS; ++q)
            if (q < m) out[q] = c[q];
    }
}

__global__ __launch_bounds__(SXG_REPEAT_STATS_THREADS) void repeat_stats_kernel(const RepeatArgs A) {
    const int t = (int)(blockIdx.x * SXG_REPEAT_STATS_THREADS + threadIdx.x);
    if (t >= A.n_work) return;
    const int s = A.work[t];
    const int32_t n = (int32_t)(A.seq_off[s + 1] - A.seq_off[s]);
    const int32_t n_lags = (int32_t)sxg_repeat_n_lags(n, A.min_copy, A.max_copy);
    int32_t best;
    double dev, v;
    sxg_repeat_stats(A.match + (A.match_off[s] - A.match_base), n, A.min_copy, n_lags, A.stride, &best, &dev, &v);
    A.best[s] = best;
    A.dev[s] = dev;
    A.v[s] = v;
}

void sxg_repeat_launch_count(const RepeatArgs& A, int n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(repeat_count_kernel, dim3((unsigned)n_groups), dim3(SXG_REPEAT_WAVE), 0, stream, A);
}
void sxg_repeat_launch_stats(const RepeatArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(repeat_stats_kernel, dim3((unsigned)((A.n_work + SXG_REPEAT_STATS_THREADS - 1) / SXG_REPEAT_STATS_THREADS)),
                       dim3(SXG_REPEAT_STATS_THREADS), 0, stream, A);
}
int sxg_repeat_occupancy(int* count_waves_per_cu) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)repeat_count_kernel, SXG_REPEAT_WAVE, 0);
    if (e != hipSuccess || n < 1) n = 1;
    *count_waves_per_cu = n;
    return 0;
}
#endif  // SXG_REPEAT_IMPL
#endif

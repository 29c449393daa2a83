// poa_letters.hip.h -- the range gather: ranges of the handle's resident path letters, cut out into the back-to-back layout the
// repeat scan (raw bytes) and the sketch of the identity estimate (codes 0..3, 4 = other) read.  DESIGN.md section 5.r.  All index
// arithmetic, the byte moves and the code table are poa_letters.h's, which the CPU checks run.
//
// Included by sxg_poa.hip for the argument struct and the launcher's prototype; kern_letters.hip defines SXG_LETTERS_IMPL.
//
// A work item is a chunk of SXG_LETTERS_CHUNK destination bytes; workgroup g takes chunks g, g + G, g + 2G, ...: no list from the
// host, no counter, no atomic.  The ranges that reach into a chunk are found from the destination prefix sums by two binary
// searches that are uniform over the workgroup; a lane then owns SXG_LETTERS_LANE_GRANULES granules of 16 bytes, 4 KB apart, so
// that the workgroup's stores of a step are one run of 4 KB.  Plain vector loads and stores only.
#ifndef SXG_POA_LETTERS_HIP_H
#define SXG_POA_LETTERS_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "poa_letters.h"

struct LettersGatherArgs {
    const uint8_t* letters;   // the resident letters
    uint8_t* dst;             // [total], 16-byte aligned
    const int64_t* dst_off;   // [n + 1] prefix sums of the range lengths
    const int64_t* src;       // [n] where range r starts in `letters`
    int64_t n, total;
};

void sxg_letters_launch_gather(const LettersGatherArgs& A, int coded, int n_groups, hipStream_t stream);

#ifdef SXG_LETTERS_IMPL
template <int CODED>
__global__ __launch_bounds__(SXG_LETTERS_THREADS) void range_gather_kernel(const LettersGatherArgs A) {
    const int lane = (int)threadIdx.x;
    const int64_t n_chunks = sxg_letters_n_chunks(A.total);
    for (int64_t c = (int64_t)blockIdx.x; c < n_chunks; c += (int64_t)gridDim.x) {
        const int64_t cb = c * SXG_LETTERS_CHUNK, ce = cb + SXG_LETTERS_CHUNK < A.total ? cb + SXG_LETTERS_CHUNK : A.total;
        const int64_t r0 = sxg_letters_find(A.dst_off, 0, A.n - 1, cb), r1 = sxg_letters_find(A.dst_off, r0, A.n - 1, ce - 1);
#pragma unroll
        for (int j = 0; j < SXG_LETTERS_LANE_GRANULES; ++j) {
            const int64_t p = sxg_letters_granule_pos(c, j, lane);
            if (p < ce) sxg_letters_granule<CODED>(A.letters, A.dst, A.dst_off, A.src, r0, r1, p, A.total);
        }
    }
}

void sxg_letters_launch_gather(const LettersGatherArgs& A, int coded, int n_groups, hipStream_t stream) {
    if (coded) hipLaunchKernelGGL(range_gather_kernel<1>, dim3((unsigned)n_groups), dim3(SXG_LETTERS_THREADS), 0, stream, A);
    else hipLaunchKernelGGL(range_gather_kernel<0>, dim3((unsigned)n_groups), dim3(SXG_LETTERS_THREADS), 0, stream, A);
}
#endif  // SXG_LETTERS_IMPL
#endif

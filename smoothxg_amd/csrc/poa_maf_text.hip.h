// poa_maf_text.hip.h -- the MAF text gather: the text of unmerged MAF blocks laid out on the device from literal bytes the host
// formatted and the rows of the resident trimmed MSA (forward, or reversed and complemented), and the letter count of those
// rows.  DESIGN.md section 5.w.  All index arithmetic, the byte moves and the complement table are poa_maf_text.h's, which the
// CPU checks run.
//
// Included by sxg_poa.hip for the argument structs and the launchers' prototypes; kern_maf.hip defines SXG_MAF_IMPL.
//
// maf_text_kernel: a work item is a chunk of SXG_MAF_CHUNK destination bytes; workgroup g takes chunks g, g + G, g + 2G, ...: no
// list from the host, no counter, no atomic.  The segments that reach into a chunk are found from the destination prefix sums by
// two binary searches that are uniform over the workgroup; a lane then owns SXG_MAF_LANE_GRANULES granules of 16 bytes, 4 KB
// apart, so that the workgroup's stores of a step are one run of 4 KB.  A granule is assembled in registers from every segment
// that overlaps it and stored as one 16-byte vector.  Plain vector loads and stores only.
//
// msa_row_letters_kernel: a wave per row, rows dealt grid-stride; a lane counts aligned 16-byte words of the row, the wave sums.
#ifndef SXG_POA_MAF_TEXT_HIP_H
#define SXG_POA_MAF_TEXT_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#if defined(SXG_MAF_IMPL) && defined(__HIP_DEVICE_COMPILE__)
#define SXG_MAF_BSWAP32(w) __builtin_amdgcn_perm(0u, (w), 0x00010203u)   /* v_perm_b32: byte i of the result = byte 3 - i of w */
#endif
#include "poa_maf_text.h"

struct MafTextArgs {
    const uint8_t* literal;   // the uploaded literal blob
    const uint8_t* rows;      // the resident trimmed MSA
    uint8_t* dst;             // [total rounded up to 16], 16-byte aligned
    const int64_t* dst_off;   // [n + 1] prefix sums of the segment lengths
    const int64_t* srck;      // [n] (start in the source) * 4 + kind
    int64_t n, total;
};
struct MafLettersArgs {
    const uint8_t* rows;        // the resident trimmed MSA
    const int64_t* row_begin;   // [n_rows + 1] row r is rows[row_begin[r] .. row_begin[r + 1])
    int32_t* letters;           // [n_rows]
    int64_t n_rows;
};

void sxg_maf_launch_text(const MafTextArgs& A, int n_groups, hipStream_t stream);
void sxg_maf_launch_letters(const MafLettersArgs& A, int n_groups, hipStream_t stream);

#ifdef SXG_MAF_IMPL
__global__ __launch_bounds__(SXG_MAF_THREADS) void maf_text_kernel(const MafTextArgs A) {
    const int lane = (int)threadIdx.x;
    const int64_t n_chunks = sxg_maf_n_chunks(A.total);
    for (int64_t c = (int64_t)blockIdx.x; c < n_chunks; c += (int64_t)gridDim.x) {
        const int64_t cb = c * SXG_MAF_CHUNK, ce = cb + SXG_MAF_CHUNK < A.total ? cb + SXG_MAF_CHUNK : A.total;
        const int64_t s0 = sxg_maf_find(A.dst_off, 0, A.n - 1, cb), s1 = sxg_maf_find(A.dst_off, s0, A.n - 1, ce - 1);
#pragma unroll
        for (int j = 0; j < SXG_MAF_LANE_GRANULES; ++j) {
            const int64_t p = sxg_maf_granule_pos(c, j, lane);
            if (p < ce) sxg_maf_granule(A.literal, A.rows, A.dst, A.dst_off, A.srck, s0, s1, p, A.total);
        }
    }
}

__global__ __launch_bounds__(SXG_MAF_THREADS) void msa_row_letters_kernel(const MafLettersArgs A) {
    const int lane = (int)(threadIdx.x & 63), waves = SXG_MAF_THREADS / 64;
    for (int64_t r = (int64_t)blockIdx.x * waves + (int)(threadIdx.x >> 6); r < A.n_rows; r += (int64_t)gridDim.x * waves) {
        const int64_t begin = A.row_begin[r];
        int32_t n = sxg_maf_row_letters(A.rows, begin, A.row_begin[r + 1] - begin, lane, 64);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) n += __shfl_xor(n, d, 64);
        if (lane == 0) A.letters[r] = n;
    }
}

void sxg_maf_launch_text(const MafTextArgs& A, int n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(maf_text_kernel, dim3((unsigned)n_groups), dim3(SXG_MAF_THREADS), 0, stream, A);
}
void sxg_maf_launch_letters(const MafLettersArgs& A, int n_groups, hipStream_t stream) {
    hipLaunchKernelGGL(msa_row_letters_kernel, dim3((unsigned)n_groups), dim3(SXG_MAF_THREADS), 0, stream, A);
}
#endif  // SXG_MAF_IMPL
#endif

// poa_identity.hip.h -- the identity estimate of the adaptive scores (-a; A14, src/smooth.cpp:1972-2069) on the device, decree Q
// of DESIGN.md section 9: for every block the Jaccard index of ALL pairs of its sequences' canonical k-mer sets and the pair at
// the percentile's rank, in integers only (no log, no float: the host library turns the one (inter, uni) a block returns into
// its threshold).
//
// Included by sxg_poa.hip for the argument structs and the launchers' prototypes; kern_split.hip defines SXG_SPLIT_IMPL and
// includes this file AFTER poa_mash.hip.h: the sets are mash_sketch_kernel's (M1 = Q1), the intersection is set_intersect.
//
// The pairs (one wavefront per pair, taken from a queue).  The sequences the device sees are the ones that take part, block
// after block, so block b's pairs are (i, j), i < j, over its blk_off[b + 1] - blk_off[b] sequences.  A flat pair index p of a
// round finds its block by a binary search in the prefix sums pair_off, its row i by a binary search over the row starts
// i (2n - i - 1) / 2, and writes ONE word, key << 16 | uni (poa_identity_key.h), to words[p]: neighbours in the queue share
// row i's set, which stays in cache.
//
// The select (one workgroup of 256 threads per block).  The idx-th smallest of the block's P words by a radix select, most
// significant digit first: seven passes of 8 bits over the 49-bit words, each a histogram of the words that match the digits
// found so far (LDS atomics), a prefix sum over the 256 bins, and the bin the rank falls into.  The result is a VALUE, so it is
// the same whatever order the adds arrive in.  P words are read seven times; nothing is sorted or moved.
#ifndef SXG_POA_IDENTITY_HIP_H
#define SXG_POA_IDENTITY_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "poa_identity_key.h"

#define SXG_IDENT_SELECT_THREADS 256
#define SXG_IDENT_DIGIT_BITS 8

struct IdentityPairArgs {
    const int32_t* blk_off;    // [n_blocks + 1] the taking-part sequences of every block
    const int64_t* seq_off;    // [n_seqs + 1]
    const unsigned long long* sets;
    const int32_t* set_size;   // [n_seqs]
    const int64_t* pair_off;   // [n_blocks + 1] prefix sums of n (n - 1) / 2
    int32_t b0, b1;            // the blocks of this round
    int32_t n_pairs;           // pair_off[b1] - pair_off[b0]
    int32_t* queue;            // [1]
    unsigned long long* words; // [n_pairs] of this round
};

struct IdentitySelectArgs {
    const int64_t* pair_off;
    const int64_t* idx;        // [n_blocks] Q3's rank (host, double)
    int32_t b0;                // block of workgroup 0
    const unsigned long long* words;   // of this round: block b's at words + pair_off[b] - pair_off[b0]
    int32_t* inter;            // [n_blocks]
    int32_t* uni;              // [n_blocks]
};

void sxg_identity_launch_pairs(const IdentityPairArgs& A, int n_slots, hipStream_t stream);
void sxg_identity_launch_select(const IdentitySelectArgs& A, int n_blocks, hipStream_t stream);
int sxg_identity_occupancy(int* pair_waves_per_cu);

#ifdef SXG_SPLIT_IMPL
__global__ __launch_bounds__(64) void identity_pairs_kernel(const IdentityPairArgs A) {
    using namespace sxg_split;
    const int lane = (int)threadIdx.x;
    __shared__ int s_work;
    const int64_t base = A.pair_off[A.b0];
    for (;;) {
        const int p = pop(A.queue, lane, &s_work);
        if (p >= A.n_pairs) break;
        const int64_t gp = base + p;
        int lo = A.b0, hi = A.b1 - 1;              // the last block with pair_off[b] <= gp (blocks without pairs are passed over)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (A.pair_off[mid] <= gp) lo = mid; else hi = mid - 1;
        }
        const int blk = uniform(lo);
        const int s0 = uniform(A.blk_off[blk]), n = uniform(A.blk_off[blk + 1]) - s0;
        const int64_t q = gp - A.pair_off[blk];
        int ilo = 0, ihi = n - 2;                  // the last row that starts at or before q
        while (ilo < ihi) {
            const int mid = (ilo + ihi + 1) >> 1;
            if (sxg_identity_row_start(mid, n) <= q) ilo = mid; else ihi = mid - 1;
        }
        const int i = uniform(ilo), j = uniform(i + 1 + (int)(q - sxg_identity_row_start(ilo, n)));
        const int ki = uniform(A.set_size[s0 + i]), kj = uniform(A.set_size[s0 + j]);
        const int inter = sxg_mash::set_intersect(A.sets + A.seq_off[s0 + i], ki, A.sets + A.seq_off[s0 + j], kj, lane);
        if (lane == 0) A.words[p] = sxg_identity_word((uint32_t)inter, (uint32_t)(ki + kj - inter));
    }
}

__global__ __launch_bounds__(SXG_IDENT_SELECT_THREADS) void identity_select_kernel(const IdentitySelectArgs A) {
    constexpr int T = SXG_IDENT_SELECT_THREADS, BITS = SXG_IDENT_DIGIT_BITS, BINS = 1 << BITS;
    static_assert(BINS == T, "one bin per thread in the prefix sum");
    static_assert(SXG_IDENT_WORD_BITS <= 7 * BITS, "seven passes cover a word");
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int blk = A.b0 + (int)blockIdx.x;
    const int64_t P = A.pair_off[blk + 1] - A.pair_off[blk];
    if (P <= 0) return;                            // n_used <= 1: the host's zeros stay
    const unsigned long long* w = A.words + (A.pair_off[blk] - A.pair_off[A.b0]);
    __shared__ unsigned int s_hist[BINS];
    __shared__ unsigned int s_wsum[T / 64];
    __shared__ unsigned int s_digit, s_rank;
    unsigned long long prefix = 0;                 // the digits found so far, in place
    unsigned int rank = (unsigned int)A.idx[blk];  // the rank among the words that share them
    for (int shift = 6 * BITS; shift >= 0; shift -= BITS) {
        s_hist[tid] = 0;
        __syncthreads();
        const unsigned long long above = ~0ull << (shift + BITS);   // (shift + BITS <= 56)
        for (int64_t q = tid; q < P; q += T) {
            const unsigned long long v = w[q];
            if ((v & above) == prefix) atomicAdd(&s_hist[(unsigned int)(v >> shift) & (BINS - 1)], 1u);
        }
        __syncthreads();
        // inclusive prefix sum over the bins: inside every wave, then over the waves
        const unsigned int mine = s_hist[tid];
        unsigned int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        for (int k = 0; k < wave; ++k) incl += s_wsum[k];
        if (rank < incl && rank >= incl - mine) { s_digit = (unsigned int)tid; s_rank = rank - (incl - mine); }   // exactly one bin
        __syncthreads();
        prefix |= (unsigned long long)s_digit << shift;
        rank = s_rank;
    }
    if (tid == 0) {
        uint32_t inter, uni;
        sxg_identity_counts(prefix, &inter, &uni);
        A.inter[blk] = (int32_t)inter;
        A.uni[blk] = (int32_t)uni;
    }
}

void sxg_identity_launch_pairs(const IdentityPairArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(identity_pairs_kernel, dim3((unsigned)n_slots), dim3(64), 0, stream, A);
}
void sxg_identity_launch_select(const IdentitySelectArgs& A, int n_blocks, hipStream_t stream) {
    hipLaunchKernelGGL(identity_select_kernel, dim3((unsigned)n_blocks), dim3(SXG_IDENT_SELECT_THREADS), 0, stream, A);
}
int sxg_identity_occupancy(int* pair_waves_per_cu) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)identity_pairs_kernel, 64, 0);
    if (e != hipSuccess || n < 1) n = 1;
    *pair_waves_per_cu = n;
    return 0;
}
#endif  // SXG_SPLIT_IMPL
#endif

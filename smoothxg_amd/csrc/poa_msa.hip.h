// poa_msa.hip.h -- the trimmed MSA of every block on the device (sxg_poa_batch_in::want_msa == SXG_MSA_TRIMMED): the rows that
// src/smooth.cpp:782-847 leaves for the MAF -- padding blanked at both ends of every row, all-gap columns cut off in front and
// behind --, written straight from the arrays the alignments left in HBM.  Nothing per base goes to the host but the rows.
//
// Included by sxg_poa.hip for the argument structs and the launchers' prototypes; kern_msa.hip defines SXG_MSA_IMPL.
//
// Columns (msa_cols_kernel, one workgroup per block, blocks taken from a queue, largest first).  The ranks of a block's nodes are
// a permutation of 0..n-1: the groups are scattered into rank order (tmp[rank[v]] = group[v]), a head flag marks rank 0 and every
// change of group (decree S8), and ONE running workgroup scan over the ranks -- 4 per thread and step, the carry in a register,
// the group in front of a step in LDS because the scan overwrites tmp in place -- turns the flags into columns; col[v] =
// tmp[rank[v]] then lies in a compact node layout (block b's nodes from node_o[b] on, sized from the node counts).  Columns rise strictly along a sequence and along the consensus, so the
// kept columns [b0, e0) of the block are the least column of any row's first kept letter and one past the greatest column of
// any row's last kept letter: two reads per row, LDS atomics.
//
// Rows (msa_rows_kernel, one workgroup per work item, grid-stride over a flat list).  An item is (block, row, chunk of
// SXG_MSA_CHUNK kept letters); it owns the columns from its first letter's column to the next chunk's first column
// (poa_msa_cols.h: sxg_msa_span), i.e. one contiguous run of bytes of the result.  The workgroup keeps its letters and their byte
// positions in registers (8 per thread, read coalesced), then walks the run in windows of SXG_MSA_TILE bytes that start on a
// 16-byte boundary OF THE RESULT: fill the window with '-' in LDS (one 16-byte group per thread), drop the letters that fall
// into it (byte writes to LDS), and store it -- whole groups as 16-byte vectors, the bytes in front of the run's first boundary
// and behind its last one by one (sxg_msa_split16): rows start at any byte, and the groups at a run's ends belong in part to
// the neighbouring run.  No byte store reaches HBM except those at most 30 per item.
#ifndef SXG_POA_MSA_HIP_H
#define SXG_POA_MSA_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "poa_msa_cols.h"

#define SXG_MSA_THREADS 256
#define SXG_MSA_SCAN_ITEMS 4

struct MsaColsArgs {
    const int32_t* blk_off; const int64_t* seq_off;
    const int32_t* paths;      // [n_bases] node of every base
    const int32_t* cons;       // consensus nodes, worst-case layout (NULL: no consensus row)
    const int32_t *node_rank, *node_group;   // worst-case layout
    const int32_t *nn, *nc;    // [n_blocks] nodes / consensus nodes
    const int32_t* trim;       // [n_blocks]
    const int32_t* work; int32_t n_work; int32_t* queue;
    const int64_t* node_o;     // [n_blocks + 1] where block b's nodes lie in tmp and col (prefix sums of the node counts)
    int32_t* tmp;              // [nodes] scratch
    int32_t* col;              // [nodes] out: column of every node
    int32_t* be;               // [2 * n_blocks] out: b0, e0 (both 0: nothing is kept)
};

struct MsaItem { int32_t blk, row, chunk, pad; };

struct MsaRowsArgs {
    const int32_t* blk_off; const int64_t* seq_off;
    const int32_t* paths; const int32_t* cons; const uint8_t* node_code;
    const int32_t *nn, *nc; const int32_t* trim;
    const int32_t* col; const int64_t* node_o; const int32_t* be;
    const int64_t* msa_off;    // [n_blocks + 1]
    const MsaItem* items; int64_t n_items;
    char* msa; int64_t msa_bytes;   // 16-byte aligned
};

void sxg_msa_launch_cols(const MsaColsArgs& A, int n_slots, hipStream_t stream);
void sxg_msa_launch_rows(const MsaRowsArgs& A, int n_slots, hipStream_t stream);

#ifdef SXG_MSA_IMPL
static_assert(SXG_MSA_TILE == 16 * SXG_MSA_THREADS, "one 16-byte group of the window per thread");
static_assert(SXG_MSA_CHUNK % SXG_MSA_THREADS == 0, "a chunk's letters are dealt evenly");

__global__ __launch_bounds__(SXG_MSA_THREADS) void msa_cols_kernel(const MsaColsArgs A) {
    constexpr int T = SXG_MSA_THREADS, IT = SXG_MSA_SCAN_ITEMS;
    __shared__ int s_work, s_wsum[T / 64], s_total, s_last, s_min, s_max;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    for (;;) {
        __syncthreads();
        if (t == 0) s_work = atomicAdd(A.queue, 1);
        __syncthreads();
        const int wi = s_work;
        if (wi >= A.n_work) break;
        const int b = A.work[wi];
        const int s0 = A.blk_off[b], s1 = A.blk_off[b + 1];
        const int64_t base0 = A.seq_off[s0];
        const int n = A.nn[b];
        const int32_t* rank = A.node_rank + base0;
        const int32_t* grp = A.node_group + base0;
        int32_t* tmp = A.tmp + A.node_o[b];
        int32_t* col = A.col + A.node_o[b];
        for (int v = t; v < n; v += T) {
            const int r = rank[v];
            if ((unsigned)r < (unsigned)n) tmp[r] = grp[v];
        }
        if (t == 0) { s_min = 0x7fffffff; s_max = -1; s_last = 0; }
        __syncthreads();
        int carry = 0;   // heads in front of this step
        for (int r0 = 0; r0 < n; r0 += T * IT) {
            const int r = r0 + t * IT;
            int g[IT + 1];
            g[0] = r == 0 || r >= n ? 0 : (t == 0 ? s_last : tmp[r - 1]);
#pragma unroll
            for (int i = 0; i < IT; ++i) g[i + 1] = r + i < n ? tmp[r + i] : 0;
            int f[IT], mine = 0;
#pragma unroll
            for (int i = 0; i < IT; ++i) { f[i] = r + i < n ? sxg_msa_head(r + i, g[i], g[i + 1]) : 0; mine += f[i]; }
            int incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(incl, d, 64);
                if (lane >= d) incl += up;
            }
            if (lane == 63) s_wsum[wave] = incl;
            __syncthreads();   // (every read of tmp of this step is done)
            for (int k = 0; k < wave; ++k) incl += s_wsum[k];
            int run = carry + incl - mine;
#pragma unroll
            for (int i = 0; i < IT; ++i) { run += f[i]; if (r + i < n) tmp[r + i] = run - 1; }
            if (t == T - 1) { s_total = incl; s_last = g[IT]; }
            __syncthreads();
            carry += s_total;
        }
        for (int v = t; v < n; v += T) {
            const int r = rank[v];
            col[v] = (unsigned)r < (unsigned)n ? tmp[r] : 0;
        }
        __syncthreads();
        const int rows = (s1 - s0) + (A.cons ? 1 : 0);
        const int64_t trim = A.trim ? A.trim[b] : 0;
        for (int row = t; row < rows; row += T) {
            const bool is_cons = row == s1 - s0;
            const int32_t* nodes = is_cons ? A.cons + base0 : A.paths + A.seq_off[s0 + row];
            const int64_t len = is_cons ? A.nc[b] : A.seq_off[s0 + row + 1] - A.seq_off[s0 + row];
            int64_t k0, k1;
            sxg_msa_kept(len, trim, &k0, &k1);
            if (k1 <= k0) continue;
            const int va = nodes[k0], vz = nodes[k1 - 1];
            if ((unsigned)va >= (unsigned)n || (unsigned)vz >= (unsigned)n) continue;
            atomicMin(&s_min, col[va]);
            atomicMax(&s_max, col[vz]);
        }
        __syncthreads();
        if (t == 0) {
            const bool any = s_max >= 0 && s_min <= s_max;
            A.be[2 * b] = any ? s_min : 0;
            A.be[2 * b + 1] = any ? s_max + 1 : 0;
        }
    }
}

__global__ __launch_bounds__(SXG_MSA_THREADS) void msa_rows_kernel(const MsaRowsArgs A) {
    constexpr int T = SXG_MSA_THREADS, PER = SXG_MSA_CHUNK / SXG_MSA_THREADS;
    __shared__ uint4 s_tile[SXG_MSA_TILE / 16];
    unsigned char* tile = (unsigned char*)s_tile;
    const int t = (int)threadIdx.x;
    const unsigned G4 = SXG_MSA_GAP * 0x01010101u;
    for (int64_t it = blockIdx.x; it < A.n_items; it += gridDim.x) {
        const MsaItem I = A.items[it];
        const int b = I.blk, row = I.row;
        const int s0 = A.blk_off[b], s1 = A.blk_off[b + 1];
        const int64_t base0 = A.seq_off[s0];
        const int n = A.nn[b];
        const bool is_cons = row == s1 - s0;
        const int32_t* nodes = is_cons ? A.cons + base0 : A.paths + A.seq_off[s0 + row];
        const int64_t len = is_cons ? A.nc[b] : A.seq_off[s0 + row + 1] - A.seq_off[s0 + row];
        const int32_t* col = A.col + A.node_o[b];
        const uint8_t* code = A.node_code + base0;
        int64_t k0, k1, a, z;
        sxg_msa_kept(len, A.trim ? A.trim[b] : 0, &k0, &k1);
        sxg_msa_chunk_letters(k0, k1, I.chunk, SXG_MSA_CHUNK, &a, &z);
        const int b0 = A.be[2 * b], e0 = A.be[2 * b + 1];
        const int64_t cols = (int64_t)e0 - b0;
        if (cols <= 0) continue;   // (uniform over the workgroup)
        int col_a = 0, col_z = 0;
        if (a > k0 && a < k1) { const int v = nodes[a]; col_a = (unsigned)v < (unsigned)n ? col[v] : b0; }
        if (z < k1) { const int v = nodes[z]; col_z = (unsigned)v < (unsigned)n ? col[v] : e0; }
        int32_t sp, ep;
        sxg_msa_span(k0, k1, a, z, b0, e0, col_a, col_z, &sp, &ep);
        const int64_t nbytes = (int64_t)ep - sp;
        const int64_t dst = A.msa_off[b] + (int64_t)row * cols + (sp - b0);
        if (sp < b0 || ep > e0 || nbytes <= 0 || dst < 0 || dst + nbytes > A.msa_bytes) continue;   // (never on a consistent batch)
        // this thread's letters: byte position inside the run, -1 = none; positions rise with j, [pmin, pmax] holds them all
        int pmin = 0x7fffffff, pmax = -1;
        int pos[PER];
        unsigned char ch[PER];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int64_t k = a + t + (int64_t)j * T;
            pos[j] = -1; ch[j] = SXG_MSA_GAP;
            if (k < z) {
                const int v = nodes[k];
                if ((unsigned)v < (unsigned)n) {
                    const int64_t p = (int64_t)col[v] - sp;
                    if (p >= 0 && p < nbytes) {
                        pos[j] = (int)p;
                        pmin = pmin < (int)p ? pmin : (int)p; pmax = pmax > (int)p ? pmax : (int)p;
                        const unsigned c = code[v] > 4 ? 4u : code[v];
                        ch[j] = (unsigned char)((0x4e54474341ull >> (8 * c)) & 0xff);   // "ACGTN"
                    }
                }
            }
        }
        int64_t head, body, tail;
        sxg_msa_split16((uint64_t)dst, nbytes, &head, &body, &tail);
        const int64_t body0 = dst + head, body1 = body0 + body, end = dst + nbytes;
        for (int64_t w = dst & ~(int64_t)15; w < end; w += SXG_MSA_TILE) {
            __syncthreads();   // (the window of the step before is stored)
            s_tile[t] = uint4{G4, G4, G4, G4};
            __syncthreads();
            if (pmax >= 0 && dst + pmax >= w && dst + pmin < w + SXG_MSA_TILE) {   // (a window none of this thread's letters falls into costs one test)
#pragma unroll
                for (int j = 0; j < PER; ++j) {
                    const int64_t o = dst + pos[j] - w;
                    if (pos[j] >= 0 && o >= 0 && o < SXG_MSA_TILE) tile[o] = ch[j];
                }
            }
            __syncthreads();
            const int64_t gs = w + 16 * (int64_t)t, ge = gs + 16;
            if (gs >= body0 && ge <= body1) *(uint4*)(A.msa + gs) = s_tile[t];
            else {
                const int64_t lo = gs > dst ? gs : dst, hi = ge < end ? ge : end;
                for (int64_t x = lo; x < hi; ++x) A.msa[x] = (char)tile[x - w];   // (head and tail of the run only)
            }
        }
    }
}

void sxg_msa_launch_cols(const MsaColsArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(msa_cols_kernel, dim3((unsigned)n_slots), dim3(SXG_MSA_THREADS), 0, stream, A);
}
void sxg_msa_launch_rows(const MsaRowsArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(msa_rows_kernel, dim3((unsigned)n_slots), dim3(SXG_MSA_THREADS), 0, stream, A);
}
#endif  // SXG_MSA_IMPL
#endif

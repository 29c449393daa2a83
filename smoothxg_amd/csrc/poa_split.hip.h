// poa_split.hip.h -- the identity split of break_blocks (src/breaks.cpp:335-586) on the device, decrees P1-P4 of DESIGN.md
// section 9: the gap-compressed identity of a pair of sequences as the lexicographically smallest (penalty, cols, nonmatch)
// over all global alignments, and the greedy clustering loop that calls it.
//
// Included by sxg_poa.hip for the argument structs and the launchers' prototypes; kern_split.hip defines SXG_SPLIT_IMPL and
// holds the kernels and the launchers (a translation unit of its own, so that the kernel classes of kern_part.hip are not
// recompiled -- or reshuffled by the optimiser -- when this file changes).
//
// The sweep (one wavefront per pair).  Rows run over a, columns over b.  A column PANEL is 64 * SPLIT_W columns; lane l owns
// SPLIT_W consecutive columns of it and keeps the three states of each (last column diagonal M / consumed a: I / consumed
// b: D) of the previous row in registers: 3 * SPLIT_W 64-bit keys.  The rows of a panel run top to bottom; the panel's right
// boundary column (three keys per row) goes to a slot-private buffer in HBM that the next panel reads 64 rows at a time,
// so any length runs with the same registers.  One key = penalty << 40 | cols << 20 | nonmatch: the steps of P1 are key
// additions (no field carries into the next at lengths <= SXG_POA_MAX_SEQ_LEN: penalty < 2^24, cols and nonmatch < 2^20) and
// the minimum of keys is the lexicographic minimum.  M and I of a row depend on the previous row only; the in-row state is
// T[j] = min(T[j-1] + ext, open[j]) (T[j] = D[j+1]), a min-plus prefix problem solved as the packed sweep solves its own:
// every lane folds its columns, one biased inclusive min-scan over the wave on the DPP path, every lane replays its columns.
#ifndef SXG_POA_SPLIT_HIP_H
#define SXG_POA_SPLIT_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SXG_SPLIT_W 8                        /* columns per lane */
#define SXG_SPLIT_PANEL (64 * SXG_SPLIT_W)   /* columns per panel */
#define SXG_SPLIT_WAVES_PER_CU 8             /* resident wavefronts (= slots) per CU the launches ask for */

typedef unsigned long long sxg_key_t;

struct SplitPairArgs {
    const int64_t* seq_off;   // [n_seqs + 1]
    const uint8_t* bases;     // codes 0..4
    const int32_t* pair_a;    // [n_pairs] rows
    const int32_t* pair_b;    // [n_pairs] columns
    const uint8_t* b_rev;     // [n_pairs] 1 = b is read reverse-complemented
    const int32_t* cap;       // [n_pairs]
    const int32_t* work;      // [n_work] pair indices, most expensive first
    int32_t n_work;
    int32_t* queue;           // [1] next entry of work
    sxg_key_t* bound;         // [n_slots * 3 * bound_rows] right boundary columns
    int64_t bound_rows;       // rows per slot (longest a + 1)
    int32_t* penalty;         // [n_pairs]
    int32_t* cols;            // [n_pairs] 0 = penalty >= cap (P2)
    int32_t* matches;         // [n_pairs]
};

struct SplitBlockArgs {
    const int32_t* blk_off;   // [n_blocks + 1]
    const int64_t* seq_off;   // [n_seqs + 1]
    const uint8_t* bases;
    const double* identity;   // [n_blocks] block_group_identity, in (0, 1]
    const double* ratio_min;  // [n_blocks] length_ratio_min
    const int32_t* work;      // [n_work] block indices, most expensive first
    int32_t n_work;
    int32_t* queue;
    sxg_key_t* bound;         // [n_slots * 3 * bound_rows]
    int64_t bound_rows;
    int32_t* lists;           // [n_slots * 2 * list_cap] per slot: last member of every group, previous member of every sequence
    int64_t list_cap;         // sequences of the deepest block
    int32_t* group;           // [n_seqs] group of every sequence
    int32_t* n_groups;        // [n_blocks]
    int64_t* n_pairs;         // [n_blocks] pair sweeps run
    uint64_t* cells;          // [n_blocks] cells of those sweeps
};

void sxg_split_launch_pairs(const SplitPairArgs& A, int n_slots, hipStream_t stream);
void sxg_split_launch_blocks(const SplitBlockArgs& A, int n_slots, hipStream_t stream);
int sxg_split_occupancy(int which, int* waves_per_cu);   // which: 0 = pair_identity_kernel, 1 = split_kernel

#ifdef SXG_SPLIT_IMPL
#define SPLIT_GLOBAL __attribute__((address_space(1)))

namespace sxg_split {

constexpr int W = SXG_SPLIT_W;
constexpr int SH_P = 40, SH_C = 20;
constexpr sxg_key_t K_MATCH = 1ull << SH_C;                                   // (0, 1, 0)
constexpr sxg_key_t K_MISMATCH = (7ull << SH_P) | (1ull << SH_C) | 1ull;       // (7, 1, 1)
constexpr sxg_key_t K_OPEN_NEW = (12ull << SH_P) | (1ull << SH_C) | 1ull;      // (12, 1, 1): after a diagonal column / at the start
constexpr sxg_key_t K_OPEN_SWITCH = 12ull << SH_P;                             // (12, 0, 0): after a gap of the other kind
constexpr sxg_key_t K_EXT = 1ull << SH_P;                                      // (1, 0, 0)
constexpr sxg_key_t K_INF = 1ull << 61;   // rows * (largest step) < 2^59: sums of it never wrap

__device__ __forceinline__ sxg_key_t kmin(const sxg_key_t a, const sxg_key_t b) { return a < b ? a : b; }
__device__ __forceinline__ sxg_key_t kmin3(const sxg_key_t a, const sxg_key_t b, const sxg_key_t c) { return kmin(kmin(a, b), c); }

// a 64-bit key moved on the DPP path as its two halves; lanes without a source keep `old`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ sxg_key_t dpp_mov(const sxg_key_t old, const sxg_key_t v) {
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)old, (int)(unsigned)v, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(old >> 32), (int)(unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((sxg_key_t)(unsigned)hi << 32) | (unsigned)lo;
}
__device__ __forceinline__ sxg_key_t wave_incl_min(sxg_key_t v) {
    v = kmin(v, dpp_mov<0x111, 0xf>(~0ull, v));  // row_shr:1
    v = kmin(v, dpp_mov<0x112, 0xf>(~0ull, v));  // row_shr:2
    v = kmin(v, dpp_mov<0x114, 0xf>(~0ull, v));  // row_shr:4
    v = kmin(v, dpp_mov<0x118, 0xf>(~0ull, v));  // row_shr:8
    v = kmin(v, dpp_mov<0x142, 0xa>(~0ull, v));  // row_bcast:15 into rows 1 and 3
    v = kmin(v, dpp_mov<0x143, 0xc>(~0ull, v));  // row_bcast:31 into rows 2 and 3
    return v;
}
// lane l receives v of lane l-1; lane 0 receives `first`
__device__ __forceinline__ sxg_key_t wave_shr1(const sxg_key_t v, const sxg_key_t first) { return dpp_mov<0x138, 0xf>(first, v); }
__device__ __forceinline__ sxg_key_t read_lane(const sxg_key_t v, const int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), lane);
    return ((sxg_key_t)hi << 32) | lo;
}
__device__ __forceinline__ int uniform(const int v) { return __builtin_amdgcn_readfirstlane(v); }

// The optimal key of a (rows, la >= 1) against b (columns, lb >= 1; brev: read reverse-complemented), the same value in every
// lane.  bound: this slot's 3 * (la + 1) boundary keys.  Every lane of the wave calls it with the same arguments.
__device__ __forceinline__ sxg_key_t pair_sweep(const SPLIT_GLOBAL uint8_t* a, const int la, const SPLIT_GLOBAL uint8_t* b, const int lb,
                                                const int brev, SPLIT_GLOBAL sxg_key_t* bound, const int lane) {
    const int n_panels = (lb + SXG_SPLIT_PANEL - 1) / SXG_SPLIT_PANEL;
    sxg_key_t result = K_INF;
    for (int p = 0; p < n_panels; ++p) {
        const int base = p * SXG_SPLIT_PANEL;          // columns base + 1 .. base + PANEL (1-based) belong to this panel
        const int first = base + lane * W;             // this lane's columns are first + 1 .. first + W
        const bool last_panel = p == n_panels - 1;
        if (p > 0) __syncthreads();   // (one wave per workgroup: lane 63's boundary column is visible to the lanes that load it)
        int bc[W];
        sxg_key_t M[W], I[W], D[W];
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const int j = first + c + 1;
            int code = 255;                            // a column past the end of b matches nothing; nobody reads its cells
            if (j <= lb) {
                const int raw = (int)b[brev ? lb - j : j - 1];
                code = brev ? (raw < 4 ? 3 - raw : raw) : raw;
            }
            bc[c] = code;
            M[c] = K_INF;
            I[c] = K_INF;
            D[c] = K_OPEN_NEW + (sxg_key_t)(j - 1) * K_EXT;    // row 0: one gap from the start
        }
        if (!last_panel && lane == 63) { bound[0] = M[W - 1]; bound[1] = I[W - 1]; bound[2] = D[W - 1]; }
        // the column left of the panel at row 0 (panel 0: the corner, M = 0)
        sxg_key_t left_best;                           // min(M, I, D) of the left boundary at the previous row
        if (p == 0) left_best = 0;
        else left_best = K_OPEN_NEW + (sxg_key_t)(base - 1) * K_EXT;
        sxg_key_t last_best = D[W - 1];                // min(M, I, D) of this lane's last column at the previous row
        const sxg_key_t bias = (sxg_key_t)(63 - lane) * W * K_EXT;
        sxg_key_t bM = K_INF, bI = K_INF, bD = K_INF;  // 64 rows of the left boundary, row i0 + lane in lane `lane`
        int av = 4;                                    // 64 letters of a
        for (int i0 = 1; i0 <= la; i0 += 64) {
            const int mine = i0 + lane;
            if (mine <= la) {
                av = (int)a[mine - 1];
                if (p > 0) { bM = bound[3 * (int64_t)mine]; bI = bound[3 * (int64_t)mine + 1]; bD = bound[3 * (int64_t)mine + 2]; }
            }
            const int i1 = min(i0 + 63, la);
            for (int i = i0; i <= i1; ++i) {
                const int r = i - i0;
                const int ai = __builtin_amdgcn_readlane(av, r);
                // the left boundary at row i: column 0 of the matrix (one gap from the start) or what the panel before wrote
                sxg_key_t lM, lI, lD;
                if (p == 0) { lM = K_INF; lI = K_OPEN_NEW + (sxg_key_t)(i - 1) * K_EXT; lD = K_INF; }
                else { lM = read_lane(bM, r); lI = read_lane(bI, r); lD = read_lane(bD, r); }
                const sxg_key_t t_left = kmin(lD + K_EXT, kmin(lM + K_OPEN_NEW, lI + K_OPEN_SWITCH));   // D of column base + 1
                sxg_key_t diag = wave_shr1(last_best, left_best);
                left_best = kmin3(lM, lI, lD);
                sxg_key_t t_loc = K_INF;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const sxg_key_t best = kmin3(M[c], I[c], D[c]);
                    const sxg_key_t nI = kmin3(I[c] + K_EXT, M[c] + K_OPEN_NEW, D[c] + K_OPEN_SWITCH);
                    const sxg_key_t nM = diag + (bc[c] == ai ? K_MATCH : K_MISMATCH);
                    diag = best;
                    M[c] = nM;
                    I[c] = nI;
                    const sxg_key_t opn = kmin(nM + K_OPEN_NEW, nI + K_OPEN_SWITCH);
                    D[c] = opn;                        // (parked here until the replay below)
                    t_loc = kmin(t_loc + K_EXT, opn);
                }
                t_loc = lane == 0 ? kmin(t_loc, t_left + (sxg_key_t)W * K_EXT) : t_loc;
                const sxg_key_t scan = wave_incl_min(t_loc + bias);
                // T of the column left of this lane: the scan of lane - 1 without that lane's bias
                const sxg_key_t t_prev = wave_shr1(scan, 0) - (bias + (sxg_key_t)W * K_EXT);
                sxg_key_t t_in = lane == 0 ? t_left : t_prev;
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const sxg_key_t opn = D[c];
                    D[c] = t_in;
                    t_in = kmin(t_in + K_EXT, opn);
                }
                last_best = kmin3(M[W - 1], I[W - 1], D[W - 1]);
                if (!last_panel && lane == 63) {
                    bound[3 * (int64_t)i] = M[W - 1]; bound[3 * (int64_t)i + 1] = I[W - 1]; bound[3 * (int64_t)i + 2] = D[W - 1];
                }
            }
        }
        if (last_panel) {
            const int col = lb - 1 - base;             // 0-based column of the panel that holds the end of b
            sxg_key_t mine = K_INF;
#pragma unroll
            for (int c = 0; c < W; ++c)
                if (c == col % W) mine = kmin3(M[c], I[c], D[c]);
            result = read_lane(mine, uniform(col / W));
        }
    }
    return result;
}

// Next entry of the queue, the same in every lane: lane 0 takes it and hands it round through LDS, as the POA kernels do.
// (A first form -- readfirstlane of a value only lane 0 had set -- was compiled into a loop that dropped lane 0 and kept the
//  other lanes on entry 0 for ever: the optimiser threads the `lane == 0` branch through the loop.)
__device__ __forceinline__ int pop(int32_t* queue, const int lane, int* s_work) {
    __syncthreads();
    if (lane == 0) *s_work = atomicAdd(queue, 1);
    __syncthreads();
    return uniform(*s_work);
}

}  // namespace sxg_split

// One wavefront per pair, taken from a queue; slot = workgroup.
__global__ __launch_bounds__(64) void pair_identity_kernel(const SplitPairArgs A) {
    using namespace sxg_split;
    const int lane = (int)threadIdx.x;
    __shared__ int s_work;
    SPLIT_GLOBAL sxg_key_t* bound = (SPLIT_GLOBAL sxg_key_t*)(A.bound + (int64_t)blockIdx.x * 3 * A.bound_rows);
    const SPLIT_GLOBAL uint8_t* bases = (const SPLIT_GLOBAL uint8_t*)A.bases;
    for (;;) {
        const int w = pop(A.queue, lane, &s_work);
        if (w >= A.n_work) break;
        const int k = uniform(A.work[w]);
        const int sa = uniform(A.pair_a[k]), sb = uniform(A.pair_b[k]);
        const int64_t oa = A.seq_off[sa], ob = A.seq_off[sb];
        const int la = uniform((int)(A.seq_off[sa + 1] - oa)), lb = uniform((int)(A.seq_off[sb + 1] - ob));
        const sxg_key_t key = pair_sweep(bases + oa, la, bases + ob, lb, uniform((int)A.b_rev[k]), bound, lane);
        const int pen = (int)(key >> SH_P), cols = (int)((key >> SH_C) & 0xfffffu), non = (int)(key & 0xfffffu);
        const bool ok = pen < A.cap[k];                // P2
        if (lane == 0) {
            A.penalty[k] = pen;
            A.cols[k] = ok ? cols : 0;
            A.matches[k] = ok ? cols - non : 0;
        }
    }
}

// One persistent wavefront per block: P3's loops with wave-uniform control, one sweep per pair.
__global__ __launch_bounds__(64) void split_kernel(const SplitBlockArgs A) {
    using namespace sxg_split;
    const int lane = (int)threadIdx.x;
    __shared__ int s_work;
    SPLIT_GLOBAL sxg_key_t* bound = (SPLIT_GLOBAL sxg_key_t*)(A.bound + (int64_t)blockIdx.x * 3 * A.bound_rows);
    int32_t* tail = A.lists + (int64_t)blockIdx.x * 2 * A.list_cap;   // last member of group g (block-local sequence index)
    int32_t* prev = tail + A.list_cap;                                // the member that joined the same group before sequence i; -1
    const SPLIT_GLOBAL uint8_t* bases = (const SPLIT_GLOBAL uint8_t*)A.bases;
    for (;;) {
        const int w = pop(A.queue, lane, &s_work);
        if (w >= A.n_work) break;
        const int blk = uniform(A.work[w]);
        const int s0 = uniform(A.blk_off[blk]), n = uniform(A.blk_off[blk + 1]) - s0;
        const double t = A.identity[blk], ratio_min = A.ratio_min[blk];
        const double one_minus = 1.0 - t;
        const unsigned long long len_thr = one_minus == 0.0 ? ~0ull : (unsigned long long)(t / one_minus);
        int ng = n > 0 ? 1 : 0;
        long long n_pairs = 0;
        unsigned long long cells = 0;
        if (lane == 0 && n > 0) { tail[0] = 0; prev[0] = -1; A.group[s0] = 0; }
        __syncthreads();
        for (int i = 1; i < n; ++i) {
            const int64_t oc = A.seq_off[s0 + i];
            const int curr_len = uniform((int)(A.seq_off[s0 + i + 1] - oc));
            int found = -1;
            for (int rev = 0; rev < 2 && found < 0; ++rev) {
                for (int g = ng - 1; g >= 0 && found < 0; --g) {
                    for (int k = uniform(tail[g]); k >= 0; k = uniform(prev[k])) {
                        const int64_t oo = A.seq_off[s0 + k];
                        const int other_len = uniform((int)(A.seq_off[s0 + k + 1] - oo));
                        if ((double)other_len / (double)curr_len < ratio_min) break;
                        if (other_len < curr_len && (unsigned long long)other_len < len_thr) break;
                        ++n_pairs;
                        cells += (unsigned long long)other_len * (unsigned long long)curr_len;
                        // identity(rc(curr), other) = identity(other, rc(curr)): rows over the member, columns over curr
                        const sxg_key_t key = pair_sweep(bases + oo, other_len, bases + oc, curr_len, rev, bound, lane);
                        const int pen = (int)(key >> SH_P), cols = (int)((key >> SH_C) & 0xfffffu), non = (int)(key & 0xfffffu);
                        if (pen < curr_len && (double)(cols - non) / (double)cols >= t) { found = g; break; }
                    }
                }
            }
            const bool fresh = found < 0;
            found = uniform(fresh ? ng : found);
            ng = uniform(ng + (fresh ? 1 : 0));
            if (lane == 0) {
                prev[i] = fresh ? -1 : tail[found];
                tail[found] = i;
                A.group[s0 + i] = found;
            }
            __syncthreads();   // (one wave per workgroup: orders lane 0's list update before every lane's reads)
        }
        if (lane == 0) { A.n_groups[blk] = ng; A.n_pairs[blk] = n_pairs; A.cells[blk] = cells; }
    }
}

void sxg_split_launch_pairs(const SplitPairArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(pair_identity_kernel, dim3((unsigned)n_slots), dim3(64), 0, stream, A);
}
void sxg_split_launch_blocks(const SplitBlockArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(split_kernel, dim3((unsigned)n_slots), dim3(64), 0, stream, A);
}
int sxg_split_occupancy(int which, int* waves_per_cu) {
    int n = 0;
    const hipError_t e = which == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)pair_identity_kernel, 64, 0)
                                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)split_kernel, 64, 0);
    if (e != hipSuccess || n < 1) n = 1;
    *waves_per_cu = n;
    return 0;
}
#endif  // SXG_SPLIT_IMPL
#endif

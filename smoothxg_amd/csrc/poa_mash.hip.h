// poa_mash.hip.h -- the mash-based branch of the identity split of break_blocks (src/breaks.cpp:388-471) on the device,
// decrees M1-M5 of DESIGN.md section 9: the set of distinct canonical k-mers of every eligible sequence (built, sorted and
// de-duplicated here), the exact size of the intersection of two such sets, and the greedy walk of P3 with M4's rules.
//
// Included by sxg_poa.hip for the argument structs and the launchers' prototypes; kern_split.hip defines SXG_SPLIT_IMPL and
// includes this file AFTER poa_split.hip.h, whose pair_sweep / pop / uniform it calls.
//
// The sketch (one workgroup of 256 threads per sequence, taken from a queue, longest first).  A TILE of SXG_MASH_SORT_TILE
// windows is rolled into LDS (every thread rolls TILE / 256 consecutive windows: forward and reverse-complement codes as
// canonical_kmers of sxg_smooth.cpp rolls them, a window with an N or past the end becomes the key ~0, which no canonical k-mer
// equals: of a k-mer and its reverse complement one is below 2^63), sorted there by a bitonic network, and -- when the sequence
// has more windows than one tile -- written to the slot's scratch in HBM, where sorted runs are merged pairwise, ping to pong,
// every key finding its place by one binary search in the other run.  The sorted keys lose their duplicates by a prefix sum over
// "differs from the key before" and go to sets + seq_off[s] (capacity: the length of the sequence) with their number.
// 8 KB of LDS per workgroup: as many workgroups per CU as its wave slots allow.
//
// The intersection (one wavefront, two sorted sets in HBM): a merge-path partition -- lane l finds by one binary search where
// diagonal l * ceil((|A| + |B|) / 64) cuts the merge of A and B (A first on ties) -- and a sequential merge of every lane's
// stretch, counting the A keys that meet their equal at the head of B; the counts are summed over the wave.
//
// The walk (one persistent wavefront per block, as split_kernel): P3's loops with M4 inside the member loop.  The candidates of
// a walk are evaluated one after the other, in order, so group / n_pairs / n_mash are the sequential walk's by construction.
#ifndef SXG_POA_MASH_HIP_H
#define SXG_POA_MASH_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SXG_MASH_SORT_TILE 1024    /* keys a workgroup sorts in LDS at once */
#define SXG_MASH_THREADS 256

struct MashSketchArgs {
    const int64_t* seq_off;    // [n_seqs + 1]
    const uint8_t* bases;      // codes 0..4
    const int32_t* work;       // [n_work] sequences with at least k bases, longest first
    int32_t n_work;
    int32_t* queue;            // [1]
    int32_t k;                 // 1..32
    unsigned long long* scratch;   // [n_slots * 2 * scratch_keys] ping and pong of every slot
    int64_t scratch_keys;      // windows of the longest sequence rounded up to whole tiles; 0 when one tile holds every sequence
    unsigned long long* sets;  // [seq_off[n_seqs]] the sorted set of sequence s at sets + seq_off[s]
    int32_t* set_size;         // [n_seqs] (sequences that are not in `work` keep what the caller wrote: 0)
};

struct MashPairArgs {
    const int64_t* seq_off;
    const unsigned long long* sets;
    const int32_t* set_size;
    const int32_t* pair_a;     // [n_pairs]
    const int32_t* pair_b;
    int32_t n_pairs;
    int32_t* queue;
    int32_t* inter;            // [n_pairs]
};

struct MashBlockArgs {
    SplitBlockArgs S;          // P3's arguments, as split_kernel takes them
    const int32_t* min_len;    // [n_blocks] 0 = this block runs P3 only
    const double* f;           // [n_blocks] M3: v / (2 - v), v = exp(-(1 - t) k)
    const double* jmin;        // [n_blocks] M3: w / (2 - w), w = exp(-(1 - e) k)
    const unsigned long long* sets;
    const int32_t* set_size;
    int64_t* n_mash;           // [n_blocks] set comparisons run
};

void sxg_mash_launch_sketch(const MashSketchArgs& A, int n_slots, hipStream_t stream);
void sxg_mash_launch_pairs(const MashPairArgs& A, int n_slots, hipStream_t stream);
void sxg_mash_launch_blocks(const MashBlockArgs& A, int n_slots, hipStream_t stream);
int sxg_mash_occupancy(int which, int* groups_per_cu);   // which: 0 = mash_sketch_kernel, 1 = mash_pair_kernel, 2 = split_mash_kernel

#ifdef SXG_SPLIT_IMPL
namespace sxg_mash {

typedef unsigned long long kmer_t;
constexpr int TILE = SXG_MASH_SORT_TILE;
constexpr int THREADS = SXG_MASH_THREADS;
constexpr int PER = TILE / THREADS;            // consecutive windows a thread rolls
constexpr kmer_t NONE = ~0ull;
static_assert(TILE % THREADS == 0 && (TILE & (TILE - 1)) == 0, "tile: a power of two, whole windows per thread");

// |A n B| of two sorted sets of distinct keys, the same value in every lane; every lane of the wave calls it with the same arguments
__device__ __forceinline__ int set_intersect(const kmer_t* a, const int na, const kmer_t* b, const int nb, const int lane) {
    int cnt = 0;
    if (na > 0 && nb > 0) {
        const int total = na + nb, seg = (total + 63) / 64;
        const int d0 = min(lane * seg, total), d1 = min(d0 + seg, total);
        // i keys of A and d0 - i keys of B precede diagonal d0 in the merge (A first on ties): the smallest i with A[i] > B[d0 - i - 1]
        int lo = max(0, d0 - nb), hi = min(d0, na);
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a[mid] <= b[d0 - mid - 1]) lo = mid + 1; else hi = mid;
        }
        int i = lo, j = d0 - lo;
        kmer_t x = i < na ? a[i] : NONE, y = j < nb ? b[j] : NONE;
        for (int step = d0; step < d1 && i < na && j < nb; ++step) {
            if (x <= y) {
                cnt += x == y ? 1 : 0;
                ++i;
                x = i < na ? a[i] : NONE;
            } else {
                ++j;
                y = j < nb ? b[j] : NONE;
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    return sxg_split::uniform(cnt);
}

// keys src[0 .. n) sorted, NONE last: the distinct ones to out, their number returned (the same in every thread)
template <class Src>
__device__ __forceinline__ int write_distinct(const Src src, const int n, kmer_t* out, const int tid, int* s_wsum) {
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += THREADS) {
        const int idx = c0 + tid;
        const kmer_t key = idx < n ? src[idx] : NONE;
        const kmer_t before = idx > 0 && idx < n ? src[idx - 1] : NONE;
        const bool keep = key != NONE && (idx == 0 || key != before);
        const unsigned long long votes = __ballot(keep);
        const int lane = tid & 63, wave = tid >> 6;
        const int rank = __popcll(votes & ((1ull << lane) - 1ull));
        __syncthreads();                       // (the sums of the chunk before have been read)
        if (lane == 0) s_wsum[wave] = __popcll(votes);
        __syncthreads();
        int off = base, all = 0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            const int s = s_wsum[w];
            off += w < wave ? s : 0;
            all += s;
        }
        if (keep) out[off + rank] = key;
        base += all;
    }
    return base;
}

}  // namespace sxg_mash

__global__ __launch_bounds__(SXG_MASH_THREADS) void mash_sketch_kernel(const MashSketchArgs A) {
    using namespace sxg_mash;
    const int tid = (int)threadIdx.x;
    __shared__ kmer_t s_key[TILE];
    __shared__ int s_work;
    __shared__ int s_wsum[THREADS / 64];
    const int k = A.k;
    const kmer_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1ull);
    kmer_t* ping = A.scratch + (int64_t)blockIdx.x * 2 * A.scratch_keys;
    kmer_t* pong = ping + A.scratch_keys;
    for (;;) {
        __syncthreads();
        if (tid == 0) s_work = atomicAdd(A.queue, 1);
        __syncthreads();
        const int w = s_work;
        if (w >= A.n_work) break;
        const int s = A.work[w];
        const int64_t o = A.seq_off[s];
        const int len = (int)(A.seq_off[s + 1] - o);
        const int nk = len - k + 1;                            // windows (the host queues sequences with nk >= 1 only)
        const int n_tiles = (nk + TILE - 1) / TILE;
        const uint8_t* seq = A.bases + o;
        kmer_t* out = A.sets + o;
        int count = 0;
        for (int t = 0; t < n_tiles; ++t) {
            const int in_tile = min(TILE, nk - t * TILE);      // windows of this tile
            int m = 64;                                        // the power of two that is sorted
            while (m < in_tile) m <<= 1;
            // roll PER consecutive windows
            const int w0 = t * TILE + tid * PER;
            kmer_t fw = 0, rc = 0;
            int run = 0;
            if (w0 < nk) {
                for (int p = 0; p < k - 1; ++p) {
                    const int c = (int)seq[w0 + p];
                    if (c > 3) { run = 0; fw = rc = 0; continue; }
                    fw = ((fw << 2) | (kmer_t)c) & mask;
                    rc = (rc >> 2) | ((kmer_t)(3 - c) << (2 * (k - 1)));
                    ++run;
                }
            }
#pragma unroll
            for (int q = 0; q < PER; ++q) {
                kmer_t key = NONE;
                if (w0 + q < nk) {
                    const int c = (int)seq[w0 + q + k - 1];
                    if (c > 3) { run = 0; fw = rc = 0; }
                    else {
                        fw = ((fw << 2) | (kmer_t)c) & mask;
                        rc = (rc >> 2) | ((kmer_t)(3 - c) << (2 * (k - 1)));
                        if (++run >= k) key = fw < rc ? fw : rc;
                    }
                }
                s_key[tid * PER + q] = key;
            }
            __syncthreads();
            for (int size = 2; size <= m; size <<= 1)
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int p = tid; p < m / 2; p += THREADS) {
                        const int lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                        const bool up = (lo & size) == 0;
                        const kmer_t x = s_key[lo], y = s_key[hi];
                        if ((x > y) == up) { s_key[lo] = y; s_key[hi] = x; }
                    }
                    __syncthreads();
                }
            if (n_tiles == 1) count = write_distinct((const kmer_t*)s_key, m, out, tid, s_wsum);
            else {
                for (int p = tid; p < TILE; p += THREADS) ping[(int64_t)t * TILE + p] = s_key[p];
                __syncthreads();                               // (the tile is rolled again)
            }
        }
        if (n_tiles > 1) {
            const int n = n_tiles * TILE;
            kmer_t* src = ping;
            kmer_t* dst = pong;
            for (int width = TILE; width < n; width <<= 1) {
                __syncthreads();                               // the runs of the pass before are in memory
                for (int e = tid; e < n; e += THREADS) {
                    const int r = e / width;
                    const int a0 = (r >> 1) * 2 * width, b0 = min(a0 + width, n), b1 = min(a0 + 2 * width, n);
                    const kmer_t key = src[e];
                    int lo, hi, pos;
                    if ((r & 1) == 0) {                        // a key of the first run: behind the keys of the second that are smaller
                        lo = b0; hi = b1;
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if (src[mid] < key) lo = mid + 1; else hi = mid; }
                        pos = e + (lo - b0);
                    } else {                                   // of the second: behind the keys of the first that are not larger
                        lo = a0; hi = b0;
                        while (lo < hi) { const int mid = (lo + hi) >> 1; if (src[mid] <= key) lo = mid + 1; else hi = mid; }
                        pos = a0 + (e - b0) + (lo - a0);
                    }
                    dst[pos] = key;
                }
                kmer_t* const tmp = src; src = dst; dst = tmp;
            }
            __syncthreads();
            count = write_distinct((const kmer_t*)src, n, out, tid, s_wsum);
        }
        if (tid == 0) A.set_size[s] = count;
    }
}

// One wavefront per pair of sets, taken from a queue.
__global__ __launch_bounds__(64) void mash_pair_kernel(const MashPairArgs A) {
    using namespace sxg_split;
    const int lane = (int)threadIdx.x;
    __shared__ int s_work;
    for (;;) {
        const int p = pop(A.queue, lane, &s_work);
        if (p >= A.n_pairs) break;
        const int sa = uniform(A.pair_a[p]), sb = uniform(A.pair_b[p]);
        const int got = sxg_mash::set_intersect(A.sets + A.seq_off[sa], uniform(A.set_size[sa]), A.sets + A.seq_off[sb], uniform(A.set_size[sb]), lane);
        if (lane == 0) A.inter[p] = got;
    }
}

// One persistent wavefront per block: split_kernel's loops with M4 inside the member loop.
__global__ __launch_bounds__(64) void split_mash_kernel(const MashBlockArgs B) {
    using namespace sxg_split;
    const SplitBlockArgs& A = B.S;
    const int lane = (int)threadIdx.x;
    __shared__ int s_work;
    SPLIT_GLOBAL sxg_key_t* bound = (SPLIT_GLOBAL sxg_key_t*)(A.bound + (int64_t)blockIdx.x * 3 * A.bound_rows);
    int32_t* tail = A.lists + (int64_t)blockIdx.x * 2 * A.list_cap;
    int32_t* prev = tail + A.list_cap;
    const SPLIT_GLOBAL uint8_t* bases = (const SPLIT_GLOBAL uint8_t*)A.bases;
    for (;;) {
        const int w = pop(A.queue, lane, &s_work);
        if (w >= A.n_work) break;
        const int blk = uniform(A.work[w]);
        const int s0 = uniform(A.blk_off[blk]), n = uniform(A.blk_off[blk + 1]) - s0;
        const double t = A.identity[blk], ratio_min = A.ratio_min[blk];
        const double one_minus = 1.0 - t;
        const unsigned long long len_thr = one_minus == 0.0 ? ~0ull : (unsigned long long)(t / one_minus);
        const int min_len = uniform(B.min_len[blk]);
        const double f = B.f[blk], jmin = B.jmin[blk];
        int ng = n > 0 ? 1 : 0;
        long long n_pairs = 0, n_mash = 0;
        unsigned long long cells = 0;
        if (lane == 0 && n > 0) { tail[0] = 0; prev[0] = -1; A.group[s0] = 0; }
        __syncthreads();
        for (int i = 1; i < n; ++i) {
            const int64_t oc = A.seq_off[s0 + i];
            const int curr_len = uniform((int)(A.seq_off[s0 + i + 1] - oc));
            const int ki = uniform(B.set_size[s0 + i]);
            const unsigned long long size_thr = (unsigned long long)((double)ki * f);
            const bool curr_mash = min_len > 0 && curr_len >= min_len;
            int found = -1;
            for (int rev = 0; rev < 2 && found < 0; ++rev) {
                for (int g = ng - 1; g >= 0 && found < 0; --g) {
                    for (int k = uniform(tail[g]); k >= 0; k = uniform(prev[k])) {
                        const int64_t oo = A.seq_off[s0 + k];
                        const int other_len = uniform((int)(A.seq_off[s0 + k + 1] - oo));
                        if ((double)other_len / (double)curr_len < ratio_min) break;
                        if (curr_mash && other_len >= min_len) {
                            if (rev) continue;                 // the strand is in the canonical k-mer (:471)
                            const int ko = uniform(B.set_size[s0 + k]);
                            if ((unsigned long long)ko < size_thr) break;
                            ++n_mash;
                            const int inter = sxg_mash::set_intersect(B.sets + oc, ki, B.sets + oo, ko, lane);
                            const int uni = ki + ko - inter;
                            if (uni > 0 && (double)inter / (double)uni >= jmin) { found = g; break; }
                            continue;
                        }
                        if (other_len < curr_len && (unsigned long long)other_len < len_thr) break;
                        ++n_pairs;
                        cells += (unsigned long long)other_len * (unsigned long long)curr_len;
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
        if (lane == 0) { A.n_groups[blk] = ng; A.n_pairs[blk] = n_pairs; A.cells[blk] = cells; B.n_mash[blk] = n_mash; }
    }
}

void sxg_mash_launch_sketch(const MashSketchArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(mash_sketch_kernel, dim3((unsigned)n_slots), dim3(SXG_MASH_THREADS), 0, stream, A);
}
void sxg_mash_launch_pairs(const MashPairArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(mash_pair_kernel, dim3((unsigned)n_slots), dim3(64), 0, stream, A);
}
void sxg_mash_launch_blocks(const MashBlockArgs& A, int n_slots, hipStream_t stream) {
    hipLaunchKernelGGL(split_mash_kernel, dim3((unsigned)n_slots), dim3(64), 0, stream, A);
}
int sxg_mash_occupancy(int which, int* groups_per_cu) {
    int n = 0;
    const hipError_t e = which == 0   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mash_sketch_kernel, SXG_MASH_THREADS, 0)
                         : which == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)mash_pair_kernel, 64, 0)
                                      : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)split_mash_kernel, 64, 0);
    if (e != hipSuccess || n < 1) n = 1;
    *groups_per_cu = n;
    return 0;
}
#endif  // SXG_SPLIT_IMPL
#endif

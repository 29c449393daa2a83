// poa_sgd.hip.h -- the path-guided SGD node order of `prep` (src/prep.cpp:11-163) on the device, decree Y (Y1-Y7) of DESIGN.md
// section 9: a deterministic stand-in for odgi's hogwild path_linear_sgd.  Terms are drawn by a counter-based generator, run in
// synchronous batches that all read the coordinates of the batch's start, and add their moves as 64-bit INTEGERS (units of
// 2^-20 bp): integer sums do not depend on the order the atomics arrive in, so the result is the same bits on every run and on
// both paths below.
//
// Included by sxg_poa.hip for the argument struct and the launchers' prototypes; kern_sgd.hip defines SXG_SGD_IMPL and holds the
// kernels (a translation unit of its own, built with -ffp-contract=off: Y5 rounds every double operation once).
//
// LDS path:    one workgroup keeps X and D (16 bytes per node) on chip for the whole sort; batches are separated by
//              __syncthreads; one launch.  N <= SXG_SGD_LDS_NODES.
// global path: one launch of sgd_term_kernel (one thread per term, atomicAdd on unsigned long long in HBM) and one of
//              sgd_apply_kernel (X += D, D = 0) per batch; the kernel boundary is the barrier.
#ifndef SXG_POA_SGD_HIP_H
#define SXG_POA_SGD_HIP_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SXG_SGD_LDS_NODES 8192   /* 16 * N bytes of dynamic LDS: 128 KiB of the CU's 160 */
#define SXG_SGD_SHIFT 20         /* X counts 2^-20 bp */
#define SXG_SGD_TERM_THREADS 256

struct SgdArgs {
    const int32_t* node_len;    // [n_nodes]
    const int64_t* path_off;    // [n_paths + 1]
    const int32_t* step_node;   // [S]
    const int64_t* step_pos;    // [S]
    const double* eta;          // [iter_max]
    unsigned long long* X;      // [n_nodes] two's complement int64; Y1's start on entry
    unsigned long long* D;      // [n_nodes] zero on entry (global path only)
    int32_t n_nodes, n_paths;
    uint64_t S;                 // path_off[n_paths] >= 1
    int32_t iter_max, cooling_start;
    int32_t nb;                 // Y4: max(1, bitlength(longest path in steps - 1))
    uint64_t terms_per_iter, seed;
    uint64_t B;                 // Y6: max(1, n_nodes / 8)
};

int sxg_sgd_prepare_lds(size_t smem);   // 0, or the hipError_t of the dynamic-LDS attribute
void sxg_sgd_launch_lds(const SgdArgs& A, int threads, size_t smem, hipStream_t stream);
void sxg_sgd_launch_terms(const SgdArgs& A, int it, uint64_t k0, uint32_t count, hipStream_t stream);
void sxg_sgd_launch_apply(const SgdArgs& A, hipStream_t stream);

#ifdef SXG_SGD_IMPL
namespace sxg_sgd {

typedef unsigned long long u64;

__device__ __forceinline__ u64 mix(u64 x) {   // Y3
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// Y3 + Y4: the two nodes of term k of iteration `it` and the distance of the chosen node ends along their path; false = skipped
__device__ __forceinline__ bool draw(const SgdArgs& A, const int it, const u64 k, int& ni, int& nj, long long& d) {
    const u64 base = mix(A.seed ^ ((u64)it << 40) ^ k);
    const u64 r1 = mix(base), r2 = mix(r1), r3 = mix(r2);
    const long long a = (long long)(r1 % A.S);
    int lo = 0, hi = A.n_paths;                       // the last path that starts at or before a (empty paths start where the next does)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (A.path_off[mid] <= a) lo = mid; else hi = mid;
    }
    const long long p0 = A.path_off[lo], n = A.path_off[lo + 1] - p0, ia = a - p0;
    long long ib;
    if ((r2 & 1) || it >= A.cooling_start) {
        const int bits = (int)((r2 >> 1) % (u64)A.nb);
        const long long j = (1ll << bits) + (long long)((r2 >> 8) & ((1ull << bits) - 1));
        const bool fwd = (r2 >> 7) & 1;
        ib = fwd ? ia + j : ia - j;
        if (ib < 0 || ib >= n) ib = fwd ? ia - j : ia + j;
        ib = ib < 0 ? 0 : (ib > n - 1 ? n - 1 : ib);
    } else ib = (long long)(r3 % (u64)n);
    const long long b = p0 + ib;
    ni = A.step_node[a];
    nj = A.step_node[b];
    const long long pa = A.step_pos[a] + (((r3 >> 62) & 1) ? (long long)A.node_len[ni] : 0);
    const long long pb = A.step_pos[b] + ((r3 >> 63) ? (long long)A.node_len[nj] : 0);
    d = pa > pb ? pa - pb : pb - pa;
    return d != 0 && ni != nj;
}

// Y5: what node i loses and node j gains.  IEEE double, one rounding per operation (this translation unit is built without
// contraction; the divisions and multiplications by powers of two are exact).
__device__ __forceinline__ long long move(const long long xi, const long long xj, const bool i_before_j, const double eta, const long long d) {
    const double scale = (double)(1 << SXG_SGD_SHIFT);
    const double dd = (double)d;
    const double dx = (double)(xi - xj) / scale;
    const double mag = fabs(dx);
    const double sgn = dx > 0.0 ? 1.0 : (dx < 0.0 ? -1.0 : (i_before_j ? -1.0 : 1.0));
    double mu = eta / dd;
    mu = mu < 1.0 ? mu : 1.0;
    const double delta = mu * (mag - dd) / 2.0;
    return __double2ll_rn(delta * sgn * scale);   // half to even
}

}  // namespace sxg_sgd

__global__ __launch_bounds__(SXG_SGD_TERM_THREADS) void sgd_term_kernel(const SgdArgs A, const int it, const uint64_t k0, const uint32_t count) {
    using namespace sxg_sgd;
    const uint32_t t = blockIdx.x * SXG_SGD_TERM_THREADS + threadIdx.x;
    if (t >= count) return;
    int ni, nj;
    long long d;
    if (!draw(A, it, k0 + t, ni, nj, d)) return;
    const long long q = move((long long)A.X[ni], (long long)A.X[nj], ni < nj, A.eta[it], d);
    atomicAdd(A.D + ni, 0ull - (u64)q);
    atomicAdd(A.D + nj, (u64)q);
}

__global__ __launch_bounds__(256) void sgd_apply_kernel(const SgdArgs A) {
    const int n = (int)(blockIdx.x * 256 + threadIdx.x);
    if (n >= A.n_nodes) return;
    A.X[n] += A.D[n];
    A.D[n] = 0;
}

__global__ __launch_bounds__(1024) void sgd_lds_kernel(const SgdArgs A) {
    using namespace sxg_sgd;
    extern __shared__ u64 sgd_smem[];
    u64* X = sgd_smem;
    u64* D = sgd_smem + A.n_nodes;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    for (int n = tid; n < A.n_nodes; n += nt) { X[n] = A.X[n]; D[n] = 0; }
    __syncthreads();
    for (int it = 0; it < A.iter_max; ++it) {
        const double eta = A.eta[it];
        for (u64 k0 = 0; k0 < A.terms_per_iter; k0 += A.B) {     // (bounds are the same in every thread: the barriers are met by all)
            const u64 k1 = k0 + A.B < A.terms_per_iter ? k0 + A.B : A.terms_per_iter;
            for (u64 k = k0 + (u64)tid; k < k1; k += (u64)nt) {
                int ni, nj;
                long long d;
                if (draw(A, it, k, ni, nj, d)) {
                    const long long q = move((long long)X[ni], (long long)X[nj], ni < nj, eta, d);
                    atomicAdd(D + ni, 0ull - (u64)q);
                    atomicAdd(D + nj, (u64)q);
                }
            }
            __syncthreads();
            for (int n = tid; n < A.n_nodes; n += nt) { X[n] += D[n]; D[n] = 0; }
            __syncthreads();
        }
    }
    for (int n = tid; n < A.n_nodes; n += nt) A.X[n] = X[n];
}

int sxg_sgd_prepare_lds(size_t smem) {
    return (int)hipFuncSetAttribute((const void*)sgd_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
}
void sxg_sgd_launch_lds(const SgdArgs& A, int threads, size_t smem, hipStream_t stream) {
    hipLaunchKernelGGL(sgd_lds_kernel, dim3(1), dim3((unsigned)threads), smem, stream, A);
}
void sxg_sgd_launch_terms(const SgdArgs& A, int it, uint64_t k0, uint32_t count, hipStream_t stream) {
    hipLaunchKernelGGL(sgd_term_kernel, dim3((count + SXG_SGD_TERM_THREADS - 1) / SXG_SGD_TERM_THREADS), dim3(SXG_SGD_TERM_THREADS), 0, stream, A, it, k0, count);
}
void sxg_sgd_launch_apply(const SgdArgs& A, hipStream_t stream) {
    hipLaunchKernelGGL(sgd_apply_kernel, dim3(((unsigned)A.n_nodes + 255u) / 256u), dim3(256), 0, stream, A);
}
#endif  // SXG_SGD_IMPL
#endif

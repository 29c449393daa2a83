// poa_identity_key.h -- the integer arithmetic of decree Q (include/sxg_poa.h): the order key of a pair of
// k-mer sets, the word the device keeps per pair, and the rank of the percentile.  No HIP in here: the kernels of
// poa_identity.hip.h, the host side of sxg_poa_block_identity_batch and tests/csrc/identity_key_check.cpp include this one file.
#ifndef SXG_POA_IDENTITY_KEY_H
#define SXG_POA_IDENTITY_KEY_H
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SXG_IDENT_FN __host__ __device__ static inline
#else
#define SXG_IDENT_FN static inline
#endif

#define SXG_IDENT_UNI_BITS 16   /* uni = |K_i| + |K_j| - inter <= 2 * SXG_POA_MAX_SEQ_LEN < 2^16 */
#define SXG_IDENT_WORD_BITS 49  /* a key is at most 2^32 (inter == uni): 33 bits above the 16 of uni */

// Q2: J = inter / uni as a fixed-point floor.  Two different J with denominators below 2^16 differ by more than 2^-32, so the
// keys order pairs exactly as J does and equal keys mean equal J.
SXG_IDENT_FN uint64_t sxg_identity_key(const uint32_t inter, const uint32_t uni) {
    return uni ? ((uint64_t)inter << 32) / uni : 0;
}
// The word of a pair: its key above its uni.  Words order by key first, so the idx-th smallest word holds an idx-th smallest key;
// which of the pairs of equal J it is does not depend on the order the pairs were written in, only on the values.
SXG_IDENT_FN uint64_t sxg_identity_word(const uint32_t inter, const uint32_t uni) {
    return (sxg_identity_key(inter, uni) << SXG_IDENT_UNI_BITS) | (uint64_t)uni;
}
// inter back from (key, uni): inter * 2^32 = key * uni + r with 0 <= r < uni, so inter = ceil(key * uni / 2^32)
SXG_IDENT_FN void sxg_identity_counts(const uint64_t word, uint32_t* inter, uint32_t* uni) {
    const uint64_t u = word & ((1ull << SXG_IDENT_UNI_BITS) - 1ull), key = word >> SXG_IDENT_UNI_BITS;
    *uni = (uint32_t)u;
    *inter = (uint32_t)((key * u + 0xffffffffull) >> 32);
}
// Q3: the 0-based rank of the percentile among P >= 1 values, as the host estimator computes it (src/smooth.cpp:2026)
SXG_IDENT_FN uint64_t sxg_identity_idx(const uint64_t n_pairs, const double percentile) {
    return (uint64_t)(size_t)((double)(n_pairs - 1) * percentile);
}
// pairs i < j of n sequences in row-major order: the pairs of the rows before row i
SXG_IDENT_FN int64_t sxg_identity_row_start(const int64_t i, const int64_t n) { return i * (2 * n - i - 1) / 2; }

#endif

// poa_msa_cols.h -- the arithmetic of the trimmed MSA (sxg_poa_batch_in::want_msa == SXG_MSA_TRIMMED, include/sxg_poa.h): where
// a column starts (decree S8), which letters of a row survive the trim (src/smooth.cpp:791-812), the columns a chunk of a row
// owns, and how a run of bytes at an arbitrary address splits into a byte-granular head, 16-byte groups and a byte-granular tail.
// No HIP in here: the kernels of poa_msa.hip.h, the host side of sxg_poa.hip and tests/csrc/msa_cols_check.cpp include this one
// file.
#ifndef SXG_POA_MSA_COLS_H
#define SXG_POA_MSA_COLS_H
#include <stdint.h>

#if defined(__HIPCC__)
#define SXG_MSA_FN __host__ __device__ static inline
#else
#define SXG_MSA_FN static inline
#endif

#define SXG_MSA_CHUNK 2048   /* letters of a row one work item of the rows kernel places */
#define SXG_MSA_TILE 4096    /* bytes of a row the rows kernel builds on chip at once (a multiple of 16) */
#define SXG_MSA_GAP 0x2d     /* '-' (GAP_CHAR, src/smooth.cpp:8-11) */

// S8: the nodes of a block in rank order; a column starts at rank 0 and wherever the aligned group changes.  The column of
// the node at rank r is (the number of heads at ranks 0..r) - 1.
SXG_MSA_FN int sxg_msa_head(const int64_t r, const int32_t group_before, const int32_t group_here) {
    return r == 0 || group_before != group_here ? 1 : 0;
}

// The letters [k0, k1) of a row of `len` letters that stay after `trim` letters were blanked at both ends (:791-812).  A row
// with fewer than 2 * trim letters keeps none (the reference would run off the row).
SXG_MSA_FN void sxg_msa_kept(const int64_t len, const int64_t trim, int64_t* k0, int64_t* k1) {
    if (trim < 0 || len < 2 * trim) { *k0 = 0; *k1 = 0; return; }
    *k0 = trim; *k1 = len - trim;
}

// Chunks of a row's kept letters: chunk c holds `chunk` letters from k0 + c * chunk on (the kernels pass SXG_MSA_CHUNK) -- a row
// that keeps nothing still has ONE chunk, which owns the whole (all-gap) row.
SXG_MSA_FN int64_t sxg_msa_chunks(const int64_t k0, const int64_t k1, const int64_t chunk) {
    return k1 <= k0 ? 1 : (k1 - k0 + chunk - 1) / chunk;
}
SXG_MSA_FN void sxg_msa_chunk_letters(const int64_t k0, const int64_t k1, const int64_t c, const int64_t chunk, int64_t* a, int64_t* z) {
    const int64_t lo = k0 + c * chunk, hi = lo + chunk;
    *a = lo < k1 ? lo : k1;
    *z = hi < k1 ? hi : k1;
    if (*a < k0) *a = k0;
}
// The columns [*s, *e) a chunk [a, z) of the kept letters [k0, k1) owns inside the block's kept columns [b0, e0): from its first
// letter's column (b0 for the row's first chunk) to the first column of the next chunk (e0 for the last).  col_a / col_z: the
// column of letter a / of letter z (read only where that letter exists and the chunk is not the first / the last).  Columns rise
// strictly along a row, so the spans of a row's chunks are disjoint and cover [b0, e0).
SXG_MSA_FN void sxg_msa_span(const int64_t k0, const int64_t k1, const int64_t a, const int64_t z, const int32_t b0, const int32_t e0,
                             const int32_t col_a, const int32_t col_z, int32_t* s, int32_t* e) {
    *s = a <= k0 ? b0 : col_a;
    *e = z >= k1 ? e0 : col_z;
}

// n bytes at byte address addr: `head` bytes up to the next 16-byte boundary (all n if the run ends before it), then `body` bytes
// in whole 16-byte groups, then `tail` bytes.
SXG_MSA_FN void sxg_msa_split16(const uint64_t addr, const int64_t n, int64_t* head, int64_t* body, int64_t* tail) {
    int64_t h = (int64_t)((16 - (addr & 15)) & 15);
    if (h > n) h = n;
    if (n <= 0) { *head = 0; *body = 0; *tail = 0; return; }
    *head = h;
    *body = (n - h) & ~(int64_t)15;
    *tail = n - h - *body;
}

#endif

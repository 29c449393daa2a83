// poa_letters.h -- the index arithmetic of the range gather (poa_letters.hip.h): ranges of a graph's
// resident path letters, cut out into a destination that holds them back to back.  HIP-free: the kernel does nothing with the
// letters but call sxg_letters_granule once per lane and 16-byte destination granule, and tests/csrc/letters_check.cpp makes
// the same calls on the host.
//
// The destination is one buffer whose base is 16-byte aligned; range r owns its bytes [off[r], off[r + 1]) (off: the prefix sums of
// the range lengths, [n + 1], off[0] == 0) and reads letters[src[r] ...].  A work item is a chunk of SXG_LETTERS_CHUNK destination
// bytes; the ranges of a chunk, and of a granule in it, are found from `off` by binary search (sxg_letters_find).  A granule that
// lies inside ONE range is an unaligned 16-byte load and an aligned 16-byte store; a granule that holds an edge of a range (or
// the end of the destination) goes out byte by byte -- at most 15 head and 15 tail bytes of a range -- so no store of a range
// touches a byte of its neighbours, and every destination byte is written once, by one lane.  Source and destination alignment
// are independent: the load takes the address as it is.  Nothing is read outside [src[r], src[r] + length of r): the resident
// letters need no padding.
#ifndef SXG_POA_LETTERS_H
#define SXG_POA_LETTERS_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SXG_LETTERS_FN __host__ __device__ static inline
#else
#define SXG_LETTERS_FN static inline
#endif

#define SXG_LETTERS_THREADS 256
#define SXG_LETTERS_LANE_GRANULES 4
#define SXG_LETTERS_CHUNK (16 * SXG_LETTERS_THREADS * SXG_LETTERS_LANE_GRANULES)   /* 16384 destination bytes per work item */

// THE code table of the identity estimate (identity_table of sxg_smooth.cpp): either case of A C G T -> 0..3, anything else -> 4
SXG_LETTERS_FN uint8_t sxg_letters_code(uint8_t ch) {
    const uint8_t u = (uint8_t)(ch & 0xDF);   // (clears the case bit: only 'a' and 'A' give 'A', and so on)
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}
// 0x01 in every byte of x that is zero, exactly (no carry leaves a byte)
SXG_LETTERS_FN uint32_t sxg_letters_zero_bytes(uint32_t x) {
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    return (~(t | x | 0x7F7F7F7Fu)) >> 7;
}
// the table on the four bytes of a word, in registers: 4 - (4 [A] + 3 [C] + 2 [G] + 1 [T]) per byte
SXG_LETTERS_FN uint32_t sxg_letters_code4(uint32_t w) {
    const uint32_t u = w & 0xDFDFDFDFu;
    const uint32_t a = sxg_letters_zero_bytes(u ^ 0x41414141u), c = sxg_letters_zero_bytes(u ^ 0x43434343u),
                   g = sxg_letters_zero_bytes(u ^ 0x47474747u), t = sxg_letters_zero_bytes(u ^ 0x54545454u);
    return 0x04040404u - (a << 2) - (c + (c << 1)) - (g << 1) - t;
}

// the greatest r in [lo, hi] with off[r] <= p (off non-decreasing, off[lo] <= p): for p inside the destination, the range that owns
// byte p -- the empty ranges that start at p come before it
SXG_LETTERS_FN int64_t sxg_letters_find(const int64_t* off, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
SXG_LETTERS_FN int64_t sxg_letters_n_chunks(int64_t total) { return (total + SXG_LETTERS_CHUNK - 1) / SXG_LETTERS_CHUNK; }
// destination position of granule j of `lane` in chunk c: the lanes of a step write 4 KB in a row
SXG_LETTERS_FN int64_t sxg_letters_granule_pos(int64_t c, int j, int lane) {
    return c * SXG_LETTERS_CHUNK + 16 * ((int64_t)j * SXG_LETTERS_THREADS + lane);
}

typedef struct sxg_letters_q { uint32_t w[4]; } sxg_letters_q;

// the granule [p, p + 16) of the destination, p a multiple of 16 below `total`; [r0, r1]: ranges that hold the granule's owners
template <int CODED>
SXG_LETTERS_FN void sxg_letters_granule(const uint8_t* letters, uint8_t* dst, const int64_t* off, const int64_t* src, int64_t r0, int64_t r1,
                                        int64_t p, int64_t total) {
    int64_t r = sxg_letters_find(off, r0, r1, p);
    if (off[r + 1] - p >= 16) {   // inside one range
        sxg_letters_q q;
        __builtin_memcpy(&q, letters + src[r] + (p - off[r]), 16);
        if (CODED) { q.w[0] = sxg_letters_code4(q.w[0]); q.w[1] = sxg_letters_code4(q.w[1]); q.w[2] = sxg_letters_code4(q.w[2]); q.w[3] = sxg_letters_code4(q.w[3]); }
        __builtin_memcpy(__builtin_assume_aligned(dst + p, 16), &q, 16);
        return;
    }
    const int64_t pe = p + 16 < total ? p + 16 : total;
    for (int64_t x = p; x < pe; ++x) {
        while (off[r + 1] <= x) ++r;
        const uint8_t ch = letters[src[r] + (x - off[r])];
        dst[x] = CODED ? sxg_letters_code(ch) : ch;
    }
}
#endif

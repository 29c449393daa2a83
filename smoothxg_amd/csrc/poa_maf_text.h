// poa_maf_text.h -- the index arithmetic and the byte moves of the MAF text gather (poa_maf_text.hip.h): a
// list of segments -- literal bytes the host formatted, rows of the resident trimmed MSA as they stand, rows reversed and
// complemented -- laid out back to back in one destination.  Free of any GPU runtime: the kernel does nothing but call
// sxg_maf_granule once per lane and 16-byte destination granule, and tests/csrc/maf_text_check.cpp makes the same calls on the host.
//
// The destination is one buffer whose base is 16-byte aligned and whose size is a multiple of 16; segment s owns its bytes
// [off[s], off[s + 1]) (off: the prefix sums of the segment lengths, [n + 1], off[0] == 0).  srck[s] = (where the segment starts in
// its source) * 4 + kind; kind 0 reads the literal blob, kinds 1 and 2 the rows.  A work item is a chunk of SXG_MAF_CHUNK
// destination bytes; the segments of a chunk, and of a granule in it, are found from `off` by binary search (sxg_maf_find).
//
// A granule is ASSEMBLED IN REGISTERS from every segment that overlaps it -- a literal is a few tens of bytes, so two or three
// segments in a granule are the rule -- and leaves as one aligned 16-byte store; the bytes of the last granule behind `total`
// are written as zeros (the destination has room for them).  Every destination byte is written once, by one lane; there is no
// byte store.  A piece of a segment of 16 bytes or more is ONE unaligned 16-byte load whose address is clipped to the segment
// (and a shift in registers); a piece of a shorter segment is read byte by byte.  Nothing is read outside
// [start, start + length) of a segment's source: neither source needs padding.
//
// Kind 2 reads the mirrored 16 source bytes, reverses them in registers (a byte swap of each half, the halves exchanged) and
// complements them on packed bytes with the table of revcomp_gapped (sxg_smooth.cpp): '-' -> '-', 'A' <-> 'T', 'C' <-> 'G',
// EVERY other byte value (lower case included) -> 'N'.  sxg_maf_comp states that table for one byte, sxg_maf_comp4 for four.
#ifndef SXG_POA_MAF_TEXT_H
#define SXG_POA_MAF_TEXT_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SXG_MAF_FN __host__ __device__ static inline
#else
#define SXG_MAF_FN static inline
#endif

#define SXG_MAF_THREADS 256
#define SXG_MAF_LANE_GRANULES 4
#define SXG_MAF_CHUNK (16 * SXG_MAF_THREADS * SXG_MAF_LANE_GRANULES)   /* 16384 destination bytes per work item */

#define SXG_MAF_LITERAL 0
#define SXG_MAF_ROW 1
#define SXG_MAF_ROW_REVCOMP 2

// the bytes of a 32-bit word in reverse order (the kernel's translation unit names the instruction: poa_maf_text.hip.h)
#ifndef SXG_MAF_BSWAP32
#define SXG_MAF_BSWAP32(w) __builtin_bswap32(w)
#endif

// THE table, for all 256 byte values
SXG_MAF_FN uint8_t sxg_maf_comp(uint8_t ch) {
    return ch == '-' ? '-' : ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : 'N';
}
// 0xFF in every byte of x that is zero, exactly (no carry leaves a byte)
SXG_MAF_FN uint32_t sxg_maf_zero_bytes(uint32_t x) {
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    const uint32_t f = (~(t | x | 0x7F7F7F7Fu)) >> 7;   // 0x01 per zero byte
    return (f << 8) - f;                               // f * 255, modulo 2^32
}
// the table on the four bytes of a word, in registers, without a branch: 'N' everywhere, exchanged for the image where a byte matches
SXG_MAF_FN uint32_t sxg_maf_comp4(uint32_t w) {
    const uint32_t a = sxg_maf_zero_bytes(w ^ 0x41414141u), c = sxg_maf_zero_bytes(w ^ 0x43434343u), g = sxg_maf_zero_bytes(w ^ 0x47474747u),
                   t = sxg_maf_zero_bytes(w ^ 0x54545454u), gap = sxg_maf_zero_bytes(w ^ 0x2D2D2D2Du);
    return 0x4E4E4E4Eu ^ (a & (0x4E4E4E4Eu ^ 0x54545454u)) ^ (t & (0x4E4E4E4Eu ^ 0x41414141u)) ^ (c & (0x4E4E4E4Eu ^ 0x47474747u)) ^
           (g & (0x4E4E4E4Eu ^ 0x43434343u)) ^ (gap & (0x4E4E4E4Eu ^ 0x2D2D2D2Du));
}

// 16 bytes in registers: byte i of the granule is byte i of the little-endian pair (lo, hi)
typedef struct sxg_maf_v { uint64_t lo, hi; } sxg_maf_v;

// byte i of the result = byte i + k of v, zeros from above; k in 0 .. 15
SXG_MAF_FN sxg_maf_v sxg_maf_down(sxg_maf_v v, int k) {
    const int b = 8 * (k & 7);
    const uint64_t lo = b ? (v.lo >> b) | (v.hi << (64 - b)) : v.lo, hi = v.hi >> b;
    sxg_maf_v r;
    r.lo = k & 8 ? hi : lo; r.hi = k & 8 ? 0 : hi;
    return r;
}
// byte i + k of the result = byte i of v, zeros from below; k in 0 .. 15
SXG_MAF_FN sxg_maf_v sxg_maf_up(sxg_maf_v v, int k) {
    const int b = 8 * (k & 7);
    const uint64_t hi = b ? (v.hi << b) | (v.lo >> (64 - b)) : v.hi, lo = v.lo << b;
    sxg_maf_v r;
    r.hi = k & 8 ? lo : hi; r.lo = k & 8 ? 0 : lo;
    return r;
}
// the lowest n bytes of v, zeros above; n in 0 .. 16
SXG_MAF_FN sxg_maf_v sxg_maf_keep(sxg_maf_v v, int n) {
    const int m = n & 7;
    const uint64_t part = m ? ~(uint64_t)0 >> (64 - 8 * m) : 0;
    sxg_maf_v r;
    r.lo = n >= 8 ? v.lo : v.lo & part;
    r.hi = n >= 16 ? v.hi : n > 8 ? v.hi & part : 0;
    return r;
}
SXG_MAF_FN sxg_maf_v sxg_maf_load16(const uint8_t* q) {
    sxg_maf_v v;
    __builtin_memcpy(&v, q, 16);
    return v;
}
// the 16 bytes in reverse order, each complemented
SXG_MAF_FN sxg_maf_v sxg_maf_revcomp16(sxg_maf_v v) {
    const uint32_t w0 = (uint32_t)v.lo, w1 = (uint32_t)(v.lo >> 32), w2 = (uint32_t)v.hi, w3 = (uint32_t)(v.hi >> 32);
    sxg_maf_v r;
    r.lo = (uint64_t)sxg_maf_comp4(SXG_MAF_BSWAP32(w3)) | ((uint64_t)sxg_maf_comp4(SXG_MAF_BSWAP32(w2)) << 32);
    r.hi = (uint64_t)sxg_maf_comp4(SXG_MAF_BSWAP32(w1)) | ((uint64_t)sxg_maf_comp4(SXG_MAF_BSWAP32(w0)) << 32);
    return r;
}

// n bytes (1 .. 16) of a segment's text from its byte t on, in the low bytes of the result, zeros above.  The segment's source
// is base[0 .. len); t + n <= len.  Forward: text byte x = base[x].
SXG_MAF_FN sxg_maf_v sxg_maf_piece(const uint8_t* base, int64_t len, int64_t t, int n) {
    if (len >= 16) {
        const int64_t a = t < len - 16 ? t : len - 16;   // the load clipped to the segment
        return sxg_maf_keep(sxg_maf_down(sxg_maf_load16(base + a), (int)(t - a)), n);
    }
    sxg_maf_v v;
    v.lo = 0; v.hi = 0;
    for (int i = 0; i < n; ++i) {   // (a segment below 16 bytes: n <= 15)
        const uint64_t ch = base[t + i];
        if (i < 8) v.lo |= ch << (8 * i); else v.hi |= ch << (8 * (i - 8));
    }
    return v;
}
// reversed and complemented: text byte x = comp(base[len - 1 - x])
SXG_MAF_FN sxg_maf_v sxg_maf_piece_revcomp(const uint8_t* base, int64_t len, int64_t t, int n) {
    if (len >= 16) {
        const int64_t want = len - t - 16, a = want > 0 ? want : 0;   // the mirrored load, clipped to the segment
        // reversed byte j is base[a + 15 - j]; text byte t + i is base[len - 1 - t - i]: j = i + (a - want)
        return sxg_maf_keep(sxg_maf_down(sxg_maf_revcomp16(sxg_maf_load16(base + a)), (int)(a - want)), n);
    }
    sxg_maf_v v;
    v.lo = 0; v.hi = 0;
    for (int i = 0; i < n; ++i) {
        const uint64_t ch = sxg_maf_comp(base[len - 1 - t - i]);
        if (i < 8) v.lo |= ch << (8 * i); else v.hi |= ch << (8 * (i - 8));
    }
    return v;
}

// the greatest s in [lo, hi] with off[s] <= p (off non-decreasing, off[lo] <= p): for p inside the destination, the segment that
// owns byte p -- the empty segments that start at p come before it
SXG_MAF_FN int64_t sxg_maf_find(const int64_t* off, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}
SXG_MAF_FN int64_t sxg_maf_n_chunks(int64_t total) { return (total + SXG_MAF_CHUNK - 1) / SXG_MAF_CHUNK; }
// destination position of granule j of `lane` in chunk c: the lanes of a step write 4 KB in a row
SXG_MAF_FN int64_t sxg_maf_granule_pos(int64_t c, int j, int lane) {
    return c * SXG_MAF_CHUNK + 16 * ((int64_t)j * SXG_MAF_THREADS + lane);
}

// the granule [p, p + 16) of the destination, p a multiple of 16 below `total`; [s0, s1]: segments that hold the granule's owners
SXG_MAF_FN void sxg_maf_granule(const uint8_t* literal, const uint8_t* rows, uint8_t* dst, const int64_t* off, const int64_t* srck, int64_t s0,
                                int64_t s1, int64_t p, int64_t total) {
    int64_t s = sxg_maf_find(off, s0, s1, p);
    const int64_t pe = p + 16 < total ? p + 16 : total;
    sxg_maf_v acc;
    acc.lo = 0; acc.hi = 0;
    for (int64_t x = p; x < pe;) {
        while (off[s + 1] <= x) ++s;   // (empty segments; x < total = off[n] ends the walk)
        const int64_t b = off[s], e = off[s + 1], d1 = e < pe ? e : pe;
        const int kind = (int)(srck[s] & 3);
        const uint8_t* base = (kind == SXG_MAF_LITERAL ? literal : rows) + (srck[s] >> 2);
        const sxg_maf_v piece = kind == SXG_MAF_ROW_REVCOMP ? sxg_maf_piece_revcomp(base, e - b, x - b, (int)(d1 - x))
                                                            : sxg_maf_piece(base, e - b, x - b, (int)(d1 - x));
        const sxg_maf_v placed = sxg_maf_up(piece, (int)(x - p));
        acc.lo |= placed.lo; acc.hi |= placed.hi;
        x = d1;
    }
    __builtin_memcpy(__builtin_assume_aligned(dst + p, 16), &acc, 16);
}

// the letters of a row: bytes other than '-' in rows[begin .. begin + len), read in aligned 16-byte words -- the first and the
// last word reach outside the row but never outside [0, cap), cap a multiple of 16 that covers the row --, masked to the row.
// One call does the words w, w + stride, ... of the row (the kernel: one lane each, then a sum over the workgroup).
SXG_MAF_FN uint32_t sxg_maf_gap_bytes(uint32_t w) {   // how many of the four bytes are '-'
    const uint32_t f = sxg_maf_zero_bytes(w ^ 0x2D2D2D2Du) & 0x01010101u;
    return (f * 0x01010101u) >> 24;
}
SXG_MAF_FN int32_t sxg_maf_row_letters(const uint8_t* rows, int64_t begin, int64_t len, int64_t first, int64_t stride) {
    if (len <= 0) return 0;
    const int64_t end = begin + len, w0 = begin & ~(int64_t)15;
    int32_t letters = 0;
    for (int64_t a = w0 + 16 * first; a < end; a += 16 * stride) {
        sxg_maf_v v;
        __builtin_memcpy(&v, __builtin_assume_aligned(rows + a, 16), 16);
        const int64_t lo = a > begin ? a : begin, hi = a + 16 < end ? a + 16 : end;   // the row's bytes of this word: [lo, hi)
        // the bytes outside the row are shifted and masked away: what is left of them is zero, never '-'
        v = sxg_maf_keep(sxg_maf_down(v, (int)(lo - a)), (int)(hi - lo));
        const uint32_t gaps = sxg_maf_gap_bytes((uint32_t)v.lo) + sxg_maf_gap_bytes((uint32_t)(v.lo >> 32)) + sxg_maf_gap_bytes((uint32_t)v.hi) +
                              sxg_maf_gap_bytes((uint32_t)(v.hi >> 32));
        letters += (int32_t)(hi - lo) - (int32_t)gaps;
    }
    return letters;
}
#endif

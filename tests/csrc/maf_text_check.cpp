// TEST HARNESS: the arithmetic of the MAF text gather (smoothxg_amd/csrc/poa_maf_text.h) on the host, plain C++.  Never shipped.
//
// maf_text_kernel does nothing with the text but call sxg_maf_find twice per chunk and sxg_maf_granule once per lane and granule;
// this program makes the same calls, chunk by chunk and lane by lane, over heap buffers of exactly the sizes the engine needs --
// the literal blob and the rows end with their last byte, the destination is [total rounded up to 16] on a 16-byte boundary --
// so under AddressSanitizer a read past a source or a store past the destination shows.  The segment under test is the LAST
// thing in its source and, at source alignment 0, the FIRST: a load that leaves the segment on either side leaves the heap block.
// It checks
//   * the complement of all 256 byte values against a literal restatement of revcomp_gapped's table (sxg_smooth.cpp), the
//     four-bytes-per-word form against it in every byte position, and the shifts and masks of the 16-byte registers;
//   * sxg_maf_find against a linear scan, empty segments included;
//   * the three kinds x destination alignment 0..15 x source alignment 0..15 x lengths 0..49 and chunk - 1, chunk, chunk + 1,
//     the segment between two guard literals; every destination byte against a byte-wise restatement, the bytes of the last
//     granule behind the total zero;
//   * runs of 1-, 2-, 3- and 15-byte segments of mixed kinds (up to 16 segments in one granule), with empty segments between
//     them, totals that are no multiple of 16, random lists over several chunks, one row used several times, the empty list;
//   * that nothing is written outside [0, total rounded up to 16): a second walk into a buffer between guard bytes;
//   * the letter count of a row (sxg_maf_row_letters, 64 lanes) for every begin and length against a byte loop, the rows'
//     buffer being exactly the total rounded up to 16.
// Lanes and workgroups are walked once ascending and once descending.
// Prints "maf_text <chunk> <cases> <granules walked>"; exit status 1 with the first failures on stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_maf_text.h"

static int bad = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (bad < 20) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
            ++bad;                                           \
        }                                                    \
    } while (0)

static uint64_t lcg_state = 12345;
static uint32_t lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg_state >> 33); }

// revcomp_gapped's table, restated: '-' stays, comp() otherwise
static uint8_t table(uint8_t ch) {
    switch (ch) { case '-': return '-'; case 'A': return 'T'; case 'T': return 'A'; case 'C': return 'G'; case 'G': return 'C'; default: return 'N'; }
}

struct seg_t { int kind; int64_t src, len; };   // src: offset in the literal blob (kind 0) or in the rows
static long n_cases = 0, n_granules = 0;

// a heap block of exactly `bytes` bytes on a 16-byte boundary (bytes == 0: one byte nobody touches)
static uint8_t* block16(size_t bytes) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, bytes ? bytes : 1)) { fprintf(stderr, "out of memory\n"); exit(2); }
    return (uint8_t*)q;
}

// the kernel's walk over one destination, as `groups` workgroups; lanes and workgroups ascending or descending
static void walk(const uint8_t* literal, const uint8_t* rows, uint8_t* dst, const std::vector<int64_t>& off, const std::vector<int64_t>& srck, int64_t total,
                 int groups, bool up) {
    const int64_t n = (int64_t)srck.size(), n_chunks = sxg_maf_n_chunks(total);
    for (int gi = 0; gi < groups; ++gi) {
        const int g = up ? gi : groups - 1 - gi;
        for (int64_t c = g; c < n_chunks; c += groups) {
            const int64_t cb = c * SXG_MAF_CHUNK, ce = cb + SXG_MAF_CHUNK < total ? cb + SXG_MAF_CHUNK : total;
            const int64_t s0 = sxg_maf_find(off.data(), 0, n - 1, cb), s1 = sxg_maf_find(off.data(), s0, n - 1, ce - 1);
            for (int li = 0; li < SXG_MAF_THREADS; ++li) {
                const int lane = up ? li : SXG_MAF_THREADS - 1 - li;
                for (int j = 0; j < SXG_MAF_LANE_GRANULES; ++j) {
                    const int64_t p = sxg_maf_granule_pos(c, j, lane);
                    if (p < ce) { sxg_maf_granule(literal, rows, dst, off.data(), srck.data(), s0, s1, p, total); ++n_granules; }
                }
            }
        }
    }
}

// one segment list over sources of exactly lit_bytes / row_bytes bytes
static void run_case(const std::vector<uint8_t>& lit, const std::vector<uint8_t>& rw, const std::vector<seg_t>& segs, const char* what, int64_t tag) {
    ++n_cases;
    uint8_t* literal = block16(lit.size());
    uint8_t* rows = block16(rw.size());
    if (!lit.empty()) memcpy(literal, lit.data(), lit.size());
    if (!rw.empty()) memcpy(rows, rw.data(), rw.size());
    std::vector<int64_t> off(segs.size() + 1, 0), srck(segs.size(), 0);
    std::vector<uint8_t> want;
    for (size_t s = 0; s < segs.size(); ++s) {
        const seg_t& g = segs[s];
        off[s + 1] = off[s] + g.len;
        srck[s] = g.src * 4 + g.kind;
        const std::vector<uint8_t>& from = g.kind == SXG_MAF_LITERAL ? lit : rw;
        for (int64_t x = 0; x < g.len; ++x) want.push_back(g.kind == SXG_MAF_ROW_REVCOMP ? table(from[(size_t)(g.src + g.len - 1 - x)]) : from[(size_t)(g.src + x)]);
    }
    const int64_t total = off.back(), padded = (total + 15) & ~(int64_t)15;
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: the destination is a heap block of exactly the padded size (the sanitizer sees a store past it);
        // pass 1: it stands between guard bytes, which must come through
        const int64_t guard = pass ? 64 : 0;
        uint8_t* buf = block16((size_t)(padded + 2 * guard));
        memset(buf, 0xA5, (size_t)(padded + 2 * guard) ? (size_t)(padded + 2 * guard) : 1);
        uint8_t* dst = buf + guard;
        walk(literal, rows, dst, off, srck, total, pass ? 3 : 1, pass == 0);
        for (int64_t x = 0; x < total; ++x)
            if (dst[x] != want[(size_t)x]) { CHECK(false, "%s %lld pass %d: byte %lld of %lld is %d, want %d", what, (long long)tag, pass, (long long)x, (long long)total, dst[x], want[(size_t)x]); break; }
        for (int64_t x = total; x < padded; ++x) CHECK(dst[x] == 0, "%s %lld pass %d: byte %lld behind the total is %d", what, (long long)tag, pass, (long long)x, dst[x]);
        for (int64_t x = 0; x < guard; ++x) CHECK(buf[x] == 0xA5 && dst[padded + x] == 0xA5, "%s %lld: a guard byte was written", what, (long long)tag);
        free(buf);
    }
    free(literal); free(rows);
}

static uint8_t row_letter() { static const char a[] = "ACGT-N-ACGTacgtRY*"; return (uint8_t)a[lcg() % (sizeof(a) - 1)]; }

int main() {
    // the table, byte by byte and four at a time in every position
    for (int ch = 0; ch < 256; ++ch) {
        CHECK(sxg_maf_comp((uint8_t)ch) == table((uint8_t)ch), "comp(%d)", ch);
        for (int pos = 0; pos < 4; ++pos) {
            const uint32_t others = lcg();
            const uint32_t w = (others & ~(0xFFu << (8 * pos))) | ((uint32_t)ch << (8 * pos));
            const uint32_t r = sxg_maf_comp4(w);
            for (int k = 0; k < 4; ++k) CHECK(((r >> (8 * k)) & 0xFF) == table((uint8_t)(w >> (8 * k))), "comp4(%08x) byte %d", w, k);
        }
    }
    // the registers: shifts by 0..15 bytes, masks of 0..16 bytes, the reversal
    {
        uint8_t in[16], out[16];
        for (int i = 0; i < 16; ++i) in[i] = (uint8_t)(0x10 + i);
        sxg_maf_v v = sxg_maf_load16(in);
        for (int k = 0; k < 16; ++k) {
            sxg_maf_v d = sxg_maf_down(v, k), u = sxg_maf_up(v, k);
            memcpy(out, &d, 16);
            for (int i = 0; i < 16; ++i) CHECK(out[i] == (i + k < 16 ? in[i + k] : 0), "down %d byte %d", k, i);
            memcpy(out, &u, 16);
            for (int i = 0; i < 16; ++i) CHECK(out[i] == (i >= k ? in[i - k] : 0), "up %d byte %d", k, i);
        }
        for (int n = 0; n <= 16; ++n) {
            sxg_maf_v m = sxg_maf_keep(v, n);
            memcpy(out, &m, 16);
            for (int i = 0; i < 16; ++i) CHECK(out[i] == (i < n ? in[i] : 0), "keep %d byte %d", n, i);
        }
        for (int i = 0; i < 16; ++i) in[i] = (uint8_t)"ACGT-NacgtTTGCA-"[i];
        sxg_maf_v r = sxg_maf_revcomp16(sxg_maf_load16(in));
        memcpy(out, &r, 16);
        for (int i = 0; i < 16; ++i) CHECK(out[i] == table(in[15 - i]), "revcomp16 byte %d", i);
    }
    // the search against a linear scan
    for (int round = 0; round < 200; ++round) {
        const int n = 1 + (int)(lcg() % 40);
        std::vector<int64_t> off((size_t)n + 1, 0);
        for (int s = 0; s < n; ++s) off[(size_t)s + 1] = off[(size_t)s] + (lcg() % 3 == 0 ? 0 : lcg() % 40);
        if (off[(size_t)n] == 0) off[(size_t)n] = 1;
        for (int64_t p = 0; p < off[(size_t)n]; ++p) {
            int64_t lin = 0;
            for (int s = 0; s < n; ++s) if (off[(size_t)s] <= p) lin = s;
            CHECK(sxg_maf_find(off.data(), 0, n - 1, p) == lin, "find %lld", (long long)p);
            CHECK(off[(size_t)lin] <= p && p < off[(size_t)lin + 1], "owner of %lld", (long long)p);
        }
    }
    // kinds x destination alignment x source alignment x length
    std::vector<int64_t> lens;
    for (int64_t l = 0; l <= 49; ++l) lens.push_back(l);
    for (int64_t l = SXG_MAF_CHUNK - 1; l <= SXG_MAF_CHUNK + 1; ++l) lens.push_back(l);
    for (int kind = 0; kind < 3; ++kind)
        for (int da = 0; da < 16; ++da)
            for (int sa = 0; sa < 16; ++sa)
                for (int64_t len : lens) {
                    std::vector<uint8_t> lit, rw;
                    for (int i = 0; i < da; ++i) lit.push_back((uint8_t)('a' + i));   // guard literal in front: da bytes
                    for (int i = 0; i < 7; ++i) lit.push_back((uint8_t)('0' + i));    // guard literal behind: 7 bytes at [da, da + 7)
                    std::vector<uint8_t>& from = kind == SXG_MAF_LITERAL ? lit : rw;
                    while ((int)(from.size() % 16) != sa) from.push_back('#');
                    const int64_t src = (int64_t)from.size();
                    for (int64_t x = 0; x < len; ++x) from.push_back(row_letter());
                    run_case(lit, rw, {seg_t{0, 0, da}, seg_t{kind, src, len}, seg_t{0, da, 7}}, "grid", ((kind * 16 + da) * 16 + sa) * 100000 + len);
                }
    // runs of short segments, mixed kinds, empty ones between
    for (int w : {1, 2, 3, 15})
        for (int shift = 0; shift < 16; ++shift) {
            std::vector<uint8_t> lit, rw;
            for (int i = 0; i < 300 * w + 16; ++i) { lit.push_back((uint8_t)(33 + lcg() % 90)); rw.push_back(row_letter()); }
            std::vector<seg_t> segs;
            if (shift) segs.push_back(seg_t{0, 0, shift});
            for (int s = 0; s < 300; ++s) {
                const int kind = (int)(lcg() % 3);
                if (lcg() % 5 == 0) segs.push_back(seg_t{(int)(lcg() % 3), (int64_t)(lcg() % 50), 0});
                // (the sources end with the blobs' last byte in the last run)
                segs.push_back(seg_t{kind, s == 299 ? (int64_t)lit.size() - w : (int64_t)(lcg() % (lit.size() - (size_t)w)), w});
            }
            run_case(lit, rw, segs, "run", w * 100 + shift);
        }
    // random lists over several chunks; one row used several times
    for (int round = 0; round < 12; ++round) {
        std::vector<uint8_t> lit, rw;
        const int nl = 64 + (int)(lcg() % 200), nr = 5000 + (int)(lcg() % 3000);
        for (int i = 0; i < nl; ++i) lit.push_back((uint8_t)(33 + lcg() % 90));
        for (int i = 0; i < nr; ++i) rw.push_back(row_letter());
        std::vector<seg_t> segs;
        int64_t total = 0;
        while (total < 2 * SXG_MAF_CHUNK + 1000 * round) {
            const int kind = (int)(lcg() % 3);
            const int64_t room = kind == 0 ? nl : nr;
            const int64_t len = kind == 0 ? lcg() % 40 : (lcg() % 4 == 0 ? room : lcg() % 700);
            const int64_t l = len > room ? room : len;
            segs.push_back(seg_t{kind, (int64_t)(lcg() % (uint64_t)(room - l + 1)), l});
            total += l;
        }
        segs.push_back(seg_t{2, 0, nr}); segs.push_back(seg_t{1, 0, nr}); segs.push_back(seg_t{2, 0, nr});
        segs.push_back(seg_t{0, 0, 1 + round});   // (totals of every residue)
        run_case(lit, rw, segs, "random", round);
    }
    // nothing at all, and only empty segments
    run_case({}, {}, {}, "empty", 0);
    run_case({'x'}, {'A'}, {seg_t{0, 0, 0}, seg_t{1, 0, 0}, seg_t{2, 1, 0}}, "empty segments", 0);
    // the letters of a row: every begin and length in a rows' buffer of exactly the padded size, as 64 lanes
    {
        const int64_t total = 16 * 70 + 5, cap = (total + 15) & ~(int64_t)15;
        uint8_t* rows = block16((size_t)cap);
        for (int64_t i = 0; i < cap; ++i) rows[i] = i < total ? row_letter() : (uint8_t)'-';
        for (int64_t begin = 0; begin < 40; ++begin)
            for (int64_t len : {(int64_t)0, (int64_t)1, (int64_t)15, (int64_t)16, (int64_t)17, (int64_t)33, (int64_t)255, (int64_t)1030, total - begin}) {
                if (begin + len > total) continue;
                int32_t want = 0, got = 0;
                for (int64_t x = 0; x < len; ++x) want += rows[begin + x] != '-';
                for (int lane = 0; lane < 64; ++lane) got += sxg_maf_row_letters(rows, begin, len, lane, 64);
                CHECK(got == want, "letters of [%lld, +%lld): %d, want %d", (long long)begin, (long long)len, got, want);
                ++n_cases;
            }
        free(rows);
    }
    if (bad) { fprintf(stderr, "%d failures\n", bad); return 1; }
    printf("maf_text %d %ld %ld\n", SXG_MAF_CHUNK, n_cases, n_granules);
    return 0;
}

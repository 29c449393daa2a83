// TEST HARNESS: the arithmetic of the range gather (smoothxg_amd/csrc/poa_letters.h) on the host, plain C++.  Never shipped.
//
// range_gather_kernel does nothing with the letters but call sxg_letters_find twice per chunk and sxg_letters_granule once per
// lane and granule; this program makes the same calls, chunk by chunk and lane by lane, over heap buffers of exactly the sizes
// the engine allocates -- the letters [n_letters] without padding, the destination [total] on a 16-byte boundary -- so under
// AddressSanitizer a read or a store past either shows.  It checks
//   * the code table over all 256 byte values against a literal restatement of identity_table's switch (sxg_smooth.cpp), and the
//     four-bytes-per-word form against it in every byte position;
//   * sxg_letters_find against a linear scan, empty ranges included;
//   * every source alignment 0..15 x destination alignment 0..15 x length 0..48, then lengths chunk - 1, chunk, chunk + 1 and
//     2 chunk + 3, ranges that touch the first and the last letter of the store, empty, repeated and overlapping ranges: every
//     destination byte against the slice, raw and coded.  The range under test stands between two guard ranges cut from letters
//     that occur nowhere else, and the lanes are walked once in ascending and once in descending order: a store over a range's
//     edge would leave a wrong byte in a guard in one of the two orders.
// Prints "letters <chunk> <cases> <granules walked>"; exit status 1 with the first failures on stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_letters.h"

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

// identity_table's switch, restated
static uint8_t table(uint8_t ch) {
    switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': return 3; default: return 4; }
}

struct range_t { int64_t src, len; };
static long n_cases = 0, n_granules = 0;

// the kernel's walk over one destination, as `groups` workgroups; lanes and chunks ascending or descending
template <int CODED>
static void walk(const uint8_t* letters, uint8_t* dst, const std::vector<int64_t>& off, const std::vector<int64_t>& src, int64_t total, int groups, bool up) {
    const int64_t n = (int64_t)src.size(), n_chunks = sxg_letters_n_chunks(total);
    for (int gi = 0; gi < groups; ++gi) {
        const int g = up ? gi : groups - 1 - gi;
        for (int64_t c = g; c < n_chunks; c += groups) {
            const int64_t cb = c * SXG_LETTERS_CHUNK, ce = cb + SXG_LETTERS_CHUNK < total ? cb + SXG_LETTERS_CHUNK : total;
            const int64_t r0 = sxg_letters_find(off.data(), 0, n - 1, cb), r1 = sxg_letters_find(off.data(), r0, n - 1, ce - 1);
            for (int li = 0; li < SXG_LETTERS_THREADS; ++li) {
                const int lane = up ? li : SXG_LETTERS_THREADS - 1 - li;
                for (int j = 0; j < SXG_LETTERS_LANE_GRANULES; ++j) {
                    const int64_t p = sxg_letters_granule_pos(c, j, lane);
                    if (p < ce) { sxg_letters_granule<CODED>(letters, dst, off.data(), src.data(), r0, r1, p, total); ++n_granules; }
                }
            }
        }
    }
}

static void run_case(const uint8_t* letters, const std::vector<range_t>& ranges, const char* what) {
    ++n_cases;
    std::vector<int64_t> off{0}, src;
    for (auto& r : ranges) { off.push_back(off.back() + r.len); src.push_back(r.src); }
    const int64_t total = off.back();
    if (total == 0) return;   // (the engine launches nothing)
    for (int coded = 0; coded < 2; ++coded)
        for (int up = 0; up < 2; ++up) {
            void* mem = nullptr;
            if (posix_memalign(&mem, 16, (size_t)total) != 0) { fprintf(stderr, "no memory\n"); exit(2); }
            uint8_t* dst = (uint8_t*)mem;
            memset(dst, 0xEE, (size_t)total);
            const int groups = up ? 3 : 2;
            if (coded) walk<1>(letters, dst, off, src, total, groups, up != 0); else walk<0>(letters, dst, off, src, total, groups, up != 0);
            for (size_t r = 0; r < ranges.size(); ++r)
                for (int64_t x = 0; x < ranges[r].len; ++x) {
                    const uint8_t ch = letters[ranges[r].src + x], want = coded ? table(ch) : ch;
                    CHECK(dst[off[r] + x] == want, "%s: coded %d up %d range %zu (src %lld len %lld) byte %lld: got %d, want %d", what, coded, up, r,
                          (long long)ranges[r].src, (long long)ranges[r].len, (long long)x, dst[off[r] + x], want);
                }
            free(dst);
        }
}

int main() {
    // the code table
    for (int b = 0; b < 256; ++b) {
        CHECK(sxg_letters_code((uint8_t)b) == table((uint8_t)b), "code(%d) = %d, want %d", b, sxg_letters_code((uint8_t)b), table((uint8_t)b));
        for (int pos = 0; pos < 4; ++pos) {
            const uint32_t others = lcg(), w = (others & ~(0xFFu << (8 * pos))) | ((uint32_t)b << (8 * pos)), got = sxg_letters_code4(w);
            for (int q = 0; q < 4; ++q)
                CHECK(((got >> (8 * q)) & 0xFF) == table((uint8_t)(w >> (8 * q))), "code4(%08x) byte %d = %u", w, q, (got >> (8 * q)) & 0xFF);
        }
    }
    // the search
    for (int trial = 0; trial < 400; ++trial) {
        const int n = 1 + (int)(lcg() % 40);
        std::vector<int64_t> off{0};
        for (int r = 0; r < n; ++r) off.push_back(off.back() + (lcg() % 3 == 0 ? 0 : (int64_t)(lcg() % 50)));
        for (int64_t p = 0; p < off.back(); ++p) {
            int64_t want = 0;
            for (int r = 0; r < n; ++r) if (off[(size_t)r] <= p) want = r;
            const int64_t got = sxg_letters_find(off.data(), 0, n - 1, p);
            CHECK(got == want && off[(size_t)got + 1] > p, "find: n %d p %lld: got %lld, want %lld", n, (long long)p, (long long)got, (long long)want);
            const int64_t lo = (int64_t)(lcg() % (uint32_t)(want + 1));
            CHECK(sxg_letters_find(off.data(), lo, n - 1, p) == want, "find from %lld: n %d p %lld", (long long)lo, n, (long long)p);
        }
    }
    // the store: exactly S letters on the heap; the last 64 are guard letters ('x', 'y') that occur nowhere else
    const int64_t chunk = SXG_LETTERS_CHUNK, S = 3 * chunk + 101 + 64, body = S - 64;
    static const char alphabet[] = "ACGTNacgtn*-R";
    uint8_t* letters = new uint8_t[(size_t)S];
    for (int64_t i = 0; i < body; ++i) letters[i] = (uint8_t)alphabet[lcg() % 13];
    for (int64_t i = body; i < S; ++i) letters[i] = (i & 1) ? 'x' : 'y';
    const range_t tail_guard{body + 16, 20};
    for (int sa = 0; sa < 16; ++sa)
        for (int da = 0; da < 16; ++da) {
            for (int64_t len = 0; len <= 48; ++len) run_case(letters, {{body, da}, {32 + sa, len}, tail_guard}, "grid");
            if ((sa & 3) == 3 || sa == 0)
                for (int64_t len : {chunk - 1, chunk, chunk + 1, 2 * chunk + 3}) run_case(letters, {{body, da}, {16 + sa, len}, tail_guard}, "chunk");
        }
    for (int da = 0; da < 16; ++da) {
        run_case(letters, {{body, da}, {0, 1}, tail_guard}, "first letter");
        run_case(letters, {{body, da}, {0, 37}, tail_guard}, "from the first letter");
        run_case(letters, {{body, da}, {S - 1, 1}}, "last letter");
        run_case(letters, {{body, da}, {S - 33, 33}}, "to the last letter");
        run_case(letters, {{body, da}, {0, S}, tail_guard}, "whole store");
        run_case(letters, {{0, 0}, {body, da}, {0, 0}, {0, 0}, {5, 40}, {0, 0}, {5, 40}, {20, 40}, {0, 0}}, "empty, repeated and overlapping");
    }
    run_case(letters, {{7, 0}, {9, 0}}, "nothing");
    {   // many short ranges over several chunks: the per-granule search between a chunk's first and last range
        std::vector<range_t> many;
        for (int r = 0; r < 3000; ++r) many.push_back({(int64_t)(lcg() % (uint32_t)(body - 40)), (int64_t)(lcg() % 40)});
        run_case(letters, many, "many");
    }
    delete[] letters;
    printf("letters %d %ld %ld\n", SXG_LETTERS_CHUNK, n_cases, n_granules);
    if (bad) { fprintf(stderr, "%d checks failed\n", bad); return 1; }
    return 0;
}

// TEST HARNESS: the arithmetic of the tandem-repeat scan (smoothxg_amd/csrc/poa_repeat.h, decree R) on the host, plain C++.
// Never shipped.
//
// The counting kernel does nothing with the letters but call sxg_repeat_lane_counts, once per lane and work item; this program
// makes the same calls, lane by lane and item by item, over a heap buffer of exactly n bytes -- so under AddressSanitizer a read
// past a sequence's end shows -- and compares
//   * the lag range, cnt and the tiling with restatements of decree R2;
//   * every count with the naive double loop of the host scan (sxg_smooth.cpp, repeat_length);
//   * sxg_repeat_stats + sxg_repeat_decide with a restatement of repeat_length's sums and its z loop: best, dev and v bit for
//     bit, and the reported length.
// Grid: every n = 0 .. 200 with min_copy in {1, 8, 17}, max_copy in {min_copy, 64, 1000}, stride in {1, 3, 7, 50, 500}; then a few
// long sequences at the reference's parameters (1000, 20000, 50).  Letters come from a 64-bit LCG (tests/test_repeat_counts.py
// restates it): a tandem repeat with substitutions over A C G T a N.
// Prints "grid <cases> <lanes walked>" and one line per long case: "long n period n_lags best length fnv64(counts)"; exit status
// 1 with the first failures on stderr.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_repeat.h"

static int bad = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (bad < 20) { fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
            ++bad;                                           \
        }                                                    \
    } while (0)

static uint64_t lcg_state;
static uint32_t lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg_state >> 33); }

// n letters on the heap, exactly: a unit of `period` letters repeated, every letter replaced with probability sub_pct / 100
static uint8_t* make_seq(int64_t n, int64_t period, uint32_t sub_pct, uint64_t seed) {
    static const char alphabet[] = "ACGTaN";
    lcg_state = seed;
    std::vector<uint8_t> unit((size_t)period);
    for (auto& c : unit) c = (uint8_t)alphabet[lcg() % 6];
    uint8_t* s = new uint8_t[(size_t)n];
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t roll = lcg() % 100, other = lcg() % 6;
        s[i] = roll < sub_pct ? (uint8_t)alphabet[other] : unit[(size_t)(i % period)];
    }
    return s;
}

// repeat_length of sxg_smooth.cpp, restated with what it leaves behind
struct host_scan_t { std::vector<int32_t> match; int64_t best; double dev, v, length; };
static host_scan_t host_scan(const uint8_t* s, uint64_t n, uint64_t min_copy, uint64_t max_copy, double min_z, uint64_t stride) {
    host_scan_t h{{}, -1, 0.0, 0.0, 0.0};
    if (min_copy == 0 || stride == 0 || n < 2 * min_copy) return h;
    const uint64_t hi = max_copy < n - min_copy ? max_copy : n - min_copy;
    if (hi < min_copy) return h;
    std::vector<double> r;
    for (uint64_t L = min_copy; L <= hi; ++L) {
        uint64_t match = 0, cnt = 0;
        for (uint64_t i = 0; i < n - L; i += stride) { match += s[i] == s[i + L] ? 1 : 0; ++cnt; }
        h.match.push_back((int32_t)match);
        r.push_back((double)match / (double)cnt);
    }
    double mean = 0.0;
    for (double x : r) mean += x;
    mean /= (double)r.size();
    double var = 0.0;
    for (double x : r) var += (x - mean) * (x - mean);
    h.v = var / (double)r.size();
    const double sd = std::sqrt(h.v);
    double best_z = 0.0;
    for (size_t k = 0; k < r.size(); ++k) {   // (sd == 0: every z is NaN or 0 / 0 -- the host returns before this loop; best stays the first lag)
        const double z = sd == 0.0 ? 0.0 : (r[k] - mean) / sd;
        if (h.best < 0 || z > best_z) { h.best = (int64_t)k; best_z = z; }
    }
    h.dev = r[(size_t)h.best] - mean;
    h.length = sd != 0.0 && best_z >= min_z ? (double)(min_copy + (uint64_t)h.best) : 0.0;
    return h;
}

static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }

static long long lanes_walked = 0;
// the kernel's walk over one sequence; returns its counts
static std::vector<int32_t> device_walk(const uint8_t* s, int32_t n, int32_t min_copy, int32_t max_copy, int32_t stride) {
    const int32_t n_lags = (int32_t)sxg_repeat_n_lags(n, min_copy, max_copy);
    std::vector<int32_t> match((size_t)n_lags, -1);
    const int32_t tiles = sxg_repeat_n_tiles(n_lags);
    CHECK((int64_t)tiles * SXG_REPEAT_TILE_LAGS >= n_lags && ((int64_t)tiles - 1) * SXG_REPEAT_TILE_LAGS < (n_lags ? n_lags : 1), "tiles of %d lags: %d", n_lags, tiles);
    for (int32_t t = 0; t <= tiles; ++t)   // (one item past the last: every lane of it must decline)
        for (int lane = 0; lane < SXG_REPEAT_WAVE; ++lane) {
            int32_t c[SXG_REPEAT_LANE_LAGS];
            const int m = sxg_repeat_lane_counts(s, n, min_copy, n_lags, stride, t, lane, c);
            ++lanes_walked;
            const int64_t k0 = (int64_t)t * SXG_REPEAT_TILE_LAGS + lane * SXG_REPEAT_LANE_LAGS;
            const int64_t want_m = k0 >= n_lags ? 0 : (n_lags - k0 < SXG_REPEAT_LANE_LAGS ? n_lags - k0 : SXG_REPEAT_LANE_LAGS);
            CHECK(m == want_m && sxg_repeat_lane_first(t, lane) == k0, "n %d tile %d lane %d: %d lags, want %lld", n, t, lane, m, (long long)want_m);
            for (int q = 0; q < m && q < want_m; ++q) {
                CHECK(match[(size_t)(k0 + q)] == -1, "lag index %lld written twice", (long long)(k0 + q));
                match[(size_t)(k0 + q)] = c[q];
            }
        }
    return match;
}

static void check_case(const uint8_t* s, int32_t n, int32_t min_copy, int32_t max_copy, int32_t stride, double min_z, host_scan_t* keep) {
    const host_scan_t h = host_scan(s, (uint64_t)n, (uint64_t)min_copy, (uint64_t)max_copy, min_z, (uint64_t)stride);
    const int32_t n_lags = (int32_t)sxg_repeat_n_lags(n, min_copy, max_copy);
    CHECK((size_t)n_lags == h.match.size(), "n %d (%d, %d): %d lags, the host has %zu", n, min_copy, max_copy, n_lags, h.match.size());
    for (int32_t k = 0; k < n_lags; ++k) {
        int32_t cnt = 0;
        for (int64_t i = 0; i < n - (min_copy + k); i += stride) ++cnt;
        CHECK(sxg_repeat_cnt(n, min_copy + k, stride) == cnt, "cnt(n %d, L %d, stride %d)", n, min_copy + k, stride);
    }
    const std::vector<int32_t> match = device_walk(s, n, min_copy, max_copy, stride);
    CHECK(match == h.match, "n %d (%d, %d, stride %d): counts differ from the naive loop", n, min_copy, max_copy, stride);
    if (n_lags > 0 && match == h.match) {
        int32_t best = -1;
        double dev = 0, v = 0;
        sxg_repeat_stats(match.data(), n, min_copy, n_lags, stride, &best, &dev, &v);
        CHECK(same_bits(v, h.v), "n %d (%d, %d, stride %d): v %a, the host has %a", n, min_copy, max_copy, stride, v, h.v);
        CHECK(best == h.best && same_bits(dev, h.dev), "n %d (%d, %d, stride %d): best %d dev %a, the host has %lld %a", n, min_copy, max_copy, stride, best, dev, (long long)h.best, h.dev);
        CHECK(sxg_repeat_decide(min_copy, best, dev, v, min_z) == h.length, "n %d (%d, %d, stride %d): length", n, min_copy, max_copy, stride);
    }
    if (keep) *keep = h;
}

int main() {
    long long cases = 0;
    const int32_t min_copies[] = {1, 8, 17}, strides[] = {1, 3, 7, 50, 500};
    for (int32_t n = 0; n <= 200; ++n)
        for (int32_t min_copy : min_copies) {
            const int32_t max_copies[] = {min_copy, 64, 1000};
            for (int32_t max_copy : max_copies)
                for (int32_t stride : strides) {
                    // periods inside and outside the lag range; every fifth case an exact repeat (equal greatest r at several lags)
                    const int64_t period = 1 + (n * 7 + min_copy + stride) % 45;
                    uint8_t* s = make_seq(n, period, cases % 5 == 0 ? 0 : 4, 1000 + (uint64_t)cases);
                    check_case(s, n, min_copy, max_copy, stride, cases % 2 ? 5.0 : 2.0, nullptr);
                    delete[] s;
                    ++cases;
                }
        }
    printf("grid %lld %lld\n", cases, lanes_walked);
    const int32_t long_n[] = {2000, 2001, 21000, 21049, 45000}, long_period[] = {1000, 1000, 1200, 7000, 3000};
    for (int k = 0; k < 5; ++k) {
        uint8_t* s = make_seq(long_n[k], long_period[k], 5, 77 + (uint64_t)k);
        host_scan_t h;
        check_case(s, long_n[k], 1000, 20000, 50, 5.0, &h);
        delete[] s;
        uint64_t fnv = 1469598103934665603ull;
        for (int32_t m : h.match)
            for (int b = 0; b < 4; ++b) { fnv ^= (uint64_t)((uint32_t)m >> (8 * b)) & 0xffu; fnv *= 1099511628211ull; }
        printf("long %d %d %zu %lld %.0f %016llx\n", long_n[k], long_period[k], h.match.size(), (long long)h.best, h.length, (unsigned long long)fnv);
    }
    if (bad) fprintf(stderr, "%d checks failed\n", bad);
    return bad ? 1 : 0;
}

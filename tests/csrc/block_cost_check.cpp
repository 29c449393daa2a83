// TEST HARNESS: a block's cost in swept columns and the deal of a launch's blocks over the CUs (smoothxg_amd/csrc/poa_cost.h:
// cost_cols, block_cost, deal_over_cus) -- what sxg_poa.hip sorts, deals and prices launches with and uploads as BlockArgs::est /
// est_done.  Plain C++17, no HIP, no GPU: compile with g++ (the test also builds it with -fsanitize=address,undefined).  Never shipped.
//
//   block_cost_check     fails (exit status 1, reasons on stderr) when
//     * the columns of an alignment are not the kernel's rule -- T * 2 * W2 when W2 != 0 and len + 1 <= T * 2 * W2, T * 2 * W
//       otherwise -- at the boundary len + 1 = T * 2 * W2, one below and one above, for every built class with a second width,
//     * the prefix sums do not start at 0, grow by rows_k * cols_k, or end at the total,
//     * a class without a second width, a banded block or a 32-bit block does not reproduce its columns,
//     * the deal over CUs with ns % ncu != 0 does not give the light CUs the largest costs, loses or repeats a block, or moves
//       anything when there is nothing to deal.
//   It prints one line per dual-width class: tmax W W2 boundary-length cols-below cols-at cols-above.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_cost.h"

using namespace sxg;

static int bad = 0;
static void fault(const char* what, long a, long b, long c, long d) {
    if (++bad <= 20) fprintf(stderr, "%s: %ld %ld (%ld against %ld)\n", what, a, b, c, d);
}

// the model's rows when sequence k is aligned, written out independently of block_cost
static double rows_at(const std::vector<int64_t>& len, int k) {
    double prev = 0;
    for (int j = 0; j < k; ++j) prev += (double)len[(size_t)j];
    return (double)len[0] + 0.05 * prev;
}

// block_cost of the lengths against cols[k] given by the caller: prefix sums and total
static void check_block(const char* what, const std::vector<int64_t>& len, int rm, int T, int W, int W2, const std::vector<uint64_t>& cols) {
    const int n = (int)len.size();
    std::vector<int64_t> off((size_t)n + 1, 1000);   // (offsets of a block in the middle of a batch)
    for (int k = 0; k < n; ++k) off[(size_t)k + 1] = off[(size_t)k] + len[(size_t)k];
    std::vector<uint64_t> done((size_t)n + 1, 0xdeadbeefull);   // one guard word behind the block's n
    const uint64_t total = block_cost(off.data(), n, rm, T, W, W2, done.data());
    if (done[(size_t)n] != 0xdeadbeefull) fault(what, n, 0, (long)done[(size_t)n], 0xdeadbeefl);
    if (n > 0 && done[0] != 0) fault(what, 0, 0, (long)done[0], 0);
    if (n > 1 && done[1] != 0) fault(what, 1, 0, (long)done[1], 0);
    uint64_t sum = 0;
    for (int k = 1; k < n; ++k) {
        if (done[(size_t)k] != sum) fault(what, k, 1, (long)done[(size_t)k], (long)sum);
        if (cost_cols(rm, T, W, W2, len[(size_t)k]) != cols[(size_t)k]) fault(what, k, 2, (long)cost_cols(rm, T, W, W2, len[(size_t)k]), (long)cols[(size_t)k]);
        sum += (uint64_t)(rows_at(len, k) * (double)cols[(size_t)k]);
    }
    if (total != sum) fault(what, n, 3, (long)total, (long)sum);
    if (block_cost(off.data(), n, rm, T, W, W2, nullptr) != total) fault(what, n, 4, 0, 0);
}

int main() {
    // every built packed block class: the width per alignment at the boundary of the second width
    int dual = 0;
    for (int r = 0; r < kNumClasses; ++r) {
        const ClassRow& c = kClasses[r];
        if (c.kind != CLASS_BLOCK || !(c.rms & RM2)) continue;
        for (int W = CLASS_W_MIN; W <= CLASS_W_MAX; ++W) {
            if (!(c.widths & cw(W))) continue;
            const Variant v{W, c.tmax / 64, c.tmax, 2, c.cb};
            const int T = v.T(), W2 = class_w2(c.kind, v, true);
            if (!W2) {
                // no second width: every length the geometry takes sweeps all its columns
                const std::vector<int64_t> len = {(int64_t)T * 2 * W - 1, 1, (int64_t)T * 2 * (W - 1) - 1, (int64_t)T * 2 * W - 1};
                check_block("single width", len, 2, T, W, 0, std::vector<uint64_t>(4, (uint64_t)T * 2 * W));
                continue;
            }
            ++dual;
            const int64_t cap = (int64_t)T * 2 * W2 - 1;   // len + 1 == T * 2 * W2: the longest sequence at W2
            const uint64_t wide = (uint64_t)T * 2 * W, narrow = (uint64_t)T * 2 * W2;
            // the founder long, then: one below the boundary, at it, one above, a short one, the geometry's longest
            const std::vector<int64_t> len = {cap + 1, cap - 1, cap, cap + 1, 7, (int64_t)T * 2 * W - 1};
            check_block("dual width", len, 2, T, W, W2, {0, narrow, narrow, wide, narrow, wide});
            // the same lengths in the class run without its second width (SXG_POA_WIDTH2=0)
            check_block("dual-width class, second width off", len, 2, T, W, 0, std::vector<uint64_t>(6, wide));
            // against the kernel's own expression, every length around the boundary
            for (int64_t l = cap - 2; l <= cap + 2; ++l) {
                const uint64_t want = (W2 != 0 && l + 1 <= (int64_t)T * 2 * W2) ? narrow : wide;
                if (cost_cols(2, T, W, W2, l) != want) fault("kernel's rule", (long)l, W, (long)cost_cols(2, T, W, W2, l), (long)want);
            }
            printf("%d %d %d %ld %lu %lu %lu\n", c.tmax, W, W2, (long)cap, (unsigned long)cost_cols(2, T, W, W2, cap - 1), (unsigned long)cost_cols(2, T, W, W2, cap),
                   (unsigned long)cost_cols(2, T, W, W2, cap + 1));
        }
    }
    // (only the 2-byte classes of four and eight waves, W = 9 .. 12, have a second width: 8 of them)
    if (dual != 8) { fprintf(stderr, "%d dual-width block classes, 8 expected\n", dual); ++bad; }

    // the headline's pair: a W = 10 block costs the same on its own class (W2 = 9 never fits 5 kbp) as merged into the W = 11 class
    {
        const std::vector<int64_t> len = {5000, 4990, 5010, 4800};
        std::vector<int64_t> off = {0};
        for (int64_t l : len) off.push_back(off.back() + l);
        const uint64_t own = block_cost(off.data(), 4, 2, 256, 10, 9, nullptr), merged = block_cost(off.data(), 4, 2, 256, 11, 10, nullptr);
        const uint64_t full = block_cost(off.data(), 4, 2, 256, 11, 0, nullptr);
        if (own != merged) fault("W = 10 block in the W = 11 class", 0, 0, (long)own, (long)merged);
        if (!(full > merged)) fault("W = 11 without its second width costs more", 0, 0, (long)full, (long)merged);
    }

    // banded: 2 * half-width cells per row, half-width = 311 + 3 % of the sequence, capped at 693
    {
        const std::vector<int64_t> len = {3000, 100, 3000, 12733, 20000};
        check_block("banded", len, 3, 64, 11, 0, {0, 2 * (311 + 3), 2 * (311 + 90), 2 * (311 + 381), 2 * 693});
    }
    // 32-bit sweeps: T * W columns whatever the length, a second width is ignored
    {
        const std::vector<int64_t> len = {4000, 10, 4095, 2000};
        check_block("32-bit, int16 rows", len, 0, 256, 16, 0, std::vector<uint64_t>(4, 256 * 16));
        check_block("32-bit, int32 rows", len, 1, 512, 12, 11, std::vector<uint64_t>(4, 512 * 12));
    }
    // degenerate blocks: no sequence, one sequence (nothing is swept)
    check_block("empty block", {}, 2, 256, 11, 10, {});
    check_block("one sequence", {5000}, 2, 256, 11, 10, {0});

    // the deal over CUs.  Block id = its rank by cost (0 = costliest), so work = 0, 1, 2, ... is "sorted by cost, largest first".
    for (const int ncu : {4, 7, 256}) {
        for (const int64_t ns : {(int64_t)ncu + 1, (int64_t)2 * ncu - 1, (int64_t)3 * ncu + ncu / 2, (int64_t)3 * ncu + 232 % ncu}) {
            const int64_t extra = 5;   // blocks beyond the slots: they come from the queue and must not move
            std::vector<int32_t> work((size_t)(ns + extra));
            std::iota(work.begin(), work.end(), 0);
            deal_over_cus(work, ns, ncu);
            const int64_t rem = ns % ncu, full = ns / ncu;
            if (rem == 0) continue;
            std::vector<int> seen((size_t)(ns + extra), 0);
            for (int32_t b : work) if (b < 0 || b >= ns + extra || seen[(size_t)b]++) { fault("deal loses or repeats a block", ncu, (long)ns, b, 0); break; }
            for (int64_t k = ns; k < ns + extra; ++k) if (work[(size_t)k] != k) fault("deal moved a queued block", ncu, (long)ns, work[(size_t)k], (long)k);
            // the light CUs (cu >= rem: `full` workgroups each) hold exactly the (ncu - rem) * full costliest blocks
            const int64_t n_light = (ncu - rem) * full;
            for (int64_t p = 0; p < ns; ++p) {
                const bool light = p % ncu >= rem;
                if (light != (work[(size_t)p] < n_light)) { fault("light CUs do not hold the largest costs", ncu, (long)ns, (long)p, work[(size_t)p]); break; }
            }
            // snake over the crowded CUs: per-CU rank sums differ by less than one round's span
            long lo = -1, hi = -1;
            for (int64_t cu = 0; cu < rem; ++cu) {
                long sum = 0;
                for (int64_t p = cu; p < ns; p += ncu) sum += work[(size_t)p];
                lo = lo < 0 || sum < lo ? sum : lo;
                hi = sum > hi ? sum : hi;
            }
            if (hi - lo > rem) fault("snake order does not even out the crowded CUs", ncu, (long)ns, hi, lo);
        }
        // nothing to deal: slots divide evenly, no CU has a full workgroup, fewer blocks than slots
        for (const int64_t ns : {(int64_t)2 * ncu, (int64_t)ncu - 1}) {
            std::vector<int32_t> work((size_t)ns), same;
            std::iota(work.begin(), work.end(), 0);
            same = work;
            deal_over_cus(work, ns, ncu);
            if (work != same) fault("deal moved blocks with nothing to deal", ncu, (long)ns, 0, 0);
        }
        std::vector<int32_t> few((size_t)ncu), same;
        std::iota(few.begin(), few.end(), 0);
        same = few;
        deal_over_cus(few, 2 * ncu + 1, ncu);
        if (few != same) fault("deal moved blocks of a list shorter than the slots", ncu, 0, 0, 0);
    }
    if (bad) fprintf(stderr, "%d faults\n", bad);
    return bad ? 1 : 0;
}

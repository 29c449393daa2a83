// TEST HARNESS: the deal of a batch over the members of a device group (smoothxg_amd/csrc/poa_deal.h: deal_block_cost, deal_cuts,
// deal_batch) -- what sxg_poa_group_batch_upload cuts the batch by.  Plain C++17, no HIP, no GPU: compile with g++ (the test also
// builds it with -fsanitize=address,undefined).  Never shipped.
//
//   deal_check     fails (exit status 1, reasons on stderr) when, for a random batch and a group of 1 .. 16 members,
//     * a block appears in no member's list or in more than one, or a member's list is not ascending,
//     * two runs over the same batch give different parts,
//     * a member costs more than total / n + the costliest block (checked in integers: cost_m * n <= total + max * n),
//     * the cost of a block is not the sharded deal's: sum over k >= 1 of L_k * (L_0 + 0.05 * sum_{j<k} L_j), truncated.
//   The batches: no blocks, fewer blocks than members, blocks without sequences, blocks that cost nothing (one sequence, or
//   sequences of no letters), one huge block among small ones (first, in the middle, last), and plain random ones.
//   It prints one line per case: name, blocks, and for n = 1, 2, 3, 8, 16 the largest member's share of the total in 1/1000.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_deal.h"

using namespace sxg;

static int bad = 0;
static void fault(const char* what, const char* name, long a, long b) {
    if (++bad <= 20) fprintf(stderr, "%s [%s]: %ld %ld\n", what, name, a, b);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

struct Batch {
    std::vector<int32_t> blk_off{0};
    std::vector<int64_t> seq_off{0};
    void block(const std::vector<int64_t>& lens) {
        for (int64_t l : lens) seq_off.push_back(seq_off.back() + l);
        blk_off.push_back((int32_t)(seq_off.size() - 1));
    }
    void random_block(int max_seqs, int max_len) {
        std::vector<int64_t> lens((size_t)(rnd() % (uint64_t)(max_seqs + 1)));
        for (auto& l : lens) l = (int64_t)(rnd() % (uint64_t)(max_len + 1));
        block(lens);
    }
    int n() const { return (int)blk_off.size() - 1; }
};

// the cost as lpt_partition writes it, independently of the header
static uint64_t cost_ref(const Batch& B, int b) {
    double cost = 0, prev = 0;
    const int s0 = B.blk_off[(size_t)b], s1 = B.blk_off[(size_t)b + 1];
    const double l1 = s1 > s0 ? (double)(B.seq_off[(size_t)s0 + 1] - B.seq_off[(size_t)s0]) : 0.0;
    for (int s = s0; s < s1; ++s) {
        const double len = (double)(B.seq_off[(size_t)s + 1] - B.seq_off[(size_t)s]);
        if (s > s0) cost += len * (l1 + 0.05 * prev);
        prev += len;
    }
    return (uint64_t)cost;
}

static void check(const char* name, const Batch& B) {
    const int nb = B.n();
    printf("%s %d", name, nb);
    for (int n = 1; n <= 16; ++n) {
        std::vector<int32_t> cut(3, -7), again;
        std::vector<uint64_t> cost;
        deal_batch(nb, B.blk_off.data(), B.seq_off.data(), n, cut, &cost);
        deal_batch(nb, B.blk_off.data(), B.seq_off.data(), n, again);
        if (cut != again) fault("two runs differ", name, n, nb);
        if ((int)cut.size() != n + 1 || cut[0] != 0 || cut[(size_t)n] != nb) { fault("cuts do not span the batch", name, n, (long)cut.size()); continue; }
        if ((int)cost.size() != nb) { fault("costs", name, n, (long)cost.size()); continue; }
        unsigned __int128 total = 0;
        uint64_t biggest = 0;
        for (int b = 0; b < nb; ++b) {
            if (cost[(size_t)b] != cost_ref(B, b)) fault("cost of a block", name, b, (long)cost[(size_t)b]);
            total += cost[(size_t)b];
            if (cost[(size_t)b] > biggest) biggest = cost[(size_t)b];
        }
        // the members' lists, written out: every block exactly once, each list ascending
        std::vector<int> seen((size_t)(nb > 0 ? nb : 1), 0);
        unsigned __int128 heaviest = 0;
        for (int m = 0; m < n; ++m) {
            if (cut[(size_t)m + 1] < cut[(size_t)m]) { fault("cuts not monotone", name, n, m); break; }
            std::vector<int32_t> part;
            for (int b = cut[(size_t)m]; b < cut[(size_t)m + 1]; ++b) part.push_back(b);
            unsigned __int128 load = 0;
            for (size_t k = 0; k < part.size(); ++k) {
                if (part[k] < 0 || part[k] >= nb) { fault("block out of range", name, n, part[k]); continue; }
                if (k && part[k] <= part[k - 1]) fault("list not ascending", name, n, m);
                seen[(size_t)part[k]] += 1;
                load += cost[(size_t)part[k]];
            }
            if (load > heaviest) heaviest = load;
        }
        for (int b = 0; b < nb; ++b)
            if (seen[(size_t)b] != 1) fault("block not dealt exactly once", name, n, b);
        if (heaviest * (unsigned)n > total + (unsigned __int128)biggest * (unsigned)n) fault("a member above total / n + the costliest block", name, n, nb);
        if (n == 1 || n == 2 || n == 3 || n == 8 || n == 16) printf(" %ld", total ? (long)(heaviest * 1000 / total) : 0L);
    }
    printf("\n");
}

int main() {
    { Batch B; check("empty", B); }
    { Batch B; for (int k = 0; k < 3; ++k) B.random_block(6, 800); check("fewer-blocks-than-members", B); }
    { Batch B; B.block({300, 310, 290}); check("one-block", B); }
    { Batch B; for (int k = 0; k < 40; ++k) { if (k % 3 == 0) B.block({}); else B.random_block(6, 800); } check("blocks-without-sequences", B); }
    { Batch B; for (int k = 0; k < 25; ++k) B.block({}); check("only-empty-blocks", B); }
    { Batch B; for (int k = 0; k < 30; ++k) { if (k % 2) B.block({(int64_t)(rnd() % 500)}); else B.block({0, 0, 0}); } check("zero-cost-blocks", B); }
    { Batch B; for (int k = 0; k < 30; ++k) { if (k % 4 == 1) B.block({700}); else B.random_block(5, 600); } check("some-zero-cost-blocks", B); }
    for (int where = 0; where < 3; ++where) {
        Batch B;
        for (int k = 0; k < 41; ++k) {
            if (k == where * 20) B.block({26623, 26623, 26000, 25000, 26623, 26623}); else B.random_block(6, 300);
        }
        check(where == 0 ? "huge-block-first" : where == 1 ? "huge-block-middle" : "huge-block-last", B);
    }
    for (int r = 0; r < 40; ++r) {
        Batch B;
        const int nb = (int)(rnd() % 200);
        for (int k = 0; k < nb; ++k) B.random_block(1 + (int)(rnd() % 12), 1 + (int)(rnd() % 3000));
        char name[32];
        snprintf(name, sizeof(name), "random-%d", r);
        check(name, B);
    }
    { Batch B; for (int k = 0; k < 1000; ++k) B.block({1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000}); check("headline-shape", B); }
    if (bad) { fprintf(stderr, "%d faults\n", bad); return 1; }
    return 0;
}

// poa_deal.h -- how a batch of blocks is dealt over the members of a device group (sxg_poa_group, include/sxg_poa.h).
//
// Plain C++17, no HIP: included by the host (sxg_poa.hip: sxg_poa_group_batch_upload) and by the host-only check
// tests/csrc/deal_check.cpp.
//
// The deal is a function of the batch alone: COST-BALANCED CONTIGUOUS CUTS.  A block costs what the sharded run's deal
// (lpt_partition) charges it -- sum over its alignments k >= 1 of L_k * (L_0 + 0.05 * sum_{j<k} L_j), truncated to
// an integer so that everything after it is exact -- and block b, whose blocks in front of it cost P_b of the batch's total C,
// goes to member floor(P_b * n / C) (the last member at most): the prefix sum of the cost is cut at C * k / n, a block belongs
// to the member its START falls to.  Every member therefore runs one slice [cut[m], cut[m + 1]) of the batch -- its dense
// result arrays are slices of the batch's, the reassembly is one copy per array and member -- and carries at most C / n plus
// one block: the blocks that start inside its window cost less than C / n without the last of them.  A batch that costs
// nothing (no block with a second sequence) is dealt by count, block b to member b * n / n_blocks.  A member may be empty: a
// group with more members than blocks, a window that one huge block spans.
#pragma once
#include <stdint.h>

#include <vector>

namespace sxg {

// the cost of block b of a batch (blk_off / seq_off of sxg_poa_batch_in); a block with fewer than two sequences costs nothing
inline uint64_t deal_block_cost(const int32_t* blk_off, const int64_t* seq_off, int b) {
    const int s0 = blk_off[b], s1 = blk_off[b + 1];
    if (s1 - s0 < 2) return 0;
    const double l0 = (double)(seq_off[s0 + 1] - seq_off[s0]);
    double cost = 0, prev = 0;
    for (int s = s0; s < s1; ++s) {
        const double len = (double)(seq_off[s + 1] - seq_off[s]);
        if (s > s0) cost += len * (l0 + 0.05 * prev);
        prev += len;
    }
    return cost < 9.0e18 ? (uint64_t)cost : (uint64_t)9.0e18;
}

// cut[0 .. n]: member m runs the blocks cut[m] .. cut[m + 1] - 1 of the cost.size() blocks; cut[0] = 0, cut[n] = their number
inline void deal_cuts(const std::vector<uint64_t>& cost, int n, std::vector<int32_t>& cut) {
    const int nb = (int)cost.size();
    if (n < 1) n = 1;
    unsigned __int128 total = 0;
    for (uint64_t c : cost) total += c;
    cut.assign((size_t)n + 1, nb);
    cut[0] = 0;
    int m = 0;
    unsigned __int128 before = 0;
    for (int b = 0; b < nb; ++b) {
        unsigned __int128 mb = total ? before * (unsigned)n / total : (unsigned __int128)((uint64_t)b * (uint64_t)n / (uint64_t)nb);
        if (mb > (unsigned)(n - 1)) mb = (unsigned)(n - 1);
        while (m < (int)mb) cut[(size_t)++m] = b;
        before += cost[(size_t)b];
    }
}

inline void deal_batch(int n_blocks, const int32_t* blk_off, const int64_t* seq_off, int n, std::vector<int32_t>& cut, std::vector<uint64_t>* cost_out = nullptr) {
    std::vector<uint64_t> cost((size_t)(n_blocks > 0 ? n_blocks : 0));
    for (int b = 0; b < n_blocks; ++b) cost[(size_t)b] = deal_block_cost(blk_off, seq_off, b);
    deal_cuts(cost, n, cut);
    if (cost_out) cost_out->swap(cost);
}

}  // namespace sxg

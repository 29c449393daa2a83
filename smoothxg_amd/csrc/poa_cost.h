// poa_cost.h -- what a block costs the launch it runs in, in SWEPT COLUMNS, and how a launch's blocks are dealt over the CUs.
//
// Plain C++17, no HIP: included by the host (sxg_poa.hip: the per-launch sort, the deal over CUs, BlockArgs::est / est_done,
// the slot shares of launches that run side by side), by the banded sweep (poa_band16.hip.h: the band's half-width) and by the
// host-only check tests/csrc/block_cost_check.cpp.
//
// Round 14.  Every row of a sweep costs all the columns of the width the sweep runs at, whatever the sequence's length, so the
// unit of work is rows x swept columns: cost = sum over the alignments k >= 1 of rows_k * cols_k.
//   rows_k: the graph's rows when sequence k is aligned -- an ESTIMATE, SURVEY 8(e)'s L_0 + 0.05 * sum_{j<k} L_j;
//   cols_k: EXACT -- the packed sweep's T * 2 * W2 when the class has a second width and the sequence fits it (width_for_len: the
//           test poa_block_kernel makes per sequence), T * 2 * W otherwise; the 32-bit sweeps' T * W, times the tiles of the
//           sequence when the launch sweeps in column tiles (poa_tiles.h: rows x Lpad_total); the banded sweep's band,
//           2 * band_half_width(L_k) cells per row.
// The sweeps report their progress to the priority board in the same unit (rows done x the columns they sweep), and the block
// kernel takes the part of a block that is done from the prefix sums of the same terms (BlockArgs::est_done).
#pragma once
#include <stdint.h>

#include <cstddef>
#include <vector>

#include "poa_classes.h"
#include "poa_tiles.h"

namespace sxg {

constexpr int BAND_WB = 311;        // abpt->wb, src/smooth.cpp:269
constexpr double BAND_WF = 0.03;    // abpt->wf, src/smooth.cpp:271
constexpr int BAND_WMAX = 693;      // decree B1: cap of the half-width -- a band never exceeds the window (2 * 693 / 11 + 2 = 128 strips)
// half-width of the band of a sequence of L letters, in columns (poa_band16.hip.h)
constexpr int band_half_width(int L) { const int w = BAND_WB + (int)(BAND_WF * L); return w < BAND_WMAX ? w : BAND_WMAX; }

// columns (banded: band cells) one row of the alignment of a sequence of `len` letters costs a launch of row mode rm, T threads,
// strip width W and second width W2 (0 = none; only the packed sweep has one); tiles > 1: a 32-bit launch in column tiles
constexpr uint64_t cost_cols(int rm, int T, int W, int W2, int64_t len, int tiles = 1) {
    if (rm == 3) return 2u * (uint64_t)band_half_width((int)len);
    if (rm == 2) return (uint64_t)T * 2u * (uint64_t)width_for_len(W, W2, T, (int)len);
    return (uint64_t)T * (uint64_t)W * (uint64_t)(tiles > 1 ? n_tiles((int)len, T, W) : 1);
}

// Cost of the block whose n sequences have the offsets off[0 .. n] (lengths off[k + 1] - off[k], in alignment order).
// done[k], k = 0 .. n - 1 (nullptr: not wanted), receives the cost of the alignments BEFORE k: done[0] = done[1] = 0 -- the first
// sequence founds the graph and is not swept -- and done[n - 1] + the last term is the returned total.
inline uint64_t block_cost(const int64_t* off, int n, int rm, int T, int W, int W2, uint64_t* done, int tiles = 1) {
    uint64_t total = 0;
    double prev = 0;
    const double l0 = n > 0 ? (double)(off[1] - off[0]) : 0.0;
    for (int k = 0; k < n; ++k) {
        const int64_t len = off[k + 1] - off[k];
        if (done) done[k] = total;
        if (k > 0) total += (uint64_t)((l0 + 0.05 * prev) * (double)cost_cols(rm, T, W, W2, len, tiles));
        prev += (double)len;
    }
    return total;
}

// The deal of a launch's work list over the CUs.  Workgroup p of a launch of ns workgroups runs on CU p mod ncu (measured,
// profiles/tools/slot_report.py): when ns is no multiple of ncu, the CUs with one workgroup less ("light") run theirs faster --
// they get the costliest blocks, so that those are not what the launch ends on; the crowded CUs are dealt the rest in snake
// order (round 0 left to right, round 1 right to left, ...), which evens out the sum of costs per CU.
// work: block ids sorted by cost, largest first; its first ns entries are rearranged so that work[p] is workgroup p's first
// block.  Nothing moves when the slots divide evenly, when no CU has a full workgroup, or when there are fewer blocks than slots.
inline void deal_over_cus(std::vector<int32_t>& work, int64_t ns, int64_t ncu) {
    if (ncu < 1) ncu = 1;
    const int64_t rem = ns % ncu, full = ns / ncu;
    if (rem <= 0 || full < 1 || (int64_t)work.size() < ns) return;
    std::vector<int32_t> first((size_t)ns, -1);
    size_t next = 0;
    for (int64_t p = 0; p < ns; ++p)          // light CUs first
        if (p % ncu >= rem && p / ncu < full) first[(size_t)p] = work[next++];
    for (int64_t round = 0; round <= full; ++round)
        for (int64_t c = 0; c < rem; ++c) {
            const int64_t cu = (round & 1) ? rem - 1 - c : c, p = round * ncu + cu;
            if (p < ns && first[(size_t)p] < 0) first[(size_t)p] = work[next++];
        }
    for (int64_t p = 0; p < ns; ++p) work[(size_t)p] = first[(size_t)p];
}

}  // namespace sxg

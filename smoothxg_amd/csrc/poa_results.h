// poa_results.h -- the result arrays of a batch (sxg_poa_batch_out, include/sxg_poa.h) as ONE table, and what follows from it.
//
// Plain C++17, no HIP: included by the host (sxg_poa.hip: the download of a handle, the blob of a sharded rank, the root's
// assembly, the device group's download) and by the host-only check tests/csrc/results_check.cpp.
//
// Every array of the result is either one of an OFFSET FAMILY -- offsets over the blocks (or the sequences) of the batch plus up
// to three payload arrays that those offsets index -- or FLAT: one entry per block, sequence or base.  The result of a part of
// a batch (a slice a group member ran, the blocks the sharded deal gave a rank) is therefore a set of pieces of the batch's dense
// arrays, and putting the parts together is "rebase the offsets, copy the payloads", driven by the table: reassemble_results.
// The one array that is not copied but computed from others, the full MSA, is formatted by format_full_msa.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/sxg_poa.h"

namespace sxg {

// Fields are addressed by their place in the (standard-layout) struct; every one of them is a data pointer.
struct ResultPayload { size_t field, elem; };                                  // elem = 0: no such payload
struct ResultFamily { size_t off_field; int per_seq; ResultPayload pay[3]; };   // offsets [blocks + 1] (per_seq: [sequences + 1]) and what they index
struct ResultFlat { size_t field, elem; int index; };                          // one entry per block (0), sequence (1) or base (2)
#define SXG_RF(f) offsetof(sxg_poa_batch_out, f)
constexpr ResultFamily RESULT_FAMILIES[] = {
    {SXG_RF(node_off), 0, {{SXG_RF(node_code), 1}, {SXG_RF(node_rank), 4}, {SXG_RF(node_group), 4}}},
    {SXG_RF(edge_off), 0, {{SXG_RF(edge_tail), 4}, {SXG_RF(edge_head), 4}, {SXG_RF(edge_weight), 4}}},
    {SXG_RF(cons_off), 0, {{SXG_RF(cons_nodes), 4}, {0, 0}, {0, 0}}},
    {SXG_RF(msa_off), 0, {{SXG_RF(msa), 1}, {0, 0}, {0, 0}}},
    {SXG_RF(bg_node_off), 0, {{SXG_RF(bg_node_len), 4}, {SXG_RF(bg_node_outdeg), 4}, {SXG_RF(bg_node_indeg), 1}}},
    {SXG_RF(bg_seq_off), 0, {{SXG_RF(bg_seq), 1}, {0, 0}, {0, 0}}},
    {SXG_RF(bg_edge_off), 0, {{SXG_RF(bg_edge_to), 4}, {0, 0}, {0, 0}}},
    {SXG_RF(bg_step_off), 1, {{SXG_RF(bg_steps), 4}, {0, 0}, {0, 0}}},
    {SXG_RF(bg_cons_off), 0, {{SXG_RF(bg_cons_steps), 4}, {0, 0}, {0, 0}}},
};
constexpr ResultFlat RESULT_FLAT[] = {
    {SXG_RF(status), 4, 0}, {SXG_RF(msa_cols), 4, 0}, {SXG_RF(block_cycles), 8, 0},
    {SXG_RF(score), 4, 1}, {SXG_RF(cells), 8, 1}, {SXG_RF(seq_path_nodes), 4, 2},
};
constexpr int N_RESULT_FAMILIES = (int)(sizeof(RESULT_FAMILIES) / sizeof(RESULT_FAMILIES[0]));
constexpr int N_RESULT_FLAT = (int)(sizeof(RESULT_FLAT) / sizeof(RESULT_FLAT[0]));
// the families and flat arrays that code outside the table has to name (the special cases of the download, the full MSA)
enum { RF_NODE = 0, RF_EDGE, RF_CONS, RF_MSA, RF_BG_NODE, RF_BG_SEQ, RF_BG_EDGE, RF_BG_STEP, RF_BG_CONS };

// The table is complete: its entries are distinct pointer fields between the struct's head (n_blocks, n_seqs and their padding,
// in front of `status`) and `_owner`, and there are as many of them as the struct has room for.  A result array added to the
// header without an entry here changes sizeof(sxg_poa_batch_out) and stops the build.
constexpr int result_table_fields(size_t* at) {
    int n = 0;
    for (const ResultFamily& A : RESULT_FAMILIES) {
        at[n++] = A.off_field;
        for (const ResultPayload& P : A.pay)
            if (P.elem) at[n++] = P.field;
    }
    for (const ResultFlat& F : RESULT_FLAT) at[n++] = F.field;
    return n;
}
constexpr bool result_table_sound() {
    size_t at[4 * N_RESULT_FAMILIES + N_RESULT_FLAT] = {};
    const int n = result_table_fields(at);
    for (int i = 0; i < n; ++i) {
        if (at[i] < SXG_RF(status) || at[i] >= SXG_RF(_owner) || at[i] % sizeof(void*)) return false;
        for (int k = 0; k < i; ++k)
            if (at[k] == at[i]) return false;
    }
    return (size_t)n * sizeof(void*) + SXG_RF(status) + sizeof(void*) == sizeof(sxg_poa_batch_out);
}
static_assert(result_table_sound(), "RESULT_FAMILIES / RESULT_FLAT must name every array of sxg_poa_batch_out exactly once");
#undef SXG_RF

inline void* get_field(const sxg_poa_batch_out& o, size_t at) { void* q; memcpy(&q, (const char*)&o + at, sizeof(q)); return q; }
inline void set_field(sxg_poa_batch_out& o, size_t at, void* q) { memcpy((char*)&o + at, &q, sizeof(q)); }

// The shape of a batch: what sxg_poa_batch_in says about it.
struct BatchShape {
    int32_t n_blocks;
    const int32_t* blk_off;   // [n_blocks + 1]
    const int64_t* seq_off;   // [sequences + 1]
    int64_t n_seqs() const { return n_blocks > 0 ? blk_off[n_blocks] : 0; }
    int64_t n_bases() const { return n_seqs() > 0 ? seq_off[n_seqs()] : 0; }
    int64_t count(int index) const { return index == 0 ? n_blocks : index == 1 ? n_seqs() : n_bases(); }
    // where block b starts on that index
    int64_t start(int index, int64_t b) const { return index == 0 ? b : index == 1 ? (n_blocks > 0 ? blk_off[b] : 0) : (n_seqs() > 0 ? seq_off[blk_off[b]] : 0); }
};

// part[k0 .. k1): a maximal run of consecutive block ids
inline size_t consecutive_run_end(const std::vector<int32_t>& part, size_t k0) {
    size_t k1 = k0 + 1;
    while (k1 < part.size() && part[k1] == part[k1 - 1] + 1) ++k1;
    return k1;
}

// Reassembly, first half: parts[p] is the ascending list of the batch's blocks that part p ran, outs[p] that part's result in
// part-local order (pointers may be NULL where the request did not ask for the array, and may point into any memory).  Fills
// `out` (zeroed by the caller but for _owner) with the batch's offsets and with room for every payload and flat array; an
// array is present iff it is present in the first part that has blocks.  alloc(bytes) returns uninitialised memory that the
// caller owns, or NULL: the call then returns false.
template <class Alloc>
bool reassemble_layout(const BatchShape& S, const std::vector<std::vector<int32_t>>& parts, const std::vector<sxg_poa_batch_out>& outs, Alloc alloc,
                       sxg_poa_batch_out* out) {
    out->n_blocks = S.n_blocks; out->n_seqs = S.n_seqs();
    if (parts.empty()) return true;
    size_t first = 0;
    while (first + 1 < parts.size() && parts[first].empty()) ++first;
    if (parts[first].empty()) first = 0;   // (a batch without blocks: every part is empty and they are all alike)
    const sxg_poa_batch_out& T = outs[first];
    for (const ResultFamily& A : RESULT_FAMILIES) {
        if (!get_field(T, A.off_field)) continue;
        const int index = A.per_seq ? 1 : 0;
        const int64_t n = S.count(index);
        int64_t* off = (int64_t*)alloc(8 * (size_t)(n + 1));
        if (!off) return false;
        memset(off, 0, 8 * (size_t)(n + 1));
        // every entry's size from the part that holds it, then the running sum (one pass each over the batch's blocks or
        // sequences: 72 000 entries in all on 1000 blocks of 64 sequences)
        for (size_t p = 0; p < parts.size(); ++p) {
            const int64_t* src = (const int64_t*)get_field(outs[p], A.off_field);
            if (!src) continue;
            for (int32_t b : parts[p])
                for (int64_t j = S.start(index, b), j1 = S.start(index, (int64_t)b + 1); j < j1; ++j, ++src) off[j + 1] = src[1] - src[0];
        }
        for (int64_t j = 0; j < n; ++j) off[j + 1] += off[j];
        set_field(*out, A.off_field, off);
        for (const ResultPayload& P : A.pay) {
            if (!P.elem || !get_field(T, P.field)) continue;
            void* q = alloc((size_t)off[n] * P.elem);
            if (!q) return false;
            set_field(*out, P.field, q);
        }
    }
    for (const ResultFlat& F : RESULT_FLAT) {
        if (!get_field(T, F.field)) continue;
        void* q = alloc((size_t)S.count(F.index) * F.elem);
        if (!q) return false;
        set_field(*out, F.field, q);
    }
    return true;
}

// Reassembly, second half: the payloads and flat arrays of ONE part into their places in `out`, one copy per array and maximal
// run of consecutive block ids (a contiguous slice is one run).  Parts write disjoint ranges: they may be copied side by side.
inline void reassemble_part(const BatchShape& S, const std::vector<int32_t>& part, const sxg_poa_batch_out& M, sxg_poa_batch_out* out) {
    int64_t local[3] = {0, 0, 0};   // where the run starts in the part's own blocks, sequences and bases
    for (size_t k0 = 0; k0 < part.size(); k0 = consecutive_run_end(part, k0)) {
        const size_t k1 = consecutive_run_end(part, k0);
        int64_t j0[3], len[3];
        for (int x = 0; x < 3; ++x) { j0[x] = S.start(x, part[k0]); len[x] = S.start(x, (int64_t)part[k1 - 1] + 1) - j0[x]; }
        for (const ResultFamily& A : RESULT_FAMILIES) {
            const int64_t* dst_off = (const int64_t*)get_field(*out, A.off_field);
            const int64_t* src_off = (const int64_t*)get_field(M, A.off_field);
            if (!dst_off || !src_off) continue;
            const int x = A.per_seq ? 1 : 0;
            const int64_t s0 = src_off[local[x]], bytes = src_off[local[x] + len[x]] - s0, d0 = dst_off[j0[x]];
            for (const ResultPayload& P : A.pay) {
                uint8_t* dst = P.elem ? (uint8_t*)get_field(*out, P.field) : nullptr;
                const uint8_t* src = P.elem ? (const uint8_t*)get_field(M, P.field) : nullptr;
                if (dst && src && bytes) memcpy(dst + (size_t)d0 * P.elem, src + (size_t)s0 * P.elem, (size_t)bytes * P.elem);
            }
        }
        for (const ResultFlat& F : RESULT_FLAT) {
            uint8_t* dst = (uint8_t*)get_field(*out, F.field);
            const uint8_t* src = (const uint8_t*)get_field(M, F.field);
            const int x = F.index;
            if (dst && src && len[x]) memcpy(dst + (size_t)j0[x] * F.elem, src + (size_t)local[x] * F.elem, (size_t)len[x] * F.elem);
        }
        for (int x = 0; x < 3; ++x) local[x] += len[x];
    }
}

template <class Alloc>
bool reassemble_results(const BatchShape& S, const std::vector<std::vector<int32_t>>& parts, const std::vector<sxg_poa_batch_out>& outs, Alloc alloc,
                        sxg_poa_batch_out* out) {
    if (!reassemble_layout(S, parts, outs, alloc, out)) return false;
    for (size_t p = 0; p < parts.size(); ++p) reassemble_part(S, parts[p], outs[p], out);
    return true;
}

// The full MSA (want_msa = SXG_MSA_FULL), decree S8: an MSA column is an aligned group, the columns in rank order; rows = the
// block's sequences (+ the consensus row when want_consensus), a block that failed owns no bytes.  Pure formatting of
// out->status, node_off, node_code, node_rank, node_group, seq_path_nodes (and cons_off, cons_nodes), which must be there;
// fills out->msa_off, msa_cols and msa from alloc (as above).
template <class Alloc>
bool format_full_msa(const BatchShape& S, bool want_consensus, Alloc alloc, sxg_poa_batch_out* out) {
    static const char dec[5] = {'A', 'C', 'G', 'T', 'N'};
    const int nb = S.n_blocks;
    int64_t* msa_off = (int64_t*)alloc(8 * ((size_t)nb + 1));
    int32_t* msa_cols = (int32_t*)alloc(4 * (size_t)nb);
    if (!msa_off || !msa_cols) return false;
    msa_off[0] = 0;
    std::vector<std::vector<int32_t>> cols((size_t)nb);
    for (int b = 0; b < nb; ++b) {
        const int64_t n0 = out->node_off[b];
        const int n = (int)(out->node_off[b + 1] - n0);
        std::vector<int32_t> by_rank((size_t)n);
        for (int v = 0; v < n; ++v) by_rank[(size_t)out->node_rank[n0 + v]] = v;
        cols[(size_t)b].assign((size_t)n, 0);
        int ncol = 0;
        for (int r = 0; r < n; ++r) {
            const int v = by_rank[(size_t)r];
            if (r > 0 && out->node_group[n0 + by_rank[(size_t)r - 1]] == out->node_group[n0 + v]) cols[(size_t)b][(size_t)v] = ncol - 1;
            else cols[(size_t)b][(size_t)v] = ncol++;
        }
        msa_cols[b] = ncol;
        const int rows = (S.blk_off[b + 1] - S.blk_off[b]) + (want_consensus ? 1 : 0);
        msa_off[b + 1] = msa_off[b] + (out->status[b] == SXG_ST_OK ? (int64_t)rows * ncol : 0);
    }
    char* msa = (char*)alloc((size_t)msa_off[nb]);
    if (!msa) return false;
    memset(msa, '-', (size_t)msa_off[nb]);
    for (int b = 0; b < nb; ++b) {
        if (out->status[b] != SXG_ST_OK) continue;
        const int64_t n0 = out->node_off[b];
        const int ncol = msa_cols[b];
        char* base = msa + msa_off[b];
        int row = 0;
        for (int s = S.blk_off[b]; s < S.blk_off[b + 1]; ++s, ++row)
            for (int64_t k = S.seq_off[s]; k < S.seq_off[s + 1]; ++k) {
                const int v = out->seq_path_nodes[k];
                base[(int64_t)row * ncol + cols[(size_t)b][(size_t)v]] = dec[out->node_code[n0 + v]];
            }
        if (want_consensus)
            for (int64_t k = out->cons_off[b]; k < out->cons_off[b + 1]; ++k) {
                const int v = out->cons_nodes[k];
                base[(int64_t)row * ncol + cols[(size_t)b][(size_t)v]] = dec[out->node_code[n0 + v]];
            }
    }
    out->msa_off = msa_off; out->msa_cols = msa_cols; out->msa = msa;
    return true;
}

}  // namespace sxg

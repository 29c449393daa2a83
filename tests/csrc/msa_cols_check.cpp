// msa_cols_check.cpp -- the arithmetic of the trimmed MSA (smoothxg_amd/csrc/poa_msa_cols.h, the HIP-free header the kernels of
// poa_msa.hip.h and the engine's host side include) against a naive restatement, on random small graphs: columns from head flags,
// the kept letters of a row, the kept columns of a block from two reads per row, the spans of a row's chunks, and the split of a
// run of bytes into head, 16-byte groups and tail over every alignment 0..15 and every length 0..40.
// Prints "<checks> <failures>"; built by tests/test_msa_cols.py with the undefined-behaviour and address sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_msa_cols.h"

static long n_checks = 0, n_bad = 0;
static void check(bool ok, const char* what) {
    ++n_checks;
    if (!ok) { if (++n_bad <= 20) fprintf(stderr, "FAIL %s\n", what); }
}

// the reference's trim, letter by letter (src/smooth.cpp:791-812), on a row that holds enough letters
static void naive_blank(std::string& r, int pad) {
    int letters = 0;
    for (char c : r) letters += c != '-';
    if (letters < 2 * pad) { std::fill(r.begin(), r.end(), '-'); return; }
    size_t j = 0;
    for (int left = pad; left > 0; ++j) if (r[j] != '-') { r[j] = '-'; --left; }
    j = r.size();
    for (int left = pad; left > 0;) { --j; if (r[j] != '-') { r[j] = '-'; --left; } }
}

static void split_checks() {
    for (int al = 0; al < 16; ++al)
        for (int n = 0; n <= 40; ++n) {
            int64_t h, b, t;
            sxg_msa_split16((uint64_t)(4096 + al), n, &h, &b, &t);
            check(h >= 0 && b >= 0 && t >= 0 && h + b + t == n, "split: sum");
            check(h < 16 && t < 16 && b % 16 == 0, "split: ranges");
            check(b + t == 0 || (4096 + al + h) % 16 == 0, "split: the body starts on a boundary");
            check(h == std::min<int64_t>(n, (16 - al) % 16), "split: head");
            // written the way the rows kernel writes: bytes, whole groups, bytes -- nothing outside the run
            std::vector<unsigned char> dst(96, 0xee), src(96), want(96, 0xee);
            for (int i = 0; i < 96; ++i) src[(size_t)i] = (unsigned char)(i + 1);
            for (int i = 0; i < n; ++i) want[(size_t)(al + i)] = src[(size_t)(al + i)];
            int64_t x = al;
            for (int64_t i = 0; i < h; ++i, ++x) dst[(size_t)x] = src[(size_t)x];
            for (int64_t i = 0; i < b; i += 16, x += 16) { check(x % 16 == 0, "split: group alignment"); memcpy(&dst[(size_t)x], &src[(size_t)x], 16); }
            for (int64_t i = 0; i < t; ++i, ++x) dst[(size_t)x] = src[(size_t)x];
            check(dst == want, "split: bytes");
        }
}

int main() {
    std::mt19937_64 rng(20260519);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint64_t)(hi - lo + 1)); };
    split_checks();
    for (int trial = 0; trial < 4000; ++trial) {
        // a graph: ncol columns of 1..3 aligned nodes each; node ids shuffled; ranks follow the columns; group = a node id of the column
        const int ncol = rnd(1, 40);
        std::vector<int> col_of_slot;
        for (int c = 0; c < ncol; ++c) for (int k = rnd(1, 3); k > 0; --k) col_of_slot.push_back(c);
        const int n = (int)col_of_slot.size();
        std::vector<int> id_of_slot((size_t)n);
        for (int i = 0; i < n; ++i) id_of_slot[(size_t)i] = i;
        std::shuffle(id_of_slot.begin(), id_of_slot.end(), rng);
        std::vector<int32_t> rank((size_t)n), group((size_t)n);
        std::vector<char> letter((size_t)n);
        for (int s = 0, first = 0; s < n; ++s) {
            if (s > 0 && col_of_slot[(size_t)s] != col_of_slot[(size_t)s - 1]) first = s;
            rank[(size_t)id_of_slot[(size_t)s]] = s;
            group[(size_t)id_of_slot[(size_t)s]] = id_of_slot[(size_t)first];
            letter[(size_t)id_of_slot[(size_t)s]] = "ACGTN"[rnd(0, 4)];
        }
        // columns: the naive loop of the host formatter against head flags + prefix sum
        std::vector<int32_t> by_rank((size_t)n), naive_col((size_t)n), col((size_t)n), tmp((size_t)n);
        for (int v = 0; v < n; ++v) by_rank[(size_t)rank[(size_t)v]] = v;
        int nc = 0;
        for (int r = 0; r < n; ++r) {
            const int v = by_rank[(size_t)r];
            if (r > 0 && group[(size_t)by_rank[(size_t)r - 1]] == group[(size_t)v]) naive_col[(size_t)v] = nc - 1; else naive_col[(size_t)v] = nc++;
        }
        for (int v = 0; v < n; ++v) tmp[(size_t)rank[(size_t)v]] = group[(size_t)v];
        for (int r = 0, run = 0; r < n; ++r) { run += sxg_msa_head(r, r ? tmp[(size_t)r - 1] : 0, tmp[(size_t)r]); by_rank[(size_t)r] = run - 1; }
        for (int v = 0; v < n; ++v) col[(size_t)v] = by_rank[(size_t)rank[(size_t)v]];
        check(col == naive_col && nc == ncol, "columns");
        // rows: every row takes one node of some of the columns, in column order
        const int nrows = rnd(1, 6), pad = rnd(0, 9) < 3 ? 0 : rnd(1, 12);
        std::vector<std::vector<int>> rows((size_t)nrows);
        std::vector<std::vector<int>> nodes_of_col((size_t)ncol);
        for (int v = 0; v < n; ++v) nodes_of_col[(size_t)col[(size_t)v]].push_back(v);
        const int dens = rnd(1, 10);
        for (auto& row : rows)
            for (int c = 0; c < ncol; ++c)
                if (rnd(0, 9) < dens) row.push_back(nodes_of_col[(size_t)c][(size_t)rnd(0, (int)nodes_of_col[(size_t)c].size() - 1)]);
        std::vector<std::string> full((size_t)nrows, std::string((size_t)ncol, '-'));
        for (int r = 0; r < nrows; ++r) for (int v : rows[(size_t)r]) full[(size_t)r][(size_t)col[(size_t)v]] = letter[(size_t)v];
        for (auto& r : full) naive_blank(r, pad);
        int nb0 = 0, ne0 = ncol;
        auto has = [&](int c) { for (auto& r : full) if (r[(size_t)c] != '-') return true; return false; };
        while (nb0 < ncol && !has(nb0)) ++nb0;
        while (ne0 > 0 && !has(ne0 - 1)) --ne0;
        if (nb0 >= ne0) { nb0 = 0; ne0 = 0; }
        // the header's way: two reads per row
        int b0 = 0x7fffffff, e0m = -1;
        for (int r = 0; r < nrows; ++r) {
            int64_t k0, k1;
            sxg_msa_kept((int64_t)rows[(size_t)r].size(), pad, &k0, &k1);
            check(k0 <= k1 && k1 - k0 == std::max<int64_t>(0, (int64_t)rows[(size_t)r].size() - 2 * pad), "kept range");
            if (k1 <= k0) continue;
            b0 = std::min(b0, (int)col[(size_t)rows[(size_t)r][(size_t)k0]]);
            e0m = std::max(e0m, (int)col[(size_t)rows[(size_t)r][(size_t)k1 - 1]]);
        }
        const int e0 = e0m < 0 ? 0 : e0m + 1;
        if (e0m < 0) b0 = 0;
        check(b0 == nb0 && e0 == ne0, "kept columns");
        if (e0 <= b0) continue;
        // every row rebuilt from the spans of its chunks, for several chunk sizes
        for (int chunk : {1, 2, 3, 7, 64}) {
            for (int r = 0; r < nrows; ++r) {
                const std::vector<int>& row = rows[(size_t)r];
                int64_t k0, k1;
                sxg_msa_kept((int64_t)row.size(), pad, &k0, &k1);
                std::string built((size_t)(e0 - b0), '?');
                int at = b0;   // spans must follow one another
                const int64_t nch = sxg_msa_chunks(k0, k1, chunk);
                for (int64_t c = 0; c < nch; ++c) {
                    int64_t a, z;
                    sxg_msa_chunk_letters(k0, k1, c, chunk, &a, &z);
                    check(a <= z && z - a <= chunk && (k1 <= k0 || a < z), "chunk letters");
                    int32_t s, e;
                    sxg_msa_span(k0, k1, a, z, b0, e0, a > k0 && a < k1 ? col[(size_t)row[(size_t)a]] : -777, z < k1 ? col[(size_t)row[(size_t)z]] : -777, &s, &e);
                    check(s == at && e >= s && e <= e0, "span order");
                    at = e;
                    for (int x = s; x < e; ++x) built[(size_t)(x - b0)] = '-';
                    for (int64_t k = a; k < z; ++k) {
                        const int cc = col[(size_t)row[(size_t)k]];
                        check(cc >= s && cc < e, "letter inside its span");
                        if (cc >= s && cc < e) built[(size_t)(cc - b0)] = letter[(size_t)row[(size_t)k]];
                    }
                }
                check(at == e0, "spans cover the row");
                check(built == full[(size_t)r].substr((size_t)b0, (size_t)(e0 - b0)), "row text");
            }
        }
    }
    printf("%ld %ld\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}

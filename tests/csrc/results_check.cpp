// TEST HARNESS: the table of the result arrays and the reassembly of a batch's result from its parts
// (smoothxg_amd/csrc/poa_results.h: RESULT_FAMILIES / RESULT_FLAT, reassemble_results, format_full_msa) -- what the download of
// a device group and the root of a sharded run put results together with.  Plain C++17, no HIP, no GPU: compile with g++ (the
// test also builds it with -fsanitize=address,undefined).  Never shipped.
//
//   results_check   builds a random whole result for a random batch shape (every array of its own exact size, so that the
//   sanitizers see a read or write past any of them), cuts it into the results of parts -- block by block, without the header's
//   runs --, reassembles them and fails (exit status 1, reasons on stderr) when an array that the whole has is missing, differs in
//   a byte, or one that the whole lacks is there.  The cases: contiguous slices for 1, 2, 3 and 16 parts; interleaved ascending
//   parts as a longest-first deal leaves them (runs of one block and longer); a part without blocks in the middle; fewer blocks
//   than parts; blocks without sequences; a batch without blocks; each optional group of arrays absent in turn; parts without
//   blocks, the first among them, whose results hold no array at all.
//   It prints one line per case: name, blocks, sequences, parts, runs, arrays and bytes compared; then the rows of the full MSA of two small
//   hand-made blocks (and a failed one between them), which are also compared with the rows written down here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../smoothxg_amd/csrc/poa_results.h"

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
    void block(int n_seqs, int max_len) {
        for (int s = 0; s < n_seqs; ++s) seq_off.push_back(seq_off.back() + (int64_t)(rnd() % (uint64_t)(max_len + 1)));
        blk_off.push_back((int32_t)(seq_off.size() - 1));
    }
    BatchShape shape() const { return BatchShape{(int32_t)blk_off.size() - 1, blk_off.data(), seq_off.data()}; }
};

// a result whose arrays are allocations of exactly their size
struct Res {
    sxg_poa_batch_out o;
    std::vector<std::unique_ptr<uint8_t[]>> mem;
    Res() { memset(&o, 0, sizeof(o)); }
    void* take(size_t bytes) { mem.emplace_back(new uint8_t[bytes]); return mem.back().get(); }
    void* put(size_t field, const std::vector<uint8_t>& bytes) {
        void* q = take(bytes.size());
        if (!bytes.empty()) memcpy(q, bytes.data(), bytes.size());
        set_field(o, field, q);
        return q;
    }
};

// the optional groups of arrays
enum { DROP_NONE, DROP_CONSENSUS, DROP_MSA, DROP_BLOCK_GRAPHS, DROP_PATHS, DROP_RAW_GRAPHS, DROP_BLOCK_CYCLES, DROP_N };
#define AT(f) offsetof(sxg_poa_batch_out, f)
static bool dropped(size_t field, int drop) {
    const size_t cons[] = {AT(cons_off), AT(cons_nodes), AT(bg_cons_off), AT(bg_cons_steps)};
    const size_t msa[] = {AT(msa_off), AT(msa_cols), AT(msa)};
    const size_t raw[] = {AT(node_code), AT(node_rank), AT(node_group), AT(edge_tail), AT(edge_head), AT(edge_weight), AT(cons_nodes)};
    auto in = [&](const size_t* v, size_t n) { for (size_t i = 0; i < n; ++i) if (v[i] == field) return true; return false; };
    switch (drop) {
    case DROP_CONSENSUS: return in(cons, 4);
    case DROP_MSA: return in(msa, 3);
    case DROP_BLOCK_GRAPHS: return field >= AT(bg_node_off) && field <= AT(bg_cons_steps);
    case DROP_PATHS: return field == AT(seq_path_nodes);
    case DROP_RAW_GRAPHS: return in(raw, 7);
    case DROP_BLOCK_CYCLES: return field == AT(block_cycles);
    default: return false;
    }
}

static std::vector<uint8_t> random_bytes(size_t n) {
    std::vector<uint8_t> v(n);
    for (auto& x : v) x = (uint8_t)rnd();
    return v;
}

static void make_whole(const BatchShape& S, int drop, Res& W) {
    W.o.n_blocks = S.n_blocks; W.o.n_seqs = S.n_seqs();
    for (const ResultFamily& A : RESULT_FAMILIES) {
        if (dropped(A.off_field, drop)) continue;
        const int64_t n = S.count(A.per_seq ? 1 : 0);
        std::vector<int64_t> off((size_t)n + 1, 0);
        for (int64_t j = 0; j < n; ++j) off[(size_t)j + 1] = off[(size_t)j] + (rnd() % 4 == 0 ? 0 : (int64_t)(rnd() % 40));
        std::vector<uint8_t> raw(8 * off.size());
        memcpy(raw.data(), off.data(), raw.size());
        W.put(A.off_field, raw);
        for (const ResultPayload& P : A.pay)
            if (P.elem && !dropped(P.field, drop)) W.put(P.field, random_bytes((size_t)off[(size_t)n] * P.elem));
    }
    for (const ResultFlat& F : RESULT_FLAT)
        if (!dropped(F.field, drop)) W.put(F.field, random_bytes((size_t)S.count(F.index) * F.elem));
}

// where block b starts among the blocks (0), sequences (1) or bases (2), read off the batch's own arrays
static int64_t at(const BatchShape& S, int x, int64_t b) {
    if (x == 0) return b;
    const int64_t s = S.blk_off[b];
    return x == 1 ? s : S.seq_off[s];
}

// the result of the part that ran the blocks `ids`, cut out of the whole one block at a time
static void cut_part(const BatchShape& S, const Res& W, const std::vector<int32_t>& ids, Res& P) {
    P.o.n_blocks = (int32_t)ids.size();
    for (const ResultFamily& A : RESULT_FAMILIES) {
        const int64_t* woff = (const int64_t*)get_field(W.o, A.off_field);
        if (!woff) continue;
        const int x = A.per_seq ? 1 : 0;
        std::vector<int64_t> off{0};
        std::vector<uint8_t> pay[3];
        for (int32_t b : ids)
            for (int64_t j = at(S, x, b); j < at(S, x, b + 1); ++j) {
                off.push_back(off.back() + woff[j + 1] - woff[j]);
                for (int p = 0; p < 3; ++p) {
                    const uint8_t* src = A.pay[p].elem ? (const uint8_t*)get_field(W.o, A.pay[p].field) : nullptr;
                    if (src) pay[p].insert(pay[p].end(), src + woff[j] * (int64_t)A.pay[p].elem, src + woff[j + 1] * (int64_t)A.pay[p].elem);
                }
            }
        if (x == 1) P.o.n_seqs = (int64_t)off.size() - 1;
        std::vector<uint8_t> raw(8 * off.size());
        memcpy(raw.data(), off.data(), raw.size());
        P.put(A.off_field, raw);
        for (int p = 0; p < 3; ++p)
            if (A.pay[p].elem && get_field(W.o, A.pay[p].field)) P.put(A.pay[p].field, pay[p]);
    }
    for (const ResultFlat& F : RESULT_FLAT) {
        const uint8_t* src = (const uint8_t*)get_field(W.o, F.field);
        if (!src) continue;
        std::vector<uint8_t> v;
        for (int32_t b : ids) v.insert(v.end(), src + at(S, F.index, b) * (int64_t)F.elem, src + at(S, F.index, b + 1) * (int64_t)F.elem);
        P.put(F.field, v);
    }
}

// null_empty: a part without blocks hands in a result without any array (a rank that had nothing to run and built nothing)
static void check(const char* name, const Batch& B, const std::vector<std::vector<int32_t>>& parts, int drop = DROP_NONE, bool null_empty = false) {
    const BatchShape S = B.shape();
    Res W;
    make_whole(S, drop, W);
    std::vector<Res> cut(parts.size());
    std::vector<sxg_poa_batch_out> outs;
    long runs = 0;
    for (size_t p = 0; p < parts.size(); ++p) {
        if (!(null_empty && parts[p].empty())) cut_part(S, W, parts[p], cut[p]);
        outs.push_back(cut[p].o);
        for (size_t k = 0; k < parts[p].size(); k = consecutive_run_end(parts[p], k)) ++runs;
    }
    Res G;
    if (!reassemble_results(S, parts, outs, [&](size_t bytes) { return G.take(bytes); }, &G.o)) fault("allocation", name, 0, 0);
    if (G.o.n_blocks != S.n_blocks || G.o.n_seqs != S.n_seqs()) fault("shape", name, G.o.n_blocks, (long)G.o.n_seqs);
    long bytes = 0, arrays = 0;
    auto same = [&](size_t field, size_t n) {
        const void* w = get_field(W.o, field);
        const void* g = get_field(G.o, field);
        if (!w != !g) { fault(w ? "an array is missing" : "an array that nobody asked for", name, (long)field, 0); return; }
        if (w && n && memcmp(w, g, n)) fault("an array differs", name, (long)field, (long)n);
        if (w) { bytes += (long)n; ++arrays; }
    };
    for (const ResultFamily& A : RESULT_FAMILIES) {
        const int64_t n = S.count(A.per_seq ? 1 : 0);
        same(A.off_field, 8 * (size_t)(n + 1));
        const int64_t* off = (const int64_t*)get_field(W.o, A.off_field);
        for (const ResultPayload& P : A.pay)
            if (P.elem) same(P.field, off ? (size_t)off[n] * P.elem : 0);
    }
    for (const ResultFlat& F : RESULT_FLAT) same(F.field, (size_t)S.count(F.index) * F.elem);
    printf("%s %d %ld %d %ld %ld %ld\n", name, S.n_blocks, (long)S.n_seqs(), (int)parts.size(), runs, arrays, bytes);
}

static std::vector<std::vector<int32_t>> slices(int nb, int n) {
    std::vector<std::vector<int32_t>> parts((size_t)n);
    for (int b = 0; b < nb; ++b) parts[(size_t)((int64_t)b * n / nb)].push_back(b);
    return parts;
}
// ascending lists with runs of 1 .. 4 consecutive blocks, as blocks dealt longest first onto the least loaded rank end up
static std::vector<std::vector<int32_t>> interleaved(int nb, int n) {
    std::vector<std::vector<int32_t>> parts((size_t)n);
    for (int b = 0; b < nb;) {
        const size_t p = (size_t)(rnd() % (uint64_t)n);
        for (int len = 1 + (int)(rnd() % 4); len > 0 && b < nb; --len) parts[p].push_back(b++);
    }
    return parts;
}

static Batch random_batch(int nb, int max_seqs, int max_len, int empty_every = 0) {
    Batch B;
    for (int b = 0; b < nb; ++b) B.block(empty_every && b % empty_every == 1 ? 0 : (int)(rnd() % (uint64_t)(max_seqs + 1)), max_len);
    return B;
}

// ---- the full MSA: block 0 = ACGT, AGT (consensus A G T); block 1 failed; block 2 = ACT, AGT, AT with C and G aligned
static void check_msa(bool want_consensus, const std::vector<std::string>& expect) {
    const int32_t blk_off[] = {0, 2, 3, 6};
    const int64_t seq_off[] = {0, 4, 7, 9, 12, 15, 17};
    int32_t status[] = {SXG_ST_OK, SXG_ST_TOO_LONG, SXG_ST_OK};
    int64_t node_off[] = {0, 4, 4, 8};
    uint8_t node_code[] = {0, 1, 2, 3, /* block 2: A C T G */ 0, 1, 3, 2};
    int32_t node_rank[] = {0, 1, 2, 3, 0, 1, 3, 2};
    int32_t node_group[] = {0, 1, 2, 3, 0, 1, 2, 1};
    int32_t paths[] = {0, 1, 2, 3, 0, 2, 3, /* failed */ 0, 0, /* block 2 */ 0, 1, 2, 0, 3, 2, 0, 2};
    int64_t cons_off[] = {0, 3, 3, 6};
    int32_t cons_nodes[] = {0, 2, 3, 0, 1, 2};
    Res G;
    G.o.n_blocks = 3; G.o.n_seqs = 6;
    G.o.status = status; G.o.node_off = node_off; G.o.node_code = node_code; G.o.node_rank = node_rank; G.o.node_group = node_group;
    G.o.seq_path_nodes = paths;
    if (want_consensus) { G.o.cons_off = cons_off; G.o.cons_nodes = cons_nodes; }
    const BatchShape S{3, blk_off, seq_off};
    if (!format_full_msa(S, want_consensus, [&](size_t bytes) { return G.take(bytes); }, &G.o)) { fault("allocation", "msa", 0, 0); return; }
    std::vector<std::string> rows;
    for (int b = 0; b < 3; ++b) {
        const int n_rows = blk_off[b + 1] - blk_off[b] + (want_consensus ? 1 : 0), ncol = G.o.msa_cols[b];
        const int64_t bytes = G.o.msa_off[b + 1] - G.o.msa_off[b];
        if (bytes != (status[b] == SXG_ST_OK ? (int64_t)n_rows * ncol : 0)) fault("bytes of a block's MSA", "msa", b, (long)bytes);
        for (int r = 0; bytes && r < n_rows; ++r) rows.emplace_back(G.o.msa + G.o.msa_off[b] + (int64_t)r * ncol, (size_t)ncol);
    }
    printf("msa consensus=%d", (int)want_consensus);
    for (const std::string& r : rows) printf(" %s", r.c_str());
    printf("\n");
    if (rows != expect) fault("the rows of the full MSA", "msa", (long)rows.size(), (long)expect.size());
}

int main() {
    const Batch base = random_batch(37, 6, 300);
    for (int n : {1, 2, 3, 16}) check(("slices-" + std::to_string(n)).c_str(), base, slices(37, n));
    for (int n : {2, 3, 5, 8}) check(("interleaved-" + std::to_string(n)).c_str(), base, interleaved(37, n));
    { auto parts = slices(37, 3); parts[2].insert(parts[2].begin(), parts[1].begin(), parts[1].end()); parts[1].clear(); check("empty-part-in-the-middle", base, parts); }
    { auto parts = interleaved(37, 4); parts.insert(parts.begin(), std::vector<int32_t>()); check("empty-part-first", base, parts); }
    { auto parts = interleaved(37, 4); parts.insert(parts.begin(), std::vector<int32_t>()); parts.insert(parts.begin() + 3, std::vector<int32_t>());
      check("empty-parts-without-arrays", base, parts, DROP_NONE, true); check("empty-parts-without-arrays-or-block-graphs", base, parts, DROP_BLOCK_GRAPHS, true); }
    { const Batch B = random_batch(2, 5, 200); check("fewer-blocks-than-parts", B, slices(2, 5)); check("fewer-blocks-than-parts-interleaved", B, {{1}, {}, {0}, {}}); }
    { const Batch B = random_batch(40, 5, 200, 3); check("blocks-without-sequences", B, slices(40, 4)); check("blocks-without-sequences-interleaved", B, interleaved(40, 4)); }
    { Batch B; for (int k = 0; k < 9; ++k) B.block(0, 0); check("only-empty-blocks", B, interleaved(9, 3)); }
    { Batch B; for (int k = 0; k < 9; ++k) B.block(3, 0); check("sequences-without-letters", B, interleaved(9, 3)); }
    { Batch B; check("no-blocks", B, {{}, {}, {}}); check("no-blocks-one-part", B, {{}}); }
    const char* drops[DROP_N] = {"", "consensus", "msa", "block-graphs", "paths", "raw-graphs", "block-cycles"};
    for (int d = 1; d < DROP_N; ++d) {
        check((std::string("without-") + drops[d] + "-slices").c_str(), base, slices(37, 3), d);
        check((std::string("without-") + drops[d] + "-interleaved").c_str(), base, interleaved(37, 3), d);
    }
    for (int r = 0; r < 30; ++r) {
        const int nb = 1 + (int)(rnd() % 120), n = 1 + (int)(rnd() % 16);
        const Batch B = random_batch(nb, 1 + (int)(rnd() % 8), 1 + (int)(rnd() % 500), (int)(rnd() % 5));
        check(("random-" + std::to_string(r)).c_str(), B, r % 2 ? interleaved(nb, n) : slices(nb, n), (int)(rnd() % DROP_N));
    }
    check_msa(true, {"ACGT", "A-GT", "A-GT", "ACT", "AGT", "A-T", "ACT"});
    check_msa(false, {"ACGT", "A-GT", "ACT", "AGT", "A-T"});
    if (bad) { fprintf(stderr, "%d faults\n", bad); return 1; }
    return 0;
}

// graph_emul_ids.cpp -- TEST HARNESS ONLY (built by tests/test_graph_emul_ids.py into a temporary directory).  The product's
// graph code (smoothxg_amd/csrc/poa_graph_dev.h) on the host with a one-thread context, driven by the oracle's DP:
// add_alignment with the id rule of decree S6' (mode | SXG_IDS_SPOA) followed by the re-sort of decree S7', so that the rule can be
// checked against tests/spoa_ids_ref.py without a GPU.  The sibling of graph_emul.cpp, which stays as it is.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../smoothxg_amd/csrc/poa_graph_dev.h"
#include "../../oracle/poa_oracle.h"

using namespace sxg;

namespace {
struct OneThread {
    static constexpr int GB = 4, GBH = 4, SCAN_K = 4;
    int tid() const { return 0; }
    int nthreads() const { return 1; }
    void sync() {}
    int scan_excl_add(int v, int* total) { *total = v; return 0; }
    int scan_excl_max(int v, int* total) { *total = v; return -0x7fffffff; }
    int reduce_max(int v) { return v; }
    int atomic_add(int32_t* p, int v) { const int o = *p; *p += v; return o; }
    int atomic_min(int32_t* p, int v) { const int o = *p; if (v < o) *p = v; return o; }
    int load_fresh(const int32_t* p) { return *p; }
    int hp[4];
    int* heap() { return hp; }
    int heap_cap() { return 4; }
};
}  // namespace

// storage: how the re-sort keeps its per-node words and what it keeps between two re-sorts, as graph_emul.cpp's spoa_order --
//   1: on the chip only while the graph is below 16 nodes, else in the slot's scratch; no static chain named
//   2: always on the chip, the block's first sequence named as the static chain
//   4: as 2, every re-sort builds everything
// ids_spoa: the caller's mode & SXG_IDS_SPOA; as in the kernel, the rule applies to local alignments only.
extern "C" int emul_ids_block_run(const uint8_t* bases, const int32_t* seq_off, int n_seqs, const uint32_t* weights, const poa_params_t* p,
                                  int storage, int ids_spoa, int32_t* out_counts /* n_nodes, n_edges */, uint8_t* code, int32_t* rank,
                                  int32_t* leader, int32_t* e_tail, int32_t* e_head, uint32_t* e_w, int32_t* paths, int32_t* scores) {
    int64_t cap = 1;
    for (int s = 0; s < n_seqs; ++s) cap += seq_off[s + 1] - seq_off[s];
    const size_t C = (size_t)cap + 2;
    std::vector<std::vector<int32_t>> a(26, std::vector<int32_t>(C));
    std::vector<int32_t> hdr(2, 0), gm(5 * C), dfs(8 * C + 8), drec(16 * C + 16);
    std::vector<uint8_t> words(4 * C + 64), cd(C);
    std::vector<uint32_t> ew(C);
    std::vector<int8_t> kd(C);
    GraphView G;
    G.n_nodes = &hdr[0]; G.n_edges = &hdr[1]; G.code = cd.data(); G.rank = a[0].data(); G.order = a[1].data(); G.order_tmp = a[2].data();
    G.leader = a[3].data(); G.gmem = gm.data(); G.in_head = a[4].data(); G.in_tail = a[5].data(); G.out_head = a[6].data();
    G.out_tail = a[7].data(); G.in_deg = a[8].data(); G.out_deg = a[9].data(); G.e_tail = a[10].data(); G.e_head = a[11].data();
    G.e_next_in = a[12].data(); G.e_next_out = a[13].data(); G.e_w = ew.data(); G.posnode = a[14].data(); G.target = a[15].data();
    G.newidx = a[16].data(); G.nexta = a[17].data(); G.preva = a[18].data(); G.slotadd = a[19].data(); G.kind = kd.data();
    G.xpos = a[20].data(); G.via = a[21].data(); G.dfs_stack = dfs.data(); G.dfs_rec = drec.data(); G.sp_rank = a[22].data();
    G.sp_first = a[23].data(); G.sp_cnt = a[24].data();
    std::vector<uint8_t> rcode(C), rflags(C), sink(C);
    std::vector<int32_t> poff(C + 1), preds(C), slot(C), tbx(C), sseq(C + 1), rnode(C), meta(8 * C), an(2 * C), ap(2 * C);
    RowsView R{rcode.data(), rflags.data(), poff.data(), preds.data(), slot.data(), tbx.data(), sseq.data(), rnode.data(), meta.data()};
    RowCaps caps{(int)C, (int)C, (int)C};
    OneThread c;
    const bool local = (p->mode & 1) == 0;
    for (int s = 0; s < n_seqs; ++s) {
        const uint8_t* seq = bases + seq_off[s];
        const int len = seq_off[s + 1] - seq_off[s];
        for (int i = 0; i < len; ++i) G.posnode[i] = -1;
        int32_t sc = 0;
        if (hdr[0] > 0 && len > 0) {
            const int st = prep_rows(c, G, R, caps);
            if (st != ST_OK) return st;
            for (int r = 0; r < hdr[0]; ++r) sink[r] = (rflags[r] & ROW_SINK) ? 1 : 0;
            const int n = poa_align_csr(hdr[0], rcode.data(), poff.data(), preds.data(), sink.data(), seq, len, p, an.data(), ap.data(), &sc);
            for (int k = 0; k < n; ++k)
                if (an[k] >= 0 && ap[k] >= 0) G.posnode[ap[k]] = rnode[an[k]];
        }
        scores[s] = sc;
        const int n_before = hdr[0];
        add_alignment(c, G, seq, len, weights ? weights[s] : 1u, paths + seq_off[s], false, ids_spoa != 0 && local);
        spoa_resort(c, G, words.data(), storage == 1 ? 64 : (int)words.size(), storage == 1 ? 0 : seq_off[1] - seq_off[0], len, n_before,
                    s == 0 || storage == 4);
    }
    out_counts[0] = hdr[0]; out_counts[1] = hdr[1];
    memcpy(code, cd.data(), (size_t)hdr[0]);
    memcpy(rank, G.rank, 4 * (size_t)hdr[0]);
    memcpy(leader, G.leader, 4 * (size_t)hdr[0]);
    memcpy(e_tail, G.e_tail, 4 * (size_t)hdr[1]);
    memcpy(e_head, G.e_head, 4 * (size_t)hdr[1]);
    memcpy(e_w, ew.data(), 4 * (size_t)hdr[1]);
    return 0;
}

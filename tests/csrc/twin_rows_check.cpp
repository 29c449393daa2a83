// twin_rows_check.cpp -- TEST HARNESS ONLY.  The product's row preparation (smoothxg_amd/csrc/poa_graph_dev.h) compiled for the
// host with a one-thread context, as graph_emul.cpp does, driven by the oracle's DP: after every sequence of a block the rows
// the packed sweep would get -- with the twin step's trait (prep_rows_twin) or without it (prep_rows) -- are handed out.
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../smoothxg_amd/csrc/poa_graph_dev.h"
#include "../../oracle/poa_oracle.h"

using namespace sxg;

struct SerialCtx {
    static constexpr int GB = 4, GBH = 4, SCAN_K = 4;
    int tid() const { return 0; }
    int nthreads() const { return 1; }
    void sync() {}
    int scan_excl_add(int v, int* total) { *total = v; return 0; }
    int scan_excl_max(int v, int* total) { *total = v; return -0x7fffffff; }
    int reduce_max(int v) { return v; }
    int atomic_add(int32_t* p, int v) { int o = *p; *p += v; return o; }
    int atomic_min(int32_t* p, int v) { int o = *p; if (v < o) *p = v; return o; }
    int load_fresh(const int32_t* p) { return *p; }
    std::vector<int> hp = std::vector<int>(64);
    int* heap() { return hp.data(); }
    int heap_cap() { return (int)hp.size(); }
};

// trait: 1 = prep_rows_twin(..., twin_on), 0 = prep_rows.  Per alignment s = 1 .. n_seqs - 1 (graph of the first s sequences):
// n_rows[s], and at row_base[s] (rows) / pred_base[s] (predecessors) the flags, slots, pred_off (n + 1 entries at
// row_base[s] + s: one spare per graph) and preds.  Returns 0, or the status prep returned.
extern "C" int twin_rows_run(const uint8_t* bases, const int32_t* seq_off, int n_seqs, const poa_params_t* p, int pool_slots, int lds_rows,
                             int trait, int twin_on, int32_t* n_rows, int64_t* row_base, int64_t* pred_base, uint8_t* flags_out,
                             int32_t* slot_out, int32_t* off_out, int32_t* pred_out) {
    int64_t cap = 1;
    for (int s = 0; s < n_seqs; ++s) cap += seq_off[s + 1] - seq_off[s];
    const size_t C = (size_t)cap + 2;
    std::vector<int32_t> hdr(2, 0), rk(C), ord(C), ordt(C), ld(C), gm(5 * C), ih(C), it(C), oh(C), ot(C),
        id(C), od(C), et(C), eh(C), eni(C), eno(C), posn(C), tgt(C), nidx(C), nxa(C), pva(C), sla(C), xps(C);
    std::vector<int32_t> via(C), dfs(8 * C + 8), drec(16 * C + 16), sprank(C), spfirst(C), spcnt(C);
    std::vector<uint8_t> lst(4 * C + 64);
    std::vector<uint32_t> ew(C);
    std::vector<uint8_t> cd(C);
    std::vector<int8_t> kd(C);
    GraphView G{&hdr[0], &hdr[1], cd.data(), rk.data(), ord.data(), ordt.data(), ld.data(), gm.data(),
                ih.data(), it.data(), oh.data(), ot.data(), id.data(), od.data(), et.data(), eh.data(),
                eni.data(), eno.data(), ew.data(), posn.data(), tgt.data(), nidx.data(), nxa.data(),
                pva.data(), sla.data(), kd.data(), xps.data(), via.data(), dfs.data(), drec.data(), sprank.data(), spfirst.data(), spcnt.data()};
    std::vector<uint8_t> rcode(C), rflags(C), sink(C);
    std::vector<int32_t> poff(C + 1), preds(C), slot(C), tbx(C), sseq(C + 1), rnode(C), meta(8 * C);
    RowsView R{rcode.data(), rflags.data(), poff.data(), preds.data(), slot.data(), tbx.data(), sseq.data(), rnode.data(), meta.data()};
    RowCaps caps{(int)C, pool_slots, (int)C, lds_rows};
    SerialCtx c;
    std::vector<int32_t> an(2 * C), ap(2 * C), paths(C);
    int64_t rb = 0, pb = 0;
    unsigned long long counted = 0;
    for (int s = 0; s < n_seqs; ++s) {
        const uint8_t* seq = bases + seq_off[s];
        const int len = seq_off[s + 1] - seq_off[s];
        for (int i = 0; i < len; ++i) posn[i] = -1;
        if (hdr[0] > 0 && len > 0) {
            const int st = trait ? prep_rows_twin(c, G, R, caps, 1, twin_on, &counted) : prep_rows(c, G, R, caps, 1);
            if (st != ST_OK) return st;
            const int n = hdr[0];
            n_rows[s] = n; row_base[s] = rb; pred_base[s] = pb;
            memcpy(flags_out + rb, rflags.data(), (size_t)n);
            memcpy(slot_out + rb, slot.data(), 4 * (size_t)n);
            memcpy(off_out + rb + s, poff.data(), 4 * ((size_t)n + 1));
            memcpy(pred_out + pb, preds.data(), 4 * (size_t)poff[n]);
            rb += n; pb += poff[n];
            for (int r = 0; r < n; ++r) sink[r] = (rflags[r] & ROW_SINK) ? 1 : 0;
            int32_t sc = 0;
            const int k = poa_align_csr(n, rcode.data(), poff.data(), preds.data(), sink.data(), seq, len, p, an.data(), ap.data(), &sc);
            for (int x = 0; x < k; ++x)
                if (an[x] >= 0 && ap[x] >= 0) posn[ap[x]] = rnode[an[x]];
        }
        const int n_before = hdr[0];
        add_alignment(c, G, seq, len, 1u, paths.data(), false);
        spoa_resort(c, G, lst.data(), (int)lst.size(), seq_off[1] - seq_off[0], len, n_before, s == 0);   // spoa's node order
    }
    return 0;
}

// twin_flags on a row CSR handed in (rows 0 .. n-1, predecessors as 1-based row numbers): the harness sets what prep_rows leaves
// in R.flags on entry -- ROW_STORE by the plain rule, ROW_T_NEXT2 / ROW_T_FAR by where the readers lie -- and the product does the rest.
extern "C" void twin_flags_csr(int n, const int32_t* off, const int32_t* pred, uint8_t* flags) {
    std::vector<int32_t> poff(off, off + n + 1), preds(pred, pred + off[n] + 1);
    for (int r = 0; r < n; ++r) flags[r] = 0;
    for (int h = 0; h < n; ++h)
        for (int x = off[h]; x < off[h + 1]; ++x) {
            const int p = pred[x] - 1;
            if (p < 0 || h == p + 1) continue;
            flags[p] |= ROW_STORE | (h == p + 2 ? ROW_T_NEXT2 : ROW_T_FAR);
        }
    RowsView R{};
    R.flags = flags; R.pred_off = poff.data(); R.preds = preds.data();
    SerialCtx c;
    twin_flags(c, n, R);
}

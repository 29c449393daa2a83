// prep_host.h -- the host half of prep (sxg_graph_prep, include/sxg_smooth.h): flatten the graph, compute the schedule Y2, call
// the sort provider, give the nodes their ids in the new order and chop (decree C of DESIGN.md section 9), as GFA text.  Plain
// C++17 on plain containers, included by sxg_smooth.cpp; a header of its own so that tests/csrc/prep_check.cpp can build these
// steps stand-alone under the sanitizers.  Mirrored by tests/prep_ref.py.
#ifndef SXG_PREP_HOST_H
#define SXG_PREP_HOST_H
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/sxg_smooth.h"

namespace sxg_prep {

typedef uint64_t handle_t;  // node index << 1 | is_reverse
inline handle_t mk(uint64_t n, bool r) { return (n << 1) | (r ? 1u : 0u); }
inline uint64_t nid(handle_t h) { return h >> 1; }
inline bool rev(handle_t h) { return h & 1; }

struct graph_view {
    const std::vector<std::string>& seq;                         // by rank
    const std::vector<std::string>& pname;
    const std::vector<std::vector<handle_t>>& steps;
    const std::vector<std::vector<uint64_t>>& pos;               // bp offset of every step
    const std::vector<std::pair<handle_t, handle_t>>& edges;     // the L lines as written
};

// pp was checked by the caller.  Returns SXG_OK with the prepped GFA in o, or a negative code with its reason in err.
inline int run(const graph_view& g, const sxg_prep_params& pp, sxg_sgd_fn sort, void* ctx, std::string& o, std::string& err) {
    // flatten
    const size_t N = g.seq.size(), P = g.steps.size();
    if (N >= (1ull << 31) || P >= (1ull << 31)) { err = "2^31 nodes or paths, or more (decree Y1)"; return SXG_E_INVALID; }
    std::vector<int32_t> node_len(std::max<size_t>(N, 1));
    for (size_t n = 0; n < N; ++n) {
        if (g.seq[n].size() > 0x7fffffffu) { err = "node longer than 2^31 bases"; return SXG_E_INVALID; }
        node_len[n] = (int32_t)g.seq[n].size();
    }
    std::vector<int64_t> path_off(P + 1, 0);
    for (size_t p = 0; p < P; ++p) path_off[p + 1] = path_off[p] + (int64_t)g.steps[p].size();
    const size_t S = (size_t)path_off[P];
    if (S >= (1ull << 32)) { err = "2^32 path steps or more (decree Y1)"; return SXG_E_INVALID; }
    // (uint64)(term_updates * S) is only defined below 2^64; no sort runs 2^63 terms per iteration
    if (!(pp.term_updates * (double)S < 9223372036854775808.0)) { err = "term_updates * steps reaches 2^63"; return SXG_E_INVALID; }
    std::vector<int32_t> step_node(std::max<size_t>(S, 1));
    std::vector<int64_t> step_pos(std::max<size_t>(S, 1));
    uint64_t maxsteps = 0;
    for (size_t p = 0; p < P; ++p) {
        maxsteps = std::max<uint64_t>(maxsteps, g.steps[p].size());
        for (size_t st = 0; st < g.steps[p].size(); ++st) {
            step_node[(size_t)path_off[p] + st] = (int32_t)nid(g.steps[p][st]);
            step_pos[(size_t)path_off[p] + st] = (int64_t)g.pos[p][st];
        }
    }
    // Y2
    const double eta_max = maxsteps > 0 ? (double)maxsteps * (double)maxsteps : 1.0;
    const double lambda = pp.iter_max > 1 ? std::log(eta_max / pp.eps) / (double)(pp.iter_max - 1) : 0.0;
    std::vector<double> eta((size_t)std::max(pp.iter_max, 1));
    for (int t = 0; t < pp.iter_max; ++t) eta[(size_t)t] = eta_max * std::exp(-lambda * (double)t);
    sxg_poa_sgd_in in;
    memset(&in, 0, sizeof(in));
    in.n_nodes = (int64_t)N; in.node_len = node_len.data();
    in.n_paths = (int64_t)P; in.path_off = path_off.data(); in.step_node = step_node.data(); in.step_pos = step_pos.data();
    in.iter_max = pp.iter_max; in.cooling_start = (int32_t)((double)pp.iter_max * pp.cooling); in.eta = eta.data();
    in.terms_per_iter = (uint64_t)(pp.term_updates * (double)S); in.seed = pp.seed; in.mode = pp.mode;
    std::vector<int32_t> order(std::max<size_t>(N, 1), -1);
    if (int rc = sort(ctx, &in, order.data(), nullptr)) { err = "the sort provider failed"; return rc; }
    // apply: the node of old rank order[k] becomes rank k; the provider's answer is checked to be a permutation
    std::vector<int64_t> new_rank(N, -1);
    for (size_t k = 0; k < N; ++k) {
        if (order[k] < 0 || (size_t)order[k] >= N || new_rank[(size_t)order[k]] >= 0) { err = "the sort provider's order is not a permutation"; return SXG_E_INVALID; }
        new_rank[(size_t)order[k]] = (int64_t)k;
    }
    // chop: pieces first[k] .. first[k + 1] - 1 (0-based new ids) of the node at new rank k
    const size_t maxlen = (size_t)pp.max_node_length;
    std::vector<uint64_t> first(N + 1, 0);
    for (size_t k = 0; k < N; ++k) {
        const size_t len = g.seq[(size_t)order[k]].size();
        first[k + 1] = first[k] + (maxlen == 0 || len <= maxlen ? 1 : (len + maxlen - 1) / maxlen);
    }
    o = "H\tVN:Z:1.0\n";
    for (size_t k = 0; k < N; ++k) {
        const std::string& sq = g.seq[(size_t)order[k]];
        const uint64_t pieces = first[k + 1] - first[k];
        for (uint64_t q = 0; q < pieces; ++q) {
            o += "S\t"; o += std::to_string(first[k] + q + 1); o += '\t';
            if (pieces == 1) o += sq; else o.append(sq, (size_t)q * maxlen, maxlen);
            o += '\n';
        }
    }
    std::vector<std::pair<handle_t, handle_t>> edges;
    edges.reserve(g.edges.size() + (size_t)(first[N] - N));
    for (const auto& e : g.edges) {
        const size_t a = (size_t)new_rank[nid(e.first)], b = (size_t)new_rank[nid(e.second)];
        edges.emplace_back(mk(rev(e.first) ? first[a] : first[a + 1] - 1, rev(e.first)), mk(rev(e.second) ? first[b + 1] - 1 : first[b], rev(e.second)));
    }
    for (size_t k = 0; k < N; ++k)
        for (uint64_t q = first[k]; q + 1 < first[k + 1]; ++q) edges.emplace_back(mk(q, false), mk(q + 1, false));
    std::sort(edges.begin(), edges.end());   // (a handle is id << 1 | is_reverse: the order of the decree)
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    for (const auto& e : edges) {
        o += "L\t"; o += std::to_string(nid(e.first) + 1); o += rev(e.first) ? "\t-\t" : "\t+\t";
        o += std::to_string(nid(e.second) + 1); o += rev(e.second) ? "\t-\t0M\n" : "\t+\t0M\n";
    }
    for (size_t p = 0; p < P; ++p) {
        o += "P\t"; o += g.pname[p]; o += '\t';
        bool any = false;
        for (handle_t h : g.steps[p]) {
            const size_t k = (size_t)new_rank[nid(h)];
            const uint64_t pieces = first[k + 1] - first[k];
            for (uint64_t q = 0; q < pieces; ++q) {
                if (any) o += ',';
                any = true;
                o += std::to_string((rev(h) ? first[k + 1] - 1 - q : first[k] + q) + 1);
                o += rev(h) ? '-' : '+';
            }
        }
        o += "\t*\n";
    }
    return SXG_OK;
}

}  // namespace sxg_prep
#endif

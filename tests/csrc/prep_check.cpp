// TEST HARNESS: the host half of prep (smoothxg_amd/csrc/prep_host.h: flatten, apply the order, chop -- what sxg_graph_prep
// runs) as a stand-alone program, so that it can be built with -fsanitize=address,undefined and run as a child process:
//   prep_check GFA ORDER MAX_NODE_LENGTH   -> the prepped GFA on stdout
// GFA: S, L and P lines with integer ids (a reader of its own, a few lines); ORDER: a file of whitespace-separated old ranks in
// the new order.  The sort provider here hands that order back after checking what the library flattened (offsets monotone,
// every step names a node, positions add up, a falling schedule).  Never shipped.
#include "../../smoothxg_amd/csrc/prep_host.h"

#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

using sxg_prep::handle_t;
static std::vector<int32_t> g_order;

static int provider(void*, const sxg_poa_sgd_in* in, int32_t* order, int64_t* x) {
    if (x) return -1;
    if ((size_t)in->n_nodes != g_order.size()) return -2;
    for (int64_t p = 0; p < in->n_paths; ++p) {
        int64_t bp = 0;
        if (in->path_off[p + 1] < in->path_off[p]) return -3;
        for (int64_t s = in->path_off[p]; s < in->path_off[p + 1]; ++s) {
            if (in->step_node[s] < 0 || in->step_node[s] >= in->n_nodes || in->step_pos[s] != bp) return -4;
            bp += in->node_len[in->step_node[s]];
        }
    }
    for (int t = 1; t < in->iter_max; ++t) if (!(in->eta[t] < in->eta[t - 1])) return -5;
    for (size_t k = 0; k < g_order.size(); ++k) order[k] = g_order[k];
    return 0;
}

static std::vector<std::string> split(const std::string& s, char c) {
    std::vector<std::string> f;
    std::stringstream ss(s);
    for (std::string x; std::getline(ss, x, c);) f.push_back(x);
    return f;
}

int main(int argc, char** argv) {
    if (argc != 4) { std::cerr << "usage: prep_check GFA ORDER MAX_NODE_LENGTH\n"; return 2; }
    std::map<long, std::string> nodes;   // id order = rank order
    std::vector<std::vector<std::string>> llines, plines;
    std::ifstream f(argv[1]);
    for (std::string line; std::getline(f, line);) {
        const std::vector<std::string> t = split(line, '\t');
        if (t.size() >= 3 && t[0] == "S") nodes[atol(t[1].c_str())] = t[2];
        else if (t.size() >= 5 && t[0] == "L") llines.push_back(t);
        else if (t.size() >= 3 && t[0] == "P") plines.push_back(t);
    }
    std::map<long, uint64_t> rank;
    std::vector<std::string> seq, pname;
    for (const auto& n : nodes) { rank[n.first] = seq.size(); seq.push_back(n.second); }
    std::vector<std::pair<handle_t, handle_t>> edges;
    for (const auto& t : llines) edges.emplace_back(sxg_prep::mk(rank.at(atol(t[1].c_str())), t[2] == "-"), sxg_prep::mk(rank.at(atol(t[3].c_str())), t[4] == "-"));
    std::vector<std::vector<handle_t>> steps;
    std::vector<std::vector<uint64_t>> pos;
    for (const auto& t : plines) {
        pname.push_back(t[1]);
        steps.emplace_back();
        pos.emplace_back();
        uint64_t bp = 0;
        for (const std::string& st : split(t[2], ',')) {
            const uint64_t r = rank.at(atol(st.substr(0, st.size() - 1).c_str()));
            steps.back().push_back(sxg_prep::mk(r, st.back() == '-'));
            pos.back().push_back(bp);
            bp += seq[r].size();
        }
        pos.back().push_back(bp);
    }
    std::ifstream o(argv[2]);
    for (int32_t v; o >> v;) g_order.push_back(v);
    sxg_prep_params pp;
    memset(&pp, 0, sizeof(pp));
    pp.struct_size = sizeof(pp); pp.max_node_length = atoi(argv[3]); pp.term_updates = 1; pp.iter_max = 100; pp.eps = 0.01; pp.cooling = 0.5;
    std::string out, err;
    const int rc = sxg_prep::run(sxg_prep::graph_view{seq, pname, steps, pos, edges}, pp, provider, nullptr, out, err);
    if (rc) { std::cerr << "prep: " << rc << " " << err << "\n"; return 1; }
    std::cout << out;
    return 0;
}

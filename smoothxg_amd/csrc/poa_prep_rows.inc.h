// poa_prep_rows.inc.h -- the body of prep_rows / prep_rows_twin (poa_graph_dev.h).  NOT a header: the text of the two functions'
// bodies, included once by each with TWIN (constexpr bool) and twin_on defined in front -- prep_rows compiles from the same
// tokens as before round 13.
    const GraphView G = sxg_scalar_view(G_);
    const RowsView R = sxg_scalar_view(R_);
    const int T = c.nthreads(), t = c.tid();
    c.sync();
    const int N = *G.n_nodes;
    if (N > caps.rows_cap) return ST_ROWS_OVERFLOW;
    // (GB rows per thread and iteration, every stage of dependent loads issued for all of them before the next: the chains
    // order -> in_head -> e_tail -> rank are four HBM round trips deep, and one wave per block has nothing else to hide them)
    constexpr int GB = Ctx::GB;
    for (int r0 = t; r0 < N; r0 += GB * T) {
        int v[GB], cd[GB], xp[GB];
#pragma unroll
        for (int u = 0; u < GB; ++u) v[u] = r0 + u * T < N ? G.order[r0 + u * T] : 0;
#pragma unroll
        for (int u = 0; u < GB; ++u) { cd[u] = G.code[v[u]]; xp[u] = hinted ? G.xpos[v[u]] : 0; }
#pragma unroll
        for (int u = 0; u < GB; ++u) {
            const int r = r0 + u * T;
            if (r >= N) continue;
            R.row_node[r] = v[u];
            R.code[r] = (uint8_t)cd[u];
            if (hinted && hinted != 3) R.tbx[r] = xp[u];
        }
    }
    if (hinted == 3) rows_remain(c, G, N, R.tbx);
    const int E = array_excl_sum(c, N, [&](int r) { return G.in_deg[G.order[r]]; }, R.pred_off);
    if (t == 0) R.pred_off[N] = E;
    c.sync();
    // preds in rank space; store / sink flags; last reader of every row (kept in R.slot)
    constexpr int GBH = Ctx::GBH;   // (eleven values per row)
    for (int r0 = t; r0 < N; r0 += GBH * T) {
        int v[GBH], o[GBH], ei[GBH], eo[GBH], od[GBH], ti[GBH], ho[GBH], ni[GBH], no[GBH], ri[GBH], ro[GBH];
#pragma unroll
        for (int u = 0; u < GBH; ++u) {
            const int r = r0 + u * T;
            v[u] = r < N ? G.order[r] : -1;
            o[u] = r < N ? R.pred_off[r] : 0;
        }
#pragma unroll
        for (int u = 0; u < GBH; ++u) {
            ei[u] = v[u] >= 0 ? G.in_head[v[u]] : -1;
            eo[u] = v[u] >= 0 ? G.out_head[v[u]] : -1;
            od[u] = v[u] >= 0 ? G.out_deg[v[u]] : 0;
        }
#pragma unroll
        for (int u = 0; u < GBH; ++u) {   // the first edge of either list (most nodes have one of each)
            ti[u] = ei[u] >= 0 ? G.e_tail[ei[u]] : -1;
            ni[u] = ei[u] >= 0 ? G.e_next_in[ei[u]] : -1;
            ho[u] = eo[u] >= 0 ? G.e_head[eo[u]] : -1;
            no[u] = eo[u] >= 0 ? G.e_next_out[eo[u]] : -1;
        }
#pragma unroll
        for (int u = 0; u < GBH; ++u) {
            ri[u] = ti[u] >= 0 ? G.rank[ti[u]] : -1;
            ro[u] = ho[u] >= 0 ? G.rank[ho[u]] : -1;
        }
#pragma unroll
        for (int u = 0; u < GBH; ++u) {
            const int r = r0 + u * T;
            if (r >= N) continue;
            int oo = o[u], regpred = 0;
            if (ei[u] >= 0) { R.preds[oo++] = ri[u] + 1; regpred |= (int)(ri[u] + 1 == r); }
            for (int e = ni[u]; e >= 0; e = G.e_next_in[e]) { const int pr = G.rank[G.e_tail[e]] + 1; R.preds[oo++] = pr; regpred |= (int)(pr == r); }
            int store = 0, lu = r, two = 0;   // (two: TWIN only -- 1 = a reader at r + 2, 2 = a reader that is neither r + 1 nor r + 2)
            if (eo[u] >= 0) { if (ro[u] != r + 1) store = 1; if (ro[u] > lu) lu = ro[u]; if constexpr (TWIN) two |= ro[u] == r + 2 ? 1 : (ro[u] != r + 1 ? 2 : 0); }
            for (int e = no[u]; e >= 0; e = G.e_next_out[e]) {
                const int hr = G.rank[G.e_head[e]];
                if (hr != r + 1) store = 1;
                if (hr > lu) lu = hr;
                if constexpr (TWIN) two |= hr == r + 2 ? 1 : (hr != r + 1 ? 2 : 0);
            }
            if constexpr (TWIN)
                R.flags[r] = (uint8_t)((store ? ROW_STORE : 0) | (od[u] == 0 ? ROW_SINK : 0) | (regpred ? ROW_REGPRED : 0) |
                                       (twin_on ? (two & 1 ? ROW_T_NEXT2 : 0) | (two & 2 ? ROW_T_FAR : 0) : 0));
            else
            R.flags[r] = (uint8_t)((store ? ROW_STORE : 0) | (od[u] == 0 ? ROW_SINK : 0) | (regpred ? ROW_REGPRED : 0));
            R.slot[r] = lu;
        }
    }
    if constexpr (TWIN) { if (twin_on) *twin_count += twin_flags(c, N, R); }
    return finish_rows(c, N, R, caps, hinted);

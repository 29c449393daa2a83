// poa_dp16_row.inc.h -- one row of the packed sweep (dp_fill_p16, poa_dp16.hip.h) from the point where its inputs stand in
// Hp / Fp / Op / Hleft.  NOT a header: a piece of dp_fill_p16's row loop, included there with
//   P16_ROW_PART & 1   the row's letters and pass 1: Hc (H before the in-row gaps) and the strip's carries a, b, which it declares;
//   P16_ROW_PART & 2   the carry scans, the mailbox, pass 2, the end-cell keys and the stores, in P16_ROW_MODE
//       0  an ordinary row: the registers leave as the row's own state;
//       1  the first row of a twin step (ROW_TWIN): Hp / Fp / Op stay the shared predecessor's, the row's H stays in Hc, HLB gets
//          the column left of it;
//       2  the second row of a twin step (its pass 1 ran in front of the first row's part 2, off the same inputs): the registers
//          leave as the pair's maxima (with HB / HLB, the first row's) when `twin_joined`, else as this row alone.
// It reads the row's number, flags, slot, hint and score table under the names i, flags, myslot, hint, SC_T0, SC_T1.
#if P16_ROW_PART & 1
        RP_MARK(0);  // predecessor rows read, F/O/diagonal set up
        {   // this row's copy of my query letters (an opaque address keeps the loads inside the loop)
            unsigned lo_ = llet_off;
            asm volatile("" : "+v"(lo_));
#pragma unroll
            for (int k2 = 0; k2 < NL; ++k2) let[k2] = ((lds_u32*)(size_t)lo_)[k2];
        }
        // ---- pass 1 (right to left): H before the in-row gaps, strip-local carries
        int a = NEG2, b = NEG2;
        unsigned sc4 = 0;
#pragma unroll
        for (int k = W - 1; k >= 0; --k) {
            if (EXP & 128) { Hc[k] = Fp[k]; continue; }
            // four scores per letter register in one table look-up; the odd bytes -- column k's pair, after a byte shift
            // column k+1's -- are sign-extended into a packed pair by a second permute.  (2 + 1/2 instructions and an
            // add per column; the compare-free form before -- xor, extract, min with 1, multiply-add, add m -- took 4 1/2)
            if ((k & 1) || k == W - 1) sc4 = __builtin_amdgcn_perm(SC_T1, SC_T0, let[k >> 1]);
            const int sc = (int)__builtin_amdgcn_perm(0u, (k & 1) ? (sc4 << 8) : sc4, 0x09030801u);
            int h = pk_add(k ? Hp[k - 1] : Hleft, sc);    // diagonal + (match ? m : n)
            // (MAX3: the three-way maximum of biased fields in one instruction -- pk_max3, poa_fields.h)
            if constexpr (MAX3) h = pk_max3(h, Fp[k], Op[k]);
            else {
                h = pk_max(h, Fp[k]);
                if (CVX) h = pk_max(h, Op[k]);
            }
            Hc[k] = h;
            if constexpr (CTREE) { SXG_PIN("+v"(Hc[k])); continue; }   // (the carries: a tree over the finished columns, below)
            // a = max_k' (h_k' - (k'-k) e) over the columns k' >= k done so far: "the gap is e longer, or restarts here";
            // shifted by (W-1) e below it is max_k (h_k + (W-1-k) e), the carry the strip hands on.  The opening cost
            // and the local-alignment clamp (whose best term is k = W-1) are applied once per row
            a = pk_max(P16_INC(a, Em, E2), h);
            if (CVX) b = pk_max(P16_INC(b, Cm, C2), h);
            SXG_PIN("+v"(Hc[k]), "+v"(a), "+v"(b));
        }
        if constexpr (CTREE) {
            // (round 19) the same two maxima, a = max_k (h_k + (W-1-k) e) and b with c, without the running form's chain of 2 W
            // dependent instructions per carry: W - 1 independent full-rate subtractions of constants -- on both halves at once,
            // no half borrows (p16_carry_leaf_bottom, poa_fields.h) --, the clamp at the bias as one more leaf, and a tree of
            // three-input nodes as the row maximum's below (a node writes ta_[k] after reading ta_[3 k ..])
            int ta_[W + 1], tb_[W + 1];
#pragma unroll
            for (int k = 0; k < W - 1; ++k) {
                ta_[k] = (int)((unsigned)Hc[k] - (unsigned)(W - 1 - k) * Em);
                tb_[k] = (int)((unsigned)Hc[k] - (unsigned)(W - 1 - k) * Cm);
            }
            ta_[W - 1] = tb_[W - 1] = Hc[W - 1];
            ta_[W] = tb_[W] = B2;
#pragma unroll
            for (int n = W + 1; n > 1; n = n / 3 + (n % 3 ? 1 : 0)) {
#pragma unroll
                for (int k = 0; k < n / 3; ++k) {
                    ta_[k] = pk_max3(ta_[3 * k], ta_[3 * k + 1], ta_[3 * k + 2]);
                    tb_[k] = pk_max3(tb_[3 * k], tb_[3 * k + 1], tb_[3 * k + 2]);
                }
                if (n % 3 == 1) { ta_[n / 3] = ta_[n - 1]; tb_[n / 3] = tb_[n - 1]; }
                if (n % 3 == 2) { ta_[n / 3] = pk_max(ta_[n - 2], ta_[n - 1]); tb_[n / 3] = pk_max(tb_[n - 2], tb_[n - 1]); }
            }
            a = ta_[0]; b = tb_[0];
        } else {
        a = P16_DEC(a, (unsigned)(W - 1) * Em, pk2((W - 1) * e, (W - 1) * e));
        if (CVX) b = P16_DEC(b, (unsigned)(W - 1) * Cm, pk2((W - 1) * c, (W - 1) * c));
        if (SW) { a = pk_max(a, B2); if (CVX) b = pk_max(b, B2); }
        }
        a = P16_DEC(a, Gm, G2);
        if (CVX) b = P16_DEC(b, Qm, Q2);
#endif
#if P16_ROW_PART & 2
        // ---- carries (32-bit), inside the wave.  Wave-local strip index u = 2 lane (lo strip), 2 lane + 1 (hi strip); what
        // came in through the mailbox is strip u = -1.  y_u = a_u - u*W*e;  E entering strip u = max_{u'<u} y_u' + (u-1)*W*e.
        // The strips left of a lane's pair are those of the lanes before it: ONE inclusive scan per gap piece over the lanes'
        // max(y_lo, y_hi), shifted by a lane and joined with the mailbox, is X = max_{u' < 2 lane} y_u'; the hi strip adds its
        // own lane's y_lo.  (max is associative: the same values as the two scans per piece of the 64-apart layout.)
        // (the lane's offsets are rebuilt from an opaque copy of the lane every row: hoisted out of the loop
        // they are six more loop-invariant VGPRs, which the allocator spills and reloads per row --
        // and a scratch reload is an in-order vmcnt wait behind every store still in flight)
        int tt = lane;
        asm volatile("" : "+v"(tt));
        const int tWe = __mul24(tt, We), tWc = __mul24(tt, Wc);
        const int ya_lo = pk_lo(a) - 2 * tWe, ya_hi = pk_hi(a) - 2 * tWe - We;
        const int yb_lo = CVX ? pk_lo(b) - 2 * tWc : NEG, yb_hi = CVX ? pk_hi(b) - 2 * tWc - Wc : NEG;
        int xa = max(ya_lo, ya_hi), xb = max(yb_lo, yb_hi);
        if (!(EXP & 8)) {
        xa = sxg_wave_incl_max(xa);
        if (CVX) xb = sxg_wave_incl_max(xb);
        }
        RP_MARK(1);  // pass 1 + in-wave scan
        // what crosses my left edge in this row: {E, Q entering my first column, H of the column left of it, row}
        int in_e = NEG * 2, in_q = NEG * 2, in_h = FLOORV;
        if (wv > 0 && !(EXP & 16)) {
            i32x4 m = mb_in[i & (P16_MBOX - 1)];
            while (__builtin_amdgcn_readfirstlane(m.w) != i) { __builtin_amdgcn_s_sleep(2); m = mb_in[i & (P16_MBOX - 1)]; }
            in_e = __builtin_amdgcn_readfirstlane(m.x) + We;   // (as y of strip u = -1)
            in_q = __builtin_amdgcn_readfirstlane(m.y) + Wc;
            in_h = __builtin_amdgcn_readfirstlane(m.z);
            if (lane == 0) prog[wv] = i;
        }
        RP_MARK(2);  // waiting for the left neighbour
        xa = max(sxg_wave_shr1(xa, NEG * 2), in_e);   // max over every strip left of my lo strip, the mailbox's included
        xb = max(sxg_wave_shr1(xb, NEG * 2), in_q);
        // (MAX3, round 18: E enters a strip no lower than the bias and stays there -- E is neither stored nor returned, and an E
        //  raised to the bias proposes nothing the clamp of H at the bias would not have produced: the clamp rides in E's update)
        constexpr int EFLOOR = MAX3 ? BIAS : FLOORV;
        const int Ein_lo = max(xa + 2 * tWe - We, EFLOOR);
        const int Ein_hi = max(max(xa, ya_lo) + 2 * tWe, EFLOOR);
        const int Qin_lo = !CVX ? FLOORV : max(xb + 2 * tWc - Wc, FLOORV);
        const int Qin_hi = !CVX ? FLOORV : max(max(xb, yb_lo) + 2 * tWc, FLOORV);
        int E = pk2(Ein_lo, Ein_hi), Q = pk2(Qin_lo, Qin_hi);
        // (QDOM: Q stays the carry that entered the strips.  What the long piece is after my hi strip's last column -- the word
        //  the next wave reads -- is that carry run over the strip, or an opening inside the strip: b, which is built for the scan
        //  from H before the in-row gaps exactly as the carries of the strips in between are)
        int mbq = 0;
        if constexpr (QDOM) {
            static_assert(p16_strip_q_dominated(P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, W), "pass 2 without Q needs the short piece to dominate inside a strip");
            mbq = max(Qin_hi + Wc, pk_hi(b));
        }

        // ---- pass 2: final H
        int rowmax = SW ? 0 : NEG2;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            if (EXP & 64) { rowmax = pk_max(rowmax, Hc[k] ^ E ^ Q); continue; }
            int h;
            if constexpr (QDOM) {
                // the long piece at column k of the strip: the carry, k extensions on (each from Q itself: no chain)
                const int Qr = k ? P16_DEC(Q, (unsigned)k * Cm, pk2(k * c, k * c)) : Q;
                if constexpr (MAX3) h = pk_max3(Hc[k], E, Qr);   // (>= the bias: E is)
                else h = pk_max(pk_max(pk_max(Hc[k], E), Qr), NWF2);
            } else {
                if constexpr (MAX3) h = pk_max3(Hc[k], E, Q);
                else {
                    h = pk_max(Hc[k], E);
                    if (CVX) h = pk_max(h, Q);
                }
                h = pk_max(h, SW ? B2 : NWF2);   // (local: 0; global: P16_NWFLOOR)
            }
            Hc[k] = h;
            if constexpr (W >= 12 || !SW) rowmax = pk_max(rowmax, h);
            if constexpr (MAX3) E = pk_max3(P16_DEC(h, Gm, G2), P16_DEC(E, Em, E2), B2);
            else E = pk_max(P16_DEC(h, Gm, G2), P16_DEC(E, Em, E2));
            if constexpr (!QDOM) { if (CVX) Q = pk_max(P16_DEC(h, Qm, Q2), P16_DEC(Q, Cm, C2)); }
            // (round 6: no register pin behind a column below W = 12.  The empty asm made the hazard recogniser pad every column
            //  with three s_nop and kept the compiler from reusing h + g and h + q -- computed here for E and Q -- as the opening
            //  halves of the row's outgoing candidates: 15 + 21 VALU instructions and 18 s_nop per row of the W = 11 headline
            //  class, 124 VGPRs instead of 120, no scratch.  The 16-wave classes W = 12, 13 spill without it.)
            // (round 18, QDOM: there is no Q update to share h + q with; the outgoing candidates below form it themselves)
            if constexpr (W >= 12) {
                if constexpr (QDOM) SXG_PIN("+v"(Hc[k]), "+v"(E), "+v"(rowmax));
                else SXG_PIN("+v"(Hc[k]), "+v"(E), "+v"(Q), "+v"(rowmax));
            }
        }
        if constexpr (W < 12 && SW) {
            // (round 6) the row's greatest H as a TREE over the columns: accumulated column by column the compiler sank the chain of
            // W dependent packed maxima to the loop's end, one s_nop between each (local alignment: every H is >= the bias, no floor needed)
            if (!(EXP & 64)) {
                int t_[W];
#pragma unroll
                for (int k = 0; k < W; ++k) t_[k] = Hc[k];
                if constexpr (MAX3) {
                    // three-input nodes: 5 instead of 9 instructions at W = 10 (a node writes t_[k] after reading t_[3 k ..])
#pragma unroll
                    for (int n = W; n > 1; n = n / 3 + (n % 3 ? 1 : 0)) {
#pragma unroll
                        for (int k = 0; k < n / 3; ++k) t_[k] = pk_max3(t_[3 * k], t_[3 * k + 1], t_[3 * k + 2]);
                        if (n % 3 == 1) t_[n / 3] = t_[n - 1];
                        if (n % 3 == 2) t_[n / 3] = pk_max(t_[n - 2], t_[n - 1]);
                    }
                } else {
#pragma unroll
                for (int n = W; n > 1; n = (n + 1) / 2)
#pragma unroll
                    for (int k = 0; k < n / 2; ++k) t_[k] = pk_max(t_[k], t_[n - 1 - k]);
                }
                rowmax = t_[0];
            }
        }
        // hand my last column to the right neighbour: my hi strip begins where my own lo strip ends, my lo strip where the hi
        // strip of the lane before me ends (lane 0: what came in through the mailbox) -- a lane shift and one v_alignbit;
        // lane 63's hi strip is the wave's right edge -- E, Q after its last column and its H go into the next wave's mailbox
        // of this row (QDOM: Q after the last column is mbq, formed in front of pass 2)
        const int xh = Hc[W - 1];
        const int lh = (int)__builtin_amdgcn_alignbit((unsigned)xh, (unsigned)sxg_wave_shr1(xh, in_h << 16), 16);
        RP_MARK(3);  // carry combine + pass 2
        if (wv + 1 < NW && !(EXP & 16)) {
            if ((i & (P16_MBOX / 2 - 1)) == 0)   // the slots of the next P16_MBOX / 2 rows: has my reader freed them?
                while (__builtin_amdgcn_readfirstlane(prog[wv + 1]) < i - P16_MBOX / 2) __builtin_amdgcn_s_sleep(2);
            if (lane == 63) mb_out[i & (P16_MBOX - 1)] = i32x4{pk_hi(E), QDOM ? mbq : pk_hi(Q), pk_hi(xh), i};
        }
        RP_MARK(4);  // waiting for the right neighbour's progress

        // ---- end cell bookkeeping
        if (EXP & 4) { key_lo ^= (unsigned)rowmax & 1u; }
        else if (SW) {
            // (biased fields: 512 <= field <= 32767, so the keys order as unsigned numbers; a row that merely equals the
            //  strip's best has a smaller lower half and changes nothing: first strictly greatest, decree S4)
            if ((i & 0xffff) == 0) fold_keys(i);
            unsigned inv = 0xffffu - ((unsigned)i & 0xffffu);
            asm volatile("" : "+v"(inv));   // (one VGPR copy: v_perm / v_and_or take one scalar operand each)
            key_lo = max(key_lo, __builtin_amdgcn_perm((unsigned)rowmax, inv, 0x05040100u));
            key_hi = max(key_hi, ((unsigned)rowmax & 0xffff0000u) | inv);
        } else if (flags & ROW_SINK) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                if (k == kL_lo && (bi_lo < 0 || pk_lo(Hc[k]) > best_lo)) { best_lo = pk_lo(Hc[k]); bi_lo = i; bk_lo = k; }
                if (k == kL_hi && (bi_hi < 0 || pk_hi(Hc[k]) > best_hi)) { best_hi = pk_hi(Hc[k]); bi_hi = i; bk_hi = k; }
            }
        }

        RP_MARK(5);  // hand-over + end-cell bookkeeping
        // ---- outgoing candidates (see p16_pack_row), ring store, band store
        // band of this row: strips [bs0, bs0 + BS); my wave covers the strips [128 wv, 128 wv + 128), lo and hi strips
        // alternating: a wave that overlaps the band stores both halves.  (wave-uniform test; the lane tests pick the slot)
        const int bs0 = band_first_strip(hint, W, BS, T);
        const int w0 = wv << 7;
        const bool band_any = !(EXP & 1) && (w0 + 127 >= bs0) && (w0 < bs0 + BS);
        const bool ring = !(EXP & 2) && (flags & ROW_STORE) != 0;
        const __amdgpu_buffer_rsrc_t rs_ring = p16_rsrc((const void*)((SXG_GLOBAL const char*)g_pool + (size_t)(ring && myslot >= 0 ? myslot : 0) * (size_t)RB), RB);
        const __amdgpu_buffer_rsrc_t rs_plane = p16_rsrc((const void*)(g_tb + (size_t)i * (size_t)(SD * BS)), SD * BS * 4);
        const bool in_lo = (unsigned)(w0 + 2 * tt - bs0) < (unsigned)BS, in_hi = (unsigned)(w0 + 2 * tt + 1 - bs0) < (unsigned)BS;
        const unsigned sl_lo = soff & 0xffffu, sl_hi = soff >> 16;   // strip s lives in slot s mod BS of its row
        // (CB = 2) the H left of my strips as the plane row keeps it: strip 0 has no left neighbour -- its own first column,
        // whose step is then 0
        int lhs = lh;
        if (CB == 2 && t == 0) lhs = (int)(((unsigned)lh & 0xffff0000u) | ((unsigned)Hc[0] & 0x0000ffffu));
// (round 6) a lane whose strip lies outside the row's band stores to a slot beyond the row's buffer descriptor -- the hardware
// drops the access -- instead of sitting out a lane-divergent branch around the stores: the structurised branch made the
// compiler keep two sets of the 2 W gap-state registers and copy between them on every row (22 to 66 v_mov per row).
// ring row + band cells of this row; CF(k) / CO(k) = the row's outgoing candidates of column k
#define P16_STORES(CF, CO)                                                                                  \
    do {                                                                                                    \
        if constexpr (CB == 4) if (ring) {                                                                  \
            if (myslot <= -2) {                                                                             \
                P16_LDS_ROW(la_, lf_, -2 - myslot);                                                         \
                _Pragma("unroll") for (int k = 0; k < W; ++k) la_[k * 64] = p16_pack_row<CVX, SW>(Hc[k], CF, CO); \
                *lf_ = (unsigned)lh;                                                                        \
            } else if (!ring_plane) {                                                                       \
                _Pragma("unroll") for (int k = 0; k < W; ++k)                                               \
                    __builtin_amdgcn_raw_buffer_store_b64(p16_pack_row<CVX, SW>(Hc[k], CF, CO), rs_ring, ut8, k * T * 8, 0); \
                __builtin_amdgcn_raw_buffer_store_b32((unsigned)lh, rs_ring, ut8 >> 1, TW * 8, 0);          \
            }                                                                                               \
        }                                                                                                   \
        if constexpr (CB == 2) {                                                                            \
            const bool copy_lds = ring && myslot <= -2, copy_hbm = ring && myslot > -2 && !ring_plane;      \
            /* ONE code per cell (P16RowCode), both halves of a register at once, computed once per row: a stored row \
               and the band cells of the plane are the same words (wave-uniform tests: no lane sits anything out) */ \
            if (copy_lds || copy_hbm || band_any) {                                                         \
                int code_[W];                                                                               \
                _Pragma("unroll") for (int k = 0; k < W; ++k)                                               \
                    code_[k] = p16_row_encode<CVX, SW>(Hc[k], k ? Hc[k ? k - 1 : 0] : lhs, (CF), (CO), DFu, RC); \
                /* a stored row: the codes of my two strips as they stand, and the left word */             \
                if (copy_lds) {                                                                             \
                    P16_LDS_ROW(la_, lf_, -2 - myslot);                                                     \
                    _Pragma("unroll") for (int k = 0; k < W; ++k) la_[k * 64] = (unsigned)code_[k];         \
                    *lf_ = (unsigned)lhs;                                                                   \
                } else if (copy_hbm) {                                                                      \
                    _Pragma("unroll") for (int k = 0; k < W; ++k)                                           \
                        __builtin_amdgcn_raw_buffer_store_b32((unsigned)code_[k], rs_ring, ut8 >> 1, k * T * 4, 0); \
                    __builtin_amdgcn_raw_buffer_store_b32((unsigned)lhs, rs_ring, ut8 >> 1, TW * 4, 0);     \
                }                                                                                           \
                if (band_any) {                                                                             \
                    /* dword x of a strip: halfwords 2x, 2x + 1 of (left H, code 0, ..., code W-1) */        \
                    plane_store_strip<SD>(rs_plane, in_lo ? sl_lo : P16_SLOT_OOB, BS, [&](const int x) -> unsigned { \
                            return __builtin_amdgcn_perm((unsigned)(2 * x < W ? code_[2 * x < W ? 2 * x : 0] : 0), (unsigned)(x ? code_[x ? 2 * x - 1 : 0] : lhs), 0x05040100u); }); \
                    plane_store_strip<SD>(rs_plane, in_hi ? sl_hi : P16_SLOT_OOB, BS, [&](const int x) -> unsigned { \
                            return __builtin_amdgcn_perm((unsigned)(2 * x < W ? code_[2 * x < W ? 2 * x : 0] : 0), (unsigned)(x ? code_[x ? 2 * x - 1 : 0] : lhs), 0x07060302u); }); \
                }                                                                                           \
            }                                                                                               \
        } else {                                                                                            \
        if (band_any) {                                                                                     \
                plane_store_strip<W>(rs_plane, in_lo ? sl_lo : P16_SLOT_OOB, BS, [&](const int k) -> unsigned { \
                    const u32x2 w = p16_pack_row<CVX, SW>(Hc[k], CF, CO);                                   \
                    return __builtin_amdgcn_perm(w.y, w.x, 0x05040100u); });                                \
                plane_store_strip<W>(rs_plane, in_hi ? sl_hi : P16_SLOT_OOB, BS, [&](const int k) -> unsigned { \
                    const u32x2 w = p16_pack_row<CVX, SW>(Hc[k], CF, CO);                                   \
                    return __builtin_amdgcn_perm(w.y, w.x, 0x07060302u); });                                \
        }                                                                                                   \
        }                                                                                                   \
    } while (0)
#if P16_ROW_MODE == 0
#pragma unroll
        for (int k = 0; k < W; ++k) {
            Fp[k] = pk_max(P16_DEC(Hc[k], Gm, G2), P16_DEC(Fp[k], Em, E2));
            if (CVX) Op[k] = pk_max(P16_DEC(Hc[k], Qm, Q2), P16_DEC(Op[k], Cm, C2));
            SXG_PIN("+v"(Fp[k]), "+v"(Op[k]));
        }
        P16_STORES(Fp[k], Op[k]);
#undef P16_STORES
#pragma unroll
        for (int k = 0; k < W; ++k) Hp[k] = Hc[k];
        Hleft = lh;
#else
        // a row of a twin step: its codes take its OWN outgoing candidates, computed on the way into the code -- Fp / Op still
        // hold the shared predecessor's, which the pair's other row and the merged state need
        P16_STORES(pk_max(P16_DEC(Hc[k], Gm, G2), P16_DEC(Fp[k], Em, E2)), (CVX ? pk_max(P16_DEC(Hc[k], Qm, Q2), P16_DEC(Op[k], Cm, C2)) : Op[k]));
#undef P16_STORES
#if P16_ROW_MODE == 1
        // first row of the pair: the inputs stay as they are; its H (Hc) waits for the join
        HLB = lh;
#else
        // second row: the registers leave as the pair's maxima when the next row joins it --
        // max(max(H_B + g, F_A + e), max(H_B' + g, F_A + e)) = max(max(H_B, H_B') + g, F_A + e), the same for O -- else as this row alone
        if (twin_joined) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int hm = pk_max(Hc[k], HB[k]);
                Fp[k] = pk_max(P16_DEC(hm, Gm, G2), P16_DEC(Fp[k], Em, E2));
                if (CVX) Op[k] = pk_max(P16_DEC(hm, Qm, Q2), P16_DEC(Op[k], Cm, C2));
                Hp[k] = hm;
            }
            Hleft = pk_max(lh, HLB);
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                Fp[k] = pk_max(P16_DEC(Hc[k], Gm, G2), P16_DEC(Fp[k], Em, E2));
                if (CVX) Op[k] = pk_max(P16_DEC(Hc[k], Qm, Q2), P16_DEC(Op[k], Cm, C2));
                Hp[k] = Hc[k];
            }
            Hleft = lh;
        }
#endif
#endif
        RP_MARK(7);  // outgoing candidates + stores
#endif

// poa_dp16_fill.inc.h -- the body of the packed sweep, dp_fill_p16 / dp_fill_p16_twin (poa_dp16.hip.h; their comments are there).
// NOT a header: the text of the two functions' bodies, included once by each with TWIN (constexpr bool) defined in front --
// the sweep without the twin step compiles from the same tokens as before round 13.
    DpResult res;
    const int N = __builtin_amdgcn_readfirstlane(N_), L = __builtin_amdgcn_readfirstlane(L_);
    static_assert(W >= 4 && W <= 15, "strip width");
    // (TFIX: the class runs at exactly this many threads -- everything derived from T folds into immediates: 1.2 % on the headline)
    const int T = TFIX ? TFIX : (int)blockDim.x;
    constexpr bool ONEW = TFIX == 64;
    const int NW = T >> 6;
    const int TW = T * W;           // columns of one half
    const int MB = dp16_meta_bytes(T);   // (bytes of the LDS area the traceback window uses; the sweep keeps its mailboxes there)
    int* lds = (int*)smem;
    // (TFIX = 64: a one-wave class -- no left or right neighbour, the mailbox code folds away: 1.7 % on 8000 x 16 x 1 kbp)
    const int t = threadIdx.x, lane = t & 63, wv = ONEW ? 0 : __builtin_amdgcn_readfirstlane(t >> 6);
    // Wave w owns the 128 strips [128 w, 128 w + 128): lane l its strips 128 w + 2 l (low halves) and 128 w + 2 l + 1 (high
    // halves).  A wave's columns are contiguous, so the ONLY thing that crosses a wave boundary inside a row is what crosses
    // one column boundary: the gap states entering the wave's first column and the diagonal's source left of it.
    // (Round 10: ADJACENT strips in a lane.  With strips l and 64 + l the low and the high halves were two separate 64-element
    //  prefix problems per gap piece, stitched by a v_readlane; now a lane's 2 W columns are contiguous, the wave is ONE prefix
    //  problem over the lanes, and what enters a high strip is lane-local.)
    const int s_lo = wv * 128 + 2 * lane, s_hi = s_lo + 1;
    const int j0 = s_lo * W, j0h = s_hi * W;   // first columns of my two strips
    // scoring values are block-uniform: keep them (and everything derived) in SGPRs
    // DS: the class is compiled FOR smoothxg's default scores 1,4,6,2,26,1 (src/main.cpp:322-327) -- the six values and everything
    // derived from them are immediates instead of ~16 loop-invariant scalar registers, which the row loop otherwise spills to
    // VGPR lanes and reads back per use (headline, same box: 1 910 -> 1 848 ms).  Other score sets take the generic class.
    const int g = DS ? P16_DEF_G : __builtin_amdgcn_readfirstlane(S.g), e = DS ? P16_DEF_E : __builtin_amdgcn_readfirstlane(S.e);
    const int q = DS ? P16_DEF_Q : __builtin_amdgcn_readfirstlane(S.q), c = DS ? P16_DEF_C : __builtin_amdgcn_readfirstlane(S.c);
    const int sm = DS ? P16_DEF_M : __builtin_amdgcn_readfirstlane(S.m), sn = DS ? P16_DEF_N : __builtin_amdgcn_readfirstlane(S.n);
    const int G2 = pk2(g, g), E2 = pk2(e, e), Q2 = pk2(q, q), C2 = pk2(c, c);
    // local alignment: biased fields (see P16_BIAS); "x + K" for a penalty K <= 0 is then x - |K| * 0x10001 in 32 bits
    constexpr int BIAS = SW ? P16_BIAS : 0, FLOORV = SW ? P16_FLOOR : NEGP;
    // the local classes compiled for the default scores take three-way maxima of their biased fields as ONE binary16
    // instruction (pk_max3): the fields stay inside the patterns whose binary16 order is the integer order (poa_fields.h)
    constexpr bool MAX3 = SW && DS && CVX;
    static_assert(!MAX3 || p16_fields_are_f16_ordered(P16_DEF_N, P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, W), "biased fields leave the ordered binary16 patterns");
    // ... and build pass 1's strip carries as trees of such maxima over the strip's columns, each run down to the strip's last
    // column by one plain 32-bit subtraction (p16_carry_leaf_bottom, poa_fields.h: no half borrows, every leaf stays ordered).
    // (every width: W = 12 and 13, which spill without their pins, keep their registers and scratch with it -- profiles/r22)
    constexpr bool CTREE = MAX3;
    static_assert(!CTREE || p16_carry_leaf_bottom(P16_DEF_N, P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, W) >= 0, "a leaf of the carry trees borrows");
    // the classes compiled for the default scores read the long gap piece inside a strip off the strip's carry: opened inside
    // the strip it never beats the short piece there (p16_strip_q_dominated, poa_fields.h), so pass 2 keeps no Q state
    constexpr bool QDOM = CVX && DS;
    static_assert(!QDOM || p16_strip_q_dominated(P16_DEF_G, P16_DEF_E, P16_DEF_Q, P16_DEF_C, W), "the long piece may win inside a strip of this width");
    const int NEG2 = pk2(FLOORV, FLOORV), B2 = pk2(BIAS, BIAS), NWF2 = pk2(P16_NWFLOOR, P16_NWFLOOR);
    const unsigned Gm = (unsigned)(-g) * 0x10001u, Em = (unsigned)(-e) * 0x10001u, Qm = (unsigned)(-q) * 0x10001u, Cm = (unsigned)(-c) * 0x10001u;
#define P16_DEC(x, Km, K2) (SW ? (int)((unsigned)(x) - (Km)) : pk_add((x), (K2)))   /* x + K */
#define P16_INC(x, Km, K2) (SW ? (int)((unsigned)(x) + (Km)) : pk_sub((x), (K2)))   /* x - K */
    // substitution scores come out of a per-row byte table (see pass 1): all-mismatch rows of it, and match ^ mismatch
    const unsigned SC_N4 = (unsigned)(sn & 0xff) * 0x01010101u, SC_MX = (unsigned)((sm ^ sn) & 0xff);
    const int We = W * e, Wc = W * c;
    const int BS = __builtin_amdgcn_readfirstlane(B.band_strips);
    constexpr int SD = p16_slot_dwords(W, CB);   // dwords of one strip in a plane row
    // (CB = 2) the field widths of the 2-byte cell code
    Scoring SD_ = S;
    if (DS) { SD_.m = P16_DEF_M; SD_.n = P16_DEF_N; SD_.g = P16_DEF_G; SD_.e = P16_DEF_E; SD_.q = P16_DEF_Q; SD_.c = P16_DEF_C; SD_.convex = 1; }
    const P16Delta DF = p16_delta_of(SD_);
    const int dbH_ = __builtin_amdgcn_readfirstlane(DF.bH), dbF_ = __builtin_amdgcn_readfirstlane(DF.bF);
    // (CB = 2) the ONE code of a cell (round 11): the row code (P16RowCode, poa_rowcode.h) is what the ring, the on-chip row
    // copies and the plane hold
    P16Delta DFu = DF;
    DFu.bH = dbH_; DFu.bF = dbF_; DFu.bO = __builtin_amdgcn_readfirstlane(DF.bO);
    DFu.g = g; DFu.eabs = -e; DFu.cabs = -c;
    const P16RowCode RC = p16_row_code_of(DFu, CVX);
    // A plane that keeps EVERY strip of every row (sequences up to ~1.4 kbp -- the blocks smoothxg's default -l 700 ... 1100
    // produces --, the every-strip plane of a band-miss re-run) already holds what the row ring would: stored rows are not
    // written a second time, a stored predecessor is read back from its plane row and decoded.  (Cost map of 8000 x 16 x 1 kbp,
    // round 5: ring stores 14 % of the sweep, at the HBM write roof.)
    const bool ring_plane = RP == 2 ? true : (RP == 1 && CB == 2 && BS == 2 * T);
    // ---- wave pipeline.  The waves of a workgroup do NOT meet inside the row loop.  Wave w sweeps row i as soon as wave
    // w-1 has handed over, through a ring of P16_MBOX mailboxes in LDS, the three values that cross its left edge in row i:
    // E and Q entering its first column and H of the column left of it (one 16-byte word {E, Q, H, row}, written and read
    // by single LDS instructions; the row number is the "full" flag).  Everything else a wave reads it wrote itself: rows
    // in the ring are lane-private, and a stored row carries the left-neighbour columns of every lane's two strips (the last
    // column of the lane before it, and of its own low strip) as one more word.
    // Waves drift apart by up to P16_MBOX rows (a writer checks every P16_MBOX / 2 rows that its reader has freed the
    // slots it is about to reuse), so a wave that waits -- for a stored predecessor row, for its SIMD -- delays its
    // successors only once that slack is used up: the per-row cost is the AVERAGE over the waves, not the maximum that
    // two s_barrier per row made it (47 % of the wave time was parked in round 2).
    typedef __attribute__((address_space(3))) i32x4 lds_i32x4;
    typedef __attribute__((address_space(3))) int lds_i32;
    constexpr int P16_MBOX = 16;
    const unsigned lds0 = (unsigned)__builtin_amdgcn_groupstaticsize();
    volatile lds_i32x4* const mb_in = (volatile lds_i32x4*)(size_t)(lds0 + (unsigned)(LDS_CTL_BYTES + (max(wv, 1) - 1) * P16_MBOX * 16));
    volatile lds_i32x4* const mb_out = (volatile lds_i32x4*)(size_t)(lds0 + (unsigned)(LDS_CTL_BYTES + wv * P16_MBOX * 16));
    volatile lds_i32* const prog = (volatile lds_i32*)(size_t)(lds0 + 64u * 4u);   // [16] rows consumed by wave w
    if (lane < P16_MBOX) mb_out[lane] = i32x4{0, 0, 0, 0};
    if (lane == 0) prog[wv] = 0;
    __syncthreads();

    // query letters, one byte per (strip, column), as SELECTORS into the row's score table: A,C,G,T,N = 0..4, "no letter"
    // (padding columns, never a match) = 5.  Register k2 holds the bytes (lo_k+1, lo_k, hi_k+1, hi_k) of columns
    // k = 2 k2 and k + 1 -- the order in which one v_perm turns them into four scores with column k's pair on the odd
    // bytes, where a second v_perm can sign-extend them into a packed pair.
    constexpr int NL = (W + 1) / 2;
    unsigned let[NL];
#pragma unroll
    for (int k2 = 0; k2 < NL; ++k2) {
        unsigned v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int kc = 2 * k2 + ((b & 1) ? 0 : 1);  // strip-local column (W odd: one spare pair)
            const int j = ((b >> 1) ? j0h : j0) + kc;
            const bool valid = kc < W && j >= 1 && j <= L;
            const unsigned ch = valid ? (unsigned)seq[j - 1] : 5u;
            v |= (valid && ch > 4u ? 4u : ch) << (8 * b);
        }
        let[k2] = v;
    }
    // The letters live in LDS, not in registers: six loop-invariant VGPRs less, which is what the
    // allocator otherwise evicts to scratch around the multi-predecessor path -- and a scratch reload
    // is an in-order vmcnt wait behind the stores just issued.  Lane-major, read back with
    // two wide LDS loads per row.
    // (raw LDS byte offset: the dynamic LDS starts right behind the kernel's static LDS)
    typedef __attribute__((address_space(3))) unsigned lds_u32;
    const int LDS_ROWS = __builtin_amdgcn_readfirstlane(B.lds_rows);
    // a stored row: W columns of row words [column][lane] (CB = 4: 8-byte words, packed H + two distances; CB = 2: one dword of
    // row codes, see P16RowCode), then the column LEFT of every lane's strips (4 bytes per lane).
    // (Pairs of columns per 16-byte access, as in the plane, were measured in round 4: 90 instead of 131 memory instructions in
    // the row loop, 2 010 against 1 996 ms on the headline, c3 -1 %, c4 +1 %: the ring's cost is its volume, not its instruction
    // count -- kept at one word per column.)
    constexpr int RWB = CB == 2 ? 4 : 8;   // bytes of one row word
    const int RB = dp16_row_bytes(T, W, CB);
    const unsigned llet_off = (unsigned)__builtin_amdgcn_groupstaticsize() + (unsigned)(LDS_CTL_BYTES + MB + LDS_ROWS * RB + t * NL * 4);
#pragma unroll
    for (int k2 = 0; k2 < NL; ++k2) ((lds_u32*)(size_t)llet_off)[k2] = let[k2];

    // Rows in HBM (ring, row 0) are laid out [column-in-strip][lane] and the plane
    // [row][column-in-strip][strip of the band]: a load/store instruction then covers consecutive words of
    // a wave instead of 64 different cache lines.  Every access is "uniform pointer"[lane offset]: scalar
    // base, one loop-invariant lane offset register, no per-access address arithmetic.
    const unsigned ut8 = (unsigned)t * 8u;   // my byte offset inside a [column][lane] row of 8-byte words
    SXG_GLOBAL u32x2* const g_row0 = sxg_uniform(sxg_global((u32x2*)B.row0));
    SXG_GLOBAL u32x2* const g_pool = sxg_uniform(sxg_global((u32x2*)B.pool));
    SXG_GLOBAL uint32_t* const g_tb = sxg_uniform(sxg_global((uint32_t*)B.tb));
    SXG_GLOBAL const int32_t* const g_meta = sxg_uniform(sxg_global((const int32_t*)R.meta));
    SXG_GLOBAL const int32_t* const g_preds = sxg_uniform(sxg_global((const int32_t*)R.preds));
    SXG_GLOBAL const int32_t* const g_slot = sxg_uniform(sxg_global((const int32_t*)R.slot));
    int Hp[W], Fp[W], Op[W], Hleft;
    // virtual row 0
#pragma unroll
    for (int k = 0; k < W; ++k) {
        int h2[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int j = (hf ? j0h : j0) + k;
            int h = BIAS;
            if (!SW && j > 0) { const int a = g + (j - 1) * e, b = q + (j - 1) * c; h = max(a > b ? a : b, P16_NWFLOOR); }
            h2[hf] = h;
        }
        Hp[k] = pk2(h2[0], h2[1]);
        Fp[k] = P16_DEC(Hp[k], Gm, G2);             // nothing to extend in row 0: both candidates open
        Op[k] = CVX ? P16_DEC(Hp[k], Qm, Q2) : NEG2;
    }
    {
        int h2[2];
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const int j = (hf ? j0h : j0) - 1;
            int h = BIAS;
            if (!SW && j > 0) { const int a = g + (j - 1) * e, b = q + (j - 1) * c; h = max(a > b ? a : b, P16_NWFLOOR); }
            h2[hf] = j < 0 ? FLOORV : h;
        }
        Hleft = pk2(h2[0], h2[1]);
    }
    {
        const __amdgpu_buffer_rsrc_t rs0 = p16_rsrc((const void*)g_row0, RB);
        if constexpr (CB == 2) {
            // (strip 0 has no left neighbour: its codes start from its own first column, as in the plane)
            const int lh0 = t == 0 ? (int)(((unsigned)Hleft & 0xffff0000u) | ((unsigned)Hp[0] & 0x0000ffffu)) : Hleft;
            int prev = lh0;
#pragma unroll
            for (int k = 0; k < W; ++k) {
                __builtin_amdgcn_raw_buffer_store_b32((unsigned)p16_row_encode<CVX, SW>(Hp[k], prev, Fp[k], Op[k], DFu, RC), rs0, (unsigned)t * 4u, k * T * 4, 0);
                prev = Hp[k];
            }
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)lh0, rs0, (unsigned)t * 4u, TW * 4, 0);
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k)
                __builtin_amdgcn_raw_buffer_store_b64(p16_pack_row<CVX, SW>(Hp[k], Fp[k], Op[k]), rs0, ut8, k * T * 8, 0);
            __builtin_amdgcn_raw_buffer_store_b32((unsigned)Hleft, rs0, (unsigned)t * 4u, TW * 8, 0);
        }
    }
    int best_lo = NEGP * 2, best_hi = best_lo, bi_lo = -1, bi_hi = -1, bk_lo = 0, bk_hi = 0;   // (global alignment only)
    const int kL_lo = L - j0, kL_hi = L - j0h;  // strip-local index of the end column L
    unsigned key_lo = 0u, key_hi = 0u;          // local alignment: (greatest H of my strip) << 16 | 0xffff - (row & 0xffff)
    unsigned long long ekey = 0ull;             // wave-uniform: best of the finished epochs (value, row, strip -- see fold_keys)
    // per-lane keys of the epoch that ends in front of row `i_end` -> ekey.  value << 32 | (0xFFFFF - row) << 12 | (0xFFF - strip):
    // greatest score, then smallest row, then smallest strip (strips are disjoint column ranges in ascending order)
    auto fold_keys = [&](const int i_end) {
        const unsigned ep = (unsigned)(i_end - 1) >> 16;
        auto k64 = [&](const unsigned k, const int strip) -> unsigned long long {
            if (k == 0u) return 0ull;
            const unsigned row = (ep << 16) | (0xffffu - (k & 0xffffu));
            return ((unsigned long long)(k >> 16) << 32) | ((unsigned long long)(0xFFFFFu - row) << 12) | (unsigned long long)(0xFFFu - (unsigned)strip);
        };
        unsigned long long kk = k64(key_lo, s_lo);
        const unsigned long long k2 = k64(key_hi, s_hi);
        kk = k2 > kk ? k2 : kk;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(kk, d);
            kk = o > kk ? o : kk;
        }
        const unsigned hi_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(kk >> 32)), lo_ = (unsigned)__builtin_amdgcn_readfirstlane((int)kk);
        const unsigned long long ku = ((unsigned long long)hi_ << 32) | lo_;
        ekey = ku > ekey ? ku : ekey;
        key_lo = 0u; key_hi = 0u;
    };

    // (An L2 warm-up for the next row's stored predecessor -- one load per wave touching its 44 cache lines a row ahead,
    // retired before the stores -- measured 0-5 % SLOWER in round 2: returns are in order, so whatever is in front of the
    // demand loads holds them back, and a wait behind it stalls.)
    // (A register/LDS prefetch of the next row's stored predecessor, requested after pass 2 and collected before
    // this row's stores, was measured again in round 2 with the spills gone: 2.81 s against 2.68 s.  At this VALU
    // occupancy the co-resident workgroups already hide the round trip; its ~60 extra instructions do not pay.)
    typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
    // on-chip copies of stored rows (finish_rows: a stored row whose last reader comes before LDS_ROWS more rows are stored
    // lives in LDS only and never travels to HBM): behind the control words and the mailbox / traceback-window area
    const unsigned lds_rows0 = lds0 + (unsigned)(LDS_CTL_BYTES + MB);
// my words of on-chip row copy b_: W row words [wave][column][lane] (a wave's 64 lanes side by side: every LDS access of
// the sweep is conflict-free, and column k is the immediate offset k * 64 * RWB), then the left-neighbour word [lane].  The
// addresses are rebuilt from an opaque copy of the thread index: no loop-invariant address registers.
#define P16_LDS_ROW(words_, left_, b_)                                                                      \
    int tq_ = t;                                                                                            \
    asm volatile("" : "+v"(tq_));                                                                           \
    const unsigned lb_ = lds_rows0 + (unsigned)(b_) * (unsigned)RB;                                         \
    std::conditional_t<CB == 2, lds_u32, lds_u32x2>* const words_ = (std::conditional_t<CB == 2, lds_u32, lds_u32x2>*)(size_t)(lb_ + (unsigned)(wv * (64 * RWB * W - 64 * RWB)) + (unsigned)tq_ * (unsigned)RWB); \
    lds_u32* const left_ = (lds_u32*)(size_t)(lb_ + (unsigned)(TW * RWB) + (unsigned)tq_ * 4u)
    // (B lives in the kernel's private memory: testing B.prio_board per row was a scratch load plus an
    // in-order vmcnt(0) -- a wait for every store of the previous row -- at the top of EVERY row)
    const bool has_board = __builtin_amdgcn_readfirstlane((int)(B.prio_board != nullptr)) != 0;
    // slots of my two strips in a plane row (strip s -> slot s mod BS: the address of a cell does not depend
    // on where the row's band starts, so the traceback fetches cells and row descriptors in ONE round trip)
    const unsigned soff = (unsigned)(s_lo % BS) | ((unsigned)(s_hi % BS) << 16);
    const int prio_rank = __builtin_amdgcn_readfirstlane(B.prio_rank);
#ifdef SXG_ROW_PROF
// profiling builds: wait for the fetched row right away and book the time as segment 6 ("stored row fetch")
#define P16_PROF_FETCH() do { RP_MARK(0); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); RP_MARK(6); } while (0)
#else
#define P16_PROF_FETCH() do { } while (0)
#endif
#ifdef SXG_ROW_PROF
    unsigned long long racc[ROWP_SEGS] = {0};  // per row segment; scalar registers (s_memtime deltas)
#define RP_MARK(seg) do { const unsigned long long tn_ = __builtin_readcyclecounter(); racc[seg] += tn_ - rt_; rt_ = tn_; } while (0)
#else
#define RP_MARK(seg) do { } while (0)
#endif
    // Row descriptors (RowMeta, 32 bytes) come through the SCALAR data path, one s_load_dwordx8 per row issued a row ahead:
    // every wave is at its own row, so there is no chunk of descriptors the workgroup could stage together.  The scalar
    // cache is not coherent with the vector stores that wrote the descriptors (prep_rows, the band-miss hint shift): it is
    // invalidated once per sweep, after the workgroup barrier that follows those stores.
    typedef int i32x8 __attribute__((ext_vector_type(8)));
    typedef __attribute__((address_space(4))) const i32x8 const_i32x8;
    const_i32x8* const cmeta = (const_i32x8*)(unsigned long long)g_meta;
    __builtin_amdgcn_s_dcache_inv();
    i32x8 dnext = cmeta[0];
    // (twin classes: the first descriptor has arrived before the loop is entered.  Scalar loads return out of order, so with it
    //  still in flight at the loop's head the first read of a descriptor word inside the loop needs lgkmcnt(0) -- which also waits
    //  for the next row's descriptor, asked for a few instructions earlier: an exposed scalar-load latency in every row)
    if constexpr (TWIN) { const int d1_ = dnext[1]; asm volatile("" :: "s"(d1_)); }   /* (a use: the compiler waits for the load here) */
    for (int i = 1; i <= N; ++i) {
        if (has_board) { if ((i & 127) == 1) sxg_balance_prio(B, (unsigned long long)i * (unsigned long long)(2 * TW)); }   /* rows done x swept columns (poa_cost.h) */
        else if ((i & 63) == 1) sxg_rotate_prio(prio_rank);
        // (not const: behind a twin step the iteration goes on with the row that follows the pair)
        i32x8 dsc = dnext;
        dnext = cmeta[min(i, N - 1)];
        int pb = dsc[0], info = dsc[1], p0 = dsc[2], s0 = dsc[3], p1 = dsc[4], s1 = dsc[5], myslot = dsc[6], hint = dsc[7];
        int np = info & 0xffff, code = (info >> 16) & 0xff, flags = (info >> 24) & 0xff;
        // score table of this row: byte c = score(node letter, query letter c); c = 5 (no letter) never matches
        unsigned SC_T0 = SC_N4 ^ (code < 4 ? SC_MX << (8 * code) : 0u), SC_T1 = SC_N4 ^ (code == 4 ? SC_MX : 0u);

#ifdef SXG_ROW_PROF
        unsigned long long rt_ = __builtin_readcyclecounter();
#endif
        int Hc[W];
        // Fp/Op arrive holding the previous row's OUTGOING candidates.  (Rounds 1-5 had a sibling rule: a row whose successor has
        // the same single predecessor -- an alternative allele, 15 % of the rows -- kept its own F/O for it and the successor fetched
        // only the diagonal.  Round 6 measured it as a LOSS: "update in place or keep" was a merge the register allocator resolved
        // with a second set of 2 W registers and 22 v_mov at the top of four rows in five, and the second store path doubled the
        // loop's code.  Without it a sibling unpacks F/O from its predecessor's stored row like any other row: headline
        // 1 859 -> 1 786 ms on one box, 1 417 -> 1 025 static VALU instructions and 132 -> 42 v_mov in the loop.)
// words of the stored row of predecessor p_ (slot sl_) and the column to their left (stored with the row: every word of
// a stored row was written by the lane that reads it).  sl_ <= -2: the row is one of the LDS_ROWS on-chip copies.
// (CB = 2: wr_ are the row codes, unsigned [W], and hl_ is the left word as stored -- P16_DECODE turns both into values)
#define P16_FETCH(p_, sl_, wr_, hl_)                                                                        \
    do {                                                                                                    \
        if ((sl_) <= -2) {                                                                                  \
            P16_LDS_ROW(la_, lf_, -2 - (sl_));                                                              \
            _Pragma("unroll") for (int k = 0; k < W; ++k) wr_[k] = la_[k * 64];                             \
            hl_ = (int)*lf_;                                                                                \
        } else {                                                                                            \
            const __amdgpu_buffer_rsrc_t rs_ = p16_rsrc(((p_) == 0) ? (const void*)g_row0 : (const void*)((SXG_GLOBAL const char*)g_pool + (size_t)(sl_) * (size_t)RB), RB); \
            if constexpr (CB == 2) {                                                                        \
                _Pragma("unroll") for (int k = 0; k < W; ++k) wr_[k] = __builtin_amdgcn_raw_buffer_load_b32(rs_, ut8 >> 1, k * T * 4, 0); \
            } else {                                                                                        \
                _Pragma("unroll") for (int k = 0; k < W; ++k) wr_[k] = __builtin_amdgcn_raw_buffer_load_b64(rs_, ut8, k * T * 8, 0); \
            }                                                                                               \
            P16_PROF_FETCH();                                                                               \
            hl_ = (int)__builtin_amdgcn_raw_buffer_load_b32(rs_, ut8 >> 1, TW * RWB, 0);                     \
            P16_DRAIN();                                                                                    \
        }                                                                                                   \
    } while (0)
// (CB = 2) a fetched row's codes -> HS_/FS_/OS_[k], the row's H and outgoing candidates, summing the steps from the left word;
// then the left word as the sweep keeps it (strip 0: "minus infinity", see the left word of P16RowCode)
#define P16_DECODE(wr_, hl_, HS_, FS_, OS_)                                                                 \
    do {                                                                                                    \
        int run_ = hl_;                                                                                     \
        _Pragma("unroll") for (int k = 0; k < W; ++k) {                                                     \
            p16_row_decode<CVX, SW>(wr_[k], run_, FS_[k], OS_[k], RC);                                      \
            HS_[k] = run_;                                                                                  \
        }                                                                                                   \
        if (t == 0) hl_ = (int)(((unsigned)hl_ & 0xffff0000u) | ((unsigned)FLOORV & 0xffffu));               \
    } while (0)

// ... or, with ring_plane, the row's strips out of its plane row: H of the column left of the strips, then per column the
// row code of my two strips, one v_perm picking the halves out of the two strips' dwords; HS_/FS_/OS_[k] receive the row's H
// and outgoing candidates -- the same p16_row_decode as a row out of the ring
#define P16_FETCH_PLANE(p_, HS_, FS_, OS_, hl_)                                                             \
    do {                                                                                                    \
        const __amdgpu_buffer_rsrc_t rsp_ = p16_rsrc((const void*)(g_tb + (size_t)(p_) * (size_t)(SD * BS)), SD * BS * 4); \
        unsigned dl_[SD], dh_[SD];                                                                          \
        plane_load_strip<SD>(rsp_, soff & 0xffffu, BS, dl_);                                                \
        plane_load_strip<SD>(rsp_, soff >> 16, BS, dh_);                                                    \
        P16_PROF_FETCH();                                                                                   \
        P16_DRAIN();                                                                                        \
        int run_ = (int)__builtin_amdgcn_perm(dh_[0], dl_[0], 0x05040100u);                                 \
        hl_ = t == 0 ? (int)(((unsigned)run_ & 0xffff0000u) | ((unsigned)FLOORV & 0xffffu)) : run_;         \
        _Pragma("unroll") for (int k = 0; k < W; ++k) {                                                     \
            const unsigned cn_ = __builtin_amdgcn_perm(dh_[(k + 1) >> 1], dl_[(k + 1) >> 1], ((k + 1) & 1) ? 0x07060302u : 0x05040100u); \
            p16_row_decode<CVX, SW>(cn_, run_, FS_[k], OS_[k], RC);                                         \
            HS_[k] = run_;                                                                                  \
        }                                                                                                   \
    } while (0)

// Every branch that loaded a stored row from HBM ends by draining its loads itself.  Otherwise the compiler, which cannot
// know at the join which branch ran, waits for vmcnt(0) at the top of pass 1 of EVERY row (a loaded register that a branch
// did not consume is reused there) -- and on gfx9 vmcnt also counts stores, so rows that read nothing waited for the
// write acknowledgements of the previous row's ring and band stores.
#define P16_DRAIN() __builtin_amdgcn_s_waitcnt(0x0F70) /* vmcnt(0), expcnt / lgkmcnt untouched */
        // The diagonal sources are left WHERE THEY ARE -- Hp[k] = max over the predecessors of their H in column k,
        // Hleft the column left of the strip -- and pass 1 walks the strip right to left, so that column k's new value
        // can take the register of Hp[k] (dead once column k+1 has used it): the shifted copy Hc[k] = Hp[k-1] that an
        // ascending pass needs cost 11-23 v_mov per row.
        if constexpr (TWIN) {
            // (a loop in front of the ordinary row, not a second way through the iteration: the ordinary row's registers then run
            //  from the loop's head to its one back edge as they did, and what the allocator moves for the step stays beside it)
            bool swept_out = false;
            while (flags & ROW_TWIN) {
                // ---- twin step (round 13): rows i and i + 1 have the same single predecessor, whose values stand in the registers
                // now (the previous row, or one fetch and decode above).  Pass 1 of both rows runs off them first -- the second row's
                // takes the registers of the diagonal sources --, then each row finishes under its own number: mailbox words,
                // progress, end-cell keys, band and ring stores are the two rows' own, in row order.
                // (the step sets its inputs up itself, in front of the ordinary rows' own set-up: the two paths share no block
                //  between the loop's head and its end, so whatever the allocator moves for the step stays on the step's side)
                // (the turns at the priority board of the second row and of the row behind the pair -- the iteration goes on with
                //  that row without passing the loop's head -- are taken here, a row or two early: a call between the two rows
                //  would have the step's whole state live across it.  At most one of the two is due.)
                if (has_board) {
                    const int due = ((i + 1) & 127) == 1 ? i + 1 : ((((i + 2) & 127) == 1 && i + 2 <= N) ? i + 2 : 0);
                    if (due) sxg_balance_prio(B, (unsigned long long)due * (unsigned long long)(2 * TW));
                } else if (((i + 1) & 63) == 1 || (((i + 2) & 63) == 1 && i + 2 <= N)) sxg_rotate_prio(prio_rank);
                if (p0 != i - 1) {
                    int hl;
                    unsigned wr[W];
                    P16_FETCH(p0, s0, wr, hl);
                    P16_DECODE(wr, hl, Hp, Fp, Op);
#pragma unroll
                    for (int k = 0; k < W; ++k) SXG_PIN("+v"(Hp[k]), "+v"(Fp[k]), "+v"(Op[k]));
                    Hleft = hl;
                }
                if (!CVX) {
#pragma unroll
                    for (int k = 0; k < W; ++k) Op[k] = NEG2;
                }
                const i32x8 dsc2 = dnext;
                dnext = cmeta[min(i + 1, N - 1)];
                const int i2 = i + 1;
                const int info2 = dsc2[1], cd2 = (info2 >> 16) & 0xff;
                const unsigned t0_2 = SC_N4 ^ (cd2 < 4 ? SC_MX << (8 * cd2) : 0u), t1_2 = SC_N4 ^ (cd2 == 4 ? SC_MX : 0u);
                int Hc2[W], a2, b2, HLB;
                // The fragment poa_dp16_row.inc.h speaks of the row under FIXED names, which every inclusion below binds on purpose:
                //   part 1 reads  SC_T0, SC_T1 (the row's score table), Hp, Fp, Op, Hleft;  writes Hc[], declares a, b
                //                 (and sc4; the leaves of its carry trees, ta_ / tb_, live in a block of their own);
                //   part 2 reads  i, flags, myslot, hint, Hc[], a, b;  modes 1 / 2 also HLB, HB[], twin_joined (see its header).
                // A rename inside the fragment has to be followed here, or a shadowed name silently binds to the outer row's.
                // (1) first row, pass 1: every name is the loop's own (row i); declares a, b for (3)
#define P16_ROW_MODE 1
#define P16_ROW_PART 1
#include "poa_dp16_row.inc.h"
#undef P16_ROW_PART
                {   // (2) second row, pass 1: shadows SC_T0, SC_T1 (row i + 1's table) and Hc (-> Hc2); its a, b leave as a2, b2
                    const unsigned SC_T0 = t0_2, SC_T1 = t1_2;
                    int (&Hc)[W] = Hc2;
#define P16_ROW_PART 1
#include "poa_dp16_row.inc.h"
#undef P16_ROW_PART
                    a2 = a; b2 = b;
                }
                {   // (3) first row, the rest (mode 1): i, flags, myslot, hint, Hc, a, b are the loop's own and (1)'s
#define P16_ROW_PART 2
#include "poa_dp16_row.inc.h"
#undef P16_ROW_PART
                }
#undef P16_ROW_MODE
                {
                    // does row i + 2 take both rows out of the registers?  (its descriptor was asked for a row ago; behind the last
                    // row dnext is row i + 1's own, which has one predecessor and never joins)
                    const bool twin_joined = (((dnext[1] >> 24) & 0xff) & ROW_JOIN) != 0;
                    const int fl2 = (info2 >> 24) & 0xff, ms2 = dsc2[6], hn2 = dsc2[7];
                    int (&HB)[W] = Hc;
                    {   // (4) second row, the rest (mode 2): shadows i, flags, myslot, hint, SC_T0, SC_T1, Hc (-> Hc2), a, b (<- a2, b2);
                        //     HB names the first row's H (the outer Hc), HLB the column left of it
                        const int i = i2, flags = fl2, myslot = ms2, hint = hn2;
                        const unsigned SC_T0 = t0_2, SC_T1 = t1_2;
                        int (&Hc)[W] = Hc2;
                        int a = a2, b = b2;
#define P16_ROW_MODE 2
#define P16_ROW_PART 2
#include "poa_dp16_row.inc.h"
#undef P16_ROW_PART
#undef P16_ROW_MODE
                    }
                }
                i += 2;
                if (i > N) { swept_out = true; break; }
                dsc = dnext;
                dnext = cmeta[min(i, N - 1)];
                pb = dsc[0]; info = dsc[1]; p0 = dsc[2]; s0 = dsc[3]; p1 = dsc[4]; s1 = dsc[5]; myslot = dsc[6]; hint = dsc[7];
                np = info & 0xffff; code = (info >> 16) & 0xff; flags = (info >> 24) & 0xff;
                SC_T0 = SC_N4 ^ (code < 4 ? SC_MX << (8 * code) : 0u); SC_T1 = SC_N4 ^ (code == 4 ? SC_MX : 0u);
            }
            if (swept_out) break;
        }
        if ((EXP & 32) || (np <= 1 && p0 == i - 1)) {
            // register predecessor: its outgoing candidates ARE this row's F and O
        } else {
            // Several predecessors: D, F and O are plain maxima over them (which predecessor won is re-derived by the
            // traceback), so the fold order is free: when the previous row is one of them (ROW_REGPRED) the registers are
            // the running maxima as they stand, otherwise the first predecessor's stored row is unpacked into them; every
            // other predecessor is folded in.
            const bool regbase = (flags & ROW_REGPRED) != 0;
            // (twin step: a row that joins the pair in front of it -- ROW_JOIN, rows i - 2 and i - 1 -- finds their maxima in the registers)
            bool joinrow = false;
            if constexpr (TWIN) joinrow = (flags & ROW_JOIN) != 0;
#define P16_NOT_PAIR(p_) (!TWIN || !joinrow || (p_) != i - 2)
            if (!regbase) {
                int hl;
                if (ring_plane && s0 >= 0 && p0 != 0) P16_FETCH_PLANE(p0, Hp, Fp, Op, hl);
                else if constexpr (CB == 2) {
                    unsigned wr[W];
                    P16_FETCH(p0, s0, wr, hl);
                    P16_DECODE(wr, hl, Hp, Fp, Op);
#pragma unroll
                    for (int k = 0; k < W; ++k) SXG_PIN("+v"(Hp[k]), "+v"(Fp[k]), "+v"(Op[k]));
                } else {
                    u32x2 wr[W];
                    P16_FETCH(p0, s0, wr, hl);
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        p16_unpack_row<SW>(wr[k], Hp[k], Fp[k], Op[k]);
                        SXG_PIN("+v"(Hp[k]), "+v"(Fp[k]), "+v"(Op[k]));
                    }
                }
                Hleft = hl;
            }
// fold one more predecessor row (p_, slot sl_) into the running maxima
#define P16_FOLD(p_, sl_)                                                                                   \
    do {                                                                                                    \
        int hl;                                                                                             \
        if constexpr (CB == 2) {                                                                            \
            int hs_[W], fs_[W], os_[W];                                                                     \
            if (ring_plane && (sl_) >= 0 && (p_) != 0) P16_FETCH_PLANE(p_, hs_, fs_, os_, hl);              \
            else { unsigned wr_[W]; P16_FETCH(p_, sl_, wr_, hl); P16_DECODE(wr_, hl, hs_, fs_, os_); }      \
            _Pragma("unroll") for (int k = 0; k < W; ++k) {                                                 \
                Fp[k] = pk_max(Fp[k], fs_[k]);                                                              \
                if (CVX) Op[k] = pk_max(Op[k], os_[k]);                                                     \
                Hp[k] = pk_max(Hp[k], hs_[k]);                                                              \
                SXG_PIN("+v"(Hp[k]), "+v"(Fp[k]), "+v"(Op[k]));                                             \
            }                                                                                               \
        } else {                                                                                            \
            u32x2 wr[W];                                                                                    \
            P16_FETCH(p_, sl_, wr, hl);                                                                     \
            _Pragma("unroll") for (int k = 0; k < W; ++k) {                                                 \
                int hs, fs, os;                                                                             \
                p16_unpack_row<SW>(wr[k], hs, fs, os);                                                      \
                Fp[k] = pk_max(Fp[k], fs);                                                                  \
                if (CVX) Op[k] = pk_max(Op[k], os);                                                         \
                Hp[k] = pk_max(Hp[k], hs);                                                                  \
                SXG_PIN("+v"(Hp[k]), "+v"(Fp[k]), "+v"(Op[k]));                                             \
            }                                                                                               \
        }                                                                                                   \
        Hleft = pk_max(Hleft, hl);                                                                          \
    } while (0)
            // (the first two predecessors in straight-line code: two-predecessor rows -- the closing node of every
            // bubble -- are a third of all rows; the loop form made the allocator spill around them)
            if (regbase && p0 != i - 1 && P16_NOT_PAIR(p0)) P16_FOLD(p0, s0);
            if (np >= 2 && p1 != i - 1 && P16_NOT_PAIR(p1)) P16_FOLD(p1, s1);
            for (int x = 2; x < np; ++x) {
                const int p = __builtin_amdgcn_readfirstlane(g_preds[pb + x]);
                if (p == i - 1 || !P16_NOT_PAIR(p)) continue;
                const int sl = p >= 1 ? __builtin_amdgcn_readfirstlane(g_slot[p - 1]) : -1;
                P16_FOLD(p, sl);
            }
#undef P16_FOLD
#undef P16_NOT_PAIR
        }
#undef P16_DRAIN
#undef P16_FETCH
#undef P16_DECODE
        if (!CVX) {
#pragma unroll
            for (int k = 0; k < W; ++k) Op[k] = NEG2;
        }

        // (the ordinary row: both parts of the fragment, every name the loop's own)
#define P16_ROW_MODE 0
#define P16_ROW_PART 3
#include "poa_dp16_row.inc.h"
#undef P16_ROW_PART
#undef P16_ROW_MODE
    }
#undef P16_LDS_ROW
#ifdef SXG_ROW_PROF
    if (t == 0 && B.row_prof)
        for (int k = 0; k < ROWP_SEGS; ++k) B.row_prof[k] += racc[k];
#endif
#undef RP_MARK
#undef P16_DEC
#undef P16_INC

    if (SW) {
        // ---- end cell of a local alignment: the wave's keys, then the workgroup's; the column is found by the traceback
        fold_keys(N + 1);
        __syncthreads();
        unsigned long long* kl = (unsigned long long*)lds;
        if (lane == 0) kl[wv] = ekey;
        __syncthreads();
        unsigned long long key = kl[0];
        for (int x = 1; x < NW; ++x) key = kl[x] > key ? kl[x] : key;
        __syncthreads();
        const int val = (int)(unsigned)(key >> 32) - BIAS;
        if (key == 0ull || val <= 0) { res.best = 0; res.bi = -1; res.bj = -1; }
        else {
            res.best = val;
            res.bi = (int)(0xFFFFFu - (unsigned)((key >> 12) & 0xFFFFFu));
            res.bj = -1 - (int)(0xFFFu - (unsigned)(key & 0xFFFu));   // -(strip + 1): see traceback_p16
        }
        return res;
    }
    // ---- end cell: greatest score, then smallest row, then smallest column (two candidates per lane)
    unsigned long long key = 0;
    if (bi_lo >= 0)
        key = ((unsigned long long)(unsigned)(best_lo + (1 << 27)) << 35) |
              ((unsigned long long)(0xFFFFFu - (unsigned)bi_lo) << 15) | (unsigned long long)(0x7FFFu - (unsigned)(j0 + bk_lo));
    if (bi_hi >= 0) {
        const unsigned long long k2 = ((unsigned long long)(unsigned)(best_hi + (1 << 27)) << 35) |
                                      ((unsigned long long)(0xFFFFFu - (unsigned)bi_hi) << 15) |
                                      (unsigned long long)(0x7FFFu - (unsigned)(j0h + bk_hi));
        key = k2 > key ? k2 : key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d);
        key = o > key ? o : key;
    }
    __syncthreads();
    unsigned long long* kl = (unsigned long long*)lds;
    if (lane == 0) kl[wv] = key;
    __syncthreads();
    key = kl[0];
    for (int x = 1; x < NW; ++x) key = kl[x] > key ? kl[x] : key;
    __syncthreads();
    if (key == 0) { res.best = 0; res.bi = -1; res.bj = -1; }
    else {
        res.best = (int)(unsigned)(key >> 35) - (1 << 27) - BIAS;
        res.bi = (int)(0xFFFFFu - (unsigned)((key >> 15) & 0xFFFFFu));
        res.bj = (int)(0x7FFFu - (unsigned)(key & 0x7FFFu));
    }
    return res;

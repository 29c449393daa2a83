// poa_dp16.hip.h -- packed-int16 DP sweep (gfx950 v_pk_add_i16 / v_pk_max_i16 / v_pk_sub_i16) and the
// traceback that DERIVES the alignment from stored values.
//
// Same semantics (S1-S5) and the same row-uniform structure as poa_dp.hip.h, but every VGPR
// holds TWO cells: lane t owns two ADJACENT strips, "lo" = columns [2t*W, (2t+1)*W) and "hi" = columns
// [(2t+1)*W, (2t+2)*W) (round 10; before that the two strips of a lane lay 64 strips apart); the low / high 16 bits of a
// register are the two strips, so every add/max serves two cells.  Measured on MI355X (profiles/ubench/valu_rate.hip): a wave64
// integer VALU instruction issues every 4 cycles whether it is 32-bit or packed 16-bit, and the
// 32-bit sweep is bound by exactly that issue rate -- packing is the lever.
//
// Round 2: the sweep records NO decisions.  No packed compare exists on gfx950, so every "which
// candidate won" bit used to be the sign of a packed difference shifted into a mask word (3 VALU
// instructions per decision, 8 decisions per packed column: a third of the row) and the mask plane was
// 40 % of the kernel's HBM writes -- for a walk that visits ~10^4 of 2.7*10^7 cells.  Now:
//  * rows carry OUTGOING gap candidates oF = max(H+g, F+e), oO = max(H+q, O+c) instead of F and O:
//    computed once at the end of a row, consumed for free by a register successor and with an unpack
//    by a stored one; a row word is packed H plus the two 8-bit distances H-oF, H-oO;
//  * every row additionally writes those words for a BAND of strips around the column where its node
//    is expected to align (the node's backbone coordinate, kept by add_alignment) to the traceback
//    plane, one dword per cell: H int16 | dF << 16 | dO << 24;
//  * the traceback re-applies the tie rules S3 to the candidates of each visited cell (executable
//    specification: oracle/poa_vtb.c, checked against the recorded-choice oracle): D from the
//    predecessors' H, F / O from their outgoing candidates, E / Q from a leftward scan of the row's own
//    H; the walk carries the value of the state it is in, so OPEN-versus-EXTEND is one equality test.
//    A cell outside the band is a BAND MISS: the hints of the rows above are shifted and the alignment's
//    sweep is repeated (rare: the band is ~1100 columns wide; see poa_block_kernel).
//  * the end cell of a local alignment is found with a packed running maximum per row and a
//    wave-uniform search of the column only in rows that improve it.
// Applicability: every reachable score and intermediate fits +-15800 (host check); otherwise the
// 32-bit sweep runs.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <utility>
#include "poa_dp.hip.h"
#include "poa_rowcode.h"
#include "poa_fields.h"

namespace sxg {

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

constexpr int NEGP = -16384;  // "minus infinity" of the packed sweep
// GLOBAL alignments whose all-gap corner scores leave int16 (affine 1,4,6,2 at 5 kbp: -20 006) still run the packed sweep
// (round 5): H is clamped at P16_NWFLOOR from below -- the same one instruction per cell that clamps a local alignment at
// 0 -- which bounds every gap state too (each is some H plus one opening at least).  A clamped cell is larger than its true
// value, and whatever it feeds gains at most m per column, so every cell with H > P16_NWFLOOR + m * L + m is EXACT, and so is
// every decision the traceback takes in such a cell (a candidate out of the clamped region cannot equal its value).  The
// traceback checks that of every cell it visits; a walk that meets a smaller H -- two sequences with little in common --
// reports ST_RANGE_OVERFLOW and the block is re-run on the 32-bit sweep, as before.  (Rounds 1-4 sent every global
// alignment whose corner did not fit down that ladder up front: 130 blocks/s instead of the packed sweep's rate.)
constexpr int P16_NWFLOOR = -16000;
// (the default scores P16_DEF_* the DS kernel classes are compiled for: poa_fields.h)
__host__ __device__ inline bool p16_default_scores(const Scoring& S) {
    return S.convex && S.m == P16_DEF_M && S.n == P16_DEF_N && S.g == P16_DEF_G && S.e == P16_DEF_E && S.q == P16_DEF_Q && S.c == P16_DEF_C;
}
// (LOCAL alignments run the packed sweep on BIASED fields: P16_BIAS, P16_FLOOR and the range they stay in -- poa_fields.h)

__device__ __forceinline__ int pk_add(int a, int b) { return __builtin_bit_cast(int, (s16x2)(__builtin_bit_cast(s16x2, a) + __builtin_bit_cast(s16x2, b))); }
__device__ __forceinline__ int pk_sub(int a, int b) { return __builtin_bit_cast(int, (s16x2)(__builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b))); }
__device__ __forceinline__ int pk_max(int a, int b) { return __builtin_bit_cast(int, __builtin_elementwise_max(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b))); }
// Three-way maximum of BIASED fields in one instruction (v_pk_maximum3_f16): exactly pk_max(pk_max(a, b), c) while every field
// of a, b, c is a pattern in [0, P16_F16_TOP] -- the local classes compiled for the default scores (poa_fields.h has the
// argument and the bound).  The builtin form, not inline asm: the scheduler and the hazard recogniser know the instruction.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int pk_max3(int a, int b, int c) {
    return __builtin_bit_cast(int, __builtin_elementwise_maximum(__builtin_elementwise_maximum(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b)), __builtin_bit_cast(f16x2, c)));
}
__device__ __forceinline__ int pk_mad(int a, int b, int c) { return __builtin_bit_cast(int, (s16x2)(__builtin_bit_cast(s16x2, a) * __builtin_bit_cast(s16x2, b) + __builtin_bit_cast(s16x2, c))); }
__device__ __forceinline__ int pk_lshr(int a, int sh) { return __builtin_bit_cast(int, (u16x2)(__builtin_bit_cast(u16x2, a) >> __builtin_bit_cast(u16x2, sh))); }
__device__ __forceinline__ int pk2(int lo, int hi) { return (lo & 0xffff) | (hi << 16); }
__device__ __forceinline__ int pk_lo(int v) { return (int)(short)(v & 0xffff); }
__device__ __forceinline__ int pk_hi(int v) { return v >> 16; }

// Row words of the packed ring, per lane and column: packed H, and the distances H - oF, H - oO
// to the row's OUTGOING gap candidates oF = max(H + g, F + e), oO = max(H + q, O + c) -- what every
// successor takes as its F / O.  H >= F and g <= e < 0 bound the distances to [-e, -g] and [-c, -q]:
// one byte each, never clamped (host check: |g|, |q| <= 120).
// (BIASED: the fields are biased and h >= of, oo field by field, so the differences are plain 32-bit subtractions)
template <bool CVX, bool BIASED = false>
__device__ __forceinline__ u32x2 p16_pack_row(int h, int of, int oo) {
    const int df = BIASED ? (int)((unsigned)h - (unsigned)of) : pk_sub(h, of);
    const int dq = BIASED ? (int)((unsigned)h - (unsigned)oo) : pk_sub(h, oo);
    return u32x2{(unsigned)h, (unsigned)(CVX ? (df | (dq << 8)) : df)};
}
template <bool BIASED = false>
__device__ __forceinline__ void p16_unpack_row(u32x2 w, int& h, int& of, int& oo) {
    h = (int)w.x;
    const int df = (int)(w.y & 0x00ff00ffu), dq = (int)((w.y >> 8) & 0x00ff00ffu);
    of = BIASED ? (int)((unsigned)h - (unsigned)df) : pk_sub(h, df);
    oo = BIASED ? (int)((unsigned)h - (unsigned)dq) : pk_sub(h, dq);
}

// 2-byte plane cells (CB = 2): row codes (P16RowCode; the banded sweep: delta codes, P16Delta), poa_rowcode.h
// dwords of one strip of a row: W + 1 halfwords
__host__ __device__ constexpr int p16_slot_dwords(int W, int CB) { return CB == 2 ? (W + 2) / 2 : W; }

// Buffer addressing for the sweep's rows: address = descriptor base (one row of the ring / of the plane,
// built per row with a few SALU instructions) + SGPR offset (column k of the strip) + ONE loop-invariant VGPR
// offset (the lane).  With global_load/store the compiler formed 64-bit VGPR addresses per access
// (v_lshl_add_u64) and kept the per-column offsets in SGPR pairs, which it then spilled to VGPR lanes
// (v_readlane per use): ~25 % of the row's VALU instructions were address bookkeeping.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t p16_rsrc(const void* base, const int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

// ---- the traceback plane of the packed sweep: a band of strips per row -------------------------
// Strip s = columns [s*W, (s+1)*W) (even s: the lo strip of lane s / 2 mod 64, odd s: its hi strip).  Row r keeps the BS strips
// starting at band_first_strip(hint of r), strip s in slot s mod BS.  A row's cells are laid out in GROUPS of four
// columns-in-strip: [group][slot][column of the group], i.e. cell (r, column j), k = j % W, slot = (j / W) % BS is the dword
//     plane[(r * W + 4 * (k / 4)) * BS + slot * gw(k / 4) + k % 4]  =  H int16 | (H - oF) << 16 | (H - oO) << 24,
// gw(group) = min(4, W - 4 * group).  A lane then writes (reads) its strip with ceil(W / 4) 16-byte instructions, each of
// which covers 1 KB of consecutive memory per wave (round 4; rounds 1-3 had [column][slot]: W four-byte instructions of
// 256 B each -- the packed sweep's band stores were 24 % of its launch, most of it instruction issue and the vmcnt they hold).
// BS is a multiple of 4: rows and groups start on 16-byte boundaries.
// (geometries of up to 1408 columns keep every strip: the band would cover most of the row anyway, and a plane that holds
//  whole rows doubles as the row ring -- see ring_plane in dp_fill_p16)
__host__ __device__ constexpr int p16_band_strips(int T, int W) {
    return 2 * T * W <= 1408 ? 2 * T : (plane_round4((1100 + W - 1) / W) < 2 * T ? plane_round4((1100 + W - 1) / W) : 2 * T);
}
// Adaptive band (round 8): the strips one alignment keeps, from the largest |path column - hint| the block's earlier walks
// saw (`drift`) plus `margin` columns.  band_first_strip centres the band on the hint's strip, so every column within
// (BS / 2 - 1) * W of the hint is kept: BS = 2 (ceil((drift + margin) / W) + 1), rounded up to 4, at least lo, and never
// more than cap (the plane's arena is sized for cap strips per row; a cap narrowed below lo by SXG_POA_BAND_COLS wins).
// (defaults of BlockArgs::band_floor, band_margin, band_full -- see sxg_poa.hip::band_adapt_args.  Measured on the headline,
//  1000 x 64 x 5 kbp: floor 48 strips, margin 96 columns keep 54-64 strips per row on average, with 0.4 % of the sweeps
//  repeated; floor 32, margin 64 keep 41-55 strips but repeat twice as many sweeps, and the launch was no faster)
constexpr int P16_BAND_FLOOR = 48, P16_BAND_MARGIN = 96, P16_BAND_FULL = 2;
__host__ __device__ constexpr int p16_drift_strips(int drift, int margin, int W, int lo, int cap) {
    const int bs = plane_round4(2 * ((drift + margin + W - 1) / W + 1));
    return (bs < lo ? lo : bs) < cap ? (bs < lo ? lo : bs) : cap;
}
static_assert(p16_drift_strips(0, 96, 8, 48, 12) == 12 && p16_drift_strips(300, 96, 11, 48, 100) == 76 &&
              p16_drift_strips(0, 96, 11, 48, 100) == 48, "adaptive band: floor, then the arena's cap");
template <int W>
__device__ __forceinline__ size_t plane_cell(const size_t row, const int BS, const int slot, const int k) {
    return row * (size_t)(W * BS) + (size_t)plane_cell_in_row(W, BS, slot, k);   // (poa_types.h)
}
// byte offset of cell k of slot `slot` inside its row (for buffer accesses through a per-row descriptor)
template <int W>
__device__ __forceinline__ unsigned plane_cell_byte(const int BS, const unsigned slot, const int k) {
    return (unsigned)plane_cell_in_row(W, BS, (int)slot, k) * 4u;
}
// Cache policy of the plane stores: NON-TEMPORAL (aux bit 1 = nt).  The plane is written once per row and read back by the
// traceback for ~1 % of its cells (the banded sweep: by 40 % of the rows, a few rows later); streamed past the L2 it stops evicting
// the ring rows and descriptors that ARE re-read.  Same box, one gpurun call: headline 1 987 -> 1 922 ms, c3b 1 400 -> 1 514
// blocks/s, c2 +5 %.  (nt on the ring stores as well: +-0 on the headline; nt on the banded sweep's plane LOADS: c3b -2 %.)
#ifndef SXG_PLANE_AUX
#define SXG_PLANE_AUX 2
#endif
// a slot no row has: slot * (bytes of a group) lies beyond every row's buffer descriptor and stays below 2^32 (see P16_STORES)
#define P16_SLOT_OOB 0x04000000u
// one strip of a row: cell(k) -> the dword of column k; rs = the row's descriptor
template <int W, int GI, class F>
__device__ __forceinline__ void plane_store_group(const __amdgpu_buffer_rsrc_t rs, const unsigned slot, const int BS, F& cell) {
    constexpr int k = 4 * GI, gw = W - k >= 4 ? 4 : W - k;
    // The group's offset travels in the VGPR offset, the SGPR offset field stays 0: a store of more than 64 bits reads its
    // upper data registers after it has issued, and the compiler only keeps the next VALU write away from them (the "VMEM
    // store data" hazard) when the SGPR offset field is NOT a register -- with `s_offset` = GI * BS * 16 it scheduled the next
    // group's v_perm right behind the store, and on gfx950 the stored cells were then the NEXT group's (measured: band misses
    // on every deep block; the same layout with dword stores was exact).
    const unsigned vo = slot * (unsigned)(gw * 4) + (unsigned)(GI * BS * 16);
#ifdef SXG_PLANE_NARROW
    for (int x = 0; x < gw; ++x) __builtin_amdgcn_raw_buffer_store_b32(cell(k + x), rs, vo, 4 * x, 0);
    return;
#endif
    if constexpr (gw == 4)
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{cell(k), cell(k + 1), cell(k + 2), cell(k + 3)}, rs, vo, 0, SXG_PLANE_AUX);
    else if constexpr (gw == 3)
        __builtin_amdgcn_raw_buffer_store_b96(u32x3{cell(k), cell(k + 1), cell(k + 2)}, rs, vo, 0, SXG_PLANE_AUX);
    else if constexpr (gw == 2)
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{cell(k), cell(k + 1)}, rs, vo, 0, SXG_PLANE_AUX);
    else
        __builtin_amdgcn_raw_buffer_store_b32(cell(k), rs, vo, 0, SXG_PLANE_AUX);
}
template <int W, class F, int... GI>
__device__ __forceinline__ void plane_store_groups(const __amdgpu_buffer_rsrc_t rs, const unsigned slot, const int BS, F& cell, std::integer_sequence<int, GI...>) {
    (plane_store_group<W, GI>(rs, slot, BS, cell), ...);
}
template <int W, class F>
__device__ __forceinline__ void plane_store_strip(const __amdgpu_buffer_rsrc_t rs, const unsigned slot, const int BS, F cell) {
    plane_store_groups<W>(rs, slot, BS, cell, std::make_integer_sequence<int, (W + 3) / 4>{});
}
template <int W, int GI>
__device__ __forceinline__ void plane_load_group(const __amdgpu_buffer_rsrc_t rs, const unsigned slot, const int BS, unsigned (&out)[W]) {
    constexpr int k = 4 * GI, gw = W - k >= 4 ? 4 : W - k;
    if constexpr (gw == 4) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, slot << 4, GI * BS * 16, 0);
        out[k] = v.x; out[k + 1] = v.y; out[k + 2] = v.z; out[k + 3] = v.w;
    } else if constexpr (gw == 3) {
        const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(rs, slot * 12u, GI * BS * 16, 0);
        out[k] = v.x; out[k + 1] = v.y; out[k + 2] = v.z;
    } else if constexpr (gw == 2) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, slot << 3, GI * BS * 16, 0);
        out[k] = v.x; out[k + 1] = v.y;
    } else
        out[k] = __builtin_amdgcn_raw_buffer_load_b32(rs, slot << 2, GI * BS * 16, 0);
}
template <int W, int... GI>
__device__ __forceinline__ void plane_load_groups(const __amdgpu_buffer_rsrc_t rs, const unsigned slot, const int BS, unsigned (&out)[W], std::integer_sequence<int, GI...>) {
    (plane_load_group<W, GI>(rs, slot, BS, out), ...);
}
template <int W>
__device__ __forceinline__ void plane_load_strip(const __amdgpu_buffer_rsrc_t rs, const unsigned slot, const int BS, unsigned (&out)[W]) {
    plane_load_groups<W>(rs, slot, BS, out, std::make_integer_sequence<int, (W + 3) / 4>{});
}
// one strip of a row through a plain pointer (the traceback: every lane its own row): group by group, as wide as the group
template <int SDW>
__device__ __forceinline__ void plane_load_slot(SXG_GLOBAL const uint32_t* const row, const int BS, const int slot, unsigned (&out)[SDW]) {
#pragma unroll
    for (int gi = 0; gi < (SDW + 3) / 4; ++gi) {
        const int gw = SDW - 4 * gi >= 4 ? 4 : SDW - 4 * gi;
        SXG_GLOBAL const uint32_t* const q = row + 4 * gi * BS + slot * gw;
        if (gw == 4) { const u32x4 v = *(SXG_GLOBAL const u32x4*)q; out[4 * gi] = v.x; out[4 * gi + 1] = v.y; out[4 * gi + 2] = v.z; out[4 * gi + 3] = v.w; }
        else if (gw == 3) { typedef u32x3 __attribute__((aligned(4))) u32x3_a4; const u32x3 v = *(SXG_GLOBAL const u32x3_a4*)q; out[4 * gi] = v.x; out[4 * gi + 1] = v.y; out[4 * gi + 2] = v.z; }
        else if (gw == 2) { const u32x2 v = *(SXG_GLOBAL const u32x2*)q; out[4 * gi] = v.x; out[4 * gi + 1] = v.y; }
        else out[4 * gi] = *q;
    }
}
__device__ __forceinline__ int band_first_strip(const int hint_col, const int W, const int BS, const int T) {
    const int c = hint_col / W - (BS >> 1);
    return min(max(c, 0), 2 * T - BS);
}

#ifndef SXG_P16_INLINE
#define SXG_P16_INLINE __noinline__
#endif
// (out of line, views by value: inlined into the persistent kernel the sweep shared ~100 SGPRs with the
// kernel's own state and reloaded its loop-invariant scalars from VGPR lanes -- v_readlane + hazard nops --
// all over the row loop)
// EXP (development, profiles/tools/cost_map.sh): bits switch parts of the row OFF in a sweep whose results are thrown away
// (the kernel runs it in front of the real one), so that the difference between two builds prices a part of the row:
// 1 = no band stores, 2 = no ring stores, 4 = no end-cell bookkeeping, 8 = no carry scans, 16 = no mailbox exchange,
// 32 = every row takes the register-predecessor path (no fetch, no fold), 64 = no pass 2, 128 = no pass 1.
// CB: bytes per plane cell (2: the stored rows' code, see P16RowCode; 4: H | H - oF | H - oO).
// End cell of a LOCAL alignment (round 5): every lane keeps, per strip, ONE 32-bit key -- the strip's greatest H so far in the
// upper half, 0xffff minus the row that first reached it in the lower -- updated with a max per row (5 instructions; rounds 2-4
// compared, voted and searched the strip's columns in every row that improved any lane, i.e. nearly every row of the waves the
// best diagonal runs through: 15 % of the row on 1 kbp blocks).  Rows are numbered within epochs of 65536; at an epoch's end the
// wave folds its keys into a scalar 64-bit best.  The sweep returns the STRIP of the end cell (bj = -(strip + 1)); the
// traceback reads the column out of the plane row it starts from.
// RP: the class may run with a plane that keeps every strip and read stored rows back from it (ring_plane below) -- the
// one- and two-wave classes (TMAX = 128); the wider classes are compiled without that path (its three fetch sites and their
// scalars cost the four-wave headline class SGPR spills in the row loop).
// (RP: 0 = never; 1 = when the launch's plane keeps every strip, a run-time test; 2 = ALWAYS -- round 6: the one-wave classes up to W = 11
//  cover at most 1 408 columns, their plane keeps every strip by construction (p16_band_strips), and compiled for that alone the fold has
//  ONE form: with both, every fold ended in 30 v_mov that merged the two forms' registers.  The host sends a one-wave launch whose plane
//  was narrowed -- the test knob SXG_POA_BAND_COLS -- to the two-wave class run at 64 threads.)
// TWIN (round 13): the class sweeps a row that carries ROW_TWIN together with the row behind it, and a ROW_JOIN row takes the
// pair out of the registers (poa_graph_dev.h::twin_flags sets both for the classes with class_traits().twin).  One body
// (poa_dp16_fill.inc.h; a row's passes and stores: poa_dp16_row.inc.h) in two out-of-line functions: dp_fill_p16 (no twin step:
// the rows every class ran before round 13, from the same tokens) and dp_fill_p16_twin.
template <int W, bool CVX, bool SW, int CB = 4, int RP = 0, int TFIX = 0, bool DS = false, int EXP = 0>
__device__ SXG_P16_INLINE DpResult dp_fill_p16(const Scoring S, const RowsView R, const int N_,
                                             const uint8_t* seq, const int L_, const DpBuffers B,
                                             char* smem) {
    constexpr bool TWIN = false;
#include "poa_dp16_fill.inc.h"
}
template <int W, bool CVX, bool SW, int CB = 4, int RP = 0, int TFIX = 0, bool DS = false, int EXP = 0>
__device__ SXG_P16_INLINE DpResult dp_fill_p16_twin(const Scoring S, const RowsView R, const int N_,
                                                  const uint8_t* seq, const int L_, const DpBuffers B,
                                                  char* smem) {
    static_assert(CB == 2 && RP == 0, "the twin step: 2-byte cells, stored rows in the ring or on the chip");
    constexpr bool TWIN = true;
#include "poa_dp16_fill.inc.h"
}

// ---------------------------------------------------------------------------------------------------
// Traceback of the packed sweep: the alignment is DERIVED from the plane's values (rules: header of this
// file and oracle/poa_vtb.c).  The walk is a chain of dependent reads, so the whole of wave 0 takes part:
// lane l fetches, in two round trips, what a step through row (top - l) can need -- the row descriptor,
// the node id and the plane cells of 8 columns around the column where the alignment is expected to cross
// that row (L/N columns per graph row) -- into an LDS window of 64 rows; the walk itself runs out of LDS on
// the scalar unit (every lane executes it redundantly, lane 0 writes) and returns to HBM only for a cell
// the window does not hold (an indel run, a predecessor far up the order) and for the leftward scans that
// resolve a gap in the graph (E/Q), which all 64 lanes do together, 64 columns per round trip.
constexpr int TBW_ROWS = 64;
constexpr int TBW_STRIDE = 13;  // dwords per window row (odd: conflict-free fills)
constexpr int TBW_COLS = 8;     // plane cells per window row
// window row: TBW_COLS cells, then
enum : int { EO_PB = 8, EO_INFO = 9, EO_Q0 = 10, EO_Q1 = 11, EO_NODE = 12 /* node | valid-cell mask << 24 */ };
constexpr int TBW_LET = 128;    // query letters of columns jtop, jtop-1, ... kept beside the window
static_assert((TBW_ROWS * TBW_STRIDE + TBW_LET) * 4 <= LDS_META_BYTES / 2, "traceback window lives in the descriptor area");

// words of LDS (control area) through which the walk reports a band miss to the workgroup
enum : int { TBM_FLAG = 208, TBM_ROW = 209, TBM_DELTA = 210, TBM_RANGE = 211 /* a clamped cell on the walk: see P16_NWFLOOR */ };

// BANDED (poa_band16.hip.h): a row keeps exactly the strips of its band, max(0, hint - w) / W .. (hint + w) / W, and a
// cell outside the band does not exist (it reads as -inf and is never a miss).
// CB = 2: the plane holds 2-byte codes (row codes; BANDED: delta codes -- poa_rowcode.h); the helpers below rebuild the cells
// the walk asks for -- H by summing a strip's steps from its left end -- in the round-4 word format (H | H - oF | H - oO), so the
// walk itself is the same code.
// j < 0 on entry: the sweep of a local alignment names the STRIP of the end cell, -(strip + 1); the column is the first
// of that strip's cells in row i that holds the best score.
// STRICT: the caller admitted the alignment under the strict range rule (every cell above P16_NWFLOOR: nothing is ever clamped,
// sxg_poa.hip::p16_safe without clamp_ok -- the align-only kernel, which has no wider re-run): the walk takes every cell at its word.
template <bool PAIRS, int W, bool CVX, bool BANDED = false, int CB = 4, bool STRICT = false>
// (views by value: a reference to the kernel's private copy trips an AMDGPU back-end assertion on
// the private-aperture null check for some strip widths)
__device__ __noinline__ int traceback_p16(const RowsView R, const DpBuffers B, const Scoring S_, const uint8_t* seq, const int L_,
                                          const int best_, const int T_, const int slope_, int i, int j, int32_t* posnode,
                                          int32_t* pair_row, int32_t* pair_pos, char* smem) {
    // arguments arrive in vector registers: make the uniform ones scalar again
    const int T = __builtin_amdgcn_readfirstlane(T_), best = __builtin_amdgcn_readfirstlane(best_);
    const int L = __builtin_amdgcn_readfirstlane(L_);
    // columns the alignment advances per graph row, in 1/256: a graph of N rows against L letters is
    // walked at about L/N columns per row (rows of other branches are skipped), which is where the
    // window is laid
    const int slope = __builtin_amdgcn_readfirstlane(slope_);
    i = __builtin_amdgcn_readfirstlane(i); j = __builtin_amdgcn_readfirstlane(j);
    const int sm = __builtin_amdgcn_readfirstlane(S_.m), sn = __builtin_amdgcn_readfirstlane(S_.n);
    const int g = __builtin_amdgcn_readfirstlane(S_.g), e = __builtin_amdgcn_readfirstlane(S_.e);
    const int q = __builtin_amdgcn_readfirstlane(S_.q), c = __builtin_amdgcn_readfirstlane(S_.c);
    const int sw = __builtin_amdgcn_readfirstlane(S_.sw);
    // the full-matrix sweep of a local alignment stores biased H (P16_BIAS): "zero" is the bias
    const int bias = (!BANDED && sw) ? P16_BIAS : 0;
    const int BS = __builtin_amdgcn_readfirstlane(B.band_strips);
    const int bw = __builtin_amdgcn_readfirstlane(B.band_w), last_strip = L / W;
    // adaptive band (B4): the sweep left every row's band -- first | last strip << 16 -- in word 6 of its descriptor
    const bool ada = BANDED && __builtin_amdgcn_readfirstlane(B.band_mode) == 2;
    const int HW = ada ? 6 : 7;   // descriptor word that says which strips the row kept
    // The adaptive sweep rewrote words 6, 7 of every row descriptor with device-scope (sc1) stores; the chunk the sweep
    // staged earlier may still sit in this CU's L1, and __syncthreads does not invalidate it: drop the L1 copies once per
    // walk (buffer_inv sc1) so that the plain loads below see the band words the sweep left.
    if (ada) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // is strip s of a row with band hint `hint` kept in the plane?
    auto kept = [&](int hint, int s) -> bool {
        if (BANDED) {
            if (ada) return s >= (hint & 0xffff) && s <= (int)((unsigned)hint >> 16);
            return s >= max(hint - bw, 0) / W && s <= min((hint + bw) / W, last_strip);
        }
        return (unsigned)(s - band_first_strip(hint, W, BS, T)) < (unsigned)BS;
    };
    // (BANDED with CB = 2 -- round 6, local alignment: every strip starts with the H of its OWN first column and a step of 0, the
    //  packed sweep's "strip 0" form, so the decoders below need nothing of a strip's left neighbour; strips are ABSOLUTE there)
    constexpr int SD = p16_slot_dwords(W, CB);     // dwords of one strip in a plane row
    // (CB = 2) fields of a cell's code
    const P16Delta DF = p16_delta_of(S_);
    const int dbH = __builtin_amdgcn_readfirstlane(DF.bH), dbF = __builtin_amdgcn_readfirstlane(DF.bF);
    // Which code the plane holds: the full-matrix sweep writes row codes (round 11: the ONE code of its stored rows and its
    // plane), the banded sweep its delta codes.  Both decode through poa_rowcode.h: p16_code_step (one column: the step of H and
    // the two distances) and p16_strip_decode (column k of a strip, summing the steps from its left end).
    constexpr bool DELTA = BANDED;
    P16Delta DT;
    DT.bH = dbH; DT.bF = dbF; DT.bO = __builtin_amdgcn_readfirstlane(DF.bO);
    DT.g = __builtin_amdgcn_readfirstlane(DF.g); DT.eabs = __builtin_amdgcn_readfirstlane(DF.eabs); DT.cabs = __builtin_amdgcn_readfirstlane(DF.cabs);
    // the cell word the walk reads, given H and the distances H - oF, H - oO
    auto d_word = [&](const int h, const int df, const int dq) -> uint32_t {
        return ((uint32_t)h & 0xffffu) | ((uint32_t)df << 16) | ((uint32_t)dq << 24);
    };
    // outputs and letters through global pointers: a FLAT store also counts on lgkmcnt, and the walk
    // waits on lgkmcnt for its LDS reads every step -- i.e. it would wait for the previous step's store to
    // reach HBM
    SXG_GLOBAL int32_t* const g_posnode = sxg_global(posnode);
    SXG_GLOBAL int32_t* const g_pair_row = sxg_global(pair_row);
    SXG_GLOBAL int32_t* const g_pair_pos = sxg_global(pair_pos);
    SXG_GLOBAL const uint8_t* const g_seq = sxg_global(seq);
    SXG_GLOBAL const uint32_t* const g_plane = sxg_global((const uint32_t*)B.tb);
    SXG_GLOBAL const int32_t* const g_meta = sxg_global((const int32_t*)R.meta);
    SXG_GLOBAL const int32_t* const g_preds = sxg_global((const int32_t*)R.preds);
    SXG_GLOBAL const int32_t* const g_row_node = sxg_global((const int32_t*)R.row_node);
    const int lane = threadIdx.x & 63;
    int* ctl = (int*)smem;
    // the block's only serial phase (the other waves wait for this one): a dependent-read chain that
    // rarely has an instruction ready, so top priority costs the co-residents next to nothing
    __builtin_amdgcn_s_setprio(3);
    uint32_t* win = (uint32_t*)(smem + LDS_CTL_BYTES);
    const int WR = TBW_ROWS;  // window rows
    uint32_t* wlet = win + TBW_ROWS * TBW_STRIDE;  // [TBW_LET] query letters of columns jtop, jtop-1, ...
    // Diagonal steps are precomputed for the whole window by all 64 lanes (lane l: the 8 cells of row wtop - l): a word
    // per cell saying "from here the walk takes a D step to window cell (l', x')" -- or 0 when the cell needs the
    // general code below (a gap, three or more predecessors, a cell the window does not hold, the end of a local
    // alignment).  The serial part of a run of matches/mismatches is then one LDS read per step instead of ~150
    // scalar instructions, and its outputs are written by 64 lanes at once.  Lives in the parked-row area of the
    // sweep (free during the walk).
    uint32_t* trans = (uint32_t*)(smem + LDS_CTL_BYTES + dp16_meta_bytes(T));   // [TBW_ROWS][TBW_COLS]
    uint32_t* chain = trans + TBW_ROWS * TBW_COLS;                               // [TBW_ROWS] cells of the current run
    int* whint = (int*)(chain + TBW_ROWS);                                        // [TBW_ROWS] backbone hint of every window row (the last 256 of the area's 2 560 bytes)
    const int kmax_e = CVX ? 1 + (g - q) / (c - e) : 0x7fffffff;  // longest gap the first piece can win (poa_vtb.c)
#define TBU(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
    // H of the virtual row 0
    auto h_row0 = [&](int col) -> int {
        if (sw || col <= 0) return bias;
        const int a = g + (col - 1) * e, b = q + (col - 1) * c;
        return max(a > b ? a : b, BANDED ? NEGP : P16_NWFLOOR);
    };
    // global alignment on the full matrix: cells at or below `thr` may be clamped ones (see P16_NWFLOOR); the walk must not
    // take a decision in one
    const int thr = (!BANDED && !STRICT && !sw) ? P16_NWFLOOR + sm * L + sm : -0x40000000;
    bool range = false;
    int wtop = -1, wj = 0;
    bool miss = false;
    int miss_row = 0, miss_delta = 0;
    // plane cell (row p >= 1, column col) straight from HBM; a cell outside the row's band is a miss
    auto gcell = [&](int p, int col) -> uint32_t {
        const int hint = (int)TBU(g_meta[8 * (size_t)(p - 1) + HW]);
        const int s = col / W, k = col - s * W;
        if (!kept(hint, s)) {
            if (BANDED) return 0x0000C000u;   // (NEGCELL: H = -inf)
            if (!miss) { miss = true; miss_row = p; miss_delta = col - hint; }
            return 0u;
        }
        if constexpr (CB == 2) {
            // lanes 0 .. SD-1 fetch the strip's dwords; the steps up to column k are summed on the scalar unit
            const unsigned dw = lane < SD ? g_plane[(size_t)p * (size_t)(SD * BS) + (size_t)plane_cell_in_row(SD, BS, s % BS, min(lane, SD - 1))] : 0u;
            int h, of, oo;
            p16_strip_decode<CVX, DELTA>([&](const int hw) -> unsigned {
                    const unsigned d = TBU(__builtin_amdgcn_readlane((int)dw, hw >> 1));
                    return (hw & 1) ? d >> 16 : d & 0xffffu; }, k, h, of, oo, DT);
            return d_word(h, h - of, h - oo);
        }
        return TBU(g_plane[plane_cell<W>((size_t)p, BS, s % BS, k)]);
    };
    int wgeo = slope;   // slope the current window was laid out with
    auto wcol0 = [&](int l) -> int { return wj - ((l * wgeo) >> 8) - (TBW_COLS - 3); };  // first column the window holds of row wtop-l
    auto cell = [&](int p, int col) -> uint32_t {
        const int l = wtop - p;
        if (wtop >= 0 && (unsigned)l < (unsigned)WR) {
            const int x = col - wcol0(l);
            if ((unsigned)x < (unsigned)TBW_COLS && ((TBU(win[l * TBW_STRIDE + EO_NODE]) >> (24 + x)) & 1u))
                return TBU(win[l * TBW_STRIDE + x]);
        }
        return gcell(p, col);
    };
    auto sext = [](uint32_t w) -> int { return (int)(short)(w & 0xffffu); };
    // ---- window fills in two halves (round 5): win_issue sends a window's loads (lane l: row top - l -- descriptor, node id, the
    // plane cells around the column where the walk is expected to cross that row, and two query letters), win_commit decodes
    // them into the LDS window and precomputes the diagonal runs.  The NEXT window is issued as soon as the current one is
    // committed, at the place the running slope predicts, and committed without a round trip when the walk enters it there
    // (rounds 2-4: every window was two dependent round trips, half of the walk's time on 1 kbp blocks).
    constexpr int NSW = CB == 2 ? (W >= 8 ? 2 : 3) : 1;            // strips a lane fetches (CB = 2: whole strips)
    constexpr int NRAW = CB == 2 ? NSW * SD : TBW_COLS;
    struct WinRaw { i32x4 d0, d1; int node; unsigned cells[NRAW]; uint32_t let0, let1; };
    auto win_issue = [&](const int top, const int jj, const int slp, WinRaw& R_) {
        const int row = top - lane;
        R_.d0 = i32x4{0, 0, 0, 0}; R_.d1 = R_.d0; R_.node = 0;
#pragma unroll
        for (int x2 = 0; x2 < NRAW; ++x2) R_.cells[x2] = 0u;
        if (row >= 1) {
            SXG_GLOBAL const i32x4* dm = (SXG_GLOBAL const i32x4*)(g_meta + 8 * (size_t)(row - 1));
            R_.d0 = dm[0]; R_.d1 = dm[1];
            R_.node = g_row_node[row - 1];
            const int c0 = jj - ((lane * slp) >> 8) - (TBW_COLS - 3);
            // (a cell's address does not depend on the row's band start: cells and descriptor travel together)
            if constexpr (CB == 2) {
                const int s0w = max(c0, 0) / W;
#pragma unroll
                for (int si = 0; si < NSW; ++si) {
                    unsigned tmp[SD];
                    plane_load_slot<SD>(g_plane + (size_t)row * (size_t)(SD * BS), BS, min(s0w + si, BANDED ? last_strip : 2 * T - 1) % BS, tmp);
#pragma unroll
                    for (int x2 = 0; x2 < SD; ++x2) R_.cells[si * SD + x2] = tmp[x2];
                }
            } else {
#pragma unroll
                for (int x2 = 0; x2 < TBW_COLS; ++x2) {
                    const int col = min(max(c0 + x2, 0), L);
                    const int s = col / W, k = col - s * W;
                    R_.cells[x2] = g_plane[plane_cell<W>((size_t)row, BS, s % BS, k)];
                }
            }
        }
        // (letters: one per column; the walk never reads them from HBM -- a global load inside a step
        // makes the compiler wait for vmcnt(0) there, i.e. for the previous step's output store)
        R_.let0 = (jj - lane >= 1) ? (uint32_t)g_seq[jj - lane - 1] : 255u;
        R_.let1 = (jj - 64 - lane >= 1) ? (uint32_t)g_seq[jj - 64 - lane - 1] : 255u;
    };
    // (the window's geometry -- wtop, wj, wgeo -- is set by the caller before the commit)
    auto win_commit = [&](const WinRaw& R_) {
        const int row = wtop - lane;
        if (row >= 1 && lane < WR) {
            const i32x4 d0 = R_.d0, d1 = R_.d1;
            const int c0 = wcol0(lane);
            uint32_t v[TBW_COLS], valid = 0;
            uint32_t* en = win + lane * TBW_STRIDE;
            if constexpr (CB == 2) {
                // whole strips of the row, from the one that holds the window's first column: every strip is decoded from
                // its left end and each cell that falls into the window goes straight to its place in my window row
                const int s0w = max(c0, 0) / W;
#pragma unroll
                for (int x2 = 0; x2 < TBW_COLS; ++x2) v[x2] = 0u;
#pragma unroll
                for (int si = 0; si < NSW; ++si) {
                    int h = (int)(short)(R_.cells[si * SD] & 0xffffu), df = 0, dq = 0;
                    const int xb = (s0w + si) * W - c0;   // window place of the strip's first column
#pragma unroll
                    for (int k = 0; k < W; ++k) {
                        const unsigned dwk = R_.cells[si * SD + ((1 + k) >> 1)];
                        p16_code_step<CVX, DELTA>(((1 + k) & 1) ? dwk >> 16 : dwk & 0xffffu, h, df, dq, DT);
                        if ((unsigned)(xb + k) < (unsigned)TBW_COLS && s0w + si <= (BANDED ? last_strip : 2 * T - 1)) en[xb + k] = d_word(h, df, dq);
                    }
                }
            } else {
#pragma unroll
                for (int x2 = 0; x2 < TBW_COLS; ++x2) v[x2] = R_.cells[x2];
            }
#pragma unroll
            for (int x2 = 0; x2 < TBW_COLS; ++x2) {
                const int col = c0 + x2;
                if (col >= 0 && col <= L) {
                    if (kept(ada ? d1.z : d1.w, col / W)) valid |= 1u << x2;
                    else if (BANDED) { if constexpr (CB == 2) en[x2] = 0x0000C000u; else v[x2] = 0x0000C000u; valid |= 1u << x2; }
                }
            }
            if constexpr (CB != 2) {
#pragma unroll
                for (int x2 = 0; x2 < TBW_COLS; ++x2) en[x2] = v[x2];
            }
            en[EO_PB] = (uint32_t)d0.x; en[EO_INFO] = (uint32_t)d0.y; en[EO_Q0] = (uint32_t)d0.z; en[EO_Q1] = (uint32_t)d1.x;
            en[EO_NODE] = (uint32_t)R_.node | (valid << 24);
            whint[lane] = d1.w;
        }
        wlet[lane] = R_.let0;
        wlet[64 + lane] = R_.let1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        {   // D transitions of my row's cells (rule D of poa_vtb.c, rows with one or two predecessors)
            const int row2 = wtop - lane;
            uint32_t tw[TBW_COLS];
#pragma unroll
            for (int x2 = 0; x2 < TBW_COLS; ++x2) tw[x2] = 0u;
            if (row2 >= 1 && lane < WR) {
                const uint32_t* me = win + lane * TBW_STRIDE;
                const uint32_t nv = me[EO_NODE];
                const int inf2 = (int)me[EO_INFO], np2 = inf2 & 0xffff, code2 = (inf2 >> 16) & 0xff;
                const int pa = (int)me[EO_Q0], pbb = (int)me[EO_Q1];
                const int c0 = wcol0(lane);
                if (np2 >= 1 && np2 <= 2 && pa >= 1 && (np2 == 1 || pbb >= 1)) {
                    const int la = wtop - pa, lb = np2 == 2 ? wtop - pbb : la;
                    if ((unsigned)la < (unsigned)WR && (unsigned)lb < (unsigned)WR) {
                        const int ca = wcol0(la), cb = wcol0(lb);
                        const uint32_t nva = win[la * TBW_STRIDE + EO_NODE], nvb = win[lb * TBW_STRIDE + EO_NODE];
#pragma unroll
                        for (int x2 = 0; x2 < TBW_COLS; ++x2) {
                            const int col = c0 + x2;
                            const int xa = col - 1 - ca, xb = col - 1 - cb, lo = wj - col;
                            if (!((nv >> (24 + x2)) & 1u) || col < 1 || (unsigned)xa >= (unsigned)TBW_COLS || (unsigned)xb >= (unsigned)TBW_COLS ||
                                (unsigned)lo >= (unsigned)TBW_LET) continue;
                            if (!((nva >> (24 + xa)) & 1u) || !((nvb >> (24 + xb)) & 1u)) continue;
                            const int hcell = sext(me[x2]);
                            if ((sw && hcell == bias) || hcell <= thr) continue;
                            const int ha = sext(win[la * TBW_STRIDE + xa]), hb = np2 == 2 ? sext(win[lb * TBW_STRIDE + xb]) : ha;
                            const bool second = np2 == 2 && hb > ha;    // (first predecessor in list order on ties)
                            const int best2 = second ? hb : ha;
                            if (best2 + ((int)wlet[lo] == code2 ? sm : sn) == hcell)
                                tw[x2] = 0x80000000u | (uint32_t)(second ? lb : la) | ((uint32_t)(second ? xb : xa) << 6);
                        }
                    }
                }
            }
            if (lane < WR) {
#pragma unroll
                for (int x2 = 0; x2 < TBW_COLS; ++x2) trans[lane * TBW_COLS + x2] = tw[x2];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };
    WinRaw pf;                     // the window asked for ahead of the walk
    int pf_top = -1, pf_j = 0, pf_slope = 0;
    int wslope = slope;            // running estimate of the columns the walk advances per row (1/256)
    int n = 0;
    int st = SRC_STOP;           // SRC_STOP = "in H", SRC_F / SRC_O = walking up a gap in the sequence
    int hv = best + bias, gv = 0;       // H of the current cell / value of the gap state being walked
#ifdef SXG_ROW_PROF
    unsigned long long tb_steps = 0, tb_loads = 0, tb_t0 = __builtin_readcyclecounter(), tb_ld = 0, tb_hits = 0;
#endif
    if (j < 0) {
        // The sweep of a local alignment found the end cell's row and STRIP (dp_fill_p16): its column is the first cell of
        // that strip, in row i, that holds the score.  A strip the row did not keep is a band miss like any other.
        const int s = -1 - j;
        const int hint = (int)TBU(g_meta[8 * (size_t)(i - 1) + HW]);
        j = 0;
        if (!kept(hint, s)) { miss = true; miss_row = i; miss_delta = s * W + W / 2 - hint; }
        else {
            int kf = -1;
            if constexpr (CB == 2) {
                const unsigned dw = lane < SD ? g_plane[(size_t)i * (size_t)(SD * BS) + (size_t)plane_cell_in_row(SD, BS, s % BS, min(lane, SD - 1))] : 0u;
                int h = (int)(short)(TBU(__builtin_amdgcn_readlane((int)dw, 0)) & 0xffffu), df = 0, dq = 0;
                for (int t2 = 0; t2 < W && kf < 0; ++t2) {
                    const unsigned d = TBU(__builtin_amdgcn_readlane((int)dw, (t2 + 1) >> 1));
                    p16_code_step<CVX, DELTA>(((t2 + 1) & 1) ? d >> 16 : d & 0xffffu, h, df, dq, DT);
                    if (h == hv) kf = t2;
                }
            } else {
                const uint32_t cw = lane < W ? g_plane[plane_cell<W>((size_t)i, BS, s % BS, min(lane, W - 1))] : 0u;
                const unsigned long long meq = __ballot(lane < W && sext(cw) == hv);
                if (meq) kf = (int)__builtin_ctzll(meq);
            }
            if (kf < 0) { miss = true; miss_row = i; miss_delta = 0; }   // (cannot happen: the strip's key came from these cells)
            else j = s * W + kf;
        }
    }
    while (!miss) {
#ifdef SXG_ROW_PROF
        ++tb_steps;
#endif
        if (i == 0) {
            if (j == 0 || sw) break;
            if (PAIRS && lane == 0) { g_pair_row[n] = 0; g_pair_pos[n] = j - 1; }
            ++n; --j;
            continue;
        }
        if (sw && st == SRC_STOP && hv == bias) break;
        if (st == SRC_STOP && hv <= thr) { range = true; break; }
        {   // (re)fill the window when row i or column j leave it
            const int l = wtop - i;
            const int x = j - wcol0(l);
            if (wtop < 0 || l < 0 || l > WR - 3 || x < 2 || x >= TBW_COLS) {
#ifdef SXG_ROW_PROF
                ++tb_loads;
                const unsigned long long tl0 = __builtin_readcyclecounter();
#endif
                // the slope the walk really had across the window it leaves (rows of other branches are skipped, so it differs from
                // L / N locally), blended into the running estimate
                if (wtop >= 0 && wtop > i) {
                    const int est = ((wj - j) << 8) / (wtop - i);
                    wslope = min(max((wslope + est) >> 1, 16), 512);
                }
                // the window asked for while the walk was still in the last one, if the walk enters it where it was expected
                bool hit = false;
                if (pf_top >= 1) {
                    const int l2 = pf_top - i;
                    const int x2 = j - (pf_j - ((l2 * pf_slope) >> 8) - (TBW_COLS - 3));
                    hit = l2 >= 0 && l2 <= WR / 2 && x2 >= 3 && x2 < TBW_COLS - 1;
                }
#ifdef SXG_ROW_PROF
                if (hit) ++tb_hits;
#endif
                if (hit) { wtop = pf_top; wj = pf_j; wgeo = pf_slope; win_commit(pf); }
                else {
                    wtop = i; wj = j; wgeo = wslope;
                    WinRaw cur;
                    win_issue(wtop, wj, wgeo, cur);
                    win_commit(cur);
                }
                // ... and ask for the next one right away: its loads travel while the walk crosses this window
                // Where will the walk enter it?  Every row's descriptor carries the DP column its node is expected to align at (the
                // backbone hint that centres the plane's band): the walk runs at a nearly constant offset from those -- it changes
                // with this sequence's own indels only --, and the next window's top row is a row of this window.  (The adaptive
                // band keeps another quantity in that word: there the running slope predicts.)
                pf_top = wtop - (WR - 6); pf_slope = wslope; pf_j = max(wj - (((WR - 6) * wslope) >> 8), 0);
                if (!ada && pf_top >= 1 && wtop - i >= 0 && wtop - i < WR)
                    pf_j = min(max((int)TBU(whint[WR - 6]) + (j - (int)TBU(whint[wtop - i])), 0), L);
#ifdef SXG_TB_NO_PREFETCH
                pf_top = -1;   // (A/B builds: every window is fetched when the walk needs it, as in rounds 2-4)
#endif
                // (Measured, round 5: the walk enters the predicted window in only 16-22 % of the cases -- rows of other branches make
                //  its path through rank space too irregular for a straight line eight columns wide -- which pays on one- and
                //  two-wave workgroups, where nothing else hides the round trips (16 x 1 kbp: 43.2 -> 42.1 ms), and costs 1.6 % on the
                //  four-wave headline class, whose other waves do: those keep fetching on demand.)
#ifndef SXG_TB_PREFETCH_ALL
                if (T > 128) pf_top = -1;
#endif
                if (pf_top >= 1) win_issue(pf_top, pf_j, pf_slope, pf); else pf_top = -1;
#ifdef SXG_ROW_PROF
                tb_ld += __builtin_readcyclecounter() - tl0;
#endif
            }
        }
        if (st == SRC_STOP) {   // a run of precomputed diagonal steps
            int cl = wtop - i, cx = j - wcol0(cl), ns = 0;
            for (;;) {
                const uint32_t tr = TBU(trans[cl * TBW_COLS + cx]);
                if (!(tr >> 31)) break;
                if (lane == 0) chain[ns] = (uint32_t)cl | ((uint32_t)cx << 6);
                ++ns;
                cl = (int)(tr & 63u); cx = (int)((tr >> 6) & 7u);
            }
            if (ns) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (lane < ns) {   // the run's outputs, one lane per step
                    const uint32_t ce = chain[lane];
                    const int l2 = (int)(ce & 63u), col = wcol0(l2) + (int)(ce >> 6);
                    if (PAIRS) { g_pair_row[n + lane] = wtop - l2; g_pair_pos[n + lane] = col - 1; }
                    if (posnode) g_posnode[col - 1] = (int)(win[l2 * TBW_STRIDE + EO_NODE] & 0x00ffffffu);
                }
                n += ns;
                i = wtop - cl; j = wcol0(cl) + cx;
                hv = sext(TBU(win[cl * TBW_STRIDE + cx]));
#ifdef SXG_ROW_PROF
                tb_steps += (unsigned long long)(ns - 1);
#endif
                continue;
            }
        }
        // Everything the walk reads is the same for all lanes; saying so (readfirstlane) keeps its state
        // in scalar registers and its control flow on the scalar unit instead of 64-wide selects and
        // exec-mask juggling.
        const uint32_t* en = win + (wtop - i) * TBW_STRIDE;
        const int pb = (int)TBU(en[EO_PB]), info = (int)TBU(en[EO_INFO]), q0 = (int)TBU(en[EO_Q0]), q1 = (int)TBU(en[EO_Q1]);
        const int node = (int)(TBU(en[EO_NODE]) & 0x00ffffffu);
        const int np = info & 0xffff, npe = np > 0 ? np : 1;
        auto pred_at = [&](int x) -> int {
            if (np == 0) return 0;
            return x == 0 ? q0 : (x == 1 ? q1 : (int)TBU(g_preds[pb + x]));
        };
        if (st == SRC_STOP) {
            bool done = false;
            if (j >= 1) {   // D: the first predecessor (list order) with the greatest H[p][j-1]
                int dmax = -0x40000000, dp = 0;
                for (int x = 0; x < npe; ++x) {
                    const int p = pred_at(x);
                    const int hp = p == 0 ? h_row0(j - 1) : sext(cell(p, j - 1));
                    if (hp > dmax) { dmax = hp; dp = p; }
                }
                const int lo = wj - j;
                const int letter = (unsigned)lo < (unsigned)TBW_LET ? (int)TBU(wlet[lo]) : (int)TBU(g_seq[j - 1]);
                if (!miss && dmax + (letter == ((info >> 16) & 0xff) ? sm : sn) == hv) {
                    if (lane == 0) {
                        if (PAIRS) { g_pair_row[n] = i; g_pair_pos[n] = j - 1; }
                        if (posnode) g_posnode[j - 1] = node;
                    }
                    ++n;
                    i = dp; --j; hv = dmax;
                    done = true;
                }
            }
            if (!done && !miss) {   // F, then O: a predecessor's outgoing candidate equals H
                int fmax = -0x40000000, omax = -0x40000000;
                for (int x = 0; x < npe; ++x) {
                    const int p = pred_at(x);
                    int of, oo;
                    if (p == 0) { const int h0 = h_row0(j); of = h0 + g; oo = h0 + q; }
                    else { const uint32_t w = cell(p, j); const int h = sext(w); of = h - (int)((w >> 16) & 0xffu); oo = h - (int)(w >> 24); }
                    fmax = max(fmax, of); omax = max(omax, oo);
                }
                if (!miss) {
                    if (fmax == hv) { st = SRC_F; gv = hv; done = true; }
                    else if (CVX && omax == hv) { st = SRC_O; gv = hv; done = true; }
                }
            }
            if (!done && !miss) {
                // a gap in the graph.  E: smallest k with H[i][j-k] + g + (k-1) e == hv (k <= kmax_e), else Q
                // likewise with q, c; 64 columns per round trip, straight from the plane.
                const int hint = (int)TBU(g_meta[8 * (size_t)(i - 1) + HW]);
                int kk = 0, hnew = 0;
                for (int piece = 0; piece < (CVX ? 2 : 1) && !kk && !miss; ++piece) {
                    const int go = piece ? q : g, ge = piece ? c : e;
                    const int kcap = piece ? j : min(j, kmax_e);
                    for (int base = 0; base < kcap && !kk && !miss; base += 64) {
                        const int x = base + lane + 1;
                        const bool act = x <= kcap;
                        const int col = j - x;
                        const int s = col / W, k = col - s * W;
                        const bool inb = act && kept(hint, s);
                        int hval = 0;
                        if constexpr (CB == 2) {
                            if (act && inb) {
                                unsigned raw[SD];
                                plane_load_slot<SD>(g_plane + (size_t)i * (size_t)(SD * BS), BS, s % BS, raw);
                                int h, of, oo;
                                p16_strip_decode<CVX, DELTA, W>([&](const int hw) -> unsigned { return p16_strip_half(raw, hw); }, k, h, of, oo, DT);
                                hval = h;
                            }
                        } else
                        if (act && inb) hval = sext(g_plane[plane_cell<W>((size_t)i, BS, s % BS, k)]);
                        const unsigned long long meq = __ballot(act && inb && hval + go + (x - 1) * ge == hv);
                        const unsigned long long moob = BANDED ? 0ull : __ballot(act && !inb);
                        const int feq = meq ? (int)__builtin_ctzll(meq) : 64, foob = moob ? (int)__builtin_ctzll(moob) : 64;
                        if (foob < feq) { miss = true; miss_row = i; miss_delta = (j - (base + foob + 1)) - hint; }
                        else if (meq) { kk = base + feq + 1; hnew = __builtin_amdgcn_readlane(hval, feq); }
                    }
                }
                if (!miss) {
                    if (!kk) { miss = true; miss_row = i; miss_delta = 0; }   // (cannot happen: some candidate equals H)
                    else {
                        if (PAIRS)
                            for (int x = lane; x < kk; x += 64) { g_pair_row[n + x] = 0; g_pair_pos[n + x] = j - 1 - x; }
                        n += kk; j -= kk; hv = hnew;
                    }
                }
            }
        } else {
            // walking up a gap in the sequence: the first predecessor whose outgoing candidate carries gv;
            // it OPENED the gap iff its H + g (q) is that value, else the walk continues in it with gv - e (c)
            const bool isf = st == SRC_F;
            const int go = isf ? g : q, ge = isf ? e : c;
            int pp = -1, hp = 0;
            for (int x = 0; x < npe && pp < 0; ++x) {
                const int p = pred_at(x);
                int h, oc;
                if (p == 0) { h = h_row0(j); oc = h + go; }
                else { const uint32_t w = cell(p, j); h = sext(w); oc = h - (int)(isf ? ((w >> 16) & 0xffu) : (w >> 24)); }
                if (oc == gv) { pp = p; hp = h; }
            }
            if (!miss) {
                if (pp < 0) { miss = true; miss_row = i; miss_delta = 0; }   // (cannot happen)
                else {
                    if (PAIRS && lane == 0) { g_pair_row[n] = i; g_pair_pos[n] = -1; }
                    ++n;
                    i = pp;
                    if (hp + go == gv) { st = SRC_STOP; hv = hp; } else gv -= ge;
                }
            }
        }
    }
#undef TBU
    if (lane == 0) { ctl[TBM_FLAG] = miss ? 1 : 0; ctl[TBM_ROW] = miss_row; ctl[TBM_DELTA] = miss_delta; ctl[TBM_RANGE] = range ? 1 : 0; }
#ifdef SXG_ROW_PROF
    if (lane == 0 && B.row_prof) {
        B.row_prof[ROWP_TB_STEPS] += tb_steps; B.row_prof[ROWP_TB_LOADS] += tb_loads;
        B.row_prof[ROWP_TB_CYCLES] += __builtin_readcyclecounter() - tb_t0; B.row_prof[ROWP_TB_FILL_CYCLES] += tb_ld; B.row_prof[ROWP_TB_HITS] += tb_hits;
    }
#endif
    __builtin_amdgcn_s_setprio(0);
    return n;
}

}  // namespace sxg

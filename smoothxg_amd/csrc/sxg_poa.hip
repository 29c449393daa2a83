// sxg_poa.hip -- kernels + host side of the C ABI declared in include/sxg_poa.h.
//
// One persistent workgroup ("slot") owns one smoothxg block at a time and runs the whole
// sequential chain of src/smooth.cpp:760-769 on the device:
//     for every sequence: rows <- graph; DP fill; traceback; fuse; re-rank
// Slots pull blocks from a cost-sorted queue (largest first), so thousands of blocks are
// processed per launch with no host round trip between the alignments of a block.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <sys/mman.h>
#include <thread>
#include <vector>

#include "../../include/sxg_poa.h"
#include <rccl/rccl.h>   // (types and prototypes only: the library is opened on first use, see rccl_api)
#include <dlfcn.h>
#include "poa_kernels.hip.h"       // slot layout, launch arguments, the persistent kernels (device side)
#include "poa_cost.h"              // a block's cost in its launch (rows x swept columns), the deal over CUs
#include "poa_deal.h"              // the deal of a batch over the members of a device group (contiguous cuts of the cost)
#include "poa_results.h"           // the table of the result arrays, the reassembly of a batch's result from its parts, the full MSA
#include "poa_kern_tables.hip.h"   // kernel classes by geometry; instantiated in the kern_*.hip translation units
#include "poa_split.hip.h"         // the identity split: argument structs and launchers (kernels in kern_split.hip)
#include "poa_mash.hip.h"          // its mash-based branch: k-mer sets, intersections, the walk of M4 (kernels in kern_split.hip)
#include "poa_identity.hip.h"      // the identity estimate of -a on those sets: all pairs of a block, the percentile's pair (kern_split.hip)
#include "poa_repeat.hip.h"        // the tandem-repeat scan of the cutting half of break_blocks: counts per lag, then the double pass (kern_repeat.hip)
#include "poa_letters.hip.h"       // the resident path letters: the gather that cuts ranges out of them for the two calls above (kern_letters.hip)
#include "poa_sgd.hip.h"           // the path-guided SGD node order of prep: argument struct and launchers (kernels in kern_sgd.hip)
#include "poa_msa.hip.h"           // the trimmed MSA (want_msa == SXG_MSA_TRIMMED): argument structs and launchers (kernels in kern_msa.hip)
#include "poa_maf_text.hip.h"      // the MAF text of the resident trimmed rows, their letter counts: argument structs and launchers (kernels in kern_maf.hip)


// ---------------------------------------------------------------------------------------
// Block graphs (sxg_poa_batch_in::want_block_graph): after the POA kernels, one workgroup per block turns the block's POA
// result -- letters, edges, one node id per base, consensus -- into its normalised block graph (poa_bgraph_dev.h: trim,
// path-supported edges, unchop, topological re-numbering, compact step lists) in a slot-private scratch arena.
struct BgArgs {
    const int32_t* blk_off; const int64_t* seq_off; const uint8_t* bases; const int32_t* paths;
    const uint8_t* node_code; const int32_t* edge_tail; const int32_t* edge_head; const int32_t* cons;
    const int32_t *nn, *ne, *nc; const int32_t* trim; int cons_mode;
    const int32_t* work; int n_work; int32_t* queue;
    uint8_t* arena; size_t slot_bytes; int capV, capE, capC, capT;
    const int64_t *node_o, *edge_o;   // where block b's nodes / edges go in the output arrays
    int32_t *o_len, *o_outdeg; uint8_t* o_indeg; char* o_seq; int32_t* o_eto; int32_t* o_steps; int32_t* o_nsteps;
    int32_t* o_cons; int32_t* o_counts;
};
constexpr int BG_THREADS = 256, BG_HEAP = 3072;
static size_t bg_slot_bytes(int capV, int capE, int capC, int capT) {
    return 4 * (27 * ((size_t)capV + 2) + 3 * ((size_t)capE + capC + 2) + ((size_t)capC + 2) + ((size_t)capT + 2) + 4) + 256;
}
struct BgCtx : WgCtx {
    int* hp;
    __device__ __forceinline__ int load_fresh(const int32_t* p) const { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int* heap() const { return hp; }
    __device__ __forceinline__ int heap_cap() const { return BG_HEAP; }
};
__global__ __launch_bounds__(BG_THREADS) void block_graph_kernel(const BgArgs A) {
    __shared__ int s_scan[64];
    __shared__ int s_heap[BG_HEAP];
    __shared__ int s_work;
    BgCtx ctx;
    ctx.lds = (sxg_lds_int*)s_scan;
    ctx.hp = s_heap;
    const int t = threadIdx.x;
    int32_t* w = (int32_t*)(A.arena + (size_t)blockIdx.x * A.slot_bytes);
    const size_t C = (size_t)A.capV + 2, EC = (size_t)A.capE + A.capC + 2;
    BgScratch W;
    auto take = [&](size_t n) { int32_t* q = w; w += n; return q; };
    W.vis = take(C); W.front = take(C); W.back = take(C); W.ecnt = take(C); W.eoff = take(C);
    W.ehead = take(EC); W.eused = take(EC);
    W.outdeg = take(C); W.indeg = take(C); W.only = take(C); W.nxt = take(C); W.prv = take(C);
    W.pj0 = take(C); W.pj1 = take(C); W.pd0 = take(C); W.pd1 = take(C); W.cid = take(C);
    W.head_of = take(C); W.tail_of = take(C); W.clen = take(C); W.indc = take(C); W.coff = take(C); W.newid = take(C);
    W.csucc = take(EC); W.cc = take((size_t)A.capC + 2); W.tmp = take((size_t)A.capT + 2);
    W.lenN = take(C); W.odN = take(C); W.soffN = take(C); W.eoffN = take(C); W.flag = take(4);
    for (;;) {
        __syncthreads();
        if (t == 0) s_work = atomicAdd(A.queue, 1);
        __syncthreads();
        const int wi = s_work;
        if (wi >= A.n_work) break;
        const int b = A.work[wi];
        const int s0 = A.blk_off[b], s1 = A.blk_off[b + 1];
        const int64_t base0 = A.seq_off[s0];
        BgIn I;
        I.node_code = A.node_code + base0; I.V = A.nn[b]; I.E = A.ne[b];
        I.e_tail = A.edge_tail + base0; I.e_head = A.edge_head + base0;
        I.paths = A.paths + base0; I.bases = A.bases + base0; I.seq_off = A.seq_off; I.s0 = s0; I.s1 = s1;
        I.trim = A.trim ? A.trim[b] : 0;
        I.cons = A.cons ? A.cons + base0 : nullptr; I.n_cons = A.cons ? A.nc[b] : 0; I.cons_mode = A.cons ? A.cons_mode : 0;
        BgOut O;
        const int64_t no = A.node_o[b], eo = A.edge_o[b];
        O.node_len = A.o_len + no; O.node_outdeg = A.o_outdeg + no; O.node_indeg = A.o_indeg + no; O.seq = A.o_seq + no;
        O.eto = A.o_eto + eo; O.steps = A.o_steps + base0; O.nsteps = A.o_nsteps + s0; O.cons_steps = A.o_cons + no;
        O.counts = A.o_counts + (size_t)BGC_N * b;
        block_graph(ctx, I, W, O);
    }
}

// dense <- worst-case gather (one workgroup per block, grid-stride over blocks)
// upload: letters above 4 read as N (4).  16 bytes per thread and step; the buffer is allocated with 16 bytes of slack.
__global__ void clamp_bases_kernel(uint8_t* bases, const int64_t n) {
    const int64_t n16 = (n + 15) / 16;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x) {
        u32x4 v = ((const u32x4*)bases)[i];
        unsigned w[4] = {v.x, v.y, v.z, v.w};
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned o = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) { const unsigned c = (w[k] >> (8 * b)) & 0xffu; o |= (c > 4u ? 4u : c) << (8 * b); }
            any |= o != w[k];
            w[k] = o;
        }
        if (any) ((u32x4*)bases)[i] = u32x4{w[0], w[1], w[2], w[3]};
    }
}

template <class Tv>
__global__ void gather_kernel(const Tv* __restrict__ src, Tv* __restrict__ dst, const int64_t* __restrict__ src_off,
                              const int64_t* __restrict__ dst_off, int n) {
    for (int b = blockIdx.x; b < n; b += gridDim.x) {
        const int64_t s = src_off[b], d = dst_off[b], cnt = dst_off[b + 1] - d;
        for (int64_t i = threadIdx.x; i < cnt; i += blockDim.x) dst[d + i] = src[s + i];
    }
}

// =======================================================================================
// host side
// =======================================================================================

// Error text: per calling thread (as the header promises) plus the most recent one of ANY thread -- a caller that ran the
// engine on a worker thread (sxg_smooth's chunk pipeline) and asks from its own thread gets that one instead of nothing.
static thread_local std::string g_err;
#include <mutex>
static std::mutex g_err_mu;
static std::string g_err_any;
static thread_local std::string g_err_ret;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    { std::lock_guard<std::mutex> lk(g_err_mu); g_err_any = msg; }
    return code;
}
#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t _e = (x);                                                                   \
        if (_e != hipSuccess)                                                                  \
            return fail(_e == hipErrorOutOfMemory ? SXG_E_NOMEM : SXG_E_NODEVICE,              \
                        std::string(#x) + ": " + hipGetErrorString(_e));                       \
    } while (0)

// Plane cell format of the packed sweep for a score set: 2-byte codes when the three fields fit 16 bits (poa_rowcode.h:
// the stored rows' code, field widths of P16Delta), the 4-byte cells of rounds 2-4 otherwise.  SXG_POA_CELL_BYTES=4 forces the latter (A/B runs, tests).
static int plane_cell_bytes(const Scoring& S) {
    if (const char* e = getenv("SXG_POA_CELL_BYTES")) if (atoi(e) == 4) return 4;
    return p16_delta_fits(S) ? 2 : 4;
}
// ... and of the banded sweep (round 6): 2-byte codes for LOCAL alignments whose delta code fits -- every cell of a band is a real
// score there; a global alignment's bands hold "minus infinity" cells, whose steps no code holds.  SXG_POA_BAND_CELL_BYTES=4: the
// 4-byte cells of rounds 2-5 (A/B runs, tests).
static int band_cell_bytes(const Scoring& S) {
    if (const char* e = getenv("SXG_POA_BAND_CELL_BYTES")) if (atoi(e) == 4) return 4;
    return S.sw ? plane_cell_bytes(S) : 4;
}

// Score ranges.  Local alignment: 0..m*L.  Global: additionally down to the all-gap path through
// `rows` graph rows (sxg_gap_cost).  `rows` is exact for the align-only API; for whole blocks the
// graph grows while the block runs, so the host assumes the smallest possible graph (one node per base
// of the longest sequence) and the kernel re-checks with the true row count before every sweep,
// answering ST_RANGE_OVERFLOW when it no longer fits: the block is then re-run one step wider.
static long score_floor(const Scoring& S, int maxlen, int rows) {
    if (S.sw) return 0;
    return -(sxg_gap_cost(S.g, S.e, S.q, S.c, rows) + sxg_gap_cost(S.g, S.e, S.q, S.c, maxlen));
}
// int16 H in the row words of the 32-bit sweep
static bool h16_safe(const Scoring& S, int maxlen, int rows) {
    return (long)std::abs(S.m) * maxlen < 30000 && score_floor(S, maxlen, rows) < 30000;
}
// Packed-int16 sweep: every reachable score and every intermediate (score +- one penalty, difference
// of two scores) must stay inside int16 with NEGP = -16384 as "-inf".
// clamp_ok: the caller can re-run a block whose walk met a clamped cell (whole blocks on the full matrix: P16_NWFLOOR in
// poa_dp16.hip.h) -- a global alignment then only needs its POSITIVE range to fit; the align-only API and the banded sweep
// keep the strict rule (no re-run / -inf cells of their own).  SXG_POA_NO_NW_CLAMP=1: strict everywhere (A/B runs).
static bool p16_safe(const Scoring& S, int maxlen, int rows, bool clamp_ok = false) {
    if (getenv("SXG_POA_NO_PACKED")) return false;
    // stored rows keep H - max(H+g, F+e) and H - max(H+q, O+c) in one byte each
    if (std::abs(S.g) > 120 || std::abs(S.q) > 120) return false;
    // local alignment: every existing cell has 0 <= H <= m * L and F, O, E, Q >= -|q|; the range is one-sided
    if (S.sw) return (long)std::abs(S.m) * maxlen < P16_LOCAL_LIMIT;
    if ((long)std::abs(S.m) * maxlen >= 15800) return false;
    // (the walk may dip to -16 000 + m L + m before it is called clamped: 1 500 below zero at the limit -- a global alignment of
    //  related sequences stays far above; one that does not is re-run on the 32-bit sweep while that sweep reaches it, 12 287 letters)
    if (clamp_ok && !getenv("SXG_POA_NO_NW_CLAMP")) return (long)std::abs(S.m) * maxlen + std::abs(S.m) < 14500;
    return score_floor(S, maxlen, rows) < 15800;
}
// narrowest mode >= `at_least` (2 = packed < 0 = int16 row words < 1 = int32 row words)
static int row_mode(const Scoring& S, int maxlen, int rows, int at_least = 2, bool clamp_ok = false) {
    if (at_least == 2 && p16_safe(S, maxlen, rows, clamp_ok)) return 2;
    if (at_least != 1 && h16_safe(S, maxlen, rows)) return 0;
    return 1;
}

// development knob: SXG_POA_FORCE_P16="W,NW" forces one packed geometry (A/B runs of a single-class build)
static void forced_p16(int* w, int* nw) {
    *w = *nw = 0;
    if (const char* e = getenv("SXG_POA_FORCE_P16"))
        if (sscanf(e, "%d,%d", w, nw) != 2) *w = *nw = 0;
}

// SXG_POA_DEBUG: wall-clock laps of the host side (stderr)
struct HostLaps {
    bool on = getenv("SXG_POA_DEBUG") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[sxg] host %-22s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

#include "poa_devres.h"            // DevBuf, DevEvent, DevStream, OutGuard: every device resource here frees itself (uses fail above)

struct BlockMeta {
    int maxlen = 0, nseq = 0, rm = 0; bool fits = false; Variant variant{16, 1, 256, 0};
    int tier = 0;      // arena capacity tier the block runs at next (raised by ROWS/POOL/TBX overflow only)
    int tiles = 1;     // 32-bit sweep in column tiles (poa_tiles.h): tiles of the block's longest sequence at `variant`; 1 = no tiles
    bool wide_band = false;   // packed sweep re-run with a traceback plane that keeps EVERY strip (after ST_BAND_MISS)
    bool no_wide = false;     // that plane did not fit the arena budget: the block takes the widening ladder instead
    int64_t sumlen = 0;
    double cost = 0;
    bool cvx = false, sw = true;
    Scoring S;
};

// Row mode (the narrowest >= at_least that holds the block's scores), plane cell format and launch geometry of a block
// (optimistic: the kernel re-checks -- see score_floor -- and a packed global sweep checks the cells its traceback visits)
// long_blocks (sxg_poa_set_long_blocks): a block on a 32-bit sweep that no geometry covers runs the widest one, 16 waves of 12
// columns, in as many column tiles as its longest sequence needs, up to SXG_POA_MAX_SEQ_LEN_TILED.  SXG_POA_TILE_COLS=n (a
// multiple of 512; honoured with the switch on only -- a test knob, tiles change speed, never results): every 32-bit block takes
// the geometry of a sequence of n - 1 letters and the tiles its own length needs at it.
static_assert(SXG_POA_MAX_SEQ_LEN_TILED == TILED_MAX_SEQ_LEN && TILED_MAX_SEQ_LEN + 1 == TILED_MAX_TILES * (SXG_POA_MAX_SEQ_LEN_WIDE + 1), "tiled limit of the header");
static void classify_block(BlockMeta& m, int at_least, bool clamp_ok, bool long_blocks) {
    m.rm = row_mode(m.S, m.maxlen, m.maxlen, at_least, clamp_ok);
    int cb = m.rm == 2 ? plane_cell_bytes(m.S) : 4;
    int fw, fnw;
    forced_p16(&fw, &fnw);
    m.fits = variant_for_len(m.maxlen, m.rm, &m.variant, m.S.sw, cb, fw, fnw);
    m.tiles = 1;
    // (a block whose scores the packed sweep holds but whose length no packed geometry covers -- local beyond 26 623 letters with
    //  m L < 30 000 -- takes the 32-bit sweep, tiled, as well: below the tiled limit the switch leaves no length refused)
    if (long_blocks && m.rm == 2 && !m.fits && m.maxlen <= SXG_POA_MAX_SEQ_LEN_TILED) {
        m.rm = row_mode(m.S, m.maxlen, m.maxlen, 0, false);
        cb = 4;
        m.fits = variant_for_len(m.maxlen, m.rm, &m.variant, m.S.sw, cb, 0, 0);
    }
    if (long_blocks && m.rm < 2 && m.maxlen <= SXG_POA_MAX_SEQ_LEN_TILED) {
        int cols = 0;
        if (const char* e = getenv("SXG_POA_TILE_COLS")) cols = atoi(e);
        Variant v = m.variant;
        if (cols >= 512 && cols % 512 == 0 && variant_for_len(cols - 1, m.rm, &v)) { m.variant = v; m.fits = true; }
        else if (!m.fits) { m.variant = Variant{12, 16, class_tmax(12, 16, m.rm, 4, true), m.rm, 4}; m.fits = true; }
        m.tiles = n_tiles(m.maxlen, m.variant.T(), m.variant.W);
    }
    m.variant.CB = cb;   // (also of a block that does not fit)
    m.variant.DS = m.rm == 2 && cb == 2 && p16_default_scores(m.S) && !getenv("SXG_POA_NO_DEFAULT_CLASS");
}

struct PlanRes {   // (members die in reverse order: the buffers before the stream that used them)
    DevStream stream;
    DevEvent e0, e1;
    DevBuf arena, work, queue, est;
};

// Pinned host memory for the one big array of a download (the block graphs' step lists: 1.3 GB on the headline batch).  A
// copy into pageable memory runs at about half the link's rate (the runtime stages it); pinning 1.3 GB takes longer than the
// copy saves, so the buffers are pinned ONCE and lent out: a result holds one until sxg_poa_batch_free (any thread), the pool
// lives as long as the handle or the last result that borrowed from it.  SXG_POA_NO_PINNED=1 switches it off.
struct PinPool {
    struct Buf { void* p; size_t cap; bool busy; };
    std::mutex mu;
    std::vector<Buf> bufs;
    void* acquire(size_t bytes) {   // nullptr: nothing to lend (the caller allocates pageable memory)
        std::lock_guard<std::mutex> g(mu);
        for (auto& b : bufs) if (!b.busy && b.cap >= bytes) { b.busy = true; return b.p; }
        for (size_t i = 0; i < bufs.size(); ++i)
            if (!bufs[i].busy) { (void)hipHostFree(bufs[i].p); bufs.erase(bufs.begin() + (long)i); break; }   // (an idle one that is too small)
        if (bufs.size() >= 4) return nullptr;
        void* q = nullptr;
        const size_t cap = bytes + bytes / 8;
        if (hipHostMalloc(&q, cap, hipHostMallocDefault) != hipSuccess || !q) { (void)hipGetLastError(); return nullptr; }
        bufs.push_back(Buf{q, cap, true});
        return q;
    }
    void release(void* p) {
        std::lock_guard<std::mutex> g(mu);
        for (auto& b : bufs) if (b.p == p) b.busy = false;
    }
    void prewarm(size_t bytes) { if (void* p = acquire(bytes)) release(p); }   // (pin now, lend later)
    ~PinPool() { for (auto& b : bufs) (void)hipHostFree(b.p); }
};
static inline bool msa_trimmed(int want_msa) { return want_msa == SXG_MSA_TRIMMED || want_msa == SXG_MSA_TRIMMED_RESIDENT; }
struct sxg_poa_handle {
    // Every device resource of the handle is a member that frees itself (poa_devres.h): `delete h`, with h->device current, is the
    // whole teardown.  The stream and the events stand first: members die in reverse order, the buffers before their stream.
    int device = 0;
    DevStream stream;
    DevEvent ev0, ev1;
    std::vector<std::unique_ptr<PlanRes>> planres;   // per launch of a round: stream, events, arena (kept between executes)
    int num_cu = 256;
    uint64_t mem_budget = 0;
    bool long_blocks = false;   // sxg_poa_set_long_blocks: 32-bit sweeps beyond their widest geometry run in column tiles
    int64_t tile_blocks = 0, tile_sweeps = 0, tile_tiles = 0;   // tiled launches of the last execute (sxg_poa_get_tile_stats)
    int budget_share = 1;   // members of a device group on this handle's device: the default arena cap is divided among them
    // resident batch
    bool have_batch = false, executed = false;
    int n_blocks = 0;
    int64_t n_seqs = 0, n_bases = 0;
    int want_consensus = 0, want_msa = 0, per_block_params = 0;
    std::vector<int32_t> h_blk_off;
    std::vector<int64_t> h_seq_off;
    std::vector<sxg_poa_params> h_params;
    std::vector<BlockMeta> meta;
    DevBuf d_blk_off, d_seq_off, d_bases, d_weights, d_params;
    bool has_weights = false;
    DevBuf d_status, d_nn, d_ne, d_nc, d_node_code, d_node_rank, d_node_group, d_edge_tail, d_edge_head, d_edge_w,
        d_paths, d_score, d_cells, d_cons, d_work, d_queue, d_arena, d_blk_cycles;
    DevBuf d_tmp_a, d_tmp_b, d_tmp_c, d_tmp_d;
    DevBuf d_board;   // the per-CU progress board (sxg_balance_prio) the launches of a round share
    // a round's cost model, rows x swept columns (poa_cost.h): per block in the launch it runs in, and per sequence the part of its
    // block's cost that lies before it (BlockArgs::est_done -- one array for all launches of the round: a block is in one of them)
    std::vector<uint64_t> blk_cost, seq_done;
    DevBuf d_est_done;
    // block graphs (want_block_graph): inputs, outputs in per-block layouts, the per-block counts of the last execute
    int want_block_graph = 0, bg_cons_visited_only = 0;
    std::shared_ptr<PinPool> pins;   // pinned host buffers lent to results (created with the handle)
    std::thread pin_thread;          // pins the buffer of the coming download while the kernels run (joined before it is needed)
    bool bg_done = false;
    DevBuf d_trim, d_bg_no, d_bg_eo, d_bg_len, d_bg_od, d_bg_id, d_bg_seq, d_bg_eto, d_bg_steps, d_bg_nsteps, d_bg_cons, d_bg_counts,
        d_bg_work, d_bg_queue, d_bg_arena;
    std::vector<int64_t> bg_node_o, bg_edge_o;
    std::vector<int32_t> bg_counts;
    // trimmed MSA (want_msa == SXG_MSA_TRIMMED): columns of the nodes, kept columns and offsets of the blocks, the rows
    bool msa_done = false;
    DevBuf d_msa_no, d_msa_tmp, d_msa_col, d_msa_be, d_msa_off, d_msa_items, d_msa_work, d_msa_queue, d_msa;
    std::vector<int64_t> msa_off_h;
    std::vector<int32_t> d_trim_h;   // host copy of d_trim
    std::vector<int32_t> msa_cols_h;
    double msa_cols_ms = 0, msa_rows_ms = 0;
    // the MAF text (sxg_poa_maf_text) and the letter counts of the resident rows: where every row starts in d_msa (built on first
    // use after an execute), the per-call arrays and the text on the device, events and sums of the text kernel
    std::vector<int64_t> msa_row_begin_h;
    std::vector<char> msa_live_h;   // [n_blocks] the blocks run_msa_rows built rows for (status OK, with sequences)
    bool msa_rows_staged = false;
    DevBuf d_maf_rowb, d_maf_letters, d_maf_off, d_maf_srck, d_maf_lit, d_maf_text;
    DevEvent maf_e0, maf_e1;
    double maf_text_ms = 0;
    uint64_t maf_text_bytes = 0;
    // resident path letters (sxg_poa_letters_*): outside the memory budget, kept across batches; path_off is the host's copy for
    // the validation of ranges, d_src / d_off the per-call arrays of the gather (kept here so that they outlive its launch)
    struct Letters {
        uint64_t id = 0;
        int64_t n_paths = 0, n_letters = 0;
        std::vector<int64_t> path_off;
        DevBuf d, d_src, d_off;
        DevEvent g0, g1;
        bool pending = false;   // a gather stands between g0 and g1 and is not yet in the sums
        uint64_t pending_bytes = 0;
        uint64_t uploads = 0, bytes_uploaded = 0, gathered_bytes = 0;
        double gather_ms = 0;
    } letters;
    sxg_poa_stats stats{};
    sxg_poa_width_stats wstats{};   // packed sweeps of the last execute per strip width (sxg_poa_get_width_stats)
    sxg_poa_twin_stats tstats{};    // twin steps and join rows of the last execute (sxg_poa_get_twin_stats)
    // multi-GPU (sxg_poa_batch_run_sharded): communicator of this rank, result blob of the local shard, and -- on the
    // root -- the blobs of the other ranks, delivered by RCCL
    ncclComm_t comm = nullptr;
    bool own_comm = false;
    int nranks = 1, rank = 0;
    DevBuf d_blob, d_recv, d_counts;
    // staged sharded run: the deal of the last sxg_poa_batch_upload_sharded, the counts every rank announced in the last
    // sxg_poa_batch_execute_sharded and where the root put their blobs
    std::vector<std::vector<int32_t>> sh_parts;
    std::vector<int64_t> sh_counts;
    std::vector<size_t> sh_at;
    bool sh_dealt = false, sh_exchanged = false;
    uint64_t sh_bytes_received = 0;
    int sh_ranks_seen = 0;
    double sh_pack_ms = 0, sh_exchange_ms = 0;   // last sxg_poa_batch_execute_sharded: packing the blob; size all-gathers + blob exchange (waits for the slowest rank)
};

// ---------------------------------------------------------------------------------------
// ROCTx ranges around the phases of the C ABI (the reference brackets its phases with timers on stderr;
// here `rocprofv3 --marker-trace` shows upload / execute / pack / exchange / download next to the kernels).  The marker
// library is looked up at first use -- rocprofiler-sdk's, then roctracer's -- and the ranges are no-ops without it: the
// engine does not link against a profiler.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        if (getenv("SXG_POA_NO_ROCTX")) return;
        void* lib = dlopen("librocprofiler-sdk-roctx.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return;
        push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
        pop = (int (*)())dlsym(lib, "roctxRangePop");
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
static Roctx& roctx() { static Roctx r; return r; }
struct RoctxRange {
    bool on;
    explicit RoctxRange(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~RoctxRange() { if (on) roctx().pop(); }
    RoctxRange(const RoctxRange&) = delete;
    RoctxRange& operator=(const RoctxRange&) = delete;
};
}  // namespace
extern "C" int sxg_poa_roctx_available(void) { return roctx().push != nullptr ? 1 : 0; }

// A streaming copy on this device, timed with HIP events on the engine's stream: what SURVEY 8(d) asks to be printed beside the
// 8 TB/s of the data sheet (bench.py: roofline.hbm.copy_GBps_measured).  16 bytes per lane and step, grid-stride, non-temporal
// both ways; bytes read + bytes written over the mean of `reps` launches after one warm-up.
__global__ __launch_bounds__(256) void sxg_copy_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, const size_t n16) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride)
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + i), dst + i);
}
extern "C" int sxg_poa_measure_copy(sxg_poa_handle* h, uint64_t bytes, int reps, double* gbps) {
    if (!h || !gbps) return fail(SXG_E_INVALID, "NULL argument");
    *gbps = 0;
    HIPCHK(hipSetDevice(h->device));
    const size_t n16 = (size_t)std::max<uint64_t>(bytes, 1u << 20) / 16;
    DevBuf a, b;
    if (int rc = a.ensure(n16 * 16)) return rc;
    if (int rc = b.ensure(n16 * 16)) return rc;
    HIPCHK(hipMemsetAsync(a.p, 1, n16 * 16, h->stream));
    DevEvent e0, e1;
    HIPCHK(e0.create()); HIPCHK(e1.create());
    const int grid = std::max(h->num_cu, 1) * 16;
    reps = std::max(reps, 1);
    hipLaunchKernelGGL(sxg_copy_kernel, dim3((unsigned)grid), dim3(256), 0, h->stream, a.as<u32x4>(), b.as<u32x4>(), n16);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e0, h->stream));
    for (int r = 0; r < reps; ++r)
        hipLaunchKernelGGL(sxg_copy_kernel, dim3((unsigned)grid), dim3(256), 0, h->stream, a.as<u32x4>(), b.as<u32x4>(), n16);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e1, h->stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    if (ms > 0) *gbps = 2.0 * (double)(n16 * 16) * reps / ((double)ms * 1e-3) / 1e9;
    return SXG_OK;
}

extern "C" int sxg_poa_abi_version(void) { return SXG_POA_ABI_VERSION; }
extern "C" const char* sxg_poa_last_error(void) {
    if (!g_err.empty()) return g_err.c_str();
    { std::lock_guard<std::mutex> lk(g_err_mu); g_err_ret = g_err_any; }
    return g_err_ret.c_str();
}
extern "C" int sxg_poa_compute_units(sxg_poa_handle* h) { return h ? h->num_cu : -1; }
extern "C" int sxg_poa_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int sxg_poa_create(int device, sxg_poa_handle** out) {
    if (!out) return fail(SXG_E_INVALID, "out is NULL");
    *out = nullptr;
    // Batches of mixed lengths run one launch per geometry on separate streams.  The HIP runtime maps
    // streams onto 4 hardware queues by default and launches sharing a queue run one after the other
    // (measured on a 12-geometry batch: 44.5 s vs 17.9 s with 16 queues).  Takes effect only if the
    // runtime is not initialised yet; callers that initialise HIP first should export it themselves.
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SXG_E_NODEVICE, "no HIP device available");
    if (device < 0 || device >= n) return fail(SXG_E_INVALID, "device index out of range");
    HIPCHK(hipSetDevice(device));
    auto h = std::make_unique<sxg_poa_handle>();   // (freed on every early return below)
    h->device = device;
    h->pins = std::make_shared<PinPool>();
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    h->num_cu = prop.multiProcessorCount;
    HIPCHK(h->stream.create(hipStreamNonBlocking));
    HIPCHK(h->ev0.create());
    HIPCHK(h->ev1.create());
    *out = h.release();
    return SXG_OK;
}

extern "C" void sxg_poa_comm_destroy(sxg_poa_handle* h);
extern "C" void sxg_poa_destroy(sxg_poa_handle* h) {
    if (!h) return;
    if (h->pin_thread.joinable()) h->pin_thread.join();
    (void)hipSetDevice(h->device);   // (a group holds handles of several devices: the members below free on this one)
    sxg_poa_comm_destroy(h);
    delete h;
}

extern "C" int sxg_poa_set_memory_budget(sxg_poa_handle* h, uint64_t bytes) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    h->mem_budget = bytes;
    return SXG_OK;
}

extern "C" int sxg_poa_set_long_blocks(sxg_poa_handle* h, int on) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    h->long_blocks = on != 0;   // (read when a batch is uploaded and when a block changes its sweep)
    return SXG_OK;
}

extern "C" int sxg_poa_get_tile_stats(sxg_poa_handle* h, int64_t* blocks, int64_t* sweeps, int64_t* tiles) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (blocks) *blocks = h->tile_blocks;
    if (sweeps) *sweeps = h->tile_sweeps;
    if (tiles) *tiles = h->tile_tiles;
    return SXG_OK;
}

extern "C" int sxg_poa_get_stats(sxg_poa_handle* h, sxg_poa_stats* out) {
    if (!h || !out) return fail(SXG_E_INVALID, "NULL argument");
    *out = h->stats;
    return SXG_OK;
}

extern "C" int sxg_poa_get_width_stats(sxg_poa_handle* h, sxg_poa_width_stats* out) {
    if (!h || !out) return fail(SXG_E_INVALID, "NULL argument");
    *out = h->wstats;
    return SXG_OK;
}

extern "C" int sxg_poa_get_twin_stats(sxg_poa_handle* h, sxg_poa_twin_stats* out) {
    if (!h || !out) return fail(SXG_E_INVALID, "NULL argument");
    *out = h->tstats;
    return SXG_OK;
}

// SXG_POA_TWIN=0: the classes with a twin step run the rows of round 12 (prep sets neither ROW_TWIN nor ROW_JOIN)
static bool twin_enabled() {
    const char* e = getenv("SXG_POA_TWIN");
    return !(e && atoi(e) == 0);
}

static uint64_t arena_budget(sxg_poa_handle* h) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return 8ull << 30;
    uint64_t avail = (uint64_t)fr + h->d_arena.cap;  // the arenas we already hold can be reused
    for (const auto& r : h->planres) avail += r->arena.cap;
    uint64_t b = avail / 4 * 3 / (uint64_t)std::max(h->budget_share, 1);
    if (h->mem_budget && h->mem_budget < b) b = h->mem_budget;
    return b;
}

// ---------------------------------------------------------------------------------------
extern "C" int sxg_poa_batch_upload(sxg_poa_handle* h, const sxg_poa_batch_in* in) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    if (in->n_blocks < 0 || (in->n_blocks > 0 && (!in->blk_off || !in->seq_off || !in->params)))
        return fail(SXG_E_INVALID, "batch_in has NULL arrays");
    HIPCHK(hipSetDevice(h->device));
    const RoctxRange range_("sxg_poa_batch_upload");
    HostLaps laps;
    h->have_batch = false; h->executed = false;
    const int nb = in->n_blocks;
    if (nb > 0 && in->blk_off[0] != 0) return fail(SXG_E_INVALID, "blk_off[0] must be 0");
    const int64_t ns = nb ? in->blk_off[nb] : 0;
    for (int b = 0; b < nb; ++b)
        if (in->blk_off[b + 1] < in->blk_off[b]) return fail(SXG_E_INVALID, "blk_off not monotone");
    if (ns > 0 && in->seq_off[0] != 0) return fail(SXG_E_INVALID, "seq_off[0] must be 0");
    for (int64_t s = 0; s < ns; ++s)
        if (in->seq_off[s + 1] < in->seq_off[s]) return fail(SXG_E_INVALID, "seq_off not monotone");
    const int64_t nbases = ns ? in->seq_off[ns] : 0;
    if (nbases > 0 && !in->bases) return fail(SXG_E_INVALID, "bases is NULL");
    const int np = in->per_block_params ? nb : 1;
    for (int k = 0; k < np && nb > 0; ++k) {
        const sxg_poa_params& p = in->params[k];
        if (p.m < 0 || p.n > 0 || p.g > 0 || p.e > 0 || p.q > 0 || p.c > 0 || (p.mode & ~(1 | SXG_ORDER_SPOA | SXG_IDS_SPOA)) != 0 || p.banded > 2)
            return fail(SXG_E_INVALID, "scores must follow spoa's sign convention (m>=0, others <=0), mode 0|1");
        // (S6' numbers the new nodes for the re-sort S7'; the incrementally kept order places them by their sequence-order index)
        if ((p.mode & SXG_IDS_SPOA) && !(p.mode & SXG_ORDER_SPOA))
            return fail(SXG_E_INVALID, "mode | SXG_IDS_SPOA needs SXG_ORDER_SPOA");
    }
    h->n_blocks = nb; h->n_seqs = ns; h->n_bases = nbases;
    h->want_consensus = in->want_consensus; h->want_msa = in->want_msa;
    h->want_block_graph = in->want_block_graph < 0 || in->want_block_graph > 3 ? 0 : in->want_block_graph;
    // (the full MSA is formatted on the host from the per-base paths; the trimmed one is built on the device)
    if (h->want_block_graph >= 2 && in->want_msa && !msa_trimmed(in->want_msa)) h->want_block_graph = 1;
    h->bg_cons_visited_only = in->bg_consensus_visited_only ? 1 : 0;
    h->bg_done = false; h->msa_done = false; h->msa_rows_staged = false;
    h->per_block_params = in->per_block_params;
    h->h_blk_off.assign(in->blk_off, in->blk_off + nb + 1);
    h->h_seq_off.assign(in->seq_off, in->seq_off + ns + 1);
    h->h_params.assign(in->params, in->params + np);
    h->meta.assign(nb, BlockMeta());
    for (int b = 0; b < nb; ++b) {
        BlockMeta& m = h->meta[b];
        m.S = normalise(h->h_params[in->per_block_params ? b : 0]);
        m.cvx = m.S.convex; m.sw = m.S.sw;
        m.nseq = in->blk_off[b + 1] - in->blk_off[b];
        double prev = 0;
        for (int s = in->blk_off[b]; s < in->blk_off[b + 1]; ++s) {
            const int64_t len = in->seq_off[s + 1] - in->seq_off[s];
            m.maxlen = (int)std::max<int64_t>(m.maxlen, len);
            m.sumlen += len;
            // cost_b = sum_k L_k * (L_1 + 0.05 * sum_{j<k} L_j)
            const double l1 = (double)(in->seq_off[in->blk_off[b] + 1] - in->seq_off[in->blk_off[b]]);
            if (s > in->blk_off[b]) m.cost += (double)len * (l1 + 0.05 * prev);
            prev += (double)len;
        }
        classify_block(m, 2, h->h_params[in->per_block_params ? b : 0].banded == 0, h->long_blocks);
        // A11: the reference's abPOA path is banded (wb=311, wf=0.03); local alignments whose scores fit the packed
        // sweep run the one-wave banded kernel, everything else asked to be banded runs the full matrix
        // (global alignment: the adaptive band only -- the band of a row without successors holds the end column by
        //  construction, a band around backbone coordinates need not)
        const int bnd = h->h_params[in->per_block_params ? b : 0].banded;
        if (bnd && (m.S.sw || bnd == 2) && m.rm == 2 && m.maxlen <= SXG_POA_MAX_SEQ_LEN) {
            m.rm = 3;
            // decree B2: strip width from the block's longest sequence
            const int bw = band_strip_width(m.maxlen), bcb = band_cell_bytes(m.S);
            m.variant = Variant{bw, 1, class_tmax(bw, 1, 3, bcb, true), 3, bcb};
            m.fits = true;
        }
    }
    // letters > 4 are read as N: clamped on the device after the copy (clamp_bases_kernel; a host scan of the 320 MB of the
    // headline batch was 10 ms of every upload, the unconditional staging copy before it 0.15 s)
    laps.lap("upload: checks");
    const uint8_t* host_bases = in->bases;
    int rc;
    if ((rc = h->d_blk_off.ensure(4 * (size_t)(nb + 1)))) return rc;
    if ((rc = h->d_seq_off.ensure(8 * (size_t)(ns + 1)))) return rc;
    if ((rc = h->d_bases.ensure((size_t)nbases + 16))) return rc;
    if ((rc = h->d_params.ensure(sizeof(sxg_poa_params) * (size_t)std::max(np, 1)))) return rc;
    HIPCHK(hipMemcpyAsync(h->d_blk_off.p, in->blk_off, 4 * (size_t)(nb + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_seq_off.p, in->seq_off, 8 * (size_t)(ns + 1), hipMemcpyHostToDevice, h->stream));
    if (nbases) HIPCHK(hipMemcpyAsync(h->d_bases.p, host_bases, (size_t)nbases, hipMemcpyHostToDevice, h->stream));
    if (nbases) {
        hipLaunchKernelGGL(clamp_bases_kernel, dim3((unsigned)std::min<int64_t>((nbases / 16 + 255) / 256 + 1, 16384)), dim3(256), 0, h->stream,
                           h->d_bases.as<uint8_t>(), nbases);
        HIPCHK(hipGetLastError());
    }
    if (nb) HIPCHK(hipMemcpyAsync(h->d_params.p, in->params, sizeof(sxg_poa_params) * (size_t)np, hipMemcpyHostToDevice, h->stream));
    h->has_weights = in->weights != nullptr;
    if (h->has_weights) {
        if ((rc = h->d_weights.ensure(4 * (size_t)std::max<int64_t>(ns, 1)))) return rc;
        if (ns) HIPCHK(hipMemcpyAsync(h->d_weights.p, in->weights, 4 * (size_t)ns, hipMemcpyHostToDevice, h->stream));
    }
    if (h->want_block_graph || msa_trimmed(h->want_msa)) {
        std::vector<int32_t> trim((size_t)std::max(nb, 1), 0);
        for (int b = 0; b < nb; ++b) {
            trim[b] = in->bg_trim ? in->bg_trim[b] : 0;
            if (trim[b] < 0) return fail(SXG_E_INVALID, "bg_trim must not be negative");
        }
        if ((rc = h->d_trim.ensure(4 * trim.size()))) return rc;
        HIPCHK(hipMemcpy(h->d_trim.p, trim.data(), 4 * trim.size(), hipMemcpyHostToDevice));
        h->d_trim_h.swap(trim);
    }
    const size_t NB = (size_t)std::max<int64_t>(nbases, 1), NS = (size_t)std::max<int64_t>(ns, 1), NBL = (size_t)std::max(nb, 1);
    if ((rc = h->d_status.ensure(4 * NBL)) || (rc = h->d_nn.ensure(4 * NBL)) || (rc = h->d_ne.ensure(4 * NBL)) ||
        (rc = h->d_nc.ensure(4 * NBL)) || (rc = h->d_node_code.ensure(NB)) || (rc = h->d_node_rank.ensure(4 * NB)) ||
        (rc = h->d_node_group.ensure(4 * NB)) || (rc = h->d_edge_tail.ensure(4 * NB)) ||
        (rc = h->d_edge_head.ensure(4 * NB)) || (rc = h->d_edge_w.ensure(4 * NB)) || (rc = h->d_paths.ensure(4 * NB)) ||
        (rc = h->d_score.ensure(4 * NS)) || (rc = h->d_cells.ensure(8 * NS)) || (rc = h->d_queue.ensure(256)) ||
        (rc = h->d_work.ensure(4 * NBL)) || (rc = h->d_blk_cycles.ensure(8 * NBL)))
        return rc;
    if (h->want_consensus && (rc = h->d_cons.ensure(4 * NB))) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    laps.lap("upload: copies");
    h->have_batch = true;
    h->sh_dealt = false; h->sh_exchanged = false;   // (a plain upload: no deal the root could reassemble by)
    return SXG_OK;
}

struct LaunchPlan {
    Variant variant; bool cvx, sw; int tier = 0; bool wide_band = false;
    int tiles = 1;        // 32-bit sweep in column tiles: the tile count its blocks share (a launch of its own); 1 = no tiles
    size_t bnd_off = 0;   // where a slot's boundary buffers lie (make_layout)
    std::vector<int32_t> work;  // block ids, largest cost first
    std::vector<unsigned long long> est;  // cost-model cells per work item (priority balancing)
    // filled by prepare_plan
    SlotLayout lay; KernelFn<BlockArgs> kern = nullptr; std::string why; int per_cu = 1; int64_t want_slots = 0, n_slots = 0;
    int clock_mhz = 0;   // shader clock this launch ran at, sampled from its slots (see sample_clock)
    int smem = 0, pf_off = -1; bool park_lds = true; uint64_t cells = 0, bytes = 0; float ms = 0;
};

// Adaptive band of the packed sweep (BlockArgs::band_floor): the later alignments of a block keep
// 2 (ceil((drift + margin) / W) + 1) strips per plane row, at least `floor`, at most the layout's.  SXG_POA_BAND_ADAPT =
// "floor,margin,full" sets the three (full: alignments of a block that keep the layout's width); "0" keeps the layout's width
// for every alignment -- the fixed band, a test knob: the adaptive band changes speed, never results.
static void band_adapt_args(BlockArgs& A) {
    A.band_floor = P16_BAND_FLOOR; A.band_margin = P16_BAND_MARGIN; A.band_full = P16_BAND_FULL;
    if (const char* e = getenv("SXG_POA_BAND_ADAPT")) {
        int f = 0, m = A.band_margin, n = A.band_full;
        const int k = sscanf(e, "%d,%d,%d", &f, &m, &n);
        A.band_floor = k >= 1 && f > 0 ? plane_round4(f) : 0;
        if (k >= 2) A.band_margin = std::max(m, 0);
        if (k >= 3) A.band_full = std::max(n, 0);
    }
}

static void prepare_plan(sxg_poa_handle* h, LaunchPlan& P, int attempt) {
    const Variant V = P.variant;
    const int Lpad = V.Lpad();
    int nodes_cap = 0, maxlen = 0;
    bool any_adaptive = false;   // banded blocks with the adaptive band (B4): a row's band may span the whole 128-strip window
    bool any_spoa = false;       // blocks that ask for spoa's depth-first order: the only ones whose arena carries its scratch
    double rows_est = 0;  // graph rows a block is expected to reach: every further sequence adds ~1.5 % of its
                          // length in new nodes on pangenome-like input (measured on the synthetic blocks: 1.43 %)
    for (int b : P.work) {
        const BlockMeta& m = h->meta[b];
        any_adaptive = any_adaptive || h->h_params[h->per_block_params ? b : 0].banded == 2;
        any_spoa = any_spoa || (h->h_params[h->per_block_params ? b : 0].mode & SXG_ORDER_SPOA) != 0;
        nodes_cap = (int)std::max<int64_t>(nodes_cap, m.sumlen);
        maxlen = std::max(maxlen, m.maxlen);
        rows_est = std::max(rows_est, (double)m.maxlen * std::max(2.0, 1.0 + 0.0165 * m.nseq));
    }
    nodes_cap += 8;
    // The graph arrays (~100 B per node and edge) used to be sized for the worst case -- one node per base of the
    // block, 34 MB of a 64 x 5 kbp slot whose graph ends at ~10 k nodes and ~14 k edges.  The first two tiers size
    // them from the row estimate (edges and nodes each stay below twice the rows); a block that outgrows them
    // answers NODES_OVERFLOW and moves up a tier like any other capacity overflow.
    const int nodes_full = nodes_cap;
    int rows_cap, pool_slots, step_cap;
    if (attempt == 0) {
        rows_cap = (int)std::min<double>(nodes_cap, rows_est + 1024);
        pool_slots = std::min(rows_cap + 1, 768);
        step_cap = rows_cap;
        nodes_cap = (int)std::min<int64_t>(nodes_full, 2LL * rows_cap + maxlen + 8);
    } else if (attempt == 1) {
        rows_cap = (int)std::min<double>(nodes_cap, 2.5 * rows_est + 4096);
        pool_slots = std::min(rows_cap + 1, 4096);
        step_cap = 3 * rows_cap;
        nodes_cap = (int)std::min<int64_t>(nodes_full, 2LL * rows_cap + maxlen + 8);
    } else if (attempt == 2) {
        rows_cap = nodes_cap; pool_slots = std::min(rows_cap + 1, 32768); step_cap = nodes_cap;  // edges <= nodes_cap
    } else {
        rows_cap = nodes_cap; pool_slots = rows_cap + 1; step_cap = nodes_cap;                    // worst case
    }
    if (rows_cap >= (1 << 20)) rows_cap = (1 << 20) - 1;
    const int wb = V.RM == 1 ? 8 : 4;
    if (V.RM == 3) pool_slots = 1;   // (the banded sweep has no row ring: predecessors come from the plane)
    // (a class compiled for a plane that keeps every strip -- class_traits' rp == 2 -- gives way when the launch's plane was narrowed,
    //  SXG_POA_BAND_COLS: class_tmax)
    const int strips1 = V.RM == 3 ? (any_adaptive ? BAND_WIN : band_plane_strips(maxlen, V.W)) : (V.RM == 2 ? p16_launch_sizes(V.T(), V.W, 0, V.CB, P.wide_band).strips : 0);
    P.variant.TMAX = class_tmax(V.W, V.NW, V.RM, V.CB, strips1 == 2 * V.T());
    // The class's second strip width, for the alignments it covers (poa_kernels.hip.h).  SXG_POA_WIDTH2=0: every alignment runs at
    // the geometry's width -- the A/B inside one build, and a test knob: the width changes speed, never results.
    P.variant.W2 = width2_enabled() ? class_w2(CLASS_BLOCK, P.variant, P.sw) : 0;
    // strips per plane row at either width, on-chip rows and dynamic LDS of a packed launch: p16_launch_sizes
    const P16LaunchSizes LS = p16_launch_sizes(V.T(), V.W, P.variant.W2, V.CB, P.wide_band);
    P.lay = make_layout(nodes_cap, rows_cap, pool_slots, step_cap, V.T(), Lpad, wb, false, strips1, V.RM >= 2 ? V.CB : 4, any_spoa,
                        V.RM == 2 ? P.variant.W2 : 0, LS.strips2, P.tiles, &P.bnd_off);
    P.kern = block_kernel(P.variant, P.cvx, P.sw);
    const int tfix = class_traits(P.variant.TMAX, V.W, V.RM, V.CB).tfix;
    if (tfix && tfix != V.T()) { P.kern = nullptr; P.why = "kernel class compiled for " + std::to_string(tfix) + " threads asked to run at " + std::to_string(V.T()); }
    if (!P.kern && P.why.empty()) P.why = "no kernel class built for this geometry";   // (launch_plan fails this launch)
    P.smem = dp_lds_launch_bytes(Lpad, wb);
    P.park_lds = dp_park_in_lds(Lpad, wb);
    if (V.RM == 2) { P.lay.lds_rows = LS.lds_rows; P.smem = LS.smem; P.park_lds = true; }
    if (V.RM == 3) { P.smem = band_lds_bytes(V.W); P.park_lds = true; }
    // (the LDS-DMA prefetch knows one tile: off in sweeps of more)
    P.pf_off = (V.RM < 2 && P.tiles == 1 && getenv("SXG_POA_PREFETCH")) ? dp_pf_offset(Lpad, wb, V.T()) : -1;
    if (P.pf_off >= 0) P.smem += dp_pf_bytes(Lpad, wb, V.T());
    if (P.smem > 48 * 1024)
        (void)hipFuncSetAttribute((const void*)P.kern, hipFuncAttributeMaxDynamicSharedMemorySize, P.smem);
    P.per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&P.per_cu, (const void*)P.kern, V.T(), (size_t)P.smem) != hipSuccess || P.per_cu < 1)
        P.per_cu = 1;
    P.want_slots = std::min<int64_t>((int64_t)P.work.size(), (int64_t)h->num_cu * P.per_cu);
}

// The profiles of a launch's slots (poa_slot_prof.h), SLOT_PROF_WORDS words per slot: one strided copy out of the slot headers.
static int fetch_slot_prof(const LaunchPlan& P, const PlanRes& R, std::vector<unsigned long long>& prof) {
    prof.resize((size_t)std::max<int64_t>(P.n_slots, 0) * SLOT_PROF_WORDS);
    if (!prof.empty())
        HIPCHK(hipMemcpy2D(prof.data(), SLOT_PROF_BYTES, R.arena.as<uint8_t>() + P.lay.hdr + SLOT_PROF_OFF, P.lay.total, SLOT_PROF_BYTES, (size_t)P.n_slots,
                           hipMemcpyDeviceToHost));
    return SXG_OK;
}

// The shader clock a launch ran at: every slot reads the core-clock counter (s_memtime) and the constant 100 MHz counter
// (s_memrealtime) when it starts and when it ends; cycles / ticks * 100 MHz, over a sample of slots.  bench.py
// prices the VALU roof with it -- the boxes of the pool sustain different clocks under this kernel.
static int sample_clock(const LaunchPlan& P, const std::vector<unsigned long long>& prof) {
    unsigned long long cyc = 0, ticks = 0;
    const int64_t step = std::max<int64_t>(1, P.n_slots / 24);
    for (int64_t sl = 0; sl < P.n_slots; sl += step) {
        const unsigned long long* v = prof.data() + (size_t)sl * SLOT_PROF_WORDS;
        if (v[SP_WALL1] <= v[SP_WALL0] || v[SP_CLOCK1] <= v[SP_CLOCK0]) continue;
        cyc += v[SP_CLOCK1] - v[SP_CLOCK0];
        ticks += v[SP_WALL1] - v[SP_WALL0];
    }
    return ticks ? (int)((double)cyc / (double)ticks * 100.0 + 0.5) : 0;
}

static int launch_plan(sxg_poa_handle* h, LaunchPlan& P, PlanRes& R, const int prio_base) {
    const Variant V = P.variant;
    int rc;
    if (!P.kern) return fail(SXG_E_INVALID, P.why);
    if ((rc = R.arena.ensure((size_t)P.n_slots * P.lay.total))) return rc;
    // light CUs first, then snake: deal_over_cus (poa_cost.h).  P.work arrives sorted by the blocks' cost IN THIS LAUNCH, largest first.
    deal_over_cus(P.work, P.n_slots, std::max(h->num_cu, 1));
    if ((rc = R.work.ensure(4 * P.work.size())) || (rc = R.queue.ensure(256)) || (rc = R.est.ensure(8 * P.work.size()))) return rc;
    HIPCHK(hipMemcpyAsync(R.work.p, P.work.data(), 4 * P.work.size(), hipMemcpyHostToDevice, R.stream));
    P.est.resize(P.work.size());
    for (size_t k = 0; k < P.work.size(); ++k) P.est[k] = (unsigned long long)std::max<uint64_t>(h->blk_cost[(size_t)P.work[k]], 1);
    HIPCHK(hipMemcpyAsync(R.est.p, P.est.data(), 8 * P.est.size(), hipMemcpyHostToDevice, R.stream));
    HIPCHK(hipMemsetAsync(R.queue.p, 0, 256, R.stream));
    BlockArgs A;
    A.blk_off = h->d_blk_off.as<int32_t>(); A.seq_off = h->d_seq_off.as<int64_t>(); A.bases = h->d_bases.as<uint8_t>();
    A.weights = h->has_weights ? h->d_weights.as<uint32_t>() : nullptr;
    A.params = h->d_params.as<sxg_poa_params>(); A.per_block_params = h->per_block_params;
    A.n_tiles = P.tiles; A.bnd_off256 = (unsigned)(P.bnd_off / 256);   // (make_layout aligns every array to 256 bytes)
    A.work = R.work.as<int32_t>(); A.n_work = (int)P.work.size(); A.queue = R.queue.as<int32_t>();
    A.arena = R.arena.as<uint8_t>(); A.lay = P.lay;
    A.status = h->d_status.as<int32_t>(); A.n_nodes = h->d_nn.as<int32_t>(); A.n_edges = h->d_ne.as<int32_t>();
    A.n_cons = h->d_nc.as<int32_t>(); A.node_code = h->d_node_code.as<uint8_t>();
    A.node_rank = h->d_node_rank.as<int32_t>(); A.node_group = h->d_node_group.as<int32_t>();
    A.edge_tail = h->d_edge_tail.as<int32_t>(); A.edge_head = h->d_edge_head.as<int32_t>();
    A.edge_weight = h->d_edge_w.as<uint32_t>(); A.paths = h->d_paths.as<int32_t>(); A.score = h->d_score.as<int32_t>();
    A.cells = h->d_cells.as<unsigned long long>(); A.cons_nodes = h->d_cons.as<int32_t>();
    A.want_consensus = h->want_consensus;
    A.park_in_lds = P.park_lds ? 1 : 0;
    A.pf_off = P.pf_off;
    A.num_cu = std::max(h->num_cu, 1);
    // One board for all launches of the round: workgroups of different geometries share CUs, and each takes as priority
    // the number of co-residents -- of ANY launch -- with less work left.  (Round 3 kept a board per launch: two launches
    // side by side were balanced pair by pair and lost more than their narrower geometry saved.)
    A.prio_board = getenv("SXG_POA_NO_BALANCE") ? nullptr : h->d_board.as<uint32_t>();
    A.prio_base = prio_base;
    A.est = R.est.as<unsigned long long>();
    A.est_done = h->d_est_done.as<unsigned long long>();   // (uploaded on h->stream in front of ev0, which this launch waits for)
    A.blk_cycles = h->d_blk_cycles.as<unsigned long long>();
    A.lds_bytes = getenv("SXG_POA_RESORT_NO_LDS") ? 0 : P.smem;   // (test knob: the S7' re-sort keeps its states in the slot's scratch, as it does for graphs beyond its LDS)
    band_adapt_args(A);
    A.twin = twin_enabled() ? 1 : 0;
    // every slot's header (counters, phase times, clock readings) starts a launch at zero: one strided memset
    HIPCHK(hipMemset2DAsync(R.arena.as<uint8_t>() + P.lay.hdr, P.lay.total, 0, SLOT_HDR_BYTES, (size_t)P.n_slots, R.stream));
    HIPCHK(hipStreamWaitEvent(R.stream, h->ev0, 0));
    HIPCHK(hipEventRecord(R.e0, R.stream));
    hipLaunchKernelGGL(P.kern, dim3((unsigned)P.n_slots), dim3(V.T()), (size_t)P.smem, R.stream, A);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(R.e1, R.stream));
    HIPCHK(hipStreamWaitEvent(h->stream, R.e1, 0));
    return SXG_OK;
}

// Packed sweep: what the launch's sweeps ran at, from its slots' profiles (fetch_slot_prof).
static void width_stats_of(const LaunchPlan& P, const std::vector<unsigned long long>& prof, sxg_poa_width_stats& w, sxg_poa_twin_stats* tw = nullptr) {
    if (P.variant.RM != 2) return;
    for (int64_t sl = 0; sl < P.n_slots; ++sl) {
        const unsigned long long* c = prof.data() + (size_t)sl * SLOT_PROF_WORDS;
        w.hint_shift_repeats += c[SP_HINT_REPEATS];
        for (int k = 0; k < 2; ++k) { w.sweeps[k] += c[SP_SWEEPS + k]; w.swept_cols[k] += c[SP_SWEPT_COLS + k]; w.swept_cells[k] += c[SP_SWEPT_CELLS + k]; }
        if (tw) { tw->twin_steps += c[SP_TWIN] & 0xffffffffull; tw->join_rows += c[SP_TWIN] >> 32; }
    }
}

// SXG_POA_DEBUG: what a launch did, from its slots' profiles (stderr; SXG_POA_SLOT_CSV: one line per slot appended to that file)
static void debug_plan(const LaunchPlan& P, const std::vector<unsigned long long>& prof, int attempt) {
    const Variant V = P.variant;
    auto word_sum = [&](int k) {   // word k of the profile, summed over the slots
        unsigned long long sum = 0;
        for (int64_t sl = 0; sl < P.n_slots; ++sl) sum += prof[(size_t)sl * SLOT_PROF_WORDS + k];
        return sum;
    };
    unsigned long long acc[SP_PHASES], smin = ~0ull, smax = 0;
    for (int k = 0; k < SP_PHASES; ++k) acc[k] = word_sum(k);
    for (int64_t sl = 0; sl < P.n_slots; ++sl) {
        unsigned long long st = 0;
        for (int k = 0; k < SP_PHASES; ++k) st += prof[(size_t)sl * SLOT_PROF_WORDS + k];
        smin = std::min(smin, st); smax = std::max(smax, st);
    }
    if (V.RM == 2) {   // packed sweep: the width of the plane rows the sweeps kept (adaptive band) and the hint-shift repeats
        const unsigned long long rep = word_sum(SP_HINT_REPEATS), wsum = word_sum(SP_BAND_STRIPS), nsw = word_sum(SP_BAND_SWEEPS);
        fprintf(stderr, "[sxg]   band: %llu sweeps, mean width %.1f strips of %d (%.0f columns), %llu hint-shift repeats\n", nsw,
                (double)wsum / (double)std::max(nsw, 1ull), P.lay.band_strips, (double)wsum / (double)std::max(nsw, 1ull) * V.W, rep);
        // (with a second width the band line's strips are a mix of both widths' and its columns an upper bound)
        sxg_poa_width_stats w{};
        sxg_poa_twin_stats tw{};
        width_stats_of(P, prof, w, &tw);
        fprintf(stderr, "[sxg]   width: W=%d %llu sweeps %llu columns %.4g cells; W2=%d %llu sweeps %llu columns %.4g cells\n", V.W, (unsigned long long)w.sweeps[0],
                (unsigned long long)w.swept_cols[0], (double)w.swept_cells[0], P.lay.W2, (unsigned long long)w.sweeps[1], (unsigned long long)w.swept_cols[1], (double)w.swept_cells[1]);
        fprintf(stderr, "[sxg]   twin: %llu twin steps, %llu join rows\n", (unsigned long long)tw.twin_steps, (unsigned long long)tw.join_rows);
    }
    if (const char* path = getenv("SXG_POA_SLOT_CSV")) {  // per-slot placement and wall-clock span
        if (FILE* f = fopen(path, "a")) {
            for (int64_t sl = 0; sl < P.n_slots; ++sl) {
                const unsigned long long* v = prof.data() + (size_t)sl * SLOT_PROF_WORDS;
                fprintf(f, "%lld,%llu,%llu", (long long)sl, v[SP_WALL0], v[SP_WALL1]);
                for (int w = 0; w < V.NW && w < SP_WAVES; ++w) fprintf(f, ",%llx", v[SP_WAVE + w]);
                fprintf(f, "\n");
            }
            fclose(f);
        }
    }
#ifdef SXG_ROW_PROF
    {
        unsigned long long ra[ROWP_WORDS];
        for (int k = 0; k < ROWP_WORDS; ++k) ra[k] = word_sum(SP_ROW + k);
        double rt = 1e-9;
        for (int k = 0; k < ROWP_SEGS; ++k) rt += (double)ra[k];
        static const char* seg16[ROWP_SEGS] = {"setup", "pass1+scan", "wait left wave", "combine+pass2", "wait right wave", "hand-over+end cell", "stored row fetch", "outgoing+row store"};
        static const char* segb[ROWP_SEGS] = {"descriptor+band", "predecessor fetch+fold", "pass1+scan+pass2", "end cell+best-cell search", "outgoing+band stores", "-", "-", "-"};
        const char* const* seg = V.RM == 3 ? segb : seg16;
        fprintf(stderr, "[sxg]   row profile:");
        for (int k = 0; k < ROWP_SEGS; ++k) fprintf(stderr, " %s %.1f%%", seg[k], 100.0 * (double)ra[k] / rt);
        fprintf(stderr, "\n");
        fprintf(stderr, "[sxg]   traceback: %.3g steps, %.1f steps per window, %.0f %% of the windows prefetched, %.0f cycles per step of which %.0f in window fills\n",
                (double)ra[ROWP_TB_STEPS], (double)ra[ROWP_TB_STEPS] / std::max<double>((double)ra[ROWP_TB_LOADS], 1),
                100.0 * (double)ra[ROWP_TB_HITS] / std::max<double>((double)ra[ROWP_TB_LOADS], 1),
                (double)ra[ROWP_TB_CYCLES] / std::max<double>((double)ra[ROWP_TB_STEPS], 1), (double)ra[ROWP_TB_FILL_CYCLES] / std::max<double>((double)ra[ROWP_TB_STEPS], 1));
    }
#endif
#ifdef SXG_RESORT_PROF
    {   // phases of the S7' re-sort (poa_graph_dev.h::spoa_resort_par), thread 0's clock
        unsigned long long ra[RSP_WORDS];
        for (int k = 0; k < RSP_WORDS; ++k) ra[k] = word_sum(SP_RESORT + k);
        double rt = 1e-9;
        for (int k = 0; k < RSP_PHASES; ++k) rt += (double)ra[k];
        fprintf(stderr, "[sxg]   re-sort: records %.1f%% first() %.1f%% counts %.1f%% walks %.1f%% ranks %.1f%%; %.3g cycles per slot, %.1f rounds per slot\n",
                100 * ra[0] / rt, 100 * ra[1] / rt, 100 * ra[2] / rt, 100 * ra[3] / rt, 100 * ra[4] / rt, rt / (double)P.n_slots, (double)ra[RSP_ROUNDS] / (double)P.n_slots);
    }
#endif
    double tot = 1e-9;
    for (int k = 0; k < SP_PHASES; ++k) tot += (double)acc[k];
    size_t fr = 0, tt = 0;
    (void)hipMemGetInfo(&fr, &tt);
    fprintf(stderr, "[sxg] variant T=%d W=%d cvx=%d rowmode=%d attempt=%d work=%zu slots=%lld per_cu=%d smem=%d slot_bytes=%zu free=%zu ms=%.2f tmax=%d cb=%d ds=%d w2=%d\n",
            V.T(), V.W, (int)P.cvx, V.RM, attempt, P.work.size(), (long long)P.n_slots, P.per_cu, P.smem, P.lay.total, fr, P.ms,
            V.TMAX, V.CB, (int)V.DS, V.W2);   // (the class that ran: tests read these)
    fprintf(stderr, "[sxg]   slot busy (of the longest slot): min %.1f%% mean %.1f%%\n", 100.0 * (double)smin / (double)std::max(smax, 1ull),
            100.0 * tot / (double)P.n_slots / (double)std::max(smax, 1ull));
    fprintf(stderr, "[sxg]   slot time: other %.1f%% prep_rows %.1f%% dp_fill %.1f%% traceback %.1f%% add_alignment %.1f%% output %.1f%%\n",
            100 * acc[SP_OTHER] / tot, 100 * acc[SP_PREP_ROWS] / tot, 100 * acc[SP_DP_FILL] / tot, 100 * acc[SP_TRACEBACK] / tot, 100 * acc[SP_ADD_ALIGNMENT] / tot,
            100 * acc[SP_OUTPUT] / tot);
}

// A9 + A10 of every block on the device (block_graph_kernel), after the batch's alignments: outputs in per-block
// layouts (nodes: prefix of the POA node counts, edges: prefix of POA edges + consensus nodes, steps: the input layout).
static int run_block_graphs(sxg_poa_handle* h, std::vector<int32_t>& status) {
    const int nb = h->n_blocks;
    h->bg_done = false;
    std::vector<int32_t> nn(std::max(nb, 1), 0), ne(std::max(nb, 1), 0), nc(std::max(nb, 1), 0);
    if (nb) {
        HIPCHK(hipMemcpy(nn.data(), h->d_nn.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ne.data(), h->d_ne.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nc.data(), h->d_nc.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
    }
    h->bg_node_o.assign((size_t)nb + 1, 0); h->bg_edge_o.assign((size_t)nb + 1, 0);
    int capV = 1, capE = 1, capC = 1, capT = 1;
    std::vector<int32_t> work;
    for (int b = 0; b < nb; ++b) {
        const bool ok = status[b] == ST_OK && h->meta[b].nseq > 0;
        const int cn = h->want_consensus ? nc[b] : 0;
        h->bg_node_o[(size_t)b + 1] = h->bg_node_o[(size_t)b] + (ok ? nn[b] : 0);
        h->bg_edge_o[(size_t)b + 1] = h->bg_edge_o[(size_t)b] + (ok ? ne[b] + cn : 0);
        if (!ok) continue;
        work.push_back(b);
        capV = std::max(capV, nn[b]); capE = std::max(capE, ne[b]); capC = std::max(capC, cn);
        capT = std::max(capT, std::max(std::max(nn[b], h->meta[b].maxlen), cn));
    }
    std::stable_sort(work.begin(), work.end(), [&](int a, int b) { return h->meta[a].sumlen > h->meta[b].sumlen; });
    const size_t NT = (size_t)std::max<int64_t>(h->bg_node_o[(size_t)nb], 1), ET = (size_t)std::max<int64_t>(h->bg_edge_o[(size_t)nb], 1);
    const size_t NB = (size_t)std::max<int64_t>(h->n_bases, 1), NS = (size_t)std::max<int64_t>(h->n_seqs, 1), NBL = (size_t)std::max(nb, 1);
    int rc;
    if ((rc = h->d_bg_no.ensure(8 * (NBL + 1))) || (rc = h->d_bg_eo.ensure(8 * (NBL + 1))) || (rc = h->d_bg_len.ensure(4 * NT)) ||
        (rc = h->d_bg_od.ensure(4 * NT)) || (rc = h->d_bg_id.ensure(NT)) || (rc = h->d_bg_seq.ensure(NT)) || (rc = h->d_bg_eto.ensure(4 * ET)) ||
        (rc = h->d_bg_steps.ensure(4 * NB)) || (rc = h->d_bg_nsteps.ensure(4 * NS)) || (rc = h->d_bg_cons.ensure(4 * NT)) ||
        (rc = h->d_bg_counts.ensure(4 * (size_t)BGC_N * NBL)) || (rc = h->d_bg_work.ensure(4 * std::max<size_t>(work.size(), 1))) ||
        (rc = h->d_bg_queue.ensure(256)))
        return rc;
    HIPCHK(hipMemcpyAsync(h->d_bg_no.p, h->bg_node_o.data(), 8 * ((size_t)nb + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_bg_eo.p, h->bg_edge_o.data(), 8 * ((size_t)nb + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_bg_counts.p, 0, 4 * (size_t)BGC_N * NBL, h->stream));
    HIPCHK(hipMemsetAsync(h->d_bg_nsteps.p, 0, 4 * NS, h->stream));
    HIPCHK(hipMemsetAsync(h->d_bg_queue.p, 0, 256, h->stream));
    if (!work.empty()) {
        HIPCHK(hipMemcpyAsync(h->d_bg_work.p, work.data(), 4 * work.size(), hipMemcpyHostToDevice, h->stream));
        const size_t slot = bg_slot_bytes(capV, capE, capC, capT);
        int per_cu = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)block_graph_kernel, BG_THREADS, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        int64_t slots = std::min<int64_t>((int64_t)work.size(), (int64_t)h->num_cu * per_cu);
        slots = std::max<int64_t>(1, std::min<int64_t>(slots, (int64_t)(arena_budget(h) / slot)));
        if ((rc = h->d_bg_arena.ensure((size_t)slots * slot))) return rc;
        BgArgs A;
        A.blk_off = h->d_blk_off.as<int32_t>(); A.seq_off = h->d_seq_off.as<int64_t>(); A.bases = h->d_bases.as<uint8_t>();
        A.paths = h->d_paths.as<int32_t>(); A.node_code = h->d_node_code.as<uint8_t>(); A.edge_tail = h->d_edge_tail.as<int32_t>();
        A.edge_head = h->d_edge_head.as<int32_t>(); A.cons = h->want_consensus ? h->d_cons.as<int32_t>() : nullptr;
        A.nn = h->d_nn.as<int32_t>(); A.ne = h->d_ne.as<int32_t>(); A.nc = h->d_nc.as<int32_t>(); A.trim = h->d_trim.as<int32_t>();
        A.cons_mode = h->bg_cons_visited_only ? 2 : 1;
        A.work = h->d_bg_work.as<int32_t>(); A.n_work = (int)work.size(); A.queue = h->d_bg_queue.as<int32_t>();
        A.arena = h->d_bg_arena.as<uint8_t>(); A.slot_bytes = slot; A.capV = capV; A.capE = capE; A.capC = capC; A.capT = capT;
        A.node_o = h->d_bg_no.as<int64_t>(); A.edge_o = h->d_bg_eo.as<int64_t>();
        A.o_len = h->d_bg_len.as<int32_t>(); A.o_outdeg = h->d_bg_od.as<int32_t>(); A.o_indeg = h->d_bg_id.as<uint8_t>();
        A.o_seq = h->d_bg_seq.as<char>(); A.o_eto = h->d_bg_eto.as<int32_t>(); A.o_steps = h->d_bg_steps.as<int32_t>();
        A.o_nsteps = h->d_bg_nsteps.as<int32_t>(); A.o_cons = h->d_bg_cons.as<int32_t>(); A.o_counts = h->d_bg_counts.as<int32_t>();
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        hipLaunchKernelGGL(block_graph_kernel, dim3((unsigned)slots), dim3(BG_THREADS), 0, h->stream, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    if (!work.empty()) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1)); h->stats.bg_ms = ms; }
    h->bg_counts.assign((size_t)BGC_N * NBL, 0);
    if (nb) HIPCHK(hipMemcpy(h->bg_counts.data(), h->d_bg_counts.p, 4 * (size_t)BGC_N * (size_t)nb, hipMemcpyDeviceToHost));
    bool changed = false;
    for (int b : work)
        if (h->bg_counts[(size_t)BGC_N * b + BGC_STATUS] != ST_OK) { status[b] = ST_INTERNAL; changed = true; }
    if (changed) HIPCHK(hipMemcpy(h->d_status.p, status.data(), 4 * (size_t)nb, hipMemcpyHostToDevice));
    h->bg_done = true;
    return SXG_OK;
}

// The trimmed MSA of every block on the device (poa_msa.hip.h), after the batch's alignments: the columns kernel leaves every
// node's column and every block's kept columns [b0, e0); the host turns the nb pairs into widths, offsets and the flat list of
// (block, row, chunk) items; the rows kernel writes the rows, which stay in HBM until the download.
static int run_msa_rows(sxg_poa_handle* h, const std::vector<int32_t>& status) {
    const int nb = h->n_blocks;
    h->msa_done = false; h->msa_cols_ms = 0; h->msa_rows_ms = 0;
    h->msa_off_h.assign((size_t)nb + 1, 0); h->msa_cols_h.assign((size_t)std::max(nb, 1), 0);
    std::vector<int32_t> nc(std::max(nb, 1), 0), nn(std::max(nb, 1), 0), work;
    if (nb && h->want_consensus) HIPCHK(hipMemcpy(nc.data(), h->d_nc.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
    if (nb) HIPCHK(hipMemcpy(nn.data(), h->d_nn.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
    std::vector<int64_t> node_o((size_t)nb + 1, 0);   // columns and scan scratch in a compact layout: the nodes the blocks really have
    for (int b = 0; b < nb; ++b) {
        const bool live = status[b] == ST_OK && h->meta[b].nseq > 0;
        if (live && (nn[b] < 0 || nn[b] > h->meta[b].sumlen)) return fail(SXG_E_NODEVICE, "node count of block " + std::to_string(b) + " out of range");
        node_o[(size_t)b + 1] = node_o[(size_t)b] + (live ? nn[b] : 0);
        if (live) work.push_back(b);
    }
    h->msa_live_h.assign((size_t)std::max(nb, 1), 0);
    for (int b : work) h->msa_live_h[(size_t)b] = 1;
    std::stable_sort(work.begin(), work.end(), [&](int a, int b) { return h->meta[a].sumlen > h->meta[b].sumlen; });
    const size_t NN = (size_t)std::max<int64_t>(node_o[(size_t)nb], 1), NBL = (size_t)std::max(nb, 1);
    int rc;
    if ((rc = h->d_msa_tmp.ensure(4 * NN)) || (rc = h->d_msa_col.ensure(4 * NN)) || (rc = h->d_msa_be.ensure(8 * NBL)) || (rc = h->d_msa_no.ensure(8 * (NBL + 1))) ||
        (rc = h->d_msa_off.ensure(8 * (NBL + 1))) || (rc = h->d_msa_work.ensure(4 * std::max<size_t>(work.size(), 1))) ||
        (rc = h->d_msa_queue.ensure(256)))
        return rc;
    if (work.empty()) { h->msa_done = true; return SXG_OK; }
    HIPCHK(hipMemsetAsync(h->d_msa_be.p, 0, 8 * NBL, h->stream));
    HIPCHK(hipMemsetAsync(h->d_msa_queue.p, 0, 256, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_msa_work.p, work.data(), 4 * work.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_msa_no.p, node_o.data(), 8 * ((size_t)nb + 1), hipMemcpyHostToDevice, h->stream));
    MsaColsArgs C;
    C.blk_off = h->d_blk_off.as<int32_t>(); C.seq_off = h->d_seq_off.as<int64_t>(); C.paths = h->d_paths.as<int32_t>();
    C.cons = h->want_consensus ? h->d_cons.as<int32_t>() : nullptr;
    C.node_rank = h->d_node_rank.as<int32_t>(); C.node_group = h->d_node_group.as<int32_t>();
    C.nn = h->d_nn.as<int32_t>(); C.nc = h->d_nc.as<int32_t>(); C.trim = h->d_trim.as<int32_t>();
    C.work = h->d_msa_work.as<int32_t>(); C.n_work = (int32_t)work.size(); C.queue = h->d_msa_queue.as<int32_t>();
    C.node_o = h->d_msa_no.as<int64_t>(); C.tmp = h->d_msa_tmp.as<int32_t>(); C.col = h->d_msa_col.as<int32_t>(); C.be = h->d_msa_be.as<int32_t>();
    const int slots_c = (int)std::min<int64_t>((int64_t)work.size(), (int64_t)h->num_cu * 8);
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    sxg_msa_launch_cols(C, slots_c, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    std::vector<int32_t> be(2 * NBL, 0);
    HIPCHK(hipMemcpyAsync(be.data(), h->d_msa_be.p, 8 * (size_t)nb, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1)); h->msa_cols_ms = ms; }
    std::vector<char> live((size_t)NBL, 0);
    for (int b : work) live[(size_t)b] = 1;
    std::vector<MsaItem> items;
    for (int b = 0; b < nb; ++b) {
        const int64_t cols = live[(size_t)b] ? (int64_t)be[2 * (size_t)b + 1] - be[2 * (size_t)b] : 0;
        if (cols < 0 || cols > 0x7fffffff) return fail(SXG_E_NODEVICE, "MSA columns kernel returned an impossible width for block " + std::to_string(b));
        const int rows = h->meta[b].nseq + (h->want_consensus ? 1 : 0);
        h->msa_cols_h[(size_t)b] = (int32_t)cols;
        h->msa_off_h[(size_t)b + 1] = h->msa_off_h[(size_t)b] + (live[(size_t)b] ? (int64_t)rows * cols : 0);
        if (!cols) continue;
        const int64_t trim = h->d_trim_h.empty() ? 0 : h->d_trim_h[(size_t)b];
        for (int row = 0; row < rows; ++row) {
            const int s = h->h_blk_off[b] + row;
            const int64_t len = row < h->meta[b].nseq ? h->h_seq_off[(size_t)s + 1] - h->h_seq_off[(size_t)s] : nc[(size_t)b];
            int64_t k0, k1;
            sxg_msa_kept(len, trim, &k0, &k1);
            const int64_t n_chunks = sxg_msa_chunks(k0, k1, SXG_MSA_CHUNK);
            for (int64_t c = 0; c < n_chunks; ++c) items.push_back(MsaItem{b, row, (int32_t)c, 0});
        }
    }
    const int64_t total = h->msa_off_h[(size_t)nb];
    if ((rc = h->d_msa.ensure((size_t)std::max<int64_t>(total, 16) + 16))) return rc;
    if (!items.empty()) {
        if ((rc = h->d_msa_items.ensure(sizeof(MsaItem) * items.size()))) return rc;
        HIPCHK(hipMemcpyAsync(h->d_msa_off.p, h->msa_off_h.data(), 8 * ((size_t)nb + 1), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_msa_items.p, items.data(), sizeof(MsaItem) * items.size(), hipMemcpyHostToDevice, h->stream));
        MsaRowsArgs R;
        R.blk_off = C.blk_off; R.seq_off = C.seq_off; R.paths = C.paths; R.cons = C.cons; R.node_code = h->d_node_code.as<uint8_t>();
        R.nn = C.nn; R.nc = C.nc; R.trim = C.trim; R.col = C.col; R.node_o = C.node_o; R.be = C.be; R.msa_off = h->d_msa_off.as<int64_t>();
        R.items = h->d_msa_items.as<MsaItem>(); R.n_items = (int64_t)items.size();
        R.msa = h->d_msa.as<char>(); R.msa_bytes = total;
        const int slots_r = (int)std::min<int64_t>((int64_t)items.size(), (int64_t)h->num_cu * 8);
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        sxg_msa_launch_rows(R, slots_r, h->stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1)); h->msa_rows_ms = ms; }
    }
    h->msa_done = true;
    return SXG_OK;
}

extern "C" void sxg_poa_msa_geometry(int32_t* chunk_letters, int32_t* tile_bytes) {
    if (chunk_letters) *chunk_letters = SXG_MSA_CHUNK;
    if (tile_bytes) *tile_bytes = SXG_MSA_TILE;
}

extern "C" int sxg_poa_get_msa_stats(sxg_poa_handle* h, double* cols_ms, double* rows_ms, uint64_t* msa_bytes) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (cols_ms) *cols_ms = h->msa_cols_ms;
    if (rows_ms) *rows_ms = h->msa_rows_ms;
    if (msa_bytes) *msa_bytes = h->msa_done && !h->msa_off_h.empty() ? (uint64_t)h->msa_off_h.back() : 0;
    return SXG_OK;
}

// The resident rows of the executed batch, for sxg_poa_msa_row_letters and sxg_poa_maf_text: which batch qualifies, and where
// every row (global row index: block after block, live blocks only) starts in d_msa -- on the host for the checks, on the device
// for the letters kernel.
static int msa_resident_rows(sxg_poa_handle* h, const char* what) {
    if (!h->have_batch || !h->executed || !h->msa_done || !msa_trimmed(h->want_msa))
        return fail(SXG_E_INVALID, std::string(what) + ": the handle holds no resident trimmed MSA (want_msa = SXG_MSA_TRIMMED or SXG_MSA_TRIMMED_RESIDENT, executed, nothing uploaded since)");
    if (h->msa_rows_staged) return SXG_OK;
    const int nb = h->n_blocks;
    if (h->msa_off_h.size() != (size_t)nb + 1 || h->msa_cols_h.size() < (size_t)nb) return fail(SXG_E_INVALID, std::string(what) + ": the trimmed MSA's offsets do not match the batch");
    h->msa_row_begin_h.assign(1, 0);
    for (int b = 0; b < nb; ++b) {
        const int64_t cols = h->msa_cols_h[(size_t)b], bytes = h->msa_off_h[(size_t)b + 1] - h->msa_off_h[(size_t)b];
        const int rows_all = h->meta[b].nseq + (h->want_consensus ? 1 : 0);
        // (a live block owns rows x cols bytes, cols possibly 0; a block that is not live owns none and has no rows)
        const bool live = (size_t)b < h->msa_live_h.size() && h->msa_live_h[(size_t)b];
        const int rows = live ? rows_all : 0;
        if (bytes != (int64_t)rows * cols) return fail(SXG_E_INVALID, std::string(what) + ": block " + std::to_string(b) + " of the trimmed MSA is not rows x columns");
        for (int r = 0; r < rows; ++r) h->msa_row_begin_h.push_back(h->msa_off_h[(size_t)b] + (int64_t)(r + 1) * cols);
    }
    if ((uint64_t)h->msa_row_begin_h.back() > h->d_msa.cap) return fail(SXG_E_INVALID, std::string(what) + ": the trimmed MSA does not fit its buffer");
    if (int rc = h->d_maf_rowb.ensure(8 * h->msa_row_begin_h.size())) return rc;
    HIPCHK(hipMemcpy(h->d_maf_rowb.p, h->msa_row_begin_h.data(), 8 * h->msa_row_begin_h.size(), hipMemcpyHostToDevice));
    h->msa_rows_staged = true;
    return SXG_OK;
}

extern "C" int sxg_poa_msa_row_letters(sxg_poa_handle* h, int32_t* letters) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    HIPCHK(hipSetDevice(h->device));
    const RoctxRange range_("sxg_poa_msa_row_letters");
    if (int rc = msa_resident_rows(h, "msa_row_letters")) return rc;
    const int64_t n_rows = (int64_t)h->msa_row_begin_h.size() - 1;
    if (n_rows == 0) return SXG_OK;
    if (!letters) return fail(SXG_E_INVALID, "msa_row_letters: letters is NULL");
    // the kernel reads whole aligned 16-byte words: the last one ends at most 15 bytes behind the rows, inside the allocation
    if ((((uint64_t)h->msa_row_begin_h.back() + 15) & ~(uint64_t)15) > h->d_msa.cap) return fail(SXG_E_INVALID, "msa_row_letters: the rows' buffer is not padded to 16 bytes");
    if (int rc = h->d_maf_letters.ensure(4 * (size_t)n_rows)) return rc;
    MafLettersArgs A;
    A.rows = h->d_msa.as<uint8_t>(); A.row_begin = h->d_maf_rowb.as<int64_t>(); A.letters = h->d_maf_letters.as<int32_t>(); A.n_rows = n_rows;
    const int64_t groups = std::min<int64_t>((n_rows + SXG_MAF_THREADS / 64 - 1) / (SXG_MAF_THREADS / 64), (int64_t)std::max(h->num_cu, 1) * 8);
    sxg_maf_launch_letters(A, (int)groups, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(letters, h->d_maf_letters.p, 4 * (size_t)n_rows, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return SXG_OK;
}

extern "C" void sxg_poa_maf_text_geometry(int32_t* chunk_bytes) {
    if (chunk_bytes) *chunk_bytes = SXG_MAF_CHUNK;
}

extern "C" int sxg_poa_maf_text_stats(sxg_poa_handle* h, double* kernel_ms, uint64_t* bytes) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (kernel_ms) *kernel_ms = h->maf_text_ms;
    if (bytes) *bytes = h->maf_text_bytes;
    return SXG_OK;
}

extern "C" int sxg_poa_maf_text(sxg_poa_handle* h, const sxg_poa_maf_text_in* in, char* out, int64_t out_bytes) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    HIPCHK(hipSetDevice(h->device));
    const RoctxRange range_("sxg_poa_maf_text");
    if (int rc = msa_resident_rows(h, "maf_text")) return rc;
    const int64_t n = in->n_segs, n_rows = (int64_t)h->msa_row_begin_h.size() - 1;
    if (n < 0 || (n > 0 && !in->segs) || in->literal_bytes < 0 || (in->literal_bytes > 0 && !in->literal)) return fail(SXG_E_INVALID, "maf_text: NULL arrays");
    // every segment against its source, before anything is launched: a mistake comes back as a return code, not as a fault of the device
    std::vector<int64_t> off((size_t)n + 1, 0), srck((size_t)std::max<int64_t>(n, 1), 0);
    for (int64_t s = 0; s < n; ++s) {
        const sxg_poa_maf_seg& g = in->segs[s];
        const std::string name = "maf_text: segment " + std::to_string(s);
        if (g.len < 0) return fail(SXG_E_INVALID, name + " has a negative length");
        int64_t start = 0;
        if (g.kind == SXG_MAF_LITERAL) {
            if (g.src < 0 || g.src > in->literal_bytes || g.len > in->literal_bytes - g.src) return fail(SXG_E_INVALID, name + " lies outside the literal bytes");
            start = g.src;
        } else if (g.kind == SXG_MAF_ROW || g.kind == SXG_MAF_ROW_REVCOMP) {
            if (g.src < 0 || g.src >= n_rows) return fail(SXG_E_INVALID, name + " names row " + std::to_string(g.src) + " of " + std::to_string(n_rows));
            start = h->msa_row_begin_h[(size_t)g.src];
            if (g.len != h->msa_row_begin_h[(size_t)g.src + 1] - start) return fail(SXG_E_INVALID, name + ": len is not the msa_cols of the row's block");
            if ((uint64_t)(start + g.len) > h->d_msa.cap) return fail(SXG_E_INVALID, name + " reads outside the rows' buffer");
        } else return fail(SXG_E_INVALID, name + " has kind " + std::to_string(g.kind));
        off[(size_t)s + 1] = off[(size_t)s] + g.len;
        srck[(size_t)s] = start * 4 + g.kind;
    }
    const int64_t total = off[(size_t)n];
    if (out_bytes != total) return fail(SXG_E_INVALID, "maf_text: out_bytes is " + std::to_string(out_bytes) + ", the segments hold " + std::to_string(total));
    if (total == 0) return SXG_OK;
    if (!out) return fail(SXG_E_INVALID, "maf_text: out is NULL");
    int rc;
    const size_t padded = ((size_t)total + 15) & ~(size_t)15;   // (the last granule is stored whole)
    if ((rc = h->d_maf_off.ensure(8 * ((size_t)n + 1))) || (rc = h->d_maf_srck.ensure(8 * (size_t)n)) || (rc = h->d_maf_lit.ensure((size_t)std::max<int64_t>(in->literal_bytes, 16))) ||
        (rc = h->d_maf_text.ensure(padded)))
        return rc;
    if (!h->maf_e0.raw) HIPCHK(h->maf_e0.create());
    if (!h->maf_e1.raw) HIPCHK(h->maf_e1.create());
    HIPCHK(hipMemcpyAsync(h->d_maf_off.p, off.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_maf_srck.p, srck.data(), 8 * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (in->literal_bytes) HIPCHK(hipMemcpyAsync(h->d_maf_lit.p, in->literal, (size_t)in->literal_bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // (the host arrays above leave scope with this call; pageable copies may still be staged)
    MafTextArgs A;
    A.literal = h->d_maf_lit.as<uint8_t>(); A.rows = h->d_msa.as<uint8_t>(); A.dst = h->d_maf_text.as<uint8_t>();
    A.dst_off = h->d_maf_off.as<int64_t>(); A.srck = h->d_maf_srck.as<int64_t>(); A.n = n; A.total = total;
    const int64_t groups = std::min<int64_t>(sxg_maf_n_chunks(total), (int64_t)std::max(h->num_cu, 1) * 8);
    HIPCHK(hipEventRecord(h->maf_e0, h->stream));
    sxg_maf_launch_text(A, (int)groups, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->maf_e1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->maf_e0, h->maf_e1)); h->maf_text_ms += ms; h->maf_text_bytes += (uint64_t)total; }
    // (the staging of the MSA rows' download: one straight copy into the caller's memory)
    HIPCHK(hipMemcpy(out, h->d_maf_text.p, (size_t)total, hipMemcpyDeviceToHost));
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
// The steps of sxg_poa_batch_execute, in the order a round runs them.

// group by (variant, convex, local, capacity tier): one launch per group, all groups concurrently
static void group_pending(sxg_poa_handle* h, std::vector<LaunchPlan>& plans, const std::vector<int32_t>& pending) {
    for (int b : pending) {
        const BlockMeta& m = h->meta[b];
        LaunchPlan* pl = nullptr;
        for (auto& q : plans)
            if (q.variant == m.variant && q.cvx == m.cvx && q.sw == m.sw && q.tier == m.tier && q.wide_band == m.wide_band && q.tiles == m.tiles) { pl = &q; break; }
        if (!pl) { plans.emplace_back(); pl = &plans.back(); pl->variant = m.variant; pl->cvx = m.cvx; pl->sw = m.sw; pl->tier = m.tier; pl->wide_band = m.wide_band; pl->tiles = m.tiles; }
        pl->work.push_back(b);
    }
    std::sort(plans.begin(), plans.end(), [](const LaunchPlan& a, const LaunchPlan& b) { return a.variant.Lpad() > b.variant.Lpad(); });
}

static void merge_plans(sxg_poa_handle* h, std::vector<LaunchPlan>& plans) {
    // a geometry with at least 75 % of the columns of a wider one of the same kind joins it: fewer,
    // fuller launches beat many partial ones, but every joined block sweeps the wider geometry's columns
    // (measured on the mixed batch, round 2 with over-subscribed launches: 0.60 39.6 s, 0.75 33.8 s, 0.90 34.3 s)
    // Round 4, with ONE priority board for all launches of a round: the headline's two geometries (5 120 and 5 632 columns)
    // run 2.4 % faster apart than merged (2 137 -> 2 088 ms, same box) and the mixed batch 1.8 %; the small geometries of
    // config 2 (three launches of 1-2 waves per block) still lose 15 % apart.  So: wide geometries merge only within 8 %,
    // the others within 25 % as before.
    const double merge_env = getenv("SXG_POA_MERGE") ? atof(getenv("SXG_POA_MERGE")) : 0.0;
    // Round 14: neighbouring widths -- a geometry whose strip width IS the second width of a wider one's class at the same wave
    // count (the headline's W = 10 beside its W = 11) -- run as ONE launch wherever there is something to deal: in a round
    // whose packed launches together ask for at least one workgroup per CU.  Inside the wider class every alignment of the
    // joined blocks runs at their own width, so the reason to keep wide geometries apart (above) does not apply; one launch
    // is what the deal over CUs models ("workgroup k runs on CU k mod #CU": two launches side by side each pick their own
    // light CUs, and the hardware puts the second one's workgroups wherever there is room), one block queue has no launch
    // that drains before the other, and the priority board ranks all co-residents by one cost.  Below that size nothing
    // shares a CU and the launches stay apart.  SXG_POA_MERGE_WIDTH2=0: never (the plan of round 13), =1: at any size.
    // (measured: profiles/r15.)
    bool merge_w2 = width2_enabled();
    if (const char* e = getenv("SXG_POA_MERGE_WIDTH2")) merge_w2 = merge_w2 && atoi(e) != 0;
    else {
        size_t packed = 0;
        for (const auto& q : plans) if (q.variant.RM == 2) packed += q.work.size();
        merge_w2 = merge_w2 && packed >= (size_t)std::max(h->num_cu, 1);
    }
    for (size_t i = 0; i < plans.size(); ++i)
        for (size_t j = i + 1; j < plans.size();) {
            const LaunchPlan &a = plans[i], &b = plans[j];
            // (neighbouring widths: see merge_w2 above)
            const bool join_w2 = merge_w2 && a.variant.NW == b.variant.NW && b.variant.W == class_w2(CLASS_BLOCK, a.variant, a.sw);
            // (a launch in column tiles stays on its own: its arenas are laid out for its tile count at its geometry)
            if (a.tiles == 1 && b.tiles == 1 && same_kind(a.variant, b.variant) && a.variant.RM != 3 && a.cvx == b.cvx && a.sw == b.sw && a.tier == b.tier && a.wide_band == b.wide_band &&
                (join_w2 || (double)b.variant.Lpad() >= (merge_env > 0 ? merge_env : (a.variant.Lpad() >= 4096 ? 0.92 : 0.75)) * (double)a.variant.Lpad())) {
                plans[i].work.insert(plans[i].work.end(), b.work.begin(), b.work.end());
                plans.erase(plans.begin() + (long)j);
            } else ++j;
        }
}

static void spread_small_plans(sxg_poa_handle* h, std::vector<LaunchPlan>& plans) {
    // A batch that cannot fill the device with one workgroup per block (1000 blocks of 1 kbp are 1000 waves of 4096)
    // gives every block twice the waves at half the strip width: the same columns, shorter rows.
    if (!getenv("SXG_POA_NO_SPREAD")) {
        uint64_t waves = 0;
        for (auto& pl : plans) waves += (uint64_t)pl.work.size() * (uint64_t)pl.variant.NW;
        for (auto& pl : plans) {
            Variant& v = pl.variant;
            while (v.RM == 2 && v.NW <= 2 && v.W % 2 == 0 && v.W / 2 >= 4 && 2 * waves <= (uint64_t)h->num_cu * 16u) {
                waves += (uint64_t)pl.work.size() * (uint64_t)v.NW;
                v = Variant{v.W / 2, 2 * v.NW, class_tmax(v.W / 2, 2 * v.NW, 2, v.CB, true), 2, v.CB, v.DS};   // (NW 1 -> 2: the two-wave class; 2 -> 4: the four-wave class)
            }
        }
    }
}

static void price_plans(sxg_poa_handle* h, std::vector<LaunchPlan>& plans) {
    // A block's cost depends on the launch it ended up in (poa_cost.h: rows x swept columns -- a W = 10 block merged into the
    // W = 11 class runs every alignment at W2 = 10, one spread over twice the waves half the strip width), so it is priced
    // here, from the launch's variant as prepare_plan settled it, and the launch's blocks are sorted by THAT cost.
    h->blk_cost.assign((size_t)std::max(h->n_blocks, 1), 0);
    h->seq_done.assign((size_t)std::max<int64_t>(h->n_seqs, 1), 0);
    for (auto& pl : plans) {
        prepare_plan(h, pl, pl.tier);
        const Variant& v = pl.variant;
        for (int b : pl.work)
            h->blk_cost[(size_t)b] = block_cost(h->h_seq_off.data() + h->h_blk_off[b], h->h_blk_off[b + 1] - h->h_blk_off[b], v.RM, v.T(), v.W, v.W2,
                                                h->seq_done.data() + h->h_blk_off[b], pl.tiles);
        std::stable_sort(pl.work.begin(), pl.work.end(), [&](int a, int b) { return h->blk_cost[(size_t)a] > h->blk_cost[(size_t)b]; });
    }
}

static void drop_over_budget(sxg_poa_handle* h, std::vector<LaunchPlan>& plans, const uint64_t budget, std::vector<int32_t>& status,
                             std::vector<int32_t>& nomem_blocks) {
    // A geometry whose single arena does not fit the budget fails ITS blocks (per-block status, as the
    // ABI promises) and the rest of the batch goes on.
    for (size_t i = 0; i < plans.size();) {
        if ((uint64_t)plans[i].lay.total > budget && plans[i].wide_band) {
            // the every-strip plane (rows x columns dwords) is what does not fit: these blocks are not final -- their
            // status stays ST_BAND_MISS and the round's bookkeeping below sends them down the widening ladder
            // (packed -> 32-bit sweep, one byte per cell), which is where a band miss went before the wide plane existed
            for (int b : plans[i].work) { h->meta[b].wide_band = false; h->meta[b].no_wide = true; }
            plans.erase(plans.begin() + (long)i);
        } else if ((uint64_t)plans[i].lay.total > budget) {
            for (int b : plans[i].work) status[b] = plans[i].tier >= 2 ? ST_POOL_OVERFLOW : ST_ROWS_OVERFLOW;
            g_err = "memory budget too small for a block arena of " + std::to_string(plans[i].lay.total) + " bytes";
            nomem_blocks.insert(nomem_blocks.end(), plans[i].work.begin(), plans[i].work.end());
            plans.erase(plans.begin() + (long)i);
        } else ++i;
    }
}

static void size_slots(sxg_poa_handle* h, std::vector<LaunchPlan>& plans, const uint64_t budget) {
    // Slots per launch.  One geometry: as many as there are blocks / as fit.  Several geometries
    // running side by side should end together, so their WAVES are made proportional to their
    // work (cost model of SURVEY 8e): slots_p = lambda * cost_p / waves_per_slot_p, with the largest
    // lambda that respects the arena budget and the wave capacity of the device.
    // (the blocks' costs in THEIR launch, as priced above: a block swept by a wider geometry than its own -- merged launches --
    //  costs the columns of that geometry, and an alignment that a dual-width class sweeps at W2 costs W2's.  Until round 14
    //  a dual-width launch was priced at its full width, cost * Lpad / maxlen, and the headline's W = 11 launch, 80 % of whose
    //  sweeps run at W2 = 10, ended ~2 % before the W = 10 launch beside it.)
    std::vector<double> pcost(plans.size(), 0.0);
    for (size_t i = 0; i < plans.size(); ++i)
        for (int b : plans[i].work) pcost[i] += (double)std::max<uint64_t>(h->blk_cost[(size_t)b], 1);
    const int oversub = getenv("SXG_POA_OVERSUB") ? std::max(1, atoi(getenv("SXG_POA_OVERSUB"))) : 2;
    auto slots_at = [&](size_t i, double lambda) {
        const double s = lambda * pcost[i] / (double)plans[i].variant.NW;
        return (int64_t)std::min<double>((double)plans[i].want_slots, std::max(1.0, std::floor(s)));
    };
    auto fits = [&](double lambda) {
        uint64_t bytes = 0, waves = 0;
        for (size_t i = 0; i < plans.size(); ++i) {
            const int64_t n = slots_at(i, lambda);
            bytes += (uint64_t)n * plans[i].lay.total;
            waves += (uint64_t)n * (uint64_t)plans[i].variant.NW;
        }
        // Side by side the launches may ask for up to TWICE the wave slots of the device: workgroups that find no room wait
        // in their hardware queue and start -- pulling from their launch's block queue -- as soon as another launch
        // drains, so a launch the cost model under-estimated is not left alone on a half-empty chip at the end.
        return bytes <= budget && (plans.size() == 1 || waves <= (uint64_t)h->num_cu * 16u * (uint64_t)oversub);
    };
    double lam_lo = 0.0, lam_hi = 1.0;
    while (lam_hi < 1e30 && fits(lam_hi)) {
        bool all_full = true;
        for (size_t i = 0; i < plans.size(); ++i) all_full = all_full && slots_at(i, lam_hi) >= plans[i].want_slots;
        if (all_full) break;
        lam_hi *= 2.0;
    }
    if (!fits(lam_hi))
        for (int it = 0; it < 100; ++it) {
            const double mid = 0.5 * (lam_lo + lam_hi);
            if (fits(mid)) lam_lo = mid; else lam_hi = mid;
        }
    const double lambda = fits(lam_hi) ? lam_hi : lam_lo;
    for (size_t i = 0; i < plans.size(); ++i) plans[i].n_slots = slots_at(i, lambda);
}

// launches the round, waits for it, and collects its times and statistics
static int launch_round(sxg_poa_handle* h, std::vector<LaunchPlan>& plans, const int attempt, const bool dbg, float& ms_total) {
    while (h->planres.size() < plans.size()) {
        auto r = std::make_unique<PlanRes>();
        HIPCHK(r->stream.create(hipStreamNonBlocking));
        HIPCHK(r->e0.create());
        HIPCHK(r->e1.create());
        h->planres.push_back(std::move(r));
    }
    {
        const size_t board_bytes = (size_t)PRIO_BOARD_CUS * PRIO_BOARD_SLOTS * 4;
        int rcb = h->d_board.ensure(board_bytes);
        if (rcb) return rcb;
        HIPCHK(hipMemsetAsync(h->d_board.p, 0, board_bytes, h->stream));
        if ((rcb = h->d_est_done.ensure(8 * h->seq_done.size()))) return rcb;
        HIPCHK(hipMemcpyAsync(h->d_est_done.p, h->seq_done.data(), 8 * h->seq_done.size(), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    int prio_base = 0;
    for (size_t i = 0; i < plans.size(); ++i) {
        int rc = launch_plan(h, plans[i], *h->planres[i], prio_base);
        if (rc) return rc;
        prio_base += (int)((plans[i].n_slots + h->num_cu - 1) / std::max(h->num_cu, 1));
    }
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    // While the kernels run: pin the host buffer the step lists will be downloaded into (first call of a handle, or a
    // bigger batch than before; afterwards the pool already has it).  n_bases bounds the number of steps.
    if (attempt == 0 && h->want_block_graph && h->pins && h->n_bases >= ((int64_t)16 << 20) && !getenv("SXG_POA_NO_PINNED")) {
        if (h->pin_thread.joinable()) h->pin_thread.join();
        try {
            h->pin_thread = std::thread([pool = h->pins, dev = h->device, bytes = 4 * (size_t)h->n_bases] {
                if (hipSetDevice(dev) == hipSuccess) pool->prewarm(bytes);
            });
        } catch (...) {}   // (no thread: the download pins, or falls back to pageable memory, itself)
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    ms_total += ms;
    std::vector<unsigned long long> prof;   // the slot profiles of one launch
    for (size_t i = 0; i < plans.size(); ++i) {
        HIPCHK(hipEventElapsedTime(&plans[i].ms, h->planres[i]->e0, h->planres[i]->e1));
        if (int rcp = fetch_slot_prof(plans[i], *h->planres[i], prof)) return rcp;
        plans[i].clock_mhz = sample_clock(plans[i], prof);
        h->stats.dp_launches += 1;
        h->stats.n_slots += (int)plans[i].n_slots;
        h->stats.device_bytes += (uint64_t)plans[i].n_slots * plans[i].lay.total;
        width_stats_of(plans[i], prof, h->wstats, &h->tstats);
        if (plans[i].tiles > 1) {   // (a tiled launch counts its sweeps and their tiles in SP_TILES)
            h->tile_blocks += (int64_t)plans[i].work.size();
            for (int64_t sl = 0; sl < plans[i].n_slots; ++sl) {
                const unsigned long long w = prof[(size_t)sl * SLOT_PROF_WORDS + SP_TILES];
                h->tile_sweeps += (int64_t)(w & 0xffffffffull);
                h->tile_tiles += (int64_t)(w >> 32);
            }
            if (dbg) fprintf(stderr, "[sxg]   tiles: %d per row of the arena, %d columns each\n", plans[i].tiles, plans[i].variant.Lpad());
        }
        if (dbg) debug_plan(plans[i], prof, attempt);
    }
    return SXG_OK;
}

// the statuses of the blocks that ran, and from them the blocks of the next round: `pending`
static int advance_ladders(sxg_poa_handle* h, const std::vector<LaunchPlan>& plans, const int attempt, const bool dbg, std::vector<int32_t>& status,
                           std::vector<int32_t>& pending, const std::vector<int32_t>& nomem_blocks) {
    const int nb = h->n_blocks;
    {
        std::vector<int32_t> dev(std::max(nb, 1));
        HIPCHK(hipMemcpy(dev.data(), h->d_status.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        for (auto& pl : plans) for (int b : pl.work) status[b] = dev[b];   // only blocks that ran this round
    }
    std::vector<int32_t> again;
    if (dbg) {
        int cnt[16] = {0};
        for (int b : pending) cnt[status[b] & 15]++;
        fprintf(stderr, "[sxg] round %d: ok %d rows %d pool %d steps %d nodes %d long %d range %d band %d\n", attempt, cnt[0], cnt[1], cnt[2], cnt[3],
                cnt[4], cnt[5], cnt[6], cnt[7]);
    }
    for (int b : pending) {
        BlockMeta& m = h->meta[b];
        if (std::find(nomem_blocks.begin(), nomem_blocks.end(), b) != nomem_blocks.end()) continue;
        if (status[b] == ST_ROWS_OVERFLOW || status[b] == ST_POOL_OVERFLOW || status[b] == ST_TBX_OVERFLOW || status[b] == ST_NODES_OVERFLOW) {
            if (m.tier < 3) { m.tier += 1; again.push_back(b); }
        } else if (status[b] == ST_BAND_MISS && m.rm == 2 && !m.wide_band && !m.no_wide) {
            // The traceback kept leaving the ~1100 columns the plane holds around the backbone hints (a structural variant
            // that carries the alignment further off).  The same packed sweep is repeated with a plane that keeps EVERY
            // strip of every row -- rows x columns dwords, up to ~6 GB for a 26 kbp block, but it cannot miss, it covers
            // every length the packed sweep covers (the 32-bit sweeps end at SXG_POA_MAX_SEQ_LEN_WIDE) and it runs at the
            // packed sweep's speed.
            m.wide_band = true;
            again.push_back(b);
        } else if (status[b] == ST_RANGE_OVERFLOW || status[b] == ST_BAND_MISS) {
            // one step wider at the same capacity tier: packed -> int16 row words -> int32 row words
            if (m.rm != 1) {
                classify_block(m, m.rm >= 2 ? 0 : 1, false, h->long_blocks);
                if (m.fits) again.push_back(b);
                else status[b] = ST_TOO_LONG;    // (a score range beyond int16 on a sequence beyond SXG_POA_MAX_SEQ_LEN_WIDE)
            } else status[b] = ST_TOO_LONG;      // (unreachable: the int32 sweep reports neither)
        }
    }
    h->stats.retries += (int)again.size();
    pending.swap(again);
    return SXG_OK;
}

// cells and bytes of the blocks that succeeded, and the dominant launch, into h->stats
static int account_cells(sxg_poa_handle* h, std::vector<LaunchPlan>& all_plans, const std::vector<int32_t>& status) {
    const int nb = h->n_blocks;
    std::vector<unsigned long long> cells((size_t)std::max<int64_t>(h->n_seqs, 1));
    if (h->n_seqs) HIPCHK(hipMemcpy(cells.data(), h->d_cells.p, 8 * (size_t)h->n_seqs, hipMemcpyDeviceToHost));
    uint64_t total = 0, bytes = 0;
    std::vector<uint64_t> blk_cells(std::max(nb, 1), 0), blk_bytes(std::max(nb, 1), 0);
    for (int b = 0; b < nb; ++b) {
        if (status[b] != ST_OK) continue;
        uint64_t cb = 0;
        for (int s = h->h_blk_off[b]; s < h->h_blk_off[b + 1]; ++s) cb += cells[s];
        const BlockMeta& m = h->meta[b];
        const int ncross = m.S.convex ? 3 : (m.S.g == m.S.e ? 1 : 2);
        const int sz = m.rm == 1 ? 4 : 2;   // (banded: cells = band cells, as counted by the kernel)
        blk_cells[b] = cb; blk_bytes[b] = cb * (uint64_t)(2 * ncross * sz + 1);
        total += cb;
        bytes += blk_bytes[b];
    }
    // dominant launch = the one that evaluated the most cells
    for (auto& pl : all_plans) {
        for (int b : pl.work) if (status[b] == ST_OK) { pl.cells += blk_cells[b]; pl.bytes += blk_bytes[b]; }
        if (pl.cells >= h->stats.dom_cells) {
            h->stats.dom_cells = pl.cells; h->stats.dom_algo_bytes = pl.bytes; h->stats.dom_kernel_ms = pl.ms;
            h->stats.dom_threads = pl.variant.T(); h->stats.dom_cols_per_lane = pl.variant.W * (pl.variant.RM >= 2 ? 2 : 1);
            h->stats.dom_row_mode = pl.variant.RM;
            h->stats.dom_clock_mhz = pl.clock_mhz;
            // (dom_cols_per_lane stays the class's W: an upper bound of the columns a dual-width launch's alignments swept)
            h->wstats.dom_width = pl.variant.W; h->wstats.dom_width2 = pl.lay.W2;
        }
    }
    h->stats.cells = total;
    h->stats.algo_bytes = bytes;
    return SXG_OK;
}

extern "C" int sxg_poa_batch_execute(sxg_poa_handle* h) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (!h->have_batch) return fail(SXG_E_INVALID, "no batch uploaded");
    HIPCHK(hipSetDevice(h->device));
    const RoctxRange range_("sxg_poa_batch_execute");
    h->stats = sxg_poa_stats{};
    h->wstats = sxg_poa_width_stats{};
    h->tstats = sxg_poa_twin_stats{};
    h->tile_blocks = h->tile_sweeps = h->tile_tiles = 0;
    const bool dbg = getenv("SXG_POA_DEBUG") != nullptr;
    auto T0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        auto T1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[sxg] host %-18s %.3f ms\n", what, std::chrono::duration<double, std::milli>(T1 - T0).count());
        T0 = T1;
    };
    const int nb = h->n_blocks;
    std::vector<int32_t> status(std::max(nb, 1), 0);
    float ms_total = 0;
    // blocks whose longest sequence exceeds the largest variant fail up front
    std::vector<int32_t> pending;
    for (int b = 0; b < nb; ++b) {
        if (!h->meta[b].fits) status[b] = ST_TOO_LONG; else pending.push_back(b);
    }
    if (nb) HIPCHK(hipMemcpyAsync(h->d_status.p, status.data(), 4 * (size_t)nb, hipMemcpyHostToDevice, h->stream));
    if (nb) {
        HIPCHK(hipMemsetAsync(h->d_nn.p, 0, 4 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(h->d_ne.p, 0, 4 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(h->d_nc.p, 0, 4 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(h->d_blk_cycles.p, 0, 8 * (size_t)nb, h->stream));
    }
    lap("setup");
    std::vector<LaunchPlan> all_plans;
    std::vector<int32_t> nomem_blocks;  // failed for lack of arena memory: their status is final
    for (int b = 0; b < nb; ++b) h->meta[b].tier = 0;
    // Rounds.  A block comes back for two independent reasons, each with its own ladder: its arena was too
    // small (ROWS / POOL / TBX overflow: capacity tier 0..3, the last one is the worst case) or its sweep was
    // too narrow (RANGE overflow / BAND miss: packed -> int16 row words -> int32 row words, at the SAME
    // capacity tier; a band miss first repeats the packed sweep with a plane that keeps every strip).  3 + 3 steps at most, so 7
    // rounds always suffice; neither internal status is ever final.
    for (int attempt = 0; attempt < 7 && !pending.empty(); ++attempt) {
        std::vector<LaunchPlan> plans;
        group_pending(h, plans, pending);
        merge_plans(h, plans);
        spread_small_plans(h, plans);
        const uint64_t budget = arena_budget(h);
        price_plans(h, plans);
        drop_over_budget(h, plans, budget, status, nomem_blocks);
        size_slots(h, plans, budget);
        lap("plan");
        if (int rc = launch_round(h, plans, attempt, dbg, ms_total)) return rc;
        lap("launches");
        if (int rc = advance_ladders(h, plans, attempt, dbg, status, pending, nomem_blocks)) return rc;
        for (auto& pl : plans) all_plans.push_back(std::move(pl));
    }
    for (int b : pending) status[b] = ST_POOL_OVERFLOW;  // (unreachable: the ladders are shorter than the round limit)
    if (nb) HIPCHK(hipMemcpy(h->d_status.p, status.data(), 4 * (size_t)nb, hipMemcpyHostToDevice));
    lap("status");
    if (int rc = account_cells(h, all_plans, status)) return rc;
    lap("accounting");
    h->stats.kernel_ms = ms_total;
    h->executed = true;
    if (h->want_block_graph) {
        int rc = run_block_graphs(h, status);
        if (rc) return rc;
        lap("block graphs");
    }
    if (msa_trimmed(h->want_msa)) {
        int rc = run_msa_rows(h, status);
        if (rc) return rc;
        lap("MSA rows");
    }
    for (int b = 0; b < nb; ++b)
        if (status[b] != ST_OK) return fail(SXG_E_BLOCK, "block " + std::to_string(b) + " failed with status " + std::to_string(status[b]));
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
// Host result arrays: allocated without std::vector's serial zero-fill (the download overwrites every element), and
// from 8 MiB on 2 MiB-aligned and marked for transparent huge pages -- the headline batch downloads 1.7 GB, and the
// first-touch faults of 4 KiB pages under the copy (and their unmapping at _free) were a third of the
// provider's time outside the kernels.
static void* host_big_alloc(size_t bytes) {
    if (bytes < ((size_t)8 << 20)) return malloc(bytes ? bytes : 1);
    void* q = nullptr;
    if (posix_memalign(&q, (size_t)2 << 20, bytes)) return nullptr;
    madvise(q, bytes, MADV_HUGEPAGE);
    return q;
}
// What a result owns: its arrays (every one from host_big_alloc) and, when the step lists went into a borrowed pinned buffer,
// that buffer and the pool it goes back to.
struct OutOwner {
    std::shared_ptr<PinPool> pin_pool;
    void* pinned = nullptr;
    std::vector<void*> raw;
    ~OutOwner() { if (pinned && pin_pool) pin_pool->release(pinned); for (void* q : raw) free(q); }
    void* alloc(size_t bytes) {
        void* q = host_big_alloc(bytes);
        if (q) raw.push_back(q);
        return q;
    }
};

// Where the arrays of the result table (poa_results.h) live on the device after an execute, entry for entry beside
// sxg::RESULT_FAMILIES / RESULT_FLAT: the handle's buffer, the per-block offsets its entries start at there (SRC_DENSE: the
// buffer already is the dense array), and when the array is part of the result.
enum { SRC_DENSE, SRC_BASE /* the block's first base: the worst-case layout of the raw graphs */, SRC_NODE, SRC_EDGE /* bg_node_o, bg_edge_o */, SRC_N };
enum { WHEN_ALWAYS, WHEN_GRAPHS, WHEN_CONS, WHEN_GRAPHS_CONS, WHEN_PATHS, WHEN_BG, WHEN_BG_CONS, WHEN_MSA_ROWS, WHEN_MSA_ROWS_HOST /* the rows themselves: not when they stay resident */ };
struct DevSource { DevBuf sxg_poa_handle::*buf; int src, when; };
struct FamilySource { int when; DevSource pay[3]; };
static const FamilySource FAMILY_SRC[] = {
    /* node_off    */ {WHEN_ALWAYS, {{&sxg_poa_handle::d_node_code, SRC_BASE, WHEN_GRAPHS}, {&sxg_poa_handle::d_node_rank, SRC_BASE, WHEN_GRAPHS}, {&sxg_poa_handle::d_node_group, SRC_BASE, WHEN_GRAPHS}}},
    /* edge_off    */ {WHEN_ALWAYS, {{&sxg_poa_handle::d_edge_tail, SRC_BASE, WHEN_GRAPHS}, {&sxg_poa_handle::d_edge_head, SRC_BASE, WHEN_GRAPHS}, {&sxg_poa_handle::d_edge_w, SRC_BASE, WHEN_GRAPHS}}},
    /* cons_off    */ {WHEN_CONS, {{&sxg_poa_handle::d_cons, SRC_BASE, WHEN_GRAPHS_CONS}}},
    /* msa_off     */ {WHEN_MSA_ROWS, {{&sxg_poa_handle::d_msa, SRC_DENSE, WHEN_MSA_ROWS_HOST}}},   // (the trimmed MSA; the full one is formatted on the host)
    /* bg_node_off */ {WHEN_BG, {{&sxg_poa_handle::d_bg_len, SRC_NODE, WHEN_BG}, {&sxg_poa_handle::d_bg_od, SRC_NODE, WHEN_BG}, {&sxg_poa_handle::d_bg_id, SRC_NODE, WHEN_BG}}},
    /* bg_seq_off  */ {WHEN_BG, {{&sxg_poa_handle::d_bg_seq, SRC_NODE, WHEN_BG}}},
    /* bg_edge_off */ {WHEN_BG, {{&sxg_poa_handle::d_bg_eto, SRC_EDGE, WHEN_BG}}},
    /* bg_step_off */ {WHEN_BG, {{&sxg_poa_handle::d_bg_steps, SRC_BASE, WHEN_BG}}},
    /* bg_cons_off */ {WHEN_BG_CONS, {{&sxg_poa_handle::d_bg_cons, SRC_NODE, WHEN_BG_CONS}}},
};
static const DevSource FLAT_SRC[] = {
    {&sxg_poa_handle::d_status, SRC_DENSE, WHEN_ALWAYS}, {nullptr /* msa_cols_h, on the host */, SRC_DENSE, WHEN_MSA_ROWS}, {&sxg_poa_handle::d_blk_cycles, SRC_DENSE, WHEN_ALWAYS},
    {&sxg_poa_handle::d_score, SRC_DENSE, WHEN_ALWAYS}, {&sxg_poa_handle::d_cells, SRC_DENSE, WHEN_ALWAYS}, {&sxg_poa_handle::d_paths, SRC_DENSE, WHEN_PATHS},
};
static_assert(sizeof(FAMILY_SRC) / sizeof(FAMILY_SRC[0]) == sxg::N_RESULT_FAMILIES && sizeof(FLAT_SRC) / sizeof(FLAT_SRC[0]) == sxg::N_RESULT_FLAT,
              "one device source per entry of the result table");
static bool present(const sxg_poa_handle* h, int when) {
    const bool bg = h->want_block_graph && h->bg_done;
    const bool graphs = !(h->want_block_graph == 3 && h->bg_done);   // (3: the caller laces block graphs and reads nothing else)
    switch (when) {
    case WHEN_GRAPHS: return graphs;
    case WHEN_CONS: return h->want_consensus != 0;
    case WHEN_GRAPHS_CONS: return graphs && h->want_consensus;
    case WHEN_PATHS: return !(h->want_block_graph >= 2 && h->bg_done);
    case WHEN_BG: return bg;
    case WHEN_BG_CONS: return bg && h->want_consensus;
    case WHEN_MSA_ROWS: return msa_trimmed(h->want_msa);
    case WHEN_MSA_ROWS_HOST: return h->want_msa == SXG_MSA_TRIMMED;
    default: return true;
    }
}

// The dense layout of the executed batch: the offsets of every family the run produced (the others stay empty) and, per block,
// where its entries start in the device buffers.  From the per-block counts of the POA kernels and of the block-graph kernel.
struct DenseLayout {
    std::vector<int64_t> off[sxg::N_RESULT_FAMILIES];
    std::vector<int64_t> src[SRC_N];
    std::vector<int64_t> step_blocks;   // bg_step_off at every block's first sequence: what a gather of the step lists runs over
    int resident = SRC_DENSE;           // which of src[] the device copy of the source offsets (d_tmp_a) holds: none yet
    const std::vector<int64_t>& per_block(int a) const { return sxg::RESULT_FAMILIES[a].per_seq ? step_blocks : off[a]; }
};
static int dense_layout(sxg_poa_handle* h, DenseLayout& D) {
    const int nb = h->n_blocks;
    const int64_t ns = h->n_seqs;
    if (msa_trimmed(h->want_msa) && !h->msa_done) return fail(SXG_E_INVALID, "the trimmed MSA of this batch was not built");
    std::vector<int32_t> status(std::max(nb, 1)), nn(std::max(nb, 1)), ne(std::max(nb, 1)), nc(std::max(nb, 1));
    if (nb) {
        HIPCHK(hipMemcpy(status.data(), h->d_status.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nn.data(), h->d_nn.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ne.data(), h->d_ne.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(nc.data(), h->d_nc.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
    }
    for (int a = 0; a < sxg::N_RESULT_FAMILIES; ++a)
        if (present(h, FAMILY_SRC[a].when)) D.off[a].assign((size_t)(sxg::RESULT_FAMILIES[a].per_seq ? ns : (int64_t)nb) + 1, 0);
    for (auto& s : D.src) s.assign((size_t)nb + 1, 0);
    const bool cons = present(h, WHEN_CONS), bg = present(h, WHEN_BG);
    if (bg) {
        std::vector<int32_t> nsteps((size_t)std::max<int64_t>(ns, 1), 0);
        if (ns) HIPCHK(hipMemcpy(nsteps.data(), h->d_bg_nsteps.p, 4 * (size_t)ns, hipMemcpyDeviceToHost));
        for (int64_t sq = 0; sq < ns; ++sq) D.off[sxg::RF_BG_STEP][(size_t)sq + 1] = D.off[sxg::RF_BG_STEP][(size_t)sq] + nsteps[(size_t)sq];
        D.step_blocks.assign((size_t)nb + 1, 0);
    }
    for (int b = 0; b < nb; ++b) {
        D.off[sxg::RF_NODE][b + 1] = D.off[sxg::RF_NODE][b] + nn[b];
        D.off[sxg::RF_EDGE][b + 1] = D.off[sxg::RF_EDGE][b] + ne[b];
        if (cons) D.off[sxg::RF_CONS][b + 1] = D.off[sxg::RF_CONS][b] + nc[b];
        D.src[SRC_BASE][b] = h->h_seq_off[h->h_blk_off[b]];
        if (!bg) continue;
        const int32_t* c = h->bg_counts.data() + (size_t)BGC_N * b;
        const bool ok = status[b] == ST_OK;
        D.off[sxg::RF_BG_NODE][b + 1] = D.off[sxg::RF_BG_NODE][b] + (ok ? c[BGC_NODES] : 0);
        D.off[sxg::RF_BG_SEQ][b + 1] = D.off[sxg::RF_BG_SEQ][b] + (ok ? c[BGC_SEQ] : 0);
        D.off[sxg::RF_BG_EDGE][b + 1] = D.off[sxg::RF_BG_EDGE][b] + (ok ? c[BGC_EDGES] : 0);
        if (cons) D.off[sxg::RF_BG_CONS][b + 1] = D.off[sxg::RF_BG_CONS][b] + (ok ? c[BGC_CONS] : 0);
        D.step_blocks[b + 1] = D.off[sxg::RF_BG_STEP][(size_t)h->h_blk_off[b + 1]];
        D.src[SRC_NODE][b] = h->bg_node_o[(size_t)b]; D.src[SRC_EDGE][b] = h->bg_edge_o[(size_t)b];
    }
    if (present(h, WHEN_MSA_ROWS)) {
        if (h->msa_off_h.size() != (size_t)nb + 1) return fail(SXG_E_INVALID, "the trimmed MSA's offsets do not match the batch");
        D.off[sxg::RF_MSA] = h->msa_off_h;
    }
    int rc;   // (the two offset vectors of a gather)
    if ((rc = h->d_tmp_a.ensure(8 * (size_t)(nb + 1))) || (rc = h->d_tmp_b.ensure(8 * (size_t)(nb + 1)))) return rc;
    return SXG_OK;
}

// One gather launch on the handle's stream (not waited for), for a payload of family a whose entries start at D.src[kind] in
// src: dst[dst_off[b] ..) = src[src_off[b] ..) for every block, `elem` bytes per entry, dst_off[b + 1] - dst_off[b] entries.
// Both ranges are checked against the buffers first: a mistake in the tables above comes back as a return code, not as a
// fault of the device.  The source offsets are uploaded when they change, the destination offsets every time.
static int gather(sxg_poa_handle* h, DenseLayout& D, int kind, int a, const DevBuf& src, size_t elem, void* dst, size_t dst_bytes) {
    const int nb = h->n_blocks;
    const std::vector<int64_t>&src_off = D.src[kind], &dst_off = D.per_block(a);
    if (src_off.size() != (size_t)nb + 1 || dst_off.size() != (size_t)nb + 1 || (elem != 1 && elem != 4) || !dst || !src.p || dst_off[0] != 0 ||
        (uint64_t)dst_off[nb] > dst_bytes / elem)
        return fail(SXG_E_INVALID, "gather: the dense array does not fit its buffer");
    for (int b = 0; b < nb; ++b) {
        const int64_t cnt = dst_off[b + 1] - dst_off[b];
        if (cnt < 0 || (cnt > 0 && (src_off[b] < 0 || (uint64_t)(src_off[b] + cnt) > src.cap / elem)))
            return fail(SXG_E_INVALID, "gather: block " + std::to_string(b) + " reads outside its device buffer");
    }
    if (nb == 0 || dst_off[nb] == 0) return SXG_OK;
    if (D.resident != kind) HIPCHK(hipMemcpy(h->d_tmp_a.p, src_off.data(), 8 * (size_t)(nb + 1), hipMemcpyHostToDevice));
    D.resident = kind;
    HIPCHK(hipMemcpy(h->d_tmp_b.p, dst_off.data(), 8 * (size_t)(nb + 1), hipMemcpyHostToDevice));
    const dim3 grid((unsigned)std::min(nb, 4096)), block(256);
    if (elem == 1)
        hipLaunchKernelGGL((gather_kernel<uint8_t>), grid, block, 0, h->stream, src.as<uint8_t>(), (uint8_t*)dst, h->d_tmp_a.as<int64_t>(), h->d_tmp_b.as<int64_t>(), nb);
    else
        hipLaunchKernelGGL((gather_kernel<uint32_t>), grid, block, 0, h->stream, src.as<uint32_t>(), (uint32_t*)dst, h->d_tmp_a.as<int64_t>(), h->d_tmp_b.as<int64_t>(), nb);
    HIPCHK(hipGetLastError());
    return SXG_OK;
}

extern "C" int sxg_poa_batch_download(sxg_poa_handle* h, sxg_poa_batch_out* out) {
    if (!h || !out) return fail(SXG_E_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    if (!h->have_batch || !h->executed) return fail(SXG_E_INVALID, "no executed batch to download");
    HIPCHK(hipSetDevice(h->device));
    const RoctxRange range_("sxg_poa_batch_download");
    HostLaps laps;
    const int nb = h->n_blocks;
    OutOwner* o = new OutOwner();
    out->_owner = o;
    out->n_blocks = nb; out->n_seqs = h->n_seqs;
    OutGuard<sxg_poa_batch_out, sxg_poa_batch_free> guard(out);   // (every return below but the last frees the result)
    auto hip = [&](hipError_t e, const char* what) { return e == hipSuccess ? SXG_OK : fail(SXG_E_NODEVICE, std::string(what) + ": " + hipGetErrorString(e)); };
    DenseLayout D;
    int rc = dense_layout(h, D);
    if (rc) return rc;
    for (int a = 0; a < sxg::N_RESULT_FAMILIES; ++a) {
        const sxg::ResultFamily& A = sxg::RESULT_FAMILIES[a];
        if (a == sxg::RF_MSA) laps.lap("download: POA graphs");
        if (a == sxg::RF_BG_NODE) laps.lap("download: MSA rows");
        if (!present(h, FAMILY_SRC[a].when)) continue;
        int64_t* off = (int64_t*)o->alloc(8 * D.off[a].size());
        if (!off) return fail(SXG_E_NOMEM, "host allocation of the result failed");
        memcpy(off, D.off[a].data(), 8 * D.off[a].size());
        sxg::set_field(*out, A.off_field, off);
        const size_t total = (size_t)D.off[a].back();
        for (int p = 0; p < 3; ++p) {
            const DevSource& S = FAMILY_SRC[a].pay[p];
            const size_t elem = A.pay[p].elem;
            if (!elem || !present(h, S.when)) continue;
            void* dst = nullptr;
            if (A.pay[p].field == offsetof(sxg_poa_batch_out, bg_steps)) {   // the step lists: into a borrowed pinned buffer when the pool has one (see PinPool)
                if (h->pin_thread.joinable()) h->pin_thread.join();
                if (total >= ((size_t)16 << 20) && h->pins && !getenv("SXG_POA_NO_PINNED") && (dst = h->pins->acquire(elem * total))) { o->pin_pool = h->pins; o->pinned = dst; }
            }
            if (!dst && !(dst = o->alloc(elem * total))) return fail(SXG_E_NOMEM, "host allocation of the result failed");
            sxg::set_field(*out, A.pay[p].field, dst);
            if (!total) continue;
            const DevBuf& src = h->*S.buf;
            if (S.src == SRC_DENSE) {   // (the rows of the trimmed MSA, as the device wrote them)
                if ((rc = hip(hipMemcpy(dst, src.p, elem * total, hipMemcpyDeviceToHost), "download of the MSA rows"))) return rc;
                continue;
            }
            if ((rc = h->d_tmp_c.ensure(elem * total)) || (rc = gather(h, D, S.src, a, src, elem, h->d_tmp_c.p, h->d_tmp_c.cap)) ||
                (rc = hip(hipMemcpyAsync(dst, h->d_tmp_c.p, elem * total, hipMemcpyDeviceToHost, h->stream), "download of a gathered array")) ||
                (rc = hip(hipStreamSynchronize(h->stream), "download of a gathered array")))
                return rc;
        }
    }
    laps.lap("download: block graphs");
    for (int f = 0; f < sxg::N_RESULT_FLAT; ++f) {
        const sxg::ResultFlat& F = sxg::RESULT_FLAT[f];
        if (!present(h, FLAT_SRC[f].when)) continue;
        const size_t bytes = F.elem * (size_t)(F.index == 0 ? nb : F.index == 1 ? h->n_seqs : h->n_bases);
        void* dst = o->alloc(bytes);   // (seq_path_nodes, one node id per base, is the big one: 1.3 GB on the headline batch, one straight copy)
        if (!dst) return fail(SXG_E_NOMEM, "host allocation of the result failed");
        sxg::set_field(*out, F.field, dst);
        if (!bytes) continue;
        if (!FLAT_SRC[f].buf) memcpy(dst, h->msa_cols_h.data(), std::min(bytes, 4 * h->msa_cols_h.size()));
        else if ((rc = hip(hipMemcpy(dst, (h->*FLAT_SRC[f].buf).p, bytes, hipMemcpyDeviceToHost), "download of a flat array"))) return rc;
    }
    laps.lap("download: paths");   // (and the small per-block and per-sequence arrays)
    if (h->want_msa && !msa_trimmed(h->want_msa) && out->seq_path_nodes) {
        const sxg::BatchShape S{nb, h->h_blk_off.data(), h->h_seq_off.data()};
        if (!sxg::format_full_msa(S, h->want_consensus != 0, [o](size_t bytes) { return o->alloc(bytes); }, out))
            return fail(SXG_E_NOMEM, "host allocation of the MSA failed");
        laps.lap("download: full MSA");
    }
    guard.dismiss();
    return SXG_OK;
}

extern "C" int sxg_poa_batch_device_view(sxg_poa_handle* h, sxg_poa_device_view* v) {
    if (!h || !v) return fail(SXG_E_INVALID, "NULL argument");
    memset(v, 0, sizeof(*v));
    if (!h->have_batch || !h->executed) return fail(SXG_E_INVALID, "no executed batch");
    v->n_blocks = h->n_blocks; v->n_seqs = h->n_seqs; v->n_bases = h->n_bases;
    v->status = h->d_status.as<int32_t>(); v->n_nodes = h->d_nn.as<int32_t>(); v->n_edges = h->d_ne.as<int32_t>();
    v->node_code = h->d_node_code.as<uint8_t>(); v->node_rank = h->d_node_rank.as<int32_t>();
    v->node_group = h->d_node_group.as<int32_t>(); v->edge_tail = h->d_edge_tail.as<int32_t>();
    v->edge_head = h->d_edge_head.as<int32_t>(); v->edge_weight = h->d_edge_w.as<uint32_t>();
    v->seq_path_nodes = h->d_paths.as<int32_t>(); v->score = h->d_score.as<int32_t>();
    return SXG_OK;
}

extern "C" void sxg_poa_batch_free(sxg_poa_batch_out* out) {
    if (!out) return;
    delete (OutOwner*)out->_owner;
    memset(out, 0, sizeof(*out));
}

extern "C" int sxg_poa_batch_run(sxg_poa_handle* h, const sxg_poa_batch_in* in, sxg_poa_batch_out* out) {
    if (out) memset(out, 0, sizeof(*out));
    int rc = sxg_poa_batch_upload(h, in);
    if (rc) return rc;
    rc = sxg_poa_batch_execute(h);
    if (rc && rc != SXG_E_BLOCK) return rc;
    const std::string keep = g_err;
    int rc2 = sxg_poa_batch_download(h, out);
    if (rc2) return rc2;
    if (rc) g_err = keep;
    return rc;
}

// ---------------------------------------------------------------------------------------
// Multi-GPU: blocks are independent (src/smooth.cpp:1931), so every rank aligns its own share and the only
// exchange is the reassembly of the per-block results on the rank that laces (src/main.cpp:599+).
// sxg_poa_batch_run_sharded is sxg_poa_batch_run for a communicator: EVERY rank calls it with the SAME batch,
// the blocks are dealt by cost (longest processing time first), each rank runs its share, packs its
// dense results into one device blob, the blob sizes are all-gathered and the blobs travel to the root with ONE
// grouped ncclSend/ncclRecv per peer of exactly that size -- device to device over xGMI, no padding to the
// largest rank, buffers kept by the handle.  The root assembles the results in the ORIGINAL block order.
// RCCL is OPTIONAL at load time: a single-GPU user of libsxgpoa.so needs no librccl.so.  The entry points are resolved
// with dlopen/dlsym the first time a communicator is asked for (in a process that already loaded RCCL -- PyTorch-ROCm --
// the SONAME resolves to that very instance).
namespace {
struct RcclApi {
    decltype(&::ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&::ncclCommInitRank) CommInitRank = nullptr;
    decltype(&::ncclCommDestroy) CommDestroy = nullptr;
    decltype(&::ncclCommAbort) CommAbort = nullptr;
    decltype(&::ncclCommGetAsyncError) CommGetAsyncError = nullptr;
    decltype(&::ncclAllGather) AllGather = nullptr;
    decltype(&::ncclGroupStart) GroupStart = nullptr;
    decltype(&::ncclGroupEnd) GroupEnd = nullptr;
    decltype(&::ncclSend) Send = nullptr;
    decltype(&::ncclRecv) Recv = nullptr;
    decltype(&::ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
    std::string why;
};
RcclApi& rccl_api() {
    static RcclApi A = [] {
        RcclApi a;
        void* lib = nullptr;
        // SXG_POA_RCCL_LIB names the library instead of the default search (tests point it at a file that does not exist to
        // take the RCCL-missing path: SXG_E_NODEVICE with a message, not a crash)
        if (const char* forced = getenv("SXG_POA_RCCL_LIB")) lib = dlopen(forced, RTLD_NOW | RTLD_GLOBAL);
        else
            for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
                if ((lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
        if (!lib) {   // (dlerror() clears the error it returns: ask once)
            const char* e = dlerror();
            a.why = std::string("librccl.so not found (") + (e ? e : "dlopen failed") + ")";
            return a;
        }
        bool all = true;
#define SXG_RCCL_SYM(f) do { a.f = (decltype(a.f))dlsym(lib, "nccl" #f); if (!a.f) { all = false; a.why += " nccl" #f; } } while (0)
        SXG_RCCL_SYM(GetUniqueId); SXG_RCCL_SYM(CommInitRank); SXG_RCCL_SYM(CommDestroy); SXG_RCCL_SYM(CommAbort);
        SXG_RCCL_SYM(CommGetAsyncError); SXG_RCCL_SYM(AllGather); SXG_RCCL_SYM(GroupStart); SXG_RCCL_SYM(GroupEnd);
        SXG_RCCL_SYM(Send); SXG_RCCL_SYM(Recv); SXG_RCCL_SYM(GetErrorString);
#undef SXG_RCCL_SYM
        a.ok = all;
        if (!all) a.why = "librccl.so lacks" + a.why;
        return a;
    }();
    return A;
}
}  // namespace
#define RCCL_NEEDED() do { if (!rccl_api().ok) return fail(SXG_E_NODEVICE, "multi-GPU needs RCCL: " + rccl_api().why); } while (0)
#define ncclGetUniqueId rccl_api().GetUniqueId
#define ncclCommInitRank rccl_api().CommInitRank
#define ncclCommDestroy rccl_api().CommDestroy
#define ncclCommAbort rccl_api().CommAbort
#define ncclCommGetAsyncError rccl_api().CommGetAsyncError
#define ncclAllGather rccl_api().AllGather
#define ncclGroupStart rccl_api().GroupStart
#define ncclGroupEnd rccl_api().GroupEnd
#define ncclSend rccl_api().Send
#define ncclRecv rccl_api().Recv
#define ncclGetErrorString rccl_api().GetErrorString

#define NCCLCHK(x)                                                                                      \
    do {                                                                                               \
        ncclResult_t _r = (x);                                                                         \
        if (_r != ncclSuccess) return fail(SXG_E_NODEVICE, std::string(#x) + ": " + ncclGetErrorString(_r)); \
    } while (0)

constexpr int BC_N_WORDS = 16;   // words per rank in the count exchange (BC_N below)
extern "C" int sxg_poa_comm_unique_id(uint8_t* id) {
    if (!id) return fail(SXG_E_INVALID, "NULL argument");
    static_assert(sizeof(ncclUniqueId) == SXG_POA_COMM_ID_BYTES, "ncclUniqueId size");
    RCCL_NEEDED();
    ncclUniqueId u;
    NCCLCHK(ncclGetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return SXG_OK;
}
extern "C" void sxg_poa_comm_destroy(sxg_poa_handle* h) {
    if (!h) return;
    if (h->comm && h->own_comm) (void)ncclCommDestroy(h->comm);
    h->comm = nullptr; h->own_comm = false; h->nranks = 1; h->rank = 0;
}
extern "C" int sxg_poa_comm_init(sxg_poa_handle* h, const uint8_t* id, int nranks, int rank) {
    if (!h || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(SXG_E_INVALID, "bad argument");
    RCCL_NEEDED();
    HIPCHK(hipSetDevice(h->device));
    sxg_poa_comm_destroy(h);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    NCCLCHK(ncclCommInitRank(&h->comm, nranks, u, rank));
    h->own_comm = true; h->nranks = nranks; h->rank = rank;
    // (the exchange buffer of the sharded run's counts: allocated here so that the run itself cannot fail before its collectives)
    return h->d_counts.ensure(8 * (size_t)BC_N_WORDS * (size_t)(nranks + 1));
}
extern "C" int sxg_poa_comm_attach(sxg_poa_handle* h, void* nccl_comm, int nranks, int rank) {
    if (!h || !nccl_comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(SXG_E_INVALID, "bad argument");
    RCCL_NEEDED();
    sxg_poa_comm_destroy(h);
    h->comm = (ncclComm_t)nccl_comm; h->own_comm = false; h->nranks = nranks; h->rank = rank;
    HIPCHK(hipSetDevice(h->device));
    return h->d_counts.ensure(8 * (size_t)BC_N_WORDS * (size_t)(nranks + 1));
}

namespace {
// blocks by descending cost (ties: lower id) onto the least-loaded rank (ties: lower rank)
void lpt_partition(const sxg_poa_batch_in* in, int nranks, std::vector<std::vector<int32_t>>& parts) {
    const int nb = in->n_blocks;
    std::vector<double> cost(std::max(nb, 1), 0.0);
    for (int b = 0; b < nb; ++b) {
        double prev = 0;
        const double l1 = in->blk_off[b + 1] > in->blk_off[b] ? (double)(in->seq_off[in->blk_off[b] + 1] - in->seq_off[in->blk_off[b]]) : 0.0;
        for (int sq = in->blk_off[b]; sq < in->blk_off[b + 1]; ++sq) {
            const double len = (double)(in->seq_off[sq + 1] - in->seq_off[sq]);
            if (sq > in->blk_off[b]) cost[b] += len * (l1 + 0.05 * prev);
            prev += len;
        }
    }
    std::vector<int32_t> order(nb);
    for (int b = 0; b < nb; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return cost[a] > cost[c]; });
    parts.assign(nranks, {});
    std::vector<double> load(nranks, 0.0);
    for (int b : order) {
        int r = 0;
        for (int k = 1; k < nranks; ++k) if (load[k] < load[r]) r = k;
        parts[r].push_back(b);
        load[r] += cost[b];
    }
    for (auto& pt : parts) std::sort(pt.begin(), pt.end());
}
struct LocalBatch {
    std::vector<int32_t> blk_off{0};
    std::vector<int64_t> seq_off{0};
    std::vector<uint8_t> bases;
    std::vector<uint32_t> weights;
    std::vector<sxg_poa_params> params;
    std::vector<int32_t> trims;
    sxg_poa_batch_in in;
};
void build_local(const sxg_poa_batch_in* in, const std::vector<int32_t>& part, LocalBatch& L) {
    for (int b : part) {
        for (int sq = in->blk_off[b]; sq < in->blk_off[b + 1]; ++sq) {
            L.bases.insert(L.bases.end(), in->bases + in->seq_off[sq], in->bases + in->seq_off[sq + 1]);
            L.seq_off.push_back((int64_t)L.bases.size());
            L.weights.push_back(in->weights ? in->weights[sq] : 1u);
        }
        L.blk_off.push_back((int32_t)(L.seq_off.size() - 1));
        if (in->per_block_params) L.params.push_back(in->params[b]);
    }
    if (!in->per_block_params) L.params.push_back(in->params[0]);
    if (L.bases.empty()) L.bases.push_back(0);
    if (L.weights.empty()) L.weights.push_back(1);
    memset(&L.in, 0, sizeof(L.in));
    L.in.n_blocks = (int32_t)part.size(); L.in.blk_off = L.blk_off.data(); L.in.seq_off = L.seq_off.data();
    L.in.bases = L.bases.data(); L.in.weights = L.weights.data(); L.in.params = L.params.data();
    L.in.per_block_params = in->per_block_params; L.in.want_consensus = in->want_consensus; L.in.want_msa = 0;
    // the owning rank builds the block graphs of its blocks (the root only laces); the MSA is formatted on the root from
    // the per-base paths, which then travel as well
    L.in.want_block_graph = in->want_block_graph >= 2 ? (in->want_msa ? 1 : 2) : in->want_block_graph;   // (3: the raw POA graphs travel with the blob; the root drops them)
    L.in.bg_consensus_visited_only = in->bg_consensus_visited_only;
    if (in->want_block_graph) {
        for (int b : part) L.trims.push_back(in->bg_trim ? in->bg_trim[b] : 0);
        if (L.trims.empty()) L.trims.push_back(0);
        L.in.bg_trim = L.trims.data();
    }
}
// The blob of one rank is its result, serialised in the order of the result table: for every array the rank's run produced
// (bit of BC_PRESENT: 4 * family + 0 for the offsets, + 1 .. 3 for the payloads; 4 * families + f for flat array f) one
// 16-byte-aligned section.  The count words travel ahead of it (the size all-gather) and say everything the root needs to find
// the sections: blob_views, the one function both ends use.
enum { BC_NB = 0, BC_NS, BC_NBASES, BC_NODES, BC_EDGES, BC_CONS, BC_BYTES, BC_PAD /* error code of the rank (0 = fine) */,
       // block graphs of the rank's blocks (want_block_graph): the owning rank builds them, the root only laces
       BC_BG /* 0 = none, 1 = with, 2 = instead of the per-base paths */, BC_BG_NODES, BC_BG_EDGES, BC_BG_SEQ, BC_BG_STEPS, BC_BG_CONS,
       BC_MSA /* 0: the sharded entries refuse the trimmed MSA */, BC_PRESENT, BC_N };
static_assert(BC_N == BC_N_WORDS, "count words");
const int FAMILY_TOTAL[] = {BC_NODES, BC_EDGES, BC_CONS, BC_MSA, BC_BG_NODES, BC_BG_SEQ, BC_BG_EDGES, BC_BG_STEPS, BC_BG_CONS};   // (the total of every family, by sxg::RF_*)
static_assert(sizeof(FAMILY_TOTAL) / sizeof(FAMILY_TOTAL[0]) == sxg::N_RESULT_FAMILIES, "one total per family");
constexpr int family_bit(int a, int slot) { return 4 * a + slot; }
constexpr int flat_bit(int f) { return 4 * sxg::N_RESULT_FAMILIES + f; }
// the sections of the blob that the counts c describe, as the arrays of *v (when given) at base; returns the blob's size
size_t blob_views(const int64_t* c, uint8_t* base, sxg_poa_batch_out* v) {
    size_t cur = 0;
    auto sec = [&](int bit, size_t field, size_t bytes) {
        if (!((c[BC_PRESENT] >> bit) & 1)) return;
        if (v) sxg::set_field(*v, field, base + cur);
        cur += (bytes + 15) & ~(size_t)15;
    };
    const size_t n[3] = {(size_t)c[BC_NB], (size_t)c[BC_NS], (size_t)c[BC_NBASES]};
    for (int a = 0; a < sxg::N_RESULT_FAMILIES; ++a) {
        const sxg::ResultFamily& A = sxg::RESULT_FAMILIES[a];
        sec(family_bit(a, 0), A.off_field, 8 * (n[A.per_seq ? 1 : 0] + 1));
        for (int p = 0; p < 3; ++p)
            if (A.pay[p].elem) sec(family_bit(a, p + 1), A.pay[p].field, A.pay[p].elem * (size_t)c[FAMILY_TOTAL[a]]);
    }
    for (int f = 0; f < sxg::N_RESULT_FLAT; ++f) sec(flat_bit(f), sxg::RESULT_FLAT[f].field, sxg::RESULT_FLAT[f].elem * n[sxg::RESULT_FLAT[f].index]);
    return cur;
}
// dense results of the handle's executed batch, packed into h->d_blob on the device
int pack_blob(sxg_poa_handle* h, int64_t* counts) {
    DenseLayout D;
    int rc = dense_layout(h, D);
    if (rc) return rc;
    memset(counts, 0, sizeof(int64_t) * BC_N);
    counts[BC_NB] = h->n_blocks; counts[BC_NS] = h->n_seqs; counts[BC_NBASES] = h->n_bases;
    counts[BC_BG] = present(h, WHEN_BG) ? h->want_block_graph : 0;
    // what travels: everything the run produced but the two arrays the root does not reassemble (the trimmed MSA, block_cycles)
    for (int a = 0; a < sxg::N_RESULT_FAMILIES; ++a) {
        if (a == sxg::RF_MSA || !present(h, FAMILY_SRC[a].when)) continue;
        counts[BC_PRESENT] |= (int64_t)1 << family_bit(a, 0);
        counts[FAMILY_TOTAL[a]] = D.off[a].back();
        for (int p = 0; p < 3; ++p)
            if (sxg::RESULT_FAMILIES[a].pay[p].elem && present(h, FAMILY_SRC[a].pay[p].when)) counts[BC_PRESENT] |= (int64_t)1 << family_bit(a, p + 1);
    }
    for (int f = 0; f < sxg::N_RESULT_FLAT; ++f)
        if (FLAT_SRC[f].buf && sxg::RESULT_FLAT[f].field != offsetof(sxg_poa_batch_out, block_cycles) && present(h, FLAT_SRC[f].when))
            counts[BC_PRESENT] |= (int64_t)1 << flat_bit(f);
    const size_t total = blob_views(counts, nullptr, nullptr);
    counts[BC_BYTES] = (int64_t)total;
    if ((rc = h->d_blob.ensure(total + 16))) return rc;
    sxg_poa_batch_out v;
    memset(&v, 0, sizeof(v));
    blob_views(counts, h->d_blob.as<uint8_t>(), &v);
    for (int a = 0; a < sxg::N_RESULT_FAMILIES; ++a) {
        const sxg::ResultFamily& A = sxg::RESULT_FAMILIES[a];
        if (void* off = sxg::get_field(v, A.off_field)) HIPCHK(hipMemcpy(off, D.off[a].data(), 8 * D.off[a].size(), hipMemcpyHostToDevice));
        for (int p = 0; p < 3; ++p) {
            void* dst = A.pay[p].elem ? sxg::get_field(v, A.pay[p].field) : nullptr;
            const size_t bytes = A.pay[p].elem * (size_t)counts[FAMILY_TOTAL[a]];
            if (!dst || !bytes) continue;
            const DevSource& S = FAMILY_SRC[a].pay[p];
            if (S.src == SRC_DENSE) { HIPCHK(hipMemcpyAsync(dst, (h->*S.buf).p, bytes, hipMemcpyDeviceToDevice, h->stream)); continue; }
            if ((rc = gather(h, D, S.src, a, h->*S.buf, A.pay[p].elem, dst, bytes))) return rc;
            HIPCHK(hipStreamSynchronize(h->stream));   // (the offset vectors on the device are reused by the next array)
        }
    }
    for (int f = 0; f < sxg::N_RESULT_FLAT; ++f) {
        void* dst = sxg::get_field(v, sxg::RESULT_FLAT[f].field);
        const size_t bytes = sxg::RESULT_FLAT[f].elem * (size_t)counts[sxg::RESULT_FLAT[f].index == 0 ? BC_NB : sxg::RESULT_FLAT[f].index == 1 ? BC_NS : BC_NBASES];
        if (dst && bytes) HIPCHK(hipMemcpyAsync(dst, (h->*FLAT_SRC[f].buf).p, bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return SXG_OK;
}
// root: results of all ranks (host copies of their blobs) -> one result set in the batch's block order
int assemble(const sxg_poa_batch_in* in, const std::vector<std::vector<int32_t>>& parts, const std::vector<std::vector<uint8_t>>& blobs,
             const std::vector<int64_t>& counts, sxg_poa_batch_out* out) {
    OutOwner* o = new OutOwner();
    out->_owner = o;
    std::vector<sxg_poa_batch_out> views(parts.size());
    for (size_t r = 0; r < parts.size(); ++r) {
        memset(&views[r], 0, sizeof(views[r]));
        const int64_t* c = counts.data() + r * BC_N;
        if (c[BC_NB] != (int64_t)parts[r].size() || (size_t)c[BC_BYTES] > blobs[r].size() || blob_views(c, nullptr, nullptr) != (size_t)c[BC_BYTES])
            return fail(SXG_E_INVALID, "rank " + std::to_string(r) + " sent a blob that does not match the deal");
        blob_views(counts.data() + r * BC_N, const_cast<uint8_t*>(blobs[r].data()), &views[r]);
    }
    const sxg::BatchShape S{in->n_blocks, in->blk_off, in->seq_off};
    auto alloc = [o](size_t bytes) { return o->alloc(bytes); };
    if (!sxg::reassemble_results(S, parts, views, alloc, out)) return fail(SXG_E_NOMEM, "host allocation of the reassembled result failed");
    if (in->want_msa && out->seq_path_nodes && !sxg::format_full_msa(S, in->want_consensus != 0, alloc, out))
        return fail(SXG_E_NOMEM, "host allocation of the MSA failed");
    for (int b = 0; b < in->n_blocks; ++b)
        if (out->status[b] != ST_OK) return fail(SXG_E_BLOCK, "block " + std::to_string(b) + " failed with status " + std::to_string(out->status[b]));
    return SXG_OK;
}
int run_shard(sxg_poa_handle* h, const sxg_poa_batch_in* in, const std::vector<int32_t>& part, int64_t* counts) {
    LocalBatch L;
    build_local(in, part, L);
    int rc = sxg_poa_batch_upload(h, &L.in);
    if (rc) return rc;
    rc = sxg_poa_batch_execute(h);
    if (rc && rc != SXG_E_BLOCK) return rc;   // (per-block failures travel in the status array)
    return pack_blob(h, counts);
}
}  // namespace

// Waiting for a collective with a deadline: a peer that died (or never called) would otherwise park this rank in
// hipStreamSynchronize for ever.  The stream is polled; after SXG_POA_COMM_TIMEOUT_S seconds (default 600) or on an
// asynchronous RCCL error the communicator is aborted and the call returns SXG_E_NODEVICE.
static void comm_abort(sxg_poa_handle* h) {
    if (h->comm && h->own_comm) (void)ncclCommAbort(h->comm);   // (an attached communicator stays the caller's to abort)
    h->comm = nullptr; h->own_comm = false; h->nranks = 1; h->rank = 0;
}
static int comm_wait(sxg_poa_handle* h, const char* what) {
    static const double limit = [] { const char* e = getenv("SXG_POA_COMM_TIMEOUT_S"); const double v = e ? atof(e) : 0.0; return v > 0 ? v : 600.0; }();
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; ++spin) {
        const hipError_t q = hipStreamQuery(h->stream);
        if (q == hipSuccess) return SXG_OK;
        if (q != hipErrorNotReady) { comm_abort(h); return fail(SXG_E_NODEVICE, std::string(what) + ": " + hipGetErrorString(q)); }
        ncclResult_t ar = ncclSuccess;
        if (h->comm && (spin & 255) == 255 && (ncclCommGetAsyncError(h->comm, &ar) != ncclSuccess || (ar != ncclSuccess && ar != ncclInProgress))) {
            comm_abort(h);
            return fail(SXG_E_NODEVICE, std::string(what) + ": RCCL reported " + ncclGetErrorString(ar));
        }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
            comm_abort(h);
            return fail(SXG_E_NODEVICE, std::string(what) + ": no completion after " + std::to_string((int)limit) + " s (a peer rank failed or never called); communicator aborted");
        }
        if (spin > 1000) std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

static int check_batch(const sxg_poa_batch_in* in) {
    if (in->want_msa == SXG_MSA_TRIMMED || in->want_msa == SXG_MSA_TRIMMED_RESIDENT) return fail(SXG_E_INVALID, "the trimmed MSA (want_msa = SXG_MSA_TRIMMED) is not reassembled across ranks: use sxg_poa_batch_run");
    if (in->n_blocks < 0 || (in->n_blocks > 0 && (!in->blk_off || !in->seq_off || !in->params || !in->bases))) return fail(SXG_E_INVALID, "batch_in has NULL arrays");
    return SXG_OK;
}

// The sharded run in three stages, like upload / execute / download of the single-GPU call:
//   sxg_poa_batch_upload_sharded   deals the blocks of the SAME batch on every rank (LPT) and uploads this rank's share;
//   sxg_poa_batch_execute_sharded  aligns the uploaded share (whatever uploaded it: the deal above, or a plain
//                                  sxg_poa_batch_upload of a share the caller cut himself), packs the results into one
//                                  device blob and brings every blob to rank 0 -- the collective part;
//   sxg_poa_batch_download_sharded rank 0: results of all ranks in the batch's block order; others: SXG_NOT_ROOT.
extern "C" int sxg_poa_batch_upload_sharded(sxg_poa_handle* h, const sxg_poa_batch_in* in) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    int rc = check_batch(in);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    const int nranks = h->comm ? h->nranks : 1, rank = h->comm ? h->rank : 0;
    lpt_partition(in, nranks, h->sh_parts);
    h->sh_dealt = false; h->sh_exchanged = false;
    LocalBatch L;
    build_local(in, h->sh_parts[rank], L);
    if ((rc = sxg_poa_batch_upload(h, &L.in))) return rc;
    h->sh_dealt = true;
    return SXG_OK;
}

extern "C" int sxg_poa_batch_execute_sharded(sxg_poa_handle* h) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    HIPCHK(hipSetDevice(h->device));
    const int nranks = h->comm ? h->nranks : 1, rank = h->comm ? h->rank : 0;
    h->sh_exchanged = false; h->sh_bytes_received = 0; h->sh_ranks_seen = 0;
    std::vector<int64_t>& counts = h->sh_counts;
    counts.assign((size_t)nranks * BC_N, 0);
    int64_t* mine = counts.data() + (size_t)rank * BC_N;
    int rc = h->have_batch ? sxg_poa_batch_execute(h) : fail(SXG_E_INVALID, "no batch uploaded");
    const auto t_pack = std::chrono::steady_clock::now();
    { const RoctxRange range_("sxg_poa sharded: pack"); if (!rc || rc == SXG_E_BLOCK) rc = pack_blob(h, mine); }   // (per-block failures travel in the status array)
    const auto t_xch = std::chrono::steady_clock::now();
    h->sh_pack_ms = std::chrono::duration<double, std::milli>(t_xch - t_pack).count();
    h->sh_exchange_ms = 0;
    if (!h->comm) {
        if (rc) return rc;
        h->sh_at.assign(2, 0); h->sh_exchanged = true; h->sh_ranks_seen = 1;
        return SXG_OK;
    }
    {   // (a communicator of ONE rank takes the same way: the collectives run, nothing is sent)
        const RoctxRange range_("sxg_poa sharded: exchange");
        // A rank-local failure (allocation, HIP error) must not leave the peers blocked in a collective: the failing rank
        // still takes part in the size exchange, with its error code in BC_PAD and nothing to send, and EVERY rank then
        // returns that failure -- the ranks fail together.  (d_counts is allocated by sxg_poa_comm_init / _attach.)
        std::string local_err = rc ? std::string(sxg_poa_last_error()) : std::string();
        if (rc) { memset(mine, 0, sizeof(int64_t) * BC_N); mine[BC_PAD] = rc; }
        int64_t* dc = h->d_counts.as<int64_t>();
        if (!dc) return fail(SXG_E_INVALID, "sharded run without sxg_poa_comm_init / sxg_poa_comm_attach");
        auto gathered_failure = [&](const char* what) -> int {
            for (int r = 0; r < nranks; ++r)
                if (counts[(size_t)r * BC_N + BC_PAD]) {
                    const int code = (int)counts[(size_t)r * BC_N + BC_PAD];
                    return fail(code, std::string("sharded run: rank ") + std::to_string(r) + " failed " + what + " (code " + std::to_string(code) + ")" +
                                      (r == rank && !local_err.empty() ? ": " + local_err : std::string()));
                }
            return SXG_OK;
        };
        // sizes first (RCCL has no all-gather-v) ...
        std::vector<int64_t> my_counts(mine, mine + BC_N);
        HIPCHK(hipMemcpyAsync(dc + (size_t)nranks * BC_N, my_counts.data(), 8 * BC_N, hipMemcpyHostToDevice, h->stream));
        NCCLCHK(ncclAllGather(dc + (size_t)nranks * BC_N, dc, BC_N, ncclInt64, h->comm, h->stream));
        HIPCHK(hipMemcpyAsync(counts.data(), dc, 8 * (size_t)BC_N * nranks, hipMemcpyDeviceToHost, h->stream));
        if ((rc = comm_wait(h, "size all-gather"))) return rc;
        if ((rc = gathered_failure("while aligning its share"))) return rc;
        // ... the root makes room (the one step after the size exchange that can fail on one rank only: its outcome is
        // all-gathered too, one word per rank, before anybody posts a send) ...
        std::vector<size_t>& at = h->sh_at;
        at.assign(nranks + 1, 0);
        for (int r = 1; r < nranks; ++r) at[r + 1] = at[r] + (((size_t)counts[(size_t)r * BC_N + BC_BYTES] + 255) & ~(size_t)255);
        int64_t ready = 0;
        if (rank == 0 && (rc = h->d_recv.ensure(at[nranks] + 256))) { ready = rc; local_err = sxg_poa_last_error(); }
        std::vector<int64_t> readies((size_t)nranks, 0);
        HIPCHK(hipMemcpyAsync(dc + (size_t)nranks * BC_N, &ready, 8, hipMemcpyHostToDevice, h->stream));
        NCCLCHK(ncclAllGather(dc + (size_t)nranks * BC_N, dc, 1, ncclInt64, h->comm, h->stream));
        HIPCHK(hipMemcpyAsync(readies.data(), dc, 8 * (size_t)nranks, hipMemcpyDeviceToHost, h->stream));
        if ((rc = comm_wait(h, "receive-buffer all-gather"))) return rc;
        for (int r = 0; r < nranks; ++r) counts[(size_t)r * BC_N + BC_PAD] = readies[r];
        if ((rc = gathered_failure("to allocate the receive buffer"))) return rc;
        // ... then every blob straight to the root, exact sizes, one group: the seven peers use their own xGMI links.
        // ncclGroupStart is ALWAYS paired with ncclGroupEnd: an error inside the group is reported after the group is closed.
        ncclResult_t gr = ncclGroupStart(), g2;
        if (gr == ncclSuccess) {
            if (rank == 0) {
                for (int r = 1; r < nranks && gr == ncclSuccess; ++r)
                    if (counts[(size_t)r * BC_N + BC_BYTES] > 0)
                        gr = ncclRecv(h->d_recv.as<uint8_t>() + at[r], (size_t)counts[(size_t)r * BC_N + BC_BYTES], ncclUint8, r, h->comm, h->stream);
            } else if (mine[BC_BYTES] > 0)
                gr = ncclSend(h->d_blob.p, (size_t)mine[BC_BYTES], ncclUint8, 0, h->comm, h->stream);
            g2 = ncclGroupEnd();
            if (gr == ncclSuccess) gr = g2;
        }
        if (gr != ncclSuccess) { comm_abort(h); return fail(SXG_E_NODEVICE, std::string("blob exchange: ") + ncclGetErrorString(gr)); }
        if ((rc = comm_wait(h, "blob exchange"))) return rc;
        for (int r = 0; r < nranks; ++r) {
            h->sh_ranks_seen += 1;   // (every rank's counts arrived; a rank with an empty share sends nothing)
            if (r != 0 && rank == 0) h->sh_bytes_received += (uint64_t)counts[(size_t)r * BC_N + BC_BYTES];
        }
    }
    h->sh_exchange_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_xch).count();
    h->sh_exchanged = true;
    return SXG_OK;
}

extern "C" int sxg_poa_sharded_timing(sxg_poa_handle* h, double* pack_ms, double* exchange_ms) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (pack_ms) *pack_ms = h->sh_pack_ms;
    if (exchange_ms) *exchange_ms = h->sh_exchange_ms;
    return SXG_OK;
}

extern "C" int sxg_poa_batch_download_sharded(sxg_poa_handle* h, const sxg_poa_batch_in* in, sxg_poa_batch_out* out) {
    if (!h || !in || !out) return fail(SXG_E_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    if (!h->sh_exchanged) return fail(SXG_E_INVALID, "no sharded batch executed");
    if (!h->sh_dealt) return fail(SXG_E_INVALID, "the batch was not dealt by sxg_poa_batch_upload_sharded: the root cannot know its block order");
    HIPCHK(hipSetDevice(h->device));
    const int nranks = h->comm ? h->nranks : 1, rank = h->comm ? h->rank : 0;
    if (rank != 0) return SXG_NOT_ROOT;
    if ((int)h->sh_parts.size() != nranks) return fail(SXG_E_INVALID, "communicator changed since the upload");
    std::vector<std::vector<uint8_t>> blobs(nranks);
    for (int r = 0; r < nranks; ++r) {
        const size_t bytes = (size_t)h->sh_counts[(size_t)r * BC_N + BC_BYTES];
        blobs[r].resize(std::max<size_t>(bytes, 16));
        if (bytes) HIPCHK(hipMemcpy(blobs[r].data(), r == 0 ? h->d_blob.p : (void*)(h->d_recv.as<uint8_t>() + h->sh_at[r]), bytes, hipMemcpyDeviceToHost));
    }
    int rc = assemble(in, h->sh_parts, blobs, h->sh_counts, out);
    if (rc && rc != SXG_E_BLOCK) sxg_poa_batch_free(out);
    return rc;
}

extern "C" int sxg_poa_sharded_info(sxg_poa_handle* h, int32_t* ranks_seen, uint64_t* bytes_received) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (ranks_seen) *ranks_seen = h->sh_ranks_seen;
    if (bytes_received) *bytes_received = h->sh_bytes_received;
    return SXG_OK;
}

extern "C" int sxg_poa_batch_run_sharded(sxg_poa_handle* h, const sxg_poa_batch_in* in, sxg_poa_batch_out* out) {
    if (!h || !in || !out) return fail(SXG_E_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    if (int crc = check_batch(in)) return crc;   // (the same answer on every rank, before the collective)
    // (an upload that fails on one rank only -- a host or device allocation -- must still reach the collective: the
    //  execute stage then reports "no batch" as this rank's error and all ranks fail together)
    const int urc = sxg_poa_batch_upload_sharded(h, in);
    const std::string uerr = urc ? std::string(sxg_poa_last_error()) : std::string();
    if (urc && !(h->comm && h->nranks > 1)) return urc;
    if (urc) h->have_batch = false;
    int rc = sxg_poa_batch_execute_sharded(h);
    if (rc) return urc ? fail(urc, uerr) : rc;
    return sxg_poa_batch_download_sharded(h, in, out);
}

// TEST ENTRY: the sharded run with `nranks` SIMULATED ranks on this one GPU -- every shard is aligned here, one after
// the other, and its blob is put where RCCL would have delivered it.  Exercises the partition, the blob packing
// and the root's assembly with more than one rank on a box that has one GPU; only ncclSend/ncclRecv are not taken.
extern "C" int sxg_poa_batch_run_sharded_local(sxg_poa_handle* h, const sxg_poa_batch_in* in, int nranks, sxg_poa_batch_out* out) {
    if (!h || !in || !out || nranks < 1) return fail(SXG_E_INVALID, "bad argument");
    memset(out, 0, sizeof(*out));
    int rc = check_batch(in);
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    std::vector<std::vector<int32_t>> parts;
    lpt_partition(in, nranks, parts);
    std::vector<int64_t> counts((size_t)nranks * BC_N, 0);
    std::vector<std::vector<uint8_t>> blobs(nranks);
    for (int r = 0; r < nranks; ++r) {
        if ((rc = run_shard(h, in, parts[r], counts.data() + (size_t)r * BC_N))) return rc;
        const size_t bytes = (size_t)counts[(size_t)r * BC_N + BC_BYTES];
        blobs[r].resize(std::max<size_t>(bytes, 16));
        if (bytes) HIPCHK(hipMemcpy(blobs[r].data(), h->d_blob.p, bytes, hipMemcpyDeviceToHost));
    }
    rc = assemble(in, parts, blobs, counts, out);
    if (rc && rc != SXG_E_BLOCK) sxg_poa_batch_free(out);
    return rc;
}

// ---------------------------------------------------------------------------------------
// Device group: one process, several GPUs (include/sxg_poa.h).  A group owns one engine handle per entry
// of its device list; a batch is dealt over the members in contiguous slices of equal cost (poa_deal.h), every member runs
// the single-handle upload / execute / download on its slice from a host thread of its own -- on its own device, streams and
// arenas, at the same time as the others --, and the results, being slices of the batch's dense arrays, are put back with one
// copy per array and member (sxg::reassemble_results of poa_results.h, over the table of the result arrays).  No communicator,
// no rank, no collective, and no blob: what a member downloads IS its part of the result (trimmed MSA rows, block graphs and
// block cycles included), only the offsets are rebased.
struct sxg_poa_group {
    std::vector<sxg_poa_handle*> members;
    // the uploaded batch: its shape, its deal (member m runs blocks cut[m] .. cut[m + 1] - 1, listed in parts[m]), who has work
    bool have_batch = false, executed = false;
    int n_blocks = 0;
    int64_t n_seqs = 0;
    std::vector<int32_t> cut, blk_off;
    std::vector<int64_t> seq_off;
    std::vector<std::vector<int32_t>> parts;
    std::vector<char> active;
    // last execute + download: wall milliseconds per member, the longest download, the reassembly on the host
    std::vector<double> exec_ms, down_ms;
    double assemble_ms = 0;
};

namespace {
bool group_serial() {
    const char* e = getenv("SXG_POA_GROUP_SERIAL");
    return e && atoi(e) != 0;
}
// fn(m) for every member with work, one host thread per member (SXG_POA_GROUP_SERIAL=1: one after the other on the calling
// thread); every thread is joined before this returns.  A member that failed as a whole (anything but SXG_E_BLOCK) makes the
// call return its code, with the member and the text of ITS thread's error in the caller's sxg_poa_last_error(); otherwise
// SXG_E_BLOCK if some member reported failed blocks, else SXG_OK.
template <class F>
int group_for_each(sxg_poa_group* g, const char* what, F fn) {
    const int n = (int)g->members.size();
    std::vector<int> rc((size_t)n, SXG_OK);
    std::vector<std::string> err((size_t)n);
    auto body = [&](int m) {
        const hipError_t e = hipSetDevice(g->members[(size_t)m]->device);
        if (e != hipSuccess) { rc[(size_t)m] = SXG_E_NODEVICE; err[(size_t)m] = std::string("hipSetDevice: ") + hipGetErrorString(e); return; }
        rc[(size_t)m] = fn(m);
        if (rc[(size_t)m]) err[(size_t)m] = g_err;   // (the error text is per thread: carried over to the caller's below)
    };
    std::vector<std::thread> threads;
    const bool serial = group_serial();
    for (int m = 0; m < n; ++m) {
        if (!g->active[(size_t)m]) continue;
        bool started = false;
        if (!serial) {
            try { threads.emplace_back(body, m); started = true; } catch (...) { started = false; }   // (no thread to be had: run it here)
        }
        if (!started) body(m);
    }
    for (auto& t : threads) t.join();
    for (int m = 0; m < n; ++m)
        if (rc[(size_t)m] && rc[(size_t)m] != SXG_E_BLOCK)
            return fail(rc[(size_t)m], std::string("group member ") + std::to_string(m) + " (device " + std::to_string(g->members[(size_t)m]->device) + ") failed in " +
                                           what + ": " + err[(size_t)m]);
    for (int m = 0; m < n; ++m)
        if (rc[(size_t)m]) return fail(SXG_E_BLOCK, std::string("group member ") + std::to_string(m) + ": " + err[(size_t)m]);
    return SXG_OK;
}
double ms_since(const std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
}  // namespace

extern "C" int sxg_poa_group_create(const int32_t* devices, int32_t n, sxg_poa_group** out) {
    if (!out) return fail(SXG_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!devices || n < 1 || n > 16) return fail(SXG_E_INVALID, "a group has 1 to 16 members");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SXG_E_NODEVICE, "no HIP device available");
    for (int i = 0; i < n; ++i)
        if (devices[i] < 0 || devices[i] >= ndev) return fail(SXG_E_INVALID, "group member " + std::to_string(i) + ": device index out of range");
    sxg_poa_group* g = new sxg_poa_group();
    for (int i = 0; i < n; ++i) {
        sxg_poa_handle* h = nullptr;
        const int rc = sxg_poa_create(devices[i], &h);
        if (rc) {
            const std::string keep = g_err;
            sxg_poa_group_destroy(g);
            return fail(rc, "group member " + std::to_string(i) + ": " + keep);
        }
        g->members.push_back(h);
    }
    // members that share a device share its memory: each takes 1/k of what one handle would take by default
    for (sxg_poa_handle* h : g->members) {
        int k = 0;
        for (sxg_poa_handle* o : g->members) k += o->device == h->device;
        h->budget_share = k;
    }
    g->active.assign((size_t)n, 0);
    g->exec_ms.assign((size_t)n, 0.0); g->down_ms.assign((size_t)n, 0.0);
    *out = g;
    return SXG_OK;
}

extern "C" void sxg_poa_group_destroy(sxg_poa_group* g) {
    if (!g) return;
    for (sxg_poa_handle* h : g->members) sxg_poa_destroy(h);
    delete g;
}

extern "C" int sxg_poa_group_size(const sxg_poa_group* g) { return g ? (int)g->members.size() : 0; }

extern "C" sxg_poa_handle* sxg_poa_group_member(sxg_poa_group* g, int32_t i) {
    return g && i >= 0 && i < (int32_t)g->members.size() ? g->members[(size_t)i] : nullptr;
}

extern "C" int sxg_poa_group_set_memory_budget(sxg_poa_group* g, uint64_t bytes_per_member) {
    if (!g) return fail(SXG_E_INVALID, "group is NULL");
    for (sxg_poa_handle* h : g->members) h->mem_budget = bytes_per_member;
    return SXG_OK;
}

extern "C" int sxg_poa_group_set_long_blocks(sxg_poa_group* g, int on) {
    if (!g) return fail(SXG_E_INVALID, "group is NULL");
    for (sxg_poa_handle* h : g->members) h->long_blocks = on != 0;
    return SXG_OK;
}

extern "C" int sxg_poa_group_batch_upload(sxg_poa_group* g, const sxg_poa_batch_in* in) {
    if (!g || !in) return fail(SXG_E_INVALID, "NULL argument");
    g->have_batch = false; g->executed = false;
    if (in->want_msa == SXG_MSA_TRIMMED_RESIDENT) return fail(SXG_E_INVALID, "resident MSA rows (want_msa = SXG_MSA_TRIMMED_RESIDENT) would lie on several members of a group: use one handle");
    const int nb = in->n_blocks, n = (int)g->members.size();
    if (nb < 0 || (nb > 0 && (!in->blk_off || !in->seq_off || !in->params))) return fail(SXG_E_INVALID, "batch_in has NULL arrays");
    // (what the deal reads is checked here; everything else by every member's own upload)
    if (nb > 0 && in->blk_off[0] != 0) return fail(SXG_E_INVALID, "blk_off[0] must be 0");
    for (int b = 0; b < nb; ++b)
        if (in->blk_off[b + 1] < in->blk_off[b]) return fail(SXG_E_INVALID, "blk_off not monotone");
    const int64_t ns = nb ? in->blk_off[nb] : 0;
    if (ns > 0 && in->seq_off[0] != 0) return fail(SXG_E_INVALID, "seq_off[0] must be 0");
    for (int64_t s = 0; s < ns; ++s)
        if (in->seq_off[s + 1] < in->seq_off[s]) return fail(SXG_E_INVALID, "seq_off not monotone");
    if (ns > 0 && in->seq_off[ns] > 0 && !in->bases) return fail(SXG_E_INVALID, "bases is NULL");
    sxg::deal_batch(nb, in->blk_off, in->seq_off, n, g->cut);
    g->n_blocks = nb; g->n_seqs = ns;
    g->blk_off.assign(in->blk_off, in->blk_off + (nb ? nb + 1 : 0)); g->seq_off.assign(in->seq_off, in->seq_off + (nb ? ns + 1 : 0));
    g->parts.assign((size_t)n, {});
    struct Slice { std::vector<int32_t> blk_off; std::vector<int64_t> seq_off; sxg_poa_batch_in in; };
    std::vector<Slice> slices((size_t)n);
    for (int m = 0; m < n; ++m) {
        const int b0 = g->cut[(size_t)m], b1 = g->cut[(size_t)m + 1];
        const int32_t s0 = nb ? in->blk_off[b0] : 0, s1 = nb ? in->blk_off[b1] : 0;
        const int64_t x0 = ns ? in->seq_off[s0] : 0;
        for (int b = b0; b < b1; ++b) g->parts[(size_t)m].push_back(b);
        g->active[(size_t)m] = b1 > b0 || (nb == 0 && m == 0);   // (a batch without blocks is member 0's: it answers as one handle does)
        if (!g->active[(size_t)m]) continue;
        Slice& S = slices[(size_t)m];
        S.in = *in;
        if (nb == 0) continue;
        S.blk_off.resize((size_t)(b1 - b0) + 1); S.seq_off.resize((size_t)(s1 - s0) + 1);
        for (int k = 0; k <= b1 - b0; ++k) S.blk_off[(size_t)k] = in->blk_off[b0 + k] - s0;
        for (int k = 0; k <= s1 - s0; ++k) S.seq_off[(size_t)k] = in->seq_off[s0 + k] - x0;
        // the slice reads the caller's letters, weights, params and trims in place: only the offsets are rebased
        S.in.n_blocks = b1 - b0; S.in.blk_off = S.blk_off.data(); S.in.seq_off = S.seq_off.data();
        S.in.bases = in->bases ? in->bases + x0 : nullptr;
        S.in.weights = in->weights ? in->weights + s0 : nullptr;
        S.in.params = in->per_block_params ? in->params + b0 : in->params;
        S.in.bg_trim = in->bg_trim ? in->bg_trim + b0 : nullptr;
    }
    const int rc = group_for_each(g, "upload", [&](int m) { return sxg_poa_batch_upload(g->members[(size_t)m], &slices[(size_t)m].in); });
    if (rc) return rc;
    g->have_batch = true;
    return SXG_OK;
}

extern "C" int sxg_poa_group_batch_execute(sxg_poa_group* g) {
    if (!g) return fail(SXG_E_INVALID, "group is NULL");
    if (!g->have_batch) return fail(SXG_E_INVALID, "no batch uploaded");
    g->executed = false;
    std::fill(g->exec_ms.begin(), g->exec_ms.end(), 0.0);
    std::fill(g->down_ms.begin(), g->down_ms.end(), 0.0);
    g->assemble_ms = 0;
    const int rc = group_for_each(g, "execute", [&](int m) {
        const auto t0 = std::chrono::steady_clock::now();
        const int r = sxg_poa_batch_execute(g->members[(size_t)m]);
        g->exec_ms[(size_t)m] = ms_since(t0);
        return r;
    });
    if (rc && rc != SXG_E_BLOCK) return rc;
    g->executed = true;
    if (rc) {   // the first failed block, by its number in the batch (as sxg_poa_batch_execute names it)
        for (int m = 0; m < (int)g->members.size(); ++m) {
            if (!g->active[(size_t)m]) continue;
            const sxg_poa_handle* h = g->members[(size_t)m];
            std::vector<int32_t> st((size_t)std::max(h->n_blocks, 1), 0);
            if (h->n_blocks && (hipSetDevice(h->device) != hipSuccess ||
                                hipMemcpy(st.data(), h->d_status.p, 4 * (size_t)h->n_blocks, hipMemcpyDeviceToHost) != hipSuccess))
                return fail(SXG_E_NODEVICE, "group member " + std::to_string(m) + ": reading the block status failed");
            for (int k = 0; k < h->n_blocks; ++k)
                if (st[(size_t)k] != ST_OK)
                    return fail(SXG_E_BLOCK, "block " + std::to_string(g->cut[(size_t)m] + k) + " failed with status " + std::to_string(st[(size_t)k]));
        }
    }
    return rc;
}

extern "C" int sxg_poa_group_batch_download(sxg_poa_group* g, sxg_poa_batch_out* out) {
    if (!g || !out) return fail(SXG_E_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    if (!g->have_batch || !g->executed) return fail(SXG_E_INVALID, "no executed batch to download");
    const int n = (int)g->members.size();
    std::vector<sxg_poa_batch_out> outs((size_t)n);
    for (auto& o : outs) memset(&o, 0, sizeof(o));
    auto drop = [&] { for (auto& o : outs) sxg_poa_batch_free(&o); };
    int rc = group_for_each(g, "download", [&](int m) {
        const auto t0 = std::chrono::steady_clock::now();
        const int r = sxg_poa_batch_download(g->members[(size_t)m], &outs[(size_t)m]);
        g->down_ms[(size_t)m] = ms_since(t0);
        return r;
    });
    if (rc) { const std::string keep = g_err; drop(); return fail(rc, keep); }
    const auto t_asm = std::chrono::steady_clock::now();
    int first = -1, n_active = 0;
    for (int m = 0; m < n; ++m)
        if (g->active[(size_t)m]) { if (first < 0) first = m; ++n_active; }
    if (n_active == 1) {
        *out = outs[(size_t)first];   // one slice is the whole batch: the member's result is the group's
        memset(&outs[(size_t)first], 0, sizeof(sxg_poa_batch_out));
    } else {
        // Several slices: the batch's offsets and room for every array first, then every member's arrays into their places,
        // one thread per member.
        OutOwner* o = new OutOwner();
        out->_owner = o;
        const sxg::BatchShape S{g->n_blocks, g->blk_off.data(), g->seq_off.data()};
        if (!sxg::reassemble_layout(S, g->parts, outs, [o](size_t bytes) { return o->alloc(bytes); }, out)) {
            drop(); sxg_poa_batch_free(out);
            return fail(SXG_E_NOMEM, "host allocation of the group's result failed");
        }
        rc = group_for_each(g, "reassembly", [&](int m) { sxg::reassemble_part(S, g->parts[(size_t)m], outs[(size_t)m], out); return SXG_OK; });
        if (rc) { const std::string keep = g_err; drop(); sxg_poa_batch_free(out); return fail(rc, keep); }
    }
    drop();
    g->assemble_ms = ms_since(t_asm);
    return SXG_OK;
}

extern "C" int sxg_poa_group_batch_run(sxg_poa_group* g, const sxg_poa_batch_in* in, sxg_poa_batch_out* out) {
    if (out) memset(out, 0, sizeof(*out));
    if (!out) return fail(SXG_E_INVALID, "NULL argument");
    int rc = sxg_poa_group_batch_upload(g, in);
    if (rc) return rc;
    rc = sxg_poa_group_batch_execute(g);
    if (rc && rc != SXG_E_BLOCK) return rc;
    const std::string keep = g_err;
    const int rc2 = sxg_poa_group_batch_download(g, out);
    if (rc2) return rc2;
    if (rc) g_err = keep;
    return rc;
}

extern "C" int sxg_poa_group_timing(sxg_poa_group* g, double* member_ms, double* pack_ms, double* assemble_ms) {
    if (!g) return fail(SXG_E_INVALID, "group is NULL");
    double longest = 0;
    for (size_t m = 0; m < g->members.size(); ++m) {
        if (member_ms) member_ms[m] = g->exec_ms[m] + g->down_ms[m];
        longest = std::max(longest, g->down_ms[m]);
    }
    if (pack_ms) *pack_ms = longest;
    if (assemble_ms) *assemble_ms = g->assemble_ms;
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
struct AlignOwner {
    std::vector<int32_t> status, score, pair_row, pair_pos;
    std::vector<int64_t> pair_off;
};

extern "C" void sxg_poa_align_free(sxg_poa_align_out* out) {
    if (!out) return;
    delete (AlignOwner*)out->_owner;
    memset(out, 0, sizeof(*out));
}

extern "C" int sxg_poa_align_batch(sxg_poa_handle* h, const sxg_poa_align_in* in, sxg_poa_align_out* out) {
    if (!h || !in || !out) return fail(SXG_E_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    const int n = in->n;
    if (n < 0 || (n > 0 && (!in->row_off || !in->pred_off || !in->seq_off || !in->params)))
        return fail(SXG_E_INVALID, "align_in has NULL arrays");
    HIPCHK(hipSetDevice(h->device));
    h->have_batch = false; h->executed = false;
    if (n > 0 && (in->row_off[0] != 0 || in->seq_off[0] != 0)) return fail(SXG_E_INVALID, "row_off[0] and seq_off[0] must be 0");
    const int64_t rows = n ? in->row_off[n] : 0, nbases = n ? in->seq_off[n] : 0;
    if (rows < 0 || nbases < 0) return fail(SXG_E_INVALID, "negative totals");
    if (rows > 0 && (!in->row_code || !in->row_sink)) return fail(SXG_E_INVALID, "row_code / row_sink is NULL");
    if (nbases > 0 && !in->bases) return fail(SXG_E_INVALID, "bases is NULL");
    if (rows > 0 && in->pred_off[0] != 0) return fail(SXG_E_INVALID, "pred_off[0] must be 0");
    for (int64_t r = 0; r < rows; ++r)
        if (in->pred_off[r + 1] < in->pred_off[r]) return fail(SXG_E_INVALID, "pred_off not monotone");
    const int64_t ne = rows ? in->pred_off[rows] : 0;
    if (ne > 0 && !in->preds) return fail(SXG_E_INVALID, "preds is NULL");
    // validate topology: every predecessor is an earlier row of the same problem
    for (int p = 0; p < n; ++p) {
        const int64_t r0 = in->row_off[p], r1 = in->row_off[p + 1];
        if (r1 < r0 || in->seq_off[p + 1] < in->seq_off[p]) return fail(SXG_E_INVALID, "offsets not monotone");
        if (r1 - r0 >= (1 << 20)) return fail(SXG_E_INVALID, "graph too large");
        for (int64_t r = r0; r < r1; ++r)
            for (int64_t k = in->pred_off[r]; k < in->pred_off[r + 1]; ++k)
                if (in->preds[k] < 1 || in->preds[k] > r - r0) return fail(SXG_E_INVALID, "predecessor rows must precede their successor");
    }
    AlignOwner* o = new AlignOwner();
    out->_owner = o; out->n = n;
    o->status.assign(std::max(n, 1), 0); o->score.assign(std::max(n, 1), 0); o->pair_off.assign(n + 1, 0);
    OutGuard<sxg_poa_align_out, sxg_poa_align_free> guard(out);   // (every return below but those after dismiss() frees the result)
    DevBuf d_row_off, d_code, d_sink, d_pred_off, d_preds, d_seq_off, d_bases, d_params, d_status, d_score, d_np, d_pr, d_pp, d_work,
        d_queue, d_arena;
    int rc;
    const int np = in->per_problem_params ? n : 1;
    std::vector<uint8_t> stage((size_t)std::max<int64_t>(nbases, 1));
    for (int64_t i = 0; i < nbases; ++i) stage[i] = in->bases[i] > 4 ? 4 : in->bases[i];
    std::vector<uint8_t> codes((size_t)std::max<int64_t>(rows, 1));
    for (int64_t i = 0; i < rows; ++i) codes[i] = in->row_code[i] > 4 ? 4 : in->row_code[i];
    const size_t outcap = (size_t)(rows + nbases + 1);
    if ((rc = d_row_off.ensure(8 * (size_t)(n + 1))) || (rc = d_code.ensure((size_t)rows + 16)) || (rc = d_sink.ensure((size_t)rows + 16)) ||
        (rc = d_pred_off.ensure(8 * (size_t)(rows + 1))) || (rc = d_preds.ensure(4 * (size_t)(ne + 1))) || (rc = d_seq_off.ensure(8 * (size_t)(n + 1))) ||
        (rc = d_bases.ensure((size_t)nbases + 16)) || (rc = d_params.ensure(sizeof(sxg_poa_params) * (size_t)std::max(np, 1))) ||
        (rc = d_status.ensure(4 * (size_t)std::max(n, 1))) || (rc = d_score.ensure(4 * (size_t)std::max(n, 1))) || (rc = d_np.ensure(4 * (size_t)std::max(n, 1))) ||
        (rc = d_pr.ensure(4 * outcap)) || (rc = d_pp.ensure(4 * outcap)) || (rc = d_work.ensure(4 * (size_t)std::max(n, 1))) || (rc = d_queue.ensure(256)))
        return rc;
    if (n) {
        HIPCHK(hipMemcpy(d_row_off.p, in->row_off, 8 * (size_t)(n + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_seq_off.p, in->seq_off, 8 * (size_t)(n + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_pred_off.p, in->pred_off, 8 * (size_t)(rows + 1), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_params.p, in->params, sizeof(sxg_poa_params) * (size_t)np, hipMemcpyHostToDevice));
        if (rows) {
            HIPCHK(hipMemcpy(d_code.p, codes.data(), (size_t)rows, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(d_sink.p, in->row_sink, (size_t)rows, hipMemcpyHostToDevice));
        }
        if (ne) HIPCHK(hipMemcpy(d_preds.p, in->preds, 4 * (size_t)ne, hipMemcpyHostToDevice));
        if (nbases) HIPCHK(hipMemcpy(d_bases.p, stage.data(), (size_t)nbases, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_status.p, 0, 4 * (size_t)n)); HIPCHK(hipMemset(d_score.p, 0, 4 * (size_t)n)); HIPCHK(hipMemset(d_np.p, 0, 4 * (size_t)n));
    }
    // plans (the statistics of an align batch: launches, kernel time and the geometry of the plan with the most work)
    h->stats = sxg_poa_stats{};
    h->wstats = sxg_poa_width_stats{};
    h->tstats = sxg_poa_twin_stats{};
    const bool dbg = getenv("SXG_POA_DEBUG") != nullptr;
    double dom_work = -1;
    struct APlan { Variant variant; bool cvx, sw; std::vector<int32_t> work; int rows_cap = 0; };
    std::vector<APlan> plans;
    for (int p = 0; p < n; ++p) {
        const Scoring S = normalise(in->params[in->per_problem_params ? p : 0]);
        const int len = (int)(in->seq_off[p + 1] - in->seq_off[p]), N = (int)(in->row_off[p + 1] - in->row_off[p]);
        Variant v;   // (the align-only kernels run the 4-byte cells, no default-score class)
        int fw, fnw;
        forced_p16(&fw, &fnw);
        if (!variant_for_len(len, row_mode(S, len, N), &v, S.sw, 4, fw, fnw)) { o->status[p] = ST_TOO_LONG; continue; }
        APlan* pl = nullptr;
        for (auto& q : plans)
            if (q.variant == v && q.cvx == (bool)S.convex && q.sw == (bool)S.sw) { pl = &q; break; }
        if (!pl) { plans.push_back(APlan{v, (bool)S.convex, (bool)S.sw, {}, 0}); pl = &plans.back(); }
        pl->work.push_back(p);
        pl->rows_cap = std::max(pl->rows_cap, N);
    }
    if (n) HIPCHK(hipMemcpy(d_status.p, o->status.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    for (auto& pl : plans) {
        const Variant V = pl.variant;
        const int rows_cap = pl.rows_cap + 1;
        int64_t maxe = 0;
        for (int p : pl.work) maxe = std::max<int64_t>(maxe, in->pred_off[in->row_off[p + 1]] - in->pred_off[in->row_off[p]]);
        // r_preds is sized by nodes_cap in make_layout: give it the edge count
        const int wb = V.RM == 1 ? 8 : 4;
        SlotLayout lay2 = make_layout((int)std::max<int64_t>(maxe + 8, rows_cap + 8), rows_cap, rows_cap + 1,
                                      (int)maxe + 8, V.T(), V.Lpad(), wb, true, V.RM == 2 ? 2 * V.T() : 0);  // every strip kept
        if (V.RM == 2) lay2.lds_rows = p16_lds_rows(V.T(), V.W, 4);   // (the align-only kernel runs the 4-byte cells)
        auto kern = align_kernel(pl.variant, pl.cvx, pl.sw);
        const int tfix = class_traits(V.TMAX, V.W, V.RM, V.CB).tfix;
        if (!kern || (tfix && tfix != V.T())) return fail(SXG_E_INVALID, kern ? "kernel class compiled for another thread count" : "no kernel class built for this geometry");
        int per_cu = 1;
        int smem = V.RM == 2 ? dp16_lds_bytes(V.T(), V.W, lay2.lds_rows, 4) : dp_lds_launch_bytes(V.Lpad(), wb);
        const int pf_off = (V.RM != 2 && getenv("SXG_POA_PREFETCH")) ? dp_pf_offset(V.Lpad(), wb, V.T()) : -1;
        if (pf_off >= 0) smem += dp_pf_bytes(V.Lpad(), wb, V.T());
        if (smem > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)kern, V.T(), (size_t)smem) != hipSuccess || per_cu < 1) per_cu = 1;
        const uint64_t budget = arena_budget(h);
        int64_t n_slots = std::min<int64_t>((int64_t)pl.work.size(), (int64_t)h->num_cu * per_cu);
        n_slots = std::min<int64_t>(n_slots, (int64_t)(budget / lay2.total));
        if (n_slots < 1) return fail(SXG_E_NOMEM, "memory budget too small for one alignment arena");
        if ((rc = d_arena.ensure((size_t)n_slots * lay2.total))) return rc;
        HIPCHK(hipMemcpy(d_work.p, pl.work.data(), 4 * pl.work.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_queue.p, 0, 4));
        AlignArgs A;
        A.row_off = d_row_off.as<int64_t>(); A.row_code = d_code.as<uint8_t>(); A.row_sink = d_sink.as<uint8_t>();
        A.pred_off = d_pred_off.as<int64_t>(); A.preds = d_preds.as<int32_t>(); A.seq_off = d_seq_off.as<int64_t>();
        A.bases = d_bases.as<uint8_t>(); A.params = d_params.as<sxg_poa_params>(); A.per_problem_params = in->per_problem_params;
        A.work = d_work.as<int32_t>(); A.n_work = (int)pl.work.size(); A.queue = d_queue.as<int32_t>();
        A.arena = d_arena.as<uint8_t>(); A.lay = lay2;
        A.status = d_status.as<int32_t>(); A.score = d_score.as<int32_t>(); A.n_pairs = d_np.as<int32_t>();
        A.pair_row = d_pr.as<int32_t>(); A.pair_pos = d_pp.as<int32_t>();
        A.park_in_lds = (V.RM == 2 || dp_park_in_lds(V.Lpad(), wb)) ? 1 : 0;
        A.pf_off = pf_off;
        A.num_cu = std::max(h->num_cu, 1);
        HIPCHK(hipEventRecord(h->ev0, h->stream));
        hipLaunchKernelGGL(kern, dim3((unsigned)n_slots), dim3(V.T()), (size_t)smem, h->stream, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(h->ev1, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
        double work = 0;   // rows x letters of the plan's problems
        for (int p : pl.work) work += (double)(in->row_off[p + 1] - in->row_off[p]) * (double)(in->seq_off[p + 1] - in->seq_off[p]);
        h->stats.dp_launches += 1;
        h->stats.kernel_ms += ms;
        h->stats.n_slots += (int)n_slots;
        if (work > dom_work) {
            dom_work = work;
            h->stats.dom_kernel_ms = ms;
            h->stats.dom_threads = V.T(); h->stats.dom_cols_per_lane = V.W * (V.RM >= 2 ? 2 : 1); h->stats.dom_row_mode = V.RM;
            h->wstats.dom_width = V.W;
        }
        if (dbg)
            fprintf(stderr, "[sxg] variant T=%d W=%d cvx=%d rowmode=%d attempt=0 work=%zu slots=%lld per_cu=%d smem=%d slot_bytes=%zu free=0 ms=%.2f tmax=%d cb=%d ds=%d w2=%d\n",
                    V.T(), V.W, (int)pl.cvx, V.RM, pl.work.size(), (long long)n_slots, per_cu, smem, lay2.total, ms, V.TMAX, V.CB, (int)V.DS, V.W2);
    }
    std::vector<int32_t> npairs(std::max(n, 1), 0), pr(outcap), pp(outcap);
    if (n) {
        HIPCHK(hipMemcpy(o->status.data(), d_status.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(o->score.data(), d_score.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(npairs.data(), d_np.p, 4 * (size_t)n, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pr.data(), d_pr.p, 4 * outcap, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pp.data(), d_pp.p, 4 * outcap, hipMemcpyDeviceToHost));
    }
    for (int p = 0; p < n; ++p) o->pair_off[p + 1] = o->pair_off[p] + npairs[p];
    o->pair_row.resize((size_t)std::max<int64_t>(o->pair_off[n], 1)); o->pair_pos.resize(o->pair_row.size());
    for (int p = 0; p < n; ++p) {
        const int64_t s0 = in->row_off[p] + in->seq_off[p];
        std::copy(pr.begin() + s0, pr.begin() + s0 + npairs[p], o->pair_row.begin() + o->pair_off[p]);
        std::copy(pp.begin() + s0, pp.begin() + s0 + npairs[p], o->pair_pos.begin() + o->pair_off[p]);
    }
    guard.dismiss();   // (the caller keeps the result, also when a problem failed: SXG_E_BLOCK below)
    out->status = o->status.data(); out->score = o->score.data(); out->pair_off = o->pair_off.data();
    out->pair_row = o->pair_row.data(); out->pair_pos = o->pair_pos.data();
    for (int p = 0; p < n; ++p)
        if (o->status[p] != ST_OK) return fail(SXG_E_BLOCK, "problem " + std::to_string(p) + " failed with status " + std::to_string(o->status[p]));
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
// The identity split of break_blocks (src/breaks.cpp:335-586): decrees P1-P4 (include/sxg_poa.h).  Kernels in
// poa_split.hip.h / kern_split.hip; here the validation, the cost-sorted queues, the scratch (out of the memory budget) and the timing.
static_assert(SXG_POA_SPLIT_PANEL == SXG_SPLIT_PANEL, "panel width of the header");
static_assert(SXG_POA_MASH_SORT_TILE == SXG_MASH_SORT_TILE, "sort tile of the header");
namespace {
struct MashSets { DevBuf seq_off, bases, sets, set_size, sort_scratch, sketch_work, sketch_queue; };   // a call's uploaded sequences and, where it sketches them (mash_sketch), their k-mer sets
// kernel time of a call: the launches between the two on the handle's stream, by the handle's two events (timer_stop waits for them)
int timer_start(sxg_poa_handle* h) { HIPCHK(hipEventRecord(h->ev0, h->stream)); return SXG_OK; }
int timer_stop(sxg_poa_handle* h, float* ms) {
    HIPCHK(hipEventRecord(h->ev1, h->stream)); HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return SXG_OK;
}
// slots of a split launch: what fits the chip, the work and the budget (one slot = one wavefront with its boundary column)
int split_slots(sxg_poa_handle* h, int per_cu, int64_t n_work, size_t slot_bytes, int64_t* n_slots) {
    int64_t n = std::min<int64_t>(n_work, (int64_t)std::max(h->num_cu, 1) * per_cu);
    n = std::min<int64_t>(n, (int64_t)(arena_budget(h) / std::max<size_t>(slot_bytes, 1)));
    if (n < 1) return fail(SXG_E_NOMEM, "memory budget too small for one split slot");
    *n_slots = n;
    return SXG_OK;
}
int split_upload_seqs(sxg_poa_handle* h, MashSets& B, int64_t n_seqs, const int64_t* seq_off, const uint8_t* bases) {
    const int64_t nbases = seq_off[n_seqs];
    std::vector<uint8_t> stage((size_t)std::max<int64_t>(nbases, 1));
    for (int64_t i = 0; i < nbases; ++i) stage[(size_t)i] = bases[i] > 4 ? 4 : bases[i];
    if (int rc = B.seq_off.ensure(8 * (size_t)(n_seqs + 1))) return rc;
    if (int rc = B.bases.ensure((size_t)nbases + 16)) return rc;
    HIPCHK(hipMemcpyAsync(B.seq_off.p, seq_off, 8 * (size_t)(n_seqs + 1), hipMemcpyHostToDevice, h->stream));
    if (nbases) HIPCHK(hipMemcpyAsync(B.bases.p, stage.data(), (size_t)nbases, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));   // (stage leaves scope)
    return SXG_OK;
}
template <class Tp> int split_up(sxg_poa_handle* h, DevBuf& d, const Tp* src, size_t n) {
    if (int rc = d.ensure(sizeof(Tp) * std::max<size_t>(n, 1))) return rc;
    if (n) HIPCHK(hipMemcpy(d.p, src, sizeof(Tp) * n, hipMemcpyHostToDevice));
    return SXG_OK;
}
// M1 on the device: the sets of the sequences in `work` (made longest first here) into B.sets / B.set_size, every other sequence
// with size 0.  B.seq_off / B.bases are uploaded; the launch goes on the handle's stream; *dev_bytes: sets and sort scratch.
int mash_sketch(sxg_poa_handle* h, MashSets& B, int64_t ns, const int64_t* seq_off, std::vector<int32_t>& work, int k, bool clear_sets, size_t* dev_bytes) {
    const int64_t nbases = seq_off[ns];
    if (int rc = B.sets.ensure(8 * (size_t)std::max<int64_t>(nbases, 1))) return rc;
    if (int rc = B.set_size.ensure(4 * (size_t)std::max<int64_t>(ns, 1))) return rc;
    HIPCHK(hipMemsetAsync(B.set_size.p, 0, 4 * (size_t)std::max<int64_t>(ns, 1), h->stream));
    if (clear_sets) HIPCHK(hipMemsetAsync(B.sets.p, 0, 8 * (size_t)std::max<int64_t>(nbases, 1), h->stream));
    *dev_bytes = B.sets.cap + B.set_size.cap;
    if (work.empty()) return SXG_OK;
    auto len_of = [&](int32_t s) { return seq_off[s + 1] - seq_off[s]; };
    std::stable_sort(work.begin(), work.end(), [&](int32_t x, int32_t y) { return len_of(x) > len_of(y); });
    const int64_t max_nk = len_of(work[0]) - k + 1;
    const int64_t scratch_keys = max_nk > SXG_MASH_SORT_TILE ? (max_nk + SXG_MASH_SORT_TILE - 1) / SXG_MASH_SORT_TILE * SXG_MASH_SORT_TILE : 0;
    const size_t slot_bytes = 2 * sizeof(unsigned long long) * (size_t)scratch_keys;
    int per_cu = 1;
    sxg_mash_occupancy(0, &per_cu);
    int64_t n_slots = std::min<int64_t>((int64_t)work.size(), (int64_t)std::max(h->num_cu, 1) * per_cu);
    if (slot_bytes) n_slots = std::min<int64_t>(n_slots, (int64_t)(arena_budget(h) / slot_bytes));
    if (n_slots < 1) return fail(SXG_E_NOMEM, "memory budget too small for one sort slot of the k-mer sets");
    if (int rc = B.sort_scratch.ensure(std::max<size_t>(slot_bytes * (size_t)n_slots, 16))) return rc;
    if (int rc = split_up(h, B.sketch_work, work.data(), work.size())) return rc;
    if (int rc = B.sketch_queue.ensure(256)) return rc;
    HIPCHK(hipMemsetAsync(B.sketch_queue.p, 0, 4, h->stream));
    MashSketchArgs A;
    A.seq_off = B.seq_off.as<int64_t>(); A.bases = B.bases.as<uint8_t>(); A.work = B.sketch_work.as<int32_t>(); A.n_work = (int32_t)work.size();
    A.queue = B.sketch_queue.as<int32_t>(); A.k = k; A.scratch = B.sort_scratch.as<unsigned long long>(); A.scratch_keys = scratch_keys;
    A.sets = B.sets.as<unsigned long long>(); A.set_size = B.set_size.as<int32_t>();
    sxg_mash_launch_sketch(A, (int)n_slots, h->stream);
    HIPCHK(hipGetLastError());
    *dev_bytes += B.sort_scratch.cap;
    return SXG_OK;
}
void split_stats(sxg_poa_handle* h, float ms, uint64_t cells, int64_t n_slots, size_t dev_bytes) {
    h->stats = sxg_poa_stats{};
    h->stats.kernel_ms = ms; h->stats.cells = cells; h->stats.dp_launches = 1; h->stats.n_slots = (int32_t)n_slots;
    h->stats.device_bytes = dev_bytes;
    h->stats.dom_kernel_ms = ms; h->stats.dom_cells = cells; h->stats.dom_threads = 64; h->stats.dom_cols_per_lane = SXG_SPLIT_W;
}
}  // namespace

extern "C" int sxg_poa_pair_identity_batch(sxg_poa_handle* h, int64_t n_seqs, const int64_t* seq_off, const uint8_t* bases, int64_t n_pairs,
                                           const int32_t* pair_a, const int32_t* pair_b, const uint8_t* b_rev, const int32_t* cap,
                                           int32_t* penalty, int32_t* cols, int32_t* matches) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (n_seqs < 0 || n_pairs < 0 || n_pairs > 0x7fffffff || !seq_off || (n_pairs > 0 && (!pair_a || !pair_b || !cap || !penalty || !cols || !matches)))
        return fail(SXG_E_INVALID, "pair_identity: bad argument");
    if (seq_off[0] != 0) return fail(SXG_E_INVALID, "seq_off[0] must be 0");
    for (int64_t s = 0; s < n_seqs; ++s)
        if (seq_off[s + 1] < seq_off[s]) return fail(SXG_E_INVALID, "seq_off not monotone");
    if (seq_off[n_seqs] > 0 && !bases) return fail(SXG_E_INVALID, "bases is NULL");
    RoctxRange range("sxg_poa_pair_identity_batch");
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    if (n_pairs == 0) return SXG_OK;
    uint64_t cells = 0;
    int64_t max_la = 0;
    std::vector<std::pair<int64_t, int32_t>> cost((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; ++k) {
        if (pair_a[k] < 0 || pair_a[k] >= n_seqs || pair_b[k] < 0 || pair_b[k] >= n_seqs) return fail(SXG_E_INVALID, "pair " + std::to_string(k) + ": no such sequence");
        const int64_t la = seq_off[pair_a[k] + 1] - seq_off[pair_a[k]], lb = seq_off[pair_b[k] + 1] - seq_off[pair_b[k]];
        if (la < 1 || lb < 1) return fail(SXG_E_INVALID, "pair " + std::to_string(k) + ": zero-length sequence");
        if (la > SXG_POA_MAX_SEQ_LEN || lb > SXG_POA_MAX_SEQ_LEN) return fail(SXG_E_INVALID, "pair " + std::to_string(k) + ": sequence longer than SXG_POA_MAX_SEQ_LEN");
        cost[(size_t)k] = {la * lb, (int32_t)k};
        cells += (uint64_t)(la * lb);
        max_la = std::max(max_la, la);
    }
    std::stable_sort(cost.begin(), cost.end(), [](const std::pair<int64_t, int32_t>& x, const std::pair<int64_t, int32_t>& y) { return x.first > y.first; });
    std::vector<int32_t> work((size_t)n_pairs);
    for (int64_t k = 0; k < n_pairs; ++k) work[(size_t)k] = cost[(size_t)k].second;
    std::vector<uint8_t> rev((size_t)n_pairs, 0);
    if (b_rev) for (int64_t k = 0; k < n_pairs; ++k) rev[(size_t)k] = b_rev[k] ? 1 : 0;
    MashSets seqs;   // (the sequences only: this call sketches nothing)
    DevBuf d_pair_a, d_pair_b, d_rev, d_cap, d_work, d_queue, d_bound, d_penalty, d_cols, d_matches;
    int rc;
    if ((rc = split_upload_seqs(h, seqs, n_seqs, seq_off, bases)) || (rc = split_up(h, d_pair_a, pair_a, (size_t)n_pairs)) ||
        (rc = split_up(h, d_pair_b, pair_b, (size_t)n_pairs)) || (rc = split_up(h, d_rev, rev.data(), (size_t)n_pairs)) ||
        (rc = split_up(h, d_cap, cap, (size_t)n_pairs)) || (rc = split_up(h, d_work, work.data(), (size_t)n_pairs)) ||
        (rc = d_penalty.ensure(4 * (size_t)n_pairs)) || (rc = d_cols.ensure(4 * (size_t)n_pairs)) || (rc = d_matches.ensure(4 * (size_t)n_pairs)) || (rc = d_queue.ensure(256)))
        return rc;
    const int64_t bound_rows = max_la + 1;
    const size_t slot_bytes = 3 * sizeof(sxg_key_t) * (size_t)bound_rows;
    int64_t n_slots = 0;
    int per_cu = 1;
    sxg_split_occupancy(0, &per_cu);
    if ((rc = split_slots(h, per_cu, n_pairs, slot_bytes, &n_slots)) || (rc = d_bound.ensure(slot_bytes * (size_t)n_slots))) return rc;
    HIPCHK(hipMemsetAsync(d_queue.p, 0, 4, h->stream));
    SplitPairArgs A;
    A.seq_off = seqs.seq_off.as<int64_t>(); A.bases = seqs.bases.as<uint8_t>(); A.pair_a = d_pair_a.as<int32_t>(); A.pair_b = d_pair_b.as<int32_t>();
    A.b_rev = d_rev.as<uint8_t>(); A.cap = d_cap.as<int32_t>(); A.work = d_work.as<int32_t>(); A.n_work = (int32_t)n_pairs;
    A.queue = d_queue.as<int32_t>(); A.bound = d_bound.as<sxg_key_t>(); A.bound_rows = bound_rows;
    A.penalty = d_penalty.as<int32_t>(); A.cols = d_cols.as<int32_t>(); A.matches = d_matches.as<int32_t>();
    float ms = 0;
    if ((rc = timer_start(h))) return rc;
    sxg_split_launch_pairs(A, (int)n_slots, h->stream);
    HIPCHK(hipGetLastError());
    if ((rc = timer_stop(h, &ms))) return rc;
    HIPCHK(hipMemcpy(penalty, d_penalty.p, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cols, d_cols.p, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(matches, d_matches.p, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost));
    split_stats(h, ms, cells, n_slots, d_bound.cap);
    return SXG_OK;
}

struct SplitOwner {
    std::vector<int32_t> group, n_groups, status;
    std::vector<int64_t> n_pairs;
};
extern "C" void sxg_poa_split_free(sxg_poa_split_out* out) {
    if (!out) return;
    delete (SplitOwner*)out->_owner;
    memset(out, 0, sizeof(*out));
}
// P3 for every block; with `mash`, M1-M5 on top of it (the blocks with min_len > 0 get their sets first)
static int split_batch(sxg_poa_handle* h, const sxg_poa_split_in* in, const sxg_poa_split_mash* mash, sxg_poa_split_out* out, int64_t* n_mash,
                       const char* range_name) {
    if (!h || !in || !out) return fail(SXG_E_INVALID, "NULL argument");
    memset(out, 0, sizeof(*out));
    const int nb = in->n_blocks;
    if (nb < 0 || (nb > 0 && (!in->blk_off || !in->seq_off || !in->identity || !in->length_ratio_min))) return fail(SXG_E_INVALID, "split_in has NULL arrays");
    if (nb > 0 && (in->blk_off[0] != 0 || in->seq_off[0] != 0)) return fail(SXG_E_INVALID, "blk_off[0] and seq_off[0] must be 0");
    for (int b = 0; b < nb; ++b) {
        if (in->blk_off[b + 1] < in->blk_off[b]) return fail(SXG_E_INVALID, "blk_off not monotone");
        if (!(in->identity[b] > 0.0 && in->identity[b] <= 1.0)) return fail(SXG_E_INVALID, "block " + std::to_string(b) + ": identity must be in (0, 1]");
        if (!(in->length_ratio_min[b] == in->length_ratio_min[b])) return fail(SXG_E_INVALID, "block " + std::to_string(b) + ": length_ratio_min is NaN");
    }
    const int64_t ns = nb ? in->blk_off[nb] : 0;
    for (int64_t s = 0; s < ns; ++s)
        if (in->seq_off[s + 1] <= in->seq_off[s]) return fail(SXG_E_INVALID, "sequence " + std::to_string(s) + " has no bases (or seq_off is not monotone)");
    if (ns > 0 && !in->bases) return fail(SXG_E_INVALID, "bases is NULL");
    std::vector<double> mash_f, mash_jmin;
    if (mash) {                                                                     // M2, M3, M5
        const int k = mash->kmer_size;
        if (k < 1 || k > 32) return fail(SXG_E_INVALID, "kmer_size must be in 1..32");
        if (nb > 0 && (!mash->min_len || !mash->est_identity)) return fail(SXG_E_INVALID, "split_mash has NULL arrays");
        mash_f.assign((size_t)std::max(nb, 1), 0.0); mash_jmin.assign((size_t)std::max(nb, 1), 0.0);
        for (int b = 0; b < nb; ++b) {
            const double e = mash->est_identity[b];
            if (mash->min_len[b] < 0 || (mash->min_len[b] > 0 && mash->min_len[b] < k))
                return fail(SXG_E_INVALID, "block " + std::to_string(b) + ": min_len must be 0 or at least kmer_size");
            if (!(e > 0.0 && e <= 1.0)) return fail(SXG_E_INVALID, "block " + std::to_string(b) + ": est_identity must be in (0, 1]");
            const double v = exp(-(1.0 - in->identity[b]) * (double)k), w = exp(-(1.0 - e) * (double)k);
            mash_f[(size_t)b] = v / (2.0 - v);
            mash_jmin[(size_t)b] = w / (2.0 - w);
        }
        if (n_mash) for (int b = 0; b < nb; ++b) n_mash[b] = 0;
    }
    RoctxRange range(range_name);
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    SplitOwner* o = new SplitOwner();
    out->_owner = o; out->n_blocks = nb; out->n_seqs = ns;
    OutGuard<sxg_poa_split_out, sxg_poa_split_free> guard(out);   // (every return below but those after dismiss() frees the result)
    o->group.assign((size_t)std::max<int64_t>(ns, 1), 0); o->n_groups.assign((size_t)std::max(nb, 1), 0);
    o->status.assign((size_t)std::max(nb, 1), 0); o->n_pairs.assign((size_t)std::max(nb, 1), 0);
    out->group = o->group.data(); out->n_groups = o->n_groups.data(); out->status = o->status.data(); out->n_pairs = o->n_pairs.data();
    // the queue: blocks by cost (sum of len_i * len_(i-1)), most expensive first; a block with a sequence too long stays out
    std::vector<std::pair<uint64_t, int32_t>> cost;
    int64_t max_len = 0, max_depth = 0;
    bool any_failed = false;
    for (int b = 0; b < nb; ++b) {
        const int64_t s0 = in->blk_off[b], s1 = in->blk_off[b + 1];
        uint64_t c = 0;
        int64_t longest = 0;
        for (int64_t s = s0; s < s1; ++s) {
            const int64_t len = in->seq_off[s + 1] - in->seq_off[s];
            longest = std::max(longest, len);
            if (s > s0) c += (uint64_t)len * (uint64_t)(in->seq_off[s] - in->seq_off[s - 1]);
        }
        if (longest > SXG_POA_MAX_SEQ_LEN) { o->status[(size_t)b] = SXG_ST_TOO_LONG; any_failed = true; continue; }
        if (s1 == s0) continue;
        cost.push_back({c, b});
        max_len = std::max(max_len, longest);
        max_depth = std::max(max_depth, s1 - s0);
    }
    if (!cost.empty()) {
        std::stable_sort(cost.begin(), cost.end(), [](const std::pair<uint64_t, int32_t>& x, const std::pair<uint64_t, int32_t>& y) { return x.first > y.first; });
        std::vector<int32_t> work(cost.size());
        for (size_t k = 0; k < cost.size(); ++k) work[k] = cost[k].second;
        MashSets seqs;
        DevBuf d_blk_off, d_identity, d_ratio_min, d_work, d_queue, d_bound, d_lists, d_group, d_n_groups, d_n_pairs, d_cells,
            d_min_len, d_mash_f, d_mash_jmin, d_n_mash;   // (the last four: the mash-based branch)
        int rc;
        if ((rc = split_upload_seqs(h, seqs, ns, in->seq_off, in->bases)) || (rc = split_up(h, d_blk_off, in->blk_off, (size_t)nb + 1)) ||
            (rc = split_up(h, d_identity, in->identity, (size_t)nb)) || (rc = split_up(h, d_ratio_min, in->length_ratio_min, (size_t)nb)) ||
            (rc = split_up(h, d_work, work.data(), work.size())) ||
            (rc = d_group.ensure(4 * (size_t)ns)) || (rc = d_n_groups.ensure(4 * (size_t)nb)) || (rc = d_n_pairs.ensure(8 * (size_t)nb)) ||
            (rc = d_cells.ensure(8 * (size_t)nb)) || (rc = d_queue.ensure(256)))
            return rc;
        const int64_t bound_rows = max_len + 1;
        const size_t slot_bytes = 3 * sizeof(sxg_key_t) * (size_t)bound_rows + 2 * sizeof(int32_t) * (size_t)max_depth;
        int64_t n_slots = 0;
        int per_cu = 1;
        if (mash) sxg_mash_occupancy(2, &per_cu); else sxg_split_occupancy(1, &per_cu);
        if ((rc = split_slots(h, per_cu, (int64_t)work.size(), slot_bytes, &n_slots))) return rc;
        if ((rc = d_bound.ensure(3 * sizeof(sxg_key_t) * (size_t)bound_rows * (size_t)n_slots))) return rc;
        if ((rc = d_lists.ensure(2 * sizeof(int32_t) * (size_t)max_depth * (size_t)n_slots))) return rc;
        HIPCHK(hipMemsetAsync(d_queue.p, 0, 4, h->stream));
        HIPCHK(hipMemsetAsync(d_group.p, 0, 4 * (size_t)ns, h->stream));
        HIPCHK(hipMemsetAsync(d_n_groups.p, 0, 4 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(d_n_pairs.p, 0, 8 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(d_cells.p, 0, 8 * (size_t)nb, h->stream));
        SplitBlockArgs A;
        A.blk_off = d_blk_off.as<int32_t>(); A.seq_off = seqs.seq_off.as<int64_t>(); A.bases = seqs.bases.as<uint8_t>();
        A.identity = d_identity.as<double>(); A.ratio_min = d_ratio_min.as<double>(); A.work = d_work.as<int32_t>(); A.n_work = (int32_t)work.size();
        A.queue = d_queue.as<int32_t>(); A.bound = d_bound.as<sxg_key_t>(); A.bound_rows = bound_rows;
        A.lists = d_lists.as<int32_t>(); A.list_cap = max_depth;
        A.group = d_group.as<int32_t>(); A.n_groups = d_n_groups.as<int32_t>(); A.n_pairs = d_n_pairs.as<int64_t>(); A.cells = d_cells.as<uint64_t>();
        size_t mash_bytes = 0;
        MashBlockArgs M;
        std::vector<int32_t> sketch_work;
        if (mash) {
            for (const auto& cb : cost) {                                          // M1: the eligible sequences of the blocks that run
                const int b = cb.second;
                if (mash->min_len[b] <= 0) continue;
                for (int64_t s = in->blk_off[b]; s < in->blk_off[b + 1]; ++s)
                    if (in->seq_off[s + 1] - in->seq_off[s] >= mash->min_len[b]) sketch_work.push_back((int32_t)s);
            }
            if ((rc = split_up(h, d_min_len, mash->min_len, (size_t)nb)) || (rc = split_up(h, d_mash_f, mash_f.data(), (size_t)nb)) ||
                (rc = split_up(h, d_mash_jmin, mash_jmin.data(), (size_t)nb)) || (rc = d_n_mash.ensure(8 * (size_t)nb)))
                return rc;
            HIPCHK(hipMemsetAsync(d_n_mash.p, 0, 8 * (size_t)nb, h->stream));
        }
        float ms = 0;
        if ((rc = timer_start(h))) return rc;
        if (mash) {
            if ((rc = mash_sketch(h, seqs, ns, in->seq_off, sketch_work, mash->kmer_size, false, &mash_bytes))) return rc;
            M.S = A; M.min_len = d_min_len.as<int32_t>(); M.f = d_mash_f.as<double>(); M.jmin = d_mash_jmin.as<double>();
            M.sets = seqs.sets.as<unsigned long long>(); M.set_size = seqs.set_size.as<int32_t>(); M.n_mash = d_n_mash.as<int64_t>();
            sxg_mash_launch_blocks(M, (int)n_slots, h->stream);
        } else sxg_split_launch_blocks(A, (int)n_slots, h->stream);
        HIPCHK(hipGetLastError());
        if ((rc = timer_stop(h, &ms))) return rc;
        std::vector<uint64_t> cells((size_t)nb);
        HIPCHK(hipMemcpy(o->group.data(), d_group.p, 4 * (size_t)ns, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(o->n_groups.data(), d_n_groups.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(o->n_pairs.data(), d_n_pairs.p, 8 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cells.data(), d_cells.p, 8 * (size_t)nb, hipMemcpyDeviceToHost));
        if (mash && n_mash) HIPCHK(hipMemcpy(n_mash, d_n_mash.p, 8 * (size_t)nb, hipMemcpyDeviceToHost));
        uint64_t total = 0;
        for (uint64_t c : cells) total += c;
        split_stats(h, ms, total, n_slots, d_bound.cap + d_lists.cap + mash_bytes);
        if (mash && !sketch_work.empty()) h->stats.dp_launches = 2;
    }
    guard.dismiss();   // (the caller keeps the result, also when a block failed: SXG_E_BLOCK below)
    if (any_failed) return fail(SXG_E_BLOCK, "a block holds a sequence longer than SXG_POA_MAX_SEQ_LEN");
    return SXG_OK;
}
extern "C" int sxg_poa_split_batch(sxg_poa_handle* h, const sxg_poa_split_in* in, sxg_poa_split_out* out) {
    return split_batch(h, in, nullptr, out, nullptr, "sxg_poa_split_batch");
}
extern "C" int sxg_poa_split_mash_batch(sxg_poa_handle* h, const sxg_poa_split_in* in, const sxg_poa_split_mash* mash, sxg_poa_split_out* out,
                                        int64_t* n_mash) {
    if (!mash) return fail(SXG_E_INVALID, "NULL argument");
    return split_batch(h, in, mash, out, n_mash, "sxg_poa_split_mash_batch");
}

// M1 for callers and tests: the set of every sequence (no min_len), and the exact intersection of pairs of them.
extern "C" int sxg_poa_kmer_jaccard_batch(sxg_poa_handle* h, int64_t n_seqs, const int64_t* seq_off, const uint8_t* bases, int32_t kmer_size,
                                          int64_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, int32_t* set_size, int32_t* inter,
                                          uint64_t* kmers) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (n_seqs < 0 || n_seqs > 0x7fffffff || n_pairs < 0 || n_pairs > 0x7fffffff || !seq_off || (n_seqs > 0 && !set_size) ||
        (n_pairs > 0 && (!pair_a || !pair_b || !inter)))
        return fail(SXG_E_INVALID, "kmer_jaccard: bad argument");
    if (kmer_size < 1 || kmer_size > 32) return fail(SXG_E_INVALID, "kmer_size must be in 1..32");
    if (seq_off[0] != 0) return fail(SXG_E_INVALID, "seq_off[0] must be 0");
    std::vector<int32_t> work;
    for (int64_t s = 0; s < n_seqs; ++s) {
        const int64_t len = seq_off[s + 1] - seq_off[s];
        if (len < 0) return fail(SXG_E_INVALID, "seq_off not monotone");
        if (len > SXG_POA_MAX_SEQ_LEN) return fail(SXG_E_INVALID, "sequence " + std::to_string(s) + " is longer than SXG_POA_MAX_SEQ_LEN");
        if (len >= kmer_size) work.push_back((int32_t)s);
    }
    if (seq_off[n_seqs] > 0 && !bases) return fail(SXG_E_INVALID, "bases is NULL");
    for (int64_t p = 0; p < n_pairs; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= n_seqs || pair_b[p] < 0 || pair_b[p] >= n_seqs) return fail(SXG_E_INVALID, "pair " + std::to_string(p) + ": no such sequence");
    RoctxRange range("sxg_poa_kmer_jaccard_batch");
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    if (n_seqs == 0) return SXG_OK;
    MashSets seqs;
    DevBuf d_pair_a, d_pair_b, d_inter, d_queue;
    if (int rc = split_upload_seqs(h, seqs, n_seqs, seq_off, bases)) return rc;
    size_t dev_bytes = 0;
    int64_t n_slots = 0;
    if (n_pairs) {
        int rc;
        if ((rc = split_up(h, d_pair_a, pair_a, (size_t)n_pairs)) || (rc = split_up(h, d_pair_b, pair_b, (size_t)n_pairs)) ||
            (rc = d_inter.ensure(4 * (size_t)n_pairs)) || (rc = d_queue.ensure(256)))
            return rc;
        HIPCHK(hipMemsetAsync(d_queue.p, 0, 4, h->stream));
    }
    float ms = 0;
    if (int rc = timer_start(h)) return rc;
    if (int rc = mash_sketch(h, seqs, n_seqs, seq_off, work, kmer_size, kmers != nullptr, &dev_bytes)) return rc;
    if (n_pairs) {
        int per_cu = 1;
        sxg_mash_occupancy(1, &per_cu);
        n_slots = std::min<int64_t>(n_pairs, (int64_t)std::max(h->num_cu, 1) * per_cu);
        MashPairArgs A;
        A.seq_off = seqs.seq_off.as<int64_t>(); A.sets = seqs.sets.as<unsigned long long>(); A.set_size = seqs.set_size.as<int32_t>();
        A.pair_a = d_pair_a.as<int32_t>(); A.pair_b = d_pair_b.as<int32_t>(); A.n_pairs = (int32_t)n_pairs; A.queue = d_queue.as<int32_t>();
        A.inter = d_inter.as<int32_t>();
        sxg_mash_launch_pairs(A, (int)n_slots, h->stream);
        HIPCHK(hipGetLastError());
    }
    if (int rc = timer_stop(h, &ms)) return rc;
    HIPCHK(hipMemcpy(set_size, seqs.set_size.p, 4 * (size_t)n_seqs, hipMemcpyDeviceToHost));
    if (n_pairs) HIPCHK(hipMemcpy(inter, d_inter.p, 4 * (size_t)n_pairs, hipMemcpyDeviceToHost));
    if (kmers && seq_off[n_seqs] > 0) HIPCHK(hipMemcpy(kmers, seqs.sets.p, 8 * (size_t)seq_off[n_seqs], hipMemcpyDeviceToHost));
    split_stats(h, ms, 0, n_slots, dev_bytes);
    h->stats.dp_launches = n_pairs ? 2 : 1;
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
// Resident path letters (include/sxg_poa.h): one copy of a graph's path letters per handle, outside the
// memory budget; the ranges calls below cut their sequences out of it with range_gather_kernel (poa_letters.hip.h /
// kern_letters.hip) instead of uploading them.  Here the staged upload, the validation of ranges and the gather's launch and timing.
static_assert(SXG_LETTERS_CHUNK % 16 == 0, "a chunk is whole granules");
namespace {
constexpr size_t LETTERS_STAGE_BYTES = (size_t)8 << 20;   // one pinned staging buffer of the upload; two are in flight
struct PinLoan {   // a buffer of the pool, given back on every way out
    PinPool* pool = nullptr;
    void* p = nullptr;
    PinLoan() = default;
    PinLoan(const PinLoan&) = delete;
    PinLoan& operator=(const PinLoan&) = delete;
    ~PinLoan() { if (p) pool->release(p); }
};
void letters_forget(sxg_poa_handle* h) {
    auto& L = h->letters;
    L.id = 0; L.n_paths = 0; L.n_letters = 0;
    L.path_off.clear();
    L.d.release();
}
int letters_upload(sxg_poa_handle* h, const sxg_poa_letters* l) {
    if (!l || l->id == 0 || l->n_paths < 0 || !l->path_off || l->path_off[0] != 0) return fail(SXG_E_INVALID, "letters: id must be non-zero, path_off[0] must be 0");
    for (int64_t p = 0; p < l->n_paths; ++p)
        if (l->path_off[p + 1] < l->path_off[p]) return fail(SXG_E_INVALID, "letters: path_off not monotone");
    const int64_t n = l->path_off[l->n_paths];
    if (n > 0 && !l->letters) return fail(SXG_E_INVALID, "letters is NULL");
    auto& L = h->letters;
    letters_forget(h);   // (a failure below leaves nothing resident)
    if (int rc = L.d.ensure((size_t)std::max<int64_t>(n, 1))) return rc;
    PinLoan pin[2];
    DevEvent done[2];
    if (h->pins && !getenv("SXG_POA_NO_PINNED"))
        for (int b = 0; b < 2 && (b == 0 || (size_t)n > LETTERS_STAGE_BYTES); ++b) {
            pin[b].pool = h->pins.get();
            pin[b].p = h->pins->acquire(std::min<size_t>(LETTERS_STAGE_BYTES, (size_t)std::max<int64_t>(n, 1)));
            if (pin[b].p && done[b].create() != hipSuccess) { (void)hipGetLastError(); h->pins->release(pin[b].p); pin[b].p = nullptr; }
        }
    struct Forget { sxg_poa_handle* h; ~Forget() { if (h) letters_forget(h); } } forget{h};
    int64_t k = 0;
    for (int64_t at = 0; at < n; at += (int64_t)LETTERS_STAGE_BYTES, ++k) {
        const size_t len = (size_t)std::min<int64_t>((int64_t)LETTERS_STAGE_BYTES, n - at);
        const int b = pin[1].p ? (int)(k & 1) : 0;
        if (pin[b].p) {
            if (k >= (pin[1].p ? 2 : 1)) HIPCHK(hipEventSynchronize(done[b]));   // (the copy that last read this buffer)
            memcpy(pin[b].p, l->letters + at, len);
            HIPCHK(hipMemcpyAsync(L.d.as<uint8_t>() + at, pin[b].p, len, hipMemcpyHostToDevice, h->stream));
            HIPCHK(hipEventRecord(done[b], h->stream));
        } else {   // (no pinned buffer to borrow: the runtime stages the pageable copy itself)
            HIPCHK(hipMemcpyAsync(L.d.as<uint8_t>() + at, l->letters + at, len, hipMemcpyHostToDevice, h->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    forget.h = nullptr;
    L.id = l->id; L.n_paths = l->n_paths; L.n_letters = n;
    L.path_off.assign(l->path_off, l->path_off + l->n_paths + 1);
    ++L.uploads; L.bytes_uploaded += (uint64_t)n;
    return SXG_OK;
}
// The letters a ranges call works on -- uploaded here when other letters, or none, are resident and the caller passed these --
// and its ranges, checked: len[s] and src[s], the length of range s and where it starts in the resident letters.
int letters_resolve(sxg_poa_handle* h, const sxg_poa_letters* l, uint64_t id, int64_t n, const sxg_poa_range* r, const char* what,
                    std::vector<int64_t>& len, std::vector<int64_t>& src) {
    auto& L = h->letters;
    if (id == 0) return fail(SXG_E_INVALID, std::string(what) + ": letters_id is 0");
    if (n < 0 || (n > 0 && !r)) return fail(SXG_E_INVALID, std::string(what) + ": ranges is NULL");
    if (L.id != id) {
        if (!l || l->id != id) return fail(SXG_E_INVALID, std::string(what) + ": letters " + std::to_string(id) + " are not resident and were not passed");
        if (int rc = letters_upload(h, l)) return rc;
    }
    len.assign((size_t)n, 0); src.assign((size_t)n, 0);
    for (int64_t s = 0; s < n; ++s) {
        if (r[s].path < 0 || r[s].path >= L.n_paths || r[s].begin < 0 || r[s].end < r[s].begin ||
            r[s].end > L.path_off[(size_t)r[s].path + 1] - L.path_off[(size_t)r[s].path])
            return fail(SXG_E_INVALID, std::string(what) + ": range " + std::to_string(s) + " (path " + std::to_string(r[s].path) + ", " + std::to_string(r[s].begin) + " .. " +
                                           std::to_string(r[s].end) + ") lies outside the resident letters");
        len[(size_t)s] = r[s].end - r[s].begin;
        src[(size_t)s] = L.path_off[(size_t)r[s].path] + r[s].begin;
    }
    return SXG_OK;
}
// the gather's per-call arrays, enqueued on the handle's stream: where every destination sequence starts in the resident letters
// and -- unless the caller has them on the device already -- the destination offsets.  The caller waits for the stream.
int letters_stage(sxg_poa_handle* h, const std::vector<int64_t>& src, const int64_t* dst_off) {
    auto& L = h->letters;
    const size_t n = src.size();
    if (int rc = L.d_src.ensure(8 * std::max<size_t>(n, 1))) return rc;
    if (n) HIPCHK(hipMemcpyAsync(L.d_src.p, src.data(), 8 * n, hipMemcpyHostToDevice, h->stream));
    if (dst_off) {
        if (int rc = L.d_off.ensure(8 * (n + 1))) return rc;
        HIPCHK(hipMemcpyAsync(L.d_off.p, dst_off, 8 * (n + 1), hipMemcpyHostToDevice, h->stream));
    }
    return SXG_OK;
}
// the launch, between the call's timer_start and timer_stop, bracketed by events of its own; letters_account after timer_stop
int letters_launch(sxg_poa_handle* h, int64_t n, int64_t total, const int64_t* d_dst_off, uint8_t* d_dst, int coded) {
    auto& L = h->letters;
    if (n <= 0 || total <= 0) return SXG_OK;
    if (!L.g0.raw) HIPCHK(L.g0.create());
    if (!L.g1.raw) HIPCHK(L.g1.create());
    LettersGatherArgs A;
    A.letters = L.d.as<uint8_t>(); A.dst = d_dst; A.dst_off = d_dst_off; A.src = L.d_src.as<int64_t>(); A.n = n; A.total = total;
    const int64_t groups = std::min<int64_t>(sxg_letters_n_chunks(total), (int64_t)std::max(h->num_cu, 1) * 8);
    HIPCHK(hipEventRecord(L.g0, h->stream));
    sxg_letters_launch_gather(A, coded, (int)groups, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(L.g1, h->stream));
    L.pending = true; L.pending_bytes = (uint64_t)total;
    return SXG_OK;
}
int letters_account(sxg_poa_handle* h) {
    auto& L = h->letters;
    if (!L.pending) return SXG_OK;
    L.pending = false;
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, L.g0, L.g1));
    L.gather_ms += ms; L.gathered_bytes += L.pending_bytes;
    return SXG_OK;
}
}  // namespace

extern "C" int sxg_poa_letters_upload(sxg_poa_handle* h, const sxg_poa_letters* l) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    RoctxRange range("sxg_poa_letters_upload");
    HIPCHK(hipSetDevice(h->device));
    return letters_upload(h, l);
}
extern "C" void sxg_poa_letters_drop(sxg_poa_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    letters_forget(h);
}
extern "C" int sxg_poa_letters_resident(sxg_poa_handle* h, uint64_t* id, int64_t* n_paths, int64_t* n_letters) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (id) *id = h->letters.id;
    if (n_paths) *n_paths = h->letters.n_paths;
    if (n_letters) *n_letters = h->letters.n_letters;
    return SXG_OK;
}
extern "C" int sxg_poa_letters_stats(sxg_poa_handle* h, uint64_t* uploads, uint64_t* bytes_uploaded, double* gather_ms, uint64_t* gathered_bytes) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    if (uploads) *uploads = h->letters.uploads;
    if (bytes_uploaded) *bytes_uploaded = h->letters.bytes_uploaded;
    if (gather_ms) *gather_ms = h->letters.gather_ms;
    if (gathered_bytes) *gathered_bytes = h->letters.gathered_bytes;
    return SXG_OK;
}
extern "C" void sxg_poa_letters_geometry(int32_t* chunk_bytes) {
    if (chunk_bytes) *chunk_bytes = SXG_LETTERS_CHUNK;
}
extern "C" int sxg_poa_range_gather(sxg_poa_handle* h, const sxg_poa_letters* l, uint64_t id, int64_t n, const sxg_poa_range* r, int coded, uint8_t* out) {
    if (!h) return fail(SXG_E_INVALID, "handle is NULL");
    RoctxRange range("sxg_poa_range_gather");
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    std::vector<int64_t> len, src;
    if (int rc = letters_resolve(h, l, id, n, r, "range_gather", len, src)) return rc;
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int64_t s = 0; s < n; ++s) off[(size_t)s + 1] = off[(size_t)s] + len[(size_t)s];
    const int64_t total = off[(size_t)n];
    if (total == 0) return SXG_OK;
    if (!out) return fail(SXG_E_INVALID, "range_gather: out is NULL");
    DevBuf d_dst;
    if (int rc = d_dst.ensure((size_t)total)) return rc;
    if (int rc = letters_stage(h, src, off.data())) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    float ms = 0;
    if (int rc = timer_start(h)) return rc;
    if (int rc = letters_launch(h, n, total, h->letters.d_off.as<int64_t>(), d_dst.as<uint8_t>(), coded ? 1 : 0)) return rc;
    if (int rc = timer_stop(h, &ms)) return rc;
    if (int rc = letters_account(h)) return rc;
    HIPCHK(hipMemcpy(out, d_dst.p, (size_t)total, hipMemcpyDeviceToHost));
    h->stats.kernel_ms = ms; h->stats.dom_kernel_ms = ms; h->stats.dp_launches = 1; h->stats.dom_threads = SXG_LETTERS_THREADS;
    h->stats.device_bytes = h->letters.d.cap + h->letters.d_src.cap + h->letters.d_off.cap + d_dst.cap;
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
// The identity estimate of the adaptive scores (A14, src/smooth.cpp:1972-2069): decree Q (include/sxg_poa.h).
// Kernels in poa_identity.hip.h / kern_split.hip on the sets of poa_mash.hip.h; here the validation, the sequences that take
// part (the device sees no others), Q3's ranks, the rounds and the timing.  Memory: the sets (8 bytes per base that takes part
// + 4 per sequence) and the words of a round (8 bytes per pair) share the handle's budget -- the sort scratch of the sketch is
// bounded by it on its own, as in the split calls --; blocks go round after round, in order, as many as their words fit; a
// block whose words alone do not fit, or sets that do not, are SXG_E_NOMEM.  Everything is enqueued on the handle's stream
// without a host wait in between: the words' buffer is reused by the next round in stream order.
// Three steps: (a) validation and planning from the sequence LENGTHS; (b) the letters of the sequences that take part: uploaded
// from in->bases, or -- src != nullptr, the ranges entry point: src[s] is where sequence s starts in the resident letters and
// in->bases is not read -- cut out of the resident letters by the gather, coded; (c) the launches and the downloads.
static int block_identity_run(sxg_poa_handle* h, const sxg_poa_identity_in* in, const int64_t* src, const char* name, int32_t* n_used, int32_t* inter,
                              int32_t* uni, int32_t* status) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    const int nb = in->n_blocks;
    if (nb < 0 || (nb > 0 && (!in->blk_off || !in->seq_off || !n_used || !inter || !uni || !status))) return fail(SXG_E_INVALID, "block_identity: NULL arrays");
    const int k = in->kmer_size;
    if (k < 1 || k > 32) return fail(SXG_E_INVALID, "kmer_size must be in 1..32");
    if (in->min_len < k) return fail(SXG_E_INVALID, "min_len must be at least kmer_size");
    if (!(in->percentile >= 0.0 && in->percentile <= 1.0)) return fail(SXG_E_INVALID, "percentile must be in [0, 1]");
    if (nb > 0 && (in->blk_off[0] != 0 || in->seq_off[0] != 0)) return fail(SXG_E_INVALID, "blk_off[0] and seq_off[0] must be 0");
    for (int b = 0; b < nb; ++b)
        if (in->blk_off[b + 1] < in->blk_off[b]) return fail(SXG_E_INVALID, "blk_off not monotone");
    const int64_t ns_in = nb ? in->blk_off[nb] : 0;
    for (int64_t s = 0; s < ns_in; ++s)
        if (in->seq_off[s + 1] < in->seq_off[s]) return fail(SXG_E_INVALID, "seq_off not monotone");
    if (!src && ns_in > 0 && in->seq_off[ns_in] > 0 && !in->bases) return fail(SXG_E_INVALID, "bases is NULL");
    RoctxRange range(name);
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    // the sequences that take part, block after block: the batch the device sees (a block with one of them too long stays out)
    std::vector<int32_t> blk_off((size_t)nb + 1, 0);
    std::vector<int64_t> seq_off{0}, pair_off((size_t)nb + 1, 0), idx((size_t)std::max(nb, 1), 0);
    std::vector<uint8_t> bases;
    std::vector<int64_t> gather_src;
    if (!src) bases.reserve((size_t)(ns_in ? in->seq_off[ns_in] : 0));
    bool any_failed = false;
    int64_t max_pairs = 0;
    for (int b = 0; b < nb; ++b) {
        n_used[b] = inter[b] = uni[b] = 0;
        status[b] = SXG_ST_OK;
        int64_t used = 0;
        for (int64_t s = in->blk_off[b]; s < in->blk_off[b + 1]; ++s) {
            const int64_t len = in->seq_off[s + 1] - in->seq_off[s];
            if (len < in->min_len) continue;
            ++used;
            if (len > SXG_POA_MAX_SEQ_LEN) status[b] = SXG_ST_TOO_LONG;
        }
        if (used > 65536) return fail(SXG_E_INVALID, "block " + std::to_string(b) + ": more than 65536 sequences take part (pairs must stay below 2^31)");
        n_used[b] = (int32_t)used;
        if (status[b] != SXG_ST_OK) { any_failed = true; used = 0; }
        if (used > 1) {   // (a block with one sequence, or none, has no pair: nothing of it goes to the device)
            for (int64_t s = in->blk_off[b]; s < in->blk_off[b + 1]; ++s) {
                const int64_t o = in->seq_off[s], len = in->seq_off[s + 1] - o;
                if (len < in->min_len) continue;
                if (src) { gather_src.push_back(src[s]); seq_off.push_back(seq_off.back() + len); continue; }
                const size_t at = bases.size();
                bases.resize(at + (size_t)len);
                for (int64_t x = 0; x < len; ++x) bases[at + (size_t)x] = in->bases[o + x] > 4 ? 4 : in->bases[o + x];
                seq_off.push_back((int64_t)bases.size());
            }
            const int64_t P = used * (used - 1) / 2;
            pair_off[(size_t)b + 1] = P;
            idx[(size_t)b] = (int64_t)sxg_identity_idx((uint64_t)P, in->percentile);
            max_pairs = std::max(max_pairs, P);
        }
        blk_off[(size_t)b + 1] = (int32_t)(seq_off.size() - 1);
    }
    for (int b = 0; b < nb; ++b) pair_off[(size_t)b + 1] += pair_off[(size_t)b];
    const int64_t ns = (int64_t)seq_off.size() - 1, nbases = seq_off.back();
    if (ns > 0) {
        const uint64_t budget = arena_budget(h);
        const uint64_t sets_bytes = 8ull * (uint64_t)nbases + 4ull * (uint64_t)ns;
        if (sets_bytes + 8ull * (uint64_t)max_pairs > budget)
            return fail(SXG_E_NOMEM, "memory budget too small for the k-mer sets (" + std::to_string(sets_bytes) + " bytes) and the pairs of the deepest block (" +
                                         std::to_string(8 * max_pairs) + " bytes)");
        const int64_t words_cap = (int64_t)std::min<uint64_t>((budget - sets_bytes) / 8, 0x7fffffffull);   // (a round's pair index is an int32)
        // rounds: consecutive blocks while their words fit
        std::vector<int32_t> round_end;
        for (int b = 0, b0 = 0; b < nb; ++b) {
            if (pair_off[(size_t)b + 1] - pair_off[(size_t)b0] > words_cap) { round_end.push_back(b); b0 = b; }
            if (b + 1 == nb) round_end.push_back(nb);
        }
        int64_t round_pairs = 0;
        for (size_t r = 0, b0 = 0; r < round_end.size(); b0 = (size_t)round_end[r++]) round_pairs = std::max(round_pairs, pair_off[(size_t)round_end[r]] - pair_off[b0]);
        MashSets seqs;
        DevBuf d_blk_off, d_pair_off, d_idx, d_inter, d_uni, d_words, d_queue;
        int rc;
        if ((rc = seqs.seq_off.ensure(8 * (size_t)(ns + 1))) || (rc = seqs.bases.ensure((size_t)nbases + 16))) return rc;
        HIPCHK(hipMemcpyAsync(seqs.seq_off.p, seq_off.data(), 8 * (size_t)(ns + 1), hipMemcpyHostToDevice, h->stream));
        if (src) { if ((rc = letters_stage(h, gather_src, nullptr))) return rc; }
        else HIPCHK(hipMemcpyAsync(seqs.bases.p, bases.data(), (size_t)nbases, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if ((rc = split_up(h, d_blk_off, blk_off.data(), (size_t)nb + 1)) || (rc = split_up(h, d_pair_off, pair_off.data(), (size_t)nb + 1)) ||
            (rc = split_up(h, d_idx, idx.data(), (size_t)nb)) || (rc = d_inter.ensure(4 * (size_t)nb)) || (rc = d_uni.ensure(4 * (size_t)nb)) ||
            (rc = d_words.ensure(8 * (size_t)std::max<int64_t>(round_pairs, 1))) || (rc = d_queue.ensure(4 * round_end.size() + 256)))
            return rc;
        HIPCHK(hipMemsetAsync(d_inter.p, 0, 4 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(d_uni.p, 0, 4 * (size_t)nb, h->stream));
        HIPCHK(hipMemsetAsync(d_queue.p, 0, 4 * round_end.size(), h->stream));
        std::vector<int32_t> work((size_t)ns);   // (min_len >= k: every sequence here has a window)
        for (int64_t s = 0; s < ns; ++s) work[(size_t)s] = (int32_t)s;
        size_t dev_bytes = 0;
        int per_cu = 1;
        sxg_identity_occupancy(&per_cu);
        int64_t pair_slots = 0;
        uint64_t launches = 1;
        float ms = 0;
        if (int rc = timer_start(h)) return rc;
        if (src) {   // the taking-part ranges out of the resident letters, coded, into the layout the sketch reads
            if (int rc = letters_launch(h, ns, nbases, seqs.seq_off.as<int64_t>(), seqs.bases.as<uint8_t>(), 1)) return rc;
            ++launches;
        }
        if (int rc = mash_sketch(h, seqs, ns, seq_off.data(), work, k, false, &dev_bytes)) return rc;   // Q1: M1's sets, one launch
        for (size_t r = 0, b0 = 0; r < round_end.size(); b0 = (size_t)round_end[r++]) {
            const int32_t b1 = round_end[r];
            const int64_t n_pairs = pair_off[(size_t)b1] - pair_off[b0];
            if (n_pairs == 0) continue;
            const int64_t n_slots = std::min<int64_t>(n_pairs, (int64_t)std::max(h->num_cu, 1) * per_cu);
            pair_slots = std::max(pair_slots, n_slots);
            IdentityPairArgs A;
            A.blk_off = d_blk_off.as<int32_t>(); A.seq_off = seqs.seq_off.as<int64_t>(); A.sets = seqs.sets.as<unsigned long long>(); A.set_size = seqs.set_size.as<int32_t>();
            A.pair_off = d_pair_off.as<int64_t>(); A.b0 = (int32_t)b0; A.b1 = b1; A.n_pairs = (int32_t)n_pairs; A.queue = d_queue.as<int32_t>() + r;
            A.words = d_words.as<unsigned long long>();
            sxg_identity_launch_pairs(A, (int)n_slots, h->stream);
            HIPCHK(hipGetLastError());
            IdentitySelectArgs S;
            S.pair_off = d_pair_off.as<int64_t>(); S.idx = d_idx.as<int64_t>(); S.b0 = (int32_t)b0; S.words = d_words.as<unsigned long long>();
            S.inter = d_inter.as<int32_t>(); S.uni = d_uni.as<int32_t>();
            sxg_identity_launch_select(S, b1 - (int32_t)b0, h->stream);
            HIPCHK(hipGetLastError());
            launches += 2;
        }
        if (int rc = timer_stop(h, &ms)) return rc;
        if (int rc = letters_account(h)) return rc;
        HIPCHK(hipMemcpy(inter, d_inter.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(uni, d_uni.p, 4 * (size_t)nb, hipMemcpyDeviceToHost));
        split_stats(h, ms, 0, pair_slots, dev_bytes + d_words.cap + (src ? h->letters.d.cap + h->letters.d_src.cap : 0));
        h->stats.dp_launches = launches;   // the sketch + (pairs, select) of every round (+ the gather of a ranges call)
    }
    if (any_failed) return fail(SXG_E_BLOCK, "a block holds a sequence longer than SXG_POA_MAX_SEQ_LEN");
    return SXG_OK;
}
extern "C" int sxg_poa_block_identity_batch(sxg_poa_handle* h, const sxg_poa_identity_in* in, int32_t* n_used, int32_t* inter, int32_t* uni,
                                            int32_t* status) {
    return block_identity_run(h, in, nullptr, "sxg_poa_block_identity_batch", n_used, inter, uni, status);
}
extern "C" int sxg_poa_block_identity_ranges(sxg_poa_handle* h, const sxg_poa_identity_ranges_in* in, int32_t* n_used, int32_t* inter, int32_t* uni,
                                             int32_t* status) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    const int nb = in->n_blocks;
    if (nb < 0 || (nb > 0 && !in->blk_off)) return fail(SXG_E_INVALID, "block_identity: NULL arrays");
    if (nb > 0 && in->blk_off[0] != 0) return fail(SXG_E_INVALID, "blk_off[0] and seq_off[0] must be 0");
    for (int b = 0; b < nb; ++b)
        if (in->blk_off[b + 1] < in->blk_off[b]) return fail(SXG_E_INVALID, "blk_off not monotone");
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    const int64_t ns = nb ? in->blk_off[nb] : 0;
    std::vector<int64_t> len, src, seq_off((size_t)ns + 1, 0);
    if (int rc = letters_resolve(h, in->letters, in->letters_id, ns, in->ranges, "block_identity_ranges", len, src)) return rc;
    for (int64_t s = 0; s < ns; ++s) seq_off[(size_t)s + 1] = seq_off[(size_t)s] + len[(size_t)s];
    sxg_poa_identity_in seqs;
    memset(&seqs, 0, sizeof(seqs));
    seqs.n_blocks = nb; seqs.blk_off = in->blk_off; seqs.seq_off = seq_off.data();
    seqs.kmer_size = in->kmer_size; seqs.min_len = in->min_len; seqs.percentile = in->percentile;
    return block_identity_run(h, &seqs, src.data(), "sxg_poa_block_identity_ranges", n_used, inter, uni, status);
}

// ---------------------------------------------------------------------------------------
// The tandem-repeat scan of the cutting half of break_blocks (src/breaks.cpp:224-272): decree R (include/sxg_poa.h, DESIGN.md
// section 9).  Kernels in poa_repeat.hip.h / kern_repeat.hip on the arithmetic of poa_repeat.h; here the validation, the work items
// (largest first), the rounds and the timing.  Memory: the letters as they came, their offsets and the item list (uploaded once)
// and the counts of a round (4 bytes per lag and sequence) share the handle's budget; sequences go round after round, in order, as
// many as their counts fit; a sequence whose counts alone do not fit is SXG_E_NOMEM.  Everything is enqueued on the handle's
// stream without a host wait in between: the counts' buffer is reused by the next round in stream order.
static_assert(SXG_POA_REPEAT_MAX_LEN == SXG_REPEAT_MAX_LEN, "length limit of the header");
// Three steps: (a) validation and planning from the sequence LENGTHS; (b) the letters: uploaded from in->bases as they came, or
// -- src != nullptr, the ranges entry point: src[s] is where sequence s starts in the resident letters and in->bases is not read
// -- the sequences that are scanned cut out of the resident letters by the gather (the device's offsets then give every other
// sequence no letters; the budget's sums stay those of the lengths, so the rounds are the bases call's); (c) the launches and
// the downloads.
static int repeat_scan_run(sxg_poa_handle* h, const sxg_poa_repeat_in* in, const int64_t* src, const char* name, int32_t* n_lags, int32_t* best, double* dev,
                           double* v, int32_t* status, int32_t* match) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    const int64_t ns = in->n_seqs;
    if (ns < 0 || ns > 0x7fffffff || (ns > 0 && (!in->seq_off || !n_lags || !best || !dev || !v || !status))) return fail(SXG_E_INVALID, "repeat_scan: bad argument");
    if (in->min_copy == 0 || in->stride == 0 || in->max_copy < in->min_copy) return fail(SXG_E_INVALID, "repeat_scan: min_copy and stride must be positive and max_copy at least min_copy");
    if (ns > 0 && in->seq_off[0] != 0) return fail(SXG_E_INVALID, "seq_off[0] must be 0");
    for (int64_t s = 0; s < ns; ++s)
        if (in->seq_off[s + 1] < in->seq_off[s]) return fail(SXG_E_INVALID, "seq_off not monotone");
    const int64_t nbases = ns ? in->seq_off[ns] : 0;
    if (!src && nbases > 0 && !in->bases) return fail(SXG_E_INVALID, "bases is NULL");
    RoctxRange range(name);
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    // what the device sees is 32-bit: a stride or a max_copy beyond the length limit, clamped to it, changes no count
    const int64_t lim = SXG_REPEAT_MAX_LEN;
    const int64_t min_copy = (int64_t)std::min<uint64_t>(in->min_copy, (uint64_t)lim), max_copy = (int64_t)std::min<uint64_t>(in->max_copy, (uint64_t)lim),
                  stride = (int64_t)std::min<uint64_t>(in->stride, (uint64_t)lim);
    std::vector<int64_t> match_off((size_t)ns + 1, 0);   // of the sequences the device scans: a declined one has no counts
    std::vector<int32_t> work;
    bool any_failed = false;
    int64_t max_lags = 0;
    for (int64_t s = 0; s < ns; ++s) {
        const int64_t n = in->seq_off[s + 1] - in->seq_off[s];
        n_lags[s] = best[s] = 0; dev[s] = v[s] = 0.0;
        status[s] = SXG_ST_OK;
        int64_t lags = 0;
        if ((uint64_t)n / 2 >= in->min_copy) {   // (n < 2 min_copy: no lags, SXG_ST_OK)
            if (n > lim) { status[s] = SXG_ST_TOO_LONG; any_failed = true; }   // R4: the host scans it itself
            else { lags = sxg_repeat_n_lags(n, min_copy, max_copy); n_lags[s] = (int32_t)lags; work.push_back((int32_t)s); }
        }
        match_off[(size_t)s + 1] = match_off[(size_t)s] + lags;   // (= sxg_repeat_match_offsets: the caller's layout of `match`)
        max_lags = std::max(max_lags, lags);
    }
    if (!work.empty()) {
        // the items of every sequence, and the rounds: consecutive sequences while their counts fit
        int64_t n_items_all = 0;
        for (int32_t s : work) n_items_all += sxg_repeat_n_tiles(n_lags[s]);
        if (n_items_all > 0x3fffffff) return fail(SXG_E_INVALID, "repeat_scan: too many work items for one call");
        const uint64_t budget = arena_budget(h);
        const uint64_t fixed_bytes = (uint64_t)nbases + 16ull * (uint64_t)(ns + 1) + 8ull * (uint64_t)n_items_all + 4ull * work.size() + 20ull * (uint64_t)ns;
        if (fixed_bytes + 4ull * (uint64_t)max_lags > budget)
            return fail(SXG_E_NOMEM, "memory budget too small for the letters (" + std::to_string(fixed_bytes) + " bytes) and the counts of the longest sequence (" +
                                         std::to_string(4 * max_lags) + " bytes)");
        const int64_t counts_cap = (int64_t)((budget - fixed_bytes) / 4);
        struct round_t { size_t w0, w1; int64_t i0, i1; };
        std::vector<round_t> rounds;
        std::vector<int32_t> items;
        items.reserve(2 * (size_t)n_items_all);
        int64_t round_counts = 0;
        for (size_t w0 = 0; w0 < work.size();) {
            size_t w1 = w0;
            const int64_t base = match_off[(size_t)work[w0]];
            while (w1 < work.size() && match_off[(size_t)work[w1] + 1] - base <= counts_cap) ++w1;
            round_counts = std::max(round_counts, match_off[(size_t)work[w1 - 1] + 1] - base);
            // largest first: an item's work is the samples of its first lag times its lags
            std::vector<std::pair<int64_t, std::pair<int32_t, int32_t>>> order;
            for (size_t w = w0; w < w1; ++w) {
                const int32_t s = work[w];
                const int32_t n = (int32_t)(in->seq_off[s + 1] - in->seq_off[s]);
                for (int32_t t = 0; t < sxg_repeat_n_tiles(n_lags[s]); ++t) {
                    const int32_t k0 = t * SXG_REPEAT_TILE_LAGS;
                    order.push_back({-(int64_t)sxg_repeat_cnt(n, (int32_t)min_copy + k0, (int32_t)stride) * std::min<int32_t>(SXG_REPEAT_TILE_LAGS, n_lags[s] - k0), {s, t}});
                }
            }
            std::sort(order.begin(), order.end());
            const int64_t i0 = (int64_t)items.size() / 2;
            for (auto& o : order) { items.push_back(o.second.first); items.push_back(o.second.second); }
            rounds.push_back(round_t{w0, w1, i0, (int64_t)items.size() / 2});
            w0 = w1;
        }
        DevBuf d_bases, d_seq_off, d_match_off, d_items, d_work, d_match, d_best, d_dev, d_v;
        int rc;
        std::vector<int64_t> dev_off, gather_src;   // a ranges call: the scanned sequences back to back, and where each comes from
        if (src) {
            dev_off.assign((size_t)ns + 1, 0);
            gather_src.assign((size_t)ns, 0);
            for (int32_t s : work) { dev_off[(size_t)s + 1] = in->seq_off[s + 1] - in->seq_off[s]; gather_src[(size_t)s] = src[s]; }
            for (int64_t s = 0; s < ns; ++s) dev_off[(size_t)s + 1] += dev_off[(size_t)s];
        }
        const int64_t dev_bases = src ? dev_off[(size_t)ns] : nbases;
        const int64_t* const seq_off_up = src ? dev_off.data() : in->seq_off;
        if ((rc = d_bases.ensure((size_t)std::max<int64_t>(dev_bases, 1))) || (rc = d_seq_off.ensure(8 * (size_t)(ns + 1))) || (rc = d_match_off.ensure(8 * (size_t)(ns + 1))) ||
            (rc = d_items.ensure(4 * items.size())) || (rc = d_work.ensure(4 * work.size())) || (rc = d_match.ensure(4 * (size_t)std::max<int64_t>(round_counts, 1))) ||
            (rc = d_best.ensure(4 * (size_t)ns)) || (rc = d_dev.ensure(8 * (size_t)ns)) || (rc = d_v.ensure(8 * (size_t)ns)))
            return rc;
        if (src) { if ((rc = letters_stage(h, gather_src, nullptr))) return rc; }
        else if (nbases > 0) HIPCHK(hipMemcpyAsync(d_bases.p, in->bases, (size_t)nbases, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_seq_off.p, seq_off_up, 8 * (size_t)(ns + 1), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_match_off.p, match_off.data(), 8 * (size_t)(ns + 1), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_items.p, items.data(), 4 * items.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(d_work.p, work.data(), 4 * work.size(), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemsetAsync(d_best.p, 0, 4 * (size_t)ns, h->stream));
        HIPCHK(hipMemsetAsync(d_dev.p, 0, 8 * (size_t)ns, h->stream));
        HIPCHK(hipMemsetAsync(d_v.p, 0, 8 * (size_t)ns, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));   // (the uploads read the caller's and this frame's memory; the kernels' time starts after them)
        int per_cu = 1;
        sxg_repeat_occupancy(&per_cu);
        int64_t groups_max = 0;
        uint64_t launches = 0;
        float ms = 0;
        if (int rc = timer_start(h)) return rc;
        if (src) {   // the scanned ranges out of the resident letters, as they stand, into the layout the counting kernel reads
            if (int rc = letters_launch(h, ns, dev_bases, d_seq_off.as<int64_t>(), d_bases.as<uint8_t>(), 0)) return rc;
            ++launches;
        }
        for (const round_t& r : rounds) {
            RepeatArgs A;
            A.bases = d_bases.as<uint8_t>(); A.seq_off = d_seq_off.as<int64_t>(); A.match_off = d_match_off.as<int64_t>();
            A.match_base = match_off[(size_t)work[r.w0]]; A.match = d_match.as<int32_t>();
            A.items = d_items.as<int32_t>() + 2 * r.i0; A.n_items = (int32_t)(r.i1 - r.i0);
            A.work = d_work.as<int32_t>() + r.w0; A.n_work = (int32_t)(r.w1 - r.w0);
            A.min_copy = (int32_t)min_copy; A.max_copy = (int32_t)max_copy; A.stride = (int32_t)stride;
            A.best = d_best.as<int32_t>(); A.dev = d_dev.as<double>(); A.v = d_v.as<double>();
            const int64_t groups = std::min<int64_t>(A.n_items, (int64_t)std::max(h->num_cu, 1) * per_cu);
            groups_max = std::max(groups_max, groups);
            sxg_repeat_launch_count(A, (int)groups, h->stream);
            HIPCHK(hipGetLastError());
            sxg_repeat_launch_stats(A, h->stream);
            HIPCHK(hipGetLastError());
            launches += 2;
            if (match)   // (tests only: the round's counts, sequence by sequence before the next round overwrites them)
                for (size_t w = r.w0; w < r.w1; ++w) {
                    const int32_t s = work[w];
                    HIPCHK(hipMemcpyAsync(match + match_off[(size_t)s], d_match.as<int32_t>() + (match_off[(size_t)s] - A.match_base), 4 * (size_t)n_lags[s], hipMemcpyDeviceToHost, h->stream));
                }
        }
        if (int rc = timer_stop(h, &ms)) return rc;
        if (int rc = letters_account(h)) return rc;
        std::vector<int32_t> got_best((size_t)ns);
        std::vector<double> got_dev((size_t)ns), got_v((size_t)ns);
        HIPCHK(hipMemcpy(got_best.data(), d_best.p, 4 * (size_t)ns, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(got_dev.data(), d_dev.p, 8 * (size_t)ns, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(got_v.data(), d_v.p, 8 * (size_t)ns, hipMemcpyDeviceToHost));
        for (int32_t s : work) { best[s] = got_best[(size_t)s]; dev[s] = got_dev[(size_t)s]; v[s] = got_v[(size_t)s]; }
        h->stats.kernel_ms = ms; h->stats.dom_kernel_ms = ms; h->stats.dp_launches = launches; h->stats.n_slots = (int32_t)groups_max;
        h->stats.device_bytes = d_bases.cap + d_seq_off.cap + d_match_off.cap + d_items.cap + d_work.cap + d_match.cap + d_best.cap + d_dev.cap + d_v.cap;
        if (src) h->stats.device_bytes += h->letters.d.cap + h->letters.d_src.cap;
        h->stats.dom_threads = SXG_REPEAT_WAVE;
    }
    if (any_failed) return fail(SXG_E_BLOCK, "a sequence is longer than SXG_POA_REPEAT_MAX_LEN");
    return SXG_OK;
}
extern "C" int sxg_poa_repeat_scan_batch(sxg_poa_handle* h, const sxg_poa_repeat_in* in, int32_t* n_lags, int32_t* best, double* dev, double* v,
                                         int32_t* status, int32_t* match) {
    return repeat_scan_run(h, in, nullptr, "sxg_poa_repeat_scan_batch", n_lags, best, dev, v, status, match);
}
extern "C" int sxg_poa_repeat_scan_ranges(sxg_poa_handle* h, const sxg_poa_repeat_ranges_in* in, int32_t* n_lags, int32_t* best, double* dev, double* v,
                                          int32_t* status, int32_t* match) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    const int64_t ns = in->n_seqs;
    if (ns < 0 || ns > 0x7fffffff) return fail(SXG_E_INVALID, "repeat_scan: bad argument");
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    std::vector<int64_t> len, src, seq_off((size_t)ns + 1, 0);
    if (int rc = letters_resolve(h, in->letters, in->letters_id, ns, in->ranges, "repeat_scan_ranges", len, src)) return rc;
    for (int64_t s = 0; s < ns; ++s) seq_off[(size_t)s + 1] = seq_off[(size_t)s] + len[(size_t)s];
    sxg_poa_repeat_in seqs;
    memset(&seqs, 0, sizeof(seqs));
    seqs.n_seqs = ns; seqs.seq_off = seq_off.data(); seqs.min_copy = in->min_copy; seqs.max_copy = in->max_copy; seqs.stride = in->stride;
    return repeat_scan_run(h, &seqs, src.data(), "sxg_poa_repeat_scan_ranges", n_lags, best, dev, v, status, match);
}

// ---------------------------------------------------------------------------------------
// The path-guided SGD node order of prep (src/prep.cpp:11-163): decree Y (include/sxg_poa.h).  Kernels in
// poa_sgd.hip.h / kern_sgd.hip; here the validation, Y1's start coordinates, the choice of the path, the batch loop of the global
// path (one term launch + one apply launch per batch, on the handle's stream) and Y7's sort.
static_assert(SXG_POA_SGD_LDS_NODES == SXG_SGD_LDS_NODES, "LDS bound of the header");
extern "C" int sxg_poa_path_sgd_order(sxg_poa_handle* h, const sxg_poa_sgd_in* in, int32_t* order, int64_t* x) {
    if (!h || !in) return fail(SXG_E_INVALID, "NULL argument");
    const int64_t N = in->n_nodes, P = in->n_paths;
    if (N < 0 || P < 0 || N >= (1ll << 31) || P >= (1ll << 31)) return fail(SXG_E_INVALID, "path_sgd_order: node or path count out of range");
    if (N > 0 && (!in->node_len || !order)) return fail(SXG_E_INVALID, "path_sgd_order: node_len or order is NULL");
    if (P > 0 && !in->path_off) return fail(SXG_E_INVALID, "path_sgd_order: path_off is NULL");
    if (in->mode < 0 || in->mode > 2) return fail(SXG_E_INVALID, "path_sgd_order: mode must be 0, 1 or 2");
    if (in->iter_max < 0 || in->cooling_start < 0) return fail(SXG_E_INVALID, "path_sgd_order: negative iteration count");
    if (in->iter_max > 0 && !in->eta) return fail(SXG_E_INVALID, "path_sgd_order: eta is NULL");
    std::vector<int64_t> X((size_t)std::max<int64_t>(N, 1));
    int64_t total = 0;
    for (int64_t n = 0; n < N; ++n) {                                                   // Y1
        if (in->node_len[n] < 0) return fail(SXG_E_INVALID, "path_sgd_order: negative node length");
        X[(size_t)n] = total << SXG_SGD_SHIFT;
        total += in->node_len[n];
        if (total >= (1ll << 40)) return fail(SXG_E_INVALID, "path_sgd_order: total node length reaches 2^40");
    }
    const int64_t S = P > 0 ? in->path_off[P] : 0;
    int64_t maxsteps = 0;
    if (P > 0) {
        if (in->path_off[0] != 0) return fail(SXG_E_INVALID, "path_off[0] must be 0");
        for (int64_t p = 0; p < P; ++p) {
            if (in->path_off[p + 1] < in->path_off[p]) return fail(SXG_E_INVALID, "path_off not monotone");
            maxsteps = std::max(maxsteps, in->path_off[p + 1] - in->path_off[p]);
        }
        if (S >= (1ll << 32)) return fail(SXG_E_INVALID, "path_sgd_order: 2^32 steps or more");
        if (S > 0 && (!in->step_node || !in->step_pos)) return fail(SXG_E_INVALID, "path_sgd_order: step arrays are NULL");
        for (int64_t s = 0; s < S; ++s)
            if (in->step_node[s] < 0 || in->step_node[s] >= N || in->step_pos[s] < 0 || in->step_pos[s] >= (1ll << 41))
                return fail(SXG_E_INVALID, "path_sgd_order: step " + std::to_string(s) + " names no node or lies beyond 2^41 bp");
    }
    // mode 0 takes the LDS path when the nodes fit AND the whole sort is at most SXG_POA_SGD_LDS_TERMS terms: one workgroup in
    // one launch runs them all, and a launch should end in seconds.  Beyond that (or if the runtime refuses the dynamic LDS) the
    // choice is the global path, which gives the same bits.
    const bool few_terms = in->iter_max == 0 || in->terms_per_iter <= SXG_POA_SGD_LDS_TERMS / (uint64_t)in->iter_max;
    bool lds = in->mode == 1 || (in->mode == 0 && N <= SXG_SGD_LDS_NODES && few_terms);
    if (in->mode == 1 && N > SXG_SGD_LDS_NODES) return fail(SXG_E_INVALID, "path_sgd_order: the LDS path holds at most " + std::to_string(SXG_SGD_LDS_NODES) + " nodes");
    RoctxRange range("sxg_poa_path_sgd_order");
    HIPCHK(hipSetDevice(h->device));
    h->stats = sxg_poa_stats{};
    if (N == 0) return SXG_OK;
    const uint64_t terms = S > 0 ? in->terms_per_iter : 0;
    const uint64_t B = (uint64_t)std::max<int64_t>(1, N / 8);                           // Y6
    uint64_t launches = 0;
    if (terms > 0 && in->iter_max > 0) {
        const uint64_t batches = (terms + B - 1) / B;
        if (lds) {
            if (int e = sxg_sgd_prepare_lds(16 * (size_t)N)) {
                if (in->mode == 1) return fail(SXG_E_NODEVICE, "path_sgd_order: " + std::to_string(16 * (size_t)N) + " bytes of dynamic LDS refused (HIP error " + std::to_string(e) + ")");
                (void)hipGetLastError();
                lds = false;
            }
        }
        if (!lds && batches > (1ull << 40) / (uint64_t)in->iter_max) return fail(SXG_E_INVALID, "path_sgd_order: too many batches");
        const size_t dev_bytes = 16 * (size_t)N + 4 * (size_t)N + 8 * (size_t)(P + 1) + 12 * (size_t)S + 8 * (size_t)in->iter_max;
        if ((uint64_t)dev_bytes > arena_budget(h)) return fail(SXG_E_NOMEM, "memory budget too small for the node coordinates and the path steps");
        DevBuf d_node_len, d_path_off, d_step_node, d_step_pos, d_eta, d_X, d_D;
        int rc;
        if ((rc = split_up(h, d_node_len, in->node_len, (size_t)N)) || (rc = split_up(h, d_path_off, in->path_off, (size_t)(P + 1))) ||
            (rc = split_up(h, d_step_node, in->step_node, (size_t)S)) || (rc = split_up(h, d_step_pos, in->step_pos, (size_t)S)) ||
            (rc = split_up(h, d_eta, in->eta, (size_t)in->iter_max)) || (rc = split_up(h, d_X, X.data(), (size_t)N)) || (rc = d_D.ensure(8 * (size_t)N)))
            return rc;
        HIPCHK(hipMemsetAsync(d_D.p, 0, 8 * (size_t)N, h->stream));
        SgdArgs A;
        A.node_len = d_node_len.as<int32_t>(); A.path_off = d_path_off.as<int64_t>(); A.step_node = d_step_node.as<int32_t>(); A.step_pos = d_step_pos.as<int64_t>();
        A.eta = d_eta.as<double>(); A.X = d_X.as<unsigned long long>(); A.D = d_D.as<unsigned long long>();
        A.n_nodes = (int32_t)N; A.n_paths = (int32_t)P; A.S = (uint64_t)S; A.iter_max = in->iter_max; A.cooling_start = in->cooling_start;
        int nb = 0;
        for (uint64_t v = (uint64_t)(maxsteps - 1); v; v >>= 1) ++nb;                   // Y4: bitlength(maxsteps - 1)
        A.nb = std::max(nb, 1);
        A.terms_per_iter = terms; A.seed = in->seed; A.B = B;
        const int threads = lds ? (int)std::min<uint64_t>(1024, (std::min<uint64_t>(B, terms) + 63) / 64 * 64) : SXG_SGD_TERM_THREADS;
        float ms = 0;
        if (int rc = timer_start(h)) return rc;
        if (lds) {
            sxg_sgd_launch_lds(A, threads, 16 * (size_t)N, h->stream);
            launches = 1;
        } else {
            for (int it = 0; it < in->iter_max; ++it)
                for (uint64_t k0 = 0; k0 < terms; k0 += B) {
                    sxg_sgd_launch_terms(A, it, k0, (uint32_t)std::min<uint64_t>(B, terms - k0), h->stream);
                    sxg_sgd_launch_apply(A, h->stream);
                    launches += 2;
                }
        }
        HIPCHK(hipGetLastError());
        if (int rc = timer_stop(h, &ms)) return rc;
        HIPCHK(hipMemcpy(X.data(), d_X.p, 8 * (size_t)N, hipMemcpyDeviceToHost));
        h->stats.kernel_ms = ms; h->stats.dom_kernel_ms = ms; h->stats.dp_launches = launches; h->stats.n_slots = (int32_t)std::min<uint64_t>(launches, 0x7fffffff);
        h->stats.device_bytes = dev_bytes; h->stats.dom_threads = threads;
    }
    std::vector<int32_t> ord((size_t)N);                                                // Y7: by (X, old rank)
    for (int64_t n = 0; n < N; ++n) ord[(size_t)n] = (int32_t)n;
    std::stable_sort(ord.begin(), ord.end(), [&](int32_t a, int32_t b) { return X[(size_t)a] < X[(size_t)b]; });
    memcpy(order, ord.data(), 4 * (size_t)N);
    if (x) memcpy(x, X.data(), 8 * (size_t)N);
    return SXG_OK;
}

// ---------------------------------------------------------------------------------------
// XXH64 (published xxHash specification); dedup key of src/smooth.cpp:716.
static inline uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
extern "C" uint64_t sxg_xxh64(const void* data, uint64_t len, uint64_t seed) {
    const uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL,
                   P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
    auto rd64 = [](const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; };
    auto rd32 = [](const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; };
    auto round = [&](uint64_t acc, uint64_t in) { return rotl64(acc + in * P2, 31) * P1; };
    auto merge = [&](uint64_t hh, uint64_t v) { return (hh ^ round(0, v)) * P1 + P4; };
    const uint8_t *p = (const uint8_t*)data, *end = p + len;
    uint64_t hh;
    if (len >= 32) {
        uint64_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
        const uint8_t* lim = end - 32;
        do {
            v1 = round(v1, rd64(p)); v2 = round(v2, rd64(p + 8)); v3 = round(v3, rd64(p + 16)); v4 = round(v4, rd64(p + 24));
            p += 32;
        } while (p <= lim);
        hh = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        hh = merge(hh, v1); hh = merge(hh, v2); hh = merge(hh, v3); hh = merge(hh, v4);
    } else hh = seed + P5;
    hh += len;
    while (p + 8 <= end) { hh ^= round(0, rd64(p)); hh = rotl64(hh, 27) * P1 + P4; p += 8; }
    if (p + 4 <= end) { hh ^= (uint64_t)rd32(p) * P1; hh = rotl64(hh, 23) * P2 + P3; p += 4; }
    while (p < end) { hh ^= (*p) * P5; hh = rotl64(hh, 11) * P1; ++p; }
    hh ^= hh >> 33; hh *= P2; hh ^= hh >> 29; hh *= P3; hh ^= hh >> 32;
    return hh;
}

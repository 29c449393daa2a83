/*
 * sxg_poa.h -- C ABI of the MI355X-native blocked partial-order-alignment engine.
 *
 * Drop-in boundary for the per-block POA of pangenome/smoothxg.  The reference has no
 * plugin/FFI interface for this path; the seam is the block of spoa calls inside
 *   smooth_spoa()  src/smooth.cpp:752-786   (Create / Align / AddAlignment / consensus / MSA)
 * executed once per block by the OpenMP loop of
 *   smooth_and_lace()  src/smooth.cpp:1931-2312.
 * This library replaces that inner sequence for a whole BATCH of blocks per call:
 * everything above it (XG access, padding, dedup: src/smooth.cpp:676-743) and below it
 * (build_odgi_SPOA, unchop, lacing: src/smooth.cpp:2576-2654, 935-1010, src/main.cpp:599+)
 * stays with the caller.  INTEGRATION.md shows the binding a smoothxg maintainer adds.
 *
 * Conventions
 *   - bases are codes 0..4 = A,C,G,T,N (the XG alphabet, src/xg.cpp:24-53); >4 is read as N.
 *   - scoring uses spoa's sign convention exactly as smooth_spoa receives it
 *     (src/smooth.cpp:2098-2106): m > 0, n,g,e,q,c <= 0; mode 0 = local (kSW, default,
 *     src/main.cpp:487), 1 = global (kNW).
 *   - all functions return 0 on success or a negative SXG_E_* code; they never throw,
 *     exit() or abort() (the reference exit(1)s, src/smooth.cpp:943).  The text of the
 *     last error of the calling thread is available from sxg_poa_last_error().
 *   - every *_out struct is library-owned; release it with the matching *_free.
 *   - a handle is bound to one GPU and one HIP stream; one in-flight batch per handle.
 *     Use one handle per host thread / per rank.
 *
 * What "drop-in" does and does not promise: alignment SCORES are those of the published recurrences and are
 * checked against independent implementations; node ids, topological ranks, tie-breaks between equally good
 * alignments, the consensus and the MSA column order follow the tie rules written down in oracle/poa_oracle.c
 * (S1-S8, B1-B4), NOT necessarily spoa's / abPOA's: both are absent from the reference snapshot, so their
 * choices could not be pinned ("PARITY UNPINNED").  One divergence is KNOWN and is a switch: after
 * every AddAlignment spoa re-sorts the whole graph depth-first (node-id order, in-edge tails first, aligned siblings
 * together); with mode | SXG_ORDER_SPOA (what libsxgsmooth.so and bench.py ask for by default since round 6) the engine
 * does the same, as recollected; without it the order is kept incrementally (decree S7: new nodes are slotted next to
 * their aligned group).  Any such order is a legal POA order, but it decides ties between equally good alignments, the
 * end cell of a local alignment and the MSA column order.  Graphs are valid POA graphs of the same sequences either way --
 * every path spells its sequence -- but need not be byte-identical to the reference's.
 */
#ifndef SXG_POA_H
#define SXG_POA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (addition, no number change, no struct change): sxg_poa_letters_*, sxg_poa_range_gather, sxg_poa_repeat_scan_ranges,
 *    sxg_poa_block_identity_ranges and their structs -- a graph's path letters resident on the device, and the repeat scan and the
 *    identity estimate fed with ranges of them.
 * 5 (addition, no number change, no struct change): sxg_poa_set_long_blocks, sxg_poa_group_set_long_blocks, sxg_poa_get_tile_stats
 *    and SXG_POA_MAX_SEQ_LEN_TILED -- the 32-bit sweep in column tiles: with the switch on, one length limit for every mode.
 * 5 (addition, no number change, no struct change): sxg_poa_group_* -- one process, several GPUs: a group of handles, one host
 *    thread per member, the results reassembled in the batch's block order (trimmed MSA and block cycles included).
 * 5 (addition, no number change, no struct change): want_msa = SXG_MSA_TRIMMED -- the rows of the MAF built on the device -- and
 *    sxg_poa_get_msa_stats.
 * 5 (addition, no number change, no struct change): want_msa = SXG_MSA_TRIMMED_RESIDENT, sxg_poa_msa_row_letters and
 *    sxg_poa_maf_text (with sxg_poa_maf_seg, sxg_poa_maf_text_in, _geometry, _stats) -- the text of unmerged MAF blocks laid out on
 *    the device from the resident trimmed rows.
 * 5 (addition, no number change): sxg_poa_path_sgd_order and struct sxg_poa_sgd_in -- the path-guided SGD node order of prep
 *    (src/prep.cpp:11-163) on the device, decree Y.
 * 5 (addition, no number change: no struct or existing entry point changed): sxg_poa_repeat_scan_batch and struct
 *    sxg_poa_repeat_in -- the tandem-repeat scan of the cutting half of break_blocks (src/breaks.cpp:224-272), decree R.
 * 5 (addition, no number change): sxg_poa_kmer_jaccard_batch, sxg_poa_split_mash_batch and struct sxg_poa_split_mash -- the
 *    mash-based branch of the identity split (src/breaks.cpp:388-471) on the device, decrees M1-M5.
 * 5 (addition, no number change: no struct or existing entry point changed): sxg_poa_pair_identity_batch, sxg_poa_split_batch,
 *    sxg_poa_split_free and their two structs -- the identity split of break_blocks (src/breaks.cpp:335-586) on the device.
 * 5: sxg_poa_batch_out gained block_cycles (before _owner): per-block time on the device, the reference's POA_DEBUG column
 *    poa.time.ms (src/smooth.cpp:2121-2265); sxg_poa_sharded_timing.
 * 4: block graphs on the device: sxg_poa_batch_in gained want_block_graph / bg_consensus_visited_only / bg_trim at its END
 *    (callers must zero-initialise the struct, as before), sxg_poa_batch_out the bg_* arrays before _owner; stats.bg_ms.
 * 3: params.banded = 2 (adaptive band); sxg_poa_batch_run_sharded fails on all ranks together and needs the exchange buffer
 *    that sxg_poa_comm_init / _attach allocate; a band miss is repaired inside the engine at any length.
 * 2 (round 2, never numbered): params.reserved became params.banded -- callers must zero it --, stats.reserved became
 *    dom_clock_mhz, status 7 (SXG_ST_BAND_MISS), SXG_POA_MAX_SEQ_LEN 12287 -> 26623 with SXG_POA_MAX_SEQ_LEN_WIDE. */
#define SXG_POA_ABI_VERSION 5

#define SXG_MODE_LOCAL 0  /* spoa::AlignmentType::kSW */
#define SXG_MODE_GLOBAL 1 /* spoa::AlignmentType::kNW */
/* OR-ed into sxg_poa_params::mode: after every AddAlignment the block's graph is re-sorted depth-first the way spoa's
 * Graph::TopologicalSort is BELIEVED to do it (node-id order, in-edge tails first, aligned nodes together; restated from
 * memory -- the library is absent from the reference snapshot -- as decree S7' of oracle/poa_oracle.c) instead of being kept
 * in order incrementally (decree S7).  Both are valid POA orders; they differ in how ties between equally good alignments
 * fall.  Round 6: every thread of the block's workgroup walks its own roots and only the pieces of the order the last alignment
 * touched are walked again -- 1.01 x the kernel time on 64 x 5 kbp blocks, 1.05 x on 8000 blocks of 16 x 1 kbp; the
 * host library sets the flag by default. */
#define SXG_ORDER_SPOA 0x10
/* OR-ed into sxg_poa_params::mode, only together with SXG_ORDER_SPOA (alone: SXG_E_INVALID): the new nodes of a sequence get
 * their ids in the order spoa's Graph::AddAlignment is BELIEVED to create them (decree S6' of DESIGN.md section 2, restated
 * from memory, unverified) -- the unaligned prefix chain, then the unaligned suffix chain, then the new nodes inside the span
 * the alignment covers -- instead of in sequence order (decree S6).  Ids decide where the re-sort's walks start, hence ranks,
 * ties of later alignments and MSA columns.  Global alignments cover every position: there the flag changes nothing.  An
 * addition (no struct changed): the ABI version stays 5.  Off by default everywhere. */
#define SXG_IDS_SPOA 0x20

/* return codes */
#define SXG_OK 0
#define SXG_E_INVALID (-1)   /* bad argument */
#define SXG_E_NODEVICE (-2)  /* no usable HIP device / HIP runtime error */
#define SXG_E_NOMEM (-3)     /* device or host allocation failed */
#define SXG_E_BLOCK (-4)     /* at least one block failed; see out->status[] */
#define SXG_NOT_ROOT 1        /* sxg_poa_batch_run_sharded on a rank other than 0: its share is done, the results are on rank 0 */

/* per-block status (out->status[b]) */
#define SXG_ST_OK 0
#define SXG_ST_ROWS_OVERFLOW 1
#define SXG_ST_POOL_OVERFLOW 2
#define SXG_ST_TBX_OVERFLOW 3
#define SXG_ST_NODES_OVERFLOW 4
#define SXG_ST_TOO_LONG 5 /* a sequence exceeds SXG_POA_MAX_SEQ_LEN (local) / SXG_POA_MAX_SEQ_LEN_WIDE, or, with
                           * sxg_poa_set_long_blocks on, SXG_POA_MAX_SEQ_LEN_TILED in every mode (see below) */
#define SXG_ST_RANGE_OVERFLOW 6 /* internal: scores left the narrow sweep's range; the engine re-runs the block wider */
#define SXG_ST_INTERNAL 8       /* an internal invariant failed (e.g. the banded traceback left its band): final, please report */
#define SXG_ST_BAND_MISS 7      /* internal: the packed sweep's traceback left its band of kept cells; re-run wider */

/* Longest sequence.  Local alignment (smoothxg's default) with m * length < 30000 runs the packed int16 sweep, whose
 * largest workgroup covers 2 * 1024 * 13 columns: enough for -l 13k cut at -q 2 * 13k (src/main.cpp:376) plus padding.
 * Global alignment runs the packed sweep with m * length < 14500 whatever its gap scores (round 5: the sweep clamps far below
 * any score a related pair reaches and its traceback checks itself; a block whose walk does meet a clamped cell is re-run on
 * the 32-bit sweep).  Longer global alignments and score sets outside the int16 range (|g| or |q| > 120) need the 32-bit sweep:
 * 1024 lanes * 12 columns. */
#define SXG_POA_MAX_SEQ_LEN 26623
#define SXG_POA_MAX_SEQ_LEN_WIDE 12287
/* With sxg_poa_set_long_blocks(h, 1) (off by default) a block that no geometry of its sweep covers -- global beyond the packed
 * sweep, a walk that met a clamped cell, |g| or |q| > 120, local with m * length >= 30000, and local beyond SXG_POA_MAX_SEQ_LEN
 * whose scores the packed sweep would hold (it then runs the 32-bit sweep) -- is swept by the widest 32-bit
 * geometry in column tiles, left to right: up to 4 tiles of 12 288 columns, enough for -l 20k cut at 40k plus padding.  Below
 * this length no mode and no score set answers SXG_ST_TOO_LONG, and a global block's status no longer depends on its data.
 * The traceback plane of such a block takes rows x padded columns bytes (about 5 GB at the limit); an arena that does not fit
 * fails that block alone.  The align-only API and the split / identity entry points keep their limits. */
#define SXG_POA_MAX_SEQ_LEN_TILED 49151

/* The six scores + alignment type that smooth_spoa hands to
 * spoa::AlignmentEngine::Create (src/smooth.cpp:752-755).                                */
typedef struct sxg_poa_params {
    int8_t m, n, g, e, q, c;
    uint8_t mode;
    uint8_t banded; /* 0 = full matrix (the spoa path, smooth_spoa).
                       2 = ADAPTIVE band as the abPOA path runs it (smooth_abpoa, src/smooth.cpp:133-627: wb = 311,
                           wf = 0.03 at :266-271, `true` at :2090): the band of a graph row spans, w = 311 + (int)(0.03 L)
                           columns either side, from the leftmost to the rightmost best-scoring column of its predecessor
                           rows (+1) and the node's position counted back from the end of the graph -- abPOA's published
                           rule, restated as decree B4 of oracle/poa_oracle.c (abPOA itself is absent from the reference
                           snapshot); whole 6-, 8- or 11-column strips, at most 128 strips.
                       1 = STATIC band: w columns either side of the node's backbone coordinate (decrees B1-B3), known
                           before the sweep starts; same kernel, no per-row search of the best cell.
                       The adaptive band serves local AND global alignments (smooth_abpoa sets wb / wf for both modes,
                       src/smooth.cpp:259-271); the static band is for local mode only (a global alignment that asks for
                       it runs the full matrix, and so does a global alignment whose scores leave the packed sweep's
                       int16 range: affine defaults beyond ~3.9 kbp).  out->cells then counts band cells.
                       sxg_poa_align_batch ignores it.                                                            */
} sxg_poa_params;

/* sxg_poa_batch_in::want_msa.
 * SXG_MSA_FULL: rows = the block's sequences (+ the consensus row when want_consensus), columns = every aligned group in rank order
 *   (decree S8); formatted on the host from the per-base paths.  Any other non-zero value but SXG_MSA_TRIMMED and
 *   SXG_MSA_TRIMMED_RESIDENT means this.
 * SXG_MSA_TRIMMED (an addition to ABI 5): the rows the MAF is written from (src/smooth.cpp:791-847; the `text` fields of
 *   maf_rows_from_msa, before rows are repeated for duplicates), built on the device: in every row -- the consensus row, which
 *   comes last, included -- the first and the last bg_trim[b] letters are blanked (bg_trim NULL = 0; a row with fewer than
 *   2 * trim letters is all gaps); the columns in front of the first column that still holds a letter in any row are removed, and
 *   those behind the last such column; interior columns stay, all-gap ones too.  msa_cols[b] is the width that remains (0 if
 *   nothing remains), msa_off / msa as for the full MSA; a block whose status is not SXG_ST_OK, or without sequences, owns no
 *   bytes.  want_block_graph is NOT downgraded: with 2 or 3 seq_path_nodes stays NULL, with 3 the raw graphs too -- nothing per
 *   base crosses PCIe but the rows.  Works through sxg_poa_batch_run and upload / execute / download, for full-matrix and banded
 *   blocks and per-block params.  The sharded entry points (sxg_poa_batch_run_sharded, _upload_sharded and the test entry
 *   _run_sharded_local) refuse it with SXG_E_INVALID before any work, identically on every rank: device MSAs are not
 *   reassembled across ranks.
 *   sxg_poa_get_msa_stats: HIP-event milliseconds of the two kernels of the last execute (columns; rows) and the bytes of rows
 *   it wrote (any pointer may be NULL).  The columns and the scan scratch take 8 bytes per POA node of the batch, allocated
 *   with the handle's other result buffers (outside sxg_poa_set_memory_budget, which caps the block arenas).
 * SXG_MSA_TRIMMED_RESIDENT (an addition to ABI 5): everything SXG_MSA_TRIMMED does on the device, want_block_graph not downgraded
 *   either, but the rows do not cross PCIe: the download fills msa_off and msa_cols and leaves msa NULL.  The rows stay on the
 *   handle until its next upload, for sxg_poa_msa_row_letters and sxg_poa_maf_text (below).  The sharded entry points refuse it
 *   as they refuse SXG_MSA_TRIMMED; sxg_poa_group_batch_upload / _run refuse it with SXG_E_INVALID: the rows would lie on several
 *   members. */
#define SXG_MSA_FULL 1
#define SXG_MSA_TRIMMED 2
#define SXG_MSA_TRIMMED_RESIDENT 3

typedef struct sxg_poa_handle sxg_poa_handle;

/* A batch of blocks.  Block b owns sequences blk_off[b] .. blk_off[b+1]-1, in the order
 * they are to be aligned (smoothxg: longest first, src/blocks.cpp:206-219); sequence s owns
 * bases[seq_off[s] .. seq_off[s+1]).  weights[s] is the dedup multiplicity passed to
 * AddAlignment (src/smooth.cpp:764); NULL = all 1.                                        */
typedef struct sxg_poa_batch_in {
    int32_t n_blocks;
    const int32_t *blk_off;       /* [n_blocks+1] */
    const int64_t *seq_off;       /* [n_seqs+1]   */
    const uint8_t *bases;         /* [seq_off[n_seqs]] */
    const uint32_t *weights;      /* [n_seqs] or NULL */
    const sxg_poa_params *params; /* [n_blocks] if per_block_params else [1] */
    int32_t per_block_params;
    int32_t want_consensus; /* GenerateConsensus(), src/smooth.cpp:773 */
    int32_t want_msa;       /* GenerateMultipleSequenceAlignment(), src/smooth.cpp:785: 0, SXG_MSA_FULL or SXG_MSA_TRIMMED (below) */
    /* ABI 4.  The NORMALISED BLOCK GRAPH of every block, computed on the device right after the block's chain of
     * alignments: what smooth_spoa returns to its caller (src/smooth.cpp:931-1010) -- build_odgi_SPOA (:2576-2654: one
     * node per POA node, a path per sequence with bg_trim[b] = poa_padding steps trimmed at both ends, consensus path,
     * nodes no path visits dropped), only path-supported edges (:980-994), unchop (:935) and the topological re-numbering
     * (:947), the last two by the decrees of DESIGN.md section 9 (odgi is absent from the reference snapshot).
     *   0 = off (the caller builds block graphs from the raw POA results);
     *   1 = bg_* arrays of the result are filled in addition to the raw results;
     *   2 = ... and seq_path_nodes (one node id per base: two thirds of the download) is left out (NULL);
     *   3 = ... and the per-node / per-edge arrays of the raw POA graphs and cons_nodes as well (NULL; status, n_nodes,
     *       n_edges, the offsets, score and cells stay): for a caller that only laces block graphs (sxg_smooth_gfa).
     *   A request for the full MSA (want_msa = SXG_MSA_FULL) turns 2 and 3 into 1: that MSA is formatted from the per-base
     *   paths.  The trimmed MSA (SXG_MSA_TRIMMED) is built on the device and leaves the value as it is. */
    int32_t want_block_graph;
    int32_t bg_consensus_visited_only; /* 1 = the consensus path keeps only nodes some sequence path visits (build_odgi_abPOA,
                                          src/smooth.cpp:2542-2548); 0 = every consensus node (build_odgi_SPOA, :2624-2627) */
    const int32_t *bg_trim;            /* [n_blocks] poa_padding of every block (src/smooth.cpp:2611); NULL = 0 */
} sxg_poa_batch_in;

/* Per-block POA results, dense and block-major.  Node ids are block-local, 0-based, in
 * creation order (build_odgi_SPOA adds 1, src/smooth.cpp:2587).                            */
typedef struct sxg_poa_batch_out {
    int32_t n_blocks;
    int64_t n_seqs;
    int32_t *status;       /* [n_blocks] SXG_ST_* */
    int64_t *node_off;     /* [n_blocks+1] */
    uint8_t *node_code;    /* letter of every node */
    int32_t *node_rank;    /* topological rank inside the block */
    int32_t *node_group;   /* aligned-group leader (node id); group == MSA column class */
    int64_t *edge_off;     /* [n_blocks+1] */
    int32_t *edge_tail;    /* edges in creation order */
    int32_t *edge_head;
    uint32_t *edge_weight;
    int32_t *seq_path_nodes; /* [total bases] node of every base, indexed like in->bases;
                                replaces sequences()[i] + Successor(i), src/smooth.cpp:2604-2610 */
    int32_t *score;          /* [n_seqs] optimal alignment score of sequence s vs. the graph
                                of its predecessors (0 for the first sequence of a block)    */
    uint64_t *cells;         /* [n_seqs] DP cells = graph nodes x sequence length           */
    int64_t *cons_off;       /* [n_blocks+1] (NULL unless want_consensus) */
    int32_t *cons_nodes;     /* consensus node ids, src/smooth.cpp:2624-2637 */
    int64_t *msa_off;        /* [n_blocks+1] byte offsets into msa (NULL unless want_msa) */
    int32_t *msa_cols;       /* [n_blocks] columns; rows = #seqs (+1 consensus row if wanted) */
    char *msa;               /* row-major 'A','C','G','T','N','-' (GAP_CHAR, src/smooth.cpp:8-11) */
    /* Block graphs (in->want_block_graph; NULL otherwise).  Node ids are block-local, 0-based, in the block graph's final
     * order -- topological: Kahn over the edges, smallest id first (decree of DESIGN.md section 9) --, so every edge runs
     * forward-to-forward from a lower to a higher id and the edges listed per tail, heads ascending, ARE the L lines of
     * the block graph in their order.  A path per (dedup'd) input sequence in the orientation it was aligned in: the caller
     * reverses + flips it for ranges it collected in reverse (src/smooth.cpp:2612-2615) and repeats it for duplicates
     * (:2598-2602).  A failed block has no nodes. */
    int64_t *bg_node_off;     /* [n_blocks+1] */
    int32_t *bg_node_len;     /* [nodes] bases of every node */
    int32_t *bg_node_outdeg;  /* [nodes] out-degree: the edges of the nodes follow one another in bg_edge_to (CSR order) */
    uint8_t *bg_node_indeg;   /* [nodes] in-degree, saturating at 255 */
    int64_t *bg_seq_off;      /* [n_blocks+1] where the block's node sequences start in bg_seq */
    char *bg_seq;             /* node sequences back to back in node order, 'A','C','G','T','N' */
    int64_t *bg_edge_off;     /* [n_blocks+1] */
    int32_t *bg_edge_to;      /* [edges] head of every edge, ascending per tail */
    int64_t *bg_step_off;     /* [n_seqs+1] */
    int32_t *bg_steps;        /* node id of every step of every sequence path */
    int64_t *bg_cons_off;     /* [n_blocks+1] (NULL unless want_consensus) */
    int32_t *bg_cons_steps;   /* steps of the consensus path */
    /* Per-block time on the device (what the reference's -DPOA_DEBUG build tabulates per block as poa.time.ms,
     * src/smooth.cpp:2121-2265, 2319-2350): shader-clock cycles between the moment a slot took the block and the moment it
     * wrote the block's status -- every alignment, traceback and graph update of the block, in its LAST run (a block that
     * was re-run on a larger arena or a wider sweep reports that run).  Milliseconds = cycles / (stats.dom_clock_mhz * 1e3).
     * NULL in the results of a sharded run (the peers' blobs do not carry it). */
    uint64_t *block_cycles;   /* [n_blocks] */
    void *_owner;
} sxg_poa_batch_out;

/* Stand-alone Align(sequence, graph) problems (src/smooth.cpp:761).  Graph p is given in
 * topological order: row r of problem p is global row row_off[p]+r; its predecessors are
 * preds[pred_off[R] .. pred_off[R+1]) as 1-based row numbers LOCAL to the problem (rank+1),
 * in edge-insertion order; an empty list means "source".                                   */
typedef struct sxg_poa_align_in {
    int32_t n;
    const int64_t *row_off;  /* [n+1] */
    const uint8_t *row_code; /* [rows] */
    const uint8_t *row_sink; /* [rows] 1 = node has no out-edge */
    const int64_t *pred_off; /* [rows+1] */
    const int32_t *preds;
    const int64_t *seq_off; /* [n+1] */
    const uint8_t *bases;
    const sxg_poa_params *params;
    int32_t per_problem_params;
} sxg_poa_align_in;

/* Alignment p = pairs pair_off[p]..pair_off[p+1]: (row | -1, sequence position | -1) in
 * forward order -- spoa::Alignment with ranks in place of node ids.                         */
typedef struct sxg_poa_align_out {
    int32_t n;
    int32_t *status;
    int32_t *score;
    int64_t *pair_off;
    int32_t *pair_row;
    int32_t *pair_pos;
    void *_owner;
} sxg_poa_align_out;

/* Timing / accounting of the last execute on a handle. */
typedef struct sxg_poa_stats {
    double kernel_ms;     /* HIP-event time of the POA kernels on the handle's stream */
    uint64_t cells;       /* DP cells evaluated */
    uint64_t dp_launches; /* number of POA kernel launches */
    uint64_t algo_bytes;  /* algorithmic bytes (2*n_cross*sizeof(score)+1 per cell) */
    int32_t n_slots;      /* resident workgroups used */
    int32_t retries;      /* blocks re-run with a larger arena */
    uint64_t device_bytes;/* device memory of the block arenas */
    /* the dominant launch (most cells) of the last execute: what bench.py's roofline quotes */
    double dom_kernel_ms;
    uint64_t dom_cells, dom_algo_bytes;
    int32_t dom_threads, dom_cols_per_lane; /* launch geometry */
    int32_t dom_row_mode;  /* 0/1 = 32-bit sweep (int16 / int32 row words), 2 = packed-int16 sweep, 3 = banded packed sweep */
    int32_t dom_clock_mhz; /* shader clock that launch ran at (cycles of its slots / their 100 MHz wall ticks); 0 = unknown */
    double bg_ms;          /* HIP-event time of the block-graph kernel (want_block_graph), not part of kernel_ms */
} sxg_poa_stats;

/* Packed sweep, strip width per alignment (the classes with a second width W2 = W - 1 run every alignment whose sequence fits
 * T * 2 * W2 columns in strips of W2 columns; SXG_POA_WIDTH2=0 switches that off): what the sweeps of the last execute ran at,
 * summed over its launches from the slots' counters.  Index 0: the geometry's width W, 1: the second width.  A repeated sweep
 * (hint shift after a band miss) counts again. */
typedef struct sxg_poa_width_stats {
    uint64_t sweeps[2];       /* sweeps (alignments and their repeats) */
    uint64_t swept_cols[2];   /* columns of those sweeps' geometries, T * 2 * width each */
    uint64_t swept_cells[2];  /* graph rows x columns of those sweeps */
    uint64_t hint_shift_repeats; /* sweeps repeated inside the kernel with shifted hints */
    int32_t dom_width, dom_width2; /* strip widths of the dominant launch (dom_width2 = 0: one width only) */
} sxg_poa_width_stats;

/* Packed sweep, twin step (the classes of three waves and more with 2-byte cells sweep two consecutive rows with the same
 * single predecessor in one step, and the row that joins them takes their maxima out of the registers; SXG_POA_TWIN=0 switches
 * that off): the rows the last execute prepared that way, summed over its launches from the slots' counters. */
typedef struct sxg_poa_twin_stats {
    uint64_t twin_steps;  /* pairs of rows swept in one step */
    uint64_t join_rows;   /* rows that took both rows of the pair in front of them from registers */
} sxg_poa_twin_stats;

int sxg_poa_abi_version(void);
/* Measurement aids (no counterpart in the reference; SURVEY sections 5 and 8d).
 * _measure_copy: a streaming device-to-device copy of `bytes` bytes on this engine's device and stream, timed with HIP events over
 *   `reps` launches: *gbps = (bytes read + bytes written) / time.  The figure bench.py prints beside the data sheet's HBM peak.
 * _roctx_available: 1 when a ROCTx marker library was found -- _upload / _execute / _download and the pack / exchange halves of
 *   _execute_sharded then run inside named ranges (rocprofv3 --marker-trace); 0: the ranges are no-ops. */
int sxg_poa_measure_copy(sxg_poa_handle *h, uint64_t bytes, int reps, double *gbps);
int sxg_poa_roctx_available(void);
int sxg_poa_device_count(void);
/* compute units of the engine's device: what the launch plan deals workgroups over (a round whose packed launches ask for at
 * least one workgroup per unit runs neighbouring strip widths as one launch); -1: no handle */
int sxg_poa_compute_units(sxg_poa_handle *h);
const char *sxg_poa_last_error(void);

int sxg_poa_create(int device, sxg_poa_handle **out);
void sxg_poa_destroy(sxg_poa_handle *h);

/* One-shot: upload, run, download. */
int sxg_poa_batch_run(sxg_poa_handle *h, const sxg_poa_batch_in *in, sxg_poa_batch_out *out);
/* Staged form (what bench.py times): inputs become resident in HBM with _upload; _execute
 * runs the whole batch on the device and leaves results in HBM; _download copies them out. */
int sxg_poa_batch_upload(sxg_poa_handle *h, const sxg_poa_batch_in *in);
int sxg_poa_batch_execute(sxg_poa_handle *h);
int sxg_poa_batch_download(sxg_poa_handle *h, sxg_poa_batch_out *out);
void sxg_poa_batch_free(sxg_poa_batch_out *out);

/* Zero-copy view of the executed batch's results in HBM (valid until the next upload on this
 * handle): what a caller hands to RCCL to reassemble the per-block graphs across GPUs before
 * lacing (src/main.cpp:599+) without a host round trip.  Node/edge arrays use the worst-case
 * layout: block b's entries start at index seq_off[blk_off[b]].                              */
typedef struct sxg_poa_device_view {
    int32_t n_blocks;
    int64_t n_seqs, n_bases;
    const int32_t *status, *n_nodes, *n_edges;           /* [n_blocks] */
    const uint8_t *node_code;                            /* [n_bases] worst-case layout */
    const int32_t *node_rank, *node_group;               /* [n_bases] */
    const int32_t *edge_tail, *edge_head;                /* [n_bases] */
    const uint32_t *edge_weight;                         /* [n_bases] */
    const int32_t *seq_path_nodes;                       /* [n_bases] dense */
    const int32_t *score;                                /* [n_seqs] */
} sxg_poa_device_view;
int sxg_poa_batch_device_view(sxg_poa_handle *h, sxg_poa_device_view *out);

/* Multi-GPU, one handle (= one GPU) per rank.  Blocks are independent (src/smooth.cpp:1931): every rank aligns its
 * share and the only exchange is the reassembly of the results on the rank that laces (src/main.cpp:599+), over
 * RCCL/xGMI.  The communicator is either created here from an id that rank 0 generated and handed to the others
 * (any side channel: MPI, a file, torch.distributed), or a ncclComm_t the caller already owns.
 * sxg_poa_batch_run_sharded is sxg_poa_batch_run for that communicator: EVERY rank calls it with the SAME batch;
 * blocks are dealt by cost (longest first onto the least loaded rank), results travel to rank 0 as one blob per
 * peer (exact size, grouped ncclSend/ncclRecv) and rank 0 returns them in the batch's block order.  Other ranks
 * return SXG_NOT_ROOT with an empty result.  Without a communicator it equals sxg_poa_batch_run. */
#define SXG_POA_COMM_ID_BYTES 128
int sxg_poa_comm_unique_id(uint8_t *id);                                   /* ncclGetUniqueId (rank 0) */
int sxg_poa_comm_init(sxg_poa_handle *h, const uint8_t *id, int nranks, int rank);
int sxg_poa_comm_attach(sxg_poa_handle *h, void *nccl_comm, int nranks, int rank); /* caller-owned ncclComm_t */
void sxg_poa_comm_destroy(sxg_poa_handle *h);
int sxg_poa_batch_run_sharded(sxg_poa_handle *h, const sxg_poa_batch_in *in, sxg_poa_batch_out *out);
/* The same in three stages (sxg_poa_batch_run_sharded = upload + execute + download), for callers that keep the inputs
 * resident or cut the shares themselves:
 *   _upload_sharded    every rank, SAME batch: deals the blocks by cost and uploads this rank's share;
 *   _execute_sharded   every rank (collective): aligns the uploaded share -- dealt above, or uploaded by the caller with
 *                      sxg_poa_batch_upload --, packs the results into one device blob, all-gathers the blob sizes and sends
 *                      every blob to rank 0 (grouped ncclSend/ncclRecv).  A failure on one rank is returned by ALL ranks;
 *                      a collective that does not complete within SXG_POA_COMM_TIMEOUT_S seconds (default 600) aborts the
 *                      communicator and returns SXG_E_NODEVICE instead of hanging;
 *   _download_sharded  rank 0: the results of all ranks in the batch's block order (needs the deal of _upload_sharded);
 *                      other ranks: SXG_NOT_ROOT.
 * sxg_poa_sharded_info: ranks whose counts arrived in the last exchange and bytes rank 0 received from its peers. */
int sxg_poa_batch_upload_sharded(sxg_poa_handle *h, const sxg_poa_batch_in *in);
int sxg_poa_batch_execute_sharded(sxg_poa_handle *h);
int sxg_poa_batch_download_sharded(sxg_poa_handle *h, const sxg_poa_batch_in *in, sxg_poa_batch_out *out);
int sxg_poa_sharded_info(sxg_poa_handle *h, int32_t *ranks_seen, uint64_t *bytes_received);
/* Host-clock milliseconds of the last _execute_sharded on this rank: packing its results into one device blob, and the
 * exchange (two size all-gathers + the blobs to rank 0; includes waiting for the slowest rank to finish its share). */
int sxg_poa_sharded_timing(sxg_poa_handle *h, double *pack_ms, double *exchange_ms);
/* Test entry: the same partition / packing / assembly with `nranks` simulated ranks on this one GPU. */
int sxg_poa_batch_run_sharded_local(sxg_poa_handle *h, const sxg_poa_batch_in *in, int nranks, sxg_poa_batch_out *out);

/* Device group (an addition to ABI 5): ONE process, several GPUs, every result reassembled.  A group owns one engine handle
 * per entry of `devices` (1 <= n <= 16, each an existing device; anything else is SXG_E_INVALID).  The SAME device id may
 * appear more than once: every entry is an independent handle with its own streams and arenas, so a group of {0, 0} runs --
 * and is tested -- on a machine with one GPU (it shows that members coexist, not a speed-up).  There is no communicator, no
 * rank, no collective, no timeout and no SXG_NOT_ROOT.
 *   Deal: a function of the batch alone (smoothxg_amd/csrc/poa_deal.h): the prefix sum of the blocks' cost -- the cost the
 *     sharded deal uses -- is cut at total * k / n, member k runs the contiguous slice of blocks that START in its window.  A
 *     member carries at most total / n plus one block; a group with more members than blocks has empty members.
 *   Run: one host thread per member with work, each on its member's device; upload, execute and download of a member run on
 *     that member's streams at the same time as the others'; every thread is joined before a call returns, on success and on
 *     failure.  SXG_POA_GROUP_SERIAL=1 runs the members one after the other on the calling thread (A/B runs, debugging).
 *   Memory: sxg_poa_group_set_memory_budget sets the arena cap of every member.  The default cap of a handle (3/4 of its
 *     device's free memory) is divided by the number of members on the same device, so that members which share a device do
 *     not starve each other.
 *   Result: everything sxg_poa_batch_run returns for the same input, in the batch's block order and byte for byte the same
 *     arrays, for any n, any order of `devices`, concurrent or serial: statuses, scores, cells, raw graphs, per-base paths,
 *     consensus, the full and the TRIMMED MSA (msa_off, msa_cols, msa), block graphs at want_block_graph 1, 2 and 3 (the rule
 *     that a full MSA turns 2 and 3 into 1 applies unchanged), per-block params; block_cycles is present, one entry per block
 *     (timings: not comparable between runs).  Every member downloads its slice as a single handle would; the slices are
 *     copied into place by one thread per member and only the offsets are rebased.  Release with sxg_poa_batch_free.
 *   Errors: a failed block sets status[b] and the call returns SXG_E_BLOCK with every other block complete, as
 *     sxg_poa_batch_run does.  A member that fails as a whole (SXG_E_NOMEM, SXG_E_NODEVICE, ...) makes the call return that
 *     code after all threads have joined, with `out` zeroed; the caller's thread then reads "group member <i> (device <d>)
 *     failed in <stage>: <the member's message>" from the error text.
 * sxg_poa_group_batch_run has the signature of the host library's provider (sxg_poa_run_fn) with the group as ctx;
 * _upload / _execute / _download are its stages (_execute is repeatable).  sxg_poa_group_member returns member i (NULL out of
 * range), owned by the group: for its stats and for the split, identity and SGD calls, which stay single-device.
 * sxg_poa_group_timing, after a download: member_ms[n] host-clock milliseconds of every member's last execute + download (0
 * for a member without blocks), pack_ms the longest member download (the device-side compaction of its arrays and their copy
 * to the host), assemble_ms the reassembly on the host; any pointer may be NULL. */
typedef struct sxg_poa_group sxg_poa_group;
int sxg_poa_group_create(const int32_t *devices, int32_t n, sxg_poa_group **out);
void sxg_poa_group_destroy(sxg_poa_group *g);
int sxg_poa_group_size(const sxg_poa_group *g);
sxg_poa_handle *sxg_poa_group_member(sxg_poa_group *g, int32_t i);
int sxg_poa_group_set_memory_budget(sxg_poa_group *g, uint64_t bytes_per_member);
int sxg_poa_group_set_long_blocks(sxg_poa_group *g, int on); /* sxg_poa_set_long_blocks on every member */
int sxg_poa_group_batch_run(sxg_poa_group *g, const sxg_poa_batch_in *in, sxg_poa_batch_out *out);
int sxg_poa_group_batch_upload(sxg_poa_group *g, const sxg_poa_batch_in *in);
int sxg_poa_group_batch_execute(sxg_poa_group *g);
int sxg_poa_group_batch_download(sxg_poa_group *g, sxg_poa_batch_out *out);
int sxg_poa_group_timing(sxg_poa_group *g, double *member_ms, double *pack_ms, double *assemble_ms);

/* sxg_poa_stats after the call: dp_launches, kernel_ms and n_slots of its launches (one per geometry, gap model and alignment
 * mode), dom_threads / dom_cols_per_lane / dom_row_mode / dom_kernel_ms of the launch with the most rows x letters. */
int sxg_poa_align_batch(sxg_poa_handle *h, const sxg_poa_align_in *in, sxg_poa_align_out *out);
void sxg_poa_align_free(sxg_poa_align_out *out);

/* The identity split of break_blocks (src/breaks.cpp:335-586; -I / --block-id-min, -R / --block-ratio-min), decrees P1-P4
 * of DESIGN.md section 9.  WFA, the aligner the reference calls there, is absent from the snapshot (deps/WFA is empty), so the
 * pair identity is restated as an OPTIMUM, with no tie-break to pin:
 *   P1  a global alignment of a and b is a string of columns: diagonal (match / mismatch), I (consumes a), D (consumes b).  Its
 *       cost is the triple (penalty, cols, nonmatch): penalty = 7 per mismatch + (11 + k) per gap of k bases, a switch between I
 *       and D opening a new gap (the reference's penalties 0/7/11/1); cols = matches + mismatches + maximal runs of consecutive
 *       gap columns, I and D mixed counting as ONE run (wfa_gap_compressed_identity, src/breaks.cpp:72-102); nonmatch =
 *       mismatches + those runs.  The pair's result is the lexicographically smallest triple over all alignments;
 *       matches = cols - nonmatch, identity = (double)matches / (double)cols.  N is a letter like any other.
 *   P2  with cap given per pair (the reference: max_score = curr_len, :491-500): an optimal penalty >= cap means "no identity",
 *       reported as cols = matches = 0 (penalty is still the optimum).  The reference's REDUCED wavefront (a heuristic that may
 *       miss the optimum) is not restated: the optimum here is exact.
 *   P3  sxg_poa_split_batch runs the greedy of :414-528 for every block, statement by statement: block b holds its dedup'd
 *       sequences sorted by (length, letters); sequence 0 seeds group 0; every later sequence i is tried forward then reverse-
 *       complemented, against the groups last to first, against each group's members last to first, and joins the group of the
 *       first member with (double)matches / (double)cols >= identity[b] (IEEE double, cap = the length of i); a group's member
 *       loop is left at the first member with (double)other_len / (double)curr_len < length_ratio_min[b] or with
 *       other_len < curr_len && other_len < (uint64)(identity / (1 - identity)) ("always" at identity 1); a sequence that
 *       joins nobody opens a new group.
 *   P4  the mash-based branch (:388-471, the CLI's default at a dedup depth >= 12000) is sxg_poa_split_mash_batch below, decrees
 *       M1-M5; sxg_poa_split_batch is the walk without it.
 * One wavefront per pair / one persistent wavefront per block; the scratch comes out of the handle's memory budget; both calls run
 * inside ROCTx ranges and fill kernel_ms / cells / n_slots / dp_launches of sxg_poa_stats. */
#define SXG_POA_SPLIT_PANEL 512 /* columns a wavefront sweeps at once; longer second sequences run panel after panel */
/* n_pairs pairs over one flat sequence set: pair k aligns sequence pair_a[k] with sequence pair_b[k], the latter reverse-
 * complemented where b_rev[k] (NULL = none), with bound cap[k].  Results go to the caller's arrays [n_pairs].  A zero-length
 * sequence or one longer than SXG_POA_MAX_SEQ_LEN in a pair is SXG_E_INVALID. */
int sxg_poa_pair_identity_batch(sxg_poa_handle *h, int64_t n_seqs, const int64_t *seq_off, const uint8_t *bases, int64_t n_pairs,
                                const int32_t *pair_a, const int32_t *pair_b, const uint8_t *b_rev, const int32_t *cap,
                                int32_t *penalty, int32_t *cols, int32_t *matches);
typedef struct sxg_poa_split_in {
    int32_t n_blocks;
    const int32_t *blk_off;          /* [n_blocks+1] */
    const int64_t *seq_off;          /* [n_seqs+1] */
    const uint8_t *bases;            /* dedup'd sequences of every block, sorted by (length, letters) */
    const double *identity;          /* [n_blocks] block_group_identity, 0 < t <= 1 */
    const double *length_ratio_min;  /* [n_blocks] */
} sxg_poa_split_in;
typedef struct sxg_poa_split_out {
    int32_t n_blocks;
    int64_t n_seqs;
    int32_t *group;    /* [n_seqs] group of every sequence, 0-based in order of creation (0 for a failed block) */
    int32_t *n_groups; /* [n_blocks] (0 for a failed or empty block) */
    int64_t *n_pairs;  /* [n_blocks] pair alignments the block's greedy ran */
    int32_t *status;   /* [n_blocks] SXG_ST_OK, or SXG_ST_TOO_LONG: a sequence exceeds SXG_POA_MAX_SEQ_LEN */
    void *_owner;
} sxg_poa_split_out;
/* Returns SXG_E_BLOCK when some block failed (the others are valid), SXG_E_INVALID for a zero-length sequence. */
int sxg_poa_split_batch(sxg_poa_handle *h, const sxg_poa_split_in *in, sxg_poa_split_out *out);
void sxg_poa_split_free(sxg_poa_split_out *out);

/* The mash-based branch of that split (src/breaks.cpp:388-471; -D / -L / -e / -k of src/main.cpp:102-112,302-320), decrees M1-M5
 * of DESIGN.md section 9.  mkmh / rkmh are absent from the snapshot, so the sketch is fixed by decree:
 *   M1  K(s, k) is the set of distinct canonical k-mers of s: 2 bits per letter, 1 <= k <= 32, the smaller of the forward value
 *       and the value of the reverse complement; a window with an N (code 4) contributes nothing.  A sequence shorter than
 *       min_len has the empty set.  |K| stands for seq_hashes[i].size().
 *   M2  block b runs the mash rules iff min_len[b] > 0 (the caller applies the depth test of :388-390); min_len[b] >= k.
 *   M3  two thresholds, computed on the host in double: f = v / (2 - v), v = exp(-(1 - t) k) with t = identity[b], and
 *       jmin = w / (2 - w), w = exp(-(1 - e) k) with e = est_identity[b]; "1 - dist >= e" with dist = -ln(2J / (1 + J)) / k is
 *       J >= jmin.
 *   M4  P3's loops.  For sequence i, size_thr = (uint64)((double)|K_i| * f).  After the length-ratio break a pair with
 *       curr_len >= min_len and other_len >= min_len is ELIGIBLE: in the forward pass, |K_other| < size_thr leaves the member
 *       loop; otherwise one comparison is counted in n_mash, inter = |K_i n K_other|, uni = |K_i| + |K_other| - inter, and i
 *       joins iff uni > 0 && (double)inter / (double)uni >= jmin; in the reverse-complement pass an eligible pair does nothing
 *       and the walk goes on.  Any other pair takes P3's path unchanged (early exit, alignment, n_pairs).
 *   M5  identity in (0, 1] as for sxg_poa_split_batch, est_identity in (0, 1], min_len 0 or >= k: anything else is SXG_E_INVALID.
 * One workgroup per sequence builds, sorts (tiles of SXG_POA_MASH_SORT_TILE keys in LDS, merged in HBM) and de-duplicates the
 * sets; one wavefront intersects two of them by a merge-path partition; one persistent wavefront per block walks M4.
 * sxg_poa_stats after these calls: kernel_ms is the sum of the kernels, cells the cells of the alignments run, device_bytes the
 * scratch including the sets. */
#define SXG_POA_MASH_SORT_TILE 1024 /* keys sorted on chip at once; longer sequences merge tiles in device memory */
/* Sets and intersections, for callers and tests: set_size[n_seqs] = |K(s, k)| of every sequence (no min_len here; a sequence
 * longer than SXG_POA_MAX_SEQ_LEN is SXG_E_INVALID), inter[n_pairs] = |K(a) n K(b)|; kmers: NULL, or [seq_off[n_seqs]] -- the
 * sorted set of sequence s at kmers + seq_off[s], the rest of its stretch zero. */
int sxg_poa_kmer_jaccard_batch(sxg_poa_handle *h, int64_t n_seqs, const int64_t *seq_off, const uint8_t *bases, int32_t kmer_size,
                               int64_t n_pairs, const int32_t *pair_a, const int32_t *pair_b,
                               int32_t *set_size, int32_t *inter, uint64_t *kmers);
typedef struct sxg_poa_split_mash {
    int32_t kmer_size;
    const int32_t *min_len;       /* [n_blocks] 0 = this block runs P3 only */
    const double *est_identity;   /* [n_blocks] in (0, 1] */
} sxg_poa_split_mash;
/* sxg_poa_split_batch's contract plus M1-M5; n_mash: [n_blocks] set comparisons run, or NULL; out is freed by sxg_poa_split_free */
int sxg_poa_split_mash_batch(sxg_poa_handle *h, const sxg_poa_split_in *in, const sxg_poa_split_mash *mash,
                             sxg_poa_split_out *out, int64_t *n_mash);

/* The identity estimate of the adaptive scores (-a; A14, src/smooth.cpp:1972-2069) for every block of a batch, decree Q of
 * DESIGN.md section 9 (an addition to ABI 5).  The estimate itself is include/sxg_smooth.h's (sxg_block_identity_threshold: exact
 * Jaccard of canonical k-mer sets -> mash distance -> the 30 % percentile of the sorted pair identities, floored at 0.7); this
 * call computes it without a logarithm and without a float, in exact integers:
 *   Q1  the sets are M1's (2 bits per letter, 1 <= k <= 32, a window with code 4 contributes nothing), built by the sketch kernel
 *       of the mash split.  A sequence of block b takes part iff its length is at least min_len (the caller passes 8 * k);
 *       n_used[b] counts them; the letters arrive coded (0..3, anything else = 4: the caller codes either case of A C G T).
 *   Q2  for every pair i < j of a block's taking-part sequences: inter = |K_i n K_j|, uni = |K_i| + |K_j| - inter, and the pair's
 *       key is uni ? ((uint64)inter << 32) / uni : 0.  Sequences are at most SXG_POA_MAX_SEQ_LEN long, so uni < 2^16, two different
 *       J = inter / uni differ by more than 2^-32, and the key order is exactly the order of J; equal keys mean equal J.
 *   Q3  with P = n_used (n_used - 1) / 2 and idx = (size_t)((double)(P - 1) * percentile), computed on the host in double, block b
 *       returns (inter[b], uni[b]) of a pair whose key is the idx-th smallest (0-based) of its P keys.  Which pair among those of
 *       equal J is unspecified (equal J give the same float); it is the same from run to run.
 *   Q4  the pair identity f(J) = (float)(1 - (-ln(2J / (1 + J)) / k)) (0 at J = 0) is non-decreasing in J for J > 0, and the pairs
 *       with f <= 0 -- J = 0, and very small J at small k -- are a lower set in both orders, every one of which ends at the floor;
 *       so max(0.7f, f(J of the idx-th key)) is max(0.7f, sorted f [idx]), bit for bit.
 *   Q5  the float is computed once per block, by the host library, from (inter, uni): identity_from_counts of sxg_smooth.cpp, the
 *       expression its own all-pairs estimator uses.
 * One workgroup per sequence builds the sets (ONE launch for the batch); one wavefront per pair -- the pairs are enumerated on the
 * device from per-block prefix sums, the host sends no pair lists -- intersects two sets by the merge-path partition of the mash
 * split and writes one word (key << 16 | uni); one workgroup per block finds the idx-th smallest word by a radix select over LDS
 * histograms (no sort; deterministic).  The sets (8 bytes per taking-part base) and the words (8 bytes per pair) come out of the
 * handle's memory budget: blocks run in rounds, in order, as many as their words fit beside the sets; sets that do not fit, or a
 * single block whose words do not, are SXG_E_NOMEM (a block of the depth cap, 1000 ranges, needs 4 MB of words).
 * SXG_E_INVALID: kmer_size outside 1..32, min_len < kmer_size, a percentile outside [0, 1], more than 65536 taking-part
 * sequences in a block.  A block with a taking-part sequence longer than SXG_POA_MAX_SEQ_LEN gets SXG_ST_TOO_LONG (inter = uni =
 * 0) and the call returns SXG_E_BLOCK, the other blocks being valid.  Empty blocks and blocks with n_used <= 1 are SXG_ST_OK with
 * inter = uni = 0.  The call runs inside a ROCTx range; sxg_poa_stats after it: kernel_ms the sum of the kernels, dp_launches
 * their number (1 + 2 per round), n_slots the wavefronts of the widest pairs launch, device_bytes the sets, the sort scratch and
 * the words. */
typedef struct sxg_poa_identity_in {
    int32_t n_blocks; const int32_t *blk_off; const int64_t *seq_off; const uint8_t *bases; /* codes 0..3, 4 = other */
    int32_t kmer_size;   /* 1..32 */
    int32_t min_len;     /* shorter sequences take no part (the caller passes 8 * k); >= kmer_size */
    double percentile;   /* 0.30 */
} sxg_poa_identity_in;
/* caller-allocated [n_blocks] each */
int sxg_poa_block_identity_batch(sxg_poa_handle *h, const sxg_poa_identity_in *in,
                                 int32_t *n_used, int32_t *inter, int32_t *uni, int32_t *status);

/* The tandem-repeat scan of the cutting half of break_blocks (src/breaks.cpp:224-272) for every sequence of a batch, decree R of
 * DESIGN.md section 9 (an addition to ABI 5, no struct changed).  The scan itself is include/sxg_smooth.h's (the stand-in for
 * sautocorr::repeat, itself a decree: match-fraction autocorrelation over sampled positions, z-score across the lags); this call
 * computes it in exact integers plus one short double-precision pass whose every operation is pinned:
 *   R1  letters are the bytes as they stand in the graph, compared for equality only: case matters and N == N, as on the host.
 *   R2  a sequence of n bytes with n >= 2 min_copy has the lags L = min_copy ... hi, hi = min(max_copy, n - min_copy), n_lags =
 *       hi - min_copy + 1; match(L) = #{ i = 0, stride, 2 stride, ... < n - L : s[i] == s[i + L] }, cnt(L) = ceil((n - L) / stride).
 *       The device produces match as 32-bit integers; nothing about the counts is approximate or depends on an order.
 *   R3  a second kernel finishes each sequence in IEEE double, sums in lag order k = 0 ... n_lags - 1, one rounding per operation
 *       (its translation unit is built without contraction): r[k] = (double)match / (double)cnt; mean = (sum of r[k], from 0.0) /
 *       n_lags; var = sum of (r[k] - mean) * (r[k] - mean); it returns best = the first k of the greatest r[k], dev = r[best] -
 *       mean and v = var / n_lags.  The host does the three operations that remain: sd = sqrt(v); sd == 0 means no repeat; a
 *       repeat of length min_copy + best is reported iff dev / sd >= min_z -- the host scan's own operations on best (one
 *       function of smoothxg_amd/csrc/poa_repeat.h, sxg_repeat_decide, serves both).
 *   R4  "first lag of greatest r" is the host scan's "first lag of greatest z", z[k] = (r[k] - mean) / sd: rounding is monotone,
 *       so z is non-decreasing in r, and the two can differ only if two DIFFERENT r round to one z.  Two different r = m / c
 *       differ by at least 1 / c_max^2 >= 1 / n^2, less 2^-53 for their own roundings; the subtraction of the mean adds at most
 *       2^-53 (|r - mean| <= 1), the division by sd <= 1/2 doubles the gap, and its rounding adds at most 2^-53 |z| to either z
 *       with |z| <= sqrt(n_lags) <= sqrt(n).  So the z differ whenever 1 / n^2 > 2^-52 + sqrt(n) 2^-53, which holds with a factor
 *       of 8 to spare up to n = SXG_POA_REPEAT_MAX_LEN = 2^20.  A longer sequence gets SXG_ST_TOO_LONG (n_lags = 0) and the call
 *       returns SXG_E_BLOCK, the other sequences being valid: the host scans it itself.
 * A work item is (sequence, tile of 256 consecutive lags), one wavefront, the items of a round sorted largest first and dealt
 * to the workgroups in that order; a lane owns four consecutive lags, reads them as one word per sample and compares it with the
 * replicated sampled letter; the counts leave as plain stores.  No atomics, no cooperative launch, no grid-wide wait, no captured
 * graph: two launches per round on the handle's stream.  The letters (as they came, plus 16 bytes per sequence and 8 per item)
 * and the counts (4 bytes per lag and sequence) come out of the handle's memory budget: sequences run in rounds, in order, as
 * many as their counts fit; a sequence whose counts alone do not fit is SXG_E_NOMEM.  A sequence shorter than 2 min_copy is
 * SXG_ST_OK with n_lags = 0.  SXG_E_INVALID: min_copy = 0, stride = 0, max_copy < min_copy.  match: NULL, or the counts of every
 * scanned sequence, sequence s's n_lags[s] counts at the prefix sum of the n_lags before it (sxg_repeat_match_offsets of
 * poa_repeat.h); for tests.  The call runs inside a ROCTx range; sxg_poa_stats after it: kernel_ms the sum of the kernels,
 * dp_launches their number (2 per round), n_slots the workgroups of the widest counting launch, device_bytes the buffers. */
#define SXG_POA_REPEAT_MAX_LEN (1 << 20)
typedef struct sxg_poa_repeat_in {
    int64_t n_seqs; const int64_t *seq_off; const uint8_t *bases;   /* [n_seqs + 1], [seq_off[n_seqs]] the letters as they are */
    uint64_t min_copy, max_copy, stride;                            /* src/main.cpp:285-286,458: 1000, 20000, 50 */
} sxg_poa_repeat_in;
/* caller-allocated [n_seqs] each; match: NULL or [sum of n_lags] */
int sxg_poa_repeat_scan_batch(sxg_poa_handle *h, const sxg_poa_repeat_in *in, int32_t *n_lags, int32_t *best, double *dev, double *v,
                              int32_t *status, int32_t *match);

/* Resident path letters (an addition to ABI 5, no struct changed): a graph's path letters go to the device ONCE, and the repeat
 * scan and the identity estimate take RANGES of them; a kernel cuts the ranges out of the resident copy into the layout each
 * consumer reads.  Both providers of the host library are fed ranges of paths -- contiguous substrings of
 * a path's spelled sequence --, so this replaces the per-call concatenation and upload of those substrings.
 *   Which letters a call uses.  A ranges call works on the resident letters if their id equals letters_id.  If it differs and
 *     letters != NULL with letters->id == letters_id, the call uploads them first: the one upload of an iteration, whichever
 *     provider comes first; a caller that always passes the pointer keeps no call order and cannot read stale letters.  If the
 *     id differs and there is no usable pointer, the call returns SXG_E_INVALID before any work.  id 0 names nothing.
 *   Validation.  A range with path outside 0 .. n_paths - 1, begin < 0, end < begin or end beyond the path is SXG_E_INVALID; the
 *     message names the range, and nothing is launched.  Empty ranges are legal; ranges may overlap and may repeat.
 *   Results.  Results, statuses and return codes are those of the `bases` calls on the same sequences, array for array:
 *     SXG_ST_TOO_LONG / SXG_E_BLOCK, the identity's min_len filter and its 65 536 cap, the rounds under a small memory budget,
 *     `match`, and sxg_poa_stats -- whose kernel_ms now includes the gather, which sxg_poa_letters_stats also reports by itself
 *     (dp_launches counts the gather as one more launch).  Only the sequences that take part are cut out.
 *   Memory.  The resident letters lie OUTSIDE sxg_poa_set_memory_budget, like the handle's result buffers; they are counted in
 *     device_bytes of the ranges calls.  They survive sxg_poa_batch_* calls and are freed by _drop, by a replacing upload or by
 *     sxg_poa_destroy.  An allocation that fails is SXG_E_NOMEM and leaves nothing resident.
 *   Upload.  Staged through pinned memory of bounded size -- two buffers of the handle's pool in flight --, never a pinned copy of
 *     the whole text.
 *   Scope.  Every handle holds its own copy; a device-group member is a handle.  The sharded entry points are not touched.
 *   Orientation.  There is no reverse-complement flag: ranges are read in step orientation, the path's own spelling, and neither
 *     consumer has a use for another.
 * The gather: a work item is a chunk of sxg_poa_letters_geometry's chunk_bytes destination bytes, dealt grid-stride, its ranges
 * found on the device from the prefix sums of the range lengths by binary search (the host sends no item list, no atomics); 16-byte
 * stores inside a range, byte stores for the at most 15 head and 15 tail bytes, unaligned 16-byte loads that stay inside the
 * range: the resident buffer needs no padding.  coded == 1 applies the table of the identity estimate: either case of A C G T ->
 * 0..3, anything else -> 4. */
typedef struct sxg_poa_letters {   /* a graph's path letters, on the host */
    uint64_t id;                   /* caller-chosen, non-zero: names this set of letters */
    int64_t n_paths;
    const int64_t *path_off;       /* [n_paths+1], path_off[0] == 0 */
    const uint8_t *letters;        /* [path_off[n_paths]] the bytes as they stand in the graph, step orientation */
} sxg_poa_letters;
typedef struct sxg_poa_range { int64_t path, begin, end; } sxg_poa_range;   /* letters [begin, end) of `path` */

int  sxg_poa_letters_upload(sxg_poa_handle *h, const sxg_poa_letters *l);   /* replaces what is resident */
void sxg_poa_letters_drop(sxg_poa_handle *h);
int  sxg_poa_letters_resident(sxg_poa_handle *h, uint64_t *id, int64_t *n_paths, int64_t *n_letters);   /* id 0 = none */
/* since the handle was created: uploads and their bytes, the gathers' kernel time (HIP events) and the bytes they wrote */
int  sxg_poa_letters_stats(sxg_poa_handle *h, uint64_t *uploads, uint64_t *bytes_uploaded, double *gather_ms, uint64_t *gathered_bytes);
void sxg_poa_letters_geometry(int32_t *chunk_bytes);   /* the gather kernel's work-item size, for tests */

/* what the gather kernel writes, for callers and tests: coded == 0 the bytes as they are, coded == 1 the identity code */
int  sxg_poa_range_gather(sxg_poa_handle *h, const sxg_poa_letters *l, uint64_t id, int64_t n, const sxg_poa_range *r, int coded, uint8_t *out /* [sum of lengths] */);

typedef struct sxg_poa_repeat_ranges_in {
    const sxg_poa_letters *letters; uint64_t letters_id;
    int64_t n_seqs; const sxg_poa_range *ranges;
    uint64_t min_copy, max_copy, stride;
} sxg_poa_repeat_ranges_in;
/* as sxg_poa_repeat_scan_batch on the sequences the ranges spell */
int sxg_poa_repeat_scan_ranges(sxg_poa_handle *h, const sxg_poa_repeat_ranges_in *in, int32_t *n_lags, int32_t *best, double *dev, double *v, int32_t *status, int32_t *match);

typedef struct sxg_poa_identity_ranges_in {
    const sxg_poa_letters *letters; uint64_t letters_id;
    int32_t n_blocks; const int32_t *blk_off; const sxg_poa_range *ranges;
    int32_t kmer_size, min_len; double percentile;
} sxg_poa_identity_ranges_in;
/* as sxg_poa_block_identity_batch on the sequences the ranges spell, coded by the table above */
int sxg_poa_block_identity_ranges(sxg_poa_handle *h, const sxg_poa_identity_ranges_in *in, int32_t *n_used, int32_t *inter, int32_t *uni, int32_t *status);

/* The node order of prep (src/prep.cpp:11-163: odgi's path_linear_sgd_order, called from src/main.cpp:423-433 before every
 * iteration unless -n), decree Y of DESIGN.md section 9.  odgi is absent from the snapshot and its hogwild updates are not
 * reproducible, so the order is fixed by decree, bit for bit:
 *   Y1  state: X[n], an int64 in units of 2^-20 bp, starts as (sum of len of the nodes before n) << 20.  SXG_E_INVALID if the
 *       total length >= 2^40, the steps S >= 2^32 or the nodes N >= 2^31.  Orientation plays no part.
 *   Y2  the schedule is the caller's: eta[iter_max] (double) and cooling_start.  The host library computes what prep.cpp asks
 *       for (sxg_graph_prep: eta_max = (steps of the longest path)^2, eps = 0.01, lambda = ln(eta_max / eps) / (iter_max - 1),
 *       eta[t] = eta_max * exp(-lambda t), iter_max = 100, cooling_start = iter_max / 2, terms_per_iter = (uint64)(term_updates
 *       * S)); the device never calls exp.
 *   Y3  counter-based random numbers.  mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *       x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31 (mod 2^64).  Term k of iteration it:
 *       base = mix(seed ^ (it << 40) ^ k), r1 = mix(base), r2 = mix(r1), r3 = mix(r2).
 *   Y4  the pair.  a = r1 mod S is a flat step; p its path (the last path that starts at or before a), n its step count, ia the
 *       index of a in it.  If (r2 & 1) or it >= cooling_start the second step is drawn log-uniformly by octave (the integer
 *       stand-in for odgi's Zipf with theta 0.99): nb = max(1, bitlength(maxsteps - 1)) with maxsteps the steps of the longest
 *       path, bits = (r2 >> 1) mod nb, j = (1 << bits) + ((r2 >> 8) & ((1 << bits) - 1)), ib = ia + j if bit 7 of r2 is set,
 *       else ia - j; outside [0, n) the other direction is taken, then clamped to [0, n - 1].  Otherwise ib = r3 mod n.
 *       Node ends: pa = step_pos[a] + len[node of a] if bit 62 of r3 is set, else step_pos[a]; pb likewise for b with bit 63;
 *       d = |pa - pb|.  The term is skipped if d == 0 or the two nodes are equal.
 *   Y5  the update for nodes i (of a) and j (of b), in IEEE double, every operation rounded once (no contraction, no fast-math):
 *       dx = (double)(X[i] - X[j]) / 2^20, mag = |dx|, sgn = the sign of dx, or when dx == 0: -1 if i < j, else +1;
 *       mu = min(eta[it] / d, 1); delta = mu * (mag - d) / 2; q = llrint(delta * sgn * 2^20), half to even;
 *       D[i] -= q, D[j] += q.
 *   Y6  the terms of an iteration run in batches of B = max(1, N div 8) consecutive k (the last one partial); every term of a
 *       batch reads the X of the batch's start; the q are summed into D with 64-bit INTEGER atomic adds (integer sums do not
 *       depend on the order of arrival: no float atomics); at the batch's end X += D, D = 0.
 *   Y7  the new order is the nodes sorted by (X, old rank).
 * Two paths with the same results: with 16 * N bytes of dynamic LDS (N <= SXG_POA_SGD_LDS_NODES) one workgroup keeps X and D on
 * chip for the whole sort -- batches separated by __syncthreads, ONE launch, which therefore lasts as long as the sort: mode 0
 * chooses it only when iter_max * terms_per_iter <= SXG_POA_SGD_LDS_TERMS (seconds), and falls back to the other path if the
 * runtime refuses the dynamic LDS; mode 1 asks for it whatever the term count --; otherwise one launch of the term kernel (one
 * thread per term) and one of the apply kernel per batch, on the handle's stream.  No cooperative launch, no grid-wide wait,
 * no captured graph.  The scratch comes out of the handle's memory budget; the call runs inside a ROCTx range and fills
 * kernel_ms, n_slots / dp_launches (the number of launches) and device_bytes of sxg_poa_stats.  Y7's sort runs on the host.
 * Not restated: odgi's groom pass and its final topological_order pass. */
#define SXG_POA_SGD_LDS_NODES 8192
#define SXG_POA_SGD_LDS_TERMS (1ull << 30)
typedef struct sxg_poa_sgd_in {
    int64_t n_nodes; const int32_t *node_len;      /* nodes in rank order */
    int64_t n_paths; const int64_t *path_off;      /* [n_paths+1] flat steps of every path */
    const int32_t *step_node; const int64_t *step_pos; /* [path_off[n_paths]] node rank; bp offset of the step in its path */
    int32_t iter_max, cooling_start; const double *eta; /* [iter_max] */
    uint64_t terms_per_iter, seed;
    int32_t mode;   /* 0 = choose, 1 = LDS path (SXG_E_INVALID if it does not fit), 2 = global path */
} sxg_poa_sgd_in;
/* order: [n_nodes] old ranks in the new order; x: [n_nodes] the final X by old rank, or NULL. */
int sxg_poa_path_sgd_order(sxg_poa_handle *h, const sxg_poa_sgd_in *in, int32_t *order, int64_t *x);

int sxg_poa_get_stats(sxg_poa_handle *h, sxg_poa_stats *out);
int sxg_poa_get_width_stats(sxg_poa_handle *h, sxg_poa_width_stats *out);
/* The switch of SXG_POA_MAX_SEQ_LEN_TILED (on != 0; read by the next sxg_poa_batch_upload and by the executes of that batch),
 * and what the last execute ran in column tiles: blocks of its tiled launches, the sweeps (alignments) of those launches and the
 * tiles they swept -- more tiles than sweeps means some sweep crossed a tile edge.  Any of the three pointers may be NULL. */
int sxg_poa_set_long_blocks(sxg_poa_handle *h, int on);
int sxg_poa_get_tile_stats(sxg_poa_handle *h, int64_t *blocks, int64_t *sweeps, int64_t *tiles);
int sxg_poa_get_twin_stats(sxg_poa_handle *h, sxg_poa_twin_stats *out);
int sxg_poa_get_msa_stats(sxg_poa_handle *h, double *cols_ms, double *rows_ms, uint64_t *msa_bytes);
/* The rows kernel's geometry: kept letters of a row one work item places, bytes of a row it builds on chip at once (tests). */
void sxg_poa_msa_geometry(int32_t *chunk_letters, int32_t *tile_bytes);

/* The resident trimmed MSA of the batch last executed on the handle (want_msa = SXG_MSA_TRIMMED or SXG_MSA_TRIMMED_RESIDENT,
 * nothing uploaded since; anything else is SXG_E_INVALID).  Rows are counted block after block -- GLOBAL ROW INDEX --: a block's
 * rows number nseq (+ 1 with consensus), and 0 for a block that is not live (status not SXG_ST_OK, or no sequences).
 *
 * sxg_poa_msa_row_letters: letters[r] = the bytes other than '-' of row r: what a caller checks the contract of SXG_MSA_TRIMMED
 *   with (a sequence row holds its length minus twice the trim, or nothing) without seeing a row.
 *
 * sxg_poa_maf_text: `out` receives the segments back to back; out_bytes must equal the sum of their len.
 *   kind 0: `len` bytes of `literal` from offset src;
 *   kind 1: row `src` as it stands, len must equal its block's msa_cols;
 *   kind 2: the same row reversed and complemented: '-' -> '-', 'A' <-> 'T', 'C' <-> 'G', every other byte value -> 'N'.
 *   Every segment is checked on the host before anything is launched (kind, row index, len == msa_cols, literal range, out_bytes):
 *   a bad one is SXG_E_INVALID, nothing is launched and `out` is untouched.  One kernel lays the text out in a device buffer
 *   (16-byte stores, granules assembled in registers from every segment that overlaps them), one copy brings it to `out`.
 * sxg_poa_maf_text_geometry: the destination bytes of one work item of that kernel (tests).
 * sxg_poa_maf_text_stats: HIP-event milliseconds of the text kernel and the bytes it wrote, summed over the handle's calls (either
 *   pointer may be NULL). */
typedef struct sxg_poa_maf_seg { int64_t src; int32_t len; int32_t kind; } sxg_poa_maf_seg;
typedef struct sxg_poa_maf_text_in {
    int64_t n_segs; const sxg_poa_maf_seg *segs;
    const uint8_t *literal; int64_t literal_bytes;
} sxg_poa_maf_text_in;
int sxg_poa_msa_row_letters(sxg_poa_handle *h, int32_t *letters /* [sum over blocks of rows] */);
int sxg_poa_maf_text(sxg_poa_handle *h, const sxg_poa_maf_text_in *in, char *out, int64_t out_bytes);
void sxg_poa_maf_text_geometry(int32_t *chunk_bytes);
int sxg_poa_maf_text_stats(sxg_poa_handle *h, double *kernel_ms, uint64_t *bytes);
/* Cap on device memory the handle may use for scratch arenas (bytes; 0 = default 3/4 of free). */
int sxg_poa_set_memory_budget(sxg_poa_handle *h, uint64_t bytes);

/* XXH64 of a sequence: the dedup key smooth_spoa uses (src/smooth.cpp:716, seed 0). */
uint64_t sxg_xxh64(const void *data, uint64_t len, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif

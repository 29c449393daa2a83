/*
 * sxg_smooth.h -- C ABI of the host-side rows around the blocked-POA engine:
 *
 *   A2  append_to_sequence (flank padding)            src/smooth.cpp:75-126
 *   A3  sequence collection, orientation, XXH64 dedup src/smooth.cpp:676-743
 *   A4  padding size                                  src/smooth.cpp:1946-1970
 *   A14 adaptive POA scores per block (-a)            src/smooth.cpp:1972-2069
 *   A8' MSA -> MAF rows of a block (-m)               src/smooth.cpp:782-905, src/maf.hpp:35-66
 *   A9  build_odgi_SPOA (POA graph -> block graph)    src/smooth.cpp:2576-2654
 *   A10 unchop + topological order + re-copy          src/smooth.cpp:935-1010
 *   8f-1 lacing of the block graphs + GFA writer      src/main.cpp:599-1061
 *   8f-3 minimal GFA reader (S/P lines)               src/xg.cpp:696-741 (what the path needs of it)
 *
 * Built by g++ into libsxgsmooth.so (no HIP inside): the POA itself is reached through a callback
 * with the signature of sxg_poa_batch_run (include/sxg_poa.h), so production passes the GPU engine
 * and nothing in this library can fall back to a CPU aligner.
 *
 * odgi (unchop, topological_order, to_gfa) is absent from the reference snapshot, so those three
 * are restated by decree: parity with real odgi bytes is unpinned.
 * All strings returned through char** are malloc'ed; release with sxg_smooth_free().
 */
#ifndef SXG_SMOOTH_H
#define SXG_SMOOTH_H
#include <stddef.h>
#include <stdint.h>
#include "sxg_poa.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sxg_graph sxg_graph;       /* input graph: node sequences + paths (XG's role) */
typedef struct sxg_blockset sxg_blockset; /* blockset_t: blocks of path ranges, src/blocks.hpp:29-120 */

/* POA provider: exactly sxg_poa_batch_run's contract, ctx is its handle.  Both callbacks are only called while the
 * sxg_* entry point they were passed to is running -- `run` possibly from a worker thread of that call (one call at a
 * time), `free` on the calling thread, once per successful `run`, before the entry point returns: callbacks and ctx
 * need not outlive the call. */
typedef int (*sxg_poa_run_fn)(void *ctx, const sxg_poa_batch_in *in, sxg_poa_batch_out *out);
typedef void (*sxg_poa_free_fn)(sxg_poa_batch_out *out);

/* smoothxg's knobs on this path with their defaults (src/main.cpp:291-361,487). */
/* 2: sxg_smooth_params starts with struct_size (set by sxg_smooth_default_params, checked by every entry point: a caller
 *    built against another header gets SXG_E_INVALID instead of fields read from whatever follows its struct) and ends
 *    with poa_spoa_order; scores whose engine form leaves int8 are rejected. */
#define SXG_SMOOTH_ABI_VERSION 2
int sxg_smooth_abi_version(void);

typedef struct sxg_smooth_params {
    uint32_t struct_size;                             /* sizeof(sxg_smooth_params) of the caller's header */
    int32_t poa_m, poa_n, poa_g, poa_e, poa_q, poa_c; /* CLI convention: positive penalties (1,4,6,2,26,1) */
    int32_t local_alignment;                          /* 1 = default; 0 = -Z */
    float poa_padding_fraction;                       /* -O, default 0.001 */
    uint64_t max_block_depth_for_padding_more;        /* -Y, default 1000 */
    int32_t add_consensus;                            /* embed Consensus_<block> paths (last iteration) */
    const char *consensus_base_name;                  /* default "Consensus_" */
    int32_t adaptive_poa_params;                      /* -a: per-block scores from the estimated identity, default 0 */
    int32_t kmer_size;                                /* -k: k-mer size of the identity estimate, default 17 */
    int32_t use_abpoa;                                /* -A (src/main.cpp:130-132): the smooth_abpoa path, src/smooth.cpp:133-627.  The
                                                         scores are then in abPOA's convention -- a gap of k costs min(g + k e, q + k c);
                                                         g = 0: linear, q = 0: affine (the 4-parameter form sets q = c = 0,
                                                         src/main.cpp:355-358) --, alignments run with the ADAPTIVE band
                                                         (params.banded = 2: wb = 311, wf = 0.03, src/smooth.cpp:266-271,2090) and the
                                                         consensus path keeps only nodes some sequence visits (build_odgi_abPOA,
                                                         src/smooth.cpp:2542-2548).  Default 0. */
    int32_t abpoa_band_local;                         /* use_abpoa with LOCAL alignment (the default mode): 1 = banded as the call
                                                         site asks (src/smooth.cpp:266-271 sets wb / wf for both modes; default);
                                                         0 = full matrix -- upstream abPOA is believed to switch its adaptive band
                                                         off in local mode (abpoa_post_set_para; unverifiable here, the library is
                                                         absent from the snapshot), in which case this is what -A without -Z runs.
                                                         Global alignment (-Z) is banded either way. */
    int32_t poa_spoa_order;                           /* 1 = the engine re-sorts a block's graph after every alignment the way
                                                         spoa's TopologicalSort is believed to (SXG_ORDER_SPOA, include/sxg_poa.h:
                                                         decree S7', restated from memory, unverified) instead of keeping it in
                                                         order incrementally (decree S7).  DEFAULT 1 since round 6: it is what
                                                         graph.AddAlignment does at src/smooth.cpp:764, and the re-sort is a
                                                         parallel, incremental device phase now (1-5 % of the kernel time at full batches,
                                                         DESIGN.md).  Ignored with use_abpoa (abPOA does not call spoa's sort).
                                                         0 = the order of rounds 1-5.
                                                         2 = as 1, and the new nodes of a sequence get their ids in the order spoa's
                                                         AddAlignment is believed to create them (SXG_IDS_SPOA, decree S6', restated
                                                         from memory, unverified); opt-in, dropped with use_abpoa as 1 is. */
} sxg_smooth_params;

void sxg_smooth_default_params(sxg_smooth_params *p);
const char *sxg_smooth_last_error(void);
void sxg_smooth_free(void *p);

/* GFA reader: S, P and L lines (the L lines only serve block discovery's edge-jump limit).
 * Letters outside ACGT become N as in XG's 3-bit alphabet (src/xg.cpp:24-53). */
int sxg_graph_from_gfa(const char *text, size_t len, sxg_graph **out);
void sxg_graph_free(sxg_graph *g);
int64_t sxg_graph_node_count(const sxg_graph *g);
int64_t sxg_graph_path_count(const sxg_graph *g);

/* Test/demo blockset: every path is cut into consecutive windows of >= target_bp and the k-th window
 * of every path forms block k.  This is NOT the reference's smoothable_blocks()/break_blocks() (block
 * discovery is out of scope): it only provides a valid partition of all path
 * steps -- roughly homologous for collinear haplotypes -- so that collection, POA and lacing can be
 * exercised end to end.  Ranges of a block are ordered longest first (src/blocks.cpp:206-219). */
int sxg_blockset_by_path_windows(const sxg_graph *g, uint64_t target_bp, sxg_blockset **out);

/* path_range_t of the reference (src/blocks.hpp:29-33): steps [step_begin, step_end) of path `path`
 * (rank of the P line in the input GFA), `length` = their bases (0 = let the library compute it; a
 * non-zero value is checked against the steps). */
typedef struct sxg_path_range {
    int64_t path, step_begin, step_end, length;
} sxg_path_range;
/* blockset_t from the caller's own blocks (src/blocks.hpp:70-120, what smoothable_blocks / break_blocks
 * produce): block k owns ranges[blk_off[k] .. blk_off[k+1]) in alignment order. */
int sxg_blockset_from_ranges(const sxg_graph *g, int64_t n_blocks, const int64_t *blk_off, const sxg_path_range *ranges,
                             sxg_blockset **out);
/* Block discovery, src/blocks.cpp:7-327 (smoothable_blocks): the greedy sweep over the nodes in rank order
 * with the weight / path-length / path-jump / edge-jump limits, ranges broken at steps an earlier block took,
 * blocks split into the connected components of their path adjacencies.  smoothxg passes
 * max_block_weight = target_poa_length * n_haps (-w), max_block_path_length = target_poa_length (-l),
 * max_path_jump (-j, default 100), max_edge_jump (-e, default 0 = off), src/main.cpp:282-283,376-377,447-455.
 * Needs the L lines of the GFA (edge jumps).  Decrees: stable ordering of equal-length ranges, id order = XG
 * node order. */
int sxg_blockset_smoothable(const sxg_graph *g, uint64_t max_block_weight, uint64_t max_block_path_length,
                            uint64_t max_path_jump, uint64_t max_edge_jump, int order_paths_from_longest,
                            sxg_blockset **out);
/* The cutting half of break_blocks, src/breaks.cpp:210-330: a block that holds a range longer than max_poa_length (-q,
 * default 2 * target) is cut.  As the reference always does (break_repeats = true, src/main.cpp:476), the ranges of such a
 * block of at least 2 * min_copy_length bases are searched for a tandem repeat first (src/breaks.cpp:224-272); if any is
 * found, EVERY range of the block is cut at half the mean repeat length, otherwise the long ranges are cut blindly at
 * max_poa_length.  sxg_blockset_break uses the reference's repeat parameters (min_copy_length 1000, max_copy_length 20000,
 * min_autocorr_z 5, autocorr_stride 50: src/main.cpp:285-286,457-458); sxg_blockset_break_ex takes them (break_repeats = 0:
 * blind cuts only).  The repeat detector stands in for sautocorr::repeat, an un-vendored dependency absent from the
 * snapshot, BY DECREE: match-fraction autocorrelation at every lag in [min_copy_length,
 * max_copy_length] over positions sampled every autocorr_stride bases, z-score across the lags, first lag of greatest z
 * if that z reaches min_autocorr_z.  Identity splitting (src/breaks.cpp:335+; off by default) is not applied by these two:
 * it is the call below, sxg_blockset_split, run on their result. */
int sxg_blockset_break(const sxg_graph *g, const sxg_blockset *in, uint64_t max_poa_length, int order_paths_from_longest,
                       sxg_blockset **out);
int sxg_blockset_break_ex(const sxg_graph *g, const sxg_blockset *in, uint64_t max_poa_length, int break_repeats,
                          uint64_t min_copy_length, uint64_t max_copy_length, double min_autocorr_z, uint64_t autocorr_stride,
                          int order_paths_from_longest, sxg_blockset **out);
/* The same cut with the repeat scan behind a provider, and the two counts the reference prints (an addition to ABI 2, no struct
 * changed).  Scan provider: exactly sxg_poa_repeat_scan_batch's contract (decree R of include/sxg_poa.h: the match count of every
 * lag in exact integers, then best / dev / v of a pinned double-precision pass), ctx is its handle.  sxg_blockset_break_scan finds
 * the blocks that will be cut, collects the range sequences of at least 2 * min_copy_length bases of ALL of them (step
 * orientation, the letters as they stand), makes ONE provider call on the calling thread, turns every (best, dev, v) into a repeat
 * length with the host scan's own three operations (sd = sqrt(v); none if sd == 0; min_copy_length + best iff dev / sd >=
 * min_autocorr_z) and cuts as sxg_blockset_break_ex does.  *n_cut: the blocks cut, *n_repeat: those of them cut at a repeat
 * (src/breaks.cpp:220,265,596); *n_host: the sequences the provider reported with a status other than SXG_ST_OK, which the host
 * scanned itself; any of the three may be NULL.  scan == NULL: sxg_blockset_break_ex with break_repeats = 1 and the counts
 * (*n_host = 0).  A provider that returns anything but SXG_OK / SXG_E_BLOCK, a wrong n_lags, or best out of range fails the call. */
typedef int (*sxg_repeat_fn)(void *ctx, const sxg_poa_repeat_in *in, int32_t *n_lags, int32_t *best, double *dev, double *v,
                             int32_t *status, int32_t *match);
int sxg_blockset_break_scan(const sxg_graph *g, const sxg_blockset *in, uint64_t max_poa_length, uint64_t min_copy_length,
                            uint64_t max_copy_length, double min_autocorr_z, uint64_t autocorr_stride, int order_paths_from_longest,
                            sxg_repeat_fn scan, void *ctx, sxg_blockset **out, int64_t *n_cut, int64_t *n_repeat, int64_t *n_host);
/* Range providers (additions to ABI 2, no struct changed).  Both providers above are fed ranges of paths, contiguous substrings of
 * a path's spelled sequence; with these forms the library sends the RANGES -- sxg_poa_range{path, pos[begin], pos[end]} in letters of
 * the path -- and the graph's path letters by pointer, and builds no sequence (include/sxg_poa.h, "Resident path letters": the engine
 * uploads the letters once per graph, whichever provider comes first).  Everything behind the provider call is shared with the
 * `bases` forms: the checks of the returned counts, the decision, the host's own scan or estimate of a declined item; a provider
 * error fails the call.
 * sxg_graph_path_letters: the graph's path letters, concatenated once and cached in the graph (OpenMP over paths; path p ==
 * its spelled sequence); out points into the graph and lives as long as it; id is unique per graph object in the process. */
int sxg_graph_path_letters(const sxg_graph *g, sxg_poa_letters *out);
typedef int (*sxg_repeat_ranges_fn)(void *ctx, const sxg_poa_repeat_ranges_in *in, int32_t *n_lags, int32_t *best, double *dev, double *v,
                                    int32_t *status, int32_t *match);
typedef int (*sxg_identity_ranges_fn)(void *ctx, const sxg_poa_identity_ranges_in *in, int32_t *n_used, int32_t *inter, int32_t *uni,
                                      int32_t *status);
/* as sxg_blockset_break_scan (scan must not be NULL) */
int sxg_blockset_break_scan_ranges(const sxg_graph *g, const sxg_blockset *in, uint64_t max_poa_length, uint64_t min_copy_length,
                                   uint64_t max_copy_length, double min_autocorr_z, uint64_t autocorr_stride, int order_paths_from_longest,
                                   sxg_repeat_ranges_fn scan, void *ctx, sxg_blockset **out, int64_t *n_cut, int64_t *n_repeat,
                                   int64_t *n_host);
/* as sxg_blockset_identity_thresholds (ident == NULL: the host estimator) */
int sxg_blockset_identity_thresholds_ranges(const sxg_graph *g, const sxg_blockset *b, int32_t kmer_size, uint64_t max_depth,
                                            sxg_identity_ranges_fn ident, void *ctx, float *est_identity_threshold, int32_t *n_used);
/* The range providers of an iteration and their context (the engine handle).  sxg_smooth_iteration_ranges is the iteration with
 * the identity estimate of -a fed ranges: mp == NULL (then out_maf must be NULL and device_rows 0) is sxg_smooth_gfa_adaptive,
 * mp != NULL sxg_smooth_maf_gfa_adaptive, and with device_rows != 0 sxg_smooth_maf_gfa_device_rows; rp == NULL or rp->identity ==
 * NULL: the host estimator.  rp->scan is not called by the iteration (block discovery runs before it: sxg_blockset_break_scan_ranges);
 * the record carries it so that a caller binds both providers to one handle in one place. */
typedef struct sxg_range_providers {
    sxg_repeat_ranges_fn scan;
    sxg_identity_ranges_fn identity;
    void *ctx;
} sxg_range_providers;
struct sxg_merge_params;
int sxg_smooth_iteration_ranges(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p, const struct sxg_merge_params *mp,
                                sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, const sxg_range_providers *rp, int device_rows,
                                char **out_gfa, char **out_maf, int64_t *n_flipped);
/* The splitting half of break_blocks, src/breaks.cpp:335-586 (-I / --block-id-min, -R / --block-ratio-min and the dedup
 * depth; an addition to ABI 2, no struct changed): a block whose sequences fall into more than one identity group becomes one
 * block per group.  Decree P3 of DESIGN.md section 9, statement by statement as the reference: nothing happens to a block
 * unless block_group_identity > 0 and it has more than one range; its range sequences are dedup'd ("equal to a kept sequence
 * or to its reverse complement": the first occurrence is kept, in its orientation, with the list of original ranks); nothing
 * happens unless min_dedup_depth != 0 && dedup'd sequences >= min_dedup_depth -- the quirk is kept: the CLI default 0 means
 * "never split" --; the kept sequences are sorted by (length, letters) and handed, all candidate blocks in ONE call, to the
 * split provider, which runs the greedy clustering (sxg_poa_split_batch: the pair alignments are the hot part and run on the
 * GPU; this library holds no alignment code).  One group: the block is unchanged.  More: one new block per group in group
 * order, a group's members in the order they joined, each member contributing its original ranges in their original order.
 * New blocks are numbered consecutively in old-block order.  A block the provider reports with a status other than
 * SXG_ST_OK stays whole and is counted in *n_too_long; *n_split counts the blocks that were split.  The mash-based branch
 * (:388-471, dedup depth >= 12000 on the CLI) is sxg_blockset_split_mash below; this call is the walk without it.
 * Split provider: exactly sxg_poa_split_batch's contract, ctx is its handle; called at most once, on the calling thread. */
typedef int (*sxg_split_fn)(void *ctx, const sxg_poa_split_in *in, sxg_poa_split_out *out);
typedef void (*sxg_split_free_fn)(sxg_poa_split_out *out);
int sxg_blockset_split(const sxg_graph *g, const sxg_blockset *in, double block_group_identity, double length_ratio_min,
                       uint64_t min_dedup_depth, sxg_split_fn split, sxg_split_free_fn split_free, void *ctx, sxg_blockset **out,
                       int64_t *n_split, int64_t *n_too_long);
/* The same with the mash-based branch of :388-471 (decrees M1-M5 of DESIGN.md section 9; -L / -D / -e / -k of src/main.cpp:
 * 102-112,302-320): a candidate block whose dedup depth reaches min_depth_mash (0 = every candidate) compares its sequences of
 * at least min_len_mash bases by the Jaccard index of their canonical k-mer sets against block_group_est_identity (<= 0: equal
 * to block_group_identity); min_len_mash = 0 turns the branch off and the result is sxg_blockset_split's.  min_len_mash below
 * kmer_size (when not 0), kmer_size outside 1..32 and an est identity above 1 are SXG_E_INVALID.
 * Mash split provider: exactly sxg_poa_split_mash_batch's contract (n_mash is passed as NULL), ctx is its handle. */
typedef int (*sxg_split_mash_fn)(void *ctx, const sxg_poa_split_in *in, const sxg_poa_split_mash *mash, sxg_poa_split_out *out,
                                 int64_t *n_mash);
int sxg_blockset_split_mash(const sxg_graph *g, const sxg_blockset *in, double block_group_identity, double length_ratio_min,
                            uint64_t min_dedup_depth, uint64_t min_len_mash, uint64_t min_depth_mash, double block_group_est_identity,
                            int32_t kmer_size, sxg_split_mash_fn split, sxg_split_free_fn split_free, void *ctx, sxg_blockset **out,
                            int64_t *n_split, int64_t *n_too_long);
int64_t sxg_blockset_block_size(const sxg_blockset *b, int64_t block_id);              /* ranges of a block, -1 on error */
int sxg_blockset_block_ranges(const sxg_blockset *b, int64_t block_id, sxg_path_range *out); /* out[block size] */
void sxg_blockset_free(sxg_blockset *b);
int64_t sxg_blockset_size(const sxg_blockset *b);

/* A2-A4 for one block, as text (one line per record) for inspection and tests:
 *   "padding\t<poa_padding>"
 *   "seq\t<rank>\t<weight>\t<sequence>"                     dedup'd, alignment order
 *   "dup\t<rank>\t<path_range index>\t<is_rev 0|1>\t<name>"  every original range            */
int sxg_block_collect_text(const sxg_graph *g, const sxg_blockset *b, int64_t block_id,
                           const sxg_smooth_params *p, char **out_text);

/* A14, the score tiers of src/smooth.cpp:2032-2069: CLI-convention scores (m,n,g,e,q,c) for a block
 * whose identity threshold is `est_identity_threshold`; below 0.90 the set/default scores are kept. */
void sxg_adaptive_poa_scores(float est_identity_threshold, const int32_t set_scores[6], int32_t out_scores[6]);

/* A14, the identity threshold of one block (src/smooth.cpp:1980-2030): the block's path-range
 * sequences of at least 8*k bases, all-vs-all identity = 1 - mash distance, the 30 % percentile of
 * the sorted identities, floored at 0.7.  *n_used = sequences that took part; the threshold is only
 * defined (and only applied) when *n_used > 1.
 * The reference hashes and compares with rkmh/mkmh, an un-vendored dependency absent from the
 * snapshot; by decree the Jaccard index is taken EXACTLY over the sets of
 * canonical k-mers (no sketch), distance = -ln(2J/(1+J))/k, 1 when J = 0.  k <= 32. */
int sxg_block_identity_threshold(const sxg_graph *g, const sxg_blockset *b, int64_t block_id, int32_t kmer_size,
                                 float *est_identity_threshold, int32_t *n_used);

/* A14 for every block at once, and the identity provider (an addition to ABI 2, no struct changed).
 * Identity provider: exactly sxg_poa_block_identity_batch's contract (decree Q of include/sxg_poa.h: the all-pairs Jaccard
 * estimate in exact integers, one (inter, uni) per block), ctx is its handle.  This library cannot run a device estimator
 * by itself, as it cannot align; without a provider it runs the estimator above on the host cores.
 * sxg_blockset_identity_thresholds: thr / n_used [sxg_blockset_size(b)], caller-allocated.  A block with at most one range or
 * with more than max_depth ranges (-Y, max_block_depth_for_padding_more: src/smooth.cpp:1982) is not estimated and reports
 * n_used = 0, thr = 0; thr is defined where n_used > 1.  ident == NULL: sxg_block_identity_threshold's estimator, block by
 * block over the host threads.  Otherwise the estimated blocks' range sequences (step orientation, unpadded, not dedup'd, coded
 * here: either case of A C G T is a letter, anything else is code 4) go to the provider in ONE call with min_len = 8 * kmer_size
 * and percentile = 0.30, and thr = max(0.7f, identity(inter, uni, k)) -- the host estimator's value bit for bit (decree Q4).
 * A block the provider reports with a status other than SXG_ST_OK falls back to the host estimator; a provider that returns
 * anything but SXG_OK / SXG_E_BLOCK, a wrong n_used or counts out of range fails the call. */
typedef int (*sxg_identity_fn)(void *ctx, const sxg_poa_identity_in *in, int32_t *n_used, int32_t *inter, int32_t *uni, int32_t *status);
int sxg_blockset_identity_thresholds(const sxg_graph *g, const sxg_blockset *b, int32_t kmer_size, uint64_t max_depth,
                                     sxg_identity_fn ident, void *ctx, float *est_identity_threshold, int32_t *n_used);

/* A9+A10 for one block given its POA result: the normalised block graph as GFA text. */
int sxg_block_graph_gfa(const sxg_graph *g, const sxg_blockset *b, int64_t block_id,
                        const sxg_smooth_params *p, sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx,
                        char **out_gfa);

/* MAF rows of one block (src/smooth.cpp:782-905): the block's MSA (consensus row last when
 * add_consensus) with the padding blanked (first/last poa_padding non-gap characters of every row),
 * all-gap flank columns trimmed, and one record per (sequence, duplicate) in the reference's emission
 * order, as text lines  "<src>\t<start>\t<size>\t<+|->\t<srcSize>\t<text>".  For a reverse range
 * start counts from the end of the path (MAF convention, :873-876). */
int sxg_block_maf_rows(const sxg_graph *g, const sxg_blockset *b, int64_t block_id, const sxg_smooth_params *p,
                       sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, char **out_rows);

/* The same rows as one MAF block, formatted as write_maf_rows does (src/maf.hpp:35-66: "s " lines,
 * columns padded to the widest entry, a blank line at the end).  The reference walks a hash map there,
 * so its order of sources is unspecified; here sources appear in first-emission order. */
int sxg_block_maf(const sxg_graph *g, const sxg_blockset *b, int64_t block_id, const sxg_smooth_params *p,
                  sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, char **out_maf);

/* One smoothing iteration over all blocks: collect -> ONE batched POA call -> block graphs ->
 * lace -> validate (every path spells its original sequence, src/main.cpp:770-810) -> unchop ->
 * GFA text.  Returns SXG_OK, or SXG_E_INVALID if validation fails. */
int sxg_smooth_gfa(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p,
                   sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, char **out_gfa);

/* The same iteration with an identity provider for -a (ident == NULL: sxg_smooth_gfa itself).  With adaptive_poa_params the
 * estimates of ALL blocks come from one provider call (sxg_blockset_identity_thresholds' rules), made on the calling thread
 * BEFORE the chunk pipeline starts: the POA provider runs in a thread of its own, usually on the same engine handle, and the
 * two are never in flight together.  Without adaptive_poa_params the identity provider is never called. */
int sxg_smooth_gfa_adaptive(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p,
                            sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, sxg_identity_fn ident, void *ident_ctx,
                            char **out_gfa);

/* A13 + 8f-4: the iteration with the in-order MAF consumer of smooth_and_lace (src/smooth.cpp:1600-1919): every
 * block's MAF rows are merged into groups of blocks whose path ranges continue one another (contiguous-path Jaccard
 * >= the threshold, -M / -J), a block that joins a group in the opposite orientation is FLIPPED -- its block graph is
 * rebuilt reverse-complemented (src/smooth.cpp:2352-2436), which changes the laced GFA --, merged groups get one
 * merged consensus path (src/main.cpp:870-960) and the MAF text is written group by group (src/smooth.cpp:1312-1544).
 * Decrees: hash-map walks of the reference become insertion order; the flip applies the intended transformation
 * (see sxg_smooth.cpp: the reference indexes its handle table with keys it never inserted). */
typedef struct sxg_merge_params {
    int32_t merge_blocks;                 /* -M, default 0 */
    double contiguous_path_jaccard;       /* -J, default 1.0 */
    int32_t preserve_unmerged_consensus;  /* -N, default 0 */
    uint64_t max_merged_groups_in_memory; /* default 50 */
    const char *maf_header;               /* written before the first block (src/main.cpp:489-520); NULL = none */
} sxg_merge_params;
void sxg_merge_default_params(sxg_merge_params *mp);
int sxg_smooth_maf_gfa(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p, const sxg_merge_params *mp,
                       sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, char **out_gfa, char **out_maf, int64_t *n_flipped);

/* sxg_smooth_maf_gfa with an identity provider for -a: see sxg_smooth_gfa_adaptive. */
int sxg_smooth_maf_gfa_adaptive(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p, const sxg_merge_params *mp,
                                sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, sxg_identity_fn ident, void *ident_ctx,
                                char **out_gfa, char **out_maf, int64_t *n_flipped);

/* sxg_smooth_maf_gfa_adaptive (ident may be NULL) over MAF rows built by the provider (an addition to ABI 2).  With
 * mp->merge_blocks == 0 the iteration asks the provider for want_msa = SXG_MSA_TRIMMED, want_block_graph = 3 and bg_trim
 * (include/sxg_poa.h), so the provider MUST honour SXG_MSA_TRIMMED; it builds the MAF rows straight from the trimmed rows --
 * names, starts, sizes and strands from the collected ranges --, takes every block's grooming orientation from the collected
 * ranges (the lowest-ranked input path's range: collected in reverse or not), runs the same in-order consumer and laces the
 * compact block graphs as sxg_smooth_gfa does (chunk pipeline, validation); a provider that returns no block graphs but raw
 * results with per-base paths works as it does there.  Same GFA, same MAF, no flips.  Every sequence row must hold its padded
 * length minus twice the padding in letters and every row must be msa_cols wide: otherwise -- a provider that answered with
 * the full MSA -- the call fails with SXG_E_INVALID.  With mp->merge_blocks != 0, or SXG_SMOOTH_LEGACY=1, it is
 * sxg_smooth_maf_gfa_adaptive call for call (merging flips block graphs and strings consensus paths together). */
int sxg_smooth_maf_gfa_device_rows(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p, const sxg_merge_params *mp,
                                   sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx, sxg_identity_fn ident, void *ident_ctx,
                                   char **out_gfa, char **out_maf, int64_t *n_flipped);

/* sxg_smooth_maf_gfa_device_rows over MAF TEXT laid out by a provider (an addition to ABI 2, no struct changed): without block
 * merging every block is its own MAF group, whose text is literals the library formats without looking at a row -- the "a
 * blocks=K loops=..." line, "s name start size strand srcSize " of every row, newlines -- and the block's trimmed rows, one copy
 * per duplicate, reversed and complemented where the block is groom-flipped.  With tp != NULL, mp->merge_blocks == 0 and
 * SXG_SMOOTH_LEGACY unset the iteration asks the POA provider for want_msa = SXG_MSA_TRIMMED_RESIDENT (include/sxg_poa.h: msa_off
 * and msa_cols come back, the rows stay with the provider until its next call) and, per chunk of blocks, in the thread that made
 * the provider call and before the next one, calls tp->letters once -- letters[r] = bytes other than '-' of row r, rows counted
 * block after block of the chunk: nseq (+ 1 with consensus) per block with sequences and status SXG_ST_OK --, checks the contract
 * sxg_smooth_maf_gfa_device_rows checks (a violation fails the call with the same message, naming the first bad block), and
 * calls tp->text once with the chunk's literal bytes and segment list (struct sxg_poa_maf_text_in) and the chunk's part of the
 * MAF as `out`.  The host never holds a row.  sxg_poa_msa_row_letters and sxg_poa_maf_text with the engine handle as ctx are such
 * a provider, next to sxg_poa_batch_run on the same handle (not a device group, not the sharded entry: both refuse resident
 * rows).  rp: NULL, or the identity estimate of -a fed ranges (rp->identity; rp->scan is not called).
 * Same GFA, same MAF, *n_flipped = 0, as sxg_smooth_maf_gfa_device_rows.  In every other case -- tp == NULL, mp->merge_blocks != 0,
 * SXG_SMOOTH_LEGACY=1 -- the call IS sxg_smooth_maf_gfa_device_rows (with the identity estimate over rp's ranges), fallbacks
 * included: same bytes, and the text provider is never called. */
typedef int (*sxg_msa_letters_fn)(void *ctx, int32_t *letters);
typedef int (*sxg_maf_text_fn)(void *ctx, const sxg_poa_maf_text_in *in, char *out, int64_t out_bytes);
typedef struct sxg_maf_text_provider { sxg_msa_letters_fn letters; sxg_maf_text_fn text; void *ctx; } sxg_maf_text_provider;
int sxg_smooth_maf_gfa_device_text(const sxg_graph *g, const sxg_blockset *b, const sxg_smooth_params *p,
                                   const struct sxg_merge_params *mp, sxg_poa_run_fn run, sxg_poa_free_fn fre, void *ctx,
                                   const sxg_maf_text_provider *tp, const sxg_range_providers *rp /* NULL or the -a identity over ranges */,
                                   char **out_gfa, char **out_maf, int64_t *n_flipped);

/* prep (src/prep.cpp:11-163, called from src/main.cpp:423-433 before every iteration unless -n): the graph is sorted by
 * path-guided SGD and chopped to nodes of at most max_node_length bases, so that block discovery -- a sweep over the nodes in
 * rank order -- meets the nodes in the order the paths walk them (an addition to ABI 2, no existing struct changed).  odgi is
 * absent from the snapshot: the sort is decree Y of include/sxg_poa.h, the chop decree C of DESIGN.md section 9.  This library
 * cannot sort by itself, as it cannot align: the order comes from a sort provider with exactly sxg_poa_path_sgd_order's
 * contract (ctx is its handle), called once, on the calling thread.
 *   sxg_graph_prep flattens the graph (nodes in rank order, every path as flat steps with their bp offsets), computes the
 *   schedule Y2 -- eta_max = (steps of the longest path)^2 (1 without paths), lambda = ln(eta_max / eps) / (iter_max - 1) (0 when
 *   iter_max == 1), eta[t] = eta_max * exp(-lambda t), cooling_start = (int)(iter_max * cooling), terms_per_iter =
 *   (uint64)(term_updates * steps) --, calls the provider, gives the nodes the ids 1..N in the new order and chops:
 *   C   a node longer than max_node_length becomes ceil(len / max) consecutive nodes of max bases each, the last one taking the
 *       rest; ids are renumbered 1..N' in order; a forward step becomes the pieces in order, a reverse step the pieces in reverse
 *       order, each reversed; an edge attaches to the end piece its orientation touches (leaving n+: the last piece, leaving n-:
 *       the first, entering n+: the first, entering n-: the last), in the orientation the L line was written in; the piece-to-
 *       piece edges k+ -> (k+1)+ are added.  Output: the H line, S lines in id order, L lines sorted by (from, from-orientation,
 *       to, to-orientation; + before -) with duplicates removed, P lines in input order.
 *   sxg_graph keeps the L lines as read for this call (16 bytes per line, also in graphs that are never prepped).
 *   term_updates * steps must stay below 2^63, nodes below 2^31 and steps below 2^32 (decree Y1): SXG_E_INVALID otherwise.
 *   max_node_length 0 = do not chop.  out / out_gfa: either may be NULL; release with sxg_graph_free / sxg_smooth_free. */
typedef struct sxg_prep_params {
    uint32_t struct_size;     /* sizeof(sxg_prep_params) of the caller's header */
    int32_t max_node_length;  /* src/main.cpp:426 (odgi chop to 100), default 100 */
    double term_updates;      /* path_sgd_term_updates: terms per iteration as a multiple of the path steps, default 1 */
    int32_t iter_max;         /* default 100 */
    int32_t mode;             /* handed to the provider: 0 = choose, 1 = LDS path, 2 = global path; default 0 */
    double eps;               /* default 0.01 */
    double cooling;           /* the share of the iterations before cooling starts, default 0.5 */
    uint64_t seed;            /* default SXG_PREP_SEED */
} sxg_prep_params;
#define SXG_PREP_SEED 9399220ull
void sxg_prep_default_params(sxg_prep_params *pp);
typedef int (*sxg_sgd_fn)(void *ctx, const sxg_poa_sgd_in *in, int32_t *order, int64_t *x);
int sxg_graph_prep(const sxg_graph *g, const sxg_prep_params *pp, sxg_sgd_fn sort, void *ctx, sxg_graph **out, char **out_gfa);

#ifdef __cplusplus
}
#endif
#endif

"""ctypes binding of include/sxg_smooth.h (libsxgsmooth.so): the host-side rows around the POA --
sequence collection / padding / dedup (A2-A4), block-graph normalisation (A9, A10), lacing and GFA
I/O.  The POA provider is a C function pointer: `gpu_provider(engine)` hands the
library `sxg_poa_batch_run` of libsxgpoa.so and the engine handle, so a smoothing iteration runs
collect -> one batched GPU call -> lace without Python in the loop."""
import ctypes as C
import os

from . import build as _build
from . import poa as _poa

_lib = None

RUN_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.BatchIn), C.POINTER(_poa.BatchOut))
FREE_FN = C.CFUNCTYPE(None, C.POINTER(_poa.BatchOut))
SPLIT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.SplitIn), C.POINTER(_poa.SplitOut))
SPLIT_FREE_FN = C.CFUNCTYPE(None, C.POINTER(_poa.SplitOut))
SPLIT_MASH_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.SplitIn), C.POINTER(_poa.SplitMash), C.POINTER(_poa.SplitOut), C.POINTER(C.c_int64))
IDENT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.IdentityIn), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                       C.POINTER(C.c_int32))
REPEAT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.RepeatIn), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                        C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32))
IDENT_RANGES_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.IdentityRangesIn), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                              C.POINTER(C.c_int32))
REPEAT_RANGES_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.RepeatRangesIn), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                               C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32))
MSA_LETTERS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int32))
MAF_TEXT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.MafTextIn), C.c_void_p, C.c_int64)
SGD_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(_poa.SgdIn), C.POINTER(C.c_int32), C.POINTER(C.c_int64))


class SmoothParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("poa_m", C.c_int32), ("poa_n", C.c_int32), ("poa_g", C.c_int32), ("poa_e", C.c_int32),
                ("poa_q", C.c_int32), ("poa_c", C.c_int32), ("local_alignment", C.c_int32),
                ("poa_padding_fraction", C.c_float), ("max_block_depth_for_padding_more", C.c_uint64),
                ("add_consensus", C.c_int32), ("consensus_base_name", C.c_char_p),
                ("adaptive_poa_params", C.c_int32), ("kmer_size", C.c_int32), ("use_abpoa", C.c_int32),
                ("abpoa_band_local", C.c_int32), ("poa_spoa_order", C.c_int32)]


EXPORTS = ["sxg_smooth_abi_version", "sxg_smooth_default_params", "sxg_smooth_last_error", "sxg_smooth_free", "sxg_graph_from_gfa",
           "sxg_graph_free", "sxg_graph_node_count", "sxg_graph_path_count", "sxg_blockset_by_path_windows",
           "sxg_blockset_free", "sxg_blockset_size", "sxg_block_collect_text", "sxg_block_graph_gfa",
           "sxg_smooth_gfa", "sxg_adaptive_poa_scores", "sxg_block_identity_threshold",
           "sxg_block_maf_rows", "sxg_block_maf", "sxg_blockset_from_ranges", "sxg_blockset_block_size",
           "sxg_blockset_block_ranges", "sxg_blockset_smoothable", "sxg_blockset_break", "sxg_blockset_break_ex", "sxg_blockset_break_scan", "sxg_blockset_split", "sxg_blockset_split_mash", "sxg_merge_default_params", "sxg_smooth_maf_gfa",
           "sxg_prep_default_params", "sxg_graph_prep", "sxg_blockset_identity_thresholds", "sxg_smooth_gfa_adaptive",
           "sxg_smooth_maf_gfa_adaptive", "sxg_smooth_maf_gfa_device_rows", "sxg_smooth_maf_gfa_device_text", "sxg_graph_path_letters", "sxg_blockset_break_scan_ranges",
           "sxg_blockset_identity_thresholds_ranges", "sxg_smooth_iteration_ranges"]


class PrepParams(C.Structure):
    """sxg_prep_params: the knobs of prep (src/prep.cpp, src/main.cpp:423-433) with the reference's defaults."""
    _fields_ = [("struct_size", C.c_uint32), ("max_node_length", C.c_int32), ("term_updates", C.c_double), ("iter_max", C.c_int32),
                ("mode", C.c_int32), ("eps", C.c_double), ("cooling", C.c_double), ("seed", C.c_uint64)]


class MergeParams(C.Structure):
    """sxg_merge_params: -M / -J / -N of smoothxg (src/main.cpp:282,297-298)."""
    _fields_ = [("merge_blocks", C.c_int32), ("contiguous_path_jaccard", C.c_double), ("preserve_unmerged_consensus", C.c_int32),
                ("max_merged_groups_in_memory", C.c_uint64), ("maf_header", C.c_char_p)]


class RangeProviders(C.Structure):
    """sxg_range_providers: the scan provider, the identity provider and their context."""
    _fields_ = [("scan", C.c_void_p), ("identity", C.c_void_p), ("ctx", C.c_void_p)]


class MafTextProvider(C.Structure):
    """sxg_maf_text_provider: the letters function, the text function and their context."""
    _fields_ = [("letters", C.c_void_p), ("text", C.c_void_p), ("ctx", C.c_void_p)]


class RangeProvider(tuple):
    """A provider that takes RANGES of the graph's path letters (gpu_range_scanner, gpu_range_identifier and their python_ forms):
    a (function, ctx[, keep-alive]) tuple like every provider; the type tells Smoother which form of the call to make."""


class PathRange(C.Structure):
    """path_range_t (src/blocks.hpp:29-33): steps [step_begin, step_end) of path `path`, `length` bases."""
    _fields_ = [("path", C.c_int64), ("step_begin", C.c_int64), ("step_end", C.c_int64), ("length", C.c_int64)]


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    so = _build.SMOOTH_SO
    if not os.path.exists(so):
        _build.build_smooth()
    L = C.CDLL(so)
    vp = C.c_void_p
    L.sxg_smooth_last_error.restype = C.c_char_p
    L.sxg_smooth_free.argtypes = [vp]
    L.sxg_smooth_default_params.argtypes = [C.POINTER(SmoothParams)]
    L.sxg_graph_from_gfa.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    L.sxg_graph_free.argtypes = [vp]
    L.sxg_graph_node_count.restype = C.c_int64
    L.sxg_graph_node_count.argtypes = [vp]
    L.sxg_graph_path_count.restype = C.c_int64
    L.sxg_graph_path_count.argtypes = [vp]
    L.sxg_blockset_by_path_windows.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.sxg_blockset_from_ranges.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(PathRange), C.POINTER(vp)]
    L.sxg_blockset_block_size.restype = C.c_int64
    L.sxg_blockset_block_size.argtypes = [vp, C.c_int64]
    L.sxg_blockset_block_ranges.argtypes = [vp, C.c_int64, C.POINTER(PathRange)]
    L.sxg_blockset_smoothable.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.sxg_blockset_break.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.sxg_blockset_break_ex.argtypes = [vp, vp, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_double, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.sxg_blockset_break_scan.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_uint64, C.c_int, vp, vp, C.POINTER(vp),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.sxg_blockset_split.argtypes = [vp, vp, C.c_double, C.c_double, C.c_uint64, vp, vp, vp, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.sxg_blockset_split_mash.argtypes = [vp, vp, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_int32, vp, vp, vp,
                                          C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.sxg_blockset_free.argtypes = [vp]
    L.sxg_blockset_size.restype = C.c_int64
    L.sxg_blockset_size.argtypes = [vp]
    L.sxg_block_collect_text.argtypes = [vp, vp, C.c_int64, C.POINTER(SmoothParams), C.POINTER(vp)]
    L.sxg_block_graph_gfa.argtypes = [vp, vp, C.c_int64, C.POINTER(SmoothParams), vp, vp, vp, C.POINTER(vp)]
    L.sxg_smooth_gfa.argtypes = [vp, vp, C.POINTER(SmoothParams), vp, vp, vp, C.POINTER(vp)]
    L.sxg_merge_default_params.argtypes = [C.POINTER(MergeParams)]
    L.sxg_smooth_maf_gfa.argtypes = [vp, vp, C.POINTER(SmoothParams), C.POINTER(MergeParams), vp, vp, vp, C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(C.c_int64)]
    L.sxg_smooth_gfa_adaptive.argtypes = [vp, vp, C.POINTER(SmoothParams), vp, vp, vp, vp, vp, C.POINTER(vp)]
    L.sxg_smooth_maf_gfa_adaptive.argtypes = [vp, vp, C.POINTER(SmoothParams), C.POINTER(MergeParams), vp, vp, vp, vp, vp, C.POINTER(vp),
                                              C.POINTER(vp), C.POINTER(C.c_int64)]
    L.sxg_smooth_maf_gfa_device_rows.argtypes = L.sxg_smooth_maf_gfa_adaptive.argtypes
    L.sxg_smooth_maf_gfa_device_text.argtypes = [vp, vp, C.POINTER(SmoothParams), C.POINTER(MergeParams), vp, vp, vp, C.POINTER(MafTextProvider),
                                                 C.POINTER(RangeProviders), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.sxg_blockset_identity_thresholds.argtypes = [vp, vp, C.c_int32, C.c_uint64, vp, vp, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    L.sxg_graph_path_letters.argtypes = [vp, C.POINTER(_poa.LettersIn)]
    L.sxg_blockset_break_scan_ranges.argtypes = L.sxg_blockset_break_scan.argtypes
    L.sxg_blockset_identity_thresholds_ranges.argtypes = L.sxg_blockset_identity_thresholds.argtypes
    L.sxg_smooth_iteration_ranges.argtypes = [vp, vp, C.POINTER(SmoothParams), C.POINTER(MergeParams), vp, vp, vp, C.POINTER(RangeProviders), C.c_int,
                                              C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.sxg_block_maf_rows.argtypes = [vp, vp, C.c_int64, C.POINTER(SmoothParams), vp, vp, vp, C.POINTER(vp)]
    L.sxg_block_maf.argtypes = [vp, vp, C.c_int64, C.POINTER(SmoothParams), vp, vp, vp, C.POINTER(vp)]
    L.sxg_prep_default_params.restype = None
    L.sxg_prep_default_params.argtypes = [C.POINTER(PrepParams)]
    L.sxg_graph_prep.argtypes = [vp, C.POINTER(PrepParams), vp, vp, C.POINTER(vp), C.POINTER(vp)]
    L.sxg_adaptive_poa_scores.restype = None
    L.sxg_adaptive_poa_scores.argtypes = [C.c_float, C.POINTER(C.c_int32 * 6), C.POINTER(C.c_int32 * 6)]
    L.sxg_block_identity_threshold.argtypes = [vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
    _lib = L
    return L


class SmoothError(RuntimeError):
    pass


def default_params(**kw):
    p = SmoothParams()
    load_library().sxg_smooth_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def adaptive_poa_scores(est_identity_threshold, set_scores=(1, 4, 6, 2, 26, 1)):
    """A14: the score tier (m, n, g, e, q, c; CLI convention) of src/smooth.cpp:2032-2069."""
    a, o = (C.c_int32 * 6)(*set_scores), (C.c_int32 * 6)()
    load_library().sxg_adaptive_poa_scores(est_identity_threshold, C.byref(a), C.byref(o))
    return tuple(o)


def gpu_provider(engine, sharded=False):
    """(run, free, ctx) backed by the GPU engine: raw C entry points of libsxgpoa.so.  sharded=True: the multi-GPU
    entry (sxg_poa_batch_run_sharded over the engine's communicator): every rank runs the same iteration, rank 0 laces.
    A PoaGroup in place of the engine: sxg_poa_group_batch_run with the group as ctx -- every provider call of the iteration
    spreads over the group's members; the identity, split and sort providers take one of its members (group.member(i))."""
    L = engine.lib
    if isinstance(engine, _poa.PoaGroup):
        if sharded:
            raise ValueError("a device group runs in one process: it has no sharded entry")
        return C.cast(L.sxg_poa_group_batch_run, C.c_void_p), C.cast(L.sxg_poa_batch_free, C.c_void_p), engine.h
    run = C.cast(L.sxg_poa_batch_run_sharded if sharded else L.sxg_poa_batch_run, C.c_void_p)
    fre = C.cast(L.sxg_poa_batch_free, C.c_void_p)
    return run, fre, engine.h


def gpu_splitter(engine):
    """(split, free, ctx) backed by the GPU engine: sxg_poa_split_batch / sxg_poa_split_free of libsxgpoa.so and the
    engine handle -- the split provider of Smoother.split_blocks."""
    L = engine.lib
    return C.cast(L.sxg_poa_split_batch, C.c_void_p), C.cast(L.sxg_poa_split_free, C.c_void_p), engine.h


def gpu_mash_splitter(engine):
    """(split, free, ctx) backed by the GPU engine: sxg_poa_split_mash_batch / sxg_poa_split_free and the engine handle --
    the mash split provider of Smoother.split_blocks_mash."""
    L = engine.lib
    return C.cast(L.sxg_poa_split_mash_batch, C.c_void_p), C.cast(L.sxg_poa_split_free, C.c_void_p), engine.h


def gpu_sorter(engine):
    """(sort, ctx) backed by the GPU engine: sxg_poa_path_sgd_order of libsxgpoa.so and the engine handle -- the sort
    provider of prep_gfa."""
    return C.cast(engine.lib.sxg_poa_path_sgd_order, C.c_void_p), engine.h


def gpu_identifier(engine):
    """(identify, ctx) backed by the GPU engine: sxg_poa_block_identity_batch of libsxgpoa.so and the engine handle -- the
    identity provider of Smoother.identity_thresholds and of the `identity` keyword of smooth_gfa / smooth_maf_gfa: with
    adaptive_poa_params every block's identity estimate then runs on the device, in one call, before the POA calls."""
    return C.cast(engine.lib.sxg_poa_block_identity_batch, C.c_void_p), engine.h


def python_identifier(fn):
    """(identify, ctx) around a Python function fn(blk_off, seq_off, bases, kmer_size, min_len, percentile) -> (n_used,
    inter, uni, status) or (n_used, inter, uni, status, return code), one entry per block, the arrays being numpy copies of
    the batch the library coded: for tests and experiments, the production provider is gpu_identifier.  The tuple keeps the
    callback alive."""
    import numpy as np

    def view(ptr, n, dtype):
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)

    def call(ctx, inp, n_used, inter, uni, status):
        try:
            a = inp.contents
            blk_off = view(a.blk_off, a.n_blocks + 1, np.int32) if a.n_blocks else np.zeros(1, np.int32)
            seq_off = view(a.seq_off, int(blk_off[-1]) + 1, np.int64) if blk_off[-1] else np.zeros(1, np.int64)
            res = fn(blk_off, seq_off, view(a.bases, int(seq_off[-1]), np.uint8), a.kmer_size, a.min_len, a.percentile)
            for dst, src in zip((n_used, inter, uni, status), res[:4]):
                if len(src) != a.n_blocks:
                    return -1
                for k in range(a.n_blocks):
                    dst[k] = int(src[k])
            return int(res[4]) if len(res) > 4 else 0
        except Exception:   # (an exception must not cross the C frames)
            return -1
    cb = IDENT_FN(call)
    return C.cast(cb, C.c_void_p), None, cb


def gpu_repeat_scanner(engine):
    """(scan, ctx) backed by the GPU engine: sxg_poa_repeat_scan_batch of libsxgpoa.so and the engine handle -- the scan provider
    of the `scanner` key of Smoother's discover dict: the tandem-repeat scan of every range of every block that is cut then runs
    on the device, in one call (decree R).  For a device group pass one of its members: gpu_repeat_scanner(group.member(i))."""
    return C.cast(engine.lib.sxg_poa_repeat_scan_batch, C.c_void_p), engine.h


def python_repeat_scanner(fn):
    """(scan, ctx) around a Python function fn(seq_off, bases, min_copy, max_copy, stride) -> (n_lags, best, dev, v, status) or
    (n_lags, best, dev, v, status, return code), one entry per sequence, the arrays being numpy copies of the batch the library
    collected: for tests and experiments, the production provider is gpu_repeat_scanner.  The tuple keeps the callback alive."""
    import numpy as np

    def view(ptr, n, dtype):
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)

    def call(ctx, inp, n_lags, best, dev, v, status, match):
        try:
            a = inp.contents
            seq_off = view(a.seq_off, a.n_seqs + 1, np.int64) if a.n_seqs else np.zeros(1, np.int64)
            res = fn(seq_off, view(a.bases, int(seq_off[-1]), np.uint8), a.min_copy, a.max_copy, a.stride)
            for dst, src, conv in zip((n_lags, best, dev, v, status), res[:5], (int, int, float, float, int)):
                if len(src) != a.n_seqs:
                    return -1
                for k in range(a.n_seqs):
                    dst[k] = conv(src[k])
            return int(res[5]) if len(res) > 5 else 0
        except Exception:   # (an exception must not cross the C frames)
            return -1
    cb = REPEAT_FN(call)
    return C.cast(cb, C.c_void_p), None, cb


def gpu_range_scanner(engine):
    """gpu_repeat_scanner on RANGES: sxg_poa_repeat_scan_ranges and the engine handle.  The host library sends the candidates as
    ranges of the graph's path letters, which go to the device once per graph -- with this call or with gpu_range_identifier's,
    whichever comes first on the handle -- and a kernel cuts the sequences out there.  The same blocks, the same counts."""
    return RangeProvider((C.cast(engine.lib.sxg_poa_repeat_scan_ranges, C.c_void_p), engine.h))


def gpu_range_identifier(engine):
    """gpu_identifier on RANGES: sxg_poa_block_identity_ranges and the engine handle (see gpu_range_scanner); the letters are coded
    on the device.  The same thresholds, the same GFA."""
    return RangeProvider((C.cast(engine.lib.sxg_poa_block_identity_ranges, C.c_void_p), engine.h))


def _ranges_view(a, n):
    """(letters bytes per range) of a ranges call, read through the letters pointer the library passed"""
    import numpy as np
    L = a.letters.contents
    path_off = np.ctypeslib.as_array(L.path_off, shape=(L.n_paths + 1,))
    total = int(path_off[-1])
    letters = np.ctypeslib.as_array(L.letters, shape=(total,)) if total else np.zeros(0, np.uint8)
    out = []
    for s in range(n):
        r = a.ranges[s]
        if not (0 <= r.path < L.n_paths and 0 <= r.begin <= r.end <= path_off[r.path + 1] - path_off[r.path]) or a.letters_id != L.id or L.id == 0:
            raise ValueError("range outside its path")
        out.append(letters[path_off[r.path] + r.begin:path_off[r.path] + r.end].copy())
    return out


def python_range_scanner(fn):
    """python_repeat_scanner on RANGES: the same fn(seq_off, bases, min_copy, max_copy, stride), fed the sequences the ranges spell
    in the letters the library passed.  For CPU tests; the production provider is gpu_range_scanner."""
    import numpy as np

    def call(ctx, inp, n_lags, best, dev, v, status, match):
        try:
            a = inp.contents
            seqs = _ranges_view(a, a.n_seqs)
            seq_off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
            res = fn(seq_off, np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), a.min_copy, a.max_copy, a.stride)
            for dst, src, conv in zip((n_lags, best, dev, v, status), res[:5], (int, int, float, float, int)):
                if len(src) != a.n_seqs:
                    return -1
                for k in range(a.n_seqs):
                    dst[k] = conv(src[k])
            return int(res[5]) if len(res) > 5 else 0
        except Exception:   # (an exception must not cross the C frames)
            return -1
    cb = REPEAT_RANGES_FN(call)
    return RangeProvider((C.cast(cb, C.c_void_p), None, cb))


class MafTexter(tuple):
    """(letters, text, ctx[, keep-alive ...]): the MAF text provider of Smoother.smooth_maf_gfa(..., device_text=...)"""


def gpu_maf_texter(engine):
    """The MAF text provider backed by the GPU engine: sxg_poa_msa_row_letters and sxg_poa_maf_text of libsxgpoa.so and the engine
    handle -- the SAME engine the POA provider of the call runs on, whose trimmed rows then stay on the device
    (SXG_MSA_TRIMMED_RESIDENT) and leave it as MAF text.  A device group has no resident rows (they would lie on several members)."""
    if isinstance(engine, _poa.PoaGroup):
        raise ValueError("a device group keeps no resident MSA rows: the MAF text needs one engine")
    L = engine.lib
    return MafTexter((C.cast(L.sxg_poa_msa_row_letters, C.c_void_p), C.cast(L.sxg_poa_maf_text, C.c_void_p), engine.h))


def python_maf_texter(letters_fn, text_fn):
    """The MAF text provider around two Python functions, for CPU tests (the production provider is gpu_maf_texter):
    letters_fn() -> the letter count of every resident row (bytes other than '-'), rows counted block after block;
    text_fn(segs, literal) -> the text as bytes (or a uint8 array), segs a numpy array of poa.MAF_SEG_DTYPE (src, len, kind),
    literal the literal bytes as a uint8 array.  Either may return None, or raise, to fail the call.  The tuple keeps the callbacks
    alive."""
    import numpy as np

    def letters(ctx, out):
        try:
            res = letters_fn()
            if res is None:
                return -1
            for k, v in enumerate(res):
                out[k] = int(v)
            return 0
        except Exception:   # (an exception must not cross the C frames)
            return -1

    def text(ctx, inp, out, out_bytes):
        try:
            a = inp.contents
            segs = np.zeros(a.n_segs, _poa.MAF_SEG_DTYPE)
            if a.n_segs:
                C.memmove(segs.ctypes.data, a.segs, a.n_segs * C.sizeof(_poa.MafSeg))
            lit = np.ctypeslib.as_array(a.literal, shape=(a.literal_bytes,)).copy() if a.literal_bytes else np.zeros(0, np.uint8)
            res = text_fn(segs, lit)
            if res is None:
                return -1
            res = bytes(res) if not isinstance(res, np.ndarray) else res.astype(np.uint8).tobytes()
            if len(res) != out_bytes:
                return -1
            C.memmove(out, res, out_bytes)
            return 0
        except Exception:   # (an exception must not cross the C frames)
            return -1
    cl, ct = MSA_LETTERS_FN(letters), MAF_TEXT_FN(text)
    return MafTexter((C.cast(cl, C.c_void_p), C.cast(ct, C.c_void_p), None, cl, ct))


def python_range_identifier(fn):
    """python_identifier on RANGES: the same fn(blk_off, seq_off, bases, kmer_size, min_len, percentile), fed the sequences the
    ranges spell, coded by the table of the identity estimate.  For CPU tests; the production provider is gpu_range_identifier."""
    import numpy as np

    def call(ctx, inp, n_used, inter, uni, status):
        try:
            a = inp.contents
            blk_off = np.ctypeslib.as_array(a.blk_off, shape=(a.n_blocks + 1,)).astype(np.int32) if a.n_blocks else np.zeros(1, np.int32)
            seqs = [_poa.LETTERS_CODE[x] for x in _ranges_view(a, int(blk_off[-1]))]
            seq_off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
            res = fn(blk_off, seq_off, np.concatenate(seqs) if seqs else np.zeros(0, np.uint8), a.kmer_size, a.min_len, a.percentile)
            for dst, src in zip((n_used, inter, uni, status), res[:4]):
                if len(src) != a.n_blocks:
                    return -1
                for k in range(a.n_blocks):
                    dst[k] = int(src[k])
            return int(res[4]) if len(res) > 4 else 0
        except Exception:   # (an exception must not cross the C frames)
            return -1
    cb = IDENT_RANGES_FN(call)
    return RangeProvider((C.cast(cb, C.c_void_p), None, cb))


def python_sorter(fn):
    """(sort, ctx) around a Python function fn(node_len, path_off, step_node, step_pos, eta, cooling_start, terms_per_iter,
    seed) -> order (or (order, x)), the arrays being numpy copies of what the library flattened: for tests and experiments,
    the production provider is gpu_sorter.  The tuple keeps the callback alive."""
    import numpy as np

    def view(ptr, n, dtype):
        return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)

    def call(ctx, inp, order, x):
        try:
            a = inp.contents
            path_off = view(a.path_off, a.n_paths + 1, np.int64) if a.n_paths else np.zeros(1, np.int64)
            n_steps = int(path_off[-1])
            res = fn(view(a.node_len, a.n_nodes, np.int32), path_off, view(a.step_node, n_steps, np.int32), view(a.step_pos, n_steps, np.int64),
                     view(a.eta, a.iter_max, np.float64), a.cooling_start, a.terms_per_iter, a.seed)
            ord_ = np.asarray(res[0] if isinstance(res, tuple) else res, np.int32)
            if len(ord_) != a.n_nodes:
                return -1
            for k in range(a.n_nodes):
                order[k] = int(ord_[k])
            return 0
        except Exception:   # (an exception must not cross the C frames)
            return -1
    cb = SGD_FN(call)
    return C.cast(cb, C.c_void_p), None, cb


def prep_gfa(text, sorter, **params):
    """prep (sxg_graph_prep): the GFA sorted by path-guided SGD -- the order comes from `sorter`, gpu_sorter(engine) in
    production -- and chopped to nodes of at most max_node_length bases.  params: fields of sxg_prep_params
    (max_node_length, term_updates, iter_max, eps, cooling, seed, mode).  A prepped smoothing iteration is
    Smoother(prep_gfa(text, gpu_sorter(engine)), discover=...)."""
    L = load_library()
    pp = PrepParams()
    L.sxg_prep_default_params(C.byref(pp))
    for k, v in params.items():
        if k not in dict(PrepParams._fields_) or k == "struct_size":
            raise TypeError("prep_gfa: no such parameter: " + k)
        setattr(pp, k, v)
    data = text.encode() if isinstance(text, str) else text
    g, out = C.c_void_p(), C.c_void_p()
    if L.sxg_graph_from_gfa(data, len(data), C.byref(g)):
        raise SmoothError(L.sxg_smooth_last_error().decode())
    try:
        if L.sxg_graph_prep(g, C.byref(pp), sorter[0], sorter[1], None, C.byref(out)):
            raise SmoothError(L.sxg_smooth_last_error().decode())
        try:
            return C.string_at(out).decode()
        finally:
            L.sxg_smooth_free(out)
    finally:
        L.sxg_graph_free(g)


class Smoother:
    """An input GFA + a blockset; collect / block graph / full iteration through the C ABI."""

    def __init__(self, gfa_text, target_bp=None, blocks=None, discover=None):
        """discover: block discovery as smoothxg does it -- a dict with target_poa_length and n_haps (and optionally
        max_path_jump, max_edge_jump, max_poa_length, repeats, scanner): smoothable_blocks then the cutting half of break_blocks
        (repeat-aware cut lengths with the reference's defaults unless repeats=None).  scanner: a scan provider
        (gpu_repeat_scanner(engine): the tandem-repeat scan of all cut blocks in ONE call on the device, sxg_blockset_break_scan;
        the counts it reports are kept in self.break_counts; gpu_range_scanner(engine): the same through sxg_blockset_break_scan_ranges,
        the candidates sent as ranges of the graph's path letters); without the key the host scans, as it always did.
        blocks: the caller's own blockset -- a list of blocks, each a list of (path, step_begin, step_end)
        or (path, step_begin, step_end, length) in alignment order (sxg_blockset_from_ranges); otherwise the
        demo partition into path windows of target_bp."""
        self.L = load_library()
        data = gfa_text.encode() if isinstance(gfa_text, str) else gfa_text
        g = C.c_void_p()
        if self.L.sxg_graph_from_gfa(data, len(data), C.byref(g)):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        self.g = g
        b = C.c_void_p()
        if discover is not None:
            tl = int(discover["target_poa_length"])
            raw = C.c_void_p()
            rc = self.L.sxg_blockset_smoothable(g, int(discover.get("max_block_weight", tl * int(discover["n_haps"]))), tl,
                                                int(discover.get("max_path_jump", 100)), int(discover.get("max_edge_jump", 0)), 1,
                                                C.byref(raw))
            if not rc:
                rep = discover.get("repeats", (1000, 20000, 5, 50))   # (min_copy_length, max_copy_length, min_autocorr_z, autocorr_stride) or None
                if rep is None:
                    rc = self.L.sxg_blockset_break_ex(g, raw, int(discover.get("max_poa_length", 2 * tl)), 0, 1000, 20000, 5.0, 50, 1, C.byref(b))
                elif "scanner" in discover:
                    scan = discover["scanner"]
                    counts = [C.c_int64(), C.c_int64(), C.c_int64()]
                    call = self.L.sxg_blockset_break_scan_ranges if isinstance(scan, RangeProvider) else self.L.sxg_blockset_break_scan
                    rc = call(g, raw, int(discover.get("max_poa_length", 2 * tl)), int(rep[0]), int(rep[1]), float(rep[2]),
                              int(rep[3]), 1, scan[0], scan[1], C.byref(b), *(C.byref(c) for c in counts))
                    self.break_counts = tuple(c.value for c in counts)   # (blocks cut, of which at a repeat, sequences the scanner declined)
                else:
                    rc = self.L.sxg_blockset_break_ex(g, raw, int(discover.get("max_poa_length", 2 * tl)), 1, int(rep[0]), int(rep[1]),
                                                      float(rep[2]), int(rep[3]), 1, C.byref(b))
                self.L.sxg_blockset_free(raw)
        elif blocks is not None:
            flat = [r for blk in blocks for r in blk]
            arr = (PathRange * max(len(flat), 1))(*[PathRange(r[0], r[1], r[2], r[3] if len(r) > 3 else 0) for r in flat])
            off = (C.c_int64 * (len(blocks) + 1))()
            for k, blk in enumerate(blocks):
                off[k + 1] = off[k] + len(blk)
            rc = self.L.sxg_blockset_from_ranges(g, len(blocks), off, arr, C.byref(b))
        else:
            rc = self.L.sxg_blockset_by_path_windows(g, target_bp, C.byref(b))
        if rc:
            msg = self.L.sxg_smooth_last_error().decode()
            self.L.sxg_graph_free(g)
            self.g = None
            raise SmoothError(msg)
        self.b = b

    def path_letters(self):
        """sxg_graph_path_letters: the graph's path letters as a PathLetters (id, path_off, letters) -- what the range providers
        read; built once per graph and cached in it.  The arrays are copies."""
        import numpy as np
        li = _poa.LettersIn()
        if self.L.sxg_graph_path_letters(self.g, C.byref(li)):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        path_off = np.ctypeslib.as_array(li.path_off, shape=(li.n_paths + 1,)).copy()
        letters = np.ctypeslib.as_array(li.letters, shape=(int(path_off[-1]),)).copy() if path_off[-1] else np.zeros(0, np.uint8)
        return _poa.PathLetters(path_off=path_off, letters=letters, id=li.id)

    def block_ranges(self, block_id):
        """The ranges of a block as (path, step_begin, step_end, length) tuples."""
        n = self.L.sxg_blockset_block_size(self.b, block_id)
        if n < 0:
            raise SmoothError("no such block")
        arr = (PathRange * max(n, 1))()
        if self.L.sxg_blockset_block_ranges(self.b, block_id, arr):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        return [(arr[k].path, arr[k].step_begin, arr[k].step_end, arr[k].length) for k in range(n)]

    def split_blocks(self, splitter, block_id_min, ratio_min=0.0, min_dedup_depth=0):
        """The splitting half of break_blocks (sxg_blockset_split; -I, -R and the dedup depth of the reference, whose
        default depth 0 means "never split"): REPLACES the blockset.  Returns (blocks split, blocks left whole because
        the provider could not take them)."""
        split, fre, ctx = splitter
        nb, ns, nl = C.c_void_p(), C.c_int64(), C.c_int64()
        if self.L.sxg_blockset_split(self.g, self.b, float(block_id_min), float(ratio_min), int(min_dedup_depth), split, fre, ctx,
                                     C.byref(nb), C.byref(ns), C.byref(nl)):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        self.L.sxg_blockset_free(self.b)
        self.b = nb
        return ns.value, nl.value

    def split_blocks_mash(self, splitter, block_id_min, ratio_min=0.0, min_dedup_depth=0, min_len_mash=200, min_depth_mash=12000,
                          est_identity=0.0, kmer_size=17):
        """split_blocks with the mash-based branch (sxg_blockset_split_mash; -L, -D, -e and -k of the reference, with its
        defaults): a block of at least min_depth_mash dedup'd sequences (0: every block) compares its sequences of at least
        min_len_mash bases by their k-mer sets; est_identity <= 0 means block_id_min.  splitter: a mash split provider
        (gpu_mash_splitter).  REPLACES the blockset; returns as split_blocks does."""
        split, fre, ctx = splitter
        nb, ns, nl = C.c_void_p(), C.c_int64(), C.c_int64()
        if self.L.sxg_blockset_split_mash(self.g, self.b, float(block_id_min), float(ratio_min), int(min_dedup_depth), int(min_len_mash),
                                          int(min_depth_mash), float(est_identity), int(kmer_size), split, fre, ctx,
                                          C.byref(nb), C.byref(ns), C.byref(nl)):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        self.L.sxg_blockset_free(self.b)
        self.b = nb
        return ns.value, nl.value

    def close(self):
        if getattr(self, "b", None):
            self.L.sxg_blockset_free(self.b)
            self.b = None
        if getattr(self, "g", None):
            self.L.sxg_graph_free(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_blocks(self):
        return self.L.sxg_blockset_size(self.b)

    def _text(self, rc, out):
        if rc:
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        try:
            return C.string_at(out).decode()
        finally:
            self.L.sxg_smooth_free(out)

    def identity_threshold(self, block_id, kmer_size=17):
        """A14: (threshold, sequences used); the threshold only counts when more than one was used."""
        thr, n = C.c_float(), C.c_int32()
        if self.L.sxg_block_identity_threshold(self.g, self.b, block_id, kmer_size, C.byref(thr), C.byref(n)):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        return thr.value, n.value

    def collect_text(self, block_id, params):
        out = C.c_void_p()
        return self._text(self.L.sxg_block_collect_text(self.g, self.b, block_id, C.byref(params), C.byref(out)), out)

    def block_graph_gfa(self, block_id, params, provider):
        run, fre, ctx = provider
        out = C.c_void_p()
        return self._text(self.L.sxg_block_graph_gfa(self.g, self.b, block_id, C.byref(params), run, fre, ctx, C.byref(out)), out)

    def block_maf_rows(self, block_id, params, provider):
        run, fre, ctx = provider
        out = C.c_void_p()
        return self._text(self.L.sxg_block_maf_rows(self.g, self.b, block_id, C.byref(params), run, fre, ctx, C.byref(out)), out)

    def block_maf(self, block_id, params, provider):
        run, fre, ctx = provider
        out = C.c_void_p()
        return self._text(self.L.sxg_block_maf(self.g, self.b, block_id, C.byref(params), run, fre, ctx, C.byref(out)), out)

    def identity_thresholds(self, kmer_size=17, identity=None, max_depth=1000):
        """A14 for every block (sxg_blockset_identity_thresholds): (thresholds as float32, sequences used as int32), one entry
        per block; a threshold only counts where more than one sequence was used, and a block with at most one range or more
        than max_depth ranges reports 0 used.  identity: an identity provider (gpu_identifier(engine): ONE call on the device
        for all blocks); None = the host estimator, block by block over the host threads."""
        import numpy as np
        n = self.n_blocks
        thr, used = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32)
        ident = identity if identity is not None else (None, None)
        call = self.L.sxg_blockset_identity_thresholds_ranges if isinstance(ident, RangeProvider) else self.L.sxg_blockset_identity_thresholds
        if call(self.g, self.b, int(kmer_size), int(max_depth), ident[0], ident[1],
                thr.ctypes.data_as(C.POINTER(C.c_float)), used.ctypes.data_as(C.POINTER(C.c_int32))):
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        return thr[:n], used[:n]

    def smooth_maf_gfa(self, params, provider, merge_blocks=False, jaccard=1.0, preserve_unmerged=False, max_groups=50, header=None,
                       identity=None, device_rows=False, device_text=None):
        """The iteration with the in-order MAF consumer (block merging, flips): -> (GFA text, MAF text, flipped blocks).
        device_text=texter (gpu_maf_texter(engine), the engine of `provider`): sxg_smooth_maf_gfa_device_text -- without
        merge_blocks the trimmed rows stay on the device and the MAF text is laid out there; identity: None or a range provider
        (gpu_range_identifier).  With merge_blocks it is device_rows=True.  Same outputs.
        identity: as for smooth_gfa.  device_rows=True: sxg_smooth_maf_gfa_device_rows -- without merge_blocks the provider
        builds the trimmed MSA rows (SXG_MSA_TRIMMED: the GPU engine does, on the device) and the iteration laces compact
        block graphs; same outputs."""
        run, fre, ctx = provider
        ident = identity if identity is not None else (None, None)
        mp = MergeParams()
        self.L.sxg_merge_default_params(C.byref(mp))
        mp.merge_blocks, mp.contiguous_path_jaccard, mp.preserve_unmerged_consensus = int(merge_blocks), jaccard, int(preserve_unmerged)
        mp.max_merged_groups_in_memory = max_groups
        mp.maf_header = header.encode() if header is not None else None
        gfa, maf, nf = C.c_void_p(), C.c_void_p(), C.c_int64()
        call = self.L.sxg_smooth_maf_gfa_device_rows if device_rows else self.L.sxg_smooth_maf_gfa_adaptive
        if device_text is not None:
            if not isinstance(device_text, MafTexter):
                raise TypeError("device_text takes gpu_maf_texter(engine) or python_maf_texter(...)")
            if identity is not None and not isinstance(ident, RangeProvider):
                raise ValueError("device_text takes the identity estimate over ranges (gpu_range_identifier) or none")
            tp = MafTextProvider(device_text[0], device_text[1], device_text[2])
            rp = RangeProviders(None, ident[0], ident[1]) if identity is not None else None
            rc = self.L.sxg_smooth_maf_gfa_device_text(self.g, self.b, C.byref(params), C.byref(mp), run, fre, ctx, C.byref(tp),
                                                       C.byref(rp) if rp is not None else None, C.byref(gfa), C.byref(maf), C.byref(nf))
        elif isinstance(ident, RangeProvider):
            rp = RangeProviders(None, ident[0], ident[1])
            rc = self.L.sxg_smooth_iteration_ranges(self.g, self.b, C.byref(params), C.byref(mp), run, fre, ctx, C.byref(rp), int(bool(device_rows)),
                                                    C.byref(gfa), C.byref(maf), C.byref(nf))
        else:
            rc = call(self.g, self.b, C.byref(params), C.byref(mp), run, fre, ctx, ident[0], ident[1], C.byref(gfa), C.byref(maf), C.byref(nf))
        if rc:
            raise SmoothError(self.L.sxg_smooth_last_error().decode())
        try:
            return C.string_at(gfa).decode(), C.string_at(maf).decode(), nf.value
        finally:
            self.L.sxg_smooth_free(gfa)
            self.L.sxg_smooth_free(maf)

    def smooth_gfa(self, params, provider, identity=None):
        """One smoothing iteration -> GFA text; None on a rank of a multi-GPU provider that does not lace.
        identity: an identity provider for adaptive_poa_params (gpu_identifier(engine): the estimates of all blocks in one
        device call before the POA calls; gpu_range_identifier(engine): the same on ranges of the resident path letters); None = the host estimator.  Without adaptive_poa_params it is never called."""
        run, fre, ctx = provider
        ident = identity if identity is not None else (None, None)
        out = C.c_void_p()
        if isinstance(ident, RangeProvider):
            rp = RangeProviders(None, ident[0], ident[1])
            rc = self.L.sxg_smooth_iteration_ranges(self.g, self.b, C.byref(params), None, run, fre, ctx, C.byref(rp), 0, C.byref(out), None, None)
        else:
            rc = self.L.sxg_smooth_gfa_adaptive(self.g, self.b, C.byref(params), run, fre, ctx, ident[0], ident[1], C.byref(out))
        if rc == 1:   # SXG_NOT_ROOT
            return None
        return self._text(rc, out)

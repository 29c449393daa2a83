"""ctypes binding of the C ABI in include/sxg_poa.h (libsxgpoa.so, HIP/gfx950).

This is the host-side mirror of the reference's per-block POA call sequence
(src/smooth.cpp:752-786): `PoaEngine.run_blocks` takes what smooth_spoa has after its
dedup step (sequences, weights, the six scores in spoa's sign convention, local/global) and
returns what build_odgi_SPOA consumes (nodes, edges, per-sequence node paths, consensus).
There is NO CPU fallback: a missing library or GPU raises.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MODE_LOCAL, MODE_GLOBAL = 0, 1
ORDER_SPOA = 0x10   # SXG_ORDER_SPOA, OR-ed into Params.mode: spoa's depth-first re-sort after every alignment (decree S7')
IDS_SPOA = 0x20     # SXG_IDS_SPOA, only with ORDER_SPOA: new node ids in spoa's AddAlignment order (decree S6')


class Params(C.Structure):
    _fields_ = [("m", C.c_int8), ("n", C.c_int8), ("g", C.c_int8), ("e", C.c_int8),
                ("q", C.c_int8), ("c", C.c_int8), ("mode", C.c_uint8), ("banded", C.c_uint8)]


def params_from_cli(m=1, n=4, g=6, e=2, q=26, c=1, local=True):
    """smoothxg CLI values (positive penalties, src/main.cpp:322-361) -> spoa convention
    exactly as src/smooth.cpp:2098-2106 negates them."""
    return Params(m, -n, -g, -e, -q, -c, MODE_LOCAL if local else MODE_GLOBAL, 0)


_i32p, _i64p, _u8p, _u32p, _u64p = (C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8),
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint64))


class BatchIn(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("blk_off", _i32p), ("seq_off", _i64p), ("bases", _u8p),
                ("weights", _u32p), ("params", C.POINTER(Params)), ("per_block_params", C.c_int32),
                ("want_consensus", C.c_int32), ("want_msa", C.c_int32),
                ("want_block_graph", C.c_int32), ("bg_consensus_visited_only", C.c_int32), ("bg_trim", _i32p)]


class BatchOut(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_seqs", C.c_int64), ("status", _i32p), ("node_off", _i64p),
                ("node_code", _u8p), ("node_rank", _i32p), ("node_group", _i32p), ("edge_off", _i64p),
                ("edge_tail", _i32p), ("edge_head", _i32p), ("edge_weight", _u32p),
                ("seq_path_nodes", _i32p), ("score", _i32p), ("cells", _u64p), ("cons_off", _i64p),
                ("cons_nodes", _i32p), ("msa_off", _i64p), ("msa_cols", _i32p), ("msa", C.c_void_p),
                ("bg_node_off", _i64p), ("bg_node_len", _i32p), ("bg_node_outdeg", _i32p), ("bg_node_indeg", _u8p),
                ("bg_seq_off", _i64p), ("bg_seq", C.c_void_p), ("bg_edge_off", _i64p), ("bg_edge_to", _i32p),
                ("bg_step_off", _i64p), ("bg_steps", _i32p), ("bg_cons_off", _i64p), ("bg_cons_steps", _i32p),
                ("block_cycles", _u64p), ("_owner", C.c_void_p)]


class AlignIn(C.Structure):
    _fields_ = [("n", C.c_int32), ("row_off", _i64p), ("row_code", _u8p), ("row_sink", _u8p),
                ("pred_off", _i64p), ("preds", _i32p), ("seq_off", _i64p), ("bases", _u8p),
                ("params", C.POINTER(Params)), ("per_problem_params", C.c_int32)]


class AlignOut(C.Structure):
    _fields_ = [("n", C.c_int32), ("status", _i32p), ("score", _i32p), ("pair_off", _i64p),
                ("pair_row", _i32p), ("pair_pos", _i32p), ("_owner", C.c_void_p)]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("cells", C.c_uint64), ("dp_launches", C.c_uint64),
                ("algo_bytes", C.c_uint64), ("n_slots", C.c_int32), ("retries", C.c_int32),
                ("device_bytes", C.c_uint64), ("dom_kernel_ms", C.c_double), ("dom_cells", C.c_uint64),
                ("dom_algo_bytes", C.c_uint64), ("dom_threads", C.c_int32), ("dom_cols_per_lane", C.c_int32),
                ("dom_row_mode", C.c_int32), ("dom_clock_mhz", C.c_int32), ("bg_ms", C.c_double)]


class WidthStats(C.Structure):
    """sxg_poa_width_stats: the packed sweeps of the last execute per strip width ([0] the geometry's, [1] the second width)."""
    _fields_ = [("sweeps", C.c_uint64 * 2), ("swept_cols", C.c_uint64 * 2), ("swept_cells", C.c_uint64 * 2),
                ("hint_shift_repeats", C.c_uint64), ("dom_width", C.c_int32), ("dom_width2", C.c_int32)]


class TwinStats(C.Structure):
    """sxg_poa_twin_stats: twin steps and join rows of the last execute (packed classes with the twin step)."""
    _fields_ = [("twin_steps", C.c_uint64), ("join_rows", C.c_uint64)]


class DeviceView(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_seqs", C.c_int64), ("n_bases", C.c_int64),
                ("status", C.c_void_p), ("n_nodes", C.c_void_p), ("n_edges", C.c_void_p),
                ("node_code", C.c_void_p), ("node_rank", C.c_void_p), ("node_group", C.c_void_p),
                ("edge_tail", C.c_void_p), ("edge_head", C.c_void_p), ("edge_weight", C.c_void_p),
                ("seq_path_nodes", C.c_void_p), ("score", C.c_void_p)]


class SplitIn(C.Structure):
    """sxg_poa_split_in: blocks of dedup'd, sorted sequences with their identity threshold and length ratio."""
    _fields_ = [("n_blocks", C.c_int32), ("blk_off", _i32p), ("seq_off", _i64p), ("bases", _u8p),
                ("identity", C.POINTER(C.c_double)), ("length_ratio_min", C.POINTER(C.c_double))]


class SplitOut(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_seqs", C.c_int64), ("group", _i32p), ("n_groups", _i32p),
                ("n_pairs", _i64p), ("status", _i32p), ("_owner", C.c_void_p)]


class SplitMash(C.Structure):
    """sxg_poa_split_mash: the k-mer size and, per block, the least length of a sequence compared by its k-mer set (0: the
    block runs the edit-based walk only) and the estimated-identity threshold."""
    _fields_ = [("kmer_size", C.c_int32), ("min_len", _i32p), ("est_identity", C.POINTER(C.c_double))]


class IdentityIn(C.Structure):
    """sxg_poa_identity_in: blocks of coded sequences for the identity estimate of the adaptive scores (decree Q)."""
    _fields_ = [("n_blocks", C.c_int32), ("blk_off", _i32p), ("seq_off", _i64p), ("bases", _u8p), ("kmer_size", C.c_int32),
                ("min_len", C.c_int32), ("percentile", C.c_double)]


class RepeatIn(C.Structure):
    """sxg_poa_repeat_in: a flat set of sequences (the letters as they are) and the parameters of the tandem-repeat scan (decree R)."""
    _fields_ = [("n_seqs", C.c_int64), ("seq_off", _i64p), ("bases", _u8p), ("min_copy", C.c_uint64), ("max_copy", C.c_uint64),
                ("stride", C.c_uint64)]


class LettersIn(C.Structure):
    """sxg_poa_letters: a graph's path letters on the host (the bytes as they stand, step orientation) and the id that names them."""
    _fields_ = [("id", C.c_uint64), ("n_paths", C.c_int64), ("path_off", _i64p), ("letters", _u8p)]


class Range(C.Structure):
    """sxg_poa_range: letters [begin, end) of `path`."""
    _fields_ = [("path", C.c_int64), ("begin", C.c_int64), ("end", C.c_int64)]


class RepeatRangesIn(C.Structure):
    """sxg_poa_repeat_ranges_in: the repeat scan's sequences as ranges of the resident letters."""
    _fields_ = [("letters", C.POINTER(LettersIn)), ("letters_id", C.c_uint64), ("n_seqs", C.c_int64), ("ranges", C.POINTER(Range)),
                ("min_copy", C.c_uint64), ("max_copy", C.c_uint64), ("stride", C.c_uint64)]


class IdentityRangesIn(C.Structure):
    """sxg_poa_identity_ranges_in: the identity estimate's blocks as ranges of the resident letters."""
    _fields_ = [("letters", C.POINTER(LettersIn)), ("letters_id", C.c_uint64), ("n_blocks", C.c_int32), ("blk_off", _i32p),
                ("ranges", C.POINTER(Range)), ("kmer_size", C.c_int32), ("min_len", C.c_int32), ("percentile", C.c_double)]


class SgdIn(C.Structure):
    """sxg_poa_sgd_in: the flattened graph, the schedule and the seed of the path-guided SGD node order (decree Y)."""
    _fields_ = [("n_nodes", C.c_int64), ("node_len", _i32p), ("n_paths", C.c_int64), ("path_off", _i64p), ("step_node", _i32p),
                ("step_pos", _i64p), ("iter_max", C.c_int32), ("cooling_start", C.c_int32), ("eta", C.POINTER(C.c_double)),
                ("terms_per_iter", C.c_uint64), ("seed", C.c_uint64), ("mode", C.c_int32)]


SGD_LDS_NODES = 8192   # SXG_POA_SGD_LDS_NODES: nodes the one-workgroup path of the SGD order keeps on chip
MASH_SORT_TILE = 1024   # SXG_POA_MASH_SORT_TILE: k-mers a workgroup sorts on chip at once
SPLIT_PANEL = 512   # SXG_POA_SPLIT_PANEL: columns of the second sequence a wavefront sweeps at once
MAX_SEQ_LEN = 26623  # SXG_POA_MAX_SEQ_LEN
REPEAT_MAX_LEN = 1 << 20   # SXG_POA_REPEAT_MAX_LEN: the longest sequence the repeat scan takes (decree R4)
MAX_SEQ_LEN_TILED = 49151  # SXG_POA_MAX_SEQ_LEN_TILED: every mode and score set, with set_long_blocks(True)
ST_TOO_LONG = 5
MSA_FULL, MSA_TRIMMED = 1, 2   # SXG_MSA_FULL / SXG_MSA_TRIMMED: values of want_msa (True = the full MSA)
MSA_TRIMMED_RESIDENT = 3       # SXG_MSA_TRIMMED_RESIDENT: the trimmed rows stay on the device (msa_row_letters, maf_text)
MAF_LITERAL, MAF_ROW, MAF_ROW_REVCOMP = 0, 1, 2   # sxg_poa_maf_seg::kind

EXPORTS = ["sxg_poa_letters_upload", "sxg_poa_letters_drop", "sxg_poa_letters_resident", "sxg_poa_letters_stats", "sxg_poa_letters_geometry", "sxg_poa_range_gather",
           "sxg_poa_repeat_scan_ranges", "sxg_poa_block_identity_ranges", "sxg_poa_repeat_scan_batch", "sxg_poa_block_identity_batch", "sxg_poa_path_sgd_order", "sxg_poa_kmer_jaccard_batch", "sxg_poa_split_mash_batch", "sxg_poa_pair_identity_batch", "sxg_poa_split_batch", "sxg_poa_split_free", "sxg_poa_batch_device_view", "sxg_poa_abi_version", "sxg_poa_device_count", "sxg_poa_compute_units", "sxg_poa_last_error", "sxg_poa_create",
           "sxg_poa_destroy", "sxg_poa_batch_run", "sxg_poa_batch_upload", "sxg_poa_batch_execute",
           "sxg_poa_batch_download", "sxg_poa_batch_free", "sxg_poa_align_batch", "sxg_poa_align_free",
           "sxg_poa_get_stats", "sxg_poa_get_width_stats", "sxg_poa_get_twin_stats", "sxg_poa_set_memory_budget", "sxg_xxh64", "sxg_poa_comm_unique_id", "sxg_poa_comm_init",
           "sxg_poa_comm_attach", "sxg_poa_comm_destroy", "sxg_poa_batch_run_sharded", "sxg_poa_batch_run_sharded_local",
           "sxg_poa_batch_upload_sharded", "sxg_poa_batch_execute_sharded", "sxg_poa_batch_download_sharded", "sxg_poa_sharded_info",
           "sxg_poa_sharded_timing", "sxg_poa_measure_copy", "sxg_poa_roctx_available", "sxg_poa_get_msa_stats", "sxg_poa_msa_geometry",
           "sxg_poa_group_create", "sxg_poa_group_destroy", "sxg_poa_group_size", "sxg_poa_group_member", "sxg_poa_group_set_memory_budget",
           "sxg_poa_group_batch_run", "sxg_poa_group_batch_upload", "sxg_poa_group_batch_execute", "sxg_poa_group_batch_download",
           "sxg_poa_group_timing", "sxg_poa_set_long_blocks", "sxg_poa_group_set_long_blocks", "sxg_poa_get_tile_stats",
           "sxg_poa_msa_row_letters", "sxg_poa_maf_text", "sxg_poa_maf_text_geometry", "sxg_poa_maf_text_stats"]
COMM_ID_BYTES = 128
NOT_ROOT = 1

_lib = None


def load_library(build_if_missing=True):
    """Loads libsxgpoa.so; raises if it is missing and cannot be built."""
    global _lib
    if _lib is not None:
        return _lib
    so = os.environ.get("SXG_POA_LIB", _build.SO)  # override: A/B builds of the same source
    if not os.path.exists(so):
        if not build_if_missing:
            raise RuntimeError("libsxgpoa.so is missing: run `python -m smoothxg_amd.build`")
        _build.build()
    L = C.CDLL(so)
    vp = C.c_void_p
    L.sxg_poa_last_error.restype = C.c_char_p
    L.sxg_poa_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.sxg_poa_destroy.argtypes = [vp]
    L.sxg_poa_batch_run.argtypes = [vp, C.POINTER(BatchIn), C.POINTER(BatchOut)]
    L.sxg_poa_batch_upload.argtypes = [vp, C.POINTER(BatchIn)]
    L.sxg_poa_batch_execute.argtypes = [vp]
    L.sxg_poa_batch_download.argtypes = [vp, C.POINTER(BatchOut)]
    L.sxg_poa_batch_free.argtypes = [C.POINTER(BatchOut)]
    L.sxg_poa_batch_device_view.argtypes = [vp, C.POINTER(DeviceView)]
    L.sxg_poa_align_batch.argtypes = [vp, C.POINTER(AlignIn), C.POINTER(AlignOut)]
    L.sxg_poa_align_free.argtypes = [C.POINTER(AlignOut)]
    L.sxg_poa_compute_units.argtypes = [vp]
    L.sxg_poa_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.sxg_poa_get_width_stats.argtypes = [vp, C.POINTER(WidthStats)]
    L.sxg_poa_get_twin_stats.argtypes = [vp, C.POINTER(TwinStats)]
    L.sxg_poa_set_memory_budget.argtypes = [vp, C.c_uint64]
    L.sxg_poa_set_long_blocks.argtypes = [vp, C.c_int]
    L.sxg_poa_group_set_long_blocks.argtypes = [vp, C.c_int]
    L.sxg_poa_get_tile_stats.argtypes = [vp, _i64p, _i64p, _i64p]
    L.sxg_poa_get_msa_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sxg_poa_msa_geometry.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.sxg_poa_msa_geometry.restype = None
    L.sxg_poa_measure_copy.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(C.c_double)]
    L.sxg_poa_comm_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.sxg_poa_comm_init.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int, C.c_int]
    L.sxg_poa_comm_attach.argtypes = [vp, vp, C.c_int, C.c_int]
    L.sxg_poa_comm_destroy.argtypes = [vp]
    L.sxg_poa_comm_destroy.restype = None
    L.sxg_poa_batch_run_sharded.argtypes = [vp, C.POINTER(BatchIn), C.POINTER(BatchOut)]
    L.sxg_poa_batch_run_sharded_local.argtypes = [vp, C.POINTER(BatchIn), C.c_int, C.POINTER(BatchOut)]
    L.sxg_poa_batch_upload_sharded.argtypes = [vp, C.POINTER(BatchIn)]
    L.sxg_poa_batch_execute_sharded.argtypes = [vp]
    L.sxg_poa_batch_download_sharded.argtypes = [vp, C.POINTER(BatchIn), C.POINTER(BatchOut)]
    L.sxg_poa_sharded_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    L.sxg_poa_sharded_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sxg_poa_group_create.argtypes = [_i32p, C.c_int32, C.POINTER(vp)]
    L.sxg_poa_group_destroy.argtypes = [vp]
    L.sxg_poa_group_destroy.restype = None
    L.sxg_poa_group_size.argtypes = [vp]
    L.sxg_poa_group_member.argtypes = [vp, C.c_int32]
    L.sxg_poa_group_member.restype = vp
    L.sxg_poa_group_set_memory_budget.argtypes = [vp, C.c_uint64]
    L.sxg_poa_group_batch_run.argtypes = [vp, C.POINTER(BatchIn), C.POINTER(BatchOut)]
    L.sxg_poa_group_batch_upload.argtypes = [vp, C.POINTER(BatchIn)]
    L.sxg_poa_group_batch_execute.argtypes = [vp]
    L.sxg_poa_group_batch_download.argtypes = [vp, C.POINTER(BatchOut)]
    L.sxg_poa_group_timing.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.sxg_poa_pair_identity_batch.argtypes = [vp, C.c_int64, _i64p, _u8p, C.c_int64, _i32p, _i32p, _u8p, _i32p, _i32p, _i32p, _i32p]
    L.sxg_poa_split_batch.argtypes = [vp, C.POINTER(SplitIn), C.POINTER(SplitOut)]
    L.sxg_poa_split_free.argtypes = [C.POINTER(SplitOut)]
    L.sxg_poa_kmer_jaccard_batch.argtypes = [vp, C.c_int64, _i64p, _u8p, C.c_int32, C.c_int64, _i32p, _i32p, _i32p, _i32p, C.POINTER(C.c_uint64)]
    L.sxg_poa_split_mash_batch.argtypes = [vp, C.POINTER(SplitIn), C.POINTER(SplitMash), C.POINTER(SplitOut), _i64p]
    L.sxg_poa_split_free.restype = None
    L.sxg_poa_block_identity_batch.argtypes = [vp, C.POINTER(IdentityIn), _i32p, _i32p, _i32p, _i32p]
    L.sxg_poa_path_sgd_order.argtypes = [vp, C.POINTER(SgdIn), _i32p, _i64p]
    L.sxg_poa_repeat_scan_batch.argtypes = [vp, C.POINTER(RepeatIn), _i32p, _i32p, C.POINTER(C.c_double), C.POINTER(C.c_double), _i32p, _i32p]
    L.sxg_poa_letters_upload.argtypes = [vp, C.POINTER(LettersIn)]
    L.sxg_poa_letters_drop.argtypes = [vp]
    L.sxg_poa_letters_drop.restype = None
    L.sxg_poa_letters_resident.argtypes = [vp, C.POINTER(C.c_uint64), _i64p, _i64p]
    L.sxg_poa_letters_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sxg_poa_letters_geometry.argtypes = [C.POINTER(C.c_int32)]
    L.sxg_poa_letters_geometry.restype = None
    L.sxg_poa_msa_row_letters.argtypes = [vp, _i32p]
    L.sxg_poa_maf_text.argtypes = [vp, C.POINTER(MafTextIn), C.c_void_p, C.c_int64]
    L.sxg_poa_maf_text_geometry.argtypes = [C.POINTER(C.c_int32)]
    L.sxg_poa_maf_text_geometry.restype = None
    L.sxg_poa_maf_text_stats.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    L.sxg_poa_range_gather.argtypes = [vp, C.POINTER(LettersIn), C.c_uint64, C.c_int64, C.POINTER(Range), C.c_int, _u8p]
    L.sxg_poa_repeat_scan_ranges.argtypes = [vp, C.POINTER(RepeatRangesIn), _i32p, _i32p, C.POINTER(C.c_double), C.POINTER(C.c_double), _i32p, _i32p]
    L.sxg_poa_block_identity_ranges.argtypes = [vp, C.POINTER(IdentityRangesIn), _i32p, _i32p, _i32p, _i32p]
    L.sxg_xxh64.restype = C.c_uint64
    L.sxg_xxh64.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]
    _lib = L
    return L


class PoaError(RuntimeError):
    pass


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class PathLetters:
    """A graph's path letters on the host, as the engine takes them (sxg_poa_letters): `letters`, the paths' spelled sequences
    back to back, `path_off` [n_paths + 1], and the non-zero `id` that names them on a handle.  Built from a list of byte strings
    or uint8 arrays, or from (path_off, letters) arrays that are used as they are; id: None = a fresh one in this process."""
    _next_id = [1]

    def __init__(self, paths=None, path_off=None, letters=None, id=None):
        if paths is not None:
            arrs = [np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.asarray(x, np.uint8) for x in paths]
            path_off = np.zeros(len(arrs) + 1, np.int64)
            if arrs:
                path_off[1:] = np.cumsum([len(a) for a in arrs])
            letters = np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)
        self.path_off = np.ascontiguousarray(path_off, np.int64)
        self.letters = np.ascontiguousarray(letters, np.uint8)
        if id is None:
            id = PathLetters._next_id[0]
            PathLetters._next_id[0] += 1
        self.id = int(id)
        self._hold = self.letters if len(self.letters) else np.zeros(1, np.uint8)
        self.c = LettersIn(self.id, len(self.path_off) - 1, _p(self.path_off, C.c_int64), _p(self._hold, C.c_uint8))

    @property
    def n_paths(self):
        return len(self.path_off) - 1

    def slice(self, path, begin, end):
        o = int(self.path_off[path])
        return self.letters[o + begin:o + end]


def _ranges(ranges):
    """(n, 3) int64 (path, begin, end) -> the array and its sxg_poa_range pointer"""
    r = np.ascontiguousarray(np.asarray(ranges, np.int64).reshape(-1, 3))
    hold = r if len(r) else np.zeros((1, 3), np.int64)
    return r, hold, C.cast(hold.ctypes.data, C.POINTER(Range))


LETTERS_CODE = np.full(256, 4, np.uint8)   # the code of the identity estimate: either case of A C G T -> 0..3, anything else -> 4
for _i, _ch in enumerate("ACGT"):
    LETTERS_CODE[ord(_ch)] = LETTERS_CODE[ord(_ch.lower())] = _i


class BlockResult:
    """POA result of one block (what build_odgi_SPOA reads from spoa::Graph)."""
    __slots__ = ("status", "node_code", "node_rank", "node_group", "edge_tail", "edge_head", "edge_weight",
                 "paths", "scores", "cells", "consensus", "msa", "bg", "device_cycles")


class MafSeg(C.Structure):
    """sxg_poa_maf_seg"""
    _fields_ = [("src", C.c_int64), ("len", C.c_int32), ("kind", C.c_int32)]


class MafTextIn(C.Structure):
    """sxg_poa_maf_text_in"""
    _fields_ = [("n_segs", C.c_int64), ("segs", C.POINTER(MafSeg)), ("literal", C.POINTER(C.c_uint8)), ("literal_bytes", C.c_int64)]


MAF_SEG_DTYPE = np.dtype([("src", np.int64), ("len", np.int32), ("kind", np.int32)])   # the layout of MafSeg, for numpy


class BlockGraph:
    """Normalised block graph of one block (want_block_graph): node sequences, forward edges (from, to) sorted, one path
    of node ids per dedup'd sequence, the consensus path."""
    __slots__ = ("node_seq", "node_indeg", "edges", "paths", "consensus")

    def gfa(self, names, revs=None, consensus_name=None):
        """GFA text in the convention of sxg_block_graph_gfa (names[i]: names of the duplicates of sequence i,
        revs[i][j]: collected in reverse)."""
        o = ["H\tVN:Z:1.0"]
        o += ["S\t%d\t%s" % (i + 1, s) for i, s in enumerate(self.node_seq)]
        o += ["L\t%d\t+\t%d\t+\t0M" % (a + 1, b + 1) for a, b in self.edges]
        for i, p in enumerate(self.paths):
            for j, nm in enumerate(names[i]):
                st = ["%d-" % (v + 1) for v in p[::-1]] if revs is not None and revs[i][j] else ["%d+" % (v + 1) for v in p]
                o.append("P\t%s\t%s\t*" % (nm, ",".join(st)))
        if consensus_name is not None:
            o.append("P\t%s\t%s\t*" % (consensus_name, ",".join("%d+" % (v + 1) for v in self.consensus)))
        return "\n".join(o) + "\n"


class PoaEngine:
    """One engine = one GPU + one stream (sxg_poa_handle)."""

    def __init__(self, device=0):
        self.lib = load_library()
        if self.lib.sxg_poa_device_count() <= 0:
            raise PoaError("no HIP device: the blocked-POA engine has no CPU fallback")
        h = C.c_void_p()
        rc = self.lib.sxg_poa_create(device, C.byref(h))
        if rc:
            raise PoaError("sxg_poa_create: %s" % self.lib.sxg_poa_last_error().decode())
        self.h = h
        self._keep = None
        self._shape = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.sxg_poa_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self, what):
        return PoaError("%s: %s" % (what, self.lib.sxg_poa_last_error().decode()))

    def set_memory_budget(self, nbytes):
        self.lib.sxg_poa_set_memory_budget(self.h, int(nbytes))

    def set_long_blocks(self, on):
        """sxg_poa_set_long_blocks: with the switch on (default off) a block whose 32-bit sweep no geometry covers runs in column
        tiles instead of answering ST_TOO_LONG, up to MAX_SEQ_LEN_TILED letters; read by the next upload."""
        if self.lib.sxg_poa_set_long_blocks(self.h, int(bool(on))):
            raise self._err("sxg_poa_set_long_blocks")

    def tile_stats(self):
        """sxg_poa_get_tile_stats of the last execute: blocks of its tiled launches, their sweeps, the tiles those swept."""
        b, s, t = C.c_int64(), C.c_int64(), C.c_int64()
        if self.lib.sxg_poa_get_tile_stats(self.h, C.byref(b), C.byref(s), C.byref(t)):
            raise self._err("sxg_poa_get_tile_stats")
        return {"blocks": b.value, "sweeps": s.value, "tiles": t.value}

    # -- flat batch -----------------------------------------------------------------
    def _mk_in(self, bases, seq_off, blk_off, weights, params, want_consensus, want_msa, block_graph=0, bg_trim=None,
               bg_cons_visited_only=False):
        bases = np.ascontiguousarray(bases, np.uint8)
        seq_off = np.ascontiguousarray(seq_off, np.int64)
        blk_off = np.ascontiguousarray(blk_off, np.int32)
        nb = len(blk_off) - 1
        if isinstance(params, Params):
            parr = (Params * 1)(params)
            per = 0
        else:
            parr = (Params * max(len(params), 1))(*params)
            per = 1
        w = None if weights is None else np.ascontiguousarray(weights, np.uint32)
        bpad = bases if len(bases) else np.zeros(1, np.uint8)
        trim = None if bg_trim is None else np.ascontiguousarray(bg_trim, np.int32)
        bi = BatchIn(nb, _p(blk_off, C.c_int32), _p(seq_off, C.c_int64), _p(bpad, C.c_uint8),
                     _p(w, C.c_uint32) if w is not None else None, parr, per, int(want_consensus),
                     int(want_msa), int(block_graph), int(bool(bg_cons_visited_only)),
                     _p(trim, C.c_int32) if trim is not None else None)
        self._keep = (bpad, seq_off, blk_off, w, parr, trim)
        return bi

    def upload(self, bases, seq_off, blk_off, weights, params, want_consensus=False, want_msa=False, block_graph=0,
               bg_trim=None, bg_cons_visited_only=False):
        """want_msa: False, True / MSA_FULL, or MSA_TRIMMED (the rows of the MAF, built on the device; BlockResult.msa).
        block_graph: 1 = also the normalised block graphs (BlockResult.bg), 2 = ... without the per-base paths,
        3 = ... and without the raw POA graphs (node_* / edge_* / consensus of the results are None)."""
        bi = self._mk_in(bases, seq_off, blk_off, weights, params, want_consensus, want_msa, block_graph, bg_trim,
                         bg_cons_visited_only)
        if self.lib.sxg_poa_batch_upload(self.h, C.byref(bi)):
            raise self._err("sxg_poa_batch_upload")
        self._shape = (np.asarray(blk_off).copy(), np.asarray(seq_off).copy(), int(want_msa))

    def execute(self, check=True):
        rc = self.lib.sxg_poa_batch_execute(self.h)
        if rc and (check or rc != -4):
            raise self._err("sxg_poa_batch_execute")
        return rc

    def stats(self):
        s = Stats()
        self.lib.sxg_poa_get_stats(self.h, C.byref(s))
        st = {f[0]: getattr(s, f[0]) for f in Stats._fields_}
        # packed sweeps per strip width: "width_*" is a pair (at the geometry's width, at the class's second width)
        w = WidthStats()
        self.lib.sxg_poa_get_width_stats(self.h, C.byref(w))
        st.update(width_sweeps=tuple(w.sweeps), width_swept_cols=tuple(w.swept_cols), width_swept_cells=tuple(w.swept_cells),
                  hint_shift_repeats=w.hint_shift_repeats, dom_width=w.dom_width, dom_width2=w.dom_width2)
        tw = TwinStats()
        self.lib.sxg_poa_get_twin_stats(self.h, C.byref(tw))
        st.update(twin_steps=tw.twin_steps, join_rows=tw.join_rows)
        return st

    def compute_units(self):
        """Compute units of the engine's device (what the launch plan deals workgroups over)."""
        return int(self.lib.sxg_poa_compute_units(self.h))

    def msa_geometry(self):
        """sxg_poa_msa_geometry: (kept letters of a row per work item of the rows kernel, bytes of its on-chip window)."""
        a, b = C.c_int32(), C.c_int32()
        self.lib.sxg_poa_msa_geometry(C.byref(a), C.byref(b))
        return a.value, b.value

    def msa_stats(self):
        """sxg_poa_get_msa_stats: (columns kernel ms, rows kernel ms, bytes of rows) of the last execute with want_msa=MSA_TRIMMED."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint64()
        self.lib.sxg_poa_get_msa_stats(self.h, C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def msa_row_letters(self):
        """sxg_poa_msa_row_letters: the bytes other than '-' of every row of the resident trimmed MSA (want_msa = MSA_TRIMMED or
        MSA_TRIMMED_RESIDENT, nothing uploaded since), rows counted block after block: nseq (+ 1 with consensus) per live block."""
        blk_off = self._shape[0] if getattr(self, "_shape", None) is not None else np.zeros(1, np.int32)
        room = int(blk_off[-1]) + len(blk_off)    # (at least every sequence and one consensus row per block)
        letters = np.full(room, -1, np.int32)
        if self.lib.sxg_poa_msa_row_letters(self.h, _p(letters, C.c_int32)):
            raise self._err("sxg_poa_msa_row_letters")
        return letters[:int(np.argmax(letters < 0))] if (letters < 0).any() else letters

    def maf_text(self, segs, literal=b"", out=None):
        """sxg_poa_maf_text: the segments back to back.  segs: [(src, len, kind)] or an array of MAF_SEG_DTYPE -- kind MAF_LITERAL:
        `len` bytes of `literal` from src; MAF_ROW: row src of the resident trimmed MSA; MAF_ROW_REVCOMP: that row reversed and
        complemented.  out: a writable uint8 array of exactly the segments' bytes to fill (default: a new one, returned as bytes)."""
        sa = np.ascontiguousarray(segs, MAF_SEG_DTYPE) if isinstance(segs, np.ndarray) else np.array([tuple(x) for x in segs], MAF_SEG_DTYPE).reshape(-1)
        lit = np.frombuffer(bytes(literal), np.uint8) if not isinstance(literal, np.ndarray) else np.ascontiguousarray(literal, np.uint8)
        total = int(sa["len"].astype(np.int64).sum()) if len(sa) else 0
        buf = np.empty(total, np.uint8) if out is None else out
        ti = MafTextIn(len(sa), C.cast(sa.ctypes.data, C.POINTER(MafSeg)) if len(sa) else None, _p(lit, C.c_uint8) if len(lit) else None, len(lit))
        if self.lib.sxg_poa_maf_text(self.h, C.byref(ti), buf.ctypes.data if buf.size else None, buf.size):
            raise self._err("sxg_poa_maf_text")
        return buf.tobytes() if out is None else out

    def maf_text_geometry(self):
        """sxg_poa_maf_text_geometry: destination bytes of one work item of the text kernel."""
        c = C.c_int32()
        self.lib.sxg_poa_maf_text_geometry(C.byref(c))
        return c.value

    def maf_text_stats(self):
        """sxg_poa_maf_text_stats: (milliseconds of the text kernel, bytes it wrote), summed over the engine's calls."""
        ms, n = C.c_double(), C.c_uint64()
        self.lib.sxg_poa_maf_text_stats(self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def device_view(self):
        """Raw HBM pointers of the executed batch's results (see sxg_poa_device_view)."""
        v = DeviceView()
        if self.lib.sxg_poa_batch_device_view(self.h, C.byref(v)):
            raise self._err("sxg_poa_batch_device_view")
        return v

    def download(self):
        out = BatchOut()
        if self.lib.sxg_poa_batch_download(self.h, C.byref(out)):
            raise self._err("sxg_poa_batch_download")
        try:
            return self._unpack(out)
        finally:
            self.lib.sxg_poa_batch_free(C.byref(out))

    def _unpack(self, out, shape=None):
        # shape: offsets and want_msa of the batch these results belong to (default: the batch upload() made resident)
        shape = shape if shape is not None else self._shape
        blk_off, seq_off = shape[:2]
        msa_mode = shape[2] if len(shape) > 2 else 0
        nb = out.n_blocks
        ns = int(out.n_seqs)
        status = _arr(out.status, nb, np.int32)
        node_off = _arr(out.node_off, nb + 1, np.int64)
        edge_off = _arr(out.edge_off, nb + 1, np.int64)
        nn, ne = (int(node_off[-1]), int(edge_off[-1])) if nb else (0, 0)
        has_raw = bool(out.node_code) or nn == 0      # (block_graph=3: the raw POA graphs are left out)
        node_code = _arr(out.node_code, nn, np.uint8) if has_raw else None
        node_rank = _arr(out.node_rank, nn, np.int32) if has_raw else None
        node_group = _arr(out.node_group, nn, np.int32) if has_raw else None
        et = _arr(out.edge_tail, ne, np.int32) if has_raw else None
        eh = _arr(out.edge_head, ne, np.int32) if has_raw else None
        ew = _arr(out.edge_weight, ne, np.uint32) if has_raw else None
        nbases = int(seq_off[-1]) if ns else 0
        paths = _arr(out.seq_path_nodes, nbases, np.int32) if out.seq_path_nodes else None
        bg = None
        if out.bg_node_off:
            bno = _arr(out.bg_node_off, nb + 1, np.int64)
            bso = _arr(out.bg_seq_off, nb + 1, np.int64)
            beo = _arr(out.bg_edge_off, nb + 1, np.int64)
            bpo = _arr(out.bg_step_off, ns + 1, np.int64)
            bg = dict(no=bno, so=bso, eo=beo, po=bpo, ln=_arr(out.bg_node_len, int(bno[-1]), np.int32),
                      od=_arr(out.bg_node_outdeg, int(bno[-1]), np.int32), idg=_arr(out.bg_node_indeg, int(bno[-1]), np.uint8),
                      sq=C.string_at(out.bg_seq, int(bso[-1])) if bso[-1] else b"", to=_arr(out.bg_edge_to, int(beo[-1]), np.int32),
                      st=_arr(out.bg_steps, int(bpo[-1]), np.int32))
            if out.bg_cons_off:
                bg["co"] = _arr(out.bg_cons_off, nb + 1, np.int64)
                bg["cs"] = _arr(out.bg_cons_steps, int(bg["co"][-1]), np.int32)
        score = _arr(out.score, ns, np.int32)
        cells = _arr(out.cells, ns, np.uint64)
        cycles = _arr(out.block_cycles, nb, np.uint64) if out.block_cycles else None
        cons_off = _arr(out.cons_off, nb + 1, np.int64) if out.cons_off else None
        cons = _arr(out.cons_nodes, int(cons_off[-1]), np.int32) if cons_off is not None and nb and out.cons_nodes else None
        msa_off = _arr(out.msa_off, nb + 1, np.int64) if out.msa_off else None
        msa_cols = _arr(out.msa_cols, nb, np.int32) if out.msa_cols else None
        msa_raw = None
        # (offsets and widths of the last result with a trimmed MSA: all there is of it when the rows stay resident)
        self.msa_layout = (msa_off.copy(), msa_cols.copy()) if msa_off is not None and msa_cols is not None else None
        if msa_off is not None and nb and msa_off[-1] > 0 and out.msa:
            msa_raw = C.string_at(out.msa, int(msa_off[-1]))
        res = []
        for b in range(nb):
            r = BlockResult()
            r.status = int(status[b])
            a, z = node_off[b], node_off[b + 1]
            r.node_code, r.node_rank, r.node_group = (node_code[a:z], node_rank[a:z], node_group[a:z]) if has_raw else (None, None, None)
            a, z = edge_off[b], edge_off[b + 1]
            r.edge_tail, r.edge_head, r.edge_weight = (et[a:z], eh[a:z], ew[a:z]) if has_raw else (None, None, None)
            s0, s1 = int(blk_off[b]), int(blk_off[b + 1])
            r.paths = [paths[int(seq_off[s]):int(seq_off[s + 1])] for s in range(s0, s1)] if paths is not None else None
            r.bg = None
            if bg is not None:
                g = BlockGraph()
                a, z = int(bg["no"][b]), int(bg["no"][b + 1])
                ln, od = bg["ln"][a:z], bg["od"][a:z]
                g.node_indeg = bg["idg"][a:z]
                so = int(bg["so"][b]) + np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
                g.node_seq = [bg["sq"][int(so[i]):int(so[i + 1])].decode() for i in range(z - a)]
                to = bg["to"][int(bg["eo"][b]):int(bg["eo"][b + 1])]
                g.edges = list(zip(np.repeat(np.arange(z - a), od).tolist(), to.tolist()))
                g.paths = [bg["st"][int(bg["po"][s]):int(bg["po"][s + 1])] for s in range(s0, s1)]
                g.consensus = bg["cs"][int(bg["co"][b]):int(bg["co"][b + 1])] if "co" in bg else None
                r.bg = g
            r.scores, r.cells = score[s0:s1], cells[s0:s1]
            r.device_cycles = int(cycles[b]) if cycles is not None else None   # (sxg_poa_batch_out::block_cycles)
            r.consensus = cons[cons_off[b]:cons_off[b + 1]] if cons is not None else None
            r.msa = None
            if msa_mode == MSA_TRIMMED and msa_cols is not None and r.status == 0 and s1 > s0 and int(msa_cols[b]) == 0:
                r.msa = [""] * ((s1 - s0) + (1 if cons_off is not None else 0))   # (nothing remains after the trim: rows x "")
            elif msa_raw is not None and r.status == 0:
                ncol = int(msa_cols[b])
                raw = msa_raw[int(msa_off[b]):int(msa_off[b + 1])]
                r.msa = [raw[i * ncol:(i + 1) * ncol].decode() for i in range(len(raw) // ncol)] if ncol else []
            res.append(r)
        return res

    def run_flat(self, bases, seq_off, blk_off, weights, params, want_consensus=False, want_msa=False,
                 check=True, block_graph=0, bg_trim=None, bg_cons_visited_only=False):
        self.upload(bases, seq_off, blk_off, weights, params, want_consensus, want_msa, block_graph, bg_trim,
                    bg_cons_visited_only)
        self.execute(check=check)
        return self.download()

    # -- multi-GPU (one engine per rank) ---------------------------------------------------
    def comm_unique_id(self):
        """Rank 0: the id every rank passes to comm_init (send it through any side channel)."""
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        if self.lib.sxg_poa_comm_unique_id(buf):
            raise self._err("sxg_poa_comm_unique_id")
        return bytes(buf)

    def comm_init(self, comm_id, nranks, rank):
        buf = (C.c_uint8 * COMM_ID_BYTES)(*comm_id)
        if self.lib.sxg_poa_comm_init(self.h, buf, nranks, rank):
            raise self._err("sxg_poa_comm_init")

    def run_flat_sharded(self, bases, seq_off, blk_off, weights, params, want_consensus=False, want_msa=False, check=True,
                         simulate_ranks=0, block_graph=0, bg_trim=None, bg_cons_visited_only=False):
        """sxg_poa_batch_run_sharded: every rank passes the SAME batch; rank 0 gets all results (list), the others None.
        simulate_ranks > 0: the test entry that plays that many ranks on this one GPU."""
        bi = self._mk_in(bases, seq_off, blk_off, weights, params, want_consensus, want_msa, block_graph, bg_trim, bg_cons_visited_only)
        shape = (np.asarray(blk_off).copy(), np.asarray(seq_off).copy(), int(want_msa))   # (of THIS call: a refused call leaves the resident batch and its shape alone)
        out = BatchOut()
        if simulate_ranks:
            rc = self.lib.sxg_poa_batch_run_sharded_local(self.h, C.byref(bi), simulate_ranks, C.byref(out))
        else:
            rc = self.lib.sxg_poa_batch_run_sharded(self.h, C.byref(bi), C.byref(out))
        if rc == NOT_ROOT:
            return None
        try:
            if rc and (check or rc != -4):
                raise self._err("sxg_poa_batch_run_sharded")
            return self._unpack(out, shape)
        finally:
            self.lib.sxg_poa_batch_free(C.byref(out))

    # -- the sharded run in stages (inputs stay resident between executes) ------------------
    def upload_sharded(self, bases, seq_off, blk_off, weights, params, want_consensus=False, want_msa=False):
        """Every rank, SAME batch: deal the blocks by cost over the communicator's ranks, upload this rank's share."""
        sh_in = self._mk_in(bases, seq_off, blk_off, weights, params, want_consensus, want_msa)
        if self.lib.sxg_poa_batch_upload_sharded(self.h, C.byref(sh_in)):
            raise self._err("sxg_poa_batch_upload_sharded")
        self._sh_in = sh_in
        self._sh_shape = (np.asarray(blk_off).copy(), np.asarray(seq_off).copy(), int(want_msa))

    def execute_sharded(self):
        """Collective: align the uploaded share, pack it, bring every rank's blob to rank 0 (RCCL)."""
        if self.lib.sxg_poa_batch_execute_sharded(self.h):
            raise self._err("sxg_poa_batch_execute_sharded")

    def download_sharded(self, check=True):
        """Rank 0: all results in the batch's block order; other ranks: None."""
        out = BatchOut()
        rc = self.lib.sxg_poa_batch_download_sharded(self.h, C.byref(self._sh_in), C.byref(out))
        if rc == NOT_ROOT:
            return None
        try:
            if rc and (check or rc != -4):
                raise self._err("sxg_poa_batch_download_sharded")
            return self._unpack(out, self._sh_shape)
        finally:
            self.lib.sxg_poa_batch_free(C.byref(out))

    def measure_copy(self, nbytes=1 << 30, reps=5):
        """GB/s (read + written) of a streaming device-to-device copy on this engine's device (sxg_poa_measure_copy)."""
        g = C.c_double()
        if self.lib.sxg_poa_measure_copy(self.h, C.c_uint64(int(nbytes)), int(reps), C.byref(g)):
            raise self._err("sxg_poa_measure_copy")
        return g.value

    def roctx_available(self):
        return int(self.lib.sxg_poa_roctx_available())

    def sharded_info(self):
        n, b = C.c_int32(), C.c_uint64()
        self.lib.sxg_poa_sharded_info(self.h, C.byref(n), C.byref(b))
        pk, ex = C.c_double(), C.c_double()
        self.lib.sxg_poa_sharded_timing(self.h, C.byref(pk), C.byref(ex))
        return {"ranks_seen": n.value, "bytes_received": b.value, "pack_ms": pk.value, "exchange_ms": ex.value}

    def run_blocks(self, blocks, params, weights=None, want_consensus=False, want_msa=False, check=True):
        """blocks: list of lists of uint8 code arrays (one inner list per block, alignment order)."""
        seqs = [s for blk in blocks for s in blk]
        bases = np.concatenate([np.asarray(s, np.uint8) for s in seqs]) if seqs else np.zeros(0, np.uint8)
        seq_off = np.zeros(len(seqs) + 1, np.int64)
        if seqs:
            seq_off[1:] = np.cumsum([len(s) for s in seqs])
        blk_off = np.zeros(len(blocks) + 1, np.int32)
        if blocks:
            blk_off[1:] = np.cumsum([len(b) for b in blocks])
        w = None if weights is None else np.concatenate([np.asarray(x, np.uint32) for x in weights])
        return self.run_flat(bases, seq_off, blk_off, w, params, want_consensus, want_msa, check)

    # -- the identity split of break_blocks (src/breaks.cpp:335-586) -------------------------
    @staticmethod
    def _flat(seqs):
        seqs = [np.ascontiguousarray(x, np.uint8) for x in seqs]
        seq_off = np.zeros(len(seqs) + 1, np.int64)
        if seqs:
            seq_off[1:] = np.cumsum([len(x) for x in seqs])
        bases = np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)
        return (bases if len(bases) else np.zeros(1, np.uint8)), seq_off

    def pair_identity(self, seqs, pairs, caps, rev=None):
        """sxg_poa_pair_identity_batch.  seqs: code arrays; pairs: (a, b) indices into seqs; caps: one bound per pair;
        rev: per pair, b is read reverse-complemented.  Returns int32 arrays (penalty, cols, matches); cols == 0 means
        the optimal penalty is not below the cap."""
        bases, seq_off = self._flat(seqs)
        n = len(pairs)
        pa = np.ascontiguousarray([p[0] for p in pairs], np.int32) if n else np.zeros(1, np.int32)
        pb = np.ascontiguousarray([p[1] for p in pairs], np.int32) if n else np.zeros(1, np.int32)
        cap = np.ascontiguousarray(caps, np.int32) if n else np.zeros(1, np.int32)
        rv = None if rev is None else (np.ascontiguousarray(rev, np.uint8) if n else np.zeros(1, np.uint8))
        pen, cols, mat = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        rc = self.lib.sxg_poa_pair_identity_batch(self.h, len(seqs), _p(seq_off, C.c_int64), _p(bases, C.c_uint8), n, _p(pa, C.c_int32),
                                                  _p(pb, C.c_int32), _p(rv, C.c_uint8) if rv is not None else None, _p(cap, C.c_int32),
                                                  _p(pen, C.c_int32), _p(cols, C.c_int32), _p(mat, C.c_int32))
        if rc:
            raise self._err("sxg_poa_pair_identity_batch")
        return pen[:n], cols[:n], mat[:n]

    def split(self, blocks, identity, length_ratio_min=0.0, check=True):
        """sxg_poa_split_batch.  blocks: list of lists of code arrays, each block dedup'd and sorted by (length, letters);
        identity / length_ratio_min: one value or one per block.  Returns one (groups, n_groups, n_pairs, status) per
        block, groups being the int32 group id of every sequence."""
        nb = len(blocks)
        bases, seq_off = self._flat([x for blk in blocks for x in blk])
        blk_off = np.zeros(nb + 1, np.int32)
        if nb:
            blk_off[1:] = np.cumsum([len(b) for b in blocks])
        ident = np.ascontiguousarray(np.broadcast_to(np.asarray(identity, np.float64), (nb,)) if nb else np.zeros(1), np.float64)
        ratio = np.ascontiguousarray(np.broadcast_to(np.asarray(length_ratio_min, np.float64), (nb,)) if nb else np.zeros(1), np.float64)
        si = SplitIn(nb, _p(blk_off, C.c_int32), _p(seq_off, C.c_int64), _p(bases, C.c_uint8), _p(ident, C.c_double), _p(ratio, C.c_double))
        out = SplitOut()
        rc = self.lib.sxg_poa_split_batch(self.h, C.byref(si), C.byref(out))
        try:
            if rc and (check or rc != -4):
                raise self._err("sxg_poa_split_batch")
            grp = _arr(out.group, int(blk_off[-1]), np.int32)
            ng, npairs, st = _arr(out.n_groups, nb, np.int32), _arr(out.n_pairs, nb, np.int64), _arr(out.status, nb, np.int32)
            return [(grp[blk_off[b]:blk_off[b + 1]], int(ng[b]), int(npairs[b]), int(st[b])) for b in range(nb)]
        finally:
            self.lib.sxg_poa_split_free(C.byref(out))

    def kmer_jaccard(self, seqs, pairs, k, want_sets=False):
        """sxg_poa_kmer_jaccard_batch.  seqs: code arrays; pairs: (a, b) indices into seqs.  Returns (set_size, inter): the
        number of distinct canonical k-mers of every sequence and the size of the intersection of every pair (int32
        arrays); with want_sets also the sorted uint64 set of every sequence, as a list."""
        bases, seq_off = self._flat(seqs)
        ns, n = len(seqs), len(pairs)
        pa = np.ascontiguousarray([p[0] for p in pairs], np.int32) if n else np.zeros(1, np.int32)
        pb = np.ascontiguousarray([p[1] for p in pairs], np.int32) if n else np.zeros(1, np.int32)
        size, inter = np.zeros(max(ns, 1), np.int32), np.zeros(max(n, 1), np.int32)
        kmers = np.zeros(max(int(seq_off[-1]), 1), np.uint64) if want_sets else None
        rc = self.lib.sxg_poa_kmer_jaccard_batch(self.h, ns, _p(seq_off, C.c_int64), _p(bases, C.c_uint8), int(k), n, _p(pa, C.c_int32),
                                                 _p(pb, C.c_int32), _p(size, C.c_int32), _p(inter, C.c_int32),
                                                 _p(kmers, C.c_uint64) if want_sets else None)
        if rc:
            raise self._err("sxg_poa_kmer_jaccard_batch")
        if want_sets:
            return size[:ns], inter[:n], [kmers[seq_off[s]:seq_off[s] + size[s]].copy() for s in range(ns)]
        return size[:ns], inter[:n]

    def split_mash(self, blocks, identity, length_ratio_min, kmer_size, min_len, est_identity=None, check=True):
        """sxg_poa_split_mash_batch: split() with the mash-based branch.  min_len: one value or one per block, 0 = that block
        runs the edit-based walk only; est_identity: one value or one per block, None = identity.  Returns one (groups,
        n_groups, n_pairs, n_mash, status) per block."""
        nb = len(blocks)
        bases, seq_off = self._flat([x for blk in blocks for x in blk])
        blk_off = np.zeros(nb + 1, np.int32)
        if nb:
            blk_off[1:] = np.cumsum([len(b) for b in blocks])
        per_block = lambda v, dt: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dt), (nb,)) if nb else np.zeros(1), dt)
        ident, ratio = per_block(identity, np.float64), per_block(length_ratio_min, np.float64)
        est = ident.copy() if est_identity is None else per_block(est_identity, np.float64)
        ml = per_block(min_len, np.int32)
        si = SplitIn(nb, _p(blk_off, C.c_int32), _p(seq_off, C.c_int64), _p(bases, C.c_uint8), _p(ident, C.c_double), _p(ratio, C.c_double))
        sm = SplitMash(int(kmer_size), _p(ml, C.c_int32), _p(est, C.c_double))
        nm = np.zeros(max(nb, 1), np.int64)
        out = SplitOut()
        rc = self.lib.sxg_poa_split_mash_batch(self.h, C.byref(si), C.byref(sm), C.byref(out), _p(nm, C.c_int64))
        try:
            if rc and (check or rc != -4):
                raise self._err("sxg_poa_split_mash_batch")
            grp = _arr(out.group, int(blk_off[-1]), np.int32)
            ng, npairs, st = _arr(out.n_groups, nb, np.int32), _arr(out.n_pairs, nb, np.int64), _arr(out.status, nb, np.int32)
            return [(grp[blk_off[b]:blk_off[b + 1]], int(ng[b]), int(npairs[b]), int(nm[b]), int(st[b])) for b in range(nb)]
        finally:
            self.lib.sxg_poa_split_free(C.byref(out))

    def block_identity(self, blocks, kmer_size=17, min_len=None, percentile=0.30, check=True):
        """sxg_poa_block_identity_batch (decree Q): the identity estimate of the adaptive scores.  blocks: list of lists of code
        arrays (a block's path-range sequences, not dedup'd); min_len: None = 8 * kmer_size.  Returns int32 arrays (n_used,
        inter, uni, status), one entry per block: the sizes of the intersection and the union of the k-mer sets of the pair
        at the percentile's rank among the block's pairs ordered by Jaccard index."""
        nb = len(blocks)
        bases, seq_off = self._flat([x for blk in blocks for x in blk])
        blk_off = np.zeros(nb + 1, np.int32)
        if nb:
            blk_off[1:] = np.cumsum([len(b) for b in blocks])
        ii = IdentityIn(nb, _p(blk_off, C.c_int32), _p(seq_off, C.c_int64), _p(bases, C.c_uint8), int(kmer_size),
                        8 * int(kmer_size) if min_len is None else int(min_len), float(percentile))
        used, inter, uni, st = (np.zeros(max(nb, 1), np.int32) for _ in range(4))
        rc = self.lib.sxg_poa_block_identity_batch(self.h, C.byref(ii), _p(used, C.c_int32), _p(inter, C.c_int32), _p(uni, C.c_int32),
                                                   _p(st, C.c_int32))
        if rc and (check or rc != -4):
            raise self._err("sxg_poa_block_identity_batch")
        return used[:nb], inter[:nb], uni[:nb], st[:nb]

    # -- the tandem-repeat scan of break_blocks (src/breaks.cpp:224-272) ----------------------
    def repeat_scan(self, seqs, min_copy=1000, max_copy=20000, stride=50, want_match=False, check=True):
        """sxg_poa_repeat_scan_batch (decree R).  seqs: byte strings or uint8 arrays, the letters as they are.  Returns (n_lags,
        best, dev, v, status) -- int32, int32, float64, float64, int32, one entry per sequence -- and with want_match a sixth
        entry, the list of every sequence's int32 match counts (lag min_copy + k at index k).  A repeat of length min_copy +
        best is reported iff sqrt(v) != 0 and dev / sqrt(v) >= min_z (the host's part of the decree)."""
        ns = len(seqs)
        bases, seq_off = self._flat([np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else x for x in seqs])
        ri = RepeatIn(ns, _p(seq_off, C.c_int64), _p(bases, C.c_uint8), int(min_copy), int(max_copy), int(stride))
        lags, best, st = (np.zeros(max(ns, 1), np.int32) for _ in range(3))
        dev, v = (np.zeros(max(ns, 1), np.float64) for _ in range(2))
        match = None
        if want_match:   # the layout of sxg_repeat_match_offsets (poa_repeat.h): a declined sequence has no counts
            n = np.diff(seq_off)
            want = np.where((n >= 2 * int(min_copy)) & (n <= REPEAT_MAX_LEN) & (int(min_copy) > 0) & (int(max_copy) >= int(min_copy)),
                            np.minimum(int(max_copy), n - int(min_copy)) - int(min_copy) + 1, 0)
            off = np.concatenate([[0], np.cumsum(want)]).astype(np.int64)
            match = np.zeros(max(int(off[-1]), 1), np.int32)
        rc = self.lib.sxg_poa_repeat_scan_batch(self.h, C.byref(ri), _p(lags, C.c_int32), _p(best, C.c_int32), _p(dev, C.c_double), _p(v, C.c_double),
                                                _p(st, C.c_int32), _p(match, C.c_int32) if want_match else None)
        if rc and (check or rc != -4):
            raise self._err("sxg_poa_repeat_scan_batch")
        res = (lags[:ns], best[:ns], dev[:ns], v[:ns], st[:ns])
        return res + ([match[off[s]:off[s + 1]] for s in range(ns)],) if want_match else res

    # -- resident path letters: the two calls above on ranges of them ---------------------------
    def upload_letters(self, letters):
        """sxg_poa_letters_upload: `letters` (a PathLetters) replace what is resident on this handle."""
        if self.lib.sxg_poa_letters_upload(self.h, C.byref(letters.c)):
            raise self._err("sxg_poa_letters_upload")

    def drop_letters(self):
        self.lib.sxg_poa_letters_drop(self.h)

    def letters_resident(self):
        """(id, n_paths, n_letters) of the resident letters; id 0 = none."""
        i, p, n = C.c_uint64(), C.c_int64(), C.c_int64()
        if self.lib.sxg_poa_letters_resident(self.h, C.byref(i), C.byref(p), C.byref(n)):
            raise self._err("sxg_poa_letters_resident")
        return int(i.value), int(p.value), int(n.value)

    def letters_stats(self):
        """Since the handle was created: uploads, their bytes, the gather kernels' time and the bytes they wrote."""
        u, b, g = C.c_uint64(), C.c_uint64(), C.c_uint64()
        ms = C.c_double()
        if self.lib.sxg_poa_letters_stats(self.h, C.byref(u), C.byref(b), C.byref(ms), C.byref(g)):
            raise self._err("sxg_poa_letters_stats")
        return {"uploads": int(u.value), "bytes_uploaded": int(b.value), "gather_ms": float(ms.value), "gathered_bytes": int(g.value)}

    def letters_geometry(self):
        c = C.c_int32()
        self.lib.sxg_poa_letters_geometry(C.byref(c))
        return int(c.value)

    @staticmethod
    def _letters_arg(letters, letters_id):
        """letters: a PathLetters (passed to the call, which uploads them if they are not resident) or None with letters_id"""
        if letters is None:
            return None, int(letters_id)
        return C.pointer(letters.c), int(letters.id if letters_id is None else letters_id)

    def gather_ranges(self, letters, ranges, coded=False, letters_id=None):
        """sxg_poa_range_gather: what the gather kernel writes for `ranges` ((n, 3) int64: path, begin, end), one uint8 array."""
        r, hold, rp = _ranges(ranges)
        lp, lid = self._letters_arg(letters, letters_id)
        total = int((r[:, 2] - r[:, 1]).sum()) if len(r) else 0
        out = np.zeros(max(total, 1), np.uint8)
        if self.lib.sxg_poa_range_gather(self.h, lp, lid, len(r), rp, 1 if coded else 0, _p(out, C.c_uint8)):
            raise self._err("sxg_poa_range_gather")
        return out[:total]

    def repeat_scan_ranges(self, letters, ranges, min_copy=1000, max_copy=20000, stride=50, want_match=False, check=True, letters_id=None):
        """sxg_poa_repeat_scan_ranges: repeat_scan on the sequences `ranges` spell in `letters`; the same results."""
        r, hold, rp = _ranges(ranges)
        ns = len(r)
        lp, lid = self._letters_arg(letters, letters_id)
        ri = RepeatRangesIn(lp, lid, ns, rp, int(min_copy), int(max_copy), int(stride))
        lags, best, st = (np.zeros(max(ns, 1), np.int32) for _ in range(3))
        dev, v = (np.zeros(max(ns, 1), np.float64) for _ in range(2))
        match = None
        if want_match:
            n = (r[:, 2] - r[:, 1]) if ns else np.zeros(0, np.int64)
            want = np.where((n >= 2 * int(min_copy)) & (n <= REPEAT_MAX_LEN) & (int(min_copy) > 0) & (int(max_copy) >= int(min_copy)),
                            np.minimum(int(max_copy), n - int(min_copy)) - int(min_copy) + 1, 0)
            off = np.concatenate([[0], np.cumsum(want)]).astype(np.int64)
            match = np.zeros(max(int(off[-1]), 1), np.int32)
        rc = self.lib.sxg_poa_repeat_scan_ranges(self.h, C.byref(ri), _p(lags, C.c_int32), _p(best, C.c_int32), _p(dev, C.c_double), _p(v, C.c_double),
                                                 _p(st, C.c_int32), _p(match, C.c_int32) if want_match else None)
        if rc and (check or rc != -4):
            raise self._err("sxg_poa_repeat_scan_ranges")
        res = (lags[:ns], best[:ns], dev[:ns], v[:ns], st[:ns])
        return res + ([match[off[s]:off[s + 1]] for s in range(ns)],) if want_match else res

    def block_identity_ranges(self, letters, blocks, kmer_size=17, min_len=None, percentile=0.30, check=True, letters_id=None):
        """sxg_poa_block_identity_ranges: block_identity on the sequences the blocks' ranges spell in `letters`, coded on the device.
        blocks: list of lists of (path, begin, end)."""
        nb = len(blocks)
        r, hold, rp = _ranges([x for blk in blocks for x in blk])
        blk_off = np.zeros(nb + 1, np.int32)
        if nb:
            blk_off[1:] = np.cumsum([len(b) for b in blocks])
        lp, lid = self._letters_arg(letters, letters_id)
        ii = IdentityRangesIn(lp, lid, nb, _p(blk_off, C.c_int32), rp, int(kmer_size), 8 * int(kmer_size) if min_len is None else int(min_len),
                              float(percentile))
        used, inter, uni, st = (np.zeros(max(nb, 1), np.int32) for _ in range(4))
        rc = self.lib.sxg_poa_block_identity_ranges(self.h, C.byref(ii), _p(used, C.c_int32), _p(inter, C.c_int32), _p(uni, C.c_int32),
                                                    _p(st, C.c_int32))
        if rc and (check or rc != -4):
            raise self._err("sxg_poa_block_identity_ranges")
        return used[:nb], inter[:nb], uni[:nb], st[:nb]

    # -- the node order of prep (src/prep.cpp:11-163) ----------------------------------------
    def path_sgd_order(self, node_len, path_off, step_node, step_pos, eta, cooling_start, terms_per_iter, seed, mode=0, want_x=True):
        """sxg_poa_path_sgd_order (decree Y).  node_len: bases of every node in rank order; path_off / step_node / step_pos:
        the paths as flat steps (node rank, bp offset in the path); eta: the learning rate of every iteration (None reaches
        the library as NULL); mode: 0 = choose, 1 = LDS path, 2 = global path.  Returns (order, x): the old ranks in the new
        order (int32) and the final coordinates by old rank (int64, units of 2^-20 bp; None unless want_x)."""
        def arr(a, t):   # (an empty array has no address worth passing)
            a = np.ascontiguousarray(a, t)
            return a if len(a) else np.zeros(1, t)
        n, n_paths = len(node_len), len(path_off) - 1
        node_len, path_off, step_node, step_pos = arr(node_len, np.int32), arr(path_off, np.int64), arr(step_node, np.int32), arr(step_pos, np.int64)
        si = SgdIn(n, _p(node_len, C.c_int32), n_paths, _p(path_off, C.c_int64), _p(step_node, C.c_int32), _p(step_pos, C.c_int64),
                   1, int(cooling_start), None, int(terms_per_iter), int(seed), int(mode))
        if eta is not None:
            si.iter_max = len(eta)
            eta = arr(eta, np.float64)
            si.eta = _p(eta, C.c_double)
        order, x = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int64)
        if self.lib.sxg_poa_path_sgd_order(self.h, C.byref(si), _p(order, C.c_int32), _p(x, C.c_int64) if want_x else None):
            raise self._err("sxg_poa_path_sgd_order")
        return order[:n], (x[:n] if want_x else None)

    # -- stand-alone Align(sequence, graph) --------------------------------------------
    def align(self, problems, params, check=True):
        """problems: list of (codes, off, pred, sink, seq) with the CSR of oracle `rows()`.
        Returns list of (pair_row, pair_pos, score, status)."""
        n = len(problems)
        row_off = np.zeros(n + 1, np.int64)
        seq_off = np.zeros(n + 1, np.int64)
        codes, sinks, preds, poffs, bases = [], [], [], [np.zeros(1, np.int64)], []
        eo = 0
        for k, (cd, off, pr, sk, sq) in enumerate(problems):
            row_off[k + 1] = row_off[k] + len(cd)
            seq_off[k + 1] = seq_off[k] + len(sq)
            codes.append(np.asarray(cd, np.uint8))
            sinks.append(np.asarray(sk, np.uint8))
            preds.append(np.asarray(pr, np.int32))
            bases.append(np.asarray(sq, np.uint8))
            poffs.append(np.asarray(off[1:], np.int64) + eo)
            eo += int(off[-1]) if len(off) else 0

        def cat(xs, dt):
            return np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0, dt), dt)

        def pad(a):
            return a if len(a) else np.zeros(1, a.dtype)

        codes, sinks, preds, bases = cat(codes, np.uint8), cat(sinks, np.uint8), cat(preds, np.int32), cat(bases, np.uint8)
        poff = cat(poffs, np.int64)
        if isinstance(params, Params):
            parr, per = (Params * 1)(params), 0
        else:
            parr, per = (Params * max(len(params), 1))(*params), 1
        codes, sinks, preds, bases = pad(codes), pad(sinks), pad(preds), pad(bases)
        ai = AlignIn(n, _p(row_off, C.c_int64), _p(codes, C.c_uint8), _p(sinks, C.c_uint8),
                     _p(poff, C.c_int64), _p(preds, C.c_int32), _p(seq_off, C.c_int64),
                     _p(bases, C.c_uint8), parr, per)
        out = AlignOut()
        rc = self.lib.sxg_poa_align_batch(self.h, C.byref(ai), C.byref(out))
        try:
            if rc and (check or rc != -4):
                raise self._err("sxg_poa_align_batch")
            status = _arr(out.status, n, np.int32)
            score = _arr(out.score, n, np.int32)
            po = _arr(out.pair_off, n + 1, np.int64)
            tot = int(po[-1]) if n else 0
            pr_ = _arr(out.pair_row, tot, np.int32)
            pp_ = _arr(out.pair_pos, tot, np.int32)
            return [(pr_[po[k]:po[k + 1]], pp_[po[k]:po[k + 1]], int(score[k]), int(status[k]))
                    for k in range(n)]
        finally:
            self.lib.sxg_poa_align_free(C.byref(out))


class _MemberEngine(PoaEngine):
    """Member i of a PoaGroup as an engine: the handle is the group's, so close() leaves it alone."""

    def __init__(self, lib, h):
        self.lib, self.h, self._keep, self._shape = lib, h, None, None

    def close(self):
        self.h = None


class PoaGroup:
    """One process, several GPUs (sxg_poa_group): one engine handle per entry of `devices` -- the same device may appear more
    than once --, a batch dealt over them in contiguous slices of equal cost, one host thread per member, the results
    reassembled in the batch's block order.  Mirrors PoaEngine: run_flat / run_blocks / upload / execute / download return
    what a single engine returns for the same input."""

    def __init__(self, devices):
        self.lib = load_library()
        if self.lib.sxg_poa_device_count() <= 0:
            raise PoaError("no HIP device: the blocked-POA engine has no CPU fallback")
        devices = [int(d) for d in devices]
        arr = (C.c_int32 * max(len(devices), 1))(*devices)
        h = C.c_void_p()
        if self.lib.sxg_poa_group_create(arr, len(devices), C.byref(h)):
            raise PoaError("sxg_poa_group_create: %s" % self.lib.sxg_poa_last_error().decode())
        self.h = h
        self.devices = devices
        self._keep = None
        self._shape = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.sxg_poa_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self.lib.sxg_poa_group_size(self.h))

    _err = PoaEngine._err
    _mk_in = PoaEngine._mk_in
    _unpack = PoaEngine._unpack
    run_blocks = PoaEngine.run_blocks

    def set_memory_budget(self, nbytes_per_member):
        self.lib.sxg_poa_group_set_memory_budget(self.h, int(nbytes_per_member))

    def set_long_blocks(self, on):
        """PoaEngine.set_long_blocks on every member."""
        if self.lib.sxg_poa_group_set_long_blocks(self.h, int(bool(on))):
            raise self._err("sxg_poa_group_set_long_blocks")

    def tile_stats(self):
        """PoaEngine.tile_stats, summed over the members."""
        tot = {"blocks": 0, "sweeps": 0, "tiles": 0}
        for i in range(len(self)):
            for k, v in self.member(i).tile_stats().items():
                tot[k] += v
        return tot

    def member(self, i):
        """Member i as a PoaEngine (owned by the group): its stats, and the split, identity and SGD calls, which stay
        single-device."""
        h = self.lib.sxg_poa_group_member(self.h, int(i))
        if not h:
            raise IndexError("no such group member: %r" % (i,))
        return _MemberEngine(self.lib, C.c_void_p(h))

    def stats(self, i):
        return self.member(i).stats()

    def timing(self):
        """sxg_poa_group_timing of the last execute + download: milliseconds per member, of the longest member download and
        of the reassembly on the host."""
        n = len(self)
        ms = (C.c_double * n)()
        pk, asm = C.c_double(), C.c_double()
        self.lib.sxg_poa_group_timing(self.h, ms, C.byref(pk), C.byref(asm))
        return {"member_ms": list(ms), "pack_ms": pk.value, "assemble_ms": asm.value}

    def upload(self, bases, seq_off, blk_off, weights, params, want_consensus=False, want_msa=False, block_graph=0,
               bg_trim=None, bg_cons_visited_only=False):
        bi = self._mk_in(bases, seq_off, blk_off, weights, params, want_consensus, want_msa, block_graph, bg_trim,
                         bg_cons_visited_only)
        if self.lib.sxg_poa_group_batch_upload(self.h, C.byref(bi)):
            raise self._err("sxg_poa_group_batch_upload")
        self._shape = (np.asarray(blk_off).copy(), np.asarray(seq_off).copy(), int(want_msa))

    def execute(self, check=True):
        rc = self.lib.sxg_poa_group_batch_execute(self.h)
        if rc and (check or rc != -4):
            raise self._err("sxg_poa_group_batch_execute")
        return rc

    def download(self):
        out = BatchOut()
        if self.lib.sxg_poa_group_batch_download(self.h, C.byref(out)):
            raise self._err("sxg_poa_group_batch_download")
        try:
            return self._unpack(out)
        finally:
            self.lib.sxg_poa_batch_free(C.byref(out))

    def run_flat(self, bases, seq_off, blk_off, weights, params, want_consensus=False, want_msa=False,
                 check=True, block_graph=0, bg_trim=None, bg_cons_visited_only=False):
        bi = self._mk_in(bases, seq_off, blk_off, weights, params, want_consensus, want_msa, block_graph, bg_trim,
                         bg_cons_visited_only)
        self._shape = (np.asarray(blk_off).copy(), np.asarray(seq_off).copy(), int(want_msa))
        out = BatchOut()
        rc = self.lib.sxg_poa_group_batch_run(self.h, C.byref(bi), C.byref(out))
        self.last_rc = rc      # (0, or -4 = SXG_E_BLOCK with check=False: some block failed, see the results' status)
        try:
            if rc and (check or rc != -4):
                raise self._err("sxg_poa_group_batch_run")
            return self._unpack(out)
        finally:
            self.lib.sxg_poa_batch_free(C.byref(out))


def xxh64(data: bytes, seed=0):
    return load_library().sxg_xxh64(data, len(data), seed)

"""ctypes binding of the C ABI in ``include/gpusim_hip.h`` (libgsim_hip.so).

This is the only way Python reaches the GPU in this package: there is no
PyTorch/numpy fallback.  If the library is missing or no GPU is usable the calls
fail loudly (``GsimError``).
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSIM_LIB: alternative build of the same ABI (kernel ablation experiments only)
LIB_PATH = os.environ.get("GSIM_LIB") or os.path.join(_HERE, "libgsim_hip.so")

OK = 0
METRIC_TANIMOTO = 0
METRIC_TVERSKY = 1
JOIN_BY_ROW = 0
JOIN_BY_SCORE = 1
SYNTH_SPARSE = 0
SYNTH_DENSE = 1
SYNTH_MORGAN = 2
SELECT_CAP = 8192
GROUP_MAX = 0
GROUP_MIN = 1
GROUP_MEAN = 2
GROUP_MAX_QUERIES = 1024
LEADER_NONE = 0xFFFFFFFF
KNN_MAX_K = 128
KNN_EXCLUDE_SELF = 1
HIST_MAX_EDGES = 128
HIST_EXCLUDE_SELF = 1
POPINDEX_ROWS = 1
ROW_NONE = 0xFFFFFFFF
ROWHASH_REPEATS = 1

HIT_DTYPE = np.dtype([("row", "<u4"), ("score", "<f4"), ("common", "<u2"), ("popc_db", "<u2")])
GROUP_HIT_DTYPE = np.dtype([("row", "<u4"), ("score", "<f4"), ("which", "<u2"), ("popc_db", "<u2")])
HEADER_DTYPE = np.dtype([("count", "<u4"), ("flags", "<u4"), ("approx", "<u8")])


class GsimTiming(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("scan_ms_sum", C.c_double), ("select_ms_sum", C.c_double),
                ("candidates_sum", C.c_uint64), ("finalists_sum", C.c_uint64), ("handed_back", C.c_uint64),
                ("batches", C.c_uint64), ("batch_kernel_ms_sum", C.c_double), ("handed_back_why", C.c_uint64), ("batches_dense_cutoff", C.c_uint64),
                ("collectives", C.c_uint64), ("gather_ms_sum", C.c_double), ("merge_ms_sum", C.c_double),
                ("blocks_rechecked", C.c_uint64), ("blocks_torn", C.c_uint64), ("batches_regrown", C.c_uint64),
                ("large_k_single_scan", C.c_uint64), ("rerun_own", C.c_uint64), ("rerun_publish", C.c_uint64),
                ("rerun_behind", C.c_uint64), ("rerun_torn", C.c_uint64), ("lane_queries", C.c_uint64), ("backoff_skips", C.c_uint64)]


class GsimGraphStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("launches_rerun", C.c_uint64), ("pairs", C.c_uint64), ("tile_ms", C.c_double),
                ("csr_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


class GsimJoinStats(C.Structure):
    _fields_ = [("rows_streamed", C.c_uint64), ("rows_tiled", C.c_uint64), ("stream_launches", C.c_uint64),
                ("tile_launches", C.c_uint64), ("launches_rerun", C.c_uint64), ("pairs", C.c_uint64), ("stream_ms", C.c_double),
                ("tile_ms", C.c_double), ("csr_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double),
                ("clock_mhz", C.c_double)]


class GsimMaxMinStats(C.Structure):
    _fields_ = [("picks", C.c_uint64), ("launches", C.c_uint64), ("rows_updated", C.c_uint64), ("kernel_ms", C.c_double),
                ("d2h_ms", C.c_double), ("wall_ms", C.c_double)]


class GsimRowsetStats(C.Structure):
    _fields_ = [("selected", C.c_uint64), ("queries_gather", C.c_uint64), ("queries_stream", C.c_uint64), ("launches", C.c_uint64),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double)]


class GsimPopindexStats(C.Structure):
    _fields_ = [("rows_scanned", C.c_uint64), ("rows_window", C.c_uint64), ("queries_one_stage", C.c_uint64),
                ("queries_two_stage", C.c_uint64), ("queries_plain", C.c_uint64), ("launches", C.c_uint64), ("bounds_ms", C.c_double),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double)]


class GsimRowhashStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("groups", C.c_uint64), ("repeated_groups", C.c_uint64), ("largest_group", C.c_uint64),
                ("slots", C.c_uint64), ("launches", C.c_uint64), ("kernel_ms", C.c_double), ("wall_ms", C.c_double)]


class GsimGroupStats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("launches", C.c_uint64), ("pairs", C.c_uint64), ("scan_ms", C.c_double),
                ("kernel_ms", C.c_double), ("wall_ms", C.c_double)]


class GsimLeaderStats(C.Structure):
    _fields_ = [("leaders", C.c_uint64), ("rounds", C.c_uint64), ("launches", C.c_uint64), ("pairs", C.c_uint64),
                ("assigned", C.c_uint64), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double),
                ("resolve_ms", C.c_double), ("compact_ms", C.c_double)]


class GsimKnnStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("launches", C.c_uint64), ("pairs", C.c_uint64), ("inserts", C.c_uint64),
                ("entries", C.c_uint64), ("kernel_ms", C.c_double), ("csr_ms", C.c_double), ("d2h_ms", C.c_double),
                ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


class GsimKnnJoinStats(C.Structure):
    _fields_ = [("left_rows", C.c_uint64), ("table_rows", C.c_uint64), ("segments", C.c_uint64), ("fold_launches", C.c_uint64),
                ("merge_launches", C.c_uint64), ("pairs", C.c_uint64), ("inserts", C.c_uint64), ("partial_entries", C.c_uint64),
                ("entries", C.c_uint64), ("kernel_ms", C.c_double), ("merge_ms", C.c_double), ("csr_ms", C.c_double),
                ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


class GsimHistStats(C.Structure):
    _fields_ = [("left_rows", C.c_uint64), ("rows_streamed", C.c_uint64), ("rows_tiled", C.c_uint64), ("stream_launches", C.c_uint64),
                ("tile_launches", C.c_uint64), ("pairs", C.c_uint64), ("stream_ms", C.c_double), ("tile_ms", C.c_double),
                ("reduce_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


class GsimScoresStats(C.Structure):
    _fields_ = [("left_rows", C.c_uint64), ("right_rows", C.c_uint64), ("launches", C.c_uint64), ("slabs", C.c_uint64),
                ("pairs", C.c_uint64), ("prepare_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double),
                ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


class GsimComponentsStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("levels", C.c_uint64), ("launches", C.c_uint64), ("pairs", C.c_uint64), ("kept", C.c_uint64),
                ("unions", C.c_uint64), ("cas_failed", C.c_uint64), ("kernel_ms", C.c_double), ("label_ms", C.c_double),
                ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


DBSCAN_NOISE = 0xFFFFFFFF


class GsimDbscanStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("launches_count", C.c_uint64), ("launches_link", C.c_uint64), ("pairs", C.c_uint64),
                ("kept", C.c_uint64), ("cores", C.c_uint64), ("borders", C.c_uint64), ("noise", C.c_uint64), ("clusters", C.c_uint64),
                ("unions", C.c_uint64), ("cas_failed", C.c_uint64), ("count_ms", C.c_double), ("link_ms", C.c_double),
                ("label_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


MST_MAX_ROUNDS = 33
MST_EDGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("score", np.float32)])
MST_MERGE_DTYPE = np.dtype([("left", np.uint32), ("right", np.uint32), ("score", np.float32), ("size", np.uint32)])


class GsimMstStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("rounds", C.c_uint64), ("scans", C.c_uint64), ("launches", C.c_uint64), ("pairs", C.c_uint64),
                ("owner_rows", C.c_uint64), ("edges", C.c_uint64), ("kernel_ms", C.c_double), ("round_ms", C.c_double),
                ("sort_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double),
                ("scan_owners", C.c_uint64 * MST_MAX_ROUNDS), ("scan_kernel_ms", C.c_double * MST_MAX_ROUNDS)]


HDBSCAN_NOISE = 0xFFFFFFFF
HDBSCAN_EOM, HDBSCAN_LEAF, HDBSCAN_NO_ROOTS = 0, 1, 2


class GsimMreachStats(C.Structure):
    _fields_ = [("mst", GsimMstStats), ("core_launches", C.c_uint64), ("core_inserts", C.c_uint64), ("core_rows", C.c_uint64),
                ("core_kernel_ms", C.c_double), ("core_tail_ms", C.c_double)]


class GsimHdbscanStats(C.Structure):
    _fields_ = [("forest", GsimMreachStats), ("clusters", C.c_uint64), ("noise", C.c_uint64), ("select_ms", C.c_double),
                ("wall_ms", C.c_double)]


def _stats_dict(st):
    """every field of a stats struct"""
    return {f: getattr(st, f) for f, _ in st._fields_}


def _level_buffers(n, nl, first_row=True, sizes=True):
    """The outputs of a call with levels: labels [nl, n], counts [nl], first_row and sizes [nl, n] (None where not asked for)"""
    shape = (max(nl, 1), n)
    return (np.empty(shape, dtype=np.uint32), np.zeros(shape[0], dtype=np.uint32), np.empty(shape, dtype=np.uint32) if first_row else None,
            np.empty(shape, dtype=np.uint32) if sizes else None)


def _levels(nl, comp, ncomp, first, size):
    """levels[l] = (labels [n], first_row [count], sizes [count]) from _level_buffers' arrays once the call has filled them"""
    return [(comp[l].copy(), first[l, :ncomp[l]].copy() if first is not None else None, size[l, :ncomp[l]].copy() if size is not None else None)
            for l in range(nl)]


def _mst_stats_dict(st):
    stats = {f: getattr(st, f) for f, _ in GsimMstStats._fields_[:-2]}
    stats["scan_owners"] = list(st.scan_owners)[:st.scans]
    stats["scan_kernel_ms"] = list(st.scan_kernel_ms)[:st.scans]
    return stats


def _mreach_stats_dict(st):
    stats = _mst_stats_dict(st.mst)
    stats.update({f: getattr(st, f) for f, _ in GsimMreachStats._fields_[1:]})
    return stats


PROFILE_STREAMED, PROFILE_GATHERED, PROFILE_MATRIX, PROFILE_VALU = 1, 2, 4, 8
ISIM_TANIMOTO, ISIM_RUSSELL_RAO, ISIM_SIMPLE_MATCHING = 0, 1, 2


class GsimProfileStats(C.Structure):
    _fields_ = [("rows_read", C.c_uint64), ("rows_counted", C.c_uint64), ("launches", C.c_uint64), ("route", C.c_uint64),
                ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double)]


LABEL_NONE = 0xFFFFFFFF  # == LEADER_NONE: gsim_db_label_counts counts the row nowhere
ASSIGN_MAX_CENTRES = 65536


class GsimAssignStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("centres", C.c_uint64), ("launches", C.c_uint64), ("pairs", C.c_uint64),
                ("prepare_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double),
                ("clock_mhz", C.c_double)]


class GsimLabelStats(C.Structure):
    _fields_ = [("rows_read", C.c_uint64), ("rows_counted", C.c_uint64), ("labels", C.c_uint64), ("launches", C.c_uint64),
                ("sort_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double)]


class GsimKmeansStats(C.Structure):
    _fields_ = [("iterations", C.c_uint64), ("converged", C.c_uint64), ("changed_last", C.c_uint64), ("assign_ms", C.c_double),
                ("counts_ms", C.c_double), ("update_ms", C.c_double), ("wall_ms", C.c_double)]


LABEL_SUMS_OWN_ONLY = 1


class GsimLabelSumsStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("rows_labelled", C.c_uint64), ("labels_nonempty", C.c_uint64), ("pairs", C.c_uint64),
                ("launches", C.c_uint64), ("sort_ms", C.c_double), ("gather_ms", C.c_double), ("kernel_ms", C.c_double),
                ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


class GsimLabelSearchStats(C.Structure):
    _fields_ = [("queries", C.c_uint64), ("labels", C.c_uint64), ("passes", C.c_uint64), ("passes_lds", C.c_uint64),
                ("passes_global", C.c_uint64), ("launches", C.c_uint64), ("scan_ms", C.c_double), ("finish_ms", C.c_double),
                ("d2h_ms", C.c_double), ("wall_ms", C.c_double)]


LINKAGE_COMPLETE = 0
LINKAGE_AVERAGE = 1
LINKAGE_MAX_ROWS = 65536
LINKAGE_MERGE_DTYPE = np.dtype([("a", np.uint32), ("b", np.uint32), ("left", np.uint32), ("right", np.uint32), ("size", np.uint32),
                                ("score", np.float32), ("sum_q", np.uint64)])


class GsimLinkageStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("merges", C.c_uint64), ("scans", C.c_uint64), ("chain_max", C.c_uint64), ("launches", C.c_uint64),
                ("launch_steps", C.c_uint64), ("matrix_ms", C.c_double), ("chain_ms", C.c_double), ("order_ms", C.c_double),
                ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


SNN_CLOSED = 1  # the lists count their owners (the 1973 paper's convention)
SNN_EITHER = 2  # jarvis_patrick: one-sided pairs may link too
SNN_MUTUAL_BIT = 0x80000000


class GsimSnnStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("k", C.c_uint64), ("entries", C.c_uint64), ("mutual_entries", C.c_uint64),
                ("links", C.c_uint64 * 8), ("unions", C.c_uint64), ("cas_failed", C.c_uint64), ("launches", C.c_uint64),
                ("pairs", C.c_uint64), ("inserts", C.c_uint64), ("knn_ms", C.c_double), ("sort_ms", C.c_double), ("link_ms", C.c_double),
                ("label_ms", C.c_double), ("d2h_ms", C.c_double), ("wall_ms", C.c_double), ("clock_mhz", C.c_double)]


def _snn_stats_dict(st):
    d = _stats_dict(st)
    d["links"] = list(st.links)
    return d


class GsimError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("gsim error %d: %s" % (code, msg))
        self.code = code


_lib = None

EXPORTS = [
    "gsim_device_count", "gsim_device_free_bytes", "gsim_available_device_bytes", "gsim_next_device",
    "gsim_db_create", "gsim_db_add_rows", "gsim_db_finalize", "gsim_db_set_fold_factor", "gsim_db_fold_factor", "gsim_db_set_fold_full_on_device",
    "gsim_fold_fingerprint", "gsim_db_generate", "gsim_db_generate_sharded", "gsim_synth_row", "gsim_db_attach_device_rows",
    "gsim_db_destroy", "gsim_db_count", "gsim_db_fp_bits", "gsim_db_data_bytes", "gsim_db_row",
    "gsim_db_shard_count", "gsim_db_shard_device", "gsim_db_search", "gsim_db_search_each", "gsim_db_search_timed", "gsim_db_search_cpu", "gsim_db_set_stream", "gsim_db_set_row_base",
    "gsim_result_block_bytes", "gsim_db_search_device", "gsim_merge_device", "gsim_db_search_batch_device",
    "gsim_merge_device_batch", "gsim_merge_host",
    "gsim_comm_create", "gsim_comm_destroy", "gsim_comm_size", "gsim_rccl_info", "gsim_db_set_comm", "gsim_db_set_comm_root",
    "gsim_db_enable_timing",
    "gsim_db_neighbors", "gsim_graph_shape", "gsim_graph_copy", "gsim_graph_get_stats", "gsim_graph_destroy", "gsim_butina",
    "gsim_db_join_queries", "gsim_db_join", "gsim_graph_get_join_stats",
    "gsim_db_maxmin",
    "gsim_rowset_from_rows", "gsim_rowset_from_bitmap", "gsim_rowset_count", "gsim_rowset_rows", "gsim_rowset_destroy", "gsim_db_search_rows",
    "gsim_db_search_group",
    "gsim_db_leader",
    "gsim_db_knn", "gsim_graph_get_knn_stats",
    "gsim_db_knn_join", "gsim_db_knn_queries", "gsim_graph_get_knn_join_stats",
    "gsim_db_histogram_queries", "gsim_db_histogram",
    "gsim_db_scores", "gsim_db_scores_queries", "gsim_db_scores_device",
    "gsim_db_components", "gsim_components",
    "gsim_db_mst", "gsim_mst", "gsim_mst_linkage", "gsim_mst_cut",
    "gsim_db_dbscan", "gsim_dbscan",
    "gsim_db_core_scores", "gsim_db_mreach_mst", "gsim_db_hdbscan", "gsim_mreach_mst", "gsim_mst_hdbscan",
    "gsim_db_bit_counts", "gsim_db_overlap_sums", "gsim_isim", "gsim_isim_complement",
    "gsim_db_assign", "gsim_db_label_counts", "gsim_label_centroids", "gsim_db_kmeans",
    "gsim_db_label_sums", "gsim_label_silhouette", "gsim_label_medoids",
    "gsim_labelset_create", "gsim_labelset_sizes", "gsim_labelset_destroy", "gsim_db_search_labels",
    "gsim_db_linkage", "gsim_linkage",
    "gsim_db_snn", "gsim_graph_copy_shared", "gsim_graph_get_snn_stats", "gsim_db_jarvis_patrick", "gsim_snn", "gsim_jarvis_patrick",
    "gsim_popindex_create", "gsim_popindex_first", "gsim_popindex_order", "gsim_popindex_destroy", "gsim_popcount_bounds", "gsim_db_search_bounded",
    "gsim_rowhash_create", "gsim_rowhash_get_stats", "gsim_rowhash_groups", "gsim_rowhash_rowset", "gsim_rowhash_find", "gsim_rowhash_find_db",
    "gsim_rowhash_destroy", "gsim_row_hash", "gsim_duplicates",
    "gsim_db_get_timing", "gsim_debug_query_flags", "gsim_debug_litmus", "gsim_debug_score_table", "gsim_debug_prefilter_constants", "gsim_debug_sort_desc", "gsim_last_error", "gsim_version",
]


def load():
    """Load libgsim_hip.so.  PyTorch (when importable) is imported FIRST so that the
    process holds exactly one HIP runtime: torch ships its own libamdhip64.so.7 and
    the dynamic linker then resolves our NEEDED entry to that same object."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GsimError(-100, "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C gpusimilarity_amd/csrc`" % LIB_PATH)
    if os.environ.get("GSIM_NO_TORCH", "") != "1" and "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:  # torch is plumbing, not a requirement of the ABI
            pass
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    u32p, u64p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.c_void_p
    sig = {
        "gsim_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "gsim_device_free_bytes": (C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
        "gsim_available_device_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
        "gsim_next_device": (C.c_int, [C.c_size_t, C.POINTER(C.c_int)]),
        "gsim_db_create": (C.c_int, [C.c_uint32, C.POINTER(vp)]),
        "gsim_db_add_rows": (C.c_int, [vp, u32p, C.c_uint64]),
        "gsim_db_finalize": (C.c_int, [vp, C.c_int, C.c_int]),
        "gsim_db_set_fold_factor": (C.c_int, [vp, C.c_uint32]),
        "gsim_db_fold_factor": (C.c_uint32, [vp]),
        "gsim_db_set_fold_full_on_device": (C.c_int, [vp, C.c_int]),
        "gsim_fold_fingerprint": (C.c_int, [u32p, C.c_uint32, C.c_uint32, u32p]),
        "gsim_db_generate": (C.c_int, [vp, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int]),
        "gsim_db_generate_sharded": (C.c_int, [vp, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int]),
        "gsim_synth_row": (C.c_int, [C.c_uint64, C.c_int, C.c_uint64, C.c_uint32, u32p]),
        "gsim_db_attach_device_rows": (C.c_int, [vp, vp, C.c_uint64, C.c_int]),
        "gsim_db_destroy": (C.c_int, [vp]),
        "gsim_db_count": (C.c_uint64, [vp]),
        "gsim_db_fp_bits": (C.c_uint32, [vp]),
        "gsim_db_data_bytes": (C.c_size_t, [vp]),
        "gsim_db_row": (C.c_int, [vp, C.c_uint64, u32p]),
        "gsim_db_shard_count": (C.c_int, [vp]),
        "gsim_db_shard_device": (C.c_int, [vp, C.c_int]),
        "gsim_db_search": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float,
                                     vp, u32p, u64p]),
        "gsim_db_search_each": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float,
                                          vp, u32p, u64p]),
        "gsim_db_search_timed": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float,
                                           vp, u32p, u64p, C.POINTER(C.c_double)]),
        "gsim_db_search_cpu": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, C.c_float, vp, u32p]),
        "gsim_db_set_stream": (C.c_int, [vp, vp]),
        "gsim_db_set_row_base": (C.c_int, [vp, C.c_uint32]),
        "gsim_result_block_bytes": (C.c_size_t, [C.c_uint32]),
        "gsim_db_search_device": (C.c_int, [vp, u32p, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, vp]),
        "gsim_merge_device": (C.c_int, [C.c_int, vp, vp, C.c_uint32, C.c_size_t, C.c_uint32, vp]),
        "gsim_db_search_batch_device": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float,
                                                  C.c_float, vp]),
        "gsim_merge_device_batch": (C.c_int, [C.c_int, vp, vp, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32, vp]),
        "gsim_merge_host": (C.c_int, [vp, C.c_uint32, C.c_size_t, C.c_uint32, vp]),
        "gsim_comm_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]),
        "gsim_comm_destroy": (C.c_int, [vp]),
        "gsim_rccl_info": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_size_t]),
        "gsim_comm_size": (C.c_int, [vp]),
        "gsim_db_set_comm": (C.c_int, [vp, vp]),
        "gsim_db_set_comm_root": (C.c_int, [vp, C.c_int]),
        "gsim_db_enable_timing": (C.c_int, [vp, C.c_int]),
        "gsim_db_get_timing": (C.c_int, [vp, C.POINTER(GsimTiming)]),
        "gsim_debug_litmus": (C.c_int, [C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_ulonglong)]),
        "gsim_debug_query_flags": (C.c_int, [vp, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)]),
        "gsim_debug_score_table": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.POINTER(C.c_float)]),
        "gsim_debug_sort_desc": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32]),
        "gsim_debug_prefilter_constants": (C.c_int, [C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_int, C.c_float,
                                                      C.POINTER(C.c_float)]),
        "gsim_db_neighbors": (C.c_int, [vp, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.POINTER(vp)]),
        "gsim_graph_shape": (C.c_int, [vp, u64p, u64p]),
        "gsim_graph_copy": (C.c_int, [vp, u64p, u32p, C.POINTER(C.c_float)]),
        "gsim_graph_get_stats": (C.c_int, [vp, C.POINTER(GsimGraphStats)]),
        "gsim_graph_destroy": (C.c_int, [vp]),
        "gsim_db_join_queries": (C.c_int, [vp, u32p, C.c_uint64, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(vp)]),
        "gsim_db_join": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.c_float, C.c_int, C.c_float, C.c_float, C.c_int, C.POINTER(vp)]),
        "gsim_graph_get_join_stats": (C.c_int, [vp, C.POINTER(GsimJoinStats)]),
        "gsim_butina": (C.c_int, [u64p, u32p, C.c_uint64, u32p, u32p, u64p]),
        "gsim_db_maxmin": (C.c_int, [vp, C.c_uint32, u32p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_float, u32p,
                                     C.POINTER(C.c_float), u32p, C.POINTER(C.c_float), u32p, C.POINTER(GsimMaxMinStats)]),
        "gsim_rowset_from_rows": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint32, C.POINTER(vp)]),
        "gsim_rowset_from_bitmap": (C.c_int, [vp, u32p, C.c_uint32, C.POINTER(vp)]),
        "gsim_rowset_count": (C.c_int, [vp, u64p]),
        "gsim_rowset_rows": (C.c_int, [vp, u32p]),
        "gsim_rowset_destroy": (C.c_int, [vp]),
        "gsim_db_search_rows": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, vp, u32p, u64p,
                                          C.POINTER(GsimRowsetStats)]),
        "gsim_db_search_group": (C.c_int, [vp, u32p, C.c_uint32, C.c_int, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, vp, u32p, u64p,
                                           C.POINTER(GsimGroupStats)]),
        "gsim_db_knn": (C.c_int, [vp, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.POINTER(vp)]),
        "gsim_graph_get_knn_stats": (C.c_int, [vp, C.POINTER(GsimKnnStats)]),
        "gsim_db_knn_join": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint32,
                                       C.POINTER(vp)]),
        "gsim_db_knn_queries": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(vp)]),
        "gsim_graph_get_knn_join_stats": (C.c_int, [vp, C.POINTER(GsimKnnJoinStats)]),
        "gsim_db_histogram_queries": (C.c_int, [vp, u32p, C.c_uint64, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_float, C.c_float, u64p, u64p,
                                                C.POINTER(GsimHistStats)]),
        "gsim_db_histogram": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_float, C.c_float,
                                        C.c_uint32, u64p, u64p, C.POINTER(GsimHistStats)]),
        "gsim_db_scores": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float,
                                     C.POINTER(C.c_float), C.c_uint64, C.POINTER(GsimScoresStats)]),
        "gsim_db_scores_queries": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float,
                                             C.POINTER(C.c_float), C.c_uint64, C.POINTER(GsimScoresStats)]),
        "gsim_db_scores_device": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float,
                                            vp, C.c_uint64, C.POINTER(GsimScoresStats)]),
        "gsim_db_leader": (C.c_int, [vp, C.c_float, u32p, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, u32p, u32p, u32p,
                                     C.POINTER(C.c_float), C.POINTER(GsimLeaderStats)]),
        "gsim_db_components": (C.c_int, [vp, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.c_float, C.c_float, u32p, u32p, u32p, u32p,
                                         C.POINTER(GsimComponentsStats)]),
        "gsim_components": (C.c_int, [u64p, u32p, C.c_uint64, u32p, u32p, u32p, u64p]),
        "gsim_db_mst": (C.c_int, [vp, C.c_float, C.c_int, C.c_float, C.c_float, vp, u64p, C.POINTER(GsimMstStats)]),
        "gsim_mst": (C.c_int, [u64p, u32p, C.POINTER(C.c_float), C.c_uint64, vp, u64p]),
        "gsim_db_dbscan": (C.c_int, [vp, C.c_float, C.c_uint32, C.c_int, C.c_float, C.c_float, u32p, u32p, u32p, u32p, u32p, u32p,
                                     C.POINTER(GsimDbscanStats)]),
        "gsim_dbscan": (C.c_int, [u64p, u32p, C.POINTER(C.c_float), C.c_uint64, C.c_uint32, u32p, u32p, u32p, u32p, u64p]),
        "gsim_mst_linkage": (C.c_int, [vp, C.c_uint64, C.c_uint64, vp]),
        "gsim_mst_cut": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_float, u32p, u32p, u32p, u64p]),
        "gsim_db_core_scores": (C.c_int, [vp, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float),
                                          C.POINTER(GsimKnnStats)]),
        "gsim_db_mreach_mst": (C.c_int, [vp, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, vp, u64p, C.POINTER(C.c_float),
                                         C.POINTER(GsimMreachStats)]),
        "gsim_db_hdbscan": (C.c_int, [vp, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint32, u32p, u64p,
                                      C.POINTER(C.c_float), u32p, u32p, C.POINTER(C.c_float), C.POINTER(C.c_double),
                                      C.POINTER(GsimHdbscanStats)]),
        "gsim_mreach_mst": (C.c_int, [u64p, u32p, C.POINTER(C.c_float), C.c_uint64, C.c_uint32, vp, u64p, C.POINTER(C.c_float)]),
        "gsim_mst_hdbscan": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_float, C.c_uint32, C.c_uint32, u32p, u64p, C.POINTER(C.c_float),
                                       u32p, u32p, C.POINTER(C.c_float), C.POINTER(C.c_double)]),
        "gsim_db_bit_counts": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, u64p, u64p, C.POINTER(GsimProfileStats)]),
        "gsim_db_overlap_sums": (C.c_int, [vp, u32p, C.c_uint64, C.c_uint64, u64p, u32p, C.POINTER(GsimProfileStats)]),
        "gsim_isim": (C.c_int, [u64p, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(C.c_double)]),
        "gsim_isim_complement": (C.c_int, [u64p, C.c_uint32, C.c_uint64, C.c_int, u64p, u32p, C.c_uint64, C.POINTER(C.c_double)]),
        "gsim_db_assign": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float, u32p,
                                     C.POINTER(C.c_float), C.POINTER(GsimAssignStats)]),
        "gsim_db_label_counts": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint64, C.c_uint64, u32p, u32p, C.POINTER(GsimLabelStats)]),
        "gsim_label_centroids": (C.c_int, [u32p, u32p, C.c_uint32, C.c_uint32, u32p, u32p]),
        "gsim_db_label_sums": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_uint64,
                                         C.POINTER(C.c_uint64), u32p, C.POINTER(C.c_uint64), u32p, C.POINTER(GsimLabelSumsStats)]),
        "gsim_label_silhouette": (C.c_int, [u32p, C.POINTER(C.c_uint64), u32p, C.POINTER(C.c_uint64), u32p, C.c_uint64, C.c_uint32,
                                            C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "gsim_label_medoids": (C.c_int, [u32p, C.POINTER(C.c_uint64), C.c_uint64, C.c_uint32, u32p]),
        "gsim_labelset_create": (C.c_int, [vp, u32p, C.c_uint32, C.POINTER(vp)]),
        "gsim_labelset_sizes": (C.c_int, [vp, u32p, u64p, u64p]),
        "gsim_labelset_destroy": (C.c_int, [vp]),
        "gsim_db_search_labels": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint64,
                                            vp, u32p, u32p, u64p, u64p, vp, u32p, C.POINTER(GsimLabelSearchStats)]),
        "gsim_db_linkage": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32, vp, u64p,
                                      C.POINTER(GsimLinkageStats)]),
        "gsim_linkage": (C.c_int, [C.POINTER(C.c_float), C.c_uint64, C.c_uint64, C.c_int, vp, u64p, u64p]),
        "gsim_db_snn": (C.c_int, [vp, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint32, C.POINTER(vp)]),
        "gsim_graph_copy_shared": (C.c_int, [vp, u32p]),
        "gsim_graph_get_snn_stats": (C.c_int, [vp, C.POINTER(GsimSnnStats)]),
        "gsim_db_jarvis_patrick": (C.c_int, [vp, C.c_uint32, u32p, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, C.c_uint32, u32p, u32p,
                                             u32p, u32p, C.POINTER(GsimSnnStats)]),
        "gsim_snn": (C.c_int, [u64p, u32p, C.c_uint64, C.c_uint32, u32p]),
        "gsim_jarvis_patrick": (C.c_int, [u64p, u32p, C.c_uint64, u32p, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p]),
        "gsim_db_kmeans": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, u32p, u32p,
                                     C.POINTER(C.c_float), u32p, C.POINTER(GsimKmeansStats)]),
        "gsim_popindex_create": (C.c_int, [vp, C.c_uint32, C.POINTER(vp)]),
        "gsim_popindex_first": (C.c_int, [vp, u64p]),
        "gsim_popindex_order": (C.c_int, [vp, u32p]),
        "gsim_popindex_destroy": (C.c_int, [vp]),
        "gsim_popcount_bounds": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float)]),
        "gsim_db_search_bounded": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, C.c_float, C.c_int, C.c_float, C.c_float, vp, u32p, u64p,
                                             C.POINTER(GsimPopindexStats)]),
        "gsim_rowhash_create": (C.c_int, [vp, C.c_uint32, C.POINTER(vp)]),
        "gsim_rowhash_get_stats": (C.c_int, [vp, C.POINTER(GsimRowhashStats)]),
        "gsim_rowhash_groups": (C.c_int, [vp, u32p, u32p]),
        "gsim_rowhash_rowset": (C.c_int, [vp, C.c_uint32, C.POINTER(vp)]),
        "gsim_rowhash_find": (C.c_int, [vp, u32p, C.c_uint64, u32p, u32p]),
        "gsim_rowhash_find_db": (C.c_int, [vp, vp, C.c_uint64, C.c_uint64, u32p, u32p]),
        "gsim_rowhash_destroy": (C.c_int, [vp]),
        "gsim_row_hash": (C.c_int, [u32p, C.c_uint64, C.c_uint32, u64p]),
        "gsim_duplicates": (C.c_int, [u32p, C.c_uint64, C.c_uint32, u32p, u32p, u64p]),
        "gsim_last_error": (C.c_char_p, []),
        "gsim_version": (C.c_char_p, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise GsimError(rc, load().gsim_last_error().decode("utf-8", "replace"))


def device_count() -> int:
    n = C.c_int(0)
    check(load().gsim_device_count(C.byref(n)))
    return n.value


def device_free_bytes(device: int) -> int:
    v = C.c_size_t(0)
    check(load().gsim_device_free_bytes(device, C.byref(v)))
    return v.value


def available_device_bytes() -> int:
    v = C.c_size_t(0)
    check(load().gsim_available_device_bytes(C.byref(v)))
    return v.value


def next_device(required_bytes: int) -> int:
    d = C.c_int(-1)
    check(load().gsim_next_device(required_bytes, C.byref(d)))
    return d.value


def synth_row(seed: int, kind: int, row: int, fp_bits: int) -> np.ndarray:
    """Row `row` of the synthetic table gsim_db_generate makes (host twin of the device generator)."""
    out = np.empty(fp_bits // 32, dtype=np.uint32)
    check(load().gsim_synth_row(seed, kind, row, fp_bits, _u32(out)))
    return out


def result_block_bytes(k: int) -> int:
    return int(load().gsim_result_block_bytes(k))


def _u32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _f32(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _hdbscan_buffers(n):
    """label_of, leave [n]; first_row, sizes, birth, stability [capacity n]"""
    m = max(n, 1)
    return [np.empty(n, np.uint32), np.empty(n, np.float32), np.empty(m, np.uint32), np.empty(m, np.uint32), np.empty(m, np.float32),
            np.empty(m, np.float64)]


class RowSet:
    """``gsim_rowset``: a set of rows of one :class:`Table` (Table.rowset makes it, Table.search_rows searches inside it).
    It lives in the table's device memory: close it (or drop it) before the table."""

    def __init__(self, table, handle):
        self._L = table._L
        self._h = handle
        self._table = table  # (keeps the handle it belongs to alive)

    @property
    def count(self) -> int:
        n = C.c_uint64(0)
        check(self._L.gsim_rowset_count(self._h, C.byref(n)))
        return n.value

    def rows(self) -> np.ndarray:
        """The selected rows, ascending, row base included."""
        out = np.empty(self.count, dtype=np.uint32)
        check(self._L.gsim_rowset_rows(self._h, _u32(out) if len(out) else None))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsim_rowset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PopIndex:
    """``gsim_popindex``: the rows of one :class:`Table` ordered by popcount (Table.popindex makes it, Table.search_bounded searches
    through it).  It lives in the table's device memory: close it (or drop it) before the table."""

    def __init__(self, table, handle, flags):
        self._L = table._L
        self._h = handle
        self._table = table  # (keeps the handle it belongs to alive)
        self.flags = int(flags)
        self.fp_bits = table.W * 32
        self.nrows = table.count()

    def first(self) -> np.ndarray:
        """first[b], b = 0 .. fp_bits + 1: the number of rows with a popcount below b (uint64)."""
        out = np.zeros(self.fp_bits + 2, dtype=np.uint64)
        check(self._L.gsim_popindex_first(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out

    def order(self) -> np.ndarray:
        """The table's rows sorted by (popcount, row), row base included (uint32)."""
        out = np.empty(self.nrows, dtype=np.uint32)
        check(self._L.gsim_popindex_order(self._h, _u32(out) if len(out) else None))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsim_popindex_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def popcount_bounds(fp_bits, popc_query, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0) -> np.ndarray:
    """gsim_popcount_bounds (host): ub[b], b = 0 .. fp_bits -- the largest score a row with b bits set can have against a query with
    `popc_query` bits set, exact in f32."""
    ub = np.empty(fp_bits + 1 if 0 < fp_bits <= 32768 else 1, dtype=np.float32)
    check(load().gsim_popcount_bounds(fp_bits, popc_query, metric, alpha, beta, _f32(ub)))
    return ub


class RowHash:
    """``gsim_rowhash``: the hash table over the rows of one :class:`Table` (Table.rowhash makes it): which rows are the same
    fingerprint, and where a given fingerprint is.  It lives in the table's device memory: close it (or drop it) before the table."""

    def __init__(self, table, handle):
        self._L = table._L
        self._h = handle
        self._table = table  # (keeps the handle it belongs to alive)
        self.nrows = table.count()

    def stats(self) -> dict:
        """The build's gsim_rowhash_stats: rows, groups, repeated_groups, largest_group, slots, launches, kernel_ms, wall_ms."""
        st = GsimRowhashStats()
        check(self._L.gsim_rowhash_get_stats(self._h, C.byref(st)))
        return _stats_dict(st)

    def groups(self):
        """(first, size), uint32 [N]: the lowest row identical to row i (row base included) and the number of rows identical to it."""
        first, size = np.empty(self.nrows, np.uint32), np.empty(self.nrows, np.uint32)
        check(self._L.gsim_rowhash_groups(self._h, _u32(first), _u32(size)))
        return first, size

    def rowset(self, repeats=False) -> RowSet:
        """The rows that are their group's first -- one per distinct fingerprint -- as a :class:`RowSet` of the table;
        repeats=True (GSIM_ROWHASH_REPEATS): every other row."""
        h = C.c_void_p()
        check(self._L.gsim_rowhash_rowset(self._h, ROWHASH_REPEATS if repeats else 0, C.byref(h)))
        return RowSet(self._table, h)

    def find(self, queries, size=True):
        """gsim_rowhash_find: (row, size), uint32 [nq] -- the lowest table row identical to each query (row base included; ROW_NONE
        where there is none) and the size of its group; size=False passes NULL for it (None in its place)."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self._table.W)
        row = np.empty(len(q), np.uint32)
        sz = np.empty(len(q), np.uint32) if size else None
        check(self._L.gsim_rowhash_find(self._h, _u32(q) if len(q) else None, len(q), _u32(row), _u32(sz) if size else None))
        return row, sz

    def find_db(self, table, begin=0, end=None):
        """gsim_rowhash_find_db: :meth:`find` for the rows [begin, end) of another :class:`Table` on the same device (or of this one)."""
        if end is None:
            end = table.count()
        n = max(end - begin, 0)
        row, sz = np.empty(n, np.uint32), np.empty(n, np.uint32)
        check(self._L.gsim_rowhash_find_db(self._h, table._h, begin, end, _u32(row), _u32(sz)))
        return row, sz

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsim_rowhash_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _host_rows(rows):
    r = np.ascontiguousarray(rows, dtype=np.uint32)
    if r.ndim != 2 or r.shape[1] == 0:
        raise ValueError("rows: an (n, fp_bits / 32) uint32 array")
    return r


def row_hash(rows) -> np.ndarray:
    """gsim_row_hash (host): the library's 64-bit hash of every row of an (n, W) uint32 array."""
    r = _host_rows(rows)
    out = np.empty(len(r), np.uint64)
    check(load().gsim_row_hash(_u32(r), len(r), r.shape[1] * 32, out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def duplicates(rows):
    """gsim_duplicates (host): (first, size, ngroups) of an (n, W) uint32 array -- the lowest row identical to row i, the number of
    rows identical to it, the number of distinct rows."""
    r = _host_rows(rows)
    first, size, n = np.empty(len(r), np.uint32), np.empty(len(r), np.uint32), C.c_uint64(0)
    check(load().gsim_duplicates(_u32(r), len(r), r.shape[1] * 32, _u32(first), _u32(size), C.byref(n)))
    return first, size, n.value


class LabelSet:
    """``gsim_labelset``: a labelling of one :class:`Table` on the device (Table.labelset makes it, Table.search_labels searches by
    it).  It lives in the table's device memory: close it (or drop it) before the table."""

    def __init__(self, table, handle, nlabels):
        self._L = table._L
        self._h = handle
        self._table = table  # (keeps the handle it belongs to alive)
        self.nlabels = int(nlabels)

    def sizes(self):
        """-> (sizes uint32 [nlabels], rows whose label is not LABEL_NONE, labels with at least one row)"""
        sizes = np.zeros(self.nlabels, dtype=np.uint32)
        labelled, nonempty = C.c_uint64(0), C.c_uint64(0)
        check(self._L.gsim_labelset_sizes(self._h, _u32(sizes), C.byref(labelled), C.byref(nonempty)))
        return sizes, labelled.value, nonempty.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsim_labelset_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Table:
    """A fingerprint table on the GPU(s): thin object wrapper over ``gsim_db``."""

    def __init__(self, fp_bits: int):
        self._L = load()
        h = C.c_void_p()
        check(self._L.gsim_db_create(fp_bits, C.byref(h)))
        self._h = h
        self.fp_bits = fp_bits
        self.W = fp_bits // 32

    # -- lifecycle ---------------------------------------------------------
    def add_rows(self, rows: np.ndarray):
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, self.W)
        check(self._L.gsim_db_add_rows(self._h, _u32(rows), rows.shape[0]))
        return self

    def set_fold_factor(self, fold_factor: int):
        check(self._L.gsim_db_set_fold_factor(self._h, fold_factor))
        return self

    def set_fold_full_on_device(self, allow: bool):
        check(self._L.gsim_db_set_fold_full_on_device(self._h, 1 if allow else 0))
        return self

    def fold_factor(self) -> int:
        return int(self._L.gsim_db_fold_factor(self._h))

    def finalize(self, device: int = 0, ndevices: int = 1):
        check(self._L.gsim_db_finalize(self._h, device, ndevices))
        return self

    def generate(self, seed: int, kind: int, first_row: int, nrows: int, device: int = 0, ndevices: int = 1):
        """The synthetic table in HBM; ndevices > 1: split over that many GPUs like finalize(device, ndevices)."""
        if ndevices > 1:
            check(self._L.gsim_db_generate_sharded(self._h, seed, kind, first_row, nrows, device, ndevices))
        else:
            check(self._L.gsim_db_generate(self._h, seed, kind, first_row, nrows, device))
        return self

    def attach_device_rows(self, ptr: int, nrows: int, device: int = 0):
        check(self._L.gsim_db_attach_device_rows(self._h, C.c_void_p(ptr), nrows, device))
        return self

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsim_db_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- accessors -----------------------------------------------------------
    def count(self) -> int:
        return int(self._L.gsim_db_count(self._h))

    def data_bytes(self) -> int:
        return int(self._L.gsim_db_data_bytes(self._h))

    def shard_count(self) -> int:
        return int(self._L.gsim_db_shard_count(self._h))

    def shard_devices(self):
        return [int(self._L.gsim_db_shard_device(self._h, i)) for i in range(self.shard_count())]

    def row(self, i: int) -> np.ndarray:
        out = np.empty(self.W, dtype=np.uint32)
        check(self._L.gsim_db_row(self._h, i, _u32(out)))
        return out

    # -- search ----------------------------------------------------------------
    def search(self, queries, k, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """-> (list of HIT_DTYPE arrays, one per query; approx uint64 array)"""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        nq = q.shape[0]
        hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
        counts = np.zeros(nq, dtype=np.uint32)
        approx = np.zeros(nq, dtype=np.uint64)
        check(self._L.gsim_db_search(self._h, _u32(q), nq, k, cutoff, metric, alpha, beta,
                                     hits.ctypes.data_as(C.c_void_p), _u32(counts),
                                     approx.ctypes.data_as(C.POINTER(C.c_uint64))))
        return [hits[i, :counts[i]].copy() for i in range(nq)], approx

    def neighbors(self, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, row_begin=0, row_end=None, stats=None):
        """gsim_db_neighbors: every row j != i with score(row i, row j) >= cutoff, for the rows i of [row_begin, row_end)
        -> CSR (indptr uint64 [n + 1], indices uint32 (+ row base), scores float32), each row's list by column.
        `stats`: a dict that receives the call's gsim_graph_stats."""
        if row_end is None:
            row_end = self.count()
        g = C.c_void_p()
        check(self._L.gsim_db_neighbors(self._h, cutoff, metric, alpha, beta, row_begin, row_end, C.byref(g)))
        return self._take_graph(g, stats, GsimGraphStats, self._L.gsim_graph_get_stats)

    def knn(self, k, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, row_begin=0, row_end=None, stats=None):
        """gsim_db_knn: for the rows i of [row_begin, row_end), the k most similar other rows j with
        score(query = row i, row j) >= cutoff -- gsim_db_search(row i, k + 1, cutoff) minus row i, cut to k
        -> CSR (indptr uint64 [n + 1], indices uint32 (+ row base), scores float32), each list by (score descending, row ascending).
        `stats`: a dict that receives the call's gsim_knn_stats."""
        if row_end is None:
            row_end = self.count()
        g = C.c_void_p()
        check(self._L.gsim_db_knn(self._h, k, cutoff, metric, alpha, beta, row_begin, row_end, C.byref(g)))
        return self._take_graph(g, stats, GsimKnnStats, self._L.gsim_graph_get_knn_stats)

    def knn_join(self, left, k, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, row_begin=0, row_end=None, exclude_self=False,
                 stats=None):
        """gsim_db_knn_join / gsim_db_knn_queries: for every left row, the k most similar rows j of THIS table with
        score(query = left row, row j) >= cutoff -- gsim_db_search(left row, k, cutoff) on this table
        -> CSR (indptr uint64 [nl + 1], indices uint32 (+ this table's row base), scores float32), each list by (score descending,
        row ascending).
        `left`: a Table on the same device (its rows [row_begin, row_end)) or a (nq, W) / (W,) uint32 array.
        `exclude_self` (only with left = this table): the pair (left row i, table row i) is not listed -- knn's lists.
        `stats`: a dict that receives the call's gsim_knn_join_stats."""
        g = C.c_void_p()
        if isinstance(left, Table):
            if row_end is None:
                row_end = left.count()
            check(self._L.gsim_db_knn_join(self._h, left._h, row_begin, row_end, k, cutoff, metric, alpha, beta,
                                           KNN_EXCLUDE_SELF if exclude_self else 0, C.byref(g)))
        else:
            if exclude_self:
                raise ValueError("exclude_self needs left to be this table")
            q = np.ascontiguousarray(left, dtype=np.uint32).reshape(-1, self.W)
            if row_end is None:
                row_end = q.shape[0]
            q = np.ascontiguousarray(q[row_begin:row_end])
            check(self._L.gsim_db_knn_queries(self._h, _u32(q) if len(q) else None, len(q), k, cutoff, metric, alpha, beta, C.byref(g)))
        return self._take_graph(g, stats, GsimKnnJoinStats, self._L.gsim_graph_get_knn_join_stats)

    def _take_graph(self, g, stats, stats_type, get_stats):
        """A gsim_graph -> (indptr, indices, scores) (+ its stats into the dict `stats`); the graph is destroyed."""
        try:
            n, nnz = C.c_uint64(0), C.c_uint64(0)
            check(self._L.gsim_graph_shape(g, C.byref(n), C.byref(nnz)))
            indptr = np.empty(n.value + 1, dtype=np.uint64)
            indices = np.empty(nnz.value, dtype=np.uint32)
            scores = np.empty(nnz.value, dtype=np.float32)
            check(self._L.gsim_graph_copy(g, indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices),
                                          scores.ctypes.data_as(C.POINTER(C.c_float))))
            if stats is not None:
                st = stats_type()
                check(get_stats(g, C.byref(st)))
                stats.update(_stats_dict(st))
        finally:
            self._L.gsim_graph_destroy(g)
        return indptr, indices, scores

    def join(self, left, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, order=JOIN_BY_ROW, row_begin=0, row_end=None,
             stats=None):
        """gsim_db_join / gsim_db_join_queries: for every left row, every row j of THIS table with
        score(query = left row, row j) >= cutoff -> CSR (indptr uint64 [nl + 1], indices uint32 (+ row base), scores float32).
        `left`: a Table on the same device (its rows [row_begin, row_end)) or a (nq, W) / (W,) uint32 array.
        `order`: JOIN_BY_ROW (each list by table row) or JOIN_BY_SCORE (search's order: score descending, row ascending).
        `stats`: a dict that receives the call's gsim_join_stats."""
        g = C.c_void_p()
        if isinstance(left, Table):
            if row_end is None:
                row_end = left.count()
            check(self._L.gsim_db_join(self._h, left._h, row_begin, row_end, cutoff, metric, alpha, beta, order, C.byref(g)))
        else:
            q = np.ascontiguousarray(left, dtype=np.uint32).reshape(-1, self.W)
            if row_end is None:
                row_end = q.shape[0]
            q = np.ascontiguousarray(q[row_begin:row_end])
            check(self._L.gsim_db_join_queries(self._h, _u32(q) if len(q) else None, len(q), cutoff, metric, alpha, beta, order,
                                               C.byref(g)))
        return self._take_graph(g, stats, GsimJoinStats, self._L.gsim_graph_get_join_stats)

    def histogram(self, left, edges, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, row_begin=0, row_end=None, exclude_self=False,
                  per_row=True, total=True, stats=None):
        """gsim_db_histogram / gsim_db_histogram_queries: for every left row, the number of rows j of THIS table in each bin of
        score(query = left row, row j), bin(s) = the number of `edges` e with s >= e -> (hist uint64 [nl, len(edges) + 1] or None,
        total uint64 [len(edges) + 1] or None).  `left`: a Table on the same device (its rows [row_begin, row_end)) or a (nq, W) /
        (W,) uint32 array.  `exclude_self` (only with left being this table): the pair (row i, row i) is not counted.
        `per_row` / `total`: which of the two outputs to make.  `stats`: a dict that receives the call's gsim_hist_stats."""
        e = np.ascontiguousarray(edges, dtype=np.float32).reshape(-1)
        nb = len(e) + 1
        ep = e.ctypes.data_as(C.POINTER(C.c_float)) if len(e) else None
        u64p = C.POINTER(C.c_uint64)
        st = GsimHistStats()
        if isinstance(left, Table):
            if row_end is None:
                row_end = left.count()
            nl = max(row_end - row_begin, 0)
        else:
            q = np.ascontiguousarray(left, dtype=np.uint32).reshape(-1, self.W)
            if row_end is None:
                row_end = q.shape[0]
            q = np.ascontiguousarray(q[row_begin:row_end])
            nl = len(q)
        hist = np.zeros((nl, nb), dtype=np.uint64) if per_row else None
        tot = np.zeros(nb, dtype=np.uint64) if total else None
        hp = hist.ctypes.data_as(u64p) if per_row else None
        tp = tot.ctypes.data_as(u64p) if total else None
        if isinstance(left, Table):
            check(self._L.gsim_db_histogram(self._h, left._h, row_begin, row_end, ep, len(e), metric, alpha, beta,
                                            HIST_EXCLUDE_SELF if exclude_self else 0, hp, tp, C.byref(st)))
        else:
            if exclude_self:
                raise GsimError(-1, "exclude_self needs the table itself as the left side")
            check(self._L.gsim_db_histogram_queries(self._h, _u32(q) if nl else None, nl, ep, len(e), metric, alpha, beta, hp, tp,
                                                    C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        return hist, tot

    def scores(self, left, row_begin=0, row_end=None, col_begin=0, col_end=None, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0,
               out_ptr=None, ld=None, stats=None):
        """gsim_db_scores / gsim_db_scores_queries / gsim_db_scores_device: the dense matrix S[i, j] = score(query = left row
        row_begin + i, row col_begin + j of THIS table) -> float32 [nl, nr].  `left`: a Table on the same device (its rows
        [row_begin, row_end)) or a (nq, W) / (W,) uint32 array.  `out_ptr`: a device address on this table's device (a torch
        tensor's data_ptr()) -- the matrix is written there, row i at out_ptr + i * ld * 4 (`ld` floats per row, default nr; only
        the first nr of a row are written), nothing is copied to the host and None is returned; `left` must then be a Table.
        `stats`: a dict that receives the call's gsim_scores_stats."""
        if col_end is None:
            col_end = self.count()
        nr = max(col_end - col_begin, 0)
        st = GsimScoresStats()
        fp = C.POINTER(C.c_float)
        out = None
        if out_ptr is not None:
            if not isinstance(left, Table):
                raise GsimError(-1, "out_ptr needs a Table as the left side")
            if row_end is None:
                row_end = left.count()
            check(self._L.gsim_db_scores_device(self._h, left._h, row_begin, row_end, col_begin, col_end, metric, alpha, beta,
                                                C.c_void_p(out_ptr), nr if ld is None else ld, C.byref(st)))
        elif ld is not None:
            raise GsimError(-1, "ld goes with out_ptr: the returned array has nr floats per row")
        elif isinstance(left, Table):
            if row_end is None:
                row_end = left.count()
            out = np.empty((max(row_end - row_begin, 0), nr), dtype=np.float32)
            check(self._L.gsim_db_scores(self._h, left._h, row_begin, row_end, col_begin, col_end, metric, alpha, beta,
                                         out.ctypes.data_as(fp), nr, C.byref(st)))
        else:
            q = np.ascontiguousarray(left, dtype=np.uint32).reshape(-1, self.W)
            if row_end is None:
                row_end = q.shape[0]
            q = np.ascontiguousarray(q[row_begin:row_end])
            out = np.empty((len(q), nr), dtype=np.float32)
            check(self._L.gsim_db_scores_queries(self._h, _u32(q) if len(q) else None, len(q), col_begin, col_end, metric, alpha, beta,
                                                 out.ctypes.data_as(fp), nr, C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        return out

    def maxmin(self, npicks, seeds=(), metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, max_score=1.0, assign=False, stats=None):
        """gsim_db_maxmin: MaxMin diversity picking, one pass over the table per pick -> (picks uint32 (+ row base),
        pick_scores float32), both of length npicked; assign=True also returns (row_score float32 [N], nearest uint32 [N]).
        `stats`: a dict that receives the call's gsim_maxmin_stats."""
        sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        picks = np.zeros(max(npicks, 1), dtype=np.uint32)
        scores = np.zeros(max(npicks, 1), dtype=np.float32)
        n = C.c_uint32(0)
        fp = C.POINTER(C.c_float)
        row_score = nearest = None
        if assign:
            row_score = np.empty(self.count(), dtype=np.float32)
            nearest = np.empty(self.count(), dtype=np.uint32)
        st = GsimMaxMinStats()
        check(self._L.gsim_db_maxmin(self._h, npicks, _u32(sd) if len(sd) else None, len(sd), metric, alpha, beta, max_score,
                                     _u32(picks), scores.ctypes.data_as(fp), C.byref(n),
                                     row_score.ctypes.data_as(fp) if assign else None, _u32(nearest) if assign else None,
                                     C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        out = (picks[:n.value].copy(), scores[:n.value].copy())
        return out + (row_score, nearest) if assign else out

    def leader(self, cutoff, seeds=(), max_leaders=None, assign=True, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_leader: leader (sphere-exclusion) clustering at `cutoff` -> (leaders uint32 (+ row base), leader_of uint32 [N],
        row_score float32 [N], stats dict); leader_of holds positions in `leaders`, LEADER_NONE for a row left unassigned by the
        cap.  max_leaders=None: no cap.  assign=False: leader_of and row_score are None (nothing but the leaders is copied back)."""
        sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
        n = self.count()
        cap = n if max_leaders is None else int(max_leaders)
        leaders = np.zeros(max(min(cap, n), 1), dtype=np.uint32)
        nl = C.c_uint32(0)
        leader_of = row_score = None
        if assign:
            leader_of = np.empty(n, dtype=np.uint32)
            row_score = np.empty(n, dtype=np.float32)
        st = GsimLeaderStats()
        check(self._L.gsim_db_leader(self._h, cutoff, _u32(sd) if len(sd) else None, len(sd), cap, metric, alpha, beta, _u32(leaders),
                                     C.byref(nl), _u32(leader_of) if assign else None,
                                     row_score.ctypes.data_as(C.POINTER(C.c_float)) if assign else None, C.byref(st)))
        return leaders[:nl.value].copy(), leader_of, row_score, _stats_dict(st)

    def components(self, cutoffs, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, first_row=True, sizes=True):
        """gsim_db_components: single-linkage clustering (connected components of "score >= cutoff") at an ascending list of cutoffs,
        or one scalar cutoff -> (levels, stats dict); levels[l] = (component_of uint32 [N], first_row uint32 [ncomponents] (+ row
        base), sizes uint32 [ncomponents]) for cutoffs[l]; first_row / sizes are None where not asked for."""
        cut = np.ascontiguousarray(np.atleast_1d(cutoffs), dtype=np.float32).reshape(-1)
        n, nl = self.count(), len(cut)
        comp, ncomp, first, size = _level_buffers(n, nl, first_row, sizes)
        st = GsimComponentsStats()
        check(self._L.gsim_db_components(self._h, cut.ctypes.data_as(C.POINTER(C.c_float)), nl, metric, alpha, beta, _u32(comp), _u32(ncomp),
                                         _u32(first) if first_row else None, _u32(size) if sizes else None, C.byref(st)))
        return _levels(nl, comp, ncomp, first, size), _stats_dict(st)

    def snn(self, k, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, closed=False, stats=None):
        """gsim_db_snn: knn(k, cutoff)'s graph of the whole table with the shared-nearest-neighbour count of every entry
        -> (indptr, indices, scores, shared); shared[e] = |L(i) & L(j)| for the entry e = (i, j) (`closed`: the lists count their
        owners), with SNN_MUTUAL_BIT set where i is in list j too.  `stats`: a dict that receives the call's gsim_snn_stats."""
        g = C.c_void_p()
        check(self._L.gsim_db_snn(self._h, k, cutoff, metric, alpha, beta, SNN_CLOSED if closed else 0, C.byref(g)))
        try:
            nnz = C.c_uint64(0)
            check(self._L.gsim_graph_shape(g, None, C.byref(nnz)))
            shared = np.empty(nnz.value, dtype=np.uint32)
            check(self._L.gsim_graph_copy_shared(g, _u32(shared)))
            if stats is not None:
                st = GsimSnnStats()
                check(self._L.gsim_graph_get_snn_stats(g, C.byref(st)))
                stats.update(_snn_stats_dict(st))
        except Exception:
            self._L.gsim_graph_destroy(g)
            raise
        return self._take_graph(g, None, None, None) + (shared,)

    def jarvis_patrick(self, k, kmins, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, closed=False, either=False, first_row=True,
                       sizes=True):
        """gsim_db_jarvis_patrick: Jarvis-Patrick clustering on knn(k, cutoff)'s lists at an ascending list of kmin values, or one
        scalar -> (levels, stats dict); levels[l] = (cluster_of uint32 [N], first_row uint32 [nclusters] (+ row base), sizes uint32
        [nclusters]) for kmins[l], in components()'s numbering; first_row / sizes are None where not asked for.  Two rows link when
        each is in the other's list (`either`: one of them suffices) and the lists share at least kmin rows (`closed`: the lists count
        their owners)."""
        km = np.ascontiguousarray(np.atleast_1d(kmins), dtype=np.uint32).reshape(-1)
        n, nl = self.count(), len(km)
        comp, ncomp, first, size = _level_buffers(n, nl, first_row, sizes)
        flags = (SNN_CLOSED if closed else 0) | (SNN_EITHER if either else 0)
        st = GsimSnnStats()
        check(self._L.gsim_db_jarvis_patrick(self._h, k, _u32(km), nl, cutoff, metric, alpha, beta, flags, _u32(comp), _u32(ncomp),
                                             _u32(first) if first_row else None, _u32(size) if sizes else None, C.byref(st)))
        return _levels(nl, comp, ncomp, first, size), _snn_stats_dict(st)

    def mst(self, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_mst: the single-linkage dendrogram as its maximum-similarity spanning forest -> (edges, stats dict); edges is a
        structured array (MST_EDGE_DTYPE: a < b with the row base added, score) in order E = (score descending, a, b); the per-scan
        arrays of the stats are cut to the scans made."""
        n = self.count()
        edges = np.empty(max(n - 1, 1), dtype=MST_EDGE_DTYPE)
        ne = C.c_uint64(0)
        st = GsimMstStats()
        check(self._L.gsim_db_mst(self._h, cutoff, metric, alpha, beta, edges.ctypes.data, C.byref(ne), C.byref(st)))
        return edges[:ne.value].copy(), _mst_stats_dict(st)

    def dbscan(self, cutoff, min_pts, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, degree=True, anchor=True, first_row=True, sizes=True):
        """gsim_db_dbscan: DBSCAN density clustering -> (label_of uint32 [N] (DBSCAN_NOISE for noise), degree uint32 [N], anchor uint32
        [N] (+ row base; DBSCAN_NOISE for noise), first_row uint32 [nclusters] (+ row base), sizes uint32 [nclusters], stats dict);
        degree / anchor / first_row / sizes are None where not asked for.  A row is a core when degree + 1 >= min_pts; clusters are
        the cores' connected components; a border row joins the cluster of its best-scoring core neighbour (ties: the smallest row)."""
        n = self.count()
        label_of = np.empty(n, dtype=np.uint32)
        ncl = C.c_uint32(0)
        deg = np.empty(n, dtype=np.uint32) if degree else None
        anc = np.empty(n, dtype=np.uint32) if anchor else None
        first = np.empty(max(n, 1), dtype=np.uint32) if first_row else None
        size = np.empty(max(n, 1), dtype=np.uint32) if sizes else None
        st = GsimDbscanStats()
        check(self._L.gsim_db_dbscan(self._h, cutoff, min_pts, metric, alpha, beta, _u32(label_of), C.byref(ncl), _u32(deg) if degree else None,
                                     _u32(anc) if anchor else None, _u32(first) if first_row else None, _u32(size) if sizes else None,
                                     C.byref(st)))
        return (label_of, deg, anc, first[:ncl.value].copy() if first_row else None, size[:ncl.value].copy() if sizes else None,
                _stats_dict(st))

    def core_scores(self, min_pts, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_core_scores: every row's HDBSCAN core score -> (core float32 [N], stats dict: gsim_knn_stats of the core pass).
        core[i] is the score of row i's (min_pts - 1)-th nearest neighbour at or above the cutoff, 0 where it has fewer, 1 for
        min_pts == 1: for t >= cutoff, core[i] >= t iff row i is a core of dbscan(t, min_pts)."""
        core = np.empty(self.count(), dtype=np.float32)
        st = GsimKnnStats()
        check(self._L.gsim_db_core_scores(self._h, min_pts, cutoff, metric, alpha, beta, _f32(core), C.byref(st)))
        return core, _stats_dict(st)

    def mreach_mst(self, min_pts, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_mreach_mst: the mutual-reachability forest -> (edges, core float32 [N], stats dict).  gsim_db_mst's rule with
        m(i, j) = min(score(i, j), core[i], core[j]) in place of the score: edges (MST_EDGE_DTYPE, a < b with the row base added,
        score = m) in order E; the stats are `mst`'s plus the core pass's (core_launches, core_inserts, core_rows, core_kernel_ms,
        core_tail_ms)."""
        n = self.count()
        edges = np.empty(max(n - 1, 1), dtype=MST_EDGE_DTYPE)
        core = np.empty(n, dtype=np.float32)
        ne = C.c_uint64(0)
        st = GsimMreachStats()
        check(self._L.gsim_db_mreach_mst(self._h, min_pts, cutoff, metric, alpha, beta, edges.ctypes.data, C.byref(ne), _f32(core), C.byref(st)))
        return edges[:ne.value].copy(), core, _mreach_stats_dict(st)

    def hdbscan(self, min_pts, min_cluster_size, cutoff, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, flags=HDBSCAN_EOM):
        """gsim_db_hdbscan: HDBSCAN clustering of the table -> (label_of uint32 [N] (HDBSCAN_NOISE for noise; no row base), leave
        float32 [N], first_row uint32 [nclusters] (+ row base), sizes uint32 [nclusters], birth float32 [nclusters], stability
        float64 [nclusters], stats dict).  The mutual-reachability forest at `cutoff`, its condensed tree with similarity as the
        level, and the selection `flags` name: HDBSCAN_EOM or HDBSCAN_LEAF, either with HDBSCAN_NO_ROOTS."""
        n = self.count()
        out = _hdbscan_buffers(n)
        ncl = C.c_uint64(0)
        st = GsimHdbscanStats()
        check(self._L.gsim_db_hdbscan(self._h, min_pts, min_cluster_size, cutoff, metric, alpha, beta, flags, _u32(out[0]), C.byref(ncl),
                                      _f32(out[1]), _u32(out[2]), _u32(out[3]), _f32(out[4]), out[5].ctypes.data_as(C.POINTER(C.c_double)),
                                      C.byref(st)))
        stats = _mreach_stats_dict(st.forest)
        stats.update({f: getattr(st, f) for f, _ in GsimHdbscanStats._fields_[1:]})
        return tuple(out[:2]) + tuple(x[:ncl.value].copy() for x in out[2:]) + (stats,)

    def bit_counts(self, rowset=None, row_begin=0, row_end=None, stats=None):
        """gsim_db_bit_counts: how many of the counted rows have each bit set -> (counts uint64 [fp_bits], counted int).  The counted
        rows are the rows of [row_begin, row_end) (indices without the row base) that are in `rowset` (a :class:`RowSet` of this
        table), or all of them.  Bit k is bit k % 32 of word k // 32.  `stats`: a dict that receives the call's gsim_profile_stats."""
        if row_end is None:
            row_end = self.count()
        counts = np.zeros(self.fp_bits, dtype=np.uint64)
        counted = C.c_uint64(0)
        st = GsimProfileStats()
        check(self._L.gsim_db_bit_counts(self._h, rowset._h if rowset is not None else None, row_begin, row_end,
                                         counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(counted), C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        return counts, counted.value

    def overlap_sums(self, weights, row_begin=0, row_end=None, popc=False, stats=None):
        """gsim_db_overlap_sums: for every row of [row_begin, row_end) the sum of weights[k] over its set bits k -> sums uint64
        [row_end - row_begin], or (sums, popc uint32) with popc=True.  `weights`: fp_bits non-negative integers below 2^32 -- the
        counts of :meth:`bit_counts` as they are; anything larger is refused.  `stats`: as :meth:`bit_counts`."""
        if row_end is None:
            row_end = self.count()
        w = _weights32(weights, self.fp_bits)
        n = max(row_end - row_begin, 0)
        sums = np.zeros(max(n, 1), dtype=np.uint64)
        pc = np.zeros(max(n, 1), dtype=np.uint32) if popc else None
        st = GsimProfileStats()
        check(self._L.gsim_db_overlap_sums(self._h, _u32(w), row_begin, row_end, sums.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           _u32(pc) if popc else None, C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        return (sums[:n], pc[:n]) if popc else sums[:n]

    def _centres(self, centres):
        c = np.ascontiguousarray(centres, dtype=np.uint32).reshape(-1, self.fp_bits // 32)
        return c, (_u32(c) if len(c) else None)

    def assign(self, centres, row_begin=0, row_end=None, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, stats=None):
        """gsim_db_assign: for every row of [row_begin, row_end) the nearest of the m `centres` (m x fp_bits / 32 uint32 words) ->
        (label uint32, score float32), both of length row_end - row_begin.  label[i] is the centre of the greatest f32
        score(query = centre, row i), the lowest index among equal scores; an all-zero row gets (0, 0.0).  `stats`: a dict that
        receives the call's gsim_assign_stats."""
        if row_end is None:
            row_end = self.count()
        c, cp = self._centres(centres)
        n = max(row_end - row_begin, 0)
        label = np.zeros(max(n, 1), dtype=np.uint32)
        score = np.zeros(max(n, 1), dtype=np.float32)
        st = GsimAssignStats()
        check(self._L.gsim_db_assign(self._h, cp, len(c), row_begin, row_end, metric, alpha, beta, _u32(label),
                                     score.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        return label[:n], score[:n]

    def label_counts(self, labels, nlabels, row_begin=0, row_end=None, stats=None):
        """gsim_db_label_counts: the column counts of every label in one pass -> (counts uint32 [nlabels, fp_bits], sizes uint32
        [nlabels]).  labels[i] is the label of row row_begin + i: below `nlabels`, or LABEL_NONE for a row that is counted nowhere
        (the outputs of :meth:`leader`, :meth:`maxmin` with assign=True and :func:`butina` go in as they are).  Row l of counts is
        :meth:`bit_counts` over the rows with label l; widen it to uint64 for :func:`isim`.  `stats`: a dict that receives the
        call's gsim_label_stats."""
        if row_end is None:
            row_end = self.count()
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        if len(lab) != max(row_end - row_begin, 0):
            raise GsimError(-1, "labels: %d entries for %d rows" % (len(lab), row_end - row_begin))
        counts = np.zeros((max(int(nlabels), 1), self.fp_bits), dtype=np.uint32)
        sizes = np.zeros(max(int(nlabels), 1), dtype=np.uint32)
        st = GsimLabelStats()
        check(self._L.gsim_db_label_counts(self._h, _u32(lab) if len(lab) else None, nlabels, row_begin, row_end, _u32(counts), _u32(sizes),
                                           C.byref(st)))
        if stats is not None:
            stats.update(_stats_dict(st))
        return counts, sizes

    def label_sums(self, labels, nlabels, row_begin=0, row_end=None, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, own_only=False, launch_pairs=0):
        """gsim_db_label_sums: the quantised score sums of every row of [row_begin, row_end) by label -> (own_q uint64, other_label
        uint32, other_q uint64, sizes uint32 [nlabels], stats dict); other_label and other_q are None with own_only=True (the medoid
        route: only the pairs inside a cluster are scored).  q = floor(score * 2^31) per ordered pair, so every sum is an integer;
        own_q[i] sums row i's scores against the other rows of its label, other_label[i] is the other label of the greatest mean
        (exact fractions, the lowest label among equals) and other_q[i] its sum.  A LABEL_NONE row gets (0, LABEL_NONE, 0).
        :func:`label_silhouette` and :func:`label_medoids` take the output as it is."""
        if row_end is None:
            row_end = self.count()
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        n = max(row_end - row_begin, 0)
        if len(lab) != n:
            raise GsimError(-1, "labels: %d entries for %d rows" % (len(lab), row_end - row_begin))
        u64p = C.POINTER(C.c_uint64)
        own = np.zeros(max(n, 1), dtype=np.uint64)
        other = None if own_only else np.full(max(n, 1), LABEL_NONE, dtype=np.uint32)
        other_q = None if own_only else np.zeros(max(n, 1), dtype=np.uint64)
        sizes = np.zeros(max(int(nlabels), 1), dtype=np.uint32)
        st = GsimLabelSumsStats()
        check(self._L.gsim_db_label_sums(self._h, _u32(lab) if len(lab) else None, nlabels, row_begin, row_end, metric, alpha, beta,
                                         LABEL_SUMS_OWN_ONLY if own_only else 0, int(launch_pairs), own.ctypes.data_as(u64p),
                                         None if own_only else _u32(other), None if own_only else other_q.ctypes.data_as(u64p), _u32(sizes),
                                         C.byref(st)))
        stats = _stats_dict(st)
        return own[:n], (None if own_only else other[:n]), (None if own_only else other_q[:n]), sizes[:int(nlabels)], stats

    def linkage(self, linkage, row_begin=0, row_end=None, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, launch_steps=0):
        """gsim_db_linkage: the complete-linkage (LINKAGE_COMPLETE) or average-linkage (LINKAGE_AVERAGE) dendrogram of the rows
        [row_begin, row_end), at most LINKAGE_MAX_ROWS of them -> (merges, stats dict); merges is a structured array
        (LINKAGE_MERGE_DTYPE) of n - 1 entries in the order of execution: a < b the smallest rows of the two clusters (row_begin
        and the row base added), left / right in scipy's numbering within the range, size, score (complete: the minimum; average:
        the mean of the quantised scores) and sum_q (the exact sum of q = floor(score * 2^31) over the pairs between the two).
        :func:`linkage_edges` makes them :func:`mst_cut`'s input, :func:`linkage_to_scipy` scipy's Z matrix."""
        if row_end is None:
            row_end = self.count()
        n = max(row_end - row_begin, 0)
        merges = np.zeros(max(n - 1, 1), dtype=LINKAGE_MERGE_DTYPE)
        nm = C.c_uint64(0)
        st = GsimLinkageStats()
        check(self._L.gsim_db_linkage(self._h, row_begin, row_end, linkage, metric, alpha, beta, int(launch_steps), merges.ctypes.data,
                                      C.byref(nm), C.byref(st)))
        return merges[:nm.value].copy(), _stats_dict(st)

    def kmeans(self, init, max_iter=20, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_kmeans: Lloyd's iteration from the m centres `init` over the whole table -- assign, count, majority-vote centroid,
        until the labels repeat or `max_iter` assignments were made -> (centres uint32 [m, words], label uint32 [N], score float32
        [N], sizes uint32 [m], stats dict).  The centres returned are the ones the labels were assigned to:
        ``assign(centres)`` reproduces label and score; an empty cluster keeps its centre."""
        c, cp = self._centres(init)
        n = self.count()
        centres = np.zeros_like(c)
        label = np.zeros(max(n, 1), dtype=np.uint32)
        score = np.zeros(max(n, 1), dtype=np.float32)
        sizes = np.zeros(max(len(c), 1), dtype=np.uint32)
        st = GsimKmeansStats()
        check(self._L.gsim_db_kmeans(self._h, cp, len(c), max_iter, metric, alpha, beta, _u32(centres) if len(c) else None, _u32(label),
                                     score.ctypes.data_as(C.POINTER(C.c_float)), _u32(sizes), C.byref(st)))
        return centres, label[:n], score[:n], sizes[:len(c)], _stats_dict(st)

    def rowset(self, rows=None, bitmap=None, exclude=False) -> RowSet:
        """gsim_rowset_from_rows / _from_bitmap: `rows` are row indices including the row base (gsim_hit.row values), any order,
        duplicates collapse; `bitmap` is (count + 31) // 32 uint32 words, bit r % 32 of word r // 32 selecting row r without the
        row base.  exclude=True: every row of the table except those."""
        if (rows is None) == (bitmap is None):
            raise ValueError("give either rows or bitmap")
        h = C.c_void_p()
        flags = 1 if exclude else 0
        if bitmap is not None:
            b = np.ascontiguousarray(bitmap, dtype=np.uint32).reshape(-1)
            if len(b) < (self.count() + 31) // 32:
                raise ValueError("bitmap needs (count + 31) // 32 words")
            check(self._L.gsim_rowset_from_bitmap(self._h, _u32(b), flags, C.byref(h)))
        else:
            r = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
            check(self._L.gsim_rowset_from_rows(self._h, _u32(r) if len(r) else None, len(r), flags, C.byref(h)))
        return RowSet(self, h)

    def search_rows(self, rowset, queries, k, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, stats=False):
        """gsim_db_search_rows: the top k of the rows in `rowset` -> what :meth:`search` returns (list of HIT_DTYPE arrays, approx);
        with stats=True a third item, the call's gsim_rowset_stats as a dict."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        nq = q.shape[0]
        hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
        counts = np.zeros(nq, dtype=np.uint32)
        approx = np.zeros(nq, dtype=np.uint64)
        st = GsimRowsetStats()
        check(self._L.gsim_db_search_rows(self._h, rowset._h, _u32(q), nq, k, cutoff, metric, alpha, beta,
                                          hits.ctypes.data_as(C.c_void_p), _u32(counts),
                                          approx.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st)))
        out = [hits[i, :counts[i]].copy() for i in range(nq)], approx
        if stats:
            out += (_stats_dict(st),)
        return out

    def popindex(self, rows=False) -> PopIndex:
        """gsim_popindex_create: the popcount index of this table; rows=True (GSIM_POPINDEX_ROWS) also keeps a popcount-ordered copy
        of the rows, so that windows stream instead of gathering."""
        flags = POPINDEX_ROWS if rows else 0
        h = C.c_void_p()
        check(self._L.gsim_popindex_create(self._h, flags, C.byref(h)))
        return PopIndex(self, h, flags)

    def search_bounded(self, popindex, queries, k, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, approx=True, stats=False):
        """gsim_db_search_bounded: what :meth:`search` returns (list of HIT_DTYPE arrays, approx), read from a window of the popcount
        order; approx=False passes NULL for it (None is returned in its place), which lets a query with a cutoff narrow to its top
        k; with stats=True a third item, the call's gsim_popindex_stats as a dict."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        nq = q.shape[0]
        hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
        counts = np.zeros(nq, dtype=np.uint32)
        ap = np.zeros(nq, dtype=np.uint64) if approx else None
        st = GsimPopindexStats()
        check(self._L.gsim_db_search_bounded(self._h, popindex._h, _u32(q), nq, k, cutoff, metric, alpha, beta,
                                             hits.ctypes.data_as(C.c_void_p), _u32(counts),
                                             ap.ctypes.data_as(C.POINTER(C.c_uint64)) if approx else None, C.byref(st)))
        out = [hits[i, :counts[i]].copy() for i in range(nq)], ap
        if stats:
            out += (_stats_dict(st),)
        return out

    def rowhash(self) -> RowHash:
        """gsim_rowhash_create: the hash table over this table's rows (duplicate groups, exact-row lookup)."""
        h = C.c_void_p()
        check(self._L.gsim_rowhash_create(self._h, 0, C.byref(h)))
        return RowHash(self, h)

    def labelset(self, labels, nlabels) -> LabelSet:
        """gsim_labelset_create: labels[r] is the label of table row r (without the row base): below `nlabels`, or LABEL_NONE for a
        row that belongs nowhere -- the outputs of :meth:`leader`, :meth:`dbscan`, :meth:`hdbscan`, :meth:`kmeans`, :meth:`maxmin`
        with assign=True and :func:`butina` go in as they are."""
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        if len(lab) != self.count():
            raise GsimError(-1, "labels: %d entries for %d rows" % (len(lab), self.count()))
        h = C.c_void_p()
        check(self._L.gsim_labelset_create(self._h, _u32(lab) if len(lab) else None, nlabels, C.byref(h)))
        return LabelSet(self, h, nlabels)

    def search_labels(self, labelset, queries, k, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, launch_rows=0, per_label=False,
                      stats=False):
        """gsim_db_search_labels: per query the best kept row of every label, best labels first -> a dict of arrays:
        ``hits`` (HIT_DTYPE [nq, max(k, 1)]), ``hit_labels`` (uint32, the same shape), ``counts`` (uint32 [nq]: the valid entries of
        both), ``approx`` (uint64 [nq]: labels with a kept row), ``rows_kept`` (uint64 [nq]); with per_label=True also ``label_best``
        (HIT_DTYPE [nq, nlabels]; row 0xFFFFFFFF for a label without a kept row) and ``label_kept`` (uint32 [nq, nlabels]); with
        stats=True ``stats``, the call's gsim_label_search_stats as a dict."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        nq = q.shape[0]
        u64p = C.POINTER(C.c_uint64)
        out = {"hits": np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE), "hit_labels": np.zeros((nq, max(k, 1)), dtype=np.uint32),
               "counts": np.zeros(nq, dtype=np.uint32), "approx": np.zeros(nq, dtype=np.uint64), "rows_kept": np.zeros(nq, dtype=np.uint64)}
        if per_label:
            out["label_best"] = np.zeros((nq, labelset.nlabels), dtype=HIT_DTYPE)
            out["label_kept"] = np.zeros((nq, labelset.nlabels), dtype=np.uint32)
        st = GsimLabelSearchStats()
        check(self._L.gsim_db_search_labels(self._h, labelset._h, _u32(q) if nq else None, nq, k, cutoff, metric, alpha, beta, int(launch_rows),
                                            out["hits"].ctypes.data_as(C.c_void_p), _u32(out["hit_labels"]), _u32(out["counts"]),
                                            out["approx"].ctypes.data_as(u64p), out["rows_kept"].ctypes.data_as(u64p),
                                            out["label_best"].ctypes.data_as(C.c_void_p) if per_label else None,
                                            _u32(out["label_kept"]) if per_label else None, C.byref(st)))
        if stats:
            out["stats"] = _stats_dict(st)
        return out

    def search_group(self, queries, k, mode=GROUP_MAX, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0, stats=False):
        """gsim_db_search_group: the top k rows by the MAX, MIN or MEAN of their scores against the set `queries` ->
        (GROUP_HIT_DTYPE array, approx); with stats=True a third item, the call's gsim_group_stats as a dict."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        hits = np.zeros(max(k, 1), dtype=GROUP_HIT_DTYPE)
        count = C.c_uint32(0)
        approx = C.c_uint64(0)
        st = GsimGroupStats()
        check(self._L.gsim_db_search_group(self._h, _u32(q), q.shape[0], mode, k, cutoff, metric, alpha, beta,
                                           hits.ctypes.data_as(C.c_void_p), C.byref(count), C.byref(approx), C.byref(st)))
        out = hits[:count.value].copy(), approx.value
        if stats:
            out += (_stats_dict(st),)
        return out

    def make_search_buffers(self, nq, k):
        """Preallocated outputs for :meth:`search_into` (latency-sensitive callers)."""
        return (np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE), np.zeros(nq, dtype=np.uint32),
                np.zeros(nq, dtype=np.uint64))

    def search_into(self, queries, k, bufs, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_search into caller-owned buffers; queries must be a C-contiguous uint32 array."""
        hits, counts, approx = bufs
        check(self._L.gsim_db_search(self._h, _u32(queries), hits.shape[0], k, cutoff, metric, alpha, beta,
                                     hits.ctypes.data_as(C.c_void_p), _u32(counts),
                                     approx.ctypes.data_as(C.POINTER(C.c_uint64))))

    def search_each_into(self, queries, k, bufs, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """gsim_db_search_each into caller-owned buffers: the queries one after the other through the single-query path."""
        hits, counts, approx = bufs
        check(self._L.gsim_db_search_each(self._h, _u32(queries), hits.shape[0], k, cutoff, metric, alpha, beta,
                                          hits.ctypes.data_as(C.c_void_p), _u32(counts),
                                          approx.ctypes.data_as(C.POINTER(C.c_uint64))))

    def search_timed_into(self, queries, k, bufs, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0) -> np.ndarray:
        """gsim_db_search_timed: the queries one at a time, nothing enqueued ahead; -> seconds per query (measured in the library)."""
        hits, counts, approx = bufs
        sec = np.zeros(hits.shape[0], dtype=np.float64)
        check(self._L.gsim_db_search_timed(self._h, _u32(queries), hits.shape[0], k, cutoff, metric, alpha, beta,
                                           hits.ctypes.data_as(C.c_void_p), _u32(counts),
                                           approx.ctypes.data_as(C.POINTER(C.c_uint64)), sec.ctypes.data_as(C.POINTER(C.c_double))))
        return sec

    def search_cpu(self, queries, k, cutoff=0.0):
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        nq = q.shape[0]
        hits = np.zeros((nq, max(k, 1)), dtype=HIT_DTYPE)
        counts = np.zeros(nq, dtype=np.uint32)
        check(self._L.gsim_db_search_cpu(self._h, _u32(q), nq, k, cutoff, hits.ctypes.data_as(C.c_void_p),
                                         _u32(counts)))
        return [hits[i, :counts[i]].copy() for i in range(nq)]

    def set_stream(self, stream_ptr: int):
        check(self._L.gsim_db_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_row_base(self, base: int):
        check(self._L.gsim_db_set_row_base(self._h, base))

    def search_device(self, query, k, d_result_ptr, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        q = np.ascontiguousarray(query, dtype=np.uint32).reshape(self.W)
        check(self._L.gsim_db_search_device(self._h, _u32(q), k, cutoff, metric, alpha, beta,
                                            C.c_void_p(d_result_ptr)))

    def search_batch_device(self, queries, k, d_results_ptr, cutoff=0.0, metric=METRIC_TANIMOTO, alpha=1.0, beta=1.0):
        """nq queries; result block q lands at d_results_ptr + q * result_block_bytes(k) (device)."""
        q = np.ascontiguousarray(queries, dtype=np.uint32).reshape(-1, self.W)
        check(self._L.gsim_db_search_batch_device(self._h, _u32(q), len(q), k, cutoff, metric, alpha, beta,
                                                  C.c_void_p(d_results_ptr)))

    def set_comm(self, comm):
        """Route multi-shard searches through `comm` (a :class:`Comm`; None: back to the host merge)."""
        check(self._L.gsim_db_set_comm(self._h, comm._h if comm is not None else None))
        self._comm = comm  # (keeps it alive)

    def set_comm_root(self, shard: int):
        """The shard whose device merges the gathered blocks (every device holds them all after the all-gather)."""
        check(self._L.gsim_db_set_comm_root(self._h, shard))

    def enable_timing(self, enable=True):
        check(self._L.gsim_db_enable_timing(self._h, 1 if enable else 0))

    def timing(self) -> dict:
        t = GsimTiming()
        check(self._L.gsim_db_get_timing(self._h, C.byref(t)))
        return _stats_dict(t)

    def query_flags(self, n: int) -> np.ndarray:
        """One byte per query of the last search call made with timing enabled (gsim_debug_query_flags): 1 handed back by its own
        single launch, 2 re-run behind a launch that did not close, 4 torn block, 8 routed around the single launch by the
        back-off, 16 / 32 the same two for the large-k publishing route."""
        out = np.zeros(n, dtype=np.uint8)
        w = C.c_uint32(0)
        check(self._L.gsim_debug_query_flags(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(w)))
        return out[:w.value]


def butina(indptr, indices):
    """gsim_butina (host code): Taylor-Butina clustering of a symmetric CSR graph -> (cluster_of uint32 [n],
    centroids uint32 [nclusters]); cluster ids follow creation order (include/gpusim_hip.h states the rule)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    n = len(indptr) - 1
    if n < 0:
        raise GsimError(-1, "indptr needs at least one entry")
    cluster_of = np.empty(n, dtype=np.uint32)
    centroids = np.empty(max(n, 1), dtype=np.uint32)
    nc = C.c_uint64(0)
    check(load().gsim_butina(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), n, _u32(cluster_of),
                             _u32(centroids), C.byref(nc)))
    return cluster_of, centroids[:nc.value].copy()


def components(indptr, indices, nrows=None):
    """gsim_components (host code): the connected components of a symmetric CSR graph -> (component_of uint32 [n],
    first_row uint32 [ncomponents], sizes uint32 [ncomponents]); components are numbered in ascending order of their smallest row
    (include/gpusim_hip.h states the rule)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    n = len(indptr) - 1 if nrows is None else int(nrows)
    if n < 0 or len(indptr) < n + 1:
        raise GsimError(-1, "indptr needs nrows + 1 entries")
    component_of = np.empty(n, dtype=np.uint32)
    first_row = np.empty(max(n, 1), dtype=np.uint32)
    sizes = np.empty(max(n, 1), dtype=np.uint32)
    nc = C.c_uint64(0)
    check(load().gsim_components(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), n, _u32(component_of), _u32(first_row),
                                 _u32(sizes), C.byref(nc)))
    return component_of, first_row[:nc.value].copy(), sizes[:nc.value].copy()


def snn(indptr, indices, nrows=None, closed=False):
    """gsim_snn (host code): the shared-nearest-neighbour count of every entry of a CSR of lists (any lengths, any order) -> shared
    uint32 [nnz]; shared[e] = |L(i) & L(j)| for e = (i, j) (`closed`: + [j in L(i)] + [i in L(j)]), with SNN_MUTUAL_BIT set where i is
    in list j (include/gpusim_hip.h states the rule)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    n = len(indptr) - 1 if nrows is None else int(nrows)
    if n < 0 or len(indptr) < n + 1:
        raise GsimError(-1, "indptr needs nrows + 1 entries")
    shared = np.empty(int(indptr[n]), dtype=np.uint32)
    check(load().gsim_snn(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), n, SNN_CLOSED if closed else 0, _u32(shared)))
    return shared


def jarvis_patrick(indptr, indices, kmins, nrows=None, closed=False, either=False):
    """gsim_jarvis_patrick (host code): Jarvis-Patrick clustering of a CSR of lists at an ascending list of kmin values, or one
    scalar -> levels; levels[l] = (cluster_of uint32 [n], first_row uint32 [nclusters], sizes uint32 [nclusters]), clusters numbered
    in ascending order of their smallest row (include/gpusim_hip.h states the rule)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    km = np.ascontiguousarray(np.atleast_1d(kmins), dtype=np.uint32).reshape(-1)
    n = len(indptr) - 1 if nrows is None else int(nrows)
    if n < 0 or len(indptr) < n + 1:
        raise GsimError(-1, "indptr needs nrows + 1 entries")
    nl = len(km)
    comp, nc, first, size = _level_buffers(n, nl)
    flags = (SNN_CLOSED if closed else 0) | (SNN_EITHER if either else 0)
    check(load().gsim_jarvis_patrick(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), n, _u32(km), nl, flags, _u32(comp),
                                     _u32(first), _u32(size), _u32(nc)))
    return _levels(nl, comp, nc, first, size)


def _mst_edges(edges):
    edges = np.ascontiguousarray(edges, dtype=MST_EDGE_DTYPE).reshape(-1)
    return edges, (edges.ctypes.data if len(edges) else None)


def mst(indptr, indices, scores, nrows=None):
    """gsim_mst (host code): the rule of gsim_db_mst on a symmetric scored CSR graph (Table.neighbors' output) -> edges
    (MST_EDGE_DTYPE, rows without any row base) in order E."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n = len(indptr) - 1 if nrows is None else int(nrows)
    if n < 0 or len(indptr) < n + 1 or len(scores) != len(indices):
        raise GsimError(-1, "indptr needs nrows + 1 entries, scores one per index")
    edges = np.empty(max(n - 1, 1), dtype=MST_EDGE_DTYPE)
    ne = C.c_uint64(0)
    check(load().gsim_mst(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), scores.ctypes.data_as(C.POINTER(C.c_float)), n,
                          edges.ctypes.data, C.byref(ne)))
    return edges[:ne.value].copy()


def dbscan(indptr, indices, scores, min_pts, nrows=None):
    """gsim_dbscan (host code): the rule of gsim_db_dbscan on a symmetric scored CSR graph (Table.neighbors' output) -> (label_of uint32
    [n], anchor uint32 [n], first_row uint32 [nclusters], sizes uint32 [nclusters]); rows without any row base, DBSCAN_NOISE for noise."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n = len(indptr) - 1 if nrows is None else int(nrows)
    if n < 0 or len(indptr) < n + 1 or len(scores) != len(indices):
        raise GsimError(-1, "indptr needs nrows + 1 entries, scores one per index")
    label_of = np.empty(n, dtype=np.uint32)
    anchor = np.empty(n, dtype=np.uint32)
    first_row = np.empty(max(n, 1), dtype=np.uint32)
    sizes = np.empty(max(n, 1), dtype=np.uint32)
    nc = C.c_uint64(0)
    check(load().gsim_dbscan(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), scores.ctypes.data_as(C.POINTER(C.c_float)), n,
                             min_pts, _u32(label_of), _u32(anchor), _u32(first_row), _u32(sizes), C.byref(nc)))
    return label_of, anchor, first_row[:nc.value].copy(), sizes[:nc.value].copy()


def mst_linkage(edges, nrows):
    """gsim_mst_linkage (host code): the dendrogram of a forest in order E (rows without any row base) -> merges (MST_MERGE_DTYPE), one
    per edge; a row is cluster `row`, merge m creates cluster nrows + m, `left` holds the smaller smallest row."""
    edges, ptr = _mst_edges(edges)
    merges = np.empty(max(len(edges), 1), dtype=MST_MERGE_DTYPE)
    check(load().gsim_mst_linkage(ptr, len(edges), int(nrows), merges.ctypes.data))
    return merges[:len(edges)].copy()


def mst_cut(edges, nrows, t):
    """gsim_mst_cut (host code): the components of the edges with score >= t -> (component_of uint32 [n], first_row uint32
    [ncomponents], sizes uint32 [ncomponents]), as `components`."""
    edges, ptr = _mst_edges(edges)
    n = int(nrows)
    component_of = np.empty(n, dtype=np.uint32)
    first_row = np.empty(max(n, 1), dtype=np.uint32)
    sizes = np.empty(max(n, 1), dtype=np.uint32)
    nc = C.c_uint64(0)
    check(load().gsim_mst_cut(ptr, len(edges), n, t, _u32(component_of), _u32(first_row), _u32(sizes), C.byref(nc)))
    return component_of, first_row[:nc.value].copy(), sizes[:nc.value].copy()


def linkage(scores, kind):
    """gsim_linkage (host code): the rule of gsim_db_linkage on a square float32 matrix of scores in [0, 1], of which only the
    entries i < j are read -> (merges (LINKAGE_MERGE_DTYPE, rows without any offset), the chain's nearest-neighbour scans)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    if s.size == 0:
        s = s.reshape(0, 0)
    if s.ndim != 2 or s.shape[0] != s.shape[1]:
        raise GsimError(-1, "linkage: the scores must be a square matrix")
    n = s.shape[0]
    merges = np.zeros(max(n - 1, 1), dtype=LINKAGE_MERGE_DTYPE)
    nm, scans = C.c_uint64(0), C.c_uint64(0)
    check(load().gsim_linkage(_f32(s) if n else None, n, n, kind, merges.ctypes.data, C.byref(nm), C.byref(scans)))
    return merges[:nm.value].copy(), scans.value


def linkage_edges(merges, offset=0):
    """The merges of :meth:`Table.linkage` / :func:`linkage` as MST_EDGE_DTYPE edges (a - offset, b - offset, score) in their order:
    :func:`mst_cut` of them at t gives the flat clusters at t.  offset: row_begin plus the row base of a device call."""
    m = np.ascontiguousarray(merges, dtype=LINKAGE_MERGE_DTYPE).reshape(-1)
    edges = np.zeros(len(m), dtype=MST_EDGE_DTYPE)
    edges["a"] = m["a"] - np.uint32(offset)
    edges["b"] = m["b"] - np.uint32(offset)
    edges["score"] = m["score"]
    return edges


def linkage_to_scipy(merges, n):
    """The merges as scipy's linkage matrix Z: float64 [n - 1, 4] of (left, right, distance = 1 - score, size)."""
    m = np.ascontiguousarray(merges, dtype=LINKAGE_MERGE_DTYPE).reshape(-1)
    if len(m) != max(int(n) - 1, 0):
        raise GsimError(-1, "linkage: %d merges for %d rows" % (len(m), n))
    z = np.zeros((len(m), 4), dtype=np.float64)
    z[:, 0] = m["left"]
    z[:, 1] = m["right"]
    z[:, 2] = 1.0 - m["score"].astype(np.float64)
    z[:, 3] = m["size"]
    return z


def mreach_mst(indptr, indices, scores, min_pts, nrows=None):
    """gsim_mreach_mst (host code): the rule of gsim_db_mreach_mst on a symmetric scored CSR graph (Table.neighbors' output) ->
    (edges (MST_EDGE_DTYPE, rows without any row base, score = min(score, core, core)) in order E, core float32 [n])."""
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n = len(indptr) - 1 if nrows is None else int(nrows)
    if n < 0 or len(indptr) < n + 1 or len(scores) != len(indices):
        raise GsimError(-1, "indptr needs nrows + 1 entries, scores one per index")
    edges = np.empty(max(n - 1, 1), dtype=MST_EDGE_DTYPE)
    core = np.empty(n, dtype=np.float32)
    ne = C.c_uint64(0)
    check(load().gsim_mreach_mst(indptr.ctypes.data_as(C.POINTER(C.c_uint64)), _u32(indices), _f32(scores), n, min_pts, edges.ctypes.data,
                                 C.byref(ne), _f32(core)))
    return edges[:ne.value].copy(), core


def mst_hdbscan(edges, nrows, floor, min_cluster_size, flags=HDBSCAN_EOM):
    """gsim_mst_hdbscan (host code): the condensed tree of a forest in order E (rows without any row base; Table.mst's or
    Table.mreach_mst's edges) and the selection of its clusters -> (label_of uint32 [n] (HDBSCAN_NOISE for noise), leave float32 [n],
    first_row uint32 [nclusters], sizes uint32 [nclusters], birth float32 [nclusters], stability float64 [nclusters]).  `floor`: the
    cutoff of the call that made the forest."""
    edges, ptr = _mst_edges(edges)
    n = int(nrows)
    out = _hdbscan_buffers(n)
    ncl = C.c_uint64(0)
    check(load().gsim_mst_hdbscan(ptr, len(edges), n, floor, min_cluster_size, flags, _u32(out[0]), C.byref(ncl), _f32(out[1]), _u32(out[2]),
                                  _u32(out[3]), _f32(out[4]), out[5].ctypes.data_as(C.POINTER(C.c_double))))
    return tuple(out[:2]) + tuple(x[:ncl.value].copy() for x in out[2:])


def _weights32(weights, fp_bits):
    w = np.asarray(weights).reshape(-1)
    if len(w) != fp_bits:
        raise GsimError(-1, "weights: %d entries for %d bits" % (len(w), fp_bits))
    if w.dtype.kind not in "ui" or (len(w) and (int(w.min()) < 0 or int(w.max()) > 0xFFFFFFFF)):
        raise GsimError(-1, "weights must be integers in [0, 2^32)")
    return np.ascontiguousarray(w, dtype=np.uint32)


def isim(counts, n, index=ISIM_TANIMOTO) -> float:
    """gsim_isim (host code): the iSIM index of a set of n rows from its column counts (Table.bit_counts' output) -- a ratio of sums
    over all pairs, not the mean of the pairwise scores."""
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    v = C.c_double(0.0)
    check(load().gsim_isim(c.ctypes.data_as(C.POINTER(C.c_uint64)) if len(c) else None, len(c), int(n), index, C.byref(v)))
    return v.value


def isim_complement(counts, n, sums, popc, index=ISIM_TANIMOTO) -> np.ndarray:
    """gsim_isim_complement (host code): for every row i given by sums[i] (Table.overlap_sums with weights = counts) and popc[i], a
    member of the counted set, the index of the n - 1 rows left without it -> float64 array; its argmin is the medoid, its largest
    values are the outliers."""
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    s = np.ascontiguousarray(sums, dtype=np.uint64).reshape(-1)
    p = np.ascontiguousarray(popc, dtype=np.uint32).reshape(-1)
    if len(s) != len(p):
        raise GsimError(-1, "sums and popc differ in length")
    out = np.zeros(len(s), dtype=np.float64)
    u64p = C.POINTER(C.c_uint64)
    check(load().gsim_isim_complement(c.ctypes.data_as(u64p) if len(c) else None, len(c), int(n), index,
                                      s.ctypes.data_as(u64p) if len(s) else None, _u32(p) if len(p) else None, len(s),
                                      out.ctypes.data_as(C.POINTER(C.c_double)) if len(s) else None))
    return out


def label_centroids(counts, sizes, previous=None) -> np.ndarray:
    """gsim_label_centroids (host code): the majority-vote centroids of Table.label_counts' output -> uint32 [nlabels, fp_bits / 32];
    bit k of centre l is set iff 2 * counts[l, k] >= sizes[l].  An empty label keeps its row of `previous`, or is all zeros."""
    c = np.ascontiguousarray(counts, dtype=np.uint32)
    if c.ndim != 2:
        raise GsimError(-1, "counts must be nlabels x fp_bits")
    z = np.ascontiguousarray(sizes, dtype=np.uint32).reshape(-1)
    nlabels, fp_bits = c.shape
    if len(z) != nlabels:
        raise GsimError(-1, "sizes: %d entries for %d labels" % (len(z), nlabels))
    out = np.zeros((nlabels, fp_bits // 32), dtype=np.uint32)
    prev = None
    if previous is not None:
        prev = np.ascontiguousarray(previous, dtype=np.uint32)
        if prev.shape != out.shape:
            raise GsimError(-1, "previous must be nlabels x fp_bits / 32")
    check(load().gsim_label_centroids(_u32(c) if c.size else None, _u32(z) if nlabels else None, nlabels, fp_bits,
                                      _u32(prev) if prev is not None and prev.size else None, _u32(out) if out.size else None))
    return out


def label_silhouette(labels, own_q, other_label, other_q, sizes):
    """gsim_label_silhouette (host code): the silhouette of every row on the distance 1 - score from Table.label_sums' output ->
    (sil float64 [n], label_mean float64 [nlabels], mean float).  a = own_q / (size - 1) * 2^-31, b = other_q / size(other) * 2^-31,
    sil = (a - b) / (1 - min(a, b)), 0.0 where that is 0 / 0, for a singleton, a row without another cluster and a LABEL_NONE row."""
    u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
    lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    own = np.ascontiguousarray(own_q, dtype=np.uint64).reshape(-1)
    oth = np.ascontiguousarray(other_label, dtype=np.uint32).reshape(-1)
    othq = np.ascontiguousarray(other_q, dtype=np.uint64).reshape(-1)
    z = np.ascontiguousarray(sizes, dtype=np.uint32).reshape(-1)
    n = len(lab)
    if not (len(own) == len(oth) == len(othq) == n):
        raise GsimError(-1, "label silhouette: own_q, other_label and other_q need one entry per label")
    sil = np.zeros(max(n, 1), dtype=np.float64)
    lmean = np.zeros(max(len(z), 1), dtype=np.float64)
    mean = C.c_double(0.0)
    check(load().gsim_label_silhouette(_u32(lab) if n else None, own.ctypes.data_as(u64p) if n else None, _u32(oth) if n else None,
                                       othq.ctypes.data_as(u64p) if n else None, _u32(z) if len(z) else None, n, len(z),
                                       sil.ctypes.data_as(f64p), lmean.ctypes.data_as(f64p), C.byref(mean)))
    return sil[:n], lmean[:len(z)], mean.value


def label_medoids(labels, own_q, nlabels) -> np.ndarray:
    """gsim_label_medoids (host code): for every label the row of the greatest own_q (Table.label_sums, own_only=True is enough), the
    lowest row among equals -> uint32 [nlabels]; LABEL_NONE for a label without rows."""
    lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
    own = np.ascontiguousarray(own_q, dtype=np.uint64).reshape(-1)
    if len(own) != len(lab):
        raise GsimError(-1, "label medoids: own_q needs one entry per label")
    out = np.zeros(max(int(nlabels), 1), dtype=np.uint32)
    check(load().gsim_label_medoids(_u32(lab) if len(lab) else None, own.ctypes.data_as(C.POINTER(C.c_uint64)) if len(lab) else None, len(lab),
                                    nlabels, _u32(out)))
    return out[:int(nlabels)]


def litmus(test: int, workgroups: int = 256, iterations: int = 100000, device: int = 0) -> dict:
    """gsim_debug_litmus -> {loads, torn, headers_seen, stale_first_read, never_landed, rereads, timed_out, stores}"""
    st = (C.c_ulonglong * 8)()
    check(load().gsim_debug_litmus(device, test, workgroups, iterations, st))
    return dict(zip(("loads", "torn", "headers_seen", "stale_first_read", "never_landed", "rereads", "timed_out", "stores"), [int(x) for x in st]))


def rccl_info() -> dict:
    """gsim_rccl_info: the RCCL header version the library was built with, the version and file of the librccl.so bound to this process."""
    L = load()
    h, r = C.c_int(0), C.c_int(0)
    buf = C.create_string_buffer(1024)
    check(L.gsim_rccl_info(C.byref(h), C.byref(r), buf, len(buf)))
    return {"header_version": h.value, "runtime_version": r.value, "path": buf.value.decode()}


class Comm:
    """``gsim_comm``: the RCCL communicator of an in-process multi-device handle (ncclCommInitAll)."""

    def __init__(self, devices):
        self._L = load()
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        check(self._L.gsim_comm_create(devs, len(devices), C.byref(h)))
        self._h = h

    def size(self) -> int:
        return int(self._L.gsim_comm_size(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.gsim_comm_destroy(self._h)
            self._h = None


def fold_fingerprint(fp, fold_factor: int) -> np.ndarray:
    fp = np.ascontiguousarray(fp, dtype=np.uint32)
    out = np.zeros(len(fp) // fold_factor, dtype=np.uint32)
    check(load().gsim_fold_fingerprint(_u32(fp), len(fp), fold_factor, _u32(out)))
    return out


def merge_device(device, stream_ptr, d_blocks_ptr, nblocks, block_bytes, k, d_result_ptr):
    check(load().gsim_merge_device(device, C.c_void_p(stream_ptr), C.c_void_p(d_blocks_ptr), nblocks, block_bytes, k,
                                   C.c_void_p(d_result_ptr)))


def merge_device_batch(device, stream_ptr, d_blocks_ptr, nranks, nq, block_bytes, k, d_results_ptr):
    check(load().gsim_merge_device_batch(device, C.c_void_p(stream_ptr), C.c_void_p(d_blocks_ptr), nranks, nq,
                                         block_bytes, k, C.c_void_p(d_results_ptr)))


def merge_host(blocks: bytes, nblocks: int, block_bytes: int, k: int) -> bytes:
    """gsim_merge_host on a bytes object holding nblocks result blocks."""
    src = (C.c_ubyte * len(blocks)).from_buffer_copy(blocks)
    out = (C.c_ubyte * result_block_bytes(k))()
    check(load().gsim_merge_host(C.cast(src, C.c_void_p), nblocks, block_bytes, k, C.cast(out, C.c_void_p)))
    return bytes(out)


def make_result_block(hits: np.ndarray, approx: int, k: int, flags: int = 0) -> bytes:
    """Serialise (hits, approx) as one result block of capacity k."""
    hdr = np.zeros(1, dtype=HEADER_DTYPE)
    hdr["count"], hdr["flags"], hdr["approx"] = len(hits), flags, approx
    body = np.zeros(k, dtype=HIT_DTYPE)
    body[:len(hits)] = hits
    raw = hdr.tobytes() + body.tobytes()
    return raw + b"\0" * (result_block_bytes(k) - len(raw))


def parse_result_block(buf: bytes, k: int):
    """bytes of one result block -> (HIT_DTYPE array, approx, flags)"""
    hdr = np.frombuffer(buf, dtype=HEADER_DTYPE, count=1)[0]
    hits = np.frombuffer(buf, dtype=HIT_DTYPE, count=int(hdr["count"]), offset=HEADER_DTYPE.itemsize)
    return hits.copy(), int(hdr["approx"]), int(hdr["flags"])


def debug_score_table(metric, alpha, beta, a, max_b, max_c, device=0) -> np.ndarray:
    out = np.empty((max_c + 1, max_b + 1), dtype=np.float32)
    check(load().gsim_debug_score_table(device, metric, alpha, beta, a, max_b, max_c,
                                        out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def debug_sort_desc(keys: np.ndarray, device=0) -> np.ndarray:
    """The device sort of the large-k and folded paths (launch_sort_desc) on a uint64 array of 2^i keys, descending."""
    out = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    check(load().gsim_debug_sort_desc(device, out.ctypes.data_as(C.c_void_p), len(out)))
    return out


def debug_prefilter_constants(metric, alpha, beta, max_qa, cutoff=None, device=0) -> np.ndarray:
    """Pre-filter constants of the matrix-core pass, [max_qa+1, 512 (or 1 with a cutoff), 4]; device < 0: host twin."""
    nlev = 1 if cutoff is not None else 512
    out = np.empty((max_qa + 1, nlev, 4), dtype=np.float32)
    check(load().gsim_debug_prefilter_constants(device, metric, alpha, beta, max_qa, 1 if cutoff is not None else 0,
                                                0.0 if cutoff is None else cutoff, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out

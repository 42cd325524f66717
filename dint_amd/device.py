"""ctypes binding of the device decode path (include/dint_hip.h).

torch is used for what it is good at here — owning device memory and streams;
every decode goes through the C ABI into the hand-written HIP kernels. There is
no CPU fallback: if libdint_hip.so is missing the import fails, and a decode
without a GPU fails with DINT_ERR_NO_DEVICE.
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import numpy as np

try:
    # torch ships its own HIP runtime under the same soname as the system one. Whichever is loaded first serves
    # the whole process; with the system's loaded first (by libdint_hip.so), torch later finds "No HIP GPUs".
    # So torch — which owns device memory and streams in this layer anyway — is imported before the library.
    import torch  # noqa: F401
except ImportError:  # (the C ABI itself does not need torch)
    pass

from .host import UNIT_DTYPE, KIND_BY_TYPE, RECTANGULAR, SINGLE_PACKED, MULTI_PACKED  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("DINT_HIP_LIB") or os.path.join(_HERE, "libdint_hip.so")

#: every symbol include/dint_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "dint_abi_version", "dint_set_option", "dint_get_option", "dint_option_name", "dint_reset_options", "dint_strerror", "dint_last_hip_error", "dint_device_count",
    "dint_dict_create", "dint_dict_destroy", "dint_dict_info_get", "dint_index_stream", "dint_free",
    "dint_decode_units", "dint_unit_table_create", "dint_unit_table_destroy", "dint_decode_unit_table", "dint_unit_table_rank_outputs", "dint_probe_placement", "dint_decode_list_host", "dint_last_kernel_ms", "dint_recent_kernel_ms",
    "dint_stream_stats_get",
    "dint_decode_block_host", "dint_index_posting_lists", "dint_decode_posting_blocks",
    "dint_list_cache_create", "dint_list_cache_decode", "dint_list_cache_decode_part", "dint_list_cache_destroy",
    "dint_block_table_create", "dint_block_table_destroy", "dint_block_table_learn", "dint_block_table_ready", "dint_block_table_info_get", "dint_decode_block_table",
    "dint_query_index_create", "dint_query_index_destroy", "dint_and_queries", "dint_and_queries_freqs", "dint_or_queries", "dint_or_queries_freqs",
    "dint_wand_data_create", "dint_wand_data_destroy", "dint_ranked_and_queries", "dint_ranked_bool_queries", "dint_ranked_or_queries",
    "dint_ranked_or_bool_queries", "dint_ranked_or_range_queries", "dint_ranked_and_range_queries",
    "dint_doc_filter_create", "dint_doc_filter_info_get", "dint_doc_filter_destroy", "dint_ranked_or_filtered_queries", "dint_ranked_and_filtered_queries",
    "dint_doc_facets_create", "dint_doc_facets_info_get", "dint_doc_facets_group_sizes", "dint_doc_facets_destroy",
    "dint_ranked_or_faceted_queries", "dint_ranked_and_faceted_queries",
    "dint_ranked_or_collapsed_queries", "dint_ranked_and_collapsed_queries",
    "dint_ranked_or_paged_queries", "dint_ranked_and_paged_queries",
    "dint_ranked_or_collapsed_paged_queries", "dint_ranked_and_collapsed_paged_queries",
    "dint_ranked_or_group_limit_queries", "dint_ranked_and_group_limit_queries",
    "dint_doc_values_create", "dint_doc_values_info_get", "dint_doc_values_destroy", "dint_doc_filter_create_from_values",
    "dint_ranked_or_sorted_queries", "dint_ranked_and_sorted_queries",
    "dint_ranked_or_value_stats_queries", "dint_ranked_and_value_stats_queries",
    "dint_ranked_or_group_stats_queries", "dint_ranked_and_group_stats_queries",
    "dint_ranked_or_percentile_queries", "dint_ranked_and_percentile_queries",
    "dint_ranked_or_top_values_queries", "dint_ranked_and_top_values_queries",
    "dint_wand_data_create_with_max_weights", "dint_ranked_or_maxscore_queries", "dint_score_documents",
    "dint_index_max_weights", "dint_wand_data_set_block_max_weights", "dint_check_index", "dint_count_ngrams", "dint_select_ngrams", "dint_last_kernel_clock_mhz",
)

#: dint_block_ref (include/dint_hip.h)
BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("n", "<u4"), ("base", "<u4"), ("max", "<u4"),
                        ("list", "<u4")], align=False)
assert BLOCK_DTYPE.itemsize == 32


class DictInfo(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("device", C.c_int32), ("num_dicts", C.c_uint32),
        ("entries", C.c_uint32), ("hot_entries", C.c_uint32), ("lds_bytes", C.c_uint32),
        ("table_words", C.c_uint32), ("compute_units", C.c_uint32),
    ]


class BlockTableInfo(C.Structure):  # dint_block_table_info
    _fields_ = [("n_blocks", C.c_uint64), ("n_short_blocks", C.c_uint64)] + [(k, C.c_uint32) for k in (
        "complete_decodes", "spans_exact", "freqs_units_ready", "docs_schedule", "freqs_schedule", "docs_queue_items",
        "freqs_queue_items", "short_block_tickets")]


class StreamStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in (
        "lists", "ints", "payload_bytes", "codewords", "run_codewords", "exceptions16", "exceptions32",
        "hot_codewords", "hot_ints", "wide_blocks", "narrow_blocks")]


class CollectionView(C.Structure):  # dint_collection_view
    _fields_ = [("docs", C.c_void_p), ("freqs", C.c_void_p), ("docs_at", C.c_void_p), ("freqs_at", C.c_void_p),
                ("list_len", C.c_void_p), ("n_lists", C.c_size_t)]


class DocFilterInfo(C.Structure):  # dint_doc_filter_info
    _fields_ = [(k, C.c_uint64) for k in ("num_docs", "n_set", "n_blocks", "live_blocks")]


class DocFacetsInfo(C.Structure):  # dint_doc_facets_info
    _fields_ = [(k, C.c_uint64) for k in ("num_docs", "n_groups", "n_grouped")]


class DocValuesInfo(C.Structure):  # dint_doc_values_info
    _fields_ = [("num_docs", C.c_uint64)]


class IndexMismatch(C.Structure):  # dint_index_mismatch
    _fields_ = [("kind", C.c_uint32), ("list", C.c_uint32), ("position", C.c_uint64), ("expected", C.c_uint64),
                ("got", C.c_uint64)]


#: dint_index_mismatch.kind (DINT_CHECK_*)
CHECK_OK, CHECK_LENGTH, CHECK_DOCID, CHECK_FREQ = 0, 1, 2, 3

#: what QueryIndex.check reports as the first mismatch
Mismatch = collections.namedtuple("Mismatch", "kind list position expected got")


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} is missing — the HIP extension has not been built "
            "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback."
        )
    lib = C.CDLL(_LIB_PATH)
    vp, sz, u32, u64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64
    lib.dint_abi_version.restype = C.c_int
    lib.dint_strerror.restype = C.c_char_p
    lib.dint_strerror.argtypes = [C.c_int]
    lib.dint_set_option.argtypes = [C.c_int, C.c_longlong]
    lib.dint_get_option.argtypes = [C.c_int, C.POINTER(C.c_longlong)]
    lib.dint_option_name.restype = C.c_char_p
    lib.dint_option_name.argtypes = [C.c_int]
    lib.dint_last_hip_error.restype = C.c_char_p
    lib.dint_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.dint_dict_create.argtypes = [C.c_int, vp, sz, C.c_int, C.POINTER(vp)]
    lib.dint_dict_destroy.restype = None
    lib.dint_dict_destroy.argtypes = [vp]
    lib.dint_dict_info_get.argtypes = [vp, C.POINTER(DictInfo)]
    lib.dint_index_stream.argtypes = [vp, vp, sz, u32, C.POINTER(vp), C.POINTER(sz), C.POINTER(u64),
                                      C.POINTER(u64)]
    lib.dint_free.restype = None
    lib.dint_free.argtypes = [vp]
    lib.dint_decode_units.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp]
    lib.dint_unit_table_create.argtypes = [vp, vp, sz, vp, sz, sz, vp, C.POINTER(vp)]
    lib.dint_unit_table_destroy.restype = None
    lib.dint_unit_table_destroy.argtypes = [vp]
    lib.dint_decode_unit_table.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.dint_unit_table_rank_outputs.argtypes = [vp, vp, C.POINTER(vp), sz, sz, vp, C.POINTER(C.c_float), C.POINTER(sz)]
    lib.dint_probe_placement.argtypes = [vp, C.POINTER(vp), sz, sz, vp, sz, C.POINTER(vp), sz, sz, C.c_uint64, vp, C.POINTER(C.c_float)]
    lib.dint_decode_list_host.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz)]
    lib.dint_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.dint_last_kernel_clock_mhz.argtypes = [vp, C.POINTER(C.c_float)]
    lib.dint_recent_kernel_ms.argtypes = [vp, vp, sz, C.POINTER(sz)]
    lib.dint_stream_stats_get.argtypes = [vp, vp, sz, C.POINTER(StreamStats)]
    lib.dint_decode_block_host.argtypes = [vp, vp, sz, vp, u32, sz, C.POINTER(sz)]
    lib.dint_index_posting_lists.argtypes = [vp, sz, vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(u64)]
    lib.dint_list_cache_create.argtypes = [vp, vp, vp, sz, C.POINTER(vp)]
    lib.dint_list_cache_decode.argtypes = [vp, sz, vp, sz, C.POINTER(sz)]
    lib.dint_list_cache_decode_part.argtypes = [vp, sz, u32, vp, sz, C.POINTER(sz)]
    lib.dint_list_cache_destroy.restype = None
    lib.dint_list_cache_destroy.argtypes = [vp]
    lib.dint_debug_alloc_count.argtypes = [C.POINTER(u64)]
    lib.dint_decode_posting_blocks.argtypes = [vp, vp, vp, sz, vp, sz, vp, vp, sz, vp]
    lib.dint_block_table_create.argtypes = [vp, vp, sz, sz, C.POINTER(vp)]
    lib.dint_block_table_destroy.restype = None
    lib.dint_block_table_destroy.argtypes = [vp]
    lib.dint_decode_block_table.argtypes = [vp, vp, vp, sz, vp, vp, vp, sz, vp]
    lib.dint_block_table_learn.argtypes = [vp, vp, vp, vp, sz, vp]
    lib.dint_block_table_ready.argtypes = [vp, C.c_int]
    lib.dint_block_table_info_get.argtypes = [vp, C.POINTER(BlockTableInfo)]
    lib.dint_query_index_create.argtypes = [vp, vp, sz, vp, sz, sz, C.POINTER(vp)]
    lib.dint_query_index_destroy.restype = None
    lib.dint_query_index_destroy.argtypes = [vp]
    lib.dint_and_queries.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.dint_and_queries_freqs.argtypes = [vp, vp, vp, vp, sz, vp, vp, C.POINTER(u64), vp]
    lib.dint_or_queries.argtypes = [vp, vp, vp, sz, vp, vp]
    lib.dint_or_queries_freqs.argtypes = [vp, vp, vp, vp, sz, vp, vp, C.POINTER(u64), vp]
    lib.dint_wand_data_create.argtypes = [C.c_int, vp, u64, C.POINTER(vp)]
    lib.dint_wand_data_destroy.restype = None
    lib.dint_wand_data_destroy.argtypes = [vp]
    lib.dint_ranked_and_queries.argtypes = [vp, vp, vp, u32, vp, vp, sz, vp, vp, vp, vp]
    lib.dint_ranked_bool_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_queries.argtypes = [vp, vp, vp, u32, vp, vp, sz, vp, vp, vp, vp]
    lib.dint_ranked_or_bool_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_range_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_range_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_doc_filter_create.argtypes = [vp, vp, u64, C.POINTER(vp)]
    lib.dint_doc_filter_info_get.argtypes = [vp, C.POINTER(DocFilterInfo)]
    lib.dint_doc_filter_destroy.argtypes = [vp]
    lib.dint_doc_filter_destroy.restype = None
    lib.dint_ranked_or_filtered_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_filtered_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_doc_facets_create.argtypes = [C.c_int, vp, u64, u32, C.POINTER(vp)]
    lib.dint_doc_facets_info_get.argtypes = [vp, C.POINTER(DocFacetsInfo)]
    lib.dint_doc_facets_group_sizes.argtypes = [vp, vp]
    lib.dint_doc_facets_destroy.argtypes = [vp]
    lib.dint_doc_facets_destroy.restype = None
    lib.dint_ranked_or_faceted_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_faceted_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_collapsed_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_collapsed_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_paged_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_paged_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_collapsed_paged_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_collapsed_paged_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_group_limit_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_group_limit_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_doc_values_create.argtypes = [C.c_int, vp, u64, C.POINTER(vp)]
    lib.dint_doc_values_info_get.argtypes = [vp, C.POINTER(DocValuesInfo)]
    lib.dint_doc_values_destroy.argtypes = [vp]
    lib.dint_doc_values_destroy.restype = None
    lib.dint_doc_filter_create_from_values.argtypes = [vp, vp, u32, u32, C.POINTER(vp)]
    lib.dint_ranked_or_sorted_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_sorted_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    # (qi, freqs, wand, k, terms, offsets, filter, values, edges, n_edges, n_queries, counts, matches, scores, docids, stats,
    # bucket_counts, hit_values, blocks_decoded, stream)
    lib.dint_ranked_or_value_stats_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_value_stats_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_or_group_stats_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_group_stats_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    # (qi, freqs, wand, k, terms, offsets, filter, values, per_million, n_percentiles, n_queries, counts, matches, scores, docids,
    # value_counts, percentile_values, stats, blocks_decoded, stream)
    lib.dint_ranked_or_percentile_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_percentile_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, vp, u32, sz, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    # (qi, freqs, wand, k, terms, offsets, filter, values, n_top, n_queries, counts, matches, scores, docids, value_counts,
    # distinct_counts, top_n, top_values, top_counts, blocks_decoded, stream)
    lib.dint_ranked_or_top_values_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_ranked_and_top_values_queries.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, u32, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_wand_data_create_with_max_weights.argtypes = [C.c_int, vp, u64, vp, sz, C.POINTER(vp)]
    lib.dint_ranked_or_maxscore_queries.argtypes = [vp, vp, vp, u32, vp, vp, sz, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_score_documents.argtypes = [vp, vp, vp, vp, vp, sz, vp, vp, vp, vp, C.POINTER(u64), vp]
    lib.dint_index_max_weights.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.dint_wand_data_set_block_max_weights.argtypes = [vp, vp, sz]
    lib.dint_check_index.argtypes = [vp, vp, C.POINTER(CollectionView), C.POINTER(u64), C.POINTER(IndexMismatch), vp]
    lib.dint_count_ngrams.argtypes = [C.c_int, C.c_int, vp, u64, vp, u64, C.c_uint32, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_float)]
    lib.dint_select_ngrams.argtypes = [C.c_int, vp, u64, u64, vp, sz, C.c_uint32, C.POINTER(sz)]
    lib.dint_debug_wave_scan.argtypes = [vp, vp]
    return lib


_lib = _load()


MAX_UNIT_INTS = 1 << 28  # DINT_MAX_UNIT_INTS (include/dint_hip.h)


class DintError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        detail = _lib.dint_last_hip_error().decode()
        super().__init__(f"{where}: {_lib.dint_strerror(status).decode()} ({status})"
                         + (f" — {detail}" if detail and status == -3 else ""))


def _check(status: int, where: str) -> None:
    if status != 0:
        raise DintError(status, where)


def abi_version() -> int:
    return _lib.dint_abi_version()


#: dint_option (include/dint_hip.h): name -> number, from the library itself
OPTIONS = {}
_i = 0
while _lib.dint_option_name(_i):
    OPTIONS[_lib.dint_option_name(_i).decode()] = _i
    _i += 1

#: the workspace bounds among the options (numbered apart from the switches, include/dint_hip.h): name -> number
LIMITS = {_lib.dint_option_name(32).decode(): 32}  # DINT_OPT_QUERY_OR_PASS_PAGES


def _option_number(name: str) -> int:
    return OPTIONS[name] if name in OPTIONS else LIMITS[name]


def set_option(name: str, value: int) -> None:
    """dint_set_option: a process-wide switch for tests and measurements ("bundles", "index_concurrent",
    "query_lean_pages", "query_tail_pages", "query_fused_pages", ... : device.OPTIONS lists them) or a workspace
    bound ("query_or_pass_pages": device.LIMITS)."""
    _check(_lib.dint_set_option(_option_number(name), int(value)), f"dint_set_option({name})")


def get_option(name: str) -> int:
    v = C.c_longlong()
    _check(_lib.dint_get_option(_option_number(name), C.byref(v)), f"dint_get_option({name})")
    return int(v.value)


def reset_options() -> None:
    _check(_lib.dint_reset_options(), "dint_reset_options")


class options:
    """with device.options(query_fused_pages=0): ...  — the options set inside, restored on the way out."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: get_option(k) for k in self.kw}
        for k, v in self.kw.items():
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def device_count() -> int:
    n = C.c_int()
    _check(_lib.dint_device_count(C.byref(n)), "dint_device_count")
    return n.value


class Dictionary:
    """Device-resident dictionary (reference: Dictionary::builder::load + build(dict))."""

    def __init__(self, kind: int, file_bytes: bytes, device: int = 0):
        self.kind = kind
        self._h = C.c_void_p()
        buf = (C.c_char * len(file_bytes)).from_buffer_copy(file_bytes)
        _check(_lib.dint_dict_create(kind, C.addressof(buf), len(file_bytes), device, C.byref(self._h)),
               "dint_dict_create")
        self.device = device

    def close(self) -> None:
        h, self._h = self._h, C.c_void_p()
        if h and _lib is not None:  # (None at interpreter shutdown)
            _lib.dint_dict_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> DictInfo:
        info = DictInfo()
        _check(_lib.dint_dict_info_get(self._h, C.byref(info)), "dint_dict_info_get")
        return info

    # -- H3: sidecar ---------------------------------------------------------
    def index_stream(self, enc: np.ndarray, unit_ints: int = 4096):
        """Host pre-pass over a vroom stream -> (unit table, total ints, number of lists)."""
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        units, n_units = C.c_void_p(), C.c_size_t()
        total, lists = C.c_uint64(), C.c_uint64()
        _check(_lib.dint_index_stream(self._h, enc.ctypes.data, enc.size, unit_ints, C.byref(units),
                                      C.byref(n_units), C.byref(total), C.byref(lists)), "dint_index_stream")
        try:
            arr = np.empty(n_units.value, dtype=UNIT_DTYPE)
            if n_units.value:
                C.memmove(arr.ctypes.data, units, arr.nbytes)
        finally:
            _lib.dint_free(units)
        return arr, total.value, lists.value

    # -- decode ----------------------------------------------------------------
    def decode_units(self, enc_dev, units_dev, n_units: int, out_dev, end_off_dev=None, stream=None) -> None:
        """Asynchronous batched decode. All tensors are torch CUDA tensors on this
        dictionary's device: enc_dev uint8, units_dev the raw bytes of a UNIT_DTYPE
        table, out_dev int32/uint32 storage, end_off_dev (optional) int64[n_units]."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(enc_dev.device).cuda_stream
        _check(_lib.dint_decode_units(
            self._h, enc_dev.data_ptr(), enc_dev.numel() * enc_dev.element_size(), units_dev.data_ptr(), n_units,
            out_dev.data_ptr(), out_dev.numel(), end_off_dev.data_ptr() if end_off_dev is not None else None,
            stream), "dint_decode_units")

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        _check(_lib.dint_last_kernel_ms(self._h, C.byref(ms)), "dint_last_kernel_ms")
        return ms.value

    def last_kernel_clock_mhz(self) -> float:
        """The shader clock the most recent decode kernel ran at (its first wave's cycle count / its duration)."""
        mhz = C.c_float()
        _check(_lib.dint_last_kernel_clock_mhz(self._h, C.byref(mhz)), "dint_last_kernel_clock_mhz")
        return mhz.value

    def recent_kernel_ms(self, max_n: int = 64) -> np.ndarray:
        """Kernel times (ms) of the most recent launches, oldest first (from their own event pairs)."""
        out = np.zeros(max_n, dtype=np.float32)
        n = C.c_size_t()
        _check(_lib.dint_recent_kernel_ms(self._h, out.ctypes.data, max_n, C.byref(n)), "dint_recent_kernel_ms")
        return out[: n.value].copy()

    def stream_stats(self, enc: np.ndarray) -> StreamStats:
        """Host pre-pass: what the stream is made of (codewords, exceptions, on-chip share)."""
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        st = StreamStats()
        _check(_lib.dint_stream_stats_get(self._h, enc.ctypes.data, enc.size, C.byref(st)), "dint_stream_stats_get")
        return st

    def decode_list(self, enc: np.ndarray, offset: int, n: int):
        """The reference's Decoder::decode(dict, in, out, universe, n) call shape on host
        memory -> (out[0:n], bytes consumed). One wavefront wide: for tests and small lists."""
        enc = np.ascontiguousarray(enc, dtype=np.uint8)
        out = np.empty(n, dtype=np.uint32)
        consumed = C.c_size_t()
        _check(_lib.dint_decode_list_host(self._h, enc.ctypes.data + offset, enc.size - offset, out.ctypes.data, n,
                                          C.byref(consumed)), "dint_decode_list_host")
        return out, consumed.value


class UnitTable:
    """A unit table prepared once for repeated decodes of one resident stream (dint_unit_table): the bundle schedule —
    a property of the stream and its sidecar — is computed here, a decode is then one kernel launch. Borrows the
    dictionary and the two device tensors (kept alive here)."""

    def __init__(self, dictionary: "Dictionary", enc_dev, units_dev, n_units: int, out_capacity: int, stream=None):
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(enc_dev.device).cuda_stream
        self._dict, self._enc, self._units = dictionary, enc_dev, units_dev
        self._h = C.c_void_p()
        _check(_lib.dint_unit_table_create(dictionary._h, enc_dev.data_ptr(), enc_dev.numel() * enc_dev.element_size(),
                                           units_dev.data_ptr(), n_units, out_capacity, stream, C.byref(self._h)),
               "dint_unit_table_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.dint_unit_table_destroy(h)

    __del__ = close

    def decode(self, out_dev, end_off_dev=None, stream=None) -> None:
        """Enqueue the decode of every unit (asynchronous)."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(out_dev.device).cuda_stream
        _check(_lib.dint_decode_unit_table(self._dict._h, self._h, out_dev.data_ptr(), out_dev.numel(),
                                           end_off_dev.data_ptr() if end_off_dev is not None else None, stream),
               "dint_decode_unit_table")

    def rank_outputs(self, outs, stream=None):
        """dint_unit_table_rank_outputs: decode into every candidate output tensor, -> (kernel ms of each, index of the
        fastest). The kernel's time depends on where the output lies relative to the stream."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(outs[0].device).cuda_stream
        ptrs = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        ms = (C.c_float * len(outs))()
        best = C.c_size_t(0)
        _check(_lib.dint_unit_table_rank_outputs(self._dict._h, self._h, ptrs, len(outs), min(o.numel() for o in outs), stream, ms,
                                                 C.byref(best)), "dint_unit_table_rank_outputs")
        return [float(x) for x in ms], int(best.value)


def probe_placement(dictionary: "Dictionary", encs, units_dev, n_units: int, outs, sample_ints: int = 0, stream=None) -> np.ndarray:
    """dint_probe_placement: kernel ms of a sampled decode on every (stream copy, output buffer) pair -> float array
    [len(encs), len(outs)]. `encs`: CUDA tensors holding the same encoded bytes at different addresses."""
    import torch

    if stream is None:
        stream = torch.cuda.current_stream(outs[0].device).cuda_stream
    e = (C.c_void_p * len(encs))(*[t.data_ptr() for t in encs])
    o = (C.c_void_p * len(outs))(*[t.data_ptr() for t in outs])
    ms = (C.c_float * (len(encs) * len(outs)))()
    _check(_lib.dint_probe_placement(dictionary._h, e, len(encs), min(t.numel() for t in encs), units_dev.data_ptr(), n_units, o,
                                     len(outs), min(t.numel() for t in outs), int(sample_ints), stream, ms), "dint_probe_placement")
    return np.array(list(ms), dtype=np.float64).reshape(len(encs), len(outs))


def decode_block(dictionary: "Dictionary", buf: np.ndarray, offset: int, sum_of_values: int, n: int):
    """The reference's in-index block Coder call, Coder::decode(dict, in, out, sum_of_values, n), on host
    memory -> (out[0:n], bytes consumed)."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    out = np.empty(n, dtype=np.uint32)
    consumed = C.c_size_t()
    _check(_lib.dint_decode_block_host(dictionary._h, buf.ctypes.data + offset, buf.size - offset, out.ctypes.data,
                                       sum_of_values & 0xFFFFFFFF, n, C.byref(consumed)), "dint_decode_block_host")
    return out, consumed.value


class ListCache:
    """One posting list (host bytes, dict_posting_list layout) decoded once on the device; `decode(offset, n)` is then the
    block Coder's call for the docs or freqs part that starts `offset` bytes into the list, served from host memory."""

    def __init__(self, docs_dict: "Dictionary", freqs_dict, list_bytes: np.ndarray):
        self._list = np.ascontiguousarray(list_bytes, dtype=np.uint8)
        self._h = C.c_void_p()
        _check(_lib.dint_list_cache_create(docs_dict._h, freqs_dict._h if freqs_dict is not None else None,
                                           self._list.ctypes.data, self._list.size, C.byref(self._h)), "dint_list_cache_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.dint_list_cache_destroy(h)

    __del__ = close

    def decode(self, offset: int, n: int, sum_of_values=None):
        """sum_of_values: the Coder call's (0xFFFFFFFF: the freqs part that starts at `offset`, else the docs part:
        dint_list_cache_decode_part); None: whichever part starts there (dint_list_cache_decode)."""
        out = np.empty(n, dtype=np.uint32)
        consumed = C.c_size_t()
        if sum_of_values is None:
            _check(_lib.dint_list_cache_decode(self._h, offset, out.ctypes.data, n, C.byref(consumed)), "dint_list_cache_decode")
        else:
            _check(_lib.dint_list_cache_decode_part(self._h, offset, sum_of_values & 0xFFFFFFFF, out.ctypes.data, n,
                                                    C.byref(consumed)), "dint_list_cache_decode_part")
        return out, consumed.value


def alloc_count() -> int:
    """Device / pinned allocations the library has made so far in this process (test hook)."""
    n = C.c_uint64()
    _check(_lib.dint_debug_alloc_count(C.byref(n)), "dint_debug_alloc_count")
    return n.value


def index_posting_lists(index: np.ndarray, list_offsets: np.ndarray):
    """Host: flatten the block directories of the posting lists starting at list_offsets[:-1]
    (dict_posting_list layout) -> (block table BLOCK_DTYPE[], total postings)."""
    index = np.ascontiguousarray(index, dtype=np.uint8)
    offs = np.ascontiguousarray(list_offsets, dtype=np.uint64)
    n_lists = max(0, len(offs) - 1)
    blocks, n_blocks, total = C.c_void_p(), C.c_size_t(), C.c_uint64()
    _check(_lib.dint_index_posting_lists(index.ctypes.data, index.size, offs.ctypes.data, n_lists, C.byref(blocks),
                                         C.byref(n_blocks), C.byref(total)), "dint_index_posting_lists")
    try:
        arr = np.empty(n_blocks.value, dtype=BLOCK_DTYPE)
        if n_blocks.value:
            C.memmove(arr.ctypes.data, blocks, arr.nbytes)
    finally:
        _lib.dint_free(blocks)
    return arr, total.value


def decode_posting_lists(docs_dict: "Dictionary", freqs_dict, index: np.ndarray, blocks: np.ndarray, total: int):
    """Upload an index + block table, decode every posting on the device, download.
    -> (docids u32[], freqs u32[] or None)"""
    import torch

    dev = torch.device("cuda", docs_dict.device)
    padded = np.concatenate([np.ascontiguousarray(index, dtype=np.uint8), np.zeros(16, dtype=np.uint8)])
    index_dev = torch.from_numpy(padded).to(dev)
    blocks_dev = torch.from_numpy(np.ascontiguousarray(blocks).view(np.uint8).copy()).to(dev)
    docids_dev = torch.empty(max(1, total), dtype=torch.int32, device=dev)
    freqs_dev = torch.empty(max(1, total), dtype=torch.int32, device=dev) if freqs_dict is not None else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    _check(_lib.dint_decode_posting_blocks(
        docs_dict._h, freqs_dict._h if freqs_dict is not None else None, index_dev.data_ptr(), padded.size,
        blocks_dev.data_ptr(), len(blocks), docids_dev.data_ptr(),
        freqs_dev.data_ptr() if freqs_dev is not None else None, total, stream), "dint_decode_posting_blocks")
    torch.cuda.synchronize(dev)
    docids = docids_dev.cpu().numpy().view(np.uint32)[:total]
    freqs = freqs_dev.cpu().numpy().view(np.uint32)[:total] if freqs_dev is not None else None
    return docids, freqs


class BlockTable:
    """A block table prepared once for asynchronous in-index decodes (dint_block_table)."""

    def __init__(self, docs_dict: "Dictionary", blocks: np.ndarray, index_bytes: int):
        self._h = C.c_void_p()
        self._blocks = np.ascontiguousarray(blocks)
        _check(_lib.dint_block_table_create(docs_dict._h, self._blocks.ctypes.data, len(self._blocks), index_bytes,
                                            C.byref(self._h)), "dint_block_table_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.dint_block_table_destroy(h)

    __del__ = close

    def learn(self, docs_dict, freqs_dict, index_dev, index_bytes, stream=None):
        """The sizing pass at set-up (dint_block_table_learn): after it the first decode is already the one launch."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(index_dev.device).cuda_stream
        _check(_lib.dint_block_table_learn(self._h, docs_dict._h, freqs_dict._h if freqs_dict is not None else None,
                                           index_dev.data_ptr(), index_bytes, stream), "dint_block_table_learn")

    def ready(self, with_freqs: bool = True) -> bool:
        return bool(_lib.dint_block_table_ready(self._h, int(with_freqs)))

    def info(self) -> dict:
        i = BlockTableInfo()
        _check(_lib.dint_block_table_info_get(self._h, C.byref(i)), "dint_block_table_info_get")
        return {k: int(getattr(i, k)) for k, _ in BlockTableInfo._fields_}

    def decode(self, docs_dict, freqs_dict, index_dev, index_bytes, docids_dev, freqs_dev, stream=None):
        """Enqueue the decode of every block (asynchronous); tensors are CUDA tensors on the dictionaries' device."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(index_dev.device).cuda_stream
        _check(_lib.dint_decode_block_table(
            docs_dict._h, freqs_dict._h if freqs_dict is not None else None, index_dev.data_ptr(), index_bytes, self._h,
            docids_dev.data_ptr(), freqs_dev.data_ptr() if freqs_dev is not None else None, docids_dev.numel(), stream),
            "dint_decode_block_table")


class QueryIndex:
    """An index resident on the device, ready for conjunctive, disjunctive, ranked conjunctive and ranked disjunctive
    queries: the reference's `index` + `and_query` / `or_query` / `ranked_and_query` / `ranked_or_query` pairs
    (include/ds2i/queries.hpp:34-130, :309-457), a batch per call."""

    def __init__(self, docs_dict: "Dictionary", index: np.ndarray, list_offsets: np.ndarray):
        import torch

        self.docs_dict = docs_dict
        self.blocks, self.total = index_posting_lists(index, list_offsets)
        self.n_lists = max(0, len(list_offsets) - 1)
        dev = torch.device("cuda", docs_dict.device)
        padded = np.concatenate([np.ascontiguousarray(index, dtype=np.uint8), np.zeros(16, dtype=np.uint8)])
        self._index_dev = torch.from_numpy(padded).to(dev)
        self._h = C.c_void_p()
        _check(_lib.dint_query_index_create(docs_dict._h, self._index_dev.data_ptr(), padded.size,
                                            self.blocks.ctypes.data, len(self.blocks), self.n_lists,
                                            C.byref(self._h)), "dint_query_index_create")

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:  # (None at interpreter shutdown)
            _lib.dint_query_index_destroy(h)

    __del__ = close

    def _stream(self) -> int:
        """The current stream of this index's device."""
        import torch

        return torch.cuda.current_stream(torch.device("cuda", self.docs_dict.device)).cuda_stream

    def and_queries(self, queries) -> np.ndarray:
        """queries: sequence of term-id sequences -> u64 result counts, one per query."""
        terms, offs = _pack_queries(queries)
        counts = np.zeros(len(queries), dtype=np.uint64)
        _check(_lib.dint_and_queries(self._h, terms.ctypes.data, offs.ctypes.data, len(queries), counts.ctypes.data,
                                     self._stream()), "dint_and_queries")
        return counts

    def and_queries_packed(self, terms: np.ndarray, offsets: np.ndarray, counts: np.ndarray, stream: int = 0) -> None:
        """The bare call: queries already packed (`terms` u32, `offsets` u64[n + 1], `counts` u64[n] out) — what a
        C++ caller hands over; and_queries() packs Python lists first."""
        _check(_lib.dint_and_queries(self._h, terms.ctypes.data, offsets.ctypes.data, counts.size, counts.ctypes.data, stream),
               "dint_and_queries")

    def and_queries_with_freqs(self, freqs_dict: "Dictionary", queries):
        """`and_query<true>` for a batch -> (counts u64[], sums of the freqs read at the matches u64[], freqs blocks decoded)."""
        terms, offs = _pack_queries(queries)
        counts = np.zeros(len(queries), dtype=np.uint64)
        sums = np.zeros(len(queries), dtype=np.uint64)
        nblocks = C.c_uint64()
        _check(_lib.dint_and_queries_freqs(self._h, freqs_dict._h, terms.ctypes.data, offs.ctypes.data, len(queries),
                                           counts.ctypes.data, sums.ctypes.data, C.byref(nblocks), self._stream()),
               "dint_and_queries_freqs")
        return counts, sums, nblocks.value

    def or_queries(self, queries) -> np.ndarray:
        """or_query<false> (include/ds2i/queries.hpp:86-130) for a batch: queries -> u64 counts of the union, one per query."""
        terms, offs = _pack_queries(queries)
        counts = np.zeros(len(queries), dtype=np.uint64)
        _check(_lib.dint_or_queries(self._h, terms.ctypes.data, offs.ctypes.data, len(queries), counts.ctypes.data,
                                    self._stream()), "dint_or_queries")
        return counts

    def or_queries_packed(self, terms: np.ndarray, offsets: np.ndarray, counts: np.ndarray, stream: int = 0) -> None:
        """The bare call, as and_queries_packed."""
        _check(_lib.dint_or_queries(self._h, terms.ctypes.data, offsets.ctypes.data, counts.size, counts.ctypes.data, stream),
               "dint_or_queries")

    def or_queries_with_freqs(self, freqs_dict: "Dictionary", queries):
        """`or_query<true>` for a batch -> (counts, sums of the freqs of every posting of every distinct term, freqs blocks decoded)."""
        terms, offs = _pack_queries(queries)
        counts = np.zeros(len(queries), dtype=np.uint64)
        sums = np.zeros(len(queries), dtype=np.uint64)
        nblocks = C.c_uint64()
        _check(_lib.dint_or_queries_freqs(self._h, freqs_dict._h, terms.ctypes.data, offs.ctypes.data, len(queries),
                                          counts.ctypes.data, sums.ctypes.data, C.byref(nblocks), self._stream()),
               "dint_or_queries_freqs")
        return counts, sums, nblocks.value

    def _ranked(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, k: int):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data, n,
                                 counts.ctypes.data, scores.ctypes.data, docids.ctypes.data, self._stream()), fn)
        return counts, scores, docids

    def ranked_and_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, k: int = 10):
        """ranked_and_query (include/ds2i/queries.hpp:309-385) for a batch: BM25 top-k of the intersection ->
        (counts u64[n] = min(k, matches), scores f32[n, k] descending, docids u32[n, k]; equal scores by ascending docID,
        0.0 / 0xFFFFFFFF past a query's count)."""
        return self._ranked("dint_ranked_and_queries", freqs_dict, wand, queries, k)

    def ranked_bool_queries(self, freqs_dict: "Dictionary", wand: "WandData", must, should=None, exclude=None, k: int = 10):
        """Ranked boolean queries (dint_ranked_bool_queries): per query the documents in every list of
        must[q] and in no list of exclude[q], scored over the required terms as ranked_and_queries scores them and then over
        the optional terms of should[q] whose list holds the document, in ascending term id. should / exclude: None, or a
        sequence per query like must. A query without a required term selects nothing -> (counts u64[n] = min(k, matches),
        matches u64[n], scores f32[n, k] descending, docids u32[n, k] as ranked_and_queries, blocks decoded behind the AND
        rounds)."""
        n = len(must)
        assert all(c is None or len(c) == n for c in (should, exclude))
        m_terms, m_offs = _pack_queries(must)
        packed = [_pack_queries(c) if c is not None else (None, None) for c in (should, exclude)]
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(_lib.dint_ranked_bool_queries(self._h, freqs_dict._h, wand._h, k, m_terms.ctypes.data, m_offs.ctypes.data,
                                             ptr(packed[0][0]), ptr(packed[0][1]), ptr(packed[1][0]), ptr(packed[1][1]), n,
                                             counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                             C.byref(blocks), self._stream()), "dint_ranked_bool_queries")
        return counts, matches, scores, docids, blocks.value

    def ranked_or_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, k: int = 10):
        """ranked_or_query (include/ds2i/queries.hpp:387-457) for a batch: BM25 top-k of the union, each document's score
        summed over the query's terms in ascending term id -> (counts u64[n] = min(k, |union|), scores f32[n, k]
        descending, docids u32[n, k]; equal scores by ascending docID, 0.0 / 0xFFFFFFFF past a query's count)."""
        return self._ranked("dint_ranked_or_queries", freqs_dict, wand, queries, k)

    def ranked_or_bool_queries(self, freqs_dict: "Dictionary", wand: "WandData", should, exclude=None, min_should_match=None,
                               k: int = 10):
        """Union-driven ranked boolean queries (dint_ranked_or_bool_queries): per query the documents
        held by at least m = max(1, min_should_match[q]) of the distinct lists of should[q] and by no list of exclude[q],
        each with its ranked_or_queries score over should[q] (ascending term id; excluded terms never score). exclude: None,
        or a sequence per query like should; min_should_match: None (all 1) or an integer per query. m above the query's
        distinct terms selects nothing -> (counts u64[n] = min(k, matches), matches u64[n], scores f32[n, k] descending,
        docids u32[n, k] as ranked_or_queries, blocks decoded: every block of the optional terms of the queries that can
        match, plus the blocks the exclusion steps claimed)."""
        n = len(should)
        assert exclude is None or len(exclude) == n
        s_terms, s_offs = _pack_queries(should)
        x_terms, x_offs = _pack_queries(exclude) if exclude is not None else (None, None)
        mins = None
        if min_should_match is not None:
            mins = np.ascontiguousarray(min_should_match, dtype=np.uint32)
            assert mins.shape == (n,)
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(_lib.dint_ranked_or_bool_queries(self._h, freqs_dict._h, wand._h, k, s_terms.ctypes.data, s_offs.ctypes.data,
                                                ptr(x_terms), ptr(x_offs), ptr(mins), n, counts.ctypes.data, matches.ctypes.data,
                                                scores.ctypes.data, docids.ctypes.data, C.byref(blocks), self._stream()),
               "dint_ranked_or_bool_queries")
        return counts, matches, scores, docids, blocks.value

    def _ranked_range(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, ranges, k: int, with_stats: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        pairs = None
        if ranges is not None:
            wide = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)  # (int64 first: a value past u32 is refused, not wrapped)
            assert wide.shape == (n, 2) and (n == 0 or (wide.min() >= 0 and wide.max() <= 0xFFFFFFFF))
            pairs = np.ascontiguousarray(wide, dtype=np.uint32)  # dint_doc_range {lo, hi}
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 pairs.ctypes.data if pairs is not None else None, n, counts.ctypes.data, matches.ctypes.data,
                                 scores.ctypes.data, docids.ctypes.data, C.byref(blocks), self._stream()), fn)
        return (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)

    def ranked_or_range_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, ranges, k: int = 10,
                                with_stats: bool = False):
        """ranked_or_queries over the documents of a docID interval per query (dint_ranked_or_range_queries, DESIGN.md
        4d-range): ranges is an (n, 2) array-like of u32, query q ranking over ranges[q][0] <= docID < ranges[q][1], or None
        (every query unrestricted). A match scores exactly what ranked_or_queries gives it; only the blocks that can hold a
        docID of the range are decoded -> (counts u64[n] = min(k, matches), scores f32[n, k], docids u32[n, k] as
        ranked_or_queries) and, with_stats, (matches u64[n]: the union's documents in range, blocks decoded: every distinct
        term's blocks in range, summed over the queries)."""
        return self._ranked_range("dint_ranked_or_range_queries", freqs_dict, wand, queries, ranges, k, with_stats)

    def ranked_and_range_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, ranges, k: int = 10,
                                 with_stats: bool = False):
        """ranked_and_queries over the documents of a docID interval per query (dint_ranked_and_range_queries, DESIGN.md
        4d-range): arguments and outputs as ranked_or_range_queries; matches: the intersection's documents in range, blocks
        decoded: the candidate pages, i.e. the blocks in range of every query's rarest list."""
        return self._ranked_range("dint_ranked_and_range_queries", freqs_dict, wand, queries, ranges, k, with_stats)

    def doc_filter(self, mask_or_docids, num_docs=None, form=None) -> "DocFilter":
        """A document filter for this index (dint_doc_filter_create) from a bool array (document d in
        the filter iff mask[d]; num_docs defaults to its length), a u64 array of bitmap words (bit d & 63 of word d >> 6;
        num_docs defaults to 64 * its length; with num_docs, exactly ceil(num_docs / 64) words) or a sequence of docIDs
        (num_docs defaults to the largest + 1; those at or past a given num_docs are left out). form ("mask", "words" or
        "docids") says which it is; without it the dtype does (bool, u64, anything else), so docIDs held in a u64 array
        need form="docids". Close it before the index."""
        return DocFilter(self, mask_or_docids, num_docs, form)

    def _ranked_filtered(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, doc_filter, k: int, with_stats: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, n, counts.ctypes.data, matches.ctypes.data,
                                 scores.ctypes.data, docids.ctypes.data, C.byref(blocks), self._stream()), fn)
        return (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)

    def ranked_or_filtered_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, doc_filter, k: int = 10,
                                   with_stats: bool = False):
        """ranked_or_queries over the documents of one filter for the whole batch (dint_ranked_or_filtered_queries, DESIGN.md
        4d-filter): doc_filter is a DocFilter of this index, or None (unrestricted). A match scores exactly what
        ranked_or_queries gives it; only the live blocks — those whose docID span holds a document of the filter — are
        decoded -> (counts u64[n] = min(k, matches), scores f32[n, k], docids u32[n, k] as ranked_or_queries) and,
        with_stats, (matches u64[n]: the union's documents in the filter, blocks decoded: every distinct term's live blocks,
        summed over the queries)."""
        return self._ranked_filtered("dint_ranked_or_filtered_queries", freqs_dict, wand, queries, doc_filter, k, with_stats)

    def ranked_and_filtered_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, doc_filter, k: int = 10,
                                    with_stats: bool = False):
        """ranked_and_queries over the documents of one filter (dint_ranked_and_filtered_queries):
        arguments and outputs as ranked_or_filtered_queries; matches: the intersection's documents in the filter, blocks
        decoded: the candidate pages, i.e. the live blocks of every query's rarest list."""
        return self._ranked_filtered("dint_ranked_and_filtered_queries", freqs_dict, wand, queries, doc_filter, k, with_stats)

    def _ranked_faceted(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, facets, doc_filter, k: int, with_stats: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        rows = np.zeros((n, facets.n_groups), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, facets._h, n, counts.ctypes.data,
                                 matches.ctypes.data, scores.ctypes.data, docids.ctypes.data, rows.ctypes.data, C.byref(blocks),
                                 self._stream()), fn)
        return (counts, scores, docids, matches, blocks.value, rows) if with_stats else (counts, scores, docids, rows)

    def ranked_or_faceted_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", filter=None,
                                  k: int = 10, with_stats: bool = False):
        """ranked_or_filtered_queries with the matches counted per document group (dint_ranked_or_faceted_queries, DESIGN.md
        4d-facets): facets is a DocFacets on this index's device, filter a DocFilter of this index or None (unrestricted)
        -> what ranked_or_filtered_queries returns for (queries, filter, k, with_stats), bit for bit, and behind it
        rows u32[n, n_groups]: rows[q, g] = the matches of query q in group g, over every match, not over the top k."""
        return self._ranked_faceted("dint_ranked_or_faceted_queries", freqs_dict, wand, queries, facets, filter, k, with_stats)

    def ranked_and_faceted_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", filter=None,
                                   k: int = 10, with_stats: bool = False):
        """ranked_and_filtered_queries with the matches counted per document group (dint_ranked_and_faceted_queries):
        arguments and outputs as ranked_or_faceted_queries, over the intersection."""
        return self._ranked_faceted("dint_ranked_and_faceted_queries", freqs_dict, wand, queries, facets, filter, k, with_stats)

    def _ranked_collapsed(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, facets, doc_filter, k: int, with_stats: bool,
                          with_rows: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        collapsed = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        hit_groups = np.zeros((n, k), dtype=np.uint32)
        hit_group_matches = np.zeros((n, k), dtype=np.uint32)
        rows = np.zeros((n, facets.n_groups), dtype=np.uint32) if with_rows else None
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, facets._h, n, counts.ctypes.data,
                                 matches.ctypes.data, collapsed.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                 hit_groups.ctypes.data, hit_group_matches.ctypes.data, rows.ctypes.data if with_rows else None,
                                 C.byref(blocks), self._stream()), fn)
        out = (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)
        out += (collapsed, hit_groups, hit_group_matches)
        return out + (rows,) if with_rows else out

    def ranked_or_collapsed_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", filter=None,
                                    k: int = 10, with_stats: bool = False, with_rows: bool = False):
        """ranked_or_faceted_queries with at most one hit per document group (dint_ranked_or_collapsed_queries, DESIGN.md
        4d-collapse): of every group a query matches only the match with the best key (higher score, then smaller docID) is
        kept, a match in no group stands for itself, and the top k of the kept documents are returned. Arguments as the
        faceted method takes them -> (counts, scores, docids) — with_stats: (counts, scores, docids, matches, blocks_decoded),
        matches and blocks_decoded the faceted call's — and behind them collapsed u64[n] (the kept documents: groups with a
        match plus ungrouped matches; counts = min(collapsed, k)), hit_groups u32[n, k] (FACET_NONE for an ungrouped hit and
        past the count), hit_group_matches u32[n, k] (the query's matches in the hit's group, 1 for an ungrouped hit, 0 past
        the count); with_rows: the faceted call's rows u32[n, n_groups] last."""
        return self._ranked_collapsed("dint_ranked_or_collapsed_queries", freqs_dict, wand, queries, facets, filter, k, with_stats, with_rows)

    def ranked_and_collapsed_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", filter=None,
                                     k: int = 10, with_stats: bool = False, with_rows: bool = False):
        """ranked_and_faceted_queries with at most one hit per document group (dint_ranked_and_collapsed_queries): arguments
        and outputs as ranked_or_collapsed_queries, over the intersection."""
        return self._ranked_collapsed("dint_ranked_and_collapsed_queries", freqs_dict, wand, queries, facets, filter, k, with_stats, with_rows)

    def _ranked_paged(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, after, doc_filter, k: int, with_stats: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        cursors = _pack_cursors(after, n)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        skipped = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, cursors.ctypes.data if cursors is not None else None, n,
                                 counts.ctypes.data, matches.ctypes.data, skipped.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                 C.byref(blocks), self._stream()), fn)
        return (counts, scores, docids, matches, blocks.value, skipped) if with_stats else (counts, scores, docids, skipped)

    def ranked_or_paged_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, after=None, filter=None, k: int = 10,
                                with_stats: bool = False):
        """ranked_or_filtered_queries behind a cursor per query (dint_ranked_or_paged_queries): after is
        None (every query from the start) or a list of n entries, each None (from the start) or (score, docid) — the last hit
        the caller has seen; it need not be a match. A match (s, d) lies after (cs, cd) iff s < cs, or s == cs and d > cd,
        compared on the float's bits; a score <= 0 leaves nothing after it, a NaN is refused. filter: a DocFilter of this
        index or None -> what ranked_or_filtered_queries returns for (queries, filter, k, with_stats) — counts =
        min(k, matches - skipped), scores and docids the best k AFTER the cursor, matches and blocks_decoded unchanged by it —
        and behind it skipped u64[n]: the matches not after the cursor, i.e. the rank of the page's first hit. Every page
        decodes and scores the whole query again."""
        return self._ranked_paged("dint_ranked_or_paged_queries", freqs_dict, wand, queries, after, filter, k, with_stats)

    def ranked_and_paged_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, after=None, filter=None, k: int = 10,
                                 with_stats: bool = False):
        """ranked_and_filtered_queries behind a cursor per query (dint_ranked_and_paged_queries): arguments and outputs as
        ranked_or_paged_queries, over the intersection."""
        return self._ranked_paged("dint_ranked_and_paged_queries", freqs_dict, wand, queries, after, filter, k, with_stats)

    def _ranked_collapsed_paged(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, facets, after, doc_filter, k: int,
                                with_stats: bool, with_rows: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        cursors = _pack_cursors(after, n)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        collapsed = np.zeros(n, dtype=np.uint64)
        skipped = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        hit_groups = np.zeros((n, k), dtype=np.uint32)
        hit_group_matches = np.zeros((n, k), dtype=np.uint32)
        rows = np.zeros((n, facets.n_groups), dtype=np.uint32) if with_rows else None
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, facets._h,
                                 cursors.ctypes.data if cursors is not None else None, n, counts.ctypes.data, matches.ctypes.data,
                                 collapsed.ctypes.data, skipped.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                 hit_groups.ctypes.data, hit_group_matches.ctypes.data, rows.ctypes.data if with_rows else None,
                                 C.byref(blocks), self._stream()), fn)
        out = (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)
        out += (collapsed, hit_groups, hit_group_matches)
        return (out + (rows,) if with_rows else out) + (skipped,)

    def ranked_or_collapsed_paged_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", after=None,
                                          filter=None, k: int = 10, with_stats: bool = False, with_rows: bool = False):
        """ranked_or_collapsed_queries behind a cursor per query (dint_ranked_or_collapsed_paged_queries):
        after as ranked_or_paged_queries takes it. The cursor applies to the kept documents, after the best of every group is
        taken, so the pages of a walk show every group once -> what ranked_or_collapsed_queries returns for the same
        arguments — counts = min(k, collapsed - skipped), the hits those after the cursor, collapsed, matches, the rows and
        blocks_decoded unchanged by it — and last skipped u64[n]: the kept documents not after the cursor."""
        return self._ranked_collapsed_paged("dint_ranked_or_collapsed_paged_queries", freqs_dict, wand, queries, facets, after, filter, k,
                                            with_stats, with_rows)

    def ranked_and_collapsed_paged_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", after=None,
                                           filter=None, k: int = 10, with_stats: bool = False, with_rows: bool = False):
        """ranked_and_collapsed_queries behind a cursor per query (dint_ranked_and_collapsed_paged_queries): arguments and
        outputs as ranked_or_collapsed_paged_queries, over the intersection."""
        return self._ranked_collapsed_paged("dint_ranked_and_collapsed_paged_queries", freqs_dict, wand, queries, facets, after, filter, k,
                                            with_stats, with_rows)

    def _ranked_group_limit(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, facets, per_group: int, after, doc_filter,
                            k: int, with_stats: bool, with_rows: bool):
        if not 1 <= int(per_group) <= GROUP_LIMIT_MAX:
            raise ValueError(f"{fn}: per_group must be in 1 .. {GROUP_LIMIT_MAX}, not {per_group!r}")
        terms, offs = _pack_queries(queries)
        n = len(queries)
        cursors = _pack_cursors(after, n)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        kept = np.zeros(n, dtype=np.uint64)
        skipped = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        hit_groups = np.zeros((n, k), dtype=np.uint32)
        hit_group_matches = np.zeros((n, k), dtype=np.uint32)
        hit_group_ranks = np.zeros((n, k), dtype=np.uint32)
        rows = np.zeros((n, facets.n_groups), dtype=np.uint32) if with_rows else None
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, facets._h, int(per_group),
                                 cursors.ctypes.data if cursors is not None else None, n, counts.ctypes.data, matches.ctypes.data,
                                 kept.ctypes.data, skipped.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                 hit_groups.ctypes.data, hit_group_matches.ctypes.data, hit_group_ranks.ctypes.data,
                                 rows.ctypes.data if with_rows else None, C.byref(blocks), self._stream()), fn)
        out = (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)
        out += (kept, hit_groups, hit_group_matches, hit_group_ranks)
        return (out + (rows,) if with_rows else out) + (skipped,)

    def ranked_or_group_limit_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", per_group: int,
                                      after=None, filter=None, k: int = 10, with_stats: bool = False, with_rows: bool = False):
        """ranked_or_faceted_queries with at most per_group hits per document group (dint_ranked_or_group_limit_queries,
        DESIGN.md 4d-group-limit): of every group a query matches its min(per_group, matches) matches with the best keys
        (higher score, then smaller docID) are kept, a match in no group stands for itself, and the top k of the kept
        documents after the cursor are returned. per_group: 1 .. GROUP_LIMIT_MAX (ValueError otherwise); after as
        ranked_or_paged_queries takes it, applied to the kept documents -> what ranked_or_collapsed_paged_queries returns
        for the same arguments, with kept u64[n] where collapsed stands (counts = min(k, kept - skipped)) and
        hit_group_ranks u32[n, k] behind hit_group_matches: the hit's 0-based place among all matches of its group in key
        order (< per_group; 0 for an ungrouped hit and past the count); skipped u64[n] stays last. per_group = 1 is the
        collapsed paged method, every rank 0."""
        return self._ranked_group_limit("dint_ranked_or_group_limit_queries", freqs_dict, wand, queries, facets, per_group, after, filter, k,
                                        with_stats, with_rows)

    def ranked_and_group_limit_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", per_group: int,
                                       after=None, filter=None, k: int = 10, with_stats: bool = False, with_rows: bool = False):
        """ranked_and_faceted_queries with at most per_group hits per document group (dint_ranked_and_group_limit_queries):
        arguments and outputs as ranked_or_group_limit_queries, over the intersection."""
        return self._ranked_group_limit("dint_ranked_and_group_limit_queries", freqs_dict, wand, queries, facets, per_group, after, filter, k,
                                        with_stats, with_rows)

    def doc_filter_from_values(self, values: "DocValues", lo: int, hi: int) -> "DocFilter":
        """The filter of the documents d < values.num_docs with lo <= v(d) <= hi (closed; lo > hi: the empty filter), built
        on the device from the column (dint_doc_filter_create_from_values): in its info and under every
        filtered call it equals doc_filter of the same bitmap. Close it before the index."""
        return DocFilter.from_values(self, values, lo, hi)

    def _ranked_sorted(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, values, descending, after, doc_filter, k: int,
                       with_stats: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        cursors = _pack_value_cursors(after, n)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        skipped = np.zeros(n, dtype=np.uint64)
        hit_values = np.zeros((n, k), dtype=np.uint32)
        docids = np.zeros((n, k), dtype=np.uint32)
        scores = np.zeros((n, k), dtype=np.float32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, values._h, SORT_DESC if descending else SORT_ASC,
                                 cursors.ctypes.data if cursors is not None else None, n, counts.ctypes.data, matches.ctypes.data,
                                 skipped.ctypes.data, hit_values.ctypes.data, docids.ctypes.data, scores.ctypes.data, C.byref(blocks),
                                 self._stream()), fn)
        if with_stats:
            return counts, hit_values, docids, scores, matches, blocks.value, skipped
        return counts, hit_values, docids, scores, skipped

    def ranked_or_sorted_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", descending: bool = True,
                                 after=None, filter=None, k: int = 10, with_stats: bool = False):
        """ranked_or_filtered_queries' matches ordered by a column instead of the score (dint_ranked_or_sorted_queries, DESIGN.md
        4d-values): values is a DocValues on this index's device; descending: the larger value first, else the smaller; equal
        values go by ascending docID in both orders. after is None (every query from the start) or a list of n entries, each
        None or (value, docid) — the last hit the caller has seen; it need not be a match. filter: a DocFilter of this index or
        None -> (counts u64[n] = min(k, matches - skipped), hit_values u32[n, k], docids u32[n, k], scores f32[n, k] — every
        hit's score exactly the filtered call's —, skipped u64[n]: the matches not after the cursor); with_stats: (counts,
        hit_values, docids, scores, matches, blocks_decoded, skipped), matches and blocks_decoded the filtered call's. Past
        the count: 0, 0xFFFFFFFF, 0.0."""
        return self._ranked_sorted("dint_ranked_or_sorted_queries", freqs_dict, wand, queries, values, descending, after, filter, k, with_stats)

    def ranked_and_sorted_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", descending: bool = True,
                                  after=None, filter=None, k: int = 10, with_stats: bool = False):
        """ranked_and_filtered_queries' matches ordered by a column (dint_ranked_and_sorted_queries): arguments and outputs as
        ranked_or_sorted_queries, over the intersection."""
        return self._ranked_sorted("dint_ranked_and_sorted_queries", freqs_dict, wand, queries, values, descending, after, filter, k, with_stats)

    def _ranked_value_stats(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, values, edges, doc_filter, k: int,
                            with_stats: bool):
        edges = _pack_value_edges(edges)
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        stats = np.zeros(n, dtype=_VALUE_STATS)
        buckets = np.zeros((n, edges.size + 1), dtype=np.uint32) if edges.size else None
        hit_values = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, values._h, edges.ctypes.data if edges.size else None,
                                 edges.size, n, counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                 stats.ctypes.data, buckets.ctypes.data if buckets is not None else None, hit_values.ctypes.data,
                                 C.byref(blocks), self._stream()), fn)
        head = (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)
        return head + (stats, buckets, hit_values)

    def ranked_or_value_stats_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", edges=None,
                                      filter=None, k: int = 10, with_stats: bool = False):
        """ranked_or_filtered_queries with a column reduced over every match (dint_ranked_or_value_stats_queries, DESIGN.md
        4d-stats): values is a DocValues on this index's device, edges None or up to 1023 strictly ascending u32 bucket
        boundaries (ValueError otherwise, before the call), filter a DocFilter of this index or None (unrestricted) -> what
        ranked_or_filtered_queries returns for (queries, filter, k, with_stats), bit for bit, and behind it stats (a structured
        array of n records with the fields n, sum, min, max over the matches d < values.num_docs — matches at or past the
        column have no value; no valued match: (0, 0, 0xFFFFFFFF, 0)), buckets u32[n, n_edges + 1] (None without edges):
        buckets[q, b] = the valued matches of q with b edges <= their value, and hit_values u32[n, k]: the values of the
        hits (0 past the count and for a hit past the column)."""
        return self._ranked_value_stats("dint_ranked_or_value_stats_queries", freqs_dict, wand, queries, values, edges, filter, k, with_stats)

    def ranked_and_value_stats_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", edges=None,
                                       filter=None, k: int = 10, with_stats: bool = False):
        """ranked_and_filtered_queries with a column reduced over every match (dint_ranked_and_value_stats_queries): arguments
        and outputs as ranked_or_value_stats_queries, over the intersection."""
        return self._ranked_value_stats("dint_ranked_and_value_stats_queries", freqs_dict, wand, queries, values, edges, filter, k, with_stats)

    def _ranked_group_stats(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, facets, values, doc_filter, k: int,
                            with_facet_counts: bool):
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        group_stats = np.zeros((n, facets.n_groups), dtype=_VALUE_STATS)
        rows = np.zeros((n, facets.n_groups), dtype=np.uint32) if with_facet_counts else None
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, facets._h, values._h, n, counts.ctypes.data,
                                 matches.ctypes.data, scores.ctypes.data, docids.ctypes.data, group_stats.ctypes.data,
                                 rows.ctypes.data if with_facet_counts else None, C.byref(blocks), self._stream()), fn)
        return counts, scores, docids, matches, blocks.value, group_stats, rows

    def ranked_or_group_stats_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", values: "DocValues",
                                      filter=None, k: int = 10, with_facet_counts: bool = False):
        """ranked_or_filtered_queries with a column reduced over every match per document group
        (dint_ranked_or_group_stats_queries): facets is a DocFacets and values a DocValues on this
        index's device, filter a DocFilter of this index or None (unrestricted) -> (counts, scores, docids, matches,
        blocks_decoded, group_stats, facet_counts): the first five what ranked_or_filtered_queries returns with with_stats for
        (queries, filter, k), bit for bit; group_stats a structured array [n, n_groups] with the fields n, sum, min, max over the
        matches d of the query with d < facets.num_docs, group_of[d] == g and d < values.num_docs (no such match:
        (0, 0, 0xFFFFFFFF, 0)); facet_counts u32[n, n_groups], the faceted call's rows — every match per group, valued or not —
        with with_facet_counts, else None."""
        return self._ranked_group_stats("dint_ranked_or_group_stats_queries", freqs_dict, wand, queries, facets, values, filter, k,
                                        with_facet_counts)

    def ranked_and_group_stats_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, facets: "DocFacets", values: "DocValues",
                                       filter=None, k: int = 10, with_facet_counts: bool = False):
        """ranked_and_filtered_queries with a column reduced over every match per document group
        (dint_ranked_and_group_stats_queries): arguments and outputs as ranked_or_group_stats_queries, over the intersection."""
        return self._ranked_group_stats("dint_ranked_and_group_stats_queries", freqs_dict, wand, queries, facets, values, filter, k,
                                        with_facet_counts)

    def _ranked_percentiles(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, values, percentiles, doc_filter, k: int,
                            with_stats: bool):
        per_million = _pack_percentiles(percentiles)
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        value_counts = np.zeros(n, dtype=np.uint64)
        percentile_values = np.zeros((n, per_million.size), dtype=np.uint32)
        stats = np.zeros(n, dtype=_VALUE_STATS) if with_stats else None
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, values._h, per_million.ctypes.data, per_million.size,
                                 n, counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                 value_counts.ctypes.data, percentile_values.ctypes.data,
                                 stats.ctypes.data if with_stats else None, C.byref(blocks), self._stream()), fn)
        head = (counts, scores, docids, matches, blocks.value) if with_stats else (counts, scores, docids)
        return head + (value_counts, percentile_values, stats)

    def ranked_or_percentile_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", percentiles,
                                     filter=None, k: int = 10, with_stats: bool = False):
        """ranked_or_filtered_queries with exact percentiles of a column over every match (dint_ranked_or_percentile_queries,
        DESIGN.md 4d-percentiles): values is a DocValues on this index's device, percentiles 1 to 16 numbers in percent, each in
        [0, 100], in any order, repeats allowed, taken as round(p * 10000) parts per million (ValueError otherwise, before the
        call), filter a DocFilter of this index or None (unrestricted) -> what ranked_or_filtered_queries returns for (queries,
        filter, k, with_stats), bit for bit, and behind it value_counts u64[n]: the matches d < values.num_docs of every query,
        percentile_values u32[n, n_percentiles]: [q, j] = s[((n_q - 1) * per_million[j]) // 1000000] of the ascending sort s of
        those matches' values (the lower nearest rank; 0 where n_q == 0), and stats: with_stats the value-stats records (n, sum,
        min, max; no valued match: (0, 0, 0xFFFFFFFF, 0)), else None — then the call launches nothing for them."""
        return self._ranked_percentiles("dint_ranked_or_percentile_queries", freqs_dict, wand, queries, values, percentiles, filter, k,
                                        with_stats)

    def ranked_and_percentile_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", percentiles,
                                      filter=None, k: int = 10, with_stats: bool = False):
        """ranked_and_filtered_queries with exact percentiles of a column over every match (dint_ranked_and_percentile_queries):
        arguments and outputs as ranked_or_percentile_queries, over the intersection."""
        return self._ranked_percentiles("dint_ranked_and_percentile_queries", freqs_dict, wand, queries, values, percentiles, filter, k,
                                        with_stats)

    def _ranked_top_values(self, fn: str, freqs_dict: "Dictionary", wand: "WandData", queries, values, n_top: int, doc_filter, k: int):
        terms, offs = _pack_queries(queries)
        n, n_top = len(queries), int(n_top)
        counts = np.zeros(n, dtype=np.uint64)
        matches = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        value_counts = np.zeros(n, dtype=np.uint64)
        distinct_counts = np.zeros(n, dtype=np.uint64)
        top_n = np.zeros(n, dtype=np.uint32)
        top_values = np.zeros((n, max(n_top, 0)), dtype=np.uint32)
        top_counts = np.zeros((n, max(n_top, 0)), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(getattr(_lib, fn)(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data,
                                 doc_filter._h if doc_filter is not None else None, values._h, n_top, n, counts.ctypes.data,
                                 matches.ctypes.data, scores.ctypes.data, docids.ctypes.data, value_counts.ctypes.data,
                                 distinct_counts.ctypes.data, top_n.ctypes.data, top_values.ctypes.data if n_top else None,
                                 top_counts.ctypes.data if n_top else None, C.byref(blocks), self._stream()), fn)
        return counts, scores, docids, matches, blocks.value, value_counts, distinct_counts, top_n, top_values, top_counts

    def ranked_or_top_values_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", n_top: int,
                                     filter=None, k: int = 10):
        """ranked_or_filtered_queries with the most frequent values of a column over every match and the number of different
        ones (dint_ranked_or_top_values_queries): values is a DocValues on this index's device, n_top 0
        to TOP_VALUES_MAX (0: the counts only; the library refuses more), filter a DocFilter of this index or None
        (unrestricted) -> (counts, scores, docids, matches, blocks_decoded) as ranked_or_filtered_queries returns them with
        with_stats for (queries, filter, k), bit for bit, and behind them value_counts u64[n]: the matches d < values.num_docs of
        every query, distinct_counts u64[n]: the different values among them, top_n u32[n] = min(n_top, distinct), and
        top_values, top_counts u32[n, n_top]: [q, i], i < top_n[q], the values by count descending, then value ascending, and
        their counts; 0 past top_n[q]."""
        return self._ranked_top_values("dint_ranked_or_top_values_queries", freqs_dict, wand, queries, values, n_top, filter, k)

    def ranked_and_top_values_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, values: "DocValues", n_top: int,
                                      filter=None, k: int = 10):
        """ranked_and_filtered_queries with the most frequent values of a column over every match and the number of different
        ones (dint_ranked_and_top_values_queries): arguments and outputs as ranked_or_top_values_queries, over the intersection."""
        return self._ranked_top_values("dint_ranked_and_top_values_queries", freqs_dict, wand, queries, values, n_top, filter, k)

    def ranked_pages(self, entry: str, freqs_dict: "Dictionary", wand: "WandData", queries, k: int = 10, filter=None, facets=None,
                     after=None, max_pages=None, values=None, descending: bool = True, per_group=None):
        """Walks a batch page by page: entry is "or", "and", "or_collapsed" or "and_collapsed" (the
        collapsed ones need facets), "or_group_limit" or "and_group_limit" (they need facets and
        per_group), or "or_sorted" / "and_sorted" (they need values, a DocValues, and
        take descending). The first page starts at `after` (None: from the start); each query's next cursor is its
        last hit, and a query drops out of the batch when a page comes back short (fewer than k hits: nothing lies behind it).
        Yields per page (query ids — indices into `queries` of the queries still in the batch —, counts, scores, docids,
        skipped), a row per query id — a sorted entry: (query ids, counts, hit_values, docids, scores, skipped), and the next
        cursor is (hit_value, docid) of a page's last hit; stops after max_pages pages or when no query is left. Every page is
        a call of its own and decodes and scores its queries again."""
        calls = {"or": self.ranked_or_paged_queries, "and": self.ranked_and_paged_queries,
                 "or_collapsed": self.ranked_or_collapsed_paged_queries, "and_collapsed": self.ranked_and_collapsed_paged_queries,
                 "or_group_limit": self.ranked_or_group_limit_queries, "and_group_limit": self.ranked_and_group_limit_queries,
                 "or_sorted": self.ranked_or_sorted_queries, "and_sorted": self.ranked_and_sorted_queries}
        if entry not in calls:
            raise ValueError(f"ranked_pages: entry must be one of {sorted(calls)}, not {entry!r}")
        collapsed = entry.endswith("_collapsed")
        if collapsed and facets is None:
            raise ValueError("ranked_pages: a collapsed entry needs facets")
        limited = entry.endswith("_group_limit")
        if limited and (facets is None or per_group is None):
            raise ValueError("ranked_pages: a group_limit entry needs facets and per_group")
        if entry.endswith("_sorted"):
            if values is None:
                raise ValueError("ranked_pages: a sorted entry needs values")
            ids = np.arange(len(queries), dtype=np.int64)
            cursors = list(after) if after is not None else [None] * len(queries)
            if len(cursors) != len(queries):
                raise ValueError(f"ranked_pages: {len(cursors)} cursors for {len(queries)} queries")
            page = 0
            while len(ids) and (max_pages is None or page < max_pages):
                counts, hit_values, docids, scores, skipped = calls[entry](
                    freqs_dict, wand, [queries[i] for i in ids], values, descending=descending, after=[cursors[i] for i in ids],
                    filter=filter, k=k)
                yield ids.copy(), counts, hit_values, docids, scores, skipped
                for j, i in enumerate(ids):
                    if counts[j]:
                        cursors[i] = (int(hit_values[j, int(counts[j]) - 1]), int(docids[j, int(counts[j]) - 1]))
                ids = ids[counts == k]
                page += 1
            return
        ids = np.arange(len(queries), dtype=np.int64)
        cursors = list(after) if after is not None else [None] * len(queries)
        if len(cursors) != len(queries):
            raise ValueError(f"ranked_pages: {len(cursors)} cursors for {len(queries)} queries")
        page = 0
        while len(ids) and (max_pages is None or page < max_pages):
            batch = [queries[i] for i in ids]
            batch_after = [cursors[i] for i in ids]
            if limited:
                out = calls[entry](freqs_dict, wand, batch, facets, per_group, after=batch_after, filter=filter, k=k)
            elif collapsed:
                out = calls[entry](freqs_dict, wand, batch, facets, after=batch_after, filter=filter, k=k)
            else:
                out = calls[entry](freqs_dict, wand, batch, after=batch_after, filter=filter, k=k)
            counts, scores, docids, skipped = out[0], out[1], out[2], out[-1]
            yield ids.copy(), counts, scores, docids, skipped
            for j, i in enumerate(ids):
                if counts[j]:
                    cursors[i] = (scores[j, int(counts[j]) - 1], int(docids[j, int(counts[j]) - 1]))
            ids = ids[counts == k]
            page += 1

    def ranked_or_maxscore_queries(self, freqs_dict: "Dictionary", wand: "WandData", queries, k: int = 10):
        """ranked_or_queries' answer, bit for bit, with MaxScore's pruning: the blocks of low-weight
        lists that no candidate able to reach the top k falls in are not decoded. `wand` must carry max_term_weight ->
        (counts, scores, docids as ranked_or_queries, blocks read: the distinct index blocks the queries decoded, summed)."""
        terms, offs = _pack_queries(queries)
        n = len(queries)
        counts = np.zeros(n, dtype=np.uint64)
        scores = np.zeros((n, k), dtype=np.float32)
        docids = np.zeros((n, k), dtype=np.uint32)
        blocks = C.c_uint64()
        _check(_lib.dint_ranked_or_maxscore_queries(self._h, freqs_dict._h, wand._h, k, terms.ctypes.data, offs.ctypes.data, n,
                                                    counts.ctypes.data, scores.ctypes.data, docids.ctypes.data, C.byref(blocks),
                                                    self._stream()), "dint_ranked_or_maxscore_queries")
        return counts, scores, docids, blocks.value

    def score_documents(self, freqs_dict: "Dictionary", wand: "WandData", queries, docs, with_freqs: bool = False):
        """next_geq(d) + freq() (include/dint/dict_posting_list.hpp:126-169) with ranked_or_query's sums, for documents the
        caller names (dint_score_documents): docs[q] — any u32 docIDs, in any order, repeated or not — are
        scored for queries[q] -> (scores: a list of f32 arrays, one per query, each the ranked_or_queries score of that
        document, 0.0 if no list of the query holds it; freqs: with_freqs, a list of u32 [n_docs, T] arrays, T the query's
        distinct terms in ascending id, 0 = not in the list, else None; blocks read: the distinct (term, block) pairs decoded)."""
        assert len(docs) == len(queries)
        terms, offs = _pack_queries(queries)
        ids, doc_offs = _pack_queries(docs)
        n = len(queries)
        scores = np.zeros(max(1, ids.size), dtype=np.float32)
        n_terms = [len(set(int(t) for t in q)) for q in queries]
        sizes = [int(doc_offs[q + 1] - doc_offs[q]) * n_terms[q] for q in range(n)]
        freqs = np.zeros(max(1, sum(sizes)), dtype=np.uint32) if with_freqs else None
        blocks = C.c_uint64()
        _check(_lib.dint_score_documents(self._h, freqs_dict._h, wand._h, terms.ctypes.data, offs.ctypes.data, n, ids.ctypes.data,
                                         doc_offs.ctypes.data, scores.ctypes.data, freqs.ctypes.data if with_freqs else None,
                                         C.byref(blocks), self._stream()), "dint_score_documents")
        out = [scores[int(doc_offs[q]):int(doc_offs[q + 1])] for q in range(n)]
        mats = None
        if with_freqs:
            at = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            mats = [freqs[at[q]:at[q + 1]].reshape(int(doc_offs[q + 1] - doc_offs[q]), n_terms[q]) for q in range(n)]
        return out, mats, blocks.value

    def max_weights(self, freqs_dict: "Dictionary", wand: "WandData", with_blocks: bool = False):
        """The wand data's BM25 maxima from the index, on the device (dint_index_max_weights): every
        block decoded once -> max_term_weight f32[n_lists], bit for bit host.wand_data's second array (`wand` carrying that
        call's norm_lens); with_blocks: (max_term_weight, block_max_weight f32[n_blocks]), one maximum per block of
        self.blocks, for WandData.set_block_max_weights."""
        mtw = np.zeros(self.n_lists, dtype=np.float32)
        bmw = np.zeros(len(self.blocks), dtype=np.float32) if with_blocks else None
        _check(_lib.dint_index_max_weights(self._h, freqs_dict._h, wand._h, mtw.ctypes.data if mtw.size else None,
                                           bmw.ctypes.data if with_blocks else None, self._stream()), "dint_index_max_weights")
        return (mtw, bmw) if with_blocks else mtw

    def check(self, freqs_dict, docs, freqs, docs_at, freqs_at, list_len):
        """The index checked against its collection on the device (dint_check_index; the reference's
        verify_collection): list i of the collection is docs[docs_at[i] : docs_at[i] + list_len[i]] (u32; offsets and
        lengths u64) and freqs[freqs_at[i] : ...]; freqs_dict, freqs and freqs_at None: docIDs only. Returns
        (n_mismatches, first): wrong lengths + wrong postings, and None or the Mismatch (kind, list, position, expected,
        got) the reference's walk would have stopped at."""
        def arr(a, dtype):
            return None if a is None else np.ascontiguousarray(a, dtype=dtype)

        docs, freqs = arr(docs, np.uint32), arr(freqs, np.uint32)
        docs_at, freqs_at, list_len = arr(docs_at, np.uint64), arr(freqs_at, np.uint64), arr(list_len, np.uint64)
        ptr = lambda a: None if a is None else a.ctypes.data
        view = CollectionView(ptr(docs), ptr(freqs), ptr(docs_at), ptr(freqs_at), ptr(list_len), 0 if list_len is None else list_len.size)
        n, first = C.c_uint64(), IndexMismatch()
        _check(_lib.dint_check_index(self._h, freqs_dict._h if freqs_dict is not None else None, C.byref(view), C.byref(n),
                                     C.byref(first), self._stream()), "dint_check_index")
        if first.kind == CHECK_OK:
            return n.value, None
        return n.value, Mismatch(first.kind, first.list, first.position, first.expected, first.got)


def doc_filter_words(mask_or_docids, num_docs=None, form=None):
    """What QueryIndex.doc_filter hands the library: (u64 bitmap words, num_docs) from a bool mask, u64 words or docIDs.
    form: "mask", "words" or "docids"; None: by dtype — bool, u64, anything else. A u64 array taken as words must have
    exactly ceil(num_docs / 64) of them where num_docs is given: docIDs that happen to be u64 are refused, not misread."""
    a = np.asarray(mask_or_docids)
    if form is None:
        form = "mask" if a.dtype == np.bool_ else "words" if a.dtype == np.uint64 else "docids"
    if form not in ("mask", "words", "docids"):
        raise ValueError("form is 'mask', 'words' or 'docids'")
    if form == "mask":
        a = a.astype(np.bool_, copy=False)
        n = a.size if num_docs is None else int(num_docs)
        bits = np.zeros(-(-n // 64) * 64, dtype=np.uint8)
        bits[:min(n, a.size)] = a.reshape(-1)[:n]
        words = np.packbits(bits, bitorder="little").view("<u8")
    elif form == "words":
        n = 64 * a.size if num_docs is None else int(num_docs)
        if a.size != -(-n // 64):
            raise ValueError(f"{a.size} bitmap words for num_docs = {n}: ceil(num_docs / 64) = {-(-n // 64)} are needed "
                             "(docIDs in a u64 array: pass form='docids')")
        words = a.reshape(-1).astype(np.uint64)
    else:
        d = a.astype(np.int64).reshape(-1)
        assert d.size == 0 or (d.min() >= 0 and d.max() < 0xFFFFFFFF)
        n = (int(d.max()) + 1 if d.size else 0) if num_docs is None else int(num_docs)
        d = d[d < n]
        words = np.zeros(-(-n // 64), dtype=np.uint64)
        np.bitwise_or.at(words, d >> 6, np.uint64(1) << (d & 63).astype(np.uint64))
    return np.ascontiguousarray(words, dtype=np.uint64), n


class DocFilter:
    """A document filter of one QueryIndex (dint_doc_filter): a bitmap over the docID space and, found
    on the device when it is made, which blocks of the index can hold a document of it. Immutable; one filter serves
    any number of ranked_*_filtered_queries calls, from several threads. It keeps its index alive; close() it first."""

    def __init__(self, index: "QueryIndex", mask_or_docids, num_docs=None, form=None):
        words, n = doc_filter_words(mask_or_docids, num_docs, form)
        self.index = index
        self._h = C.c_void_p()
        _check(_lib.dint_doc_filter_create(index._h, words.ctypes.data if words.size else None, n, C.byref(self._h)),
               "dint_doc_filter_create")

    @property
    def info(self) -> DocFilterInfo:
        out = DocFilterInfo()
        _check(_lib.dint_doc_filter_info_get(self._h, C.byref(out)), "dint_doc_filter_info_get")
        return out

    @classmethod
    def from_values(cls, index: "QueryIndex", values: "DocValues", lo: int, hi: int) -> "DocFilter":
        """QueryIndex.doc_filter_from_values: the documents of the column with lo <= v(d) <= hi, found on the device"""
        if not (0 <= int(lo) <= 0xFFFFFFFF and 0 <= int(hi) <= 0xFFFFFFFF):
            raise ValueError("lo and hi are u32")
        self = cls.__new__(cls)
        self.index = index
        self._h = C.c_void_p()
        _check(_lib.dint_doc_filter_create_from_values(index._h, values._h, int(lo), int(hi), C.byref(self._h)),
               "dint_doc_filter_create_from_values")
        return self

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:  # (None at interpreter shutdown)
            _lib.dint_doc_filter_destroy(h)

    __del__ = close


FACET_NONE = 0xFFFFFFFF        # DINT_FACET_NONE (include/dint_hip.h): a document in no group
FACETS_MAX_GROUPS = 65536      # DINT_FACETS_MAX_GROUPS
GROUP_LIMIT_MAX = 16           # DINT_GROUP_LIMIT_MAX: the largest per_group of the group-limited ranked calls


def doc_facets_map(group_of, n_groups=None):
    """What DocFacets hands the library: (u32 map, n_groups) from any integer array or sequence; a negative entry or None
    is FACET_NONE (and so is FACET_NONE itself). n_groups defaults to the largest group + 1 (1 if no document is in a
    group). Entries at or past a given n_groups are passed on: the library refuses them (DINT_ERR_ARG)."""
    if not isinstance(group_of, np.ndarray):
        group_of = [-1 if g is None else g for g in group_of]
    a = np.asarray(group_of)
    if a.dtype == object:
        a = np.array([-1 if g is None else int(g) for g in a.reshape(-1)], dtype=np.int64)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError("group_of holds integers (negative or None: in no group)")
    a = a.reshape(-1)
    if a.dtype.kind == "u":
        if a.size and int(a.max()) > FACET_NONE:
            raise ValueError("a group does not fit 32 bits")
        m = a.astype(np.uint32)
    else:
        a = a.astype(np.int64)
        if a.size and int(a.max()) > FACET_NONE:
            raise ValueError("a group does not fit 32 bits")
        m = np.where(a < 0, FACET_NONE, a).astype(np.uint32)
    if n_groups is None:
        real = m[m != FACET_NONE]
        n_groups = int(real.max()) + 1 if real.size else 1
    return np.ascontiguousarray(m, dtype=np.uint32), int(n_groups)


class DocFacets:
    """A document -> group map on a device (dint_doc_facets): group_of[d] is document d's group, a
    negative entry or None no group, and so is every document at or past len(group_of). It belongs to no index — it
    describes documents — holds 4 bytes per document on the device, is immutable and serves any number of
    ranked_*_faceted_queries calls, from several threads. Creation raises DintError (DINT_ERR_ARG) for n_groups of 0 or above
    FACETS_MAX_GROUPS and for an entry at or past n_groups."""

    def __init__(self, device: int, group_of, n_groups=None):
        m, n_groups = doc_facets_map(group_of, n_groups)
        if not 0 <= n_groups <= 0xFFFFFFFF:
            raise ValueError("n_groups does not fit 32 bits")
        self.device = device
        self._h = C.c_void_p()
        _check(_lib.dint_doc_facets_create(device, m.ctypes.data if m.size else None, m.size, n_groups, C.byref(self._h)),
               "dint_doc_facets_create")
        info = DocFacetsInfo()
        _check(_lib.dint_doc_facets_info_get(self._h, C.byref(info)), "dint_doc_facets_info_get")
        self.num_docs, self.n_groups, self.n_grouped = int(info.num_docs), int(info.n_groups), int(info.n_grouped)
        self.group_sizes = np.zeros(self.n_groups, dtype=np.uint32)
        _check(_lib.dint_doc_facets_group_sizes(self._h, self.group_sizes.ctypes.data), "dint_doc_facets_group_sizes")

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:  # (None at interpreter shutdown)
            _lib.dint_doc_facets_destroy(h)

    __del__ = close


SORT_DESC, SORT_ASC = 0, 1    # DINT_SORT_DESC, DINT_SORT_ASC (include/dint_hip.h)


class DocValues:
    """A document -> u32 value column on a device (dint_doc_values): values[d] is document d's value,
    every 32-bit value is legal, and a document at or past len(values) sorts as value 0. It belongs to no index, holds 4
    bytes per document on the device, is immutable and serves any number of ranked_*_sorted_queries and
    doc_filter_from_values calls, from several threads."""

    def __init__(self, device: int, values):
        a = np.asarray(values)
        if a.size and a.dtype.kind not in "iu":
            raise TypeError("values holds integers (floats: DocValues.from_float32)")
        if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("a value does not fit u32")
        v = np.ascontiguousarray(a.reshape(-1), dtype=np.uint32)
        self.device = device
        self._h = C.c_void_p()
        _check(_lib.dint_doc_values_create(device, v.ctypes.data if v.size else None, v.size, C.byref(self._h)), "dint_doc_values_create")
        info = DocValuesInfo()
        _check(_lib.dint_doc_values_info_get(self._h, C.byref(info)), "dint_doc_values_info_get")
        self.num_docs = int(info.num_docs)

    @staticmethod
    def float32_keys(x) -> np.ndarray:
        """binary32 -> order-preserving u32: bits with the sign bit set are inverted, all others get the sign bit set, so
        -0.0 sorts directly below +0.0. A NaN raises."""
        f = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        if np.isnan(f).any():
            raise ValueError("a NaN has no place in the order")
        bits = f.view(np.uint32)
        return np.where(bits >> 31 != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)

    @classmethod
    def from_float32(cls, device: int, x) -> "DocValues":
        """A column of binary32 numbers, mapped by float32_keys: sorting by the column sorts by the numbers."""
        return cls(device, cls.float32_keys(x))

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:  # (None at interpreter shutdown)
            _lib.dint_doc_values_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


class WandData:
    """The wand data's document lengths on the device (dint_wand_data_create): norm_lens f32[num_docs], as
    host.wand_data / host.read_wand_data give them; with max_term_weight f32[n_lists] (the same functions' second array)
    the handle also carries the term maxima that ranked_or_maxscore_queries needs (dint_wand_data_create_with_max_weights).
    Creation raises DintError (DINT_ERR_ARG) for a NaN or negative maximum; maxima above the true ones, up to +inf, are
    legal and only make the pruned call read more blocks."""

    MAX_K = 1024  # DINT_RANKED_MAX_K (include/dint_hip.h)

    def __init__(self, norm_lens: np.ndarray, device: int = 0, max_term_weight=None):
        nl = np.ascontiguousarray(norm_lens, dtype=np.float32)
        self.num_docs = nl.size
        self.device = device
        self._h = C.c_void_p()
        if max_term_weight is None:
            _check(_lib.dint_wand_data_create(device, nl.ctypes.data, nl.size, C.byref(self._h)), "dint_wand_data_create")
        else:
            mw = np.ascontiguousarray(max_term_weight, dtype=np.float32)
            _check(_lib.dint_wand_data_create_with_max_weights(device, nl.ctypes.data, nl.size, mw.ctypes.data, mw.size,
                                                               C.byref(self._h)), "dint_wand_data_create_with_max_weights")

    def set_block_max_weights(self, block_max_weight) -> None:
        """Block maxima (QueryIndex.max_weights(..., with_blocks=True)'s second array) for ranked_or_maxscore_queries: with
        them the call bounds a candidate by the maxima of the blocks it falls in (dint_wand_data_set_block_max_weights).
        Raises DintError (DINT_ERR_ARG) for a NaN or negative value and leaves the handle as it was; a second call replaces
        the first's maxima. Not to be called while another thread runs a query with this handle."""
        bm = np.ascontiguousarray(block_max_weight, dtype=np.float32)
        _check(_lib.dint_wand_data_set_block_max_weights(self._h, bm.ctypes.data if bm.size else None, bm.size),
               "dint_wand_data_set_block_max_weights")

    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:  # (None at interpreter shutdown)
            _lib.dint_wand_data_destroy(h)

    __del__ = close


# dint_rank_cursor {float score; uint32_t docid;}
_CURSOR = np.dtype([("score", np.float32), ("docid", np.uint32)])


def _pack_cursors(after, n: int):
    """after (None, or n entries each None or (score, docid)) as an array of dint_rank_cursor, or None: a missing entry is
    score +inf (from the start); the score goes in as the binary32 it is or rounds to."""
    if after is None:
        return None
    if len(after) != n:
        raise ValueError(f"{len(after)} cursors for {n} queries")
    out = np.zeros(n, dtype=_CURSOR)
    for i, c in enumerate(after):
        if c is None:
            out[i] = (np.float32(np.inf), 0)
            continue
        score, docid = c
        if not 0 <= int(docid) <= 0xFFFFFFFF:
            raise ValueError(f"cursor {i}: the docID {docid} is not a u32")
        out[i] = (np.float32(score), int(docid))
    return out


# dint_value_cursor {uint32_t value; uint32_t docid; uint32_t set;}
_VALUE_CURSOR = np.dtype([("value", np.uint32), ("docid", np.uint32), ("set", np.uint32)])


def _pack_value_cursors(after, n: int):
    """after (None, or n entries each None or (value, docid)) as an array of dint_value_cursor, or None: a missing entry has
    set == 0 (from the start)."""
    if after is None:
        return None
    if len(after) != n:
        raise ValueError(f"{len(after)} cursors for {n} queries")
    out = np.zeros(n, dtype=_VALUE_CURSOR)
    for i, c in enumerate(after):
        if c is None:
            continue
        value, docid = c
        if not (0 <= int(value) <= 0xFFFFFFFF and 0 <= int(docid) <= 0xFFFFFFFF):
            raise ValueError(f"cursor {i}: ({value}, {docid}) are not u32")
        out[i] = (int(value), int(docid), 1)
    return out


#: dint_value_stats (include/dint_hip.h): 24 bytes
_VALUE_STATS = np.dtype([("n", np.uint64), ("sum", np.uint64), ("min", np.uint32), ("max", np.uint32)])
VALUE_STATS_MAX_EDGES = 1023


def _pack_value_edges(edges):
    """-> the bucket boundaries as a contiguous u32 array (None: none). ValueError for more than VALUE_STATS_MAX_EDGES, for a
    value outside 0 .. 2^32 - 1 and for edges that are not strictly ascending."""
    if edges is None:
        return np.zeros(0, dtype=np.uint32)
    e = [int(x) for x in np.asarray(edges).reshape(-1).tolist()]
    if len(e) > VALUE_STATS_MAX_EDGES:
        raise ValueError(f"value edges: at most {VALUE_STATS_MAX_EDGES}, not {len(e)}")
    if any(x < 0 or x > 0xFFFFFFFF for x in e):
        raise ValueError("value edges: every edge must lie in 0 .. 2^32 - 1")
    if any(a >= b for a, b in zip(e, e[1:])):
        raise ValueError("value edges: must be strictly ascending")
    return np.array(e, dtype=np.uint32)


PERCENTILES_MAX = 16  # DINT_PERCENTILES_MAX (include/dint_hip.h)
TOP_VALUES_MAX = 1024  # DINT_TOP_VALUES_MAX


def _pack_percentiles(percentiles):
    """-> the percentiles, given in percent, as a contiguous u32 array of parts per million: round(p * 10000). ValueError for
    none, for more than PERCENTILES_MAX and for a value outside [0, 100]."""
    p = [float(x) for x in np.asarray(percentiles, dtype=np.float64).reshape(-1).tolist()]
    if not p or len(p) > PERCENTILES_MAX:
        raise ValueError(f"percentiles: 1 to {PERCENTILES_MAX}, not {len(p)}")
    if any(not 0.0 <= x <= 100.0 for x in p):  # (a NaN fails both comparisons)
        raise ValueError("percentiles: every percentile must lie in [0, 100]")
    return np.array([int(round(x * 10000)) for x in p], dtype=np.uint32)


def _pack_queries(queries):
    lens = np.fromiter((len(q) for q in queries), dtype=np.uint64, count=len(queries))
    offs = np.zeros(len(queries) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offs[1:])
    terms = np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.uint32) for q in queries])
                                 if len(queries) else np.zeros(0, np.uint32), dtype=np.uint32)
    return terms, offs


NGRAM_DTYPE = np.dtype([("pos", "<u8"), ("freq", "<u4"), ("len", "u1"), ("ctx", "u1"), ("pad", "<u2")])  # dint_ngram


def count_ngrams(gaps_dev, list_starts: np.ndarray, multi: bool, device: int = 0, top_k: int = 0):
    """Block statistics on the device (dint_count_ngrams): gaps_dev — a torch CUDA tensor of u32 d-gaps, lists back
    to back; list_starts — their n + 1 offsets; top_k > 0: only the entries that can make the first top_k of their
    context. -> (entries NGRAM_DTYPE[], kernel ms)."""
    starts = np.ascontiguousarray(list_starts, dtype=np.uint64)
    out, n, ms = C.c_void_p(), C.c_size_t(), C.c_float()
    _check(_lib.dint_count_ngrams(device, int(bool(multi)), gaps_dev.data_ptr(), gaps_dev.numel(), starts.ctypes.data,
                                  len(starts) - 1, top_k, C.byref(out), C.byref(n), C.byref(ms)), "dint_count_ngrams")
    try:
        arr = np.empty(n.value, dtype=NGRAM_DTYPE)
        if n.value:
            C.memmove(arr.ctypes.data, out, arr.nbytes)
    finally:
        _lib.dint_free(out)
    return arr, ms.value


def select_ngrams(gaps_dev, entries: np.ndarray, total_ints: int, device: int = 0, top_k: int = 65536) -> np.ndarray:
    """The selection on the device (dint_select_ngrams): of count_ngrams' entries, the ones the filter keeps, every context's
    in dictionary order, the first top_k of each."""
    e = np.ascontiguousarray(entries, dtype=NGRAM_DTYPE).copy()
    n = C.c_size_t()
    _check(_lib.dint_select_ngrams(device, gaps_dev.data_ptr(), gaps_dev.numel(), total_ints, e.ctypes.data, e.size, top_k, C.byref(n)),
           "dint_select_ngrams")
    return e[: n.value]


def build_dictionary(kind: int, coll, max_sample_ints: int = 0, device: int = 0):
    """host.build_dictionary with counting AND selection on the device: the sampled lists' n-grams counted by
    dint_count_ngrams, filtered / sorted / cut to the first 65536 of every context by dint_select_ngrams, packed by the host
    library — byte-identical to the host-only path. -> (dictionary file, counting kernel ms)."""
    import torch

    from . import host

    n_lists, ints = 0, 0
    for n_lists in range(len(coll.lens) + 1):  # the same prefix sample as dinth_build_dictionary
        if n_lists == len(coll.lens):
            break
        if max_sample_ints and n_lists and ints + int(coll.lens[n_lists]) > max_sample_ints:
            break
        ints += int(coll.lens[n_lists])
    starts = np.zeros(n_lists + 1, dtype=np.uint64)
    np.cumsum(coll.lens[:n_lists], out=starts[1:])
    gaps = np.ascontiguousarray(coll.gaps[:ints], dtype=np.uint32)
    gaps_dev = torch.from_numpy(gaps.view(np.int32)).to(torch.device("cuda", device))
    entries, ms = count_ngrams(gaps_dev, starts, kind == host.MULTI_PACKED, device, top_k=65536)  # DSF-65536-16
    chosen = select_ngrams(gaps_dev, entries, ints, device, top_k=65536)
    return host.pack_dictionary(kind, gaps, chosen), ms


def units_to_device(units: np.ndarray, device):
    """Upload a UNIT_DTYPE table as raw bytes."""
    import torch

    raw = np.ascontiguousarray(units).view(np.uint8)
    return torch.from_numpy(raw.copy()).to(device)


def decode_stream(dictionary: Dictionary, enc: np.ndarray, units: np.ndarray, total_ints: int):
    """Upload, decode every unit, download. -> (integers, end offsets, kernel ms)"""
    import torch

    dev = torch.device("cuda", dictionary.device)
    enc_dev = torch.from_numpy(np.ascontiguousarray(enc, dtype=np.uint8)).to(dev)
    units_dev = units_to_device(units, dev)
    out_dev = torch.empty(max(1, total_ints), dtype=torch.int32, device=dev)
    end_dev = torch.zeros(max(1, len(units)), dtype=torch.int64, device=dev)
    dictionary.decode_units(enc_dev, units_dev, len(units), out_dev, end_dev)
    torch.cuda.synchronize(dev)
    ms = dictionary.last_kernel_ms() if len(units) else 0.0
    out = out_dev.cpu().numpy().view(np.uint32)[:total_ints]
    return out, end_dev.cpu().numpy().view(np.uint64)[: len(units)], ms


def debug_wave_scan(values) -> np.ndarray:
    v = np.ascontiguousarray(values, dtype=np.uint32)
    assert v.size == 64
    out = np.empty(64, dtype=np.uint32)
    _check(_lib.dint_debug_wave_scan(v.ctypes.data, out.ctypes.data), "dint_debug_wave_scan")
    return out

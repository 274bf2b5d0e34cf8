"""ctypes binding of include/sbx_depth.h (no torch types, plain pointers and sizes)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(HERE, "csrc", "libsbx_depth.so")
_CLI_PATH = os.path.join(HERE, "csrc", "sbx-depth")
_FLAGSTAT_CLI_PATH = os.path.join(HERE, "csrc", "sbx-flagstat")
_SORT_CLI_PATH = os.path.join(HERE, "csrc", "sbx-sort")
_MARKDUP_CLI_PATH = os.path.join(HERE, "csrc", "sbx-markdup")
_MERGE_CLI_PATH = os.path.join(HERE, "csrc", "sbx-merge")
_VIEW_CLI_PATH = os.path.join(HERE, "csrc", "sbx-view")
_SLICE_CLI_PATH = os.path.join(HERE, "csrc", "sbx-slice")
_SAM_CLI_PATH = os.path.join(HERE, "csrc", "sbx-sam")
_NSORT_CLI_PATH = os.path.join(HERE, "csrc", "sbx-nsort")
_IVIEW_CLI_PATH = os.path.join(HERE, "csrc", "sbx-iview")
_IMPORT_CLI_PATH = os.path.join(HERE, "csrc", "sbx-import")
_INDEX_CLI_PATH = os.path.join(HERE, "csrc", "sbx-index")
_FIXBINS_CLI_PATH = os.path.join(HERE, "csrc", "sbx-fixbins")
_VALIDATE_CLI_PATH = os.path.join(HERE, "csrc", "sbx-validate")
_SUBSAMPLE_CLI_PATH = os.path.join(HERE, "csrc", "sbx-subsample")

SBX_MODE_BASE, SBX_MODE_REGION, SBX_MODE_WINDOW = 0, 1, 2
SBX_FILTER_MAX_OPS = 64
NCOUNTERS = 7


class SbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("sbx error %d: %s" % (code, msg))
        self.code = code
        self.msg = msg


class Region(C.Structure):
    _fields_ = [("ref_id", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32)]


class HeaderInfo(C.Structure):
    _fields_ = [("n_ref", C.c_int32), ("n_samples", C.c_int32), ("n_read_groups", C.c_int32),
                ("sorted_by_coordinate", C.c_int32), ("has_index", C.c_int32), ("reserved", C.c_int32),
                ("n_bgzf_blocks", C.c_uint64), ("compressed_bytes", C.c_uint64), ("uncompressed_bytes", C.c_uint64)]


class RegionStats(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("n_bases", C.c_uint32)]


class FilterOp(C.Structure):
    _fields_ = [("kind", C.c_uint8), ("field", C.c_uint8), ("cmp", C.c_uint8), ("pad", C.c_uint8),
                ("mask", C.c_uint32), ("value", C.c_int64)]


class RegexState(C.Structure):
    _fields_ = [("type", C.c_uint8), ("a", C.c_uint8), ("b", C.c_uint8), ("c", C.c_uint8)]


class Regex(C.Structure):
    _fields_ = [("n_states", C.c_uint8), ("n_classes", C.c_uint8), ("start", C.c_uint8), ("reserved", C.c_uint8),
                ("states", RegexState * 64), ("classes", (C.c_uint8 * 32) * 8)]


class Filter(C.Structure):
    _fields_ = [("n_ops", C.c_int32), ("reserved", C.c_int32), ("ops", FilterOp * SBX_FILTER_MAX_OPS),
                ("strings", C.c_char * 512), ("n_regex", C.c_int32), ("reserved2", C.c_int32), ("regex", Regex * 2)]


class RunStats(C.Structure):
    _fields_ = [("ms_inflate", C.c_double), ("ms_index", C.c_double), ("ms_accumulate", C.c_double),
                ("ms_reduce", C.c_double), ("ms_total", C.c_double), ("ms_h2d", C.c_double),
                ("n_records", C.c_uint64), ("n_admitted", C.c_uint64), ("n_bgzf_blocks", C.c_uint64),
                ("compressed_bytes", C.c_uint64), ("uncompressed_bytes", C.c_uint64), ("counter_bytes", C.c_uint64),
                ("covered_positions", C.c_uint64), ("launches_inflate", C.c_uint64), ("launches_index", C.c_uint64),
                ("launches_accumulate", C.c_uint64), ("ms_huffman", C.c_double), ("ms_lz77", C.c_double),
                ("n_malformed", C.c_uint64), ("n_runs", C.c_uint64), ("uploaded_bytes", C.c_uint64), ("accumulate_read_bytes", C.c_uint64),
                ("token_bytes", C.c_uint64), ("max_alignment_span", C.c_uint64), ("reserved2", C.c_uint64), ("reserved3", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/sbx_depth.h declares (checked by tests/test_abi.py)
ENOMEM = -8


class Batch(C.Structure):
    _fields_ = [("first_ref", C.c_uint32), ("n_refs", C.c_uint32), ("est_bytes", C.c_uint64)]

FLAGSTAT_FIELDS = ("reads", "secondary", "supplementary", "dup", "mapped", "pair_all", "first", "second", "pair_good", "pair_map",
                   "single", "diff_chr", "diff_high")


class Flagstat(C.Structure):
    _fields_ = [(k, C.c_uint64 * 2) for k in FLAGSTAT_FIELDS]

class SortStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records_in", "n_records_out", "inflated_bytes", "sorted_stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("key_bits", "n_sort_passes", "n_batches", "n_windows")] +
                [(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_keys", "ms_sort", "ms_gather", "ms_deflate", "ms_total_wall")])

class MarkdupStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records_in", "n_records_out", "n_end_pairs", "n_single_ends", "n_unmatched_pairs", "n_duplicates",
                                           "inflated_bytes", "stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("n_sort_passes", "n_batches")] +
                [(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_ends", "ms_pairing", "ms_groups", "ms_gather", "ms_deflate", "ms_total_wall")])

class MarkdupStreamStats(C.Structure):
    _fields_ = ([(k, C.c_uint32) for k in ("struct_size", "n_windows", "n_batch_runs", "n_batches_skipped")] +
                [(k, C.c_uint64) for k in ("window_bytes", "key_store_bytes", "n_key_records")] +
                [(k, C.c_double) for k in ("ms_keys", "ms_plan", "ms_scatter", "ms_inflate_replay", "ms_index_replay")])

class MergeStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records_in", "n_records_out", "n_records_rewritten")] + [("bytes_grown", C.c_int64)] +
                [(k, C.c_uint64) for k in ("inflated_bytes", "merged_stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("n_inputs", "key_bits", "n_sort_passes", "n_batches")] +
                [(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_rewrite", "ms_sort", "ms_gather", "ms_deflate", "ms_total_wall")])

class MergeWindowStats(C.Structure):
    _fields_ = ([(k, C.c_uint32) for k in ("struct_size", "n_windows", "n_batch_runs", "n_batches_skipped", "n_input_opens")] +
                [("window_bytes", C.c_uint64)] +
                [(k, C.c_double) for k in ("ms_dest", "ms_scatter", "ms_inflate_replay", "ms_index_replay")])

class ViewOpts(C.Structure):
    _fields_ = [("flags_set", C.c_uint16), ("flags_unset", C.c_uint16), ("subsample", C.c_int32), ("fraction", C.c_double), ("seed", C.c_uint64)]

class ViewStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records_in", "n_records_selected", "n_entries_out", "inflated_bytes", "stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("n_regions", "n_sort_passes", "n_batches", "reserved")] +
                [(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_select", "ms_emit", "ms_sort", "ms_gather", "ms_deflate", "ms_total_wall")])

VIEW_SINKS = {"count": 0, "bam": 1, "sam": 2}


class ViewRequest(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("sink", C.c_int32), ("in_path", C.c_char_p), ("out_path", C.c_char_p),
                ("filter", C.POINTER(Filter)), ("opts", C.POINTER(ViewOpts)), ("regions", C.POINTER(C.c_char_p)), ("n_regions", C.c_size_t),
                ("bed_path", C.c_char_p), ("pg_command_line", C.c_char_p), ("level", C.c_int32), ("with_index", C.c_int32),
                ("with_header", C.c_int32), ("device", C.c_int32), ("valid_only", C.c_int32), ("reserved", C.c_int32)]


VALIDATE_CLASSES = ("name-empty", "name-chars", "position", "qualities", "cigar-hard", "cigar-soft", "cigar-length", "tag-value",
                    "tag-duplicate", "malformed")


class ValidateReport(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_invalid", C.c_uint64), ("class_count", C.c_uint64 * len(VALIDATE_CLASSES)),
                ("first_ordinal", C.c_uint64), ("first_mask", C.c_uint32), ("first_name_len", C.c_uint32), ("first_name", C.c_char * 256)]


class ValidateStats(C.Structure):
    _fields_ = ([(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_valid", "ms_total_wall")] + [("inflated_bytes", C.c_uint64)] +
                [(k, C.c_uint32) for k in ("n_batches", "reserved")])

class SliceStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_regions", "records_r1", "blocks_inflated", "blocks_copied", "bytes_copied", "stream_bytes",
                                           "compressed_bytes")] +
                [(k, C.c_double) for k in ("ms_read", "ms_select", "ms_write", "ms_total_wall")])

class ImportStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_lines", "n_records", "text_bytes", "stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("n_chunks", "reserved")] +
                [(k, C.c_double) for k in ("ms_index", "ms_measure", "ms_emit", "ms_deflate", "ms_total_wall")])

class FixbinsStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records", "n_bins_changed", "inflated_bytes", "stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("n_batches", "reserved")] +
                [(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_bins", "ms_gather", "ms_deflate", "ms_total_wall")])

class FastaStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_sequences", "n_lines", "n_bytes")] +
                [(k, C.c_uint32) for k in ("n_chunks", "reserved")] +
                [(k, C.c_double) for k in ("ms_lines", "ms_segments", "ms_total_wall")])

class ViewIndexStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("blocks_in_file", "blocks_read", "runs", "compressed_bytes_read", "inflated_bytes_read")] +
                [("ms_plan", C.c_double)])

class StreamStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("window_bytes", "n_pack_launches")] + [(k, C.c_uint32) for k in ("n_windows", "reserved")] +
                [("ms_pack", C.c_double)])

class SubsampleStats(C.Structure):
    _fields_ = ([(k, C.c_uint64) for k in ("n_records", "n_counted", "n_over", "n_dropped", "n_written", "max_cov_seen", "cov_array_bytes",
                                           "inflated_bytes", "stream_bytes", "compressed_bytes")] +
                [(k, C.c_uint32) for k in ("n_batches", "reserved")] +
                [(k, C.c_double) for k in ("ms_inflate", "ms_index", "ms_mark", "ms_scan", "ms_verdict", "ms_deflate", "ms_total_wall")])

STREAM_KEYS = ("n_windows", "window_bytes", "n_pack_launches", "ms_pack")

VIEW_INDEX_MODES = {False: 0, True: 1, "auto": 2}       # SBX_VIEW_INDEX_OFF / _REQUIRED / _AUTO

WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_size_t)

EXPORTS = [
    "sbx_abi_sizeof", "sbx_bgzf_compress", "sbx_write_bam", "sbx_build_index", "sbx_run_interval", "sbx_run_interval_owned", "sbx_prefetch_interval", "sbx_depth_base_tile_device", "sbx_parse_regions", "sbx_parsed_regions", "sbx_parsed_region_line", "sbx_inflate_blocks", "sbx_open", "sbx_close", "sbx_last_error", "sbx_header", "sbx_ref_name", "sbx_ref_length",
    "sbx_ref_id", "sbx_sample_name", "sbx_header_text", "sbx_compile_filter", "sbx_set_filter", "sbx_regex_search", "sbx_set_params",
    "sbx_set_regions", "sbx_run", "sbx_depth_base_tile", "sbx_depth_region_stats", "sbx_depth_region_stats_from",
    "sbx_depth_window_stats",
    "sbx_format_base_rows", "sbx_stream_base_rows", "sbx_plan_batches", "sbx_run_batch", "sbx_last_run_stats", "sbx_tile_info", "sbx_next_active_range", "sbx_preload",
    "sbx_device_count", "sbx_plan_shards", "sbx_format_base_rows_device", "sbx_flagstat", "sbx_format_flagstat",
    "sbx_sort_bam", "sbx_sort_bam_by_name", "sbx_sort_header_text", "sbx_markdup", "sbx_markdup_run", "sbx_markdup_header_text",
    "sbx_merge_bam", "sbx_merge_bam_run", "sbx_merge_header_text",
    "sbx_view_count", "sbx_view_bam", "sbx_view_sam", "sbx_view_run", "sbx_view_run_indexed", "sbx_view_run_streamed", "sbx_view_num_filter", "sbx_view_reference_info",
    "sbx_validate_bam", "sbx_format_validate_report",
    "sbx_slice_bam",
    "sbx_import_sam", "sbx_import_sam_run",
    "sbx_index_bam", "sbx_fixbins", "sbx_fixbins_run", "sbx_index_fasta",
    "sbx_subsample",
]

_lib = None


def lib_path():
    return _LIB_PATH


def cli_path():
    return _CLI_PATH


def flagstat_cli_path():
    return _FLAGSTAT_CLI_PATH


def sort_cli_path():
    return _SORT_CLI_PATH


def markdup_cli_path():
    return _MARKDUP_CLI_PATH


def merge_cli_path():
    return _MERGE_CLI_PATH


def view_cli_path():
    return _VIEW_CLI_PATH


def slice_cli_path():
    return _SLICE_CLI_PATH


def sam_cli_path():
    return _SAM_CLI_PATH


def nsort_cli_path():
    return _NSORT_CLI_PATH


def iview_cli_path():
    return _IVIEW_CLI_PATH


def import_cli_path():
    return _IMPORT_CLI_PATH


def index_cli_path():
    return _INDEX_CLI_PATH


def fixbins_cli_path():
    return _FIXBINS_CLI_PATH


def validate_cli_path():
    return _VALIDATE_CLI_PATH


def subsample_cli_path():
    return _SUBSAMPLE_CLI_PATH


def lib():
    """Load libsbx_depth.so; raises if it has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError("libsbx_depth.so is missing at %s -- run `python -m sambamba_amd.build` "
                          "(the HIP library is the product; there is no CPU fallback)" % _LIB_PATH)
    L = C.CDLL(_LIB_PATH)
    u8p, u32p, u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.sbx_inflate_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                     C.c_char_p, C.c_size_t]
    L.sbx_inflate_blocks.restype = C.c_int
    L.sbx_open.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.sbx_open.restype = C.c_void_p
    L.sbx_close.argtypes = [C.c_void_p]
    L.sbx_close.restype = None
    L.sbx_last_error.argtypes = [C.c_void_p]
    L.sbx_last_error.restype = C.c_char_p
    L.sbx_header.argtypes = [C.c_void_p, C.POINTER(HeaderInfo)]
    L.sbx_ref_name.argtypes = [C.c_void_p, C.c_int]
    L.sbx_ref_name.restype = C.c_char_p
    L.sbx_ref_length.argtypes = [C.c_void_p, C.c_int]
    L.sbx_ref_length.restype = C.c_int64
    L.sbx_ref_id.argtypes = [C.c_void_p, C.c_char_p]
    L.sbx_sample_name.argtypes = [C.c_void_p, C.c_int]
    L.sbx_sample_name.restype = C.c_char_p
    L.sbx_header_text.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    L.sbx_header_text.restype = C.c_char_p
    L.sbx_compile_filter.argtypes = [C.c_char_p, C.POINTER(Filter), C.c_char_p, C.c_size_t]
    L.sbx_set_filter.argtypes = [C.c_void_p, C.POINTER(Filter)]
    L.sbx_set_params.argtypes = [C.c_void_p, C.c_int, C.c_uint8, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int]
    L.sbx_set_regions.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.sbx_run.argtypes = [C.c_void_p]
    L.sbx_depth_base_tile.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.sbx_depth_region_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sbx_depth_window_stats.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    L.sbx_format_base_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_int,
                                       C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_stream_base_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_int, WRITE_FN, C.c_void_p]
    L.sbx_plan_batches.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_run_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    L.sbx_last_run_stats.argtypes = [C.c_void_p, C.POINTER(RunStats)]
    L.sbx_tile_info.argtypes = [C.c_void_p, u32p, u32p]
    L.sbx_next_active_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, u64p, u64p]
    L.sbx_preload.argtypes = [C.c_void_p]
    L.sbx_format_base_rows_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_int, C.c_void_p,
                                              C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_device_count.argtypes = []
    L.sbx_plan_shards.argtypes = [C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_run_interval.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.sbx_bgzf_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    L.sbx_write_bam.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.sbx_build_index.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.sbx_flagstat.argtypes = [C.c_char_p, C.c_int, C.POINTER(Flagstat), C.c_char_p, C.c_size_t]
    L.sbx_format_flagstat.argtypes = [C.POINTER(Flagstat), C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_sort_bam.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Filter), C.c_int, C.c_int, C.c_int, C.POINTER(SortStats), C.c_char_p, C.c_size_t]
    L.sbx_sort_bam_by_name.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Filter), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(SortStats), C.c_char_p,
                                       C.c_size_t]
    L.sbx_sort_header_text.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_markdup.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(MarkdupStats), C.c_char_p, C.c_size_t]
    L.sbx_markdup_run.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(MarkdupStats),
                                  C.POINTER(MarkdupStreamStats), C.c_char_p, C.c_size_t]
    L.sbx_markdup_header_text.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_merge_bam.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(Filter), C.c_int, C.c_int, C.c_int, C.POINTER(MergeStats),
                                C.c_char_p, C.c_size_t]
    L.sbx_merge_bam_run.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(Filter), C.c_int, C.c_int, C.c_int, C.POINTER(MergeStats),
                                    C.POINTER(MergeWindowStats), C.c_char_p, C.c_size_t]
    L.sbx_merge_header_text.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_view_count.argtypes = [C.c_char_p, C.POINTER(Filter), C.POINTER(ViewOpts), C.POINTER(C.c_char_p), C.c_size_t, C.c_char_p, C.c_int,
                                 C.POINTER(C.c_uint64), C.POINTER(ViewStats), C.c_char_p, C.c_size_t]
    L.sbx_view_bam.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Filter), C.POINTER(ViewOpts), C.POINTER(C.c_char_p), C.c_size_t, C.c_char_p, C.c_char_p,
                               C.c_int, C.c_int, C.c_int, C.POINTER(ViewStats), C.c_char_p, C.c_size_t]
    L.sbx_view_sam.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(Filter), C.POINTER(ViewOpts), C.POINTER(C.c_char_p), C.c_size_t, C.c_char_p, C.c_char_p,
                               C.c_int, C.c_int, C.POINTER(ViewStats), C.c_char_p, C.c_size_t]
    L.sbx_view_run.argtypes = [C.POINTER(ViewRequest), C.POINTER(C.c_uint64), C.POINTER(ViewStats), C.c_char_p, C.c_size_t]
    L.sbx_view_run_indexed.argtypes = [C.POINTER(ViewRequest), C.c_int, C.POINTER(C.c_uint64), C.POINTER(ViewStats), C.POINTER(ViewIndexStats),
                                       C.c_char_p, C.c_size_t]
    L.sbx_view_run_streamed.argtypes = [C.POINTER(ViewRequest), C.c_int, C.POINTER(C.c_uint64), C.POINTER(ViewStats), C.POINTER(ViewIndexStats),
                                        C.POINTER(StreamStats), C.c_char_p, C.c_size_t]
    L.sbx_validate_bam.argtypes = [C.c_char_p, C.c_int, C.POINTER(ValidateReport), C.POINTER(ValidateStats), C.c_char_p, C.c_size_t]
    L.sbx_format_validate_report.argtypes = [C.c_char_p, C.POINTER(ValidateReport), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_view_num_filter.argtypes = [C.c_char_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]
    L.sbx_view_reference_info.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.sbx_slice_bam.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), C.c_size_t, C.c_char_p, C.c_int, C.POINTER(SliceStats), C.c_char_p,
                                C.c_size_t]
    L.sbx_import_sam.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(ImportStats), C.c_char_p, C.c_size_t]
    L.sbx_import_sam_run.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(ImportStats), C.POINTER(StreamStats),
                                     C.c_char_p, C.c_size_t]
    L.sbx_index_bam.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.sbx_fixbins.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(FixbinsStats), C.c_char_p, C.c_size_t]
    L.sbx_fixbins_run.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(FixbinsStats), C.POINTER(StreamStats), C.c_char_p, C.c_size_t]
    L.sbx_subsample.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(SubsampleStats),
                                C.POINTER(StreamStats), C.c_char_p, C.c_size_t]
    L.sbx_index_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(FastaStats), C.c_char_p, C.c_size_t]
    L.sbx_prefetch_interval.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.sbx_run_interval_owned.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.sbx_depth_base_tile_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.sbx_parse_regions.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.sbx_parsed_regions.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.sbx_parsed_region_line.argtypes = [C.c_void_p, C.c_size_t]
    L.sbx_parsed_region_line.restype = C.c_char_p
    L.sbx_abi_sizeof.argtypes = [C.c_char_p]
    L.sbx_abi_sizeof.restype = C.c_size_t
    L.sbx_depth_region_stats_from.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sbx_regex_search.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    # the structures above must have the layout the library was compiled with
    for name, ty in (("sbx_region", Region), ("sbx_header_info", HeaderInfo), ("sbx_region_stats", RegionStats),
                     ("sbx_filter_op", FilterOp), ("sbx_regex_state", RegexState), ("sbx_regex", Regex), ("sbx_filter", Filter),
                     ("sbx_run_stats", RunStats), ("sbx_batch", Batch), ("sbx_flagstat_counts", Flagstat),
                     ("sbx_sort_stats", SortStats), ("sbx_markdup_stats", MarkdupStats), ("sbx_markdup_stream_stats", MarkdupStreamStats),
                     ("sbx_merge_stats", MergeStats), ("sbx_merge_window_stats", MergeWindowStats),
                     ("sbx_view_opts", ViewOpts), ("sbx_view_stats", ViewStats), ("sbx_import_stats", ImportStats),
                     ("sbx_fixbins_stats", FixbinsStats), ("sbx_fasta_stats", FastaStats), ("sbx_slice_stats", SliceStats),
                     ("sbx_view_request", ViewRequest), ("sbx_validate_report", ValidateReport), ("sbx_validate_stats", ValidateStats),
                     ("sbx_view_index_stats", ViewIndexStats), ("sbx_stream_stats", StreamStats),
                     ("sbx_subsample_stats", SubsampleStats)):
        if L.sbx_abi_sizeof(name.encode()) != C.sizeof(ty):
            raise ImportError("ctypes layout of %s (%d bytes) differs from libsbx_depth.so (%d bytes)" % (
                name, C.sizeof(ty), L.sbx_abi_sizeof(name.encode())))
    _lib = L
    return L


def inflate_blocks(comp, comp_off, comp_len, isize, out_off, out_size):
    """sbx_inflate_blocks over numpy arrays; returns the inflated bytes (numpy uint8)."""
    L = lib()
    comp = np.ascontiguousarray(comp, dtype=np.uint8)
    comp_off = np.ascontiguousarray(comp_off, dtype=np.uint64)
    comp_len = np.ascontiguousarray(comp_len, dtype=np.uint32)
    isize = np.ascontiguousarray(isize, dtype=np.uint32)
    out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
    out = np.zeros(int(out_size), dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc = L.sbx_inflate_blocks(comp.ctypes.data, comp_off.ctypes.data, comp_len.ctypes.data, isize.ctypes.data,
                              len(comp_len), out.ctypes.data, out_off.ctypes.data, err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return out


def bgzf_compress(data, level=6, with_eof=True, device=-1):
    """sbx_bgzf_compress: the BGZF stream (bytes) of `data`, compressed on the device."""
    L = lib()
    src = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    cap = len(src) + len(src) // 2048 + 64 + 28 + 31
    out = np.empty(cap, dtype=np.uint8)
    n = C.c_size_t(0)
    err = C.create_string_buffer(512)
    rc = L.sbx_bgzf_compress(src.ctypes.data if len(src) else None, len(src), int(level), int(with_eof), device, out.ctypes.data, cap, C.byref(n), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return out[:n.value].tobytes()


def write_bam(path, stream, level=6, with_index=True, device=-1):
    """sbx_write_bam: the uncompressed BAM byte stream `stream` as a BGZF file (+ .bai)."""
    L = lib()
    src = np.frombuffer(bytes(stream), dtype=np.uint8)
    err = C.create_string_buffer(512)
    rc = L.sbx_write_bam(path.encode(), src.ctypes.data, len(src), int(level), int(with_index), device, err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())


def build_index(bam_path, bai_path=None, device=-1, check_bins=False):
    """sbx_build_index (`sambamba index`): writes bai_path (default: bam_path + ".bai").  check_bins=True is `index -c`
    (sbx_index_bam): a placed record whose stored bin is not reg2bin of its position and CIGAR raises SbxError(-3) with the
    reference's message for the first such record and their number, and no index is written."""
    L = lib()
    err = C.create_string_buffer(512)
    out = (bai_path or bam_path + ".bai").encode()
    if check_bins:
        rc = L.sbx_index_bam(bam_path.encode(), out, 1, device, err, 512)
    else:
        rc = L.sbx_build_index(bam_path.encode(), out, device, err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())


def fixbins(in_path, out_path, level=-1, device=-1):
    """sbx_fixbins (`sambamba fixbins`): in_path written to out_path with the bin of every record set to reg2bin of its position and
    CIGAR; nothing else changes.  Returns the fields of sbx_fixbins_stats as a dict, plus n_windows, window_bytes, n_pack_launches and
    ms_pack of sbx_stream_stats: zeros when the records stayed on the device, the figures of the streamed path when they did not fit
    (or SBX_STREAM_WINDOW_BYTES is set)."""
    L = lib()
    st = FixbinsStats()
    ss = StreamStats()
    err = C.create_string_buffer(512)
    rc = L.sbx_fixbins_run(in_path.encode(), out_path.encode(), int(level), device, C.byref(st), C.byref(ss), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    out = {k: getattr(st, k) for k, _ in FixbinsStats._fields_ if k != "reserved"}
    out.update({k: getattr(ss, k) for k in STREAM_KEYS})
    return out


def subsample(in_path, out_path, max_cov, *, remove=False, level=-1, index=False, command_line=None, device=-1):
    """sbx_subsample (`sambamba subsample --type fasthash --max-cov N [-r]`): in_path written to out_path in file order with the
    coverage capped at about max_cov.  The coverage is counted over the whole file from the records that are mapped, pass QC and are
    no duplicates; such a record whose coverage (the larger of that at its first and at its last position) exceeds max_cov is kept
    with probability max_cov / coverage, decided by a hash of its name -- so mates share the hash, not necessarily the verdict.
    remove=True leaves the dropped records out; otherwise they are written with flag bit 0x200 set.  command_line: the CL of the @PG
    line (None: no @PG line); index=True also writes out_path + ".bai".  Returns the fields of sbx_subsample_stats as a dict, plus
    n_windows, window_bytes, n_pack_launches and ms_pack of sbx_stream_stats (the output is always streamed)."""
    L = lib()
    st = SubsampleStats()
    ss = StreamStats()
    err = C.create_string_buffer(1024)
    cl = command_line.encode() if command_line is not None else None
    rc = L.sbx_subsample(in_path.encode(), out_path.encode(), int(max_cov), int(bool(remove)), int(level), int(bool(index)), cl, device,
                         C.byref(st), C.byref(ss), err, 1024)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    out = {k: getattr(st, k) for k, _ in SubsampleStats._fields_ if k != "reserved"}
    out.update({k: getattr(ss, k) for k in STREAM_KEYS})
    return out


def index_fasta(path, fai_path=None, device=-1):
    """sbx_index_fasta (`sambamba index -F`): the .fai of the FASTA file at `path` (default: path + ".fai"), its lines found and
    added up on the device.  Returns the fields of sbx_fasta_stats as a dict."""
    L = lib()
    st = FastaStats()
    err = C.create_string_buffer(512)
    rc = L.sbx_index_fasta(path.encode(), (fai_path or path + ".fai").encode(), device, C.byref(st), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return {k: getattr(st, k) for k, _ in FastaStats._fields_ if k != "reserved"}


def flagstat(path, device=-1):
    """sbx_flagstat (`sambamba flagstat`): {counter: (QC-passed, QC-failed)} over every record of the BAM, counted on the device."""
    L = lib()
    f = Flagstat()
    err = C.create_string_buffer(512)
    rc = L.sbx_flagstat(path.encode(), device, C.byref(f), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return {k: (int(getattr(f, k)[0]), int(getattr(f, k)[1])) for k in FLAGSTAT_FIELDS}


def format_flagstat(counts, tabular=False):
    """sbx_format_flagstat: the text `sambamba flagstat` prints for `counts` (as flagstat() returns them), host only."""
    L = lib()
    f = Flagstat()
    for k in FLAGSTAT_FIELDS:
        getattr(f, k)[0], getattr(f, k)[1] = counts[k]
    n = C.c_size_t(0)
    L.sbx_format_flagstat(C.byref(f), int(tabular), None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value + 1)
    rc = L.sbx_format_flagstat(C.byref(f), int(tabular), buf, n.value + 1, C.byref(n))
    if rc != 0:
        raise SbxError(rc, "sbx_format_flagstat failed")
    return buf.raw[:n.value].decode()


SORT_ORDERS = {"coordinate": 0, "queryname": 1, "natural": 2}


def sort_bam(in_path, out_path, filter=None, level=-1, index=False, device=-1, order="coordinate", match_mates=False):
    """sbx_sort_bam (`sambamba sort`): sorts in_path into out_path on the device; filter is a -F query string (None: every record);
    index=True also writes out_path + ".bai".  order: "coordinate", or through sbx_sort_bam_by_name "queryname" (sort -n: names as
    bytes) or "natural" (sort -N: digit runs as numbers); match_mates (sort -M, name orders only): equal names by HI tag, then flag.
    Returns the fields of sbx_sort_stats as a dict."""
    if order not in SORT_ORDERS:
        raise ValueError("order must be one of coordinate, queryname, natural")
    by_name = SORT_ORDERS[order]
    if by_name and index:
        raise ValueError("a BAM sorted by name has no index")
    if match_mates and not by_name:
        raise ValueError("match_mates only works with order queryname or natural")
    L = lib()
    f = compile_filter(filter) if filter else None
    st = SortStats()
    err = C.create_string_buffer(512)
    fp = C.byref(f) if f is not None else None
    if by_name:
        rc = L.sbx_sort_bam_by_name(in_path.encode(), out_path.encode(), fp, int(level), by_name, int(bool(match_mates)), device, C.byref(st), err, 512)
    else:
        rc = L.sbx_sort_bam(in_path.encode(), out_path.encode(), fp, int(level), int(index), device, C.byref(st), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return {k: getattr(st, k) for k, _ in SortStats._fields_ if k != "reserved"}


def sort_header_text(text):
    """sbx_sort_header_text: the header text `sambamba sort` writes for the input header text (str or bytes -> same type), host only."""
    L = lib()
    data = text if isinstance(text, bytes) else text.encode()
    n = C.c_size_t(0)
    rc = L.sbx_sort_header_text(data, len(data), None, 0, C.byref(n))
    if rc not in (0, -8):
        raise SbxError(rc, "malformed SAM header text")
    buf = C.create_string_buffer(n.value + 1)
    rc = L.sbx_sort_header_text(data, len(data), buf, n.value + 1, C.byref(n))
    if rc != 0:
        raise SbxError(rc, "sbx_sort_header_text failed")
    out = buf.raw[:n.value]
    return out if isinstance(text, bytes) else out.decode()


def markdup(in_path, out_path, remove_duplicates=False, level=-1, command_line=None, device=-1):
    """sbx_markdup (`sambamba markdup`): marks (remove_duplicates: removes) the duplicates of in_path into out_path on the device;
    command_line is the CL field of the @PG line that is added (None: no @PG).  Returns the fields of sbx_markdup_stats as a dict,
    plus n_windows, n_batch_runs, window_bytes and key_store_bytes of sbx_markdup_stream_stats: zeros when the records stayed on the
    device, the figures of the streamed path when they did not fit (or SBX_MARKDUP_WINDOW_BYTES is set)."""
    L = lib()
    st = MarkdupStats()
    ss = MarkdupStreamStats()
    ss.struct_size = C.sizeof(MarkdupStreamStats)
    err = C.create_string_buffer(512)
    rc = L.sbx_markdup_run(in_path.encode(), out_path.encode(), int(bool(remove_duplicates)), int(level),
                           command_line.encode() if command_line is not None else None, device, C.byref(st), C.byref(ss), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    out = {k: getattr(st, k) for k, _ in MarkdupStats._fields_}
    out.update({k: getattr(ss, k) for k in ("n_windows", "n_batch_runs", "window_bytes", "key_store_bytes")})
    return out


def markdup_header_text(text, command_line=None):
    """sbx_markdup_header_text: the header text `sambamba markdup` writes for the input header text (str or bytes -> same type), host only."""
    L = lib()
    data = text if isinstance(text, bytes) else text.encode()
    cl = command_line.encode() if command_line is not None else None
    n = C.c_size_t(0)
    rc = L.sbx_markdup_header_text(data, len(data), cl, None, 0, C.byref(n))
    if rc not in (0, -8):
        raise SbxError(rc, "malformed SAM header text")
    buf = C.create_string_buffer(n.value + 1)
    rc = L.sbx_markdup_header_text(data, len(data), cl, buf, n.value + 1, C.byref(n))
    if rc != 0:
        raise SbxError(rc, "sbx_markdup_header_text failed")
    out = buf.raw[:n.value]
    return out if isinstance(text, bytes) else out.decode()


def regex_search(pattern, text, options=""):
    """Host-side evaluation of `text =~ /pattern/options` with the NFA the device runs (sbx_regex_search)."""
    L = lib()
    L.sbx_regex_search.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    err = C.create_string_buffer(512)
    data = text if isinstance(text, bytes) else text.encode()
    rc = L.sbx_regex_search(pattern.encode(), options.encode(), data, len(data), err, 512)
    if rc < 0:
        raise SbxError(rc, err.value.decode())
    return bool(rc)


def compile_filter(query):
    f = Filter()
    err = C.create_string_buffer(512)
    rc = lib().sbx_compile_filter(query.encode() if query is not None else None, C.byref(f), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return f


class Depth:
    """Thin object wrapper over an sbx_ctx (one BAM or a list of BAMs, one device)."""

    def __init__(self, bam_path, device=-1):
        self._L = lib()
        paths = [bam_path] if isinstance(bam_path, str) else list(bam_path)
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        err = C.create_string_buffer(1024)
        self._ctx = self._L.sbx_open(arr, len(paths), device, err, 1024)
        if not self._ctx:
            raise SbxError(-1, err.value.decode())
        hi = HeaderInfo()
        self._check(self._L.sbx_header(self._ctx, C.byref(hi)))
        self.info = hi
        self.ref_names = [self._L.sbx_ref_name(self._ctx, i).decode() for i in range(hi.n_ref)]
        self.ref_lengths = [self._L.sbx_ref_length(self._ctx, i) for i in range(hi.n_ref)]
        self.sample_names = [self._L.sbx_sample_name(self._ctx, i).decode() for i in range(hi.n_samples)]
        self.n_samples_eff = hi.n_samples

    def _check(self, rc):
        if rc != 0:
            raise SbxError(rc, self._L.sbx_last_error(self._ctx).decode())

    def close(self):
        if self._ctx:
            self._L.sbx_close(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_filter(self, query):
        f = compile_filter(query)
        self._check(self._L.sbx_set_filter(self._ctx, C.byref(f)))

    def set_params(self, mode=SBX_MODE_BASE, min_bq=0, fix_mate_overlaps=False, combined=False, window=0, overlap=0,
                   thresholds=()):
        thr = np.asarray(list(thresholds), dtype=np.uint32)
        self._check(self._L.sbx_set_params(self._ctx, mode, min_bq, int(fix_mate_overlaps), int(combined), window, overlap,
                                           thr.ctypes.data if len(thr) else None, len(thr)))
        self.n_samples_eff = 1 if combined else self.info.n_samples

    def set_regions(self, regions):
        arr = (Region * len(regions))(*[Region(*r) for r in regions])
        self._check(self._L.sbx_set_regions(self._ctx, arr, len(regions)))

    def parse_regions(self, arg):
        """-L argument (BED file or region string) -> (merged [(ref, start, end)], raw [(ref, start, end)], raw input lines),
        parsed by the library exactly as the CLI parses it."""
        nm, nr = C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.sbx_parse_regions(self._ctx, arg.encode(), C.byref(nm), C.byref(nr)))
        out = []
        for merged, n in ((1, nm.value), (0, nr.value)):
            arr = (Region * max(1, n))()
            self._check(self._L.sbx_parsed_regions(self._ctx, merged, arr, n))
            out.append([(arr[i].ref_id, arr[i].start, arr[i].end) for i in range(n)])
        lines = [self._L.sbx_parsed_region_line(self._ctx, i).decode() for i in range(nr.value)]
        return out[0], out[1], lines

    def preload(self):
        self._check(self._L.sbx_preload(self._ctx))

    def run(self):
        self._check(self._L.sbx_run(self._ctx))
        st = RunStats()
        self._check(self._L.sbx_last_run_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    def region_stats(self, regions, n_thresholds=0):
        """sbx_depth_region_stats: returns (n_reads[n][S], n_bases[n][S], cov[n][S][n_thr], seen[n])."""
        n, S = len(regions), self.n_samples_eff
        # a uint32 array [n][3] (ref_id, start, end) is the sbx_region layout itself: passed as is (200,000 BED lines cost
        # 0.2 s per call as a list of ctypes structures)
        arr = np.ascontiguousarray(regions, dtype=np.uint32).reshape(n, 3) if n else np.zeros((1, 3), dtype=np.uint32)
        st = np.zeros((n, S, 2), dtype=np.uint32)
        cov = np.zeros((n, S, max(1, n_thresholds)), dtype=np.uint32)
        seen = np.zeros(n, dtype=np.uint8)
        self._check(self._L.sbx_depth_region_stats(self._ctx, arr.ctypes.data, n, st.ctypes.data, cov.ctypes.data, seen.ctypes.data))
        return st[:, :, 0].copy(), st[:, :, 1].copy(), cov[:, :, :n_thresholds].copy(), seen

    def window_stats(self, ref_id, first, count, n_thresholds=0):
        S = self.n_samples_eff
        st = np.zeros((count, S, 2), dtype=np.uint32)
        cov = np.zeros((count, S, max(1, n_thresholds)), dtype=np.uint32)
        self._check(self._L.sbx_depth_window_stats(self._ctx, ref_id, first, count, st.ctypes.data, cov.ctypes.data))
        return st[:, :, 0].copy(), st[:, :, 1].copy(), cov[:, :, :n_thresholds].copy()

    def plan_batches(self, budget_bytes=0):
        """[(first_ref, n_refs, est_bytes)]: consecutive batches of contigs that fit the device (sbx_plan_batches)."""
        n = C.c_size_t(0)
        self._check(self._L.sbx_plan_batches(self._ctx, int(budget_bytes), None, 0, C.byref(n)))
        arr = (Batch * max(1, n.value))()
        self._check(self._L.sbx_plan_batches(self._ctx, int(budget_bytes), arr, n.value, C.byref(n)))
        return [(arr[i].first_ref, arr[i].n_refs, arr[i].est_bytes) for i in range(n.value)]

    def run_batch(self, first_ref, n_refs):
        """sbx_run restricted to the reads of contigs [first_ref, first_ref + n_refs)."""
        self._check(self._L.sbx_run_batch(self._ctx, int(first_ref), int(n_refs)))
        st = RunStats()
        self._check(self._L.sbx_last_run_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    def run_interval(self, ref_id, beg, end):
        """sbx_run restricted to the reads overlapping [beg, end) of ref_id (position sharding / streaming)."""
        self._check(self._L.sbx_run_interval(self._ctx, int(ref_id), int(beg), int(end)))
        st = RunStats()
        self._check(self._L.sbx_last_run_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    def run_interval_owned(self, ref_id, beg, end):
        """sbx_run_interval_owned: only the reads whose leftmost position lies in [beg, end), counted over all they cover."""
        self._check(self._L.sbx_run_interval_owned(self._ctx, int(ref_id), int(beg), int(end)))
        st = RunStats()
        self._check(self._L.sbx_last_run_stats(self._ctx, C.byref(st)))
        return st.as_dict()

    def base_counters_to_device(self, ref_id, beg, end, device_ptr):
        """sbx_depth_base_tile_device: counters of [beg, end) into device memory ((end - beg) * S * 7 uint32 at device_ptr)."""
        self._check(self._L.sbx_depth_base_tile_device(self._ctx, int(ref_id), int(beg), int(end), C.c_void_p(int(device_ptr))))

    def measure_base_rows(self, ref_id, beg, end, min_cov=1.0, max_cov=float("inf"), annotate=False):
        """Bytes of the text of [beg, end) (the device's measuring pass alone; nothing is copied)."""
        need = C.c_size_t(0)
        rc = self._L.sbx_format_base_rows(self._ctx, ref_id, beg, end, float(min_cov), float(max_cov), int(annotate), None, 0, C.byref(need))
        if rc != 0 and rc != ENOMEM:
            self._check(rc)
        return int(need.value)

    def format_base_rows_to_device(self, ref_id, beg, end, device_ptr, cap, min_cov=1.0, max_cov=float("inf"), annotate=False):
        """sbx_format_base_rows_device: the text of [beg, end) into device memory at device_ptr (cap bytes); returns its size."""
        need = C.c_size_t(0)
        self._check(self._L.sbx_format_base_rows_device(self._ctx, ref_id, beg, end, float(min_cov), float(max_cov), int(annotate),
                                                        C.c_void_p(int(device_ptr)) if device_ptr else None, int(cap), C.byref(need)))
        return int(need.value)

    def format_base_rows(self, ref_id, beg, end, min_cov=1.0, max_cov=float("inf"), annotate=False):
        """Text of `depth base` for [beg, end) of ref_id, formatted on the device (bytes)."""
        need = C.c_size_t(0)
        cap = max(1 << 16, (end - beg) * 40 * self.n_samples_eff)
        for _ in range(2):
            buf = C.create_string_buffer(cap)
            rc = self._L.sbx_format_base_rows(self._ctx, ref_id, beg, end, float(min_cov), float(max_cov), int(annotate),
                                              buf, cap, C.byref(need))
            if rc == ENOMEM and need.value > cap:
                cap = need.value
                continue
            self._check(rc)
            return buf.raw[:need.value]
        self._check(rc)

    def stream_base_rows(self, ref_id, beg, end, write, min_cov=1.0, max_cov=float("inf"), annotate=False):
        """sbx_stream_base_rows: `write(bytes)` is called with consecutive pieces of the text of [beg, end)."""
        def cb(_user, data, n):
            try:
                write(C.string_at(data, n))
                return 0
            except Exception:       # the library turns it into SBX_EIO
                return 1
        fn = WRITE_FN(cb)
        self._check(self._L.sbx_stream_base_rows(self._ctx, ref_id, beg, end, float(min_cov), float(max_cov), int(annotate), fn, None))

    def next_active_range(self, ref_id, start):
        """[beg, end) of the next stretch of tiles at or after `start` that hold admitted reads, or None (sbx_next_active_range)."""
        b, e = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.sbx_next_active_range(self._ctx, ref_id, int(start), C.byref(b), C.byref(e)))
        if b.value == 0xFFFFFFFFFFFFFFFF:
            return None
        return int(b.value), int(e.value)

    def active_end(self, ref_id):
        """End of the last stretch of tiles of ref_id that hold admitted reads after the last run, or 0: beyond the contig's length
        when alignments hang over its end (the engine lays out as many spare tiles as they need)."""
        end, at = 0, 0
        while True:
            r = self.next_active_range(ref_id, at)
            if r is None:
                return end
            end = at = r[1]

    def covered(self, ref_id, beg, end):
        """One byte per position of [beg, end): non-zero iff a pileup column exists there (available after every kind of run)."""
        cov = np.zeros(end - beg, dtype=np.uint8)
        self._check(self._L.sbx_depth_base_tile(self._ctx, ref_id, beg, end, None, cov.ctypes.data))
        return cov

    def base_counters(self, ref_id, beg, end, with_covered=False):
        S = self.n_samples_eff
        out = np.zeros((end - beg, S, NCOUNTERS), dtype=np.uint32)
        cov = np.zeros(end - beg, dtype=np.uint8) if with_covered else None
        self._check(self._L.sbx_depth_base_tile(self._ctx, ref_id, beg, end, out.ctypes.data,
                                                cov.ctypes.data if with_covered else None))
        return (out, cov) if with_covered else out


def merge(out_path, inputs, filter=None, level=-1, index=False, device=-1):
    """sbx_merge_bam (`sambamba merge`): merges the coordinate-sorted BAMs `inputs` into out_path on the device; filter is a -F query
    string (None: every record); index=True also writes out_path + ".bai".  Returns the fields of sbx_merge_stats as a dict, plus
    those of sbx_merge_window_stats but struct_size (n_windows, n_batch_runs, n_batches_skipped, n_input_opens, window_bytes and
    the four times): zeros when the records of all inputs stayed on the device, the figures of the windowed path when they did not
    fit (or SBX_MERGE_WINDOW_BYTES is set)."""
    L = lib()
    f = compile_filter(filter) if filter else None
    st = MergeStats()
    ws = MergeWindowStats()
    ws.struct_size = C.sizeof(MergeWindowStats)
    err = C.create_string_buffer(512)
    paths = (C.c_char_p * max(1, len(inputs)))(*[p.encode() for p in inputs])
    rc = L.sbx_merge_bam_run(out_path.encode(), paths, len(inputs), C.byref(f) if f is not None else None, int(level), int(index), device,
                             C.byref(st), C.byref(ws), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    out = {k: getattr(st, k) for k, _ in MergeStats._fields_}
    out.update({k: getattr(ws, k) for k, _ in MergeWindowStats._fields_ if k != "struct_size"})
    return out


def merge_header_text(texts):
    """sbx_merge_header_text: the header text `sambamba merge` writes for the header texts of its inputs, in input order (str or bytes
    -> the type of the first), host only.  A refusal raises SbxError with the reference's message."""
    L = lib()
    data = [t if isinstance(t, bytes) else t.encode() for t in texts]
    arr = (C.c_char_p * max(1, len(data)))(*data)
    lens = (C.c_size_t * max(1, len(data)))(*[len(d) for d in data])
    n = C.c_size_t(0)
    first = L.sbx_merge_header_text(arr, lens, len(data), None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value + 1)
    rc = L.sbx_merge_header_text(arr, lens, len(data), buf, n.value + 1, C.byref(n))
    if first not in (0, -8) or rc != 0:
        raise SbxError(rc if rc != 0 else first, buf.raw[:n.value].decode())
    out = buf.raw[:n.value]
    return out if not texts or isinstance(texts[0], bytes) else out.decode()


def view_num_filter(text):
    """sbx_view_num_filter: "i1/i2" of `view --num-filter` -> (flags_set, flags_unset), host only; SbxError(-1) for anything else."""
    L = lib()
    a, b = C.c_uint16(0), C.c_uint16(0)
    rc = L.sbx_view_num_filter(text.encode(), C.byref(a), C.byref(b))
    if rc != 0:
        raise SbxError(rc, "invalid num-filter %r" % text)
    return a.value, b.value


def view(in_path, out_path=None, *, count=False, filter=None, num_filter=None, regions=(), bed=None, subsample=None, seed=None, level=-1,
         index=False, command_line=None, device=-1, format="bam", with_header=False, valid=False, use_index=False, with_stats=False):
    """sbx_view_run (`sambamba view -c` / `-f bam` / `-f sam`): the records of in_path that pass the -F query string `filter`,
    `num_filter` ("i1/i2"), the subsampling (`subsample` = fraction, `seed` = 64-bit seed, drawn at random when None) and overlap
    `regions` ("chr", "chr:beg-end", "*": once per listed region, in listed order) or the BED file `bed` (once, in file order).
    count=True returns their number; otherwise they are written to out_path ("-": stdout) as a BAM -- index=True also writes
    out_path + ".bai", command_line is the CL field of the @PG line that is added (None: no @PG) -- and the fields of sbx_view_stats
    come back as a dict.  format="sam" writes SAM text instead, formatted on the device: one line per record, after the header text
    when with_header (`view -h`); level and index do not apply to it (ValueError).  valid=True (`view -v`): only the records validate() calls
    valid are selected.
    use_index (sbx_view_run_indexed): False reads the whole file, as ever; True reads only the blocks the .bai of in_path names for
    the regions or the BED file and fails with SBX_ENOINDEX (-7) without one; "auto" falls back to the whole file then.  The stats
    dict then also carries the fields of sbx_view_index_stats (blocks_in_file, blocks_read, runs, ...), and n_records_in counts the
    records that were described.  with_stats=True makes count=True return (count, stats dict).  The dict also carries n_windows,
    window_bytes, n_pack_launches and ms_pack of sbx_stream_stats (sbx_view_run_streamed): zeros on the resident path, the figures of
    the streamed path when a BAM or SAM output in file order did not fit the device (or SBX_STREAM_WINDOW_BYTES is set); for
    format="sam", which has no window, n_windows counts the pieces of text written and window_bytes is the piece size."""
    if use_index not in (False, True, "auto"):
        raise ValueError("view: use_index must be False, True or 'auto'")
    if format not in ("bam", "sam"):
        raise ValueError("view: format must be 'bam' or 'sam'")
    if format == "sam" and (level != -1 or index):
        raise ValueError("view: level and index do not apply to format='sam'")
    L = lib()
    f = compile_filter(filter) if filter else None
    o = ViewOpts()
    if num_filter is not None:
        o.flags_set, o.flags_unset = view_num_filter(num_filter)
    if subsample is not None:
        o.subsample, o.fraction = 1, float(subsample)
        o.seed = int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)
    regions = [regions] if isinstance(regions, str) else list(regions)
    arr = (C.c_char_p * max(1, len(regions)))(*[r.encode() for r in regions])
    st = ViewStats()
    err = C.create_string_buffer(512)
    fp = C.byref(f) if f is not None else None
    bedp = bed.encode() if bed else None
    if not count and out_path is None:
        raise ValueError("view: out_path is required unless count=True ('-' writes to stdout)")
    q = ViewRequest()
    q.struct_size = C.sizeof(ViewRequest)
    q.sink = VIEW_SINKS["count" if count else format]
    q.in_path = in_path.encode()
    q.out_path = None if count else out_path.encode()
    q.filter = C.pointer(f) if f is not None else None
    q.opts = C.pointer(o)
    q.regions, q.n_regions = arr, len(regions)
    q.bed_path = bed.encode() if bed else None
    q.pg_command_line = command_line.encode() if command_line is not None else None
    q.level, q.with_index, q.with_header, q.device = int(level), int(index), int(bool(with_header)), device
    q.valid_only = int(bool(valid))
    n = C.c_uint64(0)
    ix = ViewIndexStats()
    ss = StreamStats()
    rc = L.sbx_view_run_streamed(C.byref(q), VIEW_INDEX_MODES[use_index], C.byref(n), C.byref(st), C.byref(ix), C.byref(ss), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    stats = {k: getattr(st, k) for k, _ in ViewStats._fields_ if k != "reserved"}
    stats.update({k: getattr(ss, k) for k in STREAM_KEYS})
    if use_index is not False:
        stats.update({k: getattr(ix, k) for k, _ in ViewIndexStats._fields_})
    if count:
        return (int(n.value), stats) if with_stats else int(n.value)
    return stats


def validate(path, device=-1):
    """sbx_validate_bam (`sambamba view -v` as a report): every record of the BAM judged on the device by the reference's isValid.
    Returns n_records, n_invalid, class_count ({class name: records}; a record can be in several) and, when n_invalid > 0,
    first_invalid = {ordinal, mask, classes, name (bytes)} for the first invalid record in file order (else None), plus the fields of
    sbx_validate_stats under "stats"."""
    L = lib()
    r, st = ValidateReport(), ValidateStats()
    err = C.create_string_buffer(512)
    rc = L.sbx_validate_bam(path.encode(), device, C.byref(r), C.byref(st), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    first = None
    if r.n_invalid:
        first = {"ordinal": int(r.first_ordinal), "mask": int(r.first_mask),
                 "classes": [c for k, c in enumerate(VALIDATE_CLASSES) if r.first_mask >> k & 1],
                 "name": C.string_at(C.addressof(r) + ValidateReport.first_name.offset, r.first_name_len)}
    return {"n_records": int(r.n_records), "n_invalid": int(r.n_invalid),
            "class_count": {c: int(r.class_count[k]) for k, c in enumerate(VALIDATE_CLASSES)}, "first_invalid": first,
            "stats": {k: getattr(st, k) for k, _ in ValidateStats._fields_ if k != "reserved"}}


def format_validate_report(path, n_records, n_invalid, class_count, first_invalid=None):
    """sbx_format_validate_report: the text `sbx-validate` prints for one file (host only); the arguments as validate() returns them."""
    L = lib()
    r = ValidateReport()
    r.n_records, r.n_invalid = n_records, n_invalid
    for k, c in enumerate(VALIDATE_CLASSES):
        r.class_count[k] = class_count.get(c, 0)
    if first_invalid is not None:
        r.first_ordinal, r.first_mask, r.first_name_len = first_invalid["ordinal"], first_invalid["mask"], len(first_invalid["name"])
        C.memmove(C.addressof(r) + ValidateReport.first_name.offset, first_invalid["name"], len(first_invalid["name"]))
    n = C.c_size_t(0)
    L.sbx_format_validate_report(path.encode(), C.byref(r), None, 0, C.byref(n))
    buf = C.create_string_buffer(n.value + 1)
    rc = L.sbx_format_validate_report(path.encode(), C.byref(r), buf, n.value + 1, C.byref(n))
    if rc != 0:
        raise SbxError(rc, "sbx_format_validate_report failed")
    return buf.raw[:n.value]


def slice_bam(in_path, out_path=None, regions=(), bed=None, device=-1):
    """sbx_slice_bam (`sambamba slice`): the regions ("chr", "chr:beg-end", or "*" alone) or the BED file `bed` of the indexed BAM
    in_path copied to out_path (None or "-": stdout) -- per region the records that start in front of it and reach it, then the
    stretch of the stream from the first record at or behind its start to the first at or behind its end, with every BGZF block
    that lies wholly inside written as it is in the file.  Returns the fields of sbx_slice_stats as a dict."""
    L = lib()
    regions = [regions] if isinstance(regions, str) else list(regions)
    arr = (C.c_char_p * max(1, len(regions)))(*[r.encode() for r in regions])
    st = SliceStats()
    err = C.create_string_buffer(512)
    rc = L.sbx_slice_bam(in_path.encode(), out_path.encode() if out_path else None, arr, len(regions), bed.encode() if bed else None, device,
                         C.byref(st), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    return {k: getattr(st, k) for k, _ in SliceStats._fields_}


def import_sam(in_path, out_path, level=-1, index=False, command_line=None, device=-1):
    """sbx_import_sam (`sambamba view -S -f bam`): the SAM text at in_path ("-": stdin) parsed on the device and written to out_path
    ("-": stdout) as a BAM -- index=True also writes out_path + ".bai", command_line is the CL field of the @PG line that is added
    (None: no @PG).  A line outside the grammar raises SbxError(-3) naming how many there are and the first.  Returns the fields
    of sbx_import_stats as a dict, plus n_windows, window_bytes, n_pack_launches and ms_pack of sbx_stream_stats (sbx_import_sam_run):
    zeros when the records stayed on the device, the figures of the streamed path when they did not fit (or SBX_STREAM_WINDOW_BYTES
    or SBX_IMPORT_STORE_BYTES made it so)."""
    L = lib()
    st = ImportStats()
    ss = StreamStats()
    err = C.create_string_buffer(512)
    cl = command_line.encode() if command_line is not None else None
    rc = L.sbx_import_sam_run(in_path.encode(), out_path.encode(), cl, int(level), int(index), device, C.byref(st), C.byref(ss), err, 512)
    if rc != 0:
        raise SbxError(rc, err.value.decode())
    out = {k: getattr(st, k) for k, _ in ImportStats._fields_ if k != "reserved"}
    out.update({k: getattr(ss, k) for k in STREAM_KEYS})
    return out


def view_reference_info(path, device=-1):
    """sbx_view_reference_info: the text `sambamba view -I` prints for the BAM at `path`."""
    L = lib()
    err = C.create_string_buffer(512)
    paths = (C.c_char_p * 1)(path.encode())
    ctx = L.sbx_open(paths, 1, device, err, 512)
    if not ctx:
        raise SbxError(-2, err.value.decode())
    try:
        n = C.c_size_t(0)
        L.sbx_view_reference_info(ctx, None, 0, C.byref(n))
        buf = C.create_string_buffer(n.value + 1)
        rc = L.sbx_view_reference_info(ctx, buf, n.value + 1, C.byref(n))
        if rc != 0:
            raise SbxError(rc, "sbx_view_reference_info failed")
        return buf.raw[:n.value].decode()
    finally:
        L.sbx_close(ctx)

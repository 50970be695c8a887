"""ctypes binding of libzng_amd.so (C ABI declared in include/zng_amd.h).

There is no fallback: if the library is missing, or no MI355X-class GPU is usable, importing
works but the first call that needs the engine raises ``RuntimeError``.
"""
import ctypes as C
import weakref

import numpy as np
import mmap as _mmap
import os
import sys
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# ZNGAMD_LIB: measurement builds of the same library kept elsewhere (profiles/*.sh compile their variants to a scratch path and
# point this at them -- the product library in the tree is never overwritten)
LIB_PATH = os.environ.get("ZNGAMD_LIB") or os.path.join(_HERE, "libzng_amd.so")

OK, STREAM_END, NEED_DICT = 0, 1, 2
STREAM_ERROR, DATA_ERROR, MEM_ERROR, BUF_ERROR = -2, -3, -4, -5
E_GZ_MAGIC, E_GZ_METHOD, E_GZ_HCRC, E_GZ_CRC, E_GZ_LENGTH, E_GZ_TRUNC = -101, -102, -103, -104, -105, -106
E_HIP, E_ARG, E_OVERFLOW = -201, -202, -203

FLAG_FINAL = 1
FLAG_FLATHDR = 2
CHUNK_SHIFT = 11
UNIT_MAX = 131072
SLOT_STRIDE = 131136
SEG = 2048
INDEX_STRIDE = 68        # ZNGAMD_INDEX_STRIDE
FLAG_FINAL, FLAG_FLATHDR, FLAG_SEG2K, FLAG_UNITS16K = 1, 2, 16, 32
# ZNGAMD_STRATEGY_* (zlib's values), carried by a call's first block as ZNGAMD_FLAG_STRATEGY
STRATEGY_DEFAULT, STRATEGY_FILTERED, STRATEGY_HUFFMAN_ONLY, STRATEGY_RLE, STRATEGY_FIXED = 0, 1, 2, 3, 4


def flag_strategy(strategy):
    """ZNGAMD_FLAG_STRATEGY(strategy)"""
    if not STRATEGY_DEFAULT <= strategy <= STRATEGY_FIXED:
        raise ValueError(f"bad compression strategy {strategy}")
    return strategy << 12


def with_strategy(table, strategy):
    """A copy of a block table (from block_table()) with `strategy` on every block: the caller's table is left as it is."""
    arr, n = table
    fl = flag_strategy(strategy)
    out = (Block * max(n, 1))()
    C.memmove(out, arr, C.sizeof(Block) * max(n, 1))
    for i in range(n):
        out[i].flags = (out[i].flags & ~(7 << 12)) | fl
    return out, n
# The writer's segment index in a FILE (r06): behind the data member, EMPTY gzip members (header with FEXTRA, `03 00`, zero CRC and
# ISIZE) whose 'Z','A' subfield holds: version 3, kind 1, the number of records (u16), the first record's unit number (u32), then
# records of 138 bytes -- a unit's compressed bytes (u32, sync marker included), its output bytes (u32), 65 x u16: the bit offset of
# its first segment's first token, then each segment's length in bits (the last one ends at the end-of-block code; zeros behind
# it; all zeros = stored blocks).  The LAST of these members is a locator of 54 bytes (kind 2): members, units, bytes of the index
# members, bytes of the data member in front of them -- a reader that can seek finds the index from the file's end.
INDEX_REC = None
INDEX_PER_MEMBER = 470
INDEX_LOCATOR_BYTES = 54
E_INDEX = -204
K_NAMES = ["chains", "search", "parse", "plan", "pack", "gather", "scan", "inflate", "other", "optparse"]

# every symbol include/zng_amd.h declares (tests check that the library exports all of them)
SYMBOLS = [
    "zngamd_device_count", "zngamd_ctx_create", "zngamd_ctx_destroy", "zngamd_last_error", "zngamd_version",
    "zngamd_set_stream", "zngamd_sync", "zngamd_dmalloc", "zngamd_dfree", "zngamd_h2d", "zngamd_d2h",
    "zngamd_crc32", "zngamd_adler32", "zngamd_crc32_dev", "zngamd_crc32_combine", "zngamd_crc32_combine_many", "zngamd_level_ok",
    "zngamd_deflate_blocks", "zngamd_deflate_blocks_packed", "zngamd_count_units", "zngamd_deflate_blocks_dev", "zngamd_deflate_blocks_packed_dev", "zngamd_gather_dev",
    "zngamd_deflate_stream", "zngamd_inflate_raw", "zngamd_inflate_resume", "zngamd_gzip_scan_dev", "zngamd_gzip_inflate_members_dev",
    "zngamd_gzip_inflate_plain_members_dev", "zngamd_inflate_raw_dev", "zngamd_compare_dev", "zngamd_crc32_fold_dev",
    "zngamd_stream_deflate_init", "zngamd_stream_deflate", "zngamd_stream_deflate_set_dictionary", "zngamd_stream_deflate_copy", "zngamd_stream_pending", "zngamd_stream_inflate_ahead",
    "zngamd_stream_deflate_end", "zngamd_stream_deflate_reset", "zngamd_stream_inflate_reset", "zngamd_stream_inflate_init", "zngamd_stream_inflate", "zngamd_stream_inflate_set_dictionary",
    "zngamd_stream_inflate_copy", "zngamd_stream_inflate_end",
    "zngamd_comm_unique_id", "zngamd_comm_create", "zngamd_comm_destroy", "zngamd_comm_last_error", "zngamd_comm_count", "zngamd_comm_layout",
    "zngamd_comm_allgather_stream", "zngamd_comm_offsets", "zngamd_comm_wait", "zngamd_comm_barrier", "zngamd_comm_max_f64",
    "zngamd_gunzip", "zngamd_gunzip_partial", "zngamd_gunzip_stream", "zngamd_gzip_members", "zngamd_gzip_members_dev", "zngamd_profiling",
    "zngamd_kernel_times", "zngamd_kernel_class_count", "zngamd_abi", "zngamd_decode_paths", "zngamd_deflate_index_dev", "zngamd_inflate_units_indexed_dev", "zngamd_index_create", "zngamd_index_destroy", "zngamd_deflate_index", "zngamd_deflate_blocks_packed_indexed", "zngamd_indexed_units", "zngamd_debug_fetch", "zngamd_debug_keep", "zngamd_d2d", "zngamd_dmemset", "zngamd_mem_info",
    "zngamd_inflate_spans_dev", "zngamd_inflate_spans", "zngamd_span_stats", "zngamd_chunk_stats",
    "zngamd_inflate_batch_dev", "zngamd_inflate_batch", "zngamd_deflate_batch_dev", "zngamd_deflate_batch",
    "zngamd_inflate_batch_dict_dev", "zngamd_inflate_batch_dict", "zngamd_deflate_batch_dict_dev", "zngamd_deflate_batch_dict",
    "zngamd_train_dict_dev", "zngamd_train_dict",
    "zngamd_bgzf_compress_dev", "zngamd_bgzf_compress", "zngamd_bgzf_scan", "zngamd_bgzf_read_dev", "zngamd_bgzf_read", "zngamd_bgzf_stats",
    "zngamd_bgzf_count_dev", "zngamd_bgzf_count", "zngamd_bgzf_line_positions_dev", "zngamd_bgzf_line_positions", "zngamd_bgzf_read_lines_dev",
    "zngamd_bgzf_read_lines", "zngamd_bgzf_grep_dev", "zngamd_bgzf_grep", "zngamd_bgzf_grep_records_dev", "zngamd_bgzf_grep_records",
    "zngamd_bgzf_grep_approx_dev", "zngamd_bgzf_grep_approx", "zngamd_bgzf_grep_records_approx_dev", "zngamd_bgzf_grep_records_approx",
    "zngamd_bgzf_classify_records_dev", "zngamd_bgzf_classify_records",
    "zngamd_bgzf_partition_records_dev", "zngamd_bgzf_partition_records",
    "zngamd_bgzf_trim_records_dev", "zngamd_bgzf_trim_records",
    "zngamd_bgzf_qc_records_dev", "zngamd_bgzf_qc_records",
    "zngamd_bgzf_key_records_dev", "zngamd_bgzf_key_records", "zngamd_dedup_scratch_bytes", "zngamd_dedup_keys_dev", "zngamd_dedup_keys",
    "zngamd_bgzf_sort_key_records_dev", "zngamd_bgzf_sort_key_records", "zngamd_sort_scratch_bytes", "zngamd_sort_keys_dev", "zngamd_sort_keys",
    "zngamd_bgzf_place_records_dev", "zngamd_bgzf_place_records",
    "zngamd_kmer_set_build", "zngamd_kmer_set_load", "zngamd_kmer_set_export", "zngamd_kmer_set_describe", "zngamd_kmer_set_free",
    "zngamd_bgzf_screen_records_dev", "zngamd_bgzf_screen_records",
    "zngamd_kmer_counter_new", "zngamd_kmer_counter_reserve", "zngamd_kmer_counter_add", "zngamd_kmer_counter_describe", "zngamd_kmer_counter_histogram",
    "zngamd_kmer_counter_export", "zngamd_kmer_counter_free", "zngamd_bgzf_count_kmers_dev", "zngamd_bgzf_count_kmers",
    "zngamd_bgzf_overlap_records_dev", "zngamd_bgzf_overlap_records",
    "zngamd_bgzf_tabix_dev", "zngamd_bgzf_tabix", "zngamd_bgzf_fetch_dev", "zngamd_bgzf_fetch",
    "zngamd_bgzf_faidx_dev", "zngamd_bgzf_faidx", "zngamd_bgzf_faidx_fetch_dev", "zngamd_bgzf_faidx_fetch",
]


class GzState(C.Structure):                    # zngamd_gz_state
    _fields_ = [("in_member", C.c_uint32), ("start_bit", C.c_uint32), ("crc", C.c_uint32), ("window_len", C.c_uint32),
                ("out_total", C.c_uint64), ("window", C.c_uint8 * 32768), ("index", C.c_void_p)]


class Span(C.Structure):                       # zngamd_span
    _fields_ = [("in_bit", C.c_uint64), ("end_bit", C.c_uint64), ("win_off", C.c_uint64), ("out_off", C.c_uint64),
                ("win_len", C.c_uint32), ("out_len", C.c_uint32), ("crc", C.c_uint32), ("reserved", C.c_uint32)]


SPAN_OK, SPAN_DATA, SPAN_LENGTH, SPAN_CRC = 0, 1, 2, 3
SPAN_PAD = 64


class BatchItem(C.Structure):                  # zngamd_batch_item
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("in_len", C.c_uint32), ("out_cap", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class BatchResult(C.Structure):                # zngamd_batch_result
    _fields_ = [("status", C.c_int32), ("out_len", C.c_uint32), ("in_used", C.c_uint32), ("reserved", C.c_uint32)]


# ZNGAMD_BATCH_*: the verdict per item of the batch API
(BATCH_OK, BATCH_TRUNCATED, BATCH_OUTFULL, BATCH_NEED_DICT, BATCH_HEADER, BATCH_WINDOW, BATCH_METHOD, BATCH_FLAGS, BATCH_HCRC,
 BATCH_DATA, BATCH_CHECK, BATCH_LENGTH, BATCH_TABLE) = range(13)
BATCH_PAD = 64
ZDICT_MISMATCH = 13                            # ZNGAMD_ZDICT_MISMATCH: a zlib item's DICTID is not the dictionary's Adler-32
ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_uint64)      # zngamd_alloc_fn


class Block(C.Structure):
    _fields_ = [("off", C.c_uint64), ("len", C.c_uint32), ("dict_len", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Member(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint64), ("out_off", C.c_uint64),
                ("out_len", C.c_uint32), ("crc", C.c_uint32), ("index_off", C.c_uint32), ("nseg", C.c_uint32)]


class BgzfBlock(C.Structure):                  # zngamd_bgzf_block
    _fields_ = [("coffset", C.c_uint64), ("uoffset", C.c_uint64), ("csize", C.c_uint32), ("isize", C.c_uint32)]


class BgzfSlice(C.Structure):                  # zngamd_bgzf_slice
    _fields_ = [("src_off", C.c_uint64), ("dst_off", C.c_uint64), ("len", C.c_uint32), ("reserved", C.c_uint32)]


E_BGZF = -107                                  # ZNGAMD_E_BGZF: zngamd_bgzf_scan on data that is not BGZF
BGZF_SLICE_OK, BGZF_SLICE_BLOCK, BGZF_SLICE_TABLE = 0, 1, 2
BGZF_SLICE_RANK = 3                            # ZNGAMD_BGZF_SLICE_RANK: a rank beyond the block's delimiter count (a stale line index)
BGZF_RANK_END = 0xFFFFFFFF                     # ZNGAMD_BGZF_RANK_END: the position one past a block's last byte
BGZF_COUNT_LAST = 1                            # ZNGAMD_BGZF_COUNT_LAST
BGZF_GREP_INVERT, BGZF_GREP_LINE_START, BGZF_GREP_FINAL, BGZF_GREP_COUNT_ONLY = 1, 2, 4, 8      # ZNGAMD_BGZF_GREP_*
BGZF_GREP_MAX_PATTERNS, BGZF_GREP_MAX_PATTERN = 64, 255
BGZF_GREP_MAX_MISMATCH = 16                    # ZNGAMD_BGZF_GREP_MAX_MISMATCH
GREP_ROW_DTYPE = np.dtype([("src_off", "<u8"), ("number", "<u8"), ("len", "<u4"), ("reserved", "<u4")])      # zngamd_bgzf_grep_row


class BgzfGrepTotals(C.Structure):             # zngamd_bgzf_grep_totals
    _fields_ = [("seen", C.c_uint64), ("matched", C.c_uint64), ("bytes", C.c_uint64), ("tail_off", C.c_uint64),
                ("covered", C.c_uint32), ("reserved", C.c_uint32)]


BGZF_GREP_MAX_RECORD_LINES = 64                # ZNGAMD_BGZF_GREP_MAX_RECORD_LINES


class BgzfGrepRecordsTotals(C.Structure):      # zngamd_bgzf_grep_records_totals
    _fields_ = [("seen", C.c_uint64), ("selected", C.c_uint64), ("bytes", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64),
                ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("reserved", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads)
        return self.selected


BGZF_CLASSIFY_GROUP, BGZF_CLASSIFY_MAX_CLASSES = 16, 66      # ZNGAMD_BGZF_CLASSIFY_*
BGZF_CLASS_ASSIGNED, BGZF_CLASS_AMBIGUOUS = 1, 2               # ZNGAMD_BGZF_CLASS_*: a class row's flags (0: unassigned)
CLASS_ROW_DTYPE = np.dtype([("pattern", "u1"), ("other", "u1"), ("distance", "u1"), ("flags", "u1")])      # zngamd_bgzf_class_row


class BgzfClassifyTotals(C.Structure):         # zngamd_bgzf_classify_totals
    _fields_ = [("seen", C.c_uint64), ("bytes", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64), ("bad_src", C.c_uint64),
                ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("n_classes", C.c_uint32),
                ("class_records", C.c_uint64 * BGZF_CLASSIFY_MAX_CLASSES), ("class_bytes", C.c_uint64 * BGZF_CLASSIFY_MAX_CLASSES)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is classified)
        return self.seen


BGZF_PARTITION_MAX_CLASSES, BGZF_PARTITION_DROP = 1024, 0xFFFF      # ZNGAMD_BGZF_PARTITION_*


class BgzfPartitionTotals(C.Structure):        # zngamd_bgzf_partition_totals
    _fields_ = [("seen", C.c_uint64), ("bytes", C.c_uint64), ("dropped", C.c_uint64), ("dropped_bytes", C.c_uint64), ("tail_off", C.c_uint64),
                ("bad_record", C.c_uint64), ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32),
                ("labels_short", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is labelled)
        return self.seen


BGZF_TRIM_KEPT, BGZF_TRIM_TOO_SHORT, BGZF_TRIM_DROPPED = 0, 1, 2      # ZNGAMD_BGZF_TRIM_*: a trim row's verdict
BGZF_TRIM_KEEP_SHORT, BGZF_TRIM_NO_ADAPTER, BGZF_TRIM_MAX_QUALITY = 1, 255, 93
TRIM_ROW_DTYPE = np.dtype([("begin", "<u4"), ("end", "<u4"), ("adapter", "u1"), ("verdict", "u1"), ("steps", "u1"), ("reserved", "u1")])      # zngamd_bgzf_trim_row


class BgzfTrimConf(C.Structure):               # zngamd_bgzf_trim_conf
    _fields_ = [("record_lines", C.c_uint32), ("seq_line", C.c_int32), ("qual_line", C.c_int32), ("first_byte", C.c_int32), ("cut_front", C.c_uint32),
                ("cut_back", C.c_uint32), ("qual_front", C.c_uint32), ("qual_back", C.c_uint32), ("quality_base", C.c_uint32),
                ("max_mismatch", C.c_uint32), ("min_overlap", C.c_uint32), ("min_length", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class BgzfTrimTotals(C.Structure):             # zngamd_bgzf_trim_totals
    _fields_ = [("seen", C.c_uint64), ("kept", C.c_uint64), ("too_short", C.c_uint64), ("dropped", C.c_uint64), ("bytes_in", C.c_uint64),
                ("bytes", C.c_uint64), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64), ("quality_trimmed", C.c_uint64),
                ("adapter_trimmed", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64), ("bad_src", C.c_uint64),
                ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("drop_short", C.c_uint32),
                ("adapter_records", C.c_uint64 * BGZF_GREP_MAX_PATTERNS)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is judged)
        return self.seen


BGZF_OVERLAP_NONE, BGZF_OVERLAP_FOUND, BGZF_OVERLAP_MERGED, BGZF_OVERLAP_TOO_LONG = 0, 1, 2, 3      # ZNGAMD_BGZF_OVERLAP_*: an overlap row's verdict
BGZF_OVERLAP_MERGE, BGZF_OVERLAP_CORRECT, BGZF_OVERLAP_CUT, BGZF_OVERLAP_KEEP_UNMERGED = 1, 2, 4, 8      # conf.flags
BGZF_OVERLAP_MAX_READ, BGZF_OVERLAP_MAX_QUALITY = 1024, 93
OVERLAP_ROW_DTYPE = np.dtype([("offset", "<i4"), ("insert", "<u4"), ("overlap", "<u2"), ("mismatches", "<u2"), ("corrected", "<u2"), ("verdict", "u1"),
                              ("steps", "u1")])      # zngamd_bgzf_overlap_row


class BgzfOverlapConf(C.Structure):            # zngamd_bgzf_overlap_conf
    _fields_ = [("record_lines", C.c_uint32), ("seq_line", C.c_int32), ("qual_line", C.c_int32), ("first_byte", C.c_int32), ("quality_base", C.c_uint32),
                ("min_overlap", C.c_uint32), ("max_mismatch", C.c_uint32), ("max_percent", C.c_uint32), ("q_high", C.c_uint32), ("q_low", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class BgzfOverlapTotals(C.Structure):          # zngamd_bgzf_overlap_totals
    _fields_ = [("seen", C.c_uint64), ("none", C.c_uint64), ("found", C.c_uint64), ("merged", C.c_uint64), ("too_long", C.c_uint64), ("bytes_in", C.c_uint64),
                ("bytes", C.c_uint64), ("bases_in", C.c_uint64), ("bases_merged", C.c_uint64), ("corrected", C.c_uint64), ("corrected_pairs", C.c_uint64),
                ("adapter_pairs", C.c_uint64), ("adapter_trimmed", C.c_uint64), ("overlap_sum", C.c_uint64), ("mismatch_sum", C.c_uint64),
                ("tail_off", C.c_uint64), ("bad_record", C.c_uint64), ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32),
                ("bad", C.c_uint32), ("reserved", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every pair is judged)
        return self.seen


BGZF_QC_MAX_CYCLES, BGZF_QC_BASES, BGZF_QC_QUALITIES, BGZF_QC_MAX_LOW, BGZF_QC_GC_BINS, BGZF_QC_ROWS = 4096, 6, 94, 93, 101, 1      # ZNGAMD_BGZF_QC_*
QC_ROW_DTYPE = np.dtype([("qsum", "<u8"), ("len", "<u4"), ("gc", "<u4"), ("n", "<u4"), ("low", "<u4")])      # zngamd_bgzf_qc_row


def bgzf_qc_table_words(cycles):
    """ZNGAMD_BGZF_QC_TABLE_WORDS: the words of base_pos, qual_pos, length_hist, gc_hist and meanq_hist for `cycles`"""
    return (cycles + 1) * (BGZF_QC_BASES + BGZF_QC_QUALITIES) + (cycles + 2) + BGZF_QC_GC_BINS + BGZF_QC_QUALITIES


def bgzf_qc_split(tables, cycles):
    """the five tables of a zngamd_bgzf_qc_records call as views of its words: base_pos, qual_pos, length_hist, gc_hist, meanq_hist"""
    a = (cycles + 1) * BGZF_QC_BASES
    b = a + (cycles + 1) * BGZF_QC_QUALITIES
    c = b + cycles + 2
    d = c + BGZF_QC_GC_BINS
    return (tables[:a].reshape(cycles + 1, BGZF_QC_BASES), tables[a:b].reshape(cycles + 1, BGZF_QC_QUALITIES), tables[b:c], tables[c:d],
            tables[d:d + BGZF_QC_QUALITIES])


class BgzfQcConf(C.Structure):                 # zngamd_bgzf_qc_conf
    _fields_ = [("record_lines", C.c_uint32), ("seq_line", C.c_int32), ("qual_line", C.c_int32), ("first_byte", C.c_int32), ("quality_base", C.c_uint32),
                ("cycles", C.c_uint32), ("low_quality", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 8)]


class BgzfQcTotals(C.Structure):               # zngamd_bgzf_qc_totals
    _fields_ = [("seen", C.c_uint64), ("bytes_in", C.c_uint64), ("bases", C.c_uint64), ("min_len", C.c_uint64), ("max_len", C.c_uint64),
                ("empty", C.c_uint64), ("base_total", C.c_uint64 * BGZF_QC_BASES), ("quality_sum", C.c_uint64), ("q20_bases", C.c_uint64),
                ("q30_bases", C.c_uint64), ("low_bases", C.c_uint64), ("quality_clamped", C.c_uint64), ("tail_off", C.c_uint64),
                ("bad_record", C.c_uint64), ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32),
                ("reserved", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is counted)
        return self.seen


BGZF_KEY_IGNORE_CASE, BGZF_KEY_CANONICAL = 1, 2                                             # ZNGAMD_BGZF_KEY_*
BGZF_KEY_SEED0, BGZF_KEY_SEED1 = 0x243F6A8885A308D3, 0x13198A2E03707344                       # ZNGAMD_BGZF_KEY_SEED0 / 1
DEDUP_MAX_KEYS = 1 << 30                                                                      # ZNGAMD_DEDUP_MAX_KEYS
KEY_ROW_DTYPE = np.dtype([("lo", "<u8"), ("hi", "<u8")])                                      # zngamd_bgzf_key_row


class BgzfKeyConf(C.Structure):                # zngamd_bgzf_key_conf
    _fields_ = [("record_lines", C.c_uint32), ("seq_line", C.c_int32), ("first_byte", C.c_int32), ("first", C.c_uint32), ("length", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 10)]


class BgzfKeyTotals(C.Structure):              # zngamd_bgzf_key_totals
    _fields_ = [("seen", C.c_uint64), ("bytes_in", C.c_uint64), ("bases", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64),
                ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("reserved", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is keyed)
        return self.seen


class DedupTotals(C.Structure):                # zngamd_dedup_totals
    _fields_ = [("n", C.c_uint64), ("unique", C.c_uint64), ("duplicates", C.c_uint64), ("max_count", C.c_uint64), ("max_first", C.c_uint64),
                ("reserved", C.c_uint64)]


BGZF_SORT_BYTES, BGZF_SORT_NUMBER, BGZF_SORT_LENGTH = 0, 1, 2                               # ZNGAMD_BGZF_SORT_*: a part's kind
BGZF_SORT_REVERSE, BGZF_SORT_IGNORE_CASE, BGZF_SORT_TRUNCATE = 1, 2, 4                      # a part's flags
BGZF_SORT_MAX_PARTS, SORT_MAX_WIDTH, SORT_MAX_KEYS = 4, 256, 1 << 30                        # ZNGAMD_BGZF_SORT_MAX_PARTS, ZNGAMD_SORT_MAX_*
BGZF_PLACE_SKIP = (1 << 64) - 1                                                             # ZNGAMD_BGZF_PLACE_SKIP


class BgzfSortPart(C.Structure):               # zngamd_bgzf_sort_part
    _fields_ = [("line", C.c_int32), ("column", C.c_int32), ("width", C.c_uint32), ("first", C.c_uint32), ("flags", C.c_uint16), ("kind", C.c_uint8),
                ("sep", C.c_uint8)]


class BgzfSortConf(C.Structure):               # zngamd_bgzf_sort_conf
    _fields_ = [("record_lines", C.c_uint32), ("first_byte", C.c_int32), ("meta_byte", C.c_int32), ("n_parts", C.c_uint32), ("part", BgzfSortPart * 4),
                ("reserved", C.c_uint32 * 8)]


class BgzfSortKeyTotals(C.Structure):          # zngamd_bgzf_sort_key_totals
    _fields_ = [("seen", C.c_uint64), ("bytes_in", C.c_uint64), ("max_field", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64),
                ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("key_width", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is keyed)
        return self.seen


KMER_CANONICAL, KMER_NONE, KMER_MAX_K, KMER_MAX_REFS, KMER_MAX_POSITIONS = 1, 0xFFFFFFFF, 31, 64, 1 << 28      # ZNGAMD_KMER_*
SCREEN_ROW_DTYPE = np.dtype([("refs", "<u8"), ("kmers", "<u4"), ("hits", "<u4"), ("best", "<u4"), ("best_hits", "<u4")])      # zngamd_bgzf_screen_row


class KmerSetInfo(C.Structure):                # zngamd_kmer_set_info
    _fields_ = [("k", C.c_uint32), ("flags", C.c_uint32), ("n_refs", C.c_uint32), ("reserved", C.c_uint32), ("positions", C.c_uint64),
                ("valid", C.c_uint64), ("distinct", C.c_uint64), ("cap", C.c_uint64)]


class BgzfScreenConf(C.Structure):             # zngamd_bgzf_screen_conf
    _fields_ = [("record_lines", C.c_uint32), ("seq_line", C.c_int32), ("first_byte", C.c_int32), ("min_hits", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 11)]


class BgzfScreenTotals(C.Structure):           # zngamd_bgzf_screen_totals
    _fields_ = [("seen", C.c_uint64), ("bytes_in", C.c_uint64), ("bases", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64),
                ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("reserved", C.c_uint32),
                ("kmers", C.c_uint64), ("hits", C.c_uint64), ("matched", C.c_uint64)]


KMER_COUNTER_MAX_CAP, KMER_HIST_MAX_BINS = 1 << 33, 16384      # ZNGAMD_KMER_COUNTER_MAX_CAP, ZNGAMD_KMER_HIST_MAX_BINS


class KmerCounterInfo(C.Structure):            # zngamd_kmer_counter_info
    _fields_ = [("k", C.c_uint32), ("flags", C.c_uint32), ("poisoned", C.c_uint32), ("reserved", C.c_uint32), ("cap", C.c_uint64),
                ("distinct", C.c_uint64), ("total", C.c_uint64), ("reserved2", C.c_uint64 * 3)]


class BgzfCountConf(C.Structure):              # zngamd_bgzf_count_conf
    _fields_ = [("record_lines", C.c_uint32), ("seq_line", C.c_int32), ("first_byte", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 12)]


class BgzfCountTotals(C.Structure):            # zngamd_bgzf_count_totals
    _fields_ = [("seen", C.c_uint64), ("bytes_in", C.c_uint64), ("bases", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64),
                ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("reserved", C.c_uint32),
                ("kmers", C.c_uint64), ("claimed", C.c_uint64), ("adds", C.c_uint64)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is counted)
        return self.seen


class BgzfPlaceTotals(C.Structure):            # zngamd_bgzf_place_totals
    _fields_ = [("seen", C.c_uint64), ("placed", C.c_uint64), ("placed_bytes", C.c_uint64), ("tail_off", C.c_uint64), ("bad_record", C.c_uint64),
                ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("short_lines", C.c_uint32), ("bad", C.c_uint32), ("labels_short", C.c_uint32)]

    @property
    def matched(self):                         # (the name the window loop of bgzf.grep reads: every record is looked at)
        return self.seen


BGZF_TABIX_FINAL, BGZF_FETCH_COUNT_ONLY, BGZF_FETCH_MAX_REGIONS = 4, 8, 4096      # ZNGAMD_BGZF_TABIX_FINAL, ZNGAMD_BGZF_FETCH_*
TABIX_MAX_POS = 1 << 29                        # ZNGAMD_TABIX_MAX_POS
TABIX_NAME_DTYPE = np.dtype([("src_off", "<u8"), ("first", "<u8"), ("line", "<u8"), ("len", "<u4"), ("reserved", "<u4")])      # zngamd_tabix_name
TABIX_BIN_DTYPE = np.dtype([("src_beg", "<u8"), ("src_end", "<u8"), ("first", "<u8"), ("lines", "<u8"), ("name", "<u4"), ("bin", "<u4")])      # zngamd_tabix_bin
TABIX_WIN_DTYPE = np.dtype([("src_off", "<u8"), ("name", "<u4"), ("window", "<u4")])                      # zngamd_tabix_win
TABIX_REGION_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u4"), ("beg", "<u4"), ("end", "<u4")])   # zngamd_tabix_region
TABIX_SPAN_DTYPE = np.dtype([("text_off", "<u8"), ("text_end", "<u8"), ("region", "<u4"), ("reserved", "<u4")])      # zngamd_tabix_span
TABIX_ROW_DTYPE = np.dtype([("src_off", "<u8"), ("len", "<u4"), ("region", "<u4")])                        # zngamd_tabix_row


class TabixConf(C.Structure):                  # zngamd_tabix_conf
    _fields_ = [("format", C.c_int32), ("col_seq", C.c_int32), ("col_beg", C.c_int32), ("col_end", C.c_int32), ("meta", C.c_int32),
                ("skip", C.c_int32)]


class BgzfTabixTotals(C.Structure):            # zngamd_bgzf_tabix_totals
    _fields_ = [("seen", C.c_uint64), ("data", C.c_uint64), ("tail_off", C.c_uint64), ("bad_line", C.c_uint64), ("bad_src", C.c_uint64),
                ("n_names", C.c_uint64), ("name_bytes", C.c_uint64), ("n_bins", C.c_uint64), ("n_wins", C.c_uint64),
                ("first_line", C.c_uint64), ("first_src", C.c_uint64), ("first_beg", C.c_uint32), ("last_beg", C.c_uint32),
                ("covered", C.c_uint32), ("bad_kind", C.c_uint32)]


class BgzfFetchTotals(C.Structure):            # zngamd_bgzf_fetch_totals
    _fields_ = [("matched", C.c_uint64), ("bytes", C.c_uint64)]


BGZF_FAIDX_FINAL, BGZF_SLICE_STALE = 4, 4      # ZNGAMD_BGZF_FAIDX_FINAL, ZNGAMD_BGZF_SLICE_STALE
FAIDX_OPEN, FAIDX_GAP, FAIDX_SPAN_RC, FAIDX_MAX_SPAN = 1, 2, 1, 65536      # ZNGAMD_FAIDX_*
FAIDX_ROW_DTYPE = np.dtype([("name_src", "<u8"), ("seq_src", "<u8"), ("line", "<u8"), ("bases", "<u8"), ("name_len", "<u4"), ("line_bases", "<u4"),
                            ("line_width", "<u4"), ("reserved", "<u4")])                                    # zngamd_faidx_row
FAIDX_SPAN_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("n", "<u4"), ("col", "<u4"), ("line_bases", "<u4"), ("line_width", "<u4"),
                             ("flags", "<u4"), ("reserved", "<u4")])                                        # zngamd_faidx_span


class FaidxCarry(C.Structure):                 # zngamd_faidx_carry
    _fields_ = [("last_line", C.c_uint64), ("first_bases", C.c_uint32), ("first_width", C.c_uint32), ("last_bases", C.c_uint32),
                ("last_width", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class BgzfFaidxTotals(C.Structure):            # zngamd_bgzf_faidx_totals
    _fields_ = [("seen", C.c_uint64), ("records", C.c_uint64), ("tail_off", C.c_uint64), ("head_bases", C.c_uint64), ("name_bytes", C.c_uint64),
                ("bad_line", C.c_uint64), ("bad_src", C.c_uint64), ("covered", C.c_uint32), ("bad_kind", C.c_uint32), ("carry", FaidxCarry),
                ("head_line_bases", C.c_uint32), ("head_line_width", C.c_uint32)]


def grep_pattern_table(patterns):
    """the patterns (bytes objects) as zngamd_bgzf_grep takes them -> (blob, uint32[n, 2] of (off, len))"""
    blob = b"".join(patterns)
    lens = np.array([len(p) for p in patterns], np.uint32)
    tab = np.empty((len(patterns), 2), np.uint32)
    tab[:, 1] = lens
    tab[:, 0] = np.cumsum(lens, dtype=np.uint64) - lens
    return blob, tab

_lib = None
_lib_lock = threading.Lock()


def load():
    """Load the shared library (no GPU needed for this step)."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python python-zlib-ng_amd/build.py` "
                "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        vp, u8p, u32p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
        L.zngamd_device_count.restype = C.c_int
        L.zngamd_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.zngamd_ctx_destroy.argtypes = [vp]
        L.zngamd_ctx_destroy.restype = None
        L.zngamd_last_error.argtypes = [vp]
        L.zngamd_last_error.restype = C.c_char_p
        L.zngamd_version.restype = C.c_char_p
        L.zngamd_set_stream.argtypes = [vp, vp]
        L.zngamd_sync.argtypes = [vp]
        L.zngamd_dmalloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.zngamd_dfree.argtypes = [vp, vp]
        L.zngamd_h2d.argtypes = [vp, vp, vp, C.c_size_t]
        L.zngamd_d2h.argtypes = [vp, vp, vp, C.c_size_t]
        L.zngamd_crc32.argtypes = [vp, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.zngamd_adler32.argtypes = [vp, C.c_uint32, u8p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.zngamd_crc32_dev.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_uint32)]
        L.zngamd_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
        L.zngamd_crc32_combine.restype = C.c_uint32
        L.zngamd_crc32_combine_many.argtypes = [C.c_uint32, u32p, C.POINTER(C.c_uint64), C.c_uint32]
        L.zngamd_crc32_combine_many.restype = C.c_uint32
        L.zngamd_level_ok.argtypes = [C.c_int]
        L.zngamd_deflate_blocks.argtypes = [vp, u8p, C.c_uint64, C.POINTER(Block), C.c_uint32, C.c_int,
                                            u8p, C.c_uint64, u32p, u32p]
        L.zngamd_deflate_blocks_packed.argtypes = [vp, u8p, C.c_uint64, C.POINTER(Block), C.c_uint32, C.c_int,
                                                   u8p, C.c_uint64, C.c_uint64, u32p, u32p, C.POINTER(C.c_uint64)]
        L.zngamd_deflate_blocks_packed_indexed.argtypes = [vp, u8p, C.c_uint64, C.POINTER(Block), C.c_uint32, C.c_int,
                                                           u8p, C.c_uint64, C.c_uint64, u32p, u32p, C.POINTER(C.c_uint64),
                                                           C.c_uint32, vp, vp, vp]
        L.zngamd_count_units.argtypes = [C.POINTER(Block), C.c_uint32]
        L.zngamd_count_units.restype = C.c_uint32
        L.zngamd_deflate_blocks_dev.argtypes = [vp, vp, C.c_uint64, C.POINTER(Block), C.c_uint32, C.c_int,
                                                vp, vp, vp, u32p]
        L.zngamd_deflate_blocks_packed_dev.argtypes = [vp, vp, C.c_uint64, C.POINTER(Block), C.c_uint32, C.c_int, vp, C.c_uint64, vp, vp, vp,
                                                       C.POINTER(C.c_uint64)]
        L.zngamd_gather_dev.argtypes = [vp, vp, vp, C.c_uint32, vp, C.c_uint64, C.c_uint64, vp,
                                        C.POINTER(C.c_uint64)]
        L.zngamd_deflate_stream.argtypes = [vp, u8p, C.c_uint64, C.c_int, C.c_int, u8p, C.c_uint64,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.zngamd_inflate_raw.argtypes = [vp, u8p, C.c_uint64, u8p, C.c_uint32, u8p, C.c_uint64,
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.zngamd_inflate_resume.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, u8p, C.c_uint32, u8p, C.c_uint64,
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]
        L.zngamd_gzip_scan_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint64)]
        L.zngamd_gzip_inflate_members_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, vp]
        L.zngamd_gzip_inflate_plain_members_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, vp]
        L.zngamd_inflate_raw_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.zngamd_inflate_spans_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp]
        L.zngamd_inflate_spans.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, u8p, C.c_uint64, u8p, C.c_uint64, vp]
        L.zngamd_span_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.zngamd_chunk_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.zngamd_inflate_batch_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint64, vp]
        L.zngamd_inflate_batch.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, ALLOC_FN, vp, vp]
        L.zngamd_deflate_batch_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, C.c_uint64, vp,
                                               C.POINTER(C.c_uint64)]
        L.zngamd_deflate_batch.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, ALLOC_FN, vp, vp,
                                           C.POINTER(C.c_uint64)]
        L.zngamd_inflate_batch_dict_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, C.c_uint32, C.c_int, vp, C.c_uint64, vp]
        L.zngamd_inflate_batch_dict.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, C.c_uint32, ALLOC_FN, vp, vp]
        L.zngamd_deflate_batch_dict_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, vp, C.c_uint64,
                                                    vp, C.POINTER(C.c_uint64)]
        L.zngamd_deflate_batch_dict.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, C.c_uint32, ALLOC_FN, vp,
                                                vp, C.POINTER(C.c_uint64)]
        L.zngamd_train_dict_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u8p,
                                            C.POINTER(C.c_uint32)]
        L.zngamd_train_dict.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u8p,
                                        C.POINTER(C.c_uint32)]
        if hasattr(L, "zngamd_bgzf_scan"):           # (a variant build of an earlier revision under ZNGAMD_LIB has no BGZF entry points)
            L.zngamd_bgzf_compress_dev.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint64, C.POINTER(C.c_uint64), vp,
                                                   C.POINTER(C.c_uint32)]
            L.zngamd_bgzf_compress.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, C.c_int, u8p, C.c_uint64, C.POINTER(C.c_uint64), vp,
                                               C.c_uint32, C.POINTER(C.c_uint32)]
            L.zngamd_bgzf_scan.argtypes = [u8p, C.c_uint64, vp, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            L.zngamd_bgzf_read_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp]
            L.zngamd_bgzf_read.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, u8p, C.c_uint64, vp, vp]
            L.zngamd_bgzf_stats.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        if hasattr(L, "zngamd_bgzf_grep"):
            L.zngamd_bgzf_grep_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int,
                                               C.c_uint32, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_grep.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int,
                                           C.c_uint32, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, ALLOC_FN, vp, vp]
        if hasattr(L, "zngamd_bgzf_grep_records"):
            L.zngamd_bgzf_grep_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int,
                                                       C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint64, vp, C.c_uint64, vp, vp, C.c_uint64, vp,
                                                       C.c_uint64, vp]
            L.zngamd_bgzf_grep_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int,
                                                   C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, ALLOC_FN,
                                                   vp, vp]
        if hasattr(L, "zngamd_bgzf_grep_approx"):           # the exact calls' parameters with max_mismatch behind flags
            for name in ("zngamd_bgzf_grep", "zngamd_bgzf_grep_records"):
                for form in ("", "_dev"):
                    exact = getattr(L, name + form).argtypes
                    getattr(L, name + "_approx" + form).argtypes = exact[:13] + [C.c_uint32] + exact[13:]
        if hasattr(L, "zngamd_bgzf_classify_records"):      # the records calls with mismatches, class rows in front of the rows
            exact = L.zngamd_bgzf_grep_records_approx_dev.argtypes
            L.zngamd_bgzf_classify_records_dev.argtypes = exact[:21] + [vp, C.c_uint64] + exact[21:]
            exact = L.zngamd_bgzf_grep_records_approx.argtypes
            L.zngamd_bgzf_classify_records.argtypes = exact[:19] + [vp, C.c_uint64] + exact[19:]
        if hasattr(L, "zngamd_bgzf_partition_records"):     # the records calls without the patterns and match_line; labels and counts behind the results
            tail = [vp, C.c_uint64, C.c_uint32, vp, vp, vp]
            exact = L.zngamd_bgzf_grep_records_dev.argtypes
            L.zngamd_bgzf_partition_records_dev.argtypes = exact[:7] + exact[11:14] + exact[15:-1] + tail
            exact = L.zngamd_bgzf_grep_records.argtypes
            L.zngamd_bgzf_partition_records.argtypes = exact[:7] + exact[11:14] + exact[15:-1] + tail
        if hasattr(L, "zngamd_bgzf_trim_records"):          # the records calls with a conf for record_lines .. first_byte; mask and trim rows in front of the rows
            exact = L.zngamd_bgzf_grep_records_dev.argtypes
            L.zngamd_bgzf_trim_records_dev.argtypes = exact[:13] + [vp] + exact[16:20] + [vp, C.c_uint64, vp, C.c_uint64] + exact[20:]
            exact = L.zngamd_bgzf_grep_records.argtypes
            L.zngamd_bgzf_trim_records.argtypes = exact[:13] + [vp] + exact[16:18] + [vp, C.c_uint64, vp, C.c_uint64] + exact[18:]
        if hasattr(L, "zngamd_bgzf_qc_records"):            # no patterns: delim and flags behind text_end, then the conf; tables and rows with their capacities
            L.zngamd_bgzf_qc_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp,
                                                     C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_qc_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp, vp,
                                                 C.c_uint64, vp, C.c_uint64, ALLOC_FN, vp, vp]
        if hasattr(L, "zngamd_bgzf_key_records"):           # as qc without the tables; then the two resolve calls and the size of their work area
            L.zngamd_bgzf_key_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp,
                                                      C.c_uint64, vp, vp, C.c_uint64, vp]
            L.zngamd_bgzf_key_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp, vp,
                                                  C.c_uint64, ALLOC_FN, vp, vp]
            L.zngamd_dedup_scratch_bytes.argtypes = [C.c_uint64]
            L.zngamd_dedup_scratch_bytes.restype = C.c_uint64
            L.zngamd_dedup_keys_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp]
            L.zngamd_dedup_keys.argtypes = [vp, vp, C.c_uint64, vp, vp, vp]
        if hasattr(L, "zngamd_bgzf_sort_key_records"):      # as key with the lengths beside the rows; the sort and the size of its work area; place
            L.zngamd_bgzf_sort_key_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp,
                                                           C.c_uint64, vp, vp, vp, C.c_uint64, vp]
            L.zngamd_bgzf_sort_key_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp, vp,
                                                       vp, C.c_uint64, ALLOC_FN, vp, vp]
            L.zngamd_sort_scratch_bytes.argtypes = [C.c_uint64, C.c_uint32]
            L.zngamd_sort_scratch_bytes.restype = C.c_uint64
            L.zngamd_sort_keys_dev.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, C.c_uint64, vp, vp]
            L.zngamd_sort_keys.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp]
            L.zngamd_bgzf_place_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int32,
                                                        C.c_uint64, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_place_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_int32,
                                                    C.c_uint64, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
        if hasattr(L, "zngamd_bgzf_screen_records"):        # the set's calls; the screen: as key with the set behind the conf
            L.zngamd_kmer_set_build.argtypes = [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]
            L.zngamd_kmer_set_load.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_uint64, vp, vp]
            L.zngamd_kmer_set_export.argtypes = [vp, vp, vp, C.c_uint64, vp]
            L.zngamd_kmer_set_describe.argtypes = [vp, vp]
            L.zngamd_kmer_set_free.argtypes = [vp]
            L.zngamd_kmer_set_free.restype = None
            L.zngamd_bgzf_screen_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.c_uint64, vp,
                                                         C.c_uint64, vp, vp, C.c_uint64, vp]
            L.zngamd_bgzf_screen_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.c_uint64, vp, vp,
                                                     C.c_uint64, ALLOC_FN, vp, vp]
        if hasattr(L, "zngamd_bgzf_count_kmers"):           # the counter's calls; the count: as screen without the rows
            L.zngamd_kmer_counter_new.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint64, vp]
            L.zngamd_kmer_counter_reserve.argtypes = [vp, C.c_uint64]
            L.zngamd_kmer_counter_add.argtypes = [vp, vp, vp, C.c_uint64]
            L.zngamd_kmer_counter_describe.argtypes = [vp, vp]
            L.zngamd_kmer_counter_histogram.argtypes = [vp, vp, C.c_uint32]
            L.zngamd_kmer_counter_export.argtypes = [vp, C.c_uint64, C.c_uint64, vp, vp, C.c_uint64, vp]
            L.zngamd_kmer_counter_free.argtypes = [vp]
            L.zngamd_kmer_counter_free.restype = None
            L.zngamd_bgzf_count_kmers_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.c_uint64, vp,
                                                      C.c_uint64, vp, vp]
            L.zngamd_bgzf_count_kmers.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, vp, C.c_uint64, vp, vp]
        if hasattr(L, "zngamd_bgzf_overlap_records"):       # as qc without the tables: overlap rows, rows and bytes with their capacities
            L.zngamd_bgzf_overlap_records_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp,
                                                          C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_overlap_records.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, vp, C.c_uint64, vp, vp,
                                                      C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, ALLOC_FN, vp, vp]
        if hasattr(L, "zngamd_bgzf_tabix"):
            L.zngamd_bgzf_tabix_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_int, C.c_uint32, C.c_uint64, vp,
                                                C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_tabix.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, C.c_int, C.c_uint32, C.c_uint64, vp,
                                            vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, ALLOC_FN, vp, vp]
            L.zngamd_bgzf_fetch_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_int, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp,
                                                C.c_uint32, vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_fetch.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, vp, C.c_int, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp,
                                            C.c_uint32, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, ALLOC_FN, vp, vp]
        if hasattr(L, "zngamd_bgzf_faidx"):
            L.zngamd_bgzf_faidx_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, vp, vp,
                                                C.c_uint64, vp, vp, C.c_uint64, vp, C.c_uint64, vp]
            L.zngamd_bgzf_faidx.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, vp, vp,
                                            vp, C.c_uint64, vp, C.c_uint64, ALLOC_FN, vp, vp]
            L.zngamd_bgzf_faidx_fetch_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint64, vp, C.c_uint64, vp, vp]
            L.zngamd_bgzf_faidx_fetch.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, u8p, C.c_uint64, vp, vp]
        if hasattr(L, "zngamd_bgzf_count"):
            L.zngamd_bgzf_count_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_int, vp, C.c_uint64, vp, vp]
            L.zngamd_bgzf_count.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, C.c_int, vp, vp]
            L.zngamd_bgzf_line_positions_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int, vp, C.c_uint64, vp, vp, vp]
            L.zngamd_bgzf_line_positions.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int, vp, vp, vp]
            L.zngamd_bgzf_read_lines_dev.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int, vp, C.c_uint64, vp, C.c_uint64,
                                                     C.POINTER(C.c_uint64), vp, vp, vp]
            L.zngamd_bgzf_read_lines.argtypes = [vp, u8p, C.c_uint64, vp, C.c_uint32, vp, C.c_uint32, C.c_int, u8p, C.c_uint64, ALLOC_FN, vp,
                                                 C.POINTER(C.c_uint64), vp, vp, vp]
        L.zngamd_compare_dev.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.zngamd_crc32_fold_dev.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
        L.zngamd_gunzip.argtypes = [vp, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint32)]
        L.zngamd_gunzip_partial.argtypes = [vp, u8p, C.c_uint64, u8p, C.c_uint64, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.zngamd_gunzip_stream.argtypes = [vp, C.POINTER(GzState), u8p, C.c_uint64, C.c_int, u8p, C.c_uint64,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.zngamd_gzip_members.argtypes = [vp, u8p, C.c_uint64, C.c_uint32, C.c_int, u8p, C.c_uint64,
                                          C.POINTER(C.c_uint64)]
        L.zngamd_gzip_members_dev.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_int, vp, C.c_uint64,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.zngamd_profiling.argtypes = [vp, C.c_int]
        L.zngamd_kernel_times.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
        L.zngamd_decode_paths.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int]
        L.zngamd_debug_fetch.argtypes = [vp, C.c_int, C.c_uint32, vp, C.c_size_t]
        L.zngamd_deflate_index_dev.argtypes = [vp, vp, C.c_uint32]
        L.zngamd_index_create.argtypes = [vp, C.c_uint32, vp, vp, vp, C.POINTER(vp)]
        L.zngamd_index_destroy.argtypes = [vp]
        L.zngamd_index_destroy.restype = None
        L.zngamd_deflate_index.argtypes = [vp, C.c_uint32, vp, vp, vp]
        L.zngamd_indexed_units.argtypes = [vp, C.c_int]
        L.zngamd_indexed_units.restype = C.c_uint64
        L.zngamd_inflate_units_indexed_dev.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32, vp, vp, C.c_uint32,
                                                       vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.zngamd_debug_keep.argtypes = [vp, C.c_int]
        L.zngamd_d2d.argtypes = [vp, vp, vp, C.c_size_t]
        L.zngamd_dmemset.argtypes = [vp, vp, C.c_int, C.c_size_t]
        L.zngamd_mem_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.zngamd_comm_offsets.restype = C.c_uint64
        L.zngamd_comm_offsets.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.POINTER(C.c_uint64)]
        _lib = L
        return L


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"zng_amd error {code}: {msg}")
        self.code = code
        self.msg = msg


class _PyBuffer(C.Structure):                  # Py_buffer (CPython's buffer protocol view)
    _fields_ = [("buf", C.c_void_p), ("obj", C.c_void_p), ("len", C.c_ssize_t), ("itemsize", C.c_ssize_t),
                ("readonly", C.c_int), ("ndim", C.c_int), ("format", C.c_char_p), ("shape", C.c_void_p),
                ("strides", C.c_void_p), ("suboffsets", C.c_void_p), ("internal", C.c_void_p)]


C.pythonapi.PyObject_GetBuffer.argtypes = [C.py_object, C.POINTER(_PyBuffer), C.c_int]
C.pythonapi.PyObject_GetBuffer.restype = C.c_int
C.pythonapi.PyBuffer_Release.argtypes = [C.POINTER(_PyBuffer)]
C.pythonapi.PyBuffer_Release.restype = None


class _Pinned:
    """Holds a buffer-protocol view of an object (read-only ones included) for the duration of an engine call."""

    def __init__(self, obj):
        self.view = _PyBuffer()
        self.ok = C.pythonapi.PyObject_GetBuffer(obj, C.byref(self.view), 0) == 0      # PyBUF_SIMPLE

    def __del__(self):
        if getattr(self, "ok", False):
            C.pythonapi.PyBuffer_Release(C.byref(self.view))
            self.ok = False


def _dict_arg(zdict):
    """(pointer, keep-alive, length) of a batch call's dictionary: NULL and 0 for None ("no dictionary"), and never a NULL pointer for
    an empty one"""
    if zdict is None:
        return None, None, 0
    n = memoryview(zdict).nbytes
    if n == 0:
        b = b"\0"
        return C.cast(C.c_char_p(b), C.c_void_p), b, 0
    p, keep = _addr(zdict)
    return p, keep, n


def _addr(buf):
    """Address + keep-alive object of a bytes-like, without copying (contiguous buffers of any kind)."""
    if isinstance(buf, bytes):
        return C.cast(C.c_char_p(buf), C.c_void_p), buf
    try:
        pin = _Pinned(buf)                       # raises BufferError for non-contiguous exporters
    except Exception:
        pin = None
    if pin is not None and pin.ok:
        return C.c_void_p(pin.view.buf), (pin, buf)
    b = memoryview(buf).tobytes()
    return C.cast(C.c_char_p(b), C.c_void_p), b


def _dv(x):
    """A device pointer as the _dev forms take it (an int or anything int() takes; 0 or None: NULL)."""
    return C.c_void_p(int(x)) if x else None


def _window_in(data, members):
    """What every host form of a BGZF call begins with: data = packed compressed blocks, members = numpy table of MEMBER rows ->
    (the four arguments (input, its bytes, member rows or NULL, their number), the block statuses int32[n] for the engine to fill,
    what keeps the input alive)"""
    nm = len(members)
    p, keep = _addr(data)
    st = np.zeros(max(1, nm), np.int32)[:nm]         # (no member: a view of no entries whose address is still a real one)
    return (p, memoryview(data).nbytes, C.c_void_p(members.ctypes.data) if nm else None, nm), st, keep


class _RowsOut:
    """Where the rows of a host form come back, one row of `dtype` per record.  caps None: the engine asks .fn for them once it knows
    how many there are; a number: a buffer of that many rows (.ptr, .cap), which the engine refuses with BUF_ERROR when it is too small."""

    def __init__(self, dtype, caps):
        self.dtype, self.box, self.rows = dtype, [], None

        def alloc(_user, nbytes):
            self.box.append(np.empty(nbytes // dtype.itemsize, dtype))
            return self.box[0].ctypes.data

        if caps is None:
            self.ptr, self.cap, self.fn = None, 0, ALLOC_FN(alloc)
        else:
            self.rows = np.zeros(max(1, caps), dtype)
            self.ptr, self.cap, self.fn = C.c_void_p(self.rows.ctypes.data), caps, ALLOC_FN()

    def take(self, got, seen):
        """the rows when the call has left them (got), otherwise none"""
        if not got:
            return np.empty(0, self.dtype)
        return self.box[0] if self.rows is None else self.rows[:seen]


_py = C.pythonapi
_py.PyBytes_FromStringAndSize.restype = C.py_object
_py.PyBytes_FromStringAndSize.argtypes = [C.c_void_p, C.c_ssize_t]
_py.PyBytes_AsString.restype = C.c_void_p
_py.PyBytes_AsString.argtypes = [C.py_object]


_HUGE_MIN = 8 << 20
try:
    _madvise = C.CDLL(None, use_errno=True).madvise
    _madvise.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    _madvise.restype = C.c_int
except Exception:                                    # pragma: no cover
    _madvise = None


def _advise_huge(addr, n):
    """Fresh memory of a large buffer is first touched by the engine's copy threads or a file read, one page fault per 4 KiB
    (21 000 for an 88 MB result, more time than the copy itself) -- with transparent huge pages one per 2 MiB, where the
    system allows them on request.  A refusal changes nothing."""
    if n >= _HUGE_MIN and _madvise is not None:
        lo = (addr + 0x1FFFFF) & ~0x1FFFFF
        hi = (addr + n) & ~0x1FFFFF
        if hi > lo:
            _madvise(C.c_void_p(lo), C.c_size_t(hi - lo), 14)       # MADV_HUGEPAGE


def _new_bytes(n):
    """A fresh, uninitialised bytes object of n >= 1 bytes for the engine to fill, and its address: no zero fill,
    and no copy when the engine fills it completely."""
    obj = _py.PyBytes_FromStringAndSize(None, max(int(n), 1))
    addr = _py.PyBytes_AsString(obj)
    _advise_huge(addr, int(n))
    return obj, C.c_void_p(addr)


new_buffer = _new_bytes          # for callers that keep an output buffer across calls (see Context.gunzip_stream)


def new_fillable(n):
    """(bytes object, writable byte view of it) for `readinto`: an input window that is not zero-filled first -- a
    bytearray(n) costs a memset of the whole window however little the file then delivers."""
    obj, addr = _new_bytes(n)
    return obj, memoryview((C.c_ubyte * max(int(n), 1)).from_address(addr.value)).cast("B")


# raw-pointer views of four C-API functions: the object below is owned through a bare pointer until it is handed over
_raw_new = C.PYFUNCTYPE(C.c_void_p, C.c_void_p, C.c_ssize_t)(("PyBytes_FromStringAndSize", C.pythonapi))
_raw_buf = C.PYFUNCTYPE(C.c_void_p, C.c_void_p)(("PyBytes_AsString", C.pythonapi))
_raw_resize = C.PYFUNCTYPE(C.c_int, C.POINTER(C.c_void_p), C.c_ssize_t)(("_PyBytes_Resize", C.pythonapi))
_raw_decref = C.PYFUNCTYPE(None, C.c_void_p)(("Py_DecRef", C.pythonapi))


class _Out:
    """An engine output buffer on its way to becoming the result: a fresh bytes object that Python has not seen yet (it is
    held through a bare pointer with its single reference), so it can be cut to the produced length in place
    (_PyBytes_Resize, what CPython's own zlib module does) instead of being copied into a second object."""
    __slots__ = ("ptr", "cap")

    def __init__(self, n):
        self.cap = max(int(n), 1)
        self.ptr = C.c_void_p(_raw_new(None, self.cap))
        if not self.ptr.value:
            raise MemoryError("cannot allocate the result")
        _advise_huge(_raw_buf(self.ptr), self.cap)

    def addr(self):
        return C.c_void_p(_raw_buf(self.ptr))

    def resize(self, n):
        """Grow (or cut) the buffer in place; its address may change."""
        n = max(int(n), 1)
        if _raw_resize(C.byref(self.ptr), n) != 0:
            self.ptr = C.c_void_p(None)          # _PyBytes_Resize released the object on failure
            raise MemoryError("cannot resize the result")
        self.cap = n

    def take(self, n):
        n = min(int(n), self.cap)
        if n == 0:
            self._drop()
            return b""
        if n != self.cap and _raw_resize(C.byref(self.ptr), n) != 0:
            self.ptr = C.c_void_p(None)          # _PyBytes_Resize released the object on failure
            raise MemoryError("cannot resize the result")
        res = C.cast(self.ptr, C.py_object).value     # a new reference for Python ...
        self._drop()                                   # ... and ours is given up
        return res

    def _drop(self):
        if self.ptr is not None and self.ptr.value:
            _raw_decref(self.ptr)
        self.ptr = C.c_void_p(None)

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass


def _take(obj, n):
    return obj if n == len(obj) else obj[:n]


# Large host buffers of the streaming writers and readers (collected input, packed output, file windows).  Fresh memory costs a
# page fault per 4 KiB on first touch -- 3.3 us each on the GPU boxes, 54 ms for a 64 MiB buffer, more than compressing it -- so
# such buffers ask for transparent huge pages and go back to a small process-wide pool when their owner closes (like the
# contexts' device workspaces, which also live as long as the process): the next file opened finds them warm.
_POOL_MAX_BYTES = max(0, int(os.environ.get("ZNGAMD_HOST_POOL_MIB", "1024"))) << 20      # (0: nothing is kept)
_buffer_pool, _buffer_pool_lock = [], threading.Lock()


def take_buffer(n):
    """A writable buffer of at least n bytes (contents arbitrary), warm if the pool has one."""
    n = max(int(n), 1)
    with _buffer_pool_lock:
        best = None
        for i, b in enumerate(_buffer_pool):
            if len(b) >= n and (best is None or len(b) < len(_buffer_pool[best])):
                best = i
        if best is not None and len(_buffer_pool[best]) <= 2 * n + (1 << 20):
            return _buffer_pool.pop(best)
    # an anonymous private mapping, not a bytearray: bytearray(n) writes n zeros at once -- a page fault per 4 KiB before the request
    # for huge pages can be made, 100 ms for the 320 MiB of a reader's window -- where the mapping's pages come into being when
    # they are first written, two MiB at a time
    buf = _mmap.mmap(-1, n, flags=_mmap.MAP_PRIVATE | _mmap.MAP_ANONYMOUS)
    if n >= _HUGE_MIN:
        try:
            buf.madvise(_mmap.MADV_HUGEPAGE)
        except (AttributeError, OSError, ValueError):
            pass
    return buf


def give_buffer(buf):
    """Hand a buffer from take_buffer() back (nothing may still read or write it)."""
    if not isinstance(buf, (bytearray, _mmap.mmap)) or len(buf) < (1 << 20):
        return
    with _buffer_pool_lock:
        if sum(len(b) for b in _buffer_pool) + len(buf) <= _POOL_MAX_BYTES:
            _buffer_pool.append(buf)


def take_window(n):
    """(buffer, address) for Context.gunzip_stream(into=...): a pooled buffer the engine decodes a window into."""
    buf = take_buffer(n)
    anchor = C.c_char.from_buffer(buf)
    addr = C.c_void_p(C.addressof(anchor))
    del anchor
    return buf, addr


def crc32_combine_many(crc, crcs, lens):
    """crc32_combine over a run of pieces in one call (a writer thread that folds 512 blocks one foreign call at a time hands
    the interpreter lock back and forth 1 000 times while its caller wants it)."""
    n = len(crcs)
    a = (C.c_uint32 * max(n, 1))(*crcs)
    b = (C.c_uint64 * max(n, 1))(*lens)
    return load().zngamd_crc32_combine_many(crc & 0xFFFFFFFF, a, b, n)


def _index_rec_dtype():
    global INDEX_REC
    if INDEX_REC is None:
        INDEX_REC = np.dtype([("in_len", "<u4"), ("out_len", "<u4"), ("e", "<u2", (65,))])
        assert INDEX_REC.itemsize == 138
    return INDEX_REC


def _za_member(payload):
    """an empty gzip member whose FEXTRA field is one 'Z','A' subfield"""
    import struct
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff" + struct.pack("<H", 4 + len(payload)) + b"ZA" + struct.pack("<H", len(payload)) +
            payload + b"\x03\x00" + bytes(8))


def index_members(recs, data_member_bytes):
    """The index members + locator for the records of one data member (a list of INDEX_REC arrays in unit order)."""
    import struct
    allrec = np.concatenate(recs) if len(recs) != 1 else recs[0]
    out, nm = [], 0
    for lo in range(0, len(allrec), INDEX_PER_MEMBER):
        part = allrec[lo:lo + INDEX_PER_MEMBER]
        out.append(_za_member(struct.pack("<BBHI", 3, 1, len(part), lo) + part.tobytes()))
        nm += 1
    body = b"".join(out)
    loc = _za_member(struct.pack("<BBHIIQQ", 3, 2, 0, nm, len(allrec), len(body), data_member_bytes))
    assert len(loc) == INDEX_LOCATOR_BYTES
    return body + loc


def parse_index_tail(fp, start, end):
    """The index of a file [start, end) that is ONE data member followed by index members (and, possibly, the plain empty member
    the reference's close() leaves): -> (in_len, out_len, rows) as numpy arrays (rows: units x INDEX_STRIDE u32), or None.  The
    file position is left where it was."""
    import struct
    here = fp.tell()
    try:
        tail_skip = 0
        for attempt in (0, 1):
            if end - start < INDEX_LOCATOR_BYTES + tail_skip + 20:
                return None
            fp.seek(end - tail_skip - INDEX_LOCATOR_BYTES)
            loc = fp.read(INDEX_LOCATOR_BYTES)
            if len(loc) == INDEX_LOCATOR_BYTES and loc[:4] == b"\x1f\x8b\x08\x04" and loc[12:14] == b"ZA" and loc[16] == 3 and loc[17] == 2:
                break
            if attempt == 0:                          # behind a trailing plain empty member?
                fp.seek(end - 20)
                plain = fp.read(20)
                if len(plain) == 20 and plain[:4] == b"\x1f\x8b\x08\x00" and plain[10:] == b"\x03\x00" + bytes(8):
                    tail_skip = 20
                    continue
            return None
        _v, _k, _p, nm, nu, ibytes, dbytes = struct.unpack("<BBHIIQQ", loc[16:44])
        if loc[44:] != b"\x03\x00" + bytes(8):
            return None
        ix0 = end - tail_skip - INDEX_LOCATOR_BYTES - ibytes
        if ix0 - dbytes != start or nu == 0 or nu > (1 << 26) or ibytes > (1 << 34):
            return None
        fp.seek(ix0)
        blob = fp.read(ibytes)
        if len(blob) != ibytes:
            return None
        rt = _index_rec_dtype()
        parts, at, seen = [], 0, 0
        for _ in range(nm):
            if blob[at:at + 4] != b"\x1f\x8b\x08\x04" or blob[at + 12:at + 14] != b"ZA":
                return None
            slen = struct.unpack_from("<H", blob, at + 14)[0]
            v, k, n, first = struct.unpack_from("<BBHI", blob, at + 16)
            if v != 3 or k != 1 or first != seen or slen != 8 + n * rt.itemsize:
                return None
            parts.append(np.frombuffer(blob, rt, n, at + 24))
            seen += n
            at += 16 + slen + 10
        if seen != nu or at != ibytes:
            return None
        rec = np.concatenate(parts) if len(parts) != 1 else parts[0]
        if int(rec["in_len"].astype(np.int64).sum()) + 10 + 10 != dbytes:        # header, units, 03 00, trailer
            return None
        fp.seek(start + dbytes - 4)                                  # the units' output is the member's: ISIZE (modulo 2^32)
        isize = fp.read(4)
        if len(isize) != 4 or (int(rec["out_len"].astype(np.int64).sum()) & 0xFFFFFFFF) != struct.unpack("<I", isize)[0]:
            return None
        rows = np.zeros((nu, INDEX_STRIDE), np.uint32)
        nseg = (rec["out_len"].astype(np.int64) + 2047) >> 11
        cum = np.cumsum(rec["e"].astype(np.uint32), axis=1, dtype=np.uint32)
        cum[np.arange(65)[None, :] > nseg[:, None]] = 0
        cum[rec["e"].max(axis=1) == 0] = 0                          # stored units
        rows[:, :65] = cum
        return np.ascontiguousarray(rec["in_len"]), np.ascontiguousarray(rec["out_len"]), rows
    except (OSError, ValueError, struct.error):
        return None
    finally:
        try:
            fp.seek(here)
        except (OSError, ValueError):
            pass


def bgzf_scan(data, max_blocks=None):
    """zngamd_bgzf_scan (no GPU) -> (code, [(coffset, uoffset, block bytes, isize), ...], consumed, total_out)"""
    L = load()
    p, keep = _addr(data)
    n = memoryview(data).nbytes
    cap = n // 26 + 1 if max_blocks is None else int(max_blocks)
    tab = (BgzfBlock * max(cap, 1))()
    nb, used, tot = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
    r = L.zngamd_bgzf_scan(p, n, tab, cap, C.byref(nb), C.byref(used), C.byref(tot))
    return r, [(t.coffset, t.uoffset, t.csize, t.isize) for t in tab[:nb.value]], used.value, tot.value


def block_table(blocks):
    """(ctypes table, count) of a list of (off, len, dict_len, flags) for Context.deflate_blocks."""
    n = len(blocks)
    arr = (Block * max(n, 1))()
    for i, (off, ln, dl, fl) in enumerate(blocks):
        if ln > 0xFFFFFFFF or dl > 0xFFFFFFFF:            # ctypes would cut the u32 fields silently
            raise OverflowError("a block is limited to 4 GiB - 1 bytes: split it")
        arr[i] = Block(off, ln, dl, fl, 0)
    return arr, n


class DeviceKmerSet:
    """A zngamd_kmer_set: the table of a k-mer set on the device, read-only, bound to the context it was made in.  free() releases it;
    so do the end of the object and the close() of its context."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def info(self):
        info = KmerSetInfo()
        if self.ctx.L.zngamd_kmer_set_describe(self.h, C.byref(info)) != OK:
            raise ValueError("the set was freed")
        return info

    def export(self):
        """-> (codes, masks), uint64, in no particular order"""
        n = C.c_uint64(self.info.distinct)
        codes, masks = np.empty(n.value, np.uint64), np.empty(n.value, np.uint64)
        p = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
        self.ctx._chk(self.ctx.L.zngamd_kmer_set_export(self.h, p(codes), p(masks), len(codes), C.byref(n)))
        return codes[:n.value], masks[:n.value]

    def free(self):
        if self.h:
            self.ctx.L.zngamd_kmer_set_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceKmerCounter:
    """A zngamd_kmer_counter: the (code, count) table of a k-mer counter on the device, bound to the context it was made in.  free()
    releases it; so do the end of the object and the close() of its context.  Every call on a freed counter is a ValueError."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def _handle(self):
        if not self.h:
            raise ValueError("the counter was freed")
        return self.h

    @property
    def info(self):
        info = KmerCounterInfo()
        if self.ctx.L.zngamd_kmer_counter_describe(self._handle(), C.byref(info)) != OK:
            raise ValueError("the counter was freed")
        return info

    def reserve(self, room):
        """zngamd_kmer_counter_reserve -> code: OK, or MEM_ERROR when the device cannot give the grown table (the counter is unchanged)"""
        return self.ctx._chk(self.ctx.L.zngamd_kmer_counter_reserve(self._handle(), room), (OK, MEM_ERROR))

    def add(self, codes, counts):
        """zngamd_kmer_counter_add: (code, count) pairs (uint64 arrays of equal length) -> code: OK, or BUF_ERROR when the table lacks the
        room (nothing was added: reserve first)"""
        codes, counts = np.ascontiguousarray(codes, np.uint64), np.ascontiguousarray(counts, np.uint64)
        n = len(codes)
        if len(counts) != n:
            raise ValueError("codes and counts are of equal length")
        p = lambda a: C.c_void_p(a.ctypes.data) if n else None
        return self.ctx._chk(self.ctx.L.zngamd_kmer_counter_add(self._handle(), p(codes), p(counts), n), (OK, BUF_ERROR))

    def histogram(self, bins):
        """zngamd_kmer_counter_histogram -> uint64 of `bins` entries: [c] the codes with count c, [bins - 1] those with at least that"""
        hist = np.zeros(max(int(bins), 1), np.uint64)
        self.ctx._chk(self.ctx.L.zngamd_kmer_counter_histogram(self._handle(), C.c_void_p(hist.ctypes.data), bins))
        return hist

    def export(self, min_count=1, max_count=0, cap_pairs=None):
        """zngamd_kmer_counter_export -> (code, codes, counts, n): the pairs with min_count <= count <= max_count (0: no upper bound) in no
        particular order.  cap_pairs None: the pairs are counted first and all come back; an integer: room for that many, and code is
        BUF_ERROR, with n set and no pair, when there are more"""
        h = self._handle()
        n = C.c_uint64(0)
        if cap_pairs is None:
            self.ctx._chk(self.ctx.L.zngamd_kmer_counter_export(h, min_count, max_count, None, None, 0, C.byref(n)), (OK, BUF_ERROR))
            cap_pairs = n.value
        codes, counts = np.empty(cap_pairs, np.uint64), np.empty(cap_pairs, np.uint64)
        p = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
        r = self.ctx._chk(self.ctx.L.zngamd_kmer_counter_export(h, min_count, max_count, p(codes), p(counts), cap_pairs, C.byref(n)), (OK, BUF_ERROR))
        got = n.value if r == OK else 0
        return r, codes[:got], counts[:got], n.value

    def free(self):
        if self.h:
            self.ctx.L.zngamd_kmer_counter_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    """One engine context = one GPU + one HIP stream + grow-only device workspaces."""

    def __init__(self, device=None):
        L = load()
        if device is None:
            device = int(os.environ.get("ZNGAMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
            n = L.zngamd_device_count()
            if n > 0:
                device %= n
        h = C.c_void_p()
        r = L.zngamd_ctx_create(device, C.byref(h))
        if r != OK:
            raise RuntimeError(
                f"zng_amd: no usable GPU (zngamd_ctx_create({device}) -> {r}); this engine has no CPU path")
        self.L, self.h, self.device = L, h, device
        self._scratch, self._scratch_lock = None, threading.Lock()
        self._tls = threading.local()

    @property
    def last_needed(self):
        """Room the calling thread's last inflate call asked for (0 = it fitted); per thread, like the engine's message."""
        return getattr(self._tls, "needed", 0)

    @last_needed.setter
    def last_needed(self, v):
        self._tls.needed = v

    def close(self):
        if self.h:
            for kset in list(self.__dict__.get("_kmer_sets", ())):      # (a set is freed before the context it was made in)
                kset.free()
            self.L.zngamd_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def err(self):
        return self.L.zngamd_last_error(self.h).decode("utf-8", "replace")

    def _chk(self, r, ok=(OK,)):
        if r not in ok:
            raise EngineError(r, self.err())
        return r

    def sync(self):
        """wait for everything queued on the context's stream"""
        self._chk(self.L.zngamd_sync(self.h))

    # ---- checksums
    def crc32(self, data, value=0):
        p, keep = _addr(data)
        out = C.c_uint32(0)
        self._chk(self.L.zngamd_crc32(self.h, value & 0xFFFFFFFF, p, memoryview(data).nbytes, C.byref(out)))
        return out.value

    def adler32(self, data, value=1):
        p, keep = _addr(data)
        out = C.c_uint32(0)
        self._chk(self.L.zngamd_adler32(self.h, value & 0xFFFFFFFF, p, memoryview(data).nbytes, C.byref(out)))
        return out.value

    def crc32_combine(self, crc1, crc2, len2):
        return self.L.zngamd_crc32_combine(crc1 & 0xFFFFFFFF, crc2 & 0xFFFFFFFF, len2)

    # ---- deflate
    def deflate_blocks(self, buf, blocks, level, out_cap, joined=False, into=None, index=False, strategy=STRATEGY_DEFAULT):
        """blocks: list of (off, len, dict_len, flags), or a table made by block_table() (a writer whose batches have the
        same shape makes it once).  -> (list of bytes|None, list of crc, overflowed); with joined=True the first element is
        ONE object, the blocks' outputs back to back (a writer that only concatenates them saves the allocation and release
        of one object per block) and a list of lengths is appended to the result: the engine copies the packed stream
        straight into it (zngamd_deflate_blocks_packed).  `into` (joined only): a bytearray of at least n * out_cap bytes
        that takes the output -- the result is then a memoryview of its filled part (a writer that keeps two of them
        writes into warm memory; a fresh object costs a page fault per 4 KiB).  `index` (joined only): the segment-index records
        of the call's units come back as a fifth element (None after an overflow) -- from the SAME engine call
        (zngamd_deflate_blocks_packed_indexed): a context that several writer threads share answers zngamd_deflate_index for its
        last deflate call, whoever made it.  `strategy`: zlib's compression strategy (STRATEGY_*) for every block of the call."""
        arr, n = blocks if isinstance(blocks, tuple) and len(blocks) == 2 and isinstance(blocks[0], C.Array) else block_table(blocks)
        if strategy != STRATEGY_DEFAULT:
            arr, n = with_strategy((arr, n), strategy)
        p, keep = _addr(buf)
        lens = (C.c_uint32 * max(n, 1))()
        crcs = (C.c_uint32 * max(n, 1))()
        need = max(n, 1) * out_cap
        if joined:
            total = C.c_uint64(0)
            if index:
                nu = int(self.L.zngamd_count_units(arr, n))
                uin = np.empty(max(nu, 1), np.uint32); uout = np.empty(max(nu, 1), np.uint32); rows = np.empty((max(nu, 1), INDEX_STRIDE), np.uint32)
                tail = (nu, uin.ctypes.data_as(C.c_void_p), uout.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p))
                call = self.L.zngamd_deflate_blocks_packed_indexed
            else:
                tail = ()
                call = self.L.zngamd_deflate_blocks_packed
            if into is not None and len(into) >= need:
                anchor = C.c_char.from_buffer(into)
                r = call(self.h, p, memoryview(buf).nbytes, arr, n, level,
                         C.cast(C.addressof(anchor), C.c_void_p), len(into), out_cap,
                         C.cast(lens, C.c_void_p), C.cast(crcs, C.c_void_p), C.byref(total), *tail)
                del anchor
                self._chk(r, (OK, E_OVERFLOW))
                res = None if r == E_OVERFLOW else memoryview(into)[:total.value]
            else:
                out = _Out(need)
                r = call(self.h, p, memoryview(buf).nbytes, arr, n, level, out.addr(), need, out_cap,
                         C.cast(lens, C.c_void_p), C.cast(crcs, C.c_void_p), C.byref(total), *tail)
                self._chk(r, (OK, E_OVERFLOW))
                res = None if r == E_OVERFLOW else out.take(total.value)
            if index:
                return res, list(crcs[:n]), r == E_OVERFLOW, list(lens[:n]), (None if r == E_OVERFLOW else self._index_records(nu, uin[:nu], uout[:nu], rows[:nu]))
            return res, list(crcs[:n]), r == E_OVERFLOW, list(lens[:n])
        # The per-block outputs land in a buffer that lives with the context: device-to-host copies into memory that has
        # been touched (and registered by the runtime) before run several times faster than into fresh pages.  The lock
        # covers the call and the slicing (engine calls of one context are serial anyway).
        with self._scratch_lock:
            if self._scratch is None or len(self._scratch) < need:
                self._scratch = bytearray(need + need // 4)
            out = self._scratch
            arr_out = (C.c_char * len(out)).from_buffer(out)
            r = self.L.zngamd_deflate_blocks(self.h, p, memoryview(buf).nbytes, arr, n, level,
                                             C.cast(arr_out, C.c_void_p), out_cap, C.cast(lens, C.c_void_p), C.cast(crcs, C.c_void_p))
            del arr_out
            self._chk(r, (OK, E_OVERFLOW))
            res = []
            mv = memoryview(out)
            for i in range(n):
                if lens[i] == 0xFFFFFFFF:
                    res.append(None)
                else:
                    res.append(bytes(mv[i * out_cap:i * out_cap + lens[i]]))
            del mv
        return res, list(crcs[:n]), r == E_OVERFLOW

    def deflate_stream(self, data, level, window_bits=15, prefix=b"", trailer=None):
        """-> (prefix + raw deflate bytes + trailer(crc32, adler32), crc32, adler32).  The container's header and trailer are
        written into the result object itself, around the bytes the engine puts there: no second copy of the payload."""
        p, keep = _addr(data)
        n = memoryview(data).nbytes
        cap = n + (n // 16384 + 1) * 16 + 192          # (a call of up to 128 KiB is cut into units of 16 KiB: 10 bytes each at worst, stored)
        room = len(prefix) + (8 if trailer is not None else 0)
        out = _Out(cap + room)
        base = out.addr().value
        ol = C.c_uint64(0)
        crc, ad = C.c_uint32(0), C.c_uint32(1)
        self._chk(self.L.zngamd_deflate_stream(self.h, p, n, level, window_bits, C.c_void_p(base + len(prefix)), cap,
                                               C.byref(ol), C.byref(crc), C.byref(ad)))
        total = len(prefix) + ol.value
        if prefix:
            C.memmove(base, prefix, len(prefix))
        if trailer is not None:
            t = trailer(crc.value, ad.value)
            C.memmove(base + total, t, len(t))
            total += len(t)
        return out.take(total), crc.value, ad.value

    def debug_keep(self, on=True):
        self._chk(self.L.zngamd_debug_keep(self.h, 1 if on else 0))

    def debug_fetch(self, what, unit, nbytes):
        b = C.create_string_buffer(nbytes)
        self._chk(self.L.zngamd_debug_fetch(self.h, what, unit, C.cast(b, C.c_void_p), nbytes))
        return b.raw

    # ---- inflate
    def inflate_raw(self, data, out_cap, zdict=b""):
        """-> (code, out bytes, in_used, crc32, adler32)"""
        p, keep = _addr(data)
        dp, dkeep = _addr(zdict) if len(zdict) else (None, None)
        out = _Out(out_cap)
        ol, used = C.c_uint64(0), C.c_uint64(0)
        crc, ad = C.c_uint32(0), C.c_uint32(1)
        r = self.L.zngamd_inflate_raw(self.h, p, memoryview(data).nbytes, dp, len(zdict),
                                      out.addr(), out_cap, C.byref(ol), C.byref(used),
                                      C.byref(crc), C.byref(ad))
        if r in (E_HIP, E_ARG):
            raise EngineError(r, self.err())
        # BUF_ERROR with a size above the capacity = "this is how much room the stream needs" (nothing was copied)
        self.last_needed = ol.value if (r == BUF_ERROR and ol.value > out_cap) else 0
        if self.last_needed:
            return r, b"", 0, 0, 1
        return r, out.take(min(ol.value, out_cap)), used.value, crc.value, ad.value

    def inflate_resume(self, data, start_bit, zdict, out_cap):
        """-> (code, out bytes, in_bits, block_bits, block_out); code E_OVERFLOW = out_cap reached"""
        p, keep = _addr(data)
        dp, dkeep = _addr(zdict) if len(zdict) else (None, None)
        out = _Out(out_cap)
        ol, ib, bb, bo = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        r = self.L.zngamd_inflate_resume(self.h, p, memoryview(data).nbytes, start_bit, dp, len(zdict),
                                         out.addr(), out_cap, C.byref(ol), C.byref(ib), C.byref(bb), C.byref(bo))
        if r in (E_HIP, E_ARG):
            raise EngineError(r, self.err())
        return r, out.take(min(ol.value, out_cap)), ib.value, bb.value, bo.value

    def gunzip(self, data, out_cap):
        """-> (code, out bytes, n_members)"""
        p, keep = _addr(data)
        out = _Out(out_cap)
        ol, nm = C.c_uint64(0), C.c_uint32(0)
        r = self.L.zngamd_gunzip(self.h, p, memoryview(data).nbytes, out.addr(), out_cap,
                                 C.byref(ol), C.byref(nm))
        if r in (E_HIP, E_ARG):
            raise EngineError(r, self.err())
        # BUF_ERROR with a size above the capacity = "this is how much room the stream needs"
        self.last_needed = ol.value if (r == BUF_ERROR and ol.value > out_cap) else 0
        return r, out.take(min(ol.value, out_cap)), nm.value

    def gunzip_partial(self, data, out_cap):
        """Window of a longer stream -> (code, out bytes, n_members, in_consumed); see zngamd_gunzip_partial."""
        p, keep = _addr(data)
        out = _Out(out_cap)
        ol, nm, used = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        r = self.L.zngamd_gunzip_partial(self.h, p, memoryview(data).nbytes, out.addr(), out_cap,
                                         C.byref(ol), C.byref(nm), C.byref(used))
        if r in (E_HIP, E_ARG):
            raise EngineError(r, self.err())
        self.last_needed = ol.value if (r == BUF_ERROR and ol.value > out_cap) else 0
        return r, out.take(min(ol.value, out_cap)), nm.value, used.value

    def gunzip_stream(self, state, data, out_cap, last, view=False, into=None):
        """Stateful window of a longer stream -> (code, out bytes, n_members, in_consumed); see zngamd_gunzip_stream."""
        p, keep = _addr(data)
        if into is not None:                    # (object, address) from new_buffer(): reused from window to window, so
            out, op = into                      # its pages are faulted in once
            view = True
        else:
            out, op = _new_bytes(out_cap)
        ol, nm, used = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        r = self.L.zngamd_gunzip_stream(self.h, C.byref(state), p, memoryview(data).nbytes, 1 if last else 0, op, out_cap,
                                        C.byref(ol), C.byref(nm), C.byref(used))
        if r in (E_HIP, E_ARG):
            raise EngineError(r, self.err())
        self.last_needed = ol.value if (r == BUF_ERROR and ol.value > out_cap) else 0
        n = min(ol.value, out_cap)
        if view:                                # the caller only reads from it: no copy of the filled part
            return r, memoryview(out)[:n], nm.value, used.value
        return r, _take(out, n), nm.value, used.value

    @staticmethod
    def gzip_members_room(n, block_size):
        """Bytes that always hold the members of n bytes of input."""
        nb = max(1, (n + block_size - 1) // max(block_size, 1))
        return n + n // 16 + nb * 2800 + 64         # index: 4 bytes per 256 bytes of input; flat headers; stored worst case

    def gzip_members(self, data, block_size, level, into=None):
        """One indexed gzip member per block_size bytes of `data`; into = a buffer of the caller's with gzip_members_room()
        bytes (warm memory: a fresh result object costs a page fault per 4 KiB): the result is then a view of it."""
        p, keep = _addr(data)
        n = memoryview(data).nbytes
        cap = self.gzip_members_room(n, block_size)
        ol = C.c_uint64(0)
        if into is not None and len(into) >= cap:
            anchor = C.c_char.from_buffer(into)
            r = self.L.zngamd_gzip_members(self.h, p, n, block_size, level, C.cast(C.addressof(anchor), C.c_void_p), len(into), C.byref(ol))
            del anchor
            self._chk(r)
            return memoryview(into)[:ol.value]
        out = _Out(cap)
        self._chk(self.L.zngamd_gzip_members(self.h, p, n, block_size, level, out.addr(), cap, C.byref(ol)))
        return out.take(ol.value)

    # ---- the writer's segment index (dict-chained streams written with FLAG_FLATHDR)
    def deflate_index(self, n_units):
        """The segment index of this context's LAST deflate call: n_units rows of INDEX_STRIDE u32, as a device buffer
        (zngamd_deflate_index_dev)."""
        from . import devmem
        d = devmem.empty(self, 4 * INDEX_STRIDE * max(1, n_units))
        self._chk(self.L.zngamd_deflate_index_dev(self.h, d.vp(), n_units))
        return d

    def inflate_units_indexed_dev(self, d_def, def_len, unit_in_len, unit_out_len, d_index, d_out, out_cap, d_dict=None, dict_len=0):
        """zngamd_inflate_units_indexed_dev: unit-parallel decode of ONE dict-chained stream of this engine with its index.
        d_def / d_index / d_out / d_dict: device pointers (ints or c_void_p); unit_*_len: sequences of ints.
        -> (code, out_len); code STREAM_END, or E_INDEX / DATA_ERROR / BUF_ERROR as the C call returns them."""
        n = len(unit_in_len)
        # (numpy arrays go to the engine as they are: a list of 32 768 sizes costs a millisecond to turn into a C array)
        ka = np.ascontiguousarray(unit_in_len, dtype=np.uint32)
        kb = np.ascontiguousarray(unit_out_len, dtype=np.uint32)
        a = ka.ctypes.data_as(C.POINTER(C.c_uint32))
        b = kb.ctypes.data_as(C.POINTER(C.c_uint32))
        ol = C.c_uint64(0)
        r = self.L.zngamd_inflate_units_indexed_dev(self.h, C.c_void_p(int(d_def)), def_len, a, b, n, C.c_void_p(int(d_index)),
                                                    C.c_void_p(int(d_dict)) if d_dict else None, dict_len,
                                                    C.c_void_p(int(d_out)), out_cap, C.byref(ol))
        return r, ol.value

    def deflate_index_records(self, blocks):
        """The units of this context's LAST deflate call (made with `blocks`: a list or a block_table) as index records
        (INDEX_REC: compressed bytes, output bytes, 65 two-byte entries -- the first segment's bit offset, then every segment's
        length in bits; all zeros: a unit of stored blocks)."""
        arr, n = blocks if isinstance(blocks, tuple) and len(blocks) == 2 and isinstance(blocks[0], C.Array) else block_table(blocks)
        nu = int(self.L.zngamd_count_units(arr, n))
        uin = np.empty(nu, np.uint32); uout = np.empty(nu, np.uint32); rows = np.empty((nu, INDEX_STRIDE), np.uint32)
        self._chk(self.L.zngamd_deflate_index(self.h, nu, uin.ctypes.data_as(C.c_void_p), uout.ctypes.data_as(C.c_void_p),
                                              rows.ctypes.data_as(C.c_void_p)))
        return self._index_records(nu, uin, uout, rows)

    @staticmethod
    def _index_records(nu, uin, uout, rows):
        rec = np.zeros(nu, _index_rec_dtype())
        rec["in_len"], rec["out_len"] = uin, uout
        nseg = (uout.astype(np.int64) + 2047) >> 11
        e = rows[:, :65].astype(np.int64)
        d = np.diff(e, axis=1, prepend=0)
        d[np.arange(65)[None, :] > nseg[:, None]] = 0            # (entries behind the end-of-block one mean nothing)
        if d.min(initial=0) < 0 or d.max(initial=0) > 0xFFFF:
            raise EngineError(E_ARG, "segment index out of range")
        rec["e"] = d.astype(np.uint16)
        return rec

    # ---- spans of a seek-point index (gzip_index.py)
    def inflate_spans(self, data, spans, windows, out_cap):
        """zngamd_inflate_spans: data = the packed compressed bytes (a bytes-like object), spans = a ctypes array of Span,
        windows = the dictionaries the spans name (bytes-like).  One launch.  -> (statuses: list of int, out bytes)"""
        n = len(spans)
        p, keep = _addr(data)
        wp, wkeep = _addr(windows) if len(windows) else (None, None)
        out, op = _new_bytes(out_cap)
        st = (C.c_int32 * max(1, n))()
        self._chk(self.L.zngamd_inflate_spans(self.h, p, memoryview(data).nbytes, C.cast(spans, C.c_void_p) if n else None, n,
                                              wp, len(windows), op, out_cap, st))
        return list(st[:n]), _take(out, out_cap)

    def inflate_spans_dev(self, d_in, in_len, d_spans, n, d_windows, windows_len, d_out, out_cap, d_status):
        """zngamd_inflate_spans_dev on device pointers (ints or c_void_p); the statuses stay in d_status."""
        self._chk(self.L.zngamd_inflate_spans_dev(self.h, _dv(d_in), in_len, _dv(d_spans), n, _dv(d_windows), windows_len, _dv(d_out), out_cap,
                                                  _dv(d_status)))

    def span_stats(self, reset=True):
        """(spans launched, bytes decoded OK by the host-buffer form) since the last reset"""
        m = (C.c_uint64 * 2)()
        self._chk(self.L.zngamd_span_stats(self.h, m, 1 if reset else 0))
        return int(m[0]), int(m[1])

    def chunk_stats(self, reset=True):
        """(sync-scan hits, header-finder survivors, boundaries, chunks decoded) of the chunk-parallel decoder since the last reset"""
        m = (C.c_uint64 * 4)()
        self._chk(self.L.zngamd_chunk_stats(self.h, m, 1 if reset else 0))
        return tuple(int(x) for x in m)

    # ---- the batch API (batch.py): always the _dict entry points; zdict None = no dictionary (NULL, 0), else a bytes-like shared
    # by every item
    def inflate_batch(self, data, items, n, wbits, zdict=None):
        """zngamd_inflate_batch_dict: data = the items back to back (bytes-like), items = a ctypes array of BatchItem (out_off / out_cap
        are written).  -> (output bytes object, ctypes array of BatchResult)"""
        p, keep = _addr(data)
        dp, dkeep, dlen = _dict_arg(zdict)
        res = (BatchResult * max(n, 1))()
        box = []

        def alloc(_user, nbytes):
            obj, addr = _new_bytes(nbytes)
            box.append(obj)
            return addr.value

        fn = ALLOC_FN(alloc)
        self._chk(self.L.zngamd_inflate_batch_dict(self.h, p, memoryview(data).nbytes, C.cast(items, C.c_void_p), n, wbits, dp, dlen, fn, None,
                                                   C.cast(res, C.c_void_p)))
        return (box[0] if box else b""), res

    def deflate_batch(self, data, items, n, level, wbits, strategy=STRATEGY_DEFAULT, zdict=None):
        """zngamd_deflate_batch_dict -> (output bytes object, ctypes array of BatchResult, total); items[i].out_off is written"""
        p, keep = _addr(data)
        dp, dkeep, dlen = _dict_arg(zdict)
        res = (BatchResult * max(n, 1))()
        box = []

        def alloc(_user, nbytes):
            obj, addr = _new_bytes(nbytes)
            box.append(obj)
            return addr.value

        fn = ALLOC_FN(alloc)
        total = C.c_uint64(0)
        self._chk(self.L.zngamd_deflate_batch_dict(self.h, p, memoryview(data).nbytes, C.cast(items, C.c_void_p), n, level, wbits, strategy,
                                                   dp, dlen, fn, None, C.cast(res, C.c_void_p), C.byref(total)))
        return (box[0] if box else b""), res, total.value

    def inflate_batch_dev(self, d_in, in_len, d_items, n, wbits, count_only, d_out, out_cap, d_results, zdict=None):
        """zngamd_inflate_batch_dict_dev on device pointers (ints or c_void_p); the results stay in d_results."""
        dp, dkeep, dlen = _dict_arg(zdict)
        self._chk(self.L.zngamd_inflate_batch_dict_dev(self.h, _dv(d_in), in_len, _dv(d_items), n, wbits, dp, dlen, 1 if count_only else 0,
                                                       _dv(d_out), out_cap, _dv(d_results)))

    def deflate_batch_dev(self, d_in, in_len, items, n, level, wbits, strategy, d_out, out_cap, d_results, zdict=None):
        """zngamd_deflate_batch_dict_dev: items = a HOST ctypes array of BatchItem (out_off written) -> (code, total); code OK or
        BUF_ERROR (total = the size needed)"""
        dp, dkeep, dlen = _dict_arg(zdict)
        total = C.c_uint64(0)
        r = self._chk(self.L.zngamd_deflate_batch_dict_dev(self.h, _dv(d_in), in_len, C.cast(items, C.c_void_p), n, level, wbits, strategy,
                                                           dp, dlen, _dv(d_out), out_cap, _dv(d_results), C.byref(total)), (OK, BUF_ERROR))
        return r, total.value

    def train_dict(self, data, items, n, dict_size, k, d):
        """zngamd_train_dict: data = the samples' buffer (bytes-like), items = a ctypes array of BatchItem (in_off, in_len read)
        -> the dictionary (bytes)"""
        p, keep = _addr(data)
        out = (C.c_uint8 * dict_size)()
        ln = C.c_uint32(0)
        self._chk(self.L.zngamd_train_dict(self.h, p, memoryview(data).nbytes, C.cast(items, C.c_void_p), n, dict_size, k, d,
                                           C.cast(out, C.c_void_p), C.byref(ln)))
        return bytes(out[:ln.value])

    def train_dict_dev(self, d_in, in_len, d_items, n, dict_size, k, d):
        """zngamd_train_dict_dev on device pointers (ints or c_void_p): the samples and the item table in device memory -> (code, the
        dictionary as bytes); code OK or E_ARG (an item outside the buffer, samples outside [k, 4 GiB): no bytes)"""
        out = (C.c_uint8 * dict_size)()
        ln = C.c_uint32(0)
        r = self._chk(self.L.zngamd_train_dict_dev(self.h, _dv(d_in), in_len, _dv(d_items), n, dict_size, k, d, C.cast(out, C.c_void_p),
                                                   C.byref(ln)), (OK, E_ARG))
        return r, bytes(out[:ln.value])

    # ---- measurement
    # ---- BGZF (bgzf.py)
    @staticmethod
    def bgzf_room(n, block_size):
        """Bytes that always hold the BGZF stream of n bytes of input (EOF block included)."""
        nb = (n + block_size - 1) // max(block_size, 1)
        return n + n // 32 + nb * 626 + 28

    def bgzf_compress(self, data, block_size, level, eof=True):
        """zngamd_bgzf_compress -> (stream bytes, [(coffset, uoffset, block bytes, isize), ...] with the EOF block's row)"""
        p, keep = _addr(data)
        n = memoryview(data).nbytes
        cap = self.bgzf_room(n, block_size)
        rows = (n + block_size - 1) // max(block_size, 1) + 1
        tab = (BgzfBlock * rows)()
        out = _Out(cap)
        ol, nb = C.c_uint64(0), C.c_uint32(0)
        self._chk(self.L.zngamd_bgzf_compress(self.h, p, n, block_size, level, 1 if eof else 0, out.addr(), cap, C.byref(ol), tab, rows, C.byref(nb)))
        return out.take(ol.value), [(t.coffset, t.uoffset, t.csize, t.isize) for t in tab[:nb.value]]

    def bgzf_compress_dev(self, d_in, n, block_size, level, eof, d_out, out_cap, d_table):
        """zngamd_bgzf_compress_dev on device pointers -> (stream bytes, rows written to d_table)"""
        ol, nb = C.c_uint64(0), C.c_uint32(0)
        self._chk(self.L.zngamd_bgzf_compress_dev(self.h, _dv(d_in), n, block_size, level, 1 if eof else 0, _dv(d_out), out_cap, C.byref(ol), _dv(d_table),
                                                  C.byref(nb)))
        return ol.value, nb.value

    def gunzip_into(self, data, addr, out_cap):
        """zngamd_gunzip into memory of the caller's (an address from take_window(): a reader that decodes window after window
        into the same warm buffer) -> (code, bytes produced, n_members)"""
        p, keep = _addr(data)
        ol, nm = C.c_uint64(0), C.c_uint32(0)
        r = self.L.zngamd_gunzip(self.h, p, memoryview(data).nbytes, addr, out_cap, C.byref(ol), C.byref(nm))
        if r in (E_HIP, E_ARG):
            raise EngineError(r, self.err())
        return r, min(ol.value, out_cap), nm.value

    def bgzf_read(self, data, members, slices, out_cap):
        """zngamd_bgzf_read: data = packed compressed blocks, members / slices = tables of Member / BgzfSlice rows (ctypes arrays, or
        numpy arrays of the same layout).  -> (block statuses, slice statuses, packed result)"""
        nm, ns = len(members), len(slices)
        ptr = lambda t: C.c_void_p(t.ctypes.data) if isinstance(t, np.ndarray) else C.cast(t, C.c_void_p)
        p, keep = _addr(data)
        out, op = _new_bytes(out_cap)
        st = (C.c_int32 * max(1, nm))()
        ss = (C.c_int32 * max(1, ns))()
        self._chk(self.L.zngamd_bgzf_read(self.h, p, memoryview(data).nbytes, ptr(members) if nm else None, nm,
                                          ptr(slices) if ns else None, ns, op, out_cap, st, ss))
        return list(st[:nm]), list(ss[:ns]), _take(out, out_cap)

    def bgzf_read_dev(self, d_in, in_len, d_members, n_members, d_slices, n_slices, d_scratch, scratch_cap, d_out, out_cap, d_status,
                      d_slice_status):
        """zngamd_bgzf_read_dev on device pointers (ints or c_void_p); statuses and result stay on the device."""
        self._chk(self.L.zngamd_bgzf_read_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, _dv(d_slices), n_slices, _dv(d_scratch), scratch_cap,
                                              _dv(d_out), out_cap, _dv(d_status), _dv(d_slice_status)))

    def bgzf_count(self, data, members, delim):
        """zngamd_bgzf_count: data = packed compressed blocks, members = numpy table of MEMBER rows -> (block statuses int32[n],
        rows uint32[n, 2] of (count, flags)); the decoded bytes stay on the device"""
        win, st, keep = _window_in(data, members)
        rows = np.zeros((max(1, len(members)), 2), np.uint32)
        self._chk(self.L.zngamd_bgzf_count(self.h, *win, delim, C.c_void_p(st.ctypes.data), C.c_void_p(rows.ctypes.data)))
        return st, rows[:len(members)]

    def bgzf_line_positions(self, data, members, queries, delim):
        """zngamd_bgzf_line_positions: queries = uint32[n, 2] of (member, rank) -> (block statuses, scratch offsets uint64[n], verdicts
        int32[n])"""
        nq = len(queries)
        win, st, keep = _window_in(data, members)
        queries = np.ascontiguousarray(queries, np.uint32)
        pos = np.zeros(max(1, nq), np.uint64)
        ps = np.zeros(max(1, nq), np.int32)
        self._chk(self.L.zngamd_bgzf_line_positions(self.h, *win, C.c_void_p(queries.ctypes.data) if nq else None, nq, delim, C.c_void_p(st.ctypes.data),
                                                    C.c_void_p(pos.ctypes.data), C.c_void_p(ps.ctypes.data)))
        return st, pos[:nq], ps[:nq]

    def bgzf_read_lines(self, data, members, ranges, delim, out_cap=None):
        """zngamd_bgzf_read_lines: ranges = uint32[n, 4] of (m0, r0, m1, r1) -> (code, block statuses, range verdicts, range lengths,
        packed lines, bytes needed).  out_cap None: the result is allocated once the engine knows its size; a number: a buffer of that
        size, and code is BUF_ERROR (no lines) when the lines need more"""
        nr = len(ranges)
        win, st, keep = _window_in(data, members)
        ranges = np.ascontiguousarray(ranges, np.uint32)
        rs = np.zeros(max(1, nr), np.int32)
        rl = np.zeros(max(1, nr), np.uint32)
        ol = C.c_uint64(0)
        box = []

        def alloc(_user, nbytes):
            obj, addr = _new_bytes(nbytes)
            box.append(obj)
            return addr.value

        if out_cap is None:
            op, cap, fn = None, 0, ALLOC_FN(alloc)
        else:
            out, op = _new_bytes(out_cap)
            cap, fn = out_cap, ALLOC_FN()
        r = self._chk(self.L.zngamd_bgzf_read_lines(self.h, *win,
                                                    C.c_void_p(ranges.ctypes.data) if nr else None, nr, delim, op, cap, fn, None, C.byref(ol),
                                                    C.c_void_p(rl.ctypes.data), C.c_void_p(st.ctypes.data), C.c_void_p(rs.ctypes.data)),
                      (OK, BUF_ERROR))
        if out_cap is None:
            packed = box[0] if box else b""
        else:
            packed = _take(out, ol.value) if r == OK else b""
        return r, st, rs[:nr], rl[:nr], packed, ol.value

    def bgzf_count_dev(self, d_in, in_len, d_members, n_members, delim, d_scratch, scratch_cap, d_status, d_rows):
        """zngamd_bgzf_count_dev on device pointers; statuses and rows stay on the device."""
        self._chk(self.L.zngamd_bgzf_count_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, delim, _dv(d_scratch), scratch_cap, _dv(d_status),
                                               _dv(d_rows)))

    def bgzf_line_positions_dev(self, d_in, in_len, d_members, n_members, d_queries, n_queries, delim, d_scratch, scratch_cap, d_status, d_pos,
                                d_pos_status):
        """zngamd_bgzf_line_positions_dev on device pointers."""
        self._chk(self.L.zngamd_bgzf_line_positions_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, _dv(d_queries), n_queries, delim,
                                                        _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_pos), _dv(d_pos_status)))

    def bgzf_read_lines_dev(self, d_in, in_len, d_members, n_members, d_ranges, n_ranges, delim, d_scratch, scratch_cap, d_out, out_cap,
                            d_range_len, d_status, d_range_status):
        """zngamd_bgzf_read_lines_dev on device pointers -> (code, packed bytes, or the bytes needed when code is BUF_ERROR)"""
        ol = C.c_uint64(0)
        r = self._chk(self.L.zngamd_bgzf_read_lines_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, _dv(d_ranges), n_ranges, delim,
                                                        _dv(d_scratch), scratch_cap, _dv(d_out), out_cap, C.byref(ol), _dv(d_range_len), _dv(d_status),
                                                        _dv(d_range_status)), (OK, BUF_ERROR))
        return r, ol.value

    def bgzf_grep(self, data, members, text_off, text_end, blob, table, delim, flags, line_base=0, caps=None, mismatches=0):
        """zngamd_bgzf_grep: data = packed compressed blocks, members = numpy table of MEMBER rows, (blob, table) as
        grep_pattern_table gives them -> (code, block statuses, totals, rows (GREP_ROW_DTYPE), packed lines).  caps None: rows and
        lines are allocated once the engine knows their sizes; (rows, bytes): buffers of those sizes, and code is BUF_ERROR (nothing
        written) when the result needs more.  mismatches k > 0: zngamd_bgzf_grep_approx, a pattern matches with up to k bytes substituted"""
        if mismatches:
            return self._bgzf_grep(self.L.zngamd_bgzf_grep_approx, BgzfGrepTotals(), data, members, text_off, text_end, blob, table, delim, flags,
                                   (mismatches, line_base), caps)
        return self._bgzf_grep(self.L.zngamd_bgzf_grep, BgzfGrepTotals(), data, members, text_off, text_end, blob, table, delim, flags, (line_base,), caps)

    def bgzf_grep_records(self, data, members, text_off, text_end, blob, table, delim, flags, record_lines, match_line=-1, first_byte=-1,
                          record_base=0, caps=None, mismatches=0):
        """zngamd_bgzf_grep_records: bgzf_grep on records of record_lines lines (match_line, first_byte: -1 for none) -> (code, block
        statuses, totals (BgzfGrepRecordsTotals), rows, the records packed); nothing comes back when totals.bad is set.  mismatches k > 0:
        zngamd_bgzf_grep_records_approx"""
        if mismatches:
            return self._bgzf_grep(self.L.zngamd_bgzf_grep_records_approx, BgzfGrepRecordsTotals(), data, members, text_off, text_end, blob, table, delim,
                                   flags, (mismatches, record_lines, match_line, first_byte, record_base), caps)
        return self._bgzf_grep(self.L.zngamd_bgzf_grep_records, BgzfGrepRecordsTotals(), data, members, text_off, text_end, blob, table, delim, flags,
                               (record_lines, match_line, first_byte, record_base), caps)

    def bgzf_classify_records(self, data, members, text_off, text_end, blob, table, delim, flags, mismatches, record_lines, match_line=-1,
                              first_byte=-1, record_base=0, caps=None):
        """zngamd_bgzf_classify_records: every record's nearest pattern -> (code, block statuses, totals (BgzfClassifyTotals), class rows
        (CLASS_ROW_DTYPE, one per record in record order), rows (GREP_ROW_DTYPE, ordered by class then number; reserved: the class row),
        the records packed in that order); rows and records only with BGZF_CLASSIFY_GROUP in flags; nothing comes back when totals.bad
        is set.  caps None: the arrays are allocated once the engine knows their sizes; (class rows, rows, bytes): buffers of those sizes,
        and code is BUF_ERROR (nothing written) when the result needs more"""
        win, st, keep = _window_in(data, members)
        table = np.ascontiguousarray(table, np.uint32)
        tot = BgzfClassifyTotals()
        group = bool(flags & BGZF_CLASSIFY_GROUP)
        box = []

        def alloc(_user, nbytes):
            if not box:
                arr = np.empty(nbytes // CLASS_ROW_DTYPE.itemsize, CLASS_ROW_DTYPE)
            elif len(box) == 1:
                arr = np.empty(nbytes // GREP_ROW_DTYPE.itemsize, GREP_ROW_DTYPE)
            else:
                obj, addr = _new_bytes(nbytes)
                box.append(obj)
                return addr.value
            box.append(arr)
            return arr.ctypes.data

        if caps is None:
            cp, ccap, rp, rcap, op, ocap, fn = None, 0, None, 0, None, 0, ALLOC_FN(alloc)
        else:
            ccap, rcap, ocap = caps
            cls, rows = np.zeros(max(1, ccap), CLASS_ROW_DTYPE), np.zeros(max(1, rcap), GREP_ROW_DTYPE)
            out, op = _new_bytes(ocap)
            cp, rp, fn = C.c_void_p(cls.ctypes.data) if ccap else None, C.c_void_p(rows.ctypes.data) if rcap else None, ALLOC_FN()
            if not ocap:
                op = None
        bp, bkeep = _addr(blob)
        r = self._chk(self.L.zngamd_bgzf_classify_records(self.h, *win,
                                                          text_off, text_end, bp, len(blob), C.c_void_p(table.ctypes.data), len(table), delim, flags,
                                                          mismatches, record_lines, match_line, first_byte, record_base, C.c_void_p(st.ctypes.data),
                                                          cp, ccap, rp, rcap, op, ocap, fn, None, C.byref(tot)), (OK, BUF_ERROR))
        got = r == OK and tot.covered and tot.seen and not tot.bad
        if caps is None:
            cls_out = box[0] if got else np.empty(0, CLASS_ROW_DTYPE)
            rows_out = box[1] if got and group else np.empty(0, GREP_ROW_DTYPE)
            packed = box[2] if got and group else b""
        else:
            cls_out = cls[:tot.seen] if got else np.empty(0, CLASS_ROW_DTYPE)
            rows_out = rows[:tot.seen] if got and group else np.empty(0, GREP_ROW_DTYPE)
            packed = _take(out, tot.bytes) if got and group else b""
        return r, st, tot, cls_out, rows_out, packed

    def bgzf_classify_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, blob, table, delim, flags, mismatches, record_lines,
                                  match_line, first_byte, record_base, d_scratch, scratch_cap, d_status, d_class, class_cap, d_rows, rows_cap, d_out,
                                  out_cap):
        """zngamd_bgzf_classify_records_dev on device pointers (the patterns: host memory) -> (code, totals); class rows, rows and records
        stay on the device"""
        table = np.ascontiguousarray(table, np.uint32)
        tot = BgzfClassifyTotals()
        bp, bkeep = _addr(blob)
        r = self._chk(self.L.zngamd_bgzf_classify_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, bp, len(blob),
                                                              C.c_void_p(table.ctypes.data), len(table), delim, flags, mismatches, record_lines,
                                                              match_line, first_byte, record_base, _dv(d_scratch), scratch_cap, _dv(d_status),
                                                              _dv(d_class), class_cap, _dv(d_rows), rows_cap, _dv(d_out), out_cap, C.byref(tot)),
                      (OK, BUF_ERROR))
        return r, tot

    def bgzf_partition_records(self, data, members, text_off, text_end, delim, flags, record_lines, first_byte, record_base, labels, n_classes,
                               caps=None):
        """zngamd_bgzf_partition_records: the records split by labels (a uint16 array; entry r belongs to record record_base + r;
        BGZF_PARTITION_DROP: the record is dropped) -> (code, block statuses, totals (BgzfPartitionTotals), records per class, bytes per class
        (uint64[n_classes]), rows (GREP_ROW_DTYPE, ordered by class then number; reserved: the label), the kept records packed in that
        order); rows and records only with BGZF_CLASSIFY_GROUP in flags; nothing comes back when totals.bad or totals.labels_short is set.
        caps None: the arrays are allocated once the engine knows their sizes; (rows, bytes): buffers of those sizes, and code is
        BUF_ERROR (nothing written) when the result needs more"""
        win, st, keep = _window_in(data, members)
        labels = np.ascontiguousarray(labels, np.uint16)
        tot = BgzfPartitionTotals()
        crec, cbytes = np.zeros(max(1, n_classes), np.uint64), np.zeros(max(1, n_classes), np.uint64)
        box = []

        def alloc(_user, nbytes):
            if not box:
                arr = np.empty(nbytes // GREP_ROW_DTYPE.itemsize, GREP_ROW_DTYPE)
                box.append(arr)
                return arr.ctypes.data
            obj, addr = _new_bytes(nbytes)
            box.append(obj)
            return addr.value

        if caps is None:
            rp, rcap, op, ocap, fn = None, 0, None, 0, ALLOC_FN(alloc)
        else:
            rcap, ocap = caps
            rows = np.zeros(max(1, rcap), GREP_ROW_DTYPE)
            out, op = _new_bytes(ocap)
            rp, fn = C.c_void_p(rows.ctypes.data) if rcap else None, ALLOC_FN()
            if not ocap:
                op = None
        r = self._chk(self.L.zngamd_bgzf_partition_records(self.h, *win,
                                                           text_off, text_end, delim, flags, record_lines, first_byte, record_base,
                                                           C.c_void_p(st.ctypes.data), rp, rcap, op, ocap, fn, None,
                                                           C.c_void_p(labels.ctypes.data) if len(labels) else None, len(labels), n_classes,
                                                           C.c_void_p(crec.ctypes.data), C.c_void_p(cbytes.ctypes.data), C.byref(tot)), (OK, BUF_ERROR))
        kept = tot.seen - tot.dropped
        got = r == OK and tot.covered and kept and not tot.bad and not tot.labels_short and bool(flags & BGZF_CLASSIFY_GROUP)
        if caps is None:
            rows_out, packed = (box[0], box[1]) if got else (np.empty(0, GREP_ROW_DTYPE), b"")
        else:
            rows_out, packed = (rows[:kept], _take(out, tot.bytes)) if got else (np.empty(0, GREP_ROW_DTYPE), b"")
        return r, st, tot, crec[:n_classes], cbytes[:n_classes], rows_out, packed

    def bgzf_partition_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, record_lines, first_byte, record_base,
                                   d_scratch, scratch_cap, d_status, d_rows, rows_cap, d_out, out_cap, d_labels, n_labels, n_classes):
        """zngamd_bgzf_partition_records_dev on device pointers -> (code, totals, records per class, bytes per class); rows and records stay
        on the device"""
        tot = BgzfPartitionTotals()
        crec, cbytes = np.zeros(max(1, n_classes), np.uint64), np.zeros(max(1, n_classes), np.uint64)
        r = self._chk(self.L.zngamd_bgzf_partition_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                               record_lines, first_byte, record_base, _dv(d_scratch), scratch_cap, _dv(d_status),
                                                               _dv(d_rows), rows_cap, _dv(d_out), out_cap, _dv(d_labels), n_labels, n_classes,
                                                               C.c_void_p(crec.ctypes.data), C.c_void_p(cbytes.ctypes.data), C.byref(tot)),
                      (OK, BUF_ERROR))
        return r, tot, crec[:n_classes], cbytes[:n_classes]

    def bgzf_trim_records(self, data, members, text_off, text_end, blob, table, delim, flags, conf, record_base=0, drop=None, caps=None):
        """zngamd_bgzf_trim_records: every record cut by the rule of conf (a BgzfTrimConf) and the adapters (blob, table: as bgzf_grep takes
        patterns; the table may be empty) -> (code, block statuses, totals (BgzfTrimTotals), trim rows (TRIM_ROW_DTYPE, one per record in
        record order), rows (GREP_ROW_DTYPE: the kept records, then with BGZF_TRIM_KEEP_SHORT the too-short ones; len: the bytes as
        written), the records as written in that order); rows and records only with BGZF_CLASSIFY_GROUP in flags; nothing comes back
        when totals.bad or totals.drop_short is set.  drop: None or a uint8 array, entry r belongs to record record_base + r.  caps None:
        the arrays are allocated once the engine knows their sizes; (trim rows, rows, bytes): buffers of those sizes, and code is
        BUF_ERROR (nothing written) when the result needs more"""
        win, st, keep = _window_in(data, members)
        table = np.ascontiguousarray(table, np.uint32).reshape(-1, 2)
        tot = BgzfTrimTotals()
        group = bool(flags & BGZF_CLASSIFY_GROUP)
        box = []

        def alloc(_user, nbytes):
            if not box:
                arr = np.empty(nbytes // TRIM_ROW_DTYPE.itemsize, TRIM_ROW_DTYPE)
            elif len(box) == 1:
                arr = np.empty(nbytes // GREP_ROW_DTYPE.itemsize, GREP_ROW_DTYPE)
            else:
                obj, addr = _new_bytes(nbytes)
                box.append(obj)
                return addr.value
            box.append(arr)
            return arr.ctypes.data

        if caps is None:
            tp, tcap, rp, rcap, op, ocap, fn = None, 0, None, 0, None, 0, ALLOC_FN(alloc)
        else:
            tcap, rcap, ocap = caps
            trim, rows = np.zeros(max(1, tcap), TRIM_ROW_DTYPE), np.zeros(max(1, rcap), GREP_ROW_DTYPE)
            out, op = _new_bytes(ocap)
            tp, rp, fn = C.c_void_p(trim.ctypes.data) if tcap else None, C.c_void_p(rows.ctypes.data) if rcap else None, ALLOC_FN()
            if not ocap:
                op = None
        if drop is not None:                               # (an empty mask is still a mask: every record lies beyond it)
            drop = np.ascontiguousarray(drop, np.uint8)
            mask = drop if len(drop) else np.zeros(1, np.uint8)
            dp, nd = C.c_void_p(mask.ctypes.data), len(drop)
        else:
            dp, nd = None, 0
        bp, bkeep = _addr(blob) if len(table) else (None, None)
        r = self._chk(self.L.zngamd_bgzf_trim_records(self.h, *win,
                                                      text_off, text_end, bp, len(blob) if len(table) else 0,
                                                      C.c_void_p(table.ctypes.data) if len(table) else None, len(table), delim, flags, C.byref(conf),
                                                      record_base, C.c_void_p(st.ctypes.data), dp, nd, tp, tcap, rp, rcap, op, ocap, fn, None,
                                                      C.byref(tot)), (OK, BUF_ERROR))
        got = r == OK and tot.covered and tot.seen and not tot.bad and not tot.drop_short
        n = tot.kept + (tot.too_short if conf.flags & BGZF_TRIM_KEEP_SHORT else 0) if got and group else 0
        if caps is None:
            trim_out = box[0] if got else np.empty(0, TRIM_ROW_DTYPE)
            rows_out, packed = (box[1], box[2]) if n else (np.empty(0, GREP_ROW_DTYPE), b"")
        else:
            trim_out = trim[:tot.seen] if got else np.empty(0, TRIM_ROW_DTYPE)
            rows_out, packed = (rows[:n], _take(out, tot.bytes)) if n else (np.empty(0, GREP_ROW_DTYPE), b"")
        return r, st, tot, trim_out, rows_out, packed

    def bgzf_trim_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, blob, table, delim, flags, conf, record_base, d_scratch,
                              scratch_cap, d_status, d_drop, n_drop, d_trim, trim_cap, d_rows, rows_cap, d_out, out_cap):
        """zngamd_bgzf_trim_records_dev on device pointers (the adapters and conf: host memory) -> (code, totals); trim rows, rows and records
        stay on the device"""
        table = np.ascontiguousarray(table, np.uint32).reshape(-1, 2)
        tot = BgzfTrimTotals()
        bp, bkeep = _addr(blob) if len(table) else (None, None)
        r = self._chk(self.L.zngamd_bgzf_trim_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, bp,
                                                          len(blob) if len(table) else 0, C.c_void_p(table.ctypes.data) if len(table) else None,
                                                          len(table), delim, flags, C.byref(conf), record_base, _dv(d_scratch), scratch_cap, _dv(d_status),
                                                          _dv(d_drop), n_drop, _dv(d_trim), trim_cap, _dv(d_rows), rows_cap, _dv(d_out), out_cap, C.byref(tot)),
                      (OK, BUF_ERROR))
        return r, tot

    def bgzf_overlap_records(self, data, members, text_off, text_end, delim, flags, conf, record_base=0, caps=None):
        """zngamd_bgzf_overlap_records: every pair judged by the rule of conf (a BgzfOverlapConf) -> (code, block statuses, totals
        (BgzfOverlapTotals), overlap rows (OVERLAP_ROW_DTYPE, one per pair in record order), rows (GREP_ROW_DTYPE: the merged pairs, then
        with BGZF_OVERLAP_KEEP_UNMERGED the others; len: the bytes as written), the records as written in that order); rows and records
        only with BGZF_CLASSIFY_GROUP in flags; nothing comes back when totals.bad is set.  caps None: the arrays are allocated once the
        engine knows their sizes; (overlap rows, rows, bytes): buffers of those sizes, and code is BUF_ERROR (nothing written) when the
        result needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfOverlapTotals()
        group = bool(flags & BGZF_CLASSIFY_GROUP)
        box = []

        def alloc(_user, nbytes):
            if not box:
                arr = np.empty(nbytes // OVERLAP_ROW_DTYPE.itemsize, OVERLAP_ROW_DTYPE)
            elif len(box) == 1:
                arr = np.empty(nbytes // GREP_ROW_DTYPE.itemsize, GREP_ROW_DTYPE)
            else:
                obj, addr = _new_bytes(nbytes)
                box.append(obj)
                return addr.value
            box.append(arr)
            return arr.ctypes.data

        if caps is None:
            vrp, vcap, rp, rcap, op, ocap, fn = None, 0, None, 0, None, 0, ALLOC_FN(alloc)
        else:
            vcap, rcap, ocap = caps
            ovl, rows = np.zeros(max(1, vcap), OVERLAP_ROW_DTYPE), np.zeros(max(1, rcap), GREP_ROW_DTYPE)
            out, op = _new_bytes(ocap)
            vrp, rp, fn = C.c_void_p(ovl.ctypes.data) if vcap else None, C.c_void_p(rows.ctypes.data) if rcap else None, ALLOC_FN()
            if not ocap:
                op = None
        r = self._chk(self.L.zngamd_bgzf_overlap_records(self.h, *win,
                                                         text_off, text_end, delim, flags, C.byref(conf), record_base, C.c_void_p(st.ctypes.data),
                                                         vrp, vcap, rp, rcap, op, ocap, fn, None, C.byref(tot)), (OK, BUF_ERROR))
        got = r == OK and tot.covered and tot.seen and not tot.bad
        n = tot.merged + (tot.seen - tot.merged if conf.flags & BGZF_OVERLAP_KEEP_UNMERGED else 0) if got and group else 0
        if caps is None:
            ovl_out = box[0] if got else np.empty(0, OVERLAP_ROW_DTYPE)
            rows_out, packed = (box[1], box[2]) if n else (np.empty(0, GREP_ROW_DTYPE), b"")
        else:
            ovl_out = ovl[:tot.seen] if got else np.empty(0, OVERLAP_ROW_DTYPE)
            rows_out, packed = (rows[:n], _take(out, tot.bytes)) if n else (np.empty(0, GREP_ROW_DTYPE), b"")
        return r, st, tot, ovl_out, rows_out, packed

    def bgzf_overlap_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, conf, record_base, d_scratch, scratch_cap,
                                 d_status, d_overlap, overlap_cap, d_rows, rows_cap, d_out, out_cap):
        """zngamd_bgzf_overlap_records_dev on device pointers (conf: host memory) -> (code, totals); overlap rows, rows and records stay on
        the device"""
        tot = BgzfOverlapTotals()
        r = self._chk(self.L.zngamd_bgzf_overlap_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                             C.byref(conf), record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_overlap),
                                                             overlap_cap, _dv(d_rows), rows_cap, _dv(d_out), out_cap, C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_qc_records(self, data, members, text_off, text_end, delim, flags, conf, record_base=0, caps=None):
        """zngamd_bgzf_qc_records: every record counted by the rule of conf (a BgzfQcConf) -> (code, block statuses, totals (BgzfQcTotals),
        tables (uint64, bgzf_qc_table_words(conf.cycles) words: bgzf_qc_split() names them), rows (QC_ROW_DTYPE, one per record in record
        order; empty without BGZF_QC_ROWS in conf.flags or when totals.bad is set)).  caps None: the tables are sized for conf.cycles and
        the rows are allocated once the engine knows how many there are; (table words, rows): buffers of those sizes, and code is
        BUF_ERROR when the result needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfQcTotals()
        want = bool(conf.flags & BGZF_QC_ROWS)
        tcap, rcap = (bgzf_qc_table_words(conf.cycles), None) if caps is None else caps
        out = _RowsOut(QC_ROW_DTYPE, rcap)
        rp = out.ptr if out.cap or want else None                           # (no rows asked for and no room for any: no pointer either)
        tables = np.full(max(1, tcap), 0x5A5A5A5A5A5A5A5A, np.uint64)       # (the engine overwrites what it is given)
        r = self._chk(self.L.zngamd_bgzf_qc_records(self.h, *win, text_off, text_end, delim, flags, C.byref(conf), record_base, C.c_void_p(st.ctypes.data),
                                                    C.c_void_p(tables.ctypes.data), tcap, rp, out.cap, out.fn, None, C.byref(tot)), (OK, BUF_ERROR))
        return r, st, tot, tables[:tcap], out.take(r == OK and want and tot.covered and tot.seen and not tot.bad, tot.seen)

    def bgzf_qc_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, conf, record_base, d_scratch, scratch_cap,
                            d_status, d_tables, tables_cap, d_rows, rows_cap):
        """zngamd_bgzf_qc_records_dev on device pointers (conf: host memory) -> (code, totals); tables and rows stay on the device"""
        tot = BgzfQcTotals()
        r = self._chk(self.L.zngamd_bgzf_qc_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                        C.byref(conf), record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_tables), tables_cap,
                                                        _dv(d_rows), rows_cap, C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_key_records(self, data, members, text_off, text_end, delim, flags, conf, record_base=0, caps=None):
        """zngamd_bgzf_key_records: the key of every record by the rule of conf (a BgzfKeyConf) -> (code, block statuses, totals
        (BgzfKeyTotals), rows (KEY_ROW_DTYPE, one per record in record order; empty when totals.bad is set)).  caps None: the rows are
        allocated once the engine knows how many there are; an integer: a buffer of that many rows, and code is BUF_ERROR when the
        result needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfKeyTotals()
        out = _RowsOut(KEY_ROW_DTYPE, caps)
        r = self._chk(self.L.zngamd_bgzf_key_records(self.h, *win, text_off, text_end, delim, flags, C.byref(conf), record_base, C.c_void_p(st.ctypes.data),
                                                     out.ptr, out.cap, out.fn, None, C.byref(tot)), (OK, BUF_ERROR))
        return r, st, tot, out.take(r == OK and tot.covered and tot.seen and not tot.bad, tot.seen)

    def bgzf_key_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, conf, record_base, d_scratch, scratch_cap,
                             d_status, d_rows, rows_cap):
        """zngamd_bgzf_key_records_dev on device pointers (conf: host memory) -> (code, totals); the rows stay on the device"""
        tot = BgzfKeyTotals()
        r = self._chk(self.L.zngamd_bgzf_key_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                         C.byref(conf), record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_rows), rows_cap,
                                                         C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def dedup_keys(self, keys, want_first=True, want_count=True):
        """zngamd_dedup_keys: keys (KEY_ROW_DTYPE) -> (totals (DedupTotals), first (uint64, or None), count (uint32, or None))"""
        keys = np.ascontiguousarray(keys, KEY_ROW_DTYPE)
        n = len(keys)
        first = np.empty(n, np.uint64) if want_first else None
        count = np.empty(n, np.uint32) if want_count else None
        tot = DedupTotals()
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None and len(a) else None
        self._chk(self.L.zngamd_dedup_keys(self.h, p(keys), n, p(first), p(count), C.byref(tot)))
        return tot, first, count

    def dedup_keys_dev(self, d_keys, n, d_scratch, scratch_cap, d_first, d_count):
        """zngamd_dedup_keys_dev on device pointers -> (code, totals); first and count (either may be 0) stay on the device"""
        tot = DedupTotals()
        r = self._chk(self.L.zngamd_dedup_keys_dev(self.h, _dv(d_keys), n, _dv(d_scratch), scratch_cap, _dv(d_first), _dv(d_count), C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def _kmer_set(self, handle):
        kset = DeviceKmerSet(self, handle)
        self.__dict__.setdefault("_kmer_sets", weakref.WeakSet()).add(kset)
        return kset

    def kmer_set_build(self, references, k, flags=KMER_CANONICAL):
        """zngamd_kmer_set_build: references (a list of bytes-likes, at most 64) -> DeviceKmerSet; the set is built on the GPU"""
        refs = [bytes(r) for r in references]
        blob = b"".join(refs)
        offsets = np.zeros(len(refs) + 1, np.uint64)
        np.cumsum([len(r) for r in refs], out=offsets[1:])
        h, info = C.c_void_p(), KmerSetInfo()
        self._chk(self.L.zngamd_kmer_set_build(self.h, C.cast(C.c_char_p(blob), C.c_void_p) if blob else None, C.c_void_p(offsets.ctypes.data), len(refs), k,
                                               flags, C.byref(h), C.byref(info)))
        return self._kmer_set(h)

    def kmer_set_load(self, k, flags, n_refs, codes, masks):
        """zngamd_kmer_set_load: (code, mask) pairs (uint64 arrays of equal length) -> DeviceKmerSet"""
        codes, masks = np.ascontiguousarray(codes, np.uint64), np.ascontiguousarray(masks, np.uint64)
        n = len(codes)
        if len(masks) != n:
            raise ValueError("codes and masks are of equal length")
        p = lambda a: C.c_void_p(a.ctypes.data) if n else None
        h, info = C.c_void_p(), KmerSetInfo()
        self._chk(self.L.zngamd_kmer_set_load(self.h, k, flags, n_refs, p(codes), p(masks), n, C.byref(h), C.byref(info)))
        return self._kmer_set(h)

    def bgzf_screen_records(self, data, members, text_off, text_end, delim, flags, conf, kset, record_base=0, caps=None):
        """zngamd_bgzf_screen_records: every k-mer of every record looked up in kset (a DeviceKmerSet of this context) by conf (a
        BgzfScreenConf) -> (code, block statuses, totals (BgzfScreenTotals), rows (SCREEN_ROW_DTYPE, one per record in record order; empty
        when totals.bad is set)).  caps None: the rows are allocated once the engine knows how many there are; an integer: a buffer of
        that many rows, and code is BUF_ERROR when the result needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfScreenTotals()
        out = _RowsOut(SCREEN_ROW_DTYPE, caps)
        r = self._chk(self.L.zngamd_bgzf_screen_records(self.h, *win, text_off, text_end, delim, flags, C.byref(conf), kset.h, record_base,
                                                        C.c_void_p(st.ctypes.data), out.ptr, out.cap, out.fn, None, C.byref(tot)), (OK, BUF_ERROR))
        return r, st, tot, out.take(r == OK and tot.covered and tot.seen and not tot.bad, tot.seen)

    def bgzf_screen_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, conf, kset, record_base, d_scratch, scratch_cap,
                                d_status, d_rows, rows_cap):
        """zngamd_bgzf_screen_records_dev on device pointers (conf: host memory) -> (code, totals); the rows stay on the device"""
        tot = BgzfScreenTotals()
        r = self._chk(self.L.zngamd_bgzf_screen_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                            C.byref(conf), kset.h, record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_rows), rows_cap,
                                                            C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def kmer_counter_new(self, k, flags=KMER_CANONICAL, room=0):
        """zngamd_kmer_counter_new: an empty counter with a table for `room` codes -> DeviceKmerCounter"""
        h = C.c_void_p()
        self._chk(self.L.zngamd_kmer_counter_new(self.h, k, flags, room, C.byref(h)))
        counter = DeviceKmerCounter(self, h)
        self.__dict__.setdefault("_kmer_sets", weakref.WeakSet()).add(counter)      # (freed before the context, as a set is)
        return counter

    def bgzf_count_kmers(self, data, members, text_off, text_end, delim, flags, conf, counter, record_base=0):
        """zngamd_bgzf_count_kmers: every valid k-mer of every record added to counter (a DeviceKmerCounter of this context) by conf (a
        BgzfCountConf) -> (code, block statuses, totals (BgzfCountTotals)); code is BUF_ERROR when the table lacks the room for the
        window (nothing was launched: reserve text_end - text_off first)"""
        win, st, keep = _window_in(data, members)
        tot = BgzfCountTotals()
        r = self._chk(self.L.zngamd_bgzf_count_kmers(self.h, *win,
                                                     text_off, text_end, delim, flags, C.byref(conf), counter._handle(), record_base,
                                                     C.c_void_p(st.ctypes.data), C.byref(tot)), (OK, BUF_ERROR))
        return r, st, tot

    def bgzf_count_kmers_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, conf, counter, record_base, d_scratch, scratch_cap,
                             d_status):
        """zngamd_bgzf_count_kmers_dev on device pointers (conf: host memory) -> (code, totals)"""
        tot = BgzfCountTotals()
        r = self._chk(self.L.zngamd_bgzf_count_kmers_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                         C.byref(conf), counter._handle(), record_base, _dv(d_scratch), scratch_cap, _dv(d_status),
                                                         C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_sort_key_records(self, data, members, text_off, text_end, delim, flags, conf, record_base=0, caps=None):
        """zngamd_bgzf_sort_key_records: the sort key of every record by conf (a BgzfSortConf) -> (code, block statuses, totals
        (BgzfSortKeyTotals), rows (uint8 of shape (seen, W)), lengths (uint32); both empty when totals.bad is set).  caps None: the
        arrays are allocated once the engine knows how many rows there are; an integer: buffers of that many rows, and code is BUF_ERROR
        when the result needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfSortKeyTotals()
        W = sum(q.width if q.kind == BGZF_SORT_BYTES else 8 if q.kind == BGZF_SORT_NUMBER else 4 for q in conf.part[:conf.n_parts]) + 7 & ~7
        box = []

        def alloc(_user, nbytes):
            box.append(np.empty(nbytes, np.uint8))
            return box[-1].ctypes.data

        if caps is None:
            rp, lp, rcap, fn = None, None, 0, ALLOC_FN(alloc)
        else:
            rcap = caps
            rows, lens = np.zeros(max(1, rcap * W), np.uint8), np.zeros(max(1, rcap), np.uint32)
            rp, lp, fn = C.c_void_p(rows.ctypes.data), C.c_void_p(lens.ctypes.data), ALLOC_FN()
        r = self._chk(self.L.zngamd_bgzf_sort_key_records(self.h, *win,
                                                          text_off, text_end, delim, flags, C.byref(conf), record_base, C.c_void_p(st.ctypes.data),
                                                          rp, lp, rcap, fn, None, C.byref(tot)), (OK, BUF_ERROR))
        got = r == OK and tot.covered and tot.seen and not tot.bad
        n = tot.seen if got else 0
        if caps is None and got:
            rows_out = box[0] if W else np.empty(0, np.uint8)
            lens_out = box[-1].view(np.uint32)
        elif got:
            rows_out, lens_out = rows[:n * W], lens[:n]
        else:
            rows_out, lens_out = np.empty(0, np.uint8), np.empty(0, np.uint32)
        return r, st, tot, rows_out.reshape(n, W), lens_out

    def bgzf_sort_key_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, conf, record_base, d_scratch, scratch_cap,
                                  d_status, d_rows, d_lengths, rows_cap):
        """zngamd_bgzf_sort_key_records_dev on device pointers (conf: host memory) -> (code, totals); rows and lengths stay on the device"""
        tot = BgzfSortKeyTotals()
        r = self._chk(self.L.zngamd_bgzf_sort_key_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                              C.byref(conf), record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_rows), _dv(d_lengths),
                                                              rows_cap, C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def sort_keys(self, keys, want_rank=False):
        """zngamd_sort_keys: keys (C-contiguous uint8 of shape (n, W)) -> (order (uint32), rank (uint32, or None))"""
        n, w = keys.shape
        order = np.empty(n, np.uint32)
        rank = np.empty(n, np.uint32) if want_rank else None
        p = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None
        self._chk(self.L.zngamd_sort_keys(self.h, p(keys), n, w, p(order), p(rank)))
        return order, rank

    def sort_keys_dev(self, d_keys, n, width, d_scratch, scratch_cap, d_order, d_rank):
        """zngamd_sort_keys_dev on device pointers -> code; order and rank (which may be 0) stay on the device"""
        return self._chk(self.L.zngamd_sort_keys_dev(self.h, _dv(d_keys), n, width, _dv(d_scratch), scratch_cap, _dv(d_order), _dv(d_rank)), (OK, BUF_ERROR))

    def bgzf_place_records(self, data, members, text_off, text_end, delim, flags, record_lines, first_byte, record_base, dst, length, d_out, out_cap):
        """zngamd_bgzf_place_records: record record_base + r copied to the device buffer d_out + dst[r] (uint64; BGZF_PLACE_SKIP: not in
        this pass) with length[r] (uint32) as bgzf_sort_key_records reported it -> (code, block statuses, totals (BgzfPlaceTotals))"""
        win, st, keep = _window_in(data, members)
        dst, length = np.ascontiguousarray(dst, np.uint64), np.ascontiguousarray(length, np.uint32)
        n = min(len(dst), len(length))
        tot = BgzfPlaceTotals()
        r = self._chk(self.L.zngamd_bgzf_place_records(self.h, *win,
                                                       text_off, text_end, delim, flags, record_lines, first_byte, record_base,
                                                       C.c_void_p(st.ctypes.data), C.c_void_p(dst.ctypes.data) if n else None,
                                                       C.c_void_p(length.ctypes.data) if n else None, n, C.c_void_p(int(d_out)) if d_out else None, out_cap,
                                                       C.byref(tot)))
        return r, st, tot

    def bgzf_place_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, record_lines, first_byte, record_base,
                               d_scratch, scratch_cap, d_status, d_dst, d_length, n, d_out, out_cap):
        """zngamd_bgzf_place_records_dev on device pointers -> (code, totals)"""
        tot = BgzfPlaceTotals()
        r = self._chk(self.L.zngamd_bgzf_place_records_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags,
                                                           record_lines, first_byte, record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_dst),
                                                           _dv(d_length), n, _dv(d_out), out_cap, C.byref(tot)))
        return r, tot

    def _bgzf_grep(self, fn_c, tot, data, members, text_off, text_end, blob, table, delim, flags, extra, caps):
        win, st, keep = _window_in(data, members)
        table = np.ascontiguousarray(table, np.uint32)
        box = []

        def alloc(_user, nbytes):
            if not box:
                arr = np.empty(nbytes // GREP_ROW_DTYPE.itemsize, GREP_ROW_DTYPE)
                box.append(arr)
                return arr.ctypes.data
            obj, addr = _new_bytes(nbytes)
            box.append(obj)
            return addr.value

        if caps is None:
            rp, rcap, op, ocap, fn = None, 0, None, 0, ALLOC_FN(alloc)
        else:
            rows = np.zeros(max(1, caps[0]), GREP_ROW_DTYPE)
            out, op = _new_bytes(caps[1])
            rp, rcap, ocap, fn = C.c_void_p(rows.ctypes.data), caps[0], caps[1], ALLOC_FN()
            if not ocap:
                op = None
            if not rcap:
                rp = None
        bp, bkeep = _addr(blob)
        r = self._chk(fn_c(self.h, *win, text_off, text_end, bp, len(blob),
                           C.c_void_p(table.ctypes.data), len(table), delim, flags, *extra, C.c_void_p(st.ctypes.data), rp, rcap, op, ocap, fn, None,
                           C.byref(tot)), (OK, BUF_ERROR))
        got = r == OK and tot.covered and tot.matched and not flags & BGZF_GREP_COUNT_ONLY and not getattr(tot, "bad", 0)
        if caps is None:
            rows_out = box[0] if got else np.empty(0, GREP_ROW_DTYPE)
            packed = box[1] if got else b""
        else:
            rows_out = rows[:tot.matched] if got else np.empty(0, GREP_ROW_DTYPE)
            packed = _take(out, tot.bytes) if got else b""
        return r, st, tot, rows_out, packed

    def bgzf_grep_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, blob, table, delim, flags, line_base, d_scratch,
                      scratch_cap, d_status, d_rows, rows_cap, d_out, out_cap, mismatches=0):
        """zngamd_bgzf_grep_dev (mismatches > 0: zngamd_bgzf_grep_approx_dev) on device pointers (the patterns: host memory) -> (code, totals);
        rows and lines stay on the device"""
        table = np.ascontiguousarray(table, np.uint32)
        tot = BgzfGrepTotals()
        bp, bkeep = _addr(blob)
        fn, k = (self.L.zngamd_bgzf_grep_approx_dev, (mismatches,)) if mismatches else (self.L.zngamd_bgzf_grep_dev, ())
        r = self._chk(fn(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, bp, len(blob), C.c_void_p(table.ctypes.data), len(table),
                         delim, flags, *k, line_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_rows), rows_cap, _dv(d_out), out_cap, C.byref(tot)),
                      (OK, BUF_ERROR))
        return r, tot

    def bgzf_grep_records_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, blob, table, delim, flags, record_lines, match_line,
                              first_byte, record_base, d_scratch, scratch_cap, d_status, d_rows, rows_cap, d_out, out_cap, mismatches=0):
        """zngamd_bgzf_grep_records_dev (mismatches > 0: zngamd_bgzf_grep_records_approx_dev) on device pointers (the patterns: host memory)
        -> (code, totals); rows and records stay on the device"""
        table = np.ascontiguousarray(table, np.uint32)
        tot = BgzfGrepRecordsTotals()
        bp, bkeep = _addr(blob)
        fn, k = (self.L.zngamd_bgzf_grep_records_approx_dev, (mismatches,)) if mismatches else (self.L.zngamd_bgzf_grep_records_dev, ())
        r = self._chk(fn(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, bp, len(blob), C.c_void_p(table.ctypes.data), len(table),
                         delim, flags, *k, record_lines, match_line, first_byte, record_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_rows), rows_cap,
                         _dv(d_out), out_cap, C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_tabix(self, data, members, text_off, text_end, conf, delim, flags, line_base=0, caps=None):
        """zngamd_bgzf_tabix: conf = (format, col_seq, col_beg, col_end, meta, skip) -> (code, block statuses, totals, names
        (TABIX_NAME_DTYPE), the names packed, bins (TABIX_BIN_DTYPE), wins (TABIX_WIN_DTYPE)).  caps None: the tables are allocated once
        the engine knows their sizes; (names, name bytes, bins, wins): buffers of those sizes, and code is BUF_ERROR (nothing written)
        when a table needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfTabixTotals()
        cf = TabixConf(*[int(x) for x in conf])
        dts = (TABIX_NAME_DTYPE, np.dtype("u1"), TABIX_BIN_DTYPE, TABIX_WIN_DTYPE)
        box = []

        def alloc(_user, nbytes):
            k = len(box) + (1 if box and not tot.name_bytes else 0)      # (no call for names that are all empty)
            arr = np.empty(nbytes // dts[k].itemsize, dts[k])
            box.append(arr)
            return arr.ctypes.data

        if caps is None:
            ptrs, fn = [None, 0] * 4, ALLOC_FN(alloc)
        else:
            bufs = [np.zeros(max(1, n), dt) for n, dt in zip(caps, dts)]
            ptrs, fn = [], ALLOC_FN()
            for b, n in zip(bufs, caps):
                ptrs += [C.c_void_p(b.ctypes.data) if n else None, n]
        r = self._chk(self.L.zngamd_bgzf_tabix(self.h, *win, text_off,
                                               text_end, C.byref(cf), delim, flags, line_base, C.c_void_p(st.ctypes.data), *ptrs, fn, None,
                                               C.byref(tot)), (OK, BUF_ERROR))
        counts = (tot.n_names, tot.name_bytes, tot.n_bins, tot.n_wins)
        if r != OK or not tot.covered or not tot.n_names:
            out = [np.empty(0, dt) for dt in dts]
        elif caps is None:
            if not tot.name_bytes:
                box.insert(1, np.empty(0, np.uint8))
            out = box
        else:
            out = [b[:n] for b, n in zip(bufs, counts)]
        return r, st, tot, out[0], out[1].tobytes(), out[2], out[3]

    def bgzf_tabix_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, conf, delim, flags, line_base, d_scratch, scratch_cap,
                       d_status, d_names, names_cap, d_blob, blob_cap, d_bins, bins_cap, d_wins, wins_cap):
        """zngamd_bgzf_tabix_dev on device pointers -> (code, totals); the tables stay on the device"""
        tot = BgzfTabixTotals()
        cf = TabixConf(*[int(x) for x in conf])
        r = self._chk(self.L.zngamd_bgzf_tabix_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, C.byref(cf), delim, flags,
                                                   line_base, _dv(d_scratch), scratch_cap, _dv(d_status), _dv(d_names), names_cap, _dv(d_blob), blob_cap,
                                                   _dv(d_bins), bins_cap, _dv(d_wins), wins_cap, C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_fetch(self, data, members, conf, delim, flags, names, regions, spans, caps=None):
        """zngamd_bgzf_fetch: names = the regions' names packed, regions = TABIX_REGION_DTYPE rows, spans = TABIX_SPAN_DTYPE rows ->
        (code, block statuses, span verdicts, rows per span, totals, rows (TABIX_ROW_DTYPE), packed lines).  caps None: rows and lines
        are allocated once the engine knows their sizes; (rows, bytes): buffers of those sizes, and code is BUF_ERROR when the result
        needs more"""
        ns = len(spans)
        win, st, keep = _window_in(data, members)
        regions = np.ascontiguousarray(regions, TABIX_REGION_DTYPE)
        spans = np.ascontiguousarray(spans, TABIX_SPAN_DTYPE)
        ss = np.zeros(max(1, ns), np.int32)
        sr = np.zeros(max(1, ns), np.uint32)
        tot = BgzfFetchTotals()
        cf = TabixConf(*[int(x) for x in conf])
        box = []

        def alloc(_user, nbytes):
            if not box:
                arr = np.empty(nbytes // TABIX_ROW_DTYPE.itemsize, TABIX_ROW_DTYPE)
                box.append(arr)
                return arr.ctypes.data
            obj, addr = _new_bytes(nbytes)
            box.append(obj)
            return addr.value

        if caps is None:
            rp, rcap, op, ocap, fn = None, 0, None, 0, ALLOC_FN(alloc)
        else:
            rows = np.zeros(max(1, caps[0]), TABIX_ROW_DTYPE)
            out, op = _new_bytes(caps[1])
            rp, rcap, ocap, fn = C.c_void_p(rows.ctypes.data), caps[0], caps[1], ALLOC_FN()
            if not ocap:
                op = None
            if not rcap:
                rp = None
        names = bytes(names)
        bp, bkeep = _addr(names) if names else (None, None)
        r = self._chk(self.L.zngamd_bgzf_fetch(self.h, *win,
                                               C.byref(cf), delim, flags, bp, len(names), C.c_void_p(regions.ctypes.data), len(regions),
                                               C.c_void_p(spans.ctypes.data) if ns else None, ns, C.c_void_p(st.ctypes.data),
                                               C.c_void_p(ss.ctypes.data), C.c_void_p(sr.ctypes.data), rp, rcap, op, ocap, fn, None,
                                               C.byref(tot)), (OK, BUF_ERROR))
        got = r == OK and tot.matched and not flags & BGZF_FETCH_COUNT_ONLY
        if caps is None:
            rows_out = box[0] if got else np.empty(0, TABIX_ROW_DTYPE)
            packed = box[1] if got else b""
        else:
            rows_out = rows[:tot.matched] if got else np.empty(0, TABIX_ROW_DTYPE)
            packed = _take(out, tot.bytes) if got else b""
        return r, st, ss[:ns], sr[:ns], tot, rows_out, packed

    def bgzf_fetch_dev(self, d_in, in_len, d_members, n_members, conf, delim, flags, names, regions, d_spans, n_spans, d_scratch, scratch_cap,
                       d_status, d_span_status, d_span_rows, d_rows, rows_cap, d_out, out_cap):
        """zngamd_bgzf_fetch_dev on device pointers (the regions: host memory) -> (code, totals)"""
        regions = np.ascontiguousarray(regions, TABIX_REGION_DTYPE)
        tot = BgzfFetchTotals()
        cf = TabixConf(*[int(x) for x in conf])
        names = bytes(names)
        bp, bkeep = _addr(names) if names else (None, None)
        r = self._chk(self.L.zngamd_bgzf_fetch_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, C.byref(cf), delim, flags, bp, len(names),
                                                   C.c_void_p(regions.ctypes.data), len(regions), _dv(d_spans), n_spans, _dv(d_scratch), scratch_cap,
                                                   _dv(d_status), _dv(d_span_status), _dv(d_span_rows), _dv(d_rows), rows_cap, _dv(d_out), out_cap,
                                                   C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_faidx(self, data, members, text_off, text_end, delim, flags, line_base=0, carry=None, caps=None):
        """zngamd_bgzf_faidx: carry = None (nothing is open) or a FaidxCarry -> (code, block statuses, totals (with the carry for the
        next call), rows (FAIDX_ROW_DTYPE), the names packed).  caps None: the tables are allocated once the engine knows their sizes;
        (rows, name bytes): buffers of those sizes, and code is BUF_ERROR (nothing written) when a table needs more"""
        win, st, keep = _window_in(data, members)
        tot = BgzfFaidxTotals()
        dts = (FAIDX_ROW_DTYPE, np.dtype("u1"))
        box = []

        def alloc(_user, nbytes):
            arr = np.empty(nbytes // dts[len(box)].itemsize, dts[len(box)])
            box.append(arr)
            return arr.ctypes.data

        if caps is None:
            ptrs, fn = [None, 0] * 2, ALLOC_FN(alloc)
        else:
            bufs = [np.zeros(max(1, n), dt) for n, dt in zip(caps, dts)]
            ptrs, fn = [], ALLOC_FN()
            for b, n in zip(bufs, caps):
                ptrs += [C.c_void_p(b.ctypes.data) if n else None, n]
        r = self._chk(self.L.zngamd_bgzf_faidx(self.h, *win, text_off,
                                               text_end, delim, flags, line_base, C.byref(carry) if carry is not None else None,
                                               C.c_void_p(st.ctypes.data), *ptrs, fn, None, C.byref(tot)), (OK, BUF_ERROR))
        if r != OK or not tot.covered or not tot.records:
            out = [np.empty(0, dt) for dt in dts]
        elif caps is None:
            out = box + [np.empty(0, np.uint8)] * (2 - len(box))
        else:
            out = [b[:n] for b, n in zip(bufs, (tot.records, tot.name_bytes))]
        return r, st, tot, out[0], out[1].tobytes()

    def bgzf_faidx_dev(self, d_in, in_len, d_members, n_members, text_off, text_end, delim, flags, line_base, carry, d_scratch, scratch_cap,
                       d_status, d_rows, rows_cap, d_blob, blob_cap):
        """zngamd_bgzf_faidx_dev on device pointers (the carry: host memory) -> (code, totals); rows and names stay on the device"""
        tot = BgzfFaidxTotals()
        r = self._chk(self.L.zngamd_bgzf_faidx_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, text_off, text_end, delim, flags, line_base,
                                                   C.byref(carry) if carry is not None else None, _dv(d_scratch), scratch_cap, _dv(d_status),
                                                   _dv(d_rows), rows_cap, _dv(d_blob), blob_cap, C.byref(tot)), (OK, BUF_ERROR))
        return r, tot

    def bgzf_faidx_fetch(self, data, members, spans, out_cap):
        """zngamd_bgzf_faidx_fetch: spans = FAIDX_SPAN_DTYPE rows -> (block statuses int32[n], span verdicts int32[n], packed bases)"""
        ns = len(spans)
        win, st, keep = _window_in(data, members)
        spans = np.ascontiguousarray(spans, FAIDX_SPAN_DTYPE)
        out, op = _new_bytes(out_cap)
        ss = np.zeros(max(1, ns), np.int32)
        self._chk(self.L.zngamd_bgzf_faidx_fetch(self.h, *win,
                                                 C.c_void_p(spans.ctypes.data) if ns else None, ns, op if out_cap else None, out_cap,
                                                 C.c_void_p(st.ctypes.data), C.c_void_p(ss.ctypes.data)))
        return st, ss[:ns], _take(out, out_cap)

    def bgzf_faidx_fetch_dev(self, d_in, in_len, d_members, n_members, d_spans, n_spans, d_scratch, scratch_cap, d_out, out_cap, d_status,
                             d_span_status):
        """zngamd_bgzf_faidx_fetch_dev on device pointers; statuses and bases stay on the device."""
        self._chk(self.L.zngamd_bgzf_faidx_fetch_dev(self.h, _dv(d_in), in_len, _dv(d_members), n_members, _dv(d_spans), n_spans, _dv(d_scratch),
                                                     scratch_cap, _dv(d_out), out_cap, _dv(d_status), _dv(d_span_status)))

    def bgzf_stats(self, reset=True):
        """(decode launches, blocks decoded, slices gathered) of the ranged reads since the last reset"""
        m = (C.c_uint64 * 3)()
        self._chk(self.L.zngamd_bgzf_stats(self.h, m, 1 if reset else 0))
        return int(m[0]), int(m[1]), int(m[2])

    def profiling(self, on):
        self._chk(self.L.zngamd_profiling(self.h, 1 if on else 0))

    def kernel_times(self, reset=True):
        # the library says how many it writes (a library older than the query -- a variant build of an earlier round under
        # ZNGAMD_LIB -- wrote as many as this table is long)
        nk = max(len(K_NAMES), int(self.L.zngamd_kernel_class_count())) if hasattr(self.L, "zngamd_kernel_class_count") else len(K_NAMES)
        ms = (C.c_double * nk)()
        ln = (C.c_uint64 * nk)()
        self._chk(self.L.zngamd_kernel_times(self.h, ms, ln, 1 if reset else 0))
        return {k: (ms[i], ln[i]) for i, k in enumerate(K_NAMES)}

    def decode_paths(self, reset=True):
        """Members gunzip() decoded per path since the last reset: indexed, bgzf, chunked, sequential."""
        m = (C.c_uint64 * 4)()
        self._chk(self.L.zngamd_decode_paths(self.h, m, 1 if reset else 0))
        return dict(zip(("indexed", "bgzf", "chunked", "sequential"), (int(x) for x in m)))


_default = None
_default_lock = threading.Lock()
_pool = {}


def writer_devices(limit=None):
    """Devices a block-parallel writer of THIS process spreads its batches over: ZNGAMD_DEVICES ("0,1,2,3"; a device may be
    named twice, which gives two contexts on it) or every visible GPU, cut to `limit` entries.  A process that was given
    one GPU by its launcher (LOCAL_RANK / ZNGAMD_DEVICE set) stays on it."""
    spec = os.environ.get("ZNGAMD_DEVICES")
    if spec:
        devs = [int(x) for x in spec.replace(";", ",").split(",") if x.strip() != ""]
    elif "ZNGAMD_DEVICE" in os.environ or "LOCAL_RANK" in os.environ:
        devs = [default_context().device]
    else:
        devs = list(range(max(1, load().zngamd_device_count())))
    if limit is not None:
        devs = devs[:max(1, limit)]
    return devs


def contexts(limit=None):
    """One context per entry of writer_devices(limit); entry 0 is the process-wide default context when it names its device.
    Contexts live as long as the process (their device workspaces are grow-only)."""
    out = []
    with _default_lock:
        pass
    seen = {}
    for d in writer_devices(limit):
        k = (d, seen.get(d, 0))
        seen[d] = seen.get(d, 0) + 1
        with _default_lock:
            c = _pool.get(k)
        if c is None:
            if k[1] == 0 and default_context().device == d:
                c = default_context()
            else:
                c = Context(device=d)
            with _default_lock:
                c = _pool.setdefault(k, c)
        out.append(c)
    return out


def deflate_blocks_multi(ctxs, buf, blocks, level, out_cap, into=None, table=None, index=None):
    """deflate_blocks(joined=True) over several contexts: the blocks are cut into contiguous ranges of about equal input,
    one per context; every range goes to its GPU as the slice of `buf` it needs (its blocks and the dictionary in front of
    its first block -- the previous range's input tail), the ranges run side by side (the engine calls release the GIL) and
    the results come back in block order.  This is the reference's worker fan-out (gzip_ng_threaded.py:233-246, :316-321)
    with contiguous ranges in place of round-robin, and its in-order drain (:382-398).
    -> (packed bytes, crcs, overflowed, lens) like Context.deflate_blocks(joined=True); `into` and `table` (block_table(blocks),
    made once by a caller whose batches repeat) serve the one-GPU case."""
    n = len(blocks)
    g = min(len(ctxs), n)
    # `index` (a list, or None): the batch's segment-index records are appended to it, in unit order (Context.deflate_index_records
    # of every range, taken right behind the range's engine call on its own context)
    def one():
        r = ctxs[0].deflate_blocks(buf, table if table is not None else blocks, level, out_cap, joined=True, into=into, index=index is not None)
        if index is not None and r[4] is not None:
            index.append(r[4])
        return r[:4]
    if g <= 1 or sys.is_finalizing():      # (no new threads while the interpreter shuts down)
        return one()
    total = sum(b[1] for b in blocks)
    if total < (8 << 20):
        return one()
    mv = memoryview(buf)
    if mv.format != "B" or mv.ndim != 1:
        mv = mv.cast("B")
    # contiguous ranges by cumulative input bytes
    cuts, acc, k = [0], 0, 1
    for i, b in enumerate(blocks):
        acc += b[1]
        if k < g and acc * g >= total * k and i + 1 < n:
            cuts.append(i + 1)
            k += 1
    cuts.append(n)
    parts = [None] * (len(cuts) - 1)
    recs = [None] * (len(cuts) - 1)
    errs = []

    def run(j):
        try:
            sub = blocks[cuts[j]:cuts[j + 1]]
            lo = min(o - d for o, _, d, _ in sub)
            hi = max(o + ln for o, ln, _, _ in sub)
            rel = [(o - lo, ln, d, f) for o, ln, d, f in sub]
            r = ctxs[j].deflate_blocks(mv[lo:hi], rel, level, out_cap, joined=True, index=index is not None)
            parts[j] = r[:4]
            if index is not None:
                recs[j] = r[4]
        except BaseException as exc:                      # raised in the caller's thread below
            errs.append(exc)
    ths = [threading.Thread(target=run, args=(j,), name=f"zng-amd-gpu{j}") for j in range(1, len(parts))]
    for t in ths:
        t.start()
    run(0)
    for t in ths:
        t.join()
    if errs:
        raise errs[0]
    if index is not None and all(r is not None for r in recs):
        index.extend(recs)
    packed = b"".join(p[0] for p in parts)
    crcs = [c for p in parts for c in p[1]]
    lens = [x for p in parts for x in p[3]]
    return packed, crcs, any(p[2] for p in parts), lens


def default_context():
    """Process-wide context on the GPU chosen by ZNGAMD_DEVICE / LOCAL_RANK (default 0)."""
    global _default
    with _default_lock:
        if _default is None:
            _default = Context()
        return _default

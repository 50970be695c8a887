// libzng_amd.so -- host side of the C ABI declared in include/zng_amd.h.  Product code.
// One translation unit: the kernel files are included so that no relocatable device code is needed.
//
// Nothing in this library computes a checksum, a match, a Huffman code or a decoded byte on the
// CPU: the host code cuts blocks into units, owns device workspaces and streams, launches the
// kernels and assembles container framing bytes (gzip / zlib headers and trailers).
#include "za_deflate.hip"
#include "za_inflate.hip"
#include "za_inflate_units.hip"
#include "za_inflate_spans.hip"
#include "za_bgzf.hip"
#include "za_grep.hip"
#include "za_grep_records.hip"
#include "za_classify.hip"
#include "za_partition.hip"
#include "za_trim.hip"
#include "za_qc.hip"
#include "za_dedup.hip"
#include "za_sort.hip"
#include "za_screen.hip"
#include "za_kcount.hip"
#include "za_overlap.hip"
#include "za_tabix.hip"
#include "za_faidx.hip"
#include "za_batch.hip"
#include "za_dict.hip"
#include "za_checksum.hip"
#include "../../include/zng_amd.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

static_assert(sizeof(zngamd_member) == sizeof(ZaMember), "member layout");
static_assert(sizeof(zngamd_span) == sizeof(ZaSpan) && ZNGAMD_SPAN_PAD == ZA_SPAN_PAD && ZNGAMD_SPAN_CRC == ZA_SPAN_CRC, "span layout");
static_assert(sizeof(zngamd_batch_item) == sizeof(ZaBatchItem) && sizeof(zngamd_batch_result) == sizeof(ZaBatchResult) &&
              ZNGAMD_BATCH_PAD == ZA_BATCH_PAD && ZNGAMD_BATCH_TABLE == ZA_BATCH_TABLE && ZNGAMD_BATCH_OUTFULL == ZA_BATCH_OUTFULL, "batch layout");
static_assert(ZNGAMD_ZDICT_MISMATCH == ZA_ZDICT_MISMATCH, "zdict status");
static_assert(sizeof(zngamd_bgzf_block) == sizeof(ZaBgzfBlock) && sizeof(zngamd_bgzf_slice) == sizeof(ZaBgzfSlice) && ZNGAMD_BGZF_MAX_INPUT == ZA_BGZF_MAX_IN &&
              ZNGAMD_BGZF_SLICE_BLOCK == ZA_SLICE_BLOCK && ZNGAMD_BGZF_SLICE_TABLE == ZA_SLICE_TABLE, "bgzf layout");
static_assert(sizeof(zngamd_bgzf_count_row) == sizeof(ZaBgzfCount) && sizeof(zngamd_bgzf_pos) == sizeof(ZaBgzfPos) && sizeof(zngamd_bgzf_line_range) == 2 * sizeof(ZaBgzfPos) &&
              ZNGAMD_BGZF_SLICE_RANK == ZA_SLICE_RANK && ZNGAMD_BGZF_RANK_END == ZA_RANK_END && ZNGAMD_BGZF_COUNT_LAST == ZA_COUNT_LAST, "bgzf line layout");
static_assert(sizeof(zngamd_bgzf_pattern) == sizeof(ZaGrepPat) && sizeof(zngamd_bgzf_grep_row) == sizeof(ZaGrepRow) && sizeof(ZaGrepRow) == sizeof(ZaBgzfSlice) &&
              sizeof(zngamd_bgzf_grep_totals) == 40 && offsetof(ZaGrepTotals, covered) == offsetof(zngamd_bgzf_grep_totals, covered) && sizeof(ZaGrepTotals) <= 64 &&
              ZNGAMD_BGZF_GREP_INVERT == ZA_GREP_INVERT && ZNGAMD_BGZF_GREP_LINE_START == ZA_GREP_LINE_START && ZNGAMD_BGZF_GREP_FINAL == ZA_GREP_FINAL &&
              ZNGAMD_BGZF_GREP_COUNT_ONLY == ZA_GREP_COUNT_ONLY && ZNGAMD_BGZF_GREP_MAX_PATTERNS == ZA_GREP_MAX_PAT && ZNGAMD_BGZF_GREP_MAX_PATTERN == ZA_GREP_MAX_LEN && ZNGAMD_BGZF_GREP_MAX_MISMATCH == ZA_GREP_MAX_MISMATCH,
              "bgzf grep layout");
static_assert(sizeof(zngamd_bgzf_grep_records_totals) == sizeof(ZaGrepRecTotals) && sizeof(ZaGrepRecTotals) == 64 &&
              offsetof(ZaGrepRecTotals, covered) == offsetof(zngamd_bgzf_grep_records_totals, covered) && sizeof(ZaGrepTotals) == 56 &&
              ZNGAMD_BGZF_GREP_MAX_RECORD_LINES == ZA_GREP_REC_MAX, "bgzf grep records layout");
static_assert(sizeof(zngamd_bgzf_classify_totals) == sizeof(ZaClsTotals) && offsetof(ZaClsTotals, class_bytes) == offsetof(zngamd_bgzf_classify_totals, class_bytes) &&
              sizeof(zngamd_bgzf_class_row) == 4 && ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES == ZA_CLS_MAX_CLASSES && ZNGAMD_BGZF_CLASSIFY_GROUP == ZA_CLS_GROUP &&
              ZNGAMD_BGZF_CLASS_ASSIGNED == ZA_CLS_ASSIGNED && ZNGAMD_BGZF_CLASS_AMBIGUOUS == ZA_CLS_AMBIGUOUS, "bgzf classify layout");
static_assert(sizeof(zngamd_bgzf_partition_totals) == sizeof(ZaPartTotals) && sizeof(ZaPartTotals) == 72 && offsetof(ZaPartTotals, covered) == offsetof(zngamd_bgzf_partition_totals, covered) &&
              offsetof(ZaPartTotals, labels_short) == offsetof(zngamd_bgzf_partition_totals, labels_short) && ZNGAMD_BGZF_PARTITION_MAX_CLASSES == ZA_PART_MAX_CLASSES &&
              ZNGAMD_BGZF_PARTITION_DROP == ZA_PART_DROP && ZA_PART_WG_RECORDS == ZA_CLS_WG_RECORDS, "bgzf partition layout");
static_assert(sizeof(zngamd_bgzf_trim_totals) == sizeof(ZaTrimTotals) && sizeof(ZaTrimTotals) == 632 && offsetof(ZaTrimTotals, covered) == offsetof(zngamd_bgzf_trim_totals, covered) &&
              offsetof(ZaTrimTotals, adapter_records) == offsetof(zngamd_bgzf_trim_totals, adapter_records) && sizeof(zngamd_bgzf_trim_row) == sizeof(ZaTrimRow) &&
              sizeof(ZaTrimRow) == 12 && sizeof(zngamd_bgzf_trim_conf) == 64 && ZNGAMD_BGZF_TRIM_KEPT == ZA_TRIM_KEPT && ZNGAMD_BGZF_TRIM_TOO_SHORT == ZA_TRIM_TOO_SHORT &&
              ZNGAMD_BGZF_TRIM_DROPPED == ZA_TRIM_DROPPED && ZNGAMD_BGZF_TRIM_KEEP_SHORT == ZA_TRIM_KEEP_SHORT && ZNGAMD_BGZF_TRIM_NO_ADAPTER == ZA_TRIM_NO_ADAPTER &&
              ZA_TRIM_STAGE_WORDS == 16u + (ZA_GREP_MAX_LEN + 3u) / 4u, "bgzf trim layout");
static_assert(sizeof(zngamd_bgzf_qc_totals) == sizeof(ZaQcTotals) && sizeof(ZaQcTotals) == 176 && offsetof(ZaQcTotals, covered) == offsetof(zngamd_bgzf_qc_totals, covered) &&
              offsetof(ZaQcTotals, tail_off) == offsetof(zngamd_bgzf_qc_totals, tail_off) && offsetof(ZaQcTotals, min_len) == offsetof(zngamd_bgzf_qc_totals, min_len) &&
              sizeof(zngamd_bgzf_qc_row) == sizeof(ZaQcRow) && sizeof(ZaQcRow) == 24 && sizeof(zngamd_bgzf_qc_conf) == 64 && ZNGAMD_BGZF_QC_MAX_CYCLES == ZA_QC_MAX_CYCLES &&
              ZNGAMD_BGZF_QC_BASES == ZA_QC_BASES && ZNGAMD_BGZF_QC_QUALITIES == ZA_QC_QUALS && ZNGAMD_BGZF_QC_GC_BINS == ZA_QC_GC_BINS && ZNGAMD_BGZF_QC_ROWS == ZA_QC_ROWS &&
              ZNGAMD_BGZF_QC_TABLE_WORDS(ZA_QC_MAX_CYCLES) == (uint64_t)(ZA_QC_MAX_CYCLES + 1u) * ZA_QC_COLS + ZA_QC_HIST_MAX, "bgzf qc layout");
static_assert(sizeof(zngamd_bgzf_key_totals) == sizeof(ZaKeyTotals) && sizeof(ZaKeyTotals) == 64 && offsetof(ZaKeyTotals, covered) == offsetof(zngamd_bgzf_key_totals, covered) &&
              offsetof(ZaKeyTotals, tail_off) == offsetof(zngamd_bgzf_key_totals, tail_off) && sizeof(zngamd_bgzf_key_row) == sizeof(ZaKeyRow) && sizeof(ZaKeyRow) == 16 &&
              sizeof(zngamd_bgzf_key_conf) == 64 && ZNGAMD_BGZF_KEY_IGNORE_CASE == ZA_KEY_IGNORE_CASE && ZNGAMD_BGZF_KEY_CANONICAL == ZA_KEY_CANONICAL &&
              ZNGAMD_BGZF_KEY_SEED0 == ZA_KEY_SEED0 && ZNGAMD_BGZF_KEY_SEED1 == ZA_KEY_SEED1 && sizeof(zngamd_dedup_totals) == sizeof(ZaDedupTotals) &&
              sizeof(ZaDedupTotals) == 48, "bgzf dedup layout");
static_assert(sizeof(zngamd_bgzf_screen_totals) == sizeof(ZaScreenTotals) && sizeof(ZaScreenTotals) == 88 && offsetof(ZaScreenTotals, covered) == offsetof(zngamd_bgzf_screen_totals, covered) &&
              offsetof(ZaScreenTotals, tail_off) == offsetof(zngamd_bgzf_key_totals, tail_off) && offsetof(ZaScreenTotals, kmers) == sizeof(zngamd_bgzf_key_totals) &&
              sizeof(zngamd_bgzf_screen_row) == sizeof(ZaScreenRow) && sizeof(ZaScreenRow) == 24 && sizeof(zngamd_bgzf_screen_conf) == 64 && sizeof(ZaKmerSlot) == 16 &&
              sizeof(zngamd_kmer_set_info) == 48 && ZNGAMD_KMER_CANONICAL == ZA_KMER_CANONICAL && ZNGAMD_KMER_NONE == ZA_KMER_NONE, "bgzf screen layout");
static_assert(sizeof(zngamd_bgzf_count_totals) == sizeof(ZaKcountTotals) && sizeof(ZaKcountTotals) == sizeof(ZaScreenTotals) && offsetof(ZaKcountTotals, covered) == offsetof(ZaScreenTotals, covered) &&
              offsetof(ZaKcountTotals, tail_off) == offsetof(zngamd_bgzf_key_totals, tail_off) && offsetof(ZaKcountTotals, kmers) == sizeof(zngamd_bgzf_key_totals) &&
              offsetof(zngamd_bgzf_count_totals, adds) == 80 && sizeof(zngamd_bgzf_count_conf) == 64 && sizeof(zngamd_kmer_counter_info) == 64 &&
              ZNGAMD_KMER_HIST_MAX_BINS == ZA_KCOUNT_MAX_BINS && ZNGAMD_KMER_HIST_MAX_BINS * 4u == 65536u, "bgzf count layout");
static_assert(sizeof(zngamd_bgzf_overlap_totals) == sizeof(ZaOvlTotals) && sizeof(ZaOvlTotals) == 160 && offsetof(ZaOvlTotals, covered) == offsetof(zngamd_bgzf_overlap_totals, covered) &&
              offsetof(ZaOvlTotals, mismatch_sum) == offsetof(zngamd_bgzf_overlap_totals, mismatch_sum) && offsetof(ZaOvlTotals, mismatch_sum) == (ZA_OVL_SUMS - 1u) * 8u &&
              sizeof(zngamd_bgzf_overlap_row) == sizeof(ZaOvlRow) && sizeof(ZaOvlRow) == 16 && sizeof(zngamd_bgzf_overlap_conf) == 64 &&
              ZNGAMD_BGZF_OVERLAP_NONE == ZA_OVL_NONE && ZNGAMD_BGZF_OVERLAP_FOUND == ZA_OVL_FOUND && ZNGAMD_BGZF_OVERLAP_MERGED == ZA_OVL_MERGED &&
              ZNGAMD_BGZF_OVERLAP_TOO_LONG == ZA_OVL_TOO_LONG && ZNGAMD_BGZF_OVERLAP_MERGE == ZA_OVL_MERGE && ZNGAMD_BGZF_OVERLAP_CORRECT == ZA_OVL_CORRECT &&
              ZNGAMD_BGZF_OVERLAP_CUT == ZA_OVL_CUT && ZNGAMD_BGZF_OVERLAP_KEEP_UNMERGED == ZA_OVL_KEEP_UNMERGED && ZNGAMD_BGZF_OVERLAP_MAX_READ == ZA_OVL_MAX_READ,
              "bgzf overlap layout");
static_assert(sizeof(zngamd_tabix_conf) == sizeof(ZaTbxConf) && sizeof(zngamd_tabix_name) == sizeof(ZaTbxName) && sizeof(zngamd_tabix_bin) == sizeof(ZaTbxBin) &&
              sizeof(zngamd_tabix_win) == sizeof(ZaTbxWin) && sizeof(zngamd_tabix_region) == sizeof(ZaTbxRegion) && sizeof(zngamd_tabix_span) == sizeof(ZaTbxSpan) &&
              sizeof(zngamd_tabix_row) == sizeof(ZaTbxRow) && sizeof(zngamd_bgzf_tabix_totals) == 104 && sizeof(ZaTbxState) <= 64 &&
              ZNGAMD_BGZF_TABIX_FINAL == ZA_TBX_FINAL && ZNGAMD_BGZF_FETCH_COUNT_ONLY == ZA_TBX_COUNT_ONLY && ZNGAMD_TABIX_MAX_POS == ZA_TBX_MAX_POS, "bgzf tabix layout");
static_assert(sizeof(zngamd_faidx_carry) == sizeof(ZaFaiCarry) && sizeof(ZaFaiCarry) == 32 && sizeof(zngamd_faidx_row) == sizeof(ZaFaiRow) && sizeof(ZaFaiRow) == 48 &&
              sizeof(zngamd_faidx_span) == sizeof(ZaFaiSpan) && sizeof(ZaFaiSpan) == 40 && sizeof(zngamd_bgzf_faidx_totals) == 104 && sizeof(ZaFaiState) == 88 &&
              ZNGAMD_BGZF_FAIDX_FINAL == ZA_FAI_FINAL && ZNGAMD_FAIDX_SPAN_RC == ZA_FAI_RC && ZNGAMD_FAIDX_MAX_SPAN == ZA_FAI_MAX_SPAN &&
              ZNGAMD_BGZF_SLICE_STALE == ZA_SLICE_STALE && ZNGAMD_FAIDX_OPEN == ZA_FAI_OPEN && ZNGAMD_FAIDX_GAP == ZA_FAI_GAP, "bgzf faidx layout");
static_assert(ZNGAMD_SLOT_STRIDE % 4 == 0 && ZNGAMD_SLOT_STRIDE >= ZA_MAX_UNIT + 32, "slot stride");
static_assert(ZNGAMD_UNIT_MAX == ZA_MAX_UNIT && ZNGAMD_SEG == ZA_SEG, "constants");

// the level table (the same numbers as the oracle's): chain steps over table A, nice, cap, table C, dynamic programme,
// too_far3, too_far4, shortest match (6 under Z_FILTERED, set per call), fixed-code costs (Z_FIXED, set per call).  Within 2 % of zlib 1.2.11 at the same level on held-out real files, at least zlib on the synthetic corpora.
#define ZA_CH_STREAMS_PER_CU (ZA_HASH_BITS >= 14 ? 2u : 3u)     // what the single-table chain kernel's LDS (table + 14 KiB) lets a CU hold (the two-table kernel: one workgroup, as the search)
#define ZA_WS_SHARE_DIV 4u          // ZA_WS_SHARE = 1 / 4: the most of the free device memory that the deflate workspace of a call without ZNGAMD_CHUNK_UNITS takes
static const ZaLevel ZA_LEVELS[10] = {
    {0, 0, ZA_WIN, 0, 0, 0, 0, 0, 3, 0},
    {1, 16, ZA_WIN, 16, 0, 0, 256, 4096, 3, 0}, {2, 16, ZA_WIN, 16, 0, 0, 256, 4096, 3, 0}, {3, 16, ZA_WIN, 16, 0, 0, 256, 4096, 3, 0},
    {2, 16, ZA_WIN, 16, 0, 1, 4096, 32768, 3, 0}, {2, 16, ZA_WIN, 16, 1, 1, 4096, 32768, 3, 0}, {3, 16, ZA_WIN, 16, 1, 1, 4096, 32768, 3, 0},
    {4, 32, ZA_WIN, 258, 1, 1, 4096, 32768, 3, 0}, {8, 64, ZA_WIN, 258, 1, 1, 4096, 32768, 3, 0}, {12, 128, ZA_WIN, 258, 1, 1, 4096, 32768, 3, 0}};

template <typename T> struct DevBuf {
    T *p = nullptr; size_t cap = 0;
    hipError_t ensure(size_t n)
    {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        // (small buffers grow with an eighth of slack so that a caller whose batches creep up does not reallocate every call; the
        // large per-chunk workspaces are sized exactly: an eighth of 48 GB is memory another context on the device may need)
        size_t want = n * sizeof(T) >= ((size_t)64 << 20) ? n + 64 : n + n / 8 + 64;
        hipError_t e = hipMalloc((void **)&p, want * sizeof(T));
        if (e != hipSuccess) { want = n; e = hipMalloc((void **)&p, want * sizeof(T)); }
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct EvPair { hipEvent_t a, b; int cls; };

// Message of the last failing call, kept per calling thread: a context is shared by many threads (readers, writers, the
// pump of the threaded reader), and the message is read after the call has left the context's mutex.
static thread_local std::string za_tl_err;
struct ZaErrSlot {
    ZaErrSlot &operator=(const char *m) { za_tl_err = m; return *this; }
    ZaErrSlot &operator=(const std::string &m) { za_tl_err = m; return *this; }
    const char *c_str() const { return za_tl_err.c_str(); }
};

struct zngamd_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    ZaErrSlot err;
    std::mutex mu;
    // constant tables
    uint32_t *d_crc_table = nullptr, *d_x8k = nullptr;
    uint32_t *d_crc_slice4 = nullptr;                                         // CRC slice-by-4 table of za_k_inflate_members
    // deflate workspaces (per chunk of units)
    // units per launch set (ZNGAMD_CHUNK_UNITS; 0 = not set: the whole call).  Workspace per unit (r06): link tables 3 x 320 KiB (two
    // below level 5), entries 512 KiB, about 5 KiB of small arrays -- 1.44 MiB; the token words (512 KiB) live IN the link tables'
    // memory, which nobody reads once the search is through (r05: 1.94 MiB with an eighth of slack on top).  Every launch set drains
    // the device once per kernel: a 4 GiB shard in two sets of 16 384 units (24 GB, the default of r06) took 2.1 % longer than in
    // one of 32 768 (47 GB; measured on the r06 kernels: deflate 64.5 -> 65.9 ms; 8 192: 68.4 ms).  So a call is ONE set unless
    // memory forbids: a set whose workspace would take more than ZA_WS_SHARE of the memory that is free (what these buffers hold
    // already counted as free), or that does not fit what is free at all, is halved until it does.
    uint32_t chunk_units = 0;
    DevBuf<uint16_t> links; DevBuf<uint32_t> best, tok, segtok, hist, codes; DevBuf<ZaPlan> plan;
    uint16_t *prev_p = nullptr, *linkb_p = nullptr, *linkc_p = nullptr; uint32_t *tok_p = nullptr;     // where the current chunk size puts the tables inside `links`, and the token words (inside `links` too unless zngamd_debug_keep asked for all stages to stay)
    bool debug_keep = false, last_kept = false; DevBuf<uint32_t> best_keep, dpcost;
    std::vector<uint32_t> last_ulen_host; bool last_ulen_on_host = false;      // ... and on the host, where the call fetched them with its results (the device copy lies in a staging buffer that an inflate call of another thread may give back)
    const uint32_t *last_unit_len = nullptr;     // the last deflate call's per-unit compressed sizes (device; the caller's array or a staging buffer of this context)     // zngamd_debug_keep: the search results as they were before the dynamic programme, its cost tables
    // per call
    DevBuf<ZaUnit> units; DevBuf<uint32_t> segbits, cidx, status, runs;
    uint32_t last_units = 0; bool last_single_chunk = false;
    std::vector<ZaUnit> last_hu;                 // the units of the last deflate call as the kernels saw them (zngamd_debug_fetch)
    std::vector<ZaUnit> plan_in; std::vector<uint32_t> plan_runs; uint32_t plan_ch = 0;     // the unit table the device holds was planned from this one: a caller that compresses batch after batch of the same shape pays for the planning once
    std::vector<zngamd_block> blocks_in; std::vector<ZaUnit> blocks_hu; uint64_t blocks_len = 0;
    uint32_t chain_slots = 512;                  // chain-kernel workgroups the device holds at once: CUs x ZA_CH_STREAMS_PER_CU (two with the 64 KiB table); ZNGAMD_CHAIN_SLOTS overrides
    uint32_t search_slots = 256;                 // search workgroups the device holds at once: one per CU (its LDS)
    uint32_t chain_run = 0;                      // ZNGAMD_CHAIN_RUN: fixed run length of the chain kernel (0 = sized to the device)
    // staging
    DevBuf<uint8_t> st_in, st_out, st_slots, st_aux, hdr; DevBuf<uint32_t> st_len, st_crc; DevBuf<uint64_t> st_off;
    DevBuf<uint64_t> ccand, csurv; DevBuf<ZaChunkRes> cres; DevBuf<ZaChunk> cchunks; DevBuf<uint16_t> out16, ccomp; DevBuf<uint8_t> winbuf;
    DevBuf<uint16_t> uarea; uint32_t uarea_marked = 0;     // symbol areas of the indexed unit decoder (32 768 marker symbols + 131 072 per unit) and how many of them have their markers
    DevBuf<ZaCkPart> ck; DevBuf<uint32_t> matchq; DevBuf<ZaCand> cands; DevBuf<ZaMember> members; DevBuf<int32_t> mstatus;
    void *d_small = nullptr;     // 256 B scratch for counters / results
    // profiling
    uint64_t paths[4] = {0, 0, 0, 0};            // members decoded per path, see zngamd_decode_paths
    uint64_t indexed_units = 0;                  // units decoded with a writer's index (zngamd_indexed_units)
    uint64_t span_stats[2] = {0, 0};             // spans and bytes of the span decoder (zngamd_span_stats)
    uint64_t chunk_stats[4] = {0, 0, 0, 0};      // sync hits, finder survivors, boundaries, chunks of inflate_chunked_once (zngamd_chunk_stats)
    DevBuf<uint8_t> sp_in, sp_win, sp_out; DevBuf<ZaSpan> sp_tab; DevBuf<int32_t> sp_status;      // staging of zngamd_inflate_spans
    DevBuf<uint8_t> bt_out, bt_out2, bt_def; DevBuf<ZaBatchItem> bt_items, bt_items2; DevBuf<ZaBatchResult> bt_res, bt_res2;    // the batch API (za_batch.hip)
    DevBuf<uint32_t> bt_first, bt_ulen, bt_ucrc; DevBuf<uint64_t> bt_uoff, bt_total;
    DevBuf<uint8_t> bt_dict, bt_prime;           // the batch API with a dictionary: its kept tail, the primed items ([tail][item] each)
    DevBuf<uint8_t> dt_data, dt_dict; DevBuf<uint32_t> dt_hash, dt_freq; DevBuf<uint16_t> dt_shadow;      // the dictionary trainer (za_dict.hip)
    DevBuf<ZaBatchItem> dt_items; DevBuf<ZaDictBest> dt_best; DevBuf<ZaDictState> dt_state;
    DevBuf<uint32_t> bg_len; DevBuf<ZaBgzfBlock> bg_table; DevBuf<ZaBgzfSlice> bg_slices; DevBuf<int32_t> bg_sstat; DevBuf<uint8_t> bg_out;      // BGZF (za_bgzf.hip): block sizes, block table, slices of a ranged read
    uint64_t bgzf_stats[3] = {0, 0, 0};          // ranged reads: decode launches, blocks decoded, slices gathered (zngamd_bgzf_stats)
    DevBuf<ZaBgzfCount> bg_rows; DevBuf<ZaBgzfPos> bg_q; DevBuf<uint64_t> bg_pos; DevBuf<int32_t> bg_pstat, bg_pre; DevBuf<uint32_t> bg_rlen;      // lines (section 5e): count rows, position queries, positions and their verdicts, range lengths
    DevBuf<uint8_t> gp_par; DevBuf<ulonglong2> gp_bits; DevBuf<ZaGrepTile> gp_tiles; DevBuf<ZaGrepCarry> gp_carry; DevBuf<ZaGrepRow> gp_rows; DevBuf<uint32_t> gp_lens;      // lines by content (za_grep.hip, section 5f): prefilter + pattern table + patterns, bits / summary / carry per tile, rows and their lengths
    // fields of a line (za_tabix.hip, section 5g): delimiter bits / number / delimiters in front per tile, the line records, the ordinals of
    // the data lines, the five scanned arrays and the scans' partial results, state and totals; the tables; the region filter's tables
    DevBuf<unsigned long long> tb_bits, tb_data, tb_name, tb_bin, tb_key, tb_raise, tb_blk, tb_tot; DevBuf<uint32_t> tb_tcnt, tb_di, tb_lens; DevBuf<uint64_t> tb_tbase;
    DevBuf<ZaTbxLine> tb_lines; DevBuf<ZaTbxName> tb_names; DevBuf<ZaTbxBin> tb_bins; DevBuf<ZaTbxWin> tb_wins;
    DevBuf<uint8_t> tb_par; DevBuf<ZaTbxSpan> tb_spans; DevBuf<ZaTbxRow> tb_rows; DevBuf<uint32_t> tb_srows; DevBuf<int32_t> tb_sstat; DevBuf<uint64_t> tb_sbase;
    std::vector<uint8_t> tb_host;
    // records of a FASTA (za_faidx.hip, section 5h; the bits, the tile counts, three scanned arrays and the totals are those of 5g): bad-byte
    // bits, line starts, bases | width per line, where header r stands, first / last non-empty line per record, rows, spans
    DevBuf<unsigned long long> fa_x, fa_bw; DevBuf<uint64_t> fa_start; DevBuf<uint32_t> fa_hline, fa_first, fa_last; DevBuf<ZaFaiRow> fa_rows; DevBuf<ZaFaiSpan> fa_spans;
    DevBuf<unsigned long long> gr_start, gr_sel, gr_len; DevBuf<uint8_t> gr_hit;      // records by content (za_grep_records.hip, section 5f.1): line starts; per record selected / bytes (scanned in place) and hit
    // records by their nearest pattern (za_classify.hip, section 5f.3): the two minima per record; per record class row, length and class;
    // the table of counts per (class, workgroup); the totals and the first bad record
    DevBuf<uint32_t> cl_min, cl_row, cl_len; DevBuf<uint8_t> cl_cls, cl_tot; DevBuf<unsigned long long> cl_tab;
    // records by the caller's labels (za_partition.hip, section 5f.4; lengths and table are cl_len and cl_tab): the host form's labels; the
    // totals, the two first faults, the scan's sum, records and bytes per class
    DevBuf<uint16_t> pt_lab; DevBuf<unsigned long long> pt_tot;
    // records trimmed (za_trim.hip, section 5f.5; line starts, lengths, table and labels are gr_start, cl_len, cl_tab and pt_lab): the trim
    // rows; the host form's drop mask; the totals, the two first faults, the scan's sum, the counts and what za_k_part_hist sums beside them
    DevBuf<ZaTrimRow> tr_row; DevBuf<uint8_t> tr_drop; DevBuf<unsigned long long> tr_tot;
    // records counted (za_qc.hip, section 5f.6; line starts are gr_start): the totals and the two first faults; the host form's tables and rows
    DevBuf<unsigned long long> qc_tot, qc_tab; DevBuf<ZaQcRow> qc_row;
    // records keyed and keys resolved (za_dedup.hip, section 5f.7; line starts are gr_start): the key pass's totals and first fault; the host
    // forms' rows, table, first[] and count[]
    DevBuf<unsigned long long> dd_tot, dd_first; DevBuf<ZaKeyRow> dd_row; DevBuf<uint8_t> dd_tab; DevBuf<uint32_t> dd_count;
    // records in another order (za_sort.hip, section 5f.9; line starts are gr_start): the totals and faults of the key and place passes; the
    // host forms' rows and lengths, keys, work area, order[] and rank[], dst[]
    DevBuf<unsigned long long> so_tot, so_key, so_tab, so_dst; DevBuf<uint8_t> so_row; DevBuf<uint32_t> so_len, so_ord, so_rank;
    // reads screened against reference k-mers (za_screen.hip, section 5f.10; line starts are gr_start): the totals and first fault of the
    // screen pass, or the two counts of a set being made, or the cursor of an export; the host form's rows; references, pairs and exports on
    // their way (a set's table is the set's own)
    DevBuf<unsigned long long> sc_tot; DevBuf<ZaScreenRow> sc_row; DevBuf<uint8_t> sc_tmp;
    // pairs laid over each other (za_overlap.hip, section 5f.8; line starts, lengths, table, labels and the totals' words are gr_start, cl_len,
    // cl_tab, pt_lab and tr_tot): the overlap rows
    DevBuf<ZaOvlRow> ov_row;
    std::vector<uint8_t> gp_host;                // the parameter block of the last grep call as it was uploaded
    uint8_t *h_stage = nullptr; size_t h_stage_cap = 0;      // pinned host staging for device-to-host results (grow-only)
    uint8_t *h_up = nullptr; size_t h_up_cap = 0;            // pinned host staging for small uploads (r06): the input of a small call, the unit / run tables
    uint8_t *h_tab = nullptr; size_t h_tab_cap = 0;
    hipEvent_t ev_up = nullptr, ev_tab = nullptr; bool up_busy = false, tab_busy = false;      // behind the last copy out of either: a buffer is written again only once that copy has run
    hipEvent_t ev_copy[2] = {nullptr, nullptr};              // ends of the staged device-to-host pieces
    bool prof = false; std::vector<EvPair> evs; std::vector<hipEvent_t> pool;
    double ms[ZNGAMD_K_COUNT] = {0}; uint64_t launches[ZNGAMD_K_COUNT] = {0};
};

#define HIPCHK(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return ZNGAMD_E_HIP; } } while (0)

static int fail(zngamd_ctx *c, int code, const char *msg) { c->err = msg; return code; }
// no C++ exception leaves the C ABI (host allocations of the batch paths can fail): reported as ZNGAMD_MEM_ERROR
#define ZA_ABI_GUARD catch (const std::bad_alloc &) { return ZNGAMD_MEM_ERROR; } catch (...) { return ZNGAMD_E_ARG; }


// ZNGAMD_TRACE=1: wall clock of the host phases of a call on stderr, the stream drained at the end of each so that a phase
// owns what it launched (diagnostics only: the drains cost time; profiles/time_threaded_rw.py and time_oneshot.py read it)
static bool trace_on() { static const bool on = getenv("ZNGAMD_TRACE") != nullptr; return on; }
struct PhaseClock {
    zngamd_ctx *c; const char *name; std::chrono::steady_clock::time_point t;
    PhaseClock(zngamd_ctx *c_, const char *n) : c(c_), name(n) { if (trace_on()) t = std::chrono::steady_clock::now(); }
    ~PhaseClock()
    {
        if (!trace_on()) return;
        if (c) (void)hipStreamSynchronize(c->stream);
        fprintf(stderr, "zng_amd trace: %-34s %9.3f ms\n", name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count());
    }
};

static hipEvent_t ev_get(zngamd_ctx *c)
{
    if (!c->pool.empty()) { hipEvent_t e = c->pool.back(); c->pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
struct ProfScope {
    zngamd_ctx *c; int cls; hipEvent_t a = nullptr;
    ProfScope(zngamd_ctx *c_, int cls_) : c(c_), cls(cls_) { if (c->prof) { a = ev_get(c); (void)hipEventRecord(a, c->stream); } }
    ~ProfScope() { if (c->prof) { hipEvent_t b = ev_get(c); (void)hipEventRecord(b, c->stream); c->evs.push_back({a, b, cls}); } }
};
static void prof_collect(zngamd_ctx *c)
{
    for (auto &e : c->evs) {
        float t = 0; (void)hipEventSynchronize(e.b);
        if (hipEventElapsedTime(&t, e.a, e.b) == hipSuccess) { c->ms[e.cls] += t; c->launches[e.cls]++; }
        c->pool.push_back(e.a); c->pool.push_back(e.b);
    }
    c->evs.clear();
}

extern "C" {

const char *zngamd_version(void) { return "zng_amd 0.6 (gfx950)"; }
int zngamd_abi(void) { return ZNGAMD_ABI; }
int zngamd_kernel_class_count(void) { return ZNGAMD_K_COUNT; }

int zngamd_device_count(void)
try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} ZA_ABI_GUARD

int zngamd_ctx_create(int device, zngamd_ctx **out)
try {
    if (!out) return ZNGAMD_E_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return ZNGAMD_E_HIP;
    if (hipSetDevice(device) != hipSuccess) return ZNGAMD_E_HIP;
    zngamd_ctx *c = new zngamd_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) { delete c; return ZNGAMD_E_HIP; }
    c->stream = c->own_stream;
    if (const char *e = getenv("ZNGAMD_CHUNK_UNITS")) { long v = atol(e); if (v >= 1 && v <= (1 << 20)) c->chunk_units = (uint32_t)v; }
    if (const char *e = getenv("ZNGAMD_CHAIN_RUN")) { long v = atol(e); if (v >= 1 && v <= (1 << 20)) c->chain_run = (uint32_t)v; }
    { int cus = 0; if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) { c->chain_slots = (uint32_t)cus * ZA_CH_STREAMS_PER_CU; c->search_slots = (uint32_t)cus; } }
    // (tests and sweeps: a device of v / ZA_CH_STREAMS_PER_CU CUs as far as the run plan is concerned -- all tiers within a few dozen units)
    if (const char *e = getenv("ZNGAMD_CHAIN_SLOTS")) { long v = atol(e); if (v >= 1 && v <= (1 << 20)) { c->chain_slots = (uint32_t)v; c->search_slots = std::max<uint32_t>(1u, (uint32_t)v / ZA_CH_STREAMS_PER_CU); } }
    // tables: CRC-32 byte table and x^(8*2048*k) mod P
    uint32_t tab[256], x8k[64];
    for (uint32_t i = 0; i < 256; i++) { uint32_t v = i; for (int k = 0; k < 8; k++) v = (v & 1) ? (0xEDB88320u ^ (v >> 1)) : (v >> 1); tab[i] = v; }
    {
        uint32_t xs = 0x80000000u, sq = 0x00800000u;      // x^(8*2048): square x^8 eleven times
        for (int i = 0; i < 11; i++) sq = za_multmodp(sq, sq);
        for (int k = 0; k < 64; k++) { x8k[k] = xs; xs = za_multmodp(xs, sq); }
    }
    if (hipMalloc((void **)&c->d_crc_table, sizeof tab) != hipSuccess || hipMalloc((void **)&c->d_x8k, sizeof x8k) != hipSuccess ||
        hipMalloc(&c->d_small, 256) != hipSuccess ||
        hipMemcpy(c->d_crc_table, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_x8k, x8k, sizeof x8k, hipMemcpyHostToDevice) != hipSuccess) {
        zngamd_ctx_destroy(c); return ZNGAMD_E_HIP;
    }
    {   // tables of the indexed-member decoder's CRC-32: [0, 1024) slice-by-4; [1024, 1152) the raw state advanced over 2 016 zero
        // bytes (what the other 63 lanes hold of a 2 KiB segment), one 16-entry table per nibble of the state; [1152, 1280)
        // x^(8 * 32 k) mod P for k < 128
        // [1280, 2304) and [2304, 2817): the checksum kernel's multipliers (za_checksum.hip)
        std::vector<uint32_t> s4(ZA_CK_TABS);
        for (int i = 0; i < 256; i++) s4[i] = tab[i];
        for (int t = 1; t < 4; t++) for (int i = 0; i < 256; i++) s4[256 * t + i] = (s4[256 * (t - 1) + i] >> 8) ^ tab[s4[256 * (t - 1) + i] & 0xFF];
        uint32_t x32 = 0x00800000u;                               // x^8 -> x^(8*32): squared five times
        for (int i = 0; i < 5; i++) x32 = za_multmodp(x32, x32);
        uint32_t xs = 0x80000000u;
        for (int k = 0; k < 128; k++) { s4[1152 + k] = xs; xs = za_multmodp(xs, x32); }
        const uint32_t x2016 = s4[1152 + 63];                     // x^(8 * 2016)
        for (int k = 0; k < 8; k++) for (uint32_t v = 0; v < 16; v++) s4[1024 + 16 * k + v] = za_multmodp(x2016, v << (4 * k));
        {
            uint32_t xt = 0x80000000u;                            // x^(8 t), t <= 512
            for (int t = 0; t <= 512; t++) { s4[ZA_CK_XT + t] = xt; xt = za_multmodp(xt, 0x00800000u); }
            for (int j = 0; j < 4; j++) {                         // x^(8 * (64 << j) * k), k < 256
                const uint32_t step = s4[ZA_CK_XT + (64 << j)];
                uint32_t xk = 0x80000000u;
                for (int k = 0; k < 256; k++) { s4[ZA_CK_XS + 256 * j + k] = xk; xk = za_multmodp(xk, step); }
            }
        }
        if (hipMalloc((void **)&c->d_crc_slice4, s4.size() * 4) != hipSuccess ||
            hipMemcpy(c->d_crc_slice4, s4.data(), s4.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
            zngamd_ctx_destroy(c); return ZNGAMD_E_HIP;
        }
    }
    *out = c;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

void zngamd_ctx_destroy(zngamd_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    for (auto e : c->pool) (void)hipEventDestroy(e);
    c->links.release(); c->best_keep.release(); c->dpcost.release(); c->hdr.release(); c->best.release(); c->tok.release(); c->segtok.release(); c->hist.release(); c->codes.release();
    c->plan.release(); c->units.release(); c->segbits.release(); c->cidx.release(); c->status.release();
    c->st_in.release(); c->st_out.release(); c->st_slots.release(); c->st_aux.release(); c->st_len.release(); c->st_crc.release();
    c->ccand.release(); c->csurv.release(); c->cres.release(); c->cchunks.release(); c->out16.release(); c->ccomp.release(); c->winbuf.release(); c->uarea.release();
    c->st_off.release(); c->runs.release(); c->ck.release(); c->matchq.release(); c->cands.release(); c->members.release(); c->mstatus.release();
    c->sp_in.release(); c->sp_win.release(); c->sp_out.release(); c->sp_tab.release(); c->sp_status.release();
    c->bt_out.release(); c->bt_out2.release(); c->bt_def.release(); c->bt_items.release(); c->bt_items2.release(); c->bt_res.release(); c->bt_res2.release();
    c->bt_first.release(); c->bt_ulen.release(); c->bt_ucrc.release(); c->bt_uoff.release(); c->bt_total.release();
    c->bt_dict.release(); c->bt_prime.release();
    c->dt_data.release(); c->dt_dict.release(); c->dt_hash.release(); c->dt_freq.release(); c->dt_shadow.release();
    c->dt_items.release(); c->dt_best.release(); c->dt_state.release();
    c->bg_len.release(); c->bg_table.release(); c->bg_slices.release(); c->bg_sstat.release(); c->bg_out.release();
    c->bg_rows.release(); c->bg_q.release(); c->bg_pos.release(); c->bg_pstat.release(); c->bg_pre.release(); c->bg_rlen.release();
    c->tb_bits.release(); c->tb_data.release(); c->tb_name.release(); c->tb_bin.release(); c->tb_key.release(); c->tb_raise.release(); c->tb_blk.release();
    c->tb_tot.release(); c->tb_tcnt.release(); c->tb_di.release(); c->tb_lens.release(); c->tb_tbase.release(); c->tb_lines.release(); c->tb_names.release();
    c->tb_bins.release(); c->tb_wins.release(); c->tb_par.release(); c->tb_spans.release(); c->tb_rows.release(); c->tb_srows.release(); c->tb_sstat.release(); c->tb_sbase.release();
    c->fa_x.release(); c->fa_bw.release(); c->fa_start.release(); c->fa_hline.release(); c->fa_first.release(); c->fa_last.release(); c->fa_rows.release(); c->fa_spans.release();
    c->gp_par.release(); c->gp_bits.release(); c->gp_tiles.release(); c->gp_carry.release(); c->gp_rows.release(); c->gp_lens.release();
    c->gr_start.release(); c->gr_sel.release(); c->gr_len.release(); c->gr_hit.release();
    c->cl_min.release(); c->cl_row.release(); c->cl_len.release(); c->cl_cls.release(); c->cl_tot.release(); c->cl_tab.release(); c->pt_lab.release(); c->pt_tot.release();
    c->tr_row.release(); c->tr_drop.release(); c->tr_tot.release(); c->ov_row.release();
    c->qc_tot.release(); c->qc_tab.release(); c->qc_row.release();
    c->dd_tot.release(); c->dd_first.release(); c->dd_row.release(); c->dd_tab.release(); c->dd_count.release();
    c->so_tot.release(); c->so_key.release(); c->so_tab.release(); c->so_dst.release(); c->so_row.release(); c->so_len.release(); c->so_ord.release(); c->so_rank.release();
    c->sc_tot.release(); c->sc_row.release(); c->sc_tmp.release();
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_up) (void)hipHostFree(c->h_up);
    if (c->h_tab) (void)hipHostFree(c->h_tab);
    if (c->ev_up) (void)hipEventDestroy(c->ev_up);
    if (c->ev_tab) (void)hipEventDestroy(c->ev_tab);
    for (auto &e : c->ev_copy) if (e) (void)hipEventDestroy(e);
    if (c->d_crc_table) (void)hipFree(c->d_crc_table);
    if (c->d_x8k) (void)hipFree(c->d_x8k);
    if (c->d_crc_slice4) (void)hipFree(c->d_crc_slice4);
    if (c->d_small) (void)hipFree(c->d_small);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char *zngamd_last_error(zngamd_ctx *c) { return c ? c->err.c_str() : "no context"; }

int zngamd_set_stream(zngamd_ctx *c, void *s)
try {
    if (!c) return ZNGAMD_E_ARG;
    (void)hipStreamSynchronize(c->stream);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_sync(zngamd_ctx *c)
try {
    if (!c) return ZNGAMD_E_ARG;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_dmalloc(zngamd_ctx *c, size_t bytes, void **dptr)
try {
    if (!c || !dptr) return ZNGAMD_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc(dptr, bytes ? bytes : 1));
    return ZNGAMD_OK;
} ZA_ABI_GUARD
int zngamd_dfree(zngamd_ctx *c, void *dptr) { if (!c) return ZNGAMD_E_ARG; HIPCHK(c, hipFree(dptr)); return ZNGAMD_OK; }
int zngamd_h2d(zngamd_ctx *c, void *dst, const void *src, size_t bytes)
try {
    if (!c) return ZNGAMD_E_ARG;
    if (bytes) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_d2h(zngamd_ctx *c, void *dst, const void *src, size_t bytes)
try {
    if (!c) return ZNGAMD_E_ARG;
    if (bytes) { HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// device-to-device copy and fill on the context's stream (ordered with the engine's kernels; no host synchronisation), and the
// device's free / total memory: what a harness needs to do without a tensor library
int zngamd_d2d(zngamd_ctx *c, void *dst, const void *src, size_t bytes)
try {
    if (!c) return ZNGAMD_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_dmemset(zngamd_ctx *c, void *dst, int value, size_t bytes)
try {
    if (!c) return ZNGAMD_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (bytes) HIPCHK(c, hipMemsetAsync(dst, value, bytes, c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_mem_info(zngamd_ctx *c, uint64_t *free_bytes, uint64_t *total_bytes)
try {
    if (!c || !free_bytes || !total_bytes) return ZNGAMD_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    size_t f = 0, t = 0;
    HIPCHK(c, hipMemGetInfo(&f, &t));
    *free_bytes = f; *total_bytes = t;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_decode_paths(zngamd_ctx *c, uint64_t *members, int reset)
try {
    if (!c || !members) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    for (int i = 0; i < ZNGAMD_PATH_COUNT; i++) { members[i] = c->paths[i]; if (reset) c->paths[i] = 0; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD
uint64_t zngamd_indexed_units(zngamd_ctx *c, int reset) { if (!c) return 0; std::lock_guard<std::mutex> g(c->mu); const uint64_t v = c->indexed_units; if (reset) c->indexed_units = 0; return v; }
int zngamd_profiling(zngamd_ctx *c, int on) { if (!c) return ZNGAMD_E_ARG; c->prof = on != 0; return ZNGAMD_OK; }
int zngamd_kernel_times(zngamd_ctx *c, double *ms, uint64_t *launches, int reset)
try {
    if (!c) return ZNGAMD_E_ARG;
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    for (int i = 0; i < ZNGAMD_K_COUNT; i++) { if (ms) ms[i] = c->ms[i]; if (launches) launches[i] = c->launches[i]; if (reset) { c->ms[i] = 0; c->launches[i] = 0; } }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---------------------------------------------------------------------------------------------
// checksums
// ---------------------------------------------------------------------------------------------
uint32_t zngamd_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2)
{
    uint32_t p = 0x80000000u, sq = 0x00800000u;
    while (len2) { if (len2 & 1) p = za_multmodp(sq, p); sq = za_multmodp(sq, sq); len2 >>= 1; }
    return za_multmodp(p, crc1) ^ crc2;
}

uint32_t zngamd_crc32_combine_many(uint32_t crc, const uint32_t *crcs, const uint64_t *lens, uint32_t n)
{
    if (!crcs || !lens) return crc;
    for (uint32_t i = 0; i < n; i++) crc = zngamd_crc32_combine(crc, crcs[i], lens[i]);
    return crc;
}

// run the checksum kernel over a device buffer and fold the per-span partials
// In two halves, so that a caller with kernels of its own to run can put them between the two and wait once: checksum_launch
// enqueues the kernel and the copy of its partial results, checksum_fold (behind a synchronisation of the stream) folds them.
static int checksum_launch(zngamd_ctx *c, const uint8_t *d, uint64_t n, bool want_crc, bool want_adler, std::vector<ZaCkPart> &parts)
{
    parts.clear();
    if (n == 0) return ZNGAMD_OK;
    const uint64_t nspan = (n + ZA_MAX_UNIT - 1) / ZA_MAX_UNIT;
    if (nspan > 0x7FFFFFFFull) return fail(c, ZNGAMD_E_ARG, "buffer too large");
    HIPCHK(c, c->ck.ensure(nspan));
    {
        ProfScope ps(c, ZNGAMD_K_OTHER);
        hipLaunchKernelGGL(za_k_checksum, dim3((uint32_t)nspan), dim3(256), 0, c->stream, d, n, c->d_crc_slice4, c->ck.p, want_crc ? 1 : 0, want_adler ? 1 : 0);
    }
    HIPCHK(c, hipGetLastError());
    parts.resize(nspan);
    HIPCHK(c, hipMemcpyAsync(parts.data(), c->ck.p, nspan * sizeof(ZaCkPart), hipMemcpyDeviceToHost, c->stream));
    return ZNGAMD_OK;
}

static void checksum_fold(const std::vector<ZaCkPart> &parts, uint32_t *crc_io, uint32_t *adler_io)
{
    const uint64_t nspan = parts.size();
    if (crc_io) {
        // all spans but the last are ZA_MAX_UNIT long: one multiplier, x^(8 * ZA_MAX_UNIT) mod P, serves them (2 048 spans of a
        // 256 MiB result cost 0.6 ms when each call worked its multiplier out again)
        uint32_t crc = *crc_io;
        uint32_t xp = 0x80000000u, sq = 0x00800000u;                          // x^0, x^8
        for (uint64_t k = ZA_MAX_UNIT; k; k >>= 1) { if (k & 1) xp = za_multmodp(sq, xp); sq = za_multmodp(sq, sq); }
        for (uint64_t i = 0; i < nspan; i++) {
            if (parts[i].len == ZA_MAX_UNIT) crc = za_multmodp(xp, crc) ^ parts[i].crc;
            else crc = zngamd_crc32_combine(crc, parts[i].crc, parts[i].len);
        }
        *crc_io = crc;
    }
    if (adler_io) {
        uint64_t A = *adler_io & 0xFFFF, B = (*adler_io >> 16) & 0xFFFF;
        for (uint64_t i = 0; i < nspan; i++) {
            B = (B + (uint64_t)(parts[i].len % 65521u) * A + parts[i].b) % 65521u;
            A = (A + parts[i].a) % 65521u;
        }
        *adler_io = (uint32_t)((B << 16) | A);
    }
}

static int checksum_dev(zngamd_ctx *c, const uint8_t *d, uint64_t n, uint32_t *crc_io, uint32_t *adler_io)
{
    if (n == 0) return ZNGAMD_OK;
    PhaseClock pc(c, "checksum of a device buffer");
    std::vector<ZaCkPart> parts;
    const int r = checksum_launch(c, d, n, crc_io != nullptr, adler_io != nullptr, parts);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    checksum_fold(parts, crc_io, adler_io);
    return ZNGAMD_OK;
}

// a grow-only pinned buffer (uploads from pinned memory are queued and return; from pageable memory the call stages them itself
// and waits -- 15 to 30 us per copy of a small call)
static int pinned_ensure(zngamd_ctx *c, uint8_t **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return ZNGAMD_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr; *cap = 0;
    const size_t want = bytes + bytes / 4 + 4096;
    HIPCHK(c, hipHostMalloc((void **)p, want, hipHostMallocDefault));
    *cap = want;
    return ZNGAMD_OK;
}

#define ZNGAMD_SMALL_UP (1u << 20)       // inputs up to this size travel through the pinned upload buffer (one queued copy, the 64 zero bytes behind the input included)
static int stage_in(zngamd_ctx *c, const uint8_t *in, uint64_t n, uint64_t pad_front = 0)
{
    PhaseClock pc(c, "stage_in (host -> device)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->st_in.ensure(pad_front + n + 64));
    if (n <= ZNGAMD_SMALL_UP) {
        // (nearly every call ends behind a synchronisation of the stream, but one that failed half way may have left its copy queued)
        if (!c->ev_up) HIPCHK(c, hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
        if (c->up_busy) { HIPCHK(c, hipEventSynchronize(c->ev_up)); c->up_busy = false; }
        const int r = pinned_ensure(c, &c->h_up, &c->h_up_cap, n + 64);
        if (r) return r;
        if (n) memcpy(c->h_up, in, n);
        memset(c->h_up + n, 0, 64);
        HIPCHK(c, hipMemcpyAsync(c->st_in.p + pad_front, c->h_up, n + 64, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_up, c->stream));
        c->up_busy = true;
        return ZNGAMD_OK;
    }
    if (n) HIPCHK(c, hipMemcpyAsync(c->st_in.p + pad_front, in, n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->st_in.p + pad_front + n, 0, 64, c->stream));
    return ZNGAMD_OK;
}

int zngamd_crc32_dev(zngamd_ctx *c, uint32_t crc, const void *dbuf, size_t len, uint32_t *out)
try {
    if (!c || !out) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t v = crc;
    int r = checksum_dev(c, (const uint8_t *)dbuf, len, &v, nullptr);
    *out = v;
    return r;
} ZA_ABI_GUARD

int zngamd_crc32(zngamd_ctx *c, uint32_t crc, const uint8_t *buf, size_t len, uint32_t *out)
try {
    if (!c || !out || (!buf && len)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    int r = stage_in(c, buf, len);
    if (r) return r;
    uint32_t v = crc;
    r = checksum_dev(c, c->st_in.p, len, &v, nullptr);
    *out = v;
    return r;
} ZA_ABI_GUARD

int zngamd_adler32(zngamd_ctx *c, uint32_t adler, const uint8_t *buf, size_t len, uint32_t *out)
try {
    if (!c || !out || (!buf && len)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    int r = stage_in(c, buf, len);
    if (r) return r;
    // the seed halves are reduced even when there is no data (zlib semantics the reference inherits)
    uint32_t v = ((((adler >> 16) & 0xFFFFu) % 65521u) << 16) | ((adler & 0xFFFFu) % 65521u);
    r = checksum_dev(c, c->st_in.p, len, nullptr, &v);
    *out = v;
    return r;
} ZA_ABI_GUARD

// ---------------------------------------------------------------------------------------------
// deflate
// ---------------------------------------------------------------------------------------------
int zngamd_level_ok(int level) { return level >= -1 && level <= 9; }

// the strategy of a call: ZNGAMD_FLAG_STRATEGY of its first block, like the window (0 = the default; 5..7 are refused)
static int strategy_of(const zngamd_block *blocks, uint32_t n_blocks) { return n_blocks ? ZNGAMD_STRATEGY_OF(blocks[0].flags) : ZNGAMD_STRATEGY_DEFAULT; }

static uint32_t unit_size_of(const zngamd_block &b) { return (b.flags & ZNGAMD_FLAG_UNITS16K) ? ZA_SMALL_UNIT : (uint32_t)ZA_MAX_UNIT; }
static uint32_t units_of(const zngamd_block &b) { const uint64_t U = unit_size_of(b); return b.len == 0 ? 1u : (uint32_t)(((uint64_t)b.len + U - 1) / U); }

// The most bytes a unit of in_len bytes takes in a packed stream under the call's strategy (every host bound is a
// sum of these).  A unit is never larger than its stored form: its bytes + 5 per stored chunk of 65 535 (three in a full unit) +
// an empty stored block behind it -- but for Z_FIXED, which takes a fixed block wherever a dynamic one would have won, also where
// stored beats fixed: at most 9 bits a byte (a literal is 8 or 9 bits, and a match of l bytes at most 7 + 5 + 13 extra bits for
// l = 3, 4, at most 8 + 5 + 5 + 13 for longer ones: never more than 9 l), so ceil((3 + 9 n + 7 + 3) / 8) + 4 bytes.
static uint64_t unit_bound(uint32_t in_len, int strategy)
{
    return (uint64_t)in_len + (strategy == ZNGAMD_STRATEGY_FIXED ? in_len / 8u : 0u) + 32u;
}

uint32_t zngamd_count_units(const zngamd_block *blocks, uint32_t n_blocks)
{
    uint64_t t = 0;
    for (uint32_t i = 0; i < n_blocks; i++) t += units_of(blocks[i]);
    return t > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)t;
}

static int build_units(zngamd_ctx *c, const zngamd_block *blocks, uint32_t n_blocks, uint64_t in_len, std::vector<ZaUnit> &hu)
{
    hu.clear();
    for (uint32_t b = 0; b < n_blocks; b++) {
        const zngamd_block &B = blocks[b];
        if (B.dict_len > ZA_WIN || B.dict_len > B.off || B.off + B.len > in_len) return fail(c, ZNGAMD_E_ARG, "block outside the input buffer");
        const uint32_t nu = units_of(B);
        const uint64_t U = unit_size_of(B);
        for (uint32_t k = 0; k < nu; k++) {
            ZaUnit u;
            const uint64_t rel = (uint64_t)k * U;
            u.in_off = B.off + rel;
            u.in_len = (uint32_t)std::min<uint64_t>(U, B.len - rel);
            u.dict_len = (uint32_t)std::min<uint64_t>(ZA_WIN, (uint64_t)B.dict_len + rel);
            u.flags = (B.flags & (ZNGAMD_FLAG_FLATHDR | ZNGAMD_FLAG_SEG2K)) | ((k == nu - 1) ? (B.flags & ZNGAMD_FLAG_FINAL) : 0u);
            u.flags |= (uint32_t)za_seg_shift_for(u.in_len, u.flags) << 8;       // the unit's segment size (za_common.h: small units take small segments)
            u.block = b;
            // the unit's whole 32 KiB dictionary is the tail of the unit in front of it: the chain tables may be carried over
            if (!hu.empty()) {
                const ZaUnit &pv = hu.back();
                if (u.dict_len == ZA_WIN && pv.in_len >= ZA_WIN && (pv.in_len & 3u) == 0u && pv.in_off + pv.in_len == u.in_off) u.flags |= ZA_FLAG_CARRY;   // (a multiple of 4: the search stages its byte ring in aligned dwords)
            }
            hu.push_back(u);
        }
    }
    return ZNGAMD_OK;
}

// launch the five deflate kernels over all units (in chunks that bound the workspace)
// `packed` set: no slots -- the plan kernel sizes every unit exactly, a prefix sum places it, the packer writes it there
struct PackedDst { uint8_t *d_dst = nullptr; uint64_t cap = 0; uint64_t *d_unit_off = nullptr;
                   uint64_t *d_total = nullptr; uint32_t *d_status = nullptr; };      // (optional) where the stream's size and the units' pack status go: a caller that fetches all results with one copy
static int deflate_units_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const std::vector<ZaUnit> &hu, int level,
                             uint8_t *d_slots, uint32_t *d_unit_len, uint32_t *d_unit_crc, int max_dist = ZA_WIN,
                             const PackedDst *packed = nullptr, int strategy = ZNGAMD_STRATEGY_DEFAULT)
{
    if (level == -1) level = 6;
    if (level < 0 || level > 9) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (strategy < ZNGAMD_STRATEGY_DEFAULT || strategy > ZNGAMD_STRATEGY_FIXED) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression strategy");
    // Z_HUFFMAN_ONLY / Z_RLE (level >= 1): no link tables, no search -- k_parse_rle reads the input itself
    const bool runs_only = level > 0 && (strategy == ZNGAMD_STRATEGY_HUFFMAN_ONLY || strategy == ZNGAMD_STRATEGY_RLE);
    const bool search = level > 0 && !runs_only;
    const uint32_t n = (uint32_t)hu.size();
    if (n == 0) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    uint32_t ch = c->chunk_units ? std::min(n, c->chunk_units) : n;
    const size_t ntab = ZA_LEVELS[level].use_c ? 3 : 2;
    // a set's workspaces (`per_unit` bytes a unit) must fit what the device has free (plus `held`, what these buffers hold already):
    // halve it until they do (a hipMalloc failure further down is still a hard error, but no longer the first thing a smaller
    // device or a second context on this one meets).  A set that nobody sized (no ZNGAMD_CHUNK_UNITS) also stays within
    // ZA_WS_SHARE of that memory: the caller's own buffers and a second context want room too.  `held` counts as free on both
    // sides, so a call of the same shape gets the same set size every time and the kept plan stays valid.
    auto fit_set = [&](size_t per_unit, size_t held) {
        size_t free_b = 0, total_b = 0;
        if (ch <= 64 || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;       // (a driver call: tens of microseconds, and a small call has nothing to halve)
        auto need = [&](uint32_t k) { return (size_t)k * per_unit; };
        while (ch > 64 && need(ch) > held && need(ch) - held > free_b - free_b / 16) ch = (ch + 1) / 2;
        if (!c->chunk_units) while (ch > 64 && need(ch) > (free_b + held) / ZA_WS_SHARE_DIV) ch = (ch + 1) / 2;
    };
    if (search)
        fit_set(ntab * ZA_PREV_STRIDE * 2 + ZA_BEST_STRIDE * 4 + (c->debug_keep ? (ZA_BEST_STRIDE + ZA_TOK_STRIDE) * 4 : 0) + 8192,
                c->links.cap * 2 + c->best.cap * 4 + c->tok.cap * 4 + c->best_keep.cap * 4);
    HIPCHK(c, c->units.ensure(n)); HIPCHK(c, c->segbits.ensure((size_t)n * ZA_SEGB_STRIDE)); HIPCHK(c, c->cidx.ensure((size_t)n * ZA_CIDX_STRIDE)); HIPCHK(c, c->status.ensure(n));
    if (runs_only) {
        // only the token words: in the link tables' buffer (grown to 512 KiB a unit if a search never made it larger), or, when the
        // debug copies are kept, in their own
        fit_set(ZA_TOK_STRIDE * 4 + 8192, c->links.cap * 2 + (c->debug_keep ? c->tok.cap * 4 : 0));
        if (c->debug_keep) { HIPCHK(c, c->tok.ensure((size_t)ch * ZA_TOK_STRIDE)); c->tok_p = c->tok.p; }
        else { HIPCHK(c, c->links.ensure((size_t)ch * ZA_TOK_STRIDE * 2)); c->tok_p = (uint32_t *)c->links.p; }
    }
    if (search) {
        const size_t tab = (size_t)ch * ZA_PREV_STRIDE + 8;              // entries of one link table (+ slack for the search's four-link loads)
        HIPCHK(c, c->links.ensure(ntab * tab)); HIPCHK(c, c->best.ensure((size_t)ch * ZA_BEST_STRIDE));
        c->prev_p = c->links.p; c->linkb_p = c->links.p + tab; c->linkc_p = ntab > 2 ? c->links.p + 2 * tab : nullptr;
        if (ZA_LEVELS[level].dp) HIPCHK(c, c->dpcost.ensure((size_t)ch * ZA_DP_COSTS));
        if (c->debug_keep) {
            HIPCHK(c, c->best_keep.ensure((size_t)ch * ZA_BEST_STRIDE));
            HIPCHK(c, c->tok.ensure((size_t)ch * ZA_TOK_STRIDE));
            c->tok_p = c->tok.p;
        } else {
            // the token words (and the dynamic programme's acc[] scratch inside them) take the place of the link tables: written by
            // kernels that run after the search of the same chunk on the same stream, 512 KiB a unit inside >= 640 KiB a unit
            static_assert(2 * ZA_PREV_STRIDE * 2 >= ZA_TOK_STRIDE * 4, "token words fit two link tables");
            c->tok_p = (uint32_t *)c->links.p;
        }
    }
    HIPCHK(c, c->segtok.ensure((size_t)ch * ZA_MAX_SEGS)); HIPCHK(c, c->hist.ensure((size_t)ch * ZA_HIST_STRIDE));
    HIPCHK(c, c->codes.ensure((size_t)ch * ZA_CODE_STRIDE)); HIPCHK(c, c->plan.ensure(ch));
    uint64_t *d_run_total = (uint64_t *)((uint8_t *)c->d_small + 224);      // (packed) bytes of the launches so far
    uint64_t *d_offs = nullptr;
    if (packed) {
        HIPCHK(c, c->hdr.ensure((size_t)ch * ZA_HDR_STRIDE));
        d_offs = packed->d_unit_off;
        if (!d_offs) { HIPCHK(c, c->st_off.ensure(n)); d_offs = c->st_off.p; }
        if (packed->d_total) d_run_total = packed->d_total;
        // (no memset of the running total: the first launch's prefix sum starts from nothing and writes it)
    }
    uint32_t *d_status = (packed && packed->d_status) ? packed->d_status : c->status.p;
    // Runs of the chain kernel: one workgroup walks a run of consecutive units and carries its tables from unit to unit where
    // the next unit's dictionary is the tail of the one before (ZA_FLAG_CARRY); a run costs its first unit's dictionary
    // again, so longer runs save more (a quarter of the positions at most) -- but workgroups are handed out in order, and a
    // launch ends with its last workgroup -- of the chain kernel, and of the search, which walks the same runs with half as
    // many workgroups at once and spends three times as long on a unit.  Hence three tiers: runs of L units (L bounded by what
    // keeps every slot of the device busy at least twice), runs of L / 4 behind them, single units at the end.  When the last
    // run of a tier is handed out, every slot holds a run of that tier with anything between nothing and all of it left: the
    // tiers behind it hold `slots` x the tier's run length in units to even the slots out -- all that the search's slots can
    // have left, and what the chain kernel's twice as many slots have left on average.  (Measured at 32 768 units against a
    // whole run length for every slot of the chain kernel: chains 13.81 / 13.92 ms, search 29.05 / 29.04; until the search was
    // looked at, short runs simply took the last fifth: 14.07 and 29.45.)  Runs never cross a launch set.
    const bool same_plan = c->plan_ch == ch && c->plan_in.size() == hu.size() && c->last_hu.size() == hu.size() &&
                           memcmp(c->plan_in.data(), hu.data(), hu.size() * sizeof(ZaUnit)) == 0;
    if (!same_plan) {
        // (the kept plan describes device tables that are about to be overwritten: should an upload fail half way, a later call
        // with the old shape must not find it valid)
        c->plan_in.clear(); c->plan_ch = 0; c->last_hu.clear();
        std::vector<ZaUnit> hv(hu);
        std::vector<uint32_t> run_start;
        for (uint32_t c0 = 0; c0 < n; c0 += ch) {
            const uint32_t m = std::min(ch, n - c0);
            const uint32_t L = c->chain_run ? c->chain_run : std::min<uint32_t>(8u, std::max<uint32_t>(1u, m / (2u * c->chain_slots)));
            const uint32_t Ls = c->chain_run ? c->chain_run : std::max<uint32_t>(1u, L / 4u);
            const uint64_t slots = std::max<uint32_t>(c->search_slots, (c->chain_slots + 1u) / 2u);
            const uint32_t n_single = (c->chain_run || Ls == 1u) ? 0u : (uint32_t)std::min<uint64_t>(m, slots * Ls);       // (Ls = 1: the middle tier IS single units)
            const uint32_t n_mid = c->chain_run ? 0u : (uint32_t)std::min<uint64_t>(m - n_single, slots * L);
            const uint32_t big_end = (m - n_single - n_mid) / L * L, mid_end = m - n_single;
            uint32_t next_cut = 0;
            for (uint32_t i = 0; i < m; i++) {
                ZaUnit &u = hv[c0 + i];
                const bool cut = i == next_cut || !(u.flags & ZA_FLAG_CARRY);
                if (cut) { u.flags |= ZA_FLAG_RUNHEAD; run_start.push_back(i); next_cut = i + (i < big_end ? L : i < mid_end ? Ls : 1u); }
            }
            run_start.push_back(m);                                  // (the runs of one launch: starts relative to the launch, then its end)
        }
        HIPCHK(c, c->runs.ensure(run_start.size()));
        if (n <= 4096) {
            // a small table travels from pinned memory: two queued copies and no wait (r06: a call whose shape differs from the
            // last one's paid 40 us for the two staged copies and the synchronisation)
            const size_t rb = run_start.size() * 4, ub = (size_t)n * sizeof(ZaUnit);
            if (!c->ev_tab) HIPCHK(c, hipEventCreateWithFlags(&c->ev_tab, hipEventDisableTiming));
            if (c->tab_busy) { HIPCHK(c, hipEventSynchronize(c->ev_tab)); c->tab_busy = false; }
            const int rp = pinned_ensure(c, &c->h_tab, &c->h_tab_cap, rb + ub);
            if (rp) return rp;
            memcpy(c->h_tab, hv.data(), ub);
            memcpy(c->h_tab + ub, run_start.data(), rb);
            HIPCHK(c, hipMemcpyAsync(c->units.p, c->h_tab, ub, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->runs.p, c->h_tab + ub, rb, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipEventRecord(c->ev_tab, c->stream));
            c->tab_busy = true;
        } else {
        HIPCHK(c, hipMemcpyAsync(c->runs.p, run_start.data(), run_start.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->units.p, hv.data(), (size_t)n * sizeof(ZaUnit), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));                  // (hv and run_start are locals)
        }
        c->last_hu.swap(hv);
        c->plan_runs.swap(run_start);
        c->plan_in = hu; c->plan_ch = ch;
    }
    const std::vector<uint32_t> &run_start = c->plan_runs;
    // (no memset of the slots: the pack kernel zeroes the few words it merges with atomic OR and writes the rest whole)
    ZaLevel L = ZA_LEVELS[level];
    L.max_dist = (max_dist < 1 || max_dist > ZA_WIN) ? ZA_WIN : max_dist;
    if (strategy == ZNGAMD_STRATEGY_FILTERED) L.min_len = 6;             // zlib's deflate_slow under Z_FILTERED: match_length <= 5 is dropped
    const int fixed_only = strategy == ZNGAMD_STRATEGY_FIXED ? 1 : 0;
    L.fixed_cost = fixed_only;
    size_t run_pos = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += ch) {
        const uint32_t m = std::min(ch, n - c0);
        const ZaUnit *du = c->units.p + c0;
        uint32_t nruns = 0;
        while (run_start[run_pos + nruns] != m) nruns++;
        const uint32_t *d_runs = c->runs.p + run_pos;
        run_pos += nruns + 1;
        if (runs_only) {
            ProfScope ps(c, ZNGAMD_K_PARSE);
            if (strategy == ZNGAMD_STRATEGY_RLE)
                hipLaunchKernelGGL(za_k_parse_rle<true>, dim3(m), dim3(64), 0, c->stream, d_in, du, c->tok_p, c->segtok.p, c->hist.p,
                                   d_unit_crc + c0, c->d_crc_table, c->d_x8k);
            else
                hipLaunchKernelGGL(za_k_parse_rle<false>, dim3(m), dim3(64), 0, c->stream, d_in, du, c->tok_p, c->segtok.p, c->hist.p,
                                   d_unit_crc + c0, c->d_crc_table, c->d_x8k);
        } else if (search) {
            { ProfScope ps(c, ZNGAMD_K_CHAINS);
              uint32_t *const d_clear = L.dp ? c->dpcost.p : (uint32_t *)nullptr;       // (with table A) the units' long-match words
              // Two of the tables come from one launch (za_k_chains2; ZA_CH_PAIR, za_deflate.hip): with table C (levels 5-9) A on its
              // own, then B and C together -- measured, that pairing is the faster one --, without it A and B together.
#define ZA_LAUNCH_CH1(T, dst, clr) hipLaunchKernelGGL(za_k_chains<T>, dim3(nruns), dim3(256), 0, c->stream, d_in, du, d_runs, dst, clr)
#define ZA_LAUNCH_CH2(T1, T2, dst1, dst2, clr) hipLaunchKernelGGL((za_k_chains2<T1, T2>), dim3(nruns), dim3(512), 0, c->stream, d_in, du, d_runs, dst1, dst2, clr)
              uint32_t *const no_clear = nullptr;
#if ZA_CH_PAIR == 0
              ZA_LAUNCH_CH1(ZA_TABLE_A, c->prev_p, d_clear);
              ZA_LAUNCH_CH1(ZA_TABLE_B, c->linkb_p, no_clear);
              if (L.use_c) ZA_LAUNCH_CH1(ZA_TABLE_C, c->linkc_p, no_clear);
#else
              if (L.use_c && ZA_CH_PAIR == 1) {
                  ZA_LAUNCH_CH1(ZA_TABLE_A, c->prev_p, d_clear);
                  ZA_LAUNCH_CH2(ZA_TABLE_B, ZA_TABLE_C, c->linkb_p, c->linkc_p, no_clear);
              } else {
                  ZA_LAUNCH_CH2(ZA_TABLE_A, ZA_TABLE_B, c->prev_p, c->linkb_p, d_clear);
                  if (L.use_c) ZA_LAUNCH_CH1(ZA_TABLE_C, c->linkc_p, no_clear);
              }
#endif
#undef ZA_LAUNCH_CH1
#undef ZA_LAUNCH_CH2
            }
            { ProfScope ps(c, ZNGAMD_K_SEARCH);
#define ZA_LAUNCH_SEARCH(...) hipLaunchKernelGGL((za_k_search<__VA_ARGS__>), dim3(nruns), dim3(ZA_SEARCH_THREADS), 0, c->stream, d_in, in_len, du, d_runs, \
                                                 c->prev_p, c->linkb_p, L.use_c ? c->linkc_p : c->linkb_p, c->best.p, c->dpcost.p, L)
              if (L.cap > 16) { if (L.use_c) ZA_LAUNCH_SEARCH(true, 0, true); else ZA_LAUNCH_SEARCH(true, 0, false); }
              else if (L.chain == 1) { if (L.use_c) ZA_LAUNCH_SEARCH(false, 1, true); else ZA_LAUNCH_SEARCH(false, 1, false); }
              else if (L.chain == 2) { if (L.use_c) ZA_LAUNCH_SEARCH(false, 2, true); else ZA_LAUNCH_SEARCH(false, 2, false); }
              else if (L.chain == 3) { if (L.use_c) ZA_LAUNCH_SEARCH(false, 3, true); else ZA_LAUNCH_SEARCH(false, 3, false); }
              else { if (L.use_c) ZA_LAUNCH_SEARCH(false, 0, true); else ZA_LAUNCH_SEARCH(false, 0, false); }
#undef ZA_LAUNCH_SEARCH
            }
            if (L.dp) {
                if (c->debug_keep) HIPCHK(c, hipMemcpyAsync(c->best_keep.p, c->best.p, (size_t)m * ZA_BEST_STRIDE * 4, hipMemcpyDeviceToDevice, c->stream));
                ProfScope ps(c, ZNGAMD_K_OPTPARSE);
                // (levels 4-6: the search took the statistics itself)
                if (L.cap > 16 || !ZA_STATS_FOLD) hipLaunchKernelGGL(za_k_dpstats, dim3(m), dim3(256), 0, c->stream, du, c->best.p, c->dpcost.p);
                hipLaunchKernelGGL(za_k_optparse, dim3(m), dim3(64), 0, c->stream, du, c->best.p, c->dpcost.p, c->tok_p, L);
            }
            { ProfScope ps(c, ZNGAMD_K_PARSE);
              if (L.min_len > ZA_MIN_MATCH)
                  hipLaunchKernelGGL(za_k_parse<true>, dim3(m), dim3(64), 0, c->stream, du, c->best.p, c->tok_p, c->segtok.p, c->hist.p,
                                     d_unit_crc + c0, c->d_crc_table, c->d_x8k, L);
              else
                  hipLaunchKernelGGL(za_k_parse<false>, dim3(m), dim3(64), 0, c->stream, du, c->best.p, c->tok_p, c->segtok.p, c->hist.p,
                                     d_unit_crc + c0, c->d_crc_table, c->d_x8k, L); }
        } else {       // level 0: stored blocks, nothing to search or parse -- only the units' CRC-32
            ProfScope ps(c, ZNGAMD_K_PARSE);
            hipLaunchKernelGGL(za_k_unit_crc, dim3(m), dim3(64), 0, c->stream, d_in, du, d_unit_crc + c0, c->d_crc_table, c->d_x8k);
        }
        if (packed) {
            { ProfScope ps(c, ZNGAMD_K_PLAN);
              hipLaunchKernelGGL(za_k_plan, dim3(m), dim3(64), 0, c->stream, du, c->hist.p, c->codes.p, c->plan.p,
                                 (uint8_t *)nullptr, 0u, level, c->hdr.p, d_unit_len + c0, fixed_only); }
            { ProfScope ps(c, ZNGAMD_K_GATHER);          // (what is left of the gather: the prefix sum)
              hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(m <= 64 ? 64 : 1024), 0, c->stream, d_unit_len + c0, m, 0u, 0ull, d_offs + c0, d_run_total,
                                 (const ZaUnit *)nullptr, c0 ? (const uint64_t *)d_run_total : (const uint64_t *)nullptr, 1); }
            { ProfScope ps(c, ZNGAMD_K_PACK);
              hipLaunchKernelGGL(za_k_pack, dim3(m), dim3(64), 0, c->stream, d_in, du, c->tok_p, c->segtok.p, c->codes.p, c->plan.p,
                                 c->segbits.p + (size_t)c0 * ZA_SEGB_STRIDE, c->cidx.p + (size_t)c0 * ZA_CIDX_STRIDE, packed->d_dst,
                                 0u, d_unit_len + c0, d_status + c0, (const uint64_t *)(d_offs + c0), packed->cap, (const uint8_t *)c->hdr.p); }
        } else {
        { ProfScope ps(c, ZNGAMD_K_PLAN);
          hipLaunchKernelGGL(za_k_plan, dim3(m), dim3(64), 0, c->stream, du, c->hist.p, c->codes.p, c->plan.p,
                             d_slots + (size_t)c0 * ZNGAMD_SLOT_STRIDE, (uint32_t)ZNGAMD_SLOT_STRIDE, level, (uint8_t *)nullptr, (uint32_t *)nullptr, fixed_only); }
        { ProfScope ps(c, ZNGAMD_K_PACK);
          hipLaunchKernelGGL(za_k_pack, dim3(m), dim3(64), 0, c->stream, d_in, du, c->tok_p, c->segtok.p, c->codes.p, c->plan.p,
                             c->segbits.p + (size_t)c0 * ZA_SEGB_STRIDE, c->cidx.p + (size_t)c0 * ZA_CIDX_STRIDE, d_slots + (size_t)c0 * ZNGAMD_SLOT_STRIDE,
                             (uint32_t)ZNGAMD_SLOT_STRIDE, d_unit_len + c0, c->status.p + c0, (const uint64_t *)nullptr, 0ull, (const uint8_t *)nullptr); }
        }
        HIPCHK(c, hipGetLastError());
    }
    c->last_units = n; c->last_single_chunk = (n <= ch); c->last_kept = c->debug_keep; c->last_unit_len = d_unit_len; c->last_ulen_on_host = false;
    return ZNGAMD_OK;
}

int zngamd_deflate_blocks_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                              int level, void *d_slots, uint32_t *d_unit_len, uint32_t *d_unit_crc, uint32_t *h_unit_block)
try {
    if (!c || (!blocks && n_blocks) || !d_slots || !d_unit_len || !d_unit_crc) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    // (a caller that compresses batch after batch with the same block table -- the reference's writer does, block size and
    // dictionary rule never change -- pays for cutting the blocks into units once)
    int r = ZNGAMD_OK;
    if (!(n_blocks && c->blocks_in.size() == n_blocks && c->blocks_len == in_len &&
          memcmp(c->blocks_in.data(), blocks, (size_t)n_blocks * sizeof(zngamd_block)) == 0)) {
        c->blocks_in.clear();
        r = build_units(c, blocks, n_blocks, in_len, c->blocks_hu);
        if (r) return r;
        c->blocks_in.assign(blocks, blocks + n_blocks); c->blocks_len = in_len;
    }
    const std::vector<ZaUnit> &hu = c->blocks_hu;
    if (h_unit_block) for (size_t i = 0; i < hu.size(); i++) h_unit_block[i] = hu[i].block;
    r = deflate_units_dev(c, (const uint8_t *)d_in, in_len, hu, level, (uint8_t *)d_slots, d_unit_len, d_unit_crc, ZA_WIN, nullptr,
                          strategy_of(blocks, n_blocks));
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// The blocks' compressed bytes back to back at d_out (no slots, no gather pass): *total_bytes and, per unit, its size, CRC-32 and
// (optional) offset.  ZNGAMD_BUF_ERROR with *total_bytes = the size needed when out_cap is too small (units that did not fit are
// not written); ZNGAMD_E_OVERFLOW never (a unit has no cap of its own here).
int zngamd_deflate_blocks_packed_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                                     int level, void *d_out, uint64_t out_cap, uint32_t *d_unit_len, uint32_t *d_unit_crc,
                                     uint64_t *d_unit_off, uint64_t *total_bytes)
try {
    if (!c || (!blocks && n_blocks) || !d_out || !d_unit_len || !d_unit_crc || !total_bytes) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    int r = ZNGAMD_OK;
    if (!(n_blocks && c->blocks_in.size() == n_blocks && c->blocks_len == in_len &&
          memcmp(c->blocks_in.data(), blocks, (size_t)n_blocks * sizeof(zngamd_block)) == 0)) {
        c->blocks_in.clear();
        r = build_units(c, blocks, n_blocks, in_len, c->blocks_hu);
        if (r) return r;
        c->blocks_in.assign(blocks, blocks + n_blocks); c->blocks_len = in_len;
    }
    const std::vector<ZaUnit> &hu = c->blocks_hu;
    *total_bytes = 0;
    if (hu.empty()) return ZNGAMD_OK;
    PackedDst pd; pd.d_dst = (uint8_t *)d_out; pd.cap = out_cap; pd.d_unit_off = d_unit_off;
    r = deflate_units_dev(c, (const uint8_t *)d_in, in_len, hu, level, nullptr, d_unit_len, d_unit_crc, ZA_WIN, &pd, strategy_of(blocks, n_blocks));
    if (r) return r;
    const uint64_t *d_run_total = (const uint64_t *)((const uint8_t *)c->d_small + 224);
    std::vector<uint32_t> st(hu.size());
    HIPCHK(c, hipMemcpyAsync(total_bytes, d_run_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, st.size() * 4ull, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (*total_bytes > out_cap) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    // a unit whose packed size is not the planned one would have shifted everything behind it: never expected, always checked
    for (uint32_t v : st) if (v) return fail(c, ZNGAMD_E_HIP, "packed deflate: a unit's size differs from its plan");
    return ZNGAMD_OK;
} ZA_ABI_GUARD

static int gather_dev(zngamd_ctx *c, const uint8_t *d_slots, const uint32_t *d_unit_len, uint32_t n, uint32_t extra,
                      uint8_t *d_dst, uint64_t dst_base, uint64_t dst_cap, uint64_t *d_unit_off, uint64_t *total, bool do_copy,
                      const ZaUnit *d_units_for_index = nullptr)
{
    if (n == 0) { *total = 0; return ZNGAMD_OK; }
    uint64_t *offs = d_unit_off;
    if (!offs) { HIPCHK(c, c->st_off.ensure(n)); offs = c->st_off.p; }
    uint64_t *d_total = (uint64_t *)c->d_small;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(1024), 0, c->stream, d_unit_len, n, extra, dst_base, offs, d_total, d_units_for_index); }
    HIPCHK(c, hipMemcpyAsync(total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dst_base + *total > dst_cap) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    if (do_copy) {
        ProfScope ps(c, ZNGAMD_K_GATHER);
        hipLaunchKernelGGL(za_k_gather, dim3(n), dim3(256), 0, c->stream, d_slots, (uint32_t)ZNGAMD_SLOT_STRIDE, d_unit_len, offs, d_dst);
    }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_gather_dev(zngamd_ctx *c, const void *d_slots, const uint32_t *d_unit_len, uint32_t n_units, void *d_dst,
                      uint64_t dst_base, uint64_t dst_cap, uint64_t *d_unit_off, uint64_t *total_bytes)
try {
    if (!c || !d_slots || !d_unit_len || !d_dst || !total_bytes) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = gather_dev(c, (const uint8_t *)d_slots, d_unit_len, n_units, 0, (uint8_t *)d_dst, dst_base, dst_cap, d_unit_off, total_bytes, true);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// shared by the two host-buffer entry points: input already staged at st_in.p
// pinned host memory for results that are re-distributed on the host afterwards: a device-to-host copy into pinned memory
// runs at link speed, into fresh pageable memory several times slower
static int host_stage(zngamd_ctx *c, size_t bytes, uint8_t **p)
{
    if (bytes > c->h_stage_cap) {
        if (c->h_stage) (void)hipHostFree(c->h_stage);
        c->h_stage = nullptr; c->h_stage_cap = 0;
        const size_t want = bytes + bytes / 4 + (1u << 20);
        HIPCHK(c, hipHostMalloc((void **)&c->h_stage, want, hipHostMallocDefault));
        c->h_stage_cap = want;
    }
    *p = c->h_stage;
    return ZNGAMD_OK;
}

// Host copies of payload: several threads for large pieces.  A result usually lands in memory the process has never touched
// (a Python bytes object made for this call): the first touch of a page costs far more than the copy, one thread reaches
// 12 GB/s there, and the device-to-host DMA itself 56 GB/s (profiles/r03_pcie.txt).
static void par_memcpy(uint8_t *dst, const uint8_t *src, size_t n)
{
    const size_t piece = 4u << 20;
    static const long env_threads = [] { const char *e = getenv("ZNGAMD_COPY_THREADS"); return e ? atol(e) : 0L; }();      // (read once, not per piece)
    unsigned hw = std::thread::hardware_concurrency();
    size_t t = std::min<size_t>(std::min<size_t>(hw ? hw / 2 : 4, 8), n / piece);
    if (env_threads >= 1 && env_threads <= 64) t = std::min<size_t>((size_t)env_threads, std::max<size_t>(n / (1u << 20), 1));
    if (t <= 1) { memcpy(dst, src, n); return; }
    const size_t step = ((n / t) + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    th.reserve(t);
    size_t started_to = step;                                  // bytes [0, started_to) have a copier (this thread takes the first piece)
    for (size_t i = 1; i < t; i++) {
        const size_t o = i * step;
        if (o >= n) break;
        // a thread that cannot be started (EAGAIN under a pids limit) must not unwind through the joinable ones -- that is
        // std::terminate(), the host process gone: whatever has no copier yet is copied here
        try { th.emplace_back([=] { memcpy(dst + o, src + o, std::min(step, n - o)); }); }
        catch (...) { break; }
        started_to = std::min(n, o + step);
    }
    memcpy(dst, src, std::min(step, n));
    if (started_to < n) memcpy(dst + started_to, src + started_to, n - started_to);
    for (auto &x : th) x.join();
}

// Decoded / compressed payload to the caller's buffer, PIPELINED through two halves of the pinned staging buffer: the DMA of
// piece k + 1 runs while the host threads copy piece k into the caller's (usually fresh) memory.  Copying straight into fresh
// pageable memory makes the driver pin its pages and unpin them when the object is cut to size afterwards -- 25 ms of fixed
// cost for a 3 MiB result, and 12 GB/s at best for a large one.
#define ZNGAMD_D2H_PIECE (16ull << 20)
static int d2h_payload(zngamd_ctx *c, uint8_t *dst, const uint8_t *src_dev, uint64_t n)
{
    if (!n) return ZNGAMD_OK;
    PhaseClock pc(c, "d2h_payload (device -> caller)");
    const uint64_t piece = std::min<uint64_t>(ZNGAMD_D2H_PIECE, n);
    uint8_t *st = nullptr;
    int r = host_stage(c, n <= piece ? n : 2 * piece, &st);
    if (r) return r;
    if (!c->ev_copy[0]) { HIPCHK(c, hipEventCreateWithFlags(&c->ev_copy[0], hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&c->ev_copy[1], hipEventDisableTiming)); }
    const uint64_t np = (n + piece - 1) / piece;
    double wait_ms = 0, copy_ms = 0;
    for (uint64_t k = 0; k <= np; k++) {
        if (k < np) {
            const uint64_t o = k * piece, ln = std::min(piece, n - o);
            HIPCHK(c, hipMemcpyAsync(st + (k & 1) * piece, src_dev + o, ln, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(c->ev_copy[k & 1], c->stream));
        }
        if (k > 0) {
            const uint64_t o = (k - 1) * piece, ln = std::min(piece, n - o);
            const auto t0 = std::chrono::steady_clock::now();
            HIPCHK(c, hipEventSynchronize(c->ev_copy[(k - 1) & 1]));
            const auto t1 = std::chrono::steady_clock::now();
            par_memcpy(dst + o, st + ((k - 1) & 1) * piece, ln);
            if (trace_on()) { wait_ms += std::chrono::duration<double, std::milli>(t1 - t0).count(); copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count(); }
        }
    }
    if (trace_on()) fprintf(stderr, "zng_amd trace:   d2h: waiting for the DMA %.3f ms, host copies %.3f ms (%llu pieces)\n", wait_ms, copy_ms, (unsigned long long)np);
    return ZNGAMD_OK;
}

// (optional) a checksum of the staged input worked out beside the deflate kernels; its partial results travel with theirs
struct CkReq { bool want_crc = false, want_adler = false; std::vector<ZaCkPart> parts; };

static int deflate_host_common(zngamd_ctx *c, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks, int level,
                               std::vector<ZaUnit> &hu, std::vector<uint32_t> &ulen, std::vector<uint32_t> &ucrc,
                               const uint8_t **packed, int max_dist = ZA_WIN,
                               uint8_t *direct_out = nullptr, uint64_t direct_cap = 0, uint64_t *direct_len = nullptr, CkReq *ck = nullptr)
{
    int r;
    { PhaseClock pc(nullptr, "build_units"); r = build_units(c, blocks, n_blocks, in_len, hu); }
    if (r) return r;
    const uint32_t n = (uint32_t)hu.size();
    // Packed: every unit's size is planned before it is packed and the packer writes at its final offset (no slots, no gather).
    // The stream's bound is the sum of its units' (unit_bound: a unit's stored form, under Z_FIXED nine bits a byte).
    const int strategy = strategy_of(blocks, n_blocks);
    uint64_t bound = 64;
    for (const ZaUnit &u : hu) bound += unit_bound(u.in_len, strategy);
    // Everything the host wants back lies in ONE device buffer, the results in front of the stream -- the stream's size, the units'
    // sizes, CRCs and pack status, the checksum kernel's partial sums -- so that a small call fetches results and bytes with one
    // copy (r06: five copies of a few bytes each, staged one after the other, cost a small call 60 us):
    //   [0, 16) size of the stream | [16, ..) n sizes | n CRCs | n status words | checksum parts | (to a multiple of 256) the stream
    const uint64_t nspan = ck ? (in_len + ZA_MAX_UNIT - 1) / ZA_MAX_UNIT : 0;
    const uint64_t o_len = 16, o_crc = o_len + 4ull * n, o_st = o_crc + 4ull * n, o_ck = (o_st + 4ull * n + 15) & ~15ull;
    const uint64_t head = (o_ck + nspan * sizeof(ZaCkPart) + 255) & ~255ull;
    HIPCHK(c, c->st_out.ensure(head + bound));
    uint8_t *d_head = c->st_out.p;
    PackedDst pd; pd.d_dst = d_head + head; pd.cap = bound; pd.d_unit_off = nullptr;
    pd.d_total = (uint64_t *)d_head; pd.d_status = (uint32_t *)(d_head + o_st);
    if (ck && nspan) {
        // the container's checksum: its kernel goes out in front of the deflate kernels and is waited for with them
        ProfScope ps(c, ZNGAMD_K_OTHER);
        hipLaunchKernelGGL(za_k_checksum, dim3((uint32_t)nspan), dim3(256), 0, c->stream, (const uint8_t *)c->st_in.p, in_len, c->d_crc_slice4,
                           (ZaCkPart *)(d_head + o_ck), ck->want_crc ? 1 : 0, ck->want_adler ? 1 : 0);
    }
    { PhaseClock pc(c, "deflate kernels");
      r = deflate_units_dev(c, c->st_in.p, in_len, hu, level, nullptr, (uint32_t *)(d_head + o_len), (uint32_t *)(d_head + o_crc), max_dist, &pd,
                            strategy_of(blocks, n_blocks)); }
    if (r) return r;
    const bool direct = direct_out != nullptr;
    // One round trip for the results, and for a small stream the bytes as well (its upper bound travels: the size is not known yet)
    const uint64_t EAGER = 512u << 10;
    uint8_t *stage = nullptr;
    const bool eager = bound <= EAGER;
    { int rs = host_stage(c, head + (eager ? bound : 0), &stage); if (rs) return rs; }
    {
        PhaseClock pc(c, "results to the host");
        HIPCHK(c, hipMemcpyAsync(stage, d_head, head + (eager ? bound : 0), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->up_busy = false; c->tab_busy = false;                       // (the stream has drained: the upload buffers are free)
    prof_collect(c);
    uint64_t total = 0;
    memcpy(&total, stage, 8);
    ulen.resize(n); ucrc.resize(n);
    if (n) { memcpy(ulen.data(), stage + o_len, 4ull * n); memcpy(ucrc.data(), stage + o_crc, 4ull * n); }
    c->last_ulen_host = ulen; c->last_ulen_on_host = true;
    const uint32_t *st = (const uint32_t *)(stage + o_st);
    for (uint32_t i = 0; i < n; i++) if (st[i]) return fail(c, ZNGAMD_E_HIP, "packed deflate: a unit's size differs from its plan");
    if (total > bound) return fail(c, ZNGAMD_E_HIP, "packed deflate: stream larger than its bound");
    if (ck) { ck->parts.resize(nspan); if (nspan) memcpy(ck->parts.data(), stage + o_ck, nspan * sizeof(ZaCkPart)); }
    // one-shot callers take the packed stream straight into their buffer (no intermediate copy)
    if (direct) { *direct_len = total; if (total > direct_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
    if (eager) {
        if (direct) memcpy(direct_out, stage + head, total); else *packed = stage + head;
        return ZNGAMD_OK;
    }
    if (!direct) { int rs = host_stage(c, total, &stage); if (rs) return rs; *packed = stage; }
    if (total && !direct) { HIPCHK(c, hipMemcpyAsync(stage, pd.d_dst, total, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    if (total && direct) { const int rc_ = d2h_payload(c, direct_out, pd.d_dst, total); if (rc_) return rc_; HIPCHK(c, hipStreamSynchronize(c->stream)); }
    return ZNGAMD_OK;
}

int zngamd_deflate_blocks(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                          int level, uint8_t *out, uint64_t out_cap_per_block, uint32_t *out_len, uint32_t *crc)
try {
    if (!c || (!in && in_len) || (!blocks && n_blocks) || !out || !out_len || !crc) return ZNGAMD_E_ARG;
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    std::lock_guard<std::mutex> g(c->mu);
    int r = stage_in(c, in, in_len);
    if (r) return r;
    std::vector<ZaUnit> hu; std::vector<uint32_t> ulen, ucrc; const uint8_t *packed = nullptr;
    const uint32_t wb = n_blocks ? (blocks[0].flags >> 8) & 15u : 0u;
    if (wb != 0 && wb < 9) return fail(c, ZNGAMD_STREAM_ERROR, "window bits must be 9..15");
    r = deflate_host_common(c, in_len, blocks, n_blocks, level, hu, ulen, ucrc, &packed, wb ? (1 << wb) : ZA_WIN);
    if (r) return r;
    int ret = ZNGAMD_OK;
    size_t pos = 0, u = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint64_t tot = 0; uint32_t bc = 0; size_t start = pos;
        bool first = true;
        for (; u < hu.size() && hu[u].block == b; u++) {
            tot += ulen[u]; pos += ulen[u];
            bc = first ? ucrc[u] : zngamd_crc32_combine(bc, ucrc[u], hu[u].in_len);
            first = false;
        }
        crc[b] = bc;
        if (tot >= out_cap_per_block) { out_len[b] = 0xFFFFFFFFu; ret = ZNGAMD_E_OVERFLOW; continue; }
        memcpy(out + (size_t)b * out_cap_per_block, packed + start, tot);
        out_len[b] = (uint32_t)tot;
    }
    if (ret) c->err = "Compressed output exceeds buffer size";
    return ret;
} ZA_ABI_GUARD

static int deflate_blocks_packed_locked(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                                        int level, uint8_t *out, uint64_t out_cap, uint64_t block_cap, uint32_t *out_len, uint32_t *crc, uint64_t *total)
{
    *total = 0;
    int r = stage_in(c, in, in_len);
    if (r) return r;
    std::vector<ZaUnit> hu; std::vector<uint32_t> ulen, ucrc; const uint8_t *packed = nullptr;
    const uint32_t wb = n_blocks ? (blocks[0].flags >> 8) & 15u : 0u;
    if (wb != 0 && wb < 9) return fail(c, ZNGAMD_STREAM_ERROR, "window bits must be 9..15");
    r = deflate_host_common(c, in_len, blocks, n_blocks, level, hu, ulen, ucrc, &packed, wb ? (1 << wb) : ZA_WIN, out, out_cap, total);
    if (r == ZNGAMD_BUF_ERROR && !hu.empty()) {
        // the packed stream does not fit: because a block outgrew its cap (an overflow, reported like the per-block form does),
        // or because the caller's buffer is simply too small (ZNGAMD_BUF_ERROR, *total = the size needed)
        // (the units' sizes came back with the results: deflate_host_common fills `ulen` before it looks at the caller's room)
        if (ulen.size() != hu.size()) return r;
        bool any = false;
        size_t u2 = 0;
        for (uint32_t b = 0; b < n_blocks; b++) {
            uint64_t tot = 0;
            for (; u2 < hu.size() && hu[u2].block == b; u2++) tot += ulen[u2];
            crc[b] = 0;
            out_len[b] = tot >= block_cap ? 0xFFFFFFFFu : (uint32_t)tot;
            any = any || tot >= block_cap;
        }
        if (any) { c->err = "Compressed output exceeds buffer size"; return ZNGAMD_E_OVERFLOW; }
    }
    if (r) return r;
    int ret = ZNGAMD_OK;
    size_t u = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint64_t tot = 0; uint32_t bc = 0;
        bool first = true;
        for (; u < hu.size() && hu[u].block == b; u++) {
            tot += ulen[u];
            bc = first ? ucrc[u] : zngamd_crc32_combine(bc, ucrc[u], hu[u].in_len);
            first = false;
        }
        crc[b] = bc;
        if (tot >= block_cap) { out_len[b] = 0xFFFFFFFFu; ret = ZNGAMD_E_OVERFLOW; continue; }
        out_len[b] = (uint32_t)tot;
    }
    if (ret) c->err = "Compressed output exceeds buffer size";
    return ret;
}

int zngamd_deflate_blocks_packed(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                                 int level, uint8_t *out, uint64_t out_cap, uint64_t block_cap, uint32_t *out_len, uint32_t *crc, uint64_t *total)
try {
    if (!c || (!in && in_len) || (!blocks && n_blocks) || !out || !out_len || !crc || !total) return ZNGAMD_E_ARG;
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    std::lock_guard<std::mutex> g(c->mu);
    return deflate_blocks_packed_locked(c, in, in_len, blocks, n_blocks, level, out, out_cap, block_cap, out_len, crc, total);
} ZA_ABI_GUARD

static int deflate_index_locked(zngamd_ctx *c, uint32_t n_units, uint32_t *unit_in_len, uint32_t *unit_out_len, uint32_t *rows);
// The packed call and the segment index of ITS units in one: a context shared by several writer threads would otherwise have to
// keep them from slipping a deflate call of their own between a thread's two calls (zngamd_deflate_index answers for the
// context's last deflate call, whoever made it).
int zngamd_deflate_blocks_packed_indexed(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                                         int level, uint8_t *out, uint64_t out_cap, uint64_t block_cap, uint32_t *out_len, uint32_t *crc, uint64_t *total,
                                         uint32_t n_units, uint32_t *unit_in_len, uint32_t *unit_out_len, uint32_t *rows)
try {
    if (!c || (!in && in_len) || (!blocks && n_blocks) || !out || !out_len || !crc || !total || !unit_in_len || !unit_out_len || !rows) return ZNGAMD_E_ARG;
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (n_units != zngamd_count_units(blocks, n_blocks)) return fail(c, ZNGAMD_E_ARG, "n_units is not what zngamd_count_units says for these blocks");
    std::lock_guard<std::mutex> g(c->mu);
    const int r = deflate_blocks_packed_locked(c, in, in_len, blocks, n_blocks, level, out, out_cap, block_cap, out_len, crc, total);
    if (r) return r;
    return deflate_index_locked(c, n_units, unit_in_len, unit_out_len, rows);
} ZA_ABI_GUARD

int zngamd_deflate_stream(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, int level, int window_bits, uint8_t *out,
                          uint64_t out_cap, uint64_t *out_len, uint32_t *crc, uint32_t *adler)
try {
    if (!c || (!in && in_len) || !out || !out_len) return ZNGAMD_E_ARG;
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (in_len > 0xFFFFFFFFull) return fail(c, ZNGAMD_E_ARG, "one-shot input limited to 4 GiB - 1");
    std::lock_guard<std::mutex> g(c->mu);
    int r = stage_in(c, in, in_len);
    if (r) return r;
    zngamd_block B; B.off = 0; B.len = (uint32_t)in_len; B.dict_len = 0; B.flags = ZNGAMD_FLAG_FINAL; B.reserved = 0;
    // a call of up to one unit's size is cut into units of 16 KiB (oracle: za_o_deflate_stream): eight wavefronts instead of one
    if (in_len <= ZA_MAX_UNIT) B.flags |= ZNGAMD_FLAG_UNITS16K;
    std::vector<ZaUnit> hu; std::vector<uint32_t> ulen, ucrc; const uint8_t *packed = nullptr;
    if (window_bits < 9 || window_bits > 15) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    // the zlib container's Adler-32: its kernel goes out in front of the deflate kernels and its sums come back with their results
    CkReq ck; ck.want_adler = adler != nullptr;
    r = deflate_host_common(c, in_len, &B, 1, level, hu, ulen, ucrc, &packed, 1 << window_bits, out, out_cap, out_len, adler ? &ck : nullptr);
    if (r) { (void)hipStreamSynchronize(c->stream); return r; }
    if (crc) { uint32_t v = 0; for (size_t u = 0; u < hu.size(); u++) v = u ? zngamd_crc32_combine(v, ucrc[u], hu[u].in_len) : ucrc[u]; *crc = v; }
    if (adler) { uint32_t a = 1; checksum_fold(ck.parts, nullptr, &a); *adler = a; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_debug_keep(zngamd_ctx *c, int on)
try {
    if (!c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    c->debug_keep = on != 0;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_debug_fetch(zngamd_ctx *c, int what, uint32_t unit, void *dst, size_t bytes)
try {
    if (!c || !dst) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (unit >= c->last_units || !c->last_single_chunk) return fail(c, ZNGAMD_E_ARG, "unit not resident");
    const void *src = nullptr; size_t lim = 0;
    switch (what) {
    case 0: src = c->prev_p ? c->prev_p + (size_t)unit * ZA_PREV_STRIDE : nullptr; lim = ZA_PREV_STRIDE * 2ull; break;
    case 1: src = c->best.p + (size_t)unit * ZA_BEST_STRIDE; lim = ZA_BEST_STRIDE * 4ull; break;
    case 2: src = c->tok_p ? c->tok_p + (size_t)unit * ZA_TOK_STRIDE : nullptr; lim = ZA_TOK_STRIDE * 4ull; break;
    case 3: src = c->segtok.p + (size_t)unit * ZA_MAX_SEGS; lim = ZA_MAX_SEGS * 4ull; break;
    case 4: src = c->hist.p + (size_t)unit * ZA_HIST_STRIDE; lim = ZA_HIST_STRIDE * 4ull; break;
    case 5: src = c->codes.p + (size_t)unit * ZA_CODE_STRIDE; lim = ZA_CODE_STRIDE * 4ull; break;
    case 6: src = c->segbits.p + (size_t)unit * ZA_SEGB_STRIDE; lim = ZA_SEGB_STRIDE * 4ull; break;
    case 7: src = c->plan.p + unit; lim = sizeof(ZaPlan); break;
    case 8: src = c->cidx.p + (size_t)unit * ZA_CIDX_STRIDE; lim = ZA_CIDX_STRIDE * 4ull; break;
    case 9: src = c->linkb_p ? c->linkb_p + (size_t)unit * ZA_PREV_STRIDE : nullptr; lim = ZA_PREV_STRIDE * 2ull; break;
    case 10: src = c->linkc_p ? c->linkc_p + (size_t)unit * ZA_PREV_STRIDE : nullptr; lim = ZA_PREV_STRIDE * 2ull; break;
    case 11: src = c->best_keep.p ? c->best_keep.p + (size_t)unit * ZA_BEST_STRIDE : nullptr; lim = ZA_BEST_STRIDE * 4ull; break;
    case 12: src = c->dpcost.p ? c->dpcost.p + (size_t)unit * ZA_DP_COSTS : nullptr; lim = ZA_DP_COSTS * 4ull; break;
    default: return fail(c, ZNGAMD_E_ARG, "unknown stage");
    }
    if (!src || bytes > lim) return fail(c, ZNGAMD_E_ARG, "stage not available");
    // (without zngamd_debug_keep the token words are written over the link tables: only one of the two survives a call)
    if (!c->last_kept && (what == 0 || what == 9 || what == 10)) return fail(c, ZNGAMD_E_ARG, "link tables are kept only after zngamd_debug_keep(1): the token words take their place");
    HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    if ((what == 0 || what == 9 || what == 10) && unit < c->last_hu.size() && (c->last_hu[unit].flags & ZA_FLAG_CARRY) && !(c->last_hu[unit].flags & ZA_FLAG_RUNHEAD) && unit > 0) {
        // a unit whose chain tables were carried over: the links of its dictionary are the links of the last 32 KiB of the unit in
        // front of it (that unit's row) -- all but the last few (context length - 1), which this unit inserted itself; links that
        // reach in front of the dictionary are "no link" for this unit
        const ZaUnit &u = c->last_hu[unit], &pv = c->last_hu[unit - 1];
        const uint16_t *tab = what == 0 ? c->prev_p : what == 9 ? c->linkb_p : c->linkc_p;
        const size_t late = (what == 0 ? ZA_HASH_BYTES_A : what == 9 ? ZA_HASH_BYTES_B : ZA_HASH_BYTES_C) - 1;
        const size_t nd = std::min<size_t>(bytes / 2, u.dict_len - late);
        uint16_t *d16 = (uint16_t *)dst;
        HIPCHK(c, hipMemcpy(d16, tab + (size_t)(unit - 1) * ZA_PREV_STRIDE + pv.dict_len + pv.in_len - u.dict_len, nd * 2, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nd; i++) if (d16[i] > i) d16[i] = 0;
    }
    if (what == 1 || what == 11) {     // the kernels' entry (distance - 1 | length << 15 | the position's byte << 24) in the documented form len << 16 | dist
        uint32_t *e = (uint32_t *)dst;
        for (size_t i = 0; i < bytes / 4; i++) { const uint32_t lf = ZA_ELEN(e[i]); e[i] = lf ? (lf << 16) | ZA_EDIST(e[i]) : 0u; }
    }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---------------------------------------------------------------------------------------------
// inflate
// ---------------------------------------------------------------------------------------------
static int map_status(int s)
{
    switch (s) {
    case ZA_I_OK: return ZNGAMD_OK;
    case ZA_I_END: return ZNGAMD_STREAM_END;
    case ZA_I_DATA: return ZNGAMD_DATA_ERROR;
    case ZA_I_INPUT: case ZA_I_OUTFULL: return ZNGAMD_BUF_ERROR;
    case ZA_I_CRC: return ZNGAMD_E_GZ_CRC;
    case ZA_I_LENGTH: return ZNGAMD_E_GZ_LENGTH;
    default: return ZNGAMD_DATA_ERROR;
    }
}

// sequential decode of one raw stream that already sits (padded) on the device
static int inflate_serial_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const uint8_t *d_dict, uint32_t dict_len,
                              uint8_t *d_out, uint64_t out_cap, ZaInfResult *hres, uint32_t start_bit = 0)
{
    ZaInfResult *dres = (ZaInfResult *)((uint8_t *)c->d_small + 64);
    { ProfScope ps(c, ZNGAMD_K_INFLATE);
      hipLaunchKernelGGL(za_k_inflate_serial, dim3(1), dim3(ZA_SERIAL_THREADS), 0, c->stream, d_in, in_len, start_bit, d_dict, dict_len, d_out, out_cap, dres); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hres, dres, sizeof(ZaInfResult), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
}

// a stream that is resumed at a block header (bit offset + history) and / or may run past the end of the buffer
struct ChunkOpts { uint32_t start_bit = 0; const uint8_t *d_dict = nullptr; uint32_t dict_len = 0; bool allow_cut = false; };
struct ChunkInfo { bool cut = false; bool ended = false; uint64_t end_bit = 0; uint64_t last_bit = 0, last_out = 0; };    // last_*: the last listed block header the chain entered, and the output in front of it
// from this many chunks (or block candidates) on, the chunk kernels run in their small-LDS size: more than the 1 024
// wavefronts the large size keeps resident (256 CUs x 4 workgroups)
#ifndef ZNGAMD_CHUNKS_SMALL_FROM
#define ZNGAMD_CHUNKS_SMALL_FROM 1u             // (r03: with three passes at most and sweeps that follow one another the 512-bit footprint wins at every chunk count -- 512 chunks 3.94 -> 3.38 ms, 1 408 chunks 4.08 -> 3.76 ms; the 1 024-bit one, 4 per CU, stays compiled for comparison: -DZNGAMD_CHUNKS_SMALL_FROM=1536u)
#endif
#ifndef ZNGAMD_CHUNKS_MANY_FROM
#define ZNGAMD_CHUNKS_MANY_FROM 2049u          // more chunks than the middle footprint holds at once (8 per CU x 256): the smallest footprint (384-bit sub-sequences, queue of 768, 256 symbols of ring, decode tables of 9 / 8 index bits: 16 per CU) wins -- 320 MiB of this engine's stream 7.1 -> 4.9 ms, 1 GiB 15.2 -> 10.4 ms
#endif
#ifndef ZA_CHUNK_Q_M
#define ZA_CHUNK_Q_M 768               // the marker decoder where chunks outnumber the wavefronts: queue entries, symbols of history in LDS (768 / 256: 16 per CU, 1 GiB 12.4 -> 10.4 ms; 768 / 512 11.8, 1 024 / 256 12.1)
#endif
#ifndef ZA_CHUNK_RING_M
#define ZA_CHUNK_RING_M 256
#endif
#ifndef ZA_CHUNK_LB_2P
#define ZA_CHUNK_LB_2P ZA_LUT_L_BITS     // table index bits of the marker decoder behind a count pass (streams of other writers)
#define ZA_CHUNK_DB_2P ZA_LUT_D_BITS
#endif
#ifndef ZA_CHUNK_BITS_S
#define ZA_CHUNK_BITS_S 512          // the marker decoder where chunks are many: bits per sub-sequence, queue entries, symbols of history in LDS
#endif
#ifndef ZA_CHUNK_Q_S
#define ZA_CHUNK_Q_S 1536
#endif
#ifndef ZA_CHUNK_RING_S
#define ZA_CHUNK_RING_S 1024
#endif
static int inflate_chunked_dev(zngamd_ctx *c, const uint8_t *d_def, uint64_t avail, uint8_t *d_out, uint64_t out_room,
                               uint64_t *out_len, uint64_t *in_used, const ChunkOpts &o = ChunkOpts(), ChunkInfo *info = nullptr);
static int inflate_chunked_once(zngamd_ctx *c, const uint8_t *d_def, uint64_t avail, uint8_t *d_out, uint64_t out_room,
                                uint64_t *out_len, uint64_t *in_used, const ChunkOpts &o, ChunkInfo *info);

int zngamd_inflate_raw(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const uint8_t *dict, uint32_t dict_len,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *in_used, uint32_t *crc, uint32_t *adler)
try {
    if (!c || (!in && in_len) || (!out && out_cap) || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (dict_len > ZA_WIN) { dict += dict_len - ZA_WIN; dict_len = ZA_WIN; }
    // staging layout: [dictionary, padded to 64][stream][64 zero bytes]
    const uint64_t front = (dict_len + 63u) & ~63ull;
    int r = stage_in(c, in, in_len, front);
    if (r) return r;
    if (dict_len) HIPCHK(c, hipMemcpyAsync(c->st_in.p, dict, dict_len, hipMemcpyHostToDevice, c->stream));
    if (in_len < (1u << 16) && out_cap <= (512u << 10)) {
        // A small call (r06): the decoder, the checksum kernel -- which takes the output's length from where the decoder left it --
        // and ONE copy that brings result, checksum parts and the bytes up to the caller's limit, behind one synchronisation (the
        // result, the parts and the payload each had a round trip of their own: 60 of a 1 KiB call's 330 us).
        const uint64_t head = 256;                                   // [0, 40) the decoder's result | [64, 128) checksum parts of up to four spans | the output
        const uint64_t nspan = (crc || adler) ? (out_cap + ZA_MAX_UNIT - 1) / ZA_MAX_UNIT : 0;
        HIPCHK(c, c->st_out.ensure(head + out_cap + 64));
        ZaInfResult *dres = (ZaInfResult *)c->st_out.p;
        // (the output is assembled in LDS by za_k_inflate_serial_small; a stream that outgrows the image -- ZA_SMALL_IMG bytes --
        // comes back as "output full" at exactly that size and goes to the ordinary kernel: second == true)
        static const bool no_img = getenv("ZNGAMD_NO_SMALL_IMAGE") != nullptr;
        for (int second = no_img ? 1 : 0; second < 2; second++) {
        { ProfScope ps(c, ZNGAMD_K_INFLATE);
          if (second) hipLaunchKernelGGL(za_k_inflate_serial, dim3(1), dim3(ZA_SERIAL_THREADS), 0, c->stream, (const uint8_t *)(c->st_in.p + front), in_len, 0u, (const uint8_t *)c->st_in.p, dict_len,
                             c->st_out.p + head, out_cap, dres);
          else hipLaunchKernelGGL(za_k_inflate_serial_small, dim3(1), dim3(128), 0, c->stream, (const uint8_t *)(c->st_in.p + front), in_len, 0u, (const uint8_t *)c->st_in.p, dict_len,
                             c->st_out.p + head, out_cap, dres); }
        if (nspan) {
            ProfScope ps(c, ZNGAMD_K_OTHER);
            hipLaunchKernelGGL(za_k_checksum, dim3((uint32_t)nspan), dim3(256), 0, c->stream, (const uint8_t *)(c->st_out.p + head), out_cap, c->d_crc_slice4,
                               (ZaCkPart *)(c->st_out.p + 64), crc ? 1 : 0, adler ? 1 : 0, (const uint64_t *)&dres->out_len);
        }
        HIPCHK(c, hipGetLastError());
        uint8_t *stage = nullptr;
        r = host_stage(c, head + out_cap, &stage);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(stage, c->st_out.p, head + out_cap, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->up_busy = false;
        prof_collect(c);
        ZaInfResult res;
        memcpy(&res, stage, sizeof res);
        if (!second && res.status == ZA_I_OUTFULL && res.out_len == (uint64_t)ZA_SMALL_IMG && out_cap > (uint64_t)ZA_SMALL_IMG) continue;      // the image was full, the caller's buffer is not
        c->paths[ZNGAMD_PATH_SEQUENTIAL]++;
        *out_len = res.out_len;
        if (in_used) *in_used = (res.in_bits + 7) >> 3;
        if (nspan) {
            std::vector<ZaCkPart> parts(nspan);
            memcpy(parts.data(), stage + 64, nspan * sizeof(ZaCkPart));
            uint32_t cv = 0, av = 1;
            checksum_fold(parts, crc ? &cv : nullptr, adler ? &av : nullptr);
            if (crc) *crc = cv;
            if (adler) *adler = av;
        }
        if (res.out_len) memcpy(out, stage + head, res.out_len <= out_cap ? res.out_len : out_cap);
        if (res.status == ZA_I_DATA) c->err = "invalid deflate data";
        return map_status(res.status);
        }
        return fail(c, ZNGAMD_E_HIP, "small inflate: no result");       // (not reached: the second pass always returns)
    }
    HIPCHK(c, c->st_out.ensure(out_cap + 64));
    ZaInfResult res;
    bool chunked = false;
    if (dict_len == 0) {
        // large complete streams: chunk-parallel (sync-flush points / dynamic block headers), see zngamd_gunzip
        uint64_t clen = 0, cused = 0;
        const int cr = inflate_chunked_dev(c, c->st_in.p + front, in_len, c->st_out.p, out_cap, &clen, &cused);
        if (cr < 0 && cr != ZNGAMD_BUF_ERROR) return cr;
        if (cr == ZNGAMD_BUF_ERROR) { *out_len = clen; if (in_used) *in_used = 0; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
        if (cr == 0) { chunked = true; res.status = ZA_I_END; res.out_len = clen; res.in_bits = cused * 8; res.block_bits = 0; res.block_out = 0; }
    }
    if (!chunked) {
        r = inflate_serial_dev(c, c->st_in.p + front, in_len, c->st_in.p, dict_len, c->st_out.p, out_cap, &res);
        if (r) return r;
    }
    c->paths[chunked ? ZNGAMD_PATH_CHUNKED : ZNGAMD_PATH_SEQUENTIAL]++;
    *out_len = res.out_len;
    if (in_used) *in_used = (res.in_bits + 7) >> 3;
    if (crc || adler) {                       // (before the payload leaves: the kernel is short, the copies keep the host busy for milliseconds)
        uint32_t cv = 0, av = 1;
        r = checksum_dev(c, c->st_out.p, res.out_len, crc ? &cv : nullptr, adler ? &av : nullptr);
        if (r) return r;
        if (crc) *crc = cv;
        if (adler) *adler = av;
    }
    if (res.out_len) { const int rc_ = d2h_payload(c, out, c->st_out.p, res.out_len); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (res.status == ZA_I_DATA) c->err = "invalid deflate data";
    return map_status(res.status);
} ZA_ABI_GUARD


int zngamd_inflate_resume(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t start_bit, const uint8_t *dict, uint32_t dict_len,
                          uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *in_bits, uint64_t *block_bits, uint64_t *block_out)
try {
    if (!c || (!in && in_len) || (!out && out_cap) || !out_len || !in_bits || !block_bits || !block_out || start_bit > 7) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (dict_len > ZA_WIN) { dict += dict_len - ZA_WIN; dict_len = ZA_WIN; }
    const uint64_t front = (dict_len + 63u) & ~63ull;
    int r = stage_in(c, in, in_len, front);
    if (r) return r;
    if (dict_len) HIPCHK(c, hipMemcpyAsync(c->st_in.p, dict, dict_len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->st_out.ensure(out_cap + 64));
    ZaInfResult res;
    bool chunked = false;
    if (in_len >= (1u << 16)) {
        // a large piece of a stream: its complete blocks are decoded chunk-parallel; what follows the last complete block
        // stays for the next call (the checkpoint is exactly that boundary)
        ChunkOpts o; o.start_bit = start_bit; o.d_dict = c->st_in.p; o.dict_len = dict_len; o.allow_cut = true;
        ChunkInfo ci;
        uint64_t clen = 0, cused = 0;
        const int cr = inflate_chunked_dev(c, c->st_in.p + front, in_len, c->st_out.p, out_cap, &clen, &cused, o, &ci);
        if (cr < 0 && cr != ZNGAMD_BUF_ERROR) return cr;
        if (cr == 0) {
            chunked = true;
            res.status = ci.ended ? ZA_I_END : ZA_I_INPUT; res.out_len = clen; res.in_bits = ci.end_bit;
            // the checkpoint: the header of the block that was cut off; of a stream that ended, the last listed header it entered
            res.block_bits = ci.ended ? ci.last_bit : ci.end_bit; res.block_out = ci.ended ? ci.last_out : clen;
        }   // (not enough room, or nothing to gain: the sequential decoder below fills out_cap / gives the verdict)
    }
    if (!chunked) {
        r = inflate_serial_dev(c, c->st_in.p + front, in_len, c->st_in.p, dict_len, c->st_out.p, out_cap, &res, start_bit);
        if (r) return r;
    }
    *out_len = res.out_len; *in_bits = res.in_bits; *block_bits = res.block_bits; *block_out = res.block_out;
    if (res.out_len) { const int rc_ = d2h_payload(c, out, c->st_out.p, res.out_len); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (res.status == ZA_I_OUTFULL) return ZNGAMD_E_OVERFLOW;          // out_cap reached: call again with more room
    if (res.status == ZA_I_DATA) c->err = "invalid deflate data";
    return map_status(res.status);
} ZA_ABI_GUARD

// ---- two-pass reader for indexed members -----------------------------------------------------
// allow_tail: the chain may stop before the end of the buffer (what follows is an incomplete member, or not an indexed
// one); *covered = bytes the chain spans.
static int scan_members_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, std::vector<ZaMember> &hm, uint64_t *total_out,
                            bool allow_tail = false, uint64_t *covered = nullptr)
{
    hm.clear(); *total_out = 0;
    if (in_len < ZA_MEMBER_FIXED + 8) return ZNGAMD_E_ARG;
    const uint32_t max_c = (uint32_t)std::min<uint64_t>(in_len / (ZA_MEMBER_FIXED + 8) + 1, 1u << 26);
    HIPCHK(c, c->cands.ensure(max_c));
    uint32_t *d_n = (uint32_t *)((uint8_t *)c->d_small + 128);
    HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
    const uint64_t threads = (in_len + 15) / 16;
    { ProfScope ps(c, ZNGAMD_K_SCAN);
      hipLaunchKernelGGL(za_k_scan_members, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, c->stream, d_in, in_len, c->cands.p, max_c, d_n); }
    HIPCHK(c, hipGetLastError());
    uint32_t n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, d_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n == 0 || n > max_c) return ZNGAMD_E_ARG;
    std::vector<ZaCand> hc(n);
    HIPCHK(c, hipMemcpy(hc.data(), c->cands.p, (size_t)n * sizeof(ZaCand), hipMemcpyDeviceToHost));
    // order by offset (the kernel hands the candidates out in the order its atomics happened): no comparison sort of the whole
    // table -- it was a millisecond of every inflate step for 32 768 members -- but a counting pass over buckets of 16 KiB of
    // stream, which hold a member or two, and a sort inside the few buckets that hold more
    {
        const unsigned SH = 14;
        const size_t nbk = (size_t)(in_len >> SH) + 2;
        if (nbk <= 4 * (size_t)n + 1024) {
            std::vector<uint32_t> start(nbk + 1, 0u);
            for (const ZaCand &cd : hc) start[(size_t)(cd.off >> SH) + 1]++;
            for (size_t b = 0; b < nbk; b++) start[b + 1] += start[b];
            std::vector<ZaCand> so(n);
            std::vector<uint32_t> fill(start.begin(), start.end() - 1);
            for (const ZaCand &cd : hc) so[fill[(size_t)(cd.off >> SH)]++] = cd;
            for (size_t b = 0; b < nbk; b++)
                if (start[b + 1] - start[b] > 1)
                    std::sort(so.begin() + start[b], so.begin() + start[b + 1], [](const ZaCand &a, const ZaCand &b2) { return a.off < b2.off; });
            hc.swap(so);
        } else std::sort(hc.begin(), hc.end(), [](const ZaCand &a, const ZaCand &b) { return a.off < b.off; });
    }
    hm.reserve(n);
    // keep the chain that starts at offset 0 and tiles the stream exactly (signature hits inside
    // compressed data are skipped because nothing points at them)
    uint64_t pos = 0, outp = 0;
    size_t i = 0;
    while (pos < in_len) {
        while (i < hc.size() && hc[i].off < pos) i++;
        if (i == hc.size() || hc[i].off != pos) { if (allow_tail && !hm.empty()) break; return ZNGAMD_E_ARG; }
        ZaMember m;
        const uint32_t nchunk = (hc[i].isize + (1u << ZA_CHUNK_SHIFT) - 1u) >> ZA_CHUNK_SHIFT, hdr = ZA_MEMBER_HDR(nchunk);
        m.in_off = pos + hdr; m.in_len = hc[i].size - hdr - 8; m.out_off = outp;
        m.out_len = hc[i].isize; m.crc = 0; m.index_off = hdr - 28; m.nseg = nchunk;
        hm.push_back(m);
        pos += hc[i].size; outp += hc[i].isize;
    }
    if (pos != in_len && !allow_tail) return ZNGAMD_E_ARG;
    if (covered) *covered = pos;
    *total_out = outp;
    return ZNGAMD_OK;
}

int zngamd_gzip_scan_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, zngamd_member *d_members, uint32_t max_members,
                         uint32_t *n_members, uint64_t *total_out)
try {
    if (!c || !d_in || !d_members || !n_members || !total_out) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<ZaMember> hm;
    int r = scan_members_dev(c, (const uint8_t *)d_in, in_len, hm, total_out);
    prof_collect(c);
    if (r) return fail(c, r, "stream is not made of indexed members");
    if (hm.size() > max_members) return fail(c, ZNGAMD_BUF_ERROR, "member table too small");
    *n_members = (uint32_t)hm.size();
    HIPCHK(c, hipMemcpy(d_members, hm.data(), hm.size() * sizeof(ZaMember), hipMemcpyHostToDevice));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

static int inflate_members_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n,
                               uint8_t *d_out, uint64_t out_cap, int32_t *d_status)
{
    const uint32_t ch = std::min<uint32_t>(n, 32768);          // members per launch: 176 KiB of match queue each (5.8 GB)
    HIPCHK(c, c->matchq.ensure((size_t)ch * 64 * ZA_MATCHQ_PER_SEG));
    for (uint32_t c0 = 0; c0 < n; c0 += ch) {
        const uint32_t m = std::min(ch, n - c0);
        ProfScope ps(c, ZNGAMD_K_INFLATE);
        hipLaunchKernelGGL(za_k_inflate_members, dim3(m), dim3(64), 0, c->stream, d_in, in_len, d_members + c0, d_out, out_cap,
                           c->matchq.p, c->d_crc_slice4, c->d_x8k, d_status + c0);
    }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_gzip_inflate_members_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members,
                                    uint32_t n_members, void *d_out, uint64_t out_cap, int32_t *d_status)
try {
    if (!c || !d_in || !d_members || !d_out || !d_status) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = inflate_members_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, (uint8_t *)d_out, out_cap, d_status);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_gzip_inflate_plain_members_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members,
                                          uint32_t n_members, void *d_out, uint64_t out_cap, int32_t *d_status)
try {
    if (!c || !d_in || !d_members || !d_out || !d_status) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    if (n_members) {
        ProfScope ps(c, ZNGAMD_K_INFLATE);
        hipLaunchKernelGGL(za_k_inflate_serial_members, dim3(n_members), dim3(64), 0, c->stream, (const uint8_t *)d_in, in_len,
                           (const ZaMember *)d_members, (uint8_t *)d_out, out_cap, c->d_crc_table, c->d_x8k, d_status);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- spans of a seek-point index (za_inflate_spans.hip)
static int inflate_spans_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaSpan *d_spans, uint32_t n, const uint8_t *d_windows,
                             uint64_t windows_len, uint8_t *d_out, uint64_t out_cap, int32_t *d_status)
{
    if (n) {
        ProfScope ps(c, ZNGAMD_K_INFLATE);
        hipLaunchKernelGGL(za_k_inflate_spans, dim3(n), dim3(64), 0, c->stream, d_in, in_len, d_spans, d_windows, windows_len, d_out, out_cap,
                           c->d_crc_table, c->d_x8k, d_status);
    }
    HIPCHK(c, hipGetLastError());
    c->span_stats[0] += n;
    return ZNGAMD_OK;
}

int zngamd_inflate_spans_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_span *d_spans, uint32_t n,
                             const void *d_windows, uint64_t windows_len, void *d_out, uint64_t out_cap, int32_t *d_status)
try {
    if (!c || (n && (!d_in || !d_spans || !d_out || !d_status)) || (windows_len && !d_windows)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = inflate_spans_dev(c, (const uint8_t *)d_in, in_len, (const ZaSpan *)d_spans, n, (const uint8_t *)d_windows, windows_len,
                              (uint8_t *)d_out, out_cap, d_status);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_inflate_spans(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_span *spans, uint32_t n,
                         const uint8_t *windows, uint64_t windows_len, uint8_t *out, uint64_t out_cap, int32_t *status)
try {
    if (!c || (!in && in_len) || (n && (!spans || !status)) || (!windows && windows_len) || (!out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->sp_in.ensure(in_len + ZA_SPAN_PAD)); HIPCHK(c, c->sp_win.ensure(windows_len + 1)); HIPCHK(c, c->sp_out.ensure(out_cap + 64));
    HIPCHK(c, c->sp_tab.ensure(n + 1)); HIPCHK(c, c->sp_status.ensure(n + 1));
    if (in_len) HIPCHK(c, hipMemcpyAsync(c->sp_in.p, in, in_len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->sp_in.p + in_len, 0, ZA_SPAN_PAD, c->stream));
    if (windows_len) HIPCHK(c, hipMemcpyAsync(c->sp_win.p, windows, windows_len, hipMemcpyHostToDevice, c->stream));
    if (n) HIPCHK(c, hipMemcpyAsync(c->sp_tab.p, spans, (size_t)n * sizeof(ZaSpan), hipMemcpyHostToDevice, c->stream));
    // (the copies read pageable host memory: the stream is drained before the caller may touch it again, below)
    int r = inflate_spans_dev(c, c->sp_in.p, in_len + ZA_SPAN_PAD, c->sp_tab.p, n, c->sp_win.p, windows_len, c->sp_out.p, out_cap, c->sp_status.p);
    if (r) return r;
    if (n) HIPCHK(c, hipMemcpyAsync(status, c->sp_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (out_cap) { const int rc_ = d2h_payload(c, out, c->sp_out.p, out_cap); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (uint32_t i = 0; i < n; i++) if (status[i] == ZA_SPAN_OK) c->span_stats[1] += spans[i].out_len;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_span_stats(zngamd_ctx *c, uint64_t *out, int reset)
try {
    if (!c || !out) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    out[0] = c->span_stats[0]; out[1] = c->span_stats[1];
    if (reset) c->span_stats[0] = c->span_stats[1] = 0;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_chunk_stats(zngamd_ctx *c, uint64_t *out, int reset)
try {
    if (!c || !out) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    for (int i = 0; i < 4; i++) { out[i] = c->chunk_stats[i]; if (reset) c->chunk_stats[i] = 0; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- the batch API (za_batch.hip): many independent streams per call, one wavefront per item
// zlib_ng.decompress's wbits classes -> container and the largest window a zlib header may name (0: any)
static int batch_inflate_container(int wbits, int *kind, int *wmax)
{
    *wmax = 0;
    if (wbits == 0 || (wbits >= 8 && wbits <= 15)) { *kind = ZA_BATCH_ZLIB; *wmax = wbits; return ZNGAMD_OK; }
    if (wbits >= -15 && wbits <= -8) { *kind = ZA_BATCH_RAW; return ZNGAMD_OK; }
    if (wbits == 16 || (wbits >= 24 && wbits <= 31)) { *kind = ZA_BATCH_GZIP; return ZNGAMD_OK; }
    if (wbits == 32 || (wbits >= 40 && wbits <= 47)) { *kind = ZA_BATCH_AUTO; *wmax = wbits - 32; return ZNGAMD_OK; }
    return ZNGAMD_STREAM_ERROR;
}

// zlib_ng.compress's wbits classes (_container) -> container and window bits
static int batch_deflate_container(int wbits, int *kind, int *wb)
{
    if (wbits >= 9 && wbits <= 15) { *kind = ZA_BATCH_ZLIB; *wb = wbits; return ZNGAMD_OK; }
    if (wbits >= -15 && wbits <= -9) { *kind = ZA_BATCH_RAW; *wb = -wbits; return ZNGAMD_OK; }
    if (wbits >= 25 && wbits <= 31) { *kind = ZA_BATCH_GZIP; *wb = wbits - 16; return ZNGAMD_OK; }
    if (wbits == 8) { *kind = ZA_BATCH_ZLIB; *wb = 9; return ZNGAMD_OK; }
    if (wbits == 24) { *kind = ZA_BATCH_GZIP; *wb = 9; return ZNGAMD_OK; }
    return ZNGAMD_STREAM_ERROR;
}

// The container header the one-shot and the stream objects write (_zlib_header / _gzip_header in zlib_ng.py, zs_zlib_header in
// zng_stream.hip): zlib 2 bytes, 6 with FDICT and the DICTID behind them when `dictid` is given; gzip 10; raw none.  h: 10 bytes of
// room.  -> the header's length
static uint32_t container_header(int kind, int level, int wb, const uint32_t *dictid, uint8_t *h)
{
    const int lv = level == -1 ? 6 : level;
    if (kind == ZA_BATCH_ZLIB) {
        const uint32_t flevel = lv < 2 ? 0 : lv < 6 ? 1 : lv == 6 ? 2 : 3;
        uint32_t head = ((((uint32_t)(wb - 8) << 4) | 8u) << 8) | (flevel << 6) | (dictid ? 0x20u : 0u);
        head += 31u - head % 31u;
        h[0] = (uint8_t)(head >> 8); h[1] = (uint8_t)head;
        if (!dictid) return 2;
        for (int k = 0; k < 4; k++) h[2 + k] = (uint8_t)(*dictid >> (24 - 8 * k));
        return 6;
    }
    if (kind == ZA_BATCH_GZIP) {
        const uint8_t g[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, (uint8_t)(lv == 9 ? 2 : lv == 1 ? 4 : 0), 3};
        memcpy(h, g, 10);
        return 10;
    }
    return 0;
}

static uint32_t batch_trailer(int kind) { return kind == ZA_BATCH_ZLIB ? 4u : kind == ZA_BATCH_GZIP ? 8u : 0u; }

// One preset dictionary for a whole call (zdict): its kept tail (the last 32 KiB, as zngamd_stream_*_set_dictionary keep) in device
// memory with 64 readable bytes behind it, and its Adler-32 (the DICTID of a zlib header)
struct BatchDict { const uint8_t *d_tail = nullptr; uint32_t tl = 0, dictid = 1; };

// the dictionary's Adler-32: zngamd_adler32 takes the context's lock and its input staging, so this runs before the caller's
static int batch_dict_id(zngamd_ctx *c, const uint8_t *dict, uint32_t len, uint32_t *id)
{
    *id = 1;
    return len ? zngamd_adler32(c, 1, dict, len, id) : ZNGAMD_OK;
}

// (under the lock) the kept tail into bt_dict
static int batch_dict_upload(zngamd_ctx *c, const uint8_t *dict, uint32_t len, uint32_t dictid, BatchDict *bd)
{
    const uint32_t keep = len > ZA_WIN ? (uint32_t)ZA_WIN : len;
    HIPCHK(c, c->bt_dict.ensure(ZA_WIN + 64));
    if (keep) HIPCHK(c, hipMemcpyAsync(c->bt_dict.p, dict + (len - keep), keep, hipMemcpyHostToDevice, c->stream));
    bd->d_tail = c->bt_dict.p; bd->tl = keep; bd->dictid = dictid;
    return ZNGAMD_OK;
}

// one launch of the batch decoder (count_only: the count pass, sizes only); with a dictionary (bd), the kernel that decodes behind its tail
static int inflate_batch_launch(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaBatchItem *d_items, uint32_t n, int kind, int wmax,
                                bool count_only, uint8_t *d_out, uint64_t out_cap, ZaBatchResult *d_res, const BatchDict *bd)
{
    if (n && bd) {
        ProfScope ps(c, ZNGAMD_K_INFLATE);
        const auto kernel = count_only ? za_k_inflate_batch_dict<1> : za_k_inflate_batch_dict<0>;
        hipLaunchKernelGGL(kernel, dim3(n), dim3(64), 0, c->stream, d_in, in_len, d_items, d_out, out_cap, c->d_crc_table, c->d_x8k, kind, wmax, d_res,
                           bd->d_tail, bd->tl, bd->dictid);
    } else if (n) {
        ProfScope ps(c, ZNGAMD_K_INFLATE);
        const auto kernel = count_only ? za_k_inflate_batch<1> : za_k_inflate_batch<0>;
        hipLaunchKernelGGL(kernel, dim3(n), dim3(64), 0, c->stream, d_in, in_len, d_items, d_out, out_cap, c->d_crc_table, c->d_x8k, kind, wmax, d_res);
    }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

// The first decode's room for an item the caller left at out_cap 0: a gzip member's ISIZE (bounded by deflate's largest ratio),
// else a multiple of its compressed size.  An item that does not fit is sized exactly by the count pass.
static uint32_t batch_guess(const uint8_t *in, uint64_t in_len, const zngamd_batch_item &it, int kind)
{
    const uint64_t hi = std::min<uint64_t>(1032ull * it.in_len + 1024, 0xFFFFFFFFull);
    if (it.in_off > in_len || in_len - it.in_off < it.in_len) return 0;            // (the kernel reports the entry)
    const uint8_t *p = in + it.in_off;
    const bool gz = kind == ZA_BATCH_GZIP || (kind == ZA_BATCH_AUTO && it.in_len >= 2 && p[0] == 0x1f && p[1] == 0x8b);
    if (gz && it.in_len >= 18) {
        const uint32_t isize = (uint32_t)p[it.in_len - 4] | ((uint32_t)p[it.in_len - 3] << 8) | ((uint32_t)p[it.in_len - 2] << 16) | ((uint32_t)p[it.in_len - 1] << 24);
        return (uint32_t)std::min<uint64_t>(isize, hi);
    }
    return (uint32_t)std::min<uint64_t>(4ull * it.in_len + 1024, hi);
}

// The batch entry points without a dictionary are these with none: NULL / 0 on deflate, dict_len == 0 on inflate (an empty dictionary
// decodes like none; on deflate a non-NULL empty one writes FDICT with DICTID 1, as compressobj(zdict=b"") does).
int zngamd_inflate_batch_dict(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int wbits,
                              const uint8_t *dict, uint32_t dict_len, zngamd_alloc_fn alloc, void *user, zngamd_batch_result *results)
try {
    if (!c || (!in && in_len) || (n && (!items || !results || !alloc)) || (!dict && dict_len)) return ZNGAMD_E_ARG;
    int kind, wmax;
    if (batch_inflate_container(wbits, &kind, &wmax)) return fail(c, ZNGAMD_STREAM_ERROR, "invalid wbits");
    if (n == 0) return ZNGAMD_OK;
    uint32_t dictid;
    int r = batch_dict_id(c, dict, dict_len, &dictid);
    if (r) return r;
    std::lock_guard<std::mutex> g(c->mu);
    r = stage_in(c, in, in_len);                        // (64 zero bytes behind the input: ZA_BATCH_PAD)
    if (r) return r;
    BatchDict bdv;
    const BatchDict *bd = nullptr;
    if (dict_len) { r = batch_dict_upload(c, dict, dict_len, dictid, &bdv); if (r) return r; bd = &bdv; }
    // first decode: every item with its guessed room, back to back
    std::vector<ZaBatchItem> t1(n);
    uint64_t r1 = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t cap = items[i].out_cap ? items[i].out_cap : batch_guess(in, in_len, items[i], kind);
        t1[i].in_off = items[i].in_off; t1[i].in_len = items[i].in_len; t1[i].out_off = r1; t1[i].out_cap = cap;
        t1[i].reserved[0] = t1[i].reserved[1] = 0;
        r1 += cap;
    }
    HIPCHK(c, c->bt_items.ensure(n)); HIPCHK(c, c->bt_res.ensure(n)); HIPCHK(c, c->bt_out.ensure(r1 + 64));
    HIPCHK(c, hipMemcpyAsync(c->bt_items.p, t1.data(), (size_t)n * sizeof(ZaBatchItem), hipMemcpyHostToDevice, c->stream));
    r = inflate_batch_launch(c, c->st_in.p, in_len, c->bt_items.p, n, kind, wmax, false, c->bt_out.p, r1, c->bt_res.p, bd);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(results, c->bt_res.p, (size_t)n * sizeof(ZaBatchResult), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->up_busy = false;
    for (uint32_t i = 0; i < n; i++) { items[i].out_off = t1[i].out_off; items[i].out_cap = t1[i].out_cap; }
    // items that ran out of room: their exact size from one count pass, then one more decode with exactly that room
    std::vector<uint32_t> full;
    for (uint32_t i = 0; i < n; i++) if (results[i].status == ZA_BATCH_OUTFULL) full.push_back(i);
    uint64_t r2 = 0;
    if (!full.empty()) {
        const uint32_t m = (uint32_t)full.size();
        std::vector<ZaBatchItem> t2(m);
        std::vector<ZaBatchResult> res2(m);
        for (uint32_t k = 0; k < m; k++) { t2[k] = t1[full[k]]; t2[k].out_off = 0; t2[k].out_cap = 0; }
        HIPCHK(c, c->bt_items2.ensure(m)); HIPCHK(c, c->bt_res2.ensure(m));
        HIPCHK(c, hipMemcpyAsync(c->bt_items2.p, t2.data(), (size_t)m * sizeof(ZaBatchItem), hipMemcpyHostToDevice, c->stream));
        r = inflate_batch_launch(c, c->st_in.p, in_len, c->bt_items2.p, m, kind, wmax, true, nullptr, 0, c->bt_res2.p, bd);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(res2.data(), c->bt_res2.p, (size_t)m * sizeof(ZaBatchResult), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < m; k++) {
            t2[k].out_off = r2; t2[k].out_cap = res2[k].status == ZA_BATCH_OK ? res2[k].out_len : 0;
            r2 += t2[k].out_cap;
        }
        HIPCHK(c, c->bt_out2.ensure(r2 + 64));
        HIPCHK(c, hipMemcpyAsync(c->bt_items2.p, t2.data(), (size_t)m * sizeof(ZaBatchItem), hipMemcpyHostToDevice, c->stream));
        r = inflate_batch_launch(c, c->st_in.p, in_len, c->bt_items2.p, m, kind, wmax, false, c->bt_out2.p, r2, c->bt_res2.p, bd);
        if (r) return r;
        std::vector<ZaBatchResult> res3(m);
        HIPCHK(c, hipMemcpyAsync(res3.data(), c->bt_res2.p, (size_t)m * sizeof(ZaBatchResult), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < m; k++) {
            const uint32_t i = full[k];
            results[i] = res2[k].status == ZA_BATCH_OK ? *(const zngamd_batch_result *)&res3[k] : *(const zngamd_batch_result *)&res2[k];
            items[i].out_off = r1 + t2[k].out_off; items[i].out_cap = t2[k].out_cap;
        }
    }
    uint8_t *dst = (uint8_t *)alloc(user, r1 + r2);
    if (!dst && r1 + r2) return fail(c, ZNGAMD_MEM_ERROR, "cannot allocate the output");
    if (r1) { const int rc_ = d2h_payload(c, dst, c->bt_out.p, r1); if (rc_) return rc_; }
    if (r2) { const int rc_ = d2h_payload(c, dst + r1, c->bt_out2.p, r2); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_inflate_batch(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int wbits,
                         zngamd_alloc_fn alloc, void *user, zngamd_batch_result *results)
{
    return zngamd_inflate_batch_dict(c, in, in_len, items, n, wbits, nullptr, 0, alloc, user, results);
}

int zngamd_inflate_batch_dict_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_batch_item *d_items, uint32_t n, int wbits,
                                  const uint8_t *dict, uint32_t dict_len, int count_only, void *d_out, uint64_t out_cap, zngamd_batch_result *d_results)
try {
    if (!c || (n && (!d_in || !d_items || !d_results)) || (!d_out && out_cap) || (!dict && dict_len)) return ZNGAMD_E_ARG;
    int kind, wmax;
    if (batch_inflate_container(wbits, &kind, &wmax)) return fail(c, ZNGAMD_STREAM_ERROR, "invalid wbits");
    uint32_t dictid;
    int r = batch_dict_id(c, dict, dict_len, &dictid);
    if (r) return r;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    BatchDict bd;
    if (dict_len) { r = batch_dict_upload(c, dict, dict_len, dictid, &bd); if (r) return r; }
    r = inflate_batch_launch(c, (const uint8_t *)d_in, in_len, (const ZaBatchItem *)d_items, n, kind, wmax, count_only != 0, (uint8_t *)d_out,
                             d_out ? out_cap : 0, (ZaBatchResult *)d_results, dict_len ? &bd : nullptr);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_inflate_batch_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_batch_item *d_items, uint32_t n, int wbits,
                             int count_only, void *d_out, uint64_t out_cap, zngamd_batch_result *d_results)
{
    return zngamd_inflate_batch_dict_dev(c, d_in, in_len, d_items, n, wbits, nullptr, 0, count_only, d_out, out_cap, d_results);
}

// One deflate block per item, the packed stream into bt_def, then the framing kernel into d_out.  items: host table (in_off, in_len
// read; out_off written).
//   bd == nullptr: every item is zlib_ng.compress's stream -- its block is the one zngamd_deflate_stream cuts for a one-shot call
//     (FINAL; units of 16 KiB up to 128 KiB) and lies where the item does in d_in; the whole call is one range.
//   bd: every item is the stream compressobj(level, DEFLATED, wbits, strategy=..., zdict=...) writes for it.  za_k_batch_prime writes
//     [tail][item] per item into bt_prime (records on 64-byte boundaries, as the stream's staged buffer), the block is the one
//     zs_deflate_pending runs -- FINAL, 128 KiB units, dict_len = the tail -- and the frame carries the FDICT header and the Adler-32
//     of the item's own bytes.  Every item carries up to 32 KiB of history, so the staging and the deflate workspace grow with
//     (tail + item): the items run in ranges whose records stay under ZA_BATCH_PRIME_BUDGET.
#define ZA_BATCH_PRIME_BUDGET (256ull << 20)
static int deflate_batch_locked(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                                int strategy, const BatchDict *bd, uint8_t *d_out, uint64_t out_cap, ZaBatchResult *d_res, uint64_t *total)
{
    *total = 0;
    int kind, wb;
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (batch_deflate_container(wbits, &kind, &wb)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (bd && kind == ZA_BATCH_GZIP) return fail(c, ZNGAMD_STREAM_ERROR, "Invalid dictionary");
    if (strategy < ZNGAMD_STRATEGY_DEFAULT || strategy > ZNGAMD_STRATEGY_FIXED) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression strategy");
    if (n == 0) return ZNGAMD_OK;
    if (bd)         // (build_units sees the primed records, not the items)
        for (uint32_t i = 0; i < n; i++)
            if (items[i].in_off > in_len || in_len - items[i].in_off < items[i].in_len) return fail(c, ZNGAMD_E_ARG, "block outside the input buffer");
    HIPCHK(c, hipSetDevice(c->device));
    ZaBatchFrameHdr head = {};
    const uint32_t hl = container_header(kind, level, wb, bd ? &bd->dictid : nullptr, head.b), ovh = hl + batch_trailer(kind);
    const uint32_t tl = bd ? bd->tl : 0;
    const uint32_t flags = ZNGAMD_FLAG_FINAL | ZNGAMD_FLAG_STRATEGY(strategy) | (bd ? ZNGAMD_FLAG_WBITS(wb) : 0u);
    std::vector<ZaBatchItem> pt(bd ? n : 0);        // the prime kernel's table: where each record lies in bt_prime
    uint64_t base = 0;
    bool fits = true;
    for (uint32_t a = 0; a < n;) {
        // the range [a, b) and the buffer its blocks lie in
        uint32_t b = n;
        const uint8_t *src = d_in;
        uint64_t src_len = in_len;
        if (bd) {
            // records of (tail + item) rounded up to 64 bytes, under the budget (a larger item goes alone)
            src_len = 0;
            for (b = a; b < n; b++) {
                const uint64_t rl = ((uint64_t)tl + items[b].in_len + 63) & ~63ull;
                if (b > a && src_len + rl > ZA_BATCH_PRIME_BUDGET) break;
                pt[b].in_off = items[b].in_off; pt[b].in_len = items[b].in_len; pt[b].out_off = src_len; pt[b].out_cap = 0;
                pt[b].reserved[0] = pt[b].reserved[1] = 0;
                src_len += rl;
            }
            HIPCHK(c, c->bt_prime.ensure(src_len + 64)); HIPCHK(c, c->bt_items2.ensure(b - a));
            HIPCHK(c, hipMemcpyAsync(c->bt_items2.p, pt.data() + a, (size_t)(b - a) * sizeof(ZaBatchItem), hipMemcpyHostToDevice, c->stream));
            {
                ProfScope ps(c, ZNGAMD_K_GATHER);
                hipLaunchKernelGGL(za_k_batch_prime, dim3(b - a), dim3(64), 0, c->stream, d_in, in_len, c->bt_items2.p, b - a, bd->d_tail, tl, c->bt_prime.p,
                                   src_len + 64);
            }
            HIPCHK(c, hipGetLastError());
            src = c->bt_prime.p;
        }
        const uint32_t m = b - a;
        std::vector<zngamd_block> blocks(m);
        for (uint32_t k = 0; k < m; k++) {
            zngamd_block &B = blocks[k];
            B.off = bd ? pt[a + k].out_off + tl : items[a + k].in_off; B.len = items[a + k].in_len; B.dict_len = tl; B.reserved = 0;
            // (the one-shot's 16 KiB units without a dictionary, the stream's 128 KiB ones with it: each is what byte identity needs)
            B.flags = flags | (!bd && B.len <= ZA_MAX_UNIT ? ZNGAMD_FLAG_UNITS16K : 0u);
        }
        std::vector<ZaUnit> hu;
        int r = build_units(c, blocks.data(), m, src_len, hu);
        if (r) return r;
        const uint32_t nu = (uint32_t)hu.size();
        std::vector<uint32_t> first(m + 1, nu);
        for (uint32_t u = nu; u-- > 0;) first[hu[u].block] = u;
        uint64_t bound = 64;
        for (const ZaUnit &u : hu) bound += unit_bound(u.in_len, strategy);
        HIPCHK(c, c->bt_def.ensure(bound)); HIPCHK(c, c->bt_uoff.ensure(nu)); HIPCHK(c, c->bt_ulen.ensure(nu)); HIPCHK(c, c->bt_ucrc.ensure(nu));
        HIPCHK(c, c->bt_total.ensure(1)); HIPCHK(c, c->bt_first.ensure(m + 1)); HIPCHK(c, c->bt_items.ensure(n));
        HIPCHK(c, hipMemcpyAsync(c->bt_first.p, first.data(), (size_t)(m + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (a == 0)     // the frame's table (the items' own bytes), for every range at once
            HIPCHK(c, hipMemcpyAsync(c->bt_items.p, items, (size_t)n * sizeof(ZaBatchItem), hipMemcpyHostToDevice, c->stream));
        PackedDst pd; pd.d_dst = c->bt_def.p; pd.cap = bound; pd.d_unit_off = c->bt_uoff.p; pd.d_total = c->bt_total.p;
        r = deflate_units_dev(c, src, src_len, hu, level, nullptr, c->bt_ulen.p, c->bt_ucrc.p, 1 << wb, &pd, strategy);
        if (r) return r;
        uint64_t def_total = 0;
        std::vector<uint32_t> st(nu);
        HIPCHK(c, hipMemcpyAsync(&def_total, c->bt_total.p, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, (size_t)nu * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->up_busy = false;
        for (uint32_t v : st) if (v) return fail(c, ZNGAMD_E_HIP, "packed deflate: a unit's size differs from its plan");
        if (def_total > bound) return fail(c, ZNGAMD_E_HIP, "packed deflate: stream larger than its bound");
        const uint64_t need = def_total + (uint64_t)m * ovh;
        fits = fits && base + need <= out_cap;
        if (fits) {
            {
                ProfScope ps(c, ZNGAMD_K_GATHER);
                hipLaunchKernelGGL(za_k_batch_frame, dim3(m), dim3(64), 0, c->stream, d_in, c->bt_items.p + a, m, c->bt_first.p, nu, c->bt_uoff.p, c->bt_ucrc.p,
                                   c->bt_total.p, c->bt_def.p, kind, head, hl, d_out + base, out_cap - base, d_res + a);
            }
            HIPCHK(c, hipGetLastError());
            std::vector<ZaBatchItem> back(m);
            HIPCHK(c, hipMemcpyAsync(back.data(), c->bt_items.p + a, (size_t)m * sizeof(ZaBatchItem), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            for (uint32_t k = 0; k < m; k++) items[a + k].out_off = base + back[k].out_off;
        }
        base += need;
        a = b;
    }
    *total = base;
    if (!fits) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    return ZNGAMD_OK;
}

int zngamd_deflate_batch_dict_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                                  int strategy, const uint8_t *dict, uint32_t dict_len, void *d_out, uint64_t out_cap,
                                  zngamd_batch_result *d_results, uint64_t *total)
try {
    if (!c || !total || (n && (!d_in || !items || !d_out || !d_results)) || (!dict && dict_len)) return ZNGAMD_E_ARG;
    *total = 0;
    int kind, wb;
    if (dict && batch_deflate_container(wbits, &kind, &wb) == ZNGAMD_OK && kind == ZA_BATCH_GZIP) return fail(c, ZNGAMD_STREAM_ERROR, "Invalid dictionary");
    uint32_t dictid;
    int r = batch_dict_id(c, dict, dict_len, &dictid);
    if (r) return r;
    std::lock_guard<std::mutex> g(c->mu);
    BatchDict bd;
    if (dict) {
        HIPCHK(c, hipSetDevice(c->device));
        r = batch_dict_upload(c, dict, dict_len, dictid, &bd);
        if (r) return r;
    }
    r = deflate_batch_locked(c, (const uint8_t *)d_in, in_len, items, n, level, wbits, strategy, dict ? &bd : nullptr, (uint8_t *)d_out, out_cap,
                             (ZaBatchResult *)d_results, total);
    if (r) return r;
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_deflate_batch_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                             int strategy, void *d_out, uint64_t out_cap, zngamd_batch_result *d_results, uint64_t *total)
{
    return zngamd_deflate_batch_dict_dev(c, d_in, in_len, items, n, level, wbits, strategy, nullptr, 0, d_out, out_cap, d_results, total);
}

int zngamd_deflate_batch_dict(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                              int strategy, const uint8_t *dict, uint32_t dict_len, zngamd_alloc_fn alloc, void *user,
                              zngamd_batch_result *results, uint64_t *total)
try {
    if (!c || (!in && in_len) || !total || (n && (!items || !results || !alloc)) || (!dict && dict_len)) return ZNGAMD_E_ARG;
    *total = 0;
    int kind, wb;
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (batch_deflate_container(wbits, &kind, &wb)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    if (dict && kind == ZA_BATCH_GZIP) return fail(c, ZNGAMD_STREAM_ERROR, "Invalid dictionary");
    if (n == 0) return ZNGAMD_OK;
    uint32_t dictid;
    int r = batch_dict_id(c, dict, dict_len, &dictid);
    if (r) return r;
    std::lock_guard<std::mutex> g(c->mu);
    r = stage_in(c, in, in_len);
    if (r) return r;
    BatchDict bd;
    if (dict) { r = batch_dict_upload(c, dict, dict_len, dictid, &bd); if (r) return r; }
    // the output's bound: every item's framing (18 bytes at most, gzip's) and the bound of each unit it is cut into (unit_bound:
    // under Z_FIXED a unit can be an eighth larger than its bytes) -- units of 16 KiB up to 128 KiB, of 128 KiB beyond; with a
    // dictionary every item goes in units of 128 KiB, which need no more than the smaller ones are given here
    uint64_t cap = 64 + (uint64_t)n * 18;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t U = items[i].in_len <= ZA_MAX_UNIT ? ZA_SMALL_UNIT : (uint32_t)ZA_MAX_UNIT;
        const uint32_t full = items[i].in_len / U, rest = items[i].in_len - full * U;
        cap += full * unit_bound(U, strategy) + (rest || !full ? unit_bound(rest, strategy) : 0u);
    }
    HIPCHK(c, c->bt_out.ensure(cap)); HIPCHK(c, c->bt_res.ensure(n));
    r = deflate_batch_locked(c, c->st_in.p, in_len, items, n, level, wbits, strategy, dict ? &bd : nullptr, c->bt_out.p, cap, c->bt_res.p, total);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(results, c->bt_res.p, (size_t)n * sizeof(ZaBatchResult), hipMemcpyDeviceToHost, c->stream));
    uint8_t *dst = (uint8_t *)alloc(user, *total);
    if (!dst && *total) { (void)hipStreamSynchronize(c->stream); return fail(c, ZNGAMD_MEM_ERROR, "cannot allocate the output"); }
    if (*total) { const int rc_ = d2h_payload(c, dst, c->bt_out.p, *total); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_deflate_batch(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                         int strategy, zngamd_alloc_fn alloc, void *user, zngamd_batch_result *results, uint64_t *total)
{
    return zngamd_deflate_batch_dict(c, in, in_len, items, n, level, wbits, strategy, nullptr, 0, alloc, user, results, total);
}

// ---- the batch API's dictionary trainer (za_dict.hip)
static bool train_args_ok(uint32_t n, uint32_t dict_size, uint32_t k, uint32_t d)
{
    return n && d >= 4 && d <= 8 && k >= d && k <= 16384 && dict_size >= d && dict_size <= ZA_WIN;
}

// items: a HOST copy of the table.  Every entry must lie inside [0, in_len) and the samples must add up to [k, 4 GiB); out_off
// becomes each one's place in the joined samples, *total their sum.
static int train_table(zngamd_ctx *c, std::vector<ZaBatchItem> &items, uint64_t in_len, uint32_t k, uint64_t *total)
{
    uint64_t t = 0;
    for (auto &it : items) {
        if (it.in_off > in_len || in_len - it.in_off < it.in_len) return fail(c, ZNGAMD_E_ARG, "a sample lies outside the input buffer");
        it.out_off = t;
        t += it.in_len;
    }
    if (t < k || t >= (1ull << 32)) return fail(c, ZNGAMD_E_ARG, "the samples must hold at least k and less than 4 GiB bytes");
    *total = t;
    return ZNGAMD_OK;
}

// (under the lock) d_in: device, ZNGAMD_BATCH_PAD readable bytes behind in_len; items: the checked table (train_table)
static int train_dict_locked(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const std::vector<ZaBatchItem> &items, uint64_t total,
                             uint32_t dict_size, uint32_t k, uint32_t d, uint8_t *dict, uint32_t *dict_len)
{
    const uint32_t n_items = (uint32_t)items.size(), n = (uint32_t)(total - d + 1), K = k - d + 1;
    uint32_t E = std::max(1u, dict_size / k / 4), S = n / E;                     // the epochs (step 4)
    if (S < 10u * k) { E = std::max(1u, n / (10u * k)); S = n / E; }
    if (S < K) return ZNGAMD_OK;
    const uint32_t ntiles = (S - K + 1 + ZA_DICT_TILE - 1) / ZA_DICT_TILE;
    HIPCHK(c, c->dt_items.ensure(n_items)); HIPCHK(c, c->dt_data.ensure(total + 64)); HIPCHK(c, c->dt_hash.ensure(n));
    HIPCHK(c, c->dt_shadow.ensure(n)); HIPCHK(c, c->dt_freq.ensure(1u << ZA_DICT_HASH_BITS)); HIPCHK(c, c->dt_best.ensure(ntiles));
    HIPCHK(c, c->dt_state.ensure(1)); HIPCHK(c, c->dt_dict.ensure(dict_size));
    HIPCHK(c, hipMemcpyAsync(c->dt_items.p, items.data(), (size_t)n_items * sizeof(ZaBatchItem), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dt_data.p + total, 0, 64, c->stream));
    HIPCHK(c, hipMemsetAsync(c->dt_freq.p, 0, sizeof(uint32_t) << ZA_DICT_HASH_BITS, c->stream));
    ZaDictState hs = {dict_size, 0, 0, 0, 0, {0, 0, 0}};
    HIPCHK(c, hipMemcpyAsync(c->dt_state.p, &hs, sizeof hs, hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, ZNGAMD_K_OTHER);
        const uint32_t hb = (uint32_t)(((uint64_t)n + 4095) / 4096), lim = E * S;
        hipLaunchKernelGGL(za_k_dict_gather, dim3(n_items), dim3(64), 0, c->stream, d_in, in_len, c->dt_items.p, n_items, c->dt_data.p, total);
        hipLaunchKernelGGL(za_k_dict_hash, dim3(hb), dim3(256), 0, c->stream, c->dt_data.p, n, d, c->dt_hash.p);
        hipLaunchKernelGGL(za_k_dict_mark, dim3((n_items + 255) / 256), dim3(256), 0, c->stream, c->dt_items.p, n_items, n, d, c->dt_hash.p);
        hipLaunchKernelGGL(za_k_dict_count, dim3(hb), dim3(256), 0, c->stream, c->dt_hash.p, n, c->dt_freq.p);
        const bool lds = K - 1 + ZA_DICT_SH_TILE <= ZA_DICT_SH_LDS;
        hipLaunchKernelGGL(lds ? za_k_dict_shadow<true> : za_k_dict_shadow<false>, dim3((lim + ZA_DICT_SH_TILE - 1) / ZA_DICT_SH_TILE), dim3(256),
                           lds ? (K - 1 + ZA_DICT_SH_TILE) * sizeof(uint32_t) : 0, c->stream, c->dt_hash.p, lim, S, K, c->dt_shadow.p);
        HIPCHK(c, hipGetLastError());
    }
    // the pick loop (step 6) in groups of launches; a pick after the last returns at once.  Every pick but the last shortens the tail
    // by at least d bytes or is one of at most E - 1 zero picks in a row: the loop ends within (dict_size / d + 1) E picks.
    const uint64_t bound = ((uint64_t)dict_size / d + 1) * E;
    uint64_t launched = 0;
    for (uint32_t group = 32;; group = std::min(group * 2, 512u)) {
        ProfScope ps(c, ZNGAMD_K_OTHER);
        for (uint32_t g = 0; g < group; g++) {
            hipLaunchKernelGGL(za_k_dict_score, dim3(ntiles), dim3(256), 0, c->stream, c->dt_hash.p, c->dt_shadow.p, c->dt_freq.p, S, K,
                               c->dt_state.p, c->dt_best.p);
            hipLaunchKernelGGL(za_k_dict_pick, dim3(1), dim3(256), 0, c->stream, c->dt_data.p, c->dt_hash.p, c->dt_freq.p, c->dt_best.p,
                               ntiles, S, K, E, d, c->dt_state.p, c->dt_dict.p);
        }
        HIPCHK(c, hipGetLastError());
        launched += group;
        HIPCHK(c, hipMemcpyAsync(&hs, c->dt_state.p, sizeof hs, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (hs.done) break;
        if (launched > bound) return fail(c, ZNGAMD_E_HIP, "the dictionary trainer's pick loop did not end");
    }
    if (hs.tail > dict_size) return fail(c, ZNGAMD_E_HIP, "the dictionary trainer's state is corrupt");
    if (trace_on()) fprintf(stderr, "[zngamd] train_dict: %u positions, %u epochs of %u, %u picks, %u bytes\n", n, E, S, hs.picks, dict_size - hs.tail);
    if (hs.tail < dict_size) HIPCHK(c, hipMemcpyAsync(dict, c->dt_dict.p + hs.tail, dict_size - hs.tail, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *dict_len = dict_size - hs.tail;
    return ZNGAMD_OK;
}

int zngamd_train_dict_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_batch_item *d_items, uint32_t n, uint32_t dict_size,
                          uint32_t k, uint32_t d, uint8_t *dict, uint32_t *dict_len)
try {
    if (!c || !d_in || !d_items || !dict || !dict_len || !train_args_ok(n, dict_size, k, d)) return ZNGAMD_E_ARG;
    *dict_len = 0;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<ZaBatchItem> items(n);
    HIPCHK(c, hipMemcpyAsync(items.data(), d_items, (size_t)n * sizeof(ZaBatchItem), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t total;
    int r = train_table(c, items, in_len, k, &total);
    if (r) return r;
    r = train_dict_locked(c, (const uint8_t *)d_in, in_len, items, total, dict_size, k, d, dict, dict_len);
    if (r) return r;
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_train_dict(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_batch_item *items, uint32_t n, uint32_t dict_size,
                      uint32_t k, uint32_t d, uint8_t *dict, uint32_t *dict_len)
try {
    if (!c || !in || !items || !dict || !dict_len || !train_args_ok(n, dict_size, k, d)) return ZNGAMD_E_ARG;
    *dict_len = 0;
    std::vector<ZaBatchItem> tab(n);
    memcpy(tab.data(), items, (size_t)n * sizeof(ZaBatchItem));
    uint64_t total;
    int r = train_table(c, tab, in_len, k, &total);
    if (r) return r;
    std::lock_guard<std::mutex> g(c->mu);
    r = stage_in(c, in, in_len);
    if (r) return r;
    r = train_dict_locked(c, c->st_in.p, in_len, tab, total, dict_size, k, d, dict, dict_len);
    if (r) return r;
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_inflate_raw_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, void *d_out, uint64_t out_cap, uint64_t *out_len,
                           uint64_t *in_used)
try {
    if (!c || !d_in || !d_out || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t clen = 0, cused = 0;
    const int cr = inflate_chunked_dev(c, (const uint8_t *)d_in, in_len, (uint8_t *)d_out, out_cap, &clen, &cused);
    if (cr < 0 && cr != ZNGAMD_BUF_ERROR) return cr;
    if (cr == ZNGAMD_BUF_ERROR) { *out_len = clen; if (in_used) *in_used = 0; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
    if (cr == 0) { *out_len = clen; if (in_used) *in_used = cused; c->paths[ZNGAMD_PATH_CHUNKED]++; return ZNGAMD_STREAM_END; }
    ZaInfResult res;
    int r = inflate_serial_dev(c, (const uint8_t *)d_in, in_len, nullptr, 0, (uint8_t *)d_out, out_cap, &res);
    if (r) return r;
    c->paths[ZNGAMD_PATH_SEQUENTIAL]++;
    *out_len = res.out_len;
    if (in_used) *in_used = (res.in_bits + 7) >> 3;
    if (res.status == ZA_I_DATA) c->err = "invalid deflate data";
    return map_status(res.status);
} ZA_ABI_GUARD

// ---- the default writer's stream with the writer's index (za_inflate_units.hip)
int zngamd_deflate_index_dev(zngamd_ctx *c, uint32_t *d_index, uint32_t n_units)
try {
    if (!c || !d_index) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (n_units == 0) return ZNGAMD_OK;
    if (n_units != c->last_units || !c->cidx.p) return fail(c, ZNGAMD_E_ARG, "the index is that of the context's last deflate call: its unit count differs");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(d_index, c->cidx.p, (size_t)n_units * ZA_CIDX_STRIDE * 4, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

static_assert(ZNGAMD_INDEX_STRIDE == ZA_CIDX_STRIDE, "index stride");
// (the caller holds the context's lock; device pointers, host size arrays; leaves the stream drained)
static int inflate_units_core(zngamd_ctx *c, const uint8_t *d_def, uint64_t def_len, const uint32_t *unit_in_len, const uint32_t *unit_out_len,
                              uint32_t n_units, const uint32_t *d_index, const void *d_dict, uint32_t dict_len,
                              uint8_t *d_out, uint64_t out_cap, uint64_t *out_len)
{
    *out_len = 0;
    uint64_t tin = 0, tout = 0;
    for (uint32_t u = 0; u < n_units; u++) {
        if (unit_out_len[u] > ZA_MAX_UNIT) return fail(c, ZNGAMD_E_ARG, "a unit is larger than 128 KiB");
        tin += unit_in_len[u]; tout += unit_out_len[u];
    }
    if (tin > def_len) return fail(c, ZNGAMD_E_ARG, "the units' bytes exceed the stream");
    *out_len = tout;
    if (tout > out_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    constexpr uint64_t AREA = (uint64_t)ZA_WIN + ZA_MAX_UNIT;                 // symbols of a unit's area: markers, then the unit
    static const uint32_t batch = [] { const char *e = getenv("ZNGAMD_UNIT_BATCH"); long v = e ? atol(e) : 16384; return (uint32_t)(v < 64 ? 64 : v > 65536 ? 65536 : v); }();
    uint64_t in_at = 0, out_at = 0;
    std::vector<ZaMember> hm, he; std::vector<ZaChunk> chain; std::vector<ZaChunkRes> res; std::vector<uint32_t> uidx;
    for (uint32_t u0 = 0; u0 < n_units; u0 += batch) {
        const uint32_t u1 = std::min(n_units, u0 + batch);
        // (the window kernels take the bytes in front of a batch from the output: a batch behind fewer than 32 768 of them -- blocks
        // of a few hundred bytes -- is left to the decoder that needs no index)
        if (out_at && out_at < (uint64_t)ZA_WIN) return fail(c, ZNGAMD_E_INDEX, "a batch of units shorter than the window: decode it without the index");
        hm.clear(); he.clear(); chain.clear(); uidx.clear();
        uint64_t acc = 0;                                                     // output of this batch so far
        for (uint32_t u = u0; u < u1; u++) {
            if (unit_out_len[u] != 0) {
                ZaMember m;
                m.in_off = in_at; m.in_len = unit_in_len[u]; m.out_off = (uint64_t)hm.size() * AREA; m.out_len = unit_out_len[u];
                m.crc = (uint32_t)std::min<uint64_t>(ZA_WIN, out_at + acc + dict_len);       // (history in front of the unit)
                m.index_off = 0; m.nseg = (unit_out_len[u] + ZA_SEG - 1) >> ZA_SEG_SHIFT;
                ZaChunk ch; ch.in_bit = in_at * 8ull; ch.out_off = acc; ch.out_len = unit_out_len[u]; ch.end_bit = (in_at + unit_in_len[u]) * 8ull;
                ch.src_off = m.out_off + ZA_WIN;
                hm.push_back(m); chain.push_back(ch); uidx.push_back(u);
                acc += unit_out_len[u];
            } else {
                // a unit the index calls empty decodes to nothing, but its bytes must BE an empty unit: the kernel looks at them
                ZaMember m;
                m.in_off = in_at; m.in_len = unit_in_len[u]; m.out_off = 0; m.out_len = 0; m.crc = 0; m.index_off = 0; m.nseg = 0;
                he.push_back(m);
            }
            in_at += unit_in_len[u];
        }
        const uint32_t m = (uint32_t)hm.size(), ne = (uint32_t)he.size();      // units with output (areas, rows, windows); then the empty ones
        hm.insert(hm.end(), he.begin(), he.end());
        // the units' index rows are picked by unit number: the kernel reads row blockIdx.x, so a batch without empty units passes
        // its first row; one with empty units has its rows gathered
        const uint32_t *d_rows = d_index + (size_t)u0 * ZA_CIDX_STRIDE;
        if (m != u1 - u0) {
            HIPCHK(c, c->st_len.ensure((size_t)m * ZA_CIDX_STRIDE));
            for (uint32_t k = 0; k < m; k++)
                HIPCHK(c, hipMemcpyAsync(c->st_len.p + (size_t)k * ZA_CIDX_STRIDE, d_index + (size_t)uidx[k] * ZA_CIDX_STRIDE, ZA_CIDX_STRIDE * 4, hipMemcpyDeviceToDevice, c->stream));
            d_rows = c->st_len.p;
        }
        {
            // (grown with a quarter of head-room: the windows of a reader hold a few units more or fewer each time, and every
            // reallocation loses the areas' markers)
            const size_t want = (size_t)std::min<uint32_t>(batch, n_units) * AREA + 64, cap0 = c->uarea.cap;
            const uint16_t *p0 = c->uarea.p;
            if (want > cap0) HIPCHK(c, c->uarea.ensure(std::min<size_t>((size_t)batch * AREA + 64, want + want / 4)));
            if (c->uarea.cap != cap0 || c->uarea.p != p0) c->uarea_marked = 0;
        }
        if (c->uarea.cap < (size_t)m * AREA + 64) return fail(c, ZNGAMD_E_HIP, "unit areas");
        HIPCHK(c, c->members.ensure(m + ne)); HIPCHK(c, c->cres.ensure(m + ne)); HIPCHK(c, c->cchunks.ensure(m));
        HIPCHK(c, c->matchq.ensure((size_t)m * 64 * ZA_MATCHQ_PER_SEG));
        const uint32_t groups = (m + ZA_CHUNK_GROUP - 1) / ZA_CHUNK_GROUP;
        HIPCHK(c, c->winbuf.ensure((size_t)groups * ZA_WIN)); HIPCHK(c, c->ccomp.ensure((size_t)m * ZA_WIN));
        HIPCHK(c, hipMemcpyAsync(c->members.p, hm.data(), (size_t)(m + ne) * sizeof(ZaMember), hipMemcpyHostToDevice, c->stream));
        if (m) HIPCHK(c, hipMemcpyAsync(c->cchunks.p, chain.data(), (size_t)m * sizeof(ZaChunk), hipMemcpyHostToDevice, c->stream));
        { ProfScope ps(c, ZNGAMD_K_INFLATE);
          if (c->uarea_marked < m) {
              hipLaunchKernelGGL(za_k_fill_marker_prefix, dim3(m - c->uarea_marked), dim3(256), 0, c->stream, c->uarea.p + (uint64_t)c->uarea_marked * AREA, AREA);
              c->uarea_marked = m;
          }
          hipLaunchKernelGGL(za_k_inflate_units_marked, dim3(m + ne), dim3(64), 0, c->stream, d_def, def_len, c->members.p, c->uarea.p, (uint64_t)c->uarea.cap,
                             c->matchq.p, d_rows, c->cres.p); }
        HIPCHK(c, hipGetLastError());
        res.resize(m + ne);
        HIPCHK(c, hipMemcpyAsync(res.data(), c->cres.p, (size_t)(m + ne) * sizeof(ZaChunkRes), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < m + ne; k++) {
            if (res[k].status == ZA_I_DATA) return fail(c, ZNGAMD_DATA_ERROR, "invalid deflate data");
            if ((res[k].status != ZA_I_SYNC && res[k].status != ZA_I_END) || res[k].out_len != hm[k].out_len)
                return fail(c, ZNGAMD_E_INDEX, "the index does not fit the stream (or the stream is not this engine's indexed form): decode it without the index");
        }
        c->indexed_units += m;                  // (counted once the index has held for them: a refused batch decodes nothing)
        if (m == 0) continue;                   // only empty units: nothing for the windows
        // windows in front of the units, then markers -> bytes (the chunk pipeline's kernels: a unit is a chunk)
        const uint8_t *bd = out_at ? d_out + out_at - std::min<uint64_t>(ZA_WIN, out_at) : (const uint8_t *)d_dict;
        const uint32_t bdl = out_at ? (uint32_t)std::min<uint64_t>(ZA_WIN, out_at) : dict_len;
        { ProfScope ps(c, ZNGAMD_K_INFLATE);
          hipLaunchKernelGGL(za_k_chunk_compose, dim3(groups), dim3(1024), 0, c->stream, c->uarea.p, c->cchunks.p, m, c->ccomp.p);
          hipLaunchKernelGGL(za_k_chunk_chain, dim3(1), dim3(1024), 0, c->stream, c->ccomp.p, m, c->winbuf.p, bd, bdl);
          hipLaunchKernelGGL(za_k_chunk_resolve, dim3(m), dim3(ZA_RESOLVE_THREADS), 0, c->stream, c->uarea.p, c->cchunks.p, c->ccomp.p, c->winbuf.p, d_out + out_at); }
        HIPCHK(c, hipGetLastError());
        out_at += acc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_STREAM_END;
}

int zngamd_inflate_units_indexed_dev(zngamd_ctx *c, const void *d_def, uint64_t def_len, const uint32_t *unit_in_len, const uint32_t *unit_out_len,
                                     uint32_t n_units, const uint32_t *d_index, const void *d_dict, uint32_t dict_len,
                                     void *d_out, uint64_t out_cap, uint64_t *out_len)
try {
    if (!c || !d_def || !unit_in_len || !unit_out_len || !d_index || !d_out || !out_len || dict_len > ZA_WIN) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    const int r = inflate_units_core(c, (const uint8_t *)d_def, def_len, unit_in_len, unit_out_len, n_units, d_index, d_dict, dict_len, (uint8_t *)d_out, out_cap, out_len);
    if (r == ZNGAMD_STREAM_END) c->paths[ZNGAMD_PATH_CHUNKED]++;
    return r;
} ZA_ABI_GUARD

// ---- the index of a FILE's data member: what the writer leaves in the trailing empty members, parsed by the caller and handed to
// the windowed reader through zngamd_gz_state.index
struct ZaFileIndex {
    uint32_t n = 0; int device = 0;
    std::vector<uint32_t> in_len, out_len;
    std::vector<uint64_t> cum_in, cum_out;       // bytes in front of unit k (n + 1 entries)
    uint32_t *d_rows = nullptr;
    bool dead = false;                           // it did not fit the stream once: never tried again
};
int zngamd_index_create(zngamd_ctx *c, uint32_t n_units, const uint32_t *unit_in_len, const uint32_t *unit_out_len, const uint32_t *rows, void **handle)
try {
    if (!c || !handle || (n_units && (!unit_in_len || !unit_out_len || !rows))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    ZaFileIndex *ix = new ZaFileIndex();
    ix->n = n_units; ix->device = c->device;
    ix->in_len.assign(unit_in_len, unit_in_len + n_units); ix->out_len.assign(unit_out_len, unit_out_len + n_units);
    ix->cum_in.resize((size_t)n_units + 1); ix->cum_out.resize((size_t)n_units + 1);
    ix->cum_in[0] = ix->cum_out[0] = 0;
    for (uint32_t u = 0; u < n_units; u++) {
        if (unit_out_len[u] > ZA_MAX_UNIT) { delete ix; return fail(c, ZNGAMD_E_ARG, "a unit is larger than 128 KiB"); }
        ix->cum_in[u + 1] = ix->cum_in[u] + unit_in_len[u]; ix->cum_out[u + 1] = ix->cum_out[u] + unit_out_len[u];
    }
    if (n_units) {
        if (hipMalloc((void **)&ix->d_rows, (size_t)n_units * ZA_CIDX_STRIDE * 4) != hipSuccess) { delete ix; return fail(c, ZNGAMD_MEM_ERROR, "index rows"); }
        if (hipMemcpy(ix->d_rows, rows, (size_t)n_units * ZA_CIDX_STRIDE * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(ix->d_rows); delete ix; return fail(c, ZNGAMD_E_HIP, "index rows"); }
    }
    *handle = ix;
    return ZNGAMD_OK;
} ZA_ABI_GUARD
void zngamd_index_destroy(void *handle)
{
    ZaFileIndex *ix = (ZaFileIndex *)handle;
    if (!ix) return;
    if (ix->d_rows) { (void)hipSetDevice(ix->device); (void)hipFree(ix->d_rows); }
    delete ix;
}
// the index of the context's last deflate call on the HOST, with the units' sizes (what a writer keeps for its file's trailing members)
static int deflate_index_locked(zngamd_ctx *c, uint32_t n_units, uint32_t *unit_in_len, uint32_t *unit_out_len, uint32_t *rows)
{
    if (n_units == 0) return ZNGAMD_OK;
    const bool on_host = c->last_ulen_on_host && c->last_ulen_host.size() == n_units;
    if (n_units != c->last_units || !c->cidx.p || (!on_host && !c->last_unit_len) || c->last_hu.size() != n_units) return fail(c, ZNGAMD_E_ARG, "the index is that of the context's last deflate call: its unit count differs");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(rows, c->cidx.p, (size_t)n_units * ZA_CIDX_STRIDE * 4, hipMemcpyDeviceToHost, c->stream));
    if (on_host) memcpy(unit_in_len, c->last_ulen_host.data(), (size_t)n_units * 4);
    else HIPCHK(c, hipMemcpyAsync(unit_in_len, c->last_unit_len, (size_t)n_units * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t u = 0; u < n_units; u++) unit_out_len[u] = c->last_hu[u].in_len;
    return ZNGAMD_OK;
}

int zngamd_deflate_index(zngamd_ctx *c, uint32_t n_units, uint32_t *unit_in_len, uint32_t *unit_out_len, uint32_t *rows)
try {
    if (!c || !unit_in_len || !unit_out_len || !rows) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    return deflate_index_locked(c, n_units, unit_in_len, unit_out_len, rows);
} ZA_ABI_GUARD

int zngamd_crc32_fold_dev(zngamd_ctx *c, const uint32_t *d_crcs, uint32_t n, uint64_t each_len, uint64_t last_len, uint32_t *crc)
try {
    if (!c || (!d_crcs && n) || !crc) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<uint32_t> v(n);
    if (n) HIPCHK(c, hipMemcpyAsync(v.data(), d_crcs, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // x^(8 each_len) once; then Horner: crc = crc * x^(8 len_i) ^ crc_i
    uint32_t xe = 0x80000000u, sq = 0x00800000u;
    for (uint64_t k = each_len; k; k >>= 1) { if (k & 1) xe = za_multmodp(sq, xe); sq = za_multmodp(sq, sq); }
    uint32_t r = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (i == 0) r = v[0];
        else if (i + 1 < n || last_len == each_len) r = za_multmodp(xe, r) ^ v[i];
        else r = zngamd_crc32_combine(r, v[i], last_len);
    }
    *crc = r;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_compare_dev(zngamd_ctx *c, const void *d_a, const void *d_b, uint64_t n, uint64_t *mismatches)
try {
    if (!c || (!d_a && n) || (!d_b && n) || !mismatches) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long *d_bad = (unsigned long long *)((uint8_t *)c->d_small + 192);
    HIPCHK(c, hipMemsetAsync(d_bad, 0, 8, c->stream));
    if (n) {
        const uint64_t threads = (n + 15) / 16;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((threads + 255) / 256, 1u << 16);
        hipLaunchKernelGGL(za_k_compare, dim3(blocks), dim3(256), 0, c->stream, (const uint8_t *)d_a, (const uint8_t *)d_b, n, d_bad);
    }
    HIPCHK(c, hipGetLastError());
    unsigned long long bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *mismatches = bad;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- general gzip reader (host buffer) --------------------------------------------------------
// Restates the member state machine of GzipReader_read_into_buffer (zlib_ngmodule.c:2443-2611):
// header fields, inflate, CRC / ISIZE check, NUL padding.  Header bytes are parsed on the host (they
// are framing, not payload); every payload byte is decoded and checksummed on the GPU.
static int parse_gzip_header(const uint8_t *in, uint64_t in_len, uint64_t pos, uint64_t *data_off, bool *za_indexed, uint32_t *hcrc_len)
{
    *za_indexed = false; *hcrc_len = 0;
    if (in_len - pos < 10) return ZNGAMD_E_GZ_TRUNC;
    if (!(in[pos] == 0x1f && in[pos + 1] == 0x8b)) return ZNGAMD_E_GZ_MAGIC;
    if (in[pos + 2] != 8) return ZNGAMD_E_GZ_METHOD;
    const int flags = in[pos + 3];
    uint64_t cur = pos + 10;
    if (flags & 4) {
        if (cur + 2 >= in_len) return ZNGAMD_E_GZ_TRUNC;
        const uint64_t fl = in[cur] | (in[cur + 1] << 8);
        cur += 2;
        if (cur + fl >= in_len) return ZNGAMD_E_GZ_TRUNC;
        if (fl >= ZA_MEMBER_FIXED - 12 && in[cur] == 'Z' && in[cur + 1] == 'A' && flags == 4 && in[pos + 26] == 2) *za_indexed = true;
        cur += fl;
    }
    if (flags & 8) {
        const void *z = memchr(in + cur, 0, in_len - cur);
        if (!z) return ZNGAMD_E_GZ_TRUNC;
        cur = (uint64_t)((const uint8_t *)z - in) + 1;
    }
    if (flags & 16) {
        const void *z = memchr(in + cur, 0, in_len - cur);
        if (!z) return ZNGAMD_E_GZ_TRUNC;
        cur = (uint64_t)((const uint8_t *)z - in) + 1;
    }
    if (flags & 2) {
        if (cur + 2 >= in_len) return ZNGAMD_E_GZ_TRUNC;
        *hcrc_len = (uint32_t)(cur - pos);
        cur += 2;
    }
    *data_off = cur;
    return ZNGAMD_OK;
}

// why the chunk-parallel path handed over to the sequential decoder (ZNGAMD_DEBUG=1 prints it)
static int chunk_bail(int why)
{
    static const bool dbg = getenv("ZNGAMD_DEBUG") != nullptr;
    if (dbg) fprintf(stderr, "zng_amd: chunk-parallel inflate not used (reason %d)\n", why);
    return 1;
}

// Chunk-parallel inflate of one member: candidate chunk starts = positions after sync-flush
// markers and bit offsets where a dynamic block header parses; a count-only pass sizes every candidate up to the
// next listed boundary, the host follows the chain of real block boundaries and groups blocks into chunks.
// d_def = device pointer to the first deflate byte (inside a padded staging buffer), avail = bytes from there to
// the end of the input.  Returns 0 when the member was decoded (out_len / in_used set; CRC / ISIZE are checked by
// the caller), 1 when this path does not apply or anything looked odd (caller uses the sequential decoder, which
// also produces the exact error), <0 on engine errors, ZNGAMD_BUF_ERROR with *out_len = needed size when the
// output does not fit.
// Options: the stream may start at a bit offset inside the first byte with up to 32 KiB of history (a stream resumed at
// a block header), and with allow_cut a stream that runs past the end of the buffer is decoded up to its last complete
// block (info->cut, info->end_bit = where the next block header starts; *in_used = that bit's byte).
// A long stream goes through the pipeline in BATCHES of compressed input (ZNGAMD_CHUNK_BATCH_MIB, 512 MiB): every batch is a
// stream resumed at a block header with the 32 KiB in front of it as its history (the options above), cut in front of its last,
// incomplete piece -- so the scratch area of the one-pass marker decode (12 bytes per compressed byte) is bounded by the batch,
// not by the stream: 4 GiB of text asked for 18 GiB of it and went through the count pass instead (7.8 of 38 ms), a 16 GiB
// stream would not have fitted a busy GPU at all.
static int inflate_chunked_dev(zngamd_ctx *c, const uint8_t *d_def, uint64_t avail, uint8_t *d_out, uint64_t out_room,
                               uint64_t *out_len, uint64_t *in_used, const ChunkOpts &o, ChunkInfo *info)
{
    static const uint64_t batch = [] { const char *e = getenv("ZNGAMD_CHUNK_BATCH_MIB"); long v = e ? atol(e) : 512; return (uint64_t)(v < 16 ? 16 : v > 8192 ? 8192 : v) << 20; }();
    ChunkInfo dummy; if (!info) info = &dummy;
    if (avail <= batch + batch / 4) return inflate_chunked_once(c, d_def, avail, d_out, out_room, out_len, in_used, o, info);
    uint64_t pos_bit = o.start_bit, acc = 0;
    const uint8_t *dict = o.d_dict; uint32_t dict_len = o.dict_len;
    for (int b = 0;; b++) {
        const uint64_t byte0 = pos_bit >> 3;
        const bool lastb = avail - byte0 <= batch + batch / 4;
        ChunkOpts bo; bo.start_bit = (uint32_t)(pos_bit & 7ull); bo.d_dict = dict; bo.dict_len = dict_len; bo.allow_cut = lastb ? o.allow_cut : true;
        ChunkInfo bi; uint64_t bl = 0, bu = 0;
        const int r = inflate_chunked_once(c, d_def + byte0, lastb ? avail - byte0 : batch, d_out + acc, out_room - acc, &bl, &bu, bo, &bi);
        if (r == ZNGAMD_BUF_ERROR) {
            // the room this batch needs is known, the batches behind it are not decoded yet: their share is extrapolated from the
            // expansion so far (+ 1/16), so that a caller who resizes to the reported size retries once, not once per batch
            uint64_t need = acc + bl;
            if (!lastb) need = std::max<uint64_t>(need, (uint64_t)((long double)need * (long double)avail / (long double)(byte0 + batch) * 1.0625L) + (1u << 20));
            *out_len = need; *info = bi; return r;
        }
        if (r < 0) return r;
        if (r != 0 || (!lastb && !bi.ended && (bl == 0 || acc + bl < (uint64_t)ZA_WIN))) {
            // a batch this path does not take (or one that made no headway): the whole stream the old way, as one
            if (b == 0 && r != 0) { *info = bi; }
            return inflate_chunked_once(c, d_def, avail, d_out, out_room, out_len, in_used, o, info);
        }
        acc += bl;
        if (lastb || bi.ended) {
            *out_len = acc; *in_used = byte0 + bu;
            info->cut = bi.cut; info->ended = bi.ended; info->end_bit = byte0 * 8ull + bi.end_bit;
            info->last_bit = byte0 * 8ull + bi.last_bit; info->last_out = acc - bl + bi.last_out;
            return 0;
        }
        pos_bit = byte0 * 8ull + bi.end_bit;
        dict = d_out + acc - ZA_WIN; dict_len = ZA_WIN;               // (acc >= 32 KiB: checked above)
    }
}

static int inflate_chunked_once(zngamd_ctx *c, const uint8_t *d_def, uint64_t avail, uint8_t *d_out, uint64_t out_room,
                                uint64_t *out_len, uint64_t *in_used, const ChunkOpts &o, ChunkInfo *info)
{
    ChunkInfo dummy; if (!info) info = &dummy;
    *info = ChunkInfo();
    const bool resumed = o.start_bit != 0 || o.dict_len != 0 || o.allow_cut;
    if (avail < (1u << 16) || avail > (1ull << 36)) return chunk_bail(1);
    const uint32_t max_c = (uint32_t)std::min<uint64_t>(avail / 8 + 64, 1u << 24);
    const uint32_t max_s = (uint32_t)std::min<uint64_t>(avail / 4 + 1024, 1u << 25);
    HIPCHK(c, c->ccand.ensure((size_t)max_c + 1)); HIPCHK(c, c->csurv.ensure(max_s));
    uint32_t *d_n = (uint32_t *)((uint8_t *)c->d_small + 128);          // [0] candidates, [1] survivors
    PhaseClock pc_all(c, "chunk-parallel inflate, all of it");
    auto *pc = new PhaseClock(c, "  sync scan + candidates");
    struct PcOwner { PhaseClock *&p; ~PcOwner() { delete p; } } pc_owner{pc};
    auto phase = [&](const char *name) { delete pc; pc = nullptr; pc = new PhaseClock(c, name); };
    HIPCHK(c, hipMemsetAsync(d_n, 0, 8, c->stream));
    {   ProfScope ps(c, ZNGAMD_K_SCAN);
        const uint64_t threads = (avail + 15) / 16;
        hipLaunchKernelGGL(za_k_scan_sync, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, c->stream, d_def, avail, c->ccand.p, max_c, d_n);
    }
    HIPCHK(c, hipGetLastError());
    uint32_t cnt[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(cnt, d_n, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (cnt[0] > max_c) return chunk_bail(2);
    // sync-scan hits are byte positions: turn them into bit offsets on the host
    std::vector<uint64_t> cand(cnt[0]);
    if (cnt[0]) HIPCHK(c, hipMemcpy(cand.data(), c->ccand.p, (size_t)cnt[0] * 8, hipMemcpyDeviceToHost));
    for (auto &q : cand) q *= 8ull;
    // A stream written block-parallel (the reference's threaded writer, pigz, this engine) has a sync point every block: when
    // no stretch of more than 2 MiB is without one, those are boundaries enough and the bit-level header finder (a pass over
    // every bit offset of the stream, about as dear as the decode itself) is not run.
    static const uint32_t dense_min = [] { const long v = getenv("ZNGAMD_DENSE_MIN") ? atol(getenv("ZNGAMD_DENSE_MIN")) : 8; return (uint32_t)(v < 1 ? 1 : v); }();
    bool dense = cnt[0] >= dense_min;
    if (dense) {
        std::sort(cand.begin(), cand.end());
        uint64_t prev = o.start_bit, gap = 0;
        for (const uint64_t q : cand) { if (q > prev && q - prev > gap) gap = q - prev; if (q > prev) prev = q; }
        if (avail * 8ull > prev && avail * 8ull - prev > gap) gap = avail * 8ull - prev;
        dense = gap <= (16ull << 20);                                   // bits: 2 MiB
    }
    if (!dense) {
        { ProfScope ps(c, ZNGAMD_K_SCAN);
          hipLaunchKernelGGL(za_k_find_blocks_a, dim3((uint32_t)((avail / 4 + 1 + ZA_FINDA_THREADS - 1) / ZA_FINDA_THREADS)), dim3(ZA_FINDA_THREADS), 0, c->stream, d_def, avail, c->csurv.p, max_s, d_n + 1); }      // a thread per aligned dword
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(cnt + 1, d_n + 1, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (cnt[1] > 0 && cnt[1] <= max_s) {
        HIPCHK(c, hipMemsetAsync(d_n, 0, 4, c->stream));
        { ProfScope ps(c, ZNGAMD_K_SCAN);
          hipLaunchKernelGGL(za_k_find_blocks_b, dim3((cnt[1] + 63) / 64), dim3(64), 0, c->stream, d_def, avail, c->csurv.p, cnt[1], c->ccand.p, max_c, d_n); }
        HIPCHK(c, hipGetLastError());
        uint32_t nb = 0;
        HIPCHK(c, hipMemcpyAsync(&nb, d_n, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (nb > 0 && nb <= max_c) {
            const size_t old = cand.size();
            cand.resize(old + nb);
            HIPCHK(c, hipMemcpy(cand.data() + old, c->ccand.p, (size_t)nb * 8, hipMemcpyDeviceToHost));
        }
    }
    cand.push_back(o.start_bit);
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    const uint32_t n = (uint32_t)cand.size();
    if (getenv("ZNGAMD_DEBUG")) fprintf(stderr, "zng_amd: chunk finder: %u sync hits, %u header survivors, %u candidates\n", cnt[0], cnt[1], n);
    c->chunk_stats[0] += cnt[0]; c->chunk_stats[1] += cnt[1]; c->chunk_stats[2] += n;
    if (n < 8 || n > max_c) return chunk_bail(3);                    // too few boundaries to be worth it
    std::vector<ZaChunk> chain;
    std::vector<ZaChunkRes> res;
    uint64_t acc = 0, end_bit = 0;
    bool ended = false, placed = false;
    // ONE decoding pass where the boundaries are the stream's own sync points and the pieces between them are large enough to be
    // chunks as they are (what block-parallel writers emit: this engine, the reference's threaded writer, pigz): every piece is
    // decoded to the next boundary into a scratch area of its own (6 symbols per compressed byte + 64 Ki; a piece that outgrows it
    // sends the stream to the two passes below), sizes and ends come out of that pass, and the window kernels read the symbols
    // where they lie.  The count pass it saves decoded everything once to learn 16 bytes per piece (1.9 of 6.9 ms for 256 MiB).
    static const bool one_pass_allowed = getenv("ZNGAMD_TWO_PASS") == nullptr;
    if (dense && one_pass_allowed && avail / n >= (8u << 10)) {
        std::vector<ZaChunk> pieces(n);
        uint64_t sc = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t ext = ((i + 1 < n ? cand[i + 1] : avail * 8ull) - cand[i] + 7) >> 3;
            ZaChunk pc; pc.in_bit = cand[i]; pc.out_off = 0; pc.out_len = 6 * ext + 65536; pc.end_bit = 0; pc.src_off = sc;
            pieces[i] = pc;
            sc += (pc.out_len + 7) & ~7ull;                            // (16-byte aligned symbol areas)
        }
        // (no room for the scratch area on this device right now: not an error -- the two passes below need a sixth of it)
        bool scratch_ok = sc * 2 <= (16ull << 30);
        if (scratch_ok && c->out16.ensure(sc + 64) != hipSuccess) { (void)hipGetLastError(); scratch_ok = false; }
        if (scratch_ok) {
            phase("  marker decode (one pass)");
            HIPCHK(c, c->cchunks.ensure(n)); HIPCHK(c, c->cres.ensure(n));
            HIPCHK(c, hipMemcpyAsync(c->ccand.p, cand.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(c->cchunks.p, pieces.data(), (size_t)n * sizeof(ZaChunk), hipMemcpyHostToDevice, c->stream));
            { ProfScope ps(c, ZNGAMD_K_INFLATE);
              if (n >= ZNGAMD_CHUNKS_MANY_FROM)
                  hipLaunchKernelGGL((za_k_chunk_decode<384, ZA_CHUNK_Q_M, ZA_CHUNK_RING_M, 9, 8>), dim3(n), dim3(64), 0, c->stream, d_def, avail, c->cchunks.p, c->out16.p, c->cres.p, (uint64_t)o.start_bit, o.dict_len, c->ccand.p, n);
              else if (n >= ZNGAMD_CHUNKS_SMALL_FROM)
                  hipLaunchKernelGGL((za_k_chunk_decode<ZA_CHUNK_BITS_S, ZA_CHUNK_Q_S, ZA_CHUNK_RING_S>), dim3(n), dim3(64), 0, c->stream, d_def, avail, c->cchunks.p, c->out16.p, c->cres.p, (uint64_t)o.start_bit, o.dict_len, c->ccand.p, n);
              else
                  hipLaunchKernelGGL((za_k_chunk_decode<1024, 3072, 4096>), dim3(n), dim3(64), 0, c->stream, d_def, avail, c->cchunks.p, c->out16.p, c->cres.p, (uint64_t)o.start_bit, o.dict_len, c->ccand.p, n); }
            HIPCHK(c, hipGetLastError());
            res.resize(n);
            HIPCHK(c, hipMemcpyAsync(res.data(), c->cres.p, (size_t)n * sizeof(ZaChunkRes), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            bool good = true, cut = false;
            size_t i = (size_t)(std::lower_bound(cand.begin(), cand.end(), (uint64_t)o.start_bit) - cand.begin());
            for (uint32_t guard = 0; guard <= n && good; guard++) {
                const ZaChunkRes &r = res[i];
                if (r.status == ZA_I_INPUT) {
                    cut = true;
                    if (o.allow_cut && !chain.empty()) { end_bit = cand[i]; break; }
                }
                if ((r.status != ZA_I_SYNC && r.status != ZA_I_END) || r.max_back > acc + o.dict_len) { good = false; break; }
                ZaChunk ch; ch.in_bit = cand[i]; ch.out_off = acc; ch.out_len = r.out_len; ch.end_bit = r.bits; ch.src_off = pieces[i].src_off;
                chain.push_back(ch);
                acc += r.out_len;
                if (r.status == ZA_I_END) { end_bit = r.bits; ended = true; break; }
                auto it = std::lower_bound(cand.begin(), cand.end(), r.bits);
                if (it == cand.end() || *it != r.bits) { good = false; break; }
                i = (size_t)(it - cand.begin());
            }
            if (good && (ended || (o.allow_cut && cut && !chain.empty())) && chain.size() >= (resumed ? 1u : 4u)) { placed = true; info->cut = cut; info->last_bit = chain.back().in_bit; info->last_out = chain.back().out_off; }
            else { chain.clear(); acc = 0; end_bit = 0; ended = false; }         // anything odd: the two passes decide
        }
    }
    if (!placed) {
    phase("  count pass");
    HIPCHK(c, hipMemcpyAsync(c->ccand.p, cand.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->cres.ensure(n));
    { ProfScope ps(c, ZNGAMD_K_INFLATE);
      if (n >= ZNGAMD_CHUNKS_SMALL_FROM)
          hipLaunchKernelGGL(za_k_chunk_count<512>, dim3(n), dim3(64), 0, c->stream, d_def, avail, c->ccand.p, n, c->cres.p, (uint64_t)o.start_bit, o.dict_len);
      else
          hipLaunchKernelGGL(za_k_chunk_count<1024>, dim3(n), dim3(64), 0, c->stream, d_def, avail, c->ccand.p, n, c->cres.p, (uint64_t)o.start_bit, o.dict_len); }
    HIPCHK(c, hipGetLastError());
    res.resize(n);
    HIPCHK(c, hipMemcpyAsync(res.data(), c->cres.p, (size_t)n * sizeof(ZaChunkRes), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // follow the chain of real block boundaries from the start of the stream, then group blocks into chunks:
    // about 4096 of them (12 marker decoders fit a CU), none below 32 KiB (a chunk's tail is the next window)
    phase("  chain of blocks on the host");
    std::vector<ZaChunk> blocks;
    {
        size_t i = (size_t)(std::lower_bound(cand.begin(), cand.end(), (uint64_t)o.start_bit) - cand.begin());
        for (uint32_t guard = 0; guard <= n; guard++) {
            const ZaChunkRes &r = res[i];
            if (r.status == ZA_I_INPUT) {
                info->cut = true;
                // stop in front of the incomplete block: the last header this piece entered (r.bits, with r.out_len bytes in front
                // of it).  Blocks that the finder does not list -- stored, fixed, a dynamic header cut by the end of the input --
                // are complete up to there, and a stream resumed at the piece's own start would decode them again on every call.
                if (o.allow_cut && r.bits > cand[i] && r.bits <= avail * 8ull && (r.out_len > 0 || !blocks.empty())) {
                    ZaChunk b; b.in_bit = cand[i]; b.out_off = acc; b.out_len = r.out_len; b.end_bit = r.bits; b.src_off = acc;
                    blocks.push_back(b);
                    acc += r.out_len;
                    end_bit = r.bits; break;
                }
                if (o.allow_cut && !blocks.empty()) { end_bit = cand[i]; break; }
            }
            if (r.status != ZA_I_SYNC && r.status != ZA_I_END) return chunk_bail(4);
            ZaChunk b; b.in_bit = cand[i]; b.out_off = acc; b.out_len = r.out_len; b.end_bit = r.bits; b.src_off = acc;
            blocks.push_back(b);
            acc += r.out_len;
            if (r.status == ZA_I_END) { end_bit = r.bits; ended = true; break; }
            auto it = std::lower_bound(cand.begin(), cand.end(), r.bits);
            if (it == cand.end() || *it != r.bits) return chunk_bail(5);
            i = (size_t)(it - cand.begin());
        }
    }
    if (!blocks.empty()) { info->last_bit = blocks.back().in_bit; info->last_out = blocks.back().out_off; }
    static const uint64_t chunk_div = [] { const long v = getenv("ZNGAMD_CHUNK_DIV") ? atol(getenv("ZNGAMD_CHUNK_DIV")) : 4096; return (uint64_t)(v < 1 ? 1 : v); }();
    const uint64_t target = std::max<uint64_t>(32u << 10, acc / chunk_div);
    for (size_t b = 0; b < blocks.size();) {
        ZaChunk cur = blocks[b++];
        while (b < blocks.size() && cur.out_len < target) { cur.out_len += blocks[b].out_len; cur.end_bit = blocks[b].end_bit; b++; }
        chain.push_back(cur);
    }
    if (chain.size() > 1 && chain.back().out_len < target) {       // short last chunk: merge into its predecessor
        ZaChunk last = chain.back(); chain.pop_back();
        chain.back().out_len += last.out_len; chain.back().end_bit = last.end_bit;
    }
    if (!ended && !(o.allow_cut && info->cut && !chain.empty())) return chunk_bail(6);
    if (chain.size() < (resumed ? 1u : 4u)) return chunk_bail(6);
    }
    info->ended = ended; info->end_bit = end_bit;
    *out_len = acc; *in_used = ended ? (end_bit + 7) >> 3 : end_bit >> 3;
    if (acc > out_room) return ZNGAMD_BUF_ERROR;
    const uint32_t m = (uint32_t)chain.size();
    const uint32_t groups = (m + ZA_CHUNK_GROUP - 1) / ZA_CHUNK_GROUP;
    HIPCHK(c, c->cchunks.ensure(m)); HIPCHK(c, c->winbuf.ensure((size_t)groups * ZA_WIN));
    HIPCHK(c, c->ccomp.ensure((size_t)m * ZA_WIN));
    if (!placed) {
        phase("  marker decode");
        HIPCHK(c, c->out16.ensure(acc + 64));
        HIPCHK(c, hipMemcpyAsync(c->cchunks.p, chain.data(), (size_t)m * sizeof(ZaChunk), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, c->cres.ensure(m));
        { ProfScope ps(c, ZNGAMD_K_INFLATE);
          if (m >= ZNGAMD_CHUNKS_MANY_FROM)
              hipLaunchKernelGGL((za_k_chunk_decode<384, ZA_CHUNK_Q_M, ZA_CHUNK_RING_M, 9, 8>), dim3(m), dim3(64), 0, c->stream, d_def, avail, c->cchunks.p, c->out16.p, c->cres.p, (uint64_t)o.start_bit, o.dict_len, (const uint64_t *)nullptr, 0u);
          else if (m >= ZNGAMD_CHUNKS_SMALL_FROM)
              hipLaunchKernelGGL((za_k_chunk_decode<ZA_CHUNK_BITS_S, ZA_CHUNK_Q_S, ZA_CHUNK_RING_S, ZA_CHUNK_LB_2P, ZA_CHUNK_DB_2P>), dim3(m), dim3(64), 0, c->stream, d_def, avail, c->cchunks.p, c->out16.p, c->cres.p, (uint64_t)o.start_bit, o.dict_len, (const uint64_t *)nullptr, 0u);
          else
              hipLaunchKernelGGL((za_k_chunk_decode<1024, 3072, 4096>), dim3(m), dim3(64), 0, c->stream, d_def, avail, c->cchunks.p, c->out16.p, c->cres.p, (uint64_t)o.start_bit, o.dict_len, (const uint64_t *)nullptr, 0u); }
        HIPCHK(c, hipGetLastError());
        res.resize(m);
        HIPCHK(c, hipMemcpyAsync(res.data(), c->cres.p, (size_t)m * sizeof(ZaChunkRes), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (uint32_t k = 0; k < m; k++) {
            const bool last = k + 1 == m;
            if (res[k].status != ((last && ended) ? ZA_I_END : ZA_I_SYNC) || res[k].out_len != chain[k].out_len || res[k].bits != chain[k].end_bit) return chunk_bail(7);
            if (res[k].max_back > chain[k].out_off + o.dict_len) return chunk_bail(8);       // reference before the start of the stream
        }
    } else HIPCHK(c, hipMemcpyAsync(c->cchunks.p, chain.data(), (size_t)m * sizeof(ZaChunk), hipMemcpyHostToDevice, c->stream));
    phase("  windows + resolve");
    { ProfScope ps(c, ZNGAMD_K_INFLATE);
      hipLaunchKernelGGL(za_k_chunk_compose, dim3(groups), dim3(1024), 0, c->stream, c->out16.p, c->cchunks.p, m, c->ccomp.p);
      hipLaunchKernelGGL(za_k_chunk_chain, dim3(1), dim3(1024), 0, c->stream, c->ccomp.p, m, c->winbuf.p, o.d_dict, o.dict_len);
      hipLaunchKernelGGL(za_k_chunk_resolve, dim3(m), dim3(ZA_RESOLVE_THREADS), 0, c->stream, c->out16.p, c->cchunks.p, c->ccomp.p, c->winbuf.p, d_out); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->chunk_stats[3] += m;
    return 0;
}

// BGZF hop: every member must be `1f 8b 08 04`, carry a 'B','C' subfield of length 2 (block size - 1) and
// tile the buffer exactly; anything else makes the caller use the general reader.
static bool hop_bgzf(const uint8_t *in, uint64_t in_len, std::vector<ZaMember> &hm, uint64_t *total_out,
                     bool allow_tail = false, uint64_t *covered = nullptr)
{
    auto le16 = [&](uint64_t o) { return (uint32_t)in[o] | ((uint32_t)in[o + 1] << 8); };
    auto le32 = [&](uint64_t o) { return (uint32_t)in[o] | ((uint32_t)in[o + 1] << 8) | ((uint32_t)in[o + 2] << 16) | ((uint32_t)in[o + 3] << 24); };
    uint64_t pos = 0, outp = 0;
    hm.clear();
    while (pos < in_len) {
        if (in_len - pos < 12 + 6 + 8) { if (allow_tail && !hm.empty()) break; return false; }
        if (in[pos] != 0x1f || in[pos + 1] != 0x8b || in[pos + 2] != 8 || in[pos + 3] != 4) { if (allow_tail && !hm.empty()) break; return false; }
        const uint64_t xlen = le16(pos + 10);
        uint64_t cur = pos + 12;
        const uint64_t end = cur + xlen;
        if (end + 8 > in_len) { if (allow_tail && !hm.empty()) break; return false; }
        long bsize = -1;
        bool bad = false;
        while (cur + 4 <= end) {
            const uint32_t sl = le16(cur + 2);
            if (cur + 4 + sl > end) { bad = true; break; }
            if (in[cur] == 'B' && in[cur + 1] == 'C' && sl == 2) bsize = (long)le16(cur + 4);
            cur += 4 + sl;
        }
        if (bad || bsize < 0) { if (allow_tail && !hm.empty()) break; return false; }
        const uint64_t msize = (uint64_t)bsize + 1;
        if (msize < (end - pos) + 8 || pos + msize > in_len) { if (allow_tail && !hm.empty()) break; return false; }
        ZaMember m;
        m.in_off = end; m.in_len = msize - (end - pos) - 8; m.out_off = outp;
        m.out_len = le32(pos + msize - 4); m.crc = le32(pos + msize - 8); m.index_off = 0; m.nseg = 0;
        hm.push_back(m);
        pos += msize; outp += m.out_len;
    }
    *total_out = outp;
    if (covered) *covered = pos;
    return pos == in_len || (allow_tail && !hm.empty());
}

// A file made of many small ordinary members (concatenated logs, `cat *.gz`, files written by appending): member by member
// every one costs a few launches and synchronisations (3.5 ms each; 2 000 members of 16 KiB took 7 s).  Where members start is
// not written anywhere, but every start shows the gzip magic: all places that look like a member header are sized at once by
// the count kernel (one wavefront each, to the end of their own stream), the host then follows the chain of members from
// offset 0 -- a false candidate inside compressed data is simply never reached -- and the members of the chain are decoded
// in one launch like BGZF members, CRC-32 and ISIZE checked in the kernel.  Returns the members of the longest chain prefix
// that is complete and unremarkable; the member loop of gunzip_impl goes on behind it (large members, errors, the tail).
static int hop_plain_members(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, std::vector<ZaMember> &hm, std::vector<uint64_t> &hpos,
                             uint64_t *total_out, uint64_t *covered)
{
    hm.clear(); hpos.clear(); *total_out = 0; *covered = 0;
    if (in_len < 40) return ZNGAMD_OK;
    struct Cand { uint64_t pos, doff; };
    std::vector<Cand> cv;
    uint64_t prev = 0, gap = 0;
    for (const uint8_t *p = in, *e = in + in_len - 18; p < e; p++) {
        p = (const uint8_t *)memchr(p, 0x1f, (size_t)(e - p));
        if (!p) break;
        if (p[1] != 0x8b || p[2] != 8 || (p[3] & 0xE0)) continue;
        const uint64_t pos = (uint64_t)(p - in);
        uint64_t doff = 0; bool za = false; uint32_t hl = 0;
        if (parse_gzip_header(in, in_len, pos, &doff, &za, &hl) != ZNGAMD_OK || hl) continue;     // (a header CRC is left to the member loop)
        if (pos - prev > gap) gap = pos - prev;
        prev = pos;
        cv.push_back(Cand{pos, doff});
        if (cv.size() > (1u << 20)) return ZNGAMD_OK;
    }
    if (in_len - prev > gap) gap = in_len - prev;
    // worth it for many small members only: a large member is better off chunk-parallel in the member loop
    if (cv.size() < 4 || cv[0].pos != 0 || gap > (1ull << 20)) return ZNGAMD_OK;
    const uint32_t n = (uint32_t)cv.size();
    std::vector<uint64_t> bits(n);
    for (uint32_t i = 0; i < n; i++) bits[i] = cv[i].doff * 8ull;
    HIPCHK(c, c->ccand.ensure((size_t)n + 1)); HIPCHK(c, c->cres.ensure(n));
    HIPCHK(c, hipMemcpyAsync(c->ccand.p, bits.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    { ProfScope ps(c, ZNGAMD_K_INFLATE);
      hipLaunchKernelGGL(za_k_chunk_count<512>, dim3(n), dim3(64), 0, c->stream, c->st_in.p, in_len, c->ccand.p, n, c->cres.p, 0ull, 0u, 1); }
    HIPCHK(c, hipGetLastError());
    std::vector<ZaChunkRes> res(n);
    HIPCHK(c, hipMemcpyAsync(res.data(), c->cres.p, (size_t)n * sizeof(ZaChunkRes), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    uint64_t pos = 0, outp = 0;
    size_t i = 0;
    while (pos < in_len) {
        while (i < n && cv[i].pos < pos) i++;
        if (i >= n || cv[i].pos != pos) break;                         // not a (plain) member header here: the member loop looks at it
        const ZaChunkRes &r = res[i];
        if (r.status != ZA_I_END || r.out_len > 0xFFFFFFFFull) break;  // truncated, damaged, huge: the member loop gives the verdict
        const uint64_t dend = (r.bits + 7) >> 3;                       // first byte behind the deflate stream
        if (dend + 8 > in_len) break;
        ZaMember m;
        m.in_off = cv[i].doff; m.in_len = dend - cv[i].doff; m.out_off = outp; m.out_len = (uint32_t)r.out_len;
        m.crc = 0; m.index_off = 0; m.nseg = 0;
        hm.push_back(m);
        hpos.push_back(cv[i].pos);
        outp += r.out_len;
        pos = dend + 8;
        while (pos < in_len && in[pos] == 0) pos++;
        *covered = pos;
    }
    *total_out = outp;
    return ZNGAMD_OK;
}

struct StreamRun { int status; uint64_t out_len; uint64_t in_bits; bool chunked; };
static int stream_finish(zngamd_ctx *c, zngamd_gz_state *st, const uint8_t *in, uint64_t in_len, uint64_t doff, bool last, const StreamRun &run,
                         uint32_t dl, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members, uint64_t *in_consumed);

// partial: more input may follow -- complete members are decoded, an incomplete last one is left alone and
// *in_consumed tells where it starts (ZNGAMD_OK; nothing consumed = the window holds no complete member yet).
// With a stream state (st, partial only) a FIRST member that runs past the window is not left alone: the blocks of it that
// are complete were decoded on the way to finding that out, so they are handed out and the state says where the next
// window continues (what zngamd_gunzip_stream would otherwise do in a second pass over the same window).
struct ZaFileIndex;
static int decode_stream_prefix_indexed(zngamd_ctx *c, ZaFileIndex *ix, uint64_t out_total, const uint8_t *h_def, const uint8_t *d_def, uint64_t avail,
                                        const uint8_t *d_dict, uint32_t dict_len, uint8_t *d_out, uint64_t out_room, bool allow_cut,
                                        StreamRun *run, uint64_t *needed);
static int gunzip_impl(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, bool partial, uint8_t *out, uint64_t out_cap,
                       uint64_t *out_len, uint32_t *n_members, uint64_t *in_consumed, zngamd_gz_state *st = nullptr, void *index = nullptr)
{
    *out_len = 0;
    *in_consumed = 0;
    if (n_members) *n_members = 0;
    int r = stage_in(c, in, in_len);
    if (r) return r;
    HIPCHK(c, c->st_out.ensure(out_cap + 64));
    uint64_t pos = 0, op = 0, last_member_bytes = 0;
    uint32_t members = 0;
    int ret = ZNGAMD_OK;
    bool prefix_done = false;                        // the fast path for indexed members took the front of the buffer
    // fast path: the whole stream is indexed members -> two-pass scheme
    {
        uint64_t doff; bool za; uint32_t hl;
        if (in_len >= ZA_MEMBER_FIXED + 8 && parse_gzip_header(in, in_len, 0, &doff, &za, &hl) == ZNGAMD_OK && za) {
            std::vector<ZaMember> hm; uint64_t total = 0;
            uint64_t covered = 0;
            // (a run of indexed members at the front is enough: what follows them -- members of another writer appended to the
            // file -- goes to the member loop below)
            if (scan_members_dev(c, c->st_in.p, in_len, hm, &total, true, &covered) == ZNGAMD_OK) {
                if (total > out_cap) { *out_len = total; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
                HIPCHK(c, c->members.ensure(hm.size())); HIPCHK(c, c->mstatus.ensure(hm.size()));
                HIPCHK(c, hipMemcpyAsync(c->members.p, hm.data(), hm.size() * sizeof(ZaMember), hipMemcpyHostToDevice, c->stream));
                r = inflate_members_dev(c, c->st_in.p, in_len, c->members.p, (uint32_t)hm.size(), c->st_out.p, out_cap, c->mstatus.p);
                if (r) return r;
                std::vector<int32_t> st(hm.size());
                HIPCHK(c, hipMemcpyAsync(st.data(), c->mstatus.p, st.size() * 4, hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                prof_collect(c);
                bool all_ok = true;
                for (size_t i = 0; i < st.size(); i++) if (st[i] != ZA_I_OK) { all_ok = false; break; }
                // NUL padding behind the members is skipped, as the reference's reader does (zlib_ngmodule.c:2604-2612) and as the member
                // loop below does behind every member it decodes
                uint64_t behind = covered;
                while (behind < in_len && ((const uint8_t *)in)[behind] == 0) behind++;
                if (all_ok && (behind == in_len || partial)) {
                    if (total) { const int rc_ = d2h_payload(c, out, c->st_out.p, total); if (rc_) return rc_; }
                    *out_len = total;
                    if (n_members) *n_members = (uint32_t)hm.size();
                    c->paths[ZNGAMD_PATH_INDEXED] += hm.size();
                    *in_consumed = behind == in_len ? in_len : covered;
                    return ZNGAMD_OK;
                }
                if (all_ok) {                        // the indexed members are a prefix of the buffer: their bytes stay where they are
                    c->paths[ZNGAMD_PATH_INDEXED] += hm.size();
                    op = total; members = (uint32_t)hm.size(); pos = behind;
                    prefix_done = true;
                }
                // anything unexpected (foreign 'ZA' field, stored blocks, corruption): the sequential
                // reader below decides, member by member
            }
        }
    }
    // second fast path: BGZF-style members ('B','C' subfield = block size - 1).  The member table comes from a
    // header hop over the host copy; all members are then decoded in one launch, one wavefront each.
    if (!prefix_done) {
        std::vector<ZaMember> hm; uint64_t total = 0;
        uint64_t covered = 0;
        if (hop_bgzf(in, in_len, hm, &total, partial, &covered) && hm.size() > 1) {
            if (total > out_cap) { *out_len = total; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
            const uint32_t n = (uint32_t)hm.size();
            HIPCHK(c, c->members.ensure(n)); HIPCHK(c, c->mstatus.ensure(n));
            HIPCHK(c, hipMemcpyAsync(c->members.p, hm.data(), (size_t)n * sizeof(ZaMember), hipMemcpyHostToDevice, c->stream));
            { ProfScope ps(c, ZNGAMD_K_INFLATE);
              hipLaunchKernelGGL(za_k_inflate_serial_members, dim3(n), dim3(64), 0, c->stream, c->st_in.p, in_len, c->members.p,
                                 c->st_out.p, out_cap, c->d_crc_table, c->d_x8k, c->mstatus.p); }
            HIPCHK(c, hipGetLastError());
            std::vector<int32_t> st(n);
            HIPCHK(c, hipMemcpyAsync(st.data(), c->mstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            prof_collect(c);
            uint32_t good = 0;
            while (good < n && st[good] == ZA_I_OK) good++;
            const uint64_t produced = good < n ? hm[good].out_off : total;
            if (produced) { const int rc_ = d2h_payload(c, out, c->st_out.p, produced); if (rc_) return rc_; }
            *out_len = produced;
            if (n_members) *n_members = good;
            c->paths[ZNGAMD_PATH_BGZF] += good;
            if (good == n) { *in_consumed = covered; return ZNGAMD_OK; }
            const int code = st[good];
            if (code == ZA_I_CRC) { c->err = "CRC check failed"; return ZNGAMD_E_GZ_CRC; }
            if (code == ZA_I_LENGTH) { c->err = "Incorrect length of data produced"; return ZNGAMD_E_GZ_LENGTH; }
            if (code == ZA_I_INPUT) return ZNGAMD_E_GZ_TRUNC;
            c->err = "invalid deflate data";
            return ZNGAMD_DATA_ERROR;
        }
    }
    // third fast path: a run of small ordinary members at the front (see hop_plain_members); the loop below continues behind it
    if (!prefix_done) {
        std::vector<ZaMember> hm; std::vector<uint64_t> hpos; uint64_t total = 0, covered = 0;
        r = hop_plain_members(c, in, in_len, hm, hpos, &total, &covered);
        if (r) return r;
        if (hm.size() >= 2) {
            if (total > out_cap) { *out_len = total; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
            const uint32_t n = (uint32_t)hm.size();
            HIPCHK(c, c->members.ensure(n)); HIPCHK(c, c->mstatus.ensure(n));
            HIPCHK(c, hipMemcpyAsync(c->members.p, hm.data(), (size_t)n * sizeof(ZaMember), hipMemcpyHostToDevice, c->stream));
            { ProfScope ps(c, ZNGAMD_K_INFLATE);
              hipLaunchKernelGGL(za_k_inflate_serial_members, dim3(n), dim3(64), 0, c->stream, c->st_in.p, in_len, c->members.p,
                                 c->st_out.p, out_cap, c->d_crc_table, c->d_x8k, c->mstatus.p); }
            HIPCHK(c, hipGetLastError());
            std::vector<int32_t> st(n);
            HIPCHK(c, hipMemcpyAsync(st.data(), c->mstatus.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            prof_collect(c);
            uint32_t good = 0;
            while (good < n && st[good] == ZA_I_OK) good++;
            if (good) {                                   // the loop takes over at the first member that did not check out
                op = good < n ? hm[good].out_off : total;
                members = good;
                c->paths[ZNGAMD_PATH_BGZF] += good;
                pos = good == n ? covered : hpos[good];
            }
        }
    }
    for (;;) {
        if (pos == in_len) break;
        uint64_t doff = 0; bool za = false; uint32_t hl = 0;
        r = parse_gzip_header(in, in_len, pos, &doff, &za, &hl);
        if (r == ZNGAMD_E_GZ_TRUNC && partial) break;                     // incomplete header: wait for more input
        if (r) { ret = r; break; }
        if (hl) {
            uint32_t hc = 0;
            r = checksum_dev(c, c->st_in.p + pos, hl, &hc, nullptr);
            if (r) return r;
            const uint32_t want = in[pos + hl] | (in[pos + hl + 1] << 8);
            if ((hc & 0xFFFFu) != want) { ret = ZNGAMD_E_GZ_HCRC; break; }
        }
        ZaInfResult res;
        bool chunked = false;
        {   // chunk-parallel decode where the stream offers enough block boundaries, else one wavefront.
            // The finder and the count pass look at everything they are given: behind the first member they get a
            // bounded piece (twice the previous member, at least 4 MiB; four times more whenever the member proves to be
            // longer) instead of the whole rest of the file, which made a file of N large members cost N^2 / 2 passes.
            uint64_t clen = 0, cused = 0;
            ChunkInfo ci;
            const uint64_t rest = in_len - doff;
            uint64_t piece = rest;
            if (members > 0) piece = std::min<uint64_t>(rest, std::max<uint64_t>(4ull << 20, 2 * last_member_bytes));
            int cr;
            if (index && members == 0 && op == 0 && pos == 0) {
                // the file's first member with the writer's index (zngamd_gz_state.index): its units inside the window side by side --
                // all of the member if the window holds it, else as far as the window goes (the state then continues it)
                StreamRun run; uint64_t needed = 0;
                HIPCHK(c, c->st_out.ensure(out_cap + 64));
                const int ri = decode_stream_prefix_indexed(c, (ZaFileIndex *)index, 0, in + doff, c->st_in.p + doff, in_len - doff, nullptr, 0,
                                                            c->st_out.p, out_cap, partial && st, &run, &needed);
                if (ri == ZNGAMD_BUF_ERROR) { *out_len = needed; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
                if (ri < 0) return ri;
                if (ri == 1 && (run.status == ZA_I_END || (partial && st && run.out_len))) {
                    zngamd_gz_state tmp_state; zngamd_gz_state *ss = st;
                    if (!ss) { memset(&tmp_state, 0, sizeof tmp_state); ss = &tmp_state; }
                    ss->in_member = 0; ss->start_bit = 0; ss->crc = 0; ss->window_len = 0; ss->out_total = 0;
                    return stream_finish(c, ss, in, in_len, doff, !partial, run, 0, out, out_cap, out_len, n_members, in_consumed);
                }
            }
            const bool may_continue = partial && st && members == 0 && op == 0 && pos == 0;
            ChunkOpts copts; copts.allow_cut = may_continue;
            for (;;) {
                cr = inflate_chunked_dev(c, c->st_in.p + doff, piece, c->st_out.p + op, out_cap - op, &clen, &cused, copts, &ci);
                if (piece < rest && ci.cut) { piece = std::min<uint64_t>(rest, piece * 4); continue; }      // the member is longer than the piece: more
                break;
            }
            if (may_continue && cr == 0 && !ci.ended) {           // the member goes on behind the window: its complete blocks are out
                st->in_member = 0; st->start_bit = 0; st->crc = 0; st->window_len = 0; st->out_total = 0;
                StreamRun run; run.status = ZA_I_INPUT; run.out_len = clen; run.in_bits = ci.end_bit; run.chunked = true;
                return stream_finish(c, st, in, in_len, doff, false, run, 0, out, out_cap, out_len, n_members, in_consumed);
            }
            const bool cut = ci.cut;
            if (cr < 0 && cr != ZNGAMD_BUF_ERROR) return cr;
            if (cr == ZNGAMD_BUF_ERROR) { *out_len = op + clen; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
            if (cr == 0) { chunked = true; res.status = ZA_I_END; res.out_len = clen; res.in_bits = cused * 8; res.block_bits = 0; res.block_out = 0; }
            else if (cut && partial) break;                               // the member runs past the window: wait for more input
            else {
                r = inflate_serial_dev(c, c->st_in.p + doff, in_len - doff, nullptr, 0, c->st_out.p + op, out_cap - op, &res);
                if (r) return r;
            }
        }
        if (res.status == ZA_I_INPUT && partial) break;
        if (res.status != ZA_I_END) {
            *out_len = op + res.out_len;
            if (res.status == ZA_I_OUTFULL) ret = ZNGAMD_BUF_ERROR;
            else if (res.status == ZA_I_INPUT) ret = ZNGAMD_E_GZ_TRUNC;
            else ret = map_status(res.status);
            if (ret == ZNGAMD_BUF_ERROR || ret == ZNGAMD_E_GZ_TRUNC) {
                if (op + res.out_len) { const int rc_ = d2h_payload(c, out, c->st_out.p, op + res.out_len); if (rc_) return rc_; }
            }
            c->err = "gzip member did not end"; return ret;
        }
        uint32_t crc = 0;
        r = checksum_dev(c, c->st_out.p + op, res.out_len, &crc, nullptr);
        if (r) return r;
        uint64_t cur = doff + ((res.in_bits + 7) >> 3);
        if (in_len - cur < 8) { if (!partial) ret = ZNGAMD_E_GZ_TRUNC; break; }
        const uint32_t tc = in[cur] | (in[cur + 1] << 8) | (in[cur + 2] << 16) | ((uint32_t)in[cur + 3] << 24);
        const uint32_t tl = in[cur + 4] | (in[cur + 5] << 8) | (in[cur + 6] << 16) | ((uint32_t)in[cur + 7] << 24);
        if (tc != crc) { ret = ZNGAMD_E_GZ_CRC; char b[96]; snprintf(b, sizeof b, "CRC check failed %u != %u", tc, crc); c->err = b; break; }
        if (tl != (uint32_t)(res.out_len & 0xFFFFFFFFull)) { ret = ZNGAMD_E_GZ_LENGTH; c->err = "Incorrect length of data produced"; break; }
        cur += 8; op += res.out_len; members++;
        last_member_bytes = cur - pos;
        c->paths[chunked ? ZNGAMD_PATH_CHUNKED : ZNGAMD_PATH_SEQUENTIAL]++;
        while (cur < in_len && in[cur] == 0) cur++;
        pos = cur;
    }
    if (op) { const int rc_ = d2h_payload(c, out, c->st_out.p, op); if (rc_) return rc_; }
    *out_len = op;
    *in_consumed = pos;
    if (n_members) *n_members = members;
    return ret;
}

int zngamd_gunzip(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members)
try {
    if (!c || (!in && in_len) || (!out && out_cap) || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t used = 0;
    return gunzip_impl(c, in, in_len, false, out, out_cap, out_len, n_members, &used);
} ZA_ABI_GUARD

// ---- one member that is larger than the caller's window: decoded block-wise across calls -------------------

// Decodes the deflate stream that starts at bit `start_bit` of d_def[0] with `dict_len` bytes of history.  With allow_cut a
// stream that runs past the buffer is decoded up to its last complete block: status ZA_I_INPUT, in_bits = where the next
// block header starts.
static int decode_stream_prefix(zngamd_ctx *c, const uint8_t *d_def, uint64_t avail, uint32_t start_bit, const uint8_t *d_dict, uint32_t dict_len,
                                uint8_t *d_out, uint64_t out_room, bool allow_cut, StreamRun *run, uint64_t *needed)
{
    ChunkOpts o; o.start_bit = start_bit; o.d_dict = d_dict; o.dict_len = dict_len; o.allow_cut = allow_cut;
    ChunkInfo ci;
    uint64_t clen = 0, cused = 0;
    const int cr = inflate_chunked_dev(c, d_def, avail, d_out, out_room, &clen, &cused, o, &ci);
    if (cr < 0 && cr != ZNGAMD_BUF_ERROR) return cr;
    if (cr == ZNGAMD_BUF_ERROR) { *needed = clen; return ZNGAMD_BUF_ERROR; }
    if (cr == 0) { run->status = ci.ended ? ZA_I_END : ZA_I_INPUT; run->out_len = clen; run->in_bits = ci.end_bit; run->chunked = true; return ZNGAMD_OK; }
    ZaInfResult res;
    int r = inflate_serial_dev(c, d_def, avail, d_dict, dict_len, d_out, out_room, &res, start_bit);
    if (r) return r;
    run->chunked = false;
    if (res.status == ZA_I_OUTFULL) { *needed = 0; return ZNGAMD_BUF_ERROR; }
    if (res.status == ZA_I_INPUT && allow_cut) { run->status = ZA_I_INPUT; run->out_len = res.block_out; run->in_bits = res.block_bits; }   // the last block header entered
    else { run->status = res.status; run->out_len = res.out_len; run->in_bits = res.in_bits; }
    return ZNGAMD_OK;
}

// A window of a member whose units the writer indexed (zngamd_gz_state.index): the whole units inside the window, decoded side by
// side.  1 = done (*run says how far), 0 = not applicable here (the caller decodes the window without the index), < 0 = error.
static int decode_stream_prefix_indexed(zngamd_ctx *c, ZaFileIndex *ix, uint64_t out_total, const uint8_t *h_def, const uint8_t *d_def, uint64_t avail,
                                        const uint8_t *d_dict, uint32_t dict_len, uint8_t *d_out, uint64_t out_room, bool allow_cut,
                                        StreamRun *run, uint64_t *needed)
{
    if (!ix || ix->dead || ix->device != c->device) return 0;
    const size_t k0 = (size_t)(std::lower_bound(ix->cum_out.begin(), ix->cum_out.end(), out_total) - ix->cum_out.begin());
    if (k0 > ix->n || ix->cum_out[k0] != out_total) return 0;               // the reader does not stand at a unit's start
    size_t k1 = k0;
    while (k1 < ix->n && ix->cum_in[k1 + 1] - ix->cum_in[k0] <= avail && ix->cum_out[k1 + 1] - out_total <= out_room) k1++;
    if (k1 < ix->n && ix->cum_in[k1 + 1] - ix->cum_in[k0] <= avail && !allow_cut) {       // (room, not input, ended the run, and nothing may be left over)
        *needed = ix->cum_out[ix->n] - out_total; return ZNGAMD_BUF_ERROR;
    }
    uint64_t olen = 0;
    const uint64_t used = ix->cum_in[k1] - ix->cum_in[k0];
    if (k1 > k0) {
        const int r = inflate_units_core(c, d_def, used, ix->in_len.data() + k0, ix->out_len.data() + k0, (uint32_t)(k1 - k0),
                                         ix->d_rows + k0 * ZA_CIDX_STRIDE, d_dict, dict_len, d_out, out_room, &olen);
        // (nothing was handed out: the window is decoded again, the ordinary way -- also behind "invalid data", which a wrong index
        // entry looks like to the lane it sends into the middle of a code; real damage is then reported by the decoder that needs no index)
        if (r == ZNGAMD_E_INDEX || r == ZNGAMD_DATA_ERROR) { ix->dead = true; return 0; }
        if (r != ZNGAMD_STREAM_END) return r;
    }
    run->chunked = true; run->out_len = olen;
    if (k1 == ix->n) {
        // behind the last unit the writer closes the stream with an empty final block (03 00: gzip_ng_threaded.py:333)
        if (avail >= used + 2 && h_def[used] == 0x03 && h_def[used + 1] == 0x00) { run->status = ZA_I_END; run->in_bits = (used + 2) * 8ull; return 1; }
        if (avail >= used + 2) { ix->dead = true; if (k1 == k0) return 0; }  // something else follows: the rest without the index
    }
    run->status = ZA_I_INPUT; run->in_bits = used * 8ull;
    return 1;
}

static int stream_step(zngamd_ctx *c, zngamd_gz_state *st, const uint8_t *in, uint64_t in_len, uint64_t doff, bool last,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members, uint64_t *in_consumed)
{
    const uint64_t front = ZA_WIN + 64;                     // staging: [history][pad][window of the stream]
    int r = stage_in(c, in, in_len, front);
    if (r) return r;
    const uint32_t dl = st->window_len > ZA_WIN ? (uint32_t)ZA_WIN : st->window_len;
    if (dl) HIPCHK(c, hipMemcpyAsync(c->st_in.p, st->window, dl, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, c->st_out.ensure(out_cap + 64));
    StreamRun run; uint64_t needed = 0;
    r = 0;
    if (st->index && (st->start_bit & 7u) == 0u)
        r = decode_stream_prefix_indexed(c, (ZaFileIndex *)st->index, st->out_total, in + doff, c->st_in.p + front + doff, in_len - doff,
                                         c->st_in.p, dl, c->st_out.p, out_cap, !last, &run, &needed);
    if (r == 1) r = ZNGAMD_OK;
    else if (r == 0)
    r = decode_stream_prefix(c, c->st_in.p + front + doff, in_len - doff, st->start_bit & 7u, c->st_in.p, dl, c->st_out.p, out_cap, !last, &run, &needed);
    if (r == ZNGAMD_BUF_ERROR) { *out_len = needed > out_cap ? needed : out_cap; return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small"); }
    if (r) return r;
    return stream_finish(c, st, in, in_len, doff, last, run, dl, out, out_cap, out_len, n_members, in_consumed);
}

// What follows the decode of a piece of a member that is continued across windows (run: how far it got; the decoded bytes are
// at st_out): CRC fold, trailer check at the end of the member, hand-out, and the state the next window continues with.
static int stream_finish(zngamd_ctx *c, zngamd_gz_state *st, const uint8_t *in, uint64_t in_len, uint64_t doff, bool last, const StreamRun &run,
                         uint32_t dl, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members, uint64_t *in_consumed)
{
    int r;
    if (run.status != ZA_I_END && run.status != ZA_I_INPUT) { c->err = "invalid deflate data"; return map_status(run.status); }
    if (run.status == ZA_I_INPUT && last) {
        if (run.out_len) { const int rc_ = d2h_payload(c, out, c->st_out.p, run.out_len); if (rc_) return rc_; }
        *out_len = run.out_len; c->err = "gzip member did not end"; return ZNGAMD_E_GZ_TRUNC;
    }
    if (run.status == ZA_I_INPUT && run.out_len == 0 && run.in_bits <= (st->start_bit & 7u)) return ZNGAMD_OK;   // not one whole block yet
    uint32_t cnew = 0;
    r = checksum_dev(c, c->st_out.p, run.out_len, &cnew, nullptr);
    if (r) return r;
    const uint32_t crc = st->out_total ? zngamd_crc32_combine(st->crc, cnew, run.out_len) : cnew;
    if (run.status == ZA_I_END) {
        uint64_t cur = doff + ((run.in_bits + 7) >> 3);
        if (in_len - cur < 8) { if (last) return ZNGAMD_E_GZ_TRUNC; return ZNGAMD_OK; }      // trailer not in the window yet
        const uint32_t tc = in[cur] | (in[cur + 1] << 8) | (in[cur + 2] << 16) | ((uint32_t)in[cur + 3] << 24);
        const uint32_t tl = in[cur + 4] | (in[cur + 5] << 8) | (in[cur + 6] << 16) | ((uint32_t)in[cur + 7] << 24);
        if (run.out_len) { const int rc_ = d2h_payload(c, out, c->st_out.p, run.out_len); if (rc_) return rc_; }
        *out_len = run.out_len;
        if (tc != crc) { char b[96]; snprintf(b, sizeof b, "CRC check failed %u != %u", tc, crc); c->err = b; return ZNGAMD_E_GZ_CRC; }
        if (tl != (uint32_t)((st->out_total + run.out_len) & 0xFFFFFFFFull)) { c->err = "Incorrect length of data produced"; return ZNGAMD_E_GZ_LENGTH; }
        cur += 8;
        while (cur < in_len && in[cur] == 0) cur++;
        *in_consumed = cur;
        if (n_members) *n_members = 1;
        c->paths[run.chunked ? ZNGAMD_PATH_CHUNKED : ZNGAMD_PATH_SEQUENTIAL]++;
        st->in_member = 0; st->start_bit = 0; st->crc = 0; st->window_len = 0; st->out_total = 0;
        st->index = nullptr;                         // (the index was this member's; the handle stays the caller's)
        return ZNGAMD_OK;
    }
    // the member goes on: hand out the complete blocks, remember where and with what history to continue
    if (run.out_len) { const int rc_ = d2h_payload(c, out, c->st_out.p, run.out_len); if (rc_) return rc_; }
    if (run.out_len >= ZA_WIN) { memcpy(st->window, out + run.out_len - ZA_WIN, ZA_WIN); st->window_len = ZA_WIN; }
    else {
        const uint32_t keep = std::min<uint32_t>(dl, (uint32_t)(ZA_WIN - run.out_len));
        memmove(st->window, st->window + (dl - keep), keep);
        memcpy(st->window + keep, out, run.out_len);
        st->window_len = keep + (uint32_t)run.out_len;
    }
    st->crc = crc; st->out_total += run.out_len; st->start_bit = (uint32_t)(run.in_bits & 7u); st->in_member = 1;
    *out_len = run.out_len;
    *in_consumed = doff + (run.in_bits >> 3);
    return ZNGAMD_OK;
}

int zngamd_gunzip_stream(zngamd_ctx *c, zngamd_gz_state *st, const uint8_t *in, uint64_t in_len, int last, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_len, uint32_t *n_members, uint64_t *in_consumed)
try {
    if (!c || !st || (!in && in_len) || (!out && out_cap) || !out_len || !in_consumed) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    *out_len = 0; *in_consumed = 0;
    if (n_members) *n_members = 0;
    if (st->in_member) return stream_step(c, st, in, in_len, 0, last != 0, out, out_cap, out_len, n_members, in_consumed);
    int r = gunzip_impl(c, in, in_len, !last, out, out_cap, out_len, n_members, in_consumed, last ? nullptr : st, st->index);
    if (*in_consumed > 0 && !st->in_member) st->index = nullptr;      // (the index was the first member's, and that one is through)
    if (r != ZNGAMD_OK || last || *in_consumed > 0 || in_len == 0) return r;
    // not even the first member is complete in this window: start it and hand out the blocks that are
    uint64_t doff = 0; bool za = false; uint32_t hl = 0;
    r = parse_gzip_header(in, in_len, 0, &doff, &za, &hl);
    if (r == ZNGAMD_E_GZ_TRUNC) return ZNGAMD_OK;                      // the header itself is cut: more input first
    if (r) return r;
    if (hl) {
        int rs = stage_in(c, in, in_len);
        if (rs) return rs;
        uint32_t hc = 0;
        rs = checksum_dev(c, c->st_in.p, hl, &hc, nullptr);
        if (rs) return rs;
        const uint32_t want = in[hl] | (in[hl + 1] << 8);
        if ((hc & 0xFFFFu) != want) return ZNGAMD_E_GZ_HCRC;
    }
    st->in_member = 0; st->start_bit = 0; st->crc = 0; st->window_len = 0; st->out_total = 0;
    return stream_step(c, st, in, in_len, doff, false, out, out_cap, out_len, n_members, in_consumed);
} ZA_ABI_GUARD

int zngamd_gunzip_partial(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                          uint32_t *n_members, uint64_t *in_consumed)
try {
    if (!c || (!in && in_len) || (!out && out_cap) || !out_len || !in_consumed) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    return gunzip_impl(c, in, in_len, true, out, out_cap, out_len, n_members, in_consumed);
} ZA_ABI_GUARD

// ---- indexed member writer ---------------------------------------------------------------------
static int gzip_members_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t block_size, int level,
                            uint8_t *d_out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members)
{
    if (block_size == 0 || block_size > ZA_MAX_UNIT) return fail(c, ZNGAMD_E_ARG, "block_size must be 1..131072");
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    const uint64_t nb64 = in_len == 0 ? 1 : (in_len + block_size - 1) / block_size;
    if (nb64 > (1u << 26)) return fail(c, ZNGAMD_E_ARG, "too many members");
    const uint32_t nb = (uint32_t)nb64;
    std::vector<ZaUnit> hu(nb);
    for (uint32_t b = 0; b < nb; b++) {
        ZaUnit u; u.in_off = (uint64_t)b * block_size; u.in_len = (uint32_t)std::min<uint64_t>(block_size, in_len - u.in_off);
        u.dict_len = 0; u.flags = ZA_FLAG_FINAL | ZA_FLAG_FLATHDR; u.flags |= (uint32_t)za_seg_shift_for(u.in_len, u.flags) << 8; u.block = b; hu[b] = u;
    }
    HIPCHK(c, c->st_slots.ensure((size_t)nb * ZNGAMD_SLOT_STRIDE)); HIPCHK(c, c->st_len.ensure(nb)); HIPCHK(c, c->st_crc.ensure(nb));
    int r = deflate_units_dev(c, d_in, in_len, hu, level, c->st_slots.p, c->st_len.p, c->st_crc.p);
    if (r) return r;
    HIPCHK(c, c->st_off.ensure(nb));
    uint64_t total = 0;
    r = gather_dev(c, c->st_slots.p, c->st_len.p, nb, ZA_MEMBER_FIXED + 8, d_out, 0, out_cap, c->st_off.p, &total, false, c->units.p);
    if (r) return r;
    const int lv = level == -1 ? 6 : level;
    const uint8_t xfl = lv == 9 ? 2 : lv == 1 ? 4 : 0;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_assemble_members, dim3(nb), dim3(256), 0, c->stream, c->st_slots.p, (uint32_t)ZNGAMD_SLOT_STRIDE, c->st_len.p,
                         c->st_crc.p, c->cidx.p, c->units.p, c->st_off.p, d_out, xfl); }
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> st(nb);
    HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, nb * 4ull, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (uint32_t i = 0; i < nb; i++) if (st[i]) return fail(c, ZNGAMD_E_OVERFLOW, "unit overflowed its slot");
    *out_len = total;
    if (n_members) *n_members = nb;
    return ZNGAMD_OK;
}

int zngamd_gzip_members_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, uint32_t block_size, int level, void *d_out,
                            uint64_t out_cap, uint64_t *out_len, uint32_t *n_members)
try {
    if (!c || (!d_in && in_len) || !d_out || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return gzip_members_dev(c, (const uint8_t *)d_in, in_len, block_size, level, (uint8_t *)d_out, out_cap, out_len, n_members);
} ZA_ABI_GUARD

int zngamd_gzip_members(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t block_size, int level, uint8_t *out,
                        uint64_t out_cap, uint64_t *out_len)
try {
    if (!c || (!in && in_len) || !out || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    int r = stage_in(c, in, in_len);
    if (r) return r;
    const uint64_t nb = in_len == 0 ? 1 : (in_len + (block_size ? block_size : 1) - 1) / (block_size ? block_size : 1);
    const uint64_t bound = in_len + in_len / 32 + nb * (ZA_MEMBER_FIXED + 8 + 600);      // worst case stored + index + flat header
    HIPCHK(c, c->st_aux.ensure(bound));
    uint64_t total = 0;
    r = gzip_members_dev(c, c->st_in.p, in_len, block_size, level, c->st_aux.p, bound, &total, nullptr);
    if (r) return r;
    *out_len = total;
    if (total > out_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    if (total) { const int rc_ = d2h_payload(c, out, c->st_aux.p, total); if (rc_) return rc_; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- BGZF (za_bgzf.hip) --------------------------------------------------
// The BSIZE walk over a host buffer: no GPU, no context.  Like hop_bgzf above (which zngamd_gunzip keeps, with its own rules for
// when to hand a stream to the general reader), but with a verdict for every way the walk can end.
int zngamd_bgzf_scan(const uint8_t *in, uint64_t in_len, zngamd_bgzf_block *table, uint32_t max_blocks, uint32_t *n_blocks,
                     uint64_t *consumed, uint64_t *total_out)
{
    if ((!in && in_len) || !n_blocks || !consumed || !total_out) return ZNGAMD_E_ARG;
    auto le16 = [&](uint64_t o) { return (uint32_t)in[o] | ((uint32_t)in[o + 1] << 8); };
    auto le32 = [&](uint64_t o) { return (uint32_t)in[o] | ((uint32_t)in[o + 1] << 8) | ((uint32_t)in[o + 2] << 16) | ((uint32_t)in[o + 3] << 24); };
    static const uint8_t magic[4] = {0x1f, 0x8b, 8, 4};
    uint64_t pos = 0, outp = 0;
    uint32_t n = 0;
    int ret = ZNGAMD_OK;
    while (pos < in_len && (!table || n < max_blocks)) {
        const uint64_t left = in_len - pos;
        // what is there of the four fixed bytes decides between "not a block" and "the start of one"
        bool is_block = true;
        for (uint64_t i = 0; i < std::min<uint64_t>(left, 4); i++) if (in[pos + i] != magic[i]) is_block = false;
        if (!is_block) { ret = pos == 0 ? ZNGAMD_E_BGZF : ZNGAMD_DATA_ERROR; break; }
        if (left < 12) { if (n == 0) ret = ZNGAMD_E_BGZF; break; }                   // a cut header: the tail (nothing but a stump is no BGZF)
        const uint64_t end = pos + 12 + le16(pos + 10);                               // end of the extra field
        if (end > in_len) { if (n == 0) ret = ZNGAMD_DATA_ERROR; break; }
        long bsize = -1;
        bool bad = false;
        for (uint64_t cur = pos + 12; cur + 4 <= end;) {
            const uint32_t sl = le16(cur + 2);
            if (cur + 4 + sl > end) { bad = true; break; }
            if (in[cur] == 'B' && in[cur + 1] == 'C' && sl == 2) bsize = (long)le16(cur + 4);
            cur += 4 + sl;
        }
        if (bad) { ret = ZNGAMD_DATA_ERROR; break; }
        if (bsize < 0) { ret = pos == 0 ? ZNGAMD_E_BGZF : ZNGAMD_DATA_ERROR; break; }    // a gzip member without the 'B','C' subfield
        const uint64_t msize = (uint64_t)bsize + 1;
        if (msize < (end - pos) + 8) { ret = ZNGAMD_DATA_ERROR; break; }             // smaller than its own header and trailer
        // A block that runs past the buffer: the incomplete tail of a longer file once a complete block stands in front of it (what
        // hop_bgzf allows too); with none in front of it nothing vouches for this BSIZE
        if (msize > left) { if (n == 0) ret = ZNGAMD_DATA_ERROR; break; }
        const uint32_t isize = le32(pos + msize - 4);
        if (isize > 65536u) { ret = ZNGAMD_DATA_ERROR; break; }
        if (table) { zngamd_bgzf_block r; r.coffset = pos; r.uoffset = outp; r.csize = (uint32_t)msize; r.isize = isize; table[n] = r; }
        n++; pos += msize; outp += isize;
    }
    *n_blocks = n; *consumed = pos; *total_out = outp;
    return ret;
}

static int bgzf_compress_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, uint32_t block_size, int level, int eof, uint8_t *d_out,
                             uint64_t out_cap, uint64_t *out_len, ZaBgzfBlock *d_table, uint32_t *n_blocks)
{
    if (block_size == 0 || block_size > ZA_BGZF_MAX_IN) return fail(c, ZNGAMD_E_ARG, "block_size must be 1..65280");
    if (!zngamd_level_ok(level)) return fail(c, ZNGAMD_STREAM_ERROR, "Bad compression level");
    const uint64_t nb64 = (in_len + block_size - 1) / block_size;
    if (nb64 > (1u << 26)) return fail(c, ZNGAMD_E_ARG, "too many blocks");
    const uint32_t nb = (uint32_t)nb64;
    *out_len = 0;
    if (n_blocks) *n_blocks = 0;
    if (nb == 0 && !eof) return ZNGAMD_OK;
    uint64_t total = 0;
    uint64_t *d_total = (uint64_t *)c->d_small;
    if (nb) {
        std::vector<ZaUnit> hu(nb);
        for (uint32_t b = 0; b < nb; b++) {
            ZaUnit u; u.in_off = (uint64_t)b * block_size; u.in_len = (uint32_t)std::min<uint64_t>(block_size, in_len - u.in_off);
            u.dict_len = 0; u.flags = ZA_FLAG_FINAL; u.flags |= (uint32_t)za_seg_shift_for(u.in_len, u.flags) << 8; u.block = b; hu[b] = u;
        }
        HIPCHK(c, c->st_slots.ensure((size_t)nb * ZNGAMD_SLOT_STRIDE)); HIPCHK(c, c->st_len.ensure(nb)); HIPCHK(c, c->st_crc.ensure(nb));
        HIPCHK(c, c->bg_len.ensure(nb)); HIPCHK(c, c->st_off.ensure(nb));
        int r = deflate_units_dev(c, d_in, in_len, hu, level, c->st_slots.p, c->st_len.p, c->st_crc.p);
        if (r) return r;
        { ProfScope ps(c, ZNGAMD_K_GATHER);
          hipLaunchKernelGGL(za_k_bgzf_lengths, dim3((nb + 255u) / 256u), dim3(256), 0, c->stream, c->st_len.p, c->units.p, nb, c->bg_len.p);
          hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(nb <= 64 ? 64 : 1024), 0, c->stream, c->bg_len.p, nb, 0u, 0ull, c->st_off.p, d_total,
                             (const ZaUnit *)nullptr); }
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else HIPCHK(c, hipMemsetAsync(d_total, 0, 8, c->stream));
    const uint64_t need = total + (eof ? ZA_BGZF_EOF_BYTES : 0u);
    *out_len = need;
    if (need > out_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_assemble_bgzf, dim3(nb + (eof ? 1u : 0u)), dim3(256), 0, c->stream, d_in, c->st_slots.p, (uint32_t)ZNGAMD_SLOT_STRIDE,
                         c->st_len.p, c->st_crc.p, c->units.p, c->bg_len.p, c->st_off.p, d_total, nb, in_len, d_out, d_table); }
    HIPCHK(c, hipGetLastError());
    std::vector<uint32_t> st(nb);
    if (nb) HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, nb * 4ull, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (uint32_t i = 0; i < nb; i++) if (st[i]) return fail(c, ZNGAMD_E_OVERFLOW, "unit overflowed its slot");
    if (n_blocks) *n_blocks = nb + (eof ? 1u : 0u);
    return ZNGAMD_OK;
}

int zngamd_bgzf_compress_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, uint32_t block_size, int level, int eof, void *d_out,
                             uint64_t out_cap, uint64_t *out_len, zngamd_bgzf_block *d_table, uint32_t *n_blocks)
try {
    if (!c || (!d_in && in_len) || (!d_out && out_cap) || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    return bgzf_compress_dev(c, (const uint8_t *)d_in, in_len, block_size, level, eof, (uint8_t *)d_out, out_cap, out_len, (ZaBgzfBlock *)d_table, n_blocks);
} ZA_ABI_GUARD

int zngamd_bgzf_compress(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, uint32_t block_size, int level, int eof, uint8_t *out,
                         uint64_t out_cap, uint64_t *out_len, zngamd_bgzf_block *table, uint32_t max_blocks, uint32_t *n_blocks)
try {
    if (!c || (!in && in_len) || (!out && out_cap) || !out_len) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (block_size == 0 || block_size > ZA_BGZF_MAX_IN) return fail(c, ZNGAMD_E_ARG, "block_size must be 1..65280");
    int r = stage_in(c, in, in_len);
    if (r) return r;
    const uint64_t nb = (in_len + block_size - 1) / block_size;
    const uint64_t bound = in_len + in_len / 32 + nb * (ZA_BGZF_FIXED + 600) + ZA_BGZF_EOF_BYTES;      // (what the pipeline writes for a unit that does not compress, with room to spare)
    HIPCHK(c, c->st_aux.ensure(bound)); HIPCHK(c, c->bg_table.ensure(nb + 1));
    uint64_t total = 0; uint32_t rows = 0;
    r = bgzf_compress_dev(c, c->st_in.p, in_len, block_size, level, eof, c->st_aux.p, bound, &total, c->bg_table.p, &rows);
    *out_len = total;
    if (r) return r;
    if (n_blocks) *n_blocks = rows;
    if (total > out_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    if (table) {
        if (rows > max_blocks) return fail(c, ZNGAMD_BUF_ERROR, "block table too small");
        if (rows) HIPCHK(c, hipMemcpyAsync(table, c->bg_table.p, (size_t)rows * sizeof(ZaBgzfBlock), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (total) { const int rc_ = d2h_payload(c, out, c->st_aux.p, total); if (rc_) return rc_; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// Ranged reads: the blocks in ONE launch of the plain-member decoder (CRC-32 and ISIZE checked there, a status per block), then the
// slice kernel.  Nothing is copied to the host here.
static int bgzf_read_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members,
                         const ZaBgzfSlice *d_slices, uint32_t n_slices, uint8_t *d_scratch, uint64_t scratch_cap, uint8_t *d_out,
                         uint64_t out_cap, int32_t *d_status, int32_t *d_slice_status)
{
    if (n_members) {
        ProfScope ps(c, ZNGAMD_K_INFLATE);
        hipLaunchKernelGGL(za_k_inflate_serial_members, dim3(n_members), dim3(64), 0, c->stream, d_in, in_len, d_members, d_scratch, scratch_cap,
                           c->d_crc_table, c->d_x8k, d_status);
        c->bgzf_stats[0]++; c->bgzf_stats[1] += n_members;
    }
    if (n_slices) {
        ProfScope ps(c, ZNGAMD_K_GATHER);
        hipLaunchKernelGGL(za_k_slice_gather, dim3(n_slices), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, d_slices,
                           d_out, out_cap, d_slice_status);
        c->bgzf_stats[2] += n_slices;
    }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_bgzf_read_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                         const zngamd_bgzf_slice *d_slices, uint32_t n_slices, void *d_scratch, uint64_t scratch_cap, void *d_out,
                         uint64_t out_cap, int32_t *d_status, int32_t *d_slice_status)
try {
    if (!c || (n_members && (!d_in || !d_members || !d_status || (!d_scratch && scratch_cap))) ||
        (n_slices && (!d_slices || !d_slice_status || (!d_out && out_cap)))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_read_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, (const ZaBgzfSlice *)d_slices, n_slices,
                          (uint8_t *)d_scratch, scratch_cap, (uint8_t *)d_out, out_cap, d_status, d_slice_status);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_read(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                     const zngamd_bgzf_slice *slices, uint32_t n_slices, uint8_t *out, uint64_t out_cap, int32_t *status, int32_t *slice_status)
try {
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (n_slices && (!slices || !slice_status)) || (!out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    // the decoded scratch is as long as the members say; a member that lies outside the input gets its verdict from the kernel
    uint64_t scratch = 0;
    for (uint32_t i = 0; i < n_members; i++) {
        if (members[i].out_off > (1ull << 40)) return fail(c, ZNGAMD_E_ARG, "member table: output offset out of range");
        scratch = std::max<uint64_t>(scratch, members[i].out_off + members[i].out_len);
    }
    int r = stage_in(c, in, in_len);
    if (r) return r;
    HIPCHK(c, c->st_out.ensure(scratch + 64)); HIPCHK(c, c->bg_out.ensure(out_cap + 64));
    HIPCHK(c, c->members.ensure(n_members + 1)); HIPCHK(c, c->mstatus.ensure(n_members + 1));
    HIPCHK(c, c->bg_slices.ensure(n_slices + 1)); HIPCHK(c, c->bg_sstat.ensure(n_slices + 1));
    if (n_members) HIPCHK(c, hipMemcpyAsync(c->members.p, members, (size_t)n_members * sizeof(ZaMember), hipMemcpyHostToDevice, c->stream));
    if (n_slices) HIPCHK(c, hipMemcpyAsync(c->bg_slices.p, slices, (size_t)n_slices * sizeof(ZaBgzfSlice), hipMemcpyHostToDevice, c->stream));
    r = bgzf_read_dev(c, c->st_in.p, in_len, c->members.p, n_members, c->bg_slices.p, n_slices, c->st_out.p, scratch, c->bg_out.p, out_cap,
                      c->mstatus.p, c->bg_sstat.p);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_slices) HIPCHK(c, hipMemcpyAsync(slice_status, c->bg_sstat.p, (size_t)n_slices * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the uploads read the caller's pageable tables: drained before it may touch them again)
    // only the packed result crosses the link: as far as the slices reach
    uint64_t used = 0;
    for (uint32_t i = 0; i < n_slices; i++)
        if (slice_status[i] != ZA_SLICE_TABLE) used = std::max<uint64_t>(used, slices[i].dst_off + slices[i].len);
    if (used) { const int rc_ = d2h_payload(c, out, c->bg_out.p, std::min(used, out_cap)); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- lines: the decode launch of the ranged reads, then the count kernel or the select kernel on the decoded
// scratch.  Nothing here copies decoded bytes to the host.
static void bgzf_decode_launch(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members, uint8_t *d_scratch,
                               uint64_t scratch_cap, int32_t *d_status)
{
    ProfScope ps(c, ZNGAMD_K_INFLATE);
    hipLaunchKernelGGL(za_k_inflate_serial_members, dim3(n_members), dim3(64), 0, c->stream, d_in, in_len, d_members, d_scratch, scratch_cap,
                       c->d_crc_table, c->d_x8k, d_status);
    c->bgzf_stats[0]++; c->bgzf_stats[1] += n_members;
}

static int bgzf_count_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members, uint32_t delim,
                          uint8_t *d_scratch, uint64_t scratch_cap, int32_t *d_status, ZaBgzfCount *d_rows)
{
    if (!n_members) return ZNGAMD_OK;
    bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_bgzf_count, dim3(n_members), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, delim, d_rows); }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

static int bgzf_positions_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members,
                              const ZaBgzfPos *d_queries, uint32_t n_queries, uint32_t delim, uint8_t *d_scratch, uint64_t scratch_cap,
                              int32_t *d_status, uint64_t *d_pos, int32_t *d_pos_status)
{
    if (n_members) bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
    if (n_queries) {
        ProfScope ps(c, ZNGAMD_K_GATHER);
        hipLaunchKernelGGL(za_k_bgzf_select, dim3(n_queries), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, d_queries,
                           delim, d_pos, d_pos_status);
    }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

// decode, select (two positions per range), pairs into slices, scan, [the host waits for the packed total], gather, verdicts
static int bgzf_read_lines_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members,
                               const ZaBgzfPos *d_ranges, uint32_t n_ranges, uint32_t delim, uint8_t *d_scratch, uint64_t scratch_cap,
                               uint8_t *d_out, uint64_t out_cap, bool own_out, uint64_t *out_len, uint32_t *d_range_len, int32_t *d_status,
                               int32_t *d_range_status)
{
    *out_len = 0;
    if (n_ranges >= (1u << 30)) return fail(c, ZNGAMD_E_ARG, "too many ranges");      // (two workgroups of the select launch per range)
    if (!n_ranges) {
        if (n_members) bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
        HIPCHK(c, hipGetLastError());
        return ZNGAMD_OK;
    }
    HIPCHK(c, c->bg_pos.ensure(2ull * n_ranges)); HIPCHK(c, c->bg_pstat.ensure(2ull * n_ranges)); HIPCHK(c, c->bg_pre.ensure(n_ranges));
    HIPCHK(c, c->bg_slices.ensure(n_ranges + 1)); HIPCHK(c, c->st_off.ensure(n_ranges));
    int r = bgzf_positions_dev(c, d_in, in_len, d_members, n_members, d_ranges, 2u * n_ranges, delim, d_scratch, scratch_cap, d_status, c->bg_pos.p,
                               c->bg_pstat.p);
    if (r) return r;
    uint64_t *d_total = (uint64_t *)c->d_small;
    uint64_t total = 0;
    const uint32_t grid = (n_ranges + 255u) / 256u;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_bgzf_line_slices, dim3(grid), dim3(256), 0, c->stream, c->bg_pos.p, c->bg_pstat.p, n_ranges, c->bg_slices.p, d_range_len,
                         c->bg_pre.p);
      hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(n_ranges <= 64 ? 64 : 1024), 0, c->stream, d_range_len, n_ranges, 0u, 0ull, c->st_off.p, d_total,
                         (const ZaUnit *)nullptr);
      hipLaunchKernelGGL(za_k_bgzf_place, dim3(grid), dim3(256), 0, c->stream, c->st_off.p, n_ranges, c->bg_slices.p); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out_len = total;
    if (own_out) { HIPCHK(c, c->bg_out.ensure(total + 64)); d_out = c->bg_out.p; }      // (the host form: the packed result is as long as the lines are)
    else if (total > out_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_slice_gather, dim3(n_ranges), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, c->bg_slices.p,
                         d_out, total, d_range_status);
      hipLaunchKernelGGL(za_k_bgzf_line_verdicts, dim3(grid), dim3(256), 0, c->stream, c->bg_pre.p, n_ranges, d_range_status); }
    c->bgzf_stats[2] += n_ranges;
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

// host forms: the member table decides the scratch; a row whose offsets could wrap the kernels' sums is refused here
static int bgzf_host_scratch(zngamd_ctx *c, const zngamd_member *members, uint32_t n_members, uint64_t *scratch)
{
    uint64_t need = 0;
    for (uint32_t i = 0; i < n_members; i++) {
        if (members[i].out_off > (1ull << 40)) return fail(c, ZNGAMD_E_ARG, "member table: output offset out of range");
        if (members[i].in_off > (1ull << 48) || members[i].in_len > (1ull << 48)) return fail(c, ZNGAMD_E_ARG, "member table: input offset out of range");
        need = std::max<uint64_t>(need, members[i].out_off + members[i].out_len);
    }
    *scratch = need;
    return ZNGAMD_OK;
}

static int bgzf_host_stage(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t *scratch)
{
    int r = bgzf_host_scratch(c, members, n_members, scratch);
    if (r) return r;
    r = stage_in(c, in, in_len);
    if (r) return r;
    HIPCHK(c, c->st_out.ensure(*scratch + 64)); HIPCHK(c, c->members.ensure(n_members + 1)); HIPCHK(c, c->mstatus.ensure(n_members + 1));
    if (n_members) HIPCHK(c, hipMemcpyAsync(c->members.p, members, (size_t)n_members * sizeof(ZaMember), hipMemcpyHostToDevice, c->stream));
    return ZNGAMD_OK;
}

int zngamd_bgzf_count_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, int delim,
                          void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_count_row *d_rows)
try {
    if (!c || delim < 0 || delim > 255 || (n_members && (!d_in || !d_members || !d_status || !d_rows || (!d_scratch && scratch_cap)))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_count_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, (uint32_t)delim, (uint8_t *)d_scratch, scratch_cap,
                           d_status, (ZaBgzfCount *)d_rows);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_count(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, int delim,
                      int32_t *status, zngamd_bgzf_count_row *rows)
try {
    if (!c || delim < 0 || delim > 255 || (!in && in_len) || (n_members && (!members || !status || !rows))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    HIPCHK(c, c->bg_rows.ensure(n_members + 1));
    r = bgzf_count_dev(c, c->st_in.p, in_len, c->members.p, n_members, (uint32_t)delim, c->st_out.p, scratch, c->mstatus.p, c->bg_rows.p);
    if (r) return r;
    if (n_members) {
        HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(rows, c->bg_rows.p, (size_t)n_members * sizeof(ZaBgzfCount), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_line_positions_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                   const zngamd_bgzf_pos *d_queries, uint32_t n_queries, int delim, void *d_scratch, uint64_t scratch_cap,
                                   int32_t *d_status, uint64_t *d_pos, int32_t *d_pos_status)
try {
    if (!c || delim < 0 || delim > 255 || (n_members && (!d_in || !d_members || !d_status || (!d_scratch && scratch_cap))) ||
        (n_queries && (!d_queries || !d_pos || !d_pos_status))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_positions_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, (const ZaBgzfPos *)d_queries, n_queries,
                               (uint32_t)delim, (uint8_t *)d_scratch, scratch_cap, d_status, d_pos, d_pos_status);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_line_positions(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                               const zngamd_bgzf_pos *queries, uint32_t n_queries, int delim, int32_t *status, uint64_t *pos, int32_t *pos_status)
try {
    if (!c || delim < 0 || delim > 255 || (!in && in_len) || (n_members && (!members || !status)) || (n_queries && (!queries || !pos || !pos_status)))
        return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    HIPCHK(c, c->bg_q.ensure(n_queries + 1)); HIPCHK(c, c->bg_pos.ensure(n_queries + 1)); HIPCHK(c, c->bg_pstat.ensure(n_queries + 1));
    if (n_queries) HIPCHK(c, hipMemcpyAsync(c->bg_q.p, queries, (size_t)n_queries * sizeof(ZaBgzfPos), hipMemcpyHostToDevice, c->stream));
    r = bgzf_positions_dev(c, c->st_in.p, in_len, c->members.p, n_members, c->bg_q.p, n_queries, (uint32_t)delim, c->st_out.p, scratch, c->mstatus.p,
                           c->bg_pos.p, c->bg_pstat.p);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_queries) {
        HIPCHK(c, hipMemcpyAsync(pos, c->bg_pos.p, (size_t)n_queries * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(pos_status, c->bg_pstat.p, (size_t)n_queries * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_read_lines_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                               const zngamd_bgzf_line_range *d_ranges, uint32_t n_ranges, int delim, void *d_scratch, uint64_t scratch_cap,
                               void *d_out, uint64_t out_cap, uint64_t *out_len, uint32_t *d_range_len, int32_t *d_status, int32_t *d_range_status)
try {
    if (!c || !out_len || delim < 0 || delim > 255 || (n_members && (!d_in || !d_members || !d_status || (!d_scratch && scratch_cap))) ||
        (n_ranges && (!d_ranges || !d_range_len || !d_range_status || (!d_out && out_cap)))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_read_lines_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, (const ZaBgzfPos *)d_ranges, n_ranges,
                                (uint32_t)delim, (uint8_t *)d_scratch, scratch_cap, (uint8_t *)d_out, out_cap, false, out_len, d_range_len, d_status,
                                d_range_status);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_read_lines(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                           const zngamd_bgzf_line_range *ranges, uint32_t n_ranges, int delim, uint8_t *out, uint64_t out_cap,
                           zngamd_alloc_fn alloc, void *user, uint64_t *out_len, uint32_t *range_len, int32_t *status, int32_t *range_status)
try {
    if (!c || !out_len || delim < 0 || delim > 255 || (!in && in_len) || (n_members && (!members || !status)) ||
        (n_ranges && (!ranges || !range_len || !range_status)) || (!out && out_cap) || (out && alloc)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    HIPCHK(c, c->bg_q.ensure(2ull * n_ranges + 2)); HIPCHK(c, c->bg_rlen.ensure(n_ranges + 1)); HIPCHK(c, c->bg_sstat.ensure(n_ranges + 1));
    if (n_ranges) HIPCHK(c, hipMemcpyAsync(c->bg_q.p, ranges, (size_t)n_ranges * 2 * sizeof(ZaBgzfPos), hipMemcpyHostToDevice, c->stream));
    r = bgzf_read_lines_dev(c, c->st_in.p, in_len, c->members.p, n_members, c->bg_q.p, n_ranges, (uint32_t)delim, c->st_out.p, scratch, nullptr, 0, true,
                            out_len, c->bg_rlen.p, c->mstatus.p, c->bg_sstat.p);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_ranges) {
        HIPCHK(c, hipMemcpyAsync(range_len, c->bg_rlen.p, (size_t)n_ranges * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(range_status, c->bg_sstat.p, (size_t)n_ranges * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (alloc) {                                          // the size is known: the caller's memory is asked for now
        if (!*out_len) return ZNGAMD_OK;
        out = (uint8_t *)alloc(user, *out_len);
        if (!out) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned no memory");
    } else if (*out_len > out_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");      // (lengths and verdicts are there; only the lines are not)
    if (*out_len) { const int rc_ = d2h_payload(c, out, c->bg_out.p, *out_len); if (rc_) return rc_; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- lines by content (za_grep.hip)
// The patterns as the caller gave them: judged on the host, before a context is touched or anything is launched.
// max_mismatch: at most ZNGAMD_BGZF_GREP_MAX_MISMATCH and less than the shortest pattern's length.
static bool grep_patterns_ok(const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim,
                             uint32_t max_mismatch)
{
    if (!patterns || !table || n_patterns < 1 || n_patterns > ZNGAMD_BGZF_GREP_MAX_PATTERNS || delim < 0 || delim > 255 ||
        max_mismatch > ZNGAMD_BGZF_GREP_MAX_MISMATCH) return false;
    for (uint32_t i = 0; i < n_patterns; i++) {
        const uint32_t off = table[i].off, len = table[i].len;
        if (len < 1 || len > ZNGAMD_BGZF_GREP_MAX_PATTERN || off > patterns_len || patterns_len - off < len || max_mismatch >= len) return false;
        if (memchr(patterns + off, delim, len)) return false;
    }
    return true;
}

#define ZA_GREP_PAR_TABLE (ZA_GREP_PAIR_WORDS * 4u)                                // the parameter block: prefilter bits, pattern table, patterns
#define ZA_GREP_PAR_BLOB  (ZA_GREP_PAR_TABLE + ZA_GREP_MAX_PAT * (uint32_t)sizeof(ZaGrepPat))
#define ZA_GREP_APAR_WORDS (ZA_GREP_MAX_PAT * (uint32_t)sizeof(ZaGrepPat))         // with mismatches: pattern table, padded patterns

// the parameter block of za_k_grep_mark_approx and za_k_grep_classify: the table {first dword, length}, then every pattern padded with zeros to whole dwords
static void grep_approx_params(std::vector<uint8_t> &par, const uint8_t *patterns, const zngamd_bgzf_pattern *table, uint32_t n_patterns)
{
    size_t nwords = 0;
    for (uint32_t i = 0; i < n_patterns; i++) nwords += (table[i].len + 3u) / 4u;
    par.assign(ZA_GREP_APAR_WORDS + nwords * 4u, 0);
    ZaGrepPat *pt = (ZaGrepPat *)par.data();
    uint32_t at = 0;
    for (uint32_t i = 0; i < n_patterns; i++) {
        pt[i].off = at; pt[i].len = table[i].len;
        memcpy(par.data() + ZA_GREP_APAR_WORDS + (size_t)at * 4u, patterns + table[i].off, table[i].len);
        at += (table[i].len + 3u) / 4u;
    }
}

// The window a content call works on, as every driver below takes it: the compressed input and its member rows, the range of the text,
// the scratch the members decode to and their status words.  And where a call's rows and bytes go: the caller's device buffers, or
// (own: the host form) the context's, as long as the totals say.
struct BgzfWindow { const uint8_t *d_in; uint64_t in_len; const ZaMember *d_members; uint32_t n_members; uint64_t text_off, text_end; uint32_t delim;
                    uint8_t *d_scratch; uint64_t scratch_cap; int32_t *d_status; };
struct BgzfDest { ZaGrepRow *d_rows; uint64_t rows_cap; uint8_t *d_out; uint64_t out_cap; bool own; };

// The window of a _dev form, out of the caller's device pointers.  -> false: a pointer that every _dev form needs is missing.
static bool bgzf_dev_window(BgzfWindow *w, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off, uint64_t text_end,
                            int delim, void *d_scratch, uint64_t scratch_cap, int32_t *d_status)
{
    if ((n_members && (!d_in || !d_members || !d_status)) || (!d_scratch && scratch_cap)) return false;
    *w = {(const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, text_off, text_end, (uint32_t)delim, (uint8_t *)d_scratch, scratch_cap, d_status};
    return true;
}

// The tail of a _dev form: the stream is waited for.  rows_short: the caller's rows_cap did not hold the rows -- an error, unless a
// record was bad: then there are no rows to miss, the code is OK and the totals name the record.
static int bgzf_dev_finish(zngamd_ctx *c, bool rows_short = false, bool bad = false)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (rows_short && !bad) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    return ZNGAMD_OK;
}

// The window of a host form: the input and its member rows are staged, the window lies over the context's buffers.
static int bgzf_host_window(zngamd_ctx *c, BgzfWindow *w, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                            uint64_t text_end, int delim)
{
    uint64_t scratch = 0;
    const int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    *w = {c->st_in.p, in_len, c->members.p, n_members, text_off, text_end, (uint32_t)delim, c->st_out.p, scratch, c->mstatus.p};
    return ZNGAMD_OK;
}

// the members' status words to the caller, and the stream is waited for
static int bgzf_host_status(zngamd_ctx *c, int32_t *status, uint32_t n_members)
{
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
}

// The `seen` rows of row_bytes each that a host form's call left in d_rows, to the caller.  The size is known, so the caller's memory is
// asked for now; without an allocator rows_cap must hold them.
static int bgzf_host_rows(zngamd_ctx *c, zngamd_alloc_fn alloc, void *user, void *rows, uint64_t rows_cap, const void *d_rows, uint64_t seen, size_t row_bytes)
{
    if (alloc) {
        rows = alloc(user, seen * row_bytes);
        if (!rows) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned NULL");
    } else if (seen > rows_cap) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    HIPCHK(c, hipMemcpyAsync(rows, d_rows, (size_t)seen * row_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
}

// [the host waits for the totals]: the launches so far are judged, and `bytes` bytes of d_tot come to `totals`
static int bgzf_totals_read(zngamd_ctx *c, void *totals, const void *d_tot, size_t bytes)
{
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(totals, d_tot, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
}

// the grid of a kernel that takes a WAVE per record: four records to a workgroup, at most per_cu workgroups per CU -- beyond that a wave
// walks on to its next record
static uint32_t bgzf_wave_grid(const zngamd_ctx *c, uint64_t nrec, uint32_t per_cu)
{
    const uint64_t slots = (uint64_t)std::max<uint32_t>(c->search_slots, 1u) * per_cu;
    return (uint32_t)std::min<uint64_t>((nrec + 3u) / 4u, slots);
}

// decode, cover, mark (max_mismatch 0: za_k_grep_mark; more: za_k_grep_mark_approx), scan, and the host waits for the scan's totals: the first `totals_len` bytes of ZaGrepTotals go to `totals`.
// After it every tile has its bits, its summary and its carry (gp_bits, gp_tiles, gp_carry), unless covered is 0.
// marks = false (with max_mismatch 0): the delimiters alone -- za_k_grep_mark with an empty prefilter and no pattern, so no line matches.
static int bgzf_grep_lines_pass(zngamd_ctx *c, const BgzfWindow &w, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table,
                                uint32_t n_patterns, uint32_t flags, uint32_t max_mismatch, uint64_t line_base, void *totals, size_t totals_len, bool marks = true)
{
    if (w.text_off > w.text_end || w.text_end > w.scratch_cap) return fail(c, ZNGAMD_E_ARG, "the text lies outside the scratch");
    if (w.text_end - w.text_off >= (1ull << 32)) return fail(c, ZNGAMD_E_ARG, "a text of 4 GiB or more");
    const uint64_t tile0 = w.text_off / ZA_GREP_TILE;
    const uint32_t ntiles = w.text_end > w.text_off ? (uint32_t)((w.text_end - 1ull) / ZA_GREP_TILE - tile0 + 1ull) : 0u;
    std::vector<uint8_t> &par = c->gp_host;
    if (!max_mismatch) {
        // the parameter block: a bit per pair of bytes that opens a pattern (a one-byte pattern: every pair with that first byte)
        par.assign((size_t)ZA_GREP_PAR_BLOB + patterns_len + 1u, 0);
        uint32_t *pairs = (uint32_t *)par.data();
        for (uint32_t i = 0; i < (marks ? n_patterns : 0u); i++) {
            const uint8_t *p = patterns + table[i].off;
            if (table[i].len == 1) for (uint32_t b = 0; b < 256u; b++) { const uint32_t pr = p[0] | b << 8; pairs[pr >> 5] |= 1u << (pr & 31u); }
            else { const uint32_t pr = p[0] | (uint32_t)p[1] << 8; pairs[pr >> 5] |= 1u << (pr & 31u); }
        }
        memcpy(par.data() + ZA_GREP_PAR_TABLE, table, (size_t)n_patterns * sizeof(ZaGrepPat));
        memcpy(par.data() + ZA_GREP_PAR_BLOB, patterns, patterns_len);
    } else grep_approx_params(par, patterns, table, n_patterns);
    HIPCHK(c, c->gp_par.ensure(par.size())); HIPCHK(c, c->gp_bits.ensure((size_t)ntiles * 256u + 1u)); HIPCHK(c, c->gp_tiles.ensure(ntiles + 1u));
    HIPCHK(c, c->gp_carry.ensure(ntiles + 1u));
    HIPCHK(c, hipMemcpyAsync(c->gp_par.p, par.data(), par.size(), hipMemcpyHostToDevice, c->stream));
    ZaGrepTotals *d_tot = (ZaGrepTotals *)c->d_small;
    unsigned long long *d_cover = (unsigned long long *)((uint8_t *)c->d_small + 64);
    HIPCHK(c, hipMemsetAsync(d_cover, 0, 16, c->stream));
    if (w.n_members) bgzf_decode_launch(c, w.d_in, w.in_len, w.d_members, w.n_members, w.d_scratch, w.scratch_cap, w.d_status);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      if (w.n_members) hipLaunchKernelGGL(za_k_grep_cover, dim3((w.n_members + 255u) / 256u), dim3(256), 0, c->stream, w.d_members, w.d_status, w.n_members,
                                          w.scratch_cap, w.text_off, w.text_end, d_cover);
      if (ntiles && !max_mismatch)
          hipLaunchKernelGGL(za_k_grep_mark, dim3(ntiles), dim3(256), 0, c->stream, w.d_scratch, w.scratch_cap, w.text_off, w.text_end, tile0,
                             (const uint32_t *)c->gp_par.p, (const ZaGrepPat *)(c->gp_par.p + ZA_GREP_PAR_TABLE), c->gp_par.p + ZA_GREP_PAR_BLOB,
                             marks ? n_patterns : 0u, w.delim, flags, c->gp_bits.p, c->gp_tiles.p);
      else if (ntiles)
          hipLaunchKernelGGL(za_k_grep_mark_approx, dim3(ntiles), dim3(256), 0, c->stream, w.d_scratch, w.scratch_cap, w.text_off, w.text_end, tile0,
                             (const ZaGrepPat *)c->gp_par.p, (const uint32_t *)(c->gp_par.p + ZA_GREP_APAR_WORDS), n_patterns, w.delim, flags, max_mismatch,
                             c->gp_bits.p, c->gp_tiles.p);
      hipLaunchKernelGGL(za_k_grep_scan, dim3(1), dim3(ZA_GREP_SCAN_THREADS), 0, c->stream, c->gp_tiles.p, ntiles, tile0, w.text_off, w.text_end, flags, line_base,
                         d_cover, c->gp_carry.p, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, totals_len);
}

// offsets, place, gather: the n rows' bytes packed into d_out in the order of the rows (gp_lens holds their lengths)
static void bgzf_grep_pack(zngamd_ctx *c, const BgzfWindow &w, const ZaGrepRow *d_rows, uint64_t n, uint8_t *d_out, uint64_t bytes)
{
    uint64_t *d_bytes = (uint64_t *)((uint8_t *)c->d_small + 128);
    hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(n <= 64 ? 64 : 1024), 0, c->stream, c->gp_lens.p, (uint32_t)n, 0u, 0ull, c->st_off.p, d_bytes,
                       (const ZaUnit *)nullptr);
    hipLaunchKernelGGL(za_k_grep_place, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, c->stream, d_rows, c->st_off.p, n, c->bg_slices.p);
    hipLaunchKernelGGL(za_k_slice_gather, dim3((uint32_t)n), dim3(256), 0, c->stream, w.d_scratch, w.scratch_cap, w.d_members, w.d_status, w.n_members,
                       c->bg_slices.p, d_out, bytes, c->bg_sstat.p);
}

// n rows and `bytes` bytes are about to be written: the context's buffers are made to hold them and d names them (own), or the
// caller's must.  The host has read the totals, so a refusal writes nothing.
static int bgzf_dest_ready(zngamd_ctx *c, BgzfDest &d, uint64_t n, uint64_t bytes)
{
    if (d.own) {
        HIPCHK(c, c->gp_rows.ensure(n)); HIPCHK(c, c->bg_out.ensure(bytes + 64));
        d.d_rows = c->gp_rows.p; d.rows_cap = n; d.d_out = c->bg_out.p; d.out_cap = bytes;
    } else if (n > d.rows_cap || bytes > d.out_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    return ZNGAMD_OK;
}

extern "C++" {
// The totals area of a record call in buf: the call's totals struct, then n_bad fault words.  The struct is zeroed, a fault word is all
// ones as long as no record has the fault.
template <typename Totals>
static int bgzf_totals_area(zngamd_ctx *c, DevBuf<unsigned long long> &buf, uint32_t n_bad, Totals **d_tot, unsigned long long **d_bad)
{
    constexpr size_t TOT_WORDS = sizeof(Totals) / 8u;
    HIPCHK(c, buf.ensure(TOT_WORDS + n_bad));
    *d_tot = (Totals *)buf.p; *d_bad = buf.p + TOT_WORDS;
    HIPCHK(c, hipMemsetAsync(buf.p, 0, TOT_WORDS * 8u, c->stream));
    HIPCHK(c, hipMemsetAsync(*d_bad, 0xFF, n_bad * 8u, c->stream));
    return ZNGAMD_OK;
}

// Where a call's nrec rows go.  own: buf, the context's, made to hold them; otherwise the caller's *d_rows when rows_cap holds them, and
// nowhere (*rows_short) when it does not.
template <typename Row>
static int bgzf_rows_dest(zngamd_ctx *c, DevBuf<Row> &buf, uint64_t nrec, bool own, Row **d_rows, uint64_t rows_cap, bool *rows_short)
{
    if (own) { HIPCHK(c, buf.ensure(nrec)); *d_rows = buf.p; }
    else if (rows_cap < nrec) { *rows_short = true; *d_rows = nullptr; }
    return ZNGAMD_OK;
}

// The last step of the four drivers below, once the host has read the totals: the destination, then emit(rows) -- the launch that
// writes the n rows and their lengths (gp_lens) -- and the pack.
template <typename Emit>
static int bgzf_pack_rows(zngamd_ctx *c, const BgzfWindow &w, BgzfDest d, uint64_t n, uint64_t bytes, Emit emit)
{
    const int r = bgzf_dest_ready(c, d, n, bytes);
    if (r) return r;
    HIPCHK(c, c->gp_lens.ensure(n)); HIPCHK(c, c->st_off.ensure(n)); HIPCHK(c, c->bg_slices.ensure(n + 1)); HIPCHK(c, c->bg_sstat.ensure(n + 1));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      emit(d.d_rows);
      bgzf_grep_pack(c, w, d.d_rows, n, d.d_out, bytes); }
    c->bgzf_stats[2] += n;
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

// The last step of the four host forms: the n rows (gp_rows) and `bytes` bytes (bg_out) to the caller.  The sizes are known, so the
// caller's memory is asked for now, rows first, then bytes; without an allocator its buffers must hold them.  head_ok: what the call
// site asked for in front of the rows is there (classify's class rows), and head() starts its download; rows_too = false: that alone.
template <typename Head>
static int bgzf_host_fetch(zngamd_ctx *c, zngamd_alloc_fn alloc, void *user, uint64_t n, uint64_t bytes, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out,
                           uint64_t out_cap, bool head_ok, bool rows_too, Head head)
{
    if (alloc) {
        if (rows_too) { rows = head_ok ? (zngamd_bgzf_grep_row *)alloc(user, n * sizeof(ZaGrepRow)) : nullptr; out = rows ? (uint8_t *)alloc(user, bytes) : nullptr; }
        if (!head_ok || (rows_too && (!rows || !out))) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned no memory");
    } else if (!head_ok || (rows_too && (n > rows_cap || bytes > out_cap))) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    const int r = head();
    if (r) return r;
    if (rows_too) HIPCHK(c, hipMemcpyAsync(rows, c->gp_rows.p, (size_t)n * sizeof(ZaGrepRow), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return rows_too ? d2h_payload(c, out, c->bg_out.p, bytes) : ZNGAMD_OK;
}
static int bgzf_host_fetch(zngamd_ctx *c, zngamd_alloc_fn alloc, void *user, uint64_t n, uint64_t bytes, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out,
                           uint64_t out_cap)
{
    return bgzf_host_fetch(c, alloc, user, n, bytes, rows, rows_cap, out, out_cap, true, true, [] { return ZNGAMD_OK; });
}
}  // extern "C++"

// the lines pass, emit, pack
static int bgzf_grep_dev(zngamd_ctx *c, const BgzfWindow &w, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                         uint32_t flags, uint32_t max_mismatch, uint64_t line_base, const BgzfDest &dst, zngamd_bgzf_grep_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    const int r = bgzf_grep_lines_pass(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, line_base, totals, sizeof *totals);
    if (r) return r;
    const uint64_t tile0 = w.text_off / ZA_GREP_TILE;
    const uint32_t ntiles = w.text_end > w.text_off ? (uint32_t)((w.text_end - 1ull) / ZA_GREP_TILE - tile0 + 1ull) : 0u;
    const ZaGrepTotals *d_tot = (const ZaGrepTotals *)c->d_small;
    totals->reserved = 0;
    if (!totals->covered || (flags & ZNGAMD_BGZF_GREP_COUNT_ONLY) || !totals->matched) return ZNGAMD_OK;
    const uint64_t n = totals->matched;
    return bgzf_pack_rows(c, w, dst, n, totals->bytes, [&](ZaGrepRow *d_rows) {
        hipLaunchKernelGGL(za_k_grep_emit, dim3(ntiles), dim3(256), 0, c->stream, c->gp_bits.p, c->gp_tiles.p, c->gp_carry.p, d_tot, tile0, line_base, w.text_end,
                           d_rows, n, c->gp_lens.p); });
}

int zngamd_bgzf_grep_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                         uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                         int delim, uint32_t flags, uint64_t line_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status,
                         zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap, zngamd_bgzf_grep_totals *totals)
{
    return zngamd_bgzf_grep_approx_dev(c, d_in, in_len, d_members, n_members, text_off, text_end, patterns, patterns_len, table, n_patterns, delim, flags, 0,
                                       line_base, d_scratch, scratch_cap, d_status, d_rows, rows_cap, d_out, out_cap, totals);
}

// the exact call is this one with max_mismatch = 0
int zngamd_bgzf_grep_approx_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                                int delim, uint32_t flags, uint32_t max_mismatch, uint64_t line_base, void *d_scratch, uint64_t scratch_cap,
                                int32_t *d_status, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                zngamd_bgzf_grep_totals *totals)
try {
    if (!grep_patterns_ok(patterns, patterns_len, table, n_patterns, delim, max_mismatch)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !totals || (flags & ~15u) || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) ||
        (!d_rows && rows_cap) || (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_grep_dev(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, line_base,
                          {(ZaGrepRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false}, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_grep(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                     uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim,
                     uint32_t flags, uint64_t line_base, int32_t *status, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap,
                     zngamd_alloc_fn alloc, void *user, zngamd_bgzf_grep_totals *totals)
{
    return zngamd_bgzf_grep_approx(c, in, in_len, members, n_members, text_off, text_end, patterns, patterns_len, table, n_patterns, delim, flags, 0,
                                   line_base, status, rows, rows_cap, out, out_cap, alloc, user, totals);
}

int zngamd_bgzf_grep_approx(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                            uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                            int delim, uint32_t flags, uint32_t max_mismatch, uint64_t line_base, int32_t *status, zngamd_bgzf_grep_row *rows,
                            uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_grep_totals *totals)
try {
    if (!grep_patterns_ok(patterns, patterns_len, table, n_patterns, delim, max_mismatch)) return ZNGAMD_E_ARG;
    if (!c || !totals || (flags & ~15u) || (!in && in_len) || (n_members && (!members || !status)) || (!rows && rows_cap) || (!out && out_cap) ||
        (alloc && (rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_grep_dev(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, line_base, {nullptr, 0, nullptr, 0, true}, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t n = totals->matched;
    if (!totals->covered || (flags & ZNGAMD_BGZF_GREP_COUNT_ONLY) || !n) return ZNGAMD_OK;
    return bgzf_host_fetch(c, alloc, user, n, totals->bytes, rows, rows_cap, out, out_cap);
} ZA_ABI_GUARD

// ---- records by content (za_grep_records.hip)
static void tbx_scan(zngamd_ctx *c, unsigned long long *v, uint64_t n, int op, unsigned long long *d_total);

static bool grep_records_ok(uint32_t record_lines, int32_t match_line, int32_t first_byte)
{
    return record_lines >= 1 && record_lines <= ZNGAMD_BGZF_GREP_MAX_RECORD_LINES && match_line >= -1 && match_line < (int32_t)record_lines &&
           first_byte >= -1 && first_byte <= 255;
}

// The records of a window, once the lines pass has said how many lines its text holds: what the eleven record drivers below begin with.
// Nine of them (partition, trim, qc, key, sort key, place, screen, count, overlap) have no patterns of their own and call open(); grep
// records and classify hand their patterns to the lines pass themselves and call begin().
struct BgzfRecords {
    uint64_t lines, nrec, tile0; uint32_t ntiles, grid;             // grid: workgroups of 256 with a thread per record
    // lt: what the lines pass read.  covered and tail_off of the call's totals are set.  -> false: the call ends here (the member rows
    // do not tile the text, or no record has ended).
    bool begin(const BgzfWindow &w, const ZaGrepTotals &lt, uint32_t flags, uint32_t k, uint32_t *covered, uint64_t *tail_off)
    {
        *tail_off = w.text_off;
        if (!lt.covered) return false;
        *covered = 1;
        const bool fin = (flags & ZA_GREP_FINAL) != 0;
        lines = lt.seen; nrec = fin ? (lines + k - 1u) / k : lines / k;
        if (fin) *tail_off = w.text_end;
        if (!nrec) return false;                                  // (without FINAL: fewer than k lines have ended, the open record starts at text_off)
        tile0 = w.text_off / ZA_GREP_TILE;
        ntiles = (uint32_t)((w.text_end - 1ull) / ZA_GREP_TILE - tile0 + 1ull);      // (a line was decided: the text is not empty)
        grid = (uint32_t)((nrec + 255u) / 256u);
        return true;
    }
    // The prologue of a call without patterns: the lines pass for the delimiters alone, [the host waits for the line count], begin, and
    // gr_start made to hold the line starts.  *done: the call ends here, with the code returned (an error, or begin said so).
    int open(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, uint32_t k, uint32_t *covered, uint64_t *tail_off, bool *done)
    {
        *done = true;
        ZaGrepTotals lt;
        static const uint8_t no_bytes[1] = {0};
        static const zngamd_bgzf_pattern no_table[1] = {{0, 0}};
        const uint32_t lflags = flags & ZA_GREP_FINAL;
        const int r = bgzf_grep_lines_pass(c, w, no_bytes, 0, no_table, 0, lflags, 0, 0, &lt, sizeof lt, false);
        if (r) return r;
        if (!begin(w, lt, flags, k, covered, tail_off)) return ZNGAMD_OK;
        HIPCHK(c, c->gr_start.ensure(lines + 1u));
        *done = false;
        return ZNGAMD_OK;
    }
    // where every line starts (gr_start, lines + 1 entries), and a byte per record with a line that matched into hit[] (or none: no pointer, capacity 0)
    void launch_lines(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, uint32_t k, int32_t match_line, uint8_t *hit, uint64_t hit_cap) const
    {
        hipLaunchKernelGGL(za_k_grep_rec_lines, dim3(ntiles), dim3(256), 0, c->stream, c->gp_bits.p, c->gp_tiles.p, c->gp_carry.p, (const ZaGrepTotals *)c->d_small,
                           ntiles, tile0, w.text_off, w.text_end, flags, k, match_line, c->gr_start.p, lines + 1u, hit, hit_cap);
    }
};

// the lines pass without INVERT, [the host waits for the line count], lines, eval, the two scans, close, [the host waits for the totals],
// emit, pack
static int bgzf_grep_records_dev(zngamd_ctx *c, const BgzfWindow &w, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table,
                                 uint32_t n_patterns, uint32_t flags, uint32_t max_mismatch, uint32_t k, int32_t match_line, int32_t first_byte, uint64_t record_base,
                                 const BgzfDest &dst, zngamd_bgzf_grep_records_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    ZaGrepTotals lt;
    const uint32_t lflags = flags & (ZA_GREP_LINE_START | ZA_GREP_FINAL);
    const int r = bgzf_grep_lines_pass(c, w, patterns, patterns_len, table, n_patterns, lflags, max_mismatch, 0, &lt, sizeof lt);
    if (r) return r;
    BgzfRecords R;
    if (!R.begin(w, lt, flags, k, &totals->covered, &totals->tail_off)) return ZNGAMD_OK;
    const uint64_t lines = R.lines, nrec = R.nrec;
    HIPCHK(c, c->gr_start.ensure(lines + 1u)); HIPCHK(c, c->gr_hit.ensure(nrec)); HIPCHK(c, c->gr_sel.ensure(nrec)); HIPCHK(c, c->gr_len.ensure(nrec));
    HIPCHK(c, c->tb_blk.ensure(nrec / ZA_TBX_SCAN_ITEMS + 2u));
    unsigned long long *d_sums = (unsigned long long *)((uint8_t *)c->d_small + 80);       // the two scans' totals, the first bad record
    ZaGrepRecTotals *d_tot = (ZaGrepRecTotals *)((uint8_t *)c->d_small + 192);
    HIPCHK(c, hipMemsetAsync(c->gr_hit.p, 0, nrec, c->stream));
    HIPCHK(c, hipMemsetAsync(d_sums + 2, 0xFF, 8, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, match_line, c->gr_hit.p, nrec);
      hipLaunchKernelGGL(za_k_grep_rec_eval, dim3(R.grid), dim3(256), 0, c->stream, w.d_scratch, w.text_off, w.text_end, c->gr_start.p, lines, c->gr_hit.p, nrec, k,
                         flags & ZA_GREP_INVERT, first_byte, c->gr_sel.p, c->gr_len.p, d_sums + 2);
      tbx_scan(c, c->gr_sel.p, nrec, ZA_TBX_SUM, d_sums);
      tbx_scan(c, c->gr_len.p, nrec, ZA_TBX_SUM, d_sums + 1);
      hipLaunchKernelGGL(za_k_grep_rec_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, d_sums, d_sums + 1,
                         d_sums + 2, d_tot); }
    const int rt = bgzf_totals_read(c, totals, d_tot, sizeof *totals);
    if (rt) return rt;
    if (totals->bad || (flags & ZNGAMD_BGZF_GREP_COUNT_ONLY) || !totals->selected) return ZNGAMD_OK;
    const uint64_t n = totals->selected;
    return bgzf_pack_rows(c, w, dst, n, totals->bytes, [&](ZaGrepRow *d_rows) {
        hipLaunchKernelGGL(za_k_grep_rec_emit, dim3(R.grid), dim3(256), 0, c->stream, c->gr_sel.p, c->gr_start.p, lines, nrec, k, record_base, d_rows, n, c->gp_lens.p); });
}

int zngamd_bgzf_grep_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                 uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                                 int delim, uint32_t flags, uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base,
                                 void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out,
                                 uint64_t out_cap, zngamd_bgzf_grep_records_totals *totals)
{
    return zngamd_bgzf_grep_records_approx_dev(c, d_in, in_len, d_members, n_members, text_off, text_end, patterns, patterns_len, table, n_patterns, delim,
                                               flags, 0, record_lines, match_line, first_byte, record_base, d_scratch, scratch_cap, d_status, d_rows, rows_cap,
                                               d_out, out_cap, totals);
}

int zngamd_bgzf_grep_records_approx_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                        uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                        const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                                        uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base, void *d_scratch,
                                        uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out,
                                        uint64_t out_cap, zngamd_bgzf_grep_records_totals *totals)
try {
    if (!grep_patterns_ok(patterns, patterns_len, table, n_patterns, delim, max_mismatch) || !grep_records_ok(record_lines, match_line, first_byte)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !totals || (flags & ~15u) || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) ||
        (!d_rows && rows_cap) || (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_grep_records_dev(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, record_lines, match_line, first_byte, record_base,
                                  {(ZaGrepRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false}, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_grep_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                             uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                             int delim, uint32_t flags, uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base,
                             int32_t *status, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc,
                             void *user, zngamd_bgzf_grep_records_totals *totals)
{
    return zngamd_bgzf_grep_records_approx(c, in, in_len, members, n_members, text_off, text_end, patterns, patterns_len, table, n_patterns, delim, flags, 0,
                                           record_lines, match_line, first_byte, record_base, status, rows, rows_cap, out, out_cap, alloc, user, totals);
}

int zngamd_bgzf_grep_records_approx(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                                    uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                    const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                                    uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base, int32_t *status,
                                    zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user,
                                    zngamd_bgzf_grep_records_totals *totals)
try {
    if (!grep_patterns_ok(patterns, patterns_len, table, n_patterns, delim, max_mismatch) || !grep_records_ok(record_lines, match_line, first_byte)) return ZNGAMD_E_ARG;
    if (!c || !totals || (flags & ~15u) || (!in && in_len) || (n_members && (!members || !status)) || (!rows && rows_cap) || (!out && out_cap) ||
        (alloc && (rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_grep_records_dev(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, record_lines, match_line, first_byte, record_base,
                              {nullptr, 0, nullptr, 0, true}, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t n = totals->selected;
    if (!totals->covered || totals->bad || (flags & ZNGAMD_BGZF_GREP_COUNT_ONLY) || !n) return ZNGAMD_OK;
    return bgzf_host_fetch(c, alloc, user, n, totals->bytes, rows, rows_cap, out, out_cap);
} ZA_ABI_GUARD

// ---- records by their nearest pattern (za_classify.hip)
// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool classify_args_ok(const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags,
                             uint32_t max_mismatch, uint32_t record_lines, int32_t match_line, int32_t first_byte, const zngamd_bgzf_classify_totals *totals)
{
    if (!totals || (flags & ~(ZNGAMD_BGZF_GREP_LINE_START | ZNGAMD_BGZF_GREP_FINAL | ZNGAMD_BGZF_CLASSIFY_GROUP))) return false;
    if (!grep_patterns_ok(patterns, patterns_len, table, n_patterns, delim, max_mismatch) || !grep_records_ok(record_lines, match_line, first_byte)) return false;
    for (uint32_t i = 1; i < n_patterns; i++)                 // two patterns with the same bytes: no record could ever be assigned to either
        for (uint32_t j = 0; j < i; j++)
            if (table[i].len == table[j].len && !memcmp(patterns + table[i].off, patterns + table[j].off, table[i].len)) return false;
    return true;
}

// the lines pass for the delimiters alone, [the host waits for the line count], lines, classify, eval, hist, the scan, close, [the host
// waits for the totals], then with _GROUP scatter and pack, and the class rows (own: they stay in cl_row).
static int bgzf_classify_dev(zngamd_ctx *c, const BgzfWindow &w, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                             uint32_t flags, uint32_t max_mismatch, uint32_t k, int32_t match_line, int32_t first_byte, uint64_t record_base,
                             zngamd_bgzf_class_row *d_class, uint64_t class_cap, BgzfDest dst, zngamd_bgzf_classify_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    const uint32_t ncls = n_patterns + 2u;
    totals->n_classes = ncls;
    ZaGrepTotals lt;
    const uint32_t lflags = flags & (ZA_GREP_LINE_START | ZA_GREP_FINAL);
    int r = bgzf_grep_lines_pass(c, w, patterns, patterns_len, table, n_patterns, flags & ZA_GREP_FINAL, 0, 0, &lt, sizeof lt, false);
    if (r) return r;
    BgzfRecords R;
    if (!R.begin(w, lt, flags, k, &totals->covered, &totals->tail_off)) return ZNGAMD_OK;
    const bool group = (flags & ZA_CLS_GROUP) != 0;
    const uint64_t lines = R.lines, nrec = R.nrec;
    const uint32_t nwg = (uint32_t)((nrec + ZA_CLS_WG_RECORDS - 1u) / ZA_CLS_WG_RECORDS);
    const uint64_t ntab = (uint64_t)ncls * nwg;
    HIPCHK(c, c->gr_start.ensure(lines + 1u)); HIPCHK(c, c->cl_min.ensure(2u * nrec)); HIPCHK(c, c->cl_row.ensure(nrec)); HIPCHK(c, c->cl_len.ensure(nrec));
    HIPCHK(c, c->cl_cls.ensure(nrec)); HIPCHK(c, c->cl_tab.ensure(ntab)); HIPCHK(c, c->tb_blk.ensure(ntab / ZA_TBX_SCAN_ITEMS + 2u));
    HIPCHK(c, c->cl_tot.ensure(sizeof(ZaClsTotals) + 16u));
    std::vector<uint8_t> &par = c->gp_host;                      // (the lines pass has been waited for: its block is no longer read)
    grep_approx_params(par, patterns, table, n_patterns);
    HIPCHK(c, c->gp_par.ensure(par.size()));
    HIPCHK(c, hipMemcpyAsync(c->gp_par.p, par.data(), par.size(), hipMemcpyHostToDevice, c->stream));
    ZaClsTotals *d_tot = (ZaClsTotals *)c->cl_tot.p;
    unsigned long long *d_bad = (unsigned long long *)(c->cl_tot.p + sizeof(ZaClsTotals)), *d_sum = d_bad + 1;
    uint32_t *d_lo = c->cl_min.p, *d_hi = c->cl_min.p + nrec;
    HIPCHK(c, hipMemsetAsync(c->cl_min.p, 0xFF, 2u * nrec * 4u, c->stream));
    HIPCHK(c, hipMemsetAsync(d_tot, 0, sizeof(ZaClsTotals), c->stream));
    HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, 8, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, match_line, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_grep_classify, dim3(R.ntiles), dim3(256), 0, c->stream, w.d_scratch, w.scratch_cap, w.text_off, w.text_end, R.tile0,
                         (const ZaGrepPat *)c->gp_par.p, (const uint32_t *)(c->gp_par.p + ZA_GREP_APAR_WORDS), n_patterns, w.delim, lflags, max_mismatch,
                         c->gp_carry.p, k, match_line, nrec, d_lo, d_hi);
      hipLaunchKernelGGL(za_k_cls_eval, dim3(R.grid), dim3(256), 0, c->stream, w.d_scratch, w.text_off, w.text_end, c->gr_start.p, lines, d_lo, d_hi, nrec, k,
                         n_patterns, first_byte, c->cl_row.p, c->cl_cls.p, c->cl_len.p, d_bad);
      hipLaunchKernelGGL(za_k_cls_hist, dim3(nwg), dim3(ZA_CLS_WG_RECORDS), 0, c->stream, c->cl_cls.p, c->cl_len.p, nrec, ncls, nwg, c->cl_tab.p, d_tot);
      tbx_scan(c, c->cl_tab.p, ntab, ZA_TBX_SUM, d_sum);
      hipLaunchKernelGGL(za_k_cls_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, ncls, d_bad, d_tot); }
    r = bgzf_totals_read(c, totals, d_tot, sizeof *totals);
    if (r) return r;
    if (totals->bad) return ZNGAMD_OK;
    const uint64_t n = totals->seen;
    // The class rows are n entries more for the caller's memory to hold: one capacity stands for both arrays; without _GROUP there
    // are no rows and no bytes, and the class rows alone are judged.
    if (!dst.own) dst.rows_cap = group ? std::min(dst.rows_cap, class_cap) : class_cap;
    if (group)
        r = bgzf_pack_rows(c, w, dst, n, totals->bytes, [&](ZaGrepRow *d_rows) {
            hipLaunchKernelGGL(za_k_cls_scatter, dim3(nwg), dim3(ZA_CLS_WG_RECORDS), 0, c->stream, c->cl_cls.p, c->cl_row.p, c->cl_len.p, c->gr_start.p, nrec, k, ncls,
                               nwg, c->cl_tab.p, record_base, d_rows, n, c->gp_lens.p); });
    else if (!dst.own) r = bgzf_dest_ready(c, dst, n, 0);
    if (r) return r;
    if (!dst.own) HIPCHK(c, hipMemcpyAsync(d_class, c->cl_row.p, (size_t)n * 4u, hipMemcpyDeviceToDevice, c->stream));
    return ZNGAMD_OK;
}

int zngamd_bgzf_classify_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                     uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                                     int delim, uint32_t flags, uint32_t max_mismatch, uint32_t record_lines, int32_t match_line, int32_t first_byte,
                                     uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_class_row *d_class,
                                     uint64_t class_cap, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                     zngamd_bgzf_classify_totals *totals)
try {
    if (!classify_args_ok(patterns, patterns_len, table, n_patterns, delim, flags, max_mismatch, record_lines, match_line, first_byte, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) || (!d_class && class_cap) ||
        (!d_rows && rows_cap) || (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_classify_dev(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, record_lines, match_line, first_byte, record_base, d_class,
                              class_cap, {(ZaGrepRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false}, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_classify_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                                 uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                                 int delim, uint32_t flags, uint32_t max_mismatch, uint32_t record_lines, int32_t match_line, int32_t first_byte,
                                 uint64_t record_base, int32_t *status, zngamd_bgzf_class_row *cls, uint64_t class_cap, zngamd_bgzf_grep_row *rows,
                                 uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_classify_totals *totals)
try {
    if (!classify_args_ok(patterns, patterns_len, table, n_patterns, delim, flags, max_mismatch, record_lines, match_line, first_byte, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (!cls && class_cap) || (!rows && rows_cap) || (!out && out_cap) ||
        (alloc && (cls || rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_classify_dev(c, w, patterns, patterns_len, table, n_patterns, flags, max_mismatch, record_lines, match_line, first_byte, record_base, nullptr, 0,
                          {nullptr, 0, nullptr, 0, true}, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t n = totals->seen;
    const bool group = (flags & ZNGAMD_BGZF_CLASSIFY_GROUP) != 0;
    if (!totals->covered || totals->bad || !n) return ZNGAMD_OK;
    if (alloc) cls = (zngamd_bgzf_class_row *)alloc(user, n * sizeof(zngamd_bgzf_class_row));      // the caller's memory is asked for: class rows, rows, bytes
    return bgzf_host_fetch(c, alloc, user, n, totals->bytes, rows, rows_cap, out, out_cap, alloc ? cls != nullptr : n <= class_cap, group,
                           [&] { HIPCHK(c, hipMemcpyAsync(cls, c->cl_row.p, (size_t)n * 4u, hipMemcpyDeviceToHost, c->stream)); return ZNGAMD_OK; });
} ZA_ABI_GUARD

// ---- records by the caller's labels (za_partition.hip)
// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool partition_args_ok(int delim, uint32_t flags, uint32_t record_lines, int32_t first_byte, const uint16_t *labels, uint64_t n_labels, uint32_t n_classes,
                              const uint64_t *class_records, const uint64_t *class_bytes, const zngamd_bgzf_partition_totals *totals)
{
    if (!totals || !class_records || !class_bytes || (flags & ~(ZNGAMD_BGZF_GREP_FINAL | ZNGAMD_BGZF_CLASSIFY_GROUP))) return false;
    if (delim < 0 || delim > 255 || !grep_records_ok(record_lines, -1, first_byte)) return false;
    return n_classes >= 1 && n_classes <= ZNGAMD_BGZF_PARTITION_MAX_CLASSES && (labels || !n_labels);
}

// the lines pass for the delimiters alone, [the host waits for the line count], lines, eval, hist, with _GROUP the scan, close, [the
// host waits for the totals and the counts], then with _GROUP scatter and pack.  dst.own: labels is host memory and goes to pt_lab once
// the line count says how many are needed.
static int bgzf_partition_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, uint32_t k, int32_t first_byte, uint64_t record_base, const BgzfDest &dst,
                              const uint16_t *labels, uint64_t n_labels, uint32_t ncls, uint64_t *class_records, uint64_t *class_bytes,
                              zngamd_bgzf_partition_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    memset(class_records, 0, (size_t)ncls * 8u); memset(class_bytes, 0, (size_t)ncls * 8u);
    const uint32_t lflags = flags & ZA_GREP_FINAL;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const bool group = (flags & ZA_CLS_GROUP) != 0;
    const uint64_t lines = R.lines, nrec = R.nrec, nlab = std::min<uint64_t>(n_labels, nrec);
    const uint32_t nwg = (uint32_t)((nrec + ZA_PART_WG_RECORDS - 1u) / ZA_PART_WG_RECORDS);
    const uint64_t ntab = (uint64_t)ncls * nwg;
    HIPCHK(c, c->cl_len.ensure(nrec)); HIPCHK(c, c->cl_tab.ensure(ntab));
    HIPCHK(c, c->tb_blk.ensure(ntab / ZA_TBX_SCAN_ITEMS + 2u)); HIPCHK(c, c->pt_tot.ensure(12u + 2u * ZA_PART_MAX_CLASSES));
    if (dst.own && nlab) {
        HIPCHK(c, c->pt_lab.ensure(nlab));
        HIPCHK(c, hipMemcpyAsync(c->pt_lab.p, labels, (size_t)nlab * 2u, hipMemcpyHostToDevice, c->stream));
        labels = c->pt_lab.p;
    }
    ZaPartTotals *d_tot = (ZaPartTotals *)c->pt_tot.p;                                   // 9 words; then the two faults, the scan's sum, the counts
    unsigned long long *d_bad = c->pt_tot.p + 9, *d_sum = c->pt_tot.p + 11, *d_cnt = c->pt_tot.p + 12;
    HIPCHK(c, hipMemsetAsync(c->pt_tot.p, 0, (12u + 2u * (size_t)ncls) * 8u, c->stream));
    HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, 16, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_part_eval, dim3(R.grid), dim3(256), 0, c->stream, w.d_scratch, w.text_off, w.text_end, c->gr_start.p, lines, labels, nlab, nrec, k,
                         ncls, first_byte, c->cl_len.p, d_bad);
      hipLaunchKernelGGL(za_k_part_hist, dim3(nwg), dim3(ZA_PART_WG_RECORDS), 0, c->stream, labels, nlab, c->cl_len.p, nrec, ncls, nwg, c->cl_tab.p, d_cnt, d_tot);
      if (group) tbx_scan(c, c->cl_tab.p, ntab, ZA_TBX_SUM, d_sum);
      hipLaunchKernelGGL(za_k_part_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, nlab, k, lflags, w.text_end, record_base, ncls, d_cnt, d_bad,
                         d_tot); }
    HIPCHK(c, hipMemcpyAsync(class_records, d_cnt, (size_t)ncls * 8u, hipMemcpyDeviceToHost, c->stream));      // (the counts come with the totals: one wait)
    HIPCHK(c, hipMemcpyAsync(class_bytes, d_cnt + ncls, (size_t)ncls * 8u, hipMemcpyDeviceToHost, c->stream));
    r = bgzf_totals_read(c, totals, d_tot, sizeof *totals);
    if (r) return r;
    const uint64_t n = totals->seen - totals->dropped;
    if (totals->bad || totals->labels_short || !group || !n) return ZNGAMD_OK;
    return bgzf_pack_rows(c, w, dst, n, totals->bytes, [&](ZaGrepRow *d_rows) {
        hipLaunchKernelGGL(za_k_part_scatter, dim3(nwg), dim3(ZA_PART_WG_RECORDS), 0, c->stream, labels, nlab, c->cl_len.p, c->gr_start.p, nrec, k, ncls, nwg,
                           c->cl_tab.p, record_base, d_rows, n, c->gp_lens.p); });
}

int zngamd_bgzf_partition_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                      uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines, int32_t first_byte, uint64_t record_base,
                                      void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out,
                                      uint64_t out_cap, const uint16_t *d_labels, uint64_t n_labels, uint32_t n_classes, uint64_t *class_records,
                                      uint64_t *class_bytes, zngamd_bgzf_partition_totals *totals)
try {
    if (!partition_args_ok(delim, flags, record_lines, first_byte, d_labels, n_labels, n_classes, class_records, class_bytes, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) || (!d_rows && rows_cap) ||
        (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_partition_dev(c, w, flags, record_lines, first_byte, record_base, {(ZaGrepRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false}, d_labels,
                               n_labels, n_classes, class_records, class_bytes, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_partition_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                                  uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines, int32_t first_byte, uint64_t record_base,
                                  int32_t *status, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc,
                                  void *user, const uint16_t *labels, uint64_t n_labels, uint32_t n_classes, uint64_t *class_records, uint64_t *class_bytes,
                                  zngamd_bgzf_partition_totals *totals)
try {
    if (!partition_args_ok(delim, flags, record_lines, first_byte, labels, n_labels, n_classes, class_records, class_bytes, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (!rows && rows_cap) || (!out && out_cap) || (alloc && (rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_partition_dev(c, w, flags, record_lines, first_byte, record_base, {nullptr, 0, nullptr, 0, true}, labels, n_labels, n_classes, class_records,
                           class_bytes, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t n = totals->seen - totals->dropped;
    if (!totals->covered || totals->bad || totals->labels_short || !(flags & ZNGAMD_BGZF_CLASSIFY_GROUP) || !n) return ZNGAMD_OK;
    return bgzf_host_fetch(c, alloc, user, n, totals->bytes, rows, rows_cap, out, out_cap);
} ZA_ABI_GUARD

// ---- records trimmed (za_trim.hip)
// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool trim_args_ok(const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags,
                         const zngamd_bgzf_trim_conf *cf, const uint8_t *drop, uint64_t n_drop, const zngamd_bgzf_trim_totals *totals)
{
    if (!totals || !cf || (flags & ~(ZNGAMD_BGZF_GREP_FINAL | ZNGAMD_BGZF_CLASSIFY_GROUP)) || delim < 0 || delim > 255 || (!drop && n_drop)) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte)) return false;
    if (cf->seq_line < 0 || cf->seq_line >= (int32_t)cf->record_lines || cf->qual_line < -1 || cf->qual_line >= (int32_t)cf->record_lines ||
        cf->qual_line == cf->seq_line) return false;
    if (cf->qual_front > ZNGAMD_BGZF_TRIM_MAX_QUALITY || cf->qual_back > ZNGAMD_BGZF_TRIM_MAX_QUALITY || cf->quality_base > 255u ||
        (cf->qual_line < 0 && (cf->qual_front || cf->qual_back))) return false;
    if (cf->max_mismatch > ZNGAMD_BGZF_GREP_MAX_MISMATCH || cf->min_overlap < 1u || cf->min_overlap > ZNGAMD_BGZF_GREP_MAX_PATTERN ||
        (cf->flags & ~ZNGAMD_BGZF_TRIM_KEEP_SHORT) || cf->reserved[0] || cf->reserved[1] || cf->reserved[2]) return false;
    return !n_patterns || grep_patterns_ok(patterns, patterns_len, table, n_patterns, delim, cf->max_mismatch);
}

// the lines pass for the delimiters alone, [the host waits for the line count], lines, eval, hist, with _GROUP the scan, close, [the
// host waits for the totals], then with _GROUP scatter, offsets and gather, and the trim rows (own: they stay in tr_row).  dst.own:
// drop is host memory and goes to tr_drop once the line count says how many bytes are needed.
static int bgzf_trim_dev(zngamd_ctx *c, const BgzfWindow &w, const uint8_t *patterns, const zngamd_bgzf_pattern *table, uint32_t n_patterns, uint32_t flags,
                         const zngamd_bgzf_trim_conf &cf, uint64_t record_base, const uint8_t *drop, uint64_t n_drop, zngamd_bgzf_trim_row *d_trim,
                         uint64_t trim_cap, BgzfDest dst, zngamd_bgzf_trim_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines, ncls = 2u;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const bool group = (flags & ZA_CLS_GROUP) != 0, keep_short = (cf.flags & ZA_TRIM_KEEP_SHORT) != 0;
    const uint64_t lines = R.lines, nrec = R.nrec, ndrop = std::min<uint64_t>(n_drop, nrec);
    const uint32_t nwg = (uint32_t)((nrec + ZA_PART_WG_RECORDS - 1u) / ZA_PART_WG_RECORDS);
    const uint64_t ntab = (uint64_t)ncls * nwg;
    constexpr size_t TOT_WORDS = sizeof(ZaTrimTotals) / 8u;                              // then the two faults, the scan's sum, the counts, hist's totals
    HIPCHK(c, c->cl_len.ensure(nrec)); HIPCHK(c, c->cl_tab.ensure(ntab)); HIPCHK(c, c->pt_lab.ensure(nrec));
    HIPCHK(c, c->tb_blk.ensure(ntab / ZA_TBX_SCAN_ITEMS + 2u)); HIPCHK(c, c->tr_row.ensure(nrec));
    HIPCHK(c, c->tr_tot.ensure(TOT_WORDS + 3u + 2u * ncls + sizeof(ZaPartTotals) / 8u));
    if (dst.own && drop && ndrop) {
        HIPCHK(c, c->tr_drop.ensure(ndrop));
        HIPCHK(c, hipMemcpyAsync(c->tr_drop.p, drop, (size_t)ndrop, hipMemcpyHostToDevice, c->stream));
        drop = c->tr_drop.p;
    }
    static_assert(ZA_GREP_APAR_WORDS == ZA_GREP_MAX_PAT * sizeof(ZaGrepPat), "where za_k_trim_eval finds the adapter words");
    std::vector<uint8_t> &par = c->gp_host;                      // (the lines pass has been waited for: its block is no longer read)
    grep_approx_params(par, patterns, table, n_patterns);
    HIPCHK(c, c->gp_par.ensure(par.size() + 4u));
    HIPCHK(c, hipMemcpyAsync(c->gp_par.p, par.data(), par.size(), hipMemcpyHostToDevice, c->stream));
    ZaTrimPar P = {k, (uint32_t)cf.seq_line, cf.qual_line, cf.first_byte, cf.cut_front, cf.cut_back, cf.qual_front, cf.qual_back, cf.quality_base,
                   cf.max_mismatch, cf.min_overlap, cf.min_length, keep_short ? 1u : 0u, w.delim, n_patterns, 0u};
    for (uint32_t i = 0; i < n_patterns; i++) P.max_len = std::max(P.max_len, table[i].len);
    ZaTrimTotals *d_tot = (ZaTrimTotals *)c->tr_tot.p;
    unsigned long long *d_bad = c->tr_tot.p + TOT_WORDS, *d_sum = d_bad + 2, *d_cnt = d_bad + 3;
    ZaPartTotals *d_ptot = (ZaPartTotals *)(d_cnt + 2u * ncls);
    HIPCHK(c, hipMemsetAsync(c->tr_tot.p, 0, (TOT_WORDS + 3u + 2u * ncls) * 8u + sizeof(ZaPartTotals), c->stream));
    HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, 16, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_trim_eval, dim3((uint32_t)((nrec + ZA_TRIM_WG_RECORDS - 1u) / ZA_TRIM_WG_RECORDS)), dim3(256), 0, c->stream, w.d_scratch,
                         w.text_end, c->gr_start.p, lines, nrec, P, (const uint8_t *)c->gp_par.p, drop, ndrop, c->tr_row.p, c->cl_len.p, c->pt_lab.p, d_tot);
      hipLaunchKernelGGL(za_k_part_hist, dim3(nwg), dim3(ZA_PART_WG_RECORDS), 0, c->stream, c->pt_lab.p, nrec, c->cl_len.p, nrec, ncls, nwg, c->cl_tab.p, d_cnt, d_ptot);
      if (group) tbx_scan(c, c->cl_tab.p, ntab, ZA_TBX_SUM, d_sum);
      hipLaunchKernelGGL(za_k_trim_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, ndrop, drop ? 1u : 0u, k, lflags, w.text_end, record_base,
                         d_cnt, d_bad, d_tot); }
    r = bgzf_totals_read(c, totals, d_tot, sizeof *totals);
    if (r) return r;
    if (totals->bad || totals->drop_short) return ZNGAMD_OK;
    const uint64_t n = group ? totals->kept + (keep_short ? totals->too_short : 0ull) : 0ull, bytes = group ? totals->bytes : 0ull;
    if (!dst.own && totals->seen > trim_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    r = bgzf_dest_ready(c, dst, n, bytes);
    if (r) return r;
    if (n) {
        HIPCHK(c, c->gp_lens.ensure(n)); HIPCHK(c, c->st_off.ensure(n));
        uint64_t *d_bytes = (uint64_t *)((uint8_t *)c->d_small + 128);
        { ProfScope ps(c, ZNGAMD_K_GATHER);
          hipLaunchKernelGGL(za_k_part_scatter, dim3(nwg), dim3(ZA_PART_WG_RECORDS), 0, c->stream, c->pt_lab.p, nrec, c->cl_len.p, c->gr_start.p, nrec, k, ncls, nwg,
                             c->cl_tab.p, record_base, dst.d_rows, n, c->gp_lens.p);
          hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(n <= 64 ? 64 : 1024), 0, c->stream, c->gp_lens.p, (uint32_t)n, 0u, 0ull, c->st_off.p, d_bytes,
                             (const ZaUnit *)nullptr);
          hipLaunchKernelGGL(za_k_trim_gather, dim3((uint32_t)((n + 3u) / 4u)), dim3(256), 0, c->stream, w.d_scratch, c->gr_start.p, lines, record_base, k,
                             (uint32_t)cf.seq_line, cf.qual_line, w.delim, c->tr_row.p, dst.d_rows, c->st_off.p, n, dst.d_out, bytes); }
        c->bgzf_stats[2] += n;
        HIPCHK(c, hipGetLastError());
    }
    if (!dst.own) HIPCHK(c, hipMemcpyAsync(d_trim, c->tr_row.p, (size_t)totals->seen * sizeof(ZaTrimRow), hipMemcpyDeviceToDevice, c->stream));
    return ZNGAMD_OK;
}

int zngamd_bgzf_trim_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                 uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns,
                                 int delim, uint32_t flags, const zngamd_bgzf_trim_conf *conf, uint64_t record_base, void *d_scratch, uint64_t scratch_cap,
                                 int32_t *d_status, const uint8_t *d_drop, uint64_t n_drop, zngamd_bgzf_trim_row *d_trim, uint64_t trim_cap,
                                 zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap, zngamd_bgzf_trim_totals *totals)
try {
    if (!trim_args_ok(patterns, patterns_len, table, n_patterns, delim, flags, conf, d_drop, n_drop, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) || (!d_trim && trim_cap) ||
        (!d_rows && rows_cap) || (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_trim_dev(c, w, patterns, table, n_patterns, flags, *conf, record_base, d_drop, n_drop, d_trim, trim_cap,
                          {(ZaGrepRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false}, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_trim_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                             uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim,
                             uint32_t flags, const zngamd_bgzf_trim_conf *conf, uint64_t record_base, int32_t *status, const uint8_t *drop, uint64_t n_drop,
                             zngamd_bgzf_trim_row *trim, uint64_t trim_cap, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap,
                             zngamd_alloc_fn alloc, void *user, zngamd_bgzf_trim_totals *totals)
try {
    if (!trim_args_ok(patterns, patterns_len, table, n_patterns, delim, flags, conf, drop, n_drop, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (!trim && trim_cap) || (!rows && rows_cap) || (!out && out_cap) ||
        (alloc && (trim || rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_trim_dev(c, w, patterns, table, n_patterns, flags, *conf, record_base, drop, n_drop, nullptr, 0, {nullptr, 0, nullptr, 0, true}, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t seen = totals->seen;
    const bool group = (flags & ZNGAMD_BGZF_CLASSIFY_GROUP) != 0;
    if (!totals->covered || totals->bad || totals->drop_short || !seen) return ZNGAMD_OK;
    const uint64_t n = group ? totals->kept + ((conf->flags & ZNGAMD_BGZF_TRIM_KEEP_SHORT) ? totals->too_short : 0ull) : 0ull;
    if (alloc) trim = (zngamd_bgzf_trim_row *)alloc(user, seen * sizeof(zngamd_bgzf_trim_row));      // the caller's memory is asked for: trim rows, rows, bytes
    return bgzf_host_fetch(c, alloc, user, n, totals->bytes, rows, rows_cap, out, out_cap, alloc ? trim != nullptr : seen <= trim_cap, n != 0,
                           [&] { HIPCHK(c, hipMemcpyAsync(trim, c->tr_row.p, (size_t)seen * sizeof(ZaTrimRow), hipMemcpyDeviceToHost, c->stream)); return ZNGAMD_OK; });
} ZA_ABI_GUARD

// ---- records counted (za_qc.hip)
// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool qc_args_ok(int delim, uint32_t flags, const zngamd_bgzf_qc_conf *cf, const uint64_t *tables, const zngamd_bgzf_qc_row *rows, bool alloc,
                       const zngamd_bgzf_qc_totals *totals)
{
    if (!totals || !cf || !tables || (flags & ~ZNGAMD_BGZF_GREP_FINAL) || delim < 0 || delim > 255) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte)) return false;
    if (cf->seq_line < 0 || cf->seq_line >= (int32_t)cf->record_lines || cf->qual_line < -1 || cf->qual_line >= (int32_t)cf->record_lines ||
        cf->qual_line == cf->seq_line) return false;
    if (cf->quality_base > 255u || cf->cycles < 1u || cf->cycles > ZNGAMD_BGZF_QC_MAX_CYCLES || cf->low_quality > ZNGAMD_BGZF_QC_MAX_LOW ||
        (cf->flags & ~ZNGAMD_BGZF_QC_ROWS)) return false;
    for (uint32_t v : cf->reserved) if (v) return false;
    return !(cf->flags & ZNGAMD_BGZF_QC_ROWS) || rows || alloc;
}

// d_tables is zeroed, the lines pass for the delimiters alone, [the host waits for the line count], lines, eval, close, [the host waits
// for the totals].  d_tables: ZNGAMD_BGZF_QC_TABLE_WORDS(cf.cycles) words of device memory.  own: the rows go to qc_row; otherwise to d_rows
// when rows_cap holds them, and nowhere (*rows_short) when it does not.
static int bgzf_qc_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, const zngamd_bgzf_qc_conf &cf, uint64_t record_base, unsigned long long *d_tables,
                       bool own, ZaQcRow *d_rows, uint64_t rows_cap, bool *rows_short, zngamd_bgzf_qc_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    totals->min_len = UINT64_MAX;
    *rows_short = false;
    HIPCHK(c, hipMemsetAsync(d_tables, 0, (size_t)ZNGAMD_BGZF_QC_TABLE_WORDS(cf.cycles) * 8u, c->stream));
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const uint64_t lines = R.lines, nrec = R.nrec;
    if (cf.flags & ZA_QC_ROWS) r = bgzf_rows_dest(c, c->qc_row, nrec, own, &d_rows, rows_cap, rows_short);
    else d_rows = nullptr;
    if (r) return r;
    // the persistent grid: ZA_QC_WG_PER_CU workgroups per CU, each with one span of at least ZA_QC_SPAN_MIN records
    const uint64_t slots = (uint64_t)std::max<uint32_t>(c->search_slots, 1u) * ZA_QC_WG_PER_CU;
    const uint64_t span = std::min<uint64_t>(std::max<uint64_t>((nrec + slots - 1u) / slots, ZA_QC_SPAN_MIN), ZA_QC_SPAN_MAX);
    const ZaQcPar P = {k, (uint32_t)cf.seq_line, cf.qual_line, cf.first_byte, cf.quality_base, cf.cycles, cf.low_quality, w.delim};
    ZaQcTotals *d_tot;
    unsigned long long *d_bad;                                                           // the two faults
    r = bgzf_totals_area(c, c->qc_tot, 2u, &d_tot, &d_bad);
    if (r) return r;
    HIPCHK(c, hipMemsetAsync(&d_tot->min_len, 0xFF, 8, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_qc_eval, dim3((uint32_t)((nrec + span - 1u) / span)), dim3(256), 0, c->stream, w.d_scratch, w.text_end, c->gr_start.p, lines, nrec, span,
                         P, d_tables, d_rows, d_tot);
      hipLaunchKernelGGL(za_k_qc_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, d_bad, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, sizeof *totals);
}

int zngamd_bgzf_qc_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                               uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_qc_conf *conf, uint64_t record_base, void *d_scratch,
                               uint64_t scratch_cap, int32_t *d_status, uint64_t *d_tables, uint64_t tables_cap, zngamd_bgzf_qc_row *d_rows, uint64_t rows_cap,
                               zngamd_bgzf_qc_totals *totals)
try {
    if (!qc_args_ok(delim, flags, conf, d_tables, d_rows, false, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) || (!d_rows && rows_cap))
        return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (tables_cap < ZNGAMD_BGZF_QC_TABLE_WORDS(conf->cycles)) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    HIPCHK(c, hipSetDevice(c->device));
    bool rows_short = false;
    int r = bgzf_qc_dev(c, w, flags, *conf, record_base, (unsigned long long *)d_tables, false, (ZaQcRow *)d_rows, rows_cap, &rows_short, totals);
    if (r) return r;
    return bgzf_dev_finish(c, rows_short, totals->bad != 0);
} ZA_ABI_GUARD

int zngamd_bgzf_qc_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                           uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_qc_conf *conf, uint64_t record_base, int32_t *status, uint64_t *tables,
                           uint64_t tables_cap, zngamd_bgzf_qc_row *rows, uint64_t rows_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_qc_totals *totals)
try {
    if (!qc_args_ok(delim, flags, conf, tables, rows, alloc != nullptr, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (!rows && rows_cap) || (alloc && rows)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    const uint64_t words = ZNGAMD_BGZF_QC_TABLE_WORDS(conf->cycles);
    if (tables_cap < words) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    HIPCHK(c, c->qc_tab.ensure(words));
    bool rows_short = false;
    r = bgzf_qc_dev(c, w, flags, *conf, record_base, c->qc_tab.p, true, nullptr, 0, &rows_short, totals);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(tables, c->qc_tab.p, (size_t)words * 8u, hipMemcpyDeviceToHost, c->stream));      // (the tables come with the status words: one wait)
    r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t seen = totals->seen;
    if (!(conf->flags & ZNGAMD_BGZF_QC_ROWS) || !totals->covered || totals->bad || !seen) return ZNGAMD_OK;
    return bgzf_host_rows(c, alloc, user, rows, rows_cap, c->qc_row.p, seen, sizeof(ZaQcRow));
} ZA_ABI_GUARD

// ---- records keyed, keys resolved (za_dedup.hip)
// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool key_args_ok(int delim, uint32_t flags, const zngamd_bgzf_key_conf *cf, const zngamd_bgzf_key_row *rows, bool alloc, const zngamd_bgzf_key_totals *totals)
{
    if (!totals || !cf || (flags & ~ZNGAMD_BGZF_GREP_FINAL) || delim < 0 || delim > 255) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte)) return false;
    if (cf->seq_line < 0 || cf->seq_line >= (int32_t)cf->record_lines || (cf->flags & ~(ZNGAMD_BGZF_KEY_IGNORE_CASE | ZNGAMD_BGZF_KEY_CANONICAL))) return false;
    for (uint32_t v : cf->reserved) if (v) return false;
    return rows || alloc;
}

// The lines pass for the delimiters alone, [the host waits for the line count], lines, keys, close, [the host waits for the totals].
// own: the rows go to dd_row; otherwise to d_rows when rows_cap holds them, and nowhere (*rows_short) when it does not.
static int bgzf_key_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, const zngamd_bgzf_key_conf &cf, uint64_t record_base, bool own, ZaKeyRow *d_rows,
                        uint64_t rows_cap, bool *rows_short, zngamd_bgzf_key_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    *rows_short = false;
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const uint64_t lines = R.lines, nrec = R.nrec;
    r = bgzf_rows_dest(c, c->dd_row, nrec, own, &d_rows, rows_cap, rows_short);
    if (r) return r;
    const uint32_t grid = bgzf_wave_grid(c, nrec, ZA_KEY_WG_PER_CU);
    const ZaKeyPar P = {k, (uint32_t)cf.seq_line, cf.first_byte, cf.first, cf.length, cf.flags, w.delim};
    ZaKeyTotals *d_tot;
    unsigned long long *d_bad;                                                           // the fault
    r = bgzf_totals_area(c, c->dd_tot, 1u, &d_tot, &d_bad);
    if (r) return r;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_dedup_keys, dim3(grid), dim3(256), 0, c->stream, w.d_scratch, w.text_end, c->gr_start.p, lines, nrec, P, d_rows, d_tot);
      hipLaunchKernelGGL(za_k_rec_close<ZaKeyTotals>, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, d_bad, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, sizeof *totals);
}

int zngamd_bgzf_key_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_key_conf *conf, uint64_t record_base, void *d_scratch,
                                uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_key_row *d_rows, uint64_t rows_cap, zngamd_bgzf_key_totals *totals)
try {
    if (!key_args_ok(delim, flags, conf, d_rows, false, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    bool rows_short = false;
    int r = bgzf_key_dev(c, w, flags, *conf, record_base, false, (ZaKeyRow *)d_rows, rows_cap, &rows_short, totals);
    if (r) return r;
    return bgzf_dev_finish(c, rows_short, totals->bad != 0);
} ZA_ABI_GUARD

int zngamd_bgzf_key_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                            uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_key_conf *conf, uint64_t record_base, int32_t *status,
                            zngamd_bgzf_key_row *rows, uint64_t rows_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_key_totals *totals)
try {
    if (!key_args_ok(delim, flags, conf, rows, alloc != nullptr, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (alloc && rows)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    bool rows_short = false;
    r = bgzf_key_dev(c, w, flags, *conf, record_base, true, nullptr, 0, &rows_short, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t seen = totals->seen;
    if (!totals->covered || totals->bad || !seen) return ZNGAMD_OK;
    return bgzf_host_rows(c, alloc, user, rows, rows_cap, c->dd_row.p, seen, sizeof(ZaKeyRow));
} ZA_ABI_GUARD

// the slots of the table for n keys: the smallest power of two that is >= 2 n and >= ZA_DEDUP_MIN_CAP (n <= ZNGAMD_DEDUP_MAX_KEYS)
static uint64_t dedup_cap(uint64_t n)
{
    uint64_t cap = ZA_DEDUP_MIN_CAP;
    while (cap < 2u * n) cap <<= 1;
    return cap;
}

// the slots, the counters, the two words the lookup sums, the totals
uint64_t zngamd_dedup_scratch_bytes(uint64_t n)
{
    return n > ZNGAMD_DEDUP_MAX_KEYS ? 0 : dedup_cap(n) * 12u + 16u + sizeof(ZaDedupTotals);
}

static bool dedup_args_ok(const zngamd_bgzf_key_row *keys, uint64_t n, const zngamd_dedup_totals *totals)
{
    return totals && n <= ZNGAMD_DEDUP_MAX_KEYS && (keys || !n);
}

// n > 0.  The table is set up (slots all ones, the rest zero), insert, lookup, close, [the host waits for the totals].
static int dedup_dev(zngamd_ctx *c, const ZaKeyRow *d_keys, uint64_t n, uint8_t *d_scratch, unsigned long long *d_first, uint32_t *d_count, zngamd_dedup_totals *totals)
{
    const uint64_t cap = dedup_cap(n);
    unsigned long long *slot = (unsigned long long *)d_scratch;
    uint32_t *cnt = (uint32_t *)(d_scratch + cap * 8u);
    unsigned long long *acc = (unsigned long long *)(d_scratch + cap * 12u);
    ZaDedupTotals *d_tot = (ZaDedupTotals *)(acc + 2);
    HIPCHK(c, hipMemsetAsync(slot, 0xFF, (size_t)cap * 8u, c->stream));
    HIPCHK(c, hipMemsetAsync(cnt, 0, (size_t)cap * 4u + 16u + sizeof(ZaDedupTotals), c->stream));
    const uint32_t grid = (uint32_t)((n + 255u) / 256u);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_dedup_insert, dim3(grid), dim3(256), 0, c->stream, d_keys, n, slot, cnt, cap - 1u);
      hipLaunchKernelGGL(za_k_dedup_lookup, dim3(grid), dim3(256), 0, c->stream, d_keys, n, slot, cnt, cap - 1u, d_first, d_count, acc);
      hipLaunchKernelGGL(za_k_dedup_close, dim3(1), dim3(1), 0, c->stream, acc, n, d_tot); }
    const int r = bgzf_totals_read(c, totals, d_tot, sizeof *totals);
    if (r) return r;
    prof_collect(c);
    return ZNGAMD_OK;
}

int zngamd_dedup_keys_dev(zngamd_ctx *c, const zngamd_bgzf_key_row *d_keys, uint64_t n, void *d_scratch, uint64_t scratch_cap, uint64_t *d_first,
                          uint32_t *d_count, zngamd_dedup_totals *totals)
try {
    if (!dedup_args_ok(d_keys, n, totals) || (n && !d_scratch) || ((uintptr_t)d_scratch & 7u)) return ZNGAMD_E_ARG;
    if (!c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (n && scratch_cap < zngamd_dedup_scratch_bytes(n)) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    memset(totals, 0, sizeof *totals);
    if (!n) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return dedup_dev(c, (const ZaKeyRow *)d_keys, n, (uint8_t *)d_scratch, (unsigned long long *)d_first, d_count, totals);
} ZA_ABI_GUARD

int zngamd_dedup_keys(zngamd_ctx *c, const zngamd_bgzf_key_row *keys, uint64_t n, uint64_t *first, uint32_t *count, zngamd_dedup_totals *totals)
try {
    if (!dedup_args_ok(keys, n, totals)) return ZNGAMD_E_ARG;
    if (!c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    memset(totals, 0, sizeof *totals);
    if (!n) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->dd_row.ensure(n)); HIPCHK(c, c->dd_tab.ensure(zngamd_dedup_scratch_bytes(n)));
    if (first) HIPCHK(c, c->dd_first.ensure(n));
    if (count) HIPCHK(c, c->dd_count.ensure(n));
    HIPCHK(c, hipMemcpyAsync(c->dd_row.p, keys, (size_t)n * sizeof(ZaKeyRow), hipMemcpyHostToDevice, c->stream));
    int r = dedup_dev(c, c->dd_row.p, n, c->dd_tab.p, first ? c->dd_first.p : nullptr, count ? c->dd_count.p : nullptr, totals);
    if (r) return r;
    if (first) HIPCHK(c, hipMemcpyAsync(first, c->dd_first.p, (size_t)n * 8u, hipMemcpyDeviceToHost, c->stream));
    if (count) HIPCHK(c, hipMemcpyAsync(count, c->dd_count.p, (size_t)n * 4u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// ---- records in another order (za_sort.hip)
// the key's width W for a judged configuration: the parts' bytes, rounded up to 8
static uint32_t sort_key_width(const zngamd_bgzf_sort_conf &cf)
{
    uint32_t w = 0;
    for (uint32_t p = 0; p < cf.n_parts; p++) w += cf.part[p].kind == ZNGAMD_BGZF_SORT_BYTES ? cf.part[p].width : cf.part[p].kind == ZNGAMD_BGZF_SORT_NUMBER ? 8u : 4u;
    return (w + 7u) & ~7u;
}

// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool sort_key_args_ok(int delim, uint32_t flags, const zngamd_bgzf_sort_conf *cf, const uint8_t *rows, const uint32_t *lengths, bool alloc,
                             const zngamd_bgzf_sort_key_totals *totals)
{
    if (!totals || !cf || (flags & ~ZNGAMD_BGZF_GREP_FINAL) || delim < 0 || delim > 255) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte) || cf->meta_byte < -1 || cf->meta_byte > 255 || cf->n_parts > ZNGAMD_BGZF_SORT_MAX_PARTS) return false;
    for (uint32_t v : cf->reserved) if (v) return false;
    uint32_t w = 0;
    for (uint32_t p = 0; p < ZNGAMD_BGZF_SORT_MAX_PARTS; p++) {
        const zngamd_bgzf_sort_part &q = cf->part[p];
        if (p >= cf->n_parts) {
            if (q.line || q.column || q.width || q.first || q.flags || q.kind || q.sep) return false;
            continue;
        }
        if (q.line < 0 || q.line >= (int32_t)cf->record_lines || q.column < -1 || q.kind > ZNGAMD_BGZF_SORT_LENGTH) return false;
        const bool bytes = q.kind == ZNGAMD_BGZF_SORT_BYTES;
        if (q.flags & ~(bytes ? ZNGAMD_BGZF_SORT_REVERSE | ZNGAMD_BGZF_SORT_IGNORE_CASE | ZNGAMD_BGZF_SORT_TRUNCATE : ZNGAMD_BGZF_SORT_REVERSE)) return false;
        if (bytes ? (q.width < 8u || q.width > 128u || (q.width & 7u)) : (q.width || q.first)) return false;
        w += bytes ? q.width : q.kind == ZNGAMD_BGZF_SORT_NUMBER ? 8u : 4u;
    }
    if (w > ZNGAMD_SORT_MAX_WIDTH) return false;
    return alloc || (lengths && (rows || !w));
}

// The lines pass for the delimiters alone, [the host waits for the line count], lines, keys, close, [the host waits for the totals].
// own: the rows and lengths go to so_row and so_len; otherwise to d_rows and d_len when rows_cap holds them, and nowhere (*rows_short)
// when it does not.
static int bgzf_sort_key_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, const zngamd_bgzf_sort_conf &cf, uint64_t record_base, bool own, uint8_t *d_rows,
                             uint32_t *d_len, uint64_t rows_cap, bool *rows_short, zngamd_bgzf_sort_key_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    *rows_short = false;
    const uint32_t W = sort_key_width(cf);
    totals->key_width = W;
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const uint64_t lines = R.lines, nrec = R.nrec;
    if (own) { HIPCHK(c, c->so_row.ensure(nrec * W + 8u)); HIPCHK(c, c->so_len.ensure(nrec)); d_rows = c->so_row.p; d_len = c->so_len.p; }
    else if (rows_cap < nrec) { *rows_short = true; d_rows = nullptr; d_len = nullptr; }
    const uint32_t grid = bgzf_wave_grid(c, nrec, ZA_SORT_WG_PER_CU);
    ZaSortPar P = {};
    P.k_lines = k; P.first_byte = cf.first_byte; P.meta_byte = cf.meta_byte; P.n_parts = cf.n_parts; P.delim = w.delim; P.width = W; P.final = lflags ? 1u : 0u;
    static_assert(sizeof(ZaSortPart) == sizeof(zngamd_bgzf_sort_part) && sizeof(ZaSortPart) == 20, "the parts are copied as they are");
    memcpy(P.part, cf.part, sizeof P.part);
    ZaSortKeyTotals *d_tot;
    unsigned long long *d_bad;                                                           // the three faults
    r = bgzf_totals_area(c, c->so_tot, 3u, &d_tot, &d_bad);
    if (r) return r;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_sort_keys, dim3(grid), dim3(256), 0, c->stream, w.d_scratch, w.text_end, c->gr_start.p, lines, nrec, P, d_rows, d_len, d_tot);
      hipLaunchKernelGGL(za_k_sort_keys_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, W, d_bad, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, sizeof *totals);
}

int zngamd_bgzf_sort_key_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                     uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_sort_conf *conf, uint64_t record_base, void *d_scratch,
                                     uint64_t scratch_cap, int32_t *d_status, uint8_t *d_rows, uint32_t *d_lengths, uint64_t rows_cap,
                                     zngamd_bgzf_sort_key_totals *totals)
try {
    if (!sort_key_args_ok(delim, flags, conf, d_rows, d_lengths, false, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    bool rows_short = false;
    int r = bgzf_sort_key_dev(c, w, flags, *conf, record_base, false, d_rows, d_lengths, rows_cap, &rows_short, totals);
    if (r) return r;
    return bgzf_dev_finish(c, rows_short, totals->bad != 0);
} ZA_ABI_GUARD

int zngamd_bgzf_sort_key_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                                 uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_sort_conf *conf, uint64_t record_base, int32_t *status,
                                 uint8_t *rows, uint32_t *lengths, uint64_t rows_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_sort_key_totals *totals)
try {
    if (!sort_key_args_ok(delim, flags, conf, rows, lengths, alloc != nullptr, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (alloc && (rows || lengths))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    bool rows_short = false;
    r = bgzf_sort_key_dev(c, w, flags, *conf, record_base, true, nullptr, nullptr, 0, &rows_short, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t seen = totals->seen, W = totals->key_width;
    if (!totals->covered || totals->bad || !seen) return ZNGAMD_OK;
    if (alloc) {
        if (W) rows = (uint8_t *)alloc(user, seen * W);
        lengths = (uint32_t *)alloc(user, seen * 4u);
        if ((W && !rows) || !lengths) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned NULL");
    } else if (seen > rows_cap) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    if (W) HIPCHK(c, hipMemcpyAsync(rows, c->so_row.p, (size_t)(seen * W), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(lengths, c->so_len.p, (size_t)seen * 4u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// the work area of the sort: the second order array, the digits, the table of counts (256 values x tiles), the 256 totals, OR and AND
static uint64_t sort_tiles(uint64_t n) { return (n + ZA_SORT_TILE - 1u) / ZA_SORT_TILE; }
static uint64_t sort_r8(uint64_t x) { return (x + 7u) & ~7ull; }
static bool sort_width_ok(uint32_t width) { return width >= 8u && width <= ZNGAMD_SORT_MAX_WIDTH && !(width & 7u); }

uint64_t zngamd_sort_scratch_bytes(uint64_t n, uint32_t width)
{
    if (n > ZNGAMD_SORT_MAX_KEYS || !sort_width_ok(width)) return 0;
    return sort_r8(n * 4u) + sort_r8(n) + sort_tiles(n) * 1024u + 1024u + 2u * width;
}

// n > 0.  OR and AND, [the host waits for them], the order array set to 0 .. n - 1 in the buffer from which the passes end in d_order,
// then per byte position that varies, the last first: hist, scan, scatter; rank.
static int sort_dev(zngamd_ctx *c, const uint8_t *d_keys, uint64_t n, uint32_t W, uint8_t *d_scratch, uint32_t *d_order, uint32_t *d_rank)
{
    const uint32_t tiles = (uint32_t)sort_tiles(n), w8 = W / 8u, n32 = (uint32_t)n, grid_n = (uint32_t)((n + 255u) / 256u);
    uint32_t *other = (uint32_t *)d_scratch;
    uint8_t *dig = d_scratch + sort_r8(n * 4u);
    uint32_t *tab = (uint32_t *)(dig + sort_r8(n)), *dtot = tab + (uint64_t)tiles * 256u;
    unsigned long long *acc = (unsigned long long *)(dtot + 256);
    uint8_t host[2u * ZNGAMD_SORT_MAX_WIDTH];
    HIPCHK(c, hipMemsetAsync(acc, 0, W, c->stream));
    HIPCHK(c, hipMemsetAsync(acc + w8, 0xFF, W, c->stream));
    const uint64_t words = n * w8;
    { ProfScope ps(c, ZNGAMD_K_SCAN);
      hipLaunchKernelGGL(za_k_sort_orand, dim3((uint32_t)std::min<uint64_t>((words + 4095u) / 4096u, 1024u)), dim3(256), 0, c->stream,
                         (const unsigned long long *)d_keys, words, w8, acc); }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(host, acc, 2u * (size_t)W, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint32_t pos[ZNGAMD_SORT_MAX_WIDTH], np = 0;                                         // the byte positions that vary, the last first
    for (uint32_t p = W; p-- > 0;) if (host[p] != host[W + p]) pos[np++] = p;
    uint32_t *src = (np & 1u) ? other : d_order, *dst = (np & 1u) ? d_order : other;
    { ProfScope ps(c, ZNGAMD_K_SCAN);
      hipLaunchKernelGGL(za_k_sort_iota, dim3(grid_n), dim3(256), 0, c->stream, src, n32);
      for (uint32_t i = 0; i < np; i++) {
          hipLaunchKernelGGL(za_k_sort_hist, dim3(tiles), dim3(256), 0, c->stream, d_keys, W, pos[i], (const uint32_t *)src, n32, dig, tab);
          hipLaunchKernelGGL(za_k_sort_scan, dim3(256), dim3(256), 0, c->stream, tab, tiles, dtot);
          hipLaunchKernelGGL(za_k_sort_scatter, dim3(tiles), dim3(256), 0, c->stream, (const uint8_t *)dig, (const uint32_t *)src, n32, (const uint32_t *)tab,
                             (const uint32_t *)dtot, dst);
          std::swap(src, dst);
      }
      if (d_rank) hipLaunchKernelGGL(za_k_sort_rank, dim3(grid_n), dim3(256), 0, c->stream, (const uint32_t *)d_order, n32, d_rank); }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_sort_keys_dev(zngamd_ctx *c, const uint8_t *d_keys, uint64_t n, uint32_t width, void *d_scratch, uint64_t scratch_cap, uint32_t *d_order,
                         uint32_t *d_rank)
try {
    if (n > ZNGAMD_SORT_MAX_KEYS || !sort_width_ok(width) || (n && (!d_keys || !d_order || !d_scratch)) || ((uintptr_t)d_scratch & 7u) ||
        ((uintptr_t)d_keys & 7u)) return ZNGAMD_E_ARG;
    if (!c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (n && scratch_cap < zngamd_sort_scratch_bytes(n, width)) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    if (!n) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int r = sort_dev(c, d_keys, n, width, (uint8_t *)d_scratch, d_order, d_rank);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_sort_keys(zngamd_ctx *c, const uint8_t *keys, uint64_t n, uint32_t width, uint32_t *order, uint32_t *rank)
try {
    if (n > ZNGAMD_SORT_MAX_KEYS || !sort_width_ok(width) || (n && (!keys || !order))) return ZNGAMD_E_ARG;
    if (!c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (!n) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->so_key.ensure(n * (width / 8u))); HIPCHK(c, c->so_tab.ensure(zngamd_sort_scratch_bytes(n, width) / 8u)); HIPCHK(c, c->so_ord.ensure(n));
    if (rank) HIPCHK(c, c->so_rank.ensure(n));
    HIPCHK(c, hipMemcpyAsync(c->so_key.p, keys, (size_t)(n * width), hipMemcpyHostToDevice, c->stream));
    int r = sort_dev(c, (const uint8_t *)c->so_key.p, n, width, (uint8_t *)c->so_tab.p, c->so_ord.p, rank ? c->so_rank.p : nullptr);
    if (r) return r;
    HIPCHK(c, hipMemcpyAsync(order, c->so_ord.p, (size_t)n * 4u, hipMemcpyDeviceToHost, c->stream));
    if (rank) HIPCHK(c, hipMemcpyAsync(rank, c->so_rank.p, (size_t)n * 4u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool place_args_ok(int delim, uint32_t flags, uint32_t record_lines, int32_t first_byte, const uint64_t *dst, const uint32_t *length, uint64_t n,
                          const void *d_out, uint64_t out_cap, const zngamd_bgzf_place_totals *totals)
{
    if (!totals || (flags & ~ZNGAMD_BGZF_GREP_FINAL) || delim < 0 || delim > 255 || !grep_records_ok(record_lines, -1, first_byte)) return false;
    return (!n || (dst && length)) && (d_out || !out_cap);
}

// the lines pass for the delimiters alone, [the host waits for the line count], lines, place, close, [the host waits for the totals].
// own: dst and length are host memory and go to so_dst and so_len once the line count says how many are needed.
static int bgzf_place_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, uint32_t k, int32_t first_byte, uint64_t record_base, bool own, const uint64_t *dst,
                          const uint32_t *length, uint64_t n, uint8_t *d_out, uint64_t out_cap, zngamd_bgzf_place_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    const uint32_t lflags = flags & ZA_GREP_FINAL;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const uint64_t lines = R.lines, nrec = R.nrec;
    const bool all = n >= nrec;                                                          // otherwise nothing is placed: labels_short
    if (own && all) {
        HIPCHK(c, c->so_dst.ensure(nrec)); HIPCHK(c, c->so_len.ensure(nrec));
        HIPCHK(c, hipMemcpyAsync(c->so_dst.p, dst, (size_t)nrec * 8u, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->so_len.p, length, (size_t)nrec * 4u, hipMemcpyHostToDevice, c->stream));
        dst = (const uint64_t *)c->so_dst.p; length = c->so_len.p;
    }
    const uint32_t grid = bgzf_wave_grid(c, nrec, ZA_SORT_WG_PER_CU);
    ZaPlaceTotals *d_tot;
    unsigned long long *d_bad;                                                           // the three faults
    r = bgzf_totals_area(c, c->so_tot, 3u, &d_tot, &d_bad);
    if (r) return r;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      if (all) hipLaunchKernelGGL(za_k_sort_place, dim3(grid), dim3(256), 0, c->stream, w.d_scratch, w.text_end, c->gr_start.p, lines, nrec, k, first_byte, w.delim,
                                  lflags ? 1u : 0u, (const unsigned long long *)dst, length, d_out, out_cap, d_tot);
      hipLaunchKernelGGL(za_k_sort_place_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, n, k, lflags, w.text_end, record_base, d_bad, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, sizeof *totals);
}

int zngamd_bgzf_place_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                  uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines, int32_t first_byte, uint64_t record_base, void *d_scratch,
                                  uint64_t scratch_cap, int32_t *d_status, const uint64_t *d_dst, const uint32_t *d_length, uint64_t n, void *d_out,
                                  uint64_t out_cap, zngamd_bgzf_place_totals *totals)
try {
    if (!place_args_ok(delim, flags, record_lines, first_byte, d_dst, d_length, n, d_out, out_cap, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_place_dev(c, w, flags, record_lines, first_byte, record_base, false, d_dst, d_length, n, (uint8_t *)d_out, out_cap, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_place_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                              uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines, int32_t first_byte, uint64_t record_base, int32_t *status,
                              const uint64_t *dst, const uint32_t *length, uint64_t n, void *d_out, uint64_t out_cap, zngamd_bgzf_place_totals *totals)
try {
    if (!place_args_ok(delim, flags, record_lines, first_byte, dst, length, n, d_out, out_cap, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_place_dev(c, w, flags, record_lines, first_byte, record_base, true, dst, length, n, (uint8_t *)d_out, out_cap, totals);
    if (r) return r;
    return bgzf_host_status(c, status, n_members);
} ZA_ABI_GUARD

// ---- reads screened against reference k-mers (za_screen.hip)
// The set: read-only once made.  The table is its own; everything else a call needs is the context's.
struct zngamd_kmer_set {
    zngamd_ctx *ctx = nullptr;
    zngamd_kmer_set_info info = {};
    ZaKmerSlot *tab = nullptr;
};

// the slots of the table for n insertions: the smallest power of two that is >= 2 n and >= ZA_KMER_MIN_CAP (n <= ZNGAMD_KMER_MAX_POSITIONS)
static uint64_t kmer_cap(uint64_t n)
{
    uint64_t cap = ZA_KMER_MIN_CAP;
    while (cap < 2u * n) cap <<= 1;
    return cap;
}

static bool kmer_rule_ok(uint32_t k, uint32_t flags, uint32_t n_refs)
{
    return k >= 1u && k <= ZNGAMD_KMER_MAX_K && !(flags & ~ZNGAMD_KMER_CANONICAL) && n_refs >= 1u && n_refs <= ZNGAMD_KMER_MAX_REFS;
}

// a set with an empty table of kmer_cap(n) slots in *out (the caller holds the context's mutex); acc = sc_tot[0 .. 2) zeroed
static int kmer_set_new(zngamd_ctx *c, uint32_t k, uint32_t flags, uint32_t n_refs, uint64_t n, zngamd_kmer_set **out)
{
    zngamd_kmer_set *s = new zngamd_kmer_set;
    s->ctx = c; s->info.k = k; s->info.flags = flags; s->info.n_refs = n_refs; s->info.positions = n; s->info.cap = kmer_cap(n);
    *out = s;                                                                       // (the caller frees it when a later step fails)
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMalloc((void **)&s->tab, (size_t)s->info.cap * sizeof(ZaKmerSlot)));
    HIPCHK(c, c->sc_tot.ensure(2));
    HIPCHK(c, hipMemsetAsync(c->sc_tot.p, 0, 16, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_kmer_clear, dim3((uint32_t)((s->info.cap + 255u) / 256u)), dim3(256), 0, c->stream, s->tab, s->info.cap); }
    return ZNGAMD_OK;
}

// [the host waits for the two counts]: valid (unless the caller knows it) and distinct
static int kmer_set_counts(zngamd_ctx *c, zngamd_kmer_set *s, bool valid_too)
{
    unsigned long long acc[2] = {0, 0};
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(acc, c->sc_tot.p, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (valid_too) s->info.valid = acc[0];
    s->info.distinct = acc[1];
    return ZNGAMD_OK;
}

static void kmer_set_drop(zngamd_kmer_set *s)
{
    if (s->tab) (void)hipFree(s->tab);
    delete s;
}

int zngamd_kmer_set_build(zngamd_ctx *c, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_refs, uint32_t k, uint32_t flags, zngamd_kmer_set **out,
                          zngamd_kmer_set_info *info)
try {
    if (!out || !offsets || !kmer_rule_ok(k, flags, n_refs)) return ZNGAMD_E_ARG;
    uint64_t positions = 0;
    for (uint32_t j = 0; j < n_refs; j++) {
        if (offsets[j + 1u] < offsets[j]) return ZNGAMD_E_ARG;
        const uint64_t len = offsets[j + 1u] - offsets[j];
        if (len >= k) positions += len - k + 1u;
        if (positions > ZNGAMD_KMER_MAX_POSITIONS) return ZNGAMD_E_ARG;
    }
    const uint64_t first = offsets[0], bytes = offsets[n_refs] - first;
    if ((bytes && !seqs) || !c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    zngamd_kmer_set *s = nullptr;
    int r = kmer_set_new(c, k, flags, n_refs, positions, &s);
    if (!r && positions) r = [&]() -> int {
        // the references and their offsets (taken from the first one's) behind each other in sc_tmp
        const size_t off_at = (size_t)((bytes + 7u) & ~7ull);
        std::vector<unsigned long long> rel(n_refs + 1u);
        for (uint32_t j = 0; j <= n_refs; j++) rel[j] = offsets[j] - first;
        HIPCHK(c, c->sc_tmp.ensure(off_at + (size_t)(n_refs + 1u) * 8u));
        HIPCHK(c, hipMemcpyAsync(c->sc_tmp.p, seqs + first, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->sc_tmp.p + off_at, rel.data(), rel.size() * 8u, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));                                // (rel leaves with this scope)
        uint64_t longest = 0;
        for (uint32_t j = 0; j < n_refs; j++) longest = std::max<uint64_t>(longest, rel[j + 1u] - rel[j]);
        // four strips to a workgroup; beyond what the device holds at once a wave walks on to its next strip
        const uint64_t slots = (uint64_t)std::max<uint32_t>(c->search_slots, 1u) * ZA_SCREEN_WG_PER_CU;
        const uint32_t gx = (uint32_t)std::min<uint64_t>((longest + 255u) / 256u, slots);
        { ProfScope ps(c, ZNGAMD_K_GATHER);
          hipLaunchKernelGGL(za_k_kmer_insert, dim3(gx, n_refs), dim3(256), 0, c->stream, c->sc_tmp.p, (const unsigned long long *)(c->sc_tmp.p + off_at), k,
                             flags & ZNGAMD_KMER_CANONICAL, s->tab, s->info.cap - 1u, c->sc_tot.p); }
        return ZNGAMD_OK;
    }();
    if (!r) r = kmer_set_counts(c, s, true);
    if (r) { if (s) kmer_set_drop(s); return r; }
    if (info) *info = s->info;
    *out = s;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_set_load(zngamd_ctx *c, uint32_t k, uint32_t flags, uint32_t n_refs, const uint64_t *codes, const uint64_t *masks, uint64_t n,
                         zngamd_kmer_set **out, zngamd_kmer_set_info *info)
try {
    if (!out || !kmer_rule_ok(k, flags, n_refs) || n > ZNGAMD_KMER_MAX_POSITIONS || (n && (!codes || !masks))) return ZNGAMD_E_ARG;
    const uint64_t code_end = 1ull << (2u * k), mask_bad = n_refs == 64u ? 0ull : ~0ull << n_refs;
    for (uint64_t i = 0; i < n; i++) if (codes[i] >= code_end || !masks[i] || (masks[i] & mask_bad)) return ZNGAMD_E_ARG;
    if (!c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    zngamd_kmer_set *s = nullptr;
    int r = kmer_set_new(c, k, flags, n_refs, n, &s);
    if (!r && n) r = [&]() -> int {
        HIPCHK(c, c->sc_tmp.ensure((size_t)n * 16u));
        unsigned long long *d_codes = (unsigned long long *)c->sc_tmp.p, *d_masks = d_codes + n;
        HIPCHK(c, hipMemcpyAsync(d_codes, codes, (size_t)n * 8u, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_masks, masks, (size_t)n * 8u, hipMemcpyHostToDevice, c->stream));
        { ProfScope ps(c, ZNGAMD_K_GATHER);
          hipLaunchKernelGGL(za_k_kmer_load, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, c->stream, d_codes, d_masks, n, s->tab, s->info.cap - 1u, c->sc_tot.p); }
        return ZNGAMD_OK;
    }();
    if (!r) r = kmer_set_counts(c, s, false);
    if (r) { if (s) kmer_set_drop(s); return r; }
    s->info.valid = n;
    if (info) *info = s->info;
    *out = s;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_set_export(zngamd_kmer_set *s, uint64_t *codes, uint64_t *masks, uint64_t cap_pairs, uint64_t *n)
try {
    if (!s || !n || !s->ctx || (cap_pairs && (!codes || !masks))) return ZNGAMD_E_ARG;
    zngamd_ctx *c = s->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    const uint64_t d = s->info.distinct;
    *n = d;
    if (cap_pairs < d) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    if (!d) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->sc_tmp.ensure((size_t)d * 16u)); HIPCHK(c, c->sc_tot.ensure(2));
    unsigned long long *d_codes = (unsigned long long *)c->sc_tmp.p, *d_masks = d_codes + d;
    HIPCHK(c, hipMemsetAsync(c->sc_tot.p, 0, 8, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_kmer_export, dim3((uint32_t)((s->info.cap + 255u) / 256u)), dim3(256), 0, c->stream, s->tab, s->info.cap, d_codes, d_masks, d, c->sc_tot.p); }
    HIPCHK(c, hipGetLastError());
    unsigned long long wrote = 0;
    HIPCHK(c, hipMemcpyAsync(&wrote, c->sc_tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(codes, d_codes, (size_t)d * 8u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(masks, d_masks, (size_t)d * 8u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (wrote != d) return fail(c, ZNGAMD_E_HIP, "the set's table does not hold the codes it was made with");
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_set_describe(const zngamd_kmer_set *s, zngamd_kmer_set_info *info)
{
    if (!s || !info) return ZNGAMD_E_ARG;
    *info = s->info;
    return ZNGAMD_OK;
}

void zngamd_kmer_set_free(zngamd_kmer_set *s)
{
    if (!s) return;
    if (s->ctx) {
        std::lock_guard<std::mutex> g(s->ctx->mu);
        (void)hipSetDevice(s->ctx->device);
        (void)hipStreamSynchronize(s->ctx->stream);                                 // (no launch of this context still reads the table)
        kmer_set_drop(s);
    } else kmer_set_drop(s);
}

// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool screen_args_ok(const zngamd_ctx *c, int delim, uint32_t flags, const zngamd_bgzf_screen_conf *cf, const zngamd_kmer_set *set,
                           const zngamd_bgzf_screen_row *rows, bool alloc, const zngamd_bgzf_screen_totals *totals)
{
    if (!totals || !cf || !set || (flags & ~ZNGAMD_BGZF_GREP_FINAL) || delim < 0 || delim > 255) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte)) return false;
    if (cf->seq_line < 0 || cf->seq_line >= (int32_t)cf->record_lines || cf->flags || !cf->min_hits) return false;
    for (uint32_t v : cf->reserved) if (v) return false;
    return (rows || alloc) && c && set->ctx == c;
}

// The lines pass for the delimiters alone, [the host waits for the line count], lines, screen, close, [the host waits for the totals].
// own: the rows go to sc_row; otherwise to d_rows when rows_cap holds them, and nowhere (*rows_short) when it does not.
static int bgzf_screen_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, const zngamd_bgzf_screen_conf &cf, const zngamd_kmer_set *set,
                           uint64_t record_base, bool own, ZaScreenRow *d_rows, uint64_t rows_cap, bool *rows_short, zngamd_bgzf_screen_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    *rows_short = false;
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const uint64_t lines = R.lines, nrec = R.nrec;
    r = bgzf_rows_dest(c, c->sc_row, nrec, own, &d_rows, rows_cap, rows_short);
    if (r) return r;
    const uint32_t grid = bgzf_wave_grid(c, nrec, ZA_SCREEN_WG_PER_CU);
    const ZaScreenPar P = {k, (uint32_t)cf.seq_line, cf.first_byte, cf.min_hits, w.delim, set->info.k, set->info.flags & ZNGAMD_KMER_CANONICAL};
    ZaScreenTotals *d_tot;
    unsigned long long *d_bad;                                                           // the fault
    r = bgzf_totals_area(c, c->sc_tot, 1u, &d_tot, &d_bad);
    if (r) return r;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_screen, dim3(grid), dim3(256), 0, c->stream, w.d_scratch, w.text_end, c->gr_start.p, lines, nrec, P, (const ZaKmerSlot *)set->tab,
                         set->info.cap - 1u, d_rows, d_tot, d_bad);
      hipLaunchKernelGGL(za_k_rec_close<ZaScreenTotals>, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, d_bad, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, sizeof *totals);
}

int zngamd_bgzf_screen_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                   uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_screen_conf *conf, const zngamd_kmer_set *set,
                                   uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_screen_row *d_rows, uint64_t rows_cap,
                                   zngamd_bgzf_screen_totals *totals)
try {
    if (!screen_args_ok(c, delim, flags, conf, set, d_rows, false, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    bool rows_short = false;
    int r = bgzf_screen_dev(c, w, flags, *conf, set, record_base, false, (ZaScreenRow *)d_rows, rows_cap, &rows_short, totals);
    if (r) return r;
    return bgzf_dev_finish(c, rows_short, totals->bad != 0);
} ZA_ABI_GUARD

int zngamd_bgzf_screen_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                               uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_screen_conf *conf, const zngamd_kmer_set *set,
                               uint64_t record_base, int32_t *status, zngamd_bgzf_screen_row *rows, uint64_t rows_cap, zngamd_alloc_fn alloc, void *user,
                               zngamd_bgzf_screen_totals *totals)
try {
    if (!screen_args_ok(c, delim, flags, conf, set, rows, alloc != nullptr, totals)) return ZNGAMD_E_ARG;
    if ((!in && in_len) || (n_members && (!members || !status)) || (alloc && rows)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    bool rows_short = false;
    r = bgzf_screen_dev(c, w, flags, *conf, set, record_base, true, nullptr, 0, &rows_short, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t seen = totals->seen;
    if (!totals->covered || totals->bad || !seen) return ZNGAMD_OK;
    return bgzf_host_rows(c, alloc, user, rows, rows_cap, c->sc_row.p, seen, sizeof(ZaScreenRow));
} ZA_ABI_GUARD

// ---- the k-mers of the reads counted (za_kcount.hip)
// The counter: the table is its own and grows; everything else a call needs is the context's (sc_tot, sc_tmp).  INVARIANT, checked by
// kcount_room_ok before anything is launched: distinct + room <= cap / 2, where room bounds what the launch can claim.  So at most
// cap / 2 slots are ever claimed and every probe loop of za_kmer_claim ends.
struct zngamd_kmer_counter {
    zngamd_ctx *ctx = nullptr;
    uint32_t k = 0, flags = 0, poisoned = 0;
    uint64_t cap = 0, distinct = 0, total = 0;
    ZaKmerSlot *tab = nullptr;
};

// A launch takes a thread per slot or pair, and a grid holds fewer than 2^32 threads: tables of 2^32 slots and more are cleared,
// rehashed and exported in launches of 2^31 each (the cursor and the claim count go on from launch to launch).
constexpr uint64_t KCOUNT_LAUNCH = 1ull << 31;

static bool kcount_room_ok(const zngamd_kmer_counter *kc, uint64_t room)
{
    const uint64_t half = kc->cap / 2u;
    return room <= half && kc->distinct <= half - room;
}

// the smallest power of two that is >= want and >= ZA_KMER_MIN_CAP (want <= ZNGAMD_KMER_COUNTER_MAX_CAP)
static uint64_t kcount_pow2(uint64_t want)
{
    uint64_t cap = ZA_KMER_MIN_CAP;
    while (cap < want) cap <<= 1;
    return cap;
}

// an empty table of cap slots in *tab (the caller holds the context's mutex); ZNGAMD_MEM_ERROR when the device cannot give it
static int kcount_table(zngamd_ctx *c, uint64_t cap, ZaKmerSlot **tab)
{
    *tab = nullptr;
    HIPCHK(c, hipSetDevice(c->device));
    const hipError_t e = hipMalloc((void **)tab, (size_t)cap * sizeof(ZaKmerSlot));
    if (e != hipSuccess) {
        *tab = nullptr;
        (void)hipGetLastError();
        if (e == hipErrorOutOfMemory) return fail(c, ZNGAMD_MEM_ERROR, "the device cannot give the k-mer table");
        HIPCHK(c, e);
    }
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      for (uint64_t at = 0; at < cap; at += KCOUNT_LAUNCH) {
          const uint64_t m = std::min<uint64_t>(KCOUNT_LAUNCH, cap - at);
          hipLaunchKernelGGL(za_k_kcount_clear, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, c->stream, *tab + at, m);
      } }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

// n pairs (codes[step i], counts[step i]) on the device into tab; [the host waits] *claimed: the slots newly claimed
static int kcount_pairs(zngamd_ctx *c, const unsigned long long *d_codes, const unsigned long long *d_counts, uint64_t n, uint32_t step, ZaKmerSlot *tab, uint64_t cap,
                        uint64_t *claimed)
{
    unsigned long long acc = 0;
    HIPCHK(c, c->sc_tot.ensure(2));
    HIPCHK(c, hipMemsetAsync(c->sc_tot.p, 0, 8, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      for (uint64_t at = 0; at < n; at += KCOUNT_LAUNCH) {
          const uint64_t m = std::min<uint64_t>(KCOUNT_LAUNCH, n - at);
          hipLaunchKernelGGL(za_k_kcount_pairs, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, c->stream, d_codes + at * step, d_counts + at * step, m, step, tab,
                             cap - 1u, c->sc_tot.p);
      } }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(&acc, c->sc_tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    *claimed = acc;
    return ZNGAMD_OK;
}

int zngamd_kmer_counter_new(zngamd_ctx *c, uint32_t k, uint32_t flags, uint64_t room, zngamd_kmer_counter **out)
try {
    if (!out || !kmer_rule_ok(k, flags, 1u) || room > ZNGAMD_KMER_COUNTER_MAX_CAP / 2u || !c) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    zngamd_kmer_counter *kc = new zngamd_kmer_counter;
    kc->ctx = c; kc->k = k; kc->flags = flags; kc->cap = kcount_pow2(2u * room);
    int r = kcount_table(c, kc->cap, &kc->tab);
    if (!r && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, ZNGAMD_E_HIP, "the k-mer table could not be cleared");
    if (r) { if (kc->tab) (void)hipFree(kc->tab); delete kc; return r; }
    *out = kc;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_counter_reserve(zngamd_kmer_counter *kc, uint64_t room)
try {
    if (!kc || !kc->ctx || kc->poisoned) return ZNGAMD_E_ARG;
    zngamd_ctx *c = kc->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    if (kcount_room_ok(kc, room)) return ZNGAMD_OK;
    if (room > ZNGAMD_KMER_COUNTER_MAX_CAP / 4u || kc->distinct + room > ZNGAMD_KMER_COUNTER_MAX_CAP / 4u) return ZNGAMD_E_ARG;
    const uint64_t cap = kcount_pow2(4u * (kc->distinct + room));
    ZaKmerSlot *tab = nullptr;
    int r = kcount_table(c, cap, &tab);
    uint64_t claimed = 0;
    // the rehash: every occupied slot of the old table is a pair; it can claim the old distinct, and distinct <= cap / 4 here
    if (!r && kc->distinct) r = kcount_pairs(c, &kc->tab->code, &kc->tab->mask, kc->cap, 2u, tab, cap, &claimed);
    else if (!r && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, ZNGAMD_E_HIP, "the k-mer table could not be cleared");
    if (!r && claimed != kc->distinct) r = fail(c, ZNGAMD_E_HIP, "the counter's table does not hold the codes it has counted");
    if (r) { if (tab) { (void)hipStreamSynchronize(c->stream); (void)hipFree(tab); } return r; }      // (the counter is as it was)
    (void)hipFree(kc->tab);                                                         // (the stream is drained: nothing reads the old table)
    kc->tab = tab; kc->cap = cap;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_counter_add(zngamd_kmer_counter *kc, const uint64_t *codes, const uint64_t *counts, uint64_t n)
try {
    if (!kc || !kc->ctx || kc->poisoned || (n && (!codes || !counts))) return ZNGAMD_E_ARG;
    const uint64_t code_end = 1ull << (2u * kc->k);
    for (uint64_t i = 0; i < n; i++) if (codes[i] >= code_end || !counts[i]) return ZNGAMD_E_ARG;
    zngamd_ctx *c = kc->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    if (!kcount_room_ok(kc, n)) return fail(c, ZNGAMD_BUF_ERROR, "the k-mer table has no room: reserve first");
    if (!n) return ZNGAMD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->sc_tmp.ensure((size_t)n * 16u));
    unsigned long long *d_codes = (unsigned long long *)c->sc_tmp.p, *d_counts = d_codes + n;
    HIPCHK(c, hipMemcpyAsync(d_codes, codes, (size_t)n * 8u, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_counts, counts, (size_t)n * 8u, hipMemcpyHostToDevice, c->stream));
    uint64_t claimed = 0;
    const int r = kcount_pairs(c, d_codes, d_counts, n, 1u, kc->tab, kc->cap, &claimed);
    if (r) { kc->poisoned = 1; return r; }                                          // (an unknown part of the pairs is in the table)
    kc->distinct += claimed;
    for (uint64_t i = 0; i < n; i++) kc->total += counts[i];
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_counter_describe(const zngamd_kmer_counter *kc, zngamd_kmer_counter_info *info)
{
    if (!kc || !info) return ZNGAMD_E_ARG;
    memset(info, 0, sizeof *info);
    info->k = kc->k; info->flags = kc->flags; info->poisoned = kc->poisoned; info->cap = kc->cap; info->distinct = kc->distinct; info->total = kc->total;
    return ZNGAMD_OK;
}

int zngamd_kmer_counter_histogram(zngamd_kmer_counter *kc, uint64_t *hist, uint32_t bins)
try {
    if (!kc || !kc->ctx || kc->poisoned || !hist || bins < 2u || bins > ZNGAMD_KMER_HIST_MAX_BINS) return ZNGAMD_E_ARG;
    zngamd_ctx *c = kc->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->sc_tot.ensure(bins));
    HIPCHK(c, hipMemsetAsync(c->sc_tot.p, 0, (size_t)bins * 8u, c->stream));
    // a few workgroups per CU, so that the flush stays small: beyond that a workgroup walks on to its next 256 slots
    const uint64_t slots = (uint64_t)std::max<uint32_t>(c->search_slots, 1u) * ZA_KCOUNT_HIST_PER_CU;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((kc->cap + 255u) / 256u, slots);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_kcount_hist, dim3(grid), dim3(256), (size_t)bins * 4u, c->stream, (const ZaKmerSlot *)kc->tab, kc->cap, bins, c->sc_tot.p); }
    HIPCHK(c, hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram words");
    HIPCHK(c, hipMemcpyAsync(hist, c->sc_tot.p, (size_t)bins * 8u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_kmer_counter_export(zngamd_kmer_counter *kc, uint64_t min_count, uint64_t max_count, uint64_t *codes, uint64_t *counts, uint64_t cap_pairs, uint64_t *n)
try {
    if (!kc || !kc->ctx || kc->poisoned || !n || !min_count || (max_count && max_count < min_count) || (cap_pairs && (!codes || !counts))) return ZNGAMD_E_ARG;
    zngamd_ctx *c = kc->ctx;
    std::lock_guard<std::mutex> g(c->mu);
    *n = 0;
    if (!kc->distinct) return ZNGAMD_OK;
    // the kernel counts every pair of the filter and writes those that have a place: room for more than distinct pairs is never used
    const uint64_t room = std::min<uint64_t>(cap_pairs, kc->distinct);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, c->sc_tmp.ensure((size_t)std::max<uint64_t>(room, 1u) * 16u)); HIPCHK(c, c->sc_tot.ensure(2));
    unsigned long long *d_codes = (unsigned long long *)c->sc_tmp.p, *d_counts = d_codes + room;
    HIPCHK(c, hipMemsetAsync(c->sc_tot.p, 0, 8, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      for (uint64_t at = 0; at < kc->cap; at += KCOUNT_LAUNCH) {
          const uint64_t m = std::min<uint64_t>(KCOUNT_LAUNCH, kc->cap - at);
          hipLaunchKernelGGL(za_k_kcount_export, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, c->stream, (const ZaKmerSlot *)kc->tab + at, m,
                             (unsigned long long)min_count, max_count ? (unsigned long long)max_count : ~0ull, d_codes, d_counts, room, c->sc_tot.p);
      } }
    HIPCHK(c, hipGetLastError());
    unsigned long long found = 0;
    HIPCHK(c, hipMemcpyAsync(&found, c->sc_tot.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    if (found > kc->distinct) return fail(c, ZNGAMD_E_HIP, "the counter's table does not hold the codes it has counted");
    *n = found;
    if (found > cap_pairs) return fail(c, ZNGAMD_BUF_ERROR, "destination too small");
    if (!found) return ZNGAMD_OK;
    HIPCHK(c, hipMemcpyAsync(codes, d_codes, (size_t)found * 8u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(counts, d_counts, (size_t)found * 8u, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

void zngamd_kmer_counter_free(zngamd_kmer_counter *kc)
{
    if (!kc) return;
    if (kc->ctx) {
        std::lock_guard<std::mutex> g(kc->ctx->mu);
        (void)hipSetDevice(kc->ctx->device);
        (void)hipStreamSynchronize(kc->ctx->stream);                                // (no launch of this context still touches the table)
        if (kc->tab) (void)hipFree(kc->tab);
    }
    delete kc;
}

// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool count_args_ok(const zngamd_ctx *c, int delim, uint32_t flags, const zngamd_bgzf_count_conf *cf, const zngamd_kmer_counter *kc,
                          const zngamd_bgzf_count_totals *totals)
{
    if (!totals || !cf || !kc || (flags & ~ZNGAMD_BGZF_GREP_FINAL) || delim < 0 || delim > 255) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte)) return false;
    if (cf->seq_line < 0 || cf->seq_line >= (int32_t)cf->record_lines || cf->flags) return false;
    for (uint32_t v : cf->reserved) if (v) return false;
    return c && kc->ctx == c && !kc->poisoned;
}

// The lines pass for the delimiters alone, [the host waits for the line count], lines, reads, close, [the host waits for the totals].
// *started: the reads kernel was launched, so the table may hold a part of the window.
static int bgzf_count_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, const zngamd_bgzf_count_conf &cf, zngamd_kmer_counter *kc, uint64_t record_base,
                          bool *started, zngamd_bgzf_count_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const uint64_t lines = R.lines, nrec = R.nrec;
    const uint32_t grid = bgzf_wave_grid(c, nrec, ZA_KCOUNT_WG_PER_CU);
    const ZaKcountPar P = {k, (uint32_t)cf.seq_line, cf.first_byte, w.delim, kc->k, kc->flags & ZNGAMD_KMER_CANONICAL};
    ZaKcountTotals *d_tot;
    unsigned long long *d_bad;                                                           // the fault
    r = bgzf_totals_area(c, c->sc_tot, 1u, &d_tot, &d_bad);
    if (r) return r;
    *started = true;
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_kcount_reads, dim3(grid), dim3(256), 0, c->stream, w.d_scratch, w.text_end, c->gr_start.p, lines, nrec, P, kc->tab, kc->cap - 1u, d_tot, d_bad);
      hipLaunchKernelGGL(za_k_rec_close<ZaKcountTotals>, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, d_bad, d_tot); }
    return bgzf_totals_read(c, totals, d_tot, sizeof *totals);      // (an error after *started: count_settle sees the code)
}

// what a window call leaves in the counter: the slots it claimed and the positions it counted, or the poison
static int count_settle(zngamd_kmer_counter *kc, int r, bool started, const zngamd_bgzf_count_totals *totals)
{
    if (started && (r || totals->bad)) kc->poisoned = 1;
    else if (!r) { kc->distinct += totals->claimed; kc->total += totals->kmers; }
    return r;
}

int zngamd_bgzf_count_kmers_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_count_conf *conf, zngamd_kmer_counter *kc, uint64_t record_base,
                                void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_count_totals *totals)
try {
    if (!count_args_ok(c, delim, flags, conf, kc, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (!kcount_room_ok(kc, text_end > text_off ? text_end - text_off : 0u)) return fail(c, ZNGAMD_BUF_ERROR, "the k-mer table has no room: reserve first");
    HIPCHK(c, hipSetDevice(c->device));
    bool started = false;
    int r = bgzf_count_dev(c, w, flags, *conf, kc, record_base, &started, totals);
    if (!r && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, ZNGAMD_E_HIP, "hipStreamSynchronize");
    prof_collect(c);
    return count_settle(kc, r, started, totals);
} ZA_ABI_GUARD

int zngamd_bgzf_count_kmers(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                            uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_count_conf *conf, zngamd_kmer_counter *kc, uint64_t record_base,
                            int32_t *status, zngamd_bgzf_count_totals *totals)
try {
    if (!count_args_ok(c, delim, flags, conf, kc, totals)) return ZNGAMD_E_ARG;
    if ((!in && in_len) || (n_members && (!members || !status))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    if (!kcount_room_ok(kc, text_end > text_off ? text_end - text_off : 0u)) return fail(c, ZNGAMD_BUF_ERROR, "the k-mer table has no room: reserve first");
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    bool started = false;
    r = bgzf_count_dev(c, w, flags, *conf, kc, record_base, &started, totals);
    if (!r && n_members && hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        r = fail(c, ZNGAMD_E_HIP, "hipMemcpyAsync of the block statuses");
    if (!r && hipStreamSynchronize(c->stream) != hipSuccess) r = fail(c, ZNGAMD_E_HIP, "hipStreamSynchronize");
    prof_collect(c);
    return count_settle(kc, r, started, totals);
} ZA_ABI_GUARD

// ---- pairs laid over each other (za_overlap.hip)
// Everything the caller gave that needs no context to be judged: before a context is touched or anything is launched.
static bool overlap_args_ok(int delim, uint32_t flags, const zngamd_bgzf_overlap_conf *cf, const zngamd_bgzf_overlap_totals *totals)
{
    if (!totals || !cf || (flags & ~(ZNGAMD_BGZF_GREP_FINAL | ZNGAMD_BGZF_CLASSIFY_GROUP)) || delim < 0 || delim > 255) return false;
    if (!grep_records_ok(cf->record_lines, -1, cf->first_byte) || cf->record_lines < 2u || (cf->record_lines & 1u)) return false;
    const int32_t m = (int32_t)(cf->record_lines / 2u);
    if (cf->seq_line < 0 || cf->seq_line >= m || cf->qual_line < -1 || cf->qual_line >= m || cf->qual_line == cf->seq_line) return false;
    if (cf->quality_base > 255u || cf->min_overlap < 1u || cf->min_overlap > ZNGAMD_BGZF_OVERLAP_MAX_READ || cf->max_mismatch > ZNGAMD_BGZF_OVERLAP_MAX_READ ||
        cf->max_percent > 100u || cf->q_high > ZNGAMD_BGZF_OVERLAP_MAX_QUALITY || cf->q_low > ZNGAMD_BGZF_OVERLAP_MAX_QUALITY) return false;
    if ((cf->flags & ~(ZNGAMD_BGZF_OVERLAP_MERGE | ZNGAMD_BGZF_OVERLAP_CORRECT | ZNGAMD_BGZF_OVERLAP_CUT | ZNGAMD_BGZF_OVERLAP_KEEP_UNMERGED)) ||
        ((cf->flags & ZNGAMD_BGZF_OVERLAP_CORRECT) && cf->qual_line < 0)) return false;
    for (uint32_t r : cf->reserved) if (r) return false;
    return true;
}

// the lines pass for the delimiters alone, [the host waits for the line count], lines, eval, hist, with _GROUP the scan, close, [the
// host waits for the totals], then with _GROUP scatter, offsets and gather, and the overlap rows (own: they stay in ov_row).
static int bgzf_overlap_dev(zngamd_ctx *c, const BgzfWindow &w, uint32_t flags, const zngamd_bgzf_overlap_conf &cf, uint64_t record_base,
                            zngamd_bgzf_overlap_row *d_overlap, uint64_t overlap_cap, BgzfDest dst, zngamd_bgzf_overlap_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    const uint32_t lflags = flags & ZA_GREP_FINAL, k = cf.record_lines, ncls = 2u;
    BgzfRecords R;
    bool done;
    int r = R.open(c, w, flags, k, &totals->covered, &totals->tail_off, &done);
    if (r || done) return r;
    const bool group = (flags & ZA_CLS_GROUP) != 0, keep = (cf.flags & ZA_OVL_KEEP_UNMERGED) != 0;
    const uint64_t lines = R.lines, nrec = R.nrec;
    const uint32_t nwg = (uint32_t)((nrec + ZA_PART_WG_RECORDS - 1u) / ZA_PART_WG_RECORDS);
    const uint64_t ntab = (uint64_t)ncls * nwg;
    constexpr size_t TOT_WORDS = sizeof(ZaOvlTotals) / 8u;                               // then the two faults, the scan's sum, the counts, hist's totals
    HIPCHK(c, c->cl_len.ensure(nrec)); HIPCHK(c, c->cl_tab.ensure(ntab)); HIPCHK(c, c->pt_lab.ensure(nrec));
    HIPCHK(c, c->tb_blk.ensure(ntab / ZA_TBX_SCAN_ITEMS + 2u)); HIPCHK(c, c->ov_row.ensure(nrec));
    HIPCHK(c, c->tr_tot.ensure(TOT_WORDS + 3u + 2u * ncls + sizeof(ZaPartTotals) / 8u));
    const ZaOvlPar P = {k, k / 2u, (uint32_t)cf.seq_line, cf.qual_line, cf.first_byte, cf.quality_base, cf.min_overlap, cf.max_mismatch, cf.max_percent,
                        (int32_t)cf.q_high, (int32_t)cf.q_low, cf.flags, w.delim};
    ZaOvlTotals *d_tot = (ZaOvlTotals *)c->tr_tot.p;
    unsigned long long *d_bad = c->tr_tot.p + TOT_WORDS, *d_sum = d_bad + 2, *d_cnt = d_bad + 3;
    ZaPartTotals *d_ptot = (ZaPartTotals *)(d_cnt + 2u * ncls);
    HIPCHK(c, hipMemsetAsync(c->tr_tot.p, 0, (TOT_WORDS + 3u + 2u * ncls) * 8u + sizeof(ZaPartTotals), c->stream));
    HIPCHK(c, hipMemsetAsync(d_bad, 0xFF, 16, c->stream));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      R.launch_lines(c, w, lflags, k, -1, nullptr, 0);      // (no line matched: the starts alone)
      hipLaunchKernelGGL(za_k_ovl_eval, dim3((uint32_t)((nrec + ZA_OVL_WG_RECORDS - 1u) / ZA_OVL_WG_RECORDS)), dim3(256), 0, c->stream, w.d_scratch, w.text_end,
                         c->gr_start.p, lines, nrec, P, c->ov_row.p, c->cl_len.p, c->pt_lab.p, d_tot);
      hipLaunchKernelGGL(za_k_part_hist, dim3(nwg), dim3(ZA_PART_WG_RECORDS), 0, c->stream, c->pt_lab.p, nrec, c->cl_len.p, nrec, ncls, nwg, c->cl_tab.p, d_cnt, d_ptot);
      if (group) tbx_scan(c, c->cl_tab.p, ntab, ZA_TBX_SUM, d_sum);
      hipLaunchKernelGGL(za_k_ovl_close, dim3(1), dim3(1), 0, c->stream, c->gr_start.p, lines, nrec, k, lflags, w.text_end, record_base, d_cnt, d_bad, d_tot); }
    r = bgzf_totals_read(c, totals, d_tot, sizeof *totals);
    if (r) return r;
    if (totals->bad) return ZNGAMD_OK;
    const uint64_t n = group ? totals->merged + (keep ? totals->seen - totals->merged : 0ull) : 0ull, bytes = group ? totals->bytes : 0ull;
    if (!dst.own && totals->seen > overlap_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    r = bgzf_dest_ready(c, dst, n, bytes);
    if (r) return r;
    if (n) {
        HIPCHK(c, c->gp_lens.ensure(n)); HIPCHK(c, c->st_off.ensure(n));
        uint64_t *d_bytes = (uint64_t *)((uint8_t *)c->d_small + 128);
        { ProfScope ps(c, ZNGAMD_K_GATHER);
          hipLaunchKernelGGL(za_k_part_scatter, dim3(nwg), dim3(ZA_PART_WG_RECORDS), 0, c->stream, c->pt_lab.p, nrec, c->cl_len.p, c->gr_start.p, nrec, k, ncls, nwg,
                             c->cl_tab.p, record_base, dst.d_rows, n, c->gp_lens.p);
          hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(n <= 64 ? 64 : 1024), 0, c->stream, c->gp_lens.p, (uint32_t)n, 0u, 0ull, c->st_off.p, d_bytes,
                             (const ZaUnit *)nullptr);
          hipLaunchKernelGGL(za_k_ovl_gather, dim3((uint32_t)((n + 3u) / 4u)), dim3(256), 0, c->stream, w.d_scratch, c->gr_start.p, lines, record_base, P,
                             c->ov_row.p, dst.d_rows, c->st_off.p, n, dst.d_out, bytes); }
        c->bgzf_stats[2] += n;
        HIPCHK(c, hipGetLastError());
    }
    if (!dst.own) HIPCHK(c, hipMemcpyAsync(d_overlap, c->ov_row.p, (size_t)totals->seen * sizeof(ZaOvlRow), hipMemcpyDeviceToDevice, c->stream));
    return ZNGAMD_OK;
}

int zngamd_bgzf_overlap_records_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                                    uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_overlap_conf *conf, uint64_t record_base, void *d_scratch,
                                    uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_overlap_row *d_overlap, uint64_t overlap_cap,
                                    zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap, zngamd_bgzf_overlap_totals *totals)
try {
    if (!overlap_args_ok(delim, flags, conf, totals)) return ZNGAMD_E_ARG;
    BgzfWindow w;
    if (!c || !bgzf_dev_window(&w, d_in, in_len, d_members, n_members, text_off, text_end, delim, d_scratch, scratch_cap, d_status) || (!d_overlap && overlap_cap) ||
        (!d_rows && rows_cap) || (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_overlap_dev(c, w, flags, *conf, record_base, d_overlap, overlap_cap, {(ZaGrepRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false}, totals);
    if (r) return r;
    return bgzf_dev_finish(c);
} ZA_ABI_GUARD

int zngamd_bgzf_overlap_records(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                                uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_overlap_conf *conf, uint64_t record_base, int32_t *status,
                                zngamd_bgzf_overlap_row *overlap, uint64_t overlap_cap, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out,
                                uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_overlap_totals *totals)
try {
    if (!overlap_args_ok(delim, flags, conf, totals)) return ZNGAMD_E_ARG;
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (!overlap && overlap_cap) || (!rows && rows_cap) || (!out && out_cap) ||
        (alloc && (overlap || rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    BgzfWindow w;
    int r = bgzf_host_window(c, &w, in, in_len, members, n_members, text_off, text_end, delim);
    if (r) return r;
    r = bgzf_overlap_dev(c, w, flags, *conf, record_base, nullptr, 0, {nullptr, 0, nullptr, 0, true}, totals);
    if (!r) r = bgzf_host_status(c, status, n_members);
    if (r) return r;
    const uint64_t seen = totals->seen;
    const bool group = (flags & ZNGAMD_BGZF_CLASSIFY_GROUP) != 0;
    if (!totals->covered || totals->bad || !seen) return ZNGAMD_OK;
    const uint64_t n = group ? totals->merged + ((conf->flags & ZNGAMD_BGZF_OVERLAP_KEEP_UNMERGED) ? seen - totals->merged : 0ull) : 0ull;
    if (alloc) overlap = (zngamd_bgzf_overlap_row *)alloc(user, seen * sizeof(zngamd_bgzf_overlap_row));      // the caller's memory is asked for: overlap rows, rows, bytes
    return bgzf_host_fetch(c, alloc, user, n, totals->bytes, rows, rows_cap, out, out_cap, alloc ? overlap != nullptr : seen <= overlap_cap, n != 0,
                           [&] { HIPCHK(c, hipMemcpyAsync(overlap, c->ov_row.p, (size_t)seen * sizeof(ZaOvlRow), hipMemcpyDeviceToHost, c->stream)); return ZNGAMD_OK; });
} ZA_ABI_GUARD

// ---- fields of a line (za_tabix.hip)
// The configuration as the caller gave it: judged on the host, before a context is touched or anything is launched.
static bool tabix_conf_ok(const zngamd_tabix_conf *cf, int delim)
{
    if (!cf || delim < 0 || delim > 255) return false;
    const int f = cf->format & 0xFFFF;
    if ((cf->format & ~0x1FFFF) || (f != 0 && f != 2)) return false;              // (1 is the SAM preset: it needs CIGAR)
    return cf->col_seq >= 1 && cf->col_beg >= 1 && cf->col_end >= 0 && cf->meta >= 0 && cf->meta <= 255 && cf->skip >= 0;
}

// one inclusive scan of v[0, n) in place (n >= 1); *d_total = the sum or the maximum of all
static void tbx_scan(zngamd_ctx *c, unsigned long long *v, uint64_t n, int op, unsigned long long *d_total)
{
    const uint32_t nb = (uint32_t)((n + ZA_TBX_SCAN_ITEMS - 1u) / ZA_TBX_SCAN_ITEMS);
    hipLaunchKernelGGL(za_k_tbx_reduce, dim3(nb), dim3(256), 0, c->stream, v, n, op, c->tb_blk.p);
    hipLaunchKernelGGL(za_k_tbx_scan_blocks, dim3(1), dim3(1024), 0, c->stream, c->tb_blk.p, nb, op, d_total);
    hipLaunchKernelGGL(za_k_tbx_apply, dim3(nb), dim3(256), 0, c->stream, v, n, op, c->tb_blk.p);
}

// tb_tot, in u64: [0, 8) ZaTbxState, [8, 10) the cover, [10] delimiters, [11] data lines, [12] name runs, [13] bin runs, [14] window rows,
// [15] (the largest key), [16] bytes of the packed names
// decode, cover, mark, offsets, [the host waits for the delimiter count], parse, the scans, [the host waits for the totals], emit,
// finish, offsets, place, gather.  own: the host form (the tables go to the context's buffers, as long as the totals say).
static int bgzf_tabix_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members, uint64_t text_off,
                          uint64_t text_end, const zngamd_tabix_conf *conf, uint32_t delim, uint32_t flags, uint64_t line_base, uint8_t *d_scratch,
                          uint64_t scratch_cap, int32_t *d_status, ZaTbxName *d_names, uint64_t names_cap, uint8_t *d_blob, uint64_t blob_cap,
                          ZaTbxBin *d_bins, uint64_t bins_cap, ZaTbxWin *d_wins, uint64_t wins_cap, bool own, zngamd_bgzf_tabix_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    if (text_off > text_end || text_end > scratch_cap) return fail(c, ZNGAMD_E_ARG, "the text lies outside the scratch");
    if (text_end - text_off >= (1ull << 32)) return fail(c, ZNGAMD_E_ARG, "a text of 4 GiB or more");
    if (line_base >= (1ull << 60)) return fail(c, ZNGAMD_E_ARG, "line_base out of range");
    const uint64_t tile0 = text_off / ZA_TBX_TILE;
    const uint32_t ntiles = text_end > text_off ? (uint32_t)((text_end - 1ull) / ZA_TBX_TILE - tile0 + 1ull) : 0u;
    ZaTbxConf cf;
    memcpy(&cf, conf, sizeof cf);
    HIPCHK(c, c->tb_tot.ensure(32)); HIPCHK(c, c->tb_bits.ensure((size_t)ntiles * 256u + 1u)); HIPCHK(c, c->tb_tcnt.ensure(ntiles + 1u));
    HIPCHK(c, c->tb_tbase.ensure(ntiles + 1u));
    unsigned long long *T = c->tb_tot.p;
    ZaTbxState *d_st = (ZaTbxState *)T;
    c->tb_host.assign(256, 0);
    { ZaTbxState *h = (ZaTbxState *)c->tb_host.data(); h->bad_key = ~0ull; h->tail_off = text_end; }
    HIPCHK(c, hipMemcpyAsync(T, c->tb_host.data(), 256, hipMemcpyHostToDevice, c->stream));
    if (n_members) bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      if (n_members) hipLaunchKernelGGL(za_k_grep_cover, dim3((n_members + 255u) / 256u), dim3(256), 0, c->stream, d_members, d_status, n_members, scratch_cap,
                                        text_off, text_end, T + 8);
      if (ntiles) {
          hipLaunchKernelGGL(za_k_tbx_mark, dim3(ntiles), dim3(256), 0, c->stream, d_scratch, scratch_cap, text_off, text_end, tile0, delim, c->tb_bits.p,
                             c->tb_tcnt.p);
          hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(ntiles <= 64 ? 64 : 1024), 0, c->stream, c->tb_tcnt.p, ntiles, 0u, 0ull, c->tb_tbase.p,
                             (uint64_t *)(T + 10), (const ZaUnit *)nullptr);
      } }
    HIPCHK(c, hipGetLastError());
    unsigned long long h3[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h3, T + 8, sizeof h3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h3[0] != text_end - text_off || h3[1] != 0) { totals->tail_off = text_off; return ZNGAMD_OK; }      // not covered: nothing is reported
    const uint64_t ndelim = h3[2], nl = ndelim + 1ull;
    HIPCHK(c, c->tb_lines.ensure(nl)); HIPCHK(c, c->tb_data.ensure(nl)); HIPCHK(c, c->tb_name.ensure(nl)); HIPCHK(c, c->tb_bin.ensure(nl));
    HIPCHK(c, c->tb_key.ensure(nl)); HIPCHK(c, c->tb_raise.ensure(nl)); HIPCHK(c, c->tb_di.ensure(nl)); HIPCHK(c, c->tb_blk.ensure(nl / ZA_TBX_SCAN_ITEMS + 2u));
    HIPCHK(c, hipMemsetAsync(c->tb_data.p + ndelim, 0, 8, c->stream));
    const uint32_t grid_l = (uint32_t)((nl + 255u) / 256u);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      if (ntiles) hipLaunchKernelGGL(za_k_tbx_parse, dim3(ntiles), dim3(256), 0, c->stream, d_scratch, text_off, text_end, tile0, delim, flags, line_base, cf,
                                     c->tb_bits.p, c->tb_tbase.p, nl, c->tb_lines.p, c->tb_data.p, d_st);
      tbx_scan(c, c->tb_data.p, nl, ZA_TBX_SUM, T + 11);
      hipLaunchKernelGGL(za_k_tbx_compact, dim3(grid_l), dim3(256), 0, c->stream, c->tb_data.p, nl, c->tb_di.p);
      hipLaunchKernelGGL(za_k_tbx_edges, dim3(grid_l), dim3(256), 0, c->stream, d_scratch, c->tb_lines.p, c->tb_di.p, T + 11, nl, line_base, c->tb_name.p,
                         c->tb_bin.p, d_st);
      tbx_scan(c, c->tb_name.p, nl, ZA_TBX_SUM, T + 12);
      tbx_scan(c, c->tb_bin.p, nl, ZA_TBX_SUM, T + 13);
      hipLaunchKernelGGL(za_k_tbx_keys, dim3(grid_l), dim3(256), 0, c->stream, c->tb_lines.p, c->tb_di.p, T + 11, nl, c->tb_name.p, c->tb_key.p);
      tbx_scan(c, c->tb_key.p, nl, ZA_TBX_MAX, T + 15);
      hipLaunchKernelGGL(za_k_tbx_raise, dim3(grid_l), dim3(256), 0, c->stream, c->tb_key.p, T + 11, nl, c->tb_raise.p);
      tbx_scan(c, c->tb_raise.p, nl, ZA_TBX_SUM, T + 14); }
    HIPCHK(c, hipGetLastError());
    unsigned long long H[16];
    HIPCHK(c, hipMemcpyAsync(H, T, sizeof H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ZaTbxState st;
    memcpy(&st, H, sizeof st);
    totals->covered = 1; totals->seen = ndelim + st.final_line; totals->data = H[11]; totals->tail_off = st.tail_off;
    if (st.bad_key != ~0ull) {                            // a bad line: where it starts
        totals->bad_kind = (uint32_t)(st.bad_key & 7u); totals->bad_line = st.bad_key >> 3;
        const uint64_t k = totals->bad_line - line_base;
        if (k >= nl) return fail(c, ZNGAMD_E_ARG, "bad line out of range");
        HIPCHK(c, hipMemcpyAsync(&totals->bad_src, &c->tb_lines.p[k].start, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    const uint64_t nd = H[11];
    if (!nd) return ZNGAMD_OK;
    totals->first_line = st.first_line; totals->first_src = st.first_src; totals->first_beg = st.first_beg; totals->last_beg = st.last_beg;
    totals->n_names = H[12]; totals->name_bytes = st.name_bytes; totals->n_bins = H[13]; totals->n_wins = H[14];
    const uint64_t nn = H[12], nb = H[13], nw = H[14];
    if (own) {
        HIPCHK(c, c->tb_names.ensure(nn)); HIPCHK(c, c->tb_bins.ensure(nb)); HIPCHK(c, c->tb_wins.ensure(nw)); HIPCHK(c, c->bg_out.ensure(st.name_bytes + 64));
        d_names = c->tb_names.p; names_cap = nn; d_bins = c->tb_bins.p; bins_cap = nb; d_wins = c->tb_wins.p; wins_cap = nw; d_blob = c->bg_out.p; blob_cap = st.name_bytes;
    } else if (nn > names_cap || nb > bins_cap || nw > wins_cap || st.name_bytes > blob_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    HIPCHK(c, c->tb_lens.ensure(nn)); HIPCHK(c, c->st_off.ensure(nn)); HIPCHK(c, c->bg_slices.ensure(nn + 1)); HIPCHK(c, c->bg_sstat.ensure(nn + 1));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_tbx_emit, dim3((uint32_t)((nd + 255u) / 256u)), dim3(256), 0, c->stream, c->tb_lines.p, c->tb_di.p, nd, line_base, c->tb_name.p,
                         c->tb_bin.p, c->tb_key.p, c->tb_raise.p, d_names, nn, c->tb_lens.p, d_bins, nb, d_wins, nw);
      hipLaunchKernelGGL(za_k_tbx_finish, dim3((uint32_t)((nb + 255u) / 256u)), dim3(256), 0, c->stream, d_bins, nb, c->tb_lines.p, c->tb_di.p, nd);
      hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(nn <= 64 ? 64 : 1024), 0, c->stream, c->tb_lens.p, (uint32_t)nn, 0u, 0ull, c->st_off.p, (uint64_t *)(T + 16),
                         (const ZaUnit *)nullptr);
      hipLaunchKernelGGL(za_k_tbx_place, dim3((uint32_t)((nn + 255u) / 256u)), dim3(256), 0, c->stream, d_names, c->st_off.p, nn, c->bg_slices.p);
      if (st.name_bytes) hipLaunchKernelGGL(za_k_slice_gather, dim3((uint32_t)nn), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members,
                                            c->bg_slices.p, d_blob, st.name_bytes, c->bg_sstat.p); }
    c->bgzf_stats[2] += nn;
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_bgzf_tabix_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                          uint64_t text_end, const zngamd_tabix_conf *conf, int delim, uint32_t flags, uint64_t line_base, void *d_scratch,
                          uint64_t scratch_cap, int32_t *d_status, zngamd_tabix_name *d_names, uint64_t names_cap, void *d_blob, uint64_t blob_cap,
                          zngamd_tabix_bin *d_bins, uint64_t bins_cap, zngamd_tabix_win *d_wins, uint64_t wins_cap, zngamd_bgzf_tabix_totals *totals)
try {
    if (!tabix_conf_ok(conf, delim)) return ZNGAMD_E_ARG;
    if (!c || !totals || (flags & ~ZNGAMD_BGZF_TABIX_FINAL) || (n_members && (!d_in || !d_members || !d_status)) || (!d_scratch && scratch_cap) ||
        (!d_names && names_cap) || (!d_blob && blob_cap) || (!d_bins && bins_cap) || (!d_wins && wins_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_tabix_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, text_off, text_end, conf, (uint32_t)delim, flags, line_base,
                           (uint8_t *)d_scratch, scratch_cap, d_status, (ZaTbxName *)d_names, names_cap, (uint8_t *)d_blob, blob_cap, (ZaTbxBin *)d_bins, bins_cap,
                           (ZaTbxWin *)d_wins, wins_cap, false, totals);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_tabix(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                      uint64_t text_end, const zngamd_tabix_conf *conf, int delim, uint32_t flags, uint64_t line_base, int32_t *status,
                      zngamd_tabix_name *names, uint64_t names_cap, uint8_t *blob, uint64_t blob_cap, zngamd_tabix_bin *bins, uint64_t bins_cap,
                      zngamd_tabix_win *wins, uint64_t wins_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_tabix_totals *totals)
try {
    if (!tabix_conf_ok(conf, delim)) return ZNGAMD_E_ARG;
    if (!c || !totals || (flags & ~ZNGAMD_BGZF_TABIX_FINAL) || (!in && in_len) || (n_members && (!members || !status)) || (!names && names_cap) ||
        (!blob && blob_cap) || (!bins && bins_cap) || (!wins && wins_cap) || (alloc && (names || blob || bins || wins))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    r = bgzf_tabix_dev(c, c->st_in.p, in_len, c->members.p, n_members, text_off, text_end, conf, (uint32_t)delim, flags, line_base, c->st_out.p, scratch,
                       c->mstatus.p, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0, true, totals);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    const uint64_t nn = totals->n_names, nb = totals->n_bins, nw = totals->n_wins, by = totals->name_bytes;
    if (!totals->covered || !nn) return ZNGAMD_OK;
    if (alloc) {                                          // the sizes are known: the caller's memory is asked for now
        names = (zngamd_tabix_name *)alloc(user, nn * sizeof(ZaTbxName));
        blob = names && by ? (uint8_t *)alloc(user, by) : nullptr;
        bins = names && (blob || !by) ? (zngamd_tabix_bin *)alloc(user, nb * sizeof(ZaTbxBin)) : nullptr;
        wins = bins ? (zngamd_tabix_win *)alloc(user, nw * sizeof(ZaTbxWin)) : nullptr;
        if (!names || (by && !blob) || !bins || !wins) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned no memory");
    } else if (nn > names_cap || nb > bins_cap || nw > wins_cap || by > blob_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    HIPCHK(c, hipMemcpyAsync(names, c->tb_names.p, (size_t)nn * sizeof(ZaTbxName), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bins, c->tb_bins.p, (size_t)nb * sizeof(ZaTbxBin), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(wins, c->tb_wins.p, (size_t)nw * sizeof(ZaTbxWin), hipMemcpyDeviceToHost, c->stream));
    if (by) HIPCHK(c, hipMemcpyAsync(blob, c->bg_out.p, by, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

static bool fetch_regions_ok(const uint8_t *names, uint32_t names_len, const zngamd_tabix_region *regions, uint32_t n_regions)
{
    if (!regions || (!names && names_len) || n_regions < 1 || n_regions > ZNGAMD_BGZF_FETCH_MAX_REGIONS) return false;
    for (uint32_t i = 0; i < n_regions; i++)
        if (regions[i].name_off > names_len || names_len - regions[i].name_off < regions[i].name_len) return false;
    return true;
}

// decode, count per span, offsets, [the host waits for the totals], emit, offsets, place, gather
static int bgzf_fetch_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members, const zngamd_tabix_conf *conf,
                          uint32_t delim, uint32_t flags, const uint8_t *names, uint32_t names_len, const zngamd_tabix_region *regions, uint32_t n_regions,
                          const ZaTbxSpan *d_spans, uint32_t n_spans, uint8_t *d_scratch, uint64_t scratch_cap, int32_t *d_status, int32_t *d_span_status,
                          uint32_t *d_span_rows, ZaTbxRow *d_rows, uint64_t rows_cap, uint8_t *d_out, uint64_t out_cap, bool own, zngamd_bgzf_fetch_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    if (n_spans >= (1u << 31)) return fail(c, ZNGAMD_E_ARG, "too many spans");
    ZaTbxConf cf;
    memcpy(&cf, conf, sizeof cf);
    const size_t tab = (size_t)n_regions * sizeof(ZaTbxRegion);
    c->tb_host.assign(tab + names_len + 1u, 0);
    memcpy(c->tb_host.data(), regions, tab);
    if (names_len) memcpy(c->tb_host.data() + tab, names, names_len);
    HIPCHK(c, c->tb_par.ensure(c->tb_host.size())); HIPCHK(c, c->tb_tot.ensure(32)); HIPCHK(c, c->tb_sbase.ensure(n_spans + 1u));
    HIPCHK(c, hipMemcpyAsync(c->tb_par.p, c->tb_host.data(), c->tb_host.size(), hipMemcpyHostToDevice, c->stream));
    unsigned long long *T = c->tb_tot.p;                 // [0] bytes, [1] rows, [2] bytes again (the offsets of the lines)
    HIPCHK(c, hipMemsetAsync(T, 0, 256, c->stream));
    if (n_members) bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
    const ZaTbxRegion *d_reg = (const ZaTbxRegion *)c->tb_par.p;
    const uint8_t *d_nm = c->tb_par.p + tab;
    if (n_spans) {
        ProfScope ps(c, ZNGAMD_K_GATHER);
        hipLaunchKernelGGL(za_k_tbx_fetch<false>, dim3(n_spans), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, d_spans, d_reg,
                           n_regions, d_nm, cf, delim, d_span_status, d_span_rows, T, (const uint64_t *)nullptr, (ZaTbxRow *)nullptr, 0ull, (uint32_t *)nullptr);
        hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(n_spans <= 64 ? 64 : 1024), 0, c->stream, d_span_rows, n_spans, 0u, 0ull, c->tb_sbase.p,
                           (uint64_t *)(T + 1), (const ZaUnit *)nullptr);
    }
    HIPCHK(c, hipGetLastError());
    unsigned long long H[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(H, T, sizeof H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    totals->bytes = H[0]; totals->matched = H[1];
    const uint64_t n = H[1];
    if ((flags & ZNGAMD_BGZF_FETCH_COUNT_ONLY) || !n) return ZNGAMD_OK;
    if (n >= (1ull << 32)) return fail(c, ZNGAMD_E_ARG, "2^32 rows or more");
    if (own) {
        HIPCHK(c, c->tb_rows.ensure(n)); HIPCHK(c, c->bg_out.ensure(H[0] + 64));
        d_rows = c->tb_rows.p; rows_cap = n; d_out = c->bg_out.p; out_cap = H[0];
    } else if (n > rows_cap || H[0] > out_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    HIPCHK(c, c->tb_lens.ensure(n)); HIPCHK(c, c->st_off.ensure(n)); HIPCHK(c, c->bg_slices.ensure(n + 1)); HIPCHK(c, c->bg_sstat.ensure(n + 1));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_tbx_fetch<true>, dim3(n_spans), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, d_spans, d_reg,
                         n_regions, d_nm, cf, delim, d_span_status, d_span_rows, T, (const uint64_t *)c->tb_sbase.p, d_rows, n, c->tb_lens.p);
      hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(n <= 64 ? 64 : 1024), 0, c->stream, c->tb_lens.p, (uint32_t)n, 0u, 0ull, c->st_off.p, (uint64_t *)(T + 2),
                         (const ZaUnit *)nullptr);
      hipLaunchKernelGGL(za_k_tbx_place_rows, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, c->stream, d_rows, c->st_off.p, n, c->bg_slices.p);
      hipLaunchKernelGGL(za_k_slice_gather, dim3((uint32_t)n), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, c->bg_slices.p,
                         d_out, H[0], c->bg_sstat.p); }
    c->bgzf_stats[2] += n;
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_bgzf_fetch_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, const zngamd_tabix_conf *conf,
                          int delim, uint32_t flags, const uint8_t *names, uint32_t names_len, const zngamd_tabix_region *regions, uint32_t n_regions,
                          const zngamd_tabix_span *d_spans, uint32_t n_spans, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, int32_t *d_span_status,
                          uint32_t *d_span_rows, zngamd_tabix_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap, zngamd_bgzf_fetch_totals *totals)
try {
    if (!tabix_conf_ok(conf, delim) || !fetch_regions_ok(names, names_len, regions, n_regions)) return ZNGAMD_E_ARG;
    if (!c || !totals || (flags & ~ZNGAMD_BGZF_FETCH_COUNT_ONLY) || (n_members && (!d_in || !d_members || !d_status)) || (!d_scratch && scratch_cap) ||
        (n_spans && (!d_spans || !d_span_status || !d_span_rows)) || (!d_rows && rows_cap) || (!d_out && out_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_fetch_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, conf, (uint32_t)delim, flags, names, names_len, regions,
                           n_regions, (const ZaTbxSpan *)d_spans, n_spans, (uint8_t *)d_scratch, scratch_cap, d_status, d_span_status, d_span_rows,
                           (ZaTbxRow *)d_rows, rows_cap, (uint8_t *)d_out, out_cap, false, totals);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_fetch(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, const zngamd_tabix_conf *conf,
                      int delim, uint32_t flags, const uint8_t *names, uint32_t names_len, const zngamd_tabix_region *regions, uint32_t n_regions,
                      const zngamd_tabix_span *spans, uint32_t n_spans, int32_t *status, int32_t *span_status, uint32_t *span_rows, zngamd_tabix_row *rows,
                      uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_fetch_totals *totals)
try {
    if (!tabix_conf_ok(conf, delim) || !fetch_regions_ok(names, names_len, regions, n_regions)) return ZNGAMD_E_ARG;
    if (!c || !totals || (flags & ~ZNGAMD_BGZF_FETCH_COUNT_ONLY) || (!in && in_len) || (n_members && (!members || !status)) ||
        (n_spans && (!spans || !span_status || !span_rows)) || (!rows && rows_cap) || (!out && out_cap) || (alloc && (rows || out))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    HIPCHK(c, c->tb_spans.ensure(n_spans + 1u)); HIPCHK(c, c->tb_sstat.ensure(n_spans + 1u)); HIPCHK(c, c->tb_srows.ensure(n_spans + 1u));
    if (n_spans) HIPCHK(c, hipMemcpyAsync(c->tb_spans.p, spans, (size_t)n_spans * sizeof(ZaTbxSpan), hipMemcpyHostToDevice, c->stream));
    r = bgzf_fetch_dev(c, c->st_in.p, in_len, c->members.p, n_members, conf, (uint32_t)delim, flags, names, names_len, regions, n_regions, c->tb_spans.p, n_spans,
                       c->st_out.p, scratch, c->mstatus.p, c->tb_sstat.p, c->tb_srows.p, nullptr, 0, nullptr, 0, true, totals);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_spans) {
        HIPCHK(c, hipMemcpyAsync(span_status, c->tb_sstat.p, (size_t)n_spans * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(span_rows, c->tb_srows.p, (size_t)n_spans * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    const uint64_t n = totals->matched;
    if ((flags & ZNGAMD_BGZF_FETCH_COUNT_ONLY) || !n) return ZNGAMD_OK;
    if (alloc) {                                          // the sizes are known: the caller's memory is asked for now, rows first
        rows = (zngamd_tabix_row *)alloc(user, n * sizeof(ZaTbxRow));
        out = rows ? (uint8_t *)alloc(user, totals->bytes) : nullptr;
        if (!rows || !out) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned no memory");
    } else if (n > rows_cap || totals->bytes > out_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    HIPCHK(c, hipMemcpyAsync(rows, c->tb_rows.p, (size_t)n * sizeof(ZaTbxRow), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return d2h_payload(c, out, c->bg_out.p, totals->bytes);
} ZA_ABI_GUARD

// ---- records of a FASTA (za_faidx.hip)
// tb_tot, in u64: [0, 11) ZaFaiState, [12, 14) the cover, [14] '\n', [15] records, [16] non-empty sequence lines, [17] bases, [18] bytes of
// the packed names, [20, 24) the carry that came in
// decode, cover, mark, offsets, [the host waits for the '\n' count], starts, bytes, classify, three scans, heads, ends, judge, close,
// [the host waits for the totals], emit, offsets, place, gather.  own: the host form (rows and names go to the context's buffers).
static int bgzf_faidx_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members, uint64_t text_off,
                          uint64_t text_end, uint32_t flags, uint64_t line_base, const zngamd_faidx_carry *carry, uint8_t *d_scratch, uint64_t scratch_cap,
                          int32_t *d_status, ZaFaiRow *d_rows, uint64_t rows_cap, uint8_t *d_blob, uint64_t blob_cap, bool own, zngamd_bgzf_faidx_totals *totals)
{
    memset(totals, 0, sizeof *totals);
    if (text_off > text_end || text_end > scratch_cap) return fail(c, ZNGAMD_E_ARG, "the text lies outside the scratch");
    if (text_end - text_off >= (1ull << 32)) return fail(c, ZNGAMD_E_ARG, "a text of 4 GiB or more");
    if (line_base >= (1ull << 60)) return fail(c, ZNGAMD_E_ARG, "line_base out of range");
    const uint64_t tile0 = text_off / ZA_TBX_TILE;
    const uint32_t ntiles = text_end > text_off ? (uint32_t)((text_end - 1ull) / ZA_TBX_TILE - tile0 + 1ull) : 0u;
    HIPCHK(c, c->tb_tot.ensure(32)); HIPCHK(c, c->tb_bits.ensure((size_t)ntiles * 256u + 1u)); HIPCHK(c, c->fa_x.ensure((size_t)ntiles * 256u + 1u));
    HIPCHK(c, c->tb_tcnt.ensure(ntiles + 1u)); HIPCHK(c, c->tb_tbase.ensure(ntiles + 1u));
    unsigned long long *T = c->tb_tot.p;
    ZaFaiState *d_st = (ZaFaiState *)T;
    const ZaFaiCarry *d_cin = (const ZaFaiCarry *)(T + 20);
    c->tb_host.assign(256, 0);
    { ZaFaiState *h = (ZaFaiState *)c->tb_host.data(); h->bad_key = ~0ull; h->tail_off = text_end;
      if (carry) memcpy(c->tb_host.data() + 160, carry, sizeof *carry); }
    HIPCHK(c, hipMemcpyAsync(T, c->tb_host.data(), 256, hipMemcpyHostToDevice, c->stream));
    if (n_members) bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      if (n_members) hipLaunchKernelGGL(za_k_grep_cover, dim3((n_members + 255u) / 256u), dim3(256), 0, c->stream, d_members, d_status, n_members, scratch_cap,
                                        text_off, text_end, T + 12);
      if (ntiles) {
          hipLaunchKernelGGL(za_k_fai_mark, dim3(ntiles), dim3(256), 0, c->stream, d_scratch, scratch_cap, text_off, text_end, tile0, c->tb_bits.p, c->fa_x.p,
                             c->tb_tcnt.p);
          hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(ntiles <= 64 ? 64 : 1024), 0, c->stream, c->tb_tcnt.p, ntiles, 0u, 0ull, c->tb_tbase.p,
                             (uint64_t *)(T + 14), (const ZaUnit *)nullptr);
      } }
    HIPCHK(c, hipGetLastError());
    unsigned long long h3[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(h3, T + 12, sizeof h3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h3[0] != text_end - text_off || h3[1] != 0) { totals->tail_off = text_off; if (carry) memcpy(&totals->carry, carry, sizeof *carry); return ZNGAMD_OK; }      // not covered: nothing is reported
    const uint64_t ndelim = h3[2], nl = ndelim + 1ull;
    if (nl >= 0xFFFFFFF0ull) return fail(c, ZNGAMD_E_ARG, "2^32 lines or more");
    HIPCHK(c, c->fa_start.ensure(nl + 2u)); HIPCHK(c, c->fa_bw.ensure(nl)); HIPCHK(c, c->tb_data.ensure(nl)); HIPCHK(c, c->tb_name.ensure(nl)); HIPCHK(c, c->tb_bin.ensure(nl));
    HIPCHK(c, c->fa_hline.ensure(nl + 2u)); HIPCHK(c, c->fa_first.ensure(nl + 2u)); HIPCHK(c, c->fa_last.ensure(nl + 2u)); HIPCHK(c, c->tb_lens.ensure(nl + 2u));
    HIPCHK(c, c->tb_blk.ensure(nl / ZA_TBX_SCAN_ITEMS + 2u));
    HIPCHK(c, hipMemsetAsync(c->fa_first.p, 0xFF, (nl + 2u) * 4u, c->stream)); HIPCHK(c, hipMemsetAsync(c->fa_last.p, 0xFF, (nl + 2u) * 4u, c->stream));
    const uint32_t grid_l = (uint32_t)((nl + 255u) / 256u);
    uint64_t nj = ndelim;                                 // the lines this call judges: with _FINAL the bytes behind the last '\n' are one
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      if (ntiles) hipLaunchKernelGGL(za_k_fai_starts, dim3(ntiles), dim3(256), 0, c->stream, text_off, text_end, tile0, c->tb_bits.p, c->tb_tbase.p, ndelim,
                                     c->fa_start.p); }
    if ((flags & ZA_FAI_FINAL) && ntiles) {               // (is there a byte behind the last '\n'?  one u64 more)
        uint64_t last_start = 0;
        HIPCHK(c, hipMemcpyAsync(&last_start, c->fa_start.p + ndelim, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (last_start < text_end) nj = ndelim + 1ull;
    }
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      if (nj) {
          hipLaunchKernelGGL(za_k_fai_bytes, dim3(ntiles), dim3(256), 0, c->stream, d_scratch, text_end, c->tb_bits.p, c->fa_x.p, c->tb_tbase.p, c->fa_start.p, nj,
                             line_base, d_st);
          hipLaunchKernelGGL(za_k_fai_classify, dim3(grid_l), dim3(256), 0, c->stream, d_scratch, text_off, text_end, c->fa_start.p, ndelim, nj, nl, line_base,
                             c->tb_data.p, c->tb_name.p, c->tb_bin.p, c->fa_bw.p, d_st);
          tbx_scan(c, c->tb_data.p, nl, ZA_TBX_SUM, T + 15);
          tbx_scan(c, c->tb_name.p, nl, ZA_TBX_SUM, T + 16);
          tbx_scan(c, c->tb_bin.p, nl, ZA_TBX_SUM, T + 17);
          hipLaunchKernelGGL(za_k_fai_heads, dim3(grid_l), dim3(256), 0, c->stream, d_scratch, c->fa_start.p, c->tb_data.p, c->fa_bw.p, nj, c->fa_hline.p,
                             c->tb_lens.p, d_st);
          hipLaunchKernelGGL(za_k_fai_ends, dim3(grid_l), dim3(256), 0, c->stream, c->tb_data.p, c->tb_name.p, c->fa_hline.p, nj, T + 15, c->fa_first.p,
                             c->fa_last.p);
          hipLaunchKernelGGL(za_k_fai_judge, dim3(grid_l), dim3(256), 0, c->stream, c->tb_data.p, c->tb_name.p, c->fa_bw.p, c->fa_hline.p, c->fa_first.p, nj,
                             line_base, flags, T + 15, d_cin, d_st);
      }
      hipLaunchKernelGGL(za_k_fai_close, dim3(1), dim3(64), 0, c->stream, c->tb_name.p, c->tb_bin.p, c->fa_bw.p, c->fa_start.p, c->fa_hline.p, c->fa_first.p,
                         c->fa_last.p, ndelim, nj, text_off, text_end, line_base, flags, T + 15, d_cin, d_st); }
    HIPCHK(c, hipGetLastError());
    unsigned long long H[18];
    HIPCHK(c, hipMemcpyAsync(H, T, sizeof H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ZaFaiState st;
    memcpy(&st, H, sizeof st);
    totals->covered = 1; totals->seen = st.seen; totals->records = st.records; totals->tail_off = st.tail_off; totals->head_bases = st.head_bases;
    totals->name_bytes = st.name_bytes; totals->head_line_bases = st.head_fb; totals->head_line_width = st.head_fw;
    memcpy(&totals->carry, &st.out, sizeof st.out);
    if (st.bad_key != ~0ull) {                            // a bad line: where it starts (a line of a window in front: ~0, the caller knows)
        totals->bad_kind = (uint32_t)(st.bad_key & 7u); totals->bad_line = st.bad_key >> 3; totals->bad_src = ~0ull;
        if (totals->bad_line >= line_base) {
            const uint64_t k = totals->bad_line - line_base;
            if (k >= nl) return fail(c, ZNGAMD_E_ARG, "bad line out of range");
            HIPCHK(c, hipMemcpyAsync(&totals->bad_src, c->fa_start.p + k, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
    }
    const uint64_t nr = st.records;
    if (!nr) return ZNGAMD_OK;
    if (nr > nl) return fail(c, ZNGAMD_E_ARG, "records out of range");
    if (own) {
        HIPCHK(c, c->fa_rows.ensure(nr)); HIPCHK(c, c->bg_out.ensure(st.name_bytes + 64));
        d_rows = c->fa_rows.p; rows_cap = nr; d_blob = c->bg_out.p; blob_cap = st.name_bytes;
    } else if (nr > rows_cap || st.name_bytes > blob_cap) { prof_collect(c); return fail(c, ZNGAMD_BUF_ERROR, "destination too small"); }
    HIPCHK(c, c->st_off.ensure(nr)); HIPCHK(c, c->bg_slices.ensure(nr + 1)); HIPCHK(c, c->bg_sstat.ensure(nr + 1));
    { ProfScope ps(c, ZNGAMD_K_GATHER);
      hipLaunchKernelGGL(za_k_fai_emit, dim3((uint32_t)((nr + 255u) / 256u)), dim3(256), 0, c->stream, c->fa_start.p, c->tb_bin.p, c->fa_bw.p, c->fa_hline.p,
                         c->fa_first.p, c->tb_lens.p, nr, nj, text_end, line_base, H[17], d_rows, nr);
      hipLaunchKernelGGL(za_k_offsets, dim3(1), dim3(nr <= 64 ? 64 : 1024), 0, c->stream, c->tb_lens.p, (uint32_t)nr, 0u, 0ull, c->st_off.p, (uint64_t *)(T + 18),
                         (const ZaUnit *)nullptr);
      hipLaunchKernelGGL(za_k_fai_place, dim3((uint32_t)((nr + 255u) / 256u)), dim3(256), 0, c->stream, d_rows, c->st_off.p, nr, c->bg_slices.p);
      if (st.name_bytes) hipLaunchKernelGGL(za_k_slice_gather, dim3((uint32_t)nr), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members,
                                            c->bg_slices.p, d_blob, st.name_bytes, c->bg_sstat.p); }
    c->bgzf_stats[2] += nr;
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_bgzf_faidx_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members, uint64_t text_off,
                          uint64_t text_end, int delim, uint32_t flags, uint64_t line_base, const zngamd_faidx_carry *carry, void *d_scratch,
                          uint64_t scratch_cap, int32_t *d_status, zngamd_faidx_row *d_rows, uint64_t rows_cap, void *d_blob, uint64_t blob_cap,
                          zngamd_bgzf_faidx_totals *totals)
try {
    if (delim != 10 || (flags & ~ZNGAMD_BGZF_FAIDX_FINAL)) return ZNGAMD_E_ARG;
    if (!c || !totals || (n_members && (!d_in || !d_members || !d_status)) || (!d_scratch && scratch_cap) || (!d_rows && rows_cap) ||
        (!d_blob && blob_cap)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_faidx_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, text_off, text_end, flags, line_base, carry,
                           (uint8_t *)d_scratch, scratch_cap, d_status, (ZaFaiRow *)d_rows, rows_cap, (uint8_t *)d_blob, blob_cap, false, totals);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_faidx(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members, uint64_t text_off,
                      uint64_t text_end, int delim, uint32_t flags, uint64_t line_base, const zngamd_faidx_carry *carry, int32_t *status,
                      zngamd_faidx_row *rows, uint64_t rows_cap, uint8_t *blob, uint64_t blob_cap, zngamd_alloc_fn alloc, void *user,
                      zngamd_bgzf_faidx_totals *totals)
try {
    if (delim != 10 || (flags & ~ZNGAMD_BGZF_FAIDX_FINAL)) return ZNGAMD_E_ARG;
    if (!c || !totals || (!in && in_len) || (n_members && (!members || !status)) || (!rows && rows_cap) || (!blob && blob_cap) ||
        (alloc && (rows || blob))) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    r = bgzf_faidx_dev(c, c->st_in.p, in_len, c->members.p, n_members, text_off, text_end, flags, line_base, carry, c->st_out.p, scratch, c->mstatus.p,
                       nullptr, 0, nullptr, 0, true, totals);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    const uint64_t nr = totals->records, by = totals->name_bytes;
    if (!totals->covered || !nr) return ZNGAMD_OK;
    if (alloc) {                                          // the sizes are known: the caller's memory is asked for now, rows first
        rows = (zngamd_faidx_row *)alloc(user, nr * sizeof(ZaFaiRow));
        blob = rows && by ? (uint8_t *)alloc(user, by) : nullptr;
        if (!rows || (by && !blob)) return fail(c, ZNGAMD_MEM_ERROR, "the caller's allocator returned no memory");
    } else if (nr > rows_cap || by > blob_cap) return fail(c, ZNGAMD_BUF_ERROR, "output buffer too small");
    HIPCHK(c, hipMemcpyAsync(rows, c->fa_rows.p, (size_t)nr * sizeof(ZaFaiRow), hipMemcpyDeviceToHost, c->stream));
    if (by) HIPCHK(c, hipMemcpyAsync(blob, c->bg_out.p, by, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

// the blocks in one launch, then one workgroup per span
static int bgzf_faidx_fetch_dev(zngamd_ctx *c, const uint8_t *d_in, uint64_t in_len, const ZaMember *d_members, uint32_t n_members, const ZaFaiSpan *d_spans,
                                uint32_t n_spans, uint8_t *d_scratch, uint64_t scratch_cap, uint8_t *d_out, uint64_t out_cap, int32_t *d_status,
                                int32_t *d_span_status)
{
    if (n_members) bgzf_decode_launch(c, d_in, in_len, d_members, n_members, d_scratch, scratch_cap, d_status);
    if (n_spans) {
        ProfScope ps(c, ZNGAMD_K_GATHER);
        hipLaunchKernelGGL(za_k_fai_gather, dim3(n_spans), dim3(256), 0, c->stream, d_scratch, scratch_cap, d_members, d_status, n_members, d_spans, d_out,
                           out_cap, d_span_status);
        c->bgzf_stats[2] += n_spans;
    }
    HIPCHK(c, hipGetLastError());
    return ZNGAMD_OK;
}

int zngamd_bgzf_faidx_fetch_dev(zngamd_ctx *c, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                const zngamd_faidx_span *d_spans, uint32_t n_spans, void *d_scratch, uint64_t scratch_cap, void *d_out, uint64_t out_cap,
                                int32_t *d_status, int32_t *d_span_status)
try {
    if (!c || (n_members && (!d_in || !d_members || !d_status)) || (!d_scratch && scratch_cap) ||
        (n_spans && (!d_spans || !d_span_status || (!d_out && out_cap))) || n_spans >= (1u << 31)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    HIPCHK(c, hipSetDevice(c->device));
    int r = bgzf_faidx_fetch_dev(c, (const uint8_t *)d_in, in_len, (const ZaMember *)d_members, n_members, (const ZaFaiSpan *)d_spans, n_spans,
                                 (uint8_t *)d_scratch, scratch_cap, (uint8_t *)d_out, out_cap, d_status, d_span_status);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_faidx_fetch(zngamd_ctx *c, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                            const zngamd_faidx_span *spans, uint32_t n_spans, uint8_t *out, uint64_t out_cap, int32_t *status, int32_t *span_status)
try {
    if (!c || (!in && in_len) || (n_members && (!members || !status)) || (n_spans && (!spans || !span_status)) || (!out && out_cap) ||
        n_spans >= (1u << 31)) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    uint64_t scratch = 0;
    int r = bgzf_host_stage(c, in, in_len, members, n_members, &scratch);
    if (r) return r;
    HIPCHK(c, c->bg_out.ensure(out_cap + 64)); HIPCHK(c, c->fa_spans.ensure(n_spans + 1u)); HIPCHK(c, c->bg_sstat.ensure(n_spans + 1u));
    if (n_spans) HIPCHK(c, hipMemcpyAsync(c->fa_spans.p, spans, (size_t)n_spans * sizeof(ZaFaiSpan), hipMemcpyHostToDevice, c->stream));
    r = bgzf_faidx_fetch_dev(c, c->st_in.p, in_len, c->members.p, n_members, c->fa_spans.p, n_spans, c->st_out.p, scratch, c->bg_out.p, out_cap,
                             c->mstatus.p, c->bg_sstat.p);
    if (r) return r;
    if (n_members) HIPCHK(c, hipMemcpyAsync(status, c->mstatus.p, (size_t)n_members * 4, hipMemcpyDeviceToHost, c->stream));
    if (n_spans) HIPCHK(c, hipMemcpyAsync(span_status, c->bg_sstat.p, (size_t)n_spans * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the uploads read the caller's pageable tables: drained before it may touch them again)
    uint64_t used = 0;                                    // only the packed bases cross the link: as far as the spans reach
    for (uint32_t i = 0; i < n_spans; i++)
        if (span_status[i] != ZA_SLICE_TABLE) used = std::max<uint64_t>(used, spans[i].dst_off + spans[i].n);
    if (used) { const int rc_ = d2h_payload(c, out, c->bg_out.p, std::min(used, out_cap)); if (rc_) return rc_; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    prof_collect(c);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_bgzf_stats(zngamd_ctx *c, uint64_t *out, int reset)
try {
    if (!c || !out) return ZNGAMD_E_ARG;
    std::lock_guard<std::mutex> g(c->mu);
    for (int i = 0; i < 3; i++) { out[i] = c->bgzf_stats[i]; if (reset) c->bgzf_stats[i] = 0; }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// multi-GPU exchange over RCCL (one process per GPU).  librccl is loaded with dlopen on first use.
// ---------------------------------------------------------------------------------------------
#include <dlfcn.h>
#include <rccl/rccl.h>

struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi *rccl_api(std::string *why)
{
    static RcclApi api;
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (api.lib) return &api;
    void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { if (why) *why = std::string("librccl not found: ") + dlerror(); return nullptr; }
#define ZA_SYM(field, name) do { api.field = (decltype(api.field))dlsym(h, name); if (!api.field) { if (why) *why = std::string("librccl lacks ") + name; return nullptr; } } while (0)
    ZA_SYM(GetUniqueId, "ncclGetUniqueId"); ZA_SYM(CommInitRank, "ncclCommInitRank"); ZA_SYM(CommDestroy, "ncclCommDestroy");
    ZA_SYM(CommCount, "ncclCommCount");
    ZA_SYM(AllGather, "ncclAllGather"); ZA_SYM(AllReduce, "ncclAllReduce"); ZA_SYM(Send, "ncclSend"); ZA_SYM(Recv, "ncclRecv");
    ZA_SYM(GroupStart, "ncclGroupStart"); ZA_SYM(GroupEnd, "ncclGroupEnd"); ZA_SYM(GetErrorString, "ncclGetErrorString");
#undef ZA_SYM
    api.lib = h;
    return &api;
}

struct zngamd_comm {
    zngamd_ctx *ctx = nullptr; RcclApi *api = nullptr; ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    hipStream_t stream = nullptr; hipEvent_t ev = nullptr;
    uint64_t *d_rec = nullptr;           // [3 * world] gathered layout records, [3] own record behind them
    double *d_val = nullptr;
    std::string err;
};
#define NCCLCHK(cm, call) do { ncclResult_t r_ = (call); if (r_ != ncclSuccess) { \
    (cm)->err = std::string(#call) + ": " + (cm)->api->GetErrorString(r_); return ZNGAMD_E_HIP; } } while (0)
#define HIPCHKM(cm, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    (cm)->err = std::string(#call) + ": " + hipGetErrorString(e_); return ZNGAMD_E_HIP; } } while (0)

extern "C" {

int zngamd_comm_unique_id(uint8_t id[ZNGAMD_COMM_ID_BYTES])
try {
    static_assert(sizeof(ncclUniqueId) == ZNGAMD_COMM_ID_BYTES, "unique id size");
    if (!id) return ZNGAMD_E_ARG;
    RcclApi *a = rccl_api(nullptr);
    if (!a) return ZNGAMD_E_HIP;
    ncclUniqueId u;
    if (a->GetUniqueId(&u) != ncclSuccess) return ZNGAMD_E_HIP;
    memcpy(id, &u, sizeof u);
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_comm_create(zngamd_ctx *c, const uint8_t id[ZNGAMD_COMM_ID_BYTES], int rank, int world, zngamd_comm **out)
try {
    if (!c || !id || !out || world < 1 || rank < 0 || rank >= world) return ZNGAMD_E_ARG;
    *out = nullptr;
    std::string why;
    RcclApi *a = rccl_api(&why);
    if (!a) { c->err = why; return ZNGAMD_E_HIP; }
    zngamd_comm *m = new zngamd_comm();
    m->ctx = c; m->api = a; m->rank = rank; m->world = world;
    ncclUniqueId u;
    memcpy(&u, id, sizeof u);
    if (hipSetDevice(c->device) != hipSuccess || hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess ||
        hipMalloc((void **)&m->d_rec, (size_t)(3 * world + 3) * 8) != hipSuccess || hipMalloc((void **)&m->d_val, 16) != hipSuccess) {
        c->err = "comm: HIP resources"; zngamd_comm_destroy(m); return ZNGAMD_E_HIP;
    }
    const ncclResult_t r = a->CommInitRank(&m->comm, world, u, rank);
    if (r != ncclSuccess) { c->err = std::string("ncclCommInitRank: ") + a->GetErrorString(r); m->comm = nullptr; zngamd_comm_destroy(m); return ZNGAMD_E_HIP; }
    *out = m;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

void zngamd_comm_destroy(zngamd_comm *m)
{
    if (!m) return;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    if (m->comm) (void)m->api->CommDestroy(m->comm);
    if (m->d_rec) (void)hipFree(m->d_rec);
    if (m->d_val) (void)hipFree(m->d_val);
    if (m->ev) (void)hipEventDestroy(m->ev);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

const char *zngamd_comm_last_error(zngamd_comm *m) { return m ? m->err.c_str() : "no communicator"; }

// the number of ranks RCCL itself reports for the communicator (ncclCommCount), not what the launcher's environment says
int zngamd_comm_count(zngamd_comm *m, int *ranks)
try {
    if (!m || !ranks) return ZNGAMD_E_ARG;
    *ranks = 0;
    NCCLCHK(m, m->api->CommCount(m->comm, ranks));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_comm_layout(zngamd_comm *m, uint64_t local_len, uint32_t local_crc, uint64_t local_ulen, uint64_t *sizes,
                       uint64_t *my_off, uint64_t *total, uint32_t *whole_crc, uint64_t *whole_ulen)
try {
    if (!m || !sizes || !my_off || !total) return ZNGAMD_E_ARG;
    HIPCHKM(m, hipSetDevice(m->ctx->device));
    const uint64_t mine[3] = {local_len, (uint64_t)local_crc, local_ulen};
    uint64_t *d_mine = m->d_rec + 3 * (size_t)m->world;
    HIPCHKM(m, hipMemcpyAsync(d_mine, mine, sizeof mine, hipMemcpyHostToDevice, m->stream));
    NCCLCHK(m, m->api->AllGather(d_mine, m->d_rec, 3, ncclUint64, m->comm, m->stream));
    std::vector<uint64_t> rec(3 * (size_t)m->world);
    HIPCHKM(m, hipMemcpyAsync(rec.data(), m->d_rec, rec.size() * 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHKM(m, hipStreamSynchronize(m->stream));
    uint64_t off = 0, tot = 0, ul = 0;
    uint32_t crc = 0;
    for (int r = 0; r < m->world; r++) {
        sizes[r] = rec[3 * r];
        if (r < m->rank) off += rec[3 * r];
        tot += rec[3 * r];
        crc = r ? zngamd_crc32_combine(crc, (uint32_t)rec[3 * r + 1], rec[3 * r + 2]) : (uint32_t)rec[1];
        ul += rec[3 * r + 2];
    }
    *my_off = off; *total = tot;
    if (whole_crc) *whole_crc = crc;
    if (whole_ulen) *whole_ulen = ul;
    return ZNGAMD_OK;
} ZA_ABI_GUARD

uint64_t zngamd_comm_offsets(const uint64_t *sizes, int world, uint64_t *offs)
{
    uint64_t run = 0;
    for (int r = 0; r < world; r++) { if (offs) offs[r] = run; run += sizes ? sizes[r] : 0; }
    return run;
}

int zngamd_comm_allgather_stream(zngamd_comm *m, const void *d_local, const uint64_t *sizes, void *d_stream, uint64_t stream_cap)
try {
    if (!m || !d_local || !sizes || !d_stream) return ZNGAMD_E_ARG;
    HIPCHKM(m, hipSetDevice(m->ctx->device));
    std::vector<uint64_t> offs((size_t)m->world);
    const uint64_t total = zngamd_comm_offsets(sizes, m->world, offs.data()), my_off = offs[(size_t)m->rank];
    if (total > stream_cap) { m->err = "stream buffer too small"; return ZNGAMD_BUF_ERROR; }
    // the slices are final once the work queued on the context's stream so far is done
    HIPCHKM(m, hipEventRecord(m->ev, m->ctx->stream));
    HIPCHKM(m, hipStreamWaitEvent(m->stream, m->ev, 0));
    uint8_t *dst = (uint8_t *)d_stream;
    if (sizes[m->rank] && dst + my_off != (const uint8_t *)d_local)
        HIPCHKM(m, hipMemcpyAsync(dst + my_off, d_local, sizes[m->rank], hipMemcpyDeviceToDevice, m->stream));
    if (m->world > 1) {
        NCCLCHK(m, m->api->GroupStart());
        // (a call that fails inside the group must not leave the group open: it is closed first, then the first error is reported)
        ncclResult_t bad = ncclSuccess;
        const char *what = "";
        for (int r = 0; r < m->world && bad == ncclSuccess; r++) {
            if (r != m->rank) {
                if (sizes[m->rank]) { bad = m->api->Send(d_local, sizes[m->rank], ncclUint8, r, m->comm, m->stream); what = "ncclSend"; }
                if (bad == ncclSuccess && sizes[r]) { bad = m->api->Recv(dst + offs[(size_t)r], sizes[r], ncclUint8, r, m->comm, m->stream); what = "ncclRecv"; }
            }
        }
        const ncclResult_t ended = m->api->GroupEnd();
        if (bad != ncclSuccess) { m->err = std::string(what) + ": " + m->api->GetErrorString(bad); return ZNGAMD_E_HIP; }
        NCCLCHK(m, ended);
    }
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_comm_wait(zngamd_comm *m)
try {
    if (!m) return ZNGAMD_E_ARG;
    HIPCHKM(m, hipStreamSynchronize(m->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_comm_max_f64(zngamd_comm *m, double *value)
try {
    if (!m || !value) return ZNGAMD_E_ARG;
    HIPCHKM(m, hipSetDevice(m->ctx->device));
    HIPCHKM(m, hipMemcpyAsync(m->d_val, value, 8, hipMemcpyHostToDevice, m->stream));
    NCCLCHK(m, m->api->AllReduce(m->d_val, m->d_val + 1, 1, ncclFloat64, ncclMax, m->comm, m->stream));
    HIPCHKM(m, hipMemcpyAsync(value, m->d_val + 1, 8, hipMemcpyDeviceToHost, m->stream));
    HIPCHKM(m, hipStreamSynchronize(m->stream));
    return ZNGAMD_OK;
} ZA_ABI_GUARD

int zngamd_comm_barrier(zngamd_comm *m)
try {
    double v = 0;
    return zngamd_comm_max_f64(m, &v);
} ZA_ABI_GUARD

}  // extern "C"

#include "zng_stream.hip"

#ifdef ZA_PLAN_STATS
// profiling build only: the plan kernel's phase clocks (za_deflate.hip), read and cleared
extern "C" int zngamd_debug_plan_stats(unsigned long long *out16)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(za_plan_stat), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[16] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(za_plan_stat), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
#ifdef ZA_CH_STATS
// profiling build only: the chain kernel's clocks (za_deflate.hip), read and cleared
extern "C" int zngamd_debug_ch_stats(unsigned long long *out32)
{
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(za_ch_stat), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[32] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(za_ch_stat), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif
#ifdef ZA_PS_STATS
// profiling build only (profiles/ps_stats.sh): counters of the parallel sweep, read and cleared
extern "C" int zngamd_debug_ps_stats(unsigned long long *out24)
{
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(za_ps_stat), 32 * sizeof(unsigned long long)) != hipSuccess) return -1;
    unsigned long long z[32] = {0};
    return hipMemcpyToSymbol(HIP_SYMBOL(za_ps_stat), z, sizeof z) == hipSuccess ? 0 : -1;
}
#endif

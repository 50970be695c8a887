// BGZF: records split by labels the caller gives.  The call of za_classify.hip without the compare: the lines
// pass of za_grep.hip has run for the delimiters alone, the host has read how many lines the text holds, and za_k_grep_rec_lines of
// za_grep_records.hip has written where every line starts.  What is new:
//   za_k_part_eval     one thread per record: its label judged, its length, its first byte
//   za_k_part_hist     one workgroup per 256 records: records and bytes per class, and the dropped ones
//   (za_k_tbx_reduce / _scan_blocks / _apply)    the table of counts, class by class, summed: where every (class, workgroup) begins
//   za_k_part_close    one thread: the totals
//   za_k_part_scatter  one workgroup per 256 records: every kept record's row behind the rows of its class in front of it
// The histogram and the scatter are za_part_hist / za_part_scatter of za_classify.hip for up to ZA_PART_MAX_CLASSES classes and 16-bit
// labels, with the label ZA_PART_DROP, whose records get no row.  A record without a label (r >= nlab) is a dropped one.
// za_k_offsets, za_k_grep_place and za_k_slice_gather pack the rows as they pack lines.  The result depends on the text and the labels
// alone: a minimum and a sum of integers do not depend on the order in which they are taken.
// Included by zng_amd.hip behind za_classify.hip.
#include "za_common.h"

#define ZA_PART_MAX_CLASSES 1024u                      // mirrors ZNGAMD_BGZF_PARTITION_MAX_CLASSES
#define ZA_PART_DROP        0xFFFFu                    // mirrors ZNGAMD_BGZF_PARTITION_DROP: all ones, the DROP of za_part_hist
#define ZA_PART_WG_RECORDS  ZA_CLS_WG_RECORDS          // records per workgroup of za_k_part_hist / za_k_part_scatter: one per thread
static_assert(ZA_PART_DROP == (uint16_t)~0u, "the label za_part_hist counts as dropped");

struct ZaPartTotals {                                  // mirrors zngamd_bgzf_partition_totals
    uint64_t seen, bytes, dropped, dropped_bytes, tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, labels_short;
};

// grid: one thread per record.  labels[] is read below nlab (<= nrec) only.  len[r]: the record's bytes.  bad[0]: the smallest r whose
// first byte is not first_byte (start, lines: as za_rec_extent takes them), bad[1]: the smallest r whose label is neither below ncls
// nor ZA_PART_DROP (both ~0 beforehand).
__global__ __launch_bounds__(256) void za_k_part_eval(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end,
                                                      const unsigned long long *__restrict__ start, uint64_t lines, const uint16_t *__restrict__ labels,
                                                      uint64_t nlab, uint64_t nrec, uint32_t k_lines, uint32_t ncls, int32_t first_byte,
                                                      uint32_t *__restrict__ len, unsigned long long *__restrict__ bad)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    len[r] = (uint32_t)za_rec_extent(scratch, text_off, text_end, start, lines, r, k_lines, first_byte, &bad[0]);
    if (r < nlab) {
        const uint32_t c = labels[r];
        if (c >= ncls && c != ZA_PART_DROP) atomicMin(&bad[1], (unsigned long long)r);
    }
}

// grid: one workgroup per ZA_PART_WG_RECORDS records.  za_part_hist with the caller's labels; the sums go to cnt[c] / cnt[ncls + c]
// and tot->dropped / dropped_bytes (all zeroed).
__global__ __launch_bounds__(ZA_PART_WG_RECORDS) void za_k_part_hist(const uint16_t *__restrict__ labels, uint64_t nlab, const uint32_t *__restrict__ len, uint64_t nrec,
                                                                     uint32_t ncls, uint32_t nwg, unsigned long long *__restrict__ tab,
                                                                     unsigned long long *__restrict__ cnt, ZaPartTotals *__restrict__ tot)
{
    za_part_hist<ZA_PART_MAX_CLASSES, uint16_t>(labels, nlab, len, nrec, ncls, nwg, tab, cnt, cnt + ncls, (unsigned long long *)&tot->dropped);
}

// one thread.  nrec > 0.  cnt[] holds the sums of za_k_part_hist, tot->dropped / dropped_bytes too.  A record with both faults is
// reported for its first byte; otherwise the fault at the smaller record is.
__global__ void za_k_part_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint64_t nlab, uint32_t k_lines, uint32_t flags,
                                uint64_t text_end, uint64_t record_base, uint32_t ncls, const unsigned long long *__restrict__ cnt,
                                const unsigned long long *__restrict__ bad, ZaPartTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    uint64_t bytes = 0;
    for (uint32_t c = 0; c < ncls; c++) bytes += cnt[ncls + c];
    tot->covered = 1; tot->seen = nrec; tot->bytes = bytes; tot->labels_short = nlab < nrec ? 1u : 0u;
    const unsigned long long fb = bad[0], lb = bad[1];
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, fb <= lb ? fb : lb, fb <= lb ? 1u : 2u, tot);
}

// grid: one workgroup per ZA_PART_WG_RECORDS records.  za_part_scatter with the caller's labels; `reserved` carries the label.  Every
// label is below ncls or ZA_PART_DROP (za_k_part_close reported none).
__global__ __launch_bounds__(ZA_PART_WG_RECORDS) void za_k_part_scatter(const uint16_t *__restrict__ labels, uint64_t nlab, const uint32_t *__restrict__ len,
                                                                        const unsigned long long *__restrict__ start, uint64_t nrec, uint32_t k_lines,
                                                                        uint32_t ncls, uint32_t nwg, const unsigned long long *__restrict__ tab,
                                                                        uint64_t record_base, ZaGrepRow *__restrict__ rows, uint64_t rows_cap,
                                                                        uint32_t *__restrict__ lens)
{
    za_part_scatter<ZA_PART_MAX_CLASSES, uint16_t>(labels, nlab, (const uint32_t *)nullptr, len, start, nrec, k_lines, ncls, nwg, tab, record_base, rows, rows_cap, lens);
}

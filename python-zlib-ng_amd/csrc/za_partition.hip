// BGZF: records split by labels the caller gives.  The call of za_classify.hip without the compare: the lines
// pass of za_grep.hip has run for the delimiters alone, the host has read how many lines the text holds, and za_k_grep_rec_lines of
// za_grep_records.hip has written where every line starts.  What is new:
//   za_k_part_eval     one thread per record: its label judged, its length, its first byte
//   za_k_part_hist     one workgroup per 256 records: records and bytes per class, and the dropped ones
//   (za_k_tbx_reduce / _scan_blocks / _apply)    the table of counts, class by class, summed: where every (class, workgroup) begins
//   za_k_part_close    one thread: the totals
//   za_k_part_scatter  one workgroup per 256 records: every kept record's row behind the rows of its class in front of it
// These are za_k_cls_hist / _close / _scatter for up to ZA_PART_MAX_CLASSES classes (what was `tid < ncls` is a strided loop) and with
// the label ZA_PART_DROP, whose records get no row.  A record without a label (r >= nlab) is a dropped one.  za_k_offsets,
// za_k_grep_place and za_k_slice_gather pack the rows as they pack lines.  The result depends on the text and the labels alone: a
// minimum and a sum of integers do not depend on the order in which they are taken.
// Included by zng_amd.hip behind za_classify.hip.
#include "za_common.h"

#define ZA_PART_MAX_CLASSES 1024u                      // mirrors ZNGAMD_BGZF_PARTITION_MAX_CLASSES
#define ZA_PART_DROP        0xFFFFu                    // mirrors ZNGAMD_BGZF_PARTITION_DROP
#define ZA_PART_WG_RECORDS  256u                       // records per workgroup of za_k_part_hist / za_k_part_scatter: one per thread

struct ZaPartTotals {                                  // mirrors zngamd_bgzf_partition_totals
    uint64_t seen, bytes, dropped, dropped_bytes, tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, labels_short;
};

// grid: one thread per record.  lines: entries 0 .. lines of start[] are written.  labels[] is read below nlab (<= nrec) only.
// len[r]: the record's bytes.  bad[0]: the smallest r whose first byte is not first_byte, bad[1]: the smallest r whose label is
// neither below ncls nor ZA_PART_DROP (both ~0 beforehand).
__global__ __launch_bounds__(256) void za_k_part_eval(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end,
                                                      const unsigned long long *__restrict__ start, uint64_t lines, const uint16_t *__restrict__ labels,
                                                      uint64_t nlab, uint64_t nrec, uint32_t k_lines, uint32_t ncls, int32_t first_byte,
                                                      uint32_t *__restrict__ len, unsigned long long *__restrict__ bad)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    const uint64_t l0 = (uint64_t)k_lines * r, l1 = lines - l0 < k_lines ? lines : l0 + k_lines;
    const uint64_t a = start[l0], e = start[l1];
    len[r] = e > a ? (uint32_t)(e - a) : 0u;
    if (first_byte >= 0 && !(a >= text_off && a < text_end && scratch[a] == (uint32_t)first_byte)) atomicMin(&bad[0], (unsigned long long)r);
    if (r < nlab) {
        const uint32_t c = labels[r];
        if (c >= ncls && c != ZA_PART_DROP) atomicMin(&bad[1], (unsigned long long)r);
    }
}

// grid: one workgroup per ZA_PART_WG_RECORDS records.  tab[c * nwg + workgroup] = its records of class c (class by class, so that ONE
// sum over the table gives every (class, workgroup) its first row); cnt[c] / cnt[ncls + c] (zeroed) += its records / bytes of class
// c; tot->dropped / dropped_bytes (zeroed) += its records without a class.  A label that is out of range counts nowhere.
__global__ __launch_bounds__(ZA_PART_WG_RECORDS) void za_k_part_hist(const uint16_t *__restrict__ labels, uint64_t nlab, const uint32_t *__restrict__ len, uint64_t nrec,
                                                                     uint32_t ncls, uint32_t nwg, unsigned long long *__restrict__ tab,
                                                                     unsigned long long *__restrict__ cnt, ZaPartTotals *__restrict__ tot)
{
    __shared__ uint32_t s_n[ZA_PART_MAX_CLASSES], s_b[ZA_PART_MAX_CLASSES];
    __shared__ uint32_t s_drop[2];
    const uint32_t tid = threadIdx.x;
    for (uint32_t c = tid; c < ncls; c += ZA_PART_WG_RECORDS) { s_n[c] = 0; s_b[c] = 0; }
    if (tid < 2u) s_drop[tid] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * ZA_PART_WG_RECORDS + tid;
    if (r < nrec) {
        const uint32_t c = r < nlab ? labels[r] : ZA_PART_DROP;
        if (c < ncls) { atomicAdd(&s_n[c], 1u); atomicAdd(&s_b[c], len[r]); }      // (the text has fewer than 4 GiB: so has a workgroup's share)
        else if (c == ZA_PART_DROP) { atomicAdd(&s_drop[0], 1u); atomicAdd(&s_drop[1], len[r]); }
    }
    __syncthreads();
    for (uint32_t c = tid; c < ncls; c += ZA_PART_WG_RECORDS) {
        tab[(size_t)c * nwg + blockIdx.x] = s_n[c];
        if (s_n[c]) { atomicAdd(&cnt[c], (unsigned long long)s_n[c]); atomicAdd(&cnt[ncls + c], (unsigned long long)s_b[c]); }
    }
    if (tid == 0 && s_drop[0]) {
        atomicAdd((unsigned long long *)&tot->dropped, (unsigned long long)s_drop[0]);
        atomicAdd((unsigned long long *)&tot->dropped_bytes, (unsigned long long)s_drop[1]);
    }
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
    const uint64_t whole = (uint64_t)k_lines * (lines / k_lines);      // lines in complete records
    tot->tail_off = (flags & ZA_GREP_FINAL) ? text_end : start[whole];
    tot->short_lines = (flags & ZA_GREP_FINAL) ? (uint32_t)(lines - whole) : 0u;
    const unsigned long long fb = bad[0], lb = bad[1];
    tot->bad = 0; tot->bad_record = 0; tot->bad_src = 0;
    const unsigned long long b = fb <= lb ? fb : lb;
    if (b < nrec) { tot->bad = fb <= lb ? 1u : 2u; tot->bad_record = record_base + b; tot->bad_src = start[(uint64_t)k_lines * b]; }
}

// grid: one workgroup per ZA_PART_WG_RECORDS records.  tab: the table of za_k_part_hist, summed inclusively in the order it lies.  A
// kept record's row goes to (the rows in front of its class and workgroup) + (the records of its class in front of it in the
// workgroup): the second is a ballot per class and a count of the bits below the lane, so the order inside a class is the input's.
// rows[] and lens[] have room for rows_cap entries.  Every label is below ncls or ZA_PART_DROP (za_k_part_close reported none).
__global__ __launch_bounds__(ZA_PART_WG_RECORDS) void za_k_part_scatter(const uint16_t *__restrict__ labels, uint64_t nlab, const uint32_t *__restrict__ len,
                                                                        const unsigned long long *__restrict__ start, uint64_t nrec, uint32_t k_lines,
                                                                        uint32_t ncls, uint32_t nwg, const unsigned long long *__restrict__ tab,
                                                                        uint64_t record_base, ZaGrepRow *__restrict__ rows, uint64_t rows_cap,
                                                                        uint32_t *__restrict__ lens)
{
    __shared__ uint32_t s_n[4][ZA_PART_MAX_CLASSES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t c = tid; c < ncls; c += ZA_PART_WG_RECORDS) { s_n[0][c] = 0; s_n[1][c] = 0; s_n[2][c] = 0; s_n[3][c] = 0; }
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * ZA_PART_WG_RECORDS + tid;
    const uint32_t c = r < nrec && r < nlab ? labels[r] : ZA_PART_DROP;
    const bool mine = c < ncls;
    uint32_t rank = 0;
    uint64_t left = __ballot(mine);
    while (left) {                                      // (the same for every lane of the wave: one round per class the wave holds)
        const uint32_t cc = (uint32_t)__shfl((int)c, __builtin_ctzll(left), 64);
        const uint64_t m = __ballot(mine && c == cc);
        if (mine && c == cc) {
            rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (rank == 0) s_n[wave][cc] = (uint32_t)__popcll(m);
        }
        left &= ~m;
    }
    __syncthreads();
    if (!mine) return;
    for (uint32_t x = 0; x < wave; x++) rank += s_n[x][c];
    const size_t at = (size_t)c * nwg + blockIdx.x;
    const uint64_t idx = (at ? tab[at - 1u] : 0ull) + rank;
    if (idx >= rows_cap) return;
    ZaGrepRow w; w.src_off = start[(uint64_t)k_lines * r]; w.number = record_base + r; w.len = len[r]; w.reserved = c;
    rows[idx] = w; lens[idx] = w.len;
}

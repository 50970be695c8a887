// BGZF: records by their nearest pattern.  The lines pass of za_grep.hip has run over the text, so every tile
// has its carry, the host has read how many lines the text holds, and za_k_grep_rec_lines of za_grep_records.hip has written where
// every line starts.  What is new:
//   za_k_grep_classify  one workgroup per tile: every (position, pattern) distance of za_k_grep_mark_approx, kept per RECORD as the
//                       two minima lo[r] = min(dist << 8 | i) and hi[r] = min(dist << 8 | 255 - i)
//   za_k_cls_eval       one thread per record: the class row, the class, the length, the first byte
//   za_k_cls_hist       one workgroup per 256 records: records and bytes per class
//   (za_k_tbx_reduce / _scan_blocks / _apply)    the table of counts, class by class, summed: where every (class, workgroup) begins
//   za_k_cls_close      one thread: the totals
//   za_k_cls_scatter    one workgroup per 256 records: every record's row behind the rows of its class in front of it
// The histogram and the scatter are za_part_hist / za_part_scatter<MAX_CLASSES, Label> below: the one stable partition, which
// za_k_part_hist / za_k_part_scatter of za_partition.hip instantiate for 1024 classes and 16-bit labels.
// za_k_offsets, za_k_grep_place and za_k_slice_gather pack the records as they pack lines.  The result depends on the text and the
// pattern list alone: a minimum and a sum of integers do not depend on the order in which they are taken.
// Included by zng_amd.hip behind za_grep_records.hip.
#include "za_common.h"

#define ZA_CLS_MAX_CLASSES (ZA_GREP_MAX_PAT + 2u)      // mirrors ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES
#define ZA_CLS_WG_RECORDS  256u                        // records per workgroup of za_k_cls_hist / za_k_cls_scatter: one per thread
#define ZA_CLS_ASSIGNED    1u                          // mirror ZNGAMD_BGZF_CLASS_*
#define ZA_CLS_AMBIGUOUS   2u
#define ZA_CLS_GROUP       16u                         // mirrors ZNGAMD_BGZF_CLASSIFY_GROUP

struct ZaClsTotals {                                   // mirrors zngamd_bgzf_classify_totals
    uint64_t seen, bytes, tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, n_classes;
    uint64_t class_records[ZA_CLS_MAX_CLASSES], class_bytes[ZA_CLS_MAX_CLASSES];
};

// grid: one workgroup per tile, tile0 + blockIdx.x; the parameters up to k as za_k_grep_mark_approx takes them.  carry: what the scan
// left (lines: the delimiters of the text in front of the tile).  A window within k that holds no stop bit starts in line
// q = carry.lines + the tile's delimiters in front of it; it counts for record q / k_lines unless match_line names another line of
// the record or the record is none of the nrec this call decides.  lo[] and hi[] have room for nrec words and were set to all ones.
__global__ __launch_bounds__(256) void za_k_grep_classify(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t text_off, uint64_t text_end,
                                                          uint64_t tile0, const ZaGrepPat *__restrict__ ptab, const uint32_t *__restrict__ words,
                                                          uint32_t np, uint32_t delim, uint32_t flags, uint32_t k, const ZaGrepCarry *__restrict__ carry,
                                                          uint32_t k_lines, int32_t match_line, uint64_t nrec, uint32_t *__restrict__ lo, uint32_t *__restrict__ hi)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_t[ZA_GREP_AP_WORDS];
    __shared__ uint32_t s_d[512], s_dpre[512];
    __shared__ uint32_t s_stop[ZA_GREP_AP_BITS], s_before[ZA_GREP_AP_BITS];
    __shared__ uint32_t s_wsum[4], s_dsum[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = (tile0 + blockIdx.x) * (uint64_t)ZA_GREP_TILE;
    s_d[tid] = 0; s_d[tid + 256u] = 0;
    for (uint32_t i = tid; i < ZA_GREP_AP_BITS; i += 256u) s_stop[i] = 0;
    __syncthreads();
    za_grep_approx_stage(scratch, scratch_cap, text_off, text_end, base, delim, s_t, s_d, s_stop, s_before, s_wsum);
    {   // s_dpre[w]: the tile's delimiters in front of bitmap word w (thread tid owns the words 2 tid and 2 tid + 1: its 64 bytes)
        const uint32_t n0 = (uint32_t)__popc(s_d[2u * tid]), n1 = (uint32_t)__popc(s_d[2u * tid + 1u]);
        const uint32_t incl = za_wave_incl_scan(n0 + n1);
        if (lane == 63u) s_dsum[wave] = incl;
        __syncthreads();
        uint32_t ex = incl - n0 - n1;
        for (uint32_t x = 0; x < wave; x++) ex += s_dsum[x];
        s_dpre[2u * tid] = ex; s_dpre[2u * tid + 1u] = ex + n0;
    }
    __syncthreads();
    const uint64_t lines0 = carry[blockIdx.x].lines;
    za_grep_approx_compare<true>(scratch, text_off, text_end, base, ptab, words, np, delim, flags, k, s_t, s_d, s_stop, s_before,
                                 [&](uint32_t b, uint32_t i, uint32_t dist) {      // (b < ZA_GREP_TILE: a window starts in the tile)
                                     const uint64_t q = lines0 + s_dpre[b >> 5] + (uint32_t)__popc(s_d[b >> 5] & ((1u << (b & 31u)) - 1u));
                                     const uint64_t r = q / k_lines;
                                     if ((match_line >= 0 && (uint32_t)(q % k_lines) != (uint32_t)match_line) || r >= nrec) return;
                                     atomicMin(&lo[r], dist << 8 | i);
                                     atomicMin(&hi[r], dist << 8 | (255u - i));
                                 },
                                 [](uint32_t, uint32_t) {});
}

// grid: one thread per record.  row[r]: the class row {pattern, other, distance, flags} as one word; cls[r]: the class; len[r]: the
// record's bytes.  start, lines, first_byte, bad: as za_rec_extent takes them.
__global__ __launch_bounds__(256) void za_k_cls_eval(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end,
                                                     const unsigned long long *__restrict__ start, uint64_t lines, const uint32_t *__restrict__ lo,
                                                     const uint32_t *__restrict__ hi, uint64_t nrec, uint32_t k_lines, uint32_t np, int32_t first_byte,
                                                     uint32_t *__restrict__ row, uint8_t *__restrict__ cls, uint32_t *__restrict__ len,
                                                     unsigned long long *__restrict__ bad)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    const uint32_t vl = lo[r], vh = hi[r];
    uint32_t w = 0x00FFFFFFu, c = np + 1u;                            // unassigned: pattern = other = distance = 255, flags = 0
    if (vl != 0xFFFFFFFFu) {
        const uint32_t first = vl & 0xFFu, last = 255u - (vh & 0xFFu), dist = vl >> 8 & 0xFFu;
        const bool one = first == last;
        w = first | last << 8 | dist << 16 | (one ? ZA_CLS_ASSIGNED : ZA_CLS_AMBIGUOUS) << 24;
        c = one ? first : np;
    }
    row[r] = w; cls[r] = (uint8_t)c;
    len[r] = (uint32_t)za_rec_extent(scratch, text_off, text_end, start, lines, r, k_lines, first_byte, bad);
}

// The stable partition's histogram, for a workgroup of ZA_CLS_WG_RECORDS records, one per thread, and ncls <= MAX_CLASSES classes.
// lab[r] is read below nlab; a record at or beyond nlab has the label DROP, all ones.  tab[c * nwg + workgroup] = its records of class c
// (class by class, so that ONE sum over the table gives every (class, workgroup) its first row); crec[c] / cbytes[c] (zeroed) += its
// records / bytes of class c; dropped[0] / dropped[1] (zeroed; or no pointer) += its records / bytes with DROP.  Any other label that
// is no class counts nowhere.
template <uint32_t MAX_CLASSES, typename Label>
__device__ __forceinline__ void za_part_hist(const Label *__restrict__ lab, uint64_t nlab, const uint32_t *__restrict__ len, uint64_t nrec, uint32_t ncls, uint32_t nwg,
                                             unsigned long long *__restrict__ tab, unsigned long long *__restrict__ crec, unsigned long long *__restrict__ cbytes,
                                             unsigned long long *__restrict__ dropped)
{
    constexpr uint32_t DROP = (Label)~(Label)0;
    __shared__ uint32_t s_n[MAX_CLASSES], s_b[MAX_CLASSES];
    __shared__ uint32_t s_drop[2];
    const uint32_t tid = threadIdx.x;
    for (uint32_t c = tid; c < ncls; c += ZA_CLS_WG_RECORDS) { s_n[c] = 0; s_b[c] = 0; }
    if (tid < 2u) s_drop[tid] = 0;
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * ZA_CLS_WG_RECORDS + tid;
    if (r < nrec) {
        const uint32_t c = r < nlab ? lab[r] : DROP;
        if (c < ncls) { atomicAdd(&s_n[c], 1u); atomicAdd(&s_b[c], len[r]); }      // (the text has fewer than 4 GiB: so has a workgroup's share)
        else if (dropped && c == DROP) { atomicAdd(&s_drop[0], 1u); atomicAdd(&s_drop[1], len[r]); }
    }
    __syncthreads();
    for (uint32_t c = tid; c < ncls; c += ZA_CLS_WG_RECORDS) {
        tab[(size_t)c * nwg + blockIdx.x] = s_n[c];
        if (s_n[c]) { atomicAdd(&crec[c], (unsigned long long)s_n[c]); atomicAdd(&cbytes[c], (unsigned long long)s_b[c]); }
    }
    if (dropped && tid == 0 && s_drop[0]) { atomicAdd(&dropped[0], (unsigned long long)s_drop[0]); atomicAdd(&dropped[1], (unsigned long long)s_drop[1]); }
}

// The stable partition's scatter, for the same workgroups and labels.  tab: the table of za_part_hist, summed inclusively in the order
// it lies.  A record of a class below ncls gets a row, at (the rows in front of its class and workgroup) + (the records of its class in
// front of it in the workgroup): the second is a ballot per class and a count of the bits below the lane, so the order inside a class
// is the input's; a wave that holds 64 different classes takes 64 rounds.  rows[] and lens[] have room for rows_cap entries.
// reserved: row[r], or without row[] the label.
template <uint32_t MAX_CLASSES, typename Label>
__device__ __forceinline__ void za_part_scatter(const Label *__restrict__ lab, uint64_t nlab, const uint32_t *__restrict__ row, const uint32_t *__restrict__ len,
                                                const unsigned long long *__restrict__ start, uint64_t nrec, uint32_t k_lines, uint32_t ncls, uint32_t nwg,
                                                const unsigned long long *__restrict__ tab, uint64_t record_base, ZaGrepRow *__restrict__ rows, uint64_t rows_cap,
                                                uint32_t *__restrict__ lens)
{
    __shared__ uint32_t s_n[4][MAX_CLASSES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t c = tid; c < ncls; c += ZA_CLS_WG_RECORDS) { s_n[0][c] = 0; s_n[1][c] = 0; s_n[2][c] = 0; s_n[3][c] = 0; }
    __syncthreads();
    const uint64_t r = (uint64_t)blockIdx.x * ZA_CLS_WG_RECORDS + tid;
    const uint32_t c = r < nrec && r < nlab ? lab[r] : 0xFFFFFFFFu;
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
    ZaGrepRow w; w.src_off = start[(uint64_t)k_lines * r]; w.number = record_base + r; w.len = len[r]; w.reserved = row ? row[r] : c;
    rows[idx] = w; lens[idx] = w.len;
}

// grid: one workgroup per ZA_CLS_WG_RECORDS records.  za_part_hist with every record's class; the sums go to tot->class_records / class_bytes (zeroed).
__global__ __launch_bounds__(ZA_CLS_WG_RECORDS) void za_k_cls_hist(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ len, uint64_t nrec, uint32_t ncls,
                                                                   uint32_t nwg, unsigned long long *__restrict__ tab, ZaClsTotals *__restrict__ tot)
{
    za_part_hist<ZA_CLS_MAX_CLASSES, uint8_t>(cls, nrec, len, nrec, ncls, nwg, tab, (unsigned long long *)tot->class_records, (unsigned long long *)tot->class_bytes, nullptr);
}

// one thread.  nrec > 0.  tot->class_records / class_bytes hold the sums of za_k_cls_hist.
__global__ void za_k_cls_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k_lines, uint32_t flags, uint64_t text_end,
                               uint64_t record_base, uint32_t ncls, const unsigned long long *__restrict__ bad, ZaClsTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    uint64_t bytes = 0;
    for (uint32_t c = 0; c < ncls; c++) bytes += tot->class_bytes[c];
    tot->covered = 1; tot->seen = nrec; tot->bytes = bytes; tot->n_classes = ncls;
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, *bad, 1u, tot);
}

// grid: one workgroup per ZA_CLS_WG_RECORDS records.  za_part_scatter with every record's class; the row carries the class row in `reserved`.
__global__ __launch_bounds__(ZA_CLS_WG_RECORDS) void za_k_cls_scatter(const uint8_t *__restrict__ cls, const uint32_t *__restrict__ row, const uint32_t *__restrict__ len,
                                                                      const unsigned long long *__restrict__ start, uint64_t nrec, uint32_t k_lines, uint32_t ncls,
                                                                      uint32_t nwg, const unsigned long long *__restrict__ tab, uint64_t record_base,
                                                                      ZaGrepRow *__restrict__ rows, uint64_t rows_cap, uint32_t *__restrict__ lens)
{
    za_part_scatter<ZA_CLS_MAX_CLASSES, uint8_t>(cls, nrec, row, len, start, nrec, k_lines, ncls, nwg, tab, record_base, rows, rows_cap, lens);
}

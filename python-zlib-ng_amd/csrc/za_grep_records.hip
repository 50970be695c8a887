// BGZF: records by content.  A record is k lines; za_k_grep_cover / _mark / _scan of za_grep.hip have run over
// the text WITHOUT INVERT, so every tile has its delimiter word, its verdict word and its carry, and the host has read how many lines
// the text holds.  What is new is the step from lines to records:
//   za_k_grep_rec_lines  one workgroup per tile: start[q + 1] = the byte behind the delimiter of line q; a line that matched and passes
//                        the match_line test stores 1 into hit[q / k]
//   za_k_grep_rec_eval   one thread per record: selected or not, its length, its first byte; the two arrays the scans sum
//                        (za_rec_extent: the length and the first byte, as za_k_cls_eval and za_k_part_eval take them too)
//   (za_k_tbx_reduce / _scan_blocks / _apply)    selected records and their bytes up to every record, inclusive
//   za_k_grep_rec_close  one thread: the totals (za_rec_close: the tail, the short last record and the fault, for the three close kernels)
//   za_k_grep_rec_emit   one thread per record: its row where the sum of the selected ones steps
// za_k_offsets, za_k_grep_place and za_k_slice_gather pack the records as they pack lines.  No thread walks a line or a record.
// Included by zng_amd.hip behind za_grep.hip.
#include "za_common.h"

#define ZA_GREP_REC_MAX 64u                // lines per record at most: mirrors ZNGAMD_BGZF_GREP_MAX_RECORD_LINES

struct ZaGrepRecTotals {                   // mirrors zngamd_bgzf_grep_records_totals
    uint64_t seen, selected, bytes, tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, reserved;
};

// grid: one workgroup per tile.  start[] has room for start_cap entries (the host has read the line count: lines + 1), hit[] for
// hit_cap records; hit[] was zeroed.  Every writer of hit[r] stores 1: no atomics.  lines: the lines the scan decided (gt->seen).
__global__ __launch_bounds__(256) void za_k_grep_rec_lines(const ulonglong2 *__restrict__ bits, const ZaGrepTile *__restrict__ tiles, const ZaGrepCarry *__restrict__ carry,
                                                           const ZaGrepTotals *__restrict__ gt, uint32_t ntiles, uint64_t tile0, uint64_t text_off, uint64_t text_end,
                                                           uint32_t flags, uint32_t k, int32_t match_line, unsigned long long *__restrict__ start,
                                                           uint64_t start_cap, uint8_t *__restrict__ hit, uint64_t hit_cap)
{
    __shared__ uint32_t s_nd[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const ZaGrepTile t = tiles[blockIdx.x];
    const ZaGrepCarry c = carry[blockIdx.x];
    const uint64_t base = (tile0 + blockIdx.x) * (uint64_t)ZA_GREP_TILE;
    if (tid == 0) {
        if (blockIdx.x == 0 && start_cap) start[0] = text_off;
        if (blockIdx.x == ntiles - 1u && (flags & ZA_GREP_FINAL)) {           // the bytes behind the last delimiter are a line
            const uint64_t open = t.ndelim ? base + t.last + 1ull : c.open_start, q = c.lines + t.ndelim;
            if (open < text_end) {
                if (q + 1ull < start_cap) start[q + 1ull] = text_end;
                if (gt->final_emit && (match_line < 0 || (uint32_t)(q % k) == (uint32_t)match_line) && q / k < hit_cap) hit[q / k] = 1;
            }
        }
    }
    if (!t.ndelim) return;                            // (the same for every thread)
    const ulonglong2 v = bits[(size_t)blockIdx.x * 256u + tid];
    const uint64_t D = v.x;
    uint64_t L = v.y;
    if (c.first_emit && (t.first >> 6) == tid) L |= 1ull << (t.first & 63u);      // the tile's first line: the scan decided it
    const uint32_t nd = (uint32_t)__popcll(D);
    const uint32_t id = za_wave_incl_scan(nd);
    if (lane == 63u) s_nd[wave] = id;
    __syncthreads();
    uint32_t rd = id - nd;
    for (uint32_t x = 0; x < wave; x++) rd += s_nd[x];
    uint64_t d = D;
    while (d) {
        const uint32_t b = (uint32_t)__builtin_ctzll(d);
        d &= d - 1ull;
        const uint64_t q = c.lines + rd;              // the ordinal of the line this delimiter ends
        if (q + 1ull < start_cap) start[q + 1ull] = base + tid * 64u + b + 1ull;
        if ((L >> b & 1ull) && (match_line < 0 || (uint32_t)(q % k) == (uint32_t)match_line) && q / k < hit_cap) hit[q / k] = 1;
        rd++;
    }
}

// What the three eval kernels (here, za_classify.hip, za_partition.hip) share.  lines: entries 0 .. lines of start[] are written.  -> the
// bytes of record r; *bad (~0 beforehand): the smallest r whose first byte is not first_byte.
__device__ __forceinline__ uint64_t za_rec_extent(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end, const unsigned long long *__restrict__ start,
                                                  uint64_t lines, uint64_t r, uint32_t k, int32_t first_byte, unsigned long long *__restrict__ bad)
{
    const uint64_t lo = (uint64_t)k * r, hi = lines - lo < k ? lines : lo + k;
    const uint64_t a = start[lo], e = start[hi];
    if (first_byte >= 0 && !(a >= text_off && a < text_end && scratch[a] == (uint32_t)first_byte)) atomicMin(bad, (unsigned long long)r);
    return e > a ? e - a : 0ull;
}

// What the three close kernels share, for a totals struct of any of them: where the rest behind the complete records begins, the lines
// of a short last record, and the fault `kind` at record b (b >= nrec: none).
template <typename Totals>
__device__ __forceinline__ void za_rec_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k, uint32_t flags, uint64_t text_end,
                                             uint64_t record_base, unsigned long long b, uint32_t kind, Totals *tot)
{
    const uint64_t whole = (uint64_t)k * (lines / k);                  // lines in complete records
    tot->tail_off = (flags & ZA_GREP_FINAL) ? text_end : start[whole];
    tot->short_lines = (flags & ZA_GREP_FINAL) ? (uint32_t)(lines - whole) : 0u;
    tot->bad = 0; tot->bad_record = 0; tot->bad_src = 0;
    if (b < nrec) { tot->bad = kind; tot->bad_record = record_base + b; tot->bad_src = start[(uint64_t)k * b]; }
}

// one thread.  nrec > 0.  The close kernel of the calls whose only fault is a wrong first byte and whose eval kernel has summed everything
// else already (za_dedup.hip, za_screen.hip, za_kcount.hip): covered, seen, and what za_rec_close sets.
template <typename Totals>
__global__ void za_k_rec_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k_lines, uint32_t flags, uint64_t text_end,
                               uint64_t record_base, const unsigned long long *__restrict__ bad, Totals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    tot->covered = 1; tot->seen = nrec;
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, bad[0], 1u, tot);
}

// grid: one thread per record.  sel[r] = 1 for a selected record, len[r] = its bytes (0 when it is not selected): what the scans sum.
__global__ __launch_bounds__(256) void za_k_grep_rec_eval(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end,
                                                          const unsigned long long *__restrict__ start, uint64_t lines, const uint8_t *__restrict__ hit,
                                                          uint64_t nrec, uint32_t k, uint32_t invert, int32_t first_byte,
                                                          unsigned long long *__restrict__ sel, unsigned long long *__restrict__ len,
                                                          unsigned long long *__restrict__ bad)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    const uint64_t n = za_rec_extent(scratch, text_off, text_end, start, lines, r, k, first_byte, bad);
    const uint32_t s = (hit[r] ? 1u : 0u) ^ invert;
    sel[r] = s;
    len[r] = s ? n : 0ull;
}

// one thread.  nrec > 0.  sum_sel / sum_len: the totals of the two scans.
__global__ void za_k_grep_rec_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k, uint32_t flags, uint64_t text_end,
                                    uint64_t record_base, const unsigned long long *__restrict__ sum_sel, const unsigned long long *__restrict__ sum_len,
                                    const unsigned long long *__restrict__ bad, ZaGrepRecTotals *__restrict__ totals)
{
    if (blockIdx.x || threadIdx.x) return;
    ZaGrepRecTotals z = {};
    z.covered = 1; z.seen = nrec; z.selected = *sum_sel; z.bytes = *sum_len;
    za_rec_close(start, lines, nrec, k, flags, text_end, record_base, *bad, 1u, &z);
    *totals = z;
}

// grid: one thread per record.  sel: the inclusive sums.  rows[] and lens[] have room for rows_cap entries (the host has read the
// totals: at least `selected`).
__global__ __launch_bounds__(256) void za_k_grep_rec_emit(const unsigned long long *__restrict__ sel, const unsigned long long *__restrict__ start, uint64_t lines,
                                                          uint64_t nrec, uint32_t k, uint64_t record_base, ZaGrepRow *__restrict__ rows, uint64_t rows_cap,
                                                          uint32_t *__restrict__ lens)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec) return;
    const unsigned long long idx = r ? sel[r - 1ull] : 0ull;
    if (sel[r] == idx || idx >= rows_cap) return;
    const uint64_t lo = (uint64_t)k * r, hi = lines - lo < k ? lines : lo + k;
    ZaGrepRow w; w.src_off = start[lo]; w.number = record_base + r; w.len = (uint32_t)(start[hi] - start[lo]); w.reserved = 0;
    rows[idx] = w; lens[idx] = w.len;
}

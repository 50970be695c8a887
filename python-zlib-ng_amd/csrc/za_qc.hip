// BGZF: records counted -- per-cycle base and quality tables, the length, GC and mean-quality distributions, the
// totals and a row of figures per record, what FastQC, fastp's report and seqkit stats -a print.  The prologue is that of za_trim.hip:
// the lines pass of za_grep.hip has run for the delimiters alone, the host has read how many lines the text holds, and
// za_k_grep_rec_lines of za_grep_records.hip has written where every line starts.  What is new:
//   za_k_qc_eval    a persistent grid; a workgroup owns a span of records.  A first sweep, one WAVE per record, reads every body whole
//                   in strips of 64 bytes: the record's figures, the three per-record histograms, the totals, the row at and beyond
//                   `cycles`, and strip 0 of the position tables.  Then the workgroup walks its span strip by strip, t = 1, 2, ..:
//                   every wave adds the bytes [64 t, 64 t + 64) of the records that have them into one LDS tile of 64 positions x 100
//                   counters, and the tile is added to the global tables once per strip.
//   za_k_qc_close   one thread: the fault words, tail_off, short_lines
// Every record of an Illumina file hits the same few (position, quality) words, so nothing is added to global memory per base or per
// record: counts are summed in LDS and leave a workgroup once per strip (the tile) or once per launch (everything else).  All sums are
// integers, so the result depends on the text and the configuration alone.
// Included by zng_amd.hip behind za_trim.hip (za_trim_body is what reads a line's body here too).
#include "za_common.h"

#define ZA_QC_MAX_CYCLES 4096u                         // mirror ZNGAMD_BGZF_QC_*
#define ZA_QC_BASES      6u
#define ZA_QC_QUALS      94u
#define ZA_QC_GC_BINS    101u
#define ZA_QC_ROWS       1u
#define ZA_QC_COLS       (ZA_QC_BASES + ZA_QC_QUALS)   // counters of a position: the classes, then the qualities
#define ZA_QC_STRIDE     (ZA_QC_COLS + 1u)             // dwords between two positions of the tile: odd, so that the 64 lanes of a wave, which
                                                       // hold 64 positions and often the same counter, fall on 32 different banks twice
                                                       // (with 100 they would fall on 8)
#define ZA_QC_HIST_MAX   (ZA_QC_MAX_CYCLES + 2u + ZA_QC_GC_BINS + ZA_QC_QUALS)      // length_hist, gc_hist, meanq_hist of a workgroup
// A workgroup's span of records.  Every 32-bit LDS counter grows by at most one per record (and strip), so a span below 2^32 records
// cannot overflow one; the row at `cycles`, where a record adds up to its length, is kept in 64 bits.
#define ZA_QC_SPAN_MIN   256u                          // below this a strip's flush (6400 counters read, the non-zero ones added) outweighs its records
#define ZA_QC_SPAN_MAX   (1u << 24)
#define ZA_QC_WG_PER_CU  3u                            // what 45 KB of LDS per workgroup let a CU hold

struct ZaQcRow { uint64_t qsum; uint32_t len, gc, n, low; };                                // mirrors zngamd_bgzf_qc_row
struct ZaQcTotals {                                    // mirrors zngamd_bgzf_qc_totals
    uint64_t seen, bytes_in, bases, min_len, max_len, empty, base_total[ZA_QC_BASES], quality_sum, q20_bases, q30_bases, low_bases, quality_clamped,
             tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, reserved;
};
struct ZaQcPar { uint32_t k_lines, seq_line; int32_t qual_line, first_byte; uint32_t quality_base, cycles, low_quality, delim; };

__device__ __forceinline__ uint32_t za_qc_class(uint32_t b)
{
    b &= 0xDFu;
    return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : b == 'N' ? 4u : 5u;
}

// Q and whether the byte was clamped
__device__ __forceinline__ uint32_t za_qc_quality(uint32_t byte, uint32_t base, bool *clamped)
{
    const int32_t d = (int32_t)byte - (int32_t)base;
    const int32_t q = d < 0 ? 0 : d > (int32_t)(ZA_QC_QUALS - 1u) ? (int32_t)(ZA_QC_QUALS - 1u) : d;
    *clamped = q != d;
    return (uint32_t)q;
}

__device__ __forceinline__ uint32_t za_wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// What both sweeps need of record r: the two bodies.  -> false: the record has qualities and the bodies differ in length (bad = 3);
// nothing of such a record is counted.
__device__ __forceinline__ bool za_qc_bodies(const uint8_t *__restrict__ scratch, const unsigned long long *__restrict__ start, uint64_t lines, uint64_t r, const ZaQcPar &P,
                                             uint64_t *ss, uint64_t *qs, uint32_t *n)
{
    const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
    const uint32_t nl = (uint32_t)(hi - lo);
    uint32_t nq = 0, sd, qd;
    *ss = za_trim_body(scratch, start, lo, nl, P.seq_line, P.delim, n, &sd);
    *qs = P.qual_line >= 0 ? za_trim_body(scratch, start, lo, nl, (uint32_t)P.qual_line, P.delim, &nq, &qd) : 0ull;
    return !(P.qual_line >= 0 && nq != *n);
}

// The whole workgroup: the tile's non-zero counters are added to rows 64 t .. 64 t + 63 of the two position tables (all below `cycles`:
// nothing else was added to the tile) and the tile is left zeroed.  Consecutive threads read consecutive dwords of the tile.
__device__ __forceinline__ void za_qc_flush_tile(uint32_t *s_tile, uint32_t t, uint32_t cycles, unsigned long long *__restrict__ base_pos,
                                                 unsigned long long *__restrict__ qual_pos)
{
    for (uint32_t idx = threadIdx.x; idx < 64u * ZA_QC_COLS; idx += blockDim.x) {
        const uint32_t pos = idx / ZA_QC_COLS, col = idx - pos * ZA_QC_COLS, at = pos * ZA_QC_STRIDE + col;
        const uint32_t v = s_tile[at];
        if (!v) continue;
        s_tile[at] = 0;
        const uint32_t p = 64u * t + pos;
        if (p >= cycles) continue;
        if (col < ZA_QC_BASES) atomicAdd(&base_pos[(uint64_t)p * ZA_QC_BASES + col], (unsigned long long)v);
        else atomicAdd(&qual_pos[(uint64_t)p * ZA_QC_QUALS + (col - ZA_QC_BASES)], (unsigned long long)v);
    }
}

// grid: workgroup g owns the records [g span, min(nrec, (g + 1) span)), ZA_QC_SPAN_MIN <= span <= ZA_QC_SPAN_MAX; wave w takes every
// fourth of them.  start, lines: as za_rec_extent takes them.  tables (zeroed): base_pos, qual_pos, length_hist, gc_hist, meanq_hist for
// P.cycles as zngamd_bgzf_qc_records lays them out.  row: a row per record, or no pointer.  tot (zeroed, min_len ~0): the sums; the two
// words behind it (~0 beforehand): the smallest r whose first byte is not first_byte, and the smallest r whose two bodies differ in length.
// Every byte read lies in the body of a line of the text; every barrier stands in control flow that is the same for the whole workgroup:
// the record loops hold none, and the strip loop's bound is the span's longest body, capped at cycles, read once behind a barrier.
__global__ __launch_bounds__(256) void za_k_qc_eval(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start, uint64_t lines,
                                                    uint64_t nrec, uint64_t span, ZaQcPar P, unsigned long long *__restrict__ tables, ZaQcRow *__restrict__ row,
                                                    ZaQcTotals *__restrict__ tot)
{
    __shared__ uint32_t s_tile[64u * ZA_QC_STRIDE];
    __shared__ uint32_t s_hist[ZA_QC_HIST_MAX];
    __shared__ unsigned long long s_over[ZA_QC_COLS];                              // the row at `cycles`
    __shared__ uint32_t s_maxn;
    const uint32_t C = P.cycles, nh = C + 2u + ZA_QC_GC_BINS + ZA_QC_QUALS;
    unsigned long long *__restrict__ base_pos = tables, *__restrict__ qual_pos = base_pos + (uint64_t)(C + 1u) * ZA_QC_BASES;
    unsigned long long *__restrict__ hists = qual_pos + (uint64_t)(C + 1u) * ZA_QC_QUALS;      // length_hist, gc_hist, meanq_hist lie as s_hist does
    unsigned long long *bad = (unsigned long long *)(tot + 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool has_q = P.qual_line >= 0;
    const uint64_t r0 = (uint64_t)blockIdx.x * span, r1 = nrec - r0 < span ? nrec : r0 + span;
    for (uint32_t i = tid; i < 64u * ZA_QC_STRIDE; i += 256u) s_tile[i] = 0;
    for (uint32_t i = tid; i < nh; i += 256u) s_hist[i] = 0;
    if (tid < ZA_QC_COLS) s_over[tid] = 0;
    if (tid == 0) s_maxn = 0;
    __syncthreads();
    uint32_t *s_len = s_hist, *s_gc = s_hist + C + 2u, *s_mq = s_gc + ZA_QC_GC_BINS;

    // ---- the first sweep: every record of the span whole.  What a record yields is the same for the 64 lanes of its wave (ballots, counts
    // and a wave sum), and so are the wave's sums over its records.
    uint64_t bytes_in = 0, bases = 0, quality_sum = 0, q20 = 0, q30 = 0, low = 0, clamped = 0, empty = 0;
    uint64_t bt0 = 0, bt1 = 0, bt2 = 0, bt3 = 0, bt4 = 0, bt5 = 0;
    uint32_t mn = 0xFFFFFFFFu, mx = 0, any = 0;
    #pragma unroll 1
    for (uint64_t r = r0 + wave; r < r1; r += 4u) {
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint64_t ra = start[lo], re = start[hi];
        if (lane == 0 && P.first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)P.first_byte)) atomicMin(&bad[0], (unsigned long long)r);
        uint64_t ss, qs; uint32_t n;
        if (!za_qc_bodies(scratch, start, lines, r, P, &ss, &qs, &n)) {
            if (lane == 0) atomicMin(&bad[1], (unsigned long long)r);
            continue;
        }
        uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, r_low = 0, r_q20 = 0, r_q30 = 0, r_cl = 0;
        uint64_t r_qsum = 0;
        const uint32_t ns = (uint32_t)(((uint64_t)n + 63u) >> 6);
        #pragma unroll 1
        for (uint32_t t = 0; t < ns; t++) {
            const uint32_t p0 = 64u * t;                                            // (< n)
            const bool in = lane < n - p0;
            const uint32_t cls = in ? za_qc_class(scratch[ss + p0 + lane]) : ZA_QC_BASES;
            c0 += (uint32_t)__popcll(__ballot(cls == 0u)); c1 += (uint32_t)__popcll(__ballot(cls == 1u)); c2 += (uint32_t)__popcll(__ballot(cls == 2u));
            c3 += (uint32_t)__popcll(__ballot(cls == 3u)); c4 += (uint32_t)__popcll(__ballot(cls == 4u));
            uint32_t Q = 0;
            if (has_q) {
                bool cl = false;
                if (in) Q = za_qc_quality(scratch[qs + p0 + lane], P.quality_base, &cl);
                r_qsum += za_wave_sum_u32(Q);
                r_q20 += (uint32_t)__popcll(__ballot(in && Q >= 20u)); r_q30 += (uint32_t)__popcll(__ballot(in && Q >= 30u));
                r_low += (uint32_t)__popcll(__ballot(in && Q < P.low_quality)); r_cl += (uint32_t)__popcll(__ballot(cl));
            }
            if (t == 0) {                                                           // strip 0 of the position tables
                if (in && lane < C) {
                    atomicAdd(&s_tile[lane * ZA_QC_STRIDE + cls], 1u);
                    if (has_q) atomicAdd(&s_tile[lane * ZA_QC_STRIDE + ZA_QC_BASES + Q], 1u);
                }
            }
            if (p0 + 64u > C || p0 >= C) {                                          // lanes at or beyond `cycles`: all of them share a row
                const bool over = in && (p0 >= C || lane >= C - p0);
                #pragma unroll
                for (uint32_t c = 0; c < ZA_QC_BASES; c++) {
                    const uint32_t cnt = (uint32_t)__popcll(__ballot(over && cls == c));
                    if (lane == 0 && cnt) atomicAdd(&s_over[c], (unsigned long long)cnt);
                }
                if (has_q && over) atomicAdd(&s_over[ZA_QC_BASES + Q], 1ull);
            }
        }
        const uint32_t ext = re > ra ? (uint32_t)(re - ra) : 0u, gc = c1 + c2;
        any = 1; bytes_in += ext; bases += n; quality_sum += r_qsum; low += r_low; q20 += r_q20; q30 += r_q30; clamped += r_cl;
        bt0 += c0; bt1 += c1; bt2 += c2; bt3 += c3; bt4 += c4; bt5 += n - (c0 + c1 + c2 + c3 + c4);
        mn = n < mn ? n : mn; mx = n > mx ? n : mx;
        if (!n) empty++;
        // (the wave's sums are touched once per record: they live in vector registers, the scalar ones are the strip loop's)
        asm volatile("" : "+v"(bytes_in), "+v"(bases), "+v"(quality_sum), "+v"(low), "+v"(q20), "+v"(q30), "+v"(clamped), "+v"(empty));
        asm volatile("" : "+v"(bt0), "+v"(bt1), "+v"(bt2), "+v"(bt3), "+v"(bt4), "+v"(bt5));
        if (lane == 0) {
            atomicAdd(&s_len[n <= C ? n : C + 1u], 1u);
            if (n) {
                atomicAdd(&s_gc[(uint32_t)((100ull * gc) / n)], 1u);
                if (has_q) atomicAdd(&s_mq[(uint32_t)(r_qsum / n)], 1u);
            }
            if (row) { ZaQcRow w; w.qsum = r_qsum; w.len = n; w.gc = gc; w.n = c4; w.low = r_low; row[r] = w; }
        }
    }
    if (lane == 0 && any) {
        atomicMax(&s_maxn, mx);
        atomicAdd((unsigned long long *)&tot->bytes_in, (unsigned long long)bytes_in);
        if (bases) atomicAdd((unsigned long long *)&tot->bases, (unsigned long long)bases);
        atomicMin((unsigned long long *)&tot->min_len, (unsigned long long)mn);
        atomicMax((unsigned long long *)&tot->max_len, (unsigned long long)mx);
        if (empty) atomicAdd((unsigned long long *)&tot->empty, (unsigned long long)empty);
        if (bt0) atomicAdd((unsigned long long *)&tot->base_total[0], (unsigned long long)bt0);
        if (bt1) atomicAdd((unsigned long long *)&tot->base_total[1], (unsigned long long)bt1);
        if (bt2) atomicAdd((unsigned long long *)&tot->base_total[2], (unsigned long long)bt2);
        if (bt3) atomicAdd((unsigned long long *)&tot->base_total[3], (unsigned long long)bt3);
        if (bt4) atomicAdd((unsigned long long *)&tot->base_total[4], (unsigned long long)bt4);
        if (bt5) atomicAdd((unsigned long long *)&tot->base_total[5], (unsigned long long)bt5);
        if (quality_sum) atomicAdd((unsigned long long *)&tot->quality_sum, (unsigned long long)quality_sum);
        if (q20) atomicAdd((unsigned long long *)&tot->q20_bases, (unsigned long long)q20);
        if (q30) atomicAdd((unsigned long long *)&tot->q30_bases, (unsigned long long)q30);
        if (low) atomicAdd((unsigned long long *)&tot->low_bases, (unsigned long long)low);
        if (clamped) atomicAdd((unsigned long long *)&tot->quality_clamped, (unsigned long long)clamped);
    }
    __syncthreads();

    // ---- the strips: strip 0 lies in the tile already
    const uint32_t top = s_maxn < C ? s_maxn : C, nstrips = (top + 63u) >> 6;      // (the same for the whole workgroup)
    #pragma unroll 1
    for (uint32_t t = 0; t < nstrips; t++) {
        if (t) {
            const uint32_t p0 = 64u * t;                                            // (< C)
            #pragma unroll 1
            for (uint64_t r = r0 + wave; r < r1; r += 4u) {
                uint64_t ss, qs; uint32_t n;
                if (!za_qc_bodies(scratch, start, lines, r, P, &ss, &qs, &n) || n <= p0) continue;
                if (lane < n - p0 && p0 + lane < C) {
                    atomicAdd(&s_tile[lane * ZA_QC_STRIDE + za_qc_class(scratch[ss + p0 + lane])], 1u);
                    if (has_q) {
                        bool cl;
                        atomicAdd(&s_tile[lane * ZA_QC_STRIDE + ZA_QC_BASES + za_qc_quality(scratch[qs + p0 + lane], P.quality_base, &cl)], 1u);
                    }
                }
            }
            __syncthreads();
        }
        za_qc_flush_tile(s_tile, t, C, base_pos, qual_pos);
        __syncthreads();
    }

    // ---- what left the sweep once per workgroup: the three histograms and the row at `cycles`
    for (uint32_t i = tid; i < nh; i += 256u) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&hists[i], (unsigned long long)v);
    }
    if (tid < ZA_QC_COLS && s_over[tid]) {
        if (tid < ZA_QC_BASES) atomicAdd(&base_pos[(uint64_t)C * ZA_QC_BASES + tid], s_over[tid]);
        else atomicAdd(&qual_pos[(uint64_t)C * ZA_QC_QUALS + (tid - ZA_QC_BASES)], s_over[tid]);
    }
}

// one thread.  nrec > 0.  tot holds the sums of za_k_qc_eval.  A record with both faults is reported for its first byte; otherwise the
// fault at the smaller record is.
__global__ void za_k_qc_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k_lines, uint32_t flags, uint64_t text_end,
                              uint64_t record_base, const unsigned long long *__restrict__ bad, ZaQcTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    tot->covered = 1; tot->seen = nrec;
    const unsigned long long fb = bad[0], lb = bad[1];
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, fb <= lb ? fb : lb, fb <= lb ? 1u : 3u, tot);
}

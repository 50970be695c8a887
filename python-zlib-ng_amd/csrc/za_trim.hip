// BGZF: records cut before they are written -- the fixed cut, the low-quality ends, the 3' adapter and the
// reads that are too short, what cutadapt / fastp / Trimmomatic do.  The prologue is that of za_partition.hip: the lines pass of
// za_grep.hip has run for the delimiters alone, the host has read how many lines the text holds, and za_k_grep_rec_lines of
// za_grep_records.hip has written where every line starts.  What is new:
//   za_k_trim_eval     one WAVE per record, 16 records one after the other: the cut [a, b) of its sequence body, the verdict, the
//                      trim row, the new length, the label za_k_part_hist / za_k_part_scatter take, the two faults, the sums
//   (za_k_part_hist, za_k_tbx_*, za_k_part_scatter of za_partition.hip)    the kept (and the too-short) records' rows, class by class
//   za_k_trim_close    one thread: the totals
//   za_k_trim_gather   one wave per row: the record's lines without what was cut, to where za_k_offsets says the row's bytes begin
// No thread walks a line: a body is read in strips of 64 bytes, a byte per lane.  The result depends on the text, the adapters, the
// configuration and the drop mask alone: sums and minima of integers do not depend on the order in which they are taken.
// Included by zng_amd.hip behind za_partition.hip.
#include "za_common.h"

#define ZA_TRIM_KEPT        0u                         // mirror ZNGAMD_BGZF_TRIM_KEPT / _TOO_SHORT / _DROPPED
#define ZA_TRIM_TOO_SHORT   1u
#define ZA_TRIM_DROPPED     2u
#define ZA_TRIM_KEEP_SHORT  1u                         // mirrors ZNGAMD_BGZF_TRIM_KEEP_SHORT (conf.flags)
#define ZA_TRIM_NO_ADAPTER  255u
#define ZA_TRIM_WG_RECORDS  64u                        // records per workgroup of za_k_trim_eval: 16 per wave
#define ZA_TRIM_STAGE_WORDS 80u                        // a strip of 64 positions and the 255 bytes behind it, as dwords

struct ZaTrimRow { uint32_t begin, end; uint8_t adapter, verdict, steps, reserved; };      // mirrors zngamd_bgzf_trim_row
struct ZaTrimTotals {                                  // mirrors zngamd_bgzf_trim_totals
    uint64_t seen, kept, too_short, dropped, bytes_in, bytes, bases_in, bases_out, quality_trimmed, adapter_trimmed, tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, drop_short;
    uint64_t adapter_records[ZA_GREP_MAX_PAT];
};
// what the rule needs beside the text: zngamd_bgzf_trim_conf, judged, and the delimiter, the adapter count and the longest adapter
struct ZaTrimPar {
    uint32_t k_lines, seq_line; int32_t qual_line, first_byte;
    uint32_t cut_front, cut_back, qual_front, qual_back, quality_base, max_mismatch, min_overlap, min_length, keep_short, delim, np, max_len;
};

// the body of line c of the record whose lines are [lo, lo + nl): where it starts and its bytes without the delimiter; a line the
// record lacks is an empty body.  The open last line of a _FINAL text holds no delimiter, every other line ends with one.
__device__ __forceinline__ uint64_t za_trim_body(const uint8_t *__restrict__ scratch, const unsigned long long *__restrict__ start, uint64_t lo, uint32_t nl, uint32_t c,
                                                 uint32_t delim, uint32_t *n, uint32_t *has_delim)
{
    *n = 0; *has_delim = 0;
    if (c >= nl) return 0;
    const uint64_t ls = start[lo + c], le = start[lo + c + 1u];
    uint32_t len = le > ls ? (uint32_t)(le - ls) : 0u;
    if (len && scratch[le - 1u] == delim) { len--; *has_delim = 1; }
    *n = len;
    return ls;
}

__device__ __forceinline__ int32_t za_wave_max_i32(int32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const int32_t o = __shfl_xor(v, d, 64); v = o > v ? o : v; }
    return v;
}

// One end of the quality rule (BWA's, the one behind cutadapt -q) over qual[a, b): back = true walks from b - 1 down to a and returns
// the new b, back = false walks from a up and returns the new a.  s = best = 0; every step adds cutoff - Q_i; s < 0 stops; s > best
// moves the cut.  A strip of 64 steps is a scan (the sums), a ballot (the first negative one) and a maximum with the lowest lane that
// holds it (the first step that reached it); s and best are carried from strip to strip in 64 bits.  The whole wave calls it.
template <bool BACK>
__device__ __forceinline__ uint32_t za_trim_quality(const uint8_t *__restrict__ qual, uint32_t a, uint32_t b, int32_t cutoff, int32_t base, uint32_t lane)
{
    long long s = 0, best = 0;
    uint32_t cut = BACK ? b : a, done = 0;
    const uint32_t m = b - a;
    #pragma unroll 1
    while (done < m) {
        const uint32_t cnt = m - done < 64u ? m - done : 64u;
        const uint32_t i = BACK ? b - 1u - done - lane : a + done + lane;
        const int32_t v = lane < cnt ? cutoff - ((int32_t)qual[i] - base) : 0;
        const int32_t inc = (int32_t)za_wave_incl_scan((uint32_t)v);
        const uint64_t neg = __ballot(lane < cnt && s + inc < 0);
        const uint32_t ok = neg ? (uint32_t)__builtin_ctzll(neg) : cnt;          // the steps in front of the stop
        if (ok) {
            const int32_t mx = za_wave_max_i32(lane < ok ? inc : INT32_MIN);
            if (s + mx > best) {
                best = s + mx;
                const uint32_t at = done + (uint32_t)__builtin_ctzll(__ballot(lane < ok && inc == mx));
                cut = BACK ? b - 1u - at : a + at + 1u;
            }
        }
        if (neg) break;
        s += __shfl(inc, (int)cnt - 1, 64);
        done += cnt;
    }
    return cut;
}

// The adapter rule over R = seq[0, m) (seq points at the cut's first byte): the smallest p at which an adapter matches, and the lowest
// such adapter.  Adapter j of L bytes matches at p with overlap o = min(L, m - p) when o >= min(min_overlap, L) and R[p, p + o) differs
// from its first o bytes in at most (k o) / L places.  A strip is 64 positions, one per lane; its bytes and the max_len - 1 behind them
// are staged in the wave's LDS as dwords (zeros behind m), and a lane compares four bytes a step as za_grep_approx_compare does: the
// loops over adapters and their dwords are the same for the whole wave, so the adapter words stay in scalar registers.  A lane leaves
// once it is past its budget, or once a lane below it has matched.  -> p (m: none); *which: the adapter.  The whole wave calls it.
__device__ __forceinline__ uint32_t za_trim_adapter(const uint8_t *__restrict__ seq, uint32_t m, const ZaTrimPar &P, const ZaGrepPat *__restrict__ ptab,
                                                    const uint32_t *__restrict__ words, uint32_t *s_t, uint32_t lane, uint32_t *which)
{
    const uint32_t nst = 16u + ((P.max_len + 3u) >> 2);                            // dwords a strip stages (<= ZA_TRIM_STAGE_WORDS)
    #pragma unroll 1
    for (uint32_t pos0 = 0; pos0 < m; pos0 += 64u) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();      // (the strip in front has been read)
        for (uint32_t w = lane; w < nst; w += 64u) {
            const uint32_t g = pos0 + 4u * w;
            uint32_t x = 0;
            if (g < m) {
                if (m - g >= 4u) x = za_ld32(seq + g);
                else for (uint32_t i = 0; i < m - g; i++) x |= (uint32_t)seq[g + i] << (8u * i);
            }
            s_t[w] = x;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
        const uint32_t p = pos0 + lane, w0 = lane >> 2, sh = lane & 3u;
        const uint32_t left = p < m ? m - p : 0u;                                  // bytes of R from p on
        bool alive = left != 0u;
        uint32_t mine = ZA_TRIM_NO_ADAPTER;
        #pragma unroll 1
        for (uint32_t q = 0; q < P.np; q++) {
            if (__ballot(alive) == 0ull) break;
            const ZaGrepPat pt = ptab[q];
            const uint32_t L = pt.len, nw = (L + 3u) >> 2, need = P.min_overlap < L ? P.min_overlap : L;
            const uint32_t *__restrict__ pw = words + pt.off;
            const uint32_t o = left < L ? left : L;
            uint32_t budget = P.max_mismatch;
            if (o < L) budget = (P.max_mismatch * o) / L;
            uint32_t c = alive && o >= need ? 0u : 256u;
            uint32_t lo = s_t[w0];
            #pragma unroll 1
            for (uint32_t j = 0; j < nw; j++) {
                const uint32_t hi = s_t[w0 + j + 1u];
                const uint32_t have = o > 4u * j ? o - 4u * j : 0u;               // bytes of this dword inside the overlap
                const uint32_t m80 = have >= 4u ? 0x80808080u : have ? 0x80808080u >> (8u * (4u - have)) : 0u;
                c += (uint32_t)__popc(za_nonzero_bytes(__builtin_amdgcn_alignbyte(hi, lo, sh) ^ pw[j]) & m80);
                lo = hi;
                if (__ballot(c <= budget) == 0ull) break;                          // every position of this wave has left
            }
            const uint64_t hit = __ballot(c <= budget);
            if (c <= budget) mine = q;
            if (hit) alive = alive && lane < (uint32_t)__builtin_ctzll(hit);       // (only a smaller p can still win)
        }
        const uint64_t any = __ballot(mine != ZA_TRIM_NO_ADAPTER);
        if (any) {
            const uint32_t l0 = (uint32_t)__builtin_ctzll(any);
            *which = (uint32_t)__shfl((int)mine, (int)l0, 64);
            return pos0 + l0;
        }
    }
    *which = ZA_TRIM_NO_ADAPTER;
    return m;
}

// grid: one workgroup per ZA_TRIM_WG_RECORDS records; wave w takes the records base + 4 i + w, i = 0 .. 15, one after the other.
// start, lines: as za_rec_extent takes them.  par: the adapters as grep_approx_params lays them out (the table, then at
// ZA_GREP_APAR_WORDS bytes the padded words).  drop[] (or no pointer: no record is dropped) is read below ndrop (<= nrec); a record at
// or beyond it is a dropped one.  row[r], len[r] (the bytes the record has once it is cut), lab[r] (0 kept, 1 too short and gathered,
// ZA_PART_DROP) for every record.  tot (zeroed): the sums; the two words behind it (~0 beforehand): the smallest r whose first byte is
// not first_byte, and the smallest r whose two bodies differ in length.  (Few pointers: the kernel lives on scalar registers.)
__global__ __launch_bounds__(256) void za_k_trim_eval(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start,
                                                      uint64_t lines, uint64_t nrec, ZaTrimPar P, const uint8_t *__restrict__ par,
                                                      const uint8_t *__restrict__ drop, uint64_t ndrop, ZaTrimRow *__restrict__ row, uint32_t *__restrict__ len,
                                                      uint16_t *__restrict__ lab, ZaTrimTotals *__restrict__ tot)
{
    const ZaGrepPat *__restrict__ ptab = (const ZaGrepPat *)par;
    const uint32_t *__restrict__ words = (const uint32_t *)(par + ZA_GREP_MAX_PAT * sizeof(ZaGrepPat));
    // The kernel lives on scalar registers: one record is a wave's, so nearly every value is the same for its 64 lanes.  What only lane 0
    // needs, and only when a record is done, is moved to vector registers by hand: the four output pointers here, a record's figures below.
    uint64_t o_row = (uint64_t)row, o_len = (uint64_t)len, o_lab = (uint64_t)lab, o_tot = (uint64_t)tot;
    asm volatile("" : "+v"(o_row), "+v"(o_len), "+v"(o_lab), "+v"(o_tot));
    ZaTrimTotals *v_tot = (ZaTrimTotals *)o_tot;
    unsigned long long *bad = (unsigned long long *)(v_tot + 1);
    __shared__ uint32_t s_t[4][ZA_TRIM_STAGE_WORDS];
    __shared__ uint32_t s_adp[ZA_GREP_MAX_PAT];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    if (tid < ZA_GREP_MAX_PAT) s_adp[tid] = 0;
    __syncthreads();
    uint32_t n_kept = 0, n_short = 0, n_drop = 0;
    uint64_t bytes_in = 0, bases_in = 0, bases_out = 0, q_trim = 0, a_trim = 0;
    #pragma unroll 1
    for (uint32_t it = 0; it < ZA_TRIM_WG_RECORDS / 4u; it++) {                    // (the same for every lane of a wave; no barrier in this loop)
        const uint64_t r = (uint64_t)blockIdx.x * ZA_TRIM_WG_RECORDS + 4u * it + wave;
        if (r >= nrec) break;
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint32_t nl = (uint32_t)(hi - lo);
        const uint64_t ra = start[lo], re = start[hi];
        const uint32_t ext = re > ra ? (uint32_t)(re - ra) : 0u;
        if (lane == 0 && P.first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)P.first_byte)) atomicMin(&bad[0], (unsigned long long)r);
        uint32_t v_drop = drop && (r >= ndrop || drop[r]) ? 1u : 0u;
        uint32_t n, nq = 0, sd, qd = 0;
        const uint64_t ss = za_trim_body(scratch, start, lo, nl, P.seq_line, P.delim, &n, &sd);
        const uint64_t qs = P.qual_line >= 0 ? za_trim_body(scratch, start, lo, nl, (uint32_t)P.qual_line, P.delim, &nq, &qd) : 0ull;
        const bool differ = P.qual_line >= 0 && nq != n;
        if (differ && lane == 0) atomicMin(&bad[1], (unsigned long long)r);
        uint32_t v_ext = ext, v_n = n, v_lines = (P.seq_line < nl ? 1u : 0u) + (P.qual_line >= 0 && (uint32_t)P.qual_line < nl ? 1u : 0u);      // (the lines that are cut)
        asm volatile("" : "+v"(v_drop), "+v"(v_ext), "+v"(v_n), "+v"(v_lines));
        // 1. the fixed cut
        uint32_t a = P.cut_front < n ? P.cut_front : n;
        uint32_t b = n - (P.cut_back < n ? P.cut_back : n);
        if (b < a) b = a;
        uint32_t steps = (a != 0u || b != n) ? 1u : 0u, q_cut = 0, a_cut = 0;
        // 2. the quality ends, both over the [a, b) of step 1 (a record at fault is cut no further: nothing of it is written)
        if (!differ && P.qual_line >= 0 && b > a) {
            const uint32_t nb = P.qual_back ? za_trim_quality<true>(scratch + qs, a, b, (int32_t)P.qual_back, (int32_t)P.quality_base, lane) : b;
            const uint32_t na = P.qual_front ? za_trim_quality<false>(scratch + qs, a, b, (int32_t)P.qual_front, (int32_t)P.quality_base, lane) : a;
            if (na != a || nb != b) steps |= 2u;
            q_cut = (b - a) - ((nb > na ? nb : na) - na);
            a = na; b = nb > na ? nb : na;
        }
        asm volatile("" : "+v"(steps), "+v"(q_cut));
        // 3. the adapters
        uint32_t which = ZA_TRIM_NO_ADAPTER;
        if (!differ && P.np && b > a) {
            const uint32_t p = za_trim_adapter(scratch + ss + a, b - a, P, ptab, words, s_t[wave], lane, &which);
            if (which != ZA_TRIM_NO_ADAPTER) {
                steps |= 4u; a_cut = (b - a) - p; b = a + p;
                if (lane == 0) atomicAdd(&s_adp[which], 1u);
            }
        }
        // 4. the verdict
        if (lane == 0) {                                                           // (the sums live in lane 0's registers)
            const uint32_t verdict = v_drop ? ZA_TRIM_DROPPED : b - a < P.min_length ? ZA_TRIM_TOO_SHORT : ZA_TRIM_KEPT;
            const uint32_t newlen = differ ? v_ext : v_ext - (v_n - (b - a)) * v_lines;
            bytes_in += v_ext; bases_in += v_n; q_trim += q_cut; a_trim += a_cut;
            if (verdict == ZA_TRIM_KEPT) { n_kept++; bases_out += b - a; }
            else if (verdict == ZA_TRIM_TOO_SHORT) n_short++;
            else n_drop++;
            ZaTrimRow w; w.begin = a; w.end = b; w.adapter = (uint8_t)which; w.verdict = (uint8_t)verdict; w.steps = (uint8_t)steps; w.reserved = 0;
            ((ZaTrimRow *)o_row)[r] = w; ((uint32_t *)o_len)[r] = newlen;
            ((uint16_t *)o_lab)[r] = (uint16_t)(verdict == ZA_TRIM_KEPT ? 0u : verdict == ZA_TRIM_TOO_SHORT && P.keep_short ? 1u : ZA_PART_DROP);
        }
    }
    if (lane == 0) {
        if (n_kept) atomicAdd((unsigned long long *)&v_tot->kept, (unsigned long long)n_kept);
        if (n_short) atomicAdd((unsigned long long *)&v_tot->too_short, (unsigned long long)n_short);
        if (n_drop) atomicAdd((unsigned long long *)&v_tot->dropped, (unsigned long long)n_drop);
        if (bytes_in) atomicAdd((unsigned long long *)&v_tot->bytes_in, (unsigned long long)bytes_in);
        if (bases_in) atomicAdd((unsigned long long *)&v_tot->bases_in, (unsigned long long)bases_in);
        if (bases_out) atomicAdd((unsigned long long *)&v_tot->bases_out, (unsigned long long)bases_out);
        if (q_trim) atomicAdd((unsigned long long *)&v_tot->quality_trimmed, (unsigned long long)q_trim);
        if (a_trim) atomicAdd((unsigned long long *)&v_tot->adapter_trimmed, (unsigned long long)a_trim);
    }
    __syncthreads();
    if (tid < ZA_GREP_MAX_PAT && s_adp[tid]) atomicAdd((unsigned long long *)&v_tot->adapter_records[tid], (unsigned long long)s_adp[tid]);
}

// one thread.  nrec > 0.  cnt[]: the sums of za_k_part_hist for the two classes (records, then bytes); tot holds the sums of
// za_k_trim_eval.  A record with both faults is reported for its first byte; otherwise the fault at the smaller record is.
__global__ void za_k_trim_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint64_t ndrop, uint32_t has_mask, uint32_t k_lines,
                                uint32_t flags, uint64_t text_end, uint64_t record_base, const unsigned long long *__restrict__ cnt,
                                const unsigned long long *__restrict__ bad, ZaTrimTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    tot->covered = 1; tot->seen = nrec; tot->bytes = cnt[2] + cnt[3]; tot->drop_short = has_mask && ndrop < nrec ? 1u : 0u;
    const unsigned long long fb = bad[0], lb = bad[1];
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, fb <= lb ? fb : lb, fb <= lb ? 1u : 3u, tot);
}

// grid: one wave per row, four rows per workgroup.  rows[i] (number = record_base + r) is written at out + offs[i], rows[i].len bytes:
// the record's lines in order, lines seq_line and qual_line without the bodies' bytes in front of row[r].begin and from row[r].end on,
// every delimiter the source has.  That is at most five ranges of the source, copied one after the other, 64 bytes a step.  Every byte
// read lies in a line of the text, so in what the lines pass reported as covered; nothing is written at or behind out_cap.
__global__ __launch_bounds__(256) void za_k_trim_gather(const uint8_t *__restrict__ scratch, const unsigned long long *__restrict__ start, uint64_t lines,
                                                        uint64_t record_base, uint32_t k_lines, uint32_t seq_line, int32_t qual_line, uint32_t delim,
                                                        const ZaTrimRow *__restrict__ row, const ZaGrepRow *__restrict__ rows, const uint64_t *__restrict__ offs,
                                                        uint64_t n, uint8_t *__restrict__ out, uint64_t out_cap)
{
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t i = (uint64_t)blockIdx.x * 4u + wave;
    if (i >= n) return;
    const uint64_t r = rows[i].number - record_base;
    const uint64_t lo = (uint64_t)k_lines * r, hi = lines - lo < k_lines ? lines : lo + k_lines;
    const uint32_t nl = (uint32_t)(hi - lo);
    const ZaTrimRow t = row[r];
    // the two cut lines in the order they lie in the record
    const uint32_t c0 = qual_line >= 0 && (uint32_t)qual_line < seq_line ? (uint32_t)qual_line : seq_line;
    const uint32_t c1 = qual_line >= 0 ? ((uint32_t)qual_line < seq_line ? seq_line : (uint32_t)qual_line) : k_lines;
    uint64_t at = start[lo], d = offs[i];
    const uint64_t end = start[hi];
    if (end < at || d > out_cap || out_cap - d < rows[i].len) return;
    auto copy = [&](uint64_t from, uint64_t c) {
        for (uint64_t j = lane; j < c; j += 64u) out[d + j] = scratch[from + j];
        d += c;
    };
    uint32_t nb, hd;
    if (c0 < nl) { const uint64_t ls = za_trim_body(scratch, start, lo, nl, c0, delim, &nb, &hd); copy(at, ls - at); copy(ls + t.begin, t.end - t.begin); at = ls + nb; }
    if (c1 < nl) { const uint64_t ls = za_trim_body(scratch, start, lo, nl, c1, delim, &nb, &hd); copy(at, ls - at); copy(ls + t.begin, t.end - t.begin); at = ls + nb; }
    copy(at, end - at);
}

// BGZF: read pairs laid over each other -- the overlap of the two mates of an interleaved pair, the bases
// corrected in it, the adapter read-through cut off and the pair merged into one read: what fastp -c / -m, bbmerge, PEAR, FLASH and
// vsearch --fastq_mergepairs do.  The prologue is that of za_trim.hip: the lines pass of za_grep.hip has run for the delimiters alone,
// the host has read how many lines the text holds, and za_k_grep_rec_lines of za_grep_records.hip has written where every line starts.
// What is new:
//   za_k_ovl_eval      one WAVE per pair, 16 pairs one after the other: mate 1 and the reverse complement of mate 2 staged in LDS, a
//                      candidate offset per lane, 64 a round in the order of shrinking overlaps; the winner, the overlap row, the new
//                      length, the label za_k_part_hist / za_k_part_scatter take, the two faults, the sums
//   (za_k_part_hist, za_k_tbx_*, za_k_part_scatter of za_partition.hip)    the merged (and the other) pairs' rows, class by class
//   za_k_ovl_close     one thread: the totals
//   za_k_ovl_gather    one wave per row: the merged read in mate 1's lines, or the pair as correction and cut left it, to where
//                      za_k_offsets says the row's bytes begin; every byte a function of the text, the row's offset and the rule
// Nothing is kept between eval and gather but the 16-byte rows.  The result depends on the text and the configuration alone: sums and
// minima of integers do not depend on the order in which they are taken.
// Included by zng_amd.hip behind za_trim.hip and za_dedup.hip (za_trim_body reads a line's body, za_key_comp complements a base).
#include "za_common.h"

#define ZA_OVL_NONE          0u                        // mirror ZNGAMD_BGZF_OVERLAP_NONE / _FOUND / _MERGED / _TOO_LONG
#define ZA_OVL_FOUND         1u
#define ZA_OVL_MERGED        2u
#define ZA_OVL_TOO_LONG      3u
#define ZA_OVL_MERGE         1u                        // mirror ZNGAMD_BGZF_OVERLAP_MERGE / _CORRECT / _CUT / _KEEP_UNMERGED (conf.flags)
#define ZA_OVL_CORRECT       2u
#define ZA_OVL_CUT           4u
#define ZA_OVL_KEEP_UNMERGED 8u
#define ZA_OVL_MAX_READ      1024u                     // mirrors ZNGAMD_BGZF_OVERLAP_MAX_READ
#define ZA_OVL_WG_RECORDS    64u                       // pairs per workgroup of za_k_ovl_eval: 16 per wave
#define ZA_OVL_STAGE_WORDS   (ZA_OVL_MAX_READ / 4u + 2u)      // a mate as dwords and the two a compare may read behind its last byte
#define ZA_OVL_NO_KEY        0xFFFFFFFFu
#define ZA_OVL_SUMS          15u                       // the words of ZaOvlTotals from `seen` to `mismatch_sum`

struct ZaOvlRow { int32_t offset; uint32_t insert; uint16_t overlap, mismatches, corrected; uint8_t verdict, steps; };      // mirrors zngamd_bgzf_overlap_row
struct ZaOvlTotals {                                   // mirrors zngamd_bgzf_overlap_totals
    uint64_t seen, none, found, merged, too_long, bytes_in, bytes, bases_in, bases_merged, corrected, corrected_pairs, adapter_pairs, adapter_trimmed,
             overlap_sum, mismatch_sum, tail_off, bad_record, bad_src;
    uint32_t covered, short_lines, bad, reserved;
};
// zngamd_bgzf_overlap_conf, judged, and the delimiter; m_lines = k_lines / 2
struct ZaOvlPar {
    uint32_t k_lines, m_lines, seq_line; int32_t qual_line, first_byte;
    uint32_t quality_base, min_overlap, max_mismatch, max_percent; int32_t q_high, q_low; uint32_t flags, delim;
};

// The four bodies of a pair and the winner of its search, as both kernels read them: a = scratch + sa (n1 bytes), y = scratch + sy
// (n2 bytes), the qualities at qa and qy (qual_line >= 0 only); o the offset, found: an overlap was accepted.
struct ZaOvlPair { uint64_t sa, qa, sy, qy; uint32_t n1, n2; int32_t o; bool found; };

// step 2 at position i of a, which lies in the overlap and where a[i] != b[i - o]: 1 mate 2 takes mate 1's byte, 2 mate 1 takes b's, 0 neither
__device__ __forceinline__ uint32_t za_ovl_correct(const uint8_t *__restrict__ scratch, const ZaOvlPair &p, const ZaOvlPar &P, uint32_t i)
{
    const int32_t Qa = (int32_t)scratch[p.qa + i] - (int32_t)P.quality_base;
    const int32_t Qb = (int32_t)scratch[p.qy + (p.n2 - 1u - (uint32_t)((int32_t)i - p.o))] - (int32_t)P.quality_base;
    return Qa >= P.q_high && Qb <= P.q_low ? 1u : Qb >= P.q_high && Qa <= P.q_low ? 2u : 0u;
}

// grid: one workgroup per ZA_OVL_WG_RECORDS pairs; wave w takes the pairs base + 4 i + w, i = 0 .. 15, one after the other.  start,
// lines: as za_rec_extent takes them.  row[r], len[r] (the bytes the pair has as it is written), lab[r] (0 merged, 1 any other pair
// that is gathered, ZA_PART_DROP) for every pair.  tot (zeroed): the sums; the two words behind it (~0 beforehand): the smallest r of
// which line 0 or line m does not begin with first_byte, and the smallest r of which a mate's two bodies differ in length.
// LDS: per wave a and b as dwords, zeros behind their last byte.  Lane l of a round compares a[ia + 4 j ..] with b[ib + 4 j ..] for one
// offset; ia + L <= n1 and ib + L <= n2, so the dwords it reads lie below (n + 3) / 4 + 1 <= ZA_OVL_STAGE_WORDS.  Lanes of a plateau
// read consecutive bytes (four lanes a dword: a broadcast), lanes of the two slopes read one stream at consecutive bytes and the other
// at its first dword, so a ds_read_b32 meets at most a two-way conflict.
__global__ __launch_bounds__(256) void za_k_ovl_eval(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start,
                                                     uint64_t lines, uint64_t nrec, ZaOvlPar P, ZaOvlRow *__restrict__ row, uint32_t *__restrict__ len,
                                                     uint16_t *__restrict__ lab, ZaOvlTotals *__restrict__ tot)
{
    unsigned long long *bad = (unsigned long long *)(tot + 1);
    __shared__ uint32_t s_a[4][ZA_OVL_STAGE_WORDS], s_b[4][ZA_OVL_STAGE_WORDS];
    __shared__ uint32_t s_sum[ZA_OVL_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    uint32_t *sa = s_a[wave], *sb = s_b[wave];
    if (tid < ZA_OVL_SUMS) s_sum[tid] = 0;
    __syncthreads();
    const uint32_t nq = P.qual_line >= 0 ? 2u : 1u;                                // the lines of a mate that change
    uint32_t n_none = 0, n_found = 0, n_merged = 0, n_long = 0;                    // (the sums live in lane 0's registers)
    uint32_t bytes_in = 0, bases_in = 0, bases_merged = 0, corr = 0, corr_pairs = 0, ad_pairs = 0, ad_bases = 0, ov_sum = 0, mm_sum = 0;
    #pragma unroll 1
    for (uint32_t it = 0; it < ZA_OVL_WG_RECORDS / 4u; it++) {                     // (the same for every lane of a wave; no barrier in this loop)
        const uint64_t r = (uint64_t)blockIdx.x * ZA_OVL_WG_RECORDS + 4u * it + wave;
        if (r >= nrec) break;
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint32_t nl = (uint32_t)(hi - lo);
        const uint64_t ra = start[lo], re = start[hi];
        const uint32_t ext = re > ra ? (uint32_t)(re - ra) : 0u;
        if (lane == 0 && P.first_byte >= 0) {
            bool ok = ra < text_end && scratch[ra] == (uint32_t)P.first_byte;
            if (ok) { const uint64_t rm = P.m_lines < nl ? start[lo + P.m_lines] : text_end; ok = rm < text_end && scratch[rm] == (uint32_t)P.first_byte; }
            if (!ok) atomicMin(&bad[0], (unsigned long long)r);
        }
        ZaOvlPair p;
        uint32_t dl, nqa = 0, nqy = 0;
        p.sa = za_trim_body(scratch, start, lo, nl, P.seq_line, P.delim, &p.n1, &dl);
        p.sy = za_trim_body(scratch, start, lo, nl, P.m_lines + P.seq_line, P.delim, &p.n2, &dl);
        p.qa = P.qual_line >= 0 ? za_trim_body(scratch, start, lo, nl, (uint32_t)P.qual_line, P.delim, &nqa, &dl) : 0ull;
        p.qy = P.qual_line >= 0 ? za_trim_body(scratch, start, lo, nl, P.m_lines + (uint32_t)P.qual_line, P.delim, &nqy, &dl) : 0ull;
        const bool differ = P.qual_line >= 0 && (nqa != p.n1 || nqy != p.n2);
        if (differ && lane == 0) atomicMin(&bad[1], (unsigned long long)r);
        const uint32_t n1 = p.n1, n2 = p.n2;
        const bool too_long = n1 > ZA_OVL_MAX_READ || n2 > ZA_OVL_MAX_READ;
        uint32_t best = ZA_OVL_NO_KEY;
        // 1. the search (a pair at fault is not searched: nothing of it is written)
        if (!differ && !too_long && n1 && n2) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();      // (the pair in front has been read)
            const uint32_t nwa = ((n1 + 3u) >> 2) + 2u, nwb = ((n2 + 3u) >> 2) + 2u;
            for (uint32_t w = lane; w < nwa; w += 64u) {
                const uint32_t g = 4u * w;
                uint32_t x = 0;
                if (g < n1) {
                    if (n1 - g >= 4u) x = za_ld32(scratch + p.sa + g);
                    else for (uint32_t i = 0; i < n1 - g; i++) x |= (uint32_t)scratch[p.sa + g + i] << (8u * i);
                }
                sa[w] = x;
            }
            for (uint32_t w = lane; w < nwb; w += 64u) sb[w] = 0;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
            for (uint32_t j = lane; j < n2; j += 64u) ((uint8_t *)sb)[j] = (uint8_t)za_key_comp(scratch[p.sy + (n2 - 1u - j)]);      // b, a byte per lane
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
            // candidate t: the |n1 - n2| + 1 offsets of the longest overlap first, then for every shorter L the two offsets that have it
            const uint32_t Lmax = n1 < n2 ? n1 : n2, plateau = (n1 < n2 ? n2 - n1 : n1 - n2) + 1u, total = n1 + n2 - 1u;
            #pragma unroll 1
            for (uint32_t t0 = 0; t0 < total; t0 += 64u) {
                const uint32_t Lr = t0 < plateau ? Lmax : Lmax - 1u - ((t0 - plateau) >> 1);      // the longest overlap of this round
                if (Lr < P.min_overlap || (best != ZA_OVL_NO_KEY && Lr < ZA_OVL_MAX_READ - (best >> 22))) break;
                const uint32_t t = t0 + lane;
                uint32_t L = Lmax;
                int32_t o = n1 >= n2 ? (int32_t)t : -(int32_t)t;
                if (t >= plateau) {
                    L = Lmax - 1u - ((t - plateau) >> 1);
                    o = ((t - plateau) & 1u) ? -(int32_t)(n2 - L) : (int32_t)(n1 - L);
                }
                bool alive = t < total && L >= P.min_overlap;
                if (!alive) L = 0;
                const uint32_t pct = (L * P.max_percent) / 100u, limit = pct < P.max_mismatch ? pct : P.max_mismatch;
                const uint32_t ia = alive && o > 0 ? (uint32_t)o : 0u, ib = alive && o < 0 ? (uint32_t)(-o) : 0u;
                const uint32_t wa = ia >> 2, wb = ib >> 2, nsteps = (L + 3u) >> 2;
                uint32_t d = 0, loa = sa[wa], lob = sb[wb];
                #pragma unroll 1
                for (uint32_t j = 0; ; j++) {
                    const bool on = alive && j < nsteps;
                    if (__ballot(on) == 0ull) break;                               // every offset of this round has left or is through
                    if (on) {
                        const uint32_t hia = sa[wa + j + 1u], hib = sb[wb + j + 1u];
                        const uint32_t have = L - 4u * j;                          // bytes of this dword inside the overlap
                        const uint32_t m80 = have >= 4u ? 0x80808080u : 0x80808080u >> (8u * (4u - have));
                        d += (uint32_t)__popc(za_nonzero_bytes(__builtin_amdgcn_alignbyte(hia, loa, ia & 3u) ^ __builtin_amdgcn_alignbyte(hib, lob, ib & 3u)) & m80);
                        loa = hia; lob = hib;
                        if (d > limit) alive = false;                              // past its limit
                    }
                }
                const uint32_t ao = (uint32_t)(o < 0 ? -o : o);
                uint32_t key = alive ? (ZA_OVL_MAX_READ - L) << 22 | d << 11 | ao << 1 | (o < 0 ? 1u : 0u) : ZA_OVL_NO_KEY;
                #pragma unroll
                for (int s = 32; s >= 1; s >>= 1) { const uint32_t x = (uint32_t)__shfl_xor((int)key, s, 64); key = x < key ? x : key; }
                best = key < best ? key : best;
            }
        }
        best = (uint32_t)__builtin_amdgcn_readfirstlane((int)best);
        p.found = best != ZA_OVL_NO_KEY;
        const uint32_t L = p.found ? ZA_OVL_MAX_READ - (best >> 22) : 0u, d = p.found ? (best >> 11) & 0x7FFu : 0u;
        p.o = p.found ? ((best & 1u) ? -(int32_t)((best >> 1) & 0x3FFu) : (int32_t)((best >> 1) & 0x3FFu)) : 0;
        // 2. the corrected positions of the winner, a strip of 64 positions of the overlap at a time (a and b are still staged)
        uint32_t ncorr = 0;
        if (p.found && (P.flags & ZA_OVL_CORRECT)) {
            const uint32_t ia = p.o > 0 ? (uint32_t)p.o : 0u;
            for (uint32_t q0 = 0; q0 < L; q0 += 64u) {
                const uint32_t i = ia + q0 + lane;
                bool c = false;
                if (q0 + lane < L && ((const uint8_t *)sa)[i] != ((const uint8_t *)sb)[(uint32_t)((int32_t)i - p.o)]) c = za_ovl_correct(scratch, p, P, i) != 0u;
                ncorr += (uint32_t)__popcll(__ballot(c));
            }
        }
        // 3, 4 and the verdict
        if (lane == 0) {
            const uint32_t insert = p.found ? (uint32_t)(p.o + (int32_t)n2) : 0u;
            const bool cut = p.found && (P.flags & ZA_OVL_CUT), merged = p.found && (P.flags & ZA_OVL_MERGE);
            const uint32_t e1 = cut && insert < n1 ? insert : n1, e2 = cut && p.o < 0 ? (uint32_t)((int32_t)n2 + p.o) : n2;
            const uint32_t verdict = too_long ? ZA_OVL_TOO_LONG : merged ? ZA_OVL_MERGED : p.found ? ZA_OVL_FOUND : ZA_OVL_NONE;
            uint32_t newlen = ext;
            if (!differ && merged) newlen = (uint32_t)(start[lo + P.m_lines] - ra) + (insert - n1) * nq;      // (unsigned wrap: insert may lie on either side of n1)
            else if (!differ) newlen = ext - ((n1 - e1) + (n2 - e2)) * nq;
            if (too_long) n_long++; else if (merged) n_merged++; else if (p.found) n_found++; else n_none++;
            bytes_in += ext; bases_in += n1 + n2; ov_sum += L; mm_sum += d;
            if (merged) bases_merged += insert;
            if (ncorr) { corr += ncorr; corr_pairs++; }
            if (e1 != n1 || e2 != n2) { ad_pairs++; ad_bases += (n1 - e1) + (n2 - e2); }
            ZaOvlRow w; w.offset = p.o; w.insert = insert; w.overlap = (uint16_t)L; w.mismatches = (uint16_t)d; w.corrected = (uint16_t)ncorr;
            w.verdict = (uint8_t)verdict; w.steps = (uint8_t)((e1 != n1 ? 1u : 0u) | (e2 != n2 ? 2u : 0u) | (ncorr ? 4u : 0u));
            row[r] = w; len[r] = newlen;
            lab[r] = (uint16_t)(merged ? 0u : (P.flags & ZA_OVL_KEEP_UNMERGED) ? 1u : ZA_PART_DROP);
        }
    }
    if (lane == 0) {                                                               // the workgroup's sums, word by word as ZaOvlTotals has them
        const uint32_t v[ZA_OVL_SUMS] = {0, n_none, n_found, n_merged, n_long, bytes_in, 0, bases_in, bases_merged, corr, corr_pairs,
                                         ad_pairs, ad_bases, ov_sum, mm_sum};
        #pragma unroll
        for (uint32_t i = 0; i < ZA_OVL_SUMS; i++) if (v[i]) atomicAdd(&s_sum[i], v[i]);
    }
    __syncthreads();
    if (tid < ZA_OVL_SUMS && s_sum[tid]) atomicAdd((unsigned long long *)tot + tid, (unsigned long long)s_sum[tid]);      // one atomic per workgroup per total
}

// one thread.  nrec > 0.  cnt[]: the sums of za_k_part_hist for the two classes (records, then bytes); tot holds the sums of
// za_k_ovl_eval.  A pair with both faults is reported for its first byte; otherwise the fault at the smaller record is.
__global__ void za_k_ovl_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k_lines, uint32_t flags, uint64_t text_end,
                               uint64_t record_base, const unsigned long long *__restrict__ cnt, const unsigned long long *__restrict__ bad,
                               ZaOvlTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    tot->covered = 1; tot->seen = nrec; tot->bytes = cnt[2] + cnt[3];
    const unsigned long long fb = bad[0], lb = bad[1];
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, fb <= lb ? fb : lb, fb <= lb ? 1u : 3u, tot);
}

// One byte of what is written, each a function of the text, the pair's offset and the rule.  qual: the byte of the quality line.
// position c of the merged read (step 4): the mate that covers it, of two the one with the higher Q, mate 1 on ties
__device__ __forceinline__ uint8_t za_ovl_merged_byte(const uint8_t *__restrict__ scratch, const ZaOvlPair &p, const ZaOvlPar &P, uint32_t c, bool qual)
{
    const bool in_a = c < p.n1, in_b = (int32_t)c >= p.o;
    const uint32_t yi = p.n2 - 1u - (uint32_t)((int32_t)c - p.o);                  // where b[c - o] lies in y (read only with in_b)
    bool use_a = in_a;
    if (in_a && in_b && P.qual_line >= 0) use_a = scratch[p.qa + c] >= scratch[p.qy + yi];      // (the same base on both sides: Qa >= Qb)
    if (use_a) return scratch[(qual ? p.qa : p.sa) + c];
    return qual ? scratch[p.qy + yi] : (uint8_t)za_key_comp(scratch[p.sy + yi]);
}

// position i of mate 1 as step 2 leaves it
__device__ __forceinline__ uint8_t za_ovl_mate1_byte(const uint8_t *__restrict__ scratch, const ZaOvlPair &p, const ZaOvlPar &P, uint32_t i, bool qual)
{
    const uint8_t own = scratch[(qual ? p.qa : p.sa) + i];
    const int32_t j = (int32_t)i - p.o;
    if (!(p.found && (P.flags & ZA_OVL_CORRECT)) || j < 0 || j >= (int32_t)p.n2) return own;
    const uint32_t yi = p.n2 - 1u - (uint32_t)j;
    const uint8_t b = (uint8_t)za_key_comp(scratch[p.sy + yi]);
    if (scratch[p.sa + i] == b || za_ovl_correct(scratch, p, P, i) != 2u) return own;
    return qual ? scratch[p.qy + yi] : b;
}

// position yi of mate 2 as step 2 leaves it
__device__ __forceinline__ uint8_t za_ovl_mate2_byte(const uint8_t *__restrict__ scratch, const ZaOvlPair &p, const ZaOvlPar &P, uint32_t yi, bool qual)
{
    const uint8_t own = scratch[(qual ? p.qy : p.sy) + yi];
    const int32_t i = p.o + (int32_t)(p.n2 - 1u - yi);
    if (!(p.found && (P.flags & ZA_OVL_CORRECT)) || i < 0 || i >= (int32_t)p.n1) return own;
    const uint8_t a = scratch[p.sa + (uint32_t)i];
    if (a == (uint8_t)za_key_comp(scratch[p.sy + yi]) || za_ovl_correct(scratch, p, P, (uint32_t)i) != 1u) return own;
    return qual ? scratch[p.qa + (uint32_t)i] : (uint8_t)za_key_comp(a);
}

// grid: one wave per row, four rows per workgroup.  rows[i] (number = record_base + r) is written at out + offs[i], rows[i].len bytes.
// A merged pair: mate 1's m lines, lines s and q with the `insert` bytes of step 4, every other line whole, every delimiter the source
// has.  Any other pair: its k lines, lines s, q, m + s, m + q as steps 2 and 3 left them.  Between the changed bodies the source is
// copied, 64 bytes a step.  Every byte read lies in a line of the text, so in what the lines pass reported as covered; nothing is
// written at or behind out_cap.  An offset is trusted only as far as it keeps every index inside its body: row[] is the one eval wrote
// for this text.
__global__ __launch_bounds__(256) void za_k_ovl_gather(const uint8_t *__restrict__ scratch, const unsigned long long *__restrict__ start, uint64_t lines,
                                                       uint64_t record_base, ZaOvlPar P, const ZaOvlRow *__restrict__ row, const ZaGrepRow *__restrict__ rows,
                                                       const uint64_t *__restrict__ offs, uint64_t n, uint8_t *__restrict__ out, uint64_t out_cap)
{
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t i = (uint64_t)blockIdx.x * 4u + wave;
    if (i >= n) return;
    const uint64_t r = rows[i].number - record_base;
    const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
    const uint32_t nl = (uint32_t)(hi - lo);
    const ZaOvlRow t = row[r];
    ZaOvlPair p;
    uint32_t dl, nqa = 0, nqy = 0;
    p.sa = za_trim_body(scratch, start, lo, nl, P.seq_line, P.delim, &p.n1, &dl);
    p.sy = za_trim_body(scratch, start, lo, nl, P.m_lines + P.seq_line, P.delim, &p.n2, &dl);
    p.qa = P.qual_line >= 0 ? za_trim_body(scratch, start, lo, nl, (uint32_t)P.qual_line, P.delim, &nqa, &dl) : 0ull;
    p.qy = P.qual_line >= 0 ? za_trim_body(scratch, start, lo, nl, P.m_lines + (uint32_t)P.qual_line, P.delim, &nqy, &dl) : 0ull;
    p.o = t.offset; p.found = t.verdict == ZA_OVL_FOUND || t.verdict == ZA_OVL_MERGED;
    const bool merged = t.verdict == ZA_OVL_MERGED;
    uint64_t at = start[lo], d = offs[i];
    const uint64_t end = merged ? start[lo + P.m_lines] : start[hi];
    if (end < at || d > out_cap || out_cap - d < rows[i].len) return;
    const uint64_t lim = d + rows[i].len;                                          // (the row's bytes end here: nothing is written behind them)
    if (P.qual_line >= 0 && (nqa != p.n1 || nqy != p.n2)) return;                  // (za_k_ovl_close reported the fault: nothing is gathered)
    if (p.found && (p.o <= -(int32_t)p.n2 || p.o >= (int32_t)p.n1 || t.insert != (uint32_t)(p.o + (int32_t)p.n2))) return;
    const bool cut = p.found && (P.flags & ZA_OVL_CUT);
    const uint32_t e1 = merged ? t.insert : cut && t.insert < p.n1 ? t.insert : p.n1;
    const uint32_t e2 = cut && p.o < 0 ? (uint32_t)((int32_t)p.n2 + p.o) : p.n2;
    // the changed lines in the order they lie in the record: the two of mate 1, then (not merged) the two of mate 2
    const uint32_t c0 = P.qual_line >= 0 && (uint32_t)P.qual_line < P.seq_line ? (uint32_t)P.qual_line : P.seq_line;
    const uint32_t c1 = P.qual_line >= 0 ? ((uint32_t)P.qual_line < P.seq_line ? P.seq_line : (uint32_t)P.qual_line) : P.k_lines;
    const uint32_t last = merged ? P.m_lines : nl;
    #pragma unroll 1
    for (uint32_t x = 0; x < 4u; x++) {
        const uint32_t c = (x & 1u) ? c1 : c0, mate2 = x >> 1, line = mate2 ? P.m_lines + c : c;
        if (c >= P.m_lines || line >= last) continue;                              // (no quality line; a line the short last record lacks; mate 2 of a merged pair)
        uint32_t nb, hd;
        const uint64_t ls = za_trim_body(scratch, start, lo, nl, line, P.delim, &nb, &hd);
        for (uint64_t j = lane; j < ls - at && d + j < lim; j += 64u) out[d + j] = scratch[at + j];
        d += ls - at;
        const bool qual = P.qual_line >= 0 && c == (uint32_t)P.qual_line;
        const uint32_t e = mate2 ? e2 : e1;
        for (uint32_t j = lane; j < e && d + j < lim; j += 64u)
            out[d + j] = merged ? za_ovl_merged_byte(scratch, p, P, j, qual) : mate2 ? za_ovl_mate2_byte(scratch, p, P, j, qual) : za_ovl_mate1_byte(scratch, p, P, j, qual);
        d += e;
        at = ls + nb;
    }
    for (uint64_t j = lane; j < end - at && d + j < lim; j += 64u) out[d + j] = scratch[at + j];
}

// BGZF: reads screened against reference k-mers -- a set of the k-mers of up to 64 references on the device, and
// for every record of a window how many of its k-mers lie in the set and in which references: what bbduk ref= k=, fastq_screen and rRNA
// depletion need.  The prologue of the screen pass is that of za_dedup.hip: the lines pass of za_grep.hip has run for the delimiters
// alone, the host has read how many lines the text holds, and za_k_grep_rec_lines of za_grep_records.hip has written where every line starts.
//   za_k_kmer_clear    one thread per slot: the code all ones, the mask 0
//   za_k_kmer_insert   one WAVE per strip of 64 positions of a reference, a lane per position: the k-mer's code out of three ballots,
//                      its slot claimed with one atomicCAS, the reference's bit set with one atomicOr when it is not set yet
//   za_k_kmer_load     one thread per (code, mask) pair: the same claim, the pair's mask ORed in
//   za_k_kmer_export   one thread per slot: the occupied slots compacted, one ballot and one atomicAdd on a cursor per wave
//   za_k_screen        one WAVE per record, its seq_line in strips of 64 positions: codes as in the insert, a plain load per probe, the
//                      counts per reference in the lane that owns the reference.  No LDS, no scratch, no atomics but the totals'.
// The close kernel of the screen pass is za_k_rec_close<ZaScreenTotals> of za_grep_records.hip.
// Included by zng_amd.hip behind za_sort.hip (za_trim_body reads a line's body, za_key_mix finds a code's home).
#include "za_common.h"

#define ZA_KMER_CANONICAL 1u                           // mirror ZNGAMD_KMER_CANONICAL
#define ZA_KMER_NONE      0xFFFFFFFFu                  // mirror ZNGAMD_KMER_NONE
#define ZA_KMER_EMPTY     (~0ull)                      // every code is below 4^31 = 2^62
#define ZA_KMER_MIN_CAP   64ull
#define ZA_SCREEN_WG_PER_CU 8u                         // workgroups of za_k_screen per CU: no LDS, so the waves alone bound it

struct alignas(16) ZaKmerSlot { unsigned long long code, mask; };                               // 16 B: a slot of the table, read with one load
struct ZaScreenRow { uint64_t refs; uint32_t kmers, hits, best, best_hits; };                   // mirrors zngamd_bgzf_screen_row
struct ZaScreenTotals { uint64_t seen, bytes_in, bases, tail_off, bad_record, bad_src; uint32_t covered, short_lines, bad, reserved;
                        uint64_t kmers, hits, matched; };                                       // zngamd_bgzf_screen_totals
struct ZaScreenPar { uint32_t k_lines, seq_line; int32_t first_byte; uint32_t min_hits, delim, k, canonical; };

// A, C, G, T in either case are 0, 1, 2, 3; U and u count as T; 4: every other byte
__device__ __forceinline__ uint32_t za_kmer_base(uint32_t b)
{
    const uint32_t c = b | 0x20u;
    return c == 'a' ? 0u : c == 'c' ? 1u : c == 'g' ? 2u : (c == 't' || c == 'u') ? 3u : 4u;
}

// bit i of the low word to bit 2 i
__device__ __forceinline__ uint64_t za_kmer_spread(uint32_t v)
{
    uint64_t x = v;
    x = (x | x << 16) & 0x0000FFFF0000FFFFull;
    x = (x | x << 8) & 0x00FF00FF00FF00FFull;
    x = (x | x << 4) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | x << 2) & 0x3333333333333333ull;
    return (x | x << 1) & 0x5555555555555555ull;
}

// The planes of a strip: bit l of (*p0, *p1) is the low and the high bit of the base that lane l holds, bit l of *px says that the lane
// holds none (an invalid byte, or no byte at all).
__device__ __forceinline__ void za_kmer_planes(uint32_t base, uint64_t *p0, uint64_t *p1, uint64_t *px)
{
    *p0 = __ballot(base & 1u); *p1 = __ballot(base & 2u); *px = __ballot(base & 4u);
}

// the k bits from bit `lane` on of the 128-bit plane (next : cur), 1 <= k <= 31
__device__ __forceinline__ uint32_t za_kmer_cut(uint64_t cur, uint64_t next, uint32_t lane, uint32_t km)
{
    const uint64_t w = lane ? (cur >> lane | next << (64u - lane)) : cur;
    return (uint32_t)w & km;
}

// The code of the k-mer whose bases have the low bits w0 and the high bits w1 (bit i: base i, the first base of the k-mer is base 0).
// Forward: base i goes to the bits 2 (k - 1 - i), so the planes are reversed and spread.  Reverse complement: its base k - 1 - i is
// 3 - base i, which lands on the bits 2 i: the complemented planes spread as they are.
__device__ __forceinline__ uint64_t za_kmer_code(uint32_t w0, uint32_t w1, uint32_t k, uint32_t km, bool canonical)
{
    const uint64_t f = za_kmer_spread(__brev(w0) >> (32u - k)) | za_kmer_spread(__brev(w1) >> (32u - k)) << 1;
    if (!canonical) return f;
    const uint64_t r = za_kmer_spread(~w0 & km) | za_kmer_spread(~w1 & km) << 1;
    return r < f ? r : f;
}

// ---- the table.  cap (a power of two, >= 2 x the codes that are ever inserted, >= 64) slots of 16 bytes: the code, all ones for an empty
// slot, and the mask of the references that hold it.  A code's home is za_key_mix(code) & (cap - 1), probing is linear with wrap.  A slot,
// once claimed, keeps its code for good; its mask only gains bits.
// No loop here waits for another thread: a probe loop moves on one slot per turn, leaves at the first slot that is empty or holds its own
// code, and ends because at most cap / 2 slots are ever claimed, so an empty slot (or the code's own) lies ahead of every home.

// the slot of `code`, claimed when it was in no slot; *claimed says whether this call claimed it
__device__ __forceinline__ uint64_t za_kmer_claim(ZaKmerSlot *__restrict__ tab, uint64_t mask, uint64_t code, bool *claimed)
{
    uint64_t s = za_key_mix(code) & mask;
    *claimed = false;
    for (;;) {
        unsigned long long v = __hip_atomic_load(&tab[s].code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a stale value is empty, and the CAS tells)
        if (v == ZA_KMER_EMPTY) {
            v = atomicCAS(&tab[s].code, ZA_KMER_EMPTY, (unsigned long long)code);
            if (v == ZA_KMER_EMPTY) { *claimed = true; return s; }
        }
        if (v == code) return s;
        s = (s + 1u) & mask;
    }
}

// the reference bits `bits` into the mask of slot s: an atomic only when one of them is not set yet (a stale value lacks bits at most)
__device__ __forceinline__ void za_kmer_mark(ZaKmerSlot *__restrict__ tab, uint64_t s, uint64_t bits)
{
    const unsigned long long m = __hip_atomic_load(&tab[s].mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (~m & bits) atomicOr(&tab[s].mask, (unsigned long long)bits);
}

// grid: one thread per slot
__global__ __launch_bounds__(256) void za_k_kmer_clear(ZaKmerSlot *__restrict__ tab, uint64_t cap)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < cap) { ZaKmerSlot z; z.code = ZA_KMER_EMPTY; z.mask = 0; tab[s] = z; }
}

// grid: (any number of workgroups of four waves, n_refs).  Reference j = blockIdx.y is seqs[off[j] .. off[j + 1]), n bytes, with the
// positions 0 .. n - k; wave w of workgroup g takes its strips 4 g + w, 4 (g + gridDim.x) + w, ...  Lane l of strip p0 holds position
// p0 + l; it reads the bytes p0 + l and p0 + 64 + l when they are below n, and its k-mer is cut from the planes only when p0 + l <= n - k.
// acc (zeroed): [0] the valid positions, [1] the slots claimed.
__global__ __launch_bounds__(256) void za_k_kmer_insert(const uint8_t *__restrict__ seqs, const unsigned long long *__restrict__ off, uint32_t k, uint32_t canonical,
                                                        ZaKmerSlot *__restrict__ tab, uint64_t mask, unsigned long long *__restrict__ acc)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t j = blockIdx.y, km = (1u << k) - 1u;
    const uint64_t a = off[j], n = off[j + 1u] - a;
    if (n < k) return;
    const uint64_t npos = n - k + 1u, stride = (uint64_t)gridDim.x * 4u * 64u;
    const uint8_t *__restrict__ seq = seqs + a;
    uint64_t valid = 0, claims = 0;
    #pragma unroll 1
    for (uint64_t p0 = ((uint64_t)blockIdx.x * 4u + wave) * 64u; p0 < npos; p0 += stride) {
        const uint64_t p = p0 + lane;
        uint64_t c0, c1, cx, n0, n1, nx;
        za_kmer_planes(p < n ? za_kmer_base(seq[p]) : 4u, &c0, &c1, &cx);
        za_kmer_planes(p + 64u < n ? za_kmer_base(seq[p + 64u]) : 4u, &n0, &n1, &nx);
        const bool ok = p < npos && !za_kmer_cut(cx, nx, lane, km);
        bool claimed = false;
        if (ok) {
            const uint64_t code = za_kmer_code(za_kmer_cut(c0, n0, lane, km), za_kmer_cut(c1, n1, lane, km), k, km, canonical != 0);
            const uint64_t s = za_kmer_claim(tab, mask, code, &claimed);
            za_kmer_mark(tab, s, 1ull << j);
        }
        valid += (uint64_t)__popcll(__ballot(ok)); claims += (uint64_t)__popcll(__ballot(claimed));
    }
    if (lane == 0) {
        if (valid) atomicAdd(&acc[0], (unsigned long long)valid);
        if (claims) atomicAdd(&acc[1], (unsigned long long)claims);
    }
}

// grid: one thread per pair (judged by the host: code < 4^k, mask not 0 and below 2^n_refs).  acc (zeroed): [1] the slots claimed.
__global__ __launch_bounds__(256) void za_k_kmer_load(const unsigned long long *__restrict__ codes, const unsigned long long *__restrict__ masks, uint64_t n,
                                                      ZaKmerSlot *__restrict__ tab, uint64_t mask, unsigned long long *__restrict__ acc)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false;
    if (i < n) {
        const uint64_t s = za_kmer_claim(tab, mask, codes[i], &claimed);
        za_kmer_mark(tab, s, masks[i]);
    }
    const uint32_t claims = (uint32_t)__popcll(__ballot(claimed));
    if ((threadIdx.x & 63u) == 0 && claims) atomicAdd(&acc[1], (unsigned long long)claims);
}

// grid: one thread per slot, in a launch behind the inserts.  cursor (zeroed): the pairs written; a wave takes its room with one
// atomicAdd.  A pair whose place is at or beyond out_cap is not written (the host gives room for every claimed slot).
__global__ __launch_bounds__(256) void za_k_kmer_export(const ZaKmerSlot *__restrict__ tab, uint64_t cap, unsigned long long *__restrict__ codes,
                                                        unsigned long long *__restrict__ masks, uint64_t out_cap, unsigned long long *__restrict__ cursor)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    ZaKmerSlot v; v.code = ZA_KMER_EMPTY; v.mask = 0;
    if (s < cap) v = tab[s];
    const uint64_t full = __ballot(v.code != ZA_KMER_EMPTY);
    if (!full) return;                                                              // (uniform for the wave)
    const uint32_t lead = (uint32_t)__builtin_ctzll(full);
    unsigned long long base = 0;
    if (lane == lead) base = atomicAdd(cursor, (unsigned long long)__popcll(full));
    const uint32_t b_lo = (uint32_t)__shfl((int)(uint32_t)base, (int)lead, 64), b_hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)lead, 64);
    const uint64_t at = ((uint64_t)b_hi << 32 | b_lo) + (uint64_t)__popcll(full & ((1ull << lane) - 1ull));
    if (v.code != ZA_KMER_EMPTY && at < out_cap) { codes[at] = v.code; masks[at] = v.mask; }
}

__device__ __forceinline__ uint64_t za_wave_or_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}

// grid: any number of workgroups of four waves; wave w of workgroup g takes the records 4 g + w, 4 (g + gridDim.x) + w, ...  start, lines:
// as za_rec_extent takes them.  row: a row per record, or no pointer.  tab: the set's table, written by earlier launches and only read
// here: a probe is a plain 16-byte load, and its loop ends at the code or at an empty slot, of which at least cap / 2 exist.  tot
// (zeroed): bytes_in, bases, kmers, hits and matched are summed here; bad (~0 beforehand): the smallest r whose first byte is not
// first_byte.  The body has n bytes and the positions 0 .. n - k: lane l of strip p0 reads body[p0 + 64 + l] only when that is below n
// (the strip's own bytes came with the strip before), and cuts a k-mer from the planes only when p0 + l <= n - k, so the k-mer covers
// body[p0 + l .. p0 + l + k - 1] and every byte read lies in the body.  A strip costs the same wherever it lies: the planes carry over,
// nothing else does.  Lane j owns the count of reference j.  No barrier, no LDS.
__global__ __launch_bounds__(256) void za_k_screen(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start, uint64_t lines,
                                                   uint64_t nrec, ZaScreenPar P, const ZaKmerSlot *__restrict__ tab, uint64_t mask, ZaScreenRow *__restrict__ row,
                                                   ZaScreenTotals *__restrict__ tot, unsigned long long *__restrict__ bad)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t k = P.k, km = (1u << k) - 1u;
    const bool canon = P.canonical != 0;
    const uint64_t stride = (uint64_t)gridDim.x * 4u;
    uint64_t bytes_in = 0, bases = 0, t_kmers = 0, t_hits = 0, t_matched = 0;
    #pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + wave; r < nrec; r += stride) {
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint64_t ra = start[lo], re = start[hi];
        if (lane == 0 && P.first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)P.first_byte)) atomicMin(&bad[0], (unsigned long long)r);
        uint32_t n, sd;
        const uint64_t ss = za_trim_body(scratch, start, lo, (uint32_t)(hi - lo), P.seq_line, P.delim, &n, &sd);
        const uint32_t npos = n >= k ? n - k + 1u : 0u;
        uint32_t kmers = 0, hits = 0, cnt = 0;                                     // cnt: this lane's reference
        uint64_t refs = 0, c0 = 0, c1 = 0, cx = 0;
        if (npos) za_kmer_planes(lane < n ? za_kmer_base(scratch[ss + lane]) : 4u, &c0, &c1, &cx);
        #pragma unroll 1
        for (uint64_t p0 = 0; p0 < npos; p0 += 64u) {                               // (64 bits: a body may end just below 2^32)
            uint64_t n0, n1, nx;
            const uint64_t q = p0 + 64u + lane;
            za_kmer_planes(q < n ? za_kmer_base(scratch[ss + q]) : 4u, &n0, &n1, &nx);
            const bool ok = lane < npos - p0 && !za_kmer_cut(cx, nx, lane, km);
            uint64_t m = 0;
            if (ok) {
                const uint64_t code = za_kmer_code(za_kmer_cut(c0, n0, lane, km), za_kmer_cut(c1, n1, lane, km), k, km, canon);
                uint64_t s = za_key_mix(code) & mask;
                for (;;) {
                    const ZaKmerSlot v = tab[s];
                    if (v.code == code) { m = v.mask; break; }
                    if (v.code == ZA_KMER_EMPTY) break;
                    s = (s + 1u) & mask;
                }
            }
            kmers += (uint32_t)__popcll(__ballot(ok));
            const uint64_t hit = __ballot(m != 0);
            if (hit) {                                                              // (uniform for the wave; most strips of most files stop here)
                hits += (uint32_t)__popcll(hit);
                const uint64_t any = za_wave_or_u64(m);
                uint64_t left = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)any) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(any >> 32)) << 32;
                refs |= left;
                while (left) {                                                      // one ballot and one popcount per reference that was hit
                    const uint32_t j = (uint32_t)__builtin_ctzll(left);
                    const uint32_t c = (uint32_t)__popcll(__ballot((m >> j & 1ull) != 0));
                    if (lane == j) cnt += c;
                    left &= left - 1ull;
                }
            }
            c0 = n0; c1 = n1; cx = nx;
        }
        // the largest count, the lowest reference among equals: one wave maximum over count << 6 | (63 - lane)
        unsigned long long top = (unsigned long long)cnt << 6 | (63u - lane);
        #pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(top, d, 64); top = o > top ? o : top; }
        bytes_in += re > ra ? re - ra : 0ull; bases += n; t_kmers += kmers; t_hits += hits; t_matched += hits >= P.min_hits ? 1u : 0u;
        if (lane == 0 && row) {
            ZaScreenRow w; w.refs = refs; w.kmers = kmers; w.hits = hits;
            w.best = hits ? 63u - (uint32_t)(top & 63u) : ZA_KMER_NONE; w.best_hits = hits ? (uint32_t)(top >> 6) : 0u;
            row[r] = w;
        }
    }
    if (lane == 0) {
        if (bytes_in) atomicAdd((unsigned long long *)&tot->bytes_in, (unsigned long long)bytes_in);
        if (bases) atomicAdd((unsigned long long *)&tot->bases, (unsigned long long)bases);
        if (t_kmers) atomicAdd((unsigned long long *)&tot->kmers, (unsigned long long)t_kmers);
        if (t_hits) atomicAdd((unsigned long long *)&tot->hits, (unsigned long long)t_hits);
        if (t_matched) atomicAdd((unsigned long long *)&tot->matched, (unsigned long long)t_matched);
    }
}

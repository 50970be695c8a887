// BGZF: duplicate records -- a 16-byte key per record, and for any number of such keys the first record that
// carries each key and how many carry it: what fastp --dedup, seqkit rmdup -s and FastQC's duplication levels need.  The prologue of
// the key pass is that of za_trim.hip and za_qc.hip: the lines pass of za_grep.hip has run for the delimiters alone, the host has read
// how many lines the text holds, and za_k_grep_rec_lines of za_grep_records.hip has written where every line starts.  What is new:
//   za_k_dedup_keys    one WAVE per record, the keyed part of its seq_line in strips of 64 bytes: every lane mixes its (position, byte)
//                      into two 64-bit words and adds them up over the strips; one wave sum per word ends the record.  The key is a sum,
//                      so strips carry nothing from one to the next.  No LDS, no scratch.
//   za_k_dedup_insert  one thread per key: the key's slot in an open-addressed table of record numbers, claimed or lowered; the
//                      slot's counter
//   za_k_dedup_lookup  one thread per key: the slot again, first[] and count[], the totals
//   za_k_dedup_close   one thread: the totals as the caller reads them
// The close kernel of the key pass is za_k_rec_close<ZaKeyTotals> of za_grep_records.hip.
// Included by zng_amd.hip behind za_qc.hip (za_trim_body reads a line's body here too).
#include "za_common.h"

#define ZA_KEY_IGNORE_CASE 1u                          // mirror ZNGAMD_BGZF_KEY_*
#define ZA_KEY_CANONICAL   2u
#define ZA_KEY_SEED0 0x243F6A8885A308D3ull             // mirror ZNGAMD_BGZF_KEY_SEED0 / 1
#define ZA_KEY_SEED1 0x13198A2E03707344ull
#define ZA_KEY_WG_PER_CU 8u                            // workgroups of za_k_dedup_keys per CU: no LDS, so the waves alone bound it
#define ZA_DEDUP_EMPTY   (~0ull)
#define ZA_DEDUP_MIN_CAP 64ull

struct ZaKeyRow { uint64_t lo, hi; };                                                        // mirrors zngamd_bgzf_key_row
struct ZaKeyTotals { uint64_t seen, bytes_in, bases, tail_off, bad_record, bad_src; uint32_t covered, short_lines, bad, reserved; };      // zngamd_bgzf_key_totals
struct ZaKeyPar { uint32_t k_lines, seq_line; int32_t first_byte; uint32_t first, length, flags, delim; };
struct ZaDedupTotals { uint64_t n, unique, duplicates, max_count, max_first, reserved; };    // mirrors zngamd_dedup_totals

// the splitmix64 step
__device__ __forceinline__ uint64_t za_key_mix(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// A<->T, C<->G in either case, U -> A, u -> a; every other byte is its own complement
__device__ __forceinline__ uint32_t za_key_comp(uint32_t b)
{
    const uint32_t u = b & 0xDFu, low = b & 0x20u;
    if ((b | 0x20u) < 'a' || (b | 0x20u) > 'z') return b;
    return u == 'A' ? ('T' | low) : (u == 'T' || u == 'U') ? ('A' | low) : u == 'C' ? ('G' | low) : u == 'G' ? ('C' | low) : b;
}

__device__ __forceinline__ uint64_t za_wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}

// grid: any number of workgroups of four waves; wave w of workgroup g takes the records 4 g + w, 4 (g + gridDim.x) + w, ...  start, lines:
// as za_rec_extent takes them.  row: a row per record, or no pointer.  tot (zeroed): bytes_in and bases are summed here; the word behind
// it (~0 beforehand): the smallest r whose first byte is not first_byte.  Every byte read lies in the body of a line of the text: lane
// l of strip p0 reads body[off + p0 + l] only when p0 + l < n, and off + n is at most the body's length.  No barrier, no LDS.
__global__ __launch_bounds__(256) void za_k_dedup_keys(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start, uint64_t lines,
                                                       uint64_t nrec, ZaKeyPar P, ZaKeyRow *__restrict__ row, ZaKeyTotals *__restrict__ tot)
{
    unsigned long long *bad = (unsigned long long *)(tot + 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool fold = (P.flags & ZA_KEY_IGNORE_CASE) != 0, canon = (P.flags & ZA_KEY_CANONICAL) != 0;
    const uint64_t stride = (uint64_t)gridDim.x * 4u;
    uint64_t bytes_in = 0, bases = 0;
    #pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + wave; r < nrec; r += stride) {
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint64_t ra = start[lo], re = start[hi];
        if (lane == 0 && P.first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)P.first_byte)) atomicMin(&bad[0], (unsigned long long)r);
        uint32_t nb, sd;
        const uint64_t ss = za_trim_body(scratch, start, lo, (uint32_t)(hi - lo), P.seq_line, P.delim, &nb, &sd);
        const uint32_t off = P.first < nb ? P.first : nb;
        uint32_t n = nb - off;
        if (P.length && n > P.length) n = P.length;
        uint64_t f0 = 0, f1 = 0, b0 = 0, b1 = 0;                                   // this lane's terms: forward, reverse complement
        #pragma unroll 1
        for (uint64_t p0 = 0; p0 < n; p0 += 64u) {
            if (lane < n - p0) {
                const uint64_t i = p0 + lane;
                uint32_t c = scratch[ss + off + i];
                if (fold && c >= 'a' && c <= 'z') c -= 0x20u;
                const uint64_t t = i << 8 | c;
                f0 += za_key_mix(ZA_KEY_SEED0 ^ t); f1 += za_key_mix(ZA_KEY_SEED1 ^ t);
                if (canon) {
                    const uint64_t u = ((uint64_t)n - 1u - i) << 8 | za_key_comp(c);
                    b0 += za_key_mix(ZA_KEY_SEED0 ^ u); b1 += za_key_mix(ZA_KEY_SEED1 ^ u);
                }
            }
        }
        const uint64_t l0 = za_key_mix(ZA_KEY_SEED0 ^ (1ull << 63 | n)), l1 = za_key_mix(ZA_KEY_SEED1 ^ (1ull << 63 | n));
        uint64_t klo = l0 + za_wave_sum_u64(f0), khi = l1 + za_wave_sum_u64(f1);
        if (canon) {
            const uint64_t rlo = l0 + za_wave_sum_u64(b0), rhi = l1 + za_wave_sum_u64(b1);
            if (rhi < khi || (rhi == khi && rlo < klo)) { klo = rlo; khi = rhi; }
        }
        bytes_in += re > ra ? re - ra : 0ull; bases += nb;
        if (lane == 0 && row) { ZaKeyRow w; w.lo = klo; w.hi = khi; row[r] = w; }
    }
    if (lane == 0) {
        if (bytes_in) atomicAdd((unsigned long long *)&tot->bytes_in, (unsigned long long)bytes_in);
        if (bases) atomicAdd((unsigned long long *)&tot->bases, (unsigned long long)bases);
    }
}

// ---- the table.  cap (a power of two, >= 2 n, >= 64) slots of 64 bits, all ones for an empty one, otherwise the number of a record;
// cap 32-bit counters beside them.  The key of slot s is key[slot[s]]: key[] does not change during the call, and a slot, once claimed,
// only ever moves to a lower record number of the SAME key, so a slot's key never changes.  A key's home is lo & (cap - 1), probing is
// linear with wrap.
// No loop here waits for another thread: a probe loop moves on one slot per turn, leaves at the first slot that is empty or holds its own
// key, and ends because at most n <= cap / 2 slots are ever claimed, so an empty slot (or the key's own) lies ahead of every home.

// the slot of key (lo, hi) for record r, claimed or lowered to r when `insert`; without it the key is in the table already
template <bool insert>
__device__ __forceinline__ uint64_t za_dedup_probe(const ZaKeyRow *__restrict__ key, unsigned long long *__restrict__ slot, uint64_t mask, uint64_t r, uint64_t lo, uint64_t hi)
{
    uint64_t s = lo & mask;
    for (;;) {
        unsigned long long v = __hip_atomic_load(&slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a stale value is a former one: still this slot's key, or empty and the CAS tells)
        if (insert && v == ZA_DEDUP_EMPTY) {
            v = atomicCAS(&slot[s], ZA_DEDUP_EMPTY, (unsigned long long)r);
            if (v == ZA_DEDUP_EMPTY) return s;                                      // claimed
        }
        if (!insert && v == ZA_DEDUP_EMPTY) return s;                               // (cannot happen behind an insert of the same keys; ends the loop)
        const ZaKeyRow q = key[v];
        if (q.lo == lo && q.hi == hi) {
            // the slot is this key's for good; only a record below the value just read has anything to say, so in a file with
            // one hot sequence almost no duplicate issues an atomic on its line
            if (insert && r < v) atomicMin(&slot[s], (unsigned long long)r);
            return s;
        }
        s = (s + 1u) & mask;
    }
}

// grid: one thread per key.  slot: all ones; cnt: zeroed.  The lanes of a wave that reached the same slot add to its counter once: a
// loop over the wave's distinct slots, the first lane of each group adds the group's size.
__global__ __launch_bounds__(256) void za_k_dedup_insert(const ZaKeyRow *__restrict__ key, uint64_t n, unsigned long long *__restrict__ slot, uint32_t *__restrict__ cnt,
                                                         uint64_t mask)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = r < n;
    uint64_t s = 0;
    if (in) { const ZaKeyRow k = key[r]; s = za_dedup_probe<true>(key, slot, mask, r, k.lo, k.hi); }
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t left = __ballot(in);
    while (left) {                                                                  // (uniform for the wave: `left` is a ballot)
        const uint32_t lead = (uint32_t)__builtin_ctzll(left);
        const uint32_t s_lo = (uint32_t)__shfl((int)(uint32_t)s, (int)lead, 64), s_hi = (uint32_t)__shfl((int)(uint32_t)(s >> 32), (int)lead, 64);
        const uint64_t group = __ballot(in && s == ((uint64_t)s_hi << 32 | s_lo)) & left;
        if (lane == lead) atomicAdd(&cnt[s], (uint32_t)__popcll(group));            // (n <= 2^30: a counter cannot wrap)
        left &= ~group;
    }
}

// grid: one thread per key, behind za_k_dedup_insert.  first, count: arrays of n, or no pointer.  acc (zeroed): [0] the keys that are their
// group's first, [1] the largest group and its first record as count << 32 | (2^32 - 1 - first), so that the maximum takes the lowest
// record among the largest groups (first < n <= 2^30).
__global__ __launch_bounds__(256) void za_k_dedup_lookup(const ZaKeyRow *__restrict__ key, uint64_t n, unsigned long long *__restrict__ slot, const uint32_t *__restrict__ cnt,
                                                         uint64_t mask, unsigned long long *__restrict__ first, uint32_t *__restrict__ count, unsigned long long *__restrict__ acc)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = r < n;
    bool head = false;
    unsigned long long best = 0;
    if (in) {
        const ZaKeyRow k = key[r];
        const uint64_t s = za_dedup_probe<false>(key, slot, mask, r, k.lo, k.hi);
        const unsigned long long f = slot[s];
        head = f == r;
        const uint32_t c = head ? cnt[s] : 0u;
        if (first) first[r] = f;
        if (count) count[r] = c;
        if (head) best = (unsigned long long)c << 32 | (0xFFFFFFFFull - r);
    }
    const uint32_t heads = (uint32_t)__popcll(__ballot(head));
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(best, d, 64); best = o > best ? o : best; }
    if ((threadIdx.x & 63u) == 0 && heads) { atomicAdd(&acc[0], (unsigned long long)heads); atomicMax(&acc[1], best); }
}

// one thread.  n > 0.
__global__ void za_k_dedup_close(const unsigned long long *__restrict__ acc, uint64_t n, ZaDedupTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    ZaDedupTotals z = {};
    z.n = n; z.unique = acc[0]; z.duplicates = n - acc[0]; z.max_count = acc[1] >> 32; z.max_first = 0xFFFFFFFFull - (acc[1] & 0xFFFFFFFFull);
    *tot = z;
}

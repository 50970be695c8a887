// BGZF: the k-mers of a file's reads counted -- a table of (code, count) pairs on the device that any number of
// windows, files and shards add to, its spectrum and its pairs: what jellyfish count + histo, KMC and FastQC's "Kmer Content" give.  The
// codes, the bit planes, the cut and the claim are those of za_screen.hip; the prologue of the reads pass is that of the screen pass.
//   za_k_kcount_clear   one thread per slot: the code all ones, the count 0
//   za_k_kcount_reads   one WAVE per record, its seq_line in strips of 64 positions: the codes as in the screen; equal codes in adjacent
//                       lanes are one run, and only the head of a run claims the slot and issues one atomicAdd of the run's length
//   za_k_kcount_pairs   one thread per (code, count) pair, given as two arrays or as the slots of an older table: claim and add
//   za_k_kcount_export  one thread per slot: the slots whose count lies in [min_count, max_count] compacted
//   za_k_kcount_hist    grid-stride over slots: a histogram of the counts per workgroup in LDS, flushed with 64-bit atomics
// The close kernel of the reads pass is za_k_rec_close<ZaKcountTotals> of za_grep_records.hip.
// Included by zng_amd.hip behind za_screen.hip.  A slot is a ZaKmerSlot whose second word is the count, so that za_kmer_claim serves as it is.
#include "za_common.h"

#define ZA_KCOUNT_WG_PER_CU    8u                      // workgroups of za_k_kcount_reads per CU: no LDS, so the waves alone bound it
#define ZA_KCOUNT_HIST_PER_CU  4u                      // workgroups of za_k_kcount_hist per CU: the flush is bins x this x CUs atomics at most
#define ZA_KCOUNT_HIST_PASS    (1u << 20)              // turns of a histogram workgroup between two flushes: 2^28 slots, so no LDS bin passes 2^32
#define ZA_KCOUNT_MAX_BINS     16384u                  // mirror ZNGAMD_KMER_HIST_MAX_BINS: 64 KiB of LDS

struct ZaKcountTotals { uint64_t seen, bytes_in, bases, tail_off, bad_record, bad_src; uint32_t covered, short_lines, bad, reserved;
                        uint64_t kmers, claimed, adds; };                               // zngamd_bgzf_count_totals
struct ZaKcountPar { uint32_t k_lines, seq_line; int32_t first_byte; uint32_t delim, k, canonical; };

// grid: one thread per slot
__global__ __launch_bounds__(256) void za_k_kcount_clear(ZaKmerSlot *__restrict__ tab, uint64_t cap)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < cap) { ZaKmerSlot z; z.code = ZA_KMER_EMPTY; z.mask = 0; tab[s] = z; }
}

// grid: any number of workgroups of four waves; wave w of workgroup g takes the records 4 g + w, 4 (g + gridDim.x) + w, ...  start, lines:
// as za_rec_extent takes them.  tab: the counter's table, mask = cap - 1.  The host has seen to it that the slots claimed so far and the
// bytes of this window together are at most cap / 2, so the claim's loop ends (za_screen.hip).  The strips, the planes and the bounds of
// every read are those of za_k_screen: lane l of strip p0 reads body[p0 + 64 + l] only when that is below n and cuts a k-mer only when
// p0 + l <= n - k.  A lane is the HEAD of a run when its k-mer is valid and lane l - 1 (none for lane 0: strips start at position 0 of the
// record) is invalid or holds another code; the run goes on to the lane before the next head or the next invalid lane, whichever comes
// first.  Only heads touch the table.  tot (zeroed): bytes_in, bases, kmers, claimed and adds are summed here; bad (~0 beforehand): the
// smallest r whose first byte is not first_byte.  No barrier, no LDS.
__global__ __launch_bounds__(256) void za_k_kcount_reads(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start, uint64_t lines,
                                                         uint64_t nrec, ZaKcountPar P, ZaKmerSlot *__restrict__ tab, uint64_t mask, ZaKcountTotals *__restrict__ tot,
                                                         unsigned long long *__restrict__ bad)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t k = P.k, km = (1u << k) - 1u;
    const bool canon = P.canonical != 0;
    const uint64_t stride = (uint64_t)gridDim.x * 4u;
    const uint64_t above = lane == 63u ? 0ull : ~0ull << (lane + 1u);              // the lanes above this one
    uint64_t bytes_in = 0, bases = 0, t_kmers = 0, t_claimed = 0, t_adds = 0;
    #pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + wave; r < nrec; r += stride) {
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint64_t ra = start[lo], re = start[hi];
        if (lane == 0 && P.first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)P.first_byte)) atomicMin(&bad[0], (unsigned long long)r);
        uint32_t n, sd;
        const uint64_t ss = za_trim_body(scratch, start, lo, (uint32_t)(hi - lo), P.seq_line, P.delim, &n, &sd);
        const uint32_t npos = n >= k ? n - k + 1u : 0u;
        uint64_t c0 = 0, c1 = 0, cx = 0;
        if (npos) za_kmer_planes(lane < n ? za_kmer_base(scratch[ss + lane]) : 4u, &c0, &c1, &cx);
        #pragma unroll 1
        for (uint64_t p0 = 0; p0 < npos; p0 += 64u) {                               // (64 bits: a body may end just below 2^32)
            uint64_t n0, n1, nx;
            const uint64_t q = p0 + 64u + lane;
            za_kmer_planes(q < n ? za_kmer_base(scratch[ss + q]) : 4u, &n0, &n1, &nx);
            const bool ok = lane < npos - p0 && !za_kmer_cut(cx, nx, lane, km);
            const unsigned long long code = ok ? (unsigned long long)za_kmer_code(za_kmer_cut(c0, n0, lane, km), za_kmer_cut(c1, n1, lane, km), k, km, canon)
                                               : (unsigned long long)ZA_KMER_EMPTY;     // (no code is all ones: an invalid lane equals no valid one)
            const unsigned long long below = __shfl_up(code, 1u, 64);
            const bool head = ok && (lane == 0u || below != code);
            const uint64_t valid = __ballot(ok), heads = __ballot(head);
            bool claimed = false;
            if (head) {
                const uint64_t stop = (heads | ~valid) & above;                     // the next head or the next invalid lane
                const uint32_t run = (stop ? (uint32_t)__builtin_ctzll(stop) : 64u) - lane;
                const uint64_t s = za_kmer_claim(tab, mask, code, &claimed);
                atomicAdd(&tab[s].mask, (unsigned long long)run);
            }
            t_kmers += (uint64_t)__popcll(valid); t_adds += (uint64_t)__popcll(heads); t_claimed += (uint64_t)__popcll(__ballot(claimed));
            c0 = n0; c1 = n1; cx = nx;
        }
        bytes_in += re > ra ? re - ra : 0ull; bases += n;
    }
    if (lane == 0) {
        if (bytes_in) atomicAdd((unsigned long long *)&tot->bytes_in, (unsigned long long)bytes_in);
        if (bases) atomicAdd((unsigned long long *)&tot->bases, (unsigned long long)bases);
        if (t_kmers) atomicAdd((unsigned long long *)&tot->kmers, (unsigned long long)t_kmers);
        if (t_claimed) atomicAdd((unsigned long long *)&tot->claimed, (unsigned long long)t_claimed);
        if (t_adds) atomicAdd((unsigned long long *)&tot->adds, (unsigned long long)t_adds);
    }
}

// grid: one thread per pair.  Pair i is (codes[step i], counts[step i]): step 1 for two arrays that the host has judged (code < 4^k,
// count not 0), step 2 with codes and counts at the two words of an older table's slot 0 for a rehash, where a slot whose code is all
// ones is empty and skipped.  acc (zeroed): [0] the slots claimed.
__global__ __launch_bounds__(256) void za_k_kcount_pairs(const unsigned long long *__restrict__ codes, const unsigned long long *__restrict__ counts, uint64_t n,
                                                         uint32_t step, ZaKmerSlot *__restrict__ tab, uint64_t mask, unsigned long long *__restrict__ acc)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool claimed = false;
    if (i < n) {
        const unsigned long long code = codes[i * step];
        if (code != ZA_KMER_EMPTY) {
            const uint64_t s = za_kmer_claim(tab, mask, code, &claimed);
            atomicAdd(&tab[s].mask, counts[i * step]);
        }
    }
    const uint32_t claims = (uint32_t)__popcll(__ballot(claimed));
    if ((threadIdx.x & 63u) == 0 && claims) atomicAdd(&acc[0], (unsigned long long)claims);
}

// grid: one thread per slot, in a launch behind every add.  The slots with min_count <= count <= max_count (min_count >= 1, so no empty
// slot) compacted as za_k_kmer_export compacts: cursor (zeroed) counts every such slot, and a pair whose place is at or beyond out_cap
// is not written.
__global__ __launch_bounds__(256) void za_k_kcount_export(const ZaKmerSlot *__restrict__ tab, uint64_t cap, unsigned long long min_count, unsigned long long max_count,
                                                          unsigned long long *__restrict__ codes, unsigned long long *__restrict__ counts, uint64_t out_cap,
                                                          unsigned long long *__restrict__ cursor)
{
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    ZaKmerSlot v; v.code = ZA_KMER_EMPTY; v.mask = 0;
    if (s < cap) v = tab[s];
    const bool take = v.code != ZA_KMER_EMPTY && v.mask >= min_count && v.mask <= max_count;
    const uint64_t full = __ballot(take);
    if (!full) return;                                                              // (uniform for the wave)
    const uint32_t lead = (uint32_t)__builtin_ctzll(full);
    unsigned long long base = 0;
    if (lane == lead) base = atomicAdd(cursor, (unsigned long long)__popcll(full));
    const uint32_t b_lo = (uint32_t)__shfl((int)(uint32_t)base, (int)lead, 64), b_hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)lead, 64);
    const uint64_t at = ((uint64_t)b_hi << 32 | b_lo) + (uint64_t)__popcll(full & ((1ull << lane) - 1ull));
    if (take && at < out_cap) { codes[at] = v.code; counts[at] = v.mask; }
}

// grid: at most ZA_KCOUNT_HIST_PER_CU workgroups per CU, of 256 threads, with bins x 4 bytes of LDS (2 <= bins <= ZA_KCOUNT_MAX_BINS).
// Workgroup g takes the blocks of 256 slots g, g + gridDim.x, ...; an occupied slot adds 1 to the LDS bin min(count, bins - 1).  After
// at most ZA_KCOUNT_HIST_PASS blocks -- 2^28 slots, so no bin has passed 2^32 -- and at the end, the non-zero bins go to hist (zeroed)
// with one 64-bit atomic each.  The loops depend on the workgroup alone, so every thread meets every barrier.
__global__ __launch_bounds__(256) void za_k_kcount_hist(const ZaKmerSlot *__restrict__ tab, uint64_t cap, uint32_t bins, unsigned long long *__restrict__ hist)
{
    extern __shared__ uint32_t za_kcount_bins[];
    const uint32_t tid = threadIdx.x;
    const uint64_t nblk = (cap + 255u) / 256u;
    uint64_t b = blockIdx.x;
    while (b < nblk) {
        for (uint32_t i = tid; i < bins; i += 256u) za_kcount_bins[i] = 0;
        __syncthreads();
        #pragma unroll 1
        for (uint32_t turn = 0; turn < ZA_KCOUNT_HIST_PASS && b < nblk; turn++, b += gridDim.x) {
            const uint64_t s = b * 256u + tid;
            if (s < cap) {
                const ZaKmerSlot v = tab[s];
                if (v.code != ZA_KMER_EMPTY) atomicAdd(&za_kcount_bins[v.mask < bins - 1u ? (uint32_t)v.mask : bins - 1u], 1u);
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < bins; i += 256u) { const uint32_t c = za_kcount_bins[i]; if (c) atomicAdd(&hist[i], (unsigned long long)c); }
        __syncthreads();
    }
}

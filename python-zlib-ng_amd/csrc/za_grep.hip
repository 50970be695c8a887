// BGZF: lines by content.  The decoded blocks of a window lie in the scratch as one byte string; the text
// to search is scratch[text_off, text_end).  Lines cross blocks freely, so the work is cut into tiles of 16 KiB of the scratch
// (absolute: tile t is [t * 16 KiB, (t + 1) * 16 KiB)), not into blocks.
//   za_k_grep_cover   one thread per member row: do rows that decoded tile the text without a gap?  (a byte count and a flag)
//   za_k_grep_mark    one workgroup per tile: a bit per delimiter, a bit per position where a pattern starts, then per line that
//                     BEGINS AND ENDS in the tile its verdict; per tile a summary for the lines that cross its edges
//   za_k_grep_mark_approx   the same with "starts" meaning "stands there with at most k bytes substituted" (section 5f.2)
//   za_k_grep_scan    one workgroup: the scan over the tile summaries (delimiters in front, where the open line began, whether it
//                     has matched), the verdict of every tile's first line, rows in front of every tile, the totals
//   za_k_grep_emit    one workgroup per tile: the rows of the matching lines that end in it, in order
//   (za_grep_approx_stage / _compare: what za_k_grep_mark_approx and za_k_grep_classify of za_classify.hip share)
//   za_k_grep_place   rows and the offsets of za_k_offsets become the slices of za_k_slice_gather, which packs the lines
// Included by zng_amd.hip behind za_bgzf.hip (za_eq_mask, za_member_in_scratch, ZaBgzfSlice).
#include "za_common.h"

#define ZA_GREP_TILE        16384u       // bytes per tile: 256 threads x 64 bytes, a 64-bit word of delimiter / match bits per thread
#define ZA_GREP_MAX_PAT     64u
#define ZA_GREP_MAX_LEN     255u
#define ZA_GREP_INVERT      1u           // flags: mirror ZNGAMD_BGZF_GREP_*
#define ZA_GREP_LINE_START  2u
#define ZA_GREP_FINAL       4u
#define ZA_GREP_COUNT_ONLY  8u
#define ZA_GREP_HEAD        1u           // tile flags: a pattern starts at or before the tile's first delimiter (anywhere, if it has none)
#define ZA_GREP_TAIL        2u           //             a pattern starts behind the tile's last delimiter
#define ZA_GREP_PAIR_WORDS  2048u        // the prefilter: a bit per pair of bytes (first, second) that opens a pattern
#define ZA_GREP_SCAN_THREADS 512u
#define ZA_GREP_MAX_MISMATCH 16u         // za_k_grep_mark_approx: mismatches at most (mirrors ZNGAMD_BGZF_GREP_MAX_MISMATCH)
#define ZA_GREP_AP_WORDS    ((ZA_GREP_TILE + 256u) / 4u)      // what it stages: the tile and 256 bytes behind it, as dwords
#define ZA_GREP_AP_BITS     ((ZA_GREP_TILE + 256u) / 32u)     //                 and a bit per staged byte, as dwords

struct ZaGrepPat { uint32_t off, len; };                                   // mirrors zngamd_bgzf_pattern
struct ZaGrepRow { uint64_t src_off, number; uint32_t len, reserved; };    // mirrors zngamd_bgzf_grep_row (and lies like a ZaBgzfSlice)
struct ZaGrepTile { uint32_t ndelim, first, last, flags, rows, bytes; };   // first / last delimiter: offsets in the tile; rows / bytes: matching lines that begin and end in it
struct ZaGrepCarry { uint64_t open_start, lines, row_base; uint32_t first_emit, reserved; };   // what a tile needs from the tiles in front of it
struct ZaGrepTotals {                                                       // the first 40 bytes mirror zngamd_bgzf_grep_totals
    uint64_t seen, matched, bytes, tail_off;
    uint32_t covered, final_emit;      // final_emit: with FINAL, the unterminated last line matched: it is the last row
    uint64_t final_src, final_number;
};

__device__ __forceinline__ uint64_t za_mask_le(uint32_t b) { return b >= 63u ? ~0ull : (2ull << b) - 1ull; }      // bits 0 .. b
// the four 0x80 marks of za_eq_mask as four adjacent bits (the products' bits do not meet: no carry)
__device__ __forceinline__ uint32_t za_mask_nibble(uint32_t m) { return ((((m >> 7) & 0x01010101u) * 0x00204081u) >> 21) & 0xFu; }

// grid: one thread per member.  The text is covered when rows that lie in ascending order without overlap, that decoded and that lie
// inside the scratch hold text_end - text_off of its bytes between them.  cover[0] += bytes, cover[1] |= a row out of order.
__global__ __launch_bounds__(256) void za_k_grep_cover(const ZaMember *__restrict__ members, const int32_t *__restrict__ member_status, uint32_t n_members,
                                                       uint64_t scratch_cap, uint64_t text_off, uint64_t text_end, unsigned long long *__restrict__ cover)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long n = 0;
    uint32_t bad = 0;
    if (i < n_members) {
        const ZaMember m = members[i];
        if (i > 0) {
            const ZaMember p = members[i - 1u];
            if (m.out_off < p.out_off || m.out_off - p.out_off < p.out_len) bad = 1;
        }
        if (member_status[i] == ZA_I_OK && za_member_in_scratch(m, scratch_cap)) {
            const uint64_t lo = m.out_off > text_off ? m.out_off : text_off, e = m.out_off + m.out_len, hi = e < text_end ? e : text_end;
            if (hi > lo) n = hi - lo;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { n += __shfl_xor(n, d, 64); bad |= __shfl_xor(bad, d, 64); }
    if ((threadIdx.x & 63u) == 0) {
        if (n) atomicAdd(&cover[0], n);
        if (bad) atomicOr(&cover[1], 1ull);
    }
}

// does one of the patterns stand at scratch[p] (p < text_end)?  Nothing at or behind text_end is read.
__device__ __forceinline__ bool za_grep_verify(const uint8_t *__restrict__ scratch, uint64_t p, uint64_t text_end,
                                               const uint32_t *s_key, const uint32_t *s_off, const uint8_t *__restrict__ blob, uint32_t np)
{
    const uint64_t avail = text_end - p;
    const uint32_t pair = scratch[p] | (avail > 1u ? (uint32_t)scratch[p + 1u] << 8 : 0u);
    for (uint32_t q = 0; q < np; q++) {
        const uint32_t key = s_key[q], len = key & 0xFFu;            // len | first byte << 8 | second byte << 16
        if (len > avail) continue;
        if (len == 1u ? (key >> 8 & 0xFFu) != (pair & 0xFFu) : (key >> 8) != pair) continue;
        const uint8_t *pp = blob + s_off[q], *t = scratch + p;
        uint32_t j = len < 2u ? len : 2u;
        while (j < len && pp[j] == t[j]) j++;
        if (j == len) return true;
    }
    return false;
}

// What both mark kernels end with.  s_d / s_m: a bit per byte of the tile (a delimiter; a position where a pattern starts), complete
// behind a barrier; v.first = 0xFFFFFFFF and v.last = 0 were set in front of that barrier.  Every thread of the workgroup calls it
// (it holds barriers): bits[tile][thread] and the tile's summary are written.
struct ZaGrepVerdictLds {
    uint32_t first, last;
    uint32_t w[4], wl[4];          // per wave: 1 = has a delimiter, 2 = head, 4 = tail; its last delimiter
    uint32_t cnt[4][3];
};
__device__ __forceinline__ void za_grep_tile_verdicts(const uint32_t *s_d, const uint32_t *s_m, ZaGrepVerdictLds &v, uint32_t flags,
                                                      ulonglong2 *__restrict__ bits, ZaGrepTile *__restrict__ tiles)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // ---- per line: thread tid owns bytes [64 tid, 64 tid + 64) of the tile
    const uint64_t D = (uint64_t)s_d[2u * tid + 1u] << 32 | s_d[2u * tid], M = (uint64_t)s_m[2u * tid + 1u] << 32 | s_m[2u * tid];
    const bool hasd = D != 0;
    const uint32_t fb = hasd ? (uint32_t)__builtin_ctzll(D) : 0u, lb = hasd ? 63u - (uint32_t)__builtin_clzll(D) : 0u;
    const bool headm = hasd ? (M & za_mask_le(fb)) != 0 : M != 0;
    const bool tailm = hasd && lb < 63u && (M >> (lb + 1u)) != 0;
    const uint64_t Dm = __ballot(hasd), Hm = __ballot(headm), Tm = __ballot(tailm);
    const uint32_t mylast = tid * 64u + lb;
    const uint64_t below = (1ull << lane) - 1ull, pd = Dm & below;
    const uint32_t j = pd ? 63u - (uint32_t)__builtin_clzll(pd) : 0u;
    const uint32_t lane_prev = (uint32_t)__shfl((int)mylast, (int)j, 64);
    const uint32_t wave_last = (uint32_t)__shfl((int)mylast, Dm ? 63 - __builtin_clzll(Dm) : 0, 64);
    if (lane == 0) {
        uint32_t s = 0;
        if (Dm) {
            const uint32_t fl = (uint32_t)__builtin_ctzll(Dm), ll = 63u - (uint32_t)__builtin_clzll(Dm);
            s = 1u | ((Hm & za_mask_le(fl)) != 0 ? 2u : 0u) | (((Tm >> ll) & 1ull) != 0 || (Hm & ~za_mask_le(ll)) != 0 ? 4u : 0u);
        } else s = Hm != 0 ? 2u : 0u;
        v.w[wave] = s; v.wl[wave] = wave_last;
    }
    if (hasd) { atomicMin(&v.first, tid * 64u + fb); atomicMax(&v.last, mylast); }
    __syncthreads();
    uint32_t win = 0, prevpos = 0;                    // in front of this wave: has the open line matched, is there a delimiter, where
    bool prevd = false;
    for (uint32_t x = 0; x < wave; x++) {
        const uint32_t s = v.w[x];
        if (s & 1u) { win = s >> 2 & 1u; prevd = true; prevpos = v.wl[x]; } else win |= s >> 1 & 1u;
    }
    uint32_t carry;
    if (pd) { carry = (uint32_t)(Tm >> j & 1ull) | ((Hm & below & ~za_mask_le(j)) != 0 ? 1u : 0u); prevd = true; prevpos = lane_prev; }
    else carry = win | ((Hm & below) != 0 ? 1u : 0u);
    const uint32_t inv = flags & ZA_GREP_INVERT;
    uint64_t L = 0, d = D;
    uint32_t rows = 0, bytes = 0;
    int pb = -1;
    while (d) {
        const uint32_t b = (uint32_t)__builtin_ctzll(d);
        d &= d - 1ull;
        const uint64_t seg = M & za_mask_le(b) & ~(pb >= 0 ? za_mask_le((uint32_t)pb) : 0ull);
        const uint32_t m = (pb >= 0 ? 0u : carry) | (seg != 0 ? 1u : 0u);
        if ((pb >= 0 || prevd) && (m ^ inv)) {        // (the tile's first delimiter ends a line that began in front of the tile: the scan decides it)
            L |= 1ull << b; rows++;
            bytes += tid * 64u + b - (pb >= 0 ? tid * 64u + (uint32_t)pb : prevpos);
        }
        pb = (int)b;
    }
    bits[(size_t)blockIdx.x * 256u + tid] = make_ulonglong2(D, L);
    uint32_t nd = (uint32_t)__popcll(D);
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) { nd += __shfl_xor(nd, x, 64); rows += __shfl_xor(rows, x, 64); bytes += __shfl_xor(bytes, x, 64); }
    if (lane == 0) { v.cnt[wave][0] = nd; v.cnt[wave][1] = rows; v.cnt[wave][2] = bytes; }
    __syncthreads();
    if (tid == 0) {
        uint32_t head = 0, tail = 0;
        bool seen = false;
        for (uint32_t x = 0; x < 4u; x++) {
            const uint32_t s = v.w[x];
            if (!seen) { head |= s >> 1 & 1u; if (s & 1u) { seen = true; tail = s >> 2 & 1u; } }
            else if (s & 1u) tail = s >> 2 & 1u;
            else tail |= s >> 1 & 1u;
        }
        ZaGrepTile t;
        t.ndelim = v.cnt[0][0] + v.cnt[1][0] + v.cnt[2][0] + v.cnt[3][0];
        t.first = t.ndelim ? v.first : 0u; t.last = v.last;
        t.flags = (head ? ZA_GREP_HEAD : 0u) | (seen && tail ? ZA_GREP_TAIL : 0u);
        t.rows = v.cnt[0][1] + v.cnt[1][1] + v.cnt[2][1] + v.cnt[3][1];
        t.bytes = v.cnt[0][2] + v.cnt[1][2] + v.cnt[2][2] + v.cnt[3][2];
        tiles[blockIdx.x] = t;
    }
}

// grid: one workgroup per tile, tile0 + blockIdx.x.  bits[tile][thread] = {delimiter bits, verdict bits} of the thread's 64 bytes: a
// verdict bit stands at the delimiter of a line that begins and ends in the tile and is selected (INVERT applied).  With LINE_START
// a pattern counts only at a line's first byte, so "a pattern starts in the line" is the test in both modes.
__global__ __launch_bounds__(256) void za_k_grep_mark(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t text_off, uint64_t text_end,
                                                      uint64_t tile0, const uint32_t *__restrict__ pairs, const ZaGrepPat *__restrict__ ptab,
                                                      const uint8_t *__restrict__ blob, uint32_t np, uint32_t delim, uint32_t flags,
                                                      ulonglong2 *__restrict__ bits, ZaGrepTile *__restrict__ tiles)
{
    __shared__ uint32_t s_pairs[ZA_GREP_PAIR_WORDS];
    __shared__ uint32_t s_d[512], s_m[512];
    __shared__ uint32_t s_key[ZA_GREP_MAX_PAT], s_off[ZA_GREP_MAX_PAT];
    __shared__ ZaGrepVerdictLds s_v;
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (tile0 + blockIdx.x) * (uint64_t)ZA_GREP_TILE;
    for (uint32_t i = tid; i < ZA_GREP_PAIR_WORDS; i += 256u) s_pairs[i] = pairs[i];
    s_d[tid] = 0; s_d[tid + 256u] = 0; s_m[tid] = 0; s_m[tid + 256u] = 0;
    if (tid < np) {
        const ZaGrepPat pt = ptab[tid];
        s_off[tid] = pt.off;
        s_key[tid] = pt.len | (uint32_t)blob[pt.off] << 8 | (pt.len > 1u ? (uint32_t)blob[pt.off + 1u] << 16 : 0u);
    }
    if (tid == 0) { s_v.first = 0xFFFFFFFFu; s_v.last = 0; }
    __syncthreads();
    const uint32_t pat = delim * 0x01010101u;
    for (uint32_t it = 0; it < 4u; it++) {            // 16 bytes per thread and round: 4 KiB per round
        const uint32_t rel = (it * 256u + tid) * 16u;
        const uint64_t g = base + rel;
        if (g >= text_end || (text_off > g && text_off - g >= 16u)) continue;       // (no barrier in this loop)
        uint32_t w[5] = {0, 0, 0, 0, 0};
        if (scratch_cap - g >= 16u) { const ZaU4u v = *(const ZaU4u *)(scratch + g); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
        else {                                                                        // the scratch ends inside these 16 bytes
            uint64_t a = 0, b = 0;
            for (uint32_t k = 0; k < (uint32_t)(scratch_cap - g); k++) { const uint64_t x = scratch[g + k]; if (k < 8u) a |= x << (8u * k); else b |= x << (8u * (k - 8u)); }
            w[0] = (uint32_t)a; w[1] = (uint32_t)(a >> 32); w[2] = (uint32_t)b; w[3] = (uint32_t)(b >> 32);
        }
        if (text_end - g > 16u) w[4] = scratch[g + 16u];
        const uint32_t lo = text_off > g ? (uint32_t)(text_off - g) : 0u, hi = text_end - g >= 16u ? 16u : (uint32_t)(text_end - g);
        const uint32_t valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        const uint32_t dmraw = za_mask_nibble(za_eq_mask(w[0], pat)) | za_mask_nibble(za_eq_mask(w[1], pat)) << 4 |
                               za_mask_nibble(za_eq_mask(w[2], pat)) << 8 | za_mask_nibble(za_eq_mask(w[3], pat)) << 12;
        uint32_t cand = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t pr = (uint32_t)((((uint64_t)w[k / 4u + 1u] << 32 | w[k / 4u]) >> (8u * (k & 3u))) & 0xFFFFu);
            cand |= (s_pairs[pr >> 5] >> (pr & 31u) & 1u) << k;
        }
        cand &= valid;
        if (flags & ZA_GREP_LINE_START) {
            uint32_t ls = (dmraw << 1) & 0xFFFFu;
            if (g > text_off) ls |= scratch[g - 1u] == delim ? 1u : 0u;
            else ls |= 1u << lo;                                       // the text begins with a line
            cand &= ls;
        }
        uint32_t mm = 0;
        while (cand) {
            const uint32_t k = (uint32_t)__builtin_ctz(cand);
            cand &= cand - 1u;
            if (za_grep_verify(scratch, g + k, text_end, s_key, s_off, blob, np)) mm |= 1u << k;
        }
        const uint32_t dm = dmraw & valid;
        if (dm) atomicOr(&s_d[rel >> 5], dm << (rel & 31u));
        if (mm) atomicOr(&s_m[rel >> 5], mm << (rel & 31u));
    }
    __syncthreads();
    za_grep_tile_verdicts(s_d, s_m, s_v, flags, bits, tiles);
}

// ---- up to k mismatches
// the non-zero bytes of x as their 0x80 bits (no carry leaves a byte: 0x7f + 0x7f = 0xfe)
__device__ __forceinline__ uint32_t za_nonzero_bytes(uint32_t x) { return ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x; }

// Steps 1 and 2 of za_k_grep_mark_approx, shared with za_k_grep_classify (za_classify.hip).  s_d and s_stop were zeroed in front of a
// barrier.  Every thread of the workgroup calls it (it holds barriers): behind it s_t holds the tile and its overhang, s_d the tile's
// delimiter bits, s_stop the stop bits and s_before[w] the stop bits in front of bitmap word w.
__device__ __forceinline__ void za_grep_approx_stage(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t text_off, uint64_t text_end, uint64_t base,
                                                     uint32_t delim, uint32_t *s_t, uint32_t *s_d, uint32_t *s_stop, uint32_t *s_before, uint32_t *s_wsum)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t pat = delim * 0x01010101u;
    for (uint32_t ch = tid; ch < ZA_GREP_AP_WORDS / 4u; ch += 256u) {       // 16 bytes per thread and round (no barrier in this loop)
        const uint32_t rel = ch * 16u;
        const uint64_t g = base + rel;
        uint32_t w[4] = {0, 0, 0, 0}, dm = 0, stop = 0xFFFFu;
        if (g < text_end && !(text_off > g && text_off - g >= 16u)) {
            if (scratch_cap - g >= 16u) { const ZaU4u v = *(const ZaU4u *)(scratch + g); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
            else {                                                                    // the scratch ends inside these 16 bytes
                uint64_t a = 0, b = 0;
                for (uint32_t i = 0; i < (uint32_t)(scratch_cap - g); i++) { const uint64_t x = scratch[g + i]; if (i < 8u) a |= x << (8u * i); else b |= x << (8u * (i - 8u)); }
                w[0] = (uint32_t)a; w[1] = (uint32_t)(a >> 32); w[2] = (uint32_t)b; w[3] = (uint32_t)(b >> 32);
            }
            const uint32_t lo = text_off > g ? (uint32_t)(text_off - g) : 0u, hi = text_end - g >= 16u ? 16u : (uint32_t)(text_end - g);
            const uint32_t dmraw = za_mask_nibble(za_eq_mask(w[0], pat)) | za_mask_nibble(za_eq_mask(w[1], pat)) << 4 |
                                   za_mask_nibble(za_eq_mask(w[2], pat)) << 8 | za_mask_nibble(za_eq_mask(w[3], pat)) << 12;
            dm = dmraw & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
            stop = (dmraw | ~((1u << hi) - 1u)) & 0xFFFFu;
        }
        *(uint4 *)&s_t[ch * 4u] = make_uint4(w[0], w[1], w[2], w[3]);
        if (dm && rel < ZA_GREP_TILE) atomicOr(&s_d[rel >> 5], dm << (rel & 31u));
        atomicOr(&s_stop[rel >> 5], stop << (rel & 31u));
    }
    __syncthreads();
    {   // s_before: thread tid sums the bitmap words 2 tid and 2 tid + 1 of the tile; the overhang's eight words follow the tile's total
        const uint32_t n0 = (uint32_t)__popc(s_stop[2u * tid]), n1 = (uint32_t)__popc(s_stop[2u * tid + 1u]);
        const uint32_t incl = za_wave_incl_scan(n0 + n1);
        if (lane == 63u) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t ex = incl - n0 - n1;
        for (uint32_t x = 0; x < wave; x++) ex += s_wsum[x];
        s_before[2u * tid] = ex; s_before[2u * tid + 1u] = ex + n0;
        if (tid < ZA_GREP_AP_BITS - 512u) {
            uint32_t t = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
            for (uint32_t i = 0; i < tid; i++) t += (uint32_t)__popc(s_stop[512u + i]);
            s_before[512u + tid] = t;
        }
    }
    __syncthreads();
}

// Step 3: every position of the tile against every pattern.  A window that is within k and holds no stop bit is a match: hit(b, q, d)
// is told its offset in the tile, the pattern and the distance, and once a round of four positions per thread is through
// round(rel, mm) is told which of the four matched.  ALL = false: a position that has matched is compared with no further pattern (a
// bit is all za_k_grep_mark_approx wants); ALL = true: every pattern is compared at every position.  No barrier in here.
template <bool ALL, typename Hit, typename Round>
__device__ __forceinline__ void za_grep_approx_compare(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end, uint64_t base,
                                                       const ZaGrepPat *__restrict__ ptab, const uint32_t *__restrict__ words, uint32_t np, uint32_t delim,
                                                       uint32_t flags, uint32_t k, const uint32_t *s_t, const uint32_t *s_d, const uint32_t *s_stop,
                                                       const uint32_t *s_before, Hit hit, Round round)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t it = 0; it < 16u; it++) {            // 4 positions per thread and round: 1 KiB per round (no barrier in this loop)
        const uint32_t w = it * 256u + tid, rel = w * 4u;
        const uint64_t g = base + rel;
        uint32_t alive = 0;                            // the positions of the four where a pattern may start
        if (g < text_end) {
            const uint32_t lo = text_off > g ? (text_off - g >= 4u ? 4u : (uint32_t)(text_off - g)) : 0u, hi = text_end - g >= 4u ? 4u : (uint32_t)(text_end - g);
            alive = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        }
        if ((flags & ZA_GREP_LINE_START) && alive) {
            uint32_t ls = (s_d[rel >> 5] >> (rel & 31u) & 7u) << 1;
            if (rel) ls |= s_d[(rel - 1u) >> 5] >> ((rel - 1u) & 31u) & 1u;
            else if (g > text_off) ls |= scratch[g - 1u] == delim ? 1u : 0u;
            if (text_off >= g && text_off - g < 4u) ls |= 1u << (uint32_t)(text_off - g);      // the text begins with a line
            alive &= ls;
        }
        if (__ballot(alive != 0) == 0ull) continue;
        const uint32_t t0 = s_t[w];
        uint32_t mm = 0;
        for (uint32_t q = 0; q < np; q++) {
            const uint32_t live = ALL ? alive : alive & ~mm;      // (a position that has matched needs no further pattern)
            if (__ballot(live != 0) == 0ull) break;
            const ZaGrepPat pt = ptab[q];
            const uint32_t nw = (pt.len + 3u) >> 2, last80 = 0x80808080u >> (8u * (nw * 4u - pt.len));
            const uint32_t *__restrict__ pw = words + pt.off;
            uint32_t c0 = live & 1u ? 0u : 256u, c1 = live & 2u ? 0u : 256u, c2 = live & 4u ? 0u : 256u, c3 = live & 8u ? 0u : 256u;
            uint32_t lo = t0;
            for (uint32_t j = 0; j < nw; j++) {
                const uint32_t hi = s_t[w + j + 1u], p = pw[j], m80 = j + 1u == nw ? last80 : 0x80808080u;
                c0 += (uint32_t)__popc(za_nonzero_bytes(lo ^ p) & m80);
                c1 += (uint32_t)__popc(za_nonzero_bytes(__builtin_amdgcn_alignbyte(hi, lo, 1u) ^ p) & m80);
                c2 += (uint32_t)__popc(za_nonzero_bytes(__builtin_amdgcn_alignbyte(hi, lo, 2u) ^ p) & m80);
                c3 += (uint32_t)__popc(za_nonzero_bytes(__builtin_amdgcn_alignbyte(hi, lo, 3u) ^ p) & m80);
                lo = hi;
                const uint32_t c01 = c0 < c1 ? c0 : c1, c23 = c2 < c3 ? c2 : c3;
                if (__ballot((c01 < c23 ? c01 : c23) <= k) == 0ull) break;      // every pair of this wave has left
            }
            uint32_t cand = (c0 <= k ? 1u : 0u) | (c1 <= k ? 2u : 0u) | (c2 <= k ? 4u : 0u) | (c3 <= k ? 8u : 0u);
            while (cand) {
                const uint32_t s = (uint32_t)__builtin_ctz(cand);
                cand &= cand - 1u;
                const uint32_t b = rel + s, e = b + pt.len;
                const uint32_t nb = s_before[b >> 5] + (uint32_t)__popc(s_stop[b >> 5] & ((1u << (b & 31u)) - 1u));
                const uint32_t ne = s_before[e >> 5] + (uint32_t)__popc(s_stop[e >> 5] & ((1u << (e & 31u)) - 1u));
                if (nb == ne) { mm |= 1u << s; hit(b, q, s == 0u ? c0 : s == 1u ? c1 : s == 2u ? c2 : c3); }
            }
        }
        round(rel, mm);
    }
}

// grid, bits[] and tiles[] as za_k_grep_mark; what differs is how a match bit comes about: a pattern of len bytes starts at p when
// scratch[p, p + len) differs from it in at most k bytes, holds no delimiter and ends at or in front of text_end (so the window lies in
// one line's body).  No prefilter: every position is compared with every pattern, four pattern bytes a step.
//   - The tile and the 255 bytes behind it (a window that starts in its last byte) are staged in LDS as dwords; nothing at or behind
//     text_end is read, and so nothing at or behind scratch_cap.
//   - s_stop has a bit per staged byte that no window may hold: a delimiter, or a byte at or behind text_end.  s_before[w] counts the
//     stop bits in front of bitmap word w, so "no stop bit in [p, p + len)" is two counts that are equal.  It is asked of the positions
//     whose count stayed within k only.
//   - A thread takes four adjacent positions a round, so a wave reads 64 adjacent dwords of the text per pattern dword; the loops over
//     patterns and pattern dwords are the same for a whole wave (they end on ballots), which leaves the pattern words in scalar registers.
// ptab[q] = {off, len}: the pattern's first DWORD in words[] and its length in bytes; the last dword is padded with zeros.
__global__ __launch_bounds__(256) void za_k_grep_mark_approx(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t text_off, uint64_t text_end,
                                                             uint64_t tile0, const ZaGrepPat *__restrict__ ptab, const uint32_t *__restrict__ words,
                                                             uint32_t np, uint32_t delim, uint32_t flags, uint32_t k,
                                                             ulonglong2 *__restrict__ bits, ZaGrepTile *__restrict__ tiles)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_t[ZA_GREP_AP_WORDS];
    __shared__ uint32_t s_d[512], s_m[512];
    __shared__ uint32_t s_stop[ZA_GREP_AP_BITS], s_before[ZA_GREP_AP_BITS];
    __shared__ uint32_t s_wsum[4];
    __shared__ ZaGrepVerdictLds s_v;
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (tile0 + blockIdx.x) * (uint64_t)ZA_GREP_TILE;
    s_d[tid] = 0; s_d[tid + 256u] = 0; s_m[tid] = 0; s_m[tid + 256u] = 0;
    for (uint32_t i = tid; i < ZA_GREP_AP_BITS; i += 256u) s_stop[i] = 0;
    if (tid == 0) { s_v.first = 0xFFFFFFFFu; s_v.last = 0; }
    __syncthreads();
    za_grep_approx_stage(scratch, scratch_cap, text_off, text_end, base, delim, s_t, s_d, s_stop, s_before, s_wsum);
    za_grep_approx_compare<false>(scratch, text_off, text_end, base, ptab, words, np, delim, flags, k, s_t, s_d, s_stop, s_before,
                                  [](uint32_t, uint32_t, uint32_t) {}, [&](uint32_t rel, uint32_t mm) { if (mm) atomicOr(&s_m[rel >> 5], mm << (rel & 31u)); });
    __syncthreads();
    za_grep_tile_verdicts(s_d, s_m, s_v, flags, bits, tiles);
}

// The scan's state in front of a tile, and its step.  The operator is associative (a segmented OR with sums beside it), so a chunk
// of tiles is summarised without knowing what lies in front of it: see ZaGrepChunk.
struct ZaGrepState { uint64_t open_start, lines, rows, bytes; uint32_t open_m; };
__device__ __forceinline__ uint32_t za_grep_step(ZaGrepState &s, const ZaGrepTile &t, uint64_t tile_base, uint32_t inv)
{
    if (!t.ndelim) { s.open_m |= t.flags & ZA_GREP_HEAD; return 0u; }
    const uint32_t dec = (s.open_m | (t.flags & ZA_GREP_HEAD)) ^ inv;
    if (dec) { s.rows++; s.bytes += tile_base + t.first - s.open_start + 1ull; }
    s.rows += t.rows; s.bytes += t.bytes; s.lines += t.ndelim;
    s.open_start = tile_base + t.last + 1ull;
    s.open_m = t.flags >> 1 & 1u;
    return dec;
}
struct ZaGrepChunk { ZaGrepState s; uint64_t first_e; uint32_t seen, pre_head; };      // s: sums WITHOUT the chunk's first line; first_e: where that line ends

// grid: one workgroup of 512.  Every thread summarises a run of tiles, thread 0 walks the 512 summaries, every thread walks its run
// again with the state in front of it (the manner of za_k_offsets).  cover: what za_k_grep_cover left.
__global__ __launch_bounds__(ZA_GREP_SCAN_THREADS) void za_k_grep_scan(const ZaGrepTile *__restrict__ tiles, uint32_t n, uint64_t tile0, uint64_t text_off,
                                                                       uint64_t text_end, uint32_t flags, uint64_t line_base,
                                                                       const unsigned long long *__restrict__ cover, ZaGrepCarry *__restrict__ carry,
                                                                       ZaGrepTotals *__restrict__ totals)
{
    __shared__ ZaGrepChunk part[ZA_GREP_SCAN_THREADS];
    const uint32_t tid = threadIdx.x, inv = flags & ZA_GREP_INVERT;
    if (cover[0] != text_end - text_off || cover[1] != 0ull) {       // (the same for every thread)
        if (tid == 0) { ZaGrepTotals z = {}; z.tail_off = text_off; *totals = z; }
        return;
    }
    const uint32_t per = (n + ZA_GREP_SCAN_THREADS - 1u) / ZA_GREP_SCAN_THREADS;
    const uint32_t b = tid * per < n ? tid * per : n, e = b + per < n ? b + per : n;
    ZaGrepChunk c = {};
    for (uint32_t i = b; i < e; i++) {
        const ZaGrepTile t = tiles[i];
        const uint64_t tb = (tile0 + i) * (uint64_t)ZA_GREP_TILE;
        if (c.seen) { (void)za_grep_step(c.s, t, tb, inv); continue; }
        c.pre_head |= t.flags & ZA_GREP_HEAD;
        if (t.ndelim) {
            c.seen = 1; c.first_e = tb + t.first;
            c.s.rows = t.rows; c.s.bytes = t.bytes; c.s.lines = t.ndelim; c.s.open_start = tb + t.last + 1ull; c.s.open_m = t.flags >> 1 & 1u;
        }
    }
    part[tid] = c;
    __syncthreads();
    if (tid == 0) {
        ZaGrepState s = {}; s.open_start = text_off;
        for (uint32_t i = 0; i < ZA_GREP_SCAN_THREADS; i++) {
            const ZaGrepChunk k = part[i];
            part[i].s = s;                                          // the state in front of chunk i
            if (!k.seen) { s.open_m |= k.pre_head; continue; }
            if ((s.open_m | k.pre_head) ^ inv) { s.rows++; s.bytes += k.first_e - s.open_start + 1ull; }
            s.rows += k.s.rows; s.bytes += k.s.bytes; s.lines += k.s.lines;
            s.open_start = k.s.open_start; s.open_m = k.s.open_m;
        }
        ZaGrepTotals z = {};
        z.covered = 1; z.seen = s.lines; z.matched = s.rows; z.bytes = s.bytes; z.tail_off = s.open_start;
        if ((flags & ZA_GREP_FINAL) && s.open_start < text_end) {    // the bytes behind the last delimiter are a line
            z.seen++; z.tail_off = text_end;
            if (s.open_m ^ inv) { z.final_emit = 1; z.final_src = s.open_start; z.final_number = line_base + s.lines; z.matched++; z.bytes += text_end - s.open_start; }
        }
        *totals = z;
    }
    __syncthreads();
    ZaGrepState s = part[tid].s;
    for (uint32_t i = b; i < e; i++) {
        const ZaGrepTile t = tiles[i];
        ZaGrepCarry r; r.open_start = s.open_start; r.lines = s.lines; r.row_base = s.rows; r.reserved = 0;
        r.first_emit = za_grep_step(s, t, (tile0 + i) * (uint64_t)ZA_GREP_TILE, inv);
        carry[i] = r;
    }
}

// grid: one workgroup per tile.  rows[] and lens[] have room for rows_cap entries (the host has seen the totals: at least `matched`).
__global__ __launch_bounds__(256) void za_k_grep_emit(const ulonglong2 *__restrict__ bits, const ZaGrepTile *__restrict__ tiles, const ZaGrepCarry *__restrict__ carry,
                                                      const ZaGrepTotals *__restrict__ totals, uint64_t tile0, uint64_t line_base, uint64_t text_end,
                                                      ZaGrepRow *__restrict__ rows, uint64_t rows_cap, uint32_t *__restrict__ lens)
{
    __shared__ uint32_t s_nd[4], s_ne[4], s_wl[4], s_wh[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (blockIdx.x == 0 && tid == 0 && totals->final_emit) {
        const uint64_t idx = totals->matched - 1ull;
        if (idx < rows_cap) {
            ZaGrepRow r; r.src_off = totals->final_src; r.number = totals->final_number; r.len = (uint32_t)(text_end - totals->final_src); r.reserved = 0;
            rows[idx] = r; lens[idx] = r.len;
        }
    }
    const ZaGrepTile t = tiles[blockIdx.x];
    if (!t.ndelim) return;                            // (the same for every thread)
    const ZaGrepCarry c = carry[blockIdx.x];
    const uint64_t base = (tile0 + blockIdx.x) * (uint64_t)ZA_GREP_TILE;
    const ulonglong2 v = bits[(size_t)blockIdx.x * 256u + tid];
    const uint64_t D = v.x;
    uint64_t L = v.y;
    if (c.first_emit && (t.first >> 6) == tid) L |= 1ull << (t.first & 63u);
    const bool hasd = D != 0;
    const uint32_t nd = (uint32_t)__popcll(D), ne = (uint32_t)__popcll(L);
    const uint32_t id = za_wave_incl_scan(nd), ie = za_wave_incl_scan(ne);
    const uint64_t Dm = __ballot(hasd);
    const uint32_t mylast = tid * 64u + (hasd ? 63u - (uint32_t)__builtin_clzll(D) : 0u);
    const uint64_t pd = Dm & ((1ull << lane) - 1ull);
    const uint32_t lane_prev = (uint32_t)__shfl((int)mylast, pd ? 63 - __builtin_clzll(pd) : 0, 64);
    const uint32_t wave_last = (uint32_t)__shfl((int)mylast, Dm ? 63 - __builtin_clzll(Dm) : 0, 64);
    if (lane == 63u) { s_nd[wave] = id; s_ne[wave] = ie; s_wl[wave] = wave_last; s_wh[wave] = Dm != 0 ? 1u : 0u; }
    __syncthreads();
    uint32_t rd = id - nd, re = ie - ne, prevpos = 0;
    bool prevd = false;
    for (uint32_t x = 0; x < wave; x++) { rd += s_nd[x]; re += s_ne[x]; if (s_wh[x]) { prevd = true; prevpos = s_wl[x]; } }
    if (pd) { prevd = true; prevpos = lane_prev; }
    uint64_t s = prevd ? base + prevpos + 1ull : c.open_start, d = D;
    while (d) {
        const uint32_t b = (uint32_t)__builtin_ctzll(d);
        d &= d - 1ull;
        const uint64_t e = base + tid * 64u + b;
        if (L >> b & 1ull) {
            const uint64_t idx = c.row_base + re;
            if (idx < rows_cap) {
                ZaGrepRow r; r.src_off = s; r.number = line_base + c.lines + rd; r.len = (uint32_t)(e - s + 1ull); r.reserved = 0;
                rows[idx] = r; lens[idx] = r.len;
            }
            re++;
        }
        rd++;
        s = e + 1ull;
    }
}

__global__ __launch_bounds__(256) void za_k_grep_place(const ZaGrepRow *__restrict__ rows, const uint64_t *__restrict__ offs, uint64_t n, ZaBgzfSlice *__restrict__ slices)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ZaBgzfSlice s; s.src_off = rows[i].src_off; s.dst_off = offs[i]; s.len = rows[i].len; s.reserved = 0;
    slices[i] = s;
}

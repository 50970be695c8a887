// BGZF: fields of a line.  The decoded blocks lie in the scratch as one byte string, as for za_grep.hip.  One
// device function, za_tbx_parse, reads the columns of a tab-separated line by the rules of tabix; two users:
//   the index build (zngamd_bgzf_tabix), over the text scratch[text_off, text_end) in tiles of 16 KiB:
//     za_k_tbx_mark     one thread per 64 bytes: the delimiter bits of its word; per tile their number
//     (za_k_offsets)    delimiters in front of every tile
//     za_k_tbx_parse    one thread per 64 bytes: every line that STARTS behind a delimiter of its word (line 0: at text_off) is parsed
//                       into a record at its ordinal
//     za_k_tbx_reduce / _scan_blocks / _apply    one inclusive scan (sum or max) over an array of u64, in place
//     za_k_tbx_compact  the ordinals of the data lines, dense
//     za_k_tbx_edges    per data line: does a name begin here, does a bin begin here, is it out of order
//     za_k_tbx_keys / _raise   name run << 15 | last window, whose running maximum is the segmented maximum of the last window:
//                       a line that raises it opens windows of the linear index
//     za_k_tbx_emit / _finish  the three tables;  za_k_tbx_place + za_k_slice_gather pack the names
//   the region filter (zngamd_bgzf_fetch): za_k_tbx_fetch, one workgroup per span, counts and then emits the rows of the lines that
//     overlap the span's region; za_k_offsets, za_k_tbx_place_rows and za_k_slice_gather pack them.
// Included by zng_amd.hip behind za_grep.hip (za_eq_mask, za_mask_nibble, za_k_grep_cover, ZaBgzfSlice).
#include "za_common.h"

#define ZA_TBX_TILE      16384u        // bytes per tile: 256 threads x 64 bytes
#define ZA_TBX_FINAL     4u            // flags: mirror ZNGAMD_BGZF_TABIX_FINAL / ZNGAMD_BGZF_FETCH_COUNT_ONLY
#define ZA_TBX_COUNT_ONLY 8u
#define ZA_TBX_DATA      0u            // kinds of a line; a bad line is ZA_TBX_SKIP + its number in the issue's order (1 .. 4)
#define ZA_TBX_SKIP      1u
#define ZA_TBX_BAD_COLS  2u            // a needed column is missing
#define ZA_TBX_BAD_NUM   3u            // a coordinate is not 1 .. 10 digits
#define ZA_TBX_BAD_RANGE 4u            // beg < 0 or end > 2^29
#define ZA_TBX_BAD_ORDER 5u            // beg below the previous data line's of the same name
#define ZA_TBX_MAX_POS   (1ll << 29)
#define ZA_TBX_SCAN_ITEMS 1024u        // elements per workgroup of the array scans (256 threads x 4)
#define ZA_TBX_SUM 0
#define ZA_TBX_MAX 1

struct ZaTbxConf { int32_t format, col_seq, col_beg, col_end, meta, skip; };                         // mirrors zngamd_tabix_conf
struct ZaTbxLine { uint64_t start; uint32_t len, name_rel, name_len, beg, end, kind; };            // len: with the delimiter
struct ZaTbxName { uint64_t src_off, first, line; uint32_t len, reserved; };                         // mirrors zngamd_tabix_name
struct ZaTbxBin { uint64_t src_beg, src_end, first, lines; uint32_t name, bin; };                    // mirrors zngamd_tabix_bin
struct ZaTbxWin { uint64_t src_off; uint32_t name, window; };                                        // mirrors zngamd_tabix_win
struct ZaTbxRegion { uint32_t name_off, name_len, beg, end; };                                       // mirrors zngamd_tabix_region
struct ZaTbxSpan { uint64_t text_off, text_end; uint32_t region, reserved; };                        // mirrors zngamd_tabix_span
struct ZaTbxRow { uint64_t src_off; uint32_t len, region; };                                         // mirrors zngamd_tabix_row
struct ZaTbxState {                    // what the kernels of one build leave for the host (device memory, at most 64 B)
    unsigned long long bad_key;        // smallest (line number << 3 | kind) of a bad line; ~0: none
    unsigned long long tail_off, name_bytes, first_line, first_src;
    uint32_t first_beg, last_beg, final_line, reserved;
};

__device__ __forceinline__ uint32_t za_tbx_reg2bin(uint32_t beg, uint32_t end)      // SAM specification section 5.3; end > beg
{
    --end;
    if (beg >> 14 == end >> 14) return 4681u + (beg >> 14);
    if (beg >> 17 == end >> 17) return 585u + (beg >> 17);
    if (beg >> 20 == end >> 20) return 73u + (beg >> 20);
    if (beg >> 23 == end >> 23) return 9u + (beg >> 23);
    if (beg >> 26 == end >> 26) return 1u + (beg >> 26);
    return 0u;
}

// s[a, b) as a coordinate: 1 to 10 ASCII digits and nothing else
__device__ __forceinline__ bool za_tbx_num(const uint8_t *__restrict__ s, uint64_t a, uint64_t b, int64_t &v)
{
    if (b <= a || b - a > 10u) return false;
    int64_t x = 0;
    for (uint64_t p = a; p < b; p++) {
        const uint32_t d = (uint32_t)s[p] - 48u;
        if (d > 9u) return false;
        x = x * 10 + (int64_t)d;
    }
    v = x;
    return true;
}

// The line that starts at s[start] (start < limit).  Nothing at or behind limit, or behind the line's delimiter, is read.  The line
// ends at its delimiter (terminated) or at limit.  out.kind and, for a data line, the name and the interval [beg, end).
__device__ __forceinline__ void za_tbx_parse(const uint8_t *__restrict__ s, uint64_t start, uint64_t limit, uint32_t delim, const ZaTbxConf &cf,
                                             uint64_t line_no, ZaTbxLine &out, bool &terminated)
{
    const bool vcf = (cf.format & 0xFFFF) == 2;
    const uint32_t ca = (uint32_t)cf.col_seq, cb = (uint32_t)cf.col_beg;
    const bool need_c = vcf || (cf.col_end != 0 && cf.col_end != cf.col_beg);
    const uint32_t cc = vcf ? 4u : (need_c ? (uint32_t)cf.col_end : 0u), cd = vcf ? 8u : 0u;
    uint64_t fa = 0, ea = 0, fb = 0, eb = 0, fc = 0, ec = 0, fd = 0, ed = 0, fs = start, p = start;
    uint32_t have = 0, col = 1;
    for (;;) {                                        // the walk over the fields: where the needed columns begin and end
        const bool stop = p >= limit;
        const uint32_t ch = stop ? delim : (uint32_t)s[p];
        const bool eol = stop || ch == delim;
        if (eol || ch == 9u) {
            uint64_t fe = p;
            if (eol && !stop && fe > fs && s[fe - 1u] == 13u) fe--;      // one CR in front of the delimiter belongs to no field
            if (col == ca) { fa = fs; ea = fe; have |= 1u; }
            if (col == cb) { fb = fs; eb = fe; have |= 2u; }
            if (col == cc) { fc = fs; ec = fe; have |= 4u; }
            if (col == cd) { fd = fs; ed = fe; have |= 8u; }
            if (eol) break;
            col++; fs = p + 1u;
        }
        p++;
    }
    terminated = p < limit;
    out.start = start; out.len = (uint32_t)(p - start) + (terminated ? 1u : 0u);
    out.name_rel = 0; out.name_len = 0; out.beg = 0; out.end = 0;
    const uint64_t ce = p - ((terminated && p > start && s[p - 1u] == 13u) ? 1u : 0u);
    if (line_no < (uint64_t)(uint32_t)cf.skip || ce == start || (uint32_t)s[start] == (uint32_t)cf.meta) { out.kind = ZA_TBX_SKIP; return; }
    if ((have & 3u) != 3u || (need_c && !(have & 4u))) { out.kind = ZA_TBX_BAD_COLS; return; }
    out.name_rel = (uint32_t)(fa - start); out.name_len = (uint32_t)(ea - fa);
    int64_t b = 0, e = 0;
    if (!za_tbx_num(s, fb, eb, b)) { out.kind = ZA_TBX_BAD_NUM; return; }
    int64_t beg, end;
    if (vcf) {
        beg = b - 1; end = beg + (int64_t)(ec - fc);
        if (have & 8u) {                              // the first END= at the first byte of INFO or behind a ';'
            bool key = true;
            for (uint64_t q = fd; q < ed; q++) {
                if (key && ed - q >= 4u && s[q] == 'E' && s[q + 1u] == 'N' && s[q + 2u] == 'D' && s[q + 3u] == '=') {
                    uint64_t r = q + 4u;
                    int64_t v = 0;
                    uint32_t nd = 0;
                    while (r < ed && (uint32_t)s[r] - 48u <= 9u) { if (v < (1ll << 40)) v = v * 10 + (int64_t)(s[r] - 48u); nd++; r++; }
                    if (nd && (r == ed || s[r] == ';') && v > beg) end = v;
                    break;
                }
                key = s[q] == ';';
            }
        }
    } else {
        beg = (cf.format & 0x10000) ? b : b - 1;
        if (need_c) { if (!za_tbx_num(s, fc, ec, e)) { out.kind = ZA_TBX_BAD_NUM; return; } end = e; }
        else end = beg + 1;
    }
    if (end <= beg) end = beg + 1;
    if (beg < 0 || end > ZA_TBX_MAX_POS) { out.kind = ZA_TBX_BAD_RANGE; return; }
    out.beg = (uint32_t)beg; out.end = (uint32_t)end; out.kind = ZA_TBX_DATA;
}

// the delimiter bits of scratch[w0, w0 + 64) that lie in [lo, hi) (hi <= scratch_cap): 16-byte loads where the scratch has them
__device__ __forceinline__ uint64_t za_tbx_word_mask(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t w0, uint64_t lo, uint64_t hi,
                                                     uint32_t delim)
{
    if (w0 >= hi || (lo > w0 && lo - w0 >= 64u)) return 0ull;
    const uint32_t pat = delim * 0x01010101u;
    uint64_t D = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint64_t g = w0 + 16u * k;
        if (g >= hi) break;
        uint32_t m;
        if (scratch_cap - g >= 16u) {
            const ZaU4u v = *(const ZaU4u *)(scratch + g);
            m = za_mask_nibble(za_eq_mask(v.x, pat)) | za_mask_nibble(za_eq_mask(v.y, pat)) << 4 | za_mask_nibble(za_eq_mask(v.z, pat)) << 8 |
                za_mask_nibble(za_eq_mask(v.w, pat)) << 12;
        } else {
            m = 0;
            for (uint32_t j = 0; j < (uint32_t)(scratch_cap - g); j++) m |= ((uint32_t)scratch[g + j] == delim ? 1u : 0u) << j;
        }
        D |= (uint64_t)m << (16u * k);
    }
    if (lo > w0) D &= ~((1ull << (lo - w0)) - 1ull);
    if (hi - w0 < 64u) D &= (1ull << (hi - w0)) - 1ull;
    return D;
}

// exclusive sum of n over the workgroup's 256 threads (all of them call it: two barriers); *total: the workgroup's sum
__device__ __forceinline__ uint32_t za_tbx_wg_excl(uint32_t n, uint32_t *s_w, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = za_wave_incl_scan(n);
    __syncthreads();                                  // (s_w may still be read from the call before)
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t x = 0; x < 4u; x++) { const uint32_t v = s_w[x]; if (x < wave) base += v; all += v; }
    *total = all;
    return base + incl - n;
}

// grid: one workgroup per tile, tile0 + blockIdx.x
__global__ __launch_bounds__(256) void za_k_tbx_mark(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t text_off, uint64_t text_end,
                                                     uint64_t tile0, uint32_t delim, unsigned long long *__restrict__ bits, uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t s_w[4];
    const uint64_t w0 = (tile0 + blockIdx.x) * (uint64_t)ZA_TBX_TILE + threadIdx.x * 64u;
    const uint64_t D = za_tbx_word_mask(scratch, scratch_cap, w0, text_off, text_end, delim);
    bits[(size_t)blockIdx.x * 256u + threadIdx.x] = D;
    uint32_t all;
    (void)za_tbx_wg_excl((uint32_t)__popcll(D), s_w, &all);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = all;
}

// grid: one workgroup per tile.  lines[] and is_data[] have room for the text's delimiters + 1 entries; the host has cleared the last
// entry of is_data.  Line k of the text starts behind its k-th delimiter (line 0: at text_off).
__global__ __launch_bounds__(256) void za_k_tbx_parse(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end, uint64_t tile0,
                                                      uint32_t delim, uint32_t flags, uint64_t line_base, ZaTbxConf cf,
                                                      const unsigned long long *__restrict__ bits, const uint64_t *__restrict__ tile_base,
                                                      uint64_t n_lines_cap, ZaTbxLine *__restrict__ lines, unsigned long long *__restrict__ is_data,
                                                      ZaTbxState *__restrict__ st)
{
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t w0 = (tile0 + blockIdx.x) * (uint64_t)ZA_TBX_TILE + tid * 64u;
    uint64_t D = bits[(size_t)blockIdx.x * 256u + tid];
    uint32_t all;
    uint64_t ord = tile_base[blockIdx.x] + za_tbx_wg_excl((uint32_t)__popcll(D), s_w, &all);      // delimiters in front of this word
    const bool first = text_off < text_end && text_off >= w0 && text_off - w0 < 64u;                // line 0 starts in this word
    auto line = [&](uint64_t start, uint64_t k) {
        if (start >= text_end || k >= n_lines_cap) return;
        ZaTbxLine L;
        bool term;
        za_tbx_parse(scratch, start, text_end, delim, cf, line_base + k, L, term);
        if (!term) {
            if (!(flags & ZA_TBX_FINAL)) { st->tail_off = start; return; }      // the open line: the next call's
            st->final_line = 1u;
        }
        lines[k] = L;
        is_data[k] = L.kind == ZA_TBX_DATA ? 1ull : 0ull;
        if (L.kind > ZA_TBX_SKIP) atomicMin(&st->bad_key, (unsigned long long)(line_base + k) << 3 | (L.kind - ZA_TBX_SKIP));
    };
    if (first) line(text_off, 0);
    while (D) {
        const uint32_t b = (uint32_t)__builtin_ctzll(D);
        D &= D - 1ull;
        line(w0 + b + 1ull, ++ord);
    }
}

// ---- one inclusive scan of v[0, n) in place: per workgroup of 1024 elements its sum or maximum, a single workgroup scans those,
// every workgroup scans its elements again behind what lies in front of it
__device__ __forceinline__ unsigned long long za_tbx_op(unsigned long long a, unsigned long long b, int op) { return op == ZA_TBX_SUM ? a + b : (a > b ? a : b); }

__device__ __forceinline__ unsigned long long za_tbx_wg_scan(unsigned long long mine, int op, unsigned long long *s_w, unsigned long long *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(incl, d, 64); if ((int)lane >= d) incl = za_tbx_op(incl, o, op); }
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    unsigned long long base = 0, all = 0;             // (0 is the identity of both: the values are unsigned)
    for (uint32_t x = 0; x < 4u; x++) { const unsigned long long v = s_w[x]; if (x < wave) base = za_tbx_op(base, v, op); all = za_tbx_op(all, v, op); }
    *total = all;
    return za_tbx_op(base, incl, op);                 // inclusive over the threads
}

__global__ __launch_bounds__(256) void za_k_tbx_reduce(const unsigned long long *__restrict__ v, uint64_t n, int op, unsigned long long *__restrict__ blk)
{
    __shared__ unsigned long long s_w[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * ZA_TBX_SCAN_ITEMS + threadIdx.x * 4u;
    unsigned long long a = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) if (i0 + k < n) a = za_tbx_op(a, v[i0 + k], op);
    unsigned long long all;
    (void)za_tbx_wg_scan(a, op, s_w, &all);
    if (threadIdx.x == 0) blk[blockIdx.x] = all;
}

// grid: one workgroup of 1024.  blk[i] becomes what lies in front of workgroup i; *total: everything
__global__ __launch_bounds__(1024) void za_k_tbx_scan_blocks(unsigned long long *__restrict__ blk, uint32_t nb, int op, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long part[1024];
    const uint32_t tid = threadIdx.x, per = (nb + 1023u) / 1024u;
    const uint32_t b = tid * per < nb ? tid * per : nb, e = b + per < nb ? b + per : nb;
    unsigned long long a = 0;
    for (uint32_t i = b; i < e; i++) a = za_tbx_op(a, blk[i], op);
    part[tid] = a;
    __syncthreads();
    if (tid == 0) {
        unsigned long long run = 0;
        for (uint32_t i = 0; i < 1024u; i++) { const unsigned long long x = part[i]; part[i] = run; run = za_tbx_op(run, x, op); }
        *total = run;
    }
    __syncthreads();
    unsigned long long run = part[tid];
    for (uint32_t i = b; i < e; i++) { const unsigned long long x = blk[i]; blk[i] = run; run = za_tbx_op(run, x, op); }
}

__global__ __launch_bounds__(256) void za_k_tbx_apply(unsigned long long *__restrict__ v, uint64_t n, int op, const unsigned long long *__restrict__ blk)
{
    __shared__ unsigned long long s_w[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * ZA_TBX_SCAN_ITEMS + threadIdx.x * 4u;
    unsigned long long x[4], a = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) { x[k] = i0 + k < n ? v[i0 + k] : 0ull; a = za_tbx_op(a, x[k], op); x[k] = a; }
    unsigned long long all;
    const unsigned long long incl = za_tbx_wg_scan(a, op, s_w, &all);
    // what lies in front of this thread: the workgroups in front, and the threads in front (the scan of the threads without `a`)
    const unsigned long long up = __shfl_up(incl, 1, 64);
    unsigned long long front = blk[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane) front = za_tbx_op(front, up, op);
    else for (uint32_t w = 0; w < wave; w++) front = za_tbx_op(front, s_w[w], op);
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) if (i0 + k < n) v[i0 + k] = za_tbx_op(front, x[k], op);
}

// ---- over the data lines.  s_data: the inclusive sums of is_data; *n_data = its total.  Threads at or behind *n_data write zeros.
__global__ __launch_bounds__(256) void za_k_tbx_compact(const unsigned long long *__restrict__ s_data, uint64_t n, uint32_t *__restrict__ di)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long a = s_data[i], p = i ? s_data[i - 1u] : 0ull;
    if (a != p) di[a - 1ull] = (uint32_t)i;
}

__device__ __forceinline__ bool za_tbx_same_name(const uint8_t *__restrict__ s, const ZaTbxLine &a, const ZaTbxLine &b)
{
    if (a.name_len != b.name_len) return false;
    const uint8_t *x = s + a.start + a.name_rel, *y = s + b.start + b.name_rel;
    for (uint32_t i = 0; i < a.name_len; i++) if (x[i] != y[i]) return false;
    return true;
}

__global__ __launch_bounds__(256) void za_k_tbx_edges(const uint8_t *__restrict__ scratch, const ZaTbxLine *__restrict__ lines, const uint32_t *__restrict__ di,
                                                      const unsigned long long *__restrict__ n_data, uint64_t n, uint64_t line_base,
                                                      unsigned long long *__restrict__ f_name, unsigned long long *__restrict__ f_bin,
                                                      ZaTbxState *__restrict__ st)
{
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, nd = *n_data;
    if (d >= n) return;
    if (d >= nd) { f_name[d] = 0; f_bin[d] = 0; return; }
    const ZaTbxLine L = lines[di[d]];
    bool name_new = true, bin_new = true;
    if (d) {
        const ZaTbxLine P = lines[di[d - 1u]];
        name_new = !za_tbx_same_name(scratch, L, P);
        bin_new = name_new || za_tbx_reg2bin(L.beg, L.end) != za_tbx_reg2bin(P.beg, P.end);
        if (!name_new && L.beg < P.beg) atomicMin(&st->bad_key, (unsigned long long)(line_base + di[d]) << 3 | (ZA_TBX_BAD_ORDER - ZA_TBX_SKIP));
    } else { st->first_line = line_base + di[0]; st->first_src = L.start; st->first_beg = L.beg; }
    if (d == nd - 1ull) st->last_beg = L.beg;
    if (name_new) atomicAdd(&st->name_bytes, (unsigned long long)L.name_len);
    f_name[d] = name_new ? 1ull : 0ull; f_bin[d] = bin_new ? 1ull : 0ull;
}

// s_name: the inclusive sums of f_name.  (end - 1) >> 14 is below 2^15: the name run stands above it, and the runs ascend
__global__ __launch_bounds__(256) void za_k_tbx_keys(const ZaTbxLine *__restrict__ lines, const uint32_t *__restrict__ di, const unsigned long long *__restrict__ n_data,
                                                     uint64_t n, const unsigned long long *__restrict__ s_name, unsigned long long *__restrict__ key)
{
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    if (d >= *n_data) { key[d] = 0; return; }
    key[d] = (s_name[d] - 1ull) << 15 | ((lines[di[d]].end - 1u) >> 14);
}

__global__ __launch_bounds__(256) void za_k_tbx_raise(const unsigned long long *__restrict__ m_key, const unsigned long long *__restrict__ n_data, uint64_t n,
                                                      unsigned long long *__restrict__ f_raise)
{
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n) return;
    f_raise[d] = d < *n_data && (d == 0 || m_key[d] > m_key[d - 1u]) ? 1ull : 0ull;
}

// the tables: a row where the inclusive sums step.  The capacities are those the host has seen in the totals.
__global__ __launch_bounds__(256) void za_k_tbx_emit(const ZaTbxLine *__restrict__ lines, const uint32_t *__restrict__ di, uint64_t nd, uint64_t line_base,
                                                     const unsigned long long *__restrict__ s_name, const unsigned long long *__restrict__ s_bin,
                                                     const unsigned long long *__restrict__ m_key, const unsigned long long *__restrict__ s_raise,
                                                     ZaTbxName *__restrict__ names, uint64_t names_cap, uint32_t *__restrict__ name_lens,
                                                     ZaTbxBin *__restrict__ bins, uint64_t bins_cap, ZaTbxWin *__restrict__ wins, uint64_t wins_cap)
{
    const uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    const ZaTbxLine L = lines[di[d]];
    const unsigned long long a = s_name[d], b = s_bin[d], w = s_raise[d];
    if (a != (d ? s_name[d - 1u] : 0ull) && a - 1ull < names_cap) {
        ZaTbxName r; r.src_off = L.start + L.name_rel; r.first = d; r.line = line_base + di[d]; r.len = L.name_len; r.reserved = 0;
        names[a - 1ull] = r; name_lens[a - 1ull] = L.name_len;
    }
    if (b != (d ? s_bin[d - 1u] : 0ull) && b - 1ull < bins_cap) {
        ZaTbxBin r; r.src_beg = L.start; r.src_end = 0; r.first = d; r.lines = 0; r.name = (uint32_t)(a - 1ull); r.bin = za_tbx_reg2bin(L.beg, L.end);
        bins[b - 1ull] = r;
    }
    if (w != (d ? s_raise[d - 1u] : 0ull) && w - 1ull < wins_cap) {
        ZaTbxWin r; r.src_off = L.start; r.name = (uint32_t)(a - 1ull); r.window = (uint32_t)(m_key[d] & 0x7FFFull);
        wins[w - 1ull] = r;
    }
}

// a bin run ends where the next one begins
__global__ __launch_bounds__(256) void za_k_tbx_finish(ZaTbxBin *__restrict__ bins, uint64_t nb, const ZaTbxLine *__restrict__ lines,
                                                       const uint32_t *__restrict__ di, uint64_t nd)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nb) return;
    const uint64_t first = bins[r].first, next = r + 1u < nb ? bins[r + 1u].first : nd;
    if (next <= first || next > nd) return;
    const ZaTbxLine L = lines[di[next - 1u]];
    bins[r].lines = next - first; bins[r].src_end = L.start + L.len;
}

__global__ __launch_bounds__(256) void za_k_tbx_place(const ZaTbxName *__restrict__ names, const uint64_t *__restrict__ offs, uint64_t n, ZaBgzfSlice *__restrict__ slices)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ZaBgzfSlice s; s.src_off = names[i].src_off; s.dst_off = offs[i]; s.len = names[i].len; s.reserved = 0;
    slices[i] = s;
}

__global__ __launch_bounds__(256) void za_k_tbx_place_rows(const ZaTbxRow *__restrict__ rows, const uint64_t *__restrict__ offs, uint64_t n, ZaBgzfSlice *__restrict__ slices)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ZaBgzfSlice s; s.src_off = rows[i].src_off; s.dst_off = offs[i]; s.len = rows[i].len; s.reserved = 0;
    slices[i] = s;
}

// ---- the region filter.  grid: one workgroup per span.  EMIT false: span_status[s], span_rows[s] and *bytes; EMIT true: the rows of
// span s from rows[span_base[s]] on and their lengths.  The spans and the member table are untrusted; the regions were judged on the host.
template <bool EMIT>
__global__ __launch_bounds__(256) void za_k_tbx_fetch(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, const ZaMember *__restrict__ members,
                                                      const int32_t *__restrict__ member_status, uint32_t n_members, const ZaTbxSpan *__restrict__ spans,
                                                      const ZaTbxRegion *__restrict__ regions, uint32_t n_regions, const uint8_t *__restrict__ blob,
                                                      ZaTbxConf cf, uint32_t delim, int32_t *__restrict__ span_status, uint32_t *__restrict__ span_rows,
                                                      unsigned long long *__restrict__ bytes, const uint64_t *__restrict__ span_base,
                                                      ZaTbxRow *__restrict__ rows, uint64_t rows_cap, uint32_t *__restrict__ lens)
{
    __shared__ int s_verdict;
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x;
    const ZaTbxSpan sp = spans[blockIdx.x];
    if (tid == 0) {
        int v = ZA_SLICE_OK;
        if (sp.text_off > sp.text_end || sp.text_end > scratch_cap || sp.text_end - sp.text_off >= (1ull << 32) || sp.region >= n_regions) v = ZA_SLICE_TABLE;
        else if (sp.text_end > sp.text_off) {         // members that decoded cover the span without a gap (as za_k_slice_gather judges a slice)
            uint32_t lo = 0, hi = n_members;
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (members[mid].out_off <= sp.text_off) lo = mid + 1; else hi = mid; }
            v = ZA_SLICE_BLOCK;
            if (lo > 0) {
                uint64_t at = sp.text_off;
                for (uint32_t m = lo - 1; m < n_members; m++) {
                    const ZaMember mm = members[m];
                    if (mm.out_off > at || member_status[m] != ZA_I_OK || !za_member_in_scratch(mm, scratch_cap)) break;
                    if (mm.out_off + mm.out_len > at) at = mm.out_off + mm.out_len;
                    if (at >= sp.text_end) { v = ZA_SLICE_OK; break; }
                }
            }
        }
        s_verdict = v;
        if (!EMIT) span_status[blockIdx.x] = v;
    }
    __syncthreads();
    if (s_verdict != ZA_SLICE_OK) { if (!EMIT && tid == 0) span_rows[blockIdx.x] = 0; return; }      // (the same for every thread)
    const ZaTbxRegion rg = regions[sp.region];
    const uint64_t lo = sp.text_off, hi = sp.text_end;
    uint64_t run = EMIT ? span_base[blockIdx.x] : 0ull;
    unsigned long long nbytes = 0;
    uint32_t nrows = 0;
    for (uint64_t base = lo & ~63ull; base < hi; base += ZA_TBX_TILE) {      // (the same trips for every thread)
        const uint64_t w0 = base + tid * 64u;
        uint64_t S = za_tbx_word_mask(scratch, scratch_cap, w0, lo, hi, delim) << 1;      // a line starts behind a delimiter; the one
        if (w0 > lo && w0 < hi && scratch[w0 - 1u] == delim) S |= 1ull;                   // behind the word's last byte is the next word's
        if (lo >= w0 && lo - w0 < 64u) S |= 1ull << (lo - w0);
        if (w0 >= hi) S = 0; else if (hi - w0 < 64u) S &= (1ull << (hi - w0)) - 1ull;
        uint64_t sel = 0;
        uint32_t cnt = 0;
        for (uint64_t t = S; t; t &= t - 1ull) {
            const uint32_t b = (uint32_t)__builtin_ctzll(t);
            ZaTbxLine L;
            bool term;
            za_tbx_parse(scratch, w0 + b, hi, delim, cf, ~0ull, L, term);
            if (L.kind != ZA_TBX_DATA || L.name_len != rg.name_len || L.beg >= rg.end || L.end <= rg.beg) continue;
            const uint8_t *x = scratch + L.start + L.name_rel, *y = blob + rg.name_off;
            uint32_t i = 0;
            while (i < L.name_len && x[i] == y[i]) i++;
            if (i != L.name_len) continue;
            sel |= 1ull << b; cnt++; nbytes += L.len;
        }
        uint32_t all;
        const uint32_t ex = za_tbx_wg_excl(cnt, s_w, &all);
        if (EMIT) {
            uint64_t idx = run + ex;
            for (uint64_t t = sel; t; t &= t - 1ull) {
                const uint32_t b = (uint32_t)__builtin_ctzll(t);
                ZaTbxLine L;
                bool term;
                za_tbx_parse(scratch, w0 + b, hi, delim, cf, ~0ull, L, term);
                if (idx < rows_cap) { ZaTbxRow r; r.src_off = L.start; r.len = L.len; r.region = sp.region; rows[idx] = r; lens[idx] = L.len; }
                idx++;
            }
        }
        run += all; nrows += cnt;
    }
    if (!EMIT) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) nbytes += __shfl_xor(nbytes, d, 64);
        if ((tid & 63u) == 0 && nbytes) atomicAdd(bytes, nbytes);
        if (tid == 0) span_rows[blockIdx.x] = (uint32_t)run;
    }
}

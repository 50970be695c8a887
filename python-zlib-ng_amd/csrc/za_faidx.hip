// BGZF by sequence: the records of a FASTA.  The decoded blocks lie in the scratch as one byte string, as for
// za_tabix.hip.  No thread walks a line: the text is read once, 64 bytes per thread, and everything behind that is work per line.
//   the index build (zngamd_bgzf_faidx), over the text scratch[text_off, text_end) in tiles of 16 KiB:
//     za_k_fai_mark      one thread per 64 bytes: the '\n' bits of its word and the bits of its bytes outside 0x21 .. 0x7E (without the
//                        terminators); per tile the number of '\n'
//     (za_k_offsets)     '\n' in front of every tile
//     za_k_fai_starts    one thread per 64 bytes: line k of the text starts behind its k-th '\n' (line 0: at text_off)
//     za_k_fai_bytes     one thread per 64 bytes, idle unless its word holds a bad byte: per line that crosses the word, is it a
//                        sequence line?
//     za_k_fai_classify  one thread per line: bases, width, header or not; three arrays for the scans
//     (za_k_tbx_reduce / _scan_blocks / _apply)    headers, non-empty sequence lines and bases up to every line, inclusive
//     za_k_fai_heads     one thread per line: header number r writes where it stands and how long its name is
//     za_k_fai_ends      one thread per line: the first and the last non-empty line of every record say so
//     za_k_fai_judge     one thread per line: the line against the first non-empty line of its record (the head of the window:
//                        against the carry)
//     za_k_fai_close     one thread: what the carry left to judge, the carry for the next window, the totals
//     za_k_fai_emit      one thread per header: its row;  za_k_offsets, za_k_fai_place and za_k_slice_gather pack the names
//   the gather (zngamd_bgzf_faidx_fetch): za_k_fai_gather, one workgroup per span, copies bases line by line without the terminators,
//     reverse-complemented on request.
// Included by zng_amd.hip behind za_tabix.hip (za_eq_mask, za_mask_nibble, za_tbx_wg_excl, ZaBgzfSlice, ZA_TBX_TILE).
#include "za_common.h"

#define ZA_FAI_FINAL    4u             // flags of the build: mirrors ZNGAMD_BGZF_FAIDX_FINAL
#define ZA_FAI_RC       1u             // flags of a span: mirrors ZNGAMD_FAIDX_SPAN_RC
#define ZA_FAI_MAX_SPAN 65536u         // bases per span at most: mirrors ZNGAMD_FAIDX_MAX_SPAN
#define ZA_SLICE_STALE  4              // a gathered byte is no printable character: the index belongs to another file
#define ZA_FAI_OPEN     1u             // flags of a carry
#define ZA_FAI_GAP      2u
#define ZA_FAI_NONE     0xFFFFFFFFu
#define ZA_FAI_BAD_NAME  1u            // the kinds of a bad line, in the issue's order
#define ZA_FAI_BAD_BYTE  2u
#define ZA_FAI_BAD_WIDTH 3u
#define ZA_FAI_BAD_BLANK 4u
#define ZA_FAI_BAD_LOOSE 5u

struct ZaFaiCarry { uint64_t last_line; uint32_t first_bases, first_width, last_bases, last_width, flags, reserved; };      // mirrors zngamd_faidx_carry
struct ZaFaiRow { uint64_t name_src, seq_src, line, bases; uint32_t name_len, line_bases, line_width, reserved; };          // mirrors zngamd_faidx_row
struct ZaFaiSpan { uint64_t src_off, dst_off; uint32_t n, col, line_bases, line_width, flags, reserved; };                  // mirrors zngamd_faidx_span
struct ZaFaiState {                    // what the kernels of one build leave for the host (device memory, 88 B)
    unsigned long long bad_key;        // smallest (line number << 3 | kind) of a bad line; ~0: none
    unsigned long long tail_off, name_bytes, head_bases, seen, records;
    ZaFaiCarry out;
    uint32_t head_fb, head_fw;         // the head's first non-empty line where the carry has none: the open sequence's first line
};

// 0x80 in the bytes of x outside 0x21 .. 0x7E.  Exact per byte: t <= 0x7F, so neither sum leaves its byte.
__device__ __forceinline__ uint32_t za_fai_unprintable(uint32_t x)
{
    const uint32_t t = x & 0x7f7f7f7fu;
    return (x | ~(t + 0x5f5f5f5fu) | (t + 0x01010101u)) & 0x80808080u;      // the top bit, below 0x21, 0x7F
}

// of scratch[w0, w0 + 64) inside [lo, hi) (hi <= scratch_cap): D the '\n' bits, X the bytes outside 0x21 .. 0x7E that are neither a
// '\n' nor the CR in front of one.  16-byte loads where the scratch has them.
__device__ __forceinline__ void za_fai_word(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t w0, uint64_t lo, uint64_t hi,
                                            uint64_t &D, uint64_t &X)
{
    D = 0; X = 0;
    if (w0 >= hi || (lo > w0 && lo - w0 >= 64u)) return;
    uint64_t R = 0, U = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint64_t g = w0 + 16u * k;
        if (g >= hi) break;
        uint32_t d, r, u;
        if (scratch_cap - g >= 16u) {
            const ZaU4u v = *(const ZaU4u *)(scratch + g);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            d = r = u = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                d |= za_mask_nibble(za_eq_mask(w[j], 0x0a0a0a0au)) << (4u * j);
                r |= za_mask_nibble(za_eq_mask(w[j], 0x0d0d0d0du)) << (4u * j);
                u |= za_mask_nibble(za_fai_unprintable(w[j])) << (4u * j);
            }
        } else {
            d = r = u = 0;
            for (uint32_t j = 0; j < (uint32_t)(scratch_cap - g); j++) {
                const uint32_t ch = scratch[g + j];
                d |= (ch == 10u ? 1u : 0u) << j; r |= (ch == 13u ? 1u : 0u) << j; u |= ((ch < 0x21u || ch > 0x7eu) ? 1u : 0u) << j;
            }
        }
        D |= (uint64_t)d << (16u * k); R |= (uint64_t)r << (16u * k); U |= (uint64_t)u << (16u * k);
    }
    uint64_t in = ~0ull;
    if (lo > w0) in &= ~((1ull << (lo - w0)) - 1ull);
    if (hi - w0 < 64u) in &= (1ull << (hi - w0)) - 1ull;
    D &= in;
    uint64_t next = D >> 1;                               // the byte behind is a '\n' of the text
    if ((R >> 63) && hi - w0 > 64u && scratch[w0 + 64u] == 10u) next |= 1ull << 63;
    X = U & in & ~D & ~(R & next);
}

// grid: one workgroup per tile, tile0 + blockIdx.x
__global__ __launch_bounds__(256) void za_k_fai_mark(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, uint64_t text_off, uint64_t text_end,
                                                     uint64_t tile0, unsigned long long *__restrict__ bits, unsigned long long *__restrict__ xbits,
                                                     uint32_t *__restrict__ tile_cnt)
{
    __shared__ uint32_t s_w[4];
    const uint64_t w0 = (tile0 + blockIdx.x) * (uint64_t)ZA_TBX_TILE + threadIdx.x * 64u;
    uint64_t D, X;
    za_fai_word(scratch, scratch_cap, w0, text_off, text_end, D, X);
    bits[(size_t)blockIdx.x * 256u + threadIdx.x] = D;
    xbits[(size_t)blockIdx.x * 256u + threadIdx.x] = X;
    uint32_t all;
    (void)za_tbx_wg_excl((uint32_t)__popcll(D), s_w, &all);
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = all;
}

// grid: one workgroup per tile.  start[] has room for the text's '\n' + 2 entries: start[k] is where line k begins, k = 0 .. the
// number of '\n'; the entry behind them is text_end + 1, so that every line ends one byte in front of the next entry.
__global__ __launch_bounds__(256) void za_k_fai_starts(uint64_t text_off, uint64_t text_end, uint64_t tile0, const unsigned long long *__restrict__ bits,
                                                       const uint64_t *__restrict__ tile_base, uint64_t n_delim, uint64_t *__restrict__ start)
{
    __shared__ uint32_t s_w[4];
    const uint64_t w0 = (tile0 + blockIdx.x) * (uint64_t)ZA_TBX_TILE + threadIdx.x * 64u;
    uint64_t D = bits[(size_t)blockIdx.x * 256u + threadIdx.x];
    uint32_t all;
    uint64_t ord = tile_base[blockIdx.x] + za_tbx_wg_excl((uint32_t)__popcll(D), s_w, &all);      // '\n' in front of this word
    if (text_off >= w0 && text_off - w0 < 64u) { start[0] = text_off; start[n_delim + 1ull] = text_end + 1ull; }
    while (D) {
        const uint32_t b = (uint32_t)__builtin_ctzll(D);
        D &= D - 1ull;
        if (++ord <= n_delim) start[ord] = w0 + b + 1ull;
    }
}

// grid: one workgroup per tile.  n_judged: the lines of this call (the open tail is not one of them).
__global__ __launch_bounds__(256) void za_k_fai_bytes(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ bits,
                                                      const unsigned long long *__restrict__ xbits, const uint64_t *__restrict__ tile_base,
                                                      const uint64_t *__restrict__ start, uint64_t n_judged, uint64_t line_base, ZaFaiState *__restrict__ st)
{
    __shared__ uint32_t s_w[4];
    uint64_t D = bits[(size_t)blockIdx.x * 256u + threadIdx.x];
    const uint64_t X = xbits[(size_t)blockIdx.x * 256u + threadIdx.x];
    uint32_t all;
    uint64_t k = tile_base[blockIdx.x] + za_tbx_wg_excl((uint32_t)__popcll(D), s_w, &all);      // the line that is open where the word begins
    if (!X) return;
    uint64_t done = 0;                                    // the bits of the lines in front
    for (;;) {
        const uint64_t upto = D ? ((D & (0ull - D)) << 1) - 1ull : ~0ull;      // through this line's '\n'
        if ((X & upto & ~done) && k < n_judged) {
            const uint64_t s = start[k];
            if (s < text_end && scratch[s] != '>') atomicMin(&st->bad_key, (unsigned long long)(line_base + k) << 3 | ZA_FAI_BAD_BYTE);
        }
        if (!D) break;
        done = upto; D &= D - 1ull; k++;
    }
}

// one thread per entry of the arrays (n_lines of them); lines at or behind n_judged write zeros.  bw: bases | width << 32.
__global__ __launch_bounds__(256) void za_k_fai_classify(const uint8_t *__restrict__ scratch, uint64_t text_off, uint64_t text_end,
                                                         const uint64_t *__restrict__ start, uint64_t n_delim, uint64_t n_judged, uint64_t n_lines,
                                                         uint64_t line_base, unsigned long long *__restrict__ hdr, unsigned long long *__restrict__ ne,
                                                         unsigned long long *__restrict__ bs, unsigned long long *__restrict__ bw, ZaFaiState *__restrict__ st)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_lines) return;
    unsigned long long h = 0, n = 0, b = 0, w = 0;
    if (k < n_judged) {
        const uint64_t s = start[k], e = start[k + 1u] - 1ull;                  // e: the line's '\n', or text_end
        if (s >= text_off && s <= e && e <= text_end) {
            const bool term = k < n_delim;
            const uint64_t be = e - ((term && e > s && scratch[e - 1u] == 13u) ? 1u : 0u);
            const uint32_t bases = (uint32_t)(be - s), width = (uint32_t)(e - s) + (term ? 1u : 0u);
            const bool header = bases && scratch[s] == '>';
            if (header) {
                const uint32_t c = bases > 1u ? scratch[s + 1u] : 32u;
                if (c == 32u || c == 9u || c == 13u) atomicMin(&st->bad_key, (unsigned long long)(line_base + k) << 3 | ZA_FAI_BAD_NAME);
            }
            h = header ? 1ull : 0ull; n = (!header && bases) ? 1ull : 0ull; b = header ? 0ull : bases; w = (unsigned long long)bases | (unsigned long long)width << 32;
        }
    }
    hdr[k] = h; ne[k] = n; bs[k] = b; bw[k] = w;
}

// H: the inclusive sums of hdr.  Header number r (from 1) writes hline[r - 1] and the length of its name: from the byte behind '>' to
// the first space, tab or CR or to the end of the body -- the one walk over bytes here, and it ends with the name.
__global__ __launch_bounds__(256) void za_k_fai_heads(const uint8_t *__restrict__ scratch, const uint64_t *__restrict__ start,
                                                      const unsigned long long *__restrict__ H, const unsigned long long *__restrict__ bw, uint64_t n_judged,
                                                      uint32_t *__restrict__ hline, uint32_t *__restrict__ name_len, ZaFaiState *__restrict__ st)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_judged) return;
    const unsigned long long r = H[k];
    if (r == (k ? H[k - 1u] : 0ull)) return;
    const uint64_t s = start[k] + 1ull;
    const uint32_t body = (uint32_t)bw[k] - 1u;
    uint32_t n = 0;
    while (n < body) { const uint32_t c = scratch[s + n]; if (c == 32u || c == 9u || c == 13u) break; n++; }
    hline[r - 1ull] = (uint32_t)k; name_len[r - 1ull] = n;
    if (n) atomicAdd(&st->name_bytes, (unsigned long long)n);
}

// the non-empty sequence lines in front of record r's end (r = 0: the head of the window, the lines in front of its first header)
__device__ __forceinline__ unsigned long long za_fai_nend(const unsigned long long *__restrict__ N, const uint32_t *__restrict__ hline, uint64_t r, uint64_t nrec,
                                                          unsigned long long ntot, uint64_t n_judged)
{
    if (r >= nrec) return ntot;
    const uint32_t h = hline[r];
    return h < n_judged ? N[h] : ntot;
}

// N: the inclusive sums of ne.  first[r] / last[r], r = 0 .. records: the first and the last non-empty line of record r (the host
// has set them to ZA_FAI_NONE).  tot: [0] records, [1] non-empty sequence lines, [2] bases.
__global__ __launch_bounds__(256) void za_k_fai_ends(const unsigned long long *__restrict__ H, const unsigned long long *__restrict__ N,
                                                     const uint32_t *__restrict__ hline, uint64_t n_judged, const unsigned long long *__restrict__ tot,
                                                     uint32_t *__restrict__ first, uint32_t *__restrict__ last)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_judged) return;
    const unsigned long long n = N[k];
    if (n == (k ? N[k - 1u] : 0ull)) return;
    const uint64_t r = H[k], nrec = tot[0];
    const unsigned long long front = r ? za_fai_nend(N, hline, r - 1u, nrec, tot[1], n_judged) : 0ull;
    if (n == front + 1ull) first[r] = (uint32_t)k;
    if (n == za_fai_nend(N, hline, r, nrec, tot[1], n_judged)) last[r] = (uint32_t)k;
}

__global__ __launch_bounds__(256) void za_k_fai_judge(const unsigned long long *__restrict__ H, const unsigned long long *__restrict__ N,
                                                      const unsigned long long *__restrict__ bw, const uint32_t *__restrict__ hline,
                                                      const uint32_t *__restrict__ first, uint64_t n_judged, uint64_t line_base, uint32_t flags,
                                                      const unsigned long long *__restrict__ tot, const ZaFaiCarry *__restrict__ in, ZaFaiState *__restrict__ st)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_judged) return;
    const uint64_t r = H[k], nrec = tot[0];
    if (r != (k ? H[k - 1u] : 0ull)) return;              // a header: judged where it was classified
    const ZaFaiCarry ci = *in;
    const uint32_t bases = (uint32_t)bw[k], width = (uint32_t)(bw[k] >> 32);
    uint32_t kind = 0;
    if (!r && !(ci.flags & ZA_FAI_OPEN)) kind = bases ? ZA_FAI_BAD_LOOSE : 0u;
    else {
        const unsigned long long nend = za_fai_nend(N, hline, r, nrec, tot[1], n_judged);
        if (!bases) kind = N[k] < nend ? ZA_FAI_BAD_BLANK : 0u;
        else {
            const bool carried = !r && ci.first_width;     // the record's first non-empty line lies in a window in front
            const uint32_t f = first[r];
            uint32_t fb = ci.first_bases, fw = ci.first_width;
            if (!carried && f < n_judged) { fb = (uint32_t)bw[f]; fw = (uint32_t)(bw[f] >> 32); }
            if (carried || f != (uint32_t)k) {
                if (N[k] != nend) kind = (bases != fb || width != fw) ? ZA_FAI_BAD_WIDTH : 0u;
                else if (r < nrec || (flags & ZA_FAI_FINAL)) kind = bases > fb ? ZA_FAI_BAD_WIDTH : 0u;
                // else: the window's last non-empty line; the next call judges it through the carry
            }
        }
    }
    if (kind) atomicMin(&st->bad_key, (unsigned long long)(line_base + k) << 3 | kind);
}

// grid: one thread.  B: the inclusive sums of bs.
__global__ void za_k_fai_close(const unsigned long long *__restrict__ N, const unsigned long long *__restrict__ B, const unsigned long long *__restrict__ bw,
                               const uint64_t *__restrict__ start, const uint32_t *__restrict__ hline, const uint32_t *__restrict__ first,
                               const uint32_t *__restrict__ last, uint64_t n_delim, uint64_t n_judged, uint64_t text_off, uint64_t text_end,
                               uint64_t line_base, uint32_t flags, const unsigned long long *__restrict__ tot, const ZaFaiCarry *__restrict__ in,
                               ZaFaiState *__restrict__ st)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t nrec = n_judged ? tot[0] : 0ull;
    const unsigned long long ntot = n_judged ? tot[1] : 0ull, btot = n_judged ? tot[2] : 0ull;
    const ZaFaiCarry ci = *in;
    const bool open = ci.flags & ZA_FAI_OPEN, final = flags & ZA_FAI_FINAL;
    const uint32_t h0 = nrec ? hline[0] : 0u;
    const bool h0ok = nrec && h0 < n_judged;
    const unsigned long long nhead = h0ok ? N[h0] : ntot;
    st->head_bases = !open ? 0ull : h0ok ? B[h0] : btot;      // (without an open sequence those lines are faults, or empty)
    st->seen = n_judged; st->records = nrec;
    { const uint32_t f0 = (open && !ci.first_width) ? first[0] : ZA_FAI_NONE;
      st->head_fb = f0 < n_judged ? (uint32_t)bw[f0] : 0u; st->head_fw = f0 < n_judged ? (uint32_t)(bw[f0] >> 32) : 0u; }
    st->tail_off = (!final && n_judged == n_delim && text_end > text_off && start[n_delim] < text_end) ? start[n_delim] : text_end;
    if (open) {                                           // what the windows in front left undecided
        unsigned long long key = ~0ull;
        if (nhead) {                                      // the carried last line is a middle line
            if (ci.first_width && (ci.last_bases != ci.first_bases || ci.last_width != ci.first_width)) key = ci.last_line << 3 | ZA_FAI_BAD_WIDTH;
            if (ci.flags & ZA_FAI_GAP) { const unsigned long long g = (ci.last_line + 1ull) << 3 | ZA_FAI_BAD_BLANK; if (g < key) key = g; }
        } else if ((nrec || final) && ci.first_width && ci.last_bases > ci.first_bases) key = ci.last_line << 3 | ZA_FAI_BAD_WIDTH;
        if (key != ~0ull) atomicMin(&st->bad_key, key);
    }
    ZaFaiCarry co;
    co.last_line = 0; co.first_bases = co.first_width = co.last_bases = co.last_width = co.flags = co.reserved = 0;
    if (!final && (nrec || open)) {
        uint64_t idx;                                     // the record's last non-empty line, or its header
        bool have = true;
        if (nrec) {
            co.flags = ZA_FAI_OPEN;
            const uint32_t h = hline[nrec - 1u];
            idx = h < n_judged ? h : 0u;
        } else {
            co = ci;
            idx = 0; have = false;
            if (n_judged) co.flags |= ntot ? 0u : ZA_FAI_GAP;      // (with a non-empty line the gap is judged anew below)
        }
        const uint32_t f = (nrec || !ci.first_width) ? first[nrec] : ZA_FAI_NONE, l = last[nrec];
        if (f < n_judged) { co.first_bases = (uint32_t)bw[f]; co.first_width = (uint32_t)(bw[f] >> 32); }
        if (l < n_judged) { co.last_bases = (uint32_t)bw[l]; co.last_width = (uint32_t)(bw[l] >> 32); idx = l; have = true; }
        if (have) {
            co.last_line = line_base + idx;
            co.flags = ZA_FAI_OPEN | (idx + 1u < n_judged ? ZA_FAI_GAP : 0u);
            const uint64_t nx = start[idx + 1u] < text_end ? start[idx + 1u] : text_end;
            co.reserved = (uint32_t)(nx - text_off);      // where the line behind it starts, from text_off
        }
    }
    st->out = co;
}

// one thread per header, r = 0 .. records - 1; rows at or behind rows_cap are not written
__global__ __launch_bounds__(256) void za_k_fai_emit(const uint64_t *__restrict__ start, const unsigned long long *__restrict__ B, const unsigned long long *__restrict__ bw,
                                                     const uint32_t *__restrict__ hline, const uint32_t *__restrict__ first, const uint32_t *__restrict__ name_len,
                                                     uint64_t nrec, uint64_t n_judged, uint64_t text_end, uint64_t line_base, unsigned long long btot,
                                                     ZaFaiRow *__restrict__ rows, uint64_t rows_cap)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrec || r >= rows_cap) return;
    const uint32_t h = hline[r];
    if (h >= n_judged) return;
    ZaFaiRow o;
    o.name_src = start[h] + 1ull; o.name_len = name_len[r];
    o.seq_src = start[h + 1u] < text_end ? start[h + 1u] : text_end;
    o.line = line_base + h;
    const uint32_t hn = r + 1u < nrec ? hline[r + 1u] : ZA_FAI_NONE;
    o.bases = (hn < n_judged ? B[hn] : btot) - B[h];
    const uint32_t f = first[r + 1u];
    o.line_bases = f < n_judged ? (uint32_t)bw[f] : 0u; o.line_width = f < n_judged ? (uint32_t)(bw[f] >> 32) : 0u;
    o.reserved = 0;
    rows[r] = o;
}

__global__ __launch_bounds__(256) void za_k_fai_place(const ZaFaiRow *__restrict__ rows, const uint64_t *__restrict__ offs, uint64_t n, ZaBgzfSlice *__restrict__ slices)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    ZaBgzfSlice s; s.src_off = rows[i].name_src; s.dst_off = offs[i]; s.len = rows[i].name_len; s.reserved = 0;
    slices[i] = s;
}

// ---- the gather.  IUPAC complement of an ASCII letter, in its case; everything else unchanged
__device__ __forceinline__ uint32_t za_fai_complement(uint32_t c)
{
    uint32_t r;
    switch (c & ~32u) {                                   // (equals an upper-case letter only for that letter in either case)
        case 'A': r = 'T'; break; case 'T': r = 'A'; break; case 'U': r = 'A'; break; case 'C': r = 'G'; break; case 'G': r = 'C'; break;
        case 'R': r = 'Y'; break; case 'Y': r = 'R'; break; case 'K': r = 'M'; break; case 'M': r = 'K'; break;
        case 'B': r = 'V'; break; case 'V': r = 'B'; break; case 'D': r = 'H'; break; case 'H': r = 'D'; break;
        default: return c;
    }
    return r | (c & 32u);
}

// grid: one workgroup per span.  Base k of the span, q = col + k, lies at src_off - col + (q / line_bases) * line_width + q %
// line_bases: one division per thread, then steps of 256 bases as whole lines and a rest.  The spans and the member table are
// untrusted: the last base's place is computed first, in 64 bits (q / line_bases <= 65 536), and judged against the scratch.
__global__ __launch_bounds__(256) void za_k_fai_gather(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, const ZaMember *__restrict__ members,
                                                       const int32_t *__restrict__ member_status, uint32_t n_members, const ZaFaiSpan *__restrict__ spans,
                                                       uint8_t *__restrict__ out, uint64_t out_cap, int32_t *__restrict__ span_status)
{
    __shared__ int s_verdict;
    __shared__ uint8_t s_comp[256];
    const uint32_t tid = threadIdx.x;
    const ZaFaiSpan sp = spans[blockIdx.x];
    s_comp[tid] = (uint8_t)za_fai_complement(tid);
    if (tid == 0) {
        int v = ZA_SLICE_OK;
        if (sp.n > ZA_FAI_MAX_SPAN || !sp.line_bases || sp.line_width < sp.line_bases || sp.col >= sp.line_bases || sp.src_off < sp.col ||
            sp.src_off > scratch_cap || sp.dst_off > out_cap || out_cap - sp.dst_off < sp.n) v = ZA_SLICE_TABLE;
        else if (sp.n) {
            const uint64_t q = (uint64_t)sp.col + sp.n - 1u;
            const uint64_t reach = (q / sp.line_bases) * sp.line_width + q % sp.line_bases - sp.col;      // the last base, from src_off
            if (scratch_cap - sp.src_off <= reach) v = ZA_SLICE_TABLE;
            else {                                        // members that decoded cover the bytes without a gap (the walk of za_k_slice_gather)
                uint32_t lo = 0, hi = n_members;
                while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (members[mid].out_off <= sp.src_off) lo = mid + 1; else hi = mid; }
                v = ZA_SLICE_BLOCK;
                if (lo > 0) {
                    uint64_t at = sp.src_off;
                    const uint64_t end = sp.src_off + reach + 1ull;
                    for (uint32_t m = lo - 1; m < n_members; m++) {
                        const ZaMember mm = members[m];
                        if (mm.out_off > at || member_status[m] != ZA_I_OK || !za_member_in_scratch(mm, scratch_cap)) break;
                        if (mm.out_off + mm.out_len > at) at = mm.out_off + mm.out_len;
                        if (at >= end) { v = ZA_SLICE_OK; break; }
                    }
                }
            }
        }
        s_verdict = v;
    }
    __syncthreads();
    const int verdict = s_verdict;                        // (the same for every thread)
    int stale = 0;
    if (verdict == ZA_SLICE_OK && sp.n) {
        const uint32_t lb = sp.line_bases, lw = sp.line_width, step_l = 256u / lb, step_r = 256u % lb;
        const bool rc = sp.flags & ZA_FAI_RC;
        const uint64_t q0 = (uint64_t)sp.col + tid;
        uint64_t line = q0 / lb;
        uint32_t rest = (uint32_t)(q0 % lb);
        const uint8_t *base = scratch + (sp.src_off - sp.col);
        uint8_t *d = out + sp.dst_off;
        for (uint32_t k = tid; k < sp.n; k += 256u) {
            const uint32_t c = base[line * lw + rest];
            stale |= (c < 0x21u || c > 0x7eu) ? 1 : 0;
            if (rc) d[sp.n - 1u - k] = s_comp[c]; else d[k] = (uint8_t)c;
            line += step_l; rest += step_r;
            if (rest >= lb) { rest -= lb; line++; }
        }
    } else if (verdict == ZA_SLICE_BLOCK) {
        for (uint32_t k = tid; k < sp.n; k += 256u) out[sp.dst_off + k] = 0;      // never the bytes of a block that failed
    }
    stale = __syncthreads_or(stale);
    if (tid == 0) span_status[blockIdx.x] = verdict == ZA_SLICE_OK && stale ? ZA_SLICE_STALE : verdict;
}

// Span decoder of a seek-point index (zlib_ng_amd/gzip_index.py): one 64-lane wavefront per span of a gzip member's deflate data.
// A span starts at a block header (absolute bit in_bit) with the 32 KiB of output in front of it as its dictionary and ends at a
// later block header (end_bit, a stop of the sequential core) or where its member's final block ends (end_bit = that end rounded
// up to a byte, the rule of za_k_inflate_serial_members).  After the decode the wave checks the CRC-32 of the span's output
// against the one the index recorded.  Same LDS layout and occupancy as za_k_inflate_serial_members: what makes a file with an
// index decode like a file of independent members.  Product code; included by zng_amd.hip behind za_inflate.hip.
#pragma once

struct ZaSpan {                      // zngamd_span
    uint64_t in_bit, end_bit;        // absolute bits in the input buffer: first block header, end (see above)
    uint64_t win_off, out_off;       // byte offsets into the windows array and the output
    uint32_t win_len, out_len;       // dictionary bytes (<= 32 768), output bytes
    uint32_t crc, reserved;          // CRC-32 of the span's output
};

#define ZA_SPAN_OK     0
#define ZA_SPAN_DATA   1             // invalid deflate data, a table entry out of bounds, or the decode did not stop at end_bit
#define ZA_SPAN_LENGTH 2             // stopped at end_bit with another output length
#define ZA_SPAN_CRC    3
#define ZA_SPAN_PAD    64            // bytes the input buffer must hold behind the end of every span

__global__ __launch_bounds__(64) void za_k_inflate_spans(const uint8_t *__restrict__ in, uint64_t in_len,
                                                         const ZaSpan *__restrict__ spans,
                                                         const uint8_t *__restrict__ windows, uint64_t windows_len,
                                                         uint8_t *__restrict__ out, uint64_t out_cap,
                                                         const uint32_t *__restrict__ crc_table,
                                                         const uint32_t *__restrict__ x8k_table,
                                                         int32_t *__restrict__ status_out)
{
    __shared__ ZaInfTabsT<ZA_MEMBER_LBITS, ZA_MEMBER_DBITS> T;
    __shared__ uint8_t win[ZA_MEMBER_RING];
    __shared__ int scratch[2];
    __shared__ ZaParBufT<ZA_MEMBER_BITS, ZA_MEMBER_Q> P;
    uint32_t *crct = P.stage;                      // the CRC table takes the staged stream's place once the span is decoded
    const int lane = za_lane();
    const ZaSpan s = spans[blockIdx.x];
    // the table is untrusted: every offset is checked before a byte is read or written (the end_bit / in_bit arithmetic cannot
    // wrap: in_len is a buffer size, far below 2^61)
    const uint64_t first = s.in_bit >> 3, last = (s.end_bit + 7) >> 3;
    if (s.in_bit > s.end_bit || last + ZA_SPAN_PAD > in_len || last - first > in_len || s.win_len > ZA_WIN ||
        s.win_off > windows_len || windows_len - s.win_off < s.win_len || s.out_off > out_cap || out_cap - s.out_off < s.out_len) {
        if (lane == 0) status_out[blockIdx.x] = ZA_SPAN_DATA;
        return;
    }
    const uint8_t *src = in + first;
    uint8_t *dst = out + s.out_off;
    const uint64_t stop = s.end_bit;
    uint64_t bits = 0, op = 0;
    int status = za_inflate_serial_core<0, uint8_t, ZA_MEMBER_RING, ZaParBufT<ZA_MEMBER_BITS, ZA_MEMBER_Q>>(src, last - first, windows + s.win_off, s.win_len,
                                                                       dst, s.out_len, T, win, scratch, P.stage, bits, op, (uint32_t)(s.in_bit & 7u),
                                                                       nullptr, nullptr, 0xFFFFFFFFu, false, nullptr, &stop, 1u, first * 8ull, &P);
    if (status == ZA_I_SYNC || status == ZA_I_END) {
        // SYNC: stopped at the block header end_bit names; END: the member's final block ended, which must be end_bit too
        const uint64_t at = first * 8ull + bits;
        if (status == ZA_I_END ? ((at + 7) & ~7ull) != s.end_bit : at != s.end_bit) status = ZA_SPAN_DATA;
        else if (op != s.out_len) status = ZA_SPAN_LENGTH;
        else {
            __threadfence_block();
            __syncthreads();
            for (int i = lane; i < 256; i += 64) crct[i] = crc_table[i];
            __syncthreads();
            uint32_t crc = 0;
            for (uint64_t o = 0; o < op; o += ZA_MAX_UNIT) {
                const int len = (int)((op - o) > ZA_MAX_UNIT ? ZA_MAX_UNIT : (op - o));
                const uint32_t c = za_wave_crc32(dst + o, len, crct, x8k_table);
                uint32_t xp = 0x80000000u, sq = 0x00800000u;            // crc = crc * x^(8 len) ^ c
                for (int k = len; k; k >>= 1) { if (k & 1) xp = za_multmodp(sq, xp); sq = za_multmodp(sq, sq); }
                crc = za_multmodp(xp, crc) ^ c;
            }
            status = crc == s.crc ? ZA_SPAN_OK : ZA_SPAN_CRC;
        }
    } else status = status == ZA_I_OUTFULL ? ZA_SPAN_LENGTH : ZA_SPAN_DATA;
    if (lane == 0) status_out[blockIdx.x] = status;
}

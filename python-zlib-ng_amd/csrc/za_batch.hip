// Batch API (zlib_ng_amd/batch.py): many independent small streams per call, one 64-lane wavefront per item, all items in one
// launch.  Product code; included by zng_amd.hip behind za_inflate.hip and za_deflate.hip.
//   za_k_inflate_batch<COUNT>  parses the item's container (zlib / gzip / raw, or auto per item), decodes its deflate data with
//                              za_inflate_serial_core (the decoder of za_k_inflate_serial_members, same LDS layout and occupancy)
//                              and checks its trailer on the wave.  COUNT = 1: the same walk and checks, nothing stored; the
//                              result's out_len is the exact output size (items whose first decode ran out of room).
//   za_k_inflate_batch_dict<COUNT>  the same with one shared preset dictionary (zdict): a zlib item with FDICT whose DICTID is the
//                              dictionary's Adler-32 and every raw item decode with its tail as history; a wrong DICTID is
//                              ZA_ZDICT_MISMATCH.  Same body (za_inflate_batch_item<COUNT, true>), same LDS, occupancy and scratch.
//   za_k_batch_prime           compress side with a dictionary: [dictionary tail][item] for every item into a staging buffer, so
//                              that the deflate pipeline runs one block per item with the tail as its dict_len.
//   za_k_batch_frame           compress side, after za_k_pack: header, the item's deflate bytes, Adler-32 (worked out from the
//                              item's input) or CRC-32 (folded from its units' CRCs) and ISIZE, at the item's place in one output.
// The item table is untrusted (device callers pass device tables): every offset and length is checked before a byte is read or
// written; an entry outside the buffers gets ZA_BATCH_TABLE.
#pragma once

struct ZaBatchItem {                 // zngamd_batch_item
    uint64_t in_off, out_off;
    uint32_t in_len, out_cap;
    uint32_t reserved[2];
};
struct ZaBatchResult {               // zngamd_batch_result
    int32_t status;
    uint32_t out_len, in_used, reserved;
};

#define ZA_BATCH_OK        0
#define ZA_BATCH_TRUNCATED 1         // Z_BUF_ERROR: the stream or its trailer needs bytes beyond the item
#define ZA_BATCH_OUTFULL   2         // out_cap reached (not an error: the count pass sizes the item)
#define ZA_BATCH_NEED_DICT 3
#define ZA_BATCH_HEADER    4         // incorrect header check
#define ZA_BATCH_WINDOW    5         // invalid window size
#define ZA_BATCH_METHOD    6         // unknown compression method
#define ZA_BATCH_FLAGS     7         // unknown header flags set
#define ZA_BATCH_HCRC      8         // header crc mismatch
#define ZA_BATCH_DATA      9         // invalid deflate data
#define ZA_BATCH_CHECK     10        // incorrect data check (Adler-32 / CRC-32)
#define ZA_BATCH_LENGTH    11        // incorrect length check (ISIZE)
#define ZA_BATCH_TABLE     12        // the table entry lies outside the buffers
#define ZA_ZDICT_MISMATCH  13        // a zlib item's DICTID is not the Adler-32 of the call's dictionary
#define ZA_BATCH_PAD       64        // readable bytes the input buffer must hold behind in_len

// containers (the host maps the call's wbits onto these)
#define ZA_BATCH_RAW  0
#define ZA_BATCH_ZLIB 1
#define ZA_BATCH_GZIP 2
#define ZA_BATCH_AUTO 3

// Adler-32 of n bytes on one wavefront (all lanes call with uniform arguments): rounds of 64 KiB, a lane per KiB, the lane's byte
// sum a and running-sum sum b (dwords through v_dot4_u32_u8, as za_k_checksum), folded with the bytes behind each lane's piece.
__device__ __forceinline__ uint32_t za_wave_adler32(const uint8_t *data, uint64_t n)
{
    const int lane = za_lane();
    unsigned long long A = 0, B = 0;
    for (uint64_t r = 0; r < n; r += 65536) {
        const uint64_t s0 = r + ((uint64_t)lane << 10);
        uint32_t a = 0, b = 0;
        uint64_t after = 0;
        if (s0 < n) {
            const uint64_t s1 = s0 + 1024 < n ? s0 + 1024 : n;
            const uint8_t *p = data + s0, *e = data + s1;
            for (; p < e && (((uintptr_t)p) & 3u); p++) { a += *p; b += a; }
            for (; p + 4 <= e; p += 4) {
                const uint32_t v = *(const uint32_t *)p;
                b += 4u * a + __builtin_amdgcn_udot4(v, 0x01020304u, 0u, false);      // the dword's first byte is its lowest: weight 4
                a = __builtin_amdgcn_udot4(v, 0x01010101u, a, false);
            }
            for (; p < e; p++) { a += *p; b += a; }
            after = n - s1;
        }
        A += a;
        B += ((unsigned long long)b + (after % 65521ull) * a) % 65521ull;
    }
    for (int d = 32; d >= 1; d >>= 1) { A += __shfl_xor(A, d, 64); B += __shfl_xor(B, d, 64); }
    const uint32_t a = (uint32_t)((1ull + A) % 65521ull);
    const uint32_t b = (uint32_t)(((n % 65521ull) + B) % 65521ull);
    return (b << 16) | a;
}

// CRC-32 of n bytes (any length) on one wavefront: za_wave_crc32 per 128 KiB, folded.  crct: the 256-entry table in LDS.
__device__ __forceinline__ uint32_t za_wave_crc32_any(const uint8_t *data, uint64_t n, const uint32_t *crct, const uint32_t *__restrict__ x8k)
{
    uint32_t crc = 0;
    for (uint64_t o = 0; o < n; o += ZA_MAX_UNIT) {
        const int len = (int)((n - o) > ZA_MAX_UNIT ? ZA_MAX_UNIT : (n - o));
        const uint32_t c = za_wave_crc32(data + o, len, crct, x8k);
        uint32_t xp = 0x80000000u, sq = 0x00800000u;            // crc = crc * x^(8 len) ^ c
        for (int k = len; k; k >>= 1) { if (k & 1) xp = za_multmodp(sq, xp); sq = za_multmodp(sq, sq); }
        crc = za_multmodp(xp, crc) ^ c;
    }
    return crc;
}

// first NUL byte in [from, n) of p, or n when there is none (wave-uniform)
__device__ __forceinline__ uint64_t za_wave_find_nul(const uint8_t *p, uint64_t from, uint64_t n)
{
    const int lane = za_lane();
    for (uint64_t q = from; q < n; q += 64) {
        const bool z = q + (uint64_t)lane < n && p[q + (uint64_t)lane] == 0;
        const unsigned long long m = __ballot(z);
        if (m) return q + (uint64_t)__builtin_ctzll(m);
    }
    return n;
}

// One item of za_k_inflate_batch[_dict].  DICT: dict / dict_len = the dictionary's kept tail (device), dictid = its Adler-32.
template <int COUNT, bool DICT>
__device__ __forceinline__ void za_inflate_batch_item(const uint8_t *__restrict__ in, uint64_t in_len,
                                                      const ZaBatchItem *__restrict__ items,
                                                      uint8_t *__restrict__ out, uint64_t out_cap,
                                                      const uint32_t *__restrict__ crc_table,
                                                      const uint32_t *__restrict__ x8k_table,
                                                      int kind0, int wmax,
                                                      ZaBatchResult *__restrict__ results,
                                                      const uint8_t *__restrict__ dict, uint32_t dict_len, uint32_t dictid)
{
    __shared__ ZaInfTabsT<ZA_MEMBER_LBITS, ZA_MEMBER_DBITS> T;
    __shared__ uint8_t win[ZA_MEMBER_RING];
    __shared__ int scratch[2];
    __shared__ ZaParBufT<ZA_MEMBER_BITS, ZA_MEMBER_Q> P;
    uint32_t *crct = P.stage;                      // the CRC table takes the staged stream's place before and after the decode
    const int lane = za_lane();
    const ZaBatchItem it = items[blockIdx.x];
    ZaBatchResult res; res.status = ZA_BATCH_TABLE; res.out_len = 0; res.in_used = 0; res.reserved = 0;
    if (it.in_off > in_len || in_len - it.in_off < it.in_len || (!COUNT && (it.out_off > out_cap || out_cap - it.out_off < it.out_cap))) {
        if (lane == 0) results[blockIdx.x] = res;
        return;
    }
    const uint8_t *src = in + it.in_off;
    const uint64_t n = it.in_len;
    int kind = kind0;
    if (kind == ZA_BATCH_AUTO) kind = (n >= 2 && src[0] == 0x1f && src[1] == 0x8b) ? ZA_BATCH_GZIP : ZA_BATCH_ZLIB;
    // ---- the container's header (the order of checks is zlib_ng.decompress's)
    int st = ZA_BATCH_OK;
    uint64_t hdr = 0;
    bool use_dict = DICT && kind == ZA_BATCH_RAW;     // a raw item has the dictionary as history from its first byte, a gzip item never
    if (kind == ZA_BATCH_ZLIB) {
        if (n < 2) st = ZA_BATCH_TRUNCATED;
        else {
            const uint32_t cmf = src[0], flg = src[1];
            const uint32_t win_bits = (cmf >> 4) + 8;
            if ((cmf & 15u) != 8u || ((cmf << 8) | flg) % 31u) st = ZA_BATCH_HEADER;
            else if (win_bits > 15 || (wmax != 0 && win_bits > (uint32_t)wmax)) st = ZA_BATCH_WINDOW;
            else if (flg & 0x20u) {
                if constexpr (DICT) {
                    if (n < 6) st = ZA_BATCH_TRUNCATED;              // the item ends inside its DICTID
                    else if (((uint32_t)src[2] << 24 | (uint32_t)src[3] << 16 | (uint32_t)src[4] << 8 | src[5]) != dictid) st = ZA_ZDICT_MISMATCH;
                    else use_dict = true;
                } else st = ZA_BATCH_NEED_DICT;
            }
            hdr = 2;
            if constexpr (DICT) if (use_dict) hdr = 6;
        }
    } else if (kind == ZA_BATCH_GZIP) {
        if (n < 10) st = ZA_BATCH_TRUNCATED;
        else if (src[0] != 0x1f || src[1] != 0x8b) st = ZA_BATCH_HEADER;
        else if (src[2] != 8) st = ZA_BATCH_METHOD;
        else if (src[3] & 0xE0u) st = ZA_BATCH_FLAGS;
        else {
            const uint32_t flags = src[3];
            uint64_t cur = 10;
            if (flags & 4u) {
                if (cur + 2 >= n) st = ZA_BATCH_TRUNCATED;
                else {
                    cur += 2 + ((uint32_t)src[cur] | ((uint32_t)src[cur + 1] << 8));
                    if (cur >= n) st = ZA_BATCH_TRUNCATED;
                }
            }
            for (uint32_t bit = 8; bit <= 16 && st == ZA_BATCH_OK; bit <<= 1) {
                if (!(flags & bit)) continue;
                const uint64_t z = za_wave_find_nul(src, cur, n);
                if (z >= n) st = ZA_BATCH_TRUNCATED;
                else cur = z + 1;
            }
            if (st == ZA_BATCH_OK && (flags & 2u)) {
                if (cur + 2 >= n) st = ZA_BATCH_TRUNCATED;
                else {
                    for (int i = lane; i < 256; i += 64) crct[i] = crc_table[i];
                    __syncthreads();
                    const uint32_t got = za_wave_crc32_any(src, cur, crct, x8k_table) & 0xFFFFu;
                    const uint32_t want = (uint32_t)src[cur] | ((uint32_t)src[cur + 1] << 8);
                    __syncthreads();
                    if (got != want) st = ZA_BATCH_HCRC;
                    cur += 2;
                }
            }
            hdr = cur;
        }
    }
    if (st != ZA_BATCH_OK) {
        res.status = st;
        if (lane == 0) results[blockIdx.x] = res;
        return;
    }
    // ---- the deflate data: only the item's own bytes (a stream that needs more is truncated, whatever follows in the buffer)
    uint64_t bits = 0, op = 0;
    int status;
    const uint8_t *hd = nullptr;
    uint32_t hl = 0;
    if constexpr (DICT) if (use_dict) { hd = dict; hl = dict_len; }
    if (COUNT)
        status = za_inflate_serial_core<1, uint8_t, ZA_MEMBER_RING, ZaParBufT<ZA_MEMBER_BITS, ZA_MEMBER_Q>>(src + hdr, n - hdr, hd, hl, nullptr, 0xFFFFFFFFull, T, nullptr, scratch, P.stage,
                                                                       bits, op, 0, nullptr, nullptr, 0xFFFFFFFFu, false, nullptr, nullptr, 0, 0, &P);
    else
        status = za_inflate_serial_core<0, uint8_t, ZA_MEMBER_RING, ZaParBufT<ZA_MEMBER_BITS, ZA_MEMBER_Q>>(src + hdr, n - hdr, hd, hl, out + it.out_off, it.out_cap, T, win, scratch, P.stage,
                                                                       bits, op, 0, nullptr, nullptr, 0xFFFFFFFFu, false, nullptr, nullptr, 0, 0, &P);
    res.out_len = (uint32_t)op;
    if (status == ZA_I_END) {
        const uint64_t used = hdr + ((bits + 7) >> 3);
        const uint64_t tl = kind == ZA_BATCH_ZLIB ? 4 : kind == ZA_BATCH_GZIP ? 8 : 0;
        res.in_used = (uint32_t)(used + tl);
        if (n - used < tl) st = ZA_BATCH_TRUNCATED;
        else if (!COUNT && kind == ZA_BATCH_ZLIB) {
            __threadfence_block();
            __syncthreads();
            const uint32_t want = ((uint32_t)src[used] << 24) | ((uint32_t)src[used + 1] << 16) | ((uint32_t)src[used + 2] << 8) | src[used + 3];
            if (za_wave_adler32(out + it.out_off, op) != want) st = ZA_BATCH_CHECK;
        } else if (!COUNT && kind == ZA_BATCH_GZIP) {
            __threadfence_block();
            __syncthreads();
            for (int i = lane; i < 256; i += 64) crct[i] = crc_table[i];
            __syncthreads();
            const uint32_t crc = za_wave_crc32_any(out + it.out_off, op, crct, x8k_table);
            const uint32_t want_crc = za_ld32(src + used), want_len = za_ld32(src + used + 4);
            if (crc != want_crc) st = ZA_BATCH_CHECK;
            else if (want_len != (uint32_t)op) st = ZA_BATCH_LENGTH;
        }
    } else st = status == ZA_I_OUTFULL ? ZA_BATCH_OUTFULL : status == ZA_I_INPUT ? ZA_BATCH_TRUNCATED : ZA_BATCH_DATA;
    res.status = st;
    if (lane == 0) results[blockIdx.x] = res;
}

template <int COUNT>
__global__ __launch_bounds__(64) void za_k_inflate_batch(const uint8_t *__restrict__ in, uint64_t in_len,
                                                         const ZaBatchItem *__restrict__ items,
                                                         uint8_t *__restrict__ out, uint64_t out_cap,
                                                         const uint32_t *__restrict__ crc_table,
                                                         const uint32_t *__restrict__ x8k_table,
                                                         int kind0, int wmax,
                                                         ZaBatchResult *__restrict__ results)
{
    za_inflate_batch_item<COUNT, false>(in, in_len, items, out, out_cap, crc_table, x8k_table, kind0, wmax, results, nullptr, 0u, 0u);
}

template <int COUNT>
__global__ __launch_bounds__(64) void za_k_inflate_batch_dict(const uint8_t *__restrict__ in, uint64_t in_len,
                                                              const ZaBatchItem *__restrict__ items,
                                                              uint8_t *__restrict__ out, uint64_t out_cap,
                                                              const uint32_t *__restrict__ crc_table,
                                                              const uint32_t *__restrict__ x8k_table,
                                                              int kind0, int wmax,
                                                              ZaBatchResult *__restrict__ results,
                                                              const uint8_t *__restrict__ dict, uint32_t dict_len, uint32_t dictid)
{
    za_inflate_batch_item<COUNT, true>(in, in_len, items, out, out_cap, crc_table, x8k_table, kind0, wmax, results, dict, dict_len, dictid);
}

// n bytes from src to dst on one wavefront: the stores are whole aligned 16-byte pieces of dst (a few single bytes in front of the
// first and behind the last), each lane assembling its piece from five aligned dwords of src (v_alignbyte).  src must be readable
// up to 20 bytes past n (ZA_BATCH_PAD behind the input, 64 behind the dictionary).
__device__ __forceinline__ void za_wave_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, uint64_t n)
{
    const int lane = za_lane();
    const uint64_t h0 = (16u - ((uintptr_t)dst & 15u)) & 15u, h = h0 < n ? h0 : n;
    if ((uint64_t)lane < h) dst[lane] = src[lane];
    dst += h; src += h; n -= h;
    const uint32_t sh = (uint32_t)((uintptr_t)src & 3u);
    const uint32_t *s4 = (const uint32_t *)(src - sh);
    const uint64_t nv = n >> 4;
    for (uint64_t k = (uint64_t)lane; k < nv; k += 64) {
        const uint32_t *p = s4 + 4 * k;
        const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
        uint4 v;
        v.x = __builtin_amdgcn_alignbyte(w1, w0, sh); v.y = __builtin_amdgcn_alignbyte(w2, w1, sh);
        v.z = __builtin_amdgcn_alignbyte(w3, w2, sh); v.w = __builtin_amdgcn_alignbyte(w4, w3, sh);
        *(uint4 *)(dst + 16 * k) = v;
    }
    for (uint64_t k = (nv << 4) + (uint64_t)lane; k < n; k += 64) dst[k] = src[k];
}

// Compress side with a dictionary: item i (in_off, in_len of the host-built table; out_off = the place of its record in `prime`)
// becomes [the tail's tl bytes][the item] at out_off.  The records start on 64-byte boundaries, as a stream's staged buffer does.
__global__ __launch_bounds__(64) void za_k_batch_prime(const uint8_t *__restrict__ in, uint64_t in_len, const ZaBatchItem *__restrict__ items,
                                                       uint32_t n, const uint8_t *__restrict__ tail, uint32_t tl,
                                                       uint8_t *__restrict__ prime, uint64_t prime_cap)
{
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const ZaBatchItem it = items[i];
    // (the host checked the table; a record outside the buffers is left alone, and the deflate of that block is garbage, not a fault)
    if (it.in_off > in_len || in_len - it.in_off < it.in_len || it.out_off > prime_cap || prime_cap - it.out_off < (uint64_t)tl + it.in_len) return;
    uint8_t *dst = prime + it.out_off;
    za_wave_copy(dst, tail, tl);
    za_wave_copy(dst + tl, in + it.in_off, it.in_len);
}

// The compress side's framing.  Items are packed by za_k_pack unit after unit, so item i's deflate bytes run from the offset of its
// first unit to that of the next item's first unit (or the stream's end): the units' prefix sum (za_k_offsets) places them, and
// with a header and trailer of the same size for every item (ovh bytes), item i lands at that offset + i * ovh.
struct ZaBatchFrameHdr { uint8_t b[16]; };
__global__ __launch_bounds__(64) void za_k_batch_frame(const uint8_t *__restrict__ in, ZaBatchItem *__restrict__ items, uint32_t n,
                                                       const uint32_t *__restrict__ first_unit, uint32_t n_units,
                                                       const uint64_t *__restrict__ unit_off, const uint32_t *__restrict__ unit_crc,
                                                       const uint64_t *__restrict__ def_total, const uint8_t *__restrict__ packed,
                                                       int kind, ZaBatchFrameHdr head, uint32_t head_len,
                                                       uint8_t *__restrict__ out, uint64_t out_cap, ZaBatchResult *__restrict__ results)
{
    const int lane = za_lane();
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const ZaBatchItem it = items[i];
    const uint32_t u0 = first_unit[i], u1 = first_unit[i + 1];
    const uint32_t ovh = head_len + (kind == ZA_BATCH_ZLIB ? 4u : kind == ZA_BATCH_GZIP ? 8u : 0u);
    const uint64_t d0 = unit_off[u0], d1 = u1 < n_units ? unit_off[u1] : *def_total;
    const uint64_t dlen = d1 - d0, o = d0 + (uint64_t)i * ovh, olen = dlen + ovh;
    ZaBatchResult res; res.status = ZA_BATCH_OK; res.out_len = (uint32_t)olen; res.in_used = it.in_len; res.reserved = 0;
    if (d1 < d0 || o > out_cap || out_cap - o < olen) {
        res.status = ZA_BATCH_TABLE;
        if (lane == 0) results[i] = res;
        return;
    }
    uint8_t *dst = out + o;
    for (uint32_t k = (uint32_t)lane; k < head_len; k += 64) dst[k] = head.b[k];
    const uint8_t *s = packed + d0;
    for (uint64_t k = (uint64_t)lane; k < dlen; k += 64) dst[head_len + k] = s[k];
    uint8_t *t = dst + head_len + dlen;
    if (kind == ZA_BATCH_ZLIB) {
        const uint32_t a = za_wave_adler32(in + it.in_off, it.in_len);
        if (lane < 4) t[lane] = (uint8_t)(a >> (24 - 8 * lane));
    } else if (kind == ZA_BATCH_GZIP) {
        // the units' CRCs folded in order: crc = crc * x^(8 len) ^ crc(unit); units of 16 KiB for an item of up to 128 KiB, else 128 KiB
        const uint64_t U = it.in_len <= ZA_MAX_UNIT ? ZA_SMALL_UNIT : ZA_MAX_UNIT;
        uint32_t crc = 0;
        for (uint32_t u = u0; u < u1; u++) {
            const uint64_t rel = (uint64_t)(u - u0) * U;
            const uint64_t len = rel >= it.in_len ? 0 : (it.in_len - rel < U ? it.in_len - rel : U);
            uint32_t xp = 0x80000000u, sq = 0x00800000u;
            for (uint64_t k = len; k; k >>= 1) { if (k & 1) xp = za_multmodp(sq, xp); sq = za_multmodp(sq, sq); }
            crc = za_multmodp(xp, crc) ^ unit_crc[u];
        }
        const uint32_t w[2] = {crc, it.in_len};
        if (lane < 8) t[lane] = (uint8_t)(w[lane >> 2] >> (8 * (lane & 3)));
    }
    if (lane == 0) { items[i].out_off = o; results[i] = res; }
}

// The default writer's stream -- ONE deflate stream of dict-chained, sync-flushed units (gzip_ng_threaded.py:299-338) -- decoded with
// the writer's own segment index: the member decoder's lane-per-segment phase A (the same code: za_mem_tables and za_mem_phase_a
// in za_inflate.hip, called by both kernels) and an in-order phase B like the member decoder's, on 16-bit symbols, so
// that the units need not wait for each other (a source in front of a unit is a marker; the chunk pipeline's window kernels
// -- za_k_chunk_compose / _chain / _resolve -- turn markers into bytes).  Product code; included by zng_amd.hip behind za_inflate.hip.
//
// The unit's stream must be what this engine writes for full-size units (or with ZA_FLAG_FLATHDR for smaller ones): one block per
// unit -- stored blocks, fixed, or dynamic with the header in either form --, token boundaries at every 2 KiB of output, codes of at
// most 10 / 9 bits; the index = cidx of za_k_pack.  Anything else is reported (ZA_I_INDEX) and the caller decodes the stream
// without the index.
#pragma once

__global__ __launch_bounds__(64, 5) void za_k_inflate_units_marked(const uint8_t *__restrict__ in, uint64_t in_total,
                                                                   const ZaMember *__restrict__ members,     // per unit: in_off / in_len = its bytes in the stream (sync marker included), out_off = first symbol of its AREA in out16, out_len, crc = bytes of history in front of it (<= 32 768), nseg
                                                                   uint16_t *__restrict__ out16, uint64_t out_cap,     // symbols
                                                                   uint32_t *__restrict__ matchq,            // [grid][64][ZA_MATCHQ_PER_SEG]
                                                                   const uint32_t *__restrict__ ext_index,   // [grid][ZA_CIDX_STRIDE]: the units' segment indices (what za_k_pack left in cidx)
                                                                   ZaChunkRes *__restrict__ res_out)
{
#define ZA_UM_FAIL(code) do { if (lane == 0) { ZaChunkRes r_; r_.status = (code); r_.max_back = 0; r_.bits = 0; r_.out_len = 0; res_out[blockIdx.x] = r_; } return; } while (0)
    __shared__ ZaMemTabs T;
    __shared__ int scratch[2];
    __shared__ __attribute__((aligned(16))) uint32_t rows[64 * ZA_IROW];      // table build: ZaMemBuild; phase A: staged input; then the CRC table
    static_assert(sizeof(ZaMemBuild) <= sizeof(uint32_t) * 64 * ZA_IROW, "build area");
    ZaMemBuild &B = *(ZaMemBuild *)rows;
    const int lane = za_lane();
    const ZaMember m = members[blockIdx.x];
    const uint8_t *src = in + m.in_off;
    const uint64_t in_bits = m.in_len * 8ull;
    // area coordinates: symbol 0 of the area is the first of the 32 768 marker symbols in front of the unit, so that no source
    // position is ever negative and a source in front of the unit is read like any other far source
    uint16_t *dst16 = out16 + m.out_off;
    const uint32_t hist = m.crc;                                      // (the field's role here)
    const int n = (int)m.out_len;
    const int nseg = (int)m.nseg;
    if (m.in_off + m.in_len > in_total || m.out_off + ZA_WIN + (uint64_t)m.out_len > out_cap || n > ZA_MAX_UNIT || m.in_len > (1u << 20) ||
        nseg != ((n + ZA_SEG - 1) >> ZA_SEG_SHIFT) || hist > (uint32_t)ZA_WIN) ZA_UM_FAIL(ZA_I_INDEX);
    if (n == 0) {
        // a unit the index calls EMPTY must be what za_k_pack writes for no input: the sync marker alone (an empty stored block,
        // 00 00 00 FF FF) or, as the stream's last block, 03 00 -- anything else holds bytes that the index would hide.  (The host
        // puts these units behind the batch's others: no area, no queue, no index row is theirs, and none is touched.)
        const bool sync = m.in_len == 5u && src[0] == 0u && za_ld32(src + 1) == 0xFFFF0000u;
        const bool fin = m.in_len == 2u && src[0] == 0x03u && src[1] == 0u;
        if (!sync && !fin) ZA_UM_FAIL(ZA_I_INDEX);
        if (lane == 0) { ZaChunkRes r; r.status = fin ? ZA_I_END : ZA_I_SYNC; r.max_back = 0; r.bits = (m.in_off + m.in_len) * 8ull; r.out_len = 0; res_out[blockIdx.x] = r; }
        return;
    }
    const uint32_t *index = ext_index + (size_t)blockIdx.x * ZA_CIDX_STRIDE;
    if (index[nseg] == 0u) {
        // a unit of STORED blocks (what the packer writes for input that does not compress; its index is all zeros): blocks of at
        // most 65 535 bytes, each `BFINAL | 00`, LEN, ~LEN, bytes, on byte boundaries -- and the sync marker behind the last
        const uint32_t nblk = ((uint32_t)n + 65534u) / 65535u;
        uint32_t at = 0;
        bool ok = true, fin = false;
        for (uint32_t c = 0; c < nblk && ok; c++) {
            const uint32_t len = (uint32_t)n - 65535u * c > 65535u ? 65535u : (uint32_t)n - 65535u * c;
            if ((uint64_t)at + 5u + len > m.in_len) { ok = false; break; }
            const uint32_t h = src[at], l = za_ld16(src + at + 1), nl = za_ld16(src + at + 3);
            fin = (h & 1u) != 0u;
            ok = (h & 0xFEu) == 0u && l == len && nl == (~len & 0xFFFFu) && (!fin || c + 1 == nblk);
            const uint8_t *pb = src + at + 5;
            uint16_t *ps = dst16 + ZA_WIN + 65535u * c;
            const uint32_t full = len & ~7u;
            for (uint32_t i = 8u * (uint32_t)lane; i < full; i += 8u * 64u) {
                const ZaU2u w = *(const ZaU2u *)(pb + i);
                ZaU4u v;
                v.x = __builtin_amdgcn_perm(0u, w.x, 0x0C010C00u); v.y = __builtin_amdgcn_perm(0u, w.x, 0x0C030C02u);
                v.z = __builtin_amdgcn_perm(0u, w.y, 0x0C010C00u); v.w = __builtin_amdgcn_perm(0u, w.y, 0x0C030C02u);
                *(ZaU4u *)(ps + i) = v;
            }
            for (uint32_t i = full + (uint32_t)lane; i < len; i += 64) ps[i] = pb[i];
            at += 5u + len;
        }
        if (ok) ok = fin ? (uint64_t)at == m.in_len : ((uint64_t)at + 5u == m.in_len && src[at] == 0u && za_ld32(src + at + 1) == 0xFFFF0000u);
        if (!ok) ZA_UM_FAIL(ZA_I_INDEX);
        if (lane == 0) { ZaChunkRes r; r.status = fin ? ZA_I_END : ZA_I_SYNC; r.max_back = 0; r.bits = (m.in_off + m.in_len) * 8ull; r.out_len = (uint64_t)n; res_out[blockIdx.x] = r; }
        return;
    }
    // index entries: bit offset | overshoot << 23; at this granularity (one entry per 2 KiB segment, where the codec forces a
    // token boundary) the overshoot is zero
    const uint32_t my_start = za_ld32((const uint8_t *)(index + (lane < nseg ? lane : nseg)));
    const uint32_t my_stop = za_ld32((const uint8_t *)(index + (lane < nseg ? lane + 1 : nseg)));
    if (__ballot((my_start >> 23) != 0u || (my_stop >> 23) != 0u) != 0ull || in_bits < 3) ZA_UM_FAIL(ZA_I_INDEX);
    // (the block header, the tables and phase A are the member decoder's: za_mem_tables and za_mem_phase_a in za_inflate.hip)
    int last;
    if (za_mem_tables<true>(src, in_bits, __shfl(my_start, 0, 64), T, B, scratch, last) != ZA_I_OK) ZA_UM_FAIL(ZA_I_INDEX);

    // ---- phase A (za_mem_phase_a): the literal bytes go to the front of the segment's own 4 KiB of symbols -- twice its bytes, so
    // the open block always fits --, and a match may reach the `hist` bytes in front of the unit
    uint32_t nmatch, nlit;
    int lane_err;
    za_mem_phase_a<true>(in, in_total, src, in_bits, m.in_len, my_start, my_stop, n, nseg, rows, T,
                         matchq + ((size_t)blockIdx.x * 64 + (size_t)lane) * ZA_MATCHQ_PER_SEG, (uint8_t *)(dst16 + ZA_WIN + (lane << ZA_SEG_SHIFT)), hist, last,
                         nlit, nmatch, lane_err);
    const unsigned long long e1 = __ballot(lane_err == 1), e2 = __ballot(lane_err == 2);
    if (e1 || e2) ZA_UM_FAIL(e2 ? ZA_I_DATA : ZA_I_INDEX);
    __threadfence_block();       // the literal bytes and the match queues are visible to the whole wave

    // ---- phase B: expand, segment by segment, as za_k_inflate_members does -- but every symbol is 16 bits wide (a byte, or
    // 256 + j = "byte j of the 32 KiB in front of this unit", which nobody knows yet), kept as TWO BYTE PLANES: the low bytes in
    // the row area, the high bytes where the decode tables stood.  A copy moves the same offsets of both planes, so the index
    // arithmetic, the dependency masks and the tail handling are the member decoder's; literals have a zero high byte (the high
    // plane of a segment starts as zeros and only matches write it).  Positions are AREA coordinates (unit position + 32 768): a
    // source in front of the unit is a far source like any other and reads marker symbols, which an initialisation kernel put in
    // front of every unit's symbols once.  No CRC here: the bytes are not known until the windows are.
    // Kept as an implementation of its own (only the masked store, za_put32, is shared): one image there against two planes here,
    // a CRC there against none, the ablation switches of the far sources and of the CRC there only -- shared code would branch on
    // its caller at every store.
    {
        uint8_t *img = (uint8_t *)rows;                            // [0, 272): symbols in front of the segment, [272, 272 + 2048): the segment -- low bytes
        uint8_t *imh = (uint8_t *)&T;                              // ... high bytes
        const uint32_t TAIL = 272u, AB = (uint32_t)ZA_WIN;
        static_assert(sizeof(uint32_t) * 64 * ZA_IROW >= 272 + ZA_SEG + 32, "low plane");
        static_assert(sizeof(ZaMemTabs) >= 272 + ZA_SEG + 32, "high plane");
        __builtin_amdgcn_wave_barrier();
        // the 272 symbols in front of the unit: markers
        for (uint32_t i = (uint32_t)lane; i < TAIL; i += 64) { const uint32_t sy = 256u + (AB - TAIL + i); img[i] = (uint8_t)sy; imh[i] = (uint8_t)(sy >> 8); }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // 16 symbols at dst16 + a -> their low and high bytes
        auto ld_syms = [&](uint32_t a, ZaU4u &lo, ZaU4u &hi) {
            const ZaU4u d0 = *(const ZaU4u *)(dst16 + a), d1 = *(const ZaU4u *)(dst16 + a + 8);
            lo.x = __builtin_amdgcn_perm(d0.y, d0.x, 0x06040200u); lo.y = __builtin_amdgcn_perm(d0.w, d0.z, 0x06040200u);
            lo.z = __builtin_amdgcn_perm(d1.y, d1.x, 0x06040200u); lo.w = __builtin_amdgcn_perm(d1.w, d1.z, 0x06040200u);
            hi.x = __builtin_amdgcn_perm(d0.y, d0.x, 0x07050301u); hi.y = __builtin_amdgcn_perm(d0.w, d0.z, 0x07050301u);
            hi.z = __builtin_amdgcn_perm(d1.y, d1.x, 0x07050301u); hi.w = __builtin_amdgcn_perm(d1.w, d1.z, 0x07050301u);
        };
        for (int s = 0; s < nseg; s++) {
            const uint32_t cnt = __shfl(nmatch, s, 64), lits = __shfl(nlit, s, 64);
            const uint32_t *q = matchq + ((size_t)blockIdx.x * 64 + (size_t)s) * ZA_MATCHQ_PER_SEG;
            const uint32_t seg_start = AB + ((uint32_t)s << ZA_SEG_SHIFT);
            const uint32_t seg_len = (uint32_t)n - ((uint32_t)s << ZA_SEG_SHIFT) < (uint32_t)ZA_SEG ? (uint32_t)n - ((uint32_t)s << ZA_SEG_SHIFT) : (uint32_t)ZA_SEG;
            uint32_t ent_next = (uint32_t)lane < cnt ? q[lane] : 0u;
            // images: the tail of the previous segment moves to the front (final symbols); the literal BYTES come from the front of
            // the segment's own symbol area, piece by piece of 16 where a piece holds any (image byte x is literal byte x - shift)
            __builtin_amdgcn_wave_barrier();
            uint32_t t0 = 0, t1 = 0, u0 = 0, u1 = 0;
            if (s > 0) {
                t0 = ((const uint32_t *)(img + ZA_SEG))[lane]; u0 = ((const uint32_t *)(imh + ZA_SEG))[lane];
                if (lane < 4) { t1 = ((const uint32_t *)(img + ZA_SEG))[64 + lane]; u1 = ((const uint32_t *)(imh + ZA_SEG))[64 + lane]; }
            }
            {
                const int shift = (int)(seg_len - lits);             // match symbols of the segment
                const uint8_t *litb = (const uint8_t *)(dst16 + seg_start);
                ZaU4u pc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    const int x = lane * 32 + 16 * j, o = x - shift;
                    // (bytes in front of the first literal or behind the last are of no meaning; they are readable: the area in front is
                    // the segment before or the marker symbols, the area behind is this segment's own 4 KiB)
                    if (x < (int)seg_len && o + 16 > 0) pc[j] = *(const ZaU4u *)(litb + o);
                }
                __builtin_amdgcn_wave_barrier();
                if (s > 0) {
                    ((uint32_t *)img)[lane] = t0; ((uint32_t *)imh)[lane] = u0;
                    if (lane < 4) { ((uint32_t *)img)[64 + lane] = t1; ((uint32_t *)imh)[64 + lane] = u1; }
                }
                *(uint4 *)(img + TAIL + lane * 32) = make_uint4(pc[0].x, pc[0].y, pc[0].z, pc[0].w);
                *(uint4 *)(img + TAIL + lane * 32 + 16) = make_uint4(pc[1].x, pc[1].y, pc[1].z, pc[1].w);
                *(uint4 *)(imh + TAIL + lane * 32) = make_uint4(0u, 0u, 0u, 0u);
                *(uint4 *)(imh + TAIL + lane * 32 + 16) = make_uint4(0u, 0u, 0u, 0u);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint32_t segpos = seg_start;
            uint32_t mrem = seg_len - lits;
            for (uint32_t g = 0; g < cnt; g += 64) {
                const bool hasq = g + (uint32_t)lane < cnt;
                const uint32_t ent = ent_next;
                ent_next = g + 64u + (uint32_t)lane < cnt ? q[g + 64u + lane] : 0u;
                const uint32_t l2 = (ent >> 15) & 0x1FFu;
                const bool has = hasq && l2 != 0u;
                const uint32_t mlen = has ? l2 + 2u : 0u, mdist = (ent & 0x7FFFu) + 1u;
                const uint32_t glit = !hasq ? 0u : has ? (ent >> 24) : ent;
                const uint32_t incl = za_wave_incl_scan(glit + mlen), incm = za_wave_incl_scan(mlen);
                const uint32_t mdst = segpos + incl - mlen;
                const uint32_t up = mrem - (incm - mlen);
                segpos += (uint32_t)__shfl((int)incl, 63, 64);
                mrem -= (uint32_t)__shfl((int)incm, 63, 64);
                const uint32_t ioff = TAIL + (mdst - seg_start);       // my match's destination inside the images; my literals end there
                uint8_t *od = img + ioff, *oh = imh + ioff;
                // the runs of literals move down (low plane only: their high bytes are the zeros the plane started with)
                if (__ballot(glit != 0u && up != 0u) != 0ull) {
                    const uint8_t *sp = od - glit + up;
                    ZaU4u a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
                    const bool mv = glit != 0u && up != 0u;
                    if (mv) {
                        a.x = *(const za_u32u *)sp; a.y = *(const za_u32u *)(sp + 4); a.z = *(const za_u32u *)(sp + 8); a.w = *(const za_u32u *)(sp + 12);
                        if (glit > 16u) { b.x = *(const za_u32u *)(sp + 16); b.y = *(const za_u32u *)(sp + 20); b.z = *(const za_u32u *)(sp + 24); b.w = *(const za_u32u *)(sp + 28); }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    if (mv) za_put32(od - glit, glit, a, b);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                bool done = !has;
                unsigned long long pending = __ballot(!done);
                const uint32_t sdst = hasq ? mdst : 0xFFFFFFFFu, send = hasq ? mdst + mlen : 0xFFFFFFFFu;
                const uint32_t src_a = mdst - mdist, src_b = src_a + (mlen < mdist ? mlen : mdist);      // (area coordinates: never negative)
                uint32_t jhi = 0, jlo = 0;
#pragma unroll
                for (uint32_t step = 32; step; step >>= 1) {
                    const uint32_t vd = (uint32_t)__shfl((int)sdst, (int)(jhi + step - 1u), 64);
                    const uint32_t ve = (uint32_t)__shfl((int)send, (int)(jlo + step - 1u), 64);
                    if (vd < src_b) jhi += step;
                    if (ve <= src_a) jlo += step;
                }
                const unsigned long long deps = ((1ull << jhi) - 1ull) & ~((1ull << jlo) - 1ull);
                const bool far = src_a + TAIL < seg_start;             // final symbols in memory (or the markers in front of the unit)
                const bool simple = mdist >= mlen && mlen <= 32u;
                ZaU4u fl = {0, 0, 0, 0}, fh = {0, 0, 0, 0}, fl2 = {0, 0, 0, 0}, fh2 = {0, 0, 0, 0};
                if (has && far && simple) {
                    ld_syms(src_a, fl, fh);
                    if (mlen > 16u) ld_syms(src_a + 16u, fl2, fh2);
                }
                while (pending) {
                    const bool ready = !done && (pending & deps) == 0ull;
                    if (ready && simple) {
                        ZaU4u v = fl, v2 = fl2, w = fh, w2 = fh2;
                        if (!far) {
                            const uint8_t *sp = od - mdist, *sh = oh - mdist;       // inside the images: src_a >= seg_start - 272
                            v.x = *(const za_u32u *)sp; v.y = *(const za_u32u *)(sp + 4); v.z = *(const za_u32u *)(sp + 8); v.w = *(const za_u32u *)(sp + 12);
                            w.x = *(const za_u32u *)sh; w.y = *(const za_u32u *)(sh + 4); w.z = *(const za_u32u *)(sh + 8); w.w = *(const za_u32u *)(sh + 12);
                            if (mlen > 16u) {
                                v2.x = *(const za_u32u *)(sp + 16); v2.y = *(const za_u32u *)(sp + 20); v2.z = *(const za_u32u *)(sp + 24); v2.w = *(const za_u32u *)(sp + 28);
                                w2.x = *(const za_u32u *)(sh + 16); w2.y = *(const za_u32u *)(sh + 20); w2.z = *(const za_u32u *)(sh + 24); w2.w = *(const za_u32u *)(sh + 28);
                            }
                        }
                        za_put32(od, mlen, v, v2);
                        za_put32(oh, mlen, w, w2);
                    }
                    // long or self-overlapping matches: the whole wave copies them, one at a time
                    unsigned long long coop = __ballot(ready && !simple);
                    while (coop) {
                        const int j = __builtin_ctzll(coop);
                        coop &= coop - 1ull;
                        const uint32_t cd = (uint32_t)__builtin_amdgcn_readlane((int)mdst, j);
                        const uint32_t cl = (uint32_t)__builtin_amdgcn_readlane((int)mlen, j);
                        const uint32_t cdist = (uint32_t)__builtin_amdgcn_readlane((int)mdist, j);
                        const bool cfar = cd - cdist + TAIL < seg_start;      // (then cdist > cl: no overlap)
                        uint8_t *o = img + TAIL + (cd - seg_start), *ohh = imh + TAIL + (cd - seg_start);
                        const float rd = 1.0f / (float)cdist;
                        for (uint32_t base = 0; base < cl; base += 64) {
                            const uint32_t i = base + (uint32_t)lane;
                            if (i < cl) {
                                int k = (int)i;
                                if (cdist < cl) {
                                    k = (int)i - (int)cdist * (int)((float)i * rd);
                                    if (k < 0) k += (int)cdist;
                                    if (k >= (int)cdist) k -= (int)cdist;
                                }
                                if (cfar) { const uint32_t sy = dst16[cd - cdist + (uint32_t)k]; o[i] = (uint8_t)sy; ohh[i] = (uint8_t)(sy >> 8); }
                                else { o[i] = (o - cdist)[k]; ohh[i] = (ohh - cdist)[k]; }
                            }
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    done = done || ready;
                    pending = __ballot(!done);
                }
            }
            // the finished segment: 32 symbols per lane, the planes interleaved on the way out (its last, partial piece symbol by symbol)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            {
                const uint32_t o = (uint32_t)lane * 32u;
                if (o + 32u <= seg_len) {
                    const uint4 a = *(const uint4 *)(img + TAIL + o), b2 = *(const uint4 *)(img + TAIL + o + 16);
                    const uint4 c4 = *(const uint4 *)(imh + TAIL + o), d4 = *(const uint4 *)(imh + TAIL + o + 16);
                    const uint32_t lw[8] = {a.x, a.y, a.z, a.w, b2.x, b2.y, b2.z, b2.w}, hw[8] = {c4.x, c4.y, c4.z, c4.w, d4.x, d4.y, d4.z, d4.w};
                    uint16_t *od16 = dst16 + seg_start + o;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        ZaU4u v;
                        v.x = __builtin_amdgcn_perm(hw[2 * k], lw[2 * k], 0x05010400u); v.y = __builtin_amdgcn_perm(hw[2 * k], lw[2 * k], 0x07030602u);
                        v.z = __builtin_amdgcn_perm(hw[2 * k + 1], lw[2 * k + 1], 0x05010400u); v.w = __builtin_amdgcn_perm(hw[2 * k + 1], lw[2 * k + 1], 0x07030602u);
                        *(ZaU4u *)(od16 + 8 * k) = v;
                    }
                } else for (uint32_t k = 0; k < 32u && o + k < seg_len; k++)
                    dst16[seg_start + o + k] = (uint16_t)((uint32_t)img[TAIL + o + k] | ((uint32_t)imh[TAIL + o + k] << 8));
            }
            __threadfence_block();       // later segments read these symbols from memory
        }
    }
    if (lane == 0) { ZaChunkRes r; r.status = last ? ZA_I_END : ZA_I_SYNC; r.max_back = 0; r.bits = (m.in_off + m.in_len) * 8ull; r.out_len = (uint64_t)n; res_out[blockIdx.x] = r; }
#undef ZA_UM_FAIL
}

// the 32 768 marker symbols in front of every unit's symbols (256 + j = "byte j of the window in front of this unit")
__global__ __launch_bounds__(256) void za_k_fill_marker_prefix(uint16_t *__restrict__ out16, uint64_t area_stride)
{
    uint16_t *p = out16 + (uint64_t)blockIdx.x * area_stride;
    for (uint32_t j = 8u * threadIdx.x; j < (uint32_t)ZA_WIN; j += 8u * 256u) {
        uint4 v;
        v.x = (256u + j) | ((257u + j) << 16); v.y = (258u + j) | ((259u + j) << 16); v.z = (260u + j) | ((261u + j) << 16); v.w = (262u + j) | ((263u + j) << 16);
        *(uint4 *)(p + j) = v;
    }
}

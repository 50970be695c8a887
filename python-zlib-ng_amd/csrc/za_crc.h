// Wave-cooperative CRC-32 over one <=128 KiB span: one lane per 2 KiB segment, partial results folded with
// GF(2) products.  Product code.
// Replaces zng_crc32_z (reference call sites zlib_ngmodule.c:1741, :2556).  Adler-32 is za_k_checksum's and za_wave_adler32's.
#pragma once
#include "za_common.h"

// All 64 lanes call with wave-uniform arguments.  crct: 256-entry table in LDS; x8k[k] = x^(8*2048*k).
__device__ __forceinline__ uint32_t za_wave_crc32(const uint8_t *data, int n, const uint32_t *crct,
                                                  const uint32_t *__restrict__ x8k)
{
    const int lane = za_lane();
    const int nseg = (n + ZA_SEG - 1) >> ZA_SEG_SHIFT;
    const int s0 = lane << ZA_SEG_SHIFT;
    int s1 = s0 + ZA_SEG;
    if (s1 > n) s1 = n;
    uint32_t c = 0;
    if (lane < nseg) {
        uint32_t r = 0xFFFFFFFFu;
        int p = s0;
        // byte steps until 4-byte aligned, then a dword per load
        for (; p < s1 && (((uintptr_t)(data + p)) & 3u); p++) r = crct[(r ^ data[p]) & 0xFF] ^ (r >> 8);
        for (; p + 4 <= s1; p += 4) {
            r ^= *(const uint32_t *)(data + p);
            r = crct[r & 0xFF] ^ (r >> 8);
            r = crct[r & 0xFF] ^ (r >> 8);
            r = crct[r & 0xFF] ^ (r >> 8);
            r = crct[r & 0xFF] ^ (r >> 8);
        }
        for (; p < s1; p++) r = crct[(r ^ data[p]) & 0xFF] ^ (r >> 8);
        c = r ^ 0xFFFFFFFFu;
        if (lane < nseg - 1) {
            // crc(A||B) = crc(A) * x^(8|B|) ^ crc(B);  |B| = (nseg-2-lane) full segments + the tail
            const int tail = n - ((nseg - 1) << ZA_SEG_SHIFT);
            uint32_t xt = 0x80000000u, sq = 0x00800000u;       // x^0, x^8
            for (int m = tail; m; m >>= 1) { if (m & 1) xt = za_multmodp(sq, xt); sq = za_multmodp(sq, sq); }
            c = za_multmodp(za_multmodp(x8k[nseg - 2 - lane], xt), c);
        }
    }
    return za_wave_xor_reduce(c);
}

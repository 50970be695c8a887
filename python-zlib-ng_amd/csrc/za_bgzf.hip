// BGZF (SAM specification section 4.1): the blocked gzip of htslib / samtools / tabix / bgzip.  DESIGN.md section 5d.
//   za_k_bgzf_lengths     bytes of every block: header + payload + trailer, the payload the unit pipeline's -- or ONE stored block
//                         where that one would not fit a 64 KiB block
//   za_k_assemble_bgzf    one workgroup per block: header with BSIZE, payload from the unit's slot (or the stored replacement, from
//                         the input), CRC-32, ISIZE, and the block's row of the block table; one more workgroup writes the EOF block
//   za_k_slice_gather     ranged reads: one workgroup per slice copies the requested bytes of the decoded blocks into a packed
//                         result, after it has made sure that every block the slice touches decoded and checked out
//   za_k_bgzf_count, za_k_bgzf_select and their helpers: lines by number (at the end of this file)
// Included by zng_amd.hip behind za_inflate.hip (ZaMember, ZA_I_OK).
#include "za_common.h"

#define ZA_BGZF_HDR        18u       // 1f 8b 08 04, MTIME, XFL, OS, XLEN = 6, 'B' 'C', SLEN = 2, BSIZE
#define ZA_BGZF_FIXED      26u       // header + CRC-32 + ISIZE
#define ZA_BGZF_MAX_IN     65280u    // htslib's 0xff00
#define ZA_BGZF_MAX_PAYLOAD (65536u - ZA_BGZF_FIXED)
#define ZA_BGZF_EOF_BYTES  28u

#define ZA_SLICE_OK    0
#define ZA_SLICE_BLOCK 1             // a block the slice touches failed (or the blocks do not cover the slice)
#define ZA_SLICE_TABLE 2             // the row points outside the buffers

struct ZaBgzfBlock {       // mirrors zngamd_bgzf_block
    uint64_t coffset, uoffset;
    uint32_t csize, isize;
};
struct ZaBgzfSlice {       // mirrors zngamd_bgzf_slice
    uint64_t src_off, dst_off;
    uint32_t len, reserved;
};

__device__ __constant__ uint8_t za_bgzf_eof[ZA_BGZF_EOF_BYTES] = {
    0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43, 0x02, 0x00, 0x1b, 0x00,
    0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};

// n bytes from src to dst by one workgroup: bytes until dst is 4-byte aligned, dwords (the 18-byte header leaves every payload
// misaligned against its slot: the loads take any address), bytes behind them
__device__ __forceinline__ void za_wg_copy(uint8_t *__restrict__ d, const uint8_t *__restrict__ src, uint32_t len)
{
    uint32_t headb = (uint32_t)((4u - ((uintptr_t)d & 3u)) & 3u);
    if (headb > len) headb = len;
    if (threadIdx.x < headb) d[threadIdx.x] = src[threadIdx.x];
    const uint32_t nw = (len - headb) >> 2;
    uint32_t *d32 = (uint32_t *)(d + headb);
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) d32[i] = za_ld32(src + headb + 4u * i);
    const uint32_t done = headb + 4u * nw;
    if (threadIdx.x < len - done) d[done + threadIdx.x] = src[done + threadIdx.x];
}

__global__ __launch_bounds__(256) void za_k_bgzf_lengths(const uint32_t *__restrict__ unit_len, const ZaUnit *__restrict__ units, uint32_t n,
                                                         uint32_t *__restrict__ block_bytes)
{
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const uint32_t dl = unit_len[b];
    block_bytes[b] = ZA_BGZF_FIXED + (dl > ZA_BGZF_MAX_PAYLOAD ? units[b].in_len + 5u : dl);
}

// grid: n blocks (+ 1 with eof: that workgroup writes the EOF block at *total and its row)
__global__ __launch_bounds__(256) void za_k_assemble_bgzf(const uint8_t *__restrict__ in, const uint8_t *__restrict__ slots, uint32_t slot_stride,
                                                          const uint32_t *__restrict__ unit_len, const uint32_t *__restrict__ unit_crc,
                                                          const ZaUnit *__restrict__ units, const uint32_t *__restrict__ block_bytes,
                                                          const uint64_t *__restrict__ block_off, const uint64_t *__restrict__ total,
                                                          uint32_t n, uint64_t in_len, uint8_t *__restrict__ dst, ZaBgzfBlock *__restrict__ table)
{
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    if (b >= n) {
        uint8_t *d = dst + *total;
        if (tid < ZA_BGZF_EOF_BYTES) d[tid] = za_bgzf_eof[tid];
        if (tid == 0 && table) { ZaBgzfBlock r; r.coffset = *total; r.uoffset = in_len; r.csize = ZA_BGZF_EOF_BYTES; r.isize = 0; table[n] = r; }
        return;
    }
    const uint32_t isize = units[b].in_len, size = block_bytes[b], dlen = size - ZA_BGZF_FIXED;
    const bool stored = unit_len[b] > ZA_BGZF_MAX_PAYLOAD;
    uint8_t *d = dst + block_off[b];
    if (tid < ZA_BGZF_HDR) {
        uint8_t v = 0;
        switch (tid) {
        case 0: v = 0x1f; break; case 1: v = 0x8b; break; case 2: v = 8; break; case 3: v = 4; break;
        case 9: v = 0xff; break; case 10: v = 6; break; case 12: v = 'B'; break; case 13: v = 'C'; break; case 14: v = 2; break;
        case 16: v = (uint8_t)((size - 1u) & 0xFF); break; case 17: v = (uint8_t)((size - 1u) >> 8); break;
        }
        d[tid] = v;
    }
    uint8_t *p = d + ZA_BGZF_HDR;
    if (stored) {
        // the unit pipeline's payload does not fit a block: one stored deflate block with the input itself
        if (tid < 5) p[tid] = tid == 0 ? 1 : (uint8_t)((tid < 3 ? isize : ~isize) >> (8 * ((tid - 1) & 1)));
        za_wg_copy(p + 5, in + units[b].in_off, isize);
    } else za_wg_copy(p, slots + (size_t)b * slot_stride, dlen);
    if (tid < 8) {
        const uint32_t v = tid < 4 ? unit_crc[b] : isize;
        p[dlen + tid] = (uint8_t)(v >> (8 * (tid & 3)));
    }
    if (tid == 0 && table) { ZaBgzfBlock r; r.coffset = block_off[b]; r.uoffset = units[b].in_off; r.csize = size; r.isize = isize; table[b] = r; }
}

// One workgroup per slice.  The members lie in ascending order of out_off (the caller's contract; a table that breaks it costs
// slices their verdict, never an access outside the buffers): the slice is good when members that decoded cover it without a gap.
__global__ __launch_bounds__(256) void za_k_slice_gather(const uint8_t *__restrict__ scratch, uint64_t scratch_len, const ZaMember *__restrict__ members,
                                                         const int32_t *__restrict__ member_status, uint32_t n_members,
                                                         const ZaBgzfSlice *__restrict__ slices, uint8_t *__restrict__ out, uint64_t out_cap,
                                                         int32_t *__restrict__ slice_status)
{
    __shared__ int verdict;
    const ZaBgzfSlice s = slices[blockIdx.x];
    if (threadIdx.x == 0) {
        int v = ZA_SLICE_OK;
        if (s.src_off > scratch_len || scratch_len - s.src_off < s.len || s.dst_off > out_cap || out_cap - s.dst_off < s.len) v = ZA_SLICE_TABLE;
        else if (s.len) {
            uint32_t lo = 0, hi = n_members;            // the last member that starts at or before the slice
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (members[mid].out_off <= s.src_off) lo = mid + 1; else hi = mid; }
            v = ZA_SLICE_BLOCK;
            if (lo > 0) {
                uint64_t at = s.src_off;
                const uint64_t end = s.src_off + s.len;
                for (uint32_t m = lo - 1; m < n_members; m++) {
                    const uint64_t mo = members[m].out_off, ml = members[m].out_len;
                    if (mo > at || member_status[m] != ZA_I_OK) break;
                    if (mo + ml > at) at = mo + ml;
                    if (at >= end) { v = ZA_SLICE_OK; break; }
                }
            }
        }
        verdict = v;
        slice_status[blockIdx.x] = v;
    }
    __syncthreads();
    if (verdict == ZA_SLICE_TABLE || s.len == 0) return;
    uint8_t *d = out + s.dst_off;
    if (verdict == ZA_SLICE_OK) za_wg_copy(d, scratch + s.src_off, s.len);
    else for (uint32_t i = threadIdx.x; i < s.len; i += blockDim.x) d[i] = 0;      // never the bytes of a block that failed
}

// ---- lines: counting a delimiter in the decoded blocks, and finding the r-th one of a block ------------
//   za_k_bgzf_count        one workgroup per block: how many of its output bytes equal the delimiter, and whether its last one does
//   za_k_bgzf_select       one workgroup per position query (block m, rank r): the scratch offset of the byte behind the r-th delimiter
//   za_k_bgzf_line_slices  pairs of positions become the slices of za_k_slice_gather (placed by za_k_offsets, za_k_bgzf_place)
//   za_k_bgzf_line_verdicts  a range keeps the verdict of its positions where the gather kernel had nothing to object to
#define ZA_SLICE_RANK  3             // a rank beyond the block's count: the index was built for another file
#define ZA_RANK_END    0xFFFFFFFFu   // the reserved rank: one past the block's last byte
#define ZA_COUNT_LAST  1u            // flags of a count row: the block's last output byte is the delimiter

struct ZaBgzfCount { uint32_t count, flags; };       // mirrors zngamd_bgzf_count_row
struct ZaBgzfPos { uint32_t m, r; };                 // mirrors zngamd_bgzf_pos; a zngamd_bgzf_line_range is two of them

// 0x80 in exactly the bytes of x that equal the byte `pat` repeats.  Exact per byte: no carry leaves a byte, unlike
// (y - 0x01010101) & ~y & 0x80808080, whose borrow marks a 0x01 byte above a zero one (a test, not a count).
__device__ __forceinline__ uint32_t za_eq_mask(uint32_t x, uint32_t pat)
{
    const uint32_t y = x ^ pat;
    const uint32_t t = (y & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | y | 0x7f7f7f7fu);
}
__device__ __forceinline__ uint32_t za_eq_count16(uint32_t x, uint32_t y, uint32_t z, uint32_t w, uint32_t pat)
{
    return (uint32_t)(__popc(za_eq_mask(x, pat)) + __popc(za_eq_mask(y, pat)) + __popc(za_eq_mask(z, pat)) + __popc(za_eq_mask(w, pat)));
}

// the member's output lies inside the scratch (the tables are untrusted; no sum that could wrap)
__device__ __forceinline__ bool za_member_in_scratch(const ZaMember &m, uint64_t scratch_cap)
{
    return m.out_off <= scratch_cap && scratch_cap - m.out_off >= m.out_len;
}

// grid: one workgroup per member.  16-byte loads on the aligned body (out_off is not aligned in general), bytes in front and behind.
__global__ __launch_bounds__(256) void za_k_bgzf_count(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, const ZaMember *__restrict__ members,
                                                       const int32_t *__restrict__ member_status, uint32_t delim, ZaBgzfCount *__restrict__ rows)
{
    __shared__ uint32_t part[4];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const ZaMember m = members[b];
    if (member_status[b] != ZA_I_OK || !za_member_in_scratch(m, scratch_cap)) {       // (the same for every thread)
        if (tid == 0) { ZaBgzfCount r; r.count = 0; r.flags = 0; rows[b] = r; }
        return;
    }
    const uint8_t *p = scratch + m.out_off;
    const uint32_t len = m.out_len, pat = delim * 0x01010101u;
    uint32_t head = (uint32_t)((16u - ((uintptr_t)p & 15u)) & 15u);
    if (head > len) head = len;
    uint32_t n = 0;
    if (tid < head) n += p[tid] == delim;
    const uint4 *body = (const uint4 *)(p + head);
    const uint32_t nv = (len - head) >> 4;
    for (uint32_t i = tid; i < nv; i += 256u) { const uint4 v = body[i]; n += za_eq_count16(v.x, v.y, v.z, v.w, pat); }
    const uint32_t done = head + 16u * nv;
    if (tid < len - done) n += p[done + tid] == delim;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
    if ((tid & 63u) == 0) part[tid >> 6] = n;
    __syncthreads();
    if (tid == 0) {
        ZaBgzfCount r; r.count = part[0] + part[1] + part[2] + part[3];
        r.flags = (len && p[len - 1u] == delim) ? ZA_COUNT_LAST : 0u;
        rows[b] = r;
    }
}

// grid: one workgroup per query.  Every thread counts its stretch of 256 bytes, a scan over the 256 counts finds the stretch that
// holds the r-th delimiter, and its thread walks it.  Whatever the tables say, nothing outside [scratch, scratch + scratch_cap) is read.
__global__ __launch_bounds__(256) void za_k_bgzf_select(const uint8_t *__restrict__ scratch, uint64_t scratch_cap, const ZaMember *__restrict__ members,
                                                        const int32_t *__restrict__ member_status, uint32_t n_members,
                                                        const ZaBgzfPos *__restrict__ queries, uint32_t delim, uint64_t *__restrict__ pos_out,
                                                        int32_t *__restrict__ pos_status)
{
    __shared__ uint32_t wave_sum[4];
    __shared__ uint32_t found;
    const uint32_t tid = threadIdx.x;
    const ZaBgzfPos q = queries[blockIdx.x];
    int verdict = ZA_SLICE_OK;                        // (everything up to the scan is the same for every thread)
    uint64_t pos = 0;
    ZaMember m = {};
    if (q.m >= n_members) verdict = ZA_SLICE_TABLE;
    else {
        m = members[q.m];
        if (!za_member_in_scratch(m, scratch_cap) || m.out_len > 65536u) verdict = ZA_SLICE_TABLE;      // (256 threads x 256 bytes)
        else if (member_status[q.m] != ZA_I_OK) verdict = ZA_SLICE_BLOCK;
    }
    if (verdict == ZA_SLICE_OK) {
        if (q.r == 0) pos = m.out_off;
        else if (q.r == ZA_RANK_END) pos = m.out_off + m.out_len;
        else {
            const uint8_t *p = scratch + m.out_off;
            const uint32_t len = m.out_len, pat = delim * 0x01010101u;
            const uint32_t b = tid * 256u < len ? tid * 256u : len, e = b + 256u < len ? b + 256u : len;
            uint32_t n = 0, i = b;
            for (; i + 16u <= e; i += 16u) { const ZaU4u v = *(const ZaU4u *)(p + i); n += za_eq_count16(v.x, v.y, v.z, v.w, pat); }
            for (; i < e; i++) n += p[i] == delim;
            const uint32_t incl = za_wave_incl_scan(n);
            if ((tid & 63u) == 63u) wave_sum[tid >> 6] = incl;
            if (tid == 0) found = 0xFFFFFFFFu;
            __syncthreads();
            uint32_t base = 0, total = 0;
            for (uint32_t w = 0; w < 4u; w++) { const uint32_t s = wave_sum[w]; if (w < (tid >> 6)) base += s; total += s; }
            if (q.r > total) verdict = ZA_SLICE_RANK;
            else {
                const uint32_t excl = base + incl - n;
                if (excl < q.r && q.r <= excl + n) {           // exactly one thread
                    uint32_t left = q.r - excl, j = b;
                    for (; j < e; j++) if (p[j] == delim && --left == 0) break;
                    found = j + 1u;
                }
                __syncthreads();
                pos = m.out_off + found;
            }
        }
    }
    if (tid == 0) { pos_out[blockIdx.x] = verdict == ZA_SLICE_OK ? pos : 0ull; pos_status[blockIdx.x] = verdict; }
}

// One thread per range: positions 2 i and 2 i + 1 become slice i.  A range whose positions have no verdict of 0, whose second
// position lies below its first, or that is 4 GiB long or longer, is an empty slice with a verdict in `pre`.
__global__ __launch_bounds__(256) void za_k_bgzf_line_slices(const uint64_t *__restrict__ pos, const int32_t *__restrict__ pos_status, uint32_t n,
                                                             ZaBgzfSlice *__restrict__ slices, uint32_t *__restrict__ lens, int32_t *__restrict__ pre)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t p0 = pos[2u * i], p1 = pos[2u * i + 1u];
    int v = pos_status[2u * i] ? pos_status[2u * i] : pos_status[2u * i + 1u];
    uint32_t len = 0;
    if (v == ZA_SLICE_OK) {
        if (p1 < p0 || p1 - p0 >= (1ull << 32)) v = ZA_SLICE_TABLE;
        else len = (uint32_t)(p1 - p0);
    }
    ZaBgzfSlice s; s.src_off = v == ZA_SLICE_OK ? p0 : 0ull; s.dst_off = 0; s.len = len; s.reserved = 0;
    slices[i] = s; lens[i] = len; pre[i] = v;
}

__global__ __launch_bounds__(256) void za_k_bgzf_place(const uint64_t *__restrict__ offs, uint32_t n, ZaBgzfSlice *__restrict__ slices)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slices[i].dst_off = offs[i];
}

__global__ __launch_bounds__(256) void za_k_bgzf_line_verdicts(const int32_t *__restrict__ pre, uint32_t n, int32_t *__restrict__ range_status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && pre[i] != ZA_SLICE_OK) range_status[i] = pre[i];
}

// Batch API: a preset dictionary trained from sample records (zngamd_train_dict[_dev], batch.train_dict).  Product code; included
// by zng_amd.hip behind za_batch.hip.  The algorithm is the deterministic FastCOVER variant of DESIGN.md section 5c.2, restated in
// tests/dict_train_ref.py; every kernel keeps its result independent of the launch shape and of the order of the atomics.
//   za_k_dict_gather   the items, one wave each, back to back into one staging buffer (the host placed them: out_off)
//   za_k_dict_hash     the d-mer hash of every position (16 positions a thread)
//   za_k_dict_mark     the sentinel on the d - 1 positions in front of every sample's end (their d-mers cross it)
//   za_k_dict_count    freq[h] += 1 for every valid position: integer atomics, summed per thread and per wave first
//   za_k_dict_shadow   once: for every position p of the scanned epochs, p - lo_p (the first window start p counts for)
//   za_k_dict_score    per pick: the windows' scores of the current epoch, 4096 starts a workgroup, as a difference array in LDS
//                      and its prefix sum; the tile's best (score, start)
//   za_k_dict_pick     per pick, one workgroup: the best of the tiles, the trim, the zeroing of freq, the bytes to the dictionary's
//                      tail, and the state (tail, epoch, zero_run, done)
// score and pick return at once when `done` is set: the host enqueues picks in groups and reads the state once per group.
#pragma once

#define ZA_DICT_HASH_BITS 20
#define ZA_DICT_SENT      0xFFFFFFFFu          // no hash: the d-mer crosses its sample's end
#define ZA_DICT_PRIME     0xCF1BBCDCB7A56463ull
#define ZA_DICT_TILE      4096                 // window starts per za_k_dict_score workgroup
#define ZA_DICT_SH_TILE   1024                 // positions per za_k_dict_shadow workgroup
#define ZA_DICT_SH_LDS    16384                // hashes za_k_dict_shadow keeps in LDS (64 KiB): look-back + tile

struct ZaDictState { uint32_t tail, epoch, zero_run, done, picks, reserved[3]; };
struct ZaDictBest { unsigned long long score; uint32_t start, reserved; };

// item i (in_off, in_len in `in`; out_off = its place in `data`) copied to data + out_off.  The host checked the table; an entry
// outside the buffers is left alone here as well.
__global__ __launch_bounds__(64) void za_k_dict_gather(const uint8_t *__restrict__ in, uint64_t in_len, const ZaBatchItem *__restrict__ items,
                                                       uint32_t n, uint8_t *__restrict__ data, uint64_t data_len)
{
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const ZaBatchItem it = items[i];
    if (it.in_off > in_len || in_len - it.in_off < it.in_len || it.out_off > data_len || data_len - it.out_off < it.in_len) return;
    za_wave_copy(data + it.out_off, in + it.in_off, it.in_len);
}

// hash[p] for p < n: the d bytes at p little-endian (upper bytes zero) times the prime, the top 20 bits.  data: 16-byte aligned,
// readable 24 bytes past every p < n (the staging buffer has 64 zero bytes behind the samples).
__global__ __launch_bounds__(256) void za_k_dict_hash(const uint8_t *__restrict__ data, uint32_t n, uint32_t d, uint32_t *__restrict__ hash)
{
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    if (p0 >= n) return;
    const uint4 a = *(const uint4 *)(data + p0);
    const uint2 b = *(const uint2 *)(data + p0 + 16);
    const uint32_t w[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
    const unsigned long long mask = d >= 8 ? ~0ull : (1ull << (8 * d)) - 1;
    uint32_t h[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const int q = j >> 2, s = (j & 3) * 8;
        const unsigned long long lo = ((unsigned long long)w[q + 1] << 32) | w[q];
        const unsigned long long v = (s ? (lo >> s) | ((unsigned long long)w[q + 2] << (64 - s)) : lo) & mask;
        h[j] = (uint32_t)((v * ZA_DICT_PRIME) >> (64 - ZA_DICT_HASH_BITS));
    }
    if (p0 + 16 <= n) {
        uint4 *o = (uint4 *)(hash + p0);
#pragma unroll
        for (int j = 0; j < 4; j++) o[j] = make_uint4(h[4 * j], h[4 * j + 1], h[4 * j + 2], h[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) if (p0 + j < n) hash[p0 + j] = h[j];
    }
}

// Positions [end - d + 1, end) of every sample (end = out_off + in_len) get the sentinel: a d-mer there runs past the end of the
// sample it starts in (a sample shorter than d marks positions of the one before it, whose d-mers cross into it: they are invalid too).
__global__ __launch_bounds__(256) void za_k_dict_mark(const ZaBatchItem *__restrict__ items, uint32_t n_items, uint32_t n, uint32_t d,
                                                      uint32_t *__restrict__ hash)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_items) return;
    const uint64_t end = items[i].out_off + items[i].in_len;
    for (uint64_t p = end >= d - 1 ? end - (d - 1) : 0; p < end && p < n; p++) hash[p] = ZA_DICT_SENT;
}

// freq[hash[p]] += 1 over the valid positions.  A thread's 16 positions are summed per hash first, then up to four rounds take one
// hash across the wave (a run of one byte value -- zeros in ELF files -- is one atomic per 1 024 positions); the rest are one atomic
// each.  Integer sums: the same in any order.
__global__ __launch_bounds__(256) void za_k_dict_count(const uint32_t *__restrict__ hash, uint32_t n, uint32_t *__restrict__ freq)
{
    const uint64_t p0 = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    uint32_t h[16], c[16];
    if (p0 + 16 <= n) {
        const uint4 *s = (const uint4 *)(hash + p0);
#pragma unroll
        for (int j = 0; j < 4; j++) { const uint4 v = s[j]; h[4 * j] = v.x; h[4 * j + 1] = v.y; h[4 * j + 2] = v.z; h[4 * j + 3] = v.w; }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) h[j] = p0 + j < n ? hash[p0 + j] : ZA_DICT_SENT;
    }
#pragma unroll
    for (int j = 0; j < 16; j++) c[j] = h[j] != ZA_DICT_SENT;
#pragma unroll
    for (int j = 1; j < 16; j++) {
#pragma unroll
        for (int i = 0; i < j; i++)
            if (c[j] && c[i] && h[i] == h[j]) { c[i] += c[j]; c[j] = 0; }
    }
    const int lane = za_lane();
    for (int round = 0; round < 4; round++) {
        uint32_t mine = ZA_DICT_SENT;
#pragma unroll
        for (int j = 15; j >= 0; j--) if (c[j]) mine = h[j];
        const unsigned long long m = __ballot(mine != ZA_DICT_SENT);
        if (!m) return;
        const int leader = __builtin_ctzll(m);
        const uint32_t hw = __shfl(mine, leader, 64);
        uint32_t s = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) if (c[j] && h[j] == hw) { s += c[j]; c[j] = 0; }
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == leader) atomicAdd(&freq[hw], s);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) if (c[j]) atomicAdd(&freq[h[j]], c[j]);
}

// shadow[p] = p - lo_p for the positions p < limit (= E * S) of the epochs (size S):  lo_p = max(prev_p + 1, p - K + 1, epoch start),
// prev_p the nearest earlier position of p's epoch with p's hash.  The look-back runs through the hashes of [b0, tile end) in LDS
// (LDS = true: they fit ZA_DICT_SH_LDS, 64 KiB) or through global memory (k close to 16 384).  Invalid positions get 0 (never read).
template <bool LDS>
__global__ __launch_bounds__(256) void za_k_dict_shadow(const uint32_t *__restrict__ hash, uint32_t limit, uint32_t S, uint32_t K,
                                                        uint16_t *__restrict__ shadow)
{
    extern __shared__ uint32_t lh[];                                        // LDS: K - 1 + ZA_DICT_SH_TILE hashes
    const uint32_t t0 = blockIdx.x * ZA_DICT_SH_TILE;
    const uint64_t t1 = min((uint64_t)t0 + ZA_DICT_SH_TILE, (uint64_t)limit);     // (64-bit: positions run up to 4 GiB)
    const uint32_t es0 = t0 / S * S;
    const uint32_t b0 = max(t0 >= K - 1 ? t0 - (K - 1) : 0u, es0);
    if (LDS) {
        for (uint64_t q = (uint64_t)b0 + threadIdx.x; q < t1; q += 256) lh[q - b0] = hash[q];
        __syncthreads();
    }
    for (uint64_t pp = (uint64_t)t0 + threadIdx.x; pp < t1; pp += 256) {
        const uint32_t p = (uint32_t)pp;
        const uint32_t h = LDS ? lh[p - b0] : hash[p];
        uint32_t off = 0;
        if (h != ZA_DICT_SENT) {
            const uint32_t lim = min(K - 1, p - p / S * S);          // look back j = 1 .. lim (p - lim >= b0)
            uint32_t j = 1;
            if (LDS) { for (; j <= lim; j++) if (lh[p - j - b0] == h) break; }
            else { for (; j <= lim; j++) if (hash[p - j] == h) break; }
            off = j <= lim ? j - 1 : lim;
        }
        shadow[p] = (uint16_t)off;
    }
}

__device__ __forceinline__ bool za_dict_better(unsigned long long s, uint32_t i, unsigned long long bs, uint32_t bi)
{
    return s > bs || (s == bs && i < bi);
}

// (score, start) of the best in the workgroup: the highest score, the lowest start among equals.  red: 4 entries of LDS.
__device__ __forceinline__ void za_dict_block_best(unsigned long long &s, uint32_t &i, ZaDictBest *red)
{
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long s2 = __shfl_xor(s, o, 64);
        const uint32_t i2 = __shfl_xor(i, o, 64);
        if (za_dict_better(s2, i2, s, i)) { s = s2; i = i2; }
    }
    const int w = threadIdx.x >> 6;
    if (za_lane() == 0) { red[w].score = s; red[w].start = i; }
    __syncthreads();
    s = red[0].score; i = red[0].start;
    for (int k = 1; k < 4; k++) if (za_dict_better(red[k].score, red[k].start, s, i)) { s = red[k].score; i = red[k].start; }
}

// The windows of epoch st->epoch starting at [j0, j0 + 4096) (relative to the epoch; nst = S - K + 1 starts in all): every valid p
// adds freq[hash[p]] on [max(lo_p, first start), min(p, last start)] of a difference array in LDS (64-bit adds: a score is the sum of
// up to K frequencies of up to n each); its prefix sum is the scores.  -> best[blockIdx.x] = the tile's best (score, start in epoch).
__global__ __launch_bounds__(256) void za_k_dict_score(const uint32_t *__restrict__ hash, const uint16_t *__restrict__ shadow,
                                                       const uint32_t *__restrict__ freq, uint32_t S, uint32_t K,
                                                       const ZaDictState *__restrict__ st, ZaDictBest *__restrict__ best)
{
    __shared__ unsigned long long D[ZA_DICT_TILE + 1];
    __shared__ unsigned long long wsum[4];
    __shared__ ZaDictBest red[4];
    if (st->done) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t es = st->epoch * S, nst = S - K + 1;
    const uint32_t j0 = blockIdx.x * ZA_DICT_TILE;
    const uint32_t nb = min((uint32_t)ZA_DICT_TILE, nst - j0);
    const uint32_t a = es + j0, pend = es + min(S, j0 + nb + K - 1);
    for (uint32_t i = tid; i <= ZA_DICT_TILE; i += 256) D[i] = 0;
    __syncthreads();
    for (uint64_t pp = (uint64_t)a + tid; pp < pend; pp += 256) {
        const uint32_t p = (uint32_t)pp;
        const uint32_t h = hash[p];
        if (h == ZA_DICT_SENT) continue;
        const uint32_t f = freq[h];
        if (!f) continue;
        const uint32_t lo = p - shadow[p];
        const uint32_t L = lo > a ? lo - a : 0;
        if (L >= nb) continue;
        const uint32_t R = min(p - a, nb - 1);
        atomicAdd(&D[L], (unsigned long long)f);
        atomicAdd(&D[R + 1], 0ull - f);
    }
    __syncthreads();
    // prefix sum: thread t owns [16 t, 16 t + 16)
    unsigned long long v[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) { v[k] = D[16 * tid + k]; sum += v[k]; }
    const int lane = za_lane(), w = tid >> 6;
    unsigned long long inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long run = inc - sum;
    for (int k = 0; k < w; k++) run += wsum[k];
    unsigned long long bs = 0;
    uint32_t bi = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        run += v[k];
        const uint32_t i = 16 * tid + k;
        if (i < nb && za_dict_better(run, j0 + i, bs, bi)) { bs = run; bi = j0 + i; }
    }
    za_dict_block_best(bs, bi, red);
    if (tid == 0) { best[blockIdx.x].score = bs; best[blockIdx.x].start = bi; best[blockIdx.x].reserved = 0; }
}

// One pick (one workgroup): the best window of the epoch from the tiles' bests; score 0 counts towards zero_run, else the window
// is trimmed to [s0, s1] (its first and last positions whose hash still has a frequency), those hashes' frequencies become 0 (after
// every read of the trim), and min(s1 - s0 + d, tail) bytes from s0 go in front of what the dictionary's tail holds.
__global__ __launch_bounds__(256) void za_k_dict_pick(const uint8_t *__restrict__ data, const uint32_t *__restrict__ hash,
                                                      uint32_t *__restrict__ freq, const ZaDictBest *__restrict__ best, uint32_t ntiles,
                                                      uint32_t S, uint32_t K, uint32_t E, uint32_t d, ZaDictState *__restrict__ st,
                                                      uint8_t *__restrict__ dict)
{
    __shared__ ZaDictBest red[4];
    __shared__ uint32_t lim[2][4];
    if (st->done) return;
    const uint32_t tid = threadIdx.x;
    const ZaDictState s = *st;
    unsigned long long bs = 0;
    uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t t = tid; t < ntiles; t += 256)
        if (za_dict_better(best[t].score, best[t].start, bs, bi)) { bs = best[t].score; bi = best[t].start; }
    za_dict_block_best(bs, bi, red);
    ZaDictState ns = s;
    ns.picks = s.picks + 1;
    if (bs == 0) {
        ns.zero_run = s.zero_run + 1;
        if (ns.zero_run >= E) ns.done = 1;
        else ns.epoch = (s.epoch + 1) % E;
        __syncthreads();
        if (tid == 0) *st = ns;
        return;
    }
    const uint32_t start = s.epoch * S + bi;
    uint32_t mn = 0xFFFFFFFFu, mx = 0;
    for (uint32_t q = tid; q < K; q += 256) {
        const uint32_t h = hash[start + q];
        if (h != ZA_DICT_SENT && freq[h]) { mn = min(mn, q); mx = max(mx, q); }
    }
    for (int o = 32; o >= 1; o >>= 1) { mn = min(mn, (uint32_t)__shfl_xor(mn, o, 64)); mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64)); }
    if (za_lane() == 0) { lim[0][tid >> 6] = mn; lim[1][tid >> 6] = mx; }
    __syncthreads();                                                        // every read of freq by the trim is done
    mn = min(min(lim[0][0], lim[0][1]), min(lim[0][2], lim[0][3]));
    mx = max(max(lim[1][0], lim[1][1]), max(lim[1][2], lim[1][3]));
    if (mn > mx) {                                                          // (a score above 0 has a position with a frequency)
        ns.done = 1;
        if (tid == 0) *st = ns;
        return;
    }
    const uint32_t s0 = start + mn, s1 = start + mx;
    for (uint64_t p = (uint64_t)s0 + tid; p <= s1; p += 256) {
        const uint32_t h = hash[p];
        if (h != ZA_DICT_SENT) freq[h] = 0;
    }
    const uint32_t size = min(s1 - s0 + d, s.tail);
    ns.zero_run = 0;
    if (size < d) ns.done = 1;
    else {
        ns.tail = s.tail - size;
        for (uint32_t q = tid; q < size; q += 256) dict[ns.tail + q] = data[s0 + q];
        ns.epoch = (s.epoch + 1) % E;
        if (ns.tail == 0) ns.done = 1;
    }
    __syncthreads();
    if (tid == 0) *st = ns;
}

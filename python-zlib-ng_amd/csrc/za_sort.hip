// BGZF: records in another order -- a key per record whose memcmp order is the order wanted, a stable sort of
// any such keys, and records written where the caller says.  The prologue of the key pass and of the place pass is that of
// za_dedup.hip: the lines pass of za_grep.hip has run for the delimiters alone, the host has read how many lines the text holds, and
// za_k_grep_rec_lines of za_grep_records.hip has written where every line starts.  What is new:
//   za_k_sort_keys        one WAVE per record: for every part of the key its field of its line, found and read in strips of 64 bytes, and
//                         the part's bytes written big-endian into the record's row; the record's length
//   za_k_sort_keys_close  one thread: the totals and the fault of the key pass
//   za_k_sort_orand       the OR and the AND of all rows, word by word: a byte whose OR equals its AND is the same in every row
//   za_k_sort_iota        order[i] = i
//   za_k_sort_hist        one workgroup per tile of ZA_SORT_TILE rows: the digit of every row of the order array as it stands, and
//                         how often the tile holds every digit value
//   za_k_sort_scan        one workgroup per digit value: where every tile's rows of that value begin among the rows of that value
//   za_k_sort_scatter     one workgroup per tile: every row's place = the rows of smaller values + the rows of its value in earlier
//                         tiles, in earlier waves of its tile, in earlier strips of its wave and below its lane
//   za_k_sort_rank        rank[order[j]] = j
//   za_k_sort_place       one WAVE per record: its bytes copied to out + dst[r], the closing delimiter added where the key pass counted it
//   za_k_sort_place_close one thread: the totals and the fault of the place pass
// Why every kernel ends: no kernel here reads a word that another workgroup of the same launch writes, none spins, and every loop
// runs over a count fixed at launch (strips of a tile, tiles of a digit, strips of a field, records of a stride).  The sort's result
// depends on the rows alone: counts are sums of integers, places follow from counts, no atomic decides an order.
// Included by zng_amd.hip behind za_dedup.hip (za_trim_body reads a line's body, za_wave_incl_scan sums a wave).
#include "za_common.h"

#define ZA_SORT_BYTES   0u                             // mirror ZNGAMD_BGZF_SORT_BYTES / _NUMBER / _LENGTH
#define ZA_SORT_NUMBER  1u
#define ZA_SORT_LENGTH  2u
#define ZA_SORT_REVERSE     1u                         // mirror ZNGAMD_BGZF_SORT_REVERSE / _IGNORE_CASE / _TRUNCATE
#define ZA_SORT_IGNORE_CASE 2u
#define ZA_SORT_TRUNCATE    4u
#define ZA_SORT_MAX_PARTS 4u                           // mirrors ZNGAMD_BGZF_SORT_MAX_PARTS
#define ZA_SORT_MAX_WIDTH 256u                         // mirrors ZNGAMD_SORT_MAX_WIDTH
#define ZA_SORT_WG_PER_CU 8u                           // workgroups of za_k_sort_keys / za_k_sort_place per CU: no LDS, the waves alone bound it
#define ZA_SORT_STRIPS  8u                             // strips of 64 rows a wave of the hist and scatter kernels takes
#define ZA_SORT_TILE    (4u * 64u * ZA_SORT_STRIPS)    // rows per workgroup of them: 2048
#define ZA_SORT_SKIP    (~0ull)                        // mirrors ZNGAMD_BGZF_PLACE_SKIP

struct ZaSortPart { int32_t line, column; uint32_t width, first; uint16_t flags; uint8_t kind, sep; };      // mirrors zngamd_bgzf_sort_part
struct ZaSortPar { uint32_t k_lines; int32_t first_byte, meta_byte; uint32_t n_parts, delim, width, final; ZaSortPart part[ZA_SORT_MAX_PARTS]; };
struct ZaSortKeyTotals { uint64_t seen, bytes_in, max_field, tail_off, bad_record, bad_src; uint32_t covered, short_lines, bad, key_width; };   // zngamd_bgzf_sort_key_totals
struct ZaPlaceTotals { uint64_t seen, placed, placed_bytes, tail_off, bad_record, bad_src; uint32_t covered, short_lines, bad, labels_short; }; // zngamd_bgzf_place_totals

__device__ const uint64_t za_sort_pow10[20] = {
    1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull, 10000000000ull, 100000000000ull,
    1000000000000ull, 10000000000000ull, 100000000000000ull, 1000000000000000ull, 10000000000000000ull, 100000000000000000ull,
    1000000000000000000ull, 10000000000000000000ull};
__device__ const uint8_t za_sort_u64max[20] = {1, 8, 4, 4, 6, 7, 4, 4, 0, 7, 3, 7, 0, 9, 5, 5, 1, 6, 1, 5};      // 2^64 - 1, digit by digit

// the lane of the k-th (from 0) set bit of m; 64 when m holds k bits or fewer.  The whole wave calls it with the same m and k.
__device__ __forceinline__ uint32_t za_sort_kth(uint64_t m, uint32_t k, uint32_t lane)
{
    const uint64_t sel = __ballot((m >> lane & 1ull) && (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) == k);
    return sel ? (uint32_t)__builtin_ctzll(sel) : 64u;
}

// field `column` (>= 0) of body[0, nb) cut at `sep`, in strips of 64 bytes: *fs its first byte, -> its length; a body with fewer
// separators than `column` has no such field: an empty one.  Lane l of strip p0 reads body[p0 + l] only when p0 + l < nb.
__device__ __forceinline__ uint32_t za_sort_field(const uint8_t *__restrict__ body, uint32_t nb, uint32_t column, uint32_t sep, uint32_t lane, uint32_t *fs)
{
    uint32_t seen = 0, a = column ? ~0u : 0u, e = nb;
    #pragma unroll 1
    for (uint32_t p0 = 0; p0 < nb; p0 += 64u) {
        const bool in = lane < nb - p0;
        const uint64_t m = __ballot(in && body[p0 + lane] == sep);
        const uint32_t c = (uint32_t)__popcll(m);
        if (a == ~0u && seen + c >= column) a = p0 + za_sort_kth(m, column - 1u - seen, lane) + 1u;
        if (seen + c > column) { e = p0 + za_sort_kth(m, column - seen, lane); break; }
        seen += c;
    }
    if (a == ~0u) { *fs = 0; return 0; }
    *fs = a;
    return e - a;
}

// grid: any number of workgroups of four waves; wave w of workgroup g takes the records 4 g + w, 4 (g + gridDim.x) + w, ...  start, lines:
// as za_rec_extent takes them.  row: nrec rows of P.width bytes, or no pointer; len: nrec words, or no pointer.  tot (zeroed): bytes_in
// is summed and max_field raised here; the three words behind it (~0 beforehand): the smallest r whose first byte is not first_byte,
// whose number is none, whose field is too long.  Every byte read lies in the body of a line of the text; every byte written lies in
// row[r * width, (r + 1) * width) or len[r].  No barrier, no LDS.
__global__ __launch_bounds__(256) void za_k_sort_keys(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start, uint64_t lines,
                                                      uint64_t nrec, ZaSortPar P, uint8_t *__restrict__ row, uint32_t *__restrict__ len, ZaSortKeyTotals *__restrict__ tot)
{
    unsigned long long *bad = (unsigned long long *)(tot + 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t stride = (uint64_t)gridDim.x * 4u;
    uint64_t bytes_in = 0;
    uint32_t max_field = 0;
    #pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + wave; r < nrec; r += stride) {
        const uint64_t lo = (uint64_t)P.k_lines * r, hi = lines - lo < P.k_lines ? lines : lo + P.k_lines;
        const uint64_t ra = start[lo], re = start[hi];
        const uint32_t rlen = re > ra ? (uint32_t)(re - ra) : 0u;
        const bool open = P.final && hi == lines && rlen && scratch[re - 1u] != P.delim;      // the text's last line has no delimiter: it gets one
        if (lane == 0) {
            if (P.first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)P.first_byte)) atomicMin(&bad[0], (unsigned long long)r);
            if (len) len[r] = rlen + (open ? 1u : 0u);
        }
        bytes_in += rlen;
        if (!row || !P.width) continue;
        uint8_t *out = row + r * P.width;
        const bool meta = P.meta_byte >= 0 && rlen && scratch[ra] == (uint32_t)P.meta_byte;
        uint32_t at = 0;                                                           // bytes of the row written so far
        #pragma unroll 1
        for (uint32_t p = 0; p < P.n_parts && !meta; p++) {
            const ZaSortPart q = P.part[p];
            const uint32_t inv = (q.flags & ZA_SORT_REVERSE) ? 0xFFu : 0u;
            uint32_t nb, hd, fs = 0;
            const uint64_t ls = za_trim_body(scratch, start, lo, (uint32_t)(hi - lo), (uint32_t)q.line, P.delim, &nb, &hd);
            const uint8_t *body = scratch + ls;
            const uint32_t fl = q.column < 0 ? nb : za_sort_field(body, nb, (uint32_t)q.column, q.sep, lane, &fs);
            const uint8_t *f = body + fs;
            if (q.kind == ZA_SORT_BYTES) {
                const uint32_t off = q.first < fl ? q.first : fl, avail = fl - off;
                if (avail > q.width && !(q.flags & ZA_SORT_TRUNCATE)) {
                    if (lane == 0) atomicMin(&bad[2], (unsigned long long)r);
                    max_field = fl > max_field ? fl : max_field;
                }
                const bool fold = (q.flags & ZA_SORT_IGNORE_CASE) != 0;
                #pragma unroll 1
                for (uint32_t i = lane; i < q.width; i += 64u) {
                    uint32_t c = i < avail ? f[off + i] : 0u;
                    if (fold && c >= 'a' && c <= 'z') c -= 0x20u;
                    out[at + i] = (uint8_t)(c ^ inv);
                }
                at += q.width;
            } else if (q.kind == ZA_SORT_NUMBER) {
                uint32_t lead = fl;                                                // where the first byte that is not '0' stands
                bool wrong = fl == 0;
                #pragma unroll 1
                for (uint32_t p0 = 0; p0 < fl; p0 += 64u) {
                    const bool in = lane < fl - p0;
                    const uint32_t c = in ? f[p0 + lane] : (uint32_t)'0';
                    if (__ballot(c < '0' || c > '9')) { wrong = true; break; }
                    const uint64_t nz = __ballot(c != '0');
                    if (lead == fl && nz) lead = p0 + (uint32_t)__builtin_ctzll(nz);
                }
                const uint32_t sig = fl - lead;
                uint64_t term = 0;
                if (!wrong && sig > 20u) wrong = true;
                if (!wrong) {
                    const uint32_t d = lane < sig ? (uint32_t)f[lead + lane] - '0' : 0u;
                    if (sig == 20u) {                                              // 20 digits: none above 2^64 - 1, told at the first digit that differs
                        const uint32_t lim = lane < 20u ? za_sort_u64max[lane] : 0u;
                        const uint64_t gt = __ballot(lane < 20u && d > lim), ne = __ballot(lane < 20u && d != lim);
                        if (ne && (gt >> __builtin_ctzll(ne) & 1ull)) wrong = true;
                    }
                    if (lane < sig) term = (uint64_t)d * za_sort_pow10[sig - 1u - lane];
                }
                if (wrong && lane == 0) atomicMin(&bad[1], (unsigned long long)r);
                const uint64_t v = wrong ? 0ull : za_wave_sum_u64(term);
                if (lane < 8u) out[at + lane] = (uint8_t)((uint32_t)(v >> (8u * (7u - lane))) ^ inv);
                at += 8u;
            } else {
                if (lane < 4u) out[at + lane] = (uint8_t)((fl >> (8u * (3u - lane))) ^ inv);
                at += 4u;
            }
        }
        #pragma unroll 1
        for (uint32_t i = at + lane; i < P.width; i += 64u) out[i] = 0;           // the padding; a meta record's whole row
    }
    if (lane == 0) {
        if (bytes_in) atomicAdd((unsigned long long *)&tot->bytes_in, (unsigned long long)bytes_in);
        if (max_field) atomicMax((unsigned long long *)&tot->max_field, (unsigned long long)max_field);
    }
}

// the smallest record at fault among n fault words, and its kind: kinds[i] for word i; of two faults at one record the earlier word's
__device__ __forceinline__ void za_sort_fault(const unsigned long long *__restrict__ bad, const uint32_t *kinds, uint32_t n, unsigned long long *b, uint32_t *kind)
{
    *b = ~0ull; *kind = 0;
    for (uint32_t i = 0; i < n; i++) if (bad[i] < *b) { *b = bad[i]; *kind = kinds[i]; }
}

// one thread.  nrec > 0.
__global__ void za_k_sort_keys_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint32_t k_lines, uint32_t flags, uint64_t text_end,
                                     uint64_t record_base, uint32_t width, const unsigned long long *__restrict__ bad, ZaSortKeyTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t kinds[3] = {1u, 2u, 3u};
    unsigned long long b; uint32_t kind;
    za_sort_fault(bad, kinds, 3u, &b, &kind);
    tot->covered = 1; tot->seen = nrec; tot->key_width = width;
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, b, kind, tot);
}

// ---- the sort.  key: n rows of W bytes, row-major, never written.  The order array travels, the rows stay: a pass reads one byte of
// every row through the order array (za_k_sort_hist) and keeps it in dig[] for the scatter, so a pass moves 4 + 4 + 1 + 1 bytes per row
// whatever W is.

// grid: any; words = n * W / 8.  acc[0, w8) (zeroed): the OR of every row's word; acc[w8, 2 w8) (all ones): the AND.  Thread t takes the
// words t, t + span, ... with span a multiple of w8, so all of them are the same word of a row.
__global__ __launch_bounds__(256) void za_k_sort_orand(const unsigned long long *__restrict__ key, uint64_t words, uint32_t w8, unsigned long long *__restrict__ acc)
{
    const uint64_t all = (uint64_t)gridDim.x * 256u, span = all / w8 * w8, t = (uint64_t)blockIdx.x * 256u + threadIdx.x;      // (all >= 256 > w8)
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long o = 0, a = ~0ull;
    if (t < span) {
        #pragma unroll 1
        for (uint64_t i = t; i < words; i += span) { const unsigned long long v = key[i]; o |= v; a &= v; }
    }
    uint32_t col = (uint32_t)(t % w8);
    bool mine = t < span && t < words;
    if (!(w8 & (w8 - 1u))) {            // w8 divides 64: the lanes l, l + w8, ... of a wave hold the same word of a row and are combined first
        #pragma unroll
        for (uint32_t d = 32u; d >= 1u; d >>= 1) {
            if (d < w8) break;          // (the same for every thread)
            o |= __shfl_xor(o, (int)d, 64); a &= __shfl_xor(a, (int)d, 64);
        }
        col = lane; mine = lane < w8;   // (a lane without a word of its own holds the identities, and col = t % w8 = lane % w8 here)
    }
    if (mine) { atomicOr(&acc[col], o); atomicAnd(&acc[w8 + col], a); }
}

__global__ __launch_bounds__(256) void za_k_sort_iota(uint32_t *__restrict__ ord, uint32_t n)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) ord[i] = (uint32_t)i;
}

// What a strip of 64 rows adds to the counts a lane keeps: lane l keeps the digit values l, l + 64, l + 128, l + 192.  g: the lane's
// digit; in: the lane holds a row.  Eight ballots tell every lane which lanes hold which value.  -> the lanes that hold this lane's value.
__device__ __forceinline__ uint64_t za_sort_strip(uint32_t g, bool in, uint32_t lane, uint32_t cnt[4])
{
    uint64_t b[8];
    const uint64_t act = __ballot(in);
    #pragma unroll
    for (uint32_t k = 0; k < 8u; k++) b[k] = __ballot(in && (g >> k & 1u));
    uint64_t low = act, own = act;                                                 // the lanes whose low six bits are this lane's number; this lane's digit
    #pragma unroll
    for (uint32_t k = 0; k < 6u; k++) low &= (lane >> k & 1u) ? b[k] : ~b[k];
    #pragma unroll
    for (uint32_t k = 0; k < 8u; k++) own &= (g >> k & 1u) ? b[k] : ~b[k];
    cnt[0] += (uint32_t)__popcll(low & ~b[6] & ~b[7]); cnt[1] += (uint32_t)__popcll(low & b[6] & ~b[7]);
    cnt[2] += (uint32_t)__popcll(low & ~b[6] & b[7]);  cnt[3] += (uint32_t)__popcll(low & b[6] & b[7]);
    return own;
}

// grid: one workgroup per tile; tiles = gridDim.x.  ord[0, n): the order as it stands; d: the byte of the rows this pass sorts by.
// dig[i] = that byte of row ord[i]; tab[v * tiles + tile] = how many rows of the tile hold the value v.  LDS: the four waves' counts.
__global__ __launch_bounds__(256) void za_k_sort_hist(const uint8_t *__restrict__ key, uint32_t W, uint32_t d, const uint32_t *__restrict__ ord, uint32_t n,
                                                      uint8_t *__restrict__ dig, uint32_t *__restrict__ tab)
{
    __shared__ uint32_t s_cnt[4][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * ZA_SORT_TILE + wave * (64u * ZA_SORT_STRIPS);
    uint32_t cnt[4] = {0, 0, 0, 0};
    #pragma unroll
    for (uint32_t s = 0; s < ZA_SORT_STRIPS; s++) {
        const uint64_t i = base + s * 64u + lane;
        const bool in = i < n;
        uint32_t g = 0;
        if (in) {
            const uint32_t o = ord[i];                                             // (below n: the order array is a permutation; the test keeps a wrong one inside the rows)
            g = o < n ? key[(uint64_t)o * W + d] : 0u;
            dig[i] = (uint8_t)g;
        }
        za_sort_strip(g, in, lane, cnt);
    }
    #pragma unroll
    for (uint32_t j = 0; j < 4u; j++) s_cnt[wave][lane + 64u * j] = cnt[j];
    __syncthreads();
    tab[(uint64_t)tid * gridDim.x + blockIdx.x] = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
}

// grid: 256 workgroups, one per digit value v.  tab[v * tiles + t] becomes the rows of value v in the tiles before t; dtot[v] = all
// rows of value v.  256 tiles per turn, the sum so far carried from turn to turn: ceil(tiles / 256) turns.
__global__ __launch_bounds__(256) void za_k_sort_scan(uint32_t *__restrict__ tab, uint32_t tiles, uint32_t *__restrict__ dtot)
{
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t *t = tab + (uint64_t)blockIdx.x * tiles;
    uint32_t carry = 0;
    #pragma unroll 1
    for (uint32_t c0 = 0; c0 < tiles; c0 += 256u) {
        const uint32_t i = c0 + tid, v = i < tiles ? t[i] : 0u;
        const uint32_t incl = za_wave_incl_scan(v);
        if (lane == 63u) s_w[wave] = incl;
        __syncthreads();
        uint32_t pre = 0, all = 0;
        #pragma unroll
        for (uint32_t x = 0; x < 4u; x++) { const uint32_t y = s_w[x]; if (x < wave) pre += y; all += y; }
        if (i < tiles) t[i] = carry + pre + incl - v;
        carry += all;
        __syncthreads();                                                           // (s_w is written again in the next turn)
    }
    if (tid == 0) dtot[blockIdx.x] = carry;
}

// grid: one workgroup per tile, as za_k_sort_hist; dig, tab and dtot as it and za_k_sort_scan left them.  out[place] = in[i] for every
// i < n, and every place is below n (they are a permutation of 0 .. n - 1; the test against n keeps a wrong table from writing
// outside the array).  Stable: among the rows of one value, earlier i gets the lower place.
__global__ __launch_bounds__(256) void za_k_sort_scatter(const uint8_t *__restrict__ dig, const uint32_t *__restrict__ in, uint32_t n, const uint32_t *__restrict__ tab,
                                                         const uint32_t *__restrict__ dtot, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_cnt[4][256];
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * ZA_SORT_TILE + wave * (64u * ZA_SORT_STRIPS);
    uint32_t cnt[4] = {0, 0, 0, 0};
    #pragma unroll 2
    for (uint32_t s = 0; s < ZA_SORT_STRIPS; s++) {
        const uint64_t i = base + s * 64u + lane;
        za_sort_strip(i < n ? dig[i] : 0u, i < n, lane, cnt);
    }
    #pragma unroll
    for (uint32_t j = 0; j < 4u; j++) s_cnt[wave][lane + 64u * j] = cnt[j];
    {   // the rows of the values below tid, in all tiles
        const uint32_t v = dtot[tid], incl = za_wave_incl_scan(v);
        if (lane == 63u) s_w[wave] = incl;
        __syncthreads();
        uint32_t pre = 0;
        for (uint32_t x = 0; x < wave; x++) pre += s_w[x];
        s_base[tid] = pre + incl - v + tab[(uint64_t)tid * gridDim.x + blockIdx.x];
    }
    __syncthreads();
    uint32_t run[4];                                                               // where the next row of this lane's four values goes
    #pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t v = lane + 64u * j;
        uint32_t a = s_base[v];
        for (uint32_t x = 0; x < wave; x++) a += s_cnt[x][v];
        run[j] = a;
    }
    #pragma unroll 2
    for (uint32_t s = 0; s < ZA_SORT_STRIPS; s++) {
        const uint64_t i = base + s * 64u + lane;
        const bool on = i < n;
        const uint32_t gs = on ? dig[i] : 0u;                                      // (read a second time: eight digits kept per lane cost more registers than the reload)
        uint32_t add[4] = {0, 0, 0, 0};
        const uint64_t own = za_sort_strip(gs, on, lane, add);
        const int src = (int)(gs & 63u);
        const uint32_t r0 = (uint32_t)__shfl((int)run[0], src, 64), r1 = (uint32_t)__shfl((int)run[1], src, 64);
        const uint32_t r2 = (uint32_t)__shfl((int)run[2], src, 64), r3 = (uint32_t)__shfl((int)run[3], src, 64);
        const uint32_t hi2 = gs >> 6;
        const uint32_t place = (hi2 == 0u ? r0 : hi2 == 1u ? r1 : hi2 == 2u ? r2 : r3) + (uint32_t)__popcll(own & ((1ull << lane) - 1ull));
        if (on && place < n) out[place] = in[i];
        #pragma unroll
        for (uint32_t j = 0; j < 4u; j++) run[j] += add[j];
    }
}

__global__ __launch_bounds__(256) void za_k_sort_rank(const uint32_t *__restrict__ ord, uint32_t n, uint32_t *__restrict__ rank)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = ord[j];
    if (r < n) rank[r] = (uint32_t)j;
}

// ---- records placed.  grid: as za_k_sort_keys.  dst[r], length[r] for r < nrec (the host launches nothing when the arrays are
// shorter).  A record with dst = ZA_SORT_SKIP is not looked at beyond its first byte.  bad (three words behind tot, ~0 beforehand): the
// smallest r whose first byte is not first_byte, whose length in the text (with the delimiter an open last line gets) is not
// length[r], whose bytes do not fit below out_cap.  A record at fault is not copied; every byte written lies in
// out[dst[r], dst[r] + length[r]) with dst[r] + length[r] <= out_cap, and every byte read in the record.  No barrier, no LDS.
__global__ __launch_bounds__(256) void za_k_sort_place(const uint8_t *__restrict__ scratch, uint64_t text_end, const unsigned long long *__restrict__ start, uint64_t lines,
                                                       uint64_t nrec, uint32_t k_lines, int32_t first_byte, uint32_t delim, uint32_t final,
                                                       const unsigned long long *__restrict__ dst, const uint32_t *__restrict__ length, uint8_t *__restrict__ out,
                                                       uint64_t out_cap, ZaPlaceTotals *__restrict__ tot)
{
    unsigned long long *bad = (unsigned long long *)(tot + 1);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint64_t stride = (uint64_t)gridDim.x * 4u;
    uint64_t placed = 0, bytes = 0;
    #pragma unroll 1
    for (uint64_t r = (uint64_t)blockIdx.x * 4u + wave; r < nrec; r += stride) {
        const uint64_t lo = (uint64_t)k_lines * r, hi = lines - lo < k_lines ? lines : lo + k_lines;
        const uint64_t ra = start[lo], re = start[hi];
        const uint32_t rlen = re > ra ? (uint32_t)(re - ra) : 0u;
        if (lane == 0 && first_byte >= 0 && !(ra < text_end && scratch[ra] == (uint32_t)first_byte)) atomicMin(&bad[0], (unsigned long long)r);
        const unsigned long long d = dst[r];
        if (d == ZA_SORT_SKIP) continue;
        const bool open = final && hi == lines && rlen && scratch[re - 1u] != delim;
        const uint32_t want = length[r];
        if (rlen + (open ? 1u : 0u) != want) { if (lane == 0) atomicMin(&bad[1], (unsigned long long)r); continue; }
        if (d > out_cap || want > out_cap - d) { if (lane == 0) atomicMin(&bad[2], (unsigned long long)r); continue; }
        const uint8_t *s = scratch + ra;
        uint8_t *o = out + d;
        #pragma unroll 4
        for (uint32_t i = lane; i < rlen; i += 64u) o[i] = s[i];
        if (open && lane == 0) o[rlen] = (uint8_t)delim;
        placed++; bytes += want;
    }
    if (lane == 0 && placed) {
        atomicAdd((unsigned long long *)&tot->placed, (unsigned long long)placed);
        atomicAdd((unsigned long long *)&tot->placed_bytes, (unsigned long long)bytes);
    }
}

// one thread.  nrec > 0.  launched: za_k_sort_place ran (the arrays cover the records).
__global__ void za_k_sort_place_close(const unsigned long long *__restrict__ start, uint64_t lines, uint64_t nrec, uint64_t narr, uint32_t k_lines, uint32_t flags,
                                      uint64_t text_end, uint64_t record_base, const unsigned long long *__restrict__ bad, ZaPlaceTotals *__restrict__ tot)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t kinds[3] = {1u, 4u, 5u};
    unsigned long long b; uint32_t kind;
    za_sort_fault(bad, kinds, 3u, &b, &kind);
    tot->covered = 1; tot->seen = nrec; tot->labels_short = narr < nrec ? 1u : 0u;
    za_rec_close(start, lines, nrec, k_lines, flags, text_end, record_base, b, kind, tot);
}

/*
 * zng_amd.h -- C ABI of the MI355X-native DEFLATE / inflate engine (libzng_amd.so).
 *
 * This is the drop-in boundary for the hot path of pycompression/python-zlib-ng: the entry points
 * below are what a binding of the reference would call instead of the zlib-ng `zng_*` functions it
 * uses today.  Plain pointers and sizes only; no Python, no torch types.  Every function that
 * compresses, decompresses or checksums runs hand-written HIP kernels on the GPU -- there is no CPU
 * fallback, and a missing / unusable GPU is an error (ZNGAMD_E_HIP).
 *
 * Reference interface each group replaces (file:line in the reference tree):
 *   zngamd_deflate_blocks*      ParallelCompress_compress_and_crc      src/zlib_ng/zlib_ngmodule.c:1696-1782
 *                               (zng_deflateReset :1725, zng_deflateSetDictionary :1735,
 *                                zng_crc32_z :1741, zng_deflate(Z_SYNC_FLUSH) :1742), batched over the
 *                               blocks that gzip_ng_threaded.py:299-322 cuts and round-robins
 *   zngamd_level_ok             level validation of zng_deflateInit2    zlib_ngmodule.c:1645-1658
 *   zngamd_deflate_stream       zlib_compress_impl body                 zlib_ngmodule.c:199-273
 *   zngamd_inflate*             zng_inflate call sites                  zlib_ngmodule.c:328, :2539
 *   zngamd_gzip_scan / _members GzipReader_read_into_buffer             zlib_ngmodule.c:2426-2637
 *   zngamd_crc32 / _adler32     zlib_crc32 / zlib_adler32               zlib_ngmodule.c:1455-1562
 *   zngamd_crc32_combine        zlib_crc32_combine                      zlib_ngmodule.c:1585-1596
 */
#ifndef ZNG_AMD_H
#define ZNG_AMD_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zngamd_ctx zngamd_ctx;

/* status codes: zlib numbering for the codec, -2xx for the engine */
#define ZNGAMD_OK              0
#define ZNGAMD_STREAM_END      1
#define ZNGAMD_NEED_DICT       2
#define ZNGAMD_STREAM_ERROR  (-2)
#define ZNGAMD_DATA_ERROR    (-3)
#define ZNGAMD_MEM_ERROR     (-4)
#define ZNGAMD_BUF_ERROR     (-5)
#define ZNGAMD_E_GZ_MAGIC    (-101)
#define ZNGAMD_E_GZ_METHOD   (-102)
#define ZNGAMD_E_GZ_HCRC     (-103)
#define ZNGAMD_E_GZ_CRC      (-104)
#define ZNGAMD_E_GZ_LENGTH   (-105)
#define ZNGAMD_E_GZ_TRUNC    (-106)
#define ZNGAMD_E_HIP         (-201)   /* HIP runtime error or no usable GPU */
#define ZNGAMD_E_ARG         (-202)
#define ZNGAMD_E_OVERFLOW    (-203)   /* a block's compressed output reached its buffer size */
#define ZNGAMD_E_INDEX       (-204)   /* a segment index does not fit its stream: decode the stream without the index */

#define ZNGAMD_FLAG_FINAL      1u     /* block ends the deflate stream (BFINAL=1, no sync flush) */
#define ZNGAMD_FLAG_FLATHDR    2u     /* dynamic block headers in their flat form: the code-length code is the fixed 4-bit
                                         code of the symbols 0..15, so a decoder finds every code length at a known bit offset
                                         (what zngamd_gzip_members* writes; any inflater reads it as an ordinary dynamic header) */
#define ZNGAMD_FLAG_SEG2K      16u    /* segments of 2 KiB whatever the block's size (small blocks take smaller ones otherwise): what the
                                       * segment index of a dict-chained stream is counted in (zngamd_deflate_index) */
#define ZNGAMD_FLAG_UNITS16K   32u    /* the block is cut into units of 16 KiB (deflate blocks of their own, each with the 32 KiB before it as
                                        its dictionary) instead of 128 KiB: latency before size -- what zngamd_deflate_stream does by itself for
                                        inputs of up to 128 KiB (r06; +0.2 .. 1.2 % of compressed size, a 64 KiB call 970 -> 435 us) */
/* window of the stream the blocks belong to: match distances stay within 2^bits (deflateInit2's windowBits 9..15).
 * Taken from the FIRST block of a call and applied to all of them; 0 = 15. */
#define ZNGAMD_FLAG_WBITS(bits) (((uint32_t)(bits) & 15u) << 8)
/* compression strategy of the blocks (deflateInit2's strategy, ZNGAMD_STRATEGY_*).  Like the window, taken from the FIRST block
 * of a call and applied to all of them; 0 = the default.  Level 0 writes stored blocks whatever the strategy, as zlib does. */
#define ZNGAMD_FLAG_STRATEGY(s) (((uint32_t)(s) & 7u) << 12)
#define ZNGAMD_STRATEGY_OF(flags) ((int)(((flags) >> 12) & 7u))
#define ZNGAMD_STRATEGY_DEFAULT      0   /* Z_DEFAULT_STRATEGY */
#define ZNGAMD_STRATEGY_FILTERED     1   /* Z_FILTERED: matches of 5 bytes or fewer are not taken */
#define ZNGAMD_STRATEGY_HUFFMAN_ONLY 2   /* Z_HUFFMAN_ONLY: literals only, no match search */
#define ZNGAMD_STRATEGY_RLE          3   /* Z_RLE: matches of distance 1 only (runs), no match search */
#define ZNGAMD_STRATEGY_FIXED        4   /* Z_FIXED: fixed-code blocks (or stored), never a dynamic block */

#define ZNGAMD_UNIT_MAX        131072u  /* largest span one kernel unit covers */
#define ZNGAMD_SLOT_STRIDE     131136u  /* bytes reserved per unit in a device slot buffer */
#define ZNGAMD_SEG             2048u    /* parse / index segment */

/* ---- context ---- */
int         zngamd_device_count(void);
int         zngamd_ctx_create(int device, zngamd_ctx **out);
void        zngamd_ctx_destroy(zngamd_ctx *ctx);
const char *zngamd_last_error(zngamd_ctx *ctx);     /* message of the calling thread's last failing call (thread-local) */
const char *zngamd_version(void);
/* run all work of this context on a caller-owned hipStream_t (pass NULL to go back to the own stream) */
int         zngamd_set_stream(zngamd_ctx *ctx, void *hip_stream);
int         zngamd_sync(zngamd_ctx *ctx);

/* device memory helpers for callers that have no allocator of their own */
int zngamd_dmalloc(zngamd_ctx *ctx, size_t bytes, void **dptr);
int zngamd_dfree(zngamd_ctx *ctx, void *dptr);
int zngamd_h2d(zngamd_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int zngamd_d2h(zngamd_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* device-to-device copy / fill on the context's stream (ordered with the engine's kernels, no host synchronisation), and the
 * device's free / total memory: what a harness needs to do without a tensor library (bench.py) */
int zngamd_d2d(zngamd_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
int zngamd_dmemset(zngamd_ctx *ctx, void *dst_dev, int value, size_t bytes);
int zngamd_mem_info(zngamd_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- checksums (GPU) ---- */
int      zngamd_crc32(zngamd_ctx *ctx, uint32_t crc, const uint8_t *buf, size_t len, uint32_t *out);
int      zngamd_adler32(zngamd_ctx *ctx, uint32_t adler, const uint8_t *buf, size_t len, uint32_t *out);
int      zngamd_crc32_dev(zngamd_ctx *ctx, uint32_t crc, const void *dbuf, size_t len, uint32_t *out);
/* scalar GF(2) arithmetic on three integers (no data pass) */
uint32_t zngamd_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);
/* the same over a run of pieces: crc of (what `crc` covers, followed by n pieces of lens[i] bytes whose CRC-32s are crcs[i]) -- the fold
 * the reference's writer thread does block by block (src/zlib_ng/gzip_ng_threaded.py:392-396), as one call */
uint32_t zngamd_crc32_combine_many(uint32_t crc, const uint32_t *crcs, const uint64_t *lens, uint32_t n);

/* ---- deflate ---- */
int zngamd_level_ok(int level);   /* 1 for -1..9, else 0 ("Bad compression level") */

typedef struct {
    uint64_t off;        /* offset of the block's first byte in `in` */
    uint32_t len;        /* block length (any size; cut into <=128 KiB units inside) */
    uint32_t dict_len;   /* bytes of `in` directly before `off` that prime the window (<= 32768) */
    uint32_t flags;      /* ZNGAMD_FLAG_FINAL | ZNGAMD_FLAG_WBITS(n) | ZNGAMD_FLAG_STRATEGY(s) */
    uint32_t reserved;
} zngamd_block;

/* Compress n_blocks independent blocks of a host buffer.  Block b's raw-deflate bytes go to
 * out + b*out_cap_per_block, its size to out_len[b], the CRC-32 of its input to crc[b].  Each block
 * ends on a byte boundary with a sync-flush marker (00 00 FF FF) unless FINAL.  A block whose output
 * reaches out_cap_per_block gets out_len[b] = 0xFFFFFFFF and the call returns ZNGAMD_E_OVERFLOW. */
int zngamd_deflate_blocks(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len,
                          const zngamd_block *blocks, uint32_t n_blocks, int level,
                          uint8_t *out, uint64_t out_cap_per_block,
                          uint32_t *out_len, uint32_t *crc);

/* The same blocks, their outputs back to back in `out` (block b at the sum of out_len[0 .. b-1]; *total = all of them): what a
 * writer that only concatenates the blocks needs (the reference's writer thread, src/zlib_ng/gzip_ng_threaded.py:382-398) --
 * the packed stream is copied from the device straight into `out`, no per-block slots in between.  A block whose output
 * reaches block_cap is an overflow as above (ZNGAMD_E_OVERFLOW, out_len[b] = 0xFFFFFFFF; `out` is then not to be used);
 * ZNGAMD_BUF_ERROR with *total = the size needed when out_cap is too small. */
int zngamd_deflate_blocks_packed(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len,
                                 const zngamd_block *blocks, uint32_t n_blocks, int level,
                                 uint8_t *out, uint64_t out_cap, uint64_t block_cap,
                                 uint32_t *out_len, uint32_t *crc, uint64_t *total);

/* Device-resident form.  d_in holds the input; blocks are cut into units as above.
 * d_slots must hold n_units * ZNGAMD_SLOT_STRIDE bytes, where n_units = zngamd_count_units(...).
 * Per-unit results stay on the device: d_unit_len[u], d_unit_crc[u]; unit -> block map in h_unit_block
 * (host, optional).  zngamd_gather_dev then packs the used bytes of the slots contiguously. */
uint32_t zngamd_count_units(const zngamd_block *blocks, uint32_t n_blocks);
int zngamd_deflate_blocks_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len,
                              const zngamd_block *blocks, uint32_t n_blocks, int level,
                              void *d_slots, uint32_t *d_unit_len, uint32_t *d_unit_crc,
                              uint32_t *h_unit_block);
/* The same blocks straight into ONE contiguous stream at d_out (what zngamd_deflate_blocks_dev + zngamd_gather_dev leave at
 * d_dst, without the slots and without the copy: every unit's exact size is known before it is packed, a prefix sum places it).
 * Per unit: d_unit_len, d_unit_crc and (optional) d_unit_off = its byte offset in the stream; *total_bytes (host) = the
 * stream's size.  ZNGAMD_BUF_ERROR with *total_bytes = the size needed when out_cap is too small.  Replaces, for a batch of
 * blocks, the copies of ParallelCompress_compress_and_crc's results (reference src/zlib_ng/zlib_ngmodule.c:1765-1777) and the
 * in-order concatenation of the writer thread (src/zlib_ng/gzip_ng_threaded.py:382-398). */
int zngamd_deflate_blocks_packed_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len,
                                     const zngamd_block *blocks, uint32_t n_blocks, int level,
                                     void *d_out, uint64_t out_cap, uint32_t *d_unit_len, uint32_t *d_unit_crc,
                                     uint64_t *d_unit_off, uint64_t *total_bytes);
/* ---- the writer's segment index for a dict-chained stream (r06).  A batch compressed with ZNGAMD_FLAG_FLATHDR on its blocks
 * (one Huffman block per unit with the header in its flat form, 2 KiB segments) leaves, per unit, ZNGAMD_INDEX_STRIDE u32: entry s
 * = bit offset of the first token of segment s from the unit's first byte, entry nseg = bit offset of the end-of-block code, the
 * rest zeros (all zeros: a unit of stored blocks).  zngamd_deflate_index_dev copies the index of the context's LAST deflate call
 * (n_units as zngamd_count_units gave it) to device memory of the caller.  zngamd_inflate_units_indexed_dev decodes such a
 * stream -- what the reference's threaded writer frames as one gzip member (gzip_ng_threaded.py:299-338), and what
 * GzipReader_read_into_buffer (zlib_ngmodule.c:2426-2637) reads with one zng_inflate stream -- unit-parallel: a lane per 2 KiB
 * segment decodes, matches that reach in front of their unit become markers, the window kernels of the chunk-parallel inflate
 * resolve them.  unit_in_len / unit_out_len are HOST arrays (compressed bytes of a unit including its sync marker; its output
 * bytes), d_index device memory, d_dict / dict_len the history in front of the first unit (may be NULL / 0).  Returns
 * ZNGAMD_STREAM_END with *out_len, ZNGAMD_BUF_ERROR with the size needed, ZNGAMD_E_INDEX when stream and index do not fit (the
 * caller then decodes with zngamd_inflate_raw_dev), ZNGAMD_DATA_ERROR for invalid deflate data.
 * d_def must be readable for 64 bytes past def_len (the decoder's look-ahead, as for the other device entry points); the three
 * index arrays may hold anything: every number in them is checked against the stream before a byte is handed out (see DESIGN.md
 * section 5, "What pins the index"), so ZNGAMD_STREAM_END means the bytes any inflater decodes from the sum(unit_in_len) bytes
 * the units cover (whether those are all of the stream is the caller's to compare: the call does not look behind them) -- an index the
 * checks cannot vouch for is ZNGAMD_E_INDEX (or ZNGAMD_DATA_ERROR where a wrong entry sends a lane into the middle of a code).
 * A unit with unit_out_len 0 must be the empty unit the packer writes (00 00 00 FF FF, or 03 00 closing the stream).  Also
 * ZNGAMD_E_INDEX: a batch of units (ZNGAMD_UNIT_BATCH, default 16 384) that starts behind fewer than 32 768 bytes of output --
 * units of a few hundred bytes; such a stream is decoded without its index. */
#define ZNGAMD_INDEX_STRIDE 68
int zngamd_deflate_index_dev(zngamd_ctx *ctx, uint32_t *d_index, uint32_t n_units);
int zngamd_inflate_units_indexed_dev(zngamd_ctx *ctx, const void *d_def, uint64_t def_len, const uint32_t *unit_in_len,
                                     const uint32_t *unit_out_len, uint32_t n_units, const uint32_t *d_index,
                                     const void *d_dict, uint32_t dict_len, void *d_out, uint64_t out_cap, uint64_t *out_len);

/* Packs unit slots back to back at d_dst + dst_base; returns the total in *total_bytes (host).
 * d_unit_off (device, n_units x u64, may be NULL) receives each unit's byte offset. */
int zngamd_gather_dev(zngamd_ctx *ctx, const void *d_slots, const uint32_t *d_unit_len, uint32_t n_units,
                      void *d_dst, uint64_t dst_base, uint64_t dst_cap, uint64_t *d_unit_off,
                      uint64_t *total_bytes);

/* One whole raw-deflate stream from a host buffer: units chained through the previous 32 KiB of
 * input, last block FINAL.  window_bits 9..15 bounds match distances to 2^window_bits (the window a
 * decoder opened with that wbits keeps).  Returns the size in *out_len, CRC-32 and Adler-32 of the input. */
int zngamd_deflate_stream(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, int level, int window_bits,
                          uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                          uint32_t *crc, uint32_t *adler);

/* ---- inflate ---- */
/* Raw RFC 1951 stream from a host buffer, optional preset dictionary.  Returns ZNGAMD_STREAM_END when
 * a final block ended, ZNGAMD_BUF_ERROR when input ran out or out_cap was reached (distinguish with
 * *out_len == out_cap), ZNGAMD_DATA_ERROR on invalid data.  *in_used = bytes consumed.
 * Complete streams of at least 64 KiB without a dictionary are decoded chunk-parallel (see zngamd_gunzip,
 * path 3); for those an output buffer that is too small gives ZNGAMD_BUF_ERROR with *out_len > out_cap =
 * the size the stream needs, and nothing is copied. */
int zngamd_inflate_raw(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len,
                       const uint8_t *dict, uint32_t dict_len,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *in_used,
                       uint32_t *crc, uint32_t *adler);

/* Resumable form for incremental readers (decompressobj).  Decoding starts `start_bit` (0..7) bits into
 * in[0] with `dict` as history.  Besides the totals it reports the last deflate-block header that was
 * entered (*block_bits from bit 0 of `in`, *block_out bytes produced before it): when the call ends with
 * ZNGAMD_BUF_ERROR (input ran out), the caller keeps in[*block_bits/8 ..], the last 32 KiB of output up to
 * *block_out, and calls again once more input has arrived.  ZNGAMD_E_OVERFLOW = out_cap reached.
 * Pieces of at least 64 KiB are decoded chunk-parallel up to their last complete block (then *out_len == *block_out:
 * the incomplete block is not decoded at all; with ZNGAMD_STREAM_END the checkpoint is a block header that was entered, not
 * necessarily the last one); smaller pieces run on the sequential wavefront decoder. */
int zngamd_inflate_resume(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t start_bit,
                          const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t out_cap,
                          uint64_t *out_len, uint64_t *in_bits, uint64_t *block_bits, uint64_t *block_out);
/* what the chunk-parallel decoder of streams without an index (zngamd_gunzip path 3, large zngamd_inflate_raw / _resume calls) found
 * since the last reset, summed over every attempt that completed its list of chunk boundaries: out[0] hits of the sync-marker scan
 * (00 00 FF FF), out[1] bit offsets that passed the first test of the block-header finder (0 where sync markers were dense enough
 * and the finder did not run), out[2] boundaries after sorting and removing duplicates, the start of the stream among them,
 * out[3] chunks of the attempts that produced the call's bytes.  A header the finder misses costs speed, never bytes: these
 * numbers are the only place where a miss shows.  Costs no launch and no synchronisation. */
int zngamd_chunk_stats(zngamd_ctx *ctx, uint64_t *out /*[4]*/, int reset);

/* gzip member table entry produced by the index scan (pass 1) */
typedef struct {
    uint64_t in_off;       /* offset of the member's first deflate byte */
    uint64_t in_len;       /* deflate bytes (0 = unknown: decode sequentially)                     */
    uint64_t out_off;      /* offset of the member's first output byte                             */
    uint32_t out_len;      /* ISIZE                                                                 */
    uint32_t crc;          /* CRC-32 from the trailer                                               */
    uint32_t index_off;    /* bytes from the start of the chunk index to in_off, 0 = no index       */
    uint32_t nseg;         /* index entries - 1 = ceil(out_len / 256)                              */
} zngamd_member;

/* Pass 1 on the device: find every member of a multi-member stream written by this engine
 * (FEXTRA subfield 'Z','A' carrying member size, ISIZE and the chunk bit index).  d_members must
 * hold max_members entries; *n_members / *total_out on the host.  Returns ZNGAMD_E_ARG when the
 * stream is not fully made of indexed members (caller then uses the sequential reader). */
int zngamd_gzip_scan_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len,
                         zngamd_member *d_members, uint32_t max_members,
                         uint32_t *n_members, uint64_t *total_out);
/* Pass 2: decode all members (one wavefront per member, one lane per 2 KiB segment of the chunk index:
 * symbols decoded through LDS tables, matches resolved in an LDS image of the segment), verify CRC-32 and
 * ISIZE.  d_status[m] receives a ZNGAMD_* code per member. */
int zngamd_gzip_inflate_members_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len,
                                    const zngamd_member *d_members, uint32_t n_members,
                                    void *d_out, uint64_t out_cap, int32_t *d_status);

/* Pass 2 for members WITHOUT this engine's index whose extent is known (BGZF 'B','C' members, members written by any
 * gzip with their sizes recorded by the caller): d_members[i].index_off = 0, in_off / in_len = the member's deflate bytes
 * (the 8-byte trailer follows them), out_off / out_len = where its ISIZE bytes go.  One wavefront per member (64
 * self-synchronising sub-sequences inside every Huffman block), CRC-32 / ISIZE verified against the trailer. */
int zngamd_gzip_inflate_plain_members_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len,
                                          const zngamd_member *d_members, uint32_t n_members,
                                          void *d_out, uint64_t out_cap, int32_t *d_status);

/* ---- spans of a seek-point index (zlib_ng_amd/gzip_index.py): pieces of gzip members' deflate data that decode on their own.
 * A span starts at a deflate block header, absolute bit in_bit of d_in, with win_len (0..32768) bytes of d_windows at win_off as
 * history.  It ends at the block header at absolute bit end_bit, or where its member's final block ends (end_bit = that end
 * rounded up to a whole byte).  It must produce exactly out_len bytes (at out_off of d_out) whose CRC-32 is crc.  One 64-lane
 * wavefront per span, all spans in one launch.  d_in must hold ZNGAMD_SPAN_PAD readable bytes behind the end of every span; no
 * span reads outside [in_bit / 8, end_bit / 8 + ZNGAMD_SPAN_PAD) or writes outside its output range.  d_status[i] receives a
 * ZNGAMD_SPAN_* code (an entry that points outside the buffers is ZNGAMD_SPAN_DATA). */
typedef struct {
    uint64_t in_bit, end_bit;
    uint64_t win_off, out_off;
    uint32_t win_len, out_len;
    uint32_t crc, reserved;
} zngamd_span;
#define ZNGAMD_SPAN_OK     0
#define ZNGAMD_SPAN_DATA   1
#define ZNGAMD_SPAN_LENGTH 2
#define ZNGAMD_SPAN_CRC    3
#define ZNGAMD_SPAN_PAD    64
int zngamd_inflate_spans_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_span *d_spans, uint32_t n,
                             const void *d_windows, uint64_t windows_len, void *d_out, uint64_t out_cap, int32_t *d_status);
/* Host-buffer form: stages in (padded here), the span table and the windows, launches once, copies the statuses (n entries)
 * and out_cap bytes of output back.  Returns ZNGAMD_OK when the call ran; the verdict per span is in status[]. */
int zngamd_inflate_spans(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_span *spans, uint32_t n,
                         const uint8_t *windows, uint64_t windows_len, uint8_t *out, uint64_t out_cap, int32_t *status);
/* what the span decoder did since the last reset: out[0] spans launched (either form), out[1] output bytes of the spans that
 * zngamd_inflate_spans decoded with ZNGAMD_SPAN_OK (the device form leaves its statuses on the device and does not count bytes) */
int zngamd_span_stats(zngamd_ctx *ctx, uint64_t *out /*[2]*/, int reset);

/* ---- the batch API (zlib_ng_amd/batch.py): many independent streams per call.  One 64-lane wavefront per item, all items of a call in
 * one launch; a status per item.  Items lie anywhere in one input buffer (in_off, in_len); each decodes into its own output range
 * (out_off, out_cap).  Tables given to the device forms are untrusted: an entry that points outside the buffers gets
 * ZNGAMD_BATCH_TABLE and nothing of it is read or written. */
typedef struct { uint64_t in_off, out_off; uint32_t in_len, out_cap; uint32_t reserved[2]; } zngamd_batch_item;     /* 32 B */
typedef struct { int32_t status; uint32_t out_len; uint32_t in_used; uint32_t reserved; } zngamd_batch_result;   /* 16 B */
#define ZNGAMD_BATCH_OK        0
#define ZNGAMD_BATCH_TRUNCATED 1    /* Z_BUF_ERROR: the stream or its trailer needs bytes beyond the item ("incomplete or truncated stream") */
#define ZNGAMD_BATCH_OUTFULL   2    /* out_cap reached: not an error, the item's size comes from a count-only pass */
#define ZNGAMD_BATCH_NEED_DICT 3    /* Z_NEED_DICT: a zlib header with FDICT */
#define ZNGAMD_BATCH_HEADER    4    /* "incorrect header check" */
#define ZNGAMD_BATCH_WINDOW    5    /* "invalid window size" */
#define ZNGAMD_BATCH_METHOD    6    /* "unknown compression method" (gzip) */
#define ZNGAMD_BATCH_FLAGS     7    /* "unknown header flags set" (gzip) */
#define ZNGAMD_BATCH_HCRC      8    /* "header crc mismatch" (gzip FHCRC) */
#define ZNGAMD_BATCH_DATA      9    /* invalid deflate data */
#define ZNGAMD_BATCH_CHECK     10   /* "incorrect data check" (Adler-32 / CRC-32) */
#define ZNGAMD_BATCH_LENGTH    11   /* "incorrect length check" (gzip ISIZE) */
#define ZNGAMD_BATCH_TABLE     12   /* the table entry lies outside the buffers */
#define ZNGAMD_BATCH_PAD       64   /* readable bytes the device input must hold behind in_len */
/* the host forms hand their output to memory the caller allocates once the size is known: alloc(user, bytes) returns it (NULL = fail) */
typedef void *(*zngamd_alloc_fn)(void *user, uint64_t bytes);
/* Decode: wbits takes zlib_ng.decompress's classes (zlib 0 / 8..15, raw -8..-15, gzip 16 / 24..31, auto 32 / 40..47 per item by its first
 * two bytes).  Device form: one launch over d_items (in device memory); count_only: the same walk and checks with nothing stored,
 * out_len = the exact output size (d_out may be NULL).  d_results[i] gets status, out_len, in_used (bytes up to the trailer's end). */
int zngamd_inflate_batch_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_batch_item *d_items, uint32_t n, int wbits,
                             int count_only, void *d_out, uint64_t out_cap, zngamd_batch_result *d_results);
/* Host form: items (host) give in_off / in_len and a room guess out_cap (0: the engine guesses: gzip ISIZE, else a multiple of in_len);
 * an item that outgrows its room is sized by a count pass and decoded again with exactly that room.  On return items[i].out_off /
 * out_cap say where item i's output lies in the buffer alloc() gave, results[i] what became of it. */
int zngamd_inflate_batch(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int wbits,
                         zngamd_alloc_fn alloc, void *user, zngamd_batch_result *results);
/* Encode: every item becomes the stream zngamd_deflate_stream + the one-shot's container would write for it (wbits: zlib_ng.compress's
 * classes; strategy: ZNGAMD_STRATEGY_*).  items: HOST table (in_off, in_len read; out_off written); the framed items lie back to back
 * in d_out, results[i].out_len bytes each.  *total = the bytes written; ZNGAMD_BUF_ERROR with *total = the size needed when out_cap is
 * too small.  Device form: d_in holds ZNGAMD_BATCH_PAD readable bytes behind in_len; d_results in device memory. */
int zngamd_deflate_batch_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                             int strategy, void *d_out, uint64_t out_cap, zngamd_batch_result *d_results, uint64_t *total);
int zngamd_deflate_batch(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                         int strategy, zngamd_alloc_fn alloc, void *user, zngamd_batch_result *results, uint64_t *total);
/* The batch API with one preset dictionary shared by every item of the call (zdict).  dict: HOST memory, dict_len bytes; the library
 * works out its Adler-32 once and keeps its last 32 KiB, as zngamd_stream_*_set_dictionary do.
 * Decode: a zlib item with FDICT decodes with the dictionary when its DICTID is the dictionary's Adler-32 (else ZNGAMD_ZDICT_MISMATCH;
 * an item that ends inside its DICTID is ZNGAMD_BATCH_TRUNCATED), a raw item has it as history from its first byte, a gzip item or a
 * zlib item without FDICT ignores it.  dict_len == 0: the call is zngamd_inflate_batch[_dev] (FDICT items get ZNGAMD_BATCH_NEED_DICT).
 * Encode: every item becomes the stream zngamd_stream_deflate_* writes for it after zngamd_stream_deflate_set_dictionary (one block,
 * FDICT + DICTID in a zlib header, the Adler-32 of the item's own bytes); dict == NULL: the call is zngamd_deflate_batch[_dev];
 * dict_len == 0 with a non-NULL dict is an empty dictionary (FDICT is written).  A gzip wbits is ZNGAMD_STREAM_ERROR ("Invalid
 * dictionary").  Every item is primed with the tail in a staging buffer: the device form runs its items in ranges of at most
 * 256 MiB of (tail + item) each, whatever n is. */
#define ZNGAMD_ZDICT_MISMATCH  13   /* a zlib item's DICTID is not the Adler-32 of the dictionary ("Error -3 while setting zdict") */
int zngamd_inflate_batch_dict_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_batch_item *d_items, uint32_t n, int wbits,
                                  const uint8_t *dict, uint32_t dict_len, int count_only, void *d_out, uint64_t out_cap, zngamd_batch_result *d_results);
int zngamd_inflate_batch_dict(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int wbits,
                              const uint8_t *dict, uint32_t dict_len, zngamd_alloc_fn alloc, void *user, zngamd_batch_result *results);
int zngamd_deflate_batch_dict_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                                  int strategy, const uint8_t *dict, uint32_t dict_len, void *d_out, uint64_t out_cap,
                                  zngamd_batch_result *d_results, uint64_t *total);
int zngamd_deflate_batch_dict(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, zngamd_batch_item *items, uint32_t n, int level, int wbits,
                              int strategy, const uint8_t *dict, uint32_t dict_len, zngamd_alloc_fn alloc, void *user,
                              zngamd_batch_result *results, uint64_t *total);
/* A preset dictionary trained from sample records (a deterministic FastCOVER variant; segments of k bytes
 * scored by the d-mers, 4 <= d <= 8, they share with all samples).  The samples are the items in table order (in_off, in_len read);
 * d_in holds ZNGAMD_BATCH_PAD readable bytes behind in_len, d_items lies in device memory.  dict: HOST memory of dict_size bytes, the
 * result fills dict[0 .. *dict_len), *dict_len <= dict_size; it depends only on the sample bytes, their order and the parameters.
 * ZNGAMD_E_ARG before any device work unless n >= 1, d <= dict_size <= 32768, 4 <= d <= 8 and d <= k <= 16384; ZNGAMD_E_ARG also for an
 * item outside [0, in_len) or samples that add up to fewer than k bytes or to 4 GiB or more (nothing written to dict). */
int zngamd_train_dict_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_batch_item *d_items, uint32_t n,
                          uint32_t dict_size, uint32_t k, uint32_t d, uint8_t *dict, uint32_t *dict_len);
int zngamd_train_dict(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_batch_item *items, uint32_t n,
                      uint32_t dict_size, uint32_t k, uint32_t d, uint8_t *dict, uint32_t *dict_len);

/* One raw deflate stream that lies in device memory (d_in must be readable 64 bytes past in_len), decoded into device
 * memory: chunk-parallel where the stream offers block boundaries (sync-flush points, dynamic block headers), else on one
 * wavefront.  Returns ZNGAMD_STREAM_END when the final block ended; *out_len = bytes produced, *in_used = bytes consumed. */
int zngamd_inflate_raw_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, void *d_out, uint64_t out_cap,
                           uint64_t *out_len, uint64_t *in_used);

/* CRC-32 of the concatenation of n pieces from their CRC-32s (a device array, e.g. the d_unit_crc of
 * zngamd_deflate_blocks_dev): pieces 0 .. n-2 are each_len bytes long, the last one last_len -- the in-order fold of the
 * reference's writer thread (gzip_ng_threaded.py:394), GF(2) arithmetic on the host. */
int zngamd_crc32_fold_dev(zngamd_ctx *ctx, const uint32_t *d_crcs, uint32_t n, uint64_t each_len, uint64_t last_len, uint32_t *crc);

/* Number of differing 4-byte words (bytes in the tail) of two device buffers: the round-trip check of device-resident callers. */
int zngamd_compare_dev(zngamd_ctx *ctx, const void *d_a, const void *d_b, uint64_t n, uint64_t *mismatches);

/* Host-buffer gzip reader: any multi-member gzip stream (headers with FEXTRA/FNAME/FCOMMENT/FHCRC,
 * NUL padding between members).  Four decode paths, picked per stream / member:
 *   1. this engine's indexed members          -> two-pass, lane-parallel inside each member
 *   2. BGZF-style members ('B','C' subfield)  -> one wavefront per member, one launch; runs of small ordinary members
 *      (no member is more than 1 MiB of input from the next) likewise, after a count launch that finds where each ends
 *   3. any other member of at least 64 KiB with enough block boundaries -> chunk-parallel: chunk starts are
 *      the positions after sync-flush markers (block-parallel writers: gzip_ng_threaded, pigz) and the bit
 *      offsets where a dynamic block header parses (ordinary gzip files); a count-only pass sizes and
 *      validates them, a marker pass decodes the chunks independently, the 32 KiB windows are propagated
 *      along the chain and the markers resolved
 *   4. anything else (small members, stored / fixed-Huffman only streams) -> the sequential wavefront decoder
 * Paths 1-3 hand over to 4 whenever something does not check out, so errors are always the sequential
 * reader's.  *out_len = bytes produced (also on error), except that ZNGAMD_BUF_ERROR with
 * *out_len > out_cap means "the stream needs *out_len bytes of output" (size known up front). */
int zngamd_gunzip(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len,
                  uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members);

/* The same reader for a WINDOW of a longer stream (bounded-memory readers: GzipReader_read_into_buffer keeps a fixed
 * input buffer, zlib_ngmodule.c:2426-2450): every member that is complete inside the window is decoded; an incomplete
 * last member (cut header, deflate data or trailer) is left alone.  Returns ZNGAMD_OK with *in_consumed = offset of the
 * first byte not consumed: feed the stream from there next time, with more input behind it.  *in_consumed == 0 means the
 * window holds no complete member yet.  Real errors are reported as by zngamd_gunzip. */
int zngamd_gunzip_partial(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len,
                          uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members,
                          uint64_t *in_consumed);

/* The windowed reader with state: also a member LARGER than the window is decoded, block-wise.  *st starts zeroed.
 * At a member boundary this is zngamd_gunzip_partial; when not even the first member of the window is complete, the
 * complete deflate blocks of that member are decoded (chunk-parallel) and handed out, and *st remembers the bit offset
 * of the next block header, the last 32 KiB of output (the history that block may reference), the CRC-32 and length so
 * far.  The next call continues there: `in` must start at byte *in_consumed of the previous input.  last != 0: no more
 * input exists (a stream that does not end is an error).  *in_consumed == 0 with ZNGAMD_OK: supply a larger window. */
typedef struct zngamd_gz_state {
    uint32_t in_member;      /* 0 at a member boundary, 1 inside a member's deflate data */
    uint32_t start_bit;      /* bit (0..7) of in[0] where the next block header starts */
    uint32_t crc;            /* CRC-32 of the member's output so far */
    uint32_t window_len;     /* valid bytes in window[] */
    uint64_t out_total;      /* bytes the member has produced so far */
    uint8_t  window[32768];  /* the last window_len bytes of the member's output */
    void    *index;          /* (r06, may be NULL) zngamd_index_create's handle for the member being read: the writer's segment index,
                              * taken from the file's trailing members by the caller; the units inside a window then decode side by side */
} zngamd_gz_state;
/* The index of one data member for the windowed reader: per unit its compressed bytes (sync marker included), its output bytes and
 * its ZNGAMD_INDEX_STRIDE u32 of segment bit offsets (host arrays; see zngamd_deflate_index, which gives them for the units of the
 * context's last deflate call).  The handle belongs to the caller (zngamd_index_destroy) and must outlive every state that names it. */
int zngamd_index_create(zngamd_ctx *ctx, uint32_t n_units, const uint32_t *unit_in_len, const uint32_t *unit_out_len,
                        const uint32_t *rows, void **handle);
void zngamd_index_destroy(void *handle);
int zngamd_deflate_index(zngamd_ctx *ctx, uint32_t n_units, uint32_t *unit_in_len, uint32_t *unit_out_len, uint32_t *rows);
/* zngamd_deflate_blocks_packed and zngamd_deflate_index of ITS units in one call (n_units = zngamd_count_units(blocks, n_blocks)):
 * what a writer that shares its context with other threads calls -- between two calls another thread's deflate could slip, and
 * zngamd_deflate_index answers for the context's last deflate call, whoever made it.  Replaces, with the index, the writer
 * thread's join of its blocks (gzip_ng_threaded.py:382-398). */
int zngamd_deflate_blocks_packed_indexed(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_block *blocks, uint32_t n_blocks,
                                         int level, uint8_t *out, uint64_t out_cap, uint64_t block_cap, uint32_t *out_len, uint32_t *crc,
                                         uint64_t *total, uint32_t n_units, uint32_t *unit_in_len, uint32_t *unit_out_len, uint32_t *rows);
int zngamd_gunzip_stream(zngamd_ctx *ctx, zngamd_gz_state *st, const uint8_t *in, uint64_t in_len, int last,
                         uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t *n_members,
                         uint64_t *in_consumed);

/* Build one indexed gzip member stream (one member per block, FINAL blocks, 'ZA' index) from a host
 * buffer.  level as above; block_size <= 128 KiB. */
int zngamd_gzip_members(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                        int level, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* Device-resident form of the same (input and output stay in HBM). */
int zngamd_gzip_members_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, uint32_t block_size,
                            int level, void *d_out, uint64_t out_cap, uint64_t *out_len,
                            uint32_t *n_members);

/* ---- BGZF (SAM specification section 4.1; zlib_ng_amd/bgzf.py): gzip members of at most 64 KiB, each with its
 * own size in a 'B','C' extra subfield, each a deflate stream of its own; a file ends with an empty block of 28 fixed bytes.  A
 * position is a virtual offset, coffset << 16 | uoffset: the file offset of a block and a byte offset inside its output. */
#define ZNGAMD_E_BGZF          (-107)    /* zngamd_bgzf_scan: the buffer does not start with a BGZF block */
#define ZNGAMD_BGZF_MAX_INPUT  65280u    /* input bytes per block (htslib's 0xff00) */
#define ZNGAMD_BGZF_MAX_BLOCK  65536u
#define ZNGAMD_BGZF_EOF_BYTES  28u
typedef struct {
    uint64_t coffset;      /* offset of the block's first byte in the compressed stream */
    uint64_t uoffset;      /* offset of its first output byte in the uncompressed data  */
    uint32_t csize;        /* the block's bytes, header and trailer included (BSIZE + 1) */
    uint32_t isize;        /* its output bytes (ISIZE)                                   */
} zngamd_bgzf_block;       /* 24 B */
/* The writer.  The input is cut into blocks of block_size bytes (1 .. ZNGAMD_BGZF_MAX_INPUT; the last one shorter; no block for no
 * input); each is compressed on its own by the deflate kernels, one final deflate block sequence with ordinary dynamic headers, and
 * framed by one workgroup of the assemble kernel.  A payload of more than 65 510 bytes (it would not fit a block) is replaced by one
 * stored deflate block of the input.  eof != 0: the EOF block follows the data blocks.  d_out / d_table: device memory; d_table (may
 * be NULL) receives one row per block written, the EOF block's included (room for ceil(in_len / block_size) + 1 rows); *n_blocks =
 * the rows.  *out_len = the stream's bytes; ZNGAMD_BUF_ERROR with *out_len = the size needed when out_cap is too small (nothing is
 * written then).  Levels as zngamd_level_ok; level 0 writes stored blocks. */
int zngamd_bgzf_compress_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, uint32_t block_size, int level, int eof,
                             void *d_out, uint64_t out_cap, uint64_t *out_len, zngamd_bgzf_block *d_table, uint32_t *n_blocks);
/* Host-buffer form: table (may be NULL) is host memory of max_blocks rows (ZNGAMD_BUF_ERROR when it has fewer than *n_blocks). */
int zngamd_bgzf_compress(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, uint32_t block_size, int level, int eof,
                         uint8_t *out, uint64_t out_cap, uint64_t *out_len, zngamd_bgzf_block *table, uint32_t max_blocks,
                         uint32_t *n_blocks);
/* The walk from block to block through BSIZE, on the host: no GPU, no context (ctx-free, like zngamd_crc32_combine).  Every complete
 * block of `in` gets a row of `table` (NULL: the blocks are only counted; else the walk stops after max_blocks rows, *consumed says
 * where); *n_blocks = blocks walked, *consumed = offset of the first byte behind them, *total_out = the sum of their ISIZE.
 *   ZNGAMD_OK          the walk ended at in_len, at a full table, or in front of an incomplete last block (a cut header, or a BSIZE
 *                      that reaches beyond in_len) that follows at least one complete block: the tail starts at *consumed
 *   ZNGAMD_E_BGZF      `in` does not start with a BGZF block: other magic bytes, or a gzip member without the 'B','C' subfield
 *   ZNGAMD_DATA_ERROR  a BSIZE smaller than the block's own header and trailer; an ISIZE above 65 536; an extra field whose
 *                      subfields overrun it; behind the first block: bytes that are no BGZF header; and a FIRST block whose
 *                      header or BSIZE reaches beyond in_len (no complete block vouches for the stream: a reader that holds at
 *                      least 64 KiB, or the whole file, never sees this for a sound file).  The outputs describe the blocks in
 *                      front of the bad one. */
int zngamd_bgzf_scan(const uint8_t *in, uint64_t in_len, zngamd_bgzf_block *table, uint32_t max_blocks, uint32_t *n_blocks,
                     uint64_t *consumed, uint64_t *total_out);
/* Ranged reads.  d_in holds compressed blocks (any selection of a file's blocks, packed in any way; 64 readable bytes behind in_len),
 * d_members names them as zngamd_gzip_inflate_plain_members_dev takes it (in_off / in_len = a block's deflate payload, the trailer
 * behind it; out_off / out_len = where its output goes in d_scratch), in ascending order of out_off.  One launch of that decoder
 * decodes all of them into d_scratch, CRC-32 and ISIZE verified, d_status[m] = the verdict per block (0 = good).  Then one workgroup
 * per row of d_slices copies scratch[src_off, src_off + len) to d_out + dst_off -- only when blocks that decoded cover those bytes
 * without a gap: d_slice_status[i] = ZNGAMD_BGZF_SLICE_OK, _BLOCK (a block the slice touches failed or is missing; the slice's
 * bytes in d_out are zeros) or _TABLE (the row points outside scratch_cap / out_cap; nothing is written).  The tables are
 * untrusted: no entry makes a kernel read or write outside the buffers. */
typedef struct { uint64_t src_off, dst_off; uint32_t len, reserved; } zngamd_bgzf_slice;      /* 24 B */
#define ZNGAMD_BGZF_SLICE_OK    0
#define ZNGAMD_BGZF_SLICE_BLOCK 1
#define ZNGAMD_BGZF_SLICE_TABLE 2
int zngamd_bgzf_read_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                         const zngamd_bgzf_slice *d_slices, uint32_t n_slices, void *d_scratch, uint64_t scratch_cap,
                         void *d_out, uint64_t out_cap, int32_t *d_status, int32_t *d_slice_status);
/* Host-buffer form: stages in and the tables, keeps the decoded blocks on the device and copies back the statuses and the packed
 * result only (out[0 .. the end of the last slice)). */
int zngamd_bgzf_read(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                     const zngamd_bgzf_slice *slices, uint32_t n_slices, uint8_t *out, uint64_t out_cap, int32_t *status,
                     int32_t *slice_status);
/* what the ranged reads and the line calls below did since the last reset: out[0] decode launches, out[1] blocks decoded, out[2]
 * slices gathered */
int zngamd_bgzf_stats(zngamd_ctx *ctx, uint64_t *out /*[3]*/, int reset);

/* ---- BGZF by line (zlib_ng_amd/bgzf.py: LineIndex, BgzfReader.read_lines).  A line ends with one delimiter
 * byte (delim, 0 .. 255; anything else is ZNGAMD_E_ARG).  All three calls take the compressed blocks and the member table as
 * zngamd_bgzf_read_dev takes them (64 readable bytes behind in_len in d_in), decode all of them in one launch into the scratch and
 * leave the decoded bytes on the device.  d_status[m] = the decoder's verdict per block (0 = good).  The tables are untrusted: no
 * entry makes a kernel read or write outside the buffers. */
typedef struct { uint32_t count, flags; } zngamd_bgzf_count_row;      /* 8 B (12 per block with its status) */
#define ZNGAMD_BGZF_COUNT_LAST  1u           /* flags: the block's last output byte is the delimiter */
/* Counting: d_rows[m] = the delimiter bytes in block m's output and ZNGAMD_BGZF_COUNT_LAST; a block that failed, or whose output
 * lies outside scratch_cap, gets {0, 0}. */
int zngamd_bgzf_count_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                          int delim, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_count_row *d_rows);
/* Host-buffer form: stages in and the table, copies back the statuses and the rows only. */
int zngamd_bgzf_count(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                      int delim, int32_t *status, zngamd_bgzf_count_row *rows);
/* A position query: the scratch offset of the byte BEHIND the rank-th delimiter (counted from 1) of block `member`'s output.  rank 0
 * is the block's first byte, ZNGAMD_BGZF_RANK_END one past its last.  Verdict per query: ZNGAMD_BGZF_SLICE_OK; _TABLE (member outside
 * the table, a block outside scratch_cap or of more than 65 536 bytes); _BLOCK (the block failed); _RANK (the block has fewer
 * delimiters than rank: the index that made the query was built for another file).  Only _OK comes with a position (0 otherwise). */
typedef struct { uint32_t member, rank; } zngamd_bgzf_pos;              /* 8 B */
#define ZNGAMD_BGZF_RANK_END    0xFFFFFFFFu
#define ZNGAMD_BGZF_SLICE_RANK  3
int zngamd_bgzf_line_positions_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members,
                                   uint32_t n_members, const zngamd_bgzf_pos *d_queries, uint32_t n_queries, int delim,
                                   void *d_scratch, uint64_t scratch_cap, int32_t *d_status, uint64_t *d_pos, int32_t *d_pos_status);
int zngamd_bgzf_line_positions(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                               const zngamd_bgzf_pos *queries, uint32_t n_queries, int delim, int32_t *status, uint64_t *pos,
                               int32_t *pos_status);
/* Reading lines: a range is two positions, from (m0, r0) up to (m1, r1); the bytes between them are packed into d_out in the order
 * of the table, d_range_len[i] bytes each, *out_len in all.  d_range_status[i]: the verdict of the range's positions if one is not
 * _OK, _TABLE for a second position below the first or a range of 4 GiB or more, else what the slice kernel of the ranged reads
 * says (_BLOCK: a block between the two positions failed or is missing).  A range without the verdict _OK has length 0 or zeros
 * for bytes.  ZNGAMD_BUF_ERROR with *out_len = the size needed when out_cap is too small: no line is written then, d_range_len is
 * valid, d_range_status is NOT written (the slice kernel, which has the last word on it, has not run).  Fewer than 2^30 ranges. */
typedef struct { uint32_t m0, r0, m1, r1; } zngamd_bgzf_line_range;    /* 16 B */
int zngamd_bgzf_read_lines_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                               const zngamd_bgzf_line_range *d_ranges, uint32_t n_ranges, int delim, void *d_scratch,
                               uint64_t scratch_cap, void *d_out, uint64_t out_cap, uint64_t *out_len, uint32_t *d_range_len,
                               int32_t *d_status, int32_t *d_range_status);
/* Host-buffer form: the lengths and the verdicts are copied back in either case, the packed lines when they fit out_cap.  A caller
 * that cannot bound the lines passes out = NULL, out_cap = 0 and alloc: once the size is known, alloc(user, *out_len) is asked for
 * the memory the lines go to (not called for no bytes; NULL from it: ZNGAMD_MEM_ERROR), as in the batch API's host forms. */
int zngamd_bgzf_read_lines(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                           const zngamd_bgzf_line_range *ranges, uint32_t n_ranges, int delim, uint8_t *out, uint64_t out_cap,
                           zngamd_alloc_fn alloc, void *user, uint64_t *out_len, uint32_t *range_len, int32_t *status,
                           int32_t *range_status);

/* ---- BGZF by content (zlib_ng_amd/bgzf.py: grep).  The blocks and the member table as the line calls take
 * them; one decode launch; then the text scratch[text_off, text_end) (text_off: the first byte of a line; text_end <= scratch_cap;
 * fewer than 4 GiB) is searched on the device for fixed byte strings.  A line is selected when one of the patterns occurs in it (with
 * _LINE_START: stands at its first byte; with _INVERT: when none does).  Lines end with `delim` and are returned with it; with
 * _FINAL the bytes behind the last delimiter are a line too, without it they are the open tail, which the next call takes up again
 * at totals->tail_off.  Patterns: host memory in both forms, n_patterns (1 .. 64) rows {off, len} into `patterns` (patterns_len
 * bytes), each 1 .. 255 bytes without the delimiter byte; anything else is ZNGAMD_E_ARG, found before anything is launched.
 * Results: one row per selected line in ascending order (src_off: where it starts in the scratch; number: line_base + the lines of
 * the text in front of it; len: its bytes, delimiter included) and the lines packed in that order.  *totals is always valid on
 * ZNGAMD_OK and ZNGAMD_BUF_ERROR.  covered = 0: the member rows do not tile the text in ascending order without a gap or an
 * overlap, or a block that touches the text did not decode (d_status says which): nothing is counted and no line is emitted.
 * ZNGAMD_BUF_ERROR: rows_cap < totals->matched or out_cap < totals->bytes; nothing is written.  _COUNT_ONLY: the totals alone, no
 * buffers needed.  The tables are untrusted: no entry makes a kernel read or write outside the buffers. */
typedef struct { uint32_t off, len; } zngamd_bgzf_pattern;                                        /* 8 B */
typedef struct { uint64_t src_off, number; uint32_t len, reserved; } zngamd_bgzf_grep_row;        /* 24 B */
typedef struct {
    uint64_t seen;         /* lines of the text that were decided (the open tail is not one of them) */
    uint64_t matched;      /* of them, selected */
    uint64_t bytes;        /* bytes of the selected lines */
    uint64_t tail_off;     /* scratch offset where the open line starts; text_end when there is none */
    uint32_t covered;      /* 1: decoded blocks cover the text and the figures above describe it */
    uint32_t reserved;
} zngamd_bgzf_grep_totals;                                                                        /* 40 B */
#define ZNGAMD_BGZF_GREP_INVERT      1u
#define ZNGAMD_BGZF_GREP_LINE_START  2u
#define ZNGAMD_BGZF_GREP_FINAL       4u
#define ZNGAMD_BGZF_GREP_COUNT_ONLY  8u
#define ZNGAMD_BGZF_GREP_MAX_PATTERNS 64u
#define ZNGAMD_BGZF_GREP_MAX_PATTERN  255u
int zngamd_bgzf_grep_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                         uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                         const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint64_t line_base,
                         void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap,
                         void *d_out, uint64_t out_cap, zngamd_bgzf_grep_totals *totals);
/* Host-buffer form: stages in and the member table; the scratch is as long as the table says; status, rows and the packed lines come
 * back.  A caller that cannot bound the result passes rows = out = NULL, the capacities 0 and alloc: once the sizes are known it is
 * asked first for the rows (matched * 24 bytes), then for the lines (bytes); it is not asked for an empty array; NULL from it:
 * ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_grep(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                     uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                     const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint64_t line_base,
                     int32_t *status, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap,
                     zngamd_alloc_fn alloc, void *user, zngamd_bgzf_grep_totals *totals);

/* ---- BGZF by content, with mismatches (zlib_ng_amd/bgzf.py: grep(..., mismatches=k)).  The four calls above
 * with max_mismatch (k) directly behind flags; every other parameter, the results, the totals and the errors are those of the call
 * without _approx, and max_mismatch = 0 selects exactly what that call selects.  Hamming distance, that is substitutions only: a
 * pattern of L bytes matches a line when the line's body (the line without its delimiter) has L consecutive bytes that differ from it
 * in at most k positions.  The window lies wholly inside the body: one that holds the delimiter byte never matches, though the count
 * would fit (a pattern holds no delimiter, so it would be one mismatch); one that would need a byte at or behind text_end never
 * matches; a line shorter than L cannot match.  With _LINE_START the window starts at the line's first byte.  One k for all patterns
 * of a call, 0 .. ZNGAMD_BGZF_GREP_MAX_MISMATCH and less than the length of the shortest pattern; anything else is ZNGAMD_E_ARG, found
 * before the context is touched, like everything the exact calls refuse.  Not reported: which pattern matched, and at what distance
 * (the row's reserved word stays 0; zngamd_bgzf_classify_records below answers that).  Cost: there is no prefilter, every text byte is compared with every pattern byte until a window's
 * count passes k -- 64 x 255 pattern bytes per text byte at the worst; the exact calls do not pay for it. */
#define ZNGAMD_BGZF_GREP_MAX_MISMATCH 16u
int zngamd_bgzf_grep_approx_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                                uint64_t line_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_grep_row *d_rows,
                                uint64_t rows_cap, void *d_out, uint64_t out_cap, zngamd_bgzf_grep_totals *totals);
int zngamd_bgzf_grep_approx(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                            uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                            const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                            uint64_t line_base, int32_t *status, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out,
                            uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_grep_totals *totals);

/* ---- BGZF by record (zlib_ng_amd/bgzf.py: grep_records).  zngamd_bgzf_grep on records of record_lines
 * (k, 1 .. 64) lines each: FASTQ 4, two-line FASTA 2, interleaved pairs 8; k = 1 is zngamd_bgzf_grep.  Blocks, member table, text,
 * patterns, delimiter, the lines, _FINAL, _LINE_START, _COUNT_ONLY, the cover contract, ZNGAMD_BUF_ERROR and alloc are those of
 * zngamd_bgzf_grep.  The record model:
 *   - text_off is a record start.  Record r of the call is its lines [k r, k r + k).
 *   - A record is hit when one of the patterns occurs in one of its lines; with match_line = j (0 <= j < k; -1: any line) only line j
 *     of the record counts; with _LINE_START the pattern must stand at that line's first byte.
 *   - A record is selected when hit != _INVERT: invert works on records, the line verdicts are computed without it.
 *   - A record whose last line has not ended in the text is the open tail: tail_off is where its FIRST line starts, and the next
 *     call takes it up there.
 *   - With _FINAL the lines left over (lines % k != 0) form one short last record, judged like any other on the lines it has;
 *     short_lines says how many it has (0: the last record is whole).
 *   - first_byte (0 .. 255; -1: no check): a record whose first byte differs is bad.  bad = 1: bad_record is the smallest such record's
 *     number and bad_src its scratch offset; no row and no byte is written, the other totals are valid.
 * Results: one row per selected record in ascending order (src_off: where its first line starts in the scratch; number: record_base +
 * r; len: the bytes of its lines, delimiters included) and the records packed whole in that order.  record_lines, match_line or
 * first_byte out of range: ZNGAMD_E_ARG, found before the context is touched, like everything zngamd_bgzf_grep refuses.  Device
 * memory beside the tiles of zngamd_bgzf_grep: 8 bytes per line and 17 bytes per record of the text. */
typedef struct {
    uint64_t seen;         /* records of the text that were decided (the open tail is not one of them) */
    uint64_t selected;     /* of them, selected */
    uint64_t bytes;        /* bytes of the selected records */
    uint64_t tail_off;     /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;   /* bad = 1: the number of the first record whose first byte is not first_byte */
    uint64_t bad_src;      /*          and where it starts in the scratch */
    uint32_t covered;      /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;  /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;
    uint32_t reserved;
} zngamd_bgzf_grep_records_totals;                                                                /* 64 B */
#define ZNGAMD_BGZF_GREP_MAX_RECORD_LINES 64u
int zngamd_bgzf_grep_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                 uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                 const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t record_lines,
                                 int32_t match_line, int32_t first_byte, uint64_t record_base, void *d_scratch, uint64_t scratch_cap,
                                 int32_t *d_status, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                 zngamd_bgzf_grep_records_totals *totals);
int zngamd_bgzf_grep_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                             uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                             const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t record_lines,
                             int32_t match_line, int32_t first_byte, uint64_t record_base, int32_t *status, zngamd_bgzf_grep_row *rows,
                             uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user,
                             zngamd_bgzf_grep_records_totals *totals);
/* With mismatches: max_mismatch directly behind flags, the matching rule of zngamd_bgzf_grep_approx on the lines that count for a
 * record; match_line, first_byte and _INVERT on records mean what they mean above. */
int zngamd_bgzf_grep_records_approx_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members,
                                        uint32_t n_members, uint64_t text_off, uint64_t text_end, const uint8_t *patterns,
                                        uint32_t patterns_len, const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim,
                                        uint32_t flags, uint32_t max_mismatch, uint32_t record_lines, int32_t match_line,
                                        int32_t first_byte, uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status,
                                        zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                        zngamd_bgzf_grep_records_totals *totals);
int zngamd_bgzf_grep_records_approx(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                                    uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                    const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                                    uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base, int32_t *status,
                                    zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc,
                                    void *user, zngamd_bgzf_grep_records_totals *totals);

/* ---- BGZF by nearest pattern (zlib_ng_amd/bgzf.py: classify_records, demux).  Not "which records carry one of
 * the patterns" but, for every record, "which of the patterns is it, and how surely": what a demultiplexer asks of its 8 to 64
 * barcodes.  The record model is that of zngamd_bgzf_grep_records (record_lines, match_line, first_byte, _LINE_START, _FINAL, the
 * open tail, the short last record, the cover contract), the window rule that of zngamd_bgzf_grep_approx (a window lies wholly inside
 * a line's body, holds no delimiter, needs no byte at or behind text_end, with _LINE_START starts at the line's first byte), and
 * max_mismatch (k) is 0 .. 16 and less than the shortest pattern's length; k = 0 is exact assignment.  The rule:
 *   - d_i(r), for record r and pattern i, is the smallest distance <= k over all windows of the record's lines that count (all of
 *     them, or line match_line alone); "none" when no window is within k.
 *   - unassigned: every d_i is none.                    row {255, 255, 255, 0}
 *   - assigned to i at distance d = min d_i when exactly one pattern reaches d.          row {i, i, d, _CLASS_ASSIGNED}
 *   - ambiguous when two or more patterns reach the minimum: the lowest and the highest index among them.   row {lo, hi, d, _CLASS_AMBIGUOUS}
 * The result depends on the text and the pattern list alone.  Two patterns with the same bytes are ZNGAMD_E_ARG (neither could ever
 * be assigned); a pattern that is a prefix of another is allowed, the rule settles the pair.  Classes, for counting and grouping:
 * i (0 .. n_patterns - 1) for the records assigned to pattern i, n_patterns for the ambiguous ones, n_patterns + 1 for the unassigned
 * ones; n_classes = n_patterns + 2, at most 66.
 * flags: _LINE_START, _FINAL and ZNGAMD_BGZF_CLASSIFY_GROUP; anything else, _INVERT and _COUNT_ONLY included, is ZNGAMD_E_ARG.
 * Without _GROUP only d_class[0 .. seen), one row per record in record order, and the totals leave the kernels; d_rows and d_out may
 * be NULL with capacity 0.  With _GROUP d_rows[0 .. seen) holds a row per record ordered by class, then by record number (src_off,
 * number = record_base + r, len as in zngamd_bgzf_grep_records; reserved: the record's class row), and d_out the records packed whole
 * in that order: class c has the rows [sum of class_records[< c], ... + class_records[c]) and the bytes [sum of class_bytes[< c], ...).
 * ZNGAMD_BUF_ERROR: class_cap < seen or, with _GROUP, rows_cap < seen or out_cap < bytes; nothing is written, the totals are valid.
 * bad / bad_record / bad_src / covered / short_lines / tail_off mean what they mean in zngamd_bgzf_grep_records_totals; with bad set
 * no row and no byte is written.  Hostile arguments -- patterns, max_mismatch, record_lines / match_line / first_byte, flags, duplicate
 * patterns, totals = NULL -- are ZNGAMD_E_ARG before the context is touched.  Device memory beside the tiles: 8 bytes per line and 17
 * bytes per record of the text, and 8 bytes per class and 256 records. */
typedef struct { uint8_t pattern, other, distance, flags; } zngamd_bgzf_class_row;               /* 4 B */
#define ZNGAMD_BGZF_CLASS_ASSIGNED  1u   /* pattern == other: the one nearest pattern, at `distance` */
#define ZNGAMD_BGZF_CLASS_AMBIGUOUS 2u   /* pattern < other: the lowest and the highest index at `distance` */
/* flags == 0: unassigned; pattern = other = distance = 255 */
#define ZNGAMD_BGZF_CLASSIFY_GROUP  16u  /* flags of the call: also return the records, grouped by class */
#define ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES 66u
typedef struct {
    uint64_t seen;         /* records of the text that were decided (the open tail is not one of them) */
    uint64_t bytes;        /* their bytes: the sum of class_bytes */
    uint64_t tail_off;     /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;   /* bad = 1: the number of the first record whose first byte is not first_byte */
    uint64_t bad_src;      /*          and where it starts in the scratch */
    uint32_t covered;      /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;  /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;
    uint32_t n_classes;    /* n_patterns + 2 */
    uint64_t class_records[ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES];      /* records per class; entries from n_classes on are 0 */
    uint64_t class_bytes[ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES];        /* and their bytes */
} zngamd_bgzf_classify_totals;                                                                    /* 1112 B */
int zngamd_bgzf_classify_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                     uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                     const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                                     uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base, void *d_scratch,
                                     uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_class_row *d_class, uint64_t class_cap,
                                     zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                     zngamd_bgzf_classify_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status, the class rows and, with _GROUP, the rows and the packed records
 * come back.  With alloc (class_rows = rows = out = NULL, the capacities 0) the caller's memory is asked for once the sizes are known,
 * in the order class rows (seen * 4 bytes), rows (seen * 24 bytes), bytes -- the last two with _GROUP only; NULL from it:
 * ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_classify_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                                 uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                 const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags, uint32_t max_mismatch,
                                 uint32_t record_lines, int32_t match_line, int32_t first_byte, uint64_t record_base, int32_t *status,
                                 zngamd_bgzf_class_row *class_rows, uint64_t class_cap, zngamd_bgzf_grep_row *rows, uint64_t rows_cap,
                                 uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_classify_totals *totals);

/* ---- BGZF by a label per record (zlib_ng_amd/bgzf.py: partition_records, demux_paired).  The call above
 * without the compare: the class of record r is not computed from patterns but read from labels[r], which the caller computed --
 * from the mate file of a paired run, from the index reads of a dual-index run, or by any rule of their own.  The record model is that
 * of zngamd_bgzf_grep_records (record_lines, first_byte, _FINAL, the open tail, the short last record, the cover contract); there are
 * no patterns, no match_line and no max_mismatch.  The labels:
 *   - labels[r] (uint16_t) belongs to record record_base + r of the call: a class 0 .. n_classes - 1 (n_classes: 1 .. 1024), or
 *     ZNGAMD_BGZF_PARTITION_DROP: the record is counted in dropped / dropped_bytes, gets no row and none of its bytes is gathered.
 *   - Only the first min(n_labels, seen) labels are read.  seen > n_labels: labels_short = 1, no row and no byte is written, and the
 *     totals are valid, the records without a label counted as dropped ones.  n_labels > seen is no fault: the next call takes
 *     labels + seen.
 *   - Any other value is a fault: bad = 2, bad_record the smallest such record's number and bad_src its scratch offset.  A first_byte
 *     violation is bad = 1 as in zngamd_bgzf_grep_records.  Of the two faults the one at the smaller record is reported; a record
 *     with both is reported for its first byte.  With bad set no row and no byte is written; the other totals are valid, except that
 *     a record whose label is out of range counts in no class.
 * flags: _FINAL and ZNGAMD_BGZF_CLASSIFY_GROUP; anything else, _LINE_START included, is ZNGAMD_E_ARG.  class_records and class_bytes
 * are HOST arrays of n_classes entries that the caller owns, in both forms: records and bytes per class (zeros when nothing was
 * decided).  Without _GROUP only they and the totals leave the kernels; d_rows and d_out may be NULL with capacity 0.  With _GROUP
 * d_rows[0 .. seen - dropped) holds a row per kept record ordered by class, then by record number (src_off, number = record_base + r,
 * len as in zngamd_bgzf_grep_records; reserved: the label), and d_out the records packed whole in that order: class c has the rows
 * [sum of class_records[< c], ... + class_records[c]) and the bytes [sum of class_bytes[< c], ...).
 * ZNGAMD_BUF_ERROR: with _GROUP, rows_cap < seen - dropped or out_cap < bytes; nothing is written, the totals and the counts are valid.
 * Hostile arguments -- n_classes 0 or above 1024, labels NULL with n_labels > 0, record_lines / first_byte, delim, flags, totals or a
 * count array NULL -- are ZNGAMD_E_ARG before the context is touched.  Device memory beside the tiles: 8 bytes per line and 6 bytes per
 * record of the text (4 without the host form's copy of the labels), 8 bytes per class and 256 records, and 16 bytes per class. */
#define ZNGAMD_BGZF_PARTITION_MAX_CLASSES 1024u
#define ZNGAMD_BGZF_PARTITION_DROP        0xFFFFu
typedef struct {
    uint64_t seen;          /* records of the text that were decided (the open tail is not one of them) */
    uint64_t bytes;         /* bytes of the kept records: the sum of class_bytes */
    uint64_t dropped;       /* records labelled _DROP (or, with labels_short, without a label) */
    uint64_t dropped_bytes; /* and their bytes */
    uint64_t tail_off;      /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;    /* bad != 0: the number of the record at fault */
    uint64_t bad_src;       /*           and where it starts in the scratch */
    uint32_t covered;       /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;   /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;           /* 0; 1: the first byte is not first_byte; 2: the label is out of range */
    uint32_t labels_short;  /* 1: the text holds more records than n_labels */
} zngamd_bgzf_partition_totals;                                                                   /* 72 B */
int zngamd_bgzf_partition_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                      uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines,
                                      int32_t first_byte, uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status,
                                      zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                      const uint16_t *d_labels, uint64_t n_labels, uint32_t n_classes, uint64_t *class_records,
                                      uint64_t *class_bytes, zngamd_bgzf_partition_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; labels is host memory, of which min(n_labels, seen) entries are uploaded
 * once the line count is known; status and, with _GROUP, the rows and the packed records come back.  With alloc (rows = out = NULL,
 * the capacities 0) the caller's memory is asked for once the sizes are known, in the order rows ((seen - dropped) * 24 bytes),
 * bytes -- with _GROUP and seen > dropped only; NULL from it: ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_partition_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                                  uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines,
                                  int32_t first_byte, uint64_t record_base, int32_t *status, zngamd_bgzf_grep_row *rows, uint64_t rows_cap,
                                  uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user, const uint16_t *labels,
                                  uint64_t n_labels, uint32_t n_classes, uint64_t *class_records, uint64_t *class_bytes,
                                  zngamd_bgzf_partition_totals *totals);

/* ---- BGZF trimmed (zlib_ng_amd/bgzf.py: trim_records).  The first record call that changes the records it
 * returns: the read of every record is cut as cutadapt, fastp or Trimmomatic cut it, and what is left is written.  The record model is
 * that of zngamd_bgzf_grep_records (record_lines k, first_byte, _FINAL, the open tail, the cover contract).  conf names two lines of
 * the record: seq_line s (0 <= s < k) and qual_line q (-1: none; otherwise 0 <= q < k, q != s).  A line's body is its bytes without
 * the delimiter; a CR is a body byte.  A short last record under _FINAL is judged on the lines it has: a line it lacks is an empty
 * body and is not written.  For a seq body of n bytes the rule yields a cut [a, b), 0 <= a <= b <= n, in this order, in integers:
 *   1. fixed cut: a = min(cut_front, n); b = max(a, n - min(cut_back, n)).
 *   2. quality (q >= 0; qual_front / qual_back 0 .. 93, 0: off; Q_i = qual[i] - quality_base, signed).  Both scans run over the [a, b)
 *      of step 1, independently.  3' scan: s = best = 0, b' = b; for i = b - 1 down to a: s += qual_back - Q_i; s < 0 stops; s > best:
 *      best = s, b' = i.  5' scan: s = best = 0, a' = a; for i = a up: s += qual_front - Q_i; s < 0 stops; s > best: best = s,
 *      a' = i + 1.  Then a = a', b = max(a', b').  (BWA's rule, the one behind cutadapt -q.)  The sums are kept in 64 bits.
 *   3. adapters (3' adapters: n_patterns 0 .. 64 of 1 .. 255 bytes, none holding the delimiter).  R = seq[a, b), m = b - a.  Adapter j of
 *      L bytes matches at p (0 <= p < m) with overlap o = min(L, m - p) when o >= min(min_overlap, L) and R[p, p + o) differs from its
 *      first o bytes in at most (max_mismatch * o) / L places.  max_mismatch is 0 .. 16 and less than the shortest adapter: a budget for
 *      the whole adapter, of which a partial overlap gets its share.  min_overlap is 1 .. 255.  The smallest p at which any adapter
 *      matches wins, there the lowest j; then b = a + p and the record counts in adapter_records[j].  Bytes are compared as they are.
 *   4. verdict: _TRIM_DROPPED when the drop mask says so (drop[r] != 0 for record record_base + r of the call; drop = NULL: no record is
 *      dropped; with a mask, records at or beyond n_drop are dropped ones and set drop_short, and nothing is written); otherwise
 *      _TRIM_TOO_SHORT when b - a < min_length; otherwise _TRIM_KEPT.  Dropped records are cut and counted like the others.
 * Written for a record: its lines in order, lines s and q with the body bytes [a, b), every other line whole, every delimiter the
 * source has; a read cut to nothing leaves two empty lines.  Faults: bad = 1, a first_byte violation; bad = 3, q >= 0 and the two
 * bodies differ in length (2 is the label fault of zngamd_bgzf_partition_records and is not used here).  Of the two the one at the
 * smaller record is reported, a record with both for its first byte; with bad set nothing is written, the counts are valid except that
 * a record whose bodies differ is cut by step 1 alone.
 * flags: _FINAL and ZNGAMD_BGZF_CLASSIFY_GROUP; anything else is ZNGAMD_E_ARG.  Without _GROUP only d_trim[0 .. seen), one row per
 * record in record order, and the totals leave the kernels.  With _GROUP d_rows holds a row per kept record (and, with
 * ZNGAMD_BGZF_TRIM_KEEP_SHORT in conf.flags, behind them one per too-short record), each class in record order (src_off: where the
 * record starts in the scratch; number = record_base + r; len: its bytes as written; reserved: 0 kept, 1 too short), and d_out the
 * records as written in that order: `kept` rows and then `too_short` rows.  ZNGAMD_BUF_ERROR: trim_cap < seen or, with _GROUP,
 * rows_cap or out_cap too small; nothing is written, the totals are valid.  Hostile arguments -- conf NULL or a field out of range,
 * q == s, a quality cutoff with q = -1, a reserved word set, adapters that break the limits above, max_mismatch >= an adapter's
 * length, drop NULL with n_drop > 0, flags, totals NULL -- are ZNGAMD_E_ARG before the context is touched.  Device memory beside the
 * tiles: 8 bytes per line and 18 bytes per record of the text (19 with the host form's copy of the mask), and 16 bytes per 256 records. */
#define ZNGAMD_BGZF_TRIM_KEPT       0u
#define ZNGAMD_BGZF_TRIM_TOO_SHORT  1u
#define ZNGAMD_BGZF_TRIM_DROPPED    2u
#define ZNGAMD_BGZF_TRIM_KEEP_SHORT 1u   /* conf.flags: the too-short records are gathered behind the kept ones, not only counted */
#define ZNGAMD_BGZF_TRIM_NO_ADAPTER 255u
#define ZNGAMD_BGZF_TRIM_MAX_QUALITY 93u
typedef struct {
    uint32_t record_lines;  /* k, 1 .. 64 */
    int32_t  seq_line;      /* s */
    int32_t  qual_line;     /* q; -1: none */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    uint32_t cut_front;     /* step 1 */
    uint32_t cut_back;
    uint32_t qual_front;    /* step 2: 0 .. 93; 0: off */
    uint32_t qual_back;
    uint32_t quality_base;  /* 0 .. 255; 33 for Sanger / Illumina 1.8+ */
    uint32_t max_mismatch;  /* step 3 */
    uint32_t min_overlap;   /* 1 .. 255 */
    uint32_t min_length;    /* step 4 */
    uint32_t flags;         /* ZNGAMD_BGZF_TRIM_KEEP_SHORT */
    uint32_t reserved[3];   /* 0 */
} zngamd_bgzf_trim_conf;                                                                          /* 64 B */
typedef struct {
    uint32_t begin;         /* a */
    uint32_t end;           /* b */
    uint8_t  adapter;       /* j; ZNGAMD_BGZF_TRIM_NO_ADAPTER: none */
    uint8_t  verdict;       /* ZNGAMD_BGZF_TRIM_KEPT / _TOO_SHORT / _DROPPED */
    uint8_t  steps;         /* bit 0: the fixed cut moved an end, bit 1: quality did, bit 2: an adapter did */
    uint8_t  reserved;
} zngamd_bgzf_trim_row;                                                                           /* 12 B */
typedef struct {
    uint64_t seen;            /* records of the text that were decided (the open tail is not one of them) */
    uint64_t kept;            /* of them, per verdict */
    uint64_t too_short;
    uint64_t dropped;
    uint64_t bytes_in;        /* bytes of the records as they lie in the text */
    uint64_t bytes;           /* bytes of the records as written: the kept ones and, with _TRIM_KEEP_SHORT, the too-short ones */
    uint64_t bases_in;        /* sum of n */
    uint64_t bases_out;       /* sum of b - a over the kept records */
    uint64_t quality_trimmed; /* bases step 2 took, over all records */
    uint64_t adapter_trimmed; /* bases step 3 took, over all records */
    uint64_t tail_off;        /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;      /* bad != 0: the number of the record at fault */
    uint64_t bad_src;         /*           and where it starts in the scratch */
    uint32_t covered;         /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;     /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;             /* 0; 1: the first byte is not first_byte; 3: the bodies of seq_line and qual_line differ in length */
    uint32_t drop_short;      /* 1: the text holds more records than n_drop */
    uint64_t adapter_records[ZNGAMD_BGZF_GREP_MAX_PATTERNS];      /* records cut at adapter j */
} zngamd_bgzf_trim_totals;                                                                        /* 632 B */
int zngamd_bgzf_trim_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                 uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                                 const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags,
                                 const zngamd_bgzf_trim_conf *conf, uint64_t record_base, void *d_scratch, uint64_t scratch_cap,
                                 int32_t *d_status, const uint8_t *d_drop, uint64_t n_drop, zngamd_bgzf_trim_row *d_trim, uint64_t trim_cap,
                                 zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap,
                                 zngamd_bgzf_trim_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; drop is host memory, of which min(n_drop, seen) bytes are uploaded once
 * the line count is known; status, the trim rows and, with _GROUP, the rows and the written records come back.  With alloc (trim =
 * rows = out = NULL, the capacities 0) the caller's memory is asked for once the sizes are known, in the order trim rows (seen * 12
 * bytes), rows ((kept [+ too_short]) * 24 bytes), bytes -- the last two with _GROUP and a record to write only; NULL from it:
 * ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_trim_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                             uint64_t text_off, uint64_t text_end, const uint8_t *patterns, uint32_t patterns_len,
                             const zngamd_bgzf_pattern *table, uint32_t n_patterns, int delim, uint32_t flags,
                             const zngamd_bgzf_trim_conf *conf, uint64_t record_base, int32_t *status, const uint8_t *drop, uint64_t n_drop,
                             zngamd_bgzf_trim_row *trim, uint64_t trim_cap, zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out,
                             uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_trim_totals *totals);

/* ---- BGZF quality control (zlib_ng_amd/bgzf.py: qc_records).  What FastQC, fastp's report and seqkit stats -a
 * count: per-cycle base composition and quality tables, the length, GC and mean-quality distributions, the totals and, when asked for,
 * one row of figures per record.  Nothing is selected, cut or written.  The record model is that of zngamd_bgzf_grep_records
 * (record_lines k, first_byte, _FINAL, the open tail, the cover contract).  conf names two lines of the record: seq_line s (0 <= s < k)
 * and qual_line q (-1: none; otherwise 0 <= q < k, q != s).  A line's body is its bytes without the delimiter; a CR is a body byte.  A
 * short last record under _FINAL is judged on the lines it has: a line it lacks is an empty body.  For a record with a seq body of n
 * bytes, all in integers:
 *   class   of a byte, case folded (byte & 0xDF): 0 A, 1 C, 2 G, 3 T, 4 N, 5 anything else.
 *   quality Q_i = clamp(qual[i] - quality_base, 0, 93); every byte that was clamped counts in quality_clamped.
 *   row     of position i: min(i, C), C = cycles.  Row C collects everything at or beyond `cycles`: a long read is counted whole.
 *   tables  uint64_t, contiguous, in this order (ZNGAMD_BGZF_QC_TABLE_WORDS(C) words; the call overwrites them, the caller does not
 *           zero them):
 *             base_pos[C + 1][6]     bytes of every class at every row
 *             qual_pos[C + 1][94]    bytes of every quality at every row (all zero when q = -1)
 *             length_hist[C + 2]     records with n bases at index n (n <= C), longer ones at index C + 1
 *             gc_hist[101]           records with n >= 1 at bin (100 * gc) / n, gc = bases of class 1 or 2
 *             meanq_hist[94]         records with n >= 1 at bin qsum / n, qsum = the sum of Q_i (q >= 0 only)
 *   totals  seen, bytes_in, bases (sum of n), min_len and max_len (min_len = UINT64_MAX when seen = 0), empty (n = 0), base_total[6],
 *           quality_sum, q20_bases and q30_bases (Q >= 20, Q >= 30), low_bases (Q < low_quality), quality_clamped; the quality figures
 *           are 0 when q = -1.
 *   rows    (ZNGAMD_BGZF_QC_ROWS in conf.flags) one zngamd_bgzf_qc_row per record in record order: qsum, len = n, gc, n = bases of
 *           class 4, low = bases with Q < low_quality.  Without the flag only the tables and the totals leave the device.
 * Faults: bad = 1, a first_byte violation; bad = 3, q >= 0 and the two bodies differ in length (2 is the label fault of
 * zngamd_bgzf_partition_records and is not used here).  Of the two the one at the smaller record is reported, a record with both for its
 * first byte; with bad set the tables, the rows and the totals other than the fault fields are not to be used.
 * flags: _FINAL; anything else is ZNGAMD_E_ARG.  ZNGAMD_BUF_ERROR: tables_cap (in words) below ZNGAMD_BGZF_QC_TABLE_WORDS(cycles), before
 * anything is launched; or, with _QC_ROWS, rows_cap < seen: no row is written, tables and totals are valid.  Hostile arguments -- conf
 * NULL or a field out of range, q == s, a reserved word set, flags, totals or the tables NULL, rows NULL with _QC_ROWS (and, in the
 * host form, no alloc) -- are ZNGAMD_E_ARG before the context is touched.  Device memory beside the tiles: 8 bytes per line of the
 * text, and in the host form the tables (at most 3.3 MB) and 24 bytes per record with _QC_ROWS. */
#define ZNGAMD_BGZF_QC_MAX_CYCLES 4096u
#define ZNGAMD_BGZF_QC_BASES      6u
#define ZNGAMD_BGZF_QC_QUALITIES  94u
#define ZNGAMD_BGZF_QC_MAX_LOW    93u
#define ZNGAMD_BGZF_QC_GC_BINS    101u
#define ZNGAMD_BGZF_QC_ROWS       1u     /* conf.flags: one row per record leaves the device */
/* words of the tables for `cycles` C: (C + 1) * (6 + 94) + (C + 2) + 101 + 94 */
#define ZNGAMD_BGZF_QC_TABLE_WORDS(C) (((uint64_t)(C) + 1u) * (ZNGAMD_BGZF_QC_BASES + ZNGAMD_BGZF_QC_QUALITIES) + ((uint64_t)(C) + 2u) + \
                                       ZNGAMD_BGZF_QC_GC_BINS + ZNGAMD_BGZF_QC_QUALITIES)
typedef struct {
    uint32_t record_lines;  /* k, 1 .. 64 */
    int32_t  seq_line;      /* s */
    int32_t  qual_line;     /* q; -1: none */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    uint32_t quality_base;  /* 0 .. 255; 33 for Sanger / Illumina 1.8+ */
    uint32_t cycles;        /* C, 1 .. ZNGAMD_BGZF_QC_MAX_CYCLES */
    uint32_t low_quality;   /* 0 .. 93: a base with Q below it is a low one */
    uint32_t flags;         /* ZNGAMD_BGZF_QC_ROWS */
    uint32_t reserved[8];   /* 0 */
} zngamd_bgzf_qc_conf;                                                                            /* 64 B */
typedef struct {
    uint64_t qsum;          /* sum of Q_i; 0 when q = -1 */
    uint32_t len;           /* n */
    uint32_t gc;            /* bases of class 1 or 2 */
    uint32_t n;             /* bases of class 4 */
    uint32_t low;           /* bases with Q < low_quality; 0 when q = -1 */
} zngamd_bgzf_qc_row;                                                                             /* 24 B */
typedef struct {
    uint64_t seen;            /* records of the text that were counted (the open tail is not one of them) */
    uint64_t bytes_in;        /* bytes of the records as they lie in the text */
    uint64_t bases;           /* sum of n */
    uint64_t min_len;         /* UINT64_MAX when seen = 0 */
    uint64_t max_len;
    uint64_t empty;           /* records with n = 0 */
    uint64_t base_total[ZNGAMD_BGZF_QC_BASES];
    uint64_t quality_sum;     /* sum of Q_i over all records */
    uint64_t q20_bases;       /* Q >= 20 */
    uint64_t q30_bases;       /* Q >= 30 */
    uint64_t low_bases;       /* Q < low_quality */
    uint64_t quality_clamped; /* quality bytes below quality_base or above quality_base + 93 */
    uint64_t tail_off;        /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;      /* bad != 0: the number of the record at fault */
    uint64_t bad_src;         /*           and where it starts in the scratch */
    uint32_t covered;         /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;     /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;             /* 0; 1: the first byte is not first_byte; 3: the bodies of seq_line and qual_line differ in length */
    uint32_t reserved;
} zngamd_bgzf_qc_totals;                                                                          /* 176 B */
int zngamd_bgzf_qc_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                               uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_qc_conf *conf,
                               uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, uint64_t *d_tables,
                               uint64_t tables_cap, zngamd_bgzf_qc_row *d_rows, uint64_t rows_cap, zngamd_bgzf_qc_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status, the tables and, with _QC_ROWS, the rows come back.  With alloc
 * (rows = NULL, rows_cap 0) the caller's memory is asked for seen * 24 bytes once seen is known and not 0; NULL from it:
 * ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_qc_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                           uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_qc_conf *conf,
                           uint64_t record_base, int32_t *status, uint64_t *tables, uint64_t tables_cap, zngamd_bgzf_qc_row *rows,
                           uint64_t rows_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_qc_totals *totals);

/* ---- BGZF duplicate records (zlib_ng_amd/bgzf.py: key_records, dedup_keys, dedup_records, dedup_paired).  Two
 * calls.  zngamd_bgzf_key_records reduces the sequence of every record of a window to a 16-byte key; zngamd_dedup_keys finds, for any
 * number of such keys -- of one window, a file, several files, all shards -- the first record that carries each key and how many carry
 * it.  Keys are comparable wherever they were made, so the key function is part of this interface:
 *   part    the keyed part of a record is body[first : first + length] of its seq_line (length 0: to the end), clipped to the body: a
 *           body shorter than `first` has an empty part.  n is the part's length, c_0 .. c_{n-1} its bytes; with _KEY_IGNORE_CASE every
 *           byte a .. z is taken as A .. Z.  The record model is that of zngamd_bgzf_qc_records (a line the record lacks is an empty body).
 *   mix(x)  the splitmix64 step, modulo 2^64: x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 *           x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^= x >> 31.
 *   word_w  = mix(S_w ^ (1 << 63 | n)) + sum over i of mix(S_w ^ (i << 8 | c_i)), modulo 2^64, for w = 0, 1 with the seeds
 *           S_0 = ZNGAMD_BGZF_KEY_SEED0 and S_1 = ZNGAMD_BGZF_KEY_SEED1.  The key is (lo, hi) = (word_0, word_1).
 *   _KEY_CANONICAL  the key of the reverse complement -- position n - 1 - i and byte comp(c_i) in place of i and c_i; comp maps A<->T,
 *           C<->G, a<->t, c<->g, U->A, u->a and every other byte to itself (applied behind the case fold) -- is formed beside it, and the
 *           record's key is the smaller of the two as the 128-bit number hi << 64 | lo.
 * Equal keys are taken as equal sequences (as fastp takes its hashes): two different sequences share a key with a probability of about
 * 2^-128 per pair.
 * rows: one zngamd_bgzf_key_row per record in record order.  totals: seen, bytes_in, bases (the bytes of the seq_line bodies, whole),
 * tail_off, covered, short_lines and the fault words as zngamd_bgzf_qc_totals has them; bad = 1 is a first_byte violation, the smallest
 * record at fault is reported, and with bad set the rows are not to be used.  flags: _FINAL; anything else is ZNGAMD_E_ARG.
 * ZNGAMD_BUF_ERROR: rows_cap < seen: no row is written, the totals are valid.  Hostile arguments -- conf NULL or a field out of range, a
 * reserved word set, flags, totals NULL, rows NULL (and, in the host form, no alloc) -- are ZNGAMD_E_ARG before the context is touched.
 * Device memory beside the tiles: 8 bytes per line of the text, and in the host form 16 bytes per record. */
#define ZNGAMD_BGZF_KEY_IGNORE_CASE 1u
#define ZNGAMD_BGZF_KEY_CANONICAL   2u
#define ZNGAMD_BGZF_KEY_SEED0 0x243F6A8885A308D3ull
#define ZNGAMD_BGZF_KEY_SEED1 0x13198A2E03707344ull
typedef struct {
    uint32_t record_lines;  /* k, 1 .. 64 */
    int32_t  seq_line;      /* s, 0 <= s < k */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    uint32_t first;         /* where the keyed part begins in the body */
    uint32_t length;        /* its length; 0: to the end of the body */
    uint32_t flags;         /* ZNGAMD_BGZF_KEY_IGNORE_CASE | ZNGAMD_BGZF_KEY_CANONICAL */
    uint32_t reserved[10];  /* 0 */
} zngamd_bgzf_key_conf;                                                                           /* 64 B */
typedef struct {
    uint64_t lo;            /* word_0 */
    uint64_t hi;            /* word_1 */
} zngamd_bgzf_key_row;                                                                            /* 16 B */
typedef struct {
    uint64_t seen;            /* records of the text that were keyed (the open tail is not one of them) */
    uint64_t bytes_in;        /* bytes of the records as they lie in the text */
    uint64_t bases;           /* bytes of the seq_line bodies */
    uint64_t tail_off;        /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;      /* bad != 0: the number of the record at fault */
    uint64_t bad_src;         /*           and where it starts in the scratch */
    uint32_t covered;         /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;     /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;             /* 0; 1: the first byte is not first_byte */
    uint32_t reserved;
} zngamd_bgzf_key_totals;                                                                         /* 64 B */
int zngamd_bgzf_key_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_key_conf *conf,
                                uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_bgzf_key_row *d_rows,
                                uint64_t rows_cap, zngamd_bgzf_key_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status and the rows come back.  With alloc (rows = NULL, rows_cap 0) the
 * caller's memory is asked for seen * 16 bytes once seen is known and not 0; NULL from it: ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_key_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                            uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_key_conf *conf,
                            uint64_t record_base, int32_t *status, zngamd_bgzf_key_row *rows, uint64_t rows_cap, zngamd_alloc_fn alloc,
                            void *user, zngamd_bgzf_key_totals *totals);

/* zngamd_dedup_keys: for n keys (any 16-byte rows; those of zngamd_bgzf_key_records, or of pairs, files and shards put together),
 * first[r] = the smallest r' with keys[r'] == keys[r] (both words), count[r] = how many rows carry keys[r] when first[r] == r and 0
 * otherwise (it would saturate at 2^32 - 1; n <= ZNGAMD_DEDUP_MAX_KEYS keeps it below), and the totals: unique (the distinct keys),
 * duplicates = n - unique, max_count (the largest group) and max_first (its first row; the lowest such row when groups tie; 0 when n = 0).
 * first and count, either or both, may be NULL: the totals alone.  The result depends on the keys alone.  The work area is an
 * open-addressed table of cap = the smallest power of two that is >= 2 n and >= 64 slots of 8 bytes with cap counters of 4 bytes:
 * zngamd_dedup_scratch_bytes(n) bytes (0 for n > ZNGAMD_DEDUP_MAX_KEYS), 8-byte aligned.  n = 0 launches nothing.  ZNGAMD_E_ARG before
 * the context is touched: totals NULL, keys NULL with n != 0, n > ZNGAMD_DEDUP_MAX_KEYS, a scratch pointer that is NULL with n != 0 or
 * not 8-byte aligned.  ZNGAMD_BUF_ERROR: scratch_cap below zngamd_dedup_scratch_bytes(n); nothing is launched. */
#define ZNGAMD_DEDUP_MAX_KEYS (1ull << 30)
typedef struct {
    uint64_t n;
    uint64_t unique;
    uint64_t duplicates;
    uint64_t max_count;
    uint64_t max_first;
    uint64_t reserved;
} zngamd_dedup_totals;                                                                            /* 48 B */
uint64_t zngamd_dedup_scratch_bytes(uint64_t n);
int zngamd_dedup_keys_dev(zngamd_ctx *ctx, const zngamd_bgzf_key_row *d_keys, uint64_t n, void *d_scratch, uint64_t scratch_cap,
                          uint64_t *d_first, uint32_t *d_count, zngamd_dedup_totals *totals);
/* Host-buffer form: the keys are uploaded, the table is the context's, first and count (each NULL or n entries) come back. */
int zngamd_dedup_keys(zngamd_ctx *ctx, const zngamd_bgzf_key_row *keys, uint64_t n, uint64_t *first, uint32_t *count,
                      zngamd_dedup_totals *totals);

/* ---- BGZF sort (zlib_ng_amd/bgzf.py: sort_key_records, sort_keys, permute_records, sort_records).  Three
 * calls, each usable alone: a key per record whose memcmp order is the order wanted, a stable sort of any such keys, and records
 * written to the places the caller names.  The record model of zngamd_bgzf_key_records applies (record_lines k, first_byte, _FINAL, the
 * open tail, the cover contract; a line the record lacks is an empty body).
 * The key.  conf holds 0 .. 4 parts; the key is the parts' bytes one behind the other, padded with 0x00 to W = the next multiple of 8
 * (W <= 256; W = 0 with no part: the lengths alone).  A part names a field -- line `line` of the record, whole (column = -1) or its
 * 0-based field `column` when the body is cut at the byte `sep`; a line the record lacks or a column the line lacks is an empty field --
 * and how its bytes are made:
 *   _SORT_BYTES   width bytes (8 .. 128, a multiple of 8): field[first : first + width], padded with 0x00; with _IGNORE_CASE a .. z
 *                 become A .. Z.  A field longer than first + width is fault 3 unless the part has _TRUNCATE.
 *   _SORT_NUMBER  8 bytes, big-endian: the field as an unsigned decimal number; leading zeros are allowed.  An empty field, a byte that
 *                 is no digit, or a value above 2^64 - 1 is fault 2.
 *   _SORT_LENGTH  4 bytes, big-endian: the length of the field.
 * _REVERSE complements the part's bytes.  A record whose first byte is meta_byte (-1: none) gets the all-zero key and no fault of a
 * part: with the stable sort the header lines of a VCF stay in front and in order.
 * Rows.  rows: row r is the W key bytes of record r, row-major; lengths[r] (uint32_t): the record's bytes as they lie in the text --
 * except that the last record of a _FINAL text whose last line lacks its delimiter counts one byte more: zngamd_bgzf_place_records
 * writes that delimiter, so a reordered file never glues two lines together.  This is the one deviation from "the output's bytes
 * are a permutation of the input's records".
 * totals: seen, bytes_in, tail_off, covered, short_lines and the fault words as zngamd_bgzf_key_totals has them; key_width = W; bad:
 * 1 a first_byte violation, 2 not a number, 3 a _SORT_BYTES field too long (max_field: the longest such field of the window, so
 * that a caller can say which width would do).  The smallest record at fault is reported (of two faults at one record the one
 * with the lower number); with bad set the rows are not to be used.  flags: _FINAL; anything else is ZNGAMD_E_ARG.
 * ZNGAMD_BUF_ERROR: rows_cap < seen: nothing is written, the totals are valid.  Hostile arguments -- conf NULL or a field out of range
 * (record_lines, first_byte, meta_byte, n_parts > 4, line, column < -1, kind, width, a part's flags), a reserved word set, W > 256,
 * flags, delim, totals NULL, lengths NULL or rows NULL with W != 0 (and, in the host form, no alloc) -- are ZNGAMD_E_ARG before the
 * context is touched.  Device memory beside the tiles: 8 bytes per line of the text, and in the host form W + 4 bytes per record. */
#define ZNGAMD_BGZF_SORT_BYTES  0u
#define ZNGAMD_BGZF_SORT_NUMBER 1u
#define ZNGAMD_BGZF_SORT_LENGTH 2u
#define ZNGAMD_BGZF_SORT_REVERSE     1u
#define ZNGAMD_BGZF_SORT_IGNORE_CASE 2u
#define ZNGAMD_BGZF_SORT_TRUNCATE    4u
#define ZNGAMD_BGZF_SORT_MAX_PARTS 4u
#define ZNGAMD_SORT_MAX_WIDTH 256u
typedef struct {
    int32_t  line;          /* 0 <= line < record_lines */
    int32_t  column;        /* -1: the whole body; otherwise the 0-based field between separators */
    uint32_t width;         /* _SORT_BYTES: 8 .. 128, a multiple of 8; otherwise 0 */
    uint32_t first;         /* _SORT_BYTES: where the keyed bytes begin in the field; otherwise 0 */
    uint16_t flags;         /* ZNGAMD_BGZF_SORT_REVERSE | _IGNORE_CASE | _TRUNCATE (the last two: _SORT_BYTES only) */
    uint8_t  kind;          /* ZNGAMD_BGZF_SORT_BYTES, _NUMBER, _LENGTH */
    uint8_t  sep;           /* the separator of the columns */
} zngamd_bgzf_sort_part;                                                                          /* 20 B */
typedef struct {
    uint32_t record_lines;  /* k, 1 .. 64 */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    int32_t  meta_byte;     /* 0 .. 255; -1: none */
    uint32_t n_parts;       /* 0 .. 4 */
    zngamd_bgzf_sort_part part[4];
    uint32_t reserved[8];   /* 0; so are the parts at and behind n_parts */
} zngamd_bgzf_sort_conf;                                                                          /* 128 B */
typedef struct {
    uint64_t seen;            /* records of the text that were keyed (the open tail is not one of them) */
    uint64_t bytes_in;        /* bytes of the records as they lie in the text */
    uint64_t max_field;       /* bad = 3: the longest field that was too long */
    uint64_t tail_off;        /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;      /* bad != 0: the number of the record at fault */
    uint64_t bad_src;         /*           and where it starts in the scratch */
    uint32_t covered;         /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;     /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;             /* 0; 1: the first byte is not first_byte; 2: not a number; 3: a field too long */
    uint32_t key_width;       /* W */
} zngamd_bgzf_sort_key_totals;                                                                    /* 64 B */
int zngamd_bgzf_sort_key_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                     uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_sort_conf *conf,
                                     uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, uint8_t *d_rows,
                                     uint32_t *d_lengths, uint64_t rows_cap, zngamd_bgzf_sort_key_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status, the rows and the lengths come back.  With alloc (rows = lengths =
 * NULL, rows_cap 0) the caller's memory is asked for once seen is known and not 0, in the order rows (seen * W bytes; not with W = 0),
 * lengths (seen * 4 bytes); NULL from it: ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_sort_key_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                                 uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_sort_conf *conf,
                                 uint64_t record_base, int32_t *status, uint8_t *rows, uint32_t *lengths, uint64_t rows_cap,
                                 zngamd_alloc_fn alloc, void *user, zngamd_bgzf_sort_key_totals *totals);

/* zngamd_sort_keys: n rows of `width` bytes (a multiple of 8, 8 .. 256), row-major, of any origin.  order[j] (uint32_t) = the row that
 * stands j-th in memcmp order; equal rows come in ascending row number (the sort is stable), so the result depends on the rows
 * alone.  rank (NULL, or n entries) is the inverse: rank[order[j]] = j.  An LSD radix sort over bytes, the last byte first; a byte
 * position that is the same in every row (the OR of the rows equals their AND there) gets no pass, so the cost follows the bytes
 * that vary, not the width.  The rows are never written.  The device form's work area is zngamd_sort_scratch_bytes(n, width)
 * bytes (0 for n > ZNGAMD_SORT_MAX_KEYS or a width out of range), 8-byte aligned, as d_keys is.  n = 0 launches nothing.
 * ZNGAMD_E_ARG before the context is touched: order NULL or keys NULL with n != 0, n > ZNGAMD_SORT_MAX_KEYS, a width out of range, a
 * work area or d_keys that is NULL with n != 0 or not 8-byte aligned.  ZNGAMD_BUF_ERROR: scratch_cap below
 * zngamd_sort_scratch_bytes(n, width); nothing is launched. */
#define ZNGAMD_SORT_MAX_KEYS (1ull << 30)
uint64_t zngamd_sort_scratch_bytes(uint64_t n, uint32_t width);
int zngamd_sort_keys_dev(zngamd_ctx *ctx, const uint8_t *d_keys, uint64_t n, uint32_t width, void *d_scratch, uint64_t scratch_cap,
                         uint32_t *d_order, uint32_t *d_rank);
/* Host-buffer form: the rows are uploaded, the work area is the context's, order and rank (NULL or n entries) come back. */
int zngamd_sort_keys(zngamd_ctx *ctx, const uint8_t *keys, uint64_t n, uint32_t width, uint32_t *order, uint32_t *rank);

/* zngamd_bgzf_place_records: the window is decoded as in every record call, and record record_base + r is copied whole to
 * d_out + dst[r]; dst[r] = ZNGAMD_BGZF_PLACE_SKIP: the record is not in this pass.  length[r] is what zngamd_bgzf_sort_key_records
 * reported: where it counted the delimiter an open last line lacks, the delimiter is written behind the record.  Nothing is written
 * outside [dst[r], dst[r] + length[r]), and d_out (out_cap bytes) is DEVICE memory in both forms.  Faults (the smallest record at
 * fault; a record at fault is not copied, the others are): bad = 1 a first_byte violation; 4 the record's length in the text is not
 * length[r] -- the file changed between the passes; 5 dst[r] + length[r] > out_cap.  Only the first min(n, seen) entries of the
 * arrays are read; seen > n: labels_short = 1 and nothing is written, as in zngamd_bgzf_partition_records; n > seen is no fault: the
 * next call takes dst + seen.  totals: seen, placed (records copied), placed_bytes (the sum of their length[r]) and the rest as
 * zngamd_bgzf_partition_totals has it.  flags: _FINAL.  Hostile arguments -- dst or length NULL with n != 0, d_out NULL with
 * out_cap != 0, record_lines / first_byte, delim, flags, totals NULL -- are ZNGAMD_E_ARG before the context is touched. */
#define ZNGAMD_BGZF_PLACE_SKIP (~0ull)
typedef struct {
    uint64_t seen;          /* records of the text that were decided (the open tail is not one of them) */
    uint64_t placed;        /* records copied */
    uint64_t placed_bytes;  /* and the bytes written for them */
    uint64_t tail_off;      /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;    /* bad != 0: the number of the record at fault */
    uint64_t bad_src;       /*           and where it starts in the scratch */
    uint32_t covered;       /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;   /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;           /* 0; 1: the first byte is not first_byte; 4: the length is not length[r]; 5: the record does not fit */
    uint32_t labels_short;  /* 1: the text holds more records than n */
} zngamd_bgzf_place_totals;                                                                       /* 64 B */
int zngamd_bgzf_place_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                  uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines,
                                  int32_t first_byte, uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status,
                                  const uint64_t *d_dst, const uint32_t *d_length, uint64_t n, void *d_out, uint64_t out_cap,
                                  zngamd_bgzf_place_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; dst and length are host memory, of which min(n, seen) entries are
 * uploaded once the line count is known; status comes back; d_out stays a device pointer. */
int zngamd_bgzf_place_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                              uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, uint32_t record_lines,
                              int32_t first_byte, uint64_t record_base, int32_t *status, const uint64_t *dst, const uint32_t *length,
                              uint64_t n, void *d_out, uint64_t out_cap, zngamd_bgzf_place_totals *totals);

/* ---- BGZF screen (zlib_ng_amd/bgzf.py: KmerSet, screen_records, screen_filter).  Which reads come from
 * something that should not be in the library -- bbduk ref=phix.fa k=31, fastq_screen, rRNA depletion, spike-in and vector removal: a
 * set of the k-mers of up to 64 references on the device, and every k-mer of every read looked up in it.  The rule:
 *   bases      A, C, G, T in either case are 0, 1, 2, 3; U and u count as T; every other byte is invalid.
 *   forward    a k-mer is k consecutive bytes of ONE sequence, 1 <= k <= 31; its forward code is the sum over i of base_i << 2 (k - 1 - i):
 *              the first base is the most significant.
 *   canonical  with ZNGAMD_KMER_CANONICAL the code is the smaller of the forward code and the code of the reverse complement (the
 *              complement of base b is 3 - b).  A k-mer with an invalid byte has no code.
 *   empty      every code is below 4^31 = 2^62; the all-ones word marks an empty slot.
 *   set        made from R references, 1 <= R <= 64, each a byte string: every code that occurs at some position of some reference, with
 *              a 64-bit mask whose bit j is set when reference j holds the code.  k-mers do not span references; a reference shorter
 *              than k adds nothing; a set may be empty.
 *   record     the sequence is the body of seq_line, n bytes (the record model is that of the key call above; a line the record lacks
 *              is an empty body); its positions are p = 0 .. n - k, none when n < k.  kmers: the positions whose k-mer is valid.  hits: the
 *              valid positions whose code is in the set.  refs: the OR of the masks of the hit codes.  best: the reference that the most
 *              hit positions count for -- a position counts for every reference whose bit is set in its mask -- the lowest number among
 *              equals, ZNGAMD_KMER_NONE when hits == 0.  best_hits: the count for best.
 *   match      a record is matched when hits >= min_hits (min_hits >= 1).
 * The set is an opaque object: read-only once made, bound to the context it was made in (free it before that context is destroyed), and
 * usable by any number of later calls.  Its table is cap slots of 16 bytes, code and mask; cap is the smallest power of two that is
 * >= 2 x positions (so >= 2 x valid; for the load call: >= 2 n) and >= 64; a code's home slot is mix(code) & (cap - 1) with the mix of the
 * key call above, probing is linear with wrap.  At most ZNGAMD_KMER_MAX_POSITIONS reference positions (the sum of len - k + 1 over the
 * references of at least k bytes).
 *   _build   the references lie one behind the other in seqs (host memory): reference j is seqs[offsets[j] .. offsets[j + 1]); offsets
 *            has n_refs + 1 entries that do not decrease.  The set is built on the GPU.  info (may be NULL): k, flags, n_refs, positions,
 *            valid (the positions whose k-mer is valid), distinct (the codes of the set), cap.
 *   _load    the same table from n (code, mask) pairs; a code that appears twice ORs its masks.  ZNGAMD_E_ARG when a code is >= 4^k, or
 *            a mask is 0 or has a bit at or above n_refs.  info: positions = valid = n.
 *   _export  the set's pairs in no particular order; *n = distinct.  ZNGAMD_BUF_ERROR, with *n set, when cap_pairs < distinct.
 *   _describe  the info of a set; _free releases it (NULL: nothing happens).
 * ZNGAMD_E_ARG before the context is touched: k out of range, n_refs 0 or above 64, offsets that decrease, too many positions, unknown
 * flags, a NULL pointer (seqs may be NULL when the references hold no byte, codes and masks when n = 0). */
#define ZNGAMD_KMER_CANONICAL     1u
#define ZNGAMD_KMER_NONE          0xFFFFFFFFu
#define ZNGAMD_KMER_MAX_K         31u
#define ZNGAMD_KMER_MAX_REFS      64u
#define ZNGAMD_KMER_MAX_POSITIONS (1ull << 28)
typedef struct zngamd_kmer_set zngamd_kmer_set;
typedef struct {
    uint32_t k;
    uint32_t flags;           /* ZNGAMD_KMER_CANONICAL */
    uint32_t n_refs;
    uint32_t reserved;
    uint64_t positions;       /* reference positions (pairs given, for a loaded set) */
    uint64_t valid;           /* of them, those whose k-mer is valid */
    uint64_t distinct;        /* codes in the set */
    uint64_t cap;             /* slots of the table */
} zngamd_kmer_set_info;                                                                           /* 48 B */
int zngamd_kmer_set_build(zngamd_ctx *ctx, const uint8_t *seqs, const uint64_t *offsets, uint32_t n_refs, uint32_t k, uint32_t flags,
                          zngamd_kmer_set **out, zngamd_kmer_set_info *info);
int zngamd_kmer_set_load(zngamd_ctx *ctx, uint32_t k, uint32_t flags, uint32_t n_refs, const uint64_t *codes, const uint64_t *masks,
                         uint64_t n, zngamd_kmer_set **out, zngamd_kmer_set_info *info);
int zngamd_kmer_set_export(zngamd_kmer_set *set, uint64_t *codes, uint64_t *masks, uint64_t cap_pairs, uint64_t *n);
int zngamd_kmer_set_describe(const zngamd_kmer_set *set, zngamd_kmer_set_info *info);
void zngamd_kmer_set_free(zngamd_kmer_set *set);

/* The screen of a window: the window arguments, delimiter and flags of the key call, the rule above with the k and flags of the set.
 * rows: one zngamd_bgzf_screen_row per record in record order.  totals: those of zngamd_bgzf_key_totals, then kmers, hits (summed
 * over the records) and matched (the records with hits >= min_hits).  bad, tail_off, short_lines, _FINAL, rows_cap < seen
 * (ZNGAMD_BUF_ERROR: no row is written, the totals are valid) and the alloc form behave exactly as in the key call.  ZNGAMD_E_ARG before
 * the context is touched: what the key call refuses, conf.flags or a reserved word set, min_hits == 0, set NULL, a set made in
 * another context.  Device memory beside the tiles: 8 bytes per line of the text, and in the host form 24 bytes per record. */
typedef struct {
    uint32_t record_lines;  /* 1 .. 64 */
    int32_t  seq_line;      /* 0 <= s < record_lines */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    uint32_t min_hits;      /* >= 1 */
    uint32_t flags;         /* 0: none yet */
    uint32_t reserved[11];  /* 0 */
} zngamd_bgzf_screen_conf;                                                                        /* 64 B */
typedef struct {
    uint64_t refs;          /* the OR of the masks of the hit codes */
    uint32_t kmers;         /* valid positions */
    uint32_t hits;          /* of them, those whose code is in the set */
    uint32_t best;          /* the reference with the most hit positions; ZNGAMD_KMER_NONE */
    uint32_t best_hits;     /* its count */
} zngamd_bgzf_screen_row;                                                                         /* 24 B */
typedef struct {
    uint64_t seen;            /* as zngamd_bgzf_key_totals ... */
    uint64_t bytes_in;
    uint64_t bases;
    uint64_t tail_off;
    uint64_t bad_record;
    uint64_t bad_src;
    uint32_t covered;
    uint32_t short_lines;
    uint32_t bad;
    uint32_t reserved;
    uint64_t kmers;           /* ... then the valid positions of all records */
    uint64_t hits;            /* the hit positions of all records */
    uint64_t matched;         /* records with hits >= min_hits */
} zngamd_bgzf_screen_totals;                                                                      /* 88 B */
int zngamd_bgzf_screen_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                   uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_screen_conf *conf,
                                   const zngamd_kmer_set *set, uint64_t record_base, void *d_scratch, uint64_t scratch_cap,
                                   int32_t *d_status, zngamd_bgzf_screen_row *d_rows, uint64_t rows_cap,
                                   zngamd_bgzf_screen_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status and the rows come back.  With alloc (rows = NULL, rows_cap 0) the
 * caller's memory is asked for seen * 24 bytes once seen is known and not 0; NULL from it: ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_screen_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                               uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_screen_conf *conf,
                               const zngamd_kmer_set *set, uint64_t record_base, int32_t *status, zngamd_bgzf_screen_row *rows,
                               uint64_t rows_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_screen_totals *totals);

/* ---- BGZF count (zlib_ng_amd/bgzf.py: KmerCounter, count_kmers, KmerCounts).  Which k-mers the reads of a
 * library hold themselves, and how often -- jellyfish count and histo, KMC, FastQC's "Kmer Content", the k-mer spectrum behind
 * genome-size and heterozygosity estimates, and the solid k-mers that become the set of the next screen.  The rule:
 *   codes      bases, forward and canonical codes and invalid bytes are exactly those of the screen section above; 1 <= k <= 31;
 *              ZNGAMD_KMER_CANONICAL applies as there.
 *   record     the sequence is the body of seq_line, n bytes (the record model is that of the key call); its positions are 0 .. n - k,
 *              none when n < k.  Every position whose k-mer is valid adds 1 to the count of its code.
 *   counter    an opaque object that accumulates over any number of calls -- windows, files, shards.  Counts are exact uint64_t.
 *   runs       (bookkeeping only, it changes no count) the positions of a record are taken in strips of 64 from position 0; within a
 *              strip a run is a longest stretch of consecutive valid positions with one code, and costs one atomic add.  adds: the runs.
 * The counter owns its device table and is bound to the context it was made in (free it before that context is destroyed).  The table
 * is cap slots of 16 bytes, code and count; cap is a power of two >= 64; an empty slot has the code all ones and the count 0; a code's
 * home slot is mix(code) & (cap - 1) with the mix of the key call, probing is linear with wrap.  INVARIANT: before anything is launched
 * the host checks distinct + room <= cap / 2, where distinct is the slots claimed so far and room bounds what the launch can claim
 * (text_end - text_off for a window, n for _add, the old distinct for a rehash); so at most cap / 2 slots are ever claimed, an empty
 * slot lies ahead of every home and every probe loop ends.  A call that fails the check returns ZNGAMD_BUF_ERROR, launches nothing and
 * leaves the counter as it was: _reserve first.
 *   _new        k, flags, and room for `room` codes: cap is the smallest power of two >= max(64, 2 * room).
 *   _reserve    nothing when distinct + room <= cap / 2; otherwise a table of the smallest power of two >= 4 * (distinct + room) slots is
 *               cleared, the pairs are rehashed into it and the old one is freed after that.  ZNGAMD_MEM_ERROR when the device cannot give
 *               the table, ZNGAMD_E_ARG above ZNGAMD_KMER_COUNTER_MAX_CAP slots: the counter is unchanged in both cases.
 *   _add        n (code, count) pairs from host memory; a code that appears twice adds its counts.  ZNGAMD_E_ARG, judged before any
 *               launch, for a code >= 4^k or a count of 0; ZNGAMD_BUF_ERROR unless distinct + n <= cap / 2.
 *   _describe   k, flags, poisoned, cap, distinct and total, the sum of all counts.
 *   _histogram  2 <= bins <= ZNGAMD_KMER_HIST_MAX_BINS.  hist[0] = 0; hist[c] is the number of codes with count c for c < bins - 1;
 *               hist[bins - 1] is the number of codes with count >= bins - 1 (jellyfish histo -h).
 *   _export     the pairs with min_count <= count <= max_count in no particular order; min_count >= 1; max_count 0: no upper bound.
 *               *n: how many there are.  ZNGAMD_BUF_ERROR, with *n set and nothing written, when cap_pairs is less.
 *   _free       releases it (NULL: nothing happens).
 * POISON: a window call that ends with totals.bad != 0, or that fails after its kernels have started, has added an unknown part of the
 * window.  The counter is then poisoned: info.poisoned = 1, and every later call on it but _describe and _free returns ZNGAMD_E_ARG. */
#define ZNGAMD_KMER_COUNTER_MAX_CAP (1ull << 33)
#define ZNGAMD_KMER_HIST_MAX_BINS   16384u
typedef struct zngamd_kmer_counter zngamd_kmer_counter;
typedef struct {
    uint32_t k;
    uint32_t flags;           /* ZNGAMD_KMER_CANONICAL */
    uint32_t poisoned;        /* 1: a window call left an unknown part of its window in the counts */
    uint32_t reserved;
    uint64_t cap;             /* slots of the table */
    uint64_t distinct;        /* codes counted: the slots claimed */
    uint64_t total;           /* the sum of all counts */
    uint64_t reserved2[3];
} zngamd_kmer_counter_info;                                                                       /* 64 B */
int zngamd_kmer_counter_new(zngamd_ctx *ctx, uint32_t k, uint32_t flags, uint64_t room, zngamd_kmer_counter **out);
int zngamd_kmer_counter_reserve(zngamd_kmer_counter *counter, uint64_t room);
int zngamd_kmer_counter_add(zngamd_kmer_counter *counter, const uint64_t *codes, const uint64_t *counts, uint64_t n);
int zngamd_kmer_counter_describe(const zngamd_kmer_counter *counter, zngamd_kmer_counter_info *info);
int zngamd_kmer_counter_histogram(zngamd_kmer_counter *counter, uint64_t *hist, uint32_t bins);
int zngamd_kmer_counter_export(zngamd_kmer_counter *counter, uint64_t min_count, uint64_t max_count, uint64_t *codes, uint64_t *counts,
                               uint64_t cap_pairs, uint64_t *n);
void zngamd_kmer_counter_free(zngamd_kmer_counter *counter);

/* The count of a window: the window arguments, delimiter and flags of the screen call, the rule above with the k and flags of the
 * counter.  No rows.  totals: those of zngamd_bgzf_key_totals at their offsets, then kmers (the valid positions), claimed (the slots
 * newly claimed: the counter's distinct grows by it) and adds (the runs).  bad, tail_off, short_lines, covered and _FINAL behave as in
 * the key call; the open tail behind the last complete record is not counted, the next window counts it.  ZNGAMD_E_ARG before the
 * context is touched: what the screen call refuses, a counter that is NULL, poisoned or of another context.  ZNGAMD_BUF_ERROR, with
 * nothing launched, unless distinct + (text_end - text_off) <= cap / 2.  Device memory beside the tiles: 8 bytes per line of the text. */
typedef struct {
    uint32_t record_lines;  /* 1 .. 64 */
    int32_t  seq_line;      /* 0 <= s < record_lines */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    uint32_t flags;         /* 0: none yet */
    uint32_t reserved[12];  /* 0 */
} zngamd_bgzf_count_conf;                                                                         /* 64 B */
typedef struct {
    uint64_t seen;            /* as zngamd_bgzf_key_totals ... */
    uint64_t bytes_in;
    uint64_t bases;
    uint64_t tail_off;
    uint64_t bad_record;
    uint64_t bad_src;
    uint32_t covered;
    uint32_t short_lines;
    uint32_t bad;
    uint32_t reserved;
    uint64_t kmers;           /* ... then the valid positions of all records */
    uint64_t claimed;         /* the slots newly claimed */
    uint64_t adds;            /* the atomic adds issued: the runs */
} zngamd_bgzf_count_totals;                                                                       /* 88 B */
int zngamd_bgzf_count_kmers_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_count_conf *conf,
                                zngamd_kmer_counter *counter, uint64_t record_base, void *d_scratch, uint64_t scratch_cap,
                                int32_t *d_status, zngamd_bgzf_count_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status comes back. */
int zngamd_bgzf_count_kmers(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                            uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_count_conf *conf,
                            zngamd_kmer_counter *counter, uint64_t record_base, int32_t *status, zngamd_bgzf_count_totals *totals);

/* ---- BGZF overlap (zlib_ng_amd/bgzf.py: overlap_records).  The one preprocessing step that needs both mates
 * of a pair at once: where the two reads of a pair lie over each other, and with that the adapter read-through cut off, bases
 * corrected and the pair merged into one read -- fastp's overlap analysis (-c, -m), bbmerge, PEAR, FLASH, vsearch
 * --fastq_mergepairs.  Interleaved input only: one record is one pair.  All integers, all bytes exact.
 * Record model.  The record model of zngamd_bgzf_grep_records applies (record_lines k, first_byte, _FINAL, the open tail, the cover
 * contract).
 *   - record_lines k is even, 2 <= k <= 64, m = k / 2.
 *   - Mate 1 is lines [0, m) of the record.  Mate 2 is lines [m, k).
 *   - seq_line s and qual_line q (-1: none) lie in [0, m), q != s.  They name the same line of both mates.
 *   - Bodies are the lines without the delimiter.
 *   - Under _FINAL, a line the short last record lacks is an empty body.
 * Notation.
 *   - a is mate 1's sequence body (n1 bytes), qa its quality body.
 *   - y, qy are mate 2's bodies (n2 bytes).
 *   - b[j] = comp(y[n2 - 1 - j]) and qb[j] = qy[n2 - 1 - j].
 *   - comp is za_key_comp's map (the one behind ZNGAMD_BGZF_KEY_CANONICAL): A<->T and C<->G in either case, U -> A, u -> a, every
 *     other byte itself.
 *   - Qx = qx - quality_base, signed.  With q = -1 every Q counts as 0.
 * 1. Search.  For every offset o in [-(n2 - 1), n1 - 1], b[j] lies under a[o + j].
 *   - The overlap is i in [max(0, o), min(n1, o + n2)).
 *   - L(o) is its length.
 *   - d(o) is the number of i with a[i] != b[i - o].  Bytes are compared as they are, so N equals N.
 *   - o is acceptable when L >= min_overlap and d <= min(max_mismatch, L * max_percent / 100).
 *   - The acceptable offset that is first in this order wins:
 *       1. larger L;
 *       2. then smaller d;
 *       3. then smaller |o|;
 *       4. then o >= 0 before o < 0.
 *   - No two offsets share all four values, so the winner is unique.  This is fastp's "longest acceptable overlap first", made total.
 *   - Limits: min_overlap 1 .. 1024, max_mismatch 0 .. 1024, max_percent 0 .. 100.
 *   - A pair with n1 or n2 above ZNGAMD_BGZF_OVERLAP_MAX_READ (1024) is not searched: verdict _TOO_LONG.
 *   - Reason for the limit: it bounds a wave's LDS stage and the worst case.  Illumina's longest mate is 300.
 *   - With an overlap found, insert = o + n2 (>= 1).
 * 2. Correction (conf.flags & _OVERLAP_CORRECT; needs q >= 0, else ZNGAMD_E_ARG).  At every overlap position with a[i] != b[i - o]:
 *   - if Qa >= q_high and Qb <= q_low, mate 2 takes mate 1's byte and quality there (y gets comp(a[i]));
 *   - else if Qb >= q_high and Qa <= q_low, mate 1 takes b's byte and quality.
 *   - q_high and q_low are 0 .. 93; fastp's are 30 and 14.
 *   - `corrected` counts the positions.  It is counted whether or not the pair is then merged.
 * 3. Cut (_OVERLAP_CUT), for a pair with an overlap found.
 *   - Mate 1 keeps a[0, min(n1, insert)).
 *   - Mate 2 keeps y[0, min(n2, n2 + o)).
 *   - What falls off is adapter read-through.
 *   - It is summed in adapter_trimmed (bases) and adapter_pairs, whether or not the pair is then merged.
 * 4. Merge (_OVERLAP_MERGE), for a pair with an overlap found.  The merged read has `insert` positions c.
 *   - Where only one mate covers c, it gives base and quality.
 *   - Where both cover c, the mate with the higher Q gives base and quality.  This uses the Q of the source text as it stood before
 *     step 2.  Mate 1 wins on ties, so always with q = -1.
 *   - Correction therefore changes no merged byte; it only counts.
 *   - Written: mate 1's m lines, with lines s and q carrying the merged bodies, every other line whole, every delimiter mate 1's
 *     source has.  Nothing of mate 2's other lines is written.
 * Verdicts (uint8): _NONE 0, _FOUND 1 (overlap, _MERGE off), _MERGED 2, _TOO_LONG 3.
 * Classes.
 *   - Class 0 is the merged records (m lines each).
 *   - Class 1 is every other pair (k lines each, as step 2 and step 3 left them; a _TOO_LONG pair whole).
 *   - With ZNGAMD_BGZF_CLASSIFY_GROUP, class 0 is gathered: d_rows holds a row per merged pair in record order (src_off: where the
 *     record starts in the scratch; number = record_base + r; len: its bytes as written; reserved: the class), d_out the bytes.
 *   - Class 1 is gathered behind it only with _OVERLAP_KEEP_UNMERGED.  This is exactly how _TRIM_KEEP_SHORT works.
 *   - Without _GROUP only d_overlap[0 .. seen), one row per pair in record order, and the totals leave the kernels.
 * Faults.
 *   - bad = 1: the first byte of line 0 or of line m is not first_byte (a line the record lacks has no first byte).
 *   - bad = 3: a mate's sequence and quality bodies differ in length.
 *   - The smaller record wins.  A record with both faults reports 1.  With bad set, nothing is written; the counts are valid except
 *     that a pair whose bodies differ is not searched.  This is trim's contract.
 * flags: _FINAL and ZNGAMD_BGZF_CLASSIFY_GROUP; anything else is ZNGAMD_E_ARG.  ZNGAMD_BUF_ERROR: overlap_cap < seen or, with _GROUP,
 * rows_cap or out_cap too small; nothing is written, the totals are valid.  Hostile arguments -- conf NULL or a field out of range, k
 * odd, s or q not below m, q == s, _OVERLAP_CORRECT with q = -1, a reserved word set, flags, totals NULL -- are ZNGAMD_E_ARG before
 * the context is touched.  Device memory beside the tiles: 8 bytes per line and 22 bytes per record of the text, and 16 bytes per 256
 * records. */
#define ZNGAMD_BGZF_OVERLAP_NONE     0u
#define ZNGAMD_BGZF_OVERLAP_FOUND    1u
#define ZNGAMD_BGZF_OVERLAP_MERGED   2u
#define ZNGAMD_BGZF_OVERLAP_TOO_LONG 3u
#define ZNGAMD_BGZF_OVERLAP_MERGE         1u   /* conf.flags: step 4 */
#define ZNGAMD_BGZF_OVERLAP_CORRECT       2u   /*             step 2 */
#define ZNGAMD_BGZF_OVERLAP_CUT           4u   /*             step 3 */
#define ZNGAMD_BGZF_OVERLAP_KEEP_UNMERGED 8u   /*             class 1 is gathered behind class 0, not only counted */
#define ZNGAMD_BGZF_OVERLAP_MAX_READ    1024u
#define ZNGAMD_BGZF_OVERLAP_MAX_QUALITY 93u
typedef struct {
    uint32_t record_lines;  /* k, even, 2 .. 64 */
    int32_t  seq_line;      /* s, below k / 2 */
    int32_t  qual_line;     /* q; -1: none */
    int32_t  first_byte;    /* 0 .. 255; -1: no check */
    uint32_t quality_base;  /* 0 .. 255; 33 for Sanger / Illumina 1.8+ */
    uint32_t min_overlap;   /* step 1: 1 .. 1024 */
    uint32_t max_mismatch;  /* 0 .. 1024 */
    uint32_t max_percent;   /* 0 .. 100 */
    uint32_t q_high;        /* step 2: 0 .. 93 */
    uint32_t q_low;
    uint32_t flags;         /* ZNGAMD_BGZF_OVERLAP_MERGE | _CORRECT | _CUT | _KEEP_UNMERGED */
    uint32_t reserved[5];   /* 0 */
} zngamd_bgzf_overlap_conf;                                                                       /* 64 B */
typedef struct {
    int32_t  offset;        /* o; 0 without an overlap */
    uint32_t insert;        /* o + n2; 0: none */
    uint16_t overlap;       /* L */
    uint16_t mismatches;    /* d */
    uint16_t corrected;     /* positions step 2 changed */
    uint8_t  verdict;       /* ZNGAMD_BGZF_OVERLAP_NONE / _FOUND / _MERGED / _TOO_LONG */
    uint8_t  steps;         /* bit 0: mate 1 cut, bit 1: mate 2 cut, bit 2: corrected */
} zngamd_bgzf_overlap_row;                                                                        /* 16 B */
typedef struct {
    uint64_t seen;            /* pairs of the text that were decided (the open tail is not one of them) */
    uint64_t none;            /* of them, per verdict */
    uint64_t found;
    uint64_t merged;
    uint64_t too_long;
    uint64_t bytes_in;        /* bytes of the records as they lie in the text */
    uint64_t bytes;           /* bytes of the records as written: class 0 and, with _OVERLAP_KEEP_UNMERGED, class 1 */
    uint64_t bases_in;        /* sum of n1 + n2 */
    uint64_t bases_merged;    /* sum of insert over the merged pairs */
    uint64_t corrected;       /* positions step 2 changed, over all pairs */
    uint64_t corrected_pairs; /* pairs with at least one */
    uint64_t adapter_pairs;   /* pairs step 3 cut */
    uint64_t adapter_trimmed; /* bases step 3 took, over both mates */
    uint64_t overlap_sum;     /* sum of L over the pairs with an overlap */
    uint64_t mismatch_sum;    /* sum of d over them */
    uint64_t tail_off;        /* scratch offset where the open record starts; text_end when there is none */
    uint64_t bad_record;      /* bad != 0: the number of the record at fault */
    uint64_t bad_src;         /*           and where it starts in the scratch */
    uint32_t covered;         /* 1: decoded blocks cover the text and the figures describe it */
    uint32_t short_lines;     /* with _FINAL: lines of a short last record; 0 when the last record is whole */
    uint32_t bad;             /* 0; 1: line 0 or line m does not begin with first_byte; 3: a mate's two bodies differ in length */
    uint32_t reserved;
} zngamd_bgzf_overlap_totals;                                                                     /* 160 B */
int zngamd_bgzf_overlap_records_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                    uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_overlap_conf *conf,
                                    uint64_t record_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status,
                                    zngamd_bgzf_overlap_row *d_overlap, uint64_t overlap_cap, zngamd_bgzf_grep_row *d_rows, uint64_t rows_cap,
                                    void *d_out, uint64_t out_cap, zngamd_bgzf_overlap_totals *totals);
/* Host-buffer form: stages as zngamd_bgzf_grep_records does; status, the overlap rows and, with _GROUP, the rows and the written
 * records come back.  With alloc (overlap = rows = out = NULL, the capacities 0) the caller's memory is asked for once the sizes are
 * known, in the order overlap rows (seen * 16 bytes), rows ((merged [+ the others]) * 24 bytes), bytes -- the last two with _GROUP
 * and a record to write only; NULL from it: ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_overlap_records(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                                uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, const zngamd_bgzf_overlap_conf *conf,
                                uint64_t record_base, int32_t *status, zngamd_bgzf_overlap_row *overlap, uint64_t overlap_cap,
                                zngamd_bgzf_grep_row *rows, uint64_t rows_cap, uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc,
                                void *user, zngamd_bgzf_overlap_totals *totals);

/* ---- BGZF by region (zlib_ng_amd/bgzf.py: TabixIndex, fetch).  Both calls read the FIELDS of tab-separated
 * lines by the rules of tabix.  conf: format (0 generic, 2 VCF, | 0x10000: the coordinates are zero-based, half-open; 1, the SAM
 * preset, is ZNGAMD_E_ARG), the columns of the name, the start and the end (from 1; col_end 0: none), the byte that opens a comment
 * line, the lines at the top to skip.  A line ends with `delim`; one CR in front of it belongs to no field.  A line is skipped when
 * its number is below conf.skip, its first byte is conf.meta or it is empty.  The interval [beg, end), zero-based: generic, beg =
 * col_beg - 1 (with 0x10000: col_beg) and end = col_end, or beg + 1 without one; VCF, beg = POS - 1, end = beg + the length of
 * column 4, or the value of the first END= that opens column 8 or follows a ';' in it, if digits follow it up to ';' or the column's
 * end and it lies above beg; end <= beg becomes beg + 1.  A coordinate is 1 to 10 digits and nothing else.  A data line is bad,
 * checked in this order, when (1) a needed column is missing (VCF: 1, 2 and 4), (2) a coordinate is not digits, (3) beg < 0 or end >
 * 2^29, (4) its name equals the previous data line's and its beg is smaller.
 *
 * zngamd_bgzf_tabix: what an index of the text scratch[text_off, text_end) is made of.  Blocks, member table, text, delimiter,
 * _FINAL, line_base and the cover contract (covered = 0: nothing is reported) are those of zngamd_bgzf_grep.  Data lines are counted
 * from 0 in the order of the text (their ordinal).  Three tables come back:
 *   names  one row per maximal run of data lines with the same name: where the name stands in the scratch, its length, the ordinal
 *          and the line number of the run's first line; the names themselves packed in that order into `blob`
 *   bins   one row per maximal run of data lines with the same name and the same bin (reg2bin, SAM specification 5.3): the scratch
 *          offset of its first line and of the byte behind its last line, its name run, the bin, its first ordinal, its lines
 *   wins   one row per data line that raises the running maximum of (end - 1) >> 14 within its name run: name run, that window, the
 *          scratch offset of the line -- the windows between the previous row's and this one are first overlapped by this line
 * Skipped lines break no run.  The totals first: with a bad line (bad_kind 1 .. 4, bad_line the smallest such line number, bad_src its
 * scratch offset) the tables describe the data lines without those that are bad by (1) to (3): a caller that wants to know whether a
 * name came back earlier than the bad line still can; an index is not to be built from them.  ZNGAMD_BUF_ERROR: a capacity is below
 * its count; nothing is written.  *totals is always valid on ZNGAMD_OK and ZNGAMD_BUF_ERROR.  The tables are untrusted: no entry makes a kernel read or
 * write outside the buffers. */
typedef struct { int32_t format, col_seq, col_beg, col_end, meta, skip; } zngamd_tabix_conf;                  /* 24 B */
typedef struct { uint64_t src_off, first, line; uint32_t len, reserved; } zngamd_tabix_name;                  /* 32 B */
typedef struct { uint64_t src_beg, src_end, first, lines; uint32_t name, bin; } zngamd_tabix_bin;             /* 40 B */
typedef struct { uint64_t src_off; uint32_t name, window; } zngamd_tabix_win;                                 /* 16 B */
typedef struct {
    uint64_t seen;         /* lines of the text that were decided (the open tail is not one of them) */
    uint64_t data;         /* of them, data lines */
    uint64_t tail_off;     /* scratch offset where the open line starts; text_end when there is none */
    uint64_t bad_line;     /* bad_kind != 0: the smallest number of a bad line */
    uint64_t bad_src;      /*                where that line starts in the scratch */
    uint64_t n_names, name_bytes, n_bins, n_wins;      /* rows of the three tables, bytes of the packed names */
    uint64_t first_line;   /* data != 0: the number of the first data line, */
    uint64_t first_src;    /*            where it starts, */
    uint32_t first_beg;    /*            its beg, */
    uint32_t last_beg;     /*            and the last data line's (the caller compares across two calls) */
    uint32_t covered;      /* 1: decoded blocks cover the text and the figures above describe it */
    uint32_t bad_kind;     /* 0, or 1 .. 4 as numbered above */
} zngamd_bgzf_tabix_totals;                                                                                    /* 104 B */
#define ZNGAMD_BGZF_TABIX_FINAL      4u
#define ZNGAMD_TABIX_MAX_POS         536870912      /* 2^29: the largest end a .tbi can hold */
int zngamd_bgzf_tabix_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                          uint64_t text_off, uint64_t text_end, const zngamd_tabix_conf *conf, int delim, uint32_t flags,
                          uint64_t line_base, void *d_scratch, uint64_t scratch_cap, int32_t *d_status, zngamd_tabix_name *d_names,
                          uint64_t names_cap, void *d_blob, uint64_t blob_cap, zngamd_tabix_bin *d_bins, uint64_t bins_cap,
                          zngamd_tabix_win *d_wins, uint64_t wins_cap, zngamd_bgzf_tabix_totals *totals);
/* Host-buffer form: stages in and the member table; status and the tables come back.  A caller that cannot bound the tables passes
 * NULL pointers, the capacities 0 and alloc: once the sizes are known it is asked for names, blob, bins and wins in this order; it is
 * not asked for an empty one; NULL from it: ZNGAMD_MEM_ERROR. */
int zngamd_bgzf_tabix(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                      uint64_t text_off, uint64_t text_end, const zngamd_tabix_conf *conf, int delim, uint32_t flags,
                      uint64_t line_base, int32_t *status, zngamd_tabix_name *names, uint64_t names_cap, uint8_t *blob,
                      uint64_t blob_cap, zngamd_tabix_bin *bins, uint64_t bins_cap, zngamd_tabix_win *wins, uint64_t wins_cap,
                      zngamd_alloc_fn alloc, void *user, zngamd_bgzf_tabix_totals *totals);
/* zngamd_bgzf_fetch: the lines of a region.  The blocks a plan needs and their member rows as zngamd_bgzf_read takes them, decoded
 * once in one launch.  regions (host memory in both forms): 1 .. ZNGAMD_BGZF_FETCH_MAX_REGIONS rows {name_off, name_len, beg, end}
 * into `names` (names_len bytes); anything else is ZNGAMD_E_ARG, found before anything is launched.  spans: rows {text_off, text_end,
 * region} of the scratch; a span begins where a line begins and ends behind a delimiter or at the end of the decoded text (the bytes
 * behind its last delimiter are a line); spans of different regions may overlap.  span_status[s]: ZNGAMD_BGZF_SLICE_OK; _TABLE (the
 * span lies outside the scratch, is 4 GiB or longer or names no region); _BLOCK (blocks that decoded do not cover it): such a span
 * selects nothing.  span_rows[s]: the lines span s selects.  A data line is selected when its name equals the region's, beg <
 * region.end and end > region.beg; bad and skipped lines are never selected and are no error.  rows: {src_off, len, region} of the
 * selected lines in span order, then in the order of the text; the lines packed in that order into out.  Totals, ZNGAMD_BUF_ERROR and
 * alloc (rows, then lines) as for zngamd_bgzf_grep; _COUNT_ONLY: the totals, span_status and span_rows alone. */
typedef struct { uint32_t name_off, name_len, beg, end; } zngamd_tabix_region;                                 /* 16 B */
typedef struct { uint64_t text_off, text_end; uint32_t region, reserved; } zngamd_tabix_span;                 /* 24 B */
typedef struct { uint64_t src_off; uint32_t len, region; } zngamd_tabix_row;                                  /* 16 B */
typedef struct { uint64_t matched, bytes; } zngamd_bgzf_fetch_totals;                                         /* 16 B */
#define ZNGAMD_BGZF_FETCH_COUNT_ONLY  8u
#define ZNGAMD_BGZF_FETCH_MAX_REGIONS 4096u
int zngamd_bgzf_fetch_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                          const zngamd_tabix_conf *conf, int delim, uint32_t flags, const uint8_t *names, uint32_t names_len,
                          const zngamd_tabix_region *regions, uint32_t n_regions, const zngamd_tabix_span *d_spans, uint32_t n_spans,
                          void *d_scratch, uint64_t scratch_cap, int32_t *d_status, int32_t *d_span_status, uint32_t *d_span_rows,
                          zngamd_tabix_row *d_rows, uint64_t rows_cap, void *d_out, uint64_t out_cap, zngamd_bgzf_fetch_totals *totals);
int zngamd_bgzf_fetch(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                      const zngamd_tabix_conf *conf, int delim, uint32_t flags, const uint8_t *names, uint32_t names_len,
                      const zngamd_tabix_region *regions, uint32_t n_regions, const zngamd_tabix_span *spans, uint32_t n_spans,
                      int32_t *status, int32_t *span_status, uint32_t *span_rows, zngamd_tabix_row *rows, uint64_t rows_cap,
                      uint8_t *out, uint64_t out_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_fetch_totals *totals);

/* ---- BGZF by sequence (zlib_ng_amd/bgzf.py: FaidxIndex, fetch_seq).  Both calls read a FASTA.
 * The line model.  The text is cut into lines by '\n' (delim must be 10; anything else, and flags other than _FINAL, is ZNGAMD_E_ARG,
 * found before the context is touched).  One CR directly in front of the '\n' belongs to the terminator.  A line's bases are the bytes
 * of its body, without the terminator; its width is the body plus the terminator bytes.  With _FINAL, non-empty bytes behind the last
 * '\n' are a line whose width equals its bases.  A line whose first byte is '>' is a header: its name runs from the byte behind '>'
 * to the first space, tab or CR, or to the end of the body, and it opens a sequence.  Every other line is a sequence line of the open
 * sequence; one with 0 bases is empty.  Per sequence: bases, the sum of the bases of its lines; seq_src, the first byte behind the
 * header line (also when no sequence line follows); line_bases and line_width, those of its first non-empty line, or 0 and 0.
 * A line is bad, smallest kind first, when (1) it is a header with an empty name, (2) a sequence line with a byte outside 0x21 ..
 * 0x7E in its body, (3) a non-empty sequence line that is not the last non-empty line of its sequence and whose bases or width
 * differ from the first one's, or the last non-empty line with more bases than the first (its width is free), (4) an empty line that
 * a non-empty line follows inside the same sequence, (5) a non-empty sequence line while no sequence is open (empty lines in front
 * of the first header are skipped).  Of several faults the smallest line number is reported, and of one line's the smallest kind.
 *
 * zngamd_bgzf_faidx: the records of the text scratch[text_off, text_end).  Blocks, member table, text, _FINAL, line_base, tail_off
 * and the cover contract (covered = 0: nothing is reported, the carry comes back as it went in) are those of zngamd_bgzf_tabix.
 * carry (NULL: nothing is open) describes the sequence that is open at text_off: its first non-empty line (first_width 0: none yet),
 * its last non-empty line so far and that line's number (without one: 0, 0 and the header's number), flags ZNGAMD_FAIDX_OPEN and
 * ZNGAMD_FAIDX_GAP (an empty line follows last_line).  With it every line of the text is judged by the rules above, the lines in
 * front of the text's first header too; head_bases is the sum of their bases, to be added to the open sequence by the caller.  One
 * judgement waits for the next call, whether the text's last non-empty line is a middle line or its sequence's last: a call that
 * meets a non-empty line in front of its first header applies (3) to carry.last_line as a middle line and (4) to last_line + 1 with
 * _GAP; one that meets a header, or has _FINAL, applies (3) as to a last line.  A bad line in front of line_base has bad_src ~0;
 * carry.reserved of the carry that comes back says where it starts: the scratch offset, from text_off, of the line behind last_line,
 * valid while last_line >= line_base (bad_line == last_line starts last_width bytes in front of it).  totals.carry is what the next
 * call takes; with _FINAL it is zero.  rows: one per header line, in text order: where the name stands and its length, seq_src, the
 * header's line number, and bases, line_bases, line_width as far as this text shows them (the record the text ends in is continued
 * by the next call's head); the names packed in that order into blob.  Nothing per line leaves the device.  ZNGAMD_BUF_ERROR: a
 * capacity is below its count; nothing is written.  *totals is always valid on ZNGAMD_OK and ZNGAMD_BUF_ERROR.  The member table is
 * untrusted: no entry makes a kernel read or write outside the buffers. */
typedef struct { uint64_t last_line; uint32_t first_bases, first_width, last_bases, last_width, flags, reserved; } zngamd_faidx_carry;   /* 32 B */
typedef struct { uint64_t name_src, seq_src, line, bases; uint32_t name_len, line_bases, line_width, reserved; } zngamd_faidx_row;       /* 48 B */
typedef struct {
    uint64_t seen;         /* lines of the text that were decided (the open tail is not one of them) */
    uint64_t records;      /* of them, headers: the rows */
    uint64_t tail_off;     /* scratch offset where the open line starts; text_end when there is none */
    uint64_t head_bases;   /* bases of the lines in front of the text's first header when the carry that came in is open */
    uint64_t name_bytes;   /* bytes of the packed names */
    uint64_t bad_line;     /* bad_kind != 0: the smallest number of a bad line */
    uint64_t bad_src;      /*                where that line starts in the scratch; ~0 for a line in front of line_base */
    uint32_t covered;      /* 1: decoded blocks cover the text and the figures above describe it */
    uint32_t bad_kind;     /* 0, or 1 .. 5 as numbered above */
    zngamd_faidx_carry carry;
    uint32_t head_line_bases, head_line_width;      /* the first non-empty line in front of the text's first header when the carry that
                                                       came in is open and has none: the open sequence's line_bases and line_width */
} zngamd_bgzf_faidx_totals;                                                                                    /* 104 B */
#define ZNGAMD_BGZF_FAIDX_FINAL 4u
#define ZNGAMD_FAIDX_OPEN       1u
#define ZNGAMD_FAIDX_GAP        2u
int zngamd_bgzf_faidx_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                          uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, uint64_t line_base,
                          const zngamd_faidx_carry *carry, void *d_scratch, uint64_t scratch_cap, int32_t *d_status,
                          zngamd_faidx_row *d_rows, uint64_t rows_cap, void *d_blob, uint64_t blob_cap, zngamd_bgzf_faidx_totals *totals);
/* Host-buffer form: stages in and the member table; status, rows and names come back.  alloc as for zngamd_bgzf_tabix: rows, then
 * blob; it is not asked for an empty one. */
int zngamd_bgzf_faidx(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                      uint64_t text_off, uint64_t text_end, int delim, uint32_t flags, uint64_t line_base,
                      const zngamd_faidx_carry *carry, int32_t *status, zngamd_faidx_row *rows, uint64_t rows_cap, uint8_t *blob,
                      uint64_t blob_cap, zngamd_alloc_fn alloc, void *user, zngamd_bgzf_faidx_totals *totals);
/* zngamd_bgzf_faidx_fetch: bases without their line terminators.  Blocks and member rows as zngamd_bgzf_read takes them, decoded
 * once in one launch; then one workgroup per span.  src_off: the scratch offset of the span's first base; col: that base's position
 * in its line; n: bases, at most ZNGAMD_FAIDX_MAX_SPAN.  Base k, with q = col + k, comes from src_off - col + (q / line_bases) *
 * line_width + q % line_bases and goes to dst_off + k; with ZNGAMD_FAIDX_SPAN_RC to dst_off + n - 1 - k, complemented (A<->T, C<->G,
 * U->A, R<->Y, K<->M, B<->V, D<->H, in both letter cases; everything else unchanged).  span_status[s]: ZNGAMD_BGZF_SLICE_OK; _TABLE
 * (the span lies outside scratch_cap or out_cap, line_bases == 0, line_width < line_bases, col >= line_bases, src_off < col or n >
 * 65 536: nothing is written); _BLOCK (blocks that decoded do not cover its bytes: zeros are written); _STALE (a gathered byte lies
 * outside 0x21 .. 0x7E: the index belongs to another file).  The spans are untrusted as the member table is. */
typedef struct { uint64_t src_off, dst_off; uint32_t n, col, line_bases, line_width, flags, reserved; } zngamd_faidx_span;   /* 40 B */
#define ZNGAMD_BGZF_SLICE_STALE 4
#define ZNGAMD_FAIDX_SPAN_RC    1u
#define ZNGAMD_FAIDX_MAX_SPAN   65536u
int zngamd_bgzf_faidx_fetch_dev(zngamd_ctx *ctx, const void *d_in, uint64_t in_len, const zngamd_member *d_members, uint32_t n_members,
                                const zngamd_faidx_span *d_spans, uint32_t n_spans, void *d_scratch, uint64_t scratch_cap, void *d_out,
                                uint64_t out_cap, int32_t *d_status, int32_t *d_span_status);
int zngamd_bgzf_faidx_fetch(zngamd_ctx *ctx, const uint8_t *in, uint64_t in_len, const zngamd_member *members, uint32_t n_members,
                            const zngamd_faidx_span *spans, uint32_t n_spans, uint8_t *out, uint64_t out_cap, int32_t *status,
                            int32_t *span_status);

/* ---- streaming: the zng_stream calling convention ------------------------------------------------
 * What a binding of the reference swaps in for zng_deflateInit2 / zng_deflate / zng_deflateSetDictionary / zng_deflateCopy /
 * zng_deflateEnd (zlib_ngmodule.c:394, :552, :743, :401, :811) and zng_inflateInit2 / zng_inflate / zng_inflateSetDictionary /
 * zng_inflateCopy / zng_inflateEnd (:477, :667, :995, :1150, :446, :893): same fields, same flush values (Z_FULL_FLUSH forgets the history: nothing behind
 * the flush point refers to anything in front of it), same return codes
 * (ZNGAMD_OK 0, ZNGAMD_STREAM_END 1, ZNGAMD_NEED_DICT 2, ZNGAMD_STREAM_ERROR -2, ZNGAMD_DATA_ERROR -3, ZNGAMD_MEM_ERROR -4,
 * ZNGAMD_BUF_ERROR -5), `msg` set where zng_inflate sets it ("incorrect header check", "invalid window size", "incorrect data
 * check", ...).  deflate collects input until a flush or 32 MiB and compresses it as one dictionary-chained engine batch
 * (a piece of 32 MiB or more handed in at once is compressed where it lies); inflate keeps the compressed bytes from the last
 * block header on, decodes from there (bit offset + 32 KiB of history) and hands out what is new; input the stream does not
 * need yet comes back through avail_in, as with zng_inflate. */
typedef struct zngamd_stream_state zngamd_stream_state;
typedef struct zngamd_stream {
    const uint8_t *next_in;   /* next input byte */
    uint32_t avail_in;        /* bytes available at next_in */
    uint64_t total_in;
    uint8_t *next_out;        /* next output byte goes here */
    uint32_t avail_out;       /* room at next_out */
    uint64_t total_out;
    const char *msg;          /* last error message, NULL if none */
    zngamd_stream_state *state;
    uint32_t adler;           /* Adler-32 (zlib) or CRC-32 (gzip) of the uncompressed data so far; DICTID after ZNGAMD_NEED_DICT */
    uint32_t reserved;
    /* zng_stream's allocator hooks, which the reference sets (zlib_ngmodule.c:210-212, :391-393, :474-476): accepted and never
     * called -- the engine's memory is device memory and its own host buffers; a binding keeps those three lines as they are */
    void *zalloc, *zfree, *opaque;
} zngamd_stream;
#define ZNGAMD_NO_FLUSH 0
#define ZNGAMD_PARTIAL_FLUSH 1
#define ZNGAMD_SYNC_FLUSH 2
#define ZNGAMD_FULL_FLUSH 3
#define ZNGAMD_FINISH 4
#define ZNGAMD_BLOCK 5
int zngamd_stream_deflate_init(zngamd_ctx *ctx, zngamd_stream *strm, int level, int method, int wbits, int mem_level, int strategy);
int zngamd_stream_deflate(zngamd_stream *strm, int flush);
int zngamd_stream_deflate_set_dictionary(zngamd_stream *strm, const uint8_t *dict, uint32_t len);
int zngamd_stream_deflate_copy(zngamd_stream *dst, const zngamd_stream *src);
/* output produced and not yet handed out (zng_deflatePending; also valid for an inflate stream): lets the caller size its buffer once */
int zngamd_stream_pending(const zngamd_stream *strm, uint64_t *pending);
/* zng_deflateReset (zlib_ngmodule.c:1725): the stream as deflate_init left it -- same level, container and window */
int zngamd_stream_deflate_reset(zngamd_stream *strm);
int zngamd_stream_deflate_end(zngamd_stream *strm);
int zngamd_stream_inflate_init(zngamd_ctx *ctx, zngamd_stream *strm, int wbits);
int zngamd_stream_inflate(zngamd_stream *strm, int flush);
int zngamd_stream_inflate_set_dictionary(zngamd_stream *strm, const uint8_t *dict, uint32_t len);
/* A caller that grows its output buffer (arrange_output_buffer, zlib_ngmodule.c:142-197) announces how much output it will take
 * in total over the next calls (its max_length; UINT64_MAX = as much as the input yields): the engine then decodes that far in one
 * batch and hands the bytes out as buffers arrive (zngamd_stream_pending says how many wait), instead of decoding the current
 * block again for every doubling of a 16 KiB buffer.  0 (the default) = strictly avail_out, as zng_inflate. */
int zngamd_stream_inflate_ahead(zngamd_stream *strm, uint64_t bytes);
int zngamd_stream_inflate_copy(zngamd_stream *dst, const zngamd_stream *src);
/* zng_inflateReset (zlib_ngmodule.c:2525, :2715): the stream as inflate_init left it; the next input byte starts a new stream */
int zngamd_stream_inflate_reset(zngamd_stream *strm);
int zngamd_stream_inflate_end(zngamd_stream *strm);

/* ---- multi-GPU exchange: RCCL over xGMI, one process per GPU (gzip_ng_threaded.py:233-246 gives every worker thread a
 * compressor, :316-321 deals the blocks round-robin, :382-398 drains them in order; here every rank owns a contiguous block
 * range and the ranks reassemble the member stream with ONE exchange step) -------------------------------------------------
 * librccl is loaded on the first call (dlopen), so the library itself does not depend on it.  The 128-byte unique id is made
 * on one rank and handed to the others by the launcher's own means (bench.py: a TCP socket on MASTER_ADDR). */
typedef struct zngamd_comm zngamd_comm;
#define ZNGAMD_COMM_ID_BYTES 128
int zngamd_comm_unique_id(uint8_t id[ZNGAMD_COMM_ID_BYTES]);
/* collective over all ranks: communicator bound to ctx's device, with a stream of its own (exchanges overlap ctx's kernels) */
int zngamd_comm_create(zngamd_ctx *ctx, const uint8_t id[ZNGAMD_COMM_ID_BYTES], int rank, int world, zngamd_comm **out);
void zngamd_comm_destroy(zngamd_comm *comm);
const char *zngamd_comm_last_error(zngamd_comm *comm);
/* number of ranks the communicator really has, as RCCL reports it (ncclCommCount) -- not what the launcher's environment claims */
int zngamd_comm_count(zngamd_comm *comm, int *ranks);
/* layout of the one output stream: all-gather of {compressed bytes, CRC-32 of the rank's input, input bytes} (24 bytes per
 * rank), then on every rank: sizes[world], the offset of the own slice, the total, the CRC-32 of the whole input folded with
 * crc32_combine in rank order, and the whole input length -- what header / trailer and a positional write need */
int zngamd_comm_layout(zngamd_comm *comm, uint64_t local_len, uint32_t local_crc, uint64_t local_ulen, uint64_t *sizes,
                       uint64_t *my_off, uint64_t *total, uint32_t *whole_crc, uint64_t *whole_ulen);
/* exact-size exchange of the slices (no padding): every rank sends d_local[0 .. sizes[rank]) to every other rank and
 * receives their slices at their offsets, grouped ncclSend / ncclRecv over all links at once; afterwards d_stream holds the
 * whole stream on every rank.  Starts behind the work queued on ctx's stream so far and returns at once;
 * zngamd_comm_wait blocks until the exchange is done. */
int zngamd_comm_allgather_stream(zngamd_comm *comm, const void *d_local, const uint64_t *sizes, void *d_stream, uint64_t stream_cap);
/* where the slices lie in the assembled stream: offs[r] = sizes[0] + ... + sizes[r-1]; returns the total (pure arithmetic, no GPU:
 * the placement rule of the exchange above and of a positional write, testable on its own) */
uint64_t zngamd_comm_offsets(const uint64_t *sizes, int world, uint64_t *offs);
int zngamd_comm_wait(zngamd_comm *comm);
/* plumbing for a driver: barrier, and the maximum of one double over the ranks (step time of the slowest rank) */
int zngamd_comm_barrier(zngamd_comm *comm);
int zngamd_comm_max_f64(zngamd_comm *comm, double *value);

/* ---- measurement ---- */
/* With profiling on, every kernel launch is bracketed by HIP events on the context's stream. */
#define ZNGAMD_K_CHAINS 0
#define ZNGAMD_K_SEARCH 1
#define ZNGAMD_K_PARSE  2
#define ZNGAMD_K_PLAN   3
#define ZNGAMD_K_PACK   4
#define ZNGAMD_K_GATHER 5
#define ZNGAMD_K_SCAN   6
#define ZNGAMD_K_INFLATE 7
#define ZNGAMD_K_OTHER  8
#define ZNGAMD_K_OPTPARSE 9     /* the dynamic programme between search and parse (levels 4-9) */
#define ZNGAMD_K_COUNT  10
int zngamd_profiling(zngamd_ctx *ctx, int on);
/* accumulated milliseconds and launch counts per kernel class since the last reset.  The library writes
 * zngamd_kernel_class_count() elements into each array: a caller built against an older header (ZNGAMD_K_COUNT was 9 before the
 * dynamic programme's class) asks the library, not its own header, how much room to give -- or compares ZNGAMD_ABI with
 * zngamd_abi() once. */
int zngamd_kernel_times(zngamd_ctx *ctx, double *ms /*[ZNGAMD_K_COUNT]*/, uint64_t *launches /*[ZNGAMD_K_COUNT]*/, int reset);
int zngamd_kernel_class_count(void);
#define ZNGAMD_ABI 6            /* bumped whenever an array size, a struct layout or an argument list of this header changes */
int zngamd_abi(void);

/* how many gzip members zngamd_gunzip (and whole streams zngamd_inflate_raw) decoded through each path since the last reset:
 * ZA-indexed two-pass, BGZF one-launch, chunk-parallel (sync points / block finder), one sequential wavefront */
#define ZNGAMD_PATH_INDEXED    0
#define ZNGAMD_PATH_BGZF       1
#define ZNGAMD_PATH_CHUNKED    2
#define ZNGAMD_PATH_SEQUENTIAL 3
#define ZNGAMD_PATH_COUNT      4
int zngamd_decode_paths(zngamd_ctx *ctx, uint64_t *members /*[ZNGAMD_PATH_COUNT]*/, int reset);
/* units decoded with a writer's segment index (zngamd_inflate_units_indexed_dev, or the windowed reader with zngamd_gz_state.index);
 * a batch the index was refused for is not counted */
uint64_t zngamd_indexed_units(zngamd_ctx *ctx, int reset);

/* ---- debugging aid for the parity tests: copy a stage's intermediate of unit `u` of the last
 * deflate call to the host.  what: 0 links of table A (u16) 1 best(u32, as the parse kernel read it: behind the dynamic
 * programme on levels 4-9) 2 tokens(u32) 3 seg_ntok(u32) 4 hist(u32) 5 codes(u32) 6 seg_bits(u32) 7 plan(4 x u32)
 * 8 chunk index(u32) 9 / 10 links of tables B / C (u16) 11 best as the search left it (u32) 12 the dynamic programme's cost
 * table (258 x u32, levels 4-9).  Forms: stages 1 and 11 come back as length << 16 | distance, 0 = no match (the kernels keep
 * distance - 1 | length << 15 | the position's byte << 24; zngamd_debug_fetch converts and drops the byte); stage 2 is the
 * kernels' own token word (a match: bit 31 | length code << 26 | length extra << 21 | distance code << 16 | distance extra; else
 * one to three literals in bits 0..23, their number - 1 in bits 24..25); every other stage is the kernels' own array.  Under
 * Z_FIXED stage 12 holds the ESTIMATED table: the programme puts the fixed code's costs over it when it loads it.
 * Stages 0, 9, 10 and 11 exist only for calls made after zngamd_debug_keep(ctx, 1): without it the
 * token words are written over the link tables (a third of the workspace saved), and nothing copies the search results aside. */
int zngamd_debug_keep(zngamd_ctx *ctx, int on);
int zngamd_debug_fetch(zngamd_ctx *ctx, int what, uint32_t unit, void *host_dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif

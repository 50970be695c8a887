"""Throughput and ratio per compression strategy at levels 1, 6 and 9.

    python profiles/time_strategies.py            # SIZE_MIB (4096) of corpus.text device resident, COBJ_MIB (256) through compressobj

(1) device resident: zngamd_deflate_blocks_packed_dev over SIZE_MIB of corpus.text (a 256 MiB tile repeated), blocks of 128 KiB
    primed by the 32 KiB in front, the strategy on the blocks (ZNGAMD_FLAG_STRATEGY); one warm-up call, then the best of REPS.
(2) zlib_ng.compressobj(level, DEFLATED, 15, 8, strategy) over COBJ_MIB of corpus.text: one call to compress + flush, after a warm-up.
Every stream of (2) is checked with the system zlib."""
import ctypes as C
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
from zlib_ng_amd import _lib, corpus, devmem, zlib_ng  # noqa: E402

NAMES = ["default", "filtered", "huffman", "rle", "fixed"]
SIZE = int(os.environ.get("SIZE_MIB", "4096")) << 20
COBJ = int(os.environ.get("COBJ_MIB", "256")) << 20
REPS = int(os.environ.get("REPS", "3"))
B, HALO = 131072, 32768


def main():
    ctx = _lib.default_context()
    L, h = ctx.L, ctx.h
    tile_n = min(SIZE, 256 << 20)
    tile = corpus.text(tile_n, seed=1)
    d_tile = devmem.from_host(ctx, tile)
    d_buf = devmem.empty(ctx, HALO + SIZE + 64)
    pos = 0
    while pos < HALO + SIZE:
        k = min(tile_n, HALO + SIZE - pos)
        d_buf[pos:pos + k] = d_tile[0:k]
        pos += k
    d_buf[HALO + SIZE:] = 0
    d_tile.free()
    nb = SIZE // B
    d_out = devmem.empty(ctx, SIZE + SIZE // 8 + (64 << 20))
    d_len, d_crc = devmem.empty(ctx, 4 * nb), devmem.empty(ctx, 4 * nb)
    ctx.sync()
    print("device resident: %d MiB of corpus.text, %d blocks of 128 KiB" % (SIZE >> 20, nb), flush=True)
    for level in (1, 6, 9):
        for s, name in enumerate(NAMES):
            blocks = (_lib.Block * nb)()
            for b in range(nb):
                blocks[b] = _lib.Block(HALO + b * B, B, 32768, _lib.flag_strategy(s), 0)
            total = C.c_uint64(0)
            best = None
            for rep in range(REPS + 1):
                ctx.sync()
                t0 = time.perf_counter()
                r = L.zngamd_deflate_blocks_packed_dev(h, d_buf.vp(), HALO + SIZE, blocks, nb, level, d_out.vp(), d_out.numel() - 64,
                                                       d_len.vp(), d_crc.vp(), None, C.byref(total))
                ctx.sync()
                dt = time.perf_counter() - t0
                if r != 0:
                    raise RuntimeError("deflate_blocks_packed_dev: %d %s" % (r, ctx.err()))
                if rep:
                    best = dt if best is None else min(best, dt)
            print("  level %d %-9s %8.1f GB/s  ratio %6.3f  (%.2f ms)" % (level, name, SIZE / best / 1e9, SIZE / total.value, best * 1e3), flush=True)
    for d in (d_buf, d_out, d_len, d_crc):
        d.free()
    data = corpus.text(COBJ, seed=3).tobytes()
    print("compressobj: %d MiB of corpus.text (wbits 15)" % (COBJ >> 20), flush=True)
    for level in (1, 6, 9):
        for s, name in enumerate(NAMES):
            c = zlib_ng.compressobj(level, zlib_ng.DEFLATED, 15, 8, s)
            c.compress(data[:1 << 20]); c.flush()
            t0 = time.perf_counter()
            c = zlib_ng.compressobj(level, zlib_ng.DEFLATED, 15, 8, s)
            out = c.compress(data) + c.flush()
            dt = time.perf_counter() - t0
            assert zlib.decompress(out) == data
            print("  level %d %-9s %8.2f GB/s  ratio %6.3f  (%.1f ms)" % (level, name, COBJ / dt / 1e9, COBJ / len(out), dt * 1e3), flush=True)


if __name__ == "__main__":
    main()

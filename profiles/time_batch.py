"""Batch API timings: item sizes 1 KiB, 4 KiB, 64 KiB x 1 000, 10 000, 100 000 items (at most ~2 GiB of input per
cell), levels 1 and 6, zlib container.  Records are cut from corpus.text(), corpus.fastq() and the FASTQ fixture under tests/golden.

Columns per direction:
  batch host   batch.compress / batch.decompress wall time (Python lists in and out)
  batch dev    batch.compress_dev / decompress_dev wall time with input and output in device memory
  kernels      sum of the engine's own kernel timers (hipEvent pairs) for one batch.compress / decompress call
  one-shot     zlib_ng.compress / decompress in a loop, timed on a sample of 500 items and scaled to the cell
  zlib 1t      CPython zlib in a loop, timed on a sample of 2 000 items and scaled
  zlib 16t     CPython zlib on 16 threads (it releases the GIL), timed on a sample of 16 000 items and scaled

    python profiles/time_batch.py [--quick]
"""
import gzip
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
from zlib_ng_amd import _lib, batch, corpus, devmem, zlib_ng  # noqa: E402

CAP = 2 << 30


def records(size, n):
    """n records of `size` bytes cut from the three sources in turn"""
    pool_len = min(size * n, 96 << 20)
    fixture = gzip.open(os.path.join(ROOT, "tests", "golden", "test.fastq.gz")).read()
    pools = [corpus.text(pool_len // 3 + size, seed=1).tobytes(), corpus.fastq(pool_len // 3 + size, seed=2).tobytes(),
             (fixture * (pool_len // 3 // len(fixture) + 2))[:pool_len // 3 + size]]
    out = []
    for i in range(n):
        p = pools[i % 3]
        o = (i // 3 * size * 7919) % (len(p) - size)
        out.append(p[o:o + size])
    return out


def best(f, reps=2):
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); r = f(); ts.append(time.perf_counter() - t)
    return min(ts), r


def sampled(f, items, k):
    s = items[:k]
    t = time.perf_counter()
    for x in s:
        f(x)
    return (time.perf_counter() - t) / len(s) * len(items)


def threaded(f, items, k, threads=16):
    s = items[:k]
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(f, s[:threads]))
        t = time.perf_counter()
        list(ex.map(f, s, chunksize=64))
        return (time.perf_counter() - t) / len(s) * len(items)


def kernels(ctx, f):
    ctx.profiling(True); ctx.kernel_times(True)
    f()
    k = ctx.kernel_times(True); ctx.profiling(False)
    return sum(v[0] for v in k.values()) / 1e3      # ms -> s


def main():
    quick = "--quick" in sys.argv
    ctx = _lib.default_context()
    sizes = (1 << 10, 4 << 10, 64 << 10)
    counts = (1000, 10000) if quick else (1000, 10000, 100000)
    print("time_batch: zlib container; times in ms for the whole cell; one-shot / zlib columns scaled from samples (see the header)")
    print(f"{'size':>6} {'items':>7} {'lvl':>3} {'dir':>4} | {'batch host':>10} {'batch dev':>10} {'kernels':>8} | {'one-shot':>9} {'zlib 1t':>9} {'zlib 16t':>9} | {'MB/s host':>9} {'x one-shot':>10} {'x zlib1t':>8} {'x zlib16t':>9}")
    for size in sizes:
        for n in counts:
            n = min(n, CAP // size)
            items = records(size, n)
            raw = size * n
            lens = np.full(n, size, dtype=np.uint64)
            offs = np.arange(n, dtype=np.uint64) * np.uint64(size)
            d_in = devmem.from_host(ctx, np.frombuffer(b"".join(items) + bytes(64), np.uint8))
            for level in (1, 6):
                batch.compress(items[:64], level)
                th, comp = best(lambda: batch.compress(items, level))
                td, _ = best(lambda: batch.compress_dev(ctx, d_in, offs, lens, level))
                tk = kernels(ctx, lambda: batch.compress(items, level))
                to = sampled(lambda x: zlib_ng.compress(x, level), items, 500)
                tz = sampled(lambda x: zlib.compress(x, level), items, 2000)
                tz16 = threaded(lambda x: zlib.compress(x, level), items, 16000)
                print(f"{size:6d} {n:7d} {level:3d} {'c':>4} | {th*1e3:10.1f} {td*1e3:10.1f} {tk*1e3:8.1f} | {to*1e3:9.0f} {tz*1e3:9.0f} {tz16*1e3:9.0f} | "
                      f"{raw/th/1e6:9.0f} {to/th:10.1f} {tz/th:8.1f} {tz16/th:9.2f}", flush=True)
                clens = np.array([len(c) for c in comp], dtype=np.uint64)
                coffs = np.zeros(n, dtype=np.uint64); coffs[1:] = np.cumsum(clens)[:-1]
                d_c = devmem.from_host(ctx, np.frombuffer(b"".join(comp) + bytes(64), np.uint8))
                batch.decompress(comp[:64])
                th, outs = best(lambda: batch.decompress(comp))
                assert outs[:7] == items[:7]
                td, _ = best(lambda: batch.decompress_dev(ctx, d_c, coffs, clens))
                tk = kernels(ctx, lambda: batch.decompress(comp))
                to = sampled(zlib_ng.decompress, comp, 500)
                tz = sampled(zlib.decompress, comp, 2000)
                tz16 = threaded(zlib.decompress, comp, 16000)
                print(f"{size:6d} {n:7d} {level:3d} {'d':>4} | {th*1e3:10.1f} {td*1e3:10.1f} {tk*1e3:8.1f} | {to*1e3:9.0f} {tz*1e3:9.0f} {tz16*1e3:9.0f} | "
                      f"{raw/th/1e6:9.0f} {to/th:10.1f} {tz/th:8.1f} {tz16/th:9.2f}", flush=True)
                del d_c, comp, outs
            del d_in, items


if __name__ == "__main__":
    main()

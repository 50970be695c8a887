"""Batch API with a shared preset dictionary: 10 000 x 4 KiB and 100 000 x 1 KiB records of JSON lines and of
Python sources, level 6, zlib container, a 32 KiB dictionary cut from records outside the batch.

Columns per direction (times in ms for the whole cell):
  host / host+d    batch.compress / batch.decompress without / with zdict (Python lists in and out)
  dev / dev+d      batch.compress_dev / decompress_dev without / with zdict (input and output in device memory)
  zlib 1t          CPython zlib compressobj(zdict) / decompressobj(zdict) in a loop, timed on 2 000 items and scaled
  zlib 16t         the same on 16 threads (zlib releases the GIL), timed on 16 000 items and scaled
  ratio / ratio+d  input / output bytes of the batch without / with the dictionary

    python profiles/time_batch_zdict.py            # the table
    python profiles/time_batch_zdict.py --trace    # one call of each batch form per cell, for rocprofv3 --kernel-trace --stats
"""
import json
import os
import random
import sys
import sysconfig
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
from zlib_ng_amd import _lib, batch, devmem  # noqa: E402

DICT = 32768


def json_lines(n_bytes, seed):
    rng = random.Random(seed)
    users = [f"user{rng.randrange(10 ** 6):06d}" for _ in range(300)]
    paths = ["/api/v1/items", "/api/v1/orders", "/login", "/static/app.js", "/api/v2/search", "/health", "/cart"]
    agents = ["Mozilla/5.0 (X11; Linux x86_64)", "curl/8.4.0", "python-requests/2.31", "Mozilla/5.0 (Macintosh; Intel Mac OS X 14_1)"]
    out, size = [], 0
    while size < n_bytes:
        rec = {"ts": 1_700_000_000 + rng.randrange(10 ** 7), "level": rng.choice(["INFO", "INFO", "INFO", "WARN", "ERROR"]),
               "user": rng.choice(users), "method": rng.choice(["GET", "GET", "POST", "PUT"]), "path": rng.choice(paths),
               "status": rng.choice([200, 200, 200, 201, 304, 404, 500]), "ms": round(rng.expovariate(1 / 40), 2),
               "agent": rng.choice(agents), "region": rng.choice(["eu-west-1", "us-east-1", "ap-south-1"])}
        line = json.dumps(rec).encode() + b"\n"
        out.append(line)
        size += len(line)
    return b"".join(out)


def python_sources(n_bytes):
    """the interpreter's own library sources, in a fixed order"""
    lib = sysconfig.get_paths()["stdlib"]
    out, size = [], 0
    for dp, dn, fn in sorted(os.walk(lib)):
        dn.sort()
        if "site-packages" in dp or "test" in dp.split(os.sep):
            continue
        for f in sorted(fn):
            if f.endswith(".py"):
                b = open(os.path.join(dp, f), "rb").read()
                out.append(b)
                size += len(b)
                if size >= n_bytes:
                    return b"".join(out)
    return b"".join(out)


def cell(source, size, n):
    """-> (dictionary, records): the dictionary is the first 32 KiB, the records are cut from what follows it"""
    data = json_lines(size * n + (1 << 20), seed=7) if source == "json" else python_sources(size * n + (1 << 20))
    d, body = data[:DICT], data[DICT + 4096:]
    body = (body * (size * n // max(1, len(body)) + 1))[:size * n]
    return d, [body[i * size:(i + 1) * size] for i in range(n)]


def best(f, reps=3):
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


def zc(d):
    def f(x):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, d)
        return c.compress(x) + c.flush()
    return f


def zd(d):
    def f(x):
        return zlib.decompressobj(15, zdict=d).decompress(x)
    return f


def main():
    trace = "--trace" in sys.argv
    ctx = _lib.default_context()
    print("time_batch_zdict: level 6, zlib, 32 KiB dictionary; ms for the whole cell; zlib columns scaled from samples (see the header)")
    print(f"{'source':>6} {'size':>5} {'items':>6} {'dir':>3} | {'host':>7} {'host+d':>7} {'dev':>7} {'dev+d':>7} | {'zlib 1t':>8} {'zlib 16t':>8} | "
          f"{'ratio':>5} {'ratio+d':>7}")
    for source in ("json", "py"):
        for size, n in ((4096, 10000), (1024, 100000)):
            d, items = cell(source, size, n)
            raw = size * n
            lens = np.full(n, size, dtype=np.uint64)
            offs = np.arange(n, dtype=np.uint64) * np.uint64(size)
            d_in = devmem.from_host(ctx, np.frombuffer(b"".join(items) + bytes(64), np.uint8))
            if trace:
                c0 = batch.compress(items, 6)
                c1 = batch.compress(items, 6, zdict=d)
                batch.compress_dev(ctx, d_in, offs, lens, 6, zdict=d)
                batch.decompress(c0)
                batch.decompress(c1, zdict=d)
                print(f"{source} {size} {n}: traced", flush=True)
                continue
            batch.compress(items[:64], 6); batch.compress(items[:64], 6, zdict=d)
            th, c0 = best(lambda: batch.compress(items, 6))
            thd, c1 = best(lambda: batch.compress(items, 6, zdict=d))
            td, _ = best(lambda: batch.compress_dev(ctx, d_in, offs, lens, 6))
            tdd, _ = best(lambda: batch.compress_dev(ctx, d_in, offs, lens, 6, zdict=d))
            tz = sampled(zc(d), items, 2000)
            tz16 = threaded(zc(d), items, 16000)
            r0, r1 = raw / sum(map(len, c0)), raw / sum(map(len, c1))
            print(f"{source:>6} {size:5d} {n:6d} {'c':>3} | {th*1e3:7.1f} {thd*1e3:7.1f} {td*1e3:7.1f} {tdd*1e3:7.1f} | {tz*1e3:8.0f} {tz16*1e3:8.0f} | "
                  f"{r0:5.2f} {r1:7.2f}", flush=True)
            outs = {}
            for key, comp, zz in (("0", c0, None), ("1", c1, d)):
                clens = np.array([len(c) for c in comp], dtype=np.uint64)
                coffs = np.zeros(n, dtype=np.uint64); coffs[1:] = np.cumsum(clens)[:-1]
                d_c = devmem.from_host(ctx, np.frombuffer(b"".join(comp) + bytes(64), np.uint8))
                batch.decompress(comp[:64], zdict=zz)
                t, o = best(lambda: batch.decompress(comp, zdict=zz))
                assert o == items
                tdev, _ = best(lambda: batch.decompress_dev(ctx, d_c, coffs, clens, zdict=zz))
                outs[key] = (t, tdev)
                del d_c
            tz = sampled(zd(d), c1, 2000)
            tz16 = threaded(zd(d), c1, 16000)
            print(f"{source:>6} {size:5d} {n:6d} {'d':>3} | {outs['0'][0]*1e3:7.1f} {outs['1'][0]*1e3:7.1f} {outs['0'][1]*1e3:7.1f} "
                  f"{outs['1'][1]*1e3:7.1f} | {tz*1e3:8.0f} {tz16*1e3:8.0f} | {r0:5.2f} {r1:7.2f}", flush=True)
            del d_in, items, c0, c1


if __name__ == "__main__":
    main()

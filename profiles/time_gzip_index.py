"""Seek-point index (zlib_ng_amd/gzip_index.py) on 1 GiB of the bench text written as ONE member by the stdlib gzip at levels 6 and
1: index build time, the indexed whole-file decode (wall and kernel time) against gzip_ng.open(...).read() of the same file without
an index, random 4 KiB read_at latency through the span kernel and through the chunk-parallel resume decoder, read_ranges of 1 000
random 4 KiB ranges, and the index file's size.  For comparison, the same text as independent 128 KiB members decoded by
za_k_inflate_serial_members.  No torch: plain host buffers.

    python profiles/time_gzip_index.py [GiB] [out.txt]
"""
import gzip
import io
import os
import random
import statistics
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
from zlib_ng_amd import corpus, gzip_index, gzip_ng, zlib_ng  # noqa: E402

GIB = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
OUT = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def kernel_ms(ctx):
    return {k: round(v[0], 2) for k, v in ctx.kernel_times(True).items() if v[1]}


ctx = zlib_ng._ctx()
piece = corpus.text(64 << 20, seed=1).tobytes()
n = int(GIB * (1 << 30))
data = (piece * ((n + len(piece) - 1) // len(piece)))[:n]
tmp = tempfile.mkdtemp()
say(f"data: {n / 2**20:.0f} MiB of corpus.text (seed 1), one gzip member written by the stdlib zlib {zlib.ZLIB_RUNTIME_VERSION}")
for level in (6, 1):
    path = os.path.join(tmp, f"l{level}.gz")
    t = time.perf_counter()
    with open(path, "wb") as f:
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        for o in range(0, n, 64 << 20):
            f.write(c.compress(data[o:o + (64 << 20)]))
        f.write(c.flush())
    fsize = os.path.getsize(path)
    say(f"\n== level {level}: {fsize / 2**20:.1f} MiB compressed (written in {time.perf_counter() - t:.1f} s)")

    t = time.perf_counter()
    with gzip_ng.open(path, "rb") as g:
        back = g.read()
    t_plain = time.perf_counter() - t
    assert back == data
    del back
    say(f"gzip_ng.open(...).read(), no index: {t_plain * 1e3:.0f} ms = {n / t_plain / 1e9:.2f} GB/s")

    t = time.perf_counter()
    idx = gzip_index.build(path, spacing=1 << 20)
    t_build = time.perf_counter() - t
    kern = sum(1 for p in idx.points if p.kernel)
    gaps = sorted(p.out_len for p in idx.points)
    say(f"build (spacing 1 MiB): {t_build * 1e3:.0f} ms = {n / t_build / 1e9:.2f} GB/s; {len(idx.points)} points, {kern} kernel spans, "
        f"span bytes p50 {gaps[len(gaps) // 2]} max {gaps[-1]}")
    buf = io.BytesIO()
    idx.save(buf)
    say(f"index file: {len(buf.getvalue())} bytes ({len(buf.getvalue()) / fsize * 100:.2f} % of the data file; raw windows {idx._win_raw} bytes)")
    idx = gzip_index.GzipIndex.load(io.BytesIO(buf.getvalue()))

    with open(path, "rb") as f:
        assert idx.read_at(f, 0, 10) == data[:10]            # (warm: windows section decompressed, buffers allocated)
        for rep in range(2):
            ctx.profiling(True)
            ctx.kernel_times(True)
            ctx.span_stats(True)
            t = time.perf_counter()
            whole = idx.decompress(f)
            t_dec = time.perf_counter() - t
            km = kernel_ms(ctx)
            ctx.profiling(False)
            spans, nbytes = ctx.span_stats(True)
        assert whole == data
        del whole
        inf = km.get("inflate", 0.0)
        say(f"GzipIndex.decompress: {t_dec * 1e3:.0f} ms wall = {n / t_dec / 1e9:.2f} GB/s, {spans} spans in one launch; kernel ms {km}; "
            f"span kernel {inf / (n / 2**30):.1f} ms per GiB ({n / (inf / 1e3) / 1e9:.1f} GB/s device)")
        say(f"  indexed decode vs plain read: {t_plain / t_dec:.2f}x")

        rnd = random.Random(1)
        for label, thr in (("span kernel", 1 << 62), ("resume (chunk-parallel)", 0)):
            gzip_index.LONE_RESUME_MIN = thr
            ctx.span_stats(True)
            lat = []
            for _ in range(60):
                o = rnd.randrange(n - 4096)
                t = time.perf_counter()
                got = idx.read_at(f, o, 4096)
                lat.append(time.perf_counter() - t)
                assert got == data[o:o + 4096]
            lat.sort()
            say(f"read_at 4 KiB via {label}: p50 {lat[len(lat) // 2] * 1e3:.2f} ms, p99 {lat[int(len(lat) * 0.99) - 1] * 1e3:.2f} ms, "
                f"mean {statistics.mean(lat) * 1e3:.2f} ms ({ctx.span_stats(True)[0]} of {len(lat)} reads took the span kernel)")
        gzip_index.LONE_RESUME_MIN = 256 << 10
        lat = []
        for _ in range(200):
            o = rnd.randrange(n - 4096)
            t = time.perf_counter()
            got = idx.read_at(f, o, 4096)
            lat.append(time.perf_counter() - t)
            assert got == data[o:o + 4096]
        lat.sort()
        say(f"read_at 4 KiB (default route), 200 random: p50 {lat[100] * 1e3:.2f} ms, p99 {lat[197] * 1e3:.2f} ms")
        ranges = [(rnd.randrange(n - 4096), 4096) for _ in range(1000)]
        t = time.perf_counter()
        got = idx.read_ranges(f, ranges)
        t_rr = time.perf_counter() - t
        assert all(g == data[o:o + k] for g, (o, k) in zip(got, ranges))
        say(f"read_ranges of 1000 random 4 KiB ranges: {t_rr * 1e3:.0f} ms ({len({i for o, k in ranges for i in idx._spans_for(o, k)})} spans decoded)")

    with gzip_ng.open(path, "rb", index=idx) as g:
        t = time.perf_counter()
        g.seek(n - (1 << 20))
        g.read(4096)
        say(f"gzip_ng.open(index=...): seek to the last MiB + 4 KiB read {(time.perf_counter() - t) * 1e3:.1f} ms")
    os.unlink(path)

# the member-parallel reference point: the same text as independent 128 KiB members (what za_k_inflate_serial_members decodes)
m = min(n, 256 << 20)
mem = b"".join(gzip.compress(data[o:o + (128 << 10)], 6, mtime=0) for o in range(0, m, 128 << 10))
ctx.gunzip(mem, m)
ctx.profiling(True)
ctx.kernel_times(True)
code, out, nm = ctx.gunzip(mem, m)
km = kernel_ms(ctx)
ctx.profiling(False)
assert code == 0 and out == data[:m]
say(f"\n{nm} stdlib members of 128 KiB (level 6, {m >> 20} MiB): kernel ms {km}; inflate {km.get('inflate', 0) / (m / 2**30):.1f} ms per GiB")
if OUT:
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")

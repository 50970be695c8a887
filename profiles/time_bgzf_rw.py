"""BGZF timings.  No torch: device memory through zlib_ng_amd.devmem, wall clock around calls that end in a
synchronisation, every pair of legs alternated inside one process.

  write   bgzf.compress_dev on WRITE_MIB (4096) MiB of corpus.text, level 6, device resident, against zngamd_gzip_members_dev with
          block_size 65280 on the same buffer (the same deflate kernels; another frame): five runs each, then one profiled run each
          for the per-class kernel times
  ranges  RANGES (10000) random 100-byte read_ranges on a FILE_MIB (1024) MiB BGZF file, against the same reads answered by decoding
          the same blocks in one launch and slicing on the host (all decoded bytes cross the link: the code without the slice kernel)
  read    BgzfReader against gzip_ng.open, the whole file through readinto

    python profiles/time_bgzf_rw.py [write] [ranges] [read]
"""
import ctypes as C
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
from zlib_ng_amd import _lib, bgzf, corpus, devmem, gzip_ng, zlib_ng  # noqa: E402

BLOCK = 65280
RUNS = int(os.environ.get("RUNS", "5"))


def device_text(ctx, n):
    """n bytes of corpus.text on the device: 64 MiB generated on the host, repeated by device copies"""
    host = corpus.text(min(n, 64 << 20), seed=1)
    d = devmem.empty(ctx, n + 64)
    d[:host.size] = host
    done = host.size
    while done < n:
        k = min(done, n - done)
        d[done:done + k] = d[:k]
        done += k
    d[n:n + 64] = 0
    ctx.sync()
    return d


def report(name, times, nbytes=None):
    med, spread = statistics.median(times), max(times) - min(times)
    rate = f"  {nbytes / med / 1e9:7.2f} GB/s at the median" if nbytes else ""
    print(f"{name:<44s} median {med * 1e3:9.3f} ms  min {min(times) * 1e3:9.3f}  max {max(times) * 1e3:9.3f}  spread {spread * 1e3:8.3f} ms{rate}"
          f"   runs {' '.join('%.3f' % (t * 1e3) for t in times)}")
    return med, spread


def time_write(ctx):
    n = int(os.environ.get("WRITE_MIB", "4096")) << 20
    d_in = device_text(ctx, n)
    out_b = devmem.empty(ctx, ctx.bgzf_room(n, BLOCK))
    out_m = devmem.empty(ctx, ctx.gzip_members_room(n, BLOCK) + 64)
    L, h = ctx.L, ctx.h
    ml, mn = C.c_uint64(0), C.c_uint32(0)

    def leg_bgzf():
        t = time.perf_counter()
        _, nbytes, tab = bgzf.compress_dev(ctx, d_in, n, 6, out=out_b)
        return time.perf_counter() - t, nbytes

    def leg_members():
        t = time.perf_counter()
        ctx._chk(L.zngamd_gzip_members_dev(h, d_in.vp(), n, BLOCK, 6, out_m.vp(), out_m.nbytes - 64, C.byref(ml), C.byref(mn)))
        return time.perf_counter() - t, ml.value

    leg_bgzf(), leg_members()                                # warm-up: code objects, workspaces
    tb, tm = [], []
    for _ in range(RUNS):
        dt, nb_bytes = leg_bgzf()
        tb.append(dt)
        dt, nm_bytes = leg_members()
        tm.append(dt)
    print(f"write: {n >> 20} MiB of corpus.text, level 6, blocks of {BLOCK}: BGZF stream {nb_bytes} bytes, 'ZA' member stream {nm_bytes} bytes")
    mb, _ = report("bgzf.compress_dev", tb, n)
    mm, sm = report("zngamd_gzip_members_dev (block_size 65280)", tm, n)
    rb, rm = sorted(n / t / 1e9 for t in tb), sorted(n / t / 1e9 for t in tm)
    bound = statistics.median(rm) - (rm[-1] - rm[0])
    print(f"write: BGZF median {statistics.median(rb):.2f} GB/s; the member leg's median {statistics.median(rm):.2f} GB/s minus its spread "
          f"{rm[-1] - rm[0]:.2f} GB/s = {bound:.2f} GB/s: {'met' if statistics.median(rb) >= bound else 'MISSED'}")
    for name, leg in (("bgzf.compress_dev", leg_bgzf), ("zngamd_gzip_members_dev", leg_members)):
        ctx.profiling(True)
        ctx.kernel_times(True)
        leg()
        kt = ctx.kernel_times(True)
        ctx.profiling(False)
        print(f"kernel times of one profiled run of {name}: " + ", ".join(f"{k} {v[0]:.3f} ms / {v[1]}" for k, v in kt.items() if v[1]))


def make_file(ctx, path):
    n = int(os.environ.get("FILE_MIB", "1024")) << 20
    d_in = device_text(ctx, n)
    out, nbytes, tab = bgzf.compress_dev(ctx, d_in, n, 6)
    with open(path, "wb") as f:
        step = 256 << 20
        for o in range(0, nbytes, step):
            f.write(out[o:min(nbytes, o + step)].cpu().tobytes())
    ref = d_in[:n].cpu().tobytes()
    return n, nbytes, tab, ref


def time_ranges(ctx, path, n, tab, ref):
    rng = random.Random(1)
    rows = [r for r in tab if r["isize"]]
    ranges, want = [], []
    for _ in range(int(os.environ.get("RANGES", "10000"))):
        r = rows[rng.randrange(len(rows))]
        w = rng.randrange(int(r["isize"]))
        ranges.append((bgzf.make_virtual_offset(int(r["coffset"]), w), 100))
        want.append(ref[int(r["uoffset"]) + w:int(r["uoffset"]) + w + 100])
    rd = bgzf.BgzfReader(path)

    def leg_kernel():
        t = time.perf_counter()
        got = rd.read_ranges(ranges)
        return time.perf_counter() - t, got

    def leg_host():
        """the same plan, the same blocks in one launch of the same decoder -- all of their output copied back and sliced here"""
        t = time.perf_counter()
        here = rd._fp.tell()
        cache, plans = rd._plan_ranges(ranges)
        rd._fp.seek(here)
        need = sorted({p[0] for pieces in plans for p in pieces})
        where, opos = {}, 0
        for c in need:
            where[c] = opos
            opos += cache[c][2]
        code, out, nm = ctx.gunzip(b"".join(cache[c][0] for c in need), opos)
        assert code == 0 and len(out) == opos
        mv = memoryview(out)
        got = [b"".join(bytes(mv[where[c] + a:where[c] + b]) for c, a, b in pieces) for pieces in plans]
        return time.perf_counter() - t, got

    assert leg_kernel()[1] == want and leg_host()[1] == want
    tk, th = [], []
    for _ in range(RUNS):
        tk.append(leg_kernel()[0])
        th.append(leg_host()[0])
    print(f"ranges: {len(ranges)} x 100 bytes on a BGZF file of {os.path.getsize(path)} bytes ({n >> 20} MiB of text)")
    mk, sk = report("read_ranges (slice kernel)", tk)
    mh, sh = report("same blocks decoded, sliced on the host", th)
    print(f"ranges: the slice kernel {'wins' if mh - mk > max(sk, sh) else 'does NOT win'} by more than the spread ({(mh - mk) * 1e3:.3f} ms against {max(sk, sh) * 1e3:.3f} ms)")
    # where the time goes: planning (file reads + host scan) is common to both legs
    t = time.perf_counter()
    cache, plans = rd._plan_ranges(ranges)
    tp = time.perf_counter() - t
    t = time.perf_counter()
    rd._read_planned(cache, plans)
    print(f"ranges: planning (10^4 block reads from the file, host scan) {tp * 1e3:.3f} ms, pack + engine call + result {1e3 * (time.perf_counter() - t):.3f} ms")
    rd.close()


def time_read(path, n, ref):
    buf = bytearray(64 << 20)

    def drain(f):
        t = time.perf_counter()
        total = 0
        while True:
            k = f.readinto(buf)
            if not k:
                break
            total += k
        f.close()
        assert total == n
        return time.perf_counter() - t

    with bgzf.open(path) as f:
        assert f.read(1 << 20) == ref[:1 << 20]
    drain(bgzf.open(path)), drain(gzip_ng.open(path))
    tb, tg = [], []
    for _ in range(RUNS):
        tb.append(drain(bgzf.open(path)))
        tg.append(drain(gzip_ng.open(path)))
    print(f"read: the whole file ({n >> 20} MiB of text) through readinto, 64 MiB at a time")
    mb, sb = report("BgzfReader", tb, n)
    mg, sg = report("gzip_ng.open", tg, n)
    print(f"read: BgzfReader is {'not slower' if mb - mg <= max(sb, sg) else 'SLOWER'} than gzip_ng.open by more than the spread "
          f"({(mb - mg) * 1e3:.3f} ms against {max(sb, sg) * 1e3:.3f} ms)")


def main():
    what = set(sys.argv[1:]) or {"write", "ranges", "read"}
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    if "write" in what:
        time_write(ctx)
    if what & {"ranges", "read"}:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "t.bgzf")
            n, nbytes, tab, ref = make_file(ctx, path)
            if "ranges" in what:
                time_ranges(ctx, path, n, tab, ref)
            if "read" in what:
                time_read(path, n, ref)


if __name__ == "__main__":
    main()

"""BGZF by line: timings, in the manner of profiles/time_bgzf_rw.py.  No torch, wall clock around calls that end
in a synchronisation, the two legs of a comparison alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.
The file is the one of section 5d: FILE_MIB (1024) MiB of corpus.text, level 6, written by bgzf.compress_dev.

  build   LineIndex.build against BgzfReader.readinto over the same file (what counting lines cost before: every decoded byte crosses
          the link).  Bar: build is at least as fast as the readinto leg's median minus that leg's spread (max - min).  Then one
          profiled build for the share of za_k_bgzf_count (class "gather") against the decode (class "inflate").
  lines   read_lines of LINES (10000) random single lines against read_ranges on the true (virtual offset, length) of the same lines,
          computed once from the decoded data.  Bar: read_lines is no slower than the read_ranges leg's median plus that leg's spread.

    python profiles/time_bgzf_lines.py [build] [lines]
"""
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from zlib_ng_amd import _lib, bgzf, zlib_ng  # noqa: E402
from time_bgzf_rw import RUNS, make_file, report  # noqa: E402


def profiled(ctx, what, leg):
    ctx.profiling(True)
    ctx.kernel_times(True)
    leg()
    kt = ctx.kernel_times(True)
    ctx.profiling(False)
    print(f"kernel times of one profiled run of {what}: " + ", ".join(f"{k} {v[0]:.3f} ms / {v[1]}" for k, v in kt.items() if v[1]))
    return kt


def time_build(ctx, path, n, ref):
    buf = bytearray(64 << 20)
    want = ref.count(b"\n")

    def leg_build():
        t = time.perf_counter()
        idx = bgzf.LineIndex.build(path)
        return time.perf_counter() - t, idx

    def leg_readinto():
        """the whole file through readinto; the count on the host that a caller then needs is left out: the leg is the read alone"""
        f = bgzf.open(path)
        t = time.perf_counter()
        total = 0
        while True:
            k = f.readinto(buf)
            if not k:
                break
            total += k
        dt = time.perf_counter() - t
        f.close()
        assert total == n
        return dt, None

    idx = leg_build()[1]
    leg_readinto()
    assert idx.delimiters == want and idx.usize == n
    tb, tr = [], []
    for _ in range(RUNS):
        tb.append(leg_build()[0])
        tr.append(leg_readinto()[0])
    print(f"build: a BGZF file of {os.path.getsize(path)} bytes ({n >> 20} MiB of text, {len(idx)} blocks, {idx.lines} lines); the index is {len(idx.to_bytes())} bytes")
    mb, sb = report("LineIndex.build", tb, n)
    mr, sr = report("BgzfReader.readinto (64 MiB at a time)", tr, n)
    rb, rr = sorted(n / t / 1e9 for t in tb), sorted(n / t / 1e9 for t in tr)
    med_b, med_r = rb[len(rb) // 2], rr[len(rr) // 2]
    bound = med_r - (rr[-1] - rr[0])
    print(f"build: median {med_b:.2f} GB/s; the readinto leg's median {med_r:.2f} GB/s minus its spread {rr[-1] - rr[0]:.2f} GB/s = {bound:.2f} GB/s: "
          f"{'met' if med_b >= bound else 'MISSED'}")
    kt = profiled(ctx, "LineIndex.build", leg_build)
    count_ms, decode_ms = kt["gather"][0], kt["inflate"][0]
    print(f"build: za_k_bgzf_count {count_ms:.3f} ms in {kt['gather'][1]} launches against {decode_ms:.3f} ms of decode in {kt['inflate'][1]}: "
          f"{100 * count_ms / max(decode_ms, 1e-9):.2f} % of the decode, {100 * count_ms / (count_ms + decode_ms):.2f} % of a window's kernel time")
    return idx


def time_lines(ctx, path, n, tab, ref, idx):
    arr = np.frombuffer(ref, np.uint8)
    nl = np.flatnonzero(arr == 10)
    rng = random.Random(1)
    picks = np.array([rng.randrange(idx.lines) for _ in range(int(os.environ.get("LINES", "10000")))], np.int64)
    starts = np.where(picks > 0, nl[np.maximum(picks, 1) - 1] + 1, 0)
    ends = np.where(picks < len(nl), nl[np.minimum(picks, len(nl) - 1)] + 1, n)
    rows = tab[tab["isize"] > 0]
    blk = np.searchsorted(rows["uoffset"], starts, "right") - 1
    ranges = [(bgzf.make_virtual_offset(int(c), int(s - u)), int(e - s)) for c, u, s, e in zip(rows["coffset"][blk], rows["uoffset"][blk], starts, ends)]
    line_ranges = [(int(p), 1) for p in picks]
    want = [ref[s:e] for s, e in zip(starts.tolist(), ends.tolist())]
    rd = bgzf.BgzfReader(path)

    def leg_lines():
        t = time.perf_counter()
        got = rd.read_lines(idx, line_ranges)
        return time.perf_counter() - t, got

    def leg_ranges():
        t = time.perf_counter()
        got = rd.read_ranges(ranges)
        return time.perf_counter() - t, got

    assert leg_lines()[1] == want and leg_ranges()[1] == want
    tl, tr = [], []
    for _ in range(RUNS):
        tl.append(leg_lines()[0])
        tr.append(leg_ranges()[0])
    print(f"lines: {len(picks)} random single lines ({sum(len(w) for w in want)} bytes) of {idx.lines}")
    ml, sl = report("read_lines (index, select kernel)", tl)
    mr, sr = report("read_ranges on the true (voffset, length)", tr)
    print(f"lines: read_lines median {ml * 1e3:.3f} ms; the read_ranges leg's median {mr * 1e3:.3f} ms plus its spread {sr * 1e3:.3f} ms = "
          f"{(mr + sr) * 1e3:.3f} ms: {'met' if ml <= mr + sr else 'MISSED'}")
    ctx.bgzf_stats()
    kt = profiled(ctx, "read_lines", leg_lines)
    print("lines: decode launches, blocks decoded, slices gathered of that run:", ctx.bgzf_stats())
    profiled(ctx, "read_ranges", leg_ranges)
    print("lines: the same for read_ranges:", ctx.bgzf_stats())
    rd.close()


def main():
    what = set(sys.argv[1:]) or {"build", "lines"}
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.bgzf")
        n, nbytes, tab, ref = make_file(ctx, path)
        idx = time_build(ctx, path, n, ref) if "build" in what else bgzf.LineIndex.build(path)
        if "lines" in what:
            time_lines(ctx, path, n, tab, ref, idx)


if __name__ == "__main__":
    main()

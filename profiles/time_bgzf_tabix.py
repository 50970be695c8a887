"""BGZF by region: timings, in the manner of profiles/time_bgzf_grep.py.  No torch, wall clock around calls that
end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  The file is
generated here: FILE_MIB (1024) MiB of a sorted VCF-like text (NAMES (24) names, lines of equal length, positions ascending up to
2**29), level 6, written by BgzfWriter.

  a    TabixIndex.build
  b    LineIndex.build: the same decode -- the floor
  c    BgzfReader.readinto of the whole file, 64 MiB at a time: what any host indexer has to do first
  d1   fetch of 1 random region of 10 kb          d100, d10000: of 100 and of 10 000 such regions in one call
  e    what a caller did before: grep(name + b"\\t", line_start=True) and a filter of the positions on the host, for d1's region

Bars: a's median lies below c's median minus c's spread (max - min); d1's median lies below e's median minus e's spread.  Reported
without a bar: a against b, and the share of the new kernels (class "gather") in the decode (class "inflate") of one profiled run.

    python profiles/time_bgzf_tabix.py
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
from time_bgzf_lines import profiled  # noqa: E402
from time_bgzf_rw import RUNS, report  # noqa: E402

TEMPLATE = b"chr00\t000000000\trs000000000\tA\tG\t50\tPASS\tDP=000;AF=0.25\n"


def digits(mat, col, width, values):
    for k in range(width):
        mat[:, col + width - 1 - k] = 48 + (values // 10 ** k) % 10


def make_vcf(path, nbytes, names):
    """-> (bytes of text, lines, per name the positions): `names` names of equally many lines each, POS ascending with repeats"""
    rng = np.random.default_rng(5)
    per = nbytes // len(TEMPLATE) // names
    step = ((1 << 29) - 10) // per
    tpl = np.frombuffer(TEMPLATE, np.uint8)
    pos_of, total = [], 0
    with bgzf.open(path, "wb", 6) as w:
        head = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
        w.write(head)
        for i in range(names):
            pos = 1 + np.cumsum(rng.integers(0, 2 * step - 1, per))
            pos = np.minimum(pos, (1 << 29) - 1)
            mat = np.tile(tpl, (per, 1))
            digits(mat, 3, 2, np.full(per, i + 1))
            digits(mat, 6, 9, pos)
            digits(mat, 18, 9, np.arange(per) + i * per)
            digits(mat, 43, 3, rng.integers(0, 1000, per))
            w.write(mat.tobytes())
            pos_of.append(pos)
            total += mat.size
    return total + len(head), per * names + 2, pos_of


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_want, names = int(os.environ.get("FILE_MIB", "1024")) << 20, int(os.environ.get("NAMES", "24"))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.vcf.gz")
        n, nlines, pos_of = make_vcf(path, n_want, names)
        print(f"file: {os.path.getsize(path)} bytes ({n >> 20} MiB of text, {nlines} lines, {names} names)")
        rng = random.Random(9)

        def region():
            i = rng.randrange(names)
            beg = rng.randrange(int(pos_of[i][-1]) - 10000)
            return b"chr%02d" % (i + 1), beg, beg + 10000

        regions = {k: [region() for _ in range(k)] for k in (1, 100, 10000)}
        want = {k: [int(np.searchsorted(pos_of[int(r[0][3:]) - 1], r[2], "right") - np.searchsorted(pos_of[int(r[0][3:]) - 1], r[1], "right"))
                    for r in regs] for k, regs in regions.items()}       # beg < POS <= end: REF is one base
        buf = bytearray(64 << 20)
        tbi = bgzf.TabixIndex.build(path, "vcf")
        tbi.validate(os.path.getsize(path))
        reader = bgzf.BgzfReader(path)

        def leg_build():
            t = time.perf_counter()
            idx = bgzf.TabixIndex.build(path, "vcf")
            return time.perf_counter() - t, idx

        def leg_lines():
            t = time.perf_counter()
            idx = bgzf.LineIndex.build(path)
            return time.perf_counter() - t, idx

        def leg_readinto():
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
            return dt, total

        def leg_fetch(k):
            def leg():
                t = time.perf_counter()
                got = reader.fetch(tbi, regions[k])
                return time.perf_counter() - t, got
            return leg

        def leg_grep():
            name, beg, end = regions[1][0]
            t = time.perf_counter()
            hits = bgzf.grep(path, name + b"\t", line_start=True)
            rows = [ln for ln in hits if beg < int(ln.split(b"\t", 2)[1]) <= end]      # POS - 1 in [beg, end): REF is one base
            return time.perf_counter() - t, rows

        legs = [("a TabixIndex.build", leg_build), ("b LineIndex.build", leg_lines), ("c BgzfReader.readinto, whole file", leg_readinto),
                ("d1 fetch, 1 region of 10 kb", leg_fetch(1)), ("d100 fetch, 100 regions", leg_fetch(100)),
                ("d10000 fetch, 10 000 regions", leg_fetch(10000)), ("e grep(name + tab) + host filter, 1 region", leg_grep)]
        warm = [leg() for _, leg in legs]
        assert warm[0][1] == tbi and len(tbi) == names and warm[1][1].lines == nlines
        for k, w in zip((1, 100, 10000), warm[3:6]):
            assert np.bincount(w[1].region, minlength=k).tolist() == want[k], k
        assert list(warm[3][1]) == warm[6][1]
        print(f"index: {len(tbi.to_bytes(compressed=False))} bytes plain; d1 returns {len(warm[3][1])} lines, d100 {len(warm[4][1])}, "
              f"d10000 {len(warm[5][1])}; e's grep returns {len(pos_of[0])} lines to the host")
        del warm
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, leg) in enumerate(legs):
                times[k].append(leg()[0])
        med = [report(name, t, n if k < 3 else None) for k, ((name, _), t) in enumerate(zip(legs, times))]
        (ma, _), (mb, _), (mc, sc), (md, _), _, _, (me, se) = med
        print(f"bar: a median {ma * 1e3:.3f} ms against c's median {mc * 1e3:.3f} ms minus its spread {sc * 1e3:.3f} ms = {(mc - sc) * 1e3:.3f} ms: "
              f"{'met' if ma < mc - sc else 'MISSED'}")
        print(f"bar: d1 median {md * 1e3:.3f} ms against e's median {me * 1e3:.3f} ms minus its spread {se * 1e3:.3f} ms = {(me - se) * 1e3:.3f} ms: "
              f"{'met' if md < me - se else 'MISSED'}")
        print(f"a against b (the floor): {ma * 1e3:.3f} ms against {mb * 1e3:.3f} ms, {100 * (ma - mb) / mb:+.1f} %")
        for what, leg in (("TabixIndex.build", leg_build), ("fetch, 1 region", leg_fetch(1)), ("fetch, 10 000 regions", leg_fetch(10000))):
            ctx.bgzf_stats()
            kt = profiled(ctx, what, leg)
            g, i = kt["gather"][0], kt["inflate"][0]
            print(f"{what}: field kernels {g:.3f} ms in {kt['gather'][1]} timed spans against {i:.3f} ms of decode in {kt['inflate'][1]}: "
                  f"{100 * g / max(i, 1e-9):.2f} % of the decode; decode launches, blocks decoded, slices gathered: {ctx.bgzf_stats()}")
        reader.close()


if __name__ == "__main__":
    main()

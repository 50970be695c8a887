"""BGZF by content: timings, in the manner of profiles/time_bgzf_lines.py.  No torch, wall clock around calls that
end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  The file is the
one of sections 5d and 5e: FILE_MIB (1024) MiB of corpus.text, level 6, written by bgzf.compress_dev.

  a   grep(count=True) of a pattern that well under 1 % of the lines contain
  b   grep of the same pattern, returning the lines
  c   what it replaces: BgzfReader.readinto, 64 MiB at a time, WITHOUT any search on the host
  d   c plus the host's filter: bytes.find over every window
  e   LineIndex.build: the same decode, the same bytes over the link -- the floor
  f   grep of a pattern that about half of the lines contain (reported only: bound by the link by construction)

Bars: the medians of a and b lie below c's median minus c's spread (max - min).  Reported without a bar: a against e, and the share of
the grep kernels (class "gather") in the decode (class "inflate") of one profiled run.

    python profiles/time_bgzf_grep.py
"""
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from zlib_ng_amd import _lib, bgzf, zlib_ng  # noqa: E402
from time_bgzf_lines import profiled  # noqa: E402
from time_bgzf_rw import RUNS, make_file, report  # noqa: E402


def pick_patterns(ref):
    """(a pattern in about 0.3 % of the lines, one in about half of them), judged on the first 32 MiB of the text"""
    lines = ref[:32 << 20].split(b"\n")
    rng = random.Random(7)
    best = {0.003: (None, 9.0), 0.5: (None, 9.0)}
    for _ in range(80):
        ln = lines[rng.randrange(len(lines))]
        if len(ln) < 8:
            continue
        o = rng.randrange(len(ln) - 6)
        p = ln[o:o + rng.randrange(1, 7)]
        share = sum(1 for x in lines if p in x) / len(lines)
        for goal in best:
            miss = abs(share - goal) / goal
            if miss < best[goal][1]:
                best[goal] = (p, miss, share)
    return best[0.003][0], best[0.5][0]


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t.bgzf")
        n, nbytes, tab, ref = make_file(ctx, path)
        rare, common = pick_patterns(ref)
        lines = ref.split(b"\n")
        want_rare, want_common = sum(1 for x in lines if rare in x), sum(1 for x in lines if common in x)
        nlines = len(lines) - (0 if lines[-1] else 1)
        del lines
        print(f"file: {nbytes} bytes ({n >> 20} MiB of text, {nlines} lines); rare pattern {rare!r} in {want_rare} lines "
              f"({100 * want_rare / nlines:.3f} %), common pattern {common!r} in {want_common} ({100 * want_common / nlines:.1f} %)")
        buf = bytearray(64 << 20)

        def leg_count():
            t = time.perf_counter()
            got = bgzf.grep(path, rare, count=True)
            return time.perf_counter() - t, got

        def leg_lines(p=None):
            t = time.perf_counter()
            got = bgzf.grep(path, p or rare)
            return time.perf_counter() - t, got

        def leg_common():
            return leg_lines(common)

        def leg_readinto(search=False):
            f = bgzf.open(path)
            t = time.perf_counter()
            total = hits = 0
            while True:
                k = f.readinto(buf)
                if not k:
                    break
                total += k
                if search:                             # (occurrences, not lines, and none across a window's edge: the cheapest host filter)
                    at = buf.find(rare, 0, k)
                    while at >= 0:
                        hits += 1
                        at = buf.find(rare, at + 1, k)
            dt = time.perf_counter() - t
            f.close()
            assert total == n
            return dt, hits

        def leg_filter():
            return leg_readinto(True)

        def leg_build():
            t = time.perf_counter()
            idx = bgzf.LineIndex.build(path)
            return time.perf_counter() - t, idx

        legs = [("a grep(count=True), rare pattern", leg_count), ("b grep, rare pattern, lines returned", leg_lines),
                ("c BgzfReader.readinto, no search", leg_readinto), ("d readinto + bytes.find per window", leg_filter),
                ("e LineIndex.build", leg_build), ("f grep, common pattern, lines returned", leg_common)]
        warm = [leg() for _, leg in legs]
        assert warm[0][1] == want_rare and len(warm[1][1]) == want_rare and len(warm[5][1]) == want_common and warm[1][1].searched == nlines
        assert warm[4][1].lines == nlines and warm[3][1] >= want_rare
        print(f"b returns {int(warm[1][1].offsets[-1])} bytes of lines, f {int(warm[5][1].offsets[-1])}")
        del warm
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, leg) in enumerate(legs):
                times[k].append(leg()[0])
        med = [report(name, t, n) for (name, _), t in zip(legs, times)]
        (ma, _), (mb, _), (mc, sc), (md, _), (me, _), (mf, _) = med
        bound = mc - sc
        for name, m in (("a", ma), ("b", mb)):
            print(f"bar: {name} median {m * 1e3:.3f} ms against c's median {mc * 1e3:.3f} ms minus its spread {sc * 1e3:.3f} ms = {bound * 1e3:.3f} ms: "
                  f"{'met' if m < bound else 'MISSED'}")
        print(f"a against e (the floor): {ma * 1e3:.3f} ms against {me * 1e3:.3f} ms, {100 * (ma - me) / me:+.1f} %; d (what a caller pays today) "
              f"{md * 1e3:.3f} ms; f {mf * 1e3:.3f} ms")
        for what, leg in (("grep(count=True)", leg_count), ("grep, rare pattern", leg_lines), ("grep, common pattern", leg_common)):
            ctx.bgzf_stats()
            kt = profiled(ctx, what, leg)
            g, i = kt["gather"][0], kt["inflate"][0]
            print(f"{what}: grep kernels {g:.3f} ms in {kt['gather'][1]} timed spans against {i:.3f} ms of decode in {kt['inflate'][1]}: "
                  f"{100 * g / max(i, 1e-9):.2f} % of the decode; decode launches, blocks decoded, lines gathered: {ctx.bgzf_stats()}")


if __name__ == "__main__":
    main()

"""BGZF by sequence: timings, in the manner of profiles/time_bgzf_tabix.py.  No torch, wall clock around calls
that end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  The file
is generated here: FILE_MIB (1024) MiB of FASTA, NAMES (24) sequences of equal length in lines of 60 bases, level 6, written by
BgzfWriter; and a variant of the same bases with every sequence on one line.

  a    FaidxIndex.build                      a1: of the variant with one line per sequence
  b    LineIndex.build: the same decode -- the floor
  c    BgzfReader.readinto of the whole file, 64 MiB at a time: what any host indexer has to do first
  d1   fetch_seq of 1 random region of 100 bases      d100, d10000: of 100 and of 10 000 such regions in one call; dseq: one whole sequence
  e    what a caller did before: the same byte spans, computed by hand from the .fai columns, through read_ranges, and bytes.replace
       on the host (e1, e100, e10000, eseq)

Bars: a's median lies below c's median minus c's spread (max - min); d10000's median lies below e10000's median minus e10000's
spread.  Reported without a bar: a against b, a1 against a (no thread walks a line: the ratio should be near 1), and the share of
the new kernels (class "gather") in the decode (class "inflate") of one profiled run.

    python profiles/time_bgzf_faidx.py
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

LB = 60


def make_fasta(path, path1, nbytes, names):
    """-> (per sequence its bases as a uint8 array, bytes of text of the wrapped file, its lines, bytes of text of the other)"""
    rng = np.random.default_rng(5)
    per = nbytes // names // (LB + 1) * LB                   # bases per sequence: whole lines
    seqs, total, total1, nlines = [], 0, 0, 0
    with bgzf.open(path, "wb", 6) as w, bgzf.open(path1, "wb", 6) as w1:
        for i in range(names):
            seq = np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, per)]
            # (long runs of one repeated block, as a genome has them, so that level 6 has something to find)
            seq[per // 3:per // 3 + per // 4] = np.resize(seq[:5000], per // 4)
            head = b">chr%02d sequence %d of the timing file\n" % (i + 1, i)
            mat = np.full((per // LB, LB + 1), 10, np.uint8)
            mat[:, :LB] = seq.reshape(-1, LB)
            w.write(head)
            w.write(mat.tobytes())
            w1.write(head)
            w1.write(seq.tobytes())
            w1.write(b"\n")
            seqs.append(seq)
            total += len(head) + mat.size
            total1 += len(head) + per + 1
            nlines += 1 + per // LB
    return seqs, total, nlines, total1


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_want, names = int(os.environ.get("FILE_MIB", "1024")) << 20, int(os.environ.get("NAMES", "24"))
    with tempfile.TemporaryDirectory() as d:
        path, path1 = os.path.join(d, "ref.fa.gz"), os.path.join(d, "ref1.fa.gz")
        seqs, n, nlines, n1 = make_fasta(path, path1, n_want, names)
        per = len(seqs[0])
        print(f"file: {os.path.getsize(path)} bytes ({n >> 20} MiB of text, {nlines} lines, {names} sequences of {per} bases); "
              f"one line per sequence: {os.path.getsize(path1)} bytes ({n1 >> 20} MiB of text)")
        rng = random.Random(9)

        def region():
            i = rng.randrange(names)
            beg = rng.randrange(per - 100)
            return b"chr%02d" % (i + 1), beg, beg + 100

        regions = {k: [region() for _ in range(k)] for k in (1, 100, 10000)}
        regions["seq"] = [(b"chr07", 0, per)]
        want = {k: [seqs[int(r[0][3:]) - 1][r[1]:r[2]].tobytes() for r in regs] for k, regs in regions.items()}
        buf = bytearray(64 << 20)
        fai = bgzf.FaidxIndex.build(path)
        fai1 = bgzf.FaidxIndex.build(path1)
        assert len(fai) == len(fai1) == names and all(fai[nm][0] == per and fai[nm][2:] == (LB, LB + 1) for nm in fai.names)
        assert all(fai1[nm][0] == per and fai1[nm][2:] == (per, per + 1) for nm in fai1.names) and fai.gzi == bgzf.GziIndex.build(path)
        reader = bgzf.BgzfReader(path)

        def leg_build(p):
            def leg():
                t = time.perf_counter()
                idx = bgzf.FaidxIndex.build(p)
                return time.perf_counter() - t, idx
            return leg

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
                got = reader.fetch_seq(fai, regions[k])
                return time.perf_counter() - t, list(got)
            return leg

        def leg_ranges(k):
            def leg():
                t = time.perf_counter()
                ranges = []
                for name, beg, end in regions[k]:                # the arithmetic of faidx on the .fai columns, by hand
                    _, off, lb, lw = fai[name]
                    first, last = off + beg // lb * lw + beg % lb, off + (end - 1) // lb * lw + (end - 1) % lb
                    ranges.append((fai.gzi.voffset(first), last + 1 - first))
                got = [x.replace(b"\n", b"") for x in reader.read_ranges(ranges)]
                return time.perf_counter() - t, got
            return leg

        legs = [("a FaidxIndex.build", leg_build(path)), ("a1 FaidxIndex.build, one line per sequence", leg_build(path1)),
                ("b LineIndex.build", leg_lines), ("c BgzfReader.readinto, whole file", leg_readinto)]
        legs += [(f"d{k} fetch_seq, {k} region(s) of 100 bases", leg_fetch(k)) for k in (1, 100, 10000)] + [("dseq fetch_seq, one whole sequence", leg_fetch("seq"))]
        legs += [(f"e{k} read_ranges + bytes.replace, {k} region(s)", leg_ranges(k)) for k in (1, 100, 10000)] + [("eseq read_ranges + bytes.replace, one whole sequence", leg_ranges("seq"))]
        warm = [leg() for _, leg in legs]
        assert warm[0][1] == fai and warm[1][1] == fai1 and warm[2][1].lines == nlines
        for k, wd, we in zip((1, 100, 10000, "seq"), warm[4:8], warm[8:12]):
            assert wd[1] == want[k] and we[1] == want[k], k
        del warm
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, leg) in enumerate(legs):
                times[k].append(leg()[0])
        med = [report(name, t, (n1 if k == 1 else n) if k < 4 else None) for k, ((name, _), t) in enumerate(zip(legs, times))]
        (ma, _), (ma1, _), (mb, _), (mc, sc) = med[:4]
        (md, _), (me, se) = med[6], med[10]
        print(f"bar: a median {ma * 1e3:.3f} ms against c's median {mc * 1e3:.3f} ms minus its spread {sc * 1e3:.3f} ms = {(mc - sc) * 1e3:.3f} ms: "
              f"{'met' if ma < mc - sc else 'MISSED'}")
        print(f"bar: d10000 median {md * 1e3:.3f} ms against e10000's median {me * 1e3:.3f} ms minus its spread {se * 1e3:.3f} ms = "
              f"{(me - se) * 1e3:.3f} ms: {'met' if md < me - se else 'MISSED'}")
        print(f"a against b (the floor): {ma * 1e3:.3f} ms against {mb * 1e3:.3f} ms, {100 * (ma - mb) / mb:+.1f} %")
        print(f"a1 against a (one line per sequence against lines of {LB}): {ma1 * 1e3:.3f} ms against {ma * 1e3:.3f} ms, ratio {ma1 / ma:.3f}")
        for what, leg in (("FaidxIndex.build", leg_build(path)), ("FaidxIndex.build, one line per sequence", leg_build(path1)),
                          ("fetch_seq, 10 000 regions", leg_fetch(10000)), ("fetch_seq, one whole sequence", leg_fetch("seq"))):
            ctx.bgzf_stats()
            kt = profiled(ctx, what, leg)
            g, i = kt["gather"][0], kt["inflate"][0]
            print(f"{what}: record kernels {g:.3f} ms in {kt['gather'][1]} timed spans against {i:.3f} ms of decode in {kt['inflate'][1]}: "
                  f"{100 * g / max(i, 1e-9):.2f} % of the decode; decode launches, blocks decoded, spans gathered: {ctx.bgzf_stats()}")
        reader.close()


if __name__ == "__main__":
    main()

"""BGZF by a label per record: timings, in the manner of profiles/time_bgzf_classify.py: its generated FASTQ of
about FILE_MIB (1024) MiB as R1 (every read begins with one of eight barcodes of 16 bases, a third of the reads each with 0, 1 and 2
bases substituted) and a mate file R2 of the same reads (the same headers, bases of their own, no barcode); wall clock around calls
that end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.

  a    demux of R1 to ten files (os.devnull) at level 6: the call that exists without this section, the yardstick
  b    partition_records of R2 with the labels of a's classification, to ten files
  c    b with the unassigned class's output None: its records are dropped on the device
  d    demux_paired of both files to twice ten files

Every leg is checked against the generator: a read whose barcode has at most one base substituted belongs to that barcode's class, a
read with two is unassigned -- the reads in which 16 bases further on lie within one substitution of a barcode by chance are found by
numpy (near_reads of time_bgzf_grep_approx.py) and left out of the comparison of the classes; the warm-up runs of b, c and d go to
files, which the system gzip decodes and which must be R2's (and R1's) records of each class, whole and in order.
Bars: (1) b's median <= a's median, beyond the larger of the two spreads; (2) c's median < b's median by more than the larger spread;
(3) d's median <= a's median + b's median, within the spreads.

    python profiles/time_bgzf_partition.py > profiles/bgzf_partition.txt
"""
import gzip
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
from zlib_ng_amd import _lib, bgzf, devmem, zlib_ng  # noqa: E402
from time_bgzf_rw import RUNS, report  # noqa: E402
from time_bgzf_grep_records import HEAD, READ, REC, make_fastq  # noqa: E402
from time_bgzf_grep_approx import ACGT, L, near_reads  # noqa: E402
from time_bgzf_classify import barcodes  # noqa: E402


def write_bgzf(ctx, text, path):
    n = len(text)
    d_in = devmem.empty(ctx, n + 64)
    for o in range(0, n, 64 << 20):
        piece = np.frombuffer(text, np.uint8, min(64 << 20, n - o), o)
        d_in[o:o + piece.size] = piece
    d_in[n:n + 64] = 0
    ctx.sync()
    out, nbytes, tab = bgzf.compress_dev(ctx, d_in, n, 6)
    with open(path, "wb") as f:
        for o in range(0, nbytes, 256 << 20):
            f.write(out[o:min(nbytes, o + (256 << 20))].cpu().tobytes())
    return nbytes


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, tagged = make_fastq(n_reads)
    mate = arr.copy()                                          # R2: the same reads' headers, the bases the generator gave them
    rng = np.random.default_rng(23)
    eight = barcodes(rng, 64)[:8]
    t = time.perf_counter()
    i = np.arange(n_reads)
    which, subst = i % 8, i // 8 % 3
    table = np.array([np.frombuffer(p, np.uint8) for p in eight])
    arr[:, HEAD:HEAD + L] = table[which]
    for s in (1, 2):                                           # s bases substituted: places r % L and (r + 7) % L of read r
        rows = np.nonzero(subst >= s)[0]
        col = (rows + 7 * (s - 1)) % L
        old = arr[rows, HEAD + col]
        arr[rows, HEAD + col] = ACGT[(np.searchsorted(ACGT, old) + 1 + rows % 3) % 4]
    bases = arr[:, HEAD:HEAD + READ]
    assert ((bases[:, :L] != table[which]).sum(1) == subst).all()
    want = np.where(subst <= 1, which, 9).astype(np.int32)     # the generator's classes: the barcode, or unassigned
    chance = []
    for o in range(0, n_reads, 1 << 18):
        blk = np.empty_like(bases[o:o + (1 << 18)])
        blk[:, :-1], blk[:, -1] = bases[o:o + (1 << 18), 1:], ord("A")
        chance += [o + r for r in near_reads(blk, eight, 1)]
    keep = np.ones(n_reads, bool)
    keep[chance] = False
    text1, text2 = arr.tobytes(), mate.tobytes()
    del arr, bases, mate
    n = len(text1)
    print(f"expected classes found on the host in {time.perf_counter() - t:.1f} s; reads within one substitution of a barcode by chance: {len(chance)}")

    with tempfile.TemporaryDirectory() as d:
        p1, p2 = os.path.join(d, "r1.fastq.gz"), os.path.join(d, "r2.fastq.gz")
        nb1, nb2 = write_bgzf(ctx, text1, p1), write_bgzf(ctx, text2, p2)
        print(f"files: R1 {nb1} bytes, R2 {nb2} bytes ({n} bytes of text each, {n_reads} reads of {READ} bases); 8 barcodes of {L} bases at the start of "
              f"every R1 read's bases, a third of the reads each with 0, 1 and 2 bases substituted")
        kw = dict(match_line=1, first_byte=b"@", mismatches=1)
        null10 = [os.devnull] * 10
        res = bgzf.classify_records(p1, eight, 4, **kw)
        labels = res.labels()
        assert res.searched == n_reads and (labels[keep] == want[keep]).all(), "the classification is not the generator's"

        def timed(fn):
            def run():
                t = time.perf_counter()
                got = fn()
                return time.perf_counter() - t, got
            return run

        def demux(outs):
            return bgzf.demux(p1, eight, outs[:8], 4, ambiguous=outs[8], unassigned=outs[9], compresslevel=6, **kw)

        def partition(outs):
            return bgzf.partition_records(p2, labels, outs, 4, first_byte=b"@", compresslevel=6)

        def paired(outs1, outs2):
            return bgzf.demux_paired([p1, p2], eight, [outs1[:8], outs2[:8]], 4, ambiguous=[outs1[8], outs2[8]], unassigned=[outs1[9], outs2[9]],
                                     compresslevel=6, **kw)

        legs = [("a demux of R1 to 10 outputs, level 6", timed(lambda: demux(null10))),
                ("b partition_records of R2 to 10 outputs", timed(lambda: partition(null10))),
                ("c b, the unassigned class dropped", timed(lambda: partition(null10[:9] + [None]))),
                ("d demux_paired of R1 and R2", timed(lambda: paired(null10, null10)))]
        warm = [run()[1] for _, run in legs]
        counts = np.bincount(labels, minlength=10)
        assert np.array_equal(warm[0], res.counts) and np.array_equal(res.counts, counts), "a"
        assert np.array_equal(warm[1], np.append(counts, 0)) and np.array_equal(warm[2], np.append(counts, 0)), "b, c"
        assert np.array_equal(warm[3], res.counts), "d"
        # the warm-up of b, c and d once more, to files: every output holds its class's records of its file, whole and in order
        recs1, recs2 = np.frombuffer(text1, np.uint8).reshape(n_reads, REC), np.frombuffer(text2, np.uint8).reshape(n_reads, REC)

        def check(paths, recs, dropped=()):
            for c, p in enumerate(paths):
                if c in dropped:
                    continue
                with open(p, "rb") as f:
                    blob = f.read()
                assert blob.endswith(bgzf.EOF_BLOCK) and gzip.decompress(blob) == recs[labels == c].tobytes(), (p, c)
                os.unlink(p)

        o1, o2 = [os.path.join(d, "r1_%d.gz" % c) for c in range(10)], [os.path.join(d, "r2_%d.gz" % c) for c in range(10)]
        partition(o2)
        check(o2, recs2)
        partition(o2[:9] + [None])
        check(o2, recs2, dropped=(9,))
        paired(o1, o2)
        check(o1, recs1)
        check(o2, recs2)
        print("every leg returns what the generator planted; the files of b, c and d hold each class's records of R2 (and R1), whole and in order")
        del warm, recs1, recs2
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, run) in enumerate(legs):
                times[k].append(run()[0])
        (ma, sa), (mb, sb), (mc, sc), (md, sd) = [report(name, t, n) for (name, _), t in zip(legs, times)]
        fmt = lambda x: f"{x * 1e3:.3f} ms"
        print(f"bar 1: b median {fmt(mb)} against a's median {fmt(ma)}, the larger spread {fmt(max(sa, sb))}: "
              f"{'met' if mb <= ma + max(sa, sb) else 'MISSED'}{' (b below a by more than the spread)' if mb < ma - max(sa, sb) else ''}")
        print(f"bar 2: c median {fmt(mc)} against b's median {fmt(mb)}, the larger spread {fmt(max(sb, sc))}: {'met' if mc < mb - max(sb, sc) else 'MISSED'}")
        print(f"bar 3: d median {fmt(md)} against a + b = {fmt(ma + mb)}, the largest spread {fmt(max(sa, sb, sd))}: "
              f"{'met' if md <= ma + mb + max(sa, sb, sd) else 'MISSED'}")
        ctx.profiling(True)                                    # where the time goes: one profiled run of each leg, by kernel class
        for name, run in legs:
            ctx.kernel_times()
            run()
            kt = ctx.kernel_times()
            print(f"profiled {name}: " + ", ".join(f"{k} {ms:.3f} ms in {cnt} launches" for k, (ms, cnt) in kt.items() if cnt))
        ctx.profiling(False)


if __name__ == "__main__":
    main()

"""BGZF by nearest pattern: timings, in the manner of profiles/time_bgzf_grep_approx.py: a generated FASTQ of
about FILE_MIB (1024) MiB, wall clock around calls that end in a synchronisation, the legs alternated inside one process, RUNS (5) runs
of each behind a warm-up run of each.  Every read begins with one of eight barcodes of 16 bases (read i: barcode i % 8), in turn as it
is, with one base substituted and with two (i // 8 % 3 places).

  a    grep_records(the 8 barcodes, mismatches=1, count=True): the call that exists without this section, the yardstick
  b    classify_records with the same arguments
  c    b with 64 barcodes
  d1   demux to 10 outputs (os.devnull) at level 1
  d6   the same at level 6
  e    eight grep_records calls, one per barcode, each result written through a BgzfWriter at level 6: what a caller did before

Every leg is checked against the generator: a read whose barcode has at most one base substituted is assigned to it at that distance, a
read with two is unassigned -- unless 16 bases further on in the read happen to lie within one substitution of a barcode: those reads are
found by numpy (near_reads of time_bgzf_grep_approx.py on the windows behind a read's first base) and left out of the comparison; the warm-up run of d1
goes to files, which the system gzip decodes and which must be the partition by the classes of b.
Bars: (1) b's median <= 2 x a's median; (2) d6's median < e's median.

    python profiles/time_bgzf_classify.py > profiles/bgzf_classify.txt
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


def barcodes(rng, n, apart=6):
    """n barcodes of L bases, any two at least `apart` places apart"""
    out = []
    while len(out) < n:
        p = ACGT[rng.integers(0, 4, L)]
        if all((p != q).sum() >= apart for q in out):
            out.append(p)
    return [p.tobytes() for p in out]


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, tagged = make_fastq(n_reads)
    rng = np.random.default_rng(23)
    sixty_four = barcodes(rng, 64)
    eight = sixty_four[:8]
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
    # what the generator says, and the reads with a chance window further on: every window that starts behind a read's first base is looked
    # at (the bases moved one column to the left, an A behind them: a few reads too many, never one too few)
    want8 = np.where(subst <= 1, which, -1).astype(np.int16)
    dist8 = np.where(subst <= 1, subst, 255).astype(np.uint8)
    chance = {8: [], 64: []}
    for o in range(0, n_reads, 1 << 18):
        blk = np.empty_like(bases[o:o + (1 << 18)])
        blk[:, :-1], blk[:, -1] = bases[o:o + (1 << 18), 1:], ord("A")
        for nb, pats in ((8, eight), (64, sixty_four)):
            chance[nb] += [o + r for r in near_reads(blk, pats, 1)]
    text = arr.tobytes()
    del arr, bases
    n = len(text)
    print(f"expected classes found on the host in {time.perf_counter() - t:.1f} s; reads within one substitution of a barcode by chance: "
          f"{len(chance[8])} with 8 barcodes, {len(chance[64])} with 64")

    def expect(nb):
        """(pattern, distance) by the generator; the chance reads are left out of the comparison"""
        keep = np.ones(n_reads, bool)
        keep[chance[nb]] = False
        return keep

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq.gz")
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
        del d_in, out
        print(f"file: {nbytes} bytes ({n} bytes of text, {n_reads} reads of {READ} bases); 8 barcodes of {L} bases at the start of every read's bases, "
              f"a third of the reads each with 0, 1 and 2 bases substituted")
        kw = dict(match_line=1, first_byte=b"@", mismatches=1)

        def timed(fn):
            def run():
                t = time.perf_counter()
                got = fn()
                return time.perf_counter() - t, got
            return run

        def demux(level, outs=None):
            outs = outs or [os.devnull] * 10
            return bgzf.demux(path, eight, outs[:8], 4, ambiguous=outs[8], unassigned=outs[9], compresslevel=level, **kw)

        def one_by_one(level):
            total = 0
            for p in eight:
                got = bgzf.grep_records(path, p, 4, **kw)
                with bgzf.BgzfWriter(os.devnull, "wb", level) as w:
                    w.write(got.data)
                total += len(got)
            return total

        legs = [("a grep_records, 8 barcodes, count", timed(lambda: bgzf.grep_records(path, eight, 4, count=True, **kw))),
                ("b classify_records, 8 barcodes", timed(lambda: bgzf.classify_records(path, eight, 4, **kw))),
                ("c classify_records, 64 barcodes", timed(lambda: bgzf.classify_records(path, sixty_four, 4, **kw))),
                ("d1 demux to 10 outputs, level 1", timed(lambda: demux(1))),
                ("d6 demux to 10 outputs, level 6", timed(lambda: demux(6))),
                ("e 8 x grep_records + BgzfWriter, level 6", timed(lambda: one_by_one(6)))]
        warm = [run()[1] for _, run in legs]
        keep8, keep64 = expect(8), expect(64)
        n_near = int((subst <= 1).sum())
        assert n_near <= warm[0] <= n_near + len(chance[8]), ("a", warm[0], n_near)
        for key, got, keep, nb in (("b", warm[1], keep8, 8), ("c", warm[2], keep64, 64)):
            assert got.searched == n_reads and len(got.counts) == nb + 2, key
            assert (got.pattern[keep] == want8[keep]).all() and (got.distance[keep] == dist8[keep]).all(), key
            assert got.counts.sum() == n_reads and abs(int(got.counts[-1]) - int((subst == 2).sum())) <= len(chance[nb]), key
        assert np.array_equal(warm[3], warm[1].counts) and np.array_equal(warm[4], warm[1].counts), "d"
        assert warm[5] >= n_near, "e"
        # the warm-up of d1 once more, to files: every output is the generator's partition (the chance reads aside: by the classes of b)
        outs = [os.path.join(d, "out%d.gz" % c) for c in range(10)]
        assert np.array_equal(demux(1, outs), warm[1].counts)
        cls = np.where(warm[1].pattern >= 0, warm[1].pattern, np.where(warm[1].pattern == bgzf.AMBIGUOUS, 8, 9))
        assert (cls[keep8] == np.where(want8 >= 0, want8, 9)[keep8]).all()
        recs = np.frombuffer(text, np.uint8).reshape(n_reads, REC)
        for c, p in enumerate(outs):
            with open(p, "rb") as f:
                blob = f.read()
            assert blob.endswith(bgzf.EOF_BLOCK) and gzip.decompress(blob) == recs[cls == c].tobytes(), c
            os.unlink(p)
        print("every leg returns what the generator planted; the ten files of d1 hold the generator's partition, whole and in order")
        del warm, recs
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, run) in enumerate(legs):
                times[k].append(run()[0])
        (ma, sa), (mb, sb), (mc, _), (md1, _), (md6, sd6), (me, se) = [report(name, t, n) for (name, _), t in zip(legs, times)]
        print(f"bar 1: b median {mb * 1e3:.3f} ms against 2 x a's median {ma * 1e3:.3f} ms = {2 * ma * 1e3:.3f} ms: {'met' if mb <= 2 * ma else 'MISSED'}")
        print(f"bar 2: d6 median {md6 * 1e3:.3f} ms against e's median {me * 1e3:.3f} ms: {'met' if md6 < me else 'MISSED'}")
        print(f"against a: b {100 * (mb - ma) / ma:+.1f} %, c {100 * (mc - ma) / ma:+.1f} %, d1 {100 * (md1 - ma) / ma:+.1f} %, d6 {100 * (md6 - ma) / ma:+.1f} %, "
              f"e {100 * (me - ma) / ma:+.1f} %")
        ctx.profiling(True)                                    # where the time goes: one profiled run of a and of b, by kernel class
        for name, run in legs[:2]:
            ctx.kernel_times()
            run()
            kt = ctx.kernel_times()
            print(f"profiled {name}: " + ", ".join(f"{k} {ms:.3f} ms in {cnt} launches" for k, (ms, cnt) in kt.items() if cnt))
        ctx.profiling(False)


if __name__ == "__main__":
    main()

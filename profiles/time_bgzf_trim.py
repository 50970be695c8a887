"""BGZF trimmed: timings, in the manner of profiles/time_bgzf_partition.py: the generated FASTQ of about
FILE_MIB (1024) MiB of profiles/time_bgzf_grep_records.py (reads of 150 bases, qualities drawn evenly from 2 .. 40), in which every
third read is given one of three adapters of 20 bases at column 100 + r % 50, so that a fifth of them run over the read's end; wall
clock around calls that end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of
each.  Every output goes to os.devnull at level 6.

  a    partition_records with one class: the records whole -- code this section does not touch, the yardstick
  b    trim_records with nothing to cut
  c    trim_records with quality=(0, 20)
  d    c with the three adapters, mismatches=2, min_length=20
  e    d with output=None: judged and counted only

Checked: the warm-up of b goes to a file, which the system gzip decodes and which must be the input; d ends every read with a planted adapter at the
adapter's column or in front of it (a cut by quality or a chance match may come first; two bytes of an adapter that quality left are
below min_overlap and stay), judges every read, and e returns d's arrays.
No bar: nobody has measured this path.  What is printed is every leg's ratio to a, and a's own spread.

    python profiles/time_bgzf_trim.py > profiles/bgzf_trim.txt
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
from zlib_ng_amd import _lib, bgzf, zlib_ng  # noqa: E402
from time_bgzf_rw import RUNS, report  # noqa: E402
from time_bgzf_grep_records import HEAD, READ, REC, make_fastq  # noqa: E402
from time_bgzf_partition import write_bgzf  # noqa: E402

ADAPTERS = [b"AGATCGGAAGAGCACACGTC", b"CTGTCTCTTATACACATCTC", b"TGGAATTCTCGGGTGCCAAG"]


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, _ = make_fastq(n_reads)
    planted = np.arange(0, n_reads, 3)
    col = 100 + planted % 50
    table = np.array([np.frombuffer(a, np.uint8) for a in ADAPTERS])
    for j in range(20):                                        # byte j of the adapter, where the read still has room for it
        rows = planted[col + j < READ]
        arr[rows, HEAD + 100 + rows % 50 + j] = table[rows // 3 % 3, j]
    text = arr.tobytes()
    del arr
    n = len(text)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq.gz")
        nb = write_bgzf(ctx, text, path)
        print(f"file: {nb} bytes ({n} bytes of text, {n_reads} reads of {READ} bases); every third read holds one of 3 adapters of 20 bases at column "
              f"100 + r % 50")
        labels = np.zeros(n_reads, np.int32)
        kw = dict(first_byte=b"@", compresslevel=6)
        full = dict(quality=(0, 20), adapters=ADAPTERS, mismatches=2, min_length=20)

        def timed(fn):
            def run():
                t = time.perf_counter()
                got = fn()
                return time.perf_counter() - t, got
            return run

        legs = [("a partition_records, one class", timed(lambda: bgzf.partition_records(path, labels, [os.devnull], 4, **kw))),
                ("b trim_records, nothing to cut", timed(lambda: bgzf.trim_records(path, os.devnull, **kw))),
                ("c trim_records, quality=(0, 20)", timed(lambda: bgzf.trim_records(path, os.devnull, quality=(0, 20), **kw))),
                ("d c + 3 adapters, k=2, min_length=20", timed(lambda: bgzf.trim_records(path, os.devnull, **full, **kw))),
                ("e d, counted only", timed(lambda: bgzf.trim_records(path, None, first_byte=b"@", **full)))]
        warm = [run()[1] for _, run in legs]
        assert warm[0].tolist() == [n_reads, 0], "a"
        b, c, dd, e = warm[1:]
        assert (b.records, b.kept, b.bases_out) == (n_reads, n_reads, n_reads * READ) and not b.steps.any(), "b"
        assert c.records == n_reads and c.quality_trimmed > 0 and c.adapter_trimmed == 0, "c"
        assert dd.kept + dd.too_short == n_reads and (dd.end[planted] <= col + 2).all() and int(dd.adapter_counts.sum()) >= len(planted) // 2, "d"
        for name in ("begin", "end", "adapter", "verdict", "steps", "adapter_counts"):
            assert np.array_equal(getattr(dd, name), getattr(e, name)), ("e", name)
        out = os.path.join(d, "same.gz")
        bgzf.trim_records(path, out, **kw)
        with open(out, "rb") as f:
            blob = f.read()
        assert blob.endswith(bgzf.EOF_BLOCK) and gzip.decompress(blob) == text, "b's file is not the input"
        os.unlink(out)
        print(f"b writes the input; d cut {int(dd.adapter_counts.sum())} reads at an adapter ({dd.adapter_counts.tolist()}), took {dd.quality_trimmed} bases by "
              f"quality and {dd.adapter_trimmed} by adapter, kept {dd.kept} reads and found {dd.too_short} too short; e returns d's arrays")
        del warm, b, c, dd, e, blob
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, run) in enumerate(legs):
                times[k].append(run()[0])
        stats = [report(name, t, n) for (name, _), t in zip(legs, times)]
        ma, sa = stats[0]
        print(f"the yardstick a: median {ma * 1e3:.3f} ms, run-to-run spread {sa * 1e3:.3f} ms ({100 * sa / ma:.1f} % of the median)")
        for (name, _), (m, s) in zip(legs[1:], stats[1:]):
            print(f"{name[:1]} / a = {m / ma:.3f} (median {m * 1e3:.3f} ms, spread {s * 1e3:.3f} ms)")
        ctx.profiling(True)                                    # where the time goes: one profiled run of each leg, by kernel class
        for name, run in legs:
            ctx.kernel_times()
            run()
            kt = ctx.kernel_times()
            print(f"profiled {name}: " + ", ".join(f"{k} {ms:.3f} ms in {cnt} launches" for k, (ms, cnt) in kt.items() if cnt))
        ctx.profiling(False)


if __name__ == "__main__":
    main()

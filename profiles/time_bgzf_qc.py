"""BGZF quality control: timings, in the manner of profiles/time_bgzf_trim.py: the generated FASTQ of about
FILE_MIB (1024) MiB of profiles/time_bgzf_grep_records.py (reads of 150 bases, qualities drawn evenly from 2 .. 40); wall clock around
calls that end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.

  a    trim_records(output=None) with nothing to cut: the code in front of this section, which reads the same lines behind the same
       prologue -- the yardstick
  b    qc_records at cycles=512
  c    b with per_record=True
  d    b at cycles=4096

Checked: b counts every read and every base, its per-cycle rows add up to the reads, its quality sum is numpy's on the text; c returns
b's tables and a row per read; d's tables are b's with more empty rows.
No bar: nobody has measured this path.  What is printed is every leg's ratio to a, and a's own spread.

    python profiles/time_bgzf_qc.py > profiles/bgzf_qc.txt
"""
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


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, _ = make_fastq(n_reads)
    qual0 = HEAD + READ + 3                                    # where a record's qualities begin: behind the bases, "\n+\n"
    qsum = int(arr[:, qual0:qual0 + READ].sum(dtype=np.int64)) - 33 * n_reads * READ
    seq = arr[:, HEAD:HEAD + READ]
    gc = int(np.count_nonzero(seq == ord("C")) + np.count_nonzero(seq == ord("G")))
    del seq
    text = arr.tobytes()
    del arr
    n = len(text)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq.gz")
        nb = write_bgzf(ctx, text, path)
        print(f"file: {nb} bytes ({n} bytes of text, {n_reads} reads of {READ} bases)")
        del text

        def timed(fn):
            def run():
                t = time.perf_counter()
                got = fn()
                return time.perf_counter() - t, got
            return run

        legs = [("a trim_records, nothing to cut, counted only", timed(lambda: bgzf.trim_records(path, None, first_byte=b"@"))),
                ("b qc_records, cycles=512", timed(lambda: bgzf.qc_records(path, first_byte=b"@"))),
                ("c b, per_record=True", timed(lambda: bgzf.qc_records(path, first_byte=b"@", per_record=True))),
                ("d b, cycles=4096", timed(lambda: bgzf.qc_records(path, first_byte=b"@", cycles=4096)))]
        warm = [run()[1] for _, run in legs]
        a, b, c, dd = warm
        assert (a.records, a.kept, a.bases_out) == (n_reads, n_reads, n_reads * READ), "a"
        assert (b.records, b.bases, b.min_len, b.max_len, b.bytes_in) == (n_reads, n_reads * READ, READ, READ, n), "b"
        assert (b.base_pos[:READ].sum(axis=1) == n_reads).all() and (b.qual_pos[:READ].sum(axis=1) == n_reads).all() and not b.base_pos[READ:].any(), "b rows"
        assert b.quality_sum == qsum and int(b.base_total[1] + b.base_total[2]) == gc and b.quality_clamped == 0 and int(b.length_hist[READ]) == n_reads, "b sums"
        assert np.array_equal(c._tables, b._tables) and (c.length == READ).all() and int(c.quality_sum_per_record.sum()) == qsum and int(c.gc.sum()) == gc, "c"
        assert np.array_equal(dd.base_pos[:513], b.base_pos) and np.array_equal(dd.qual_pos[:513], b.qual_pos) and not dd.base_pos[513:].any(), "d"
        print(f"b: {b!r}; mean quality at cycle 0 {b.mean_quality_by_cycle()[0]:.2f}; c returns b's tables and {len(c.length)} rows; d's rows are b's")
        del warm, a, b, c, dd
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

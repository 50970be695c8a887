"""BGZF k-mer count: timings, in the manner of profiles/time_bgzf_screen.py: the generated FASTQ of about
FILE_MIB (1024) MiB of profiles/time_bgzf_grep_records.py (reads of 150 random bases); wall clock around calls that end in a
synchronisation, the legs of a step alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  Every step that
uses the GPU is a child process under a time limit of its own, and the steps are chained: one that fails or runs out of time ends the
script.

  make   the file is written, and beside it the worst case: the same number of reads, all of them the file's first read
  a      k = 31, canonical.  key_records -- the yardstick: the existing call that decodes the file and reads every base of every read
         once; count-only screen_records against a PhiX-sized random reference -- the same code extraction with a read-only probe;
         count_kmers(min_count=None) -- the spectrum only, no pair leaves the device; count_kmers(min_count=2) -- the pairs that occur
         twice come back.  The ratio of interest is a3 / a2: count-only counting against count-only screening
  b      the worst case: count_kmers(min_count=None) over the file of identical reads (amplicons), where every wave's atomics go to the
         same 120 slots and the run combine does not help, against the same call over the random file

Checked: the reads are random, so (almost) every 31-mer is new: kmers is 120 per read and distinct is within a thousandth of it; the
spectrum sums to distinct; in b distinct is 120 and every count is the number of reads.
No bar: nobody has measured this path.  The ratios are reported.

    python profiles/time_bgzf_kcount.py > profiles/bgzf_kcount.txt
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from time_bgzf_dedup import measure, profiled, timed      # noqa: E402

LIMITS = {"make": 420, "a": 560, "b": 420}      # seconds, each step's own
K = 31
PHIX = 5386


def repeat_path(path):
    return os.path.join(os.path.dirname(path), "repeat.fastq.gz")


def step_make(path):
    from zlib_ng_amd import zlib_ng
    from time_bgzf_grep_records import READ, REC, make_fastq
    from time_bgzf_partition import write_bgzf
    ctx = zlib_ng._ctx()
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, _ = make_fastq(n_reads)
    text = arr.tobytes()
    del arr
    nb = write_bgzf(ctx, text, path)
    print(f"file: {nb} bytes ({len(text)} bytes of text, {n_reads} reads of {READ} bases)")
    text = text[:REC] * n_reads
    nb = write_bgzf(ctx, text, repeat_path(path))
    print(f"worst case: {nb} bytes ({len(text)} bytes of text, {n_reads} copies of the first read)")


def sizes():
    from time_bgzf_grep_records import READ, REC
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    return n_reads, READ, n_reads * REC


def step_a(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads, read, n = sizes()
    ref = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(11).integers(0, 4, PHIX)].tobytes()
    small = bgzf.KmerSet.build([ref], K, names=["PhiX-sized"])
    legs = [("a1 key_records", timed(lambda: bgzf.key_records(path, first_byte=b"@"))),
            ("a2 screen_records, k = 31, PhiX-sized set", timed(lambda: bgzf.screen_records(path, small, first_byte=b"@"))),
            ("a3 count_kmers, k = 31, min_count=None", timed(lambda: bgzf.count_kmers(path, K, min_count=None, first_byte=b"@"))),
            ("a4 count_kmers, k = 31, min_count=2", timed(lambda: bgzf.count_kmers(path, K, min_count=2, first_byte=b"@")))]
    key, s, c0, c2 = [run()[1] for _, run in legs]
    kmers = n_reads * (read - K + 1)
    assert (key.records, key.bases) == (n_reads, n_reads * read), "a1"
    assert (s.records, int(s.kmers.sum())) == (n_reads, kmers), "a2"
    for res, what in ((c0, "a3"), (c2, "a4")):
        assert (res.records, res.bases, res.kmers) == (n_reads, n_reads * read, kmers), what
        assert kmers - kmers // 1000 <= res.distinct <= kmers and int(res.spectrum.sum()) == res.distinct, what
        print(f"{what}: {res.distinct} codes of {res.kmers} k-mers, {len(res)} pairs came back; spectrum[1:4] = {res.spectrum[1:4].tolist()}")
    assert len(c0) == 0 and len(c2) == int(c2.spectrum[2:].sum())
    del key, s, c0, c2
    (mk, sk), (ms, ss), (m0, s0), (m2, s2) = measure(legs, n, RUNS)
    print(f"the yardstick a1: median {mk * 1e3:.3f} ms, run-to-run spread {sk * 1e3:.3f} ms ({100 * sk / mk:.1f} % of the median)")
    print(f"a2 / a1 = {ms / mk:.3f} (median {ms * 1e3:.3f} ms, spread {ss * 1e3:.3f} ms)")
    print(f"a3 / a1 = {m0 / mk:.3f} (median {m0 * 1e3:.3f} ms, spread {s0 * 1e3:.3f} ms)")
    print(f"a4 / a1 = {m2 / mk:.3f} (median {m2 * 1e3:.3f} ms, spread {s2 * 1e3:.3f} ms)")
    print(f"a3 / a2 = {m0 / ms:.3f}: count-only counting against count-only screening")
    profiled(ctx, legs)


def step_b(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads, read, n = sizes()
    legs = [("b1 count_kmers, k = 31, min_count=None, random reads", timed(lambda: bgzf.count_kmers(path, K, min_count=None, first_byte=b"@"))),
            ("b2 count_kmers, k = 31, min_count=None, one read repeated", timed(lambda: bgzf.count_kmers(repeat_path(path), K, min_count=None, first_byte=b"@")))]
    rnd, rep = [run()[1] for _, run in legs]
    assert (rep.records, rep.kmers, rep.distinct) == (n_reads, n_reads * (read - K + 1), read - K + 1), "b2"
    assert int(rep.spectrum[-1]) == rep.distinct and rnd.records == n_reads, "b2: every count is the number of reads"
    del rnd, rep
    (m1, s1), (m2, s2) = measure(legs, n, RUNS)
    print(f"b1: median {m1 * 1e3:.3f} ms, run-to-run spread {s1 * 1e3:.3f} ms ({100 * s1 / m1:.1f} % of the median)")
    print(f"b2 / b1 = {m2 / m1:.3f} (median {m2 * 1e3:.3f} ms, spread {s2 * 1e3:.3f} ms)")
    profiled(ctx, legs)


def main():
    if len(sys.argv) == 3:
        {"make": step_make, "a": step_a, "b": step_b}[sys.argv[1]](sys.argv[2])
        return
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq.gz")
        for step in ("make", "a", "b"):
            print(f"---- step {step} (time limit {LIMITS[step]} s)", flush=True)
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), step, path])
            if r.returncode:
                print(f"step {step} ended with status {r.returncode}: the script ends here", flush=True)
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()

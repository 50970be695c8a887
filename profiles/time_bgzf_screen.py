"""BGZF contaminant screen: timings, in the manner of profiles/time_bgzf_dedup.py: the generated FASTQ of
about FILE_MIB (1024) MiB of profiles/time_bgzf_grep_records.py (reads of 150 random bases); wall clock around calls that end in a
synchronisation, the legs of a step alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  Every step that
uses the GPU is a child process under a time limit of its own, and the steps are chained: one that fails or runs out of time ends the
script.

  make   the file is written
  a      count only: screen_records at k = 31 against a PhiX-sized random reference (5 386 bases) and against a random reference of
         5 Mb, with key_records over the same file as the yardstick -- the existing call that decodes the file and reads every base of
         every read once; the ratios, the time to build each set, and the kernel time by class from one profiled run of each
  b      end to end: screen_filter to one output at level 6 against partition_records of the same file with one class to one output at
         level 6 -- the second pass alone, the floor

Checked: the reads are random, so (almost) none holds a 31-mer of a random reference: a's kmers are 120 per read, its hits at most a
handful; b's output is byte for byte the file partition_records writes when no read is matched.
No bar: nobody has measured this path.  The ratios are reported.

    python profiles/time_bgzf_screen.py > profiles/bgzf_screen.txt
"""
import filecmp
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from time_bgzf_dedup import measure, profiled, step_make, timed      # noqa: E402

LIMITS = {"make": 300, "a": 420, "b": 420}      # seconds, each step's own
K = 31
PHIX, GENOME = 5386, 5_000_000


def reference(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def build_sets():
    from zlib_ng_amd import bgzf
    sets = []
    for name, n, seed in (("PhiX-sized", PHIX, 11), ("5 Mb", GENOME, 12)):
        ref = reference(n, seed)
        t = time.perf_counter()
        kset = bgzf.KmerSet.build([ref], K, names=[name])
        dt = time.perf_counter() - t
        assert n - K + 1 - 8 <= len(kset) <= n - K + 1, name
        print(f"set {name}: {n} bases, {len(kset)} codes, built and exported in {dt * 1e3:.1f} ms")
        sets.append(kset)
    return sets


def step_a(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS
    from time_bgzf_grep_records import READ, REC
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    n = n_reads * REC
    small, big = build_sets()
    legs = [("a1 key_records", timed(lambda: bgzf.key_records(path, first_byte=b"@"))),
            ("a2 screen_records, k = 31, PhiX-sized set", timed(lambda: bgzf.screen_records(path, small, first_byte=b"@"))),
            ("a3 screen_records, k = 31, 5 Mb set", timed(lambda: bgzf.screen_records(path, big, first_byte=b"@")))]
    key, s, b = [run()[1] for _, run in legs]
    assert (key.records, key.bases) == (n_reads, n_reads * READ), "a1"
    for res, what in ((s, "a2"), (b, "a3")):
        assert (res.records, res.bases, int(res.kmers.sum())) == (n_reads, n_reads * READ, n_reads * (READ - K + 1)), what
        print(f"{what}: {int(res.hits.sum())} hit positions in {res.matched_records} reads")
    assert s.matched_records == 0 and b.matched_records < 100
    del key, s, b
    (mk, sk), (ms, ss), (mb, sb) = measure(legs, n, RUNS)
    print(f"the yardstick a1: median {mk * 1e3:.3f} ms, run-to-run spread {sk * 1e3:.3f} ms ({100 * sk / mk:.1f} % of the median)")
    print(f"a2 / a1 = {ms / mk:.3f} (median {ms * 1e3:.3f} ms, spread {ss * 1e3:.3f} ms)")
    print(f"a3 / a1 = {mb / mk:.3f} (median {mb * 1e3:.3f} ms, spread {sb * 1e3:.3f} ms)")
    profiled(ctx, legs)


def step_b(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS
    from time_bgzf_grep_records import REC
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    n = n_reads * REC
    small = build_sets()[0]
    d = os.path.dirname(path)
    out_p, out_s = os.path.join(d, "part.gz"), os.path.join(d, "screen.gz")
    labels = np.zeros(n_reads, np.int64)
    legs = [("b1 partition_records, one class, level 6", timed(lambda: bgzf.partition_records(path, labels, [out_p], first_byte=b"@", compresslevel=6))),
            ("b2 screen_filter, PhiX-sized set, one output, level 6", timed(lambda: bgzf.screen_filter(path, small, out_s, first_byte=b"@", compresslevel=6)))]
    counts, res = [run()[1] for _, run in legs]
    assert counts.tolist() == [n_reads, 0] and (res.records, res.matched_records) == (n_reads, 0), "b"
    assert filecmp.cmp(out_p, out_s, shallow=False), "no read is matched: the two outputs are the same file"
    print(f"outputs: {os.path.getsize(out_s)} bytes each")
    (mp, sp), (ms, ss) = measure(legs, n, RUNS)
    print(f"the floor b1: median {mp * 1e3:.3f} ms, run-to-run spread {sp * 1e3:.3f} ms ({100 * sp / mp:.1f} % of the median)")
    print(f"b2 / b1 = {ms / mp:.3f} (median {ms * 1e3:.3f} ms, spread {ss * 1e3:.3f} ms); b2 - b1 = {(ms - mp) * 1e3:.3f} ms")
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

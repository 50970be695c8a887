"""BGZF duplicate removal: timings, in the manner of profiles/time_bgzf_qc.py: the generated FASTQ of about
FILE_MIB (1024) MiB of profiles/time_bgzf_grep_records.py (reads of 150 random bases, so every read is distinct); wall clock around
calls that end in a synchronisation, the legs of a step alternated inside one process, RUNS (5) runs of each behind a warm-up run of
each.  Every step that uses the GPU is a child process under a time limit of its own, and the steps are chained: one that fails or
runs out of time ends the script.

  make   the file is written
  a      the key pass: key_records against qc_records (no rows) on the same file, both from the same process; the ratio, and the
         kernel time by class from one profiled run of each
  b      the resolve: dedup_keys on the file's own keys -- all distinct; with 30 % of the records made copies of others;
         with 5 % of the records sharing one sequence (the hot slot) -- against
         np.unique(keys, return_index=True, return_counts=True) on the host, what a caller would do today (3 runs: it is slow)
  c      end to end: dedup_records to one output at level 6 against partition_records of the same file with one class to one output at
         level 6 -- the second pass alone, the floor

Checked: a's keys are one per read and all distinct, its bases are the file's; every result of b is np.unique's (the first records,
the counts, the totals); c's output is byte for byte the file partition_records writes.
No bar: nobody has measured this path.

    python profiles/time_bgzf_dedup.py > profiles/bgzf_dedup.txt
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

LIMITS = {"make": 300, "a": 300, "b": 420, "c": 420}      # seconds, each step's own


def timed(fn):
    def run():
        t = time.perf_counter()
        got = fn()
        return time.perf_counter() - t, got
    return run


def measure(legs, nbytes, runs):
    """the legs alternated, `runs` runs of each behind the warm-up the caller made -> [(median, spread)]"""
    from time_bgzf_rw import report
    times = [[] for _ in legs]
    for _ in range(runs):
        for k, (_, run) in enumerate(legs):
            times[k].append(run()[0])
    return [report(name, t, nbytes) for (name, _), t in zip(legs, times)]


def profiled(ctx, legs):
    ctx.profiling(True)                                    # where the time goes: one profiled run of each leg, by kernel class
    for name, run in legs:
        ctx.kernel_times()
        run()
        kt = ctx.kernel_times()
        print(f"profiled {name}: " + ", ".join(f"{k} {ms:.3f} ms in {cnt} launches" for k, (ms, cnt) in kt.items() if cnt))
    ctx.profiling(False)


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


def step_a(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS
    from time_bgzf_grep_records import READ, REC
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    n = n_reads * REC
    legs = [("a1 qc_records, cycles=512, no rows", timed(lambda: bgzf.qc_records(path, first_byte=b"@"))),
            ("a2 key_records", timed(lambda: bgzf.key_records(path, first_byte=b"@"))),
            ("a3 a2, canonical=True, ignore_case=True", timed(lambda: bgzf.key_records(path, first_byte=b"@", canonical=True, ignore_case=True)))]
    q, k, kc = [run()[1] for _, run in legs]
    assert (q.records, q.bases) == (n_reads, n_reads * READ), "a1"
    assert (k.records, k.bases, kc.records) == (n_reads, n_reads * READ, n_reads), "a2"
    assert len(np.unique(k.keys)) == n_reads and len(np.unique(kc.keys)) == n_reads, "the reads are distinct and so are their keys"
    del q, k, kc
    stats = measure(legs, n, RUNS)
    (mq, sq), (mk, sk), (mc, sc) = stats
    print(f"the yardstick a1: median {mq * 1e3:.3f} ms, run-to-run spread {sq * 1e3:.3f} ms ({100 * sq / mq:.1f} % of the median)")
    print(f"a2 / a1 = {mk / mq:.3f} (median {mk * 1e3:.3f} ms, spread {sk * 1e3:.3f} ms)")
    print(f"a3 / a1 = {mc / mq:.3f} (median {mc * 1e3:.3f} ms, spread {sc * 1e3:.3f} ms)")
    profiled(ctx, legs)


def same_as_unique(res, keys, what):
    """np.unique's answer for the same array, timed; the GPU's is compared with it"""
    t = time.perf_counter()
    _, index, counts = np.unique(keys, return_index=True, return_counts=True)
    dt = time.perf_counter() - t
    order = np.argsort(index)
    heads = np.nonzero(res.count)[0]
    assert np.array_equal(index[order], heads) and np.array_equal(counts[order], res.count[heads]), what
    assert (res.unique, res.duplicates, res.max_count) == (len(index), len(keys) - len(index), int(counts.max())), what
    assert np.array_equal(res.first[heads], heads) and int(res.count.sum()) == len(keys), what
    return dt


def step_b(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS, report
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    keys = bgzf.key_records(path, first_byte=b"@").keys
    n = len(keys)
    rng = np.random.default_rng(3)
    third = keys.copy()                                     # 30 % of the records become copies of others
    at = rng.choice(n, size=3 * n // 10, replace=False)
    rest = np.setdiff1d(np.arange(n), at)
    third[at] = keys[rest[rng.integers(0, len(rest), len(at))]]
    hot = keys.copy()                                       # 5 % of the records share one sequence
    hot[rng.choice(n, size=n // 20, replace=False)] = keys[n // 2]
    cases = [("b1 all distinct", keys), ("b2 30 % duplicates", third), ("b3 5 % share one sequence", hot)]
    print(f"{n} keys; the table has {1 << (2 * n - 1).bit_length()} slots, {_lib.load().zngamd_dedup_scratch_bytes(n)} bytes")
    legs = [(name + ", dedup_keys", timed(lambda k=k: bgzf.dedup_keys(k))) for name, k in cases]
    legs.append(("b1 all distinct, totals only", timed(lambda: ctx.dedup_keys(keys, False, False))))
    host = []
    for (name, k), (_, run) in zip(cases, legs):            # the warm-up run of each is the checked one
        res = run()[1]
        host.append([same_as_unique(res, k, name)])
        print(f"{name}: {res!r}")
    assert legs[3][1]()[1][0].unique == n
    stats = measure(legs, None, RUNS)
    for (name, k), h in zip(cases, host):
        for _ in range(2):
            t = time.perf_counter()
            np.unique(k, return_index=True, return_counts=True)
            h.append(time.perf_counter() - t)
    hstats = [report(name + ", np.unique on the host", h) for (name, _), h in zip(cases, host)]
    for (name, _), (m, s), (hm, hs) in zip(cases, stats, hstats):
        print(f"{name[:2]}: dedup_keys {m * 1e3:.3f} ms ({n / m / 1e6:.1f} M keys/s), np.unique {hm * 1e3:.1f} ms: {hm / m:.1f} x; against b1 {m / stats[0][0]:.3f}")
    profiled(ctx, legs)


def step_c(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_rw import RUNS
    from time_bgzf_grep_records import REC
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    n = n_reads * REC
    d = os.path.dirname(path)
    out_p, out_d = os.path.join(d, "part.gz"), os.path.join(d, "dedup.gz")
    labels = np.zeros(n_reads, np.int64)
    legs = [("c1 partition_records, one class, level 6", timed(lambda: bgzf.partition_records(path, labels, [out_p], first_byte=b"@", compresslevel=6))),
            ("c2 dedup_records, one output, level 6", timed(lambda: bgzf.dedup_records(path, out_d, first_byte=b"@", compresslevel=6))),
            ("c3 dedup_records, output=None", timed(lambda: bgzf.dedup_records(path, None, first_byte=b"@")))]
    counts, res, counted = [run()[1] for _, run in legs]
    assert counts.tolist() == [n_reads, 0] and (res.unique, res.duplicates) == (n_reads, 0) and counted.unique == n_reads, "c"
    assert filecmp.cmp(out_p, out_d, shallow=False), "every read is kept: the two outputs are the same file"
    print(f"outputs: {os.path.getsize(out_d)} bytes each")
    (mp, sp), (md, sd), (mc, sc) = measure(legs, n, RUNS)
    print(f"the floor c1: median {mp * 1e3:.3f} ms, run-to-run spread {sp * 1e3:.3f} ms ({100 * sp / mp:.1f} % of the median)")
    print(f"c2 / c1 = {md / mp:.3f} (median {md * 1e3:.3f} ms, spread {sd * 1e3:.3f} ms); c2 - c1 = {(md - mp) * 1e3:.3f} ms; c3 = {mc * 1e3:.3f} ms")
    profiled(ctx, legs)


def main():
    if len(sys.argv) == 3:
        {"make": step_make, "a": step_a, "b": step_b, "c": step_c}[sys.argv[1]](sys.argv[2])
        return
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq.gz")
        for step in ("make", "a", "b", "c"):
            print(f"---- step {step} (time limit {LIMITS[step]} s)", flush=True)
            r = subprocess.run(["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), step, path])
            if r.returncode:
                print(f"step {step} ended with status {r.returncode}: the script ends here", flush=True)
                sys.exit(r.returncode)


if __name__ == "__main__":
    main()

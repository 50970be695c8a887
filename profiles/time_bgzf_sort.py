"""BGZF sort: timings, in the manner of profiles/time_bgzf_dedup.py: the generated FASTQ of about FILE_MIB (1024)
MiB of profiles/time_bgzf_grep_records.py (reads of 150 random bases under names that count up); wall clock around calls that end in a
synchronisation, the legs of a step alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  Every step that
uses the GPU is a child process under a time limit of its own, and the steps are chained: one that fails or runs out of time ends the
script.  Device buffers are devmem's; no torch.

  make   the file is written
  a      the sort alone: sort_keys on the file's own rows -- a1 the first 32 bases of every read (32 bytes vary: 32 passes), a2 the names
         in shuffled order (64 bytes wide, 8 vary: 8 passes), a3 the lengths (nothing varies: no pass) -- against np.lexsort over the
         big-endian 64-bit columns of the same rows on the host, what a caller would do today (3 runs: it is slow)
  b      end to end: sort_records by the first 32 bases to one output at level 6 against partition_records of the same file with one class
         to one output at level 6 -- the existing call that decodes, gathers and writes the same bytes; and the key pass alone

Checked: every order of a is np.lexsort's; b's output holds the input's records, each once, in the order of a1.
No bar: nobody has measured this path.

    python profiles/time_bgzf_sort.py > profiles/bgzf_sort.txt
"""
import gzip
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))

LIMITS = {"make": 300, "a": 420, "b": 540}      # seconds, each step's own


def lexorder(rows):
    cols = rows.view(">u8").astype(np.uint64)
    return np.lexsort(cols.T[::-1])


def bases32():
    from zlib_ng_amd import bgzf
    return [bgzf.SortKey(1, width=32, truncate=True)]


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
    from time_bgzf_dedup import measure, profiled, timed
    from time_bgzf_rw import RUNS, report
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    rng = np.random.default_rng(3)
    seq = bgzf.sort_key_records(path, bases32(), first_byte=b"@").keys
    names = bgzf.sort_key_records(path, "name", first_byte=b"@").keys
    names = np.ascontiguousarray(names[rng.permutation(len(names))])
    lens = bgzf.sort_key_records(path, "length", first_byte=b"@").keys
    cases = [("a1 32 bases, W 32", seq), ("a2 names shuffled, W 64", names), ("a3 lengths, W 8", lens)]
    n = len(seq)
    for name, k in cases:
        varying = int((k.min(axis=0) != k.max(axis=0)).sum())
        print(f"{name}: {n} rows, {varying} byte positions vary, work area {_lib.load().zngamd_sort_scratch_bytes(n, k.shape[1])} bytes")
    legs = [(name + ", sort_keys", timed(lambda k=k: bgzf.sort_keys(k))) for name, k in cases]
    legs.append(("a1 with rank", timed(lambda: bgzf.sort_keys(seq, rank=True))))
    host = []
    for (name, k), (_, run) in zip(cases, legs):            # the warm-up run of each is the checked one
        got = run()[1]
        t = time.perf_counter()
        want = lexorder(k)
        host.append([time.perf_counter() - t])
        assert np.array_equal(got, want), name
    legs[3][1]()
    stats = measure(legs, None, RUNS)
    for (name, k), h in zip(cases, host):
        for _ in range(2):
            t = time.perf_counter()
            lexorder(k)
            h.append(time.perf_counter() - t)
    hstats = [report(name + ", np.lexsort on the host", h) for (name, _), h in zip(cases, host)]
    for (name, _), (m, s), (hm, hs) in zip(cases, stats, hstats):
        print(f"{name[:2]}: sort_keys {m * 1e3:.3f} ms ({n / m / 1e6:.1f} M rows/s), np.lexsort {hm * 1e3:.1f} ms: {hm / m:.1f} x")
    profiled(ctx, legs)


def step_b(path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    from time_bgzf_dedup import measure, profiled, timed
    from time_bgzf_rw import RUNS
    from time_bgzf_grep_records import REC
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    n = n_reads * REC
    d = os.path.dirname(path)
    out_p, out_s = os.path.join(d, "part.gz"), os.path.join(d, "sorted.gz")
    labels = np.zeros(n_reads, np.int64)
    legs = [("b1 partition_records, one class, level 6", timed(lambda: bgzf.partition_records(path, labels, [out_p], first_byte=b"@", compresslevel=6))),
            ("b2 sort_records by 32 bases, level 6", timed(lambda: bgzf.sort_records(path, out_s, bases32(), first_byte=b"@", compresslevel=6))),
            ("b3 sort_key_records by 32 bases", timed(lambda: bgzf.sort_key_records(path, bases32(), first_byte=b"@")))]
    counts, res, keys = [run()[1] for _, run in legs]
    assert counts.tolist() == [n_reads, 0] and (res.records, res.bytes, res.key_width) == (n_reads, n, 32) and keys.records == n_reads, "b"
    assert np.array_equal(res.order, lexorder(keys.keys)), "the order is np.lexsort's"
    with gzip.open(path, "rb") as f:
        a = np.frombuffer(f.read(), np.uint8).reshape(n_reads, REC)
    with gzip.open(out_s, "rb") as f:
        b = np.frombuffer(f.read(), np.uint8).reshape(n_reads, REC)
    assert np.array_equal(b, a[res.order]), "the output is the input's records in that order"
    del a, b
    print(f"outputs: {os.path.getsize(out_p)} and {os.path.getsize(out_s)} bytes")
    (mp, sp), (ms, ss), (mk, sk) = measure(legs, n, RUNS)
    print(f"the yardstick b1: median {mp * 1e3:.3f} ms, run-to-run spread {sp * 1e3:.3f} ms ({100 * sp / mp:.1f} % of the median)")
    print(f"b2 / b1 = {ms / mp:.3f} (median {ms * 1e3:.3f} ms, spread {ss * 1e3:.3f} ms); b2 - b1 = {(ms - mp) * 1e3:.3f} ms; b3 = {mk * 1e3:.3f} ms")
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

"""BGZF overlap: timings, in the manner of profiles/time_bgzf_trim.py: the generated FASTQ of about FILE_MIB
(1024) MiB of profiles/time_bgzf_grep_records.py (reads of 150 bases, qualities drawn evenly from 2 .. 40) written as interleaved
pairs: read 2 i is mate 1 of pair i, and read 2 i + 1 is given the reverse complement of the last 150 bases of a fragment of 160 + i %
140 bases that begins with mate 1 and goes on with the read's own bases -- overlaps of 140 down to 1 bases, of which those of 30 and
more are found.  Wall clock around calls that end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each
behind a warm-up run of each.  Every output goes to os.devnull at level 6.

  a    trim_records(record_lines=8) with nothing to cut, counted only -- code this section does not touch, the yardstick
  b    overlap_records, counted only
  c    overlap_records, the merged reads to one output
  d    c with the unmerged pairs to a second output

Checked: b finds the planted insert in every pair whose overlap has 30 bases and more and nothing in the others; c and d return b's
arrays; the warm-up of d goes to two files which the system gzip decodes: the merged reads are the fragments, the unmerged pairs the
input's.
No bar: nobody has measured this path.  What is printed is every leg's ratio to a, and a's own spread.

    python profiles/time_bgzf_overlap.py > profiles/bgzf_overlap.txt
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

SPAN, SHORTEST = 140, 160                                    # insert = SHORTEST + i % SPAN
COMP = np.arange(256, dtype=np.uint8)
COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


def make_pairs(n_pairs):
    """-> (uint8[2 n_pairs, REC], the planted insert of every pair)"""
    arr, _ = make_fastq(2 * n_pairs)
    insert = SHORTEST + np.arange(n_pairs, dtype=np.int64) % SPAN
    seq = arr[:, HEAD:HEAD + READ]
    for ins in range(SHORTEST, SHORTEST + SPAN):
        rows = np.nonzero(insert == ins)[0]
        frag = np.concatenate([seq[2 * rows], seq[2 * rows + 1]], axis=1)[:, ins - READ:ins]      # the fragment's last READ bases
        seq[2 * rows + 1] = COMP[frag[:, ::-1]]
    return arr, insert


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_pairs = (int(os.environ.get("FILE_MIB", "1024")) << 20) // (2 * REC)
    arr, insert = make_pairs(n_pairs)
    text = arr.tobytes()
    n = len(text)
    overlap = 2 * READ - insert
    want = np.where(overlap >= 30, insert, 0)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pairs.fastq.gz")
        nb = write_bgzf(ctx, text, path)
        print(f"file: {nb} bytes ({n} bytes of text, {n_pairs} interleaved pairs of {READ} + {READ} bases); inserts of {SHORTEST} .. {SHORTEST + SPAN - 1} bases, "
              f"{int((want > 0).sum())} pairs overlap in 30 bases and more")
        kw = dict(first_byte=b"@")

        def timed(fn):
            def run():
                t = time.perf_counter()
                got = fn()
                return time.perf_counter() - t, got
            return run

        legs = [("a trim_records(record_lines=8), counted only", timed(lambda: bgzf.trim_records(path, None, 8, **kw))),
                ("b overlap_records, counted only", timed(lambda: bgzf.overlap_records(path, **kw))),
                ("c overlap_records, merged to one output", timed(lambda: bgzf.overlap_records(path, os.devnull, **kw))),
                ("d c + the unmerged pairs to a second", timed(lambda: bgzf.overlap_records(path, os.devnull, os.devnull, **kw)))]
        warm = [run()[1] for _, run in legs]
        a, b, c, dd = warm
        assert (a.records, a.kept) == (n_pairs, n_pairs) and not a.steps.any(), "a"
        assert b.records == n_pairs and np.array_equal(b.insert, want) and not b.mismatches.any() and b.merged == int((want > 0).sum()), "b"
        for other in (c, dd):
            for name in ("offset", "insert", "overlap", "mismatches", "verdict", "steps"):
                assert np.array_equal(getattr(b, name), getattr(other, name)), name
        outs = [os.path.join(d, "merged.gz"), os.path.join(d, "unmerged.gz")]
        bgzf.overlap_records(path, outs[0], outs[1], **kw)
        got = []
        for p in outs:
            with open(p, "rb") as f:
                blob = f.read()
            assert blob.endswith(bgzf.EOF_BLOCK), p
            got.append(gzip.decompress(blob))
            os.unlink(p)
        pairs = np.frombuffer(text, np.uint8).reshape(n_pairs, 2 * REC)
        assert got[1] == pairs[want == 0].tobytes(), "the unmerged pairs are not the input's"
        lines = got[0].split(b"\n")
        first = int(np.nonzero(want)[0][0])
        frag = arr[2 * first, HEAD:HEAD + READ].tobytes() + COMP[arr[2 * first + 1, HEAD:HEAD + READ][::-1]].tobytes()[2 * READ - int(insert[first]):]
        assert len(lines) == 4 * b.merged + 1 and lines[1] == frag and sum(map(len, lines[1::4])) == b.bases_merged, "the merged reads are not the fragments"
        print(f"b finds {b.merged} of {n_pairs} inserts, all of them the planted ones; mean overlap {b.mean_overlap:.1f}; c and d return b's arrays; d writes "
              f"{len(got[0])} + {len(got[1])} bytes")
        del warm, a, b, c, dd, got, lines, pairs, arr
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

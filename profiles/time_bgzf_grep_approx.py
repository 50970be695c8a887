"""BGZF by content with mismatches: timings, in the manner of profiles/time_bgzf_grep_records.py: the same
generated FASTQ of about FILE_MIB (1024) MiB, wall clock around calls that end in a synchronisation, the legs alternated inside one
process, RUNS (5) runs of each behind a warm-up run of each.  The barcode stands at the start of every 331st read, in turn as it is,
with one base substituted and with two.

  a   grep_records(k=4, match_line=1, first_byte=b"@"), exact: the floor
  b   the same with mismatches=1
  c   the same with mismatches=2 and eight barcodes
  d   the exact call given the 48 one-substitution variants of the barcode: what a caller does today
  e   64 patterns of 16 bytes with mismatches=1: the expensive end of the cost model

Every leg is checked against the reads generated here: the reads with a window within k substitutions of a pattern are found by
numpy, from the exact occurrences of one of the k + 1 pieces of each pattern (one of them is free of substitutions) and a count over
the 16 bytes there.  Bar: b's median is no more than a's median plus a's spread (max - min).  If it is missed, one more run of a and
of b is profiled by kernel class.

    python profiles/time_bgzf_grep_approx.py > profiles/bgzf_grep_approx.txt
"""
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
from time_bgzf_grep_records import BARCODE, EVERY, HEAD, READ, REC, carriers, make_fastq  # noqa: E402

L = len(BARCODE)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def other_base(b, step=1):
    return int(ACGT[(int(np.nonzero(ACGT == b)[0][0]) + step) % 4])


def plant(arr, tagged):
    """tagged read i carries the barcode with i % 3 bases substituted (the first, the second, the last one among the places)"""
    for i, r in enumerate(tagged.tolist()):
        at = [(i // 3) % L, (i // 3 + 7) % L][:i % 3]
        for p in at:
            arr[r, HEAD + p] = other_base(BARCODE[p], 1 + i % 2)


def near_reads(bases, pats, k, lo=0):
    """-> the numbers of the reads (rows of bases, uint8[n, READ], ACGT only) with L bytes that differ from one of pats in lo .. k places"""
    m = L // (k + 1)                                           # a piece's first m bytes are its seed
    lut = np.zeros(256, np.uint8)
    lut[ACGT] = np.arange(4, dtype=np.uint8)
    seeds = {}
    for pi, p in enumerate(pats):
        for piece in range(k + 1):
            code = sum(int(lut[p[piece * m + j]]) << (2 * j) for j in range(m))
            seeds.setdefault(code, []).append((pi, piece * m))
    codes = np.array(sorted(seeds), np.uint16 if m <= 8 else np.uint32)
    pat = np.array([np.frombuffer(p, np.uint8) for p in pats])
    hits, step = [np.empty(0, np.int64)], 1 << 18
    for o in range(0, len(bases), step):
        blk = bases[o:o + step]
        c = lut[blk]
        key = np.zeros((len(blk), READ - m + 1), codes.dtype)
        for j in range(m):
            key |= c[:, j:READ - m + 1 + j].astype(codes.dtype) << codes.dtype.type(2 * j)
        rr, cc = np.nonzero(np.isin(key, codes))
        kk = key[rr, cc]
        for code, owners in seeds.items():
            sel = kk == code
            for pi, off in owners:
                start = cc[sel] - off
                ok = (start >= 0) & (start <= READ - L)
                r2, s2 = rr[sel][ok], start[ok]
                n = (blk[r2[:, None], s2[:, None] + np.arange(L)] != pat[pi]).sum(1)
                hits.append(o + r2[(n <= k) & (n >= lo)])
    return np.unique(np.concatenate(hits)).tolist()


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, tagged = make_fastq(n_reads)
    plant(arr, tagged)
    rng = np.random.default_rng(11)
    others = [ACGT[rng.integers(0, 4, L)].tobytes() for _ in range(63)]
    eight, sixty_four = [BARCODE] + others[:7], [BARCODE] + others
    variants = [BARCODE[:p] + bytes([other_base(BARCODE[p], s)]) + BARCODE[p + 1:] for p in range(L) for s in (1, 2, 3)]
    assert len(set(variants)) == 48 and BARCODE not in variants
    bases = arr[:, HEAD:HEAD + READ]
    t = time.perf_counter()
    want = {"b": near_reads(bases, [BARCODE], 1), "c": near_reads(bases, eight, 2), "d": near_reads(bases, [BARCODE], 1, 1),
            "e": near_reads(bases, sixty_four, 1)}
    text = arr.tobytes()
    del arr, bases
    n = len(text)
    want["a"] = carriers(text)
    print(f"expected reads found on the host in {time.perf_counter() - t:.1f} s")
    planted = [set(tagged[s::3].tolist()) for s in range(3)]
    assert planted[0] <= set(want["a"]) and not (planted[1] | planted[2]) & set(want["a"])
    assert planted[0] | planted[1] <= set(want["b"]) and not planted[2] & set(want["b"]) and planted[1] <= set(want["d"]) and not planted[0] & set(want["d"])
    assert planted[0] | planted[1] | planted[2] <= set(want["c"]) and planted[0] | planted[1] <= set(want["e"])
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
        print(f"file: {nbytes} bytes ({n} bytes of text, {n_reads} reads of {READ} bases, {4 * n_reads} lines); barcode {BARCODE!r} planted in "
              f"{len(tagged)} reads: as it is, with one and with two bases substituted in turn")
        print("reads expected: " + ", ".join(f"{k} {len(want[k])}" for k in "abcde"))

        def leg(patterns, **kw):
            def run():
                t = time.perf_counter()
                got = bgzf.grep_records(path, patterns, 4, match_line=1, first_byte=b"@", **kw)
                return time.perf_counter() - t, got
            return run

        legs = [("a exact, one barcode", leg(BARCODE)), ("b mismatches=1, one barcode", leg(BARCODE, mismatches=1)),
                ("c mismatches=2, eight barcodes", leg(eight, mismatches=2)), ("d exact, the 48 variants of one barcode", leg(variants)),
                ("e mismatches=1, 64 patterns of 16 bytes", leg(sixty_four, mismatches=1))]
        warm = [run() for _, run in legs]
        for key, (_, got) in zip("abcde", warm):
            assert got.numbers.tolist() == want[key] and got.searched == n_reads, key
            assert bytes(got.data) == b"".join(text[r * REC:(r + 1) * REC] for r in want[key]), key
        print("every leg returns the expected reads, whole")
        del warm, got
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, run) in enumerate(legs):
                times[k].append(run()[0])
        (ma, sa), (mb, _), (mc, _), (md, _), (me, _) = [report(name, t, n) for (name, _), t in zip(legs, times)]
        met = mb <= ma + sa
        print(f"bar: b median {mb * 1e3:.3f} ms against a's median {ma * 1e3:.3f} ms plus its spread {sa * 1e3:.3f} ms = {(ma + sa) * 1e3:.3f} ms: "
              f"{'met' if met else 'MISSED'}")
        print(f"against a (the floor): b {100 * (mb - ma) / ma:+.1f} %, c {100 * (mc - ma) / ma:+.1f} %, d {100 * (md - ma) / ma:+.1f} %, e {100 * (me - ma) / ma:+.1f} %")
        if not met:                                            # where the time goes: one profiled run of a and of b, by kernel class
            ctx.profiling(True)
            for name, run in legs[:2]:
                ctx.kernel_times()
                run()
                kt = ctx.kernel_times()
                print(f"profiled {name}: " + ", ".join(f"{k} {ms:.3f} ms in {cnt} launches" for k, (ms, cnt) in kt.items() if cnt))
            ctx.profiling(False)


if __name__ == "__main__":
    main()

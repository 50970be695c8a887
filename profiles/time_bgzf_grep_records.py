"""BGZF by record: timings, in the manner of profiles/time_bgzf_grep.py.  No torch, wall clock around calls that
end in a synchronisation, the legs alternated inside one process, RUNS (5) runs of each behind a warm-up run of each.  The file is a
FASTQ of about FILE_MIB (1024) MiB generated here: reads of 150 bases, 315 bytes a record, a 16-base barcode at the start of every
331st read; level 6, written by bgzf.compress_dev.

  a   grep_records(k=4, match_line=1): the reads that carry the barcode, whole, in one pass
  b   today's way on the same commit: grep for the sequence lines, then LineIndex.build and read_lines of four lines per hit
  c   grep alone (the sequence lines, not the records): the floor
  d   grep_records(count=True)

Every leg is checked against the reads generated here.  Bar: a's median lies below b's median minus b's spread (max - min).

    python profiles/time_bgzf_grep_records.py > profiles/bgzf_grep_records.txt
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

READ, EVERY = 150, 331
BARCODE = b"GATTACAGATTACATC"
HEAD = 11                                        # b"@r%08d\n"
REC = HEAD + READ + 1 + 2 + READ + 1             # 315 bytes


def make_fastq(n_reads):
    """-> (uint8[n_reads, REC], the numbers of the reads that were given the barcode)"""
    rng = np.random.default_rng(5)
    a = np.empty((n_reads, REC), np.uint8)
    a[:, 0], a[:, 1] = ord("@"), ord("r")
    i = np.arange(n_reads, dtype=np.int64)
    for d in range(8):
        a[:, 2 + d] = (i // 10 ** (7 - d)) % 10 + 48
    a[:, HEAD - 1] = 10
    step = 1 << 18
    for o in range(0, n_reads, step):
        k = min(step, n_reads - o)
        a[o:o + k, HEAD:HEAD + READ] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (k, READ), dtype=np.uint8)]
        a[o:o + k, HEAD + READ + 3:REC - 1] = rng.integers(35, 74, (k, READ), dtype=np.uint8)
    a[:, HEAD + READ], a[:, HEAD + READ + 1], a[:, HEAD + READ + 2], a[:, REC - 1] = 10, ord("+"), 10, 10
    tagged = np.arange(7, n_reads, EVERY)
    a[tagged, HEAD:HEAD + len(BARCODE)] = np.frombuffer(BARCODE, np.uint8)
    return a, tagged


def carriers(text):
    """the numbers of the reads whose bases hold the barcode, by bytes.find over the whole text"""
    out, at = [], text.find(BARCODE)
    while at >= 0:
        r, col = divmod(at, REC)
        if HEAD <= col <= HEAD + READ - len(BARCODE) and (not out or out[-1] != r):
            out.append(r)
        at = text.find(BARCODE, at + 1)
    return out


def main():
    ctx = zlib_ng._ctx()
    print(_lib.load().zngamd_version().decode(), "RUNS", RUNS)
    n_reads = (int(os.environ.get("FILE_MIB", "1024")) << 20) // REC
    arr, tagged = make_fastq(n_reads)
    text = arr.tobytes()
    del arr
    n = len(text)
    want = carriers(text)
    assert set(tagged.tolist()) <= set(want)
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
        print(f"file: {nbytes} bytes ({n} bytes of text, {n_reads} reads of {READ} bases, {4 * n_reads} lines); barcode {BARCODE!r} in the bases of "
              f"{len(want)} reads ({100 * len(want) / n_reads:.3f} %), {len(tagged)} of them planted")
        records = [text[r * REC:(r + 1) * REC] for r in want]

        def leg_records():
            t = time.perf_counter()
            got = bgzf.grep_records(path, BARCODE, 4, match_line=1, first_byte=b"@")
            return time.perf_counter() - t, got

        def leg_today():
            t = time.perf_counter()
            hits = bgzf.grep(path, BARCODE)
            idx = bgzf.LineIndex.build(path)
            with bgzf.open(path) as r:
                got = r.read_lines(idx, [(int(x) // 4 * 4, 4) for x in hits.numbers[hits.numbers % 4 == 1]])
            return time.perf_counter() - t, got

        def leg_grep():
            t = time.perf_counter()
            got = bgzf.grep(path, BARCODE)
            return time.perf_counter() - t, got

        def leg_count():
            t = time.perf_counter()
            got = bgzf.grep_records(path, BARCODE, 4, match_line=1, count=True)
            return time.perf_counter() - t, got

        legs = [("a grep_records(k=4, match_line=1)", leg_records), ("b grep + LineIndex.build + read_lines", leg_today),
                ("c grep alone (sequence lines only)", leg_grep), ("d grep_records(count=True)", leg_count)]
        warm = [leg() for _, leg in legs]
        a, b, c, dcount = (w[1] for w in warm)
        assert a.numbers.tolist() == want and list(a) == records and a.searched == n_reads
        assert [bytes(x) for x in b] == records
        assert c.numbers.tolist() == [4 * r + 1 for r in want] and dcount == len(want)
        print(f"a returns {len(a)} records, {int(a.offsets[-1])} bytes; c returns {len(c)} lines, {int(c.offsets[-1])} bytes")
        del warm, a, b, c
        times = [[] for _ in legs]
        for _ in range(RUNS):
            for k, (_, leg) in enumerate(legs):
                times[k].append(leg()[0])
        (ma, _), (mb, sb), (mc, _), (md, _) = [report(name, t, n) for (name, _), t in zip(legs, times)]
        bound = mb - sb
        print(f"bar: a median {ma * 1e3:.3f} ms against b's median {mb * 1e3:.3f} ms minus its spread {sb * 1e3:.3f} ms = {bound * 1e3:.3f} ms: "
              f"{'met' if ma < bound else 'MISSED'}")
        print(f"a against c (the floor): {ma * 1e3:.3f} ms against {mc * 1e3:.3f} ms, {100 * (ma - mc) / mc:+.1f} %; d {md * 1e3:.3f} ms")


if __name__ == "__main__":
    main()

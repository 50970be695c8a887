"""Fuzz of the unit decoder (za_k_inflate_units_marked) with WRONG indexes: random streams of 3-10 units of the sizes where the
decoder changes its path, one to three mutations of tests/index_mutations.py composed (each made from the arrays the one before left),
one raw call per case.  The index is not authenticated, so the only acceptable outcomes are a refusal (E_INDEX / DATA_ERROR) or
STREAM_END with exactly the bytes the system zlib decodes from the unmodified stream.  Index content only: pointers, def_len and
the 64 readable bytes behind the stream stay what the ABI asks of a caller.  The first HIP error ends the run.
usage: python3 profiles/fuzz_index_rows.py <seed> <cases>"""
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from zlib_ng_amd import _lib, corpus, devmem  # noqa: E402
import index_mutations as M  # noqa: E402

seed, cases = int(sys.argv[1]), int(sys.argv[2])
rng = np.random.default_rng(seed)
ctx = _lib.default_context()
fastq = corpus.fastq(1 << 20, seed=seed + 1).tobytes()
SIZES = [0, 1, 2047, 2048, 2049, 16384, 70001, 131072]


def stitch(total):
    """pieces of FASTQ, noise, zeros, short periods and 2-bit "DNA" (tests/test_gpu_random_property._stitch)"""
    parts, n = [], 0
    while n < total:
        kind = int(rng.integers(0, 5))
        ln = int(rng.integers(1, 40000))
        if kind == 0:
            o = int(rng.integers(0, len(fastq) - ln))
            p = fastq[o:o + ln]
        elif kind == 1:
            p = rng.bytes(ln)
        elif kind == 2:
            p = bytes(ln)
        elif kind == 3:
            pat = rng.bytes(int(rng.integers(1, 40)))
            p = (pat * (ln // len(pat) + 1))[:ln]
        else:
            p = bytes(rng.integers(0, 4, ln, dtype=np.uint8) + 65)
        parts.append(p)
        n += ln
    return b"".join(parts)[:total]


bad = refused = fine = 0
for case in range(cases):
    sizes = [int(rng.choice(SIZES)) for _ in range(int(rng.integers(3, 11)))]
    d0 = stitch(int(rng.choice([0, 0, 1000, 32768])))
    data = stitch(sum(sizes))
    buf = d0 + data
    blocks, off = [], len(d0)
    for n in sizes:
        blocks.append((off, n, min(32768, off), _lib.FLAG_SEG2K))
        off += n
    level = int(rng.choice([1, 6, 9]))
    outs, crcs, ovf = ctx.deflate_blocks(buf, blocks, level, 131072 + 131072 // 8 + 600)
    assert not ovf
    nu = len(blocks)
    rows = ctx.deflate_index(nu).cpu(np.uint32).reshape(nu, -1).copy()
    stream = b"".join(outs) + b"\x03\x00"
    uin, uout = np.array([len(c) for c in outs], np.uint32), np.array(sizes, np.uint32)
    ref = (zlib.decompressobj(-15, zdict=d0) if d0 else zlib.decompressobj(-15)).decompress(stream)
    assert ref == data
    kinds = M.kinds_of(stream, uin, uout, rows)
    names = []
    for _ in range(int(rng.integers(1, 4))):
        pool = list(M.rows_cases(uin, uout, rows, kinds))
        name, uin, uout, rows, _must = pool[int(rng.integers(0, len(pool)))]
        names.append(name)
    total = int(uout.astype(np.int64).sum())
    assert int(uin.astype(np.int64).sum()) + 2 == len(stream) and int(uout.max()) <= 131072
    d_def = devmem.from_host(ctx, stream + bytes(64))
    d_out = devmem.empty(ctx, total + 64)
    d_rows = devmem.from_host(ctx, np.ascontiguousarray(rows, np.uint32))
    d_dict = devmem.from_host(ctx, d0) if d0 else None
    r, n = ctx.inflate_units_indexed_dev(d_def.ptr, len(stream), uin, uout, d_rows.ptr, d_out.ptr, total, d_dict.ptr if d_dict else None, len(d0))
    if r == _lib.E_HIP:
        print("HIP ERROR case", case, "sizes", sizes, "level", level, "dict", len(d0), "mutations", names, ctx.err())
        print("fuzz_index_rows seed %d: stopped; cases %d mismatches %d" % (seed, case + 1, bad + 1))
        sys.exit(2)
    if r == _lib.STREAM_END:
        ok = n == len(data) and d_out[0:n].cpu().tobytes() == ref
        fine += ok
    else:
        ok = r in (_lib.E_INDEX, _lib.DATA_ERROR)
        refused += ok
    if not ok:
        bad += 1
        print("MISMATCH case", case, "sizes", sizes, "level", level, "dict", len(d0), "mutations", names, "r", r, "n", n, ctx.err())
print("fuzz_index_rows seed %d: %d refused, %d decoded right; cases %d mismatches %d" % (seed, refused, fine, cases, bad))
sys.exit(1 if bad else 0)

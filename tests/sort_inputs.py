"""Inputs of the BGZF sort tests: rows for sort_keys (every pattern the radix passes can go wrong on), a table of two-line records
whose fields cross every strip and width edge for sort_key_records, the key grid that is laid over it, and a shuffled VCF.  All
generated from fixed seeds; fields hold no NUL, so the order by parsed values and the order by key bytes are one (asserted on the CPU
in test_cpu_bgzf_sort.py)."""
import functools

import numpy as np

import sort_ref as R

TILE = 2048                                                  # rows per workgroup of the sort's hist and scatter kernels (ZA_SORT_TILE)
SCAN_TURN = 256 * TILE                                       # rows beyond which the scan kernel carries a sum into a second turn
SIZES = (0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, (1 << 17) + 3)
WIDTHS = (8, 16, 256)
PATTERNS = ("equal", "byte0", "byte_last", "sorted", "reversed", "all256", "two_keys", "one_bucket", "carry", "random")


def rows(pattern, n, w, seed=5):
    """-> uint8 (n, w)"""
    rng = np.random.default_rng(seed + 1000 * w + n % 997)
    k = np.zeros((n, w), np.uint8)
    k[:] = rng.integers(1, 255, size=w, dtype=np.uint8)       # a constant row underneath: every digit skipped unless the pattern says otherwise
    if not n:
        return k
    if pattern == "equal":
        pass
    elif pattern == "byte0":
        k[:, 0] = rng.integers(0, 256, n)
    elif pattern == "byte_last":
        k[:, w - 1] = rng.integers(0, 256, n)
    elif pattern in ("sorted", "reversed"):
        v = np.arange(n, dtype=np.uint64) if pattern == "sorted" else np.arange(n, dtype=np.uint64)[::-1]
        k[:, w - 8:] = v.astype(">u8").view(np.uint8).reshape(n, 8)
    elif pattern == "all256":
        k[:, w // 2] = (np.arange(n) * 7) % 256               # all 256 values in one digit (once n >= 256), round and round
    elif pattern == "two_keys":
        k[:, w - 3] = rng.integers(0, 2, n) * 200             # stability: two distinct rows, thousands of ties
    elif pattern == "one_bucket":
        k[:, 1] = 9
        k[n // 2, 1] = 3                                      # one bucket holds every row but one
    elif pattern == "carry":
        k[:, w - 1] = rng.integers(0, 256, n)                 # the earlier pass's digit varies in all rows ...
        k[:, w - 2] = rng.integers(0, 3, n)                   # ... and the later pass must keep its order within every value of this one
    elif pattern == "random":
        k[:] = rng.integers(0, 256, size=(n, w), dtype=np.uint8)
    else:
        raise KeyError(pattern)
    return np.ascontiguousarray(k)


# ---- the table: two-line records "name <tab> number <tab> tag \n body \n"
EDGES = (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
NUMBERS = (b"0", b"007", b"18446744073709551615", b"18446744073709551614", b"1", b"10", b"9", b"0" * 70 + b"5", b"00000000000000000000", b"4294967296")
LETTERS = np.frombuffer(b"ACGTNacgtn", np.uint8)


def _word(rng, n, alphabet=LETTERS):
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


@functools.lru_cache(maxsize=None)
def table(meta=False, short_last=False, open_last=False):
    """-> the records (bytes each).  Names and bodies take every length of EDGES, names repeat (ties), the tag column is at most 8 bytes
    and missing in every seventh record, numbers come from NUMBERS and a generator.  meta: lines that begin with '#' in front and in
    the middle (their fields would be faults: they are never parsed).  short_last: a last record of one line.  open_last: the last
    line lacks its delimiter."""
    rng = np.random.default_rng(31)
    recs = []
    names = [_word(rng, n) for n in EDGES for _ in range(3)]
    for i in range(330):
        name = names[int(rng.integers(0, len(names)))] if i % 3 else names[i % len(names)]
        num = NUMBERS[i % len(NUMBERS)] if i % 4 == 0 else b"%d" % int(rng.integers(0, 1 << 40))
        tag = _word(rng, int(rng.integers(0, 9)))
        body = _word(rng, EDGES[i % len(EDGES)])
        head = name + b"\t" + num + (b"" if i % 7 == 6 else b"\t" + tag)
        recs.append(head + b"\n" + body + b"\n")
    if meta:
        m = [b"##meta line %d\tnot a number\n" % j + b"x" * (300 * j) + b"\n" for j in range(3)]
        recs = m[:2] + recs[:150] + m[2:] + recs[150:]
    if short_last:
        recs.append(b"lonely\t12\ttag\n")
    if open_last:
        recs[-1] = recs[-1][:-1]
    return tuple(recs)


TRUNC = dict(truncate=True)
GRID = {
    "name32": [R.part(0, 0, **TRUNC)],
    "name64 first5": [R.part(0, 0, width=64, first=5, **TRUNC)],
    "name8 first40": [R.part(0, 0, width=8, first=40, **TRUNC)],
    "body128 fold": [R.part(1, width=128, ignore_case=True, **TRUNC)],
    "body128 fold reverse": [R.part(1, width=128, ignore_case=True, reverse=True, **TRUNC)],
    "tag8": [R.part(0, 2, width=8)],                         # (no tag is longer: no truncation needed)
    "tag8 reverse": [R.part(0, 2, width=8, reverse=True)],
    "number": [R.part(0, 1, kind="number")],
    "number reverse": [R.part(0, 1, kind="number", reverse=True)],
    "length": [R.part(1, kind="length")],
    "length of tag reverse": [R.part(0, 2, kind="length", reverse=True)],
    "missing column": [R.part(0, 5, width=8), R.part(0, 5, kind="length")],
    "name then number": [R.part(0, 0, **TRUNC), R.part(0, 1, kind="number")],
    "four parts": [R.part(1, kind="length"), R.part(1, width=128, ignore_case=True, **TRUNC), R.part(0, 1, kind="number", reverse=True), R.part(0, 2, width=8)],
    "widest": [R.part(1, width=128, **TRUNC), R.part(1, width=128, first=128, **TRUNC)],
    "none": [],
}


def grid_conf(name, **kw):
    return R.conf(GRID[name], record_lines=2, **kw)


# ---- a VCF: header lines, 3 contigs, equal positions for ties, shuffled
@functools.lru_cache(maxsize=None)
def vcf(n=900, seed=9):
    """-> (header lines, body lines shuffled)"""
    rng = np.random.default_rng(seed)
    head = [b"##fileformat=VCFv4.2\n", b"##contig=<ID=chr1>\n", b"##contig=<ID=chr10>\n", b"##contig=<ID=chr2>\n", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"]
    contigs = (b"chr1", b"chr10", b"chr2")
    body = []
    for i in range(n):
        c = contigs[int(rng.integers(0, 3))]
        pos = int(rng.integers(1, 400)) * 1000 if i % 3 else int(rng.integers(1, 5)) * 1000      # many ties
        body.append(b"%s\t%d\tid%d\tA\tC\t50\tPASS\tDP=%d\n" % (c, pos, i, int(rng.integers(1, 99))))
    return tuple(head), tuple(body)


def fastq_records(text):
    lines = text.split(b"\n")
    if not lines[-1]:
        lines.pop()
    return [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines), 4)]

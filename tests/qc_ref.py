"""The referee of qc_records: the rule of include/zng_amd.h in plain Python on plain bytes, the serial loops as
they are stated there.  Never the code under test.  The records are split as trim_ref splits them."""
from collections import namedtuple

from trim_ref import Fault, split_records

BASES, QUALITIES, GC_BINS = 6, 94, 101

Conf = namedtuple("Conf", "record_lines seq_line qual_line quality_base cycles low_quality first_byte delimiter")


def conf(record_lines=4, seq_line=1, qual_line=3, quality_base=33, cycles=512, low_quality=15, first_byte=None, delimiter=b"\n"):
    return Conf(record_lines, seq_line, -1 if qual_line is None else qual_line, quality_base, cycles, low_quality, first_byte, bytes(delimiter))


def base_class(byte):
    return {65: 0, 67: 1, 71: 2, 84: 3, 78: 4}.get(byte & 0xDF, 5)


def quality(byte, base):
    """-> (Q, whether the byte was clamped)"""
    d = byte - base
    q = min(max(d, 0), QUALITIES - 1)
    return q, q != d


def table_words(cycles):
    return (cycles + 1) * (BASES + QUALITIES) + (cycles + 2) + GC_BINS + QUALITIES


Result = namedtuple("Result", "base_pos qual_pos length_hist gc_hist meanq_hist totals rows")
TOTALS = ("seen", "bytes_in", "bases", "min_len", "max_len", "empty", "base_total", "quality_sum", "q20_bases", "q30_bases", "low_bases", "quality_clamped")


def new_result(cycles):
    C = cycles
    t = dict.fromkeys(TOTALS, 0)
    t["min_len"], t["base_total"] = 2 ** 64 - 1, [0] * BASES
    return Result([[0] * BASES for _ in range(C + 1)], [[0] * QUALITIES for _ in range(C + 1)], [0] * (C + 2), [0] * GC_BINS, [0] * QUALITIES, t, [])


def count_record(res, cf, seq, qual, nbytes):
    """one record into res; qual: None without a qual_line.  The row appended: (qsum, len, gc, n, low)"""
    C, t = cf.cycles, res.totals
    n = len(seq)
    gc = ns = low = qsum = 0
    for i in range(n):
        c = base_class(seq[i])
        res.base_pos[min(i, C)][c] += 1
        t["base_total"][c] += 1
        gc += c in (1, 2)
        ns += c == 4
        if qual is not None:
            q, clamped = quality(qual[i], cf.quality_base)
            res.qual_pos[min(i, C)][q] += 1
            qsum += q
            t["quality_clamped"] += clamped
            t["q20_bases"] += q >= 20
            t["q30_bases"] += q >= 30
            low += q < cf.low_quality
    res.length_hist[n if n <= C else C + 1] += 1
    if n >= 1:
        res.gc_hist[(100 * gc) // n] += 1
        if qual is not None:
            res.meanq_hist[qsum // n] += 1
    t["seen"] += 1
    t["bytes_in"] += nbytes
    t["bases"] += n
    t["min_len"], t["max_len"] = min(t["min_len"], n), max(t["max_len"], n)
    t["empty"] += n == 0
    t["quality_sum"] += qsum
    t["low_bases"] += low
    res.rows.append((qsum, n, gc, ns, low))


def qc_text(text, cf, final=True):
    """The whole rule over a text: -> Result.  totals: a dict with the names of zngamd_bgzf_qc_totals that the rule decides.  Fault(1 / 3,
    record) for the first record at fault, a record with both for its first byte."""
    recs, _, _ = split_records(text, cf.record_lines, cf.delimiter, final)
    res = new_result(cf.cycles)
    for r, rec in enumerate(recs):
        if cf.first_byte is not None and not (rec[0][0] + (cf.delimiter if rec[0][1] else b"")).startswith(bytes(cf.first_byte)):
            raise Fault(1, r)
        seq = rec[cf.seq_line][0] if cf.seq_line < len(rec) else b""
        qual = None
        if cf.qual_line >= 0:
            qual = rec[cf.qual_line][0] if cf.qual_line < len(rec) else b""
            if len(qual) != len(seq):
                raise Fault(3, r, (len(seq), len(qual)))
        count_record(res, cf, seq, qual, sum(len(body) + d for body, d in rec))
    return res


def flat(res):
    """the tables as the C ABI lays them out: one list of words"""
    return [v for row in res.base_pos for v in row] + [v for row in res.qual_pos for v in row] + res.length_hist + res.gc_hist + res.meanq_hist


def add(a, b):
    """the sum of two Results over the same cycles, as the parts of a file add up"""
    t = {}
    for name in TOTALS:
        x, y = a.totals[name], b.totals[name]
        t[name] = min(x, y) if name == "min_len" else max(x, y) if name == "max_len" else [p + q for p, q in zip(x, y)] if name == "base_total" else x + y
    rows2 = lambda p, q: [[x + y for x, y in zip(r, s)] for r, s in zip(p, q)]
    rows1 = lambda p, q: [x + y for x, y in zip(p, q)]
    return Result(rows2(a.base_pos, b.base_pos), rows2(a.qual_pos, b.qual_pos), rows1(a.length_hist, b.length_hist), rows1(a.gc_hist, b.gc_hist),
                  rows1(a.meanq_hist, b.meanq_hist), t, a.rows + b.rows)

"""The referee of trim_records: the rule of include/zng_amd.h in plain Python on plain bytes, the serial loops
as they are stated there.  Never the code under test."""
from collections import namedtuple

KEPT, TOO_SHORT, DROPPED = 0, 1, 2
NO_ADAPTER = -1

Conf = namedtuple("Conf", "record_lines seq_line qual_line cut quality quality_base adapters mismatches min_overlap min_length first_byte delimiter")


def conf(record_lines=4, seq_line=1, qual_line=3, cut=(0, 0), quality=(0, 0), quality_base=33, adapters=(), mismatches=0, min_overlap=3, min_length=0,
         first_byte=None, delimiter=b"\n"):
    return Conf(record_lines, seq_line, -1 if qual_line is None else qual_line, tuple(cut), tuple(quality), quality_base, [bytes(a) for a in adapters],
                mismatches, min_overlap, min_length, first_byte, bytes(delimiter))


def fixed_cut(n, front, back):
    a = min(front, n)
    return a, max(a, n - min(back, n))


def quality_cut(qual, a, b, front, back, base=33):
    """-> (a, b): both scans over the [a, b) given, independently; a cutoff of 0 is off"""
    nb = b
    if back > 0:
        s = best = 0
        for i in range(b - 1, a - 1, -1):
            s += back - (qual[i] - base)
            if s < 0:
                break
            if s > best:
                best, nb = s, i
    na = a
    if front > 0:
        s = best = 0
        for i in range(a, b):
            s += front - (qual[i] - base)
            if s < 0:
                break
            if s > best:
                best, na = s, i + 1
    return na, max(na, nb)


def adapter_cut(R, adapters, k, min_overlap):
    """-> (p, j); (len(R), NO_ADAPTER): none"""
    m = len(R)
    for p in range(m):
        for j, A in enumerate(adapters):
            L = len(A)
            o = min(L, m - p)
            if o < min(min_overlap, L):
                continue
            d = sum(1 for x, y in zip(R[p:p + o], A[:o]) if x != y)
            if d <= (k * o) // L:
                return p, j
    return m, NO_ADAPTER


def split_records(text, k, delimiter=b"\n", final=True):
    """-> (records, where every record starts, consumed): every record a list of (body, has_delimiter); with final the bytes behind the
    last delimiter are a line and the lines left over one short last record; without it they stay for the next call (consumed: where
    the open record starts)"""
    rows, at = [], 0
    while at < len(text):
        e = text.find(delimiter, at)
        if e < 0:
            if final:
                rows.append((text[at:], False, at))
                at = len(text)
            break
        rows.append((text[at:e], True, at))
        at = e + 1
    whole = len(rows) // k * k
    used = len(rows) if final else whole
    recs = [[(b, d) for b, d, _ in rows[i:i + k]] for i in range(0, used, k)]
    starts = [rows[i][2] for i in range(0, used, k)]
    consumed = len(text) if final else rows[whole][2] if whole < len(rows) else at
    return recs, starts, consumed


class Fault(Exception):
    def __init__(self, kind, record, lengths=None):
        super().__init__(kind, record, lengths)
        self.kind, self.record, self.lengths = kind, record, lengths


def trim_record(rec, cf):
    """rec: list of (body, has_delimiter) -> (a, b, adapter, steps, n, quality_trimmed, adapter_trimmed, written bytes); Fault(3) when the bodies differ"""
    seq = rec[cf.seq_line][0] if cf.seq_line < len(rec) else b""
    n = len(seq)
    qual = None
    if cf.qual_line >= 0:
        qual = rec[cf.qual_line][0] if cf.qual_line < len(rec) else b""
        if len(qual) != n:
            raise Fault(3, None, (n, len(qual)))
    a, b = fixed_cut(n, *cf.cut)
    steps = 1 if (a, b) != (0, n) else 0
    qt = at = 0
    if qual is not None:
        na, nb = quality_cut(qual, a, b, cf.quality[0], cf.quality[1], cf.quality_base)
        if (na, nb) != (a, b):
            steps |= 2
        qt = (b - a) - (nb - na)
        a, b = na, nb
    adapter = NO_ADAPTER
    if cf.adapters:
        p, adapter = adapter_cut(seq[a:b], cf.adapters, cf.mismatches, cf.min_overlap)
        if adapter != NO_ADAPTER:
            steps |= 4
            at = (b - a) - p
            b = a + p
    out = b""
    for i, (body, d) in enumerate(rec):
        out += (body[a:b] if i in (cf.seq_line, cf.qual_line) else body) + (cf.delimiter if d else b"")
    return a, b, adapter, steps, n, qt, at, out


Result = namedtuple("Result", "begin end adapter verdict steps kept_bytes short_bytes totals")


def trim_text(text, cf, drop=None, final=True):
    """The whole rule over a text: -> Result.  drop: None or a sequence of truth values, one per record (a record beyond it is a
    dropped one and sets drop_short).  totals: a dict with the names of zngamd_bgzf_trim_totals that the rule decides.  Fault(1 / 3,
    record) for the first record at fault, a record with both for its first byte."""
    recs, _, _ = split_records(text, cf.record_lines, cf.delimiter, final)
    begin, end, adapter, verdict, steps = [], [], [], [], []
    kept, short = [], []
    t = dict(seen=len(recs), kept=0, too_short=0, dropped=0, bytes_in=0, bases_in=0, bases_out=0, quality_trimmed=0, adapter_trimmed=0,
             drop_short=int(drop is not None and len(drop) < len(recs)), adapter_records=[0] * len(cf.adapters))
    for r, rec in enumerate(recs):
        if cf.first_byte is not None and not (rec[0][0] + (cf.delimiter if rec[0][1] else b"")).startswith(bytes(cf.first_byte)):
            raise Fault(1, r)
        try:
            a, b, j, st, n, qt, at, out = trim_record(rec, cf)
        except Fault as e:
            raise Fault(3, r, e.lengths) from None
        v = DROPPED if drop is not None and (r >= len(drop) or drop[r]) else TOO_SHORT if b - a < cf.min_length else KEPT
        begin.append(a); end.append(b); adapter.append(j); verdict.append(v); steps.append(st)
        t["bytes_in"] += sum(len(body) + d for body, d in rec)
        t["bases_in"] += n
        t["quality_trimmed"] += qt
        t["adapter_trimmed"] += at
        if j != NO_ADAPTER:
            t["adapter_records"][j] += 1
        if v == KEPT:
            t["kept"] += 1
            t["bases_out"] += b - a
            kept.append(out)
        elif v == TOO_SHORT:
            t["too_short"] += 1
            short.append(out)
        else:
            t["dropped"] += 1
    return Result(begin, end, adapter, verdict, steps, kept, short, t)

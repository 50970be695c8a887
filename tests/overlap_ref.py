"""The referee of overlap_records: the rule of include/zng_amd.h in plain Python on plain bytes, the serial loops
as they are stated there.  Never the code under test."""
from collections import namedtuple

from trim_ref import Fault, split_records

NONE, FOUND, MERGED, TOO_LONG = 0, 1, 2, 3
MAX_READ = 1024

Conf = namedtuple("Conf", "record_lines seq_line qual_line quality_base min_overlap mismatches percent merge correct q_high q_low cut first_byte delimiter")


def conf(record_lines=8, seq_line=1, qual_line=3, quality_base=33, min_overlap=30, mismatches=5, percent=20, merge=True, correct=False,
         correct_quality=(30, 14), cut=False, first_byte=None, delimiter=b"\n"):
    return Conf(record_lines, seq_line, -1 if qual_line is None else qual_line, quality_base, min_overlap, mismatches, percent, bool(merge), bool(correct),
                correct_quality[0], correct_quality[1], bool(cut), first_byte, bytes(delimiter))


def comp(c):
    """A<->T, C<->G in either case, U -> A, u -> a; every other byte itself"""
    return {65: 84, 84: 65, 67: 71, 71: 67, 85: 65, 97: 116, 116: 97, 99: 103, 103: 99, 117: 97}.get(c, c)


def revcomp(y):
    return bytes(comp(c) for c in reversed(y))


_found = {}                                    # (the search does not depend on the flags: a pair is searched once per set of limits)


def find(a, y, cf):
    """step 1 -> (o, L, d) of the winner; None: no offset is acceptable, or a mate is longer than MAX_READ (the caller tells the two apart)"""
    key = (bytes(a), bytes(y), cf.min_overlap, cf.mismatches, cf.percent)
    if key not in _found:
        _found[key] = _find(a, y, cf)
    return _found[key]


def _find(a, y, cf):
    n1, n2 = len(a), len(y)
    if n1 > MAX_READ or n2 > MAX_READ:
        return None
    b = revcomp(y)
    best = None
    for o in range(-(n2 - 1), n1):
        lo, hi = max(0, o), min(n1, o + n2)
        L = hi - lo
        if L < cf.min_overlap:
            continue
        d = 0
        for i in range(lo, hi):
            if a[i] != b[i - o]:
                d += 1
        if d > min(cf.mismatches, L * cf.percent // 100):
            continue
        key = (-L, d, abs(o), 0 if o >= 0 else 1)
        if best is None or key < best[0]:
            best = (key, (o, L, d))
    return best[1] if best else None


Pair = namedtuple("Pair", "offset insert overlap mismatches corrected verdict steps cls out n1 n2 trimmed")


def overlap_record(rec, cf):
    """rec: list of (body, has_delimiter) -> Pair; Fault(3) when a mate's two bodies differ in length"""
    k = cf.record_lines
    m = k // 2
    body = lambda i: rec[i][0] if i < len(rec) else b""
    a, y = body(cf.seq_line), body(m + cf.seq_line)
    n1, n2 = len(a), len(y)
    qa = qy = None
    if cf.qual_line >= 0:
        qa, qy = body(cf.qual_line), body(m + cf.qual_line)
        if len(qa) != n1:
            raise Fault(3, None, (n1, len(qa)))
        if len(qy) != n2:
            raise Fault(3, None, (n2, len(qy)))
    Q = lambda q, i: q[i] - cf.quality_base if q is not None else 0
    too_long = n1 > MAX_READ or n2 > MAX_READ
    hit = None if too_long else find(a, y, cf)
    if hit is None:
        out = b"".join(bd + (cf.delimiter if d else b"") for bd, d in rec)
        return Pair(0, 0, 0, 0, 0, TOO_LONG if too_long else NONE, 0, 1, out, n1, n2, 0)
    o, L, d = hit
    insert = o + n2
    b, qb = revcomp(y), (qy[::-1] if qy is not None else None)
    # step 2
    na, nqa = bytearray(a), bytearray(qa) if qa is not None else None
    ny, nqy = bytearray(y), bytearray(qy) if qy is not None else None
    corrected = 0
    if cf.correct:
        for i in range(max(0, o), min(n1, o + n2)):
            j = i - o
            if a[i] == b[j]:
                continue
            if Q(qa, i) >= cf.q_high and Q(qb, j) <= cf.q_low:
                ny[n2 - 1 - j], nqy[n2 - 1 - j] = comp(a[i]), qa[i]
                corrected += 1
            elif Q(qb, j) >= cf.q_high and Q(qa, i) <= cf.q_low:
                na[i], nqa[i] = b[j], qb[j]
                corrected += 1
    # step 3
    e1, e2 = (min(n1, insert), min(n2, n2 + o)) if cf.cut else (n1, n2)
    steps = (1 if e1 < n1 else 0) | (2 if e2 < n2 else 0) | (4 if corrected else 0)
    trimmed = (n1 - e1) + (n2 - e2)
    if cf.merge:
        # step 4, on the source text as it stood before step 2
        ms, mq = bytearray(), bytearray()
        for c in range(insert):
            in_a, in_b = c < n1, c - o >= 0
            use_a = in_a and (not in_b or Q(qa, c) >= Q(qb, c - o))
            ms.append(a[c] if use_a else b[c - o])
            if qa is not None:
                mq.append(qa[c] if use_a else qb[c - o])
        out = b""
        for i in range(m):
            bd, dl = rec[i]
            out += (bytes(ms) if i == cf.seq_line else bytes(mq) if i == cf.qual_line else bd) + (cf.delimiter if dl else b"")
        return Pair(o, insert, L, d, corrected, MERGED, steps, 0, out, n1, n2, trimmed)
    out = b""
    for i, (bd, dl) in enumerate(rec):
        if i == cf.seq_line:
            bd = bytes(na[:e1])
        elif i == cf.qual_line:
            bd = bytes(nqa[:e1])
        elif i == m + cf.seq_line:
            bd = bytes(ny[:e2])
        elif cf.qual_line >= 0 and i == m + cf.qual_line:
            bd = bytes(nqy[:e2])
        out += bd + (cf.delimiter if dl else b"")
    return Pair(o, insert, L, d, corrected, FOUND, steps, 1, out, n1, n2, trimmed)


Result = namedtuple("Result", "offset insert overlap mismatches corrected verdict steps merged_bytes other_bytes totals")


def overlap_text(text, cf, final=True):
    """The whole rule over a text: -> Result; merged_bytes and other_bytes: the written bytes of class 0 and class 1, a piece per pair.
    totals: a dict with the names of zngamd_bgzf_overlap_totals that the rule decides.  Fault(1 / 3, record) for the first record at
    fault, a record with both for its first byte."""
    k = cf.record_lines
    m = k // 2
    recs, _, _ = split_records(text, k, cf.delimiter, final)
    cols = [[] for _ in range(7)]
    merged, other = [], []
    t = dict(seen=len(recs), none=0, found=0, merged=0, too_long=0, bytes_in=0, bases_in=0, bases_merged=0, corrected=0, corrected_pairs=0, adapter_pairs=0,
             adapter_trimmed=0, overlap_sum=0, mismatch_sum=0)
    for r, rec in enumerate(recs):
        if cf.first_byte is not None:
            for i in (0, m):
                line = rec[i][0] + (cf.delimiter if rec[i][1] else b"") if i < len(rec) else b""
                if not line.startswith(bytes(cf.first_byte)):
                    raise Fault(1, r)
        try:
            p = overlap_record(rec, cf)
        except Fault as e:
            raise Fault(3, r, e.lengths) from None
        for col, v in zip(cols, p[:7]):
            col.append(v)
        t[("none", "found", "merged", "too_long")[p.verdict]] += 1
        t["bytes_in"] += sum(len(bd) + d for bd, d in rec)
        t["bases_in"] += p.n1 + p.n2
        t["overlap_sum"] += p.overlap
        t["mismatch_sum"] += p.mismatches
        t["corrected"] += p.corrected
        t["corrected_pairs"] += 1 if p.corrected else 0
        t["adapter_pairs"] += 1 if p.trimmed else 0
        t["adapter_trimmed"] += p.trimmed
        if p.verdict == MERGED:
            t["bases_merged"] += p.insert
        (merged if p.cls == 0 else other).append(p.out)
    return Result(*cols, merged, other, t)

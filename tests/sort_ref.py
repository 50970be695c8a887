"""A plain referee for the BGZF sort (bgzf.sort_key_records, sort_keys, permute_records, sort_records), written from the statement of
the key encoding and of the order, never from the kernels.  encode() makes the key bytes from the text, field by field; order() sorts
by PARSED values (Python bytes, ints), not by encoded bytes, so that the encoding and the order are tested against each other;
lexorder() is np.lexsort over the big-endian 64-bit columns of any rows."""
import collections

import numpy as np

Part = collections.namedtuple("Part", "line column sep kind width first reverse ignore_case truncate")
Conf = collections.namedtuple("Conf", "record_lines parts meta delimiter first_byte")


def part(line=0, column=None, sep=b"\t", kind="bytes", width=32, first=0, reverse=False, ignore_case=False, truncate=False):
    return Part(line, column, sep, kind, width if kind == "bytes" else 0, first if kind == "bytes" else 0, reverse, ignore_case, truncate)


def conf(parts=(), record_lines=4, meta=None, delimiter=b"\n", first_byte=None):
    return Conf(record_lines, tuple(parts), meta, delimiter, first_byte)


class Fault(Exception):
    def __init__(self, kind, record):
        Exception.__init__(self, kind, record)
        self.kind, self.record = kind, record


def width_of(cf):
    w = sum(p.width if p.kind == "bytes" else 8 if p.kind == "number" else 4 for p in cf.parts)
    return (w + 7) // 8 * 8


def split(text, cf):
    """-> the records of a whole text as they lie in it: record_lines lines each; the last may be short, and may lack its delimiter"""
    d = cf.delimiter
    lines = text.split(d)
    lines = [x + d for x in lines[:-1]] + ([lines[-1]] if lines[-1] else [])
    k = cf.record_lines
    return [b"".join(lines[i:i + k]) for i in range(0, len(lines), k)]


def lengths(records, cf):
    """what the key pass reports: the record's bytes, and one more for a last record whose last line lacks its delimiter"""
    out = [len(r) for r in records]
    if records and not records[-1].endswith(cf.delimiter):
        out[-1] += 1
    return out


def written(records, cf):
    """the records as permute_records writes them"""
    return [r if r.endswith(cf.delimiter) else r + cf.delimiter for r in records]


def field(record, p, cf):
    lines = record.split(cf.delimiter)
    if record.endswith(cf.delimiter):
        lines.pop()
    if p.line >= len(lines):
        return b""
    body = lines[p.line]
    if p.column is None:
        return body
    cols = body.split(p.sep)
    return cols[p.column] if p.column < len(cols) else b""


def is_meta(record, cf):
    return cf.meta is not None and record[:1] == cf.meta


def _fold(b):
    return bytes(c - 32 if 97 <= c <= 122 else c for c in b)


def value(record, p, cf):
    """the parsed value of one part; Fault kinds 2 and 3 (the record number is filled in by the caller)"""
    f = field(record, p, cf)
    if p.kind == "length":
        return len(f)
    if p.kind == "number":
        if not f or any(not 48 <= c <= 57 for c in f) or int(f) > (1 << 64) - 1:
            raise Fault(2, None)
        return int(f)
    if len(f) > p.first + p.width and not p.truncate:
        raise Fault(3, None)
    f = f[p.first:p.first + p.width]
    return _fold(f) if p.ignore_case else f


def check(records, cf):
    """raises the Fault of the smallest record at fault (of two at one record the one with the lower number), as the key pass reports it"""
    for i, r in enumerate(records):
        if cf.first_byte is not None and r[:1] != cf.first_byte:
            raise Fault(1, i)
        if is_meta(r, cf):
            continue
        kinds = []
        for p in cf.parts:
            try:
                value(r, p, cf)
            except Fault as e:
                kinds.append(e.kind)
        if kinds:
            raise Fault(min(kinds), i)


def encode(records, cf):
    """-> uint8 (n, W): the key bytes, from the statement of the encoding"""
    check(records, cf)
    w = width_of(cf)
    out = np.zeros((len(records), w), np.uint8)
    for i, r in enumerate(records):
        if is_meta(r, cf):
            continue
        row = b""
        for p in cf.parts:
            v = value(r, p, cf)
            b = v.ljust(p.width, b"\0") if p.kind == "bytes" else v.to_bytes(8 if p.kind == "number" else 4, "big")
            row += bytes(255 - c for c in b) if p.reverse else b
        out[i, :len(row)] = np.frombuffer(row, np.uint8)
    return out


class _Rev:
    """a value whose order is turned round"""
    __slots__ = ("v",)

    def __init__(self, v):
        self.v = v

    def __lt__(self, other):
        return other.v < self.v

    def __eq__(self, other):
        return self.v == other.v


def order(records, cf):
    """sorted(range(n)) by (meta lines first, the tuple of parsed values, the record number).  A "bytes" value is compared as Python
    compares bytes, which is the order of its zero-padded form as long as the fields hold no NUL."""
    check(records, cf)

    def key(i):
        r = records[i]
        if is_meta(r, cf):
            return (0, (), i)
        vals = tuple(_Rev(v) if p.reverse else v for p, v in ((p, value(r, p, cf)) for p in cf.parts))
        return (1, vals, i)

    return sorted(range(len(records)), key=key)


def lexorder(keys):
    """np.lexsort over the big-endian uint64 columns of uint8 rows (n, W), W a multiple of 8: stable, the first column counts most"""
    keys = np.ascontiguousarray(keys, np.uint8)
    n, w = keys.shape
    if not n:
        return np.empty(0, np.int64)
    cols = keys.view(">u8").astype(np.uint64)
    return np.lexsort(cols.T[::-1]).astype(np.int64)

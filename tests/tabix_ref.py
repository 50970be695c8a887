"""The referee of the tabix tests: pure Python, written from the line model of the feature and
from the SAM specification section 5.3.  Per-line parse, reg2bin / reg2bins, chunks and linear index by the plain per-line algorithm,
brute-force overlap.  It works on the bytes the system gzip decodes and on the block headers of the BGZF file; it never calls the
code under test."""
import gzip
import struct

MAX_POS = 1 << 29
PRESETS = {"gff": (0, 1, 4, 5, ord("#"), 0), "bed": (0x10000, 1, 2, 3, ord("#"), 0), "vcf": (2, 1, 2, 0, ord("#"), 0)}


class RefBad(Exception):
    """the first line that cannot be indexed: its number and why (1 .. 4 as the feature numbers them, or "contig")"""

    def __init__(self, number, kind):
        super().__init__(number, kind)
        self.number, self.kind = number, kind


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def _coordinate(field):
    return int(field) if 1 <= len(field) <= 10 and field.isdigit() else None


def parse_line(raw, terminated, conf, number):
    """raw: the line's bytes without its delimiter; terminated: a delimiter follows.  -> ("skip",), ("bad", kind) or
    ("data", name, beg, end)"""
    fmt, cs, cb, ce, meta, skip = conf
    body = raw[:-1] if terminated and raw.endswith(b"\r") else raw
    if number < skip or not body or raw[0] == meta:
        return ("skip",)
    cols = body.split(b"\t")
    vcf = fmt & 0xFFFF == 2
    need = [cs, cb] + ([4] if vcf else [ce] if ce and ce != cb else [])
    if any(c > len(cols) for c in need):
        return ("bad", 1)
    name = cols[cs - 1]
    b = _coordinate(cols[cb - 1])
    if b is None:
        return ("bad", 2)
    if vcf:
        beg = b - 1
        end = beg + len(cols[3])
        if len(cols) >= 8:
            info, i, key = cols[7], 0, True
            while i < len(info):
                if key and info[i:i + 4] == b"END=":
                    j = i + 4
                    while j < len(info) and 48 <= info[j] <= 57:
                        j += 1
                    if j > i + 4 and (j == len(info) or info[j] == 59) and int(info[i + 4:j]) > beg:
                        end = int(info[i + 4:j])
                    break
                key = info[i] == 59
                i += 1
    else:
        beg = b if fmt & 0x10000 else b - 1
        if ce and ce != cb:
            e = _coordinate(cols[ce - 1])
            if e is None:
                return ("bad", 2)
            end = e
        else:
            end = beg + 1
    if end <= beg:
        end = beg + 1
    if beg < 0 or end > MAX_POS:
        return ("bad", 3)
    return ("data", name, beg, end)


def blocks_of(blob):
    """[(coffset, csize, isize)] of a BGZF file, from its headers and trailers"""
    out, at = [], 0
    while at < len(blob):
        xlen = struct.unpack_from("<H", blob, at + 10)[0]
        cur, end, bsize = at + 12, at + 12 + xlen, None
        while cur < end:
            si1, si2, slen = struct.unpack_from("<BBH", blob, cur)
            if (si1, si2, slen) == (66, 67, 2):
                bsize = struct.unpack_from("<H", blob, cur + 4)[0] + 1
            cur += 4 + slen
        out.append((at, bsize, struct.unpack_from("<I", blob, at + bsize - 4)[0]))
        at += bsize
    return out


class Voffsets:
    """uncompressed offset -> normalised virtual offset; behind the last data byte: where the next block starts (or the file's end)"""

    def __init__(self, blob):
        self.rows, u = [], 0
        self.after = 0
        for c, cs, isz in blocks_of(blob):
            if isz:
                self.rows.append((u, u + isz, c))
                self.after = c + cs
            u += isz
        self.total = u

    def __call__(self, u):
        if u >= self.total:
            return self.after << 16
        lo, hi = 0, len(self.rows)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if self.rows[mid][0] <= u:
                lo = mid
            else:
                hi = mid
        a, b, c = self.rows[lo]
        assert a <= u < b
        return c << 16 | (u - a)


def lines_of(data):
    """[(number, offset, raw without the delimiter, terminated)]; a non-empty remainder behind the last delimiter is a line"""
    out, at, n = [], 0, 0
    while at < len(data):
        e = data.find(b"\n", at)
        if e < 0:
            out.append((n, at, data[at:], False))
            break
        out.append((n, at, data[at:e], True))
        at, n = e + 1, n + 1
    return out


def table(blob, conf):
    """the per-line table: [(number, uncompressed offset, length with the delimiter, name, beg, end)] of the data lines; RefBad at the
    first line that cannot be indexed"""
    rows, prev, seen = [], None, set()
    for n, off, raw, term in lines_of(gzip.decompress(blob)):
        p = parse_line(raw, term, conf, n)
        if p[0] == "skip":
            continue
        if p[0] == "bad":
            raise RefBad(n, p[1])
        _, name, beg, end = p
        if prev is not None and prev[0] == name:
            if beg < prev[1]:
                raise RefBad(n, 4)
        else:
            if name in seen:
                raise RefBad(n, "contig")
            seen.add(name)
        prev = (name, beg)
        rows.append((n, off, len(raw) + (1 if term else 0), name, beg, end))
    return rows


def build(blob, conf):
    """-> (names, bins: per name {bin: [(v_beg, v_end), ...]}, linear: per name [voffset per 16 KiB window])"""
    v = Voffsets(blob)
    names, bins, linear, last = [], [], [], None
    for n, off, ln, name, beg, end in table(blob, conf):
        if not names or names[-1] != name:
            names.append(name)
            bins.append({})
            linear.append({})
            last = None
        b = reg2bin(beg, end)
        vb, ve = v(off), v(off + ln)
        if last == b:
            bins[-1][b][-1] = (bins[-1][b][-1][0], ve)
        else:
            bins[-1].setdefault(b, []).append((vb, ve))
        last = b
        for w in range(beg >> 14, ((end - 1) >> 14) + 1):
            linear[-1].setdefault(w, vb)
    filled = []
    for d in linear:
        arr, nxt = [0] * (max(d) + 1), None
        for w in range(max(d), -1, -1):
            nxt = d.get(w, nxt)
            arr[w] = nxt
        filled.append(arr)
    return names, bins, filled


def overlaps(rows, name, beg, end):
    """brute force: the rows of the per-line table that a region selects"""
    if end <= beg:
        end = beg + 1
    return [r for r in rows if r[3] == name and r[4] < end and r[5] > beg]

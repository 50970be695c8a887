"""Inputs of the tabix tests: a host-side BGZF writer (the system zlib; the tests of the host code need no GPU), generators of VCF,
BED and GFF text with the corner cases the feature names, random regions, and a stand-in for the two engine calls that computes
what they return with the referee (tests/tabix_ref.py), so that the planning and merging code of bgzf.py runs without a GPU."""
import struct
import types
import zlib

import numpy as np

import tabix_ref as R

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MAX_POS = 1 << 29


def host_bgzf(data, block_size, level=6, eof=True):
    out = []
    for i in range(0, len(data), block_size):
        chunk = data[i:i + block_size]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = co.compress(chunk) + co.flush()
        out.append(struct.pack("<4BI2BH2BHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(raw) + 25) + raw +
                   struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out) + (EOF_BLOCK if eof else b"")


def names_for(n):
    """n names: one of 1 byte, one of 200, the others ordinary"""
    return [b"1", b"L" * 200] + [b"chr%d" % i for i in range(2, n)]


def intervals(rng, n):
    """n intervals [beg, end), beg ascending with repeats: short ones, one per bin level (bin 0 included), the last ends at 2**29"""
    begs = np.sort(rng.integers(0, 1 << 27, n)).tolist()
    out = []
    for k, b in enumerate(begs):
        if k % 7 == 3 and out:
            b = out[-1][0]                                   # the same beg again
        out.append((b, b + int(rng.integers(1, 400))))
    for shift in (14, 17, 20, 23, 26):                       # one feature across a boundary of every level: shift 26 -> bin 0
        k = int(rng.integers(0, len(out)))
        edge = ((out[k][0] >> shift) + 1) << shift
        out[k] = (out[k][0], min(edge + 10, MAX_POS))
    out[-1] = (max(out[-1][0], MAX_POS - 5000), MAX_POS)
    return out


def make_text(kind, rng, n_names=6, per_name=60, crlf=False, final_newline=True, junk=0):
    """-> (text, conf, names)"""
    eol = b"\r\n" if crlf else b"\n"
    lines = [b"track line %d without tabs" % i for i in range(junk)]
    lines += [b"##header of a " + kind.encode(), b"#second header line"]
    names = names_for(n_names)
    for name in names:
        for k, (b, e) in enumerate(intervals(rng, per_name)):
            if k % 17 == 5:
                lines.append(b"#a comment in the middle")
            if k % 23 == 7:
                lines.append(b"")
            if kind == "bed":
                lines.append(b"%s\t%d\t%d\tf%d" % (name, b, e, k))
            elif kind == "gff":
                lines.append(b"%s\tsrc\tgene\t%d\t%d\t.\t+\t.\tID=g%d" % (name, b + 1, e, k))
            else:
                ref = b"ACGT"[:1 + k % 4]
                info = [b"END=%d" % e, b"DP=3;END=%d;AF=0.5" % e, b"DP=7", b"END=%d" % (b - 3 if b > 3 else 0), b"XEND=%d" % (e + 999),
                        b"DP=1;XEND=%d" % (e + 999), b"END=%dx;END=%d" % (e, e)][k % 7]
                long = e - b >= 1000                         # (the features that reach the upper bin levels need their END honoured)
                if long:
                    info = b"END=%d" % e if k % 2 else b"DP=3;END=%d" % e
                cols = [name, b"%d" % (b + 1), b"rs%d" % k, ref, b"T", b"50", b"PASS", info, b"GT", b"0/1"]
                lines.append(b"\t".join(cols[:5] if k % 11 == 9 and not long else cols))
    text = eol.join(lines) + (eol if final_newline else b"")
    return text, R.PRESETS[kind][:5] + (junk,), names


def regions_for(rng, rows, names, n=200):
    """n regions (name, beg, end): random ones, unknown names, beg == end, whole names, behind the last feature, and one that only
    bin-0 features of its name overlap"""
    out = []
    by_name = {}
    for r in rows:
        by_name.setdefault(r[3], []).append(r)
    for k in range(n):
        name = names[int(rng.integers(0, len(names)))]
        feats = by_name.get(name, [])
        mode = k % 8
        if mode == 0:
            out.append((b"nobody" + name[:3], 0, 1000))
        elif mode == 1 and feats:
            f = feats[int(rng.integers(0, len(feats)))]
            out.append((name, f[4], f[4]))
        elif mode == 2:
            out.append((name, 0, MAX_POS))
        elif mode == 3 and feats:
            last = max(f[5] for f in feats)
            out.append((name, min(last, MAX_POS - 1), MAX_POS) if last < MAX_POS else (name, MAX_POS, MAX_POS))
        elif mode == 4 and any(R.reg2bin(f[4], f[5]) == 0 for f in feats):
            f = [f for f in feats if R.reg2bin(f[4], f[5]) == 0][0]
            mid = ((f[4] >> 26) + 1) << 26
            out.append((name, mid + 1, mid + 2))
        elif feats:
            f = feats[int(rng.integers(0, len(feats)))]
            lo = max(0, f[4] - int(rng.integers(0, 20000)))
            out.append((name, lo, lo + int(rng.integers(1, 50000))))
        else:
            out.append((name, 5, 500))
    return out


NAME = np.dtype([("src_off", "<u8"), ("first", "<u8"), ("line", "<u8"), ("len", "<u4"), ("reserved", "<u4")])
BIN = np.dtype([("src_beg", "<u8"), ("src_end", "<u8"), ("first", "<u8"), ("lines", "<u8"), ("name", "<u4"), ("bin", "<u4")])
WIN = np.dtype([("src_off", "<u8"), ("name", "<u4"), ("window", "<u4")])
ROW = np.dtype([("src_off", "<u8"), ("len", "<u4"), ("region", "<u4")])


class FakeEngine:
    """ctx.bgzf_tabix and ctx.bgzf_fetch computed on the host (zlib and the referee's parse).  split_runs: name runs are broken at
    every skipped line, as the engine may break them."""

    def __init__(self, split_runs=False):
        self.split_runs, self.calls = split_runs, []

    @staticmethod
    def _scratch(data, members):
        data = bytes(data)
        size = int((members["out_off"] + members["out_len"]).max()) if len(members) else 0
        buf = bytearray(size)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        return bytes(buf)

    def bgzf_tabix(self, data, members, text_off, text_end, conf, delim, flags, line_base=0):
        text = self._scratch(data, members)
        self.calls.append((text_off, text_end, flags, line_base))
        tot = types.SimpleNamespace(seen=0, data=0, tail_off=text_end, bad_line=0, bad_src=0, bad_kind=0, first_beg=0, last_beg=0, covered=1)
        names, bins, wins, blob, at, n, prev, broke, d, maxw = [], [], [], [], text_off, 0, None, False, 0, -1
        bad = []
        while at < text_end:
            e = text.find(bytes([delim]), at, text_end)
            term = e >= 0
            if not term:
                if not flags & 4:
                    tot.tail_off = at
                    break
                e = text_end
            raw, start, ln = text[at:e], at, e - at + (1 if term else 0)
            at = e + 1
            p = R.parse_line(raw, term, conf, line_base + n)
            n += 1
            if p[0] == "skip":
                broke = self.split_runs
                continue
            if p[0] == "bad":
                bad.append((line_base + n - 1, p[1], start))
                continue
            _, name, beg, end = p
            if prev is not None and prev[0] == name and beg < prev[1]:
                bad.append((line_base + n - 1, 4, start))
            b, w = R.reg2bin(beg, end), (end - 1) >> 14
            name_new = prev is None or prev[0] != name or broke
            if name_new:
                names.append((start + _col_offset(raw, conf[1]), d, line_base + n - 1, len(name), 0))
                blob.append(name)
                maxw = -1
            if name_new or bins[-1][5] != b:
                bins.append([start, 0, d, 0, len(names) - 1, b])
            bins[-1][1], bins[-1][3] = start + ln, bins[-1][3] + 1
            if w > maxw:
                wins.append((start, len(names) - 1, w))
                maxw = w
            if d == 0:
                tot.first_beg = beg
            tot.last_beg, prev, broke, d = beg, (name, beg), False, d + 1
        tot.seen, tot.data = n, d
        if bad:
            tot.bad_line, tot.bad_kind, tot.bad_src = min(bad)
        return (0, np.zeros(len(members), np.int32), tot, np.array(names, NAME), b"".join(blob), np.array([tuple(x) for x in bins], BIN),
                np.array(wins, WIN))

    def bgzf_fetch(self, data, members, conf, delim, flags, names, regions, spans):
        text = self._scratch(data, members)
        self.calls.append(("fetch", len(members), len(spans)))
        rows, packed, srows = [], [], []
        for sp in spans:
            rg = regions[int(sp["region"])]
            want = bytes(names[int(rg["name_off"]):int(rg["name_off"] + rg["name_len"])])
            at, end, k = int(sp["text_off"]), int(sp["text_end"]), 0
            while at < end:
                e = text.find(bytes([delim]), at, end)
                term = e >= 0
                e = e if term else end
                p = R.parse_line(text[at:e], term, conf, 1 << 40)
                if p[0] == "data" and p[1] == want and p[2] < int(rg["end"]) and p[3] > int(rg["beg"]):
                    rows.append((at, e - at + (1 if term else 0), int(sp["region"])))
                    packed.append(text[at:e + (1 if term else 0)])
                    k += 1
                at = e + 1
            srows.append(k)
        tot = types.SimpleNamespace(matched=len(rows), bytes=sum(len(x) for x in packed))
        if flags & 8:
            rows, packed = [], []
        return (0, np.zeros(len(members), np.int32), np.zeros(len(spans), np.int32), np.array(srows, np.uint32), tot, np.array(rows, ROW),
                b"".join(packed))


def _col_offset(raw, col):
    """where column `col` (from 1) starts in the line"""
    at = 0
    for _ in range(col - 1):
        at = raw.index(b"\t", at) + 1
    return at

"""Inputs of the faidx tests: generators of FASTA text with the corner cases the feature names, random regions, and a stand-in for
the two engine calls (ctx.bgzf_faidx with its carry, ctx.bgzf_faidx_fetch) that computes what they return on the host, line after
line, so that the window loop and the planning code of bgzf.py run without a GPU."""
import types
import zlib

import numpy as np

from tabix_files import host_bgzf      # noqa: F401  (the tests take it from here)

ALPHABET = b"ACGTURYKMBVDHSWNacgturykmbvdhswn*-"      # every letter of the complement table in both cases, and bytes it leaves alone
ROW = np.dtype([("name_src", "<u8"), ("seq_src", "<u8"), ("line", "<u8"), ("bases", "<u8"), ("name_len", "<u4"), ("line_bases", "<u4"),
                ("line_width", "<u4"), ("reserved", "<u4")])
SPAN = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("n", "<u4"), ("col", "<u4"), ("line_bases", "<u4"), ("line_width", "<u4"),
                 ("flags", "<u4"), ("reserved", "<u4")])
OPEN, GAP, FINAL, RC, STALE = 1, 2, 4, 1, 4


def bases(rng, n):
    return bytes(np.frombuffer(ALPHABET, np.uint8)[rng.integers(0, len(ALPHABET), n)])


def record(name, seq, lb, eol, desc=b""):
    head = b">" + name + ((b" " + desc) if desc else b"")
    return [head] + [seq[i:i + lb] for i in range(0, len(seq), lb)]


def make_fasta(rng, lb, crlf=False, final_newline=True, trailing_empty=0, total=200_000):
    """-> text of about `total` bytes: sequences of LENGTH 0, 1, lb - 1, lb, lb + 1 and 5 lb, names of 1 and 200 bytes with and
    without a description, then ordinary ones"""
    eol = b"\r\n" if crlf else b"\n"
    lines = []
    special = [0, 1, max(lb - 1, 0), lb, lb + 1, 5 * lb]
    names = [b"1", b"L" * 200] + [b"s%d" % i for i in range(2, len(special))]
    for k, (name, n) in enumerate(zip(names, special)):
        lines += record(name, bases(rng, n), lb, eol, b"a description\twith a tab" if k % 2 else b"")
    k, size = len(special), sum(len(x) + len(eol) for x in lines)
    per = max(lb, (total - size) // 6)
    while size < total:
        n = int(rng.integers(per // 2, per + 1))
        rec = record(b"chr%d" % k, bases(rng, n), lb, eol, b"len=%d" % n if k % 3 == 0 else b"")
        lines += rec
        size += sum(len(x) + len(eol) for x in rec)
        k += 1
    text = eol.join(lines) + eol * (1 + trailing_empty)
    return text if final_newline else text[:-len(eol)]


def regions_for(rng, rows, n=300):
    """n regions (name, beg, end) over the .fai rows [(name, LENGTH, OFFSET, LINEBASES, LINEWIDTH)]: whole sequences, one base,
    across a line end, long ones (they cross blocks), clipped, empty, overlapping"""
    out = []
    full = [r for r in rows if r[1] > 0]
    for k in range(n):
        name, length, _, lb, _ = full[int(rng.integers(0, len(full)))] if k % 9 else rows[int(rng.integers(0, len(rows)))]
        mode = k % 8
        if mode == 0 or not length:
            out.append((name, 0, length + 5))
        elif mode == 1:
            b = int(rng.integers(0, length))
            out.append((name, b, b + 1))
        elif mode == 2:
            b = max(0, min(length - 1, int(rng.integers(1, max(2, length // max(lb, 1)))) * lb - int(rng.integers(1, 4))))
            out.append((name, b, b + int(rng.integers(2, 3 * lb + 3))))
        elif mode == 3:
            b = int(rng.integers(0, length))
            out.append((name, b, b + int(rng.integers(1, 9000))))
        elif mode == 4:
            out.append((name, max(0, length - 7), length + 1000))
        elif mode == 5:
            out.append((name, length + int(rng.integers(0, 3)), length + 50))
        elif mode == 6 and out:
            pn, pb, pe = out[-1]
            out.append((pn, pb + (pe - pb) // 2, pe + 3))
        else:
            b = int(rng.integers(0, length))
            out.append((name, b, b))
    return out


def _carry(last_line=0, first_bases=0, first_width=0, last_bases=0, last_width=0, flags=0, reserved=0):
    return types.SimpleNamespace(last_line=last_line, first_bases=first_bases, first_width=first_width, last_bases=last_bases,
                                 last_width=last_width, flags=flags, reserved=reserved)


class FakeEngine:
    """ctx.bgzf_faidx and ctx.bgzf_faidx_fetch computed on the host (zlib and a walk line after line)."""

    def __init__(self):
        self.calls, self.decoded = [], []

    @staticmethod
    def _scratch(data, members):
        data = bytes(data)
        size = int((members["out_off"] + members["out_len"]).max()) if len(members) else 0
        buf = bytearray(size)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        return bytes(buf)

    def bgzf_faidx(self, data, members, text_off, text_end, delim, flags, line_base=0, carry=None):
        assert delim == 10
        text = self._scratch(data, members)
        self.calls.append((text_off, text_end, flags, line_base))
        ci = carry if carry is not None else _carry()
        opened = bool(ci.flags & OPEN)
        first = (ci.first_bases, ci.first_width) if ci.first_width else None
        last = (ci.last_bases, ci.last_width) if ci.first_width else None
        last_line, gap, reserved = ci.last_line, bool(ci.flags & GAP), ci.reserved
        tot = types.SimpleNamespace(seen=0, records=0, tail_off=text_end, head_bases=0, name_bytes=0, bad_line=0, bad_src=0, bad_kind=0,
                                    covered=1, carry=None, head_line_bases=0, head_line_width=0)
        rows, blob, faults, starts = [], [], [], {}

        def close():
            if opened and first and last[0] > first[0]:
                faults.append((last_line, 3))

        at, no = text_off, line_base
        while at < text_end:
            e = text.find(b"\n", at, text_end)
            if e < 0:
                if not flags & FINAL:
                    tot.tail_off = at
                    break
                body, width, nxt = text[at:text_end], text_end - at, text_end
            else:
                body, width, nxt = text[at:e], e + 1 - at, e + 1
                if body.endswith(b"\r"):
                    body = body[:-1]
            starts[no] = at
            if body[:1] == b">":
                close()
                name = body[1:].replace(b"\t", b" ").replace(b"\r", b" ").split(b" ")[0]
                if not name:
                    faults.append((no, 1))
                rows.append([at + 1, nxt, no, 0, len(name), 0, 0, 0])
                blob.append(name)
                opened, first, last, last_line, gap, reserved = True, None, None, no, False, nxt - text_off
            else:
                if any(not 0x21 <= c <= 0x7E for c in body):
                    faults.append((no, 2))
                if not opened:
                    if body:
                        faults.append((no, 5))
                elif not body:
                    gap = True
                else:
                    if rows:
                        rows[-1][3] += len(body)
                    else:
                        tot.head_bases += len(body)
                    if first is None:
                        first = (len(body), width)
                        if rows:
                            rows[-1][5], rows[-1][6] = first
                        else:
                            tot.head_line_bases, tot.head_line_width = first
                    elif last != first:
                        faults.append((last_line, 3))
                    if gap:
                        faults.append((last_line + 1, 4))
                    last, last_line, gap, reserved = (len(body), width), no, False, nxt - text_off
            at, no = nxt, no + 1
        tot.seen, tot.records, tot.name_bytes = no - line_base, len(rows), sum(len(x) for x in blob)
        if flags & FINAL:
            close()
            tot.carry = _carry()
        elif not opened:
            tot.carry = _carry()
        else:
            f, l_ = first or (0, 0), last or (0, 0)
            tot.carry = _carry(last_line, f[0], f[1], l_[0], l_[1], OPEN | (GAP if gap else 0), reserved)
        if faults:
            tot.bad_line, tot.bad_kind = min(faults)
            tot.bad_src = starts.get(tot.bad_line, (1 << 64) - 1)
        return 0, np.zeros(len(members), np.int32), tot, np.array([tuple(r) for r in rows], ROW), b"".join(blob)

    def bgzf_faidx_fetch(self, data, members, spans, out_cap):
        text = self._scratch(data, members)
        self.calls.append(("fetch", len(members), len(spans)))
        self.decoded.append(len(members))
        out, sstat = bytearray(out_cap), np.zeros(len(spans), np.int32)
        comp = bytes.maketrans(b"ATUCGRYKMBVDHatucgrykmbvdh", b"TAAGCYRMKVBHDtaagcyrmkvbhd")
        for k, sp in enumerate(spans):
            n, col, lb, lw, src, dst = (int(sp[x]) for x in ("n", "col", "line_bases", "line_width", "src_off", "dst_off"))
            if n > 65536 or not lb or lw < lb or col >= lb or src < col or dst + n > out_cap:
                sstat[k] = 2
                continue
            got = bytes(text[src - col + (col + j) // lb * lw + (col + j) % lb] for j in range(n)) if n and src - col + (col + n - 1) // lb * lw + (col + n - 1) % lb < len(text) else None
            if got is None and n:
                sstat[k] = 2
                continue
            got = got or b""
            if any(not 0x21 <= c <= 0x7E for c in got):
                sstat[k] = STALE
            out[dst:dst + n] = got.translate(comp)[::-1] if int(sp["flags"]) & RC else got
        return np.zeros(len(members), np.int32), sstat, bytes(out)

"""Span tables from the vectors of tests/deflate_build.py: a vector cut at some of its block headers is a list of spans, each with
the window, the bytes and the CRC-32 a seek-point index would record for it -- all from the builder's own plaintext and
block_bits, none from a decoder.  tests/test_cpu_span_vectors.py proves every span against the system zlib.  Plain Python: holds
no test, no GPU code and no ctypes (the GPU test turns the records into the engine's table).  Not a conftest."""
import zlib
from collections import namedtuple

import deflate_build as B

WIN = 32768
PAD = 64                       # ZA_SPAN_PAD: zero bytes behind the last span's input

# in_bit / end_bit: the span's first block header and its end (the next cut's header; a final span: the stream's end rounded up
# to a byte), as bits of the stream that spans_of was given the start of; window / expect: bytes-like
Span = namedtuple("Span", "in_bit end_bit window expect crc final")
# ... and laid into the buffers of pack(): absolute bits, the window as a place in the windows blob; vec / first: the vector's
# name and the index of the span's first block
Placed = namedtuple("Placed", "in_bit end_bit win_off win_len expect crc final vec first")
Packed = namedtuple("Packed", "data spans windows")

_bits_cache = {}


def out_lens(blocks):
    """bytes that each VALID block produces, from its tokens"""
    return [len(b.data) if isinstance(b, B.Stored) else sum(t.length if isinstance(t, B.M) else 1 for t in b.tokens) for b in blocks]


def _bits(v, lead):
    """block_bits of the vector written behind `lead` < 8 bits, and those bytes (computed once per vector and lead)"""
    key = (v.name, len(v.blob), lead)
    if key not in _bits_cache:
        w, hdr = B.BitWriter(), []
        w.bits(0x55 & ((1 << lead) - 1), lead)
        for i, b in enumerate(v.blocks):                # (block_bits and assemble in one pass; the CPU test compares them)
            hdr.append(w.bitlen)
            b.write(w, i == len(v.blocks) - 1)
        _bits_cache[key] = (hdr, w.bitlen, w.getvalue())
    return _bits_cache[key]


def spans_of(v, cuts, start=0):
    """The spans that cutting the valid vector `v` at the block indexes `cuts` makes (block 0 is always a cut), the stream
    beginning at bit `start` -> [Span]"""
    hdr, end, _ = _bits(v, start & 7)
    base = start - (start & 7)
    cuts = sorted(set(cuts) | {0})
    assert 0 <= cuts[0] and cuts[-1] < len(v.blocks)
    z = len(v.zdict)
    hist = memoryview(bytes(v.zdict) + v.expect)
    pos = [0]
    for n in out_lens(v.blocks):
        pos.append(pos[-1] + n)
    assert pos[-1] == len(v.expect)
    out = []
    for a, b in zip(cuts, cuts[1:] + [len(v.blocks)]):
        final = b == len(v.blocks)
        lo, hi = z + pos[a], z + pos[b]
        expect = hist[lo:hi]
        out.append(Span(base + hdr[a], base + (((end + 7) & ~7) if final else hdr[b]), hist[max(0, lo - WIN):lo], expect,
                        zlib.crc32(expect), final))
    return out


def pack(items, lead_bits):
    """items = [(vector, cuts)]: every vector's stream written behind `lead_bits` junk bits of a byte of its own, one after the
    other, PAD zero bytes at the end; the windows blob holds each vector's zdict + plaintext ONCE, and a span's window is a
    slice of it.  -> Packed(data, [Placed] in the order of items and cuts, windows)"""
    assert 0 <= lead_bits < 8
    data, wins, spans = bytearray(), bytearray(), []
    for v, cuts in items:
        _, end, blob = _bits(v, lead_bits)
        z, hbase = len(v.zdict), len(wins)
        wins += v.zdict
        if not B.is_valid(v):
            # an invalid vector is ONE span up to the end of its bytes, with no expectation
            wl = min(WIN, z)
            spans.append(Placed(8 * len(data) + lead_bits, 8 * len(data) + ((end + 7) & ~7), hbase + z - wl, wl, None, 0, True, v.name, 0))
            data += blob
            continue
        wins += v.expect
        cuts = sorted(set(cuts) | {0})
        at = z
        for s, first in zip(spans_of(v, cuts, 8 * len(data) + lead_bits), cuts):
            wl = len(s.window)
            assert bytes(wins[hbase + at - wl:hbase + at]) == bytes(s.window) and wl == min(WIN, at)
            spans.append(Placed(s.in_bit, s.end_bit, hbase + at - wl, wl, bytes(s.expect), s.crc, s.final, v.name, first))
            at += len(s.expect)
        data += blob
    return Packed(bytes(data) + bytes(PAD), spans, bytes(wins))

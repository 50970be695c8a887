"""Seek-point index and span decoder on the GPU (zlib_ng_amd/gzip_index.py, za_k_inflate_spans): files of other writers (the
stdlib gzip / zlib as the referee) and of this package, random reads, whole-file decodes in one launch, seeking readers, and
corrupted data that must never come back as wrong bytes."""
import gzip
import io
import os
import random
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN, heldout_corpora
from zlib_ng_amd import _lib, devmem, gzip_index, gzip_ng, gzip_ng_threaded, zlib_ng

pytestmark = pytest.mark.gpu

SPACING = 256 << 10
FAIL = (zlib_ng.error, gzip.BadGzipFile, EOFError)


def _gz(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    return c.compress(data) + c.flush()


def _member_with_all_header_fields(data):
    hdr = b"\x1f\x8b\x08" + bytes([4 | 8 | 16 | 2]) + b"\0\0\0\0\0\xff"
    hdr += struct.pack("<H", 6) + b"AB\x02\0xy" + b"name.txt\0" + b"a comment\0"
    hdr += struct.pack("<H", zlib.crc32(hdr) & 0xFFFF)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return hdr + c.compress(data) + c.flush() + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


@pytest.fixture(scope="module")
def big():
    """At least 32 MiB of the held-out corpora, one after another."""
    parts, n = [], 0
    corp = list(heldout_corpora().values())
    while n < (32 << 20) + 12345:
        for c in corp:
            parts.append(c)
            n += len(c)
    return b"".join(parts)[:(32 << 20) + 12345]


@pytest.fixture(scope="module")
def files(tmp_path_factory, fastq, big):
    d = tmp_path_factory.mktemp("gzindex")
    rnd = random.Random(7)
    out = {}

    def put(name, blob, data):
        p = str(d / (name + ".gz"))
        with open(p, "wb") as f:
            f.write(blob)
        out[name] = (p, data)
    for lv in (1, 6, 9):
        put(f"fastq_l{lv}", gzip.compress(fastq, lv, mtime=0), fastq)
    put("big_l6", gzip.compress(big, 6, mtime=0), big)
    small = big[:3 << 20]
    put("level0", _gz(small, 0), small)
    put("fixed", _gz(small, 6, zlib.Z_FIXED), small)
    # many members: empty and tiny ones, NUL padding between some
    blob, data = b"", b""
    for k in range(40):
        n = rnd.choice([0, 1, 7, 100, 5000, 300000])
        piece = fastq[k * 1000:k * 1000 + n]
        blob += gzip.compress(piece, rnd.choice([1, 6, 9]), mtime=0) + b"\0" * rnd.choice([0, 0, 3, 17])
        data += piece
    put("members", blob, data)
    with open(os.path.join(GOLDEN, "test.fastq.bgzip.gz"), "rb") as f:
        put("bgzf", f.read(), fastq)
    p = str(d / "threaded.gz")
    with gzip_ng_threaded.open(p, "wb") as f:
        f.write(small)
    with open(p, "rb") as f:
        blob = f.read()
    put("threaded", blob, small)
    put("header_fields", _member_with_all_header_fields(fastq), fastq)
    return out


NAMES = ["fastq_l1", "fastq_l6", "fastq_l9", "level0", "fixed", "members", "bgzf", "threaded", "header_fields"]


def _largest_span(idx):
    return max([p.out_len for p in idx.points] + [0])


def _check_points(idx, data, spacing):
    assert idx.size == len(data)
    pts = idx.points
    assert all(a.in_bit < b.in_bit and a.out_off <= b.out_off for a, b in zip(pts, pts[1:]))
    assert sum(p.out_len for p in pts) == len(data)
    for p in pts:
        assert p.end_bit <= idx.file_size * 8


@pytest.mark.parametrize("name", NAMES)
def test_index_reads(files, name):
    path, data = files[name]
    ctx = zlib_ng._ctx()
    idx = gzip_index.build(path, spacing=SPACING)
    _check_points(idx, data, SPACING)
    # (the spans follow the spacing: a span is the output of one window, sized from the ratio seen so far)
    assert len(idx.points) >= len(data) // (4 * SPACING)
    rnd = random.Random(zlib.crc32(name.encode()))
    n = len(data)
    starts = [p.out_off for p in idx.points]
    reads = [(0, 0), (n - 1, 1), (n - 1, 100), (n, 10), (n + 5000, 10), (0, n + 7)]
    reads += [(max(0, s - 3), 4096) for s in rnd.sample(starts, min(20, len(starts)))]
    while len(reads) < 200:
        o = rnd.randrange(n + 100)
        reads.append((o, rnd.choice([0, 1, 17, 4096, 65536, 700000])))
    with open(path, "rb") as f:
        for o, k in reads:
            assert idx.read_at(f, o, k) == data[o:o + k], (o, k)
        some = reads[6:60]
        ctx.span_stats(reset=True)
        got = idx.read_ranges(f, some)
        spans, _ = ctx.span_stats(reset=True)
        assert got == [data[o:o + k] for o, k in some]
        need = {i for o, k in some for i in idx._spans_for(o, k) if idx.points[i].kernel}
        if len(need) != 1:
            assert spans == len(need)          # one launch, each needed span once
        whole = idx.decompress(f)
        spans, _ = ctx.span_stats(reset=True)
    assert whole == data
    kern = sum(1 for p in idx.points if p.kernel and p.out_len)
    if kern != 1:
        assert spans == kern
    # save / load
    buf = io.BytesIO()
    idx.save(buf)
    back = gzip_index.GzipIndex.load(io.BytesIO(buf.getvalue()))
    assert back.size == idx.size and [p.fields() for p in back.points] == [p.fields() for p in idx.points]
    with open(path, "rb") as f:
        assert back.read_at(f, n // 2, 5000) == data[n // 2:n // 2 + 5000]
    # the seeking reader
    with gzip_ng.open(path, "rb", index=back) as g:
        assert g.seek(0, 2) == n
        for _ in range(100):
            o = rnd.randrange(n + 10)
            k = rnd.choice([1, 100, 4096, 100000])
            assert g.seek(o) == o
            assert g.read(k) == data[o:o + k], (o, k)
        assert g.seek(-10, 2) == n - 10 and g.read() == data[-10:]
        g.seek(0)
        assert g.read(1000) == data[:1000]


def test_spans_in_one_launch(files):
    path, data = files["big_l6"]
    ctx = zlib_ng._ctx()
    idx = gzip_index.build(path, spacing=64 << 10)
    _check_points(idx, data, 64 << 10)
    kern = sum(1 for p in idx.points if p.kernel and p.out_len)
    assert kern >= 300
    ctx.span_stats(reset=True)
    ctx.kernel_times(reset=True)
    with open(path, "rb") as f:
        assert idx.decompress(f) == data
    spans, nbytes = ctx.span_stats(reset=True)
    assert spans == kern and nbytes == len(data)


def test_seek_near_the_end_decodes_little(files, monkeypatch):
    path, data = files["big_l6"]
    idx = gzip_index.build(path, spacing=1 << 20)
    seen = []
    orig = _lib.Context.gunzip_stream

    def counting(self, state, buf, out_cap, last, view=False, into=None):
        r = orig(self, state, buf, out_cap, last, view=view, into=into)
        seen.append(len(r[1]))
        return r
    monkeypatch.setattr(_lib.Context, "gunzip_stream", counting)
    with gzip_ng.open(path, "rb", index=idx) as g:
        assert g.seek(0, 2) == len(data)
        assert sum(seen) == 0
        o = len(data) - (1 << 20)
        g.seek(o)
        assert g.read(4096) == data[o:o + 4096]
    assert sum(seen) <= 2 * _largest_span(idx)
    assert sum(seen) < len(data) // 8


def test_index_of_another_file_is_refused(files):
    idx = gzip_index.build(files["fastq_l6"][0], spacing=SPACING)
    other = files["fastq_l9"][0]
    with pytest.raises(ValueError):
        gzip_ng.open(other, "rb", index=idx)
    with pytest.raises(ValueError):
        idx.read_at(other, 0, 100)
    with pytest.raises(ValueError):
        idx.decompress(other)


def test_flipped_bit_never_returns_wrong_bytes(files, tmp_path):
    path, data = files["fastq_l6"]
    idx = gzip_index.build(path, spacing=SPACING)
    blob = bytearray(open(path, "rb").read())
    # a bit in the middle of a block point's span, away from the bytes the index is bound to
    mid = [i for i, p in enumerate(idx.points) if p.is_block and p.in_bit // 8 > (1 << 16) + 100 and p.end_bit // 8 < len(blob) - (1 << 16) - 100]
    assert mid
    p = idx.points[mid[0]]
    at = (p.in_bit + p.end_bit) // 16
    blob[at] ^= 0x10
    bad = str(tmp_path / "bad.gz")
    with open(bad, "wb") as f:
        f.write(blob)
    o = p.out_off + p.out_len // 2
    for call in (lambda: idx.read_at(bad, o, 100), lambda: idx.read_ranges(bad, [(0, 10), (o, 100)]), lambda: idx.decompress(bad)):
        try:
            got = call()
        except FAIL:
            continue
        pytest.fail(f"a corrupted span came back as {len(got) if isinstance(got, bytes) else '?'} bytes")
    with gzip_ng.open(bad, "rb", index=idx) as g:
        with pytest.raises(FAIL):
            g.seek(o)
            g.read(100)


def test_span_dev_with_a_moved_start(files):
    path, data = files["fastq_l6"]
    ctx = zlib_ng._ctx()
    idx = gzip_index.build(path, spacing=SPACING)
    blob = open(path, "rb").read()
    kern = [i for i, p in enumerate(idx.points) if p.kernel and p.out_len]
    assert len(kern) >= 4
    wins = b"".join(idx.window(i) for i in kern) or b"\0"
    spans = (_lib.Span * len(kern))()
    wo = oo = 0
    for j, i in enumerate(kern):
        p = idx.points[i]
        spans[j] = _lib.Span(p.data_bit, p.end_bit, wo, oo, p.win_len, p.out_len, p.span_crc, 0)
        wo += p.win_len
        oo += p.out_len
    victim = 2
    spans[victim].in_bit += 1                   # off its block boundary; the rest of the table as it was
    d_in = devmem.from_host(ctx, blob + b"\0" * 64)
    d_tab = devmem.from_host(ctx, bytes(spans))
    d_win = devmem.from_host(ctx, wins)
    d_out = devmem.empty(ctx, oo + 64)
    d_st = devmem.empty(ctx, 4 * len(kern))
    ctx.inflate_spans_dev(d_in.data_ptr(), len(blob) + 64, d_tab.data_ptr(), len(kern), d_win.data_ptr(), len(wins), d_out.data_ptr(),
                          oo, d_st.data_ptr())
    st = d_st.cpu().view(np.int32)
    out = d_out.cpu().tobytes()
    assert st[victim] != _lib.SPAN_OK
    assert all(s == _lib.SPAN_OK for j, s in enumerate(st) if j != victim)
    for j, i in enumerate(kern):
        if j != victim:
            p = idx.points[i]
            assert out[spans[j].out_off:spans[j].out_off + p.out_len] == data[p.out_off:p.out_off + p.out_len]
    # a table entry that points outside the buffers is refused on the device, not followed
    spans[victim].in_bit = (len(blob) + 100) * 8
    spans[victim].end_bit = spans[victim].in_bit + 8
    d_tab2 = devmem.from_host(ctx, bytes(spans))
    ctx.inflate_spans_dev(d_in.data_ptr(), len(blob) + 64, d_tab2.data_ptr(), len(kern), d_win.data_ptr(), len(wins), d_out.data_ptr(),
                          oo, d_st.data_ptr())
    st = d_st.cpu().view(np.int32)
    assert st[victim] == _lib.SPAN_DATA and all(s == _lib.SPAN_OK for j, s in enumerate(st) if j != victim)

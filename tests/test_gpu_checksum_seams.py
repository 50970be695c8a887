"""Every CRC-32 / Adler-32 implementation of the engine against zlib, at its own seams (DESIGN.md section 4 lists them).  The
inputs are tests/checksum_inputs.py's: bytes of 128 and more, all-0xFF, zeros (only the x^(8 len) factors), a ramp, and a needle
whose Adler-32 counts the bytes behind it; the lengths sit around every segment and span size.  All comparisons are for equality.
The write side is read by CPython's zlib / gzip (which verify the trailers), the read side is shown to accept right trailers on
the intended path and to reject a wrong one."""
import ctypes as C
import gzip
import io
import struct
import zlib

import numpy as np
import pytest

import checksum_inputs as K

pytestmark = pytest.mark.gpu

THREE = ("ff", "high", "rand")


@pytest.fixture(scope="module")
def mods():
    from zlib_ng_amd import _lib, batch, devmem, gzip_index, zlib_ng
    return _lib, batch, devmem, gzip_index, zlib_ng


# ---------------------------------------------------------------------------------------------------------------------------
# helpers: gzip framing by hand
# ---------------------------------------------------------------------------------------------------------------------------
def _raw(data, level=1):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def _member(data, level=1, name=b"", hcrc=False, extra=b""):
    """one gzip member written with CPython's zlib: optional FEXTRA, FNAME and FHCRC (CRC-32 of the header, low 16 bits)"""
    flg = (4 if extra else 0) | (8 if name else 0) | (2 if hcrc else 0)
    h = b"\x1f\x8b\x08" + bytes([flg]) + bytes(4) + b"\x00\xff"
    if extra:
        h += struct.pack("<H", len(extra)) + extra
    if name:
        h += name + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + _raw(data, level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def _bgzf_member(data, level=1):
    body = _raw(data, level)
    size = 18 + len(body) + 8
    assert size <= 65536
    return _member(data, level, extra=b"BC" + struct.pack("<HH", 2, size - 1))


def _walk(stream):
    """the members of a gzip stream -> [(start, first deflate byte, first trailer byte, payload length)]"""
    out, pos = [], 0
    while pos < len(stream):
        assert stream[pos:pos + 3] == b"\x1f\x8b\x08", pos
        flg, p = stream[pos + 3], pos + 10
        if flg & 4:
            p += 2 + struct.unpack_from("<H", stream, p)[0]
        for bit in (8, 16):
            if flg & bit:
                p = stream.index(b"\0", p) + 1
        if flg & 2:
            p += 2
        d = zlib.decompressobj(-15)
        n = len(d.decompress(stream[p:]))
        assert d.eof
        end = len(stream) - len(d.unused_data)
        assert struct.unpack_from("<I", stream, end + 4)[0] == n & 0xFFFFFFFF
        out.append((pos, p, end, n))
        pos = end + 8
    return out


def _flip(stream, at, bit):
    b = bytearray(stream)
    b[at + (bit >> 3)] ^= 1 << (bit & 7)
    return bytes(b)


def _first_mid_last(n):
    return sorted({0, n // 2, n - 1})


# ---------------------------------------------------------------------------------------------------------------------------
# 1. za_k_checksum through the staged calls
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_checksum_kernel_staged(mods, name):
    """zlib_ng.crc32 / adler32: every pattern, every length of CK_LENS (the thread's piece is 64, 128, 256 and 512 bytes; one,
    two, three and four spans), every seed"""
    zlib_ng = mods[4]
    for n in K.CK_LENS:
        d = K.PATTERNS[name](n)
        for s in K.CRC_SEEDS:
            assert zlib_ng.crc32(d, s) == zlib.crc32(d, s), (name, n, hex(s))
        for s in K.ADLER_SEEDS:
            assert zlib_ng.adler32(d, s) == zlib.adler32(d, s), (name, n, hex(s))


@pytest.mark.parametrize("s", sorted(K.CK_NEEDLE))
def test_checksum_kernel_needle(mods, ctx, s):
    """a single 0x01 around the first and the last piece of s bytes, at the length that gives a thread s bytes: Adler's b counts
    the bytes behind it (a fold that is off by one byte is off by one), the CRC is x^(8 (n - 1 - k)) times a constant"""
    zlib_ng = mods[4]
    n = K.CK_NEEDLE[s]
    for m in (n, n - 1) + ((n + 1,) if s == 512 else ()):      # (whole pieces; a short last piece; for 512 a second span)
        assert 256 * (s // 2) < min(m, 131072) <= 256 * s
        for k in K.needle_positions(m, s):
            d = K.needle(m, k)
            for seed in K.ADLER_SEEDS:
                assert zlib_ng.adler32(d, seed) == zlib.adler32(d, seed), (s, m, k, hex(seed))
            for seed in K.CRC_SEEDS:
                assert ctx.crc32(d, seed) == zlib.crc32(d, seed), (s, m, k, hex(seed))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. za_k_checksum on a device pointer of any alignment
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_checksum_kernel_device_pointer(mods, ctx, name):
    """zngamd_crc32_dev(ptr + o, n): the byte steps up to the first 16-byte boundary, in the first thread's piece and in the rest"""
    devmem = mods[2]
    big = max(K.CK_OFFSET_LENS)
    d = K.PATTERNS[name](big)
    buf = devmem.DeviceBuffer(ctx, big + 16 + 64)
    assert buf.ptr % 16 == 0
    out = C.c_uint32(0)
    for o in K.CK_OFFSETS:
        buf[:] = 0xA5
        buf[o:o + big] = d
        for n in K.CK_OFFSET_LENS:
            for s in K.CRC_SEEDS:
                assert ctx.L.zngamd_crc32_dev(ctx.h, s, buf.vp(o), n, C.byref(out)) == 0, ctx.err()
                assert out.value == zlib.crc32(d[:n], s), (name, o, n, hex(s))
    buf.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. inflate_raw: the small call (checksum kernel with the length on the device, spans behind the data's end) and the large one
# ---------------------------------------------------------------------------------------------------------------------------
RAW_OUT = (16385, 65537, 131073)


@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_inflate_raw_checksums(mods, ctx, name):
    """Streams of CPython's zlib (raw, level 1).  Small form: input under 64 KiB and out_cap up to 512 KiB -- out_cap of the
    output + 16 and of 524 288, which puts up to three spans behind the data's end; 131 073 bytes outgrow the decoder's image of
    86 016 bytes, the call runs a second time and that pass's sums are the ones returned.  Large form: out_cap above 512 KiB."""
    _lib = mods[0]
    small = 0
    for n in RAW_OUT + (3 * 131072 + 77,):
        d = K.PATTERNS[name](n)
        comp = _raw(d)
        for cap in (n + 16, 524288, (512 << 10) + 4096):
            if cap < n:
                continue
            ctx.decode_paths(True)
            code, out, used, crc, ad = ctx.inflate_raw(comp, cap)
            t = (name, n, cap, len(comp))
            assert code == _lib.STREAM_END and used == len(comp) and out == d, t
            assert crc == zlib.crc32(d), t
            assert ad == zlib.adler32(d), t
            paths = ctx.decode_paths(True)
            assert paths["sequential"] + paths["chunked"] == 1, (t, paths)
            if len(comp) < 65536 and cap <= 524288:
                small += n in RAW_OUT
                assert paths["sequential"] == 1, (t, paths)      # (the small form is one wavefront)
    # what compresses takes the small form at all three sizes and both capacities
    if name in ("ff", "zero", "ramp"):
        assert small == 2 * len(RAW_OUT)
    assert small >= 2, name


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the compressor's unit CRCs
# ---------------------------------------------------------------------------------------------------------------------------
def _parse_configs():
    from zlib_ng_amd import _lib
    D = _lib.STRATEGY_DEFAULT
    # za_k_unit_crc | za_k_parse<false> without and with the dynamic programme | za_k_parse<true>: no level has a shortest match
    # above 3 in the level table -- the launch plan takes it under Z_FILTERED (shortest match 6) | za_k_parse_rle<true> / <false>
    return [("level0", 0, D), ("level1", 1, D), ("level6", 6, D), ("level9", 9, D), ("filtered6", 6, _lib.STRATEGY_FILTERED),
            ("rle6", 6, _lib.STRATEGY_RLE), ("huffman6", 6, _lib.STRATEGY_HUFFMAN_ONLY)]


@pytest.mark.parametrize("name", ["ff", "high", "rand", "ramp"])
@pytest.mark.parametrize("config", _parse_configs(), ids=lambda c: c[0])
def test_compressor_unit_crcs(ctx, config, name):
    """one deflate_blocks call: every length of SSHIFT_LENS (segments of 32 bytes .. 2 KiB, each threshold with its neighbours) a
    unit of its own, laid end to end -- so most units start unaligned; level 0 also SEG2K_LENS"""
    tag, level, strategy = config
    lens = K.SSHIFT_LENS + (K.SEG2K_LENS if level == 0 else ())
    buf = K.PATTERNS[name](sum(lens))
    blocks, at = [], 0
    for n in lens:
        blocks.append((at, n, 0, 0))
        at += n
    big = max(lens)
    outs, crcs, ovf = ctx.deflate_blocks(buf, blocks, level, big + big // 8 + 64, strategy=strategy)
    assert not ovf and all(o is not None for o in outs)
    for (off, n, _, _), crc, out in zip(blocks, crcs, outs):
        assert crc == zlib.crc32(buf[off:off + n]), (tag, name, n, off)
    # (the units are what they should be: a sample of them inflates to its bytes)
    for i in (0, len(blocks) // 2, len(blocks) - 1):
        off, n = blocks[i][:2]
        assert zlib.decompress(outs[i] + b"\x03\x00", -15) == buf[off:off + n], (tag, name, n)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. trailers the engine writes, read by CPython's zlib
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE)
def test_written_trailers(mods, ctx, name):
    _lib, batch, devmem, gzip_index, zlib_ng = mods
    f = K.PATTERNS[name]
    for wbits in (15, 31):
        for n in (1, 16385, 65537, 131073, 262145):
            assert zlib.decompress(zlib_ng.compress(f(n), 6, wbits), wbits) == f(n), (name, wbits, n)
    for bs in (2049, 32769, 131072):
        d = f(3 * bs + 77)
        stream = bytes(ctx.gzip_members(d, bs, 6))
        assert gzip.decompress(stream) == d, (name, bs)
        assert [m[3] for m in _walk(stream)] == [bs, bs, bs, 77]
    for bs in (4097, 65280):
        d = f(3 * bs + 77)
        stream, table = ctx.bgzf_compress(d, bs, 6)
        assert gzip.decompress(stream) == d, (name, bs)
        assert [m[3] for m in _walk(stream)] == [bs, bs, bs, 77, 0] and len(table) == 5
    items = [f(n) for n in K.ADLER1K_LENS + (131073, 262145)]
    for wbits in (15, 31):
        for level in (6, 9):
            outs = batch.compress(items, level, wbits)
            for a, b in zip(items, outs):
                assert zlib.decompress(b, wbits) == a, (name, wbits, level, len(a))


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the verifiers accept right trailers on their own path and reject wrong ones
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE)
def test_indexed_members_verify(mods, ctx, name):
    """(a) za_k_inflate_members on members written by gzip_members, three members of every length of LANE32_LENS.  Members of
    noise are written as stored blocks, which the indexed decoder hands to the sequential reader: for them the path asserted is
    that one.  A member whose stored CRC-32 has one bit flipped fails the kernel's check; gunzip then counts no member as
    indexed and gives the whole buffer to the sequential reader, whose own check (za_k_checksum against the trailer) is the error
    that reaches the caller: ZNGAMD_E_GZ_CRC, with the members in front of the bad one decoded."""
    _lib = mods[0]
    f = K.PATTERNS[name]
    for n in K.LANE32_LENS:
        d = f(3 * n)
        stream = bytes(ctx.gzip_members(d, n, 6))
        mem = _walk(stream)
        assert [m[3] for m in mem] == [n, n, n]
        stored = [(stream[m[1]] >> 1) & 3 == 0 for m in mem]
        ctx.decode_paths(True)
        code, out, nm = ctx.gunzip(stream, len(d))
        paths = ctx.decode_paths(True)
        assert (code, nm) == (0, 3) and out == d, (name, n)
        if not any(stored):
            assert paths["indexed"] == 3, (name, n, paths)
        else:
            assert name == "rand" and paths["indexed"] == 0 and sum(paths.values()) == 3, (name, n, paths, stored)
        for j in _first_mid_last(3):
            bad = _flip(stream, mem[j][2], (n + 5 * j) % 32)
            code, out, nm = ctx.gunzip(bad, len(d))
            paths = ctx.decode_paths(True)
            assert code == _lib.E_GZ_CRC, (name, n, j, code)
            assert nm == j and out[:j * n] == d[:j * n] and paths["indexed"] == 0, (name, n, j, nm, paths)


@pytest.mark.parametrize("name", THREE)
def test_bgzf_members_verify(mods, ctx, name):
    """(b) za_k_inflate_serial_members (za_wave_crc32) on BGZF members written with CPython's zlib and a hand-written 'BC' field"""
    _lib = mods[0]
    f = K.PATTERNS[name]
    for n in [x for x in K.SEG2K_LENS if x <= 65280] + [65280]:
        level = 0 if name == "rand" and n > 60000 else 1      # (a member is at most 64 KiB)
        d = f(3 * n)
        stream = b"".join(_bgzf_member(d[i * n:(i + 1) * n], level) for i in range(3)) + _bgzf_member(b"")
        mem = _walk(stream)
        assert gzip.decompress(stream) == d
        ctx.decode_paths(True)
        code, out, nm = ctx.gunzip(stream, len(d))
        paths = ctx.decode_paths(True)
        assert (code, nm) == (0, 4) and out == d, (name, n)
        assert paths == {"indexed": 0, "bgzf": 4, "chunked": 0, "sequential": 0}, (name, n, paths)
        for j in _first_mid_last(3):
            bad = _flip(stream, mem[j][2], (n + 7 * j) % 32)
            code, out, nm = ctx.gunzip(bad, len(d))
            paths = ctx.decode_paths(True)
            assert code == _lib.E_GZ_CRC and nm == j and out == d[:j * n], (name, n, j, code, nm)
            assert paths == {"indexed": 0, "bgzf": j, "chunked": 0, "sequential": 0}, (name, n, j, paths)


@pytest.mark.parametrize("name,size", [("rand", 1 << 20), ("high", 640 << 10)])
def test_spans_verify(mods, ctx, name, size):
    """(c) za_k_inflate_spans: an index over a gzip file of CPython's, reads across every point, then one span's recorded CRC-32
    altered in a saved index (its own CRC made right again): the read is refused"""
    _lib, batch, devmem, gzip_index, zlib_ng = mods
    d = K.PATTERNS[name](size)
    blob = _member(d, 6, name=b"x")
    idx = gzip_index.build(io.BytesIO(blob), spacing=64 << 10)
    kern = [i for i, p in enumerate(idx.points) if p.kernel and p.out_len]
    assert len(kern) >= 4 and sum(idx.points[i].out_len for i in kern) == size
    f = io.BytesIO(blob)
    ctx.span_stats(reset=True)
    assert idx.decompress(f) == d
    assert ctx.span_stats(reset=True) == (len(kern), size)
    for i in kern[1:]:
        o = idx.points[i].out_off
        assert idx.read_at(f, o - 100, 300) == d[o - 100:o + 200], (name, i)
    assert ctx.span_stats(reset=True)[0] == 2 * (len(kern) - 1)
    for i in (kern[0], kern[len(kern) // 2], kern[-1]):
        p = idx.points[i]
        assert p.span_crc == zlib.crc32(d[p.out_off:p.out_off + p.out_len])
        p.span_crc ^= 1 << (i % 32)
        saved = idx.to_bytes()
        p.span_crc ^= 1 << (i % 32)
        back = gzip_index.GzipIndex.from_bytes(saved)
        with pytest.raises(zlib_ng.BadGzipFile, match="CRC mismatch"):
            back.read_at(f, max(p.out_off - 100, 0), p.out_len + 200)
        # (the spans beside it are still read)
        other = kern[1] if i == kern[0] else kern[0]
        q = idx.points[other]
        assert back.read_at(f, q.out_off + 1, 100) == d[q.out_off + 1:q.out_off + 101]
    with pytest.raises(ValueError, match="CRC mismatch"):
        gzip_index.GzipIndex.from_bytes(_flip(idx.to_bytes(), 100, 3))


def _batch_call(_lib, ctx, pieces, wbits, sizes):
    """the pieces at odd offsets of one buffer, every item with exactly its output's room (so the outputs lie back to back, most
    of them unaligned) -> ([status], [bytes])"""
    buf, offs = bytearray(), []
    for p in pieces:
        buf += bytes(1 if len(buf) % 2 == 0 else 2)
        offs.append(len(buf))
        buf += p
    n = len(pieces)
    items = (_lib.BatchItem * n)()
    for i in range(n):
        items[i].in_off, items[i].in_len, items[i].out_cap = offs[i], len(pieces[i]), sizes[i]
    assert all(o % 2 == 1 for o in offs)
    out, res = ctx.inflate_batch(bytes(buf), items, n, wbits)
    mv = memoryview(out)
    return [r.status for r in res[:n]], [bytes(mv[items[i].out_off:items[i].out_off + res[i].out_len]) for i in range(n)], \
        [items[i].out_off for i in range(n)]


@pytest.mark.parametrize("name", THREE)
def test_batch_verify(mods, ctx, name):
    """(d) za_wave_adler32 (zlib items) and za_wave_crc32_any (gzip items, one with a header CRC) of the batch decoder"""
    _lib, batch, devmem, gzip_index, zlib_ng = mods
    f = K.PATTERNS[name]
    datas = [f(n) for n in K.ADLER1K_LENS]
    n = len(datas)
    sizes = [len(x) for x in datas]
    zl = [zlib.compress(x, 1) for x in datas]
    gz = [_member(x, 1, name=b"n" * (i % 3), hcrc=(i == n // 2)) for i, x in enumerate(datas)]
    for wbits, pieces, check_at in ((15, zl, 4), (31, gz, 8)):
        st, outs, out_offs = _batch_call(_lib, ctx, pieces, wbits, sizes)
        assert st == [_lib.BATCH_OK] * n and outs == datas, (name, wbits, st)
        assert sum(1 for o in out_offs if o % 4) >= 3
        assert batch.decompress(pieces, wbits) == datas
        for j in _first_mid_last(n):
            bad = list(pieces)
            bad[j] = _flip(pieces[j], len(pieces[j]) - check_at, (3 + 11 * j) % 32)
            st, outs, _ = _batch_call(_lib, ctx, bad, wbits, sizes)
            assert st == [_lib.BATCH_CHECK if i == j else _lib.BATCH_OK for i in range(n)], (name, wbits, j, st)
            assert [o for i, o in enumerate(outs) if i != j] == [x for i, x in enumerate(datas) if i != j]
            got = batch.decompress(bad, wbits, errors="return")
            assert [isinstance(g, Exception) for g in got] == [i == j for i in range(n)]
            assert "incorrect data check" in str(got[j]) and got[j].index == j
    # the header CRC of the one gzip item that has one
    j = n // 2
    hdr_end = _walk(gz[j])[0][1]
    bad = list(gz)
    bad[j] = _flip(gz[j], hdr_end - 2, 9)
    st, outs, _ = _batch_call(_lib, ctx, bad, 31, sizes)
    assert st == [_lib.BATCH_HCRC if i == j else _lib.BATCH_OK for i in range(n)], (name, st)


# ---------------------------------------------------------------------------------------------------------------------------
# 7. gunzip's member loop: za_k_checksum at st_out + op and at st_in + pos
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", THREE)
def test_gunzip_member_loop_checksums(mods, ctx, name):
    """Three members of CPython's zlib with payloads of 1, 16 385 and 131 073 bytes: too few for the small-member hop, so the
    member loop decodes each of them and checks its CRC-32 where it lies in the output (offsets 1 and 16 386); the second
    member's header has a name and a header CRC and starts at an odd offset."""
    _lib = mods[0]
    f = K.PATTERNS[name]
    whole = f(1 + 16385 + 131073)
    parts = [whole[:1], whole[1:16386], whole[16386:]]
    first = _member(parts[0])
    if len(first) % 2 == 0:
        first = _member(parts[0], name=b"a")
    stream = first + _member(parts[1], name=b"member two", hcrc=True) + _member(parts[2])
    mem = _walk(stream)
    assert mem[1][0] % 2 == 1 and [m[3] for m in mem] == [1, 16385, 131073] and gzip.decompress(stream) == whole
    ctx.decode_paths(True)
    code, out, nm = ctx.gunzip(stream, len(whole))
    paths = ctx.decode_paths(True)
    assert (code, nm) == (0, 3) and out == whole, (name, code, nm)
    assert paths["indexed"] == 0 and paths["bgzf"] == 0 and paths["sequential"] + paths["chunked"] == 3, paths
    code, out, nm = ctx.gunzip(_flip(stream, mem[1][1] - 2, 6), len(whole))
    assert code == _lib.E_GZ_HCRC and nm == 1 and out == parts[0], (name, code, nm)
    for j in range(3):
        code, out, nm = ctx.gunzip(_flip(stream, mem[j][2], (13 * j + 2) % 32), len(whole))
        assert code == _lib.E_GZ_CRC and nm == j and out == b"".join(parts[:j]), (name, j, code, nm)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. zngamd_crc32_fold_dev
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_crc32_fold_dev(mods, ctx, name):
    """unit CRCs in device memory, folded on the host: 1, 2 and 9 units of 128 KiB with a last one of 128 KiB, 1 and 77 777 bytes"""
    devmem = mods[2]
    each = 131072
    d = K.PATTERNS[name](9 * each)
    out = C.c_uint32(0)
    for units in (1, 2, 9):
        for last in (each, 1, 77777):
            n = (units - 1) * each + last
            crcs = np.array([zlib.crc32(d[i * each:min((i + 1) * each, n)]) for i in range(units)], np.uint32)
            buf = devmem.from_host(ctx, crcs)
            assert ctx.L.zngamd_crc32_fold_dev(ctx.h, buf.vp(), units, each, last, C.byref(out)) == 0, ctx.err()
            assert out.value == zlib.crc32(d[:n]), (name, units, last)
            buf.free()

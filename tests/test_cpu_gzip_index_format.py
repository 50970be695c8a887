"""The seek-point index file format (zlib_ng_amd/gzip_index.py, INTEGRATION.md "Seek-point index"), without a GPU: index files
built here by hand from the documented layout (the windows section made by the stdlib zlib) load, and every corrupted or hostile
one is refused with ValueError before anything could reach a kernel."""
import io
import random
import struct
import zlib

import pytest

from zlib_ng_amd import gzip_index as gi

HDR = struct.Struct("<8sIIQIIQQQQQ")
REC = struct.Struct("<QQQQQQQIIII")

DATA = bytes(random.Random(5).getrandbits(8) for _ in range(300000))     # the "data file": its bytes only matter for the binding


def _bind(data):
    return zlib.crc32(data[:1 << 16]), zlib.crc32(data[-(1 << 16):])


def _points():
    # member point (kernel span from its deflate data), two block points of that member (the second ends the member), a member run
    K, B, F = gi.F_KERNEL, gi.F_BLOCK, gi.F_FINAL
    return [
        # in_bit data_bit end_bit out_off out_len win_off member_out win_len span_crc member_crc flags
        [0, 80, 8001, 0, 1000, 0, 0, 0, 11, 0, K],
        [8001, 8001, 400003, 1000, 40000, 0, 1000, 1000, 12, 77, B | K],
        [400003, 400003, 800000, 41000, 500, 1000, 41000, 32768, 13, 78, B | K | F],
        [800640, 800640, len(DATA) * 8, 41500, 100, 33768, 0, 0, 14, 0, 0],
    ]


WINDOWS = bytes(range(256)) * 132          # 33 792 bytes: 1 000 + 32 768 are used


def _blob(points=None, size=None, n=None, windows=WINDOWS, data=DATA, version=1, magic=b"ZNGAIDX\0", fix_crc=True):
    points = _points() if points is None else points
    size = sum(p[4] for p in points) if size is None else size
    wz = zlib.compress(windows, 6)
    ch, ct = _bind(data)
    hdr = HDR.pack(magic, version, REC.size, len(data), ch, ct, size, 1 << 20, len(points) if n is None else n, len(windows), len(wz))
    body = hdr + b"".join(REC.pack(*p) for p in points) + wz
    return body + struct.pack("<I", zlib.crc32(body) if fix_crc else 0)


def test_documented_layout_sizes():
    assert HDR.size == 72 and REC.size == 72
    assert gi._HDR.format == HDR.format and gi._REC.format == REC.format and gi.MAGIC == b"ZNGAIDX\0" and gi.VERSION == 1


def test_hand_built_index_loads():
    idx = gi.GzipIndex.from_bytes(_blob())
    assert idx.size == 41600 and idx.spacing == 1 << 20 and idx.file_size == len(DATA)
    assert [p.fields() for p in idx.points] == [tuple(p) for p in _points()]
    assert [p.is_block for p in idx.points] == [False, True, True, False]
    assert [p.kernel for p in idx.points] == [True, True, True, False]
    # spans: a read of 10 bytes across the first boundary needs the first two; one inside the member run only the last
    assert idx._spans_for(995, 10) == [0, 1]
    assert idx._spans_for(41550, 1000) == [3]
    assert idx._spans_for(41600, 5) == [] and idx._spans_for(0, 0) == []
    assert idx.point_for(0) == 0 and idx.point_for(41000) == 2 and idx.point_for(40999) == 1 and idx.point_for(10 ** 9) == 3
    # save / load round trip, through a path-like and a file object
    buf = io.BytesIO()
    idx.save(buf)
    back = gi.GzipIndex.load(io.BytesIO(buf.getvalue()))
    assert [p.fields() for p in back.points] == [p.fields() for p in idx.points] and back.size == idx.size
    assert buf.getvalue() == _blob()       # (the windows section is kept as it came: the same bytes go out again)


def test_every_single_byte_flip_is_rejected():
    blob = _blob()
    for i in range(len(blob)):
        bad = bytearray(blob)
        bad[i] ^= 0x5A
        with pytest.raises(ValueError):
            gi.GzipIndex.from_bytes(bytes(bad))
    for cut in (0, 1, len(blob) // 2, len(blob) - 1):
        with pytest.raises(ValueError):
            gi.GzipIndex.from_bytes(blob[:cut])


def _hostile(edit, **kw):
    pts = _points()
    edit(pts)
    with pytest.raises(ValueError):
        gi.GzipIndex.from_bytes(_blob(pts, **kw))


def test_crc_correct_hostile_indexes_are_rejected():
    def swap(p):
        p[1][0], p[2][0] = p[2][0], p[1][0]
    _hostile(swap)                                                      # offsets not monotonic
    _hostile(lambda p: p[3].__setitem__(0, 7000))                      # a member run that starts inside another span
    _hostile(lambda p: p[2].__setitem__(7, 40000))                     # win_len 40 000
    _hostile(lambda p: p[2].__setitem__(5, len(WINDOWS) - 100))        # a window past the windows section
    _hostile(lambda p: p[3].__setitem__(2, len(DATA) * 8 + 8))         # an end bit past the file
    _hostile(lambda p: p[1].__setitem__(2, 400011))                    # a span that does not end at the next point
    _hostile(lambda p: p[1].__setitem__(4, 40001))                     # spans that do not tile the output
    _hostile(lambda p: None, size=41601)                                # spans that do not sum to size
    _hostile(lambda p: None, n=5)                                       # record count off by one
    _hostile(lambda p: None, n=3)
    _hostile(lambda p: p[0].__setitem__(10, 8))                         # unknown flags
    _hostile(lambda p: p[3].__setitem__(7, 10))                         # a member point with a window
    _hostile(lambda p: p[0].__setitem__(1, 40))                         # deflate data inside the member header
    _hostile(lambda p: p[1].__setitem__(7, 999))                        # a window shorter than the member's output before the point
    _hostile(lambda p: p.__setitem__(0, [0, 0, 8001, 0, 1000, 0, 0, 0, 11, 0, gi.F_BLOCK | gi.F_KERNEL]))    # block point first
    with pytest.raises(ValueError):
        gi.GzipIndex.from_bytes(_blob(version=2))
    with pytest.raises(ValueError):
        gi.GzipIndex.from_bytes(_blob(magic=b"ZNGAIDX\1"))
    with pytest.raises(ValueError):
        gi.GzipIndex.from_bytes(_blob(fix_crc=False))


def test_binding_to_the_data_file():
    idx = gi.GzipIndex.from_bytes(_blob())
    idx.check_file(io.BytesIO(DATA))
    with pytest.raises(ValueError):
        idx.check_file(io.BytesIO(DATA + b"\0"))                        # another size
    other = bytearray(DATA)
    other[-5] ^= 1                                                      # same size, other content in the last 64 KiB
    with pytest.raises(ValueError):
        idx.check_file(io.BytesIO(bytes(other)))
    other = bytearray(DATA)
    other[3] ^= 1                                                       # ... in the first 64 KiB
    with pytest.raises(ValueError):
        idx.check_file(io.BytesIO(bytes(other)))
    with pytest.raises(ValueError):
        idx.read_at(io.BytesIO(bytes(other)), 0, 10)                    # refused before anything is read or decoded

"""CPU: the batch API's C ABI and its Python face without a GPU -- the ctypes structures match include/zng_amd.h, the status codes
match the binding, every status maps to the text zlib_ng.decompress gives for that case, and argument errors are raised before any
device call."""
import ctypes as C
import os
import re
import struct

import pytest

from conftest import ROOT

_SIZES = {"uint64_t": 8, "uint32_t": 4, "int32_t": 4}


def _c_layout(header, name):
    """(size, {field: offset}) of `typedef struct { ... } name;` with natural alignment"""
    m = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", header)
    assert m, name
    off, fields, align = 0, {}, 1
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, rest = decl.split(None, 1)
        sz = _SIZES[typ]
        align = max(align, sz)
        for f in rest.split(","):
            f = f.strip()
            count = 1
            am = re.match(r"(\w+)\[(\d+)\]", f)
            if am:
                f, count = am.group(1), int(am.group(2))
            off = (off + sz - 1) // sz * sz
            fields[f] = off
            off += sz * count
    return (off + align - 1) // align * align, fields


@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "zng_amd.h")).read()


@pytest.mark.parametrize("cname,pyname", [("zngamd_batch_item", "BatchItem"), ("zngamd_batch_result", "BatchResult")])
def test_struct_layout_matches_header(header, cname, pyname):
    from zlib_ng_amd import _lib
    size, fields = _c_layout(header, cname)
    cls = getattr(_lib, pyname)
    assert C.sizeof(cls) == size
    assert [f[0] for f in cls._fields_] == list(fields)
    for f, off in fields.items():
        assert getattr(cls, f).offset == off, f
    assert size == {"BatchItem": 32, "BatchResult": 16}[pyname]


def test_status_constants_match_binding(header):
    from zlib_ng_amd import _lib
    consts = dict(re.findall(r"#define\s+(ZNGAMD_BATCH_[A-Z_]+)\s+(\d+)", header))
    assert len(consts) == 14
    for k, v in consts.items():
        assert getattr(_lib, k[len("ZNGAMD_"):]) == int(v), k


def _oneshot_error(data, wbits):
    from zlib_ng_amd import zlib_ng
    with pytest.raises(zlib_ng.error) as ei:
        zlib_ng.decompress(data, wbits)
    return str(ei.value)


def test_every_status_has_the_oneshot_message():
    from zlib_ng_amd import _lib, batch, zlib_ng
    W = "while decompressing data"
    expected = {
        _lib.BATCH_TRUNCATED: f"Error -5 {W}: incomplete or truncated stream",
        _lib.BATCH_NEED_DICT: f"Error 2 {W}",
        _lib.BATCH_HEADER: f"Error -3 {W}: incorrect header check",
        _lib.BATCH_WINDOW: f"Error -3 {W}: invalid window size",
        _lib.BATCH_METHOD: f"Error -3 {W}: unknown compression method",
        _lib.BATCH_FLAGS: f"Error -3 {W}: unknown header flags set",
        _lib.BATCH_HCRC: f"Error -3 {W}: header crc mismatch",
        _lib.BATCH_DATA: f"Error -3 {W}: invalid input data",
        _lib.BATCH_CHECK: f"Error -3 {W}: incorrect data check",
        _lib.BATCH_LENGTH: f"Error -3 {W}: incorrect length check",
    }
    for st, msg in expected.items():
        e = batch.status_error(st)
        assert type(e) is zlib_ng.error and str(e) == msg, st
    assert batch.status_error(_lib.BATCH_OK) is None
    assert isinstance(batch.status_error(_lib.BATCH_TABLE), ValueError)
    # the statuses the one-shot reaches without a device, checked against it
    good = bytes([0x78, 0x9c])
    assert _oneshot_error(b"\x78", 15) == expected[_lib.BATCH_TRUNCATED]
    assert _oneshot_error(b"\x78\x9d\x00\x00", 15) == expected[_lib.BATCH_HEADER]
    bad_method = 0x79 << 8                           # CM = 9 with a valid FCHECK
    bad_method += 31 - bad_method % 31
    assert _oneshot_error(struct.pack(">H", bad_method) + b"\0\0", 15) == expected[_lib.BATCH_HEADER]
    assert _oneshot_error(good, 9) == expected[_lib.BATCH_WINDOW]
    h = (0x78 << 8) | 0x20
    h += 31 - h % 31
    assert _oneshot_error(struct.pack(">H", h) + b"\0\0\0\1", 15) == expected[_lib.BATCH_NEED_DICT]
    gz = bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3])
    assert _oneshot_error(gz[:1] + b"\x8c" + gz[2:] + b"\0" * 8, 31) == expected[_lib.BATCH_HEADER]
    assert _oneshot_error(gz[:2] + b"\x07" + gz[3:] + b"\0" * 8, 31) == expected[_lib.BATCH_METHOD]
    assert _oneshot_error(gz[:3] + b"\x20" + gz[4:] + b"\0" * 8, 31) == expected[_lib.BATCH_FLAGS]
    assert _oneshot_error(gz[:5], 31) == expected[_lib.BATCH_TRUNCATED]
    assert _oneshot_error(gz[:3] + b"\x08" + gz[4:] + b"name", 31) == expected[_lib.BATCH_TRUNCATED]


def test_argument_errors_before_any_device_call(monkeypatch):
    from zlib_ng_amd import batch, zlib_ng

    def no_device():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(zlib_ng, "_ctx", no_device)
    with pytest.raises(zlib_ng.error, match="Bad compression level"):
        batch.compress([b"x"], 10)
    with pytest.raises(zlib_ng.error, match="Bad compression level"):
        batch.compress([b"x"], -2)
    with pytest.raises(TypeError):
        batch.compress([b"x"], "6")
    with pytest.raises(zlib_ng.error, match="Bad compression level"):
        batch.compress([b"x"], 6, 16)               # wbits outside the compress classes
    with pytest.raises(zlib_ng.error, match="Bad compression level"):
        batch.compress([b"x"], 6, -8)
    with pytest.raises(ValueError, match="Invalid initialization option"):
        batch.compress([b"x"], 6, 15, strategy=5)
    with pytest.raises(TypeError):
        batch.compress([b"x", 3])
    with pytest.raises(TypeError):
        batch.decompress([b"x", "text"])
    with pytest.raises(zlib_ng.error, match="Error -2 while preparing to decompress data"):
        batch.decompress([b"x"], 17)
    with pytest.raises(zlib_ng.error, match="Error -2 while preparing to decompress data"):
        batch.decompress([b"x"], -7)
    with pytest.raises(ValueError, match="errors"):
        batch.decompress([b"x"], errors="ignore")
    assert batch.compress([]) == [] and batch.decompress([]) == [] and batch.decompress((), 31, errors="return") == []


def test_sub_batches_cover_every_item_once():
    from zlib_ng_amd import batch
    sizes = [5, 1, 7, 0, 12, 3, 3]
    for budget in (1, 6, 10, 100):
        parts = batch._sub_batches(sizes, budget)
        assert [i for a, b in parts for i in range(a, b)] == list(range(len(sizes)))
        for a, b in parts:
            assert b - a == 1 or sum(sizes[a:b]) <= budget

"""CPU: BGZF by content without a GPU -- the C entry points are declared, exported and bound; the window planner of bgzf.grep on
synthetic block tables; GrepResult; argument checks that need no context; and, under the host AddressSanitizer build (as
tests/test_cpu_sanitizers_bgzf.py runs the scan), zngamd_bgzf_grep with hostile pattern tables: ZNGAMD_E_ARG before the context is
touched or anything is launched."""
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_cpu_sanitizers import _run


def test_symbols_declared_exported_and_bound():
    import ctypes as C
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    for name in ("zngamd_bgzf_grep_dev", "zngamd_bgzf_grep"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        nargs = len(re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(","))
        assert len(getattr(L, name).argtypes) == nargs, name
    for macro, value in (("INVERT", _lib.BGZF_GREP_INVERT), ("LINE_START", _lib.BGZF_GREP_LINE_START), ("FINAL", _lib.BGZF_GREP_FINAL),
                         ("COUNT_ONLY", _lib.BGZF_GREP_COUNT_ONLY), ("MAX_PATTERNS", _lib.BGZF_GREP_MAX_PATTERNS),
                         ("MAX_PATTERN", _lib.BGZF_GREP_MAX_PATTERN)):
        assert int(re.search(r"#define ZNGAMD_BGZF_GREP_%s\s+(\d+)u" % macro, header).group(1)) == value, macro
    assert C.sizeof(_lib.BgzfGrepTotals) == 40 and _lib.BgzfGrepTotals.covered.offset == 32
    assert _lib.GREP_ROW_DTYPE.itemsize == 24 and _lib.GREP_ROW_DTYPE.fields["len"][1] == 16
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_grep.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_grep.hip"))
    blob, tab = _lib.grep_pattern_table([b"ab", b"c", b"defg"])
    assert blob == b"abcdefg" and tab.tolist() == [[0, 2], [2, 1], [3, 4]] and tab.dtype == np.uint32


def test_window_planner():
    from zlib_ng_amd import bgzf
    coffs, isizes = np.array([1000, 1100, 1250, 1300, 1420], np.int64), np.array([50, 60, 0, 70, 80], np.int64)
    CAP = 1 << 30
    # the whole window; the file goes on / ends behind it
    assert bgzf._grep_window(coffs, isizes, 7, None, False, CAP) == (5, 260, False)
    assert bgzf._grep_window(coffs, isizes, 7, None, True, CAP) == (5, 260, True)
    # stop at a block start, inside a block, at a block's end (not normalised), behind the window
    assert bgzf._grep_window(coffs, isizes, 0, (1300, 0), False, CAP) == (3, 110, True)
    assert bgzf._grep_window(coffs, isizes, 0, (1300, 25), False, CAP) == (4, 135, True)
    assert bgzf._grep_window(coffs, isizes, 0, (1100, 60), True, CAP) == (2, 110, True)
    assert bgzf._grep_window(coffs, isizes, 0, (9999, 0), False, CAP) == (5, 260, False)
    assert bgzf._grep_window(coffs, isizes, 0, (9999, 0), True, CAP) == (5, 260, True)
    for stop in ((1300, 71), (1150, 0)):                     # beyond the block's ISIZE; not a block start
        with pytest.raises(ValueError):
            bgzf._grep_window(coffs, isizes, 0, stop, False, CAP)
    with pytest.raises(ValueError):
        bgzf._grep_window(coffs, isizes, 30, (1000, 20), False, CAP)      # stop in front of start
    # the cap on the decoded bytes of one engine call: whole blocks, at least one, and the window is not the file's last any more
    assert bgzf._grep_window(coffs, isizes, 0, None, True, 120) == (3, 110, False)
    assert bgzf._grep_window(coffs, isizes, 0, None, True, 10) == (1, 50, False)
    assert bgzf._grep_window(coffs, isizes, 0, (1420, 5), True, 120) == (3, 110, False)      # (stop lies behind the cut)
    assert bgzf._grep_window(coffs[:0], isizes[:0], 0, None, True, CAP) == (0, 0, True)

    W = 32 << 20
    # no open line: the next window starts behind this one
    assert bgzf._grep_advance(isizes, 5, 7, 260, 260, False, W, 1000) == (5, 0, W)
    assert bgzf._grep_advance(isizes, 3, 7, 110, 110, False, W, 1000) == (3, 0, W)
    # an open line is carried: the window restarts at the block in which it begins, text_off at its first byte
    assert bgzf._grep_advance(isizes, 5, 7, 260, 200, False, W, 1000) == (4, 20, W)
    assert bgzf._grep_advance(isizes, 5, 7, 260, 110, False, W, 1000) == (3, 0, W)      # at a block start: not the empty block in front of it
    assert bgzf._grep_advance(isizes, 5, 7, 260, 49, False, W, 1000) == (0, 49, W)      # progress inside the first block: the same window size
    # no line ended in the window: it grows
    assert bgzf._grep_advance(isizes, 5, 7, 260, 7, False, W, 1000) == (0, 7, 2 * W)
    # ... up to max_line
    with pytest.raises(ValueError) as e:
        bgzf._grep_advance(isizes, 5, 7, 260, 60, False, W, 199)
    assert (e.value.block, e.value.offset) == (1, 10)
    assert bgzf._grep_advance(isizes, 5, 7, 260, 60, False, W, 200) == (1, 10, W)
    # the last window (the file ended, or stop was reached): over
    assert bgzf._grep_advance(isizes, 5, 7, 260, 260, True, W, 1000) is None


class _FakeTotals:
    def __init__(self, seen, matched, tail_off):
        self.seen, self.matched, self.tail_off, self.covered, self.bytes = seen, matched, tail_off, 1, 0


class _FakeCtx:
    """the engine call of bgzf.grep replaced by Python on the decoded blocks: what the driver asks for, window by window"""

    def __init__(self, blocks):
        self.blocks, self.calls = blocks, []               # coffset -> decoded bytes

    def bgzf_grep(self, data, members, text_off, text_end, blob, table, delim, flags, line_base=0, caps=None):
        from zlib_ng_amd import _lib
        self.calls.append((len(members), text_off, text_end, flags, line_base))
        text = b"".join(self.window)[text_off:text_end]
        pats = [blob[o:o + n] for o, n in table.tolist()]
        parts = text.split(bytes([delim]))
        lines = [p + bytes([delim]) for p in parts[:-1]]
        tail = text_end
        if parts[-1]:
            if flags & _lib.BGZF_GREP_FINAL:
                lines.append(parts[-1])
            else:
                tail = text_end - len(parts[-1])
        rows, at, packed = [], text_off, []
        for i, ln in enumerate(lines):
            if any(p in ln for p in pats):
                rows.append((at, line_base + i, len(ln), 0))
                packed.append(ln)
            at += len(ln)
        if flags & _lib.BGZF_GREP_COUNT_ONLY:
            return 0, np.zeros(len(members), np.int32), _FakeTotals(len(lines), len(rows), tail), np.empty(0, _lib.GREP_ROW_DTYPE), b""
        return 0, np.zeros(len(members), np.int32), _FakeTotals(len(lines), len(rows), tail), np.array(rows, _lib.GREP_ROW_DTYPE), b"".join(packed)


def _stored_bgzf(data, block_size):
    """BGZF of stored deflate blocks, written here: no engine needed"""
    import struct
    import zlib
    out, blocks = [], {}
    for o in range(0, len(data), block_size):
        piece = data[o:o + block_size]
        payload = b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece
        size = 18 + len(payload) + 8
        blocks[sum(len(x) for x in out)] = piece
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + payload + struct.pack("<II", zlib.crc32(piece), len(piece)))
    eof = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    blocks[sum(len(x) for x in out)] = b""
    return b"".join(out) + eof, blocks


def test_driver_on_a_fake_engine(monkeypatch):
    """the host driver end to end with the engine call replaced: windows, the carried open line, growth, stop, max_count, virtual
    offsets -- the file is real BGZF (stored blocks), the scan and the member table are the product's"""
    import io
    from zlib_ng_amd import _lib, bgzf
    lines = [b"line %05d %s\n" % (i, b"needle" if i % 7 == 3 else b"hay" * (i % 5)) for i in range(3000)] + [b"x" * 30000 + b" needle\n", b"open needle"]
    data = b"".join(lines)
    blob, blocks = _stored_bgzf(data, 997)
    fake = _FakeCtx(blocks)
    coffs = sorted(blocks)

    orig = bgzf._member_table

    def member_table(buf, starts, csizes, isizes):
        members, bad = orig(buf, starts, csizes, isizes)
        # the bytes the fake engine "decodes": found by the blocks' ISIZE and CRC in the table the driver made
        fake.window = [fake_blocks_by_crc[(int(m["crc"]), int(m["out_len"]))] for m in members]
        return members, bad

    import zlib
    fake_blocks_by_crc = {(zlib.crc32(b), len(b)): b for b in blocks.values()}
    monkeypatch.setattr(bgzf, "_member_table", member_table)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)                                        # (what is read beyond a window: a block of this file)
    want = [i for i, ln in enumerate(lines) if b"needle" in ln]
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])])
    for window in (32 << 20, 5000, 1500):
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        fake.calls.clear()
        res = bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, False, None, None, None, 0, 64 << 20)
        assert res.numbers.tolist() == want and list(res) == [lines[i] for i in want] and res.searched == len(lines)
        for k, v in enumerate(res.voffsets.tolist()):
            c, u = bgzf.split_virtual_offset(v)
            assert coffs.index(c) * 997 + u == starts[want[k]] and u < 997
        assert all(f & _lib.BGZF_GREP_FINAL for *_, f, _ in fake.calls[-1:]) and not any(f & _lib.BGZF_GREP_FINAL for *_, f, _ in fake.calls[:-1])
        if window == 32 << 20:
            assert len(fake.calls) == 1
        else:
            assert len(fake.calls) > 10
            assert any(off > 0 for _, off, _, _, _ in fake.calls[1:])         # an open line was carried: the window began inside a block
            assert [lb for *_, lb in fake.calls] == sorted(lb for *_, lb in fake.calls)
        # max_count: the windows behind the one that reaches N are not read
        n_all = len(fake.calls)
        fake.calls.clear()
        part = bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, False, 5, None, None, 0, 64 << 20)
        assert part.numbers.tolist() == want[:5] and list(part) == [lines[i] for i in want[:5]]
        assert len(fake.calls) == 1 if window == 32 << 20 else len(fake.calls) < n_all // 4
        assert bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, True, None, None, None, 0, 64 << 20) == len(want)
        # start / stop at line starts, stop inside a block
        a, b = 700, 2100
        va = bgzf.make_virtual_offset(coffs[starts[a] // 997], starts[a] % 997)
        vb = bgzf.make_virtual_offset(coffs[starts[b] // 997], starts[b] % 997)
        assert starts[b] % 997
        mid = bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, False, None, va, vb, a, 64 << 20)
        assert mid.numbers.tolist() == [i for i in want if a <= i < b] and mid.searched == b - a
        assert len(bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, False, None, vb, va, 0, 64 << 20)) == 0
    # the window grows for the line of 30 000 bytes, and max_line bounds it
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1500)
    with pytest.raises(ValueError, match="has not ended after 20000 bytes"):
        bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, False, None, None, None, 0, 20000)


def test_grep_result():
    from zlib_ng_amd import bgzf
    data = b"alpha\nbeta\n\ngamma"
    r = bgzf.GrepResult([2, 5, 6, 9], [0, 1 << 16, 2 << 16 | 5, 7], [0, 6, 11, 12, 17], data, 10)
    assert len(r) == 4 and r.searched == 10
    assert r[0] == b"alpha\n" and r[3] == r[-1] == b"gamma" and r[-4] == b"alpha\n" and r[2] == b"\n"
    assert r[1:3] == [b"beta\n", b"\n"] and r[::-1][0] == b"gamma" and r[:0] == [] and r[10:] == []
    assert list(r) == [b"alpha\n", b"beta\n", b"\n", b"gamma"] and all(isinstance(x, bytes) for x in r)
    for bad in (4, -5):
        with pytest.raises(IndexError):
            r[bad]
    assert r.numbers.dtype == np.int64 and r.voffsets.dtype == np.uint64 and r.offsets.dtype == np.int64
    r = bgzf.GrepResult([], [], [0], memoryview(b""), 0)
    assert len(r) == 0 and list(r) == [] and r[:] == []
    with pytest.raises(ValueError):
        bgzf.GrepResult([1], [0], [0], b"", 1)
    assert "GrepResult" in bgzf.__all__ and "grep" in bgzf.__all__


def test_argument_checks_need_no_context(tmp_path):
    from zlib_ng_amd import bgzf
    path = tmp_path / "f.bgzf"
    path.write_bytes(bgzf.EOF_BLOCK)
    for bad in (b"", [], [b"ok", b""], [b"x"] * 65, b"y" * 256, b"two\nlines", [b"fine", b"a\n"]):
        with pytest.raises(ValueError):
            bgzf.grep(str(path), bad)
    for kw in (dict(delimiter=b""), dict(delimiter=b"ab"), dict(max_line=0), dict(max_line=(1 << 31) + 1), dict(max_count=-1)):
        with pytest.raises(ValueError):
            bgzf.grep(str(path), b"x", **kw)
    with pytest.raises(ValueError):
        bgzf.grep(str(path), b"a;b", delimiter=b";")
    assert bgzf._grep_patterns(bytearray(b"one"), b"\n") == ([b"one"], b"\n")
    assert bgzf._grep_patterns([b"a" * 255] * 64, b"\x00")[0] == [b"a" * 255] * 64


GREP_SCRIPT = textwrap.dedent("""
    import ctypes as C, os, sys
    sys.path.insert(0, %r)
    from zlib_ng_amd import _lib
    assert _lib.LIB_PATH == os.environ["ZNGAMD_LIB"]
    L = _lib.load()
    E_ARG = -202
    ctx = (C.c_uint8 * 1)()            # one byte where a context would be: a call that touched it before judging the patterns is a report
    tot = _lib.BgzfGrepTotals()

    def exact(b):
        return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\\0")

    def call(blob, rows, delim=10, ctx=ctx, totals=tot, dev=False, patterns_len=None):
        mem = exact(blob) if blob is not None else None
        n = len(rows) if rows is not None else 3
        tab = (C.c_uint32 * max(2 * n, 1))(*[x for row in (rows or []) for x in row]) if rows is not None else None
        plen = len(blob or b"") if patterns_len is None else patterns_len
        t = C.byref(totals) if totals is not None else None
        if dev:
            return L.zngamd_bgzf_grep_dev(ctx, None, 0, None, 0, 0, 0, mem, plen, tab, n, delim, 0, 0, None, 0, None, None, 0, None, 0, t)
        return L.zngamd_bgzf_grep(ctx, None, 0, None, 0, 0, 0, mem, plen, tab, n, delim, 0, 0, None, None, 0, None, 0, _lib.ALLOC_FN(), None, t)

    blob = b"needle" + b"x" * 300
    for dev in (False, True):
        hostile = [
            (blob, [(len(blob), 1)]), (blob, [(len(blob) - 2, 3)]), (blob, [(0xFFFFFFFF, 2)]), (blob, [(0xFFFFFFF0, 0x20)]), (blob, [(1 << 31, 1 << 31)]),
            (blob, [(0, 0)]), (blob, [(0, 6), (3, 0)]), (blob, [(6, 256)]), (blob, [(6, 300)]), (blob, [(0, 0xFFFFFFFF)]),
            (blob, [(0, 1)] * 65), (blob, [(0, 1)] * 1000), (blob, []),
            (b"nee\\ndle", [(0, 7)]), (b"nee\\ndle", [(0, 3), (3, 1)]), (b"", [(0, 1)]),
        ]
        for b, rows in hostile:
            assert call(b, rows, dev=dev) == E_ARG, (b[:8], rows[:2], dev)
        assert call(b"a;b", [(0, 3)], delim=ord(";"), dev=dev) == E_ARG
        for delim in (-1, 256, 1 << 20):
            assert call(blob, [(0, 6)], delim=delim, dev=dev) == E_ARG
        assert call(None, [(0, 6)], dev=dev, patterns_len=6) == E_ARG             # NULL pointers
        assert call(blob, None, dev=dev) == E_ARG
        assert call(blob, [(0, 6)], totals=None, dev=dev) == E_ARG
        assert call(blob, [(0, 6)], ctx=None, dev=dev) == E_ARG
        assert call(None, None, ctx=None, totals=None, dev=dev) == E_ARG
    print("bgzf grep arguments clean")
""")


def test_hostile_pattern_tables_under_asan_ubsan(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("zng_amd_build_asan", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = str(tmp_path / "libzng_amd_host_asan.so")
    mod.build_host_asan(so)
    clang = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "lib", "llvm", "bin", "clang")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang"
    runtime = subprocess.run([clang, "--print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip("no shared AddressSanitizer runtime for hipcc's clang on this host")
    r = _run(runtime, {"ZNGAMD_LIB": so, "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""}, [sys.executable, "-c", GREP_SCRIPT % (PKG_DIR,)])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf grep arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

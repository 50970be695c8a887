"""CPU: BGZF by content with mismatches, without a GPU -- the argument checks of bgzf.grep / grep_records that need no context; the
four _approx entry points refuse hostile arguments with no context at all; the window loop of bgzf.grep on a stand-in engine whose
match rule is the numpy referee; and tests/grep_approx_args.cpp, a stand-alone program, against the library's host side under
AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process, nothing preloaded)."""
import ctypes as C
import io
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_grep import _FakeTotals, _stored_bgzf


class _Unreadable:
    """a file object that must not be touched: the arguments are judged first"""

    def __getattr__(self, name):
        raise AssertionError(f"the file was touched ({name}) before the arguments were judged")


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    assert _lib.BGZF_GREP_MAX_MISMATCH == 16
    for pats, bad in ((b"ACGTACGT", -1), (b"A" * 40, 17), (b"ACGT", 4), ([b"ACGTACGT", b"AC"], 2), (b"ACGTACGT", 1.0), (b"ACGTACGT", "1"),
                      (b"ACGTACGT", None), (b"ACGTACGT", True), (b"A", 1), (b"A" * 255, 1 << 32)):
        with pytest.raises(ValueError, match="mismatches"):
            bgzf.grep(_Unreadable(), pats, mismatches=bad)
        with pytest.raises(ValueError, match="mismatches"):
            bgzf.grep_records(_Unreadable(), pats, 4, match_line=1, first_byte=b"@", mismatches=bad)
    with pytest.raises(ValueError):                            # the patterns are judged as they always were
        bgzf.grep(_Unreadable(), b"two\nlines", mismatches=1)
    assert bgzf._grep_mismatches(0, [b"A"]) == 0 and bgzf._grep_mismatches(np.int64(16), [b"A" * 17, b"C" * 255]) == 16


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    for name in ("zngamd_bgzf_grep", "zngamd_bgzf_grep_dev", "zngamd_bgzf_grep_records", "zngamd_bgzf_grep_records_dev"):
        approx = name.replace("_dev", "") + "_approx" + ("_dev" if name.endswith("_dev") else "")
        assert approx in _lib.SYMBOLS and hasattr(L, approx), approx
        params = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(",")]
        aparams = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % approx, header).group(1).split(",")]
        at = params.index("uint32_t flags") + 1
        assert aparams == params[:at] + ["uint32_t max_mismatch"] + params[at:], approx      # the exact call's parameters, max_mismatch behind flags
        exact = getattr(L, name).argtypes
        assert getattr(L, approx).argtypes == exact[:at] + [C.c_uint32] + exact[at:], approx
    assert int(re.search(r"#define ZNGAMD_BGZF_GREP_MAX_MISMATCH\s+(\d+)u", header).group(1)) == _lib.BGZF_GREP_MAX_MISMATCH == 16
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                          # no kernel class was added


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for everything the exact calls refuse and for max_mismatch out of range"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    blob = b"needle" + b"x" * 300

    def call(form, b, rows, k, delim=10, totals=True, n=None):
        mem = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0") if b is not None else None
        tab = (C.c_uint32 * max(2 * len(rows), 1))(*[x for row in rows for x in row]) if rows is not None else None
        n = (len(rows) if rows is not None else 3) if n is None else n
        lt, rt = _lib.BgzfGrepTotals(), _lib.BgzfGrepRecordsTotals()
        head = (None, None, 0, None, 0, 0, 0, mem, len(b or b""), tab, n, delim, 0, k)
        if form == 0:
            return L.zngamd_bgzf_grep_approx(*head, 0, None, None, 0, None, 0, _lib.ALLOC_FN(), None, C.byref(lt) if totals else None)
        if form == 1:
            return L.zngamd_bgzf_grep_approx_dev(*head, 0, None, 0, None, None, 0, None, 0, C.byref(lt) if totals else None)
        if form == 2:
            return L.zngamd_bgzf_grep_records_approx(*head, 4, 1, 64, 0, None, None, 0, None, 0, _lib.ALLOC_FN(), None, C.byref(rt) if totals else None)
        return L.zngamd_bgzf_grep_records_approx_dev(*head, 4, 1, 64, 0, None, 0, None, None, 0, None, 0, C.byref(rt) if totals else None)

    for form in range(4):
        for k in (17, 18, 255, 0xFFFFFFFF):
            assert call(form, blob, [(6, 255)], k) == E_ARG, (form, k)
        for rows, k in (([(0, 6)], 6), ([(0, 6)], 7), ([(0, 6), (6, 2)], 2), ([(0, 6), (6, 1)], 1), ([(0, 1)], 1)):
            assert call(form, blob, rows, k) == E_ARG, (form, rows, k)
        for rows in ([], [(0, 2)] * 65, [(0, 0)], [(0, 6), (3, 0)], [(6, 256)], [(len(blob), 1)], [(len(blob) - 2, 3)], [(0xFFFFFFFF, 2)],
                     [(1 << 31, 1 << 31)]):
            assert call(form, blob, rows, 1 if rows and rows[0][1] > 1 else 0) == E_ARG, (form, rows[:2])
        assert call(form, b"nee\ndle", [(0, 7)], 1) == E_ARG and call(form, b"a;b", [(0, 3)], 1, delim=ord(";")) == E_ARG
        assert call(form, blob, [(0, 6)], 1, delim=256) == E_ARG and call(form, blob, [(0, 6)], 1, delim=-1) == E_ARG
        assert call(form, blob, [(0, 6)], 1, totals=False) == E_ARG
        assert call(form, None, [(0, 6)], 1) == E_ARG and call(form, blob, None, 1) == E_ARG
        assert call(form, blob, [(0, 6)], 1) == E_ARG and call(form, blob, [(0, 6)], 0) == E_ARG      # (in order but for the context)


def _hit(text, delim, pats, k):
    """the numpy referee: the lines of text in which a window of a pattern's length differs from it in at most k bytes and holds no
    delimiter"""
    arr = np.frombuffer(text, np.uint8)
    n = len(arr)
    before = np.concatenate([[0], np.cumsum(arr == delim)])
    hit = set()
    for p in pats:
        L = len(p)
        if L > n:
            continue
        cnt = np.zeros(n - L + 1, np.int32)
        for j in range(L):
            cnt += arr[j:n - L + 1 + j] != p[j]
        pos = np.nonzero((cnt <= k) & (before[L:] == before[:n - L + 1]))[0]
        hit.update(before[pos].tolist())
    return hit


class _FakeApproxCtx:
    """the engine calls of bgzf.grep replaced by the referee on the decoded blocks; what the driver asked for is kept"""

    def __init__(self):
        self.calls, self.exact_calls, self.window = [], 0, []

    def _answer(self, text_off, text_end, blob, table, delim, flags, line_base, k):
        from zlib_ng_amd import _lib
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
        hit = _hit(text, delim, pats, k)
        rows, at, packed = [], text_off, []
        for i, ln in enumerate(lines):
            if i in hit:
                rows.append((at, line_base + i, len(ln), 0))
                packed.append(ln)
            at += len(ln)
        tot = _FakeTotals(len(lines), len(rows), tail)
        if flags & _lib.BGZF_GREP_COUNT_ONLY:
            return 0, np.zeros(len(self.window), np.int32), tot, np.empty(0, _lib.GREP_ROW_DTYPE), b""
        return 0, np.zeros(len(self.window), np.int32), tot, np.array(rows, _lib.GREP_ROW_DTYPE), b"".join(packed)

    def bgzf_grep(self, data, members, text_off, text_end, blob, table, delim, flags, line_base=0, caps=None, **kw):
        if not kw:
            self.exact_calls += 1
        assert set(kw) <= {"mismatches"} and kw.get("mismatches", 1) > 0      # (0 is not passed on: the call of before)
        self.calls.append((len(members), text_off, text_end, flags, line_base, kw.get("mismatches", 0)))
        return self._answer(text_off, text_end, blob, table, delim, flags, line_base, kw.get("mismatches", 0))


def test_driver_on_a_fake_engine(monkeypatch):
    from zlib_ng_amd import _lib, bgzf
    lines = [b"line %05d %s\n" % (i, b"needle" if i % 7 == 3 else b"noodle" if i % 7 == 5 else b"hay" * (i % 5)) for i in range(3000)]
    lines += [b"x" * 30000 + b" nexdle\n", b"open neeble"]
    data = b"".join(lines)
    blob, blocks = _stored_bgzf(data, 997)
    fake = _FakeApproxCtx()
    coffs = sorted(blocks)
    by_crc = {(zlib.crc32(b), len(b)): b for b in blocks.values()}
    orig = bgzf._member_table

    def member_table(buf, starts, csizes, isizes):
        members, bad = orig(buf, starts, csizes, isizes)
        fake.window = [by_crc[(int(m["crc"]), int(m["out_len"]))] for m in members]
        return members, bad

    monkeypatch.setattr(bgzf, "_member_table", member_table)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)
    want = {k: sorted(_hit(data, 10, [b"needle"], k)) for k in (0, 1, 2)}
    assert want[0] == [i for i, ln in enumerate(lines) if b"needle" in ln] and len(want[0]) < len(want[1]) < len(want[2])
    assert 3000 in want[1] and 3001 in want[1] and 5 not in want[1] and 5 in want[2]
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])])

    def grep(k, *, count=False, max_count=None, start=None, stop=None, first=0):
        return bgzf._grep_file(io.BytesIO(blob), fake, b"needle", b"\n", False, False, count, max_count, start, stop, first, 64 << 20, None, k)

    for window in (32 << 20, 5000, 1500):
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        for k in (1, 2):
            fake.calls.clear()
            res = grep(k)
            assert res.numbers.tolist() == want[k] and list(res) == [lines[i] for i in want[k]] and res.searched == len(lines)
            assert [c[5] for c in fake.calls] == [k] * len(fake.calls) and fake.exact_calls == 0      # every window's call was told k
            for j, v in enumerate(res.voffsets.tolist()):
                c, u = bgzf.split_virtual_offset(v)
                assert coffs.index(c) * 997 + u == starts[want[k][j]] and u < 997
            assert fake.calls[-1][3] & _lib.BGZF_GREP_FINAL and not any(c[3] & _lib.BGZF_GREP_FINAL for c in fake.calls[:-1])
            if window == 32 << 20:
                assert len(fake.calls) == 1
            else:
                assert len(fake.calls) > 10 and any(c[1] > 0 for c in fake.calls[1:])      # an open line was carried into the next window
                assert [c[4] for c in fake.calls] == sorted(c[4] for c in fake.calls)
            n_all = len(fake.calls)
            fake.calls.clear()
            part = grep(k, max_count=5)                                 # max_count: the windows behind the one that reaches N are not read
            assert part.numbers.tolist() == want[k][:5] and [c[5] for c in fake.calls] == [k] * len(fake.calls)
            assert len(fake.calls) == 1 if window == 32 << 20 else len(fake.calls) < n_all // 4
            assert grep(k, count=True) == len(want[k])
            a, b = 700, 2100                                            # start / stop at line starts, stop inside a block
            va = bgzf.make_virtual_offset(coffs[starts[a] // 997], starts[a] % 997)
            vb = bgzf.make_virtual_offset(coffs[starts[b] // 997], starts[b] % 997)
            mid = grep(k, start=va, stop=vb, first=a)
            assert mid.numbers.tolist() == [i for i in want[k] if a <= i < b] and mid.searched == b - a
        # without mismatches the engine is called as it always was
        fake.calls.clear()
        res = grep(0)
        assert res.numbers.tolist() == want[0] and fake.exact_calls == len(fake.calls) > 0
        fake.exact_calls = 0


def _hipcc_clang():
    clang = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang++"
    return clang if os.path.exists(clang) else None


def test_hostile_arguments_under_asan_ubsan(tmp_path):
    """a stand-alone program, linked against the library's host side under the sanitizers and run as a plain child process"""
    import importlib.util
    clang = _hipcc_clang()
    if clang is None:
        pytest.skip("hipcc's clang is not on this host")
    spec = importlib.util.spec_from_file_location("zng_amd_build_asan", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = str(tmp_path / "libzng_amd_host_asan.so")
    mod.build_host_asan(so)
    exe = str(tmp_path / "grep_approx_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "grep_approx_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf grep approx arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

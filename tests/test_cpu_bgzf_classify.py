"""CPU: BGZF by nearest pattern, without a GPU -- the argument checks of bgzf.classify_records / demux that need no context; the two
zngamd_bgzf_classify_records entry points are declared, exported and bound, and refuse hostile arguments with no context at all; the
window loop on a stand-in engine whose rule is the numpy referee of classify_ref.py (stored-block BGZF written here, the system zlib
decodes it); and tests/classify_args.cpp, a stand-alone program, against the library's host side under AddressSanitizer +
UndefinedBehaviorSanitizer (a plain child process, nothing preloaded)."""
import ctypes as C
import io
import os
import re
import subprocess
import types
import zlib

import numpy as np
import pytest

import classify_ref
from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_grep import _stored_bgzf
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    monkeypatch.setattr(bgzf, "BgzfWriter", lambda *a, **kw: pytest.fail("an output was opened before the arguments were judged"))
    A, B = b"ACGTACGT", b"TTGTACGA"
    for pats in ([A, A], [A, B, bytearray(A)], [B, A, B, A]):                # duplicates
        with pytest.raises(ValueError, match="duplicate"):
            bgzf.classify_records(_Unreadable(), pats, 4)
        with pytest.raises(ValueError, match="duplicate"):
            bgzf.demux(_Unreadable(), pats, ["x"] * len(pats))
    bgzf._classify_patterns([A, A[:4], A + b"A"], b"\n")                     # a prefix of another pattern is allowed
    for pats, bad in (([A, B], -1), ([A, B], 17), ([A, b"ACGT"], 4), ([A, B], 1.0), ([A, B], None), ([A, B], True), ([b"A", b"C"], 1)):
        with pytest.raises(ValueError, match="mismatches"):
            bgzf.classify_records(_Unreadable(), pats, 4, match_line=1, first_byte=b"@", mismatches=bad)
        with pytest.raises(ValueError, match="mismatches"):
            bgzf.demux(_Unreadable(), pats, ["x", "y"], mismatches=bad)
    for outs in ([], ["only one"], ["a", "b", "c"], "one path for two patterns"):
        with pytest.raises(ValueError, match="one output per pattern"):
            bgzf.demux(_Unreadable(), [A, B], outs, mismatches=1)
    for kw in (dict(invert=True), dict(count=True), dict(max_count=3)):      # a classification has no complement and no early end
        with pytest.raises(TypeError):
            bgzf.classify_records(_Unreadable(), [A, B], 4, **kw)
        with pytest.raises(TypeError):
            bgzf.demux(_Unreadable(), [A, B], ["x", "y"], **kw)
    for kw in (dict(match_line=4), dict(first_byte=b"@@"), dict(max_record=0), dict(delimiter=b"ab")):
        with pytest.raises(ValueError):
            bgzf.classify_records(_Unreadable(), [A, B], 4, **kw)
    for k in (0, 65):
        with pytest.raises(ValueError, match="1 to 64 lines"):
            bgzf.classify_records(_Unreadable(), [A, B], k)
        with pytest.raises(ValueError, match="1 to 64 lines"):
            bgzf.demux(_Unreadable(), [A, B], ["x", "y"], k)
    with pytest.raises(ValueError):
        bgzf.demux(_Unreadable(), [A, B], ["x", "y"], block_size=0)
    assert (bgzf.UNASSIGNED, bgzf.AMBIGUOUS) == (-1, -2) and _lib.BGZF_CLASSIFY_GROUP == 16
    for name in ("classify_records", "demux"):
        assert name in bgzf.__all__ and hasattr(bgzf.BgzfReader, name)


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    for name, base, extra in (("zngamd_bgzf_classify_records_dev", "zngamd_bgzf_grep_records_approx_dev", "zngamd_bgzf_class_row *d_class"),
                              ("zngamd_bgzf_classify_records", "zngamd_bgzf_grep_records_approx", "zngamd_bgzf_class_row *class_rows")):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        params = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(",")]
        bparams = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % base, header).group(1).split(",")]
        at = params.index(extra)
        want = bparams[:at] + [extra, "uint64_t class_cap"] + bparams[at:]       # the records call's parameters, the class rows in front of the rows
        assert params[:-1] == want[:-1] and params[-1] == "zngamd_bgzf_classify_totals *totals", name
        assert len(getattr(L, name).argtypes) == len(params), name
        assert getattr(L, name).argtypes == getattr(L, base).argtypes[:at] + [C.c_void_p, C.c_uint64] + getattr(L, base).argtypes[at:], name
    assert _lib.CLASS_ROW_DTYPE.itemsize == 4 and _lib.CLASS_ROW_DTYPE.names == ("pattern", "other", "distance", "flags")
    assert re.search(r"\}\s*zngamd_bgzf_class_row;\s*/\* 4 B \*/", header)
    n = int(re.search(r"#define ZNGAMD_BGZF_CLASSIFY_MAX_CLASSES\s+(\d+)u", header).group(1))
    assert n == _lib.BGZF_CLASSIFY_MAX_CLASSES == 66 == _lib.BGZF_GREP_MAX_PATTERNS + 2
    size = int(re.search(r"\}\s*zngamd_bgzf_classify_totals;\s*/\* (\d+) B \*/", header).group(1))
    assert size == C.sizeof(_lib.BgzfClassifyTotals) == 5 * 8 + 4 * 4 + 2 * 8 * n
    body = re.search(r"typedef struct \{([^}]*)\}\s*zngamd_bgzf_classify_totals;", header).group(1)
    fields = re.findall(r"\b(\w+)(?:\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in _lib.BgzfClassifyTotals._fields_]
    assert _lib.BgzfClassifyTotals.covered.offset == 40 and _lib.BgzfClassifyTotals.class_bytes.offset == 56 + 8 * n
    assert int(re.search(r"#define ZNGAMD_BGZF_CLASSIFY_GROUP\s+(\d+)u", header).group(1)) == _lib.BGZF_CLASSIFY_GROUP
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_classify.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_classify.hip"))


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every hostile table the calls with mismatches refuse, for duplicate patterns and forbidden flags"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    blob = b"needle" + b"x" * 300
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP

    def call(form, b, rows, k, delim=10, totals=True, n=None, flags=F, rec=(4, 1, 64)):
        mem = (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b or b"\0") if b is not None else None
        tab = (C.c_uint32 * max(2 * len(rows), 1))(*[x for row in rows for x in row]) if rows is not None else None
        n = (len(rows) if rows is not None else 3) if n is None else n
        t = _lib.BgzfClassifyTotals()
        head = (None, None, 0, None, 0, 0, 0, mem, len(b or b""), tab, n, delim, flags, k, *rec, 0)
        if form == 0:
            return L.zngamd_bgzf_classify_records(*head, None, None, 0, None, 0, None, 0, _lib.ALLOC_FN(), None, C.byref(t) if totals else None)
        return L.zngamd_bgzf_classify_records_dev(*head, None, 0, None, None, 0, None, 0, None, 0, C.byref(t) if totals else None)

    for form in range(2):
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
        # duplicates: the same row twice, the same bytes at two places, far apart in the table
        for rows in ([(0, 6), (0, 6)], [(6, 5), (11, 5)], [(0, 6), (6, 9), (2, 3), (0, 6)], [(10, 200), (50, 200)]):
            assert call(form, blob, rows, 1) == E_ARG, (form, rows)
        for flags in (_lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_COUNT_ONLY, F | _lib.BGZF_GREP_INVERT, G | _lib.BGZF_GREP_COUNT_ONLY, 32, G | 64, 1 << 31):
            assert call(form, blob, [(0, 6)], 1, flags=flags) == E_ARG, (form, flags)
        for rec in ((0, -1, -1), (65, -1, -1), (4, -2, -1), (4, 4, -1), (4, 1, -2), (4, 1, 256)):
            assert call(form, blob, [(0, 6)], 1, rec=rec) == E_ARG, (form, rec)
        for flags in (0, F, G, F | G | _lib.BGZF_GREP_LINE_START):                 # (in order but for the context)
            assert call(form, blob, [(0, 6), (1, 6)], 1, flags=flags) == E_ARG and call(form, blob, [(0, 6)], 0, flags=flags) == E_ARG


class _FakeClassifyCtx:
    """ctx.bgzf_classify_records computed on the host: the blocks through the system zlib, the rule by classify_ref"""

    def __init__(self):
        self.calls = []

    def bgzf_classify_records(self, data, members, text_off, text_end, blob, table, delim, flags, mismatches, k, match_line=-1, first_byte=-1,
                              record_base=0, caps=None):
        from zlib_ng_amd import _lib
        assert not flags & ~(_lib.BGZF_GREP_LINE_START | _lib.BGZF_GREP_FINAL | _lib.BGZF_CLASSIFY_GROUP)
        data = bytes(data)
        buf = bytearray(int((members["out_off"] + members["out_len"]).max()) if len(members) else 0)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        self.calls.append((len(members), text_off, text_end, flags, record_base, mismatches))
        text, d = bytes(buf[text_off:text_end]), bytes([delim])
        pats = [blob[o:o + n] for o, n in table.tolist()]
        final = bool(flags & _lib.BGZF_GREP_FINAL)
        lines = classify_ref.lines_of(text, d)
        if lines and not lines[-1].endswith(d) and not final:
            lines.pop()
        nrec = (len(lines) + k - 1) // k if final else len(lines) // k
        whole = b"".join(lines[:k * nrec])
        v = classify_ref.classify(whole, d, pats, mismatches, k, match_line if match_line >= 0 else None, bool(flags & _lib.BGZF_GREP_LINE_START))
        assert len(v.records) == nrec
        starts = np.concatenate([[0], np.cumsum([len(x) for x in v.records])]).astype(np.int64) + text_off
        tot = types.SimpleNamespace(seen=nrec, matched=nrec, bytes=len(whole), covered=1, bad=0, bad_record=0, bad_src=0,
                                    tail_off=text_end if final else int(starts[nrec]), short_lines=len(lines) % k if final else 0,
                                    n_classes=len(pats) + 2, class_records=np.zeros(66, np.uint64), class_bytes=np.zeros(66, np.uint64))
        if first_byte >= 0:
            bad = [r for r in range(nrec) if v.records[r][0] != first_byte]
            if bad:
                tot.bad, tot.bad_record, tot.bad_src = 1, record_base + bad[0], int(starts[bad[0]])
        tot.class_records[:len(v.counts)] = v.counts
        for c in range(len(pats) + 2):
            tot.class_bytes[c] = len(v.of_class(c))
        none = (np.empty(0, _lib.CLASS_ROW_DTYPE), np.empty(0, _lib.GREP_ROW_DTYPE), b"")
        if tot.bad or not nrec:
            return (0, np.zeros(len(members), np.int32), tot) + none
        rows = np.zeros(nrec, _lib.CLASS_ROW_DTYPE)
        rows["pattern"], rows["other"], rows["distance"] = v.tie[:, 0].astype(np.uint8), v.tie[:, 1].astype(np.uint8), v.distance
        rows["flags"] = np.where(v.pattern >= 0, 1, np.where(v.pattern == classify_ref.AMBIGUOUS, 2, 0))
        if not flags & _lib.BGZF_CLASSIFY_GROUP:
            return 0, np.zeros(len(members), np.int32), tot, rows, none[1], b""
        order = np.argsort(v.cls, kind="stable")
        grows = np.zeros(nrec, _lib.GREP_ROW_DTYPE)
        grows["src_off"], grows["number"] = starts[:-1][order], record_base + order
        grows["len"], grows["reserved"] = np.diff(starts)[order], rows.view(np.uint32)[order]
        return 0, np.zeros(len(members), np.int32), tot, rows, grows, b"".join(v.of_class(c) for c in range(len(pats) + 2))


class _Collect(io.BytesIO):
    """BgzfWriter replaced: what a class was given, and whether it was closed"""
    made = []

    def __init__(self, target, mode="wb", compresslevel=6, *, block_size=None):
        super().__init__()
        self.target, self.level, self.got = target, compresslevel, None
        _Collect.made.append(self)

    def close(self):
        if self.got is None:
            self.got = self.getvalue()
        super().close()


def _reads(n, barcodes, seed=3):
    """FASTQ reads whose bases begin with a barcode at distance 0, 1 or 2, with two barcodes at the same distance, or with none"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        bc = bytearray(barcodes[int(rng.integers(len(barcodes)))])
        kind = i % 7
        for at in rng.choice(len(bc), (0, 1, 2, 0, 1, 0, 0)[kind], replace=False).tolist():
            bc[at] = ord("N")
        if kind == 5:
            bc = bytearray(b"N" * len(bc))
        seq = bytes(bc) + bytes(rng.choice(list(b"ACGT"), int(rng.integers(5, 70))).tolist())
        if kind == 6:
            seq += barcodes[(i // 7) % len(barcodes)]                     # a second barcode further on: a tie or the same one twice
        out.append(b"@r%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq)))
    return out


def test_driver_on_a_fake_engine(monkeypatch):
    from zlib_ng_amd import _lib, bgzf
    barcodes = [b"ACGTACGTAC", b"TTGCATGCAA", b"GGATCCGGAT", b"CATGCATGTT"]
    recs = _reads(700, barcodes)
    data = b"".join(recs)
    BS = 997
    blob, blocks = _stored_bgzf(data, BS)
    coffs = sorted(blocks)
    fake = _FakeClassifyCtx()
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)
    monkeypatch.setattr(bgzf, "BgzfWriter", _Collect)
    want = {k: classify_ref.classify(data, b"\n", barcodes, k, 4, 1) for k in (0, 1, 2)}
    assert want[1].records == recs
    for k in (1, 2):                                     # the input holds every kind of verdict, and k changes it
        assert (want[k].pattern >= 0).any() and (want[k].pattern == bgzf.AMBIGUOUS).any() and (want[k].pattern == bgzf.UNASSIGNED).any()
    assert want[0].counts.tolist() != want[1].counts.tolist() != want[2].counts.tolist()
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    voff = lambda r: bgzf.make_virtual_offset(coffs[starts[r] // BS], int(starts[r] % BS))

    def classify(k, **kw):
        args = dict(match_line=1, first_byte=b"@", line_start=False, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False)
        args.update(kw)
        return bgzf._classify_file(io.BytesIO(blob), fake, barcodes, 4, args["match_line"], args["first_byte"], b"\n", args["line_start"], args["start"],
                                   args["stop"], args["first_record"], args["max_record"], args["allow_short"], k, None)

    def same(res, v, lo=0, hi=None):
        hi = len(v.pattern) if hi is None else hi
        assert res.pattern.tolist() == v.pattern[lo:hi].tolist() and res.distance.tolist() == v.distance[lo:hi].tolist()
        assert res.tie.tolist() == v.tie[lo:hi].tolist() and res.searched == hi - lo
        assert res.counts.tolist() == np.bincount(v.cls[lo:hi], minlength=len(barcodes) + 2).tolist()
        assert res.pattern.dtype == np.int16 and res.distance.dtype == np.uint8 and res.tie.shape == (hi - lo, 2)

    for window in (32 << 20, 5000, 1500):
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        for k in (0, 1, 2):
            fake.calls.clear()
            same(classify(k), want[k])
            assert [c[5] for c in fake.calls] == [k] * len(fake.calls) and not any(c[3] & _lib.BGZF_CLASSIFY_GROUP for c in fake.calls)
            assert fake.calls[-1][3] & _lib.BGZF_GREP_FINAL and not any(c[3] & _lib.BGZF_GREP_FINAL for c in fake.calls[:-1])
            if window == 32 << 20:
                assert len(fake.calls) == 1
            else:
                assert len(fake.calls) > 10 and any(c[1] > 0 for c in fake.calls[1:])      # an open record was carried into the next window
                assert [c[4] for c in fake.calls] == sorted(c[4] for c in fake.calls)
        same(classify(1, line_start=True), classify_ref.classify(data, b"\n", barcodes, 1, 4, 1, True))
        same(classify(1, match_line=None, first_byte=None), classify_ref.classify(data, b"\n", barcodes, 1, 4))
        a, b = 123, 500                                  # start / stop at record starts, stop inside a block
        mid = classify(2, start=voff(a), stop=voff(b), first_record=a)
        same(mid, want[2], a, b)
        assert mid.first_record == a
        # demux: every class's bytes are the referee's records of that class in input order; together they are the whole text
        for k, drop in ((1, False), (2, True)):
            _Collect.made.clear()
            fake.calls.clear()
            outs = ["out%d" % i for i in range(len(barcodes))]
            counts = bgzf._demux_file(io.BytesIO(blob), fake, barcodes, outs, 4, None if drop else "amb", "una", 1, bgzf.MAX_BLOCK_INPUT, 1, b"@", b"\n",
                                      False, None, None, 0, 64 << 20, False, k)
            assert counts.tolist() == want[k].counts.tolist() and all(c[3] & _lib.BGZF_CLASSIFY_GROUP for c in fake.calls)
            made = {w.target: w for w in _Collect.made}
            assert sorted(made) == sorted(outs + ["una"] + ([] if drop else ["amb"])) and all(w.closed and w.level == 1 for w in made.values())
            for i, name in enumerate(outs + ["amb", "una"]):
                if name in made:
                    assert made[name].got == want[k].of_class(i), (window, k, name)
            total = sum(len(w.got) for w in made.values())
            assert total == len(data) - (len(want[k].of_class(len(barcodes))) if drop else 0)
            if not drop:
                assert sorted(b"".join(w.got for w in made.values()).split(b"\n")) == sorted(data.split(b"\n"))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1500)
    # a short last record
    cut = data[:data.rfind(b"\n", 0, len(data) - 1) + 1]                     # the last read without its quality line
    sblob, _ = _stored_bgzf(cut, BS)
    with pytest.raises(ValueError, match=r"record 699, the last one, has 3 of 4 lines"):
        bgzf._classify_file(io.BytesIO(sblob), fake, barcodes, 4, 1, b"@", b"\n", False, None, None, 0, 64 << 20, False, 1, None)
    res = bgzf._classify_file(io.BytesIO(sblob), fake, barcodes, 4, 1, b"@", b"\n", False, None, None, 0, 64 << 20, True, 1, None)
    same(res, classify_ref.classify(cut, b"\n", barcodes, 1, 4, 1))
    # an error on the way: the outputs written so far are closed and the error says that they are incomplete
    lines = data.split(b"\n")
    del lines[4 * 600 + 2]
    bblob, _ = _stored_bgzf(b"\n".join(lines), BS)
    _Collect.made.clear()
    with pytest.raises(ValueError, match=r"record 601 at virtual offset \d+ does not start with b'@'.*incomplete"):
        bgzf._demux_file(io.BytesIO(bblob), fake, barcodes, ["o%d" % i for i in range(4)], 4, "amb", "una", 6, bgzf.MAX_BLOCK_INPUT, 1, b"@", b"\n", False,
                         None, None, 0, 64 << 20, False, 1)
    assert len(_Collect.made) == 6 and all(w.closed for w in _Collect.made) and sum(len(w.got) for w in _Collect.made) > 0
    assert sum(len(w.got) for w in _Collect.made) < len(data)                        # (some windows were written before the bad record was met)


def test_classify_result():
    from zlib_ng_amd import bgzf
    r = bgzf.ClassifyResult([0, -1, -2], [1, 255, 2], [[0, 0], [-1, -1], [1, 3]], [1, 0, 0, 0, 1, 1], 10)
    assert len(r) == r.searched == 3 and r.first_record == 10 and r.tie.shape == (3, 2) and "3 records" in repr(r)
    with pytest.raises(ValueError):
        bgzf.ClassifyResult([0, 1], [1], [[0, 0], [1, 1]], [1, 1, 0, 0])


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
    exe = str(tmp_path / "classify_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "classify_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf classify arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

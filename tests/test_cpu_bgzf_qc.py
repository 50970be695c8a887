"""CPU: BGZF quality control, without a GPU -- the referee of qc_ref.py against tables written out by hand; the argument checks of
bgzf.qc_records that need no context; the two zngamd_bgzf_qc_records entry points are declared, exported and bound, and refuse hostile
arguments with no context at all; QcResult and its sum; and tests/qc_args.cpp, a stand-alone program, against the library's host side
under AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process, nothing preloaded)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import qc_ref
from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang

# three reads at cycles = 4: a lower-case base, an N, a quality below the base (a blank: -1) and one above base + 93 (0x7f: 94); an empty
# read; a read of 7 bases, longer than cycles, with two bytes of class 5
TINY = b"@a\nAcGN\n+\nI! \x7f\n" + b"@b\n\n+\n\n" + b"@c\nACGT.RT\n+\n5555+5?\n"


def test_referee_against_tables_written_by_hand():
    r = qc_ref.qc_text(TINY, qc_ref.conf(cycles=4, low_quality=15, first_byte=b"@"))
    assert r.base_pos == [[2, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0], [0, 0, 0, 1, 1, 0], [0, 0, 0, 1, 0, 2]]
    q = [[0] * 94 for _ in range(5)]
    q[0][40] = q[0][20] = 1
    q[1][0] = q[1][20] = 1
    q[2][0] = q[2][20] = 1
    q[3][93] = q[3][20] = 1
    q[4][10] = q[4][20] = q[4][30] = 1
    assert r.qual_pos == q
    assert r.length_hist == [1, 0, 0, 0, 1, 1]
    assert [i for i, v in enumerate(r.gc_hist) if v] == [28, 50] and sum(r.gc_hist) == 2
    assert [i for i, v in enumerate(r.meanq_hist) if v] == [20, 33] and sum(r.meanq_hist) == 2
    assert r.totals == dict(seen=3, bytes_in=43, bases=11, min_len=0, max_len=7, empty=1, base_total=[2, 2, 2, 2, 1, 2], quality_sum=273, q20_bases=8,
                            q30_bases=3, low_bases=3, quality_clamped=2)
    assert r.rows == [(133, 4, 2, 1, 2), (0, 0, 0, 0, 0), (140, 7, 2, 0, 1)]
    assert len(qc_ref.flat(r)) == qc_ref.table_words(4) == 5 * 100 + 6 + 101 + 94
    # cycles beyond every read: the last row and the last length entry stay empty; quality_base 64; no qualities
    r = qc_ref.qc_text(TINY, qc_ref.conf(cycles=7))
    assert r.base_pos[7] == [0] * 6 and r.base_pos[6] == [0, 0, 0, 1, 0, 0] and r.length_hist == [1, 0, 0, 0, 1, 0, 0, 1, 0]
    r = qc_ref.qc_text(b"@a\nAC\n+\n@h\n", qc_ref.conf(quality_base=64, low_quality=1))
    assert r.rows == [(40, 2, 1, 0, 1)] and r.totals["quality_clamped"] == 0
    r = qc_ref.qc_text(b">a\nacgu\n>b\nGG\n", qc_ref.conf(record_lines=2, qual_line=None, cycles=2))
    assert r.base_pos == [[1, 0, 1, 0, 0, 0], [0, 1, 1, 0, 0, 0], [0, 0, 1, 0, 0, 1]] and not any(map(any, r.qual_pos)) and not any(r.meanq_hist)
    assert r.gc_hist[50] == r.gc_hist[100] == 1 and r.totals["quality_sum"] == 0 and r.rows == [(0, 4, 2, 0, 0), (0, 2, 2, 0, 0)]
    # nothing at all; the faults, the smaller record first, a record with both for its first byte; a short last record
    r = qc_ref.qc_text(b"", qc_ref.conf())
    assert r.totals["seen"] == 0 and r.totals["min_len"] == 2 ** 64 - 1 and not any(qc_ref.flat(r))
    ok, longer, both = b"@a\nAC\n+\nII\n", b"@b\nAC\n+\nIII\n", b"xc\nAC\n+\nI\n"
    for text, want in ((ok + longer + both, (3, 1)), (longer + both, (3, 0)), (both, (1, 0)), (ok + both + longer, (1, 1))):
        with pytest.raises(qc_ref.Fault) as e:
            qc_ref.qc_text(text, qc_ref.conf(first_byte=b"@"))
        assert (e.value.kind, e.value.record) == want
    r = qc_ref.qc_text(b"@a\nAC\n+\nII\n@s\n", qc_ref.conf())
    assert r.rows == [(80, 2, 1, 0, 0), (0, 0, 0, 0, 0)] and r.totals["bytes_in"] == 14
    assert qc_ref.qc_text(b"@a\nAC\n+\nII\n@s\n", qc_ref.conf(), final=False).totals["seen"] == 1


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    f = _Unreadable()
    for kw in (dict(seq_line=4), dict(seq_line=-1), dict(qual_line=4), dict(qual_line=1), dict(seq_line=3), dict(quality_base=256), dict(quality_base=-1),
               dict(quality_base=33.0), dict(cycles=0), dict(cycles=4097), dict(cycles=True), dict(cycles=None), dict(low_quality=94), dict(low_quality=-1),
               dict(per_record=1), dict(per_record="yes"), dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(record_lines=0), dict(record_lines=65),
               dict(max_record=0)):
        with pytest.raises(ValueError):
            bgzf.qc_records(f, **kw)
    with pytest.raises(ValueError, match="seq_line and qual_line are two lines of the record, not both 1"):
        bgzf.qc_records(f, qual_line=1)
    with pytest.raises(ValueError, match="cycles is an integer between 1 and 4096, not 5000"):
        bgzf.qc_records(f, cycles=5000)
    for kw in (dict(match_line=1), dict(patterns=[b"A"]), dict(output="x"), dict(drop=[0])):
        with pytest.raises(TypeError):
            bgzf.qc_records(f, **kw)
    with pytest.raises(ValueError):
        bgzf.qc_records("/nonexistent/reads.fq.gz", record_lines=0)                        # (judged before the file is opened)
    with pytest.raises(ValueError):
        bgzf.qc_records("/nonexistent/reads.fq.gz", cycles=0)
    cf, d = bgzf._qc_conf(4, 1, 3, 33, np.int64(100), 20, True, b"@", b"\n")
    assert (cf.record_lines, cf.seq_line, cf.qual_line, cf.first_byte, cf.quality_base, cf.cycles, cf.low_quality, cf.flags, list(cf.reserved), d) == \
        (4, 1, 3, 64, 33, 100, 20, _lib.BGZF_QC_ROWS, [0] * 8, b"\n")
    cf, d = bgzf._qc_conf(2, 1, None, 64, 1, 0, False, None, b";")
    assert (cf.qual_line, cf.first_byte, cf.flags, d) == (-1, -1, 0, b";")
    for name in ("qc_records", "QcResult"):
        assert name in bgzf.__all__
    want = ["file", "record_lines", "seq_line", "qual_line", "quality_base", "cycles", "low_quality", "per_record", "first_byte", "delimiter", "start", "stop",
            "first_record", "max_record", "allow_short"]
    sig = inspect.signature(bgzf.qc_records).parameters
    assert list(sig) == want and list(inspect.signature(bgzf.BgzfReader.qc_records).parameters) == ["self"] + want[1:]
    defaults = {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(record_lines=4, seq_line=1, qual_line=3, quality_base=33, cycles=512, low_quality=15, per_record=False, first_byte=None,
                            delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.items() if k not in ("file", "record_lines"))


def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, header).group(1)
    return [re.sub(r"\[.*", "", x) for x in re.findall(r"\b(\w+(?:\[\w+\])?);", re.sub(r"/\*.*?\*/", "", body))]


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32, "zngamd_alloc_fn": _lib.ALLOC_FN}
    for name in ("zngamd_bgzf_qc_records_dev", "zngamd_bgzf_qc_records"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        params = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(",")]
        want = []
        for p in params:
            t = p.rsplit(" ", 1)[0] if "*" not in p else None
            want.append(C.c_void_p if t is None else ctype[t])
        assert getattr(L, name).argtypes == want, name
        assert "const zngamd_bgzf_qc_conf *conf" in params and params[-1] == "zngamd_bgzf_qc_totals *totals"
        # the window as zngamd_bgzf_grep_records takes it
        assert params[1:7] == [re.sub(r"\s+", " ", x).strip() for x in
                               re.search(r"\bint %s\s*\(([^;]*)\);" % name.replace("qc", "grep"), header).group(1).split(",")][1:7]
    dev = re.search(r"\bint zngamd_bgzf_qc_records_dev\s*\(([^;]*)\);", header).group(1)
    for a, b in (("d_status", "d_tables"), ("d_tables", "tables_cap"), ("tables_cap", "d_rows"), ("d_rows", "rows_cap"), ("rows_cap", "totals")):
        assert dev.index(a) < dev.index(b)
    for struct, ct, size in (("zngamd_bgzf_qc_conf", _lib.BgzfQcConf, 64), ("zngamd_bgzf_qc_totals", _lib.BgzfQcTotals, 6 * 8 + 6 * 8 + 5 * 8 + 3 * 8 + 4 * 4)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert int(re.search(r"\}\s*zngamd_bgzf_qc_row;\s*/\* (\d+) B \*/", header).group(1)) == _lib.QC_ROW_DTYPE.itemsize == 24
    assert _struct_fields(header, "zngamd_bgzf_qc_row") == list(_lib.QC_ROW_DTYPE.names)
    assert _lib.BgzfQcTotals.min_len.offset == 24 and _lib.BgzfQcTotals.base_total.offset == 48 and _lib.BgzfQcTotals.tail_off.offset == 136
    assert _lib.BgzfQcTotals.covered.offset == 160 and _lib.BgzfQcTotals.bad.offset == 168
    for macro, value in (("MAX_CYCLES", _lib.BGZF_QC_MAX_CYCLES), ("BASES", _lib.BGZF_QC_BASES), ("QUALITIES", _lib.BGZF_QC_QUALITIES),
                         ("MAX_LOW", _lib.BGZF_QC_MAX_LOW), ("GC_BINS", _lib.BGZF_QC_GC_BINS), ("ROWS", _lib.BGZF_QC_ROWS)):
        assert int(re.search(r"#define ZNGAMD_BGZF_QC_%s\s+(\d+)u" % macro, header).group(1)) == value
    assert "#define ZNGAMD_BGZF_QC_TABLE_WORDS(C)" in header
    for c in (1, 64, 512, 4096):
        assert _lib.bgzf_qc_table_words(c) == qc_ref.table_words(c) == (c + 1) * 100 + c + 2 + 101 + 94
        parts = _lib.bgzf_qc_split(np.arange(_lib.bgzf_qc_table_words(c)), c)
        assert [p.shape for p in parts] == [(c + 1, 6), (c + 1, 94), (c + 2,), (101,), (94,)] and parts[4][-1] == _lib.bgzf_qc_table_words(c) - 1
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_qc.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_qc.hip"))
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_trim.hip"') < main.index('#include "za_qc.hip"')


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every hostile configuration, delimiter, flag and NULL pointer -- and with everything in order"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    F = _lib.BGZF_GREP_FINAL

    def call(form, delim=10, flags=F, totals=True, with_conf=True, tables=True, rows=True, alloc=False, **fields):
        cf = _lib.BgzfQcConf(4, 1, 3, 64, 33, 512, 15, _lib.BGZF_QC_ROWS)
        for k, v in fields.items():
            if k == "reserved":
                cf.reserved[v] = 1
            else:
                setattr(cf, k, v)
        t = _lib.BgzfQcTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        tab, row = np.full(1, 7, np.uint64), np.zeros(1, _lib.QC_ROW_DTYPE)
        tp, rp = C.c_void_p(tab.ctypes.data) if tables else None, C.c_void_p(row.ctypes.data) if rows else None
        head = (None, None, 0, None, 0, 0, 0, delim, flags, C.byref(cf) if with_conf else None, 0)
        tail = (C.byref(t) if totals else None,)
        if form == 0:
            fn = _lib.ALLOC_FN(lambda user, n: pytest.fail("the allocator was called")) if alloc else _lib.ALLOC_FN()
            r = L.zngamd_bgzf_qc_records(*head, None, tp, 0, rp, 0, fn, None, *tail)
        else:
            r = L.zngamd_bgzf_qc_records_dev(*head, None, 0, None, tp, 0, rp, 0, *tail)
        assert bytes(t) == b"\x5A" * C.sizeof(t) and tab[0] == 7 and not row["len"][0]      # a refused call writes nothing
        return r

    for form in range(2):
        for fields in (dict(record_lines=0), dict(record_lines=65), dict(seq_line=-1), dict(seq_line=4), dict(qual_line=-2), dict(qual_line=4), dict(qual_line=1),
                       dict(first_byte=-2), dict(first_byte=256), dict(quality_base=256), dict(cycles=0), dict(cycles=4097), dict(low_quality=94), dict(flags=2),
                       dict(flags=3), dict(reserved=0), dict(reserved=7)):
            assert call(form, **fields) == E_ARG, (form, fields)
        for kw in (dict(delim=-1), dict(delim=256), dict(flags=F | 1), dict(flags=F | 2), dict(flags=F | 8), dict(flags=F | 16), dict(flags=1 << 31),
                   dict(totals=False), dict(with_conf=False), dict(tables=False), dict(rows=False)):
            assert call(form, **kw) == E_ARG, (form, kw)
        assert call(form) == E_ARG                                                         # in order, but no context
    assert call(0, rows=False, alloc=True) == E_ARG


def _result(res, cycles, low_quality=15, rows=True):
    """a QcResult of the referee's figures, as bgzf's sink builds one"""
    from zlib_ng_amd import _lib, bgzf
    t = res.totals
    totals = {k: t[k] for k in bgzf._QC_TOTALS}
    totals.update(records=t["seen"], min_len=t["min_len"] if t["seen"] else 0, max_len=t["max_len"])
    arr = None
    if rows:
        arr = np.array(res.rows, dtype=np.int64).reshape(-1, 5)
        arr = np.rec.fromarrays([arr[:, 0].astype(np.uint64)] + [arr[:, i].astype(np.uint32) for i in range(1, 5)], dtype=_lib.QC_ROW_DTYPE)
    return bgzf.QcResult(cycles, low_quality, np.array(qc_ref.flat(res), np.int64), totals, np.array(t["base_total"], np.int64), arr)


def _same(result, want, rows=True):
    t = want.totals
    assert result.base_pos.tolist() == want.base_pos and result.qual_pos.tolist() == want.qual_pos and result.length_hist.tolist() == want.length_hist
    assert result.gc_hist.tolist() == want.gc_hist and result.meanq_hist.tolist() == want.meanq_hist
    assert all(a.dtype == np.int64 for a in (result.base_pos, result.qual_pos, result.length_hist, result.gc_hist, result.meanq_hist, result.base_total))
    assert result.records == len(result) == t["seen"] and result.base_total.tolist() == t["base_total"]
    for name in ("bytes_in", "bases", "max_len", "empty", "quality_sum", "q20_bases", "q30_bases", "low_bases", "quality_clamped"):
        assert getattr(result, name) == t[name] and type(getattr(result, name)) is int, name
    assert result.min_len == (t["min_len"] if t["seen"] else 0)
    if rows:
        got = list(zip(result.quality_sum_per_record.tolist(), result.length.tolist(), result.gc.tolist(), result.n_bases.tolist(),
                       result.low_bases_per_record.tolist()))
        assert got == want.rows
    else:
        assert result.length is None and result.gc is None and result.n_bases is None and not result.per_record


def test_result_and_its_sum():
    cf = qc_ref.conf(cycles=4)
    second = b"@d\nGGCCGGCC\n+\nIIIIII##\n@e\nA\n+\n#\n"
    a, b, whole = qc_ref.qc_text(TINY, cf), qc_ref.qc_text(second, cf), qc_ref.qc_text(TINY + second, cf)
    ra, rb = _result(a, 4), _result(b, 4)
    _same(ra, a)
    s = ra + rb
    _same(s, whole)
    _same(s, qc_ref.add(a, b))
    assert (s.min_len, s.max_len, s.records, s.cycles, s.low_quality) == (0, 8, 5, 4, 15)
    _same(ra, a)                                                                           # (the parts are left as they were)
    _same(ra.merge(rb), whole)
    # the shortest read comes from the parts that hold a record
    empty = _result(qc_ref.qc_text(b"", cf), 4)
    assert (empty.records, empty.min_len, empty.max_len, empty.mean_length, empty.q20_rate, empty.gc_fraction) == (0, 0, 0, 0.0, 0.0, 0.0)
    _same(rb + empty, b)
    _same(empty + rb, b)
    assert (rb + empty).min_len == 1 and (empty + empty).records == 0
    # rows only when both parts have them
    _same(ra + _result(b, 4, rows=False), whole, rows=False)
    with pytest.raises(ValueError, match="cycles 4 and 5"):
        ra + _result(qc_ref.qc_text(second, qc_ref.conf(cycles=5)), 5)
    with pytest.raises(ValueError):
        ra + _result(b, 4, low_quality=20)
    with pytest.raises(TypeError):
        ra + 1
    # the derived figures are arithmetic on the counts
    t = whole.totals
    assert s.mean_length == t["bases"] / 5 and s.q20_rate == t["q20_bases"] / t["bases"] and s.q30_rate == t["q30_bases"] / t["bases"]
    assert s.gc_fraction == (t["base_total"][1] + t["base_total"][2]) / t["bases"]
    mq = s.mean_quality_by_cycle()
    assert mq.shape == (5,) and mq[0] == (40 + 20 + 40 + 2) / 4 and mq[4] == (10 + 20 + 30 + 40 + 40 + 2 + 2) / 7
    bf = s.base_fraction_by_cycle()
    assert bf.shape == (5, 6) and bf[0].tolist() == [0.75, 0, 0.25, 0, 0, 0] and np.allclose(bf.sum(axis=1), 1)
    far = _result(qc_ref.qc_text(b"@a\nAC\n+\nII\n", qc_ref.conf(cycles=4)), 4)
    assert np.isnan(far.mean_quality_by_cycle()[2:]).all() and np.isnan(far.base_fraction_by_cycle()[3]).all()
    assert repr(s) == f"<QcResult: 5 records, 20 bases, lengths 0 .. 8, Q20 {100 * s.q20_rate:.1f} %, Q30 {100 * s.q30_rate:.1f} %, GC {100 * s.gc_fraction:.1f} %>"


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
    exe = str(tmp_path / "qc_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "qc_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf qc arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

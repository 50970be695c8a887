"""CPU: BGZF trimmed, without a GPU -- the referee of trim_ref.py on the literal cases of the rule and on whole records; the argument
checks of bgzf.trim_records that need no context; the two zngamd_bgzf_trim_records entry points are declared, exported and bound, and
refuse hostile arguments with no context at all; the window loop on a stand-in engine whose rule is the referee (stored-block BGZF
written here, the system zlib decodes it); and tests/trim_args.cpp, a stand-alone program, against the library's host side under
AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process, nothing preloaded)."""
import ctypes as C
import io
import os
import re
import subprocess
import types
import zlib

import numpy as np
import pytest

import trim_ref
from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_classify import _Collect
from test_cpu_bgzf_grep import _stored_bgzf
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang

ADAPTERS = [b"AGATCGGAAGAGCACACGTC", b"CTGTCTCTTATACACATCT", b"TGGAATTCTCGG"]


def test_referee_quality_literals():
    for qual, cutoffs, want in ((b"IIII##I#", (0, 20), (0, 7)), (b"IIII#I##", (0, 20), (0, 6)), (b"I#5#", (0, 20), (0, 1)), (b"II#I#", (0, 3), (0, 4)),
                                (b"##III#I#IIII", (20, 20), (2, 12)), (b"#I##IIII", (20, 0), (1, 8)), (b"####", (20, 20), (4, 4))):
        assert trim_ref.quality_cut(qual, 0, len(qual), cutoffs[0], cutoffs[1], 33) == want, qual
    for cutoffs in ((0, 0), (20, 20), (93, 93), (0, 1)):
        assert trim_ref.quality_cut(b"", 0, 0, *cutoffs, 33) == (0, 0)
    # the stop is part of the rule: the plain argmax of the suffix sums would cut IIII##I# at 4
    sums = np.cumsum([20 - (c - 33) for c in b"IIII##I#"[::-1]])[::-1]
    assert int(np.argmax(sums)) == 4
    # a byte below the base is a negative quality; both scans run over the [a, b) of the fixed cut
    assert trim_ref.quality_cut(b"III ", 0, 4, 0, 20, 33) == (0, 3) and trim_ref.quality_cut(b"\x00III", 0, 4, 20, 0, 33) == (1, 4)
    assert trim_ref.quality_cut(b"#III#", 1, 4, 20, 20, 33) == (1, 4) and trim_ref.quality_cut(b"hhhB", 0, 4, 0, 20, 64) == (0, 3)


def test_referee_adapter_literals():
    ads = [b"AGATCGGAAG", b"AGATCTTTTT"]
    none = trim_ref.NO_ADAPTER
    for R, k, want in ((b"TTTTAGATCGGAAGCC", 0, (4, 0)), (b"TTTTAGATCGG", 0, (4, 0)), (b"TTTTAGATC", 0, (4, 0)), (b"TTTTTTTAGA", 0, (7, 0)),
                       (b"TTTTTTTTAG", 0, None), (b"AGA", 0, (0, 0)), (b"GA", 0, None), (b"TTTTAGATCGGTAG", 1, (4, 0)), (b"TTTTAGATCGGTA", 1, None),
                       (b"CCCCAGATCTGAAG", 1, (4, 0))):
        assert trim_ref.adapter_cut(R, ads, k, 3) == (want if want else (len(R), none)), R
    assert trim_ref.adapter_cut(b"TTTTAGATCT", ads, 0, 3) == (4, 1) and trim_ref.adapter_cut(b"", ads, 0, 3) == (0, none)
    assert trim_ref.adapter_cut(b"TTTA", ads, 0, 1) == (3, 0) and trim_ref.adapter_cut(b"TTTAG", [b"AG"], 0, 5) == (3, 0)      # min_overlap 1; larger than the adapter


def test_referee_on_whole_records():
    c = trim_ref.conf
    rec = b"@r1\nACGTACGTAC\n+\nIIIIIIII##\n"
    two = rec + b"@r2\nTTTTAGATCGG\n+\nIIIIIIIIIII\n"
    r = trim_ref.trim_text(rec, c(cut=(2, 3)))
    assert (r.begin, r.end, r.steps, r.kept_bytes) == ([2], [7], [1], [b"@r1\nGTACG\n+\nIIIII\n"])
    r = trim_ref.trim_text(rec, c(quality=(0, 20)))
    assert (r.begin, r.end, r.steps, r.kept_bytes) == ([0], [8], [2], [b"@r1\nACGTACGT\n+\nIIIIIIII\n"]) and r.totals["quality_trimmed"] == 2
    r = trim_ref.trim_text(two, c(adapters=[b"AGATCGGAAG"], min_length=5))
    assert (r.begin, r.end, r.adapter, r.verdict, r.steps) == ([0, 0], [10, 4], [-1, 0], [0, 1], [0, 4])
    assert r.kept_bytes == [rec] and r.short_bytes == [b"@r2\nTTTT\n+\nIIII\n"]
    assert r.totals == dict(seen=2, kept=1, too_short=1, dropped=0, bytes_in=len(two), bases_in=21, bases_out=10, quality_trimmed=0, adapter_trimmed=7,
                            drop_short=0, adapter_records=[1])
    # dropped records are cut and counted like the others; a mask that is too short drops the rest and says so
    r = trim_ref.trim_text(two, c(adapters=[b"AGATCGGAAG"]), drop=[0, 1])
    assert r.verdict == [0, 2] and r.end == [10, 4] and r.totals["adapter_records"] == [1] and r.totals["dropped"] == 1 and r.kept_bytes == [rec]
    r = trim_ref.trim_text(two, c(), drop=[0])
    assert r.verdict == [0, 2] and r.totals["drop_short"] == 1
    # a read cut to nothing is written with two empty lines
    r = trim_ref.trim_text(b"@r\nAGATCGG\n+\nIIIIIII\n", c(adapters=[b"AGATCGGAAG"]))
    assert (r.begin, r.end, r.kept_bytes) == ([0], [0], [b"@r\n\n+\n\n"])
    r = trim_ref.trim_text(b"@r\nACGT\n+\n####\n", c(quality=(20, 20)))
    assert (r.begin, r.end, r.kept_bytes) == ([4], [4], [b"@r\n\n+\n\n"])
    # a short last record is judged on the lines it has; a line it lacks is empty and is not written
    r = trim_ref.trim_text(rec + b"@s\n", c(cut=(1, 0)))
    assert (r.begin, r.end, r.kept_bytes[1]) == ([1, 0], [10, 0], b"@s\n")
    with pytest.raises(trim_ref.Fault) as e:
        trim_ref.trim_text(rec + b"@s\nACGT\n", c())                  # the qualities it lacks are an empty body: 4 and 0 bytes
    assert (e.value.kind, e.value.record, e.value.lengths) == (3, 1, (4, 0))
    assert trim_ref.trim_text(rec + b"@s\nACGT\n", c(qual_line=None, cut=(0, 1))).kept_bytes[1] == b"@s\nACG\n"
    # a last line without its delimiter gets none; a CR is a body byte
    r = trim_ref.trim_text(b"@r\nACGT\n+\nIII#", c(quality=(0, 20)))
    assert r.kept_bytes == [b"@r\nACG\n+\nIII"]
    r = trim_ref.trim_text(b"@r\r\nACG\r\n+\r\nIII\r\n", c(cut=(0, 1)))
    assert r.kept_bytes == [b"@r\r\nACG\n+\r\nIII\n"]
    # the faults: the smaller record, a record with both for its first byte
    bad = b"@a\nAC\n+\nII\nxb\nAC\n+\nI\n@c\nA\n+\nII\n"
    for fb, want in ((b"@", (1, 1)), (None, (3, 1))):
        with pytest.raises(trim_ref.Fault) as e:
            trim_ref.trim_text(bad, c(first_byte=fb))
        assert (e.value.kind, e.value.record) == want
    # other record shapes
    r = trim_ref.trim_text(b">a;ACGTAC;>b;AC;", c(record_lines=2, seq_line=1, qual_line=None, cut=(0, 2), delimiter=b";"))
    assert r.kept_bytes == [b">a;ACGT;", b">b;;"]
    recs, starts, used = trim_ref.split_records(b"a\nb\nc\nd\ne", 2, final=False)
    assert (len(recs), starts, used) == (2, [0, 4], 8) and trim_ref.split_records(b"a\nb\nc\nd", 2, final=False)[2] == 4
    assert trim_ref.split_records(b"a\nb\nc", 2)[0] == [[(b"a", True), (b"b", True)], [(b"c", False)]]


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    monkeypatch.setattr(bgzf, "BgzfWriter", lambda *a, **kw: pytest.fail("an output was opened before the arguments were judged"))
    f = _Unreadable()
    with pytest.raises(ValueError, match="quality needs a qual_line"):
        bgzf.trim_records(f, "out", qual_line=None, quality=(0, 20))
    for kw in (dict(seq_line=4), dict(seq_line=-1), dict(qual_line=4), dict(qual_line=1), dict(seq_line=3), dict(cut=(-1, 0)), dict(cut=(0, 1 << 32)),
               dict(cut=(1, 2, 3)), dict(cut="12"), dict(quality=(0, 94)), dict(quality=(-1, 0)), dict(quality=(0.5, 0)), dict(quality_base=256),
               dict(quality_base=-1), dict(adapters=[b""]), dict(adapters=[b"A" * 256]), dict(adapters=[b"AC\nGT"]), dict(adapters=[b"A"] * 65),
               dict(adapters=[b"ACGT"], mismatches=4), dict(mismatches=17), dict(mismatches=-1), dict(mismatches=True), dict(min_overlap=0),
               dict(min_overlap=256), dict(min_length=-1), dict(min_length=1 << 32), dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(block_size=0),
               dict(record_lines=0), dict(record_lines=65), dict(drop=[[0, 1]]), dict(drop=[0.5, 1.0]), dict(drop="01")):
        with pytest.raises(ValueError):
            bgzf.trim_records(f, "out", **kw)
    for kw in (dict(match_line=1), dict(invert=True), dict(patterns=[b"A"]), dict(line_start=True)):
        with pytest.raises(TypeError):
            bgzf.trim_records(f, "out", **kw)
    with pytest.raises(ValueError):
        bgzf.trim_records("/nonexistent/reads.fq.gz", None, record_lines=0)                 # (judged before the file is read)
    cf, pats, d = bgzf._trim_conf(4, 1, 3, (1, 2), 20, 33, ADAPTERS[0], np.int64(2), 3, 20, b"@", b"\n")
    assert (cf.record_lines, cf.seq_line, cf.qual_line, cf.first_byte, cf.cut_front, cf.cut_back, cf.qual_front, cf.qual_back) == (4, 1, 3, 64, 1, 2, 0, 20)
    assert (cf.quality_base, cf.max_mismatch, cf.min_overlap, cf.min_length, cf.flags, list(cf.reserved), pats, d) == (33, 2, 3, 20, 0, [0, 0, 0], ADAPTERS[:1], b"\n")
    assert bgzf._trim_conf(2, 1, None, (0, 0), (0, 0), 33, (), 0, 3, 0, None, b";")[0].qual_line == -1
    for name in ("trim_records", "TrimResult"):
        assert name in bgzf.__all__
    assert hasattr(bgzf.BgzfReader, "trim_records") and (bgzf.KEPT, bgzf.TOO_SHORT, bgzf.DROPPED) == (0, 1, 2)
    import inspect
    want = ["file", "output", "record_lines", "seq_line", "qual_line", "cut", "quality", "quality_base", "adapters", "mismatches", "min_overlap", "min_length",
            "too_short", "drop", "first_byte", "delimiter", "compresslevel", "block_size", "start", "stop", "first_record", "max_record", "allow_short"]
    assert list(inspect.signature(bgzf.trim_records).parameters) == want
    assert list(inspect.signature(bgzf.BgzfReader.trim_records).parameters) == ["self"] + want[1:]


def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, header).group(1)
    return [re.sub(r"\[.*", "", x) for x in re.findall(r"\b(\w+(?:\[\w+\])?);", re.sub(r"/\*.*?\*/", "", body))]


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32, "zngamd_alloc_fn": _lib.ALLOC_FN}
    for name in ("zngamd_bgzf_trim_records_dev", "zngamd_bgzf_trim_records"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        params = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(",")]
        want = []
        for p in params:
            t = p.rsplit(" ", 1)[0] if "*" not in p else None
            want.append(C.c_void_p if t is None else ctype[t])
        assert getattr(L, name).argtypes == want, name
        assert "const zngamd_bgzf_trim_conf *conf" in params and params[-1] == "zngamd_bgzf_trim_totals *totals"
        assert params[1:13] == [re.sub(r"\s+", " ", x).strip() for x in
                                re.search(r"\bint %s\s*\(([^;]*)\);" % name.replace("trim", "grep"), header).group(1).split(",")][1:13]
    dev = re.search(r"\bint zngamd_bgzf_trim_records_dev\s*\(([^;]*)\);", header).group(1)
    for a, b in (("d_drop", "n_drop"), ("n_drop", "d_trim"), ("d_trim", "trim_cap"), ("trim_cap", "d_rows"), ("out_cap", "totals")):
        assert dev.index(a) < dev.index(b)
    for struct, ct, size in (("zngamd_bgzf_trim_conf", _lib.BgzfTrimConf, 64), ("zngamd_bgzf_trim_totals", _lib.BgzfTrimTotals, 13 * 8 + 4 * 4 + 64 * 8)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert int(re.search(r"\}\s*zngamd_bgzf_trim_row;\s*/\* (\d+) B \*/", header).group(1)) == _lib.TRIM_ROW_DTYPE.itemsize == 12
    assert _struct_fields(header, "zngamd_bgzf_trim_row") == list(_lib.TRIM_ROW_DTYPE.names)
    assert _lib.BgzfTrimTotals.covered.offset == 104 and _lib.BgzfTrimTotals.adapter_records.offset == 120
    for macro, value in (("KEPT", _lib.BGZF_TRIM_KEPT), ("TOO_SHORT", _lib.BGZF_TRIM_TOO_SHORT), ("DROPPED", _lib.BGZF_TRIM_DROPPED),
                         ("KEEP_SHORT", _lib.BGZF_TRIM_KEEP_SHORT), ("NO_ADAPTER", _lib.BGZF_TRIM_NO_ADAPTER), ("MAX_QUALITY", _lib.BGZF_TRIM_MAX_QUALITY)):
        assert int(re.search(r"#define ZNGAMD_BGZF_TRIM_%s\s+(\d+)u" % macro, header).group(1)) == value
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_trim.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_trim.hip"))
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_partition.hip"') < main.index('#include "za_trim.hip"')


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every hostile configuration, adapter list, mask, delimiter and flag -- and with everything in order"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    blob, table = _lib.grep_pattern_table(ADAPTERS)

    def call(form, conf=None, adapters=(blob, table), n_patterns=None, delim=10, flags=F, drop=(None, 0), totals=True, with_conf=True, **fields):
        cf = _lib.BgzfTrimConf(4, 1, 3, 64, 0, 0, 0, 20, 33, 2, 3, 20, 0)
        for k, v in fields.items():
            if k == "reserved":
                cf.reserved[v] = 1
            else:
                setattr(cf, k, v)
        t = _lib.BgzfTrimTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        b, tab = adapters
        tab = np.ascontiguousarray(tab, np.uint32)
        bp = C.c_char_p(b) if b is not None else None
        tp = C.c_void_p(tab.ctypes.data) if tab is not None and len(tab) else None
        head = (None, None, 0, None, 0, 0, 0, bp, len(b or b""), tp, len(tab) if n_patterns is None else n_patterns, delim, flags,
                C.byref(cf) if with_conf else None, 0)
        mask = (C.c_uint8 * max(1, len(drop[0])))(*drop[0]) if drop[0] is not None else None
        tail = (C.byref(t) if totals else None,)
        if form == 0:
            r = L.zngamd_bgzf_trim_records(*head, None, mask, drop[1], None, 0, None, 0, None, 0, _lib.ALLOC_FN(), None, *tail)
        else:
            r = L.zngamd_bgzf_trim_records_dev(*head, None, 0, None, mask, drop[1], None, 0, None, 0, None, 0, *tail)
        assert bytes(t) == b"\x5A" * C.sizeof(t)                                   # a refused call writes nothing
        return r

    none = (None, np.empty((0, 2), np.uint32))
    for form in range(2):
        for fields in (dict(record_lines=0), dict(record_lines=65), dict(record_lines=1 << 31), dict(seq_line=-1), dict(seq_line=4), dict(qual_line=-2),
                       dict(qual_line=4), dict(qual_line=1), dict(first_byte=-2), dict(first_byte=256), dict(qual_front=94), dict(qual_back=0xFFFFFFFF),
                       dict(qual_line=-1), dict(quality_base=256), dict(max_mismatch=17), dict(max_mismatch=12), dict(min_overlap=0), dict(min_overlap=256),
                       dict(flags=2), dict(flags=1 << 31), dict(reserved=0), dict(reserved=1), dict(reserved=2)):
            assert call(form, **fields) == E_ARG, (form, fields)
        assert call(form, with_conf=False) == E_ARG and call(form, totals=False) == E_ARG
        # adapters that break the limits of grep_patterns_ok
        assert call(form, adapters=_lib.grep_pattern_table([b"A"] * 65), max_mismatch=0) == E_ARG
        assert call(form, adapters=(b"A" * 256, [[0, 256]])) == E_ARG and call(form, adapters=(b"ACGT", [[0, 0]])) == E_ARG
        assert call(form, adapters=(b"ACGTACGT", [[4, 8]])) == E_ARG and call(form, adapters=(b"ACGTACGT", [[0xFFFFFFFF, 4]])) == E_ARG
        assert call(form, adapters=(b"ACGT\nACGT", [[0, 9]])) == E_ARG and call(form, adapters=(b"ACGT;ACGT", [[0, 9]]), delim=59) == E_ARG
        assert call(form, adapters=(None, table)) == E_ARG and call(form, adapters=(blob, table[:0]), n_patterns=3) == E_ARG
        assert call(form, drop=(None, 4)) == E_ARG and call(form, drop=(None, 1 << 63)) == E_ARG
        assert call(form, delim=-1) == E_ARG and call(form, delim=256) == E_ARG
        for flags in (_lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_LINE_START, _lib.BGZF_GREP_COUNT_ONLY, F | _lib.BGZF_GREP_LINE_START, G | 32, 64, 1 << 31):
            assert call(form, flags=flags) == E_ARG, (form, flags)
        for flags in (0, F, G, F | G):                                         # (in order but for the context)
            assert call(form, flags=flags) == E_ARG and call(form, flags=flags, drop=([0, 1, 0], 3)) == E_ARG
            assert call(form, flags=flags, adapters=none, qual_line=-1, qual_back=0, max_mismatch=16) == E_ARG


class _FakeTrimCtx:
    """ctx.bgzf_trim_records computed on the host: the blocks through the system zlib, the rule by trim_ref"""

    def __init__(self):
        self.calls = []

    def bgzf_trim_records(self, data, members, text_off, text_end, blob, table, delim, flags, conf, record_base=0, drop=None, caps=None):
        from zlib_ng_amd import _lib
        assert not flags & ~(_lib.BGZF_GREP_FINAL | _lib.BGZF_CLASSIFY_GROUP) and (drop is None or drop.dtype == np.uint8)
        data = bytes(data)
        buf = bytearray(int((members["out_off"] + members["out_len"]).max()) if len(members) else 0)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        text, d = bytes(buf[text_off:text_end]), bytes([delim])
        final = bool(flags & _lib.BGZF_GREP_FINAL)
        k = conf.record_lines
        recs, starts, used = trim_ref.split_records(text, k, d, final)
        nrec = len(recs)
        self.calls.append((record_base, None if drop is None else len(drop), nrec, flags, conf.flags, None if drop is None else drop.copy()))
        cf = trim_ref.conf(k, conf.seq_line, None if conf.qual_line < 0 else conf.qual_line, (conf.cut_front, conf.cut_back), (conf.qual_front, conf.qual_back),
                           conf.quality_base, [blob[o:o + n] for o, n in np.asarray(table).reshape(-1, 2).tolist()], conf.max_mismatch, conf.min_overlap,
                           conf.min_length, None if conf.first_byte < 0 else bytes([conf.first_byte]), d)
        tot = types.SimpleNamespace(seen=nrec, matched=nrec, covered=1, bad=0, bad_record=0, bad_src=0, drop_short=0, bytes=0, kept=0, too_short=0, dropped=0,
                                    tail_off=text_off + used, short_lines=len(recs[-1]) % k if final and recs else 0,
                                    adapter_records=(C.c_uint64 * 64)())
        st, none = np.zeros(len(members), np.int32), (np.empty(0, _lib.TRIM_ROW_DTYPE), np.empty(0, _lib.GREP_ROW_DTYPE), b"")
        if not nrec:
            return (0, st, tot) + none
        try:
            res = trim_ref.trim_text(text[:used], cf, None if drop is None else drop.tolist(), True)
        except trim_ref.Fault as e:
            tot.bad, tot.bad_record, tot.bad_src = e.kind, record_base + e.record, text_off + starts[e.record]
            return (0, st, tot) + none
        for name, v in res.totals.items():
            if name != "adapter_records":
                setattr(tot, name, v)
        for j, v in enumerate(res.totals["adapter_records"]):
            tot.adapter_records[j] = v
        keep_short = bool(conf.flags & _lib.BGZF_TRIM_KEEP_SHORT)
        tot.bytes = sum(map(len, res.kept_bytes)) + (sum(map(len, res.short_bytes)) if keep_short else 0)
        if tot.drop_short:
            return (0, st, tot) + none
        trim = np.zeros(nrec, _lib.TRIM_ROW_DTYPE)
        trim["begin"], trim["end"], trim["verdict"], trim["steps"] = res.begin, res.end, res.verdict, res.steps
        trim["adapter"] = [255 if j < 0 else j for j in res.adapter]
        if not flags & _lib.BGZF_CLASSIFY_GROUP:
            return 0, st, tot, trim, none[1], b""
        v = np.array(res.verdict)
        order = np.concatenate([np.nonzero(v == 0)[0], np.nonzero(v == 1)[0] if keep_short else np.empty(0, np.int64)]).astype(np.int64)
        pieces = res.kept_bytes + (res.short_bytes if keep_short else [])
        rows = np.zeros(len(order), _lib.GREP_ROW_DTYPE)
        rows["src_off"], rows["number"], rows["len"], rows["reserved"] = np.array(starts, np.int64)[order] + text_off, record_base + order, [len(x) for x in pieces], v[order]
        return 0, st, tot, trim, rows, b"".join(pieces)


def _reads(n, seed=5):
    """FASTQ reads of 0 .. 159 bases, two thirds with an adapter planted and cut off at the read's end, a low-quality tail of 0 .. 11"""
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.choice([0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 150]) if i % 7 == 0 else rng.randrange(0, 160)
        s = bytes(rng.choice(b"ACGT") for _ in range(L))
        if i % 3 and L:
            A = bytearray(ADAPTERS[i % 3 - 1 if i % 5 else 2])
            for at in rng.sample(range(len(A)), rng.randrange(0, 3)):
                A[at] = rng.choice([c for c in b"ACGT" if c != A[at]])
            s = (s[:rng.randrange(0, L + 1)] + bytes(A) + s)[:L]
        q = bytearray(rng.choice(b"FFFFF:,#") for _ in range(L))
        for x in range(max(0, L - rng.randrange(0, 12)), L):
            q[x] = rng.choice(b"#,")
        out.append(b"@r%d\n%s\n+\n%s\n" % (i, s, bytes(q)))
    return out


def _same(result, want, n_adapters=3):
    assert result.records == len(want.begin) == len(result)
    assert result.begin.tolist() == want.begin and result.end.tolist() == want.end and result.adapter.tolist() == want.adapter
    assert result.verdict.tolist() == want.verdict and result.steps.tolist() == want.steps
    assert (result.begin.dtype, result.adapter.dtype, result.verdict.dtype, result.adapter_counts.dtype) == (np.int64, np.int16, np.uint8, np.int64)
    for name in ("kept", "too_short", "dropped", "bases_in", "bases_out", "quality_trimmed", "adapter_trimmed"):
        assert getattr(result, name) == want.totals[name], name
    assert result.adapter_counts.tolist() == want.totals["adapter_records"][:n_adapters]


def test_driver_on_a_fake_engine(monkeypatch):
    from zlib_ng_amd import _lib, bgzf
    recs = _reads(700)
    data = b"".join(recs)
    BS = 997
    blob, blocks = _stored_bgzf(data, BS)
    coffs = sorted(blocks)
    fake = _FakeTrimCtx()
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)
    monkeypatch.setattr(bgzf, "BgzfWriter", _Collect)
    kw = dict(quality=(20, 20), adapters=ADAPTERS, mismatches=2, min_length=20)
    cf = trim_ref.conf(first_byte=b"@", **kw)
    want = trim_ref.trim_text(data, cf)
    assert want.totals["kept"] > 100 and want.totals["too_short"] > 100 and min(want.totals["adapter_records"]) > 50 and want.totals["quality_trimmed"] > 500
    drop = np.arange(len(recs)) % 3 == 0
    wantd = trim_ref.trim_text(data, cf, drop.tolist())
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    voff = lambda r: bgzf.make_virtual_offset(coffs[starts[r] // BS], int(starts[r] % BS))

    def trim(src, output, too_short=None, drop=None, **more):
        args = dict(first_byte=b"@", start=None, stop=None, first_record=0, allow_short=False, qual_line=3)
        args.update(kw)
        args.update(more)
        _Collect.made.clear()
        fake.calls.clear()
        return bgzf._trim_file(io.BytesIO(src), fake, output, too_short, 4, 1, args["qual_line"], (0, 0), args["quality"], 33, args["adapters"], args["mismatches"], 3,
                               args["min_length"], drop, args["first_byte"], b"\n", 1, bgzf.MAX_BLOCK_INPUT, args["start"], args["stop"], args["first_record"],
                               64 << 20, args["allow_short"])

    for window in (32 << 20, 5000, 1500):
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        # the kept records to an output, the too-short ones counted only
        r = trim(blob, "kept")
        _same(r, want)
        (w,) = _Collect.made
        assert w.closed and w.level == 1 and w.got == b"".join(want.kept_bytes)
        assert all(c[3] & _lib.BGZF_CLASSIFY_GROUP and not c[4] and c[1] is None for c in fake.calls) and fake.calls[-1][3] & _lib.BGZF_GREP_FINAL
        assert len(fake.calls) == 1 if window == 32 << 20 else len(fake.calls) > 10
        assert sum(c[2] for c in fake.calls) == len(recs)
        # a too_short output; output=None with it
        r = trim(blob, "kept", "short")
        _same(r, want)
        made = {w.target: w for w in _Collect.made}
        assert made["kept"].got == b"".join(want.kept_bytes) and made["short"].got == b"".join(want.short_bytes) and all(w.closed for w in made.values())
        assert all(c[4] == _lib.BGZF_TRIM_KEEP_SHORT for c in fake.calls)
        r = trim(blob, None, "short")
        (w,) = _Collect.made
        assert w.target == "short" and w.got == b"".join(want.short_bytes)
        # output=None: nothing is gathered
        r = trim(blob, None)
        _same(r, want)
        assert not _Collect.made and not any(c[3] & _lib.BGZF_CLASSIFY_GROUP for c in fake.calls)
        # the drop mask advances with the records: every call is handed the mask from its first record on
        r = trim(blob, "kept", "short", drop)
        _same(r, wantd)
        made = {w.target: w for w in _Collect.made}
        assert made["kept"].got == b"".join(wantd.kept_bytes) and made["short"].got == b"".join(wantd.short_bytes)
        at = 0
        for base, n_drop, nrec, flags, cflags, given in fake.calls:
            assert (base, n_drop) == (at, len(drop) - at) and np.array_equal(given, drop[at:].astype(np.uint8))
            at += nrec
        assert at == len(recs)
        # start / stop / first_record: the mask belongs to the records from first_record on
        a, b = 123, 500
        r = trim(blob, "kept", None, drop[a:b], start=voff(a), stop=voff(b), first_record=a)
        mid = trim_ref.trim_text(b"".join(recs[a:b]), cf, drop[a:b].tolist())
        _same(r, mid)
        assert _Collect.made[0].got == b"".join(mid.kept_bytes) and fake.calls[0][0] == a
        # out of step, both ways, across windows: the message names both counts, the outputs are closed
        for n_drop in (len(recs) - 1, len(recs) - 300, len(recs) + 1, len(recs) + 300, 0):
            with pytest.raises(ValueError, match=r"the file holds 700 records and drop has %d entries: the files are out of step.*incomplete" % n_drop):
                trim(blob, "kept", "short", np.resize(drop, n_drop))
            assert len(_Collect.made) == 2 and all(w.closed for w in _Collect.made)
            with pytest.raises(ValueError, match=r"holds 700 records and drop has %d entries" % n_drop):
                trim(blob, None, None, np.resize(drop, n_drop))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1500)
    # a short last record
    cut = data[:data.rfind(b"\n", 0, len(data) - 1) + 1]                     # the last read without its quality line
    sblob, _ = _stored_bgzf(cut, BS)
    with pytest.raises(ValueError, match=r"record 699, the last one, has 3 of 4 lines"):
        trim(sblob, None, qual_line=None, quality=(0, 0))
    r = trim(sblob, None, qual_line=None, quality=(0, 0), allow_short=True)
    _same(r, trim_ref.trim_text(cut, trim_ref.conf(qual_line=None, adapters=ADAPTERS, mismatches=2, min_length=20)))
    # a length fault mid-file: the record, its virtual offset and both lengths; the outputs are closed and incomplete
    lines = data.split(b"\n")
    n_seq = len(lines[4 * 600 + 1])
    lines[4 * 600 + 3] += b"F"
    fblob, fblocks = _stored_bgzf(b"\n".join(lines), BS)
    at = len(b"\n".join(lines[:4 * 600])) + 1
    v = bgzf.make_virtual_offset(sorted(fblocks)[at // BS], at % BS)
    with pytest.raises(ValueError, match=r"record 600 at virtual offset %d: line 1 \(the sequence\) has %d bytes and line 3 \(the qualities\) has %d.*trim_records.*incomplete"
                       % (v, n_seq, n_seq + 1)):
        trim(fblob, "kept", "short")
    assert len(_Collect.made) == 2 and all(w.closed for w in _Collect.made) and 0 < len(_Collect.made[0].got) < len(b"".join(want.kept_bytes))
    # a first_byte violation on the way
    lines = data.split(b"\n")
    lines[4 * 601] = b"x" + lines[4 * 601][1:]
    bblob, _ = _stored_bgzf(b"\n".join(lines), BS)
    with pytest.raises(ValueError, match=r"record 601 at virtual offset \d+ does not start with b'@'.*trim_records.*incomplete"):
        trim(bblob, "kept")
    assert len(_Collect.made) == 1 and _Collect.made[0].closed and 0 < len(_Collect.made[0].got) < len(b"".join(want.kept_bytes))


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
    exe = str(tmp_path / "trim_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "trim_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf trim arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

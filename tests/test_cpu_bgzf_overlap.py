"""CPU: BGZF overlap, without a GPU -- the referee of overlap_ref.py on the literal cases of the rule; the argument checks of
bgzf.overlap_records that need no context; the two zngamd_bgzf_overlap_records entry points are declared, exported and bound, and refuse
hostile arguments with no context at all; the window loop on a stand-in engine whose rule is the referee (stored-block BGZF written
here, the system zlib decodes it); and tests/overlap_args.cpp, a stand-alone program, against the library's host side under
AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process, nothing preloaded)."""
import ctypes as C
import inspect
import io
import os
import random
import re
import subprocess
import types
import zlib

import numpy as np
import pytest

import overlap_ref
from conftest import PKG_DIR, ROOT
from overlap_ref import conf, find, revcomp as rc
from test_cpu_bgzf_classify import _Collect
from test_cpu_bgzf_grep import _stored_bgzf
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang
from test_cpu_bgzf_trim import _FakeTrimCtx, _struct_fields
from test_gpu_bgzf_overlap import gen_pairs, interleaved

_rng = random.Random(7)
F = bytes(_rng.choice(b"ACGT") for _ in range(200))      # a fragment in which nothing matches by chance


def _sub(s, places):
    s = bytearray(s)
    for i in places:
        s[i] = {65: 67, 67: 71, 71: 84, 84: 65}[s[i]]
    return bytes(s)


def test_referee_search_literals():
    assert find(b"A" * 50, b"T" * 50, conf()) == (0, 50, 0)
    assert find(b"A" * 40, b"T" * 60, conf()) == (0, 40, 0) and find(b"A" * 60, b"T" * 40, conf()) == (0, 40, 0)      # equal L and d: the smaller |o|
    assert find(b"AC" * 30, rc(b"AC" * 30), conf()) == (0, 60, 0)                                                  # a dinucleotide repeat: the longest
    assert find(b"AC" * 30, rc(b"CA" * 30), conf()) == (1, 59, 0)                                                  # equal L, d and |o|: o >= 0 first
    assert find(b"AC" * 30, rc(b"G" + b"A" + b"CA" * 29), conf()) == (-1, 59, 0)                                   # equal L: the smaller d
    assert find(b"AC" * 30, rc(b"G" + b"A" + b"CA" * 29), conf(mismatches=0)) == (-1, 59, 0)
    # d exactly at and one over each of the two limits
    a, y = F[:100], rc(F[50:150])
    assert find(_sub(a, range(50, 55)), y, conf()) == (50, 50, 5) and find(_sub(a, range(50, 56)), y, conf()) is None
    a, y = F[:100], rc(F[70:150])
    assert find(_sub(a, (70, 80, 99)), y, conf(percent=10)) == (70, 30, 3) and find(_sub(a, (70, 80, 90, 99)), y, conf(percent=10)) is None
    assert find(_sub(a, (70, 80, 90, 99)), y, conf(percent=14)) == (70, 30, 4) and find(a, y, conf(percent=0)) == (70, 30, 0)
    assert find(_sub(a, (75,)), y, conf(percent=0)) is None and find(_sub(a, (75,)), y, conf(mismatches=0, percent=100)) is None
    # min_overlap at L and at L + 1
    a, y = F[:100], rc(F[65:150])
    assert find(a, y, conf(min_overlap=35)) == (65, 35, 0) and find(a, y, conf(min_overlap=36)) is None
    # o < 0; mate 2 contained in mate 1; an empty mate; a mate above the limit
    assert find(F[30:100], rc(F[:90]), conf()) == (-30, 60, 0) and find(F[:100], rc(F[20:60]), conf()) == (20, 40, 0)
    assert find(b"", F[:50], conf(min_overlap=1)) is None and find(F[:50], b"", conf(min_overlap=1)) is None and find(b"", b"", conf(min_overlap=1)) is None
    assert find(F * 6, rc(F * 6), conf()) is None and find((F * 6)[:1024], rc((F * 6)[:1024]), conf())[:2] == (0, 1024)
    # bytes are compared as they are: N equals N, lowercase complements in lowercase; U -> A, and A -> T is not U
    a = F[:20] + b"NnacgtRY" + F[28:60]
    assert rc(b"NnacgtRYUu") == b"aAYRacgtnN" and find(a, rc(a), conf()) == (0, 60, 0)
    u = F[:20] + b"U" + F[21:60]
    assert find(u, rc(u), conf()) == (0, 60, 1) and find(u, rc(u), conf(mismatches=0)) is None


def _pair(a, qa, y, qy):
    return [(b"@p/1", True), (a, True), (b"+", True), (qa, True), (b"@p/2", True), (y, True), (b"+", True), (qy, True)]


def test_referee_on_whole_pairs():
    rec = overlap_ref.overlap_record
    # o < 0 with both mates cut: the adapters fall off, the qualities with them
    a, y = F[30:90] + b"GGGGGGGG", rc(F[30:90]) + b"CCCCC"
    p = rec(_pair(a, b"F" * 68, y, b":" * 65), conf(merge=False, cut=True))
    assert (p.offset, p.insert, p.overlap, p.steps, p.trimmed, p.verdict, p.cls) == (-5, 60, 60, 3, 13, 1, 1)
    assert p.out == b"@p/1\n%s\n+\n%s\n@p/2\n%s\n+\n%s\n" % (F[30:90], b"F" * 60, rc(F[30:90]), b":" * 60)
    p = rec(_pair(a, b"F" * 68, y, b":" * 65), conf(cut=True))
    assert (p.verdict, p.cls, p.steps, p.out) == (2, 0, 3, b"@p/1\n%s\n+\n%s\n" % (F[30:90], b"F" * 60))
    # mate 2 contained in mate 1: mate 1 is cut at the insert, mate 2 is whole
    p = rec(_pair(F[:100], b"F" * 100, rc(F[20:60]), b"F" * 40), conf(merge=False, cut=True))
    assert (p.offset, p.insert, p.steps, p.trimmed) == (20, 60, 1, 40) and p.out.split(b"\n")[1] == F[:60]
    # correction in both directions and neither: I is 40, 5 is 20, # is 2
    a = _sub(F[:100], (60, 70, 80))
    qa = bytearray(b"I" * 100)
    qa[70], qa[80] = ord("#"), ord("5")
    qy = bytearray(b"I" * 100)
    qy[99 - (60 - 50)] = ord("#")
    cf = conf(merge=False, correct=True)
    p = rec(_pair(a, bytes(qa), rc(F[50:150]), bytes(qy)), cf)
    lines = p.out.split(b"\n")
    assert (p.offset, p.mismatches, p.corrected, p.steps) == (50, 3, 2, 4)
    assert lines[1] == _sub(F[:100], (60, 80)) and lines[3] == bytes(qa[:70]) + b"I" + bytes(qa[71:])           # mate 1 took b's byte and quality at 70
    assert rc(lines[5]) == _sub(F[50:150], (10,)) and lines[7][::-1] == b"I" * 100                                 # mate 2 took mate 1's at 60
    assert rec(_pair(a, bytes(qa), rc(F[50:150]), bytes(qy)), conf(merge=False)).out == b"\n".join([b"@p/1", a, b"+", bytes(qa), b"@p/2", rc(F[50:150]), b"+", bytes(qy), b""])
    # the merged read is taken from the source text: the higher quality wins, mate 1 on ties; correction only counts
    for cf in (conf(), conf(correct=True)):
        p = rec(_pair(a, bytes(qa), rc(F[50:150]), bytes(qy)), cf)
        lines = p.out.split(b"\n")
        assert (p.verdict, p.insert, p.corrected) == (2, 150, 2 if cf.correct else 0) and len(lines) == 5
        assert lines[1] == _sub(F[:150], (60,)) and lines[3] == b"I" * 150                                        # 60: Qa > Qb; 70 and 80: Qb > Qa
    qa[80] = qy[99 - 30] = ord("I")
    assert rec(_pair(a, bytes(qa), rc(F[50:150]), bytes(qy)), conf()).out.split(b"\n")[1] == _sub(F[:150], (60, 80))      # a tie on quality: mate 1
    # no qualities: every tie is mate 1's
    p = rec([(b">p/1", True), (a, True), (b">p/2", True), (rc(F[50:150]), True)], conf(record_lines=4, qual_line=None))
    assert p.out == b">p/1\n%s\n" % (a + F[100:150])
    # whole texts: the classes, the faults
    t = overlap_ref.overlap_text
    pair = b"@p/1\n%s\n+\n%s\n@p/2\n%s\n+\n%s\n" % (F[:80], b"F" * 80, rc(F[20:120]), b"F" * 100)
    lone = b"@q/1\nACGT\n+\nFFFF\n@q/2\nACGT\n+\nFFFF\n"
    r = t(pair + lone, conf(first_byte=b"@"))
    assert (r.verdict, r.offset, r.insert, r.merged_bytes, r.other_bytes) == ([2, 0], [20, 0], [120, 0], [b"@p/1\n%s\n+\n%s\n" % (F[:120], b"F" * 120)], [lone])
    assert r.totals == dict(seen=2, none=1, found=0, merged=1, too_long=0, bytes_in=len(pair + lone), bases_in=188, bases_merged=120, corrected=0, corrected_pairs=0,
                            adapter_pairs=0, adapter_trimmed=0, overlap_sum=60, mismatch_sum=0)
    r = t(pair + lone, conf(merge=False))
    assert r.verdict == [1, 0] and r.merged_bytes == [] and b"".join(r.other_bytes) == pair + lone
    bad = pair + lone.replace(b"@q/2", b"xq/2") + pair.replace(b"F" * 100, b"F" * 99)
    for fb, want in ((b"@", (1, 1)), (None, (3, 2))):
        with pytest.raises(overlap_ref.Fault) as e:
            t(bad, conf(first_byte=fb))
        assert (e.value.kind, e.value.record) == want
    with pytest.raises(overlap_ref.Fault) as e:
        t(pair + b"@s/1\nACGT\n+\nFFFF\n", conf(first_byte=b"@"))          # a short last pair has no line m
    assert (e.value.kind, e.value.record) == (1, 1)
    r = t(pair + b"@s/1\nACGT\n+\nFFFF\n@s/2\n", conf(first_byte=b"@"))
    assert r.verdict == [2, 0] and r.other_bytes == [b"@s/1\nACGT\n+\nFFFF\n@s/2\n"]


KW = dict(seq_line=1, qual_line=3, quality_base=33, min_overlap=30, mismatches=5, mismatch_percent=20, merge=True, correct=False, correct_quality=(30, 14),
          cut_adapters=False, first_byte=None, delimiter=b"\n")


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    monkeypatch.setattr(bgzf, "BgzfWriter", lambda *a, **kw: pytest.fail("an output was opened before the arguments were judged"))
    f = _Unreadable()
    with pytest.raises(ValueError, match="correct needs a qual_line"):
        bgzf.overlap_records(f, "out", qual_line=None, correct=True)
    with pytest.raises(ValueError, match="record_lines is even"):
        bgzf.overlap_records(f, "out", record_lines=7)
    for kw in (dict(record_lines=0), dict(record_lines=66), dict(record_lines=3), dict(seq_line=4), dict(seq_line=-1), dict(qual_line=4), dict(qual_line=7),
               dict(qual_line=1), dict(seq_line=3), dict(record_lines=4, qual_line=3), dict(quality_base=256), dict(quality_base=-1), dict(min_overlap=0),
               dict(min_overlap=1025), dict(min_overlap=30.0), dict(mismatches=-1), dict(mismatches=1025), dict(mismatches=True), dict(mismatch_percent=101),
               dict(mismatch_percent=-1), dict(mismatch_percent=0.2), dict(correct_quality=30), dict(correct_quality=(30,)), dict(correct_quality=(94, 14)),
               dict(correct_quality=(30, -1)), dict(merge=1), dict(correct="yes"), dict(cut_adapters=None), dict(first_byte=b"@@"), dict(delimiter=b"ab"),
               dict(block_size=0)):
        with pytest.raises(ValueError):
            bgzf.overlap_records(f, "out", **kw)
    for kw in (dict(match_line=1), dict(adapters=[b"A"]), dict(drop=[0]), dict(patterns=[b"A"])):
        with pytest.raises(TypeError):
            bgzf.overlap_records(f, "out", **kw)
    with pytest.raises(ValueError):
        bgzf.overlap_records("/nonexistent/pairs.fq.gz", None, None, record_lines=5)              # (judged before the file is read)
    cf, d = bgzf._overlap_conf(8, 1, 3, 33, np.int64(30), 5, 20, True, True, (30, 14), True, b"@", b"\n")
    assert (cf.record_lines, cf.seq_line, cf.qual_line, cf.first_byte, cf.quality_base, cf.min_overlap, cf.max_mismatch, cf.max_percent) == (8, 1, 3, 64, 33, 30, 5, 20)
    assert (cf.q_high, cf.q_low, cf.flags, list(cf.reserved), d) == (30, 14, _lib.BGZF_OVERLAP_MERGE | _lib.BGZF_OVERLAP_CORRECT | _lib.BGZF_OVERLAP_CUT, [0] * 5, b"\n")
    cf, d = bgzf._overlap_conf(4, 1, None, 33, 1024, 1024, 100, False, False, (0, 93), False, None, b";")
    assert (cf.qual_line, cf.first_byte, cf.flags, d) == (-1, -1, 0, b";")
    for name in ("overlap_records", "OverlapResult", "NONE", "FOUND", "MERGED", "TOO_LONG"):
        assert name in bgzf.__all__
    assert hasattr(bgzf.BgzfReader, "overlap_records") and (bgzf.NONE, bgzf.FOUND, bgzf.MERGED, bgzf.TOO_LONG) == (0, 1, 2, 3)
    want = ["file", "merged", "unmerged", "record_lines", "seq_line", "qual_line", "quality_base", "min_overlap", "mismatches", "mismatch_percent", "merge", "correct",
            "correct_quality", "cut_adapters", "first_byte", "delimiter", "compresslevel", "block_size", "start", "stop", "first_record", "max_record", "allow_short"]
    sig = inspect.signature(bgzf.overlap_records)
    assert list(sig.parameters) == want and list(inspect.signature(bgzf.BgzfReader.overlap_records).parameters) == ["self"] + want[1:]
    defaults = dict(merged=None, unmerged=None, record_lines=8, compresslevel=6, block_size=bgzf.MAX_BLOCK_INPUT, start=None, stop=None, first_record=0,
                    max_record=64 << 20, allow_short=False, **KW)
    for fn in (bgzf.overlap_records, bgzf.BgzfReader.overlap_records):
        ps = inspect.signature(fn).parameters
        assert {k: p.default for k, p in ps.items() if k not in ("file", "self")} == defaults
        assert [k for k, p in ps.items() if p.kind is p.KEYWORD_ONLY] == want[4:]
    # the positional signature of the window loop stays
    assert list(inspect.signature(bgzf._grep_file).parameters)[-4:] == ["records", "mismatches", "classify", "partition"]
    res = bgzf.OverlapResult(np.array([(5, 65, 55, 1, 0, 2, 0), (0, 0, 0, 0, 0, 0, 0), (-3, 65, 60, 0, 1, 1, 4)], _lib.OVERLAP_ROW_DTYPE),
                             dict.fromkeys(bgzf._OVERLAP_COUNTS, 0) | dict(found=1, merged=1, none=1, overlap_sum=115))
    assert len(res) == 3 and res.insert_sizes().tolist() == [1] + [0] * 64 + [2] and res.mean_overlap == 57.5 and "3 pairs, 1 merged" in repr(res)
    assert bgzf.OverlapResult(np.empty(0, _lib.OVERLAP_ROW_DTYPE), dict.fromkeys(bgzf._OVERLAP_COUNTS, 0)).mean_overlap == 0.0


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32, "zngamd_alloc_fn": _lib.ALLOC_FN}
    split = lambda name: [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(",")]
    for name in ("zngamd_bgzf_overlap_records_dev", "zngamd_bgzf_overlap_records"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        params = split(name)
        want = [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params]
        assert getattr(L, name).argtypes == want, name
        assert "const zngamd_bgzf_overlap_conf *conf" in params and params[-1] == "zngamd_bgzf_overlap_totals *totals"
        assert params[1:7] == split(name.replace("overlap", "trim"))[1:7]                 # the window, the members, the text range
        assert params[7:11] == ["int delim", "uint32_t flags", "const zngamd_bgzf_overlap_conf *conf", "uint64_t record_base"]
        assert not any("pattern" in p or "drop" in p for p in params)
    dev, host = (re.search(r"\bint %s\s*\(([^;]*)\);" % n, header).group(1) for n in ("zngamd_bgzf_overlap_records_dev", "zngamd_bgzf_overlap_records"))
    for a, b in (("record_base", "d_scratch"), ("d_status", "d_overlap"), ("d_overlap", "overlap_cap"), ("overlap_cap", "d_rows"), ("rows_cap", "d_out"), ("out_cap", "totals")):
        assert dev.index(a) < dev.index(b)
    for a, b in (("record_base", "status"), ("status", "*overlap"), ("overlap_cap", "*rows"), ("rows_cap", "*out"), ("out_cap", "alloc"), ("alloc", "user"), ("user", "totals")):
        assert host.index(a) < host.index(b)
    for struct, ct, size in (("zngamd_bgzf_overlap_conf", _lib.BgzfOverlapConf, 64), ("zngamd_bgzf_overlap_totals", _lib.BgzfOverlapTotals, 18 * 8 + 4 * 4)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert int(re.search(r"\}\s*zngamd_bgzf_overlap_row;\s*/\* (\d+) B \*/", header).group(1)) == _lib.OVERLAP_ROW_DTYPE.itemsize == 16
    assert _struct_fields(header, "zngamd_bgzf_overlap_row") == list(_lib.OVERLAP_ROW_DTYPE.names)
    assert [_lib.OVERLAP_ROW_DTYPE.fields[n][1] for n in _lib.OVERLAP_ROW_DTYPE.names] == [0, 4, 8, 10, 12, 14, 15]
    assert _lib.BgzfOverlapTotals.tail_off.offset == 120 and _lib.BgzfOverlapTotals.covered.offset == 144
    for macro, value in (("NONE", _lib.BGZF_OVERLAP_NONE), ("FOUND", _lib.BGZF_OVERLAP_FOUND), ("MERGED", _lib.BGZF_OVERLAP_MERGED), ("TOO_LONG", _lib.BGZF_OVERLAP_TOO_LONG),
                         ("MERGE", _lib.BGZF_OVERLAP_MERGE), ("CORRECT", _lib.BGZF_OVERLAP_CORRECT), ("CUT", _lib.BGZF_OVERLAP_CUT),
                         ("KEEP_UNMERGED", _lib.BGZF_OVERLAP_KEEP_UNMERGED), ("MAX_READ", _lib.BGZF_OVERLAP_MAX_READ), ("MAX_QUALITY", _lib.BGZF_OVERLAP_MAX_QUALITY)):
        assert int(re.search(r"#define ZNGAMD_BGZF_OVERLAP_%s\s+(\d+)u" % macro, header).group(1)) == value
    assert (_lib.BGZF_OVERLAP_MAX_READ, overlap_ref.MAX_READ) == (1024, 1024)
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_overlap.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_overlap.hip"))
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_trim.hip"') < main.index('#include "za_overlap.hip"')
    # the rule stands in the header as the referee states it
    for phrase in ("larger L", "then smaller d", "then smaller |o|", "then o >= 0 before o < 0", "Mate 1 wins on ties", "insert = o + n2"):
        assert phrase in header, phrase


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every hostile configuration, delimiter and flag -- and with everything in order"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    FIN, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP

    def call(form, delim=10, flags=FIN, totals=True, with_conf=True, **fields):
        cf = _lib.BgzfOverlapConf(8, 1, 3, 64, 33, 30, 5, 20, 30, 14, 7)
        for k, v in fields.items():
            if k == "reserved":
                cf.reserved[v] = 1
            else:
                setattr(cf, k, v)
        t = _lib.BgzfOverlapTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        head = (None, None, 0, None, 0, 0, 0, delim, flags, C.byref(cf) if with_conf else None, 0)
        tail = (C.byref(t) if totals else None,)
        if form == 0:
            r = L.zngamd_bgzf_overlap_records(*head, None, None, 0, None, 0, None, 0, _lib.ALLOC_FN(), None, *tail)
        else:
            r = L.zngamd_bgzf_overlap_records_dev(*head, None, 0, None, None, 0, None, 0, None, 0, *tail)
        assert bytes(t) == b"\x5A" * C.sizeof(t)                                   # a refused call writes nothing
        return r

    for form in range(2):
        for fields in (dict(record_lines=0), dict(record_lines=1), dict(record_lines=7), dict(record_lines=66), dict(record_lines=1 << 31), dict(seq_line=-1),
                       dict(seq_line=4), dict(qual_line=-2), dict(qual_line=4), dict(qual_line=7), dict(qual_line=1), dict(first_byte=-2), dict(first_byte=256),
                       dict(quality_base=256), dict(min_overlap=0), dict(min_overlap=1025), dict(max_mismatch=1025), dict(max_mismatch=0xFFFFFFFF),
                       dict(max_percent=101), dict(q_high=94), dict(q_low=94), dict(qual_line=-1), dict(flags=16), dict(flags=1 << 31), dict(reserved=0),
                       dict(reserved=2), dict(reserved=4)):
            assert call(form, **fields) == E_ARG, (form, fields)
        assert call(form, with_conf=False) == E_ARG and call(form, totals=False) == E_ARG
        assert call(form, delim=-1) == E_ARG and call(form, delim=256) == E_ARG
        for flags in (_lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_LINE_START, _lib.BGZF_GREP_COUNT_ONLY, FIN | _lib.BGZF_GREP_LINE_START, G | 32, 64, 1 << 31):
            assert call(form, flags=flags) == E_ARG, (form, flags)
        for flags in (0, FIN, G, FIN | G):                                     # (in order but for the context)
            assert call(form, flags=flags) == E_ARG
            assert call(form, flags=flags, record_lines=4, qual_line=-1, min_overlap=1024, max_mismatch=1024, max_percent=100) == E_ARG      # conf.flags 7 with q = -1
            assert call(form, flags=flags, record_lines=64, seq_line=31, qual_line=0, q_high=93, q_low=93) == E_ARG


class _FakeOverlapCtx(_FakeTrimCtx):
    """ctx.bgzf_overlap_records computed on the host: the blocks through the system zlib, the rule by overlap_ref (the lengths a length
    fault's message names come from the stand-in trim engine)"""

    def bgzf_overlap_records(self, data, members, text_off, text_end, delim, flags, conf, record_base=0, caps=None):
        from zlib_ng_amd import _lib
        assert not flags & ~(_lib.BGZF_GREP_FINAL | _lib.BGZF_CLASSIFY_GROUP)
        data = bytes(data)
        buf = bytearray(int((members["out_off"] + members["out_len"]).max()) if len(members) else 0)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        text, d = bytes(buf[text_off:text_end]), bytes([delim])
        final = bool(flags & _lib.BGZF_GREP_FINAL)
        k = conf.record_lines
        recs, starts, used = overlap_ref.split_records(text, k, d, final)
        nrec = len(recs)
        self.calls.append((record_base, nrec, flags, conf.flags))
        cf = overlap_ref.conf(k, conf.seq_line, None if conf.qual_line < 0 else conf.qual_line, conf.quality_base, conf.min_overlap, conf.max_mismatch,
                              conf.max_percent, bool(conf.flags & _lib.BGZF_OVERLAP_MERGE), bool(conf.flags & _lib.BGZF_OVERLAP_CORRECT),
                              (conf.q_high, conf.q_low), bool(conf.flags & _lib.BGZF_OVERLAP_CUT), None if conf.first_byte < 0 else bytes([conf.first_byte]), d)
        tot = types.SimpleNamespace(**dict.fromkeys(overlap_ref.overlap_text(b"", cf).totals, 0))
        tot.seen, tot.matched, tot.covered, tot.bad, tot.bad_record, tot.bad_src, tot.bytes, tot.tail_off = nrec, nrec, 1, 0, 0, 0, 0, text_off + used
        tot.short_lines = len(recs[-1]) % k if final and recs else 0
        st, none = np.zeros(len(members), np.int32), (np.empty(0, _lib.OVERLAP_ROW_DTYPE), np.empty(0, _lib.GREP_ROW_DTYPE), b"")
        if not nrec:
            return (0, st, tot) + none
        try:
            res = overlap_ref.overlap_text(text[:used], cf, True)
        except overlap_ref.Fault as e:
            tot.bad, tot.bad_record, tot.bad_src = e.kind, record_base + e.record, text_off + starts[e.record]
            return (0, st, tot) + none
        for name, v in res.totals.items():
            setattr(tot, name, v)
        keep = bool(conf.flags & _lib.BGZF_OVERLAP_KEEP_UNMERGED)
        tot.bytes = sum(map(len, res.merged_bytes)) + (sum(map(len, res.other_bytes)) if keep else 0)
        ovl = np.zeros(nrec, _lib.OVERLAP_ROW_DTYPE)
        for name in ovl.dtype.names:
            ovl[name] = getattr(res, name)
        if not flags & _lib.BGZF_CLASSIFY_GROUP:
            return 0, st, tot, ovl, none[1], b""
        v = np.array(res.verdict)
        order = np.concatenate([np.nonzero(v == 2)[0], np.nonzero(v != 2)[0] if keep else np.empty(0, np.int64)]).astype(np.int64)
        pieces = res.merged_bytes + (res.other_bytes if keep else [])
        rows = np.zeros(len(order), _lib.GREP_ROW_DTYPE)
        rows["src_off"], rows["number"], rows["len"], rows["reserved"] = np.array(starts, np.int64)[order] + text_off, record_base + order, [len(x) for x in pieces], v[order] != 2
        return 0, st, tot, ovl, rows, b"".join(pieces)


def _same(result, want):
    assert result.records == len(want.offset) == len(result)
    for name, got in (("offset", result.offset), ("insert", result.insert), ("overlap", result.overlap), ("mismatches", result.mismatches),
                      ("corrected", result.corrected_per_pair), ("verdict", result.verdict), ("steps", result.steps)):
        assert got.tolist() == getattr(want, name), name
    assert (result.offset.dtype, result.insert.dtype, result.verdict.dtype, result.steps.dtype) == (np.int64, np.int64, np.uint8, np.uint8)
    for name, v in want.totals.items():
        if name not in ("seen", "bytes_in"):
            assert getattr(result, name) == v, name
    assert result.insert_sizes().sum() == result.records


def test_driver_on_a_fake_engine(monkeypatch):
    from zlib_ng_amd import _lib, bgzf
    recs = interleaved(gen_pairs(400, 9))
    data = b"".join(recs)
    BS = 997
    blob, blocks = _stored_bgzf(data, BS)
    coffs = sorted(blocks)
    fake = _FakeOverlapCtx()
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)
    monkeypatch.setattr(bgzf, "BgzfWriter", _Collect)
    cf = conf(first_byte=b"@", correct=True, cut=True)
    want = overlap_ref.overlap_text(data, cf)
    assert want.totals["merged"] > 100 and want.totals["none"] > 100 and want.totals["corrected"] > 10 and want.totals["adapter_pairs"] > 30
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    voff = lambda r: bgzf.make_virtual_offset(coffs[starts[r] // BS], int(starts[r] % BS))

    def overlap(src, merged, unmerged=None, **more):
        args = dict(first_byte=b"@", start=None, stop=None, first_record=0, allow_short=False, qual_line=3, correct=True, merge=True)
        args.update(more)
        _Collect.made.clear()
        fake.calls.clear()
        return bgzf._overlap_file(io.BytesIO(src), fake, merged, unmerged, 8, 1, args["qual_line"], 33, 30, 5, 20, args["merge"], args["correct"], (30, 14), True,
                                  args["first_byte"], b"\n", 1, bgzf.MAX_BLOCK_INPUT, args["start"], args["stop"], args["first_record"], 64 << 20, args["allow_short"])

    for window in (32 << 20, 5000, 1500):
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        # both outputs
        r = overlap(blob, "merged", "other")
        _same(r, want)
        made = {w.target: w for w in _Collect.made}
        assert made["merged"].got == b"".join(want.merged_bytes) and made["other"].got == b"".join(want.other_bytes) and all(w.closed and w.level == 1 for w in made.values())
        assert all(c[2] & _lib.BGZF_CLASSIFY_GROUP and c[3] & _lib.BGZF_OVERLAP_KEEP_UNMERGED for c in fake.calls) and fake.calls[-1][2] & _lib.BGZF_GREP_FINAL
        assert len(fake.calls) == 1 if window == 32 << 20 else len(fake.calls) > 10
        assert sum(c[1] for c in fake.calls) == len(recs)
        # one output: the other class is counted only
        r = overlap(blob, "merged")
        _same(r, want)
        (w,) = _Collect.made
        assert w.closed and w.got == b"".join(want.merged_bytes) and not any(c[3] & _lib.BGZF_OVERLAP_KEEP_UNMERGED for c in fake.calls)
        r = overlap(blob, None, "other")
        (w,) = _Collect.made
        assert w.target == "other" and w.got == b"".join(want.other_bytes)
        # none: nothing is gathered
        r = overlap(blob, None)
        _same(r, want)
        assert not _Collect.made and not any(c[2] & _lib.BGZF_CLASSIFY_GROUP for c in fake.calls)
        # start / stop / first_record
        a, b = 123, 300
        r = overlap(blob, "merged", "other", start=voff(a), stop=voff(b), first_record=a)
        mid = overlap_ref.overlap_text(b"".join(recs[a:b]), cf)
        _same(r, mid)
        made = {w.target: w for w in _Collect.made}
        assert made["merged"].got == b"".join(mid.merged_bytes) and made["other"].got == b"".join(mid.other_bytes) and fake.calls[0][0] == a
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1500)
    # a short last pair
    cut = data[:data.rfind(b"\n", 0, len(data) - 1) + 1]                     # the last pair without mate 2's quality line
    sblob, _ = _stored_bgzf(cut, BS)
    with pytest.raises(ValueError, match=r"record 399, the last one, has 7 of 8 lines"):
        overlap(sblob, None, qual_line=None, correct=False)
    r = overlap(sblob, None, qual_line=None, correct=False, allow_short=True)
    _same(r, overlap_ref.overlap_text(cut, conf(first_byte=b"@", qual_line=None, cut=True)))
    # a length fault mid-file, in mate 2: the record, its virtual offset, the mate and both lengths; the outputs are closed and incomplete
    lines = data.split(b"\n")
    n_seq = len(lines[8 * 300 + 5])
    lines[8 * 300 + 7] += b"F"
    fblob, fblocks = _stored_bgzf(b"\n".join(lines), BS)
    at = len(b"\n".join(lines[:8 * 300])) + 1
    v = bgzf.make_virtual_offset(sorted(fblocks)[at // BS], at % BS)
    with pytest.raises(ValueError, match=r"record 300 at virtual offset %d: line 5 \(the sequence of mate 2\) has %d bytes and line 7 \(its qualities\) has %d.*overlap_records.*incomplete"
                       % (v, n_seq, n_seq + 1)):
        overlap(fblob, "merged", "other")
    assert len(_Collect.made) == 2 and all(w.closed for w in _Collect.made) and 0 < len(_Collect.made[0].got) < len(b"".join(want.merged_bytes))
    lines = data.split(b"\n")
    lines[8 * 300 + 3] = lines[8 * 300 + 3][:-1]
    fblob, _ = _stored_bgzf(b"\n".join(lines), BS)
    with pytest.raises(ValueError, match=r"record 300 at virtual offset \d+: line 1 \(the sequence of mate 1\) has (\d+) bytes and line 3 \(its qualities\) has \d+.*incomplete"):
        overlap(fblob, "merged")
    # a first_byte violation on the way, in mate 2's first line
    lines = data.split(b"\n")
    lines[8 * 301 + 4] = b"x" + lines[8 * 301 + 4][1:]
    bblob, _ = _stored_bgzf(b"\n".join(lines), BS)
    with pytest.raises(ValueError, match=r"record 301 at virtual offset \d+ does not start with b'@'.*overlap_records.*incomplete"):
        overlap(bblob, "merged", "other")
    assert len(_Collect.made) == 2 and all(w.closed for w in _Collect.made) and 0 < len(_Collect.made[0].got) < len(b"".join(want.merged_bytes))


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
    exe = str(tmp_path / "overlap_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "overlap_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf overlap arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

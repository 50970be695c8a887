"""CPU: the BGZF contaminant screen, without a GPU -- the referee of screen_ref.py against codes worked out by hand; the new entry points
are declared, exported and bound, keep ZNGAMD_ABI and the kernel classes, and refuse hostile arguments with no context at all; the
Python argument checks raise before a file is opened; KmerSet and ScreenResult on arrays written by hand; and tests/screen_args.cpp, a
stand-alone program, against the library's host side under AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process,
nothing preloaded)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import screen_inputs as I
import screen_ref as R
from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_dedup import _struct_fields
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang


def test_referee_against_codes_worked_out_by_hand():
    # ACGT, k = 2: AC = 0 * 4 + 1, CG = 1 * 4 + 2, GT = 2 * 4 + 3; canonical: GT is AC read backwards, CG is its own reverse complement
    assert R.codes_of(b"ACGT", 2, False) == [1, 6, 11] and R.codes_of(b"ACGT", 2, True) == [1, 6, 1]
    # a palindrome at k = 4: 0 << 6 | 1 << 4 | 2 << 2 | 3
    assert R.codes_of(b"ACGT", 4, False) == [27] == R.codes_of(b"ACGT", 4, True) and I.rc(b"ACGT") == b"ACGT"
    assert R.codes_of(b"ACGT", 5, True) == [] and R.codes_of(b"", 1, True) == [] and R.codes_of(b"ACGT", 1, False) == [0, 1, 2, 3]
    assert R.codes_of(b"ACGT", 1, True) == [0, 1, 1, 0]                             # (a base and its complement)
    # U as T; lower case
    assert R.codes_of(b"ACGU", 2, False) == [1, 6, 11] == R.codes_of(b"acgu", 2, False) == R.codes_of(b"aCgT", 2, False)
    # canonical against forward: TT = 15, its reverse complement AA = 0
    assert R.codes_of(b"TT", 2, False) == [15] and R.codes_of(b"TT", 2, True) == [0] and R.codes_of(b"AA", 2, True) == [0]
    # the largest code: 31 T, forward, is 4^31 - 1 < 2^62; canonical it is 31 A
    assert R.codes_of(b"T" * 31, 31, False) == [4 ** 31 - 1] and R.codes_of(b"T" * 31, 31, True) == [0] and 4 ** 31 - 1 < (1 << 64) - 1
    # an N kills exactly k positions; every other byte does too
    for k in (1, 3, 7):
        seq = b"ACGTTGCA" * 4
        for bad in (b"N", b"n", b"-", b"R", b"\x00", b"@"):
            codes = R.codes_of(seq[:12] + bad + seq[13:], k, False)
            assert [i for i, c in enumerate(codes) if c is None] == list(range(12 - k + 1, 13)), (k, bad)
    # a k-mer in two references; k-mers do not span references; a reference shorter than k adds nothing
    table, positions, valid = R.build([b"ACG", b"CGT", b"A", b""], 2, False)
    assert table == {1: 1, 6: 3, 11: 2} and (positions, valid) == (4, 4) and R.pairs(table) == [(1, 1), (6, 3), (11, 2)]
    assert 9 not in table                                                           # GC, which only the joint of the first two would hold
    table, positions, valid = R.build([b"ACG", b"CGT"], 2, True)
    assert table == {1: 3, 6: 3} and R.build([b"ANG"], 2, True) == ({}, 2, 0) and R.build([b""], 2, True) == ({}, 0, 0)
    # a record: kmers, hits, refs, best, best_hits
    table = R.build([b"AC", b"GT"], 2, False)[0]
    assert R.screen(b"ACGT", table, 2, False) == R.Row(3, 3, 2, 0, 1)               # a tie: the lowest number wins
    table = R.build([b"GT", b"AC"], 2, False)[0]
    assert R.screen(b"ACGT", table, 2, False) == R.Row(3, 3, 2, 0, 1)
    assert R.screen(b"ACGTAC", R.build([b"GT", b"AC"], 2, False)[0], 2, False) == R.Row(3, 5, 3, 1, 2)
    assert R.screen(b"ACGT", R.build([b"CG", b"CG", b"ACGT"], 2, False)[0], 2, False) == R.Row(7, 3, 3, 2, 3)      # a position counts for every reference
    assert R.screen(b"AANAA", table, 2, False) == R.Row(0, 2, 0, R.NONE, 0) and R.screen(b"A", table, 2, False) == R.Row(0, 0, 0, R.NONE, 0)
    assert R.NONE == 0xFFFFFFFF and [R.cap_of(n) for n in (0, 1, 32, 33, 64, 65)] == [64, 64, 64, 128, 128, 256]
    # the records of a text
    text = b"@a\nAC\n+\nII\n@s\nGT"
    rows, tot = R.screen_text(text, table, 2, False)
    assert rows == [R.Row(2, 1, 1, 1, 1), R.Row(1, 1, 1, 0, 1)] and tot == R.Totals(2, 16, 4, 2, 2, 2)
    rows, tot = R.screen_text(text, table, 2, False, final=False)
    assert rows == [R.Row(2, 1, 1, 1, 1)] and tot == R.Totals(1, 11, 2, 1, 1, 1)
    assert R.screen_text(text, table, 2, False, min_hits=2)[1].matched == 0 and R.screen_text(b"@a\nAC\n", table, 2, False, final=False)[1].seen == 0


def test_inputs_are_what_they_say():
    for k in I.BUILD_K:
        refs = I.build_references(k, 64)
        assert {0, k - 1, k, k + 1, 63 + k, 64 + k, 5003} <= {len(r) for r in refs} and refs[-1] == I.rc(refs[0])
        assert any(r[:1] == b"N" for r in refs) and any(len(r) > 64 and r[63] == r[64] == ord("n") for r in refs) and any(r.islower() for r in refs)
    table, positions, valid = R.build([I.wrap_reference()], 4, False)
    assert len(table) == positions == valid == 32 and R.cap_of(positions) == 64
    refs = I.screen_references()
    assert len(refs) == 64 and len(refs[0]) > I.LONG and len({r[100:100 + I.COMMON] for r in refs}) == 1
    for k, canonical in I.SCREEN_RULES:
        bodies = I.screen_bodies(k)
        assert {0, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127, 128, 129, I.LONG} <= {len(b) for b in bodies} and len(bodies) > 1900


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32, "zngamd_alloc_fn": _lib.ALLOC_FN}

    def params_of(name, ret="int"):
        return [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\b%s %s\s*\(([^;]*)\);" % (ret, name), header).group(1).split(",")]

    names = ("zngamd_kmer_set_build", "zngamd_kmer_set_load", "zngamd_kmer_set_export", "zngamd_kmer_set_describe", "zngamd_bgzf_screen_records_dev",
             "zngamd_bgzf_screen_records")
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        want = [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params_of(name)]
        assert getattr(L, name).argtypes == want, name
    assert "zngamd_kmer_set_free" in _lib.SYMBOLS and params_of("zngamd_kmer_set_free", "void") == ["zngamd_kmer_set *set"]
    assert L.zngamd_kmer_set_free.argtypes == [C.c_void_p] and L.zngamd_kmer_set_free.restype is None
    for name in ("zngamd_bgzf_screen_records_dev", "zngamd_bgzf_screen_records"):
        params = params_of(name)
        key = params_of(name.replace("screen", "key"))
        assert params[:9] == key[:9] and params[9:12] == ["const zngamd_bgzf_screen_conf *conf", "const zngamd_kmer_set *set", "uint64_t record_base"]
        assert [p.replace("screen", "key") for p in params[12:]] == key[11:]                 # the scratch (or status), the rows, alloc, the totals
    assert params_of("zngamd_kmer_set_build") == ["zngamd_ctx *ctx", "const uint8_t *seqs", "const uint64_t *offsets", "uint32_t n_refs", "uint32_t k",
                                                  "uint32_t flags", "zngamd_kmer_set **out", "zngamd_kmer_set_info *info"]
    assert params_of("zngamd_kmer_set_load") == ["zngamd_ctx *ctx", "uint32_t k", "uint32_t flags", "uint32_t n_refs", "const uint64_t *codes",
                                                 "const uint64_t *masks", "uint64_t n", "zngamd_kmer_set **out", "zngamd_kmer_set_info *info"]
    assert params_of("zngamd_kmer_set_export") == ["zngamd_kmer_set *set", "uint64_t *codes", "uint64_t *masks", "uint64_t cap_pairs", "uint64_t *n"]
    for struct, ct, size in (("zngamd_bgzf_screen_conf", _lib.BgzfScreenConf, 64), ("zngamd_bgzf_screen_totals", _lib.BgzfScreenTotals, 88),
                             ("zngamd_kmer_set_info", _lib.KmerSetInfo, 48)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert int(re.search(r"\}\s*zngamd_bgzf_screen_row;\s*/\* (\d+) B \*/", header).group(1)) == _lib.SCREEN_ROW_DTYPE.itemsize == 24
    assert _struct_fields(header, "zngamd_bgzf_screen_row") == list(_lib.SCREEN_ROW_DTYPE.names) == ["refs", "kmers", "hits", "best", "best_hits"]
    # the totals are the key call's, then kmers, hits, matched
    key_fields = [f[0] for f in _lib.BgzfKeyTotals._fields_]
    assert [f[0] for f in _lib.BgzfScreenTotals._fields_] == key_fields + ["kmers", "hits", "matched"]
    assert all(getattr(_lib.BgzfScreenTotals, f).offset == getattr(_lib.BgzfKeyTotals, f).offset for f in key_fields) and _lib.BgzfScreenTotals.kmers.offset == 64
    assert len(_lib.BgzfScreenConf().reserved) == 11
    for macro, value in (("CANONICAL", _lib.KMER_CANONICAL), ("MAX_K", _lib.KMER_MAX_K), ("MAX_REFS", _lib.KMER_MAX_REFS)):
        assert int(re.search(r"#define ZNGAMD_KMER_%s\s+(\d+)u" % macro, header).group(1)) == value
    assert int(re.search(r"#define ZNGAMD_KMER_NONE\s+(0x[0-9A-F]+)u", header).group(1), 16) == _lib.KMER_NONE == R.NONE
    assert re.search(r"#define ZNGAMD_KMER_MAX_POSITIONS\s+\(1ull << 28\)", header) and _lib.KMER_MAX_POSITIONS == 1 << 28
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_screen.hip"' in build
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_sort.hip"') < main.index('#include "za_screen.hip"')
    kernel = open(os.path.join(PKG_DIR, "csrc", "za_screen.hip")).read()
    for k in ("za_k_kmer_clear", "za_k_kmer_insert", "za_k_kmer_load", "za_k_kmer_export", "za_k_screen"):
        assert "void %s(" % k in kernel and k in main
    # the close kernel is the one the one-fault calls share, for the screen's totals
    assert "void za_k_rec_close(" in open(os.path.join(PKG_DIR, "csrc", "za_grep_records.hip")).read() and "za_k_rec_close<ZaScreenTotals>" in main
    assert "__shared__" not in kernel                                              # no LDS


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every fault of the arguments -- and with everything in order -- and nothing is written"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    p = lambda a: C.c_void_p(a.ctypes.data)

    def build(seqs=True, offsets=(0, 40, 90), n_refs=2, k=21, flags=1, out=True, info=True):
        blob = np.frombuffer(b"ACGT" * 25, np.uint8).copy()
        off = np.array(offsets if offsets is not None else (0,), np.uint64)
        h, i = C.c_void_p(0x5A5A), _lib.KmerSetInfo()
        C.memset(C.byref(i), 0x5A, C.sizeof(i))
        r = L.zngamd_kmer_set_build(None, p(blob) if seqs else None, p(off) if offsets is not None else None, n_refs, k, flags,
                                    C.byref(h) if out else None, C.byref(i) if info else None)
        assert h.value == 0x5A5A and bytes(i) == b"\x5A" * C.sizeof(i)
        return r

    for kw in (dict(k=0), dict(k=32), dict(k=1 << 31), dict(n_refs=0), dict(n_refs=65, offsets=tuple(range(66))), dict(offsets=(0, 50, 40)), dict(offsets=(10, 0, 90)),
               dict(offsets=None), dict(out=False), dict(seqs=False), dict(flags=2), dict(flags=3), dict(flags=1 << 31),
               dict(offsets=(0, (1 << 28) + 21), n_refs=1), dict(offsets=(0, 1 << 63, 1 << 63), k=1), dict()):
        assert build(**kw) == E_ARG, kw

    def load(codes=(1, 2), masks=(1, 3), n=None, k=2, flags=1, n_refs=2, out=True, with_arrays=True):
        c, m = np.array(codes, np.uint64), np.array(masks, np.uint64)
        h = C.c_void_p(0x5A5A)
        r = L.zngamd_kmer_set_load(None, k, flags, n_refs, p(c) if with_arrays else None, p(m) if with_arrays else None, len(c) if n is None else n,
                                   C.byref(h) if out else None, None)
        assert h.value == 0x5A5A
        return r

    for kw in (dict(k=0), dict(k=32), dict(n_refs=0), dict(n_refs=65), dict(flags=2), dict(out=False), dict(with_arrays=False), dict(codes=(1, 16)),
               dict(codes=(1, (1 << 64) - 1)), dict(masks=(1, 0)), dict(masks=(1, 4)), dict(masks=(1, 1 << 63)), dict(n=(1 << 28) + 1), dict(n=(1 << 64) - 1),
               dict(codes=(4 ** 31,), masks=(1,), k=31), dict(), dict(codes=(), masks=(), with_arrays=False)):
        assert load(**kw) == E_ARG, kw

    n = C.c_uint64(0x5A)
    assert L.zngamd_kmer_set_export(None, None, None, 0, C.byref(n)) == E_ARG and n.value == 0x5A
    info = _lib.KmerSetInfo()
    assert L.zngamd_kmer_set_describe(None, C.byref(info)) == E_ARG
    L.zngamd_kmer_set_free(None)                                                     # nothing happens

    F = _lib.BGZF_GREP_FINAL

    def screen(form, delim=10, flags=F, totals=True, with_conf=True, rows=True, alloc=False, **fields):
        cf = _lib.BgzfScreenConf(4, 1, 64, 1, 0)
        for name, v in fields.items():
            if name == "reserved":
                cf.reserved[v] = 1
            else:
                setattr(cf, name, v)
        t = _lib.BgzfScreenTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        row = np.zeros(1, _lib.SCREEN_ROW_DTYPE)
        rp = C.c_void_p(row.ctypes.data) if rows else None
        head = (None, None, 0, None, 0, 0, 0, delim, flags, C.byref(cf) if with_conf else None, None, 0)      # (no context: no set either)
        tail = (C.byref(t) if totals else None,)
        if form == 0:
            fn = _lib.ALLOC_FN(lambda user, n: pytest.fail("the allocator was called")) if alloc else _lib.ALLOC_FN()
            r = L.zngamd_bgzf_screen_records(*head, None, rp, 0, fn, None, *tail)
        else:
            r = L.zngamd_bgzf_screen_records_dev(*head, None, 0, None, rp, 0, *tail)
        assert bytes(t) == b"\x5A" * C.sizeof(t) and not row["refs"][0] and not row["hits"][0]      # a refused call writes nothing
        return r

    for form in range(2):
        for fields in (dict(record_lines=0), dict(record_lines=65), dict(seq_line=-1), dict(seq_line=4), dict(first_byte=-2), dict(first_byte=256), dict(min_hits=0),
                       dict(flags=1), dict(flags=1 << 31), dict(reserved=0), dict(reserved=10)):
            assert screen(form, **fields) == E_ARG, (form, fields)
        for kw in (dict(delim=-1), dict(delim=256), dict(flags=F | 1), dict(flags=F | 2), dict(flags=F | 8), dict(flags=1 << 31), dict(totals=False),
                   dict(with_conf=False), dict(rows=False), dict()):
            assert screen(form, **kw) == E_ARG, (form, kw)
    assert screen(0, rows=False, alloc=True) == E_ARG


def _hand_set():
    from zlib_ng_amd import bgzf
    return bgzf.KmerSet.from_codes(2, [11, 1, 6, 6], [2, 1, 1, 2], 2, canonical=False, names=["phix", b"vector"])


def test_python_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    f, kset = _Unreadable(), _hand_set()
    bad = (dict(seq_line=4), dict(seq_line=-1), dict(min_hits=0), dict(min_hits=-1), dict(min_hits=1 << 32), dict(min_hits=1.0), dict(min_hits=None),
           dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(record_lines=0), dict(record_lines=65), dict(max_record=0))
    for kw in bad:
        with pytest.raises(ValueError):
            bgzf.screen_records(f, kset, **kw)
        with pytest.raises(ValueError):
            bgzf.screen_filter(f, kset, None, **kw)
        if "max_record" not in kw:
            with pytest.raises(ValueError):
                bgzf.screen_records("/nonexistent/reads.fq.gz", kset, **kw)             # (judged before a file is opened)
            with pytest.raises(ValueError):
                bgzf.screen_filter("/nonexistent/reads.fq.gz", kset, "/nonexistent/out.gz", "/nonexistent/hit.gz", **kw)
    for not_a_set in (None, b"ACGT", [b"ACGT"], 31):
        with pytest.raises(ValueError, match="kset is a KmerSet"):
            bgzf.screen_records("/nonexistent/reads.fq.gz", not_a_set)
        with pytest.raises(ValueError, match="kset is a KmerSet"):
            bgzf.screen_filter(f, not_a_set, None)
    with pytest.raises(ValueError, match="min_hits is an integer between 1 and 4294967295, not 0"):
        bgzf.screen_records(f, kset, min_hits=0)
    with pytest.raises(ValueError, match="block_size"):
        bgzf.screen_filter("/nonexistent/reads.fq.gz", kset, "/nonexistent/out.gz", block_size=0)
    for kw in (dict(qual_line=3), dict(canonical=True), dict(k=21)):
        with pytest.raises(TypeError):
            bgzf.screen_records(f, kset, **kw)
    # the set's own arguments
    for kw in (dict(k=0), dict(k=32), dict(k=21.0), dict(canonical=1), dict(names=["a"]), dict(references=[]), dict(references=[b"A"] * 65)):
        args = dict(references=[b"ACGT" * 20, b"TTGA" * 20], k=21, canonical=True, names=None)
        args.update(kw)
        with pytest.raises(ValueError):
            bgzf.KmerSet.build(**args)
    with pytest.raises(ValueError):
        bgzf.KmerSet.from_fasta("/nonexistent/ref.fa.gz", k=32)
    for args in ((2, [16], [1], 1), (2, [1], [0], 1), (2, [1], [2], 1), (2, [1, 2], [1], 1), (2, [1], [1], 0), (2, [1], [1], 65), (0, [0], [1], 1),
                 (2, [-1], [1], 1), (2, [[1]], [[1]], 1), (2, [1.5], [1], 1)):
        with pytest.raises(ValueError):
            bgzf.KmerSet.from_codes(*args)
    cf, d = bgzf._screen_conf(kset, 4, np.int64(1), 5, b"@", b"\n")
    assert (cf.record_lines, cf.seq_line, cf.first_byte, cf.min_hits, cf.flags, list(cf.reserved), d) == (4, 1, 64, 5, 0, [0] * 11, b"\n")
    cf, d = bgzf._screen_conf(kset, 2, 0, 1, None, b";")
    assert (cf.seq_line, cf.first_byte, d) == (0, -1, b";")
    for name in ("KmerSet", "ScreenResult", "screen_records", "screen_filter"):
        assert name in bgzf.__all__
    rec_kw = ["first_byte", "delimiter", "start", "stop", "first_record", "max_record", "allow_short"]
    sig = inspect.signature(bgzf.screen_records).parameters
    assert list(sig) == ["file", "kset", "record_lines", "seq_line", "min_hits"] + rec_kw
    assert list(inspect.signature(bgzf.BgzfReader.screen_records).parameters) == ["self", "kset", "record_lines", "seq_line", "min_hits"] + rec_kw
    defaults = {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(record_lines=4, seq_line=1, min_hits=1, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0,
                            max_record=64 << 20, allow_short=False)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.items() if k not in ("file", "kset", "record_lines"))
    out_kw = ["seq_line", "min_hits", "compresslevel", "block_size"]
    sig = inspect.signature(bgzf.screen_filter).parameters
    assert list(sig) == ["file", "kset", "output", "matched", "record_lines"] + out_kw + rec_kw
    assert list(inspect.signature(bgzf.BgzfReader.screen_filter).parameters) == ["self", "kset", "output", "matched", "record_lines"] + out_kw + rec_kw
    assert (sig["matched"].default, sig["compresslevel"].default, sig["block_size"].default) == (None, 6, bgzf.MAX_BLOCK_INPUT)
    build = inspect.signature(bgzf.KmerSet.build).parameters
    assert {k: v.default for k, v in build.items() if k != "references"} == dict(k=31, canonical=True, names=None)


def test_kmer_set_on_arrays_written_by_hand(tmp_path):
    from zlib_ng_amd import bgzf
    s = _hand_set()
    assert (s.k, s.canonical, s.names, s.n_refs, len(s)) == (2, False, ("phix", "vector"), 2, 3)
    assert s.codes.dtype == s.masks.dtype == np.uint64 and s.codes.tolist() == [1, 6, 11] and s.masks.tolist() == [1, 3, 2]      # sorted; twice: ORed
    assert list(zip(s.codes.tolist(), s.masks.tolist())) == R.pairs(R.build([b"ACG", b"CGT"], 2, False)[0])
    assert repr(s) == "<KmerSet: k = 2, 2 references, 3 codes>"
    t = bgzf.KmerSet.from_codes(2, [15, 1], [2, 2], 2, canonical=False, names=["phix", "vector"])
    u = s | t
    assert u.codes.tolist() == [1, 6, 11, 15] and u.masks.tolist() == [3, 3, 2, 2] and (u.k, u.canonical, u.names) == (2, False, s.names)
    assert s.codes.tolist() == [1, 6, 11] and (t | s) == u and (s | s) == s and u != s
    for other in (bgzf.KmerSet.from_codes(3, [1], [1], 2, canonical=False, names=s.names), bgzf.KmerSet.from_codes(2, [1], [1], 2, canonical=True, names=s.names),
                  bgzf.KmerSet.from_codes(2, [1], [1], 2, canonical=False), bgzf.KmerSet.from_codes(2, [1], [1], 3, canonical=False)):
        with pytest.raises(ValueError, match="equal k, canonical and names"):
            s | other
    with pytest.raises(TypeError):
        s | {1}
    path = str(tmp_path / "set.npz")
    u.save(path)
    back = bgzf.KmerSet.load(path)
    assert back == u and (back.k, back.canonical, back.names) == (2, False, ("phix", "vector")) and back.codes.tolist() == u.codes.tolist()
    assert back.masks.tolist() == u.masks.tolist() and back.codes.dtype == np.uint64
    empty = bgzf.KmerSet.from_codes(31, [], [], 64)
    assert len(empty) == 0 and empty.canonical and empty.names[63] == "ref63" and (empty | empty) == empty
    empty.save(path)
    assert bgzf.KmerSet.load(path) == empty
    big = bgzf.KmerSet.from_codes(31, [4 ** 31 - 1], [1 << 63], 64)
    assert big.codes.tolist() == [4 ** 31 - 1] and big.masks.tolist() == [1 << 63]


def test_screen_result_on_arrays_written_by_hand():
    from zlib_ng_amd import bgzf
    a = lambda *v: np.array(v, np.int64)
    names = ("phix", "vector", "rrna")
    #                       record: 0  1  2  3  4  5
    r = bgzf.ScreenResult(a(70, 70, 0, 70, 12, 70), a(0, 5, 0, 70, 4, 1), np.array([0, 3, 0, 4, 2, 1], np.uint64), a(-1, 0, -1, 2, 1, 0), a(0, 5, 0, 70, 4, 1),
                          600, 5, names, "id")
    assert (r.records, len(r), r.bases, r.min_hits, r.matched_records) == (6, 6, 600, 5, 2)
    assert r.matched.dtype == np.bool_ and r.matched.tolist() == [False, True, False, True, False, False]
    assert r.by_reference().dtype == np.int64 and r.by_reference().tolist() == [2, 1, 1]
    assert r.drop().dtype == np.uint8 and r.drop().tolist() == [0, 1, 0, 1, 0, 0]
    assert r.labels().dtype == np.int64 and r.labels().tolist() == [0, 1, 0, 1, 0, 0]
    assert r.labels(bgzf.DROP).tolist() == [0, -1, 0, -1, 0, 0] and r.labels(0, bgzf.DROP).tolist() == [-1, 0, -1, 0, -1, -1] and r.labels(7, 3).tolist() == [3, 7, 3, 7, 3, 3]
    one = bgzf.ScreenResult(a(9), a(9), np.array([4], np.uint64), a(2), a(9), 40, 5, names, "id")
    s = r + one
    assert (s.records, s.bases, s.matched_records) == (7, 640, 3) and s.hits.tolist() == [0, 5, 0, 70, 4, 1, 9] and s.refs.dtype == np.uint64
    assert s.best.tolist() == [-1, 0, -1, 2, 1, 0, 2] and s.by_reference().tolist() == [2, 1, 2] and r.records == 6 and (one + r).hits.tolist()[0] == 9
    for other in (bgzf.ScreenResult(a(9), a(9), np.array([4], np.uint64), a(2), a(9), 40, 1, names, "id"),
                  bgzf.ScreenResult(a(9), a(9), np.array([4], np.uint64), a(2), a(9), 40, 5, names, "another"),
                  bgzf.ScreenResult(a(9), a(9), np.array([4], np.uint64), a(2), a(9), 40, 5, names[:2], "id")):
        with pytest.raises(ValueError, match="not comparable"):
            r + other
    with pytest.raises(TypeError):
        r + 1
    none = bgzf.ScreenResult(a(), a(), np.empty(0, np.uint64), a(), a(), 0, 1, names, "id")
    assert (none.records, none.matched_records, none.by_reference().tolist(), none.drop().tolist()) == (0, 0, [0, 0, 0], [])
    assert repr(r) == "<ScreenResult: 6 records, 2 matched (min_hits 5)>"


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
    exe = str(tmp_path / "screen_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "screen_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf screen arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

"""CPU: the BGZF k-mer count, without a GPU -- the referee of kcount_ref.py against codes, counts and runs worked out by hand; the new
entry points are declared, exported and bound, keep ZNGAMD_ABI and the kernel classes, and refuse hostile arguments with no context at
all; the Python argument checks raise before a file is opened; KmerCounts on arrays written by hand; and tests/kcount_args.cpp, a
stand-alone program, against the library's host side under AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process,
nothing preloaded)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import kcount_inputs as I
import kcount_ref as R
from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_dedup import _struct_fields
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang


def test_referee_against_counts_worked_out_by_hand():
    # ACGT, k = 2: AC = 1, CG = 6, GT = 11; canonical: GT is AC read backwards, CG is its own reverse complement
    assert R.codes_of(b"ACGT", 2, False) == [1, 6, 11] and R.codes_of(b"ACGT", 2, True) == [1, 6, 1]
    assert R.count_bodies([b"ACGT"], 2, False) == ({1: 1, 6: 1, 11: 1}, 3, 3, 3) and R.count_bodies([b"ACGT"], 2, True) == ({1: 2, 6: 1}, 3, 3, 2)
    # the sliding codes are the codes of the definition
    rng = np.random.default_rng(3)
    for k in (1, 2, 5, 16, 31):
        seq = I.spoil(I.rand_seq(rng, 200), (0, 17, 18, 90, 199)).replace(b"T", b"u", 3)
        for canonical in (False, True):
            assert R.codes_of(seq, k, canonical) == [R.code_at(seq, p, k, canonical) for p in range(len(seq) - k + 1)]
    assert R.codes_of(b"ACG", 4, True) == [] and R.codes_of(b"", 1, False) == [] and R.codes_of(b"T" * 31, 31, False) == [4 ** 31 - 1]
    # AAAAA, k = 2: four positions, one code, one run; with an N in the middle two runs of one
    assert R.count_bodies([b"AAAAA"], 2, False) == ({0: 4}, 4, 1, 1) and R.count_bodies([b"AANAA"], 2, False) == ({0: 2}, 2, 2, 1)
    # ACACAC, k = 2: AC CA AC CA AC -- no two neighbours are equal, five runs; canonical CA is TG: still alternating
    assert R.count_bodies([b"ACACAC"], 2, False) == ({1: 3, 4: 2}, 5, 5, 2) and R.count_bodies([b"ACACAC"], 2, True) == ({1: 3, 4: 2}, 5, 5, 2)
    # ATATAT, k = 2, canonical: AT and TA are both their own reverse complements
    assert R.count_bodies([b"ATATA"], 2, True) == ({3: 2, 12: 2}, 4, 4, 2)
    # AATT, k = 2, canonical: AA = 0, AT = 3, TT -> AA = 0: the two AA are not neighbours
    assert R.count_bodies([b"AATT"], 2, True) == ({0: 2, 3: 1}, 3, 3, 2)
    # 150 G, k = 31: 120 positions in strips of 64 and 56: two runs.  Forward the code is 31 times 2; canonical it is 31 C, 31 times 1
    g, c = sum(2 << 2 * i for i in range(31)), sum(1 << 2 * i for i in range(31))
    assert R.count_bodies([b"G" * 150], 31, False) == ({g: 120}, 120, 2, 1) and R.count_bodies([b"G" * 150], 31, True) == ({c: 120}, 120, 2, 1)
    # the strip edge: 64 positions are one run, 65 are two; an invalid byte ends a run and the strip's first position begins one
    assert [R.count_bodies([b"G" * (n + 30)], 31, True)[2] for n in (1, 63, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert R.count_bodies([b"G" * 40 + b"N" + b"G" * 80], 31, False)[1:3] == (10 + 50, 3)      # 0 .. 9; 41 .. 63; 64 .. 90
    assert R.count_bodies([b"G" * 40 + b"N" + b"G" * 53], 31, False)[1:3] == (10 + 23, 2)      # 0 .. 9; 41 .. 63
    assert R.count_bodies([b"G" * 100 + b"N" + b"G" * 100], 31, False)[1:3] == (140, 4)      # 70 positions: two strips; 31 invalid; 70 more from 101: 27 + 43
    # two records: runs do not carry over; a second read of the same adds and claims nothing
    table, kmers, adds, claimed = R.count_bodies([b"GGGG", b"GGGG"], 2, False)
    assert (table, kmers, adds, claimed) == ({10: 6}, 6, 2, 1) and R.count_bodies([b"GGG"], 2, False, table)[1:] == (2, 1, 0) and table == {10: 8}
    # pairs, the filter, the spectrum and its last bin
    table = {5: 1, 9: 2, 1: 2, 7: 5, 3: 9}
    assert R.pairs(table) == [(1, 2), (3, 9), (5, 1), (7, 5), (9, 2)] and R.pairs(table, 2) == [(1, 2), (3, 9), (7, 5), (9, 2)]
    assert R.pairs(table, 2, 5) == [(1, 2), (7, 5), (9, 2)] and R.pairs(table, 10) == []
    assert R.spectrum(table, 11) == [0, 1, 2, 0, 0, 1, 0, 0, 0, 1, 0] and R.spectrum(table, 10) == [0, 1, 2, 0, 0, 1, 0, 0, 0, 1]
    assert R.spectrum(table, 6) == [0, 1, 2, 0, 0, 2] and R.spectrum(table, 3) == [0, 1, 4] and R.spectrum(table, 2) == [0, 5] and R.spectrum({}, 2) == [0, 0]
    # the table's size and the reserve rule
    assert [R.cap_of(n) for n in (0, 1, 32, 33, 64, 65)] == [64, 64, 64, 128, 128, 256]
    assert R.reserve(64, 0, 32) == 64 and R.reserve(64, 0, 33) == 256 and R.reserve(64, 20, 12) == 64 and R.reserve(64, 20, 13) == 256
    assert R.reserve(256, 20, 108) == 256 and R.reserve(256, 20, 109) == 1024 and R.reserve(1024, 0, 1) == 1024
    # the records of a text
    text = b"@a\nACAC\n+\nIIII\n@s\nGTG"
    assert R.count_text(text, 2, False) == ({1: 2, 4: 1, 11: 1, 14: 1}, R.Totals(2, 21, 7, 5, 4, 5))
    assert R.count_text(text, 2, False, final=False) == ({1: 2, 4: 1}, R.Totals(1, 15, 4, 3, 2, 3))
    assert R.count_text(text, 2, True)[0] == {1: 3, 4: 2} and R.count_text(b"@a\nAC\n", 2, False, final=False)[1].seen == 0


def test_inputs_are_what_they_say():
    for k, canonical in I.GRID:
        bodies = I.screen_bodies(k)
        assert {0, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127, 128, 129, 3000} <= {len(b) for b in bodies} and len(bodies) > 1900
        assert any(b[63:64] == b"N" for b in bodies) and any(b[64:65] == b"n" for b in bodies) and any(b"U" in b for b in bodies)
    assert [(k, c) for k, c in I.GRID] == [(1, False), (2, True), (15, True), (16, False), (17, True), (31, False), (31, True)]
    for k in (3, 15, 31):
        bodies = I.repeat_bodies(k)
        assert [len(b) for b in bodies[:5]] == [150, 64, 65, 63 + k, 64 + k] and all(set(b) == {ord("G")} for b in bodies[:5])
        assert any(b.endswith(b"G" * 60) and set(b) != {ord("G")} for b in bodies) and b"AC" * 75 in bodies and b"ACG" * 50 in bodies
        assert any(len(b) > 40 and b == I.rc(b) for b in bodies) and any(b"N" in b and b.count(b"G") == 120 for b in bodies)
        # a run that crosses the strip edge at 64: the referee gives it two adds where one strip would give one
        crossing = [b for b in bodies if b[50:90] == b"C" * 40]
        assert len(crossing) == 1
        codes = R.codes_of(crossing[0], k, False)
        if k <= 15:
            assert codes[63] == codes[64] is not None and R.runs_of(codes) == R.runs_of(codes[:64]) + R.runs_of(codes[64:])
    read = I.contention_read()
    assert len(read) == 150 and len(set(R.codes_of(read, 31, True))) == 120 and I.CONTENTION == 4096


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32}

    def params_of(name, ret="int"):
        return [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\b%s %s\s*\(([^;]*)\);" % (ret, name), header).group(1).split(",")]

    names = ("zngamd_kmer_counter_new", "zngamd_kmer_counter_reserve", "zngamd_kmer_counter_add", "zngamd_kmer_counter_describe",
             "zngamd_kmer_counter_histogram", "zngamd_kmer_counter_export", "zngamd_bgzf_count_kmers_dev", "zngamd_bgzf_count_kmers")
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        want = [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params_of(name)]
        assert getattr(L, name).argtypes == want, name
    assert "zngamd_kmer_counter_free" in _lib.SYMBOLS and params_of("zngamd_kmer_counter_free", "void") == ["zngamd_kmer_counter *counter"]
    assert L.zngamd_kmer_counter_free.argtypes == [C.c_void_p] and L.zngamd_kmer_counter_free.restype is None
    # the window calls: the screen's parameters without the rows
    for name in ("zngamd_bgzf_count_kmers_dev", "zngamd_bgzf_count_kmers"):
        params = params_of(name)
        screen = params_of(name.replace("count_kmers", "screen_records"))
        assert params[:9] == screen[:9] and params[9:12] == ["const zngamd_bgzf_count_conf *conf", "zngamd_kmer_counter *counter", "uint64_t record_base"]
        rest = [p.replace("screen", "count") for p in screen[12:]]
        rows = [p for p in rest if "rows" in p or "alloc" in p or p == "void *user"]
        assert [p for p in rest if p not in rows] == params[12:] and len(rows) == (4 if name.endswith("kmers") else 2)
    assert params_of("zngamd_kmer_counter_new") == ["zngamd_ctx *ctx", "uint32_t k", "uint32_t flags", "uint64_t room", "zngamd_kmer_counter **out"]
    assert params_of("zngamd_kmer_counter_reserve") == ["zngamd_kmer_counter *counter", "uint64_t room"]
    assert params_of("zngamd_kmer_counter_add") == ["zngamd_kmer_counter *counter", "const uint64_t *codes", "const uint64_t *counts", "uint64_t n"]
    assert params_of("zngamd_kmer_counter_histogram") == ["zngamd_kmer_counter *counter", "uint64_t *hist", "uint32_t bins"]
    assert params_of("zngamd_kmer_counter_export") == ["zngamd_kmer_counter *counter", "uint64_t min_count", "uint64_t max_count", "uint64_t *codes",
                                                       "uint64_t *counts", "uint64_t cap_pairs", "uint64_t *n"]
    for struct, ct, size in (("zngamd_bgzf_count_conf", _lib.BgzfCountConf, 64), ("zngamd_bgzf_count_totals", _lib.BgzfCountTotals, 88),
                             ("zngamd_kmer_counter_info", _lib.KmerCounterInfo, 64)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert [f[0] for f in _lib.KmerCounterInfo._fields_][:7] == ["k", "flags", "poisoned", "reserved", "cap", "distinct", "total"]
    # the totals are the key call's, then kmers, claimed, adds
    key_fields = [f[0] for f in _lib.BgzfKeyTotals._fields_]
    assert [f[0] for f in _lib.BgzfCountTotals._fields_] == key_fields + ["kmers", "claimed", "adds"]
    assert all(getattr(_lib.BgzfCountTotals, f).offset == getattr(_lib.BgzfKeyTotals, f).offset for f in key_fields) and _lib.BgzfCountTotals.kmers.offset == 64
    assert len(_lib.BgzfCountConf().reserved) == 12
    assert re.search(r"#define ZNGAMD_KMER_COUNTER_MAX_CAP\s+\(1ull << 33\)", header) and _lib.KMER_COUNTER_MAX_CAP == 1 << 33
    assert int(re.search(r"#define ZNGAMD_KMER_HIST_MAX_BINS\s+(\d+)u", header).group(1)) == _lib.KMER_HIST_MAX_BINS == 16384
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_kcount.hip"' in build
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_screen.hip"') < main.index('#include "za_kcount.hip"')
    kernel = open(os.path.join(PKG_DIR, "csrc", "za_kcount.hip")).read()
    for k in ("za_k_kcount_clear", "za_k_kcount_reads", "za_k_kcount_pairs", "za_k_kcount_export", "za_k_kcount_hist"):
        assert "void %s(" % k in kernel and k in main
    assert "za_k_rec_close<ZaKcountTotals>" in main[main.index("za_k_kcount_reads"):][:1000]      # the close kernel is the shared one, for these totals
    assert kernel.count("__shared__") == 1                                         # the histogram's bins, nothing else
    for fn in ("za_kmer_claim", "za_kmer_cut", "za_kmer_code", "za_kmer_planes"):
        assert fn + "(" in kernel and not re.search(r"__device__[^\n]*\b%s\(" % fn, kernel)      # used here, defined in za_screen.hip alone


def test_entry_points_refuse_without_a_context():
    """ctx / counter = NULL: ZNGAMD_E_ARG for every fault of the arguments -- and with everything in order -- and nothing is written"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    p = lambda a: C.c_void_p(a.ctypes.data)
    for k, flags, room, out in ((0, 1, 0, True), (32, 1, 0, True), (31, 2, 0, True), (31, 1, (1 << 32) + 1, True), (31, 1, (1 << 64) - 1, True),
                                (31, 1, 0, False), (31, 1, 100, True)):
        h = C.c_void_p(0x5A5A)
        assert L.zngamd_kmer_counter_new(None, k, flags, room, C.byref(h) if out else None) == E_ARG and h.value == 0x5A5A, (k, flags, room, out)
    codes, counts, hist, n = np.array([1, 2], np.uint64), np.array([1, 1], np.uint64), np.full(4, 0x5A, np.uint64), C.c_uint64(0x5A)
    info = _lib.KmerCounterInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    assert L.zngamd_kmer_counter_reserve(None, 0) == E_ARG and L.zngamd_kmer_counter_reserve(None, (1 << 64) - 1) == E_ARG
    assert L.zngamd_kmer_counter_add(None, p(codes), p(counts), 2) == E_ARG and L.zngamd_kmer_counter_add(None, None, None, 0) == E_ARG
    assert L.zngamd_kmer_counter_describe(None, C.byref(info)) == E_ARG and bytes(info) == b"\x5A" * 64
    for bins in (0, 1, 2, 4, 16384, 16385):
        assert L.zngamd_kmer_counter_histogram(None, p(hist), bins) == E_ARG
    for lo, hi in ((1, 0), (0, 0), (3, 2)):
        assert L.zngamd_kmer_counter_export(None, lo, hi, p(codes), p(counts), 2, C.byref(n)) == E_ARG
    assert L.zngamd_kmer_counter_export(None, 1, 0, p(codes), p(counts), 2, None) == E_ARG
    assert hist.tolist() == [0x5A] * 4 and n.value == 0x5A and codes.tolist() == [1, 2] and counts.tolist() == [1, 1]
    L.zngamd_kmer_counter_free(None)                                                 # nothing happens

    F = _lib.BGZF_GREP_FINAL

    def count(form, delim=10, flags=F, totals=True, with_conf=True, **fields):
        cf = _lib.BgzfCountConf(4, 1, 64, 0)
        for name, v in fields.items():
            if name == "reserved":
                cf.reserved[v] = 1
            else:
                setattr(cf, name, v)
        t = _lib.BgzfCountTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        head = (None, None, 0, None, 0, 0, 0, delim, flags, C.byref(cf) if with_conf else None, None, 0)      # (no context: no counter either)
        tail = (C.byref(t) if totals else None,)
        r = L.zngamd_bgzf_count_kmers(*head, None, *tail) if form == 0 else L.zngamd_bgzf_count_kmers_dev(*head, None, 0, None, *tail)
        assert bytes(t) == b"\x5A" * C.sizeof(t)                                    # a refused call writes nothing
        return r

    for form in range(2):
        for fields in (dict(record_lines=0), dict(record_lines=65), dict(seq_line=-1), dict(seq_line=4), dict(first_byte=-2), dict(first_byte=256),
                       dict(flags=1), dict(flags=1 << 31), dict(reserved=0), dict(reserved=11)):
            assert count(form, **fields) == E_ARG, (form, fields)
        for kw in (dict(delim=-1), dict(delim=256), dict(flags=F | 1), dict(flags=F | 2), dict(flags=F | 8), dict(flags=1 << 31), dict(totals=False),
                   dict(with_conf=False), dict()):
            assert count(form, **kw) == E_ARG, (form, kw)


def _hand_counts(bins=8):
    from zlib_ng_amd import bgzf
    codes, counts = [1, 6, 11], [2, 7, 1]
    return bgzf.KmerCounts(2, False, codes, counts, R.spectrum(dict(zip(codes, counts)), bins), records=3, bases=13)


def test_python_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    f = _Unreadable()
    for kw in (dict(k=0), dict(k=32), dict(k=21.0), dict(k=None), dict(canonical=1), dict(canonical=None), dict(max_table_bytes=-1), dict(max_table_bytes=1.5),
               dict(_room=-1), dict(_room=(1 << 32) + 1)):
        with pytest.raises(ValueError):
            bgzf.KmerCounter(**kw)
    bad = (dict(seq_line=4), dict(seq_line=-1), dict(seq_line=1.0), dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(record_lines=0), dict(record_lines=65),
           dict(max_record=0))
    for kw in bad:
        kc = bgzf.KmerCounter(21)
        with pytest.raises(ValueError):
            kc.add_file(f, **kw)
        with pytest.raises(ValueError):
            bgzf.count_kmers(f, 21, **{k: v for k, v in kw.items()})
        if "max_record" not in kw:
            with pytest.raises(ValueError):
                kc.add_file("/nonexistent/reads.fq.gz", **kw)                           # (judged before a file is opened)
            with pytest.raises(ValueError):
                bgzf.count_kmers(["/nonexistent/r1.fq.gz", "/nonexistent/r2.fq.gz"], **kw)
        assert kc._table is None and not kc._broken                                    # nothing was made, nothing is lost
    for kw in (dict(min_count=0), dict(min_count=-1), dict(min_count=1.0), dict(max_count=0), dict(min_count=3, max_count=2), dict(bins=1), dict(bins=16385),
               dict(bins=None), dict(bins=10.0)):
        with pytest.raises(ValueError):
            bgzf.count_kmers("/nonexistent/reads.fq.gz", 21, **kw)
        with pytest.raises(ValueError):
            bgzf.KmerCounter(21).result(**kw)
    for kw in (dict(k=0), dict(k=32), dict(canonical="yes")):
        with pytest.raises(ValueError):
            bgzf.count_kmers("/nonexistent/reads.fq.gz", **kw)
    kc = bgzf.KmerCounter(2, False)
    for not_counts in (None, {1: 2}, bgzf.KmerCounts(3, False, [1], [2], [0, 0, 1]), bgzf.KmerCounts(2, True, [1], [2], [0, 0, 1]),
                       bgzf.KmerCounts(2, False, [1], [2], [0, 0, 1], min_count=2, kmers=9), bgzf.KmerCounts(2, False, [], [], [0, 0, 1], min_count=None, kmers=9)):
        with pytest.raises(ValueError, match="add_counts takes unfiltered KmerCounts"):
            kc.add_counts(not_counts)
    kc.close()
    for use in (lambda: kc.add_file(f), kc.result, lambda: kc.add_counts(_hand_counts())):
        with pytest.raises(ValueError, match="closed"):
            use()
    kc.close()                                                                     # (twice is once)
    cf, d = bgzf._count_conf(4, np.int64(1), b"@", b"\n")
    assert (cf.record_lines, cf.seq_line, cf.first_byte, cf.flags, list(cf.reserved), d) == (4, 1, 64, 0, [0] * 12, b"\n")
    cf, d = bgzf._count_conf(2, 0, None, b";")
    assert (cf.seq_line, cf.first_byte, d) == (0, -1, b";")
    for name in ("KmerCounter", "KmerCounts", "count_kmers"):
        assert name in bgzf.__all__
    rec_kw = ["first_byte", "delimiter", "start", "stop", "first_record", "max_record", "allow_short"]
    sig = inspect.signature(bgzf.KmerCounter.add_file).parameters
    assert list(sig)[:4] == ["self", "file", "record_lines", "seq_line"] and [p for p in list(sig)[4:] if not p.startswith("_")] == rec_kw
    defaults = {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty and not k.startswith("_")}
    assert defaults == dict(record_lines=4, seq_line=1, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20,
                            allow_short=False)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.items() if k not in ("self", "file", "record_lines"))
    sig = inspect.signature(bgzf.KmerCounter.__init__).parameters
    assert (sig["k"].default, sig["canonical"].default, sig["max_table_bytes"].default) == (31, True, None)
    assert sig["max_table_bytes"].kind is inspect.Parameter.KEYWORD_ONLY and sig["_room"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(bgzf.KmerCounter.result).parameters
    assert {k: v.default for k, v in sig.items() if k != "self"} == dict(min_count=1, max_count=None, bins=10001)
    sig = inspect.signature(bgzf.count_kmers).parameters
    assert list(sig)[:2] == ["file_or_files", "k"] and (sig["k"].default, sig["canonical"].default, sig["min_count"].default, sig["max_count"].default,
                                                       sig["bins"].default) == (31, True, 1, None, 10001)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.items() if k not in ("file_or_files", "k"))
    assert "_KmerCountSink" in bgzf._grep_file.__doc__


def test_kmer_counts_on_arrays_written_by_hand(tmp_path):
    from zlib_ng_amd import bgzf
    a = _hand_counts()
    assert (a.k, a.canonical, a.min_count, a.max_count, a.records, a.bases, a.kmers, a.distinct, len(a), a.bins) == (2, False, 1, None, 3, 13, 10, 3, 3, 8)
    assert a.codes.dtype == a.counts.dtype == a.spectrum.dtype == np.uint64 and a.spectrum.tolist() == [0, 1, 1, 0, 0, 0, 0, 1] and a.unfiltered
    assert a.kmer_bytes() == [b"AC", b"CG", b"GT"]
    # count_of: strings by the rule, codes as they are, what is not held is 0
    assert a.count_of(b"AC") == 2 and a.count_of("cg") == 7 and a.count_of(11) == 1 and a.count_of(b"TT") == 0 and a.count_of(15) == 0
    assert a.count_of([b"GU", "AC", 6, 0, 12]).tolist() == [1, 2, 7, 0, 0] and a.count_of([]).tolist() == [] and a.count_of([b"GT"]).dtype == np.uint64
    for bad in (b"ACG", b"A", b"AN", "A-"):
        with pytest.raises(ValueError):
            a.count_of(bad)
    canon = bgzf.KmerCounts(2, True, [1, 6], [3, 7], [0, 0, 0, 1, 0, 0, 0, 1])
    assert canon.count_of([b"AC", b"GT", b"CG"]).tolist() == [3, 3, 7]                # GT is AC read backwards
    # most_common: the largest first, equal counts by ascending code
    ties = bgzf.KmerCounts(2, False, [0, 3, 5, 9, 15], [4, 9, 4, 9, 1], R.spectrum({0: 4, 3: 9, 5: 4, 9: 9, 15: 1}, 5))
    assert ties.most_common(3) == [(b"AT", 9), (b"GC", 9), (b"AA", 4)] and ties.most_common() == [(b"AT", 9), (b"GC", 9), (b"AA", 4), (b"CC", 4), (b"TT", 1)]
    assert ties.most_common(0) == [] and ties.spectrum.tolist() == [0, 1, 0, 0, 4]
    # to_kmerset: one reference, the filter on the counts
    s = a.to_kmerset()
    assert isinstance(s, bgzf.KmerSet) and (s.k, s.canonical, s.names, s.n_refs) == (2, False, ("counted",), 1) and s.codes.tolist() == [1, 6, 11]
    assert s.masks.tolist() == [1, 1, 1] and a.to_kmerset(2).codes.tolist() == [1, 6] and a.to_kmerset(2, 6, name="solid").codes.tolist() == [1]
    assert a.to_kmerset(2, 6, name="solid").names == ("solid",) and len(a.to_kmerset(8)) == 0
    for kw in (dict(min_count=0), dict(min_count=None), dict(min_count=3, max_count=2)):
        with pytest.raises(ValueError):
            a.to_kmerset(**kw)
    # a + b: counts, spectra and totals; the last bin comes from the merged counts
    b = bgzf.KmerCounts(2, False, [6, 15], [5, 6], [0, 0, 0, 0, 0, 1, 1, 0], records=2, bases=20)
    c = a + b
    assert c.codes.tolist() == [1, 6, 11, 15] and c.counts.tolist() == [2, 12, 1, 6] and (c.records, c.bases, c.kmers, c.distinct) == (5, 33, 21, 4)
    assert c.spectrum.tolist() == [0, 1, 1, 0, 0, 0, 1, 1] == R.spectrum({1: 2, 6: 12, 11: 1, 15: 6}, 8) and (b + a) == c and a.codes.tolist() == [1, 6, 11]
    small = bgzf.KmerCounts(2, False, [6], [3], [0, 0, 0, 1]) + bgzf.KmerCounts(2, False, [6, 7], [2, 2], [0, 0, 2, 0])
    assert small.spectrum.tolist() == [0, 0, 1, 1] and small.counts.tolist() == [5, 2]      # 3 + 2 = 5 lies in the last bin, >= 3; not [0, 0, 2, 1]
    empty = bgzf.KmerCounts(2, False, [], [], [0] * 8)
    assert (a + empty) == a and (empty + empty) == empty and len(empty) == 0 and empty.kmers == 0
    for other in (bgzf.KmerCounts(3, False, [1], [2], [0, 0, 1, 0, 0, 0, 0, 0]), bgzf.KmerCounts(2, True, [1], [2], [0, 0, 1, 0, 0, 0, 0, 0])):
        with pytest.raises(ValueError, match="different k or canonical"):
            a + other
    for other in (bgzf.KmerCounts(2, False, [1], [2], [0, 0, 1]), bgzf.KmerCounts(2, False, [6], [7], a.spectrum, min_count=3, kmers=10),
                  bgzf.KmerCounts(2, False, [1, 11], [2, 1], a.spectrum, max_count=6, kmers=10), bgzf.KmerCounts(2, False, [], [], a.spectrum, min_count=None, kmers=10)):
        with pytest.raises(ValueError, match="only unfiltered k-mer counts of equal bins add"):
            a + other
        with pytest.raises(ValueError, match="only unfiltered"):
            other + a
    with pytest.raises(TypeError):
        a + 1
    # what the constructor refuses
    for args, kw in (((2, False, [16], [1], [0, 1]), {}), ((2, False, [1], [0], [0, 1]), {}), ((2, False, [6, 1], [1, 1], [0, 2]), {}), ((2, False, [1, 1], [1, 1], [0, 2]), {}),
                     ((2, False, [1], [1, 2], [0, 1]), {}), ((2, False, [1], [1], [1, 1]), {}), ((2, False, [1], [1], [0]), {}), ((2, False, [1], [1], [0, 2]), {}),
                     ((2, False, [1], [1], [0, 1]), dict(kmers=2)), ((2, False, [1], [1], [0, 1]), dict(distinct=2)), ((2, False, [1], [5], [0, 1]), dict(min_count=6)),
                     ((2, False, [1], [5], [0, 1]), dict(max_count=4)), ((2, False, [1], [5], [0, 1]), dict(min_count=None)), ((0, False, [], [], [0, 0]), {}),
                     ((2, 1, [], [], [0, 0]), {}), ((2, False, [-1], [1], [0, 1]), {}), ((2, False, [1.5], [1], [0, 1]), {}), ((2, False, [[1]], [[1]], [0, 1]), {}),
                     ((2, False, [1], [1], [0] * 16385), {})):
        with pytest.raises(ValueError):
            bgzf.KmerCounts(*args, **kw)
    # save and load, judged on load as the constructor judges
    path = str(tmp_path / "counts.npz")
    for x in (c, empty, bgzf.KmerCounts(2, False, [6], [7], a.spectrum, min_count=3, max_count=8, records=3, bases=13, kmers=10),
              bgzf.KmerCounts(31, True, [4 ** 31 - 1], [2 ** 64 - 1], [0, 1], records=1, bases=31),
              bgzf.KmerCounts(2, False, [], [], a.spectrum, min_count=None, records=3, bases=13, kmers=10)):
        x.save(path)
        back = bgzf.KmerCounts.load(path)
        assert back == x and (back.min_count, back.max_count, back.records, back.bases, back.kmers, back.distinct) == \
            (x.min_count, x.max_count, x.records, x.bases, x.kmers, x.distinct) and back.codes.dtype == np.uint64
    np.savez(path, k=np.int64(2), canonical=np.bool_(False), codes=np.array([6, 1], np.uint64), counts=np.array([1, 1], np.uint64), spectrum=np.array([0, 2], np.uint64),
             filter=np.array([1, 0], np.uint64), totals=np.array([1, 4, 2, 2], np.uint64))
    with pytest.raises(ValueError, match="ascend"):
        bgzf.KmerCounts.load(path)
    assert c != a and a != "a" and repr(a) == "<KmerCounts: k = 2, 3 codes of 10 k-mers in 3 records, 3 pairs (count >= 1)>"
    with pytest.raises(TypeError):
        hash(a)


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
    exe = str(tmp_path / "kcount_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "kcount_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf count arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

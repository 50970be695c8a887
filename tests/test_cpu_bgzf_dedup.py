"""CPU: BGZF duplicate removal, without a GPU -- the referee of dedup_ref.py against keys worked out by hand; for every input of the GPU
tests, the referee's keys group the records exactly as their bytes do (what keeps a collision from hiding behind the referee); the
argument checks that need no context; the new entry points are declared, exported and bound, and refuse hostile arguments with no
context at all; KeyResult's sum, pair_keys and DedupResult on arrays written by hand; and tests/dedup_args.cpp, a stand-alone program,
against the library's host side under AddressSanitizer + UndefinedBehaviorSanitizer (a plain child process, nothing preloaded)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import dedup_inputs as I
import dedup_ref
from conftest import PKG_DIR, ROOT
from dedup_ref import M, S, mix
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang


def test_referee_against_keys_worked_out_by_hand():
    # the mixer, step by step in Python integers
    def mix_by_hand(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ x >> 30) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ x >> 27) * 0x94D049BB133111EB) & M
        return x ^ x >> 31
    for x in (0, 1, M, S[0], S[1], 1 << 63, 0x0123456789ABCDEF):
        assert mix(x) == mix_by_hand(x)
    assert mix(0) == 0xE220A8397B1DCDAF                                            # splitmix64's first output for the seed 0
    cf = dedup_ref.conf()
    # the empty part: the length term alone; a body shorter than `first`
    empty = tuple(mix_by_hand(s ^ 1 << 63) for s in S)
    assert dedup_ref.key(b"", cf) == empty == dedup_ref.key(b"ACG", cf._replace(first=3)) == dedup_ref.key(b"ACG", cf._replace(first=200, length=5))
    # one byte: the length term and the term of (0, 'A')
    one = tuple((mix_by_hand(s ^ (1 << 63 | 1)) + mix_by_hand(s ^ 65)) & M for s in S)
    assert dedup_ref.key(b"A", cf) == one == dedup_ref.key(b"GAT", cf._replace(first=1, length=1)) == dedup_ref.key(b"a", cf._replace(ignore_case=True))
    assert dedup_ref.key(b"a", cf) == tuple((mix_by_hand(s ^ (1 << 63 | 1)) + mix_by_hand(s ^ 97)) & M for s in S) != one
    # two bytes: the position counts
    two = tuple((mix_by_hand(s ^ (1 << 63 | 2)) + mix_by_hand(s ^ 67) + mix_by_hand(s ^ (1 << 8 | 71))) & M for s in S)
    assert dedup_ref.key(b"CG", cf) == two != dedup_ref.key(b"GC", cf)
    assert dedup_ref.key(b"ACGTAC", cf._replace(first=1, length=2)) == two and dedup_ref.key(b"ACG", cf._replace(first=1, length=9)) == two
    # a read and its reverse complement share a canonical key, which is the smaller of their two plain keys as hi << 64 | lo
    ca = cf._replace(canonical=True)
    read, back = b"AACGTTTGNu", b"aNCAAACGTT"
    assert I.rc(read) == back and I.rc(back) == b"AACGTTTGNt"                      # (U -> A: the way back is not the way there)
    k, r = dedup_ref.key(read, cf), dedup_ref.key(back, cf)
    assert k != r and dedup_ref.key(read, ca) == min(k, r, key=lambda w: w[1] << 64 | w[0])
    plain, plain_rc = b"AACGTTTGNC", b"GNCAAACGTT"
    assert dedup_ref.key(plain, ca) == dedup_ref.key(plain_rc, ca) and dedup_ref.key(plain, cf) != dedup_ref.key(plain_rc, cf)
    assert dedup_ref.key(plain, ca) in (dedup_ref.key(plain, cf), dedup_ref.key(plain_rc, cf))
    # a palindrome is its own reverse complement: canonical changes nothing
    assert I.rc(b"ACGCGT") == b"ACGCGT" and dedup_ref.key(b"ACGCGT", ca) == dedup_ref.key(b"ACGCGT", cf)
    # every other byte is its own complement; the fold comes first
    assert I.rc(b"N.R-") == b"-R.N" and dedup_ref.key(b"acgu", ca._replace(ignore_case=True)) == dedup_ref.key(b"ACGU", ca)
    # the resolve and the bytes
    r = dedup_ref.resolve([(1, 2), (1, 3), (1, 2), (9, 9), (1, 3), (1, 2)])
    assert r == ([0, 1, 0, 3, 1, 0], [3, 2, 0, 1, 0, 0], 3, 3, 3, 0)
    assert dedup_ref.resolve([]) == ([], [], 0, 0, 0, 0) and dedup_ref.resolve([(5, 5), (6, 6), (6, 6), (5, 5)]).max_first == 0
    e = dedup_ref.exact([b"ACGT", b"acgt", b"ACGT", b"ACGA", b"TCGT"], cf)
    assert e.first == [0, 1, 0, 3, 4] and e.count == [2, 1, 0, 1, 1]
    assert dedup_ref.exact([b"ACGT", b"acgt", b"ACGA", b"TCGT"], cf._replace(ignore_case=True)).first == [0, 0, 2, 3]
    assert dedup_ref.exact([b"ACGA", b"TCGT", b"ACGA"], ca).first == [0, 0, 0] and dedup_ref.exact([b"ACGA", b"TCGT"], cf._replace(length=2, first=1)).first == [0, 0]
    with pytest.raises(ValueError):
        dedup_ref.exact([b"ACGU"], ca)
    assert dedup_ref.no_collision([b"U", b"A", b"T", b"A"], dedup_ref.keys([b"U", b"A", b"T", b"A"], ca), ca)
    with pytest.raises(AssertionError, match="share a key"):
        dedup_ref.no_collision([b"AC", b"AG"], np.array([[1, 2], [1, 2]], np.uint64), ca)
    with pytest.raises(AssertionError, match="two keys"):
        dedup_ref.no_collision([b"AC", b"GT"], np.array([[1, 2], [1, 3]], np.uint64), ca)
    bodies, nbytes, consumed = dedup_ref.bodies_of(b"@a\nAC\n+\nII\n@s\nG", cf)
    assert (bodies, nbytes, consumed) == ([b"AC", b"G"], 15, 15) and dedup_ref.bodies_of(b"@a\nAC\n+\nII\n@s\nG", cf, final=False)[::2] == ([b"AC"], 11)
    with pytest.raises(dedup_ref.Fault):
        dedup_ref.bodies_of(b"@a\nAC\n+\nII\nxs\nG\n+\nI\n", cf._replace(first_byte=b"@"))


@pytest.mark.parametrize("name", [n for n, _, _ in I.with_bodies()])
def test_no_collision_hides_behind_the_referee(name):
    """for every input the GPU tests key, and every configuration: the dict walk over the referee's keys == the comparison of the bytes"""
    bodies, confs = {n: (b, c) for n, b, c in I.with_bodies()}[name]
    assert len(bodies) >= 700
    found = {}
    for cf in confs:
        k = dedup_ref.keys(bodies, cf)
        found[cf] = dedup_ref.resolve(k).duplicates
        if cf.canonical and name == "grid":
            # the grid's reads hold U and u, where the complement is no involution (U -> A -> T): the bytes say which records may and
            # which must share a key, and the GPU test compares these keys word for word and groups nothing by them
            with pytest.raises(ValueError):
                dedup_ref.exact(bodies, cf)
            assert dedup_ref.no_collision(bodies, k, cf)
        else:
            assert dedup_ref.resolve(k) == dedup_ref.exact(bodies, cf), cf
            assert dedup_ref.no_collision(bodies, k, cf)
    if name == "grid":                                                             # the options matter on this input: each finds other duplicates
        plain = dedup_ref.conf()
        assert 0 < found[plain] < found[plain._replace(ignore_case=True)] < found[plain._replace(ignore_case=True, canonical=True)]
        assert found[plain] < found[plain._replace(canonical=True)] and found[plain] < found[plain._replace(length=50)] < found[plain._replace(first=200)]


def test_paired_inputs_group_as_their_bytes_do():
    r1, r2 = I.paired_bodies()
    cf = dedup_ref.conf()
    pairs = dedup_ref.pair(dedup_ref.keys(r1, cf), dedup_ref.keys(r2, cf))
    assert dedup_ref.resolve(pairs) == dedup_ref.walk(list(zip(r1, r2)))


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    f = _Unreadable()
    bad = (dict(seq_line=4), dict(seq_line=-1), dict(first=-1), dict(first=1 << 32), dict(first=1.0), dict(length=-1), dict(length=1 << 32), dict(length=None),
           dict(ignore_case=1), dict(canonical="yes"), dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(record_lines=0), dict(record_lines=65), dict(max_record=0))
    for kw in bad:
        with pytest.raises(ValueError):
            bgzf.key_records(f, **kw)
        with pytest.raises(ValueError):
            bgzf.dedup_records(f, None, **kw)
        if "max_record" not in kw:
            with pytest.raises(ValueError):
                bgzf.dedup_paired(["/nonexistent/r1.fq.gz", "/nonexistent/r2.fq.gz"], None, **kw)      # (judged before a file is opened)
            with pytest.raises(ValueError):
                bgzf.key_records("/nonexistent/reads.fq.gz", **kw)
            with pytest.raises(ValueError):
                bgzf.dedup_records("/nonexistent/reads.fq.gz", "/nonexistent/out.gz", **kw)
    with pytest.raises(ValueError, match="first is an integer between 0 and 4294967295, not -1"):
        bgzf.key_records(f, first=-1)
    for kw in (dict(qual_line=3), dict(patterns=[b"A"]), dict(cycles=4)):
        with pytest.raises(TypeError):
            bgzf.key_records(f, **kw)
    with pytest.raises(ValueError, match="block_size"):
        bgzf.dedup_records("/nonexistent/reads.fq.gz", "/nonexistent/out.gz", block_size=0)
    with pytest.raises(ValueError, match="the two files of a paired run, not 3"):
        bgzf.dedup_paired(["a", "b", "c"], None)
    with pytest.raises(ValueError, match="one entry per file"):
        bgzf.dedup_paired(["/nonexistent/a", "/nonexistent/b"], ["x"])
    with pytest.raises(ValueError, match="one entry per file"):
        bgzf.dedup_paired(["/nonexistent/a", "/nonexistent/b"], None, duplicates=["x"])
    for keys in (np.zeros(3, np.uint64), np.zeros((3, 3), np.uint64), np.zeros((3, 2), np.int64), [1, 2, 3], "keys"):
        with pytest.raises(ValueError, match="keys is a KeyResult"):
            bgzf.dedup_keys(keys)
    cf, d, opt = bgzf._key_conf(4, 1, np.int64(3), 50, True, np.True_, b"@", b"\n")
    assert (cf.record_lines, cf.seq_line, cf.first_byte, cf.first, cf.length, cf.flags, list(cf.reserved), d) == \
        (4, 1, 64, 3, 50, _lib.BGZF_KEY_IGNORE_CASE | _lib.BGZF_KEY_CANONICAL, [0] * 10, b"\n")
    assert opt == dict(first=3, length=50, ignore_case=True, canonical=True)
    cf, d, opt = bgzf._key_conf(2, 0, 0, 0, False, False, None, b";")
    assert (cf.seq_line, cf.first_byte, cf.flags, d) == (0, -1, 0, b";")
    for name in ("key_records", "KeyResult", "pair_keys", "dedup_keys", "DedupResult", "dedup_records", "dedup_paired"):
        assert name in bgzf.__all__
    key_kw = ["seq_line", "first", "length", "ignore_case", "canonical"]
    rec_kw = ["first_byte", "delimiter", "start", "stop", "first_record", "max_record", "allow_short"]
    sig = inspect.signature(bgzf.key_records).parameters
    assert list(sig) == ["file", "record_lines"] + key_kw + rec_kw
    assert list(inspect.signature(bgzf.BgzfReader.key_records).parameters) == ["self", "record_lines"] + key_kw + rec_kw
    defaults = {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(record_lines=4, seq_line=1, first=0, length=0, ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n", start=None,
                            stop=None, first_record=0, max_record=64 << 20, allow_short=False)
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in sig.items() if k not in ("file", "record_lines"))
    out_kw = ["duplicates", "compresslevel", "block_size"]
    sig = inspect.signature(bgzf.dedup_records).parameters
    assert list(sig) == ["file", "output", "record_lines"] + out_kw + key_kw + rec_kw
    assert list(inspect.signature(bgzf.BgzfReader.dedup_records).parameters) == ["self", "output", "record_lines"] + out_kw + key_kw + rec_kw
    assert list(inspect.signature(bgzf.dedup_paired).parameters) == ["files", "outputs", "record_lines"] + out_kw + key_kw + rec_kw
    assert (sig["duplicates"].default, sig["compresslevel"].default, sig["block_size"].default) == (None, 6, bgzf.MAX_BLOCK_INPUT)
    for text in (bgzf.key_records.__doc__, bgzf.dedup_keys.__doc__, bgzf.dedup_records.__doc__):
        assert "Equal keys are treated as equal sequences" in text


def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, header).group(1)
    return [re.sub(r"\[.*", "", x) for x in re.findall(r"\b(\w+(?:\[\w+\])?);", re.sub(r"/\*.*?\*/", "", body))]


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib, bgzf
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32, "zngamd_alloc_fn": _lib.ALLOC_FN}

    def params_of(name, ret="int"):
        return [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\b%s %s\s*\(([^;]*)\);" % (ret, name), header).group(1).split(",")]

    for name in ("zngamd_bgzf_key_records_dev", "zngamd_bgzf_key_records", "zngamd_dedup_keys_dev", "zngamd_dedup_keys"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        params = params_of(name)
        want = [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params]
        assert getattr(L, name).argtypes == want, name
    for name in ("zngamd_bgzf_key_records_dev", "zngamd_bgzf_key_records"):
        params = params_of(name)
        assert "const zngamd_bgzf_key_conf *conf" in params and params[-1] == "zngamd_bgzf_key_totals *totals"
        assert params[:11] == params_of(name.replace("key", "qc"))[:11][:9] + ["const zngamd_bgzf_key_conf *conf", "uint64_t record_base"]      # the window of qc
    assert params_of("zngamd_dedup_keys_dev") == ["zngamd_ctx *ctx", "const zngamd_bgzf_key_row *d_keys", "uint64_t n", "void *d_scratch", "uint64_t scratch_cap",
                                                  "uint64_t *d_first", "uint32_t *d_count", "zngamd_dedup_totals *totals"]
    assert "zngamd_dedup_scratch_bytes" in _lib.SYMBOLS and params_of("zngamd_dedup_scratch_bytes", "uint64_t") == ["uint64_t n"]
    assert L.zngamd_dedup_scratch_bytes.restype is C.c_uint64 and L.zngamd_dedup_scratch_bytes.argtypes == [C.c_uint64]
    for n, cap in ((0, 64), (1, 64), (32, 64), (33, 128), (4096, 8192), (4097, 16384), (1 << 30, 1 << 31)):
        assert L.zngamd_dedup_scratch_bytes(n) == 12 * cap + 64, n
    assert L.zngamd_dedup_scratch_bytes((1 << 30) + 1) == 0
    for struct, ct, size in (("zngamd_bgzf_key_conf", _lib.BgzfKeyConf, 64), ("zngamd_bgzf_key_totals", _lib.BgzfKeyTotals, 64),
                             ("zngamd_dedup_totals", _lib.DedupTotals, 48)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert int(re.search(r"\}\s*zngamd_bgzf_key_row;\s*/\* (\d+) B \*/", header).group(1)) == _lib.KEY_ROW_DTYPE.itemsize == 16
    assert _struct_fields(header, "zngamd_bgzf_key_row") == list(_lib.KEY_ROW_DTYPE.names) == ["lo", "hi"]
    assert _lib.BgzfKeyTotals.tail_off.offset == 24 and _lib.BgzfKeyTotals.covered.offset == 48 and _lib.BgzfKeyTotals.bad.offset == 56
    for macro, value in (("KEY_IGNORE_CASE", _lib.BGZF_KEY_IGNORE_CASE), ("KEY_CANONICAL", _lib.BGZF_KEY_CANONICAL)):
        assert int(re.search(r"#define ZNGAMD_BGZF_%s\s+(\d+)u" % macro, header).group(1)) == value
    # the seeds stand in the header, and the referee, the bindings and the kernel file hold the same two
    seeds = tuple(int(re.search(r"#define ZNGAMD_BGZF_KEY_SEED%d\s+(0x[0-9A-Fa-f]+)ull" % w, header).group(1), 16) for w in range(2))
    assert seeds == S == (_lib.BGZF_KEY_SEED0, _lib.BGZF_KEY_SEED1) and S[0] != S[1]
    kernel = open(os.path.join(PKG_DIR, "csrc", "za_dedup.hip")).read()
    assert tuple(int(re.search(r"#define ZA_KEY_SEED%d\s+(0x[0-9A-Fa-f]+)ull" % w, kernel).group(1), 16) for w in range(2)) == S
    assert re.search(r"#define ZNGAMD_DEDUP_MAX_KEYS\s+\(1ull << 30\)", header) and _lib.DEDUP_MAX_KEYS == 1 << 30
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_dedup.hip"' in build
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_qc.hip"') < main.index('#include "za_dedup.hip"')
    for k in ("za_k_dedup_keys", "za_k_dedup_insert", "za_k_dedup_lookup", "za_k_dedup_close"):
        assert "void %s(" % k in kernel and k in main
    assert "__shared__" not in kernel                                              # no LDS tables
    # the mixer of pair_keys is the referee's
    x = np.array([0, 1, M, S[0], 1 << 63], np.uint64)
    assert np.array_equal(bgzf._mix64(x), mix(x))


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every hostile configuration, delimiter, flag, count and NULL pointer -- and with everything in order"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    F = _lib.BGZF_GREP_FINAL

    def call(form, delim=10, flags=F, totals=True, with_conf=True, rows=True, alloc=False, **fields):
        cf = _lib.BgzfKeyConf(4, 1, 64, 3, 50, 3)
        for k, v in fields.items():
            if k == "reserved":
                cf.reserved[v] = 1
            else:
                setattr(cf, k, v)
        t = _lib.BgzfKeyTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        row = np.zeros(1, _lib.KEY_ROW_DTYPE)
        rp = C.c_void_p(row.ctypes.data) if rows else None
        head = (None, None, 0, None, 0, 0, 0, delim, flags, C.byref(cf) if with_conf else None, 0)
        tail = (C.byref(t) if totals else None,)
        if form == 0:
            fn = _lib.ALLOC_FN(lambda user, n: pytest.fail("the allocator was called")) if alloc else _lib.ALLOC_FN()
            r = L.zngamd_bgzf_key_records(*head, None, rp, 0, fn, None, *tail)
        else:
            r = L.zngamd_bgzf_key_records_dev(*head, None, 0, None, rp, 0, *tail)
        assert bytes(t) == b"\x5A" * C.sizeof(t) and not row["lo"][0] and not row["hi"][0]      # a refused call writes nothing
        return r

    for form in range(2):
        for fields in (dict(record_lines=0), dict(record_lines=65), dict(seq_line=-1), dict(seq_line=4), dict(first_byte=-2), dict(first_byte=256), dict(flags=4),
                       dict(flags=7), dict(flags=1 << 31), dict(reserved=0), dict(reserved=9)):
            assert call(form, **fields) == E_ARG, (form, fields)
        for kw in (dict(delim=-1), dict(delim=256), dict(flags=F | 1), dict(flags=F | 2), dict(flags=F | 8), dict(flags=F | 16), dict(flags=1 << 31),
                   dict(totals=False), dict(with_conf=False), dict(rows=False)):
            assert call(form, **kw) == E_ARG, (form, kw)
        assert call(form) == E_ARG                                                         # in order, but no context
        assert call(form, first=0xFFFFFFFF, length=0xFFFFFFFF) == E_ARG
    assert call(0, rows=False, alloc=True) == E_ARG

    def resolve(form, keys=True, n=1, totals=True, scratch=True):
        t = _lib.DedupTotals()
        C.memset(C.byref(t), 0x5A, C.sizeof(t))
        key, first, count, area = np.zeros(1, _lib.KEY_ROW_DTYPE), np.full(1, 7, np.uint64), np.full(1, 7, np.uint32), np.full(8, 7, np.uint64)
        p = lambda a, on=True: C.c_void_p(a.ctypes.data) if on else None
        if form == 0:
            r = L.zngamd_dedup_keys(None, p(key, keys), n, p(first), p(count), C.byref(t) if totals else None)
        else:
            r = L.zngamd_dedup_keys_dev(None, p(key, keys), n, p(area, scratch), 64, p(first), p(count), C.byref(t) if totals else None)
        assert bytes(t) == b"\x5A" * C.sizeof(t) and first[0] == count[0] == 7 and (area == 7).all()
        return r

    for form in range(2):
        for kw in (dict(keys=False), dict(n=(1 << 30) + 1), dict(n=(1 << 64) - 1), dict(totals=False), dict(), dict(keys=False, n=0)):
            assert resolve(form, **kw) == E_ARG, (form, kw)
    assert resolve(1, scratch=False) == E_ARG


def _keys(pairs):
    from zlib_ng_amd import _lib
    return np.array(pairs, np.uint64).reshape(-1, 2).copy().view(_lib.KEY_ROW_DTYPE).reshape(-1)


def test_key_result_and_pair_keys():
    from zlib_ng_amd import bgzf
    opt = dict(first=0, length=0, ignore_case=False, canonical=True)
    a, b = bgzf.KeyResult(_keys([(1, 2), (3, 4)]), 10, opt), bgzf.KeyResult(_keys([(5, 6)]), 7, opt)
    s = a + b
    assert (s.records, len(s), s.bases, s.options) == (3, 3, 17, opt) and s.keys.tolist() == [(1, 2), (3, 4), (5, 6)] and s.canonical and not s.ignore_case
    assert (a.records, b.records) == (2, 1) and (b + a).keys.tolist() == [(5, 6), (1, 2), (3, 4)]      # (the parts are left as they were)
    empty = bgzf.KeyResult(_keys([]), 0, opt)
    assert (empty + a).keys.tolist() == a.keys.tolist() and (empty + empty).records == 0
    for other in (dict(opt, length=50), dict(opt, canonical=False), dict(opt, first=1), dict(opt, ignore_case=True)):
        with pytest.raises(ValueError, match="not comparable"):
            a + bgzf.KeyResult(_keys([(5, 6)]), 7, other)
    with pytest.raises(TypeError):
        a + 1
    assert repr(s) == "<KeyResult: 3 records, 17 bases>"
    # pairs: equal pairs get equal keys; the order of the mates counts; every one of the four words counts
    x = bgzf.KeyResult(_keys([(1, 2), (3, 4), (1, 2), (3, 4), (1, 2), (1, 2), (1, 2)]), 70, opt)
    y = bgzf.KeyResult(_keys([(3, 4), (1, 2), (3, 4), (3, 4), (3, 5), (4, 4), (3, 4)]), 70, opt)
    p = bgzf.pair_keys(x, y)
    assert isinstance(p, bgzf.KeyResult) and p.records == 7 and p.bases == 140 and p.options == opt
    k = p.keys.tolist()
    assert k[0] == k[2] == k[6] and len(set(k)) == 5 and k[0] != k[1]              # (x, y) and (y, x) differ
    flat = lambda r: np.stack([r.keys["lo"], r.keys["hi"]], axis=1)
    assert np.array_equal(flat(p), dedup_ref.pair(flat(x), flat(y)))
    assert bgzf.pair_keys(y, x).keys.tolist()[0] == k[1]
    w0 = mix(mix(mix(mix(S[0] ^ 1) ^ 2) ^ 3) ^ 4)
    assert k[0] == (w0, mix(mix(mix(mix(S[1] ^ 1) ^ 2) ^ 3) ^ 4))
    arrays = bgzf.pair_keys(x.keys, flat(y))                                       # arrays in, an array out
    assert isinstance(arrays, np.ndarray) and arrays.tolist() == k
    with pytest.raises(ValueError, match="hold 7 and 2 records"):
        bgzf.pair_keys(x, a)
    with pytest.raises(ValueError, match="not comparable"):
        bgzf.pair_keys(x, bgzf.KeyResult(y.keys, 70, dict(opt, canonical=False)))


def test_dedup_result_on_arrays_written_by_hand():
    from zlib_ng_amd import bgzf
    #        record: 0  1  2  3  4  5  6  7  8  9
    first = np.array([0, 1, 0, 3, 1, 0, 6, 1, 1, 9], np.int64)
    count = np.array([3, 4, 0, 1, 0, 0, 1, 0, 0, 1], np.int64)
    r = bgzf.DedupResult(first, count, 5, 4, 1)
    assert (r.records, len(r), r.unique, r.duplicates, r.max_count, r.max_first, r.duplication_rate) == (10, 10, 5, 5, 4, 1, 0.5)
    assert r.duplicate.tolist() == [False, False, True, False, True, True, False, True, True, False]
    assert r.drop().dtype == np.uint8 and r.drop().tolist() == [0, 0, 1, 0, 1, 1, 0, 1, 1, 0]
    assert r.labels().dtype == np.int64 and r.labels().tolist() == [0, 0, 1, 0, 1, 1, 0, 1, 1, 0]
    assert r.labels(bgzf.DROP).tolist() == [0, 0, -1, 0, -1, -1, 0, -1, -1, 0] and r.labels(5).max() == 5
    idx, cnt = r.most_common(2)
    assert idx.tolist() == [1, 0] and cnt.tolist() == [4, 3]
    idx, cnt = r.most_common(99)
    assert idx.tolist() == [1, 0, 3, 6, 9] and cnt.tolist() == [4, 3, 1, 1, 1]     # the earlier record first among equals
    assert r.most_common(0)[0].tolist() == []
    distinct, reads = r.levels()
    assert len(distinct) == len(reads) == len(bgzf.DEDUP_LEVELS) == 16 and bgzf.DEDUP_LEVELS[:11] == (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50)
    assert distinct.tolist() == [3, 0, 1, 1] + [0] * 12 and reads.tolist() == [3, 0, 3, 4] + [0] * 12
    distinct, reads = r.levels((1, 2, 4))
    assert distinct.tolist() == [3, 1, 1] and reads.tolist() == [3, 3, 4]
    big = bgzf.DedupResult(np.zeros(12000, np.int64), np.array([12000] + [0] * 11999, np.int64), 1, 12000, 0)
    assert big.levels()[0].tolist() == [0] * 15 + [1] and big.levels()[1].tolist() == [0] * 15 + [12000] and big.duplication_rate == 11999 / 12000
    for edges in ((), (2, 3), (1, 1), (1, 3, 2), (1.0, 2.0), [[1, 2]]):
        with pytest.raises(ValueError):
            r.levels(edges)
    none = bgzf.DedupResult(np.zeros(0, np.int64), np.zeros(0, np.int64), 0, 0, 0)
    assert (none.records, none.duplication_rate, none.drop().tolist(), none.most_common()[0].tolist(), none.levels()[0].sum()) == (0, 0.0, [], [], 0)
    assert repr(r) == "<DedupResult: 10 records, 5 unique, 5 duplicates (50.0 %), the most common one 4 times>"


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
    exe = str(tmp_path / "dedup_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dedup_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf dedup arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

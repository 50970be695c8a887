"""BGZF sort without a GPU: the referee against itself on every input table (the order by parsed values is the memcmp order of the
encoded keys, so the inputs give one defined answer), every ValueError of the Python layer with no context, SortKeyResult arithmetic,
the header's declarations against the library and the bindings, and every hostile argument of the entry points under the sanitizers."""
import ctypes as C
import gzip
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sort_inputs as I
import sort_ref as R
from conftest import GOLDEN, PKG_DIR, ROOT
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang

PRESETS = {
    "name": R.conf([R.part(0, 0, b" ", width=64)]),
    "sequence": R.conf([R.part(1, width=128, truncate=True), R.part(1, width=128, first=128, truncate=True)]),
    "length": R.conf([R.part(1, kind="length")]),
    "vcf": R.conf([R.part(0, 0), R.part(0, 1, kind="number")], record_lines=1, meta=b"#"),
    "bed": R.conf([R.part(0, 0), R.part(0, 1, kind="number")], record_lines=1, meta=b"#"),
    "gff": R.conf([R.part(0, 0), R.part(0, 3, kind="number")], record_lines=1, meta=b"#"),
    "sam": R.conf([R.part(0, 2), R.part(0, 3, kind="number")], record_lines=1, meta=b"@"),
}


def golden_records():
    with gzip.open(os.path.join(GOLDEN, "test.fastq.bgzip.gz"), "rb") as f:
        return I.fastq_records(f.read())


@pytest.mark.parametrize("variant", [dict(), dict(meta=True), dict(short_last=True), dict(open_last=True), dict(meta=True, short_last=True, open_last=True)],
                         ids=lambda v: "+".join(v) or "plain")
@pytest.mark.parametrize("name", list(I.GRID))
def test_referee_against_itself(name, variant):
    recs = list(I.table(**variant))
    cf = I.grid_conf(name, meta=b"#" if variant.get("meta") else None)
    keys = R.encode(recs, cf)
    assert keys.shape == (len(recs), R.width_of(cf)) and keys.dtype == np.uint8
    if not keys.shape[1]:
        return
    meta = [R.is_meta(r, cf) for r in recs]
    assert all(not keys[i].any() for i in range(len(recs)) if meta[i])
    # a meta line in the MIDDLE stays in front only of records whose own key is not all zero (an empty field, the number 0): where the
    # table holds such records the two orders differ by definition, and the key bytes alone are compared on the GPU
    if not any(m for m in meta[2:]) or all(keys[i].any() for i in range(len(recs)) if not meta[i]):
        assert R.lexorder(keys).tolist() == R.order(recs, cf)
    else:
        assert name not in ("four parts", "length of tag reverse")     # (these stay defined with meta lines in the middle)
    # and the text splits back into the records, with the length rule of the last one
    text = b"".join(recs)
    assert R.split(text, cf) == recs and sum(R.lengths(recs, cf)) == len(text) + (0 if text.endswith(b"\n") else 1)


def test_referee_on_the_files():
    head, body = I.vcf()
    recs = list(head) + list(body)
    cf = PRESETS["vcf"]
    got = R.order(recs, cf)
    assert R.lexorder(R.encode(recs, cf)).tolist() == got and got[:len(head)] == list(range(len(head)))
    out = [recs[i] for i in got][len(head):]
    rows = [(x.split(b"\t")[0], int(x.split(b"\t")[1])) for x in out]
    assert rows == sorted(rows) and len({r for r in rows}) < len(rows)             # sorted by name, then position; there are ties
    recs = golden_records()
    assert len(recs) == 10000
    for name in ("name", "sequence", "length"):
        assert R.lexorder(R.encode(recs, PRESETS[name])).tolist() == R.order(recs, PRESETS[name]), name
    assert all(b"\0" not in r for r in recs)


def test_referee_by_hand():
    cf = R.conf([R.part(0, 1, kind="number"), R.part(0, 0, width=8, reverse=True, ignore_case=True), R.part(0, 2, kind="length")], record_lines=1)
    recs = [b"b\t007\txyz\n", b"A\t7\t\n", b"a\t18446744073709551615\n"]
    k = R.encode(recs, cf)
    assert k.shape == (3, 24) and bytes(k[0]) == (7).to_bytes(8, "big") + bytes([255 - 66] + [255] * 7) + (3).to_bytes(4, "big") + bytes(4)
    assert bytes(k[2]) == b"\xff" * 8 + bytes([255 - 65] + [255] * 7) + bytes(8)
    assert R.order(recs, cf) == [0, 1, 2] == R.lexorder(k).tolist()                # 7: "b" before "A" when reversed; then the largest number
    for bad, kind in ((b"a\t\tz\n", 2), (b"a\t12a\tz\n", 2), (b"a\t18446744073709551616\tz\n", 2), (b"abcdefghi\t1\tz\n", 3)):
        with pytest.raises(R.Fault) as e:
            R.encode(recs + [bad], cf)
        assert (e.value.kind, e.value.record) == (kind, 3)
    with pytest.raises(R.Fault) as e:
        R.encode([b"abcdefghi\tx\n"] + recs, cf._replace(first_byte=b"a"))
    assert (e.value.kind, e.value.record) == (2, 0)                                # of two faults at one record the lower number
    with pytest.raises(R.Fault) as e:
        R.encode(recs, cf._replace(first_byte=b"b"))
    assert (e.value.kind, e.value.record) == (1, 1)
    assert R.lengths([b"a\n", b"b"], cf) == [2, 2] and R.written([b"a\n", b"b"], cf) == [b"a\n", b"b\n"]
    rows = I.rows("random", 500, 16)
    assert R.lexorder(rows).tolist() == sorted(range(500), key=lambda i: (bytes(rows[i]), i))
    two = I.rows("two_keys", 10000, 8)
    assert len(np.unique(two, axis=0)) == 2 and R.lexorder(two).tolist() == sorted(range(10000), key=lambda i: (bytes(two[i]), i))
    assert len(np.unique(I.rows("all256", 300, 8)[:, 4])) == 256 and (I.rows("equal", 70, 16) == I.rows("equal", 70, 16)[0]).all()


def test_argument_checks_need_no_context(monkeypatch, tmp_path):
    from zlib_ng_amd import _lib, bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    f = _Unreadable()
    K = bgzf.SortKey
    for kw in (dict(kind="float"), dict(width=12), dict(width=0), dict(width=136), dict(width=8.0), dict(first=-1), dict(line=-1), dict(line=64), dict(column=-1),
               dict(sep=b"ab"), dict(sep=b""), dict(reverse=1), dict(ignore_case="yes"), dict(kind="number", ignore_case=True), dict(kind="length", truncate=True)):
        with pytest.raises(ValueError):
            K(**kw)
    with pytest.raises(ValueError, match="width is a multiple of 8, not 12"):
        K(width=12)
    five = [K(width=8)] * 5
    wide = [K(width=128), K(width=128), K(kind="number")]
    for key, match in ((five, "at most 4 parts, not 5"), (wide, "add up to 264 bytes: at most 256"), ("names", "unknown preset 'names'"), ([K(), "name"], "key is a SortKey"),
                       (K(line=4), "line lies between 0 and 3, not 4")):
        for call in (lambda: bgzf.sort_key_records(f, key), lambda: bgzf.sort_key_records("/nonexistent/x.gz", key),
                     lambda: bgzf.sort_records(f, str(tmp_path / "o.gz"), key), lambda: bgzf.sort_records("/nonexistent/x.gz", str(tmp_path / "o.gz"), key)):
            with pytest.raises(ValueError, match=match):
                call()
    for kw in (dict(meta=b"##"), dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(record_lines=0), dict(record_lines=65), dict(truncate=1), dict(max_record=0)):
        with pytest.raises(ValueError):
            bgzf.sort_key_records(f, "name", **kw)
    with pytest.raises(ValueError):
        bgzf.sort_records(f, str(tmp_path / "o.gz"), "name", reverse="yes")
    assert not os.path.exists(str(tmp_path / "o.gz"))                              # nothing was opened
    # sort_keys: the rows
    for keys in (np.zeros((3, 12), np.uint8), np.zeros((3, 4), np.uint8), np.zeros((3, 264), np.uint8), np.zeros((3, 0), np.uint8), np.zeros((3, 8), np.uint16),
                 np.zeros(8, np.uint8), np.zeros((3, 16), np.uint8)[:, ::2], [[1, 2]], "keys"):
        with pytest.raises(ValueError):
            bgzf.sort_keys(keys)
    with pytest.raises(ValueError, match="a multiple of 8 between 8 and 256, not 12"):
        bgzf.sort_keys(np.zeros((3, 12), np.uint8))
    # permute_records: the order
    out = str(tmp_path / "p.gz")
    lens = np.array([10, 20, 30], np.uint32)
    for order, match in (([0, 1, 1], "holds record 1 more than once"), ([0, 3], r"order\[1\] is 3: a record number lies between 0 and 2"), ([-1], r"order\[0\] is -1"),
                         ([[0, 1]], "one-dimensional"), ([0.5], "one-dimensional")):
        for src in (f, "/nonexistent/x.gz"):
            with pytest.raises(ValueError, match=match):
                bgzf.permute_records(src, order, out, lengths=lens)
    for order, match in (([2, 2], "more than once"), ([-5, 1], r"order\[0\] is -5")):      # without lengths: what can be judged is
        with pytest.raises(ValueError, match=match):
            bgzf.permute_records(f, order, out)
    for kw in (dict(lengths=[[1]]), dict(lengths=[-1]), dict(lengths=[1 << 32]), dict(chunk_bytes=0), dict(block_size=0), dict(delimiter=b""), dict(first_byte=b"ab"),
               dict(record_lines=0)):
        with pytest.raises(ValueError):
            bgzf.permute_records(f, [0], out, **dict(dict(lengths=lens), **kw))
    assert not os.path.exists(out)
    # the configuration as the engine gets it
    cf, d, k, spec = bgzf._sort_conf([K(0, 1, kind="number", reverse=True), K(1, width=64, first=3, ignore_case=True)], 4, b"#", True, False, b"@", b"\n")
    assert (cf.record_lines, cf.first_byte, cf.meta_byte, cf.n_parts, list(cf.reserved), d, k) == (4, 64, 35, 2, [0] * 8, b"\n", 4)
    p = cf.part[0]
    assert (p.line, p.column, p.width, p.first, p.flags, p.kind, p.sep) == (0, 1, 0, 0, _lib.BGZF_SORT_REVERSE, _lib.BGZF_SORT_NUMBER, 9)
    p = cf.part[1]
    assert (p.line, p.column, p.width, p.first, p.flags, p.kind) == (1, -1, 64, 3, _lib.BGZF_SORT_IGNORE_CASE | _lib.BGZF_SORT_TRUNCATE, _lib.BGZF_SORT_BYTES)
    assert bytes(cf.part[2]) == bytes(cf.part[3]) == bytes(20) and spec["width"] == 72 and spec["meta"] == 35
    cf, _, k, spec = bgzf._sort_conf("vcf", 4, None, False, True, None, b"\n")      # a line format: one line per record; reverse turns every part round
    assert (k, cf.meta_byte, cf.n_parts, spec["width"]) == (1, 35, 2, 40) and cf.part[0].flags == cf.part[1].flags == _lib.BGZF_SORT_REVERSE
    assert (cf.part[0].column, cf.part[1].column, cf.part[1].kind) == (0, 1, _lib.BGZF_SORT_NUMBER)
    for preset, cols, meta in (("bed", (0, 1), 35), ("gff", (0, 3), 35), ("sam", (2, 3), 64)):
        cf = bgzf._sort_conf(preset, 4, None, False, False, None, b"\n")[0]
        assert (cf.part[0].column, cf.part[1].column, cf.meta_byte, cf.record_lines) == cols + (meta, 1)
    cf, _, _, spec = bgzf._sort_conf("sequence", 4, None, False, False, None, b"\n")
    assert spec["width"] == 256 and [(q.first, q.width, q.flags) for q in cf.part[:2]] == [(0, 128, 4), (128, 128, 4)]
    cf, _, _, spec = bgzf._sort_conf("name", 4, None, False, False, None, b"\n")
    assert (cf.part[0].line, cf.part[0].column, cf.part[0].sep, cf.part[0].width, spec["width"]) == (0, 0, 32, 64, 64)
    names = ["SortKey", "SortKeyResult", "SortResult", "sort_key_records", "sort_keys", "permute_records", "sort_records"]
    assert all(n in bgzf.__all__ for n in names)
    rec_kw = ["first_byte", "delimiter", "start", "stop", "first_record", "max_record", "allow_short"]
    sig = inspect.signature(bgzf.sort_key_records).parameters
    assert list(sig) == ["file", "key", "record_lines", "meta", "truncate"] + rec_kw
    assert list(inspect.signature(bgzf.BgzfReader.sort_key_records).parameters) == ["self"] + list(sig)[1:]
    sig = inspect.signature(bgzf.permute_records).parameters
    assert list(sig) == ["file", "order", "output", "record_lines", "lengths", "chunk_bytes", "compresslevel", "block_size", "first_byte", "delimiter"]
    assert (sig["chunk_bytes"].default, sig["compresslevel"].default, sig["block_size"].default, sig["lengths"].default) == (1 << 30, 6, bgzf.MAX_BLOCK_INPUT, None)
    assert list(inspect.signature(bgzf.BgzfReader.permute_records).parameters) == ["self"] + list(sig)[1:]
    sig = inspect.signature(bgzf.sort_records).parameters
    assert list(sig)[:4] == ["file", "output", "key", "record_lines"] and sig["reverse"].default is False and sig["record_lines"].default == 4
    assert list(inspect.signature(bgzf.BgzfReader.sort_records).parameters) == ["self"] + list(sig)[1:]
    assert list(inspect.signature(bgzf.sort_keys).parameters) == ["keys", "rank"] and "ceil(text / chunk_bytes)" in bgzf.permute_records.__doc__


def test_sort_key_result_arithmetic():
    from zlib_ng_amd import bgzf
    spec = bgzf._sort_conf([bgzf.SortKey(width=8)], 4, None, False, False, None, b"\n")[3]
    a = bgzf.SortKeyResult(np.arange(16, dtype=np.uint8).reshape(2, 8), np.array([5, 6], np.uint32), spec)
    b = bgzf.SortKeyResult(np.full((1, 8), 7, np.uint8), np.array([9], np.uint32), spec)
    s = a + b
    assert (s.records, len(s), s.key_width, s.spec) == (3, 3, 8, spec) and s.lengths.tolist() == [5, 6, 9] and s.keys.shape == (3, 8) and s.keys[2].tolist() == [7] * 8
    assert (a.records, b.records) == (2, 1) and (b + a).lengths.tolist() == [9, 5, 6]      # (the parts are left as they were)
    empty = bgzf.SortKeyResult(np.empty((0, 8), np.uint8), np.empty(0, np.uint32), spec)
    assert (empty + a).keys.tolist() == a.keys.tolist() and (empty + empty).records == 0
    for other in ([bgzf.SortKey(width=8, reverse=True)], [bgzf.SortKey(width=8, first=1)], [bgzf.SortKey(kind="number")], [bgzf.SortKey(1, width=8)]):
        o = bgzf._sort_conf(other, 4, None, False, False, None, b"\n")[3]
        with pytest.raises(ValueError, match="not comparable"):
            a + bgzf.SortKeyResult(np.zeros((1, 8), np.uint8), np.array([1], np.uint32), o)
    with pytest.raises(ValueError, match="not comparable"):
        a + bgzf.SortKeyResult(np.zeros((1, 8), np.uint8), np.array([1], np.uint32), dict(spec, meta=35))
    with pytest.raises(TypeError):
        a + 1
    with pytest.raises(ValueError):
        bgzf.SortKeyResult(np.zeros((2, 16), np.uint8), np.array([1, 2], np.uint32), spec)
    assert repr(s) == "<SortKeyResult: 3 records, keys of 8 bytes>"
    assert bgzf._permute_buckets(np.array([5, 5, 5, 20, 1, 1], np.uint32), 10) == [(0, 2), (2, 3), (3, 4), (4, 6)]      # a record larger than the chunk stands alone
    assert bgzf._permute_buckets(np.array([], np.uint32), 10) == [] and bgzf._permute_buckets(np.array([3, 3, 3], np.uint32), 100) == [(0, 3)]
    r = bgzf.SortResult(np.array([1, 0]), 2, 99, 64)
    assert (len(r), r.bytes, r.key_width) == (2, 99, 64) and repr(r) == "<SortResult: 2 records, 99 bytes, keys of 64 bytes>"


def _struct_fields(header, name):
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % name, header).group(1)
    return [re.sub(r"\[.*", "", x) for x in re.findall(r"\b(\w+(?:\[\w+\])?);", re.sub(r"/\*.*?\*/", "", body))]


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    ctype = {"zngamd_ctx *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int, "int32_t": C.c_int32, "zngamd_alloc_fn": _lib.ALLOC_FN}

    def params_of(name, ret="int"):
        return [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\b%s %s\s*\(([^;]*)\);" % (ret, name), header).group(1).split(",")]

    for name in ("zngamd_bgzf_sort_key_records_dev", "zngamd_bgzf_sort_key_records", "zngamd_sort_keys_dev", "zngamd_sort_keys", "zngamd_bgzf_place_records_dev",
                 "zngamd_bgzf_place_records"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        want = [C.c_void_p if "*" in p else ctype[p.rsplit(" ", 1)[0]] for p in params_of(name)]
        assert getattr(L, name).argtypes == want, name
    for name in ("zngamd_bgzf_sort_key_records_dev", "zngamd_bgzf_sort_key_records"):
        params = params_of(name)
        assert params[:11] == params_of(name.replace("sort_key", "key"))[:9] + ["const zngamd_bgzf_sort_conf *conf", "uint64_t record_base"]      # the window of the key pass
        assert params[-1] == "zngamd_bgzf_sort_key_totals *totals"
    for name in ("zngamd_bgzf_place_records_dev", "zngamd_bgzf_place_records"):
        assert params_of(name)[:12] == params_of(name.replace("place", "partition"))[:12]                  # the window of the partition call
    assert params_of("zngamd_sort_keys_dev") == ["zngamd_ctx *ctx", "const uint8_t *d_keys", "uint64_t n", "uint32_t width", "void *d_scratch", "uint64_t scratch_cap",
                                                 "uint32_t *d_order", "uint32_t *d_rank"]
    assert "zngamd_sort_scratch_bytes" in _lib.SYMBOLS and params_of("zngamd_sort_scratch_bytes", "uint64_t") == ["uint64_t n", "uint32_t width"]
    assert L.zngamd_sort_scratch_bytes.restype is C.c_uint64 and L.zngamd_sort_scratch_bytes.argtypes == [C.c_uint64, C.c_uint32]
    for (n, w), want in (((0, 8), 1040), ((1, 8), 2080), ((2048, 256), 12800), ((2049, 16), 13360), ((1 << 30, 256), (1 << 32) + (1 << 30) + (1 << 29) + 1536)):
        assert L.zngamd_sort_scratch_bytes(n, w) == want, (n, w)
    for n, w in (((1 << 30) + 1, 8), (1, 0), (1, 4), (1, 12), (1, 264)):
        assert L.zngamd_sort_scratch_bytes(n, w) == 0, (n, w)
    for struct, ct, size in (("zngamd_bgzf_sort_part", _lib.BgzfSortPart, 20), ("zngamd_bgzf_sort_conf", _lib.BgzfSortConf, 128),
                             ("zngamd_bgzf_sort_key_totals", _lib.BgzfSortKeyTotals, 64), ("zngamd_bgzf_place_totals", _lib.BgzfPlaceTotals, 64)):
        assert int(re.search(r"\}\s*%s;\s*/\* (\d+) B \*/" % struct, header).group(1)) == C.sizeof(ct) == size
        assert _struct_fields(header, struct) == [f[0] for f in ct._fields_], struct
    assert _lib.BgzfSortKeyTotals.tail_off.offset == _lib.BgzfPlaceTotals.tail_off.offset == 24 and _lib.BgzfSortKeyTotals.bad.offset == _lib.BgzfPlaceTotals.bad.offset == 56
    for macro, value in (("SORT_BYTES", _lib.BGZF_SORT_BYTES), ("SORT_NUMBER", _lib.BGZF_SORT_NUMBER), ("SORT_LENGTH", _lib.BGZF_SORT_LENGTH),
                         ("SORT_REVERSE", _lib.BGZF_SORT_REVERSE), ("SORT_IGNORE_CASE", _lib.BGZF_SORT_IGNORE_CASE), ("SORT_TRUNCATE", _lib.BGZF_SORT_TRUNCATE),
                         ("SORT_MAX_PARTS", _lib.BGZF_SORT_MAX_PARTS)):
        assert int(re.search(r"#define ZNGAMD_BGZF_%s\s+(\d+)u" % macro, header).group(1)) == value
    assert re.search(r"#define ZNGAMD_SORT_MAX_KEYS\s+\(1ull << 30\)", header) and _lib.SORT_MAX_KEYS == 1 << 30
    assert re.search(r"#define ZNGAMD_SORT_MAX_WIDTH\s+256u", header) and _lib.SORT_MAX_WIDTH == 256
    assert re.search(r"#define ZNGAMD_BGZF_PLACE_SKIP\s+\(~0ull\)", header) and _lib.BGZF_PLACE_SKIP == (1 << 64) - 1
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_sort.hip"' in build
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_dedup.hip"') < main.index('#include "za_sort.hip"') < main.index('#include "za_overlap.hip"')
    kernel = open(os.path.join(PKG_DIR, "csrc", "za_sort.hip")).read()
    for k in ("za_k_sort_keys", "za_k_sort_orand", "za_k_sort_hist", "za_k_sort_scan", "za_k_sort_scatter", "za_k_sort_rank", "za_k_sort_place"):
        assert "void %s(" % k in kernel and k in main
    assert int(re.search(r"#define ZA_SORT_STRIPS\s+(\d+)u", kernel).group(1)) * 256 == I.TILE      # the tile the test sizes are built around


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
    exe = str(tmp_path / "sort_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sort_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf sort arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

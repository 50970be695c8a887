"""CPU: BGZF by region without a GPU -- the referee pinned with literals and a hand-worked file; the .tbi layout as written and as
accepted, with truncated and hostile blobs; TabixIndex.chunks against brute force; parse_region; presets and argument errors that
need no context; and the window loop, the merging of the per-window tables and the fetch planner of bgzf.py, driven by a stand-in
for the two engine calls (tests/tabix_files.py: FakeEngine) on files written with the system zlib."""
import gzip
import io
import os
import re
import struct

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
import tabix_files as F
import tabix_ref as R

# five lines of 32 bytes in blocks of 64 bytes, stored: a block of n bytes takes n + 31 -> blocks at 0, 95, 190, the EOF block at 253
def _line32(name, pos, rest):
    """a VCF line of exactly 32 bytes: the ID column takes up the slack"""
    fixed = len(name) + len(pos) + len(rest) + 3
    return name + b"\t" + pos + b"\t" + b"i" * (31 - fixed) + b"\t" + rest + b"\n"


HAND = (b"#" + b"c" * 30 + b"\n" + _line32(b"chr1", b"100", b"A\tT\t50\tPASS\tDP=1") + _line32(b"chr1", b"20000", b"AC\tT\t5\tq\tEND=40000") +
        _line32(b"chr1", b"40000", b"A\tT\t50\tPASS\tDP=1") + _line32(b"chr2", b"5", b"A\tT\t50\tPASS\tDP=1"))
V = lambda c, u=0: c << 16 | u
HAND_BINS = [{4681: [(V(0, 32), V(95))], 585: [(V(95), V(95, 32))], 4683: [(V(95, 32), V(190))]}, {4681: [(V(190), V(253))]}]
HAND_LINEAR = [[V(0, 32), V(95), V(95)], [V(190)]]


def test_referee_pinned_with_literals():
    assert R.reg2bin(0, 1) == 4681 and R.reg2bin(16383, 16385) == 585 and R.reg2bin(0, 2 ** 29) == 0
    assert len(R.reg2bins(0, 2 ** 29)) == 37449 and len(set(R.reg2bins(0, 2 ** 29))) == 37449
    assert R.reg2bin((1 << 26) - 1, (1 << 26) + 1) == 0 and R.reg2bin(1 << 26, (1 << 26) + 1) == 4681 + 4096
    assert len(HAND) == 160 and all(len(x) == 31 for x in HAND.split(b"\n")[:-1])
    blob = F.host_bgzf(HAND, 64, level=0)
    assert [b[0] for b in R.blocks_of(blob)] == [0, 95, 190, 253] and gzip.decompress(blob) == HAND
    names, bins, linear = R.build(blob, R.PRESETS["vcf"])
    assert names == [b"chr1", b"chr2"] and bins == HAND_BINS and linear == HAND_LINEAR
    P = lambda raw, conf=R.PRESETS["vcf"], n=9, term=True: R.parse_line(raw, term, conf, n)
    assert P(b"c\t10\t.\tACG\tT") == ("data", b"c", 9, 12)
    assert P(b"c\t10\t.\tACG\tT\t.\t.\tDP=1;END=50\r") == ("data", b"c", 9, 50)
    assert P(b"c\t10\t.\tACG\tT\t.\t.\tXEND=50;END=60") == ("data", b"c", 9, 60)
    assert P(b"c\t10\t.\tACG\tT\t.\t.\tEND=5;END=60") == ("data", b"c", 9, 12)        # the first END= decides: 5 <= beg
    assert P(b"c\t10\t.\tACG\tT\t.\t.\tEND=;END=60") == ("data", b"c", 9, 12)
    assert P(b"c\t10\t.") == ("bad", 1) and P(b"c\t1x\t.\tA") == ("bad", 2) and P(b"c\t12345678901\t.\tA") == ("bad", 2)
    assert P(b"c\t0\t.\tA") == ("bad", 3) and P(b"c\t%d\t.\tAC" % 2 ** 29) == ("bad", 3) and P(b"c\t%d\t.\tA" % 2 ** 29)[0] == "data"
    assert P(b"#c\t10") == ("skip",) and P(b"") == ("skip",) and P(b"\r") == ("skip",) and P(b"c", n=2, conf=(2, 1, 2, 0, 35, 3)) == ("skip",)
    assert P(b"c\t5\t9", conf=R.PRESETS["bed"]) == ("data", b"c", 5, 9) and P(b"c\t5\t5", conf=R.PRESETS["bed"]) == ("data", b"c", 5, 6)
    assert P(b"c\t.\t.\t5\t9", conf=R.PRESETS["gff"]) == ("data", b"c", 4, 9)
    assert P(b"x\tc\t7", conf=(0, 2, 3, 0, 35, 0)) == ("data", b"c", 6, 7) and P(b"c\t7\r", conf=(0, 1, 2, 0, 35, 0), term=False) == ("bad", 2)


def test_symbols_declared_exported_and_bound():
    import ctypes as C
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    for name in ("zngamd_bgzf_tabix_dev", "zngamd_bgzf_tabix", "zngamd_bgzf_fetch_dev", "zngamd_bgzf_fetch"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        nargs = len(re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(","))
        assert len(getattr(L, name).argtypes) == nargs, name
    assert C.sizeof(_lib.BgzfTabixTotals) == 104 and C.sizeof(_lib.BgzfFetchTotals) == 16 and C.sizeof(_lib.TabixConf) == 24
    assert [_lib.TABIX_NAME_DTYPE.itemsize, _lib.TABIX_BIN_DTYPE.itemsize, _lib.TABIX_WIN_DTYPE.itemsize, _lib.TABIX_REGION_DTYPE.itemsize,
            _lib.TABIX_SPAN_DTYPE.itemsize, _lib.TABIX_ROW_DTYPE.itemsize] == [32, 40, 16, 16, 24, 16]
    assert (F.NAME, F.BIN, F.WIN, F.ROW) == (_lib.TABIX_NAME_DTYPE, _lib.TABIX_BIN_DTYPE, _lib.TABIX_WIN_DTYPE, _lib.TABIX_ROW_DTYPE)
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES)                            # no kernel class was added
    assert '"za_tabix.hip"' in open(os.path.join(PKG_DIR, "build.py")).read()
    # hostile configurations and region tables are refused before the context is looked at (a NULL context is never touched)
    tot, ftot = _lib.BgzfTabixTotals(), _lib.BgzfFetchTotals()
    for conf in ((1, 1, 2, 0, 35, 0), (2, 0, 2, 0, 35, 0), (0, 1, 0, 0, 35, 0), (0, 1, 2, -1, 35, 0), (0, 1, 2, 0, 256, 0), (0, 1, 2, 0, 35, -1),
                 (0x20000, 1, 2, 0, 35, 0)):
        cf = _lib.TabixConf(*conf)
        args = [None, None, 0, None, 0, 0, 0, C.byref(cf), 10, 0, 0, None, None, 0, None, 0, None, 0, None, 0, _lib.ALLOC_FN(), None, C.byref(tot)]
        assert L.zngamd_bgzf_tabix(*args) == _lib.E_ARG, conf
    cf = _lib.TabixConf(2, 1, 2, 0, 35, 0)
    for reg, n in (((0, 5, 0, 9), 1), ((3, 2, 0, 9), 1), ((0, 1, 0, 9), 0), ((0, 1, 0, 9), 4097)):
        tab = np.array([reg] * max(n, 1), _lib.TABIX_REGION_DTYPE)
        args = [None, None, 0, None, 0, C.byref(cf), 10, 0, b"abcd", 4, C.c_void_p(tab.ctypes.data), n, None, 0, None, None, None, None, 0, None, 0,
                _lib.ALLOC_FN(), None, C.byref(ftot)]
        assert L.zngamd_bgzf_fetch(*args) == _lib.E_ARG, (reg, n)


def test_parse_region():
    from zlib_ng_amd import bgzf
    M = bgzf.TABIX_MAX_POS
    assert bgzf.parse_region("chr1:1,000-2,000") == (b"chr1", 999, 2000)
    assert bgzf.parse_region("chr1") == (b"chr1", 0, M) and bgzf.parse_region(b"chr1:1000") == (b"chr1", 999, M)
    assert bgzf.parse_region("HLA-A*01:01:5-7") == (b"HLA-A*01:01", 4, 7) and bgzf.parse_region("HLA:x") == (b"HLA:x", 0, M)
    assert bgzf.parse_region("c:0-5") == (b"c", 0, 5) and bgzf.parse_region(("c", 3, 3)) == (b"c", 3, 3)
    for bad in ("", "c:9-3", ("c", -1, 4), ("c", 1)):
        with pytest.raises(ValueError):
            bgzf.parse_region(bad)
    assert bgzf.reg2bin(0, 1) == 4681 and bgzf.reg2bin(16383, 16385) == 585 and bgzf.reg2bin(0, M) == 0 and len(bgzf.reg2bins(0, M)) == 37449
    rng = np.random.default_rng(1)
    for _ in range(300):
        b = int(rng.integers(0, M - 1))
        e = min(M, b + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 29)))))
        assert bgzf.reg2bin(b, e) == R.reg2bin(b, e) and bgzf.reg2bins(b, e) == R.reg2bins(b, e) and R.reg2bin(b, e) in R.reg2bins(b, e)


def test_presets_and_argument_errors_need_no_context(monkeypatch, tmp_path):
    from zlib_ng_amd import bgzf, zlib_ng

    def no_ctx():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(zlib_ng, "_ctx", no_ctx)
    C = bgzf._tabix_conf
    assert C("gff", None, None, None, False, b"#", 0) == (0, 1, 4, 5, 35, 0) and C("bed", None, None, None, False, b"#", 0) == (0x10000, 1, 2, 3, 35, 0)
    assert C("vcf", None, None, None, False, b"@", 3) == (2, 1, 2, 0, 64, 3) and C(None, 2, 3, None, True, b"#", 0) == (0x10000, 2, 3, 0, 35, 0)
    path = tmp_path / "x.gz"
    path.write_bytes(F.host_bgzf(HAND, 64, level=0))
    for args, kw in ((("sam",), {}), (("bcf",), {}), ((), {}), ((), {"seq_col": 1}), (("vcf",), {"seq_col": 1}), ((), {"seq_col": 0, "start_col": 2}),
                     (("vcf",), {"meta": b"##"}), (("vcf",), {"skip": -1})):
        with pytest.raises(ValueError):
            bgzf.TabixIndex.build(str(path), *args, **kw)
    idx = bgzf.TabixIndex((2, 1, 2, 0, 35, 0), [b"chr1", b"chr2"], HAND_BINS, HAND_LINEAR)
    for regions in ("c:9-3", [("c", -1, 4)], [""]):
        with pytest.raises(ValueError):
            bgzf.fetch(str(path), idx, regions)
    with pytest.raises(TypeError):
        bgzf.fetch(str(path), object(), "chr1")
    with pytest.raises(ValueError, match="does not fit"):
        bgzf.fetch(io.BytesIO(path.read_bytes()[:200]), idx, "chr1")              # the index is for a longer file
    sam = bgzf.TabixIndex((1, 3, 4, 0, 64, 0), [b"chr1", b"chr2"], HAND_BINS, HAND_LINEAR)
    with pytest.raises(ValueError, match="configuration"):
        bgzf.fetch(str(path), sam, "chr1")
    assert len(bgzf.fetch(str(path), idx, "chr9")) == 0 and bgzf.fetch(str(path), idx, ["chr9", "chr1:900000"], count=True) == [0, 0]


def _plain(conf, names, tables, tail=b""):
    """a .tbi packed by hand: tables = per name ([(bin, [(beg, end), ...])], [linear])"""
    nm = b"".join(n + b"\0" for n in names)
    out = [b"TBI\1", struct.pack("<8i", len(names), *conf, len(nm)), nm]
    for bins, lin in tables:
        out.append(struct.pack("<i", len(bins)))
        for b, cs in bins:
            out.append(struct.pack("<Ii", b, len(cs)) + b"".join(struct.pack("<QQ", x, y) for x, y in cs))
        out.append(struct.pack("<i", len(lin)) + b"".join(struct.pack("<Q", v) for v in lin))
    return b"".join(out) + tail


def test_tbi_layout_round_trip_and_hostile_blobs(monkeypatch):
    from zlib_ng_amd import bgzf
    conf = (2, 1, 2, 0, 35, 0)
    idx = bgzf.TabixIndex(conf, [b"chr1", b"chr2"], HAND_BINS, HAND_LINEAR)
    raw = idx.to_bytes(compressed=False)
    assert raw == _plain(conf, [b"chr1", b"chr2"], [(sorted(d.items()), lin) for d, lin in zip(HAND_BINS, HAND_LINEAR)])
    back = bgzf.TabixIndex.from_bytes(raw)
    assert back == idx and back.names == [b"chr1", b"chr2"] and len(back) == 2 and back.to_bytes(compressed=False) == raw
    assert idx != bgzf.TabixIndex(conf, [b"chr1", b"chrX"], HAND_BINS, HAND_LINEAR)
    idx.validate(281)
    for size in (252, 100):
        with pytest.raises(ValueError, match="does not fit"):
            idx.validate(size)
    with pytest.raises(ValueError):
        bgzf.TabixIndex(conf, [b"a"], [{1: [(5, 5)]}], [[0]]).validate(1000)
    # htslib's pseudo-bin and n_no_coor are accepted, and the bin is dropped
    tables = [(sorted(d.items()) + [(37450, [(V(0, 32), V(190)), (3, 0)])], lin) for d, lin in zip(HAND_BINS, HAND_LINEAR)]
    foreign = _plain(conf, [b"chr1", b"chr2"], tables, struct.pack("<Q", 7))
    assert bgzf.TabixIndex.from_bytes(foreign) == idx
    # BGZF-compressed and plain both load (the decoder stands in for the engine's here; the GPU test loads what save() wrote)
    monkeypatch.setattr(bgzf, "decompress", gzip.decompress)
    assert bgzf.TabixIndex.from_bytes(F.host_bgzf(foreign, 100)) == idx and bgzf.TabixIndex.load(io.BytesIO(F.host_bgzf(raw, 1000))) == idx
    # every truncation, and hostile counts: ValueError (with an offset) or an equal index, never another exception
    for blob in (raw, foreign):
        for n in range(len(blob)):
            try:
                assert bgzf.TabixIndex.from_bytes(blob[:n]) == idx
            except ValueError as e:
                assert "offset" in str(e), (n, e)
    for at in range(4, len(raw) - 3, 4):
        for v in (-1, 0x7FFFFFFF, 0x10000000, -(1 << 31)):
            try:
                got = bgzf.TabixIndex.from_bytes(raw[:at] + struct.pack("<i", v) + raw[at + 4:])
                got.chunks(b"chr1", 0, 1 << 29), got.validate(281)
            except ValueError:
                pass
    for bad in (raw[:40] + b"x" + raw[41:], b"TBI\2" + raw[4:], raw + b"\0", b"\x1f\x8b" + raw, gzip.compress(b"nothing")):
        with pytest.raises(ValueError):
            bgzf.TabixIndex.from_bytes(bad)


@pytest.mark.parametrize("kind", ["vcf", "bed", "gff"])
def test_chunks_never_miss_an_overlapping_line(kind):
    from zlib_ng_amd import bgzf
    rng = np.random.default_rng({"vcf": 3, "bed": 4, "gff": 5}[kind])
    text, conf, names = F.make_text(kind, rng, n_names=5, per_name=80)
    blob = F.host_bgzf(text, 777)
    rows, v = R.table(blob, conf), R.Voffsets(blob)
    idx = bgzf.TabixIndex(conf, *R.build(blob, conf))
    idx.validate(len(blob))
    assert {R.reg2bin(r[4], r[5]) for r in rows} >= {0} and max(r[5] for r in rows) == 1 << 29
    regions = F.regions_for(rng, rows, names, 300)
    hit = 0
    for name, beg, end in regions:
        chunks = idx.chunks(name, beg, end)
        assert chunks == sorted(chunks) and all(a[1] < b[0] for a, b in zip(chunks, chunks[1:]))      # merged: neither overlap nor touch
        for r in R.overlaps(rows, name, beg, end):
            assert any(vb <= v(r[1]) < ve for vb, ve in chunks), (name, beg, end, r)
            hit += 1
    assert hit > 300 and idx.chunks(b"nobody", 0, 100) == [] and idx.chunks(names[0], 1 << 29, 1 << 30) == []


def _cpu_build(blob, conf, window=None, split=False, monkeypatch=None, slack=1200):
    """window: compressed bytes per window; a window is read with room for one more block, which for these files of small blocks
    is cut down with it (no block of theirs is longer than `slack` bytes)"""
    from zlib_ng_amd import bgzf
    if window is not None:
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        monkeypatch.setattr(bgzf, "MAX_BLOCK", slack)
    assert max(b[1] for b in R.blocks_of(blob)) <= slack
    eng = F.FakeEngine(split_runs=split)
    return bgzf._tabix_build(io.BytesIO(blob), eng, conf), eng


def test_hand_worked_file_through_the_window_loop(monkeypatch):
    from zlib_ng_amd import bgzf
    blob = F.host_bgzf(HAND, 64, level=0)
    want = bgzf.TabixIndex(R.PRESETS["vcf"], [b"chr1", b"chr2"], HAND_BINS, HAND_LINEAR)
    idx, eng = _cpu_build(blob, R.PRESETS["vcf"])
    assert idx == want and len(eng.calls) == 1
    idx, eng = _cpu_build(blob, R.PRESETS["vcf"], window=1, split=True, monkeypatch=monkeypatch, slack=96)      # one block per window
    assert idx == want and len(eng.calls) >= 3


@pytest.mark.parametrize("kind,crlf,final_newline,junk", [("vcf", False, True, 0), ("bed", True, True, 3), ("gff", False, False, 0),
                                                          ("vcf", True, False, 3)])
def test_window_loop_merges_to_the_referee_index(monkeypatch, kind, crlf, final_newline, junk):
    """merge across a window cut (many windows, cuts between equal names and inside bin runs), across skipped lines (the stand-in
    breaks every name run there), with the open line carried over"""
    from zlib_ng_amd import bgzf
    rng = np.random.default_rng(11)
    text, conf, names = F.make_text(kind, rng, n_names=5, per_name=40, crlf=crlf, final_newline=final_newline, junk=junk)
    for block_size in (37, 1001):
        blob = F.host_bgzf(text, block_size) + (b"" if block_size == 37 else F.host_bgzf(b"", 1))      # (a second EOF block behind the first)
        want = bgzf.TabixIndex(conf, *R.build(blob, conf))
        one, eng1 = _cpu_build(blob, conf)
        many, eng = _cpu_build(blob, conf, window=300, split=True, monkeypatch=monkeypatch)
        monkeypatch.undo()
        assert one == want and many == want and len(eng1.calls) == 1 and len(eng.calls) >= 3
        one.validate(len(blob))
        assert bgzf.TabixIndex.from_bytes(one.to_bytes(compressed=False)) == want


def test_merge_of_synthetic_run_records():
    from zlib_ng_amd import bgzf
    m = bgzf._TabixMerge()
    # window 1: name a, bins 4681 and 4682; the last run ends where the window's text ends (v_end None)
    m.add([(b"a", 3, 100)], [(0, 4681, 100, 200), (0, 4682, 200, None)], [(0, 0, 100), (0, 1, 200)], 5, 20000, head=100)
    # window 2 goes on with the same name and bin: the cut disappears; then a skipped line broke the name run (two rows, one name)
    m.add([(b"a", 9, 300), (b"a", 12, 400), (b"b", 13, 500)], [(0, 4682, 300, 400), (1, 4682, 400, 500), (2, 4681, 500, None)],
          [(0, 1, 300), (1, 1, 400), (2, 0, 500)], 20001, 7, head=300)
    idx = m.finish((0, 1, 2, 0, 35, 0), 900)
    assert idx.names == [b"a", b"b"] and idx.bins == [{4681: [(100, 200)], 4682: [(200, 500)]}, {4681: [(500, 900)]}]
    assert idx.linear == [[100, 200], [500]]
    # a run that ends with its window, and the next window starts another bin: the end is that window's first byte
    m = bgzf._TabixMerge()
    m.add([(b"a", 0, 10)], [(0, 4681, 10, None)], [(0, 0, 10)], 1, 1, head=10)
    m.add([], [], [], 0, 0, head=None)                      # (a window without text resolves nothing)
    m.add([(b"a", 5, 70)], [(0, 4683, 70, 80)], [(0, 2, 70)], 40000, 40000, head=64)
    assert m.finish((0, 1, 2, 0, 35, 0), 99).bins == [{4681: [(10, 64)], 4683: [(70, 80)]}] and m.linear == [[10, 70, 70]]
    # out of order across the cut, a name that comes back, and the smallest line wins
    m = bgzf._TabixMerge()
    m.add([(b"a", 0, 10), (b"b", 4, 50)], [(0, 4681, 10, 50), (1, 4681, 50, 90)], [(0, 0, 10), (1, 0, 50)], 1, 500, head=10)
    with pytest.raises(ValueError, match=r"line 7 at virtual offset 90 .*below") as e:
        m.add([(b"b", 7, 90)], [(0, 4681, 90, 95)], [(0, 0, 90)], 499, 499, head=90)
    assert e.value.line == 7 and e.value.kind == 4
    with pytest.raises(ValueError, match=r"line 8 .*came before"):
        m.add([(b"b", 7, 90), (b"a", 8, 95)], [], [], 500, 500, head=90)
    with pytest.raises(ValueError, match=r"line 6 .*column"):
        m.add([(b"b", 7, 90), (b"a", 8, 95)], [], [], 500, 500, head=90, bad=(6, 1, 88))
    with pytest.raises(ValueError, match=r"line 8 .*came before"):
        m.add([(b"b", 7, 90), (b"a", 8, 95)], [], [], 500, 500, head=90, bad=(9, 2, 99))


def _with_line(text, where, line):
    lines = text.split(b"\n")
    data = [i for i, ln in enumerate(lines) if ln and not ln.startswith(b"#")]
    lines.insert(data[where], line)
    return b"\n".join(lines)


def test_bad_lines_report_the_referees_line_through_the_window_loop(monkeypatch):
    from zlib_ng_amd import bgzf
    rng = np.random.default_rng(12)
    text, conf, names = F.make_text("bed", rng, n_names=4, per_name=30)
    cases = {1: b"chr2\t5", 2: b"chr2\t5\tx", 3: b"chr2\t5\t%d" % (2 ** 29 + 1), 4: b"1\t0\t1", "contig": b"1\t%d\t%d" % (2 ** 29 - 1, 2 ** 29)}
    for kind, line in cases.items():
        where = {4: 10, "contig": 70}.get(kind, 75)
        bad = _with_line(_with_line(text, 100, b"chr3\tx\ty") if kind != "contig" else text, where, line)      # (a second bad line further down)
        blob = F.host_bgzf(bad, 300)
        with pytest.raises(R.RefBad) as ref:
            R.table(blob, conf)
        assert ref.value.kind == kind
        for window in (None, 1500):
            with pytest.raises(ValueError, match=r"line %d at virtual offset" % ref.value.number) as e:
                _cpu_build(blob, conf, window=window, monkeypatch=monkeypatch)
            assert e.value.kind == kind and e.value.voffset == R.Voffsets(blob)(bad.index(line + b"\n"))


def test_fetch_plan_against_brute_force(monkeypatch):
    from zlib_ng_amd import bgzf, zlib_ng
    rng = np.random.default_rng(13)
    text, conf, names = F.make_text("vcf", rng, n_names=5, per_name=50, final_newline=False)
    blob = F.host_bgzf(text, 500)
    rows, v = R.table(blob, conf), R.Voffsets(blob)
    idx = bgzf.TabixIndex(conf, *R.build(blob, conf))
    eng = F.FakeEngine()
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: eng)
    regions = F.regions_for(rng, rows, names, 60)
    want = [R.overlaps(rows, *r) for r in regions]
    fp = io.BytesIO(blob)
    fp.seek(123)
    got = bgzf.fetch(fp, idx, regions)
    assert len(eng.calls) == 1 and eng.calls[0][1] < len(R.blocks_of(blob))                      # one call, every needed block once
    assert got.region.tolist() == [i for i, w in enumerate(want) for _ in w] and len(got) == sum(map(len, want)) > 60
    assert list(got) == [text[r[1]:r[1] + r[2]] for w in want for r in w] and got.voffsets.tolist() == [v(r[1]) for w in want for r in w]
    assert all(got.of(i) == [text[r[1]:r[1] + r[2]] for r in w] for i, w in enumerate(want)) and got[-1] == got[len(got) - 1]
    assert bgzf.fetch(io.BytesIO(blob), idx, regions, count=True) == [len(w) for w in want]
    assert bgzf.fetch(io.BytesIO(blob), idx, regions[2], count=True) == len(want[2]) and list(bgzf.fetch(io.BytesIO(blob), idx, regions[2])) == got.of(2)
    # a small cap on the decoded bytes of one call: several calls, the same answer
    monkeypatch.setattr(bgzf, "_GREP_TEXT", 3000)
    eng.calls.clear()
    again = bgzf.fetch(io.BytesIO(blob), idx, regions)
    assert len(eng.calls) > 3 and list(again) == list(got) and again.region.tolist() == got.region.tolist() and again.voffsets.tolist() == got.voffsets.tolist()
    spans = [(0, 1, 2), (0, 3, 4), (1, 5, 6), (2, 7, 8)]
    assert bgzf._fetch_groups(spans, [[0], [0, 10], [20], [10]], {0: 50, 10: 60, 20: 70}, 130, 4096) == [(0, 2), (2, 4)]
    assert bgzf._fetch_groups(spans, [[0], [0, 10], [20], [10]], {0: 50, 10: 60, 20: 70}, 1 << 30, 2) == [(0, 3), (3, 4)]
    assert bgzf._fetch_groups(spans[:1], [[0]], {0: 500}, 120, 4096) == [(0, 1)]

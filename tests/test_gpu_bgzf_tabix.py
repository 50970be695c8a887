"""GPU: BGZF by region -- TabixIndex.build against the referee's index (tests/tabix_ref.py) on VCF, BED and GFF files with the corner
cases of the line model, in blocks of 37, 1001 and 65280 bytes and as two concatenated streams; window cuts; the errors; fetch against
brute force; and the contract of the two engine calls through _lib."""
import gzip
import io

import numpy as np
import pytest

import tabix_files as F
import tabix_ref as R
from test_gpu_bgzf_lines import member_table

pytestmark = pytest.mark.gpu

KINDS = {"vcf": dict(n_names=40, per_name=120), "bed": dict(n_names=5, per_name=1400, crlf=True, junk=3),
         "gff": dict(n_names=12, per_name=400, final_newline=False)}
LAYOUTS = (37, 1001, 65280, "two streams")
_cache = {}


def case(kind, layout=None):
    """-> (text, conf, names, per-line table) and, with a layout, (blob, referee index as a TabixIndex) as well; made once"""
    from zlib_ng_amd import bgzf
    if kind not in _cache:
        rng = np.random.default_rng(sorted(KINDS).index(kind) + 20)
        text, conf, names = F.make_text(kind, rng, **KINDS[kind])
        assert 200 << 10 < len(text) < 900 << 10
        _cache[kind] = (text, conf, names)
    text, conf, names = _cache[kind]
    if layout is None:
        return text, conf, names
    if (kind, layout) not in _cache:
        if layout == "two streams":
            cut = text.index(b"\n", len(text) // 2) - 20          # (the cut lies inside a line)
            blob = bgzf.compress(text[:cut], block_size=4000) + bgzf.compress(text[cut:], block_size=3001)
        else:
            blob = bgzf.compress(text, block_size=layout)
        assert gzip.decompress(blob) == text
        _cache[kind, layout] = (blob, R.table(blob, conf), bgzf.TabixIndex(conf, *R.build(blob, conf)))
    return (text, conf, names) + _cache[kind, layout]


def build_kw(conf):
    kind = {v[:4]: k for k, v in R.PRESETS.items()}[conf[:4]]
    return (kind,), {"skip": conf[5]}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_build_equals_the_referee(kind, layout, tmp_path):
    from zlib_ng_amd import bgzf
    text, conf, names, blob, rows, want = case(kind, layout)
    assert {R.reg2bin(r[4], r[5]) for r in rows} >= {0} and max(r[5] for r in rows) == 1 << 29
    assert {len(n) for n in want.names} >= {1, 200} and 5 <= len(want) <= 40
    args, kw = build_kw(conf)
    path = tmp_path / "f.gz"
    path.write_bytes(blob)
    idx = bgzf.TabixIndex.build(str(path), *args, **kw)
    assert idx.names == want.names and idx.linear == want.linear and idx.bins == want.bins and idx == want
    idx.validate(len(blob))
    idx.save(str(path) + ".tbi")
    assert bgzf.TabixIndex.load(str(path) + ".tbi") == want and bgzf.TabixIndex.from_bytes(idx.to_bytes(compressed=False)) == want
    if kind != "vcf":                                       # the same columns given by keyword
        kw2 = dict(seq_col=conf[1], start_col=conf[2], end_col=conf[3], zero_based=bool(conf[0] & 0x10000), skip=conf[5])
        assert bgzf.TabixIndex.build(io.BytesIO(blob), **kw2) == want


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_window_cuts(kind, ctx, monkeypatch):
    """small windows (one byte and the block that is read beyond it: 64 KiB of a file of 37-byte blocks): the same index"""
    from zlib_ng_amd import bgzf
    text, conf, names, blob, rows, want = case(kind, 37)
    calls = []
    real = type(ctx).bgzf_tabix

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        calls.append((a[7] if len(a) > 7 else k.get("line_base", 0), out[2].data))
        return out
    monkeypatch.setattr(type(ctx), "bgzf_tabix", spy)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    args, kw = build_kw(conf)
    assert bgzf.TabixIndex.build(io.BytesIO(blob), *args, **kw) == want
    assert len(calls) >= 4 and sum(1 for _, d in calls if d) >= 4      # several windows with data lines: cuts between equal names


def _fixed_bed(n):
    """n BED lines of one name and of equal length (zero-padded coordinates): swapping two of them moves no byte of a stored block"""
    return [b"c\t%09d\t%09d" % (100 * i, 100 * i + 50) for i in range(n)]


def test_order_is_checked_across_a_window_cut(ctx, monkeypatch):
    from zlib_ng_amd import bgzf
    lines = _fixed_bed(6000)
    calls = []
    real = type(ctx).bgzf_tabix

    def spy(self, *a, **k):
        calls.append(a[7] if len(a) > 7 else k.get("line_base", 0))
        return real(self, *a, **k)
    monkeypatch.setattr(type(ctx), "bgzf_tabix", spy)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    blob = bgzf.compress(b"\n".join(lines) + b"\n", 0, block_size=37)
    bgzf.TabixIndex.build(io.BytesIO(blob), "bed")
    assert len(calls) >= 3
    cut = calls[1]                                          # the number of the first line of the second window
    assert 1 <= cut < len(lines) - 1
    lines[cut - 1], lines[cut] = lines[cut], lines[cut - 1]            # line `cut` now starts below the line in front of it
    bad = b"\n".join(lines) + b"\n"
    blob2 = bgzf.compress(bad, 0, block_size=37)
    assert len(blob2) == len(blob)
    with pytest.raises(R.RefBad) as ref:
        R.table(blob2, R.PRESETS["bed"])
    assert (ref.value.number, ref.value.kind) == (cut, 4)
    calls.clear()
    with pytest.raises(ValueError, match=r"line %d at virtual offset %d " % (cut, R.Voffsets(blob2)(cut * len(lines[0] + b"\n")))):
        bgzf.TabixIndex.build(io.BytesIO(blob2), "bed")
    assert calls[:2] == [0, cut]                            # the pair was cut apart: the first window saw nothing wrong


def _with_line(text, where, line):
    lines = text.split(b"\n")
    data = [i for i, ln in enumerate(lines) if ln and not ln.startswith(b"#")]
    lines.insert(data[where], line)
    return b"\n".join(lines)


@pytest.mark.parametrize("kind", [1, 2, 3, 4, "contig", "vcf columns", "vcf range"])
def test_bad_lines_name_the_referees_line(kind, monkeypatch):
    from zlib_ng_amd import bgzf
    rng = np.random.default_rng(31)
    vcf = str(kind).startswith("vcf")
    text, conf, names = F.make_text("vcf" if vcf else "bed", rng, n_names=4, per_name=700)
    n = text.count(b"\n")
    line = {1: b"chr2\t5", 2: b"chr2\t5\t1x", 3: b"chr2\t5\t%d" % (2 ** 29 + 1), 4: b"1\t0\t1", "contig": b"1\t%d\t%d" % (2 ** 29 - 1, 2 ** 29),
            "vcf columns": b"chr2\t77\trs", "vcf range": b"chr2\t77\trs\tA\tT\t.\t.\tEND=%d" % (2 ** 29 + 1)}[kind]
    where = {4: 300, "contig": 1500}.get(kind, 1600)
    first = _with_line(text, where, line)
    both = _with_line(first, 2700, b"chr3\tx\ty")           # a second bad line, in a later window
    want_kind = {"vcf columns": 1, "vcf range": 3}.get(kind, kind)
    for bad in (first, both):
        blob = bgzf.compress(bad, block_size=37)
        with pytest.raises(R.RefBad) as ref:
            R.table(blob, conf)
        assert ref.value.kind == want_kind
        at = bad.index(b"\n" + line + b"\n") + 1
        for window in (None, 1):
            if window:
                monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
            with pytest.raises(ValueError, match=r"line %d at virtual offset %d " % (ref.value.number, R.Voffsets(blob)(at))):
                bgzf.TabixIndex.build(io.BytesIO(blob), "vcf" if vcf else "bed")
            monkeypatch.undo()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fetch_against_brute_force(kind, layout, ctx, tmp_path):
    from zlib_ng_amd import bgzf
    text, conf, names, blob, rows, idx = case(kind, layout)
    v = R.Voffsets(blob)
    regions = F.regions_for(np.random.default_rng(41), rows, names, 200)
    want = [R.overlaps(rows, *r) for r in regions]
    assert sum(1 for w in want if not w) > 20 and sum(1 for w in want if w) > 100
    assert any(w and all(R.reg2bin(r[4], r[5]) == 0 for r in w) for w in want)      # a region that only bin-0 features overlap
    path = tmp_path / "f.gz"
    path.write_bytes(blob)
    with bgzf.open(str(path)) as r:
        r.read(1000)
        here = r.tell()
        got = r.fetch(idx, regions)
        counts = r.fetch(idx, regions, count=True)
        assert r.tell() == here and r.read(50) == text[1000:1050]
        assert counts == [len(w) for w in want]
        assert got.region.tolist() == [i for i, w in enumerate(want) for _ in w]
        assert got.voffsets.tolist() == [v(x[1]) for w in want for x in w]
        assert bytes(got.data) == b"".join(text[x[1]:x[1] + x[2]] for w in want for x in w)
        assert list(got)[:50] == [text[x[1]:x[1] + x[2]] for w in want for x in w][:50] and got.of(2) == [text[x[1]:x[1] + x[2]] for x in want[2]]
        for k in np.random.default_rng(42).integers(0, len(got), 40).tolist():
            r.seek(int(got.voffsets[k]))
            assert r.read(len(got[k])) == got[k]
        if layout == 1001:                                  # singly: strings and tuples, lines and counts
            for i, (reg, w) in enumerate(zip(regions, want)):
                one = r.fetch(idx, reg) if i % 2 else bgzf.fetch(str(path), idx, reg)
                assert list(one) == [text[x[1]:x[1] + x[2]] for x in w] and one.voffsets.tolist() == [v(x[1]) for x in w], reg
                if i % 5 == 0:
                    assert r.fetch(idx, reg, count=True) == len(w)
            name = names[3].decode()
            assert list(r.fetch(idx, name + ":1,000-2,000,000")) == [text[x[1]:x[1] + x[2]] for x in R.overlaps(rows, names[3], 999, 2000000)]
        if layout == 65280:                                 # a narrow region decodes the blocks its chunks touch and no others
            nblocks = sum(1 for b in R.blocks_of(blob) if b[2])
            mine = [x for x in rows if x[3] == names[-1]]
            reg = (names[-1], mine[len(mine) // 2][4], mine[len(mine) // 2][4] + 100)
            touched = {c for vb, ve in idx.chunks(*reg) for c, cs, isz in R.blocks_of(blob) if isz and vb >> 16 <= c and (c << 16) < ve}
            ctx.bgzf_stats()
            assert len(r.fetch(idx, reg)) == len(R.overlaps(rows, *reg))
            launches, decoded, _ = ctx.bgzf_stats()
            assert nblocks >= 4 and launches == 1 and decoded <= len(touched) < nblocks


def test_fetch_refuses_a_stale_index_and_a_damaged_block(tmp_path):
    from zlib_ng_amd import bgzf
    text, conf, names, blob, rows, idx = case("gff", 1001)
    with pytest.raises(ValueError):
        bgzf.fetch(io.BytesIO(blob[:len(blob) // 2]), idx, names[-1].decode())
    tab = R.blocks_of(blob)
    c, cs, _ = tab[len(tab) // 2]
    hurt = bytearray(blob)
    hurt[c + cs - 12] ^= 0x55                               # inside the deflate data of a block in the middle
    with pytest.raises(bgzf.BadGzipFile, match="offset %d" % c):
        bgzf.fetch(io.BytesIO(bytes(hurt)), idx, [(n, 0, 1 << 29) for n in names])


def _engine_case():
    from zlib_ng_amd import _lib
    text, conf, names, blob, rows, idx = case("vcf", 1001)
    tab = _lib.bgzf_scan(blob)[1]
    return text, conf, names, blob, rows, tab, member_table(tab)


def _same_tables(got, want):
    return all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(got, want))


def test_tabix_entry_point(ctx):
    from zlib_ng_amd import _lib
    text, conf, names, blob, rows, tab, members = _engine_case()
    fake = F.FakeEngine()
    cut = text.index(b"\n", len(text) // 3) + 1             # a line start in the middle
    for lo, hi, flags in ((0, len(text), 4), (cut, len(text) - 7, 0), (cut, len(text) - 7, 4), (0, 0, 4), (cut, cut + 5, 0)):
        ctx.bgzf_stats()
        code, status, tot, *tables = ctx.bgzf_tabix(blob, members, lo, hi, conf, 10, flags, 1000)
        assert ctx.bgzf_stats()[:2] == (1, len(tab))
        _, _, want, *wtables = fake.bgzf_tabix(blob, members, lo, hi, conf, 10, flags, 1000)
        assert code == 0 and not status.any() and tot.covered == 1
        assert (tot.seen, tot.data, tot.tail_off, tot.bad_kind) == (want.seen, want.data, want.tail_off, 0), (lo, hi, flags)
        assert _same_tables(tables, wtables), (lo, hi, flags)
        assert (tot.n_names, tot.name_bytes, tot.n_bins, tot.n_wins) == (len(wtables[0]), len(wtables[1]), len(wtables[2]), len(wtables[3]))
        if want.data:
            assert (tot.first_beg, tot.last_beg, tot.first_line) == (want.first_beg, want.last_beg, int(wtables[0]["line"][0]))
    # the sizing protocol: a short capacity gives the totals and writes nothing
    code, status, tot, *tables = ctx.bgzf_tabix(blob, members, 0, len(text), conf, 10, 4, 0)
    caps = (tot.n_names, tot.name_bytes, tot.n_bins, tot.n_wins)
    assert min(caps) > 0
    for k in range(4):
        short = tuple(c - (1 if i == k else 0) for i, c in enumerate(caps))
        code, status, t2, *none = ctx.bgzf_tabix(blob, members, 0, len(text), conf, 10, 4, 0, short)
        assert code == _lib.BUF_ERROR and (t2.n_names, t2.name_bytes, t2.n_bins, t2.n_wins, t2.seen, t2.covered) == caps + (tot.seen, 1)
        assert all(len(x) == 0 for x in none)
    code, status, t2, *exact = ctx.bgzf_tabix(blob, members, 0, len(text), conf, 10, 4, 0, caps)
    assert code == 0 and _same_tables(exact, tables)
    # a member table with a gap: not covered, nothing reported
    code, status, tot, *tables = ctx.bgzf_tabix(blob, np.delete(members, 7), 0, len(text), conf, 10, 4, 0)
    assert code == 0 and (tot.covered, tot.seen, tot.data, tot.n_names, tot.n_bins, tot.n_wins) == (0, 0, 0, 0, 0, 0) and all(len(x) == 0 for x in tables)
    for bad_conf in ((1, 1, 2, 0, 35, 0), (2, 0, 2, 0, 35, 0)):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_tabix(blob, members, 0, len(text), bad_conf, 10, 4, 0)
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_tabix(blob, members, 0, len(text) + 1, conf, 10, 4, 0)


def _spans(text, rows, names, members):
    """regions and spans over the whole decoded text of the engine case: two regions over all of it, one over its second half"""
    from zlib_ng_amd import _lib
    half = text.index(b"\n", len(text) // 2) + 1
    regs = [(names[0], 0, 1 << 29), (names[5], 1000, 1 << 27), (names[-1], 0, 1 << 29)]
    rtab = np.zeros(3, _lib.TABIX_REGION_DTYPE)
    rtab["name_len"] = [len(r[0]) for r in regs]
    rtab["name_off"] = np.cumsum(rtab["name_len"]) - rtab["name_len"]
    rtab["beg"], rtab["end"] = [r[1] for r in regs], [r[2] for r in regs]
    stab = np.array([(0, len(text), 0, 0), (0, half, 1, 0), (half, len(text), 2, 0)], _lib.TABIX_SPAN_DTYPE)
    return b"".join(r[0] for r in regs), rtab, stab


def test_fetch_entry_point(ctx):
    from zlib_ng_amd import _lib
    text, conf, names, blob, rows, tab, members = _engine_case()
    nblob, rtab, stab = _spans(text, rows, names, members)
    fake = F.FakeEngine()
    _, _, _, wrows_per, wtot, wrows, wpacked = fake.bgzf_fetch(blob, members, conf, 10, 0, nblob, rtab, stab)
    assert wtot.matched > 100 and all(wrows_per)
    code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, members, conf, 10, 0, nblob, rtab, stab)
    assert code == 0 and not status.any() and not sstat.any() and srows.tolist() == wrows_per.tolist()
    assert (tot.matched, tot.bytes) == (wtot.matched, wtot.bytes) and np.array_equal(got, wrows) and packed == wpacked
    code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, members, conf, 10, _lib.BGZF_FETCH_COUNT_ONLY, nblob, rtab, stab)
    assert code == 0 and srows.tolist() == wrows_per.tolist() and tot.matched == wtot.matched and len(got) == 0 and packed == b""
    # a span out of bounds, one that names no region, one that a failed block touches: their verdicts, and the others are answered
    wild = np.concatenate([stab[:1], np.array([(5, len(text) + 1, 0, 0), (0, 10, 3, 0), (9, 3, 1, 0)], _lib.TABIX_SPAN_DTYPE), stab[1:]])
    code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, members, conf, 10, 0, nblob, rtab, wild)
    assert code == 0 and sstat.tolist() == [0, _lib.BGZF_SLICE_TABLE, _lib.BGZF_SLICE_TABLE, _lib.BGZF_SLICE_TABLE, 0, 0]
    assert srows.tolist() == [wrows_per[0], 0, 0, 0, wrows_per[1], wrows_per[2]] and np.array_equal(got, wrows) and packed == wpacked
    hostile = members.copy()
    hostile["in_off"][len(members) - 2] = len(blob) + 1000
    code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, hostile, conf, 10, 0, nblob, rtab, stab)
    assert code == 0 and status[len(members) - 2] != 0 and sstat.tolist() == [_lib.BGZF_SLICE_BLOCK, 0, _lib.BGZF_SLICE_BLOCK]
    assert srows.tolist() == [0, wrows_per[1], 0] and packed == b"".join(text[int(r["src_off"]):int(r["src_off"] + r["len"])] for r in wrows if r["region"] == 1)
    code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, np.delete(members, 3), conf, 10, 0, nblob, rtab, stab)
    assert code == 0 and sstat.tolist() == [_lib.BGZF_SLICE_BLOCK, _lib.BGZF_SLICE_BLOCK, 0] and srows.tolist() == [0, 0, wrows_per[2]]
    # the sizing protocol
    for caps in ((wtot.matched - 1, wtot.bytes), (wtot.matched, wtot.bytes - 1), (0, 0)):
        code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, members, conf, 10, 0, nblob, rtab, stab, caps)
        assert code == _lib.BUF_ERROR and (tot.matched, tot.bytes) == (wtot.matched, wtot.bytes) and len(got) == 0 and packed == b""
    code, status, sstat, srows, tot, got, packed = ctx.bgzf_fetch(blob, members, conf, 10, 0, nblob, rtab, stab, (wtot.matched, wtot.bytes))
    assert code == 0 and np.array_equal(got, wrows) and packed == wpacked
    for bad in (dict(regions=rtab[:0]), dict(names=nblob[:-1]), dict(conf=(1, 1, 2, 0, 35, 0))):
        kw = dict(conf=conf, names=nblob, regions=rtab)
        kw.update(bad)
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_fetch(blob, members, kw["conf"], 10, 0, kw["names"], kw["regions"], stab)


def test_device_forms(ctx):
    from zlib_ng_amd import _lib, devmem
    text, conf, names, blob, rows, tab, members = _engine_case()
    n, cap = len(tab), len(text)
    _, _, want, wn, wblob, wb, ww = ctx.bgzf_tabix(blob, members, 0, len(text), conf, 10, 4, 5)
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, cap), devmem.empty(ctx, 4 * n)
    d_n, d_b = devmem.empty(ctx, 32 * len(wn)).zero_(), devmem.empty(ctx, len(wblob)).zero_()
    d_bins, d_w = devmem.empty(ctx, 40 * len(wb)).zero_(), devmem.empty(ctx, 16 * len(ww)).zero_()
    args = (d_in.ptr, len(blob), d_m.ptr, n, 0, len(text), conf, 10, 4, 5, d_scratch.ptr, cap, d_st.ptr)
    code, tot = ctx.bgzf_tabix_dev(*args, d_n.ptr, len(wn), d_b.ptr, len(wblob), d_bins.ptr, len(wb) - 1, d_w.ptr, len(ww))
    assert code == _lib.BUF_ERROR and (tot.n_names, tot.n_bins, tot.n_wins, tot.seen, tot.covered) == (len(wn), len(wb), len(ww), want.seen, 1)
    assert d_n.cpu().tobytes() == bytes(32 * len(wn)) and d_bins.cpu().tobytes() == bytes(40 * len(wb))
    code, tot = ctx.bgzf_tabix_dev(*args, d_n.ptr, len(wn), d_b.ptr, len(wblob), d_bins.ptr, len(wb), d_w.ptr, len(ww))
    assert code == 0 and (tot.seen, tot.data, tot.tail_off, tot.covered) == (want.seen, want.data, want.tail_off, 1)
    assert np.array_equal(d_n.cpu(_lib.TABIX_NAME_DTYPE), wn) and d_b.cpu().tobytes() == wblob
    assert np.array_equal(d_bins.cpu(_lib.TABIX_BIN_DTYPE), wb) and np.array_equal(d_w.cpu(_lib.TABIX_WIN_DTYPE), ww)
    assert not d_st.cpu(np.int32).any()
    nblob, rtab, stab = _spans(text, rows, names, members)
    _, _, _, wper, wtot, wrows, wpacked = ctx.bgzf_fetch(blob, members, conf, 10, 0, nblob, rtab, stab)
    d_sp, d_ss, d_sr = devmem.from_host(ctx, stab.tobytes()), devmem.empty(ctx, 4 * len(stab)), devmem.empty(ctx, 4 * len(stab))
    d_rows, d_out = devmem.empty(ctx, 16 * len(wrows)).zero_(), devmem.empty(ctx, len(wpacked)).zero_()
    args = (d_in.ptr, len(blob), d_m.ptr, n, conf, 10, 0, nblob, rtab, d_sp.ptr, len(stab), d_scratch.ptr, cap, d_st.ptr, d_ss.ptr, d_sr.ptr)
    code, tot = ctx.bgzf_fetch_dev(*args, d_rows.ptr, len(wrows) - 1, d_out.ptr, len(wpacked))
    assert code == _lib.BUF_ERROR and (tot.matched, tot.bytes) == (len(wrows), len(wpacked)) and d_out.cpu().tobytes() == bytes(len(wpacked))
    code, tot = ctx.bgzf_fetch_dev(*args, d_rows.ptr, len(wrows), d_out.ptr, len(wpacked))
    assert code == 0 and (tot.matched, tot.bytes) == (len(wrows), len(wpacked))
    assert np.array_equal(d_rows.cpu(_lib.TABIX_ROW_DTYPE), wrows) and d_out.cpu().tobytes() == wpacked
    assert d_sr.cpu(np.uint32).tolist() == wper.tolist() and not d_ss.cpu(np.int32).any()

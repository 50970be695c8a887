"""GPU: BGZF by sequence -- FaidxIndex.build against the referee (tests/faidx_ref.py) on FASTA files with the corner cases of the
line model, in blocks of 64 and 4 096 bytes (stored) and as the library's own writer leaves them; window cuts and the carry; the bad
lines; fetch_seq against plain slicing; a stale index and a damaged block; and the contract of the two engine calls through _lib."""
import gzip
import io

import numpy as np
import pytest

import faidx_files as F
import faidx_ref as R
import tabix_ref
from test_gpu_bgzf_lines import member_table

pytestmark = pytest.mark.gpu

# line bases, CRLF, final newline, trailing empty lines
SHAPES = {"lb1": (1, False, True, 0), "lb60crlf": (60, True, True, 2), "lb63": (63, False, False, 0), "lb64crlf": (64, True, False, 0),
          "lb70": (70, False, True, 3)}
LAYOUTS = (64, 4096, "writer")
_cache = {}


def pack(text, layout):
    from zlib_ng_amd import bgzf
    blob = bgzf.compress(text, 6) if layout == "writer" else F.host_bgzf(text, layout, level=0)
    assert gzip.decompress(blob) == text
    return blob


def case(shape, layout=None):
    """-> (text, referee rows) and, with a layout, the blob as well; made once.  Every text holds one sequence of more than 65 536
    bases behind the corner cases."""
    if shape not in _cache:
        lb, crlf, final_newline, trailing = SHAPES[shape]
        rng = np.random.default_rng(sorted(SHAPES).index(shape) + 40)
        eol = b"\r\n" if crlf else b"\n"
        big = eol.join(F.record(b"big", F.bases(rng, 70_000), lb, eol, b"more than one span")) + eol
        text = big + F.make_fasta(rng, lb, crlf, final_newline, trailing, total=130_000)
        verdict, rows = R.index(text)
        assert verdict == "ok" and 200_000 < len(text) < 450_000
        _cache[shape] = (text, rows)
    text, rows = _cache[shape]
    if layout is None:
        return text, rows
    if (shape, layout) not in _cache:
        _cache[shape, layout] = pack(text, layout)
    return text, rows, _cache[shape, layout]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_build_equals_the_referee(shape, layout, tmp_path):
    from zlib_ng_amd import bgzf
    text, rows, blob = case(shape, layout)
    lb = SHAPES[shape][0]
    assert {r[1] for r in rows} >= {0, 1, lb, lb + 1, 5 * lb, 70_000} and {len(r[0]) for r in rows} >= {1, 200}
    path = tmp_path / "f.fa.gz"
    path.write_bytes(blob)
    idx = bgzf.FaidxIndex.build(str(path))
    assert idx.names == [r[0] for r in rows] and [idx[r[0]] for r in rows] == [r[1:] for r in rows] and idx == bgzf.FaidxIndex(rows)
    assert idx.to_bytes() == b"".join(b"%s\t%d\t%d\t%d\t%d\n" % r for r in rows)
    assert idx.gzi == bgzf.GziIndex.build(str(path))
    idx.save(str(path) + ".fai", str(path) + ".gzi")
    back = bgzf.FaidxIndex.load(str(path) + ".fai", str(path) + ".gzi")
    assert back == idx and back.gzi == idx.gzi and bgzf.FaidxIndex.build(io.BytesIO(blob)) == idx


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_sequence_on_a_single_line(layout):
    """300 000 bases without a line end: 18 tiles, several blocks; and the same with a second record behind it"""
    from zlib_ng_amd import bgzf
    rng = np.random.default_rng(7)
    seq = F.bases(rng, 300_000)
    for text in (b">chrL one line\n" + seq + b"\n", b">chrL\n" + seq, b">chrL\r\n" + seq + b"\r\n>next\r\nACGT\r\n"):
        verdict, rows = R.index(text)
        assert verdict == "ok" and rows[0][1:4] == (300_000, text.index(b"\n") + 1, 300_000)
        idx = bgzf.FaidxIndex.build(io.BytesIO(pack(text, layout)))
        assert idx == bgzf.FaidxIndex(rows) and idx["chrL"][0] == 300_000


def _spy(ctx, monkeypatch, calls):
    real = type(ctx).bgzf_faidx

    def spy(self, *a, **k):
        out = real(self, *a, **k)
        calls.append((a[6] if len(a) > 6 else k.get("line_base", 0), out[2].seen, out[2].records, out[2].carry.flags))
        return out
    monkeypatch.setattr(type(ctx), "bgzf_faidx", spy)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_window_cuts(shape, ctx, monkeypatch):
    """small windows (one byte and the block that is read beyond it: 64 KiB of a file of 64-byte blocks): the same index; the sequence
    of 70 000 bases spans more than one window"""
    from zlib_ng_amd import bgzf
    text, rows, blob = case(shape, 64)
    calls, gzi = [], bgzf.GziIndex.build(io.BytesIO(blob))
    _spy(ctx, monkeypatch, calls)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    idx = bgzf.FaidxIndex.build(io.BytesIO(blob))
    assert idx == bgzf.FaidxIndex(rows) and idx.gzi == gzi
    assert len(calls) >= 4 and sum(c[1] for c in calls) == len(R.lines_of(text)) and calls[0][2] == 1 and calls[0][3] & 1


def _fixed(n, per=400):
    """n lines of 16 bytes each: a header every `per` lines, sequence lines of 15 bases"""
    return [b">h%013d" % i if i % per == 0 else b"ACGTACGTACGTACG" for i in range(n)]


def _cuts(ctx, monkeypatch, lines):
    """the numbers of the first lines of the windows when the file of these lines is read in windows of one block and a bit"""
    from zlib_ng_amd import bgzf
    calls = []
    _spy(ctx, monkeypatch, calls)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    blob = F.host_bgzf(b"\n".join(lines) + b"\n", 64, level=0)
    try:
        bgzf.FaidxIndex.build(io.BytesIO(blob))
    except ValueError:
        pass
    return [c[0] for c in calls]


def test_a_sequence_over_three_windows_and_a_header_that_ends_a_window(ctx, monkeypatch):
    from zlib_ng_amd import bgzf
    lines = _fixed(14_000, per=13_000)                      # the first sequence: 13 000 lines, 208 000 bytes
    cuts = _cuts(ctx, monkeypatch, lines)
    assert len(cuts) >= 4 and cuts[3] < 13_000               # it spans the first three windows and more
    lines[cuts[1] - 1] = b">lastofwindow00"                  # a header as a window's last line: its first non-empty line is the next window's
    lines[cuts[2] - 2] = b">twobeforecut00"                  # one whose only line in its window is its first
    text = b"\n".join(lines) + b"\n"
    verdict, rows = R.index(text)
    assert verdict == "ok" and len(rows) == 4 and rows[1][0] == b"lastofwindow00" and rows[1][3:] == (15, 16)
    assert _cuts(ctx, monkeypatch, lines)[:3] == cuts[:3]
    monkeypatch.undo()
    calls = []
    _spy(ctx, monkeypatch, calls)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    assert bgzf.FaidxIndex.build(io.BytesIO(F.host_bgzf(text, 64, level=0))) == bgzf.FaidxIndex(rows)
    assert calls[1][0] == cuts[1] and calls[0][2] == 2 and calls[2][2] == 0      # (the third window holds no header at all)
    monkeypatch.undo()
    assert bgzf.FaidxIndex.build(io.BytesIO(F.host_bgzf(text, 4096, level=0))) == bgzf.FaidxIndex(rows)


def _expect_bad(text, kind, monkeypatch, layout=64, line=None):
    from zlib_ng_amd import bgzf
    verdict, ref_line, ref_kind = R.index(text)
    assert (verdict, ref_kind) == ("bad", kind) and (line is None or ref_line == line), (verdict, ref_line, ref_kind)
    blob = F.host_bgzf(text, layout, level=0)
    v = tabix_ref.Voffsets(blob)(R.line_start(text, ref_line))
    for window in (None, 1):
        if window:
            monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        with pytest.raises(ValueError, match=r"line %d at virtual offset %d " % (ref_line, v)) as e:
            bgzf.FaidxIndex.build(io.BytesIO(blob))
        assert (e.value.line, e.value.kind, e.value.voffset) == (ref_line, kind, v)
        monkeypatch.undo()


BAD_LINE = {1: b">  no name here", 2: b"ACGTACG ACGTACG", 3: b"ACGTACGTACGT", 4: b""}


@pytest.mark.parametrize("where", ["first", "tile", "word"])
@pytest.mark.parametrize("kind", [1, 2, 3, 4, 5])
def test_bad_lines_name_the_referees_line(kind, where, monkeypatch):
    """the file's first line that can be bad in this way; the line that starts at scratch offset 16 384, a tile's first; a line that
    lies across a 64-byte word (the lines of 16 bytes behind a first line of 3)"""
    if kind == 5:
        text = {"first": b"ACGT\n", "tile": b"\n" * 16_384 + b"ACGT\n", "word": b"\n" * 60 + b"ACGTACGTAC\n"}[where] + b">a\nACGT\n" * 3000
        return _expect_bad(text, 5, monkeypatch, line={"first": 0, "tile": 16_384, "word": 60}[where])
    lines = _fixed(16_000)
    if where == "word":
        lines[0] = b">a"                                     # every later line starts at 3 + 16 k: one in four lies across a word
    at = {"first": {1: 0, 2: 1, 3: 2, 4: 1}[kind], "tile": 1024, "word": 1028}[where]
    assert where != "tile" or sum(len(x) + 1 for x in lines[:at]) == 16_384
    assert where != "word" or sum(len(x) + 1 for x in lines[:at]) % 64 > 48
    lines[at] = BAD_LINE[kind]
    _expect_bad(b"\n".join(lines) + b"\n", kind, monkeypatch, line=at)


@pytest.mark.parametrize("kind", [3, 4])
def test_the_carry_catches_what_a_window_cut_separates(kind, ctx, monkeypatch):
    """the window's last line is judged by what the next window begins with"""
    from zlib_ng_amd import bgzf
    lines = _fixed(16_000)
    cut = _cuts(ctx, monkeypatch, lines)[1]
    monkeypatch.undo()
    assert cut % 400 > 2
    # the same bytes per line, so the cut stays: a middle line of 14 bases and a CR; sixteen empty lines in place of one line
    lines[cut - 1] = b"ACGTACGTACGTAC\r" if kind == 3 else b"\n" * 15
    text = b"\n".join(lines) + b"\n"
    assert len(text) == 16 * 16_000
    calls = []
    _spy(ctx, monkeypatch, calls)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    with pytest.raises(ValueError) as e:
        bgzf.FaidxIndex.build(io.BytesIO(F.host_bgzf(text, 64, level=0)))
    assert len(calls) == 2 and calls[1][0] == cut + (15 if kind == 4 else 0) and calls[0][3] == (1 if kind == 3 else 3)
    monkeypatch.undo()
    assert (e.value.line, e.value.kind) == (cut - 1, kind)
    _expect_bad(text, kind, monkeypatch, line=cut - 1)


def test_two_faults_and_a_duplicate_name(monkeypatch):
    from zlib_ng_amd import bgzf
    lines = _fixed(4000)
    lines[900], lines[700] = BAD_LINE[2], BAD_LINE[3]
    _expect_bad(b"\n".join(lines) + b"\n", 3, monkeypatch, line=700)
    lines = _fixed(9000)
    lines[8000] = lines[400]
    blob = F.host_bgzf(b"\n".join(lines) + b"\n", 64, level=0)
    for window in (None, 1):
        if window:
            monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        with pytest.raises(ValueError, match=r"occurs twice: header lines 400 and 8000"):
            bgzf.FaidxIndex.build(io.BytesIO(blob))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fetch_seq_against_the_referee(shape, layout, ctx, tmp_path):
    from zlib_ng_amd import bgzf
    text, rows, blob = case(shape, layout)
    by = {r[0]: r[1:] for r in rows}
    rng = np.random.default_rng(3)
    regs = F.regions_for(rng, rows, 296) + [(b"big", 11, 69_990), ("big", 0, None), "big:65,000-66,000", "1"]
    idx = bgzf.FaidxIndex(rows, bgzf.GziIndex.build(io.BytesIO(blob)))
    path = tmp_path / "f.fa.gz"
    path.write_bytes(blob)
    with bgzf.open(str(path)) as r:
        for rc in (False, True):
            ctx.bgzf_stats()
            got = r.fetch_seq(idx, regs, reverse_complement=rc)
            launches, decoded, _ = ctx.bgzf_stats()
            assert len(got) == 300 and launches == 1 and decoded <= len(idx.gzi) + 1
            for k, reg in enumerate(regs):
                name, beg, end = bgzf.parse_region(reg if not (isinstance(reg, tuple) and reg[2] is None) else (reg[0], reg[1], 1 << 40))
                end = 1 << 40 if reg == "1" else end
                assert got[k] == R.subseq(text, by[name], beg, end, rc), (k, reg, rc)
            assert int(got.offsets[-1]) == len(got.data) == sum(len(x) for x in got)
    assert bgzf.fetch_seq(str(path), bgzf.FaidxIndex(rows), ("big", 5, 300), reverse_complement=True)[0] == R.subseq(text, by[b"big"], 5, 300, True)
    assert set(b"ATUCGRYKMBVDHatucgrykmbvdh") <= set(R.subseq(text, by[b"big"], 0, 70_000))


def test_fetch_seq_refuses_a_stale_index_and_a_damaged_block():
    from zlib_ng_amd import bgzf
    text, rows, blob = case("lb70", 4096)
    with pytest.raises(ValueError, match="faidx index does not match the file"):      # (the device finds line ends among the bases)
        bgzf.fetch_seq(io.BytesIO(blob), bgzf.FaidxIndex([(n, ln, off, lb, lw + 1) for n, ln, off, lb, lw in rows]), ("big", 0, 5000))
    with pytest.raises(ValueError, match="faidx index does not match the file"):      # (the host finds blocks of other sizes)
        bgzf.fetch_seq(io.BytesIO(pack(text, 64)), bgzf.FaidxIndex(rows, bgzf.GziIndex.build(io.BytesIO(blob))), ("big", 0, 5000))
    with pytest.raises(ValueError, match="does not fit"):
        bgzf.fetch_seq(io.BytesIO(blob), bgzf.FaidxIndex([(b"far", 100, len(text) + 64, 70, 71)]), "far")
    tab = tabix_ref.blocks_of(blob)
    c, cs, _ = tab[5]
    hurt = bytearray(blob)
    hurt[c + cs - 12] ^= 0x55                               # inside the stored data of a block that holds bases of `big`
    idx = bgzf.FaidxIndex(rows, bgzf.GziIndex.build(io.BytesIO(blob)))
    with pytest.raises(bgzf.BadGzipFile, match="offset %d" % c):
        bgzf.fetch_seq(io.BytesIO(bytes(hurt)), idx, ("big", 0, 60_000))
    assert bgzf.fetch_seq(io.BytesIO(bytes(hurt)), idx, ("big", 0, 100))[0] == R.subseq(text, rows[0][1:], 0, 100)


def _engine_case():
    from zlib_ng_amd import _lib
    text, rows, blob = case("lb60crlf", 4096)
    tab = _lib.bgzf_scan(blob)[1]
    return text, rows, blob, tab, member_table(tab)


def _totals(t):
    c = t.carry
    return (t.seen, t.records, t.tail_off, t.head_bases, t.name_bytes, t.bad_kind, t.covered, t.head_line_bases, t.head_line_width,
            c.flags, c.first_bases, c.first_width, c.last_bases, c.last_width, c.last_line if c.flags else 0)


def test_faidx_entry_point(ctx):
    from zlib_ng_amd import _lib
    text, rows, blob, tab, members = _engine_case()
    fake = F.FakeEngine()
    cut = text.index(b"\n", len(text) // 3) + 1             # a line start inside the sequence of 70 000 bases
    carry = _lib.FaidxCarry(999, 60, 62, 60, 62, 1, 0)
    for lo, hi, flags, cin in ((0, len(text), 4, None), (0, cut + 7, 0, None), (cut, len(text) - 3, 0, carry), (cut, len(text), 4, carry), (0, 0, 0, carry),
                               (0, 0, 4, None), (cut, cut + 5, 0, carry)):
        ctx.bgzf_stats()
        code, status, tot, got, names = ctx.bgzf_faidx(blob, members, lo, hi, 10, flags, 1000, cin)
        assert ctx.bgzf_stats()[:2] == (1, len(tab))
        _, _, want, wrows, wnames = fake.bgzf_faidx(blob, members, lo, hi, 10, flags, 1000, cin)
        assert code == 0 and not status.any() and _totals(tot) == _totals(want), (lo, hi, flags)
        assert np.array_equal(got, wrows) and names == wnames, (lo, hi, flags)
        if tot.carry.flags and tot.carry.last_line >= 1000:
            assert tot.carry.reserved == want.carry.reserved
    # the sizing protocol: a short capacity gives the totals and writes nothing
    code, status, tot, got, names = ctx.bgzf_faidx(blob, members, 0, len(text), 10, 4, 0)
    assert tot.records == len(rows) and names == b"".join(r[0] for r in rows)
    for caps in ((tot.records - 1, tot.name_bytes), (tot.records, tot.name_bytes - 1), (0, 0)):
        code, status, t2, none, nothing = ctx.bgzf_faidx(blob, members, 0, len(text), 10, 4, 0, None, caps)
        assert code == _lib.BUF_ERROR and _totals(t2) == _totals(tot) and len(none) == 0 and nothing == b""
    code, status, t2, exact, same = ctx.bgzf_faidx(blob, members, 0, len(text), 10, 4, 0, None, (tot.records, tot.name_bytes))
    assert code == 0 and np.array_equal(exact, got) and same == names
    # a member table with a gap: not covered, nothing reported, the carry comes back
    code, status, tot, got, names = ctx.bgzf_faidx(blob, np.delete(members, 7), 0, len(text), 10, 4, 0, carry)
    assert code == 0 and (tot.covered, tot.seen, tot.records, tot.carry.last_line) == (0, 0, 0, 999) and len(got) == 0 and names == b""
    for delim, flags in ((9, 4), (10, 1)):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_faidx(blob, members, 0, len(text), delim, flags, 0)
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_faidx(blob, members, 0, len(text) + 1, 10, 4, 0)


def _spans_case(text, rows):
    """good spans over the first sequence (60 bases per line of 62 bytes) and hostile ones"""
    from zlib_ng_amd import _lib
    off = rows[0][2]
    good = [(off, 0, 60, 0, 60, 62, 0, 0), (off + 62 * 3 + 7, 60, 500, 7, 60, 62, 1, 0), (off + 59, 560, 65_536, 59, 60, 62, 0, 0), (off, 66_096, 0, 0, 60, 62, 0, 0),
            (off + 5, 66_096, 1, 5, 60, 62, 1, 0)]
    cap = 66_097
    wild = [(len(text), 0, 1, 0, 60, 62, 0, 0), (1 << 62, 0, 1, 0, 60, 62, 0, 0), (off, cap, 1, 0, 60, 62, 0, 0), (off, 1 << 63, 1, 0, 60, 62, 0, 0),
            (off, 0, 60, 0, 0, 62, 0, 0), (off, 0, 60, 0, 60, 59, 0, 0), (off, 0, 60, 60, 60, 62, 0, 0), (off, 0, 65_537, 0, 60, 62, 0, 0),
            (3, 0, 10, 5, 60, 62, 0, 0), (len(text) - 30, 0, 60, 0, 60, 62, 0, 0), (off, 0, 65_536, 0, 1, 0xFFFFFFFF, 0, 0)]
    return np.array(good, _lib.FAIDX_SPAN_DTYPE), np.array(wild, _lib.FAIDX_SPAN_DTYPE), cap


def _want_bases(text, sp):
    n, col, lb, lw, src = (int(sp[x]) for x in ("n", "col", "line_bases", "line_width", "src_off"))
    got = bytes(text[src - col + (col + j) // lb * lw + (col + j) % lb] for j in range(n))
    return got.translate(R.COMPLEMENT)[::-1] if int(sp["flags"]) & 1 else got


def test_fetch_entry_point_and_device_forms(ctx):
    from zlib_ng_amd import _lib, devmem
    text, rows, blob, tab, members = _engine_case()
    good, wild, cap = _spans_case(text, rows)
    want = bytearray(cap)
    for sp in good:
        want[int(sp["dst_off"]):int(sp["dst_off"] + sp["n"])] = _want_bases(text, sp)
    status, sstat, out = ctx.bgzf_faidx_fetch(blob, members, good, cap)
    assert not status.any() and not sstat.any() and out == bytes(want)
    # hostile spans get _TABLE and nothing of theirs is written: a guard pattern around and under the output
    n = len(tab)
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, len(text)), devmem.empty(ctx, 4 * n)
    both = np.concatenate([wild, good])
    d_sp, d_ss = devmem.from_host(ctx, both.tobytes()), devmem.empty(ctx, 4 * len(both))
    d_out = devmem.from_host(ctx, b"\xa5" * (cap + 4096))
    ctx.bgzf_faidx_fetch_dev(d_in.ptr, len(blob), d_m.ptr, n, d_sp.ptr, len(both), d_scratch.ptr, len(text), d_out.ptr + 2048, cap, d_st.ptr, d_ss.ptr)
    assert d_ss.cpu(np.int32).tolist() == [_lib.BGZF_SLICE_TABLE] * len(wild) + [0] * len(good) and not d_st.cpu(np.int32).any()
    assert d_out.cpu().tobytes() == b"\xa5" * 2048 + bytes(want) + b"\xa5" * 2048
    d_out = devmem.from_host(ctx, b"\xa5" * (cap + 4096))
    ctx.bgzf_faidx_fetch_dev(d_in.ptr, len(blob), d_m.ptr, n, d_sp.ptr, len(wild), d_scratch.ptr, len(text), d_out.ptr + 2048, cap, d_st.ptr, d_ss.ptr)
    assert d_out.cpu().tobytes() == b"\xa5" * (cap + 4096)
    # a span over a line end is stale; one that a failed or a missing block touches has _BLOCK and zeros
    off = rows[0][2]
    probe = np.array([(off, 0, 62, 0, 62, 63, 0, 0), (off + 62 * 70, 100, 10, 0, 60, 62, 0, 0), (off, 200, 10, 0, 60, 62, 0, 0)], _lib.FAIDX_SPAN_DTYPE)
    hostile = members.copy()
    hostile["in_off"][1] = len(blob) + 1000
    status, sstat, out = ctx.bgzf_faidx_fetch(blob, hostile, probe, 300)
    assert status[1] != 0 and sstat.tolist() == [_lib.BGZF_SLICE_STALE, _lib.BGZF_SLICE_BLOCK, 0]
    assert out[100:110] == bytes(10) and out[200:210] == text[off:off + 10]
    status, sstat, out = ctx.bgzf_faidx_fetch(blob, np.delete(members, 1), probe, 300)
    assert sstat.tolist() == [_lib.BGZF_SLICE_STALE, _lib.BGZF_SLICE_BLOCK, 0]
    # the build on device pointers: the same rows and names as the host form
    _, _, wtot, wrows, wnames = ctx.bgzf_faidx(blob, members, 0, len(text), 10, 4, 5)
    d_rows, d_b = devmem.empty(ctx, 48 * len(wrows)).zero_(), devmem.empty(ctx, len(wnames)).zero_()
    args = (d_in.ptr, len(blob), d_m.ptr, n, 0, len(text), 10, 4, 5, None, d_scratch.ptr, len(text), d_st.ptr)
    code, tot = ctx.bgzf_faidx_dev(*args, d_rows.ptr, len(wrows) - 1, d_b.ptr, len(wnames))
    assert code == _lib.BUF_ERROR and _totals(tot) == _totals(wtot) and d_rows.cpu().tobytes() == bytes(48 * len(wrows))
    code, tot = ctx.bgzf_faidx_dev(*args, d_rows.ptr, len(wrows), d_b.ptr, len(wnames))
    assert code == 0 and _totals(tot) == _totals(wtot)
    assert np.array_equal(d_rows.cpu(_lib.FAIDX_ROW_DTYPE), wrows) and d_b.cpu().tobytes() == wnames and not d_st.cpu(np.int32).any()

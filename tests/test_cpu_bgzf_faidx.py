"""CPU: BGZF by sequence without a GPU -- the referee pinned with a hand-worked file; the layouts of the binding; argument errors that
need no context; the .fai text as written and as refused; and the window loop (carry included), the duplicate check and the
fetch_seq planner of bgzf.py, driven by a stand-in for the two engine calls (tests/faidx_files.py: FakeEngine) on files written with
the system zlib."""
import ctypes as C
import gzip
import io
import os
import re

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
import faidx_files as F
import faidx_ref as R

HAND = b">one first\nACGT\nAC\n>two\n\n>three\tx\r\nAAA\r\nCCC\r\nG"
HAND_ROWS = [(b"one", 6, 11, 4, 5), (b"two", 0, 24, 0, 0), (b"three", 7, 35, 3, 5)]


def test_referee_pinned_with_literals():
    assert R.index(HAND) == ("ok", HAND_ROWS)
    assert R.lines_of(b"A\r\n\nB") == [(0, 1, 3, b"A"), (3, 0, 1, b""), (4, 1, 1, b"B")]
    assert R.subseq(HAND, HAND_ROWS[2][1:], 2, 7) == b"ACCCG" and R.subseq(HAND, HAND_ROWS[2][1:], 2, 7, True) == b"CGGGT"
    assert R.subseq(HAND, HAND_ROWS[0][1:], 3, 99) == b"TAC" and R.subseq(HAND, HAND_ROWS[1][1:], 0, 5) == b""
    assert b"ACGTURYKMBVDHNacgturykmbvdhn*".translate(R.COMPLEMENT) == b"TGCAAYRMKVBHDNtgcaayrmkvbhdn*"
    bad = lambda text: R.index(text)[1:]
    assert bad(b">\nA\n") == (0, 1) and bad(b"> x\nA\n") == (0, 1) and bad(b">a\nA C\n") == (1, 2) and bad(b">a\nAC\r") == (1, 2)
    assert bad(b">a\nAC\nA\nAC\n") == (2, 3) and bad(b">a\nAC\nACG\n") == (2, 3) and R.index(b">a\nAC\nA\r\n")[0] == "ok"
    assert bad(b">a\nAC\nAC\r\nAC\n") == (2, 3)                       # a middle line of another width
    assert bad(b">a\nAC\n\nAC\n") == (2, 4) and R.index(b">a\nAC\n\n\n>b\n\n")[0] == "ok" and bad(b">a\n\nAC\n") == (1, 4)
    assert bad(b"\n\nAC\n>a\n") == (2, 5) and R.index(b"\n\n>a\nAC")[0] == "ok" and bad(b" \n>a\n") == (0, 2)
    assert bad(b">a\nAC\nA\nAC\n>\n") == (2, 3) and R.index(b">a\nA\n>b\nC\n>a\nG\n") == ("dup", b"a", 0, 4)


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    for name in ("zngamd_bgzf_faidx_dev", "zngamd_bgzf_faidx", "zngamd_bgzf_faidx_fetch_dev", "zngamd_bgzf_faidx_fetch"):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        nargs = len(re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(","))
        assert len(getattr(L, name).argtypes) == nargs, name
    assert C.sizeof(_lib.FaidxCarry) == 32 and _lib.FAIDX_ROW_DTYPE.itemsize == 48 and _lib.FAIDX_SPAN_DTYPE.itemsize == 40
    assert C.sizeof(_lib.BgzfFaidxTotals) == 104 and _lib.BgzfFaidxTotals.carry.offset == 64
    assert (F.ROW, F.SPAN) == (_lib.FAIDX_ROW_DTYPE, _lib.FAIDX_SPAN_DTYPE)
    assert (F.OPEN, F.GAP, F.FINAL, F.RC, F.STALE) == (_lib.FAIDX_OPEN, _lib.FAIDX_GAP, _lib.BGZF_FAIDX_FINAL, _lib.FAIDX_SPAN_RC, _lib.BGZF_SLICE_STALE)
    consts = dict(re.findall(r"#define\s+(ZNGAMD_[A-Z_]+)\s+\(?(-?\d+)u?\)?", header))
    assert int(consts["ZNGAMD_BGZF_SLICE_STALE"]) == _lib.BGZF_SLICE_STALE == 4 and int(consts["ZNGAMD_FAIDX_MAX_SPAN"]) == _lib.FAIDX_MAX_SPAN == 65536
    assert int(consts["ZNGAMD_BGZF_FAIDX_FINAL"]) == _lib.BGZF_FAIDX_FINAL
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES)                            # no kernel class was added
    assert '"za_faidx.hip"' in open(os.path.join(PKG_DIR, "build.py")).read() and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_faidx.hip"))
    assert '#include "za_faidx.hip"' in open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    # a bad delimiter and bad flags are refused before the context is looked at (a NULL context is never touched)
    tot = _lib.BgzfFaidxTotals()
    for delim, flags in ((9, 0), (-1, 0), (256, 0), (10, 1), (10, 8), (10, 4 | 2)):
        args = [None, None, 0, None, 0, 0, 0, delim, flags, 0, None, None, None, 0, None, 0, _lib.ALLOC_FN(), None, C.byref(tot)]
        assert L.zngamd_bgzf_faidx(*args) == _lib.E_ARG, (delim, flags)
        args = [None, None, 0, None, 0, 0, 0, delim, flags, 0, None, None, 0, None, None, 0, None, 0, C.byref(tot)]
        assert L.zngamd_bgzf_faidx_dev(*args) == _lib.E_ARG, (delim, flags)
    assert L.zngamd_bgzf_faidx_fetch(None, None, 0, None, 0, None, 0, None, 0, None, None) == _lib.E_ARG


def test_fai_text_round_trip_and_refusals(tmp_path):
    from zlib_ng_amd import bgzf
    idx = bgzf.FaidxIndex(HAND_ROWS)
    assert idx.to_bytes() == b"one\t6\t11\t4\t5\ntwo\t0\t24\t0\t0\nthree\t7\t35\t3\t5\n"
    assert bgzf.FaidxIndex.from_bytes(idx.to_bytes()) == idx and bgzf.FaidxIndex.from_bytes(idx.to_bytes().replace(b"\n", b"\r\n")) == idx
    assert idx.names == [b"one", b"two", b"three"] and len(idx) == 3 and idx["three"] == (7, 35, 3, 5) and idx[b"one"] == (6, 11, 4, 5)
    assert "two" in idx and "four" not in idx and idx != bgzf.FaidxIndex(HAND_ROWS[:2]) and idx != bgzf.FaidxIndex(HAND_ROWS[::-1])
    with pytest.raises(KeyError):
        idx["four"]
    gzi = bgzf.GziIndex([(100, 65280)])
    both = bgzf.FaidxIndex(HAND_ROWS, gzi)
    both.save(str(tmp_path / "x.fai"), str(tmp_path / "x.gzi"))
    back = bgzf.FaidxIndex.load(str(tmp_path / "x.fai"), str(tmp_path / "x.gzi"))
    assert back == idx and back.gzi == gzi and bgzf.FaidxIndex.load(str(tmp_path / "x.fai")).gzi is None
    buf = io.BytesIO()
    idx.save(buf)
    assert buf.getvalue() == idx.to_bytes() and bgzf.FaidxIndex.load(io.BytesIO(buf.getvalue())) == idx
    with pytest.raises(ValueError, match="holds no gzi"):
        idx.save(str(tmp_path / "y.fai"), str(tmp_path / "y.gzi"))
    with pytest.raises(ValueError, match="FASTQ"):
        bgzf.FaidxIndex.from_bytes(b"r1\t100\t4\t100\t101\t106\n")
    for blob in (b"one\t6\t11\t4\n", b"one\t6\t11\t4\tx\n", b"one\t6\t11\t-4\t5\n", b"one 6 11 4 5\n", b"\t6\t11\t4\t5\n", b"one\t6\t11\t5\t4\n",
                 b"one\t6\t11\t4\t5\none\t6\t30\t4\t5\n", b"one\t6\t11\t4\t5\t\n", b"one\t%d\t11\t4\t5\n" % (1 << 63)):
        with pytest.raises(ValueError):
            bgzf.FaidxIndex.from_bytes(blob)


def _cpu_build(blob, window=None, monkeypatch=None, slack=1200):
    """window: compressed bytes per window; a window is read with room for one more block, which for these files of small blocks
    is cut down with it (no block of theirs is longer than `slack` bytes)"""
    from zlib_ng_amd import bgzf
    if window is not None:
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        monkeypatch.setattr(bgzf, "MAX_BLOCK", slack)
    eng = F.FakeEngine()
    try:
        return bgzf._faidx_build(io.BytesIO(blob), eng), eng
    finally:
        if window is not None:
            monkeypatch.undo()


def test_hand_worked_file_through_the_window_loop(monkeypatch):
    from zlib_ng_amd import bgzf
    blob = F.host_bgzf(HAND, 7, level=0)                     # seven bytes per block: every line is cut
    assert gzip.decompress(blob) == HAND
    idx, eng = _cpu_build(blob)
    assert idx == bgzf.FaidxIndex(HAND_ROWS) and len(eng.calls) == 1 and idx.gzi == bgzf.GziIndex.build(io.BytesIO(blob))
    idx, eng = _cpu_build(blob, window=1, monkeypatch=monkeypatch, slack=40)      # one or two blocks per window
    assert idx == bgzf.FaidxIndex(HAND_ROWS) and len(eng.calls) >= 4 and idx.gzi == bgzf.GziIndex.build(io.BytesIO(blob))


@pytest.mark.parametrize("lb,crlf,final_newline,trailing", [(1, False, True, 0), (60, True, True, 2), (63, False, False, 0), (64, True, False, 0),
                                                            (70, False, True, 3)])
def test_window_loop_equals_whole_file_equals_referee(monkeypatch, lb, crlf, final_newline, trailing):
    from zlib_ng_amd import bgzf
    rng = np.random.default_rng(lb)
    text = F.make_fasta(rng, lb, crlf, final_newline, trailing, total=30_000)
    verdict, rows = R.index(text)
    assert verdict == "ok" and {r[1] for r in rows} >= {0, 1, lb, lb + 1, 5 * lb} and {len(r[0]) for r in rows} >= {1, 200}
    blob = F.host_bgzf(text, 700, level=1)
    want = bgzf.FaidxIndex(rows)
    whole, eng = _cpu_build(blob)
    assert whole == want and len(eng.calls) == 1
    many, eng = _cpu_build(blob, window=1, monkeypatch=monkeypatch, slack=800)
    assert many == want and len(eng.calls) >= 8 and many.gzi == whole.gzi == bgzf.GziIndex.build(io.BytesIO(blob))


def _bad_cases():
    """(text, what it shows): every kind at the file's first lines, in the middle, and with the deciding line far behind"""
    seq = [b"ACGTACGTAC"] * 40
    body = b"\n".join([b">a"] + seq + [b">b x"] + seq + [b">c"] + seq) + b"\n"
    lines = body.split(b"\n")[:-1]

    def edit(no, new, insert=False):
        out = list(lines)
        if insert:
            out.insert(no, new)
        else:
            out[no] = new
        return b"\n".join(out) + b"\n"
    yield edit(0, b">"), "1 first"
    yield edit(41, b">\tx"), "1 middle"
    yield edit(1, b"ACGT CGTAC"), "2 first"
    yield edit(60, b"ACGTACGT\x7f"), "2 middle"
    yield edit(60, b"ACGTACGTACG"), "3 longer middle"
    yield edit(60, b"ACGTACG"), "3 shorter middle"
    yield edit(60, b"ACGTACGTAC\r"), "3 width"
    yield edit(81, b"ACGTACGTACGT"), "3 last longer"
    yield edit(60, b""), "4 middle"
    yield edit(42, b"", insert=True), "4 behind the header"
    yield b"\n" + edit(0, b"ACGT", insert=True), "5"
    yield b"\n".join([b">a", b"ACGT"] + [b""] * 300 + [b"ACGT", b">b", b"AC"]) + b"\n", "4 with the deciding line far behind"
    yield b"\n".join([b">a", b"ACGT", b"AC"] + [b""] * 300 + [b">b", b"AC"] + [b""] * 300 + [b"ACG"]) + b"\n", "4 behind a header, far behind"
    yield b"\n".join([b">a", b"ACGT", b"ACGTA"] + [b""] * 300 + [b">b", b"AC"]) + b"\n", "3 last longer, the header far behind"
    yield b"\n".join([b">a", b"ACGT", b"ACGTA"] + [b""] * 300) + b"\n", "3 last longer, the end far behind"
    yield edit(60, b"ACGT") + b">d\n>\n", "3 and then 1: two faults"


@pytest.mark.parametrize("text,what", list(_bad_cases()), ids=[w for _, w in _bad_cases()])
def test_bad_lines_report_the_referees_line_through_the_window_loop(monkeypatch, text, what):
    import tabix_ref
    verdict, line, kind = R.index(text)
    assert verdict == "bad" and kind == int(what[0])
    blob = F.host_bgzf(text, 100, level=0)
    v = tabix_ref.Voffsets(blob)(R.line_start(text, line))
    for window in (None, 1):
        with pytest.raises(ValueError, match=r"line %d at virtual offset %d " % (line, v)) as e:
            _cpu_build(blob, window=window, monkeypatch=monkeypatch, slack=200)
        assert (e.value.line, e.value.kind, e.value.voffset) == (line, kind, v)


def test_duplicate_names_are_refused(monkeypatch):
    text = b">a\nAC\n" + b">b\nACGT\n" * 200 + b">a d\nAC\n"
    assert R.index(text.replace(b">b", b">b%d", 0))[0] in ("dup",)
    for window in (None, 1):
        with pytest.raises(ValueError, match=r"b'b' occurs twice: header lines 2 and 4"):
            _cpu_build(F.host_bgzf(text, 100, level=0), window=window, monkeypatch=monkeypatch, slack=200)


def _block_loader(blob):
    import struct
    from zlib_ng_amd import _lib

    def load_block(c, cache):
        if c not in cache:
            raw = blob[c:c + 65536]
            code, tab, used, total = _lib.bgzf_scan(raw, 1)
            cache[c] = (raw[:used], 12 + struct.unpack_from("<H", raw, 10)[0], tab[0][3])
        return cache[c]
    return load_block


def test_fetch_seq_plan(monkeypatch):
    from zlib_ng_amd import bgzf, zlib_ng
    rng = np.random.default_rng(5)
    text = b">big\n" + b"\n".join(F.bases(rng, 61) for _ in range(3000)) + b"\n" + F.make_fasta(rng, 60, crlf=True, total=20_000)
    rows = R.index(text)[1]
    blob = F.host_bgzf(text, 5000, level=1)
    idx, _ = _cpu_build(blob)
    assert idx == bgzf.FaidxIndex(rows) and idx["big"][0] == 183_000
    eng = F.FakeEngine()

    def fetch(regions, rc=False, index=idx):
        return bgzf._fetch_seq_file(io.BytesIO(blob), len(blob), eng, index, regions, rc, _block_loader(blob))
    by = {r[0]: r[1:] for r in rows}
    regs = [(n, b, e) for n, b, e in F.regions_for(rng, rows, 120)] + [("big", 0, 183_000), ("big", 100, None), "big:2-3", "big:182,999", "big"]
    for rc in (False, True):
        eng.calls.clear()
        got = fetch(regs, rc)
        assert len(got) == len(regs) and len(got.offsets) == len(regs) + 1 and got.offsets.dtype == np.int64
        for k, r in enumerate(regs):
            name, beg, end = bgzf.parse_region(r if not (isinstance(r, tuple) and r[2] is None) else (r[0], r[1], 1 << 40))
            if isinstance(r, str) and "-" not in r:
                end = 1 << 40                                # an absent end is the sequence's end, not 2**29
            assert got[k] == R.subseq(text, by[name], beg, end, rc), (k, r, rc)
        assert list(got) == [got[k] for k in range(len(regs))] and got[-1] == got[len(regs) - 1] and got[1:3] == [got[1], got[2]]
        assert len(eng.calls) == 1 and eng.calls[0][1] <= len(text) // 5000 + 1      # one call; every block once
    # spans of at most 65 536 bases that begin at line starts; a region's spans lie reversed under reverse_complement
    spans = bgzf._seq_spans([(by[b"big"], 7, 183_000)], False)
    assert [s[3] for s in spans] == [65514 - 7, 65514, 183_000 - 2 * 65514] and [s[4] for s in spans] == [7, 0, 0] and [s[7] for s in spans] == [0, 65507, 131021]
    assert [s[7] for s in bgzf._seq_spans([(by[b"big"], 7, 183_000)], True)] == [183_000 - 65514, 183_000 - 2 * 65514, 0]
    assert [s[3] for s in bgzf._seq_spans([((200_000, 5, 100_000, 100_001), 10, 150_000)], False)] == [65536, 65536, 149_990 - 2 * 65536]
    # groups: a small text cap decodes every needed block once per group
    monkeypatch.setattr(bgzf, "_GREP_TEXT", 12_000)
    eng.calls.clear()
    got = fetch([("big", 0, 60_000), ("big", 30_000, 90_000)], True)
    assert got[0] == R.subseq(text, by[b"big"], 0, 60_000, True) and got[1] == R.subseq(text, by[b"big"], 30_000, 90_000, True)
    assert len(eng.calls) > 3 and max(c[1] for c in eng.calls) <= 4
    monkeypatch.undo()
    # errors: an unknown name before anything is decoded, a stale index, a region behind the data
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: (_ for _ in ()).throw(AssertionError("a context was asked for")))
    eng.calls.clear()
    with pytest.raises(KeyError):
        fetch([("big", 0, 5), ("nobody", 0, 5)])
    assert not eng.calls
    assert len(fetch([])) == 0 and fetch(("big", 5, 5))[0] == b"" and not eng.calls
    other = bgzf.FaidxIndex([(b"big", 183_000, 5, 60, 61)], idx.gzi)
    with pytest.raises(ValueError, match="faidx index does not match the file"):
        fetch(("big", 0, 200), index=other)
    with pytest.raises(ValueError, match="does not fit"):
        fetch(("far", 0, 10), index=bgzf.FaidxIndex([(b"far", 100, len(text) + 50, 60, 61)], idx.gzi))
    with pytest.raises(ValueError, match="faidx index does not match the file"):
        fetch(("big", 0, 200_000), index=bgzf.FaidxIndex(rows, bgzf.GziIndex([(c, u + 1) for c, u in idx.gzi.entries])))
    with pytest.raises(TypeError):
        fetch("big", index=object())

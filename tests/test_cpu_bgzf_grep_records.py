"""CPU: BGZF by record without a GPU -- the two C entry points are declared, exported and bound; their argument checks with a NULL
context; the Python argument checks, which ask for no context; and the window loop of bgzf.grep_records driven with a stand-in for the
engine call (Python on blocks the system zlib decodes) over files written on the host.  The referee is plain Python on the text: split
the lines, group them by k, `p in line` / startswith."""
import ctypes as C
import io
import os
import re
import types
import zlib

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from tabix_files import host_bgzf


def referee_records(data, delim, k, pats, match_line=None, invert=False, line_start=False, allow_short=True):
    """-> (records as bytes, numbers of the selected ones)"""
    parts = data.split(delim)
    lines = [p + delim for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])
    recs, sel = [], []
    for r in range(0, len(lines), k):
        group = lines[r:r + k]
        if len(group) < k and not allow_short:
            raise ValueError("short")
        look = group if match_line is None else group[match_line:match_line + 1]
        hit = any(ln.startswith(p) if line_start else p in ln for ln in look for p in pats)
        if hit != invert:
            sel.append(r // k)
        recs.append(b"".join(group))
    return recs, sel


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    for name in ("zngamd_bgzf_grep_records_dev", "zngamd_bgzf_grep_records"):
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        nargs = len(re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(","))
        assert len(getattr(L, name).argtypes) == nargs, name
        plain = len(re.search(r"\bint %s\s*\(([^;]*)\);" % name.replace("_records", ""), header).group(1).split(","))
        assert nargs == plain + 3, name                                              # record_lines, match_line, first_byte
    assert int(re.search(r"#define ZNGAMD_BGZF_GREP_MAX_RECORD_LINES\s+(\d+)u", header).group(1)) == _lib.BGZF_GREP_MAX_RECORD_LINES == 64
    assert C.sizeof(_lib.BgzfGrepRecordsTotals) == 64 and _lib.BgzfGrepRecordsTotals.covered.offset == 48
    assert re.search(r"\}\s*zngamd_bgzf_grep_records_totals;\s*/\* 64 B \*/", header)
    assert C.sizeof(_lib.BgzfGrepTotals) == 40                                       # the grep calls keep their layout
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES)                        # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_grep_records.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_grep_records.hip"))


def test_bad_arguments_are_refused_without_a_context():
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    tot = _lib.BgzfGrepRecordsTotals()
    blob = (C.c_uint8 * 6).from_buffer_copy(b"needle")
    tab = (C.c_uint32 * 2)(0, 6)

    def call(k, j, fb, dev, blob=blob, tab=tab, n=1, delim=10, totals=tot):
        t = C.byref(totals) if totals is not None else None
        if dev:
            return L.zngamd_bgzf_grep_records_dev(None, None, 0, None, 0, 0, 0, blob, 6, tab, n, delim, 0, k, j, fb, 0, None, 0, None, None, 0, None, 0, t)
        return L.zngamd_bgzf_grep_records(None, None, 0, None, 0, 0, 0, blob, 6, tab, n, delim, 0, k, j, fb, 0, None, None, 0, None, 0, _lib.ALLOC_FN(), None, t)

    for dev in (False, True):
        for k, j, fb in ((0, -1, -1), (65, -1, -1), (1 << 31, 0, -1), (4, -2, -1), (4, 4, -1), (1, 1, -1), (64, 64, -1), (4, 1, -2), (4, 1, 256),
                         (4, 1, 1 << 20), (4, 1, 64)):                                # (the last one is fine but for the NULL context)
            assert call(k, j, fb, dev) == E_ARG, (k, j, fb, dev)
        # everything zngamd_bgzf_grep refuses
        assert call(4, 1, 64, dev, tab=(C.c_uint32 * 2)(3, 6)) == E_ARG
        assert call(4, 1, 64, dev, tab=(C.c_uint32 * 2)(0, 0)) == E_ARG
        assert call(4, 1, 64, dev, n=0) == E_ARG and call(4, 1, 64, dev, n=65) == E_ARG
        assert call(4, 1, 64, dev, delim=256) == E_ARG and call(4, 1, 64, dev, delim=ord("d")) == E_ARG
        assert call(4, 1, 64, dev, blob=None) == E_ARG and call(4, 1, 64, dev, tab=None) == E_ARG and call(4, 1, 64, dev, totals=None) == E_ARG


def test_python_argument_errors_need_no_context(monkeypatch, tmp_path):
    from zlib_ng_amd import bgzf, zlib_ng

    def no_ctx():
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(zlib_ng, "_ctx", no_ctx)
    path = tmp_path / "f.bgzf"
    path.write_bytes(bgzf.EOF_BLOCK)
    for k in (0, 65, -4):
        with pytest.raises(ValueError, match="1 to 64 lines"):
            bgzf.grep_records(str(path), b"x", k)
    for kw in (dict(match_line=4), dict(match_line=-1), dict(first_byte=b""), dict(first_byte=b"@@"), dict(first_byte=256), dict(first_byte=-1),
               dict(max_record=0), dict(max_record=(1 << 31) + 1), dict(max_count=-1), dict(delimiter=b"ab")):
        with pytest.raises(ValueError):
            bgzf.grep_records(str(path), b"x", 4, **kw)
    with pytest.raises(ValueError, match="max_record"):
        bgzf.grep_records(str(path), b"x", 4, max_record=0)
    for bad in (b"", [], [b"x"] * 65, b"y" * 256, b"two\nlines"):
        with pytest.raises(ValueError):
            bgzf.grep_records(str(path), bad, 4)
    assert bgzf._grep_record_args(4, None, None) == (4, -1, -1) and bgzf._grep_record_args(8, 7, b"@") == (8, 7, 64)
    assert bgzf._grep_record_args(1, 0, 0) == (1, 0, 0) and bgzf._grep_record_args(64, 63, bytearray(b"\xff")) == (64, 63, 255)
    assert "grep_records" in bgzf.__all__ and hasattr(bgzf.BgzfReader, "grep_records")


class FakeEngine:
    """ctx.bgzf_grep_records computed on the host by the record model of include/zng_amd.h"""

    def __init__(self):
        self.calls = []

    def bgzf_grep_records(self, data, members, text_off, text_end, blob, table, delim, flags, k, match_line=-1, first_byte=-1, record_base=0, caps=None):
        from zlib_ng_amd import _lib
        data = bytes(data)
        buf = bytearray(int((members["out_off"] + members["out_len"]).max()) if len(members) else 0)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        self.calls.append((len(members), text_off, text_end, flags, record_base))
        text, d = bytes(buf[text_off:text_end]), bytes([delim])
        pats = [blob[o:o + n] for o, n in table.tolist()]
        parts = text.split(d)
        lines = [p + d for p in parts[:-1]]
        final = bool(flags & _lib.BGZF_GREP_FINAL)
        if parts[-1] and final:
            lines.append(parts[-1])
        nrec = (len(lines) + k - 1) // k if final else len(lines) // k
        starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64) + text_off
        tot = types.SimpleNamespace(seen=nrec, selected=0, matched=0, bytes=0, covered=1, bad=0, bad_record=0, bad_src=0,
                                    tail_off=text_end if final else int(starts[k * nrec]), short_lines=len(lines) % k if final else 0)
        rows, packed = [], []
        for r in range(nrec):
            group = lines[k * r:k * r + k]
            look = group if match_line < 0 else group[match_line:match_line + 1]
            hit = any(ln.startswith(p) if flags & _lib.BGZF_GREP_LINE_START else p in ln for ln in look for p in pats)
            if first_byte >= 0 and group[0][0] != first_byte and not tot.bad:
                tot.bad, tot.bad_record, tot.bad_src = 1, record_base + r, int(starts[k * r])
            if hit != bool(flags & _lib.BGZF_GREP_INVERT):
                rows.append((int(starts[k * r]), record_base + r, sum(len(x) for x in group), 0))
                packed.append(b"".join(group))
        tot.selected = tot.matched = len(rows)
        tot.bytes = sum(len(x) for x in packed)
        if flags & _lib.BGZF_GREP_COUNT_ONLY or tot.bad:
            rows, packed = [], []
        return 0, np.zeros(len(members), np.int32), tot, np.array(rows, _lib.GREP_ROW_DTYPE), b"".join(packed)


def reads(n, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(20, 90))
        seq = bytes(rng.choice(list(b"ACGT"), ln).tolist())
        if i % 9 == 4:
            seq = seq[:7] + b"GGNEEDLEGG" + seq[17:]
        out.append(b"@read%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq)))
    return out


def run(blob, eng, pats, k, window=None, monkeypatch=None, **kw):
    from zlib_ng_amd import bgzf
    args = dict(match_line=None, first_byte=None, delimiter=b"\n", invert=False, line_start=False, count=False, max_count=None, start=None,
                stop=None, first_record=0, max_record=64 << 20, allow_short=False)
    args.update(kw)
    if window is not None:
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        monkeypatch.setattr(bgzf, "MAX_BLOCK", 600)                                  # (what is read beyond a window: a block of these files)
    return bgzf._grep_file(io.BytesIO(blob), eng, pats, args["delimiter"], args["invert"], args["line_start"], args["count"], args["max_count"],
                           args["start"], args["stop"], args["first_record"], args["max_record"],
                           (k, args["match_line"], args["first_byte"], args["allow_short"]))


def voffset_at(blob, pos, block_size):
    """the normalised virtual offset of byte `pos` of the text (blocks of block_size input bytes, written by host_bgzf)"""
    from zlib_ng_amd import _lib
    code, tab, used, total = _lib.bgzf_scan(blob)
    c, u, cs, isz = tab[pos // block_size]
    assert u == pos // block_size * block_size
    return c << 16 | pos % block_size


@pytest.mark.parametrize("window", [None, 600, 1])
def test_window_loop_on_a_fake_engine(monkeypatch, window):
    recs = reads(400)
    data = b"".join(recs)
    BS = 500
    blob = host_bgzf(data, BS, level=1)
    eng = FakeEngine()
    want_recs, want = referee_records(data, b"\n", 4, [b"NEEDLE"], match_line=1)
    assert want_recs == recs and len(want) == 44
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    res = run(blob, eng, b"NEEDLE", 4, window, monkeypatch, match_line=1, first_byte=b"@")
    assert res.numbers.tolist() == want and list(res) == [recs[i] for i in want] and res.searched == len(recs)
    assert res.voffsets.tolist() == [voffset_at(blob, int(starts[i]), BS) for i in want]
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum([len(recs[i]) for i in want])]).tolist()
    n_all = len(eng.calls)
    if window is None:
        assert n_all == 1
    else:
        assert n_all > 10
        # a record cut by a window is taken up at its first line: every window starts at a record start, its number the records in front
        assert [b for *_, b in eng.calls] == sorted(b for *_, b in eng.calls) and eng.calls[-1][4] < len(recs)
        assert any(off > 0 for _, off, _, _, _ in eng.calls[1:])
    # a match on another line does not count with match_line; without it, it does
    assert run(blob, eng, b"@read7", 4, match_line=1, count=True) == 0
    assert run(blob, eng, b"@read7", 4).numbers.tolist() == referee_records(data, b"\n", 4, [b"@read7"])[1] == [7] + list(range(70, 80))
    inv = run(blob, eng, b"NEEDLE", 4, invert=True, first_record=1000)
    assert inv.numbers.tolist() == [1000 + i for i in range(len(recs)) if i not in want]
    # count and max_count count records; max_count stops reading
    assert run(blob, eng, b"NEEDLE", 4, count=True) == len(want) and run(blob, eng, b"NEEDLE", 4, count=True, max_count=5) == 5
    eng.calls.clear()
    part = run(blob, eng, b"NEEDLE", 4, max_count=3)
    assert part.numbers.tolist() == want[:3] and list(part) == [recs[i] for i in want[:3]]
    assert len(eng.calls) == 1 if window is None else len(eng.calls) < n_all // 4
    # start / stop at record starts, numbered by first_record
    a, b = 100, 301
    mid = run(blob, eng, b"NEEDLE", 4, start=voffset_at(blob, int(starts[a]), BS), stop=voffset_at(blob, int(starts[b]), BS), first_record=a)
    assert mid.numbers.tolist() == [i for i in want if a <= i < b] and mid.searched == b - a
    # first_byte: a line removed shifts every record behind it
    lines = data.split(b"\n")
    del lines[4 * 123 + 2]
    broken = b"\n".join(lines)
    bblob = host_bgzf(broken, BS, level=1)
    at = sum(len(x) for x in recs[:124]) - 2 + len(b"@read124\n")                    # where record 124 now starts: behind the header of read 124
    with pytest.raises(ValueError, match=r"record 124 at virtual offset %d does not start with b'@'" % voffset_at(bblob, at, BS)):
        run(bblob, eng, b"NEEDLE", 4, first_byte=b"@")
    # a short last record
    with pytest.raises(ValueError, match=r"record 399, the last one, has 3 of 4 lines"):
        run(bblob, eng, b"NEEDLE", 4)
    short = run(bblob, eng, b"\x02absent", 4, allow_short=True, invert=True)
    assert short.searched == 400 and short.numbers.tolist() == list(range(400))
    assert short[399] == b"".join(x + b"\n" for x in broken.split(b"\n")[4 * 399:-1]) and short[399].count(b"\n") == 3
    assert list(short) == referee_records(broken, b"\n", 4, [b"\x02absent"], invert=True)[0]


def test_a_window_without_a_record_end_doubles_and_max_record_bounds_it(monkeypatch):
    from zlib_ng_amd import bgzf
    big = b"@big\n" + b"ACGT" * 5000 + b"NEEDLE\n+\n" + b"I" * 20006 + b"\n"
    recs = reads(30) + [big] + reads(30, 2)
    data = b"".join(recs)
    blob = host_bgzf(data, 500, level=1)
    eng = FakeEngine()
    res = run(blob, eng, b"NEEDLE", 4, 1200, monkeypatch, match_line=1)
    want = referee_records(data, b"\n", 4, [b"NEEDLE"], match_line=1)[1]
    assert 30 in want and res.numbers.tolist() == want and res[want.index(30)] == big
    # the same text_off was searched again with more text behind it, several times, until the record ended
    at_big = [(off, end) for nm, off, end, flags, base in eng.calls if base == 30]
    assert len(at_big) >= 3 and len({off for off, _ in at_big}) == 1 and [e for _, e in at_big] == sorted({e for _, e in at_big})
    v = int(res.voffsets[want.index(30)])
    with pytest.raises(ValueError, match=r"the record at virtual offset %d has not ended after 30000 bytes \(max_record\)" % v):
        run(blob, eng, b"NEEDLE", 4, 1200, monkeypatch, match_line=1, max_record=30000)
    assert run(blob, eng, b"NEEDLE", 4, 1200, monkeypatch, match_line=1, max_record=len(big), count=True) == len(want)

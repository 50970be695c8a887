"""BGZF by content (bgzf.grep, BgzfReader.grep; csrc/za_grep.hip: za_k_grep_mark / _scan / _emit).  The referee is Python on the bytes
the system gzip decodes: referee_lines of tests/test_gpu_bgzf_lines.py, then `any(p in line for p in patterns)` or line.startswith --
never the code under test."""
import gzip
import os
import random

import numpy as np
import pytest

from test_gpu_bgzf_lines import BLOCK, awkward, inputs, member_table, referee_lines      # noqa: F401  (inputs, awkward: fixtures)

pytestmark = pytest.mark.gpu


def referee(data, delim, pats, invert=False, line_start=False):
    """-> (the lines, the numbers of the selected ones)"""
    lines = referee_lines(data, delim)
    if line_start:
        hit = [any(ln.startswith(p) for p in pats) for ln in lines]
    else:
        hit = [any(p in ln for p in pats) for ln in lines]
    return lines, [i for i, h in enumerate(hit) if h != invert]


def pattern_sets(rng, data, delim):
    """pattern lists for one input: absent, one byte, a whole line, a piece of a line, a prefix beside its extension, 255 bytes, 64 at
    once -- all cut from the data itself, so that they occur, and across whatever block, tile and window edges the data has"""
    bodies = [ln[:-1] if ln.endswith(delim) else ln for ln in referee_lines(data, delim)]
    bodies = [b for b in bodies if b]
    absent = bytes(b for b in b"\x02nowhere in the data\x03" if b != delim[0])
    sets = [[absent]]
    if not bodies:
        return sets + [[bytes([(delim[0] + 1) & 0xFF])]]
    b = rng.choice(bodies)
    k = rng.randrange(len(b))
    sets += [[b[:1]], [b[:255]], [b[k:k + rng.randrange(1, 9)]], [b[:2], b[:5], absent], [bodies[-1][-3:]]]
    longs = [x for x in bodies if len(x) >= 255]
    if longs:
        x = rng.choice(longs)
        o = rng.randrange(len(x) - 254)
        sets.append([x[o:o + 255]])
    many = []
    while len(many) < 64:
        x = rng.choice(bodies)
        o = rng.randrange(len(x))
        many.append(x[o:o + rng.randrange(1, 13)] if len(many) % 3 else absent[:len(many) % 7 + 2] + bytes([65 + len(many) % 26]))
    sets.append(many)
    return sets


def block_map(blob):
    from zlib_ng_amd import _lib
    code, tab, used, total = _lib.bgzf_scan(blob)
    assert code == 0 and used == len(blob)
    return tab, {c: (u, isz) for c, u, cs, isz in tab}


def check_result(res, lines, sel, by_c, reader=None, rng=None, what=None):
    want = [lines[i] for i in sel]
    assert len(res) == len(sel), what
    assert res.numbers.dtype == np.int64 and res.voffsets.dtype == np.uint64 and res.offsets.dtype == np.int64
    assert res.numbers.tolist() == sel, what
    assert res.offsets.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want], dtype=np.int64)]).tolist(), what
    assert bytes(res.data) == b"".join(want), what
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines], dtype=np.int64)])
    if len(sel):                                                 # normalised virtual offsets of the lines' first bytes
        c, u = (res.voffsets >> np.uint64(16)).astype(np.int64), (res.voffsets & np.uint64(0xFFFF)).astype(np.int64)
        cs = np.array(sorted(by_c), np.int64)
        k = np.minimum(np.searchsorted(cs, c), len(cs) - 1)
        assert (cs[k] == c).all(), what
        u0, isz = np.array([by_c[x][0] for x in cs.tolist()], np.int64)[k], np.array([by_c[x][1] for x in cs.tolist()], np.int64)[k]
        assert (u < isz).all() and (u0 + u == starts[np.array(sel)]).all(), (what, "voffsets")
    if reader is not None and len(sel):
        for k in sorted(set(rng.sample(range(len(sel)), min(len(sel), 12))) | {0, len(sel) - 1}):
            reader.seek(int(res.voffsets[k]))
            assert reader.read(len(want[k])) == want[k] == res[k], (what, k)


MODES = [dict(), dict(invert=True), dict(line_start=True), dict(line_start=True, invert=True)]


def test_grep_against_the_referee(ctx, inputs, tmp_path):
    from zlib_ng_amd import bgzf
    rng = random.Random(5)
    for name, (blob, delims) in inputs.items():
        path = tmp_path / "t.bgzf"
        path.write_bytes(blob)
        data = gzip.decompress(blob)
        tab, by_c = block_map(blob)
        for delim in delims:
            idx = bgzf.LineIndex.build(str(path), delim)
            with bgzf.open(str(path)) as r:
                for pats in pattern_sets(rng, data, delim):
                    for mode in MODES:
                        what = (name, delim, pats[:3], mode)
                        lines, sel = referee(data, delim, pats, **mode)
                        r.seek(0)
                        head = r.read(7)
                        res = r.grep(pats if len(pats) > 1 else pats[0], delimiter=delim, **mode)
                        assert head + r.read(9) == data[:16], what                       # the reader's position stayed where it was
                        assert res.searched == len(lines), what
                        check_result(res, lines, sel, by_c, r, rng, what)
                        assert list(res) == [lines[i] for i in sel] and res[:2] == [lines[i] for i in sel[:2]]
                        assert r.grep(pats, delimiter=delim, count=True, **mode) == len(sel), what
                        for n in sorted({0, 1, len(sel) // 2, len(sel) + 3}):
                            part = r.grep(pats, delimiter=delim, max_count=n, **mode)
                            check_result(part, lines, sel[:n], by_c, what=what + (n,))
                            assert r.grep(pats, delimiter=delim, max_count=n, count=True, **mode) == min(n, len(sel))
                    # the parts LineIndex.shards gives, each searched on its own
                    lines, sel = referee(data, delim, pats)
                    for n in (1, 3, 7):
                        cuts = idx.shards(r, n)
                        firsts = [min(i * idx.lines // n, idx.lines) for i in range(n + 1)]
                        parts = [r.grep(pats, delimiter=delim, start=cuts[i], stop=cuts[i + 1], first_line=firsts[i]) for i in range(n)]
                        assert [p.searched for p in parts] == [b - a for a, b in zip(firsts, firsts[1:])], (name, delim, n)
                        assert sum((p.numbers.tolist() for p in parts), []) == sel, (name, delim, n)
                        assert b"".join(bytes(p.data) for p in parts) == b"".join(lines[i] for i in sel)
                        assert sum((p.voffsets.tolist() for p in parts), []) == r.grep(pats, delimiter=delim).voffsets.tolist()
                        assert sum(r.grep(pats, delimiter=delim, start=cuts[i], stop=cuts[i + 1], count=True) for i in range(n)) == len(sel)
            assert bgzf.grep(str(path), b"\x02", delimiter=delim).searched == len(referee_lines(data, delim))


def test_path_file_object_and_arguments(ctx, inputs, tmp_path):
    from zlib_ng_amd import bgzf
    blob = inputs["fastq"][0]
    path = tmp_path / "t.bgzf"
    path.write_bytes(blob)
    data = gzip.decompress(blob)
    lines, sel = referee(data, b"\n", [b"GATC"])
    a = bgzf.grep(str(path), b"GATC")
    with open(path, "rb") as f:
        b = bgzf.grep(f, [bytearray(b"GATC")])
    assert a.numbers.tolist() == b.numbers.tolist() == sel and bytes(a.data) == bytes(b.data)
    assert bgzf.grep(str(path), b"GATC", first_line=1000).numbers.tolist() == [1000 + i for i in sel]
    for bad in (b"", [], [b"ok", b""], [b"x"] * 65, b"y" * 256, b"two\nlines"):
        with pytest.raises(ValueError):
            bgzf.grep(str(path), bad)
    with pytest.raises(ValueError):
        bgzf.grep(str(path), b"x", delimiter=b"ab")
    with pytest.raises(ValueError):
        bgzf.grep(str(path), b"a;b", delimiter=b";")
    tab, by_c = block_map(blob)
    with pytest.raises(ValueError, match="bytes into a block"):
        bgzf.grep(str(path), b"x", start=bgzf.make_virtual_offset(tab[1][0], tab[1][3] + 1))


def straddling(rng, nlines=9, width=200000):
    """lines of `width` bytes that do not compress, so that a line spans several blocks, tiles and (with a small window) windows;
    needles planted across every 16 KiB tile edge of some lines and across block edges"""
    needle = b"<needle:straddles>"
    out = []
    for i in range(nlines):
        body = bytearray(os.urandom(width - 1).replace(b"\n", b"\x0b"))
        if i % 3 == 1:
            at = (sum(len(x) for x in out) // 16384 + 2 + i) * 16384 - sum(len(x) for x in out) - len(needle) // 2      # across a tile edge of the text
            body[at:at + len(needle)] = needle
        if i % 3 == 2:
            at = BLOCK * ((sum(len(x) for x in out) + BLOCK - 1) // BLOCK + 1) - sum(len(x) for x in out) - 5            # across a block edge
            body[at:at + len(needle)] = needle
        out.append(bytes(body) + b"\n")
    return b"".join(out), needle


def test_windows_tiles_and_long_lines(ctx, inputs, tmp_path, monkeypatch):
    """a small read window: lines and patterns straddle windows, the open line's blocks are decoded again, a line longer than the
    window makes it grow, one longer than max_line is refused"""
    from zlib_ng_amd import bgzf
    rng = random.Random(9)
    data, needle = straddling(rng)
    blob = bgzf.compress(data)
    assert len(blob) > 9 * 190000
    path = tmp_path / "long.bgzf"
    path.write_bytes(blob)
    tab, by_c = block_map(blob)
    whole = bgzf.grep(str(path), needle)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 100000)
    for pats, mode in (([needle], {}), ([needle], dict(invert=True)), ([needle[:3], b"\x00\x01\x02\x03\x04"], {}), ([data[:200]], dict(line_start=True)),
                       ([data[400000:400255]], {}), ([data[-256:-1]], {})):
        lines, sel = referee(data, b"\n", pats, **mode)
        ctx.bgzf_stats()
        res = bgzf.grep(str(path), pats, **mode)
        launches = ctx.bgzf_stats()[0]
        assert launches > 9                                        # the windows grew: every line is longer than the first window
        assert res.searched == len(lines)
        check_result(res, lines, sel, by_c, what=(pats[0][:8], mode))
    assert bgzf.grep(str(path), needle).voffsets.tolist() == whole.voffsets.tolist() and len(whole) == 6
    with pytest.raises(ValueError, match="max_line"):
        bgzf.grep(str(path), needle, max_line=100000)
    assert bgzf.grep(str(path), needle, max_line=200000, count=True) == 6
    # no delimiter at all: one line, and a bound on what it may claim
    for delim in (b"\x00", b"\n"):
        nodelim = data.replace(delim, b"\x0c")
        p2 = tmp_path / "nodelim.bgzf"
        p2.write_bytes(bgzf.compress(nodelim))
        res = bgzf.grep(str(p2), needle, delimiter=delim)
        assert res.searched == 1 and res.numbers.tolist() == [0] and bytes(res.data) == nodelim and res.voffsets.tolist() == [0]
        assert bgzf.grep(str(p2), needle, delimiter=delim, invert=True, count=True) == 0
        with pytest.raises(ValueError, match="virtual offset 0 has not ended"):
            bgzf.grep(str(p2), needle, delimiter=delim, max_line=1 << 20)
    # short lines: windows straddle lines and patterns; economy -- one launch per window, the open line's block decoded twice
    for name in ("fastq", "bgzip", "text", "small blocks", "edges"):
        blob = inputs[name][0]
        data = gzip.decompress(blob)
        path = tmp_path / "short.bgzf"
        path.write_bytes(blob)
        tab, by_c = block_map(blob)
        monkeypatch.setattr(bgzf, "_READ_WINDOW", 100000 if len(blob) > 300000 else 70000)
        for pats in pattern_sets(rng, data, b"\n"):
            for mode in MODES[:3]:
                lines, sel = referee(data, b"\n", pats, **mode)
                ctx.bgzf_stats()
                res = bgzf.grep(str(path), pats, **mode)
                launches, decoded, _ = ctx.bgzf_stats()
                check_result(res, lines, sel, by_c, what=(name, pats[:2], mode))
                assert res.searched == len(lines)
                assert launches <= len(blob) // bgzf._READ_WINDOW + 2 and decoded <= len(tab) + 2 * launches, (name, launches, decoded, len(tab))
                if name in ("fastq", "bgzip"):
                    assert launches >= 3, (name, launches)
                n = len(sel) // 3
                ctx.bgzf_stats()
                part = bgzf.grep(str(path), pats, max_count=n, **mode)
                assert part.numbers.tolist() == sel[:n] and ctx.bgzf_stats()[0] <= launches


def test_edges_by_hand(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    cases = [
        (b"aaaa\naa\na\n", b"\n", [b"aa"], 4),                          # a pattern that overlaps itself
        (b"chr7\t1\nchr77\t2\nxchr7\t3\nchr7", b"\n", [b"chr7\t"], 4),  # the last line has no delimiter and is too short for the pattern
        (b"one\ntwo\nthree", b"\n", [b"ree"], 5),                      # the pattern in the last bytes of data without a final delimiter
        (b"one\ntwo\nthree", b"\n", [b"three"], 3),                    # ... equal to the whole last line
        (b"\n\n\nx\n\n", b"\n", [b"x"], 1),
        (b"\x00\x01\x7f\x80\x81\xff" * 50, b"\x7f", [b"\x80\x81\xff\x00\x01"], 3),
        (b"\x00\x01\x7f\x80\x81\xff" * 50, b"\x00", [b"\xff", b"\x01\x7f"], 4),
        (b"\x00\x01\x7f\x80\x81\xff" * 50, b"\xff", [b"\x00", b"\x81"], 37),
        (b"a;b;;ab;ba;", b";", [b"ab", b"a"], 4),
        (b"x" * 40000 + b"needle" + b"y" * 40000, b"\n", [b"needle"], 65280),
    ]
    for data, delim, pats, bs in cases:
        path = tmp_path / "c.bgzf"
        blob = bgzf.compress(data, block_size=bs)
        path.write_bytes(blob)
        assert gzip.decompress(blob) == data
        tab, by_c = block_map(blob)
        with bgzf.open(str(path)) as r:
            for mode in MODES:
                lines, sel = referee(data, delim, pats, **mode)
                res = r.grep(pats, delimiter=delim, **mode)
                assert res.searched == len(lines)
                check_result(res, lines, sel, by_c, r, random.Random(1), (data[:12], pats, mode))
    path = tmp_path / "eof.bgzf"
    path.write_bytes(bgzf.EOF_BLOCK)
    res = bgzf.grep(str(path), b"x")
    assert len(res) == 0 and res.searched == 0 and res.offsets.tolist() == [0] and bytes(res.data) == b"" and list(res) == []
    assert bgzf.grep(str(path), b"x", invert=True, count=True) == 0
    path.write_bytes(b"")
    assert bgzf.grep(str(path), b"x", count=True) == 0


def test_damage(ctx, tmp_path, fastq):
    from zlib_ng_amd import _lib, bgzf
    data = fastq[:10 * BLOCK]
    blob = bytearray(bgzf.compress(data))
    _, tab, _, _ = _lib.bgzf_scan(bytes(blob))
    c, u, cs, isz = tab[4]
    blob[c + 18 + cs // 2] ^= 0x5A                                          # a payload byte of block 4
    bad = str(tmp_path / "bad.bgzf")
    open(bad, "wb").write(blob)
    for kw in (dict(), dict(count=True), dict(max_count=10 ** 9), dict(invert=True)):
        with pytest.raises(bgzf.BadGzipFile, match=f"offset {c}:"):
            bgzf.grep(bad, b"@", **kw)
    cut = str(tmp_path / "cut.bgzf")
    open(cut, "wb").write(bgzf.compress(data)[:tab[6][0] + 100])            # the file ends inside block 6
    with bgzf.open(cut) as r:
        with pytest.raises(EOFError) as reader_error:
            r.read()
    with pytest.raises(type(reader_error.value), match=f"offset {tab[6][0]}: the file ends inside the block"):
        bgzf.grep(cut, b"@")
    notbgzf = str(tmp_path / "plain.gz")
    open(notbgzf, "wb").write(gzip.compress(data))
    with pytest.raises(bgzf.BadGzipFile, match="Not a BGZF file"):
        bgzf.grep(notbgzf, b"@")


# ---- the C entry points directly
def c_referee(data, text_off, text_end, delim, pats, flags, line_base):
    """what zngamd_bgzf_grep reports for data[text_off:text_end): (seen, rows [(src_off, number, len)], tail_off)"""
    from zlib_ng_amd import _lib
    text = data[text_off:text_end]
    d = bytes([delim])
    lines = referee_lines(text, d)
    tail = text_end
    if lines and not lines[-1].endswith(d) and not flags & _lib.BGZF_GREP_FINAL:
        tail = text_end - len(lines.pop())
    rows, at = [], text_off
    for i, ln in enumerate(lines):
        hit = any(ln.startswith(p) for p in pats) if flags & _lib.BGZF_GREP_LINE_START else any(p in ln for p in pats)
        if hit != bool(flags & _lib.BGZF_GREP_INVERT):
            rows.append((at, line_base + i, len(ln)))
        at += len(ln)
    return len(lines), rows, tail


def test_entry_point(ctx, awkward):
    from zlib_ng_amd import _lib
    data, blob, tab = awkward
    members = member_table(tab)
    arr = np.frombuffer(data, np.uint8)
    rng = random.Random(4)
    F = _lib.BGZF_GREP_FINAL
    for delim in (0, 1, 10, 0x7f, 0x80, 0xff):
        cuts = (np.nonzero(arr == delim)[0] + 1).tolist()
        alphabet = [b for b in b"\x00\x01\x02\x7f\x80\x81\xff\n\x0b" if b != delim]
        for trial in range(6):
            pats = [bytes(rng.choice(alphabet) for _ in range(rng.choice([1, 1, 2, 3, 5]))) for _ in range(rng.choice([1, 2, 64]))]
            table = _lib.grep_pattern_table(pats)
            text_off = rng.choice([0] + cuts[:50])
            text_end = rng.choice([len(data), len(data), rng.choice(cuts), rng.randrange(text_off, len(data) + 1)])
            text_end = max(text_end, text_off)
            for flags in (0, F, _lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_LINE_START | F, _lib.BGZF_GREP_LINE_START | _lib.BGZF_GREP_INVERT):
                seen, rows, tail = c_referee(data, text_off, text_end, delim, pats, flags, 1000)
                ctx.bgzf_stats()
                code, status, tot, got, packed = ctx.bgzf_grep(blob, members, text_off, text_end, *table, delim, flags, 1000)
                assert ctx.bgzf_stats()[:2] == (1, len(tab))
                what = (delim, trial, flags, text_off, text_end)
                assert code == 0 and not status.any() and tot.covered == 1, what
                assert (tot.seen, tot.matched, tot.tail_off) == (seen, len(rows), tail), what
                assert [(int(r["src_off"]), int(r["number"]), int(r["len"])) for r in got] == rows, what
                assert packed == b"".join(data[s:s + n] for s, _, n in rows) and tot.bytes == len(packed), what
                code, status, tot2, got2, packed2 = ctx.bgzf_grep(blob, members, text_off, text_end, *table, delim, flags | _lib.BGZF_GREP_COUNT_ONLY, 1000)
                assert (tot2.seen, tot2.matched, tot2.bytes, tot2.tail_off, len(got2), packed2) == (seen, len(rows), tot.bytes, tail, 0, b""), what
    # the sizing protocol
    pats = [b"\x01"]
    table = _lib.grep_pattern_table(pats)
    seen, rows, tail = c_referee(data, 0, len(data), 10, pats, F, 0)
    nbytes = sum(n for _, _, n in rows)
    assert len(rows) > 100
    for caps in ((len(rows) - 1, nbytes), (len(rows), nbytes - 1), (0, 0)):
        code, status, tot, got, packed = ctx.bgzf_grep(blob, members, 0, len(data), *table, 10, F, 0, caps)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.matched, tot.bytes, tot.covered) == (seen, len(rows), nbytes, 1) and len(got) == 0 and packed == b""
    code, status, tot, got, packed = ctx.bgzf_grep(blob, members, 0, len(data), *table, 10, F, 0, (len(rows), nbytes))
    assert code == 0 and got["src_off"].tolist() == [s for s, _, _ in rows] and len(packed) == nbytes
    code, status, tot, got, packed = ctx.bgzf_grep(blob, members, 0, len(data), *table, 10, F | _lib.BGZF_GREP_COUNT_ONLY, 0, (0, 0))
    assert code == 0 and tot.matched == len(rows)
    # arguments
    for bad_pats, delim in (([b""], 10), ([b"a\nb"], 10), ([b"x"] * 65, 10), ([b"y" * 256], 10), ([b"x"], 256), ([b"x"], -1)):
        blob_, tab_ = _lib.grep_pattern_table(bad_pats)
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_grep(blob, members, 0, len(data), blob_ or b"\0", tab_, delim, 0)
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_grep(blob, members, 0, len(data), b"abc", np.array([[2, 2]], np.uint32), 10, 0)          # a row outside the blob
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_grep(blob, members, 0, len(data) + 1, *table, 10, 0)                                       # the text outside the scratch
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_grep(blob, members, 5, 4, *table, 10, 0)
    assert ctx.bgzf_grep(blob, members[:0], 0, 0, *table, 10, F)[2].covered == 1


def test_tables_are_untrusted(ctx, awkward):
    """only what the contract defines: a table with a gap, rows out of order, a block that did not decode -- covered = 0, no rows"""
    from zlib_ng_amd import _lib
    data, blob, tab = awkward
    members = member_table(tab)
    table = _lib.grep_pattern_table([b"\x01"])
    F = _lib.BGZF_GREP_FINAL

    def run(m, lo=0, hi=len(data)):
        code, status, tot, got, packed = ctx.bgzf_grep(blob, m, lo, hi, *table, 10, F, 0)
        assert code == 0
        return status, tot, got, packed

    gap = np.delete(members, 7)
    status, tot, got, packed = run(gap)
    assert not status.any() and (tot.covered, tot.seen, tot.matched, tot.bytes) == (0, 0, 0, 0) and len(got) == 0 and packed == b""
    # the same table covers a text in front of the gap and one behind it
    status, tot, got, packed = run(gap, 0, tab[7][1])
    seen, rows, tail = c_referee(data, 0, tab[7][1], 10, [b"\x01"], F, 0)
    assert tot.covered == 1 and (tot.seen, tot.matched) == (seen, len(rows)) and got["src_off"].tolist() == [s for s, _, _ in rows]
    status, tot, got, packed = run(gap, tab[8][1], len(data))
    assert tot.covered == 1 and tot.seen == c_referee(data, tab[8][1], len(data), 10, [b"\x01"], F, 0)[0]
    swapped = members.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert run(swapped)[1].covered == 0
    hostile = members.copy()
    hostile["in_off"][5] = len(blob) + 1000                                   # block 5 does not decode
    status, tot, got, packed = run(hostile)
    assert [bool(s) for s in status.tolist()] == [i == 5 for i in range(len(tab))]
    assert (tot.covered, tot.matched) == (0, 0) and len(got) == 0 and packed == b""
    assert run(hostile, 0, tab[5][1])[1].covered == 1 and run(hostile, tab[6][1], len(data))[1].covered == 1
    assert run(hostile, 0, tab[5][1] + 1)[1].covered == 0
    for field, value in (("in_off", 1 << 63), ("in_len", (1 << 64) - 1), ("out_off", 1 << 50)):
        wild = members.copy()
        wild[field][3] = value
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_grep(blob, wild, 0, len(data), *table, 10, F, 0)


def test_device_form(ctx, awkward):
    """zngamd_bgzf_grep_dev on device buffers, with a scratch that is shorter than the member table says"""
    from zlib_ng_amd import _lib, devmem
    data, blob, tab = awkward
    members = member_table(tab)
    n = len(tab)
    cap = tab[30][1] + 5                                             # block 30 and everything behind it lie outside the scratch
    pats = [b"\x80", b"\x01\x01"]
    table = _lib.grep_pattern_table(pats)
    arr = np.frombuffer(data, np.uint8)
    text_off = int(np.nonzero(arr == 10)[0][3]) + 1
    text_end = tab[30][1]
    seen, rows, tail = c_referee(data, text_off, text_end, 10, pats, 0, 7)
    nbytes = sum(ln for _, _, ln in rows)
    assert len(rows) > 20 and tail < text_end
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, cap), devmem.empty(ctx, 4 * n)
    d_rows, d_out = devmem.empty(ctx, 24 * len(rows)).zero_(), devmem.empty(ctx, nbytes).zero_()
    args = (d_in.ptr, len(blob), d_m.ptr, n, text_off, text_end, *table, 10, 0, 7, d_scratch.ptr, cap, d_st.ptr)
    ctx.bgzf_stats()
    code, tot = ctx.bgzf_grep_dev(*args, d_rows.ptr, len(rows) - 1, d_out.ptr, nbytes)
    assert code == _lib.BUF_ERROR and (tot.seen, tot.matched, tot.bytes, tot.tail_off, tot.covered) == (seen, len(rows), nbytes, tail, 1)
    assert d_rows.cpu().tobytes() == bytes(24 * len(rows)) and d_out.cpu().tobytes() == bytes(nbytes)
    code, tot = ctx.bgzf_grep_dev(*args, d_rows.ptr, len(rows), d_out.ptr, nbytes)
    assert code == 0 and (tot.seen, tot.matched, tot.bytes, tot.tail_off, tot.covered) == (seen, len(rows), nbytes, tail, 1)
    assert ctx.bgzf_stats()[:2] == (2, 2 * n)
    got = d_rows.cpu(_lib.GREP_ROW_DTYPE)
    assert [(int(r["src_off"]), int(r["number"]), int(r["len"])) for r in got] == rows
    assert d_out.cpu().tobytes() == b"".join(data[s:s + ln] for s, _, ln in rows)
    assert [bool(s) for s in d_st.cpu(np.int32).tolist()] == [i >= 30 for i in range(n)]
    code, tot = ctx.bgzf_grep_dev(*args[:5], tab[30][1] + 5, *args[6:], d_rows.ptr, len(rows), d_out.ptr, nbytes)      # block 30 touches the text and failed
    assert code == 0 and (tot.covered, tot.matched) == (0, 0)
    code, tot = ctx.bgzf_grep_dev(*args[:9], _lib.BGZF_GREP_COUNT_ONLY, *args[10:], 0, 0, 0, 0)
    assert code == 0 and (tot.seen, tot.matched, tot.covered) == (seen, len(rows), 1)
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_grep_dev(*args[:5], cap + 1, *args[6:], d_rows.ptr, len(rows), d_out.ptr, nbytes)

"""BGZF by record (bgzf.grep_records, BgzfReader.grep_records; csrc/za_grep_records.hip: za_k_grep_rec_lines / _eval / _close / _emit
behind the tiles of za_grep.hip).  The referee is Python on the bytes the system gzip decodes: split the lines, group them by k, test
`p in line` or line.startswith (referee_records of tests/test_cpu_bgzf_grep_records.py) -- never the code under test.  Everything is
compared exactly: numbers, voffsets, offsets and data byte for byte."""
import gzip
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN
from test_cpu_bgzf_grep_records import referee_records
from test_gpu_bgzf_grep import MODES, block_map, check_result, pattern_sets
from test_gpu_bgzf_lines import awkward, inputs, member_table      # noqa: F401  (inputs, awkward: fixtures)

pytestmark = pytest.mark.gpu

T = 16384                                                          # a tile of za_grep.hip
BGZIP = os.path.join(GOLDEN, "test.fastq.bgzip.gz")
INPUTS = ["eof only", "one delimiter", "one byte", "fastq", "bgzip", "long line", "only delimiters", "edges", "small blocks", "text", "two streams",
          "crlf", "urandom"]


def same(a, b, what=None):
    assert a.numbers.tolist() == b.numbers.tolist() and a.voffsets.tolist() == b.voffsets.tolist(), what
    assert a.offsets.tolist() == b.offsets.tolist() and bytes(a.data) == bytes(b.data) and a.searched == b.searched, what


@pytest.mark.parametrize("name", INPUTS + ["awkward"])
def test_one_line_records_equal_grep(ctx, inputs, awkward, tmp_path, name):
    from zlib_ng_amd import bgzf
    assert sorted(INPUTS) == sorted(inputs)
    blob, delims = (awkward[1], [b"\n", b"\x00", b"\x80"]) if name == "awkward" else inputs[name]
    data = gzip.decompress(blob)
    path = tmp_path / "t.bgzf"
    path.write_bytes(blob)
    rng = random.Random(11)
    with bgzf.open(str(path)) as r:
        for delim in delims:
            for pats in pattern_sets(rng, data, delim):
                for mode in MODES:
                    what = (name, delim, pats[:2], mode)
                    same(r.grep_records(pats, 1, delimiter=delim, **mode), r.grep(pats, delimiter=delim, **mode), what)
                    same(r.grep_records(pats, 1, match_line=0, delimiter=delim, allow_short=True, **mode), r.grep(pats, delimiter=delim, **mode), what)
                assert r.grep_records(pats, 1, delimiter=delim, count=True) == r.grep(pats, delimiter=delim, count=True)
                part = r.grep_records(pats, 1, delimiter=delim, max_count=3, first_record=50)
                same(part, r.grep(pats, delimiter=delim, max_count=3, first_line=50), (name, delim, pats[:2], "max_count"))


_texts = {}


def mixed_text():
    """about 100 KiB of lines of 0 to 400 bytes over a small alphabet, some of 255 bytes and more; 8 * 331 + 5 lines, no final delimiter"""
    if "mixed" not in _texts:
        rng = random.Random(21)
        lines = []
        for i in range(8 * 331 + 5):
            n = rng.choice([0, 1, 3, 12, 30, 60]) if i % 11 else rng.randrange(255, 400)
            lines.append(bytes(rng.choice(b"ACGTN@+") for _ in range(n)))
        _texts["mixed"] = b"\n".join(lines[:-1] + [b"END"])
    return _texts["mixed"]


@pytest.mark.parametrize("block_size", [37, 65280])
@pytest.mark.parametrize("k", [2, 4, 8])
def test_against_the_referee(ctx, tmp_path, k, block_size):
    from zlib_ng_amd import bgzf
    data = mixed_text()
    assert (data.count(b"\n") + 1) % k                              # the last record is short
    blob = bgzf.compress(data, block_size=block_size)
    path = tmp_path / "m.bgzf"
    path.write_bytes(blob)
    tab, by_c = block_map(blob)
    rng = random.Random(k)
    sets = pattern_sets(rng, data, b"\n")
    assert {len(s) for s in sets} >= {1, 64} and any(len(s[0]) == 255 for s in sets) and any(len(s[0]) == 1 for s in sets)
    with bgzf.open(str(path)) as r:
        for pats in sets:
            for j in [None] + list(range(k)):
                for mode in MODES:
                    what = (k, block_size, pats[:2], j, mode)
                    recs, sel = referee_records(data, b"\n", k, pats, j, **mode)
                    res = r.grep_records(pats, k, match_line=j, allow_short=True, **mode)
                    assert res.searched == len(recs), what
                    check_result(res, recs, sel, by_c, r if j in (None, 1) and not mode else None, rng, what)
        with pytest.raises(ValueError, match=r"record %d, the last one, has %d of %d lines" % (len(recs) - 1, (data.count(b"\n") + 1) % k, k)):
            r.grep_records(sets[0], k)


def rec(l0, l1, l2, l3, needle_in=(), tag=b"x"):
    """one record of four lines with these lengths (delimiters included); NEEDLE in the lines named"""
    out = []
    for i, n in enumerate((l0, l1, l2, l3)):
        body = bytearray((b"@" if i == 0 else b"") + tag * n)[:n - 1]
        if i in needle_in:
            at = (n - 1 - 6) // 2
            body[at:at + 6] = b"NEEDLE"
        out.append(bytes(body) + b"\n")
    return b"".join(out)


def tile_edge_text():
    """-> (text, {name: record number}): records of four lines placed against the edges of the 16 KiB tiles and 64 KiB blocks"""
    recs, at, where = [], 0, {}

    def add(r, name=None):
        nonlocal at
        if name:
            where[name] = len(recs)
        recs.append(r)
        at += len(r)

    def pad_to(pos):                                                # filler records up to `pos`
        while pos - at > 3000:
            add(rec(10, 900, 2, 900, tag=b"p"))
        add(rec(10, pos - at - 42, 2, 30, tag=b"q"))
        assert at == pos

    add(rec(10, 30, 2, 30, (1,)), "plain")
    pad_to(T - 50)
    add(rec(10, 30, 2, 30, (1,)), "match line ends in t, last line in t + 1")            # lines end at T - 41, T - 11, T - 9, T + 21
    pad_to(2 * T - 15)
    add(rec(15, 40, 2, 40, (1,)), "first line in t, match line in t + 1")                # line 1 is [2T, 2T + 40)
    add(rec(10, 40, 2, 40, (3,)), "needle in line 3 only")
    add(rec(10, 20000, 2, 20000, (1,)), "longer than a tile")
    add(rec(10, 20000, 2, 20000, (0,)), "longer than a tile, needle in line 0")
    add(rec(10, 70000, 2, 70000, (3,)), "longer than a block")
    add(rec(10, 70000, 2, 70000, (1,)), "longer than a block, needle in line 1")
    pad_to((at // T + 2) * T)
    add(rec(10, 30, 2, 30, (1,)), "starts a tile")
    add(rec(10, 30, 12, 30, (2,)), "needle in line 2")
    add(rec(10, 30, 2, 30), "no needle")
    add(rec(10, 30, 12, 30, (0, 1, 2, 3)), "needles everywhere")
    return recs, where


def test_placement_at_tile_edges(ctx, tmp_path, monkeypatch):
    from zlib_ng_amd import bgzf
    recs, where = tile_edge_text()
    data = b"".join(recs)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])]).tolist()

    def line_ends(name):                                            # where the four lines of the record end (their delimiters)
        r, out, at = recs[where[name]], [], starts[where[name]]
        for ln in r.split(b"\n")[:-1]:
            at += len(ln) + 1
            out.append(at - 1)
        return out
    e = line_ends("match line ends in t, last line in t + 1")
    assert e[1] // T == 0 and e[3] // T == 1
    e = line_ends("first line in t, match line in t + 1")
    assert e[0] == 2 * T - 1 and (e[0] + 1) // T == e[1] // T == 2 and starts[where["first line in t, match line in t + 1"]] // T == 1
    assert len(recs[where["longer than a tile"]]) > T and len(recs[where["longer than a block"]]) > 65536
    assert starts[where["starts a tile"]] % T == 0 and starts[where["starts a tile"]] > 0
    for level, window in ((6, None), (0, 1)):                       # stored blocks and a window of one byte: the windows cut the long records
        blob = bgzf.compress(data, level)
        path = tmp_path / "edges.bgzf"
        path.write_bytes(blob)
        tab, by_c = block_map(blob)
        with bgzf.open(str(path)) as r:
            for j in (None, 0, 1, 2, 3):
                for mode in MODES:
                    pats = [b"NEEDLE"] if not mode.get("line_start") else [b"@x"]
                    wrecs, sel = referee_records(data, b"\n", 4, pats, j, **mode)
                    assert wrecs == recs
                    if window:                                      # (for the search alone: the reader's own reads below keep their window)
                        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
                    ctx.bgzf_stats()
                    res = r.grep_records(pats, 4, match_line=j, first_byte=b"@", **mode)
                    launches = ctx.bgzf_stats()[0]
                    monkeypatch.undo()
                    assert launches == 1 if not window else launches >= 4      # (400 KiB in windows of 64 KiB, and the long records make them grow)
                    assert res.searched == len(recs)
                    check_result(res, recs, sel, by_c, r, random.Random(2), (level, j, mode))
    want = [where[n] for n in ("plain", "match line ends in t, last line in t + 1", "first line in t, match line in t + 1", "longer than a tile",
                               "longer than a block, needle in line 1", "starts a tile", "needles everywhere")]
    assert referee_records(data, b"\n", 4, [b"NEEDLE"], 1)[1] == want


def test_windows(ctx, tmp_path, monkeypatch):
    """a reading window of one byte over 37-byte blocks (64 KiB of the file per window): the same result, one launch per window, and
    only the blocks of the open record -- at most two, a record is shorter than a block -- are decoded again"""
    from zlib_ng_amd import bgzf
    rng = random.Random(31)
    recs = [b"".join(bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 8))) + b"\n" for _ in range(4)) for _ in range(9000)]
    assert max(len(x) for x in recs) <= 36
    data = b"".join(recs)
    blob = bgzf.compress(data, 0, block_size=37)
    path = tmp_path / "w.bgzf"
    path.write_bytes(blob)
    tab, by_c = block_map(blob)
    whole = {}
    for j in (None, 2):
        whole[j] = bgzf.grep_records(str(path), b"GAT", 4, match_line=j)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1)
    for j in (None, 2):
        wrecs, sel = referee_records(data, b"\n", 4, [b"GAT"], j)
        ctx.bgzf_stats()
        res = bgzf.grep_records(str(path), b"GAT", 4, match_line=j)
        launches, decoded, _ = ctx.bgzf_stats()
        assert launches >= 3 and launches <= len(blob) // 65536 + 2, launches
        assert decoded <= len(tab) + 2 * launches, (launches, decoded, len(tab))
        assert res.searched == len(recs) and 100 < len(sel) < len(recs)
        check_result(res, recs, sel, by_c, what=j)
        same(res, whole[j])


def test_the_fastq_fixture(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    blob = open(BGZIP, "rb").read()
    data = gzip.decompress(blob)
    tab, by_c = block_map(blob)
    lines = data.split(b"\n")
    pat = lines[4 * 777 + 1][5:17]                                  # twelve bases of read 777
    recs, sel = referee_records(data, b"\n", 4, [pat], 1)
    assert 777 in sel and len(lines[-1]) == 0 and (len(lines) - 1) % 4 == 0
    with bgzf.open(BGZIP) as r:
        res = r.grep_records(pat, 4, match_line=1, first_byte=b"@")
        assert res.searched == len(recs)
        for x in res:
            assert x.count(b"\n") == 4 and x.startswith(b"@") and x.endswith(b"\n")
        check_result(res, recs, sel, by_c, r, random.Random(3))
        # count and max_count count records
        assert r.grep_records(pat, 4, match_line=1, count=True) == len(sel)
        _, every = referee_records(data, b"\n", 4, [b"GATC"], 1)
        assert len(every) > 50
        assert r.grep_records(b"GATC", 4, match_line=1, count=True) == len(every)
        for n in (0, 1, len(every) // 2, len(every) + 3):
            part = r.grep_records(b"GATC", 4, match_line=1, max_count=n)
            check_result(part, recs, every[:n], by_c, what=n)
            assert r.grep_records(b"GATC", 4, match_line=1, max_count=n, count=True) == min(n, len(every))
        # the shards of a line index, each searched on its own
        idx = bgzf.LineIndex.build(BGZIP)
        cuts = idx.shards(r, 3, lines_per_record=4)
        firsts = [i * len(recs) // 3 for i in range(4)]
        parts = [r.grep_records(b"GATC", 4, match_line=1, first_byte=b"@", start=cuts[i], stop=cuts[i + 1], first_record=firsts[i]) for i in range(3)]
        assert [p.searched for p in parts] == [b - a for a, b in zip(firsts, firsts[1:])]
        full = r.grep_records(b"GATC", 4, match_line=1)
        assert sum((p.numbers.tolist() for p in parts), []) == full.numbers.tolist() == every
        assert sum((p.voffsets.tolist() for p in parts), []) == full.voffsets.tolist()
        assert b"".join(bytes(p.data) for p in parts) == bytes(full.data)
        assert sum(r.grep_records(b"GATC", 4, match_line=1, start=cuts[i], stop=cuts[i + 1], count=True) for i in range(3)) == len(every)
    # one line removed: every record behind it is shifted
    del lines[4 * 500 + 2]
    broken = b"\n".join(lines)
    bblob = bgzf.compress(broken)
    path = tmp_path / "broken.bgzf"
    path.write_bytes(bblob)
    brecs = referee_records(broken, b"\n", 4, [pat])[0]
    bad = next(i for i, x in enumerate(brecs) if not x.startswith(b"@"))
    assert bad == 501
    btab, _ = block_map(bblob)
    pos = sum(len(x) for x in brecs[:bad])
    c, u, cs, isz = [row for row in btab if row[1] <= pos < row[1] + row[3]][0]
    with pytest.raises(ValueError, match=r"record %d at virtual offset %d does not start with b'@'" % (bad, c << 16 | pos - u)):
        bgzf.grep_records(str(path), pat, 4, match_line=1, first_byte=b"@")
    with pytest.raises(ValueError, match=r"record %d at virtual offset" % bad):
        bgzf.grep_records(str(path), pat, 4, match_line=1, first_byte=b"@", count=True)
    # ... and the last record is short
    assert len(brecs[-1].split(b"\n")) == 4
    with pytest.raises(ValueError, match=r"record %d, the last one, has 3 of 4 lines" % (len(brecs) - 1)):
        bgzf.grep_records(str(path), pat, 4)
    tail = brecs[-1].split(b"\n")[0][:9]
    wrecs, sel = referee_records(broken, b"\n", 4, [tail])
    assert sel[-1] == len(brecs) - 1
    res = bgzf.grep_records(str(path), tail, 4, allow_short=True)
    check_result(res, wrecs, sel, block_map(bblob)[1])
    assert res[-1] == brecs[-1] and res[-1].count(b"\n") == 3


# ---- the C entry points directly
def c_referee(data, text_off, text_end, delim, k, pats, flags, match_line, first_byte, base):
    """what zngamd_bgzf_grep_records reports for data[text_off:text_end): (seen, rows [(src_off, number, len)], tail_off, short_lines, bad)"""
    from zlib_ng_amd import _lib
    text, d = data[text_off:text_end], bytes([delim])
    parts = text.split(d)
    lines = [p + d for p in parts[:-1]]
    final = bool(flags & _lib.BGZF_GREP_FINAL)
    if parts[-1] and final:
        lines.append(parts[-1])
    nrec = (len(lines) + k - 1) // k if final else len(lines) // k
    starts = [text_off]
    for ln in lines:
        starts.append(starts[-1] + len(ln))
    rows, bad = [], None
    for r in range(nrec):
        group = lines[k * r:k * r + k]
        look = group if match_line < 0 else group[match_line:match_line + 1]
        hit = any(ln.startswith(p) if flags & _lib.BGZF_GREP_LINE_START else p in ln for ln in look for p in pats)
        if first_byte >= 0 and group[0][0] != first_byte and bad is None:
            bad = (base + r, starts[k * r])
        if hit != bool(flags & _lib.BGZF_GREP_INVERT):
            rows.append((starts[k * r], base + r, sum(len(x) for x in group)))
    return nrec, rows, (text_end if final else starts[k * nrec]), (len(lines) % k if final else 0), bad


def test_entry_point(ctx, awkward):
    from zlib_ng_amd import _lib
    data, blob, tab = awkward
    members = member_table(tab)
    arr = np.frombuffer(data, np.uint8)
    rng = random.Random(6)
    F = _lib.BGZF_GREP_FINAL
    for delim in (0, 10, 0x80, 0xff):
        cuts = (np.nonzero(arr == delim)[0] + 1).tolist()
        alphabet = [b for b in b"\x00\x01\x02\x7f\x80\x81\xff\n\x0b" if b != delim]
        for trial in range(5):
            k = rng.choice([1, 2, 3, 4, 7, 64])
            j = rng.choice([-1, rng.randrange(k)])
            fb = rng.choice([-1, rng.choice(alphabet)])
            pats = [bytes(rng.choice(alphabet) for _ in range(rng.choice([1, 1, 2, 3]))) for _ in range(rng.choice([1, 2, 64]))]
            table = _lib.grep_pattern_table(pats)
            text_off = rng.choice([0] + cuts[:50])
            text_end = max(text_off, rng.choice([len(data), len(data), rng.choice(cuts), rng.randrange(text_off, len(data) + 1)]))
            for flags in (0, F, _lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_LINE_START | F, _lib.BGZF_GREP_INVERT | F):
                seen, rows, tail, short, bad = c_referee(data, text_off, text_end, delim, k, pats, flags, j, fb, 1000)
                what = (delim, trial, k, j, fb, flags, text_off, text_end)
                ctx.bgzf_stats()
                code, status, tot, got, packed = ctx.bgzf_grep_records(blob, members, text_off, text_end, *table, delim, flags, k, j, fb, 1000)
                assert ctx.bgzf_stats()[:2] == (1, len(tab))
                assert code == 0 and not status.any() and tot.covered == 1, what
                assert (tot.seen, tot.selected, tot.tail_off, tot.short_lines) == (seen, len(rows), tail, short), what
                assert tot.bytes == sum(n for _, _, n in rows), what
                if bad is not None:
                    assert (tot.bad, tot.bad_record, tot.bad_src) == (1, *bad) and len(got) == 0 and packed == b"", what
                    continue
                assert tot.bad == 0, what
                assert [(int(r["src_off"]), int(r["number"]), int(r["len"])) for r in got] == rows, what
                assert packed == b"".join(data[s:s + n] for s, _, n in rows), what
                code, status, tot2, got2, packed2 = ctx.bgzf_grep_records(blob, members, text_off, text_end, *table, delim,
                                                                          flags | _lib.BGZF_GREP_COUNT_ONLY, k, j, fb, 1000)
                assert (tot2.seen, tot2.selected, tot2.bytes, tot2.tail_off, len(got2), packed2) == (seen, len(rows), tot.bytes, tail, 0, b""), what
    # arguments
    table = _lib.grep_pattern_table([b"\x01"])
    for k, j, fb in ((0, -1, -1), (65, -1, -1), (4, 4, -1), (4, -2, -1), (4, 0, 256), (4, 0, -2)):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_grep_records(blob, members, 0, len(data), *table, 10, 0, k, j, fb)
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_grep_records(blob, members, 0, len(data) + 1, *table, 10, 0, 4)
    tot = ctx.bgzf_grep_records(blob, members[:0], 0, 0, *table, 10, F, 4)[2]
    assert (tot.covered, tot.seen, tot.tail_off) == (1, 0, 0)
    # the host form's capacities
    seen, rows, tail, short, bad = c_referee(data, 0, len(data), 10, 3, [b"\x01"], F, -1, -1, 0)
    nbytes = sum(n for _, _, n in rows)
    assert len(rows) > 100
    for caps in ((len(rows) - 1, nbytes), (len(rows), nbytes - 1), (0, 0)):
        code, status, tot, got, packed = ctx.bgzf_grep_records(blob, members, 0, len(data), *table, 10, F, 3, caps=caps)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.selected, tot.bytes, tot.covered) == (seen, len(rows), nbytes, 1) and len(got) == 0 and packed == b""
    code, status, tot, got, packed = ctx.bgzf_grep_records(blob, members, 0, len(data), *table, 10, F, 3, caps=(len(rows), nbytes))
    assert code == 0 and got["src_off"].tolist() == [s for s, _, _ in rows] and len(packed) == nbytes


def test_tables_are_untrusted(ctx, awkward):
    """a table with a gap, an overlap, rows out of order, a block that did not decode: covered = 0, no rows"""
    from zlib_ng_amd import _lib
    data, blob, tab = awkward
    members = member_table(tab)
    table = _lib.grep_pattern_table([b"\x01"])
    F = _lib.BGZF_GREP_FINAL

    def run(m, lo=0, hi=len(data)):
        code, status, tot, got, packed = ctx.bgzf_grep_records(blob, m, lo, hi, *table, 10, F, 4, 1)
        assert code == 0
        return status, tot, got, packed

    gap = np.delete(members, 7)
    status, tot, got, packed = run(gap)
    assert not status.any() and (tot.covered, tot.seen, tot.selected, tot.bytes, tot.bad) == (0, 0, 0, 0, 0) and len(got) == 0 and packed == b""
    status, tot, got, packed = run(gap, 0, tab[7][1])                 # the same table covers a text in front of the gap
    seen, rows, tail, short, bad = c_referee(data, 0, tab[7][1], 10, 4, [b"\x01"], F, 1, -1, 0)
    assert tot.covered == 1 and (tot.seen, tot.selected) == (seen, len(rows)) and got["src_off"].tolist() == [s for s, _, _ in rows]
    overlap = members.copy()
    overlap["out_off"][9] -= 3
    assert run(overlap)[1].covered == 0
    swapped = members.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert run(swapped)[1].covered == 0
    hostile = members.copy()
    hostile["in_off"][5] = len(blob) + 1000                           # block 5 does not decode
    status, tot, got, packed = run(hostile)
    assert [bool(s) for s in status.tolist()] == [i == 5 for i in range(len(tab))]
    assert (tot.covered, tot.selected) == (0, 0) and len(got) == 0 and packed == b""
    assert run(hostile, 0, tab[5][1])[1].covered == 1 and run(hostile, 0, tab[5][1] + 1)[1].covered == 0


def test_device_form(ctx, awkward):
    """zngamd_bgzf_grep_records_dev on device buffers: capacities one below the totals write nothing"""
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
    seen, rows, tail, short, bad = c_referee(data, text_off, text_end, 10, 3, pats, 0, -1, -1, 7)
    nbytes = sum(ln for _, _, ln in rows)
    assert len(rows) > 20 and tail < text_end
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, cap), devmem.empty(ctx, 4 * n)
    d_rows, d_out = devmem.empty(ctx, 24 * len(rows)).zero_(), devmem.empty(ctx, nbytes).zero_()
    args = (d_in.ptr, len(blob), d_m.ptr, n, text_off, text_end, *table, 10, 0, 3, -1, -1, 7, d_scratch.ptr, cap, d_st.ptr)
    for rcap, ocap in ((len(rows) - 1, nbytes), (len(rows), nbytes - 1)):
        code, tot = ctx.bgzf_grep_records_dev(*args, d_rows.ptr, rcap, d_out.ptr, ocap)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.selected, tot.bytes, tot.tail_off, tot.covered) == (seen, len(rows), nbytes, tail, 1)
        assert d_rows.cpu().tobytes() == bytes(24 * len(rows)) and d_out.cpu().tobytes() == bytes(nbytes)
    code, tot = ctx.bgzf_grep_records_dev(*args, d_rows.ptr, len(rows), d_out.ptr, nbytes)
    assert code == 0 and (tot.seen, tot.selected, tot.bytes, tot.tail_off, tot.covered, tot.bad) == (seen, len(rows), nbytes, tail, 1, 0)
    got = d_rows.cpu(_lib.GREP_ROW_DTYPE)
    assert [(int(r["src_off"]), int(r["number"]), int(r["len"])) for r in got] == rows
    assert d_out.cpu().tobytes() == b"".join(data[s:s + ln] for s, _, ln in rows)
    assert [bool(s) for s in d_st.cpu(np.int32).tolist()] == [i >= 30 for i in range(n)]
    code, tot = ctx.bgzf_grep_records_dev(*args[:5], tab[30][1] + 5, *args[6:], d_rows.ptr, len(rows), d_out.ptr, nbytes)      # block 30 touches the text and failed
    assert code == 0 and (tot.covered, tot.selected) == (0, 0)
    code, tot = ctx.bgzf_grep_records_dev(*args[:9], _lib.BGZF_GREP_COUNT_ONLY, *args[10:], 0, 0, 0, 0)
    assert code == 0 and (tot.seen, tot.selected, tot.covered) == (seen, len(rows), 1)

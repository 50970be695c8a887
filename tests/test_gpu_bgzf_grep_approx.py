"""BGZF by content with mismatches (bgzf.grep / grep_records with mismatches=k; csrc/za_grep.hip: za_k_grep_mark_approx).  The
referee is numpy on the bytes the system gzip decodes, never the code under test: for each pattern the mismatches of every window
are summed byte by byte (data[j : n - L + 1 + j] != p[j] over j), windows that hold a delimiter are dropped by a prefix sum of the
delimiters, with line_start the start must be the first byte of a line, and a line is hit when a surviving start lies in it.  The sum
is taken eight bytes at a time and windows that are past k already are left out of the bytes that follow: a count never falls, so
the result is that of the whole sum."""
import gzip
import random

import numpy as np
import pytest

from test_gpu_bgzf_grep import MODES, block_map, check_result, straddling
from test_gpu_bgzf_lines import BGZIP, BLOCK, awkward, inputs, member_table, referee_lines      # noqa: F401  (inputs, awkward: fixtures)

pytestmark = pytest.mark.gpu

INPUTS = ["eof only", "one delimiter", "one byte", "fastq", "bgzip", "long line", "only delimiters", "edges", "small blocks", "text",
          "two streams", "crlf", "urandom"]


def hit_lines(text, delim, pats, k, line_start=False, both=False):
    """-> the sorted numbers of the lines of `text` (bytes; delim: an int) that a pattern matches with at most k mismatches; both: the
    pair of lists without and with line_start"""
    arr = np.frombuffer(text, np.uint8)
    n = len(arr)
    isd = arr == delim
    before = np.concatenate([[0], np.cumsum(isd, dtype=np.int64)])           # before[i]: delimiters in text[:i] = the line of byte i
    starts = [np.empty(0, np.int64)]
    for p in pats:
        L = len(p)
        if L > n:
            continue
        pos, cnt = None, np.zeros(n - L + 1, np.uint8)                       # (a count is 255 at most)
        for j0 in range(0, L, 8):
            for j in range(j0, min(j0 + 8, L)):
                cnt += (arr[j:n - L + 1 + j] if pos is None else arr[pos + j]) != p[j]
            keep = np.nonzero(cnt <= k)[0]
            pos, cnt = (keep if pos is None else pos[keep]), cnt[keep]
        starts.append(pos[before[pos + L] == before[pos]])                   # no delimiter inside the window
    pos = np.concatenate(starts)
    anywhere = np.unique(before[pos]).tolist()
    pos = pos[(pos == 0) | isd[np.maximum(pos, 1) - 1]]                      # the first byte of a line
    at_start = np.unique(before[pos]).tolist()
    return (anywhere, at_start) if both else at_start if line_start else anywhere


def referee(data, delim, pats, k, invert=False, line_start=False):
    """-> (the lines, the numbers of the selected ones)"""
    lines = referee_lines(data, delim)
    hit = set(hit_lines(data, delim[0], pats, k, line_start))
    return lines, [i for i in range(len(lines)) if (i in hit) != invert]


def mutate(rng, p, m, delim, where="random"):
    """p with m of its bytes substituted by values that are neither the original nor the delimiter; where: the first place"""
    q, L = bytearray(p), len(p)
    at = {"first": {0}, "second": {min(1, L - 1)}, "last": {L - 1}, "random": set()}[where] if m else set()
    while len(at) < m:
        at.add(rng.randrange(L))
    for i in at:
        q[i] = rng.choice([b for b in range(256) if b != p[i] and b != delim[0]])
    return bytes(q)


def pattern_sets(rng, data, delim, k):
    """pattern lists cut from the data and mutated in 0, k and k + 1 places (first byte, second byte, last byte, anywhere): a piece
    of a line, a whole line, a line's first bytes, 255 bytes where a line is that long, and with k = 1 64 pieces of 2 to 12 bytes"""
    bodies = [ln[:-1] if ln.endswith(delim) else ln for ln in referee_lines(data, delim)]
    bodies = [b for b in bodies if len(b) > k]
    if not bodies:
        return [[bytes(b for b in b"\x02nowhere in the data at all\x03" if b != delim[0])]]
    sets = []
    pieces = []
    for m, where in ((0, "random"), (k, "first"), (k + 1, "second"), (k, "random")):
        b = rng.choice(bodies)
        L = rng.randrange(k + 1, max(k + 1, min(len(b), 40)) + 1)
        o = rng.randrange(len(b) - L + 1)
        pieces.append(mutate(rng, b[o:o + L], m, delim, where))
    sets.append(pieces)
    whole = rng.choice(bodies)[:255]
    first = rng.choice(bodies)
    first2 = rng.choice(bodies)
    sets.append([mutate(rng, whole, k, delim, "last"), mutate(rng, first[:max(k + 1, min(len(first), 24))], k, delim, "second"),
                 mutate(rng, first2[:max(k + 1, min(len(first2), 9))], k + 1, delim, "first")])
    longs = [x for x in bodies if len(x) >= 255]
    if longs:
        x, y = rng.choice(longs), rng.choice(longs)
        o, o2 = rng.randrange(len(x) - 254), rng.randrange(len(y) - 254)
        sets.append([mutate(rng, x[o:o + 255], k, delim, "first"), mutate(rng, y[o2:o2 + 255], k + 1, delim, "last")])
    short = [b for b in bodies if len(b) >= 2]
    if k == 1 and short:
        many = []
        while len(many) < 64:
            x = rng.choice(short)
            L = rng.randrange(2, min(len(x), 12) + 1)
            o = rng.randrange(len(x) - L + 1)
            many.append(mutate(rng, x[o:o + L], len(many) % 3 if L > 2 else len(many) % 2, delim, ("first", "second", "last", "random")[len(many) % 4]))
        sets.append(many)
    return sets


@pytest.mark.parametrize("name", INPUTS)
def test_against_the_referee(ctx, inputs, tmp_path, name):
    from zlib_ng_amd import bgzf
    rng = random.Random(INPUTS.index(name))
    blob, delims = inputs[name]
    path = tmp_path / "t.bgzf"
    path.write_bytes(blob)
    data = gzip.decompress(blob)
    tab, by_c = block_map(blob)
    for delim in delims:
        idx = bgzf.LineIndex.build(str(path), delim)
        all_lines = referee_lines(data, delim)
        with bgzf.open(str(path)) as r:
            for k in (1, 2, 16):
                for pats in pattern_sets(rng, data, delim, k):
                    assert min(len(p) for p in pats) > k
                    hit = dict(zip((False, True), map(set, hit_lines(data, delim[0], pats, k, both=True))))
                    for mode in MODES:
                        what = (name, delim, k, pats[:3], mode)
                        sel = [i for i in range(len(all_lines)) if (i in hit[bool(mode.get("line_start"))]) != bool(mode.get("invert"))]
                        res = r.grep(pats if len(pats) > 1 else pats[0], delimiter=delim, mismatches=k, **mode)
                        assert res.searched == len(all_lines), what
                        check_result(res, all_lines, sel, by_c, r, rng, what)
                        assert r.grep(pats, delimiter=delim, count=True, mismatches=k, **mode) == len(sel), what
                        for n in (1, len(sel) // 2):
                            part = r.grep(pats, delimiter=delim, max_count=n, mismatches=k, **mode)
                            check_result(part, all_lines, sel[:n], by_c, what=what + (n,))
                            assert r.grep(pats, delimiter=delim, max_count=n, count=True, mismatches=k, **mode) == min(n, len(sel))
                    # the parts LineIndex.shards gives, each searched on its own
                    sel = sorted(hit[False])
                    cuts = idx.shards(r, 3)
                    firsts = [min(i * idx.lines // 3, idx.lines) for i in range(4)]
                    parts = [r.grep(pats, delimiter=delim, start=cuts[i], stop=cuts[i + 1], first_line=firsts[i], mismatches=k) for i in range(3)]
                    assert [p.searched for p in parts] == [b - a for a, b in zip(firsts, firsts[1:])], (name, delim, k)
                    assert sum((p.numbers.tolist() for p in parts), []) == sel, (name, delim, k)
                    assert b"".join(bytes(p.data) for p in parts) == b"".join(all_lines[i] for i in sel)


def same(a, b, what):
    assert a.numbers.tolist() == b.numbers.tolist() and a.voffsets.tolist() == b.voffsets.tolist() and a.offsets.tolist() == b.offsets.tolist(), what
    assert bytes(a.data) == bytes(b.data) and a.searched == b.searched, what


def test_no_mismatches_is_the_exact_search(ctx, inputs, tmp_path):
    from zlib_ng_amd import bgzf
    rng = random.Random(21)
    for name in ("fastq", "text"):
        blob, delims = inputs[name]
        path = tmp_path / "t.bgzf"
        path.write_bytes(blob)
        data = gzip.decompress(blob)
        bodies = [b for b in data.split(delims[0]) if len(b) > 8]
        pats = [rng.choice(bodies)[2:8], rng.choice(bodies)[:5], b"\x02absent"]
        with bgzf.open(str(path)) as r:
            for mode in MODES:
                same(r.grep(pats, delimiter=delims[0], mismatches=0, **mode), r.grep(pats, delimiter=delims[0], **mode), (name, mode))
                assert r.grep(pats, delimiter=delims[0], mismatches=0, count=True, **mode) == r.grep(pats, delimiter=delims[0], count=True, **mode)
        if name == "fastq":
            for mode in (dict(), dict(invert=True)):
                same(bgzf.grep_records(str(path), pats[0], 4, match_line=1, first_byte=b"@", mismatches=0, **mode),
                     bgzf.grep_records(str(path), pats[0], 4, match_line=1, first_byte=b"@", **mode), (name, mode))


def run_case(tmp_path, data, delim, pats, k, bs, want=None):
    """data through bgzf.compress(block_size=bs) and a reader, all four modes against the referee; want: the numbers of the lines
    that match in the plain mode, said by hand"""
    from zlib_ng_amd import bgzf
    path = tmp_path / "c.bgzf"
    blob = bgzf.compress(data, block_size=bs)
    path.write_bytes(blob)
    assert gzip.decompress(blob) == data
    tab, by_c = block_map(blob)
    with bgzf.open(str(path)) as r:
        for mode in MODES:
            lines, sel = referee(data, delim, pats, k, **mode)
            if want is not None and not mode:
                assert sel == want, (data[:12], pats, k)
            res = r.grep(pats, delimiter=delim, mismatches=k, **mode)
            assert res.searched == len(lines)
            check_result(res, lines, sel, by_c, r, random.Random(1), (data[:12], [p[:12] for p in pats], k, bs, mode))


def test_edges_by_hand(ctx, tmp_path):
    # the only window with one mismatch spans the delimiter
    run_case(tmp_path, b"AAAA\nAAAA\n", b"\n", [b"A" * 9], 1, 4, [])
    run_case(tmp_path, b"AAAA\nAAAA\n", b"\n", [b"A" * 9], 8, 65280, [])
    # a last line without a delimiter whose final window matches with exactly k mismatches; one byte shorter, nothing does
    tail = b"one\ntwo\nxxACGTACGTAC"
    for k, pat in ((1, b"ACGTACGTAG"), (2, b"TCGTACGTAG"), (3, b"TCGTTCGTAG")):
        run_case(tmp_path, tail, b"\n", [pat], k, 5, [2])
        run_case(tmp_path, tail[:-1], b"\n", [pat], k, 5, [])
    # a pattern longer than every line
    run_case(tmp_path, b"abc\nabcdef\nab\n\nabcde", b"\n", [b"abcdefg"], 6, 3, [])
    run_case(tmp_path, b"abc\nabcdef\nab\n\nabcde", b"\n", [b"abcdefg", b"zbcdef"], 1, 3, [1])
    # k = len - 1 on two bytes: every line of at least two bytes matches
    run_case(tmp_path, b"a\nab\n\nabc\nq\nzz\nz", b"\n", [b"ab"], 1, 65280, [1, 3])
    run_case(tmp_path, b"a\nqb\n\nxyz\nq\nzz\nzb", b"\n", [b"ab"], 1, 2, [1, 6])
    # bytes whose compare could carry into a neighbour, with delimiters at both ends of the range
    rng = random.Random(17)
    alphabet = b"\x00\x01\x7f\x80\x81\xff"
    data = bytes(rng.choice(alphabet) for _ in range(3000))
    for delim in (b"\x00", b"\x7f", b"\xff"):
        letters = bytes(b for b in alphabet if b != delim[0])
        for k in (1, 2):
            pats = [bytes(rng.choice(letters) for _ in range(L)) for L in (3, 4, 5, 6)]
            run_case(tmp_path, data, delim, pats, k, 257)
            run_case(tmp_path, data, delim, pats[2:3], k, 65280)
    # the last partial word of a pattern: lengths 1 (k = 0 only) to 9, planted with len - 1 or fewer bytes right
    text = b"".join(bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(0, 40))) + b"\n" for _ in range(400))
    run_case(tmp_path, text, b"\n", [b"G"], 0, 65280)
    for L in (2, 3, 4, 5, 7, 8, 9):
        for k in sorted({1, L - 1}):
            pats = [bytes(rng.choice(b"ACGT") for _ in range(L)) for _ in range(2)]
            run_case(tmp_path, text, b"\n", pats, k, 997)
            run_case(tmp_path, text + pats[0][:-1] + b"N", b"\n", pats[:1], k, 997)          # ... its last byte wrong, in the last line
            if k == 1 and L > 2:
                run_case(tmp_path, text + pats[0][:-2] + b"NN", b"\n", pats[:1], k, 997)      # two wrong: the last word's live bytes count


def planted(rng):
    """straddling() of the exact test with its needle replaced by 255 bytes that differ from the pattern in 16 places: across 16 KiB
    tile edges of the text and across block edges; and a pattern whose window begins in the last byte of a tile"""
    data, needle = straddling(rng)
    pat = bytes(rng.choice(b"0123456789abcdef") for _ in range(255))
    body = bytearray(data)
    at = 0
    spots = []
    while True:
        at = data.find(needle, at)
        if at < 0:
            break
        spots.append(at)
        at += 1
    assert len(spots) == 6
    for i, s in enumerate(spots):
        s -= 120                                               # the needle straddled the edge by half its 18 bytes: so do the 255
        body[s:s + 255] = mutate(rng, pat, 17 if i == 3 else 16, b"\n")
    last = 3 * 200000 + 16384 - (3 * 200000) % 16384 - 1 + 5 * 16384      # the last byte of a tile, inside line 3
    assert last % 16384 == 16383 and last // 200000 == 3
    small = b"tile's last byte"
    body[last:last + len(small)] = mutate(rng, small, 2, b"\n", "first")
    return bytes(body), pat, small


def test_tile_and_block_edges(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    rng = random.Random(9)
    data, pat, small = planted(rng)
    path = tmp_path / "long.bgzf"
    blob = bgzf.compress(data)
    path.write_bytes(blob)
    tab, by_c = block_map(blob)
    for pats, k in (([pat], 16), ([pat], 15), ([small], 2), ([small], 1), ([small, pat], 2)):
        lines, sel = referee(data, b"\n", pats, k)
        res = bgzf.grep(str(path), pats, mismatches=k)
        check_result(res, lines, sel, by_c, what=(pats[0][:8], k))
    assert referee(data, b"\n", [pat], 16)[1] == [1, 2, 4, 7, 8] and referee(data, b"\n", [small], 2)[1] == [3] and referee(data, b"\n", [small], 1)[1] == []


def test_small_read_windows(ctx, inputs, tmp_path, monkeypatch):
    """near-matches straddle windows; the open line's blocks are decoded again, and no more than that"""
    from zlib_ng_amd import bgzf
    rng = random.Random(10)
    data, pat, small = planted(rng)
    blob = bgzf.compress(data)
    path = tmp_path / "long.bgzf"
    path.write_bytes(blob)
    tab, by_c = block_map(blob)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 100000)
    for pats, k, mode in (([pat], 16, {}), ([pat], 16, dict(invert=True)), ([small, pat], 2, {}), ([mutate(rng, data[:200], 3, b"\n")], 3, dict(line_start=True))):
        lines, sel = referee(data, b"\n", pats, k, **mode)
        ctx.bgzf_stats()
        res = bgzf.grep(str(path), pats, mismatches=k, **mode)
        assert ctx.bgzf_stats()[0] > 9                                # the windows grew: every line is longer than the first window
        assert res.searched == len(lines)
        check_result(res, lines, sel, by_c, what=(pats[0][:8], k, mode))
    blob = inputs["fastq"][0]
    data = gzip.decompress(blob)
    path = tmp_path / "short.bgzf"
    path.write_bytes(blob)
    tab, by_c = block_map(blob)
    for k in (1, 2):
        for pats in pattern_sets(rng, data, b"\n", k)[:2]:
            for mode in MODES[:3]:
                lines, sel = referee(data, b"\n", pats, k, **mode)
                ctx.bgzf_stats()
                res = bgzf.grep(str(path), pats, mismatches=k, **mode)
                launches, decoded, _ = ctx.bgzf_stats()
                check_result(res, lines, sel, by_c, what=(pats[:2], k, mode))
                assert res.searched == len(lines)
                assert 3 <= launches <= len(blob) // bgzf._READ_WINDOW + 2 and decoded <= len(tab) + 2 * launches, (launches, decoded, len(tab))
                n = len(sel) // 3
                ctx.bgzf_stats()
                part = bgzf.grep(str(path), pats, max_count=n, mismatches=k, **mode)
                assert part.numbers.tolist() == sel[:n] and ctx.bgzf_stats()[0] <= launches


# ---- the C entry points directly
def c_referee(data, text_off, text_end, delim, pats, k, flags, line_base):
    """what zngamd_bgzf_grep_approx reports for data[text_off:text_end): (seen, rows [(src_off, number, len)], tail_off)"""
    from zlib_ng_amd import _lib
    text = data[text_off:text_end]
    d = bytes([delim])
    lines = referee_lines(text, d)
    hit = set(hit_lines(text, delim, pats, k, bool(flags & _lib.BGZF_GREP_LINE_START)))      # (the text ends at text_end: so do the windows)
    tail = text_end
    if lines and not lines[-1].endswith(d) and not flags & _lib.BGZF_GREP_FINAL:
        tail = text_end - len(lines.pop())
    rows, at = [], text_off
    for i, ln in enumerate(lines):
        if (i in hit) != bool(flags & _lib.BGZF_GREP_INVERT):
            rows.append((at, line_base + i, len(ln)))
        at += len(ln)
    return len(lines), rows, tail


def clean_window(arr, delim, L, rng, lo=2000):
    """a place behind `lo` where L bytes hold no delimiter"""
    isd = np.concatenate([[0], np.cumsum(arr == delim)])
    free = np.nonzero(isd[L:] == isd[:-L])[0]
    return int(rng.choice(free[free > lo].tolist()))


def test_entry_point(ctx, awkward):
    from zlib_ng_amd import _lib
    data, blob, tab = awkward
    members = member_table(tab)
    arr = np.frombuffer(data, np.uint8)
    rng = random.Random(4)
    F = _lib.BGZF_GREP_FINAL

    def check(text_off, text_end, pats, k, delim, flags, what):
        table = _lib.grep_pattern_table(pats)
        seen, rows, tail = c_referee(data, text_off, text_end, delim, pats, k, flags, 1000)
        code, status, tot, got, packed = ctx.bgzf_grep(blob, members, text_off, text_end, *table, delim, flags, 1000, mismatches=k)
        assert code == 0 and not status.any() and tot.covered == 1, what
        assert (tot.seen, tot.matched, tot.tail_off) == (seen, len(rows), tail), what
        assert [(int(r["src_off"]), int(r["number"]), int(r["len"])) for r in got] == rows, what
        assert packed == b"".join(data[s:s + n] for s, _, n in rows) and tot.bytes == len(packed), what
        assert (got["reserved"] == 0).all()
        return rows, tail

    for delim in (0, 10, 0x7f, 0xff):
        cuts = (np.nonzero(arr == delim)[0] + 1).tolist()
        alphabet = [b for b in b"\x00\x01\x02\x7f\x80\x81\xff\n\x0b" if b != delim]
        for trial in range(4):
            k = rng.choice([1, 1, 2])
            pats = [bytes(rng.choice(alphabet) for _ in range(rng.choice([k + 1, 3, 4, 5, 6]))) for _ in range(rng.choice([1, 2, 64]))]
            text_off = rng.choice([0] + cuts[:50])
            text_end = max(text_off, rng.choice([len(data), rng.choice(cuts), rng.randrange(text_off, len(data) + 1)]))      # inside blocks
            for flags in (0, F, _lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_LINE_START | F, _lib.BGZF_GREP_LINE_START | _lib.BGZF_GREP_INVERT):
                check(text_off, text_end, pats, k, delim, flags, (delim, trial, k, flags, text_off, text_end))
    # a near-match at the end of the text: twelve bytes without a delimiter, one of them substituted in the pattern
    L, delim = 12, 10
    s = clean_window(arr, delim, L, rng)
    pat = mutate(rng, data[s:s + L], 1, b"\n", "last")
    line0 = data.rfind(b"\n", 0, s) + 1                                  # where the line of the window starts
    text_off = data.rfind(b"\n", 0, line0 - 1) + 1                       # the line in front of it
    assert s + L < len(data) and tab[-1][1] > s + L                      # the scratch holds the bytes behind text_end
    assert hit_lines(data[text_off:line0], delim, [pat], 1) == []
    rows, tail = check(text_off, s + L - 1, [pat], 1, delim, F, "the window needs the byte at text_end")
    assert rows == [] and tail == s + L - 1
    rows, tail = check(text_off, s + L, [pat], 1, delim, F, "the window ends at text_end")
    assert rows == [(line0, 1001, s + L - line0)]
    rows, tail = check(text_off, s + L, [pat], 1, delim, 0, "the same without _FINAL: the open tail")
    assert rows == [] and tail == line0
    rows, tail = check(text_off, s + L, [pat], 1, delim, _lib.BGZF_GREP_INVERT, "the line in front is selected by _INVERT")
    assert [r[1] for r in rows] == [1000] and tail == line0
    # the sizing protocol
    pats = [b"\x01\x80"]
    table = _lib.grep_pattern_table(pats)
    seen, rows, tail = c_referee(data, 0, len(data), 10, pats, 1, F, 0)
    nbytes = sum(n for _, _, n in rows)
    assert len(rows) > 100
    for caps in ((len(rows) - 1, nbytes), (len(rows), nbytes - 1)):
        code, status, tot, got, packed = ctx.bgzf_grep(blob, members, 0, len(data), *table, 10, F, 0, caps, mismatches=1)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.matched, tot.bytes, tot.covered) == (seen, len(rows), nbytes, 1) and len(got) == 0 and packed == b""
    code, status, tot, got, packed = ctx.bgzf_grep(blob, members, 0, len(data), *table, 10, F, 0, (len(rows), nbytes), mismatches=1)
    assert code == 0 and got["src_off"].tolist() == [s for s, _, _ in rows] and len(packed) == nbytes
    # the tables are untrusted: rows out of order, a block inside the text that does not decode -- covered = 0 and nothing else
    swapped = members.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    hostile = members.copy()
    hostile["in_off"][5] = len(blob) + 1000
    for m in (swapped, hostile):
        code, status, tot, got, packed = ctx.bgzf_grep(blob, m, 0, len(data), *table, 10, F, 0, mismatches=1)
        assert code == 0 and (tot.covered, tot.seen, tot.matched, tot.bytes) == (0, 0, 0, 0) and len(got) == 0 and packed == b""
    assert [bool(s) for s in status.tolist()] == [i == 5 for i in range(len(tab))]
    # arguments
    for bad_k in (2, 3, 17, 1 << 31):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_grep(blob, members, 0, len(data), *table, 10, F, 0, mismatches=bad_k)


def test_device_form(ctx, awkward):
    """zngamd_bgzf_grep_approx_dev gives the rows and bytes of the host form"""
    from zlib_ng_amd import _lib, devmem
    data, blob, tab = awkward
    members = member_table(tab)
    n = len(tab)
    pats = [b"\x80\x01\x7f", b"\x01\x01\xff\x02"]
    table = _lib.grep_pattern_table(pats)
    arr = np.frombuffer(data, np.uint8)
    text_off = int(np.nonzero(arr == 10)[0][3]) + 1
    text_end = tab[30][1] + 77
    code, status, tot_h, rows_h, packed_h = ctx.bgzf_grep(blob, members, text_off, text_end, *table, 10, 0, 7, mismatches=1)
    seen, rows, tail = c_referee(data, text_off, text_end, 10, pats, 1, 0, 7)
    assert code == 0 and len(rows) > 20 and [(int(r["src_off"]), int(r["number"]), int(r["len"])) for r in rows_h] == rows
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, len(data)), devmem.empty(ctx, 4 * n)
    d_rows, d_out = devmem.empty(ctx, 24 * len(rows)).zero_(), devmem.empty(ctx, len(packed_h)).zero_()
    args = (d_in.ptr, len(blob), d_m.ptr, n, text_off, text_end, *table, 10, 0, 7, d_scratch.ptr, len(data), d_st.ptr)
    code, tot = ctx.bgzf_grep_dev(*args, d_rows.ptr, len(rows) - 1, d_out.ptr, len(packed_h), mismatches=1)
    assert code == _lib.BUF_ERROR and (tot.seen, tot.matched, tot.bytes, tot.tail_off, tot.covered) == (seen, len(rows), len(packed_h), tail, 1)
    assert d_rows.cpu().tobytes() == bytes(24 * len(rows))
    code, tot = ctx.bgzf_grep_dev(*args, d_rows.ptr, len(rows), d_out.ptr, len(packed_h), mismatches=1)
    assert code == 0 and (tot.seen, tot.matched, tot.bytes, tot.tail_off, tot.covered) == (tot_h.seen, tot_h.matched, tot_h.bytes, tot_h.tail_off, 1)
    assert d_rows.cpu(_lib.GREP_ROW_DTYPE).tobytes() == rows_h.tobytes() and d_out.cpu().tobytes() == bytes(packed_h)


# ---- records
def test_records(ctx, tmp_path):
    from zlib_ng_amd import _lib, bgzf, devmem
    blob = open(BGZIP, "rb").read()
    data = gzip.decompress(blob)
    lines = referee_lines(data, b"\n")
    assert len(lines) % 4 == 0 and all(ln.startswith(b"@") for ln in lines[::4])
    nrec = len(lines) // 4
    rng = random.Random(6)
    r0 = rng.randrange(nrec)
    bases = lines[4 * r0 + 1][:-1]
    o = rng.randrange(len(bases) - 12)
    piece = bytearray(bases[o:o + 12])
    piece[5] = rng.choice([b for b in b"ACGT" if b != piece[5]])
    pat = bytes(piece)

    def records_of(pats, k, only=None):
        ids = np.array(hit_lines(data, 10, pats, k), np.int64)
        return sorted(set((ids[ids % 4 == only] if only is not None else ids) // 4))

    want = records_of([pat], 1, 1)                                   # numpy on line 1 of the records only
    assert r0 in want

    def check(res, sel):
        assert res.numbers.tolist() == sel and res.searched == nrec
        assert bytes(res.data) == b"".join(b"".join(lines[4 * i:4 * i + 4]) for i in sel)

    check(bgzf.grep_records(BGZIP, pat, 4, match_line=1, first_byte=b"@", mismatches=1), want)
    check(bgzf.grep_records(BGZIP, pat, 4, match_line=1, first_byte=b"@", mismatches=1, invert=True), [i for i in range(nrec) if i not in set(want)])
    assert bgzf.grep_records(BGZIP, pat, 4, match_line=1, first_byte=b"@", mismatches=1, count=True) == len(want)
    assert bgzf.grep_records(BGZIP, pat, 4, match_line=1, first_byte=b"@", mismatches=1, invert=True, count=True) == nrec - len(want)
    exact = records_of([pat], 0, 1)
    assert r0 not in exact
    check(bgzf.grep_records(BGZIP, pat, 4, match_line=1, first_byte=b"@"), exact)
    # the same near-match in a quality line only
    qual = lines[4 * r0 + 3][:-1]
    q = bytearray(qual[o:o + 12])
    q[0] = 0x7e if q[0] != 0x7e else 0x7d
    qpat = bytes(q)
    assert records_of([qpat], 1, 1) == [] and r0 in records_of([qpat], 1)
    check(bgzf.grep_records(BGZIP, qpat, 4, match_line=1, first_byte=b"@", mismatches=1), [])
    check(bgzf.grep_records(BGZIP, qpat, 4, first_byte=b"@", mismatches=1), records_of([qpat], 1))
    with bgzf.open(BGZIP) as r:
        check(r.grep_records(qpat, 4, match_line=3, mismatches=1), records_of([qpat], 1, 3))
    # the device form gives the rows and bytes of the host form
    _, tab, _, _ = _lib.bgzf_scan(blob)
    members = member_table(tab)
    table = _lib.grep_pattern_table([pat])
    F = _lib.BGZF_GREP_FINAL
    code, status, tot_h, rows_h, packed_h = ctx.bgzf_grep_records(blob, members, 0, len(data), *table, 10, F, 4, 1, ord("@"), 0, mismatches=1)
    assert code == 0 and rows_h["number"].tolist() == want and tot_h.seen == nrec
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, len(data)), devmem.empty(ctx, 4 * len(tab))
    d_rows, d_out = devmem.empty(ctx, 24 * len(want)).zero_(), devmem.empty(ctx, len(packed_h)).zero_()
    code, tot = ctx.bgzf_grep_records_dev(d_in.ptr, len(blob), d_m.ptr, len(tab), 0, len(data), *table, 10, F, 4, 1, ord("@"), 0, d_scratch.ptr, len(data),
                                          d_st.ptr, d_rows.ptr, len(want), d_out.ptr, len(packed_h), mismatches=1)
    assert code == 0 and (tot.seen, tot.selected, tot.bytes, tot.covered, tot.bad) == (nrec, len(want), len(packed_h), 1, 0)
    assert d_rows.cpu(_lib.GREP_ROW_DTYPE).tobytes() == rows_h.tobytes() and d_out.cpu().tobytes() == bytes(packed_h)

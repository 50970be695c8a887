"""BGZF by line (bgzf.LineIndex, BgzfReader.read_lines / line_voffsets, LineIndex.shards; csrc/za_bgzf.hip: za_k_bgzf_count,
za_k_bgzf_select).  The referee is Python on the bytes the system gzip decodes: data.split(delimiter); per-block counts come from
numpy on the block cuts of the host scan."""
import gzip
import io
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BLOCK = 65280
BGZIP = os.path.join(GOLDEN, "test.fastq.bgzip.gz")


def referee_lines(data, delim):
    parts = data.split(delim)
    return [p + delim for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


@pytest.fixture(scope="module")
def inputs(fastq):
    """name -> (the BGZF stream, the delimiters to index it by)"""
    from zlib_ng_amd import bgzf, corpus
    rng = random.Random(3)
    text = corpus.text(3 * BLOCK + 17, 7).tobytes()
    crlf = b"".join(b"line %d of some text\r\n" % i for i in range(9000)) + b"no end"
    edge = b"abc\n" + b"\nxyz" + b"abc\n" + b"\n\n\n\n" + b"last"           # block_size 4: a delimiter ends a block, the next block starts with one
    words = b"".join(bytes(rng.choice(b"ab\n") for _ in range(rng.randrange(0, 9))) + b"\n" for _ in range(4000))
    return {
        "eof only": (bgzf.EOF_BLOCK, [b"\n"]),
        "one delimiter": (bgzf.compress(b"\n"), [b"\n"]),
        "one byte": (bgzf.compress(b"x"), [b"\n"]),
        "fastq": (bgzf.compress(fastq), [b"\n"]),
        "bgzip": (open(BGZIP, "rb").read(), [b"\n"]),
        "long line": (bgzf.compress(b"short\n" * 5 + b"A" * 200000 + b"\n" + b"tail\nend"), [b"\n"]),
        "only delimiters": (bgzf.compress(b"\n" * (3 * BLOCK)), [b"\n"]),
        "edges": (bgzf.compress(edge, block_size=4), [b"\n"]),
        "small blocks": (bgzf.compress(words, block_size=37), [b"\n", b"a"]),
        "text": (bgzf.compress(text, block_size=1001), [b"\n", b" ", b"e"]),
        "two streams": (bgzf.compress(text[:100000] + b"\n") + bgzf.compress(b"second\nstream\n" * 3000 + b"open"), [b"\n"]),
        "crlf": (bgzf.compress(crlf), [b"\n"]),
        "urandom": (bgzf.compress(os.urandom(2 * BLOCK + 1000)), [b"\n", b"\x00"]),
    }


def referee_blocks(blob, data, delim):
    """[(coffset, uoffset, delimiters in front, last byte is one)] of every block but the EOF block at the end, from the host scan"""
    from zlib_ng_amd import _lib
    code, tab, used, total = _lib.bgzf_scan(blob)
    assert code == 0 and used == len(blob) and total == len(data)
    arr = np.frombuffer(data, np.uint8)
    rows, before = [], 0
    for c, u, cs, isz in tab:
        n = int(np.count_nonzero(arr[u:u + isz] == delim[0]))
        rows.append((c, u, before, bool(isz) and data[u + isz - 1] == delim[0]))
        before += n
    if tab and tab[-1][3] == 0:
        rows.pop()
    return tab, rows


def random_ranges(rng, nlines, k):
    ranges = [(0, nlines), (0, nlines + 100), (max(nlines - 1, 0), 1), (max(nlines - 1, 0), 5), (nlines, 1), (nlines + 7, 2), (0, 0),
              (nlines // 2, 0), (0, 1)]
    for _ in range(k):
        a = rng.randrange(0, nlines + 3)
        n = rng.choice([0, 1, 1, 1, 2, 4, 4, 17, rng.randrange(0, 400), rng.randrange(0, nlines + 2)])
        ranges.append((a, n))
    return ranges


def test_index_and_lines_against_the_referee(ctx, inputs, tmp_path):
    from zlib_ng_amd import bgzf
    rng = random.Random(11)
    for name, (blob, delims) in inputs.items():
        path = tmp_path / "t.bgzf"
        path.write_bytes(blob)
        data = gzip.decompress(blob)
        for delim in delims:
            lines = referee_lines(data, delim)
            assert b"".join(lines) == data
            tab, rows = referee_blocks(blob, data, delim)
            idx = bgzf.LineIndex.build(str(path), delim)
            assert idx.blocks == rows, name
            assert (idx.lines, len(idx), idx.usize, idx.file_size, idx.delimiter) == (len(lines), len(rows), len(data), len(blob), delim), name
            with open(path, "rb") as f:
                assert bgzf.LineIndex.build(f, delim) == idx
            assert bgzf.LineIndex.from_bytes(idx.to_bytes(), len(blob)) == idx
            if name == "only delimiters":
                assert [b - a for a, b in zip([r[2] for r in rows], [r[2] for r in rows[1:]] + [idx.delimiters])] == [BLOCK] * 3
            by_c = {c: (u, isz) for c, u, cs, isz in tab}
            starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).tolist()        # starts[i] = offset of line i; the last: len(data)
            with bgzf.open(str(path)) as r:
                # ---- read_lines
                ranges = random_ranges(rng, len(lines), 300)
                ctx.bgzf_stats()
                got = r.read_lines(idx, ranges)
                launches, decoded, _ = ctx.bgzf_stats()
                assert len(got) == len(ranges)
                for (a, n), g in zip(ranges, got):
                    assert g == b"".join(lines[a:a + n]), (name, delim, a, n)
                # economy: one launch; no more blocks than the lines lie in, plus one per range
                live = [(a, min(a + n, len(lines))) for a, n in ranges if n and a < len(lines)]
                touched = set()
                for a, e in live:
                    touched.update(i for i, (c, u, cs, isz) in enumerate(tab) if isz and u < starts[e] and u + isz > starts[a])
                assert launches == (1 if live else 0) and decoded <= len(touched) + len(live), (name, launches, decoded, len(touched))
                assert r.read_lines(idx, []) == [] and r.read_lines(idx, [(len(lines), 3)]) == [b""]
                assert ctx.bgzf_stats()[0] == 0                      # nothing to decode for ranges without lines
                for bad in ([(-1, 1)], [(0, -1)]):
                    with pytest.raises(ValueError):
                        r.read_lines(idx, bad)
                # ---- line_voffsets: normalised, and seek() goes there
                pick = sorted(set(range(min(len(lines), 40))) | set(rng.sample(range(len(lines)), min(len(lines), 120))) | {max(len(lines) - 1, 0)})
                pick = [i for i in pick if i < len(lines)] + [len(lines)]
                ctx.bgzf_stats()
                voffs = r.line_voffsets(idx, pick)
                assert ctx.bgzf_stats()[0] <= 1
                for i, v in zip(pick, voffs):
                    c, u = bgzf.split_virtual_offset(v)
                    assert c in by_c, (name, i)
                    assert by_c[c][0] + u == starts[i], (name, i)
                    if i < len(lines):
                        assert u < by_c[c][1], (name, i, "not normalised")
                    else:
                        assert u == 0 and by_c[c][0] == len(data)
                    r.seek(v)
                    if i == len(lines):
                        assert r.read(10) == b""
                    elif delim == b"\n" and len(lines[i]) < 5000:
                        assert r.readline() == lines[i], (name, i)
                    else:
                        assert r.read(len(lines[i])) == lines[i], (name, i)
                with pytest.raises(IndexError):
                    r.line_voffsets(idx, [len(lines) + 1])
                # ---- shards
                for n in (1, 2, 3, 7):
                    for per in (1, 4):
                        cuts = idx.shards(r, n, per)
                        assert len(cuts) == n + 1
                        offs = []
                        for v in cuts:
                            c, u = bgzf.split_virtual_offset(v)
                            offs.append(by_c[c][0] + u)
                        assert offs[0] == 0 and offs[-1] == len(data) and offs == sorted(offs)
                        record_starts = np.array(starts[:len(lines):per], np.int64)
                        at = np.searchsorted(record_starts, offs)              # records in front of every cut
                        assert all(o == len(data) or (k < len(record_starts) and record_starts[k] == o) for o, k in zip(offs, at)), (name, n, per)
                        sizes = np.diff(at).tolist()
                        assert max(sizes) - min(sizes) <= 1 and sum(sizes) == len(record_starts), (name, n, per, sizes)
                        assert b"".join(data[a:b] for a, b in zip(offs, offs[1:])) == data
                with pytest.raises(ValueError):
                    idx.shards(r, 0)


@pytest.mark.parametrize("name", ["fastq", "bgzip", "text"])
def test_only_the_blocks_of_the_lines_are_decoded(ctx, inputs, tmp_path, name):
    """a few short ranges on a file of many blocks: one launch, and no more blocks than the lines lie in plus one per range -- here
    exactly the referee's blocks, far fewer than the file has; line_voffsets decodes the blocks of the lines that start inside one"""
    from zlib_ng_amd import bgzf
    blob, delim = inputs[name][0], b"\n"
    path = tmp_path / "t.bgzf"
    path.write_bytes(blob)
    data = gzip.decompress(blob)
    lines = referee_lines(data, delim)
    tab, rows = referee_blocks(blob, data, delim)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).tolist()
    full = [i for i, (c, u, cs, isz) in enumerate(tab) if isz]
    assert len(full) >= 50

    def blocks_of(lo, hi):
        """the blocks that hold a byte of data[lo:hi]"""
        return {i for i in full if tab[i][1] < hi and tab[i][1] + tab[i][3] > lo}

    idx = bgzf.LineIndex.build(str(path), delim)
    rng = random.Random(21)
    block_starts = {tab[i][1] for i in full}
    at_a_block = [i for i in range(len(lines)) if starts[i] in block_starts]
    with bgzf.open(str(path)) as r:
        for trial in range(8):
            ranges = [(rng.randrange(len(lines)), rng.choice([1, 1, 2, 5])) for _ in range(rng.choice([1, 2, 3]))]
            ranges += [(len(lines) + 1, 2), (3, 0), (len(lines) - 1, 4)][:trial % 4]
            live = [(a, min(a + n, len(lines))) for a, n in ranges if n and a < len(lines)]
            touched = set().union(*(blocks_of(starts[a], starts[e]) for a, e in live))
            assert len(touched) + len(live) <= len(full) // 4                 # the bound says something: most of the file stays out
            ctx.bgzf_stats()
            got = r.read_lines(idx, ranges)
            launches, decoded, _ = ctx.bgzf_stats()
            assert got == [b"".join(lines[a:a + n]) for a, n in ranges]
            assert launches == 1 and decoded <= len(touched) + len(live), (name, ranges, decoded, len(touched))
            assert decoded == len(touched), (name, ranges, decoded, len(touched))
            # line_voffsets: a line that starts where a block starts needs no block at all
            pick = [rng.randrange(len(lines)) for _ in range(rng.choice([1, 4]))] + [0, len(lines)] + at_a_block[trial:trial + 2]
            inside = {min(blocks_of(starts[i], starts[i] + 1)) for i in pick if i < len(lines) and starts[i] not in block_starts}
            ctx.bgzf_stats()
            voffs = r.line_voffsets(idx, pick)
            launches, decoded, _ = ctx.bgzf_stats()
            assert launches == (1 if inside else 0) and decoded == len(inside) <= len(pick), (name, pick, decoded, len(inside))
            for i, v in zip(pick, voffs):
                r.seek(v)
                assert r.read(20) == data[starts[i]:starts[i] + 20]
        ctx.bgzf_stats()
        r.line_voffsets(idx, [0, len(lines)] + at_a_block[:3])
        assert ctx.bgzf_stats()[:2] == (0, 0)


def test_writer_helper(ctx, tmp_path, fastq):
    from zlib_ng_amd import bgzf
    path, ipath = str(tmp_path / "w.bgzf"), str(tmp_path / "w.lidx")
    piece = fastq[:700000]
    w = bgzf.open(path, "wb")
    w.write(piece)
    with pytest.raises(ValueError):
        w.write_line_index(ipath)
    w.close()
    idx = w.write_line_index(ipath)
    assert bgzf.LineIndex.load(ipath, os.path.getsize(path)) == idx
    lines = referee_lines(piece, b"\n")
    assert idx.lines == len(lines)
    with bgzf.open(path) as r:
        assert r.read_lines(idx, [(4 * 100, 4), (0, 1)]) == [b"".join(lines[400:404]), lines[0]]


def test_damage(ctx, tmp_path, fastq):
    from zlib_ng_amd import _lib, bgzf
    blob = bytearray(bgzf.compress(fastq[:10 * BLOCK]))
    data = fastq[:10 * BLOCK]
    lines = referee_lines(data, b"\n")
    good, bad = str(tmp_path / "good.bgzf"), str(tmp_path / "bad.bgzf")
    open(good, "wb").write(blob)
    idx = bgzf.LineIndex.build(good)
    _, tab, _, _ = _lib.bgzf_scan(bytes(blob))
    c, u, cs, isz = tab[4]
    blob[c + 18 + cs // 2] ^= 0x5A                                          # a payload byte of block 4
    open(bad, "wb").write(blob)
    with pytest.raises(bgzf.BadGzipFile, match=f"offset {c}:"):
        bgzf.LineIndex.build(bad)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])]).tolist()
    clear = [i for i in range(len(lines)) if starts[i + 1] <= u or starts[i] >= u + isz]
    hit = [i for i in range(len(lines)) if starts[i] < u + isz and starts[i + 1] > u]
    assert len(hit) > 100 and len(clear) > 1000
    rng = random.Random(2)
    with bgzf.open(bad) as r:
        ranges = [(i, 1) for i in rng.sample(clear, 300)] + [(0, hit[0]), (hit[-1] + 1, 50)]
        got = r.read_lines(idx, ranges)
        for (a, n), g in zip(ranges, got):
            assert g == b"".join(lines[a:a + n])
        for rg in ([(hit[0], 1)], [(hit[len(hit) // 2], 1)], [(hit[-1], 1)], [(hit[0] - 3, len(hit) + 6)], [(5, 1), (0, len(lines))]):
            with pytest.raises(bgzf.BadGzipFile, match=f"offset {c}:"):
                r.read_lines(idx, rg)
        with pytest.raises(bgzf.BadGzipFile, match=f"offset {c}:"):
            r.line_voffsets(idx, [hit[len(hit) // 2]])
        assert len(r.line_voffsets(idx, clear[:50])) == 50


def test_stale_index(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    a = b"".join(b"record %d\n" % i for i in range(30000))
    b = a.replace(b"\n", b" ")                                              # the same bytes per block (level 0: stored), no line structure
    pa, pb, pc = (str(tmp_path / n) for n in ("a.bgzf", "b.bgzf", "c.bgzf"))
    open(pa, "wb").write(bgzf.compress(a, 0))
    open(pb, "wb").write(bgzf.compress(b, 0))
    open(pc, "wb").write(bgzf.compress(a + b"more\n", 0))
    assert os.path.getsize(pa) == os.path.getsize(pb) != os.path.getsize(pc)
    idx = bgzf.LineIndex.build(pa)
    with bgzf.open(pa) as r:
        assert r.read_lines(idx, [(5, 2)]) == [b"record 5\nrecord 6\n"]
    for path in (pb, pc):
        with bgzf.open(path) as r:
            with pytest.raises(ValueError, match="line index does not match the file"):
                r.read_lines(idx, [(5, 2)])
            with pytest.raises(ValueError, match="line index does not match the file"):
                r.read_lines(idx, [(0, 20000)])
            with pytest.raises(ValueError, match="line index does not match the file"):
                r.line_voffsets(idx, [7])
    with pytest.raises(ValueError):
        bgzf.LineIndex.load(io.BytesIO(idx.to_bytes()), os.path.getsize(pc))


# ---- the C entry points directly
def member_table(tab):
    """the blocks of a host scan (18-byte headers) as members, outputs packed"""
    from zlib_ng_amd import bgzf
    m = np.zeros(len(tab), bgzf.MEMBER_DTYPE)
    m["in_off"] = [c + 18 for c, u, cs, isz in tab]
    m["in_len"] = [cs - 26 for c, u, cs, isz in tab]
    m["out_off"] = [u for c, u, cs, isz in tab]
    m["out_len"] = [isz for c, u, cs, isz in tab]
    return m


@pytest.fixture(scope="module")
def awkward():
    """bytes around the delimiters that a carry between bytes would miscount (0x01 above 0x00, 0x80, 0xff), in blocks whose outputs
    start at odd addresses"""
    from zlib_ng_amd import _lib, bgzf
    rng = random.Random(8)
    data = bytes(rng.choice(b"\x00\x01\x01\x02\x7f\x80\x81\xff\n\x0b") for _ in range(40 * 1001 + 13))
    blob = bgzf.compress(data, block_size=1001)
    _, tab, _, _ = _lib.bgzf_scan(blob)
    return data, blob, tab


def test_count_entry_point(ctx, awkward, inputs):
    from zlib_ng_amd import _lib
    cases = [awkward]
    for name in ("bgzip", "only delimiters", "urandom"):
        blob = inputs[name][0]
        cases.append((gzip.decompress(blob), blob, _lib.bgzf_scan(blob)[1]))
    for data, blob, tab in cases:
        arr = np.frombuffer(data, np.uint8)
        members = member_table(tab)
        for delim in (0, 1, 10, 0x7f, 0x80, 0xff):
            ctx.bgzf_stats()
            status, rows = ctx.bgzf_count(blob, members, delim)
            assert ctx.bgzf_stats()[:2] == (1, len(tab))
            assert not status.any()
            want = [(int(np.count_nonzero(arr[u:u + isz] == delim)), int(bool(isz) and arr[u + isz - 1] == delim)) for c, u, cs, isz in tab]
            assert rows.tolist() == [list(w) for w in want], delim
    data, blob, tab = awkward
    for bad in (-1, 256):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_count(blob, member_table(tab), bad)
    status, rows = ctx.bgzf_count(blob, member_table(tab)[:0], 10)
    assert len(status) == 0 and len(rows) == 0


def test_tables_are_untrusted(ctx, awkward):
    """indices, offsets and ranks outside their bounds: verdicts, and nothing read or written outside the buffers"""
    from zlib_ng_amd import _lib
    OK, BLOCK_, TABLE, RANK = _lib.BGZF_SLICE_OK, _lib.BGZF_SLICE_BLOCK, _lib.BGZF_SLICE_TABLE, _lib.BGZF_SLICE_RANK
    END = _lib.BGZF_RANK_END
    data, blob, tab = awkward
    arr = np.frombuffer(data, np.uint8)
    members = member_table(tab)
    n = len(tab)
    nl = [int(np.count_nonzero(arr[u:u + isz] == 10)) for c, u, cs, isz in tab]

    def behind(m, r):
        c, u, cs, isz = tab[m]
        return u + int(np.nonzero(arr[u:u + isz] == 10)[0][r - 1]) + 1

    assert min(nl[:5]) >= 3
    q = [(0, 0), (0, 1), (0, nl[0]), (0, nl[0] + 1), (0, 1 << 31), (0, END - 1), (0, END), (3, 2), (n - 1, 0), (n - 1, END),      # n - 1: the EOF block
         (n, 0), (n, 1), (0xFFFFFFFF, 0), (0xFFFFFFFF, END), (1 << 31, 5)]
    status, pos, verdicts = ctx.bgzf_line_positions(blob, members, np.array(q, np.uint32), 10)
    assert not status.any()
    assert verdicts.tolist() == [OK, OK, OK, RANK, RANK, RANK, OK, OK, OK, OK, TABLE, TABLE, TABLE, TABLE, TABLE]
    assert pos.tolist() == [0, behind(0, 1), behind(0, nl[0]), 0, 0, 0, tab[0][3], behind(3, 2), len(data), len(data), 0, 0, 0, 0, 0]

    # every rank of a block, and the ranges between them
    m = 2
    q = [(m, r) for r in range(nl[m] + 1)]
    status, pos, verdicts = ctx.bgzf_line_positions(blob, members, np.array(q, np.uint32), 10)
    assert not verdicts.any() and pos.tolist() == [tab[m][1]] + [behind(m, r) for r in range(1, nl[m] + 1)]

    # hostile members: a block outside the input, one whose output would not fit a block, one that lies about its length
    hostile = members.copy()
    hostile["in_off"][1] = len(blob) + 1000
    hostile["in_off"][5] = 1 << 47
    hostile["out_len"][7] += 1
    status, rows = ctx.bgzf_count(blob, hostile, 10)
    assert [bool(s) for s in status.tolist()] == [i in (1, 5, 7) for i in range(n)]
    assert rows.tolist() == [[0, 0] if i in (1, 5, 7) else [nl[i], int(bool(tab[i][3]) and arr[tab[i][1] + tab[i][3] - 1] == 10)] for i in range(n)]
    ranges = [(0, 0, 0, END), (0, 1, 2, 1), (1, 0, 1, END), (0, 0, 1, 1), (4, 1, 6, 1), (6, 0, 8, 0), (2, 2, 2, 1), (3, 1, 2, END), (2, 0, 3, nl[3] + 1),
              (n, 0, n, 0), (0, 0, 0xFFFFFFFF, 0), (8, 1, 8, 1), (9, 0, 10, END)]
    code, status, verdicts, lens, packed, need = ctx.bgzf_read_lines(blob, hostile, np.array(ranges, np.uint32), 10, 1 << 20)
    assert code == 0
    want = [(OK, data[:tab[0][3]]), (BLOCK_, None), (BLOCK_, b""), (BLOCK_, b""), (BLOCK_, None), (BLOCK_, None), (TABLE, b""), (TABLE, b""),
            (RANK, b""), (TABLE, b""), (TABLE, b""), (OK, b""), (OK, data[tab[9][1]:tab[10][1] + tab[10][3]])]
    assert verdicts.tolist() == [w[0] for w in want]
    at = 0
    for (v, body), ln, rg in zip(want, lens.tolist(), ranges):
        piece = packed[at:at + ln]
        at += ln
        assert piece == (bytes(ln) if body is None else body), rg          # never the bytes of a block that failed
    assert at == len(packed) == need
    # the same with too little room: the size comes back, no lines
    code, status, verdicts2, lens2, packed2, need2 = ctx.bgzf_read_lines(blob, hostile, np.array(ranges, np.uint32), 10, need - 1)
    assert code == _lib.BUF_ERROR and need2 == need and packed2 == b"" and lens2.tolist() == lens.tolist()
    # and with no room given: the result is allocated once its size is known
    code, status, verdicts3, lens3, packed3, need3 = ctx.bgzf_read_lines(blob, hostile, np.array(ranges, np.uint32), 10)
    assert code == 0 and (need3, packed3, lens3.tolist(), verdicts3.tolist()) == (need, packed, lens.tolist(), verdicts.tolist())
    assert ctx.bgzf_read_lines(blob, hostile, np.array(ranges[2:4], np.uint32), 10)[4:] == (b"", 0)
    for field, value in (("in_off", 1 << 63), ("in_len", (1 << 64) - 1), ("out_off", 1 << 50)):
        wild = members.copy()
        wild[field][3] = value
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_count(blob, wild, 10)
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_read_lines(blob, wild, np.array(ranges, np.uint32), 10, 1 << 20)


def test_device_forms(ctx, awkward):
    """the _dev entry points on device memory, with a scratch that is shorter than the member table says"""
    from zlib_ng_amd import _lib, devmem
    OK, BLOCK_, TABLE, RANK = _lib.BGZF_SLICE_OK, _lib.BGZF_SLICE_BLOCK, _lib.BGZF_SLICE_TABLE, _lib.BGZF_SLICE_RANK
    END = _lib.BGZF_RANK_END
    data, blob, tab = awkward
    arr = np.frombuffer(data, np.uint8)
    members = member_table(tab)
    n = len(tab)
    cap = tab[30][1] + 5                                             # block 30 and everything behind it lie outside the scratch
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch = devmem.empty(ctx, cap)
    d_st, d_rows = devmem.empty(ctx, 4 * n), devmem.empty(ctx, 8 * n)
    ctx.bgzf_count_dev(d_in.ptr, len(blob), d_m.ptr, n, 10, d_scratch.ptr, cap, d_st.ptr, d_rows.ptr)
    st = d_st.cpu(np.int32).tolist()
    assert [bool(s) for s in st] == [i >= 30 for i in range(n)]
    rows = d_rows.cpu(np.uint32).reshape(-1, 2).tolist()
    assert rows == [[0, 0] if i >= 30 else [int(np.count_nonzero(arr[u:u + isz] == 10)), int(arr[u + isz - 1] == 10)]
                    for i, (c, u, cs, isz) in enumerate(tab)]
    assert d_scratch.cpu().tobytes()[:tab[30][1]] == data[:tab[30][1]]

    q = np.array([(29, 1), (29, END), (30, 0), (30, 1), (n - 1, END), (n, 0)], np.uint32)
    d_q, d_pos, d_ps = devmem.from_host(ctx, q.tobytes()), devmem.empty(ctx, 8 * len(q)), devmem.empty(ctx, 4 * len(q))
    ctx.bgzf_line_positions_dev(d_in.ptr, len(blob), d_m.ptr, n, d_q.ptr, len(q), 10, d_scratch.ptr, cap, d_st.ptr, d_pos.ptr, d_ps.ptr)
    first = tab[29][1] + int(np.nonzero(arr[tab[29][1]:tab[30][1]] == 10)[0][0]) + 1
    assert d_ps.cpu(np.int32).tolist() == [OK, OK, TABLE, TABLE, TABLE, TABLE]
    assert d_pos.cpu(np.uint64).tolist() == [first, tab[30][1], 0, 0, 0, 0]

    ranges = np.array([(0, 0, 1, END), (28, 1, 29, END), (29, 0, 30, 1), (5, 1, 5, 1), (7, 0, 7, 1 << 20)], np.uint32)
    d_r, d_len, d_rs = devmem.from_host(ctx, ranges.tobytes()), devmem.empty(ctx, 4 * len(ranges)), devmem.empty(ctx, 4 * len(ranges))
    d_out = devmem.empty(ctx, 8192).zero_()
    ctx.bgzf_stats()
    code, total = ctx.bgzf_read_lines_dev(d_in.ptr, len(blob), d_m.ptr, n, d_r.ptr, len(ranges), 10, d_scratch.ptr, cap, d_out.ptr, 100, d_len.ptr,
                                          d_st.ptr, d_rs.ptr)
    a = tab[28][1] + int(np.nonzero(arr[tab[28][1]:tab[29][1]] == 10)[0][0]) + 1
    want = data[:tab[2][1]] + data[a:tab[30][1]]
    assert code == _lib.BUF_ERROR and total == len(want) and d_out.cpu().tobytes() == bytes(8192)
    code, total = ctx.bgzf_read_lines_dev(d_in.ptr, len(blob), d_m.ptr, n, d_r.ptr, len(ranges), 10, d_scratch.ptr, cap, d_out.ptr, 8192, d_len.ptr,
                                          d_st.ptr, d_rs.ptr)
    assert code == 0 and total == len(want)
    assert ctx.bgzf_stats() == (2, 2 * n, len(ranges))
    assert d_rs.cpu(np.int32).tolist() == [OK, OK, TABLE, OK, RANK]
    assert d_len.cpu(np.uint32).tolist() == [tab[2][1], tab[30][1] - a, 0, 0, 0]
    assert d_out.cpu().tobytes()[:total] == want and d_out.cpu().tobytes()[total:] == bytes(8192 - total)

"""bgzf.LineIndex without a GPU: the on-disk format there and back, everything from_bytes() must refuse, and locate() against a
brute-force model on synthetic block tables (empty blocks in the middle, delimiters that end a block, a last line without one)."""
import io
import random
import struct

import numpy as np
import pytest

HEAD = struct.Struct("<8sIIQQQQQ")
ROW = struct.Struct("<QQQII")


def synthetic(rng, nblocks, delim=b"\n", end_with_delim=None, p_empty=0.2, p_delim=0.2):
    """-> (blocks as from_counts takes them with the EOF block, the block's data, all data)"""
    datas = []
    for _ in range(nblocks):
        if rng.random() < p_empty:
            datas.append(b"")
            continue
        n = rng.choice([1, 2, 3, 7, 40])
        datas.append(bytes(delim[0] if rng.random() < p_delim else rng.choice(b"ab\x01\x00") for _ in range(n)))
    if end_with_delim is not None and any(datas):
        last = max(i for i, d in enumerate(datas) if d)
        datas[last] = datas[last][:-1] + (delim if end_with_delim else b"z")
    blocks, c = [], 0
    for d in datas + [b""]:
        size = 28 + len(d)
        blocks.append((c, size, len(d), d.count(delim), d.endswith(delim)))
        c += size
    return blocks, datas, b"".join(datas)


def model_locate(datas, data, delim, line):
    """where line `line` starts, found by walking the bytes"""
    starts = [0] + [i + 1 for i, ch in enumerate(data) if ch == delim[0]]
    if starts[-1] == len(data):
        starts.pop()                                    # (no line starts behind a last delimiter)
    nlines = len(starts)
    if line == nlines:
        off = len(data)
    else:
        off = starts[line]
    u = 0
    for b, d in enumerate(datas):
        if d and u <= off < u + len(d):
            rank = d[:off - u].count(delim)
            assert rank > 0 or off == u
            return nlines, (b, rank)
        u += len(d)
    assert off == len(data)
    return nlines, (len(datas), 0)


def test_locate_against_the_model():
    from zlib_ng_amd import bgzf
    rng = random.Random(5)
    seen_step = seen_open_end = seen_empty = 0
    for trial in range(300):
        delim = rng.choice([b"\n", b"\x00"])
        blocks, datas, data = synthetic(rng, rng.randrange(0, 12), delim, rng.choice([None, True, False]))
        idx = bgzf.LineIndex.from_counts(blocks, delim)
        assert len(idx) == len(datas) and idx.delimiter == delim and idx.usize == len(data) and idx.delimiters == data.count(delim)
        parts = data.split(delim)
        assert idx.lines == len(parts) - 1 + (1 if parts[-1] else 0)
        assert [(c, u) for c, u, _, _ in idx.blocks] == [(b[0], sum(len(d) for d in datas[:i])) for i, b in enumerate(blocks[:-1])]
        for line in range(idx.lines + 1):
            nlines, want = model_locate(datas, data, delim, line)
            assert nlines == idx.lines
            assert idx.locate(line) == want, (trial, line, datas)
            b, r = want
            seen_step += r == 0 and line > 0 and b < len(datas)
            seen_empty += b > 0 and b < len(datas) and r == 0 and datas[b - 1] == b""
        seen_open_end += bool(data) and not data.endswith(delim)
        for beyond in (idx.lines + 1, idx.lines + 1000):
            with pytest.raises(IndexError):
                idx.locate(beyond)
        with pytest.raises(ValueError):
            idx.locate(-1)
    assert seen_step > 50 and seen_open_end > 50 and seen_empty > 20          # the cases the model is there for did occur


def test_hand_made_table():
    from zlib_ng_amd import bgzf
    # 10 bytes with 2 delimiters | an empty block | 5 bytes ending in a delimiter | 3 bytes without one | EOF
    idx = bgzf.LineIndex.from_counts([(0, 100, 10, 2, False), (100, 28, 0, 0, False), (128, 50, 5, 1, True), (178, 60, 3, 0, False),
                                      (238, 28, 0, 0, False)])
    assert len(idx) == 4 and idx.lines == 4 and idx.file_size == 266 and idx.cend == 238 and idx.usize == 18 and idx.delimiters == 3
    assert idx.blocks == [(0, 0, 0, False), (100, 10, 2, False), (128, 10, 2, True), (178, 15, 3, False)]
    assert [idx.locate(i) for i in range(5)] == [(0, 0), (0, 1), (0, 2), (3, 0), (4, 0)]
    empty = bgzf.LineIndex.from_counts([(0, 28, 0, 0, False)])
    assert len(empty) == 0 and empty.lines == 0 and empty.locate(0) == (0, 0) and empty.file_size == 28
    with pytest.raises(IndexError):
        empty.locate(1)
    one = bgzf.LineIndex.from_counts([(0, 30, 1, 1, True), (30, 28, 0, 0, False)])
    assert one.lines == 1 and one.locate(0) == (0, 0) and one.locate(1) == (1, 0)


def test_format_round_trip(tmp_path):
    from zlib_ng_amd import bgzf
    rng = random.Random(9)
    for trial in range(40):
        delim = bytes([rng.randrange(256)])
        blocks, datas, data = synthetic(rng, rng.randrange(0, 30), delim)
        idx = bgzf.LineIndex.from_counts(blocks, delim)
        blob = idx.to_bytes()
        assert len(blob) == HEAD.size + ROW.size * len(idx) and blob[:8] == bgzf.LINE_INDEX_MAGIC
        head = HEAD.unpack_from(blob)
        assert head[1:] == (delim[0], 0, len(idx), idx.file_size, idx.cend, idx.usize, idx.delimiters)
        rows = list(ROW.iter_unpack(blob[HEAD.size:]))
        assert rows == [(c, u, b, int(f), 0) for c, u, b, f in idx.blocks]
        back = bgzf.LineIndex.from_bytes(blob, idx.file_size)
        assert back == idx and back.lines == idx.lines and back.delimiter == delim and not (back != idx)
        path = tmp_path / f"t{trial}.lidx"
        idx.save(path)
        assert bgzf.LineIndex.load(path) == idx
        f = io.BytesIO()
        idx.save(f)
        f.seek(0)
        assert bgzf.LineIndex.load(f, idx.file_size) == idx
    other = bgzf.LineIndex.from_counts(synthetic(rng, 5)[0], b"\n")
    assert other != bgzf.LineIndex.from_counts(synthetic(rng, 6)[0], b"\n") and other != "x"
    with pytest.raises(ValueError):
        bgzf.LineIndex.from_counts([(0, 28, 0, 0, False)], b"ab")


def pack(rows, delim=10, n=None, fsize=None, cend=None, usize=None, total=None, magic=b"ZNGLIDX\x01", zero=0):
    """an index file from (coffset, uoffset, before, flags[, reserved]) rows; the totals default to ones that fit blocks of 100 bytes"""
    cend = (rows[-1][0] + 100 if rows else 0) if cend is None else cend
    head = HEAD.pack(magic, delim, zero, len(rows) if n is None else n, cend + 28 if fsize is None else fsize, cend,
                     (rows[-1][1] + 10 if rows else 0) if usize is None else usize, (rows[-1][2] + 1 if rows else 0) if total is None else total)
    return head + b"".join(ROW.pack(*(tuple(r) + (0,))[:5]) for r in rows)


def test_from_bytes_rejections():
    from zlib_ng_amd import bgzf
    good = [(0, 0, 0, 0), (100, 10, 1, 1), (200, 20, 2, 0), (300, 20, 2, 0)]
    idx = bgzf.LineIndex.from_bytes(pack(good))
    assert len(idx) == 4 and idx.lines == 4 and idx.file_size == 428
    assert bgzf.LineIndex.from_bytes(pack(good), 428) == idx
    blob = pack(good)
    bad = {
        "truncated header": blob[:40],
        "truncated rows": blob[:-1],
        "a row too many": blob + b"\0" * 32,
        "count and length disagree": pack(good, n=3),
        "huge count": pack(good, n=1 << 60),
        "wrong magic": pack(good, magic=b"ZNGLIDY\x01"),
        "another version": pack(good, magic=b"ZNGLIDX\x02"),
        "gzi file": struct.pack("<Q", 1) + struct.pack("<QQ", 100, 10),
        "delimiter above a byte": pack(good, delim=256),
        "reserved header field": pack(good, zero=1),
        "compressed offsets do not ascend": pack([(0, 0, 0, 0), (200, 10, 1, 0), (100, 20, 2, 0), (300, 20, 2, 0)]),
        "compressed offsets repeat": pack([(0, 0, 0, 0), (100, 10, 1, 0), (100, 20, 2, 0)]),
        "blocks overlap": pack([(0, 0, 0, 0), (20, 10, 1, 0)]),
        "a block of more than 64 KiB": pack([(0, 0, 0, 0), (70000, 10, 1, 0)]),
        "first block not at 0": pack([(28, 0, 0, 0), (100, 10, 1, 0)]),
        "uncompressed offsets descend": pack([(0, 0, 0, 0), (100, 20, 1, 0), (200, 10, 2, 0)]),
        "uncompressed offsets jump": pack([(0, 0, 0, 0), (100, 70000, 1, 0)]),
        "first uoffset not 0": pack([(0, 5, 0, 0), (100, 10, 1, 0)]),
        "counts descend": pack([(0, 0, 0, 0), (100, 10, 5, 0), (200, 20, 4, 0)], total=6),
        "first count not 0": pack([(0, 0, 1, 0), (100, 10, 2, 0)]),
        "more delimiters than bytes": pack([(0, 0, 0, 0), (100, 10, 11, 0)]),
        "total below the last row": pack(good, total=1),
        "data ends before the last block": pack(good, usize=10),
        "blocks end behind the file": pack(good, cend=400, fsize=399),
        "blocks end before the last block": pack(good, cend=250),
        "unknown flag": pack([(0, 0, 0, 2), (100, 10, 1, 0)]),
        "reserved row field": pack([(0, 0, 0, 0, 7), (100, 10, 1, 0)]),
        "flag on a block without a delimiter": pack([(0, 0, 0, 1), (100, 10, 0, 0)], total=0),
    }
    for name, b in bad.items():
        with pytest.raises(ValueError):
            bgzf.LineIndex.from_bytes(b)
            pytest.fail(f"accepted: {name}")
    for size in (427, 429, 0):
        with pytest.raises(ValueError, match="428"):
            bgzf.LineIndex.from_bytes(blob, size)
        with pytest.raises(ValueError):
            idx.validate(size)
    idx.validate(428)
    idx.validate()


def test_numpy_views_are_not_shared():
    """an index loaded from a blob does not change when the blob's buffer does"""
    from zlib_ng_amd import bgzf
    blob = bytearray(pack([(0, 0, 0, 0), (100, 10, 1, 0)]))
    idx = bgzf.LineIndex.from_bytes(blob)
    want = idx.blocks
    blob[HEAD.size:] = b"\xff" * (len(blob) - HEAD.size)
    assert idx.blocks == want and isinstance(idx._rows, np.ndarray)


def test_member_table_checks_blocks_against_the_index():
    """the host check in front of every engine call by line: a block must be where the index says, of that size (BSIZE) and ISIZE"""
    import zlib
    from zlib_ng_amd import bgzf

    def block(data, extra=b""):
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        pay = co.compress(data) + co.flush()
        size = 12 + len(extra) + 6 + len(pay) + 8
        return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(extra) + 6) + extra + b"BC\x02\0" + struct.pack("<H", size - 1) + pay +
                struct.pack("<II", zlib.crc32(data), len(data)))

    datas = [b"first block\n" * 9, b"", b"second\n", b"third, behind another subfield\n"]
    blocks = [block(datas[0]), block(datas[1]), block(datas[2]), block(datas[3], b"XY\x03\0abc")]
    raw = b"".join(blocks)
    starts = np.cumsum([0] + [len(b) for b in blocks[:-1]])
    csizes, isizes = np.array([len(b) for b in blocks]), np.array([len(d) for d in datas])
    buf = np.frombuffer(raw, np.uint8)
    members, bad = bgzf._member_table(buf, starts, csizes, isizes)
    assert bad == -1
    assert members["in_off"].tolist() == [int(s) + 18 for s in starts[:3]] + [int(starts[3]) + 25]
    assert members["in_len"].tolist() == [len(b) - 26 for b in blocks[:3]] + [len(blocks[3]) - 33]
    assert members["out_off"].tolist() == [0, len(datas[0]), len(datas[0]), len(datas[0]) + len(datas[2])]
    assert members["out_len"].tolist() == isizes.tolist() and members["crc"].tolist() == [zlib.crc32(d) for d in datas]
    for row in range(4):
        for what, where, value in (("BSIZE", 16 if row < 3 else 23, None), ("ISIZE", len(blocks[row]) - 4, None), ("magic", 1, 0x8c),
                                   ("no FEXTRA", 3, 0), ("subfield id", 12 if row < 3 else 19, ord("X")), ("XLEN", 11, 0xff)):
            hurt = bytearray(raw)
            at = int(starts[row]) + where
            hurt[at] = hurt[at] ^ 1 if value is None else value
            assert bgzf._member_table(np.frombuffer(bytes(hurt), np.uint8), starts, csizes, isizes)[1] == row, (row, what)
    assert bgzf._member_table(buf, starts + 1, csizes, isizes)[1] == 0                       # not where the index says
    assert bgzf._member_table(buf[:-1], starts, csizes, isizes)[1] == 3                      # the last block does not fit
    assert bgzf._member_table(buf, starts, csizes - np.array([0, 0, 1, 0]), isizes)[1] == 2
    assert bgzf._member_table(buf[:10], starts[:1], csizes[:1], isizes[:1])[1] == 0
    assert bgzf._member_table(buf, starts[:0], csizes[:0], isizes[:0])[1] == -1

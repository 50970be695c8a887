"""BGZF without a GPU: virtual offsets, the host scan (zngamd_bgzf_scan) on the golden files and on damaged ones, the .gzi index
format, and the compressed size of 65 280-byte blocks through the oracle against zlib at the same level (the project's 2 % gate on
the held-out corpora, here with BGZF's block size, no history and final blocks)."""
import gzip
import os
import struct
import zlib

import pytest

from conftest import GOLDEN

BGZIP = os.path.join(GOLDEN, "test.fastq.bgzip.gz")
PLAIN = os.path.join(GOLDEN, "test.fastq.gz")
EOF_HEX = "1f8b08040000000000ff0600424302001b0003000000000000000000"


def _block(payload, data, bsize=None):
    """a BGZF block around a raw deflate payload"""
    size = 18 + len(payload) + 8
    return (bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", "")) + struct.pack("<H", (size if bsize is None else bsize) - 1) + payload +
            struct.pack("<II", zlib.crc32(data), len(data)))


def _deflate(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(data) + co.flush()


def test_virtual_offsets_round_trip_at_the_bounds_and_refuse_the_rest():
    from zlib_ng_amd import bgzf
    for c, u in ((0, 0), (0, 65535), ((1 << 48) - 1, 0), ((1 << 48) - 1, 65535), (1556511, 17)):
        v = bgzf.make_virtual_offset(c, u)
        assert v == c << 16 | u and bgzf.split_virtual_offset(v) == (c, u)
    assert bgzf.make_virtual_offset((1 << 48) - 1, 65535) == (1 << 64) - 1
    for c, u in ((-1, 0), (1 << 48, 0), (0, -1), (0, 65536)):
        with pytest.raises(ValueError):
            bgzf.make_virtual_offset(c, u)
    for v in (-1, 1 << 64):
        with pytest.raises(ValueError):
            bgzf.split_virtual_offset(v)


def test_eof_block_is_the_specified_one():
    from zlib_ng_amd import bgzf
    assert bgzf.EOF_BLOCK.hex() == EOF_HEX and len(bgzf.EOF_BLOCK) == 28
    assert gzip.decompress(bgzf.EOF_BLOCK) == b""


def test_scan_of_the_golden_bgzip_file():
    from zlib_ng_amd import _lib
    raw = open(BGZIP, "rb").read()
    assert len(raw) == 1556539
    code, blocks, used, total = _lib.bgzf_scan(raw)
    assert code == _lib.OK and used == len(raw)
    # the blocks tile the file
    pos = upos = 0
    for c, u, cs, isz in blocks:
        assert (c, u) == (pos, upos) and 28 <= cs <= 65536 and isz <= 65536
        assert raw[c:c + 4] == b"\x1f\x8b\x08\x04" and struct.unpack_from("<H", raw, c + 16)[0] == cs - 1
        pos, upos = pos + cs, upos + isz
    assert pos == len(raw)
    assert raw[blocks[-1][0]:].hex() == EOF_HEX and blocks[-1][2:] == (28, 0)
    assert total == upos == len(gzip.decompress(raw))
    # counting only, and a table that fills up
    assert _lib.load().zngamd_bgzf_scan is not None
    code, first, used3, total3 = _lib.bgzf_scan(raw, 3)
    assert code == _lib.OK and first == blocks[:3] and used3 == blocks[3][0] and total3 == blocks[3][1]


def test_scan_says_not_bgzf_for_an_ordinary_gzip_file():
    from zlib_ng_amd import _lib, bgzf
    raw = open(PLAIN, "rb").read()
    code, blocks, used, total = _lib.bgzf_scan(raw)
    assert code == _lib.E_BGZF and code != _lib.DATA_ERROR and blocks == [] and used == 0 and total == 0
    assert _lib.bgzf_scan(b"not gzip at all, just text")[0] == _lib.E_BGZF
    assert _lib.bgzf_scan(gzip.compress(b"a member without the subfield"))[0] == _lib.E_BGZF
    with pytest.raises(bgzf.BadGzipFile):
        bgzf.GziIndex.build(PLAIN)
    assert _lib.bgzf_scan(b"") == (_lib.OK, [], 0, 0)


def test_scan_of_a_truncated_file_gives_the_complete_blocks_and_the_tail():
    from zlib_ng_amd import _lib
    raw = open(BGZIP, "rb").read()
    _, blocks, _, _ = _lib.bgzf_scan(raw)
    k = len(blocks) // 2
    for cut in (blocks[k][0] + 1, blocks[k][0] + 11, blocks[k][0] + 17, blocks[k][0] + 18, blocks[k][0] + blocks[k][2] - 1):
        code, got, used, total = _lib.bgzf_scan(raw[:cut])
        assert code == _lib.OK and got == blocks[:k] and used == blocks[k][0] and total == blocks[k][1], cut
    code, got, used, total = _lib.bgzf_scan(raw[:blocks[k][0]])
    assert code == _lib.OK and got == blocks[:k] and used == blocks[k][0]


def test_scan_refuses_a_hostile_bsize():
    from zlib_ng_amd import _lib
    data = b"hello, blocked gzip " * 40
    pay = _deflate(data)
    good = _block(pay, data)
    assert _lib.bgzf_scan(good + bytes.fromhex(EOF_HEX))[:1] == (_lib.OK,) and gzip.decompress(good) == data
    # smaller than header plus trailer
    for bs in (1, 18, 25):
        code, blocks, used, _ = _lib.bgzf_scan(_block(pay, data, bsize=bs) + good)
        assert code == _lib.DATA_ERROR and blocks == [] and used == 0, bs
    # past the end of the buffer, with nothing in front to vouch for it
    code, blocks, used, _ = _lib.bgzf_scan(_block(pay, data, bsize=len(good) + 1))
    assert code == _lib.DATA_ERROR and blocks == []
    code, blocks, used, _ = _lib.bgzf_scan(_block(pay, data, bsize=65536))
    assert code == _lib.DATA_ERROR and blocks == []
    # pointed into the middle of the block: what follows is no header
    code, blocks, used, _ = _lib.bgzf_scan(good + _block(pay, data, bsize=len(good) - 7) + good)
    assert code == _lib.DATA_ERROR and 1 <= len(blocks) <= 2 and blocks[0] == (0, 0, len(good), len(data)) and used in (len(good), 2 * len(good) - 7)
    # an ISIZE no block can have
    bad = bytearray(good)
    bad[-4:] = struct.pack("<I", 65537)
    assert _lib.bgzf_scan(bytes(bad))[0] == _lib.DATA_ERROR
    # a subfield that overruns the extra field
    bad = bytearray(good)
    bad[14:16] = struct.pack("<H", 9)
    assert _lib.bgzf_scan(bytes(bad))[0] == _lib.DATA_ERROR


def test_gzi_index_build_save_load(tmp_path):
    from zlib_ng_amd import _lib, bgzf
    idx = bgzf.GziIndex.build(BGZIP)
    _, blocks, _, total = _lib.bgzf_scan(open(BGZIP, "rb").read())
    assert idx.entries == [(b[0], b[1]) for b in blocks[1:-1]] and len(idx) == len(blocks) - 2
    p = tmp_path / "x.gzi"
    idx.save(p)
    back = bgzf.GziIndex.load(p, file_size=os.path.getsize(BGZIP))
    assert back == idx and back.entries == idx.entries
    with open(BGZIP, "rb") as f:
        assert bgzf.GziIndex.build(f) == idx
    # offsets -> virtual offsets
    assert idx.voffset(0) == 0 and idx.voffset(blocks[1][1] - 1) == blocks[1][1] - 1
    for b in blocks[1:-1]:
        assert idx.voffset(b[1]) == b[0] << 16 and idx.voffset(b[1] + b[3] - 1) == b[0] << 16 | (b[3] - 1)
    assert idx.locate(total - 1) == (blocks[-2][0], blocks[-2][3] - 1)


def test_gzi_bytes_of_a_hand_built_table():
    from zlib_ng_amd import bgzf
    blocks = [(0, 0, 1000, 65280), (1000, 65280, 2000, 65280), (3000, 130560, 500, 17), (3500, 130577, 28, 0)]
    idx = bgzf.GziIndex.from_blocks(blocks)
    want = struct.pack("<Q", 2) + struct.pack("<QQ", 1000, 65280) + struct.pack("<QQ", 3000, 130560)
    assert idx.to_bytes() == want and want.hex() == "0200000000000000" "e803000000000000" "00ff000000000000" "b80b000000000000" "00fe010000000000"
    assert bgzf.GziIndex.from_bytes(want, file_size=3528) == idx
    # a trailing entry that points at the EOF block is accepted; save() writes none
    with_eof = struct.pack("<Q", 3) + want[8:] + struct.pack("<QQ", 3500, 130577)
    got = bgzf.GziIndex.from_bytes(with_eof, file_size=3528)
    assert got.entries[:2] == idx.entries and got.entries[2] == (3500, 130577) and got.voffset(130560 + 16) == 3000 << 16 | 16
    assert bgzf.GziIndex.from_blocks(blocks[:3]).to_bytes() == want        # (no EOF block in the table: the same index)
    assert bgzf.GziIndex.from_blocks([]).to_bytes() == bytes(8) and bgzf.GziIndex.from_blocks(blocks[:1]).to_bytes() == bytes(8)


def test_gzi_refuses_tables_that_could_misdirect_a_read():
    from zlib_ng_amd import bgzf
    pair = lambda *e: struct.pack("<Q", len(e)) + b"".join(struct.pack("<QQ", c, u) for c, u in e)
    for blob in (pair((3000, 130560), (1000, 65280)),               # compressed offsets fall
                 pair((1000, 65280), (1000, 130560)),               # ... or stand still
                 pair((1000, 65280), (3000, 65279)),                # uncompressed offsets fall
                 pair((0, 0)),                                      # the first block has no entry
                 pair((1 << 48, 5))):
        with pytest.raises(ValueError):
            bgzf.GziIndex.from_bytes(blob)
    ok = pair((1000, 65280), (3000, 130560))
    bgzf.GziIndex.from_bytes(ok)
    for size in (3000, 3027):                                       # beyond the file, or no room for a block behind the offset
        with pytest.raises(ValueError):
            bgzf.GziIndex.from_bytes(ok, file_size=size)
    bgzf.GziIndex.from_bytes(ok, file_size=3028)
    for blob in (b"", ok[:-1], ok + b"\0", struct.pack("<Q", 1 << 60) + ok[8:]):
        with pytest.raises(ValueError):
            bgzf.GziIndex.from_bytes(blob)
    with pytest.raises(ValueError):
        bgzf.GziIndex.from_bytes(ok).validate(file_size=100)


# ---- ratio of BGZF-sized blocks on the oracle (the bars were set against zlib 1.2.x: skipped elsewhere, as the existing gate is)
BLOCK = 65280
TOL = 1.02
zlib_1_2 = pytest.mark.skipif(not zlib.ZLIB_RUNTIME_VERSION.startswith("1.2."),
                              reason="ratio bars were set against zlib 1.2.x, this box has " + zlib.ZLIB_RUNTIME_VERSION)


@zlib_1_2
@pytest.mark.parametrize("level", [1, 6, 9])
def test_bgzf_blocks_within_two_percent_of_zlib_at_the_same_level(level):
    from conftest import heldout_corpora
    from oracle import oracle as O
    corpora = heldout_corpora()
    assert len(corpora) == 4
    for name, data in corpora.items():
        ours = ref = 0
        for off in range(0, len(data), BLOCK):
            blk = data[off:off + BLOCK]
            c, crc = O.deflate_unit(blk, b"", level, 1)
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            ref += len(co.compress(blk) + co.flush())
            ours += len(c)
            assert len(c) <= 65510 and crc == zlib.crc32(blk)
            if off % (7 * BLOCK) == 0:
                assert zlib.decompress(c, -15) == blk
        print(f"{name} level {level}: {ours} against zlib's {ref}: {ours / ref:.4f}")
        assert ours <= TOL * ref, f"{name} level {level}: {ours} against zlib's {ref} ({ours / ref:.4f})"

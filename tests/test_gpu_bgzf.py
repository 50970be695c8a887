"""BGZF on the GPU (zlib_ng_amd/bgzf.py, csrc/za_bgzf.hip): the writer byte for byte against the oracle's payloads and the format's
framing, the system gzip and the host scan as referees, the file objects against a model of the block cuts, seeks by virtual offset
and ranged reads against slices of the reference bytes, and damaged files."""
import gzip
import io
import os
import random
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BLOCK = 65280
MAX_PAYLOAD = 65510
HEADER = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZIP = os.path.join(GOLDEN, "test.fastq.bgzip.gz")


def stored(block):
    return b"\x01" + struct.pack("<HH", len(block), len(block) ^ 0xFFFF) + block


def check_stream(O, data, stream, table, level, eof, block_size=BLOCK):
    """every block of `stream` is the specified frame around the oracle's payload; the table says where they lie"""
    cuts = [data[o:o + block_size] for o in range(0, len(data), block_size)]
    assert len(table) == len(cuts) + (1 if eof else 0)
    pos = upos = 0
    for blk, row in zip(cuts, table):
        exp, ecrc = O.deflate_unit(blk, b"", level, 1)
        if len(exp) > MAX_PAYLOAD:
            exp = stored(blk)
        size = 18 + len(exp) + 8
        assert row == (pos, upos, size, len(blk))
        got = stream[pos:pos + size]
        assert got[:16] == HEADER and struct.unpack_from("<H", got, 16)[0] == size - 1 and size <= 65536
        assert got[18:-8] == exp, f"payload of the block at {pos} differs from the oracle's (level {level})"
        assert struct.unpack_from("<II", got, size - 8) == (zlib.crc32(blk), len(blk)) and ecrc == zlib.crc32(blk)
        pos, upos = pos + size, upos + len(blk)
    if eof:
        assert stream[pos:] == EOF_BLOCK and table[-1] == (pos, upos, 28, 0)
    else:
        assert pos == len(stream)
        assert not stream.endswith(EOF_BLOCK)


@pytest.fixture(scope="module")
def inputs(fastq):
    from conftest import heldout_corpora
    from zlib_ng_amd import corpus
    d = {"empty": b"", "one": b"x", "block-1": corpus.text(BLOCK - 1, 4).tobytes(), "block": corpus.text(BLOCK, 5).tobytes(),
         "block+1": corpus.text(BLOCK + 1, 6).tobytes(), "three+17": corpus.text(3 * BLOCK + 17, 7).tobytes(), "fastq": fastq,
         "urandom": os.urandom(2 * BLOCK + 1000)}
    d.update(heldout_corpora())
    return d


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_writer_matches_the_oracle_block_for_block(ctx, inputs, level):
    from oracle import oracle as O
    for name, data in inputs.items():
        for eof in (True, False):
            stream, table = ctx.bgzf_compress(data, BLOCK, level, eof)
            check_stream(O, data, stream, table, level, eof)
            if name in ("empty", "one", "three+17"):
                assert gzip.decompress(stream) == data
    assert ctx.bgzf_compress(b"", BLOCK, level, True) == (EOF_BLOCK, [(0, 0, 28, 0)])
    assert ctx.bgzf_compress(b"", BLOCK, level, False) == (b"", [])


def test_small_blocks_and_the_default_level(ctx, inputs):
    from oracle import oracle as O
    from zlib_ng_amd import bgzf
    data = inputs["three+17"]
    for bs in (1, 1000, 4096, 65279):
        piece = data[:40] if bs == 1 else data
        stream, table = ctx.bgzf_compress(piece, bs, -1, True)
        check_stream(O, piece, stream, table, 6, True, bs)
        assert gzip.decompress(stream) == piece
    for bad in (0, 65281, 1 << 20):
        with pytest.raises(ValueError):
            bgzf.compress(data, block_size=bad)
    with pytest.raises(Exception):
        bgzf.compress(data, 10)


def test_referees(ctx, inputs):
    from zlib_ng_amd import _lib, bgzf, gzip_ng
    for name in ("empty", "one", "three+17", "fastq", "urandom", "python_sources"):
        x = inputs[name]
        blob = bgzf.compress(x)
        assert gzip.decompress(blob) == x and bgzf.decompress(blob) == x
        stream, table = ctx.bgzf_compress(x, BLOCK, 6, True)
        assert stream == blob
        assert _lib.bgzf_scan(blob) == (_lib.OK, table, len(blob), len(x))
    blob = bgzf.compress(inputs["fastq"])
    ctx.decode_paths()
    assert gzip_ng.decompress(blob) == inputs["fastq"]
    assert ctx.decode_paths()["bgzf"] >= len(inputs["fastq"]) // BLOCK
    with pytest.raises(bgzf.BadGzipFile):
        bgzf.decompress(gzip.compress(b"an ordinary member"))
    with pytest.raises(bgzf.BadGzipFile):
        bgzf.decompress(blob[:-40])


def test_device_resident_writer(ctx, inputs):
    from zlib_ng_amd import bgzf, devmem
    x = inputs["fastq"]
    d_in = devmem.from_host(ctx, x)
    out, n, tab = bgzf.compress_dev(ctx, d_in, len(x), 6)
    blob = out[:n].cpu().tobytes()
    assert blob == bgzf.compress(x)
    stream, table = ctx.bgzf_compress(x, BLOCK, 6, True)
    assert [tuple(int(v) for v in r) for r in tab] == table
    out2, n2, tab2 = bgzf.compress_dev(ctx, d_in, len(x), 6, out=out, table=False, eof=False)
    assert out2 is out and tab2 is None and out[:n2].cpu().tobytes() == blob[:-28]
    # a destination that is too small: the size needed, nothing written
    small = devmem.empty(ctx, 1000)
    with pytest.raises(_lib_error()) as e:
        bgzf.compress_dev(ctx, d_in, len(x), 6, out=small)
    assert e.value.code == -5


def _lib_error():
    from zlib_ng_amd import _lib
    return _lib.EngineError


@pytest.mark.skipif(not zlib.ZLIB_RUNTIME_VERSION.startswith("1.2."), reason="ratio bars were set against zlib 1.2.x, this box has " + zlib.ZLIB_RUNTIME_VERSION)
@pytest.mark.parametrize("level", [1, 6, 9])
def test_heldout_ratio_gate_through_the_hip_path(ctx, level):
    from conftest import heldout_corpora
    for name, data in heldout_corpora().items():
        stream, table = ctx.bgzf_compress(data, BLOCK, level, False)
        ours = sum(cs - 26 for _, _, cs, _ in table)
        ref = 0
        for off in range(0, len(data), BLOCK):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            ref += len(co.compress(data[off:off + BLOCK]) + co.flush())
        print(f"{name} level {level}: {ours} against zlib's {ref}: {ours / ref:.4f}")
        assert ours <= 1.02 * ref, f"{name} level {level}: {ours} against zlib's {ref} ({ours / ref:.4f})"


# ---- the file objects
@pytest.mark.parametrize("block_size,batch", [(BLOCK, None), (1000, 4500), (BLOCK, 3 * BLOCK)])
def test_writer_against_a_model_of_the_block_cuts(tmp_path, monkeypatch, block_size, batch):
    from zlib_ng_amd import _lib, bgzf
    if batch:
        monkeypatch.setattr(bgzf, "_WRITE_BATCH", batch)
    rng = random.Random(block_size + (batch or 0))
    src = np.random.default_rng(3).integers(65, 91, 6 << 20, dtype=np.uint8).tobytes()
    path = str(tmp_path / "w.bgzf")
    model, pending, written, marks = [], 0, 0, []
    with bgzf.open(path, "wb", block_size=block_size) as w:
        for step in range(80):
            n = rng.choice([0, 1, 17, block_size - 1, block_size, block_size + 1, rng.randrange(1, 4 * block_size), rng.randrange(1, 300)])
            n = min(n, len(src) - written)
            w.write(src[written:written + n])
            written += n
            pending += n
            op = rng.random()
            if op < 0.25:
                w.flush()
                model += [block_size] * (pending // block_size) + ([pending % block_size] if pending % block_size else [])
                pending = 0
                v = w.tell()
                assert v & 0xFFFF == 0
                marks.append((v, written))
            elif op < 0.6:
                before = len(w.blocks)
                v = w.tell()
                model += [block_size] * (pending // block_size)
                pending %= block_size
                assert v & 0xFFFF == pending and len(w.blocks) >= before
                marks.append((v, written))
            assert w.utell() == written
    model += [block_size] * (pending // block_size) + ([pending % block_size] if pending % block_size else [])
    assert [b[3] for b in w.blocks] == model + [0]
    raw = open(path, "rb").read()
    data = src[:written]
    assert gzip.decompress(raw) == data and raw.endswith(EOF_BLOCK)
    assert _lib.bgzf_scan(raw) == (_lib.OK, w.blocks, len(raw), written)
    # what tell() said is what seek() needs
    with bgzf.open(path) as r:
        for v, at in marks:
            assert r.seek(v) == v
            assert r.read(300) == data[at:at + 300], (v >> 16, v & 0xFFFF, at)
            if at + 300 <= written:
                assert r.tell() >> 16 >= v >> 16
    gzi = str(tmp_path / "w.gzi")
    w.write_gzi(gzi)
    assert open(gzi, "rb").read() == bgzf.GziIndex.build(path).to_bytes()


def test_append_mode_and_text_mode(tmp_path, inputs):
    from zlib_ng_amd import _lib, bgzf
    path = str(tmp_path / "a.bgzf")
    a, b = inputs["three+17"], inputs["block+1"]
    with bgzf.open(path, "wb", compresslevel=1) as w:
        w.write(a)
    with bgzf.open(path, "ab") as w:
        v = w.tell()
        w.write(b)
    raw = open(path, "rb").read()
    assert gzip.decompress(raw) == a + b and raw.endswith(EOF_BLOCK)
    code, blocks, used, total = _lib.bgzf_scan(raw)
    assert (code, used, total) == (_lib.OK, len(raw), len(a + b)) and blocks == w.blocks
    gzi = io.BytesIO()
    w.write_gzi(gzi)
    assert gzi.getvalue() == bgzf.GziIndex.build(path).to_bytes()
    with bgzf.open(path) as r:
        r.seek(v)
        assert r.read() == b
    tpath = str(tmp_path / "t.bgzf")
    with bgzf.open(tpath, "wt", encoding="utf-8") as w:
        w.write("zeile eins\nzeile zwei ä\n")
    with bgzf.open(tpath, "rt", encoding="utf-8") as r:
        assert r.readlines() == ["zeile eins\n", "zeile zwei ä\n"]
    assert gzip.open(tpath, "rt", encoding="utf-8").read() == "zeile eins\nzeile zwei ä\n"
    with pytest.raises(ValueError):
        bgzf.open(path, "rb", encoding="utf-8")


@pytest.fixture(scope="module")
def golden():
    raw = open(BGZIP, "rb").read()
    return raw, gzip.decompress(raw)


def test_reader_sequential(golden, monkeypatch):
    from zlib_ng_amd import bgzf
    raw, ref = golden
    with bgzf.open(BGZIP) as r:
        assert r.read() == ref and r.read() == b"" and r.utell() == len(ref)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 100000)        # windows that end inside blocks
    with bgzf.BgzfReader(io.BytesIO(raw), require_eof=True) as r:
        got, buf = [], bytearray(70001)
        while True:
            n = r.readinto(buf)
            if not n:
                break
            got.append(bytes(buf[:n]))
        assert b"".join(got) == ref
    with bgzf.open(BGZIP) as r:
        assert r.read(10) == ref[:10] and r.tell() == 10 and r.read(100000) == ref[10:100010] and r.utell() == 100010


def test_reader_seeks_by_virtual_offset(golden):
    from zlib_ng_amd import _lib, bgzf
    raw, ref = golden
    _, blocks, _, _ = _lib.bgzf_scan(raw)
    rng = random.Random(9)
    with bgzf.open(BGZIP) as r:
        for c, u, cs, isz in blocks:
            r.seek(c << 16)
            assert r.read(64) == ref[u:u + 64]
        for _ in range(100):
            c, u, cs, isz = rng.choice(blocks[:-1])
            w = rng.randrange(isz)
            n = rng.choice([1, 100, 70000])
            assert r.seek(bgzf.make_virtual_offset(c, w)) == c << 16 | w
            assert r.tell() == c << 16 | w
            assert r.read(n) == ref[u + w:u + w + n]
        idx = bgzf.GziIndex.build(BGZIP)
        for off in [0, 1, 65279, 65280, len(ref) - 1, len(ref)] + [rng.randrange(len(ref)) for _ in range(30)]:
            assert r.useek(off, idx) == off and r.utell() == off
            assert r.read(500) == ref[off:off + 500] and r.utell() == min(len(ref), off + 500)
        r.seek(blocks[3][0] << 16)
        with pytest.raises(ValueError):
            r.utell()
        bad = bgzf.GziIndex([(len(raw) + 5, 70000)])
        with pytest.raises(ValueError):
            r.useek(70000, bad)


def test_read_ranges_match_slices_in_one_decode_launch(ctx, golden):
    from zlib_ng_amd import _lib, bgzf
    raw, ref = golden
    _, blocks, _, _ = _lib.bgzf_scan(raw)
    data_blocks = blocks[:-1]
    rng = random.Random(21)
    ranges, want = [], []

    def add(c, u, w, n):
        ranges.append((bgzf.make_virtual_offset(c, w), n))
        want.append(ref[u + w:u + w + n])

    for _ in range(1900):
        c, u, cs, isz = rng.choice(data_blocks)
        add(c, u, rng.randrange(isz), rng.choice([0, 1, 100, 100, 100, 4096]))
    for _ in range(40):                                      # two and three blocks
        c, u, cs, isz = rng.choice(data_blocks[:-3])
        add(c, u, isz - rng.randrange(1, 200), rng.choice([300, isz, isz + 400, 2 * isz]))
    for _ in range(30):                                      # empty ranges, at block starts and ends too
        c, u, cs, isz = rng.choice(data_blocks)
        add(c, u, rng.choice([0, isz - 1, min(isz, 65535)]), 0)
    c, u, cs, isz = data_blocks[-1]
    for w, n in ((isz - 10, 10), (isz - 10, 500), (0, 1 << 20), (min(isz, 65535), 5)):      # the end of the data
        add(c, u, w, n)
    add(blocks[-1][0], blocks[-1][1], 0, 100)                 # the EOF block itself
    while len(ranges) < 2000:
        c, u, cs, isz = rng.choice(data_blocks)
        add(c, u, rng.randrange(isz), 100)
    with bgzf.open(BGZIP) as r:
        r.read(1000)
        at = r.tell()
        ctx.bgzf_stats()
        got = r.read_ranges(ranges)
        launches, nblocks, nslices = ctx.bgzf_stats()
        assert launches == 1 and nslices == 2000 and nblocks <= len(data_blocks)
        assert len(got) == 2000
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (i, ranges[i])
        assert r.tell() == at and r.read(10) == ref[1000:1010]          # the sequential position is untouched
        assert r.read_ranges([]) == [] and r.read_ranges([(0, 0)]) == [b""]
        with pytest.raises(ValueError):
            r.read_ranges([(bgzf.make_virtual_offset(data_blocks[0][0], 65535), 1)] if data_blocks[0][3] < 65535 else [(0, -1)])


def test_slice_table_is_untrusted(ctx, golden):
    from zlib_ng_amd import _lib
    raw, ref = golden
    _, blocks, _, _ = _lib.bgzf_scan(raw)
    c, u, cs, isz = blocks[0]
    members = (_lib.Member * 1)(_lib.Member(18, cs - 26, 0, isz, 0, 0, 0))
    slices = (_lib.BgzfSlice * 4)(_lib.BgzfSlice(5, 0, 10, 0), _lib.BgzfSlice(isz - 4, 10, 10, 0), _lib.BgzfSlice(1 << 40, 20, 10, 0),
                                 _lib.BgzfSlice(0, 95, 10, 0))
    status, sstat, out = ctx.bgzf_read(raw[:cs], members, slices, 100)
    assert status == [0] and sstat == [_lib.BGZF_SLICE_OK, _lib.BGZF_SLICE_TABLE, _lib.BGZF_SLICE_TABLE, _lib.BGZF_SLICE_TABLE]
    assert out[:10] == ref[5:15]
    members[0].in_off = len(raw)                               # a block outside the input: a verdict, no access
    status, sstat, out = ctx.bgzf_read(raw[:cs], members, slices, 100)
    assert status[0] != 0 and sstat[0] == _lib.BGZF_SLICE_BLOCK and out[:10] == bytes(10)


def test_ranged_read_device_form(ctx, golden):
    """zngamd_bgzf_read_dev: blocks, tables, scratch, result and statuses all in device memory"""
    from zlib_ng_amd import _lib, bgzf, devmem
    raw, ref = golden
    _, blocks, _, _ = _lib.bgzf_scan(raw)
    take = blocks[2:6]
    base, end = take[0][0], take[-1][0] + take[-1][2]
    members = np.zeros(len(take), bgzf.MEMBER_DTYPE)
    members["in_off"] = [b[0] - base + 18 for b in take]
    members["in_len"] = [b[2] - 26 for b in take]
    members["out_off"] = [b[1] - take[0][1] for b in take]
    members["out_len"] = [b[3] for b in take]
    total = int(members["out_off"][-1] + members["out_len"][-1])
    slices = np.zeros(3, bgzf.SLICE_DTYPE)
    slices["src_off"], slices["dst_off"], slices["len"] = [7, take[1][1] - take[0][1] - 50, total - 1], [0, 100, 300], [100, 200, 1]
    d_in = devmem.from_host(ctx, raw[base:end] + bytes(64))
    d_m, d_s = devmem.from_host(ctx, members.tobytes()), devmem.from_host(ctx, slices.tobytes())
    d_scratch, d_out = devmem.empty(ctx, total), devmem.empty(ctx, 301).zero_()
    d_st, d_ss = devmem.empty(ctx, 4 * len(take)), devmem.empty(ctx, 4 * 3)
    ctx.bgzf_read_dev(d_in.ptr, end - base, d_m.ptr, len(take), d_s.ptr, 3, d_scratch.ptr, total, d_out.ptr, 301, d_st.ptr, d_ss.ptr)
    assert d_st.cpu(np.int32).tolist() == [0] * len(take) and d_ss.cpu(np.int32).tolist() == [0, 0, 0]
    want = ref[take[0][1]:take[0][1] + total]
    assert d_scratch.cpu().tobytes() == want
    out = d_out.cpu().tobytes()
    a = take[1][1] - take[0][1] - 50
    assert out[:100] == want[7:107] and out[100:300] == want[a:a + 200] and out[300:301] == want[-1:]


# ---- damage
@pytest.fixture(scope="module")
def ten_blocks(inputs):
    from zlib_ng_amd import _lib, bgzf
    data = inputs["fastq"][:10 * BLOCK - 123]
    blob = bgzf.compress(data)
    return data, blob, _lib.bgzf_scan(blob)[1]


def _damaged_reads(blob, data, blocks, bad_block, tmp_path, name):
    from zlib_ng_amd import bgzf
    path = str(tmp_path / name)
    open(path, "wb").write(blob)
    with bgzf.open(path) as r:
        with pytest.raises(bgzf.BadGzipFile, match=f"block {bad_block} "):
            r.read()
    c, u = blocks[bad_block][:2]
    with bgzf.open(path) as r:
        with pytest.raises(bgzf.BadGzipFile, match=f"offset {c}"):
            r.read_ranges([(blocks[1][0] << 16 | 5, 50), (c << 16 | 100, 50)])
        with pytest.raises(bgzf.BadGzipFile):
            r.read_ranges([(blocks[bad_block - 1][0] << 16 | 65000, 1000)])        # reaches into the bad block
        # ranges that stay clear of it are served
        c1, u1 = blocks[1][:2]
        c7, u7 = blocks[7][:2]
        assert r.read_ranges([(c1 << 16 | 5, 50), (c7 << 16 | 65000, 600)]) == [data[u1 + 5:u1 + 55], data[u7 + 65000:u7 + 65600]]
        r.seek(c7 << 16)
        assert r.read(100) == data[u7:u7 + 100]


def test_a_flipped_payload_byte_is_reported_with_its_block(ten_blocks, tmp_path):
    data, blob, blocks = ten_blocks
    bad = bytearray(blob)
    bad[blocks[4][0] + 18 + 700] ^= 0x10
    _damaged_reads(bytes(bad), data, blocks, 4, tmp_path, "payload.bgzf")


def test_a_flipped_crc_byte_is_reported_with_its_block(ten_blocks, tmp_path):
    data, blob, blocks = ten_blocks
    bad = bytearray(blob)
    bad[blocks[4][0] + blocks[4][2] - 7] ^= 0x01
    _damaged_reads(bytes(bad), data, blocks, 4, tmp_path, "crc.bgzf")


def test_a_bsize_pointed_into_the_block_is_reported(ten_blocks, tmp_path):
    from zlib_ng_amd import bgzf
    data, blob, blocks = ten_blocks
    bad = bytearray(blob)
    struct.pack_into("<H", bad, blocks[4][0] + 16, blocks[4][2] - 1 - 1000)
    path = str(tmp_path / "bsize.bgzf")
    open(path, "wb").write(bytes(bad))
    with bgzf.open(path) as r:
        with pytest.raises(bgzf.BadGzipFile, match="block [45] "):
            r.read()
    with bgzf.open(path) as r:
        assert r.read(4 * BLOCK) == data[:4 * BLOCK]            # the blocks in front of it are sound
        with pytest.raises(bgzf.BadGzipFile):
            r.read(1)
    with bgzf.open(path) as r:
        with pytest.raises(bgzf.BadGzipFile):
            r.read_ranges([(blocks[4][0] << 16 | 100, 50)])
        c7, u7 = blocks[7][:2]
        assert r.read_ranges([(c7 << 16 | 1, 50)]) == [data[u7 + 1:u7 + 51]]
    with pytest.raises(bgzf.BadGzipFile):
        bgzf.decompress(bytes(bad))


def test_a_missing_eof_block(ten_blocks, tmp_path):
    from zlib_ng_amd import bgzf
    data, blob, blocks = ten_blocks
    path = str(tmp_path / "noeof.bgzf")
    open(path, "wb").write(blob[:-28])
    with bgzf.open(path) as r:
        assert r.read() == data                                  # htslib only warns
    with pytest.raises(EOFError):
        bgzf.BgzfReader(path, require_eof=True)
    with pytest.raises(EOFError):
        bgzf.open(path, "rb", require_eof=True)
    open(path, "wb").write(blob)
    with bgzf.BgzfReader(path, require_eof=True) as r:
        assert r.read() == data
    open(path, "wb").write(blob[:blocks[6][0] + 500])         # cut inside a block
    with bgzf.open(path) as r:
        assert r.read(6 * BLOCK) == data[:6 * BLOCK]
        with pytest.raises(EOFError):
            r.read()

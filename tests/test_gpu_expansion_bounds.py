"""Worst-case expansion through every compress entry point.  Every entry point sizes its device buffers from a
host-side bound on the largest unit that can be written; the inputs of tests/expansion_inputs.py make units as large as the
format allows -- under Z_FIXED an eighth larger than their bytes -- at the sizes where the bound's terms and the unit plan change.
Per entry point: the call succeeds, CPython's zlib inflates the result to the input, every unit has the referee's size (and the
stream the referee's bytes: tests/test_cpu_expansion_bounds.py anchors it), and the output stays under the tests' own bound.

The grid is cut per entry point to what it can get wrong: the batch API and the block calls see every size at level 6 under every
strategy and the sizes up to 16 385 at levels 1, 6 and 9; the writers without a strategy see noise at their largest block."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import expansion_inputs as X

pytestmark = pytest.mark.gpu

WBITS = (15, -15, 31)
FRAME = {15: (2, 4), -15: (0, 0), 31: (10, 8)}          # bytes of header and trailer


@pytest.fixture(scope="module")
def mods():
    from zlib_ng_amd import _lib, batch, devmem, zlib_ng
    return _lib, batch, devmem, zlib_ng


# ---------------------------------------------------------------------------------------------------------------------------
# the batches
# ---------------------------------------------------------------------------------------------------------------------------
def _batches():
    h = X.high64(X.LONGEST)
    return {
        # made only of expanding items: 1, 2 and 300 of them
        "one": [X.high64(1024)],
        "two": [X.high64(1024), X.high112(1024)],
        "three_hundred": [h[1024 * i:1024 * (i + 1)] for i in range(300)],
        # one expanding item among compressible ones: the bound is a sum, and the neighbours must not be what pays for it
        "among": [X.text(3000), X.text(16384), X.high64(16384), X.text(700), b"", X.text(20000)],
        # every kind at every size up to a unit of 16 KiB and one byte
        "kinds": [d for _, _, d in X.cases(sizes=X.SMALL_SIZES)],
        # every size, and the block of which one unit in three expands
        "sizes": [d for _, _, d in X.cases(["high64"])] + [X.unit_mix()],
    }


BATCHES = _batches()
LEVELS_OF = {"sizes": (6,)}                      # (the referee's time: 1.2 MB a strategy and level)
GRID = [(b, s) for b in BATCHES for s in X.STRATEGIES]
GRID_IDS = ["%s-%s" % (b, X.STRATEGY_NAMES[s]) for b, s in GRID]


def _inflate(stream, wbits, zdict=None):
    d = zlib.decompressobj(wbits, zdict=zdict) if zdict is not None else zlib.decompressobj(wbits)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def _check_items(items, outs, level, strategy, wbits, zdict=None, tag=None):
    """every item: the round trip, the referee's bytes between header and trailer (so every unit's size), the tests' bound"""
    hl, tl = FRAME[wbits]
    if zdict is not None and wbits == 15:
        hl += 4                                  # DICTID
    assert len(outs) == len(items)
    for i, (a, b) in enumerate(zip(items, outs)):
        t = (tag, i, len(a), level, X.STRATEGY_NAMES[strategy], wbits)
        usize = X.batch_unit_size(len(a), zdict is not None)
        assert len(b) <= hl + X.bound(len(a), strategy, True, usize) + tl, (t, len(b))
        assert _inflate(b, wbits, zdict) == a, t
        sizes = X.block_sizes(a, level, strategy, usize=usize, zdict=zdict or b"")
        assert len(b) - hl - tl == sum(sizes), (t, len(b) - hl - tl, sizes)
        assert b[hl:len(b) - tl] == X.block_bytes(a, level, strategy, usize=usize, zdict=zdict or b""), t


# ---------------------------------------------------------------------------------------------------------------------------
# batch.compress
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,strategy", GRID, ids=GRID_IDS)
def test_batch_compress(mods, name, strategy):
    _lib, batch, devmem, zlib_ng = mods
    items = BATCHES[name]
    for level in LEVELS_OF.get(name, X.LEVELS):
        for wbits in WBITS:
            outs = batch.compress(items, level, wbits, strategy=strategy)
            _check_items(items, outs, level, strategy, wbits, tag=name)


ZDICT_ITEMS = [X.high64(1024), X.high64(16385), X.high112(1024), X.low_then_high(16384), X.high64(X.UNIT + 1)]
ZDICTS = {"no_help": X.noise(4096), "holds_the_item": X.text(1000) + X.high64(20000)}


@pytest.mark.parametrize("strategy", X.STRATEGIES, ids=lambda s: X.STRATEGY_NAMES[s])
@pytest.mark.parametrize("which", list(ZDICTS))
def test_batch_compress_zdict(mods, which, strategy):
    """with a dictionary that does not help and one that holds the item (the first two are its own bytes): byte for byte what
    compressobj(level, DEFLATED, wbits, strategy=..., zdict=...) writes, and the referee's units behind the dictionary's tail"""
    _lib, batch, devmem, zlib_ng = mods
    zd = ZDICTS[which]
    for level in (X.LEVELS if strategy == X.FIXED else (6,)):
        for wbits in (15, -15):
            outs = batch.compress(ZDICT_ITEMS, level, wbits, strategy=strategy, zdict=zd)
            _check_items(ZDICT_ITEMS, outs, level, strategy, wbits, zdict=zd, tag=which)
            for a, b in zip(ZDICT_ITEMS, outs):
                c = zlib_ng.compressobj(level, zlib_ng.DEFLATED, wbits, zlib_ng.DEF_MEM_LEVEL, strategy, zd)
                assert b == c.compress(a) + c.flush(), (which, len(a), level, strategy, wbits)
    if which == "holds_the_item" and strategy == X.FIXED:
        # copies of the dictionary, one match a segment (32 bytes in a unit of 1 024, 512 in one of 16 385; at most 31 bits each)
        assert len(outs[0]) <= 32 * 31 // 8 + 2 and len(outs[1]) < 16385 // 8


# ---------------------------------------------------------------------------------------------------------------------------
# batch.compress_dev and zngamd_deflate_batch_dict_dev
# ---------------------------------------------------------------------------------------------------------------------------
def _device_items(_lib, devmem, ctx, items):
    flat = b"".join(items)
    lens = [len(x) for x in items]
    offs = np.cumsum([0] + lens[:-1]).tolist()
    return devmem.from_host(ctx, np.frombuffer(flat + bytes(_lib.BATCH_PAD), np.uint8)), offs, lens


@pytest.mark.parametrize("name,strategy", GRID, ids=GRID_IDS)
def test_batch_compress_dev(mods, ctx, name, strategy):
    _lib, batch, devmem, zlib_ng = mods
    items = BATCHES[name]
    d_in, offs, lens = _device_items(_lib, devmem, ctx, items)
    for level in LEVELS_OF.get(name, X.LEVELS):
        for wbits in WBITS:
            buf, o, ln = batch.compress_dev(ctx, d_in, offs, lens, level, wbits, strategy=strategy)
            host = buf.cpu().tobytes()
            outs = [host[int(a):int(a) + int(b)] for a, b in zip(o, ln)]
            _check_items(items, outs, level, strategy, wbits, tag=name)
            assert int(o[-1]) + int(ln[-1]) <= batch._frame_bound(lens, wbits, None, strategy)
            buf.free()
    d_in.free()


def test_batch_compress_dev_zdict(mods, ctx):
    _lib, batch, devmem, zlib_ng = mods
    d_in, offs, lens = _device_items(_lib, devmem, ctx, ZDICT_ITEMS)
    for which, zd in ZDICTS.items():
        for wbits in (15, -15):
            buf, o, ln = batch.compress_dev(ctx, d_in, offs, lens, 6, wbits, strategy=X.FIXED, zdict=zd)
            host = buf.cpu().tobytes()
            _check_items(ZDICT_ITEMS, [host[int(a):int(a) + int(b)] for a, b in zip(o, ln)], 6, X.FIXED, wbits, zdict=zd, tag=which)
            buf.free()
    d_in.free()


@pytest.mark.parametrize("name", ["one", "three_hundred", "among", "sizes"])
def test_deflate_batch_dev_destination(mods, ctx, name):
    """the caller's own destination, through the C call: one byte less than the stream needs is BUF_ERROR with the size needed --
    never an engine error --, and exactly that size succeeds with the same bytes"""
    _lib, batch, devmem, zlib_ng = mods
    items = BATCHES[name]
    n = len(items)
    d_in, offs, lens = _device_items(_lib, devmem, ctx, items)
    table = (_lib.BatchItem * n)()
    for k in range(n):
        table[k].in_off, table[k].in_len = offs[k], lens[k]
    room = batch._frame_bound(lens, 15, None, X.FIXED)
    d_out, d_res = devmem.DeviceBuffer(ctx, room + 64), devmem.DeviceBuffer(ctx, 16 * n)
    r, total = ctx.deflate_batch_dev(d_in.ptr, sum(lens), table, n, 6, 15, X.FIXED, d_out.ptr, room, d_res.ptr)
    assert r == _lib.OK and total <= room, (r, ctx.err(), total, room)
    whole = d_out[:total].cpu().tobytes()
    assert total == sum(2 + sum(X.block_sizes(a, 6, X.FIXED, usize=X.batch_unit_size(len(a)))) + 4 for a in items)
    d_out[:] = 0xA5
    r, need = ctx.deflate_batch_dev(d_in.ptr, sum(lens), table, n, 6, 15, X.FIXED, d_out.ptr, total - 1, d_res.ptr)
    assert (r, need) == (_lib.BUF_ERROR, total), (r, ctx.err(), need, total)
    assert not (d_out.cpu() != 0xA5).any()                     # nothing was written
    r, again = ctx.deflate_batch_dev(d_in.ptr, sum(lens), table, n, 6, 15, X.FIXED, d_out.ptr, total, d_res.ptr)
    assert (r, again) == (_lib.OK, total), (r, ctx.err())
    back = d_out.cpu().tobytes()
    assert back[:total] == whole and back[total:] == b"\xa5" * (len(back) - total)
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)
    outs = [whole[table[k].out_off:table[k].out_off + int(res[k, 1])] for k in range(n)]
    assert not res[:, 0].any()
    _check_items(items, outs, 6, X.FIXED, 15, tag=name)
    for d in (d_in, d_out, d_res):
        d.free()


# ---------------------------------------------------------------------------------------------------------------------------
# zlib_ng.compressobj(strategy=...)
# ---------------------------------------------------------------------------------------------------------------------------
def _stream(zlib_ng, level, strategy, wbits=-15):
    return zlib_ng.compressobj(level, zlib_ng.DEFLATED, wbits, zlib_ng.DEF_MEM_LEVEL, strategy)


@pytest.mark.parametrize("strategy", X.STRATEGIES, ids=lambda s: X.STRATEGY_NAMES[s])
@pytest.mark.parametrize("which", ["kinds", "sizes"])
def test_compressobj_one_piece(mods, which, strategy):
    """one compress and flush: one FINAL block in units of 128 KiB -- 131 073 bytes make two, 262 145 three"""
    _lib, batch, devmem, zlib_ng = mods
    for level in LEVELS_OF.get(which, X.LEVELS):
        for data in BATCHES[which]:
            c = _stream(zlib_ng, level, strategy)
            out = c.compress(data) + c.flush()
            t = (which, len(data), level, X.STRATEGY_NAMES[strategy])
            assert len(out) <= X.bound(len(data), strategy), t
            assert _inflate(out, -15) == data, t
            assert len(out) == sum(X.block_sizes(data, level, strategy)), t
            assert out == X.block_bytes(data, level, strategy), t
    c = _stream(zlib_ng, 6, strategy, 31)
    data = X.high64(16385)
    assert gzip.decompress(c.compress(data) + c.flush()) == data


@pytest.mark.parametrize("strategy", X.STRATEGIES, ids=lambda s: X.STRATEGY_NAMES[s])
def test_compressobj_sync_flushed_pieces(mods, strategy):
    """pieces of 1 000 bytes with Z_SYNC_FLUSH between them: every piece a unit that is not the last, behind the bytes in front of
    it; the closing flush an empty final unit"""
    _lib, batch, devmem, zlib_ng = mods
    data = X.high64(16385)
    for level in X.LEVELS:
        c = _stream(zlib_ng, level, strategy)
        got, exp = [], []
        for p in range(0, len(data), 1000):
            got.append(c.compress(data[p:p + 1000]) + c.flush(zlib.Z_SYNC_FLUSH))
            u = X.unit_ref(data[:p + 1000], p, level, strategy)
            exp.append(u.out(False))
            assert len(got[-1]) == u.size(False) <= X.unit_bound(len(u.data), strategy, False), (level, strategy, p)
        got.append(c.flush())
        exp.append(b"\x03\x00")
        assert got == exp, (level, strategy)
        assert _inflate(b"".join(got), -15) == data


def test_compressobj_large_piece_in_place(mods):
    """A piece of 32 MiB or more is compressed where it lies (zs_deflate_batch): its first 128 KiB through the head buffer, the
    rest in place.  No referee at this size: the call succeeds, every unit is a fixed block of all literals but for chance
    repeats, and the stream is under the sum of the units' bounds."""
    _lib, batch, devmem, zlib_ng = mods
    n = (32 << 20) + 1
    data = np.random.default_rng(9100).integers(144, 208, size=n, dtype=np.uint8).tobytes()
    c = _stream(zlib_ng, 1, X.FIXED)
    out = c.compress(data) + c.flush()
    assert n + n // 9 < len(out) <= X.bound(n, X.FIXED)
    assert _inflate(out, -15) == data


# ---------------------------------------------------------------------------------------------------------------------------
# Context.deflate_blocks and zngamd_deflate_blocks_packed_dev
# ---------------------------------------------------------------------------------------------------------------------------
def _blocks_of(items):
    """every item a block of its own, without a dictionary; every other one FINAL -> (buffer, block list, [final])"""
    buf, blocks, finals = bytearray(), [], []
    for i, d in enumerate(items):
        blocks.append((len(buf), len(d), 0, i & 1))
        finals.append(bool(i & 1))
        buf += d
    return bytes(buf), blocks, finals


@pytest.mark.parametrize("strategy", X.STRATEGIES, ids=lambda s: X.STRATEGY_NAMES[s])
@pytest.mark.parametrize("which", ["kinds", "sizes"])
def test_deflate_blocks(mods, ctx, which, strategy):
    """the per-block form with a cap of n + n // 8 + 64, the joined form, and the joined form with its index (the units' sizes)"""
    _lib, batch, devmem, zlib_ng = mods
    items = BATCHES[which]
    buf, blocks, finals = _blocks_of(items)
    big = max(len(d) for d in items)
    cap = big + big // 8 + 64
    for level in LEVELS_OF.get(which, X.LEVELS):
        exp = [X.block_bytes(d, level, strategy, final=f) for d, f in zip(items, finals)]
        usz = [s for d, f in zip(items, finals) for s in X.block_sizes(d, level, strategy, final=f)]
        outs, crcs, ovf = ctx.deflate_blocks(buf, blocks, level, cap, strategy=strategy)
        assert not ovf and crcs == [zlib.crc32(d) for d in items]
        for d, f, got, want in zip(items, finals, outs, exp):
            t = (which, len(d), level, X.STRATEGY_NAMES[strategy], f)
            assert len(got) <= X.bound(len(d), strategy, f), t
            assert _inflate(got + (b"" if f else b"\x03\x00"), -15) == d, t
            assert len(got) == len(want) and got == want, t
        joined, crcs2, ovf2, lens = ctx.deflate_blocks(buf, blocks, level, cap, joined=True, strategy=strategy)
        assert not ovf2 and crcs2 == crcs and lens == [len(x) for x in exp] and bytes(joined) == b"".join(exp)
        joined, crcs3, ovf3, lens3, rec = ctx.deflate_blocks(buf, blocks, level, cap, joined=True, index=True, strategy=strategy)
        assert not ovf3 and crcs3 == crcs and lens3 == lens and bytes(joined) == b"".join(exp)
        assert rec["in_len"].tolist() == usz, (which, level, strategy)
        assert rec["out_len"].tolist() == [ln for d in items for _, ln in X.unit_plan(len(d))]


@pytest.mark.parametrize("final", [False, True])
def test_deflate_blocks_cap_is_exclusive(ctx, final):
    """a block whose size equals the per-block cap is an overflow (the engine's test is size >= cap); one byte more room holds
    it -- on an expanding unit, whose size is past its length"""
    data = X.high64(1024)
    size = X.block_sizes(data, 6, X.FIXED, final=final)[0]
    assert size > 1024 + 32
    blocks = [(0, 1024, 0, int(final))]
    for joined in (False, True):
        res = ctx.deflate_blocks(data, blocks, 6, size, joined=joined, strategy=X.FIXED)
        assert res[2] and (res[0] is None if joined else res[0] == [None])
        res = ctx.deflate_blocks(data, blocks, 6, size + 1, joined=joined, strategy=X.FIXED)
        assert not res[2] and bytes(res[0] if joined else res[0][0]) == X.block_bytes(data, 6, X.FIXED, final=final)


@pytest.mark.parametrize("strategy", [X.DEFAULT, X.FIXED], ids=lambda s: X.STRATEGY_NAMES[s])
@pytest.mark.parametrize("which", ["kinds", "sizes"])
def test_deflate_blocks_packed_dev(mods, ctx, which, strategy):
    """device resident, the caller's destination: an exact fit succeeds and writes nothing behind it, one byte less is BUF_ERROR
    with the size needed; the units' sizes are the referee's"""
    _lib, batch, devmem, zlib_ng = mods
    items = BATCHES[which]
    buf, blocks, finals = _blocks_of(items)
    arr, nb = _lib.with_strategy(_lib.block_table(blocks), strategy)
    L, h = ctx.L, ctx.h
    nu = L.zngamd_count_units(arr, nb)
    exp = b"".join(X.block_bytes(d, 6, strategy, final=f) for d, f in zip(items, finals))
    usz = [s for d, f in zip(items, finals) for s in X.block_sizes(d, 6, strategy, final=f)]
    assert nu == len(usz) and len(exp) == sum(usz) <= sum(X.bound(len(d), strategy, f) for d, f in zip(items, finals))
    d_in = devmem.from_host(ctx, np.frombuffer(buf + bytes(64), np.uint8))
    d_out, d_len, d_crc = devmem.DeviceBuffer(ctx, len(exp) + 64), devmem.DeviceBuffer(ctx, 4 * nu), devmem.DeviceBuffer(ctx, 4 * nu)
    total = C.c_uint64(0)

    def call(room):
        d_out[:] = 0xA5
        return L.zngamd_deflate_blocks_packed_dev(h, d_in.vp(), len(buf), arr, nb, 6, d_out.vp(), room, d_len.vp(), d_crc.vp(), None, C.byref(total))

    assert call(len(exp)) == _lib.OK, ctx.err()
    back = d_out.cpu().tobytes()
    assert total.value == len(exp) and back[:len(exp)] == exp and back[len(exp):] == b"\xa5" * 64
    assert d_len.cpu(np.uint32).tolist() == usz
    assert call(len(exp) - 1) == _lib.BUF_ERROR and total.value == len(exp), ctx.err()
    assert d_out[len(exp) - 1:].cpu().tobytes() == b"\xa5" * 65          # (units that did not fit are not written)
    for d in (d_in, d_out, d_len, d_crc):
        d.free()


# ---------------------------------------------------------------------------------------------------------------------------
# the writers without a strategy: noise at their largest block
# ---------------------------------------------------------------------------------------------------------------------------
def test_gzip_ng_compress_noise():
    from zlib_ng_amd import gzip_ng
    data = X.noise(3 * X.UNIT)
    for level in (1, 6, 9):
        assert gzip.decompress(gzip_ng.compress(data, level)) == data


def test_threaded_writer_noise(tmp_path):
    from zlib_ng_amd import gzip_ng_threaded
    data = X.noise(3 * X.UNIT)
    for block_size in (X.UNIT, 1000):
        path = tmp_path / ("noise%d.gz" % block_size)
        with gzip_ng_threaded.open(path, "wb", 6, threads=1, block_size=block_size) as f:
            f.write(data[:8 * block_size + 1])
        assert gzip.decompress(path.read_bytes()) == data[:8 * block_size + 1]


def test_bgzf_writer_noise(tmp_path):
    """blocks of 65 280 bytes of noise, stored: every BGZF block within 65 536 bytes (its BSIZE field is 16 bits)"""
    from zlib_ng_amd import bgzf
    data = X.noise(4 * bgzf.MAX_BLOCK_INPUT + 17)
    path = tmp_path / "noise.bgz"
    with bgzf.open(path, "wb", 6) as f:
        f.write(data)
    for stream in (bgzf.compress(data, 6), path.read_bytes()):
        assert gzip.decompress(stream) == data
        pos, sizes = 0, []
        while pos < len(stream):
            assert stream[pos:pos + 4] == b"\x1f\x8b\x08\x04" and stream[pos + 12:pos + 16] == b"BC\x02\x00"
            sizes.append(struct.unpack_from("<H", stream, pos + 16)[0] + 1)
            pos += sizes[-1]
        assert pos == len(stream) and len(sizes) == 6 and max(sizes) <= bgzf.MAX_BLOCK
        assert sizes[0] == 18 + bgzf.MAX_BLOCK_INPUT + 5 + 8              # header, one stored block, CRC-32 and ISIZE

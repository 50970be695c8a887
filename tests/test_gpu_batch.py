"""The batch API on the GPU (zlib_ng_amd.batch): every item against the one-shot calls, with CPython's zlib as referee -- byte identity
with zlib_ng.compress, strategies, foreign streams, the count pass, items above the large-item threshold, every error class in one
call, the device-resident forms and a hostile device item table."""
import ctypes as C
import gzip
import random
import struct
import zlib

import numpy as np
import pytest

import deflate_walk as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from zlib_ng_amd import _lib, batch, corpus, devmem, zlib_ng
    return _lib, batch, corpus, devmem, zlib_ng


def _mixed(corpus, n=2000, seed=1):
    rng = random.Random(seed)
    text = corpus.text(3 << 20, seed=seed).tobytes()
    sizes = [0, 1, 100, 4096, 131071, 131072, 131073, 1 << 20]
    items = []
    for i in range(n):
        s = sizes[i % len(sizes)] if i < 64 else rng.choice([0, 1, 100, 4096, 1000, 7000])
        o = rng.randrange(0, len(text) - s + 1)
        items.append(text[o:o + s] if i % 5 else bytes(rng.randrange(256) for _ in range(min(s, 300))) + text[o:o + max(0, s - 300)])
    return items


@pytest.mark.parametrize("wbits", [15, 9, 31, 25, -15, -9])
def test_compress_is_the_oneshot_byte_for_byte(mods, wbits):
    _lib, batch, corpus, devmem, zlib_ng = mods
    items = _mixed(corpus, 2000 if wbits in (15, 31, -15) else 400)
    for level in (-1, 0, 1, 6, 9):
        out = batch.compress(items, level, wbits)
        assert len(out) == len(items)
        for i, (a, b) in enumerate(zip(items, out)):
            assert b == zlib_ng.compress(a, level, wbits), (level, i, len(a))
        for a, b in zip(items[:64], out[:64]):
            assert zlib.decompress(b, wbits) == a


@pytest.mark.parametrize("strategy", [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
def test_strategies_round_trip_with_their_structure(mods, strategy):
    _lib, batch, corpus, devmem, zlib_ng = mods
    items = _mixed(corpus, 300, seed=4)
    for wbits in (15, 31, -15):
        out = batch.compress(items, 6, wbits, strategy=strategy)
        for a, b in zip(items, out):
            assert zlib.decompress(b, wbits) == a
            msg = W.check_strategy(W.walk(W.strip_container(b, wbits)), strategy)
            assert msg is None, msg


def test_decompress_foreign_streams(mods):
    _lib, batch, corpus, devmem, zlib_ng = mods
    rng = random.Random(5)
    text = corpus.text(1 << 20, seed=6).tobytes()
    raw_items, zl, gz = [], [], []
    for i in range(600):
        s = rng.choice([0, 1, 50, 1000, 4096, 20000])
        o = rng.randrange(0, len(text) - s + 1)
        d = text[o:o + s]
        level = rng.randrange(0, 10)
        strat = rng.choice([0, 1, 2, 3, 4])
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strat)
        zl.append((d, co.compress(d) + co.flush()))
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strat)
        raw_items.append((d, co.compress(d) + co.flush()))
        gz.append((d, gzip.compress(d, compresslevel=max(level, 1), mtime=0)))
    # gzip members with every header field and FHCRC
    for i in range(40):
        d = text[i * 1000:i * 1000 + 3000 + i]
        body = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = body.compress(d) + body.flush()
        head = bytes([0x1f, 0x8b, 8, 4 | 8 | 16 | 2, 1, 2, 3, 4, 0, 3]) + struct.pack("<H", 5 + i) + bytes(range(5 + i)) + \
            b"name%d\0" % i + b"comment\0"
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
        gz.append((d, head + body + struct.pack("<II", zlib.crc32(d), len(d))))
    # stored-only and fixed-only
    for lv, st in ((0, 0), (6, zlib.Z_FIXED)):
        for i in range(20):
            d = text[i * 333:i * 333 + 70000]
            co = zlib.compressobj(lv, zlib.DEFLATED, 15, 8, st)
            zl.append((d, co.compress(d) + co.flush()))
    for wbits, pairs in ((15, zl), (-15, raw_items), (31, gz)):
        out = batch.decompress([p[1] for p in pairs], wbits)
        for (d, c), o in zip(pairs, out):
            assert o == d == zlib_ng.decompress(c, wbits)
    mix = zl[:200] + gz
    rng.shuffle(mix)
    for wbits in (47, 32):
        out = batch.decompress([p[1] for p in mix], wbits)
        assert out == [p[0] for p in mix]


def test_count_pass_and_large_items(mods):
    _lib, batch, corpus, devmem, zlib_ng = mods
    text = corpus.text(1 << 20, seed=8).tobytes()
    rnd = np.random.default_rng(3).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    datas = [text[i * 1024:(i + 1) * 1024] for i in range(40)]
    datas[7] = bytes(8 << 20)                       # 8 MiB of zeros: the first room guess overflows
    datas[20] = b"a" * (3 << 20)
    datas[30] = rnd                                 # compresses to ~1 MiB: above the large-item threshold
    for wbits in (15, 31, -15):
        comp = [zlib.compress(d, 6) if wbits == 15 else gzip.compress(d, mtime=0) if wbits == 31 else zlib.compress(d, 6)[2:-4]
                for d in datas]
        assert len(comp[30]) >= batch.LARGE_ITEM
        out = batch.decompress(comp, wbits)
        assert out == datas
        assert [zlib_ng.decompress(c, wbits) for c in comp] == out


def test_every_error_class_in_one_call(mods):
    _lib, batch, corpus, devmem, zlib_ng = mods
    text = corpus.text(200000, seed=9).tobytes()
    good = zlib.compress(text[:20000], 6)
    items_z = [
        good,
        good[:len(good) // 2], good[len(good) // 2:],     # a truncated item followed by its own continuation: still truncated
        good[:40] + bytes([good[40] ^ 0x10]) + good[41:],  # a flipped deflate bit
        good[:-1] + bytes([good[-1] ^ 1]),                 # bad Adler-32
        b"\x78\x9d" + good[2:],                            # bad header check
        struct.pack(">H", (0x79 << 8) + 31 - ((0x79 << 8) % 31)) + good[2:],     # bad method
        struct.pack(">H", (0x78 << 8 | 0x20) + 31 - ((0x78 << 8 | 0x20) % 31)) + good[2:],         # FDICT
        b"\x78", b"", good[:-2],
    ]
    gz = gzip.compress(text[:30000], mtime=0)
    hc = bytes([0x1f, 0x8b, 8, 2, 0, 0, 0, 0, 0, 3]) + b"\x00\x00" + gz[10:]       # FHCRC that does not match
    items_g = [gz, gz[:-8] + struct.pack("<I", zlib.crc32(text[:30000]) ^ 1) + gz[-4:], gz[:-4] + struct.pack("<I", 7),
               gz[:1] + b"\x8c" + gz[2:], gz[:2] + b"\x09" + gz[3:], gz[:3] + b"\x40" + gz[4:], hc, gz[:-3], gz[:12]]
    for wbits, items in ((15, items_z), (9, [good]), (31, items_g), (47, items_z + items_g)):
        got = batch.decompress(items, wbits, errors="return")
        first = None
        for i, (c, g) in enumerate(zip(items, got)):
            try:
                want = zlib_ng.decompress(c, wbits)
            except Exception as e:
                assert type(g) is type(e) and str(g) == str(e), (wbits, i, g, e)
                assert g.index == i
                first = i if first is None else first
            else:
                assert g == want, (wbits, i)
        assert first is not None
        with pytest.raises(zlib_ng.error) as ei:
            batch.decompress(items, wbits)
        assert ei.value.index == first
    # the truncated piece stays truncated though the next item continues it in the buffer
    assert "truncated" in str(batch.decompress(items_z, 15, errors="return")[1])


def test_device_forms_round_trip_in_hbm(mods):
    _lib, batch, corpus, devmem, zlib_ng = mods
    ctx = _lib.default_context()
    items = _mixed(corpus, 500, seed=11)
    lens = np.array([len(x) for x in items], dtype=np.uint64)
    offs = np.zeros(len(items), dtype=np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]
    flat = b"".join(items)
    d_in = devmem.from_host(ctx, np.frombuffer(flat + bytes(_lib.BATCH_PAD), np.uint8))
    for wbits in (15, 31, -15):
        d_c, coffs, clens = batch.compress_dev(ctx, d_in, offs, lens, 6, wbits)
        host_c = d_c.cpu().tobytes()
        for i in range(0, len(items), 37):
            assert host_c[int(coffs[i]):int(coffs[i] + clens[i])] == zlib_ng.compress(items[i], 6, wbits)
        # the compressed items decoded where they lie
        total_c = int(coffs[-1] + clens[-1])
        d_cp = devmem.DeviceBuffer(ctx, total_c + _lib.BATCH_PAD)
        d_cp[:total_c] = d_c[:total_c]
        d_cp[total_c:] = 0
        d_out, ooffs, olens, st = batch.decompress_dev(ctx, d_cp, coffs, clens, wbits)
        assert (st == 0).all() and (olens == lens).all()
        assert (ooffs == offs).all()
        assert d_out[:len(flat)].equal(d_in[:len(flat)])           # zngamd_compare_dev


def test_hostile_device_item_table(mods):
    _lib, batch, corpus, devmem, zlib_ng = mods
    ctx = _lib.default_context()
    good = zlib.compress(corpus.text(5000, seed=2).tobytes(), 6)
    in_len = len(good)
    d_in = devmem.from_host(ctx, np.frombuffer(good + bytes(_lib.BATCH_PAD), np.uint8))
    G = 4096
    out_cap = 4 * 5000
    d_out = devmem.DeviceBuffer(ctx, out_cap + 2 * G)
    d_out[:] = 0xA5
    body = d_out[G:G + out_cap]
    M = 0xFFFFFFFF
    rows = [  # in_off, out_off, in_len, out_cap; good entries beside bad ones
        (0, 0, in_len, 5000),
        (1 << 40, 5000, in_len, 5000),                 # input offset far outside
        (in_len - 10, 5000, 100, 5000),                # input runs past the buffer
        (0, out_cap - 100, in_len, 5000),              # output runs past the buffer
        (0, (1 << 64) - 16, in_len, 64),               # output offset that wraps
        ((1 << 64) - 8, 5000, 16, 5000),               # input offset that wraps
        (0, 5000, M, 5000),                            # length beyond the buffer
        (0, 10000, in_len, 5000),
        (0, 15000, in_len, M),                         # room beyond the buffer
    ]
    tab = np.array([[a, b, c | (d << 32), 0] for a, b, c, d in rows], dtype=np.uint64)
    d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
    d_res = devmem.DeviceBuffer(ctx, 16 * len(rows))
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, len(rows), 15, False, body.ptr, out_cap, d_res.ptr)
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)
    assert list(res[:, 0]) == [0, 12, 12, 12, 12, 12, 12, 0, 12]
    assert res[0, 1] == res[7, 1] == 5000
    host = d_out.cpu().tobytes()
    assert host[:G] == b"\xa5" * G and host[G + out_cap:] == b"\xa5" * G
    want = corpus.text(5000, seed=2).tobytes()
    assert host[G:G + 5000] == want and host[G + 10000:G + 15000] == want
    # count-only over the same table: sizes without output
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, len(rows), 15, True, None, 0, d_res.ptr)
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)
    assert res[0, 0] == 0 and res[0, 1] == 5000 and res[0, 2] == in_len and res[1, 0] == 12
    # n = 0
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, 0, 15, False, body.ptr, out_cap, d_res.ptr)


def test_sub_batches_give_the_same_results(mods, monkeypatch):
    _lib, batch, corpus, devmem, zlib_ng = mods
    items = _mixed(corpus, 300, seed=12)
    c_whole = batch.compress(items, 6, 31)
    d_whole = batch.decompress(c_whole, 31)
    monkeypatch.setattr(batch, "SUB_BATCH_BYTES", 100000)
    assert batch.compress(items, 6, 31) == c_whole
    assert batch.decompress(c_whole, 31) == d_whole == items


def test_plain_entry_points_are_the_dict_forms_without_one(mods):
    """zngamd_{inflate,deflate}_batch[_dev] (the binding calls only the _dict forms) give what the _dict forms give with NULL / 0:
    the same return code and message, output bytes, results, item table and total, on a small mixed set and on refused calls"""
    _lib, batch, corpus, devmem, zlib_ng = mods
    ctx = _lib.default_context()
    L, h = ctx.L, ctx.h
    vp = lambda b: C.cast(C.c_char_p(b), C.c_void_p)
    items = _mixed(corpus, 100, seed=13)
    lens = [len(x) for x in items]
    flat = b"".join(items)
    n = len(items)

    def host(call, data, lens):
        """-> (code, message, item table, per item (status, out_len, its output if OK), total)"""
        tab, items_c = batch._table(lens)
        res = (_lib.BatchResult * max(len(lens), 1))()
        box = []

        def alloc(_user, nbytes):
            obj, addr = _lib._new_bytes(nbytes)
            box.append(obj)
            return addr.value

        fn = _lib.ALLOC_FN(alloc)
        total = C.c_uint64(7)
        r = call(vp(data), len(data), C.cast(items_c, C.c_void_p), len(lens), fn, C.cast(res, C.c_void_p), C.byref(total))
        out = box[0] if box else b""
        per = [(res[k].status, res[k].out_len,
                out[int(tab[k, 1]):int(tab[k, 1]) + res[k].out_len] if r == _lib.OK and res[k].status == _lib.BATCH_OK else None)
               for k in range(len(lens))]
        return r, ctx.err() if r else "", tab[:len(lens)].tolist(), per, total.value

    # host deflate: good calls, a bad level, a bad strategy, a bad wbits
    for level, wbits, strategy in ((6, 15, 0), (1, 31, zlib.Z_RLE), (9, -15, 0), (10, 15, 0), (6, 15, 9), (6, 17, 0)):
        plain = host(lambda d, dl, it, k, fn, res, tot: L.zngamd_deflate_batch(h, d, dl, it, k, level, wbits, strategy, fn, None, res, tot),
                     flat, lens)
        nulld = host(lambda d, dl, it, k, fn, res, tot: L.zngamd_deflate_batch_dict(h, d, dl, it, k, level, wbits, strategy, None, 0, fn, None,
                                                                                     res, tot), flat, lens)
        assert plain == nulld, (level, wbits, strategy)
        assert (plain[0] == _lib.OK) == (level <= 9 and strategy <= zlib.Z_FIXED and wbits != 17)

    # host inflate: good and broken items, automatic detection, a bad wbits
    comp = batch.compress(items, 6, 31)
    comp[3] = comp[3][:-5]
    comp[7] = comp[7][:20] + bytes([comp[7][20] ^ 0x55]) + comp[7][21:]
    comp[11] = b"\x00" * 30
    cflat = b"".join(comp)
    clens = [len(x) for x in comp]
    for wbits in (31, 47, 15, 7):
        plain = host(lambda d, dl, it, k, fn, res, tot: L.zngamd_inflate_batch(h, d, dl, it, k, wbits, fn, None, res), cflat, clens)
        nulld = host(lambda d, dl, it, k, fn, res, tot: L.zngamd_inflate_batch_dict(h, d, dl, it, k, wbits, None, 0, fn, None, res),
                     cflat, clens)
        assert plain == nulld, wbits
    assert plain[0] == _lib.STREAM_ERROR and nulld[1] == "invalid wbits"

    # device deflate: fitting and too small an output, a bad strategy
    d_in = devmem.from_host(ctx, np.frombuffer(flat + bytes(_lib.BATCH_PAD), np.uint8))
    cap = batch._frame_bound(lens, 15)

    def dev_deflate(call, out_cap, strategy):
        items_c = (_lib.BatchItem * n)()
        for k, (o, ln) in enumerate(zip(np.cumsum([0] + lens[:-1]).tolist(), lens)):
            items_c[k].in_off, items_c[k].in_len = o, ln
        d_out = devmem.DeviceBuffer(ctx, cap)
        d_out[:] = 0
        d_res = devmem.DeviceBuffer(ctx, 16 * n)
        d_res[:] = 0
        total = C.c_uint64(7)
        r = call(C.c_void_p(d_in.ptr), len(flat), C.cast(items_c, C.c_void_p), C.c_void_p(d_out.ptr), out_cap, C.c_void_p(d_res.ptr),
                 strategy, C.byref(total))
        return (r, ctx.err() if r else "", d_out.cpu().tobytes(), d_res.cpu().tobytes(), [items_c[k].out_off for k in range(n)],
                total.value)

    codes = []
    for out_cap, strategy in ((cap, 0), (cap, zlib.Z_FILTERED), (100, 0), (cap, 9)):
        plain = dev_deflate(lambda d, dl, it, o, oc, res, s, tot: L.zngamd_deflate_batch_dev(h, d, dl, it, n, 6, 15, s, o, oc, res, tot),
                            out_cap, strategy)
        nulld = dev_deflate(lambda d, dl, it, o, oc, res, s, tot: L.zngamd_deflate_batch_dict_dev(h, d, dl, it, n, 6, 15, s, None, 0, o, oc,
                                                                                                 res, tot), out_cap, strategy)
        assert plain == nulld, (out_cap, strategy)
        codes.append(plain[0])
    assert codes == [_lib.OK, _lib.OK, _lib.BUF_ERROR, _lib.STREAM_ERROR]

    # device inflate: the count pass, then a decode into exactly the counted room
    d_c = devmem.from_host(ctx, np.frombuffer(cflat + bytes(_lib.BATCH_PAD), np.uint8))
    sizes = [len(zlib_ng.decompress(x, 31)) if k not in (3, 7, 11) else 0 for k, x in enumerate(comp)]
    tab = np.zeros((n, 4), dtype=np.uint64)
    tab[:, 0] = np.cumsum([0] + clens[:-1])
    tab[:, 1] = np.cumsum([0] + sizes[:-1])
    tab[:, 2] = np.array(clens, dtype=np.uint64) | (np.array(sizes, dtype=np.uint64) << np.uint64(32))
    d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
    room = sum(sizes)

    def dev_inflate(call, count_only, wbits):
        d_out = devmem.DeviceBuffer(ctx, room + 64)
        d_out[:] = 0
        d_res = devmem.DeviceBuffer(ctx, 16 * n)
        d_res[:] = 0
        r = call(C.c_void_p(d_c.ptr), len(cflat), C.c_void_p(d_tab.ptr), wbits, count_only,
                 None if count_only else C.c_void_p(d_out.ptr), 0 if count_only else room, C.c_void_p(d_res.ptr))
        return r, ctx.err() if r else "", d_out.cpu().tobytes(), d_res.cpu().tobytes()

    for count_only, wbits in ((1, 31), (0, 31), (0, 47), (0, 3)):
        plain = dev_inflate(lambda d, dl, t, w, co, o, oc, res: L.zngamd_inflate_batch_dev(h, d, dl, t, n, w, co, o, oc, res), count_only, wbits)
        nulld = dev_inflate(lambda d, dl, t, w, co, o, oc, res: L.zngamd_inflate_batch_dict_dev(h, d, dl, t, n, w, None, 0, co, o, oc, res),
                            count_only, wbits)
        assert plain == nulld, (count_only, wbits)
        if (count_only, wbits) == (0, 31):
            st = np.frombuffer(plain[3], np.uint32).reshape(-1, 4)[:, 0]
            assert [k for k in range(n) if st[k] != _lib.BATCH_OK] == [3, 7, 11]
            assert plain[2][:room] == b"".join(x for k, x in enumerate(items) if k not in (3, 7, 11))
    assert plain[0] == _lib.STREAM_ERROR and plain[1] == "invalid wbits"

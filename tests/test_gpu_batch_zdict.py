"""The batch API with a shared preset dictionary on the GPU (zlib_ng_amd.batch, zdict=...): every item against the stream objects,
with CPython's zlib as referee -- byte identity with compressobj(zdict=...), foreign streams, every error class in one call against
decompressobj(zdict=...), the count pass, large items, sub-batches, the device-resident forms, a hostile device table and the ratio
a dictionary buys on small records."""
import json
import random
import struct
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from zlib_ng_amd import _lib, batch, corpus, devmem, zlib_ng
    return _lib, batch, corpus, devmem, zlib_ng


def _stream(zlib_ng, item, level, wbits, strategy, zdict):
    c = zlib_ng.compressobj(level, zlib_ng.DEFLATED, wbits, zlib_ng.DEF_MEM_LEVEL, strategy, zdict)
    return c.compress(item) + c.flush()


def _reference(zlib_ng, item, wbits, zdict):
    """decompressobj(wbits, zdict) and an unfinished stream is an error -> bytes or the exception"""
    try:
        o = zlib_ng.decompressobj(wbits, zdict=zdict)
        out = o.decompress(item)
        if not o.eof:
            raise zlib_ng.error("Error -5 while decompressing data: incomplete or truncated stream")
        return out
    except Exception as e:
        return e


def _json_lines(n_bytes, seed):
    """records of a seeded JSON-lines generator (log-like events)"""
    rng = random.Random(seed)
    users = [f"user{rng.randrange(10 ** 6):06d}" for _ in range(300)]
    paths = ["/api/v1/items", "/api/v1/orders", "/login", "/static/app.js", "/api/v2/search", "/health", "/cart"]
    agents = ["Mozilla/5.0 (X11; Linux x86_64)", "curl/8.4.0", "python-requests/2.31", "Mozilla/5.0 (Macintosh; Intel Mac OS X 14_1)"]
    out, size = [], 0
    while size < n_bytes:
        rec = {"ts": 1_700_000_000 + rng.randrange(10 ** 7), "level": rng.choice(["INFO", "INFO", "INFO", "WARN", "ERROR"]),
               "user": rng.choice(users), "method": rng.choice(["GET", "GET", "POST", "PUT"]), "path": rng.choice(paths),
               "status": rng.choice([200, 200, 200, 201, 304, 404, 500]), "ms": round(rng.expovariate(1 / 40), 2),
               "agent": rng.choice(agents), "region": rng.choice(["eu-west-1", "us-east-1", "ap-south-1"])}
        line = json.dumps(rec).encode() + b"\n"
        out.append(line)
        size += len(line)
    return b"".join(out)


@pytest.fixture(scope="module")
def text(mods):
    return mods[2].text(4 << 20, seed=21).tobytes()


def _dicts(text):
    return {1: text[7:8], 100: text[1000:1100], 4096: text[5000:9096], 32768: text[20000:52768], 40000: text[60000:100000]}


def _items(text, d):
    """items of the grid's sizes, some of them repeating dictionary content"""
    sizes = [0, 1, 100, 4096, 131071, 131072, 131073, 1 << 20]
    out = []
    for k, s in enumerate(sizes):
        o = 200000 + 37 * k * 4099
        out.append(text[o:o + s])
    rep = (d * (1 + 5000 // max(1, len(d))))[:5000]
    out += [rep, d[-min(len(d), 3000):] + text[:1000], (d * (1 + 200000 // max(1, len(d))))[:200000]]
    return out


@pytest.mark.parametrize("wbits", [15, 9, -15, -9])
def test_compress_is_the_stream_byte_for_byte(mods, text, wbits):
    _lib, batch, corpus, devmem, zlib_ng = mods
    for dl, d in _dicts(text).items():
        items = _items(text, d)
        for level in (0, 1, 6, 9):
            out = batch.compress(items, level, wbits, zdict=d)
            assert len(out) == len(items)
            for i, (a, b) in enumerate(zip(items, out)):
                assert b == _stream(zlib_ng, a, level, wbits, 0, d), (dl, level, i, len(a))
                o = zlib.decompressobj(wbits, zdict=d)
                assert o.decompress(b) == a and o.eof, (dl, level, i)
    # an empty dictionary: FDICT with the DICTID of nothing (zlib), no history
    items = _items(text, b"")
    for level in (1, 6):
        out = batch.compress(items, level, wbits, zdict=b"")
        for a, b in zip(items, out):
            assert b == _stream(zlib_ng, a, level, wbits, 0, b"")
            o = zlib.decompressobj(wbits, zdict=b"")
            assert o.decompress(b) == a and o.eof
    if wbits > 0:
        assert out[0][1] & 0x20 and out[0][2:6] == b"\0\0\0\1"


@pytest.mark.parametrize("strategy", [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
def test_strategies_with_a_dictionary(mods, text, strategy):
    _lib, batch, corpus, devmem, zlib_ng = mods
    d = _dicts(text)[32768]
    items = _items(text, d)
    for wbits in (15, -15):
        out = batch.compress(items, 6, wbits, strategy=strategy, zdict=d)
        for a, b in zip(items, out):
            assert b == _stream(zlib_ng, a, 6, wbits, strategy, d)
            o = zlib.decompressobj(wbits, zdict=d)
            assert o.decompress(b) == a and o.eof


def test_none_dictionary_changes_nothing(mods, text):
    _lib, batch, corpus, devmem, zlib_ng = mods
    items = _items(text, b"xyz")
    for wbits in (15, 31, -15):
        assert batch.compress(items, 6, wbits, zdict=None) == batch.compress(items, 6, wbits) == [zlib_ng.compress(x, 6, wbits) for x in items]


def test_decompress_foreign_streams(mods, text):
    _lib, batch, corpus, devmem, zlib_ng = mods
    rng = random.Random(5)
    d = _dicts(text)[40000]
    pairs = {15: [], -15: []}
    for i in range(300):
        s = rng.choice([0, 1, 50, 1000, 4096, 20000])
        o = rng.randrange(0, len(text) - s + 1)
        x = text[o:o + s] if i % 3 else d[rng.randrange(0, 30000):][:s] + text[o:o + s // 2]
        level = (1, 6, 9)[i % 3]
        for wbits in (15, -15):
            co = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, 0, d)
            pairs[wbits].append((x, co.compress(x) + co.flush()))
    for wbits, ps in pairs.items():
        out = batch.decompress([p[1] for p in ps], wbits, zdict=d)
        assert out == [p[0] for p in ps]
        for (x, c), o in zip(ps[:40], out[:40]):
            assert o == _reference(zlib_ng, c, wbits, d)
    # auto-detect: zlib items with FDICT beside gzip items (which ignore the dictionary)
    mix = [(x, c) for x, c in pairs[15][:100]]
    for i in range(100):
        x = text[i * 777:i * 777 + 2000 + i]
        g = zlib.compressobj(6, zlib.DEFLATED, 31)
        mix.append((x, g.compress(x) + g.flush()))
    rng.shuffle(mix)
    for wbits in (47, 32):
        out = batch.decompress([p[1] for p in mix], wbits, zdict=d)
        assert out == [p[0] for p in mix]


def test_every_error_class_in_one_call(mods, text):
    _lib, batch, corpus, devmem, zlib_ng = mods
    d = _dicts(text)[32768]
    x = d[5000:15000] + text[:10000]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, d)
    good = co.compress(x) + co.flush()
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, d[:-1])
    wrong = co.compress(x) + co.flush()                          # written with another dictionary
    plain = zlib.compress(text[:20000], 6)
    # a zlib item without FDICT whose data refers back before its start (a raw stream written with the dictionary, zlib-framed)
    co = zlib.compressobj(6, zlib.DEFLATED, -15, 8, 0, d)
    body = co.compress(x) + co.flush()
    far = b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(x))
    items = [
        good, plain, wrong,
        good[:4], good[:2], good[:6],                            # cut inside the DICTID, right after the header, at its end
        far,
        good[:len(good) // 2], good[len(good) // 2:],
        good[:40] + bytes([good[40] ^ 0x10]) + good[41:],
        good[:-1] + bytes([good[-1] ^ 1]),
        b"\x78\x9d" + good[2:], b"\x78", b"", plain[:-2], good + b"trailing bytes",
    ]
    classes = set()
    for zd in (d, None):
        got = batch.decompress(items, 15, errors="return", zdict=zd)
        first = None
        for i, (c, g) in enumerate(zip(items, got)):
            want = _reference(zlib_ng, c, 15, zd if zd is not None else b"") if zd is not None else None
            if zd is None:
                try:
                    want = zlib_ng.decompress(c, 15)
                except Exception as e:
                    want = e
            if isinstance(want, Exception):
                assert type(g) is type(want) and str(g) == str(want), (zd is None, i, g, want)
                assert g.index == i
                first = i if first is None else first
                classes.add(str(want))
            else:
                assert g == want, (zd is None, i)
        with pytest.raises(zlib_ng.error) as ei:
            batch.decompress(items, 15, zdict=zd)
        assert ei.value.index == first
    assert "Error -3 while setting zdict: invalid input data" in classes
    assert "Error 2 while decompressing data" in classes                      # FDICT and no dictionary
    assert "Error -5 while decompressing data: incomplete or truncated stream" in classes
    assert "Error -3 while decompressing data: invalid input data" in classes
    assert "Error -3 while decompressing data: incorrect data check" in classes
    assert "Error -3 while decompressing data: incorrect header check" in classes
    # raw items: the dictionary is history; without it the same item refers before its start
    got = batch.decompress([body, body[:-3]], -15, errors="return", zdict=d)
    assert got[0] == x and "truncated" in str(got[1])
    assert "invalid input data" in str(batch.decompress([body], -15, errors="return")[0])
    # an empty dictionary leaves today's behaviour: FDICT items need one
    assert str(batch.decompress([good], 15, errors="return", zdict=b"")[0]) == "Error 2 while decompressing data"


def test_count_pass_and_large_items(mods, text):
    _lib, batch, corpus, devmem, zlib_ng = mods
    d = _dicts(text)[32768]
    rnd = np.random.default_rng(3).integers(0, 256, 1 << 20, dtype=np.uint8).tobytes()
    datas = [text[i * 1024:(i + 1) * 1024] for i in range(30)]
    datas[5] = (d[-20000:] * 105)[:2 << 20]             # mostly the dictionary repeated: overflows the first room guess
    datas[9] = (d[-20000:] * 40)[:700000]
    datas[20] = rnd + d                                 # above the large-item threshold compressed
    for wbits in (15, -15):
        comp = []
        for x in datas:
            co = zlib.compressobj(6, zlib.DEFLATED, wbits, 8, 0, d)
            comp.append(co.compress(x) + co.flush())
        assert len(comp[20]) >= batch.LARGE_ITEM and len(comp[5]) * 4 + 1024 < len(datas[5])
        assert batch.decompress(comp, wbits, zdict=d) == datas
    # compress: an item at the stream's direct-piece size goes through compressobj
    big = (text * 9)[:batch.ZS_BATCH + 12345]
    out = batch.compress([b"small", big, d], 6, 15, zdict=d)
    assert out[1] == _stream(zlib_ng, big, 6, 15, 0, d)
    assert out[0] == _stream(zlib_ng, b"small", 6, 15, 0, d) and out[2] == _stream(zlib_ng, d, 6, 15, 0, d)
    assert batch.decompress(out, 15, zdict=d) == [b"small", big, d]


def test_sub_batches_give_the_same_results(mods, text, monkeypatch):
    _lib, batch, corpus, devmem, zlib_ng = mods
    d = _dicts(text)[40000]
    rng = random.Random(12)
    items = [text[o:o + s] for o, s in ((rng.randrange(1 << 21), rng.choice([0, 1, 700, 5000, 40000])) for _ in range(300))]
    c_whole = batch.compress(items, 6, 15, zdict=d)
    d_whole = batch.decompress(c_whole, 15, zdict=d)
    monkeypatch.setattr(batch, "SUB_BATCH_BYTES", 100000)
    assert batch.compress(items, 6, 15, zdict=d) == c_whole
    assert batch.decompress(c_whole, 15, zdict=d) == d_whole == items


def test_device_forms_round_trip_in_hbm(mods, text):
    _lib, batch, corpus, devmem, zlib_ng = mods
    ctx = _lib.default_context()
    d = _dicts(text)[32768]
    rng = random.Random(11)
    items = [text[o:o + s] for o, s in ((rng.randrange(1 << 21), rng.choice([0, 1, 100, 1000, 4096, 70000, 131073])) for _ in range(400))]
    lens = np.array([len(x) for x in items], dtype=np.uint64)
    offs = np.zeros(len(items), dtype=np.uint64)
    offs[1:] = np.cumsum(lens)[:-1]
    flat = b"".join(items)
    d_in = devmem.from_host(ctx, np.frombuffer(flat + bytes(_lib.BATCH_PAD), np.uint8))
    for wbits in (15, -15):
        d_c, coffs, clens = batch.compress_dev(ctx, d_in, offs, lens, 6, wbits, zdict=d)
        host_c = d_c.cpu().tobytes()
        for i in range(0, len(items), 23):
            assert host_c[int(coffs[i]):int(coffs[i] + clens[i])] == _stream(zlib_ng, items[i], 6, wbits, 0, d)
        total_c = int(coffs[-1] + clens[-1])
        d_cp = devmem.DeviceBuffer(ctx, total_c + _lib.BATCH_PAD)
        d_cp[:total_c] = d_c[:total_c]
        d_cp[total_c:] = 0
        d_out, ooffs, olens, st = batch.decompress_dev(ctx, d_cp, coffs, clens, wbits, zdict=d)
        assert (st == 0).all() and (olens == lens).all()
        assert d_out[:len(flat)].equal(d_in[:len(flat)])
        # without the dictionary the zlib items need one
        if wbits == 15:
            _, _, _, st2 = batch.decompress_dev(ctx, d_cp, coffs, clens, wbits)
            assert (st2 == _lib.BATCH_NEED_DICT).all()


def test_hostile_device_table_on_the_dictionary_path(mods, text):
    _lib, batch, corpus, devmem, zlib_ng = mods
    ctx = _lib.default_context()
    d = _dicts(text)[4096]
    x = text[:5000]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, d)
    good = co.compress(x) + co.flush()
    in_len = len(good)
    d_in = devmem.from_host(ctx, np.frombuffer(good + bytes(_lib.BATCH_PAD), np.uint8))
    G = 4096
    out_cap = 4 * 5000
    d_out = devmem.DeviceBuffer(ctx, out_cap + 2 * G)
    d_out[:] = 0xA5
    body = d_out[G:G + out_cap]
    M = 0xFFFFFFFF
    rows = [
        (0, 0, in_len, 5000),
        (1 << 40, 5000, in_len, 5000),
        (in_len - 10, 5000, 100, 5000),
        (0, out_cap - 100, in_len, 5000),
        (0, (1 << 64) - 16, in_len, 64),
        ((1 << 64) - 8, 5000, 16, 5000),
        (0, 5000, M, 5000),
        (0, 10000, in_len, 5000),
        (0, 15000, in_len, M),
    ]
    tab = np.array([[a, b, c | (e << 32), 0] for a, b, c, e in rows], dtype=np.uint64)
    d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
    d_res = devmem.DeviceBuffer(ctx, 16 * len(rows))
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, len(rows), 15, False, body.ptr, out_cap, d_res.ptr, zdict=d)
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)
    assert list(res[:, 0]) == [0, 12, 12, 12, 12, 12, 12, 0, 12]
    host = d_out.cpu().tobytes()
    assert host[:G] == b"\xa5" * G and host[G + out_cap:] == b"\xa5" * G
    assert host[G:G + 5000] == x and host[G + 10000:G + 15000] == x
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, len(rows), 15, True, None, 0, d_res.ptr, zdict=d)
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)
    assert res[0, 0] == 0 and res[0, 1] == 5000 and res[0, 2] == in_len and res[1, 0] == 12


def test_ratio_gate_on_small_json_records(mods):
    _lib, batch, corpus, devmem, zlib_ng = mods
    data = _json_lines(3 << 20, seed=77)
    d = data[:32768]                                    # the dictionary: records outside the batch
    body = data[1 << 20:]
    recs = [body[i:i + 1024] for i in range(0, 2000 * 1024, 1024)]
    plain = batch.compress(recs, 6, 15)
    primed = batch.compress(recs, 6, 15, zdict=d)
    tp, td = sum(map(len, plain)), sum(map(len, primed))
    assert td <= 0.80 * tp, (td, tp)
    assert batch.decompress(primed, 15, zdict=d) == recs

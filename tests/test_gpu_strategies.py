"""Compression strategies on the GPU engine (deflateInit2's strategy: Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED): every stream
round-trips through CPython's zlib, and the DEFLATE token walker (tests/deflate_walk.py) checks that it is the KIND of stream the
strategy asks for -- no match under Huffman-only, distance 1 only under RLE, no dynamic block under fixed, no match shorter than 6
under filtered.  The default strategy's output is unchanged."""
import ctypes as C
import os
import random
import zlib

import numpy as np
import pytest

import deflate_walk as W

pytestmark = pytest.mark.gpu

STRATS = [zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED]
NAMES = {zlib.Z_FILTERED: "filtered", zlib.Z_HUFFMAN_ONLY: "huffman", zlib.Z_RLE: "rle", zlib.Z_FIXED: "fixed"}


def run_heavy(n, seed=7):
    """random bytes, each repeated 1..400 times"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([rng.randrange(256)]) * rng.randint(1, 400)
    return bytes(out[:n])


@pytest.fixture(scope="module")
def Z():
    from zlib_ng_amd import zlib_ng
    return zlib_ng


@pytest.fixture(scope="module")
def inputs(fastq):
    from zlib_ng_amd import corpus
    n = 1 << 20
    return {"fastq": fastq[:n], "text": corpus.text(n, seed=11).tobytes(), "mixed": corpus.mixed(n, seed=12).tobytes(),
            "runs": run_heavy(n), "zeros": bytes(n), "random": os.urandom(n), "empty": b""}


@pytest.fixture(scope="module")
def big():
    """8 MiB of each generated corpus: the size the bounds were estimated on (a 1 MiB `mixed` has parts of 150 KB, and a 128 KiB
    unit -- one Huffman table -- straddles two kinds of data far more often than zlib's 16 K-symbol blocks do)"""
    from zlib_ng_amd import corpus
    n = 8 << 20
    return {"fastq": corpus.fastq(n, seed=2).tobytes(), "text": corpus.text(n, seed=11).tobytes(), "mixed": corpus.mixed(n, seed=12).tobytes()}


def _ours(Z, data, level, strategy, wbits=-15, zdict=None):
    c = Z.compressobj(level, Z.DEFLATED, wbits, 8, strategy, *((zdict,) if zdict is not None else ()))
    return c.compress(data) + c.flush()


def _check(stream, data, strategy, wbits=-15, window=b""):
    """round trip through the system zlib, then the walker's structural check"""
    if window:
        d = zlib.decompressobj(wbits, zdict=window)
        assert d.decompress(stream) + d.flush() == data
    else:
        assert zlib.decompress(stream, wbits) == data
    w = W.walk(W.strip_container(stream, wbits), window=window)
    assert w.out == data
    msg = W.check_strategy(w, strategy)
    assert msg is None, msg
    return w


@pytest.mark.parametrize("strategy", STRATS, ids=lambda s: NAMES[s])
@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("name", ["fastq", "text", "mixed", "runs", "zeros", "random", "empty"])
def test_strategy_streams(Z, inputs, name, level, strategy):
    data = inputs[name][:100_000]
    _check(_ours(Z, data, level, strategy), data, strategy)


@pytest.mark.parametrize("strategy", STRATS, ids=lambda s: NAMES[s])
@pytest.mark.parametrize("wbits", [-15, -9, 15, 31])
@pytest.mark.parametrize("size", [0, 1, 1000, 100_000, 1 << 20])
def test_strategy_sizes_and_windows(Z, inputs, size, wbits, strategy):
    data = (inputs["runs"][:size // 2] + inputs["mixed"][:size - size // 2])
    s = _ours(Z, data, 6, strategy, wbits)
    if size >= 1 << 20:
        assert zlib.decompress(s, wbits) == data          # (the walker is pure Python: the large size round-trips only ...)
        if wbits == -15:
            _check(s, data, strategy, wbits)             # (... and is walked once per strategy)
    else:
        _check(s, data, strategy, wbits)


@pytest.mark.parametrize("strategy", STRATS, ids=lambda s: NAMES[s])
@pytest.mark.parametrize("flush", [zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH])
def test_strategy_zdict_flushes_and_copy(Z, inputs, strategy, flush):
    zd = inputs["text"][500_000:520_000]
    data = inputs["text"][:60_000] + inputs["runs"][:30_000] + inputs["fastq"][:60_000]
    c = Z.compressobj(6, Z.DEFLATED, -15, 8, strategy, zd)
    s = c.compress(data[:50_000]) + c.flush(flush) + c.compress(data[50_000:100_000]) + c.flush(flush)
    c2 = c.copy()
    tail = c.compress(data[100_000:]) + c.flush()
    tail2 = c2.compress(data[100_000:]) + c2.flush()
    assert tail == tail2
    _check(s + tail, data, strategy, window=zd)


@pytest.mark.parametrize("strategy,k", [(zlib.Z_HUFFMAN_ONLY, 1.03), (zlib.Z_RLE, 1.03), (zlib.Z_FIXED, 1.02), (zlib.Z_FILTERED, 1.03)],
                         ids=lambda v: NAMES.get(v, str(v)))
@pytest.mark.parametrize("name", ["fastq", "text", "mixed"])
def test_strategy_size_against_zlib(Z, big, name, strategy, k):
    data = big[name]
    ours = _ours(Z, data, 6, strategy)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
    ref = c.compress(data) + c.flush()
    assert len(ours) <= k * len(ref), (name, NAMES[strategy], len(ours) / len(ref))


def test_rle_finds_runs(Z, inputs):
    data = inputs["runs"]
    rle, huf = _ours(Z, data, 6, zlib.Z_RLE), _ours(Z, data, 6, zlib.Z_HUFFMAN_ONLY)
    assert len(rle) < len(huf) / 2, (len(rle), len(huf))


@pytest.mark.parametrize("level", [1, 6, 9])
def test_default_strategy_unchanged(Z, ctx, inputs, level):
    data = inputs["text"][:300_000] + inputs["runs"][:100_000]
    assert _ours(Z, data, level, zlib.Z_DEFAULT_STRATEGY) == (lambda c: c.compress(data) + c.flush())(Z.compressobj(level, Z.DEFLATED, -15))
    B = 131072
    blocks = [(o, min(B, len(data) - o), min(o, 32768), 0) for o in range(0, len(data), B)]
    a = ctx.deflate_blocks(data, blocks, level, B + B // 8)
    b = ctx.deflate_blocks(data, blocks, level, B + B // 8, strategy=0)
    assert a == b


@pytest.mark.parametrize("strategy", STRATS, ids=lambda s: NAMES[s])
def test_strategies_differ_from_default(Z, inputs, strategy):
    """the strategy is honoured, not accepted and ignored"""
    data = inputs["fastq"][:200_000]
    assert _ours(Z, data, 6, strategy) != _ours(Z, data, 6, zlib.Z_DEFAULT_STRATEGY)


class Dev:
    def __init__(self, ctx, nbytes):
        self.ctx, self.n = ctx, nbytes
        self.p = C.c_void_p()
        assert ctx.L.zngamd_dmalloc(ctx.h, max(nbytes, 1), C.byref(self.p)) == 0

    def put(self, data):
        buf = bytes(data)
        assert self.ctx.L.zngamd_h2d(self.ctx.h, self.p, C.cast(C.c_char_p(buf), C.c_void_p), len(buf)) == 0

    def get(self, nbytes=None, dtype=np.uint8):
        nbytes = self.n if nbytes is None else nbytes
        out = np.empty(nbytes, np.uint8)
        assert self.ctx.L.zngamd_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.p, nbytes) == 0
        return out.view(dtype)

    def free(self):
        self.ctx.L.zngamd_dfree(self.ctx.h, self.p)


def _blocks_ok(outs, crcs, data, cuts, strategy):
    for (o, n, dl, _), out, crc in zip(cuts, outs, crcs):
        d = zlib.decompressobj(-15, zdict=data[o - dl:o]) if dl else zlib.decompressobj(-15)
        assert d.decompress(out) == data[o:o + n] and crc == zlib.crc32(data[o:o + n])
        if n <= 131072:
            msg = W.check_strategy(W.walk(out, window=data[o - dl:o]), strategy)
            assert msg is None, msg


@pytest.mark.parametrize("strategy", [zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY])
def test_engine_blocks_direct(ctx, inputs, strategy):
    """Context.deflate_blocks(strategy=...) over many 128 KiB blocks -- independent and dictionary-primed, odd sizes -- through
    the per-block call, the packed (joined) call, and the device-resident slot and packed entry points"""
    from zlib_ng_amd import _lib
    B = 131072
    data = inputs["runs"][:6 * B] + inputs["fastq"][:6 * B] + inputs["zeros"][:B] + inputs["mixed"][:3 * B + 777]
    cuts = [(o, min(B, len(data) - o), (32768 if (o // B) % 2 else 0) if o else 0, 0) for o in range(0, len(data), B)]
    outs, crcs, ovf = ctx.deflate_blocks(data, cuts, 6, B + B // 8, strategy=strategy)
    assert not ovf
    _blocks_ok(outs, crcs, data, cuts, strategy)
    joined, crcs2, ovf2, lens = ctx.deflate_blocks(data, cuts, 6, B + B // 8, joined=True, strategy=strategy)
    assert not ovf2 and bytes(joined) == b"".join(outs) and crcs2 == crcs
    # device resident: slots + gather, and packed
    arr, nb = _lib.with_strategy(_lib.block_table(cuts), strategy)
    L, h = ctx.L, ctx.h
    d_in = Dev(ctx, len(data) + 64); d_in.put(data + bytes(64))
    nu = L.zngamd_count_units(arr, nb)
    d_slots, d_len, d_crc = Dev(ctx, nu * _lib.SLOT_STRIDE), Dev(ctx, nu * 4), Dev(ctx, nu * 4)
    assert L.zngamd_deflate_blocks_dev(h, d_in.p, len(data), arr, nb, 6, d_slots.p, d_len.p, d_crc.p, None) == 0, ctx.err()
    lens_d = d_len.get(dtype=np.uint32)
    slots = d_slots.get()
    got = [slots[u * _lib.SLOT_STRIDE:u * _lib.SLOT_STRIDE + int(lens_d[u])].tobytes() for u in range(nu)]
    assert got == outs
    d_pk, d_len2, d_crc2 = Dev(ctx, len(data) + nu * 64 + 64), Dev(ctx, nu * 4), Dev(ctx, nu * 4)
    total = C.c_uint64(0)
    assert L.zngamd_deflate_blocks_packed_dev(h, d_in.p, len(data), arr, nb, 6, d_pk.p, d_pk.n, d_len2.p, d_crc2.p, None,
                                              C.byref(total)) == 0, ctx.err()
    assert d_pk.get(total.value).tobytes() == b"".join(outs)
    for d in (d_in, d_slots, d_len, d_crc, d_pk, d_len2, d_crc2):
        d.free()

"""The referee and the inputs of the checksum tests, and the host-side CRC folds of the library (no GPU): zlib's crc32 / adler32
against a bytewise restatement on every pattern; no pattern degenerate enough for a wrong kernel to match it by accident;
zngamd_crc32_combine / _combine_many against zlib on concatenations and against a Python-int polynomial referee at lengths
that cannot be materialised."""
import ctypes as C
import zlib

import pytest

import checksum_inputs as K

SMALL = [n for n in K.ALL_LENS if n <= 4097]


@pytest.fixture(scope="module")
def L():
    from zlib_ng_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_referee_is_zlib(name):
    """zlib.crc32 / adler32 == the bytewise restatement, every seed, every list length up to 4 097 (and the needles)"""
    for n in SMALL:
        datas = [K.PATTERNS[name](n)]
        if name == "zero":
            datas += [K.needle(n, k) for k in K.needle_positions(n, 64)]
        for d in datas:
            assert len(d) == n
            for s in K.CRC_SEEDS:
                assert zlib.crc32(d, s) == K.crc32_bytewise(d, s), (name, n, s)
            for s in K.ADLER_SEEDS:
                assert zlib.adler32(d, s) == K.adler32_bytewise(d, s), (name, n, s)


def test_patterns_are_what_they_say():
    n = 70000
    assert set(K.ff(n)) == {255} and set(K.zero(n)) == {0}
    assert min(K.high(n)) == 128 and max(K.high(n)) == 255 and len(set(K.high(n))) == 128
    assert min(K.rand(n)) == 0 and max(K.rand(n)) == 255
    assert K.ramp(600) == bytes((131 * i + 7) % 256 for i in range(600))
    assert K.high(1000) == K.high(n)[:1000] and K.rand(n) is not K.high(n) and K.rand(n) != K.high(n)
    assert K.needle(100, 37) == bytes(37) + b"\x01" + bytes(62)
    assert K.needle_positions(16384, 64) == [0, 63, 64, 16384 - 65, 16384 - 64, 16383]
    assert K.needle_positions(1, 64) == [0]
    # the needle's Adler-32: a = 1 + 1, b = n (the seed's 1, once a byte) + (n - k)
    for n, k in ((16384, 63), (131072, 131072 - 513)):
        assert zlib.adler32(K.needle(n, k)) == ((n + n - k) % 65521) << 16 | 2


@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_no_pattern_is_degenerate(name):
    """every pattern at every length: its sums differ from those of the same bytes with the last one XOR 1, and from those of its
    own first n - 1 bytes"""
    for n in K.ALL_LENS:
        d = K.PATTERNS[name](n)
        crc, ad = K.sums(name, n)
        flipped = d[:-1] + bytes([d[-1] ^ 1])
        assert zlib.crc32(flipped) != crc and zlib.adler32(flipped) != ad, (name, n)
        assert zlib.crc32(d[:-1]) != crc and zlib.adler32(d[:-1]) != ad, (name, n)


def test_combine_reference_is_zlib():
    """the polynomial referee on lengths that can be materialised"""
    for nb in (0, 1, 7, 2047, 2048, 131073):
        a, b = K.rand(1000), K.high(nb)
        assert K.crc32_combine_ref(zlib.crc32(a), zlib.crc32(b), nb) == zlib.crc32(a + b), nb


@pytest.mark.parametrize("name", list(K.PATTERNS))
def test_crc32_combine_vs_concatenation(L, name):
    f = K.PATTERNS[name]
    for na in (1, 77, 131073):
        for nb in (0, 1, 2047, 2048, 131072, 131073):
            a, b = f(na), f(na + nb)[na:]
            assert L.zngamd_crc32_combine(zlib.crc32(a), zlib.crc32(b), nb) == zlib.crc32(a + b), (name, na, nb)


def test_crc32_combine_beyond_memory(L):
    """lengths of 2^32, 2^32 + 1 and 2^40 + 3 (a len2 cut to 32 bits would give the answers for 0, 1 and 3)"""
    for c1 in (0, 1, 0xFFFFFFFF, 0x80000000, zlib.crc32(K.rand(100))):
        for c2 in (0, 0xDEADBEEF):
            for n in (2 ** 32, 2 ** 32 + 1, 2 ** 40 + 3):
                want = K.crc32_combine_ref(c1, c2, n)
                assert L.zngamd_crc32_combine(c1, c2, n) == want, (c1, c2, n)
                if c1:
                    assert want != K.crc32_combine_ref(c1, c2, n & 0xFFFFFFFF)


def test_crc32_combine_is_associative(L):
    comb = L.zngamd_crc32_combine
    for name, f in K.PATTERNS.items():
        d = f(2049 + 131073 + 33)
        p = [d[:2049], d[2049:2049 + 131073], d[2049 + 131073:]]
        c = [zlib.crc32(x) for x in p]
        left = comb(comb(c[0], c[1], len(p[1])), c[2], len(p[2]))
        right = comb(c[0], comb(c[1], c[2], len(p[2])), len(p[1]) + len(p[2]))
        assert left == right == zlib.crc32(d), name
    # the same at lengths beyond memory, against the referee
    a, b, c = 0x12345678, 0x9ABCDEF0, 0x0F1E2D3C
    n2, n3 = 2 ** 32 + 1, 2 ** 40 + 3
    left = comb(comb(a, b, n2), c, n3)
    assert left == comb(a, comb(b, c, n3), n2 + n3) == K.crc32_combine_ref(K.crc32_combine_ref(a, b, n2), c, n3)


@pytest.mark.parametrize("pieces", [1, 2, 513])
def test_crc32_combine_many(L, pieces):
    """1, 2 and 513 pieces of mixed lengths, empty ones among them: successive combines, and zlib of the concatenation"""
    lens = [(0, 1, 2047, 2048, 4097, 77, 0, 131073 if i == 200 else 31)[i % 8] for i in range(pieces)]
    if pieces == 1:
        lens = [2049]
    for name in ("high", "rand", "zero"):
        d = K.PATTERNS[name](100 + sum(lens))
        head, parts, at = d[:100], [], 100
        for n in lens:
            parts.append(d[at:at + n])
            at += n
        crcs = (C.c_uint32 * pieces)(*[zlib.crc32(x) for x in parts])
        ln = (C.c_uint64 * pieces)(*lens)
        start = zlib.crc32(head)
        got = L.zngamd_crc32_combine_many(start, C.cast(crcs, C.c_void_p), ln, pieces)
        step = start
        for x, n in zip(crcs, lens):
            step = L.zngamd_crc32_combine(step, x, n)
        assert got == step == zlib.crc32(d), (name, pieces)
        from zlib_ng_amd import _lib
        assert _lib.crc32_combine_many(start, list(crcs), lens) == got

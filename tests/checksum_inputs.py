"""Inputs of the checksum tests (tests/test_cpu_checksum_inputs.py pins them, tests/test_gpu_checksum_seams.py feeds them to every
CRC-32 / Adler-32 implementation of the engine).  Patterns are functions of a length; the length lists are, per geometry, the
smallest shapes at which that code can still go wrong: around every segment size, span size and threshold between two paths."""
import functools
import zlib

import numpy as np

RNG_SEED = 0x5EA75


# ---- patterns
@functools.lru_cache(maxsize=None)
def _random(lo, n):
    return np.random.default_rng(RNG_SEED + lo).integers(lo, 256, size=n, dtype=np.uint8).tobytes()


def ff(n):
    return b"\xff" * n


def zero(n):
    """its CRC depends on the length alone: the x^(8 len) factors of every fold"""
    return bytes(n)


def high(n):
    """random bytes in 128 .. 255: a byte taken as signed, a sum that only fits for small bytes"""
    return _random(128, 1 << 19)[:n] if n <= 1 << 19 else _random(128, n)


def rand(n):
    return _random(0, 1 << 19)[:n] if n <= 1 << 19 else _random(0, n)


@functools.lru_cache(maxsize=None)
def _ramp(n):
    return ((131 * np.arange(n, dtype=np.uint64) + 7) % 256).astype(np.uint8).tobytes()


def ramp(n):
    """(131 i + 7) mod 256: no two segments are alike"""
    return _ramp(1 << 19)[:n] if n <= 1 << 19 else _ramp(n)


def needle(n, k):
    """zeros with 0x01 at k: Adler's b is n - k plus the seed's terms, an "after" count off by one shows as a difference of one"""
    b = bytearray(n)
    b[k] = 1
    return bytes(b)


PATTERNS = {"ff": ff, "zero": zero, "high": high, "rand": rand, "ramp": ramp}

# ---- seeds
CRC_SEEDS = (0, 1, 0xFFFFFFFF, 0x80000000)
ADLER_SEEDS = (1, 0, 0xFFF0FFF0, 0xFFFFFFFF)        # both halves 65 520; both halves unreduced

# ---- lengths, one list per geometry
# za_k_checksum: spans of 128 KiB, a thread takes 64 << j bytes (j = 0 .. 3) with 256 threads covering the span
CK_LENS = (1, 15, 16, 17, 63, 64, 65, 16383, 16384, 16385, 32767, 32768, 32769, 65535, 65536, 65537,
           131071, 131072, 131073, 262145, 3 * 131072 + 77)
CK_OFFSETS = (0, 1, 3, 8, 15)                        # misalignment of a device pointer
CK_OFFSET_LENS = (1, 14, 15, 16, 17, 47, 16385, 131072, 131073)
CK_NEEDLE = {64: 16384, 128: 32768, 256: 65536, 512: 131072}      # a length that selects the thread's piece of s bytes
# za_wave_crc32: a lane per 2 KiB
SEG2K_LENS = (1, 3, 4, 5, 2047, 2048, 2049, 4095, 4096, 4097, 129024, 131071, 131072)
# the parse kernels' CRC: segments of 1 << s, s = 5 .. 11, the thresholds 64 << s with their neighbours
SSHIFT_LENS = (1, 31, 32, 33, 2047, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 65536, 65537, 131072)
# za_k_inflate_members: a lane owns 32 bytes of every 2 KiB
LANE32_LENS = (1, 31, 32, 33, 2015, 2016, 2017, 2047, 2048, 2049, 2080, 2081, 4095, 4096, 65535, 65536, 131072)
# za_wave_adler32: rounds of 64 KiB, a lane per KiB
ADLER1K_LENS = (1, 3, 4, 5, 1023, 1024, 1025, 65535, 65536, 65537, 131073)

ALL_LENS = tuple(sorted(set(CK_LENS + CK_OFFSET_LENS + SEG2K_LENS + SSHIFT_LENS + LANE32_LENS + ADLER1K_LENS)))


def needle_positions(n, s):
    """positions of the needle for a length n and a segment size s"""
    return sorted({min(max(k, 0), n - 1) for k in (0, s - 1, s, n - s - 1, n - s, n - 1)})


# ---- referees
def _crc_table():
    tab = []
    for c in range(256):
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
        tab.append(c)
    return tab


_CRC_TABLE = _crc_table()


def crc32_bytewise(data, value=0):
    """CRC-32 (reflected, 0xEDB88320) byte by byte"""
    c = (value & 0xFFFFFFFF) ^ 0xFFFFFFFF
    for d in data:
        c = _CRC_TABLE[(c ^ d) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32_bytewise(data, value=1):
    """Adler-32 byte by byte; the seed's halves are taken as they come, unreduced ones too (zlib does the same)"""
    a, b = value & 0xFFFF, (value >> 16) & 0xFFFF
    for d in data:
        a = (a + d) % 65521
        b = (b + a) % 65521
    return b << 16 | a


_POLY = 0x104C11DB7                                  # x^32 + ... + 1, bit k = the coefficient of x^k


def _reflect(v):
    return int("{:032b}".format(v & 0xFFFFFFFF)[::-1], 2)


def _polymod(v):
    while v.bit_length() > 32:
        v ^= _POLY << (v.bit_length() - 33)
    return v


def _polymul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        b >>= 1
    return _polymod(r)


def crc32_combine_ref(crc1, crc2, len2):
    """crc(A || B) from crc(A), crc(B) and |B|, on Python ints as polynomials over GF(2) in the natural bit order (a CRC value is
    the reflection of its polynomial): crc1 * x^(8 len2) mod P, plus crc2.  The pre- and post-inversions cancel: both values carry
    them, and the inverted start of B is what A's would have become."""
    e, sq, xp = 8 * len2, 2, 1                       # x^e by square and multiply
    while e:
        if e & 1:
            xp = _polymul(xp, sq)
        sq = _polymul(sq, sq)
        e >>= 1
    return _reflect(_polymul(_reflect(crc1), xp)) ^ (crc2 & 0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def sums(name, n):
    """(zlib.crc32, zlib.adler32) of a pattern at a length, from the seeds 0 and 1: computed once, shared"""
    d = PATTERNS[name](n)
    return zlib.crc32(d), zlib.adler32(d)

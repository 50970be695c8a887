"""The referee of the block finder of the chunk-parallel inflate (za_k_find_blocks_a / _b): where in a buffer could a non-final
dynamic block start?  Written from RFC 1951 and from what zlib's inflate accepts (inflate.c, inftrees.c), over an explicit bit
array; it shares no code and no layout with the kernels.  Holds no test and no GPU code.  Not a conftest.

    phase_a(buf)            every bit offset with BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, a COMPLETE code-length code
                            (Kraft sum of the HCLEN + 4 three-bit lengths exactly 1; a length of 0 adds nothing), and at least
                            12 bytes of buffer from the offset's byte on
    phase_b(buf, bit)       the HLIT + 257 + HDIST + 1 lengths decode: no repeat of a previous length without one, no run past
                            the end, symbol 256 has a code, the literal/length set is complete or one code of one bit, the
                            distance set is empty, complete or one code of one bit
    candidates(buf, start)  the sorted set of phase-B offsets, with the start bit

The finder kernel does not look at the last 16 bytes of a buffer; tail_is_quiet() is what every test vector must satisfy so that
the two can be compared count by count."""
import numpy as np

import deflate_build as B

TAIL = 64


def _bits(buf):
    return np.unpackbits(np.frombuffer(bytes(buf), np.uint8), bitorder="little")


def phase_a(buf):
    n = len(buf)
    if n < 12:
        return []
    bits = np.concatenate([_bits(buf), np.zeros(96, np.uint8)])
    nb = 8 * (n - 12) + 8                                # offsets whose byte has 12 bytes from it on

    def field(off, w):
        v = np.zeros(nb, np.uint32)
        for i in range(w):
            v |= bits[off + i: off + i + nb].astype(np.uint32) << i
        return v
    ok = field(0, 3) == 4                                # BFINAL 0, then BTYPE = 2 least significant bit first
    ok &= (field(3, 5) <= 29) & (field(8, 5) <= 29)
    hclen = field(13, 4) + 4
    kraft = np.zeros(nb, np.uint32)                      # in units of 2^-7: the lengths have three bits
    for j in range(19):
        ln = field(17 + 3 * j, 3)
        kraft += np.where((j < hclen) & (ln > 0), 128 >> ln, 0).astype(np.uint32)
    ok &= kraft == 128
    return [int(p) for p in np.flatnonzero(ok)]


class _Reader:
    def __init__(self, bits, pos):
        self.bits, self.pos = bits, pos

    def take(self, n):
        if self.pos + n > len(self.bits):
            raise EOFError
        v = 0
        for i in range(n):
            v |= int(self.bits[self.pos + i]) << i
        self.pos += n
        return v


def _phase_b(bits, bit):
    r = _Reader(bits, bit + 3)
    try:
        nlen, ndist, ncode = r.take(5) + 257, r.take(5) + 1, r.take(4) + 4
        cl = [0] * 19
        for k in range(ncode):
            cl[B.CLORDER[k]] = r.take(3)
        decode = {c: s for s, c in enumerate(B.canonical(cl)) if c is not None}          # (code, nbits) -> symbol
        lens = []
        while len(lens) < nlen + ndist:
            if r.pos + 7 > len(bits):                    # (a symbol of the code-length code may take seven bits)
                return False
            code = 0
            for nb in range(1, 8):
                code = (code << 1) | r.take(1)
                if (code, nb) in decode:
                    break
            else:
                return False
            sym = decode[(code, nb)]
            if sym < 16:
                run, val = 1, sym
            elif sym == 16:
                if not lens:
                    return False
                run, val = 3 + r.take(2), lens[-1]
            elif sym == 17:
                run, val = 3 + r.take(3), 0
            else:
                run, val = 11 + r.take(7), 0
            if len(lens) + run > nlen + ndist:
                return False
            lens += [val] * run
    except EOFError:
        return False
    ll, d = lens[:nlen], lens[nlen:]
    if not ll[256]:
        return False
    one = lambda s: B.kraft(s) < 32768 and max(s) == 1                     # zlib: an incomplete set is a single code of one bit
    if not (B.kraft(ll) == 32768 or one(ll)):
        return False
    return not any(d) or B.kraft(d) == 32768 or one(d)


def phase_b(buf, bit):
    return _phase_b(_bits(buf), bit)


def survivors(buf):
    """-> (phase-A offsets, those of them that pass phase B), both sorted"""
    bits = _bits(buf)
    a = phase_a(buf)
    return a, [p for p in a if _phase_b(bits, p)]


def candidates(buf, start_bit=0):
    return sorted(set(survivors(buf)[1]) | {start_bit})


def tail_is_quiet(buf, a=None):
    """no phase-A offset in the last TAIL bytes: the kernel and the referee then saw the same offsets"""
    a = phase_a(buf) if a is None else a
    return len(buf) >= TAIL and not any(p >= 8 * (len(buf) - TAIL) for p in a)


_described = {}


def describe(name, blocks, blob):
    """What the tests hold the finder and the host's chain against, computed once per vector and process:
    (phase-A offsets, candidates with the start bit, the chunks of the true chain by the host's rule)"""
    if name not in _described:
        a, b = survivors(blob)
        cands = sorted(set(b) | {0})
        chunks = B.chain_chunks(blocks, set(cands) & set(B.block_bits(blocks)[0]))
        _described[name] = (a, cands, chunks)
    return _described[name]

"""A small DEFLATE (RFC 1951) stream BUILDER for the inflate tests: streams are written bit by bit from an explicit description, so a
test can feed the decoders what no ordinary encoder writes -- 15-bit codes, one-code and empty distance sets, length 258 spelled as
code 284 + 31, references that reach exactly the first byte of the history, hundreds of tiny blocks -- and headers that are INVALID
for one chosen reason.  The builder computes the plaintext itself, by replaying its own tokens over zdict + output; it never asks a
decoder.  tests/test_cpu_handbuilt_streams.py proves every vector against the system zlib (the referee) before any GPU test uses it
(tests/test_cpu_span_vectors.py the span vectors, tests/test_cpu_finder_vectors.py the finder vectors at the end of this file).
Holds no test and no GPU code.  Not a conftest: imported by the test files that use it, like deflate_walk.

A stream is a list of blocks: Stored, Fixed or Dynamic.  A block of the two compressed kinds carries a token list:
    an int 0..255               a literal
    M(length, dist[, code])     a match; `code` chooses the spelling of the length (258 is code 285, or code 284 with extra bits 31)
    Sym(s) / DSym(s)            the literal/length (distance) code of symbol s, nothing else: for defects such as symbol 286
    Code(code, nbits)           a raw Huffman code, first bit first (the unused code of a one-code set)
    Raw(value, nbits)           raw bits, least significant first
assemble() sets BFINAL on the last block, or on none: any vector's blocks can also be embedded in a longer stream."""
from collections import namedtuple

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_L = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8       # all 288: the fixed code has codes for 286 and 287, which no stream may use
FIXED_D = [5] * 32                                         # likewise 30 and 31

DATA = "DATA"         # `expect` of a stream that zlib must refuse with a data error

M = namedtuple("M", "length dist code", defaults=(None,))
Sym = namedtuple("Sym", "sym")
DSym = namedtuple("DSym", "sym")
Code = namedtuple("Code", "code nbits")
Raw = namedtuple("Raw", "value nbits")


class BitWriter:
    """Fields least significant bit first, Huffman codes most significant bit first, both packed from bit 0 of each byte."""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, nbits):
        self.bits(int(format(code & ((1 << nbits) - 1), "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw_bytes(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitlen(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """Canonical Huffman codes of a length list -> [(code, nbits) or None per symbol].  An over-subscribed list gives codes that do
    not fit their length; they are cut to it (such a header is refused before any code is read)."""
    mx = max(lengths) if lengths else 0
    count = [0] * (mx + 2)
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for ln in lengths:
        if ln:
            out.append((nxt[ln], ln))
            nxt[ln] += 1
        else:
            out.append(None)
    return out


def kraft(lengths):
    """Sum of 2^-len over the coded symbols, as a fraction of 2^15: 32768 = complete."""
    return sum(1 << (15 - ln) for ln in lengths if ln)


def complete_lengths(k):
    """Lengths of a complete code of k >= 2 symbols, as flat as possible, shortest first."""
    assert k >= 2
    top = (k - 1).bit_length()
    short = (1 << top) - k
    return [top - 1] * short + [top] * (k - short)


def length_code(length, code=None):
    """-> (symbol, extra value, extra bits) of a match length; code = force this length code (257..285)"""
    if code is None:
        code = 285 if length == 258 else 257 + max(i for i in range(28) if LBASE[i] <= length)
    i = code - 257
    extra = length - LBASE[i]
    assert 0 <= extra < (1 << LEXT[i]) or (extra == 0 and LEXT[i] == 0), (length, code)
    return code, extra, LEXT[i]


def dist_code(dist):
    i = max(i for i in range(30) if DBASE[i] <= dist)
    return i, dist - DBASE[i], DEXT[i]


class Stored:
    btype = 0

    def __init__(self, data, nlen=None):
        self.data, self.nlen = bytes(data), nlen         # nlen: the one's complement field as written (a defect), or None

    def write(self, w, final):
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.align()
        w.bits(len(self.data), 16)
        w.bits(len(self.data) ^ 0xFFFF if self.nlen is None else self.nlen, 16)
        w.raw_bytes(self.data)


class _Coded:
    def __init__(self, tokens, eob=True):
        self.tokens, self.eob = list(tokens), eob

    def _codes(self):
        raise NotImplementedError

    def _write_tokens(self, w):
        lc, dc = self._codes()
        for t in self.tokens + ([Sym(256)] if self.eob else []):
            if isinstance(t, int):
                w.code(*lc[t])
            elif isinstance(t, M):
                s, ev, eb = length_code(t.length, t.code)
                w.code(*lc[s])
                w.bits(ev, eb)
                d, dv, db = dist_code(t.dist)
                w.code(*dc[d])
                w.bits(dv, db)
            elif isinstance(t, Sym):
                w.code(*lc[t.sym])
            elif isinstance(t, DSym):
                w.code(*dc[t.sym])
            elif isinstance(t, Code):
                w.code(t.code, t.nbits)
            elif isinstance(t, Raw):
                w.bits(t.value, t.nbits)
            else:
                raise TypeError(t)


class Fixed(_Coded):
    btype = 1

    _fixed = []                                          # the two fixed codes, computed once

    def _codes(self):
        if not Fixed._fixed:
            Fixed._fixed += [canonical(FIXED_L), canonical(FIXED_D)]
        return Fixed._fixed

    def write(self, w, final):
        w.bits(1 if final else 0, 1)
        w.bits(1, 2)
        self._write_tokens(w)


def rle_lengths(lens):
    """The code-length sequence of a length list with the repeat codes, greedily: [(symbol, extra value)]"""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            r = min(run, 138)
            out.append((18, r - 11) if r >= 11 else (17, r - 3))
            i += r
        elif v and run >= 4:
            out.append((v, 0))
            r = min(run - 1, 6)
            out.append((16, r - 3))
            i += 1 + r
        else:
            out.append((v, 0))
            i += 1
    return out


class Dynamic(_Coded):
    """ll / d: the literal/length and the distance code lengths (HLIT + 257 and HDIST + 1 of them).  Everything else has a default
    and can be forced: hlit / hdist / hclen = the header fields as written; clseq = the code-length sequence [(symbol, extra)], by
    default the lengths one by one (rle=False) or with repeat codes (rle=True); cl = the 19 lengths of the code-length code, by
    default a complete code over the symbols of clseq.  eob=False: no end-of-block code behind the tokens."""
    btype = 2

    def __init__(self, ll, d, tokens=(), eob=True, rle=False, clseq=None, cl=None, hlit=None, hdist=None, hclen=None):
        _Coded.__init__(self, tokens, eob)
        self.ll, self.d = list(ll), list(d)
        self.clseq = list(clseq) if clseq is not None else (rle_lengths(self.ll + self.d) if rle else [(v, 0) for v in self.ll + self.d])
        if cl is None:
            used = sorted({s for s, _ in self.clseq})
            if len(used) == 1:
                used = sorted(used + [0 if used[0] else 8])        # (a one-code code-length code is refused: a second, unused code)
            cl = [0] * 19
            for s, ln in zip(used, complete_lengths(len(used))):
                cl[s] = ln
        self.cl = list(cl)
        self.hlit = len(self.ll) - 257 if hlit is None else hlit
        self.hdist = len(self.d) - 1 if hdist is None else hdist
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CLORDER) if self.cl[s]])
        self.hclen = hclen

    def _codes(self):
        return canonical(self.ll), canonical(self.d)

    def write(self, w, final):
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(self.hlit, 5)
        w.bits(self.hdist, 5)
        w.bits(self.hclen - 4, 4)
        for s in CLORDER[:self.hclen]:
            w.bits(self.cl[s], 3)
        cc = canonical(self.cl)
        for s, ev in self.clseq:
            w.code(*cc[s])
            w.bits(ev, {16: 2, 17: 3, 18: 7}.get(s, 0))
        self._write_tokens(w)


class RawBlock:
    """A block given as bare bits behind BFINAL: (value, nbits) pairs.  For headers that no class above can spell (BTYPE 3)."""
    btype = None

    def __init__(self, fields):
        self.fields = list(fields)

    def write(self, w, final):
        w.bits(1 if final else 0, 1)
        for v, n in self.fields:
            w.bits(v, n)


def assemble(blocks, final=True, writer=None):
    """The stream of `blocks`; final: BFINAL on the last one.  With a writer, the blocks are appended to it (at any bit position)."""
    w = writer or BitWriter()
    for i, b in enumerate(blocks):
        b.write(w, final and i == len(blocks) - 1)
    return w if writer else w.getvalue()


def end_bit(blocks, final=True):
    w = BitWriter()
    assemble(blocks, final, w)
    return w.bitlen


def block_bits(blocks, final=True, start=0):
    """-> ([the bit at which each block's header starts], the end bit) of the stream written from bit `start` on (a stored block
    pads to a byte of the whole stream, so `start & 7` matters)"""
    w = BitWriter()
    w.bits(0, start & 7)
    base, hdr = start - (start & 7), []
    for i, b in enumerate(blocks):
        hdr.append(base + w.bitlen)
        b.write(w, final and i == len(blocks) - 1)
    return hdr, base + w.bitlen


def replay(blocks, zdict=b""):
    """The plaintext of VALID blocks, from the tokens alone, and the matches [(length, distance)] in order."""
    out = bytearray(zdict)
    matches = []
    for b in blocks:
        if isinstance(b, Stored):
            out += b.data
            continue
        for t in b.tokens:
            if isinstance(t, int):
                out.append(t)
            elif isinstance(t, M):
                assert 3 <= t.length <= 258 and 1 <= t.dist <= min(32768, len(out)), (t, len(out))
                matches.append((t.length, t.dist))
                for _ in range(t.length):
                    out.append(out[-t.dist])
            else:
                raise ValueError("replay of a defect token: %r" % (t,))
    return bytes(out[len(zdict):]), matches


Vector = namedtuple("Vector", "name blob zdict expect blocks")


def _vec(name, blocks, zdict=b"", invalid=False):
    return Vector(name, assemble(blocks), zdict, DATA if invalid else replay(blocks, zdict)[0], blocks)


def is_valid(v):
    return v.expect is not DATA


def spread(symbols, lengths, n):
    """A length list of n entries in which symbols[i] has lengths[i]"""
    out = [0] * n
    for s, ln in zip(symbols, lengths):
        out[s] = ln
    return out


SKEW = list(range(1, 16)) + [15]                      # sixteen codes, complete: 1/2 + 1/4 + ... + 2^-15 + 2^-15
_SKEW_SYMS = [97, 256, 285, 98, 99, 100, 101, 284, 102, 103, 104, 105, 106, 257, 107, 108]         # 107 and 108 get the 15-bit codes


def _pattern(n, seed):
    """n bytes that no deflate-style shortcut produces: a 32-bit multiplicative generator (no match of three bytes worth taking)"""
    out, x = bytearray(), seed * 2654435761 % (1 << 32) or 1
    for _ in range(n):
        x = (x * 1664525 + 1013904223) % (1 << 32)
        out.append(x >> 24)
    return bytes(out)


def valid_vectors():
    v = []
    skew_ll = spread(_SKEW_SYMS, SKEW, 286)
    text = [97, 98, 107, 108, 99, 106]
    # 15-bit literal codes, a 258-match at distance 1 (code 285, 3 bits) and a one-code distance set (one code of one bit: incomplete)
    v.append(_vec("skew_ll_onecode_dist", [Dynamic(skew_ll, [1], text + [M(258, 1), 108, 107, M(3, 1), M(258, 1, 284), 105])]))
    # ... the same with sixteen distance codes of 1..15,15 bits: distances 1 and 2 have the 15-bit codes, 24577.. the one-bit code
    skew_d = SKEW[::-1] + [0] * 13 + [1]
    skew_d[15] = 0                                                                    # (code 29 takes the one-bit code instead of code 15)
    v.append(_vec("skew_ll_skew_dist", [Dynamic(skew_ll, skew_d, text + [M(258, 1), 108, M(3, 2), M(258, 2, 284), M(3, 3), M(240, 8), 107, M(3, 1)])]))
    # codes one bit longer than each first-level table, and two bits: literal codes of 10 and 11 bits (tables of 9 and 10 index bits),
    # distance codes of 9 and 10 bits (tables of 8 and 9) -- every code of the block is used
    ll = spread([97, 98, 99, 256, 257, 100, 101, 102, 103, 104, 105, 106], list(range(1, 11)) + [11, 11], 258)
    d = spread([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], list(range(1, 9)) + [9, 10, 10], 11)
    toks = [97, 98, 99, 100, 101, 102, 103, 104, 105, 106] + [M(3, dd) for dd in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33)] + [104, 105, 106, M(3, 46), 103]
    v.append(_vec("one_bit_past_the_tables", [Dynamic(ll, d, toks)]))
    # ... and with the long codes in bulk: 286 codes of 8..10 bits, 30 distance codes of 4 and 5 bits (nlen = 286, ndist = 30)
    ll = [8] * 240 + [9] * 18 + [10] * 28                                             # 960 + 36 + 28 = 1024 / 1024: complete
    assert kraft(ll) == 32768 and len(ll) == 286
    d30 = [4, 4] + [5] * 28
    toks = list(range(230, 256)) + [M(3 + i, 1 + i) for i in range(20)] + [M(258, 26), M(257, 25), M(130, 24), 255, 240]
    v.append(_vec("nlen286_ndist30", [Dynamic(ll, d30, toks, rle=True)]))
    # no distance code at all (HDIST = 1, its one length 0): literals only
    ll = spread([104, 105, 256], [1, 2, 2], 257)
    v.append(_vec("no_distance_code", [Dynamic(ll, [0], [104, 105, 104, 104, 105], rle=True)]))
    # two blocks that hold an end-of-block and nothing else, their code one code of one bit
    eob_only = spread([256], [1], 257)
    v.append(_vec("two_eob_only_blocks", [Dynamic(eob_only, [0], rle=True), Dynamic(eob_only, [0], rle=True)]))
    # HCLEN: 5 is the smallest a valid header can have (with 4, only 16, 17, 18 and 0 have codes: every length is 0, no end-of-block;
    # that header is among the invalid vectors); 19 = symbol 15 is used
    ll = [8] * 255 + [0, 8]                                                           # 256 codes of 8 bits; nlen = 257
    b = Dynamic(ll, [0], [1, 2, 3, 254, 0], clseq=[(8, 0)] * 255 + [(0, 0), (8, 0), (0, 0)])
    assert b.hclen == 5
    v.append(_vec("hclen5", [b]))
    b = Dynamic(skew_ll, [1], [97, M(3, 1), 108], rle=True)
    assert b.hclen == 19
    v.append(_vec("hclen19", [b]))
    # a code-length 16 whose run starts at the last literal/length entry's value and ends in the distance entries; an 18 with 138 zeros
    ll = spread([97, 98, 256, 257], [1, 3, 3, 2], 258)
    seq = [(18, 97 - 11), (1, 0), (3, 0), (18, 138 - 11), (18, 19 - 11), (3, 0), (2, 0), (16, 4 - 3)]
    v.append(_vec("repeat_across_the_sets", [Dynamic(ll, [2, 2, 2, 2], [97, 98, M(3, 2), M(3, 4), M(3, 1), M(3, 3)], clseq=seq)]))
    ll = spread([0, 139, 256], [1, 2, 2], 257)
    seq = [(1, 0), (18, 127), (2, 0), (18, 116 - 11), (2, 0), (0, 0)]
    v.append(_vec("zeros_138", [Dynamic(ll, [0], [0, 139, 139, 0], clseq=seq)]))
    # ndist = 1, its one code used (nlen = 257 has no length code: the vectors above without a distance code have it)
    v.append(_vec("nlen258_ndist1", [Dynamic(spread([120, 256, 257], [1, 2, 2], 258), [1], [120, M(3, 1), 120])]))
    # length 258 both ways, in the fixed code; every length code with its extra bits all ones
    v.append(_vec("len258_both_spellings", [Fixed([7, M(258, 1), M(258, 1, 284), 8, M(258, 259), M(258, 2, 284)])]))
    toks = [65, 66, 67]
    for i in range(29):
        toks += [M(LBASE[i] + (1 << LEXT[i]) - 1, 1 + i % 3, 257 + i), 48 + i]
    v.append(_vec("length_codes_extra_all_ones", [Fixed(toks)]))
    v.append(_vec("length_codes_extra_all_ones_dynamic", [Dynamic([9] * 60 + [8] * 226, [4, 4] + [5] * 28, toks, rle=True)]))
    # distance 32768 with exactly 32768 bytes produced (code 29, its 13 extra bits all ones), then 24577 (extra bits 0)
    hist = _pattern(32768, 1)
    v.append(_vec("dist32768_at_32768", [Stored(hist), Fixed([M(258, 32768), M(3, 24577), M(4, 32768)])]))
    # a distance that reaches exactly the first byte of the dictionary: zdict of 1 byte and of 32768 bytes
    v.append(_vec("reach_start_zdict1", [Fixed([M(4, 1), 9, M(3, 6)])], zdict=b"\x5a"))
    big = _pattern(32768, 2)
    v.append(_vec("reach_start_zdict32768", [Fixed([M(258, 32768), M(3, 32768)])], zdict=big))
    v.append(_vec("reach_start_zdict100", [Fixed([200, 201, M(9, 102), M(3, 111)])], zdict=_pattern(100, 3)))
    # the fixed code's 9-bit literals 144..255, and distance code 29 with 13 extra bits (into a dictionary, to keep the vector small)
    v.append(_vec("fixed_9bit_literals_dist29", [Fixed(list(range(144, 256)) + [M(7, 24577 + 112), M(200, 32768), M(3, 30000)])], zdict=big))
    # a stored block of length 0 between two compressed blocks that end off a byte boundary
    b1, b2 = Fixed([1, 2, 3]), Dynamic(spread([50, 51, 256, 258], [1, 2, 3, 3], 259), [1], [50, 51, M(4, 1)], rle=True)
    assert end_bit([b1], False) % 8 and end_bit([b1, Stored(b""), b2]) % 8
    v.append(_vec("empty_stored_between", [b1, Stored(b""), b2]))
    v.append(_vec("stored_65535", [Stored(_pattern(65535, 4))]))
    v.append(_vec("stored_then_match", [Stored(b"abcdefgh"), Fixed([M(8, 8), M(3, 16)]), Stored(b"xyz"), Fixed([M(5, 3)])]))
    # final blocks that end on each of the eight bit positions of the last byte (a 9-bit literal moves the end by one bit)
    ends = set()
    for k in range(8):
        b = Fixed([33] + [200] * k)
        ends.add(end_bit([b]) % 8)
        v.append(_vec("ends_on_bit_%d" % (end_bit([b]) % 8), [b]))
    assert len(ends) == 8
    # 1500 blocks of one byte each: fixed, dynamic with a 15-bit code for the byte, stored, in turn; then an empty final block
    blocks = []
    for i in range(1500):
        c = 32 + i % 90
        if i % 3 == 0:
            blocks.append(Fixed([c]))
        elif i % 3 == 1:
            syms = [256] + [s for s in range(1, 17) if s != c][:14] + [c]
            blocks.append(Dynamic(spread(syms, SKEW, 257), [0], [c], rle=True))
        else:
            blocks.append(Stored(bytes([c])))
    blocks.append(Fixed([]))
    v.append(_vec("blocks_1500", blocks))
    return v


def invalid_vectors():
    """(vector, the phrase of zlib's message) -- every stream is invalid for exactly the reason its name gives"""
    v = []
    tail = [Raw(0x5A5A5A5A, 32)] * 4                   # bits behind a defect, so that it is not the end of the input that is met

    def add(name, blocks, phrase, zdict=b""):
        v.append((_vec(name, blocks, zdict, invalid=True), phrase))

    ok_ll = spread([97, 98, 256], [1, 2, 2], 257)
    add("block_type_3", [Fixed([1, 2]), RawBlock([(3, 2), (0x1234, 16)])], "invalid block type")
    add("stored_len_nlen_mismatch", [Stored(b"hello", nlen=0xFFFA ^ 1)], "invalid stored block lengths")
    for hlit in (30, 31):
        add("hlit_%d" % (hlit + 257), [Dynamic(ok_ll + [0] * 29, [1], hlit=hlit, eob=False, tokens=[97] + tail)], "too many length or distance symbols")
    for hdist in (30, 31):
        add("hdist_%d" % (hdist + 1), [Dynamic(ok_ll, [5] * 30, hdist=hdist, eob=False, tokens=[97] + tail)], "too many length or distance symbols")
    cl = [0] * 19
    cl[0], cl[1], cl[2] = 2, 2, 2                                                     # three codes of two bits: one missing
    add("incomplete_code_length_code", [Dynamic(ok_ll, [1], cl=cl, eob=False, tokens=tail)], "invalid code lengths set")
    cl = [0] * 19
    cl[0], cl[1], cl[2] = 1, 1, 1
    add("oversubscribed_code_length_code", [Dynamic(ok_ll, [1], cl=cl, eob=False, tokens=tail)], "invalid code lengths set")
    add("hclen4_all_lengths_zero", [Dynamic([0] * 257, [0], clseq=[(18, 127), (18, 120 - 11)], cl=spread([18, 0], [1, 1], 19), hclen=4, eob=False, tokens=tail)],
        "missing end-of-block")
    add("oversubscribed_literal_set", [Dynamic(spread([97, 98, 99, 256], [1, 2, 2, 2], 257), [1], eob=False, tokens=tail)], "invalid literal/lengths set")
    add("incomplete_literal_set", [Dynamic(spread([97, 256], [2, 2], 257), [1], eob=False, tokens=tail)], "invalid literal/lengths set")
    add("incomplete_distance_set", [Dynamic(ok_ll, [2, 2], eob=False, tokens=tail)], "invalid distances set")
    add("incomplete_distance_set_3", [Dynamic(ok_ll, [1, 2, 3], eob=False, tokens=tail)], "invalid distances set")
    add("oversubscribed_distance_set", [Dynamic(ok_ll, [1, 1, 1], eob=False, tokens=tail)], "invalid distances set")
    add("no_end_of_block_code", [Dynamic(spread([97, 98, 99], [1, 2, 2], 257), [1], eob=False, tokens=[97] + tail)], "missing end-of-block")
    add("repeat_as_first_length", [Dynamic(ok_ll, [1], clseq=[(16, 0), (1, 0), (2, 0)], cl=spread([16, 1, 2, 0], [2, 2, 2, 2], 19), eob=False, tokens=tail)],
        "invalid bit length repeat")
    seq = [(18, 86), (1, 0), (2, 0), (18, 127), (18, 8), (2, 0), (17, 0)]             # 257 lengths, then three zeros where one entry is left
    add("repeat_overruns_the_lengths", [Dynamic(ok_ll, [1], clseq=seq, eob=False, tokens=tail)], "invalid bit length repeat")
    seq = [(18, 86), (1, 0), (2, 0), (18, 127), (18, 8), (2, 0), (16, 0)]             # a 16 of three where one entry is left
    add("repeat_16_overruns_the_lengths", [Dynamic(ok_ll, [1], clseq=seq, eob=False, tokens=tail)], "invalid bit length repeat")
    for s in (286, 287):
        add("fixed_symbol_%d" % s, [Fixed([1, Sym(s)] + tail, eob=False)], "invalid literal/length code")
    for s in (30, 31):
        add("fixed_distance_code_%d" % s, [Fixed([1, Sym(257), DSym(s)] + tail, eob=False)], "invalid distance code")
        # ... as the last bits of the input: `literal, length 257, distance code 30, end-of-block` and nothing behind
        add("fixed_distance_code_%d_at_the_end" % s, [Fixed([1, Sym(257), DSym(s)])], "invalid distance code")
    # (the same with exactly the five bits of the code present and not one more: 3 + 8 + 8 + 8 + 8 + 7 + 5 + 1 bits = six bytes)
    b = Fixed([1, 2, 3, 4, Sym(257), DSym(30), Raw(0, 1)], eob=False)
    assert end_bit([b]) == 48
    add("fixed_distance_code_30_five_bits_left", [b], "invalid distance code")
    one = spread([97, 256, 257], [1, 2, 2], 258)
    add("unused_code_of_one_code_distance_set", [Dynamic(one, [1], [97, Sym(257), Code(1, 1)] + tail, eob=False)], "invalid distance code")
    add("unused_code_of_one_code_distance_set_at_the_end", [Dynamic(one, [1], [97, Sym(257), Code(1, 1)], eob=False)], "invalid distance code")
    add("length_code_without_distance_codes", [Dynamic(one, [0], [97, Sym(257)] + tail, eob=False)], "invalid distance code")
    add("distance_beyond_start", [Fixed([1, 2, 3, Sym(257), DSym(3)] + tail, eob=False)], "too far back")
    add("distance_beyond_start_at_0", [Fixed([Sym(257), DSym(0)] + tail, eob=False)], "too far back")
    add("distance_beyond_zdict1", [Fixed([9, Sym(257), DSym(2)] + tail, eob=False)], "too far back", zdict=b"\x5a")
    big = _pattern(32768, 2)
    add("distance_beyond_zdict32767", [Fixed([Sym(258), DSym(29), Raw(8191, 13)] + tail, eob=False)], "too far back", zdict=big[1:])
    hist = _pattern(32767, 1)
    add("distance_32768_at_32767", [Stored(hist), Fixed([Sym(285), DSym(29), Raw(8191, 13)] + tail, eob=False)], "too far back")
    return v


def vectors():
    """Every vector, the valid ones first: records (name, blob, zdict, expect, blocks); expect = the plaintext, or DATA"""
    return valid_vectors() + [x for x, _ in invalid_vectors()]


# ---- random valid streams ----------------------------------------------------------------------------------------------------------

def random_complete_lengths(rng, n, maxlen):
    """n >= 2 code lengths of a complete code, none longer than maxlen: the Kraft budget split at random (a leaf of the code tree is
    split in two until there are n), with a taste for the deepest leaf so that long codes do occur"""
    assert 2 <= n <= (1 << maxlen)
    leaves = [1, 1]
    while len(leaves) < n:
        can = [i for i, d in enumerate(leaves) if d < maxlen]
        deep = max(leaves[i] for i in can)
        pick = [i for i in can if leaves[i] == deep] if rng.random() < 0.5 else can
        i = pick[int(rng.integers(0, len(pick)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    return [int(x) for x in leaves]


def random_stream_blocks(rng):
    """The blocks of a valid stream of 1..12 blocks of random kind.  Output <= 40 KiB, input <= 8 KiB."""
    while True:
        blocks, out = [], 0
        for _ in range(int(rng.integers(1, 13))):
            kind = int(rng.integers(0, 4))
            if kind == 0:
                data = rng.bytes(int(rng.integers(0, 300)))
                blocks.append(Stored(data))
                out += len(data)
                continue
            ntok = int(rng.integers(0, 100))
            if kind == 1:
                lits, lens, dists = list(range(256)), list(range(257, 286)), list(range(30))
            else:
                maxlen = int(rng.integers(1, 16))
                nl = int(min(rng.integers(1, 80), 1 << maxlen))
                lsyms = [256] + [int(s) for s in rng.choice([s for s in range(286) if s != 256], nl - 1, replace=False)]
                lits, lens = [s for s in lsyms if s < 256], [s for s in lsyms if s > 256]
                ll = spread(lsyms, [1] if nl == 1 else random_complete_lengths(rng, nl, maxlen), int(rng.integers(max(lsyms) + 1, 287)) if max(lsyms) < 286 else 286)
                maxd = int(rng.integers(1, 16))
                nd = int(min(rng.integers(0, 31), 1 << maxd)) if lens else 0
                dists = sorted(int(s) for s in rng.choice(30, nd, replace=False))
                d = spread(dists, [1] if nd == 1 else random_complete_lengths(rng, nd, maxd), max(dists) + 1) if nd else [0]
            toks = []
            for _ in range(ntok):
                feas = [s for s in dists if DBASE[s] <= out]
                if lens and feas and out < 40 * 1024 - 258 and (not lits or rng.random() < 0.4):
                    ls = lens[int(rng.integers(0, len(lens)))] - 257
                    length = LBASE[ls] + int(rng.integers(0, 1 << LEXT[ls]))
                    ds = feas[int(rng.integers(0, len(feas)))]
                    dist = DBASE[ds] + int(rng.integers(0, min(1 << DEXT[ds], out - DBASE[ds] + 1)))
                    toks.append(M(length, dist, ls + 257))
                    out += length
                elif lits:
                    toks.append(lits[int(rng.integers(0, len(lits)))])
                    out += 1
            blocks.append(Fixed(toks) if kind == 1 else Dynamic(ll, d, toks, rle=bool(rng.integers(0, 2))))
        if len(assemble(blocks)) <= 8192 and out <= 40 * 1024:
            return blocks


def random_stream(rng):
    """A valid stream of random_stream_blocks -> (blob, expect)"""
    blocks = random_stream_blocks(rng)
    return assemble(blocks), replay(blocks)[0]


def random_streams(seed=1951, n=300):
    """n random_stream cases from a fixed seed -> [(blob, expect)]"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return [random_stream(rng) for _ in range(n)]


def random_block_streams(seed=1951, n=300):
    """The blocks of the same n cases -> [blocks]"""
    import numpy as np
    rng = np.random.default_rng(seed)
    return [random_stream_blocks(rng) for _ in range(n)]


def match_count(blocks):
    return sum(isinstance(t, M) for b in blocks if not isinstance(b, Stored) for t in b.tokens)


# ---- vectors for a decoder that starts behind a window: the span decoder of the seek-point index --------------------------------------
# A span is a run of blocks decoded with the 32 KiB in front of it as its dictionary (tests/span_tables.py cuts vectors into spans).
# Every valid vector's name states a property, and the builder asserts it here, from its own tokens.

RING = 512                     # the small history ring of the member / span kernels: the sources below lie around its edge
EDGE_W = (1, 511, 512, 513, 32767, 32768)
EDGE_OPS = (0, 1, 2, 300, 511, 512, 513, 700)


def _nine_bit(j):
    """nine literals of which j take nine bits in the fixed code: a fixed block of 82 + j bits"""
    return [200] * j + [33] * (9 - j)


def hdr_every_bit_blocks(target=64 << 10):
    """About `target` bytes of non-final blocks of 0..9 bytes each, and an empty final block.  Fixed blocks of nine literals, j of
    them of nine bits, move the next header by 2 + j bits; every seventh block is a dynamic one (a one-bit or a two-bit code for
    its literal), every seventh a stored one of 1..9 bytes, and every 64th an empty stored or an end-of-block-only dynamic block."""
    blocks, w, i = [], BitWriter(), 0
    eob_only = spread([256], [1], 257)
    while w.bitlen < 8 * target:
        c = 32 + i % 90
        if i % 64 == 31:
            b = Stored(b"") if i % 128 == 31 else Dynamic(eob_only, [0], rle=True)
        elif i % 7 == 3:
            n = 1 + (i // 7) % 9
            if (i // 7) % 2:
                b = Dynamic(spread([c, 256], [1, 1], 257), [0], [c] * n, rle=True)
            else:
                b = Dynamic(spread([c, c + 1, 256], [1, 2, 2], 257), [0], ([c, c + 1] * 5)[:n], rle=True)
        elif i % 7 == 6:
            b = Stored(bytes((c + k) & 0xFF for k in range(1 + (i // 7) % 9)))
        else:
            b = Fixed(_nine_bit((i * 3 + i // 10) % 10))
        blocks.append(b)
        b.write(w, False)
        i += 1
    return blocks + [Fixed([])]


def hdr_every_bit_census(blocks):
    """What the vector's name promises, counted from block_bits: {(kind of the block in front, header bit & 7)}, the bits at which
    a stored block with data starts, the kinds in front of which an empty block stands, and the lowest output / input ratio of
    any 4096 stream bytes"""
    hdr, end = block_bits(blocks)
    kind = lambda b: ("stored" if b.data else "empty_stored") if isinstance(b, Stored) else \
        ("fixed" if isinstance(b, Fixed) else ("dynamic" if b.tokens else "eob_only"))
    front = {(kind(blocks[i - 1]), hdr[i] & 7) for i in range(1, len(blocks))}
    stored_at = {hdr[i] & 7 for i, b in enumerate(blocks) if kind(b) == "stored"}
    outs = [0]
    for b in blocks:
        outs.append(outs[-1] + (len(b.data) if isinstance(b, Stored) else len(b.tokens)))
    # the output of the blocks that START in each 4096-byte piece of the stream
    per = {}
    for i, h in enumerate(hdr):
        per[h >> 15] = per.get(h >> 15, 0) + outs[i + 1] - outs[i]
    ratio = min(per[k] for k in range(max(per))) / 4096.0          # (the last piece is not a full one)
    return front, stored_at, ratio, (end + 7) >> 3


def _edge_vector(name, w, tokens, seed):
    return _vec(name, [Fixed(tokens)], zdict=_pattern(w, seed))


def win_edge_vectors():
    """win_edges_<w>: a window of w bytes and one fixed block whose FIRST token reaches the window's first byte, M(3, w); then
    overlapping copies at distances 1 and 2 with 0, 1 and 2 literals in front, one at distance 4 whose source starts at -1, and
    further on copies at exactly op + w (while that is a distance) and at 511, 512 and 513.
    win_edges_<w>_op<T>_<what>: T literals and then ONE 258-byte copy at op = T: `first` = at distance T + w, the window's first
    byte; d511 / d512 / d513 = from around the ring's edge.  At T = 0, 1, 2 and w = 1 `first` has dist < len and a source that
    straddles -1/0; so have the vectors ..._straddle (distance T + 1 and T + 2).
    -> (vectors, {name: (op, length, dist) of the copy the name is about})"""
    out, about = [], {}
    for w in EDGE_W:
        seed = 100 + w
        lit = lambda n, s: list(_pattern(n, s))
        toks = [M(3, w), M(258, 4)]
        for k in range(3):
            toks += lit(k, 7 + k) + [M(258, 1)] + lit(k, 17 + k) + [M(258, 2)]
        toks += lit(5, 3)
        op = replay([Fixed(toks)], _pattern(w, seed))[0].__len__()
        for _ in range(3):
            if op + w <= 32768:
                toks += [M(3, op + w), 77]
                op += 4
            toks += [M(258, 511), M(200, 512), M(258, 513), 78]
            op += 258 + 200 + 258 + 1
        out.append(_edge_vector("win_edges_%d" % w, w, toks, seed))
        about["win_edges_%d" % w] = (0, 3, w)
        for t in EDGE_OPS:
            cases = [("first", t + w)] + [("d%d" % d, d) for d in (511, 512, 513)]
            if t < 3:
                cases += [("straddle%d" % k, t + k) for k in (1, 2)]
            for what, d in cases:
                if d > min(32768, t + w) or (what != "first" and d == t + w):
                    continue
                name = "win_edges_%d_op%d_%s" % (w, t, what)
                out.append(_edge_vector(name, w, lit(t, 31 + t) + [M(258, d), 1, 2], seed))
                about[name] = (t, 258, d)
    return out, about


def win_beyond_vectors():
    """win_beyond_<w>: the start of win_edges_<w>, then one copy at op + w + 1, one byte in front of the window (w = 32767: at
    op = 0, since 32768 is the largest distance there is)"""
    tail = [Raw(0x5A5A5A5A, 32)] * 4
    out = []
    for w in (1, 511, 512, 32767):
        head = [] if w == 32767 else [M(3, w)]
        op = 3 * len(head)
        out.append(_vec("win_beyond_%d" % w, [Fixed(head + [M(3, op + w + 1)] + tail, eob=False)], zdict=_pattern(w, 100 + w), invalid=True))
    return out


def long_block_vector(seed=4242, ntok=6300):
    """long_block_into_window: ONE dynamic block of `ntok` tokens behind a window of 32768 bytes, a third of them matches whose
    distances are spread over 1 .. op + 32768 -> (vector, counts)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ll = [8] * 240 + [9] * 18 + [10] * 28
    d30 = [4, 4] + [5] * 28
    assert kraft(ll) == 32768 and kraft(d30) == 32768
    toks, op = [], 0
    for _ in range(ntok):
        if rng.random() < 1 / 3:
            length = 258 if rng.random() < 0.02 else int(rng.integers(3, 20))
            reach = min(32768, op + 32768)
            r = rng.random()
            if r < 0.1 and op + length - 1 <= 32768:
                dist = op + int(rng.integers(1, length))                   # starts in the window, ends in the output
            elif r < 0.2:
                dist = int(rng.integers(1, min(reach, 20) + 1))            # short, often dist < length
            elif r < 0.3:
                dist = min(reach, int(rng.integers(RING - 2, RING + 3)))   # around the ring's edge
            else:
                dist = int(rng.integers(1, reach + 1))
            toks.append(M(length, dist))
            op += length
        else:
            toks.append(int(rng.integers(0, 256)))
            op += 1
    v = _vec("long_block_into_window", [Dynamic(ll, d30, toks, rle=True)], zdict=_pattern(32768, 5))
    return v, long_block_counts(v)


def long_block_counts(v):
    """from replay alone: tokens, matches, sources that begin in the window, that straddle -1/0, that lie more than RING back"""
    plain, matches = replay(v.blocks, v.zdict)
    c = dict(tokens=len(v.blocks[0].tokens), matches=len(matches), in_window=0, straddle=0, far=0, stream=len(v.blob), out=len(plain))
    op = 0
    for t in v.blocks[0].tokens:
        if isinstance(t, M):
            c["in_window"] += t.dist > op
            c["straddle"] += op < t.dist < op + t.length
            c["far"] += t.dist > RING
            op += t.length
        else:
            op += 1
    return c


def crc_fold_vector(n):
    """crc_fold_<n>: n bytes out of fixed blocks of one literal and 63 copies of 258 bytes at distance 1 (a last, shorter block)"""
    blocks, left, i = [], n, 0
    while left:
        m = min(left, 1 + 63 * 258) - 1
        toks = [65 + i % 26] + [M(258, 1)] * (m // 258)
        m %= 258
        toks += [M(m, 1)] if m >= 3 else [65 + i % 26] * m
        blocks.append(Fixed(toks))
        left -= min(left, 1 + 63 * 258)
        i += 1
    return _vec("crc_fold_%d" % n, blocks)


REFILL_W = (1, 100, 240)


def refill_edge_vector(w, beyond=False):
    """refill_edge_<w>: a window of w bytes and one fixed block of 240 literals and eight copies, each at exactly op + w, with
    op + w < RING all the way.  The block is long enough for a parallel sweep and its last tokens are left to the sequential
    rounds behind it, whose ring is refilled from the output AND the window: the window's first byte is then the oldest byte
    that the refill has to bring back.  beyond: the last copy reaches one byte further (invalid)."""
    toks = list(_pattern(240, 9 + w))
    for k in range(8):
        toks.append(M(3, 240 + 3 * k + w + (1 if beyond and k == 7 else 0)))
    if beyond:
        return _vec("refill_beyond_%d" % w, [Fixed(toks + [Raw(0x5A5A5A5A, 32)] * 4, eob=False)], zdict=_pattern(w, 200 + w), invalid=True)
    return _vec("refill_edge_%d" % w, [Fixed(toks)], zdict=_pattern(w, 200 + w))


_span_cache = []


def span_vectors():
    """The vectors above, the valid ones first; each valid one's property is asserted here.  Built once per process."""
    if _span_cache:
        return list(_span_cache)
    v = []
    blocks = hdr_every_bit_blocks()
    front, stored_at, ratio, nbytes = hdr_every_bit_census(blocks)
    for p in range(8):
        assert ("fixed", p) in front and ("dynamic", p) in front and p in stored_at, p
    assert ("stored", 0) in front and any(k == "empty_stored" for k, _ in front) and any(k == "eob_only" for k, _ in front)
    # the index builder reads at most 4096 / ratio bytes of this stream per call (spacing 4096): more than ten calls
    assert 65536 <= nbytes <= 65536 + 64 and nbytes * ratio / 4096 > 10, (nbytes, ratio)
    assert all(0 <= (len(b.data) if isinstance(b, Stored) else len(b.tokens)) <= 9 for b in blocks)
    v.append(_vec("hdr_every_bit", blocks))
    edges, about = win_edge_vectors()
    for e in edges:
        op, length, dist = about[e.name]
        w = len(e.zdict)
        toks = e.blocks[0].tokens
        assert toks[op] == M(length, dist) and all(isinstance(t, int) for t in toks[:op]), e.name
        what = e.name.split("_")[-1]
        if what == "first" or e.name.count("_") == 2:
            assert dist == op + w                                              # the window's first byte, exactly
        elif what.startswith("straddle"):
            assert op < dist < length and dist <= op + w                       # starts in the window, runs into its own output
        else:
            assert dist in (RING - 1, RING, RING + 1) and dist <= op + w
    for w in EDGE_W:                                                           # ... and every kind of ring-edge source occurs
        kinds = set()
        for e in edges:
            op, length, dist = about[e.name]
            if len(e.zdict) == w and dist in (RING - 1, RING, RING + 1):
                kinds.add("window" if dist >= op + length else ("output" if dist <= op else "across"))
        assert kinds == ({"window", "across", "output"} if w >= RING - 1 else {"across", "output"}), (w, kinds)
    v += edges
    lb, c = long_block_vector()
    assert c["tokens"] >= 6000 and abs(c["matches"] / c["tokens"] - 1 / 3) < 0.03 and c["stream"] >= 3 * 3072, c
    assert c["in_window"] >= 200 and c["straddle"] >= 20 and c["far"] >= 200 and len(lb.zdict) == 32768, c
    v.append(lb)
    for n in (131072, 131073, 262149):
        f = crc_fold_vector(n)
        assert len(f.expect) == n and len(f.blocks) > 1
        v.append(f)
    for w in REFILL_W:
        r = refill_edge_vector(w)
        op = 0
        for t in r.blocks[0].tokens:
            if isinstance(t, M):
                assert t.dist == op + w < RING and op >= 240, (w, op)
            op += t.length if isinstance(t, M) else 1
        # (a sweep wants 12 * 64 + 64 bits of input in front of it and room for 256 bytes)
        assert op >= 256 and 8 * len(r.blob) >= 2000 and match_count(r.blocks) == 8
        v.append(r)
    v += win_beyond_vectors()
    v.append(refill_edge_vector(100, beyond=True))
    _span_cache.extend(v)
    return list(v)


# ---- vectors for the block finder and the chunk chain behind it: streams without sync points ----------------------------------------
# What inflate_chunked_once asks of a stream before it takes it is stated once, in finder_gate(); tests/finder_ref.py is the referee
# of the finder.  Every vector ends in a final stored block of QUIET_TAIL bytes 0xFF, in which no header can start.

QUIET_TAIL = 96
SYNC = b"\x00\x00\xff\xff"
WIN = 32768
FINDER_HCLENS = (5, 12, 19)


def quiet_filler(n, seed):
    """n incompressible bytes without a sync marker, from a fixed seed (drawn again until there is none)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    while True:
        data = rng.bytes(n)
        if SYNC not in data:
            return data


def block_out_lens(blocks):
    return [len(b.data) if isinstance(b, Stored) else sum(t.length if isinstance(t, M) else 1 for t in b.tokens) for b in blocks]


def stored_payload_bits(blocks, final=True):
    """[(first bit, end bit)] of the payload of every stored block"""
    hdr, _ = block_bits(blocks, final)
    return [(8 * (((h + 3 + 7) >> 3) + 4), 8 * (((h + 3 + 7) >> 3) + 4 + len(b.data))) for h, b in zip(hdr, blocks) if isinstance(b, Stored)]


def true_dynamic_bits(blocks, final=True):
    """the header bits of the non-final dynamic blocks: what the finder is there to find"""
    hdr, _ = block_bits(blocks, final)
    return [h for i, (h, b) in enumerate(zip(hdr, blocks)) if isinstance(b, Dynamic) and not (final and i == len(blocks) - 1)]


def chain_chunks(blocks, listed, start_bit=0):
    """The host's rule (inflate_chunked_once) on the builder's own numbers: the stream is cut at every block header that is in
    `listed` (and at its start), the pieces are merged front to back until each has max(32 KiB, total / 4096) bytes of output, a
    short last one joins its predecessor -> [(header bit, output offset, output length)] of the chunks"""
    hdr, _ = block_bits(blocks, True, start_bit)
    lens = block_out_lens(blocks)
    listed = set(listed) | {hdr[0]}
    pieces, off = [], 0
    for h, n in zip(hdr, lens):
        if h in listed:
            pieces.append([h, off, 0])
        pieces[-1][2] += n
        off += n
    target = max(WIN, off // 4096)
    chunks = []
    for p in pieces:
        if chunks and chunks[-1][2] < target:
            chunks[-1][2] += p[2]
        else:
            chunks.append(list(p))
    if len(chunks) > 1 and chunks[-1][2] < target:
        last = chunks.pop()
        chunks[-1][2] += last[2]
    return [tuple(c) for c in chunks]


def finder_gate(blob, ncand, chunks):
    """what inflate_chunked_once demands before it takes a stream without sync points, from the bytes: -> list of what is missing"""
    miss = []
    if len(blob) < 65536:
        miss.append("fewer than 65536 bytes of deflate data")
    if blob.count(SYNC) >= 8:
        miss.append("8 or more sync markers: the finder would not run")
    if ncand < 8:
        miss.append("fewer than 8 candidates")
    if len(chunks) < 4 or min(c[2] for c in chunks) < WIN:
        miss.append("no chain of 4 chunks of 32 KiB")
    return miss


def _quiet_end():
    return Stored(b"\xff" * QUIET_TAIL)


def _mid_hclen_block():
    """a dynamic block whose code-length code ends at symbol 4: HCLEN = 12"""
    syms = list(range(65, 96)) + [256]
    b = Dynamic(spread(syms, [4] * 8 + [5] * 8 + [6] * 16, 257), [0], [65, 80, 95, 66, 94])
    assert b.hclen == 12 and kraft(b.ll) == 32768
    return b


def _finder_kinds():
    """the dynamic blocks of the phase vector by name: the three HCLENs of the grid, then the header kinds that phase B has branches for"""
    by = {v.name: v.blocks for v in valid_vectors()}
    kinds = [("hclen5", by["hclen5"][0]), ("hclen12", _mid_hclen_block()), ("hclen19", by["hclen19"][0])]
    for name in ("no_distance_code", "skew_ll_onecode_dist", "nlen286_ndist30", "nlen258_ndist1", "repeat_across_the_sets"):
        kinds.append((name, by[name][0]))
    kinds.append(("eob_only", by["two_eob_only_blocks"][0]))
    assert [k[1].hclen for k in kinds[:3]] == list(FINDER_HCLENS)
    return kinds


def _put_at_phase(blocks, w, block, byte_phase, bit):
    """append `block` so that its header starts at a byte = byte_phase mod 4 and at bit `bit` of it: a stored block of 1..4 bytes
    moves the byte, a fixed block of nine literals the bit (82 + j bits)"""
    shim = 82 + (bit - 2) % 8
    p0 = ((w.bitlen + 3 + 7) >> 3) + 4                               # the byte behind a stored header written here
    k = (byte_phase - p0 - (shim >> 3)) % 4 or 4
    for b in (Stored(_pattern(k, 50 + len(blocks))), Fixed(_nine_bit((bit - 2) % 8)), block):
        assert not isinstance(b, Dynamic) or ((w.bitlen >> 3) & 3, w.bitlen & 7) == (byte_phase, bit)
        blocks.append(b)
        b.write(w, False)


def finder_phase_blocks(reach=0, defect=None, filler=33000):
    """Non-final dynamic blocks at every one of the 32 phases (stream byte mod 4, bit 0..7) for each HCLEN of FINDER_HCLENS, and the
    other header kinds of _finder_kinds at eight phases each; five stored blocks of incompressible filler between them, so that the
    true chain has chunks of 32 KiB.  reach: the first block is a fixed one whose first match reaches back `reach` bytes, to the
    first byte of a dictionary of that size.  defect: blocks (of an invalid vector) spliced in behind the third filler."""
    kinds = _finder_kinds()
    work = [(blk, bp, bit) for blk in (k[1] for k in kinds[:3]) for bp in range(4) for bit in range(8)]
    work += [(blk, (i + bit) & 3, bit) for i, (_, blk) in enumerate(kinds[3:]) for bit in range(8)]
    blocks, w = [], BitWriter()
    if reach:
        blocks.append(Fixed([M(3, reach), 9, M(4, 2)]))
        blocks[-1].write(w, False)
    per = -(-len(work) // 5)
    for part in range(5):
        blocks.append(Stored(quiet_filler(filler, 300 + part)))
        blocks[-1].write(w, False)
        if part == 3 and defect:
            for b in defect:
                blocks.append(b)
                b.write(w, False)
        for blk, bp, bit in work[part * per:(part + 1) * per]:
            _put_at_phase(blocks, w, blk, bp, bit)
    # the last header of the chain, then the end: a resumed call that reaches the end reports this header
    _put_at_phase(blocks, w, kinds[0][1], 0, 0)
    return blocks + [_quiet_end()]


def finder_phase_census(blocks, start=0):
    """{(byte & 3, bit & 7, hclen)} of the non-final dynamic headers, from block_bits"""
    hdr, _ = block_bits(blocks, True, start)
    return {((h >> 3) & 3, h & 7, b.hclen) for h, b in zip(hdr[:-1], blocks[:-1]) if isinstance(b, Dynamic)}


def _generated_text(n, mul):
    return b"".join(b"record %d of the run, value %d, flag %s\n" % (i * mul % 9973, i * i % 1000003, b"yes" if i % 3 else b"no") for i in range(n))


def decoy_inner_stream():
    """a complete valid raw stream of many small dynamic blocks and a final one: zlib with memLevel 1 over generated text"""
    import zlib
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 1)
    s = z.compress(_generated_text(6000, 31)) + z.flush()          # 228 non-final dynamic blocks in 49 KB: one stored payload
    assert len(s) <= 65535 and SYNC not in s
    return s


def _header_only(block):
    """the bytes of a non-final dynamic block up to the end of its code lengths and two more: a header whose tokens are whatever follows"""
    w = BitWriter()
    Dynamic(block.ll, block.d, [], eob=False, rle=True).write(w, False)
    n = (w.bitlen + 7) // 8 + 2
    return assemble([block], False)[:n]


def finder_decoy_blocks():
    """A true chain of dynamic blocks; between them stored blocks whose payloads hold headers that are none: a whole valid stream
    of its own, a byte copy of a stretch of this very stream (true headers and all, at the same bit phases), and a valid header in
    the last 20 bytes of a payload, whose tokens are the blocks behind it."""
    kinds = dict(_finder_kinds())
    text = [Dynamic([8] * 240 + [9] * 18 + [10] * 28, [4, 4] + [5] * 28, list(_generated_text(6, 7 + i)) + [M(30, 40), M(258, 33)], rle=True) for i in range(12)]
    blocks = [Stored(quiet_filler(33000, 400))]
    blocks += [text[0], Stored(decoy_inner_stream()), text[1]]
    first = len(blocks)
    blocks += [text[2], kinds["hclen19"], Fixed(_nine_bit(3)), text[3], kinds["skew_ll_onecode_dist"], Fixed(_nine_bit(6)), text[4], kinds["hclen5"], text[5]]
    hdr, end = block_bits(blocks, False)
    so_far = assemble(blocks, False)
    stretch = so_far[hdr[first] >> 3:]                               # from the byte of text[2]'s header to the end so far
    assert 200 < len(stretch) < 4000
    blocks += [Stored(quiet_filler(33000, 401)), text[6], Stored(quiet_filler(9000, 402) + stretch + quiet_filler(24000, 403)), text[7]]
    tail = _header_only(Dynamic(spread([65, 66, 256], [1, 2, 2], 257), [0], [65] * 400, rle=True))
    assert 12 <= len(tail) <= 20
    blocks += [Stored(quiet_filler(33000, 404) + tail), text[8], text[9], Stored(quiet_filler(33000, 405)), text[10], text[11]]
    return blocks + [_quiet_end()]


WINDOW_P = (0, 1, 2, 1023, 1024, 1025, 2000)                # where in its chunk an edge block's probes start
WINDOW_W = (1, 1023, 1024, 1025, 32767, 32768)               # ... and how far back they reach: around the chunk's first byte and the 1 024-symbol ring
WINDOW_ODD = (32769, 40001, 65537)
_WIN_LL, _WIN_D = [8] * 240 + [9] * 18 + [10] * 28, [4, 4] + [5] * 28


def _relay(n):
    """n bytes, all from matches at distance 32768 (n >= 3), the longest first"""
    toks = [M(258, WIN)] * (n // 258)
    r = n % 258
    if 0 < r < 3:                                               # no match is shorter than 3: shorten the last long one
        toks[-1:] = [M(255 + r, WIN), M(3, WIN)]
    elif r:
        toks.append(M(r, WIN))
    return toks


def relay_block():
    toks = [M(258, WIN)] * 126 + [M(257, WIN), M(3, WIN)]
    return Dynamic(_WIN_LL, _WIN_D, toks, rle=True)


def edge_block(p, w, total, seed):
    """One chunk of `total` bytes: p bytes of lead-in, M(3, w) and M(258, w) at chunk offset p, three marker bytes and an overlapping
    M(258, 2), a 258-copy whose source begins 100 bytes in front of the chunk -- at offset 100 where the lead-in has room for it,
    else behind the probes -- and relay matches to the end.  -> (block, {what: chunk offset})"""
    lits = list(_pattern(110, seed))
    toks, at = [], {}
    if p >= 358:
        toks += lits[:100] + [M(258, 200)] + (_relay(p - 358) if p - 358 >= 3 else lits[100:100 + p - 358])
        at["straddle"] = 100
    else:
        toks += lits[:p]
    at["probe"] = p
    toks += [M(3, w), M(258, w), M(3, WIN), M(258, 2)]
    op = p + 3 + 258 + 3 + 258
    at["overlap"] = op - 258
    if "straddle" not in at:
        toks.append(M(258, op + 100))
        at["straddle"] = op
        op += 258
    toks += _relay(total - op)
    return Dynamic(_WIN_LL, _WIN_D, toks, rle=True), at


def finder_window_blocks(nrelay=90):
    """72 KiB of stored random bytes, `nrelay` relay blocks, the 42 edge blocks (every p with every w), the quiet end.  Every
    dynamic block makes a chunk of its own; every byte behind the seed that is not one of the edge blocks' few literals reaches
    the output only through the marker windows.  -> (blocks, [the edge blocks' offsets])"""
    seed = quiet_filler(72 << 10, 500)
    blocks = [Stored(seed[:36 << 10]), Stored(seed[36 << 10:])]
    blocks += [relay_block() for _ in range(nrelay)]
    about = []
    for i, (p, w) in enumerate((p, w) for p in WINDOW_P for w in WINDOW_W):
        total = WINDOW_ODD[(i // 5) % 3] if i % 5 == 2 else WIN
        b, at = edge_block(p, w, total, 600 + i)
        blocks.append(b)
        about.append((p, w, total, at))
    return blocks + [_quiet_end()], about


FINDER_DEFECTS = ("unused_code_of_one_code_distance_set", "fixed_distance_code_30", "incomplete_distance_set")


def finder_invalid_vectors():
    """the phase vector with one defective block in its chain, behind more than two chunks -> [Vector] (expect = DATA)"""
    bad = {v.name: v.blocks for v, _ in invalid_vectors()}
    return [Vector("finder_phase_" + name, assemble(finder_phase_blocks(defect=bad[name])), b"", DATA, None) for name in FINDER_DEFECTS]


_finder_cache = {}


def finder_vectors():
    """{name: Vector} of the three valid finder vectors (blocks kept); built once per process"""
    if not _finder_cache:
        for name, blocks in (("finder_phase", finder_phase_blocks()), ("finder_decoy", finder_decoy_blocks()), ("finder_window", finder_window_blocks()[0])):
            _finder_cache[name] = _vec(name, blocks)
    return dict(_finder_cache)


def gzip_member(body, plain, name_len=0):
    """a gzip member around a deflate body; an FNAME field of name_len characters puts the first deflate byte at offset 11 + name_len"""
    import struct
    import zlib
    head = b"\x1f\x8b\x08" + (b"\x08" if name_len else b"\x00") + bytes(4) + b"\x00\xff" + ((b"n" * name_len + b"\x00") if name_len else b"")
    return head + body + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xFFFFFFFF)


FINDER_DICTS = (32768, 100, 1)


def finder_resumed_vector(reach):
    """the phase vector behind a dictionary of `reach` bytes whose first byte its first match reaches"""
    blocks = finder_phase_blocks(reach=reach)
    return _vec("finder_phase_reach%d" % reach, blocks, zdict=_pattern(reach, 700 + reach))


def finder_cuts(blocks, start=0):
    """Six places to cut the phase vector written from bit `start` on, all in its last third -> {what: bytes kept}.  The places are
    found from block_bits: inside the tokens of a dynamic block (two bytes short of its end), inside a dynamic header (three bytes
    in), in the middle of the last filler's payload, on a block boundary that is a byte boundary (behind a stored block), one
    byte behind it, and one byte short of the end."""
    hdr, end = block_bits(blocks, True, start)
    big = [i for i, b in enumerate(blocks) if isinstance(b, Stored) and len(b.data) > 4096]
    last = big[-1]
    dyn = [i for i in range(last + 1, len(blocks) - 1) if isinstance(blocks[i], Dynamic)]
    long_dyn = [i for i in dyn if len(blocks[i].tokens) >= 40]
    small = [i for i in range(last + 1, len(blocks) - 1) if isinstance(blocks[i], Stored)]
    i, j, s = long_dyn[len(long_dyn) // 2], dyn[len(dyn) // 2], small[len(small) // 2]
    assert hdr[s + 1] % 8 == 0
    cuts = {"in_tokens": (hdr[i + 1] >> 3) - 2, "in_header": (hdr[j] >> 3) + 3, "in_stored": (hdr[last] >> 3) + 5 + len(blocks[last].data) // 2,
            "on_boundary": hdr[s + 1] >> 3, "behind_boundary": (hdr[s + 1] >> 3) + 1, "short_of_end": ((end + 7) >> 3) - 1}
    return cuts

"""A small pure-Python DEFLATE (RFC 1951) token walker for the strategy tests: decodes a raw-deflate stream and reports every
block's BTYPE and every match's (length, distance), so that a test can check what KIND of stream a strategy wrote, not only that it
round-trips.  Slow (pure Python): meant for inputs of up to a few MiB.  Not a conftest: imported by the test files that use it."""

_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
          8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CLORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class WalkError(ValueError):
    pass


class _Bits:
    def __init__(self, data):
        self.d = bytes(data)
        self.n = len(self.d) * 8
        self.pos = 0

    def get(self, k):
        if self.pos + k > self.n:
            raise WalkError("stream truncated")
        i, sh = self.pos >> 3, self.pos & 7
        r = (int.from_bytes(self.d[i:i + 4], "little") >> sh) & ((1 << k) - 1)      # (k <= 16: four bytes hold it)
        self.pos += k
        return r

    def align(self):
        self.pos = (self.pos + 7) & ~7


def _table(lengths):
    """canonical Huffman code -> {(length, code): symbol}"""
    mx = max(lengths) if lengths else 0
    count = [0] * (mx + 2)
    for ln in lengths:
        if ln:
            count[ln] += 1
    code, nxt = 0, [0] * (mx + 2)
    for b in range(1, mx + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    t = {}
    for s, ln in enumerate(lengths):
        if ln:
            t[(ln, nxt[ln])] = s
            nxt[ln] += 1
    return t


def _sym(br, t):
    code = 0
    for ln in range(1, 16):
        code = (code << 1) | br.get(1)        # Huffman codes are packed MSB first
        s = t.get((ln, code))
        if s is not None:
            return s
    raise WalkError("bad Huffman code")


_FIXED_L = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
_FIXED_D = _table([5] * 32)


class Walk:
    """Result of walk(): btypes = BTYPE of every block in order, matches = [(length, distance)], out = the decoded bytes (without
    the preset window), final = whether a block with BFINAL was seen, end_bit = bit position behind the last block walked,
    tokens = the stream's tokens in order over all blocks (an int per literal, (length, distance) per match; end-of-block codes and
    stored bytes are not tokens), blocks = one Block per block."""

    def __init__(self):
        self.btypes, self.matches, self.out, self.final, self.end_bit = [], [], b"", False, 0
        self.tokens, self.blocks = [], []


class Block:
    """One block as walked: btype, final; ll_lens / d_lens = the code lengths read from a dynamic header (hlit / hdist of them; the
    fixed code's 288 / 32 for BTYPE 1, empty for stored), cl_lens = the 19 code-length code lengths (by symbol), hlit, hdist, hclen;
    start_bit = offset of the block's three header bits, header_bits = bits from there to the first token, first_token_bit and
    eob_bit = bit offsets of the first token and of the end-of-block code (stored: of the first data byte and behind the last),
    ntokens = tokens of this block."""

    def __init__(self):
        self.btype, self.final, self.ll_lens, self.d_lens, self.cl_lens = 0, False, [], [], []
        self.hlit = self.hdist = self.hclen = 0
        self.start_bit = self.header_bits = self.first_token_bit = self.eob_bit = self.ntokens = 0


def walk(data, window=b"", stop_at_final=True):
    """Walk a raw-deflate stream.  `window`: bytes in front of the stream (a preset dictionary) that distances may reach.
    Walks until a BFINAL block (or the end of the data when the stream ends on a sync flush)."""
    br = _Bits(data)
    out = bytearray(window)
    w = Walk()
    while True:
        if br.n - br.pos < 3:
            break
        blk = Block()
        blk.start_bit = br.pos
        bfinal, btype = br.get(1), br.get(2)
        w.btypes.append(btype)
        w.blocks.append(blk)
        blk.btype, blk.final = btype, bool(bfinal)
        if btype == 0:
            br.align()
            ln, nln = br.get(16), br.get(16)
            if ln ^ nln != 0xFFFF:
                raise WalkError("stored length check")
            start = br.pos // 8
            if start + ln > len(data):
                raise WalkError("stored block truncated")
            out += bytes(data[start:start + ln])
            blk.first_token_bit = br.pos
            br.pos += 8 * ln
            blk.eob_bit = br.pos
            blk.header_bits = blk.first_token_bit - blk.start_bit
        elif btype in (1, 2):
            if btype == 1:
                lt, dt = _FIXED_L, _FIXED_D
                blk.ll_lens, blk.d_lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32
            else:
                hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[_CLORDER[i]] = br.get(3)
                ct = _table(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _sym(br, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        if not lens:
                            raise WalkError("repeat with no length")
                        lens += [lens[-1]] * (3 + br.get(2))
                    elif s == 17:
                        lens += [0] * (3 + br.get(3))
                    else:
                        lens += [0] * (11 + br.get(7))
                if len(lens) > hlit + hdist:
                    raise WalkError("code lengths overrun")
                lt, dt = _table(lens[:hlit]), _table(lens[hlit:])
                blk.ll_lens, blk.d_lens, blk.cl_lens = lens[:hlit], lens[hlit:], cl
                blk.hlit, blk.hdist, blk.hclen = hlit, hdist, hclen
            blk.first_token_bit = br.pos
            blk.header_bits = br.pos - blk.start_bit
            ntok0 = len(w.tokens)
            while True:
                at = br.pos
                s = _sym(br, lt)
                if s < 256:
                    out.append(s)
                    w.tokens.append(s)
                elif s == 256:
                    blk.eob_bit = at
                    blk.ntokens = len(w.tokens) - ntok0
                    break
                else:
                    s -= 257
                    if s >= 29:
                        raise WalkError("bad length symbol")
                    ln = _LBASE[s] + br.get(_LEXT[s])
                    d = _sym(br, dt)
                    if d >= 30:
                        raise WalkError("bad distance symbol")
                    dist = _DBASE[d] + br.get(_DEXT[d])
                    if dist > len(out):
                        raise WalkError("distance too far back")
                    w.matches.append((ln, dist))
                    w.tokens.append((ln, dist))
                    for _ in range(ln):
                        out.append(out[-dist])
        else:
            raise WalkError("BTYPE 3")
        if bfinal:
            w.final = True
            if stop_at_final:
                break
        w.end_bit = br.pos
    w.end_bit = br.pos
    w.out = bytes(out[len(window):])
    return w


def strip_container(stream, wbits):
    """The raw-deflate part of a zlib (9..15), gzip (25..31) or raw (-15..-9) stream (no header flags beyond what zlib writes)."""
    if wbits < 0:
        return stream
    if wbits >= 25:
        return stream[10:-8]
    return stream[2 + (4 if stream[1] & 0x20 else 0):-4]


def check_strategy(w, strategy):
    """Assert what a stream written with `strategy` (zlib's Z_* numbers) must look like; returns a message, or None if it is fine."""
    if strategy == 2 and w.matches:
        return "Huffman-only stream has %d matches" % len(w.matches)
    if strategy == 3:
        bad = [m for m in w.matches if m[1] != 1 or not 3 <= m[0] <= 258]
        if bad:
            return "RLE stream has matches other than distance 1: %r" % bad[:5]
    if strategy == 4 and 2 in w.btypes:
        return "fixed stream has a dynamic block"
    if strategy == 1:
        short = [m for m in w.matches if m[0] < 6]
        if short:
            return "filtered stream has matches shorter than 6: %r" % short[:5]
    return None

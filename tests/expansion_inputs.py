"""Named worst-case inputs for the output bounds: inputs chosen to make a unit as LARGE as the format allows,
the unit plan of every entry point, the tests' own bound of a unit, and the referee's units for an input (search_ref /
huffman_ref, one unit at a time behind the 32 KiB in front of it).  Every input is seeded and carries the property it was built
for; tests/test_cpu_expansion_bounds.py proves on the CPU that the referee shows that property and stays under the bound,
tests/test_gpu_expansion_bounds.py takes the inputs through every compress entry point.  Not a conftest: imported by the tests
that use it.

Why these bytes: the fixed code (RFC 1951 3.2.6) spends 9 bits on a byte from 144 up.  Drawn independently from a small alphabet
they have no useful matches, a dynamic code spends log2(alphabet) bits on each and beats the stored form -- and Z_FIXED writes a
fixed block wherever a dynamic one would have won (huffman_ref.choose, fixed_only), also where stored beats fixed.  Such a unit
takes 9 bits a byte: more than its stored form."""
import numpy as np

import huffman_ref as H
import search_ref as S

DEFAULT, FILTERED, HUFFMAN_ONLY, RLE, FIXED = 0, 1, 2, 3, 4
STRATEGIES = (DEFAULT, FILTERED, HUFFMAN_ONLY, RLE, FIXED)
STRATEGY_NAMES = {DEFAULT: "default", FILTERED: "filtered", HUFFMAN_ONLY: "huffman", RLE: "rle", FIXED: "fixed"}
LEVELS = (1, 6, 9)
UNIT, SMALL_UNIT, WIN = 131072, 16384, 32768

# the edges of the bound and of the unit plan: 9 n / 8 overtakes n + 32 at 256; a unit of 16 KiB; a stored chunk of 65 535; a unit
# of 128 KiB; two units and one byte
SIZES = (0, 1, 255, 256, 257, 1024, 16383, 16384, 16385, 65535, 65536, 131071, 131072, 131073, 2 * 131072 + 1)
SMALL_SIZES = tuple(n for n in SIZES if n <= 16385)
LONGEST = 3 * UNIT


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _draw(seed, lo, hi, n=LONGEST):
    return np.random.default_rng(seed).integers(lo, hi, size=n).astype(np.uint8).tobytes()


_HIGH64 = _draw(9001, 144, 208)
_HIGH112 = _draw(9002, 144, 256)
_NOISE = np.random.default_rng(9003).bytes(LONGEST)
_LOW64 = _draw(9004, 0, 64)
_WORDS = [w.encode() for w in ("the", "of", "unit", "block", "stream", "stored", "fixed", "dynamic", "bound", "window", "literal", "match",
                               "distance", "length", "header", "packed", "batch", "strategy", "level", "and", "is", "never", "larger", "than")]


def high64(n):
    """n independent bytes from 144..207: dynamic (6 bits a byte) beats stored, stored beats fixed (9 bits a byte)"""
    return _HIGH64[:n]


def high112(n):
    """n independent bytes from 144..255: the same with dynamic (6.8 bits a byte) winning by less"""
    return _HIGH112[:n]


def noise(n):
    """n seeded uniform bytes: stored wins under every strategy"""
    return _NOISE[:n]


def low_then_high(n):
    """the first half from 0..63 (8 bits each in the fixed code), the second from 144..207 (9 bits): fixed costs about 8.5 bits a
    byte, dynamic 7"""
    return _LOW64[:n // 2] + _HIGH64[:n - n // 2]


def text(n):
    """compressible: words of a small vocabulary in a seeded order"""
    rng = np.random.default_rng(9005)
    out = b" ".join(_WORDS[i] for i in rng.integers(0, len(_WORDS), size=n // 4 + 8))
    assert len(out) >= n
    return out[:n]


def unit_mix():
    """three 128 KiB units in one block: high64, noise, text -- only the first expands"""
    return high64(UNIT) + noise(UNIT) + text(UNIT)


class Input:
    """name; make(n); expands_from: under Z_FIXED every unit of at least this many bytes is a fixed block LARGER than n + 32 (None:
    never); stored_from: every unit of at least this many bytes is stored under every strategy (None: not so)"""

    def __init__(self, name, make, expands_from=None, stored_from=None):
        self.name, self.make, self.expands_from, self.stored_from = name, make, expands_from, stored_from


# expands_from, reasoned and not measured: a fixed block of n bytes from 144 up takes ceil((3 + 9 n + 7) / 8) bytes, more than
# n + 32 from n = 240 on -- if the unit is not stored, that is if the dynamic block is smaller than n + 5.  64 symbols: 6 bits a
# byte and a header of some 40 bytes, smaller from about 200 bytes on: the size list's 255.  112 symbols: 6.8 bits a byte and a
# header of some 60 bytes, 0.15 n > 60 from about 400 on: the size list's 1024.  low_then_high: a fixed block of 8.5 n / 8 bytes is
# more than n + 32 from n = 512 on, and 128 symbols at 7 bits with a header of some 70 bytes beat stored from about 600: 1024.
# stored_from: uniform bytes take 8 + 112 / 256 bits each in the fixed code and no fewer than 8 in a dynamic one behind its header;
# the stored form's 5 bytes are less than 0.44 n bits from n = 92 on: the size list's 255.
INPUTS = {
    "high64": Input("high64", high64, expands_from=255),
    "high112": Input("high112", high112, expands_from=1024),
    "noise": Input("noise", noise, stored_from=255),
    "low_then_high": Input("low_then_high", low_then_high, expands_from=1024),
}


def cases(names=None, sizes=SIZES):
    """[(name, n, data)] of the named inputs (all four by default) at `sizes`"""
    return [(k, n, INPUTS[k].make(n)) for k in (names or INPUTS) for n in sizes]


# ---------------------------------------------------------------------------------------------------------------------------
# the tests' own bound (not the engine's: from the format)
# ---------------------------------------------------------------------------------------------------------------------------
def unit_bound(n, strategy, final):
    """The most bytes a unit of n bytes can take (one block, and behind a unit that is not the last the sync-flush
    marker -- an empty stored block: 3 bits, padding, 00 00 FF FF).

    The block type is the cheapest of stored, fixed and dynamic (3.4), so a unit never takes more than its stored form: n bytes
    and 5 per chunk of 65 535 (RFC 1951 3.2.4), huffman_ref.stored_size.  Under Z_FIXED the fixed block stands in for the dynamic
    one, and what is certain is only the fixed block's own size: 3 bits of header, the tokens, 7 bits for the end of block.  A
    literal takes 8 or 9 bits (3.2.6), and a match of l bytes never more than 9 l (test_cpu_expansion_bounds proves it by
    exhaustion): at most 3 + 9 n + 7 bits.  An empty unit is `03 00`, or the bare marker."""
    if n == 0:
        return 2 if final else 5
    if strategy == FIXED:
        return (3 + 9 * n + 7 + 7) // 8 if final else (3 + 9 * n + 7 + 3 + 7) // 8 + 4
    return H.stored_size(n, final)


def unit_plan(n, usize=UNIT):
    """[(offset, length)] of the units a block of n bytes is cut into (an empty block is one empty unit)"""
    return [(off, min(usize, n - off)) for off in range(0, n, usize)] or [(0, 0)]


def batch_unit_size(n, zdict=False):
    """the batch API's unit size for an item: 16 KiB up to 128 KiB without a dictionary (the one-shot's cut), else 128 KiB"""
    return SMALL_UNIT if not zdict and n <= UNIT else UNIT


def bound(n, strategy, final=True, usize=UNIT):
    """the bound of a block of n bytes: the sum over its units"""
    plan = unit_plan(n, usize)
    return sum(unit_bound(ln, strategy, final and k == len(plan) - 1) for k, (_, ln) in enumerate(plan))


# ---------------------------------------------------------------------------------------------------------------------------
# the referee's units
# ---------------------------------------------------------------------------------------------------------------------------
class UnitRef:
    """one unit by the referee: data, strategy, tokens; plan(final), size(final), out(final).  The tokens are kept as one array
    (a match as length << 16 | distance, a literal as its byte): a list of 131 072 tokens is a megabyte."""

    def __init__(self, data, tokens, strategy):
        self.data, self.strategy = data, strategy
        self.plans = {}
        if data:
            hl, hd = H.token_hist(tokens)
            self.plans = {f: H.plan(hl, hd, len(data), final=f, fixed_only=strategy == FIXED) for f in (False, True)}
        self._packed = np.array([(t[0] << 16) | t[1] if isinstance(t, tuple) else t for t in tokens or ()], np.uint32)
        self._out = {}

    @property
    def tokens(self):
        return [(t >> 16, t & 0xFFFF) if t >> 16 else t for t in self._packed.tolist()]

    def plan(self, final):
        return self.plans[bool(final)]

    def size(self, final):
        if not self.data:
            return 2 if final else 5
        return self.plans[bool(final)].size

    def out(self, final):
        if not self.data:
            return b"\x03\x00" if final else b"\x00\x00\x00\xff\xff"
        final = bool(final)
        if final not in self._out:
            P = self.plans[final]
            self._out[final] = H.emit(P, self.tokens if P.btype else None, self.data, final=final)
        return self._out[final]


_search_memo, _unit_memo = {}, {}
MEMO_BYTES = 32 << 20                             # bytes of units kept (a unit takes some eight times its size: key, tokens, bytes)
_memo_bytes = [0]


def _search_tokens(buf, dl, n, level, strategy, max_dist):
    """search_ref.encode's stages up to the tokens, with the search -- the same under every strategy -- run once"""
    key = (buf, dl, level, max_dist)
    shift = S.seg_shift(n, 0)
    if key not in _search_memo:
        if len(_search_memo) > 64:
            _search_memo.clear()
        _search_memo[key] = S.search(buf, dl, n, level, max_dist, shift)
    found = _search_memo[key]
    data, seg = buf[dl:], 1 << shift
    min_len = 6 if strategy == FILTERED else 3
    entries = found.entries
    if S.LEVELS[level][4]:
        table = S.cost_table(data, found.entries).table
        cost = S.fixed_costs(table) if strategy == FIXED else table
        entries = S.programme(data, found.entries, cost, seg, S.LEVELS[level][5], min_len).entries
    return S.tokens(data, entries, seg, min_len).tokens


def unit_ref(buf, dl, level, strategy, max_dist=WIN):
    """the referee's unit for buf[dl:] behind the dictionary buf[:dl] (memoised; Z_RLE and Z_HUFFMAN_ONLY know no level)"""
    buf = bytes(buf)
    n = len(buf) - dl
    searched = strategy in (DEFAULT, FILTERED, FIXED)
    key = (buf, dl, level if searched else 0, strategy, max_dist if searched else 0)
    if key not in _unit_memo:
        data = buf[dl:]
        if n == 0:
            toks = None
        elif strategy == HUFFMAN_ONLY:
            toks = H.literal_tokens(data)
        elif strategy == RLE:
            toks = H.rle_tokens(data, 1 << S.seg_shift(n, 0), buf[dl - 1] if dl else None)
        else:
            toks = _search_tokens(buf, dl, n, level, strategy, max_dist)
        while _unit_memo and _memo_bytes[0] + len(buf) > MEMO_BYTES:
            _memo_bytes[0] -= len(next(iter(_unit_memo))[0])
            del _unit_memo[next(iter(_unit_memo))]
        _memo_bytes[0] += len(buf)
        _unit_memo[key] = UnitRef(data, toks, strategy)
    return _unit_memo[key]


def block_ref(data, level, strategy, usize=UNIT, zdict=b"", max_dist=WIN):
    """the referee's units of one block: [UnitRef], each behind the 32 KiB in front of it (the dictionary's tail included)"""
    hist = bytes(zdict)[-WIN:]
    buf = hist + bytes(data)
    out = []
    for off, ln in unit_plan(len(data), usize):
        p = len(hist) + off
        dl = min(WIN, p)
        out.append(unit_ref(buf[p - dl:p + ln], dl, level, strategy, max_dist))
    return out


def block_sizes(data, level, strategy, final=True, **kw):
    units = block_ref(data, level, strategy, **kw)
    return [u.size(final and k == len(units) - 1) for k, u in enumerate(units)]


def block_bytes(data, level, strategy, final=True, **kw):
    units = block_ref(data, level, strategy, **kw)
    return b"".join(u.out(final and k == len(units) - 1) for k, u in enumerate(units))

"""Built inputs for the entropy-plan tests (tests/test_cpu_entropy_plan.py, tests/test_gpu_entropy_plan.py): each is the smallest
that still reaches its branch of the plan or of the run-length parse.  Under Z_HUFFMAN_ONLY the literal histogram is the byte
histogram, so a list of (byte value, count) IS the input.  Every unit is at most 131072 bytes.  Not a conftest: imported."""
import random

import huffman_ref as H

FLAG_FINAL, FLAG_FLATHDR, FLAG_SEG2K = 1, 2, 16


def from_counts(pairs, seed=1):
    """bytes with exactly these (value, count) pairs, in a fixed shuffled order"""
    out = bytearray()
    for v, c in pairs:
        out += bytes([v]) * c
    random.Random(seed).shuffle(out)
    return bytes(out)


def _scatter(k, seed):
    """k distinct byte values, scattered"""
    return sorted(random.Random(seed).sample(range(256), k))


def _cl_deep_pairs():
    pairs = [(v, 1) for v in range(0, 254, 2)]                  # 127 values; 254 stays unused, 256 (end of block) is the 128th
    for j in range(128):                                        # odd value 2 j + 1
        low = (j ^ (j + 1)).bit_length() - 1                    # number of trailing one bits of j: 0 for half of them, 1 for a quarter ...
        if low < 5:
            pairs.append((2 * j + 1, 2 << low))                 # 64 x 2, 32 x 4, 16 x 8, 8 x 16, 4 x 32
        elif j == 31:
            pairs.append((2 * j + 1, 256))                      # (j = 63, 95, 127 stay unused)
    return pairs


def cl_deep_1023():
    """1023 bytes: 127 values once, 64 twice, 32 x 4, 16 x 8, 8 x 16, 4 x 32 and one 256 times.  With the end-of-block code the
    counts add up to 1024, so the lengths are 10, 9, 8, 7, 6, 5 and 2 with 128, 64, 32, 16, 8, 4 and 1 symbols: the code-length
    code sees counts that halve and gets 8 bits deep before its limit of 7.  The values are interleaved -- the once-only ones on
    the even values, the others on the odd ones by the lowest set bit of their slot -- so that no two neighbours share a length and
    the run-length code 16 never shortens the sequence."""
    return from_counts(_cl_deep_pairs(), seed=1023)


def cl_deep_zero_runs():
    """The same input without the values 96..100 and 160..171: the code-length sequence gets a zero run of 5 (code 17) and one
    of 12 (code 18), and the code-length code stays deeper than 7 before limiting."""
    return from_counts([(v, c) for v, c in _cl_deep_pairs() if not (96 <= v <= 100 or 160 <= v <= 171)], seed=511)


def _fib(k):
    f = [1, 1]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def _geometric():
    """255 symbols, count i = max(1, 5200 x 0.955^i): a long tail of ones and twos under a steep head"""
    return [(i, max(1, int(5200 * 0.955 ** i))) for i in range(255)]


def m_values(m, where):
    """m - 1 byte values (the end-of-block code is the m-th symbol in use)"""
    k = m - 1
    if where == "low":
        return list(range(k))
    if where == "high":
        return list(range(256 - k, 256))
    return _scatter(k, seed=m)


def huffman_only_inputs():
    """[(name, bytes)] for Z_HUFFMAN_ONLY"""
    sc = _scatter(24, 24)
    out = [
        ("one_value_m2", bytes([65]) * 5000),
        ("two_values_m3", from_counts([(0, 3000), (255, 1000)])),
        ("pow2_depth17", from_counts([(v, c) for v, c in zip(_scatter(17, 17), [1] + [1 << i for i in range(16)])])),
        ("fib20", from_counts(list(zip(sc[:20], _fib(20))))),
        ("fib24", from_counts(list(zip(sc, _fib(24))))),
        ("all_equal_256x300", from_counts([(v, 300) for v in range(256)])),
        ("ties200_under_4000", from_counts([(v, 1) for v in range(200)] + [(222, 4000)])),
        ("ties255x2_under_one", from_counts([(v, 2) for v in range(255)] + [(255, 20000)])),
        ("geometric255", from_counts(_geometric())),
        ("stairs", from_counts([(i, 1 + (i // 16) ** 2) for i in range(256)])),
        ("cl_deep_1023", cl_deep_1023()),
        ("cl_deep_zero_runs", cl_deep_zero_runs()),
    ]
    for m in (63, 64, 65, 127, 128, 129, 255, 256, 257):
        for where in ("low", "high", "scattered"):
            vals = m_values(m, where)
            # a few ties, a few distinct counts: ranks decided by index within a count, by count across
            out.append(("m%d_%s" % (m, where), from_counts([(v, (1 + (i * 7) % 13) ** 2) for i, v in enumerate(vals)], seed=m)))
    for name, data in out:
        assert 0 < len(data) <= 131072, (name, len(data))
    return out


# inputs that are meant to fold: name -> alphabet whose depth before limiting must exceed its limit
FOLDS = {"pow2_depth17": "ll", "fib20": "ll", "fib24": "ll", "geometric255": "ll", "cl_deep_1023": "cl", "cl_deep_zero_runs": "cl"}


def rle_all_symbols():
    """Z_RLE, all 286 literal/length symbols: runs of every length code (29 of them), code c about 2^((28 - c) // 3) times --
    the short ones often, 195 and over once each --, every run of another byte value than the one before, so that every byte
    value is a literal many times.  The unit is between 16 and 32 KiB, its segments 512 bytes: a run that would cross a
    segment end is pushed behind it with literals."""
    seg = 512
    out = bytearray()
    v = 0

    def nextv():
        nonlocal v
        v = (v + 1) % 256
        return v

    for c in range(28, -1, -1):
        length = min(H.LEN_BASE[c] + (1 << H.LEN_EXTRA[c]) - 1, 257 if c < 28 else 258)     # the code's last length (258 is code 28's alone)
        for _ in range(1 << ((28 - c) // 3)):
            while len(out) % seg + 1 + length > seg:
                out.append(nextv())
            out += bytes([nextv()]) * (1 + length)
    assert 16384 < len(out) <= 32768, len(out)
    return bytes(out)


def distance_ladder(seed=5):
    """Default strategy: 32 KiB of random bytes, then steps of 1..3 random separator bytes and 8 bytes copied from a chosen
    distance back.  One target distance in each of the 30 distance codes (the code's base + half its range); code c is copied
    2^(c // 3) times over, so the copies' counts are skewed as powers of two and the distance code is deeper than 9 before
    limiting.  A distance below 8 copies a fresh random word of that period.  What the search makes of it is its own business:
    the tests take the histogram as it comes."""
    rng = random.Random(seed)
    out = bytearray(rng.randbytes(32768))
    jobs = []
    for c in range(30):
        d = H.DIST_BASE[c] + ((1 << H.DIST_EXTRA[c]) >> 1)
        jobs += [d] * (1 << (c // 3))
    rng.shuffle(jobs)
    for d in jobs:
        out += rng.randbytes(rng.randint(1, 3))
        if d < 8:
            out += rng.randbytes(d)
        for _ in range(8):
            out.append(out[-d])
    assert len(out) <= 131072, len(out)
    return bytes(out)


def sweep_stream(k, seed=0):
    """the byte stream whose prefixes the block-type sweep compresses: 4096 bytes drawn uniformly from k scattered values"""
    rng = random.Random(1000 * k + seed)
    vals = _scatter(k, 77 + k) if k < 256 else list(range(256))
    return bytes(rng.choice(vals) for _ in range(4096))


SWEEP_K = (2, 16, 64, 256)
SWEEP_MAX = 320          # the ordinary header: every change of the choice lies below
SWEEP_MAX_FLAT = 1200    # the flat header costs 74 + 4 x (HLIT + HDIST) bits: dynamic wins later (k = 2: from 1128 bytes on)


def sweep_sizes(btype_of, nmax=SWEEP_MAX):
    """btype_of(n) -> (btype, exact tie?) for n = 1 .. nmax; keeps the sizes at which the choice differs from the size in front,
    their neighbours on both sides, every size with an exact tie of the two cheapest forms, and 1 and nmax"""
    kinds = {n: btype_of(n) for n in range(1, nmax + 1)}
    keep = {1, nmax}
    for n in range(2, nmax + 1):
        if kinds[n][0] != kinds[n - 1][0]:
            keep |= {n - 2, n - 1, n, n + 1}
        if kinds[n][1]:
            keep.add(n)
    return sorted(n for n in keep if 1 <= n <= nmax), kinds


def sweep_changes(kinds):
    """the sizes at which the choice differs from the size in front"""
    return [n for n in sorted(kinds) if n - 1 in kinds and kinds[n][0] != kinds[n - 1][0]]


SWEEP_LEVEL = 1          # a greedy level: the parse, and with it the histogram, is the same under Z_FIXED
_SWEEPS = {}


def sweeps(O):
    """{(k, fixed_only, flat): (kept sizes, {n: (block type, exact tie of the two cheapest forms)})}, planned by the reference
    from the oracle's histograms of the prefixes of sweep_stream(k).  The flat header has change points of its own (its cost is
    another), so it has a sweep of its own; under Z_FIXED the header's form does not matter to the choice between fixed and
    stored, but the dynamic cost still decides where stored is allowed, so that sweep is kept apart too."""
    if _SWEEPS:
        return _SWEEPS
    for k in SWEEP_K:
        st = sweep_stream(k)
        for flat in (False, True):
            # (a unit with the flat header has segments of 2 KiB whatever its size: its parse, and so its histogram, is another)
            hists = {}
            for n in range(1, (SWEEP_MAX_FLAT if flat else SWEEP_MAX) + 1):
                h = [int(x) for x in O.deflate_unit(st[:n], b"", SWEEP_LEVEL, FLAG_FLATHDR if flat else 0, debug=True)[2]["hist"]]
                hists[n] = h[:286], h[288:318]
            plans = {n: H.plan(hists[n][0], hists[n][1], n, flat=flat) for n in hists}
            for fixed in (False, True):
                def btype_of(n):
                    P = plans[n]
                    c = sorted([P.cost_sto, P.cost_fix, P.cost_dyn])
                    return H.choose(P.cost_sto, P.cost_fix, P.cost_dyn, fixed), c[0] == c[1]
                _SWEEPS[(k, fixed, flat)] = sweep_sizes(btype_of, len(plans))
    return _SWEEPS


# ---------------------------------------------------------------------------------------------------------------------------
# Z_RLE token inputs: three symbols, so that runs abound
# ---------------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 2, 3, 4, 257, 258, 259, 260, 261, 262, 516, 517, 519)


def _put_run(buf, a, length):
    """a run of `length` equal bytes at a, of another value than the byte in front, and another value behind it"""
    n = len(buf)
    a = max(a, 0)
    b = min(a + length, n)
    if a >= b:
        return
    x = (buf[a - 1] + 1) % 3 if a > 0 else 0
    buf[a:b] = bytes([x]) * (b - a)
    if b < n:
        buf[b] = (x + 1) % 3


def rle_unit(n, seg, seed):
    """n bytes over {0, 1, 2}: runs of the listed lengths (and short random ones) one after another, then, at successive segment
    ends E, a run that ends exactly at E, runs that start 1, 2 and 3 bytes in front of E, one that spans E, and behind them one
    of 518 (258 + 258 + 2) that starts 258 bytes in front of an end: it lies across two ends or more where segments are of up
    to 256 bytes, across one where they are of 1024 or 2048 (518 bytes cannot reach two of those).  A unit with fewer ends
    than cases carries the first ones only; rle_edge_cases() says which."""
    rng = random.Random(seed)
    buf = bytearray()
    x = 0
    lengths = list(RUN_LENGTHS)
    while len(buf) < n:
        ln = lengths.pop(0) if lengths else rng.choice((1, 1, 2, 3, 4, 5, 9, 40, 300, 700))
        x = (x + rng.randint(1, 2)) % 3
        buf += bytes([x]) * ln
    buf = buf[:n]
    ends = list(range(seg, n, seg))
    # (behind the listed run lengths where the unit is long enough, else from the first end on)
    ends = [e for e in ends if e > 4200] or ends
    plans = [(-7, 7), (-1, 9), (-2, 9), (-3, 9), (-5, 11)]
    used = ends[:2 * len(plans):2] if len(ends) >= 2 * len(plans) else ends[:len(plans)]
    for (off, ln), e in zip(plans, used):
        _put_run(buf, e + off, ln)
    # (the long run behind the others, so that it does not write over them; cut at the unit's end if it must be)
    far = [e for e in ends if used and e - 258 > used[-1] + 16]
    if far:
        _put_run(buf, far[0] - 258, 518)
    return bytes(buf)


def _runs(data):
    """[(start, end)] of the maximal runs of equal bytes"""
    out, a = [], 0
    for i in range(1, len(data) + 1):
        if i == len(data) or data[i] != data[a]:
            out.append((a, i))
            a = i
    return out


def rle_edge_cases(data, seg):
    """which of the named cases a unit carries: runs of at least 4 bytes (a literal and a match) that end exactly at a segment
    end ("ends_at"), start 1 / 2 / 3 bytes in front of one ("starts_1" ...), span one ("spans"), and a run of at least 518
    bytes that starts 258 in front of an end and crosses two ends or more ("518_two_ends") or one ("518_one_end")"""
    got = set()
    n = len(data)
    for a, b in _runs(data):
        if b - a < 4:
            continue
        inside = [e for e in range(seg, n, seg) if a < e < b]
        if b % seg == 0 and b < n:
            got.add("ends_at")
        for e in inside:
            if e - a in (1, 2, 3):
                got.add("starts_%d" % (e - a))
            elif e - a >= 4 and b - e >= 4:
                got.add("spans")
        if b - a >= 518 and any(e - a == 258 for e in inside):
            got.add("518_two_ends" if len(inside) >= 2 else "518_one_end")
    return got


def rle_sized_units(seg_shift):
    """[(name, bytes, flags)]: the sizes at which the segment size changes, each with its own segments and with 2 KiB ones"""
    out = []
    for n in (33, 700, 3000, 10000, 40000, 65536, 65537):
        for flags in (0, FLAG_SEG2K):
            seg = 1 << seg_shift(n, flags)
            out.append(("n%d_seg%d" % (n, seg), rle_unit(n, seg, seed=n + flags), flags))
    return out


def rle_small_units():
    """[(name, bytes, flags)]: the densest input in tokens per 64-byte row (period 4: a literal and a match of 3), all-literal input
    whose length is no multiple of 3 (a partly filled literal word at every segment end), and unit lengths on each side of
    multiples of 64"""
    out = [("period4", bytes(b for i in range(500) for b in [97 + i % 26] * 4), 0),
           ("literals_1000", bytes((i * 7 + i // 3) % 251 for i in range(1000)), 0),
           ("literals_2047", bytes((i * 11 + i // 5) % 253 for i in range(2047)), 0)]
    for n in (63, 64, 65, 127, 128, 129, 191, 193):
        out.append(("len%d" % n, rle_unit(n, 32, seed=n), 0))
    return out


def one_segment_rle_inputs():
    """inputs for the zlib anchor: one segment covers each"""
    rng = random.Random(9)
    out = []
    for i in range(60):
        buf = bytearray()
        while len(buf) < 2048:
            buf += bytes([rng.randrange(3)]) * rng.choice(RUN_LENGTHS + (1, 1, 2, 5, 6, 30))
        out.append(bytes(buf[:rng.randint(1, 2048)]))
    out += [bytes([7]) * n for n in RUN_LENGTHS + (520, 2048)]
    out += [bytes([1]) + bytes([7]) * n + bytes([2]) for n in RUN_LENGTHS]
    return out

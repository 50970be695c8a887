"""Built inputs for the encoder's search side: units of seeded incompressible filler with planted probes.
A probe is a source string, a target position and, where a rule needs them, competing candidates that share a 5-, 3- or 12-byte
context with the target; it carries its name, the target, and for every level it names the result it was BUILT for -- (length,
distance) or None -- worked out from DESIGN.md by hand in the function that plants it, not taken from any search.
tests/test_cpu_search_ref.py proves on the CPU that the referee gives every probe's result and that the set reaches every named
branch; tests/test_gpu_search_built.py takes the units through the kernels.  Not a conftest: imported by the tests that use it.

The filler's own buckets matter: a link table keeps only the NEAREST earlier position of a bucket, and 32 768 positions fall into
16 384 buckets, so a far source is hidden behind some filler position unless its context's bucket is free in between.  The
builder draws a probe's string again until the buckets of its start are free between source and target (`clear`)."""
import numpy as np

import search_ref as S

ALL = (1, 2, 3, 4, 5, 6, 7, 8, 9)
GREEDY, DP = (1, 2, 3), (4, 5, 6, 7, 8, 9)
CHAIN = {lv: S.LEVELS[lv][0] for lv in ALL}
Z_FILTERED, Z_FIXED = 1, 4
SEG2K, UNITS16K = 16, 32


class Probe:
    def __init__(self, name, pos, expect):
        self.name, self.pos, self.expect = name, pos, expect          # expect: {level: (length, distance) or None}


class Unit:
    """name; data, zdict (bytes); flags; probes; levels (the levels its probes name); kind (which list of the issue it serves);
    strategies (beside the default, the strategies it also runs under)"""

    def __init__(self, name, kind, n, seed, dict_len=0, flags=0, fill=None):
        self.name, self.kind, self.flags, self.dict_len, self.n = name, kind, flags, dict_len, n
        self.rng = np.random.default_rng(seed)
        self.a = bytearray(self.rng.bytes(dict_len + n) if fill is None else fill)
        assert len(self.a) == dict_len + n
        self.used = np.zeros(dict_len + n + 1, bool)
        self.probes, self.levels, self.strategies = [], ALL, ()
        self.shift = S.seg_shift(n, flags)
        self.seg = 1 << self.shift
        self._fb = None

    @property
    def data(self):
        return bytes(self.a[self.dict_len:])

    @property
    def zdict(self):
        return bytes(self.a[:self.dict_len])

    def seg_end(self, p):
        return min((p // self.seg + 1) * self.seg, self.n)

    # -- planting (positions are the unit's: 0 = its first byte, negative = in the dictionary)
    def put(self, p, bs, fresh=True):
        i = p + self.dict_len
        assert 0 <= i and i + len(bs) <= len(self.a), (self.name, p, len(bs))
        assert not fresh or not self.used[i:i + len(bs)].any(), (self.name, p, "planted twice")
        self.a[i:i + len(bs)] = bs
        self.used[i:i + len(bs)] = True

    def at(self, p):
        return self.a[p + self.dict_len]

    def differ(self, p, q):
        """make the bytes at p and q differ (a match's end), where both exist"""
        if p + self.dict_len < len(self.a) and q + self.dict_len < len(self.a) and q + self.dict_len >= 0 and self.at(p) == self.at(q):
            assert not self.used[p + self.dict_len]
            self.a[p + self.dict_len] ^= 0x55
        for x in (p, q):
            if 0 <= x + self.dict_len < len(self.a):
                self.used[x + self.dict_len] = True

    def _free(self, s, lo, hi, tables, starts=(0,)):
        """the buckets of string s (at each of the offsets `starts`) are met by no filler position in (lo, hi)"""
        if self._fb is None:
            self._fb = [S.buckets(self.a, t) for t in range(3)]
        for t in tables:
            for o in starts:
                if len(s) >= o + S.CONTEXT[t]:
                    h = int(S.buckets(s[o:o + S.CONTEXT[t]], t)[0])
                    if (self._fb[t][lo + o + 1 + self.dict_len:hi + o + self.dict_len] == h).any():
                        return False
        return True

    def string(self, length, lo=None, hi=None, tables=(0, 1, 2), starts=(0,)):
        """a fresh random string whose buckets are free in (lo, hi)"""
        for _ in range(20000):
            s = self.rng.bytes(length)
            if lo is None or self._free(s, lo, hi, tables, starts):
                return s
        raise AssertionError((self.name, "no free bucket", lo, hi))

    def pair(self, tgt, dist, length, s=None, pre=True):
        """the same `length` bytes at tgt - dist and at tgt, different bytes behind them (and in front, so that the position in
        front of the target is nobody's match); overlapping for dist < length (a pattern of period dist)"""
        src = tgt - dist
        if dist < length:
            pat = self.string(dist) if s is None else s
            self.put(src, (pat * (length // dist + 2))[:dist + length])
        else:
            if s is None:
                s = self.string(length, src, tgt)
            self.put(src, s)
            self.put(tgt, s)
        self.differ(tgt + length, src + length)
        if pre and src - 1 + self.dict_len >= 0:
            self.differ(tgt - 1, src - 1)
        return s

    def probe(self, name, pos, expect):
        self.probes.append(Probe(name, pos, {lv: expect[lv] for lv in expect}))

    def same(self, name, pos, length, dist, levels=ALL):
        self.probe(name, pos, {lv: (length, dist) if length else None for lv in levels})


def far_rule(length, dist):
    """a true match of `length` at `dist` that every level finds: what the drops of 3.2 leave of it, per level"""
    out = {}
    for lv in ALL:
        f3, f4 = S.LEVELS[lv][5], S.LEVELS[lv][6]
        out[lv] = None if length < 3 or (length == 3 and dist > f3) or (length == 4 and dist > f4) else (length, dist)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# lengths and distances
# ---------------------------------------------------------------------------------------------------------------------------
LENGTHS = (3, 4, 5, 11, 12, 13, 15, 16, 17, 23, 24, 25, 39, 40, 41, 257, 258, 300)
DISTANCES = (1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 32767, 32768)


def unit_lengths():
    u = Unit("lengths", "lengths", 66000, 101)
    for k, ln in enumerate(LENGTHS):
        tgt = 2048 * (k + 2) + 100 + k                      # each in a segment of its own, 300 bytes fit; every position of a quad
        u.pair(tgt, 1000, ln)
        u.probe("len%d" % ln, tgt, far_rule(min(ln, 258), 1000))
    return u


def unit_distances():
    u = Unit("distances", "distances", 80000, 102)
    for k, d in enumerate(DISTANCES):
        tgt = 34816 + 2048 * k + 40 + 70 * k + (k & 3)
        u.pair(tgt, d, 20)
        u.same("dist%d_len20" % d, tgt, 20, d)
    tgt = 34816 + 2048 * 12 + 40 + 70 * 12
    s = u.pair(tgt, 32769, 20)                              # one byte too far: never found, and nothing else holds these bytes
    u.same("dist32769_none", tgt, 0, 0)
    k = 13
    for ln, ds in ((3, (256, 257, 4096, 4097)), (4, (4096, 4097, 32768))):
        for d in ds:
            tgt = 34816 + 2048 * k + 40 + 70 * k
            k += 1
            u.pair(tgt, d, ln)
            u.probe("len%d_dist%d" % (ln, d), tgt, far_rule(ln, d))
    return u


# ---------------------------------------------------------------------------------------------------------------------------
# selection rules
# ---------------------------------------------------------------------------------------------------------------------------
def _chain(u, tgt, ctx, sources, gap=40):
    """plants the target's string and, nearest first, `sources` behind a common context: each source is (string behind the
    context); returns their distances.  The sources stand `gap` bytes apart in front of the target."""
    dists = []
    for k, s in enumerate(sources):
        d = gap * (k + 1)
        u.put(tgt - d, ctx + s)
        dists.append(d)
    return dists


def unit_selection():
    """n = 40000: segments of 1 KiB.  Every probe has its own stretch of 1 KiB, target at offset 700"""
    u = Unit("selection", "selection", 40000, 103)
    slot = iter(range(2, 39))                                 # (the builder asserts that nothing is planted twice)

    def target():
        return 1024 * next(slot) + 700

    def body(k, stem, diff_at):
        """stem with the byte at diff_at changed (a candidate that shares exactly diff_at bytes behind the context)"""
        b = bytearray(stem)
        b[diff_at] ^= 0x33 + k
        return bytes(b)

    # nearer and farther equal on 16 bytes and beyond: the nearer wins at every level
    t = target(); ctx = u.string(5); stem = u.string(40)
    u.put(t, ctx + stem)
    _chain(u, t, ctx, [body(0, stem, 25), body(1, stem, 25)], gap=50)
    u.same("tie16_nearer", t, 30, 50)
    # the farther one longer only beyond 16 bytes: levels 1-6 take the nearer and extend it (1 has one step anyway), 7-9 the farther
    t = target(); ctx = u.string(5); stem = u.string(60)
    u.put(t, ctx + stem)
    _chain(u, t, ctx, [body(0, stem, 20), body(1, stem, 35)], gap=70)
    u.probe("longer_beyond16", t, {lv: (25, 70) if lv <= 6 else (40, 140) for lv in ALL})
    # the farther one longer within 16 bytes: every level with two steps takes it
    t = target(); ctx = u.string(5); stem = u.string(60)
    u.put(t, ctx + stem)
    _chain(u, t, ctx, [body(0, stem, 3), body(1, stem, 8)], gap=70)
    u.probe("longer_within16", t, {lv: (13, 140) if CHAIN[lv] >= 2 else (8, 70) for lv in ALL})
    # the winner at chain step k behind k - 1 candidates that share the context and one byte: each level finds exactly what its
    # depth allows (steps 6, 7, 10, 11 make every depth 1 .. 12 the winning step of some probe)
    for k in (1, 2, 3, 4, 5, 8, 9, 12, 13, 6, 7, 10, 11):
        t = target(); ctx = u.string(5); stem = u.string(30)
        u.put(t, ctx + stem)
        _chain(u, t, ctx, [body(j, stem, 1) for j in range(k - 1)] + [body(k, stem, 6)], gap=40)
        u.probe("chain_step%d" % k, t, {lv: (11, 40 * k) if CHAIN[lv] >= k else (6, 40) for lv in ALL})
    # a 3-byte repeat whose bytes 4 - 5 differ: only B finds it
    t = target()
    u.pair(t, 100, 3)
    u.probe("b_only", t, far_rule(3, 100))
    # B against an A result of length 3 (the segment's last three bytes: cap = 3).  B's candidate is the NEAREST place with the
    # three bytes, and every candidate of A has them: it is nearer than A's or the same place, never farther.  Nearer: levels 1 - 6
    # take it; on levels 7 - 9 A's three bytes are a nice match already (nice = cap = 3) and B is skipped.
    t = 1024 * next(slot) + 1021
    ctx = u.string(5, t - 220, t)
    u.put(t, ctx); u.put(t - 200, ctx)                       # (two of the five bytes lie behind the segment's end)
    u.put(t - 90, ctx[:3]); u.differ(t - 90 + 3, t + 3)
    u.probe("b_nearer_than_a3", t, {lv: (3, 90) if lv <= 6 else (3, 200) for lv in ALL})
    t = 1024 * next(slot) + 1021
    ctx = u.string(5, t - 220, t)
    u.put(t, ctx); u.put(t - 90, ctx)
    u.same("b_same_as_a3", t, 3, 90)
    # a 12-byte repeat behind more chain steps than any level below 9 walks: C finds it, and it is extended to its true length 30
    t = target(); ctx = u.string(5); stem = u.string(40)
    u.put(t, ctx + stem)
    _chain(u, t, ctx, [body(j, stem, 1) for j in range(9)] + [body(9, stem, 25)], gap=50)
    u.probe("c_only", t, {lv: (30, 500) if lv >= 5 else (6, 50) for lv in ALL})
    # C with fewer than 12 bytes to the segment's end: levels 5, 6 leave it out (cap < 12), levels 7 - 9 compare it in full;
    # level 9 reaches it by its walk as well
    t = 1024 * next(slot) + 1024 - 11
    ctx = u.string(5); stem = u.string(40)
    u.put(t, ctx + stem)
    _chain(u, t, ctx, [body(j, stem, 1) for j in range(9)] + [body(9, stem, 25)], gap=50)
    u.probe("c_short_of_12", t, {lv: (11, 500) if lv >= 7 else (6, 50) for lv in ALL})
    # levels 7 - 9: a first candidate of nice - 1 and of nice bytes with a longer one behind it (levels 1 - 6: equal on 16
    # bytes, so the nearer, extended)
    for nice in (32, 64, 128):
        for first, name in ((nice - 1, "nice%d_minus1" % nice), (nice, "nice%d_exact" % nice)):
            next(slot)
            t = 1024 * next(slot) + 300
            ctx = u.string(5); stem = u.string(260)
            u.put(t, ctx + stem)
            _chain(u, t, ctx, [body(0, stem, first - 5), body(1, stem, 195)], gap=280)
            u.probe(name, t, {lv: (first, 280) if lv <= 6 or first >= S.LEVELS[lv][1] else (200, 560) for lv in ALL})
    # B and C behind a nice match (levels 7 - 9; the walk's first step is nice here: 140 bytes).  Only for B can the skip be seen,
    # and only at cap <= 4: b_nearer_than_a3 above.  C's candidate is the NEAREST place that shares the position's 12 bytes; a
    # nice candidate shares them (or, where cap < 12, every sharer of 12 ties with it at cap from farther back), and any nearer
    # sharer shares the 5-byte context too and came earlier in the walk -- so C's place is the nice one or an earlier step's, and
    # comparing it again changes nothing.  A farther, longer place is never C's.  This probe holds the plain case: a nice first
    # step with a nearer 3-byte place in B.
    next(slot)
    t = 1024 * next(slot) + 300
    ctx = u.string(5); stem = u.string(150)
    u.put(t, ctx + stem)
    u.put(t - 280, ctx + body(0, stem, 135))
    u.put(t - 90, ctx[:3]); u.differ(t - 87, t + 3)
    u.same("bc_behind_nice", t, 140, 280)
    return u


# ---------------------------------------------------------------------------------------------------------------------------
# kernel geometry: tiles of 4096, the link ring's wrap at 8192, the byte ring's wrap at 32768, quads
# ---------------------------------------------------------------------------------------------------------------------------
def unit_geometry():
    u = Unit("geometry", "geometry", 131072, 104)
    for edge, dist in ((4096, 1000), (3 * 4096, 700), (32768, 9000), (9 * 4096, 300), (65536 + 2 * 4096, 20000)):
        # 258 bytes and more from edge - 3 on: the segment end at the edge cuts the first (3 bytes left), the next two have no
        # room, and edge .. edge + 3 take 258 each (the four positions of a quad)
        t0 = edge - 3
        u.pair(t0, dist, 268, s=u.string(268, t0 - dist, t0, (0,), (0, 3, 4, 5, 6)))
        u.probe("edge%d_minus3" % edge, t0, far_rule(3, dist))
        u.same("edge%d_minus2" % edge, t0 + 1, 0, 0)
        for q in range(4):
            u.same("edge%d_plus%d" % (edge, q), edge + q, 258, dist)
    # chain walks across p = 8192 (the link ring's wrap): the winner is the fourth candidate, two on each side
    t = 8192 + 60
    ctx = u.string(5); stem = u.string(30)
    u.put(t, ctx + stem)
    b = bytearray(stem); b[6] ^= 1
    for k, d in enumerate((40, 80, 120, 160)):
        c = bytearray(stem); c[1] ^= 0x10 + k
        u.put(t - d, ctx + bytes(c if k < 3 else b))
    u.probe("walk_across_8192", t, {lv: (11, 160) if CHAIN[lv] >= 4 else (6, 40) for lv in ALL})
    # a source inside the first 32 bytes behind the byte ring's wrap (the mirrored pad), and one that straddles the wrap
    for name, lo in (("source_in_ring_pad", 32778), ("source_across_ring_wrap", 32750)):
        src = bytes(u.a[lo:lo + 40])                             # (the bytes of the 32768 edge's copy lie there, behind filler)
        t = next(t for t in range(33500 + lo % 7, 60000, 101) if u._free(src, lo, t, (0,)) and not u.used[t - 1:t + 41].any())
        u.used[lo:lo + 40] = True
        u.put(t, src); u.differ(t + 40, lo + 40); u.differ(t - 1, lo - 1)
        u.same(name, t, 40, t - lo)
    return u


# ---------------------------------------------------------------------------------------------------------------------------
# segment ends, at every segment size
# ---------------------------------------------------------------------------------------------------------------------------
LEFT = (1, 2, 3, 4, 15, 16, 17, 258)


def segment_end_lefts(seg):
    """the numbers of bytes left that a unit with segments of `seg` bytes must have a probe for"""
    return [k for k in LEFT if k <= 17 or seg >= 512]


def units_segment_ends():
    """A string planted `left` bytes in front of a segment end and going on behind it (the source's copy is longer than the room):
    the target is cut to exactly `left`, and the positions behind it have left - 1, left - 2, ... of the same match, so one string
    17 bytes in front of an end carries the probes for 17, 16, 15, 4, 3, 2, 1, and one 258 bytes in front (segments of 512 and
    more) the probe for 258.  The 17-string stands at a segment end in the unit's middle and (units of 700 bytes and more) at the
    unit's own end, where nothing lies behind it."""
    out = []
    for n, flags in ((33, 0), (700, 0), (3000, 0), (10000, 0), (40000, 0), (65536, 0), (65537, 0), (131072, 0), (3000, SEG2K), (10000, SEG2K)):
        u = Unit("segend_n%d%s" % (n, "_seg2k" if flags else ""), "segment_ends", n, 200 + n + flags, flags=flags)
        nseg = (n + u.seg - 1) // u.seg
        mid = (nseg - 1) // 2 if nseg > 1 else 0

        def plant(end, left, tag):
            over = min(20, n - end)                           # equal bytes behind the end: the match would run over it
            t, room = end - left, left + over
            dist = room + 6 if t - room - 6 >= 1 else 8      # (in the smallest unit an overlapping source: a pattern of period 8)
            u.pair(t, dist, room)
            for j in range(left):
                if left - j in LEFT:
                    u.probe("left%d_%s" % (left - j, tag), t + j, far_rule(left - j if left - j >= 3 else 0, dist))

        plant(min((mid + 1) * u.seg, n), 17, "seg%d" % u.seg)
        end258 = None
        if u.seg >= 512:
            end258 = mid * u.seg if mid >= 1 else n
            plant(end258, 258, "seg%d" % u.seg)
        if n >= 700 and end258 != n:                      # (as much of it as the unit's last segment holds)
            plant(n, min(17, n - (nseg - 1) * u.seg), "unit_end")
        want = {"left%d_seg%d" % (k, u.seg) for k in segment_end_lefts(u.seg)}
        assert want <= {pr.name for pr in u.probes}, (u.name, sorted(want - {pr.name for pr in u.probes}))
        out.append(u)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# dictionaries
# ---------------------------------------------------------------------------------------------------------------------------
DICT_LENS = (0, 1, 3, 5, 100, 32767, 32768)


def units_dictionaries():
    out = []
    for dl in DICT_LENS:
        u = Unit("dict%d" % dl, "dictionaries", 3000, 300 + dl, dict_len=dl)
        t = 32768 - dl if dl >= 32767 else 512               # the source begins at the dictionary's first byte
        ln = min(20, max(dl, 20)) if dl != 1 and dl != 3 and dl != 5 else 20
        u.pair(t, t + dl, ln, pre=False)
        u.same("source_at_dict_start", t, ln, t + dl)
        if dl >= 100:                                         # and a source wholly inside the dictionary, nearer
            u.pair(1500, 1500 + 50, 30)
            u.same("source_in_dict", 1500, 30, 1550)
        out.append(u)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# windows
# ---------------------------------------------------------------------------------------------------------------------------
def units_windows():
    """-> [(unit, window bits)]: sources at max_dist and max_dist + 1; B and C candidates that are too far.  (A chain whose first
    candidate is too far and whose second is not cannot be built: a walk's distances only grow.)"""
    out = []
    for wb in (9, 10, 11, 12, 13, 14):
        md = 1 << wb
        u = Unit("window%d" % wb, "windows", 40000, 400 + wb)
        base = 17 * 1024 + 100
        u.pair(base, md, 20)
        u.same("at_max_dist", base, 20, md)
        u.pair(base + 1100, md + 1, 20)
        u.same("beyond_max_dist", base + 1100, 0, 0)
        u.pair(base + 2300, md + 1, 3)                        # B's candidate too far
        u.same("b_too_far", base + 2300, 0, 0)
        # C's candidate too far: nine nearer candidates in chain A, the tenth beyond the window shares 30 bytes
        t = base + 3700
        ctx = u.string(5); stem = u.string(40)
        u.put(t, ctx + stem)
        for k in range(9):
            c = bytearray(stem); c[1] ^= 0x10 + k
            u.put(t - 50 * (k + 1), ctx + bytes(c))
        c = bytearray(stem); c[25] ^= 1
        u.put(t - md - 5, ctx + bytes(c))
        u.same("c_too_far", t, 6, 50)
        out.append((u, wb))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# cost statistics (levels 4 - 9)
# ---------------------------------------------------------------------------------------------------------------------------
def units_cost_stats():
    out = []
    for n in (1, 255, 256, 257, 1023, 1024, 1025, 4097):
        fq = (b"@read/1\nACGTTGCAAACCGGTT\n+\nIIIIHHHHGGGGFFFF\n" * (n // 40 + 2))
        rng = np.random.default_rng(n)
        body = bytearray(fq[:n])
        for i in range(0, n, 7):
            body[i] = b"ACGT"[int(rng.integers(4))]
        out.append(Unit("stats_n%d" % n, "cost_stats", n, 0, fill=bytes(body)))
    out.append(Unit("stats_zeros", "cost_stats", 5000, 0, fill=bytes(5000)))                # U = 1: the first byte
    # U = 0: the first byte has a match too, and the two matchless bytes in front of each segment end lie outside the sample
    out.append(Unit("stats_zeros_dict", "cost_stats", 4608, 0, dict_len=100, flags=SEG2K, fill=bytes(4708)))
    out.append(Unit("stats_random", "cost_stats", 5000, 501))                               # NM = 0
    # sampled blocks (every fourth of 256) literal-like and all others matches, and the reverse
    rng = np.random.default_rng(502)
    rep = rng.bytes(256)
    for name, sampled_literal in (("stats_sample_literals", True), ("stats_sample_matches", False)):
        parts = [rng.bytes(1024)]
        for b in range(4, 40):
            is_sample = (b & 3) == 0
            parts.append(rng.bytes(256) if is_sample == sampled_literal else rep)
        u = Unit(name, "cost_stats", 256 * 40, 0, fill=b"".join(parts))
        out.append(u)
    # far 3-byte matches on a four-letter alphabet (literal-like), and bytes that occur only outside the sample (cost 52)
    rng = np.random.default_rng(503)
    four = bytes(b"ACGT"[i] for i in rng.integers(4, size=6000))
    out.append(Unit("stats_four_letters", "cost_stats", 6000, 0, fill=four))
    b = bytearray(four)
    b[300:310] = b"0123456789"
    out.append(Unit("stats_unsampled_bytes", "cost_stats", 6000, 0, fill=bytes(b)))
    # a run of decreasing lengths that crosses into a sampled block: the entry at p - 1 is read from an unsampled block
    u = Unit("stats_run_into_sample", "cost_stats", 5000, 504)
    u.pair(1024 - 20, 600, 60)
    u.pair(2048 - 1, 700, 30)
    u.pair(3072, 500, 30)
    out.append(u)
    for x in out:
        x.levels = DP
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# programme and parse (levels 4 - 9, also under Z_FIXED and Z_FILTERED)
# ---------------------------------------------------------------------------------------------------------------------------
ACC_MAX_TARGET = 256 * 41 + 10


def unit_acc_max(fill, seed=605):
    """The largest acc[p + 1] - acc[p + 258]: a 258-byte match over 257 positions that are all literals of 52 quarter bits (bytes
    from 128 up, which the sampled blocks of `fill` never hold).  Every position inside a match has the rest of that match, unless
    the search cannot reach it: at level 4 (two chain steps, table B, no table C) each inner position gets two nearer places of
    its 5-byte bucket and one of its 3-byte bucket with OTHER bytes, drawn from a pool of random strings by their buckets -- its
    walk ends on them, its B link points at one.  The target's own buckets stay free.  Levels with a third step find the inner
    matches again; the branch table asks for the difference at level 4."""
    # 52 is the clamp of a literal's cost; an unseen byte reaches it only with the second term, log2((U + NM) / U), near three
    # bits: the sampled blocks behind the first are 6-byte pieces of the first one, each a new match (NM) and no literal (U)
    rng = np.random.default_rng(seed)
    fill = bytearray(fill)
    first = bytes(fill[:256])
    for b in range(4, len(fill) >> 8, 4):
        fill[256 * b:256 * b + 256] = (b"".join(first[8 * k:8 * k + 6] for k in rng.integers(0, 6, size=43)))[:256]
    u = Unit("prog_acc_max", "programme", len(fill), 0, fill=bytes(fill))
    src, tgt = 256 * 9, ACC_MAX_TARGET                        # both in blocks outside the sample, the target within one segment
    s = bytes(rng.integers(128, 256, size=258).astype(np.uint8))
    while not u._free(s, src, tgt, (0, 1)):                   # (the target's own buckets free in the filler)
        s = bytes(rng.integers(128, 256, size=258).astype(np.uint8))
    pools = {}
    for table, width in ((0, 5), (1, 3)):
        rows = rng.integers(128, 256, size=(400000, width)).astype(np.uint8)
        hb = S.buckets(rows.tobytes(), table)[::width]
        order = np.argsort(hb, kind="stable")
        pools[table] = (rows, hb[order], order)

    def decoys(table, ctx, count):
        rows, sorted_h, order = pools[table]
        h = int(S.buckets(ctx, table)[0])
        lo, hi = np.searchsorted(sorted_h, h), np.searchsorted(sorted_h, h, side="right")
        got = [rows[i].tobytes() for i in order[lo:hi] if rows[i].tobytes() != ctx][:count]
        assert len(got) == count, ("no string of bucket", h)
        return got

    cursor = 256 * 13                                         # decoys: from the next blocks outside the sample on, none inside it
    for j in range(1, 256):
        lot = (decoys(0, s[j:j + 5], 2) if j <= 253 else []) + decoys(1, s[j:j + 3], 1)
        for d in lot:
            while ((cursor >> 8) & 3) == 0 or (((cursor + len(d)) >> 8) & 3) == 0:
                cursor = ((cursor >> 8) + 1) << 8
            u.put(cursor, d)
            cursor += len(d) + 1
    assert cursor < tgt - 300
    u._fb = None                                              # (the buckets of the filler WITH the decoys)
    if not u._free(s, src, tgt, (0, 1)):                      # a decoy landed in the target's own bucket: the next seed
        return unit_acc_max(bytes(fill), seed + 1)
    u.pair(tgt, tgt - src, 258, s=s)
    return u


def units_programme():
    out = []
    rng = np.random.default_rng(600)
    # every match length 3 .. 12 and 64, 65, 66, 128, 258 over literal neighbourhoods of cheap (low) and dear (high) bytes, at
    # near and far distances: the programme's choice runs through the full length, the shorter ones and the literal
    for name, lo_bytes in (("prog_low_bytes", True), ("prog_high_bytes", False), ("prog_mixed_bytes", None)):
        n = 68000
        if lo_bytes is None:
            fill = bytes(rng.integers(0, 256, size=n, dtype=np.uint8))
        else:
            fill = bytes((rng.integers(0, 144, size=n) if lo_bytes else rng.integers(144, 256, size=n)).astype(np.uint8))
        u = Unit(name, "programme", n, 0, fill=fill)
        u.rng = rng
        k = 0
        for ln in (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 64, 65, 66, 128, 258):
            for dist in (1, 40, 300, 5600):
                t = 7000 + 1000 * k + (k % 16)
                k += 1
                s = None
                if lo_bytes is not None:
                    s = bytes((rng.integers(0, 144, size=max(dist if dist < ln else ln, 1)) if lo_bytes else
                               rng.integers(144, 256, size=max(dist if dist < ln else ln, 1))).astype(np.uint8))
                u.pair(t, dist, ln, s=s)
        u.strategies = (Z_FIXED, Z_FILTERED)
        out.append(u)
    # Z_FIXED, where the costs are constants (quarter bits: a literal 32 below 144 and 36 from there, a match 48 + 4 x its extra
    # bits).  The issue's example, a 3-byte match with 13 extra bits of distance against three literals, cannot become an entry:
    # levels 4 - 9 drop 3 bytes beyond 4 096 in the search.  The same sums with entries that exist:
    # * literal against match: 8 bytes from a far source (13 extra bits: 100) whose last 7 also stand 100 (5 extra bits: 68) or
    #   150 (6: 72) bytes back.  The literal and the near match cost 32 + 68 = 100: a tie, the literal keeps it; 36 + 68 and
    #   32 + 72: the far match wins.
    u = Unit("prog_fixed_ties", "programme", 60000, 0, fill=bytes(rng.integers(0, 144, size=60000).astype(np.uint8)))
    u.rng = rng

    def low(k):
        return bytes(rng.integers(0, 144, size=k).astype(np.uint8))

    for k, (first, near) in enumerate(((7, 100), (200, 100), (7, 150), (9, 128), (210, 129))):
        t = 40000 + 1000 * k + 7
        s8 = bytes([first]) + low(7)
        u.pair(t, 20000 + k, 8, s=s8)
        u.put(t + 1 - near, s8[1:]); u.differ(t + 8 - near, t + 8); u.differ(t - near, t)
    # * a shorter length: 10 bytes, the last k + 1 of them one value, and two more of that value behind the target only: the run's
    #   own match (distance 1, no extra bits: 48) from 10 - k on beats the two literals (64) that the full length leaves: length - k
    for k in (1, 2, 3, 4):
        for rep in range(2):
            t = 30000 + 500 * (2 * k + rep)
            x = 100 + k
            s10 = low(9 - k) + bytes([x]) * (k + 1)
            u.pair(t, 300 + k, 10, s=s10)
            u.put(t + 10, bytes([x, x, x ^ 1]), fresh=False)
            u.put(t - 300 - k + 10, bytes([x ^ 2]), fresh=False)
    # * two lengths: 8 bytes whose last two are one value, nine more of it behind the target: 8 + the run's 9 cost what 7 + the
    #   run's 10 cost (no length up to 10 has extra bits): a tie, the longer keeps it
    for rep in range(3):
        t = 36000 + 500 * rep
        s8 = low(6) + bytes([120 + rep]) * 2
        u.pair(t, 400 + rep, 8, s=s8)
        u.put(t + 8, bytes([120 + rep]) * 9 + bytes([7]), fresh=False)
        u.put(t - 400 - rep + 8, bytes([9]), fresh=False)
    # * a length of 3 beyond too_far3 is no candidate: 4 bytes from 4 097 back whose last two are one value, two more of it behind
    #   the target: 3 bytes + the run's 3 (92 + 48) would beat 4 bytes + two literals (92 + 64), and is not tried
    for rep in range(2):
        t = 50000 + 500 * rep + 7
        s4 = low(2) + bytes([131 + rep]) * 2
        while not u._free(s4, t - 4097, t, (1,)):           # (only table B finds four bytes: its bucket free in between)
            s4 = low(2) + bytes([131 + rep]) * 2
        u.pair(t, 4097, 4, s=s4)
        u.put(t + 4, bytes([131 + rep]) * 2 + bytes([5]), fresh=False)
        u.put(t - 4097 + 4, bytes([6]), fresh=False)
    # * length - 5 would be cheaper and is not tried: 39 bytes (3 extra length bits; 38 .. 35 too, 34 has 2) whose last five are the
    #   first five of a 42-byte match from a nearer source (42 .. 37: 3 extra bits each).  39 + the rest of 37 costs what 38 + 38
    #   ... 35 + 41 cost; only 34 + 42 would save a bit
    t = 52000
    x34, y42 = low(34), low(42)
    u.put(t, x34 + y42)
    u.put(t - 700, x34 + y42[:5]); u.differ(t - 700 + 39, t + 39); u.differ(t - 701, t - 1)
    u.put(t + 34 - 300, y42); u.differ(t + 34 - 300 + 42, t + 76); u.differ(t + 34 - 301, t + 33)
    for k in range(40):
        t = 3000 + 400 * k
        u.pair(t, 300 + k, 8 + (k % 5), s=low(8 + (k % 5)))
    u.strategies = (Z_FIXED, Z_FILTERED)
    out.append(u)
    # the long-match flag: exactly one match of 65 and none longer, and its twin with 64
    for ln in (64, 65):
        u = Unit("prog_longest%d" % ln, "programme", 9000, 601)
        u.pair(5000, 700, ln)
        u.pair(2100, 50, 20)
        u.strategies = (Z_FIXED,)
        out.append(u)
    # long matches at a segment's first position, across 16-position chunk edges, in several segments at once; and the largest
    # acc[p + 1] - acc[p + 258]: 257 literals of cost 52 (bytes the sample never sees) under a 258-byte match
    u = Unit("prog_long_lanes", "programme", 2048 * 35, 602)
    for j in range(5, 17):                                   # sources in the even segments, targets in the odd ones
        off = (0, 1, 13, 14, 15, 16, 17, 2048 - 258, 700, 1000)[j % 10]
        ln = (258, 200, 66, 258, 129, 65, 258, 258, 100, 258)[j % 10]
        u.pair(2048 * (2 * j + 1) + off, 2048 + off - 600, ln, pre=off > 0)
    u.strategies = (Z_FIXED,)
    out.append(u)
    # acc[s0] beyond 65 536 (the kernel keeps acc modulo 2^16): 2 KiB of bytes that cost 52 each
    fill = bytearray(np.random.default_rng(603).integers(0, 128, size=70000).astype(np.uint8))
    # the sampled blocks see only bytes below 128 ...
    for b in range(273):
        if b & 3:                                            # ... every other block only bytes from 128 up: unseen, 52 quarter bits
            fill[256 * b:256 * b + 256] = np.random.default_rng(700 + b).integers(128, 256, size=256).astype(np.uint8).tobytes()
    u = Unit("prog_acc_wraps", "programme", 70000, 0, fill=bytes(fill[:70000]))
    u.rng = np.random.default_rng(604)
    u.pair(40000, 30000, 258)
    u.pair(2048 * 25 + 300, 257, 258)
    out.append(u)
    out.append(unit_acc_max(bytes(fill[:70000])))
    for x in out:
        x.levels, x.strategies = DP, (Z_FIXED, Z_FILTERED)
    return out


def units_parse():
    out = []
    # literal runs of 1 .. 7 in front of a match; runs that reach, and start one before, the chunk edges and the segment end; a
    # match that ends exactly on the segment end
    u = Unit("parse_runs", "parse", 20000, 701)                  # segments of 512
    w = u.string(12)                                             # one word; every copy matches the copy in front of it
    u.put(500, w)
    p = 2048
    for run in (1, 2, 3, 4, 5, 6, 7):
        for phase in range(3):
            u.put(p, w)
            p += 12 + run
            u.put(p, w)
            p += 12 + 29 + phase
    k = 0
    for edge in (32, 64, 480, 512):                              # literals from `back` in front of a chunk edge / the segment end up to it
        for back in (0, 1, 2, 3, 4):
            u.put(512 * (16 + k) + edge - back - 12, w)
            k += 1
    u.strategies = (Z_FIXED, Z_FILTERED)
    out.append(u)
    # entries of 3 .. 10 with one, two and three bytes between them: under Z_FILTERED 5 and below are literals, and the three-literal grouping runs over them
    u = Unit("parse_filtered", "parse", 20000, 702)
    p = 3000
    for rep in (1, 2, 3):
        for ln in (3, 4, 5, 6, 7, 8, 9, 10):
            u.pair(p, 900, ln, pre=False)
            p += ln + rep
    u.strategies = (Z_FIXED, Z_FILTERED)
    out.append(u)
    # a last segment of 1, 2 and 3 bytes; n = 1, 2, 3
    for n in (1, 2, 3, 32 * 3 + 1, 32 * 3 + 2, 32 * 3 + 3, 2048 * 3 + 1, 2048 * 3 + 2, 2048 * 3 + 3):
        u = Unit("parse_n%d" % n, "parse", n, 703 + n, flags=SEG2K if n > 2048 else 0)
        if n > 100:
            u.pair(n - 40, 30, 37 if n < 1000 else 30, pre=False)
        u.strategies = (Z_FILTERED,)
        out.append(u)
    for x in out:
        x.strategies = (Z_FIXED, Z_FILTERED)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# runs of dictionary-chained units
# ---------------------------------------------------------------------------------------------------------------------------
class Run:
    """one block that the engine cuts into units: data, flags, unit size, probes (positions are the block's)"""


def runs():
    out = []
    for name, n, flags, usize in (("run_3x128k_tail", 3 * 131072 + 10001, 0, 131072), ("run_units16k", 102400, UNITS16K, 16384)):
        u = Unit(name, "runs", n, 800 + usize)
        u.seg = 1 << 30                                          # (the builder's own segment notion is not used for runs)
        R = Run()
        R.name, R.flags, R.usize, R.probes = name, flags, usize, []
        for b in range(usize, n, usize):
            # distance 1 across the unit's edge: a run of one byte from b - 1 on, which the unit's first position copies
            u.put(b - 1, bytes([0x41 + b // usize]) * 21)
            u.differ(b - 2, b - 1); u.differ(b + 20, b + 19)
            R.probes.append(Probe("dist1_across_edge", b, {lv: (20, 1) for lv in ALL}))
            # distance 32768 from some 100 bytes behind the edge
            t = b + 100 + 21 * (b // usize)                       # (inside the unit's first segment: 256 bytes for a unit of 16 KiB)
            if t >= 32768:
                u.pair(t, 32768, 24)
                R.probes.append(Probe("dist32768_across_edge", t, {lv: (24, 32768) for lv in ALL}))
            if usize == 131072:
                # where goff + 32768 + p is a multiple of 40 960 (the link ring) and of 65 536 (the byte ring), goff = the unit's
                # offset in its run.  Such a p is a multiple of 2 048, a segment start, so no match lies across it: one 40-byte
                # match ends exactly there and one starts there, in every unit that holds such a position
                for m in (40960, 65536):
                    p = (-(b + 32768)) % m
                    while p < 3000:
                        p += m
                    if b + p + 40 > min(b + usize, n):
                        continue
                    for name, t, dist in (("ring%d_multiple_starts" % m, b + p, 6000), ("ring%d_multiple_ends" % m, b + p - 40, 5000)):
                        if not u.used[t]:                     # (in the run's third unit both multiples fall on one position)
                            u.pair(t, dist, 40, pre=name.endswith("ends"))
                        R.probes.append(Probe(name, t, {lv: (40, dist) for lv in ALL}))
        R.data = u.data
        out.append(R)
    return out


def units():
    """every single unit of the set (windows apart: units_windows; runs apart: runs)"""
    return ([unit_lengths(), unit_distances(), unit_selection(), unit_geometry()] + units_segment_ends() + units_dictionaries() +
            units_cost_stats() + units_programme() + units_parse())

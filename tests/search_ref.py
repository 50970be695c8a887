"""A plain referee of the encoder's search side (DESIGN.md 3.1 link tables, 3.2 search, 3.3 cost table, dynamic programme and
parse, 3.6 level table, 3.7 strategies), written from the text of DESIGN.md: Python and numpy.  It shares no form with
oracle/oracle_deflate.c or the kernels: links come from a stable sort of the buckets (no head array), the search lays out ALL
candidates of ALL positions as rows of (length, distance) and picks by one sort key (no running best), the programme works on
unbounded integers (no ring, no modulus), `shortest` solves the same problem forwards without any tie rule, and `check_entries`
knows nothing of the spec at all.  What anchors it is tests/test_cpu_search_ref.py.  Not a conftest: imported by the tests that
use it.

Entries are in the form zngamd_debug_fetch returns for stages 1 and 11: length << 16 | distance, 0 = no match."""
import numpy as np

import huffman_ref as H

WIN = 32768
MAX_MATCH = 258
BUCKET_BITS = 14
CONTEXT = (5, 3, 12)                              # bytes of context of tables A, B, C
K1, K2, K3 = 2654435761, 2246822519, 3266489917
NONE = 1 << 30                                    # "no limit"
WEAK_DIST = 256                                   # a 3-byte match farther back than this is literal-like (3.3)
SUB = 4                                           # the programme tries the length and its four next shorter ones

# 3.6: (chain steps over A, nice, cap, table C, dynamic programme, too_far3, too_far4)
LEVELS = {
    1: (1, 16, 16, False, False, 256, 4096), 2: (2, 16, 16, False, False, 256, 4096), 3: (3, 16, 16, False, False, 256, 4096),
    4: (2, 16, 16, False, True, 4096, NONE), 5: (2, 16, 16, True, True, 4096, NONE), 6: (3, 16, 16, True, True, 4096, NONE),
    7: (4, 32, 258, True, True, 4096, NONE), 8: (8, 64, 258, True, True, 4096, NONE), 9: (12, 128, 258, True, True, 4096, NONE),
}
SRC_B, SRC_C = 13, 14                             # `src` of a result: 1 .. 12 = the chain step that won, 13 = table B, 14 = table C
DROP_SHORT, DROP_FAR3, DROP_FAR4 = 1, 2, 3        # `drop` of a position without a result although a candidate shared 3 bytes


def seg_shift(n, flags=0):
    """log2 of a unit's segment size (3.3): 2 KiB for units above 64 KiB, for the flat header (2) and for SEG2K (16); else the
    smallest power of two from 32 up that covers the unit with 64 segments"""
    if (flags & (2 | 16)) or n > 65536:
        return 11
    s = 5
    while (64 << s) < n:
        s += 1
    return s


# ---------------------------------------------------------------------------------------------------------------------------
# 3.1 link tables
# ---------------------------------------------------------------------------------------------------------------------------
def _le32(a, off, count):
    a = a.astype(np.uint64)
    return a[off:off + count] | (a[off + 1:off + 1 + count] << 8) | (a[off + 2:off + 2 + count] << 16) | (a[off + 3:off + 3 + count] << 24)


def buckets(buf, table):
    """the bucket of every position of `buf` that has the table's whole context in front of the buffer's end (32-bit arithmetic,
    done in 64 bits and masked)"""
    a = np.frombuffer(bytes(buf), np.uint8)
    m = len(a) - CONTEXT[table] + 1
    if m <= 0:
        return np.zeros(0, np.uint32)
    M = np.uint64(0xFFFFFFFF)
    if table == 0:
        x = ((_le32(a, 0, m) * np.uint64(K1)) & M) ^ ((a[4:4 + m].astype(np.uint64) * np.uint64(K2)) & M)
    elif table == 1:
        w = a[0:m].astype(np.uint64) | (a[1:1 + m].astype(np.uint64) << 8) | (a[2:2 + m].astype(np.uint64) << 16)
        x = (w * np.uint64((K1 << 8) & 0xFFFFFFFF)) & M          # byte 3 could only reach bits above the 32 kept
    else:
        x = ((_le32(a, 0, m) * np.uint64(K1)) & M) ^ ((_le32(a, 4, m) * np.uint64(K2)) & M)
        x = (((x ^ (x >> np.uint64(15))) * np.uint64(K2)) & M) ^ ((_le32(a, 8, m) * np.uint64(K3)) & M)
    return (x >> np.uint64(32 - BUCKET_BITS)).astype(np.uint32)


def links(buf, dict_len, n, table):
    """link[i] for every position of dictionary + unit (u16): the distance to the nearest earlier position of the same bucket, if
    within 32 768 (the buffer starts at the dictionary's first byte, so nothing in front of it is ever seen); 0 otherwise and for
    positions with fewer bytes left than the context.  By grouping: a stable sort by bucket puts every bucket's positions side
    by side in rising order, and a position's nearest earlier one is its left neighbour."""
    assert len(buf) == dict_len + n
    out = np.zeros(dict_len + n, np.uint16)
    h = buckets(buf, table)
    if len(h) < 2:
        return out
    order = np.argsort(h, kind="stable")
    same = h[order[1:]] == h[order[:-1]]
    d = order[1:] - order[:-1]
    ok = same & (d <= WIN)
    out[order[1:][ok]] = d[ok]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# 3.2 search
# ---------------------------------------------------------------------------------------------------------------------------
def _common(a, pos, src, limit):
    """bytes that a[pos:] and a[src:] share, counted up to limit (arrays; limit <= 0: 0)"""
    out = np.zeros(len(pos), np.int64)
    idx = np.flatnonzero(limit > 0)
    j = 0
    while idx.size:
        idx = idx[a[pos[idx] + j] == a[src[idx] + j]]
        j += 1
        out[idx] = j
        idx = idx[limit[idx] > j]
    return out


class Search:
    """entries (u32, length << 16 | distance); src (0, or what found the result: 1 .. 12 the chain step, SRC_B, SRC_C); extended
    (the winner was extended beyond the compared bytes); drop (DROP_* where the winner was dropped); nice_stop (levels 7-9: the
    step behind which the walk stopped at a nice match, 0 where it did not); walked (candidates the chain walk gave);
    cand (rows x n lengths, -1 = no candidate) and cand_dist, rows = chain steps, then B, then C"""


def search(buf, dict_len, n, level, max_dist=WIN, sshift=None, flags=0):
    chain, nice_l, cap_l, use_c, _, too_far3, too_far4 = LEVELS[level]
    a = np.frombuffer(bytes(buf), np.uint8)
    assert len(a) == dict_len + n
    if sshift is None:
        sshift = seg_shift(n, flags)
    p = np.arange(n, dtype=np.int64)
    P = p + dict_len
    seg_end = np.minimum(((p >> sshift) + 1) << sshift, n)
    maxlen = np.minimum(MAX_MATCH, seg_end - p)
    searched = maxlen >= 3
    cap = np.minimum(cap_l, maxlen)
    nice = np.minimum(nice_l, cap)
    full = cap_l > 16                                              # levels 7-9: every candidate in full, walks stop at nice
    la = links(buf, dict_len, n, 0).astype(np.int64)
    lb = links(buf, dict_len, n, 1).astype(np.int64)
    lc = links(buf, dict_len, n, 2).astype(np.int64) if use_c else None
    rows = chain + 1 + (1 if use_c else 0)
    clen = np.full((rows, n), -1, np.int64)
    cdist = np.zeros((rows, n), np.int64)
    # the candidate list.  Chain A: `chain` steps, ended by a 0 link or by the first candidate beyond max_dist
    alive = searched.copy()
    going = searched.copy()                                        # levels 7-9: no nice match so far
    nice_stop = np.zeros(n, np.int64)
    q = P.copy()
    for k in range(chain):
        d = np.where(alive, la[q], 0)
        alive &= d != 0
        q = q - d
        dist = P - q
        alive &= dist <= max_dist
        take = alive & going
        i = np.flatnonzero(take)
        clen[k, i] = _common(a, P[i], q[i], cap[i])
        cdist[k, i] = dist[i]
        if full:
            hit = take & (clen[k] >= nice)
            nice_stop[hit] = k + 1
            going &= ~hit
    walked = (clen[:chain] >= 0).sum(axis=0)
    # tables B and C: the position's own link
    for r, lk, ctx in ((chain, lb, 3), (chain + 1, lc, 12)):
        if lk is None:
            continue
        d = lk[P]
        ok = searched & (d != 0) & (d <= max_dist)
        if full:                                                   # compared in full, skipped behind a nice match
            i = np.flatnonzero(ok & going)
            clen[r, i] = _common(a, P[i], P[i] - d[i], cap[i])
            cdist[r, i] = d[i]
            hit = np.zeros(n, bool)
            hit[i] = clen[r, i] >= nice[i]
            nice_stop[hit] = r + 1
            going &= ~hit
        else:                                                      # tested for the table's context only, and stands for exactly that
            i = np.flatnonzero(ok & (cap >= ctx))
            i = i[_common(a, P[i], P[i] - d[i], np.full(len(i), ctx)) == ctx]
            clen[r, i] = ctx
            cdist[r, i] = d[i]
    # the selection rule as one key: longer wins, nearer wins ties; (of two rows with the same length and distance the first)
    key = clen * (1 << 17) + (65536 - cdist)
    win = np.argmax(key, axis=0) if n else np.zeros(0, np.int64)
    wl = clen[win, p] if n else np.zeros(0, np.int64)
    wd = cdist[win, p] if n else np.zeros(0, np.int64)
    found = wl >= 3
    from_bc = found & (win >= chain)
    ext = found & ((wl == cap) | (from_bc & (not full)))
    i = np.flatnonzero(ext)
    tl = wl.copy()
    tl[i] = _common(a, P[i], P[i] - wd[i], maxlen[i])
    R = Search()
    R.extended = ext & (tl > wl)
    R.drop = np.zeros(n, np.int64)
    R.drop[(clen.max(axis=0) if n else wl) >= 0] = DROP_SHORT
    R.drop[found] = 0
    R.drop[found & (tl == 3) & (wd > too_far3)] = DROP_FAR3
    R.drop[found & (tl == 4) & (wd > too_far4)] = DROP_FAR4
    keep = found & (R.drop == 0)
    R.entries = np.where(keep, (tl << 16) | wd, 0).astype(np.uint32)
    R.src = np.where(found, np.where(win < chain, win + 1, np.where(win == chain, SRC_B, SRC_C)), 0)
    R.nice_stop, R.walked, R.cand, R.cand_dist = nice_stop, walked, clen, cdist
    R.links = (la, lb, lc)
    return R


# ---------------------------------------------------------------------------------------------------------------------------
# 3.3 cost table
# ---------------------------------------------------------------------------------------------------------------------------
_Q = [int(round(256 * 2 ** (k / 4))) for k in (1, 2, 3)]          # 304, 362, 431: the quotient's three thresholds


def ilog4(a, b):
    """floor(4 log2(a / b)) as 3.3 takes it: the quotient with 8 fraction bits, its leading bit, three thresholds"""
    q = (a << 8) // b
    assert q >= 256
    lg = q.bit_length() - 9
    t = q >> lg
    return 4 * lg + sum(t >= x for x in _Q)


class Costs:
    """table (258 integers: 256 literal costs, the match base 12 + bias + 20, 0), U, NM, hU"""


def cost_table(data, entries):
    data = np.frombuffer(bytes(data), np.uint8)
    e = np.asarray(entries, np.int64)
    n = len(data)
    p = np.arange(n)
    ln, dist = e >> 16, e & 0xFFFF
    lp = np.concatenate(([0], ln[:-1])) if n else ln               # the length in front; 0 in front of the unit
    sample = ((p >> 8) & 3) == 0
    lit_like = (ln == 0) | ((ln == 3) & (dist > WEAK_DIST))
    C = Costs()
    C.U = int((sample & lit_like).sum())
    C.NM = int((sample & ~lit_like & (ln + 1 != lp)).sum())
    C.hU = np.bincount(data[sample & lit_like], minlength=256).tolist()
    h = [16 * x + 1 + C.U // 64 for x in C.hU]
    T = sum(h)
    lbias = min(24, ilog4(C.U + C.NM, max(C.U, 1))) if C.U + C.NM else 0
    mbias = min(24, ilog4(C.U + C.NM, max(C.NM, 1))) if C.U + C.NM else 0
    C.table = [min(52, max(12, ilog4(T, h[b]) + lbias)) for b in range(256)] + [12 + mbias + 20, 0]
    return C


def fixed_costs(table=None):
    """Z_FIXED: the fixed code's costs in quarter bits -- 8 bits for the literals below 144, 9 for the others, 7 + 5 for a match
    before its extra bits; the rest of a table stays"""
    return [32] * 144 + [36] * 112 + [48] + (list(table[257:]) if table is not None else [0])


def match_cost(cost, length, dist):
    return cost[256] + 4 * H.LEN_EXTRA[H.len_code(length)] + 4 * H.DIST_EXTRA[H.dist_code(dist)]


def tried_lengths(length, dist, too_far3, min_len):
    """the lengths the programme tries for an entry, longest first"""
    lo = max(3, min_len, length - SUB)
    return [l for l in range(length, lo - 1, -1) if not (l == 3 and dist > too_far3)]


# ---------------------------------------------------------------------------------------------------------------------------
# 3.3 dynamic programme, and the same optimum as a shortest path
# ---------------------------------------------------------------------------------------------------------------------------
class Programme:
    """entries (rewritten), acc (n + 1 unbounded integers; acc[segment end] reads 0 from the segment in front of it), choice
    (per position: 0 literal, else 1 + how many bytes shorter than the entry), tie (0, or TIE_LITERAL: a match cost what the
    literal does; TIE_LENGTHS: two lengths cost the same and beat the literal)"""


TIE_LITERAL, TIE_LENGTHS = 1, 2


def programme(data, entries, cost, seg, too_far3=4096, min_len=3):
    data = bytes(data)
    n = len(data)
    e = [int(x) for x in entries]
    out = [0] * n
    acc = [0] * (n + 1)
    choice = [0] * n
    tie = [0] * n
    for s0 in range(0, n, seg):
        end = min(s0 + seg, n)
        nxt = {end: 0}                                             # acc of this segment alone
        for p in range(end - 1, s0 - 1, -1):
            lit = cost[data[p]] + nxt[p + 1]
            best, bl = lit, 0
            ln, dist = e[p] >> 16, e[p] & 0xFFFF
            if ln:
                cands = [(match_cost(cost, l, dist) + nxt[p + l], l) for l in tried_lengths(ln, dist, too_far3, min_len)]
                if cands:
                    mc = min(c for c, _ in cands)
                    ml = max(l for c, l in cands if c == mc)       # among matches the longest
                    if mc < lit:                                   # ties go to the literal
                        best, bl = mc, ml
                        if sum(1 for c, _ in cands if c == mc) > 1:
                            tie[p] = TIE_LENGTHS
                    elif mc == lit:
                        tie[p] = TIE_LITERAL
            nxt[p] = best
            acc[p] = best
            if bl:
                out[p] = (bl << 16) | dist
                choice[p] = 1 + ln - bl
        del nxt
    R = Programme()
    R.entries, R.acc, R.choice, R.tie = np.array(out, np.uint32), acc, choice, tie
    return R


def shortest(data, entries, cost, seg, too_far3=4096, min_len=3):
    """The cheapest way through each segment, as a shortest path over the graph "position -> position + 1 (a literal) or + l (a
    tried length)", relaxed forwards from the segment's start: no tie rule takes part.  -> [cost from each segment start]"""
    data = bytes(data)
    n = len(data)
    res = []
    for s0 in range(0, n, seg):
        end = min(s0 + seg, n)
        far = [None] * (end - s0 + 1)
        far[0] = 0
        for p in range(s0, end):
            here = far[p - s0]
            step = [(1, cost[data[p]])]
            ln, dist = int(entries[p]) >> 16, int(entries[p]) & 0xFFFF
            if ln:
                step += [(l, match_cost(cost, l, dist)) for l in tried_lengths(ln, dist, too_far3, min_len)]
            for l, c in step:
                t = p + l - s0
                if far[t] is None or here + c < far[t]:
                    far[t] = here + c
        res.append(far[end - s0])
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# 3.3 parse: the greedy walk, as tokens and as the kernels' token words
# ---------------------------------------------------------------------------------------------------------------------------
class Parse:
    """tokens (huffman_ref's form: an integer per literal, (length, distance) per match), words (per segment, the internal token
    words), counts (words per segment)"""


def tokens(data, entries, seg, min_len=3):
    data = bytes(data)
    n = len(data)
    ln = [(int(x) >> 16) if (int(x) >> 16) >= min_len else 0 for x in entries]      # Z_FILTERED: a shorter entry is a literal
    R = Parse()
    R.tokens, R.words, R.counts = [], [], []
    for s0 in range(0, n, seg):
        end = min(s0 + seg, n)
        words = []
        p = s0
        while p < end:
            if ln[p]:
                length, dist = ln[p], int(entries[p]) & 0xFFFF
                R.tokens.append((length, dist))
                lc, dc = H.len_code(length), H.dist_code(dist)
                words.append(0x80000000 | (lc << 26) | ((length - H.LEN_BASE[lc]) << 21) | (dc << 16) | (dist - H.DIST_BASE[dc]))
                p += length
                continue
            # a literal takes up to two following match-less positions into its word, up to the end of the 32-position chunk
            # (counted from the segment start) that holds its successor
            chunk_end = min(end, s0 + ((p + 1 - s0) // 32 + 1) * 32)
            group = [data[p]]
            p += 1
            while len(group) < 3 and p < chunk_end and not ln[p]:
                group.append(data[p])
                p += 1
            R.tokens += group
            words.append(sum(b << (8 * i) for i, b in enumerate(group)) | ((len(group) - 1) << 24))
        R.words.append(words)
        R.counts.append(len(words))
    return R


def replay(toks, zdict=b""):
    """the plaintext of a token sequence behind a dictionary"""
    out = bytearray(zdict)
    for t in toks:
        if isinstance(t, tuple):
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            out.append(t)
    return bytes(out[len(zdict):])


# ---------------------------------------------------------------------------------------------------------------------------
# what holds for ANY correct search
# ---------------------------------------------------------------------------------------------------------------------------
def check_entries(buf, dict_len, n, entries, max_dist=WIN, seg=2048):
    """-> None, or (position, what is wrong) of the first entry that no correct search could have written: a distance of 0, one
    beyond max_dist or in front of the dictionary; bytes that differ; a length above 258 or over the segment's end; a match
    that could go on (the next byte is equal, 258 is not reached, the segment is not at its end)"""
    a = np.frombuffer(bytes(buf), np.uint8)
    e = np.asarray(entries, np.int64)
    assert len(e) == n
    for p in np.flatnonzero(e >> 16):
        p = int(p)
        ln, dist = int(e[p]) >> 16, int(e[p]) & 0xFFFF
        end = min((p // seg + 1) * seg, n)
        if ln < 3:
            return p, "length %d" % ln
        if not 1 <= dist <= min(max_dist, p + dict_len):
            return p, "distance %d outside 1 .. %d" % (dist, min(max_dist, p + dict_len))
        if ln > MAX_MATCH or p + ln > end:
            return p, "length %d with %d bytes to the segment's end" % (ln, end - p)
        P = p + dict_len
        if not np.array_equal(a[P:P + ln], a[P - dist:P - dist + ln]):
            return p, "the %d bytes at distance %d differ" % (ln, dist)
        if ln < MAX_MATCH and p + ln < end and a[P + ln] == a[P - dist + ln]:
            return p, "length %d at distance %d could go on" % (ln, dist)
    return None


# ---------------------------------------------------------------------------------------------------------------------------
# one unit through every stage
# ---------------------------------------------------------------------------------------------------------------------------
Z_FILTERED, Z_FIXED = 1, 4


class Stages:
    """search (Search); costs (Costs: the estimated table, what stage 12 holds) and cost (the table the programme weighs: the
    fixed code's under Z_FIXED), prog (Programme) on levels 4 - 9, else None; entries (what the parse reads); parse (Parse);
    hist (320 integers in the layout of stage 4); plan (huffman_ref.Plan); out (the unit's bytes); long (a match longer than 64)"""


def encode(buf, dict_len, n, level, flags=0, max_dist=WIN, strategy=0):
    """DESIGN.md 3.1 - 3.5 and 3.7 for one unit of n > 0 bytes behind dict_len bytes of dictionary"""
    buf = bytes(buf)
    data = buf[dict_len:]
    sshift = seg_shift(n, flags)
    min_len = 6 if strategy == Z_FILTERED else 3
    R = Stages()
    R.seg = 1 << sshift
    R.search = search(buf, dict_len, n, level, max_dist, sshift)
    R.entries = R.search.entries
    R.costs = R.cost = R.prog = None
    R.long = bool(((R.search.entries >> 16) > 64).any())
    if LEVELS[level][4]:
        R.costs = cost_table(data, R.search.entries)
        R.cost = fixed_costs(R.costs.table) if strategy == Z_FIXED else R.costs.table
        R.prog = programme(data, R.search.entries, R.cost, R.seg, LEVELS[level][5], min_len)
        R.entries = R.prog.entries
    R.parse = tokens(data, R.entries, R.seg, min_len)
    hl, hd = H.token_hist(R.parse.tokens)
    R.hist = hl + [0, 0] + hd + [0, 0]
    R.plan = H.plan(hl, hd, n, final=bool(flags & 1), flat=bool(flags & 2), fixed_only=strategy == Z_FIXED)
    R.out = H.emit(R.plan, R.parse.tokens, data, final=bool(flags & 1), flat=bool(flags & 2))
    return R

"""A plain reference of the encoder's entropy plan and of its two search-free parses, written
from the text of DESIGN.md and RFC 1951: pure Python, explicit tree nodes, no numpy.  It shares no form with
oracle/oracle_deflate.c or the kernels (they build the lengths in place in one array, Moffat-Katajainen style); what anchors it is
tests/test_cpu_entropy_plan.py: the oracle's lengths, block types, end-of-block offsets and sizes, zlib's own Z_RLE and
Z_HUFFMAN_ONLY token sequences, and the package-merge optimum as a lower bound.  Not a conftest: imported by the tests that use it."""

LIMIT_L, LIMIT_D, LIMIT_CL = 10, 9, 7
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8        # RFC 1951 3.2.6 (288 symbols)
FIXED_D = [5] * 32


def len_code(length):
    """length 3..258 -> length code 0..28 (258 is code 28, not 27 + 31)"""
    if length == 258:
        return 28
    c = 27
    while LEN_BASE[c] > length:
        c -= 1
    return c


def dist_code(dist):
    c = 29
    while DIST_BASE[c] > dist:
        c -= 1
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# code lengths
# ---------------------------------------------------------------------------------------------------------------------------
class _Node:
    __slots__ = ("weight", "kids", "sym")

    def __init__(self, weight, kids=None, sym=None):
        self.weight, self.kids, self.sym = weight, kids, sym


def _ranked(freq):
    """the symbols in use, rarest first; equal counts by symbol index"""
    return sorted((s for s in range(len(freq)) if freq[s] > 0), key=lambda s: (freq[s], s))


def _leaves_per_depth(weights):
    """Huffman's algorithm with two queues over weights that are already sorted: the leaves in one, the merged nodes in the order
    they were made in the other.  The lighter head is taken; on equal weight the leaf, and of two merged nodes the older (it is
    in front of its queue anyway).  -> {depth: number of leaves}"""
    leaves = [_Node(w, sym=i) for i, w in enumerate(weights)]
    merged = []
    li = mi = 0

    def take():
        nonlocal li, mi
        if mi >= len(merged) or (li < len(leaves) and leaves[li].weight <= merged[mi].weight):
            li += 1
            return leaves[li - 1]
        mi += 1
        return merged[mi - 1]

    for _ in range(len(leaves) - 1):
        a = take()
        b = take()
        merged.append(_Node(a.weight + b.weight, kids=(a, b)))
    per = {}
    stack = [(merged[-1], 0)]
    while stack:
        node, d = stack.pop()
        if node.kids is None:
            per[d] = per.get(d, 0) + 1
        else:
            stack.append((node.kids[0], d + 1))
            stack.append((node.kids[1], d + 1))
    return per


def _fold(per, limit):
    """Count-based limiting: every leaf below the limit is counted at the limit, which over-subscribes the code space by some
    number of codes of the longest length.  Each step gives one of them back: a leaf leaves the longest length, and the longest
    code that is still shorter than the limit takes it as its sibling -- that code gets one bit longer (which frees exactly the
    space its new sibling takes), so the number of leaves stays and the Kraft sum falls by one unit of 2^-limit."""
    cnt = [0] * (limit + 1)
    for d, k in per.items():
        cnt[min(d, limit)] += k
    surplus = sum(cnt[d] << (limit - d) for d in range(1, limit + 1)) - (1 << limit)
    assert surplus >= 0
    for _ in range(surplus):
        cnt[limit] -= 1
        d = max(d for d in range(1, limit) if cnt[d])
        cnt[d] -= 1
        cnt[d + 1] += 2
    return cnt


def spec_lengths_depth(freq, limit):
    """-> (code length of every symbol, depth of the Huffman tree before limiting)"""
    lens = [0] * len(freq)
    order = _ranked(freq)
    if not order:
        return lens, 0
    if len(order) == 1:
        lens[order[0]] = 1
        return lens, 1
    per = _leaves_per_depth([freq[s] for s in order])
    cnt = _fold(per, limit)
    r = 0
    for length in range(limit, 0, -1):              # longest first, to the rarest
        for _ in range(cnt[length]):
            lens[order[r]] = length
            r += 1
    assert r == len(order)
    return lens, max(per)


def spec_lengths(freq, limit):
    return spec_lengths_depth(freq, limit)[0]


def canonical_codes(lens):
    """RFC 1951 3.2.2, then every code reversed within its length: the engine emits bits LSB first and stores the codes so"""
    mx = max(lens) if len(lens) else 0
    bl_count = [0] * (mx + 2)
    for ln in lens:
        if ln:
            bl_count[ln] += 1
    next_code = [0] * (mx + 2)
    code = 0
    for bits in range(1, mx + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = []
    for ln in lens:
        if not ln:
            out.append(0)
            continue
        c = next_code[ln]
        next_code[ln] += 1
        out.append(int(format(c, "0%db" % ln)[::-1], 2))
    return out


def cost_of(freq, lens):
    return sum(f * l for f, l in zip(freq, lens))


def optimal_cost(freq, limit):
    """The cheapest prefix code with no length above `limit`, by package-merge (Larmore & Hirschberg): `limit` rows of the sorted
    weights; the items of a row are paired into packages that join the row above; the 2 m - 2 lightest items of the top row are
    the answer, and their weights add up to sum(freq x length)."""
    w = sorted(f for f in freq if f > 0)
    m = len(w)
    if m == 0:
        return 0
    if m == 1:
        return w[0]
    assert (1 << limit) >= m
    row = list(w)
    for _ in range(limit - 1):
        packs = [row[i] + row[i + 1] for i in range(0, len(row) - 1, 2)]
        row = sorted(w + packs)
    return sum(row[:2 * m - 2])


# ---------------------------------------------------------------------------------------------------------------------------
# the header's code-length sequence
# ---------------------------------------------------------------------------------------------------------------------------
def cl_tokens(seq):
    """[(symbol, extra bits' value)] -- zeros: 138s first (code 18), then one 18 or 17 for a rest of 3 or more, else literal
    zeros; any other value: itself once, then 6s as code 16, then one 16 for a rest of 3 or more, else literals"""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        i = j
        if v == 0:
            while run >= 138:
                out.append((18, 138 - 11))
                run -= 138
            if run >= 11:
                out.append((18, run - 11))
            elif run >= 3:
                out.append((17, run - 3))
            else:
                out += [(0, 0)] * run
        else:
            out.append((v, 0))
            run -= 1
            while run >= 6:
                out.append((16, 6 - 3))
                run -= 6
            if run >= 3:
                out.append((16, run - 3))
            else:
                out += [(v, 0)] * run
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the plan of one unit
# ---------------------------------------------------------------------------------------------------------------------------
class Plan:
    """btype; ll_lens (286) / d_lens (30) / cl_lens (19) and their bit-reversed codes -- the fixed code's 288 / 32 lengths when
    btype is 1 --; hlit, hdist, hclen; header_bits (block header included; 0 for stored); eob_bit (bit offset of the end-of-block
    code); size (bytes of the unit, sync-flush tail included for a non-final one); cost_dyn, cost_fix, cost_sto (bits);
    depth_ll, depth_d, depth_cl (tree depths before limiting); dyn_* = the dynamic code whatever the block type."""


def stored_size(n, final):
    return n + 5 * ((n + 65534) // 65535) + (0 if final else 5)


def choose(cost_sto, cost_fix, cost_dyn, fixed_only=False):
    """the smallest; on equal cost stored before fixed before dynamic.  Z_FIXED: the same choice with the fixed block in the
    place of the dynamic one -- stored only where it beats both Huffman forms"""
    btype = min((cost_sto, 0), (cost_fix, 1), (cost_dyn, 2))[1]
    return 1 if fixed_only and btype == 2 else btype


def plan(hist_ll, hist_d, n, final=False, flat=False, fixed_only=False):
    """the plan of a unit of n > 0 bytes (an empty unit has no histogram and no plan)"""
    assert n > 0
    fl = [int(x) for x in hist_ll[:286]]
    fl += [0] * (286 - len(fl))
    fl[256] = 1                                                   # one end-of-block code per unit
    fd = [int(x) for x in hist_d[:30]]
    fd += [0] * (30 - len(fd))
    forced = list(fd)                                             # at least two distance codes, so that every decoder takes the set
    if sum(1 for f in forced if f) < 2 and forced[0] == 0:
        forced[0] = 1
    if sum(1 for f in forced if f) < 2:
        forced[1] = 1
    P = Plan()
    ll, P.depth_ll = spec_lengths_depth(fl, LIMIT_L)
    dl, P.depth_d = spec_lengths_depth(forced, LIMIT_D)
    P.hlit = max([257] + [s + 1 for s in range(286) if ll[s]])
    P.hdist = max([1] + [s + 1 for s in range(30) if dl[s]])
    seq = ll[:P.hlit] + dl[:P.hdist]
    toks = cl_tokens(seq)
    clf = [0] * 19
    for s, _ in toks:
        clf[s] += 1
    cl, P.depth_cl = spec_lengths_depth(clf, LIMIT_CL)
    P.hclen = max([4] + [i + 1 for i in range(19) if cl[CL_ORDER[i]]])
    P.dyn_ll_lens, P.dyn_d_lens, P.cl_lens, P.cl_tokens = ll, dl, cl, toks
    P.cl_codes = canonical_codes(cl)
    data_dyn = data_fix = 0
    for s in range(286):
        ex = LEN_EXTRA[s - 257] if s >= 257 else 0
        data_dyn += fl[s] * (ll[s] + ex)
        data_fix += fl[s] * (FIXED_LL[s] + ex)
    for s in range(30):
        data_dyn += fd[s] * (dl[s] + DIST_EXTRA[s])
        data_fix += fd[s] * (5 + DIST_EXTRA[s])
    if flat:
        hdr = 3 + 14 + 3 * 19 + 4 * (P.hlit + P.hdist)
    else:
        hdr = 3 + 14 + 3 * P.hclen + sum(cl[s] + CL_EXTRA.get(s, 0) for s, _ in toks)
    P.cost_dyn, P.cost_fix = hdr + data_dyn, 3 + data_fix
    P.cost_sto = 8 * (n + 5 * ((n + 65534) // 65535))
    P.btype = choose(P.cost_sto, P.cost_fix, P.cost_dyn, fixed_only)
    if P.btype == 2:
        P.ll_lens, P.d_lens, P.header_bits, bits = ll, dl, hdr, P.cost_dyn
        P.eob_bit = bits - ll[256]
    elif P.btype == 1:
        P.ll_lens, P.d_lens, P.header_bits, bits = list(FIXED_LL), list(FIXED_D), 3, P.cost_fix
        P.eob_bit = bits - 7
    else:
        P.ll_lens, P.d_lens, P.header_bits, bits, P.eob_bit = [0] * 286, [0] * 30, 0, 0, 0
    P.ll_codes, P.d_codes = canonical_codes(P.ll_lens), canonical_codes(P.d_lens)
    if P.btype == 0:
        P.size = stored_size(n, final)
    else:
        P.size = (bits + (0 if final else 3) + 7) // 8 + (0 if final else 4)      # `000`, pad, 00 00 FF FF behind a non-final unit
    return P


def token_hist(tokens):
    """(literal/length histogram of 286 with its one end-of-block code, distance histogram of 30) of a token sequence"""
    hl, hd = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            hl[257 + len_code(t[0])] += 1
            hd[dist_code(t[1])] += 1
        else:
            hl[t] += 1
    hl[256] = 1
    return hl, hd


# ---------------------------------------------------------------------------------------------------------------------------
# the search-free parses
# ---------------------------------------------------------------------------------------------------------------------------
def literal_tokens(data):
    """Z_HUFFMAN_ONLY: every byte a literal"""
    return list(bytes(data))


def rle_tokens(data, seg, prev=None):
    """Z_RLE, per segment of `seg` bytes: at p, with b the byte in front of p, a match of distance 1 when the
    three bytes at p all equal b; it lasts as long as the run of b does, at most 258 bytes and never past the segment's end.
    Anything else is a literal.  `prev`: the byte in front of the unit (the dictionary's last), or None."""
    data = bytes(data)
    out = []
    for s0 in range(0, len(data), seg):
        end = min(s0 + seg, len(data))
        p = s0
        while p < end:
            b = data[p - 1] if p > 0 else prev
            run = 0
            if b is not None:
                while run < 258 and p + run < end and data[p + run] == b:
                    run += 1
            if run >= 3:
                out.append((run, 1))
                p += run
            else:
                out.append(data[p])
                p += 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the unit's bytes: header, tokens, end of block, then the sync-flush marker or the final padding
# ---------------------------------------------------------------------------------------------------------------------------
class _BitsOut:
    def __init__(self):
        self.acc, self.n, self.buf = 0, 0, bytearray()

    def put(self, value, nbits):                    # LSB first (RFC 1951 3.1.1)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def pad(self):
        if self.n:
            self.put(0, 8 - self.n)


def _rev(v, nbits):
    return int(format(v, "0%db" % nbits)[::-1], 2) if nbits else 0


def emit(P, tokens, data, final=False, flat=False):
    """The bytes of a unit whose plan is P and whose tokens are `tokens` (`data`: its plaintext, for stored blocks)."""
    w = _BitsOut()
    n = len(data)
    if P.btype == 0:
        for off in range(0, n, 65535):
            piece = data[off:off + 65535]
            w.put(1 if final and off + len(piece) == n else 0, 3)
            w.pad()
            w.put(len(piece), 16)
            w.put(len(piece) ^ 0xFFFF, 16)
            w.buf += piece
    else:
        w.put((1 if final else 0) | (P.btype << 1), 3)
        if P.btype == 2:
            w.put(P.hlit - 257, 5)
            w.put(P.hdist - 1, 5)
            if flat:
                w.put(19 - 4, 4)
                for s in CL_ORDER:
                    w.put(4 if s < 16 else 0, 3)
                for v in P.ll_lens[:P.hlit] + P.d_lens[:P.hdist]:
                    w.put(_rev(v, 4), 4)             # the 4-bit code of symbol v is v itself; codes go out MSB first
            else:
                w.put(P.hclen - 4, 4)
                for s in CL_ORDER[:P.hclen]:
                    w.put(P.cl_lens[s], 3)
                for s, extra in P.cl_tokens:
                    w.put(P.cl_codes[s], P.cl_lens[s])
                    if s in CL_EXTRA:
                        w.put(extra, CL_EXTRA[s])
            assert len(w.buf) * 8 + w.n == P.header_bits
        for t in tokens:
            if isinstance(t, tuple):
                lc, dc = len_code(t[0]), dist_code(t[1])
                w.put(P.ll_codes[257 + lc], P.ll_lens[257 + lc])
                w.put(t[0] - LEN_BASE[lc], LEN_EXTRA[lc])
                w.put(P.d_codes[dc], P.d_lens[dc])
                w.put(t[1] - DIST_BASE[dc], DIST_EXTRA[dc])
            else:
                w.put(P.ll_codes[t], P.ll_lens[t])
        assert len(w.buf) * 8 + w.n == P.eob_bit
        w.put(P.ll_codes[256], P.ll_lens[256])
    if final:
        w.pad()
    else:
        w.put(0, 3)
        w.pad()
        w.buf += b"\x00\x00\xff\xff"
    assert len(w.buf) == P.size, (len(w.buf), P.size)
    return bytes(w.buf)

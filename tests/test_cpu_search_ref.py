"""The referee of the encoder's search side (tests/search_ref.py) and its built inputs (tests/search_inputs.py), proved without a
GPU: the referee equals the oracle at every stage the oracle exposes, on every built unit at levels 1 - 9 and on the inputs of the
stage-wise parity test; its programme reaches the optimum that a forward shortest path finds with no tie rule; its entries pass
the spec-free invariants, its tokens replay to the data and its bytes inflate with the system zlib under every strategy; every
probe gives, from the referee, the result it was built for; and the built set reaches every branch it names (the table is printed:
pytest -s)."""
import zlib

import numpy as np
import pytest

import deflate_walk as W
import search_inputs as I
import search_ref as S

UNITS = I.units()
BY_NAME = {u.name: u for u in UNITS}
WINDOWS = I.units_windows()
_memo = {}


def ref(u, level, strategy=0, wbits=15):
    key = (u.name, level, strategy, wbits)
    if key not in _memo:
        _memo[key] = S.encode(u.zdict + u.data, u.dict_len, u.n, level, u.flags, 1 << wbits, strategy)
    return _memo[key]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.lib()
    return oracle


def _against_oracle(O, R, data, zdict, level, flags, tag):
    n, dl = len(data), len(zdict)
    exp, crc, dbg = O.deflate_unit(data, zdict, level, flags, debug=True)
    assert S.seg_shift(n, flags) == O.seg_shift(n, flags), tag
    la, lb, lc = R.search.links
    for name, mine, key in (("A", la, "prevdist"), ("B", lb, "linkB"), ("C", lc, "linkC")):
        if mine is not None:
            assert np.array_equal(mine, dbg[key]), (tag, "links " + name, np.flatnonzero(mine != dbg[key])[:5])
    assert np.array_equal(R.search.entries, dbg["best"]), (tag, "search", np.flatnonzero(R.search.entries != dbg["best"])[:5])
    if R.prog is not None:
        assert R.costs.table == dbg["dp_cost"].tolist(), (tag, "cost table")
        assert np.array_equal(R.prog.entries, dbg["best_dp"]), (tag, "programme", np.flatnonzero(R.prog.entries != dbg["best_dp"])[:5])
    else:
        assert np.array_equal(R.entries, dbg["best_dp"]), tag
    nseg = len(R.parse.counts)
    assert R.parse.counts == dbg["seg_ntok"][:nseg].tolist() and not dbg["seg_ntok"][nseg:].any(), (tag, "token counts")
    for s in range(nseg):
        assert R.parse.words[s] == dbg["tokens"][s * R.seg:s * R.seg + R.parse.counts[s]].tolist(), (tag, "token words of segment", s)
    assert R.hist == dbg["hist"].tolist(), (tag, "histogram")
    assert R.plan.btype == dbg["btype"] and R.out == exp, (tag, "bytes")


@pytest.mark.parametrize("name", [u.name for u in UNITS])
def test_referee_equals_oracle_on_built_units(O, name):
    """every stage of every built unit, levels 1 - 9"""
    u = BY_NAME[name]
    for level in I.ALL:
        _against_oracle(O, ref(u, level), u.data, u.zdict, level, u.flags, (name, level))


@pytest.mark.parametrize("level", [1, 4, 6, 9])
def test_referee_equals_oracle_on_parity_inputs(O, fastq, level):
    """the inputs of tests/test_gpu_deflate_parity.py: FASTQ, zeros, random bytes, one period, every small size"""
    import test_gpu_deflate_parity as P
    for name, data in P._inputs(fastq).items():
        if data:
            _against_oracle(O, S.encode(data, 0, len(data), level), data, b"", level, 0, (name, level))


@pytest.mark.parametrize("wbits", [w for _, w in WINDOWS])
def test_windows_equal_oracle_stream(O, wbits):
    """window bits 9 - 14: the oracle takes a window only for a whole stream, which it cuts into units of 16 KiB behind their 32 KiB
    of dictionary; the referee's tokens of each unit, planned and emitted by huffman_ref, give the oracle's bytes"""
    u = next(x for x, w in WINDOWS if w == wbits)
    data = u.data
    for level in (1, 6, 9):
        exp = O.deflate_stream(data, level, 1, window_bits=wbits)
        got = b""
        for off in range(0, len(data), 16384):
            ul, dl = min(16384, len(data) - off), min(32768, off)
            fl = 1 if off + ul == len(data) else 0
            got += S.encode(data[off - dl:off + ul], dl, ul, level, fl, 1 << wbits).out
        assert got == exp, (wbits, level)
        assert zlib.decompress(exp, -wbits) == data


@pytest.mark.parametrize("name", [u.name for u in UNITS] + [u.name for u, _ in WINDOWS])
def test_probes_give_what_they_were_built_for(name):
    u, wb = (BY_NAME[name], 15) if name in BY_NAME else next((x, w) for x, w in WINDOWS if x.name == name)
    for level in u.levels:
        R = ref(u, level, 0, wb)
        assert S.check_entries(u.zdict + u.data, u.dict_len, u.n, R.search.entries, 1 << wb, u.seg) is None, (name, level)
        for pr in u.probes:
            if level in pr.expect:
                e = int(R.search.entries[pr.pos])
                assert ((e >> 16, e & 0xFFFF) if e else None) == pr.expect[level], (name, pr.name, pr.pos, level)


def test_run_probes():
    """the probes of the runs, from the referee run on each unit with the 32 KiB in front of it as dictionary"""
    for r in I.runs():
        n = len(r.data)
        for off in range(0, n, r.usize):
            ul, dl = min(r.usize, n - off), min(32768, off)
            for level in (1, 6, 9):
                Rs = S.search(r.data[off - dl:off + ul], dl, ul, level)
                assert S.check_entries(r.data[off - dl:off + ul], dl, ul, Rs.entries, seg=1 << S.seg_shift(ul)) is None
                for pr in r.probes:
                    if off <= pr.pos < off + ul:
                        e = int(Rs.entries[pr.pos - off])
                        assert ((e >> 16, e & 0xFFFF) if e else None) == pr.expect[level], (r.name, pr.name, pr.pos, level)


@pytest.mark.parametrize("name", [u.name for u in UNITS])
def test_optimum_and_replay(name):
    """acc[segment start] of the programme = the forward shortest path, for the estimated costs, the fixed code's and min_len 6;
    tokens replay to the data; plan + emit inflates with the system zlib; the strategy's own property holds"""
    u = BY_NAME[name]
    for level in (3, 6, 9):
        for strategy in (0, S.Z_FIXED, S.Z_FILTERED):
            R = ref(u, level, strategy)
            tag = (name, level, strategy)
            if R.prog is not None:
                min_len = 6 if strategy == S.Z_FILTERED else 3
                best = S.shortest(u.data, R.search.entries, R.cost, R.seg, S.LEVELS[level][5], min_len)
                assert best == [R.prog.acc[s0] for s0 in range(0, u.n, R.seg)], tag
            assert S.replay(R.parse.tokens, u.zdict) == u.data, tag
            d = zlib.decompressobj(-15, zdict=u.zdict) if u.zdict else zlib.decompressobj(-15)
            assert d.decompress(R.out) == u.data, tag
            if strategy and u.n <= 20000:                        # (the walker is pure Python)
                w = W.walk(R.out, window=u.zdict)
                assert w.out == u.data and W.check_strategy(w, strategy) is None, tag
                if w.blocks[0].btype:
                    assert w.tokens == R.parse.tokens, tag


# ---------------------------------------------------------------------------------------------------------------------------
# the branch table: no input may be there in name only
# ---------------------------------------------------------------------------------------------------------------------------
def branch_table():
    """{case: (unit, level or strategy, position)} from the referee's own outputs"""
    T = {}

    def note(case, unit, where, pos):
        T.setdefault(case, (unit, where, int(pos)))

    for u, wb in [(u, 15) for u in UNITS] + WINDOWS:
        for pr in u.probes:                                       # every probe is a case; that it holds is test_probes_...
            note(u.kind + ": " + pr.name, u.name, "levels " + "".join(str(l) for l in sorted(pr.expect)), pr.pos)
        for level in u.levels:
            R = ref(u, level, 0, wb)
            sr = R.search
            for k in range(1, 13):
                i = np.flatnonzero((sr.src == k) & (sr.entries != 0))
                if i.size:
                    note("search: chain step %d wins" % k, u.name, level, i[0])
            for what, code in (("B", S.SRC_B), ("C", S.SRC_C)):
                i = np.flatnonzero((sr.src == code) & (sr.entries != 0))
                if i.size:
                    note("search: table %s wins" % what, u.name, level, i[0])
                i = np.flatnonzero((sr.src == code) & sr.extended)
                if i.size:
                    note("search: a winner from %s is extended" % what, u.name, level, i[0])
            i = np.flatnonzero((sr.src > 0) & (sr.src <= 12) & sr.extended)
            if i.size:
                note("search: a winner at cap is extended", u.name, level, i[0])
            for what, code in (("too_far3", S.DROP_FAR3), ("too_far4", S.DROP_FAR4)):
                i = np.flatnonzero(sr.drop == code)
                if i.size:
                    note("search: dropped by %s (levels %s)" % (what, "1-3" if level <= 3 else "4-9"), u.name, level, i[0])
            i = np.flatnonzero(sr.nice_stop > 0)
            if i.size:
                note("search: walk stopped at nice = %d" % S.LEVELS[level][1], u.name, level, i[0])
            if R.prog is None:
                continue
            note("cost table: U = 0" if R.costs.U == 0 else "cost table: U > 0", u.name, level, 0)
            note("cost table: NM = 0" if R.costs.NM == 0 else "cost table: NM > 0", u.name, level, 0)
            if 52 in R.costs.table[:256] and R.costs.U:
                note("cost table: a byte outside the sample costs 52", u.name, level, R.costs.table.index(52))
            note("programme: long flag " + ("on" if R.long else "off"), u.name, level, 0)
            if int((sr.entries >> 16).max()) in (64, 65):
                note("programme: longest match is %d" % int((sr.entries >> 16).max()), u.name, level, int((sr.entries >> 16).argmax()))
            if max(R.prog.acc) > 65535:
                note("programme: acc[] beyond 65 535 (the modular values wrap)", u.name, level, int(np.argmax(R.prog.acc)))
            ln, dist = sr.entries >> 16, sr.entries & 0xFFFF
            pos = np.arange(u.n)
            sampled = ((pos >> 8) & 3) == 0
            i = np.flatnonzero(sampled[1:] & ((pos[1:] & 255) == 0) & (ln[1:] >= 3) & (ln[:-1] == ln[1:] + 1)) + 1
            if i.size:
                note("cost table: a run of decreasing lengths crosses into a sampled block", u.name, level, i[0])
            i = np.flatnonzero(sampled & (ln == 3) & (dist > S.WEAK_DIST))
            if i.size:
                note("cost table: a far 3-byte match inside the sample is literal-like", u.name, level, i[0])
            if u.name == "prog_acc_max" and level == 4:
                t = I.ACC_MAX_TARGET
                if int(ln[t]) == 258 and R.prog.acc[t + 1] - R.prog.acc[t + 258] == 257 * 52 and int(R.prog.entries[t]) >> 16 == 258:
                    note("programme: acc[p + 1] - acc[p + 258] = 257 x 52 under a 258-byte match that is taken", u.name, level, t)
        for strategy in (0,) + tuple(u.strategies):
            for level in (6,) if u.levels == I.ALL else (4, 6, 9):
                R = ref(u, level, strategy, wb)
                if R.prog is None:
                    continue
                sname = {0: "default", S.Z_FIXED: "Z_FIXED", S.Z_FILTERED: "Z_FILTERED"}[strategy]
                ch = np.array(R.prog.choice)
                has = (R.search.entries >> 16) > 0
                for c in range(6):
                    i = np.flatnonzero(has & (ch == c))
                    if i.size:
                        note("programme (%s): %s" % (sname, "the literal beats the match" if c == 0 else "length - %d chosen" % (c - 1)), u.name, level, i[0])
                tie = np.array(R.prog.tie)
                for t, what in ((S.TIE_LITERAL, "literal ties with a match"), (S.TIE_LENGTHS, "two lengths tie")):
                    i = np.flatnonzero(tie == t)
                    if i.size:
                        note("programme (%s): %s" % (sname, what), u.name, level, i[0])
                ln = R.search.entries >> 16
                if strategy == S.Z_FILTERED:
                    for l in range(3, 11):
                        i = np.flatnonzero(ln == l)
                        if i.size:
                            note("programme (Z_FILTERED): entry of %d" % l, u.name, level, i[0])
                if u.name == "prog_fixed_ties" and level == 6:
                    for what, kw in (("length - 5 would be cheaper and is not tried", dict(sub=5)),
                                     ("3 bytes beyond too_far3 would be cheaper and are not tried", dict(too_far3=S.NONE))):
                        i = np.flatnonzero(_programme_with(u, R, level, strategy, **kw) != R.prog.entries)
                        if i.size:
                            note("programme (%s): %s" % (sname, what), u.name, level, i[0])
                for l in (64, 65, 66, 128, 258):
                    i = np.flatnonzero((ln == l) & (ch > 0))
                    if i.size:
                        note("programme (%s): a match of %d taken" % (sname, l), u.name, level, i[0])
    return T


def _programme_with(u, R, level, strategy, sub=S.SUB, too_far3=None):
    """the programme's entries if it tried `sub` shorter lengths, or had another too_far3"""
    keep = S.SUB
    S.SUB = sub
    try:
        return S.programme(u.data, R.search.entries, R.cost, R.seg, S.LEVELS[level][5] if too_far3 is None else too_far3,
                           6 if strategy == S.Z_FILTERED else 3).entries
    finally:
        S.SUB = keep


# the probes every unit must carry (a builder that drops one fails here, not silently)
PROBES = {
    "lengths": ["len%d" % l for l in I.LENGTHS],
    "distances": ["dist%d_len20" % d for d in I.DISTANCES] + ["dist32769_none", "len3_dist256", "len3_dist257", "len3_dist4096", "len3_dist4097",
                                                              "len4_dist4096", "len4_dist4097", "len4_dist32768"],
    "selection": ["tie16_nearer", "longer_beyond16", "longer_within16"] + ["chain_step%d" % k for k in range(1, 14)] +
                 ["b_only", "b_nearer_than_a3", "b_same_as_a3", "c_only", "c_short_of_12", "bc_behind_nice"] +
                 ["nice%d_%s" % (n, w) for n in (32, 64, 128) for w in ("minus1", "exact")],
    "geometry": ["edge%d_%s" % (e, w) for e in (4096, 12288, 32768, 36864, 73728) for w in ("minus3", "minus2", "plus0", "plus1", "plus2", "plus3")] +
                ["walk_across_8192", "source_in_ring_pad", "source_across_ring_wrap"],
}
for _u in UNITS:
    if _u.kind == "segment_ends":
        PROBES[_u.name] = ["left%d_seg%d" % (k, _u.seg) for k in I.segment_end_lefts(_u.seg)]
    if _u.kind == "dictionaries":
        PROBES[_u.name] = ["source_at_dict_start"] + (["source_in_dict"] if _u.dict_len >= 100 else [])
for _u, _w in WINDOWS:
    PROBES[_u.name] = ["at_max_dist", "beyond_max_dist", "b_too_far", "c_too_far"]


def test_every_unit_carries_its_probes():
    for u in UNITS + [x for x, _ in WINDOWS]:
        want = PROBES.get(u.name)
        if want is not None:
            have = [pr.name for pr in u.probes]
            assert set(want) <= set(have), (u.name, sorted(set(want) - set(have)))
    assert {u.seg for u in UNITS if u.kind == "segment_ends"} == {32, 64, 256, 1024, 2048}
    for r in I.runs():
        names = {pr.name for pr in r.probes}
        assert {"dist1_across_edge", "dist32768_across_edge"} <= names and (r.usize != 131072 or {"ring40960_multiple_ends", "ring40960_multiple_starts", "ring65536_multiple_ends", "ring65536_multiple_starts"} <= names)


REQUIRED = (["search: chain step %d wins" % k for k in range(1, 13)] +
            ["search: table B wins", "search: table C wins", "search: a winner from B is extended", "search: a winner from C is extended",
             "search: a winner at cap is extended", "search: dropped by too_far3 (levels 1-3)", "search: dropped by too_far3 (levels 4-9)",
             "search: dropped by too_far4 (levels 1-3)", "search: walk stopped at nice = 32", "search: walk stopped at nice = 64",
             "search: walk stopped at nice = 128", "cost table: U = 0", "cost table: NM = 0", "cost table: a byte outside the sample costs 52",
             "programme: long flag on", "programme: long flag off", "programme: longest match is 64", "programme: longest match is 65",
             "programme: acc[] beyond 65 535 (the modular values wrap)",
             "programme: acc[p + 1] - acc[p + 258] = 257 x 52 under a 258-byte match that is taken",
             "cost table: a run of decreasing lengths crosses into a sampled block",
             "cost table: a far 3-byte match inside the sample is literal-like",
             "programme (Z_FIXED): length - 5 would be cheaper and is not tried",
             "programme (Z_FIXED): 3 bytes beyond too_far3 would be cheaper and are not tried"] +
            ["programme (default): " + ("the literal beats the match" if c == 0 else "length - %d chosen" % (c - 1)) for c in range(6)] +
            # (with the fixed code's constant costs a length is shortened only to meet a match that starts inside it, and then
            # shortening by one is as cheap as by more and the longer keeps the tie: lengths - 2 .. - 4 need estimated costs)
            ["programme (Z_FIXED): " + ("the literal beats the match" if c == 0 else "length - %d chosen" % (c - 1)) for c in range(3)] +
            ["programme (Z_FIXED): literal ties with a match", "programme (Z_FIXED): two lengths tie"] +
            ["programme (Z_FILTERED): entry of %d" % l for l in range(3, 11)] +
            ["programme (default): a match of %d taken" % l for l in (64, 65, 66, 128, 258)])


def test_branch_table():
    T = branch_table()
    for case in sorted(T):
        print("%-70s %s, %s, p = %d" % ((case,) + T[case]))
    missing = [c for c in REQUIRED if c not in T]
    assert not missing, missing
    kinds = {u.kind for u in UNITS} | {"windows"}
    assert kinds == {"lengths", "distances", "selection", "geometry", "segment_ends", "dictionaries", "windows", "cost_stats", "programme", "parse"}

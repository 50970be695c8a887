"""The encoder's search side on BUILT inputs: link tables (za_k_chains / za_k_chains2), search (za_k_search), cost statistics
(za_k_dpstats), dynamic programme (za_k_optparse) and parse (za_k_parse), through the C ABI under debug_keep, stage by stage
against the plain referee of DESIGN.md 3.1 - 3.3 / 3.6 / 3.7 (tests/search_ref.py, anchored on the CPU by
tests/test_cpu_search_ref.py) on the units of tests/search_inputs.py.  Nothing here comes from the oracle.

Per unit: debug_fetch 0 / 9 / 10 = the referee's links; the fetched search results (11; on levels 1 - 3 stage 1) first pass the
spec-free invariants (a failure names the probe it falls on), then equal the referee's, and every probe has the result it was
built for; 12 = the cost table; 1 = the programme's entries; 3 and 2 = the token counts and token words of every segment; 4 = the
histogram; the BYTES = huffman_ref's packing of the referee's tokens; the system zlib inflates them to the data and the CRC-32 is
the data's.  Under Z_FIXED and Z_FILTERED the same, the referee alone judging the bytes."""
import zlib

import numpy as np
import pytest

import search_inputs as I
import search_ref as S

pytestmark = pytest.mark.gpu

UNITS = I.units()
KINDS = sorted({u.kind for u in UNITS})
WINDOWS = I.units_windows()
GEOMETRY_LEVELS = (1, 3, 4, 6, 7, 9)
_memo = {}


def ref(u, level, strategy=0, wbits=15):
    key = (u.name, level, strategy, wbits)
    if key not in _memo:
        _memo[key] = S.encode(u.zdict + u.data, u.dict_len, u.n, level, u.flags, 1 << wbits, strategy)
    return _memo[key]


def _layout(units, aligns=None):
    """every unit's dictionary directly in front of it; the first dictionary starts at the buffer's first byte (no slack in front
    of it) and the last unit ends at the buffer's last; aligns[i]: the offset of unit i's first byte modulo 16"""
    buf = bytearray()
    blocks = []
    for i, u in enumerate(units):
        p = len(buf) + u.dict_len
        if aligns is not None and i > 0:
            p += (aligns[i] - p) % 16
        buf += b"\xee" * (p - u.dict_len - len(buf)) + u.zdict + u.data
        blocks.append((p, u.n, u.dict_len, u.flags))
    return bytes(buf), blocks


def _probe_at(u, p):
    for pr in u.probes:
        if pr.pos <= p < pr.pos + 300:
            return pr.name
    return None


def _check_unit(ctx, i, u, R, level, out, crc, tag, max_dist=32768, probes=None):
    """unit i of the last call against the referee's stages R"""
    n, dl = u.n, u.dict_len
    buf = u.zdict + u.data
    la, lb, lc = R.search.links
    for what, mine, name in ((0, la, "A"), (9, lb, "B"), (10, lc, "C")):
        if mine is not None:
            got = np.frombuffer(ctx.debug_fetch(what, i, 2 * (dl + n)), np.uint16)
            assert np.array_equal(got, mine), (tag, "links of table " + name, np.flatnonzero(got != mine)[:5])
    found = np.frombuffer(ctx.debug_fetch(11 if level >= 4 else 1, i, 4 * n), np.uint32)
    bad = S.check_entries(buf, dl, n, found, max_dist, R.seg)
    assert bad is None, (tag, "an entry no correct search could write", bad, _probe_at(u, bad[0]))
    for pr in (u.probes if probes is None else probes):
        if level in pr.expect:
            e = int(found[pr.pos])
            assert ((e >> 16, e & 0xFFFF) if e else None) == pr.expect[level], (tag, "probe", pr.name, pr.pos)
    diff = np.flatnonzero(found != R.search.entries)
    assert diff.size == 0, (tag, "search", diff[:5], [hex(int(found[j])) for j in diff[:5]], [hex(int(R.search.entries[j])) for j in diff[:5]],
                            _probe_at(u, int(diff[0])))
    if level >= 4:
        cost = np.frombuffer(ctx.debug_fetch(12, i, 4 * 258), np.uint32).tolist()
        assert cost == R.costs.table, (tag, "cost table", [(b, cost[b], R.costs.table[b]) for b in range(258) if cost[b] != R.costs.table[b]][:5])
        ent = np.frombuffer(ctx.debug_fetch(1, i, 4 * n), np.uint32)
        diff = np.flatnonzero(ent != R.entries)
        assert diff.size == 0, (tag, "programme", diff[:5], [hex(int(ent[j])) for j in diff[:5]], [hex(int(R.entries[j])) for j in diff[:5]])
    nseg = len(R.parse.counts)
    counts = np.frombuffer(ctx.debug_fetch(3, i, 4 * 64), np.uint32).tolist()
    assert counts[:nseg] == R.parse.counts, (tag, "token counts")
    words = np.frombuffer(ctx.debug_fetch(2, i, 4 * nseg * R.seg), np.uint32)
    for s in range(nseg):
        assert words[s * R.seg:s * R.seg + counts[s]].tolist() == R.parse.words[s], (tag, "token words of segment", s)
    hist = np.frombuffer(ctx.debug_fetch(4, i, 4 * 320), np.uint32).tolist()
    assert hist == R.hist, (tag, "histogram")
    assert out == R.out, (tag, "bytes")
    d = zlib.decompressobj(-15, zdict=u.zdict) if dl else zlib.decompressobj(-15)
    assert d.decompress(out) == u.data and (crc is None or crc == zlib.crc32(u.data)), tag


def _check_call(ctx, units, level, strategy=0, wbits=15, aligns=None):
    from zlib_ng_amd import _lib
    buf, blocks = _layout(units, aligns)
    if wbits != 15:
        blocks[0] = blocks[0][:3] + (blocks[0][3] | ((wbits & 15) << 8),)          # ZNGAMD_FLAG_WBITS on the call's first block
    assert ctx.L.zngamd_count_units(*_lib.block_table(blocks)) == len(units)       # one unit per block: debug_fetch's index
    cap = max(u.n for u in units) + max(u.n for u in units) // 8 + 1024
    ctx.debug_keep(True)
    try:
        outs, crcs, ovf = ctx.deflate_blocks(buf, blocks, level, cap, strategy=strategy)
        assert not ovf
        for i, u in enumerate(units):
            _check_unit(ctx, i, u, ref(u, level, strategy, wbits), level, outs[i], crcs[i], (u.name, level, strategy, aligns[i] if aligns else None),
                        1 << wbits)
    finally:
        ctx.debug_keep(False)


@pytest.mark.parametrize("level", I.ALL)
def test_selection_rules(ctx, level):
    """nearer / farther, longer within and beyond 16 bytes, the winner at every chain step, B only, B against A, C only, C short of
    its context, nice - 1 / nice: all nine levels"""
    _check_call(ctx, [u for u in UNITS if u.kind == "selection"], level)


@pytest.mark.parametrize("level", GEOMETRY_LEVELS)
@pytest.mark.parametrize("kind", ["lengths", "distances", "geometry", "segment_ends"])
def test_lengths_distances_geometry_segment_ends(ctx, kind, level):
    _check_call(ctx, [u for u in UNITS if u.kind == kind], level)


@pytest.mark.parametrize("level", GEOMETRY_LEVELS)
def test_dictionaries_at_every_alignment(ctx, level):
    """dictionaries of 0, 1, 3, 5, 100, 32767, 32768 bytes with a source at their first byte; the unit's first byte at every
    offset modulo 16; the first dictionary at the buffer's first byte, the last unit's end at the buffer's last"""
    units = [u for u in UNITS if u.kind == "dictionaries"]
    big = [u for u in units if u.dict_len >= 32767]
    small = [u for u in units if u.dict_len < 32767]
    for lot, aligns in ((big, range(0, 16, 5)), (small, range(16))):
        call, al = [], []
        for a in aligns:
            for u in lot:
                call.append(u)
                al.append(a)
        _check_call(ctx, call, level, aligns=al)
        _check_call(ctx, call[::-1], level, aligns=al[::-1])


@pytest.mark.parametrize("wbits", [w for _, w in WINDOWS])
def test_windows(ctx, wbits):
    """ZNGAMD_FLAG_WBITS(9 .. 14): sources at max_dist and one beyond, B and C candidates that are too far"""
    u = next(x for x, w in WINDOWS if w == wbits)
    for level in GEOMETRY_LEVELS:
        _check_call(ctx, [u], level, wbits=wbits)


GROUPS = ["cost_stats", "parse"] + [u.name for u in UNITS if u.kind == "programme"]      # (a programme unit a test: the referee's time)


@pytest.mark.parametrize("level", [4, 6, 9])
@pytest.mark.parametrize("group", GROUPS)
def test_cost_table_programme_parse(ctx, group, level):
    _check_call(ctx, [u for u in UNITS if group in (u.kind, u.name)], level)


@pytest.mark.parametrize("level", [1, 3])
def test_parse_greedy_levels(ctx, level):
    _check_call(ctx, [u for u in UNITS if u.kind == "parse"], level)


@pytest.mark.parametrize("level", [4, 6, 9])
@pytest.mark.parametrize("strategy", [S.Z_FIXED, S.Z_FILTERED], ids=["fixed", "filtered"])
@pytest.mark.parametrize("group", GROUPS[1:])
def test_strategies(ctx, group, strategy, level):
    """the programme and parse inputs under Z_FIXED (the programme weighs the fixed code's costs; stage 12 holds the estimated
    table) and Z_FILTERED (nothing below 6 bytes is tried or taken)"""
    _check_call(ctx, [u for u in UNITS if group in (u.kind, u.name)], level, strategy=strategy)


def test_filtered_greedy(ctx):
    """Z_FILTERED on a level without the programme: za_k_parse<true> alone turns the short entries into literals"""
    _check_call(ctx, [u for u in UNITS if u.kind == "parse"], 3, strategy=S.Z_FILTERED)


@pytest.mark.parametrize("level", GEOMETRY_LEVELS)
@pytest.mark.parametrize("which", [0, 1], ids=["3x128k_tail", "units16k"])
def test_runs(ctx, which, level):
    """one block that the engine cuts into dictionary-chained units (one workgroup per run carries rings and tables across them):
    every unit fetched by its index and compared with the referee run on the unit behind the 32 KiB in front of it"""
    from zlib_ng_amd import _lib
    r = I.runs()[which]
    n = len(r.data)
    blocks = [(0, n, 0, r.flags)]
    nunits = (n + r.usize - 1) // r.usize
    assert ctx.L.zngamd_count_units(*_lib.block_table(blocks)) == nunits
    ctx.debug_keep(True)
    try:
        outs, crcs, ovf = ctx.deflate_blocks(r.data, blocks, level, n + n // 8 + 1024)
        assert not ovf and crcs[0] == zlib.crc32(r.data)
        exp = b""
        for i, off in enumerate(range(0, n, r.usize)):
            ul, dl = min(r.usize, n - off), min(32768, off)
            key = (r.name, i, level)
            if key not in _memo:
                _memo[key] = S.encode(r.data[off - dl:off + ul], dl, ul, level)
            R = _memo[key]
            u = I.Unit.__new__(I.Unit)
            u.name, u.n, u.dict_len, u.a, u.probes = "%s[%d]" % (r.name, i), ul, dl, bytearray(r.data[off - dl:off + ul]), []
            probes = [I.Probe(pr.name, pr.pos - off, pr.expect) for pr in r.probes if off <= pr.pos < off + ul]
            u.probes = probes
            # the unit's own bytes: its slice of the block's output, cut by the referee's sizes (the CRC is the block's, above)
            _check_unit(ctx, i, u, R, level, outs[0][len(exp):len(exp) + len(R.out)], None, (u.name, level), probes=probes)
            exp += R.out
        assert outs[0] == exp, (r.name, level, "bytes")
        assert zlib.decompressobj(-15).decompress(outs[0]) == r.data
    finally:
        ctx.debug_keep(False)

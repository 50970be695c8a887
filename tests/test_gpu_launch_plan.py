"""GPU: the launch plan of the deflate pipeline -- launch sets sized by memory, run tiers sized from the slots of the chain
kernel and of the search.  None of it may change a byte: every chunking and every run plan gives the stream of the default
context, every table's links land in that table's row, and whole units across a tier boundary equal the oracle's.

The plan is read from the environment when a context is made (ZNGAMD_CHUNK_UNITS, ZNGAMD_CHAIN_RUN, ZNGAMD_CHAIN_SLOTS), so
every variant is a context of its own, closed when its test is through."""
import contextlib
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAN_ENV = ("ZNGAMD_CHUNK_UNITS", "ZNGAMD_CHAIN_RUN", "ZNGAMD_CHAIN_SLOTS")
N_SMALL, B_SMALL = 192, 4096           # the bench's block rule on small blocks: one unit each, the previous 32 KiB as dictionary
N_CARRY, B_UNIT = 12, 131072           # one block of twelve full units: every unit but the first carries its tables from the one in front


@contextlib.contextmanager
def _context(**env):
    """A context made under exactly these plan variables (all others of the plan unset); the environment is put back."""
    from zlib_ng_amd import _lib
    old = {k: os.environ.get(k) for k in PLAN_ENV}
    try:
        for k in PLAN_ENV:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        c = _lib.Context()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield c
    finally:
        c.close()


def _chained(n, bs):
    return [(i * bs, bs, min(32768, i * bs), 0) for i in range(n)]


def _packed(c, data, blocks, level=6):
    """-> (stream, sizes, crcs) of one packed call"""
    bs = max(b[1] for b in blocks)
    stream, crcs, ovf, lens = c.deflate_blocks(data, blocks, level, bs + bs // 8 + 1024, joined=True)
    assert not ovf
    return bytes(stream), list(lens), list(crcs)


@pytest.fixture(scope="module")
def small(fastq):
    """The 192 dict-chained 4 KiB blocks and what the default context makes of them (computed once)"""
    data = fastq[:N_SMALL * B_SMALL]
    blocks = _chained(N_SMALL, B_SMALL)
    with _context() as c:
        ref = _packed(c, data, blocks)
    return data, blocks, ref


@pytest.fixture(scope="module")
def small_links(small):
    """The oracle's three link tables of every small unit, levels 1 and 6: {level: [dbg of unit u]}"""
    from oracle import oracle as O
    data, blocks, _ = small
    return {lv: [O.deflate_unit(data[off:off + ln], data[off - dl:off], lv, 0, debug=True)[2] for off, ln, dl, _f in blocks] for lv in (1, 6)}


@pytest.fixture(scope="module")
def carry(fastq):
    """Twelve full units in one block, and the oracle's link tables of each at levels 1 and 6"""
    from oracle import oracle as O
    data = fastq[200000:200000 + N_CARRY * B_UNIT]
    units = [(u * B_UNIT, B_UNIT, min(32768, u * B_UNIT)) for u in range(N_CARRY)]
    links = {lv: [O.deflate_unit(data[off:off + ln], data[off - dl:off], lv, 0, debug=True)[2] for off, ln, dl in units] for lv in (1, 6)}
    return data, [(0, len(data), 0, 0)], units, links


def _check_links(c, data, blocks, units, links):
    """The own-position links (row index >= dictionary length) of every unit, every table the level has, against the oracle's.
    Table C exists from level 5 on (as in test_gpu_deflate_parity._stage_compare)."""
    c.debug_keep(True)
    try:
        for lv in (1, 6):
            bs = max(b[1] for b in blocks)
            _outs, _crcs, ovf = c.deflate_blocks(data, blocks, lv, bs + bs // 8 + 1024)
            assert not ovf
            for u, (_off, ln, dl) in enumerate(units):
                for what, key in ((0, "prevdist"), (9, "linkB"), (10, "linkC")) if lv >= 5 else ((0, "prevdist"), (9, "linkB")):
                    got = np.frombuffer(c.debug_fetch(what, u, 2 * (dl + ln)), np.uint16)[dl:]
                    exp = links[lv][u][key][dl:]
                    assert np.array_equal(got, exp), f"level {lv} unit {u} {key}: differs at {np.flatnonzero(got != exp)[:5]}"
    finally:
        c.debug_keep(False)


def test_same_bytes_under_any_chunking(small):
    """One set (the default), three even sets of 64, and sets of 50 with a short last one: same stream, unit sizes and CRCs."""
    data, blocks, ref = small
    for ch in (64, 50):
        with _context(ZNGAMD_CHUNK_UNITS=ch) as c:
            assert _packed(c, data, blocks) == ref, f"ZNGAMD_CHUNK_UNITS={ch}"
    stream, sizes, crcs = ref
    assert sum(sizes) == len(stream)
    assert zlib.decompress(stream + b"\x03\x00", -15) == data
    assert crcs == [zlib.crc32(data[off:off + ln]) for off, ln, _dl, _f in blocks]


@pytest.mark.parametrize("env", [{"ZNGAMD_CHAIN_SLOTS": 4}, {"ZNGAMD_CHAIN_RUN": 1}, {"ZNGAMD_CHAIN_RUN": 3}, {"ZNGAMD_CHAIN_RUN": 8}],
                         ids=lambda e: "-".join(f"{k[7:].lower()}{v}" for k, v in e.items()))
def test_run_tiers(small, small_links, carry, env):
    """Every run plan -- the three tiers within one set (four slots: runs of 8, of 2, single units over 192 units) and fixed runs
    of 1, 3 and 8 -- gives the default context's bytes, and the chain launches write every table to its own row.  The 4 KiB
    blocks are too short to carry tables from unit to unit, so the links are also checked on twelve full units of one block,
    where a run carries (one slot: a run of 6, then single units; fixed runs of 3 and of 8)."""
    data, blocks, ref = small
    with _context(**env) as c:
        assert _packed(c, data, blocks) == ref
        _check_links(c, data, blocks, [(off, ln, dl) for off, ln, dl, _f in blocks], small_links)
    cdata, cblocks, cunits, clinks = carry
    cenv = {"ZNGAMD_CHAIN_SLOTS": 1} if "ZNGAMD_CHAIN_SLOTS" in env else env
    with _context() as c:
        cref = _packed(c, cdata, cblocks)
    with _context(**cenv) as c:
        assert _packed(c, cdata, cblocks) == cref
        _check_links(c, cdata, cblocks, cunits, clinks)


def test_whole_units_across_a_tier_boundary(fastq):
    """24 dict-chained blocks of 128 KiB, `mixed` and `zeros` in turn, planned for one slot: a run of 8, runs of 2 up to unit 22,
    two single units -- both tier boundaries fall inside the 24.  Every block equals the oracle's unit."""
    from oracle import oracle as O
    rng = np.random.default_rng(7)                 # the `mixed` and `zeros` inputs of test_gpu_deflate_parity._inputs
    zeros = bytes(B_UNIT)
    rng.bytes(B_UNIT)
    mixed = fastq[:40000] + rng.bytes(30000) + bytes(20000) + fastq[50000:91072]
    assert len(mixed) == B_UNIT
    data = b"".join(mixed if b % 2 == 0 else zeros for b in range(24))
    blocks = _chained(24, B_UNIT)
    with _context(ZNGAMD_CHAIN_SLOTS=1) as c:
        outs, crcs, ovf = c.deflate_blocks(data, blocks, 6, B_UNIT + B_UNIT // 10 + 500)
    assert not ovf
    assert zlib.decompress(b"".join(outs) + b"\x03\x00", -15) == data
    exp = {}
    for (off, ln, dl, _fl), crc, out in zip(blocks, crcs, outs):
        assert crc == zlib.crc32(data[off:off + ln])
        key = (off // B_UNIT % 2, dl)          # (the units repeat: `mixed` behind `zeros` and the other way round, and the first without a dictionary)
        if key not in exp:
            exp[key] = O.deflate_unit(data[off:off + ln], data[off - dl:off], 6, 0)[0]
        assert out == exp[key], f"block at {off}"


def test_small_call_is_one_set(small):
    """No ZNGAMD_CHUNK_UNITS and a call far below what memory allows: nothing is halved, the call is one launch set -- the last
    unit's stages are resident, which they are only for a single set."""
    data, blocks, ref = small
    with _context() as c:
        assert _packed(c, data, blocks) == ref
        entries = np.frombuffer(c.debug_fetch(1, N_SMALL - 1, 4 * B_SMALL), np.uint32)
        assert entries.size == B_SMALL
    with _context(ZNGAMD_CHUNK_UNITS=64) as c:      # (and the check does tell: three sets are not resident)
        from zlib_ng_amd import _lib
        _packed(c, data, blocks)
        with pytest.raises(_lib.EngineError):
            c.debug_fetch(1, N_SMALL - 1, 4 * B_SMALL)

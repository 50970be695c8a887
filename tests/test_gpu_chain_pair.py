"""GPU: the chain kernel that builds two link tables from one staging of the input (za_k_chains2).  It must leave every link of
every table, and so every output byte, as the one-table launches left them: all three link tables of every unit against the
oracle's, and the final bytes, at the sizes where the pair kernel takes another path -- around the three context lengths,
around a group of 1 024 positions, around the prefetch depth of four groups -- with dictionaries of every kind, on data that
puts every lane of an insert into one bucket of both tables at once (zeros), and over runs that carry both tables from unit
to unit or are cut in the middle.  Everything goes through the C ABI, as in test_gpu_deflate_parity."""
import contextlib
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIN = 32768
UNIT_LENS = (1, 4, 5, 11, 12, 13, 1023, 1024, 1025, 4095, 4096, 4097, 5123)
DICT_LENS = (0, 1, 100, 32767, 32768)
LEVELS = (1, 4, 5, 6, 9)               # 1 and 4: tables A and B only; 5, 6, 9: with C
KINDS = ("zeros", "period36", "random", "fastq")
PLAN_ENV = ("ZNGAMD_CHUNK_UNITS", "ZNGAMD_CHAIN_RUN", "ZNGAMD_CHAIN_SLOTS")
TABLES = ((0, "prevdist"), (9, "linkB"), (10, "linkC"))


def _tables(level):
    return TABLES if level >= 5 else TABLES[:2]


@pytest.fixture(scope="module")
def sources(fastq):
    """Per kind of data: 32 KiB that serve as dictionaries and, behind them, the bytes of the longest unit"""
    n = WIN + max(UNIT_LENS)
    rng = np.random.default_rng(11)
    return {"zeros": bytes(n), "period36": (b"abcdefghijklmnopqrstuvwxyz0123456789" * (n // 36 + 1))[:n],
            "random": rng.bytes(n), "fastq": fastq[1000:1000 + n]}


def _compare_units(c, data, blocks, level, units, own_only):
    """One deflate call with the stages kept; every unit's link tables and every block's bytes against the oracle.
    units: (block, offset, length, dictionary length) of every unit in the order of the call; own_only: compare the unit's own
    positions only (a carried unit's dictionary links live in the row of the unit in front of it)."""
    from oracle import oracle as O
    cap = max(b[1] for b in blocks)
    c.debug_keep(True)
    try:
        outs, crcs, ovf = c.deflate_blocks(data, blocks, level, cap + cap // 8 + 1024)
        assert not ovf
        exp_out = [b""] * len(blocks)
        for u, (b, off, ln, dl) in enumerate(units):
            exp, _crc, dbg = O.deflate_unit(data[off:off + ln], data[off - dl:off], level, 0, debug=True)
            exp_out[b] += exp
            lo = dl if own_only else 0
            for what, key in _tables(level):
                got = np.frombuffer(c.debug_fetch(what, u, 2 * (dl + ln)), np.uint16)[lo:]
                want = dbg[key][lo:]
                assert np.array_equal(got, want), f"level {level} unit {u} (length {ln}, dictionary {dl}) {key}: differs at {np.flatnonzero(got != want)[:5]}"
    finally:
        c.debug_keep(False)
    for b, (off, ln, _dl, _f) in enumerate(blocks):
        assert outs[b] == exp_out[b], f"level {level} block {b}: bytes differ"
        assert crcs[b] == zlib.crc32(data[off:off + ln])


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("kind", KINDS)
def test_links_and_bytes_at_every_edge(ctx, sources, kind, level):
    """Every unit length with every dictionary length as the units of one call: each unit is a block of its own that starts
    at byte 32 768 of the source (the blocks overlap in the input, which is only read)."""
    data = sources[kind]
    blocks = [(WIN, n, dl, 0) for dl in DICT_LENS for n in UNIT_LENS]
    _compare_units(ctx, data, blocks, level, [(b, off, ln, dl) for b, (off, ln, dl, _f) in enumerate(blocks)], own_only=False)


@contextlib.contextmanager
def _context(**env):
    """A context made under exactly these plan variables; the environment is put back (as in test_gpu_launch_plan)."""
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


def _chained(n, bs, unchained=None):
    """n blocks of bs bytes, each with what lies in front of it (up to 32 KiB) as its dictionary; `unchained` has none"""
    return [(i * bs, bs, 0 if i == unchained else min(WIN, i * bs), 0) for i in range(n)]


@pytest.mark.parametrize("unchained", [None, 2], ids=["chained", "cut_at_2"])
@pytest.mark.parametrize("run", [1, 2, 1000])
def test_runs_of_short_units(fastq, run, unchained):
    """Five dict-chained units of 3 000 bytes under fixed run lengths, and with the third not chained to the second."""
    data = fastq[5000:5000 + 5 * 3000]
    blocks = _chained(5, 3000, unchained)
    units = [(b, off, ln, dl) for b, (off, ln, dl, _f) in enumerate(blocks)]
    with _context(ZNGAMD_CHAIN_RUN=run) as c:
        for level in LEVELS:
            _compare_units(c, data, blocks, level, units, own_only=False)


@pytest.mark.parametrize("unchained", [None, 2], ids=["chained", "cut_at_2"])
@pytest.mark.parametrize("run", [1, 2, 1000])
def test_runs_that_carry_both_tables(fastq, run, unchained):
    """Four units of 32 KiB, each the whole dictionary of the next: the shortest units whose tables a run carries over, so the
    late inserts at a unit's head (4 positions for A, 2 for B, 11 for C) start at a different place for each table of a pair.
    With the third unit not chained the run is cut in the middle and both tables start afresh there."""
    data = fastq[300000:300000 + 4 * WIN]
    blocks = _chained(4, WIN, unchained)
    units = [(b, off, ln, dl) for b, (off, ln, dl, _f) in enumerate(blocks)]
    with _context(ZNGAMD_CHAIN_RUN=run) as c:
        for level in LEVELS:
            _compare_units(c, data, blocks, level, units, own_only=True)


def test_carried_zeros(ctx):
    """The same four carried units, all zeros: every lane of every insert of both tables in one bucket each, across units."""
    data = bytes(4 * WIN)
    blocks = _chained(4, WIN)
    units = [(b, off, ln, dl) for b, (off, ln, dl, _f) in enumerate(blocks)]
    for level in (1, 6):
        _compare_units(ctx, data, blocks, level, units, own_only=True)

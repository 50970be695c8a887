"""BGZF sort (bgzf.sort_key_records, sort_keys, permute_records, sort_records; csrc/za_sort.hip) through the C ABI and the Python API.
The referee is sort_ref.py: the key bytes from the statement of the encoding, the order from parsed values, np.lexsort for rows of any
origin -- never the code under test.  Everything is compared for equality: every key byte, every length, every place of every row,
every byte of every output.  That the referee's two orders agree on the inputs is asserted on the CPU (test_cpu_bgzf_sort.py)."""
import functools
import gzip

import numpy as np
import pytest

import sort_inputs as I
import sort_ref as R
from test_cpu_bgzf_sort import PRESETS, golden_records
from test_gpu_bgzf_grep import block_map
from test_gpu_bgzf_lines import BGZIP, member_table

pytestmark = pytest.mark.gpu

BASE = 700                                                   # record_base of the calls through the C ABI


# ---- the sort
@functools.lru_cache(maxsize=None)
def want_order(pattern, n, w):
    return R.lexorder(I.rows(pattern, n, w))


def check_order(got, want, what):
    got = np.asarray(got, np.int64)
    if not np.array_equal(got, want):
        at = np.nonzero(got != want)[0] if len(got) == len(want) else []
        raise AssertionError((what, "order differs", len(got), len(want), list(at[:8]), got[at[:8]].tolist() if len(at) else None, want[at[:8]].tolist() if len(at) else None))


@pytest.mark.parametrize("w", I.WIDTHS)
@pytest.mark.parametrize("pattern", I.PATTERNS)
def test_sort_patterns(ctx, pattern, w):
    """every size around a wave and a tile, through the C ABI (odd sizes) and the Python API (even ones); rank is the inverse"""
    from zlib_ng_amd import bgzf
    sizes = I.SIZES + ((10000,) if pattern == "two_keys" else ())
    for n in sizes:
        k = I.rows(pattern, n, w)
        want = want_order(pattern, n, w)
        if n % 2:
            order, rank = ctx.sort_keys(k, True)
            assert order.dtype == np.uint32 and rank.dtype == np.uint32
        else:
            order, rank = bgzf.sort_keys(k, rank=True)
            assert order.dtype == np.int64 and rank.dtype == np.int64
        check_order(order, want, (pattern, w, n))
        assert np.array_equal(np.asarray(rank, np.int64)[want], np.arange(n)), (pattern, w, n)
        if pattern == "equal":
            assert np.array_equal(want, np.arange(n))                              # every digit skipped: the identity
    assert np.array_equal(bgzf.sort_keys(I.rows(pattern, 300, w)), want_order(pattern, 300, w))      # (without the rank)


@pytest.mark.parametrize("pattern", ["random", "two_keys", "carry"])
def test_sort_scan_carries(ctx, pattern):
    """more tiles than the scan kernel takes in one turn: its sum is carried into a second turn"""
    n, w = I.SCAN_TURN + I.TILE + 1, 8
    k = I.rows(pattern, n, w)
    order, _ = ctx.sort_keys(k)
    check_order(order, R.lexorder(k), (pattern, n))


def test_sort_device_forms(ctx):
    """the work area sized by zngamd_sort_scratch_bytes, to the byte; one byte less is BUF_ERROR and nothing is written; the rows stay"""
    from zlib_ng_amd import _lib, devmem
    L = _lib.load()
    for n, w, pattern in ((2 * I.TILE + 1, 16, "random"), (I.TILE, 256, "carry"), (65, 8, "byte_last"), (5000, 8, "equal")):
        k = I.rows(pattern, n, w)
        want = R.lexorder(k)
        need = int(L.zngamd_sort_scratch_bytes(n, w))
        assert need == (4 * n + 7) // 8 * 8 + (n + 7) // 8 * 8 + 1024 * ((n + I.TILE - 1) // I.TILE) + 1024 + 2 * w
        d_keys = devmem.from_host(ctx, k.tobytes())
        d_area = devmem.from_host(ctx, b"\xa5" * (need + 8))
        d_order, d_rank = devmem.from_host(ctx, b"\xa5" * (4 * (n + 1))), devmem.from_host(ctx, b"\xa5" * (4 * (n + 1)))
        code = ctx.sort_keys_dev(d_keys.ptr, n, w, d_area.ptr, need - 1, d_order.ptr, d_rank.ptr)
        assert code == _lib.BUF_ERROR and d_area.cpu().tobytes() == b"\xa5" * (need + 8) and d_order.cpu().tobytes() == b"\xa5" * (4 * (n + 1))
        code = ctx.sort_keys_dev(d_keys.ptr, n, w, d_area.ptr, need, d_order.ptr, 0)      # without the rank
        assert code == 0 and d_rank.cpu().tobytes() == b"\xa5" * (4 * (n + 1))
        o = d_order.cpu().tobytes()
        assert o[4 * n:] == b"\xa5" * 4 and d_area.cpu().tobytes()[need:] == b"\xa5" * 8
        check_order(np.frombuffer(o[:4 * n], np.uint32), want, (pattern, n, w))
        code = ctx.sort_keys_dev(d_keys.ptr, n, w, d_area.ptr, need, d_order.ptr, d_rank.ptr)
        assert code == 0
        o, r = d_order.cpu().tobytes(), d_rank.cpu().tobytes()
        assert o[4 * n:] == r[4 * n:] == b"\xa5" * 4 and d_area.cpu().tobytes()[need:] == b"\xa5" * 8
        check_order(np.frombuffer(o[:4 * n], np.uint32), want, (pattern, n, w))
        assert np.array_equal(np.frombuffer(r[:4 * n], np.uint32)[want], np.arange(n))
        assert d_keys.cpu().tobytes() == k.tobytes()                               # (the rows are read, never written)
    assert ctx.sort_keys_dev(0, 0, 8, 0, 0, 0, 0) == 0                             # no row: nothing is launched
    for bad in (dict(w=12), dict(n=(1 << 30) + 1)):
        with pytest.raises(_lib.EngineError):
            ctx.sort_keys_dev(d_keys.ptr, bad.get("n", 5), bad.get("w", 8), d_area.ptr, need, d_order.ptr, 0)


# ---- the keys
def packed_of(text, block_size=4099):
    from zlib_ng_amd import bgzf
    blob = bgzf.compress(text, block_size=block_size)
    tab, _ = block_map(blob)
    return blob, member_table(tab)


def conf_of(cf):
    from zlib_ng_amd import _lib
    kinds = {"bytes": _lib.BGZF_SORT_BYTES, "number": _lib.BGZF_SORT_NUMBER, "length": _lib.BGZF_SORT_LENGTH}
    c = _lib.BgzfSortConf(cf.record_lines, -1 if cf.first_byte is None else cf.first_byte[0], -1 if cf.meta is None else cf.meta[0], len(cf.parts))
    for i, p in enumerate(cf.parts):
        flags = (_lib.BGZF_SORT_REVERSE if p.reverse else 0) | (_lib.BGZF_SORT_IGNORE_CASE if p.ignore_case else 0) | (_lib.BGZF_SORT_TRUNCATE if p.truncate else 0)
        c.part[i] = _lib.BgzfSortPart(p.line, -1 if p.column is None else p.column, p.width, p.first, flags, kinds[p.kind], p.sep[0])
    return c


@functools.lru_cache(maxsize=None)
def table_text(**variant):
    recs = I.table(**variant)
    text = b"".join(recs)
    return (recs, text) + packed_of(text)


def engine(ctx, blob, members, nbytes, cf, flags, caps=None):
    return ctx.bgzf_sort_key_records(blob, members, 0, nbytes, cf.delimiter[0], flags, conf_of(cf), BASE, caps)


def check_rows(res, recs, cf, text_len, short_lines=0, what=None):
    code, status, tot, rows, lens = res
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.seen, tot.bytes_in, tot.tail_off, tot.short_lines, tot.key_width) == \
        (1, 0, len(recs), text_len, text_len, short_lines, R.width_of(cf)), what
    assert lens.dtype == np.uint32 and lens.tolist() == R.lengths(list(recs), cf), what
    want = R.encode(list(recs), cf)
    assert rows.shape == want.shape, what
    if not np.array_equal(rows, want):
        at = np.nonzero((rows != want).any(axis=1))[0]
        raise AssertionError((what, "keys differ at records", at[:10].tolist(), rows[at[0]].tolist(), want[at[0]].tolist()))


@pytest.mark.parametrize("name", list(I.GRID))
def test_key_grid(ctx, name):
    """every key byte and every length against the referee: the plain table; meta lines in front and in the middle; a short last record; a
    last line without its delimiter, which the length counts"""
    from zlib_ng_amd import _lib
    F = _lib.BGZF_GREP_FINAL
    for variant in (dict(), dict(meta=True), dict(short_last=True), dict(open_last=True), dict(meta=True, short_last=True, open_last=True)):
        recs, text, blob, members = table_text(**variant)
        cf = I.grid_conf(name, meta=b"#" if variant.get("meta") else None)
        check_rows(engine(ctx, blob, members, len(text), cf, F), recs, cf, len(text), 1 if variant.get("short_last") else 0, (name, variant))
    # without _FINAL the open record behind the last whole one stays for the next call
    recs, text, blob, members = table_text(short_last=True)
    cf = I.grid_conf(name)
    whole = len(text) - len(recs[-1])
    code, status, tot, rows, lens = engine(ctx, blob, members, len(text), cf, 0)
    assert code == 0 and (tot.seen, tot.bytes_in, tot.tail_off, tot.short_lines, tot.bad) == (len(recs) - 1, whole, whole, 0, 0)
    assert np.array_equal(rows, R.encode(list(recs[:-1]), cf)) and lens.tolist() == [len(r) for r in recs[:-1]]


def test_key_numbers_and_edges(ctx):
    """the numbers one by one; fields of exactly width and width + 1; first inside and beyond the field; other delimiters and separators"""
    from zlib_ng_amd import _lib
    F = _lib.BGZF_GREP_FINAL
    cf = R.conf([R.part(0, 1, kind="number"), R.part(0, 0, width=8)], record_lines=1)
    good = [b"a\t0\n", b"b\t007\n", b"c\t18446744073709551615\n", b"abcdefgh\t" + b"0" * 200 + b"18446744073709551615\n", b"\t5\n", b"d\t1\tmore\tcolumns\n"]
    text = b"".join(good)
    blob, members = packed_of(text)
    check_rows(engine(ctx, blob, members, len(text), cf, F), good, cf, len(text))
    for bad_rec, kind in ((b"e\t18446744073709551616\n", 2), (b"e\t28446744073709551615\n", 2), (b"e\t184467440737095516150\n", 2), (b"e\t12a\n", 2), (b"e\t\n", 2),
                          (b"e\n", 2), (b"e\t-1\n", 2), (b"e\t 1\n", 2), (b"abcdefghi\t1\n", 3)):
        recs = good[:3] + [bad_rec] + good[3:] + [bad_rec]
        t = b"".join(recs)
        b, m = packed_of(t)
        code, status, tot, rows, lens = engine(ctx, b, m, len(t), cf, F)
        assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (kind, BASE + 3, len(b"".join(good[:3])), len(recs), 1), bad_rec
        assert rows.shape == (0, 16) and len(lens) == 0 and (tot.max_field == 9 if kind == 3 else True)
        with pytest.raises(R.Fault) as e:
            R.encode(recs, cf)
        assert (e.value.kind, e.value.record) == (kind, 3)
    # of two faults the smallest record's; at one record the lower number; the first byte before both
    recs = [b"a\t1\n"] * 300
    recs[200], recs[77], recs[250] = b"a\tx\n", b"abcdefghij\t1\n", b"abcdefghijkl\t1\n"
    t = b"".join(recs)
    b, m = packed_of(t)
    code, status, tot, rows, lens = engine(ctx, b, m, len(t), cf, F)
    assert (tot.bad, tot.bad_record, tot.max_field) == (3, BASE + 77, 12)
    recs[77] = b"abcdefghij\tx\n"
    t = b"".join(recs)
    b, m = packed_of(t)
    assert [getattr(engine(ctx, b, m, len(t), cf, F)[2], x) for x in ("bad", "bad_record")] == [2, BASE + 77]
    tot = engine(ctx, b, m, len(t), cf._replace(first_byte=b"a"), F)[2]
    assert (tot.bad, tot.bad_record) == (2, BASE + 77)
    recs[40] = b"z\t1\n"
    t = b"".join(recs)
    b, m = packed_of(t)
    tot = engine(ctx, b, m, len(t), cf._replace(first_byte=b"a"), F)[2]
    assert (tot.bad, tot.bad_record, tot.bad_src) == (1, BASE + 40, 40 * 4)
    # another delimiter, another separator, a CR is a field byte, three lines per record
    for text, c2 in ((b"x;y z;q;" * 3, R.conf([R.part(1, 1, b" ", width=8), R.part(2, kind="length")], record_lines=3, delimiter=b";")),
                     (b"n 1\r\nn 02\r\n", R.conf([R.part(0, 1, b" ", width=8)], record_lines=1)),
                     (b">s\nAC\n>t\nGT", R.conf([R.part(1, width=8, reverse=True)], record_lines=2))):
        b, m = packed_of(text)
        check_rows(engine(ctx, b, m, len(text), c2, F), R.split(text, c2), c2, len(text), 0, text)


def test_key_capacity_and_device_form(ctx):
    from zlib_ng_amd import _lib, devmem
    F = _lib.BGZF_GREP_FINAL
    recs, text, blob, members = table_text(open_last=True)
    cf = I.grid_conf("four parts")
    n, nb, w = len(recs), len(text), R.width_of(cf)
    code, status, tot, rows, lens = engine(ctx, blob, members, nb, cf, F, caps=n - 1)
    assert code == _lib.BUF_ERROR and rows.shape == (0, w) and len(lens) == 0 and (tot.seen, tot.bad, tot.key_width) == (n, 0, w)
    check_rows(engine(ctx, blob, members, nb, cf, F, caps=n), recs, cf, nb)
    check_rows(engine(ctx, blob, members, nb, cf, F, caps=n + 9), recs, cf, nb)
    for flags in (1, 2, 8, 16):
        with pytest.raises(_lib.EngineError):
            engine(ctx, blob, members, nb, cf, flags)
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    d_rows, d_len = devmem.from_host(ctx, b"\xa5" * (w * (n + 1))), devmem.from_host(ctx, b"\xa5" * (4 * (n + 1)))

    def keys_dev(rcap, c=cf, rows=d_rows.ptr):
        return ctx.bgzf_sort_key_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, nb, 10, F, conf_of(c), BASE, d_scratch.ptr, nb, d_st.ptr, rows,
                                             d_len.ptr, rcap)

    code, tot = keys_dev(n - 1)
    assert code == _lib.BUF_ERROR and (tot.seen, tot.bad) == (n, 0) and d_rows.cpu().tobytes() == b"\xa5" * (w * (n + 1)) and d_len.cpu().tobytes() == b"\xa5" * (4 * (n + 1))
    # a fault together with a short destination: the fault wins -- the code is OK, the totals name the record, nothing is written.  (The
    # table's records share no first byte, so none is overwritten: the first record that does not begin as record 0 does is at fault.)
    fb = recs[0][:1]
    j = next(i for i, r in enumerate(recs) if r[:1] != fb)
    code, tot = keys_dev(n - 1, cf._replace(first_byte=fb))
    assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (1, BASE + j, len(b"".join(recs[:j])), n)
    assert d_rows.cpu().tobytes() == b"\xa5" * (w * (n + 1)) and d_len.cpu().tobytes() == b"\xa5" * (4 * (n + 1))
    code, tot = keys_dev(n)
    assert code == 0 and (tot.seen, tot.bytes_in, tot.tail_off, tot.covered, tot.key_width) == (n, nb, nb, 1, w)
    got, gl = d_rows.cpu().tobytes(), d_len.cpu().tobytes()
    assert got[w * n:] == b"\xa5" * w and gl[4 * n:] == b"\xa5" * 4
    assert np.array_equal(np.frombuffer(got[:w * n], np.uint8).reshape(n, w), R.encode(list(recs), cf))
    assert np.frombuffer(gl[:4 * n], np.uint32).tolist() == R.lengths(list(recs), cf)
    # no part: the lengths alone, and no rows are asked for
    d_len[:] = 0xA5
    code, tot = keys_dev(n, I.grid_conf("none"), 0)
    assert code == 0 and (tot.seen, tot.key_width) == (n, 0) and np.frombuffer(d_len.cpu().tobytes()[:4 * n], np.uint32).tolist() == R.lengths(list(recs), cf)
    assert d_rows.cpu().tobytes() == got


# ---- place and the files
def small_windows(monkeypatch):
    from zlib_ng_amd import bgzf
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)


@functools.lru_cache(maxsize=None)
def reads(n=1500, open_last=False):
    rng = np.random.default_rng(17)
    recs = [b"@r%d %d\n%s\n+\n%s\n" % (int(rng.integers(0, 1 << 30)), i, I._word(rng, int(rng.integers(30, 120))), b"F" * 5) for i in range(n)]
    if open_last:
        recs[-1] = recs[-1][:-1]
    return tuple(recs)


def unzip(path):
    return gzip.decompress(open(path, "rb").read())


def test_permute_records(ctx, tmp_path, monkeypatch):
    """the identity, the reversal, a random permutation, a subset, an empty order, a record larger than chunk_bytes; by path and by reader,
    with and without lengths; the last line's delimiter is added wherever the record lands"""
    from zlib_ng_amd import bgzf
    small_windows(monkeypatch)
    cf = R.conf(record_lines=4)
    recs = list(reads(open_last=True))
    big = b"@big\n" + b"A" * 9000 + b"\n+\n" + b"F" * 9000 + b"\n"
    recs[700] = big
    n = len(recs)
    text = b"".join(recs)
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    out_recs = R.written(recs, cf)
    ctx.bgzf_stats()
    keys = bgzf.sort_key_records(src, [], allow_short=True)
    assert ctx.bgzf_stats()[0] >= 3                                                    # (several windows)
    assert keys.lengths.tolist() == R.lengths(recs, cf) and keys.keys.shape == (n, 0) and keys.records == n
    rng = np.random.default_rng(3)
    chunk = len(text) // 4                                                         # 5 buckets or so; the big record alone overflows none, the tiny chunk below does
    orders = {"identity": np.arange(n), "reversal": np.arange(n)[::-1], "random": rng.permutation(n), "subset": rng.permutation(n)[:n // 3],
              "last first": np.array([n - 1, 0, 700]), "empty": np.empty(0, np.int64)}
    for i, (name, order) in enumerate(orders.items()):
        out = str(tmp_path / (name.replace(" ", "_") + ".gz"))
        want = b"".join(out_recs[j] for j in order)
        if i % 2:
            got = bgzf.permute_records(src, order, out, lengths=keys.lengths, chunk_bytes=chunk, compresslevel=1)
        else:
            with bgzf.open(src) as r:
                at = r.tell()
                got = r.permute_records(order.tolist(), out, chunk_bytes=chunk, compresslevel=1)
                assert r.tell() == at
        assert got == (len(order), len(want)) and unzip(out) == want, name
        assert open(out, "rb").read().endswith(bgzf.EOF_BLOCK)
    assert len(bgzf._permute_buckets(keys.lengths[orders["random"]], chunk)) >= 3
    out = str(tmp_path / "tiny.gz")                                                # a chunk smaller than a record: every bucket takes one record
    order = np.array([700, 3, n - 1, 0])
    assert bgzf.permute_records(src, order, out, lengths=keys.lengths, chunk_bytes=64, compresslevel=1)[0] == 4
    assert unzip(out) == b"".join(out_recs[j] for j in order)
    # a lengths array with one wrong entry; one record too few, one too many; an order beyond the file
    wrong = keys.lengths.copy()
    wrong[431] += 1
    with pytest.raises(ValueError, match=r"record 431 at virtual offset \d+: its length is not lengths\[431\].*incomplete"):
        bgzf.permute_records(src, np.arange(n), out, lengths=wrong, chunk_bytes=chunk)
    with pytest.raises(ValueError, match=r"the file holds 1500 records and lengths has 1499 entries: the files are out of step.*incomplete"):
        bgzf.permute_records(src, np.arange(n - 1), out, lengths=keys.lengths[:-1], chunk_bytes=chunk)
    with pytest.raises(ValueError, match=r"the file holds 1500 records and lengths has 1501 entries: the files are out of step"):
        bgzf.permute_records(src, np.arange(n), out, lengths=np.append(keys.lengths, 5), chunk_bytes=chunk)
    with pytest.raises(ValueError, match=r"order\[1\] is 1500: a record number lies between 0 and 1499"):
        bgzf.permute_records(src, [0, n], out, chunk_bytes=chunk)
    with pytest.raises(ValueError, match=r"record 0 at virtual offset 0 does not start with b'>' \(first_byte\)"):
        bgzf.permute_records(src, [5], out, first_byte=b">", lengths=keys.lengths)


def test_place_through_the_c_abi(ctx):
    """dst and length as the caller gives them: skipped records, a record that does not fit, arrays that are too short; nothing is written
    outside the places"""
    from zlib_ng_amd import _lib, devmem
    F = _lib.BGZF_GREP_FINAL
    cf = R.conf(record_lines=4)
    recs = list(reads(200, open_last=True))
    text = b"".join(recs)
    blob, members = packed_of(text)
    lens = np.array(R.lengths(recs, cf), np.uint32)
    n = len(recs)
    pick = np.array([199, 5, 77, 0])
    dst = np.full(n, _lib.BGZF_PLACE_SKIP, np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens[pick])])
    dst[pick] = offs[:-1] + 8                                                      # eight bytes in front stay as they are
    cap = int(offs[-1]) + 8
    d_out = devmem.from_host(ctx, b"\xa5" * (cap + 8))
    want = b"\xa5" * 8 + b"".join(R.written(recs, cf)[j] for j in pick) + b"\xa5" * 8
    code, status, tot = ctx.bgzf_place_records(blob, members, 0, len(text), 10, F, 4, ord("@"), BASE, dst, lens, d_out.ptr, cap)
    assert code == 0 and not status.any() and (tot.seen, tot.placed, tot.placed_bytes, tot.bad, tot.labels_short, tot.covered, tot.tail_off) == \
        (n, 4, int(offs[-1]), 0, 0, 1, len(text))
    assert d_out.cpu().tobytes() == want
    # one byte less room: the record that ends last does not fit, the others are placed
    d_out[:] = 0xA5
    code, status, tot = ctx.bgzf_place_records(blob, members, 0, len(text), 10, F, 4, -1, BASE, dst, lens, d_out.ptr, cap - 1)
    assert (tot.bad, tot.bad_record, tot.placed) == (5, BASE + 0, 3) and d_out.cpu().tobytes()[int(dst[0]):] == b"\xa5" * (cap + 8 - int(dst[0]))
    # the first byte: fault 1, also at a record that is skipped
    code, status, tot = ctx.bgzf_place_records(blob, members, 0, len(text), 10, F, 4, ord("+"), BASE, dst, lens, d_out.ptr, cap)
    assert (tot.bad, tot.bad_record, tot.bad_src) == (1, BASE + 0, 0)
    # a wrong length: fault 4 at the smallest such record
    bad = lens.copy()
    bad[77] -= 1
    bad[199] += 2
    code, status, tot = ctx.bgzf_place_records(blob, members, 0, len(text), 10, F, 4, -1, BASE, dst, bad, d_out.ptr, cap)
    assert (tot.bad, tot.bad_record, tot.bad_src, tot.placed) == (4, BASE + 77, len(b"".join(recs[:77])), 2)
    # arrays shorter than the records: nothing is written; longer ones are no fault
    d_out[:] = 0xA5
    code, status, tot = ctx.bgzf_place_records(blob, members, 0, len(text), 10, F, 4, -1, BASE, dst[:-1], lens[:-1], d_out.ptr, cap)
    assert (tot.labels_short, tot.placed, tot.seen, tot.bad) == (1, 0, n, 0) and d_out.cpu().tobytes() == b"\xa5" * (cap + 8)
    code, status, tot = ctx.bgzf_place_records(blob, members, 0, len(text), 10, F, 4, -1, BASE, np.append(dst, np.uint64(0)), np.append(lens, np.uint32(1)), d_out.ptr, cap)
    assert (tot.labels_short, tot.placed, tot.bad) == (0, 4, 0) and d_out.cpu().tobytes() == want
    # the device form
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, len(text)), devmem.empty(ctx, 4 * len(members))
    d_dst, d_len = devmem.from_host(ctx, dst.tobytes()), devmem.from_host(ctx, lens.tobytes())
    d_out[:] = 0xA5
    code, tot = ctx.bgzf_place_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, len(text), 10, F, 4, ord("@"), BASE, d_scratch.ptr, len(text), d_st.ptr,
                                           d_dst.ptr, d_len.ptr, n, d_out.ptr, cap)
    assert code == 0 and (tot.seen, tot.placed, tot.placed_bytes, tot.bad) == (n, 4, int(offs[-1]), 0) and d_out.cpu().tobytes() == want


def preset_order(recs, name):
    return R.order(recs, PRESETS[name])


@pytest.mark.parametrize("name", ["name", "sequence", "length"])
def test_sort_records_golden(ctx, tmp_path, name):
    from zlib_ng_amd import bgzf
    recs = golden_records()
    want = preset_order(recs, name)
    out = str(tmp_path / "sorted.fq.gz")
    res = bgzf.sort_records(BGZIP, out, name, first_byte=b"@", compresslevel=1)
    assert res.order.tolist() == want and (res.records, res.bytes, res.key_width) == (len(recs), sum(map(len, recs)), R.width_of(PRESETS[name]))
    assert unzip(out) == b"".join(recs[i] for i in want)
    keys = bgzf.sort_key_records(BGZIP, name)
    assert np.array_equal(keys.keys, R.encode(recs, PRESETS[name])) and keys.lengths.tolist() == [len(r) for r in recs]
    if name == "length":                                                           # reverse: the longest first, ties in input order
        res = bgzf.sort_records(BGZIP, out, name, reverse=True, compresslevel=1)
        cf = PRESETS[name]._replace(parts=tuple(p._replace(reverse=True) for p in PRESETS[name].parts))
        assert res.order.tolist() == R.order(recs, cf)


def test_sort_vcf_then_tabix(ctx, tmp_path, monkeypatch):
    """an unsorted VCF becomes one that TabixIndex.build accepts; header lines stay in front and in order; fetch returns what a filter
    over the text returns"""
    from zlib_ng_amd import bgzf
    small_windows(monkeypatch)
    head, body = I.vcf()
    recs = list(head) + list(body)
    src, out = str(tmp_path / "calls.vcf.gz"), str(tmp_path / "sorted.vcf.gz")
    open(src, "wb").write(bgzf.compress(b"".join(recs), block_size=5000))
    with pytest.raises(ValueError):
        bgzf.TabixIndex.build(src, "vcf")                                          # (unsorted: the index refuses it)
    want = preset_order(recs, "vcf")
    res = bgzf.sort_records(src, out, "vcf", chunk_bytes=len(b"".join(recs)) // 3, compresslevel=1)
    assert res.order.tolist() == want and res.key_width == 40
    text = unzip(out)
    assert text == b"".join(recs[i] for i in want) and text.startswith(b"".join(head))
    idx = bgzf.TabixIndex.build(out, "vcf")
    assert sorted(idx.names) == [b"chr1", b"chr10", b"chr2"] or sorted(idx.names) == ["chr1", "chr10", "chr2"]
    regions = [("chr1", 0, 3000), ("chr10", 100000, 250000), ("chr2", 3999, 4000)]
    got = bgzf.fetch(out, idx, regions)
    lines = [x + b"\n" for x in text.split(b"\n") if x and not x.startswith(b"#")]
    for i, (name, beg, end) in enumerate(regions):
        hit = [x for x in lines if x.split(b"\t")[0] == name.encode() and beg < int(x.split(b"\t")[1]) <= end]
        assert got.of(i) == hit and (len(hit) > 0), regions[i]


def test_paired_recipe(ctx, tmp_path, monkeypatch):
    """R1 sorted by name, R2 permuted by R1's order: mate i stays next to mate i"""
    from zlib_ng_amd import bgzf
    small_windows(monkeypatch)
    r1 = list(reads(600))
    r2 = [r.split(b"\n")[0] + b"/2\nTTTT\n+\nFFFF\n" for r in r1]
    p1, p2, o1, o2 = (str(tmp_path / x) for x in ("r1.gz", "r2.gz", "o1.gz", "o2.gz"))
    open(p1, "wb").write(bgzf.compress(b"".join(r1), block_size=5000))
    open(p2, "wb").write(bgzf.compress(b"".join(r2), block_size=5000))
    res = bgzf.sort_records(p1, o1, "name", first_byte=b"@", compresslevel=1)
    assert res.order.tolist() == preset_order(r1, "name")
    assert bgzf.permute_records(p2, res.order, o2, first_byte=b"@", compresslevel=1) == (600, sum(map(len, r2)))
    a, b = I.fastq_records(unzip(o1)), I.fastq_records(unzip(o2))
    assert len(a) == len(b) == 600 and all(y.startswith(x.split(b"\n")[0] + b"/2\n") for x, y in zip(a, b))
    assert [x.split(b" ")[0] for x in a] == sorted(x.split(b" ")[0] for x in r1)
    with pytest.raises(ValueError, match="out of step"):                           # a mate file that lost a read
        open(p2, "wb").write(bgzf.compress(b"".join(r2[:-1]), block_size=5000))
        bgzf.permute_records(p2, res.order, o2, lengths=np.array([len(r) for r in r2], np.uint32))


def test_key_faults_through_the_python_api(ctx, tmp_path, monkeypatch):
    from zlib_ng_amd import bgzf
    small_windows(monkeypatch)
    head, body = I.vcf()
    recs = list(head) + list(body)
    recs[400] = b"chr1\tnot_a_number\tid\tA\tC\t50\tPASS\tDP=1\n"
    recs[600] = b"chr1\t\tid\tA\tC\t50\tPASS\tDP=1\n"
    src = str(tmp_path / "bad.vcf.gz")
    open(src, "wb").write(bgzf.compress(b"".join(recs), block_size=5000))
    with pytest.raises(ValueError, match=r"record 400 at virtual offset \d+: a number field is empty, holds a byte that is no digit"):
        bgzf.sort_key_records(src, "vcf")
    with pytest.raises(ValueError, match=r"record 400 at virtual offset \d+.*incomplete|record 400 at virtual offset"):
        bgzf.sort_records(src, str(tmp_path / "o.gz"), "vcf")
    recs[400], recs[600] = body[0], b"chr" + b"7" * 40 + b"\t5\tid\tA\tC\t50\tPASS\tDP=1\n"
    open(src, "wb").write(bgzf.compress(b"".join(recs), block_size=5000))
    with pytest.raises(ValueError, match=r"record 600 at virtual offset \d+: a field is longer.*has 43 bytes: a width of 48 behind first would do"):
        bgzf.sort_key_records(src, "vcf")
    assert bgzf.sort_key_records(src, "vcf", truncate=True).records == len(recs)
    with bgzf.open(src) as r:
        keys = r.sort_key_records([bgzf.SortKey(0, 0, width=48), bgzf.SortKey(0, 1, kind="number")], 1, meta=b"#")
        cf = R.conf([R.part(0, 0, width=48), R.part(0, 1, kind="number")], record_lines=1, meta=b"#")
        assert np.array_equal(keys.keys, R.encode(recs, cf))
        assert r.sort_keys(keys).tolist() == R.lexorder(keys.keys).tolist()
        # the shards' keys, put together, are the whole file's
        idx = bgzf.LineIndex.build(src)
        cuts = idx.shards(r, 3)
        n = len(recs)
        firsts = [i * n // 3 for i in range(4)]
        parts = [r.sort_key_records("vcf", truncate=True, start=cuts[i], stop=cuts[i + 1], first_record=firsts[i]) for i in range(3)]
        whole = r.sort_key_records("vcf", truncate=True)
        together = parts[0] + parts[1] + parts[2]
        assert np.array_equal(together.keys, whole.keys) and np.array_equal(together.lengths, whole.lengths)

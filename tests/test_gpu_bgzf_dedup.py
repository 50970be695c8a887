"""BGZF duplicate records (bgzf.key_records, dedup_keys, dedup_records, dedup_paired; csrc/za_dedup.hip).  The referee is dedup_ref.py:
the key function in numpy from its statement, the resolve as a dict walk, never the code under test.  Everything is compared for
equality: every key word, every first, every count, every total.  That the referee's keys group the generated records exactly as their
bytes do is asserted on the CPU (test_cpu_bgzf_dedup.py), so a collision cannot hide behind the referee here."""
import functools
import gzip

import numpy as np
import pytest

import dedup_inputs as I
import dedup_ref
from test_gpu_bgzf_grep import block_map
from test_gpu_bgzf_lines import BGZIP, member_table

pytestmark = pytest.mark.gpu

BASE = 700                                                   # record_base of the calls through the C ABI


def packed_of(text, block_size=4099):
    from zlib_ng_amd import bgzf
    blob = bgzf.compress(text, block_size=block_size)
    tab, _ = block_map(blob)
    return blob, member_table(tab)


@functools.lru_cache(maxsize=None)
def grid_text(tail=b""):
    """-> (text, BGZF blob, member table) of the grid's records and what follows them; blocks of 4099 bytes, so bodies straddle them"""
    text = b"".join(I.fastq(I.grid_bodies()))
    return (text,) + packed_of(text + tail)


@functools.lru_cache(maxsize=None)
def ref_keys(name, cf):
    bodies = {n: b for n, b, _ in I.with_bodies()}[name]
    return dedup_ref.keys(bodies, cf)


def conf_of(cf):
    from zlib_ng_amd import _lib
    return _lib.BgzfKeyConf(cf.record_lines, cf.seq_line, -1 if cf.first_byte is None else cf.first_byte[0], cf.first, cf.length,
                            (_lib.BGZF_KEY_IGNORE_CASE if cf.ignore_case else 0) | (_lib.BGZF_KEY_CANONICAL if cf.canonical else 0))


def engine(ctx, blob, members, nbytes, cf, flags, caps=None):
    return ctx.bgzf_key_records(blob, members, 0, nbytes, cf.delimiter[0], flags, conf_of(cf), BASE, caps)


def flat(rows):
    return np.stack([rows["lo"], rows["hi"]], axis=1)


def check_keys(res, want, seen, bytes_in, bases, tail_off, what=None):
    code, status, tot, rows = res
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.seen, tot.bytes_in, tot.bases, tot.tail_off, tot.short_lines, tot.reserved) == (1, 0, seen, bytes_in, bases, tail_off, 0, 0), what
    got = flat(rows)
    if not np.array_equal(got, want):
        at = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError((what, "keys differ at records", at[:10].tolist(), got[at[:3]].tolist(), want[at[:3]].tolist()))


def test_inputs_cross_every_edge():
    bodies = I.grid_bodies()
    assert {len(b) for b in bodies} >= set(I.EDGES) and len(bodies[I.LONG_AT]) == I.LONG and sorted(map(len, bodies))[-2] < 160
    assert set(b"".join(bodies)) >= set(I.LETTERS) and len(bodies) == I.N_GRID       # (and what the case variants add)
    assert len(grid_text()[0]) > 100 * 4099                                        # (many BGZF blocks)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("ignore_case", [False, True])
@pytest.mark.parametrize("first,length", I.PARTS)
def test_key_grid(ctx, first, length, ignore_case, canonical):
    """every key word against the referee; with and without _FINAL; the totals and the tail"""
    from zlib_ng_amd import _lib
    cf = dedup_ref.conf(first=first, length=length, ignore_case=ignore_case, canonical=canonical, first_byte=b"@")
    want = ref_keys("grid", cf._replace(first_byte=None))
    bases = sum(map(len, I.grid_bodies()))
    text, blob, members = grid_text()
    check_keys(engine(ctx, blob, members, len(text), cf, _lib.BGZF_GREP_FINAL), want, I.N_GRID, len(text), bases, len(text), "final")
    # without _FINAL the open record behind the last whole one stays for the next call
    tail = b"@open\nACGTACGT\n+\nFFF"
    text, blob, members = grid_text(tail)
    check_keys(engine(ctx, blob, members, len(text) + len(tail), cf, 0), want, I.N_GRID, len(text), bases, len(text), "open")
    # and with it the tail is one more record
    code, status, tot, rows = engine(ctx, blob, members, len(text) + len(tail), cf, _lib.BGZF_GREP_FINAL)
    assert code == 0 and (tot.seen, tot.bad, tot.tail_off, tot.short_lines) == (I.N_GRID + 1, 0, len(text) + len(tail), 0)
    assert np.array_equal(flat(rows)[:-1], want) and tuple(flat(rows)[-1].tolist()) == dedup_ref.key(b"ACGTACGT", cf)


def test_key_capacity_and_faults(ctx):
    from zlib_ng_amd import _lib
    F = _lib.BGZF_GREP_FINAL
    cf = dedup_ref.conf(first_byte=b"@")
    want = ref_keys("grid", cf._replace(first_byte=None))
    text, blob, members = grid_text()
    bases = sum(map(len, I.grid_bodies()))
    code, status, tot, rows = engine(ctx, blob, members, len(text), cf, F, caps=I.N_GRID - 1)
    assert code == _lib.BUF_ERROR and len(rows) == 0 and (tot.seen, tot.bases, tot.bad) == (I.N_GRID, bases, 0)
    check_keys(engine(ctx, blob, members, len(text), cf, F, caps=I.N_GRID), want, I.N_GRID, len(text), bases, len(text))
    check_keys(engine(ctx, blob, members, len(text), cf, F, caps=I.N_GRID + 9), want, I.N_GRID, len(text), bases, len(text))
    for flags in (1, 2, 8, 16):
        with pytest.raises(_lib.EngineError):
            engine(ctx, blob, members, len(text), cf, flags)
    # the first byte: the smallest record at fault, where it starts
    recs = I.fastq(I.grid_bodies())
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    for wrong in ((2100, 77), (0,), (I.N_GRID - 1,)):
        t = b"".join(b"#" + r[1:] if i in wrong else r for i, r in enumerate(recs))
        b, m = packed_of(t)
        code, status, tot, rows = engine(ctx, b, m, len(t), cf, F)
        assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (1, BASE + min(wrong), starts[min(wrong)], I.N_GRID, 1) and len(rows) == 0
        check_keys(engine(ctx, b, m, len(t), cf._replace(first_byte=None), F), want, I.N_GRID, len(t), bases, len(t))
    # small texts: no record at all; a short last record; another delimiter and line; a CR is a body byte
    text = b"@a\nACGT\n+\nFF"
    b, m = packed_of(text)
    code, status, tot, rows = engine(ctx, b, m, len(text), dedup_ref.conf(), 0)
    assert code == 0 and (tot.seen, tot.covered, tot.tail_off) == (0, 1, 0) and len(rows) == 0
    for text, kw in ((b"@a\nACGT\n+\nFFFF\n@s\nACG", {}), (b"@a\nACGT\n+\nFFFF\n@s\n", {}), (b"@a;ACGT;+;FF\nF;@b;AC;+;#5;", dict(delimiter=b";")),
                     (b"@a\r\nAC\r\n+\r\nFF\r\n", {}), (b"@a\nACGT\n+\nFFFF\n", dict(seq_line=3)), (b">a\nAC\n>b\nGT\n>c\nAC\n", dict(record_lines=2, canonical=True))):
        c2 = dedup_ref.conf(**kw)
        b, m = packed_of(text)
        bodies, nbytes, _ = dedup_ref.bodies_of(text, c2)
        code, status, tot, rows = engine(ctx, b, m, len(text), c2, F)
        assert code == 0 and (tot.seen, tot.bytes_in, tot.bases, tot.bad) == (len(bodies), nbytes, sum(map(len, bodies)), 0), text
        assert np.array_equal(flat(rows), dedup_ref.keys(bodies, c2)), text


def test_reverse_complements(ctx):
    """a file of the reads' reverse complements: the same canonical keys, other plain keys.  No referee."""
    from zlib_ng_amd import _lib
    bodies = [b for b in I.dup_bodies(900, 21) if b != I.rc(b)]
    fwd, rev = b"".join(I.fastq(bodies)), b"".join(I.fastq([I.rc(b) for b in bodies]))
    out = {}
    for name, text in (("fwd", fwd), ("rev", rev)):
        blob, members = packed_of(text)
        for canonical in (False, True):
            out[name, canonical] = flat(engine(ctx, blob, members, len(text), dedup_ref.conf(canonical=canonical), _lib.BGZF_GREP_FINAL)[3])
    assert np.array_equal(out["fwd", True], out["rev", True]) and len(out["fwd", True]) == len(bodies)
    assert (out["fwd", False] != out["rev", False]).any(axis=1).all()
    own = (out["fwd", True] == out["fwd", False]).all(axis=1)                      # the smaller of the two is the read's own or its complement's
    assert np.array_equal(np.where(own[:, None], out["fwd", False], out["rev", False]), out["fwd", True]) and 0 < own.sum() < len(own)


def _rand_keys(rng, n):
    return rng.integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def resolve_cases():
    """-> {name: uint64[n, 2]}"""
    rng = np.random.default_rng(77)
    ones = np.uint64((1 << 64) - 1)
    cases = {"none": np.empty((0, 2), np.uint64), "one": _rand_keys(rng, 1), "distinct": _rand_keys(rng, 5000)}
    cases["identical"] = np.repeat(_rand_keys(rng, 1), 5000, axis=0)               # the hot slot
    values = _rand_keys(rng, 3000)
    p = 1.0 / np.arange(1, 3001)
    cases["skewed"] = values[rng.choice(3000, size=20000, p=p / p.sum())]
    chain = _rand_keys(rng, 300)
    chain[:, 0] = chain[0, 0]                                                      # one long probe chain: the same lo, distinct hi
    cases["same lo"] = np.concatenate([chain, chain[rng.integers(0, 300, 200)]])[rng.permutation(500)]
    last = _rand_keys(rng, 200)
    last[:, 0] = ones                                                              # home in the last slot of any capacity: the chain wraps
    cases["wrap"] = np.concatenate([last, _rand_keys(rng, 1000), last[:50]])[rng.permutation(1250)]
    cases["4096"], cases["4097"] = _rand_keys(rng, 4096), _rand_keys(rng, 4097)
    cases["4097 half"] = cases["4097"][rng.integers(0, 2000, 4097)]
    return cases


@pytest.mark.parametrize("name", ["none", "one", "distinct", "identical", "skewed", "same lo", "wrap", "4096", "4097", "4097 half"])
def test_resolve(ctx, name):
    """first, count and the totals word for word with the dict walk; with the outputs asked for, with each alone, and with the totals only"""
    from zlib_ng_amd import _lib
    k = resolve_cases()[name]
    want = dedup_ref.resolve(k)
    rows = np.ascontiguousarray(k).view(_lib.KEY_ROW_DTYPE).reshape(-1)
    for wf, wc in ((True, True), (False, False), (True, False), (False, True)):
        tot, first, count = ctx.dedup_keys(rows, wf, wc)
        assert (tot.n, tot.unique, tot.duplicates, tot.max_count, tot.max_first, tot.reserved) == \
            (len(k), want.unique, want.duplicates, want.max_count, want.max_first, 0), (name, wf, wc)
        assert (first is None) == (not wf) and (count is None) == (not wc)
        if wf:
            assert first.tolist() == want.first, name
        if wc:
            assert count.tolist() == want.count, name


def test_resolve_cases_are_what_they_say():
    c = resolve_cases()
    assert len(np.unique(c["same lo"][:, 0])) == 1 and len(np.unique(c["same lo"], axis=0)) == 300
    assert (c["wrap"][:, 0] == np.uint64((1 << 64) - 1)).sum() == 250 and dedup_ref.resolve(c["identical"]).max_count == 5000
    r = dedup_ref.resolve(c["skewed"])
    assert r.max_count > 1000 and 1000 < r.unique <= 3000 and dedup_ref.resolve(c["distinct"]).duplicates == 0


def test_device_forms(ctx):
    """both device forms, the work area sized by zngamd_dedup_scratch_bytes; one byte less is BUF_ERROR and nothing is written"""
    from zlib_ng_amd import _lib, devmem
    F = _lib.BGZF_GREP_FINAL
    cf = dedup_ref.conf(ignore_case=True, first_byte=b"@")
    text, blob, members = grid_text()
    n, nb = I.N_GRID, len(text)
    want = ref_keys("grid", cf._replace(first_byte=None))
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    d_rows = devmem.from_host(ctx, b"\xa5" * (16 * (n + 1)))

    def keys_dev(rcap):
        return ctx.bgzf_key_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, nb, 10, F, conf_of(cf), BASE, d_scratch.ptr, nb, d_st.ptr, d_rows.ptr, rcap)

    code, tot = keys_dev(n - 1)
    assert code == _lib.BUF_ERROR and (tot.seen, tot.bad) == (n, 0) and d_rows.cpu().tobytes() == b"\xa5" * (16 * (n + 1))
    # a fault together with a short destination: the fault wins -- the code is OK, the totals name the record, nothing is written
    recs = I.fastq(I.grid_bodies())
    bad = b"".join(recs[:n - 1]) + b"#" + recs[n - 1][1:]
    b_blob, b_members = packed_of(bad)
    d_bin, d_bm, d_bst = devmem.from_host(ctx, b_blob + bytes(64)), devmem.from_host(ctx, b_members.tobytes()), devmem.empty(ctx, 4 * len(b_members))
    code, tot = ctx.bgzf_key_records_dev(d_bin.ptr, len(b_blob), d_bm.ptr, len(b_members), 0, nb, 10, F, conf_of(cf), BASE, d_scratch.ptr, nb, d_bst.ptr,
                                         d_rows.ptr, n - 1)
    assert len(bad) == nb and code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (1, BASE + n - 1, nb - len(recs[n - 1]), n)
    assert d_rows.cpu().tobytes() == b"\xa5" * (16 * (n + 1))
    code, tot = keys_dev(n)
    assert code == 0 and (tot.seen, tot.bytes_in, tot.tail_off, tot.covered) == (n, nb, nb, 1)
    got = d_rows.cpu().tobytes()
    assert got[16 * n:] == b"\xa5" * 16 and np.array_equal(np.frombuffer(got[:16 * n], np.uint64).reshape(-1, 2), want)
    # the keys stay where they are: resolved on the device
    need = int(_lib.load().zngamd_dedup_scratch_bytes(n))
    assert need == 8192 * 12 + 64 and int(_lib.load().zngamd_dedup_scratch_bytes(4097)) == 16384 * 12 + 64
    assert int(_lib.load().zngamd_dedup_scratch_bytes(0)) == 64 * 12 + 64 and int(_lib.load().zngamd_dedup_scratch_bytes((1 << 30) + 1)) == 0
    d_tab = devmem.from_host(ctx, b"\xa5" * (need + 8))
    d_first, d_count = devmem.from_host(ctx, b"\xa5" * (8 * (n + 1))), devmem.from_host(ctx, b"\xa5" * (4 * (n + 1)))
    ref = dedup_ref.resolve(want)
    code, tot = ctx.dedup_keys_dev(d_rows.ptr, n, d_tab.ptr, need - 1, d_first.ptr, d_count.ptr)
    assert code == _lib.BUF_ERROR and d_tab.cpu().tobytes() == b"\xa5" * (need + 8) and d_first.cpu().tobytes() == b"\xa5" * (8 * (n + 1))
    code, tot = ctx.dedup_keys_dev(d_rows.ptr, n, d_tab.ptr, need, 0, 0)           # the totals alone
    assert code == 0 and (tot.n, tot.unique, tot.duplicates, tot.max_count, tot.max_first) == (n, ref.unique, ref.duplicates, ref.max_count, ref.max_first)
    assert d_first.cpu().tobytes() == b"\xa5" * (8 * (n + 1)) and d_tab.cpu().tobytes()[need:] == b"\xa5" * 8
    code, tot = ctx.dedup_keys_dev(d_rows.ptr, n, d_tab.ptr, need, d_first.ptr, d_count.ptr)
    assert code == 0 and (tot.n, tot.unique, tot.max_count, tot.max_first) == (n, ref.unique, ref.max_count, ref.max_first)
    f, c = d_first.cpu().tobytes(), d_count.cpu().tobytes()
    assert f[8 * n:] == b"\xa5" * 8 and c[4 * n:] == b"\xa5" * 4 and d_tab.cpu().tobytes()[need:] == b"\xa5" * 8
    assert np.frombuffer(f[:8 * n], np.uint64).tolist() == ref.first and np.frombuffer(c[:4 * n], np.uint32).tolist() == ref.count
    assert d_rows.cpu().tobytes() == got                                           # (the keys are read, never written)
    code, tot = ctx.dedup_keys_dev(0, 0, 0, 0, 0, 0)                               # no key: nothing is launched
    assert code == 0 and (tot.n, tot.unique, tot.duplicates, tot.max_count, tot.max_first) == (0, 0, 0, 0, 0)


def same(res, want):
    assert res.first.dtype == np.int64 and res.first.tolist() == want.first and res.count.tolist() == want.count
    assert res.duplicate.dtype == np.bool_ and res.duplicate.tolist() == [f != i for i, f in enumerate(want.first)]
    assert (res.records, res.unique, res.duplicates, res.max_count, res.max_first) == (len(want.first), want.unique, want.duplicates, want.max_count, want.max_first)


def test_file_with_small_read_windows(ctx, tmp_path, monkeypatch):
    """records straddle windows; a path and a reader; the shards' keys, put together, are the whole file's; the faults of the file"""
    from zlib_ng_amd import bgzf
    n = 1500
    bodies = I.dup_bodies(n, 11)
    text = b"".join(I.fastq(bodies))
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)
    for kw in (dict(), dict(ignore_case=True, canonical=True)):
        cf = dedup_ref.conf(**kw)
        want = ref_keys("windows", cf)
        ctx.bgzf_stats()
        res = bgzf.key_records(src, first_byte=b"@", **kw)
        assert ctx.bgzf_stats()[0] >= 3                                                # (several windows)
        assert np.array_equal(flat(res.keys), want) and (res.records, res.bases, len(res)) == (n, sum(map(len, bodies)), n)
        assert res.options == dict(first=0, length=0, ignore_case=cf.ignore_case, canonical=cf.canonical)
        same(bgzf.dedup_keys(res), dedup_ref.exact(bodies, cf))
        with bgzf.open(src) as r:
            at = r.tell()
            whole = r.key_records(first_byte=b"@", **kw)
            assert r.tell() == at and np.array_equal(whole.keys, res.keys)
            idx = bgzf.LineIndex.build(src)
            cuts = idx.shards(r, 3, lines_per_record=4)
            firsts = [i * n // 3 for i in range(4)]
            parts = [r.key_records(start=cuts[i], stop=cuts[i + 1], first_record=firsts[i], first_byte=b"@", **kw) for i in range(3)]
            assert [p.records for p in parts] == [b - a for a, b in zip(firsts, firsts[1:])]
            together = parts[0] + parts[1] + parts[2]
            assert np.array_equal(together.keys, res.keys) and together.bases == res.bases and together.options == res.options
            same(bgzf.dedup_keys(together), dedup_ref.exact(bodies, cf))
            with pytest.raises(ValueError, match="not comparable"):
                parts[0] + r.key_records(start=cuts[1], stop=cuts[2], length=30)
    lines = text.split(b"\n")
    lines[4 * 300] = b"x" + lines[4 * 300][1:]
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bgzf.compress(b"\n".join(lines), block_size=5000))
    with pytest.raises(ValueError, match=r"record 300 at virtual offset \d+ does not start with b'@' \(first_byte\)"):
        bgzf.key_records(bad, first_byte=b"@")
    assert bgzf.key_records(bad).records == n
    short = str(tmp_path / "short.fq.gz")
    open(short, "wb").write(bgzf.compress(text + b"@s\nACGT\n", block_size=5000))
    with pytest.raises(ValueError, match=r"record 1500, the last one, has 2 of 4 lines \(allow_short\)"):
        bgzf.key_records(short)
    res = bgzf.key_records(short, allow_short=True)
    assert res.records == n + 1 and tuple(flat(res.keys)[-1].tolist()) == dedup_ref.key(b"ACGT", dedup_ref.conf())


def test_dedup_records(ctx, tmp_path):
    """by path and by reader: output holds exactly the kept records in file order, duplicates the rest; output=None writes nothing"""
    from zlib_ng_amd import bgzf
    n = 900
    bodies = I.dup_bodies(n, 21)
    recs = I.fastq(bodies)
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(b"".join(recs), block_size=4099))
    for kw in (dict(), dict(ignore_case=True, canonical=True)):
        want = dedup_ref.exact(bodies, dedup_ref.conf(**kw))
        assert want.first == dedup_ref.resolve(ref_keys("dedup", dedup_ref.conf(**kw))).first and 100 < want.unique < n - 100
        kept = b"".join(r for i, r in enumerate(recs) if want.first[i] == i)
        rest = b"".join(r for i, r in enumerate(recs) if want.first[i] != i)
        out, dup = str(tmp_path / "kept.fq.gz"), str(tmp_path / "dup.fq.gz")
        res = bgzf.dedup_records(src, out, duplicates=dup, first_byte=b"@", compresslevel=1, **kw)
        same(res, want)
        assert gzip.decompress(open(out, "rb").read()) == kept and gzip.decompress(open(dup, "rb").read()) == rest
        out2 = str(tmp_path / "kept2.fq.gz")
        with bgzf.open(src) as r:
            at = r.tell()
            same(r.dedup_records(out2, first_byte=b"@", compresslevel=1, **kw), want)
            assert r.tell() == at
            same(r.dedup_records(None, **kw), want)
        assert gzip.decompress(open(out2, "rb").read()) == kept
        before = sorted(p.name for p in tmp_path.iterdir())
        counted = bgzf.dedup_records(src, None, **kw)
        same(counted, want)
        assert sorted(p.name for p in tmp_path.iterdir()) == before
        assert counted.duplication_rate == want.duplicates / n
        # the mask of the result as drop= of trim_records leaves the same reads
        out3 = str(tmp_path / "kept3.fq.gz")
        t = bgzf.trim_records(src, out3, drop=counted.drop(), first_byte=b"@", compresslevel=1)
        assert (t.kept, t.dropped) == (want.unique, want.duplicates) and gzip.decompress(open(out3, "rb").read()) == kept
        # the levels and the most common sequences, from the referee's counts
        sizes = sorted((c for c in want.count if c), reverse=True)
        idx, cnt = counted.most_common(5)
        assert cnt.tolist() == sizes[:5] and [want.count[i] for i in idx.tolist()] == sizes[:5] and idx[0] == want.max_first
        distinct, reads = counted.levels()
        assert int(distinct.sum()) == want.unique and int(reads.sum()) == n and distinct[0] == sizes.count(1)


def test_dedup_paired(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    r1, r2 = I.paired_bodies()
    n = len(r1)
    rec1, rec2 = I.fastq(r1, b"a"), I.fastq(r2, b"b")
    p1, p2 = str(tmp_path / "r1.fq.gz"), str(tmp_path / "r2.fq.gz")
    open(p1, "wb").write(bgzf.compress(b"".join(rec1), block_size=4099))
    open(p2, "wb").write(bgzf.compress(b"".join(rec2), block_size=4099))
    want = dedup_ref.walk(list(zip(r1, r2)))                                     # the pairs' bytes themselves
    only1, only2 = dedup_ref.walk(r1), dedup_ref.walk(r2)
    both = sum(1 for i in range(n) if only1.first[i] != i and only2.first[i] != i)
    assert 0 < want.duplicates <= both and want.duplicates < only1.duplicates and want.duplicates < only2.duplicates      # equal in R1 only, in R2 only, in both
    o1, o2, d1, d2 = (str(tmp_path / x) for x in ("o1.gz", "o2.gz", "d1.gz", "d2.gz"))
    res = bgzf.dedup_paired([p1, p2], [o1, o2], duplicates=[d1, d2], first_byte=b"@", compresslevel=1)
    same(res, want)
    keep = [i for i in range(n) if want.first[i] == i]
    a, b = gzip.decompress(open(o1, "rb").read()), gzip.decompress(open(o2, "rb").read())
    assert a == b"".join(rec1[i] for i in keep) and b == b"".join(rec2[i] for i in keep)      # mates at the same index
    assert a.count(b"\n") == b.count(b"\n") == 4 * len(keep)
    assert gzip.decompress(open(d1, "rb").read()) == b"".join(rec1[i] for i in range(n) if want.first[i] != i)
    assert gzip.decompress(open(d2, "rb").read()) == b"".join(rec2[i] for i in range(n) if want.first[i] != i)
    same(bgzf.dedup_paired([p1, p2], None), want)
    ka, kb = bgzf.key_records(p1), bgzf.key_records(p2)
    pk = bgzf.pair_keys(ka, kb)
    assert np.array_equal(flat(pk.keys), dedup_ref.pair(flat(ka.keys), flat(kb.keys)))
    # a mate file that lost a read
    p3 = str(tmp_path / "r3.fq.gz")
    open(p3, "wb").write(bgzf.compress(b"".join(rec2[:-1]), block_size=4099))
    with pytest.raises(ValueError, match="out of step"):
        bgzf.dedup_paired([p1, p3], None)


def test_two_line_fasta(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    bodies = I.fasta_bodies()
    recs = [b">s%d\n%s\n" % (i, s) for i, s in enumerate(bodies)]
    src = str(tmp_path / "seqs.fa.gz")
    open(src, "wb").write(bgzf.compress(b"".join(recs), block_size=4099))
    for canonical in (False, True):
        cf = dedup_ref.conf(record_lines=2, canonical=canonical)
        res = bgzf.key_records(src, 2, canonical=canonical, first_byte=b">")
        assert np.array_equal(flat(res.keys), ref_keys("fasta", cf))
        want = dedup_ref.exact(bodies, cf)
        out = str(tmp_path / "kept.fa.gz")
        same(bgzf.dedup_records(src, out, 2, canonical=canonical, first_byte=b">", compresslevel=1), want)
        assert gzip.decompress(open(out, "rb").read()) == b"".join(r for i, r in enumerate(recs) if want.first[i] == i)


def test_golden_file(ctx):
    from zlib_ng_amd import bgzf
    bodies = I.golden_bodies()
    res = bgzf.key_records(BGZIP, first_byte=b"@")
    n = res.records
    assert n == 10000 and res.bases == sum(map(len, bodies[:n]))
    assert np.array_equal(flat(res.keys), ref_keys("golden", dedup_ref.conf()))
    same(bgzf.dedup_keys(res), dedup_ref.exact(bodies[:n], dedup_ref.conf()))
    cf = dedup_ref.conf(length=8)
    short = bgzf.key_records(BGZIP, length=8)
    assert np.array_equal(flat(short.keys), ref_keys("golden", cf))
    want = dedup_ref.exact(bodies[:n], cf)
    assert want.duplicates > 0
    same(bgzf.dedup_keys(short), want)

"""BGZF contaminant screen (bgzf.KmerSet, screen_records, screen_filter; csrc/za_screen.hip).  The referee is screen_ref.py: plain
Python from the statement of the rule, a dict from code to mask and a loop over positions, never the code under test.  Everything is
compared for equality: every exported pair, every field of every row, every total."""
import functools
import gzip

import numpy as np
import pytest

import screen_inputs as I
import screen_ref as R
from test_gpu_bgzf_dedup import packed_of

pytestmark = pytest.mark.gpu

BASE = 700                                                   # record_base of the calls through the C ABI


def flags_of(canonical):
    from zlib_ng_amd import _lib
    return _lib.KMER_CANONICAL if canonical else 0


def sorted_pairs(table):
    codes, masks = table.export()
    assert codes.dtype == masks.dtype == np.uint64 and len(codes) == len(masks)
    order = np.argsort(codes)
    return list(zip(codes[order].tolist(), masks[order].tolist()))


def check_set(ctx, refs, k, canonical):
    """build -> the referee's pairs and counts; load(export(build)) -> the same pairs"""
    want, positions, valid = R.build(refs, k, canonical)
    table = ctx.kmer_set_build(refs, k, flags_of(canonical))
    i = table.info
    assert (i.k, i.flags, i.n_refs, i.reserved, i.positions, i.valid, i.distinct, i.cap) == \
        (k, flags_of(canonical), len(refs), 0, positions, valid, len(want), R.cap_of(positions))
    got = sorted_pairs(table)
    assert got == R.pairs(want)
    again = ctx.kmer_set_load(k, flags_of(canonical), len(refs), np.array([c for c, _ in got], np.uint64), np.array([m for _, m in got], np.uint64))
    j = again.info
    assert (j.k, j.flags, j.n_refs, j.positions, j.valid, j.distinct, j.cap) == (k, flags_of(canonical), len(refs), len(got), len(got), len(got), R.cap_of(len(got)))
    assert sorted_pairs(again) == got
    table.free()
    again.free()
    return want


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("n_refs", I.BUILD_R)
@pytest.mark.parametrize("k", I.BUILD_K)
def test_set_build(ctx, k, n_refs, canonical):
    """references of every length at which a strip or the k-mer ends, invalid bytes at the strip edges, a reverse complement"""
    want = check_set(ctx, list(I.build_references(k, n_refs)), k, canonical)
    if n_refs == 64 and k > 2:
        masks = set(want.values())
        assert any(m >> 63 for m in masks) and (not canonical or any(m & 1 and m >> 63 for m in masks))      # the last reference; it and the first


def test_set_small_tables_and_empty_sets(ctx):
    from zlib_ng_amd import _lib
    # 32 distinct codes in 64 slots: half full, probes wrap
    want = check_set(ctx, [I.wrap_reference()], 4, False)
    assert len(want) == 32
    # codes whose home is the last slot of a table of 64: the chain wraps whatever else the table holds
    last = [c for c in range(4 ** 6) if mix(c) & 63 == 63][:20]
    t = ctx.kmer_set_load(6, 0, 3, np.array(last + last[:5], np.uint64), np.array([1] * 20 + [4] * 5, np.uint64))
    assert (t.info.positions, t.info.distinct, t.info.cap) == (25, 20, 64)
    assert sorted_pairs(t) == sorted((c, 5 if i < 5 else 1) for i, c in enumerate(last))      # a code that appears twice ORs its masks
    t.free()
    # empty sets: no reference reaches k; no k-mer is valid; no byte at all; no pair
    for refs, k in (([b"ACGT", b"AC", b""], 5), ([b"ACGTNACGTNACGT"], 5), ([b""], 1), ([b""] * 64, 31)):
        assert check_set(ctx, refs, k, True) == {}
    e = ctx.kmer_set_load(31, 1, 64, np.empty(0, np.uint64), np.empty(0, np.uint64))
    assert (e.info.distinct, e.info.cap) == (0, 64) and sorted_pairs(e) == []
    # one k-mer, k = 1 and k = 31; U and lower case
    assert check_set(ctx, [b"a"], 1, False) == {0: 1} and check_set(ctx, [b"u" * 31, b"T" * 31], 31, False) == {4 ** 31 - 1: 3}
    # too small a room for the export: the count comes back
    import ctypes as C
    t = ctx.kmer_set_build([b"ACGT"], 2, 0)
    codes, n = np.full(3, 7, np.uint64), C.c_uint64(0)
    p = C.c_void_p(codes.ctypes.data)
    assert ctx.L.zngamd_kmer_set_export(t.h, p, p, 2, C.byref(n)) == _lib.BUF_ERROR and n.value == 3 and codes.tolist() == [7, 7, 7]
    other = _lib.Context(device=0)
    try:                                                     # a set is bound to the context it was made in
        text, blob, members = screen_text_of(21)
        with pytest.raises(_lib.EngineError):
            other.bgzf_screen_records(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, _lib.BgzfScreenConf(4, 1, -1, 1, 0), t, BASE)
    finally:
        other.close()
    t.free()
    with pytest.raises(ValueError, match="freed"):
        t.info


def mix(x):
    """the splitmix64 step (include/zng_amd.h), on a Python integer"""
    M = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & M
    x = ((x ^ x >> 30) * 0xBF58476D1CE4E5B9) & M
    x = ((x ^ x >> 27) * 0x94D049BB133111EB) & M
    return x ^ x >> 31


# ---- the screen
@functools.lru_cache(maxsize=None)
def screen_text_of(k, tail=b""):
    """-> (text, BGZF blob, member table) of the reads and what follows them; blocks of 4099 bytes, so bodies straddle them"""
    text = I.screen_text(k)
    return (text,) + packed_of(text + tail)


@functools.lru_cache(maxsize=None)
def ref_table(k, canonical):
    return R.build(I.screen_references(), k, canonical)[0]


@functools.lru_cache(maxsize=None)
def ref_rows(k, canonical):
    """the referee's rows of the reads, computed once"""
    table = ref_table(k, canonical)
    return tuple(R.screen(b, table, k, canonical) for b in I.screen_bodies(k))


def totals_of(rows, bodies, nbytes, min_hits):
    return R.Totals(len(rows), nbytes, sum(map(len, bodies)), sum(r.kmers for r in rows), sum(r.hits for r in rows), sum(1 for r in rows if r.hits >= min_hits))


def conf_of(min_hits=1, first_byte=b"@", record_lines=4, seq_line=1):
    from zlib_ng_amd import _lib
    return _lib.BgzfScreenConf(record_lines, seq_line, -1 if first_byte is None else first_byte[0], min_hits, 0)


def row_list(rows):
    return [R.Row(*t) for t in zip(rows["refs"].tolist(), rows["kmers"].tolist(), rows["hits"].tolist(), rows["best"].tolist(), rows["best_hits"].tolist())]


def check_rows(res, want, tot_want, tail_off, what=None):
    code, status, tot, rows = res
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.short_lines, tot.reserved, tot.tail_off) == (1, 0, 0, 0, tail_off), what
    assert R.Totals(tot.seen, tot.bytes_in, tot.bases, tot.kmers, tot.hits, tot.matched) == tot_want, what
    got = row_list(rows)
    if got != list(want):
        at = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        raise AssertionError((what, "rows differ at records", at[:10], [got[i] for i in at[:3]], [want[i] for i in at[:3]], len(got), len(want)))


def test_screen_inputs_hit_what_they_should():
    for k, canonical in I.SCREEN_RULES:
        rows = ref_rows(k, canonical)
        assert any(r.refs == (1 << 64) - 1 for r in rows) and rows[-3].refs == 0b111000       # all 64 references; three of them
        assert any(r.hits == 0 and r.kmers > 0 for r in rows) and any(0 < r.hits < 5 for r in rows) and any(r.kmers == 0 for r in rows)
        assert any(r.hits > 2000 for r in rows) and any(0 < r.best_hits < r.hits for r in rows) and len({r.best for r in rows}) > 40
        assert rows[-2].refs == 1 << 10 | 1 << 20 and (rows[-2].best, rows[-2].best_hits, rows[-2].hits) == (10, 60 - k + 1, 110 - 2 * k + 2)
        assert rows[-1].refs == 1 << 30 | 1 << 12 and (rows[-1].best, rows[-1].best_hits, rows[-1].hits) == (12, 50 - k + 1, 100 - 2 * k + 2)      # the tie
        assert any(0 < r.kmers < len(b) - k + 1 for r, b in zip(rows, I.screen_bodies(k)))                   # an invalid byte inside
    assert len(screen_text_of(21)[0]) > 80 * 4099                                                              # (many BGZF blocks)


@pytest.mark.parametrize("min_hits", [1, 5])
@pytest.mark.parametrize("k,canonical", I.SCREEN_RULES)
def test_screen_grid(ctx, k, canonical, min_hits):
    """every row field and every total against the referee; with and without _FINAL; the open tail"""
    from zlib_ng_amd import _lib
    kset = ctx.kmer_set_build(list(I.screen_references()), k, flags_of(canonical))
    want, bodies = ref_rows(k, canonical), I.screen_bodies(k)
    cf = conf_of(min_hits)
    text, blob, members = screen_text_of(k)
    tot_want = totals_of(want, bodies, len(text), min_hits)
    assert 0 < tot_want.matched < tot_want.seen and (min_hits == 1 or tot_want.matched < totals_of(want, bodies, len(text), 1).matched)
    check_rows(ctx.bgzf_screen_records(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, cf, kset, BASE), want, tot_want, len(text), "final")
    # without _FINAL the open record behind the last whole one stays for the next call
    tail_body = I.screen_references()[9][30:95]
    tail = b"@open\n" + tail_body + b"\n+\nFFF"
    text, blob, members = screen_text_of(k, tail)
    check_rows(ctx.bgzf_screen_records(blob, members, 0, len(text) + len(tail), 10, 0, cf, kset, BASE), want, tot_want, len(text), "open")
    # and with it the tail is one more record
    last = R.screen(tail_body, ref_table(k, canonical), k, canonical)
    assert last.hits == 65 - k + 1 and last.best == 9
    more = want + (last,)
    check_rows(ctx.bgzf_screen_records(blob, members, 0, len(text) + len(tail), 10, _lib.BGZF_GREP_FINAL, cf, kset, BASE), more,
               totals_of(more, bodies + (tail_body,), len(text) + len(tail), min_hits), len(text) + len(tail), "final with the tail")
    kset.free()


def test_screen_capacity_and_faults(ctx):
    from zlib_ng_amd import _lib, devmem
    F = _lib.BGZF_GREP_FINAL
    k, canonical = I.SCREEN_RULES[0]
    kset = ctx.kmer_set_build(list(I.screen_references()), k, flags_of(canonical))
    want, bodies = ref_rows(k, canonical), I.screen_bodies(k)
    n = len(want)
    text, blob, members = screen_text_of(k)
    tot_want = totals_of(want, bodies, len(text), 1)
    code, status, tot, rows = ctx.bgzf_screen_records(blob, members, 0, len(text), 10, F, conf_of(), kset, BASE, n - 1)
    assert code == _lib.BUF_ERROR and len(rows) == 0                                # rows_cap < seen: the totals are valid
    assert R.Totals(tot.seen, tot.bytes_in, tot.bases, tot.kmers, tot.hits, tot.matched) == tot_want and (tot.bad, tot.covered) == (0, 1)
    check_rows(ctx.bgzf_screen_records(blob, members, 0, len(text), 10, F, conf_of(), kset, BASE, n), want, tot_want, len(text))
    check_rows(ctx.bgzf_screen_records(blob, members, 0, len(text), 10, F, conf_of(), kset, BASE, n + 9), want, tot_want, len(text))
    for flags in (1, 2, 8, 16):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_screen_records(blob, members, 0, len(text), 10, flags, conf_of(), kset, BASE)
    with pytest.raises(_lib.EngineError):
        ctx.bgzf_screen_records(blob, members, 0, len(text), 10, F, conf_of(min_hits=0), kset, BASE)
    # the first byte: the smallest record at fault, where it starts
    recs = I.fastq(bodies)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    for wrong in ((1500, 77), (0,), (n - 1,)):
        t = b"".join(b"#" + r[1:] if i in wrong else r for i, r in enumerate(recs))
        b, m = packed_of(t)
        code, status, tot, rows = ctx.bgzf_screen_records(b, m, 0, len(t), 10, F, conf_of(), kset, BASE)
        assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (1, BASE + min(wrong), starts[min(wrong)], n, 1) and len(rows) == 0
        check_rows(ctx.bgzf_screen_records(b, m, 0, len(t), 10, F, conf_of(first_byte=None), kset, BASE), want, tot_want, len(t))
    # the device form: the rows stay on the device; one row less is BUF_ERROR and nothing is written
    nb = len(text)
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    d_rows = devmem.from_host(ctx, b"\xa5" * (24 * (n + 1)))
    dev = lambda rcap: ctx.bgzf_screen_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, nb, 10, F, conf_of(5), kset, BASE, d_scratch.ptr, nb, d_st.ptr,
                                                   d_rows.ptr, rcap)
    code, tot = dev(n - 1)
    assert code == _lib.BUF_ERROR and (tot.seen, tot.bad) == (n, 0) and d_rows.cpu().tobytes() == b"\xa5" * (24 * (n + 1))
    # a fault together with a short destination: the fault wins -- the code is OK, the totals name the record, nothing is written
    t = b"".join(b"#" + r[1:] if i == n - 1 else r for i, r in enumerate(recs))
    b, m = packed_of(t)
    d_bin, d_bm, d_bst = devmem.from_host(ctx, b + bytes(64)), devmem.from_host(ctx, m.tobytes()), devmem.empty(ctx, 4 * len(m))
    code, tot = ctx.bgzf_screen_records_dev(d_bin.ptr, len(b), d_bm.ptr, len(m), 0, nb, 10, F, conf_of(5), kset, BASE, d_scratch.ptr, nb, d_bst.ptr, d_rows.ptr,
                                            n - 1)
    assert len(t) == nb and code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (1, BASE + n - 1, starts[n - 1], n)
    assert d_rows.cpu().tobytes() == b"\xa5" * (24 * (n + 1))
    code, tot = dev(n)
    assert code == 0 and R.Totals(tot.seen, tot.bytes_in, tot.bases, tot.kmers, tot.hits, tot.matched) == totals_of(want, bodies, nb, 5)
    got = d_rows.cpu().tobytes()
    assert got[24 * n:] == b"\xa5" * 24 and row_list(np.frombuffer(got[:24 * n], _lib.SCREEN_ROW_DTYPE)) == list(want)
    # small texts: no record at all; a short last record; another delimiter and line; two-line records
    table = ref_table(k, canonical)
    read = I.screen_references()[7][5:80]
    for text, kw in ((b"@a\n" + read + b"\n+\nFF", dict(final=False)), (b"@a\n" + read + b"\n+\nFFFF\n@s\n" + read[:40], {}), (b"@a\n" + read + b"\n+\nFFFF\n@s\n", {}),
                     (b"@a;" + read + b";+;FF\nF;@b;" + read[3:] + b";+;#5;", dict(delimiter=b";")), (b"@a\nFFFF\n+\n" + read + b"\n", dict(seq_line=3)),
                     (b">a\n" + read + b"\n>b\nGT\n>c\n" + I.rc(read) + b"\n", dict(record_lines=2))):
        final = kw.pop("final", True)
        b, m = packed_of(text)
        rows_want, tw = R.screen_text(text, table, k, canonical, final=final, **kw)
        code, status, tot, rows = ctx.bgzf_screen_records(b, m, 0, len(text), kw.get("delimiter", b"\n")[0], F if final else 0,
                                                          conf_of(1, None, kw.get("record_lines", 4), kw.get("seq_line", 1)), kset, BASE)
        assert code == 0 and tot.bad == 0 and R.Totals(tot.seen, tot.bytes_in, tot.bases, tot.kmers, tot.hits, tot.matched) == tw, text
        assert row_list(rows) == rows_want and (not final or tw.hits > 0), text
    kset.free()


def same(res, want, bodies, min_hits):
    assert [res.kmers.dtype, res.hits.dtype, res.best.dtype, res.best_hits.dtype, res.refs.dtype, res.matched.dtype] == [np.int64] * 4 + [np.uint64, np.bool_]
    got = [R.Row(*t) for t in zip(res.refs.tolist(), res.kmers.tolist(), res.hits.tolist(), [R.NONE if b < 0 else b for b in res.best.tolist()],
                                  res.best_hits.tolist())]
    assert got == list(want)
    assert (res.records, len(res), res.bases, res.min_hits) == (len(want), len(want), sum(map(len, bodies)), min_hits)
    assert res.matched.tolist() == [r.hits >= min_hits for r in want] and res.matched_records == sum(1 for r in want if r.hits >= min_hits)
    by = [0] * 64
    for r in want:
        if r.hits:
            by[r.best] += 1
    assert res.by_reference().tolist() == by


def test_python_face(ctx, tmp_path, monkeypatch):
    """a path and a reader, small read windows; the shards' results, put together, are the whole file's; screen_filter writes exactly the
    referee's two lists in file order; the faults of the file"""
    from zlib_ng_amd import bgzf
    k, canonical = I.SCREEN_RULES[0]
    bodies, want = I.screen_bodies(k), ref_rows(k, canonical)
    n = len(bodies)
    recs = I.fastq(bodies)
    text = b"".join(recs)
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)
    names = ["c%d" % j for j in range(64)]
    kset = bgzf.KmerSet.build(I.screen_references(), k, canonical, names)
    assert list(zip(kset.codes.tolist(), kset.masks.tolist())) == R.pairs(ref_table(k, canonical)) and kset.names == tuple(names) and len(kset) == len(ref_table(k, canonical))
    ctx.bgzf_stats()
    res = bgzf.screen_records(src, kset, first_byte=b"@")
    assert ctx.bgzf_stats()[0] >= 3                                                # (several windows)
    same(res, want, bodies, 1)
    # a set from its pairs alone: the table is made on first use
    again = bgzf.KmerSet.from_codes(k, kset.codes, kset.masks, 64, canonical, names)
    assert again == kset
    same(bgzf.screen_records(src, again, min_hits=5), want, bodies, 5)
    with bgzf.open(src) as r:
        at = r.tell()
        whole = r.screen_records(again, first_byte=b"@", min_hits=5)
        assert r.tell() == at
        same(whole, want, bodies, 5)
        idx = bgzf.LineIndex.build(src)
        cuts = idx.shards(r, 3, lines_per_record=4)
        firsts = [i * n // 3 for i in range(4)]
        parts = [r.screen_records(kset, start=cuts[i], stop=cuts[i + 1], first_record=firsts[i], first_byte=b"@", min_hits=5) for i in range(3)]
        assert [p.records for p in parts] == [b - a for a, b in zip(firsts, firsts[1:])]
        same(parts[0] + parts[1] + parts[2], want, bodies, 5)
        with pytest.raises(ValueError, match="not comparable"):
            parts[0] + r.screen_records(kset, start=cuts[1], stop=cuts[2])
        other = bgzf.KmerSet.build(I.screen_references()[:3], k, canonical, names[:3])
        with pytest.raises(ValueError, match="not comparable"):
            parts[0] + r.screen_records(other, start=cuts[1], stop=cuts[2], min_hits=5)
    # the screen and the split: bbduk's out= and outm=
    for min_hits in (1, 5):
        hit = [r.hits >= min_hits for r in want]
        clean, dirty = b"".join(r for r, h in zip(recs, hit) if not h), b"".join(r for r, h in zip(recs, hit) if h)
        assert clean and dirty
        out, outm = str(tmp_path / "clean.fq.gz"), str(tmp_path / "dirty.fq.gz")
        same(bgzf.screen_filter(src, kset, out, outm, first_byte=b"@", min_hits=min_hits, compresslevel=1), want, bodies, min_hits)
        assert gzip.decompress(open(out, "rb").read()) == clean and gzip.decompress(open(outm, "rb").read()) == dirty
        out2 = str(tmp_path / "clean2.fq.gz")
        with bgzf.open(src) as r:
            at = r.tell()
            same(r.screen_filter(kset, out2, min_hits=min_hits, compresslevel=1), want, bodies, min_hits)
            assert r.tell() == at
        assert gzip.decompress(open(out2, "rb").read()) == clean
        out3 = str(tmp_path / "dirty3.fq.gz")
        res = bgzf.screen_filter(src, kset, None, out3, min_hits=min_hits, compresslevel=1)
        assert gzip.decompress(open(out3, "rb").read()) == dirty
        before = sorted(p.name for p in tmp_path.iterdir())
        same(bgzf.screen_filter(src, kset, None, min_hits=min_hits), want, bodies, min_hits)
        assert sorted(p.name for p in tmp_path.iterdir()) == before
        # the mask of the result as drop= of trim_records leaves the same reads
        out4 = str(tmp_path / "clean4.fq.gz")
        t = bgzf.trim_records(src, out4, drop=res.drop(), first_byte=b"@", compresslevel=1)
        assert (t.kept, t.dropped) == (n - sum(hit), sum(hit)) and gzip.decompress(open(out4, "rb").read()) == clean
    # the faults of the file
    lines = text.split(b"\n")
    lines[4 * 300] = b"x" + lines[4 * 300][1:]
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bgzf.compress(b"\n".join(lines), block_size=5000))
    with pytest.raises(ValueError, match=r"record 300 at virtual offset \d+ does not start with b'@' \(first_byte\)"):
        bgzf.screen_records(bad, kset, first_byte=b"@")
    assert bgzf.screen_records(bad, kset).records == n
    short = str(tmp_path / "short.fq.gz")
    open(short, "wb").write(bgzf.compress(text + b"@s\n" + I.screen_references()[2][:50] + b"\n", block_size=5000))
    with pytest.raises(ValueError, match=r"record %d, the last one, has 2 of 4 lines \(allow_short\)" % n):
        bgzf.screen_records(short, kset)
    res = bgzf.screen_records(short, kset, allow_short=True)
    assert res.records == n + 1 and (res.hits[-1], res.best[-1]) == (50 - k + 1, 2)


def test_kmer_set_from_fasta(ctx, tmp_path):
    """a bgzipped FASTA of wrapped lines: the set of its records is the set built from the same sequences, named as the records are"""
    from zlib_ng_amd import bgzf
    refs = I.screen_references()[:5] + (I.screen_references()[0][:17].lower(), b"ACGTNNNNACGTTTGACCA" * 9)
    names = ["chr%d" % j for j in range(len(refs))]
    fasta = b"".join(b">%s some words\n" % nm.encode() + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for nm, s in zip(names, refs))
    path = str(tmp_path / "ref.fa.gz")
    open(path, "wb").write(bgzf.compress(fasta, block_size=4099))
    for k, canonical in ((31, True), (11, False)):
        a = bgzf.KmerSet.from_fasta(path, k, canonical)
        b = bgzf.KmerSet.build(refs, k, canonical, names)
        assert a == b and a.names == tuple(names) and (a.k, a.canonical) == (k, canonical)
        assert list(zip(a.codes.tolist(), a.masks.tolist())) == R.pairs(R.build(refs, k, canonical)[0])
    big = b"".join(b">s%d\nACGT\n" % j for j in range(65))
    open(path, "wb").write(bgzf.compress(big))
    with pytest.raises(ValueError, match="1 to 64 references"):
        bgzf.KmerSet.from_fasta(path)

"""BGZF quality control (bgzf.qc_records; csrc/za_qc.hip).  The referee is qc_ref.py: plain Python with the serial loops of the rule as
include/zng_amd.h states it, never the code under test.  Everything is compared for equality: every table word, every total, every row.
A workgroup of za_k_qc_eval owns a span of at least 256 records, so the 3000 records of the grid are twelve workgroups and spans."""
import functools
import gzip
import random

import numpy as np
import pytest

import qc_ref
from test_gpu_bgzf_grep import block_map
from test_gpu_bgzf_lines import BGZIP, member_table

pytestmark = pytest.mark.gpu

BASE = 700                                                   # record_base of the calls through the C ABI
EDGES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 150]
LETTERS = b"ACGTNacgtnR."
QUALS = bytes(b for b in range(256) if b != 10)             # every byte that is no delimiter
N = 3000
TOTALS = ("bytes_in", "bases", "min_len", "max_len", "empty", "quality_sum", "q20_bases", "q30_bases", "low_bases", "quality_clamped")


def gen_reads(n, seed, quals=QUALS):
    """-> [(name, seq, qual)]: lengths from EDGES or random below 160, bases from LETTERS, qualities from quals"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.choice(EDGES) if i % 7 == 0 else rng.randrange(0, 160)
        out.append((b"@r%d" % i, bytes(rng.choice(LETTERS) for _ in range(L)), bytes(rng.choice(quals) for _ in range(L))))
    return out


def fastq(reads):
    return [b"%s\n%s\n+\n%s\n" % r for r in reads]


def packed_of(text, block_size=4099):
    from zlib_ng_amd import bgzf
    blob = bgzf.compress(text, block_size=block_size)
    tab, _ = block_map(blob)
    return blob, member_table(tab)


@functools.lru_cache(maxsize=None)
def text_of(n, tail=b""):
    """-> (records, text, BGZF blob, member table) of n generated reads and what follows them: computed once, never changed"""
    recs = fastq(gen_reads(n, 5))
    text = b"".join(recs)
    return (recs, text) + packed_of(text + tail)


@functools.lru_cache(maxsize=None)
def referee(n, cycles):
    return qc_ref.qc_text(text_of(n)[1], qc_ref.conf(cycles=cycles, first_byte=b"@"))


def conf_of(cf, rows):
    from zlib_ng_amd import _lib
    return _lib.BgzfQcConf(cf.record_lines, cf.seq_line, cf.qual_line, -1 if cf.first_byte is None else cf.first_byte[0], cf.quality_base, cf.cycles,
                           cf.low_quality, _lib.BGZF_QC_ROWS if rows else 0)


def engine(ctx, blob, members, nbytes, cf, flags, rows=True, caps=None):
    return ctx.bgzf_qc_records(blob, members, 0, nbytes, cf.delimiter[0], flags, conf_of(cf, rows), BASE, caps)


def check(res, want, tail_off, rows=True, what=None):
    """every table word, every total, every row"""
    code, status, tot, tables, got = res
    t = want.totals
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.seen, tot.tail_off, tot.reserved) == (1, 0, t["seen"], tail_off, 0), what
    for name in TOTALS:
        assert getattr(tot, name) == t[name], (what, name)
    assert list(tot.base_total) == t["base_total"], what
    flat = np.array(qc_ref.flat(want), np.uint64)
    assert tables.dtype == np.uint64 and len(tables) == len(flat), what
    if not np.array_equal(tables, flat):
        at = np.nonzero(tables != flat)[0]
        raise AssertionError((what, "table words differ", at[:10].tolist(), tables[at[:10]].tolist(), flat[at[:10]].tolist()))
    if rows:
        assert list(zip(got["qsum"].tolist(), got["len"].tolist(), got["gc"].tolist(), got["n"].tolist(), got["low"].tolist())) == want.rows, what
    else:
        assert len(got) == 0, what


def test_inputs_cross_every_edge():
    """what the grid relies on, asserted of the generated reads and the referee's result"""
    reads = gen_reads(N, 5)
    assert {len(s) for _, s, _ in reads} >= set(EDGES) and max(len(s) for _, s, _ in reads) < 160
    assert set(b"".join(s for _, s, _ in reads)) == set(LETTERS) and set(b"".join(q for _, _, q in reads)) == set(QUALS)
    t = referee(N, 100).totals
    assert t["quality_clamped"] > 1000 and min(t["base_total"]) > 1000 and t["empty"] >= 10 and t["min_len"] == 0 and t["max_len"] >= 150
    assert referee(N, 100).length_hist[101] > 500 and sum(referee(N, 512).base_pos[512]) == 0 and sum(referee(N, 64).base_pos[64]) > 10000


@pytest.mark.parametrize("cycles", [1, 64, 100, 512])
def test_grid(ctx, cycles):
    """the overflow row on a strip's edge (64), off it (100, 1) and beyond every read (512); with and without rows and _FINAL"""
    from zlib_ng_amd import _lib
    want = referee(N, cycles)
    cf = qc_ref.conf(cycles=cycles, first_byte=b"@")
    recs, text, blob, members = text_of(N)
    for rows in (True, False):
        check(engine(ctx, blob, members, len(text), cf, _lib.BGZF_GREP_FINAL, rows), want, len(text), rows, (cycles, rows, "final"))
    # without _FINAL the open record behind the last whole one stays for the next call
    tail = b"@open\nACGTACGT\n+\nFFF"
    recs, text, blob, members = text_of(N, tail)
    for rows in (True, False):
        res = engine(ctx, blob, members, len(text) + len(tail), cf, 0, rows)
        check(res, want, len(text), rows, (cycles, rows, "open"))
        assert res[2].short_lines == 0
    # and with it the tail is a last record whose bodies differ in length: the fault at record N
    tot = engine(ctx, blob, members, len(text) + len(tail), cf, _lib.BGZF_GREP_FINAL)[2]
    assert (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (3, BASE + N, len(text), N + 1)


def test_small_counts(ctx):
    """fewer records than a wave's turn, one more than a span, and the literal reads of the CPU test"""
    from zlib_ng_amd import _lib
    F = _lib.BGZF_GREP_FINAL
    for n in (1, 3, 4, 5, 255, 256, 257):
        recs, text, blob, members = text_of(n)
        for cycles in (63, 129):
            cf = qc_ref.conf(cycles=cycles)
            check(engine(ctx, blob, members, len(text), cf, F), qc_ref.qc_text(text, cf), len(text), what=(n, cycles))
    tiny = b"@a\nAcGN\n+\nI! \x7f\n" + b"@b\n\n+\n\n" + b"@c\nACGT.RT\n+\n5555+5?\n"
    blob, members = packed_of(tiny)
    for kw in (dict(cycles=4), dict(cycles=7), dict(cycles=4096), dict(cycles=4, quality_base=64, low_quality=93), dict(cycles=2, quality_base=0, low_quality=0),
               dict(cycles=4, seq_line=3, qual_line=1), dict(cycles=3, qual_line=0), dict(cycles=4, record_lines=2, seq_line=1, qual_line=None),
               dict(cycles=4, record_lines=8, seq_line=5, qual_line=7), dict(cycles=4, record_lines=64, seq_line=1, qual_line=3)):
        cf = qc_ref.conf(**kw)
        try:
            want = qc_ref.qc_text(tiny, cf)
        except qc_ref.Fault as e:
            tot = engine(ctx, blob, members, len(tiny), cf, F)[2]
            assert (tot.bad, tot.bad_record) == (e.kind, BASE + e.record), kw
            continue
        check(engine(ctx, blob, members, len(tiny), cf, F), want, len(tiny), what=kw)
    # a last line without its delimiter; another delimiter; a CR is a body byte; no record at all
    for text, kw in ((b"@a\nACGT\n+\nFFFF\n@s\nACG\n+\nFF#", {}), (b"@a;ACGT;+;FF\nF;@b;AC;+;#5;", dict(delimiter=b";")), (b"@a\r\nAC\r\n+\r\nFF\r\n", {}),
                     (b"@a\nACGT\n+\nFFFF\n@s\nAC\n", dict(qual_line=None))):
        cf = qc_ref.conf(cycles=3, **kw)
        blob, members = packed_of(text)
        check(engine(ctx, blob, members, len(text), cf, F), qc_ref.qc_text(text, cf), len(text), what=text)
    text = b"@a\nACGT\n+\nFF"
    blob, members = packed_of(text)
    code, status, tot, tables, rows = engine(ctx, blob, members, len(text), qc_ref.conf(cycles=9), 0)
    assert code == 0 and (tot.seen, tot.covered, tot.tail_off, tot.min_len, tot.max_len) == (0, 1, 0, 2 ** 64 - 1, 0) and not tables.any() and len(rows) == 0


def test_one_long_read(ctx):
    """70 000 bases among short reads at cycles = 512: eight strips of the tile, then more than a thousand strips of the row at cycles"""
    from zlib_ng_amd import _lib
    rng = np.random.default_rng(9)
    n = 70000
    seq = np.frombuffer(LETTERS, np.uint8)[rng.integers(0, len(LETTERS), n)].tobytes()
    qual = np.frombuffer(QUALS, np.uint8)[rng.integers(0, len(QUALS), n)].tobytes()
    short = fastq(gen_reads(40, 3))
    text = b"".join(short[:17]) + b"@long\n%s\n+\n%s\n" % (seq, qual) + b"".join(short[17:])
    cf = qc_ref.conf(cycles=512, first_byte=b"@")
    want = qc_ref.qc_text(text, cf)
    assert want.totals["max_len"] == n and sum(want.base_pos[512]) == n - 512 and want.length_hist[513] == 1 and want.rows[17][1] == n
    blob, members = packed_of(text)
    check(engine(ctx, blob, members, len(text), cf, _lib.BGZF_GREP_FINAL), want, len(text))
    # every quality at its top: the sums of a long read (70 000 x 93) and of the file
    text = b"@long\n%s\n+\n%s\n" % (seq, b"~" * n) * 3
    want = qc_ref.qc_text(text, cf)
    assert want.totals["quality_sum"] == 3 * 93 * n and want.meanq_hist[93] == 3
    blob, members = packed_of(text)
    check(engine(ctx, blob, members, len(text), cf, _lib.BGZF_GREP_FINAL), want, len(text))


def test_two_line_fasta(ctx):
    from zlib_ng_amd import _lib
    text = b"".join(b">s%d\n%s\n" % (i, s) for i, (_, s, _) in enumerate(gen_reads(700, 8)))
    cf = qc_ref.conf(record_lines=2, qual_line=None, cycles=100, first_byte=b">")
    want = qc_ref.qc_text(text, cf)
    blob, members = packed_of(text)
    res = engine(ctx, blob, members, len(text), cf, _lib.BGZF_GREP_FINAL)
    check(res, want, len(text))
    base_pos, qual_pos, length_hist, gc_hist, meanq_hist = _lib.bgzf_qc_split(res[3], 100)
    assert not qual_pos.any() and not meanq_hist.any() and base_pos.any() and gc_hist.sum() == 700 - want.totals["empty"]
    assert (res[2].quality_sum, res[2].q20_bases, res[2].low_bases, res[2].quality_clamped) == (0, 0, 0, 0) and not res[4]["qsum"].any()


def test_capacities(ctx):
    from zlib_ng_amd import _lib
    n = 300
    recs, text, blob, members = text_of(n)
    cf = qc_ref.conf(cycles=100, first_byte=b"@")
    want = qc_ref.qc_text(text, cf)
    words = qc_ref.table_words(100)
    F = _lib.BGZF_GREP_FINAL
    # the rows one too few: BUF_ERROR, no row, tables and totals valid
    code, status, tot, tables, rows = engine(ctx, blob, members, len(text), cf, F, True, caps=(words, n - 1))
    assert code == _lib.BUF_ERROR and len(rows) == 0
    check((0, status, tot, tables, rows), want, len(text), rows=False)
    # the tables one word too few: BUF_ERROR before anything is done, nothing is written
    code, status, tot, tables, rows = engine(ctx, blob, members, len(text), cf, F, True, caps=(words - 1, n))
    assert code == _lib.BUF_ERROR and (tables == 0x5A5A5A5A5A5A5A5A).all() and tot.seen == 0
    # exact capacities; more than enough; rows not asked for with no room for them
    check(engine(ctx, blob, members, len(text), cf, F, True, caps=(words, n)), want, len(text))
    res = engine(ctx, blob, members, len(text), cf, F, True, caps=(words + 7, n + 5))
    assert (res[3][words:] == 0x5A5A5A5A5A5A5A5A).all()
    check(res[:3] + (res[3][:words], res[4]), want, len(text))
    check(engine(ctx, blob, members, len(text), cf, F, False, caps=(words, 0)), want, len(text), rows=False)
    for flags in (1, 2, 8, 16):
        with pytest.raises(_lib.EngineError):
            engine(ctx, blob, members, len(text), cf, flags)


def test_device_form(ctx):
    from zlib_ng_amd import _lib, devmem
    n = 300
    recs, text, blob, members = text_of(n)
    nb = len(text)
    cf = qc_ref.conf(cycles=100, first_byte=b"@")
    words = qc_ref.table_words(100)
    F = _lib.BGZF_GREP_FINAL
    code, status, tot_h, tables_h, rows_h = engine(ctx, blob, members, nb, cf, F)
    check((code, status, tot_h, tables_h, rows_h), qc_ref.qc_text(text, cf), nb)
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    canary = lambda size: devmem.from_host(ctx, b"\xa5" * size)
    d_tab, d_rows = canary(8 * (words + 1)), canary(24 * (n + 1))

    def dev(rows, tcap, rcap):
        return ctx.bgzf_qc_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, nb, 10, F, conf_of(cf, rows), BASE, d_scratch.ptr, nb, d_st.ptr,
                                       d_tab.ptr, tcap, d_rows.ptr if rcap else 0, rcap)

    code, tot = dev(True, words - 1, n)
    assert code == _lib.BUF_ERROR and d_tab.cpu().tobytes() == b"\xa5" * (8 * (words + 1)) and d_rows.cpu().tobytes() == b"\xa5" * (24 * (n + 1))
    code, tot = dev(True, words, n - 1)
    assert code == _lib.BUF_ERROR and (tot.seen, tot.bases, tot.bad) == (n, tot_h.bases, 0) and d_rows.cpu().tobytes() == b"\xa5" * (24 * (n + 1))
    assert d_tab.cpu().tobytes() == tables_h.tobytes() + b"\xa5" * 8
    # a fault together with a short destination: the fault wins -- the code is OK, the totals name the record, no row is written
    t = b"".join(recs[:n - 1]) + b"#" + recs[n - 1][1:]
    b, m = packed_of(t)
    d_bin, d_bm, d_bst, d_btab = devmem.from_host(ctx, b + bytes(64)), devmem.from_host(ctx, m.tobytes()), devmem.empty(ctx, 4 * len(m)), canary(8 * words)
    code, tot = ctx.bgzf_qc_records_dev(d_bin.ptr, len(b), d_bm.ptr, len(m), 0, nb, 10, F, conf_of(cf, True), BASE, d_scratch.ptr, nb, d_bst.ptr, d_btab.ptr,
                                        words, d_rows.ptr, n - 1)
    assert len(t) == nb and code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (1, BASE + n - 1, nb - len(recs[n - 1]), n)
    assert d_rows.cpu().tobytes() == b"\xa5" * (24 * (n + 1))
    code, tot = dev(False, words, 0)                            # without rows the pointer may be NULL
    assert code == 0 and bytes(tot) == bytes(tot_h) and d_tab.cpu().tobytes() == tables_h.tobytes() + b"\xa5" * 8
    code, tot = dev(True, words, n)
    assert code == 0 and bytes(tot) == bytes(tot_h) and d_tab.cpu().tobytes() == tables_h.tobytes() + b"\xa5" * 8
    assert d_rows.cpu().tobytes() == rows_h.tobytes() + b"\xa5" * 24


def test_faults(ctx):
    from zlib_ng_amd import _lib
    n = 600
    recs, text, blob, members = text_of(n)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    F = _lib.BGZF_GREP_FINAL
    cf = qc_ref.conf(cycles=100, first_byte=b"@")

    def broken(longer=(), first=()):
        """the text with a byte more in the qualities of the records `longer` and '#' as the first byte of the records `first`"""
        out = []
        for r, rec in enumerate(recs):
            rec = rec[:-1] + b"F\n" if r in longer else rec
            out.append(b"#" + rec[1:] if r in first else rec)
        t = b"".join(out)
        return (t,) + packed_of(t)

    # both faults in one text, in both orders (in two spans and in one), and a record with both
    for longer, first, want in (((400, 77), (150,), (3, 77)), ((77,), (30,), (1, 30)), ((400,), (77,), (1, 77)), ((300,), (500,), (3, 300)), ((77,), (77,), (1, 77)),
                                ((77, 78), (78,), (3, 77))):
        t, b, m = broken(longer, first)
        for rows in (True, False):
            code, status, tot, tables, got = engine(ctx, b, m, len(t), cf, F, rows)
            src = starts[want[1]] + sum(1 for x in longer if x < want[1])
            assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == want[:1] + (BASE + want[1], src, n, 1) and len(got) == 0
        with pytest.raises(qc_ref.Fault) as e:
            qc_ref.qc_text(t, cf)
        assert (e.value.kind, e.value.record) == want
    # without a qual_line the lengths are not compared; without a first_byte the first bytes are not
    t, b, m = broken(longer=(77,), first=(30,))
    cf2 = qc_ref.conf(cycles=100, qual_line=None)
    check(engine(ctx, b, m, len(t), cf2, F), qc_ref.qc_text(t, cf2), len(t))


def same(result, want, rows=True):
    t = want.totals
    assert result.base_pos.tolist() == want.base_pos and result.qual_pos.tolist() == want.qual_pos and result.length_hist.tolist() == want.length_hist
    assert result.gc_hist.tolist() == want.gc_hist and result.meanq_hist.tolist() == want.meanq_hist
    assert all(a.dtype == np.int64 for a in (result.base_pos, result.qual_pos, result.length_hist, result.gc_hist, result.meanq_hist))
    assert result.records == t["seen"] and result.base_total.tolist() == t["base_total"]
    for name in TOTALS:
        assert getattr(result, name) == (t[name] if t["seen"] or name != "min_len" else 0), name
    if rows:
        got = list(zip(result.quality_sum_per_record.tolist(), result.length.tolist(), result.gc.tolist(), result.n_bases.tolist(),
                       result.low_bases_per_record.tolist()))
        assert got == want.rows
    else:
        assert result.length is None


def test_file_with_small_read_windows(ctx, tmp_path, monkeypatch):
    """records straddle windows; a path and a reader; the parts of LineIndex.shards add up to the whole; both faults' messages; allow_short"""
    from zlib_ng_amd import bgzf
    n = 1500
    text = b"".join(fastq(gen_reads(n, 11)))
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)
    cf = qc_ref.conf(cycles=100, low_quality=20, first_byte=b"@")
    want = qc_ref.qc_text(text, cf)
    kw = dict(cycles=100, low_quality=20, first_byte=b"@")
    ctx.bgzf_stats()
    res = bgzf.qc_records(src, per_record=True, **kw)
    assert ctx.bgzf_stats()[0] >= 3                                                # (several windows)
    same(res, want)
    same(bgzf.qc_records(src, **kw), want, rows=False)
    with bgzf.open(src) as r:
        at = r.tell()
        same(r.qc_records(per_record=True, **kw), want)
        assert r.tell() == at
        # the shards of a line index, each counted on its own
        idx = bgzf.LineIndex.build(src)
        cuts = idx.shards(r, 3, lines_per_record=4)
        firsts = [i * n // 3 for i in range(4)]
        parts = [r.qc_records(per_record=True, start=cuts[i], stop=cuts[i + 1], first_record=firsts[i], **kw) for i in range(3)]
        assert [p.records for p in parts] == [b - a for a, b in zip(firsts, firsts[1:])]
        same(parts[0] + parts[1] + parts[2], want)
        recs = fastq(gen_reads(n, 11))
        same(parts[1], qc_ref.qc_text(b"".join(recs[firsts[1]:firsts[2]]), cf))
        with pytest.raises(ValueError, match="cycles 100 and 64"):
            parts[0] + r.qc_records(cycles=64, start=cuts[1], stop=cuts[2])
    # bodies of different length mid-file: the record, its virtual offset, both lengths; a wrong first byte
    lines = text.split(b"\n")
    n_seq = len(lines[4 * 900 + 1])
    lines[4 * 900 + 3] += b"FF"
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bgzf.compress(b"\n".join(lines), block_size=5000))
    with pytest.raises(ValueError, match=r"record 900 at virtual offset \d+: line 1 \(the sequence\) has %d bytes and line 3 \(the qualities\) has %d" % (n_seq, n_seq + 2)):
        bgzf.qc_records(bad, **kw)
    with pytest.raises(ValueError, match=r"record 1900 at virtual offset \d+: line 1"):
        bgzf.qc_records(bad, first_record=1000, **kw)
    lines[4 * 300] = b"x" + lines[4 * 300][1:]
    open(bad, "wb").write(bgzf.compress(b"\n".join(lines), block_size=5000))
    with pytest.raises(ValueError, match=r"record 300 at virtual offset \d+ does not start with b'@' \(first_byte\)"):
        bgzf.qc_records(bad, **kw)
    assert bgzf.qc_records(bad, cycles=100, qual_line=None).records == n              # neither is looked at
    # lines left over at the end
    short = str(tmp_path / "short.fq.gz")
    open(short, "wb").write(bgzf.compress(text + b"@s\nACGT\n", block_size=5000))
    with pytest.raises(ValueError, match=r"record 1500, the last one, has 2 of 4 lines \(allow_short\)"):
        bgzf.qc_records(short, cycles=100, qual_line=None)
    cf3 = qc_ref.conf(cycles=100, qual_line=None)
    same(bgzf.qc_records(short, cycles=100, qual_line=None, allow_short=True, per_record=True), qc_ref.qc_text(text + b"@s\nACGT\n", cf3))
    with pytest.raises(ValueError, match=r"record 1500 at virtual offset \d+: line 1 \(the sequence\) has 4 bytes and line 3 \(the qualities\) has 0"):
        bgzf.qc_records(short, cycles=100, allow_short=True)


def test_golden_file(ctx):
    from zlib_ng_amd import bgzf
    data = gzip.decompress(open(BGZIP, "rb").read())
    lines = data.split(b"\n")
    nrec = 1200                                                                    # (the referee's loops on the first 1200 records)
    part = b"\n".join(lines[:4 * nrec]) + b"\n"
    tab, _ = block_map(open(BGZIP, "rb").read())
    us = np.array([u for c, u, cs, isz in tab])
    b = int(np.searchsorted(us, len(part), "right")) - 1
    stop = bgzf.make_virtual_offset(tab[b][0], len(part) - tab[b][1])
    cf = qc_ref.conf(cycles=200, low_quality=20, first_byte=b"@")
    want = qc_ref.qc_text(part, cf)
    assert want.totals["seen"] == nrec and want.totals["bases"] > 100 * nrec
    same(bgzf.qc_records(BGZIP, stop=stop, cycles=200, low_quality=20, first_byte=b"@", per_record=True), want)
    # the whole file: the figures seqkit stats prints, from plain Python on the decoded text
    res = bgzf.qc_records(BGZIP, first_byte=b"@")
    seqs = lines[1::4]
    assert res.records == data.count(b"\n") // 4
    assert res.bases == sum(map(len, seqs[:res.records])) and res.max_len == max(map(len, seqs[:res.records])) and res.bytes_in == len(data)
    assert int(res.length_hist.sum()) == res.records and int(res.base_pos.sum()) == res.bases == int(res.qual_pos.sum())


def test_fastp_filter_feeds_trim(ctx, tmp_path):
    """a mask from the per-record rows -- mean quality below 20 or more than 2 N -- as drop= of trim_records: the output holds exactly the
    records the same filter keeps when it is computed from the referee's rows"""
    from zlib_ng_amd import bgzf
    n = 900
    reads = gen_reads(n, 21, quals=b"#,5:?FFFII")                                  # qualities 2 .. 40: both sides of the filter
    recs = fastq(reads)
    text = b"".join(recs)
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=4099))
    qc = bgzf.qc_records(src, per_record=True, first_byte=b"@")
    drop = (qc.quality_sum_per_record < 20 * qc.length) | (qc.n_bases > 2)         # (mean quality below 20, in integers)
    want = qc_ref.qc_text(text, qc_ref.conf())
    keep = [r for r, (qsum, length, gc, ns, low) in enumerate(want.rows) if not (qsum < 20 * length or ns > 2)]
    assert 100 < len(keep) < n - 100 and (~drop).nonzero()[0].tolist() == keep
    out = str(tmp_path / "kept.fq.gz")
    res = bgzf.trim_records(src, out, drop=drop, first_byte=b"@", compresslevel=1)
    assert (res.kept, res.dropped, res.too_short) == (len(keep), n - len(keep), 0)
    assert gzip.decompress(open(out, "rb").read()) == b"".join(recs[r] for r in keep)

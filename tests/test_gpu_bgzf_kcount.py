"""BGZF k-mer count (bgzf.KmerCounter, count_kmers, KmerCounts; csrc/za_kcount.hip).  The referee is kcount_ref.py: plain Python from the
statement of the rule, a dict from code to count and a loop over positions, never the code under test.  Everything is compared for
equality: every exported pair, every total and every bin of the spectrum."""
import ctypes as C
import functools

import numpy as np
import pytest

import kcount_inputs as I
import kcount_ref as R
from test_gpu_bgzf_dedup import packed_of

pytestmark = pytest.mark.gpu

BASE = 700                                                   # record_base of the calls through the C ABI
M64 = (1 << 64) - 1


def flags_of(canonical):
    from zlib_ng_amd import _lib
    return _lib.KMER_CANONICAL if canonical else 0


def conf_of(first_byte=b"@", record_lines=4, seq_line=1):
    from zlib_ng_amd import _lib
    return _lib.BgzfCountConf(record_lines, seq_line, -1 if first_byte is None else first_byte[0], 0)


def mix(x):
    """the splitmix64 step (include/zng_amd.h), on a Python integer"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ x >> 30) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ x >> 27) * 0x94D049BB133111EB) & M64
    return x ^ x >> 31


def sorted_pairs(counter, min_count=1, max_count=0):
    code, codes, counts, n = counter.export(min_count, max_count)
    assert code == 0 and codes.dtype == counts.dtype == np.uint64 and len(codes) == len(counts) == n
    order = np.argsort(codes)
    return list(zip(codes[order].tolist(), counts[order].tolist()))


def state(counter):
    i = counter.info
    assert (i.reserved, list(i.reserved2)) == (0, [0, 0, 0])
    return i.poisoned, i.cap, i.distinct, i.total


def check_counter(counter, table, what=None):
    """pairs, distinct, total and the spectrum of a counter against a referee's table"""
    assert sorted_pairs(counter) == R.pairs(table), what
    assert state(counter)[2:] == (len(table), sum(table.values())) and state(counter)[0] == 0, what
    assert counter.histogram(16).tolist() == R.spectrum(table, 16), what


def test_table_by_hand(ctx):
    from zlib_ng_amd import _lib
    # codes whose home is the last slot of a table of 64: the chain wraps.  A code given twice adds.
    last = [c for c in range(4 ** 6) if mix(c) & 63 == 63][:20]
    t = ctx.kmer_counter_new(6, 0, 0)
    assert state(t) == (0, 64, 0, 0) and (t.info.k, t.info.flags) == (6, 0) and sorted_pairs(t) == [] and t.histogram(4).tolist() == [0, 0, 0, 0]
    assert t.add(np.array(last + last[:5], np.uint64), np.array([1] * 20 + [4] * 5, np.uint64)) == 0
    want = {c: 5 if i < 5 else 1 for i, c in enumerate(last)}
    check_counter(t, want)
    assert state(t) == (0, 64, 20, 40)
    # distinct + n <= cap / 2 is asked for whatever the codes are: 20 + 13 > 32
    assert t.add(np.array(last[:13], np.uint64), np.ones(13, np.uint64)) == _lib.BUF_ERROR
    check_counter(t, want)
    # too small a room for the export: the count comes back, nothing is written
    codes, n = np.full(3, 7, np.uint64), C.c_uint64(0)
    p = C.c_void_p(codes.ctypes.data)
    assert ctx.L.zngamd_kmer_counter_export(t.h, 1, 0, p, p, 2, C.byref(n)) == _lib.BUF_ERROR and n.value == 20 and codes.tolist() == [7, 7, 7]
    assert ctx.L.zngamd_kmer_counter_export(t.h, 5, 0, p, p, 3, C.byref(n)) == _lib.BUF_ERROR and n.value == 5 and codes.tolist() == [7, 7, 7]
    # grow by reserve: 64 -> 256 -> 1024 -> 4096, each at the first room that no longer fits; the pairs and the total are kept, and the chain of the last slot is spread
    cap = 64
    for room in (12, 13, 100, 108, 109, 1000):
        cap = R.reserve(cap, 20, room)
        assert t.reserve(room) == 0 and state(t) == (0, cap, 20, 40), room
        check_counter(t, want, room)
    assert cap == 4096
    assert t.add(np.array(last[:3] + [5, 6], np.uint64), np.array([10, 10, 10, 2, M64 >> 1], np.uint64)) == 0
    want.update({last[0]: 15, last[1]: 15, last[2]: 15, 5: 2, 6: M64 >> 1})
    check_counter(t, want)
    # the cap follows the rule
    e = ctx.kmer_counter_new(31, 1, 0)
    assert e.reserve(32) == 0 and state(e) == (0, 64, 0, 0) and e.reserve(33) == 0 and state(e) == (0, 256, 0, 0)
    for room in (0, 32, 33, 1000, 2048, 2049):
        c = ctx.kmer_counter_new(5, 1, room)
        assert state(c) == (0, R.cap_of(room), 0, 0)
        c.free()
    # the carry into the high word
    top = 4 ** 31 - 1
    for count in (2 ** 32 - 1, 2 ** 32 - 1, 3):
        assert e.add(np.array([top], np.uint64), np.array([count], np.uint64)) == 0
    assert sorted_pairs(e) == [(top, 2 ** 33 + 1)] and state(e) == (0, 256, 1, 2 ** 33 + 1)
    assert e.histogram(2).tolist() == [0, 1]
    # n = 33 into a fresh table of 64 slots
    f = ctx.kmer_counter_new(6, 0, 32)
    assert f.add(np.arange(33, dtype=np.uint64), np.ones(33, np.uint64)) == _lib.BUF_ERROR and state(f) == (0, 64, 0, 0) and sorted_pairs(f) == []
    assert f.add(np.arange(32, dtype=np.uint64), np.full(32, 2, np.uint64)) == 0 and state(f) == (0, 64, 32, 64)
    check_counter(f, {c: 2 for c in range(32)})                # a table of 64 slots, half full
    assert f.add(np.array([3], np.uint64), np.array([1], np.uint64)) == _lib.BUF_ERROR      # (even a code that the table holds: the bound is n)
    # what the host refuses before any launch
    for codes, counts in (([4 ** 6], [1]), ([1], [0]), ([1, 2, 4 ** 6], [1, 1, 1])):
        with pytest.raises(_lib.EngineError):
            f.add(np.array(codes, np.uint64), np.array(counts, np.uint64))
    for bins in (0, 1, 16385):
        with pytest.raises(_lib.EngineError):
            f.histogram(bins)
    for lo, hi in ((0, 0), (3, 2)):
        with pytest.raises(_lib.EngineError):
            f.export(lo, hi)
    with pytest.raises(_lib.EngineError):
        f.reserve(1 << 32)
    with pytest.raises(_lib.EngineError):
        ctx.kmer_counter_new(32, 0, 0)
    check_counter(f, {c: 2 for c in range(32)})
    # a counter is bound to the context it was made in
    other = _lib.Context(device=0)
    try:
        text = b"@a\nACGTACGTACGT\n+\nFFFFFFFFFFFF\n"
        blob, members = packed_of(text)
        with pytest.raises(_lib.EngineError):
            other.bgzf_count_kmers(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE)
    finally:
        other.close()
    check_counter(t, want)
    for c in (t, e, f):
        c.free()
    for use in (lambda: t.info, lambda: t.reserve(1), lambda: t.histogram(4), lambda: t.export(), lambda: t.add(np.array([1], np.uint64), np.array([1], np.uint64))):
        with pytest.raises(ValueError, match="freed"):
            use()
    t.free()


# ---- the count of a window
@functools.lru_cache(maxsize=None)
def grid_text_of(k, tail=b""):
    """-> (text, BGZF blob, member table) of the reads and what follows them; blocks of 4099 bytes, so bodies straddle them"""
    text = b"".join(I.fastq(I.screen_bodies(k)))
    return (text,) + packed_of(text + tail)


@functools.lru_cache(maxsize=None)
def grid_want(k, canonical):
    """the referee's table and totals of the grid's reads, computed once"""
    return R.count_text(grid_text_of(k)[0], k, canonical)


def check_window(res, tot_want, tail_off, what=None):
    code, status, tot = res
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.short_lines, tot.reserved, tot.tail_off) == (1, 0, 0, 0, tail_off), what
    assert R.Totals(tot.seen, tot.bytes_in, tot.bases, tot.kmers, tot.claimed, tot.adds) == tot_want, what


@pytest.mark.parametrize("k,canonical", I.GRID)
def test_count_grid(ctx, k, canonical):
    """every pair and every total against the referee; with and without _FINAL; the open tail"""
    from zlib_ng_amd import _lib
    want, tot_want = grid_want(k, canonical)
    text, blob, members = grid_text_of(k)
    assert tot_want.seen > 1990 and tot_want.adds <= tot_want.kmers and (k < 3 or tot_want.adds > tot_want.kmers // 2)
    t = ctx.kmer_counter_new(k, flags_of(canonical), len(text))
    cap = R.cap_of(len(text))
    check_window(ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE), tot_want, len(text), "final")
    check_counter(t, want)
    assert state(t) == (0, cap, tot_want.claimed, tot_want.kmers) and tot_want.claimed == len(want)
    t.free()
    # without _FINAL the open record behind the last whole one is not counted
    tail_body = I.rand_seq(np.random.default_rng(k), 65)
    tail = b"@open\n" + tail_body + b"\n+\nFFF"
    text, blob, members = grid_text_of(k, tail)
    t = ctx.kmer_counter_new(k, flags_of(canonical), len(text) + len(tail))
    check_window(ctx.bgzf_count_kmers(blob, members, 0, len(text) + len(tail), 10, 0, conf_of(), t, BASE), tot_want, len(text), "open")
    check_counter(t, want)
    # the next call counts it: the claims are those of the tail alone
    more, tot_more = R.count_text(tail, k, canonical, table=dict(want))
    check_window(ctx.bgzf_count_kmers(blob, members, len(text), len(text) + len(tail), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE + tot_want.seen), tot_more,
                 len(text) + len(tail), "the tail")
    check_counter(t, more)
    assert state(t)[2:] == (len(more), tot_want.kmers + tot_more.kmers)
    t.free()


@pytest.mark.parametrize("k,canonical", [(31, True), (31, False), (15, True), (3, False)])
def test_repeats(ctx, k, canonical):
    """poly-G, short periods, reverse palindromes, an N inside a run, runs across a strip edge: adds is the referee's runs"""
    from zlib_ng_amd import _lib
    bodies = I.repeat_bodies(k)
    text = b"".join(I.fastq(bodies))
    blob, members = packed_of(text)
    want, tot_want = R.count_text(text, k, canonical)
    if k == 31:
        assert R.count_bodies([b"G" * 150], k, canonical)[1:3] == (120, 2) and tot_want.adds < tot_want.kmers
    t = ctx.kmer_counter_new(k, flags_of(canonical), len(text))
    check_window(ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE), tot_want, len(text))
    check_counter(t, want)
    t.free()
    # each read alone, in a text of its own: its runs
    for b in bodies[:8]:
        one = b"@r\n" + b + b"\n+\n" + b"F" * len(b) + b"\n"
        bl, mm = packed_of(one)
        w, tw = R.count_text(one, k, canonical)
        t = ctx.kmer_counter_new(k, flags_of(canonical), len(one))
        check_window(ctx.bgzf_count_kmers(bl, mm, 0, len(one), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, 0), tw, len(one), b)
        check_counter(t, w, b)
        t.free()


def test_contention(ctx):
    """4 096 copies of one read: every wave adds to the same 120 slots"""
    from zlib_ng_amd import _lib
    k, read = 31, I.contention_read()
    single, kmers, adds, _ = R.count_bodies([read], k, True)
    assert kmers == adds == 120 == len(single)
    text = b"".join(I.fastq([read] * I.CONTENTION))
    blob, members = packed_of(text, 65280)
    t = ctx.kmer_counter_new(k, 1, len(text))
    tot_want = R.Totals(I.CONTENTION, len(text), 150 * I.CONTENTION, 120 * I.CONTENTION, 120, 120 * I.CONTENTION)
    check_window(ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE), tot_want, len(text))
    check_counter(t, {c: n * I.CONTENTION for c, n in single.items()})
    spectrum = t.histogram(I.CONTENTION + 2).tolist()
    assert spectrum[I.CONTENTION] == 120 and sum(spectrum) == 120
    t.free()


def test_accumulation(ctx):
    """two calls into one counter, the first cut by the window's end inside a record, the second from tail_off on: one call over all"""
    from zlib_ng_amd import _lib
    k, canonical = 17, True
    want, tot_want = grid_want(k, canonical)
    text, blob, members = grid_text_of(k)
    recs = I.fastq(I.screen_bodies(k))
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    cut_rec = 901                                            # the record that the first window's end cuts
    assert len(I.screen_bodies(k)[cut_rec]) >= 30
    at = int(starts[cut_rec])
    cut = at + 30                                            # inside its sequence
    t = ctx.kmer_counter_new(k, 1, 0)
    assert ctx.bgzf_count_kmers(blob, members, 0, cut, 10, 0, conf_of(), t, BASE)[0] == _lib.BUF_ERROR and state(t) == (0, 64, 0, 0)      # no room: nothing ran
    assert t.reserve(cut) == 0 and state(t)[1] == R.reserve(64, 0, cut)
    first, tot_first = R.count_text(text[:at], k, canonical)
    code, status, tot = res = ctx.bgzf_count_kmers(blob, members, 0, cut, 10, 0, conf_of(), t, BASE)
    check_window(res, tot_first, at, "first")
    assert tot.seen == cut_rec
    check_counter(t, first)
    room = len(text) - tot.tail_off
    cap = R.reserve(state(t)[1], len(first), room)
    assert t.reserve(room) == 0 and state(t) == (0, cap, len(first), tot_first.kmers)
    both, tot_second = R.count_text(text[at:], k, canonical, table=dict(first))
    check_window(ctx.bgzf_count_kmers(blob, members, tot.tail_off, len(text), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE + cut_rec), tot_second, len(text), "second")
    assert both == want and tot_first.claimed + tot_second.claimed == len(want) and tot_first.adds + tot_second.adds == tot_want.adds
    check_counter(t, want)
    t.free()


@pytest.mark.parametrize("bins", [2, 3, 16, 16384])
def test_spectrum_and_export_filter(ctx, bins):
    """the spectrum of all codes in every number of bins; the export filter leaves it as it is"""
    k, canonical = 15, True
    want, tot_want = grid_want(k, canonical)
    text, blob, members = grid_text_of(k)
    from zlib_ng_amd import _lib
    t = ctx.kmer_counter_new(k, 1, len(text))
    check_window(ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, _lib.BGZF_GREP_FINAL, conf_of(), t, BASE), tot_want, len(text))
    assert t.add(np.array([0, 1], np.uint64), np.array([20000, 16382], np.uint64)) == 0      # counts at and beyond the last bin of 16384
    want = dict(want)
    want[0], want[1] = want.get(0, 0) + 20000, want.get(1, 0) + 16382
    spectrum = R.spectrum(want, bins)
    assert spectrum[0] == 0 and sum(spectrum) == len(want) and spectrum[-1] >= 1
    assert t.histogram(bins).tolist() == spectrum
    for lo, hi in ((1, 0), (2, 0), (2, 5), (10 ** 9, 0)):
        got = sorted_pairs(t, lo, hi)
        assert got == R.pairs(want, lo, hi) and (len(got) > 0) == (lo < 10 ** 9)
        assert t.histogram(bins).tolist() == spectrum
    t.free()


def test_faults(ctx, tmp_path):
    from zlib_ng_amd import _lib, bgzf
    F = _lib.BGZF_GREP_FINAL
    k, canonical = 17, True
    want, tot_want = grid_want(k, canonical)
    text, blob, members = grid_text_of(k)
    recs = I.fastq(I.screen_bodies(k))
    n = len(recs)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    # the first byte: the smallest record at fault; the counter is poisoned and refuses everything but describe and free
    bad_text = b"".join(b"#" + r[1:] if i in (1500, 77) else r for i, r in enumerate(recs))
    b, m = packed_of(bad_text)
    t = ctx.kmer_counter_new(k, 1, len(text))
    code, status, tot = ctx.bgzf_count_kmers(b, m, 0, len(bad_text), 10, F, conf_of(), t, BASE)
    assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (1, BASE + 77, starts[77], n, 1)
    assert t.info.poisoned == 1 and (t.info.distinct, t.info.total) == (0, 0)
    for use in (lambda: ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, F, conf_of(), t, BASE), lambda: t.reserve(1), lambda: t.histogram(4),
                lambda: t.export(), lambda: t.add(np.array([1], np.uint64), np.array([1], np.uint64))):
        with pytest.raises(_lib.EngineError):
            use()
    assert t.info.poisoned == 1
    t.free()
    # without the check the same text counts
    t = ctx.kmer_counter_new(k, 1, len(text))
    check_window(ctx.bgzf_count_kmers(b, m, 0, len(bad_text), 10, F, conf_of(first_byte=None), t, BASE), tot_want, len(text))
    # what the call refuses before the context is touched leaves the counter as it was
    for flags in (1, 2, 8, 16):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, flags, conf_of(), t, BASE)
    for cf in (_lib.BgzfCountConf(0, 0, -1, 0), _lib.BgzfCountConf(65, 1, -1, 0), _lib.BgzfCountConf(4, 4, -1, 0), _lib.BgzfCountConf(4, -1, -1, 0),
               _lib.BgzfCountConf(4, 1, 256, 0), _lib.BgzfCountConf(4, 1, -1, 1)):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_count_kmers(blob, members, 0, len(text), 10, F, cf, t, BASE)
    check_counter(t, want)
    t.free()
    # through the file: the error of every record call, and the counter refuses further use
    src, bad = str(tmp_path / "reads.fq.gz"), str(tmp_path / "bad.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    open(bad, "wb").write(bgzf.compress(bad_text, block_size=5000))
    kc = bgzf.KmerCounter(k, canonical)
    with pytest.raises(ValueError, match=r"record 77 at virtual offset \d+ does not start with b'@' \(first_byte\)"):
        kc.add_file(bad, first_byte=b"@")
    for use in (lambda: kc.add_file(src), kc.result):
        with pytest.raises(ValueError, match="cannot be used"):
            use()
    kc.close()
    # a block that does not decode
    raw = bytearray(open(src, "rb").read())
    at = len(raw) // 2
    raw[at:at + 8] = bytes(x ^ 0x5A for x in raw[at:at + 8])
    broken = str(tmp_path / "broken.fq.gz")
    open(broken, "wb").write(bytes(raw))
    kc = bgzf.KmerCounter(k, canonical)
    with pytest.raises((bgzf.BadGzipFile, EOFError)):
        kc.add_file(broken)
    kc.close()
    # a short last record
    short = str(tmp_path / "short.fq.gz")
    open(short, "wb").write(bgzf.compress(text + b"@s\nACGTACGTACGTACGTACGTAAA\n", block_size=5000))
    with pytest.raises(ValueError, match=r"record %d, the last one, has 2 of 4 lines \(allow_short\)" % n):
        bgzf.count_kmers(short, k)
    res = bgzf.count_kmers(short, k, allow_short=True)
    assert res.records == n + 1 and res.kmers == tot_want.kmers + 7
    # a table that may not grow: MemoryError naming the bytes, at once, and nothing was launched
    kc = bgzf.KmerCounter(k, canonical, max_table_bytes=1024)
    with pytest.raises(MemoryError, match=r"needs %d bytes" % (16 * R.reserve(64, 0, len(text)))):
        kc.add_file(src)
    assert kc._table.info.distinct == 0 and kc._table.info.poisoned == 0 and kc.result().distinct == 0
    kc.close()
    with pytest.raises(ValueError, match="closed"):
        kc.result()


def same(res, want, tot_want, k, canonical, min_count=1, max_count=None, bins=10001, files=1):
    assert [res.codes.dtype, res.counts.dtype, res.spectrum.dtype] == [np.uint64] * 3
    assert (res.k, res.canonical, res.min_count, res.max_count, res.bins) == (k, canonical, min_count, max_count, bins)
    assert list(zip(res.codes.tolist(), res.counts.tolist())) == ([] if min_count is None else R.pairs(want, min_count, max_count or 0))
    assert res.spectrum.tolist() == R.spectrum(want, bins)
    assert (res.records, res.bases, res.kmers, res.distinct) == (files * tot_want.seen, files * tot_want.bases, sum(want.values()), len(want))


def test_python_face(ctx, tmp_path, monkeypatch):
    """a path and an open file, small read windows, a table that grows from 64 slots; shards and files add up; the counted k-mers as the
    set of a screen"""
    from zlib_ng_amd import bgzf
    k, canonical = 17, True
    want, tot_want = grid_want(k, canonical)
    text = grid_text_of(k)[0]
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)
    ctx.bgzf_stats()
    whole = bgzf.count_kmers(src, k, first_byte=b"@")
    assert ctx.bgzf_stats()[0] >= 3                                                # (several windows)
    same(whole, want, tot_want, k, canonical)
    # a counter that starts at 64 slots and must grow three times: 13 000 random reads, nearly all of their 1.09 million k-mers new, in
    # windows of some 10^5 bytes -- 64 -> 2^19 at the first window, -> 2^21 beyond 2^18 codes, -> 2^23 beyond 2^20
    rng = np.random.default_rng(11)
    grow_text = b"".join(I.fastq([I.rand_seq(rng, 100) for _ in range(13000)]))
    grow_want, grow_tot = R.count_text(grow_text, k, canonical)
    grow = str(tmp_path / "grow.fq.gz")
    open(grow, "wb").write(bgzf.compress(grow_text, block_size=5000))
    kc = bgzf.KmerCounter(k, canonical, _room=0)
    caps = []
    reserve = kc._reserve
    monkeypatch.setattr(kc, "_reserve", lambda c, room: (reserve(c, room), caps.append(kc._table.info.cap))[0])
    assert kc.add_file(grow, first_byte=b"@") is kc
    assert len(grow_want) > 1 << 20 and caps[0] > 64 and len(set(caps)) >= 3 and caps == sorted(caps) and caps[-1] >= 2 * len(grow_want)
    same(kc.result(), grow_want, grow_tot, k, canonical)
    kc.close()
    # an open file
    kc = bgzf.KmerCounter(k, canonical, _room=0)
    with open(src, "rb") as f:
        assert kc.add_file(f, first_byte=b"@") is kc
    assert kc.result() == whole
    same(kc.result(2, 5, 16), want, tot_want, k, canonical, 2, 5, 16)
    same(kc.result(None, bins=3), want, tot_want, k, canonical, None, None, 3)          # the spectrum only
    # a second file through the same counter: the sum of two results
    kc.add_file(src)
    twice = {c: 2 * v for c, v in want.items()}
    same(kc.result(), twice, tot_want, k, canonical, files=2)
    assert kc.result() == whole + whole
    kc.close()
    # both reads of a pair in one call; what a result holds goes into a counter again
    assert bgzf.count_kmers([src, src], k) == whole + whole
    with bgzf.KmerCounter(k, canonical) as kc2:
        assert kc2.add_counts(whole).add_counts(whole).result() == whole + whole
    # the shards of a file, added
    with bgzf.open(src) as r:
        idx = bgzf.LineIndex.build(src)
        cuts = idx.shards(r, 3, lines_per_record=4)
    parts = []
    for i in range(3):
        with bgzf.KmerCounter(k, canonical) as part:
            parts.append(part.add_file(src, start=cuts[i], stop=cuts[i + 1], first_byte=b"@").result())
    assert [p.records for p in parts] == [tot_want.seen * (i + 1) // 3 - tot_want.seen * i // 3 for i in range(3)]
    assert parts[0] + parts[1] + parts[2] == whole
    # the k-mers of this run as the set of a screen of the same file: every valid k-mer of every read hits
    kset = bgzf.count_kmers(src, k).to_kmerset()
    assert len(kset) == len(want) and kset.names == ("counted",)
    res = bgzf.screen_records(src, kset)
    assert (res.hits == res.kmers).all() and int(res.kmers.sum()) == tot_want.kmers
    solid = whole.to_kmerset(min_count=2)
    assert solid.codes.tolist() == [c for c, v in R.pairs(want, 2)]
    res = bgzf.screen_records(src, solid)
    assert int(res.hits.sum()) == sum(v for c, v in want.items() if v >= 2)

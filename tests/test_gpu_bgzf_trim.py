"""BGZF trimmed (bgzf.trim_records; csrc/za_trim.hip).  The referee is trim_ref.py: plain Python with the serial loops of the rule as
include/zng_amd.h states it, never the code under test.  For the one read of 70 000 bases the referee's loops are written with numpy."""
import functools
import gzip
import random

import numpy as np
import pytest

import trim_ref
from test_gpu_bgzf_grep import block_map
from test_gpu_bgzf_lines import BGZIP, member_table

pytestmark = pytest.mark.gpu

ADAPTERS = [b"AGATCGGAAGAGCACACGTC", b"CTGTCTCTTATACACATCT", b"TGGAATTCTCGG"]      # 20, 19 and 12 bytes
BASE = 500                                                   # record_base of the calls through the C ABI
EDGES = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 150]


def gen_reads(n, seed):
    """-> [(name, seq, qual)]: lengths from EDGES or random below 160; two thirds with one of ADAPTERS planted at a random place with 0 to 2
    substitutions and cut off at the read's end; a low-quality tail of 0 to 11 bytes"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = rng.choice(EDGES) if i % 7 == 0 else rng.randrange(0, 160)
        s = bytes(rng.choice(b"ACGT") for _ in range(L))
        if i % 3 and L:
            A = bytearray(ADAPTERS[i % 3 - 1 if i % 5 else 2])
            for at in rng.sample(range(len(A)), rng.randrange(0, 3)):
                A[at] = rng.choice([c for c in b"ACGT" if c != A[at]])
            s = (s[:rng.randrange(0, L + 1)] + bytes(A) + s)[:L]
        q = bytearray(rng.choice(b"FFFFF:,#") for _ in range(L))
        for x in range(max(0, L - rng.randrange(0, 12)), L):
            q[x] = rng.choice(b"#,")
        out.append((b"@r%d" % i, s, bytes(q)))
    return out


def fastq(reads):
    return [b"%s\n%s\n+\n%s\n" % r for r in reads]


def packed_of(text, block_size=4099):
    from zlib_ng_amd import bgzf
    blob = bgzf.compress(text, block_size=block_size)
    tab, _ = block_map(blob)
    return blob, member_table(tab)


@functools.lru_cache(maxsize=None)
def raw_of(n):
    recs = fastq(gen_reads(n, 5))
    return recs, b"".join(recs)


@functools.lru_cache(maxsize=None)
def text_of(n):
    """-> (records, text, BGZF blob, member table) of n generated reads: computed once per n, never changed"""
    return raw_of(n) + packed_of(raw_of(n)[1])


# name -> (the rule's arguments, the too-short records are gathered, every third record is dropped)
CONFIGS = {
    "nothing": (dict(), False, False),
    "fixed": (dict(cut=(3, 5)), False, False),
    "quality": (dict(quality=(20, 20)), False, False),
    "adapters k=0": (dict(adapters=ADAPTERS), False, False),
    "adapters k=2": (dict(adapters=ADAPTERS, mismatches=2), False, False),
    "everything": (dict(cut=(1, 0), quality=(20, 20), adapters=ADAPTERS, mismatches=2, min_length=20), True, False),
    "everything, dropped": (dict(cut=(1, 0), quality=(20, 20), adapters=ADAPTERS, mismatches=2, min_length=20), True, True),
}


@functools.lru_cache(maxsize=None)
def referee(n, name):
    kw, keep_short, dropped = CONFIGS[name]
    drop = [r % 3 == 0 for r in range(n)] if dropped else None
    return trim_ref.trim_text(raw_of(n)[1], trim_ref.conf(first_byte=b"@", **kw), drop), drop


def conf_of(cf, keep_short=False):
    from zlib_ng_amd import _lib
    return _lib.BgzfTrimConf(cf.record_lines, cf.seq_line, cf.qual_line, -1 if cf.first_byte is None else cf.first_byte[0], cf.cut[0], cf.cut[1],
                             cf.quality[0], cf.quality[1], cf.quality_base, cf.mismatches, cf.min_overlap, cf.min_length,
                             _lib.BGZF_TRIM_KEEP_SHORT if keep_short else 0)


def engine(ctx, blob, members, nbytes, cf, flags, keep_short=False, drop=None, caps=None):
    from zlib_ng_amd import _lib
    ads, table = _lib.grep_pattern_table(cf.adapters) if cf.adapters else (b"", np.empty((0, 2), np.uint32))
    return ctx.bgzf_trim_records(blob, members, 0, nbytes, ads, table, cf.delimiter[0], flags, conf_of(cf, keep_short), BASE,
                                 None if drop is None else np.array(drop, np.uint8), caps)


def check(res, want, text, cf, keep_short, group=True, final=True, what=None):
    """every trim row, every total, the rows by class then number with the new lengths, the bytes per class"""
    code, status, tot, trim, rows, packed = res
    t = want.totals
    n = t["seen"]
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.drop_short, tot.seen, tot.tail_off) == (1, 0, 0, n, len(text)), what
    assert trim["begin"].tolist() == want.begin and trim["end"].tolist() == want.end and trim["verdict"].tolist() == want.verdict, what
    assert trim["adapter"].tolist() == [255 if j < 0 else j for j in want.adapter] and trim["steps"].tolist() == want.steps and not trim["reserved"].any(), what
    for name in ("kept", "too_short", "dropped", "bytes_in", "bases_in", "bases_out", "quality_trimmed", "adapter_trimmed"):
        assert getattr(tot, name) == t[name], (what, name)
    assert list(tot.adapter_records) == t["adapter_records"] + [0] * (64 - len(cf.adapters)), what
    pieces = want.kept_bytes + (want.short_bytes if keep_short else [])
    assert tot.bytes == sum(map(len, pieces)), what
    if not group:
        assert len(rows) == 0 and packed == b"", what
        return
    v = np.array(want.verdict, np.int64)
    order = np.concatenate([np.nonzero(v == 0)[0], np.nonzero(v == 1)[0] if keep_short else np.empty(0, np.int64)])
    starts = np.array(trim_ref.split_records(text, cf.record_lines, cf.delimiter, final)[1], np.int64)
    assert rows["number"].tolist() == (BASE + order).tolist() and rows["src_off"].tolist() == starts[order].tolist(), what
    assert rows["len"].tolist() == [len(x) for x in pieces] and rows["reserved"].tolist() == v[order].tolist(), what
    assert bytes(packed) == b"".join(pieces), what


def test_inputs_cross_every_edge():
    """what the grid relies on, asserted of the referee's result for n = 773"""
    want, _ = referee(773, "everything")
    reads = gen_reads(773, 5)
    assert min(want.totals["adapter_records"]) >= 50
    partial = subs = 0
    for _, s, q in reads:
        a, b = trim_ref.fixed_cut(len(s), 1, 0)
        a, b = trim_ref.quality_cut(q, a, b, 20, 20)
        p, j = trim_ref.adapter_cut(s[a:b], ADAPTERS, 2, 3)
        if j >= 0:
            o = min(len(ADAPTERS[j]), b - a - p)
            partial += o < len(ADAPTERS[j])
            subs += any(x != y for x, y in zip(s[a + p:a + p + o], ADAPTERS[j][:o]))
    assert partial >= 50 and subs >= 50 and want.totals["too_short"] >= 100 and want.totals["kept"] >= 100
    assert {len(s) for _, s, _ in reads} >= set(EDGES)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 773])
def test_grid(ctx, n):
    from zlib_ng_amd import _lib
    recs, text, blob, members = text_of(n)
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    for name, (kw, keep_short, _) in CONFIGS.items():
        want, drop = referee(n, name)
        cf = trim_ref.conf(first_byte=b"@", **kw)
        res = engine(ctx, blob, members, len(text), cf, F | G, keep_short, drop)
        check(res, want, text, cf, keep_short, what=(n, name))
        if name == "nothing":                                  # the bytes are the input, the rows those of partition_records with one class
            assert bytes(res[5]) == text
            part = ctx.bgzf_partition_records(blob, members, 0, len(text), 10, F | G, 4, ord("@"), BASE, np.zeros(n, np.uint16), 1)
            assert res[4].tobytes() == part[5].tobytes() and bytes(part[6]) == text
        # without _GROUP: the same rows and totals, and nothing else
        check(engine(ctx, blob, members, len(text), cf, F, keep_short, drop), want, text, cf, keep_short, group=False, what=(n, name))
    # the too-short records counted only: the kept ones alone are gathered
    kw, _, _ = CONFIGS["everything"]
    want, _ = referee(n, "everything")
    cf = trim_ref.conf(first_byte=b"@", **kw)
    check(engine(ctx, blob, members, len(text), cf, F | G, False), want, text, cf, False, what=(n, "counted only"))


def run(ctx, text, keep_short=True, drop=None, final=True, **kw):
    """one small text through the engine and the referee"""
    from zlib_ng_amd import _lib
    cf = trim_ref.conf(**kw)
    blob, members = packed_of(text, 4099)
    want = trim_ref.trim_text(text, cf, drop, final)
    res = engine(ctx, blob, members, len(text), cf, (_lib.BGZF_GREP_FINAL if final else 0) | _lib.BGZF_CLASSIFY_GROUP, keep_short, drop)
    check(res, want, text, cf, keep_short, what=kw)
    return want


def np_quality_back(q, a, b, cutoff, base=33):
    s = np.cumsum((cutoff - (np.frombuffer(q, np.uint8)[a:b].astype(np.int64) - base))[::-1])
    neg = np.nonzero(s < 0)[0]
    s = s[:neg[0]] if len(neg) else s
    if not len(s) or s.max() <= 0:
        return b
    return b - 1 - int(np.argmax(s))


def np_adapter(R, adapters, k, min_overlap):
    """-> (p, j) as trim_ref.adapter_cut returns it"""
    R = np.frombuffer(R, np.uint8)
    m, best = len(R), (len(R), trim_ref.NO_ADAPTER)
    for j, A in enumerate(adapters):
        A = np.frombuffer(A, np.uint8)
        L, p = len(A), m
        if m >= L:
            hit = np.nonzero((np.lib.stride_tricks.sliding_window_view(R, L) != A).sum(1) <= k)[0]
            p = int(hit[0]) if len(hit) else m
        if p == m:
            for x in range(max(0, m - L + 1), m):
                if m - x >= min(min_overlap, L) and int((R[x:] != A[:m - x]).sum()) <= (k * (m - x)) // L:
                    p = x
                    break
        if p < best[0]:
            best = (p, j)
    return best


def test_numpy_referee_is_the_referee():
    rng = random.Random(4)
    for _ in range(300):
        n = rng.randrange(0, 90)
        s, q = bytes(rng.choice(b"ACGT") for _ in range(n)), bytes(rng.choice(b"I5#,") for _ in range(n))
        if n > 30 and rng.random() < 0.7:
            at = rng.randrange(n)
            s = (s[:at] + ADAPTERS[rng.randrange(3)] + s)[:n]
        a = rng.randrange(0, n + 1)
        b = rng.randrange(a, n + 1)
        k = rng.randrange(0, 3)
        assert np_quality_back(q, a, b, 20) == trim_ref.quality_cut(q, a, b, 0, 20)[1]
        assert np_adapter(s[a:b], ADAPTERS, k, 3) == trim_ref.adapter_cut(s[a:b], ADAPTERS, k, 3)


def test_one_long_read(ctx):
    """70 000 bases: more than a thousand strips and four tiles; a low-quality tail of 40 000 and an adapter at 65 530, behind the
    quality cut, or one at 29 990, across it; the referee's loops written with numpy"""
    from zlib_ng_amd import _lib
    rng = np.random.default_rng(9)
    n = 70000
    seq = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())
    seq[65530:65550] = ADAPTERS[0]
    qual = bytearray(np.frombuffer(b"FF:I", np.uint8)[rng.integers(0, 4, n)].tobytes())
    qual[30000:] = np.frombuffer(b"#,#5", np.uint8)[rng.integers(0, 4, 40000)].tobytes()
    seq, qual = bytes(seq), bytes(qual)
    seq2 = seq[:29990] + ADAPTERS[0] + seq[30010:]
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    ads = [ADAPTERS[0], ADAPTERS[0][:10] + b"TTTTTTTTTT"]             # (20 bytes each: two mismatches in them match nowhere by chance)
    for s, cutoff, k, expect in ((seq, 0, 2, (70000, 65530, 0)), (seq, 20, 2, None), (seq2, 20, 2, None)):
        cf = trim_ref.conf(first_byte=b"@", quality=(0, cutoff), adapters=ads, mismatches=k)
        b = np_quality_back(qual, 0, n, cutoff) if cutoff else n
        p, j = np_adapter(s[:b], ads, k, 3)
        assert expect is None or (b, p, j) == expect
        assert cutoff == 0 or 29995 < b < 30100
        assert s is seq or (p, j) == (29990, 0)
        text = b"@long\n%s\n+\n%s\n@next\nACGT\n+\nFFFF\n" % (s, qual)
        blob, members = packed_of(text)
        code, status, tot, trim, rows, packed = engine(ctx, blob, members, len(text), cf, F | G)
        assert code == 0 and (tot.seen, tot.kept, tot.bad) == (2, 2, 0)
        assert (int(trim["begin"][0]), int(trim["end"][0]), int(trim["adapter"][0])) == (0, p, 255 if j < 0 else j)
        assert int(trim["steps"][0]) == (2 if b < n else 0) | (4 if j >= 0 else 0)
        assert (tot.quality_trimmed, tot.adapter_trimmed, tot.bases_in, tot.bases_out) == (n - b, b - p, n + 4, p + 4)
        assert bytes(packed) == b"@long\n%s\n+\n%s\n@next\nACGT\n+\nFFFF\n" % (s[:p], qual[:p]) and rows["len"].tolist() == [2 * p + 10, 18]


def test_adapter_edges(ctx):
    rng = random.Random(3)
    body = lambda n: bytes(rng.choice(b"CT") for _ in range(n))           # (no A, no G: nothing matches by chance)
    fq = lambda seqs: b"".join(b"@e%d\n%s\n+\n%s\n" % (i, s, b"F" * len(s)) for i, s in enumerate(seqs))
    A = ADAPTERS[0]
    # adapters that begin at byte 60 and at byte 63 of a strip, in the first strip and in the third; cut off at the read's end
    seqs = [body(at) + A + body(tail) for at in (60, 63, 64, 128 + 60, 128 + 63) for tail in (0, 30)] + [body(at) + A[:cut] for at in (60, 63, 191) for cut in (2, 3, 4, 19)]
    want = run(ctx, fq(seqs), adapters=ADAPTERS, min_length=10)
    assert want.end[:10] == [60, 60, 63, 63, 64, 64, 188, 188, 191, 191] and want.adapter[10:14] == [-1, 0, 0, 0]
    run(ctx, fq(seqs), adapters=ADAPTERS, mismatches=2, min_overlap=1)
    # an adapter longer than the read; min_overlap 1; min_overlap larger than an adapter
    long = bytes(rng.choice(b"ACGT") for _ in range(255))
    seqs = [long[:10], long[:3], body(5) + long[:100], body(70) + long, body(70) + long[:254], long[:1], b""]
    want = run(ctx, fq(seqs), adapters=[long], mismatches=16)
    assert want.adapter == [0, 0, 0, 0, 0, -1, -1] and want.end[:5] == [0, 0, 5, 70, 70]
    run(ctx, fq(seqs), adapters=[long], min_overlap=1)
    want = run(ctx, fq([body(40) + b"AG", body(40) + b"A", body(20) + b"AG" + body(9)]), adapters=[b"AG", A], min_overlap=5)
    assert want.adapter == [0, -1, 0]
    # 64 adapters: the lowest index among those that match at the smallest place
    many = [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(8, 40))) for _ in range(62)]
    many += [many[7] + b"A", many[7][:6]]
    seqs = [body(rng.randrange(0, 100)) + many[j] + body(rng.randrange(0, 20)) for j in range(64)] + [body(30) + many[7][:5]]
    want = run(ctx, fq(seqs), adapters=many, mismatches=1)
    assert want.adapter[7] == 7 and want.adapter[62] == 7 and want.adapter[63] in (7, 63) and len(set(want.adapter)) > 50


def test_quality_and_record_edges(ctx):
    # the early stop as a real record; bytes below the base; quality_base 64
    want = run(ctx, b"@s\nACGTACGT\n+\nIIII##I#\n", quality=(0, 20))
    assert (want.begin, want.end) == ([0], [7])
    run(ctx, b"@a\nACGTAC\n+\nII \x1fI!\n@b\nACGT\n+\n\x00\x01II\n", quality=(20, 20))
    want = run(ctx, b"@a\nACGTACGT\n+\nhhhhhBBB\n@b\nACGT\n+\nBhhB\n", quality=(20, 20), quality_base=64)
    assert want.end == [5, 3] and want.begin == [0, 1]
    run(ctx, b"@a\nACGT\n+\n####\n@b\n\n+\n\n", quality=(20, 20), min_length=1)                     # cut to nothing; an empty read
    # two-line records without qualities; eight-line records; another delimiter
    run(ctx, b">a\nACGTACGTAGATCGGAAGAGC\n>b\nAC\n>c\n\n", record_lines=2, qual_line=None, cut=(1, 1), adapters=ADAPTERS, min_length=3)
    pair = b"@p/1\nAAAA\n+\nFFFF\n@p/2\nACGTACGTAGATCGG\n+\nFFFFFFFFFFFF#,#\n"
    want = run(ctx, pair * 3, record_lines=8, seq_line=5, qual_line=7, quality=(0, 20), adapters=ADAPTERS)
    assert want.end == [8] * 3 and want.kept_bytes[0] == b"@p/1\nAAAA\n+\nFFFF\n@p/2\nACGTACGT\n+\nFFFFFFFF\n"
    run(ctx, b"@a;ACGTAGATCGGAAG;+;FFFFFFFFFFFF#,;@b;AC\nGT;+;FFF#,;", delimiter=b";", quality=(0, 20), adapters=ADAPTERS)
    run(ctx, b"@a\nFFFF,#\n+\nACGTAC\n", seq_line=3, qual_line=1, quality=(0, 20))                 # the qualities in front of the sequence
    # a short last record; a last line without its delimiter; without _FINAL both stay for the next call
    rec = b"@a\nACGTACGT\n+\nFFFFFF#,\n"
    want = run(ctx, rec + b"@s\n", quality=(0, 20))
    assert want.kept_bytes == [b"@a\nACGTAC\n+\nFFFFFF\n", b"@s\n"]
    want = run(ctx, rec + b"@s\nACGTACGT\n+\nFFFFFF#,", quality=(0, 20), cut=(1, 0))
    assert want.kept_bytes[1] == b"@s\nCGTAC\n+\nFFFFF"
    run(ctx, rec + b"@s\nACGT", qual_line=None, cut=(0, 2))
    from zlib_ng_amd import _lib
    text = rec + b"@s\nACGT\n+\nFF"
    blob, members = packed_of(text)
    cf = trim_ref.conf(quality=(0, 20))
    res = engine(ctx, blob, members, len(text), cf, _lib.BGZF_CLASSIFY_GROUP)
    assert (res[2].seen, res[2].tail_off, res[2].short_lines, res[2].bad) == (1, len(rec), 0, 0) and bytes(res[5]) == b"@a\nACGTAC\n+\nFFFFFF\n"


def test_faults(ctx):
    from zlib_ng_amd import _lib
    n = 300
    recs, text, blob, members = text_of(n)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    cf = trim_ref.conf(first_byte=b"@", quality=(20, 20), adapters=ADAPTERS, mismatches=2, min_length=20)
    nothing = lambda res: len(res[3]) == 0 and len(res[4]) == 0 and res[5] == b""

    def broken(longer=(), first=()):
        """the text with a byte more in the qualities of the records `longer` and '#' as the first byte of the records `first`"""
        out = []
        for r, rec in enumerate(recs):
            rec = rec[:-1] + b"F\n" if r in longer else rec
            out.append(b"#" + rec[1:] if r in first else rec)
        t = b"".join(out)
        return (t,) + packed_of(t)

    # bodies of different length at two records: the smaller is reported, and nothing is written
    t, b, m = broken(longer=(200, 77))
    s2 = np.concatenate([[0], np.cumsum([len(x) + (r in (200, 77)) for r, x in enumerate(recs)])])
    for flags in (F, F | G):
        res = engine(ctx, b, m, len(t), cf, flags, True)
        tot = res[2]
        assert res[0] == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (3, BASE + 77, s2[77], n, 1) and nothing(res)
    with pytest.raises(trim_ref.Fault) as e:
        trim_ref.trim_text(t, cf)
    assert (e.value.kind, e.value.record) == (3, 77)
    # with a first-byte fault at a later, an earlier and the same record
    for at, want in ((150, (3, BASE + 77)), (30, (1, BASE + 30)), (77, (1, BASE + 77))):
        t, b, m = broken(longer=(77,), first=(at,))
        tot = engine(ctx, b, m, len(t), cf, F | G, True)[2]
        assert (tot.bad, tot.bad_record, tot.bad_src) == want + (starts[want[1] - BASE],), at
        with pytest.raises(trim_ref.Fault) as e:
            trim_ref.trim_text(t, cf)
        assert (e.value.kind, BASE + e.value.record) == want
    # without a qual_line the lengths are not compared
    t, b, m = broken(longer=(77,))
    assert engine(ctx, b, m, len(t), trim_ref.conf(qual_line=None), F)[2].bad == 0
    # a drop mask shorter than the text: drop_short, and nothing is written; the records beyond it count as dropped
    want = trim_ref.trim_text(text, cf, [0] * (n - 1))
    res = engine(ctx, blob, members, len(text), cf, F | G, True, [0] * (n - 1))
    tot = res[2]
    assert res[0] == 0 and (tot.drop_short, tot.bad, tot.seen, tot.dropped, tot.kept, tot.too_short) == (1, 0, n, 1, want.totals["kept"], want.totals["too_short"])
    assert nothing(res) and want.totals["drop_short"] == 1
    res = engine(ctx, blob, members, len(text), cf, F, False, [])
    assert (res[2].drop_short, res[2].dropped, res[2].kept) == (1, n, 0) and nothing(res)
    # a mask longer than the text is no fault: the entries behind the records are not read
    want = trim_ref.trim_text(text, cf, [r % 2 for r in range(n)])
    check(engine(ctx, blob, members, len(text), cf, F | G, True, [r % 2 for r in range(n + 5)]), want, text, cf, True)
    # capacities one too small, for trim rows, for rows and for bytes: BUF_ERROR, valid totals, buffers untouched
    want = trim_ref.trim_text(text, cf)
    rows_n = want.totals["kept"] + want.totals["too_short"]
    nbytes = sum(map(len, want.kept_bytes + want.short_bytes))
    for caps in ((n - 1, rows_n, nbytes), (n, rows_n - 1, nbytes), (n, rows_n, nbytes - 1)):
        res = engine(ctx, blob, members, len(text), cf, F | G, True, caps=caps)
        tot = res[2]
        assert res[0] == _lib.BUF_ERROR and (tot.seen, tot.kept, tot.too_short, tot.bytes, tot.covered, tot.bad) == (n, want.totals["kept"], want.totals["too_short"], nbytes, 1, 0), caps
        assert list(tot.adapter_records)[:3] == want.totals["adapter_records"] and nothing(res), caps
    check(engine(ctx, blob, members, len(text), cf, F | G, True, caps=(n, rows_n, nbytes)), want, text, cf, True)
    for bad in (dict(flags=1), dict(flags=2), dict(flags=8)):
        with pytest.raises(_lib.EngineError):
            engine(ctx, blob, members, len(text), cf, bad["flags"])


def test_device_form(ctx):
    from zlib_ng_amd import _lib, devmem
    n = 300
    recs, text, blob, members = text_of(n)
    nb = len(text)
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    cf = trim_ref.conf(first_byte=b"@", quality=(20, 20), adapters=ADAPTERS, mismatches=2, min_length=20)
    drop = np.array([r % 4 == 1 for r in range(n)], np.uint8)
    want = trim_ref.trim_text(text, cf, drop.tolist())
    code, status, tot_h, trim_h, rows_h, packed_h = engine(ctx, blob, members, nb, cf, F | G, True, drop)
    check((code, status, tot_h, trim_h, rows_h, packed_h), want, text, cf, True)
    kept, kb = len(rows_h), len(packed_h)
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    d_drop = devmem.from_host(ctx, drop.tobytes())
    canary = lambda size: devmem.from_host(ctx, b"\xa5" * size)
    d_trim, d_rows, d_out = canary(12 * n), canary(24 * kept), canary(kb)
    ads, table = _lib.grep_pattern_table(cf.adapters)

    def dev(flags, tcap, rcap, ocap, n_drop=n):
        return ctx.bgzf_trim_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, nb, ads, table, 10, flags, conf_of(cf, True), BASE, d_scratch.ptr, nb,
                                         d_st.ptr, d_drop.ptr, n_drop, d_trim.ptr if tcap else 0, tcap, d_rows.ptr if rcap else 0, rcap,
                                         d_out.ptr if ocap else 0, ocap)

    def untouched(trim_too=True):
        return ((not trim_too or d_trim.cpu().tobytes() == b"\xa5" * (12 * n)) and d_rows.cpu().tobytes() == b"\xa5" * (24 * kept) and
                d_out.cpu().tobytes() == b"\xa5" * kb)

    for caps in ((n - 1, kept, kb), (n, kept - 1, kb), (n, kept, kb - 1)):     # each capacity one too small
        code, tot = dev(F | G, *caps)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.bytes, tot.kept, tot.dropped, tot.covered, tot.bad) == (n, kb, tot_h.kept, tot_h.dropped, 1, 0), caps
        assert untouched(), caps
    code, tot = dev(F | G, n, kept, kb, n_drop=n - 1)
    assert code == 0 and (tot.drop_short, tot.seen) == (1, n) and untouched()
    # without _GROUP: the trim rows and the totals alone, rows and bytes may be NULL
    code, tot = dev(F, n, 0, 0)
    assert code == 0 and (tot.seen, tot.kept, tot.bytes) == (n, tot_h.kept, kb) and untouched(False)
    assert d_trim.cpu(_lib.TRIM_ROW_DTYPE).tobytes() == trim_h.tobytes()
    # exact capacities
    code, tot = dev(F | G, n, kept, kb)
    assert code == 0 and bytes(tot) == bytes(tot_h)
    assert d_trim.cpu(_lib.TRIM_ROW_DTYPE).tobytes() == trim_h.tobytes() and d_rows.cpu(_lib.GREP_ROW_DTYPE).tobytes() == rows_h.tobytes()
    assert d_out.cpu().tobytes() == bytes(packed_h)


def unzipped(path):
    from zlib_ng_amd import bgzf
    blob = open(path, "rb").read()
    assert blob.endswith(bgzf.EOF_BLOCK), path
    return gzip.decompress(blob)


def same(result, want):
    assert result.records == len(want.begin) and result.begin.tolist() == want.begin and result.end.tolist() == want.end
    assert result.adapter.tolist() == want.adapter and result.verdict.tolist() == want.verdict and result.steps.tolist() == want.steps
    for name in ("kept", "too_short", "dropped", "bases_in", "bases_out", "quality_trimmed", "adapter_trimmed"):
        assert getattr(result, name) == want.totals[name], name
    assert result.adapter_counts.tolist() == want.totals["adapter_records"]


KW = dict(quality=(20, 20), adapters=ADAPTERS, mismatches=2, min_length=20, first_byte=b"@")


def test_file_with_small_read_windows(ctx, tmp_path, monkeypatch):
    """records straddle windows; the outputs, read back with the gzip module, are the referee's bytes, the result its arrays"""
    from zlib_ng_amd import bgzf
    n = 1500
    text = b"".join(fastq(gen_reads(n, 11)))
    src = str(tmp_path / "reads.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)
    drop = np.arange(n) % 5 == 2
    want = trim_ref.trim_text(text, trim_ref.conf(**KW), drop.tolist())
    kept, short = str(tmp_path / "kept.gz"), str(tmp_path / "short.gz")
    ctx.bgzf_stats()
    res = bgzf.trim_records(src, kept, too_short=short, drop=drop, compresslevel=1, **KW)
    assert ctx.bgzf_stats()[0] >= 3                                                # (several windows)
    same(res, want)
    assert unzipped(kept) == b"".join(want.kept_bytes) and unzipped(short) == b"".join(want.short_bytes)
    with bgzf.open(src) as r:                                                      # a reader's method; output=None only counts
        same(r.trim_records(None, drop=drop, **KW), want)
    with pytest.raises(ValueError, match=r"the file holds 1500 records and drop has 1499 entries: the files are out of step"):
        bgzf.trim_records(src, None, drop=drop[:-1], **KW)
    # bodies of different length mid-file: the record, its virtual offset, both lengths
    lines = text.split(b"\n")
    lines[4 * 900 + 3] += b"FF"
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bgzf.compress(b"\n".join(lines), block_size=5000))
    n_seq = len(lines[4 * 900 + 1])
    with pytest.raises(ValueError, match=r"record 900 at virtual offset \d+: line 1 \(the sequence\) has %d bytes and line 3 \(the qualities\) has %d.*incomplete" % (n_seq, n_seq + 2)):
        bgzf.trim_records(bad, kept, **KW)
    assert 0 < len(unzipped(kept)) < len(b"".join(want.kept_bytes))


def test_paired_recipe(ctx, tmp_path):
    """two count-only passes, the OR of the too-short masks, two passes with drop=: both outputs keep the same records"""
    from zlib_ng_amd import bgzf
    n = 600
    paths, texts = [], []
    for mate, seed in ((1, 21), (2, 22)):
        texts.append(b"".join(b"%s/%d\n%s\n+\n%s\n" % (name, mate, s, q) for name, s, q in gen_reads(n, seed)))
        paths.append(str(tmp_path / ("r%d.fq.gz" % mate)))
        open(paths[-1], "wb").write(bgzf.compress(texts[-1], block_size=4099))
    first = [bgzf.trim_records(p, None, **KW) for p in paths]
    drop = (first[0].verdict == bgzf.TOO_SHORT) | (first[1].verdict == bgzf.TOO_SHORT)
    assert 50 < int(drop.sum()) < n - 50 and int((first[0].verdict == 1).sum()) < int(drop.sum())
    names = []
    for mate in range(2):
        out = str(tmp_path / ("t%d.fq.gz" % mate))
        res = bgzf.trim_records(paths[mate], out, drop=drop, compresslevel=1, **KW)
        assert (res.kept, res.too_short, res.dropped) == (n - int(drop.sum()), 0, int(drop.sum()))
        got = unzipped(out)
        assert got == b"".join(trim_ref.trim_text(texts[mate], trim_ref.conf(**KW), drop.tolist()).kept_bytes)
        names.append([x.split(b"/")[0] for x in got.split(b"\n")[0::4] if x])
    assert names[0] == names[1] == [b"@r%d" % r for r in np.nonzero(~drop)[0].tolist()]


def test_golden_file(ctx, tmp_path):
    from zlib_ng_amd import bgzf
    blob = open(BGZIP, "rb").read()
    data = gzip.decompress(blob)
    out = str(tmp_path / "same.gz")
    res = bgzf.trim_records(BGZIP, out, first_byte=b"@", compresslevel=1)
    assert unzipped(out) == data and res.records == res.kept == data.count(b"\n") // 4 and res.bases_in == res.bases_out and not res.steps.any()
    # one real adapter configuration on the first 1200 records: an adapter cut from a read's middle beside Illumina's, quality 30, one mismatch
    lines = data.split(b"\n")
    nrec = 1200
    part = b"\n".join(lines[:4 * nrec]) + b"\n"
    tab, _ = block_map(blob)
    us = np.array([u for c, u, cs, isz in tab])
    b = int(np.searchsorted(us, len(part), "right")) - 1
    stop = bgzf.make_virtual_offset(tab[b][0], len(part) - tab[b][1])
    kw = dict(quality=(0, 30), adapters=[b"AGATCGGAAGAGC", lines[4 * 5 + 1][100:113]], mismatches=1, min_length=140, first_byte=b"@")
    want = trim_ref.trim_text(part, trim_ref.conf(**kw))
    assert want.totals["adapter_records"][1] >= 1 and want.totals["quality_trimmed"] > 1000 and want.totals["too_short"] > 0
    short = str(tmp_path / "short.gz")
    res = bgzf.trim_records(BGZIP, out, too_short=short, stop=stop, compresslevel=1, **kw)
    same(res, want)
    assert unzipped(out) == b"".join(want.kept_bytes) and unzipped(short) == b"".join(want.short_bytes)

"""BGZF overlap (bgzf.overlap_records; csrc/za_overlap.hip).  The referee is overlap_ref.py: plain Python with the serial loops of the rule
as include/zng_amd.h states it, never the code under test.  Every comparison is byte for byte."""
import functools
import gzip
import random

import numpy as np
import pytest

import overlap_ref
from test_gpu_bgzf_lines import BGZIP
from test_gpu_bgzf_trim import packed_of, unzipped

pytestmark = pytest.mark.gpu

ADAPTERS = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")      # what reads through the fragment's end into mate 1 / mate 2
BASE = 700                                                   # record_base of the calls through the C ABI
EDGES = [0, 1, 29, 30, 31, 63, 64, 65, 100, 127, 128, 129, 150]


def gen_pairs(n, seed):
    """-> [(name, mate 1, its qualities, mate 2, its qualities, planted)]: both mates cut from a random fragment of `ins` bases, mate 1 =
    (fragment + adapter)[:n1], mate 2 = (revcomp(fragment) + adapter)[:n2]; n1 and n2 from EDGES or random in [20, 160), ins from 1 to
    n1 + n2 + 20; a quarter of the pairs unrelated; a third with 0 to 7 substitutions in mate 1's part of the overlap, half of them with
    a low quality; qualities from FFFFF:,#.  planted: the offset the fragment gives (None for an unrelated pair)"""
    rng = random.Random(seed)
    bases = lambda k: bytes(rng.choice(b"ACGT") for _ in range(k))
    out = []
    for i in range(n):
        n1, n2 = (rng.choice(EDGES) if rng.random() < 0.25 else rng.randrange(20, 160) for _ in range(2))
        ins = rng.randrange(1, n1 + n2 + 21)
        frag = bases(ins)
        m1 = bytearray((frag + ADAPTERS[0] + bases(160))[:n1])
        m2 = bytearray((overlap_ref.revcomp(frag) + ADAPTERS[1] + bases(160))[:n2])
        q1, q2 = (bytearray(rng.choice(b"FFFFF:,#") for _ in range(k)) for k in (n1, n2))
        planted = ins - n2
        if i % 4 == 3:
            m2, planted = bytearray(bases(n2)), None
        elif i % 3 == 0:
            lo, hi = max(0, planted), min(n1, ins)
            for at in rng.sample(range(lo, hi), min(rng.randrange(0, 8), max(0, hi - lo))):
                m1[at] = rng.choice([c for c in b"ACGT" if c != m1[at]])
                if rng.random() < 0.5:
                    q1[at] = rng.choice(b"#,")
        out.append((b"@p%d" % i, bytes(m1), bytes(q1), bytes(m2), bytes(q2), planted))
    return out


def interleaved(pairs):
    return [b"%s/1\n%s\n+\n%s\n%s/2\n%s\n+\n%s\n" % (p[0], p[1], p[2], p[0], p[3], p[4]) for p in pairs]


@functools.lru_cache(maxsize=None)
def raw_of(n):
    recs = interleaved(gen_pairs(n, 5))
    return recs, b"".join(recs)


@functools.lru_cache(maxsize=None)
def text_of(n):
    """-> (records, text, BGZF blob, member table) of n generated pairs: computed once per n, never changed"""
    return raw_of(n) + packed_of(raw_of(n)[1])


# name -> (the rule's arguments, class 1 is gathered).  "merge" has the strict limit: of the pairs with 0 to 7 substitutions those with 3 and
# more lie above it, while under the default of 5 most of them lie below.
CONFIGS = {
    "search only": (dict(merge=False), True),
    "merge": (dict(mismatches=2), False),
    "merge+unmerged": (dict(), True),
    "correct+cut without merge": (dict(merge=False, correct=True, cut=True), True),
    "everything": (dict(correct=True, cut=True), True),
}


@functools.lru_cache(maxsize=None)
def referee(n, name):
    return overlap_ref.overlap_text(raw_of(n)[1], overlap_ref.conf(first_byte=b"@", **CONFIGS[name][0]))


def conf_of(cf, keep=False):
    from zlib_ng_amd import _lib
    flags = ((_lib.BGZF_OVERLAP_MERGE if cf.merge else 0) | (_lib.BGZF_OVERLAP_CORRECT if cf.correct else 0) | (_lib.BGZF_OVERLAP_CUT if cf.cut else 0) |
             (_lib.BGZF_OVERLAP_KEEP_UNMERGED if keep else 0))
    return _lib.BgzfOverlapConf(cf.record_lines, cf.seq_line, cf.qual_line, -1 if cf.first_byte is None else cf.first_byte[0], cf.quality_base, cf.min_overlap,
                                cf.mismatches, cf.percent, cf.q_high, cf.q_low, flags)


def engine(ctx, blob, members, nbytes, cf, flags, keep=False, caps=None):
    return ctx.bgzf_overlap_records(blob, members, 0, nbytes, cf.delimiter[0], flags, conf_of(cf, keep), BASE, caps)


TOTALS = ("none", "found", "merged", "too_long", "bytes_in", "bases_in", "bases_merged", "corrected", "corrected_pairs", "adapter_pairs", "adapter_trimmed",
          "overlap_sum", "mismatch_sum")


def check(res, want, text, cf, keep, group=True, final=True, what=None):
    """every overlap row, every total, the rows by class then number with the new lengths, the bytes per class"""
    code, status, tot, ovl, rows, packed = res
    t = want.totals
    n = t["seen"]
    assert code == 0 and not status.any(), what
    assert (tot.covered, tot.bad, tot.seen, tot.reserved) == (1, 0, n, 0), what
    for name in ("offset", "insert", "overlap", "mismatches", "corrected", "verdict", "steps"):
        assert ovl[name].tolist() == getattr(want, name), (what, name)
    for name in TOTALS:
        assert getattr(tot, name) == t[name], (what, name)
    pieces = want.merged_bytes + (want.other_bytes if keep else [])
    assert tot.bytes == sum(map(len, pieces)), what
    if not group:
        assert len(rows) == 0 and packed == b"", what
        return
    v = np.array(want.verdict, np.int64)
    order = np.concatenate([np.nonzero(v == 2)[0], np.nonzero(v != 2)[0] if keep else np.empty(0, np.int64)])
    starts = np.array(overlap_ref.split_records(text, cf.record_lines, cf.delimiter, final)[1], np.int64)
    assert rows["number"].tolist() == (BASE + order).tolist() and rows["src_off"].tolist() == starts[order].tolist(), what
    assert rows["len"].tolist() == [len(x) for x in pieces] and rows["reserved"].tolist() == (v[order] != 2).astype(int).tolist(), what
    assert bytes(packed) == b"".join(pieces), what


def test_inputs_cross_every_edge():
    """what the grid relies on, asserted of the referee's result for n = 773"""
    pairs = gen_pairs(773, 5)
    want = referee(773, "everything")
    off, found = np.array(want.offset), np.array(want.verdict) == overlap_ref.MERGED
    assert int((found & (off < 0)).sum()) >= 50 and int((found & (off >= 0)).sum()) >= 50
    assert int((found & (np.array(want.mismatches) >= 1)).sum()) >= 50
    assert want.totals["corrected"] >= 50 and want.totals["none"] >= 100 and want.totals["adapter_pairs"] >= 50
    strict, cf = referee(773, "merge"), overlap_ref.conf(**CONFIGS["merge"][0])
    above = planted = 0
    for r, (_, a, _, y, _, o) in enumerate(pairs):
        if o is None:
            continue
        lo, hi = max(0, o), min(len(a), o + len(y))
        b = overlap_ref.revcomp(y)
        d = sum(1 for i in range(lo, hi) if a[i] != b[i - o])
        if hi - lo >= cf.min_overlap:
            over = d > min(cf.mismatches, (hi - lo) * cf.percent // 100)
            above += over
            assert not over or strict.offset[r] != o or strict.verdict[r] != overlap_ref.MERGED
            planted += found[r] and want.offset[r] == o
    assert above >= 50 and planted >= 200                        # d above the (strict) limit; the found insert is the planted one
    assert found.sum() == planted                                # every found insert is the planted one
    assert {len(p[1]) for p in pairs} >= set(EDGES) and {len(p[3]) for p in pairs} >= set(EDGES)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 773])
def test_grid(ctx, n):
    from zlib_ng_amd import _lib
    recs, text, blob, members = text_of(n)
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    for name, (kw, keep) in CONFIGS.items():
        want = referee(n, name)
        cf = overlap_ref.conf(first_byte=b"@", **kw)
        res = engine(ctx, blob, members, len(text), cf, F | G, keep)
        check(res, want, text, cf, keep, what=(n, name))
        if name == "search only":                              # the bytes are the input, the rows those of partition_records with one class
            assert bytes(res[5]) == text
            part = ctx.bgzf_partition_records(blob, members, 0, len(text), 10, F | G, 8, ord("@"), BASE, np.zeros(n, np.uint16), 1)
            for field in ("src_off", "number", "len"):         # (reserved is the class: 1 here, 0 there)
                assert res[4][field].tolist() == part[5][field].tolist()
            assert bytes(part[6]) == text
        # without _GROUP: the same rows and totals, and nothing else
        check(engine(ctx, blob, members, len(text), cf, F, keep), want, text, cf, keep, group=False, what=(n, name))


def run(ctx, text, keep=True, final=True, **kw):
    """one small text through the engine and the referee"""
    from zlib_ng_amd import _lib
    cf = overlap_ref.conf(**kw)
    blob, members = packed_of(text, 4099)
    want = overlap_ref.overlap_text(text, cf, final)
    res = engine(ctx, blob, members, len(text), cf, (_lib.BGZF_GREP_FINAL if final else 0) | _lib.BGZF_CLASSIFY_GROUP, keep)
    check(res, want, text, cf, keep, final=final, what=kw)
    return want


def fq(pairs):
    """[(mate 1, mate 2)] -> interleaved FASTQ with F qualities"""
    return b"".join(b"@e%d/1\n%s\n+\n%s\n@e%d/2\n%s\n+\n%s\n" % (i, a, b"F" * len(a), i, y, b"F" * len(y)) for i, (a, y) in enumerate(pairs))


def test_edges(ctx):
    rng = random.Random(3)
    bases = lambda k: bytes(rng.choice(b"ACGT") for _ in range(k))
    rc = overlap_ref.revcomp
    # the worst case: two homopolymers of 1024 bases, every offset a match or none
    for kw in (dict(), dict(min_overlap=1, mismatches=1024, percent=100), dict(min_overlap=1024), dict(merge=False, cut=True)):
        want = run(ctx, fq([(b"A" * 1024, b"T" * 1024), (b"A" * 1024, b"A" * 1024), (b"A" * 1024, b"T" * 700), (b"A" * 3, b"T" * 1024)]), **kw)
        assert (want.offset[0], want.overlap[0]) == (0, 1024) and (want.verdict[1] == 0) == (kw.get("mismatches") != 1024)
    # 1023, 1024 and 1025 bases: a mate of 1025 is not searched and is written whole
    f = bases(1025)
    want = run(ctx, fq([(f[:n], rc(f[:n])) for n in (1023, 1024, 1025)] + [(f[:100], rc(f)), (f, rc(f)[:100])]), correct=True, cut=True)
    assert want.verdict == [2, 2, 3, 3, 3] and want.overlap[:2] == [1023, 1024]
    want = run(ctx, fq([(f[:1024], rc(f[:1000]) + b"ACGT" * 6), (f[30:1024] + b"ACGT" * 7, rc(f[:1024]))]), merge=False, cut=True)
    assert want.offset == [-24, -30] and want.steps == [3, 3]
    # an overlap that starts at byte 60 and 63 of a dword stage, in the first and the third 64-byte strip; both ways round
    pairs = []
    for at in (60, 63, 64, 128 + 60, 128 + 63):
        f = bases(at + 45)
        pairs += [(f, rc(f[at:])), (f[at:], rc(f)), (f[:at + 40], rc(f[at:])), (f[at:], rc(f[:at + 40]))]
    want = run(ctx, fq(pairs))
    assert want.offset[:4] == [60, -60, 60, -60] and want.offset[16:] == [191, -191, 191, -191] and want.verdict == [2] * 20
    run(ctx, fq(pairs), merge=False, correct=True, cut=True)
    # every tie-break as a real pair: a dinucleotide repeat, equal L and d at +-o, d against L
    want = run(ctx, fq([(b"AC" * 30, rc(b"AC" * 30)), (b"AC" * 30 + b"G", b"T" + rc(b"AC" * 30)), (b"ACGT" * 12, rc(b"ACGT" * 12))]), min_overlap=10)
    assert want.offset[0] == 0
    # FASTA pairs (no qualities: mate 1 wins every tie) and 16-line records; another delimiter; the qualities in front of the sequence
    f = bases(120)
    fa = b"".join(b">a%d/1\n%s\n>a%d/2\n%s\n" % (i, f[:80 - i], i, rc(f[20 + i:110])) for i in range(5))
    want = run(ctx, fa, record_lines=4, qual_line=None)
    assert want.verdict == [2] * 5 and want.merged_bytes[0] == b">a0/1\n%s\n" % f[:110]
    run(ctx, fa, record_lines=4, qual_line=None, merge=False, cut=True)
    wide = b"".join(b"@w/1\nx\ny\n%s\nz\n%s\nu\nv\n@w/2\nx\ny\n%s\nz\n%s\nu\nv\n" % (f[:90], b"F" * 90, rc(f[30:])[:85], b":" * 85) for _ in range(3))
    run(ctx, wide, record_lines=16, seq_line=3, qual_line=5, correct=True, cut=True)
    run(ctx, wide, record_lines=16, seq_line=3, qual_line=5, merge=False, correct=True, cut=True)
    run(ctx, fq([(f[:80], rc(f[20:]))] * 2).replace(b"\n", b";"), delimiter=b";", first_byte=b"@")
    swapped = b"".join(b"@s/1\n%s\n+\n%s\n@s/2\n%s\n+\n%s\n" % (b"F,F#" * 20, f[:80], b"#F:," * 25, rc(f[20:])) for _ in range(2))
    run(ctx, swapped, seq_line=3, qual_line=1, correct=True)
    # N and lowercase bytes, a U; CR line ends (a CR is a body byte)
    g = bytearray(f[:100])
    g[10], g[20], g[30] = ord("N"), ord("a"), ord("U")
    run(ctx, fq([(bytes(g), rc(bytes(g))), (bytes(g), rc(f[:100]))]), correct=True)
    run(ctx, fq([(f[:80], rc(f[20:]))] * 2).replace(b"\n", b"\r\n"), min_overlap=20)
    # an empty mate; a short last pair; the open tail without _FINAL
    run(ctx, fq([(b"", f[:50]), (f[:50], b""), (b"", b""), (f[:50], rc(f[:50]))]))
    rec = fq([(f[:80], rc(f[20:]))])
    want = run(ctx, rec + b"@s/1\nACGT\n+\nFFFF\n@s/2\n", first_byte=b"@")
    assert want.verdict == [2, 0] and want.other_bytes == [b"@s/1\nACGT\n+\nFFFF\n@s/2\n"]
    from zlib_ng_amd import _lib
    text = rec + b"@s/1\nACGT\n+\nFFFF\n@s/2\nAC"
    blob, members = packed_of(text)
    res = engine(ctx, blob, members, len(text), overlap_ref.conf(), _lib.BGZF_CLASSIFY_GROUP, True)
    assert (res[2].seen, res[2].tail_off, res[2].short_lines, res[2].bad, res[2].merged) == (1, len(rec), 0, 0, 1)
    assert bytes(res[5]) == b"@e0/1\n%s\n+\n%s\n" % (f, b"F" * 120)


def test_faults(ctx):
    from zlib_ng_amd import _lib
    n = 300
    recs, text, blob, members = text_of(n)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    cf = overlap_ref.conf(first_byte=b"@", correct=True, cut=True)
    nothing = lambda res: len(res[3]) == 0 and len(res[4]) == 0 and res[5] == b""

    def broken(longer=(), first=()):
        """the text with a byte more in the qualities of mate 2 (even r) or mate 1 (odd r) of the records `longer`, and '#' as the first
        byte of mate 2 (even r) or mate 1 (odd r) of the records `first`"""
        out = []
        for r, rec in enumerate(recs):
            lines = rec.split(b"\n")
            if r in longer:
                lines[7 if r % 2 == 0 else 3] += b"F"
            if r in first:
                at = 4 if r % 2 == 0 else 0
                lines[at] = b"#" + lines[at][1:]
            out.append(b"\n".join(lines))
        t = b"".join(out)
        return (t,) + packed_of(t)

    # bodies of different length at two records: the smaller is reported, and nothing is written
    t, b, m = broken(longer=(200, 77))
    s2 = np.concatenate([[0], np.cumsum([len(x) + (r in (200, 77)) for r, x in enumerate(recs)])])
    for flags in (F, F | G):
        res = engine(ctx, b, m, len(t), cf, flags, True)
        tot = res[2]
        assert res[0] == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (3, BASE + 77, s2[77], n, 1) and nothing(res)
    with pytest.raises(overlap_ref.Fault) as e:
        overlap_ref.overlap_text(t, cf)
    assert (e.value.kind, e.value.record) == (3, 77)
    # with a first-byte fault at a later, an earlier and the same record; in either mate
    for at, want in ((150, (3, BASE + 77)), (30, (1, BASE + 30)), (31, (1, BASE + 31)), (77, (1, BASE + 77))):
        t, b, m = broken(longer=(77,), first=(at,))
        tot = engine(ctx, b, m, len(t), cf, F | G, True)[2]
        assert (tot.bad, tot.bad_record, tot.bad_src) == want + (starts[want[1] - BASE],), at
        with pytest.raises(overlap_ref.Fault) as e:
            overlap_ref.overlap_text(t, cf)
        assert (e.value.kind, BASE + e.value.record) == want
    # without a qual_line the lengths are not compared
    t, b, m = broken(longer=(77, 200))
    assert engine(ctx, b, m, len(t), overlap_ref.conf(qual_line=None), F)[2].bad == 0
    # capacities one too small, for overlap rows, for rows and for bytes: BUF_ERROR, valid totals, buffers untouched
    want = overlap_ref.overlap_text(text, cf)
    nbytes = sum(map(len, want.merged_bytes + want.other_bytes))
    for caps in ((n - 1, n, nbytes), (n, n - 1, nbytes), (n, n, nbytes - 1)):
        res = engine(ctx, blob, members, len(text), cf, F | G, True, caps=caps)
        tot = res[2]
        assert res[0] == _lib.BUF_ERROR and (tot.seen, tot.merged, tot.none, tot.bytes, tot.covered, tot.bad) == (n, want.totals["merged"], want.totals["none"], nbytes, 1, 0), caps
        assert tot.corrected == want.totals["corrected"] and nothing(res), caps
    check(engine(ctx, blob, members, len(text), cf, F | G, True, caps=(n, n, nbytes)), want, text, cf, True)
    for flags in (1, 2, 8):
        with pytest.raises(_lib.EngineError):
            engine(ctx, blob, members, len(text), cf, flags)


def test_device_form(ctx):
    from zlib_ng_amd import _lib, devmem
    n = 300
    recs, text, blob, members = text_of(n)
    nb = len(text)
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    cf = overlap_ref.conf(first_byte=b"@", correct=True, cut=True)
    want = overlap_ref.overlap_text(text, cf)
    code, status, tot_h, ovl_h, rows_h, packed_h = engine(ctx, blob, members, nb, cf, F | G, True)
    check((code, status, tot_h, ovl_h, rows_h, packed_h), want, text, cf, True)
    kept, kb = len(rows_h), len(packed_h)
    assert kept == n
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    canary = lambda size: devmem.from_host(ctx, b"\xa5" * size)
    d_ovl, d_rows, d_out = canary(16 * n), canary(24 * kept), canary(kb)

    def dev(flags, vcap, rcap, ocap):
        return ctx.bgzf_overlap_records_dev(d_in.ptr, len(blob), d_m.ptr, len(members), 0, nb, 10, flags, conf_of(cf, True), BASE, d_scratch.ptr, nb, d_st.ptr,
                                            d_ovl.ptr if vcap else 0, vcap, d_rows.ptr if rcap else 0, rcap, d_out.ptr if ocap else 0, ocap)

    def untouched(ovl_too=True):
        return ((not ovl_too or d_ovl.cpu().tobytes() == b"\xa5" * (16 * n)) and d_rows.cpu().tobytes() == b"\xa5" * (24 * kept) and
                d_out.cpu().tobytes() == b"\xa5" * kb)

    for caps in ((n - 1, kept, kb), (n, kept - 1, kb), (n, kept, kb - 1)):     # each capacity one too small
        code, tot = dev(F | G, *caps)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.bytes, tot.merged, tot.covered, tot.bad) == (n, kb, tot_h.merged, 1, 0), caps
        assert untouched(), caps
    # without _GROUP: the overlap rows and the totals alone, rows and bytes may be NULL
    code, tot = dev(F, n, 0, 0)
    assert code == 0 and (tot.seen, tot.merged, tot.bytes) == (n, tot_h.merged, kb) and untouched(False)
    assert d_ovl.cpu(_lib.OVERLAP_ROW_DTYPE).tobytes() == ovl_h.tobytes()
    # exact capacities
    code, tot = dev(F | G, n, kept, kb)
    assert code == 0 and bytes(tot) == bytes(tot_h)
    assert d_ovl.cpu(_lib.OVERLAP_ROW_DTYPE).tobytes() == ovl_h.tobytes() and d_rows.cpu(_lib.GREP_ROW_DTYPE).tobytes() == rows_h.tobytes()
    assert d_out.cpu().tobytes() == bytes(packed_h)


def same(result, want):
    from zlib_ng_amd import bgzf
    assert result.records == len(want.offset) == len(result)
    for name, got in (("offset", result.offset), ("insert", result.insert), ("overlap", result.overlap), ("mismatches", result.mismatches),
                      ("corrected", result.corrected_per_pair), ("verdict", result.verdict), ("steps", result.steps)):
        assert got.tolist() == getattr(want, name), name
    for name in TOTALS:
        if name != "bytes_in":
            assert getattr(result, name) == want.totals[name], name
    assert result.insert_sizes().tolist() == np.bincount(np.array(want.insert, np.int64)).tolist()
    found = want.totals["found"] + want.totals["merged"]
    assert result.mean_overlap == (want.totals["overlap_sum"] / found if found else 0.0)
    assert (bgzf.NONE, bgzf.FOUND, bgzf.MERGED, bgzf.TOO_LONG) == (0, 1, 2, 3) and "OverlapResult" in repr(result)


def test_file_with_small_read_windows(ctx, tmp_path, monkeypatch):
    """pairs straddle windows; the outputs, read back with the gzip module, are the referee's bytes, the result its arrays"""
    from zlib_ng_amd import bgzf
    n = 1500
    text = b"".join(interleaved(gen_pairs(n, 11)))
    src = str(tmp_path / "pairs.fq.gz")
    open(src, "wb").write(bgzf.compress(text, block_size=5000))
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 20000)
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 6000)               # (what is read behind a window: a block of 5000 bytes is smaller)
    kw = dict(correct=True, cut=True, first_byte=b"@")
    want = overlap_ref.overlap_text(text, overlap_ref.conf(**kw))
    merged, other = str(tmp_path / "merged.gz"), str(tmp_path / "other.gz")
    ctx.bgzf_stats()
    res = bgzf.overlap_records(src, merged, other, correct=True, cut_adapters=True, first_byte=b"@", compresslevel=1)
    assert ctx.bgzf_stats()[0] >= 3                                                # (several windows)
    same(res, want)
    assert unzipped(merged) == b"".join(want.merged_bytes) and unzipped(other) == b"".join(want.other_bytes)
    with bgzf.open(src) as r:                                                      # a reader's method; no output only counts
        same(r.overlap_records(correct=True, cut_adapters=True, first_byte=b"@"), want)
        res = r.overlap_records(merged, correct=True, cut_adapters=True, first_byte=b"@", compresslevel=1)      # one output: the others are counted only
    same(res, want)
    assert unzipped(merged) == b"".join(want.merged_bytes)
    # bodies of different length mid-file: the record, its virtual offset, the mate and both lengths
    lines = text.split(b"\n")
    lines[8 * 900 + 7] += b"FF"
    bad = str(tmp_path / "bad.fq.gz")
    open(bad, "wb").write(bgzf.compress(b"\n".join(lines), block_size=5000))
    n_seq = len(lines[8 * 900 + 5])
    with pytest.raises(ValueError, match=r"record 900 at virtual offset \d+: line 5 \(the sequence of mate 2\) has %d bytes and line 7 \(its qualities\) has %d.*incomplete" % (n_seq, n_seq + 2)):
        bgzf.overlap_records(bad, merged, first_byte=b"@")
    assert 0 < len(unzipped(merged)) < len(b"".join(want.merged_bytes))


def test_golden_pairs(ctx, tmp_path):
    """pairs made from the committed FASTQ: mate 1 a read's first 100 bases, mate 2 the reverse complement of its bases from 50 on with
    the qualities reversed; the merged output is the original reads' sequences.  Two of the 500 reads are short tandem repeats, in
    which a longer overlap with up to five mismatches exists: the rule takes the longest, as fastp does, and the referee says which"""
    from zlib_ng_amd import bgzf
    lines = gzip.decompress(open(BGZIP, "rb").read()).split(b"\n")
    nrec = 500
    reads = [(lines[4 * i], lines[4 * i + 1], lines[4 * i + 3]) for i in range(nrec)]
    assert min(len(s) for _, s, _ in reads) >= 130
    text = b"".join(b"%s/1\n%s\n+\n%s\n%s/2\n%s\n+\n%s\n" % (name, s[:100], q[:100], name, overlap_ref.revcomp(s[50:]), q[50:][::-1]) for name, s, q in reads)
    want = overlap_ref.overlap_text(text, overlap_ref.conf(first_byte=b"@"))
    plain = [i for i in range(nrec) if (want.offset[i], want.overlap[i], want.mismatches[i]) == (50, 50, 0)]
    assert len(plain) >= nrec - 5 and want.totals["merged"] == nrec
    src, out = str(tmp_path / "pairs.fq.gz"), str(tmp_path / "merged.gz")
    open(src, "wb").write(bgzf.compress(text))
    res = bgzf.overlap_records(src, out, first_byte=b"@", compresslevel=1)
    same(res, want)
    assert unzipped(out) == b"".join(want.merged_bytes)
    got = unzipped(out).split(b"\n")
    for i in plain:
        name, s, q = reads[i]
        assert got[4 * i:4 * i + 4] == [name + b"/1", s, b"+", q] and res.insert[i] == len(s)

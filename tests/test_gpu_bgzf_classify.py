"""BGZF by nearest pattern (bgzf.classify_records / demux; csrc/za_classify.hip).  The referee is classify_ref.py: numpy on the bytes
the system gzip decodes, never the code under test -- per pattern the mismatch count of every window, windows with a delimiter dropped
by a prefix sum, np.minimum.at per line, the minimum over the lines of a record that count, then the assignment rule."""
import gzip
import random

import numpy as np
import pytest

import classify_ref
from test_gpu_bgzf_grep import block_map
from test_gpu_bgzf_grep_approx import INPUTS, mutate
from test_gpu_bgzf_lines import BGZIP, inputs, member_table, referee_lines      # noqa: F401  (inputs: a fixture)

pytestmark = pytest.mark.gpu

WG = 256                                                     # ZA_CLS_WG_RECORDS: records per workgroup of the partition kernels
A, B = b"ACGTTGCAAGCTTCGA", b"TGCAACGTTCGAAGCT"             # two barcodes of 16 bases, 16 places apart


def agree(res, v, what=None, lo=0, hi=None):
    hi = len(v.pattern) if hi is None else hi
    assert res.searched == hi - lo and res.pattern.dtype == np.int16 and res.distance.dtype == np.uint8 and res.tie.shape == (hi - lo, 2), what
    assert np.array_equal(res.pattern, v.pattern[lo:hi]), what
    assert np.array_equal(res.distance, v.distance[lo:hi]), what
    assert np.array_equal(res.tie, v.tie[lo:hi]), what
    assert res.counts.tolist() == np.bincount(v.cls[lo:hi], minlength=len(v.counts)).tolist(), what


def pattern_set(rng, data, delim, k):
    """patterns cut from the data and mutated in 0, k, k + 1 and k places (anywhere, the first byte, the second, anywhere), no two the same"""
    bodies = [ln[:-1] if ln.endswith(delim) else ln for ln in referee_lines(data, delim)]
    bodies = [b for b in bodies if len(b) > k]
    if not bodies:
        return [bytes(b for b in b"\x02nowhere in the data at all\x03" if b != delim[0])]
    for _ in range(100):
        pats = []
        for m, where in ((0, "random"), (k, "first"), (k + 1, "second"), (k, "random")):
            b = rng.choice(bodies)
            L = rng.randrange(k + 1, max(k + 1, min(len(b), 40)) + 1)
            o = rng.randrange(len(b) - L + 1)
            pats.append(mutate(rng, b[o:o + L], min(m, L), delim, where))
        if len(set(pats)) == len(pats):
            return pats
    return pats[:1]


@pytest.mark.parametrize("name", INPUTS)
def test_against_the_referee(ctx, inputs, tmp_path, name):
    from zlib_ng_amd import bgzf
    rng = random.Random(100 + INPUTS.index(name))
    blob, delims = inputs[name]
    path = tmp_path / "t.bgzf"
    path.write_bytes(blob)
    data = gzip.decompress(blob)
    models = [(rl, ml) for rl in (1, 2, 4) for ml in (None, 0, 1) if ml is None or ml < rl]
    with bgzf.open(str(path)) as r:
        for delim in delims:
            for ki, k in enumerate((0, 1, 2, 16)):
                pats = pattern_set(rng, data, delim, k)
                assert min(len(p) for p in pats) > k
                ds = classify_ref.line_distances(data, delim, pats, k, both=True)
                for line_start in (False, True):
                    d = ds[line_start]
                    # every record model on the small inputs; on the large ones (megabytes: the referee's time) two per (k, line_start),
                    # chosen so that every model is met with either line_start
                    use = models if len(data) < 1 << 20 else [models[(2 * ki + line_start + j) % len(models)] for j in (0, 3)]
                    for rl, ml in use:
                        what = (name, delim, k, line_start, rl, ml, pats)
                        v = classify_ref.classify(data, delim, pats, k, rl, ml, line_start, d)
                        res = r.classify_records(pats, rl, match_line=ml, delimiter=delim, line_start=line_start, allow_short=True, mismatches=k)
                        agree(res, v, what)


def built(rng):
    """-> (text, {case: record number}): FASTQ-like records of four lines, about 40 KiB, that is three tiles of 16 KiB; the cases of the
    docstrings below planted at known records"""
    recs, at, where = [], 0, {}
    A1, B1 = mutate(rng, A, 1, b"\n"), mutate(rng, B, 1, b"\n")
    letters = b"ACGT"

    def seq(n):
        return bytes(rng.choice(letters) for _ in range(n))

    def add(lines, case=None):
        nonlocal at
        if case is not None:
            where[case] = len(recs)
        rec = b"".join(x + b"\n" for x in lines)
        recs.append(rec)
        at += len(rec)

    def filler():
        n = rng.randrange(20, 80)
        kind = len(recs) % 5
        s = seq(n)
        if kind == 0:
            s = A + s                                        # A itself
        elif kind == 1:
            s = mutate(rng, B, 2, b"\n") + s                 # B two places off
        add([b"@r%d" % len(recs), s, b"+", b"I" * len(s)])

    def until(edge):
        while at < edge - 500:
            filler()

    until(16384)
    head = b"@r%d tile" % len(recs)
    pad = 16383 - (at + len(head) + 1)                       # the bases line starts behind the header; A1 starts in the tile's last byte
    assert pad > 0
    s = b"N" * pad + A1 + seq(30)
    add([head, s, b"+", b"I" * len(s)], "tile")
    assert (at - len(recs[-1]) + len(head) + 1 + pad) == 16383
    s = seq(10) + A1 + seq(7) + B + seq(5)
    add([b"@r%d" % len(recs), s, b"+", b"I" * len(s)], "nearer")              # A at 1, B at 0 in one line: B, 0
    s = seq(9) + B1 + seq(3) + A1 + seq(11)
    add([b"@r%d" % len(recs), s, b"+", b"I" * len(s)], "tie")                 # both at 1 in one line: ambiguous, A .. B
    s = seq(40)
    add([b"@r%d " % len(recs) + A1, s, b"+" + B1, b"I" * len(s)], "lines")    # A at 1 in line 0, B at 1 in line 2
    add([b"@r%d" % len(recs), b"N" * 50, b"+", b"I" * 50], "none")
    until(32768)
    head = b"@r%d long" % len(recs)
    long255 = bytes(rng.choice(b"acgtn") for _ in range(255))
    pad = 32768 - 100 - (at + len(head) + 1)                 # 255 bytes that differ from long255 in 16 places, across the second tile edge
    assert pad > 0
    s = b"N" * pad + mutate(rng, long255, 16, b"\n") + seq(5)
    add([head, s, b"+", b"I" * len(s)], "long")
    s = seq(3) + mutate(rng, long255, 17, b"\n")
    add([b"@r%d" % len(recs), s, b"+", b"I" * len(s)], "long17")
    while at < 40000:
        filler()
    return b"".join(recs), where, long255


def test_built_text(ctx, tmp_path):
    from zlib_ng_amd import _lib, bgzf
    rng = random.Random(5)
    text, where, long255 = built(rng)
    nrec = text.count(b"\n") // 4
    assert 40000 <= len(text) < 3 * 16384 and text.count(b"\n") % 4 == 0
    starts = np.concatenate([[0], np.cumsum([len(x) for x in classify_ref.classify(text, b"\n", [A], 0, 4).records])])
    assert any(s // 16384 != (e - 1) // 16384 for s, e in zip(starts, starts[1:]))        # a record straddles a tile edge
    assert sum(s // 997 != (e - 1) // 997 for s, e in zip(starts, starts[1:])) > 30          # ... and many straddle a block edge
    path = tmp_path / "built.bgzf"
    path.write_bytes(bgzf.compress(text, block_size=997))
    assert gzip.decompress(path.read_bytes()) == text

    def run(pats, k, ml=1, **kw):
        v = classify_ref.classify(text, b"\n", pats, k, 4, ml, kw.get("line_start", False))
        res = bgzf.classify_records(str(path), pats, 4, match_line=ml, first_byte=b"@", mismatches=k, **kw)
        agree(res, v, (len(pats), k, ml, kw))
        return res, v

    # on the referee alone: the input holds every kind of verdict
    v = classify_ref.classify(text, b"\n", [A, B], 1, 4, 1)
    assert (v.pattern >= 0).any() and (v.pattern == classify_ref.AMBIGUOUS).any() and (v.pattern == classify_ref.UNASSIGNED).any()
    res, v = run([A, B], 1)
    t, n, tie, ln, none = (where[x] for x in ("tile", "nearer", "tie", "lines", "none"))
    assert (res.pattern[t], res.distance[t]) == (0, 1)                          # the window in the tile's last byte: compared in the overhang
    assert (res.pattern[n], res.distance[n], res.tie[n].tolist()) == (1, 0, [1, 1])
    assert (res.pattern[tie], res.distance[tie], res.tie[tie].tolist()) == (bgzf.AMBIGUOUS, 1, [0, 1])
    assert (res.pattern[ln], res.distance[ln]) == (bgzf.UNASSIGNED, 255) and res.pattern[none] == bgzf.UNASSIGNED
    res, v = run([A, B], 1, None)                                               # every line counts: line 0 has A, line 2 has B, both one off
    assert (res.pattern[ln], res.distance[ln], res.tie[ln].tolist()) == (bgzf.AMBIGUOUS, 1, [0, 1])
    res, v = run([A, B], 1, 0)
    assert (res.pattern[ln], res.distance[ln], res.tie[ln].tolist()) == (0, 1, [0, 0])
    res, v = run([B, A], 1)                                                     # the indices follow the pattern list
    assert (res.pattern[n], res.tie[tie].tolist()) == (0, [0, 1])
    res, v = run([A, B], 0)
    assert res.pattern[t] == bgzf.UNASSIGNED and res.pattern[n] == 1 and res.pattern[tie] == bgzf.UNASSIGNED
    run([A, B], 2, line_start=True)
    # a 255-byte pattern with k = 16, across a tile edge; one place more is none
    res, v = run([long255, A + B], 16)
    assert (res.pattern[where["long"]], res.distance[where["long"]]) == (0, 16) and res.pattern[where["long17"]] == bgzf.UNASSIGNED
    res, v = run([long255], 15)
    assert res.pattern[where["long"]] == bgzf.UNASSIGNED
    # 64 patterns
    many = [A, B]
    while len(many) < 64:
        p = bytes(rng.choice(b"ACGT") for _ in range(16))
        if p not in many:
            many.append(p)
    rng.shuffle(many)
    res, v = run(many, 2)
    assert res.counts[many.index(A)] > 0 and len(res.counts) == 66
    # a class with no record and a class with all of them
    res, v = run([b"@r", b"\x02nowhere"], 0, None)
    assert res.counts.tolist() == [nrec, 0, 0, 0]
    res, v = run([b"\x02nowhere", A + A], 1)
    assert res.counts.tolist() == [0, 0, 0, nrec]
    # _FINAL with a short last record
    short = text + b"@rlast\n" + A + b"ACGT"
    spath = tmp_path / "short.bgzf"
    spath.write_bytes(bgzf.compress(short, block_size=997))
    with pytest.raises(ValueError, match=r"record %d, the last one, has 2 of 4 lines" % nrec):
        bgzf.classify_records(str(spath), [A, B], 4, match_line=1, first_byte=b"@", mismatches=1)
    res = bgzf.classify_records(str(spath), [A, B], 4, match_line=1, first_byte=b"@", mismatches=1, allow_short=True)
    v = classify_ref.classify(short, b"\n", [A, B], 1, 4, 1)
    agree(res, v, "short")
    assert res.searched == nrec + 1 and (res.pattern[-1], res.distance[-1]) == (0, 0)
    # a first_byte violation names the record; nothing comes back
    lines = text.split(b"\n")
    del lines[4 * 7 + 2]
    broken = b"\n".join(lines)
    bpath = tmp_path / "broken.bgzf"
    bblob = bgzf.compress(broken, block_size=997)
    bpath.write_bytes(bblob)
    with pytest.raises(ValueError, match=r"record 8 at virtual offset \d+ does not start with b'@'"):
        bgzf.classify_records(str(bpath), [A, B], 4, match_line=1, first_byte=b"@", mismatches=1, allow_short=True)
    tab, _ = block_map(bblob)
    for flags in (_lib.BGZF_GREP_FINAL, _lib.BGZF_GREP_FINAL | _lib.BGZF_CLASSIFY_GROUP):
        code, status, tot, cls, rows, packed = ctx.bgzf_classify_records(bblob, member_table(tab), 0, len(broken), *_lib.grep_pattern_table([A, B]), 10,
                                                                         flags, 1, 4, 1, ord("@"), 1000)
        at8 = len(b"\n".join(lines[:32])) + 1
        assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.covered) == (1, 1008, at8, 1) and tot.seen == nrec
        assert len(cls) == 0 and len(rows) == 0 and packed == b""


def reads(rng, n, barcodes):
    """FASTQ reads that begin with a barcode 0 to 3 places off -- or, where the last barcode is two places off the first, with the
    bases half way between the two: one place off both, a tie"""
    diff = [j for j in range(len(barcodes[0])) if len(barcodes[-1]) == len(barcodes[0]) and barcodes[0][j] != barcodes[-1][j]]
    mid = barcodes[0][:diff[0]] + barcodes[-1][diff[0]:diff[0] + 1] + barcodes[0][diff[0] + 1:] if len(diff) == 2 else barcodes[0]
    out = []
    for i in range(n):
        kind = rng.randrange(7)
        bc = rng.choice(barcodes)
        head = mutate(rng, bc, (0, 0, 1, 1, 2, 3, 0)[kind], b"\n") if kind < 6 else mid
        s = head + bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 60)))
        out.append(b"@read%d\n%s\n+\n%s\n" % (i, s, b"F" * len(s)))
    return out


def grouped(ctx, n, barcodes, recs):
    """the _GROUP call at k = 1 on the bases line, from the line's start, against the referee: counts, class rows, rows, packed bytes"""
    from zlib_ng_amd import _lib, bgzf
    ncls = len(barcodes) + 2
    text = b"".join(recs)
    blob = bgzf.compress(text, block_size=4099)
    tab, _ = block_map(blob)
    members = member_table(tab)
    table = _lib.grep_pattern_table(barcodes)
    v = classify_ref.classify(text, b"\n", barcodes, 1, 4, 1, True)
    G = _lib.BGZF_GREP_FINAL | _lib.BGZF_GREP_LINE_START | _lib.BGZF_CLASSIFY_GROUP
    code, status, tot, cls, rows, packed = ctx.bgzf_classify_records(blob, members, 0, len(text), *table, 10, G, 1, 4, 1, ord("@"), 500)
    assert code == 0 and not status.any() and (tot.covered, tot.bad, tot.seen, tot.bytes, tot.n_classes) == (1, 0, n, len(text), ncls)
    assert list(tot.class_records)[:ncls] == v.counts.tolist() and not any(list(tot.class_records)[ncls:]) and not any(list(tot.class_bytes)[ncls:])
    assert sum(tot.class_bytes) == len(text) and [tot.class_bytes[c] for c in range(ncls)] == [len(v.of_class(c)) for c in range(ncls)]
    # the class rows, in record order
    want_flags = np.where(v.pattern >= 0, 1, np.where(v.pattern == classify_ref.AMBIGUOUS, 2, 0))
    assert cls["flags"].tolist() == want_flags.tolist() and cls["distance"].tolist() == v.distance.tolist()
    assert cls["pattern"].tolist() == (v.tie[:, 0] & 255).tolist() and cls["other"].tolist() == (v.tie[:, 1] & 255).tolist()
    # the rows: by class, then by number; every record once; reserved is the record's class row
    order = np.argsort(v.cls, kind="stable")
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    assert rows["number"].tolist() == (500 + order).tolist() and sorted(rows["number"].tolist()) == list(range(500, 500 + n))
    assert rows["src_off"].tolist() == starts[:-1][order].tolist() and rows["len"].tolist() == np.diff(starts)[order].tolist()
    assert rows["reserved"].tolist() == cls.view(np.uint32)[order].tolist()
    at = 0
    for c in range(ncls):
        assert bytes(packed[at:at + tot.class_bytes[c]]) == v.of_class(c), (n, c)
        at += tot.class_bytes[c]
    assert at == len(packed) == len(text)
    # without _GROUP: the class rows alone
    code, status, tot2, cls2, rows2, packed2 = ctx.bgzf_classify_records(blob, members, 0, len(text), *table, 10, G & ~_lib.BGZF_CLASSIFY_GROUP, 1, 4, 1,
                                                                         ord("@"), 500)
    assert code == 0 and cls2.tobytes() == cls.tobytes() and len(rows2) == 0 and packed2 == b"" and list(tot2.class_records) == list(tot.class_records)
    return v


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, WG + 1, 3 * WG + 5])
def test_grouping(ctx, n):
    rng = random.Random(n)
    barcodes = [A, B, b"GGGGCCCCAAAATTTT", mutate(rng, A, 2, b"\n")]          # the last one is two off the first: ties at k = 1
    grouped(ctx, n, barcodes, reads(rng, n, barcodes))


@pytest.mark.parametrize("n", [WG + 1, 3 * WG + 5])
def test_grouping_every_class(ctx, n):
    """64 barcodes, 66 classes: read i begins with barcode i % 65, and 64 stands for random bases -- so every wave of the scatter holds
    64 different classes (one round of its ballot loop each) and the class loops of both kernels run past thread 63"""
    rng = random.Random(1000 + n)
    barcodes = []
    while len(barcodes) < 64:                                                 # any two at least 3 places apart: no tie at k = 1
        p = bytes(rng.choice(b"ACGT") for _ in range(16))
        if all(sum(x != y for x, y in zip(p, q)) >= 3 for q in barcodes):
            barcodes.append(p)
    recs = []
    for i in range(n):
        head = barcodes[i % 65] if i % 65 < 64 else bytes(rng.choice(b"ACGT") for _ in range(16))
        s = head + bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(1, 60)))
        recs.append(b"@read%d\n%s\n+\n%s\n" % (i, s, b"F" * len(s)))
    v = grouped(ctx, n, barcodes, recs)
    assert len(set(v.cls.tolist())) >= 65 and all(len(set(v.cls[a:a + 64].tolist())) == 64 for a in range(0, n - 63, 64))


@pytest.fixture(scope="module")
def golden():
    """the golden FASTQ, eight barcodes cut from the first bases of its reads, and the referee's verdict at k = 1 (computed once)"""
    blob = open(BGZIP, "rb").read()
    data = gzip.decompress(blob)
    lines = referee_lines(data, b"\n")
    rng = random.Random(12)
    barcodes = []
    while len(barcodes) < 8:
        p = lines[4 * rng.randrange(len(lines) // 4) + 1][:10]
        if len(p) == 10 and b"\n" not in p and p not in barcodes:
            barcodes.append(p)
    return blob, data, barcodes, classify_ref.classify(data, b"\n", barcodes, 1, 4, 1, True)


def test_consistent_with_grep_records(ctx, golden):
    from zlib_ng_amd import bgzf
    blob, data, barcodes, v = golden
    assert (v.pattern >= 0).sum() > 8 and (v.pattern == classify_ref.UNASSIGNED).any()
    res = bgzf.classify_records(BGZIP, barcodes, 4, match_line=1, first_byte=b"@", line_start=True, mismatches=1)
    agree(res, v)
    hits = bgzf.grep_records(BGZIP, barcodes, 4, match_line=1, first_byte=b"@", line_start=True, mismatches=1)
    assert np.nonzero(res.pattern != bgzf.UNASSIGNED)[0].tolist() == hits.numbers.tolist()
    with bgzf.open(BGZIP) as r:
        agree(r.classify_records(barcodes, 4, match_line=1, line_start=True, mismatches=1), v)


def test_small_read_windows(ctx, golden, monkeypatch):
    """records are carried across windows; the result is that of one window"""
    from zlib_ng_amd import bgzf
    blob, data, barcodes, v = golden
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 100000)
    ctx.bgzf_stats()
    res = bgzf.classify_records(BGZIP, barcodes, 4, match_line=1, first_byte=b"@", line_start=True, mismatches=1)
    assert ctx.bgzf_stats()[0] > 5
    agree(res, v)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in v.records])])
    tab, _ = block_map(blob)
    us = np.array([u for c, u, cs, isz in tab])

    def voff(r):
        b = int(np.searchsorted(us, starts[r], "right")) - 1
        return bgzf.make_virtual_offset(tab[b][0], int(starts[r]) - tab[b][1])

    a, b = len(v.records) // 3, 2 * len(v.records) // 3
    mid = bgzf.classify_records(BGZIP, barcodes, 4, match_line=1, line_start=True, mismatches=1, start=voff(a), stop=voff(b), first_record=a)
    agree(mid, v, "start / stop", a, b)
    assert mid.first_record == a


def test_device_form(ctx):
    from zlib_ng_amd import _lib, bgzf, devmem
    rng = random.Random(31)
    barcodes = [A, B, b"GGGGCCCCAAAATTTT"]
    recs = reads(rng, 300, barcodes)
    text = b"".join(recs)
    blob = bgzf.compress(text, block_size=1001)
    tab, _ = block_map(blob)
    members = member_table(tab)
    table = _lib.grep_pattern_table(barcodes)
    n, nb = len(recs), len(text)
    G = _lib.BGZF_GREP_FINAL | _lib.BGZF_CLASSIFY_GROUP
    code, status, tot_h, cls_h, rows_h, packed_h = ctx.bgzf_classify_records(blob, members, 0, nb, *table, 10, G, 1, 4, 1, ord("@"), 0)
    v = classify_ref.classify(text, b"\n", barcodes, 1, 4, 1)
    assert code == 0 and list(tot_h.class_records)[:5] == v.counts.tolist() and len(cls_h) == n
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(tab))
    canary = lambda size: devmem.from_host(ctx, b"\xa5" * size)
    d_cls, d_rows, d_out = canary(4 * n), canary(24 * n), canary(nb)

    def call(m, flags, ccap, rcap, ocap, first_byte=ord("@")):
        return ctx.bgzf_classify_records_dev(d_in.ptr, len(blob), m.ptr, len(tab), 0, nb, *table, 10, flags, 1, 4, 1, first_byte, 0, d_scratch.ptr, nb,
                                             d_st.ptr, d_cls.ptr if ccap else 0, ccap, d_rows.ptr if rcap else 0, rcap, d_out.ptr if ocap else 0, ocap)

    def untouched():
        return d_cls.cpu().tobytes() == b"\xa5" * (4 * n) and d_rows.cpu().tobytes() == b"\xa5" * (24 * n) and d_out.cpu().tobytes() == b"\xa5" * nb

    for caps in ((n - 1, n, nb), (n, n - 1, nb), (n, n, nb - 1)):
        code, tot = call(d_m, G, *caps)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.bytes, tot.covered, tot.bad, tot.n_classes) == (n, nb, 1, 0, 5), caps
        assert list(tot.class_records) == list(tot_h.class_records) and list(tot.class_bytes) == list(tot_h.class_bytes) and untouched(), caps
    code, tot = call(d_m, _lib.BGZF_GREP_FINAL, n - 1, 0, 0)                      # without _GROUP only the class rows need room
    assert code == _lib.BUF_ERROR and tot.seen == n and untouched()
    # the member rows do not tile the text: covered = 0 and nothing else
    swapped = members.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    code, tot = call(devmem.from_host(ctx, swapped.tobytes()), G, n, n, nb)
    assert code == 0 and (tot.covered, tot.seen, tot.bytes) == (0, 0, 0) and not any(tot.class_records) and untouched()
    # a first_byte violation: bad, and no row and no byte
    code, tot = call(d_m, G, n, n, nb, first_byte=ord("+"))
    assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (1, 0, 0, n) and untouched()
    # without _GROUP: the class rows alone, rows and bytes may be NULL
    code, tot = call(d_m, _lib.BGZF_GREP_FINAL, n, 0, 0)
    assert code == 0 and d_cls.cpu(_lib.CLASS_ROW_DTYPE).tobytes() == cls_h.tobytes() and d_rows.cpu().tobytes() == b"\xa5" * (24 * n)
    # exact capacities
    d_cls = canary(4 * n)
    code, tot = call(d_m, G, n, n, nb)
    assert code == 0 and (tot.seen, tot.bytes, tot.tail_off) == (n, nb, nb) and list(tot.class_records) == list(tot_h.class_records)
    assert d_cls.cpu(_lib.CLASS_ROW_DTYPE).tobytes() == cls_h.tobytes() and d_rows.cpu(_lib.GREP_ROW_DTYPE).tobytes() == rows_h.tobytes()
    assert d_out.cpu().tobytes() == bytes(packed_h) == b"".join(v.of_class(c) for c in range(5))
    # without _FINAL the last record is whole here, and the tail is where the next one would start
    code, tot = call(d_m, _lib.BGZF_CLASSIFY_GROUP, n, n, nb)
    assert code == 0 and (tot.seen, tot.tail_off, tot.short_lines) == (n, nb, 0)
    for bad in (dict(mismatches=16), dict(flags=1), dict(flags=8)):
        with pytest.raises(_lib.EngineError):
            ctx.bgzf_classify_records(blob, members, 0, nb, *table, 10, bad.get("flags", G), bad.get("mismatches", 1), 4, 1, ord("@"), 0)


def check_outputs(paths, v, n_patterns, dropped=()):
    from zlib_ng_amd import bgzf
    for c, p in enumerate(paths):
        if c in dropped:
            assert p is None
            continue
        blob = open(p, "rb").read()
        assert blob.endswith(bgzf.EOF_BLOCK)
        tab, _ = block_map(blob)                                                # (the host scan walks every block to the end of the file)
        assert tab[-1][3] == 0 and sum(isz for c_, u, cs, isz in tab) == len(v.of_class(c))
        assert gzip.decompress(blob) == v.of_class(c), (c, p)


def test_demux_golden(ctx, golden, tmp_path):
    from zlib_ng_amd import bgzf
    blob, data, barcodes, v = golden
    outs = [str(tmp_path / ("bc%d.fastq.gz" % i)) for i in range(8)]
    amb, una = str(tmp_path / "amb.gz"), str(tmp_path / "una.gz")
    counts = bgzf.demux(BGZIP, barcodes, outs, 4, ambiguous=amb, unassigned=una, compresslevel=1, match_line=1, first_byte=b"@", line_start=True,
                        mismatches=1)
    assert counts.tolist() == v.counts.tolist() and counts.sum() == len(v.records)
    check_outputs(outs + [amb, una], v, 8)
    # ambiguous = None and unassigned = None drop those records and still count them; files are taken as well as paths
    with open(outs[0], "wb") as f0, bgzf.open(BGZIP) as r:
        counts = r.demux(barcodes, [f0] + outs[1:], compresslevel=6, match_line=1, line_start=True, mismatches=1)
        assert not f0.closed
    assert counts.tolist() == v.counts.tolist()
    check_outputs(outs + [None, None], v, 8, dropped=(8, 9))


def test_demux_generated(ctx, tmp_path, monkeypatch):
    from zlib_ng_amd import bgzf
    rng = random.Random(77)
    barcodes = [A, B, b"GGGGCCCCAAAATTTT", mutate(rng, A, 2, b"\n")]
    text = b"".join(reads(rng, 3000, barcodes))
    src = tmp_path / "in.bgzf"
    src.write_bytes(bgzf.compress(text, block_size=5000))
    v = classify_ref.classify(text, b"\n", barcodes, 1, 4, 1, True)
    assert (v.counts > 0).all()
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 60000)                            # several windows: every class is written piece by piece
    outs = [str(tmp_path / ("o%d.gz" % i)) for i in range(4)]
    una = str(tmp_path / "una.gz")
    counts = bgzf.demux(str(src), barcodes, outs, unassigned=una, compresslevel=1, block_size=4096, match_line=1, first_byte=b"@", line_start=True,
                        mismatches=1)
    assert counts.tolist() == v.counts.tolist()
    check_outputs(outs + [None, una], v, 4, dropped=(4,))

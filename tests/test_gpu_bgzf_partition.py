"""BGZF by a label per record (bgzf.partition_records / demux_paired / pair_labels; csrc/za_partition.hip).  The referee is
partition_ref.py: plain Python that cuts the text into records and groups them by label, never the code under test.  The tests on the
golden FASTQ pin the new path to what demux() writes."""
import functools
import gzip
import os
import random

import numpy as np
import pytest

import classify_ref
import partition_ref
from test_gpu_bgzf_classify import A, B, reads
from test_gpu_bgzf_grep import block_map
from test_gpu_bgzf_grep_approx import mutate
from test_gpu_bgzf_lines import BGZIP, member_table, referee_lines

pytestmark = pytest.mark.gpu

DROP = partition_ref.DROP
BASE = 500                                                   # record_base of the calls through the C ABI


def gen_fastq(n, seed, lo=1, hi=90):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        s = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(lo, hi)))
        out.append(b"@q%d\n%s\n+\n%s\n" % (i, s, b"F" * len(s)))
    return out


@functools.lru_cache(maxsize=None)
def text_of(n):
    """-> (records, text, BGZF blob, member table) of n generated reads: computed once per n, never changed"""
    from zlib_ng_amd import bgzf
    recs = gen_fastq(n, n)
    text = b"".join(recs)
    blob = bgzf.compress(text, block_size=4099)
    tab, _ = block_map(blob)
    return recs, text, blob, member_table(tab)


def u16(labels):
    return np.array([0xFFFF if x < 0 else x for x in labels], np.uint16)


def call(ctx, n, labels, ncls, flags, first_byte=ord("@")):
    recs, text, blob, members = text_of(n)
    return ctx.bgzf_partition_records(blob, members, 0, len(text), 10, flags, 4, first_byte, BASE, u16(labels), ncls)


def label_sets(n):
    yield "one class", [0] * n, 1
    yield "one class of five", [3] * n, 5
    for ncls in (2, 66, 67, 257, 1024):                      # a wave holds 64 different classes; most classes are empty; the strided loops run
        yield "r %% %d" % ncls, [r % ncls for r in range(n)], ncls
    yield "all dropped", [DROP] * n, 3
    yield "every third dropped", [DROP if r % 3 == 0 else (7 * r) % 5 for r in range(n)], 5
    yield "the last record alone in its class", [r % 2 for r in range(n - 1)] + [900], 901


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3 * 256 + 5])
def test_grid(ctx, n):
    from zlib_ng_amd import _lib
    recs, text, blob, members = text_of(n)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    for what, labels, ncls in label_sets(n):
        what = (n, what)
        p = partition_ref.Partition(text, labels, ncls)
        code, status, tot, crec, cbytes, rows, packed = call(ctx, n, labels, ncls, F | G)
        assert code == 0 and not status.any(), what
        assert (tot.covered, tot.bad, tot.labels_short, tot.seen, tot.short_lines, tot.tail_off) == (1, 0, 0, n, 0, len(text)), what
        assert (tot.dropped, tot.dropped_bytes, tot.bytes) == (p.dropped, p.dropped_bytes, len(text) - p.dropped_bytes), what
        assert crec.tolist() == p.counts and cbytes.tolist() == [len(p.of_class(c)) for c in range(ncls)], what
        # the rows: by class, then by number; every kept record once; reserved is the label
        order = np.array(p.order(), np.int64)
        assert len(rows) == n - p.dropped and rows["number"].tolist() == (BASE + order).tolist(), what
        assert rows["src_off"].tolist() == starts[:-1][order].tolist() and rows["len"].tolist() == np.diff(starts)[order].tolist(), what
        assert rows["reserved"].tolist() == [labels[r] for r in order.tolist()], what
        at = 0
        for c in range(ncls):
            if cbytes[c]:
                assert bytes(packed[at:at + int(cbytes[c])]) == p.of_class(c), (what, c)
            at += int(cbytes[c])
        assert at == len(packed) == tot.bytes, what
        # without _GROUP: the same counts, and nothing else
        code, status, tot2, crec2, cbytes2, rows2, packed2 = call(ctx, n, labels, ncls, F)
        assert code == 0 and crec2.tolist() == p.counts and cbytes2.tolist() == cbytes.tolist() and len(rows2) == 0 and packed2 == b"", what
        assert (tot2.seen, tot2.bytes, tot2.dropped, tot2.dropped_bytes, tot2.tail_off) == (n, tot.bytes, p.dropped, p.dropped_bytes, len(text)), what


def test_faults(ctx):
    from zlib_ng_amd import _lib, bgzf
    n, ncls = 300, 7
    recs, text, blob, members = text_of(n)
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    good = [r % ncls for r in range(n)]
    p = partition_ref.Partition(text, good, ncls)

    def nothing(res):
        return len(res[5]) == 0 and res[6] == b""

    # a label equal to n_classes: the smallest such record
    labels = list(good)
    labels[200] = labels[77] = ncls
    for flags in (F, F | G):
        res = call(ctx, n, labels, ncls, flags)
        tot = res[2]
        assert res[0] == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen, tot.covered) == (2, BASE + 77, starts[77], n, 1) and nothing(res)
    labels[77] = 0xFFFE                                                       # the largest value that is no class and not DROP
    assert call(ctx, n, labels, 1024, F | G)[2].bad_record == BASE + 77

    def with_bad_first_byte(at):
        """the text with record `at` starting with '#'"""
        broken = bytearray(text)
        broken[starts[at]] = ord("#")
        b = bgzf.compress(bytes(broken), block_size=4099)
        tab, _ = block_map(b)
        return b, member_table(tab)

    labels = list(good)
    labels[77] = ncls
    for at, want in ((150, (2, BASE + 77, starts[77])), (30, (1, BASE + 30, starts[30])), (77, (1, BASE + 77, starts[77]))):
        b, m = with_bad_first_byte(at)                                        # a later, an earlier violation, and both faults in one record
        res = ctx.bgzf_partition_records(b, m, 0, len(text), 10, F | G, 4, ord("@"), BASE, u16(labels), ncls)
        tot = res[2]
        assert res[0] == 0 and (tot.bad, tot.bad_record, tot.bad_src) == want and tot.seen == n and nothing(res), at
        res = ctx.bgzf_partition_records(b, m, 0, len(text), 10, F | G, 4, -1, BASE, u16(good), ncls)      # (no first_byte: no fault)
        assert res[2].bad == 0 and len(res[5]) == n
    # fewer labels than records: labels_short, and nothing written; the record without a label counts as dropped
    res = ctx.bgzf_partition_records(blob, members, 0, len(text), 10, F | G, 4, ord("@"), BASE, u16(good[:n - 1]), ncls)
    tot = res[2]
    assert res[0] == 0 and (tot.labels_short, tot.bad, tot.seen, tot.dropped, tot.dropped_bytes) == (1, 0, n, 1, len(recs[-1])) and nothing(res)
    assert res[3].tolist() == partition_ref.Partition(b"".join(recs[:-1]), good[:-1], ncls).counts
    res = ctx.bgzf_partition_records(blob, members, 0, len(text), 10, F, 4, ord("@"), BASE, u16([]), ncls)
    assert (res[2].labels_short, res[2].seen, res[2].dropped) == (1, n, n) and not res[3].any()
    # more labels than records: no fault, the labels behind the records are not read
    res = ctx.bgzf_partition_records(blob, members, 0, len(text), 10, F | G, 4, ord("@"), BASE, u16(good + [ncls] * 5), ncls)
    tot = res[2]
    assert res[0] == 0 and (tot.labels_short, tot.bad, tot.seen) == (0, 0, n) and res[3].tolist() == p.counts
    assert bytes(res[6]) == b"".join(p.of_class(c) for c in range(ncls))
    # an open tail: without _FINAL the two lines behind the last whole record are left to the next call; with it they are a short record
    more = text + b"@open\nACGT\n"
    b = bgzf.compress(more, block_size=4099)
    tab, _ = block_map(b)
    m = member_table(tab)
    res = ctx.bgzf_partition_records(b, m, 0, len(more), 10, G, 4, ord("@"), BASE, u16(good + [3]), ncls)
    tot = res[2]
    assert (tot.seen, tot.tail_off, tot.short_lines, tot.labels_short, tot.bad) == (n, len(text), 0, 0, 0) and res[3].tolist() == p.counts
    assert bytes(res[6]) == b"".join(p.of_class(c) for c in range(ncls))
    res = ctx.bgzf_partition_records(b, m, 0, len(more), 10, F | G, 4, ord("@"), BASE, u16(good + [3]), ncls)
    tot = res[2]
    q = partition_ref.Partition(more, good + [3], ncls)
    assert (tot.seen, tot.tail_off, tot.short_lines, tot.labels_short) == (n + 1, len(more), 2, 0) and q.short_lines == 2
    assert res[3].tolist() == q.counts and bytes(res[6]) == b"".join(q.of_class(c) for c in range(ncls))
    res = ctx.bgzf_partition_records(b, m, 0, len(more), 10, F | G, 4, ord("@"), BASE, u16(good), ncls)      # the short record has no label
    assert (res[2].seen, res[2].labels_short) == (n + 1, 1) and nothing(res)
    for bad in (dict(flags=1), dict(flags=2), dict(flags=8), dict(ncls=0), dict(ncls=1025)):
        with pytest.raises(_lib.EngineError):
            call(ctx, n, good, bad.get("ncls", ncls), bad.get("flags", F | G))


def test_device_form(ctx):
    from zlib_ng_amd import _lib, devmem
    n, ncls = 300, 70
    recs, text, blob, members = text_of(n)
    nb = len(text)
    labels = [DROP if r % 10 == 0 else (3 * r) % ncls for r in range(n)]
    p = partition_ref.Partition(text, labels, ncls)
    kept, kb = n - p.dropped, nb - p.dropped_bytes
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    code, status, tot_h, crec_h, cbytes_h, rows_h, packed_h = call(ctx, n, labels, ncls, F | G)
    assert code == 0 and crec_h.tolist() == p.counts and len(rows_h) == kept and len(packed_h) == kb
    d_in, d_m = devmem.from_host(ctx, blob + bytes(64)), devmem.from_host(ctx, members.tobytes())
    d_scratch, d_st = devmem.empty(ctx, nb), devmem.empty(ctx, 4 * len(members))
    d_lab = devmem.from_host(ctx, u16(labels).tobytes())
    canary = lambda size: devmem.from_host(ctx, b"\xa5" * size)
    d_rows, d_out = canary(24 * kept), canary(kb)

    def dev(m, flags, rcap, ocap, first_byte=ord("@"), n_labels=n):
        return ctx.bgzf_partition_records_dev(d_in.ptr, len(blob), m.ptr, len(members), 0, nb, 10, flags, 4, first_byte, BASE, d_scratch.ptr, nb, d_st.ptr,
                                              d_rows.ptr if rcap else 0, rcap, d_out.ptr if ocap else 0, ocap, d_lab.ptr, n_labels, ncls)

    def untouched():
        return d_rows.cpu().tobytes() == b"\xa5" * (24 * kept) and d_out.cpu().tobytes() == b"\xa5" * kb

    for caps in ((kept - 1, kb), (kept, kb - 1)):                             # each capacity one too small
        code, tot, crec, cbytes = dev(d_m, F | G, *caps)
        assert code == _lib.BUF_ERROR and (tot.seen, tot.bytes, tot.dropped, tot.covered, tot.bad) == (n, kb, p.dropped, 1, 0), caps
        assert crec.tolist() == p.counts and cbytes.tolist() == cbytes_h.tolist() and untouched(), caps
    # the member rows do not tile the text: covered = 0 and nothing else
    swapped = members.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    code, tot, crec, cbytes = dev(devmem.from_host(ctx, swapped.tobytes()), F | G, kept, kb)
    assert code == 0 and (tot.covered, tot.seen, tot.bytes) == (0, 0, 0) and not crec.any() and not cbytes.any() and untouched()
    # a fault, too few labels: no row and no byte
    code, tot, crec, cbytes = dev(d_m, F | G, kept, kb, first_byte=ord("+"))
    assert code == 0 and (tot.bad, tot.bad_record, tot.bad_src, tot.seen) == (1, BASE, 0, n) and untouched()
    code, tot, crec, cbytes = dev(d_m, F | G, kept, kb, n_labels=n - 1)
    assert code == 0 and (tot.labels_short, tot.seen) == (1, n) and untouched()
    # without _GROUP: the counts alone, rows and bytes may be NULL
    code, tot, crec, cbytes = dev(d_m, F, 0, 0)
    assert code == 0 and crec.tolist() == p.counts and cbytes.tolist() == cbytes_h.tolist() and (tot.seen, tot.dropped_bytes) == (n, p.dropped_bytes) and untouched()
    # exact capacities
    code, tot, crec, cbytes = dev(d_m, F | G, kept, kb)
    assert code == 0 and (tot.seen, tot.bytes, tot.tail_off, tot.dropped) == (n, kb, nb, p.dropped) and crec.tolist() == p.counts
    assert d_rows.cpu(_lib.GREP_ROW_DTYPE).tobytes() == rows_h.tobytes()
    assert d_out.cpu().tobytes() == bytes(packed_h) == b"".join(p.of_class(c) for c in range(ncls))
    # without _FINAL the last record is whole here, and the tail is where the next one would start
    code, tot, crec, cbytes = dev(d_m, G, kept, kb)
    assert code == 0 and (tot.seen, tot.tail_off, tot.short_lines) == (n, nb, 0)


@pytest.fixture(scope="module")
def golden():
    """the golden FASTQ, its record starts and eight barcodes cut from the first bases of its reads"""
    blob = open(BGZIP, "rb").read()
    data = gzip.decompress(blob)
    lines = referee_lines(data, b"\n")
    rng = random.Random(12)
    barcodes = []
    while len(barcodes) < 8:
        q = lines[4 * rng.randrange(len(lines) // 4) + 1][:10]
        if len(q) == 10 and b"\n" not in q and q not in barcodes:
            barcodes.append(q)
    recs, short = partition_ref.records_of(data, 4)
    assert short == 0
    return blob, barcodes, np.concatenate([[0], np.cumsum([len(x) for x in recs])])


def unzipped(paths):
    from zlib_ng_amd import bgzf
    out = []
    for q in paths:
        blob = open(q, "rb").read()
        assert blob.endswith(bgzf.EOF_BLOCK), q
        out.append(gzip.decompress(blob))
    return out


KW = dict(match_line=1, first_byte=b"@", line_start=True, mismatches=1)


def same_as_demux(tmp_path, barcodes, **rng):
    """partition_records with the labels of classify_records writes what demux() writes with the same arguments"""
    from zlib_ng_amd import bgzf
    d = [str(tmp_path / ("d%d.gz" % i)) for i in range(10)]
    q = [str(tmp_path / ("p%d.gz" % i)) for i in range(10)]
    counts = bgzf.demux(BGZIP, barcodes, d[:8], 4, ambiguous=d[8], unassigned=d[9], compresslevel=1, **KW, **rng)
    res = bgzf.classify_records(BGZIP, barcodes, 4, **KW, **rng)
    assert res.counts.tolist() == counts.tolist()
    got = bgzf.partition_records(BGZIP, res.labels(), q, 4, first_byte=b"@", compresslevel=1, **rng)
    assert got.tolist() == counts.tolist() + [0] and got.dtype == np.int64
    want = unzipped(d)
    assert unzipped(q) == want and sum(len(x) for x in want) > 0 and sum(1 for x in want if x) > 3
    return res, want


def test_same_as_demux_on_the_golden_file(ctx, golden, tmp_path):
    from zlib_ng_amd import bgzf
    res, want = same_as_demux(tmp_path, golden[1])
    assert sum(len(x) for x in want) == golden[2][-1]
    # an output of None and DROP labels: counted, written nowhere; a reader's method; outputs=None only counts
    labels = res.labels()
    labels[::5] = bgzf.DROP
    q = [None if i in (2, 9) else str(tmp_path / ("r%d.gz" % i)) for i in range(10)]
    with bgzf.open(BGZIP) as r:
        got = r.partition_records(labels, q, first_byte=b"@", compresslevel=1)
        assert bgzf.partition_records(BGZIP, labels, None).tolist() == got.tolist()
    assert got.tolist() == np.bincount(labels[labels >= 0], minlength=10).tolist() + [int((labels < 0).sum())]
    recs = [bytes(x) for x in np.split(np.frombuffer(gzip.decompress(golden[0]), np.uint8), golden[2][1:-1])]
    for c in range(10):
        if q[c] is not None:
            assert unzipped([q[c]])[0] == b"".join(recs[i] for i in np.nonzero(labels == c)[0].tolist()), c


def test_small_read_windows(ctx, golden, tmp_path, monkeypatch):
    """records and the label offset are carried across windows; the result is that of one window"""
    from zlib_ng_amd import bgzf
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 100000)
    res = bgzf.classify_records(BGZIP, golden[1], 4, **KW)
    q = [str(tmp_path / ("w%d.gz" % i)) for i in range(10)]
    ctx.bgzf_stats()
    bgzf.partition_records(BGZIP, res.labels(), q, first_byte=b"@", compresslevel=1)
    assert ctx.bgzf_stats()[0] > 5
    same_as_demux(tmp_path, golden[1])
    # the middle third: start, stop and first_record
    blob, barcodes, starts = golden
    tab, _ = block_map(blob)
    us = np.array([u for c, u, cs, isz in tab])

    def voff(r):
        b = int(np.searchsorted(us, starts[r], "right")) - 1
        return bgzf.make_virtual_offset(tab[b][0], int(starts[r]) - tab[b][1])

    nrec = len(starts) - 1
    a, b = nrec // 3, 2 * nrec // 3
    res, want = same_as_demux(tmp_path, barcodes, start=voff(a), stop=voff(b), first_record=a)
    assert len(res) == b - a and res.first_record == a and sum(len(x) for x in want) == starts[b] - starts[a]
    # labels for more or fewer records than the range holds: out of step
    for labels in (res.labels()[:-1], np.concatenate([res.labels(), [0]])):
        with pytest.raises(ValueError, match=r"the file holds %d records and labels has %d entries: the files are out of step" % (b - a, len(labels))):
            bgzf.partition_records(BGZIP, labels, None, start=voff(a), stop=voff(b), first_record=a)


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """R1 (a barcode, then 150 to 350 bases) and R2 (200 to 400 bases, no barcode) of 3000 reads as files, each of several read windows
    of 60000 bytes; the referee's verdict on R1 and its grouping of R2 (computed once)"""
    from zlib_ng_amd import bgzf
    rng = random.Random(77)
    barcodes = [A, B, b"GGGGCCCCAAAATTTT", mutate(rng, A, 2, b"\n")]
    r1 = []
    for rec in reads(rng, 3000, barcodes):                   # the reads of the classify tests, made longer
        head, s = rec.split(b"\n")[:2]
        s += bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(150, 300)))
        r1.append(b"%s\n%s\n+\n%s\n" % (head, s, b"F" * len(s)))
    r2 = [b"@read%d/2\n%s\n+\n%s\n" % (i, s, b"#" * len(s)) for i, s in
          enumerate(bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(200, 400))) for _ in range(3000))]
    v = classify_ref.classify(b"".join(r1), b"\n", barcodes, 1, 4, 1, True)
    assert (v.counts > 0).all()
    d = tmp_path_factory.mktemp("pair")
    f1, f2 = str(d / "r1.gz"), str(d / "r2.gz")
    open(f1, "wb").write(bgzf.compress(b"".join(r1), block_size=5000))
    open(f2, "wb").write(bgzf.compress(b"".join(r2), block_size=5000))
    assert min(os.path.getsize(f1), os.path.getsize(f2)) > 60000 + 65536      # more than a window and the block read behind it: each file takes several
    return barcodes, r2, v, partition_ref.Partition(b"".join(r2), v.cls.tolist(), 6), f1, f2


PAIR_KW = dict(compresslevel=1, block_size=4096, **KW)


@pytest.mark.parametrize("bf", [0, 1])
def test_demux_paired(ctx, pair, tmp_path, monkeypatch, bf):
    from zlib_ng_amd import bgzf
    barcodes, r2, v, mate, f1, f2 = pair
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 60000)           # several windows, cut at other records in R1 than in R2
    outs = [[str(tmp_path / ("f%d_%d.gz" % (f, i))) for i in range(6)] for f in range(2)]
    ctx.bgzf_stats()
    counts = bgzf.demux_paired([f1, f2] if bf == 0 else [f2, f1], barcodes, [o[:4] for o in outs], barcode_file=bf, ambiguous=[o[4] for o in outs],
                               unassigned=[o[5] for o in outs], **PAIR_KW)
    assert ctx.bgzf_stats()[0] >= 4                                                # (both files were read in several windows)
    assert counts.tolist() == v.counts.tolist()
    assert unzipped(outs[bf]) == [v.of_class(c) for c in range(6)]                 # the barcode file: the referee's
    assert unzipped(outs[1 - bf]) == [mate.of_class(c) for c in range(6)]          # the mate follows
    if bf == 0:                                                                    # R1's outputs are demux()'s
        d = [str(tmp_path / ("d%d.gz" % i)) for i in range(6)]
        assert bgzf.demux(f1, barcodes, d[:4], ambiguous=d[4], unassigned=d[5], **PAIR_KW).tolist() == counts.tolist()
        assert [open(x, "rb").read() for x in d] == [open(x, "rb").read() for x in outs[0]]
    else:                                                                          # a reader's method, the other reads dropped
        outs = [[str(tmp_path / ("m_f%d_%d.gz" % (f, i))) for i in range(4)] for f in range(2)]
        with bgzf.open(f1) as r:
            assert r.demux_paired([f2], barcodes, outs, **PAIR_KW).tolist() == v.counts.tolist()
        assert unzipped(outs[1]) == [mate.of_class(c) for c in range(4)]


@pytest.mark.parametrize("what", ["lost", "gained"])
def test_mate_out_of_step(ctx, pair, tmp_path, monkeypatch, what):
    """a mate that lost a read, and one that gained one: the ValueError, and the outputs are closed"""
    from zlib_ng_amd import bgzf
    barcodes, r2, v, mate, f1, f2 = pair
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 60000)
    recs = r2[:1500] + r2[1501:] if what == "lost" else r2 + r2[:1]
    fx = str(tmp_path / "mate.gz")
    open(fx, "wb").write(bgzf.compress(b"".join(recs), block_size=5000))
    outs = [[str(tmp_path / ("f%d_%d.gz" % (f, i))) for i in range(4)] for f in range(2)]
    with pytest.raises(ValueError, match=r"the file holds %d records and labels has 3000 entries: the files are out of step.*incomplete" % len(recs)):
        bgzf.demux_paired([f1, fx], barcodes, outs, **PAIR_KW)
    got = unzipped(outs[0] + outs[1])                                              # every output is a complete BGZF file: it was closed
    assert got[:4] == [v.of_class(c) for c in range(4)]


def test_dual_index(ctx, tmp_path):
    """I1 and I2 carry the barcodes, R1 the reads; the sample is the pair looked up in the sheet"""
    from zlib_ng_amd import bgzf
    rng = random.Random(41)
    i7 = [b"ACGTTGCA", b"TGCAACGT", b"GGGGCCCC", b"CATGCATG"]
    i5 = [b"AACCGGTT", b"TTGGCCAA", b"GATCGATC"]
    sheet = [(0, 0), (0, 1), (1, 1), (1, 2), (2, 0), (2, 2), (3, 0), (3, 1)]
    n = 600
    i1, i2, r1, want = [], [], [], []
    for r in range(n):
        i, j = rng.randrange(4), rng.randrange(3)
        kind = r % 9
        a, b = i7[i], i5[j]
        if kind == 7:
            a = b"N" * 8                                                           # no barcode in I1: unassigned
            want.append(len(sheet) + 1)
        elif kind == 8:
            b = b"N" * 8
            want.append(len(sheet) + 1)
        else:
            want.append(sheet.index((i, j)) if (i, j) in sheet else len(sheet) + 2)      # a pair that is not in the sheet has hopped
        s = bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(30, 120)))
        i1.append(b"@r%d 1\n%s\n+\n%s\n" % (r, a, b"F" * 8))
        i2.append(b"@r%d 2\n%s\n+\n%s\n" % (r, b, b"F" * 8))
        r1.append(b"@r%d\n%s\n+\n%s\n" % (r, s, b"F" * len(s)))
    assert len(sheet) + 2 in want and len(sheet) + 1 in want and all(s in want for s in range(len(sheet)))
    paths = []
    for name, recs in (("i1", i1), ("i2", i2), ("r1", r1)):
        paths.append(str(tmp_path / (name + ".gz")))
        open(paths[-1], "wb").write(bgzf.compress(b"".join(recs), block_size=4099))
    first = bgzf.classify_records(paths[0], i7, 4, match_line=1, first_byte=b"@", line_start=True)
    second = bgzf.classify_records(paths[1], i5, 4, match_line=1, first_byte=b"@", line_start=True)
    labels = bgzf.pair_labels(first, second, sheet)
    assert labels.tolist() == want
    ncls = len(sheet) + 3
    outs = [str(tmp_path / ("s%d.gz" % c)) for c in range(ncls)]
    counts = bgzf.partition_records(paths[2], labels, outs, first_byte=b"@", compresslevel=1)
    p = partition_ref.Partition(b"".join(r1), want, ncls)
    assert counts.tolist() == p.counts + [0] and p.counts[len(sheet)] == 0
    assert unzipped(outs) == [p.of_class(c) for c in range(ncls)]

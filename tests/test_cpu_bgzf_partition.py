"""CPU: BGZF by a label per record, without a GPU -- the referee of partition_ref.py on hand-written texts; ClassifyResult.labels() and
pair_labels(); the argument checks of bgzf.partition_records / demux_paired / pair_labels that need no context; the two
zngamd_bgzf_partition_records entry points are declared, exported and bound, and refuse hostile arguments with no context at all; the
window loop on a stand-in engine whose rule is the referee (stored-block BGZF written here, the system zlib decodes it); and
tests/partition_args.cpp, a stand-alone program, against the library's host side under AddressSanitizer + UndefinedBehaviorSanitizer
(a plain child process, nothing preloaded)."""
import ctypes as C
import io
import os
import re
import subprocess
import types
import zlib

import numpy as np
import pytest

import classify_ref
import partition_ref
from conftest import PKG_DIR, ROOT
from test_cpu_bgzf_classify import _Collect, _FakeClassifyCtx, _reads
from test_cpu_bgzf_grep import _stored_bgzf
from test_cpu_bgzf_grep_approx import _Unreadable, _hipcc_clang


def test_referee_on_hand_written_texts():
    text = b"@a\nAC\n+\nII\n@b\nG\n+\nI\n@c\nTTT\n+\nIII\n"
    recs, short = partition_ref.records_of(text, 4)
    assert recs == [b"@a\nAC\n+\nII\n", b"@b\nG\n+\nI\n", b"@c\nTTT\n+\nIII\n"] and short == 0
    p = partition_ref.Partition(text, [1, partition_ref.DROP, 1], 3)
    assert p.counts == [0, 2, 0] and (p.dropped, p.dropped_bytes) == (1, len(recs[1])) and p.order() == [0, 2]
    assert p.of_class(1) == recs[0] + recs[2] and p.of_class(0) == b"" and p.members(1) == [0, 2]
    p = partition_ref.Partition(text, [2, 0, 1], 3)
    assert p.order() == [1, 2, 0] and p.dropped == 0 and b"".join(p.of_class(c) for c in range(3)) == recs[1] + recs[2] + recs[0]
    # the lines left over are a short last record; a remainder without a delimiter is a line
    recs, short = partition_ref.records_of(text + b"@d\nA", 4)
    assert len(recs) == 4 and recs[3] == b"@d\nA" and short == 2
    recs, short = partition_ref.records_of(b"a;b;;c", 2, b";")
    assert recs == [b"a;b;", b";c"] and short == 0
    assert partition_ref.records_of(b"", 4) == ([], 0) and partition_ref.records_of(b"\n", 1) == ([b"\n"], 0)
    for labels, n in (([0, 1], 3), ([0, 1, 3], 3), ([0, -2, 1], 3)):
        with pytest.raises(ValueError):
            partition_ref.Partition(text, labels, n)


def _result(pattern, n_patterns):
    from zlib_ng_amd import bgzf
    pattern = np.asarray(pattern, np.int16)
    cls = np.where(pattern >= 0, pattern, np.where(pattern == bgzf.AMBIGUOUS, n_patterns, n_patterns + 1))
    tie = np.stack([np.maximum(pattern, -1)] * 2, 1)
    return bgzf.ClassifyResult(pattern, np.where(pattern >= 0, 0, 255), tie, np.bincount(cls, minlength=n_patterns + 2))


def test_classify_result_labels():
    from zlib_ng_amd import bgzf
    U, A = bgzf.UNASSIGNED, bgzf.AMBIGUOUS
    r = _result([0, U, A, 2, 1, U], 3)
    lab = r.labels()
    assert lab.dtype == np.int32 and lab.tolist() == [0, 4, 3, 2, 1, 4]
    assert np.bincount(lab, minlength=5).tolist() == r.counts.tolist()                 # the numbering of counts
    assert _result([], 2).labels().tolist() == [] and _result([], 2).labels().dtype == np.int32
    assert (bgzf.DROP, bgzf._lib.BGZF_PARTITION_DROP, bgzf._lib.BGZF_PARTITION_MAX_CLASSES) == (-1, 0xFFFF, 1024)


def test_pair_labels():
    from zlib_ng_amd import bgzf
    U, A = bgzf.UNASSIGNED, bgzf.AMBIGUOUS
    first = _result([0, 1, 3, 0, A, U, A, U, 2, 1], 4)
    second = _result([0, 2, 1, 1, 0, 0, U, A, A, U], 3)
    sheet = [(0, 0), (1, 2), (3, 1), (2, 2)]
    got = bgzf.pair_labels(first, second, sheet)
    n = len(sheet)
    #                            s=0 s=1 s=2 hop   amb  una  una (wins) una (wins)  amb  una
    assert got.tolist() == [0, 1, 2, n + 2, n, n + 1, n + 1, n + 1, n, n + 1] and got.dtype == np.int32
    assert bgzf.pair_labels(first, second, []).tolist() == [2, 2, 2, 2, 0, 1, 1, 1, 0, 1]      # an empty sheet: every assigned pair has hopped
    assert bgzf.pair_labels(_result([], 4), _result([], 3), sheet).tolist() == []
    with pytest.raises(ValueError, match="duplicate pairs"):
        bgzf.pair_labels(first, second, [(0, 0), (1, 2), (0, 0)])
    with pytest.raises(ValueError, match="unequal length"):
        bgzf.pair_labels(first, _result([0, 1], 3), sheet)
    for bad in ([(4, 0)], [(0, 3)], [(-1, 0)]):
        with pytest.raises(ValueError, match="outside"):
            bgzf.pair_labels(first, second, bad)


def test_argument_checks_need_no_context(monkeypatch):
    from zlib_ng_amd import bgzf, zlib_ng
    monkeypatch.setattr(zlib_ng, "_ctx", lambda: pytest.fail("a context was asked for before the arguments were judged"))
    monkeypatch.setattr(bgzf, "BgzfWriter", lambda *a, **kw: pytest.fail("an output was opened before the arguments were judged"))
    outs = ["a", "b", "c"]
    for labels in ([0, 1, 3], [0, -2], [3], np.array([0, 70000]), [0.0, 1.0], [[0, 1]], [True, False], np.array([1 << 40])):
        with pytest.raises(ValueError, match="label"):
            bgzf.partition_records(_Unreadable(), labels, outs)
    with pytest.raises(ValueError, match=r"labels\[2\] is 3"):
        bgzf.partition_records(_Unreadable(), [0, 1, 3, 9], outs)
    for n in (0, 1025):
        with pytest.raises(ValueError, match="1 to 1024 outputs"):
            bgzf.partition_records(_Unreadable(), [], ["x"] * n)
    with pytest.raises(ValueError, match="1 to 1024"):
        bgzf.partition_records(_Unreadable(), [1024], None)
    for kw in (dict(first_byte=b"@@"), dict(delimiter=b"ab"), dict(block_size=0), dict(record_lines=0), dict(record_lines=65)):
        with pytest.raises(ValueError):
            bgzf.partition_records(_Unreadable(), [0, 1], outs, **kw)
    for kw in (dict(match_line=1), dict(mismatches=1), dict(invert=True)):
        with pytest.raises(TypeError):
            bgzf.partition_records(_Unreadable(), [0, 1], outs, **kw)
    # demux_paired: a wrong count of outputs, of files' extras, a barcode file that is none of the files, duplicate patterns
    A, B = b"ACGTACGT", b"TTGTACGA"
    files = [_Unreadable(), _Unreadable()]
    for o in ([["a", "b"]], [["a", "b"], ["c"]], [["a"], ["b"]], [["a", "b"], ["c", "d"], ["e", "f"]], []):
        with pytest.raises(ValueError, match="one output per file and pattern"):
            bgzf.demux_paired(files, [A, B], o)
    good = [["a", "b"], ["c", "d"]]
    for kw in (dict(ambiguous=["x"]), dict(unassigned=["x", "y", "z"]), dict(ambiguous="one path"), dict(start=[0])):
        with pytest.raises(ValueError, match="one entry per file"):
            bgzf.demux_paired(files, [A, B], good, **kw)
    for b in (2, -1, None, 0.0, True):
        with pytest.raises(ValueError, match="barcode_file"):
            bgzf.demux_paired(files, [A, B], good, barcode_file=b)
    with pytest.raises(ValueError, match="duplicate"):
        bgzf.demux_paired(files, [A, A], good)
    with pytest.raises(ValueError, match="mismatches"):
        bgzf.demux_paired(files, [A, B], good, mismatches=8)
    with pytest.raises(ValueError):
        bgzf.demux_paired(["/nonexistent/r1", "/nonexistent/r2"], [A, B], good, record_lines=0)      # (judged before a file is opened)
    for name in ("partition_records", "demux_paired", "pair_labels", "DROP"):
        assert name in bgzf.__all__
    for name in ("partition_records", "demux_paired"):
        assert hasattr(bgzf.BgzfReader, name)


def test_symbols_declared_exported_and_bound():
    from zlib_ng_amd import _lib
    header = open(os.path.join(ROOT, "include", "zng_amd.h")).read()
    L = _lib.load()
    tail = ["uint64_t n_labels", "uint32_t n_classes", "uint64_t *class_records", "uint64_t *class_bytes", "zngamd_bgzf_partition_totals *totals"]
    for name, base, lab in (("zngamd_bgzf_partition_records_dev", "zngamd_bgzf_grep_records_dev", "const uint16_t *d_labels"),
                            ("zngamd_bgzf_partition_records", "zngamd_bgzf_grep_records", "const uint16_t *labels")):
        assert name in _lib.SYMBOLS and hasattr(L, name), name
        params = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1).split(",")]
        bparams = [re.sub(r"\s+", " ", x).strip() for x in re.search(r"\bint %s\s*\(([^;]*)\);" % base, header).group(1).split(",")]
        # the records call's parameters without the patterns and match_line; labels, class count and counts in front of the totals
        drop = {"const uint8_t *patterns", "uint32_t patterns_len", "const zngamd_bgzf_pattern *table", "uint32_t n_patterns", "int32_t match_line"}
        want = [x for x in bparams[:-1] if x not in drop] + [lab] + tail
        assert params == want, name
        keep = [i for i, x in enumerate(bparams[:-1]) if x not in drop]
        bt = getattr(L, base).argtypes
        assert getattr(L, name).argtypes == [bt[i] for i in keep] + [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p], name
    assert int(re.search(r"#define ZNGAMD_BGZF_PARTITION_MAX_CLASSES\s+(\d+)u", header).group(1)) == _lib.BGZF_PARTITION_MAX_CLASSES == 1024
    assert int(re.search(r"#define ZNGAMD_BGZF_PARTITION_DROP\s+0x([0-9A-Fa-f]+)u", header).group(1), 16) == _lib.BGZF_PARTITION_DROP == 0xFFFF
    size = int(re.search(r"\}\s*zngamd_bgzf_partition_totals;\s*/\* (\d+) B \*/", header).group(1))
    assert size == C.sizeof(_lib.BgzfPartitionTotals) == 7 * 8 + 4 * 4
    body = re.search(r"typedef struct \{([^}]*)\}\s*zngamd_bgzf_partition_totals;", header).group(1)
    fields = re.findall(r"\b(\w+);", re.sub(r"/\*.*?\*/", "", body))
    assert fields == [f[0] for f in _lib.BgzfPartitionTotals._fields_]
    assert _lib.BgzfPartitionTotals.covered.offset == 56 and _lib.BgzfPartitionTotals.labels_short.offset == 68
    assert int(re.search(r"#define ZNGAMD_ABI\s+(\d+)", header).group(1)) == L.zngamd_abi() == 6      # additions only
    assert L.zngamd_kernel_class_count() == len(_lib.K_NAMES) == 10                                     # no kernel class was added
    build = open(os.path.join(PKG_DIR, "build.py")).read()
    assert '"za_partition.hip"' in build and os.path.exists(os.path.join(PKG_DIR, "csrc", "za_partition.hip"))
    main = open(os.path.join(PKG_DIR, "csrc", "zng_amd.hip")).read()
    assert main.index('#include "za_classify.hip"') < main.index('#include "za_partition.hip"')


def test_entry_points_refuse_without_a_context():
    """ctx = NULL: ZNGAMD_E_ARG for every hostile class count, label array, record model, delimiter and flag -- and with everything in order"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    E_ARG = -202
    F, G = _lib.BGZF_GREP_FINAL, _lib.BGZF_CLASSIFY_GROUP
    lab = (C.c_uint16 * 4)(0, 1, 0xFFFF, 2)

    def call(form, n_classes=3, labels=lab, n_labels=4, delim=10, flags=F, rec=(4, 64), totals=True, counts=(True, True)):
        t = _lib.BgzfPartitionTotals()
        n = n_classes if 1 <= n_classes <= 1024 else 1
        cr, cb = (C.c_uint64 * n)(*[7] * n), (C.c_uint64 * n)(*[7] * n)
        tail = (labels, n_labels, n_classes, cr if counts[0] else None, cb if counts[1] else None, C.byref(t) if totals else None)
        head = (None, None, 0, None, 0, 0, 0, delim, flags, rec[0], rec[1], 0)
        if form == 0:
            r = L.zngamd_bgzf_partition_records(*head, None, None, 0, None, 0, _lib.ALLOC_FN(), None, *tail)
        else:
            r = L.zngamd_bgzf_partition_records_dev(*head, None, 0, None, None, 0, None, 0, *tail)
        assert list(cr) == [7] * n and list(cb) == [7] * n                     # a refused call writes nothing
        return r

    for form in range(2):
        for n in (0, 1025, 1 << 16, 0xFFFFFFFF):
            assert call(form, n_classes=n) == E_ARG, (form, n)
        assert call(form, labels=None, n_labels=4) == E_ARG and call(form, labels=None, n_labels=1 << 63) == E_ARG
        for rec in ((0, -1), (65, -1), (1 << 31, -1), (4, -2), (4, 256)):
            assert call(form, rec=rec) == E_ARG, (form, rec)
        assert call(form, delim=-1) == E_ARG and call(form, delim=256) == E_ARG
        for flags in (_lib.BGZF_GREP_INVERT, _lib.BGZF_GREP_LINE_START, _lib.BGZF_GREP_COUNT_ONLY, F | _lib.BGZF_GREP_LINE_START, G | 32, 64, 1 << 31):
            assert call(form, flags=flags) == E_ARG, (form, flags)
        assert call(form, totals=False) == E_ARG and call(form, counts=(False, True)) == E_ARG and call(form, counts=(True, False)) == E_ARG
        for flags in (0, F, G, F | G):                                         # (in order but for the context)
            assert call(form, flags=flags) == E_ARG and call(form, n_classes=1024, labels=None, n_labels=0, flags=flags) == E_ARG


class _FakePartitionCtx(_FakeClassifyCtx):
    """ctx.bgzf_partition_records computed on the host: the blocks through the system zlib, the rule by partition_ref"""

    def __init__(self):
        super().__init__()
        self.pcalls = []

    def bgzf_partition_records(self, data, members, text_off, text_end, delim, flags, k, first_byte, record_base, labels, n_classes, caps=None):
        from zlib_ng_amd import _lib
        assert not flags & ~(_lib.BGZF_GREP_FINAL | _lib.BGZF_CLASSIFY_GROUP) and labels.dtype == np.uint16
        data = bytes(data)
        buf = bytearray(int((members["out_off"] + members["out_len"]).max()) if len(members) else 0)
        for m in members:
            o, n = int(m["out_off"]), int(m["out_len"])
            buf[o:o + n] = zlib.decompress(data[int(m["in_off"]):int(m["in_off"] + m["in_len"])], -15)
        text, d = bytes(buf[text_off:text_end]), bytes([delim])
        final = bool(flags & _lib.BGZF_GREP_FINAL)
        lines = partition_ref.lines_of(text, d)
        if lines and not lines[-1].endswith(d) and not final:
            lines.pop()
        nrec = (len(lines) + k - 1) // k if final else len(lines) // k
        whole = b"".join(lines[:k * nrec])
        self.pcalls.append((record_base, len(labels), nrec, flags, labels.copy()))
        use = [partition_ref.DROP if x == 0xFFFF else int(x) for x in labels[:nrec].tolist()]
        short = len(use) < nrec
        use += [partition_ref.DROP] * (nrec - len(use))
        p = partition_ref.Partition(whole, use, n_classes, k, d)
        starts = np.concatenate([[0], np.cumsum([len(x) for x in p.records])]).astype(np.int64) + text_off
        tot = types.SimpleNamespace(seen=nrec, matched=nrec, bytes=sum(len(p.of_class(c)) for c in range(n_classes)), dropped=p.dropped,
                                    dropped_bytes=p.dropped_bytes, covered=1, bad=0, bad_record=0, bad_src=0, labels_short=int(short),
                                    tail_off=text_end if final else int(starts[nrec]), short_lines=len(lines) % k if final else 0)
        if first_byte >= 0:
            bad = [r for r in range(nrec) if p.records[r][0] != first_byte]
            if bad:
                tot.bad, tot.bad_record, tot.bad_src = 1, record_base + bad[0], int(starts[bad[0]])
        crec = np.array(p.counts, np.uint64)
        cbytes = np.array([len(p.of_class(c)) for c in range(n_classes)], np.uint64)
        st = np.zeros(len(members), np.int32)
        if tot.bad or short or not flags & _lib.BGZF_CLASSIFY_GROUP or nrec == p.dropped:
            return 0, st, tot, crec, cbytes, np.empty(0, _lib.GREP_ROW_DTYPE), b""
        order = np.array(p.order(), np.int64)
        rows = np.zeros(len(order), _lib.GREP_ROW_DTYPE)
        rows["src_off"], rows["number"], rows["len"] = starts[:-1][order], record_base + order, np.diff(starts)[order]
        rows["reserved"] = np.array(use)[order]
        return 0, st, tot, crec, cbytes, rows, b"".join(p.of_class(c) for c in range(n_classes))


def test_driver_on_a_fake_engine(monkeypatch):
    from zlib_ng_amd import _lib, bgzf
    barcodes = [b"ACGTACGTAC", b"TTGCATGCAA", b"GGATCCGGAT", b"CATGCATGTT"]
    recs = _reads(700, barcodes)
    data = b"".join(recs)
    BS = 997
    blob, blocks = _stored_bgzf(data, BS)
    coffs = sorted(blocks)
    fake = _FakePartitionCtx()
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)
    monkeypatch.setattr(bgzf, "BgzfWriter", _Collect)
    rng = np.random.default_rng(8)
    NC = 70                                              # more classes than a classification has
    labels = rng.integers(-1, NC, len(recs))
    labels[::11] = bgzf.DROP
    want = partition_ref.Partition(data, labels.tolist(), NC)
    assert want.dropped > 60 and min(want.counts) > 0
    starts = np.concatenate([[0], np.cumsum([len(x) for x in recs])])
    voff = lambda r: bgzf.make_virtual_offset(coffs[starts[r] // BS], int(starts[r] % BS))

    def part(labels, outputs, **kw):
        args = dict(first_byte=b"@", start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False)
        args.update(kw)
        return bgzf._partition_file(io.BytesIO(blob), fake, labels, outputs, 4, args["first_byte"], b"\n", 1, bgzf.MAX_BLOCK_INPUT, args["start"],
                                    args["stop"], args["first_record"], args["max_record"], args["allow_short"])

    for window in (32 << 20, 5000, 1500):
        monkeypatch.setattr(bgzf, "_READ_WINDOW", window)
        # every class to an output
        _Collect.made.clear()
        fake.pcalls.clear()
        counts = part(labels, ["o%d" % c for c in range(NC)])
        assert counts.dtype == np.int64 and counts.tolist() == want.counts + [want.dropped]
        made = {w.target: w for w in _Collect.made}
        assert len(made) == NC and all(w.closed and w.level == 1 for w in made.values())
        for c in range(NC):
            assert made["o%d" % c].got == want.of_class(c), (window, c)
        # the label offset advances with the records: every call is handed the labels from its first record on
        assert all(c[3] & _lib.BGZF_CLASSIFY_GROUP for c in fake.pcalls) and fake.pcalls[-1][3] & _lib.BGZF_GREP_FINAL
        at = 0
        for base, n_labels, nrec, flags, given in fake.pcalls:
            assert (base, n_labels) == (at, len(labels) - at) and np.array_equal(given, np.where(labels < 0, 0xFFFF, labels)[at:])
            at += nrec
        assert at == len(recs)
        if window == 32 << 20:
            assert len(fake.pcalls) == 1
        else:
            assert len(fake.pcalls) > 10
        # an output of None is counted and never gathered: the engine sees its records as DROP; outputs=None only counts
        _Collect.made.clear()
        fake.pcalls.clear()
        outs = [None if c % 3 == 0 else "o%d" % c for c in range(NC)]
        counts = part(labels, outs)
        assert counts.tolist() == want.counts + [want.dropped]
        quiet = np.isin(labels, [c for c in range(NC) if c % 3 == 0]) | (labels < 0)
        assert np.array_equal(fake.pcalls[0][4] == 0xFFFF, quiet)
        made = {w.target: w for w in _Collect.made}
        assert sorted(made) == sorted(o for o in outs if o) and all(made[o].got == want.of_class(c) for c, o in enumerate(outs) if o)
        fake.pcalls.clear()
        counts = part(labels, None)
        assert counts.tolist() == want.counts + [0] * (int(labels.max()) + 1 - NC) + [want.dropped]
        assert not any(c[3] & _lib.BGZF_CLASSIFY_GROUP for c in fake.pcalls)
        # start / stop / first_record: the labels belong to the records from first_record on
        a, b = 123, 500
        _Collect.made.clear()
        counts = part(labels[a:b], ["o%d" % c for c in range(NC)], start=voff(a), stop=voff(b), first_record=a)
        mid = partition_ref.Partition(b"".join(recs[a:b]), labels[a:b].tolist(), NC)
        assert counts.tolist() == mid.counts + [mid.dropped] and all(w.got == mid.of_class(int(w.target[1:])) for w in _Collect.made)
        # out of step, both ways, across windows: the message names both counts, the outputs are closed
        for n_labels in (len(recs) - 1, len(recs) - 300, len(recs) + 1, len(recs) + 300, 0):
            _Collect.made.clear()
            lab = np.resize(labels, n_labels) if n_labels else []
            with pytest.raises(ValueError, match=r"the file holds 700 records and labels has %d entries: the files are out of step.*incomplete" % n_labels):
                part(lab, ["o%d" % c for c in range(NC)])
            assert len(_Collect.made) == NC and all(w.closed for w in _Collect.made)
            with pytest.raises(ValueError, match=r"holds 700 records and labels has %d entries" % n_labels):
                part(lab, None)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1500)
    # a short last record
    cut = data[:data.rfind(b"\n", 0, len(data) - 1) + 1]                     # the last read without its quality line
    sblob, _ = _stored_bgzf(cut, BS)
    spart = lambda allow: bgzf._partition_file(io.BytesIO(sblob), fake, labels, None, 4, b"@", b"\n", 6, bgzf.MAX_BLOCK_INPUT, None, None, 0, 64 << 20, allow)
    with pytest.raises(ValueError, match=r"record 699, the last one, has 3 of 4 lines"):
        spart(False)
    assert spart(True).tolist()[:NC] == want.counts
    # a first_byte violation on the way: the outputs written so far are closed and the error says that they are incomplete
    lines = data.split(b"\n")
    del lines[4 * 600 + 2]
    bblob, _ = _stored_bgzf(b"\n".join(lines), BS)
    _Collect.made.clear()
    with pytest.raises(ValueError, match=r"record 601 at virtual offset \d+ does not start with b'@'.*partition_records.*incomplete"):
        bgzf._partition_file(io.BytesIO(bblob), fake, labels, ["o%d" % c for c in range(NC)], 4, b"@", b"\n", 6, bgzf.MAX_BLOCK_INPUT, None, None, 0,
                             64 << 20, True)
    assert len(_Collect.made) == NC and all(w.closed for w in _Collect.made) and 0 < sum(len(w.got) for w in _Collect.made) < len(data)


def test_demux_paired_on_a_fake_engine(monkeypatch):
    """the barcode file is classified and written in one pass; the mate follows its classes, window by window at its own pace"""
    from zlib_ng_amd import _lib, bgzf
    barcodes = [b"ACGTACGTAC", b"TTGCATGCAA", b"GGATCCGGAT", b"CATGCATGTT"]
    r1 = _reads(500, barcodes)
    r2 = [b"@r%d/2\n%s\n+\n%s\n" % (i, b"ACGT" * (1 + i % 9), b"F" * (4 * (1 + i % 9))) for i in range(500)]
    b1, _ = _stored_bgzf(b"".join(r1), 997)
    b2, _ = _stored_bgzf(b"".join(r2), 997)
    fake = _FakePartitionCtx()
    monkeypatch.setattr(bgzf, "MAX_BLOCK", 1100)
    monkeypatch.setattr(bgzf, "BgzfWriter", _Collect)
    monkeypatch.setattr(bgzf, "_READ_WINDOW", 1500)
    v = classify_ref.classify(b"".join(r1), b"\n", barcodes, 1, 4, 1)
    assert (v.counts > 0).all()
    mate = partition_ref.Partition(b"".join(r2), v.cls.tolist(), 6)

    def run(files, barcode_file, **kw):
        _Collect.made.clear()
        fake.calls.clear()
        fake.pcalls.clear()
        outs = [["f%d_%d" % (f, i) for i in range(4)] for f in range(2)]
        return bgzf._demux_paired_files([(io.BytesIO(x), fake) for x in files], barcodes, outs, 4, barcode_file, kw.get("ambiguous"),
                                        kw.get("unassigned"), 1, bgzf.MAX_BLOCK_INPUT, 1, b"@", b"\n", False, None, None, 0, 64 << 20, False, 1)

    for bf in (0, 1):
        files = [b1, b2] if bf == 0 else [b2, b1]
        counts = run(files, bf, ambiguous=["amb0", "amb1"], unassigned=[None, None])
        assert counts.tolist() == v.counts.tolist()
        made = {w.target: w for w in _Collect.made}
        assert len(made) == 10 and all(w.closed for w in made.values())
        assert len(fake.calls) > 10 and len(fake.pcalls) > 10 and all(c[3] & _lib.BGZF_CLASSIFY_GROUP for c in fake.calls)      # one pass, grouped
        for c in range(5):
            bname, mname = ("f%d_%d" % (bf, c), "f%d_%d" % (1 - bf, c)) if c < 4 else ("amb%d" % bf, "amb%d" % (1 - bf))
            assert made[bname].got == v.of_class(c) and made[mname].got == mate.of_class(c), (bf, c)
    # a mate that lost a read, and one that gained one
    for files, n in (([b1, _stored_bgzf(b"".join(r2[:250] + r2[251:]), 997)[0]], 499), ([b1, _stored_bgzf(b"".join(r2 + r2[:1]), 997)[0]], 501)):
        with pytest.raises(ValueError, match=r"the file holds %d records and labels has 500 entries: the files are out of step.*incomplete" % n):
            run(files, 0)
        assert len(_Collect.made) == 8 and all(w.closed for w in _Collect.made)


def test_hostile_arguments_under_asan_ubsan(tmp_path):
    """a stand-alone program, linked against the library's host side under the sanitizers and run as a plain child process"""
    import importlib.util
    clang = _hipcc_clang()
    if clang is None:
        pytest.skip("hipcc's clang is not on this host")
    spec = importlib.util.spec_from_file_location("zng_amd_build_asan", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = str(tmp_path / "libzng_amd_host_asan.so")
    mod.build_host_asan(so)
    exe = str(tmp_path / "partition_args")
    subprocess.check_call([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "partition_args.cpp"), "-o", exe, so,
                           "-Wl,-rpath," + str(tmp_path)])
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf partition arguments clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

"""The hand-built deflate streams of tests/deflate_build.py through the span decoder of the seek-point index (za_k_inflate_spans:
the sequential core with a 512-byte ring BEHIND a window of up to 32 KiB, stopped at a block header at any bit of a byte) and
through the index builder (gzip_index.build).  The expectations are the builder's own plaintext, its block_bits and the statuses
that the kernel's source gives for a table that is well formed but wrong -- never the engine's, never the oracle's output;
tests/test_cpu_span_vectors.py proves every span against the system zlib.  Each test makes a handful of launches, correct
tables before wrong ones.  A wrong table here changes CONTENT only: every span stays inside the buffers it is given."""
import io
import random
import struct
import zlib

import numpy as np
import pytest

import deflate_build as B
import span_tables as S

pytestmark = pytest.mark.gpu

INVALID_ROOM = 40000                              # more than any invalid vector produces in front of its defect
GAP = 64


@pytest.fixture(scope="module")
def old():
    return B.valid_vectors()


@pytest.fixture(scope="module")
def new():
    return B.span_vectors()


@pytest.fixture(scope="module")
def randoms():
    return [B.Vector("random_%d" % i, B.assemble(b), b"", B.replay(b)[0], b) for i, b in enumerate(B.random_block_streams())]


class E:
    """one table entry, free to be changed"""
    __slots__ = ("in_bit", "end_bit", "win_off", "out_off", "win_len", "out_len", "crc", "expect", "what")

    def copy(self, **kw):
        e = E()
        for k in self.__slots__:
            setattr(e, k, kw.get(k, getattr(self, k)))
        return e


def entries(spans, at=0, gap=0):
    """[E] of placed spans, their outputs one behind the other from `at` on with `gap` bytes between -> (entries, end)"""
    out = []
    for s in spans:
        e = E()
        e.in_bit, e.end_bit, e.win_off, e.win_len, e.crc = s.in_bit, s.end_bit, s.win_off, s.win_len, s.crc
        e.out_len = len(s.expect) if s.expect is not None else INVALID_ROOM
        e.expect, e.what, e.out_off = s.expect, (s.vec, s.first), at
        at += e.out_len + gap
        out.append(e)
    return out, at


def table(ents, order=None):
    from zlib_ng_amd import _lib
    tab = (_lib.Span * len(ents))()
    for j, k in enumerate(order if order is not None else range(len(ents))):
        e = ents[k]
        tab[j] = _lib.Span(e.in_bit, e.end_bit, e.win_off, e.out_off, e.win_len, e.out_len, e.crc, 0)
    return tab


def launch(ctx, p, ents, cap, order=None, windows=None):
    """one zngamd_inflate_spans call -> (status per entry, in the order of `ents`; the output).  Every entry is inside the
    buffers: checked HERE, on the host, so that no wrong table of a test reaches the device with a place outside them."""
    wins = p.windows if windows is None else windows
    for e in ents:
        assert e.in_bit <= e.end_bit and (e.end_bit + 7) // 8 + S.PAD <= len(p.data), e.what
        assert e.win_len <= S.WIN and e.win_off + e.win_len <= len(wins) and e.out_off + e.out_len <= cap, e.what
    order = list(range(len(ents))) if order is None else list(order)
    st, out = ctx.inflate_spans(p.data[:-S.PAD], table(ents, order), wins, cap)        # (the call pads the input itself)
    back = [0] * len(ents)
    for j, k in enumerate(order):
        back[k] = st[j]
    return back, out


def all_ok(ents, st, out, but=()):
    from zlib_ng_amd import _lib
    bad = [(e.what, s) for k, (e, s) in enumerate(zip(ents, st)) if k not in but and s != _lib.SPAN_OK]
    assert not bad, bad[:5]
    for k, e in enumerate(ents):
        if k not in but:
            assert out[e.out_off:e.out_off + e.out_len] == e.expect, e.what


# ---- whole vectors, at every lead ------------------------------------------------------------------------------------------------

def test_whole_vectors_as_spans(ctx, old, new):
    vs = old + [v for v in new if B.is_valid(v)]
    rng = np.random.default_rng(3)
    for lead in range(8):
        p = S.pack([(v, [0]) for v in vs], lead)
        assert {s.in_bit & 7 for s in p.spans} == {lead} and len(p.spans) == len(vs)
        ents, cap = entries(p.spans)
        order = rng.permutation(len(ents))
        offs = [ents[k].out_off for k in order]
        assert offs != sorted(offs)                                   # the outputs are not in the order of the table
        st, out = launch(ctx, p, ents, cap, order)
        all_ok(ents, st, out)


# ---- cut at every block ------------------------------------------------------------------------------------------------------------

CUT = ("blocks_1500", "hdr_every_bit", "stored_then_match", "empty_stored_between", "two_eob_only_blocks", "dist32768_at_32768")


def test_cut_at_every_block(ctx, old, new, randoms):
    by = {v.name: v for v in old + new}
    rnd = random.Random(11)
    empty, ends, starts = 0, set(), set()
    groups = [[by["hdr_every_bit"]], [by[n] for n in CUT if n != "hdr_every_bit"] + randoms]
    for lead, subset in ((5, False), (2, True)):
        for vs in groups:
            assert all(len(v.blocks) > 1 for v in vs if v.name in CUT)
            items = []
            for v in vs:
                n = len(v.blocks)
                items.append((v, sorted(rnd.sample(range(n), rnd.randint(1, n))) if subset else range(n)))
            p = S.pack(items, lead)
            ents, cap = entries(p.spans)
            assert len(ents) <= 6000
            st, out = launch(ctx, p, ents, cap)
            all_ok(ents, st, out)
            empty += sum(1 for e in ents if e.out_len == 0 and e.crc == 0)
            ends |= {s.end_bit & 7 for s in p.spans if not s.final}
            starts |= {s.in_bit & 7 for s in p.spans}
            assert b"".join(e.expect for e in ents) == b"".join(v.expect for v in vs)
    assert empty >= 10 and ends == set(range(8)) and starts == set(range(8)), (empty, ends, starts)


# ---- the device form: nothing outside a span's own output is written -------------------------------------------------------------

def test_guards_dev(ctx, new):
    from zlib_ng_amd import _lib, devmem
    by = {v.name: v for v in new}
    hdr = by["hdr_every_bit"]
    items = [(hdr, range(len(hdr.blocks)))] + [(v, [0]) for v in new if v.name.startswith("win_edges_")]
    p = S.pack(items, 6)
    ents, cap = entries(p.spans, at=GAP, gap=GAP)
    for e in ents:
        assert (e.end_bit + 7) // 8 + S.PAD <= len(p.data) and e.win_off + e.win_len <= len(p.windows) and e.out_off + e.out_len + GAP <= cap
    d_in = devmem.from_host(ctx, p.data)
    d_tab = devmem.from_host(ctx, bytes(table(ents)))
    d_win = devmem.from_host(ctx, p.windows)
    d_out = devmem.from_host(ctx, b"\xa5" * cap)
    d_st = devmem.from_host(ctx, b"\xff" * (4 * len(ents)))
    ctx.inflate_spans_dev(d_in.data_ptr(), len(p.data), d_tab.data_ptr(), len(ents), d_win.data_ptr(), len(p.windows), d_out.data_ptr(), cap,
                          d_st.data_ptr())
    st = d_st.cpu().view(np.int32)
    out = d_out.cpu().tobytes()
    all_ok(ents, list(st), out)
    at = 0
    for e in ents:                                                    # every gap, and what lies in front of the first span
        assert out[at:e.out_off] == b"\xa5" * (e.out_off - at), e.what
        at = e.out_off + e.out_len
    assert out[at:] == b"\xa5" * (cap - at) and cap - at == GAP


# ---- invalid streams ---------------------------------------------------------------------------------------------------------------

def test_invalid_streams(ctx, old, new):
    from zlib_ng_amd import _lib
    bad = [v for v, _ in B.invalid_vectors()] + [v for v in new if not B.is_valid(v)]
    good = [v for v in old + new if B.is_valid(v) and len(v.blob) < 1000]
    assert len(bad) >= 30 and sum(v.name.startswith("win_beyond_") for v in bad) == 4
    for lead in (0, 3):
        items = []
        for i, v in enumerate(bad):
            items += [(good[(7 * i) % len(good)], [0]), (v, [0])]
        p = S.pack(items, lead)
        ents, cap = entries(p.spans, gap=GAP)
        st, out = launch(ctx, p, ents, cap)
        refused = {k for k, e in enumerate(ents) if e.expect is None}
        assert len(refused) == len(bad)
        all_ok(ents, st, out, but=refused)
        wrong = [(ents[k].what[0], st[k]) for k in refused if st[k] != _lib.SPAN_DATA]
        assert not wrong, wrong


# ---- tables that are well formed but wrong -----------------------------------------------------------------------------------------

def _referenced_window_byte(v):
    """index into v.zdict of a byte that the first match with a source in the window copies"""
    op = 0
    for t in v.blocks[0].tokens:
        if isinstance(t, B.M):
            if t.dist > op:
                return len(v.zdict) + op - t.dist
            op += t.length
        else:
            op += 1
    raise AssertionError("no match reaches the window")


def test_wrong_tables(ctx, old, new):
    from zlib_ng_amd import _lib
    OK, DATA, LENGTH, CRC = _lib.SPAN_OK, _lib.SPAN_DATA, _lib.SPAN_LENGTH, _lib.SPAN_CRC
    by = {v.name: v for v in old + new}
    hv, lb, sm = by["hdr_every_bit"], by["long_block_into_window"], by["stored_then_match"]
    kind = lambda b: "empty" if (isinstance(b, B.Stored) and not b.data) or (not isinstance(b, B.Stored) and not b.tokens) else "data"
    assert kind(hv.blocks[31]) == kind(hv.blocks[95]) == "empty" and all(kind(hv.blocks[i]) == "data" for i in (5, 11, 12, 13, 30, 32, 94, 96))
    cuts = [0, 5, 12, 31, 32, 40, 95, 96, 100, 200, 1000, 3000, len(hv.blocks) - 1]
    edges = [by["win_edges_%d" % w] for w in B.EDGE_W]
    lead = 3
    p = S.pack([(hv, cuts), (lb, [0]), (sm, range(4))] + [(e, [0]) for e in edges], lead)
    base, size = entries(p.spans, gap=GAP)
    assert len(base) >= 16
    idx = {(e.what): k for k, e in enumerate(base)}
    hdr = [h + base[0].in_bit - lead for h in S._bits(hv, lead)[0]]            # every header of hdr_every_bit, absolute
    assert [hdr[c] for c in cuts] == [base[k].in_bit for k in range(len(cuts))]
    v5, v12, v40, vfin = idx[("hdr_every_bit", 5)], idx[("hdr_every_bit", 12)], idx[("hdr_every_bit", 40)], idx[("hdr_every_bit", cuts[-1])]
    vlb, vsm = idx[("long_block_into_window", 0)], idx[("stored_then_match", 1)]
    wins = bytearray(p.windows)

    def flipped_window(k, at):
        """the window of entry k once more, behind the others, with byte `at` flipped -> its offset"""
        off = len(wins)
        w = bytearray(wins[base[k].win_off:base[k].win_off + base[k].win_len])
        w[at] ^= 0x01
        wins.extend(w)
        return off

    # the correct table first, with the two changes that leave it correct: the end moved across a block that produces nothing
    # (an empty stored block, an end-of-block-only block), and a window longer than the span needs
    assert base[vsm].win_len == 8 and base[vsm].win_off >= 5
    right = [("as it is", 0, {}),
             ("end across an empty stored block", v12, dict(end_bit=hdr[32])),
             ("end across an end-of-block-only block", v40, dict(end_bit=hdr[96])),
             ("a longer window", vsm, dict(win_off=base[vsm].win_off - 5, win_len=13))]
    fin_end = S._bits(hv, lead)[1] + base[0].in_bit - lead
    assert fin_end & 7 and base[vfin].end_bit == (fin_end + 7) & ~7 and base[vfin].out_len == 0
    i_lb = _referenced_window_byte(lb)
    other = idx[("win_edges_32768", 0)]
    assert base[other].win_len == base[vlb].win_len == 32768 and lb.zdict != by["win_edges_32768"].zdict
    wrong = [("crc ^ 1", v12, dict(crc=base[v12].crc ^ 1), {CRC}),
             ("out_len + 1", v12, dict(out_len=base[v12].out_len + 1), {LENGTH}),
             ("out_len - 1", v12, dict(out_len=base[v12].out_len - 1), {LENGTH}),
             ("out_len - 1 of the long block", vlb, dict(out_len=base[vlb].out_len - 1), {LENGTH}),
             ("end = the header before", v12, dict(end_bit=hdr[30]), {LENGTH}),
             ("end = the next header", v5, dict(end_bit=hdr[13]), {LENGTH}),
             ("start = the next header", v12, dict(in_bit=hdr[13]), {LENGTH})]
    for d in (1, -1, 3, -3):
        wrong.append(("end %+d" % d, v5, dict(end_bit=base[v5].end_bit + d), {DATA, LENGTH}))
    for w in B.EDGE_W:
        k = idx[("win_edges_%d" % w, 0)]
        wrong.append(("window of %d without its oldest byte" % w, k, dict(win_off=base[k].win_off + 1, win_len=base[k].win_len - 1), {DATA}))
        wrong.append(("window of %d, first byte flipped" % w, k, dict(win_off=flipped_window(k, 0)), {CRC}))
    wrong += [("a referenced window byte flipped", vlb, dict(win_off=flipped_window(vlb, i_lb)), {CRC}),
              ("the window of another span", vlb, dict(win_off=base[other].win_off), {CRC}),
              ("a final end not rounded up", vfin, dict(end_bit=fin_end), {DATA})]

    def run(cases):
        ents, at = [], 0
        for name, k, change in [c[:3] for c in cases]:
            rep = [e.copy(out_off=e.out_off + at) for e in base]
            rep[k] = rep[k].copy(**change)
            ents += rep
            at += size + GAP
        st, out = launch(ctx, p, ents, at, windows=bytes(wins))
        return [(st[r * len(base):(r + 1) * len(base)], ents[r * len(base):(r + 1) * len(base)]) for r in range(len(cases))], out

    got, out = run(right)
    for (name, k, change), (st, ents) in zip(right, got):
        assert st[k] == OK, (name, st[k])
        all_ok(ents, st, out)
    got, out = run(wrong)
    seen = {}
    for (name, k, change, want), (st, ents) in zip(wrong, got):
        seen[name] = st[k]
        all_ok(ents, st, out, but={k})                               # every other span of the table: untouched by the wrong one
    print("statuses of the wrong tables:", seen)
    miss = {name: (seen[name], sorted(want)) for name, k, change, want in wrong if seen[name] not in want}
    assert not miss, miss


# ---- the index builder -----------------------------------------------------------------------------------------------------------

def _gz_member(raw, plain):
    return b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff" + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xFFFFFFFF)


def test_index_builder_on_handbuilt_members(ctx, old, new, randoms, tmp_path, monkeypatch):
    from zlib_ng_amd import gzip_index, gzip_ng, zlib_ng
    vs = [v for v in old + new if B.is_valid(v) and not v.zdict] + randoms[:50]
    names = {v.name for v in vs}
    assert {"hdr_every_bit", "blocks_1500", "stored_65535", "crc_fold_131072", "crc_fold_131073", "crc_fold_262149"} <= names
    rnd = random.Random(5)
    blob, plain, where = bytearray(), bytearray(), []                 # where: (first deflate byte, trailer byte, plaintext offset, vector)
    for i, v in enumerate(vs):
        where.append((len(blob) + 10, len(blob) + 10 + len(v.blob), len(plain), v))
        blob += _gz_member(v.blob, v.expect) + bytes(rnd.choice([0, 0, 0, 1, 5]))
        plain += v.expect
    blob, plain = bytes(blob), bytes(plain)
    path = str(tmp_path / "handbuilt.gz")
    with open(path, "wb") as f:
        f.write(blob)
    idx = gzip_index.build(path, spacing=4096)
    assert idx.size == len(plain)
    with open(path, "rb") as f:
        assert idx.decompress(f) == plain
        for _ in range(200):
            o, n = rnd.randrange(len(plain) + 50), rnd.choice([0, 1, 17, 300, 4096, 70000])
            assert idx.read_at(f, o, n) == plain[o:o + n], (o, n)
    with gzip_ng.open(path, "rb", index=idx) as g:
        for _ in range(100):
            o, n = rnd.randrange(len(plain) + 10), rnd.choice([1, 100, 4096, 100000])
            assert g.seek(o) == o and g.read(n) == plain[o:o + n], (o, n)
    # every point that the span kernel decodes from, against the builder: the bit is a block header, the window is the 32 KiB
    # of plaintext in front of it, the CRC is that of the plaintext slice, the end is the next header or the member's end
    inside = {}
    pts = idx.points
    for i, pt in enumerate(pts):
        if not pt.kernel:
            continue
        m = [w for w in where if w[0] * 8 <= pt.data_bit < w[1] * 8]
        assert len(m) == 1, (i, pt)
        first, trailer, pbase, v = m[0]
        hdr, end = B.block_bits(v.blocks, True, 8 * first)
        assert pt.data_bit in hdr, (v.name, i, pt.data_bit)
        blk = hdr.index(pt.data_bit)
        produced = sum(S.out_lens(v.blocks[:blk]))
        # (blocks that produce nothing share their output offset with the next header: the first of them is the point's block
        # unless the bit says otherwise, and the bit is what was looked up)
        assert pt.out_off == pbase + produced, (v.name, i)
        assert pt.span_crc == zlib.crc32(plain[pt.out_off:pt.out_off + pt.out_len]), (v.name, i)
        if pt.is_block:
            assert blk > 0 and pt.member_out == produced and pt.member_crc == zlib.crc32(v.expect[:produced]), (v.name, i)
            assert idx.window(i) == v.expect[max(0, produced - 32768):produced], (v.name, i)
            inside[v.name] = inside.get(v.name, 0) + 1
        else:
            assert blk == 0 and pt.win_len == 0 and pt.in_bit == 8 * (first - 10), (v.name, i)
        if pt.flags & gzip_index.F_FINAL:
            assert pt.end_bit == (end + 7) & ~7 == 8 * trailer and pt.out_off + pt.out_len == pbase + len(v.expect), (v.name, i)
        else:
            nxt = pts[i + 1]
            assert nxt.is_block and pt.end_bit == nxt.data_bit and pt.end_bit in hdr, (v.name, i)
    # spacing 4096: a call of the builder reads at most 4096 / ratio bytes, and span_vectors() asserts that this member's bytes
    # times its lowest ratio is more than ten times 4096
    assert inside.get("hdr_every_bit", 0) >= 8, inside
    # the windowed reader over the same file
    monkeypatch.setenv("ZNGAMD_READ_WINDOW", "65536")
    r = zlib_ng._GzipReader(io.BytesIO(blob))
    got = bytearray()
    while True:
        piece = r.read(rnd.choice([1, 100, 5000, 65536, 300000]))
        if not piece:
            break
        got += piece
    assert bytes(got) == plain

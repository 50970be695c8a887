"""The span vectors of tests/deflate_build.py and the span tables of tests/span_tables.py, proved on the CPU.  The referee is the
system zlib alone: every span that cutting a vector makes must be what zlib decodes from that span's blocks with that span's window
as its dictionary, and every invalid vector must be refused by zlib for its reason."""
import zlib

import pytest

import deflate_build as B
import span_tables as S


@pytest.fixture(scope="module")
def old_valid():
    return B.valid_vectors()


@pytest.fixture(scope="module")
def new():
    return B.span_vectors()


def as_vector(i, blocks):
    return B.Vector("random_%d" % i, B.assemble(blocks), b"", B.replay(blocks)[0], blocks)


def test_pins():
    """random_streams() is bit for bit what it was before random_stream_blocks was split off, and both give the same streams"""
    rs = B.random_streams()
    cb = ce = 0
    for blob, expect in rs:
        cb, ce = zlib.crc32(blob, cb), zlib.crc32(expect, ce)
    assert len(rs) == 300 and (cb, ce) == (0x024FA69D, 0x0D4F2551)
    for (blob, expect), blocks in zip(rs[:20], B.random_block_streams(n=20)):
        assert B.assemble(blocks) == blob and B.replay(blocks)[0] == expect


def test_block_bits(old_valid):
    for v in old_valid:
        hdr, end = B.block_bits(v.blocks)
        assert hdr[0] == 0 and end == B.end_bit(v.blocks) and (end + 7) // 8 == len(v.blob), v.name
        assert hdr == sorted(hdr) and len(hdr) == len(v.blocks)
        for start in (3, 8 * 5 + 7):
            h2, e2 = B.block_bits(v.blocks, True, start)
            w = B.BitWriter()
            w.bits(0, start)
            B.assemble(v.blocks, True, w)
            assert h2[0] == start and e2 == w.bitlen, (v.name, start)
    # `Fixed([33] + [200] * k)` moves the next header by 2..7, 0 and 1 bits
    assert [B.block_bits([B.Fixed([33] + [200] * k)], False)[1] % 8 for k in range(8)] == [2, 3, 4, 5, 6, 7, 0, 1]
    # the headers of the old chain fall on four bit positions only; those of the new one on all eight
    by = {v.name: v for v in old_valid}
    assert {h & 7 for h in B.block_bits(by["blocks_1500"].blocks)[0]} == {0, 2, 6, 7}


def test_the_new_vectors_hold_what_their_names_say(new, old_valid):
    names = [v.name for v in new]
    assert len(set(names)) == len(names) and not set(names) & {v.name for v in B.vectors()}
    valid = [v for v in new if B.is_valid(v)]
    assert names[:len(valid)] == [v.name for v in valid]                      # the valid ones first
    for w in B.EDGE_W:
        assert "win_edges_%d" % w in names
    assert {"win_beyond_%d" % w for w in (1, 511, 512, 32767)} | {"refill_beyond_100"} == {v.name for v in new if not B.is_valid(v)}
    assert {"refill_edge_%d" % w for w in B.REFILL_W} <= set(names)
    by = {v.name: v for v in new}
    hdr, end = B.block_bits(by["hdr_every_bit"].blocks)
    assert {h & 7 for h in hdr[:-1]} == set(range(8)) and 65536 <= (end + 7) // 8 <= 65536 + 64
    front, stored_at, ratio, nbytes = B.hdr_every_bit_census(by["hdr_every_bit"].blocks)
    assert {p for k, p in front if k == "fixed"} == {p for k, p in front if k == "dynamic"} == stored_at == set(range(8))
    assert nbytes * ratio / 4096 > 10
    c = B.long_block_counts(by["long_block_into_window"])
    assert c["tokens"] >= 6000 and c["in_window"] >= 200 and c["straddle"] >= 20 and c["far"] >= 200, c
    assert 3 * c["matches"] >= 0.9 * c["tokens"] and len(by["long_block_into_window"].blocks) == 1
    assert [len(by["crc_fold_%d" % n].expect) for n in (131072, 131073, 262149)] == [131072, 131073, 262149]
    assert max(len(v.blob) for v in new) <= 65536 + 64 and max(len(v.expect) for v in valid) == 262149
    # the first token of every win_edges_<w> reaches the window's first byte; its invalid twin is one further
    for w in (1, 511, 512):
        assert by["win_edges_%d" % w].blocks[0].tokens[0] == B.M(3, w)
        assert by["win_beyond_%d" % w].blocks[0].tokens[:2] == [B.M(3, w), B.M(3, 3 + w + 1)]
    assert by["win_beyond_32767"].blocks[0].tokens[0] == B.M(3, 32768) and len(by["win_beyond_32767"].zdict) == 32767


def test_new_vectors_whole(new):
    for v in new:
        d = zlib.decompressobj(-15, zdict=v.zdict) if v.zdict else zlib.decompressobj(-15)
        if B.is_valid(v):
            assert d.decompress(v.blob) == v.expect and d.eof and not d.unused_data, v.name
        else:
            with pytest.raises(zlib.error, match="too far back"):
                d.decompress(v.blob)


def _referee(v, cuts, start=0):
    """every span of the cut vector against zlib -> the spans"""
    cuts = sorted(set(cuts) | {0})
    spans = S.spans_of(v, cuts, start)
    assert len(spans) == len(cuts)
    hdr, end = B.block_bits(v.blocks, True, start)
    for s, a, b in zip(spans, cuts, cuts[1:] + [len(v.blocks)]):
        d = zlib.decompressobj(-15, zdict=s.window) if len(s.window) else zlib.decompressobj(-15)
        got = d.decompress(B.assemble(v.blocks[a:b], final=True))
        assert d.eof and got == s.expect, (v.name, a, b)
        assert s.crc == zlib.crc32(got) and s.final == (b == len(v.blocks)), (v.name, a)
        assert s.in_bit == hdr[a] and s.end_bit == (hdr[b] if b < len(hdr) else (end + 7) & ~7), (v.name, a)
    assert b"".join(bytes(s.expect) for s in spans) == v.expect, v.name       # the spans of one vector are its plaintext
    assert all(x.end_bit == y.in_bit for x, y in zip(spans, spans[1:]))
    return spans


def test_every_span_is_what_zlib_decodes(old_valid, new):
    empty, ends = 0, set()
    vs = old_valid + [v for v in new if B.is_valid(v)] + [as_vector(i, b) for i, b in enumerate(B.random_block_streams(n=100))]
    for v in vs:
        spans = _referee(v, range(len(v.blocks)))
        if len(v.blocks) > 1:
            empty += sum(1 for s in spans if not len(s.expect))
            ends |= {s.end_bit & 7 for s in spans if not s.final}
            _referee(v, range(0, len(v.blocks), 3), start=8 * 11 + 5)
        else:
            assert bytes(spans[0].window) == v.zdict[-S.WIN:] and bytes(spans[0].expect) == v.expect
    assert empty >= 10 and ends == set(range(8))


def test_pack(old_valid, new):
    """the buffers of pack() hold what spans_of says, at every lead"""
    by = {v.name: v for v in old_valid + new}
    items = [(by[n], range(len(by[n].blocks))) for n in ("stored_then_match", "win_edges_513", "empty_stored_between", "reach_start_zdict100")]
    for lead in range(8):
        p = S.pack(items, lead)
        assert p.data.endswith(bytes(S.PAD)) and {s.in_bit & 7 for s in p.spans if s.first == 0} == {lead}
        k = 0
        for v, cuts in items:
            first = p.spans[k]
            blob = p.data[first.in_bit // 8:]
            # zlib, from the byte the vector starts in: the lead bits are skipped by feeding a stream shifted back into place
            w = B.BitWriter()
            w.bits(0x55 & ((1 << lead) - 1), lead)
            B.assemble(v.blocks, True, w)
            assert blob.startswith(w.getvalue()), v.name
            for s in S.spans_of(v, cuts, first.in_bit):
                q = p.spans[k]
                assert (q.in_bit, q.end_bit, q.crc, q.final, q.expect) == (s.in_bit, s.end_bit, s.crc, s.final, bytes(s.expect))
                assert p.windows[q.win_off:q.win_off + q.win_len] == bytes(s.window) and q.vec == v.name
                assert (q.end_bit + 7) // 8 + S.PAD <= len(p.data)
                k += 1
        assert k == len(p.spans)

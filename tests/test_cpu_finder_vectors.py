"""CPU: the finder vectors of tests/deflate_build.py are what their names promise, proven before any GPU test uses them.  The system
zlib decodes every valid one to the builder's own plaintext and refuses every invalid one; what inflate_chunked_once demands of a
stream before it takes it (finder_gate) holds from the bytes, so that a bail-out on the GPU is a finding and not a badly built
vector; and the referee of the finder (tests/finder_ref.py) reports every non-final dynamic header the builder wrote, nothing in a
vector's last 64 bytes, and in the decoy vector hundreds of headers that are none -- all of them inside stored payloads."""
import gzip
import zlib

import pytest

import deflate_build as B
import finder_ref as R


@pytest.fixture(scope="module")
def vectors():
    return B.finder_vectors()


@pytest.fixture(scope="module")
def described(vectors):
    return {name: R.describe(name, v.blocks, v.blob) for name, v in vectors.items()}


def test_referee_on_streams_with_known_headers():
    """the referee against zlib's own output (every non-final dynamic header of a stream of many small blocks, and no other), against
    random bytes (survivors of phase A, none of phase B), and at the end of a buffer (12 bytes from the header's byte on)"""
    import numpy as np
    import deflate_walk as W
    inner = B.decoy_inner_stream()
    true = [b.start_bit for b in W.walk(inner).blocks if b.btype == 2 and not b.final]
    a, b = R.survivors(inner)
    assert b == true and len(true) >= 200 and set(b) <= set(a)
    assert R.candidates(inner, 0) == true and true[0] == 0 and R.candidates(inner[1:], 3)[:1] == [3]
    noise = np.random.default_rng(3).bytes(60000)
    a, b = R.survivors(noise)
    assert 100 < len(a) < 400 and b == []                              # about one offset in 2 300 passes phase A
    blk = B.finder_vectors()["finder_phase"].blocks[-2]
    for k in range(8):
        w = B.BitWriter()
        w.bits(0, k)
        blk.write(w, False)
        head = w.getvalue()
        assert len(head) > 12
        assert R.phase_a(head + bytes(4)) == [k] and R.phase_b(head + bytes(4), k), k
        assert R.phase_a(head[:12]) == [k] and R.phase_a(head[:11]) == [] and R.phase_a(b"\xff" + head[:11]) == []
        assert not R.phase_b(head[:30], k)                             # the code lengths run out of the buffer
        final = bytearray(head)
        final[0] |= 1 << k                                                # BFINAL set: not a boundary the finder may list
        assert R.phase_a(bytes(final) + bytes(4)) == []


def test_zlib_decodes_every_valid_vector_and_the_gate_is_open(vectors, described):
    for name, v in vectors.items():
        d = zlib.decompressobj(-15)
        assert d.decompress(v.blob) == v.expect and d.eof and d.unused_data == b"", name
        a, cands, chunks = described[name]
        assert B.finder_gate(v.blob, len(cands), chunks) == [], name
        assert sum(c[2] for c in chunks) == len(v.expect) and chunks[0][:2] == (0, 0), name
        # the referee finds every header the builder knows, and nothing where the kernel does not look
        true = set(B.true_dynamic_bits(v.blocks))
        assert true <= set(cands), (name, sorted(true - set(cands))[:5])
        assert R.tail_is_quiet(v.blob, a) and B.QUIET_TAIL >= R.TAIL + 16, name
        assert v.blob[-B.QUIET_TAIL:] == b"\xff" * B.QUIET_TAIL, name
        assert set(cands) - {0} <= set(a) and all(R.phase_b(v.blob, p) for p in cands[1:4]), name
        # as gzip members: the first deflate byte at offset 0, 1, 2, 3 mod 4; no sync marker comes from the framing
        for k in range(1, 5):
            m = B.gzip_member(v.blob, v.expect, k)
            assert (len(m) - 8 - len(v.blob)) % 4 == k - 1 and m.count(B.SYNC) == v.blob.count(B.SYNC), (name, k)
            if name != "finder_window" or k == 1:
                assert gzip.decompress(m) == v.expect, (name, k)


def test_phase_vector_census(vectors, described):
    v = vectors["finder_phase"]
    census = B.finder_phase_census(v.blocks)
    for h in B.FINDER_HCLENS:
        missing = [(bp, bit) for bp in range(4) for bit in range(8) if (bp, bit, h) not in census]
        assert not missing, (h, missing)
    assert min(B.FINDER_HCLENS) == 5 and max(B.FINDER_HCLENS) == 19
    # the header kinds phase B has branches of its own for, counted from the blocks themselves
    dyn = [b for b in v.blocks[:-1] if isinstance(b, B.Dynamic)]
    count = lambda f: sum(1 for b in dyn if f(b))
    assert count(lambda b: not any(b.d)) >= 8                                              # no distance code
    assert count(lambda b: sum(1 for x in b.d if x) == 1 and max(b.d) == 1) >= 16           # a one-code distance set
    assert count(lambda b: (b.hlit, b.hdist) == (29, 29)) >= 8
    assert count(lambda b: (b.hlit, b.hdist) == (1, 0) and b.d == [1]) >= 8                # 258 / 1
    assert count(lambda b: sum(1 for x in b.ll if x) == 1 and b.ll[256] == 1 and not b.tokens) >= 8      # end-of-block only
    def crosses(b):                                    # a 16 that repeats a literal/length entry's value into the distance lengths
        n = 0
        for s, e in b.clseq:
            run = {16: 3 + e, 17: 3 + e, 18: 11 + e}.get(s, 1)
            if s == 16 and n <= len(b.ll) < n + run:
                return True
            n += run
        return False
    assert count(crosses) >= 8
    # what the two finder mutations of the design notes would lose: headers at bit 7 of every byte phase, one-code distance sets
    hdr = B.true_dynamic_bits(v.blocks)
    assert {(h >> 3) & 3 for h in hdr if h & 7 == 7} == {0, 1, 2, 3}
    a, cands, chunks = described["finder_phase"]
    assert set(cands) - {0} == set(hdr), "the filler of this vector holds no false candidate"
    assert len(chunks) >= 4


def test_decoy_vector_headers_that_are_none(vectors, described):
    v = vectors["finder_decoy"]
    a, cands, chunks = described["finder_decoy"]
    true = set(B.true_dynamic_bits(v.blocks))
    unknown = [p for p in cands if p not in true and p != 0]
    assert len(unknown) >= 200
    payloads = B.stored_payload_bits(v.blocks)
    assert all(any(lo <= p < hi for lo, hi in payloads) for p in unknown)
    # the stream inside: complete, with a final block of its own, at least 200 non-final dynamic headers, all of them reported
    inner = B.decoy_inner_stream()
    at = v.blob.index(inner)
    d = zlib.decompressobj(-15)
    d.decompress(inner)
    assert d.eof
    import deflate_walk as W
    inner_true = [b.start_bit for b in W.walk(inner).blocks if b.btype == 2 and not b.final]
    assert len(inner_true) >= 200 and {8 * at + p for p in inner_true} <= set(unknown)
    # the copy of the stream's own stretch: its true headers once more, at the same bit phases
    hdr, _ = B.block_bits(v.blocks)
    stored = [i for i, b in enumerate(v.blocks) if isinstance(b, B.Stored)]
    first = stored[1] + 2                                                                  # text[2]: the stretch starts at its byte
    stretch = v.blob[hdr[first] >> 3:(hdr[stored[2]] + 7) >> 3]
    copy_at = v.blob.index(stretch, (hdr[stored[2]] >> 3) + 100)
    in_stretch = [h for h in sorted(true) if hdr[first] <= h < hdr[stored[2]]]
    assert len(in_stretch) >= 6
    assert {h - 8 * (hdr[first] >> 3) + 8 * copy_at for h in in_stretch} <= set(unknown)
    # a header in the last 20 bytes of a payload: its tokens are the blocks behind the stored block
    ends = [hi for lo, hi in payloads]
    assert any(hi - 160 <= p < hi for p in unknown for hi in ends)
    assert len(chunks) >= 4


def test_window_vector_chunks_and_edges(vectors, described):
    v = vectors["finder_window"]
    blocks, about = B.finder_window_blocks()
    a, cands, chunks = described["finder_window"]
    dyn = [i for i, b in enumerate(v.blocks[:-1]) if isinstance(b, B.Dynamic)]
    lens = B.block_out_lens(v.blocks)
    assert len(dyn) >= 130 and all(lens[i] >= B.WIN for i in dyn)
    assert len(v.blocks[0].data) + len(v.blocks[1].data) == 72 << 10
    # by the host's rule every dynamic block is a chunk of its own, behind the one chunk of the seed: more than two groups of 64
    assert len(chunks) == 1 + len(dyn) > 2 * 64 + 1
    hdr, _ = B.block_bits(v.blocks)
    assert [c[0] for c in chunks[1:]] == [hdr[i] for i in dyn]
    assert len(v.expect) // 4096 < B.WIN                                                    # (the target is 32 KiB, not total / 4096)
    # relay blocks: exactly 32 768 bytes, every one from distance 32 768
    relay = [v.blocks[i] for i in dyn[:len(dyn) - len(about)]]
    assert len(relay) >= 64
    for b in relay:
        assert [t.length for t in b.tokens] == [258] * 126 + [257, 3] and all(t.dist == B.WIN for t in b.tokens)
    # edge blocks: every p with every w, the probes where the name says, the odd lengths
    assert sorted((p, w) for p, w, _, _ in about) == sorted((p, w) for p in B.WINDOW_P for w in B.WINDOW_W)
    assert {t for _, _, t, _ in about} == {B.WIN} | set(B.WINDOW_ODD)
    for (p, w, total, at), i in zip(about, dyn[len(relay):]):
        toks, op, seen = v.blocks[i].tokens, 0, {}
        for k, t in enumerate(toks):
            if op == at["probe"] and "probe" not in seen and isinstance(t, B.M):
                assert (t, toks[k + 1]) == (B.M(3, w), B.M(258, w))
                seen["probe"] = True
            if op == at["overlap"] and t == B.M(258, 2):
                assert toks[k - 1] == B.M(3, B.WIN)                                        # two (three) marker bytes in front
                seen["overlap"] = True
            if op == at["straddle"] and isinstance(t, B.M) and t.dist == op + 100:
                assert t.length == 258                                                      # begins 100 bytes in front of the chunk, ends 158 bytes into it
                seen["straddle"] = True
            op += t.length if isinstance(t, B.M) else 1
        assert op == total == lens[i] and len(seen) == 3, (p, w, seen)
        assert at["probe"] == p and (at["straddle"] == 100 or p < 358)
    assert sum(1 for p, _, _, at in about if at["straddle"] == 100) >= 18
    assert len(v.blob) < 160 << 10 and 4 << 20 < len(v.expect) < 5 << 20


def test_invalid_forms_are_refused_by_zlib(vectors):
    plain = vectors["finder_phase"]
    for v in B.finder_invalid_vectors():
        assert len(v.blob) >= 65536 and v.blob.count(B.SYNC) == 0
        d = zlib.decompressobj(-15)
        with pytest.raises(zlib.error):
            d.decompress(v.blob)
        # the defect lies behind more than two chunks of the valid vector
        same = next(i for i, (x, y) in enumerate(zip(v.blob, plain.blob)) if x != y)
        chunks = R.describe("finder_phase", plain.blocks, plain.blob)[2]
        assert 8 * same > chunks[2][0], v.name


def test_resumed_vectors_and_their_cuts():
    for reach in B.FINDER_DICTS:
        v = B.finder_resumed_vector(reach)
        assert len(v.zdict) == reach and v.blocks[0].tokens[0] == B.M(3, reach)
        d = zlib.decompressobj(-15, v.zdict)
        assert d.decompress(v.blob) == v.expect and d.eof
        if reach != B.FINDER_DICTS[0]:
            continue
        for k in (1, 3, 7):
            hdr, end = B.block_bits(v.blocks, True, k)
            cuts = B.finder_cuts(v.blocks, k)
            assert len(set(cuts.values())) == 6 and all(65536 <= c < (end + 7) >> 3 for c in cuts.values()), cuts
            inside = lambda c: max(i for i, h in enumerate(hdr) if h < 8 * c)              # the block a cut falls in
            head_bits = lambda b: B.end_bit([B.Dynamic(b.ll, b.d, [], eob=False, clseq=b.clseq, cl=b.cl)], False)
            i = inside(cuts["in_tokens"])
            assert isinstance(v.blocks[i], B.Dynamic) and hdr[i] + head_bits(v.blocks[i]) < 8 * cuts["in_tokens"] < hdr[i + 1]
            i = inside(cuts["in_header"])
            assert isinstance(v.blocks[i], B.Dynamic) and 8 * cuts["in_header"] < hdr[i] + head_bits(v.blocks[i])
            i = inside(cuts["in_stored"])
            assert isinstance(v.blocks[i], B.Stored) and len(v.blocks[i].data) > 4096
            assert 8 * cuts["on_boundary"] in hdr and 8 * (cuts["behind_boundary"] - 1) in hdr
            assert 8 * (cuts["short_of_end"] + 1) == end

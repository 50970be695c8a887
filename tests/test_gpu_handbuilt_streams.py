"""The hand-built deflate streams of tests/deflate_build.py through every GPU decoder that foreign input can reach, each through an
existing entry point and each taking the whole vector list in a handful of launches.  The expectations are the builder's own
plaintext and the system zlib's verdict (tests/test_cpu_handbuilt_streams.py proves the two agree) -- never the engine's, never the
oracle's.  Verdicts: 1 = the stream ended, -3 = data error, -5 = wants more input / more room.

    za_k_inflate_serial_small     ctx.inflate_raw with in_len < 64 KiB and cap <= 512 KiB
    za_k_inflate_serial           ctx.inflate_raw with cap = 512 KiB + 1 (the chunk attempt finds no 8 boundaries), ctx.inflate_resume
    za_k_inflate_serial_members   ctx.bgzf_read with a member table; ctx.gunzip of the valid members as a BGZF file (tables of 9 / 8 bits)
    the batch kernel              ctx.inflate_batch(wbits=-15), with and without a dictionary; every proper prefix of the small vectors
    za_k_chunk_decode<512>        ctx.gunzip of ONE member of sync-delimited pieces: one pass (pieces of >= 8 KiB), count pass + tables
                                  of the two-pass branch (pieces of 3 KiB); markers that cross a chunk edge
    the streaming object          zlib_ng.decompressobj(-15) fed in halves and byte by byte
    za_k_inflate_spans            the span decoder of the seek-point index: tests/test_gpu_span_handbuilt.py
    za_k_find_blocks_a / _b       the block finder of a stream without sync points, za_k_chunk_count and the marker decoder behind it,
                                  compose / chain / resolve over more than two groups of chunks, ctx.inflate_resume at 64 KiB and more:
                                  tests/test_gpu_finder_handbuilt.py
The valid half of a decoder's vectors runs before its invalid half (two test functions)."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import deflate_build as B

pytestmark = pytest.mark.gpu

TAILS = (0, 1, 8, 64)
SMALL_IN, SMALL_CAP = 1 << 16, 512 << 10          # zngamd_inflate_raw: in_len < SMALL_IN and out_cap <= SMALL_CAP is the small call
INVALID_ROOM = 40000                              # more than any invalid vector produces in front of its defect


@pytest.fixture(scope="module")
def valid():
    return B.valid_vectors()


@pytest.fixture(scope="module")
def invalid():
    return [v for v, _ in B.invalid_vectors()]


@pytest.fixture(scope="module")
def randoms():
    return B.random_streams()


def _check(v, expect_code=1):
    """the builder's expectation against zlib's, once more where the test runs (cheap)"""
    d = zlib.decompressobj(-15, v.zdict) if v.zdict else zlib.decompressobj(-15)
    if expect_code == 1:
        assert d.decompress(v.blob) == v.expect and d.eof
    else:
        with pytest.raises(zlib.error):
            d.decompress(v.blob)


# ---- za_k_inflate_serial_small ------------------------------------------------------------------------------------------------------

def test_small_kernel_valid(ctx, valid, randoms):
    ctx.decode_paths(True)
    calls = 0
    # every vector but the stored block of 65535 bytes is a small call: in_len < 64 KiB and cap <= 512 KiB (that one takes the ordinary kernel)
    assert [v.name for v in valid if len(v.blob) + max(TAILS) >= SMALL_IN] == ["stored_65535"]
    for v in valid:
        _check(v)
        for tail in TAILS:
            blob, cap = v.blob + b"\xff" * tail, len(v.expect) + 64
            assert cap <= SMALL_CAP
            code, out, used, crc, ad = ctx.inflate_raw(blob, cap, v.zdict)
            calls += 1
            assert (code, used) == (1, len(v.blob)), (v.name, tail, code, used)
            assert out == v.expect, (v.name, tail)
            assert crc == zlib.crc32(v.expect) and ad == zlib.adler32(v.expect), (v.name, tail)
        # exactly the room the plaintext needs; one byte less is "no room", with every byte that fits
        code, out, used, _, _ = ctx.inflate_raw(v.blob, len(v.expect), v.zdict)
        calls += 1
        assert (code, out, used) == (1, v.expect, len(v.blob)), (v.name, "exact room", code)
        if v.expect:
            code, out, _, _, _ = ctx.inflate_raw(v.blob, len(v.expect) - 1, v.zdict)
            calls += 1
            assert code == -5 and out == v.expect[:-1], (v.name, "one byte less", code, len(out))
    for i, (blob, expect) in enumerate(randoms):
        code, out, used, _, _ = ctx.inflate_raw(blob, len(expect) + 64)
        calls += 1
        assert len(blob) < SMALL_IN and (code, used) == (1, len(blob)) and out == expect, (i, code)
    assert ctx.decode_paths(True) == {"indexed": 0, "bgzf": 0, "chunked": 0, "sequential": calls}


def test_small_kernel_invalid(ctx, invalid, valid):
    for v in invalid:
        _check(v, -3)
        assert len(v.blob) < SMALL_IN
        code, out, _, _, _ = ctx.inflate_raw(v.blob, INVALID_ROOM, v.zdict)
        assert code == -3, (v.name, code)
    # every proper prefix of a small valid vector wants more input, and has produced a prefix of the plaintext
    for v in valid:
        if len(v.blob) <= 30:
            for cut in range(len(v.blob)):
                code, out, _, _, _ = ctx.inflate_raw(v.blob[:cut], len(v.expect) + 64, v.zdict)
                assert code == -5 and v.expect.startswith(out), (v.name, cut, code)


# ---- za_k_inflate_serial ------------------------------------------------------------------------------------------------------------

def _behind_bits(v, k):
    """v's stream written behind a non-final fixed block that ends k bits into a byte -> (bytes from that byte on, k, end bit)"""
    w = B.BitWriter()
    B.assemble([B.Fixed([33] + [200] * ((k - 2) % 8))], False, w)
    start = w.bitlen
    assert start % 8 == k
    B.assemble(v.blocks, True, w)
    return w.getvalue()[start // 8:], k, w.bitlen - 8 * (start // 8)


def test_serial_kernel_valid(ctx, valid, randoms):
    cap = SMALL_CAP + 1
    ctx.decode_paths(True)
    calls = 0
    for v in valid:
        for tail in TAILS:
            code, out, used, crc, _ = ctx.inflate_raw(v.blob + b"\xff" * tail, cap, v.zdict)
            calls += 1
            assert (code, used) == (1, len(v.blob)), (v.name, tail, code, used)
            assert out == v.expect and crc == zlib.crc32(v.expect), (v.name, tail)
    for i, (blob, expect) in enumerate(randoms):
        code, out, used, _, _ = ctx.inflate_raw(blob, cap)
        calls += 1
        assert (code, used) == (1, len(blob)) and out == expect, (i, code)
    assert ctx.decode_paths(True) == {"indexed": 0, "bgzf": 0, "chunked": 0, "sequential": calls}
    # resumed at every bit offset 1..7
    for v in valid:
        for k in range(1, 8):
            data, start_bit, end = _behind_bits(v, k)
            code, out, in_bits, _, _ = ctx.inflate_resume(data, start_bit, v.zdict, len(v.expect) + 64)
            assert (code, in_bits) == (1, end), (v.name, k, code, in_bits, end)
            assert out == v.expect, (v.name, k)


def test_serial_kernel_invalid(ctx, invalid):
    for v in invalid:
        code, _, _, _, _ = ctx.inflate_raw(v.blob, SMALL_CAP + 1, v.zdict)
        assert code == -3, (v.name, code)
        for k in range(1, 8):
            data, start_bit, _ = _behind_bits(v, k)
            code, _, _, _, _ = ctx.inflate_resume(data, start_bit, v.zdict, INVALID_ROOM)
            assert code == -3, (v.name, "resumed", k, code)


# ---- za_k_inflate_serial_members ----------------------------------------------------------------------------------------------------

def _member(body, plain):
    """One BGZF member around a deflate body (the framing of test_gpu_inflate_parity._bgzf); the size field is 16 bits"""
    size = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04" + bytes(4) + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, (size - 1) & 0xFFFF) +
            body + struct.pack("<II", zlib.crc32(plain), len(plain)))


def _read_members(ctx, cases):
    """cases = [(body, plaintext or None)] as members of one bgzf_read call -> (statuses, the decoded bytes per case)"""
    from zlib_ng_amd import _lib
    data, members, slices, pos, acc, dst = [], [], [], 0, 0, 0
    for body, plain in cases:
        m = _member(body, plain or b"")
        room = len(plain) if plain is not None else INVALID_ROOM
        members.append(_lib.Member(pos + 18, len(body), acc, room, 0, 0, 0))
        if room:
            slices.append(_lib.BgzfSlice(acc, dst, room, 0))
        data.append(m)
        pos, acc, dst = pos + len(m), acc + room, dst + room
    status, sstat, out = ctx.bgzf_read(b"".join(data), (_lib.Member * len(members))(*members), (_lib.BgzfSlice * len(slices))(*slices), dst)
    got, k = [], 0
    for (body, plain), m in zip(cases, members):
        got.append(out[m.out_off:m.out_off + m.out_len] if m.out_len and sstat[k] == _lib.BGZF_SLICE_OK else b"")
        k += 1 if m.out_len else 0
    return status, got


def test_members_kernel_valid(ctx, valid, randoms):
    plain = [v for v in valid if not v.zdict]                 # (a member has no preset dictionary)
    cases = [(v.blob, v.expect) for v in plain] + list(randoms)
    status, got = _read_members(ctx, cases)
    for i, ((body, expect), st, out) in enumerate(zip(cases, status, got)):
        name = plain[i].name if i < len(plain) else "random %d" % (i - len(plain))
        assert st == 0, (name, st)
        assert out == expect, name
    # the same members as a BGZF file (all but the stored block of 65535 bytes: a BGZF block is 64 KiB at the most)
    fit = [(b, p) for b, p in cases if len(b) + 26 <= 65536]
    assert len(fit) == len(cases) - 1
    blob = b"".join(_member(b, p) for b, p in fit)
    want = b"".join(p for _, p in fit)
    assert gzip.decompress(blob) == want
    ctx.decode_paths(True)
    code, out, nm = ctx.gunzip(blob, len(want))
    assert (code, nm) == (0, len(fit)) and out == want
    assert ctx.decode_paths(True) == {"indexed": 0, "bgzf": len(fit), "chunked": 0, "sequential": 0}


def test_members_kernel_invalid(ctx, valid, invalid):
    from zlib_ng_amd import _lib
    good = [v for v in valid if not v.zdict and len(v.blob) < 1000]
    bad = [v for v in invalid if not v.zdict]
    cases = []
    for i, v in enumerate(bad):                                  # an invalid member between valid ones
        g = good[i % len(good)]
        cases += [(g.blob, g.expect), (v.blob, None)]
    status, got = _read_members(ctx, cases)
    for i, v in enumerate(bad):
        g = good[i % len(good)]
        assert status[2 * i] == 0 and got[2 * i] == g.expect, (g.name, status[2 * i])
        # the data error itself: the framing (room of INVALID_ROOM, trailer of no plaintext) would turn an ACCEPTED stream into a
        # length or CRC status, which is non-zero too
        assert status[2 * i + 1] == _lib.DATA_ERROR, (v.name, status[2 * i + 1])
    # a valid vector whose member says one byte less than it decodes to, or is cut one byte short, is refused too
    g = good[0]
    other = g.expect[:-1] + bytes([g.expect[-1] ^ 1])                   # (the third: the CRC-32 of another plaintext)
    status, _ = _read_members(ctx, [(g.blob, g.expect[:-1]), (g.blob[:-1], g.expect), (g.blob, other), (g.blob, g.expect)])
    assert status == [_lib.E_GZ_LENGTH, -5, _lib.E_GZ_CRC, 0], status             # (-5: the stream wants more input than the member has)


# ---- the batch kernel (za_batch.hip) ------------------------------------------------------------------------------------------------

def _batch(ctx, blobs, rooms, zdict=None):
    """one ctx.inflate_batch call of raw streams -> [(status, bytes, in_used)]"""
    from zlib_ng_amd import _lib
    n = len(blobs)
    items = (_lib.BatchItem * n)()
    pos = 0
    for k, (b, room) in enumerate(zip(blobs, rooms)):
        items[k].in_off, items[k].in_len, items[k].out_cap = pos, len(b), room
        pos += len(b)
    out, res = ctx.inflate_batch(b"".join(blobs), items, n, -15, zdict=zdict)
    return [(res[k].status, bytes(out[items[k].out_off:items[k].out_off + res[k].out_len]), res[k].in_used) for k in range(n)]


def _groups(vs):
    g = {}
    for v in vs:
        g.setdefault(v.zdict, []).append(v)
    return g


def test_batch_kernel_valid(ctx, valid, randoms):
    from zlib_ng_amd import _lib
    for zd, vs in _groups(valid).items():                     # one call without a dictionary, one per dictionary
        blobs = [v.blob + b"\xff" * t for v in vs for t in TAILS]
        got = _batch(ctx, blobs, [len(v.expect) + 16 for v in vs for t in TAILS], zd or None)
        for (v, t), (st, out, used) in zip([(v, t) for v in vs for t in TAILS], got):
            assert (st, used) == (_lib.BATCH_OK, len(v.blob)), (v.name, t, st, used)
            assert out == v.expect, (v.name, t)
    got = _batch(ctx, [b for b, _ in randoms], [len(e) + 16 for _, e in randoms])
    for i, ((blob, expect), (st, out, used)) in enumerate(zip(randoms, got)):
        assert (st, used) == (_lib.BATCH_OK, len(blob)) and out == expect, (i, st)
    # every proper prefix of every valid vector of up to 300 bytes: "truncated", and a prefix of the plaintext
    total = 0
    for zd, vs in _groups([v for v in valid if len(v.blob) <= 300]).items():
        cuts = [(v, c) for v in vs for c in range(len(v.blob))]
        got = _batch(ctx, [v.blob[:c] for v, c in cuts], [len(v.expect) + 16 for v, c in cuts], zd or None)
        for (v, c), (st, out, _) in zip(cuts, got):
            assert st == _lib.BATCH_TRUNCATED, (v.name, c, st)
            assert v.expect.startswith(out), (v.name, c)
        total += len(cuts)
    assert total > 1000


def test_batch_kernel_invalid(ctx, valid, invalid):
    from zlib_ng_amd import _lib
    good = _groups(valid)
    for zd, vs in _groups(invalid).items():
        mix = []
        for i, v in enumerate(vs):                               # invalid items between valid ones of the same dictionary
            mix += [v] + ([good[zd][i % len(good[zd])]] if zd in good else [])
        got = _batch(ctx, [v.blob for v in mix], [len(v.expect) + 16 if B.is_valid(v) else INVALID_ROOM for v in mix], zd or None)
        for v, (st, out, used) in zip(mix, got):
            if B.is_valid(v):
                assert (st, out, used) == (_lib.BATCH_OK, v.expect, len(v.blob)), (v.name, st)
            else:
                assert st == _lib.BATCH_DATA, (v.name, st)


# ---- za_k_chunk_decode: one member of sync-delimited pieces -------------------------------------------------------------------------

def _pieces(valid):
    """thirteen groups of blocks, each the start of one sync-delimited piece.  The vectors that reach the first byte of their
    dictionary reach into the pieces before them here; piece 5 BEGINS with a 258-match at distance 32768 and one at distance 1."""
    by = {v.name: v.blocks for v in valid}
    ends = [b for k in range(8) for b in by["ends_on_bit_%d" % k]]
    return [by["skew_ll_skew_dist"], by["one_bit_past_the_tables"], by["nlen286_ndist30"], by["length_codes_extra_all_ones_dynamic"],
            by["len258_both_spellings"], [B.Fixed([B.M(258, 32768), B.M(258, 1), 77, B.M(3, 32768), B.M(258, 32768, 284)])],
            by["reach_start_zdict32768"], by["two_eob_only_blocks"] + by["hclen5"], by["fixed_9bit_literals_dist29"],
            by["repeat_across_the_sets"] + by["zeros_138"] + by["no_distance_code"] + by["reach_start_zdict1"] + by["reach_start_zdict100"],
            by["skew_ll_onecode_dist"] + ends, by["blocks_1500"][:-1],
            by["stored_then_match"] + by["hclen19"] + by["nlen258_ndist1"] + by["length_codes_extra_all_ones"]]


def _piece_member(pieces, filler, check=True):
    """A gzip member: every piece's blocks, then `filler` incompressible bytes in a stored block and an empty stored block (the sync
    marker); an empty final block.  -> (member, plaintext or None)"""
    rng = np.random.default_rng(7)
    blocks = []
    for p in pieces:
        fill = rng.bytes(filler)
        assert b"\x00\x00\xff\xff" not in fill
        blocks += list(p) + [B.Stored(fill), B.Stored(b"")]
    blocks.append(B.Fixed([]))
    body = B.assemble(blocks)
    plain = B.replay(blocks)[0] if check else None
    return b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff" + body + struct.pack("<II", zlib.crc32(plain or b""), len(plain or b"")), plain


def _gunzip_counted(ctx, blob, room):
    """ctx.gunzip with the path counters and the launch counts of the call -> (code, bytes, members, decode paths, inflate scopes).
    Every decoding step of inflate_chunked_once is one profiled scope of the class `inflate`: the one-pass marker decode and
    windows + resolve are 2; count pass, marker decode, windows + resolve are 3; a one-pass decode that found anything odd and
    handed the stream to the two passes is 4.  So the count says which marker decoder produced the bytes."""
    ctx.decode_paths(True)
    ctx.profiling(True); ctx.kernel_times(True)
    try:
        code, out, nm = ctx.gunzip(blob, room)
        kt = ctx.kernel_times(True)
    finally:
        ctx.profiling(False)
    return code, out, nm, ctx.decode_paths(True), kt["inflate"][1]


def test_chunk_decoder_one_pass(ctx, valid, invalid):
    from zlib_ng_amd import _lib
    pieces = _pieces(valid)
    blob, plain = _piece_member(pieces, 10 << 10)
    assert gzip.decompress(blob) == plain
    # inflate_chunked_once: >= 8 sync points, none further than 2 MiB apart, and >= 8 KiB of input per boundary: the dense one-pass branch
    syncs = blob.count(b"\x00\x00\xff\xff")
    assert syncs >= 8 and len(blob) - 18 >= SMALL_IN and (len(blob) - 18) // (syncs + 1) >= 8 << 10
    code, out, nm, paths, scopes = _gunzip_counted(ctx, blob, len(plain))
    assert (code, nm) == (0, 1) and out == plain
    assert paths == {"indexed": 0, "bgzf": 0, "chunked": 1, "sequential": 0}
    assert scopes == 2, scopes                                  # the one-pass decode took every piece: no count pass, no second decode
    # the same member with an invalid vector in piece 7: the chunk path hands over, the sequential decoder refuses the member with
    # a data error (the trailer is never looked at: it is that of no plaintext)
    bad = {v.name: v.blocks for v in invalid}
    for name in ("unused_code_of_one_code_distance_set", "fixed_distance_code_30", "incomplete_distance_set"):
        broken, _ = _piece_member(pieces[:7] + [bad[name]] + pieces[8:], 10 << 10, check=False)
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(broken[10:])
        ctx.decode_paths(True)
        code, out, nm = ctx.gunzip(broken, len(plain) + 4096)
        assert code == _lib.DATA_ERROR and nm == 0, (name, code)
        assert ctx.decode_paths(True)["chunked"] == 0


def test_chunk_decoder_two_pass(ctx, valid):
    """pieces of 3 KiB: too small to be chunks as they are -- the count pass (za_k_chunk_count), chunks of >= 32 KiB of output merged
    from them, and the marker decoder with the tables of the two-pass branch"""
    pieces = [[]] * 12 + _pieces(valid) * 4                     # (12 pieces of filler first: the 32768-distances need their history)
    blob, plain = _piece_member(pieces, 3 << 10)
    assert gzip.decompress(blob) == plain
    syncs = blob.count(b"\x00\x00\xff\xff")
    assert len(blob) - 18 >= SMALL_IN and (len(blob) - 18) // (syncs + 1) < 8 << 10 and len(plain) >= 6 * (32 << 10)
    code, out, nm, paths, scopes = _gunzip_counted(ctx, blob, len(plain))
    assert (code, nm) == (0, 1) and out == plain
    assert paths == {"indexed": 0, "bgzf": 0, "chunked": 1, "sequential": 0}
    assert scopes == 3, scopes                                  # count pass, marker decode, windows + resolve: no one-pass attempt in front


def test_chunk_decoder_many_chunks(ctx, valid):
    """2100 pieces of 8 KiB: at 2049 chunks and more the one-pass branch takes the smallest marker decoder (za_k_chunk_decode<384>,
    tables of 9 / 8 index bits).  Every piece ends byte-aligned behind its sync marker, so the pieces are assembled one by one and
    joined as bytes; the plaintext is the system zlib's."""
    base = [p for p in _pieces(valid) if len(p) < 1000]          # (without the 1500 tiny blocks: 175 copies of them are 0.3 M blocks)
    rng = np.random.default_rng(11)
    fill = rng.bytes((8 << 10) + 64)
    assert b"\x00\x00\xff\xff" not in fill
    # a piece = its vectors' blocks, a stored block of filler, an empty stored block; the filler differs from piece to piece by its
    # first four bytes, so that a distance of 32768 never meets the bytes it would have met one piece later
    parts, npieces = [b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff"], 2100
    for i in range(npieces):
        w = B.BitWriter()
        B.assemble(([] if i < 4 else list(base[i % len(base)])) + [B.Stored(struct.pack("<I", 0x01010101 + i) + fill[4:]), B.Stored(b"")], False, w)
        assert w.bitlen % 8 == 0
        parts.append(w.getvalue())
    parts.append(B.assemble([B.Fixed([])]))
    body = b"".join(parts[1:])
    plain = zlib.decompressobj(-15).decompress(body)
    blob = parts[0] + body + struct.pack("<II", zlib.crc32(plain), len(plain))
    syncs = blob.count(b"\x00\x00\xff\xff")
    assert syncs + 1 >= 2049 and (len(blob) - 18) // (syncs + 1) >= 8 << 10       # ZNGAMD_CHUNKS_MANY_FROM chunks, the one-pass branch
    assert len(plain) > npieces * (8 << 10)
    code, out, nm, paths, scopes = _gunzip_counted(ctx, blob, len(plain))
    assert (code, nm) == (0, 1) and out == plain
    assert paths == {"indexed": 0, "bgzf": 0, "chunked": 1, "sequential": 0}
    assert scopes == 2, scopes                                  # all 2101 pieces decoded by the one pass: the stream never met the count pass


# ---- zlib_ng.decompressobj(-15) -----------------------------------------------------------------------------------------------------

def _feed(mod, v, pieces):
    """-> (verdict, bytes): 1 ended, -5 wants more, -3 raised"""
    d = mod.decompressobj(-15, v.zdict) if v.zdict else mod.decompressobj(-15)
    out = b""
    try:
        for p in pieces:
            out += d.decompress(p)
    except mod.error:
        return -3, out
    return (1 if d.eof else -5), out


def test_streaming_object(valid, invalid):
    from zlib_ng_amd import zlib_ng
    small = [v for v in valid + invalid if len(v.blob) <= 64]
    assert len(small) >= 30
    for v in valid + invalid:
        want = 1 if B.is_valid(v) else -3
        half = len(v.blob) // 2
        ways = [[v.blob[:half], v.blob[half:]]]
        if len(v.blob) <= 64:
            ways.append([v.blob[i:i + 1] for i in range(len(v.blob))])
        for pieces in ways:
            assert _feed(zlib, v, pieces)[0] == want, v.name          # (zlib itself, fed the same way)
            code, out = _feed(zlib_ng, v, pieces)
            assert code == want, (v.name, len(pieces), code)
            if want == 1:
                assert out == v.expect, (v.name, len(pieces))
        # a truncated stream does not raise: all but the last byte, in one piece and (small vectors) byte by byte
        if B.is_valid(v):
            cut = v.blob[:-1]
            for pieces in [[cut]] + ([[cut[i:i + 1] for i in range(len(cut))]] if len(cut) <= 64 else []):
                code, out = _feed(zlib_ng, v, pieces)
                assert code == -5 and v.expect.startswith(out), (v.name, len(pieces), code)
    # with a tail behind the end: the tail is unused_data
    for v in valid[:8]:
        d = zlib_ng.decompressobj(-15, v.zdict) if v.zdict else zlib_ng.decompressobj(-15)
        assert d.decompress(v.blob + b"\xff" * 8) == v.expect and d.eof and d.unused_data == b"\xff" * 8, v.name

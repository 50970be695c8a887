"""The finder vectors of tests/deflate_build.py through the chunk-parallel inflate of a stream WITHOUT sync points: the block finder
(za_k_find_blocks_a / _b), the count pass, the host's chain, the marker decoder behind a count pass, and compose / chain / resolve.
A header that the finder misses costs speed and never bytes, so the finder is held to account by zngamd_chunk_stats: its counts
must equal those of the referee (tests/finder_ref.py, written from RFC 1951 and zlib's rules) exactly.  The bytes are the builder's
own plaintext, which tests/test_cpu_finder_vectors.py proves against the system zlib; the engine's output is never an expectation.

    finder_phase    dynamic headers at every stream byte mod 4 x bit 0..7, for three HCLENs and the header kinds phase B branches on;
                    under four gzip headers, so that every phase meets every alignment of the kernel's dword loads
    finder_decoy    hundreds of valid headers inside stored payloads, a self-consistent chain of them among them
    finder_window   130 chunks and more of matches at distance 32 768, sources around a chunk's first byte and the 1 024-symbol ring
    resumed, cut    zngamd_inflate_resume at 64 KiB and more: the checkpoint it reports is one to continue from"""
import zlib

import pytest

import deflate_build as B
import finder_ref as R
from test_gpu_handbuilt_streams import SMALL_CAP, _behind_bits, _gunzip_counted

pytestmark = pytest.mark.gpu

CHUNKED = {"indexed": 0, "bgzf": 0, "chunked": 1, "sequential": 0}


@pytest.fixture(scope="module")
def vectors():
    return B.finder_vectors()


@pytest.fixture(scope="module")
def described(vectors):
    return {name: R.describe(name, v.blocks, v.blob) for name, v in vectors.items()}


def _raw_counted(ctx, body, cap):
    """ctx.inflate_raw with the path counters and the `inflate` scopes of the call (see _gunzip_counted)"""
    ctx.decode_paths(True)
    ctx.profiling(True); ctx.kernel_times(True)
    try:
        got = ctx.inflate_raw(body, cap)
        kt = ctx.kernel_times(True)
    finally:
        ctx.profiling(False)
    return got, ctx.decode_paths(True), kt["inflate"][1]


def _finder_counts(v, described):
    a, cands, chunks = described[v.name]
    return v.blob.count(B.SYNC), len(a), len(cands), len(chunks)


def _through_both_entries(ctx, v, described, name_lens):
    syncs, na, ncand, nchunks = _finder_counts(v, described)
    for k in name_lens:
        blob = B.gzip_member(v.blob, v.expect, k)
        assert blob.count(B.SYNC) == syncs
        ctx.chunk_stats()
        code, out, nm, paths, scopes = _gunzip_counted(ctx, blob, len(v.expect))
        stats = ctx.chunk_stats()
        assert (code, nm) == (0, 1), (v.name, k, code, nm)
        assert out == v.expect, (v.name, k)
        assert paths == CHUNKED and scopes == 3, (v.name, k, paths, scopes)          # count pass, marker decode, windows + resolve
        assert stats[:3] == (syncs, na, ncand), (v.name, k, stats, (syncs, na, ncand))
        assert stats[3] >= nchunks, (v.name, k, stats, nchunks)
    ctx.chunk_stats()
    (code, out, used, crc, _), paths, scopes = _raw_counted(ctx, v.blob, max(SMALL_CAP + 1, len(v.expect) + 64))
    stats = ctx.chunk_stats()
    assert (code, used) == (1, len(v.blob)), (v.name, code, used)
    assert out == v.expect and crc == zlib.crc32(v.expect), v.name
    assert paths == CHUNKED and scopes == 3, (v.name, paths, scopes)
    assert stats[:3] == (syncs, na, ncand) and stats[3] >= nchunks, (v.name, stats, (syncs, na, ncand, nchunks))


def test_phase_vector(ctx, vectors, described):
    _through_both_entries(ctx, vectors["finder_phase"], described, (1, 2, 3, 4))


def test_decoy_vector(ctx, vectors, described):
    v = vectors["finder_decoy"]
    assert _finder_counts(v, described)[2] > 200 + len(B.true_dynamic_bits(v.blocks))
    _through_both_entries(ctx, v, described, (1,))


def test_window_vector(ctx, vectors, described):
    v = vectors["finder_window"]
    chunks = described[v.name][2]
    blob = B.gzip_member(v.blob, v.expect, 1)
    ctx.chunk_stats()
    code, out, nm, paths, scopes = _gunzip_counted(ctx, blob, len(v.expect))
    stats = ctx.chunk_stats()
    assert (code, nm) == (0, 1) and len(out) == len(v.expect), (code, nm, len(out))
    if out != v.expect:
        at = next(i for i, (x, y) in enumerate(zip(out, v.expect)) if x != y)
        k = max(i for i, c in enumerate(chunks) if c[1] <= at)
        raise AssertionError("first wrong byte at %d: chunk %d of %d, offset %d of %d in it" % (at, k, len(chunks), at - chunks[k][1], chunks[k][2]))
    assert paths == CHUNKED and scopes == 3, (paths, scopes)
    assert stats[3] > 128 and stats[3] >= len(chunks), (stats, len(chunks))


def test_invalid_forms(ctx, vectors):
    from zlib_ng_amd import _lib
    room = len(vectors["finder_phase"].expect) + 4096
    for v in B.finder_invalid_vectors():
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(v.blob)
        blob = B.gzip_member(v.blob, b"", 1)
        ctx.decode_paths(True)
        ctx.chunk_stats()
        code, out, nm = ctx.gunzip(blob, room)
        assert code == _lib.DATA_ERROR and nm == 0, (v.name, code, nm)
        assert ctx.decode_paths(True)["chunked"] == 0, v.name
        assert ctx.chunk_stats()[3] == 0, v.name


# ---- zngamd_inflate_resume at 64 KiB and more ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def resumed():
    return {reach: B.finder_resumed_vector(reach) for reach in B.FINDER_DICTS}


def _checkpoint(ctx, v, data, start_bit, hdr, end, kept, room, want_chunks):
    """one ctx.inflate_resume call on data[:kept] and every claim its result makes; -> (code, out, in_bits, chunk_stats of the call)"""
    plain = v.expect
    offs = [0]
    for n in B.block_out_lens(v.blocks):
        offs.append(offs[-1] + n)
    ctx.chunk_stats()
    code, out, in_bits, bbits, bout = ctx.inflate_resume(data[:kept], start_bit, v.zdict, room)
    stats = ctx.chunk_stats()
    where = (v.name, start_bit, kept, room, code, in_bits, bbits, bout)
    assert out == plain[:len(out)], where
    assert bbits in hdr and bout == offs[hdr.index(bbits)], where
    assert len(out) >= bout, where
    # progress: the checkpoint is not in front of the last block that ends 64 bits or more before the cut (or the end of the room)
    done = [i for i in range(len(hdr)) if (hdr + [end])[i + 1] + 64 <= 8 * kept and offs[i + 1] <= room]
    if done:
        assert bbits >= hdr[done[-1]], where + (hdr[done[-1]],)
    if want_chunks:
        assert stats[3] >= 1, where + (stats,)
    # continuation: the whole stream from the checkpoint's byte on, with the 32 KiB in front of it as the dictionary
    hist = (v.zdict + plain[:bout])[-32768:]
    c2, out2, in2, _, _ = ctx.inflate_resume(data[bbits // 8:], bbits & 7, hist, len(plain) - bout + 64)
    assert (c2, in2) == (1, end - 8 * (bbits // 8)), where + (c2, in2)
    assert out2 == plain[bout:], where
    return code, out, in_bits, stats


@pytest.mark.parametrize("reach", B.FINDER_DICTS)
@pytest.mark.parametrize("k", (1, 3, 7))
def test_resumed_and_cut(ctx, resumed, k, reach):
    from zlib_ng_amd import _lib
    v = resumed[reach]
    data, start_bit, end = _behind_bits(v, k)
    hdr, end2 = B.block_bits(v.blocks, True, k)
    assert (start_bit, end) == (k, end2) and hdr[0] == k and len(data) == (end + 7) // 8
    room = len(v.expect) + 64
    code, out, in_bits, stats = _checkpoint(ctx, v, data, k, hdr, end, len(data), room, True)
    assert (code, in_bits) == (1, end) and out == v.expect, (code, in_bits, end)
    # the finder lists the start bit and at least every non-final dynamic header the builder wrote (none is in the last 16 bytes)
    true = [h for h, b in zip(hdr[:-1], v.blocks[:-1]) if isinstance(b, B.Dynamic)]
    assert stats[0] == 0 and stats[2] >= len(true) + 1 and stats[1] >= stats[2] - 1, (stats, len(true))
    for what, kept in B.finder_cuts(v.blocks, k).items():
        code, out, in_bits, _ = _checkpoint(ctx, v, data, k, hdr, end, kept, room, kept >= 65536)
        assert code in (_lib.BUF_ERROR, 0) and in_bits <= 8 * kept, (what, code, in_bits)


def test_resumed_with_room_for_100000_bytes(ctx, resumed):
    from zlib_ng_amd import _lib
    v = resumed[B.FINDER_DICTS[0]]
    data, k, end = _behind_bits(v, 3)
    hdr, _ = B.block_bits(v.blocks, True, k)
    code, out, in_bits, _ = _checkpoint(ctx, v, data, k, hdr, end, len(data), 100000, False)
    assert code == _lib.E_OVERFLOW and out == v.expect[:100000], (code, len(out))

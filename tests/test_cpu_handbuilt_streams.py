"""The hand-built deflate streams of tests/deflate_build.py, proved on the CPU: the system zlib, fed the whole input in one call, is
the referee for every vector (bytes, end, consumed length, and for an invalid stream the REASON it is refused); deflate_walk is a
second witness of the builder; and the oracle, which the GPU suites compare the kernels with, must give zlib's verdict on all of it
-- 1 (stream end), -3 (data error), -5 (out of input) -- with zlib's bytes and consumed length."""
import zlib

import pytest

import deflate_build as B
import deflate_walk as W

TAILS = (0, 1, 8, 64)


@pytest.fixture(scope="module")
def valid():
    return B.valid_vectors()


@pytest.fixture(scope="module")
def invalid():
    return B.invalid_vectors()


@pytest.fixture(scope="module")
def randoms():
    return B.random_streams()


def zlib_verdict(blob, zdict=b""):
    """zlib on the whole input in one call -> (code, bytes, consumed, message): 1 = ended, -5 = wants more input, -3 = refused"""
    d = zlib.decompressobj(-15, zdict) if zdict else zlib.decompressobj(-15)
    try:
        out = d.decompress(blob)
    except zlib.error as e:
        return -3, None, None, str(e)
    if d.eof:
        return 1, out, len(blob) - len(d.unused_data), ""
    return -5, out, len(blob), ""


def test_the_list_holds_what_it_should(valid, invalid):
    names = [v.name for v in valid] + [v.name for v, _ in invalid]
    assert len(set(names)) == len(names)
    assert all(B.is_valid(v) for v in valid) and not any(B.is_valid(v) for v, _ in invalid)
    assert [v.name for v in B.vectors()] == names
    assert {"ends_on_bit_%d" % k for k in range(8)} <= set(names)
    assert max(len(v.blob) for v in valid) == 65540                              # the stored block of 65535 bytes is the largest vector


def test_valid_vectors_are_what_zlib_decodes(valid):
    for v in valid:
        for tail in TAILS:
            code, out, used, msg = zlib_verdict(v.blob + b"\xff" * tail, v.zdict)
            assert code == 1, (v.name, tail, code, msg)
            assert out == v.expect, (v.name, tail)
            assert used == len(v.blob), (v.name, tail, used)


def test_invalid_vectors_are_refused_for_their_reason(invalid):
    for v, phrase in invalid:
        code, _, _, msg = zlib_verdict(v.blob, v.zdict)
        assert code == -3, (v.name, code)
        assert phrase in msg, (v.name, msg)


def test_the_distance_one_beyond_is_the_valid_one_plus_one(valid, invalid):
    """the `reach_start` vectors and their invalid twins differ by ONE in the distance"""
    good = {v.name: v for v in valid}
    bad = {v.name: v for v, _ in invalid}
    assert good["reach_start_zdict1"].blocks[0].tokens[0] == B.M(4, 1) and len(good["reach_start_zdict1"].zdict) == 1
    assert good["reach_start_zdict32768"].blocks[0].tokens[0].dist == len(good["reach_start_zdict32768"].zdict) == 32768
    assert len(bad["distance_beyond_zdict32767"].zdict) == 32767 and len(bad["distance_32768_at_32767"].blocks[0].data) == 32767
    assert len(good["dist32768_at_32768"].blocks[0].data) == 32768


def test_random_streams_are_what_zlib_decodes(randoms):
    assert len(randoms) == 300
    kinds = set()
    for i, (blob, expect) in enumerate(randoms):
        assert len(blob) <= 8192 and len(expect) <= 40 * 1024
        code, out, used, msg = zlib_verdict(blob)
        assert (code, used) == (1, len(blob)), (i, code, msg)
        assert out == expect, i
        kinds |= set(W.walk(blob).btypes)
    assert kinds == {0, 1, 2}


def test_walker_sees_the_same_tokens(valid):
    for v in valid:
        w = W.walk(v.blob, v.zdict)
        assert w.final and w.out == v.expect, v.name
        assert w.btypes == [b.btype for b in v.blocks], v.name
        assert w.matches == B.replay(v.blocks, v.zdict)[1] and len(w.matches) == B.match_count(v.blocks), v.name
        assert (w.end_bit + 7) // 8 == len(v.blob), v.name


def _oracle_vs_zlib(O, blob, zdict, cap, what):
    code, out, used, msg = zlib_verdict(blob, zdict)
    ocode, oout, oused = O.inflate_raw(blob, cap, zdict)
    assert ocode == code, (what, ocode, code, msg)
    if code != -3:
        assert oout == out, what
    if code == 1:
        assert oused == used, (what, oused, used)
    return code


def test_oracle_gives_zlibs_verdict(valid, invalid, randoms):
    from oracle import oracle as O
    for v in valid:
        for tail in TAILS:
            assert _oracle_vs_zlib(O, v.blob + b"\xff" * tail, v.zdict, len(v.expect) + 16, (v.name, tail)) == 1
    for v, _ in invalid:
        assert _oracle_vs_zlib(O, v.blob, v.zdict, 70000, v.name) == -3
    for i, (blob, expect) in enumerate(randoms):
        assert _oracle_vs_zlib(O, blob, b"", len(expect) + 16, i) == 1


def test_oracle_on_every_prefix(valid, invalid):
    """A proper prefix of a valid stream is never an error and never an end: zlib and the oracle want more input and have produced
    the same prefix of the plaintext.  A prefix of an INVALID stream is refused as soon as the defect's own bits are there, and
    wants more input before that: the oracle takes either verdict where zlib does."""
    from oracle import oracle as O
    n = 0
    for v in valid:
        if len(v.blob) > 300:
            continue
        for cut in range(len(v.blob)):
            assert _oracle_vs_zlib(O, v.blob[:cut], v.zdict, len(v.expect) + 16, (v.name, cut)) == -5
            n += 1
    assert n > 1000
    for v, _ in invalid:
        if len(v.blob) > 300:
            continue
        codes = [_oracle_vs_zlib(O, v.blob[:cut], v.zdict, 70000, (v.name, cut)) for cut in range(len(v.blob) + 1)]
        assert codes[-1] == -3 and codes[0] == -5 and 1 not in codes
        assert codes == sorted(codes), v.name                                    # once refused, refused with every byte more

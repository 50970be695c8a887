"""The DEFLATE token walker of the strategy tests (tests/deflate_walk.py), checked against CPython's zlib without a GPU: the
structural properties the GPU tests demand of each strategy hold for the system zlib's own streams, and the walker's literal /
match expansion reproduces the input."""
import os
import random
import zlib

import pytest

import deflate_walk as W

STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY,
              "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


def run_heavy(n, seed=7):
    """random bytes, each repeated 1..400 times"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += bytes([rng.randrange(256)]) * rng.randint(1, 400)
    return bytes(out[:n])


@pytest.fixture(scope="module")
def inputs(fastq):
    return {"fastq": fastq[:200_000], "runs": run_heavy(200_000)}


def _raw(data, level, strategy):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


@pytest.mark.parametrize("name", ["fastq", "runs"])
@pytest.mark.parametrize("strategy", sorted(STRATEGIES))
def test_walker_expands_zlib_streams(inputs, name, strategy):
    data = inputs[name]
    w = W.walk(_raw(data, 6, STRATEGIES[strategy]))
    assert w.final and w.out == data


@pytest.mark.parametrize("name", ["fastq", "runs"])
def test_huffman_only_has_no_matches(inputs, name):
    w = W.walk(_raw(inputs[name], 6, zlib.Z_HUFFMAN_ONLY))
    assert w.matches == [] and W.check_strategy(w, zlib.Z_HUFFMAN_ONLY) is None


@pytest.mark.parametrize("name", ["fastq", "runs"])
def test_rle_has_distance_one_only(inputs, name):
    w = W.walk(_raw(inputs[name], 6, zlib.Z_RLE))
    assert all(d == 1 and 3 <= ln <= 258 for ln, d in w.matches)
    assert W.check_strategy(w, zlib.Z_RLE) is None
    if name == "runs":
        assert len(w.matches) > 100


@pytest.mark.parametrize("name", ["fastq", "runs"])
def test_fixed_has_no_dynamic_block(inputs, name):
    w = W.walk(_raw(inputs[name], 6, zlib.Z_FIXED))
    assert 2 not in w.btypes and W.check_strategy(w, zlib.Z_FIXED) is None


@pytest.mark.parametrize("name", ["fastq", "runs"])
def test_filtered_has_no_short_match(inputs, name):
    if not zlib.ZLIB_RUNTIME_VERSION.startswith("1."):
        pytest.skip("the Z_FILTERED rule (match_length <= 5 dropped) is zlib 1.x's deflate_slow; this zlib is %s" % zlib.ZLIB_RUNTIME_VERSION)
    w = W.walk(_raw(inputs[name], 6, zlib.Z_FILTERED))
    assert w.matches and min(ln for ln, _ in w.matches) >= 6
    assert W.check_strategy(w, zlib.Z_FILTERED) is None


def test_checker_catches_default_streams(inputs):
    """the checks have teeth: a default-strategy stream fails every one of them"""
    w = W.walk(_raw(inputs["fastq"], 6, zlib.Z_DEFAULT_STRATEGY))
    for s in (zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED, zlib.Z_FILTERED):
        assert W.check_strategy(w, s) is not None


def test_walker_with_window_and_sync_flush():
    zd = os.urandom(1000)
    data = zd[100:600] * 3 + b"tail"
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, 0, zd)
    s = c.compress(data[:700]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(data[700:]) + c.flush()
    w = W.walk(s, window=zd)
    assert w.out == data and w.btypes.count(0) >= 1
    assert max(d for _, d in w.matches) > 600


def test_strip_container():
    data = b"abc" * 1000
    for wb in (-15, 9, 15, 25, 31):
        c = zlib.compressobj(6, zlib.DEFLATED, wb)
        assert W.walk(W.strip_container(c.compress(data) + c.flush(), wb)).out == data

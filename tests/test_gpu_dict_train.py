"""The batch API's dictionary trainer on the GPU (batch.train_dict / train_dict_dev, za_dict.hip): byte parity with the reference of
DESIGN.md section 5c.2 (tests/dict_train_ref.py) over sample counts, sizes, k, d and dict_size; the host and device forms and a repeated
call agree; the quality gate through the engine's own compressor; round trips through the batch API and CPython's zlib; a hostile
device item table."""
import random
import zlib

import numpy as np
import pytest

import dict_train_ref as R
from test_cpu_dict_train import gate_cases, zlib_total

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from zlib_ng_amd import _lib, batch, corpus, devmem
    return _lib, batch, corpus, devmem


def _cut(data, n, rng, odd=False):
    """data cut into n samples at random points; odd: empty and sub-d samples mixed in"""
    cuts = sorted(rng.sample(range(1, len(data)), n - 1)) if n > 1 else []
    out = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
    if odd:
        for i in range(0, len(out), 7):
            out.insert(i, b"" if i % 2 else data[i:i + (i % 4)])
    return out


def _case(corpus, name):
    rng = random.Random(name)
    if name == "one_sample_k_bytes":
        return [corpus.text(256, seed=1).tobytes()], 32768, 256, 8
    if name == "ten_d4_dict_d":
        return _cut(corpus.text(4000, seed=2).tobytes(), 10, rng), 4, 8, 4
    if name == "thousand_d6":
        return _cut(corpus.text(200000, seed=3).tobytes(), 1000, rng, odd=True), 1000, 64, 6
    if name == "hundred_thousand_8mib":
        return _cut(corpus.text(8 << 20, seed=4).tobytes(), 100000, rng), 32768, 256, 8
    if name == "k1024_odd":
        return _cut(corpus.mixed(2 << 20, seed=5).tobytes(), 3000, rng, odd=True), 32768, 1024, 8
    if name == "k16384":
        return _cut(corpus.text(3 << 20, seed=6).tobytes(), 500, rng), 32768, 16384, 8
    if name == "hot_hash":
        t = corpus.text(1 << 20, seed=7).tobytes()
        return _cut(t[:300000] + b"\0" * (1 << 20) + b"ab" * 200000 + t[300000:], 2000, rng), 32768, 256, 4
    if name == "below_dict_size":
        return _cut(corpus.text(5000, seed=8).tobytes(), 30, rng, odd=True), 32768, 64, 4
    if name == "d6_multi_epoch":
        return _cut(corpus.fastq(4 << 20, seed=9).tobytes(), 20000, rng), 32768, 256, 6
    if name == "k8_d8":
        return _cut(corpus.text(300000, seed=10).tobytes(), 100, rng, odd=True), 1000, 8, 8
    raise KeyError(name)


CASES = ["one_sample_k_bytes", "ten_d4_dict_d", "thousand_d6", "hundred_thousand_8mib", "k1024_odd", "k16384", "hot_hash",
         "below_dict_size", "d6_multi_epoch", "k8_d8"]


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(mods, name):
    _lib, batch, corpus, devmem = mods
    samples, dict_size, k, d = _case(corpus, name)
    want = R.train(samples, dict_size, k=k, d=d)
    got = batch.train_dict(samples, dict_size, k=k, d=d)
    assert len(got) <= dict_size
    assert got == want, (name, len(got), len(want))


def _dev_form(ctx, devmem, samples, gap=0):
    """the samples in one device buffer (gap bytes of 0xEE between them), -> (buffer, offsets, lengths)"""
    blob, offs = bytearray(), []
    for s in samples:
        offs.append(len(blob))
        blob += s + b"\xee" * gap
    d_in = devmem.from_host(ctx, bytes(blob) + bytes(64))
    return d_in, offs, [len(s) for s in samples]


@pytest.mark.parametrize("name", ["thousand_d6", "k1024_odd", "hot_hash"])
def test_host_and_device_forms_agree(mods, ctx, name):
    _lib, batch, corpus, devmem = mods
    samples, dict_size, k, d = _case(corpus, name)
    host = batch.train_dict(samples, dict_size, k=k, d=d)
    d_in, offs, lens = _dev_form(ctx, devmem, samples, gap=5)
    dev = batch.train_dict_dev(ctx, d_in, offs, lens, dict_size, k=k, d=d)
    assert dev == host
    assert batch.train_dict(samples, dict_size, k=k, d=d) == host          # a second call
    # samples in another order than they lie in the buffer: the table's order is the samples' order
    order = list(range(len(samples)))[::-1]
    rev = batch.train_dict_dev(ctx, d_in, [offs[i] for i in order], [lens[i] for i in order], dict_size, k=k, d=d)
    assert rev == batch.train_dict([samples[i] for i in order], dict_size, k=k, d=d)


@pytest.mark.parametrize("case", range(6))
def test_quality_gate_engine(mods, case):
    """the trained dictionary against the naive first 32 KiB, both through batch.compress: measured margins 4.3-21 % through
    CPython's zlib (test_cpu_dict_train), and the engine's own parse keeps at least 3 %"""
    _lib, batch, corpus, devmem = mods
    name, rec, samples, records, naive = gate_cases()[case]
    trained = batch.train_dict(samples)
    assert trained == R.train(samples)
    t = sum(len(x) for x in batch.compress(records, 6, zdict=trained))
    nv = sum(len(x) for x in batch.compress(records, 6, zdict=naive))
    assert t <= 0.97 * nv, (name, rec, t, nv)


def test_round_trip(mods):
    _lib, batch, corpus, devmem = mods
    name, rec, samples, records, naive = gate_cases()[1]
    trained = batch.train_dict(samples)
    comp = batch.compress(records, 6, zdict=trained)
    assert batch.decompress(comp, zdict=trained) == records
    for c, r in zip(comp[:50], records[:50]):
        o = zlib.decompressobj(zdict=trained)
        assert o.decompress(c) == r and o.eof


def test_bad_device_table_returns_an_error_and_no_bytes(mods, ctx):
    _lib, batch, corpus, devmem = mods
    samples = [corpus.text(5000, seed=20).tobytes() for _ in range(4)]
    d_in, offs, lens = _dev_form(ctx, devmem, samples)
    in_len = d_in.nbytes - _lib.BATCH_PAD
    for bad_off, bad_len in ((in_len - 100, 101), (1 << 40, 10), (0, in_len + 1)):
        tab = np.zeros((4, 4), dtype=np.uint64)
        tab[:, 0] = offs
        tab[:, 2] = lens
        tab[2, 0], tab[2, 2] = bad_off, bad_len
        d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
        r, out = ctx.train_dict_dev(d_in.ptr, in_len, d_tab.ptr, 4, 32768, 256, 8)
        assert r == _lib.E_ARG and out == b""
    # and the context still trains from a good table
    tab = np.zeros((4, 4), dtype=np.uint64)
    tab[:, 0] = offs
    tab[:, 2] = lens
    d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
    r, out = ctx.train_dict_dev(d_in.ptr, in_len, d_tab.ptr, 4, 32768, 256, 8)
    assert r == _lib.OK and out == R.train(samples)

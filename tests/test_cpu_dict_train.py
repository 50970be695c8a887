"""CPU: the batch API's dictionary trainer without a GPU -- the reference of DESIGN.md section 5c.2 (tests/dict_train_ref.py) on
hand-built cases, its quality gate on the stored held-out corpora through CPython's zlib, and the C ABI and Python face of
train_dict / train_dict_dev (exported symbols, ctypes argument types against the header, every ValueError raised before any device
call)."""
import ctypes as C
import os
import random
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT, heldout_corpora
import dict_train_ref as R

_FUNCS = ["zngamd_train_dict_dev", "zngamd_train_dict"]


def _rand(rng, n):
    return bytes(rng.randrange(256) for _ in range(n))


# ---- the reference on hand-built cases
def test_segment_in_every_sample_ends_the_dictionary():
    rng = random.Random(11)
    seg = _rand(rng, 64)
    samples = [_rand(rng, 100) + seg + _rand(rng, 836) for _ in range(40)]
    d = R.train(samples, 1000, k=64, d=8)
    assert d.endswith(seg) and len(d) == 1000


def test_samples_shorter_than_d_contribute_nothing():
    rng = random.Random(12)
    base = [_rand(rng, 300) for _ in range(20)]
    mixed = []
    for s in base:
        mixed += [s, b"", _rand(rng, 3), _rand(rng, 1)]
    for d in (4, 6, 8):
        h0, v0 = R.hashes(np.frombuffer(b"".join(base), dtype=np.uint8), [len(s) for s in base], d)
        h1, v1 = R.hashes(np.frombuffer(b"".join(mixed), dtype=np.uint8), [len(s) for s in mixed], d)
        f0 = np.bincount(h0[v0], minlength=1 << R.HASH_BITS)
        f1 = np.bincount(h1[v1], minlength=1 << R.HASH_BITS)
        assert np.array_equal(f0, f1)                        # the frequencies do not see them
        assert int(v1.sum()) == int(v0.sum()) == sum(len(s) - d + 1 for s in base)
    # a sample of exactly d bytes has one valid position, and the d - 1 in front of a sample's end are invalid
    _, v = R.hashes(np.frombuffer(b"abcdefgh" + b"12345678", dtype=np.uint8), [8, 8], 8)
    assert v.tolist() == [True] + [False] * 7 + [True]


def test_small_total_gives_a_shorter_dictionary():
    rng = random.Random(13)
    samples = [_rand(rng, 50) for _ in range(12)]             # 600 bytes
    d = R.train(samples, 32768, k=64, d=4)
    assert 0 < len(d) < 32768                                 # (picks may share their last d - 1 bytes with the next)
    assert R.train([b"\0" * 300], 32768, k=256, d=8) == b"\0" * 256    # one hash: one window of k bytes, then nothing scores


def test_ties_go_to_the_lowest_start():
    rng = random.Random(14)
    data = _rand(rng, 320)
    h, v = R.hashes(np.frombuffer(data, dtype=np.uint8), [len(data)], 4)
    assert len(set(h.tolist())) == len(h)                     # every window of K d-mers scores K
    assert R.train([data], 32, k=32, d=4) == data[:32]
    # the same with the samples cut anywhere: the first window of the epoch still wins
    assert R.train([data[:100], data[100:]], 32, k=32, d=4) == data[:32]


def test_trim_reads_freq_before_the_zeroing():
    """pick 1 takes P (three times in the data, twice more inside the two copies of P[4:8] q P[0:4]); pick 2's best window starts
    on the zeroed d-mer P[4:8] (a tie with the window one later, lowest start) and is trimmed to the four d-mers that cross q:
    P[5:8] q P[0:3].  The third pick has one byte of room, less than d."""
    rng = random.Random(15)
    P, q = _rand(rng, 8), b"\x00"
    X = [_rand(rng, 40) for _ in range(6)]
    data = X[0] + P + X[1] + P + X[2] + P + X[3] + P[4:] + q + P[:4] + X[4] + P[4:] + q + P[:4] + X[5]
    h, v = R.hashes(np.frombuffer(data, dtype=np.uint8), [len(data)], 4)
    st = {}
    d = R.train([data], 16, k=8, d=4, stats=st)
    assert d == P[5:] + q + P[:3] + P
    assert st["picks"] == 3 and st["epochs"] == 1


def test_epochs_follow_the_spec():
    assert R.epochs(1 << 20, 32768, 256) == (32, 32768)
    assert R.epochs(50000, 32768, 256) == (19, 2631)          # S < 10 k: E = n // (10 k)
    assert R.epochs(2000, 32768, 256) == (1, 2000)


# ---- the quality gate: trained against the naive first 32 KiB, on the stored corpora, through CPython's zlib
def gate_cases():
    c = heldout_corpora()
    out = []
    for name in ("python_sources", "c_headers", "libc_elf"):
        data = c[name]
        for rec in (1024, 4096):
            train, test = data[:1 << 20], data[1 << 20:2 << 20]
            samples = [train[i:i + rec] for i in range(0, len(train), rec)]
            records = [test[i * rec:(i + 1) * rec] for i in range(min(1000, len(test) // rec))]
            out.append((name, rec, samples, records, train[:32768]))
    return out


def zlib_total(records, zdict):
    t = 0
    for r in records:
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, zdict)
        t += len(c.compress(r) + c.flush())
    return t


@pytest.mark.parametrize("case", range(6))
def test_quality_gate_reference(case):
    name, rec, samples, records, naive = gate_cases()[case]
    trained = R.train(samples, 32768, k=256, d=8)
    assert len(trained) == 32768
    t, nv = zlib_total(records, trained), zlib_total(records, naive)
    assert t <= 0.97 * nv, (name, rec, t, nv)
    d = zlib.decompressobj(zdict=trained)
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, 0, trained)
    assert d.decompress(c.compress(records[0]) + c.flush()) == records[0]


# ---- the C ABI and the Python face
@pytest.fixture(scope="module")
def header():
    return open(os.path.join(ROOT, "include", "zng_amd.h")).read()


def test_symbols_declared_and_exported(header):
    from zlib_ng_amd import _lib
    L = _lib.load()
    for f in _FUNCS:
        assert re.search(r"\bint\s+" + f + r"\(", header), f
        assert f in _lib.SYMBOLS and hasattr(L, f), f


_CTYPES = {"zngamd_ctx *": C.c_void_p, "const void *": C.c_void_p, "const uint8_t *": C.c_void_p, "uint8_t *": C.c_void_p,
           "const zngamd_batch_item *": C.c_void_p, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32,
           "uint32_t *": C.POINTER(C.c_uint32)}


@pytest.mark.parametrize("fn", _FUNCS)
def test_ctypes_argtypes_match_the_header(header, fn):
    from zlib_ng_amd import _lib
    decl = header[header.index("int " + fn + "("):]
    decl = decl[decl.index("(") + 1:decl.index(");")]
    want = []
    for a in decl.split(","):
        m = re.match(r"^(.*?)\s*(\**)\s*(\w+)$", " ".join(a.split()))
        want.append(_CTYPES[m.group(1) + (" " + m.group(2) if m.group(2) else "")])
    got = getattr(_lib.load(), fn).argtypes
    assert len(got) == len(want) == 10
    assert list(got) == want, fn


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"a device call was made ({name})")


class _FakeBuf:
    nbytes = 1 << 20
    ptr = 0x1000


def test_value_errors_before_any_device_call(monkeypatch):
    from zlib_ng_amd import batch, zlib_ng

    def no_device():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(zlib_ng, "_ctx", no_device)
    ctx, buf = _NoDevice(), _FakeBuf()
    s = [b"x" * 1000]
    bad = [((), {}, "no samples"),
           ([b"x" * 255], {}, "fewer than k"),
           ([b"x" * 100, b"", b"y" * 20], {"k": 128}, "fewer than k"),
           (s, {"dict_size": 7}, "dict_size"), (s, {"dict_size": 32769}, "dict_size"), (s, {"dict_size": 0}, "dict_size"),
           (s, {"dict_size": 5, "d": 6}, "dict_size"),
           (s, {"d": 3}, "d must"), (s, {"d": 9}, "d must"),
           (s, {"k": 7}, "k must"), (s, {"k": 16385}, "k must"), (s, {"k": 5, "d": 6}, "k must")]
    for samples, kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            batch.train_dict(list(samples), **kw)
        lens = [len(x) for x in samples]
        offs = np.cumsum([0] + lens[:-1]) if lens else []
        with pytest.raises(ValueError, match=msg):
            batch.train_dict_dev(ctx, buf, offs, lens, **kw)
    with pytest.raises(ValueError, match="4 GiB"):
        batch.train_dict_dev(ctx, buf, [0, 0], [1 << 31, 1 << 31])
    with pytest.raises(ValueError, match="4 GiB"):
        batch._train_args([1 << 32], 32768, 256, 8)
    with pytest.raises(ValueError, match="outside the device buffer"):
        batch.train_dict_dev(ctx, buf, [0, buf.nbytes - 64 - 100], [500, 101])
    with pytest.raises(ValueError, match="outside the device buffer"):
        batch.train_dict_dev(ctx, buf, [1 << 40], [300])
    with pytest.raises(ValueError, match="differ in length"):
        batch.train_dict_dev(ctx, buf, [0, 10], [300])
    with pytest.raises(TypeError):
        batch.train_dict([b"x" * 1000, 3])
    with pytest.raises(TypeError):
        batch.train_dict(s, k=256.0)


def test_abi_rejects_bad_arguments_before_any_device_work():
    """the C entry points check their scalars and pointers before they touch the context: a stand-in context pointer is never
    dereferenced when an argument is bad"""
    from zlib_ng_amd import _lib
    L = _lib.load()
    fake_ctx = C.create_string_buffer(64)
    data = C.create_string_buffer(4096)
    item = (_lib.BatchItem * 1)()
    item[0].in_len = 4096
    out = (C.c_uint8 * 32768)()
    ln = C.c_uint32(7)
    good = dict(n=1, dict_size=32768, k=256, d=8)
    bad = [dict(n=0), dict(d=3), dict(d=9), dict(k=7), dict(k=16385), dict(dict_size=7), dict(dict_size=32769), dict(k=5, d=6)]
    for fn in (L.zngamd_train_dict, L.zngamd_train_dict_dev):
        assert fn(None, data, 4096, item, 1, 32768, 256, 8, out, C.byref(ln)) == _lib.E_ARG
        assert fn(fake_ctx, None, 4096, item, 1, 32768, 256, 8, out, C.byref(ln)) == _lib.E_ARG
        assert fn(fake_ctx, data, 4096, None, 1, 32768, 256, 8, out, C.byref(ln)) == _lib.E_ARG
        assert fn(fake_ctx, data, 4096, item, 1, 32768, 256, 8, None, C.byref(ln)) == _lib.E_ARG
        assert fn(fake_ctx, data, 4096, item, 1, 32768, 256, 8, out, None) == _lib.E_ARG
        for b in bad:
            a = {**good, **b}
            assert fn(fake_ctx, data, 4096, item, a["n"], a["dict_size"], a["k"], a["d"], out, C.byref(ln)) == _lib.E_ARG, b
        assert ln.value == 7                                      # nothing written

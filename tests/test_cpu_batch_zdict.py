"""CPU: the batch API's preset dictionary (zdict) without a GPU -- the header declares the four entry points and the mismatch status,
the binding has them, the ZNGAMD_BATCH_* family is unchanged, the mismatch status maps to decompressobj's text, argument errors are
raised before any device call, and sub-batches by primed size cover every item once."""
import re

import pytest

from conftest import ROOT

_FUNCS = ["zngamd_inflate_batch_dict_dev", "zngamd_inflate_batch_dict", "zngamd_deflate_batch_dict_dev", "zngamd_deflate_batch_dict"]


@pytest.fixture(scope="module")
def header():
    import os
    return open(os.path.join(ROOT, "include", "zng_amd.h")).read()


def test_header_declares_the_dictionary_entry_points(header):
    from zlib_ng_amd import _lib
    for f in _FUNCS:
        assert re.search(r"\bint\s+" + f + r"\(", header), f
        assert f in _lib.SYMBOLS, f
    m = re.search(r"#define\s+ZNGAMD_ZDICT_MISMATCH\s+(\d+)", header)
    assert m and int(m.group(1)) == _lib.ZDICT_MISMATCH == 13
    # the dictionary is a host pointer plus a length in every one of them
    for f in _FUNCS:
        decl = header[header.index("int " + f + "("):]
        decl = decl[:decl.index(");")]
        assert "const uint8_t *dict, uint32_t dict_len" in decl, f


def test_batch_status_family_is_unchanged(header):
    from zlib_ng_amd import _lib
    consts = dict(re.findall(r"#define\s+(ZNGAMD_BATCH_[A-Z_]+)\s+(\d+)", header))
    assert len(consts) == 14
    assert "ZNGAMD_BATCH_ZDICT_MISMATCH" not in consts
    assert _lib.ZDICT_MISMATCH not in {int(v) for k, v in consts.items() if k != "ZNGAMD_BATCH_PAD"}


def test_mismatch_status_has_decompressobj_text():
    from zlib_ng_amd import _lib, batch, zlib_ng
    e = batch.status_error(_lib.ZDICT_MISMATCH)
    assert type(e) is zlib_ng.error and str(e) == "Error -3 while setting zdict: invalid input data"
    # the statuses of the family keep their texts
    assert str(batch.status_error(_lib.BATCH_NEED_DICT)) == "Error 2 while decompressing data"
    assert str(batch.status_error(_lib.BATCH_TRUNCATED)) == "Error -5 while decompressing data: incomplete or truncated stream"


def test_argument_errors_before_any_device_call(monkeypatch):
    from zlib_ng_amd import batch, zlib_ng

    def no_device():
        raise AssertionError("a device call was made")

    monkeypatch.setattr(zlib_ng, "_ctx", no_device)
    for wbits in (31, 25, 24):                          # gzip: no decoder could supply the dictionary
        with pytest.raises(ValueError, match="Invalid dictionary"):
            batch.compress([b"x"], 6, wbits, zdict=b"dictionary")
        with pytest.raises(ValueError, match="Invalid dictionary"):
            batch.compress([b"x"], 6, wbits, zdict=b"")
    with pytest.raises(TypeError):
        batch.compress([b"x"], 6, 15, zdict="text")
    with pytest.raises(TypeError):
        batch.compress([b"x"], 6, 15, zdict=3)
    with pytest.raises(TypeError):
        batch.decompress([b"x"], 15, zdict="text")
    with pytest.raises(TypeError):
        batch.decompress([b"x"], 15, zdict=3)
    # compressobj's / decompressobj's own checks and texts
    with pytest.raises(ValueError, match="Invalid initialization option"):
        batch.compress([b"x"], 10, 15, zdict=b"d")
    with pytest.raises(ValueError, match="Invalid initialization option"):
        batch.compress([b"x"], 6, -8, zdict=b"d")
    with pytest.raises(ValueError, match="Invalid initialization option"):
        batch.compress([b"x"], 6, 15, strategy=5, zdict=b"d")
    with pytest.raises(TypeError):
        batch.compress([b"x"], "6", 15, zdict=b"d")
    with pytest.raises(ValueError, match="Invalid initialization option"):
        batch.decompress([b"x"], 17, zdict=b"d")
    with pytest.raises(TypeError):
        batch.decompress([b"x"], "15", zdict=b"d")
    with pytest.raises(ValueError, match="errors"):
        batch.decompress([b"x"], errors="ignore", zdict=b"d")
    with pytest.raises(TypeError):
        batch.compress([b"x", 3], zdict=b"d")
    assert batch.compress([], zdict=b"d") == [] and batch.decompress([], zdict=b"d") == []


def test_primed_sub_batches_cover_every_item_once():
    from zlib_ng_amd import batch
    lens = [5, 1, 7, 0, 12, 3, 3, 40, 0, 0]
    for tl in (0, 1, 4, 32768):
        primed = [ln + tl for ln in lens]
        for budget in (1, 6, 10, 100, 32770, 70000, 1 << 20):
            parts = batch._sub_batches(primed, budget)
            assert [i for a, b in parts for i in range(a, b)] == list(range(len(lens)))
            for a, b in parts:
                assert b - a == 1 or sum(primed[a:b]) <= budget


def test_compress_sub_batches_count_primed_bytes(monkeypatch):
    """every item staged behind its own copy of the dictionary's tail: the host form's sub-batches are bounded by (tail + item)"""
    from zlib_ng_amd import _lib, batch, zlib_ng
    calls = []

    class FakeCtx:
        def deflate_batch(self, data, items, n, level, wbits, strategy=0, zdict=None):
            lens = [items[k].in_len for k in range(n)]
            assert sum(lens) == memoryview(data).nbytes
            calls.append((lens, zdict))
            res = (_lib.BatchResult * max(n, 1))()
            for k in range(n):
                res[k].out_len = 1
                items[k].out_off = k
            return bytes(n), res, n

    monkeypatch.setattr(zlib_ng, "_ctx", lambda: FakeCtx())
    monkeypatch.setattr(batch, "SUB_BATCH_BYTES", 100000)
    lens = [10, 0, 5000, 30000, 1, 70000, 64, 64, 0, 2]
    items = [bytes(ln) for ln in lens]
    for zd in (b"", b"z" * 100, b"q" * 40000):
        calls.clear()
        out = batch.compress(items, 6, 15, zdict=zd)
        assert len(out) == len(items)
        tl = min(len(zd), 32768)
        assert [ln for c, _ in calls for ln in c] == lens          # every item once, in order
        for c, z in calls:
            assert z == zd
            assert len(c) == 1 or sum(ln + tl for ln in c) <= batch.SUB_BATCH_BYTES
        if tl == 32768:
            assert len(calls) > 2                                  # (without the tails all items fit one sub-batch)

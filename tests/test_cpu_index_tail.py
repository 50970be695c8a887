"""The file side of the segment index without a GPU: _lib.parse_index_tail on tails built by hand (the layout of
_lib.index_members) around a stand-in data member.  What the GPU file tests of test_gpu_index_hostile.py rest on is proved here:
index_mutations.rebuild yields a live index, every mutated tail of the classes F1-F5 is ACCEPTED by the parser with rows that
differ from the original (so a file test cannot pass by "no index found"), F6 (output that does not add up to ISIZE) and every
structural fault are refused, and the file position is restored either way."""
import io
import struct

import numpy as np
import pytest

import index_mutations as M

PLAIN = b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff" + b"\x03\x00" + bytes(8)


def _records():
    """500 units (two index members: 470 + 30) of every kind, with plausible numbers"""
    from zlib_ng_amd import _lib
    rng = np.random.default_rng(5)
    rec = np.zeros(500, _lib._index_rec_dtype())
    for u in range(500):
        kind = ("dynamic", "dynamic", "dynamic", "stored", "fixed", "empty", "dynamic", "stored")[u % 8]
        n = {"fixed": 80, "empty": 0}.get(kind, int(rng.choice([16384, 16384, 2049, 2047, 131072, 70000])))
        ns = (n + 2047) // 2048
        rec["out_len"][u] = n
        if kind == "dynamic":
            rec["e"][u][0] = int(rng.integers(300, 900))
            rec["e"][u][1:ns + 1] = rng.integers(2000, 9000, ns)
            rec["in_len"][u] = (int(rec["e"][u].astype(np.int64).sum()) + 7 + 10) // 8 + 4
        elif kind == "fixed":
            rec["e"][u][0], rec["e"][u][1] = 3, 200
            rec["in_len"][u] = 31
        elif kind == "stored":
            rec["in_len"][u] = n + 5 * ((n + 65534) // 65535) + 5
        else:
            rec["in_len"][u] = 5
    return rec


def _blob(rec, plain=True):
    from zlib_ng_amd import _lib
    body = int(rec["in_len"].astype(np.int64).sum())
    isize = int(rec["out_len"].astype(np.int64).sum()) & 0xFFFFFFFF
    member = b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\xff" + bytes(body) + b"\x03\x00" + struct.pack("<II", 0x12345678, isize)
    return member + _lib.index_members([rec], len(member)) + (PLAIN if plain else b"")


@pytest.fixture(scope="module")
def rec():
    return _records()


@pytest.fixture(scope="module")
def blob(rec):
    b = _blob(rec)
    assert len(b) >= 65536
    return b


def _parse(b, start=0, end=None):
    """parse_index_tail from a position that must be left alone"""
    from zlib_ng_amd import _lib
    fp = io.BytesIO(b)
    fp.seek(7)
    got = _lib.parse_index_tail(fp, start, len(b) if end is None else end)
    assert fp.tell() == 7
    return got


def test_rebuild_yields_a_live_index(rec, blob):
    kinds = M.rec_kinds(rec)
    assert {"dynamic", "fixed", "stored", "empty"} <= set(kinds)
    for plain in (True, False):
        b0 = _blob(rec, plain)
        a = _parse(b0)
        assert a is not None
        assert M.split_tail(b0) == (20 + int(rec["in_len"].astype(np.int64).sum()), plain)
        b1 = M.rebuild(b0, rec)
        assert b1 == b0
        b = _parse(b1)
        assert b is not None and all(np.array_equal(x, y) for x, y in zip(a, b))
    uin, uout, rows = _parse(blob)
    assert np.array_equal(uin, rec["in_len"]) and np.array_equal(uout, rec["out_len"]) and rows.shape == (500, 68)
    for u in (0, 3, 4, 5, 470, 499):
        ns = M.nseg_of(uout[u])
        want = np.cumsum(rec["e"][u].astype(np.int64))[:ns + 1] if kinds[u] in ("dynamic", "fixed") else np.zeros(ns + 1)
        assert np.array_equal(rows[u, :ns + 1], want) and not rows[u, ns + 1:].any(), u


def test_every_mutated_tail_but_f6_is_accepted_and_differs(rec, blob):
    """the vacuity guard of the GPU file tests (on the first 40 records: one index member, every kind of unit)"""
    rec = rec[:40].copy()
    blob = _blob(rec)
    assert len(blob) >= 65536
    base = _parse(blob)
    seen = {}
    for name, rec2, unit in M.tail_cases(rec):
        cls = name.split(":")[0]
        seen[cls] = seen.get(cls, 0) + 1
        assert 0 <= unit < len(rec)
        got = _parse(M.rebuild(blob, rec2))
        if cls == "F6":
            assert got is None, name
            continue
        assert got is not None, name
        assert any(not np.array_equal(x, y) for x, y in zip(base, got)), name
        assert int(got[0].astype(np.int64).sum()) == int(base[0].astype(np.int64).sum()), name
        assert int(got[1].astype(np.int64).sum()) == int(base[1].astype(np.int64).sum()), name
    assert set(seen) == set(M.TAIL_CLASSES), seen
    names = [n for n, _, _ in M.tail_cases(rec)]
    for part in ("claimed-empty:near", "claimed-empty:far", "empty-claimed-1", "zeros", "deltas-of-dynamic", ":swap", ":-2048"):
        assert any(part in n for n in names), part


def test_isize_is_checked_modulo_2_32(rec):
    """out_len sums are compared with ISIZE modulo 2^32: a member of 4 GiB + 5 bytes"""
    from zlib_ng_amd import _lib
    big = np.zeros(32769, _lib._index_rec_dtype())
    big["out_len"][:32768] = 131072
    big["out_len"][32768] = 5
    big["in_len"] = 5
    b = _blob(big)
    assert struct.unpack_from("<I", b, M.split_tail(b)[0] - 4)[0] == 5
    assert _parse(b) is not None
    big["out_len"][32768] = 6
    assert _parse(M.rebuild(b, big)) is None


def _edit(b, at, fmt, value):
    out = bytearray(b)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def test_structural_faults_are_refused(rec, blob):
    from zlib_ng_amd import _lib
    dbytes, plain = M.split_tail(blob)
    assert plain
    m0 = dbytes                                        # the first index member: header 12, 'ZA' slen, then v k n first
    loc = len(blob) - 20 - _lib.INDEX_LOCATOR_BYTES    # the locator: header 12, 'ZA' slen, then v k pad nm nu ibytes dbytes
    m1 = m0 + 16 + struct.unpack_from("<H", blob, m0 + 14)[0] + 10
    assert blob[m0 + 16:m0 + 18] == b"\x03\x01" and blob[m1 + 16:m1 + 18] == b"\x03\x01" and blob[loc + 16:loc + 18] == b"\x03\x02"
    assert struct.unpack_from("<HI", blob, m1 + 18) == (30, 470)
    nm, nu, ibytes, db = struct.unpack_from("<IIQQ", blob, loc + 20)
    assert (nm, nu, db) == (2, 500, dbytes)
    assert _parse(blob) is not None
    assert _parse(_edit(blob, m0 + 16, "<B", 2)) is None                       # wrong v
    assert _parse(_edit(blob, m1 + 17, "<B", 2)) is None                       # wrong k
    assert _parse(_edit(blob, m1 + 20, "<I", 469)) is None                     # first != seen
    assert _parse(_edit(blob, m1 + 18, "<H", 29)) is None                      # slen does not match n
    assert _parse(_edit(blob, loc + 24, "<I", 499)) is None                    # seen != nu
    junk = blob[:loc] + bytes(10) + _edit(blob[loc:], 28, "<Q", ibytes + 10)
    assert struct.unpack_from("<Q", junk, loc + 10 + 28)[0] == ibytes + 10
    assert _parse(junk) is None                                                # at != ibytes
    rec2 = rec.copy()
    rec2["in_len"][0] += 1
    assert _parse(M.rebuild(blob, rec2)) is None                               # in_len sum off by one
    assert _parse(_edit(blob, loc + 24, "<I", 0)) is None                      # nu == 0
    assert _parse(_edit(blob, loc + 12, "<B", ord("Y"))) is None               # locator magic
    assert _parse(_edit(blob, loc + 17, "<B", 1)) is None                      # ... its kind
    assert _parse(blob[:-25]) is None                                          # truncated tail: the locator is cut
    assert _parse(blob[:loc + 10]) is None
    assert _parse(blob, 0, 40) is None                                         # a file shorter than a locator
    # the index describes the member it stands behind: a start that is not the member's is refused
    assert _parse(blob, 1) is None

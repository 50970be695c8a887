"""Segment indexes that are well formed and WRONG, handed to the unit decoder (zngamd_inflate_units_indexed_dev ->
za_k_inflate_units_marked) and, inside files, to both readers.  The index is not authenticated: the only thing that stands
between a wrong number and wrong bytes is a check against the stream itself.  Every case comes from index_mutations.py; a refused
index must come back as E_INDEX / DATA_ERROR (raw call) or be dropped for the ordinary decoder (files: an index is advisory and
never turns a readable file into an error), and whatever the call answers, STREAM_END must mean "the bytes the system zlib decodes".

The cases change index CONTENT only -- unit_in_len, unit_out_len, rows, file tails -- never what the ABI makes the caller's duty
(pointers, def_len within the buffer, 64 readable bytes behind the stream: Stream.call provides them).  Why no case can leave a buffer,
field by field (za_inflate_units.hip, za_mem_tables / za_mem_phase_a in za_inflate.hip, inflate_units_core in zng_amd.hip):

  uin  (R8, F2)   the host refuses sum(uin) > def_len, so in_off + in_len <= in_total for every unit (the kernel's gate repeats it);
                  in_len > 2^20 fails the gate.  Stored path: `at + 5 + len > in_len` is tested before a block's header or bytes are
                  read.  Phase A stages input through prefetch(), clamped to [in, in + in_total); the single reads behind a lane's
                  stop (za_peek at bp == my_stop <= in_bits, the sync marker's four bytes once their position equals in_len - 4)
                  stay inside in_len + the 64 pad bytes.  The empty-unit check reads in_len (2 or 5) bytes after testing in_len.
  uout (R9, R10,  the host refuses uout > 131 072 and sum(uout) > out_cap; nseg is derived from uout by host and kernel alike
        F3)       (<= 64).  A unit's area is 32 768 + 131 072 symbols whatever uout says, the gate tests out_off + 32 768 + out_len
                  <= out_cap, lane < nseg writes literals at most 2 048 + 16 bytes into its own 4 096 bytes of the area.  hist =
                  min(32 768, claimed output in front): `dist <= pos + hist` keeps area coordinates >= 32 768 - hist >= 0.  A unit
                  claimed empty gets no area, no queue and no row; its bytes are compared with an empty unit's.  The window
                  kernels run only after EVERY unit of the batch reported out_len == the claimed one.
  rows (R1-R7,    only entries 0..nseg are read (S1 changes the others); an entry with any of bits 23..31 set fails the ballot
        F1, F4,   before use, so offsets are < 2^23.  A lane starts only if my_start <= my_stop <= in_bits (else lane_err and
        F5)       `done`: prefetch loads nothing for it); rows[0] must equal the header's end as the header itself gives it; every
                  lane must stop with bp == my_stop and pos == end: a token across the segment end, an end-of-block inside a
                  segment and `nmatch + 2 > ZA_MATCHQ_PER_SEG` (688 >= 2048 / 3 entries, each worth >= 3 bytes of output) are
                  index errors; the last lane must find end-of-block and the sync marker on the unit's last bytes.  rows[nseg] ==
                  0 sends the unit down the stored path, which demands stored block headers (a coded unit's first byte fails it).
  files (F1-F6)   parse_index_tail bounds nu, ibytes and every record count against the bytes it read; out_len > 131 072 fails
                  zngamd_index_create; the windowed reader takes units only while cum_in fits the staged window and cum_out the
                  output room, then everything above applies.

Decoding is deterministic from a fixed start, so only the true entries can pass: that is the claim R1-R10 test; S1 is the
converse (entries nobody reads change nothing)."""
import gzip
import io
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import index_mutations as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 131072
SEG2K = 16
WINDOW = 262144


def _mix(n, seed):
    from zlib_ng_amd import corpus
    rng = np.random.default_rng(seed)
    parts = [corpus.text(n // 3, seed + 1).tobytes(), bytes(n // 8), rng.integers(0, 256, n // 6, dtype=np.uint8).tobytes(),
             corpus.fastq(n // 4, seed + 2).tobytes(), (b"abcdefgh" * 4096)[:n // 16]]
    out = b"".join(parts)
    return (out + corpus.text(max(0, n - len(out)), seed + 3).tobytes())[:n]


def _coded(n, seed):
    """text and FASTQ: a unit that is certain to be a dynamic block"""
    from zlib_ng_amd import corpus
    return (corpus.text(n - n // 3, seed).tobytes() + corpus.fastq(n // 3, seed + 1).tobytes())[:n]


class Stream:
    """one indexed stream of 12 units of every kind on the device, its index on the host, and zlib's decode of it"""

    def __init__(self, ctx, dict_first):
        from zlib_ng_amd import devmem
        rng = np.random.default_rng(17)
        pieces = [_coded(16384, 1), rng.integers(0, 256, 16384, dtype=np.uint8).tobytes(), _coded(16384, 2), _mix(B, 3)[:B // 2] + _coded(B // 2, 4),
                  b"", _coded(2049, 5), _coded(16384, 6), b"ab" * 40, _coded(2047, 7), rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(),
                  _coded(16384, 8), _coded(16384, 9)]
        self.dict = dict_first
        self.data = b"".join(pieces)
        buf = dict_first + self.data
        blocks, off = [], len(dict_first)
        for p in pieces:
            blocks.append((off, len(p), min(32768, off), SEG2K))
            off += len(p)
        outs, crcs, ovf = ctx.deflate_blocks(buf, blocks, 6, B + B // 8 + 600)
        assert not ovf
        nu = len(blocks)
        self.rows = ctx.deflate_index(nu).cpu(np.uint32).reshape(nu, -1).copy()
        self.stream = b"".join(outs) + b"\x03\x00"
        self.uin = np.array([len(c) for c in outs], np.uint32)
        self.uout = np.array([len(p) for p in pieces], np.uint32)
        self.kinds = M.kinds_of(self.stream, self.uin, self.uout, self.rows)
        z = zlib.decompressobj(-15, zdict=dict_first) if dict_first else zlib.decompressobj(-15)
        self.ref = z.decompress(self.stream)                     # what the UNMODIFIED stream decodes to
        self.ctx = ctx
        self.d_def = devmem.from_host(ctx, self.stream + bytes(64))
        self.d_dict = devmem.from_host(ctx, dict_first) if dict_first else None
        self.d_rows = devmem.empty(ctx, self.rows.nbytes)
        self.d_out = devmem.empty(ctx, len(self.data) + 4096 + 64)
        self.cases = list(M.rows_cases(self.uin, self.uout, self.rows, self.kinds))

    def call(self, uin, uout, rows):
        """-> (code, out_len, bytes when the call said STREAM_END)"""
        from zlib_ng_amd import _lib
        total = int(np.asarray(uout, np.int64).sum())
        assert total + 64 <= self.d_out.nbytes and int(np.asarray(uin, np.int64).sum()) + 2 == len(self.stream)
        self.d_rows[:] = np.ascontiguousarray(rows, np.uint32)
        r, n = self.ctx.inflate_units_indexed_dev(self.d_def.ptr, len(self.stream), uin, uout, self.d_rows.ptr, self.d_out.ptr, total,
                                                  self.d_dict.ptr if self.d_dict else None, len(self.dict))
        return r, n, (self.d_out[0:n].cpu().tobytes() if r == _lib.STREAM_END and n <= total else None)

    def control(self):
        from zlib_ng_amd import _lib
        r, n, back = self.call(self.uin, self.uout, self.rows)
        assert r == _lib.STREAM_END and n == len(self.data) and back == self.data, (r, n, self.ctx.err())


@pytest.fixture(scope="module", params=["plain", "dict"])
def S(request, ctx):
    return Stream(ctx, _mix(32768, 13) if request.param == "dict" else b"")


def test_control(S):
    assert S.ref == S.data
    assert [M.nseg_of(n) for n in S.uout] == [8, 8, 8, 64, 0, 2, 8, 1, 1, 35, 8, 8]
    assert S.kinds == ["dynamic", "stored", "dynamic", "dynamic", "empty", "dynamic", "dynamic", "fixed", "dynamic", "stored", "dynamic", "dynamic"], S.kinds
    assert int(S.uin[4]) == 5 and int(S.uin[9]) == 70000 + 2 * 5 + 5           # the empty unit; two stored blocks and the marker
    S.control()
    # every class has instances, and the ones a stream can lack are there
    names = [c[0] for c in S.cases]
    assert {n.split(":")[0] for n in names} == set(M.ROW_CLASSES)
    for part in ("R1:u3:s63", ":swap", ":eqnext", ":eqprev", "R3:u0:zero", "rows-of-dynamic", "R4:u0:zeros", "R5:", "bit23", "bit31", ":far", "decreasing",
                 "R8:u3:swap", "R9:u5:+1", "R9:u9:+1", ":-2048", "R10:u0:claimed-empty", "R10:u1:claimed-empty", "R10:u7:claimed-empty", "R10:u4:empty-claimed-1",
                 "S1:u3:behind-eob", "S1:u1:stored-front", "S1:u9:stored-front"):
        assert any(part in n for n in names), part
    assert all(c[4] == (not c[0].startswith("S1")) for c in S.cases)


@pytest.mark.parametrize("cls", [c for c in M.ROW_CLASSES if c != "S1"])
def test_rows_refused(S, cls):
    from zlib_ng_amd import _lib
    wrong = []
    for name, uin, uout, rows, must in S.cases:
        if name.split(":")[0] != cls:
            continue
        assert must
        r, n, back = S.call(uin, uout, rows)
        if r not in (_lib.E_INDEX, _lib.DATA_ERROR):
            wrong.append((name, r, n, None if back is None else back == S.ref))
    assert not wrong, "accepted or answered with another code (name, code, out_len, bytes right): %r" % (wrong[:8],)
    S.control()                     # a refused call leaves nothing behind in the unit areas, the match queues or the windows


def test_rows_ignored(S):
    from zlib_ng_amd import _lib
    for name, uin, uout, rows, must in S.cases:
        if name.startswith("S1"):
            assert not must
            r, n, back = S.call(uin, uout, rows)
            assert r == _lib.STREAM_END and n == len(S.data) and back == S.data, (name, r, n, S.ctx.err())


@pytest.mark.parametrize("cls", M.ROW_CLASSES)
def test_any_verdict_is_honest(S, cls):
    """STREAM_END, whatever the case wanted, comes with exactly the bytes of the unmodified stream"""
    from zlib_ng_amd import _lib
    lies = []
    for name, uin, uout, rows, must in S.cases:
        if name.split(":")[0] != cls:
            continue
        r, n, back = S.call(uin, uout, rows)
        if r == _lib.STREAM_END and not (n == len(S.data) and back == S.ref):
            lies.append((name, n, len(S.data)))
    assert not lies, "STREAM_END with other bytes than the stream's (name, out_len, true length): %r" % (lies[:8],)
    S.control()


# ---- files: the index is advisory

def _write(T, data, **kw):
    bio = io.BytesIO()
    with T.open(bio, "wb", compresslevel=6, threads=1, **kw) as f:
        for o in range(0, len(data), 1 << 20):
            f.write(data[o:o + (1 << 20)])
    return bio.getvalue()


class File:
    """40 blocks of 16 KiB: five of the mix, thirty that do not compress (the stored-only stretch -- it also makes the file three
    read windows long), then one of the mix, one more that does not compress, three of the mix: units of both kinds in the first
    window and in the third"""

    def __init__(self):
        from zlib_ng_amd import gzip_ng_threaded as T, _lib
        rng = np.random.default_rng(23)
        self.data = (_mix(5 * 16384, 51) + rng.integers(0, 256, 30 * 16384, dtype=np.uint8).tobytes() + _mix(16384, 52) +
                     rng.integers(0, 256, 16384, dtype=np.uint8).tobytes() + _mix(3 * 16384, 53))
        self.blob = _write(T, self.data, block_size=16384)
        assert len(self.blob) > 65536                                  # the reader looks for a tail
        got = _lib.parse_index_tail(io.BytesIO(self.blob), 0, len(self.blob))
        assert got is not None
        self.uin, self.uout, self.rows = got
        self.nu = len(self.uin)
        dbytes, plain = M.split_tail(self.blob)
        assert plain
        self.rec = np.frombuffer(self.blob, _lib._index_rec_dtype(), self.nu, dbytes + 24).copy()       # one index member: 40 < 470
        # the read window a unit is decoded in: the one its last byte arrives with (the member's header is 10 bytes)
        ends = 10 + np.cumsum(self.uin.astype(np.int64))
        self.win = ((ends - 1) // WINDOW).astype(int)
        self.kinds = M.rec_kinds(self.rec)


@pytest.fixture(scope="module")
def F(ctx):
    return File()


def _read(opener, blob):
    with opener(io.BytesIO(blob), "rb") as f:
        return f.read()


def _read_counted(ctx, opener, blob):
    ctx.L.zngamd_indexed_units(ctx.h, 1)
    back = _read(opener, blob)
    return back, int(ctx.L.zngamd_indexed_units(ctx.h, 1))


def test_file_control(ctx, F, monkeypatch):
    from zlib_ng_amd import gzip_ng_threaded as T, gzip_ng
    monkeypatch.setenv("ZNGAMD_READ_WINDOW", str(WINDOW))
    assert F.nu == 40 and int(F.uout.sum()) == len(F.data)
    assert sorted(set(F.win)) == [0, 1, 2], F.win                      # several windows, and a third
    assert {"dynamic", "stored"} <= {F.kinds[u] for u in range(F.nu) if F.win[u] == 0}
    assert {"dynamic", "stored"} <= {F.kinds[u] for u in range(F.nu) if F.win[u] == 2}
    same = M.rebuild(F.blob, F.rec)
    assert same == F.blob
    for opener in (T.open, gzip_ng.open):
        back, used = _read_counted(ctx, opener, same)
        assert back == F.data and used == F.nu, used
    assert gzip.decompress(same) == F.data


def _file_cases(F):
    """two cases per class, variant and window (the first and the third) -- the first and the last unit there that the variant
    fits: (name, blob, window of the first wrong unit)"""
    first, last = {}, {}
    for name, rec2, unit in M.tail_cases(F.rec):
        if name.startswith("F6"):
            continue
        key = (re.sub(r"u\d+|s\d+:", "", name), int(F.win[unit]))
        if key[1] in (0, 2):
            first.setdefault(key, (name, rec2))
            last[key] = (name, rec2)
    out = []
    for key in first:
        for name, rec2 in dict([first[key], last[key]]).items():
            out.append((name, M.rebuild(F.blob, rec2), key[1]))
    return out


@pytest.mark.parametrize("cls", [c for c in M.TAIL_CLASSES if c != "F6"])
def test_file_tails(ctx, F, cls, monkeypatch):
    from zlib_ng_amd import gzip_ng_threaded as T, gzip_ng, _lib
    monkeypatch.setenv("ZNGAMD_READ_WINDOW", str(WINDOW))
    cases = [c for c in _file_cases(F) if c[0].startswith(cls)]
    assert {w for _, _, w in cases} == {0, 2}, [c[0] for c in cases]
    n_first = int((F.win == 0).sum())
    for name, blob, w in cases:
        got = _lib.parse_index_tail(io.BytesIO(blob), 0, len(blob))
        assert got is not None and any(not np.array_equal(a, b) for a, b in zip(got, (F.uin, F.uout, F.rows))), name     # a live, wrong index
        assert gzip.decompress(blob) == F.data, name
        for opener in (T.open, gzip_ng.open):
            back, used = _read_counted(ctx, opener, blob)
            assert back == F.data, (name, opener.__module__, len(back))
            if w == 2:
                assert 0 < used < F.nu, (name, used)           # in use until it failed, then dropped
            else:
                assert used <= n_first, (name, used)
            back2, used2 = _read_counted(ctx, opener, blob)      # `dead` belongs to the handle, not to the process
            assert back2 == F.data and used2 == used, (name, used, used2)
    # ... and a good file still goes through its index afterwards
    back, used = _read_counted(ctx, T.open, F.blob)
    assert back == F.data and used == F.nu


def test_file_real_damage_still_reported(ctx, F, monkeypatch):
    """falling back must not swallow real damage: a wrong tail AND a flipped byte inside a stored unit (every inflater decodes it, to
    other bytes: the member's CRC is what notices)"""
    from zlib_ng_amd import gzip_ng_threaded as T, gzip_ng
    monkeypatch.setenv("ZNGAMD_READ_WINDOW", str(WINDOW))
    u = next(u for u in range(F.nu) if F.kinds[u] == "stored" and F.win[u] == 1)
    at = 10 + int(F.uin[:u].astype(np.int64).sum()) + 100
    for name, blob, w in [c for c in _file_cases(F) if c[0].startswith(("F1", "F3"))][:4] + [("none", F.blob, -1)]:
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(Exception):
            gzip.decompress(bytes(bad))
        for opener in (T.open, gzip_ng.open):
            with pytest.raises(Exception):
                _read(opener, bytes(bad))
    monkeypatch.setenv("ZNGAMD_NO_INDEX", "1")
    with pytest.raises(Exception):
        _read(T.open, bytes(bad))


def test_short_batches_fall_back():
    """A file of the package's own writer whose blocks are so small that one batch of the unit decoder (ZNGAMD_UNIT_BATCH, at least
    64 units) holds less than the 32 KiB window: the index does not apply, the file reads.  In a child process: the batch size is
    read once per process.  (Read in one window this file went through before the fix as well -- so small a file goes the way of
    many small members and its index is never asked; read in windows of 64 KiB the engine answered "a batch of units shorter than
    the window" as an argument error, -202, and both readers raised it, as the raw call did.)"""
    code = r'''
import gzip, io, os, sys
sys.path.insert(0, os.path.join(%r, "python-zlib-ng_amd"))
import numpy as np
from zlib_ng_amd import devmem, gzip_ng, gzip_ng_threaded as T, _lib
data = np.random.default_rng(3).integers(0, 256, 300 * 400, dtype=np.uint8).tobytes()
bio = io.BytesIO()
with T.open(bio, "wb", compresslevel=6, threads=1, block_size=400) as f:
    f.write(data)
blob = bio.getvalue()
assert len(blob) > 65536
got = _lib.parse_index_tail(io.BytesIO(blob), 0, len(blob))
assert got is not None and len(got[0]) == 300 and int(got[1][:64].sum()) == 25600
assert gzip.decompress(blob) == data
ctx = _lib.default_context()
# (a file this small in ONE window goes the way of files of many small members and never asks its index: windows of 64 KiB make
# the reader take the member's first 159 units with the index -- the second batch of 64 then stands behind 25 600 bytes)
for window in (None, 65536):
    if window:
        os.environ["ZNGAMD_READ_WINDOW"] = str(window)
    for opener in (T.open, gzip_ng.open):
        ctx.L.zngamd_indexed_units(ctx.h, 1)
        with opener(io.BytesIO(blob), "rb") as f:
            back = f.read()
        assert back == data, (window, opener.__module__, len(back))
        used = ctx.L.zngamd_indexed_units(ctx.h, 1)
        assert used < 300 and (not window or used > 0), (window, used)      # asked, then dropped
# the raw call says "no index here", not "bad argument"
uin, uout, rows = got
stream = blob[10:10 + int(uin.sum())] + b"\x03\x00"
d_def, d_out, d_rows = devmem.from_host(ctx, stream + bytes(64)), devmem.empty(ctx, len(data) + 64), devmem.from_host(ctx, rows)
r, n = ctx.inflate_units_indexed_dev(d_def.ptr, len(stream), uin, uout, d_rows.ptr, d_out.ptr, len(data))
assert r == _lib.E_INDEX, (r, ctx.err())
print("ok")
''' % (ROOT,)
    env = dict(os.environ, ZNGAMD_UNIT_BATCH="64")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])

"""Batch API: compress and decompress many independent buffers in one call.

    batch.compress(items, level=-1, wbits=MAX_WBITS, *, strategy=Z_DEFAULT_STRATEGY, zdict=None) -> list[bytes]
    batch.decompress(items, wbits=MAX_WBITS, *, errors="raise", zdict=None) -> list[bytes]
    batch.compress_dev(ctx, d_in, offsets, lengths, ...) -> (DeviceBuffer, out_offsets, out_lengths)
    batch.decompress_dev(ctx, d_in, offsets, lengths, ...) -> (DeviceBuffer, out_offsets, out_lengths, statuses)
    batch.train_dict(samples, dict_size=32768, *, k=256, d=8) -> bytes
    batch.train_dict_dev(ctx, d_in, offsets, lengths, dict_size=32768, *, k=256, d=8) -> bytes

`compress(items, level, wbits)[i] == zlib_ng.compress(items[i], level, wbits)` byte for byte, and `decompress(items, wbits)[i] ==
zlib_ng.decompress(items[i], wbits)`; where the one-shot raises, the batch raises the same type with the same message for the first
failing item in index order (its index in the exception's `index` attribute), or with errors="return" puts the exception in that
item's slot.  One wavefront per item, all items of a call in one launch set (za_batch.hip).

With a preset dictionary (zdict, one for the whole call) the yardsticks are the stream objects: compress(items, level, wbits,
strategy=s, zdict=d)[i] is what compressobj(level, DEFLATED, wbits, DEF_MEM_LEVEL, s, d) writes for items[i] (compress + flush), and
decompress(items, wbits, zdict=d)[i] is decompressobj(wbits, zdict=d).decompress(items[i]), an unfinished stream being the error
"incomplete or truncated stream".

train_dict makes such a dictionary from sample records (za_dict.hip): the k-byte segments whose d-mers recur
most across the samples, the best nearest the end.  Pass it unchanged as zdict= here, to compressobj / decompressobj or to CPython's zlib.
"""

import numpy as np

from . import _lib
from . import zlib_ng as _z

MAX_WBITS = _z.MAX_WBITS
Z_DEFAULT_COMPRESSION = _z.Z_DEFAULT_COMPRESSION
Z_DEFAULT_STRATEGY = _z.Z_DEFAULT_STRATEGY

# A compressed item of at least this many bytes is decoded by the single-stream path (zlib_ng.decompress: chunk-parallel where the
# stream allows it) instead of on one wavefront: one wave decodes about 58 MB/s, so an item of 256 KiB (about 1 MB of text) keeps its
# wave busy ~15 ms, longer than a whole batch of 10 000 small items takes, while the single-stream path needs a few ms for it
# (DESIGN.md section 5c).
LARGE_ITEM = 256 << 10
# Bytes of input per engine call: a larger batch runs as consecutive sub-batches of about this size, so that the staging buffers
# (input, first-guess output room) stay bounded.  The results are the same.
SUB_BATCH_BYTES = 256 << 20
# With a dictionary, an item of at least this many bytes is compressed by compressobj itself: the stream compresses a piece of 32 MiB
# or more where it lies (zs_deflate_batch in zng_stream.hip), in other blocks than the single one of a batch item, and byte identity
# with the stream needs its cut.
ZS_BATCH = 32 << 20

W = "while decompressing data"
# the one-shot's exception for each item status (zlib_ng.decompress)
_MESSAGES = {
    _lib.BATCH_TRUNCATED: (_lib.BUF_ERROR, None),
    _lib.BATCH_NEED_DICT: (_lib.NEED_DICT, None),
    _lib.BATCH_HEADER: (_lib.DATA_ERROR, "incorrect header check"),
    _lib.BATCH_WINDOW: (_lib.DATA_ERROR, "invalid window size"),
    _lib.BATCH_METHOD: (_lib.DATA_ERROR, "unknown compression method"),
    _lib.BATCH_FLAGS: (_lib.DATA_ERROR, "unknown header flags set"),
    _lib.BATCH_HCRC: (_lib.DATA_ERROR, "header crc mismatch"),
    _lib.BATCH_DATA: (_lib.DATA_ERROR, None),
    _lib.BATCH_CHECK: (_lib.DATA_ERROR, "incorrect data check"),
    _lib.BATCH_LENGTH: (_lib.DATA_ERROR, "incorrect length check"),
}
WZ = "while setting zdict"


def status_error(status):
    """The exception zlib_ng.decompress raises for an item with this ZNGAMD_BATCH_* status (None for BATCH_OK); for
    ZNGAMD_ZDICT_MISMATCH the one decompressobj(zdict=...) raises for a stream written with another dictionary."""
    if status == _lib.ZDICT_MISMATCH:
        return _z._zerr(_lib.DATA_ERROR, WZ)
    return _status_error(status)


def _status_error(status):
    if status == _lib.BATCH_OK:
        return None
    if status in _MESSAGES:
        code, detail = _MESSAGES[status]
        return _z._zerr(code, W, detail)
    if status == _lib.BATCH_TABLE:
        return ValueError("batch item lies outside the buffers")
    return _lib.EngineError(status, "unexpected batch status")


def _check_errors(errors):
    if errors not in ("raise", "return"):
        raise ValueError(f"errors must be 'raise' or 'return', not {errors!r}")


def _inflate_wbits(w):
    """wbits zlib_ng.decompress / decompressobj accept"""
    return w == 0 or 8 <= w <= 15 or -15 <= w <= -8 or 24 <= w <= 31 or w == 16 or 40 <= w <= 47 or w == 32


def _inflate_kind(wbits):
    if not isinstance(wbits, int):
        raise TypeError(f"an integer is required (got type {type(wbits).__name__})")
    if not _inflate_wbits(wbits):
        raise _z._zerr(_lib.STREAM_ERROR, "while preparing to decompress data")


def _check_strategy(strategy):
    if not isinstance(strategy, int):
        raise TypeError(f"an integer is required (got type {type(strategy).__name__})")
    if not _lib.STRATEGY_DEFAULT <= strategy <= _lib.STRATEGY_FIXED:
        raise ValueError("Invalid initialization option")


def _zdict_compress_args(level, wbits, strategy, zdict):
    """compressobj(level, DEFLATED, wbits, DEF_MEM_LEVEL, strategy, zdict)'s checks in its order -> the dictionary as bytes"""
    for v in (level, wbits, strategy):
        if not isinstance(v, int):
            raise TypeError(f"an integer is required (got type {type(v).__name__})")
    try:
        kind, _ = _z._container(wbits)
    except _z.error:
        kind = None
    if kind is None or not -1 <= level <= 9 or not _lib.STRATEGY_DEFAULT <= strategy <= _lib.STRATEGY_FIXED:
        raise ValueError("Invalid initialization option")
    z = bytes(_z._view(zdict))
    if kind == "gzip":                   # no gzip decoder could supply it (deflateSetDictionary: Z_STREAM_ERROR)
        raise ValueError("Invalid dictionary")
    return z


def _zdict_decompress_args(wbits, zdict):
    """decompressobj(wbits, zdict)'s checks in its order -> the dictionary as bytes"""
    if not isinstance(wbits, int):
        raise TypeError(f"'{type(wbits).__name__}' object cannot be interpreted as an integer")
    z = bytes(_z._view(zdict))
    if not _inflate_wbits(wbits):
        raise ValueError("Invalid initialization option")
    return z


def _zdict_reference(view, wbits, zdict):
    """decompress with a dictionary on the single-stream path: decompressobj, and an unfinished stream is an error"""
    o = _z.decompressobj(wbits, zdict=zdict)
    out = o.decompress(view)
    if not o.eof:
        raise _z._zerr(_lib.BUF_ERROR, W)
    return out


def _views(items):
    return [_z._view(x) for x in items]


def _split(views, limit):
    """the items the engine takes -- all of them (limit None), else those under `limit` bytes -> (their indices, views, sizes)"""
    if limit is None:
        return range(len(views)), views, [v.nbytes for v in views]
    idx = [i for i, v in enumerate(views) if v.nbytes < limit]
    sv = [views[i] for i in idx]
    return idx, sv, [v.nbytes for v in sv]


def _sub_batches(sizes, budget):
    """[a, b) index ranges whose sizes add up to at most `budget` (an item larger than that goes alone)"""
    out, a, acc = [], 0, 0
    for i, s in enumerate(sizes):
        if i > a and acc + s > budget:
            out.append((a, i))
            a, acc = i, 0
        acc += s
    if a < len(sizes):
        out.append((a, len(sizes)))
    return out


def _table(lengths):
    """-> (numpy view of the item table: rows of in_off, out_off, in_len | out_cap << 32, reserved; the ctypes array over it)"""
    n = len(lengths)
    ln = np.asarray(lengths, dtype=np.uint64)
    if n and int(ln.max()) > 0xFFFFFFFF:
        raise OverflowError("a batch item is limited to 4 GiB - 1")
    tab = np.zeros((max(n, 1), 4), dtype=np.uint64)
    if n:
        tab[1:n, 0] = np.cumsum(ln)[:-1]
        tab[:n, 2] = ln
    return tab, (_lib.BatchItem * max(n, 1)).from_buffer(tab)


def _results(rs, n):
    r = np.frombuffer(rs, dtype=np.uint32, count=4 * max(n, 1)).reshape(-1, 4)[:n]
    return r[:, 0].view(np.int32).tolist(), r[:, 1].tolist()


def compress(items, level=Z_DEFAULT_COMPRESSION, wbits=MAX_WBITS, *, strategy=Z_DEFAULT_STRATEGY, zdict=None):
    """Compress every item of `items` (buffer-protocol objects) on its own: the i-th result equals zlib_ng.compress(items[i], level,
    wbits).  With a strategy, each result is the stream compressobj(level, DEFLATED, wbits, strategy=...) would write.  With zdict
    (a bytes-like; its last 32 KiB are the history of every item) each result is what compressobj(level, DEFLATED, wbits,
    DEF_MEM_LEVEL, strategy, zdict) writes for the item."""
    views = _views(items)
    if zdict is None:
        _z._check_level(level)
        _z._container(wbits)
        _check_strategy(strategy)
    else:
        zdict = _zdict_compress_args(level, wbits, strategy, zdict)
    if not views:
        return []
    ctx = _z._ctx()
    res = [None] * len(views)
    # with a dictionary an item of ZS_BATCH bytes or more is compressobj's, and every item is staged behind its own copy of the
    # dictionary's tail: a sub-batch is bounded by its primed bytes
    idx, sv, sizes = _split(views, None if zdict is None else ZS_BATCH)
    tl = 0 if zdict is None else min(len(zdict), 32768)
    for a, b in _sub_batches([s + tl for s in sizes] if tl else sizes, SUB_BATCH_BYTES):
        tab, items_c = _table(sizes[a:b])
        out, rs, _ = ctx.deflate_batch(b"".join(sv[a:b]), items_c, b - a, level, wbits, strategy, zdict=zdict)
        mv = memoryview(out)
        _, lens = _results(rs, b - a)
        for i, o, ln in zip(idx[a:b], tab[:b - a, 1].tolist(), lens):
            res[i] = bytes(mv[o:o + ln])
    if zdict is not None:
        for i, v in enumerate(views):
            if v.nbytes >= ZS_BATCH:
                c = _z.compressobj(level, _z.DEFLATED, wbits, _z.DEF_MEM_LEVEL, strategy, zdict)
                res[i] = c.compress(v) + c.flush()
    return res


def _raise_first(res, errors):
    if errors == "raise":
        for r in res:
            if isinstance(r, BaseException):
                raise r
    return res


def _with_index(exc, i):
    exc.index = i
    return exc


def decompress(items, wbits=MAX_WBITS, *, errors="raise", zdict=None):
    """Decompress every item of `items` on its own: the i-th result equals zlib_ng.decompress(items[i], wbits).  errors="raise" raises
    the one-shot's exception for the first failing item (its index in the exception's `index` attribute); errors="return" puts the
    exception in the failing items' slots instead.  With zdict, the i-th result is decompressobj(wbits, zdict=zdict)'s for the item
    (a zlib item with FDICT and a raw item decode with the dictionary; an unfinished stream is "incomplete or truncated stream")."""
    _check_errors(errors)
    views = _views(items)
    if zdict is None:
        _inflate_kind(wbits)
        large = lambda v: _z.decompress(v, wbits)
    else:
        zdict = _zdict_decompress_args(wbits, zdict)
        large = lambda v: _zdict_reference(v, wbits, zdict)
    if not views:
        return []
    ctx = _z._ctx()
    res = [None] * len(views)
    idx, sv, sizes = _split(views, LARGE_ITEM)
    for a, b in _sub_batches(sizes, SUB_BATCH_BYTES):
        tab, items_c = _table(sizes[a:b])
        out, rs = ctx.inflate_batch(b"".join(sv[a:b]), items_c, b - a, wbits, zdict=zdict)
        mv = memoryview(out)
        sts, lens = _results(rs, b - a)
        for i, o, st, ln in zip(idx[a:b], tab[:b - a, 1].tolist(), sts, lens):
            res[i] = bytes(mv[o:o + ln]) if st == _lib.BATCH_OK else _with_index(status_error(st), i)
    for i, v in enumerate(views):
        if v.nbytes >= LARGE_ITEM:
            try:
                res[i] = large(v)
            except Exception as e:          # the single-stream path's own verdict, as the one-shot gives it
                res[i] = _with_index(e, i)
    return _raise_first(res, errors)


# ---- device-resident forms
def _unit_bound(n, strategy):
    """the most bytes a unit of n bytes takes in a packed stream: unit_bound of zng_amd.hip"""
    return n + (n // 8 if strategy == _lib.STRATEGY_FIXED else 0) + 32


def _frame_bound(lengths, wbits, zdict=None, strategy=Z_DEFAULT_STRATEGY):
    """room that compress_dev's output never exceeds: every item's framing and the bound of each unit it is cut into (units of
    16 KiB up to 128 KiB, of 128 KiB beyond)"""
    kind, _ = _z._container(wbits)
    ovh = (6 if zdict is None else 10) if kind == "zlib" else 18 if kind == "gzip" else 0
    total = 64
    for ln in lengths:
        u = 16384 if ln <= 131072 else 131072
        full, rest = divmod(ln, u)
        total += full * _unit_bound(u, strategy) + (_unit_bound(rest, strategy) if rest or not full else 0) + ovh
    return total


def compress_dev(ctx, d_in, offsets, lengths, level=Z_DEFAULT_COMPRESSION, wbits=MAX_WBITS, *, strategy=Z_DEFAULT_STRATEGY, zdict=None):
    """Items that lie in device memory (d_in: a DeviceBuffer holding BATCH_PAD readable bytes behind the last item) compressed into
    one new DeviceBuffer.  -> (buffer, out_offsets, out_lengths) (numpy uint64 arrays).  zdict: as compress (host bytes-like); the
    engine primes and compresses the items in ranges of bounded size."""
    from . import devmem
    if zdict is not None:
        zdict = _zdict_compress_args(level, wbits, strategy, zdict)
    _z._check_level(level)
    _z._container(wbits)
    _check_strategy(strategy)
    offsets = np.asarray(offsets, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.uint64)
    n = len(offsets)
    if len(lengths) != n:
        raise ValueError("offsets and lengths differ in length")
    in_len = max(0, d_in.nbytes - _lib.BATCH_PAD)
    items = (_lib.BatchItem * max(n, 1))()
    for i in range(n):
        items[i].in_off = int(offsets[i])
        items[i].in_len = int(lengths[i])
    cap = _frame_bound([int(x) for x in lengths], wbits, zdict, strategy)
    out = devmem.DeviceBuffer(ctx, cap)
    d_res = devmem.DeviceBuffer(ctx, 16 * max(n, 1))
    r, total = ctx.deflate_batch_dev(d_in.ptr, in_len, items, n, level, wbits, strategy, out.ptr, cap, d_res.ptr, zdict=zdict)
    if r != _lib.OK:
        raise _lib.EngineError(r, ctx.err())
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)[:n]
    offs = np.array([items[i].out_off for i in range(n)], dtype=np.uint64)
    return out, offs, res[:, 1].astype(np.uint64)


def decompress_dev(ctx, d_in, offsets, lengths, wbits=MAX_WBITS, *, zdict=None):
    """Items that lie in device memory (d_in: a DeviceBuffer holding BATCH_PAD readable bytes behind the last item) decompressed into
    one new DeviceBuffer: a count pass sizes every item, one decode writes it.  -> (buffer, out_offsets, out_lengths, statuses)
    (numpy arrays; statuses are ZNGAMD_BATCH_* codes or ZDICT_MISMATCH, see status_error).  zdict: as decompress."""
    from . import devmem
    if zdict is not None:
        zdict = _zdict_decompress_args(wbits, zdict)
    _inflate_kind(wbits)
    offsets = np.asarray(offsets, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.uint64)
    n = len(offsets)
    if len(lengths) != n:
        raise ValueError("offsets and lengths differ in length")
    in_len = max(0, d_in.nbytes - _lib.BATCH_PAD)
    tab = np.zeros((max(n, 1), 4), dtype=np.uint64)            # in_off, out_off, (in_len | out_cap << 32), reserved
    tab[:n, 0] = offsets
    tab[:n, 2] = lengths & 0xFFFFFFFF
    d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
    d_res = devmem.DeviceBuffer(ctx, 16 * max(n, 1))
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, n, wbits, True, None, 0, d_res.ptr, zdict=zdict)
    res = d_res.cpu().view(np.uint32).reshape(-1, 4)[:n]
    ok = res[:, 0] == _lib.BATCH_OK
    sizes = np.where(ok, res[:, 1], 0).astype(np.uint64)
    offs = np.zeros(n, dtype=np.uint64)
    if n:
        offs[1:] = np.cumsum(sizes)[:-1]
    total = int(sizes.sum())
    tab[:n, 1] = offs
    tab[:n, 2] = (lengths & 0xFFFFFFFF) | (sizes << np.uint64(32))
    d_tab[:] = tab.view(np.uint8).reshape(-1)
    out = devmem.DeviceBuffer(ctx, total + 64)
    ctx.inflate_batch_dev(d_in.ptr, in_len, d_tab.ptr, n, wbits, False, out.ptr, total, d_res.ptr, zdict=zdict)
    res2 = d_res.cpu().view(np.uint32).reshape(-1, 4)[:n]
    statuses = np.where(ok, res2[:, 0], res[:, 0]).astype(np.int32)
    lens = np.where(statuses == _lib.BATCH_OK, res2[:, 1], 0).astype(np.uint64)
    return out, offs, lens, statuses


# ---- dictionary training
def _train_args(lengths, dict_size, k, d):
    """the trainer's argument checks, made before any device call"""
    for v in (dict_size, k, d):
        if not isinstance(v, int):
            raise TypeError(f"an integer is required (got type {type(v).__name__})")
    if len(lengths) == 0:
        raise ValueError("no samples to train from")
    if not 4 <= d <= 8:
        raise ValueError(f"d must lie in [4, 8], not {d}")
    if not d <= k <= 16384:
        raise ValueError(f"k must lie in [d, 16384], not {k}")
    if not d <= dict_size <= 32768:
        raise ValueError(f"dict_size must lie in [d, 32768], not {dict_size}")
    total = int(sum(int(x) for x in lengths))
    if total < k:
        raise ValueError(f"the samples hold {total} bytes, fewer than k = {k}")
    if total >= 1 << 32:
        raise ValueError("the samples hold 4 GiB or more")


def train_dict(samples, dict_size=32768, *, k=256, d=8):
    """A preset dictionary of at most dict_size bytes trained from `samples` (buffer-protocol objects, taken in order): segments of
    k bytes chosen by the d-mers they share with all samples, the most useful last (shortest match distances).  The bytes depend
    only on the samples, their order and the parameters."""
    views = _views(samples)
    lengths = [v.nbytes for v in views]
    _train_args(lengths, dict_size, k, d)
    ctx = _z._ctx()
    _, items_c = _table(lengths)
    return ctx.train_dict(b"".join(views), items_c, len(views), dict_size, k, d)


def train_dict_dev(ctx, d_in, offsets, lengths, dict_size=32768, *, k=256, d=8):
    """train_dict on samples that lie in device memory (d_in: a DeviceBuffer holding BATCH_PAD readable bytes behind the last sample;
    offsets, lengths: the samples in it, in order).  -> the dictionary as bytes."""
    from . import devmem
    offsets = np.asarray(offsets, dtype=np.uint64)
    lengths = np.asarray(lengths, dtype=np.uint64)
    n = len(offsets)
    if len(lengths) != n:
        raise ValueError("offsets and lengths differ in length")
    _train_args(lengths, dict_size, k, d)
    in_len = max(0, d_in.nbytes - _lib.BATCH_PAD)
    if n and (int(offsets.max()) > in_len or bool(np.any(lengths > in_len - np.minimum(offsets, in_len)))):
        raise ValueError("a sample lies outside the device buffer")
    tab = np.zeros((n, 4), dtype=np.uint64)                    # in_off, out_off, in_len, reserved
    tab[:, 0] = offsets
    tab[:, 2] = lengths
    d_tab = devmem.from_host(ctx, tab.view(np.uint8).reshape(-1))
    r, out = ctx.train_dict_dev(d_in.ptr, in_len, d_tab.ptr, n, dict_size, k, d)
    if r != _lib.OK:
        raise ValueError(ctx.err())
    return out

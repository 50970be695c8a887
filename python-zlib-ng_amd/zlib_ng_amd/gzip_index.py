"""Random access into any gzip file: a seek-point index (as zlib's zran.c, indexed_gzip and gztool keep one) and the span-parallel
decoder behind it.

A seek point is a place where decoding can start again on its own:
  member point  the header of a gzip member (no history);
  block point   a deflate block header inside a member: its bit offset, the 32 KiB of output in front of it (the history the
                block may reference), and the member's CRC-32 and length up to there.
Each point owns the span of output that follows it, up to the next point:
  kernel span      deflate data from a block point, or from the first deflate byte behind a member point, to the next block point
                   of the same member or to the end of the member's final block -- decoded by za_k_inflate_spans, one wavefront per
                   span, all spans of a call in one launch, each checked against the CRC-32 the index recorded for it;
  member run       whole members between two member points (their trailers checked by the existing gunzip paths); a run of BGZF
                   or small members needs no windows.
A span never crosses gzip framing.

    idx = gzip_index.build("big.gz", spacing=1 << 20)
    idx.save("big.gz.zngi")
    idx = gzip_index.GzipIndex.load("big.gz.zngi")
    with open("big.gz", "rb") as f:
        piece = idx.read_at(f, 123456789, 4096)
    with gzip_ng.open("big.gz", index=idx) as f:      # seeks jump to the nearest point
        f.seek(-4096, 2); tail = f.read()

The file format ("Seek-point index"), all little-endian:
    header   72 bytes: magic b"ZNGAIDX\\0", version u32, record size u32, the data file's compressed size u64, CRC-32 of its first
             and of its last 64 KiB (u32 each), uncompressed size u64, spacing u64, number of points u64, raw and compressed length
             of the windows section u64 each
    points   n records of 72 bytes (_REC)
    windows  the windows of all block points concatenated, one zlib stream
    crc      CRC-32 of everything before it
An index is untrusted input that steers a kernel: load() checks every field (_validate) before anything reaches the device.
"""
import binascii
import bisect
import os
import struct

from . import _lib, zlib_ng

MAGIC = b"ZNGAIDX\0"
VERSION = 1
_HDR = struct.Struct("<8sIIQIIQQQQQ")
_REC = struct.Struct("<QQQQQQQIIII")   # in_bit data_bit end_bit out_off out_len win_off member_out win_len span_crc member_crc flags
BIND = 1 << 16                         # bytes at each end of the data file that the index is bound to
WIN = 32768

F_BLOCK = 1           # a block point (else a member point)
F_KERNEL = 2          # the span is decoded by the span kernel from data_bit to end_bit (else: whole members, in_bit .. end_bit)
F_FINAL = 4           # the span ends with its member's final block (end_bit = that end rounded up to a byte; the trailer follows)

# A lone span of at least this many output bytes goes through the chunk-parallel resume decoder (zngamd_inflate_resume with the
# point's window as dictionary) instead of one wavefront of the span kernel.  See DESIGN.md, "Seek-point index".
LONE_RESUME_MIN = 256 << 10


class Point:
    """One seek point and the span it owns."""
    __slots__ = ("in_bit", "data_bit", "end_bit", "out_off", "out_len", "win_off", "member_out", "win_len", "span_crc",
                 "member_crc", "flags")

    def __init__(self, *fields):
        for k, v in zip(self.__slots__, fields):
            setattr(self, k, v)

    def fields(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    @property
    def is_block(self):
        return bool(self.flags & F_BLOCK)

    @property
    def kernel(self):
        return bool(self.flags & F_KERNEL)

    def __repr__(self):
        kind = "block" if self.is_block else "member"
        return f"Point({kind}, bit {self.in_bit}, out {self.out_off}+{self.out_len}, window {self.win_len})"


def _binding(f, fsize):
    f.seek(0)
    head = f.read(min(BIND, fsize))
    f.seek(max(0, fsize - BIND))
    tail = f.read()
    return binascii.crc32(head) & 0xFFFFFFFF, binascii.crc32(tail) & 0xFFFFFFFF


def _open(file_or_path):
    if isinstance(file_or_path, (str, bytes, os.PathLike)):
        return open(file_or_path, "rb"), True
    return file_or_path, False


def _read(f, off, n):
    f.seek(off)
    b = f.read(n)
    if len(b) != n:
        raise zlib_ng.BadGzipFile("the data file is shorter than its index says")
    return b


def _validate(points, size, fsize, win_raw):
    """The structural checks of an untrusted index (ValueError): offsets inside the file and in order, spans that tile the output,
    windows inside the windows section and no longer than 32 KiB."""
    fbits = fsize * 8
    out = 0
    prev_end = 0
    for i, p in enumerate(points):
        if p.flags & ~(F_BLOCK | F_KERNEL | F_FINAL):
            raise ValueError(f"index point {i}: unknown flags {p.flags:#x}")
        if p.out_off != out:
            raise ValueError(f"index point {i}: output offset {p.out_off} where {out} was expected")
        if p.in_bit < prev_end:
            raise ValueError(f"index point {i}: compressed offsets are not monotonic")
        if not p.in_bit <= p.data_bit < p.end_bit <= fbits:
            raise ValueError(f"index point {i}: bit offsets out of order or beyond the file")
        if p.win_len > WIN:
            raise ValueError(f"index point {i}: window of {p.win_len} bytes")
        if p.win_off > win_raw or win_raw - p.win_off < p.win_len:
            raise ValueError(f"index point {i}: window beyond the windows section")
        if p.is_block:
            if not p.kernel or p.data_bit != p.in_bit or p.win_len != min(WIN, p.member_out):
                raise ValueError(f"index point {i}: inconsistent block point")
        else:
            if p.in_bit & 7 or p.win_len or p.member_out or p.member_crc:
                raise ValueError(f"index point {i}: inconsistent member point")
            if p.kernel:
                if p.data_bit & 7 or p.data_bit - p.in_bit < 80:
                    raise ValueError(f"index point {i}: deflate data inside the member header")
            elif p.data_bit != p.in_bit or p.end_bit & 7 or p.flags & F_FINAL:
                raise ValueError(f"index point {i}: inconsistent member run")
        if p.kernel and p.out_len > 0xFFFFFFFF:
            raise ValueError(f"index point {i}: span of {p.out_len} bytes")
        if p.kernel and not p.flags & F_FINAL:
            # the span stops at the next point, a block point of the same member
            if i + 1 == len(points) or not points[i + 1].is_block or points[i + 1].in_bit != p.end_bit:
                raise ValueError(f"index point {i}: span does not end at the next point")
            if points[i + 1].member_out != p.member_out + p.out_len:
                raise ValueError(f"index point {i}: member length does not continue at the next point")
        if p.is_block and (i == 0 or not points[i - 1].kernel or points[i - 1].flags & F_FINAL):
            raise ValueError(f"index point {i}: block point not preceded by a span of its member")
        out += p.out_len
        prev_end = p.end_bit
    if out != size:
        raise ValueError(f"spans sum to {out} bytes, the index says {size}")


class GzipIndex:
    """Seek points of one gzip file (build() or GzipIndex.load()); see the module's docstring."""

    def __init__(self, points, size, spacing, fsize, bind, windows=None, windows_z=None, win_raw=0):
        self.points = points
        self.size = size
        self.spacing = spacing
        self.file_size = fsize
        self._bind = bind
        self._windows = windows            # raw windows (bytes), or None until the compressed section is first needed
        self._windows_z = windows_z
        self._win_raw = win_raw if windows is None else len(windows)
        self._starts = [p.out_off for p in points]

    # ---- file format
    def to_bytes(self):
        wz = self._windows_z if self._windows_z is not None else zlib_ng.compress(self._windows, 6)
        hdr = _HDR.pack(MAGIC, VERSION, _REC.size, self.file_size, self._bind[0], self._bind[1], self.size, self.spacing,
                        len(self.points), self._win_raw, len(wz))
        body = hdr + b"".join(_REC.pack(*p.fields()) for p in self.points) + wz
        return body + struct.pack("<I", binascii.crc32(body) & 0xFFFFFFFF)

    def save(self, path_or_file):
        blob = self.to_bytes()
        if hasattr(path_or_file, "write"):
            path_or_file.write(blob)
        else:
            with open(path_or_file, "wb") as f:
                f.write(blob)

    @classmethod
    def from_bytes(cls, blob):
        blob = bytes(blob)
        if len(blob) < _HDR.size + 4:
            raise ValueError("gzip index: too short")
        if binascii.crc32(blob[:-4]) & 0xFFFFFFFF != struct.unpack_from("<I", blob, len(blob) - 4)[0]:
            raise ValueError("gzip index: CRC mismatch")
        magic, ver, rsize, fsize, ch, ct, size, spacing, n, win_raw, win_z = _HDR.unpack_from(blob, 0)
        if magic != MAGIC:
            raise ValueError("gzip index: bad magic")
        if ver != VERSION or rsize != _REC.size:
            raise ValueError(f"gzip index: unsupported version {ver}")
        if n > len(blob) or _HDR.size + n * _REC.size + win_z + 4 != len(blob):
            raise ValueError("gzip index: record count and length disagree")
        points = [Point(*_REC.unpack_from(blob, _HDR.size + i * _REC.size)) for i in range(n)]
        _validate(points, size, fsize, win_raw)
        off = _HDR.size + n * _REC.size
        return cls(points, size, spacing, fsize, (ch, ct), windows_z=blob[off:off + win_z], win_raw=win_raw)

    @classmethod
    def load(cls, path_or_file):
        if hasattr(path_or_file, "read"):
            return cls.from_bytes(path_or_file.read())
        with open(path_or_file, "rb") as f:
            return cls.from_bytes(f.read())

    def _window_bytes(self):
        if self._windows is None:
            raw = zlib_ng.decompress(self._windows_z) if self._windows_z else b""
            if len(raw) != self._win_raw:
                raise ValueError("gzip index: the windows section has the wrong length")
            self._windows = raw
        return self._windows

    def window(self, i):
        p = self.points[i]
        return self._window_bytes()[p.win_off:p.win_off + p.win_len]

    # ---- reading
    def check_file(self, f):
        """ValueError unless `f` is the file this index was built for (size and CRC-32 of its first and last 64 KiB)."""
        fsize = f.seek(0, 2)
        if fsize != self.file_size or _binding(f, fsize) != tuple(self._bind):
            raise ValueError("gzip index: the index belongs to another file")

    def point_for(self, offset):
        """Index of the last point whose span starts at or before `offset` (spans of no output are passed over)."""
        i = max(0, bisect.bisect_right(self._starts, offset) - 1)
        while i > 0 and self.points[i].out_len == 0 and self.points[i].out_off == offset:
            i -= 1
        return i

    def _spans_for(self, o, n):
        if n <= 0 or o >= self.size:
            return []
        i = bisect.bisect_right(self._starts, o) - 1
        got = []
        while i < len(self.points) and self.points[i].out_off < o + n:
            if self.points[i].out_len:
                got.append(i)
            i += 1
        return got

    def _decode(self, f, idxs):
        """{point index: its span's output, verified}; every kernel span of the call in one launch."""
        ctx = zlib_ng._ctx()
        res = {}
        for i in idxs:
            p = self.points[i]
            if not p.kernel and p.out_len:
                res[i] = self._decode_run(ctx, f, p)
        kern = [i for i in idxs if self.points[i].kernel]
        if len(kern) == 1 and self.points[kern[0]].out_len >= LONE_RESUME_MIN:
            out = self._decode_resume(ctx, f, kern[0])
            if out is not None:
                res[kern[0]] = out
                return res
        if kern:
            out, offs = self._launch(ctx, f, kern, False)
            mv = memoryview(out)
            for i, o in zip(kern, offs):
                res[i] = mv[o:o + self.points[i].out_len]
        return res

    def _decode_run(self, ctx, f, p):
        data = _read(f, p.in_bit >> 3, (p.end_bit - p.in_bit) >> 3)
        code, out, _ = ctx.gunzip(data, p.out_len)
        if code != _lib.OK or len(out) != p.out_len:
            raise zlib_ng.BadGzipFile(f"gzip members at byte {p.in_bit >> 3} do not decode to the {p.out_len} bytes the index records"
                                      f" ({ctx.err() or code})")
        return out

    def _launch(self, ctx, f, kern, placed):
        """One zngamd_inflate_spans call for the kernel spans `kern` (ascending) -> (output, offset of each span in it).  Spans whose
        compressed bytes touch are read from the file in one piece; placed: every span's output lies at its own out_off (an output
        of self.size bytes, what decompress() hands out as it is)."""
        pts = self.points
        nblock = sum(1 for i in kern if pts[i].win_len)
        whole_win = nblock * 2 >= len(pts)             # most windows are needed: the section goes up as it is, no packing
        wins = self._window_bytes() if nblock else b""
        spans = (_lib.Span * len(kern))()
        pieces, wparts, offs = [], [], []
        base = -1                                      # file byte that the current piece starts at ...
        cur = 0                                        # ... and where that piece starts in the packed input
        run_end = -1
        wcur = ocur = 0
        for j, i in enumerate(kern):
            p = pts[i]
            first, last = p.data_bit >> 3, (p.end_bit + 7) >> 3
            if first > run_end or first < base:        # (not adjacent to the piece being gathered: a new piece)
                if run_end >= 0:
                    pieces.append(_read(f, base, run_end - base))
                    cur += run_end - base
                base, run_end = first, last
            else:
                run_end = max(run_end, last)
            rel = (cur + first - base) * 8
            if whole_win:
                wo = p.win_off
            else:
                wo = wcur
                wparts.append(wins[p.win_off:p.win_off + p.win_len])
                wcur += p.win_len
            oo = p.out_off if placed else ocur
            spans[j] = _lib.Span(rel + (p.data_bit & 7), rel + (p.end_bit - first * 8), wo, oo, p.win_len, p.out_len, p.span_crc, 0)
            offs.append(oo)
            ocur += p.out_len
        pieces.append(_read(f, base, run_end - base))
        packed = pieces[0] if len(pieces) == 1 else b"".join(pieces)
        wbuf = wins if whole_win else b"".join(wparts)
        status, out = ctx.inflate_spans(packed, spans, wbuf, self.size if placed else ocur)
        bad = [(kern[j], s) for j, s in enumerate(status) if s != _lib.SPAN_OK]
        if bad:
            i, s = bad[0]
            what = {_lib.SPAN_DATA: "invalid deflate data", _lib.SPAN_LENGTH: "wrong length", _lib.SPAN_CRC: "CRC mismatch"}.get(s, s)
            raise zlib_ng.BadGzipFile(f"span at bit {pts[i].data_bit}: {what} ({len(bad)} of {len(kern)} spans failed)")
        return out, offs

    def _decode_resume(self, ctx, f, i):
        """One span through zngamd_inflate_resume (chunk-parallel for large pieces), checked against the span's CRC-32; None when
        that decoder stops short of the span's end (it keeps back what follows the last block it knows to be complete)."""
        p = self.points[i]
        first, last = p.data_bit >> 3, (p.end_bit + 7) >> 3
        if i + 1 < len(self.points) and self.points[i + 1].kernel and not p.flags & F_FINAL:
            last = (self.points[i + 1].end_bit + 7) >> 3          # (the next span's bytes too: the span's last block is then complete)
        data = _read(f, first, last - first)
        code, out, _, _, _ = ctx.inflate_resume(data, p.data_bit & 7, self.window(i), p.out_len)
        if len(out) < p.out_len:
            return None
        if ctx.crc32(memoryview(out)[:p.out_len]) != p.span_crc:
            raise zlib_ng.BadGzipFile(f"span at bit {p.data_bit}: does not decode to the bytes the index records")
        return out[:p.out_len]

    def read_ranges(self, file, ranges):
        """[bytes of (offset, n) for each range]: every span any range needs is decoded once (short at the end of the data)."""
        ranges = [(int(o), int(n)) for o, n in ranges]
        for o, n in ranges:
            if o < 0 or n < 0:
                raise ValueError("offsets and lengths must not be negative")
        f, close = _open(file)
        try:
            self.check_file(f)
            need = sorted({i for o, n in ranges for i in self._spans_for(o, n)})
            got = self._decode(f, need) if need else {}
        finally:
            if close:
                f.close()
        outs = []
        for o, n in ranges:
            parts = []
            for i in self._spans_for(o, n):
                p = self.points[i]
                a = max(o, p.out_off) - p.out_off
                b = min(o + n, p.out_off + p.out_len) - p.out_off
                parts.append(bytes(got[i][a:b]))
            outs.append(b"".join(parts))
        return outs

    def read_at(self, file, offset, n):
        """`n` bytes of the uncompressed data at `offset` (fewer at the end)."""
        return self.read_ranges(file, [(offset, n)])[0]

    def decompress(self, file):
        """The whole uncompressed data: every kernel span in one launch (each decoded into its own place of the result), member
        runs through the gunzip paths."""
        f, close = _open(file)
        try:
            self.check_file(f)
            ctx = zlib_ng._ctx()
            kern = [i for i, p in enumerate(self.points) if p.kernel and p.out_len]
            runs = [i for i, p in enumerate(self.points) if not p.kernel and p.out_len]
            out = self._launch(ctx, f, kern, True)[0] if kern else b""
            if not runs:
                return out if kern else b""
            whole = bytearray(self.size)
            if kern:
                whole[:] = out
            for i in runs:
                p = self.points[i]
                whole[p.out_off:p.out_off + p.out_len] = self._decode_run(ctx, f, p)
            return bytes(whole)
        finally:
            if close:
                f.close()

def build(file_or_path, spacing=1 << 20):
    """Seek points about every `spacing` uncompressed bytes of a gzip file of any writer (single or many members, BGZF, this
    package's writers, any header fields, NUL padding between members).  The file is read once through the engine's windowed
    reader (zngamd_gunzip_stream), with compressed windows sized from the observed ratio; its state after every call that ends
    inside a member is a block point, a call that ends at a member boundary gives a member point."""
    if spacing < 4096:
        raise ValueError("spacing must be at least 4096 bytes")
    f, close = _open(file_or_path)
    try:
        return _build(f, int(spacing))
    finally:
        if close:
            f.close()


def _build(f, spacing):
    ctx = zlib_ng._ctx()
    fsize = f.seek(0, 2)
    bind = _binding(f, fsize)
    st = _lib.GzState()
    points, wins = [], bytearray()
    pos, total, ratio = 0, 0, 8.0
    grow = 1
    while pos < fsize:
        if not st.in_member:
            # NUL padding between members (gzip(1) skips it; the windowed reader does so inside a window only)
            f.seek(pos)
            while pos < fsize:
                probe = f.read(min(1 << 16, fsize - pos))
                z = len(probe) - len(probe.lstrip(b"\0"))
                pos += z
                if z < len(probe):
                    break
            if pos >= fsize:
                break
        want = max(4096, int(spacing / ratio)) * grow
        data = _read(f, pos, min(want, fsize - pos))
        last = pos + len(data) >= fsize
        was_member, bit0 = bool(st.in_member), pos * 8 + st.start_bit
        win = bytes(st.window[:st.window_len]) if was_member else b""
        mcrc, mout = (st.crc, st.out_total) if was_member else (0, 0)
        cap = max(1 << 16, 8 * len(data))
        while True:
            code, out, nm, used = ctx.gunzip_stream(st, data, cap, last)
            if code == _lib.BUF_ERROR and (len(out) >= cap or ctx.last_needed > cap):
                cap = max(cap * 4, ctx.last_needed + 64)
                continue
            break
        if code != _lib.OK:
            raise zlib_ng.BadGzipFile(f"gzip data at byte {pos} does not decode: {ctx.err() or code}")
        if used == 0:
            if last:
                raise zlib_ng.BadGzipFile(f"gzip data at byte {pos} does not end")
            grow *= 2                       # not one complete block or member in the window
            continue
        grow = 1
        n = len(out)
        crc = ctx.crc32(out) if n else 0
        if was_member:
            flags = F_BLOCK | F_KERNEL
            if st.in_member:
                end = (pos + used) * 8 + st.start_bit
            else:
                flags |= F_FINAL
                end = _trailer(data, used, ctx.crc32_combine(mcrc, crc, n) if mout else crc, (mout + n) & 0xFFFFFFFF, pos) * 8
            points.append(Point(bit0, bit0, end, total, n, len(wins), mout, len(win), crc, mcrc, flags))
            wins += win
        elif st.in_member:
            # the member's first blocks: from its first deflate byte, no history
            doff = zlib_ng._parse_gzip_header(data)
            points.append(Point(pos * 8, (pos + doff) * 8, (pos + used) * 8 + st.start_bit, total, n, len(wins), 0, 0, crc, 0, F_KERNEL))
        else:
            points.append(Point(pos * 8, pos * 8, (pos + used) * 8, total, n, len(wins), 0, 0, crc, 0, 0))
        total += n
        pos += used
        if n:
            # (an estimate too high costs only points closer together; one too low, gaps wider than `spacing`)
            ratio = max(n / used, 0.75 * ratio if len(points) > 1 else 1.0)
    return GzipIndex(points, total, spacing, fsize, bind, windows=bytes(wins))


def _trailer(data, used, crc, isize, pos):
    """Byte offset (in the file) of the trailer of the member that ended inside `data` (the reader consumed `used` bytes: the
    trailer and any NUL padding behind it)."""
    want = struct.pack("<II", crc & 0xFFFFFFFF, isize)
    t = used - 8
    while t >= 0:
        if bytes(data[t:t + 8]) == want:
            return pos + t
        if data[t + 7] != 0:
            break
        t -= 1
    raise zlib_ng.BadGzipFile(f"gzip member trailer not found before byte {pos + used}")

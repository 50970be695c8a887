"""BGZF -- the blocked gzip of htslib, samtools, tabix and `bgzip` (SAM specification section 4.1) on the MI355X engine: written on
the GPU, addressed by virtual offset, read in ranges.

A BGZF file is a series of gzip members ("blocks") of at most 64 KiB, each holding at most 65 280 bytes of input as a deflate stream
of its own and its own size in a 'B','C' extra subfield; it ends with an empty block of 28 fixed bytes.  Every gzip reader reads it as
an ordinary multi-member file.  A position in it is a virtual offset, `coffset << 16 | uoffset`: the file offset of a block and a byte
offset inside that block's output -- what .bai, .tbi and .csi indexes store, and all a reader needs to start there.

    blob = bgzf.compress(data)                       # one shot; gzip.decompress(blob) == data
    with bgzf.open("reads.fastq.gz", "wb") as w:     # BgzfWriter: batches of whole blocks through the deflate kernels
        w.write(header); at = w.tell(); w.write(records)
        w.write_gzi("reads.fastq.gz.gzi")            # after close(): the whole table
    with bgzf.open("reads.fastq.gz") as r:           # BgzfReader
        r.seek(at); first = r.read(100)
        pieces = r.read_ranges([(v0, 100), (v1, 4096)])      # every needed block decoded once, one launch; only the bytes asked
                                                             # for come back from the device

The .gzi index (`GziIndex`) maps uncompressed offsets to blocks.  On disk, little-endian: a u64 count, then for every data block
AFTER the first a pair of u64 (compressed offset, uncompressed offset).  save() writes no entry for the EOF block; load() accepts a
file whose last entry points at it.  An index is untrusted: load() and the reader check it before it steers a read.
"""
import bisect
import io
import os
import struct

import numpy as np

from . import _lib, devmem, zlib_ng

__all__ = ["open", "compress", "compress_dev", "decompress", "make_virtual_offset", "split_virtual_offset", "BgzfReader", "BgzfWriter",
           "GziIndex", "BadGzipFile", "EOF_BLOCK", "MAX_BLOCK_INPUT"]

BadGzipFile = zlib_ng.BadGzipFile
MAX_BLOCK_INPUT = 65280                       # htslib's 0xff00
MAX_BLOCK = 65536
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MEMBER_DTYPE = np.dtype([("in_off", "<u8"), ("in_len", "<u8"), ("out_off", "<u8"), ("out_len", "<u4"), ("crc", "<u4"), ("index_off", "<u4"),
                         ("nseg", "<u4")])                                                               # zngamd_member
SLICE_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("len", "<u4"), ("reserved", "<u4")])   # zngamd_bgzf_slice
BLOCK_DTYPE = np.dtype([("coffset", "<u8"), ("uoffset", "<u8"), ("csize", "<u4"), ("isize", "<u4")])      # zngamd_bgzf_block
_WRITE_BATCH = (64 << 20) // MAX_BLOCK_INPUT * MAX_BLOCK_INPUT      # input bytes per engine call of the writer: about 64 MiB
_READ_WINDOW = 32 << 20                       # compressed bytes per window of the sequential reader
_builtin_open = open


def make_virtual_offset(coffset, uoffset):
    """coffset << 16 | uoffset; ValueError unless 0 <= coffset < 2**48 and 0 <= uoffset < 65536"""
    coffset, uoffset = int(coffset), int(uoffset)
    if not 0 <= coffset < 1 << 48:
        raise ValueError(f"compressed offset {coffset} outside [0, 2**48)")
    if not 0 <= uoffset < 1 << 16:
        raise ValueError(f"offset {uoffset} inside a block outside [0, 65536)")
    return coffset << 16 | uoffset


def split_virtual_offset(voffset):
    """-> (coffset, uoffset); ValueError unless 0 <= voffset < 2**64"""
    voffset = int(voffset)
    if not 0 <= voffset < 1 << 64:
        raise ValueError(f"virtual offset {voffset} outside [0, 2**64)")
    return voffset >> 16, voffset & 0xFFFF


def _check_block_size(block_size):
    if not 1 <= int(block_size) <= MAX_BLOCK_INPUT:
        raise ValueError(f"block_size must be 1..{MAX_BLOCK_INPUT}")
    return int(block_size)


def compress(data, level=6, *, block_size=MAX_BLOCK_INPUT, eof=True):
    """`data` as one BGZF stream (with the EOF block unless eof=False)."""
    return zlib_ng._ctx().bgzf_compress(zlib_ng._view(data), _check_block_size(block_size), level, eof)[0]


def compress_dev(ctx, d_in, n, level=6, *, block_size=MAX_BLOCK_INPUT, eof=True, out=None, table=True):
    """Device-resident: d_in (a devmem.DeviceBuffer or a device address) holds n bytes.  -> (DeviceBuffer with the stream, its bytes,
    block table as a numpy array of BLOCK_DTYPE with the EOF block's row).  out: a DeviceBuffer of at least ctx.bgzf_room(n, block_size)
    bytes to write into (a caller that compresses batch after batch allocates once); table=False: no table is fetched (None)."""
    block_size = _check_block_size(block_size)
    rows = (n + block_size - 1) // block_size + 1
    if out is None:
        out = devmem.empty(ctx, ctx.bgzf_room(n, block_size))
    d_tab = devmem.empty(ctx, rows * BLOCK_DTYPE.itemsize) if table else None
    src = d_in.ptr if isinstance(d_in, devmem.DeviceBuffer) else int(d_in)
    nbytes, nrows = ctx.bgzf_compress_dev(src, n, block_size, level, eof, out.ptr, out.nbytes, d_tab.ptr if table else 0)
    tab = d_tab[:nrows * BLOCK_DTYPE.itemsize].cpu(BLOCK_DTYPE) if table else None
    return out, nbytes, tab


def _scan_error(code, block_no, offset):
    if code == _lib.E_BGZF and offset == 0:
        return BadGzipFile("Not a BGZF file (no block header with a 'BC' subfield at the start)")
    return BadGzipFile(f"BGZF block {block_no} at offset {offset}: bad block header or block size")


def _cut_block(data):
    """the bytes at the end of a file start a block that the file does not hold to its end"""
    if len(data) < 18:
        return EOF_BLOCK[:4].startswith(bytes(data[:4]))
    return bytes(data[:4]) == EOF_BLOCK[:4] and bytes(data[10:16]) == EOF_BLOCK[10:16] and struct.unpack_from("<H", data, 16)[0] + 1 > len(data)


def _decode_blocks(ctx, data, total, block_no, offset, blocks):
    """all whole blocks of `data` in one launch (the engine's BGZF path: one wavefront per block, CRC-32 and ISIZE checked)"""
    code, out, nm = ctx.gunzip(data, total)
    if code != _lib.OK or len(out) != total:
        bad = min(nm, len(blocks) - 1)
        raise BadGzipFile(f"BGZF block {block_no + bad} at offset {offset + blocks[bad][0]}: {ctx.err() or code}")
    return out


def decompress(data):
    """The uncompressed bytes of a whole BGZF stream; BadGzipFile for data that is not BGZF or does not decode."""
    mv = zlib_ng._view(data)
    code, blocks, used, total = _lib.bgzf_scan(mv)
    if code != _lib.OK:
        raise _scan_error(code, len(blocks), used)
    if used != mv.nbytes:
        raise BadGzipFile(f"BGZF block {len(blocks)} at offset {used}: the data ends inside the block")
    if total == 0:
        return b""
    return _decode_blocks(zlib_ng._ctx(), mv, total, 0, 0, blocks)


def open(filename, mode="rb", compresslevel=6, encoding=None, errors=None, newline=None, **kwargs):
    """"rb" -> BgzfReader, "wb" / "ab" (and "xb") -> BgzfWriter; text modes wrap them in a TextIOWrapper, as gzip_ng.open does."""
    text = "t" in mode
    if text and "b" in mode:
        raise ValueError("Invalid mode: %r" % (mode,))
    if not text:
        for name, val in (("encoding", encoding), ("errors", errors), ("newline", newline)):
            if val is not None:
                raise ValueError(f"Argument '{name}' not supported in binary mode")
    raw = mode.replace("t", "").replace("b", "")
    if raw in ("r", ""):
        fobj = BgzfReader(filename, **kwargs)
    elif raw in ("w", "a", "x"):
        fobj = BgzfWriter(filename, raw + "b", compresslevel, **kwargs)
    else:
        raise ValueError("Invalid mode: %r" % (mode,))
    return io.TextIOWrapper(fobj, encoding, errors, newline) if text else fobj


def _is_path(obj):
    return isinstance(obj, (str, bytes, os.PathLike))


class GziIndex:
    """The .gzi index of a BGZF file: (compressed offset, uncompressed offset) of every data block after the first."""

    def __init__(self, entries=(), file_size=None):
        self.entries = [(int(c), int(u)) for c, u in entries]
        self.validate(file_size)
        self._us = [u for _, u in self.entries]

    def validate(self, file_size=None):
        """ValueError unless the compressed offsets rise, the uncompressed ones do not fall, and (file_size given) every entry
        leaves room for a block inside the file."""
        pc, pu = 0, 0
        for i, (c, u) in enumerate(self.entries):
            if not pc < c < 1 << 48 or not pu <= u < 1 << 63:
                raise ValueError(f"gzi entry {i}: offsets ({c}, {u}) are not monotonic")
            if file_size is not None and c + len(EOF_BLOCK) > file_size:
                raise ValueError(f"gzi entry {i}: compressed offset {c} beyond the file ({file_size} bytes)")
            pc, pu = c, u

    @classmethod
    def from_blocks(cls, blocks, file_size=None):
        """From a block table [(coffset, uoffset, block bytes, isize), ...]; a final empty block (the EOF block) gets no entry."""
        blocks = list(blocks)
        if blocks and blocks[-1][3] == 0:
            blocks.pop()
        return cls([(b[0], b[1]) for b in blocks[1:]], file_size)

    @classmethod
    def build(cls, file):
        """Walk a BGZF file from block header to block header on the host (no GPU); BadGzipFile if it is not BGZF."""
        if _is_path(file):
            with _builtin_open(file, "rb") as f:
                return cls.build(f)
        blocks, fsize = _scan_file(file)
        return cls.from_blocks(blocks, fsize)

    def to_bytes(self):
        return struct.pack("<Q", len(self.entries)) + b"".join(struct.pack("<QQ", c, u) for c, u in self.entries)

    def save(self, path_or_file):
        if hasattr(path_or_file, "write"):
            path_or_file.write(self.to_bytes())
        else:
            with _builtin_open(path_or_file, "wb") as f:
                f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, blob, file_size=None):
        blob = bytes(blob)
        if len(blob) < 8:
            raise ValueError("gzi index: too short")
        n = struct.unpack_from("<Q", blob)[0]
        if n > len(blob) or 8 + 16 * n != len(blob):
            raise ValueError("gzi index: entry count and length disagree")
        return cls(struct.iter_unpack("<QQ", blob[8:]), file_size)

    @classmethod
    def load(cls, path_or_file, file_size=None):
        """file_size: the size of the BGZF file the index is for; entries beyond it are refused (a BgzfReader checks again)."""
        if hasattr(path_or_file, "read"):
            return cls.from_bytes(path_or_file.read(), file_size)
        with _builtin_open(path_or_file, "rb") as f:
            return cls.from_bytes(f.read(), file_size)

    def locate(self, uoffset):
        """-> (coffset of the last indexed block that starts at or before uoffset, bytes from its start)"""
        uoffset = int(uoffset)
        if uoffset < 0:
            raise ValueError("negative offset")
        i = bisect.bisect_right(self._us, uoffset) - 1
        return (0, uoffset) if i < 0 else (self.entries[i][0], uoffset - self.entries[i][1])

    def voffset(self, uoffset):
        """The virtual offset of uncompressed offset `uoffset` (ValueError when the index has no block within 64 KiB before it)."""
        c, within = self.locate(uoffset)
        return make_virtual_offset(c, within)

    def __eq__(self, other):
        return isinstance(other, GziIndex) and self.entries == other.entries

    def __len__(self):
        return len(self.entries)


def _scan_file(f):
    """-> (block table of the whole file, file size); BadGzipFile for anything that is not a complete run of BGZF blocks"""
    f.seek(0)
    blocks, base, ubase, tail = [], 0, 0, b""
    while True:
        chunk = f.read(_READ_WINDOW)
        data = tail + chunk if tail else chunk
        if not data:
            break
        code, tab, used, total = _lib.bgzf_scan(data)
        if not chunk and used < len(data) and _cut_block(data[used:]):
            raise BadGzipFile(f"BGZF block {len(blocks) + len(tab)} at offset {base + used}: the file ends inside the block")
        if code != _lib.OK and not (code == _lib.DATA_ERROR and not tab and chunk and len(data) < MAX_BLOCK):
            raise _scan_error(code if base + used == 0 else _lib.DATA_ERROR, len(blocks) + len(tab), base + used)
        blocks.extend((base + c, ubase + u, cs, isz) for c, u, cs, isz in tab)
        base, ubase, tail = base + used, ubase + total, data[used:]
        if not chunk:
            break
    return blocks, base


class BgzfWriter(io.BufferedIOBase):
    """Writes BGZF: input is collected and compressed in batches of whole blocks (about 64 MiB per engine call)."""

    def __init__(self, filename, mode="wb", compresslevel=6, *, block_size=MAX_BLOCK_INPUT):
        if mode.replace("b", "") not in ("w", "a", "x"):
            raise ValueError("Invalid mode: %r" % (mode,))
        if not _lib.load().zngamd_level_ok(compresslevel):
            raise ValueError("Bad compression level")
        self._bs = _check_block_size(block_size)
        self._level = compresslevel
        self.blocks = []                     # (coffset, uoffset, block bytes, isize) of every block written so far
        self._coffset = self._upos = 0
        self._own = _is_path(filename)
        if "a" in mode and self._own and os.path.exists(filename) and os.path.getsize(filename):
            # the table continues the file's: its blocks are walked once (host only)
            with _builtin_open(filename, "rb") as f:
                self.blocks, self._coffset = _scan_file(f)
            self._upos = sum(b[3] for b in self.blocks)
        self._fp = _builtin_open(filename, mode if "b" in mode else mode + "b") if self._own else filename
        if "a" in mode and not self._own:
            try:
                self._coffset = self._fp.seek(0, 2)
            except (OSError, ValueError, AttributeError):
                pass
        self._buf = bytearray()
        self._done = False
        self._ctx = zlib_ng._ctx()

    def writable(self):
        return True

    def _emit(self, n):
        """compress the first n pending bytes (whole blocks, or everything: the last block is then short) and write them"""
        if not n:
            return
        buf, ubase = self._buf, self._upos - len(self._buf)
        self._buf = bytearray(memoryview(buf)[n:])       # (less than a block: the batch itself is compressed where it lies)
        batch = max(1, _WRITE_BATCH // self._bs) * self._bs      # (whole blocks: only the last call of a flush ends short)
        with memoryview(buf) as mv:
            for pos in range(0, n, batch):
                with mv[pos:min(n, pos + batch)] as piece:
                    out, rows = self._ctx.bgzf_compress(piece, self._bs, self._level, eof=False)
                self._fp.write(out)
                self.blocks.extend((self._coffset + c, ubase + pos + u, cs, isz) for c, u, cs, isz in rows)
                self._coffset += len(out)

    def write(self, data):
        if self.closed:
            raise ValueError("write() on closed BgzfWriter object")
        mv = zlib_ng._view(data)
        self._buf += mv
        self._upos += mv.nbytes
        if len(self._buf) >= _WRITE_BATCH:
            self._emit(len(self._buf) // self._bs * self._bs)
        return mv.nbytes

    def flush(self):
        """End the current block short (as bgzf_flush does) and write everything pending."""
        if self.closed or self._done:
            return
        self._emit(len(self._buf))
        self._fp.flush()

    def tell(self):
        """The virtual offset of the next byte to be written: pending whole blocks go out, the partial block stays open."""
        self._emit(len(self._buf) // self._bs * self._bs)
        return make_virtual_offset(self._coffset, len(self._buf))

    def utell(self):
        return self._upos

    def close(self):
        if self.closed:
            return
        try:
            self._emit(len(self._buf))
            self._fp.write(EOF_BLOCK)
            self.blocks.append((self._coffset, self._upos, len(EOF_BLOCK), 0))
            self._coffset += len(EOF_BLOCK)
            self._fp.flush()
        finally:
            self._done = True
            if self._own:
                self._fp.close()
            super().close()

    def write_gzi(self, path_or_file):
        """Save the .gzi index of the blocks written so far."""
        GziIndex.from_blocks(self.blocks).save(path_or_file)


class BgzfReader(io.BufferedIOBase):
    """Reads BGZF sequentially, from a virtual offset, or in ranges.  require_eof: EOFError for a file that lacks the EOF block
    (htslib only warns, and so the default is to say nothing)."""

    def __init__(self, filename, *, require_eof=False):
        self._own = _is_path(filename)
        self._fp = _builtin_open(filename, "rb") if self._own else filename
        self._ctx = zlib_ng._ctx()
        self._require_eof = require_eof
        self._out, self._opos = b"", 0               # the decoded window and the read position in it
        self._wblocks, self._wstarts = [], []        # its blocks: (coffset in the file, offset in _out, isize); the offsets alone
        self._next_c = 0                             # file offset of the first block behind the window
        self._in_buf = self._in_mv = self._out_buf = None      # pooled buffers: the compressed window, the decoded one (buffer, address)
        self._tail_n = 0                             # compressed bytes behind _next_c at the front of the compressed window
        self._block_no = 0                           # number of the block at _next_c (counted from where reading began)
        self._skip = 0                               # bytes of the next block in front of the position (after a seek)
        self._upos = 0                               # uncompressed position, None when a seek by virtual offset lost it
        self._at_eof = self._saw_eof_block = False
        try:
            self._fsize = self._fp.seek(0, 2)
            self._fp.seek(0)
        except (OSError, ValueError, AttributeError):
            self._fsize = None
        if require_eof and self._fsize is not None:
            self._fp.seek(max(0, self._fsize - len(EOF_BLOCK)))
            last = self._fp.read(len(EOF_BLOCK))
            self._fp.seek(0)
            if last != EOF_BLOCK:
                self._close_fp()
                raise EOFError("BGZF file without the EOF block: it may be truncated")

    def readable(self):
        return True

    def seekable(self):
        return self._fsize is not None

    def _close_fp(self):
        if self._own:
            self._fp.close()

    def close(self):
        if not self.closed:
            self._drop_windows()
            self._close_fp()
            super().close()

    # ---- sequential
    def _read_into(self, mv):
        into = getattr(self._fp, "readinto", None)
        if into is not None:
            return into(mv) or 0
        chunk = self._fp.read(len(mv))
        mv[:len(chunk)] = chunk
        return len(chunk)

    def _drop_windows(self):
        """the window buffers go back to the process-wide pool (_lib.take_buffer): the next reader finds them warm"""
        self._out, self._in_mv = b"", None
        if self._in_buf is not None:
            _lib.give_buffer(self._in_buf)
        if self._out_buf is not None:
            _lib.give_buffer(self._out_buf[0])
        self._in_buf = self._out_buf = None

    def _fill(self):
        """Decode the next window: all whole blocks of it in one launch.  False at the end of the file.  The compressed window and
        the decoded one live in pooled buffers that are used again from window to window (fresh memory costs a page fault per 4 KiB)."""
        while not self._at_eof:
            if self._in_buf is None:
                self._win = _READ_WINDOW
                self._in_buf = _lib.take_buffer(self._win + MAX_BLOCK)
                self._in_mv = memoryview(self._in_buf)
            mv, have, ended = self._in_mv, self._tail_n, False
            if have < MAX_BLOCK:                     # (more than a block left over: only in front of a block that does not check out)
                got = self._read_into(mv[have:have + self._win])
                ended = got == 0
                have += got
            if have == 0:
                self._at_eof = True
                break
            data = mv[:have]
            code, tab, used, total = _lib.bgzf_scan(data)
            if ended and not tab and _cut_block(data):
                raise EOFError(f"BGZF block {self._block_no} at offset {self._next_c}: the file ends inside the block")
            if code != _lib.OK and not (code == _lib.DATA_ERROR and not tab and not ended and have < MAX_BLOCK):
                if not tab:
                    raise _scan_error(code if self._next_c == 0 else _lib.DATA_ERROR, self._block_no, self._next_c)
                # the whole blocks in front of the bad one are handed out first; the next window starts at it
            self._out = b""
            if total:
                if self._out_buf is None or len(self._out_buf[0]) < total:
                    if self._out_buf is not None:
                        _lib.give_buffer(self._out_buf[0])
                    self._out_buf = _lib.take_window(max(total, 4 * self._win))
                code2, n, nm = self._ctx.gunzip_into(data[:used], self._out_buf[1], total)
                if code2 != _lib.OK or n != total:
                    bad = min(nm, len(tab) - 1)
                    raise BadGzipFile(f"BGZF block {self._block_no + bad} at offset {self._next_c + tab[bad][0]}: {self._ctx.err() or code2}")
                self._out = memoryview(self._out_buf[0])[:total]
            if tab:
                self._saw_eof_block = tab[-1][2] == len(EOF_BLOCK) and tab[-1][3] == 0
            skip = self._skip
            if skip and tab:
                if skip > tab[0][3]:
                    raise ValueError(f"virtual offset points {skip} bytes into a block of {tab[0][3]}")
                self._skip = 0
            self._wblocks = [(self._next_c + c, u, isz) for c, u, cs, isz in tab if isz]
            self._wstarts = [b[1] for b in self._wblocks]
            self._opos = skip if tab else 0
            self._next_c += used
            self._block_no += len(tab)
            tail = bytes(data[used:have])
            mv[:len(tail)] = tail
            self._tail_n = len(tail)
            if self._opos < len(self._out):
                return True
        if self._require_eof and not self._saw_eof_block and self._fsize is None:
            raise EOFError("BGZF file without the EOF block: it may be truncated")
        return False

    def _take(self, n):
        """a view of the next bytes of the decoded window: valid until the next window is decoded"""
        mv = memoryview(self._out)[self._opos:self._opos + n]
        self._opos += len(mv)
        if self._upos is not None:
            self._upos += len(mv)
        return mv

    def read(self, size=-1):
        if self.closed:
            raise ValueError("read() on closed BgzfReader object")
        size = -1 if size is None else size
        parts, got = [], 0
        while size < 0 or got < size:
            if self._opos >= len(self._out) and not self._fill():
                break
            piece = bytes(self._take(len(self._out) if size < 0 else size - got))
            parts.append(piece)
            got += len(piece)
        return parts[0] if len(parts) == 1 else b"".join(parts)

    def read1(self, size=-1):
        if self._opos >= len(self._out) and not self._fill():
            return b""
        return bytes(self._take(len(self._out) if size is None or size < 0 else size))

    def readinto(self, b):
        mv = memoryview(b).cast("B")
        got = 0
        while got < len(mv):
            if self._opos >= len(self._out) and not self._fill():
                break
            piece = self._take(len(mv) - got)
            mv[got:got + len(piece)] = piece
            got += len(piece)
        return got

    # ---- positions
    def tell(self):
        """The virtual offset of the next byte (at the end of a block: the start of the next one, as htslib reports it)."""
        if self._opos < len(self._out):
            i = bisect.bisect_right(self._wstarts, self._opos) - 1
            c, start, _ = self._wblocks[i]
            return make_virtual_offset(c, self._opos - start)
        return make_virtual_offset(self._next_c, self._skip)

    def seek(self, voffset, whence=0):
        """Go to a virtual offset (whence must be 0).  Nothing is read until the next read."""
        if whence != 0:
            raise ValueError("a BGZF file is addressed by virtual offsets: whence must be 0")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        c, u = split_virtual_offset(voffset)
        if c > self._fsize:
            raise ValueError(f"compressed offset {c} beyond the file ({self._fsize} bytes)")
        self._fp.seek(c)
        self._out, self._opos, self._wblocks, self._wstarts, self._tail_n = b"", 0, [], [], 0
        self._next_c, self._skip, self._at_eof, self._upos, self._block_no = c, u, False, None, 0
        return voffset

    def utell(self):
        """The uncompressed offset of the next byte: known from the start of the file and after useek()."""
        if self._upos is None:
            raise ValueError("the uncompressed position is unknown after a seek by virtual offset: use useek()")
        return self._upos

    def useek(self, offset, gzi):
        """Go to uncompressed offset `offset` with a GziIndex of this file (checked against the file's size first)."""
        if self._fsize is not None:
            gzi.validate(self._fsize)
        c, within = gzi.locate(offset)
        self.seek(make_virtual_offset(c, 0))
        while within:                                # (more than a block only where the index is sparse)
            got = len(self.read(min(within, 1 << 24)))
            if not got:
                break
            within -= got
        self._upos = offset - within
        return self._upos

    # ---- ranges
    def _load_block(self, c, cache):
        if c not in cache:
            self._fp.seek(c)
            raw = self._fp.read(MAX_BLOCK)
            code, tab, used, total = _lib.bgzf_scan(raw, 1) if raw else (_lib.OK, [], 0, 0)
            if raw and (code != _lib.OK or not tab):
                raise BadGzipFile(f"BGZF block at offset {c}: bad block header or block size")
            cache[c] = (raw[:used], 12 + struct.unpack_from("<H", raw, 10)[0], tab[0][3]) if raw else None
        return cache[c]

    def read_ranges(self, ranges):
        """[bytes of (voffset, n) for each range] (short where the data ends).  A range may span blocks: the chain is followed from
        its first block through BSIZE.  Every needed block is decoded once, all of them in one launch; the slice kernel packs the
        requested bytes, and only those are copied back.  BadGzipFile if a block that a range touches does not check out."""
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        here = self._fp.tell()
        try:
            cache, plans = self._plan_ranges(ranges)
        finally:
            self._fp.seek(here)
        return self._read_planned(cache, plans)

    def _plan_ranges(self, ranges):
        """-> (blocks read from the file by offset, per range its pieces (coffset, from, to) in block order)"""
        cache, plans = {}, []
        for v, n in ranges:
            c, u = split_virtual_offset(v)
            n = int(n)
            if n < 0:
                raise ValueError("lengths must not be negative")
            pieces, first = [], True                  # (coffset, from, to) in block order
            while (n > 0 or first) and c < self._fsize:
                blk = self._load_block(c, cache)
                if blk is None:
                    break
                raw, hdr, isz = blk
                if first and u > isz:
                    raise ValueError(f"virtual offset points {u} bytes into a block of {isz}")
                take = min(n, isz - u)
                if take:
                    pieces.append((c, u, u + take))
                n -= take
                c, u, first = c + len(raw), 0, False
            plans.append(pieces)
        return cache, plans

    def _read_planned(self, cache, plans):
        need = sorted({p[0] for pieces in plans for p in pieces})
        if not need:
            return [b"" for _ in plans]
        raws = [cache[c][0] for c in need]
        members = np.zeros(len(need), MEMBER_DTYPE)
        lens = np.fromiter((len(r) for r in raws), np.uint64, len(need))
        hdrs = np.fromiter((cache[c][1] for c in need), np.uint64, len(need))
        members["out_len"] = np.fromiter((cache[c][2] for c in need), np.uint32, len(need))
        members["crc"] = np.fromiter((struct.unpack_from("<I", r, len(r) - 8)[0] for r in raws), np.uint32, len(need))
        members["in_off"] = np.cumsum(lens) - lens + hdrs
        members["in_len"] = lens - hdrs - 8
        opos = np.cumsum(members["out_len"], dtype=np.uint64) - members["out_len"]
        members["out_off"] = opos
        where = dict(zip(need, zip(range(len(need)), opos.tolist())))
        # the blocks of one range follow each other in the file, so their outputs follow each other in the scratch: a range is a slice
        slices = np.zeros(len(plans), SLICE_DTYPE)
        lns = np.fromiter((sum(b - a for _, a, b in pieces) for pieces in plans), np.uint64, len(plans))
        if len(lns) and int(lns.max()) >= 1 << 32:
            raise ValueError("a range is limited to 4 GiB - 1 bytes")
        slices["src_off"] = np.fromiter((where[pieces[0][0]][1] + pieces[0][1] if pieces else 0 for pieces in plans), np.uint64, len(plans))
        slices["len"] = lns
        dsts = np.cumsum(lns) - lns
        slices["dst_off"] = dsts
        spans = list(zip(dsts.tolist(), lns.tolist()))
        dst = int(lns.sum())
        status, sstat, out = self._ctx.bgzf_read(b"".join(raws), members, slices, dst)
        for i, s in enumerate(sstat):
            if s != _lib.BGZF_SLICE_OK:
                bad = [c for c, _, _ in plans[i] if status[where[c][0]] != 0]
                at = f"at offset {bad[0]}" if bad else "of the range"
                code = status[where[bad[0]][0]] if bad else s
                what = {-104: "CRC check failed", -105: "Incorrect length of data produced"}.get(code, "invalid deflate data")
                raise BadGzipFile(f"BGZF block {at}: {what} (range {i})")
        mv = memoryview(out)
        return [bytes(mv[a:a + ln]) for a, ln in spans]

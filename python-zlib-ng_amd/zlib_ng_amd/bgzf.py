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

    idx = bgzf.LineIndex.build("reads.fastq.gz")     # delimiters counted on the GPU, 32 bytes per block; idx.save(path) / load(path)
    with bgzf.open("reads.fastq.gz") as r:
        recs = r.read_lines(idx, [(40_000_000, 4000)])       # lines by number: planned on the index, one launch
        cuts = idx.shards(r, 8, lines_per_record=4)          # nine virtual offsets: eight parts that differ by at most one record

    hits = bgzf.grep("calls.vcf.gz", b"chr7\t", line_start=True)      # lines by content: matched on the GPU where the blocks were
    for number, voffset, line in zip(hits.numbers, hits.voffsets, hits):      # decoded; only the matching lines come back
        ...
    n = bgzf.grep("reads.fastq.gz", [b"ACGTTGCA", b"TGCAACGT"], count=True, start=cuts[2], stop=cuts[3])
    reads = bgzf.grep_records("reads.fastq.gz", b"ACGTTGCA", 4, match_line=1, first_byte=b"@")      # records by content: the reads whose
                                                                      # bases hold the barcode, all four lines of each, in the same one pass
    reads = bgzf.grep_records("reads.fastq.gz", b"GATTACAGATTACATC", 4, match_line=1, mismatches=1)      # ... with one base substituted at most

    tbi = bgzf.TabixIndex.build("calls.vcf.gz", "vcf")                # lines by region: the fields of every line are read on the GPU, a
    tbi.save("calls.vcf.gz.tbi")                                      # standard .tbi comes out; fetch() plans on it, decodes the blocks
    rows = bgzf.fetch("calls.vcf.gz", tbi, "chr7:55,000,000-55,200,000")      # of the region's chunks and filters their lines on the GPU

    fai = bgzf.FaidxIndex.build("ref.fa.gz")                          # bases by sequence: the records of a FASTA are read on the GPU;
    fai.save("ref.fa.gz.fai", "ref.fa.gz.gzi")                        # the standard pair of indexes comes out
    seqs = bgzf.fetch_seq("ref.fa.gz", fai, ["chr7:55,000,000-55,200,000", ("chrM", 0, 300)], reverse_complement=True)

The .gzi index (`GziIndex`) maps uncompressed offsets to blocks.  On disk, little-endian: a u64 count, then for every data block
AFTER the first a pair of u64 (compressed offset, uncompressed offset).  save() writes no entry for the EOF block; load() accepts a
file whose last entry points at it.  An index is untrusted: load() and the reader check it before it steers a read.
"""
import bisect
import contextlib
import hashlib
import io
import os
import struct
import weakref

import numpy as np

from . import _lib, devmem, zlib_ng

__all__ = ["open", "compress", "compress_dev", "decompress", "make_virtual_offset", "split_virtual_offset", "BgzfReader", "BgzfWriter",
           "GziIndex", "LineIndex", "BadGzipFile", "EOF_BLOCK", "MAX_BLOCK_INPUT", "grep", "grep_records", "GrepResult",
           "classify_records", "demux", "ClassifyResult", "UNASSIGNED", "AMBIGUOUS", "partition_records", "demux_paired", "pair_labels", "DROP", "trim_records", "TrimResult", "KEPT", "TOO_SHORT", "DROPPED", "qc_records", "QcResult",
           "key_records", "KeyResult", "pair_keys", "dedup_keys", "DedupResult", "dedup_records", "dedup_paired",
           "KmerSet", "ScreenResult", "screen_records", "screen_filter", "KmerCounter", "KmerCounts", "count_kmers",
           "SortKey", "SortKeyResult", "SortResult", "sort_key_records", "sort_keys", "permute_records", "sort_records",
           "overlap_records", "OverlapResult", "NONE", "FOUND", "MERGED", "TOO_LONG",
           "TabixIndex", "FetchResult", "fetch", "parse_region", "reg2bin", "reg2bins", "FaidxIndex", "SeqResult", "fetch_seq"]

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
_GREP_TEXT = 1 << 30                          # decoded bytes per window of grep at most (one engine call searches less than 4 GiB)
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


def _bsize_of(buf, start, end):
    """BSIZE + 1 of the header in buf[start:end) (the walk over the extra field's subfields); -1 without a 'B','C' subfield"""
    cur = start + 12
    while cur + 4 <= end:
        sl = int(buf[cur + 2]) | int(buf[cur + 3]) << 8
        if buf[cur] == 0x42 and buf[cur + 1] == 0x43 and sl == 2 and cur + 6 <= end:
            return (int(buf[cur + 4]) | int(buf[cur + 5]) << 8) + 1
        cur += 4 + sl
    return -1


def _member_table(buf, starts, csizes, isizes):
    """-> (member table (MEMBER_DTYPE) of the blocks that lie at `starts` in `buf`, a uint8 array, with their outputs packed in table
    order; -1, or the first row whose bytes are not a block of that size and ISIZE: no room in `buf`, no gzip header with the FEXTRA
    flag that fits the block, a BSIZE or an ISIZE that says otherwise)"""
    n = len(starts)
    members = np.zeros(n, MEMBER_DTYPE)
    if not n:
        return members, -1
    starts, csizes = starts.astype(np.int64), csizes.astype(np.int64)
    ends = starts + csizes
    ok = (csizes >= 26) & (starts >= 0) & (ends <= len(buf))
    at = np.where(ok, starts, 0)                             # (rows without room are judged already: they read the buffer's first bytes)
    if len(buf) < 26:
        return members, 0
    hdrs = 12 + buf[at + 10].astype(np.int64) + (buf[at + 11].astype(np.int64) << 8)
    ok &= (buf[at] == 0x1F) & (buf[at + 1] == 0x8B) & (buf[at + 2] == 8) & (buf[at + 3] & 4 != 0) & (csizes - hdrs >= 8)
    last = np.where(ok, ends, 26)
    trailer = buf[(last - 8)[:, None] + np.arange(8)].astype(np.uint32)
    ok &= (trailer[:, 4] | trailer[:, 5] << 8 | trailer[:, 6] << 16 | trailer[:, 7] << 24) == isizes.astype(np.uint32)
    # BSIZE: where the 'B','C' subfield is the only one (every writer's blocks), one gather; other headers are walked one by one
    plain = ok & (hdrs == 18) & (buf[at + 12] == 0x42) & (buf[at + 13] == 0x43) & (buf[at + 14] == 2) & (buf[at + 15] == 0)
    bsize = buf[at + 16].astype(np.int64) + (buf[at + 17].astype(np.int64) << 8) + 1
    ok &= ~plain | (bsize == csizes)
    for i in np.nonzero(ok & ~plain)[0].tolist():
        ok[i] = _bsize_of(buf, int(starts[i]), int(starts[i] + hdrs[i])) == int(csizes[i])
    if not bool(ok.all()):
        return members, int(np.argmin(ok))
    members["in_off"] = starts + hdrs
    members["in_len"] = csizes - hdrs - 8
    members["out_len"] = isizes
    members["out_off"] = np.cumsum(isizes, dtype=np.uint64) - isizes.astype(np.uint64)
    members["crc"] = trailer[:, 0] | trailer[:, 1] << 8 | trailer[:, 2] << 16 | trailer[:, 3] << 24
    return members, -1


def _block_error(offset, code, suffix=""):
    what = {-104: "CRC check failed", -105: "Incorrect length of data produced"}.get(int(code), "invalid deflate data")
    return BadGzipFile(f"BGZF block at offset {offset}: {what}{suffix}")


LINE_INDEX_MAGIC = b"ZNGLIDX\x01"              # the last byte is the format's version
LINE_ROW_DTYPE = np.dtype([("coffset", "<u8"), ("uoffset", "<u8"), ("before", "<u8"), ("flags", "<u4"), ("reserved", "<u4")])
_LINE_HEAD = struct.Struct("<8sIIQQQQQ")      # magic, delimiter, reserved, blocks, file size, end of the blocks, data bytes, delimiters
_STALE = "line index does not match the file"


class LineIndex:
    """Where the lines of a BGZF file are: per block (empty ones in the middle included, the EOF block at the end not) its offset in
    the file, the offset of its output in the data, the number of delimiter bytes in front of it and whether its last output byte is
    a delimiter.  A line number becomes a block and the ordinal of a delimiter inside it by arithmetic on these (locate); the
    delimiters themselves are counted, and found, on the GPU.  On disk (little-endian): LINE_INDEX_MAGIC, u32 delimiter, u32 0, u64
    blocks, u64 file size, u64 offset of the first byte behind the indexed blocks, u64 data bytes, u64 delimiters; then per block u64
    coffset, u64 uoffset, u64 delimiters in front, u32 flags (bit 0: the last byte is a delimiter), u32 0.  An index is untrusted:
    from_bytes() checks it, and a reader checks what it says against the file."""

    def __init__(self, rows, delimiter, file_size, cend, usize, delimiters):
        self._rows = np.ascontiguousarray(rows, LINE_ROW_DTYPE)
        self.delimiter = bytes(delimiter)
        self.file_size, self.cend, self.usize, self.delimiters = int(file_size), int(cend), int(usize), int(delimiters)
        self.validate()
        r, n = self._rows, len(self._rows)
        self._c = np.append(r["coffset"], np.uint64(self.cend)).astype(np.int64)
        self._u = np.append(r["uoffset"], np.uint64(self.usize)).astype(np.int64)
        self._before = r["before"].astype(np.int64)
        self._count = np.diff(np.append(self._before, self.delimiters))
        self._last = (r["flags"] & 1).astype(bool)
        self._isize = np.diff(self._u)
        nxt = np.where(self._isize > 0, np.arange(n), n)          # the first block at or behind i that holds data (n: none)
        self._next = np.append(np.minimum.accumulate(nxt[::-1])[::-1], n) if n else np.array([0])
        full = np.nonzero(self._isize > 0)[0]
        self._tail = int(full[-1]) if len(full) else -1           # the last block that holds data
        self.lines = self.delimiters + (1 if self._tail >= 0 and not self._last[self._tail] else 0)

    def validate(self, file_size=None):
        """ValueError unless the rows describe blocks that follow each other inside the file (and, file_size given, inside a file of
        exactly that size: an index is for one file)."""
        r, n = self._rows, len(self._rows)
        if len(self.delimiter) != 1:
            raise ValueError("line index: the delimiter is exactly one byte")
        if file_size is not None and int(file_size) != self.file_size:
            raise ValueError(f"line index: built for a file of {self.file_size} bytes, not {int(file_size)}")
        if not 0 <= self.cend <= self.file_size < 1 << 48 or not 0 <= self.delimiters <= self.usize < 1 << 62:
            raise ValueError("line index: totals out of range")
        c = np.append(r["coffset"], np.uint64(self.cend)).astype(np.int64)
        u = np.append(r["uoffset"], np.uint64(self.usize)).astype(np.int64)
        b = np.append(r["before"], np.uint64(self.delimiters)).astype(np.int64)
        if c[0] != (0 if n else self.cend) or u[0] != (0 if n else self.usize) or b[0] != (0 if n else self.delimiters):
            raise ValueError("line index: the first block does not start at 0")
        dc, du, db = np.diff(c), np.diff(u), np.diff(b)
        if n and (int(dc.min()) < 26 or int(dc.max()) > MAX_BLOCK):
            raise ValueError("line index: compressed offsets do not ascend by a block's size")
        if n and (int(du.min()) < 0 or int(du.max()) > MAX_BLOCK):
            raise ValueError("line index: uncompressed offsets do not ascend by a block's size")
        if n and (int(db.min()) < 0 or bool((db > du).any())):
            raise ValueError("line index: delimiter counts descend or exceed a block's bytes")
        flagged = (r["flags"] & 1).astype(bool)
        if n and (bool((r["flags"] > 1).any()) or bool(r["reserved"].any()) or bool((flagged & (db == 0)).any())):
            raise ValueError("line index: bad flags")

    def __len__(self):
        return len(self._rows)

    def __eq__(self, other):
        return (isinstance(other, LineIndex) and self.delimiter == other.delimiter and
                (self.file_size, self.cend, self.usize, self.delimiters) == (other.file_size, other.cend, other.usize, other.delimiters) and
                np.array_equal(self._rows, other._rows))

    __hash__ = None

    @property
    def blocks(self):
        """[(coffset, uoffset, delimiters in front, last byte is a delimiter), ...]"""
        r = self._rows
        return [(int(c), int(u), int(b), bool(f & 1)) for c, u, b, f in zip(r["coffset"], r["uoffset"], r["before"], r["flags"])]

    @classmethod
    def from_counts(cls, blocks, delimiter=b"\n", file_size=None):
        """From [(coffset, block bytes, isize, delimiters, last byte is a delimiter), ...] of blocks that follow each other from
        offset 0; a final empty block (the EOF block) gets no row.  file_size: the end of the last block unless given."""
        tab = np.asarray(blocks, np.int64).reshape(-1, 5)         # (an array of that shape is taken as it is)
        end = int(tab[-1, 0] + tab[-1, 1]) if len(tab) else 0
        if len(tab) and tab[-1, 2] == 0:
            tab = tab[:-1]
        rows = np.zeros(len(tab), LINE_ROW_DTYPE)
        if len(tab):
            rows["coffset"], rows["flags"] = tab[:, 0], tab[:, 4] != 0
            rows["uoffset"] = np.cumsum(tab[:, 2]) - tab[:, 2]
            rows["before"] = np.cumsum(tab[:, 3]) - tab[:, 3]
            cend, usize, total = int(tab[-1, 0] + tab[-1, 1]), int(tab[:, 2].sum()), int(tab[:, 3].sum())
        else:
            cend = usize = total = 0
        return cls(rows, delimiter, end if file_size is None else file_size, cend, usize, total)

    @classmethod
    def build(cls, file, delimiter=b"\n"):
        """Count `delimiter` (one byte) in every block of a BGZF file on the GPU: the file is read in windows as BgzfReader reads it,
        every window's blocks are decoded in one launch and counted where they lie, and 12 bytes per block come back.  BadGzipFile
        for a file that is not BGZF, or for a block that does not decode (with its offset)."""
        delimiter = bytes(delimiter)
        if len(delimiter) != 1:
            raise ValueError("the delimiter is exactly one byte")
        if _is_path(file):
            with _builtin_open(file, "rb") as f:
                return cls.build(f, delimiter)
        ctx = zlib_ng._ctx()
        file.seek(0)
        into = getattr(file, "readinto", None)
        buf = _lib.take_buffer(_READ_WINDOW + MAX_BLOCK)
        mv = memoryview(buf)
        parts, base, have, nblocks = [], 0, 0, 0
        try:
            while True:
                if into is not None:
                    got = into(mv[have:have + _READ_WINDOW]) or 0
                else:
                    chunk = file.read(_READ_WINDOW)
                    got = len(chunk)
                    mv[have:have + got] = chunk
                have += got
                if not have:
                    break
                data = mv[:have]
                code, tab, used, total = _lib.bgzf_scan(data)
                if not got and used < have and _cut_block(data[used:]):
                    raise BadGzipFile(f"BGZF block {nblocks + len(tab)} at offset {base + used}: the file ends inside the block")
                if code != _lib.OK and not (code == _lib.DATA_ERROR and not tab and got and have < MAX_BLOCK):
                    raise _scan_error(code if base + used == 0 else _lib.DATA_ERROR, nblocks + len(tab), base + used)
                if tab:
                    t = np.array(tab, np.int64)
                    members, bad = _member_table(np.frombuffer(data, np.uint8), t[:, 0], t[:, 2], t[:, 3])
                    if bad >= 0:
                        raise BadGzipFile(f"BGZF block {nblocks + bad} at offset {base + int(t[bad, 0])}: bad block header or block size")
                    status, rows = ctx.bgzf_count(data[:used], members, delimiter[0])
                    bad = np.nonzero(status)[0]
                    if len(bad):
                        raise _block_error(base + int(t[bad[0], 0]), status[bad[0]])
                    t[:, 0] += base
                    parts.append(np.column_stack([t[:, 0], t[:, 2], t[:, 3], rows[:, 0].astype(np.int64),
                                                  (rows[:, 1] & _lib.BGZF_COUNT_LAST).astype(np.int64)]))
                    nblocks += len(tab)
                tail = have - used
                if tail and used:
                    mv[:tail] = bytes(data[used:have])
                base, have = base + used, tail
                if not got:
                    break
        finally:
            del mv
            _lib.give_buffer(buf)
        return cls.from_counts(np.concatenate(parts) if parts else [], delimiter, base)

    # ---- on disk
    def to_bytes(self):
        return _LINE_HEAD.pack(LINE_INDEX_MAGIC, self.delimiter[0], 0, len(self._rows), self.file_size, self.cend, self.usize,
                               self.delimiters) + self._rows.tobytes()

    def save(self, path_or_file):
        if hasattr(path_or_file, "write"):
            path_or_file.write(self.to_bytes())
        else:
            with _builtin_open(path_or_file, "wb") as f:
                f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, blob, file_size=None):
        """ValueError for a truncated blob, another magic or version, rows that validate() refuses, or (file_size given) an index that
        was built for a file of another size."""
        blob = bytes(blob)
        if len(blob) < _LINE_HEAD.size:
            raise ValueError("line index: too short")
        magic, delim, zero, n, fsize, cend, usize, total = _LINE_HEAD.unpack_from(blob)
        if magic != LINE_INDEX_MAGIC:
            raise ValueError("line index: wrong magic or version")
        if delim > 255 or zero:
            raise ValueError("line index: bad header")
        if n > len(blob) or _LINE_HEAD.size + LINE_ROW_DTYPE.itemsize * n != len(blob):
            raise ValueError("line index: block count and length disagree")
        idx = cls(np.frombuffer(blob, LINE_ROW_DTYPE, n, _LINE_HEAD.size), bytes([delim]), fsize, cend, usize, total)
        if file_size is not None:
            idx.validate(file_size)
        return idx

    @classmethod
    def load(cls, path_or_file, file_size=None):
        if hasattr(path_or_file, "read"):
            return cls.from_bytes(path_or_file.read(), file_size)
        with _builtin_open(path_or_file, "rb") as f:
            return cls.from_bytes(f.read(), file_size)

    # ---- line numbers
    def _locate_many(self, lines, normalise=True):
        """-> (block numbers, ranks).  normalise: the position is where the line STARTS (behind a delimiter that ends a block: the
        next block that holds data, rank 0; the end of the data: block len(self), rank 0); else it is where the line in front of it
        ENDS (behind that delimiter, in its own block; the end of data that lacks a last delimiter: the last block, BGZF_RANK_END)."""
        L = np.asarray(lines, np.int64).reshape(-1)
        if len(L) and int(L.min()) < 0:
            raise ValueError("negative line number")
        if len(L) and int(L.max()) > self.lines:
            raise IndexError(f"line {int(L.max())} beyond the file's {self.lines} lines")
        n = len(self._rows)
        if not n:
            return np.zeros(len(L), np.int64), np.zeros(len(L), np.int64)
        inside = (L >= 1) & (L <= self.delimiters)
        b = np.clip(np.searchsorted(self._before, L, "left") - 1, 0, n - 1)        # the last block with fewer delimiters in front than L
        r = np.where(inside, L - self._before[b], 0)
        if normalise:
            step = inside & (r == self._count[b]) & self._last[b]
            b = np.where(step, self._next[np.minimum(b + 1, n)], b)
            r = np.where(step, 0, r)
            b = np.where(L == 0, self._next[0], b)
            b = np.where(L > self.delimiters, n, b)
        else:
            b = np.where(L == 0, self._next[0], b)
            over = L > self.delimiters
            b = np.where(over, max(self._tail, 0), b)
            r = np.where(over, _lib.BGZF_RANK_END, r)
        return b, r

    def locate(self, line):
        """-> (block number, rank): line `line` (from 0) starts behind the rank-th delimiter of that block's output, rank 0 being the
        block's first byte.  A line that starts behind a block's last byte starts in the next block that holds data.  line == lines
        is the end of the data: (len(self), 0) unless it lies inside a block.  IndexError beyond it."""
        b, r = self._locate_many([int(line)])
        return int(b[0]), int(r[0])

    def shards(self, reader, n, lines_per_record=1):
        """n + 1 virtual offsets (of `reader`, a BgzfReader on the file) that cut the file into n parts at record boundaries, a
        record being lines_per_record lines: adjacent parts differ by at most one record."""
        n, k = int(n), int(lines_per_record)
        if n < 1 or k < 1:
            raise ValueError("shards: n and lines_per_record are at least 1")
        records = (self.lines + k - 1) // k
        return reader.line_voffsets(self, [min(i * records // n * k, self.lines) for i in range(n + 1)])


# ---- lines by content
class GrepResult:
    """What grep() found: len() lines; numbers (int64, ascending), voffsets (uint64, the normalised virtual offset of each line's first
    byte: seek() goes there), offsets (int64, n + 1 of them) into data (the lines packed, each with its delimiter); result[i], slices
    and iteration yield bytes.  searched: the lines that were looked at."""

    def __init__(self, numbers, voffsets, offsets, data, searched):
        self.numbers = np.asarray(numbers, np.int64)
        self.voffsets = np.asarray(voffsets, np.uint64)
        self.offsets = np.asarray(offsets, np.int64)
        self.data = data
        self.searched = int(searched)
        if len(self.offsets) != len(self.numbers) + 1 or len(self.voffsets) != len(self.numbers):
            raise ValueError("GrepResult: arrays of different lengths")

    def __len__(self):
        return len(self.numbers)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        n = len(self)
        k = int(i)
        if not -n <= k < n:
            raise IndexError("GrepResult index out of range")
        k %= n
        return bytes(self.data[int(self.offsets[k]):int(self.offsets[k + 1])])

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def __repr__(self):
        return f"<GrepResult: {len(self)} of {self.searched} lines, {int(self.offsets[-1])} bytes>"


def _grep_patterns(patterns, delimiter):
    """-> (list of bytes, delimiter as bytes); ValueError as grep() documents it"""
    delimiter = bytes(delimiter)
    if len(delimiter) != 1:
        raise ValueError("the delimiter is exactly one byte")
    if isinstance(patterns, (bytes, bytearray, memoryview)):
        patterns = [patterns]
    pats = [bytes(p) for p in patterns]
    if not 1 <= len(pats) <= _lib.BGZF_GREP_MAX_PATTERNS:
        raise ValueError(f"grep takes 1 to {_lib.BGZF_GREP_MAX_PATTERNS} patterns, not {len(pats)}")
    for p in pats:
        if not 1 <= len(p) <= _lib.BGZF_GREP_MAX_PATTERN:
            raise ValueError(f"a pattern has 1 to {_lib.BGZF_GREP_MAX_PATTERN} bytes, not {len(p)}")
        if delimiter in p:
            raise ValueError("a pattern cannot contain the delimiter")
    return pats, delimiter


def _grep_mismatches(mismatches, pats):
    """-> k as zngamd_bgzf_grep_approx takes it; ValueError as grep() documents it"""
    if isinstance(mismatches, bool) or not isinstance(mismatches, (int, np.integer)):
        raise ValueError("mismatches is an integer")
    k = int(mismatches)
    if not 0 <= k <= _lib.BGZF_GREP_MAX_MISMATCH:
        raise ValueError(f"mismatches lies between 0 and {_lib.BGZF_GREP_MAX_MISMATCH}, not {k}")
    if k >= min(len(p) for p in pats):
        raise ValueError(f"mismatches is less than the length of the shortest pattern ({min(len(p) for p in pats)}), not {k}")
    return k


def _grep_window(coffs, isizes, text_off, stop, ended, text_cap):
    """Which part of a window is searched.  coffs / isizes: file offset and ISIZE of the window's blocks, in file order; text_off: where
    the first line starts in the first block's output; stop: None or (coffset, uoffset), the line start in front of which the search
    ends; ended: the file holds nothing behind these blocks; text_cap: decoded bytes per engine call at most.
    -> (blocks to decode, text_end as an offset into their packed output, final: the bytes behind the last delimiter are a line)"""
    n = len(coffs)
    ends = np.cumsum(isizes, dtype=np.int64)
    if n and int(ends[-1]) > text_cap:                       # (at least one block; what is cut off comes with the next window)
        n, ended = max(1, int(np.searchsorted(ends, text_cap, "right"))), False
    text_end, final = (int(ends[n - 1]) if n else 0), ended
    if stop is not None and n:
        c, u = stop
        k = int(np.searchsorted(coffs[:n], c))
        if k < n:
            if int(coffs[k]) != c:
                raise ValueError(f"stop: no block starts at compressed offset {c}")
            if u > int(isizes[k]):
                raise ValueError(f"stop: virtual offset points {u} bytes into a block of {int(isizes[k])}")
            n, text_end, final = k + (1 if u else 0), int(ends[k]) - int(isizes[k]) + u, True
    if text_end < text_off:
        raise ValueError("stop lies in front of start")
    return n, text_end, final


def _grep_advance(isizes, n_use, text_off, text_end, tail_off, final, window, max_line):
    """Where the next window begins.  tail_off: where the engine says the open line starts (text_end: there is none).
    -> None when the search is over, else (index of the block the next window starts with -- n_use: the block behind this window --,
    text_off in that block's output, compressed bytes to read).  The blocks from the open line's first one on are decoded again with
    the next window; a window in which no line ended is read again twice as large.  ValueError (with the index of the block and the
    offset in it where the line starts) for a line that has not ended after max_line bytes."""
    if final:
        return None
    if tail_off >= text_end:
        return n_use, 0, window
    starts = np.cumsum(isizes[:n_use], dtype=np.int64) - isizes[:n_use]
    b = int(np.searchsorted(starts, tail_off, "right")) - 1
    off = tail_off - int(starts[b])
    if text_end - tail_off > max_line:
        raise _LongLine(b, off)
    if b == 0 and off == text_off:
        window *= 2
    return b, off, window


class _LongLine(ValueError):
    def __init__(self, block, offset):
        super().__init__(block, offset)
        self.block, self.offset = block, offset


def _read_full(fp, mv):
    """fill mv from fp's position; fewer bytes only at the end of the file"""
    into, got = getattr(fp, "readinto", None), 0
    while got < len(mv):
        if into is not None:
            n = into(mv[got:]) or 0
        else:
            chunk = fp.read(len(mv) - got)
            n = len(chunk)
            mv[got:got + n] = chunk
        if not n:
            break
        got += n
    return got


def _grep_record_args(record_lines, match_line, first_byte):
    """-> (k, match_line or -1, first_byte or -1) as zngamd_bgzf_grep_records takes them; ValueError as grep_records() documents it"""
    k = int(record_lines)
    if not 1 <= k <= _lib.BGZF_GREP_MAX_RECORD_LINES:
        raise ValueError(f"a record has 1 to {_lib.BGZF_GREP_MAX_RECORD_LINES} lines, not {k}")
    j = -1 if match_line is None else int(match_line)
    if match_line is not None and not 0 <= j < k:
        raise ValueError(f"match_line lies between 0 and {k - 1}, not {j}")
    if first_byte is None:
        b = -1
    elif isinstance(first_byte, (bytes, bytearray, memoryview)):
        if len(bytes(first_byte)) != 1:
            raise ValueError("first_byte is exactly one byte")
        b = bytes(first_byte)[0]
    else:
        b = int(first_byte)
        if not 0 <= b <= 255:
            raise ValueError("first_byte lies between 0 and 255")
    return k, j, b


def _grep_file(fp, ctx, patterns, delimiter, invert, line_start, count, max_count, start, stop, first_line, max_line, records=None, mismatches=0,
               classify=None, partition=None):
    """The window loop of grep() and, with records = (record_lines, match_line, first_byte, allow_short), of grep_records(): then the
    unit that is counted, numbered, carried over a window's end and bounded by max_line is the record.  classify (with records): a
    _ClassifySink -- every window's records are not selected but assigned to their nearest pattern (classify_records(), demux()), the
    sink takes what each window gives, and what its finish() returns is the result.  partition (with records, instead of patterns): a
    _PartitionSink -- every window's records are split by the labels it holds (partition_records()) -- or a _TrimSink -- they are cut
    (trim_records()) -- or a _QcSink -- they are counted (qc_records()) -- or a _KeySink -- they are keyed (key_records()) -- or a
    _ScreenSink -- their k-mers are looked up in a set (screen_records()) -- or a _KmerCountSink -- their k-mers are counted
    (KmerCounter.add_file()) -- or an _OverlapSink -- the mates of every pair are laid over each other (overlap_records())."""
    if partition is None:
        pats, delimiter = _grep_patterns(patterns, delimiter)
        mismatches = _grep_mismatches(mismatches, pats)
    else:
        delimiter = _partition_delimiter(delimiter)
    approx = {"mismatches": mismatches} if mismatches else {}      # (0: the engine is called with the arguments it always had)
    unit, bound = ("record", "max_record") if records is not None else ("line", "max_line")
    if records is not None:
        rec_k, rec_j, rec_b = _grep_record_args(*records[:3])
    max_line = int(max_line)
    if not 1 <= max_line <= 1 << 31:
        raise ValueError(f"{bound} lies between 1 and 2**31")
    if max_count is not None and int(max_count) < 0:
        raise ValueError("max_count is not negative")
    ctx = ctx or zlib_ng._ctx()                              # (the arguments are judged before a context is asked for)
    if partition is None:
        blob, table = _lib.grep_pattern_table(pats)
    flags = (_lib.BGZF_GREP_INVERT if invert else 0) | (_lib.BGZF_GREP_LINE_START if line_start else 0) | (_lib.BGZF_GREP_COUNT_ONLY if count else 0)
    c_next, text_off = split_virtual_offset(start) if start is not None else (0, 0)
    stop = split_virtual_offset(stop) if stop is not None else None
    text_cap = max(_GREP_TEXT, max_line + 2 * MAX_BLOCK)
    window, first, nblocks, line_base, searched, matched = _READ_WINDOW, True, 0, int(first_line), 0, 0
    numbers, voffsets, lengths, pieces = [], [], [], []
    buf = mv = None
    try:
        while (stop is None or stop > (c_next, text_off)) and (max_count is None or matched < max_count):
            if buf is None or len(buf) < window + MAX_BLOCK:
                if buf is not None:
                    del mv
                    _lib.give_buffer(buf)
                buf = _lib.take_buffer(window + MAX_BLOCK)
                mv = memoryview(buf)
            fp.seek(c_next)
            got = _read_full(fp, mv[:window + MAX_BLOCK])
            if not got:
                break
            data = mv[:got]
            ended = got < window + MAX_BLOCK
            code, tab, used, total = _lib.bgzf_scan(data)
            if ended and used < got and _cut_block(data[used:]):
                raise EOFError(f"BGZF block {nblocks + len(tab)} at offset {c_next + used}: the file ends inside the block")
            if code != _lib.OK or not tab:
                raise _scan_error(code if c_next + used == 0 else _lib.DATA_ERROR, nblocks + len(tab), c_next + used)
            t = np.array(tab, np.int64)
            coffs, csizes, isizes = t[:, 0], t[:, 2], t[:, 3]
            if first and text_off > int(isizes[0]):
                raise ValueError(f"virtual offset points {text_off} bytes into a block of {int(isizes[0])}")
            first = False
            n_use, text_end, final = _grep_window(coffs + c_next, isizes, text_off, stop, ended and used == got, text_cap)
            members, bad = _member_table(np.frombuffer(data, np.uint8), coffs[:n_use], csizes[:n_use], isizes[:n_use])
            if bad >= 0:
                raise BadGzipFile(f"BGZF block {nblocks + bad} at offset {c_next + int(coffs[bad])}: bad block header or block size")
            cend = int(coffs[n_use - 1] + csizes[n_use - 1]) if n_use else 0
            wflags = flags | (_lib.BGZF_GREP_FINAL if final else 0)
            if partition is not None:
                status, tot, packed = partition.call(ctx, data[:cend], members, text_off, text_end, delimiter[0], wflags, rec_k, rec_b, line_base)
            elif classify is not None:
                _, status, tot, cls_rows, rows, packed = ctx.bgzf_classify_records(data[:cend], members, text_off, text_end, blob, table, delimiter[0],
                                                                                   wflags | classify.flags, mismatches, rec_k, rec_j, rec_b, line_base)
            elif records is None:
                _, status, tot, rows, packed = ctx.bgzf_grep(data[:cend], members, text_off, text_end, blob, table, delimiter[0], wflags, line_base, **approx)
            else:
                _, status, tot, rows, packed = ctx.bgzf_grep_records(data[:cend], members, text_off, text_end, blob, table, delimiter[0], wflags,
                                                                     rec_k, rec_j, rec_b, line_base, **approx)
            bad = np.nonzero(status)[0]
            if len(bad):
                raise _block_error(c_next + int(coffs[bad[0]]), status[bad[0]])
            if not tot.covered:
                raise BadGzipFile(f"BGZF blocks at offset {c_next}: the decoded blocks do not cover the text")

            def voffsets_of(src):                            # scratch offsets -> normalised virtual offsets
                at = np.searchsorted(members["out_off"].astype(np.int64), src, "right") - 1
                return (coffs[at] + c_next).astype(np.uint64) << np.uint64(16) | (src - members["out_off"][at].astype(np.int64)).astype(np.uint64)

            if records is not None:
                if tot.bad and hasattr(partition, "fault"):          # (a sink with faults of its own: the sort key and the place sinks)
                    msg = partition.fault(tot, int(voffsets_of(np.array([tot.bad_src], np.int64))[0]))
                    if msg:
                        raise ValueError(msg)
                if tot.bad == 2 and partition is not None:
                    raise ValueError(f"record {tot.bad_record}: its label is neither a class nor DROP")
                if tot.bad == 3 and partition is not None:
                    v = int(voffsets_of(np.array([tot.bad_src], np.int64))[0])
                    raise ValueError(partition.length_fault(int(tot.bad_record), v))
                if tot.bad:
                    v = int(voffsets_of(np.array([tot.bad_src], np.int64))[0])
                    raise ValueError(f"record {tot.bad_record} at virtual offset {v} does not start with {bytes([rec_b])!r} (first_byte)")
                if tot.short_lines and not records[3]:
                    raise ValueError(f"record {line_base + tot.seen - 1}, the last one, has {tot.short_lines} of {rec_k} lines (allow_short)")
            searched, line_base, matched = searched + tot.seen, line_base + tot.seen, matched + tot.matched
            if partition is not None:
                partition.window(tot, packed)
            elif classify is not None:
                classify.window(tot, cls_rows, packed)
            elif len(rows):
                numbers.append(rows["number"].astype(np.int64))
                voffsets.append(voffsets_of(rows["src_off"].astype(np.int64)))
                lengths.append(rows["len"].astype(np.int64))
                pieces.append(packed)
            try:
                nxt = _grep_advance(isizes, n_use, text_off, text_end, int(tot.tail_off), final, window, max_line)
            except _LongLine as e:
                v = make_virtual_offset(c_next + int(coffs[e.block]), e.offset)
                raise ValueError(f"the {unit} at virtual offset {v} has not ended after {max_line} bytes ({bound})") from None
            if nxt is None:
                break
            b, text_off, window = nxt
            nblocks += b
            c_next += int(coffs[b]) if b < len(coffs) else used
    finally:
        if buf is not None:
            del mv
            _lib.give_buffer(buf)
    if partition is not None:
        return partition.finish(searched)
    if classify is not None:
        return classify.finish(searched)
    if count:
        return matched if max_count is None else min(matched, int(max_count))
    numbers = np.concatenate(numbers) if numbers else np.empty(0, np.int64)
    voffsets = np.concatenate(voffsets) if voffsets else np.empty(0, np.uint64)
    offsets = np.zeros(len(numbers) + 1, np.int64)
    if lengths:
        np.cumsum(np.concatenate(lengths), out=offsets[1:])
    data = pieces[0] if len(pieces) == 1 else b"".join(pieces)
    if max_count is not None and len(numbers) > max_count:
        n = int(max_count)
        numbers, voffsets, offsets = numbers[:n], voffsets[:n], offsets[:n + 1]
        data = data[:int(offsets[-1])]
    return GrepResult(numbers, voffsets, offsets, data, searched)


def grep(file, patterns, *, delimiter=b"\n", invert=False, line_start=False, count=False, max_count=None, start=None, stop=None,
         first_line=0, max_line=64 << 20, mismatches=0):
    """The lines of a BGZF file (a path or a seekable binary file) that contain one of `patterns`: fixed byte strings, one bytes-like
    object or 1 to 64 of them, 1 to 255 bytes each, none holding the delimiter byte (ValueError).  The file is read in windows; each
    window's blocks are decoded in one launch and searched where they lie on the GPU, and only the matching lines, their numbers and
    their places come back: a GrepResult.
      line_start   the pattern must stand at the line's first byte      invert      the lines without a match
      count        -> int, the number of matching lines; no line leaves the device
      max_count    at most the first N matching lines; no window behind the one that reaches N is read
      start, stop  virtual offsets of line starts (LineIndex.shards, BgzfReader.line_voffsets): the part of the file to search
      first_line   the number of the first line searched
      max_line     ValueError (naming the line's virtual offset) for a line that is still open after this many bytes of a window:
                   the bound on the memory a file without delimiters can claim (at most 2**31)
      mismatches   k: a pattern of L bytes also matches L consecutive bytes of a line's body (the line without its delimiter) that
                   differ from it in at most k places -- substitutions only, no insertions or deletions; one k for all patterns, 0 to 16
                   and less than the shortest pattern's length (ValueError).  Every pattern is compared at every byte: the cost grows
                   with the patterns' total length.  0, the default, is the exact search
    A line ends with `delimiter` (one byte) and is returned with it; a non-empty remainder behind the last one is the last line.
    BadGzipFile for a file that is not BGZF or a block that does not decode (with its offset; no partial result), EOFError for a
    file that ends inside a block."""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return grep(f, patterns, delimiter=delimiter, invert=invert, line_start=line_start, count=count, max_count=max_count,
                        start=start, stop=stop, first_line=first_line, max_line=max_line, mismatches=mismatches)
    return _grep_file(file, None, patterns, delimiter, invert, line_start, count, max_count, start, stop, first_line, max_line, None, mismatches)


def grep_records(file, patterns, record_lines, *, match_line=None, first_byte=None, delimiter=b"\n", invert=False, line_start=False,
                 count=False, max_count=None, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False, mismatches=0):
    """grep() on records of `record_lines` (1 to 64) lines each -- FASTQ 4, two-line FASTA 2, interleaved pairs 8 -- in one pass: the
    records of which one line contains one of `patterns` come back WHOLE, as `grep -B1 -A2` or `seqkit grep -s -p` give them.  The
    file (or its part from `start`) begins with a record; record r is its lines [k r, k r + k).  -> a GrepResult whose numbers are
    record numbers, whose voffsets point at each record's first byte, whose data holds the records packed, and whose searched
    counts records.  patterns, delimiter, start, stop and the errors of the file are those of grep().
      match_line    only this line of a record (0 .. record_lines - 1) is looked at: 1 for the bases of a FASTQ read
      first_byte    every record starts with this byte (b"@"): ValueError naming the first record that does not and its virtual
                    offset -- what a stray blank line or a multi-line FASTQ, which shift every record behind them, turn into
      line_start    the pattern must stand at the first byte of the line       invert      the records without a match
      count         -> int, the number of selected records                      max_count   at most the first N selected records
      start, stop   virtual offsets of record starts: the cuts of LineIndex.shards(reader, n, lines_per_record=record_lines)
      first_record  the number of the first record searched
      max_record    ValueError (naming the record's virtual offset) for a record that is still open after this many bytes of a window
      allow_short   the lines left over at the end (fewer than record_lines) are a last record; without it they are a ValueError
                    that names the record and how many lines it has
      mismatches    as for grep(): a pattern matches a line of the record with up to this many bytes substituted"""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return grep_records(f, patterns, record_lines, match_line=match_line, first_byte=first_byte, delimiter=delimiter, invert=invert,
                                line_start=line_start, count=count, max_count=max_count, start=start, stop=stop, first_record=first_record,
                                max_record=max_record, allow_short=allow_short, mismatches=mismatches)
    return _grep_file(file, None, patterns, delimiter, invert, line_start, count, max_count, start, stop, first_record, max_record,
                      (record_lines, match_line, first_byte, allow_short), mismatches)


# ---- records by their nearest pattern
UNASSIGNED, AMBIGUOUS = -1, -2                # ClassifyResult.pattern for a record that no pattern is near / that two patterns are equally near


class ClassifyResult:
    """What classify_records() found, one entry per searched record in file order: pattern (int16: the index of the one nearest
    pattern, UNASSIGNED or AMBIGUOUS), distance (uint8: the mismatches of the nearest window, 255 for UNASSIGNED), tie (int16, (n, 2):
    the lowest and the highest index among the nearest patterns -- they differ where the record is AMBIGUOUS, both are the pattern where
    it is assigned and -1 where it is UNASSIGNED); counts (int64, n_patterns + 2: records per pattern, then the ambiguous, then the
    unassigned ones); searched = len(); first_record: the number of entry 0."""

    def __init__(self, pattern, distance, tie, counts, first_record=0):
        self.pattern = np.asarray(pattern, np.int16)
        self.distance = np.asarray(distance, np.uint8)
        self.tie = np.asarray(tie, np.int16).reshape(-1, 2)
        self.counts = np.asarray(counts, np.int64)
        self.searched = len(self.pattern)
        self.first_record = int(first_record)
        if len(self.distance) != self.searched or len(self.tie) != self.searched:
            raise ValueError("ClassifyResult: arrays of different lengths")

    def __len__(self):
        return self.searched

    def labels(self):
        """-> int32, one class per record in the numbering of counts: the pattern's index where assigned, n_patterns where AMBIGUOUS,
        n_patterns + 1 where UNASSIGNED -- what partition_records() takes for a file whose records go with these"""
        n = len(self.counts) - 2
        p = self.pattern.astype(np.int32)
        return np.where(p >= 0, p, np.where(p == AMBIGUOUS, np.int32(n), np.int32(n + 1))).astype(np.int32)

    def __repr__(self):
        return f"<ClassifyResult: {self.searched} records, {int(self.counts[:-2].sum())} assigned, {int(self.counts[-2])} ambiguous>"


class _ClassifySink:
    """what _grep_file hands a window's classes to: the class rows are kept (classify_records) or, with writers, every class's bytes go
    to its writer (demux; None: the class is dropped); keep with writers: both (demux_paired), and finish() gives the ClassifyResult"""

    def __init__(self, n_patterns, first_record, writers=None, keep=False):
        self.flags = _lib.BGZF_CLASSIFY_GROUP if writers is not None else 0
        self.writers, self.first_record, self.keep = writers, int(first_record), keep or writers is None
        self.counts = np.zeros(n_patterns + 2, np.int64)
        self.rows = []

    def window(self, tot, cls_rows, packed):
        n = len(self.counts)
        self.counts += np.frombuffer(tot.class_records, np.uint64, n).astype(np.int64)
        if self.keep and len(cls_rows):
            self.rows.append(cls_rows)
        if self.writers is None:
            return
        at = 0
        with memoryview(packed) as mv:
            for w, nbytes in zip(self.writers, np.frombuffer(tot.class_bytes, np.uint64, n).tolist()):
                if w is not None and nbytes:
                    w.write(mv[at:at + nbytes])
                at += nbytes
        if at != len(packed):
            raise RuntimeError("classify: the classes' bytes do not add up to the records")

    def finish(self, searched):
        if not self.keep:
            return self.counts
        rows = np.concatenate(self.rows) if self.rows else np.empty(0, _lib.CLASS_ROW_DTYPE)
        flags = rows["flags"]
        pattern = np.where(flags == _lib.BGZF_CLASS_ASSIGNED, rows["pattern"].astype(np.int16),
                           np.where(flags == _lib.BGZF_CLASS_AMBIGUOUS, np.int16(AMBIGUOUS), np.int16(UNASSIGNED))).astype(np.int16)
        tie = np.stack([rows["pattern"], rows["other"]], 1).astype(np.int16)
        tie[flags == 0] = -1
        return ClassifyResult(pattern, rows["distance"], tie, self.counts, self.first_record)


def _classify_patterns(patterns, delimiter):
    """the patterns of classify_records() and demux(): those of grep(), no two of them the same (ValueError)"""
    pats, delimiter = _grep_patterns(patterns, delimiter)
    if len(set(pats)) != len(pats):
        raise ValueError("two patterns are the same bytes: no record could be assigned to either (duplicate patterns)")
    return pats


def classify_records(file, patterns, record_lines, *, match_line=None, first_byte=None, delimiter=b"\n", line_start=False, start=None,
                     stop=None, first_record=0, max_record=64 << 20, allow_short=False, mismatches=0):
    """Every record's NEAREST pattern, in one pass over the file: what a demultiplexer asks of its barcodes.  Records, patterns,
    match_line, first_byte, line_start, start, stop, first_record, max_record, allow_short and the errors are those of grep_records();
    a window of a pattern's length counts by the rule of mismatches=k there (inside one line's body, at most k bytes substituted,
    0 <= k <= 16 and less than the shortest pattern's length; 0 is exact assignment).  For a record the distance to a pattern is the
    smallest over the windows of its lines that count; the record is
      assigned     to the one pattern at the smallest distance,
      AMBIGUOUS    when two or more patterns are at that distance (tie names the lowest and the highest of them),
      UNASSIGNED   when no pattern is within k.
    Two patterns with the same bytes are a ValueError; one that is a prefix of another is allowed.  -> a ClassifyResult; four bytes
    per record leave the device.  There is no invert and no count: counts holds every class's size."""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return classify_records(f, patterns, record_lines, match_line=match_line, first_byte=first_byte, delimiter=delimiter,
                                    line_start=line_start, start=start, stop=stop, first_record=first_record, max_record=max_record,
                                    allow_short=allow_short, mismatches=mismatches)
    return _classify_file(file, None, patterns, record_lines, match_line, first_byte, delimiter, line_start, start, stop, first_record,
                          max_record, allow_short, mismatches, None)


def _classify_file(fp, ctx, patterns, record_lines, match_line, first_byte, delimiter, line_start, start, stop, first_record, max_record,
                   allow_short, mismatches, writers, keep=False):
    pats = _classify_patterns(patterns, delimiter)
    sink = _ClassifySink(len(pats), first_record, writers, keep)
    return _grep_file(fp, ctx, pats, delimiter, False, line_start, False, None, start, stop, first_record, max_record,
                      (record_lines, match_line, first_byte, allow_short), mismatches, sink)


def _demux_file(fp, ctx, patterns, outputs, record_lines, ambiguous, unassigned, compresslevel, block_size, match_line, first_byte, delimiter,
                line_start, start, stop, first_record, max_record, allow_short, mismatches, keep=False):
    pats = _classify_patterns(patterns, delimiter)
    if _is_path(outputs) or hasattr(outputs, "write"):
        outputs = [outputs]
    outputs = list(outputs)
    if len(outputs) != len(pats):
        raise ValueError(f"demux takes one output per pattern: {len(pats)} patterns, {len(outputs)} outputs")
    _grep_mismatches(mismatches, pats)
    _grep_record_args(record_lines, match_line, first_byte)
    _check_block_size(block_size)
    return _with_writers("demux", outputs + [ambiguous, unassigned], compresslevel, block_size,
                         lambda writers: _classify_file(fp, ctx, pats, record_lines, match_line, first_byte, delimiter, line_start, start, stop,
                                                        first_record, max_record, allow_short, mismatches, writers, keep))


def _with_writers(who, outputs, compresslevel, block_size, run):
    """run(writers) with a BgzfWriter per output (None stays None).  If anything is raised the writers opened so far are closed and the
    error says that the outputs are incomplete; otherwise they are closed behind the run, whose result this returns."""
    writers = []
    try:
        for out in outputs:
            writers.append(None if out is None else BgzfWriter(out, "wb", compresslevel, block_size=block_size))
        result = run(writers)
    except Exception as e:
        for w in writers:
            if w is not None:
                try:
                    w.close()
                except Exception:
                    pass
        note = f"{who}: the outputs written so far were closed and are incomplete"
        e.args = ((f"{e.args[0]} ({note})",) + e.args[1:]) if e.args and isinstance(e.args[0], str) else e.args + (note,)
        raise
    for w in writers:
        if w is not None:
            w.close()
    return result


def demux(file, patterns, outputs, record_lines=4, *, ambiguous=None, unassigned=None, compresslevel=6, block_size=MAX_BLOCK_INPUT,
          match_line=None, first_byte=None, delimiter=b"\n", line_start=False, start=None, stop=None, first_record=0, max_record=64 << 20,
          allow_short=False, mismatches=0):
    """Split a BGZF file of records by their nearest pattern (the rule of classify_records(), whose keywords these are) in ONE pass:
    outputs is one path or writable binary file per pattern (a wrong count: ValueError); ambiguous and unassigned are a path, a file, or
    None to drop those records.  Every output is written through a BgzfWriter (compresslevel, block_size): a complete BGZF file with
    its EOF block whose decompressed bytes are exactly the records of its class, whole, in the order of the input.  -> counts (int64,
    n_patterns + 2: records per pattern, then the ambiguous, then the unassigned ones; dropped records are counted too).  If anything
    is raised the outputs written so far are closed, and the error says that they are incomplete."""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return demux(f, patterns, outputs, record_lines, ambiguous=ambiguous, unassigned=unassigned, compresslevel=compresslevel,
                         block_size=block_size, match_line=match_line, first_byte=first_byte, delimiter=delimiter, line_start=line_start,
                         start=start, stop=stop, first_record=first_record, max_record=max_record, allow_short=allow_short, mismatches=mismatches)
    return _demux_file(file, None, patterns, outputs, record_lines, ambiguous, unassigned, compresslevel, block_size, match_line, first_byte,
                       delimiter, line_start, start, stop, first_record, max_record, allow_short, mismatches)


# ---- records by a label per record: the mate file of a paired run, dual indexes, any rule of the caller's
DROP = -1                                     # a label of partition_records(): the record is counted and written nowhere
_OUT_OF_STEP = "the file holds {} records and labels has {} entries: the files are out of step"


def _partition_delimiter(delimiter):
    delimiter = bytes(delimiter)
    if len(delimiter) != 1:
        raise ValueError("the delimiter is exactly one byte")
    return delimiter


def _partition_labels(labels, outputs):
    """-> (labels as int64, outputs as a list or None, n_classes); ValueError as partition_records() documents it"""
    labels = np.asarray(labels)
    if labels.ndim != 1 or (labels.size and labels.dtype.kind not in "iu"):
        raise ValueError("labels is a one-dimensional array of integers")
    labels = labels.astype(np.int64)
    if outputs is not None:
        if _is_path(outputs) or hasattr(outputs, "write"):
            outputs = [outputs]
        outputs = list(outputs)
        n = len(outputs)
    else:
        n = max(1, int(labels.max()) + 1) if len(labels) else 1
    if not 1 <= n <= _lib.BGZF_PARTITION_MAX_CLASSES:
        raise ValueError(f"partition_records takes 1 to {_lib.BGZF_PARTITION_MAX_CLASSES} outputs (classes), not {n}")
    wrong = np.nonzero((labels < DROP) | (labels >= n))[0]
    if len(wrong):
        i = int(wrong[0])
        raise ValueError(f"labels[{i}] is {int(labels[i])}: a label is 0 .. {n - 1}, one per output, or DROP ({DROP})")
    return labels, outputs, n


class _PartitionSink:
    """what _grep_file hands a window's records to when they are split by labels: labels[i] (int64, judged) belongs to record
    first_record + i; writers: None (count only) or one per class, None where a class is written nowhere -- such a class is relabelled
    DROP before the upload, so its records are never gathered, and counted here"""

    def __init__(self, labels, n_classes, first_record, writers=None):
        self.n, self.first_record, self.writers = n_classes, int(first_record), writers
        self.flags = _lib.BGZF_CLASSIFY_GROUP if writers is not None and any(w is not None for w in writers) else 0
        self.quiet = [c for c in range(n_classes) if writers is not None and writers[c] is None]
        self.labels = labels
        dev = np.where(labels < 0, _lib.BGZF_PARTITION_DROP, labels)
        if self.quiet and self.flags:
            dev[np.isin(labels, self.quiet)] = _lib.BGZF_PARTITION_DROP
        else:
            self.quiet = []                                  # (nothing is gathered at all: every class is counted on the device)
        self.dev = dev.astype(np.uint16)
        self.counts, self.dropped, self.short = np.zeros(n_classes + 1, np.int64), 0, False

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        at = record_base - self.first_record
        lab, group = (self.dev[:0], 0) if self.short else (self.dev[at:], self.flags)      # (out of step: the records are only counted)
        _, status, tot, self.crec, self.cbytes, rows, packed = ctx.bgzf_partition_records(data, members, text_off, text_end, delim, flags | group, k,
                                                                                          first_byte, record_base, lab, self.n)
        return status, tot, packed

    def window(self, tot, packed):
        self.short = self.short or bool(tot.labels_short)
        if self.short:
            return
        self.counts[:self.n] += self.crec.astype(np.int64)
        self.dropped += int(tot.dropped)
        if not self.flags:
            return
        at = 0
        with memoryview(packed) as mv:
            for w, nbytes in zip(self.writers, self.cbytes.tolist()):
                if w is not None and nbytes:
                    w.write(mv[at:at + nbytes])
                at += nbytes
        if at != len(packed):
            raise RuntimeError("partition: the classes' bytes do not add up to the records")

    def finish(self, searched):
        if self.short or searched != len(self.labels):
            raise ValueError(_OUT_OF_STEP.format(searched, len(self.labels)))
        for c in self.quiet:
            self.counts[c] = int((self.labels == c).sum())
        self.counts[-1] = int((self.labels == DROP).sum())
        if self.dropped != int(self.counts[-1]) + sum(int(self.counts[c]) for c in self.quiet):
            raise RuntimeError("partition: the dropped records do not add up")
        return self.counts


def _partition_file(fp, ctx, labels, outputs, record_lines, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record,
                    allow_short):
    labels, outputs, n = _partition_labels(labels, outputs)
    _partition_delimiter(delimiter)
    _grep_record_args(record_lines, None, first_byte)
    _check_block_size(block_size)

    def run(writers):
        sink = _PartitionSink(labels, n, first_record, writers)
        return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                          (record_lines, None, first_byte, allow_short), 0, None, sink)

    if outputs is None:
        return run(None)
    return _with_writers("partition_records", outputs, compresslevel, block_size, run)


def partition_records(file, labels, outputs, record_lines=4, *, first_byte=None, delimiter=b"\n", compresslevel=6, block_size=MAX_BLOCK_INPUT,
                      start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
    """Split a BGZF file of records by a label per record that the caller computed: the mate file of a paired run by the classes of the
    file that holds the barcode (ClassifyResult.labels()), a read file by the pair of its index reads (pair_labels()), or by any rule
    at all -- quality, length, a hash for sharding.  labels[i] belongs to record first_record + i and is 0 .. len(outputs) - 1 or DROP;
    any other value is a ValueError before anything is opened.  outputs is one path or writable binary file per class (1 to 1024); an
    entry may be None: its records are counted and written nowhere, and like the DROP ones they are never gathered on the device.
    outputs=None only counts (the classes are 0 .. max(labels)).  Every output is written through a BgzfWriter (compresslevel,
    block_size): a complete BGZF file whose decompressed bytes are exactly the records of its class, whole, in the order of the input.
    record_lines, first_byte, delimiter, start, stop, first_record, max_record, allow_short and the errors of the file are those of
    grep_records().  -> counts (int64, len(outputs) + 1: records per class, then the DROP ones).
    A file that holds more or fewer records than labels is a ValueError that names both counts and says that the files are out of
    step: what protects a paired run from a mate file that lost a read.  If anything is raised the outputs written so far are closed,
    and the error says that they are incomplete."""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return partition_records(f, labels, outputs, record_lines, first_byte=first_byte, delimiter=delimiter, compresslevel=compresslevel,
                                     block_size=block_size, start=start, stop=stop, first_record=first_record, max_record=max_record,
                                     allow_short=allow_short)
    return _partition_file(file, None, labels, outputs, record_lines, first_byte, delimiter, compresslevel, block_size, start, stop, first_record,
                           max_record, allow_short)


# ---- records trimmed: the fixed cut, the low-quality ends, the 3' adapter, the reads that are too short
KEPT, TOO_SHORT, DROPPED = _lib.BGZF_TRIM_KEPT, _lib.BGZF_TRIM_TOO_SHORT, _lib.BGZF_TRIM_DROPPED      # a TrimResult's verdicts
_DROP_OUT_OF_STEP = "the file holds {} records and drop has {} entries: the files are out of step"


class TrimResult:
    """What trim_records() decided.  Per record, in the order of the file: begin and end (int64: the cut [begin, end) of the sequence
    body), adapter (int16: the adapter the read was cut at, -1 none), verdict (uint8: 0 kept, 1 too short, 2 dropped), steps (uint8: bit 0
    the fixed cut moved an end, bit 1 quality did, bit 2 an adapter did).  The counts: records, kept, too_short, dropped, bases_in (the
    sequence bytes read), bases_out (those of the kept records as written), quality_trimmed and adapter_trimmed (the bases each step took,
    over all records) and adapter_counts (int64, the records cut at every adapter)."""

    def __init__(self, rows, counts, adapter_counts):
        self.begin, self.end = rows["begin"].astype(np.int64), rows["end"].astype(np.int64)
        self.adapter = rows["adapter"].astype(np.int16)
        self.adapter[self.adapter == _lib.BGZF_TRIM_NO_ADAPTER] = -1
        self.verdict, self.steps = rows["verdict"].copy(), rows["steps"].copy()
        self.records = len(rows)
        for name, value in counts.items():
            setattr(self, name, int(value))
        self.adapter_counts = adapter_counts

    def __len__(self):
        return self.records

    def __repr__(self):
        return (f"<TrimResult: {self.records} records, {self.kept} kept, {self.too_short} too short, {self.dropped} dropped, "
                f"{self.bases_out} of {self.bases_in} bases>")


_TRIM_COUNTS = ("kept", "too_short", "dropped", "bases_in", "bases_out", "quality_trimmed", "adapter_trimmed")


def _trim_int(value, lo, hi, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{what} is an integer between {lo} and {hi}, not {value!r}")
    return int(value)


def _trim_pair(value, lo, hi, what):
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        value = (0, value)                                   # (one number: the 3' end, as cutadapt -q takes it)
    if not isinstance(value, (tuple, list)) or len(value) != 2:
        raise ValueError(f"{what} is a pair (5' end, 3' end)")
    return _trim_int(value[0], lo, hi, f"{what}[0]"), _trim_int(value[1], lo, hi, f"{what}[1]")


def _trim_conf(record_lines, seq_line, qual_line, cut, quality, quality_base, adapters, mismatches, min_overlap, min_length, first_byte, delimiter):
    """-> (BgzfTrimConf, adapters as a list of bytes, delimiter as bytes); ValueError as trim_records() documents it"""
    delimiter = _partition_delimiter(delimiter)
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    s = _trim_int(seq_line, 0, k - 1, "seq_line")
    q = -1 if qual_line is None else _trim_int(qual_line, 0, k - 1, "qual_line")
    if q == s:
        raise ValueError(f"seq_line and qual_line are two lines of the record, not both {s}")
    cut = _trim_pair(cut, 0, 0xFFFFFFFF, "cut")
    quality = _trim_pair(quality, 0, _lib.BGZF_TRIM_MAX_QUALITY, "quality")
    if q < 0 and any(quality):
        raise ValueError("quality needs a qual_line")
    base = _trim_int(quality_base, 0, 255, "quality_base")
    if isinstance(adapters, (bytes, bytearray, memoryview)):
        adapters = [adapters]
    pats = [bytes(a) for a in adapters]
    if pats:
        pats, _ = _grep_patterns(pats, delimiter)
        kmm = _grep_mismatches(mismatches, pats)
    else:
        kmm = _trim_int(mismatches, 0, _lib.BGZF_GREP_MAX_MISMATCH, "mismatches")
    cf = _lib.BgzfTrimConf(k, s, q, b, cut[0], cut[1], quality[0], quality[1], base, kmm, _trim_int(min_overlap, 1, _lib.BGZF_GREP_MAX_PATTERN, "min_overlap"),
                           _trim_int(min_length, 0, 0xFFFFFFFF, "min_length"), 0)
    return cf, pats, delimiter


def _trim_drop(drop):
    if drop is None:
        return None
    drop = np.asarray(drop)
    if drop.ndim != 1 or (drop.size and drop.dtype.kind not in "biu"):
        raise ValueError("drop is a one-dimensional array of booleans, one per record")
    return (drop != 0).astype(np.uint8)


class _TrimSink:
    """what _grep_file hands a window's records to when they are cut: drop[i] (uint8, or None) belongs to record first_record + i;
    writers: None (count only) or [kept, too short], None where a class is written nowhere"""

    def __init__(self, conf, pats, drop, first_record, writers=None):
        self.conf, self.pats, self.drop, self.first_record, self.writers = conf, pats, drop, int(first_record), writers
        self.blob, self.table = _lib.grep_pattern_table(pats) if pats else (b"", np.empty((0, 2), np.uint32))
        self.flags = _lib.BGZF_CLASSIFY_GROUP if writers is not None and any(w is not None for w in writers) else 0
        conf.flags = _lib.BGZF_TRIM_KEEP_SHORT if self.flags and writers[1] is not None else 0
        self.rows, self.short, self.args = [], False, None
        self.counts = dict.fromkeys(_TRIM_COUNTS, 0)
        self.adapter_counts = np.zeros(len(pats), np.int64)

    def _engine(self, ctx, conf, group, drop):
        data, members, text_off, text_end, delim, flags, record_base = self.args
        return ctx.bgzf_trim_records(data, members, text_off, text_end, self.blob if conf is self.conf else b"",
                                     self.table if conf is self.conf else self.table[:0], delim, flags | group, conf, record_base, drop)

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        self.ctx, self.args = ctx, (data, members, text_off, text_end, delim, flags, record_base)
        at = record_base - self.first_record
        drop, group = (None, self.flags) if self.drop is None else (self.drop[:0], 0) if self.short else (self.drop[at:], self.flags)
        _, status, tot, self.trim, self.grows, packed = self._engine(ctx, self.conf, group, drop)
        return status, tot, packed

    def length_fault(self, record, voffset):
        """the message for bad = 3: the engine is asked for the two bodies' lengths, each line taken as a sequence without qualities"""
        r, lens = record - self.args[6], []
        for line in (self.conf.seq_line, self.conf.qual_line):
            cf = _lib.BgzfTrimConf(self.conf.record_lines, line, -1, -1, 0, 0, 0, 0, 33, 0, 1, 0, 0)
            rows = self._engine(self.ctx, cf, 0, None)[3]
            lens.append(int(rows["end"][r]) if r < len(rows) else -1)
        return (f"record {record} at virtual offset {voffset}: line {self.conf.seq_line} (the sequence) has {lens[0]} bytes and line "
                f"{self.conf.qual_line} (the qualities) has {lens[1]}")

    def window(self, tot, packed):
        self.short = self.short or bool(tot.drop_short)
        if self.short:
            return
        self.rows.append(self.trim)
        for name in _TRIM_COUNTS:
            self.counts[name] += int(getattr(tot, name))
        self.adapter_counts += np.frombuffer(tot.adapter_records, np.uint64)[:len(self.pats)].astype(np.int64)
        if not self.flags:
            return
        nkept = int(self.grows["len"][:tot.kept].sum())
        with memoryview(packed) as mv:
            if self.writers[0] is not None and nkept:
                self.writers[0].write(mv[:nkept])
            if self.writers[1] is not None and len(packed) > nkept:
                self.writers[1].write(mv[nkept:])
        if len(packed) != int(tot.bytes):
            raise RuntimeError("trim: the classes' bytes do not add up to the records")

    def finish(self, searched):
        if self.drop is not None and (self.short or searched != len(self.drop)):
            raise ValueError(_DROP_OUT_OF_STEP.format(searched, len(self.drop)))
        rows = np.concatenate(self.rows) if self.rows else np.empty(0, _lib.TRIM_ROW_DTYPE)
        return TrimResult(rows, self.counts, self.adapter_counts)


def _trim_file(fp, ctx, output, too_short, record_lines, seq_line, qual_line, cut, quality, quality_base, adapters, mismatches, min_overlap, min_length,
               drop, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record, allow_short):
    conf, pats, delimiter = _trim_conf(record_lines, seq_line, qual_line, cut, quality, quality_base, adapters, mismatches, min_overlap, min_length,
                                       first_byte, delimiter)
    drop = _trim_drop(drop)
    _check_block_size(block_size)

    def run(writers):
        sink = _TrimSink(conf, pats, drop, first_record, writers)
        return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                          (record_lines, None, first_byte, allow_short), 0, None, sink)

    if output is None and too_short is None:
        return run(None)
    return _with_writers("trim_records", [output, too_short], compresslevel, block_size, run)


def trim_records(file, output, record_lines=4, *, seq_line=1, qual_line=3, cut=(0, 0), quality=(0, 0), quality_base=33, adapters=(), mismatches=0,
                 min_overlap=3, min_length=0, too_short=None, drop=None, first_byte=None, delimiter=b"\n", compresslevel=6,
                 block_size=MAX_BLOCK_INPUT, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
    """Cut the reads of a BGZF file of records as cutadapt, fastp or Trimmomatic cut them, on the GPU, and write what is left.  seq_line
    and qual_line (None: the records have no qualities) name the two lines of a record that are cut, at the same places; every other
    line is written whole.  For every read, in this order: cut = (front, back) takes that many bases off the two ends; quality = (5'
    cutoff, 3' cutoff) (each 0 .. 93, 0: off; one number: the 3' end) trims the low-quality ends by BWA's running-sum rule, the one of
    cutadapt -q, with qualities read as byte - quality_base; adapters (0 to 64 byte strings of 1 to 255 bytes) are 3' adapters: the read
    is cut where the first of them begins, an adapter counting as found when at least min_overlap of its bytes (or all of it) lie in the
    read and differ in at most mismatches * overlap // len(adapter) places -- so one that runs over the read's end is found too; bytes
    are compared as they are.  A read with fewer than min_length bases left is too short; drop (an array of booleans, drop[i] for record
    first_record + i) names records that are written nowhere whatever is left of them, which is how the mates of a paired run stay in
    step.  output is a path or writable binary file for the kept records, too_short an optional second one for the too-short records;
    each is written through a BgzfWriter (compresslevel, block_size): a complete BGZF file.  output=None writes nothing: the records are
    judged and counted only.  A read cut to nothing is written with empty lines.  record_lines, first_byte, delimiter, start, stop,
    first_record, max_record, allow_short and the errors of the file are those of grep_records().  -> TrimResult.
    A record whose sequence and qualities differ in length is a ValueError that names the record, its virtual offset and both lengths; a
    file that holds more or fewer records than drop is one that names both counts and says that the files are out of step.  If anything
    is raised the outputs written so far are closed, and the error says that they are incomplete."""
    if _is_path(file):
        _trim_conf(record_lines, seq_line, qual_line, cut, quality, quality_base, adapters, mismatches, min_overlap, min_length, first_byte, delimiter)
        _trim_drop(drop)                                         # (judged before the file is opened)
        _check_block_size(block_size)
        with _builtin_open(file, "rb") as f:
            return trim_records(f, output, record_lines, seq_line=seq_line, qual_line=qual_line, cut=cut, quality=quality, quality_base=quality_base,
                                adapters=adapters, mismatches=mismatches, min_overlap=min_overlap, min_length=min_length, too_short=too_short, drop=drop,
                                first_byte=first_byte, delimiter=delimiter, compresslevel=compresslevel, block_size=block_size, start=start, stop=stop,
                                first_record=first_record, max_record=max_record, allow_short=allow_short)
    return _trim_file(file, None, output, too_short, record_lines, seq_line, qual_line, cut, quality, quality_base, adapters, mismatches, min_overlap,
                      min_length, drop, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record, allow_short)


# ---- records counted: per-cycle base and quality tables, the distributions, the totals, a row per record
_QC_TOTALS = ("bytes_in", "bases", "empty", "quality_sum", "q20_bases", "q30_bases", "low_bases", "quality_clamped")
_QC_ROWS = (("length", "len"), ("gc", "gc"), ("n_bases", "n"), ("low_bases_per_record", "low"), ("quality_sum_per_record", "qsum"))


class QcResult:
    """What qc_records() counted.  The tables (numpy int64): base_pos[cycles + 1, 6] (the bases A, C, G, T, N and anything else at every
    position; the last row collects every position at or beyond cycles), qual_pos[cycles + 1, 94] (the qualities 0 .. 93 likewise; all
    zero without a qual_line), length_hist[cycles + 2] (reads of every length; the last entry collects the reads longer than cycles),
    gc_hist[101] (non-empty reads by 100 * GC // length) and meanq_hist[94] (non-empty reads by quality sum // length).  The totals
    (int): records, bytes_in, bases, min_len and max_len (0 without a record), empty, quality_sum, q20_bases, q30_bases, low_bases (below
    low_quality), quality_clamped (quality bytes outside quality_base .. quality_base + 93, counted as 0 or 93), and base_total (int64,
    6).  With per_record=True, one entry per record in the order of the file (otherwise None): length, gc, n_bases, low_bases_per_record
    (all int64) and quality_sum_per_record (int64).  Results of parts of a file add up: a + b."""

    def __init__(self, cycles, low_quality, tables, totals, base_total, rows):
        self.cycles, self.low_quality = int(cycles), int(low_quality)
        self._tables = tables
        self.base_pos, self.qual_pos, self.length_hist, self.gc_hist, self.meanq_hist = _lib.bgzf_qc_split(tables, self.cycles)
        for name, value in totals.items():
            setattr(self, name, int(value))
        self.base_total = base_total
        self.per_record = rows is not None
        for name, field in _QC_ROWS:
            setattr(self, name, rows[field].astype(np.int64) if rows is not None else None)

    def __len__(self):
        return self.records

    @property
    def mean_length(self):
        return self.bases / self.records if self.records else 0.0

    @property
    def q20_rate(self):
        return self.q20_bases / self.bases if self.bases else 0.0

    @property
    def q30_rate(self):
        return self.q30_bases / self.bases if self.bases else 0.0

    @property
    def gc_fraction(self):
        """the share of C and G among all bases"""
        return int(self.base_total[1] + self.base_total[2]) / self.bases if self.bases else 0.0

    def mean_quality_by_cycle(self):
        """float64[cycles + 1]: the mean quality at every row of qual_pos; nan where no base was counted"""
        n = self.qual_pos.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return (self.qual_pos * np.arange(_lib.BGZF_QC_QUALITIES)).sum(axis=1) / n

    def base_fraction_by_cycle(self):
        """float64[cycles + 1, 6]: the share of every base class at every row of base_pos; nan where no base was counted"""
        n = self.base_pos.sum(axis=1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.base_pos / n

    def __add__(self, other):
        if not isinstance(other, QcResult):
            return NotImplemented
        if (self.cycles, self.low_quality) != (other.cycles, other.low_quality):
            raise ValueError(f"results with cycles {self.cycles} and {other.cycles}, low_quality {self.low_quality} and {other.low_quality} do not add up")
        totals = {name: getattr(self, name) + getattr(other, name) for name in ("records",) + _QC_TOTALS}
        both = [r for r in (self, other) if r.records]
        totals["min_len"] = min((r.min_len for r in both), default=0)
        totals["max_len"] = max((r.max_len for r in both), default=0)
        rows = None
        if self.per_record and other.per_record:
            rows = np.empty(self.records + other.records, _lib.QC_ROW_DTYPE)
            for name, field in _QC_ROWS:
                rows[field] = np.concatenate([getattr(self, name), getattr(other, name)])
        return QcResult(self.cycles, self.low_quality, self._tables + other._tables, totals, self.base_total + other.base_total, rows)

    def merge(self, other):
        return self + other

    def __repr__(self):
        return (f"<QcResult: {self.records} records, {self.bases} bases, lengths {self.min_len} .. {self.max_len}, Q20 {100 * self.q20_rate:.1f} %, "
                f"Q30 {100 * self.q30_rate:.1f} %, GC {100 * self.gc_fraction:.1f} %>")


def _qc_conf(record_lines, seq_line, qual_line, quality_base, cycles, low_quality, per_record, first_byte, delimiter):
    """-> (BgzfQcConf, delimiter as bytes); ValueError as qc_records() documents it"""
    delimiter = _partition_delimiter(delimiter)
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    s = _trim_int(seq_line, 0, k - 1, "seq_line")
    q = -1 if qual_line is None else _trim_int(qual_line, 0, k - 1, "qual_line")
    if q == s:
        raise ValueError(f"seq_line and qual_line are two lines of the record, not both {s}")
    if not isinstance(per_record, (bool, np.bool_)):
        raise ValueError(f"per_record is True or False, not {per_record!r}")
    cf = _lib.BgzfQcConf(k, s, q, b, _trim_int(quality_base, 0, 255, "quality_base"), _trim_int(cycles, 1, _lib.BGZF_QC_MAX_CYCLES, "cycles"),
                         _trim_int(low_quality, 0, _lib.BGZF_QC_MAX_LOW, "low_quality"), _lib.BGZF_QC_ROWS if per_record else 0)
    return cf, delimiter


class _QcSink:
    """what _grep_file hands a window's records to when they are counted: the windows' tables and totals are added (the shortest and the
    longest read combined), their rows put one behind the other"""

    def __init__(self, conf):
        self.conf, self.args, self.rows = conf, None, []
        self.tables = np.zeros(_lib.bgzf_qc_table_words(conf.cycles), np.int64)
        self.totals = dict.fromkeys(_QC_TOTALS, 0)
        self.min_len = self.max_len = None
        self.base_total = np.zeros(_lib.BGZF_QC_BASES, np.int64)

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        self.ctx, self.args = ctx, (data, members, text_off, text_end, delim, flags, record_base)
        _, status, tot, self.win_tables, self.win_rows = ctx.bgzf_qc_records(data, members, text_off, text_end, delim, flags, self.conf, record_base)
        return status, tot, b""

    def length_fault(self, record, voffset):
        """the message for bad = 3: the engine is asked for the two bodies' lengths, each line taken as a sequence without qualities"""
        data, members, text_off, text_end, delim, flags, record_base = self.args
        r, lens = record - record_base, []
        for line in (self.conf.seq_line, self.conf.qual_line):
            cf = _lib.BgzfQcConf(self.conf.record_lines, line, -1, -1, 33, 1, 0, _lib.BGZF_QC_ROWS)
            rows = self.ctx.bgzf_qc_records(data, members, text_off, text_end, delim, flags, cf, record_base)[4]
            lens.append(int(rows["len"][r]) if r < len(rows) else -1)
        return (f"record {record} at virtual offset {voffset}: line {self.conf.seq_line} (the sequence) has {lens[0]} bytes and line "
                f"{self.conf.qual_line} (the qualities) has {lens[1]}")

    def window(self, tot, packed):
        self.tables += self.win_tables.view(np.int64)
        if not tot.seen:
            return
        for name in _QC_TOTALS:
            self.totals[name] += int(getattr(tot, name))
        self.base_total += np.frombuffer(tot.base_total, np.uint64).astype(np.int64)
        self.min_len = int(tot.min_len) if self.min_len is None else min(self.min_len, int(tot.min_len))
        self.max_len = int(tot.max_len) if self.max_len is None else max(self.max_len, int(tot.max_len))
        if self.conf.flags & _lib.BGZF_QC_ROWS:
            if len(self.win_rows) != tot.seen:
                raise RuntimeError("qc: the rows do not add up to the records")
            self.rows.append(self.win_rows)

    def finish(self, searched):
        rows = None
        if self.conf.flags & _lib.BGZF_QC_ROWS:
            rows = np.concatenate(self.rows) if self.rows else np.empty(0, _lib.QC_ROW_DTYPE)
        totals = dict(self.totals, records=searched, min_len=self.min_len or 0, max_len=self.max_len or 0)
        return QcResult(self.conf.cycles, self.conf.low_quality, self.tables, totals, self.base_total, rows)


def _qc_file(fp, ctx, record_lines, seq_line, qual_line, quality_base, cycles, low_quality, per_record, first_byte, delimiter, start, stop, first_record,
             max_record, allow_short):
    conf, delimiter = _qc_conf(record_lines, seq_line, qual_line, quality_base, cycles, low_quality, per_record, first_byte, delimiter)
    return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                      (record_lines, None, first_byte, allow_short), 0, None, _QcSink(conf))


def qc_records(file, record_lines=4, *, seq_line=1, qual_line=3, quality_base=33, cycles=512, low_quality=15, per_record=False, first_byte=None,
               delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
    """Quality control of a BGZF file of records on the GPU -- what FastQC, fastp's report and seqkit stats -a count; nothing but the
    counts leaves the device.  seq_line and qual_line (None: the records have no qualities) name the lines of a record that hold the
    bases and the qualities.  A base is A, C, G, T or N in either case, or something else; a quality is byte - quality_base, counted as
    0 below 0 and as 93 above 93 (quality_clamped says how often).  cycles (1 to 4096) is the number of positions the per-position tables
    have a row for; one further row collects everything at or beyond it, so a long read is counted whole.  low_quality (0 to 93): a base
    with a quality below it counts in low_bases.  per_record=True also returns every record's length, GC count, N count, low-quality
    bases and quality sum -- fastp's read filters are then a line of numpy whose result is the drop= of trim_records() or the labels of
    partition_records().  record_lines, first_byte, delimiter, start, stop, first_record, max_record, allow_short and the errors of the
    file are those of grep_records().  -> QcResult; the results of the parts of LineIndex.shards(reader, n, lines_per_record=k) add up
    to the whole file's.
    A record whose sequence and qualities differ in length is a ValueError that names the record, its virtual offset and both lengths."""
    if _is_path(file):
        _qc_conf(record_lines, seq_line, qual_line, quality_base, cycles, low_quality, per_record, first_byte, delimiter)      # (judged before the file is opened)
        with _builtin_open(file, "rb") as f:
            return qc_records(f, record_lines, seq_line=seq_line, qual_line=qual_line, quality_base=quality_base, cycles=cycles, low_quality=low_quality,
                              per_record=per_record, first_byte=first_byte, delimiter=delimiter, start=start, stop=stop, first_record=first_record,
                              max_record=max_record, allow_short=allow_short)
    return _qc_file(file, None, record_lines, seq_line, qual_line, quality_base, cycles, low_quality, per_record, first_byte, delimiter, start, stop,
                    first_record, max_record, allow_short)


# ---- duplicate records: a 16-byte key per record; the first record of every key and how many carry it
_KEY_OPTIONS = ("first", "length", "ignore_case", "canonical")
_M64 = (1 << 64) - 1
DEDUP_LEVELS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)      # FastQC's duplication levels: 1 .. 9, >10, >50, ..


class KeyResult:
    """What key_records() made: keys (numpy, structured: lo and hi, uint64, one per record in the order of the file), records, bases
    (the bytes of the sequence lines) and the options the keys were made with (first, length, ignore_case, canonical).  Keys made with
    the same options are comparable wherever they come from: a + b puts the keys of two shards, or of two files, one behind the other,
    and is a ValueError when the options differ."""

    def __init__(self, keys, bases, options):
        self.keys, self.records, self.bases = keys, len(keys), int(bases)
        self.options = dict(options)
        for name in _KEY_OPTIONS:
            setattr(self, name, self.options[name])

    def __len__(self):
        return self.records

    def __add__(self, other):
        if not isinstance(other, KeyResult):
            return NotImplemented
        if self.options != other.options:
            raise ValueError(f"keys made with {self.options} and with {other.options} are not comparable")
        return KeyResult(np.concatenate([self.keys, other.keys]), self.bases + other.bases, self.options)

    def __repr__(self):
        return f"<KeyResult: {self.records} records, {self.bases} bases>"


def _key_conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter):
    """-> (BgzfKeyConf, delimiter as bytes, the options of a KeyResult); ValueError as key_records() documents it"""
    delimiter = _partition_delimiter(delimiter)
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    s = _trim_int(seq_line, 0, k - 1, "seq_line")
    for name, value in (("ignore_case", ignore_case), ("canonical", canonical)):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{name} is True or False, not {value!r}")
    first, length = _trim_int(first, 0, (1 << 32) - 1, "first"), _trim_int(length, 0, (1 << 32) - 1, "length")
    flags = (_lib.BGZF_KEY_IGNORE_CASE if ignore_case else 0) | (_lib.BGZF_KEY_CANONICAL if canonical else 0)
    return (_lib.BgzfKeyConf(k, s, b, first, length, flags), delimiter,
            dict(first=first, length=length, ignore_case=bool(ignore_case), canonical=bool(canonical)))


class _KeySink:
    """what _grep_file hands a window's records to when they are keyed: the windows' rows are put one behind the other"""

    def __init__(self, conf, options):
        self.conf, self.options, self.rows, self.bases = conf, options, [], 0

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        _, status, tot, self.win_rows = ctx.bgzf_key_records(data, members, text_off, text_end, delim, flags, self.conf, record_base)
        return status, tot, b""

    def window(self, tot, packed):
        if not tot.seen:
            return
        if len(self.win_rows) != tot.seen:
            raise RuntimeError("key_records: the rows do not add up to the records")
        self.bases += int(tot.bases)
        self.rows.append(self.win_rows)

    def finish(self, searched):
        keys = np.concatenate(self.rows) if self.rows else np.empty(0, _lib.KEY_ROW_DTYPE)
        if len(keys) != searched:
            raise RuntimeError("key_records: the rows do not add up to the records")
        return KeyResult(keys, self.bases, self.options)


def _key_file(fp, ctx, record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter, start, stop, first_record, max_record,
              allow_short):
    conf, delimiter, options = _key_conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter)
    return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                      (record_lines, None, first_byte, allow_short), 0, None, _KeySink(conf, options))


def key_records(file, record_lines=4, *, seq_line=1, first=0, length=0, ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n",
                start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
    """The sequence of every record of a BGZF file reduced to a 16-byte key on the GPU: equal sequences get equal keys, in any window,
    shard or file.  The keyed part is body[first : first + length] of the line seq_line (length 0: to the end; a shorter body gives what
    it has).  ignore_case takes a .. z as A .. Z; canonical gives a read and its reverse complement (A<->T, C<->G, U->A, in either case)
    the same key.  The key function is fixed and documented: two 64-bit sums of splitmix64-mixed (position, byte)
    terms.  Equal keys are treated as equal sequences, as fastp treats its hashes: two different sequences meet in a key with a
    probability of about 2**-128 per pair.  record_lines, first_byte, delimiter, start, stop, first_record, max_record, allow_short and
    the errors of the file are those of grep_records().  -> KeyResult; the results of the parts of
    LineIndex.shards(reader, n, lines_per_record=k), put together with +, are the whole file's."""
    if _is_path(file):
        _key_conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter)      # (judged before the file is opened)
        with _builtin_open(file, "rb") as f:
            return key_records(f, record_lines, seq_line=seq_line, first=first, length=length, ignore_case=ignore_case, canonical=canonical,
                               first_byte=first_byte, delimiter=delimiter, start=start, stop=stop, first_record=first_record, max_record=max_record,
                               allow_short=allow_short)
    return _key_file(file, None, record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter, start, stop, first_record,
                     max_record, allow_short)


def _key_array(keys):
    """keys as one-dimensional KEY_ROW_DTYPE: a KeyResult, a structured array of lo and hi, or uint64 of shape (n, 2)"""
    if isinstance(keys, KeyResult):
        keys = keys.keys
    keys = np.asarray(keys)
    if keys.dtype == _lib.KEY_ROW_DTYPE and keys.ndim == 1:
        return np.ascontiguousarray(keys)
    if keys.dtype == np.uint64 and keys.ndim == 2 and keys.shape[1] == 2:
        return np.ascontiguousarray(keys).view(_lib.KEY_ROW_DTYPE).reshape(-1)
    raise ValueError("keys is a KeyResult, a one-dimensional array of (lo, hi) rows or a uint64 array of shape (n, 2)")


def _mix64(x):
    """the splitmix64 step on a uint64 array"""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def pair_keys(a, b):
    """Paired-end keys, on the host alone: the key of the pair (record i of a, record i of b), for dedup_keys().  Two pairs get the
    same key when both mates' keys are equal, as fastp dedups pairs; the order counts: (x, y) and (y, x) differ.  Word w of the pair's
    key is mix(mix(mix(mix(S_w ^ a.lo) ^ a.hi) ^ b.lo) ^ b.hi) with the mixer and seeds of key_records().  a and b are KeyResults (made
    with the same options) or key arrays of equal length; -> a KeyResult when both are, otherwise the key array."""
    results = isinstance(a, KeyResult) and isinstance(b, KeyResult)
    if results and a.options != b.options:
        raise ValueError(f"keys made with {a.options} and with {b.options} are not comparable")
    ka, kb = _key_array(a), _key_array(b)
    if len(ka) != len(kb):
        raise ValueError(f"pair_keys: the two files hold {len(ka)} and {len(kb)} records (unequal length): the files are out of step")
    out = np.empty(len(ka), _lib.KEY_ROW_DTYPE)
    for word, seed in (("lo", _lib.BGZF_KEY_SEED0), ("hi", _lib.BGZF_KEY_SEED1)):
        h = _mix64(np.uint64(seed) ^ ka["lo"])
        for x in (ka["hi"], kb["lo"], kb["hi"]):
            h = _mix64(h ^ x)
        out[word] = h
    return KeyResult(out, a.bases + b.bases, a.options) if results else out


class DedupResult:
    """What dedup_keys() found.  Per record, in the order of the keys: first (int64: the first record that carries the record's key;
    first[i] == i for a record that is kept), count (int64: at the first record of a key, how many records carry it; 0 elsewhere) and
    duplicate (bool: first[i] != i).  The totals: records, unique (the distinct keys), duplicates (records - unique),
    duplication_rate (duplicates / records), max_count (the largest group) and max_first (its first record)."""

    def __init__(self, first, count, unique, max_count, max_first):
        self.first, self.count = first, count
        self.records = len(first)
        self.duplicate = first != np.arange(self.records, dtype=np.int64)
        self.unique, self.max_count, self.max_first = int(unique), int(max_count), int(max_first)
        self.duplicates = self.records - self.unique

    def __len__(self):
        return self.records

    @property
    def duplication_rate(self):
        return self.duplicates / self.records if self.records else 0.0

    def most_common(self, k=10):
        """-> (first records, counts) of the k largest groups, the largest first, the earlier record first among equals"""
        heads = np.nonzero(self.count)[0]
        order = heads[np.argsort(-self.count[heads], kind="stable")][:max(0, int(k))]
        return order, self.count[order]

    def levels(self, edges=DEDUP_LEVELS):
        """FastQC's duplication-level table: bin i holds the sequences that occur edges[i] .. edges[i + 1] - 1 times, the last bin those
        that occur edges[-1] times or more.  -> (distinct, reads), int64, one entry per edge: the distinct sequences of every bin and
        the reads they stand for.  edges rise strictly from 1."""
        e = np.asarray(edges)
        if e.ndim != 1 or not len(e) or e.dtype.kind not in "iu" or e[0] != 1 or (np.diff(e) <= 0).any():
            raise ValueError("edges is a list of integers that rise strictly from 1")
        sizes = self.count[self.count > 0]
        at = np.searchsorted(e, sizes, "right") - 1
        distinct = np.bincount(at, minlength=len(e)).astype(np.int64)
        reads = np.bincount(at, weights=sizes, minlength=len(e)).astype(np.int64)
        return distinct, reads

    def drop(self):
        """uint8, one per record, 1 for a duplicate: the drop= of trim_records()"""
        return self.duplicate.astype(np.uint8)

    def labels(self, duplicate_class=1):
        """int64, one per record for partition_records(): 0 for a record that is kept, duplicate_class (which may be DROP) for a duplicate"""
        return np.where(self.duplicate, np.int64(duplicate_class), np.int64(0))

    def __repr__(self):
        return (f"<DedupResult: {self.records} records, {self.unique} unique, {self.duplicates} duplicates "
                f"({100 * self.duplication_rate:.1f} %), the most common one {self.max_count} times>")


def _dedup(ctx, keys):
    keys = _key_array(keys)
    if len(keys) > _lib.DEDUP_MAX_KEYS:
        raise ValueError(f"dedup_keys takes at most {_lib.DEDUP_MAX_KEYS} keys, not {len(keys)}")
    ctx = ctx or zlib_ng._ctx()                              # (the arguments are judged before a context is asked for)
    tot, first, count = ctx.dedup_keys(keys)
    if tot.n != len(keys):
        raise RuntimeError("dedup_keys: the engine counted other keys than it was given")
    return DedupResult(first.astype(np.int64), count.astype(np.int64), tot.unique, tot.max_count, tot.max_first)


def dedup_keys(keys):
    """Resolve keys on the GPU: for every key the first record that carries it and how many do.  keys is a KeyResult (of a file, or
    of several shards or files put together with +, or of pair_keys()), a structured array of (lo, hi) rows or uint64 of shape (n, 2);
    at most 2**30 of them.  Equal keys are treated as equal sequences.  -> DedupResult; it depends on the keys alone."""
    return _dedup(None, keys)


def _dedup_outputs(res, output, duplicates):
    """-> (labels, outputs) for partition_records: the first record of every key to output, the rest to duplicates or nowhere"""
    if duplicates is None:
        return res.labels(DROP), [output]
    return res.labels(1), [output, duplicates]


def _dedup_file(fp, ctx, output, duplicates, record_lines, compresslevel, block_size, seq_line, first, length, ignore_case, canonical, first_byte, delimiter,
                start, stop, first_record, max_record, allow_short):
    _key_conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter)
    _check_block_size(block_size)
    keys = _key_file(fp, ctx, record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter, start, stop, first_record, max_record,
                     allow_short)
    res = _dedup(ctx, keys)
    if output is None and duplicates is None:
        return res
    labels, outputs = _dedup_outputs(res, output, duplicates)
    _partition_file(fp, ctx, labels, outputs, record_lines, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record,
                    allow_short)
    return res


def dedup_records(file, output, record_lines=4, *, duplicates=None, compresslevel=6, block_size=MAX_BLOCK_INPUT, seq_line=1, first=0, length=0,
                  ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20,
                  allow_short=False):
    """Remove the duplicate records of a BGZF file -- fastp --dedup, seqkit rmdup -s, clumpify dedupe: records whose sequences are equal
    (by the key options of key_records(): seq_line, first, length, ignore_case, canonical).  Two passes over the file: key_records()
    and one dedup_keys(), then partition_records(): the first record of every sequence goes to output, whole and in the order of the
    file; the others go to duplicates (a path, a file, or None: they are written nowhere).  output=None (with duplicates=None) only
    counts and makes no second pass.  compresslevel and block_size are those of the outputs; the other keywords and the errors of the
    file are those of grep_records().  -> DedupResult.  Equal keys are treated as equal sequences (see key_records()).
    Not done here: keeping the copy of the best quality instead of the first, near-duplicates (reads that differ by a sequencing error),
    optical duplicates by their coordinates."""
    if _is_path(file):
        _key_conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter)      # (judged before the file is opened)
        _check_block_size(block_size)
        with _builtin_open(file, "rb") as f:
            return dedup_records(f, output, record_lines, duplicates=duplicates, compresslevel=compresslevel, block_size=block_size, seq_line=seq_line,
                                 first=first, length=length, ignore_case=ignore_case, canonical=canonical, first_byte=first_byte, delimiter=delimiter,
                                 start=start, stop=stop, first_record=first_record, max_record=max_record, allow_short=allow_short)
    return _dedup_file(file, None, output, duplicates, record_lines, compresslevel, block_size, seq_line, first, length, ignore_case, canonical, first_byte,
                       delimiter, start, stop, first_record, max_record, allow_short)


def dedup_paired(files, outputs, record_lines=4, *, duplicates=None, compresslevel=6, block_size=MAX_BLOCK_INPUT, seq_line=1, first=0, length=0,
                 ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20,
                 allow_short=False):
    """dedup_records() for the two files of a paired-end run: a pair is a duplicate when BOTH mates equal those of an earlier pair
    (pair_keys(): as fastp dedups pairs).  files are two paths or seekable binary files whose records go together; outputs one output
    per file (or None: count only); duplicates None or one entry per file; start and stop None or one virtual offset per file.  Every
    file is split by the same labels, so mates stay in step: record i of outputs[0] and record i of outputs[1] are a pair.  -> the
    DedupResult of the pairs.  Files that hold different numbers of records are a ValueError that says they are out of step."""
    files = list(files) if isinstance(files, (list, tuple)) else [files]
    nf = len(files)
    if nf != 2:
        raise ValueError(f"dedup_paired takes the two files of a paired run, not {nf}")
    _key_conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter)
    _check_block_size(block_size)
    if outputs is not None and (not isinstance(outputs, (list, tuple)) or len(outputs) != nf):
        raise ValueError(f"dedup_paired: outputs is None or one entry per file ({nf})")
    duplicates, start, stop = _per_file(duplicates, nf, "duplicates"), _per_file(start, nf, "start"), _per_file(stop, nf, "stop")
    with contextlib.ExitStack() as stack:
        fps = [stack.enter_context(_builtin_open(f, "rb")) if _is_path(f) else f for f in files]
        keys = [_key_file(fps[f], None, record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter, start[f], stop[f],
                          first_record, max_record, allow_short) for f in range(nf)]
        res = _dedup(None, pair_keys(keys[0], keys[1]))
        if outputs is not None:
            for f in range(nf):
                labels, outs = _dedup_outputs(res, outputs[f], duplicates[f])
                _partition_file(fps[f], None, labels, outs, record_lines, first_byte, delimiter, compresslevel, block_size, start[f], stop[f],
                                first_record, max_record, allow_short)
    return res


# ---- reads screened against reference k-mers: a k-mer set, the screen of a file, the screen and a split
def _kmer_rule(k, canonical):
    k = _trim_int(k, 1, _lib.KMER_MAX_K, "k")
    if not isinstance(canonical, (bool, np.bool_)):
        raise ValueError(f"canonical is True or False, not {canonical!r}")
    return k, bool(canonical)


def _kmer_names(names, n_refs):
    if not 1 <= n_refs <= _lib.KMER_MAX_REFS:
        raise ValueError(f"a k-mer set is made from 1 to {_lib.KMER_MAX_REFS} references, not {n_refs}")
    if names is None:
        return tuple(f"ref{j}" for j in range(n_refs))
    names = tuple(n.decode() if isinstance(n, (bytes, bytearray)) else str(n) for n in names)
    if len(names) != n_refs:
        raise ValueError(f"names has {len(names)} entries for {n_refs} references")
    return names


class KmerSet:
    """The k-mers of up to 64 references, as host data: k, canonical, names (one per reference) and codes and masks, sorted uint64
    arrays of equal length -- every code that occurs in some reference, and the mask whose bit j says that reference j holds it.  The
    rule of the codes is fixed and documented: A, C, G, T in either case are 0 .. 3, U counts as T, the first base of
    a k-mer is the most significant, and with canonical the code is the smaller of the k-mer's and its reverse complement's.  The
    device table that screen_records() reads is made on first use, one per context, and freed with the object.  len(): the distinct
    codes.  a | b: the union of two sets of equal k, canonical and names."""

    def __init__(self, k, canonical, names, codes, masks):
        self.k, self.canonical, self.names = int(k), bool(canonical), tuple(names)
        self.codes, self.masks = codes, masks
        self._tables = weakref.WeakKeyDictionary()       # context -> its DeviceKmerSet
        self._id = None

    @property
    def n_refs(self):
        return len(self.names)

    def __len__(self):
        return len(self.codes)

    @property
    def identity(self):
        """what two results must share to be added: the rule, the names and a digest of the pairs"""
        if self._id is None:
            h = hashlib.sha1(self.codes.tobytes())
            h.update(self.masks.tobytes())
            self._id = (self.k, self.canonical, self.names, len(self.codes), h.hexdigest())
        return self._id

    def _flags(self):
        return _lib.KMER_CANONICAL if self.canonical else 0

    def _table(self, ctx):
        t = self._tables.get(ctx)
        if t is None or not t.h:
            t = self._tables[ctx] = ctx.kmer_set_load(self.k, self._flags(), self.n_refs, self.codes, self.masks)
        return t

    @classmethod
    def from_codes(cls, k, codes, masks, n_refs, canonical=True, names=None):
        """A set from (code, mask) pairs: a code that appears twice ORs its masks.  ValueError for a code that is not below 4**k, for a
        mask that is 0 or has a bit at or above n_refs."""
        k, canonical = _kmer_rule(k, canonical)
        names = _kmer_names(names, _trim_int(n_refs, 1, _lib.KMER_MAX_REFS, "n_refs"))
        codes, masks = np.asarray(codes), np.asarray(masks)
        if codes.ndim != 1 or masks.shape != codes.shape or (len(codes) and (codes.dtype.kind not in "iu" or masks.dtype.kind not in "iu")):
            raise ValueError("codes and masks are one-dimensional integer arrays of equal length")
        if len(codes) and (codes.min() < 0 or masks.min() < 0):
            raise ValueError("codes and masks are not negative")
        codes, masks = codes.astype(np.uint64), masks.astype(np.uint64)
        if len(codes) > _lib.KMER_MAX_POSITIONS:
            raise ValueError(f"a k-mer set holds at most {_lib.KMER_MAX_POSITIONS} pairs, not {len(codes)}")
        if len(codes) and int(codes.max()) >= 4 ** k:
            raise ValueError(f"a code of a {k}-mer lies below 4**{k}")
        if len(codes) and (not masks.all() or (len(names) < 64 and int(masks.max()) >> len(names))):
            raise ValueError(f"a mask is not 0 and has no bit at or above n_refs ({len(names)})")
        order = np.argsort(codes, kind="stable")
        codes, masks = codes[order], masks[order]
        if len(codes):
            heads = np.concatenate([[True], codes[1:] != codes[:-1]])
            at = np.nonzero(heads)[0]
            codes, masks = codes[at], np.bitwise_or.reduceat(masks, at)
        return cls(k, canonical, names, codes, masks)

    @classmethod
    def build(cls, references, k=31, canonical=True, names=None):
        """The set of `references` (1 to 64 bytes-likes, or strings), built on the GPU.  k-mers do not span references; a k-mer with a byte
        other than A, C, G, T, U in either case is in no set; a reference shorter than k adds nothing."""
        k, canonical = _kmer_rule(k, canonical)
        if isinstance(references, (bytes, bytearray, memoryview, str)):
            references = [references]
        refs = [r.encode() if isinstance(r, str) else bytes(r) for r in references]
        names = _kmer_names(names, len(refs))
        positions = sum(max(0, len(r) - k + 1) for r in refs)
        if positions > _lib.KMER_MAX_POSITIONS:
            raise ValueError(f"the references hold {positions} positions; a k-mer set takes at most {_lib.KMER_MAX_POSITIONS}")
        ctx = zlib_ng._ctx()                                     # (the arguments are judged before a context is asked for)
        table = ctx.kmer_set_build(refs, k, _lib.KMER_CANONICAL if canonical else 0)
        codes, masks = table.export()
        order = np.argsort(codes, kind="stable")
        kset = cls(k, canonical, names, codes[order], masks[order])
        kset._tables[ctx] = table
        return kset

    @classmethod
    def from_fasta(cls, path, k=31, canonical=True):
        """The set of the records of a bgzipped FASTA (at most 64): FaidxIndex.build() and fetch_seq() read it, the names are the
        records' names"""
        k, canonical = _kmer_rule(k, canonical)
        index = FaidxIndex.build(path)
        names = index.names
        _kmer_names(names, len(names))
        seqs = fetch_seq(path, index, [(n, 0, None) for n in names])
        return cls.build([seqs[i] for i in range(len(names))], k, canonical, names)

    def save(self, path):
        """the set as an .npz: k, canonical, names, codes, masks"""
        np.savez(path, k=np.int64(self.k), canonical=np.bool_(self.canonical), names=np.array(self.names, dtype=np.str_), codes=self.codes,
                 masks=self.masks)

    @classmethod
    def load(cls, path):
        """a set that save() wrote; it is judged as from_codes() judges its arguments"""
        with np.load(path, allow_pickle=False) as z:
            names = [str(n) for n in z["names"]]
            return cls.from_codes(int(z["k"]), z["codes"], z["masks"], len(names), bool(z["canonical"]), names)

    def __or__(self, other):
        if not isinstance(other, KmerSet):
            return NotImplemented
        if (self.k, self.canonical, self.names) != (other.k, other.canonical, other.names):
            raise ValueError("the union is of two k-mer sets of equal k, canonical and names")
        return KmerSet.from_codes(self.k, np.concatenate([self.codes, other.codes]), np.concatenate([self.masks, other.masks]), self.n_refs, self.canonical,
                                  self.names)

    def __eq__(self, other):
        return isinstance(other, KmerSet) and self.identity == other.identity

    __hash__ = None

    def __repr__(self):
        return f"<KmerSet: k = {self.k}{', canonical' if self.canonical else ''}, {self.n_refs} references, {len(self)} codes>"


class ScreenResult:
    """What screen_records() found.  Per record, in the order of the file (int64 unless said): kmers (the positions whose k-mer is
    valid), hits (those whose code is in the set), refs (uint64: the OR of the masks of the hit codes), best (the reference that the
    most hit positions count for, the lowest among equals; -1 when nothing hit), best_hits (its count) and matched (bool: hits >=
    min_hits).  The totals: records, bases (the bytes of the sequence lines), matched_records.  a + b puts the results of two shards,
    or of two files, one behind the other, and is a ValueError when they were not made with the same set and min_hits."""

    def __init__(self, kmers, hits, refs, best, best_hits, bases, min_hits, names, set_id=None):
        self.kmers, self.hits, self.refs, self.best, self.best_hits = kmers, hits, refs, best, best_hits
        self.records, self.bases, self.min_hits = len(hits), int(bases), int(min_hits)
        self.names, self.set_id = tuple(names), set_id
        self.matched = hits >= self.min_hits
        self.matched_records = int(self.matched.sum())

    def __len__(self):
        return self.records

    def by_reference(self):
        """int64, one per reference: the records whose best reference it is"""
        return np.bincount(self.best[self.best >= 0], minlength=len(self.names)).astype(np.int64)

    def drop(self):
        """uint8, one per record, 1 for a matched one: the drop= of trim_records()"""
        return self.matched.astype(np.uint8)

    def labels(self, matched_class=1, unmatched_class=0):
        """int64, one per record for partition_records(); either class may be DROP"""
        return np.where(self.matched, np.int64(matched_class), np.int64(unmatched_class))

    def __add__(self, other):
        if not isinstance(other, ScreenResult):
            return NotImplemented
        if (self.set_id, self.names, self.min_hits) != (other.set_id, other.names, other.min_hits):
            raise ValueError("screen results made with different k-mer sets or min_hits are not comparable")
        cat = lambda name: np.concatenate([getattr(self, name), getattr(other, name)])
        return ScreenResult(cat("kmers"), cat("hits"), cat("refs"), cat("best"), cat("best_hits"), self.bases + other.bases, self.min_hits, self.names,
                            self.set_id)

    def __repr__(self):
        return f"<ScreenResult: {self.records} records, {self.matched_records} matched (min_hits {self.min_hits})>"


def _screen_conf(kset, record_lines, seq_line, min_hits, first_byte, delimiter):
    """-> (BgzfScreenConf, delimiter as bytes); ValueError as screen_records() documents it"""
    if not isinstance(kset, KmerSet):
        raise ValueError(f"kset is a KmerSet, not {type(kset).__name__}")
    delimiter = _partition_delimiter(delimiter)
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    s = _trim_int(seq_line, 0, k - 1, "seq_line")
    return _lib.BgzfScreenConf(k, s, b, _trim_int(min_hits, 1, (1 << 32) - 1, "min_hits"), 0), delimiter


class _ScreenSink:
    """what _grep_file hands a window's records to when they are screened: the windows' rows are put one behind the other"""

    def __init__(self, conf, kset):
        self.conf, self.kset, self.rows, self.bases = conf, kset, [], 0

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        _, status, tot, self.win_rows = ctx.bgzf_screen_records(data, members, text_off, text_end, delim, flags, self.conf, self.kset._table(ctx),
                                                                record_base)
        return status, tot, b""

    def window(self, tot, packed):
        if not tot.seen:
            return
        if len(self.win_rows) != tot.seen:
            raise RuntimeError("screen_records: the rows do not add up to the records")
        self.bases += int(tot.bases)
        self.rows.append(self.win_rows)

    def finish(self, searched):
        rows = np.concatenate(self.rows) if self.rows else np.empty(0, _lib.SCREEN_ROW_DTYPE)
        if len(rows) != searched:
            raise RuntimeError("screen_records: the rows do not add up to the records")
        best = rows["best"].astype(np.int64)
        best[best == _lib.KMER_NONE] = -1
        return ScreenResult(rows["kmers"].astype(np.int64), rows["hits"].astype(np.int64), rows["refs"].copy(), best, rows["best_hits"].astype(np.int64),
                            self.bases, self.conf.min_hits, self.kset.names, self.kset.identity)


def _screen_file(fp, ctx, kset, record_lines, seq_line, min_hits, first_byte, delimiter, start, stop, first_record, max_record, allow_short):
    conf, delimiter = _screen_conf(kset, record_lines, seq_line, min_hits, first_byte, delimiter)
    return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                      (record_lines, None, first_byte, allow_short), 0, None, _ScreenSink(conf, kset))


def screen_records(file, kset, record_lines=4, *, seq_line=1, min_hits=1, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0,
                   max_record=64 << 20, allow_short=False):
    """Every k-mer of every read of a BGZF file looked up in a KmerSet on the GPU -- the contaminant screen of bbduk ref= k=,
    fastq_screen and rRNA depletion.  The sequence of a record is the line seq_line; a k-mer with a byte other than A, C, G, T, U in
    either case counts for nothing; a read is matched when at least min_hits of its k-mers are in the set.  record_lines, first_byte,
    delimiter, start, stop, first_record, max_record, allow_short and the errors of the file are those of grep_records().
    -> ScreenResult; the results of the parts of LineIndex.shards(reader, n, lines_per_record=k), put together with +, are the whole
    file's."""
    if _is_path(file):
        _screen_conf(kset, record_lines, seq_line, min_hits, first_byte, delimiter)      # (judged before the file is opened)
        with _builtin_open(file, "rb") as f:
            return screen_records(f, kset, record_lines, seq_line=seq_line, min_hits=min_hits, first_byte=first_byte, delimiter=delimiter, start=start,
                                  stop=stop, first_record=first_record, max_record=max_record, allow_short=allow_short)
    return _screen_file(file, None, kset, record_lines, seq_line, min_hits, first_byte, delimiter, start, stop, first_record, max_record, allow_short)


def _screen_filter_file(fp, ctx, kset, output, matched, record_lines, compresslevel, block_size, seq_line, min_hits, first_byte, delimiter, start, stop,
                        first_record, max_record, allow_short):
    _screen_conf(kset, record_lines, seq_line, min_hits, first_byte, delimiter)
    _check_block_size(block_size)
    res = _screen_file(fp, ctx, kset, record_lines, seq_line, min_hits, first_byte, delimiter, start, stop, first_record, max_record, allow_short)
    outputs, classes = [], []
    for out in (output, matched):                            # unmatched, matched: a class each, or DROP
        classes.append(len(outputs) if out is not None else DROP)
        if out is not None:
            outputs.append(out)
    if outputs:
        _partition_file(fp, ctx, res.labels(classes[1], classes[0]), outputs, record_lines, first_byte, delimiter, compresslevel, block_size, start, stop,
                        first_record, max_record, allow_short)
    return res


def screen_filter(file, kset, output, matched=None, record_lines=4, *, seq_line=1, min_hits=1, compresslevel=6, block_size=MAX_BLOCK_INPUT,
                  first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
    """screen_records(), then partition_records() -- bbduk's out= and outm=: the reads that are not matched go to output, whole and in
    the order of the file; the matched ones go to matched (a path, a file, or None: they are written nowhere).  output may be None
    too: then only the matched reads are written, or, with both None, nothing is and no second pass is made.  compresslevel and
    block_size are those of the outputs; the other keywords and the errors of the file are those of screen_records().
    -> ScreenResult.  For a paired run screen both files and split both by a.matched | b.matched."""
    if _is_path(file):
        _screen_conf(kset, record_lines, seq_line, min_hits, first_byte, delimiter)      # (judged before the file is opened)
        _check_block_size(block_size)
        with _builtin_open(file, "rb") as f:
            return screen_filter(f, kset, output, matched, record_lines, seq_line=seq_line, min_hits=min_hits, compresslevel=compresslevel,
                                 block_size=block_size, first_byte=first_byte, delimiter=delimiter, start=start, stop=stop, first_record=first_record,
                                 max_record=max_record, allow_short=allow_short)
    return _screen_filter_file(file, None, kset, output, matched, record_lines, compresslevel, block_size, seq_line, min_hits, first_byte, delimiter, start,
                               stop, first_record, max_record, allow_short)


# ---- the k-mers of the reads counted: a counter on the device, its pairs and its spectrum as host data
_KMER_BASES = b"ACGT"


def _kmer_encode(kmer, k, canonical):
    """the code of one k-mer (bytes or str) by the rule of the screen: ValueError for another length or a byte that is no base"""
    b = kmer.encode() if isinstance(kmer, str) else bytes(kmer)
    if len(b) != k:
        raise ValueError(f"{kmer!r} is not a {k}-mer")
    f = r = 0
    for i, ch in enumerate(b):
        v = b"ACGTU".find(bytes([ch]).upper())
        if v < 0:
            raise ValueError(f"{kmer!r} holds a byte that is no base")
        v = min(v, 3)
        f = f << 2 | v
        r |= (3 - v) << (2 * i)
    return min(f, r) if canonical else f


def _kmer_decode(codes, k):
    """the k-mers of `codes` as a list of bytes, the first base from the most significant bits"""
    codes = np.asarray(codes, np.uint64)
    out = np.empty((len(codes), k), np.uint8)
    lut = np.frombuffer(_KMER_BASES, np.uint8)
    for i in range(k):
        out[:, i] = lut[((codes >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.intp)]
    return [row.tobytes() for row in out]


def _kmer_spectrum(counts, bins):
    """uint64 of `bins` entries: [c] the codes with count c, [bins - 1] those with at least that"""
    return np.bincount(np.minimum(counts, np.uint64(bins - 1)).astype(np.int64), minlength=bins).astype(np.uint64)


def _count_filter(min_count, max_count, bins):
    if min_count is not None:
        min_count = _trim_int(min_count, 1, (1 << 64) - 1, "min_count")
    if max_count is not None:
        max_count = _trim_int(max_count, min_count or 1, (1 << 64) - 1, "max_count")
    return min_count, max_count, _trim_int(bins, 2, _lib.KMER_HIST_MAX_BINS, "bins")


class KmerCounts:
    """The k-mers of a library and how often each occurs, as host data: k, canonical; codes (sorted uint64) and counts (uint64) of equal
    length -- the pairs with min_count <= count <= max_count (None: no upper bound; min_count None: no pair was exported); spectrum
    (uint64, bins entries): [c] is the number of codes that occur c times, the last entry those that occur at least bins - 1 times --
    of ALL codes, whatever the filter; records, bases, kmers (the valid positions: the sum of all counts) and distinct (all codes).
    The rule of the codes is that of KmerSet.  len(): the pairs held.  a + b: the counts of two shards or files -- of equal k and
    canonical, both unfiltered and of equal bins (ValueError otherwise: filtered counts do not add)."""

    def __init__(self, k, canonical, codes, counts, spectrum, *, min_count=1, max_count=None, records=0, bases=0, kmers=None, distinct=None):
        k, canonical = _kmer_rule(k, canonical)
        codes, counts, spectrum = np.asarray(codes), np.asarray(counts), np.asarray(spectrum)
        if codes.ndim != 1 or counts.shape != codes.shape or spectrum.ndim != 1:
            raise ValueError("codes and counts are one-dimensional arrays of equal length, spectrum is one-dimensional")
        for a in (codes, counts, spectrum):
            if len(a) and (a.dtype.kind not in "iu" or a.min() < 0):
                raise ValueError("codes, counts and spectrum are integers that are not negative")
        codes, counts, spectrum = codes.astype(np.uint64), counts.astype(np.uint64), spectrum.astype(np.uint64)
        min_count, max_count, _ = _count_filter(min_count, max_count, len(spectrum))
        if len(codes) and int(codes.max()) >= 4 ** k:
            raise ValueError(f"a code of a {k}-mer lies below 4**{k}")
        if len(codes) > 1 and not (codes[1:] > codes[:-1]).all():
            raise ValueError("codes ascend and none appears twice")
        if min_count is None and len(codes):
            raise ValueError("min_count None goes with no pair")
        if len(codes) and (int(counts.min()) < min_count or (max_count is not None and int(counts.max()) > max_count)):
            raise ValueError("a count lies outside min_count .. max_count")
        if int(spectrum[0]):
            raise ValueError("spectrum[0] is 0: no code occurs 0 times")
        self.k, self.canonical, self.codes, self.counts, self.spectrum = k, canonical, codes, counts, spectrum
        self.min_count, self.max_count = min_count, max_count
        self.records, self.bases = int(records), int(bases)
        self.distinct = int(spectrum.sum()) if distinct is None else int(distinct)
        self.kmers = (int(counts.sum()) if self.unfiltered else 0) if kmers is None else int(kmers)
        if self.distinct != int(spectrum.sum()) or (self.unfiltered and (self.distinct != len(codes) or self.kmers != int(counts.sum()))):
            raise ValueError("distinct, kmers, the spectrum and the pairs do not agree")

    @property
    def unfiltered(self):
        return self.min_count == 1 and self.max_count is None

    @property
    def bins(self):
        return len(self.spectrum)

    def __len__(self):
        return len(self.codes)

    def count_of(self, kmers_or_codes):
        """the counts (uint64; 0 for one that is not held) of k-mers -- bytes or str, one or a list -- or of codes (integers)"""
        one = isinstance(kmers_or_codes, (bytes, bytearray, str, int, np.integer))
        items = [kmers_or_codes] if one else list(kmers_or_codes)
        want = np.array([_kmer_encode(x, self.k, self.canonical) if isinstance(x, (bytes, bytearray, str)) else int(x) for x in items], np.uint64)
        at = np.searchsorted(self.codes, want)
        out = np.zeros(len(want), np.uint64)
        inside = at < len(self.codes)
        hit = np.zeros(len(want), bool)
        hit[inside] = self.codes[at[inside]] == want[inside]
        out[hit] = self.counts[at[hit]]
        return int(out[0]) if one else out

    def kmer_bytes(self):
        """the codes decoded, a list of bytes in the order of codes (`kmers` itself is the number of valid positions)"""
        return _kmer_decode(self.codes, self.k)

    def most_common(self, n=None):
        """[(k-mer as bytes, count)], the largest counts first, equal counts by ascending code"""
        order = np.lexsort((self.codes, np.iinfo(np.uint64).max - self.counts))
        if n is not None:
            order = order[:max(int(n), 0)]
        return list(zip(_kmer_decode(self.codes[order], self.k), (int(c) for c in self.counts[order])))

    def to_kmerset(self, min_count=1, max_count=None, name="counted"):
        """the codes with min_count <= count <= max_count as a KmerSet of one reference: the solid k-mers of this run as the set of the
        next screen"""
        min_count, max_count, _ = _count_filter(min_count, max_count, 2)
        if min_count is None:
            raise ValueError("min_count is an integer")
        take = self.counts >= np.uint64(min_count)
        if max_count is not None:
            take &= self.counts <= np.uint64(max_count)
        codes = self.codes[take]
        return KmerSet.from_codes(self.k, codes, np.ones(len(codes), np.uint64), 1, self.canonical, [name])

    def __add__(self, other):
        if not isinstance(other, KmerCounts):
            return NotImplemented
        if (self.k, self.canonical) != (other.k, other.canonical):
            raise ValueError("k-mer counts of different k or canonical do not add")
        if not (self.unfiltered and other.unfiltered) or self.bins != other.bins:
            raise ValueError("only unfiltered k-mer counts of equal bins add: a filtered count has lost the codes that the sum needs")
        codes, counts = np.concatenate([self.codes, other.codes]), np.concatenate([self.counts, other.counts])
        order = np.argsort(codes, kind="stable")
        codes, counts = codes[order], counts[order]
        if len(codes):
            at = np.nonzero(np.concatenate([[True], codes[1:] != codes[:-1]]))[0]
            codes, counts = codes[at], np.add.reduceat(counts, at)
        return KmerCounts(self.k, self.canonical, codes, counts, _kmer_spectrum(counts, self.bins), records=self.records + other.records,
                          bases=self.bases + other.bases, kmers=self.kmers + other.kmers, distinct=len(codes))

    def save(self, path):
        """the counts as an .npz"""
        np.savez(path, k=np.int64(self.k), canonical=np.bool_(self.canonical), codes=self.codes, counts=self.counts, spectrum=self.spectrum,
                 filter=np.array([self.min_count or 0, self.max_count or 0], np.uint64),      # (0: None)
                 totals=np.array([self.records, self.bases, self.kmers, self.distinct], np.uint64))

    @classmethod
    def load(cls, path):
        """counts that save() wrote; they are judged as the constructor judges its arguments"""
        with np.load(path, allow_pickle=False) as z:
            lo, hi = (int(v) for v in z["filter"])
            records, bases, kmers, distinct = (int(v) for v in z["totals"])
            return cls(int(z["k"]), bool(z["canonical"]), z["codes"], z["counts"], z["spectrum"], min_count=lo or None, max_count=hi or None,
                       records=records, bases=bases, kmers=kmers, distinct=distinct)

    def __eq__(self, other):
        return (isinstance(other, KmerCounts) and (self.k, self.canonical, self.min_count, self.max_count, self.records, self.bases, self.kmers, self.distinct) ==
                (other.k, other.canonical, other.min_count, other.max_count, other.records, other.bases, other.kmers, other.distinct) and
                np.array_equal(self.codes, other.codes) and np.array_equal(self.counts, other.counts) and np.array_equal(self.spectrum, other.spectrum))

    __hash__ = None

    def __repr__(self):
        return (f"<KmerCounts: k = {self.k}{', canonical' if self.canonical else ''}, {self.distinct} codes of {self.kmers} k-mers in {self.records} records, "
                f"{len(self)} pairs (count >= {self.min_count}{'' if self.max_count is None else f', <= {self.max_count}'})>")


def _count_conf(record_lines, seq_line, first_byte, delimiter):
    """-> (BgzfCountConf, delimiter as bytes); ValueError as KmerCounter.add_file() documents it"""
    delimiter = _partition_delimiter(delimiter)
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    return _lib.BgzfCountConf(k, _trim_int(seq_line, 0, k - 1, "seq_line"), b, 0), delimiter


class _KmerCountSink:
    """what _grep_file hands a window's records to when their k-mers are counted: before every window the counter's table is given
    room for the window's text, then the window is added"""

    def __init__(self, conf, owner):
        self.conf, self.owner, self.bases, self.kmers, self.started = conf, owner, 0, 0, False

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        table = self.owner._reserve(ctx, text_end - text_off)
        self.started = True
        r, status, tot = ctx.bgzf_count_kmers(data, members, text_off, text_end, delim, flags, self.conf, table, record_base)
        if r != _lib.OK:
            raise RuntimeError("count_kmers: the table had no room for a window it was reserved for")
        return status, tot, b""

    def window(self, tot, packed):
        self.bases += int(tot.bases)
        self.kmers += int(tot.kmers)

    def finish(self, searched):
        return searched, self.bases, self.kmers


class KmerCounter:
    """Counts the k-mers of the reads of any number of BGZF files -- or of shards of them -- on the GPU: jellyfish count and histo, KMC,
    the k-mer spectrum.  The table lives on the device and grows as the files are read; the text never comes to the host.
      k, canonical       the rule of KmerSet: 1 <= k <= 31; with canonical a k-mer and its reverse complement are one code
      max_table_bytes    MemoryError, naming the bytes needed, before the table would grow beyond this (None: what the device gives)
    add_file() adds a file, add_counts() a KmerCounts, result() gives the KmerCounts of everything added so far, close() frees the
    table.  After an error of a file (a bad block, a first_byte violation, ...) the counter holds an unknown part of a window and
    refuses further use (ValueError)."""

    def __init__(self, k=31, canonical=True, *, max_table_bytes=None, _room=0):
        self.k, self.canonical = _kmer_rule(k, canonical)
        self.max_table_bytes = None if max_table_bytes is None else _trim_int(max_table_bytes, 0, 1 << 62, "max_table_bytes")
        self._room = _trim_int(_room, 0, _lib.KMER_COUNTER_MAX_CAP // 2, "_room")
        self._ctx = self._table = None
        self.records = self.bases = 0
        self._closed = self._broken = False

    def _live(self):
        if self._closed:
            raise ValueError("the counter is closed")
        if self._broken:
            raise ValueError("the counter holds an unknown part of a file after an error and cannot be used")

    def _device(self, ctx):
        """the DeviceKmerCounter, made on first use in the context of that use"""
        if self._table is None:
            self._ctx = ctx or zlib_ng._ctx()
            self._table = self._ctx.kmer_counter_new(self.k, _lib.KMER_CANONICAL if self.canonical else 0, self._room)
        elif ctx is not None and ctx is not self._ctx:
            raise ValueError("a KmerCounter stays in the context of its first use")
        return self._table

    def _reserve(self, ctx, room):
        """room for `room` more codes, by the rule of the C call; MemoryError, with nothing launched, when that cannot be had"""
        table = self._device(ctx)
        info = table.info
        need = info.distinct + int(room)
        if need <= info.cap // 2:
            return table
        cap = 64
        while cap < 4 * need:
            cap <<= 1
        nbytes = cap * 16
        if cap > _lib.KMER_COUNTER_MAX_CAP or (self.max_table_bytes is not None and nbytes > self.max_table_bytes):
            raise MemoryError(f"the k-mer table needs {nbytes} bytes for {info.distinct} codes and {int(room)} more (max_table_bytes)")
        if table.reserve(int(room)) != _lib.OK:
            raise MemoryError(f"the device cannot give the {nbytes} bytes that the k-mer table needs")
        return table

    def add_file(self, file, record_lines=4, *, seq_line=1, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20,
                 allow_short=False, _ctx=None):
        """Adds the k-mers of the reads of a BGZF file (a path or a seekable binary file).  The sequence of a record is the line
        seq_line; a k-mer with a byte other than A, C, G, T, U in either case counts for nothing.  record_lines, first_byte, delimiter,
        start, stop, first_record, max_record, allow_short and the errors of the file are those of grep_records().  -> self"""
        self._live()
        conf, delimiter = _count_conf(record_lines, seq_line, first_byte, delimiter)      # (judged before the file is opened)
        if _is_path(file):
            with _builtin_open(file, "rb") as f:
                return self.add_file(f, record_lines, seq_line=seq_line, first_byte=first_byte, delimiter=delimiter, start=start, stop=stop,
                                     first_record=first_record, max_record=max_record, allow_short=allow_short, _ctx=_ctx)
        sink = _KmerCountSink(conf, self)
        try:
            records, bases, _ = _grep_file(file, _ctx or self._ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                                           (record_lines, None, first_byte, allow_short), 0, None, sink)
        except BaseException:
            self._broken = sink.started                      # (a part of the file is in the counts; before the first window nothing is)
            raise
        self.records, self.bases = self.records + records, self.bases + bases
        return self

    def add_counts(self, counts):
        """Adds a KmerCounts of the same k and canonical that holds all its pairs (unfiltered).  -> self"""
        self._live()
        if not isinstance(counts, KmerCounts) or (counts.k, counts.canonical) != (self.k, self.canonical) or not counts.unfiltered:
            raise ValueError("add_counts takes unfiltered KmerCounts of the counter's k and canonical")
        table = self._reserve(None, len(counts))
        if table.add(counts.codes, counts.counts) != _lib.OK:
            raise RuntimeError("add_counts: the table had no room for the pairs it was reserved for")
        self.records, self.bases = self.records + counts.records, self.bases + counts.bases
        return self

    def result(self, min_count=1, max_count=None, bins=10001):
        """-> KmerCounts: the pairs with min_count <= count <= max_count (max_count None: no upper bound; min_count None: no pair, the
        spectrum only) and the spectrum of ALL codes in `bins` entries (2 to 16384)."""
        self._live()
        min_count, max_count, bins = _count_filter(min_count, max_count, bins)
        table = self._device(None)
        info = table.info
        if info.poisoned:
            raise ValueError("the counter holds an unknown part of a file after an error and cannot be used")
        spectrum = table.histogram(bins)
        codes = counts = np.empty(0, np.uint64)
        if min_count is not None:
            _, codes, counts, _ = table.export(min_count, max_count or 0)
            order = np.argsort(codes, kind="stable")
            codes, counts = codes[order], counts[order]
        return KmerCounts(self.k, self.canonical, codes, counts, spectrum, min_count=min_count, max_count=max_count, records=self.records,
                          bases=self.bases, kmers=info.total, distinct=info.distinct)

    def close(self):
        if self._table is not None:
            self._table.free()
        self._table, self._closed = None, True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def count_kmers(file_or_files, k=31, *, canonical=True, min_count=1, max_count=None, bins=10001, record_lines=4, seq_line=1, first_byte=None,
                delimiter=b"\n", max_record=64 << 20, allow_short=False, max_table_bytes=None):
    """The k-mers of the reads of one BGZF file, or of a list of them (R1 and R2, the lanes of a run), counted on the GPU in one call:
    a KmerCounter, add_file() for each, result(), close().  -> KmerCounts.  k, canonical and max_table_bytes are KmerCounter's,
    min_count, max_count and bins are result()'s, the other keywords are add_file()'s."""
    _count_filter(min_count, max_count, bins)                # (judged before a file is looked at)
    _count_conf(record_lines, seq_line, first_byte, delimiter)
    files = list(file_or_files) if isinstance(file_or_files, (list, tuple)) else [file_or_files]
    with KmerCounter(k, canonical, max_table_bytes=max_table_bytes) as counter:
        for f in files:
            counter.add_file(f, record_lines, seq_line=seq_line, first_byte=first_byte, delimiter=delimiter, max_record=max_record, allow_short=allow_short)
        return counter.result(min_count, max_count, bins)


# ---- records in another order: a key per record, a stable sort of keys, records written in any order
_SORT_KINDS = {"bytes": _lib.BGZF_SORT_BYTES, "number": _lib.BGZF_SORT_NUMBER, "length": _lib.BGZF_SORT_LENGTH}
_SORT_LINE_PRESETS = {"bed": (1, 2, b"#"), "gff": (1, 4, b"#"), "vcf": (1, 2, b"#"), "sam": (3, 4, b"@")}      # name column, start column (from 1), meta
_SORT_OUT_OF_STEP = "the file holds {} records and lengths has {} entries: the files are out of step"


class SortKey:
    """One part of a sort key: the field it reads and the bytes it becomes.  line: the line of the record; column: None for the whole
    line, otherwise the 0-based field when the line is cut at sep (one byte).  kind "bytes": field[first : first + width] padded with
    0x00 (width 8 .. 128, a multiple of 8; ignore_case takes a .. z as A .. Z; a longer field is a ValueError of the call unless it
    truncates), "number": an unsigned decimal number (8 bytes), "length": the length of the field (4 bytes).  reverse turns the part's
    order round.  truncate: None follows the call's truncate=."""

    def __init__(self, line=0, column=None, sep=b"\t", kind="bytes", width=32, first=0, reverse=False, ignore_case=False, truncate=None):
        if kind not in _SORT_KINDS:
            raise ValueError(f"kind is 'bytes', 'number' or 'length', not {kind!r}")
        for name, value in (("reverse", reverse), ("ignore_case", ignore_case)):
            if not isinstance(value, (bool, np.bool_)):
                raise ValueError(f"{name} is True or False, not {value!r}")
        if truncate is not None and not isinstance(truncate, (bool, np.bool_)):
            raise ValueError(f"truncate is None, True or False, not {truncate!r}")
        sep = bytes(sep)
        if len(sep) != 1:
            raise ValueError("sep is exactly one byte")
        self.line = _trim_int(line, 0, _lib.BGZF_GREP_MAX_RECORD_LINES - 1, "line")
        self.column = None if column is None else _trim_int(column, 0, (1 << 31) - 1, "column")
        self.sep, self.kind, self.reverse, self.ignore_case, self.truncate = sep, kind, bool(reverse), bool(ignore_case), truncate
        if kind == "bytes":
            self.width, self.first = _trim_int(width, 8, 128, "width"), _trim_int(first, 0, (1 << 32) - 1, "first")
            if self.width % 8:
                raise ValueError(f"width is a multiple of 8, not {self.width}")
        else:
            self.width, self.first = 0, 0
            if ignore_case or truncate:
                raise ValueError("ignore_case and truncate belong to kind 'bytes'")

    @property
    def nbytes(self):
        return self.width if self.kind == "bytes" else 8 if self.kind == "number" else 4

    def _spec(self, truncate):
        t = self.kind == "bytes" and bool(truncate if self.truncate is None else self.truncate)
        return (self.line, -1 if self.column is None else self.column, self.sep, self.kind, self.width, self.first, self.reverse, self.ignore_case, t)

    def __repr__(self):
        return (f"SortKey(line={self.line}, column={self.column}, sep={self.sep!r}, kind={self.kind!r}, width={self.width}, first={self.first}, "
                f"reverse={self.reverse}, ignore_case={self.ignore_case}, truncate={self.truncate})")


def _sort_preset(name, record_lines, meta):
    """-> (parts, record_lines, meta) of a preset name; ValueError for any other"""
    if name == "name":
        return [SortKey(0, 0, b" ", width=64)], record_lines, meta
    if name == "sequence":
        return [SortKey(1, width=128, truncate=True), SortKey(1, width=128, first=128, truncate=True)], record_lines, meta
    if name == "length":
        return [SortKey(1, kind="length")], record_lines, meta
    if name in _SORT_LINE_PRESETS:
        seq, beg, m = _SORT_LINE_PRESETS[name]
        return [SortKey(0, seq - 1), SortKey(0, beg - 1, kind="number")], 1, m if meta is None else meta
    raise ValueError(f"unknown preset {name!r}: name, sequence, length, bed, gff, vcf or sam")


def _sort_conf(key, record_lines, meta, truncate, reverse, first_byte, delimiter):
    """-> (BgzfSortConf, delimiter as bytes, record_lines, the specification of a SortKeyResult); ValueError as sort_key_records()
    documents it"""
    delimiter = _partition_delimiter(delimiter)
    for name, value in (("truncate", truncate), ("reverse", reverse)):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{name} is True or False, not {value!r}")
    if isinstance(key, str):
        parts, record_lines, meta = _sort_preset(key, record_lines, meta)
    elif isinstance(key, SortKey):
        parts = [key]
    else:
        parts = list(key)
        if not all(isinstance(p, SortKey) for p in parts):
            raise ValueError("key is a SortKey, a list of up to four, or the name of a preset")
    if len(parts) > _lib.BGZF_SORT_MAX_PARTS:
        raise ValueError(f"a key has at most {_lib.BGZF_SORT_MAX_PARTS} parts, not {len(parts)}")
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    _, _, m = _grep_record_args(1, None, meta)
    width = sum(p.nbytes for p in parts)
    if width > _lib.SORT_MAX_WIDTH:
        raise ValueError(f"the key's parts add up to {width} bytes: at most {_lib.SORT_MAX_WIDTH}")
    conf = _lib.BgzfSortConf(k, b, m, len(parts))
    spec = []
    for i, p in enumerate(parts):
        if p.line >= k:
            raise ValueError(f"line lies between 0 and {k - 1}, not {p.line}")
        s = p._spec(truncate)
        rev = s[6] != bool(reverse)
        flags = (_lib.BGZF_SORT_REVERSE if rev else 0) | (_lib.BGZF_SORT_IGNORE_CASE if s[7] else 0) | (_lib.BGZF_SORT_TRUNCATE if s[8] else 0)
        conf.part[i] = _lib.BgzfSortPart(s[0], s[1], s[4], s[5], flags, _SORT_KINDS[s[3]], s[2][0])
        spec.append(s[:6] + (rev,) + s[7:])
    return conf, delimiter, k, dict(record_lines=k, meta=None if m < 0 else m, width=(width + 7) // 8 * 8, parts=tuple(spec))


class SortKeyResult:
    """What sort_key_records() made: keys (uint8 of shape (records, W): row r is the key of record r, and memcmp order of the rows is the
    order asked for), lengths (uint32: the bytes of every record as permute_records() writes it), records, and spec, the key
    specification the rows were made with.  a + b puts the rows of two shards, or of two files, one behind the other, and is a
    ValueError when the specifications differ."""

    def __init__(self, keys, lengths, spec):
        self.keys, self.lengths, self.records, self.spec = keys, lengths, len(lengths), dict(spec)
        if keys.ndim != 2 or keys.dtype != np.uint8 or len(keys) != self.records or keys.shape[1] != self.spec["width"]:
            raise ValueError("keys is uint8 of shape (records, W) with the specification's W")

    @property
    def key_width(self):
        return self.spec["width"]

    def __len__(self):
        return self.records

    def __add__(self, other):
        if not isinstance(other, SortKeyResult):
            return NotImplemented
        if self.spec != other.spec:
            raise ValueError(f"keys made with {self.spec} and with {other.spec} are not comparable")
        return SortKeyResult(np.concatenate([self.keys, other.keys]), np.concatenate([self.lengths, other.lengths]), self.spec)

    def __repr__(self):
        return f"<SortKeyResult: {self.records} records, keys of {self.key_width} bytes>"


class _SortKeySink:
    """what _grep_file hands a window's records to when their sort keys are made: the windows' rows and lengths are put one behind the
    other"""

    def __init__(self, conf, spec):
        self.conf, self.spec, self.rows, self.lens = conf, spec, [], []

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        _, status, tot, self.win_rows, self.win_lens = ctx.bgzf_sort_key_records(data, members, text_off, text_end, delim, flags, self.conf, record_base)
        return status, tot, b""

    def fault(self, tot, voffset):
        if tot.bad == 2:
            return f"record {tot.bad_record} at virtual offset {voffset}: a number field is empty, holds a byte that is no digit, or is above 2**64 - 1"
        if tot.bad == 3:
            return (f"record {tot.bad_record} at virtual offset {voffset}: a field is longer than its part's first + width; the longest such field of "
                    f"the window has {tot.max_field} bytes: a width of {(int(tot.max_field) + 7) // 8 * 8} behind first would do, or truncate=True")
        return None

    def window(self, tot, packed):
        if not tot.seen:
            return
        if len(self.win_rows) != tot.seen or len(self.win_lens) != tot.seen:
            raise RuntimeError("sort_key_records: the rows do not add up to the records")
        self.rows.append(self.win_rows)
        self.lens.append(self.win_lens)

    def finish(self, searched):
        w = self.spec["width"]
        keys = np.concatenate(self.rows) if self.rows else np.empty((0, w), np.uint8)
        lens = np.concatenate(self.lens) if self.lens else np.empty(0, np.uint32)
        if len(lens) != searched:
            raise RuntimeError("sort_key_records: the rows do not add up to the records")
        return SortKeyResult(keys, lens, self.spec)


def _sort_key_file(fp, ctx, key, record_lines, meta, truncate, reverse, first_byte, delimiter, start, stop, first_record, max_record, allow_short):
    conf, delimiter, k, spec = _sort_conf(key, record_lines, meta, truncate, reverse, first_byte, delimiter)
    return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record, (k, None, first_byte, allow_short), 0,
                      None, _SortKeySink(conf, spec))


def sort_key_records(file, key, record_lines=4, *, meta=None, truncate=False, first_byte=None, delimiter=b"\n", start=None, stop=None,
                     first_record=0, max_record=64 << 20, allow_short=False):
    """A sort key per record of a BGZF file, made on the GPU: rows of W bytes whose memcmp order is the order asked for.  key is a
    SortKey, a list of up to four (the first counts most), or a preset: "name" (line 0 up to the first blank, 64 bytes), "sequence"
    (line 1, its first 256 bytes), "length" (the length of line 1), or "bed", "gff", "vcf", "sam" -- line formats: record_lines is 1
    whatever is passed, the key is the name column (32 bytes) and then the start column as a number, and the lines that begin with
    meta (b"#", for sam b"@") get the all-zero key, so that a stable sort leaves them in front and in order.  The parts' bytes add up
    to at most 256; W is their sum rounded up to 8.  truncate=True cuts a "bytes" field that is longer than its width instead of
    raising.  record_lines, first_byte, delimiter, start, stop, first_record, max_record, allow_short and the errors of the file are those
    of grep_records().  A number field that is empty, holds another byte than a digit or exceeds 2**64 - 1, and a field that is too
    long, are ValueErrors that name the record and its virtual offset.  -> SortKeyResult; the results of the parts of
    LineIndex.shards(reader, n, lines_per_record=k), put together with +, are the whole file's.  A last record whose last line
    lacks its delimiter is counted with one: permute_records() writes it."""
    if _is_path(file):
        _sort_conf(key, record_lines, meta, truncate, False, first_byte, delimiter)      # (judged before the file is opened)
        with _builtin_open(file, "rb") as f:
            return sort_key_records(f, key, record_lines, meta=meta, truncate=truncate, first_byte=first_byte, delimiter=delimiter, start=start, stop=stop,
                                    first_record=first_record, max_record=max_record, allow_short=allow_short)
    return _sort_key_file(file, None, key, record_lines, meta, truncate, False, first_byte, delimiter, start, stop, first_record, max_record, allow_short)


def _sort_rows(keys):
    """keys as C-contiguous uint8 of shape (n, W), W a multiple of 8 between 8 and 256; ValueError as sort_keys() documents it"""
    if isinstance(keys, SortKeyResult):
        keys = keys.keys
    keys = np.asarray(keys)
    if keys.dtype != np.uint8 or keys.ndim != 2 or not keys.flags.c_contiguous:
        raise ValueError("keys is a SortKeyResult or a C-contiguous uint8 array of shape (n, W)")
    n, w = keys.shape
    if w % 8 or not 8 <= w <= _lib.SORT_MAX_WIDTH:
        raise ValueError(f"the rows' width is a multiple of 8 between 8 and {_lib.SORT_MAX_WIDTH}, not {w}")
    if n > _lib.SORT_MAX_KEYS:
        raise ValueError(f"sort_keys takes at most {_lib.SORT_MAX_KEYS} rows, not {n}")
    return keys


def _sort(ctx, keys, rank):
    keys = _sort_rows(keys)
    ctx = ctx or zlib_ng._ctx()                              # (the arguments are judged before a context is asked for)
    order, inverse = ctx.sort_keys(keys, bool(rank))
    return (order.astype(np.int64), inverse.astype(np.int64)) if rank else order.astype(np.int64)


def sort_keys(keys, *, rank=False):
    """Sort rows on the GPU: order[j] (int64) is the row that stands j-th in memcmp order, and equal rows come in ascending row number:
    the sort is stable, so the result depends on the rows alone.  keys is a SortKeyResult (of a file, or of shards or files put together
    with +) or any C-contiguous uint8 array of shape (n, W) with W a multiple of 8 between 8 and 256; at most 2**30 rows.
    rank=True: -> (order, rank) with rank[order[j]] == j.  Byte positions that are the same in every row cost nothing."""
    return _sort(None, keys, rank)


def _permute_order(order, n):
    """order as int64, judged: one dimension, every number at most once, and, when n is known, below it"""
    order = np.asarray(order)
    if order.ndim != 1 or (order.size and order.dtype.kind not in "iu"):
        raise ValueError("order is a one-dimensional array of record numbers")
    order = order.astype(np.int64)
    if len(order):
        if int(order.min()) < 0 or (n is not None and int(order.max()) >= n):
            i = int(np.nonzero((order < 0) | (order >= (n if n is not None else 1 << 62)))[0][0])
            raise ValueError(f"order[{i}] is {int(order[i])}: a record number lies between 0 and {'the last record' if n is None else n - 1}")
        s = np.sort(order)
        dup = np.nonzero(s[1:] == s[:-1])[0]
        if len(dup):
            raise ValueError(f"order holds record {int(s[dup[0]])} more than once")
    return order


def _permute_lengths(lengths):
    lengths = np.asarray(lengths)
    if lengths.ndim != 1 or (lengths.size and lengths.dtype.kind not in "iu") or (lengths.size and (int(lengths.min()) < 0 or int(lengths.max()) >= 1 << 32)):
        raise ValueError("lengths is a one-dimensional array of record lengths below 2**32")
    return lengths.astype(np.uint32)


class _PlaceSink:
    """what _grep_file hands a window's records to when they are written where dst says: dst[i] and lengths[i] belong to record i"""

    def __init__(self, dst, lengths, d_out, out_cap):
        self.dst, self.lengths, self.d_out, self.out_cap = dst, lengths, d_out, out_cap
        self.placed, self.bytes, self.short = 0, 0, False

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        dst, lens = (self.dst[:0], self.lengths[:0]) if self.short else (self.dst[record_base:], self.lengths[record_base:])
        _, status, tot = ctx.bgzf_place_records(data, members, text_off, text_end, delim, flags, k, first_byte, record_base, dst, lens, self.d_out, self.out_cap)
        return status, tot, b""

    def fault(self, tot, voffset):
        if tot.bad == 4:
            return (f"record {tot.bad_record} at virtual offset {voffset}: its length is not lengths[{tot.bad_record}] "
                    f"({int(self.lengths[tot.bad_record]) if tot.bad_record < len(self.lengths) else '?'}): the file changed between the passes")
        if tot.bad == 5:
            return f"record {tot.bad_record} at virtual offset {voffset} does not fit the bucket it was placed in"
        return None

    def window(self, tot, packed):
        self.short = self.short or bool(tot.labels_short)
        self.placed, self.bytes = self.placed + int(tot.placed), self.bytes + int(tot.placed_bytes)

    def finish(self, searched):
        if self.short or searched != len(self.lengths):
            raise ValueError(_SORT_OUT_OF_STEP.format(searched, len(self.lengths)))
        return self.placed, self.bytes


def _permute_buckets(sizes, chunk_bytes):
    """-> [(a, b)]: sizes[a:b] are written together; at most chunk_bytes per bucket, but at least one record"""
    ends = np.cumsum(sizes.astype(np.int64))
    cuts, a = [], 0
    while a < len(sizes):
        base = int(ends[a - 1]) if a else 0
        b = max(int(np.searchsorted(ends, base + chunk_bytes, "right")), a + 1)
        cuts.append((a, b))
        a = b
    return cuts


def _permute_file(fp, ctx, order, output, record_lines, lengths, chunk_bytes, compresslevel, block_size, first_byte, delimiter, max_record=64 << 20):
    delimiter = _partition_delimiter(delimiter)
    _grep_record_args(record_lines, None, first_byte)
    block_size = _check_block_size(block_size)
    chunk_bytes = _trim_int(chunk_bytes, 1, 1 << 40, "chunk_bytes")
    if lengths is not None:
        lengths = _permute_lengths(lengths)
    order = _permute_order(order, None if lengths is None else len(lengths))
    ctx = ctx or zlib_ng._ctx()                             # (the arguments are judged before a context is asked for)
    if lengths is None:
        lengths = _sort_key_file(fp, ctx, [], record_lines, None, False, False, first_byte, delimiter, None, None, 0, max_record, True).lengths
        order = _permute_order(order, len(lengths))
    n = len(lengths)
    sizes = lengths[order]
    buckets = _permute_buckets(sizes, chunk_bytes)
    starts = np.cumsum(sizes.astype(np.int64)) - sizes.astype(np.int64)
    cap = max([int(sizes[a:b].astype(np.int64).sum()) for a, b in buckets], default=0)
    out = _builtin_open(output, "wb") if _is_path(output) else output
    written = 0
    try:
        if buckets:
            d_out = devmem.empty(ctx, cap + 64)                  # (room behind the bucket, as every device input of the writer has)
            d_z = devmem.empty(ctx, ctx.bgzf_room(cap, block_size))
        for i, (a, b) in enumerate(buckets):
            nbytes = int(sizes[a:b].astype(np.int64).sum())
            dst = np.full(n, _lib.BGZF_PLACE_SKIP, np.uint64)
            dst[order[a:b]] = (starts[a:b] - int(starts[a])).astype(np.uint64)
            sink = _PlaceSink(dst, lengths, d_out.ptr, nbytes)
            placed, got = _grep_file(fp, ctx, None, delimiter, False, False, False, None, None, None, 0, max_record,
                                     (record_lines, None, first_byte, True), 0, None, sink)
            if placed != b - a or got != nbytes:
                raise RuntimeError(f"permute_records: {placed} records and {got} bytes were placed in a bucket of {b - a} records and {nbytes} bytes")
            _, zbytes, _ = compress_dev(ctx, d_out, nbytes, compresslevel, block_size=block_size, eof=i == len(buckets) - 1, out=d_z, table=False)
            out.write(d_z[:zbytes].cpu().tobytes())
            written += nbytes
        if not buckets:
            out.write(EOF_BLOCK)                                 # (an empty order: the empty BGZF file)
    except Exception as e:
        if out is not output:
            out.close()
        note = "permute_records: the output written so far was closed and is incomplete"
        e.args = ((f"{e.args[0]} ({note})",) + e.args[1:]) if e.args and isinstance(e.args[0], str) else e.args + (note,)
        raise
    if out is not output:
        out.close()
    return len(order), written


def permute_records(file, order, output, record_lines=4, *, lengths=None, chunk_bytes=1 << 30, compresslevel=6, block_size=MAX_BLOCK_INPUT,
                    first_byte=None, delimiter=b"\n"):
    """Write the records of a BGZF file in another order: order[j] is the number of the record written j-th.  Every record number
    appears at most once; a subset is allowed, which makes a shuffle, the head of a sorted file and a sample one call.  A number that is
    negative, repeated or -- once the record count is known: at once with lengths -- out of range is a ValueError before the output is
    opened.  lengths: SortKeyResult.lengths of the same file; without it a pass over the file gets them first.  output (a path or a
    writable binary file) becomes a complete BGZF file (compresslevel, block_size) of the records in that order, whole; a last record
    whose last line lacks its delimiter gets one, so no two lines are ever glued together.
    The output is cut at record boundaries into buckets of at most chunk_bytes (a bucket takes at least one record).  For every
    bucket the file is decoded once, its records are copied on the device to their places in a buffer of the largest bucket's size, and
    the buffer is compressed there.  A file of at most chunk_bytes costs one decode; a larger one costs ceil(text / chunk_bytes)
    decodes, with device memory bounded by chunk_bytes.  A file that holds more or fewer records than lengths is a ValueError that
    says the files are out of step; a record whose length is not its lengths entry is a ValueError that names it.  If anything is
    raised the output is closed, and the error says that it is incomplete.  -> (records written, bytes written, uncompressed)."""
    if _is_path(file):
        _permute_order(order, None if lengths is None else len(_permute_lengths(lengths)))      # (judged before a file is opened)
        _partition_delimiter(delimiter), _grep_record_args(record_lines, None, first_byte), _check_block_size(block_size)
        with _builtin_open(file, "rb") as f:
            return permute_records(f, order, output, record_lines, lengths=lengths, chunk_bytes=chunk_bytes, compresslevel=compresslevel,
                                   block_size=block_size, first_byte=first_byte, delimiter=delimiter)
    return _permute_file(file, None, order, output, record_lines, lengths, chunk_bytes, compresslevel, block_size, first_byte, delimiter)


class SortResult:
    """What sort_records() did: order (int64: order[j] is the input's record that was written j-th), records, bytes (written,
    uncompressed) and key_width."""

    def __init__(self, order, records, nbytes, key_width):
        self.order, self.records, self.bytes, self.key_width = order, int(records), int(nbytes), int(key_width)

    def __len__(self):
        return self.records

    def __repr__(self):
        return f"<SortResult: {self.records} records, {self.bytes} bytes, keys of {self.key_width} bytes>"


def _sort_file(fp, ctx, output, key, record_lines, reverse, meta, truncate, chunk_bytes, compresslevel, block_size, first_byte, delimiter, max_record,
               allow_short):
    _, _, k, _ = _sort_conf(key, record_lines, meta, truncate, reverse, first_byte, delimiter)
    _check_block_size(block_size)
    keys = _sort_key_file(fp, ctx, key, record_lines, meta, truncate, reverse, first_byte, delimiter, None, None, 0, max_record, allow_short)
    order = _sort(ctx, keys, False) if keys.key_width and keys.records else np.arange(keys.records, dtype=np.int64)
    records, nbytes = _permute_file(fp, ctx, order, output, k, keys.lengths, chunk_bytes, compresslevel, block_size, first_byte, delimiter, max_record)
    return SortResult(order, records, nbytes, keys.key_width)


def sort_records(file, output, key, record_lines=4, *, reverse=False, meta=None, truncate=False, chunk_bytes=1 << 30, compresslevel=6,
                 block_size=MAX_BLOCK_INPUT, first_byte=None, delimiter=b"\n", max_record=64 << 20, allow_short=False):
    """Sort the records of a BGZF file on the GPU: sort_key_records(), sort_keys() and permute_records() in a row.  key, meta and truncate
    are those of sort_key_records(); reverse=True turns every part's order round (meta lines stay in front).  Records with equal keys
    keep the order of the input.  output, chunk_bytes, compresslevel and block_size are those of permute_records().  -> SortResult."""
    if _is_path(file):
        _sort_conf(key, record_lines, meta, truncate, reverse, first_byte, delimiter)      # (judged before the file is opened)
        _check_block_size(block_size)
        with _builtin_open(file, "rb") as f:
            return sort_records(f, output, key, record_lines, reverse=reverse, meta=meta, truncate=truncate, chunk_bytes=chunk_bytes,
                                compresslevel=compresslevel, block_size=block_size, first_byte=first_byte, delimiter=delimiter, max_record=max_record,
                                allow_short=allow_short)
    return _sort_file(file, None, output, key, record_lines, reverse, meta, truncate, chunk_bytes, compresslevel, block_size, first_byte, delimiter,
                      max_record, allow_short)


def _per_file(value, n_files, name):
    if value is None:
        return [None] * n_files
    if not isinstance(value, (list, tuple)) or len(value) != n_files:
        raise ValueError(f"demux_paired: {name} is None or one entry per file ({n_files})")
    return list(value)


def _demux_paired_files(fps, patterns, outputs, record_lines, barcode_file, ambiguous, unassigned, compresslevel, block_size, match_line, first_byte,
                        delimiter, line_start, start, stop, first_record, max_record, allow_short, mismatches):
    """fps: (path or file, context or None) per file.  Everything is judged before the first file is opened."""
    nf = len(fps)
    pats = _classify_patterns(patterns, delimiter)
    if nf < 1 or isinstance(barcode_file, bool) or not isinstance(barcode_file, (int, np.integer)) or not 0 <= barcode_file < nf:
        raise ValueError(f"demux_paired: barcode_file is the index of one of the {nf} files")
    one = lambda o: _is_path(o) or hasattr(o, "write")       # (one output where a list of them belongs: a list of one)
    outputs = [[outputs]] if one(outputs) else [[o] if one(o) else list(o) for o in outputs]
    if len(outputs) != nf or any(len(o) != len(pats) for o in outputs):
        raise ValueError(f"demux_paired takes one output per file and pattern: {nf} files, {len(pats)} patterns")
    ambiguous, unassigned = _per_file(ambiguous, nf, "ambiguous"), _per_file(unassigned, nf, "unassigned")
    start, stop = _per_file(start, nf, "start"), _per_file(stop, nf, "stop")
    _grep_mismatches(mismatches, pats)
    _grep_record_args(record_lines, match_line, first_byte)
    _check_block_size(block_size)
    b = int(barcode_file)
    with contextlib.ExitStack() as stack:
        fps = [(stack.enter_context(_builtin_open(f, "rb")) if _is_path(f) else f, c) for f, c in fps]
        res = _demux_file(fps[b][0], fps[b][1], pats, outputs[b], record_lines, ambiguous[b], unassigned[b], compresslevel, block_size, match_line,
                          first_byte, delimiter, line_start, start[b], stop[b], first_record, max_record, allow_short, mismatches, True)
        labels = res.labels()
        for f in range(nf):
            if f != b:
                _partition_file(fps[f][0], fps[f][1], labels, outputs[f] + [ambiguous[f], unassigned[f]], record_lines, first_byte, delimiter,
                                compresslevel, block_size, start[f], stop[f], first_record, max_record, allow_short)
    return res.counts


def demux_paired(files, patterns, outputs, record_lines=4, *, barcode_file=0, ambiguous=None, unassigned=None, compresslevel=6,
                 block_size=MAX_BLOCK_INPUT, match_line=None, first_byte=None, delimiter=b"\n", line_start=False, start=None, stop=None,
                 first_record=0, max_record=64 << 20, allow_short=False, mismatches=0):
    """demux() for a run of several files whose records go together -- R1 and R2 of a paired-end run -- with the barcode in ONE of them:
    files[barcode_file] is classified and written in one pass as demux() does it, and every other file is split by those classes through
    partition_records(), record i of it following record i of the barcode file.  files are paths or seekable binary files; outputs[f][i]
    is the output of file f and pattern i; ambiguous and unassigned are None or one entry (a path, a file or None) per file, start and
    stop None or one virtual offset per file; the other keywords are demux()'s and hold for every file (match_line and mismatches for
    the barcode file alone).  -> the counts of demux().  A file whose record count differs from the barcode file's is the ValueError
    of partition_records() that says the files are out of step; the outputs written so far are closed."""
    files = [files] if _is_path(files) or hasattr(files, "read") else list(files)
    return _demux_paired_files([(f, None) for f in files], patterns, outputs, record_lines, barcode_file, ambiguous, unassigned, compresslevel,
                               block_size, match_line, first_byte, delimiter, line_start, start, stop, first_record, max_record, allow_short,
                               mismatches)


def pair_labels(first, second, pairs):
    """Dual indexes, on the host alone: first and second are the ClassifyResults of the two index reads (I1 and I2) of the same records,
    pairs the sample sheet [(i, j), ...] of pattern indices into the two.  -> int32, one label per record for partition_records():
      s                where both are assigned and (i, j) == pairs[s]
      len(pairs)       where either is AMBIGUOUS
      len(pairs) + 1   where either is UNASSIGNED (which wins over AMBIGUOUS)
      len(pairs) + 2   where both are assigned but the pair is not in the sheet: index hopping
    Results of unequal length, a pair outside the two pattern lists and a pair that stands twice are ValueErrors."""
    a, b = first.labels(), second.labels()
    if len(a) != len(b):
        raise ValueError(f"pair_labels: the two results hold {len(a)} and {len(b)} records (unequal length)")
    na, nb = len(first.counts) - 2, len(second.counts) - 2
    pairs = [(int(i), int(j)) for i, j in pairs]
    n = len(pairs)
    sheet = np.full((na, nb), n + 2, np.int32)
    for s_, (i, j) in enumerate(pairs):
        if not (0 <= i < na and 0 <= j < nb):
            raise ValueError(f"pair_labels: pair {s_} is ({i}, {j}), outside the {na} and {nb} patterns")
        if sheet[i, j] != n + 2:
            raise ValueError(f"pair_labels: pair {s_}, ({i}, {j}), stands twice in the sheet (duplicate pairs)")
        sheet[i, j] = s_
    out = np.full(len(a), n + 2, np.int32)
    both = (a < na) & (b < nb)
    out[both] = sheet[a[both], b[both]]
    out[(a == na) | (b == nb)] = n
    out[(a == na + 1) | (b == nb + 1)] = n + 1
    return out


# ---- pairs laid over each other: the overlap of the two mates, bases corrected, adapters cut, pairs merged
NONE, FOUND, MERGED, TOO_LONG = _lib.BGZF_OVERLAP_NONE, _lib.BGZF_OVERLAP_FOUND, _lib.BGZF_OVERLAP_MERGED, _lib.BGZF_OVERLAP_TOO_LONG      # an OverlapResult's verdicts
_OVERLAP_COUNTS = ("none", "found", "merged", "too_long", "bases_in", "bases_merged", "corrected", "corrected_pairs", "adapter_pairs", "adapter_trimmed",
                   "overlap_sum", "mismatch_sum")


class OverlapResult:
    """What overlap_records() decided.  Per pair, in the order of the file: offset (int64: where the reverse complement of mate 2 begins
    under mate 1, 0 without an overlap), insert (int64: the fragment's length, 0 without an overlap), overlap and mismatches (int64: the
    length of the overlap and the places in it where the mates differ), corrected_per_pair (int64: the positions correction changed),
    verdict (uint8: NONE, FOUND, MERGED, TOO_LONG), steps (uint8: bit 0 mate 1 was cut, bit 1 mate 2 was, bit 2 a base was corrected).
    The counts: records, none, found, merged, too_long, bases_in (the sequence bytes of both mates), bases_merged (those of the merged
    reads), corrected and corrected_pairs (the positions correction changed and the pairs that have one), adapter_pairs and
    adapter_trimmed (the pairs and the bases the cut took), overlap_sum and mismatch_sum (over the pairs with an overlap)."""

    def __init__(self, rows, counts):
        self.offset, self.insert = rows["offset"].astype(np.int64), rows["insert"].astype(np.int64)
        self.overlap, self.mismatches, self.corrected_per_pair = (rows[name].astype(np.int64) for name in ("overlap", "mismatches", "corrected"))
        self.verdict, self.steps = rows["verdict"].copy(), rows["steps"].copy()
        self.records = len(rows)
        for name, value in counts.items():
            setattr(self, name, int(value))

    def insert_sizes(self):
        """-> int64, entry i: the pairs whose insert is i (entry 0: the pairs without an overlap) -- fastp's insert-size histogram"""
        return np.bincount(self.insert).astype(np.int64)

    @property
    def mean_overlap(self):
        """the mean length of the overlaps found; 0.0 when there is none"""
        n = self.found + self.merged
        return self.overlap_sum / n if n else 0.0

    def __len__(self):
        return self.records

    def __repr__(self):
        return (f"<OverlapResult: {self.records} pairs, {self.merged} merged, {self.found} with an overlap, {self.none} without, "
                f"{self.too_long} too long, {self.corrected} bases corrected, {self.adapter_trimmed} cut>")


def _overlap_conf(record_lines, seq_line, qual_line, quality_base, min_overlap, mismatches, mismatch_percent, merge, correct, correct_quality,
                  cut_adapters, first_byte, delimiter):
    """-> (BgzfOverlapConf without _KEEP_UNMERGED, delimiter as bytes); ValueError as overlap_records() documents it"""
    delimiter = _partition_delimiter(delimiter)
    k, _, b = _grep_record_args(record_lines, None, first_byte)
    if k % 2:
        raise ValueError(f"record_lines is even, a pair per record (8 for interleaved FASTQ), not {k}")
    m = k // 2
    s = _trim_int(seq_line, 0, m - 1, "seq_line")
    q = -1 if qual_line is None else _trim_int(qual_line, 0, m - 1, "qual_line")
    if q == s:
        raise ValueError(f"seq_line and qual_line are two lines of a mate, not both {s}")
    for name, value in (("merge", merge), ("correct", correct), ("cut_adapters", cut_adapters)):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"{name} is True or False, not {value!r}")
    if correct and q < 0:
        raise ValueError("correct needs a qual_line")
    if not isinstance(correct_quality, (tuple, list)) or len(correct_quality) != 2:
        raise ValueError("correct_quality is a pair (high, low)")
    hi = _trim_int(correct_quality[0], 0, _lib.BGZF_OVERLAP_MAX_QUALITY, "correct_quality[0]")
    lo = _trim_int(correct_quality[1], 0, _lib.BGZF_OVERLAP_MAX_QUALITY, "correct_quality[1]")
    flags = (_lib.BGZF_OVERLAP_MERGE if merge else 0) | (_lib.BGZF_OVERLAP_CORRECT if correct else 0) | (_lib.BGZF_OVERLAP_CUT if cut_adapters else 0)
    cf = _lib.BgzfOverlapConf(k, s, q, b, _trim_int(quality_base, 0, 255, "quality_base"), _trim_int(min_overlap, 1, _lib.BGZF_OVERLAP_MAX_READ, "min_overlap"),
                              _trim_int(mismatches, 0, _lib.BGZF_OVERLAP_MAX_READ, "mismatches"), _trim_int(mismatch_percent, 0, 100, "mismatch_percent"),
                              hi, lo, flags)
    return cf, delimiter


class _OverlapSink:
    """what _grep_file hands a window's pairs to when their mates are laid over each other; writers: None (count only) or [merged,
    unmerged], None where a class is written nowhere"""

    def __init__(self, conf, writers=None):
        self.conf, self.writers = conf, writers
        self.flags = _lib.BGZF_CLASSIFY_GROUP if writers is not None and any(w is not None for w in writers) else 0
        conf.flags = (conf.flags & ~_lib.BGZF_OVERLAP_KEEP_UNMERGED) | (_lib.BGZF_OVERLAP_KEEP_UNMERGED if self.flags and writers[1] is not None else 0)
        self.rows, self.args = [], None
        self.counts = dict.fromkeys(_OVERLAP_COUNTS, 0)

    def call(self, ctx, data, members, text_off, text_end, delim, flags, k, first_byte, record_base):
        self.ctx, self.args = ctx, (data, members, text_off, text_end, delim, flags, record_base)
        _, status, tot, self.ovl, self.grows, packed = ctx.bgzf_overlap_records(data, members, text_off, text_end, delim, flags | self.flags, self.conf,
                                                                                record_base)
        return status, tot, packed

    def length_fault(self, record, voffset):
        """the message for bad = 3: the engine is asked for the four bodies' lengths, each line taken as a sequence without qualities"""
        data, members, text_off, text_end, delim, flags, record_base = self.args
        k, m, r, lens = self.conf.record_lines, self.conf.record_lines // 2, record - self.args[6], []
        for line in (self.conf.seq_line, self.conf.qual_line, m + self.conf.seq_line, m + self.conf.qual_line):
            cf = _lib.BgzfTrimConf(k, line, -1, -1, 0, 0, 0, 0, 33, 0, 1, 0, 0)
            rows = self.ctx.bgzf_trim_records(data, members, text_off, text_end, b"", np.empty((0, 2), np.uint32), delim, flags, cf, record_base)[3]
            lens.append(int(rows["end"][r]) if r < len(rows) else -1)
        mate = 0 if lens[0] != lens[1] else 1
        return (f"record {record} at virtual offset {voffset}: line {mate * m + self.conf.seq_line} (the sequence of mate {mate + 1}) has "
                f"{lens[2 * mate]} bytes and line {mate * m + self.conf.qual_line} (its qualities) has {lens[2 * mate + 1]}")

    def window(self, tot, packed):
        self.rows.append(self.ovl)
        for name in _OVERLAP_COUNTS:
            self.counts[name] += int(getattr(tot, name))
        if not self.flags:
            return
        nmerged = int(self.grows["len"][:tot.merged].sum())
        with memoryview(packed) as mv:
            if self.writers[0] is not None and nmerged:
                self.writers[0].write(mv[:nmerged])
            if self.writers[1] is not None and len(packed) > nmerged:
                self.writers[1].write(mv[nmerged:])
        if len(packed) != int(tot.bytes):
            raise RuntimeError("overlap: the classes' bytes do not add up to the records")

    def finish(self, searched):
        rows = np.concatenate(self.rows) if self.rows else np.empty(0, _lib.OVERLAP_ROW_DTYPE)
        return OverlapResult(rows, self.counts)


def _overlap_file(fp, ctx, merged, unmerged, record_lines, seq_line, qual_line, quality_base, min_overlap, mismatches, mismatch_percent, merge, correct,
                  correct_quality, cut_adapters, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record, allow_short):
    conf, delimiter = _overlap_conf(record_lines, seq_line, qual_line, quality_base, min_overlap, mismatches, mismatch_percent, merge, correct,
                                    correct_quality, cut_adapters, first_byte, delimiter)
    _check_block_size(block_size)

    def run(writers):
        sink = _OverlapSink(conf, writers)
        return _grep_file(fp, ctx, None, delimiter, False, False, False, None, start, stop, first_record, max_record,
                          (record_lines, None, first_byte, allow_short), 0, None, sink)

    if merged is None and unmerged is None:
        return run(None)
    return _with_writers("overlap_records", [merged, unmerged], compresslevel, block_size, run)


def overlap_records(file, merged=None, unmerged=None, record_lines=8, *, seq_line=1, qual_line=3, quality_base=33, min_overlap=30, mismatches=5,
                    mismatch_percent=20, merge=True, correct=False, correct_quality=(30, 14), cut_adapters=False, first_byte=None, delimiter=b"\n",
                    compresslevel=6, block_size=MAX_BLOCK_INPUT, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
    """Lay the two mates of every pair of an INTERLEAVED BGZF file over each other on the GPU, as fastp's overlap analysis, bbmerge, PEAR,
    FLASH and vsearch --fastq_mergepairs do: one record is one pair, mate 1 its first record_lines / 2 lines and mate 2 the rest (what
    fastp --interleaved_in, bbmerge in= and seqtk mergepe read and write; two separate files are not taken).  seq_line and qual_line
    (None: no qualities) name the same line of both mates.  The reverse complement of mate 2 is tried at every offset under mate 1; an
    offset counts when the mates overlap in at least min_overlap bases that differ in at most min(mismatches, overlap *
    mismatch_percent // 100) places, and of those the longest overlap wins, then the fewest mismatches, then the offset nearest 0, then
    the one that is not negative -- include/zng_amd.h states the rule.  With an overlap the fragment's length is known (insert), and
        correct       where the mates differ in the overlap and one side has a quality of at least correct_quality[0] and the other of at
                      most correct_quality[1], the weak side takes the strong side's base and quality (fastp -c)
        cut_adapters  what lies beyond the fragment's end in either mate is adapter read-through and is cut off: the one adapter finder
                      that needs no adapter sequence
        merge         the pair becomes ONE read of `insert` bases under mate 1's name: where both mates cover a position the base with
                      the higher quality stands (mate 1's on ties), its quality with it (fastp -m)
    merged is a path or writable binary file for the merged reads (record_lines / 2 lines each), unmerged an optional second one for
    every other pair (record_lines lines each, as correction and cut left them); each is written through a BgzfWriter (compresslevel,
    block_size): a complete BGZF file.  Both None: the pairs are judged and counted only.  A mate of more than 1024 bases is not
    searched (TOO_LONG) and is written whole.  Reads to be filtered first go through trim_records(..., record_lines=8, drop=); its
    output is this call's input.  record_lines, first_byte (here of both mates' first lines), delimiter, start, stop, first_record,
    max_record, allow_short and the errors of the file are those of grep_records().  -> OverlapResult.
    A mate whose sequence and qualities differ in length is a ValueError that names the record, its virtual offset and both lengths.  If
    anything is raised the outputs written so far are closed, and the error says that they are incomplete."""
    if _is_path(file):
        _overlap_conf(record_lines, seq_line, qual_line, quality_base, min_overlap, mismatches, mismatch_percent, merge, correct, correct_quality,
                      cut_adapters, first_byte, delimiter)       # (judged before the file is opened)
        _check_block_size(block_size)
        with _builtin_open(file, "rb") as f:
            return overlap_records(f, merged, unmerged, record_lines, seq_line=seq_line, qual_line=qual_line, quality_base=quality_base,
                                   min_overlap=min_overlap, mismatches=mismatches, mismatch_percent=mismatch_percent, merge=merge, correct=correct,
                                   correct_quality=correct_quality, cut_adapters=cut_adapters, first_byte=first_byte, delimiter=delimiter,
                                   compresslevel=compresslevel, block_size=block_size, start=start, stop=stop, first_record=first_record,
                                   max_record=max_record, allow_short=allow_short)
    return _overlap_file(file, None, merged, unmerged, record_lines, seq_line, qual_line, quality_base, min_overlap, mismatches, mismatch_percent, merge,
                         correct, correct_quality, cut_adapters, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record,
                         allow_short)


# ---- lines by region: a tabix index built on the GPU, and the rows of a region filtered there
TABIX_MAGIC = b"TBI\x01"
TABIX_PRESETS = {"gff": (0, 1, 4, 5, 35, 0), "bed": (0x10000, 1, 2, 3, 35, 0), "vcf": (2, 1, 2, 0, 35, 0)}
TABIX_MAX_POS = 1 << 29                       # the largest end a .tbi can hold
_TABIX_PSEUDO_BIN = 37450                     # htslib's bin of per-name statistics: read and dropped, never written
_TABIX_MAX_LINE = 64 << 20                    # a line that is still open after this many bytes of a window: ValueError
_TABIX_LEVELS = ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681))
_TABIX_KINDS = {1: "a needed column is missing", 2: "a coordinate is not 1 to 10 digits", 3: "the interval leaves [0, 2**29]",
                4: "its start lies below the previous line's of the same name", "contig": "its name came before, with other names in between"}


def reg2bin(beg, end):
    """the bin of [beg, end) (SAM specification section 5.3: five levels, 16 KiB leaves)"""
    end -= 1
    for shift, first in reversed(_TABIX_LEVELS):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def reg2bins(beg, end):
    """the bins that may hold a feature overlapping [beg, end)"""
    end -= 1
    out = [0]
    for shift, first in _TABIX_LEVELS:
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def parse_region(region):
    """"chr1:1,000-2,000" -> (b"chr1", 999, 2000): tabix's 1-based inclusive convention, commas ignored; "chr1" is the whole name and
    "chr1:1000" reaches to the end.  A tuple (name, beg0, end0) is taken as zero-based half-open."""
    if isinstance(region, tuple):
        if len(region) != 3:
            raise ValueError("a region tuple is (name, beg, end)")
        name, beg, end = region
        name = name.encode() if isinstance(name, str) else bytes(name)
        beg, end = int(beg), int(end)
        if beg < 0 or end < 0:
            raise ValueError("region coordinates are not negative")
        return name, beg, end
    text = region.encode() if isinstance(region, str) else bytes(region)
    if not text:
        raise ValueError("empty region")
    name, sep, rest = text.rpartition(b":")
    if sep:
        rest = rest.replace(b",", b"")
        lo, dash, hi = rest.partition(b"-")
        if lo.isdigit() and (not dash or hi.isdigit()) and name:
            a, b = int(lo), int(hi) if dash else TABIX_MAX_POS
            if b < a:
                raise ValueError(f"region {text!r}: the end lies below the start")
            return name, max(a - 1, 0), b
    return text, 0, TABIX_MAX_POS


def _tabix_conf(preset, seq_col, start_col, end_col, zero_based, meta, skip):
    """-> (format, col_seq, col_beg, col_end, meta, skip); ValueError as TabixIndex.build documents it"""
    meta = bytes(meta)
    skip = int(skip)
    if len(meta) != 1:
        raise ValueError("meta is exactly one byte")
    if not 0 <= skip < 1 << 31:
        raise ValueError("skip lies between 0 and 2**31 - 1")
    if preset is not None:
        if seq_col is not None or start_col is not None or end_col is not None or zero_based:
            raise ValueError("a preset or columns, not both")
        if preset == "sam":
            raise ValueError("the SAM preset needs CIGAR: not supported")
        if preset not in TABIX_PRESETS:
            raise ValueError(f"unknown preset {preset!r}: gff, bed or vcf")
        fmt, cs, cb, ce = TABIX_PRESETS[preset][:4]
    else:
        if seq_col is None or start_col is None:
            raise ValueError("a preset, or seq_col and start_col")
        fmt, cs, cb, ce = (0x10000 if zero_based else 0), int(seq_col), int(start_col), int(end_col or 0)
        if not 1 <= cs < 1 << 31 or not 1 <= cb < 1 << 31 or not 0 <= ce < 1 << 31:
            raise ValueError("columns are counted from 1")
    return fmt, cs, cb, ce, meta[0], skip


class _TabixBad(ValueError):
    def __init__(self, line, kind, voffset):
        super().__init__(f"line {line} at virtual offset {voffset} cannot be indexed: {_TABIX_KINDS[kind]}")
        self.line, self.kind, self.voffset = line, kind, voffset


class _TabixMerge:
    """The tables of the windows become one index (pure host code).  Per window: names [(name, line, voffset)] per name run, bins
    [(name run, bin, v_beg, v_end)] (v_end None: the run ends where the window's text ends), wins [(name run, window, voffset)],
    the first and last beg of its data lines, head: the virtual offset of its first text byte (None: no text)."""

    def __init__(self):
        self.names, self.ids, self.bins, self.linear = [], {}, [], []
        self.last = self.prev = self.open_end = None

    def add(self, names, bins, wins, first_beg, last_beg, head=None, bad=None):
        if self.open_end is not None and head is not None:
            self.open_end[1], self.open_end = head, None
        errs = [bad] if bad is not None else []
        if names and self.prev is not None and names[0][0] == self.prev[0] and first_beg < self.prev[1]:
            errs.append((names[0][1], 4, names[0][2]))        # out of order across the cut
        run_ids = []
        for name, line, v in names:
            if self.names and self.names[-1] == name:
                run_ids.append(len(self.names) - 1)
            elif name in self.ids:
                errs.append((line, "contig", v))
                break
            else:
                self.ids[name] = len(self.names)
                run_ids.append(len(self.names))
                self.names.append(name)
                self.bins.append({})
                self.linear.append([])
        if errs:
            raise _TabixBad(*min(errs, key=lambda e: e[0]))
        for run, b, vb, ve in bins:
            i = run_ids[run]
            if self.last == (i, b):
                chunk = self.bins[i][b][-1]
                chunk[1] = ve
            else:
                chunk = [vb, ve]
                self.bins[i].setdefault(b, []).append(chunk)
                self.last = (i, b)
            self.open_end = chunk if ve is None else None
        for run, w, v in wins:
            lin = self.linear[run_ids[run]]
            if w >= len(lin):                               # this line is the first to reach the windows up to w
                lin.extend([v] * (w + 1 - len(lin)))
        if names:
            self.prev = (names[-1][0], last_beg)

    def finish(self, conf, end_v):
        """end_v: the virtual offset behind the file's last data byte"""
        if self.open_end is not None:
            self.open_end[1], self.open_end = end_v, None
        return TabixIndex(conf, self.names, [{b: [tuple(c) for c in cs] for b, cs in d.items()} for d in self.bins], self.linear)


def _tabix_voffsets(src, out_offs, isizes, coffs):
    """scratch offsets -> (normalised virtual offsets, mask: the offset lies at or behind the end of the decoded blocks).  out_offs /
    isizes / coffs: where each decoded block's output lies, its length, the block's offset in the file."""
    src = np.asarray(src, np.int64)
    full = np.nonzero(isizes > 0)[0]
    if not len(full):
        return np.zeros(len(src), np.uint64), np.ones(len(src), bool)
    offs, cs = out_offs[full].astype(np.int64), coffs[full].astype(np.int64)
    beyond = src >= int(offs[-1] + isizes[full[-1]])
    at = np.clip(np.searchsorted(offs, src, "right") - 1, 0, len(offs) - 1)
    return (cs[at].astype(np.uint64) << np.uint64(16)) | (src - offs[at]).astype(np.uint64), beyond


class TabixIndex:
    """A tabix index (.tbi) of a BGZF file of tab-separated lines sorted by name and start: names in order of first appearance; per
    name, per bin (SAM specification section 5.3) the chunks (v_beg, v_end) of virtual offsets that hold its lines, and the linear
    index, the smallest virtual offset of a line overlapping each 16 KiB window.  build() makes one on the GPU; chunks() answers a
    region on the host; BgzfReader.fetch() reads a region's lines.  On disk the standard layout, BGZF-compressed; what this project
    writes has no pseudo-bin 37450 and no trailing n_no_coor; load() accepts both, and a plain blob that starts with the magic."""

    def __init__(self, conf, names, bins, linear):
        self.conf = tuple(int(x) for x in conf)
        self._names = [bytes(n) for n in names]
        self.bins = [{int(b): [(int(x), int(y)) for x, y in cs] for b, cs in d.items()} for d in bins]
        self.linear = [[int(v) for v in lin] for lin in linear]
        if len(self.conf) != 6 or not len(self._names) == len(self.bins) == len(self.linear):
            raise ValueError("tabix index: tables of different lengths")
        self._ids = {n: i for i, n in enumerate(self._names)}
        if len(self._ids) != len(self._names):
            raise ValueError("tabix index: a name appears twice")
        self._keys = [np.array(sorted(d), np.int64) for d in self.bins]

    @property
    def names(self):
        return list(self._names)

    def __len__(self):
        return len(self._names)

    def __eq__(self, other):
        return (isinstance(other, TabixIndex) and self.conf == other.conf and self._names == other._names and self.bins == other.bins and
                self.linear == other.linear)

    __hash__ = None

    def validate(self, file_size):
        """ValueError unless every chunk satisfies v_beg < v_end and lies inside a file of file_size bytes"""
        file_size = int(file_size)
        for name, d in zip(self._names, self.bins):
            for b, cs in d.items():
                for vb, ve in cs:
                    if not 0 <= vb < ve < 1 << 64 or vb >> 16 >= file_size or ve >> 16 > file_size:
                        raise ValueError(f"tabix index: chunk ({vb}, {ve}) of {name!r}, bin {b}, does not fit a file of {file_size} bytes")

    # ---- regions
    def chunks(self, name, beg, end):
        """[(v_beg, v_end), ...], sorted and merged where they overlap or touch: every line of `name` that overlaps [beg, end)
        (zero-based, half-open; an empty interval is [beg, beg + 1)) starts inside one of them.  An unknown name: []."""
        name = name.encode() if isinstance(name, str) else bytes(name)
        i = self._ids.get(name)
        beg, end = max(int(beg), 0), int(end)
        if end <= beg:
            end = beg + 1
        end = min(end, TABIX_MAX_POS)
        if i is None or beg >= end:
            return []
        lin = self.linear[i]
        if beg >> 14 >= len(lin):                            # no line of the name reaches this window
            return []
        floor, keys, found = lin[beg >> 14], self._keys[i], []
        levels = [(0, 0)] + [(first + (beg >> shift), first + ((end - 1) >> shift)) for shift, first in _TABIX_LEVELS]
        for lo, hi in levels:
            for b in keys[np.searchsorted(keys, lo, "left"):np.searchsorted(keys, hi, "right")].tolist():
                found.extend(c for c in self.bins[i][b] if c[1] > floor)
        found.sort()
        out = []
        for vb, ve in found:
            if out and vb <= out[-1][1]:
                out[-1] = (out[-1][0], max(out[-1][1], ve))
            else:
                out.append((vb, ve))
        return out

    # ---- on disk
    def to_bytes(self, compressed=True):
        """the .tbi bytes; compressed=False: the plain layout, not BGZF-compressed"""
        blob = b"".join(n + b"\0" for n in self._names)
        parts = [TABIX_MAGIC, struct.pack("<8i", len(self._names), *self.conf, len(blob)), blob]
        for d, lin in zip(self.bins, self.linear):
            parts.append(struct.pack("<i", len(d)))
            for b in sorted(d):
                parts.append(struct.pack("<Ii", b, len(d[b])))
                parts.append(np.array(d[b], np.uint64).reshape(-1, 2).astype("<u8").tobytes())
            parts.append(struct.pack("<i", len(lin)))
            parts.append(np.array(lin, np.uint64).astype("<u8").tobytes())
        raw = b"".join(parts)
        return compress(raw) if compressed else raw

    def save(self, path_or_file):
        if hasattr(path_or_file, "write"):
            path_or_file.write(self.to_bytes())
        else:
            with _builtin_open(path_or_file, "wb") as f:
                f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, blob):
        """ValueError (with the offset) for a blob that is not a .tbi: counts that overrun it, negative counts, names that do not end
        in NUL.  A BGZF-compressed blob is decompressed first; one that starts with the magic is taken as it is."""
        blob = bytes(blob)
        if not blob.startswith(TABIX_MAGIC):
            if not blob.startswith(b"\x1f\x8b"):
                raise ValueError("tabix index: neither BGZF nor the magic at offset 0")
            try:
                blob = bytes(decompress(blob))
            except (BadGzipFile, EOFError) as e:
                raise ValueError(f"tabix index: {e}") from None
            if not blob.startswith(TABIX_MAGIC):
                raise ValueError("tabix index: wrong magic at offset 0")
        at = 4

        def take(fmt, what):
            nonlocal at
            size = struct.calcsize(fmt)
            if len(blob) - at < size:
                raise ValueError(f"tabix index: {what} at offset {at} overruns the {len(blob)} bytes")
            vals = struct.unpack_from(fmt, blob, at)
            at += size
            return vals

        def count(what, unit):
            n, = take("<i", what)
            if n < 0 or n * unit > len(blob) - at:
                raise ValueError(f"tabix index: {what} {n} at offset {at - 4} is negative or overruns the {len(blob)} bytes")
            return n

        n_ref = count("n_ref", 1)
        conf = take("<6i", "the configuration")
        l_nm = count("l_nm", 1)
        names = blob[at:at + l_nm]
        if l_nm and not names.endswith(b"\0"):
            raise ValueError(f"tabix index: the names at offset {at} do not end in NUL")
        names = names.split(b"\0")[:-1] if l_nm else []
        if len(names) != n_ref:
            raise ValueError(f"tabix index: {len(names)} names at offset {at} for n_ref = {n_ref}")
        at += l_nm
        bins, linear = [], []
        for _ in range(n_ref):
            d = {}
            for _ in range(count("n_bin", 8)):
                b, = take("<I", "a bin")
                n = count("n_chunk", 16)
                if b > _TABIX_PSEUDO_BIN or b in d:
                    raise ValueError(f"tabix index: bin {b} at offset {at - 8} is out of range or repeated")
                cs = np.frombuffer(blob, "<u8", 2 * n, at).reshape(-1, 2).tolist()
                at += 16 * n
                if b != _TABIX_PSEUDO_BIN:
                    d[b] = cs
            n = count("n_intv", 8)
            linear.append(np.frombuffer(blob, "<u8", n, at).tolist())
            at += 8 * n
            bins.append(d)
        if len(blob) - at not in (0, 8):                     # (8: htslib's n_no_coor)
            raise ValueError(f"tabix index: {len(blob) - at} bytes behind the last name's tables at offset {at}")
        return cls(conf, names, bins, linear)

    @classmethod
    def load(cls, path_or_file):
        if hasattr(path_or_file, "read"):
            return cls.from_bytes(path_or_file.read())
        with _builtin_open(path_or_file, "rb") as f:
            return cls.from_bytes(f.read())

    # ---- building
    @classmethod
    def build(cls, file, preset=None, *, seq_col=None, start_col=None, end_col=None, zero_based=False, meta=b"#", skip=0):
        """Index a BGZF file (a path or a seekable binary file) on the GPU.  preset: "gff", "bed" or "vcf" (tabix's); or columns by
        keyword, counted from 1: seq_col, start_col, end_col (none: features of one base), zero_based (half-open, as BED).  meta: lines
        that start with this byte are skipped, and so are the first `skip` lines and empty ones.  The file is read in windows as grep()
        reads it; each window's blocks are decoded in one launch, the fields of every line are read where they lie, and name runs, bin
        runs and the window records of the linear index come back -- nothing per line.  ValueError, naming the smallest such line
        number and its virtual offset, for a line with a needed column missing, a coordinate that is not 1 to 10 digits, an interval
        outside [0, 2**29] or a start below the previous line's of the same name, and for a name that comes back after another;
        BadGzipFile for a file that is not BGZF or a block that does not decode."""
        conf = _tabix_conf(preset, seq_col, start_col, end_col, zero_based, meta, skip)
        if _is_path(file):
            with _builtin_open(file, "rb") as f:
                return _tabix_build(f, None, conf)
        return _tabix_build(file, None, conf)


def _tabix_window(tot, names, blob, bins, wins, out_offs, isizes, coffs):
    """one engine call's tables -> the arguments of _TabixMerge.add (pure host code)"""
    nv, _ = _tabix_voffsets(names["src_off"], out_offs, isizes, coffs)
    ends = np.cumsum(names["len"].astype(np.int64))
    nm = [(blob[int(e - ln):int(e)], int(line), int(v)) for e, ln, line, v in zip(ends, names["len"], names["line"], nv)]
    vb, _ = _tabix_voffsets(bins["src_beg"], out_offs, isizes, coffs)
    ve, beyond = _tabix_voffsets(bins["src_end"], out_offs, isizes, coffs)
    bn = [(int(r), int(b), int(x), None if o else int(y)) for r, b, x, y, o in zip(bins["name"], bins["bin"], vb, ve, beyond)]
    wv, _ = _tabix_voffsets(wins["src_off"], out_offs, isizes, coffs)
    wn = [(int(r), int(w), int(v)) for r, w, v in zip(wins["name"], wins["window"], wv)]
    bad = None
    if tot.bad_kind:
        v, _ = _tabix_voffsets([tot.bad_src], out_offs, isizes, coffs)
        bad = (int(tot.bad_line), int(tot.bad_kind), int(v[0]))
    return nm, bn, wn, int(tot.first_beg), int(tot.last_beg), bad


def _tabix_build(fp, ctx, conf):
    ctx = ctx or zlib_ng._ctx()                              # (the arguments are judged before a context is asked for)
    merge = _TabixMerge()
    c_next, text_off, text_cap = 0, 0, max(_GREP_TEXT, _TABIX_MAX_LINE + 2 * MAX_BLOCK)
    window, nblocks, line_base, after = _READ_WINDOW, 0, 0, 0
    buf = mv = None
    try:
        while True:
            if buf is None or len(buf) < window + MAX_BLOCK:
                if buf is not None:
                    del mv
                    _lib.give_buffer(buf)
                buf = _lib.take_buffer(window + MAX_BLOCK)
                mv = memoryview(buf)
            fp.seek(c_next)
            got = _read_full(fp, mv[:window + MAX_BLOCK])
            if not got:
                break
            data = mv[:got]
            ended = got < window + MAX_BLOCK
            code, tab, used, total = _lib.bgzf_scan(data)
            if ended and used < got and _cut_block(data[used:]):
                raise EOFError(f"BGZF block {nblocks + len(tab)} at offset {c_next + used}: the file ends inside the block")
            if code != _lib.OK or not tab:
                raise _scan_error(code if c_next + used == 0 else _lib.DATA_ERROR, nblocks + len(tab), c_next + used)
            t = np.array(tab, np.int64)
            coffs, csizes, isizes = t[:, 0], t[:, 2], t[:, 3]
            n_use, text_end, final = _grep_window(coffs + c_next, isizes, text_off, None, ended and used == got, text_cap)
            members, bad = _member_table(np.frombuffer(data, np.uint8), coffs[:n_use], csizes[:n_use], isizes[:n_use])
            if bad >= 0:
                raise BadGzipFile(f"BGZF block {nblocks + bad} at offset {c_next + int(coffs[bad])}: bad block header or block size")
            cend = int(coffs[n_use - 1] + csizes[n_use - 1]) if n_use else 0
            _, status, tot, names, blob, bins, wins = ctx.bgzf_tabix(data[:cend], members, text_off, text_end, conf, 10,
                                                                     _lib.BGZF_TABIX_FINAL if final else 0, line_base)
            bad = np.nonzero(status)[0]
            if len(bad):
                raise _block_error(c_next + int(coffs[bad[0]]), status[bad[0]])
            if not tot.covered:
                raise BadGzipFile(f"BGZF blocks at offset {c_next}: the decoded blocks do not cover the text")
            out_offs, abs_c = members["out_off"].astype(np.int64), coffs[:n_use] + c_next
            full = np.nonzero(isizes[:n_use] > 0)[0]
            if len(full):
                after = max(after, int(abs_c[full[-1]] + csizes[full[-1]]))
            head = None
            if text_end > text_off:
                hv, _ = _tabix_voffsets([text_off], out_offs, isizes[:n_use], abs_c)
                head = int(hv[0])
            nm, bn, wn, first_beg, last_beg, bad = _tabix_window(tot, names, blob, bins, wins, out_offs, isizes[:n_use], abs_c)
            merge.add(nm, bn, wn, first_beg, last_beg, head=head, bad=bad)
            line_base += tot.seen
            try:
                nxt = _grep_advance(isizes, n_use, text_off, text_end, int(tot.tail_off), final, window, _TABIX_MAX_LINE)
            except _LongLine as e:
                v = make_virtual_offset(c_next + int(coffs[e.block]), e.offset)
                raise ValueError(f"the line at virtual offset {v} has not ended after {_TABIX_MAX_LINE} bytes") from None
            if nxt is None:
                break
            b, text_off, window = nxt
            nblocks += b
            c_next += int(coffs[b]) if b < len(coffs) else used
    finally:
        if buf is not None:
            del mv
            _lib.give_buffer(buf)
    return merge.finish(conf, after << 16)


class FetchResult:
    """What fetch() found: len() lines; region (int64: the index into `regions` of each row, ascending), voffsets (uint64, the
    normalised virtual offset of each line's first byte), offsets (int64, n + 1 of them) into data (the lines packed, each with its
    delimiter); result[i], slices and iteration yield bytes; of(i): the lines of region i."""

    def __init__(self, region, voffsets, offsets, data, n_regions):
        self.region = np.asarray(region, np.int64)
        self.voffsets = np.asarray(voffsets, np.uint64)
        self.offsets = np.asarray(offsets, np.int64)
        self.data = data
        self.n_regions = int(n_regions)
        if len(self.offsets) != len(self.region) + 1 or len(self.voffsets) != len(self.region):
            raise ValueError("FetchResult: arrays of different lengths")

    def __len__(self):
        return len(self.region)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        n = len(self)
        k = int(i)
        if not -n <= k < n:
            raise IndexError("FetchResult index out of range")
        k %= n
        return bytes(self.data[int(self.offsets[k]):int(self.offsets[k + 1])])

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def of(self, i):
        """the lines of region i"""
        if not 0 <= int(i) < self.n_regions:
            raise IndexError("FetchResult.of: no such region")
        a, b = np.searchsorted(self.region, [int(i), int(i) + 1])
        return [self[k] for k in range(int(a), int(b))]

    def __repr__(self):
        return f"<FetchResult: {len(self)} lines of {self.n_regions} regions, {int(self.offsets[-1])} bytes>"


def _fetch_regions(regions):
    """-> ([(name, beg, end)], whether one region was given rather than a list)"""
    single = isinstance(regions, (str, bytes, tuple))
    out = []
    for r in ([regions] if single else list(regions)):
        name, beg, end = parse_region(r)
        if end <= beg:
            end = beg + 1
        out.append((name, min(beg, TABIX_MAX_POS), min(end, TABIX_MAX_POS)))
    return out, single


def _fetch_groups(spans, chains, isize_of, text_cap, max_regions):
    """Cut the spans [(region, v_beg, v_end)] (in order) into engine calls: each decodes the blocks of its spans once, at most text_cap
    bytes of them (one span may exceed it) for at most max_regions regions.  chains: per span its blocks' file offsets.
    -> [(first span, behind the last span)] (pure host code)"""
    groups, start, blocks, regs, size = [], 0, set(), set(), 0
    for k, (span, chain) in enumerate(zip(spans, chains)):
        new = [c for c in chain if c not in blocks]
        add = sum(isize_of[c] for c in new)
        if k > start and (size + add > text_cap or (span[0] not in regs and len(regs) >= max_regions)):
            groups.append((start, k))
            start, blocks, regs, size = k, set(), set(), 0
            new, add = list(chain), sum(isize_of[c] for c in chain)
        blocks.update(new)
        regs.add(span[0])
        size += add
    if len(spans) > start:
        groups.append((start, len(spans)))
    return groups


_STALE_TBI = "tabix index does not match the file"


def _fetch_file(fp, fsize, ctx, index, regions, count, load_block):
    regs, single = _fetch_regions(regions)
    if not isinstance(index, TabixIndex):
        raise TypeError("fetch() takes a TabixIndex")
    if index.conf[0] & 0xFFFF not in (0, 2) or index.conf[0] & ~0x1FFFF or index.conf[1] < 1 or index.conf[2] < 1 or index.conf[3] < 0 or \
            not 0 <= index.conf[4] <= 255 or index.conf[5] < 0:
        raise ValueError("fetch(): the index's configuration is not one of generic, BED-like or VCF")
    index.validate(fsize)
    spans = [(i, vb, ve) for i, (name, beg, end) in enumerate(regs) for vb, ve in index.chunks(name, beg, end)]
    counts = [0] * len(regs)
    empty = FetchResult([], [], [0], b"", len(regs))
    if not spans:
        return (counts[0] if single else counts) if count else empty
    ctx = ctx or zlib_ng._ctx()                              # (the arguments are judged before a context is asked for)
    cache, chains = {}, []
    for _, vb, ve in spans:                                  # the blocks of a chunk: from its first one through BSIZE
        (c, ub), (ce, ue) = split_virtual_offset(vb), split_virtual_offset(ve)
        chain = []
        while c < ce or (c == ce and ue > 0):
            blk = load_block(c, cache) if c < fsize else None
            if blk is None or (not chain and ub >= blk[2]) or (c == ce and ue > blk[2]):
                raise ValueError(_STALE_TBI)
            chain.append(c)
            c += len(blk[0])
        if not chain or (c != ce and ue == 0) or (ue and chain[-1] != ce):
            raise ValueError(_STALE_TBI)
        chains.append(chain)
    isize_of = {c: b[2] for c, b in cache.items() if b is not None}
    region_parts, voff_parts, len_parts, pieces = [], [], [], []
    for a, b in _fetch_groups(spans, chains, isize_of, _GREP_TEXT, _lib.BGZF_FETCH_MAX_REGIONS):
        need = sorted({c for chain in chains[a:b] for c in chain})
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
        where = dict(zip(need, opos.tolist()))
        local = {}                                           # the regions of this call, numbered from 0
        for i, _, _ in spans[a:b]:
            local.setdefault(i, len(local))
        glob = np.fromiter(local, np.int64, len(local))
        rtab = np.zeros(len(local), _lib.TABIX_REGION_DTYPE)
        blob = b"".join(regs[i][0] for i in local)
        nlen = np.fromiter((len(regs[i][0]) for i in local), np.uint32, len(local))
        rtab["name_len"], rtab["name_off"] = nlen, np.cumsum(nlen, dtype=np.uint64) - nlen
        rtab["beg"], rtab["end"] = [regs[i][1] for i in local], [regs[i][2] for i in local]
        stab = np.zeros(b - a, _lib.TABIX_SPAN_DTYPE)
        for k, ((i, vb, ve), chain) in enumerate(zip(spans[a:b], chains[a:b])):
            ue = ve & 0xFFFF
            stab[k] = (where[chain[0]] + (vb & 0xFFFF), where[chain[-1]] + (ue if ue else cache[chain[-1]][2]), local[i], 0)
        _, status, sstat, srows, tot, rows, packed = ctx.bgzf_fetch(b"".join(raws), members, index.conf, 10,
                                                                    _lib.BGZF_FETCH_COUNT_ONLY if count else 0, blob, rtab, stab)
        bad = np.nonzero(status)[0]
        if len(bad):
            raise _block_error(need[int(bad[0])], status[bad[0]])
        if bool(sstat.any()):
            raise ValueError(_STALE_TBI)
        for k, n in enumerate(srows.tolist()):
            counts[spans[a + k][0]] += n
        if len(rows):
            v, _ = _tabix_voffsets(rows["src_off"], opos.astype(np.int64), members["out_len"].astype(np.int64), np.array(need, np.int64))
            region_parts.append(glob[rows["region"]])
            voff_parts.append(v)
            len_parts.append(rows["len"].astype(np.int64))
            pieces.append(packed)
    if count:
        return counts[0] if single else counts
    if not region_parts:
        return empty
    lens = np.concatenate(len_parts)
    offsets = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    return FetchResult(np.concatenate(region_parts), np.concatenate(voff_parts), offsets, pieces[0] if len(pieces) == 1 else b"".join(pieces),
                       len(regs))


def fetch(file, index, regions, *, count=False):
    """The lines of a BGZF file (a path or a seekable binary file) that overlap `regions`: one region or a list of them, each a
    string as parse_region() reads it or a tuple (name, beg, end), zero-based and half-open.  `index`: the file's TabixIndex.  The
    plan is made on the index alone (chunks() per region); every needed block is read and decoded once, the lines of each chunk are
    filtered on the GPU by name and interval, and only the matching lines come back: a FetchResult, in the order of the regions and
    then of the file.  count=True: the number of lines per region (a list; an int for one region); no line leaves the device.
    ValueError for an index that does not fit the file, BadGzipFile (with its offset; no partial result) for a block that fails."""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return fetch(f, index, regions, count=count)
    fsize = file.seek(0, 2)

    def load_block(c, cache):                                # (as BgzfReader._load_block)
        if c not in cache:
            file.seek(c)
            raw = file.read(MAX_BLOCK)
            code, tab, used, total = _lib.bgzf_scan(raw, 1) if raw else (_lib.OK, [], 0, 0)
            if raw and (code != _lib.OK or not tab):
                raise BadGzipFile(f"BGZF block at offset {c}: bad block header or block size")
            cache[c] = (raw[:used], 12 + struct.unpack_from("<H", raw, 10)[0], tab[0][3]) if raw else None
        return cache[c]
    return _fetch_file(file, fsize, None, index, regions, count, load_block)


# ---- bases by sequence: a FASTA index built on the GPU, and subsequences gathered there
_FAIDX_MAX_LINE = 512 << 20                   # a line that is still open after this many bytes of a window: ValueError.  Twice the longest
                                              # human chromosome on one line; with two blocks it still fits the 1 GiB text of one engine call
_FAIDX_KINDS = {1: "a header with an empty name", 2: "a sequence line holds a byte outside 0x21..0x7E",
                3: "its length differs from the first line of its sequence", 4: "an empty line inside a sequence",
                5: "sequence in front of the first header"}
_STALE_FAI = "faidx index does not match the file"


class _FaidxBad(ValueError):
    def __init__(self, line, kind, voffset):
        super().__init__(f"line {line} at virtual offset {voffset} cannot be indexed: {_FAIDX_KINDS[kind]}")
        self.line, self.kind, self.voffset = line, kind, voffset


class FaidxIndex:
    """The .fai index of a FASTA file: per sequence, in file order, its name and (LENGTH, OFFSET, LINEBASES, LINEWIDTH) -- bases, the
    uncompressed offset of its first base, bases and bytes per line.  For a BGZF file it goes with a GziIndex (`gzi`, None when it
    was loaded without one).  build() makes both on the GPU; fetch_seq() reads subsequences with them."""

    def __init__(self, rows, gzi=None):
        self._names, self._rows = [], {}
        for name, length, offset, lb, lw in rows:
            name = bytes(name)
            vals = (int(length), int(offset), int(lb), int(lw))
            if not name or min(vals) < 0 or vals[3] < vals[2] or max(vals) >= 1 << 63:
                raise ValueError(f"fai row {len(self._names)}: not a name and four numbers with LINEWIDTH >= LINEBASES")
            if name in self._rows:
                raise ValueError(f"fai row {len(self._names)}: the name {name!r} occurs twice")
            self._names.append(name)
            self._rows[name] = vals
        self.gzi = gzi

    @property
    def names(self):
        return list(self._names)

    def __len__(self):
        return len(self._names)

    def __contains__(self, name):
        return (name.encode() if isinstance(name, str) else bytes(name)) in self._rows

    def __getitem__(self, name):
        """-> (length, offset, line_bases, line_width); KeyError for a name the index does not hold"""
        return self._rows[name.encode() if isinstance(name, str) else bytes(name)]

    def __eq__(self, other):
        return isinstance(other, FaidxIndex) and self._names == other._names and self._rows == other._rows

    def to_bytes(self):
        """the five-column .fai text"""
        return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % ((n,) + self._rows[n]) for n in self._names)

    @classmethod
    def from_bytes(cls, blob, gzi=None):
        rows = []
        for i, line in enumerate(bytes(blob).split(b"\n")):
            if line.endswith(b"\r"):
                line = line[:-1]
            if not line:
                continue
            cols = line.split(b"\t")
            if len(cols) == 6:
                raise ValueError(f"fai line {i}: six columns, a FASTQ index (fqidx) -- not supported")
            if len(cols) != 5 or not all(c.isdigit() for c in cols[1:]):
                raise ValueError(f"fai line {i}: not a name and four numbers")
            rows.append((cols[0],) + tuple(int(c) for c in cols[1:]))
        return cls(rows, gzi)

    def save(self, fai_path, gzi_path=None):
        """the .fai text, and with gzi_path the .gzi next to it"""
        if hasattr(fai_path, "write"):
            fai_path.write(self.to_bytes())
        else:
            with _builtin_open(fai_path, "wb") as f:
                f.write(self.to_bytes())
        if gzi_path is not None:
            if self.gzi is None:
                raise ValueError("this index holds no gzi")
            self.gzi.save(gzi_path)

    @classmethod
    def load(cls, fai_path, gzi_path=None):
        """without gzi_path, `gzi` is None and fetch_seq() walks the file's block headers for one (GziIndex.build)"""
        if hasattr(fai_path, "read"):
            blob = fai_path.read()
        else:
            with _builtin_open(fai_path, "rb") as f:
                blob = f.read()
        return cls.from_bytes(blob, GziIndex.load(gzi_path) if gzi_path is not None else None)

    @classmethod
    def build(cls, file):
        """Index a bgzipped FASTA (a path or a seekable binary file) on the GPU.  The file is read in windows as grep() reads it; each
        window's blocks are decoded in one launch, the record structure is read where the text lies, and one row per header comes
        back -- nothing per line.  ValueError with .line, .kind and .voffset for the smallest bad line (the line model: INTEGRATION.md),
        ValueError for a name that occurs twice (it names both header lines); BadGzipFile for a file that is not BGZF or a block that
        does not decode.  The GziIndex of the blocks that were walked is kept as `gzi`."""
        if _is_path(file):
            with _builtin_open(file, "rb") as f:
                return _faidx_build(f, None)
        return _faidx_build(file, None)


def _faidx_build(fp, ctx):
    ctx = ctx or zlib_ng._ctx()
    recs, blocks = [], []                                    # [name, line, length, offset, line_bases, line_width]; (coffset, uoffset, csize, isize)
    carry, last_v = None, (0, 0)                             # last_v: where carry.last_line and the line behind it start
    c_next, u_next, text_off, text_cap = 0, 0, 0, max(_GREP_TEXT, _FAIDX_MAX_LINE + 2 * MAX_BLOCK)
    window, nblocks, line_base, final = _READ_WINDOW, 0, 0, False
    buf = mv = None
    try:
        while True:
            if buf is None or len(buf) < window + MAX_BLOCK:
                if buf is not None:
                    del mv
                    _lib.give_buffer(buf)
                buf = _lib.take_buffer(window + MAX_BLOCK)
                mv = memoryview(buf)
            fp.seek(c_next)
            got = _read_full(fp, mv[:window + MAX_BLOCK])
            if not got:
                break
            data = mv[:got]
            ended = got < window + MAX_BLOCK
            code, tab, used, total = _lib.bgzf_scan(data)
            if ended and used < got and _cut_block(data[used:]):
                raise EOFError(f"BGZF block {nblocks + len(tab)} at offset {c_next + used}: the file ends inside the block")
            if code != _lib.OK or not tab:
                raise _scan_error(code if c_next + used == 0 else _lib.DATA_ERROR, nblocks + len(tab), c_next + used)
            t = np.array(tab, np.int64)
            coffs, csizes, isizes = t[:, 0], t[:, 2], t[:, 3]
            ustarts = np.cumsum(isizes) - isizes
            for k in range(len(tab)):                        # the gzi: every block once, in file order
                if not blocks or c_next + int(coffs[k]) > blocks[-1][0]:
                    blocks.append((c_next + int(coffs[k]), u_next + int(ustarts[k]), int(csizes[k]), int(isizes[k])))
            n_use, text_end, final = _grep_window(coffs + c_next, isizes, text_off, None, ended and used == got, text_cap)
            members, bad = _member_table(np.frombuffer(data, np.uint8), coffs[:n_use], csizes[:n_use], isizes[:n_use])
            if bad >= 0:
                raise BadGzipFile(f"BGZF block {nblocks + bad} at offset {c_next + int(coffs[bad])}: bad block header or block size")
            cend = int(coffs[n_use - 1] + csizes[n_use - 1]) if n_use else 0
            _, status, tot, rows, blob = ctx.bgzf_faidx(data[:cend], members, text_off, text_end, 10, _lib.BGZF_FAIDX_FINAL if final else 0,
                                                        line_base, carry)
            bad = np.nonzero(status)[0]
            if len(bad):
                raise _block_error(c_next + int(coffs[bad[0]]), status[bad[0]])
            if not tot.covered:
                raise BadGzipFile(f"BGZF blocks at offset {c_next}: the decoded blocks do not cover the text")
            out_offs, abs_c = members["out_off"].astype(np.int64), coffs[:n_use] + c_next

            def voffset(src):
                v, beyond = _tabix_voffsets([src], out_offs, isizes[:n_use], abs_c)
                return int(abs_c[-1] + csizes[n_use - 1]) << 16 if beyond[0] else int(v[0])
            if tot.bad_kind:
                if tot.bad_line >= line_base:
                    raise _FaidxBad(int(tot.bad_line), int(tot.bad_kind), voffset(int(tot.bad_src)))
                raise _FaidxBad(int(tot.bad_line), int(tot.bad_kind), last_v[0] if tot.bad_kind == 3 else last_v[1])
            if recs:                                         # the lines in front of the window's first header belong to the open sequence
                recs[-1][2] += int(tot.head_bases)
                if not recs[-1][5] and tot.head_line_width:
                    recs[-1][4], recs[-1][5] = int(tot.head_line_bases), int(tot.head_line_width)
            ends = np.cumsum(rows["name_len"].astype(np.int64))
            for r, e in zip(rows, ends.tolist()):
                recs.append([blob[e - int(r["name_len"]):e], int(r["line"]), int(r["bases"]), u_next + int(r["seq_src"]), int(r["line_bases"]),
                             int(r["line_width"])])
            carry = tot.carry
            if carry.flags & _lib.FAIDX_OPEN and carry.last_line >= line_base and n_use:
                nxt = text_off + int(carry.reserved)
                last_v = (voffset(nxt - int(carry.last_width)), voffset(nxt))
            line_base += tot.seen
            try:
                nxt = _grep_advance(isizes, n_use, text_off, text_end, int(tot.tail_off), final, window, _FAIDX_MAX_LINE)
            except _LongLine as e:
                v = make_virtual_offset(c_next + int(coffs[e.block]), e.offset)
                raise ValueError(f"the line at virtual offset {v} has not ended after {_FAIDX_MAX_LINE} bytes") from None
            if nxt is None:
                break
            b, text_off, window = nxt
            nblocks += b
            u_next += int(ustarts[b]) if b < len(coffs) else total
            c_next += int(coffs[b]) if b < len(coffs) else used
    finally:
        if buf is not None:
            del mv
            _lib.give_buffer(buf)
    if not final and carry is not None and carry.flags & _lib.FAIDX_OPEN and carry.first_width and carry.last_bases > carry.first_bases:
        raise _FaidxBad(int(carry.last_line), 3, last_v[0])  # (a file that ends exactly where a read ended: no call had _FINAL)
    seen = {}
    for name, line, *_ in recs:
        if name in seen:
            raise ValueError(f"the name {name!r} occurs twice: header lines {seen[name]} and {line}")
        seen[name] = line
    return FaidxIndex([(r[0], r[2], r[3], r[4], r[5]) for r in recs], GziIndex.from_blocks(blocks))


class SeqResult:
    """What fetch_seq() found: len() regions; offsets (int64, n + 1 of them) into data (the bases packed, without line terminators);
    result[i], slices and iteration yield bytes."""

    def __init__(self, offsets, data):
        self.offsets = np.asarray(offsets, np.int64)
        self.data = data

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        n = len(self)
        k = int(i)
        if not -n <= k < n:
            raise IndexError("SeqResult index out of range")
        k %= n
        return bytes(self.data[int(self.offsets[k]):int(self.offsets[k + 1])])

    def __iter__(self):
        return (self[k] for k in range(len(self)))

    def __repr__(self):
        return f"<SeqResult: {len(self)} regions, {int(self.offsets[-1])} bases>"


def _seq_regions(index, regions):
    """-> ([(row, beg, end)] clipped to the sequences, whether one region was given); KeyError for a name the index does not hold"""
    single = isinstance(regions, (str, bytes, tuple))
    out = []
    for r in ([regions] if single else list(regions)):
        if isinstance(r, tuple):
            open_end = len(r) == 3 and r[2] is None
            name, beg, end = parse_region((r[0], r[1], 0) if open_end else r)
        else:
            text = r.encode() if isinstance(r, str) else bytes(r)
            name, beg, end = parse_region(text)
            open_end = name == text or b"-" not in text.rpartition(b":")[2]
        row = index[name]
        end = row[0] if open_end else min(end, row[0])
        out.append((row, beg, end) if beg < end else (row, 0, 0))
    return out, single


def _seq_spans(regs, rc, text_cap=1 << 62):
    """Cut the regions into spans of at most FAIDX_MAX_SPAN bases and (with lines of that many bases at most) about text_cap bytes
    that begin at line starts behind a region's first.
    -> [(region, first byte, last byte, bases, col, line_bases, line_width, place in the region's output)] (pure host code)"""
    spans = []
    for i, ((length, offset, lb, lw), beg, end) in enumerate(regs):
        if end <= beg:
            continue
        if not lb:
            raise ValueError(_STALE_FAI)
        step = min(_lib.FAIDX_MAX_SPAN // lb, max(1, text_cap // lw)) * lb if lb <= _lib.FAIDX_MAX_SPAN else _lib.FAIDX_MAX_SPAN
        b0 = beg
        while b0 < end:
            b1 = min(end, (b0 // lb * lb if lb <= _lib.FAIDX_MAX_SPAN else b0) + step)
            first, last = offset + b0 // lb * lw + b0 % lb, offset + (b1 - 1) // lb * lw + (b1 - 1) % lb
            spans.append((i, first, last, b1 - b0, b0 % lb, lb, lw, end - b1 if rc else b0 - beg))
            b0 = b1
    return spans


def _fetch_seq_file(fp, fsize, ctx, index, regions, rc, load_block):
    if not isinstance(index, FaidxIndex):
        raise TypeError("fetch_seq() takes a FaidxIndex")
    regs, single = _seq_regions(index, regions)             # (KeyError before anything is read or decoded)
    offsets = np.zeros(len(regs) + 1, np.int64)
    np.cumsum([e - b for _, b, e in regs], out=offsets[1:])
    spans = _seq_spans(regs, rc, _GREP_TEXT)
    if not spans:
        return SeqResult(offsets, b"")
    gzi = index.gzi if index.gzi is not None else GziIndex.build(fp)
    gzi.validate(fsize)
    cs, us = [0] + [c for c, _ in gzi.entries], [0] + [u for _, u in gzi.entries]
    ctx = ctx or zlib_ng._ctx()
    cache, chains, ubase = {}, [], {}
    for _, first, last, *_ in spans:                         # byte spans -> blocks, through the gzi
        i0, i1 = bisect.bisect_right(us, first) - 1, bisect.bisect_right(us, last) - 1
        chain = cs[i0:i1 + 1]
        for k, c in enumerate(chain, i0):
            blk = load_block(c, cache) if c < fsize else None
            if blk is None or (k + 1 < len(us) and us[k + 1] - us[k] != blk[2]):
                raise ValueError(_STALE_FAI)
            ubase[c] = us[k]
        if last - us[i1] >= cache[chain[-1]][2]:
            raise ValueError(f"a region's bytes end at uncompressed offset {last}: does not fit the file's data")
        chains.append(chain)
    isize_of = {c: b[2] for c, b in cache.items() if b is not None}
    out = bytearray(int(offsets[-1]))
    for a, b in _fetch_groups(spans, chains, isize_of, _GREP_TEXT, 1 << 62):
        need = sorted({c for chain in chains[a:b] for c in chain})
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
        where = dict(zip(need, opos.tolist()))
        stab = np.zeros(b - a, _lib.FAIDX_SPAN_DTYPE)
        # a region's spans of this call lie together in the call's output, in the order of the region's output (reversed under
        # reverse_complement); runs that follow each other there and in the result are copied as one
        runs, k = [], a
        while k < b:
            e = k
            while e < b and spans[e][0] == spans[k][0]:
                e += 1
            lo = min(spans[j][7] for j in range(k, e))
            at = runs[-1][0] + runs[-1][2] if runs else 0
            g = int(offsets[spans[k][0]]) + lo
            for j in range(k, e):
                i, first, last, n, col, lb, lw, place = spans[j]
                stab[j - a] = (where[chains[j][0]] + first - ubase[chains[j][0]], at + place - lo, n, col, lb, lw, 1 if rc else 0, 0)
            n_run = sum(spans[j][3] for j in range(k, e))
            if runs and runs[-1][1] + runs[-1][2] == g:
                runs[-1][2] += n_run
            else:
                runs.append([at, g, n_run])
            k = e
        status, sstat, packed = ctx.bgzf_faidx_fetch(b"".join(raws), members, stab, runs[-1][0] + runs[-1][2])
        bad = np.nonzero(status)[0]
        if len(bad):
            raise _block_error(need[int(bad[0])], status[bad[0]])
        if bool(np.any(sstat)):
            raise ValueError(_STALE_FAI)
        pm = memoryview(packed)
        for at, g, n in runs:
            out[g:g + n] = pm[at:at + n]
    return SeqResult(offsets, bytes(out))


def fetch_seq(file, index, regions, *, reverse_complement=False):
    """The bases of `regions` of a bgzipped FASTA (a path or a seekable binary file): one region or a list of them, each a string as
    parse_region() reads it ("chr7:55,000,000-55,200,000", 1-based inclusive; without an end: to the sequence's end) or a tuple (name,
    beg, end), zero-based and half-open (end None: the sequence's end).  `index`: the file's FaidxIndex.  An end beyond the sequence is
    clipped, a start at or beyond it gives an empty result; a name the index does not hold is a KeyError, raised before anything is
    decoded.  The plan is made on the two indexes alone; every needed block is read and decoded once, the bases are gathered on the
    GPU without their line terminators (reverse_complement: reversed and complemented there, IUPAC codes in both cases), and only they
    come back: a SeqResult, in the order of the regions.  ValueError for an index that does not fit the file, BadGzipFile (with its
    offset) for a block that fails."""
    if _is_path(file):
        with _builtin_open(file, "rb") as f:
            return fetch_seq(f, index, regions, reverse_complement=reverse_complement)
    fsize = file.seek(0, 2)

    def load_block(c, cache):                                # (as BgzfReader._load_block)
        if c not in cache:
            file.seek(c)
            raw = file.read(MAX_BLOCK)
            code, tab, used, total = _lib.bgzf_scan(raw, 1) if raw else (_lib.OK, [], 0, 0)
            if raw and (code != _lib.OK or not tab):
                raise BadGzipFile(f"BGZF block at offset {c}: bad block header or block size")
            cache[c] = (raw[:used], 12 + struct.unpack_from("<H", raw, 10)[0], tab[0][3]) if raw else None
        return cache[c]
    return _fetch_seq_file(file, fsize, None, index, regions, bool(reverse_complement), load_block)


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

    def write_line_index(self, path_or_file, delimiter=b"\n"):
        """After close(), for a writer that was given a path: build the LineIndex of the finished file (LineIndex.build: the file is
        read back and counted on the GPU), save it and return it."""
        if not self._done or not self._own:
            raise ValueError("write_line_index() needs a closed writer that was opened on a path")
        idx = LineIndex.build(self._fp.name, delimiter)
        idx.save(path_or_file)
        return idx


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

    # ---- lines
    def _load_indexed(self, index, need):
        """the blocks `need` (ascending block numbers of `index`) read from the file, one read per run of adjacent ones -> (their
        bytes packed, member table); ValueError where the file does not hold what the index says"""
        c, csize = index._c[need], index._c[need + 1] - index._c[need]
        first = np.nonzero(np.append(True, need[1:] != need[:-1] + 1))[0]           # where a run starts
        last = np.append(first[1:], len(need)) - 1
        pieces = []
        for a, b in zip(first.tolist(), last.tolist()):
            self._fp.seek(int(c[a]))
            want = int(c[b] + csize[b] - c[a])
            piece = self._fp.read(want)
            if len(piece) != want:
                raise ValueError(_STALE)
            pieces.append(piece)
        data = pieces[0] if len(pieces) == 1 else b"".join(pieces)
        run_len = c[last] + csize[last] - c[first]
        run_at = np.cumsum(run_len) - run_len                                           # where each run lies in `data`
        run_of = np.cumsum(np.append(True, need[1:] != need[:-1] + 1)) - 1
        starts = run_at[run_of] + (c - c[first][run_of])
        members, bad = _member_table(np.frombuffer(data, np.uint8), starts, csize, index._isize[need])
        if bad >= 0:
            raise ValueError(_STALE)
        return data, members

    def _check_index(self, index):
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        if index.file_size != self._fsize:
            raise ValueError(_STALE)

    def read_lines(self, index, ranges):
        """[the lines first_line .. first_line + n_lines - 1 of (first_line, n_lines) for each range], lines counted from 0, each with
        its delimiter, as one bytes per range (short where the file ends, empty at or behind index.lines).  `index` is a LineIndex of
        this file.  The blocks are planned from the index alone, read with one file read per run of adjacent blocks and decoded once,
        in one launch; the select kernel finds where the lines start and end, and only the lines come back.  BadGzipFile if a block
        that a range touches does not check out; ValueError if the index does not match the file."""
        self._check_index(index)
        ranges = [(int(a), int(n)) for a, n in ranges]
        if any(a < 0 or n < 0 for a, n in ranges):
            raise ValueError("line numbers and counts must not be negative")
        out = [b""] * len(ranges)
        lo = np.fromiter((min(a, index.lines) for a, n in ranges), np.int64, len(ranges))
        hi = np.fromiter((min(a + n, index.lines) for a, n in ranges), np.int64, len(ranges))
        live = np.nonzero(hi > lo)[0]
        if not len(live):
            return out
        m0, r0 = index._locate_many(lo[live])
        m1, r1 = index._locate_many(hi[live], normalise=False)
        nb = len(index)
        cover = np.zeros(nb + 1, np.int64)                       # how many ranges reach over each block
        np.add.at(cover, m0, 1)
        np.add.at(cover, m1 + 1, -1)
        need = np.nonzero((np.cumsum(cover[:nb]) > 0) & (index._isize > 0))[0]
        here = self._fp.tell()
        try:
            data, members = self._load_indexed(index, need)
        finally:
            self._fp.seek(here)
        member_of = np.full(nb, -1, np.int64)
        member_of[need] = np.arange(len(need))
        table = np.column_stack([member_of[m0], r0, member_of[m1], r1]).astype(np.uint32)
        code, status, verdicts, lens, packed, _ = self._ctx.bgzf_read_lines(data, members, table, index.delimiter[0])
        for j in np.nonzero(verdicts)[0].tolist():
            if verdicts[j] == _lib.BGZF_SLICE_BLOCK:
                span = need[(need >= m0[j]) & (need <= m1[j])]
                bad = span[status[member_of[span]] != 0]
                if len(bad):
                    raise _block_error(int(index._c[bad[0]]), status[member_of[bad[0]]], f" (range {int(live[j])})")
            raise ValueError(_STALE)
        if code != _lib.OK:
            raise ValueError(_STALE)
        mv, at = memoryview(packed), 0
        for j, ln in zip(live.tolist(), lens.tolist()):
            out[j] = bytes(mv[at:at + ln])
            at += ln
        return out

    def grep(self, patterns, *, delimiter=b"\n", invert=False, line_start=False, count=False, max_count=None, start=None, stop=None,
             first_line=0, max_line=64 << 20, mismatches=0):
        """bgzf.grep() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("grep() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _grep_file(self._fp, self._ctx, patterns, delimiter, invert, line_start, count, max_count, start, stop, first_line,
                              max_line, None, mismatches)
        finally:
            self._fp.seek(at)

    def grep_records(self, patterns, record_lines, *, match_line=None, first_byte=None, delimiter=b"\n", invert=False, line_start=False,
                     count=False, max_count=None, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False,
                     mismatches=0):
        """bgzf.grep_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("grep_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _grep_file(self._fp, self._ctx, patterns, delimiter, invert, line_start, count, max_count, start, stop, first_record,
                              max_record, (record_lines, match_line, first_byte, allow_short), mismatches)
        finally:
            self._fp.seek(at)

    def classify_records(self, patterns, record_lines, *, match_line=None, first_byte=None, delimiter=b"\n", line_start=False, start=None,
                         stop=None, first_record=0, max_record=64 << 20, allow_short=False, mismatches=0):
        """bgzf.classify_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("classify_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _classify_file(self._fp, self._ctx, patterns, record_lines, match_line, first_byte, delimiter, line_start, start, stop,
                                  first_record, max_record, allow_short, mismatches, None)
        finally:
            self._fp.seek(at)

    def demux(self, patterns, outputs, record_lines=4, *, ambiguous=None, unassigned=None, compresslevel=6, block_size=MAX_BLOCK_INPUT,
              match_line=None, first_byte=None, delimiter=b"\n", line_start=False, start=None, stop=None, first_record=0, max_record=64 << 20,
              allow_short=False, mismatches=0):
        """bgzf.demux() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("demux() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _demux_file(self._fp, self._ctx, patterns, outputs, record_lines, ambiguous, unassigned, compresslevel, block_size, match_line,
                               first_byte, delimiter, line_start, start, stop, first_record, max_record, allow_short, mismatches)
        finally:
            self._fp.seek(at)

    def partition_records(self, labels, outputs, record_lines=4, *, first_byte=None, delimiter=b"\n", compresslevel=6, block_size=MAX_BLOCK_INPUT,
                          start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.partition_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("partition_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _partition_file(self._fp, self._ctx, labels, outputs, record_lines, first_byte, delimiter, compresslevel, block_size, start, stop,
                                   first_record, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def trim_records(self, output, record_lines=4, *, seq_line=1, qual_line=3, cut=(0, 0), quality=(0, 0), quality_base=33, adapters=(), mismatches=0,
                     min_overlap=3, min_length=0, too_short=None, drop=None, first_byte=None, delimiter=b"\n", compresslevel=6,
                     block_size=MAX_BLOCK_INPUT, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.trim_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("trim_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _trim_file(self._fp, self._ctx, output, too_short, record_lines, seq_line, qual_line, cut, quality, quality_base, adapters, mismatches,
                              min_overlap, min_length, drop, first_byte, delimiter, compresslevel, block_size, start, stop, first_record, max_record,
                              allow_short)
        finally:
            self._fp.seek(at)

    def overlap_records(self, merged=None, unmerged=None, record_lines=8, *, seq_line=1, qual_line=3, quality_base=33, min_overlap=30, mismatches=5,
                        mismatch_percent=20, merge=True, correct=False, correct_quality=(30, 14), cut_adapters=False, first_byte=None, delimiter=b"\n",
                        compresslevel=6, block_size=MAX_BLOCK_INPUT, start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.overlap_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("overlap_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _overlap_file(self._fp, self._ctx, merged, unmerged, record_lines, seq_line, qual_line, quality_base, min_overlap, mismatches,
                                 mismatch_percent, merge, correct, correct_quality, cut_adapters, first_byte, delimiter, compresslevel, block_size,
                                 start, stop, first_record, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def qc_records(self, record_lines=4, *, seq_line=1, qual_line=3, quality_base=33, cycles=512, low_quality=15, per_record=False, first_byte=None,
                   delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.qc_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("qc_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _qc_file(self._fp, self._ctx, record_lines, seq_line, qual_line, quality_base, cycles, low_quality, per_record, first_byte, delimiter,
                            start, stop, first_record, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def key_records(self, record_lines=4, *, seq_line=1, first=0, length=0, ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n",
                    start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.key_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("key_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _key_file(self._fp, self._ctx, record_lines, seq_line, first, length, ignore_case, canonical, first_byte, delimiter, start, stop,
                             first_record, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def dedup_records(self, output, record_lines=4, *, duplicates=None, compresslevel=6, block_size=MAX_BLOCK_INPUT, seq_line=1, first=0, length=0,
                      ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0,
                      max_record=64 << 20, allow_short=False):
        """bgzf.dedup_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("dedup_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _dedup_file(self._fp, self._ctx, output, duplicates, record_lines, compresslevel, block_size, seq_line, first, length, ignore_case,
                               canonical, first_byte, delimiter, start, stop, first_record, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def screen_records(self, kset, record_lines=4, *, seq_line=1, min_hits=1, first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0,
                       max_record=64 << 20, allow_short=False):
        """bgzf.screen_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("screen_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _screen_file(self._fp, self._ctx, kset, record_lines, seq_line, min_hits, first_byte, delimiter, start, stop, first_record, max_record,
                                allow_short)
        finally:
            self._fp.seek(at)

    def screen_filter(self, kset, output, matched=None, record_lines=4, *, seq_line=1, min_hits=1, compresslevel=6, block_size=MAX_BLOCK_INPUT,
                      first_byte=None, delimiter=b"\n", start=None, stop=None, first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.screen_filter() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("screen_filter() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _screen_filter_file(self._fp, self._ctx, kset, output, matched, record_lines, compresslevel, block_size, seq_line, min_hits, first_byte,
                                       delimiter, start, stop, first_record, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def sort_key_records(self, key, record_lines=4, *, meta=None, truncate=False, first_byte=None, delimiter=b"\n", start=None, stop=None,
                         first_record=0, max_record=64 << 20, allow_short=False):
        """bgzf.sort_key_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("sort_key_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _sort_key_file(self._fp, self._ctx, key, record_lines, meta, truncate, False, first_byte, delimiter, start, stop, first_record,
                                  max_record, allow_short)
        finally:
            self._fp.seek(at)

    def sort_keys(self, keys, *, rank=False):
        """bgzf.sort_keys() on this reader's context"""
        return _sort(self._ctx, keys, rank)

    def permute_records(self, order, output, record_lines=4, *, lengths=None, chunk_bytes=1 << 30, compresslevel=6, block_size=MAX_BLOCK_INPUT,
                        first_byte=None, delimiter=b"\n"):
        """bgzf.permute_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("permute_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _permute_file(self._fp, self._ctx, order, output, record_lines, lengths, chunk_bytes, compresslevel, block_size, first_byte, delimiter)
        finally:
            self._fp.seek(at)

    def sort_records(self, output, key, record_lines=4, *, reverse=False, meta=None, truncate=False, chunk_bytes=1 << 30, compresslevel=6,
                     block_size=MAX_BLOCK_INPUT, first_byte=None, delimiter=b"\n", max_record=64 << 20, allow_short=False):
        """bgzf.sort_records() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("sort_records() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _sort_file(self._fp, self._ctx, output, key, record_lines, reverse, meta, truncate, chunk_bytes, compresslevel, block_size, first_byte,
                              delimiter, max_record, allow_short)
        finally:
            self._fp.seek(at)

    def demux_paired(self, mates, patterns, outputs, record_lines=4, *, barcode_file=0, ambiguous=None, unassigned=None, compresslevel=6,
                     block_size=MAX_BLOCK_INPUT, match_line=None, first_byte=None, delimiter=b"\n", line_start=False, start=None, stop=None,
                     first_record=0, max_record=64 << 20, allow_short=False, mismatches=0):
        """bgzf.demux_paired() with this reader's file as files[0] and mates (paths or seekable binary files) behind it; the read position
        stays where it was"""
        if self.closed:
            raise ValueError("demux_paired() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            mates = [mates] if _is_path(mates) or hasattr(mates, "read") else list(mates)
            return _demux_paired_files([(self._fp, self._ctx)] + [(f, self._ctx) for f in mates], patterns, outputs, record_lines, barcode_file,
                                       ambiguous, unassigned, compresslevel, block_size, match_line, first_byte, delimiter, line_start, start, stop,
                                       first_record, max_record, allow_short, mismatches)
        finally:
            self._fp.seek(at)

    def fetch(self, index, regions, *, count=False):
        """bgzf.fetch() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("fetch() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _fetch_file(self._fp, self._fsize, self._ctx, index, regions, count, self._load_block)
        finally:
            self._fp.seek(at)

    def fetch_seq(self, index, regions, *, reverse_complement=False):
        """bgzf.fetch_seq() on this reader's file; the read position stays where it was"""
        if self.closed:
            raise ValueError("fetch_seq() on closed BgzfReader object")
        if not self.seekable():
            raise io.UnsupportedOperation("the underlying file cannot seek")
        at = self._fp.tell()
        try:
            return _fetch_seq_file(self._fp, self._fsize, self._ctx, index, regions, bool(reverse_complement), self._load_block)
        finally:
            self._fp.seek(at)

    def line_voffsets(self, index, lines):
        """[the virtual offset at which each of `lines` starts] -- what seek() takes.  Normalised: the offset inside the block is below
        the block's ISIZE; the end of the data (line == index.lines) is the offset of the first byte behind the indexed blocks.
        Lines that start where a block starts cost nothing; the others are found by the select kernel in one launch."""
        self._check_index(index)
        lines = [int(x) for x in lines]
        b, r = index._locate_many(lines)
        within = np.zeros(len(b), np.int64)
        ask = np.nonzero(r > 0)[0]
        if len(ask):
            need = np.unique(b[ask])
            here = self._fp.tell()
            try:
                data, members = self._load_indexed(index, need)
            finally:
                self._fp.seek(here)
            member_of = np.full(len(index), -1, np.int64)
            member_of[need] = np.arange(len(need))
            q = np.column_stack([member_of[b[ask]], r[ask]]).astype(np.uint32)
            status, pos, verdicts = self._ctx.bgzf_line_positions(data, members, q, index.delimiter[0])
            for j in np.nonzero(verdicts)[0].tolist():
                blk = int(b[ask[j]])
                if verdicts[j] == _lib.BGZF_SLICE_BLOCK:
                    raise _block_error(int(index._c[blk]), status[member_of[blk]], f" (line {lines[int(ask[j])]})")
                raise ValueError(_STALE)
            within[ask] = pos.astype(np.int64) - members["out_off"][q[:, 0]].astype(np.int64)
            if bool((within[ask] >= index._isize[b[ask]]).any()):
                raise ValueError(_STALE)
        return [make_virtual_offset(int(c), int(w)) for c, w in zip(index._c[b].tolist(), within.tolist())]

"""The referee of the faidx tests: the line model of a FASTA ("BGZF by sequence") in plain Python, on the decoded
text of a file.  It never calls the code under test."""

COMPLEMENT = bytes.maketrans(b"ATUCGRYKMBVDHatucgrykmbvdh", b"TAAGCYRMKVBHDtaagcyrmkvbhd")
KINDS = (1, 2, 3, 4, 5)


def lines_of(text):
    """-> [(start, bases, width, body)]: the text cut by LF; one CR in front of the LF belongs to the terminator; non-empty bytes
    behind the last LF are a line whose width equals its bases"""
    out, at = [], 0
    while at < len(text):
        e = text.find(b"\n", at)
        if e < 0:
            out.append((at, len(text) - at, len(text) - at, text[at:]))
            break
        body = text[at:e]
        if body.endswith(b"\r"):
            body = body[:-1]
        out.append((at, len(body), e + 1 - at, body))
        at = e + 1
    return out


def name_of(body):
    """the name of a header line: from the byte behind '>' to the first space, tab or CR or to the end of the body"""
    name = body[1:]
    for sep in (b" ", b"\t", b"\r"):
        name = name.split(sep)[0]
    return name


def table(text):
    """-> (records [[name, header line, LENGTH, OFFSET, LINEBASES, LINEWIDTH]], faults [(line, kind)], every fault of the text)"""
    lines = lines_of(text)
    recs, faults, cur = [], [], None                         # cur: the sequence lines of the open sequence [(number, bases, width)]

    def close():
        full = [x for x in cur if x[1]]
        if not full:
            return
        first, last = full[0], full[-1]
        for no, bases, width in full[:-1]:
            if bases != first[1] or width != first[2]:
                faults.append((no, 3))
        if last[1] > first[1]:
            faults.append((last[0], 3))
        faults.extend((no, 4) for no, bases, _ in cur if not bases and no < last[0])

    for no, (start, bases, width, body) in enumerate(lines):
        if body[:1] == b">":
            if cur is not None:
                close()
            name = name_of(body)
            if not name:
                faults.append((no, 1))
            recs.append([name, no, 0, start + width, 0, 0])
            cur = []
            continue
        if any(not 0x21 <= c <= 0x7E for c in body):
            faults.append((no, 2))
        if cur is None:
            if bases:
                faults.append((no, 5))
            continue
        cur.append((no, bases, width))
        recs[-1][2] += bases
        if bases and not recs[-1][5]:
            recs[-1][4], recs[-1][5] = bases, width
    if cur is not None:
        close()
    return recs, sorted(faults)


def index(text):
    """-> ("ok", [(name, LENGTH, OFFSET, LINEBASES, LINEWIDTH)]), ("bad", line, kind) for the smallest bad line (of one line's
    faults the smallest kind), or ("dup", name, first header line, second header line)"""
    recs, faults = table(text)
    if faults:
        return ("bad",) + faults[0]
    seen = {}
    for name, no, *_ in recs:
        if name in seen:
            return "dup", name, seen[name], no
        seen[name] = no
    return "ok", [(r[0], r[2], r[3], r[4], r[5]) for r in recs]


def line_start(text, no):
    return lines_of(text)[no][0]


def subseq(text, row, beg, end, rc=False):
    """bases [beg, end) of the sequence with the .fai row (LENGTH, OFFSET, LINEBASES, LINEWIDTH), by plain slicing"""
    length, offset, lb, lw = row
    if not lb:
        return b""
    nlines = (length + lb - 1) // lb
    seq = text[offset:offset + nlines * lw].replace(b"\n", b"").replace(b"\r", b"")[:length]
    part = seq[beg:min(end, length)] if beg < length else b""
    return part.translate(COMPLEMENT)[::-1] if rc else part

"""The referee of the contaminant screen, in plain Python from the statement of the rule in include/zng_amd.h:
a dict from code to mask, and a loop over positions.  It never uses the code under test."""
import collections

NONE = 0xFFFFFFFF
BASE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("U"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3, ord("u"): 3}

Row = collections.namedtuple("Row", "refs kmers hits best best_hits")
Totals = collections.namedtuple("Totals", "seen bytes_in bases kmers hits matched")


def code_at(seq, p, k, canonical):
    """the code of the k-mer seq[p : p + k], None when it holds an invalid byte"""
    fwd = rev = 0
    for i in range(k):
        b = BASE.get(seq[p + i])
        if b is None:
            return None
        fwd = fwd << 2 | b                                   # the first base is the most significant
        rev |= (3 - b) << (2 * i)                            # the complement of the first base is the last of the reverse complement
    return min(fwd, rev) if canonical else fwd


def codes_of(seq, k, canonical):
    """-> the code (or None) of every position 0 .. n - k"""
    return [code_at(seq, p, k, canonical) for p in range(len(seq) - k + 1)]


def build(references, k, canonical):
    """-> ({code: mask}, positions, valid)"""
    table, positions, valid = {}, 0, 0
    for j, ref in enumerate(references):
        for c in codes_of(ref, k, canonical):
            positions += 1
            if c is not None:
                valid += 1
                table[c] = table.get(c, 0) | 1 << j
    return table, positions, valid


def pairs(table):
    """the set's (code, mask) pairs, sorted"""
    return sorted(table.items())


def cap_of(n):
    """the smallest power of two that is >= 2 n and >= 64"""
    cap = 64
    while cap < 2 * n:
        cap *= 2
    return cap


def screen(seq, table, k, canonical):
    """-> the Row of one sequence"""
    kmers = hits = refs = 0
    count = [0] * 64
    for c in codes_of(seq, k, canonical):
        if c is None:
            continue
        kmers += 1
        m = table.get(c, 0)
        if m:
            hits += 1
            refs |= m
            for j in range(64):
                if m >> j & 1:
                    count[j] += 1
    if not hits:
        return Row(0, kmers, 0, NONE, 0)
    best = max(range(64), key=lambda j: (count[j], -j))     # the most hit positions, the lowest number among equals
    return Row(refs, kmers, hits, best, count[best])


def records_of(text, record_lines=4, delimiter=b"\n", final=True):
    """-> (the records of the text as lists of line bodies, the bytes they take): every line but an open last one ends with the delimiter;
    without `final` the open record behind the last whole one is left out"""
    lines = text.split(delimiter)
    open_last = lines.pop()                                  # what follows the last delimiter
    if final and open_last:
        lines.append(open_last)                              # (with `final` it is a line, and a short last record is a record)
    n = len(lines) if final else len(lines) // record_lines * record_lines
    recs = [lines[i:i + record_lines] for i in range(0, n, record_lines)]
    return recs, len(text) if final else sum(len(x) + 1 for r in recs for x in r)


def screen_text(text, table, k, canonical, min_hits=1, record_lines=4, seq_line=1, delimiter=b"\n", final=True):
    """-> (rows, Totals) of a text"""
    recs, nbytes = records_of(text, record_lines, delimiter, final)
    bodies = [r[seq_line] if seq_line < len(r) else b"" for r in recs]
    rows = [screen(b, table, k, canonical) for b in bodies]
    return rows, Totals(len(rows), nbytes, sum(map(len, bodies)), sum(r.kmers for r in rows), sum(r.hits for r in rows),
                        sum(1 for r in rows if r.hits >= min_hits))

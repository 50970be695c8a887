"""The referee of the k-mer count, in plain Python from the statement of the rule in include/zng_amd.h: a dict
from code to count, a loop over positions, the runs of a record in strips of 64 from position 0, the spectrum, and the table's size.
It never uses the code under test."""
import collections

BASE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("U"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3, ord("u"): 3}

Totals = collections.namedtuple("Totals", "seen bytes_in bases kmers claimed adds")


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
    """-> the code (or None) of every position 0 .. n - k: code_at() of every position, computed by sliding (the forward code gains a
    base at its low end and loses its top one, the reverse complement's gains at its top; `good` counts the valid bytes in a row).
    test_cpu_bgzf_kcount.py holds the two against each other."""
    out, fwd, rev, good, top, keep = [], 0, 0, 0, 2 * (k - 1), (1 << 2 * k) - 1
    for i, byte in enumerate(seq):
        b = BASE.get(byte)
        if b is None:
            fwd = rev = good = 0
        else:
            fwd, rev, good = (fwd << 2 | b) & keep, rev >> 2 | (3 - b) << top, good + 1
        if i >= k - 1:
            out.append(None if good < k else min(fwd, rev) if canonical else fwd)
    return out


def runs_of(codes):
    """the runs of one record: its positions in strips of 64 from position 0; within a strip a valid position begins a run when the
    position before it in the strip is invalid or holds another code, and the first position of a strip has none before it"""
    runs = 0
    for p, c in enumerate(codes):
        if c is not None and (p % 64 == 0 or codes[p - 1] != c):
            runs += 1
    return runs


def add_seq(table, seq, k, canonical):
    """seq counted into table ({code: count}) -> (valid positions, runs)"""
    codes = codes_of(seq, k, canonical)
    valid = 0
    for c in codes:
        if c is not None:
            valid += 1
            table[c] = table.get(c, 0) + 1
    return valid, runs_of(codes)


def pairs(table, min_count=1, max_count=0):
    """the (code, count) pairs with min_count <= count <= max_count (0: no upper bound), sorted"""
    return sorted((c, n) for c, n in table.items() if n >= min_count and (not max_count or n <= max_count))


def spectrum(table, bins):
    """[0] = 0; [c] the codes with count c for c < bins - 1; [bins - 1] the codes with count >= bins - 1"""
    hist = [0] * bins
    for n in table.values():
        hist[min(n, bins - 1)] += 1
    return hist


def cap_of(room):
    """a new counter's slots: the smallest power of two that is >= max(64, 2 room)"""
    cap = 64
    while cap < 2 * room:
        cap *= 2
    return cap


def reserve(cap, distinct, room):
    """the slots after reserve(room): unchanged when distinct + room <= cap / 2, else the smallest power of two >= 4 (distinct + room)"""
    if distinct + room <= cap // 2:
        return cap
    new = 64
    while new < 4 * (distinct + room):
        new *= 2
    return new


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


def count_bodies(bodies, k, canonical, table=None):
    """-> (table, kmers, adds, claimed) of the sequences counted into table (a new one unless given)"""
    table = {} if table is None else table
    before = len(table)
    kmers = adds = 0
    for b in bodies:
        v, r = add_seq(table, b, k, canonical)
        kmers, adds = kmers + v, adds + r
    return table, kmers, adds, len(table) - before


def count_text(text, k, canonical, record_lines=4, seq_line=1, delimiter=b"\n", final=True, table=None):
    """-> (table, Totals) of a text counted into table (a new one unless given)"""
    recs, nbytes = records_of(text, record_lines, delimiter, final)
    bodies = [r[seq_line] if seq_line < len(r) else b"" for r in recs]
    table, kmers, adds, claimed = count_bodies(bodies, k, canonical, table)
    return table, Totals(len(recs), nbytes, sum(map(len, bodies)), kmers, claimed, adds)

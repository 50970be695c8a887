"""The referee of the partition tests: plain Python on plain bytes, never the code under test.  A text is cut into records of k lines
(the lines left over at the end are a short last record, allow_short's rule), the records are grouped by a label each, and a label of
DROP (-1) puts a record nowhere."""
DROP = -1


def lines_of(text, delim=b"\n"):
    """the lines of text with their delimiters; a non-empty remainder is the last line"""
    parts = text.split(delim)
    return [p + delim for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def records_of(text, k, delim=b"\n"):
    """-> (records, short_lines): the text cut every k lines; short_lines: the lines of a short last record, 0 when it is whole"""
    lines = lines_of(text, delim)
    return [b"".join(lines[i:i + k]) for i in range(0, len(lines), k)], len(lines) % k


class Partition:
    """records (list of bytes), labels (list of int, one per record), n_classes; counts (records per class), dropped, dropped_bytes"""

    def __init__(self, text, labels, n_classes, k=4, delim=b"\n"):
        self.records, self.short_lines = records_of(text, k, delim)
        self.labels, self.n_classes = [int(x) for x in labels], n_classes
        if len(self.labels) != len(self.records):
            raise ValueError("%d records, %d labels" % (len(self.records), len(self.labels)))
        if any(not (x == DROP or 0 <= x < n_classes) for x in self.labels):
            raise ValueError("a label out of range")
        self.counts = [sum(1 for x in self.labels if x == c) for c in range(n_classes)]
        self.dropped = sum(1 for x in self.labels if x == DROP)
        self.dropped_bytes = sum(len(r) for r, x in zip(self.records, self.labels) if x == DROP)

    def members(self, c):
        """the numbers of class c's records, ascending"""
        return [r for r, x in enumerate(self.labels) if x == c]

    def of_class(self, c):
        """the bytes of class c's records, in input order"""
        return b"".join(self.records[r] for r in self.members(c))

    def order(self):
        """the kept records' numbers by class, then by number: the order of the rows"""
        return [r for c in range(self.n_classes) for r in self.members(c)]

"""The referee of the classify tests: numpy on plain bytes, never the code under test.  For each pattern the mismatches of every window
are summed byte by byte (as hit_lines of test_gpu_bgzf_grep_approx.py sums them: eight bytes at a time, windows that are past k left
out of what follows), windows that hold a delimiter are dropped by a prefix sum of the delimiters, with line_start a window starts at a
line's first byte; np.minimum.at keeps the smallest count per line, the minimum over the lines of a record that count gives d_i(r), and
the assignment rule of include/zng_amd.h is applied to the d_i."""
import numpy as np

UNASSIGNED, AMBIGUOUS, NONE = -1, -2, 255


def lines_of(text, delim):
    """the lines of text with their delimiters; a non-empty remainder is the last line"""
    parts = text.split(delim)
    return [p + delim for p in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


def line_distances(text, delim, pats, k, line_start=False, both=False):
    """-> uint8[n_patterns, n_lines]: the smallest distance <= k of a window of pattern i in line q, NONE where there is none; both: the
    pair of arrays without and with line_start, from one pass over the windows"""
    arr = np.frombuffer(text, np.uint8)
    n = len(arr)
    isd = arr == delim[0]
    before = np.concatenate([[0], np.cumsum(isd, dtype=np.int64)])           # before[i]: delimiters in text[:i] = the line of byte i
    nlines = int(before[-1]) + (1 if n and not isd[-1] else 0)
    anywhere, at_start = np.full((len(pats), nlines), NONE, np.uint8), np.full((len(pats), nlines), NONE, np.uint8)
    for i, p in enumerate(pats):
        L = len(p)
        if L > n:
            continue
        pos, cnt = None, np.zeros(n - L + 1, np.uint16)                      # pos None: every window is still in
        for j0 in range(0, L, 8):
            for j in range(j0, min(j0 + 8, L)):
                cnt += (arr[j:n - L + 1 + j] if pos is None else arr[pos + j]) != p[j]
            keep = np.nonzero(cnt <= k)[0]
            if pos is not None or len(keep) < len(cnt):
                pos, cnt = (keep if pos is None else pos[keep]), cnt[keep]
        if pos is None:
            pos = np.arange(n - L + 1)
        ok = before[pos + L] == before[pos]                                  # no delimiter inside the window
        pos, cnt = pos[ok], cnt[ok].astype(np.uint8)
        np.minimum.at(anywhere[i], before[pos], cnt)
        first = (pos == 0) | isd[np.maximum(pos, 1) - 1]                     # the first byte of a line
        np.minimum.at(at_start[i], before[pos[first]], cnt[first])
    return (anywhere, at_start) if both else at_start if line_start else anywhere


class Verdict:
    """pattern (int16), distance (uint8), tie (int16, (n, 2)), counts (int64, n_patterns + 2), records (list of bytes), cls (the class
    of every record)"""

    def __init__(self, pattern, distance, tie, counts, records, cls):
        self.pattern, self.distance, self.tie, self.counts, self.records, self.cls = pattern, distance, tie, counts, records, cls

    def of_class(self, c):
        """the bytes of class c's records, in input order"""
        return b"".join(self.records[r] for r in np.nonzero(self.cls == c)[0].tolist())


def classify(text, delim, pats, k, record_lines, match_line=None, line_start=False, d=None):
    """the rule on text whose first byte starts a record; lines left over at the end are a short last record.  d: what line_distances
    gave for these arguments, computed once for several record models"""
    lines = lines_of(text, delim)
    nrec = (len(lines) + record_lines - 1) // record_lines
    records = [b"".join(lines[record_lines * r:record_lines * r + record_lines]) for r in range(nrec)]
    d = line_distances(text, delim, pats, k, line_start) if d is None else d
    pad = np.full((len(pats), nrec * record_lines), NONE, np.uint8)
    pad[:, :len(lines)] = d
    pad = pad.reshape(len(pats), nrec, record_lines)
    per = pad[:, :, match_line] if match_line is not None else pad.min(axis=2)      # d_i(r)
    best = per.min(axis=0) if nrec else np.empty(0, np.uint8)
    reach = (per == best[None, :]) & (best[None, :] != NONE)
    n_reach = reach.sum(axis=0)
    lowest = reach.argmax(axis=0).astype(np.int16)
    highest = (len(pats) - 1 - reach[::-1].argmax(axis=0)).astype(np.int16)
    pattern = np.where(n_reach == 0, UNASSIGNED, np.where(n_reach == 1, lowest, AMBIGUOUS)).astype(np.int16)
    tie = np.stack([lowest, highest], 1).astype(np.int16)
    tie[n_reach == 0] = -1
    cls = np.where(pattern >= 0, pattern, np.where(pattern == AMBIGUOUS, len(pats), len(pats) + 1)).astype(np.int64)
    counts = np.bincount(cls, minlength=len(pats) + 2).astype(np.int64)
    return Verdict(pattern, best.astype(np.uint8), tie, counts, records, cls)

"""The referee of key_records and dedup_keys: the key function of include/zng_amd.h in numpy, straight from its
statement; the resolve as a dict walk; and `exact`, which compares the bytes themselves and hashes nothing.  Never the code under
test.  The records are split as trim_ref splits them."""
from collections import namedtuple

import numpy as np

from trim_ref import Fault, split_records

S = (0x243F6A8885A308D3, 0x13198A2E03707344)
M = (1 << 64) - 1

Conf = namedtuple("Conf", "record_lines seq_line first length ignore_case canonical first_byte delimiter")


def conf(record_lines=4, seq_line=1, first=0, length=0, ignore_case=False, canonical=False, first_byte=None, delimiter=b"\n"):
    return Conf(record_lines, seq_line, first, length, ignore_case, canonical, first_byte, bytes(delimiter))


def mix(x):
    """the splitmix64 step on a uint64 array (or a Python int)"""
    if isinstance(x, int):
        return int(mix(np.array([x & M], np.uint64))[0])
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


COMP = bytes.maketrans(b"ATCGatcgUu", b"TAGCtagcAa")


def part(body, cf):
    """the keyed part of a body, the case folded when cf says so"""
    p = body[cf.first:cf.first + cf.length] if cf.length else body[cf.first:]
    return p.translate(bytes.maketrans(bytes(range(97, 123)), bytes(range(65, 91)))) if cf.ignore_case else p


def words(p):
    """(word_0, word_1) of the bytes p"""
    c = np.frombuffer(p, np.uint8).astype(np.uint64)
    i = np.arange(len(p), dtype=np.uint64)
    return tuple((mix(s ^ (1 << 63 | len(p))) + int(mix(np.uint64(s) ^ (i << np.uint64(8) | c)).sum(dtype=np.uint64))) & M for s in S)


def key(body, cf):
    """-> (lo, hi)"""
    p = part(body, cf)
    k = words(p)
    if cf.canonical:
        r = words(p.translate(COMP)[::-1])
        if (r[1], r[0]) < (k[1], k[0]):
            k = r
    return k


def bodies_of(text, cf, final=True):
    """-> (the seq_line bodies of the records, bytes of the records, consumed); Fault(1, record) for a first byte that is not first_byte"""
    recs, _, consumed = split_records(text, cf.record_lines, cf.delimiter, final)
    out = []
    for r, rec in enumerate(recs):
        if cf.first_byte is not None and not (rec[0][0] + (cf.delimiter if rec[0][1] else b"")).startswith(bytes(cf.first_byte)):
            raise Fault(1, r)
        out.append(rec[cf.seq_line][0] if cf.seq_line < len(rec) else b"")
    return out, sum(len(b) + d for rec in recs for b, d in rec), consumed


def keys(bodies, cf):
    """-> uint64[n, 2]: lo, hi"""
    return np.array([key(b, cf) for b in bodies], np.uint64).reshape(-1, 2)


Resolved = namedtuple("Resolved", "first count unique duplicates max_count max_first")


def walk(items):
    """first, count and the totals of any hashable items, by a dict"""
    seen, first, count = {}, [], []
    for r, k in enumerate(items):
        f = seen.setdefault(k, r)
        first.append(f)
        count.append(0)
        count[f] += 1
    mc = max(count, default=0)
    return Resolved(first, count, len(seen), len(items) - len(seen), mc, count.index(mc) if items else 0)


def resolve(k):
    """a dict walk over keys (uint64[n, 2] or a list of (lo, hi))"""
    return walk([(int(lo), int(hi)) for lo, hi in k])


def exact(bodies, cf):
    """first and count by comparing the bytes: the part, case folded, and with canonical the smaller of it and its reverse complement.
    With canonical that is the keys' grouping where the complement is an involution on the parts, which is everywhere but at U and u
    (U -> A -> T): ValueError for a part that holds one; no_collision() judges such inputs."""
    def norm(b):
        p = part(b, cf)
        if cf.canonical and (b"U" in p or b"u" in p):
            raise ValueError("exact: the reverse complement of a part with U or u does not lead back to it")
        return min(p, p.translate(COMP)[::-1]) if cf.canonical else p
    return walk([norm(b) for b in bodies])


def no_collision(bodies, k, cf):
    """What can be said by bytes alone of canonical keys k (uint64[n, 2]) over parts that may hold U or u, where a part p stands for the
    set {p, rc(p)} and which of the two has the smaller key is the mixer's affair: records with equal keys have sets that share a
    sequence (no collision), and records with equal sets have equal keys (nothing is told apart that is the same).  -> True, or an
    AssertionError that names the two records."""
    sets = [frozenset((p, p.translate(COMP)[::-1]) if cf.canonical else (p,)) for p in (part(b, cf) for b in bodies)]
    by_key, by_set = {}, {}
    for r, (kk, s) in enumerate(zip(map(tuple, k.tolist()), sets)):
        q = by_key.setdefault(kk, r)
        assert sets[q] & s, ("two sequences share a key", q, r)
        q = by_set.setdefault(s, r)
        assert tuple(k[q].tolist()) == kk, ("one sequence has two keys", q, r)
    return True


def pair(a, b):
    """the keys of pairs: uint64[n, 2] each"""
    out = np.empty_like(a)
    for w in range(2):
        h = mix(np.uint64(S[w]) ^ a[:, 0])
        for x in (a[:, 1], b[:, 0], b[:, 1]):
            h = mix(h ^ x)
        out[:, w] = h
    return out

"""Inputs of the screen tests (test_cpu_bgzf_screen.py, test_gpu_bgzf_screen.py): references and reads, made from fixed seeds."""
import functools

import numpy as np

LETTERS = b"ACGT"
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
BUILD_K = (1, 2, 15, 16, 17, 31)
BUILD_R = (1, 2, 64)
SCREEN_RULES = ((21, True), (31, False))                     # (k, canonical) of the screen tests
SCREEN_R = 64
COMMON = 90                                                  # bases that all 64 screen references share
LONG = 3000                                                  # the one long read


def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(LETTERS, np.uint8), size=n).tolist())


def rc(seq):
    return seq.translate(COMP)[::-1]


def fastq(bodies, tag=b"r"):
    return [b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"F" * len(s)) for i, s in enumerate(bodies)]


def spoil(seq, places, byte=b"N"):
    """seq with `byte` at every place that it has"""
    s = bytearray(seq)
    for p in places:
        if 0 <= p < len(s):
            s[p:p + 1] = byte
    return bytes(s)


@functools.lru_cache(maxsize=None)
def build_references(k, n_refs):
    """references of the lengths 0, k - 1, k, k + 1, 63 + k, 64 + k and about 5 000 (once; about 300 afterwards), in turn; invalid bytes
    at the positions 0, 63, 64 and last; lower case and U; one reference is the reverse complement of another"""
    rng = np.random.default_rng(1000 * k + n_refs)
    lengths = [64 + k, 0, k - 1, k, k + 1, 63 + k, 5003]
    refs = []
    for j in range(n_refs):
        n = lengths[j % len(lengths)]
        if n > 5000 and j >= len(lengths):
            n = 301
        s = rand_seq(rng, n)
        if j % 3 == 0:
            s = spoil(s, (0, 63, 64, n - 1), (b"N", b"-", b"n", b"R")[j // 3 % 4])
        if j % 4 == 1:
            s = s.lower()
        if j % 5 == 2:
            s = s.replace(b"T", b"U", 3)
        refs.append(s)
    if n_refs >= 2:
        refs[-1] = rc(refs[0].upper().replace(b"-", b"N").replace(b"R", b"N"))      # (N stays N: the same positions are invalid, mirrored)
    return tuple(refs)


@functools.lru_cache(maxsize=None)
def wrap_reference():
    """35 bases whose 32 4-mers are distinct: a table of 64 slots, half full"""
    rng = np.random.default_rng(5)
    while True:
        s = rand_seq(rng, 35)
        if len({s[i:i + 4] for i in range(32)}) == 32:
            return s


@functools.lru_cache(maxsize=None)
def screen_references():
    """64 references: a common stretch in all of them, a stretch that the references 3, 4 and 5 share, one of 3 500 bases"""
    rng = np.random.default_rng(42)
    common, shared = rand_seq(rng, COMMON), rand_seq(rng, 70)
    refs = []
    for j in range(SCREEN_R):
        n = 3500 if j == 0 else 260 + 3 * j
        s = rand_seq(rng, n)
        s = s[:100] + common + s[100:]
        if j in (3, 4, 5):
            s = s[:230] + shared + s[230:]
        refs.append(s)
    return tuple(refs)


@functools.lru_cache(maxsize=None)
def screen_bodies(k):
    """about 2 000 reads: cut from the references with 0 to 3 substitutions (some reverse-complemented), random reads, every length at
    which a strip or the k-mer ends, N and lower case at the strip edges, reads from the stretch that all references share"""
    rng = np.random.default_rng(7 + k)
    refs = screen_references()
    edges = [0, k - 1, k, k + 1, 63, 64, 65, 63 + k, 64 + k, 127, 128, 129]
    bodies = []

    def cut(j, n):
        ref = refs[j]
        n = min(n, len(ref))
        at = int(rng.integers(0, len(ref) - n + 1))
        s = bytearray(ref[at:at + n])
        for _ in range(int(rng.integers(0, 4))):
            if n:
                p = int(rng.integers(0, n))
                s[p] = LETTERS[(LETTERS.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
        s = bytes(s)
        return rc(s) if rng.integers(0, 2) else s

    for i in range(1990):
        n = edges[i // 3 % len(edges)] if i % 3 == 0 else int(rng.integers(30, 160))
        kind = i % 5
        if kind in (0, 1, 2):
            s = cut(int(rng.integers(0, SCREEN_R)), n)
        elif kind == 3:
            s = rand_seq(rng, n)
        else:
            s = refs[int(rng.integers(0, SCREEN_R))][100 - 10:100 + COMMON + 10][:max(n, k + 5)]      # the stretch all references hold
        if i % 7 == 0:
            s = spoil(s, (63,), b"N")
        if i % 11 == 0:
            s = spoil(s, (64,), b"n")
        if i % 13 == 0:
            s = spoil(s, (0, len(s) - 1), b"N")
        if i % 17 == 0:
            s = s[:60] + s[60:70].lower() + s[70:]
        if i % 19 == 0:
            s = s.replace(b"T", b"U", 2)
        bodies.append(s)
    long_read = refs[0][200:200 + LONG]
    bodies.insert(1000, spoil(long_read, (63, 64, 1500), b"N"))
    bodies.append(refs[4][210:330])                                            # the references 3, 4 and 5 together
    bodies.append(refs[10][:60] + refs[20][:50])                                # two references, the first with more positions
    bodies.append(refs[30][:50] + refs[12][:50])                                # a tie: the lower number is the best
    return tuple(bodies)


@functools.lru_cache(maxsize=None)
def screen_text(k, tail=b""):
    return b"".join(fastq(screen_bodies(k))) + tail

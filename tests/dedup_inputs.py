"""The generated inputs of the dedup tests, shared by test_gpu_bgzf_dedup.py (which runs them through the engine) and
test_cpu_bgzf_dedup.py (which asserts of every one of them that the referee's keys group the records exactly as their bytes do, so that
a collision cannot hide behind the referee).  Everything is computed once and never changed."""
import functools
import gzip
import os
import random

import dedup_ref

EDGES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 150]
LETTERS = b"ACGTNacgtnUuR."
N_GRID = 3000
LONG_AT, LONG = 1234, 5000
PARTS = [(0, 0), (0, 50), (3, 0), (64, 64), (200, 0)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test.fastq.bgzip.gz")


def rc(seq):
    return seq.translate(dedup_ref.COMP)[::-1]


@functools.lru_cache(maxsize=None)
def grid_bodies():
    """about 3000 bodies: lengths from EDGES or random below 160, one of 5000; every fifth is a copy, a case variant or the reverse
    complement of an earlier one, so that keys meet"""
    rng = random.Random(5)
    out = []
    for i in range(N_GRID):
        if i == LONG_AT:
            out.append(bytes(rng.choice(LETTERS) for _ in range(LONG)))
        elif i % 5 == 4 and i > 10:
            src = out[rng.choice([j for j in range(len(out)) if j != LONG_AT])]      # (one long read is enough)
            out.append(rng.choice([src, src.upper(), src.lower(), rc(src), src[:64] + src[64:].swapcase()]))
        else:
            L = rng.choice(EDGES) if i % 7 == 0 else rng.randrange(0, 160)
            out.append(bytes(rng.choice(LETTERS) for _ in range(L)))
    return out


def fastq(bodies, tag=b"r"):
    return [b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(bodies)]


@functools.lru_cache(maxsize=None)
def dup_bodies(n, seed, pool=None):
    """n bodies drawn from a pool of n // 3 sequences of 20 to 120 plain bases, a few of them as case variants or reverse complements"""
    rng = random.Random(seed)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(20, 121))) for _ in range(pool or max(1, n // 3))]
    out = []
    for _ in range(n):
        s = rng.choice(seqs)
        v = rng.randrange(10)
        out.append(s.lower() if v == 0 else rc(s) if v == 1 else s)
    return out


@functools.lru_cache(maxsize=None)
def paired_bodies(n=600, seed=31):
    """-> (R1, R2): pairs that are equal in R1 only, in R2 only and in both"""
    rng = random.Random(seed)
    new = lambda: bytes(rng.choice(b"ACGT") for _ in range(rng.randrange(30, 80)))
    r1, r2 = [], []
    for i in range(n):
        v = rng.randrange(4) if i > 20 else 0
        j = rng.randrange(i) if i else 0
        if v == 0:
            r1.append(new()); r2.append(new())
        elif v == 1:
            r1.append(r1[j]); r2.append(new())
        elif v == 2:
            r1.append(new()); r2.append(r2[j])
        else:
            r1.append(r1[j]); r2.append(r2[j])
    return r1, r2


@functools.lru_cache(maxsize=None)
def fasta_bodies(n=700):
    return dup_bodies(n, 8)


@functools.lru_cache(maxsize=None)
def golden_bodies():
    return gzip.decompress(open(GOLDEN, "rb").read()).split(b"\n")[1::4]


def with_bodies():
    """every (name, bodies, confs) the GPU tests key"""
    grid = [dedup_ref.conf(first=f, length=l, ignore_case=ic, canonical=ca) for f, l in PARTS for ic in (False, True) for ca in (False, True)]
    plain = [dedup_ref.conf(), dedup_ref.conf(ignore_case=True, canonical=True)]
    return [("grid", grid_bodies(), grid), ("windows", dup_bodies(1500, 11), plain), ("dedup", dup_bodies(900, 21), plain),
            ("fasta", fasta_bodies(), [dedup_ref.conf(record_lines=2), dedup_ref.conf(record_lines=2, canonical=True)]),
            ("golden", golden_bodies(), [dedup_ref.conf(), dedup_ref.conf(length=8)])]

"""Inputs of the k-mer count tests (test_cpu_bgzf_kcount.py, test_gpu_bgzf_kcount.py): the reads of the screen tests, and the repeats
that the run combine of za_k_kcount_reads is for."""
import functools

import numpy as np

from screen_inputs import fastq, rand_seq, rc, screen_bodies, spoil      # noqa: F401  (the tests take them from here)

GRID = ((1, False), (2, True), (15, True), (16, False), (17, True), (31, False), (31, True))      # (k, canonical) of the count grid
CONTENTION = 4096                                            # copies of one read


@functools.lru_cache(maxsize=None)
def repeat_bodies(k):
    """poly-G of every length at which a strip or the k-mer ends, reads with a poly-G tail, period 2 and 3, a reverse palindrome, an N
    inside a run, a run across a strip edge"""
    rng = np.random.default_rng(300 + k)
    head = rand_seq(rng, 90)
    half = rand_seq(rng, 40)
    bodies = [b"G" * n for n in (150, 64, 65, 63 + k, 64 + k)]
    bodies += [head + b"G" * 60, head[:50] + b"G" * 100, head[:13] + b"g" * 70 + head[:5]]      # poly-G tails (one in lower case)
    bodies += [b"AC" * 75, b"ACG" * 50, b"CA" * 40 + b"T"]
    bodies += [half + rc(half), b"AT" * 50, b"ACGT" * 30]                                        # reverse palindromes
    bodies += [b"G" * 40 + b"N" + b"G" * 80, spoil(b"T" * 150, (10, 63, 64, 100)), b"A" * 70 + b"n" + b"A" * 70]      # an N inside a run
    bodies += [head[:50] + b"C" * 40 + head[50:], head[:60] + b"T" * (k + 10) + head[60:]]      # runs that cross the strip edge at 64
    bodies += [b"G" * (k - 1), b"G" * k, b"", b"N" * 80]
    return tuple(bodies)


@functools.lru_cache(maxsize=None)
def contention_read():
    return rand_seq(np.random.default_rng(77), 150)

#!/usr/bin/env python3
"""Regenerates tests/golden/heldout/*.xz: the held-out corpora of the ratio gates (tests/test_oracle_ratio_heldout.py,
tests/test_gpu_ratio_heldout.py), stored so that the gates see the same bytes on every machine.

Each corpus is the first 2 MiB of what zlib_ng_amd.corpus.heldout assembles from the files of the machine this runs on
(Python sources of the standard library, the Python executable, the C library, C headers), compressed with xz.  The bars of
the gates were checked against the stored bytes; a regenerated set is other data and has to be checked again."""
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))

SIZE = 2 << 20


def main():
    from zlib_ng_amd import corpus
    out = os.path.join(HERE, "heldout")
    os.makedirs(out, exist_ok=True)
    for name, data in corpus.heldout(SIZE).items():
        path = os.path.join(out, name + ".xz")
        with open(path, "wb") as f:
            f.write(lzma.compress(data, preset=9 | lzma.PRESET_EXTREME))
        print(name, len(data), "bytes ->", os.path.getsize(path))


if __name__ == "__main__":
    main()

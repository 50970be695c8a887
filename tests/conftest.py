import gzip
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "python-zlib-ng_amd")
for p in (ROOT, PKG_DIR):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def heldout_corpora():
    """The held-out corpora of the ratio gates, stored under tests/golden/heldout (tests/golden/make_heldout.py) -> {name: bytes}"""
    import lzma
    d = os.path.join(GOLDEN, "heldout")
    return {f[:-3]: lzma.decompress(open(os.path.join(d, f), "rb").read()) for f in sorted(os.listdir(d)) if f.endswith(".xz")}


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def fastq():
    """3 578 369 bytes of FASTQ text: payload of the reference's tests/data/test.fastq.gz."""
    with gzip.open(os.path.join(GOLDEN, "test.fastq.gz"), "rb") as f:
        return f.read()


@pytest.fixture(scope="session")
def ctx():
    from zlib_ng_amd import _lib
    return _lib.default_context()

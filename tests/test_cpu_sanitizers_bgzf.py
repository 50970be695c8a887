"""The BGZF host scan (zngamd_bgzf_scan: no GPU, no context) under AddressSanitizer + UndefinedBehaviorSanitizer, beside
tests/test_cpu_sanitizers.py: the golden file, every truncation of a small stream, hostile BSIZE / XLEN / SLEN values and random
bytes behind a valid header -- the walk must never read outside the buffer it was given."""
import os
import subprocess
import sys
import textwrap

import pytest

from conftest import GOLDEN, PKG_DIR
from test_cpu_sanitizers import _run

SCAN_SCRIPT = textwrap.dedent("""
    import ctypes as C, os, random, struct, sys, zlib
    sys.path.insert(0, %r)
    from zlib_ng_amd import _lib
    assert _lib.LIB_PATH == os.environ["ZNGAMD_LIB"]
    raw = open(%r, "rb").read()
    code, blocks, used, total = _lib.bgzf_scan(raw)
    assert code == 0 and used == len(raw) and blocks[-1][2:] == (28, 0)

    def scan_exact(buf):
        # the buffer in a heap allocation of exactly its size: one byte too far is a report
        n = len(buf)
        mem = (C.c_uint8 * max(n, 1)).from_buffer_copy(buf or b"\\0")
        tab = (_lib.BgzfBlock * 8)()
        nb, cons, tot = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        r = _lib.load().zngamd_bgzf_scan(mem, n, tab, 8, C.byref(nb), C.byref(cons), C.byref(tot))
        assert cons.value <= n and nb.value <= 8
        return r, nb.value, cons.value

    def block(payload, data, bsize=None, xlen=6, slen=2):
        size = 18 + len(payload) + 8
        return (b"\\x1f\\x8b\\x08\\x04\\0\\0\\0\\0\\0\\xff" + struct.pack("<H", xlen) + b"BC" + struct.pack("<HH", slen, (size if bsize is None else bsize) - 1) +
                payload + struct.pack("<II", zlib.crc32(data), len(data)))

    data = b"blocked gzip " * 50
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    pay = co.compress(data) + co.flush()
    good = block(pay, data)
    small = good + good + raw[-28:]
    for cut in range(len(small) + 1):                       # every truncation
        r, nb, cons = scan_exact(small[:cut])
        assert r in (0, -3, -107), (cut, r)
        if cut >= len(good):
            assert r == 0 and nb == cut // len(good) if cut < len(small) else nb == 3
    for bs in (1, 2, 18, 25, 26, len(good) - 7, len(good) + 1, 65536):     # hostile BSIZE, alone and behind a good block
        for head in (b"", good):
            r, nb, cons = scan_exact(head + block(pay, data, bsize=bs))
            if bs < 26 or (bs > len(good) and not head):
                assert r == -3, (bs, len(head), r)
    for xlen in (0, 5, 7, 100, 65535):                      # extra fields that overrun the block or the buffer
        scan_exact(block(pay, data, xlen=xlen))
        scan_exact(good + block(pay, data, xlen=xlen))
    for slen in (0, 1, 3, 9, 65535):
        assert scan_exact(block(pay, data, slen=slen))[0] in (-3, -107)
    rnd = random.Random(11)
    for _ in range(300):                                    # random bytes behind the first bytes of a header
        keep = rnd.randrange(0, 19)
        buf = good[:keep] + bytes(rnd.getrandbits(8) for _ in range(rnd.randrange(0, 120)))
        scan_exact(buf)
        scan_exact(good + buf)
    assert _lib.load().zngamd_bgzf_scan(None, 0, None, 0, None, None, None) == -202
    print("bgzf scan clean")
""")


def test_bgzf_scan_under_asan_ubsan(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("zng_amd_build_asan", os.path.join(PKG_DIR, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    so = str(tmp_path / "libzng_amd_host_asan.so")
    mod.build_host_asan(so)
    clang = os.path.join(os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "..", "lib", "llvm", "bin", "clang")
    if not os.path.exists(clang):
        clang = "/opt/rocm/lib/llvm/bin/clang"
    runtime = subprocess.run([clang, "--print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(runtime) or not os.path.exists(runtime):
        pytest.skip("no shared AddressSanitizer runtime for hipcc's clang on this host")
    r = _run(runtime, {"ZNGAMD_LIB": so, "CUDA_VISIBLE_DEVICES": "", "HIP_VISIBLE_DEVICES": ""},
             [sys.executable, "-c", SCAN_SCRIPT % (PKG_DIR, os.path.join(GOLDEN, "test.fastq.bgzip.gz"))])
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    assert "bgzf scan clean" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr

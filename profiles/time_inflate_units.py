"""Kernel time of the unit-parallel indexed inflate (za_k_inflate_units_marked and the window kernels behind it) on MIB (default
1024) MiB of level-6 text: ONE deflate stream of dict-chained 128 KiB units with the writer's segment index, as
profiles/time_inflate_members.py does for the member decoder; ZNGAMD_LIB points at a variant build to compare with.
usage: profiles/time_inflate_units.py [cmp variant.so ...]   (cmp: the variants, then the product build, one process each)"""
import ctypes as C, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] == "cmp":
    for so in sys.argv[2:] + [None]:
        env = dict(os.environ, ABL="[%s]" % (os.path.basename(so) if so else "product"))
        if so:
            env["ZNGAMD_LIB"] = os.path.join(ROOT, so)
        subprocess.check_call([sys.executable, os.path.abspath(__file__)], env=env)
    sys.exit(0)
sys.path.insert(0, os.path.join(ROOT, "python-zlib-ng_amd"))
import numpy as np
import torch
from zlib_ng_amd import _lib, corpus
ctx = _lib.Context(0); L, h = ctx.L, ctx.h
n = int(os.environ.get("MIB", "1024")) << 20; B = 131072; nb = n // B
host = corpus.text(64 << 20, seed=1)
d = torch.cat([torch.from_numpy(host).cuda().repeat(n // host.size), torch.zeros(64, dtype=torch.uint8, device="cuda")])
p = lambda t: C.c_void_p(t.data_ptr())
blocks = (_lib.Block * nb)()
for b in range(nb):
    blocks[b] = _lib.Block(b * B, B, 32768 if b else 0, _lib.FLAG_SEG2K, 0)
assert L.zngamd_count_units(blocks, nb) == nb
comp = torch.empty(n // 2 + (64 << 20), dtype=torch.uint8, device="cuda")
ulen = torch.empty(nb, dtype=torch.int32, device="cuda"); ucrc = torch.empty(nb, dtype=torch.int32, device="cuda")
tot = C.c_uint64(0)
assert L.zngamd_deflate_blocks_packed_dev(h, p(d), n, blocks, nb, 6, p(comp), comp.numel() - 64, p(ulen), p(ucrc), None, C.byref(tot)) == 0
index = ctx.deflate_index(nb)
comp[tot.value:tot.value + 66] = 0
comp[tot.value] = 3                                          # the empty last block
uin, uout = ulen.cpu().numpy().astype(np.uint32), np.full(nb, B, np.uint32)
out = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
best = None
for it in range(4):
    out.zero_()
    ctx.profiling(True); ctx.kernel_times(True)
    r, got = ctx.inflate_units_indexed_dev(comp.data_ptr(), tot.value + 2, uin, uout, index.ptr, out.data_ptr(), n)
    kt = ctx.kernel_times(True)
    best = kt["inflate"][0] if best is None else min(best, kt["inflate"][0])
ok = r == _lib.STREAM_END and got == n and bool((out[:n] == d[:n]).all().item())
print("%-40s rc %d output ok %-5s inflate %.3f ms (%d units, stream %d bytes)" % (os.environ.get("ABL", "product build"), r, ok, best, nb, tot.value))
sys.exit(0 if ok else 1)

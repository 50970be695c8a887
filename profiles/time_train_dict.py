"""Dictionary training (batch.train_dict): what the trained dictionary buys and what training costs.

Ratios: records of 1 and 4 KiB, level 6, zlib container, compressed with batch.compress.  Training set = the first 1 MiB of each
stored held-out corpus (tests/golden/heldout) cut into records, 4 MiB for json_lines (profiles/time_batch_zdict.py, seed 7); test set =
up to 1 000 records cut from what follows.  Columns: input / output bytes without a dictionary, with the naive one (the first 32 KiB of
the training set) and with a trained 32 KiB one for k = 128, 256, 512 (d = 8).

Times: 1 KiB records of corpus.text (seed 1), 32 KiB, k = 256, d = 8; best of 3 (1 GiB: of 2), ms for the whole call.  dev = samples
already in device memory (train_dict_dev), host = a Python list (train_dict: joined, uploaded), ref = tests/dict_train_ref.py on the
16 MiB cell only.

    python profiles/time_train_dict.py            # the tables
    python profiles/time_train_dict.py --trace    # one call of each form per size, for rocprofv3 --kernel-trace --stats; the
                                                  # number of picks per call is on stderr ([zngamd] train_dict: ...)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-zlib-ng_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "profiles")]
if "--trace" in sys.argv:
    os.environ["ZNGAMD_TRACE"] = "1"
from zlib_ng_amd import _lib, batch, corpus, devmem  # noqa: E402

DICT = 32768


def corpora():
    from conftest import heldout_corpora
    from time_batch_zdict import json_lines
    out = [(name, data, 1 << 20) for name, data in heldout_corpora().items()]
    out.append(("json_lines", json_lines(6 << 20, seed=7), 4 << 20))
    return out


def ratios():
    print("ratio: input / output bytes of the test records (batch.compress, level 6, zlib)")
    print(f"{'corpus':>15} {'rec':>5} {'items':>5} | {'none':>6} {'naive':>6} | {'k=128':>6} {'k=256':>6} {'k=512':>6} | {'256 vs naive':>12}")
    for name, data, tsize in corpora():
        for rec in (1024, 4096):
            train, rest = data[:tsize], data[tsize:]
            samples = [train[i:i + rec] for i in range(0, len(train), rec)]
            records = [rest[i * rec:(i + 1) * rec] for i in range(min(1000, len(rest) // rec))]
            raw = sum(map(len, records))
            size = lambda z: sum(len(c) for c in batch.compress(records, 6, zdict=z))
            r = {"none": raw / size(None), "naive": raw / size(train[:DICT])}
            for k in (128, 256, 512):
                r[k] = raw / size(batch.train_dict(samples, DICT, k=k, d=8))
            print(f"{name:>15} {rec:5d} {len(records):5d} | {r['none']:6.3f} {r['naive']:6.3f} | {r[128]:6.3f} {r[256]:6.3f} {r[512]:6.3f} | "
                  f"{100 * (r[256] / r['naive'] - 1):+11.1f}%", flush=True)


def best(f, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = f()
        ts.append(time.perf_counter() - t)
    return min(ts), r


def times(trace):
    import dict_train_ref as R
    ctx = _lib.default_context()
    print("\ntraining time, 1 KiB records of corpus.text, 32 KiB, k = 256, d = 8 (ms)")
    print(f"{'size':>8} {'records':>8} | {'dev':>8} {'host':>8} {'ref':>8} | dev == host == ref")
    for mib in (16, 256, 1024):
        blob = corpus.text(mib << 20, seed=1).tobytes()
        n = len(blob) // 1024
        samples = [blob[i << 10:(i + 1) << 10] for i in range(n)]
        offs = np.arange(n, dtype=np.uint64) * np.uint64(1024)
        lens = np.full(n, 1024, dtype=np.uint64)
        d_in = devmem.from_host(ctx, np.frombuffer(blob + bytes(64), np.uint8))
        del blob
        if trace:
            batch.train_dict_dev(ctx, d_in, offs, lens)
            batch.train_dict(samples)
            print(f"{mib} MiB: traced", flush=True)
            continue
        reps = 2 if mib >= 1024 else 3
        batch.train_dict(samples[:4096])
        td, dd = best(lambda: batch.train_dict_dev(ctx, d_in, offs, lens), reps)
        th, dh = best(lambda: batch.train_dict(samples), reps)
        ref, same = "", dd == dh
        if mib == 16:
            tr, dr = best(lambda: R.train(samples), 1)
            ref, same = f"{tr * 1e3:8.0f}", same and dr == dd
        print(f"{mib:5d} MiB {n:8d} | {td * 1e3:8.1f} {th * 1e3:8.1f} {ref:>8} | {same}", flush=True)
        del d_in, samples


def main():
    trace = "--trace" in sys.argv
    if not trace:
        ratios()
    times(trace)


if __name__ == "__main__":
    main()

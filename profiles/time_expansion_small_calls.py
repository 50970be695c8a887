"""Small host calls: the eager path of deflate_host_common (a bound of up to 512 KiB: results and bytes come back in one copy) and
small batch calls.  Host clock around calls that end in a stream synchronise; 30 warm-up calls, then the median of 300.

    python profiles/time_expansion_small_calls.py                  # the tree's library
    ZNGAMD_LIB=/path/to/libzng_amd.so python profiles/time_expansion_small_calls.py

To compare two builds, run them alternately, each in a process of its own (profiles/expansion_bounds_small_calls.txt)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "python-zlib-ng_amd"), os.path.join(ROOT, "tests")]


def main():
    from zlib_ng_amd import _lib, batch, corpus
    import expansion_inputs as X
    ctx = _lib.default_context()
    text = corpus.text(65536, seed=5).tobytes()
    records = [text[i * 600:i * 600 + 1024] for i in range(100)]
    cases = {
        "blocks_text64k_default": lambda: ctx.deflate_blocks(text, [(0, 65536, 0, 1)], 6, 80000),
        "blocks_text64k_fixed": lambda: ctx.deflate_blocks(text, [(0, 65536, 0, 1)], 6, 80000, strategy=4),
        "blocks_high64_64k_fixed": lambda: ctx.deflate_blocks(X.high64(65536), [(0, 65536, 0, 1)], 6, 80000, strategy=4),
        "blocks_text4k_default": lambda: ctx.deflate_blocks(text[:4096], [(0, 4096, 0, 1)], 6, 6000),
        "batch_100x1k_text_default": lambda: batch.compress(records, 6),
        "batch_100x1k_text_fixed": lambda: batch.compress(records, 6, strategy=4),
    }
    out = {}
    for name, fn in cases.items():
        for _ in range(30):
            fn()
        ts = []
        for _ in range(300):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        ts.sort()
        out[name] = {"median_us": round(1e6 * ts[150], 1), "p10_us": round(1e6 * ts[30], 1), "p90_us": round(1e6 * ts[270], 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

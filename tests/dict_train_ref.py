"""Pure-Python/numpy reference of the batch API's dictionary trainer: a FastCOVER variant whose every step is
fixed, so that the GPU trainer (za_dict.hip) and this one agree byte for byte.

    train(samples, dict_size=32768, k=256, d=8) -> bytes

A helper of the tests (like deflate_walk.py), not a test module.
"""
import numpy as np

PRIME = 0xCF1BBCDCB7A56463
HASH_BITS = 20
SENT = 0xFFFFFFFF


def epochs(n, dict_size, k):
    """-> (E, S): the number of epochs and their size in positions (step 4)"""
    E = max(1, dict_size // k // 4)
    S = n // E
    if S < 10 * k:
        E = max(1, n // (10 * k))
        S = n // E
    return E, S


def hashes(data, lengths, d):
    """-> (h, valid) over the n = len(data) - d + 1 positions: the d-mer hash of every position (step 2) and whether the d-mer lies
    inside its own sample (step 1)"""
    n = len(data) - d + 1
    v = np.zeros(n, dtype=np.uint64)
    for j in range(d):
        v |= data[j:j + n].astype(np.uint64) << np.uint64(8 * j)
    with np.errstate(over="ignore"):
        h = ((v * np.uint64(PRIME)) >> np.uint64(64 - HASH_BITS)).astype(np.int64)
    inv = np.zeros(n + 1, dtype=np.int64)
    for end in np.cumsum(np.asarray(lengths, dtype=np.int64)).tolist():
        lo, hi = max(0, end - d + 1), min(end, n)
        if lo < hi:
            inv[lo] += 1
            inv[hi] -= 1
    valid = np.cumsum(inv[:n]) == 0
    return h, valid


def train(samples, dict_size=32768, k=256, d=8, stats=None):
    """The trained dictionary (bytes, at most dict_size long) of `samples` (a sequence of bytes-like objects, taken in order).
    stats: a dict that receives the number of picks ("picks") and of epochs ("epochs")."""
    lengths = [memoryview(s).nbytes for s in samples]
    data = np.frombuffer(b"".join(bytes(s) for s in samples), dtype=np.uint8)
    total = len(data)
    assert samples and k <= total < 1 << 32 and 4 <= d <= 8 and d <= dict_size <= 32768 and d <= k <= 16384
    n = total - d + 1
    K = k - d + 1
    h, valid = hashes(data, lengths, d)
    freq = np.bincount(h[valid], minlength=1 << HASH_BITS).astype(np.int64)
    E, S = epochs(n, dict_size, k)
    # per epoch: its valid positions, their hashes and the first window start each counts for (step 5)
    ep = []
    for e in range(E):
        es = e * S
        P = np.nonzero(valid[es:es + S])[0] + es
        hp = h[P]
        order = np.argsort(hp, kind="stable")               # by hash, then position
        prev = np.full(len(P), -1, dtype=np.int64)
        same = hp[order][1:] == hp[order][:-1]
        prev[order[1:][same]] = P[order[:-1][same]]
        lo = np.maximum(np.maximum(prev + 1, P - K + 1), es)
        ep.append((es, P, hp, lo))
    out = bytearray(dict_size)
    tail, e, zero_run, picks = dict_size, 0, 0, 0
    while tail > 0:
        if S < K:
            break
        es, P, hp, lo = ep[e]
        f = freq[hp]
        nz = f > 0
        nst = S - K + 1                                      # window starts of the epoch
        diff = np.bincount(lo[nz] - es, weights=f[nz], minlength=S + 1).astype(np.int64)
        diff -= np.bincount(P[nz] - es + 1, weights=f[nz], minlength=S + 1).astype(np.int64)
        score = np.cumsum(diff[:nst])
        i = int(np.argmax(score))                            # the first of the best: ties go to the lowest start
        picks += 1
        if score[i] == 0:
            zero_run += 1
            if zero_run >= E:
                break
            e = (e + 1) % E
            continue
        zero_run = 0
        start = es + i
        w = np.arange(start, start + K)
        fw = np.where(valid[w], freq[h[w]], 0)
        hit = np.nonzero(fw > 0)[0]
        s0, s1 = start + int(hit[0]), start + int(hit[-1])   # trimmed: freq read before the zeroing
        span = np.arange(s0, s1 + 1)
        freq[h[span][valid[span]]] = 0
        size = min(s1 - s0 + d, tail)
        if size < d:
            break
        tail -= size
        out[tail:tail + size] = data[s0:s0 + size].tobytes()
        e = (e + 1) % E
    if stats is not None:
        stats["picks"], stats["epochs"] = picks, E
    return bytes(out[tail:])

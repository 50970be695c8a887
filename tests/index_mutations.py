"""Wrong segment indexes made from right ones: the one place that knows how.  Host arrays only -- the GPU tests
(test_gpu_index_hostile.py), the parser tests (test_cpu_index_tail.py) and profiles/fuzz_index_rows.py import it.

An index is what the threaded writer leaves behind its data member and what zngamd_inflate_units_indexed_dev takes: per unit the
compressed bytes (`uin`), the output bytes (`uout`) and a row of bit offsets -- entry s = where segment s (2 KiB of output) begins,
entry nseg = where the end-of-block code stands; a unit of stored blocks has entry nseg == 0.  Every case below keeps the framing
intact (array shapes, the sum of uin, every uout within 0..131 072) and changes only numbers the decoder has to check against the
stream itself.

rows_cases() -> (name, uin', uout', rows', must_refuse); tail_cases() -> (name, rec', unit): the same through a file's records.
`name` begins with the class id ("R1:", "F3:", ...).  A generator never yields a case equal to its input."""
import struct

import numpy as np

SEG = 2048
MAX_UNIT = 131072
KINDS = ("dynamic", "fixed", "stored", "empty")


def nseg_of(n):
    return (int(n) + SEG - 1) // SEG


def kinds_of(stream, uin, uout, rows):
    """a unit's kind as the decoder will see it: from uout == 0, from rows[u, nseg] == 0, and from the first three bits of its bytes"""
    kinds, at = [], 0
    for u in range(len(uin)):
        if int(uout[u]) == 0:
            kinds.append("empty")
        elif int(rows[u, nseg_of(uout[u])]) == 0:
            kinds.append("stored")
        else:
            kinds.append({1: "fixed", 2: "dynamic"}[(stream[at] >> 1) & 3])
        at += int(uin[u])
    return kinds


def _case(name, orig, new, must_refuse):
    assert any(not np.array_equal(a, b) for a, b in zip(orig, new)), "mutation %s changed nothing" % name
    assert int(new[0].astype(np.int64).sum()) == int(orig[0].astype(np.int64).sum()), name      # the units' bytes stay the stream's
    assert int(new[1].max(initial=0)) <= MAX_UNIT, name
    return (name,) + tuple(new) + (must_refuse,)


def rows_cases(uin, uout, rows, kinds):
    """uin, uout: uint32[nu]; rows: uint32[nu, INDEX_STRIDE]; kinds[u] in KINDS.  The inputs are left as they are."""
    uin = np.ascontiguousarray(uin, dtype=np.uint32)
    uout = np.ascontiguousarray(uout, dtype=np.uint32)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    nu = len(uin)
    assert rows.shape[0] == nu and rows.shape[1] >= 65 and len(kinds) == nu and all(k in KINDS for k in kinds)
    orig = (uin, uout, rows)
    ns = [nseg_of(n) for n in uout]
    coded = [u for u in range(nu) if kinds[u] in ("dynamic", "fixed") and ns[u] >= 1]
    dyn = [u for u in coded if kinds[u] == "dynamic"]

    def emit(name, u, row, must=True):
        r = rows.copy()
        r[u] = row
        return _case(name, orig, (uin, uout, r), must)

    def put(u, s, v):
        row = rows[u].copy()
        row[s] = np.uint32(v)
        return row

    # R1: an interior entry moved, swapped with the next, set equal to a neighbour
    for u in dyn:
        for s in sorted({1, ns[u] // 2, ns[u] - 1}):
            if not 0 < s < ns[u]:
                continue
            v, nxt, prv = int(rows[u, s]), int(rows[u, s + 1]), int(rows[u, s - 1])
            for d in (1, -1, 7, -7, 8, -8):
                if 0 <= v + d < (1 << 23):
                    yield emit("R1:u%d:s%d:%+d" % (u, s, d), u, put(u, s, v + d))
            if nxt != v:
                row = put(u, s, nxt)
                row[s + 1] = v
                yield emit("R1:u%d:s%d:swap" % (u, s), u, row)
                yield emit("R1:u%d:s%d:eqnext" % (u, s), u, put(u, s, nxt))
            if prv != v:
                yield emit("R1:u%d:s%d:eqprev" % (u, s), u, put(u, s, prv))
    # R2: the first token (the header's end); R3: the end-of-block entry
    for u in coded:
        for d in (1, -1):
            if int(rows[u, 0]) + d >= 0:
                yield emit("R2:u%d:%+d" % (u, d), u, put(u, 0, int(rows[u, 0]) + d))
            if int(rows[u, ns[u]]) + d > 0:
                yield emit("R3:u%d:%+d" % (u, d), u, put(u, ns[u], int(rows[u, ns[u]]) + d))
    for u in dyn:
        if rows[u, ns[u]] != 0:
            yield emit("R3:u%d:zero" % u, u, put(u, ns[u], 0))          # reads as "stored"
    # R4: a stored unit with a dynamic unit's rows, a dynamic unit with a stored unit's
    for u in range(nu):
        if kinds[u] == "stored":
            for j in dyn:
                if ns[j] == ns[u] and not np.array_equal(rows[j], rows[u]):
                    yield emit("R4:u%d:rows-of-dynamic-u%d" % (u, j), u, rows[j].copy())
                    break
    for u in dyn:
        if rows[u].any():
            yield emit("R4:u%d:zeros" % u, u, np.zeros_like(rows[u]))
    # R5: another dynamic unit's rows
    for u in dyn:
        for j in dyn:
            if j != u and ns[j] == ns[u] and not np.array_equal(rows[j, :ns[u] + 1], rows[u, :ns[u] + 1]):
                yield emit("R5:u%d:rows-of-u%d" % (u, j), u, rows[j].copy())
                break
    # R6: the overshoot field; R7: an entry beyond the unit's bits, a decreasing pair
    for u in coded:
        for s in sorted({0, ns[u] // 2, ns[u]}):
            for bit in (23, 31):
                if not (int(rows[u, s]) >> bit) & 1:
                    yield emit("R6:u%d:s%d:bit%d" % (u, s, bit), u, put(u, s, int(rows[u, s]) | (1 << bit)))
            if int(rows[u, s]) != 0x7FFFFF:
                yield emit("R7:u%d:s%d:far" % (u, s), u, put(u, s, 0x7FFFFF))
        s = max(1, ns[u] // 2)
        lo = int(rows[u, s - 1])
        if lo >= 1 and int(rows[u, s]) != lo - 1:
            yield emit("R7:u%d:s%d:decreasing" % (u, s), u, put(u, s, lo - 1))
    # R8: compressed bytes moved between neighbours (the sum kept)
    for k in range(nu - 1):
        for d in (1, 5):
            if int(uin[k + 1]) >= d:
                a = uin.copy()
                a[k] += d
                a[k + 1] -= d
                yield _case("R8:u%d:+%d" % (k, d), orig, (a, uout, rows), True)
        if uin[k] != uin[k + 1]:
            a = uin.copy()
            a[k], a[k + 1] = a[k + 1], a[k]
            yield _case("R8:u%d:swap" % k, orig, (a, uout, rows), True)
    # R9: output bytes moved between neighbours (the sum kept)
    for k in range(nu - 1):
        a, b = int(uout[k]), int(uout[k + 1])
        if a >= 1 and b >= 2 and nseg_of(a + 1) == ns[k] and nseg_of(b - 1) == ns[k + 1]:
            o = uout.copy()
            o[k] += 1
            o[k + 1] -= 1
            yield _case("R9:u%d:+1" % k, orig, (uin, o, rows), True)
        if a - SEG >= 1 and 1 <= b + SEG <= MAX_UNIT and b >= 1:
            o = uout.copy()
            o[k] -= SEG
            o[k + 1] += SEG
            yield _case("R9:u%d:-2048" % k, orig, (uin, o, rows), True)
    # R10: a unit with output claimed empty (its bytes kept); an empty one claimed to hold a byte
    for k in range(nu):
        if kinds[k] != "empty" and uout[k] != 0:
            o = uout.copy()
            o[k] = 0
            yield _case("R10:u%d:claimed-empty" % k, orig, (uin, o, rows), True)
        if kinds[k] == "empty" and uout[k] == 0:
            o = uout.copy()
            o[k] = 1
            yield _case("R10:u%d:empty-claimed-1" % k, orig, (uin, o, rows), True)
    # S1: entries nobody may read
    for u in dyn:
        if (rows[u, ns[u] + 1:] != 0xFFFFFFFF).any():
            row = rows[u].copy()
            row[ns[u] + 1:] = 0xFFFFFFFF
            yield emit("S1:u%d:behind-eob" % u, u, row, must=False)
    for u in range(nu):
        if kinds[u] == "stored" and rows[u, ns[u]] == 0:
            row = rows[u].copy()
            row[:ns[u]] = np.arange(17, 17 + ns[u], dtype=np.uint32) * 1000
            if not np.array_equal(row, rows[u]):
                yield emit("S1:u%d:stored-front" % u, u, row, must=False)


ROW_CLASSES = ("R1", "R2", "R3", "R4", "R5", "R6", "R7", "R8", "R9", "R10", "S1")


# ---- the same through a file's records (zlib_ng_amd._lib._index_rec_dtype(): in_len, out_len, e[65] two-byte deltas -- e[0] the first
# token's bit offset, e[s] the bits of segment s - 1; all zeros: stored)

def rec_kinds(rec):
    out = []
    for r in rec:
        if int(r["out_len"]) == 0:
            out.append("empty")
        elif int(r["e"].max()) == 0:
            out.append("stored")
        else:
            out.append("fixed" if int(r["e"][0]) == 3 else "dynamic")
    return out


def tail_cases(rec):
    """-> (name, rec', unit): unit = the first unit of the stream whose record is wrong.  F1-F5 keep every sum the parser can
    check (in_len against the member's size, out_len against ISIZE); F6 breaks the second."""
    nu = len(rec)
    kinds = rec_kinds(rec)
    ns = [nseg_of(r["out_len"]) for r in rec]
    dyn = [u for u in range(nu) if kinds[u] == "dynamic"]

    def case(name, new, unit):
        assert new.tobytes() != rec.tobytes(), "mutation %s changed nothing" % name
        assert int(new["in_len"].astype(np.int64).sum()) == int(rec["in_len"].astype(np.int64).sum()), name
        if not name.startswith("F6"):
            assert int(new["out_len"].astype(np.int64).sum()) == int(rec["out_len"].astype(np.int64).sum()), name
            assert int(new["out_len"].max()) <= MAX_UNIT, name
        return name, new, unit

    # F1: one entry moved, the entries behind it kept
    for u in dyn:
        for s in sorted({0, ns[u] // 2, ns[u] - 1}):
            for d in (1, 7, 8, -1, -7, -8):
                a, b = int(rec["e"][u][s]) + d, int(rec["e"][u][s + 1]) - d
                if 0 <= a <= 0xFFFF and 0 <= b <= 0xFFFF:
                    new = rec.copy()
                    new["e"][u][s], new["e"][u][s + 1] = a, b
                    yield case("F1:u%d:s%d:%+d" % (u, s, d), new, u)
    # F2 = R8
    for k in range(nu - 1):
        for d in (1, 5):
            if int(rec["in_len"][k + 1]) >= d:
                new = rec.copy()
                new["in_len"][k] += d
                new["in_len"][k + 1] -= d
                yield case("F2:u%d:+%d" % (k, d), new, k)
        if rec["in_len"][k] != rec["in_len"][k + 1]:
            new = rec.copy()
            new["in_len"][k], new["in_len"][k + 1] = rec["in_len"][k + 1], rec["in_len"][k]
            yield case("F2:u%d:swap" % k, new, k)
    # F3 = R9 and R10 (the sum kept: what a claimed-empty unit loses, another unit -- its neighbour, or the farthest with room -- gains)
    for k in range(nu - 1):
        a, b = int(rec["out_len"][k]), int(rec["out_len"][k + 1])
        if a >= 1 and b >= 2 and nseg_of(a + 1) == ns[k] and nseg_of(b - 1) == ns[k + 1]:
            new = rec.copy()
            new["out_len"][k] += 1
            new["out_len"][k + 1] -= 1
            yield case("F3:u%d:+1" % k, new, k)
        if a - SEG >= 1 and b >= 1 and b + SEG <= MAX_UNIT:
            new = rec.copy()
            new["out_len"][k] -= SEG
            new["out_len"][k + 1] += SEG
            yield case("F3:u%d:-2048" % k, new, k)
    for k in range(nu):
        n = int(rec["out_len"][k])
        if kinds[k] != "empty":
            room = [j for j in range(nu) if j != k and kinds[j] != "empty" and int(rec["out_len"][j]) + n <= MAX_UNIT]
            near = [j for j in room if abs(j - k) == 1]
            for nm, j in (("near", near[0] if near else None), ("far", max(room, key=lambda j: abs(j - k)) if room else None)):
                if j is not None:
                    new = rec.copy()
                    new["out_len"][k] = 0
                    new["out_len"][j] += n
                    yield case("F3:u%d:claimed-empty:%s-u%d" % (k, nm, j), new, min(k, j))
        else:
            for j in (k - 1, k + 1):
                if 0 <= j < nu and int(rec["out_len"][j]) >= 2:
                    new = rec.copy()
                    new["out_len"][k] = 1
                    new["out_len"][j] -= 1
                    yield case("F3:u%d:empty-claimed-1:from-u%d" % (k, j), new, min(k, j))
                    break
    # F4 = R4; F5 = R5
    for u in range(nu):
        if kinds[u] == "dynamic":
            new = rec.copy()
            new["e"][u] = 0
            yield case("F4:u%d:zeros" % u, new, u)
        if kinds[u] == "stored":
            for j in dyn:
                if ns[j] == ns[u]:
                    new = rec.copy()
                    new["e"][u] = rec["e"][j]
                    yield case("F4:u%d:deltas-of-dynamic-u%d" % (u, j), new, u)
                    break
    for u in dyn:
        for j in dyn:
            if j != u and ns[j] == ns[u] and not np.array_equal(rec["e"][j], rec["e"][u]):
                new = rec.copy()
                new["e"][u] = rec["e"][j]
                yield case("F5:u%d:deltas-of-u%d" % (u, j), new, u)
                break
    # F6: the units' output no longer adds up to the member's ISIZE
    new = rec.copy()
    new["out_len"][nu - 1] += 1
    yield case("F6:u%d:+1" % (nu - 1), new, nu - 1)


TAIL_CLASSES = ("F1", "F2", "F3", "F4", "F5", "F6")


def split_tail(blob):
    """-> (bytes of the data member, has a trailing plain empty member) of a file that begins with its data member and ends with
    an index tail"""
    from zlib_ng_amd import _lib
    skip = 0
    for _ in (0, 1):
        loc = blob[len(blob) - skip - _lib.INDEX_LOCATOR_BYTES:len(blob) - skip]
        if loc[:4] == b"\x1f\x8b\x08\x04" and loc[12:14] == b"ZA" and loc[16:18] == b"\x03\x02":
            break
        tail = blob[-20:]
        assert skip == 0 and tail[:4] == b"\x1f\x8b\x08\x00" and tail[10:] == b"\x03\x00" + bytes(8), "no index tail"
        skip = 20
    nm, nu, ibytes, dbytes = struct.unpack("<IIQQ", loc[20:44])
    assert dbytes + ibytes + _lib.INDEX_LOCATOR_BYTES + skip == len(blob)
    return dbytes, skip == 20


def rebuild(blob, rec):
    """the file with its index members and locator replaced by those of `rec`; a trailing plain empty member is kept"""
    from zlib_ng_amd import _lib
    dbytes, plain = split_tail(blob)
    return blob[:dbytes] + _lib.index_members([rec], dbytes) + (blob[-20:] if plain else b"")

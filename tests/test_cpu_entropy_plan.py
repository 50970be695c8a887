"""Anchors tests/huffman_ref.py -- the plain reference of the entropy plan and of the search-free parses (3.7) --
before any kernel is judged by it (tests/test_gpu_entropy_plan.py): its lengths, block types, end-of-block offsets, sizes and
bytes against the oracle on the oracle's own histograms; its Z_RLE and Z_HUFFMAN_ONLY tokens against the system zlib's; Kraft,
limit, monotony and the package-merge optimum on every built histogram; and that every built input reaches the branch it was
built for.  No GPU."""
import random
import zlib

import pytest

import deflate_walk as W
import huffman_ref as H
import plan_inputs as I


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.lib()
    return oracle


def _stitched(fastq):
    """random bytes, FASTQ, zeros and a short period stitched at odd places"""
    rng = random.Random(21)
    return rng.randbytes(9001) + fastq[300000:340007] + bytes(7003) + (b"0123456789abc" * 2000)[:20011] + rng.randbytes(1234) + fastq[:30001]


def _units(fastq):
    rng = random.Random(7)
    rnd = rng.randbytes(131072)
    mixed = fastq[:40000] + rnd[:30000] + bytes(20000) + fastq[50000:91072]
    return {"fastq128k": fastq[:131072], "fastq_tail": fastq[131072:131072 + 100001], "zeros": bytes(131072), "random": rnd,
            "mixed": mixed, "period36": (b"abcdefghijklmnopqrstuvwxyz0123456789" * 4000)[:131072], "tiny5": b"hello", "len1": b"x",
            "len3": b"abc", "seg_edge": fastq[:2049], "s33": fastq[:33], "s700": fastq[100:800], "s3000": fastq[:3000],
            "s10000": mixed[35000:45000], "s65537": fastq[:65537], "ladder": I.distance_ladder(), "stitched": _stitched(fastq)}


def _forced(hd):
    fd = list(hd)
    if sum(1 for f in fd if f) < 2 and fd[0] == 0:
        fd[0] = 1
    if sum(1 for f in fd if f) < 2:
        fd[1] = 1
    return fd


def _oracle_case(O, data, level, flags):
    out, crc, dbg = O.deflate_unit(data, b"", level, flags, debug=True)
    h = [int(x) for x in dbg["hist"]]
    hl, hd = h[:286], h[288:318]
    lens = [int(x) for x in dbg["lens"]]
    n = len(data)
    P = H.plan(hl, hd, n, final=bool(flags & 1), flat=bool(flags & 2))
    assert P.btype == dbg["btype"], (P.btype, dbg["btype"], P.cost_dyn, P.cost_fix, P.cost_sto)
    assert P.size == len(out)
    if dbg["btype"] != 1:           # (the oracle overwrites its lengths with the fixed code's when it takes the fixed block)
        assert H.spec_lengths(hl, 10) == lens[:286]
        assert H.spec_lengths(_forced(hd), 9) == lens[288:318]
    else:
        assert P.ll_lens == lens[:288] and P.d_lens == lens[288:320]
    if P.btype:
        seg = 1 << O.seg_shift(n, flags)
        assert P.eob_bit == int(dbg["seg_bits"][(n + seg - 1) // seg])
    # the oracle's bytes from the reference's plan and codes: the tokens are read back from the oracle's stream by the walker
    w = W.walk(out)
    assert w.out == data
    assert H.emit(P, w.tokens, data, final=bool(flags & 1), flat=bool(flags & 2)) == out
    if P.btype == 2:
        b = w.blocks[0]
        assert (b.hlit, b.hdist, b.ll_lens, b.d_lens) == (P.hlit, P.hdist, P.ll_lens[:P.hlit], P.d_lens[:P.hdist])
        assert b.header_bits == P.header_bits and b.eob_bit == P.eob_bit
        if not flags & 2:
            assert b.hclen == P.hclen and b.cl_lens == P.cl_lens
    return P


@pytest.mark.parametrize("level", [1, 6, 9])
def test_reference_against_oracle(O, fastq, level):
    """spec_lengths on the oracle's histograms == the oracle's lengths, both alphabets; block type, end-of-block offset, size;
    and the oracle's bytes rebuilt from the reference's header and canonical codes"""
    big = ("fastq128k", "zeros", "random", "period36", "fastq_tail", "mixed")
    for name, data in _units(fastq).items():
        _oracle_case(O, data, level, 0)
        if level == 6 and name not in big:
            for flags in (1, 2, 3):
                _oracle_case(O, data, level, flags)


def test_canonical_codes_rfc_example():
    """RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111, stored bit-reversed"""
    codes = H.canonical_codes([3, 3, 3, 3, 3, 2, 4, 4])
    assert codes == [0b010, 0b110, 0b001, 0b101, 0b011, 0b00, 0b0111, 0b1111]
    assert H.canonical_codes([0, 1, 0, 1]) == [0, 0, 0, 1]


def _zlib_tokens(data, strategy):
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, strategy)
    w = W.walk(c.compress(data) + c.flush())
    assert w.out == data
    return None if 0 in w.btypes else w.tokens         # (zlib stores what does not compress: no tokens to compare)


def test_rle_tokens_against_zlib():
    """one segment covering the input: zlib's own deflate_rle is the reference"""
    cases = I.one_segment_rle_inputs()
    cases += [d for _, d, _ in I.rle_small_units()]
    cases += [d for _, d, fl in I.rle_sized_units(lambda n, f: 11) if len(d) <= 10000]
    cases.append(I.rle_all_symbols())
    compared = 0
    for data in cases:
        ref = _zlib_tokens(data, zlib.Z_RLE)
        if ref is not None:
            assert H.rle_tokens(data, 1 << 20) == ref, data[:40]
            compared += 1
    assert compared >= len(cases) - 8, (compared, len(cases))
    compared = 0
    for name, data in I.huffman_only_inputs()[:12]:
        ref = _zlib_tokens(data, zlib.Z_HUFFMAN_ONLY)
        if ref is not None:
            assert H.literal_tokens(data) == ref, name
            compared += 1
    assert compared >= 10


def test_rle_segment_cut():
    """what only the text states: a run never passes a segment end, and the byte in front of a segment is its neighbour's last"""
    assert H.rle_tokens(b"a" * 10, 4) == [97, (3, 1), (4, 1), 97, 97]
    assert H.rle_tokens(b"a" * 10, 4, prev=97) == [(4, 1), (4, 1), 97, 97]
    assert H.rle_tokens(b"ab" + b"b" * 6, 4, prev=98) == [97, 98, 98, 98, (4, 1)]
    assert H.rle_tokens(b"x" * 520, 1024, prev=ord("x")) == [(258, 1), (258, 1), (4, 1)]
    assert H.rle_tokens(b"x" * 519, 1024, prev=ord("x")) == [(258, 1), (258, 1), (3, 1)]
    assert H.rle_tokens(b"x" * 518, 1024, prev=ord("x")) == [(258, 1), (258, 1), 120, 120]


def _built_histograms(O):
    """(name, literal/length histogram, distance histogram, n) of every built input"""
    out = []
    for name, data in I.huffman_only_inputs():
        out.append((name,) + H.token_hist(H.literal_tokens(data)) + (len(data),))
    d = I.rle_all_symbols()
    out.append(("rle_all_symbols",) + H.token_hist(H.rle_tokens(d, 1 << O.seg_shift(len(d), 0))) + (len(d),))
    lad = I.distance_ladder()
    for level in (1, 6):
        h = [int(x) for x in O.deflate_unit(lad, b"", level, 0, debug=True)[2]["hist"]]
        out.append(("ladder_L%d" % level, h[:286], h[288:318], len(lad)))
    return out


def test_properties_of_built_histograms(O):
    """Kraft sum exactly 1, no length above the limit, a more frequent symbol never longer, cost >= the package-merge optimum.
    The gap to the optimum is printed (`pytest -s`), not asserted: DESIGN.md's 0.08 % is a statement about text."""
    rows = []
    for name, hl, hd, n in _built_histograms(O):
        P = H.plan(hl, hd, n)
        hl = list(hl)
        hl[256] = 1
        clf = [0] * 19
        for s, _ in P.cl_tokens:
            clf[s] += 1
        gaps = []
        for freq, lens, limit in ((hl, P.dyn_ll_lens, 10), (_forced(hd), P.dyn_d_lens, 9), (clf, P.cl_lens, 7)):
            used = [s for s in range(len(freq)) if freq[s]]
            assert all(lens[s] == 0 for s in range(len(freq)) if not freq[s]), name
            if len(used) >= 2:
                assert sum(1 << (limit - lens[s]) for s in used) == 1 << limit, (name, limit)
            assert max(lens) <= limit
            # freq[a] > freq[b] implies len[a] <= len[b]: the longest code of a count against the shortest of the next lower count
            counts = sorted({freq[s] for s in used})
            longest = {c: max(lens[s] for s in used if freq[s] == c) for c in counts}
            shortest = {c: min(lens[s] for s in used if freq[s] == c) for c in counts}
            for lo, hi in zip(counts, counts[1:]):
                assert longest[hi] <= shortest[lo], (name, limit, lo, hi)
            cost, opt = H.cost_of(freq, lens), H.optimal_cost(freq, limit)
            assert cost >= opt, (name, limit, cost, opt)
            gaps.append(100.0 * (cost - opt) / opt)
        rows.append("%-22s depth %2d %2d %2d  gap to optimum %.3f %% / %.3f %% / %.3f %%" % ((name, P.depth_ll, P.depth_d, P.depth_cl) + tuple(gaps)))
    print("\n".join(rows))


def test_optimal_cost_is_the_optimum():
    """package-merge against brute force over all length multisets of small alphabets, and against Huffman where no limit binds"""
    import itertools
    rng = random.Random(3)
    for _ in range(40):
        m, limit = rng.randint(2, 6), rng.randint(3, 4)
        freq = sorted(rng.choice((1, 1, 2, 3, 5, 8, 40, 100)) for _ in range(m))
        best = min(sum(f * l for f, l in zip(freq, sorted(ls, reverse=True)))
                   for ls in itertools.product(range(1, limit + 1), repeat=m) if sum(1 << (limit - l) for l in ls) <= 1 << limit)
        assert H.optimal_cost(freq, limit) == best, (freq, limit)
    for _ in range(20):
        freq = [rng.randint(1, 50) for _ in range(rng.randint(2, 40))]
        lens, depth = H.spec_lengths_depth(freq, 15)
        if depth <= 15:
            assert H.cost_of(freq, lens) == H.optimal_cost(freq, 15)


def test_reach_of_built_inputs(O):
    """every input reaches the branch it was built for; a condition that does not hold fails"""
    hists = {name: (hl, hd, n) for name, hl, hd, n in _built_histograms(O)}
    for name, which in I.FOLDS.items():
        P = H.plan(*hists[name])
        assert P.btype == 2, name                      # (the header is really written)
        if which == "ll":
            assert P.depth_ll > 10, (name, P.depth_ll)
        else:
            assert P.depth_cl > 7, (name, P.depth_cl)
    assert 16 <= H.plan(*hists["pow2_depth17"]).depth_ll <= 17
    assert 17 <= H.plan(*hists["geometric255"]).depth_ll <= 19
    for level in (1, 6):
        hl, hd, n = hists["ladder_L%d" % level]
        P = H.plan(hl, hd, n)
        assert all(hd) and P.depth_d > 9 and P.btype == 2, (level, hd, P.depth_d)
    P = H.plan(*hists["cl_deep_zero_runs"])
    assert {17, 18} <= {s for s, _ in P.cl_tokens}
    hl, hd, n = hists["rle_all_symbols"]
    assert all(hl) and len(hl) == 286
    assert sum(1 for f in hists["one_value_m2"][0] if f) == 2 and sum(1 for f in hists["two_values_m3"][0] if f) == 3
    for m in (63, 64, 65, 127, 128, 129, 255, 256, 257):
        for where in ("low", "high", "scattered"):
            assert sum(1 for f in hists["m%d_%s" % (m, where)][0] if f) == m
    # the Z_RLE run layouts: which unit carries which case (a unit with fewer segment ends than cases carries the first ones)
    edge = {"ends_at", "starts_1", "starts_2", "starts_3", "spans"}
    carried = {}
    for name, data, flags in I.rle_sized_units(O.seg_shift):
        carried[(name, flags)] = I.rle_edge_cases(data, 1 << O.seg_shift(len(data), flags))
    for (name, flags), got in carried.items():
        n = int(name[1:name.index("_")])
        if n >= 40000:
            assert got == edge | {"518_one_end"}, (name, flags, got)       # segments of 1024 / 2048: 518 bytes reach one end
        elif n >= 700 and not flags:
            assert edge <= got, (name, got)
    assert "518_two_ends" in carried[("n3000_seg64", 0)] and "518_two_ends" in carried[("n10000_seg256", 0)]
    assert {1 << O.seg_shift(len(d), f) for _, d, f in I.rle_sized_units(O.seg_shift)} == {32, 64, 256, 1024, 2048}


def test_block_type_sweeps(O):
    """all three block types occur in the default sweep, stored and fixed in the Z_FIXED sweep (it never takes dynamic), and the
    kept sizes include exact ties of the two cheapest forms"""
    S = I.sweeps(O)
    for flat in (False, True):                      # (the flat header has a cost, and so change points, of its own)
        seen = {False: set(), True: set()}
        ties = 0
        for (k, fixed, fl), (sizes, kinds) in S.items():
            if fl != flat:
                continue
            seen[fixed] |= {kinds[n][0] for n in sizes}
            ties += sum(1 for n in sizes if kinds[n][1])
            for n in I.sweep_changes(kinds):
                assert {n - 1, n} <= set(sizes)
            for n in sizes:                         # the shared choice rule against plan()'s own Z_FIXED path
                st = I.sweep_stream(k)
                h = [int(x) for x in O.deflate_unit(st[:n], b"", I.SWEEP_LEVEL, 2 if flat else 0, debug=True)[2]["hist"]]
                assert H.plan(h[:286], h[288:318], n, flat=flat, fixed_only=fixed).btype == kinds[n][0]
        assert seen[False] == {0, 1, 2} and seen[True] == {0, 1}, (flat, seen)
        assert ties > 0

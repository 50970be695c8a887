"""The encoder's plan and pack stages (za_k_plan, za_k_pack) and the search-free parse (za_k_parse_rle) on BUILT histograms and
run layouts (tests/plan_inputs.py), against the plain reference of DESIGN.md 3.4 / 3.7 (tests/huffman_ref.py, anchored on the CPU by
tests/test_cpu_entropy_plan.py) -- not against the oracle, which states the same algorithm in the same form as the kernels.

Per unit: the fetched histogram (debug_fetch 4) equals the histogram of the tokens walked from the stream (and, under
Z_HUFFMAN_ONLY / Z_RLE, of the reference's tokens); the walked tokens equal the reference's; the reference's plan of the FETCHED
histogram gives the kernel's block type and header bits (debug_fetch 7) and its lengths and codes (debug_fetch 5, both halves of
every word); the walked block's lengths, HLIT / HDIST / HCLEN, code-length lengths, header size and end-of-block offset equal the
plan's, the stream's length its size, and the stream's BYTES the reference packer's; zlib inflates it, and the CRC is the unit's.

debug_fetch refused no stage these checks use (4, 5 and 7 come from buffers every call fills; stage 2, the token words, is not
used: the tokens are walked from the stream).  Two things about debug_fetch(5): the words of the symbols 286, 287 and of the
distance symbols 30, 31 carry a length (0, or the fixed code's) but no code that means anything, so the code halves are compared
over the alphabets' 286 + 30 symbols; and the plan kernel leaves the DYNAMIC code in the buffer when it picks a stored block, which
is compared too (an input of 256 equal counts is always stored, and the tie order of its lengths would go unseen otherwise)."""
import zlib

import numpy as np
import pytest

import deflate_walk as W
import huffman_ref as H
import plan_inputs as I

pytestmark = pytest.mark.gpu

HUFFMAN_ONLY, RLE, FIXED = zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED
FORMS = [0, 1, 2, 3]                       # flags ORed onto every unit: none, FINAL, flat header, flat header + FINAL


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    oracle.lib()
    return oracle


def _layout(units):
    """units: [(name, data, zdict, flags, align or None)] -> (buffer, blocks): every unit's dictionary directly in front of it, its
    first byte at an offset that is `align` modulo 16 (the engine keeps the call's buffer at an aligned device address)"""
    buf = bytearray()
    blocks = []
    for name, data, zd, flags, align in units:
        p = len(buf) + len(zd)
        if align is not None:
            p += (align - p) % 16
        buf += b"\xee" * (p - len(zd) - len(buf)) + zd + data
        blocks.append((p, len(data), len(zd), flags))
    return bytes(buf), blocks


def _check_call(ctx, O, units, strategy, level, form=0, ref_tokens=None, expect_btype=None):
    """one deflate_blocks call over `units` (+ the joined call), every unit checked as the module's docstring says"""
    from zlib_ng_amd import _lib
    units = [(name, data, zd, flags | form, align) for name, data, zd, flags, align in units]
    buf, blocks = _layout(units)
    assert ctx.L.zngamd_count_units(*_lib.block_table(blocks)) == len(units)           # one unit per block: debug_fetch's index
    cap = max(len(u[1]) for u in units) + max(len(u[1]) for u in units) // 8 + 1024
    joined, jcrcs, jovf, jlens = ctx.deflate_blocks(buf, blocks, level, cap, joined=True, strategy=strategy)
    outs, crcs, ovf = ctx.deflate_blocks(buf, blocks, level, cap, strategy=strategy)
    assert not ovf and not jovf
    # the joined call's packer writes every unit at the offset its PLANNED size gives it, and checks the packed size against it
    assert bytes(joined) == b"".join(outs) and jcrcs == crcs and jlens == [len(o) for o in outs]
    seen = set()
    for i, ((name, data, zd, flags, align), out, crc) in enumerate(zip(units, outs, crcs)):
        n, final, flat = len(data), bool(flags & 1), bool(flags & 2)
        tag = (name, align, len(zd), flags)
        d = zlib.decompressobj(-15, zdict=zd) if zd else zlib.decompressobj(-15)
        assert d.decompress(out) == data and d.eof == final and crc == zlib.crc32(data), tag
        hist = np.frombuffer(ctx.debug_fetch(4, i, 4 * 320), np.uint32).tolist()
        hl, hd = hist[:286], hist[288:318]
        assert hist[286:288] == [0, 0] and hist[318:320] == [0, 0] and hl[256] == 1, tag
        tokens = None
        if ref_tokens is not None:
            tokens = ref_tokens(data, n, flags, zd)
            assert (hl, hd) == H.token_hist(tokens), tag
        # (the pure-Python walker is the slow part: behind the first form, a unit of more than 16 KiB whose tokens the reference
        # knows is judged by its bytes alone -- equal to the reference packer's, they hold the same header and the same tokens)
        walked = not (form and tokens is not None and n > 16384)
        if walked:
            w = W.walk(out, window=zd)
            assert w.out == data and w.final == final, tag
            blk = w.blocks[0]
        if walked and blk.btype != 0:
            assert (hl, hd) == H.token_hist(w.tokens), tag
            assert W.check_strategy(w, strategy) is None, tag
            if tokens is not None:
                assert w.tokens == tokens, (tag, _first_diff(w.tokens, tokens))
            tokens = w.tokens
        P = H.plan(hl, hd, n, final=final, flat=flat, fixed_only=strategy == FIXED)
        if expect_btype is not None:
            assert P.btype == expect_btype[i], tag
        seen.add(P.btype)
        plan = np.frombuffer(ctx.debug_fetch(7, i, 16), np.uint32).tolist()
        assert plan[0] == P.btype, (tag, plan, P.cost_dyn, P.cost_fix, P.cost_sto)
        assert plan[1] == P.header_bits, (tag, plan, P.header_bits)
        words = np.frombuffer(ctx.debug_fetch(5, i, 4 * 320), np.uint32)
        lens, codes = (words >> 16).tolist(), (words & 0xFFFF).tolist()
        if P.btype == 1:
            assert lens == H.FIXED_LL + H.FIXED_D, tag
            assert codes[:286] == P.ll_codes[:286] and codes[288:318] == P.d_codes[:30], tag
        else:
            assert lens == P.dyn_ll_lens + [0, 0] + P.dyn_d_lens + [0, 0], (tag, _first_diff(lens, P.dyn_ll_lens + [0, 0] + P.dyn_d_lens + [0, 0]))
            assert codes[:286] == H.canonical_codes(P.dyn_ll_lens) and codes[288:318] == H.canonical_codes(P.dyn_d_lens), tag
        # the walked stream against the plan
        assert len(out) == P.size, (tag, plan, len(out), P.size)
        if walked:
            assert blk.btype == P.btype, (tag, blk.btype, P.btype)
        if walked and P.btype:
            assert blk.final == final and len(w.blocks) == (1 if final else 2), tag
            assert blk.header_bits == P.header_bits and blk.eob_bit == P.eob_bit, (tag, blk.header_bits, P.header_bits, blk.eob_bit, P.eob_bit)
        if walked and P.btype == 2:
            assert (blk.hlit, blk.hdist) == (P.hlit, P.hdist), tag
            assert blk.ll_lens == P.ll_lens[:P.hlit] and blk.d_lens == P.d_lens[:P.hdist], tag
            if flat:
                assert blk.hclen == 19 and blk.cl_lens == [4] * 16 + [0] * 3, tag
                assert P.header_bits == 74 + 4 * (P.hlit + P.hdist), tag
            else:
                assert blk.hclen == P.hclen and blk.cl_lens == P.cl_lens, (tag, blk.hclen, P.hclen, blk.cl_lens, P.cl_lens)
        if tokens is not None or P.btype == 0:
            assert out == H.emit(P, tokens, data, final=final, flat=flat), tag
    return seen


def _first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return i, a[max(0, i - 3):i + 4], b[max(0, i - 3):i + 4]
    return min(len(a), len(b)), len(a), len(b)


def _literal_ref(data, n, flags, zd):
    return H.literal_tokens(data)


def _rle_ref(O):
    memo = {}                                       # (the same unit comes at sixteen alignments: its reference once)

    def ref(data, n, flags, zd):
        key = (data, O.seg_shift(n, flags), zd[-1:])
        if key not in memo:
            memo[key] = H.rle_tokens(data, 1 << key[1], zd[-1] if zd else None)
        return memo[key]
    return ref


@pytest.mark.parametrize("form", FORMS)
def test_huffman_only_built_histograms(ctx, O, form):
    """every built literal histogram: m = 2 and 3, the deepest trees, ties decided by index alone, the strides' edges at 64/65,
    128/129, 256/257 symbols, and the two inputs that push the code-length code past its limit of 7"""
    units = [(name, data, b"", 0, None) for name, data in I.huffman_only_inputs()]
    seen = _check_call(ctx, O, units, HUFFMAN_ONLY, 6, form, ref_tokens=_literal_ref)
    assert 2 in seen


@pytest.mark.parametrize("form", FORMS)
def test_rle_all_symbols_and_sizes(ctx, O, form):
    """Z_RLE: all 286 literal/length symbols in one unit; runs at, in front of and across segment ends at every segment size"""
    units = [("rle_all_symbols", I.rle_all_symbols(), b"", 0, None)]
    units += [(name, data, b"", flags, None) for name, data, flags in I.rle_sized_units(O.seg_shift)]
    units += [(name, data, b"", flags, None) for name, data, flags in I.rle_small_units()]
    _check_call(ctx, O, units, RLE, 6, form, ref_tokens=_rle_ref(O))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_dict", [False, True], ids=["nodict", "dict100"])
def test_rle_alignments(ctx, O, with_dict, form):
    """Every Z_RLE token input with its first byte at every offset modulo 16 (the kernel's rows start at the aligned 16-byte
    piece), with and without a 100-byte dictionary whose last byte is the unit's first"""
    units = []
    for name, data, flags in I.rle_sized_units(O.seg_shift) + I.rle_small_units():
        zd = (bytes((7 * i) % 3 for i in range(99)) + data[:1]) if with_dict else b""
        units += [(name, data, zd, flags, a) for a in range(16)]
    _check_call(ctx, O, units, RLE, 1, form, ref_tokens=_rle_ref(O))


@pytest.mark.parametrize("form", FORMS)
def test_huffman_only_alignments(ctx, O, form):
    """the same rows without the run logic: literal words only, every alignment, lengths on each side of multiples of 64"""
    units = []
    for name, data, flags in I.rle_small_units():
        units += [(name, data, b"", flags, a) for a in range(16)]
    _check_call(ctx, O, units, HUFFMAN_ONLY, 1, form, ref_tokens=_literal_ref)


@pytest.mark.parametrize("level", [1, 6])
def test_distance_ladder(ctx, O, level):
    """The distance alphabet through za_lengths_small with its limit of 9: the histogram is the GPU's own (cross-checked against
    the walked tokens), and it must make the distance tree deeper than 9 before limiting -- whatever matches the search chose."""
    lad = I.distance_ladder()
    units = [("ladder", lad, b"", 0, None), ("ladder_dict", lad[32768:], lad[:32768], 0, None)]
    for form in FORMS:
        _check_call(ctx, O, units[:1] if form else units, 0, level, form)
    hist = np.frombuffer(ctx.debug_fetch(4, 0, 4 * 320), np.uint32).tolist()
    P = H.plan(hist[:286], hist[288:318], len(lad), final=True, flat=True)
    assert P.depth_d > 9 and P.btype == 2 and all(hist[288:318]), (P.depth_d, hist[288:318])


@pytest.mark.parametrize("strategy", [0, FIXED], ids=["default", "fixed"])
def test_block_type_sweeps(ctx, O, strategy):
    """k distinct byte values drawn uniformly, the sizes at which the reference says the block type changes, their neighbours,
    and the sizes with an exact tie of costs (stored before fixed before dynamic); under Z_FIXED never dynamic, stored only
    where it beats both.  The flat header costs 74 + 4 x (HLIT + HDIST) bits, so the choice changes at other sizes: forms 2
    and 3 run the sizes of a sweep of their own (and every form runs the other header's sizes too)."""
    S = I.sweeps(O)
    for form in FORMS:
        flat = bool(form & 2)
        units, expect = [], []
        for k in I.SWEEP_K:
            kinds = S[(k, strategy == FIXED, flat)][1]
            st = I.sweep_stream(k)
            for n in sorted(set(S[(k, strategy == FIXED, flat)][0]) | {m for m in S[(k, strategy == FIXED, not flat)][0] if m in kinds}):
                units.append(("k%d_n%d" % (k, n), st[:n], b"", 0, None))
                expect.append(kinds[n][0])
        seen = _check_call(ctx, O, units, strategy, I.SWEEP_LEVEL, form, expect_btype=expect)
        assert seen == ({0, 1} if strategy == FIXED else {0, 1, 2}), (form, seen)

"""The output bound of a unit against the referee, before any entry point is judged by it
(tests/test_gpu_expansion_bounds.py): the bound is stated in tests/expansion_inputs.py from RFC 1951 and DESIGN.md, its match half
proved here by exhaustion; the referee stays under it on every worst-case input at every level, strategy and finality; the inputs
built to expand do expand past n + 32 bytes a unit -- what the batch API's bounds allowed before they knew the strategy --; the
referee's final units inflate to their input; and batch._frame_bound is the sum of the units' bounds.  No GPU."""
import zlib

import pytest

import expansion_inputs as X
import huffman_ref as H
import search_ref as S


def test_a_match_never_costs_more_than_nine_bits_a_byte():
    """every length 3 .. 258 with every distance code, under the fixed code's lengths (RFC 1951 3.2.5, 3.2.6)"""
    worst = 0
    for length in range(3, 259):
        lc = H.len_code(length)
        for dc in range(30):
            bits = H.FIXED_LL[257 + lc] + H.LEN_EXTRA[lc] + H.FIXED_D[dc] + H.DIST_EXTRA[dc]
            assert bits <= 9 * length, (length, dc, bits)
            worst = max(worst, bits / length)
    assert worst == 25 / 3                       # (7 + 5 + 13 bits for three bytes: the bound's 9 is a literal's, from 144 up)
    assert max(H.FIXED_LL[:256]) == 9 and H.FIXED_LL[256] == 7


def test_bound_is_the_format():
    """the tests' bound at the sizes where its terms change"""
    assert [X.unit_bound(0, s, True) for s in X.STRATEGIES] == [2] * 5 and [X.unit_bound(0, s, False) for s in X.STRATEGIES] == [5] * 5
    assert X.unit_bound(65535, X.DEFAULT, True) == 65535 + 5 and X.unit_bound(65536, X.DEFAULT, True) == 65536 + 10
    assert X.unit_bound(131072, X.DEFAULT, False) == 131072 + 15 + 5
    # Z_FIXED: ceil((3 + 9 n + 7 + 3) / 8) + 4 behind a unit that is not the last, and 9 n / 8 overtakes n + 32 at 256
    for n in X.SIZES[1:]:
        assert X.unit_bound(n, X.FIXED, False) == -(-(3 + 9 * n + 7 + 3) // 8) + 4
        assert X.unit_bound(n, X.FIXED, True) == -(-(3 + 9 * n + 7) // 8)
    assert 9 * 256 // 8 == 256 + 32 and X.unit_bound(257, X.FIXED, True) > 257 + 32
    assert X.unit_plan(0) == [(0, 0)] and X.unit_plan(131073) == [(0, 131072), (131072, 1)]
    assert X.unit_plan(16385, X.SMALL_UNIT) == [(0, 16384), (16384, 1)]
    assert X.bound(2 * 131072 + 1, X.FIXED, True) == 2 * X.unit_bound(131072, X.FIXED, False) + X.unit_bound(1, X.FIXED, True)


def test_inputs_are_what_they_are_named_for():
    for n in (1024, 131072):
        assert set(X.high64(n)) <= set(range(144, 208)) and set(X.high112(n)) <= set(range(144, 256))
        lh = X.low_then_high(n)
        assert set(lh[:n // 2]) <= set(range(64)) and set(lh[n // 2:]) <= set(range(144, 208))
    assert len(set(X.high64(4096))) == 64 and len(set(X.high112(4096))) == 112 and len(set(X.noise(16384))) == 256
    for make in (X.high64, X.high112, X.noise, X.low_then_high, X.text):
        assert [len(make(n)) for n in X.SIZES] == list(X.SIZES) and make(1024) == make(1024)
    mix = X.unit_mix()
    assert len(mix) == 3 * X.UNIT and len(zlib.compress(X.text(X.UNIT), 6)) < X.UNIT // 3


def test_shared_search_is_the_referees_encode():
    """expansion_inputs runs the search once for all strategies: the same tokens and bytes as search_ref.encode"""
    for name, n in (("high64", 1024), ("low_then_high", 16385), ("noise", 257)):
        data = X.INPUTS[name].make(n)
        for level in X.LEVELS:
            for strategy in (X.DEFAULT, X.FILTERED, X.FIXED):
                for final in (False, True):
                    R = S.encode(data, 0, n, level, 1 if final else 0, 32768, strategy)
                    u = X.unit_ref(data, 0, level, strategy)
                    assert u.tokens == R.parse.tokens and u.size(final) == R.plan.size and u.out(final) == R.out


def _inflate(stream, zdict=b""):
    d = zlib.decompressobj(-15, zdict=zdict) if zdict else zlib.decompressobj(-15)
    out = d.decompress(stream)
    assert d.eof and not d.unused_data
    return out


def _check(name, n, data, level, emit):
    inp = X.INPUTS.get(name)
    for strategy in X.STRATEGIES:
        units = X.block_ref(data, level, strategy)
        plan = X.unit_plan(n)
        assert [len(u.data) for u in units] == [ln for _, ln in plan]
        for final in (False, True):
            for k, u in enumerate(units):
                fin = final and k == len(units) - 1
                tag = (name, n, level, X.STRATEGY_NAMES[strategy], "final" if fin else "not final", k)
                ln = len(u.data)
                size = u.size(fin)
                assert size <= X.unit_bound(ln, strategy, fin), (tag, size)
                if not ln:
                    continue
                P = u.plan(fin)
                if strategy == X.FIXED:
                    assert P.btype != 2, tag
                if inp is not None and inp.stored_from is not None and ln >= inp.stored_from:
                    assert P.btype == 0 and size == H.stored_size(ln, fin), tag
                if inp is not None and inp.expands_from is not None and strategy == X.FIXED and ln >= inp.expands_from and \
                        (name != "low_then_high" or len(units) == 1):
                    # dynamic beats stored, stored beats fixed, the unit is a fixed block larger than n + 32
                    assert P.cost_dyn < P.cost_sto < P.cost_fix and P.btype == 1, (tag, P.cost_dyn, P.cost_sto, P.cost_fix)
                    assert size > ln + 32, (tag, size)
        if emit:
            assert _inflate(X.block_bytes(data, level, strategy, final=True)) == data, (name, n, level, strategy)


@pytest.mark.parametrize("level", X.LEVELS)
@pytest.mark.parametrize("name", list(X.INPUTS))
def test_referee_under_the_bound(name, level):
    """every size x strategy x finality; the final units' bytes through CPython's zlib (the packing of a unit is a Python loop
    over its tokens: sizes above 16 385 are packed at level 6 alone)"""
    for _, n, data in X.cases([name]):
        _check(name, n, data, level, emit=n <= 16385 or level == 6)


@pytest.mark.parametrize("level", X.LEVELS)
def test_unit_mix(level):
    """three units in one block of which only the first expands: fixed and larger than its bytes, stored, and small"""
    data = X.unit_mix()
    _check("unit_mix", len(data), data, level, emit=level == 6)
    a, b, c = X.block_ref(data, level, X.FIXED)
    assert a.plan(False).btype == 1 and a.size(False) > X.UNIT + X.UNIT // 9
    assert b.plan(False).btype == 0 and b.size(False) == H.stored_size(X.UNIT, False)
    assert c.size(True) < X.UNIT // 2
    # (the call's bound is a sum: the third unit's savings pay for the first unit's growth, and only a bound per unit shows it)
    assert sum(X.block_sizes(data, level, X.FIXED)) < len(data)


def test_figures_of_the_bound():
    """the sizes the bound was found on: all literals, 257 bytes make 291 (295 when not final) and 1 024 make 1 154 (1 158); a
    chance repeat of three bytes (two are expected in 1 024 draws from 64 values) saves a bit or two each"""
    assert (X.unit_bound(257, X.FIXED, True), X.unit_bound(257, X.FIXED, False)) == (291, 295)
    assert (X.unit_bound(1024, X.FIXED, True), X.unit_bound(1024, X.FIXED, False)) == (1154, 1158)
    for level in X.LEVELS:
        for n, final, most in ((257, True, 291), (257, False, 295), (1024, True, 1154), (1024, False, 1158)):
            assert most - 4 <= X.unit_ref(X.high64(n), 0, level, X.FIXED).size(final) <= most, (level, n, final)
        # a batch of ONE such item is past the whole call's bound of 64 + n + 32: what makes the GPU tests fail on such a bound
        assert X.unit_ref(X.high64(1024), 0, level, X.FIXED).size(True) > 64 + 1024 + 32
    for level in X.LEVELS:
        for usize in (X.UNIT, X.SMALL_UNIT):
            sizes = X.block_sizes(X.high64(16384), level, X.FIXED, usize=usize)
            assert len(sizes) == 1 and 16384 + 32 < sizes[0] <= 18464


def test_frame_bound_is_the_sum_of_the_unit_bounds():
    """batch._frame_bound against the formula of the engine's unit_bound -- n + 32, and n / 8 more under Z_FIXED -- over the size
    list, unit by unit; and it covers the tests' bound and the referee's worst item"""
    from zlib_ng_amd import batch
    for wbits, ovh, ovh_dict in ((15, 6, 10), (-15, 0, 0), (31, 18, None)):
        for strategy in X.STRATEGIES:
            for n in X.SIZES:
                units = X.unit_plan(n, X.batch_unit_size(n))
                formula = sum(ln + (ln // 8 if strategy == X.FIXED else 0) + 32 for _, ln in units)
                assert batch._frame_bound([n], wbits, None, strategy) == 64 + formula + ovh, (wbits, strategy, n)
                if ovh_dict is not None:
                    assert batch._frame_bound([n], wbits, b"d", strategy) == 64 + formula + ovh_dict
                assert formula >= X.bound(n, strategy, True, X.batch_unit_size(n))
                assert formula >= X.bound(n, strategy, True, X.UNIT)              # (with a dictionary: units of 128 KiB)
            lens = list(X.SIZES)
            assert batch._frame_bound(lens, wbits, None, strategy) == 64 + sum(batch._frame_bound([n], wbits, None, strategy) - 64 for n in lens)
    # the default is the default strategy, as before the bound knew any
    assert batch._frame_bound([1024, 200000], 15) == batch._frame_bound([1024, 200000], 15, None, X.DEFAULT) == 64 + 1024 + 32 + 200000 + 64 + 12
    worst = X.unit_ref(X.high64(1024), 0, 6, X.FIXED).size(True)
    assert batch._frame_bound([1024], -15, None, X.FIXED) >= worst > batch._frame_bound([1024], -15, None, X.DEFAULT)

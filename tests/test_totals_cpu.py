"""tests/totals_ref.py -- the exact-arithmetic statement of the fixed-point collision totals that tests/test_totals_gpu.py
holds the device to -- against its own invariants.  No device call."""
import math
import random
from fractions import Fraction

import pytest

import totals_ref as tr


def _random_values(rng, n, e, span):
    return [rng.choice((-1.0, 1.0)) * math.ldexp(rng.uniform(0.5, 1.0), e - rng.randrange(0, span)) for _ in range(n)]


@pytest.mark.parametrize("e", [-70, -3, 0, 1, 37, 90])
@pytest.mark.parametrize("n", [1, 2, 32, 1024])
def test_value_is_the_exact_sum_to_the_low_words_rounding(e, n):
    """every low word is rounded once, by at most half of 2^-40 of 2^(e - 52): |value - sum v| <= n 2^(e - 93)"""
    rng = random.Random(1000 * n + e)
    v = _random_values(rng, n, e, 100)
    H, L, bad = tr.words(v, e)
    assert not bad
    exact = sum(Fraction(x) for x in v)
    assert abs(tr.value(H, L, e) - exact) <= n * Fraction(2) ** (e - 93)


@pytest.mark.parametrize("e", [-70, 0, 37])
@pytest.mark.parametrize("n", [1, 32, 1024])
def test_value_is_exact_on_the_grid(e, n):
    """values that are multiples of 2^(e - 92) lose nothing at all"""
    rng = random.Random(7 * n + e)
    v = [math.ldexp(rng.randrange(-(1 << 53), 1 << 53), e - 92 + rng.randrange(0, 40)) for _ in range(n)]
    H, L, bad = tr.words(v, e)
    assert not bad
    assert tr.value(H, L, e) == sum(Fraction(x) for x in v)


def test_split_rounds_halves_to_even_and_knows_its_range():
    assert tr.split(math.ldexp(2.5, -52), 0) == (2, 1 << 39)            # t = 2.5: the high word goes to the even 2, the rest is exactly half a unit
    assert tr.split(math.ldexp(3.5, -52), 0) == (4, -(1 << 39))
    assert tr.split(math.ldexp(1.5, -92), 0) == (0, 2) and tr.split(math.ldexp(2.5, -92), 0) == (0, 2) and tr.split(math.ldexp(-0.5, -92), 0) == (0, 0)
    assert tr.split(1.0 - 2.0 ** -53, 0) == (1 << 52, -(1 << 39))       # 2^e - 1 ulp: t = 2^52 - 1/2
    assert tr.split(math.ldexp(1.0, 10), 0) is None and tr.split(math.ldexp(-1.0, 10), 0) is None          # |t| = 2^62
    assert tr.split(math.ldexp(1.0, 10) * (1 - 2.0 ** -53), 0) is not None
    assert tr.split(math.inf, 0) is None and tr.split(math.nan, 0) is None
    assert tr.split(0.0, 5) == (0, 0) and tr.split(-0.0, 5) == (0, 0) and tr.split(5e-324, -60) == (0, 0)


def test_exponent_rules():
    # ceil((ilogb(area) + 1) / 2) for even, odd and negative exponents: sqrt(area) < 2^that
    for k in range(-81, 122):
        a = math.ldexp(1.0, k)
        kc = min(max(k, -80), 120)
        half = tr.force_exp(0, a, 1.0) - 1
        assert half == math.ceil((kc + 1) / 2)
        if -80 <= k <= 120:
            assert Fraction(a) < Fraction(4) ** half                      # sqrt(area) < 2^half, up to the next power of two
            assert Fraction(math.nextafter(a, math.inf)) < Fraction(4) ** half
    assert tr.force_exp(3, 1.0, 1.0) == 3 + 0 + 1 + 1
    assert tr.force_exp(0, 1.0, math.nextafter(1.0, 0.0)) == 0 - 1 + 1 + 1
    assert tr.force_exp(0, 1.0, 2.0 ** 50) == 40 + 1 + 1 and tr.force_exp(0, 1.0, 2.0 ** -50) == -40 + 1 + 1
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert tr.ilogb(bad, -40, 60) == -40
    assert tr.ilogb(5e-324, -2000, 0) == -1074
    assert tr.lever_exp(1.0) == 1 and tr.lever_exp(2.0 ** 70) == 61 and tr.area_exp(3.0) == 2 and tr.area_exp(0.3) == -1
    assert tr.force_scale_exp(6e6, 0.2) == 23 and tr.force_scale_exp(2.0 ** 20, 0.0) == 21 and tr.force_scale_exp(2.0 ** 20, -0.5) == 21
    assert tr.force_scale_exp(0.0, 0.2) == 1 and tr.force_scale_exp(math.inf, 0.2) == 1


def test_row_words_order():
    row = [3.0, -5.0, 12.0, 20.0, 7.0]
    w = tr.row_words(row, -1.0, 10.0, 17.0, 3, 4, 2)
    unit = lambda e: 1 << (52 - e)
    assert [h for h, _ in w] == [-3 * unit(3), 5 * unit(3), 2 * -3 * unit(5), 3 * -3 * unit(5), 2 * 5 * unit(5), 3 * 5 * unit(5), 7 * unit(4)]
    assert all(l == 0 for _, l in w)

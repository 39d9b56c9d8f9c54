"""The fixed-point collision totals in exact arithmetic, from the rules of DESIGN.md section 0.2 (not from the device code): Python integers
and fractions.Fraction, exponents by math.frexp.

    ilogb(x)        the binary exponent of x (2^ilogb <= |x| < 2^(ilogb + 1)), clamped to [lo, hi]; lo for anything that is not a positive finite
                    number (0, negative, inf, NaN)
    kexp            ilogb((1 + max(mu, 0)) E) + 1, the product formed in double; 1 when it is not in (0, 1e300)
    e_F             kexp + ilogb(height; -40, 40) + 1 + ceil((ilogb(area; -80, 120) + 1) / 2)
    e_L             ilogb(rmax; -40, 60) + 1;  e_T = e_F + e_L          (torque and stress products)
    e_O             ilogb(area; -80, 120) + 1                           (overlap areas)
    split           t = v 2^(52 - e);  hi = round_half_even(t);  lo = round_half_even((t - hi) 2^40);  |t| >= 2^62, inf, NaN: out of range, adds nothing
    words           the integer sums of hi and of lo
    value           (sum hi 2^40 + sum lo) 2^(e - 92), exactly; the double read from it is that number rounded to nearest even
"""
import math
from fractions import Fraction

H_CLAMP, AREA_CLAMP, RMAX_CLAMP = (-40, 40), (-80, 120), (-40, 60)
HEADROOM = 1 << 62


def ilogb(x, lo, hi):
    if not (x > 0.0 and x < math.inf):          # (NaN compares false)
        return lo
    return min(max(math.frexp(x)[1] - 1, lo), hi)          # frexp: x = m 2^e, 0.5 <= m < 1 -- subnormals included


def force_scale_exp(E, mu):
    b = (1.0 + max(mu, 0.0)) * E
    return (math.frexp(b)[1] - 1 if 0.0 < b < 1e300 else 0) + 1


def ceil_half(a):
    return -((-a) // 2)


def force_exp(kexp, area, height):
    return kexp + ilogb(height, *H_CLAMP) + 1 + ceil_half(ilogb(area, *AREA_CLAMP) + 1)


def lever_exp(rmax):
    return ilogb(rmax, *RMAX_CLAMP) + 1


def area_exp(area):
    return ilogb(area, *AREA_CLAMP) + 1


def round_half_even(q):
    return round(Fraction(q))          # (Fraction.__round__ rounds halves to even)


def split(v, e):
    """(hi, lo) of one double at exponent e, or None when it is out of range"""
    if v != v or v in (math.inf, -math.inf):
        return None
    t = Fraction(v) * Fraction(2) ** (52 - e)
    if abs(t) >= HEADROOM:
        return None
    hi = round_half_even(t)
    return hi, round_half_even((t - hi) * (1 << 40))


def words(vals, e):
    """(sum hi, sum lo, bad) of the values at exponent e"""
    H = L = 0; bad = 0
    for v in vals:
        s = split(float(v), e)
        if s is None:
            bad = 1
        else:
            H += s[0]; L += s[1]
    return H, L, bad


def value(H, L, e):
    """the exact number a pair of word sums stands for"""
    return Fraction((H << 40) + L) * Fraction(2) ** (e - 92)


def to_double(q):
    """q rounded to the nearest double, ties to even (int / int true division is correctly rounded)"""
    q = Fraction(q)
    return q.numerator / q.denominator


def folded_high(H, L):
    """the integer part the reader forms before it converts to double: floor((H 2^40 + L) / 2^40)"""
    return H + (L >> 40)          # (Python's >> is a floor for negative integers too)


def row_words(row5, sign, cx, cy, eF, eA, eL):
    """the seven (hi, lo) one interaction row {fx, fy, px, py, overlap} adds to a floe with centroid (cx, cy): 0 fx, 1 fy, 2 (x-cx) fx, 3 (y-cy) fx,
    4 (x-cx) fy, 5 (y-cy) fy, 6 overlap.  Levers and products are formed in double, as the rows' own torque column is (collisions.jl:673-686)."""
    fx, fy, px, py, ov = (float(x) for x in row5)
    fx *= sign; fy *= sign
    lx, ly = px - cx, py - cy
    vals = [(fx, eF), (fy, eF), (lx * fx, eF + eL), (ly * fx, eF + eL), (lx * fy, eF + eL), (ly * fy, eF + eL), (ov, eA)]
    return [split(v, e) for v, e in vals]

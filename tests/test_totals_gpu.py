"""The fixed-point collision totals (csrc/sz_geom.hpp fx_*) held to exact sums.

Part A: the device's own fx_force_exp / fx_lever_exp / fx_area_exp / fx_split / fx_join / fx_word, reached through sz_debug_fx_totals and
sz_debug_fx_word, against tests/totals_ref.py (integers and fractions): words equal as integers, the value read equal to the correctly rounded
exact value, the exponents equal, the range flag raised exactly where the rules say.

Part B: one resident step of small worlds that sit at the edges of the scales.  The reference of the summation is the exact rational sum of the
interaction rows the device itself emitted (the rows are the input of the operation under test); every world is also held to the oracle at the
suite's 1e-10, and the three-launch and the pipelined driver to each other bit for bit.

Tolerances (u = 2^-53, half an ulp relative; e the exponent of the word by totals_ref; n the number of rows):
  * a low word is rounded once, by at most half of 2^(e - 92): n rows are off by at most n 2^(e - 93) together;
  * the value read is rounded once more: + ulp(total) / 2.  Forces, overlap:  |total - sum rows| <= ulp(total) / 2 + n 2^(e - 93);
  * torque = (sum of n products) - (sum of n products), subtracted as integers: 2 n words;
  * a stress component is join * 1 / (area * height) (s12: a sum of 2 n words, halved exactly): the join, the product area * height, the
    reciprocal and the last product round once each -- four relative errors of at most u compound to less than 4.5 u -- so
    |s - S / (area height)| <= 4.5 u |s| + words 2^(e_T - 93) / (area height) (1 + 2^-40).
"""
import math
import os
import struct
from fractions import Fraction

import numpy as np
import pytest

import cases
import parity
import totals_ref as tr

pytestmark = pytest.mark.gpu

TWO = Fraction(2)


def mk(**env):
    """a context created with the switches of env in the environment (they are read at sz_create)"""
    import subzero_jl_amd
    os.environ.update(env)
    try:
        return subzero_jl_amd.World(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def dev():
    return mk()


def bits(x):
    return struct.pack("<d", x)


# ===================================================================================== part A: the arithmetic
NS = [1, 2, 32, 1024]
SETS = ["random", "ties", "low-ties", "near-bound", "integer-t", "big-tiny-big", "all-negative", "at-bound", "zeros", "subnormal"]


def value_set(name, n, e, seed=0):
    """n doubles for exponent e whose word sums fit an int64 (partial sums may wrap: the atomics add mod 2^64)"""
    rng = np.random.default_rng([seed, n, e % 1000, SETS.index(name)])
    ld = lambda m, k: math.ldexp(float(m), int(k))
    if name == "random":          # signs and magnitudes from 2^e down to 2^(e - 100)
        return [float(rng.choice((-1.0, 1.0))) * ld(rng.uniform(0.5, 1.0), e - rng.integers(0, 101)) for _ in range(n)]
    if name == "ties":            # t = k + 1/2: the high word goes to the even neighbour, the remainder is exactly +-1/2
        return [ld(2 * int(rng.integers(-(1 << 40), 1 << 40)) + 1, e - 53) for _ in range(n)]
    if name == "low-ties":        # t = k + (j + 1/2) 2^-40: the LOW word sits on a tie (k < 2^11: t has 52 bits)
        return [ld((int(rng.integers(-(1 << 10), 1 << 10)) << 41) + 2 * int(rng.integers(0, 1 << 40)) + 1, e - 93) for _ in range(n)]
    if name == "near-bound":      # +-(2^e - 1 ulp): t = 2^52 - 1/2
        return [float(rng.choice((-1.0, 1.0))) * math.nextafter(ld(1, e), 0.0) for _ in range(n)]
    if name == "integer-t":       # |t| >= 2^52: t is an integer, the remainder zero; signs alternate so that the sum stays inside an int64
        top = 3 if n <= 32 else 0
        return [(-1.0) ** k * ld((1 << 52) + int(rng.integers(0, 1 << 52)), e - 52 + int(rng.integers(0, top + 1))) for k in range(n)]
    if name == "big-tiny-big":
        big = ld(rng.uniform(0.5, 1.0), e)
        tiny = [ld(rng.uniform(0.5, 1.0), e - 95 + int(rng.integers(0, 6))) for _ in range(max(n - 2, 1))]
        return ([big] + tiny + [-big])[:n] if n >= 3 else ([big, -big] if n == 2 else tiny[:1])
    if name == "all-negative":    # t = -(k + d), 0 < d < 1/2: every low word is negative, so is their sum (fx_join's floor)
        out = []
        for _ in range(n):
            if rng.integers(0, 2):
                out.append(-ld((int(rng.integers(0, 1 << 20)) << 32) + int(rng.integers(1, 1 << 31)), e - 84))
            else:
                out.append(-ld((int(rng.integers(0, 1 << 8)) << 45) + int(rng.integers(1, 1 << 44)), e - 97))
        return out
    if name == "at-bound":        # the whole headroom: n times the largest value the bound admits
        return [math.nextafter(ld(1, e), 0.0)] * n
    if name == "zeros":
        return [0.0, -0.0][:n] * max(n // 2, 1)
    if name == "subnormal":       # (used with e = -1030: t = k 2^8)
        return [float(rng.choice((-1.0, 1.0))) * ld(int(rng.integers(1, 1 << 40)), -1074) for _ in range(n)]
    raise KeyError(name)


def check_join(joined, H, L, e):
    """The value read.  fx_join folds the low sum into the high word, H' = H + floor(L / 2^40), and returns (double)H' + (L mod 2^40) 2^-40, scaled by
    a power of two.  While |H'| < 2^53 the conversion is exact and the one addition rounds once: the result must be the correctly rounded exact
    value, bit for bit.  Beyond that (inside the headroom) (double)H' has rounded before the low part is added: two roundings, at most one ulp."""
    exact = tr.value(H, L, e)
    want = tr.to_double(exact)
    if abs(tr.folded_high(H, L)) < (1 << 53):
        assert bits(joined) == bits(want), (joined, want, H, L, e)
    else:
        assert abs(Fraction(joined) - exact) <= Fraction(max(math.ulp(joined), math.ulp(want))), (joined, want, H, L, e)


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("e", [-37, 30])
def test_words_and_value_are_the_references(dev, name, e):
    if name == "subnormal":
        e = -1030 if e < 0 else -1040
    for n in NS:
        v = value_set(name, n, e)
        H, L, bad = tr.words(v, e)
        assert not bad and abs(H) < (1 << 63) and abs(L) < (1 << 63)
        hi, lo, dbad, de, joined = dev.fx_totals(v, e=e, nthreads=min(n, 64))
        assert (hi, lo, dbad, de) == (H, L, 0, e), (name, n, e)
        check_join(joined, H, L, e)
        if name == "all-negative":
            assert L < 0
        if name == "at-bound" and n == 1024:
            assert H == 1 << 62          # ten bits of headroom, all used


def test_words_do_not_depend_on_the_order(dev):
    """the same multiset added by 1, 64 and 1024 threads under three permutations: identical words, identical value"""
    n, e = 1024, 11
    rng = np.random.default_rng(5)
    for name in ("random", "low-ties"):
        v = value_set(name, n, e, seed=1)
        H, L, _ = tr.words(v, e)
        for perm in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
            for nthreads in (1, 64, 1024):
                got = dev.fx_totals(v, e=e, perm=perm, nthreads=nthreads)
                assert got[:4] == (H, L, 0, e), (name, nthreads)
                check_join(got[4], H, L, e)


def _around(k):
    p = math.ldexp(1.0, k)
    return [math.nextafter(p, 0.0), p, math.nextafter(p, math.inf)]


ODD = [0.0, -0.0, -1.0, 5e-324, math.ldexp(1.0, -1030), 1e-300, 1e300, math.inf, -math.inf, math.nan]


def test_exponents_are_the_references(dev):
    """area = 2^k and 2^k +- 1 ulp for even, odd and negative k, across both clamps, and what is no positive finite number; height and rmax likewise"""
    areas = [a for k in (-82, -81, -80, -79, -8, -7, -6, -3, -2, -1, 0, 1, 2, 3, 26, 27, 33, 34, 119, 120, 121, 122) for a in _around(k)] + ODD
    for a in areas:
        for kexp, h in ((23, 1.0), (-5, 0.3)):
            assert dev.fx_totals([], mode=1, e=kexp, area=a, height=h)[3] == tr.force_exp(kexp, a, h), ("force", a, kexp, h)
        assert dev.fx_totals([], mode=3, area=a)[3] == tr.area_exp(a), ("area", a)
    heights = [h for k in (-42, -41, -40, -39, -4, -1, 0, 1, 3, 4, 39, 40, 41, 42) for h in _around(k)] + ODD
    for h in heights:
        for a in (1.0, 2.0 ** 27, 2.0 ** -7):
            assert dev.fx_totals([], mode=1, e=23, area=a, height=h)[3] == tr.force_exp(23, a, h), ("height", h, a)
    rmaxs = [r for k in (-42, -41, -40, -39, -1, 0, 1, 14, 59, 60, 61, 62) for r in _around(k)] + ODD
    for r in rmaxs:
        assert dev.fx_totals([], mode=4, rmax=r)[3] == tr.lever_exp(r), ("rmax", r)
        assert dev.fx_totals([], mode=2, e=23, area=3e7, height=0.7, rmax=r)[3] == tr.force_exp(23, 3e7, 0.7) + tr.lever_exp(r), ("torque", r)


@pytest.mark.parametrize("E, mu", [(6e6, 0.2), (2.0 ** 21, 1.0), (math.nextafter(2.0 ** 21, 0.0), 1.0), (2.0 ** 21, -0.5), (2.0 ** 21, 0.0), (1.5e3 * 3.7e4, 0.2),
                                   (2.0 ** -30, 0.2), (1e-3, 0.7)])
def test_force_scale_exponent_of_the_context(E, mu):
    """kexp from the context's own E and mu: (1 + mu) E just below and at a power of two, and a negative mu (taken as 0)"""
    w = mk()
    w.set_consts(E=E, mu=mu)
    want = tr.force_scale_exp(E, mu)
    assert w.fx_totals([], mode=1 | 8, e=-999, area=1.0, height=1.0)[3] == want + 0 + 1 + 1
    assert w.fx_totals([], mode=1 | 8, e=-999, area=5e7, height=0.25)[3] == tr.force_exp(want, 5e7, 0.25)


def test_range_flag(dev):
    """|t| >= 2^62, inf and NaN raise the flag and add nothing; 2^61 < |t| < 2^62 does not; one value 1000 x over the bound is summed exactly"""
    e = 7
    unit = lambda k: math.ldexp(1.0, e + k)
    good = [unit(-3) * 1.2345, -unit(-60) * 1.7]
    H, L, _ = tr.words(good, e)
    for out in (unit(10), -unit(10), unit(11) * 1.3, math.inf, -math.inf, math.nan, 1e300):
        hi, lo, bad, _, joined = dev.fx_totals(good + [out], e=e, nthreads=3)
        assert (hi, lo, bad) == (H, L, 1), out
        assert tr.words(good + [out], e) == (H, L, 1)
        check_join(joined, H, L, e)
    for ok in (math.nextafter(unit(10), 0.0), -math.nextafter(unit(10), 0.0), unit(9) * 1.5, -unit(9) * 1.0000001):
        hi, lo, bad, _, joined = dev.fx_totals([ok], e=e)
        assert 1 << 61 < abs(hi) < 1 << 62 and (hi, lo, bad) == tr.words([ok], e) == (int(Fraction(ok) * TWO ** (52 - e)), 0, 0), ok
        check_join(joined, hi, lo, e)
    over = 1000.0 * math.nextafter(unit(0), 0.0)
    hi, lo, bad, _, joined = dev.fx_totals([over], e=e)
    assert (hi, lo, bad) == tr.words([over], e) and bad == 0 and tr.value(hi, lo, e) == Fraction(over) and joined == over


def test_row_words_are_the_references(dev):
    """fx_word: word 0 fx, 1 fy, 2 (x-cx) fx, 3 (y-cy) fx, 4 (x-cx) fy, 5 (y-cy) fy, 6 overlap; forces negated for the pair's second floe; levers and
    products formed in double"""
    rng = np.random.default_rng(9)
    rows = [([3.0, -5.0, 12.0, 20.0, 7.0], 10.0, 17.0)]
    for _ in range(6):
        c = rng.uniform(0, 1e5, 2)
        rows.append(([rng.normal() * 1e7, rng.normal() * 1e7, c[0] + rng.normal() * 3e3, c[1] + rng.normal() * 3e3, rng.uniform(1, 1e6)], c[0], c[1]))
    for row, cx, cy in rows:
        for sign in (1.0, -1.0):
            eF, eA, eL = 29, 27, 14
            want = tr.row_words(row, sign, cx, cy, eF, eA, eL)
            hi, lo, bad = dev.fx_word(row, sign, cx, cy, eF, eA, eL)
            assert bad == 0 and list(zip(hi, lo)) == want, (row, sign)
    hi, lo, bad = dev.fx_word([1e30, 1.0, 0.0, 0.0, 1.0], 1.0, 0.0, 0.0, 29, 27, 14)          # a force beyond the headroom: that word adds nothing
    assert bad == 1 and hi[0] == 0 and lo[0] == 0 and hi[1] == 1 << 23 and hi[6] == 1 << 25


# ===================================================================================== part B: the totals of a real step
MU = 0.2
sq = lambda x0, y0, s, t=None: np.array([[x0, y0], [x0, y0 + (t or s)], [x0 + s, y0 + (t or s)], [x0 + s, y0], [x0, y0]], float)      # (clockwise, as the fields')
KINDS = {"open": [0, 0, 0, 0], "periodic": [1, 1, 1, 1], "collision": [2, 2, 2, 2]}


class Case:
    """a small world: rings, heights, velocities, domain -- built the same way into a HIP context and into the oracle"""
    def __init__(self, rings, heights, u=None, v=None, kinds="open", L=1e5, E=1e3, dt=10, topo=None, columns=None, hflx=0.0, settings=None, ghosts=False,
                 steps=2):
        self.rings = rings; self.heights = np.broadcast_to(np.asarray(heights, float), (len(rings),)); self.kinds = kinds; self.L = L; self.E = E
        self.dt = dt; self.u = np.zeros(len(rings)) if u is None else np.asarray(u, float); self.v = np.zeros(len(rings)) if v is None else np.asarray(v, float)
        self.topo = topo; self.columns = columns or {}; self.hflx = hflx; self.settings = settings or {}; self.ghosts = ghosts; self.steps = steps
        self.coupling = hflx != 0.0

    def build(self, w):
        from subzero_jl_amd import fields
        w.set_consts(E=self.E, mu=MU); w.set_settings(**self.settings)
        w.set_domain(KINDS[self.kinds], 0.0, self.L, 0.0, self.L)
        if self.topo:
            w.set_topography(self.topo)
        w.set_grid_fields(10, 10, 0.0, self.L, 0.0, self.L, 0.0, 0.0, self.hflx, 0.0, 0.0)
        for i, (r, h) in enumerate(zip(self.rings, self.heights)):
            w.add_floe(r, h)
            if self.coupling:
                c = r[:-1].mean(0)
                w.set_subpoints(i, *fields.subgrid_points(r, c[0], c[1], 0.25 * (r[:, 0].max() - r[:, 0].min())))
        w.set("u", self.u); w.set("v", self.v)
        for k, val in self.columns.items():
            w.set(k, val)
        return w

    def oracle(self, hw):
        """the oracle on the same numbers: built the same way, then given the HIP world's columns bit for bit"""
        from oracle import orc
        ow = self.build(orc.World())
        for f in orc.FIELDS:
            ow.set(f, hw.get(f))
        return ow

    def run(self, w, n, t):
        return w.run(n, t, self.dt, coupling_dt=1, coupling_on=self.coupling)


PRE = ("cx", "cy", "area", "height", "rmax", "overarea")


def exact_sum_check(w, pre, E, ghosts):
    """the totals of the step w has just taken against the exact sum of the rows it emitted (module docstring); pre: the columns before the step.
    Returns the rows per floe."""
    kexp = tr.force_scale_exp(E, MU)
    off, rows = w.interactions()
    tot = {k: w.get(k) for k in ("coll_fx", "coll_fy", "coll_trq", "overarea", "si11", "si12", "si21", "si22")}
    N = len(pre["cx"])
    F = lambda a: sum((Fraction(float(x)) for x in a), Fraction(0))
    for i in range(N):
        r = rows[off[i]:off[i + 1]]; n = len(r)
        area, h, rmax = (float(pre[k][i]) for k in ("area", "height", "rmax"))
        eF = tr.force_exp(kexp, area, h); eT = eF + tr.lever_exp(rmax); eO = tr.area_exp(area)
        for name, col in (("coll_fx", cases.FX), ("coll_fy", cases.FY)):
            got = float(tot[name][i])
            tol = Fraction(math.ulp(got)) / 2 + n * TWO ** (eF - 93)
            err = abs(Fraction(got) - F(r[:, col]))
            print(f"floe {i} {name}: rows {n} e {eF} |err| {float(err):.3e} tol {float(tol):.3e}")
            assert err <= tol, (i, name, got, float(err), float(tol))
        # overarea accumulates: the column before the step + the step's total (one more rounding when the column was not zero)
        got = float(tot["overarea"][i]); before = float(pre["overarea"][i]); s = F(r[:, cases.OVER])
        tol = Fraction(math.ulp(got)) / 2 + (Fraction(math.ulp(float(s))) / 2 if before != 0.0 else 0) + n * TWO ** (eO - 93)
        err = abs(Fraction(got) - Fraction(before) - s)
        print(f"floe {i} overarea: rows {n} e {eO} |err| {float(err):.3e} tol {float(tol):.3e}")
        assert err <= tol, (i, "overarea", got, float(err), float(tol))
        if ghosts:
            continue
        lx = r[:, cases.PX] - pre["cx"][i]; ly = r[:, cases.PY] - pre["cy"][i]          # (numpy float64: one rounding per lever, one per product)
        fx, fy = r[:, cases.FX], r[:, cases.FY]
        w2, w3, w4, w5 = F(lx * fx), F(ly * fx), F(lx * fy), F(ly * fy)
        got = float(tot["coll_trq"][i])
        tol = Fraction(math.ulp(got)) / 2 + 2 * n * TWO ** (eT - 93)
        err = abs(Fraction(got) - (w4 - w3))
        print(f"floe {i} coll_trq: rows {n} e {eT} |err| {float(err):.3e} tol {float(tol):.3e}")
        assert err <= tol, (i, "coll_trq", got, float(err), float(tol))
        sc = 1 / (Fraction(area) * Fraction(h))
        for name, S, nw in (("si11", w2, n), ("si12", (w3 + w4) / 2, 2 * n), ("si21", (w3 + w4) / 2, 2 * n), ("si22", w5, n)):
            got = float(tot[name][i])
            tol = Fraction(9, 2) * TWO ** -53 * abs(Fraction(got)) + nw * TWO ** (eT - 93) * sc * (1 + TWO ** -40)
            err = abs(Fraction(got) - S * sc)
            print(f"floe {i} {name}: rows {n} e {eT} |err| {float(err):.3e} tol {float(tol):.3e}")
            assert err <= tol, (i, name, got, float(err), float(tol))
        if n == 0:
            assert all(float(tot[k][i]) == 0.0 for k in ("coll_fx", "coll_fy", "coll_trq", "si11", "si12", "si21", "si22"))
    return np.diff(off[:N + 1])


def assert_bit_equal(a, b):
    for f in parity.SCALARS:
        assert np.array_equal(a.get(f), b.get(f)), f
    assert np.array_equal(a.rings()[1], b.rings()[1]) and np.array_equal(a.rings()[2], b.rings()[2])
    ia, ib = a.interactions(), b.interactions()
    assert np.array_equal(ia[0], ib[0]) and np.array_equal(ia[1], ib[1])
    assert np.array_equal(a.ids()[2], b.ids()[2])


def run_case(case):
    """One resident step from a fresh upload on the three-launch driver (SZ_PIPELINE=0), held to the exact sums of its rows and to the oracle; a second
    step from the state it left (another set of rows: the floes have moved, heights above the clamp have been cut), held to both again; then the same
    steps as ONE batch of the pipelined driver (which takes no batch shorter than two steps), bit for bit the three-launch state -- the totals
    of its first step are in the velocities the second one starts from.  Returns (three-launch world, rows per floe of the first step)."""
    a = case.build(mk(SZ_PIPELINE="0"))
    ow = case.oracle(a)
    nrows = None
    for t in range(case.steps):
        pre = {k: a.get(k) for k in PRE}
        assert case.run(a, 1, t) == 1
        assert a.totals_mode() == 2 and not a.pipelined()          # the fixed-point totals, not process mode's serial sums
        ow.timestep_sim(t, case.dt, coupling_dt=1, coupling_on=case.coupling)
        assert np.all(a.ids()[2] == cases.ACTIVE)
        n = exact_sum_check(a, pre, case.E, case.ghosts)
        parity.compare_worlds(a, ow, rtol=1e-10)
        nrows = n if nrows is None else nrows
    b = case.build(mk(SZ_PIPE_MIN_STEPS="2"))
    assert case.run(b, case.steps, 0) == case.steps
    assert b.pipelined() and b.totals_mode() == 2
    assert_bit_equal(a, b)
    return a, nrows


def test_size_ratio():
    """a floe of 1e3 m^2 indenting one of 1e10 m^2: scales 23 binary orders apart in one pair; one row, so the two forces are equal and opposite
    to the bit"""
    case = Case([sq(1e5, 1e5, 1e5), sq(2e5 - 10.0, 1.5e5, 32.0)], 0.5, u=[0.0, -0.05], v=[0.0, 0.03], L=4e5)
    a, nrows = run_case(case)
    assert list(nrows) == [1, 1]
    assert a.get("area")[0] / a.get("area")[1] > 9e6
    fx, fy = a.get("coll_fx"), a.get("coll_fy")
    assert fx[0] != 0.0 and bits(fx[0]) == bits(-fx[1]) and bits(fy[0]) == bits(-fy[1])


@pytest.mark.parametrize("heights", [(2.0 ** -4, 16.0), (20.0, 12.0)], ids=["thin-thick", "above-max-height"])
def test_heights(heights):
    """2^-4 m against 16 m (beyond max_floe_height = 10 as well); 20 m and 12 m: the update clamps both to 10 m -- another exponent for the first --
    while the narrow phase formed its scale from the column as it was: the reader must use the height before the clamp"""
    case = Case([sq(4.0e4, 4.5e4, 1e4), sq(4.95e4, 4.6e4, 1e4)], heights, u=[0.3, -0.3])
    a, nrows = run_case(case)
    assert list(nrows) == [1, 1] and np.all(a.get("height") <= 10.0)


def test_height_through_a_power_of_two_inside_a_batch():
    """the heat flux takes a height from above 1/2 m to below it between the steps of one 3-step batch: the narrow phase (collision record) and the
    update (column) of the step after the crossing must form the same exponent.  Held to the oracle, and the two drivers to each other."""
    case = Case([sq(4.0e4, 4.5e4, 1e4), sq(4.95e4, 4.6e4, 1e4)], (0.5015, 0.7), u=[0.3, -0.3], hflx=5e-4, steps=3)
    ow = None
    worlds = []
    for env in ({"SZ_PIPELINE": "0"}, {"SZ_PIPE_MIN_STEPS": "2"}):
        w = case.build(mk(**env))
        ow = ow or case.oracle(w)
        assert case.run(w, 3, 0) == 3 and w.totals_mode() == 2
        worlds.append(w)
    assert not worlds[0].pipelined() and worlds[1].pipelined()
    heights = [0.5015]
    for t in range(3):
        ow.timestep_sim(t, case.dt, coupling_dt=1, coupling_on=True)
        heights.append(float(ow.get("height")[0]))
    assert heights[0] > heights[1] > 0.5 > heights[2] > heights[3], heights          # the third step reads a height in the next binade down
    assert len(worlds[0].interactions()[1]) == 2
    parity.compare_worlds(worlds[0], ow, rtol=1e-10)
    assert_bit_equal(worlds[0], worlds[1])


def test_areas_beside_a_power_of_two():
    """areas one ulp either side of 2^26 (even) and 2^27 (odd): the contributor and the reader must take the same side"""
    rings = [sq(2.0e4, 2.0e4, 8192.0), sq(2.0e4 + 8192.0 - 300.0, 2.1e4, 8192.0),
             sq(6.0e4, 6.0e4, 8192.0, 16384.0), sq(6.0e4 + 8192.0 - 300.0, 6.1e4, 8192.0, 16384.0)]
    areas = [math.nextafter(2.0 ** 26, 0.0), 2.0 ** 26, math.nextafter(2.0 ** 27, 0.0), math.nextafter(2.0 ** 27, math.inf)]
    case = Case(rings, 0.5, u=[0.2, -0.2, 0.2, -0.2], columns={"area": areas})
    a, nrows = run_case(case)
    assert list(nrows) == [1, 1, 1, 1]


def test_lengths_in_kilometres():
    """the same kind of contact with lengths in km and E rescaled: heights of 5e-4 (exponent -11), velocities of 1e-4.  The floes are 100 km
    across: the reference drops contact regions smaller than 100 n / 1.75 square units (collisions.jl:160-166, a constant in m^2), so a floe
    whose area is below one unit can never have a row -- area exponents below zero are reached through part A only."""
    case = Case([sq(400.0, 450.0, 100.0), sq(495.0, 460.0, 100.0)], 5e-4, u=[3e-4, -3e-4], L=1000.0, E=1e6)
    a, nrows = run_case(case)
    assert list(nrows) == [1, 1]
    assert tr.ilogb(float(a.get("height")[0]), -40, 40) == -11


def hub_case():
    """one long floe with 14 staple-shaped floes along its two long edges, each reaching into it with two prongs: two contact regions, two rows
    per pair -- 28 rows on the hub from 14 neighbours (more neighbours than 22 would move the field to the wider lists: 128 rows per floe, and
    no pipelined steps).  Depths and drifts differ from floe to floe: nothing in the hub's totals cancels by symmetry."""
    def staple(x0, edge, d, up):          # body 3 km x 2.7 km beyond the edge, two 1 km prongs reaching d into the hub
        s = 1.0 if up else -1.0
        r = [(0.0, -d), (0.0, 3e3), (3e3, 3e3), (3e3, -d), (2e3, -d), (2e3, 300.0), (1e3, 300.0), (1e3, -d), (0.0, -d)]
        r = r if up else r[::-1]          # (mirrored: reversed, so that the ring stays clockwise)
        return np.array([[x0 + x, edge + s * y] for x, y in r])
    top = [staple(2.2e4 + k * 8e3, 5.5e4, 300.0 + 20.0 * k, True) for k in range(7)]
    bottom = [staple(2.2e4 + k * 8e3, 4.5e4, 200.0 + 10.0 * k, False) for k in range(7)]
    rings = top + [sq(2.0e4, 4.5e4, 6e4, 1e4)] + bottom
    u = [0.05 + 0.01 * k for k in range(7)] + [0.0] + [0.02 * k - 0.1 for k in range(7)]
    v = [-0.1] * 7 + [0.0] + [0.1] * 7
    return Case(rings, 0.5, u=u, v=v)


HUB = 7


def test_hub():
    """28 rows on one floe's words (the stride of the rows is 32); n of the bound is that count"""
    a, nrows = run_case(hub_case())
    assert nrows[HUB] == 28 and np.all(np.delete(nrows, HUB) == 2)


def ghost_case():
    """doubly periodic: a parent in the south-west corner (three ghosts) with one contact on itself and one on each ghost"""
    L = 1e5
    rings = [sq(-2e3, -2e3, 1e4), sq(7.5e3, 0.0, 5e3), sq(9.35e4, 1e3, 5e3), sq(1e3, 9.35e4, 5e3), sq(9.35e4, 9.35e4, 5e3)]
    return Case(rings, 0.5, u=[0.0, -0.1, 0.1, 0.0, 0.1], v=[0.0, 0.0, 0.0, 0.1, 0.1], kinds="periodic", L=L, ghosts=True)


def test_ghost_fold():
    """the words of four instances of one floe added at ONE scale.  Forces and overlap of every parent are exact sums of its rows (a ghost that
    split at another exponent would be off by a factor of two or more); torque and stress against the oracle.  The ghosts the library makes of the
    parent carry its area, height and rmax to the bit."""
    case = ghost_case()
    a, nrows = run_case(case)
    assert nrows[0] == 4 and list(nrows[1:]) == [1, 1, 1, 1]
    g = case.build(mk())
    g.add_ghosts()
    gl = g.ghosts()[0]
    assert len(gl) == 3 and g.M == 8
    for k in ("area", "height", "rmax"):
        col = g.get(k)
        assert all(bits(col[j]) == bits(col[0]) for j in gl), k


def test_walls_and_topography():
    """floe-wall and floe-topography rows (no second floe): the totals of the floe alone"""
    topo = [sq(4.8e4, 4.8e4, 4e3)]
    rings = [sq(-300.0, 2.0e4, 1e4), sq(4.0e4, 4.6e4, 8.3e3), sq(7.0e4, 1e5 - 9.8e3, 1e4)]
    case = Case(rings, 0.5, u=[-0.1, 0.1, 0.0], v=[0.0, 0.0, 0.1], kinds="collision", topo=topo)
    a, nrows = run_case(case)
    assert list(nrows) == [1, 1, 1]
    off, rows = a.interactions()
    assert np.all(rows[:, cases.IDX] < 0)


def _columns(w):
    ia = w.interactions()
    return {f: w.get(f) for f in parity.SCALARS}, ia[0].copy(), ia[1].copy(), w.ids()[2].copy()


def _same(x, y):
    return all(np.array_equal(x[0][f], y[0][f]) for f in x[0]) and all(np.array_equal(p, q) for p, q in zip(x[1:], y[1:]))


@pytest.mark.parametrize("env", [{"SZ_PIPELINE": "0"}, {}], ids=["three-launch", "pipelined"])
@pytest.mark.parametrize("ending", ["tag-stop", "one-step"])
def test_no_leftovers_between_batches(env, ending):
    """a batch that ended on a tag stop (its later steps were enqueued and returned at once) and a 1-step batch leave nothing in the words: the
    same state uploaded again into the same context gives the same bits"""
    if ending == "tag-stop":          # two floes closing in until their overlap passes floe_floe_max_overlap: the fuse tag ends the batch
        case = Case([sq(4.0e4, 4.5e4, 1e4), sq(4.41e4, 4.6e4, 1e4), sq(8.0e4, 1.0e4, 1e4), sq(9.6e4, 6.0e4, 1e4)], 0.5, u=[3.0, -3.0, 0.0, 0.0], kinds="periodic")
        nsteps = 12
    else:
        case = hub_case(); nsteps = 1
    w = case.build(mk(**env))
    w._push()
    cols0 = {k: np.copy(v) for k, v in w.col.items()}
    runs = []
    for _ in range(2):
        done = case.run(w, nsteps, 0)
        assert w.totals_mode() == 2
        runs.append((done, w.pipelined(), _columns(w)))
        w.load_columns(cols0)
    assert runs[0][0] == runs[1][0] and _same(runs[0][2], runs[1][2])
    if ending == "tag-stop":
        assert 2 <= runs[0][0] < 12 and np.any(runs[0][2][3] == cases.FUSE) and runs[0][1] == (not env)
        assert np.all(runs[0][2][0]["overarea"][:2] > 0.0)          # (the steps before the tag had rows; the tag step itself has none)
    else:
        assert np.all(runs[0][2][0]["coll_fy"] != 0.0)


@pytest.mark.parametrize("env", [{"SZ_PIPELINE": "0"}, {"SZ_PIPE_MIN_STEPS": "2"}], ids=["three-launch", "pipelined"])
def test_no_leftovers_after_a_contact(env):
    """a step in which a floe has contacts, then a step in which it has none: totals of exactly zero, the overlap area untouched"""
    case = Case([sq(4.0e4, 4.5e4, 1e4), sq(4.99e4, 4.6e4, 1e4)], 0.5, u=[-50.0, 50.0])
    w = case.build(mk(**env))
    if env.get("SZ_PIPELINE") == "0":
        assert case.run(w, 1, 0) == 1
        assert np.all(w.get("coll_fx") != 0.0) and len(w.interactions()[1]) == 2
        over = w.get("overarea")
        assert np.all(over > 0.0)
        assert case.run(w, 1, 1) == 1 and not w.pipelined()
    else:
        assert case.run(w, 2, 0) == 2 and w.pipelined()
        over = w.get("overarea")
        assert np.all(over > 0.0)
    assert w.totals_mode() == 2 and len(w.interactions()[1]) == 0
    for k in ("coll_fx", "coll_fy", "coll_trq", "si11", "si12", "si21", "si22"):
        assert np.all(w.get(k) == 0.0), k
    assert np.array_equal(w.get("overarea"), over)


@pytest.mark.parametrize("env, nsteps", [({"SZ_PIPELINE": "0"}, 1), ({"SZ_PIPE_MIN_STEPS": "2"}, 2)], ids=["three-launch", "pipelined"])
def test_range_error_is_returned(env, nsteps):
    """a floe whose area column is 1e-8 of its ring's area, in contact (floe_floe_max_overlap raised so that the contact is not a fuse): its overlap
    is 3e6 times the bound its words were scaled for -- beyond the ten bits of headroom.  The kernel raises ERR_FIXED_RANGE and adds nothing;
    the run must come back with the library's error status naming it, not with totals."""
    from subzero_jl_amd.capi import SzError
    case = Case([sq(4.0e4, 4.5e4, 1e4), sq(4.7e4, 4.6e4, 1e4)], 0.5, u=[0.3, -0.3], columns={"area": [1e8 * 1e-8, 1e8]},
                settings=dict(floe_floe_max_overlap=1e12))
    w = case.build(mk(**env))
    with pytest.raises(SzError) as err:
        case.run(w, nsteps, 0)
    assert "0x8000" in str(err.value) and "fixed-point-range=32768" in str(err.value), str(err.value)

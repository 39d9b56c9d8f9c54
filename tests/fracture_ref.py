"""determine_fractures (Subzero.jl src/physical_processes/fractures.jl:269-280) restated in numpy: the yardstick of the device's
fracture criterion (csrc/sz_fracture.hpp), itself pinned by tests/golden/fractures.json (the reference's own test values)."""
import json
import math
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fractures.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def julia_range_0_2pi(n=100):
    """the points of range(0, 2π, length = n): k (2π) / (n - 1), each rounded once"""
    two_pi = Fraction(2 * math.pi)
    return np.array([float(two_pi * k / (n - 1)) for k in range(n)])


def calculate_hibler(mean_height, pstar, c):
    """_calculate_hibler (fractures.jl:83-94) with _move_poly (floe_utils.jl:74-80): closed ring (px, py) of 100 points"""
    p = pstar * mean_height * math.exp(-c * (1 - 1))
    a = p * math.sqrt(2) / 2
    b = a / 2
    al = julia_range_0_2pi(100)
    x0 = a * np.cos(al); y0 = b * np.sin(al)
    x0[-1] = x0[0]; y0[-1] = y0[0]
    rc, rs = math.cos(math.pi / 4), math.sin(math.pi / 4)
    x1 = rc * x0 + (-rs) * y0; y1 = rs * x0 + rc * y0
    return x1 + (-p / 2), y1 + (-p / 2), p


def calculate_mohrs(q=5.2, sigma_c=2.5e5, sigma11=-3.375e4):
    """_calculate_mohrs (fractures.jl:170-214): the closed triangle in principal-stress space"""
    s1 = ((1 / q) + 1) * sigma_c / ((1 / q) - q)
    s2 = q * s1 + sigma_c
    s22 = q * sigma11 + sigma_c
    pts = [(-s1, -s2), (-sigma11, -s22), (-s22, -sigma11), (-s1, -s2)]
    return np.array([p[0] for p in pts]), np.array([p[1] for p in pts])


def ring_area_centroid(x, y):
    cr = x[:-1] * y[1:] - x[1:] * y[:-1]
    A = cr.sum() / 2
    return abs(A), ((x[:-1] + x[1:]) * cr).sum() / (6 * A), ((y[:-1] + y[1:]) * cr).sum() / (6 * A)


def principal_stresses(sa):
    """eigvals of the symmetric stress_accum rows (11, 12, 21, 22), ascending"""
    s11, s12, s22 = sa[:, 0], 0.5 * (sa[:, 1] + sa[:, 2]), sa[:, 3]
    m = 0.5 * (s11 + s22); h = 0.5 * (s11 - s22)
    r = np.sqrt(h * h + s12 * s12)
    return m - r, m + r


def covered(px, py, x, y):
    """GO.coveredby of the points (x, y) by the closed ring (px, py): inside (crossing rule) or on an edge"""
    x = np.asarray(x, float); y = np.asarray(y, float)
    inside = np.zeros(x.shape, bool); on = np.zeros(x.shape, bool)
    for k in range(len(px) - 1):
        x1, y1, x2, y2 = px[k], py[k], px[k + 1], py[k + 1]
        cr = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1)
        on |= (cr == 0) & (x >= min(x1, x2)) & (x <= max(x1, x2)) & (y >= min(y1, y2)) & (y <= max(y1, y2))
        straddle = (y1 > y) != (y2 > y)
        with np.errstate(divide="ignore", invalid="ignore"):
            xi = x1 + (y - y1) * (x2 - x1) / (y2 - y1)
        inside ^= straddle & (x < xi)
    return inside | on


def boundary_distance(px, py, x, y):
    """distance of each point to the ring's edges"""
    x = np.asarray(x, float); y = np.asarray(y, float)
    d = np.full(x.shape, np.inf)
    for k in range(len(px) - 1):
        ax, ay, bx, by = px[k], py[k], px[k + 1], py[k + 1]
        ex, ey = bx - ax, by - ay
        L2 = ex * ex + ey * ey
        t = np.clip(((x - ax) * ex + (y - ay) * ey) / L2, 0.0, 1.0) if L2 > 0 else np.zeros(x.shape)
        d = np.minimum(d, np.hypot(x - (ax + t * ex), y - (ay + t * ey)))
    return d


def sigma_points(sa, area, alpha, min_floe_area):
    lo, hi = principal_stresses(np.asarray(sa, float))
    if alpha != 0:
        m = (np.asarray(area, float) / min_floe_area) ** alpha
        lo = lo * m; hi = hi * m
    return lo, hi


def determine_fractures(sa, area, height, kind, pstar=2.25e5, c=20.0, poly=None, alpha=0.0, min_floe_area=1e6):
    """0-based candidate indices, the polygon and its scale (p for Hibler, |σc|-like scale for a polygon: its largest coordinate).
    kind 1: Hibler from mean(height); kind 2: the fixed polygon poly = (px, py)."""
    if kind == 1:
        px, py, p = calculate_hibler(float(np.mean(height)), pstar, c)
        scale = p
    else:
        px, py = np.asarray(poly[0], float), np.asarray(poly[1], float)
        scale = float(np.max(np.abs(np.concatenate([px, py]))))
    lo, hi = sigma_points(sa, area, alpha, min_floe_area)
    cand = ~covered(px, py, lo, hi) & ~(np.asarray(area) < min_floe_area)
    return np.nonzero(cand)[0], (px, py), scale


def ties(sa, area, poly, scale, alpha, min_floe_area, rel=1e-9):
    """floes whose σ-point lies within rel * scale of the polygon boundary: excluded from device / numpy comparisons"""
    lo, hi = sigma_points(sa, area, alpha, min_floe_area)
    return boundary_distance(poly[0], poly[1], lo, hi) <= rel * scale


def fixture_floes(g=None):
    """the four floes of test_fractures.jl:107-184: (rings, heights, stress_accum rows, areas)"""
    g = g or golden()
    d = g["determine_fractures"]
    fs = np.array(d["frac_stress"])
    rings, hs, sa, area = [], [], [], []
    for f in d["floes"]:
        r = np.array(f["coords"], float)
        rings.append(r); hs.append(f["height"])
        sa.append([fs[0, 0], fs[0, 1], fs[1, 0], fs[1, 1]] if f["stress"] else [0.0] * 4)
        area.append(ring_area_centroid(r[:, 0], r[:, 1])[0])
    return rings, np.array(hs), np.array(sa), np.array(area)


def zero_point_covered_robustly(mean_height, pstar, c=20.0, ulps=4):
    """An unstressed floe's σ-point (0, 0) is the Hibler ring's first vertex up to rounding: whether it is covered depends on the last
    bits of p (in the reference too).  True when it is covered for every mean height within `ulps` ulps of mean_height -- a device mean
    summed in another order then decides the same way."""
    for k in range(-ulps, ulps + 1):
        m = mean_height + k * np.spacing(mean_height)
        px, py, _ = calculate_hibler(m, pstar, c)
        if not covered(px, py, [0.0], [0.0])[0]:
            return False
    return True


def huge_square(s=1e30):
    """a fixed criterion polygon no σ-point leaves: a criterion that is never met"""
    return np.array([-s, s, s, -s, -s]), np.array([-s, -s, s, s, -s])

"""Floes against grid cells where rings touch grid lines, and an exact reference for the areas.

Floe ∩ rectangle areas feed the two-way coupling (sea-ice fraction and stress weights per centre cell: sz_k_tw_area_rect) and all 18 averages
of the GridOutputWriter (sz_k_eul_area_rect; with topography sz_k_eul_area / sz_k_eul_cell_area).  Random fields never put a vertex on a grid
line; grid lines, though, sit on round numbers and on the domain walls, and the candidate filters (closed box comparisons) hand exactly the
touching pairs to the clipper.  FAMILY holds the touching configurations one by one, each on a small grid of which EVERY cell is compared.

The construction.  Cells are GX x GY = 20 km x 40 km; q(a, b) is the point a eighths of a cell east and b eighths north of the grid's corner
(X0, Y0), so grid lines are the multiples of 8 and every coordinate is an integer number of metres: exact in doubles and in Fraction alike.
Where an edge passes through a cell corner it does so at a dyadic parameter (1/2), so the crossing itself is exact in doubles: whether a
ring that meets a cell in one corner point leaves 0.0 there is then a matter of the closed half-planes alone, not of one rounding.

The reference: `exact_clip`, a stored-polygon Sutherland-Hodgman clip in Fraction against the closed rectangle with a shoelace sum.  It shares
nothing with the device's streaming pipeline (RectClip) or the oracle's C (orc_rect_area) or its general trace (orc.clip).  Where a floe
leaves the window in pieces the bridging edges run along the window boundary there and back and cancel exactly.

Capacities of the grid paths are read out of the sources (`capacities`): FC_CAP centre cells per floe, and the working set of the
topography kernel's general clip (EU_CAP ring points, EU_KC crossings, EU_RC region points, EU_RM regions).
"""
import os
import re
from fractions import Fraction as Fr

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "subzero.jl_amd", "csrc")

GX, GY = 20000, 40000
X0, Y0 = -60000, -80000
NX, NY = 6, 4
FAR = 2_000_000          # the offset of the far-away copy of the family


def capacities():
    """{"FC_CAP", "EU_CAP", "EU_KC", "EU_RC", "EU_RM"} parsed from sz_kernels.hpp and sz_output.hpp"""
    out = {}
    for name in ("sz_kernels.hpp", "sz_output.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for stmt in re.findall(r"constexpr int ((?:\s*\w+\s*=\s*\d+\s*,?)+);", text):
            for k, v in re.findall(r"(\w+)\s*=\s*(\d+)", stmt):
                if k in ("FC_CAP", "EU_CAP", "EU_KC", "EU_RC", "EU_RM"):
                    out[k] = int(v)
    assert sorted(out) == ["EU_CAP", "EU_KC", "EU_RC", "EU_RM", "FC_CAP"], out
    return out


# ---------------------------------------------------------------- the exact reference
def exact_clip(ring, x0, x1, y0, y1):
    """closed ring (sequence of integer or Fraction points) against the closed window: dict(area, m, K, P) as Fractions / ints --
    area of ring ∩ window, m points of the clipped polygon, K crossings made over the four stages, P the largest |partial shoelace sum| in
    window-relative coordinates (the last three are what `rect_bound` needs)"""
    pts = [(Fr(x) - x0, Fr(y) - y0) for x, y in ring[:-1]]
    w, h = Fr(x1) - x0, Fr(y1) - y0
    K = 0
    for axis, c, upper in ((0, Fr(0), False), (0, w, True), (1, Fr(0), False), (1, h, True)):
        out = []
        for k in range(len(pts)):
            a, b = pts[k], pts[(k + 1) % len(pts)]
            ia = a[axis] <= c if upper else a[axis] >= c
            ib = b[axis] <= c if upper else b[axis] >= c
            if ia != ib:
                t = (c - a[axis]) / (b[axis] - a[axis])
                out.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
                K += 1
            if ib:
                out.append(b)
        pts = out
    s = Fr(0); P = Fr(0)
    for k in range(len(pts)):
        a, b = pts[k], pts[(k + 1) % len(pts)]
        s += a[0] * b[1] - b[0] * a[1]
        P = max(P, abs(s))
    return dict(area=abs(s) / 2, m=len(pts), K=K, P=P)


def rect_bound(ex, w, h, L):
    """absolute bound on |area in doubles - exact area| for a Sutherland-Hodgman clip against the window [0, w] x [0, h] followed by a
    shoelace sum, both in window-relative coordinates; `ex` is exact_clip's record of the same ring and window, L the largest magnitude of a
    window-relative coordinate (ring points, w and h).  u = 2^-53.

    Inputs.  Ring points and window corner are integers below 2^53, so the subtraction of the corner is exact.
    Crossings.  A crossing lies on its line exactly (the coordinate is set, not computed); the other coordinate is a + t (b - a) with
    t = (c - a') / (b' - a').  Between ring vertices the differences are exact and three roundings remain (quotient, product, sum):
    |t (b - a)| <= 2 L, so 2 u * 2 L + u L = 5 u L.  Where an end point is itself an earlier stage's crossing the two differences round as
    well (4 u L more) and the end point's own 5 u L moves the segment: the computed point is the exact crossing of a segment displaced by
    that much, and what a displaced vertex or segment changes of an area inside the window is its displacement times the window's extent.
    Taken together: every one of the K crossings moves twice the area by at most 10 u L (w + h).
    Shoelace.  The m output points lie in the window, so each product is at most w h: two products and their difference round once each
    (3 u w h per term), the running sum once per term (u P with P the largest partial sum, taken from the exact clip: the partial sums of
    the computed polygon differ from it by the terms above, far below P's own size).
    Twice the area is therefore off by at most u (m (3 w h + max(P, w h)) + 10 K L (w + h)); fused multiply-adds only remove roundings."""
    u = 2.0 ** -53
    w, h, L = float(w), float(h), float(L)
    return 0.5 * u * (ex["m"] * (3.0 * w * h + max(float(ex["P"]), w * h)) + 10.0 * ex["K"] * L * (w + h))


def cell_reference(ring, xg, yg):
    """(exact areas as an (nx, ny) object array of Fractions, bounds as a float array) of one closed ring on the grid"""
    nx, ny = len(xg) - 1, len(yg) - 1
    area = np.empty((nx, ny), object); bound = np.zeros((nx, ny))
    for ix in range(nx):
        for iy in range(ny):
            x0, x1, y0, y1 = xg[ix], xg[ix + 1], yg[iy], yg[iy + 1]
            ex = exact_clip(ring, x0, x1, y0, y1)
            L = max([abs(x - x0) for x, _ in ring] + [abs(y - y0) for _, y in ring] + [x1 - x0, y1 - y0])
            area[ix, iy] = ex["area"]; bound[ix, iy] = rect_bound(ex, x1 - x0, y1 - y0, L)
    return area, bound


def topo_reference(floe, common, topo, xg, yg):
    """with one topography element: (floe's share per cell, bounds, free area per cell) -- share = floe ∩ cell minus (floe ∩ element) ∩ cell
    with `common` = floe ∩ element written down by hand (both are rectangles), free = cell minus element ∩ cell; a cell without free area
    holds nothing"""
    a, b = cell_reference(floe, xg, yg); c, bc = cell_reference(common, xg, yg); t, _ = cell_reference(topo, xg, yg)
    free = np.empty(a.shape, object)
    for ix in range(a.shape[0]):
        for iy in range(a.shape[1]):
            free[ix, iy] = Fr(xg[ix + 1] - xg[ix]) * (yg[iy + 1] - yg[iy]) - t[ix, iy]
            a[ix, iy] = a[ix, iy] - c[ix, iy] if free[ix, iy] > 0 else Fr(0)
    return a, b + bc, free


def ring_area(ring):
    s = Fr(0)
    for (xa, ya), (xb, yb) in zip(ring[:-1], ring[1:]):
        s += Fr(xa) * yb - Fr(xb) * ya
    return abs(s) / 2


def as_array(ring):
    out = np.array([[float(x), float(y)] for x, y in ring])
    assert all(Fr(float(x)) == x and Fr(float(y)) == y for x, y in ring), "the construction must be exact in doubles"
    return out


# ---------------------------------------------------------------- the family
def q(a, b):
    return (X0 + a * GX // 8, Y0 + b * GY // 8)


def lines(lo, hi, origin, step):
    return [origin + k * step for k in range(lo, hi + 1)]


XG, YG = lines(0, NX, X0, GX), lines(0, NY, Y0, GY)
# the cell most cases are about: C = cell (3, 1), eighths 24..32 x 8..16
_DIAMOND_IN = [(24, 12), (28, 14), (30, 12), (28, 6)]          # one vertex on C's west edge from inside, two plain crossings on its south edge
_U = [(25, 2), (25, 12), (27, 12), (27, 6), (29, 6), (29, 12), (31, 12), (31, 2)]          # notch floor below C: two pieces in C
# name: (open ring in eighths, x lines, y lines)
_FAMILY = {
    "vertex-on-edge-inside-crossing": (_DIAMOND_IN, XG, YG),
    "vertex-on-edge-inside":          ([(24, 12), (28, 14), (30, 12), (28, 10)], XG, YG),
    "vertex-on-edge-outside":         ([(16, 12), (20, 14), (24, 12), (20, 10)], XG, YG),
    "vertex-on-corner":               ([(24, 16), (20, 10), (18, 14)], XG, YG),
    "diamond-on-corners":             ([(16, 16), (24, 24), (32, 16), (24, 8)], XG, YG),
    "triangle-corner-to-corner":      ([(16, 8), (16, 24), (32, 8)], XG, YG),
    "edge-on-line-part":              ([(24, 10), (24, 14), (28, 14), (28, 10)], XG, YG),
    "edge-on-line-all":               ([(24, 8), (24, 16), (28, 14), (28, 10)], XG, YG),
    "one-cell":                       ([(24, 8), (24, 16), (32, 16), (32, 8)], XG, YG),
    "two-by-one-cells":               ([(24, 8), (24, 16), (40, 16), (40, 8)], XG, YG),
    "contains-cells":                 ([(12, 4), (12, 28), (44, 28), (44, 4)], XG, YG),
    "inside-one-cell":                ([(26, 10), (26, 14), (30, 14), (30, 10)], XG, YG),
    "u-two-pieces":                   (_U, XG, YG),
    "u-notch-floor-on-line":          ([(25, 2), (25, 12), (27, 12), (27, 8), (29, 8), (29, 12), (31, 12), (31, 2)], XG, YG),
    # no touching here: crossings at sevenths, ninths and fifteenths of their edges, so that the far-away copy has digits to lose
    "skew-crossings":                 ([(22, 5), (29, 19), (37, 10)], XG, YG),
    "box-touches-outer-line":         ([(-4, 12), (-2, 14), (0, 12), (-2, 10)], XG, YG),
    "off-grid":                       ([(-20, 12), (-18, 14), (-16, 12), (-18, 10)], XG, YG),
    "half-off-grid":                  ([(-4, 9), (-4, 15), (4, 15), (4, 9)], XG, YG),
    "grid-1x1-diamond":               (_DIAMOND_IN, XG[3:5], YG[1:3]),
    "grid-1x1-u":                     (_U, XG[3:5], YG[1:3]),
    "grid-1xn-diamond":               (_DIAMOND_IN, XG[3:5], YG),
    "grid-1xn-u":                     (_U, XG[3:5], YG),
    "grid-nx1-diamond":               (_DIAMOND_IN, XG, YG[1:3]),
    "grid-nx1-u":                     (_U, XG, YG[1:3]),
}
FAMILY = tuple(_FAMILY)
ORIENTATIONS = ("cw", "ccw")
NENT_ZERO = ("off-grid",)          # no cell's box meets the ring's: the device makes no entry at all
# hand-written areas (m^2) per cell (ix, iy), every other cell 0: what the exact reference itself is held to
HAND = {
    "diamond-on-corners": {(2, 1): 4e8, (3, 1): 4e8, (2, 2): 4e8, (3, 2): 4e8},
    "u-two-pieces": {(3, 0): 15000 * 20000 + 2 * 5000 * 10000, (3, 1): 2 * 5000 * 20000},
    "u-notch-floor-on-line": {(3, 0): 15000 * 30000, (3, 1): 2 * 5000 * 20000},
    "one-cell": {(3, 1): 8e8},
    "vertex-on-edge-outside": {(2, 1): 2 * 10000 * 10000},
}


def case(name, orient="cw", offset=0):
    """(closed ring as integer points, x lines, y lines) of a family member; "cw" is the reference's orientation (clockwise)"""
    eighths, xg, yg = _FAMILY[name]
    pts = [q(a, b) for a, b in eighths]
    s = sum(xa * yb - xb * ya for (xa, ya), (xb, yb) in zip(pts, pts[1:] + pts[:1]))
    if (s > 0) == (orient == "cw"):          # positive shoelace: counter-clockwise
        pts = pts[::-1]
    pts = [(x + offset, y + offset) for x, y in pts]
    return pts + pts[:1], [x + offset for x in xg], [y + offset for y in yg]


# ---------------------------------------------------------------- many rows: the same small square in M distinct cells of a 12 x 12 grid
ROWS = (1, 63, 64, 65, 129)          # sz_k_eul_entries reserves entries per wavefront of 64 rows
ROWS_N = 12


def rows_world(M):
    """([closed rings], x lines, y lines): square k sits inside cell (k % 12, k // 12), its west edge on the cell's west line"""
    xg, yg = lines(0, ROWS_N, X0, GX), lines(0, ROWS_N, Y0, GY)
    rings = []
    for k in range(M):
        x, y = xg[k % ROWS_N], yg[k // ROWS_N] + GY // 4
        pts = [(x, y), (x, y + GY // 2), (x + GX // 2, y + GY // 2), (x + GX // 2, y)]
        rings.append(pts + pts[:1])
    return rings, xg, yg


# ---------------------------------------------------------------- large rings (the ring points of the topography kernel's general clip)
def polygon_ring(points, R=7000):
    """closed ring of `points` points: a regular polygon of radius R on integer vertices (clockwise), centred on the corner shared by the
    cells (2, 1), (3, 1), (2, 2), (3, 2) of the family's grid: the ring crosses a line of either direction twice"""
    n = points - 1
    cx, cy = q(24, 16)
    pts = [(cx + int(round(R * np.cos(-2 * np.pi * k / n))), cy + int(round(R * np.sin(-2 * np.pi * k / n)))) for k in range(n)]
    assert len(set(pts)) == n
    return pts + pts[:1]


def ring_sizes(caps):
    """closed ring points at, one past and far past EU_CAP (255: the largest ring the package takes)"""
    return (caps["EU_CAP"], caps["EU_CAP"] + 1, 255)


# ---------------------------------------------------------------- topography: one rectangular element
def _rect(a0, b0, a1, b1):
    pts = [q(a0, b0), q(a0, b1), q(a1, b1), q(a1, b0)]
    return pts + pts[:1]


TOPO_AWAY = _rect(60, 8, 64, 12)          # off the grid and off every floe: selects the topography kernels, changes no answer
# name: (floe, element, floe ∩ element), rectangles on the family's grid
TOPO_CASES = {
    "element-covers-part": (_rect(24, 8, 40, 16), _rect(28, 12, 36, 20), _rect(28, 12, 36, 16)),          # parts of four cells, of the floe in two
    "element-covers-cell": (_rect(12, 4, 44, 28), _rect(22, 6, 34, 18), _rect(22, 6, 34, 18)),          # cell (3, 1) wholly: no free area there
}


# an element the large rings run into: the rectangle east of x = centre + 2 km.  floe ∩ element ∩ cell is then the ring in the window
# cell ∩ element, exact by the same reference; on the device that part goes through the general clip in world coordinates, whose round-off
# narrow_edges_cases.exact_bound states (a shoelace over the region's points at the coordinates' own magnitude)
def ring_element():
    cx, cy = q(24, 16)
    pts = [(cx + 2000, cy - 30000), (cx + 2000, cy + 30000), (cx + 30000, cy + 30000), (cx + 30000, cy - 30000)]
    return pts + pts[:1]


def ring_element_reference(ring, xg, yg):
    """(share per cell, bounds, free area per cell) of a ring against ring_element()"""
    from narrow_edges_cases import exact_bound
    el = ring_element()
    ex0, ex1, ey0, ey1 = el[0][0], el[2][0], el[0][1], el[1][1]
    a, b = cell_reference(ring, xg, yg)
    free = np.empty(a.shape, object)
    Lc = max(max(abs(x), abs(y)) for x, y in ring + el)
    for ix in range(a.shape[0]):
        for iy in range(a.shape[1]):
            x0, x1, y0, y1 = max(xg[ix], ex0), min(xg[ix + 1], ex1), max(yg[iy], ey0), min(yg[iy + 1], ey1)
            free[ix, iy] = Fr(xg[ix + 1] - xg[ix]) * (yg[iy + 1] - yg[iy])
            if x0 < x1 and y0 < y1:
                free[ix, iy] -= Fr(x1 - x0) * (y1 - y0)
                ex = exact_clip(ring, x0, x1, y0, y1)
                if ex["area"] > 0:
                    a[ix, iy] -= ex["area"]
                    L = max([abs(x - xg[ix]) for x, _ in ring] + [abs(y - yg[iy]) for _, y in ring] + [xg[ix + 1] - xg[ix], yg[iy + 1] - yg[iy]])
                    b[ix, iy] += rect_bound(ex, x1 - x0, y1 - y0, L) + exact_bound(len(ring) + 4, float(Lc), ex["area"])[0]
    return a, b, free


# ---------------------------------------------------------------- worlds
OUT_VALUES = dict(u=0.3, v=-0.1, p_dudt=1e-3, p_dvdt=-2e-3, overarea=7.0, sa11=3.0, sa12=1.0, sa21=1.0, sa22=-2.0, e11=1e-3, e12=2e-3, e21=2e-3,
                  e22=4e-3)
HEIGHT = 0.5


def output_world(w, rings, xg, yg, topo=None):
    """open boundaries a cell beyond the grid (and the rings), the floes with the columns of the reference's output test"""
    w.set_consts(); w.set_settings()
    every = list(rings) + list(topo or [])
    xs = [x for r in every for x, _ in r] + list(xg); ys = [y for r in every for _, y in r] + list(yg)
    w.set_domain([0, 0, 0, 0], float(min(xs) - GX), float(max(xs) + GX), float(min(ys) - GY), float(max(ys) + GY))
    if topo:
        w.set_topography([as_array(t) for t in topo])
    for r in rings:
        w.add_floe(as_array(r), HEIGHT)
    for name, val in OUT_VALUES.items():
        w.set(name, [val] * len(rings))
    return w


def analytic_outputs(names, area, cell_area, mass_per_area):
    """the 18 grids of ONE floe from its exact areas per cell (float array): the averages are the floe's own values where it has area"""
    occ = (area > 0).astype(float)
    val = dict(u_grid=0.3, v_grid=-0.1, dudt_grid=1e-3, dvdt_grid=-2e-3, overarea_grid=7.0, height_grid=HEIGHT, stress_xx_grid=3.0,
               stress_yx_grid=1.0, stress_xy_grid=1.0, stress_yy_grid=-2.0, strain_ux_grid=1e-3, strain_vx_grid=2e-3, strain_uy_grid=2e-3,
               strain_vy_grid=4e-3, stress_eig_grid=0.5 + np.sqrt(6.25 + 1.0))
    out = {n: v * occ for n, v in val.items()}
    out["area_grid"] = area; out["si_frac_grid"] = area / cell_area; out["mass_grid"] = mass_per_area * area
    return np.stack([out[n] for n in names])


def assert_areas_exact(got_area, got_si, got_mass, ref, xg, yg, mass_per_area, who, cell_free=None):
    """area_grid, si_frac_grid and mass_grid of one floe against the exact reference `ref` = (areas, bounds) per cell (cell_reference,
    topo_reference), cell by cell; cells of exact area 0 must hold exactly 0.0.  cell_free: the cells' free areas where topography takes
    some (default: the whole cell).  Returns the largest error / bound met."""
    area, bound = ref
    worst = 0.0
    u = 2.0 ** -53
    for ix in range(area.shape[0]):
        for iy in range(area.shape[1]):
            ex = area[ix, iy]; b = bound[ix, iy]
            cell = Fr(xg[ix + 1] - xg[ix]) * (yg[iy + 1] - yg[iy]) if cell_free is None or cell_free[ix, iy] <= 0 else cell_free[ix, iy]
            assert b < 1e-12 * float(Fr(xg[ix + 1] - xg[ix]) * (yg[iy + 1] - yg[iy])), (who, ix, iy, b)
            g = (float(got_area[ix, iy]), float(got_si[ix, iy]), float(got_mass[ix, iy]))
            if ex == 0:
                assert g == (0.0, 0.0, 0.0), (who, ix, iy, g)
                continue
            da = abs(Fr(g[0]) - ex)
            assert da <= b, (who, ix, iy, f"area off by {float(da):.3e}, bound {b:.3e}")
            # a quotient and a product of the area: its error, scaled, and two roundings of their own
            ds = abs(Fr(g[1]) - ex / cell); dm = abs(Fr(g[2]) - Fr(mass_per_area) * ex)
            assert ds <= b / float(cell) + 2 * u * float(ex / cell), (who, ix, iy, "si_frac", float(ds))
            assert dm <= mass_per_area * b + 4 * u * mass_per_area * float(ex), (who, ix, iy, "mass", float(dm))
            worst = max(worst, float(da) / b)
    return worst


# ---------------------------------------------------------------- two-way coupling: the family against centre cells
# The coupling's centre cells straddle the grid lines of ITS grid, so the world's grid is laid half a cell off the family's: lines at
# X0 - GX/2 + i GX (i = 0 .. NX + 1).  Centre cell ix (1-based) is then the family's cell ix - 2, with a ring of further cells around; with
# walls the outermost are trimmed to half cells whose outer edges ARE the walls -- x = X0 - GX/2 is eighth -4, where `box-touches-outer-line`
# has a vertex and `half-off-grid` an edge.
def two_way_extent(offset=0):
    return (X0 - GX // 2 + offset, X0 - GX // 2 + (NX + 1) * GX + offset, Y0 - GY // 2 + offset, Y0 - GY // 2 + (NY + 1) * GY + offset)


def two_way_plan(ring, periodic, offset=0):
    """(sub-floe points [(x, y)] in world coordinates, {(ix, iy) 1-based shifted centre cell: exact area}, {(ix, iy): bound}): one point in
    every centre cell whose closed rectangle meets the ring's closed box -- cells the floe only touches included, they must come out 0 --
    at the centre of the (trimmed) cell; periodic: the unshifted cell is clipped and the result lands in the shifted one"""
    wx0, wxf, wy0, wyf = two_way_extent(offset)
    nx, ny = NX + 1, NY + 1
    bx0, bx1 = min(x for x, _ in ring), max(x for x, _ in ring); by0, by1 = min(y for _, y in ring), max(y for _, y in ring)
    pts = []; area = {}; bound = {}
    span = range(-2 * max(nx, ny), 3 * max(nx, ny))
    for ix in span:
        for iy in span:
            x0 = wx0 + (2 * ix - 3) * GX // 2; x1 = x0 + GX; y0 = wy0 + (2 * iy - 3) * GY // 2; y1 = y0 + GY
            if bx1 < x0 or x1 < bx0 or by1 < y0 or y1 < by0:
                continue
            if periodic:
                sx = ix + nx if ix < 1 else (ix - nx if ix > nx else ix); sy = iy + ny if iy < 1 else (iy - ny if iy > ny else iy)
                if not (1 <= sx <= nx + 1 and 1 <= sy <= ny + 1):
                    continue
            else:
                ux, uy = Fr(x0 + x1, 2), Fr(y0 + y1, 2)
                x0, x1, y0, y1 = max(x0, wx0), min(x1, wxf), max(y0, wy0), min(y1, wyf)
                if x0 >= x1 or y0 >= y1:          # a cell beyond the walls: its point is out of bounds and counts nowhere
                    pts.append((ux, uy))
                    continue
                sx, sy = ix, iy
            assert (sx, sy) not in area, "one unshifted cell per shifted one"
            ex = exact_clip(ring, x0, x1, y0, y1)
            L = max([abs(x - x0) for x, _ in ring] + [abs(y - y0) for _, y in ring] + [x1 - x0, y1 - y0])
            pts.append((Fr(x0 + x1, 2), Fr(y0 + y1, 2)))
            area[(sx, sy)] = ex["area"]; bound[(sx, sy)] = rect_bound(ex, x1 - x0, y1 - y0, L)
    return pts, area, bound


def two_way_world(w, ring, periodic, offset=0):
    """one floe at rest in a uniform ocean on the world's grid, its sub-floe points by two_way_plan; one coupling step"""
    pts, area, bound = two_way_plan(ring, periodic, offset)
    wx0, wxf, wy0, wyf = (float(v) for v in two_way_extent(offset))
    w.set_consts()
    w.set_domain([1 if periodic else 2] * 4, wx0, wxf, wy0, wyf)
    w.set_settings(coupling_dd=1)
    w.set_grid_fields(NX + 1, NY + 1, wx0, wxf, wy0, wyf, 0.5, 0.0, 0.0, 0.0, 0.0)
    w.add_floe(as_array(ring), HEIGHT)
    cx, cy = float(w.get("cx")[0]), float(w.get("cy")[0])
    w.set_subpoints(0, [float(x) - cx for x, _ in pts], [float(y) - cy for _, y in pts])
    w.set_two_way(True, dt=20)
    w.set_temps(0.0, -10.0)
    w.timestep_coupling()
    return w, area, bound


# ---------------------------------------------------------------- FC_CAP: one floe under whose sub-floe points lie `ncells` distinct centre cells
FC_N, FC_D = 10, 10000          # 10 x 10 cells of 10 km; the square floe [10 km, 90 km]^2 has area in 9 x 9 = 81 centre cells (the outer ones halved)


def fc_world(w, ncells):
    """walled; the floe's sub-floe points are the first `ncells` grid nodes (row by row) of the 81 whose centre cells it enters"""
    assert ncells <= 81
    L = FC_N * FC_D
    pts = [(FC_D, FC_D), (FC_D, L - FC_D), (L - FC_D, L - FC_D), (L - FC_D, FC_D)]
    ring = pts + pts[:1]
    nodes = [(ix, iy) for iy in range(2, 11) for ix in range(2, 11)][:ncells]
    area = {}; bound = {}
    for ix, iy in nodes:
        x0, y0 = (2 * ix - 3) * FC_D // 2, (2 * iy - 3) * FC_D // 2
        ex = exact_clip(ring, x0, x0 + FC_D, y0, y0 + FC_D)
        area[(ix, iy)] = ex["area"]; bound[(ix, iy)] = rect_bound(ex, FC_D, FC_D, L)
    w.set_consts()
    w.set_domain([2] * 4, 0.0, float(L), 0.0, float(L))
    w.set_settings(coupling_dd=1)
    w.set_grid_fields(FC_N, FC_N, 0.0, float(L), 0.0, float(L), 0.5, 0.0, 0.0, 0.0, 0.0)
    w.add_floe(as_array(ring), HEIGHT)
    cx, cy = float(w.get("cx")[0]), float(w.get("cy")[0])
    w.set_subpoints(0, [float((ix - 1) * FC_D) - cx for ix, _ in nodes], [float((iy - 1) * FC_D) - cy for _, iy in nodes])
    w.set_two_way(True, dt=20)
    w.set_temps(0.0, -10.0)
    return w, area, bound


def assert_si_frac_exact(si, area, bound, who, cell=GX * GY):
    """si_frac on the lattice of grid nodes against Σ area / (gdx gdy): exact zeros everywhere but in the planned cells"""
    gxy = cell; cell = float(cell); u = 2.0 ** -53
    worst = 0.0
    for ix in range(si.shape[0]):
        for iy in range(si.shape[1]):
            ex = area.get((ix + 1, iy + 1), Fr(0)); g = float(si[ix, iy])
            if ex == 0:
                assert g == 0.0, (who, ix + 1, iy + 1, g)
                continue
            b = bound[(ix + 1, iy + 1)]
            assert b < 1e-12 * cell, (who, ix, iy, b)
            d = abs(Fr(g) - ex / gxy)
            assert d <= b / cell + 2 * u * float(ex) / cell, (who, ix + 1, iy + 1, f"si_frac off by {float(d):.3e}, area bound {b:.3e}")
            worst = max(worst, float(d) * cell / b)
    return worst

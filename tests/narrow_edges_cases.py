"""Comb-against-bar pairs that sit on the edges of the narrow phase's working sets, and two references for them.

The narrow phase runs as three kernel variants with fixed LDS working sets (csrc/sz_geom.hpp GroupMem<CAP, KC, RC, RM>, instantiated in
csrc/sz_api.hip): ring points CAP (closed ring), crossings KC, closed region points per clip RC, regions per clip RM.  An item that outgrows the
first or the larger variant is flagged, emits nothing and is redone by the last one (stats()["n_retry"] counts it); an item that outgrows the
last one is an error.  `capacities()` reads the numbers out of the sources, TABLE names for every row which of them it sits on or one step
past, and `edge_claims_hold` turns those names into equalities -- a changed constant moves the table or fails, it never un-edges a case.

The generator.  A comb is a base rectangle (2 km high) with teeth on top, 1 km wide with 1 km gaps; the bar is a rectangle across all teeth
between y = 2 km and y = 3 km above the base.  A tooth is one letter:
    t  triangle, tip at 2.5 km (inside the bar)      1 region, 2 crossings, 4 closed region points
    T  triangle, tip at 4 km (through the bar)       1 region, 4 crossings, 5 closed region points (the many-intersect path)
    r  rectangle, top at 2.5 km                      1 region, 2 crossings, 5 closed region points
    R  rectangle, top at 4 km                        1 region, 4 crossings, 5 closed region points
so K, R and P are set independently, and `pad` extra vertices on a shallow convex arc below the base set the ring size without touching
the contact.  Every coordinate is an integer number of metres: the construction is exact in doubles and in fractions.Fraction alike.

References: the CPU oracle (tests/parity.py's criteria), and an exact one that does not go through any clip -- every region is the tooth cut
by the bar's two horizontal lines, its area and centroid are Fraction shoelace sums over vertices written down from the construction.
"""
import os
import re
from fractions import Fraction as Fr

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "subzero.jl_amd", "csrc")

TOOTH = {"t": (2, 4, 3), "T": (4, 5, 3), "r": (2, 5, 4), "R": (4, 5, 4)}       # letter: crossings, closed region points, ring vertices
BASE_H, BAR_Y0, BAR_Y1, TIP_IN, TIP_THROUGH, PITCH, WIDTH, ARC = 2000, 2000, 3000, 2500, 4000, 2000, 1000, 500


# ---------------------------------------------------------------- capacities, from the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def capacities():
    """{"first" | "larger" | "last": dict(G, CAP, KC, RC, RM), "MV_RING": n, "ROWS_PER_ITEM": n} parsed from sz_api.hip, sz_kernels.hpp and
    sz_state.hpp: the template arguments of the three sz_k_narrow instantiations, with every named constant resolved"""
    api, ker, st = _src("sz_api.hip"), _src("sz_kernels.hpp"), _src("sz_state.hpp")
    const = {}
    for text in (ker, st, api):
        for stmt in re.findall(r"constexpr int ((?:\s*\w+\s*=\s*\d+\s*,?)+);", text):
            for name, val in re.findall(r"(\w+)\s*=\s*(\d+)", stmt):
                const[name] = int(val)
    for name, val in re.findall(r"#define\s+(NARROW_\w+)\s+(\d+)\s*$", api, re.M):
        const[name] = int(val)

    def args(pattern):
        m = re.search(pattern, api, re.M)
        assert m, pattern
        toks = [t.strip() for t in m.group(1).split(",")]
        return dict(zip(("G", "CAP", "KC", "RC", "RM"), (int(t) if t.isdigit() else const[t] for t in toks[:5])))

    out = {"first": args(r"#define\s+NARROW_FIRST_ARGS\s+(.+)$"), "larger": args(r"narrow_larger\s*=\s*sz_k_narrow<([^>]+)>"),
           "last": args(r"narrow_last\s*=\s*sz_k_narrow<([^>]+)>"), "MV_RING": const["MV_RING"], "ROWS_PER_ITEM": const["ROWS_PER_ITEM"]}
    out["GHOST_FILL"], out["GHOST_FILL_WIDE"] = const["GHOST_RING"], const["GHOST_RING_WIDE"]          # the ghost passes: one / two ring points per lane
    return out


def first_variant_of(kernel_name):
    """World.narrow_kernel_name() -> dict(G, CAP, KC, RC, RM)"""
    m = re.fullmatch(r"sz_k_narrow<([\d,]+)>", kernel_name)
    assert m, kernel_name
    return dict(zip(("G", "CAP", "KC", "RC", "RM"), map(int, m.group(1).split(",")[:5])))


VARIANTS = ("first", "larger", "last")


def ring_class(ring_points, caps):
    """the variant an item starts in: by the larger of its two rings (csrc/sz_kernels.hpp, `big <= NARROW_CAP0 ? 0 : ...`); None: no variant"""
    for v in VARIANTS:
        if ring_points <= caps[v]["CAP"]:
            return v
    return None


# ---------------------------------------------------------------- the generator
def comb_counts(comb, pad=0):
    """(closed ring points, K, R, P) of a comb against its bar, by construction"""
    return (4 + sum(TOOTH[c][2] for c in comb) + pad + 1, sum(TOOTH[c][0] for c in comb), len(comb), sum(TOOTH[c][1] for c in comb))


def _exact(pts):
    out = np.array([[float(x), float(y)] for x, y in pts])
    assert all(Fr(float(x)) == x and Fr(float(y)) == y for x, y in pts), "the construction must be exact in doubles"
    return out


def comb_ring(comb, pad=0, ox=0, oy=0):
    """closed clockwise ring of the comb, as Fractions: base rectangle below y = oy, teeth above, `pad` arc points under the base"""
    n = len(comb); W = PITCH * n
    pts = [(0, -BASE_H), (0, 0)]
    for i, c in enumerate(comb):
        x = PITCH // 4 + PITCH * i
        top = TIP_THROUGH if c in "TR" else TIP_IN
        if c in "tT":
            pts += [(x, 0), (x + WIDTH // 2, top), (x + WIDTH, 0)]
        else:
            pts += [(x, 0), (x, top), (x + WIDTH, top), (x + WIDTH, 0)]
    pts += [(W, 0), (W, -BASE_H)]
    for k in range(1, pad + 1):          # strictly convex (a sine arc), rounded to millimetres: exact in doubles at these magnitudes
        th = np.pi * k / (pad + 1)
        pts.append((Fr(round(W * (1 - k / (pad + 1)) * 1024), 1024), -BASE_H - Fr(round(ARC * np.sin(th) * 1024), 1024)))
    pts.append(pts[0])
    return [(Fr(x) + ox, Fr(y) + oy) for x, y in pts]


def bar_ring(ntooth, ox=0, oy=0):
    W = PITCH * ntooth
    pts = [(-1000, BAR_Y0), (-1000, BAR_Y1), (W + 1000, BAR_Y1), (W + 1000, BAR_Y0), (-1000, BAR_Y0)]
    return [(Fr(x) + ox, Fr(y) + oy) for x, y in pts]


def exact_regions(comb, ox=0, oy=0):
    """[(area, cx, cy, open points)] per tooth, in tooth order, as Fractions: the tooth between the lines y = BAR_Y0 and y = BAR_Y1"""
    out = []
    for i, c in enumerate(comb):
        x = Fr(PITCH // 4 + PITCH * i); top = Fr(TIP_THROUGH if c in "TR" else TIP_IN); half = Fr(WIDTH, 2); mid = x + half
        hw = lambda y: half * (1 - Fr(y) / top)          # half width of a triangle tooth at height y
        if c == "t":
            poly = [(mid - hw(BAR_Y0), BAR_Y0), (mid, top), (mid + hw(BAR_Y0), BAR_Y0)]
        elif c == "T":
            poly = [(mid - hw(BAR_Y0), BAR_Y0), (mid - hw(BAR_Y1), BAR_Y1), (mid + hw(BAR_Y1), BAR_Y1), (mid + hw(BAR_Y0), BAR_Y0)]
        else:
            y1 = BAR_Y1 if c == "R" else top
            poly = [(x, BAR_Y0), (x, y1), (x + WIDTH, y1), (x + WIDTH, BAR_Y0)]
        poly = [(Fr(px) + ox, Fr(py) + oy) for px, py in poly]
        a2 = Fr(0); sx = Fr(0); sy = Fr(0)
        for (x0, y0), (x1, y1) in zip(poly, poly[1:] + poly[:1]):
            w = x0 * y1 - x1 * y0
            a2 += w; sx += (x0 + x1) * w; sy += (y0 + y1) * w
        out.append((abs(a2) / 2, sx / (3 * a2), sy / (3 * a2), len(poly)))
    return out


def exact_bound(n, Lc, area):
    """(area tolerance, centroid tolerance) of a double-precision shoelace over n points at coordinate scale Lc: every one of the n products
    is rounded once (2^-53 Lc^2 each) and carries the crossings' couple of ulps of Lc in its factors (2 * 2 * 2^-53 Lc^2), the running sum
    rounds n times more: inside 4 n 2^-52 Lc^2 absolute.  The centroid is a quotient of such sums (times Lc) by the area: that error over the
    area, times Lc."""
    a = 4.0 * n * 2.0 ** -52 * Lc * Lc
    return a, a / float(area) * Lc


# ---------------------------------------------------------------- the case table
# name: comb, pad, the variant whose working set the row is about, and where K / R / P / ring sit against THAT variant's KC / RM / RC / CAP:
# "at" = equal, "past" = the first reachable value beyond (K moves in steps of 2), "in" = below, "-" = the row makes no claim.
# `over`: the item outgrows the variant (past in any of K, R, P): first / larger -> retried, last -> the call is an error.
TABLE = {
    # first variant (rings of at most CAP0 points)
    "first-all-at":   dict(comb="tttt", pad=0, variant="first", K="at", R="at", P="at", ring="in", over=False),
    "first-K-past":   dict(comb="tTT", pad=0, variant="first", K="past", R="in", P="in", ring="in", over=True),
    "first-P-past":   dict(comb="rttt", pad=0, variant="first", K="at", R="at", P="past", ring="at", over=True),
    "first-inside":   dict(comb="ttt", pad=0, variant="first", K="in", R="in", P="in", ring="in", over=False),
    # larger variant (rings of CAP0 + 1 .. CAP1 points)
    "larger-R-at":    dict(comb="tttttt", pad=0, variant="larger", K="in", R="at", P="in", ring="in", over=False),
    "larger-R-past":  dict(comb="ttttttt", pad=0, variant="larger", K="in", R="past", P="in", ring="in", over=True),
    "larger-K-at":    dict(comb="TTTT", pad=2, variant="larger", K="at", R="in", P="in", ring="in", over=False),
    "larger-K-past":  dict(comb="TTTTt", pad=0, variant="larger", K="past", R="in", P="in", ring="in", over=True),
    # last variant
    "last-R-at":      dict(comb="t" * 16, pad=0, variant="last", K="in", R="at", P="in", ring="in", over=False),          # 16 regions, 16 rows: ROWS_PER_ITEM
    "last-R-past":    dict(comb="t" * 17, pad=0, variant="last", K="in", R="past", P="in", ring="in", over=True),
    "last-K-at":      dict(comb="T" * 16, pad=0, variant="last", K="at", R="at", P="in", ring="in", over=False),
    "last-K-past":    dict(comb="T" * 16 + "t", pad=0, variant="last", K="past", R="past", P="in", ring="in", over=True),
}
# Capacities that cannot be reached inside the others -- no case is invented for them:
#   first,  R past 4:   a fifth region brings at least two more crossings: K >= 10 > KC = 8, and the crossing test comes first (`first-K-past`
#                       and `ttttt` are that case);
#   larger, RC = 80:    the regions of a clip hold each crossing and each distinct ring vertex of the pair at most once, so their open points
#                       number at most KC + (CAP - 1) + (CAP - 1) = 16 + 31 + 31 = 78 <= 80; only the R <= 6 closing points could carry P past
#                       80, and only if EVERY vertex of both 32-point rings lay inside the other ring with all 16 crossings in use.  This
#                       generator cannot make that pair (a comb's base corners are never inside the bar): P of the larger variant is "in";
#   last,   RC = 640:   likewise P <= 64 + 254 + 254 + 16 closing points = 588 < 640: unreachable from 255-point rings.
UNREACHABLE = {"first": "R past RM forces K >= 10 > KC", "larger": "P <= 16 + 31 + 31 open points + 6 closures; beyond 80 only with every vertex of both rings inside the other",
               "last": "P <= 64 + 254 + 254 + 16 = 588 < RC = 640"}

RING_CLASSES = (18, 19, 20, 21, 32, 33, 64, 65, 128, 129, 255, 256)          # closed ring points `tttt` is padded to
RING_COMB = "tttt"


def ring_case(points):
    return dict(comb=RING_COMB, pad=points - comb_counts(RING_COMB)[0], variant=None, over=False)


def case(name):
    return TABLE[name] if isinstance(name, str) else ring_case(name)


def counts(name):
    c = case(name)
    return comb_counts(c["comb"], c["pad"])


def edge_claims_hold(name, caps):
    """the row's at / past / in words against the variant's parsed capacities; returns a list of the claims that do not hold"""
    c = TABLE[name]; v = caps[c["variant"]]
    ring, K, R, P = counts(name)
    bad = []
    for what, val, cap, step in (("K", K, v["KC"], 2), ("R", R, v["RM"], 1), ("P", P, v["RC"], 1), ("ring", ring, v["CAP"], 1)):
        word = c[what]
        ok = {"at": val == cap, "past": val == cap + step, "in": val < cap, "-": True}[word]
        if not ok:
            bad.append(f"{name}: {what} = {val} is not '{word}' {cap}")
    lo = {"first": 0, "larger": caps["first"]["CAP"], "last": caps["larger"]["CAP"]}[c["variant"]]
    if not lo < ring <= v["CAP"]:
        bad.append(f"{name}: a ring of {ring} points does not start in the {c['variant']} variant")
    over = K > v["KC"] or R > v["RM"] or P > v["RC"] or R > caps["ROWS_PER_ITEM"]
    if over != c["over"]:
        bad.append(f"{name}: over = {over}")
    return bad


def outgrows(name, caps):
    """(the variant the item starts in, whether it outgrows it): from the counts and the parsed capacities alone"""
    ring, K, R, P = counts(name)
    cls = ring_class(max(ring, 5), caps)
    if cls is None:
        return None, True
    v = caps[cls]
    return cls, K > v["KC"] or R > v["RM"] or P > v["RC"] or R > caps["ROWS_PER_ITEM"]


def expected_n_retry(names, caps, orders=2):
    """items of the first or the larger ring class that pass a capacity of that class (each case occurs in `orders` floe orders); items whose
    rings alone send them to the last variant are not retries"""
    n = 0
    for name in names:
        cls, over = outgrows(name, caps)
        n += orders * int(cls in ("first", "larger") and over)
    return n


# ---------------------------------------------------------------- worlds: case pairs on a lattice, each in both floe orders
CELL = (50000, 40000); NCOL = 4; ORIGIN = (30123, 20457)


def placements(names, orders=("comb-first", "bar-first")):
    """[(name, order, ox, oy)]: slot k of the lattice holds one pair; integer offsets up to a few 1e5 m"""
    out = []
    for name in names:
        for order in orders:
            k = len(out)
            out.append((name, order, ORIGIN[0] + CELL[0] * (k % NCOL), ORIGIN[1] + CELL[1] * (k // NCOL)))
    return out


def extent(place):
    rows = (len(place) + NCOL - 1) // NCOL
    return 0.0, float(CELL[0] * NCOL + 20000), 0.0, float(CELL[1] * rows + 10000)


def pair_rings(name, ox, oy):
    c = case(name)
    return _exact(comb_ring(c["comb"], c["pad"], ox, oy)), _exact(bar_ring(len(c["comb"]), ox, oy))


def build_world(w, place, kinds=(1, 1, 1, 1), E=None, ext=None):
    """floes 2k, 2k + 1 are the pair of slot k, in its order; the grid fields are still (coupling off in every use)"""
    if E is not None:
        w.set_consts(E=E)
    w.set_settings()
    x0, xf, y0, yf = ext or extent(place)
    w.set_domain(list(kinds), x0, xf, y0, yf)
    w.set_grid_fields(10, 10, x0, xf, y0, yf, 0.0, 0.0, 0.0, 0.0, 0.0)
    for name, order, ox, oy in place:
        comb, bar = pair_rings(name, ox, oy)
        for ring in ((comb, bar) if order == "comb-first" else (bar, comb)):
            w.add_floe(ring, 0.5)
    return w


def stir(w, xi=1.0e-6):
    """a slow spin on every floe, alternating in sense, for the worlds that are stepped: most combs are mirror-symmetric, so the torques of
    their teeth cancel and alpha / xi would hold nothing but round-off -- a column a max-norm comparison cannot judge.  Over 10 steps of 10 s
    a floe turns by 1e-4 rad (a tooth tip moves well under a metre: K, R and P stay the table's), and the contacts leave the integer grid."""
    w.set("xi", xi * (1.0 - 2.0 * (np.arange(w.M) % 2)))
    return w


def build_element_world(w, name, comb_is_element, ox=ORIGIN[0], oy=ORIGIN[1]):
    """open boundaries, one topography element against one floe: the comb against a bar floe, or a bar-shaped element against a comb floe"""
    comb, bar = pair_rings(name, ox, oy)
    w.set_settings()
    w.set_domain([0, 0, 0, 0], 0.0, 2.0e5, 0.0, 1.0e5)
    w.set_topography([comb if comb_is_element else bar])
    w.set_grid_fields(10, 10, 0.0, 2.0e5, 0.0, 1.0e5, 0.0, 0.0, 0.0, 0.0, 0.0)
    w.add_floe(bar if comb_is_element else comb, 0.5)
    return w


# ---------------------------------------------------------------- checks shared by the CPU test (on the oracle) and the GPU test (on the HIP rows)
def oracle_counts(name, swap=False):
    """(ring points, K, R, P) of the case as the oracle's clip and intersection_points see it"""
    from oracle import orc
    comb, bar = pair_rings(name, ORIGIN[0], ORIGIN[1])
    a, b = (bar, comb) if swap else (comb, bar)
    regs = orc.clip(a, b, max_regions=32)
    return len(comb), len(orc.intersection_points(a, b)), len(regs), sum(len(r) for r in regs)


def assert_rows_exact(rows, name, ox, oy, who):
    """the overlap (column 6) and contact point (3, 4) of one item's rows against exact_regions, every region met by exactly one row; returns
    the worst ratio error / bound"""
    c = case(name)
    ex = exact_regions(c["comb"], ox, oy)
    assert len(rows) == len(ex), (who, name, len(rows), len(ex))
    comb, bar = pair_rings(name, ox, oy)
    Lc = float(max(np.abs(comb).max(), np.abs(bar).max()))
    used = set(); worst = 0.0
    for r in rows:
        k = int(np.argmin([abs(float(e[1]) - r[3]) for e in ex]))
        assert k not in used, (who, name, "two rows on one tooth")
        used.add(k)
        area, cx, cy, n = ex[k]
        ta, tc = exact_bound(n + 1, Lc, area)
        da = abs(Fr(float(r[6])) - area); dx = abs(Fr(float(r[3])) - cx); dy = abs(Fr(float(r[4])) - cy)
        assert da <= ta and dx <= tc and dy <= tc, (who, name, f"tooth {k}: |area| off by {float(da):.3e} (bound {ta:.3e}), "
                                                    f"point by {float(dx):.3e}, {float(dy):.3e} (bound {tc:.3e})")
        worst = max(worst, float(da) / ta, float(dx) / tc, float(dy) / tc)
    return worst


def assert_world_rows_exact(w, place, who, skip=()):
    """every pair of the lattice world: the rows floe 2k holds against 2k + 1 and the mirrored ones"""
    off, rows = w.interactions()
    worst = 0.0
    for k, (name, order, ox, oy) in enumerate(place):
        if name in skip:
            continue
        for i, j in ((2 * k, 2 * k + 1), (2 * k + 1, 2 * k)):
            mine = rows[off[i]:off[i + 1]]
            mine = mine[mine[:, 0] == j + 1] if len(mine) else mine
            worst = max(worst, assert_rows_exact(mine, name, ox, oy, f"{who} floe {i}"))
    return worst


def assert_totals_are_row_sums(w, who):
    """coll_fx / coll_fy / overarea of every floe equal the sums of its own rows to 1e-12 of the largest row: a retried item was added once"""
    off, rows = w.interactions()
    M = len(off) - 1
    for col, f in ((1, "coll_fx"), (2, "coll_fy"), (6, "overarea")):
        got = w.get(f)[:M]
        big = float(np.max(np.abs(rows[:, col]))) if len(rows) else 0.0
        for i in range(M):
            s = float(np.sum(rows[off[i]:off[i + 1], col]))
            assert abs(got[i] - s) <= 1e-12 * big, (who, f, i, got[i], s)

"""The geometry and the decision loop of timestep_welding! (Subzero.jl src/physical_processes/welding.jl) restated from what the oracle exports
(orc.clip = intersect_polys, World.in_bounds, the floe columns and rings): the yardstick of the device's welding overlap table
(csrc/sz_weld.hpp), itself pinned by tests/golden/welding.json (the reference's own test values).  Indices are 0-based here."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "welding.json")
ACTIVE, REMOVE = 1, 2
KIND = {"open": 0, "periodic": 1, "collision": 2, "moving": 3}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_world(w, g, part, domain):
    """the fixture's grid, a domain and the rings of `part` ("bin_floes" / "weld_floes") in a World-like object (engine or oracle)"""
    gr = g["grid"]
    w.set_domain([KIND[k] for k in g["domains"][domain]], gr["x0"], gr["xf"], gr["y0"], gr["yf"])
    z = np.zeros((gr["nx"] + 1, gr["ny"] + 1))
    w.set_grid_fields(gr["nx"], gr["ny"], gr["x0"], gr["xf"], gr["y0"], gr["yf"], z, z, z, z, z)
    for r in g[part]["rings"]:
        w.add_floe(np.array(r, float), g[part]["height"])
    return w


def periodic_flags(kinds):
    """(per_x, per_y) of a [north, south, east, west] kind list, as in_bounds(.., domain.north, domain.east) dispatches"""
    k = [KIND[v] if isinstance(v, str) else int(v) for v in kinds]
    return k[2] == KIND["periodic"], k[0] == KIND["periodic"]


def bins(ow, grid, per_x, per_y, nx, ny):
    """bin_floe_centroids (:23-55): per floe the bin number (yidx - 1) nx + (xidx - 1) -- eachindex of the nx x ny matrix -- or -1.  The loop
    BREAKS at the first centroid that is out of bounds (:38): the floes behind it are in no bin."""
    x0, xf, y0, yf = grid
    cx, cy = ow.get("cx"), ow.get("cy")
    dx, dy = (xf - x0) / nx, (yf - y0) / ny
    out = np.full(len(cx), -1, np.int32)
    for i in range(len(cx)):
        xp, yp = float(cx[i]), float(cy[i])
        if not ow.in_bounds(xp, yp, per_x, per_y):
            break
        xidx = int(np.floor((xp - x0) / dx)) + 1
        xidx = 1 if xp <= x0 else xidx
        xidx = nx if xp >= xf else xidx
        yidx = int(np.floor((yp - y0) / dy)) + 1
        yidx = 1 if yp <= y0 else yidx
        yidx = ny if yp >= yf else yidx
        out[i] = (yidx - 1) * nx + (xidx - 1)
    return out


def shoelace(r):
    x, y = r[:, 0], r[:, 1]
    return abs(0.5 * float(np.sum(x[:-1] * y[1:] - x[1:] * y[:-1])))


def inter_area(ra, rb, clip):
    return float(sum(shoelace(r) for r in clip(ra, rb)))


def candidates(bin_, cx, cy, rmax, area, status, max_weld_area):
    """the pairs the loops of :105-132 reach, in their order: bins ascending, i then j ascending in a bin; i < j, both active, both under
    max_weld_area, potential_interaction (strict <, parents only)"""
    out = []
    ok = (bin_ >= 0) & (status == ACTIVE) & (area < max_weld_area)
    for k in np.unique(bin_[ok]):
        lst = np.nonzero(ok & (bin_ == k))[0]
        for a, i in enumerate(lst):
            js = lst[a + 1:]
            ddx, ddy, rr = cx[i] - cx[js], cy[i] - cy[js], rmax[i] + rmax[js]
            for j in js[(ddx * ddx + ddy * ddy) < rr * rr]:
                out.append((int(k), int(i), int(j)))
    return out


def overlaps(ow, grid, per_x, per_y, nx, ny, max_weld_area, clip=None, timer=None):
    """-> (candidate pairs [(k, i, j)], their inter_area): the table is the entries with inter_area > 0"""
    if clip is None:
        from oracle import orc
        clip = orc.clip
    b = bins(ow, grid, per_x, per_y, nx, ny)
    cand = candidates(b, ow.get("cx"), ow.get("cy"), ow.get("rmax"), ow.get("area"), ow.ids()[2], max_weld_area)
    off, x, y = ow.rings()
    ring = lambda i: np.stack([x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]], 1)
    areas = np.zeros(len(cand))
    for q, (_, i, j) in enumerate(cand):
        ri, rj = ring(i), ring(j)
        if timer is not None:
            t0 = timer["clock"]()
            regs = clip(ri, rj)
            timer["s"] += timer["clock"]() - t0
            areas[q] = float(sum(shoelace(r) for r in regs))
        else:
            areas[q] = inter_area(ri, rj, clip)
    return cand, areas


def table_of(cand, areas):
    return [(i, j, float(a)) for (_, i, j), a in zip(cand, areas) if a > 0]


def _decide(i, entries, area, status, s, draw, fuses):
    """one floe i with its overlapping partners [(j, inter_area)] in visiting order: the draws, the window, the sort, the running area (:135-171)"""
    group = []
    for j, a in entries:
        prob = s["welding_coeff"] * (a / area[i])
        union = area[i] + area[j] - a
        if a > 0 and prob > draw() and s["min_weld_area"] < union and s["max_weld_area"] > union:
            group.append((j, a))
    group.sort(key=lambda e: -e[1])
    for j, a in group:
        if area[i] + area[j] - a > s["max_weld_area"]:
            break
        area[i] += area[j] - a          # a successful fuse: floe i takes the union's area, floe j leaves
        status[j] = REMOVE
        fuses.append((i, j))


def plan(table, area, status, settings, draws):
    """timestep_welding! between the clip and fuse_two_floes!, driven by the overlap table computed ONCE at the start of the call (entries
    grouped by bin and by i, in visiting order).  -> (fuses [(i, j)], draws taken, area, status)"""
    area, status = np.array(area, float), np.array(status, np.int32)
    it = iter(draws); n = [0]

    def draw():
        n[0] += 1
        return next(it)
    fuses = []
    e = 0
    while e < len(table):
        i = table[e][0]
        stop = e
        while stop + 1 < len(table) and table[stop + 1][0] == i:
            stop += 1
        if status[i] == ACTIVE and area[i] < settings["max_weld_area"]:
            entries = [(j, a) for (_, j, a) in table[e:stop + 1] if status[j] == ACTIVE and area[j] < settings["max_weld_area"]]
            _decide(i, entries, area, status, settings, draw, fuses)
        e = stop + 1
    return fuses, n[0], area, status


def plan_live(bin_, cx, cy, rmax, rings, area, status, settings, draws, clip):
    """the same loop as the reference writes it: every pair is tested and clipped at the moment the loop reaches it, on the statuses and areas of
    that moment (rings of a floe that is kept stay as they are: what is compared is WHICH pairs are asked for, and when).
    -> (fuses, draws taken, area, status, pairs asked)"""
    area, status = np.array(area, float), np.array(status, np.int32)
    it = iter(draws); n = [0]

    def draw():
        n[0] += 1
        return next(it)
    fuses, asked = [], []
    mx = settings["max_weld_area"]
    for k in range(int(bin_.max()) + 1 if len(bin_) else 0):
        lst = np.nonzero(bin_ == k)[0]
        for i in lst:
            entries = []
            if status[i] == ACTIVE and area[i] < mx:
                for j in lst:
                    ddx, ddy, rr = cx[i] - cx[j], cy[i] - cy[j], rmax[i] + rmax[j]
                    if i != j and i < j and status[i] == ACTIVE and status[j] == ACTIVE and area[i] < mx and area[j] < mx and \
                            (ddx * ddx + ddy * ddy) < rr * rr:
                        asked.append((int(i), int(j)))
                        entries.append((int(j), inter_area(rings[i], rings[j], clip)))
            _decide(int(i), entries, area, status, settings, draw, fuses)
    return fuses, n[0], area, status, asked

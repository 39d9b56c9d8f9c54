"""remove_floes! (simplification.jl:279-314) with dissolve_floe! (:18-32), find_grid_cell_index (coupling.jl:440-444) and shift_cell_idx
(coupling.jl:1154-1178), restated line by line over a dict of columns with CSR rings and sub-floe points: the yardstick of
tests/test_remove_cpu.py and tests/test_remove_gpu.py."""
import math

import numpy as np

from subzero_jl_amd import capi

ACTIVE, REMOVE, FUSE = capi.ACTIVE, capi.REMOVE, capi.FUSE
PER_ROW = capi.DCOLS + capi.TCOLS + ["id", "ghost_id", "status"]


def find_grid_cell_index(xp, yp, grid):
    Nx, Ny, x0, xf, y0, yf = grid
    dx, dy = (xf - x0) / Nx, (yf - y0) / Ny
    return math.floor((xp - x0) / dx) + 1, math.floor((yp - y0) / dy) + 1


def shift_cell_idx(idx, nlines, periodic):
    if not periodic:
        return idx
    ncells = nlines - 1
    return idx + ncells if idx < 1 else idx - ncells if ncells < idx else idx


def dissolve_floe(cols, i, grid, periodic_east, periodic_north, dissolved):
    """dissolved: the (Nx+1) x (Ny+1) matrix; the reference indexes it [yidx, xidx] (1-based), an index outside it raises (BoundsError)"""
    Nx, Ny = grid[0], grid[1]
    xidx, yidx = find_grid_cell_index(float(cols["cx"][i]), float(cols["cy"][i]), grid)
    xidx = shift_cell_idx(xidx, Nx + 1, periodic_east)
    yidx = shift_cell_idx(yidx, Ny + 1, periodic_north)
    if 0 < xidx <= Nx and 0 < yidx <= Ny:
        if yidx > dissolved.shape[0] or xidx > dissolved.shape[1]:
            raise IndexError(f"BoundsError: dissolved[{yidx}, {xidx}] of a {dissolved.shape} matrix")
        dissolved[yidx - 1, xidx - 1] += cols["mass"][i]


def _deleteat(cols, i):
    """StructArrays.foreachfield(field -> deleteat!(field, i), floes), the ragged fields as CSR"""
    for n in PER_ROW:
        if n in cols:
            cols[n] = np.delete(cols[n], i, axis=0)
    for off, members in (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy"))):
        if off not in cols:
            continue
        o = cols[off]
        a, b = int(o[i]), int(o[i + 1])
        for m in members:
            cols[m] = np.delete(cols[m], np.s_[a:b])
        cols[off] = np.concatenate([o[:i + 1], o[i + 2:] - (b - a)]).astype(o.dtype)


def remove_ref(cols, grid, periodic_east, periodic_north, dissolved, min_floe_area=1e6, min_floe_height=0.1):
    """cols: dict of columns (copied); grid = (Nx, Ny, x0, xf, y0, yf); dissolved is updated in place.
    Returns (new columns, kept row indices ascending, n_removed, n_dissolved)."""
    cols = {k: np.array(v, copy=True) for k, v in cols.items()}
    n = len(cols["cx"])
    kept, n_removed, n_dissolved = [], 0, 0
    for i in reversed(range(n)):
        if cols["status"][i] != REMOVE and (cols["area"][i] < min_floe_area or cols["height"][i] < min_floe_height):
            dissolve_floe(cols, i, grid, periodic_east, periodic_north, dissolved)
            _deleteat(cols, i)
            n_dissolved += 1
        elif cols["status"][i] == REMOVE:
            _deleteat(cols, i)
            n_removed += 1
        else:
            cols["status"][i] = ACTIVE
            kept.append(i)
    return cols, np.array(kept[::-1], np.int64), n_removed, n_dissolved


def would_decline(cols, max_vertices):
    """the cases in which simplify_floes! does not reduce to remove_floes!: a fuse tag, a ring over max_vertices (closing point counted)"""
    return bool(np.any(cols["status"] == FUSE) or np.any(np.diff(cols["vert_off"]) > max_vertices))

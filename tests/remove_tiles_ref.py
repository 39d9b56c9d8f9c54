"""The cross-rank part of a tiled removal pass (csrc/sz_remove_tile.hpp) restated in numpy over dicts of columns: per rank the leaving records,
their merge into one list by global number, the renumbering of the floes that stay, and the descending walk of the merged list into ONE
lattice.  What a single rank does with its own rows is tests/remove_ref.py's; tests/test_remove_tiles_cpu.py holds the whole to remove_ref run
over the undivided list."""
import numpy as np

import remove_ref as rr


def take_rows(cols, idx):
    """the rows idx (ascending) of a dict of columns with CSR rings and sub-floe points"""
    out = {k: np.array(cols[k][idx], copy=True) for k in rr.PER_ROW if k in cols}
    for off, members in (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy"))):
        o = cols[off]
        cnt = np.diff(o)[idx]
        sel = np.concatenate([np.arange(o[i], o[i + 1]) for i in idx]) if len(idx) else np.zeros(0, int)
        out[off] = np.concatenate([[0], np.cumsum(cnt)]).astype(o.dtype)
        for m in members:
            out[m] = cols[m][sel]
    return out


def flags(cols, min_floe_area, min_floe_height):
    """the branch order of remove_floes!: dissolve first, then remove, else keep"""
    dis = (cols["status"] != rr.REMOVE) & ((cols["area"] < min_floe_area) | (cols["height"] < min_floe_height))
    rem = ~dis & (cols["status"] == rr.REMOVE)
    return dis, rem


def leaving_records(cols, gidx, dis, rem):
    """rows of {old global number, kind (1: dissolves), cx, cy, mass}, ascending like the rank's rows"""
    i = np.nonzero(dis | rem)[0]
    return np.stack([np.asarray(gidx, float)[i], dis[i].astype(float), cols["cx"][i], cols["cy"][i], cols["mass"][i]], 1).reshape(-1, 5)


def merge(lists):
    """every rank's records in one list ordered by global number: a record's place is its place in its own list plus the records of the
    other lists with a smaller number"""
    total = sum(len(l) for l in lists)
    out = np.zeros((total, 5))
    for r, l in enumerate(lists):
        for k in range(len(l)):
            pos = k + sum(int(np.searchsorted(o[:, 0], l[k, 0], side="left")) for q, o in enumerate(lists) if q != r)
            out[pos] = l[k]
    return out


def renumber(gidx_kept, merged):
    g = np.asarray(gidx_kept, np.int64)
    return g - np.searchsorted(merged[:, 0], g.astype(float), side="left")


def walk(merged, grid, periodic_east, periodic_north, dissolved):
    """the merged list in DESCENDING global number into the one lattice; IndexError where the reference's [yidx, xidx] leaves the matrix"""
    rec = {"cx": merged[:, 2], "cy": merged[:, 3], "mass": merged[:, 4]}
    for k in reversed(range(len(merged))):
        if merged[k, 1] != 0.0:
            rr.dissolve_floe(rec, k, grid, periodic_east, periodic_north, dissolved)


def tile_remove_ref(cols, owner, nranks, grid, periodic_east, periodic_north, dissolved, max_vertices=30, min_floe_area=1e6, min_floe_height=0.1):
    """cols: the undivided list; owner[i]: the rank of global row i.  Returns (done, n_removed, n_dissolved, per rank (columns, global numbers));
    done == False: declined on every rank, nothing changed (the per-rank entries are then the rows as they were).  dissolved: the lattice every
    rank holds, updated in place."""
    owner = np.asarray(owner)
    ranks = []
    for r in range(nranks):
        gidx = np.nonzero(owner == r)[0]
        c = take_rows(cols, gidx)
        dis, rem = flags(c, min_floe_area, min_floe_height)
        ranks.append(dict(cols=c, gidx=gidx, dis=dis, rem=rem, fuse=int(np.count_nonzero(c["status"] == rr.FUSE)),
                          over=int(np.count_nonzero(np.diff(c["vert_off"]) > max_vertices)), stay=int(np.count_nonzero(~(dis | rem)))))
    unchanged = [(k["cols"], k["gidx"]) for k in ranks]
    # one verdict from the gathered counts: a fuse tag or a long ring anywhere, a rank (or the world) left without a floe
    if any(k["fuse"] or k["over"] or k["stay"] == 0 for k in ranks):
        return False, 0, 0, unchanged
    merged = merge([leaving_records(k["cols"], k["gidx"], k["dis"], k["rem"]) for k in ranks])
    trial = dissolved.copy()
    try:
        walk(merged, grid, periodic_east, periodic_north, trial)
    except IndexError:
        return False, 0, 0, unchanged
    dissolved[...] = trial
    out = []
    for k in ranks:
        keep = np.nonzero(~(k["dis"] | k["rem"]))[0]
        c = take_rows(k["cols"], keep)
        c["status"][:] = rr.ACTIVE
        out.append((c, renumber(k["gidx"][keep], merged)))
    return True, int(sum(np.count_nonzero(k["rem"]) for k in ranks)), int(sum(np.count_nonzero(k["dis"]) for k in ranks)), out

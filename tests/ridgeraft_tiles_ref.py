"""numpy / Python restatement of the partition and merge rule of the tiled ridge / raft candidate pass (csrc/sz_ridgeraft_tile.hpp, tile_rr_pass;
DESIGN.md §9e, "tiled contexts"), over any World after add_ghosts() + timestep_collisions():

  keys(w)                 an order key per list row: a parent's is its number, a ghost's lies above GHOST and grows with its place -- sorted, the
                          keys are the list order; and the root parent of every row (a ghost's: the parent that made it)
  rank_lists(...)         the local list of every rank: the rows whose root parent it owns, every row those name as a partner, some rows it has
                          no use for, all in a shuffled order; the partner column of its rows holds key + 1
  local_table(...)        the rule on one rank, in keys: only rows whose root parent is owned are evaluated, i < j is key_i < key_j, a partner is
                          looked up by key, an entry is (key_i, key_j or the negative number, kind, frac)
  merge(...)              the tables of all ranks into the single context's: the distinct ghost keys of the owned roots, sorted, number the
                          ghosts (n_parents + place); ascending i, then the emitting rank's order
"""
import numpy as np

import ridgeraft_ref as rr

GHOST = 1 << 40


def keys(w, n_parents):
    M = w.M
    key = np.arange(M, dtype=np.int64)
    key[n_parents:] = GHOST + 8 * np.arange(M - n_parents, dtype=np.int64) + 3          # (any growing sequence above GHOST does)
    root = np.arange(M)
    gl = w.ghosts()
    for i in range(M):
        for g in gl[i]:
            root[g] = root[i] if i >= n_parents else i
    for g in range(n_parents, M):          # (a ghost listed under a ghost: up to its parent)
        while root[g] >= n_parents:
            assert root[root[g]] != root[g], "a ghost without a parent"
            root[g] = root[root[g]]
    return key, root


def rank_lists(view, key, root, owner, nranks, rng):
    """per rank: `glob` (the global row of every local row, shuffled) and `rows` (per local row its interaction rows, partner column in keys)"""
    out = []
    for r in range(nranks):
        mine = [i for i in range(view.M) if owner[root[i]] == r]
        need = set(mine)
        for i in mine:
            for row in view.rows[view.off[i]:view.off[i + 1]]:
                if int(row[0]) > 0:
                    need.add(int(row[0]) - 1)
        extra = rng.choice(view.M, size=min(view.M, 20), replace=False)
        glob = np.array(sorted(need | set(int(e) for e in extra)))
        rng.shuffle(glob)
        rows = []
        for g in glob:
            rr_ = view.rows[view.off[g]:view.off[g + 1]].copy()
            for row in rr_:
                if row[0] > 0:
                    row[0] = float(key[int(row[0]) - 1] + 1)
            rows.append(rr_)
        out.append(dict(glob=glob, rows=rows))
    return out


def local_table(view, key, root, owner, r, local, s, topo_n):
    """the entries rank r emits, in local row order then first-passing-row order; the rows it evaluated; its draws; the ghost keys of its roots"""
    glob = local["glob"]
    lkey = key[glob]
    by_key = {int(k): p for p, k in enumerate(lkey)}
    h, area, cx, cy, rmax, status = (a[glob] for a in (view.h, view.area, view.cx, view.cy, view.rmax, view.status))
    entries, evaluated, draws, gkeys = [], [], 0, []
    for i in range(len(glob)):
        if owner[root[glob[i]]] != r:
            continue
        evaluated.append(int(glob[i]))
        if lkey[i] >= GHOST:
            gkeys.append(int(lkey[i]))
        ridge, raft = h[i] <= s["max_floe_ridge_height"], h[i] <= s["max_floe_raft_height"]
        draws += int(ridge) + int(raft)
        rows = local["rows"][i]
        if not ((ridge or raft) and status[i] == rr.ACTIVE and len(rows) > 0):
            continue
        seen = set()
        for row in rows:
            j = int(row[0])
            if j > 0:
                p = by_key.get(j - 1)
                if p is None:
                    continue
                valid = bool(lkey[i] < lkey[p] and status[p] == rr.ACTIVE and ((cx[i] - cx[p]) ** 2 + (cy[i] - cy[p]) ** 2) < (rmax[i] + rmax[p]) ** 2)
                min_area = min(area[i], area[p])
            else:
                valid = view.valid(int(glob[i]), j)          # (the boundaries and the topography: the row's own columns, the same bits on every rank)
                min_area = area[i]
            if not valid:
                continue
            f = row[6] / min_area
            if not (1e-6 < f < 0.95):
                continue
            k = 0
            if j > 0:
                if ridge and h[p] <= s["max_floe_ridge_height"] and (h[i] >= s["min_ridge_height"] or h[p] >= s["min_ridge_height"]):
                    k |= rr.RIDGE
                if raft and h[p] <= s["max_floe_raft_height"]:
                    k |= rr.RAFT
            else:
                if ridge and h[i] <= s["max_domain_ridge_height"]:
                    k |= rr.RIDGE
                if raft and h[i] <= s["max_domain_raft_height"]:
                    k |= rr.RAFT
            if k == 0 or j in seen:
                continue
            seen.add(j)
            entries.append((int(lkey[i]), j - 1 if j > 0 else j, k, float(f)))
    return entries, evaluated, draws, gkeys


def merge(tables, gkeys, n_parents):
    """[(i, j, kind, frac)] in the single context's numbering (j as the rows name it) and order"""
    gk = sorted(set(k for g in gkeys for k in g))
    assert len(gk) == sum(len(g) for g in gkeys), "a ghost key gathered twice"
    place = {k: n_parents + p for p, k in enumerate(gk)}
    num = lambda k: k if k < GHOST else place[k]
    out = [(num(ki), num(kj) + 1 if kj >= 0 else kj, k, f) for t in tables for ki, kj, k, f in t]
    return [out[p] for p in sorted(range(len(out)), key=lambda p: out[p][0])]          # (sorted() is stable: the emitting rank's order stays)

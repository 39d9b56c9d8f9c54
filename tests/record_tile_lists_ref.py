"""The rule of the list sections of tile floe frames in numpy ("Tiled contexts", the lists): the yardstick of the list kernels of
csrc/sz_record_tile.hpp, independent of them, in the shape of tests/record_tiles_ref.py.

A tile frame with lists is record_tiles_ref's tile frame plus, over the SAME local rows,
  sub_off, sx, sy        a parent row's own points, a ghost row its root parent's (the parent is local: a ghost goes with its root parent)
  inter_off, inter_rows  a parent row's rows of the last step that ran, a ghost row none; the partner column (column 0) UNTRANSLATED: a negative
                         boundary / topography code, a floe's global number + 1, or (above 2^40) the order key + 1 of a ghost of the LAST step
  lkeys                  the rank's key table of the last step, sorted: the keys of the ghosts it made then -- of its own parents, and of halo
                         floes -- and possibly keys of halo parents (< 2^40), which count for nothing
merge() gives the single context's frame: rows by order key, both offsets a scan of the rows' counts in key order, the payload moving with its
row, and a partner key + 1 turned into N_global + (rank of the key among the sorted DISTINCT ghost keys of all ranks' tables) + 1.  That rank is
the ghost's place in the single context's ghost list of the last step BECAUSE which ghosts a parent gets depends on the parent alone: a ghost a
rank made of a halo floe is also made by the floe's owner, under the same key, so the distinct union of the tables is exactly the ghost list of
that step (§9e), however the floes are owned.  A key found in no table stays as it is."""
import numpy as np

import record_tiles_ref as rec

GHOST = rec.GHOST
LIMIT = float(GHOST)          # a partner above this is 1 + an order key
LISTS = ("inter_off", "inter_rows", "sub_off", "sx", "sy")
EXTRA = LISTS + ("lkeys", "lists")


def _spans(off, rows):
    """the elements of the CSR spans of `rows`, one span behind the other, and the spans' lengths"""
    off = np.asarray(off, np.int64)
    n = (off[1:] - off[:-1])[rows] if len(rows) else np.zeros(0, np.int64)
    sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in rows]).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
    return sel, n


def _offsets(n):
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def cut(frame, last_ghost_keys, owner, key, root, last_root, nranks, rng, pad=True):
    """the frame of a whole list with lists (partner column untranslated) cut into tile frames: record_tiles_ref.split over the columns -- row i
    goes to rank owner[root[i]], a rank's ghost rows shuffled --, the list spans of a rank's rows in its local row order, and its key table: the
    last step's ghost keys whose root parent (last_root) it owns; pad: also keys of some parents it does not own and of some ghosts of others,
    some of them twice"""
    cols = {k: v for k, v in frame.items() if k not in EXTRA}
    cols["_row"] = np.arange(frame["M"], dtype=np.int64)
    tiles = rec.split(cols, key, root, owner, nranks, rng)
    last = np.asarray(last_ghost_keys, np.int64)
    for r, t in enumerate(tiles):
        rows = t.pop("_row")
        if "sub_off" in frame:
            sel, n = _spans(frame["sub_off"], rows)
            t["sub_off"], t["sx"], t["sy"] = _offsets(n), np.asarray(frame["sx"])[sel], np.asarray(frame["sy"])[sel]
        if "inter_off" in frame:
            sel, n = _spans(frame["inter_off"], rows)
            t["inter_off"], t["inter_rows"] = _offsets(n), np.asarray(frame["inter_rows"], np.float64).reshape(-1, 7)[sel]
            mine = last[np.asarray(owner)[np.asarray(last_root)] == r] if len(last) else last
            table = [mine]
            if pad:
                foreign = last[np.asarray(owner)[np.asarray(last_root)] != r] if len(last) else last
                halo = np.nonzero(np.asarray(owner) != r)[0].astype(np.int64)
                if len(foreign):
                    f = rng.choice(foreign, size=min(len(foreign), 9), replace=False)
                    table += [f, f[:3]]          # (a foreign ghost this rank made of a halo floe, some twice)
                if len(halo):
                    table.append(rng.choice(halo, size=min(len(halo), 7), replace=False))
            t["lkeys"] = np.sort(np.concatenate(table)).astype(np.int64)
    return tiles


def merge(tiles):
    """the merged frame of tile frames with lists.  No order of a frame's rows or of the frames is assumed."""
    out = rec.merge([{k: v for k, v in t.items() if k not in EXTRA} for t in tiles])
    keys = np.concatenate([np.asarray(t["key"], np.int64) for t in tiles])
    order = np.argsort(keys, kind="stable")          # order[m]: the gathered row at merged place m
    N, M = out["N"], out["M"]

    def gather(off_name, payload):
        """offsets and payloads of the merged rows: a scan of the rows' counts in key order, every span moved whole"""
        n = np.concatenate([np.diff(np.asarray(t[off_name], np.int64)) for t in tiles]) if M else np.zeros(0, np.int64)
        base = np.concatenate([[0], np.cumsum([int(np.asarray(t[off_name])[-1]) for t in tiles])])
        start = np.concatenate([base[r] + np.asarray(t[off_name], np.int64)[:-1] for r, t in enumerate(tiles)]) if M else np.zeros(0, np.int64)
        sel = np.concatenate([np.arange(start[s], start[s] + n[s]) for s in order]).astype(np.int64) if M else np.zeros(0, np.int64)
        return n[order], [np.concatenate([np.asarray(t[p]) for t in tiles])[sel] for p in payload]

    if all("sub_off" in t for t in tiles):
        n, (sx, sy) = gather("sub_off", ("sx", "sy"))
        out["sub_off"], out["sx"], out["sy"] = _offsets(n), sx, sy
    if all("inter_off" in t for t in tiles):
        n, (rows,) = gather("inter_off", ("inter_rows",))
        assert not np.any(n[N:]), "a ghost row carries interactions"
        rows = np.array(rows, np.float64).reshape(-1, 7)
        table = np.concatenate([np.asarray(t["lkeys"], np.int64) for t in tiles])
        ghosts = np.unique(table[table >= GHOST])          # sorted, distinct: the single context's ghost list of the last step
        for q in np.nonzero(rows[:, 0] > LIMIT)[0]:
            k = int(rows[q, 0]) - 1
            a = int(np.searchsorted(ghosts, k))
            if a < len(ghosts) and ghosts[a] == k:
                rows[q, 0] = float(N + a + 1)
        out["inter_off"], out["inter_rows"] = _offsets(n), rows
    return out

"""The merge rule of tile floe frames in numpy ("Tiled contexts"): the yardstick of csrc/sz_record_tile.hpp, independent of it.

A tile frame is a dict in the layout of World.floe_frame over ONE rank's rows -- M, N, tstep, any of the per-row columns (doubles [M], tensors
[M, 4], id, ghost_id, status), the rings (vert_off, vx, vy), the ghost links (ghost_off, ghost_idx in LOCAL row numbers) -- plus `key`, the order
key of every local row.  merge() gives the frame of the whole list: the rows of all frames sorted by key, vert_off rebuilt from the rows' point
counts, ghost_off / ghost_idx rebuilt in merged row numbers.  No order of a frame's rows is assumed, and a row of any kind may carry links."""
import numpy as np

CSR = ("vert_off", "vx", "vy", "ghost_off", "ghost_idx")
SCALARS = ("tstep", "M", "N")
GHOST = 1 << 40          # the smallest key of a ghost row


def merge(frames):
    keys = np.concatenate([np.asarray(f["key"], np.int64) for f in frames])
    assert len(np.unique(keys)) == len(keys), "two rows carry the same order key"
    M = len(keys)
    assert M == sum(f["M"] for f in frames)
    row0 = np.concatenate([[0], np.cumsum([f["M"] for f in frames])]).astype(np.int64)
    order = np.argsort(keys, kind="stable")          # order[m]: the gathered row at merged place m
    pos = np.empty(M, np.int64); pos[order] = np.arange(M)
    first = frames[0]
    out = dict(tstep=first["tstep"], M=M, N=int(sum(f["N"] for f in frames)))
    assert all(f["tstep"] == first["tstep"] for f in frames)
    assert np.all(keys[order][:out["N"]] < GHOST) and np.all(keys[order][out["N"]:] >= GHOST), "parents first, then ghosts"
    for name in first:
        if name in CSR or name in SCALARS or name == "key":
            continue
        out[name] = np.concatenate([np.asarray(f[name]) for f in frames])[order]
    if "vert_off" in first:
        n = np.concatenate([np.diff(np.asarray(f["vert_off"], np.int64)) for f in frames])
        vbase = np.concatenate([[0], np.cumsum([len(f["vx"]) for f in frames])])          # a frame's first point among the gathered points
        start = np.concatenate([vbase[r] + np.asarray(f["vert_off"], np.int64)[:-1] for r, f in enumerate(frames)])
        vx = np.concatenate([f["vx"] for f in frames]); vy = np.concatenate([f["vy"] for f in frames])
        sel = np.concatenate([np.arange(start[s], start[s] + n[s]) for s in order]).astype(np.int64) if M else np.zeros(0, np.int64)
        out["vert_off"] = np.concatenate([[0], np.cumsum(n[order])]).astype(np.int32)
        out["vx"], out["vy"] = vx[sel], vy[sel]
    if "ghost_off" in first:
        off, idx = [0], []
        for s in order:
            r = int(np.searchsorted(row0, s, side="right") - 1)
            f = frames[r]; j = int(s - row0[r])
            for g in f["ghost_idx"][f["ghost_off"][j]:f["ghost_off"][j + 1]]:
                idx.append(pos[row0[r] + int(g)])
            off.append(len(idx))
        out["ghost_off"] = np.array(off, np.int32); out["ghost_idx"] = np.array(idx, np.int32)
    return out


def split(frame, key, root, owner, nranks, rng):
    """the frame of a whole list cut into tile frames: row i goes to the rank owner[root[i]] (a ghost goes with its root parent); a rank's parents
    keep their order, its ghost rows are shuffled; ghost_idx is rewritten in local row numbers"""
    M, N = frame["M"], frame["N"]
    out = []
    for r in range(nranks):
        par = [i for i in range(N) if owner[root[i]] == r]
        gh = [i for i in range(N, M) if owner[root[i]] == r]
        rows = np.array(par + [gh[k] for k in rng.permutation(len(gh))], np.int64)
        local = {int(g): j for j, g in enumerate(rows)}
        t = dict(tstep=frame["tstep"], M=len(rows), N=len(par), key=np.asarray(key, np.int64)[rows] if len(rows) else np.zeros(0, np.int64))
        for name, v in frame.items():
            if name in CSR or name in SCALARS:
                continue
            t[name] = np.asarray(v)[rows]
        if "vert_off" in frame:
            o = np.asarray(frame["vert_off"], np.int64)
            n = np.diff(o)[rows]
            sel = np.concatenate([np.arange(o[i], o[i + 1]) for i in rows]).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
            t["vert_off"] = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
            t["vx"], t["vy"] = np.asarray(frame["vx"])[sel], np.asarray(frame["vy"])[sel]
        if "ghost_off" in frame:
            off, idx = [0], []
            for i in rows:
                idx += [local[int(g)] for g in frame["ghost_idx"][frame["ghost_off"][i]:frame["ghost_off"][i + 1]]]
                off.append(len(idx))
            t["ghost_off"] = np.array(off, np.int32); t["ghost_idx"] = np.array(idx, np.int32)
        out.append(t)
    return out


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_frames_equal(got, want, where):
    assert sorted(k for k in got if k != "key") == sorted(k for k in want if k != "key"), (where, sorted(got), sorted(want))
    for k, v in want.items():
        if k == "key":
            continue
        if k in SCALARS:
            assert got[k] == v, (where, k, got[k], v)
        else:
            assert same(got[k], v), (where, k)

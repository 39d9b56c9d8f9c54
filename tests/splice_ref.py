"""What an edit of the floe list means, written once with numpy: `apply` is deleteat! / assignment in place / append! on the full host columns
and CSR lists.  The oracle of tests/test_splice_gpu.py is a fresh World loaded with apply's result, so nothing here touches the device.

A floe list ("columns") is a dict in the layout of World.download_rows: one entry per floe in every scalar column (the names of capi.DCOLS,
id, ghost_id, status), (n, 4) in the tensor columns (capi.TCOLS), and three CSR lists -- the rings (vert_off, vx, vy), the sub-floe points
(sub_off, sx, sy) and floe.interactions (inter_off, inter_rows (k, 7)).

The second half makes new floes with what the repository has: a floe cut by a line through its centroid (oracle.orc.clip against two
half-plane rectangles), a ring scaled about its centroid, a ring resampled to more points; derived properties from subzero_jl_amd.floe,
sub-floe points from fields.subgrid_points."""
import numpy as np

CSR = (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy")), ("inter_off", ("inter_rows",)))
CSR_NAMES = {n for off, vals in CSR for n in (off,) + vals}


def n_rows(cols):
    return len(cols["vert_off"]) - 1


def _split(cols):
    """per floe: ({scalar / tensor column: entry}, {CSR value name: its slice})"""
    n = n_rows(cols)
    rows = []
    for i in range(n):
        r = {k: np.array(v[i]) for k, v in cols.items() if k not in CSR_NAMES}
        for off, vals in CSR:
            o = cols[off]
            for v in vals:
                r[v] = np.array(cols[v][o[i] - o[0]:o[i + 1] - o[0]])
        rows.append(r)
    return rows


def _join(rows, like):
    out = {}
    for k, v in like.items():
        if k in CSR_NAMES:
            continue
        out[k] = np.array([r[k] for r in rows], dtype=v.dtype).reshape((len(rows),) + v.shape[1:])
    for off, vals in CSR:
        n = np.array([len(r[vals[0]]) for r in rows], np.int64)
        out[off] = np.concatenate([[0], np.cumsum(n)]).astype(like[off].dtype)
        for v in vals:
            parts = [r[v] for r in rows]
            out[v] = np.concatenate(parts).astype(like[v].dtype) if parts else like[v][:0].copy()
            if like[v].ndim == 2:
                out[v] = out[v].reshape(-1, like[v].shape[1])
    return out


def apply(cols, delete=(), replace=None, append=None):
    """the edited list: replace = (rows, floes) overwrites the rows `rows` -- numbers of the list BEFORE the deletion -- with the floes given,
    `delete` removes rows (the kept ones keep their order), `append` puts its floes behind the last kept row in the order given"""
    rows = _split(cols)
    n = len(rows)
    delete = [int(d) for d in delete]
    assert all(0 <= d < n for d in delete) and len(set(delete)) == len(delete)
    if replace is not None:
        idx, new = replace
        new = _split(new)
        assert len(idx) == len(new) and len(set(int(i) for i in idx)) == len(idx)
        for i, r in zip(idx, new):
            assert 0 <= int(i) < n and int(i) not in delete
            rows[int(i)] = r
    gone = set(delete)
    rows = [r for i, r in enumerate(rows) if i not in gone]
    if append is not None:
        rows += _split(append)
    assert rows, "the edit leaves no floe"
    return _join(rows, cols)


def take(cols, idx):
    """the floes idx of a list, as a list of their own"""
    rows = _split(cols)
    return _join([rows[int(i)] for i in idx], cols)


# ---------------------------------------------------------------- new floes
def _area(r):
    return 0.5 * abs(np.sum(r[:-1, 0] * r[1:, 1] - r[1:, 0] * r[:-1, 1]))


def _centroid(r):
    from subzero_jl_amd import floe as floe_mod
    d = floe_mod.derive(np.array([0, len(r)]), r[:, 0].copy(), r[:, 1].copy(), 1.0)
    return float(d["cx"][0]), float(d["cy"][0]), float(d["rmax"][0])


def scaled(ring, f):
    """the ring scaled by f about its centroid"""
    cx, cy, _ = _centroid(ring)
    r = np.array([cx, cy]) + f * (ring - np.array([cx, cy]))
    r[-1] = r[0]
    return r


def resampled(ring):
    """every edge split at its midpoint: twice the edges, the same shape"""
    mid = 0.5 * (ring[:-1] + ring[1:])
    r = np.empty((2 * (len(ring) - 1) + 1, 2))
    r[0:-1:2] = ring[:-1]; r[1:-1:2] = mid; r[-1] = ring[0]
    return r


def halves(ring, vertical=True):
    """the ring cut by the vertical (horizontal) line through its centroid: the largest region on either side, each shrunk by 2 % about
    its own centroid so that the pieces do not touch"""
    from oracle import orc
    from subzero_jl_amd import floe as floe_mod
    cx, cy, rm = _centroid(ring)
    B = 4.0 * rm
    if vertical:
        boxes = [(cx - B, cx, cy - B, cy + B), (cx, cx + B, cy - B, cy + B)]
    else:
        boxes = [(cx - B, cx + B, cy - B, cy), (cx - B, cx + B, cy, cy + B)]
    out = []
    for x0, x1, y0, y1 in boxes:
        rect = np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0], [x0, y0]])
        regions = [floe_mod.valid_ring(r) for r in orc.clip(ring, rect) if len(r) >= 4]
        assert regions, "the cut left nothing on one side"
        out.append(scaled(max(regions, key=_area), 0.98))
    return out


def pieces3(ring):
    """three pieces of a floe: cut once, then the second half cut across"""
    a, b = halves(ring, True)
    return [a] + halves(b, False)


def floes_from(rings, like, ids, dg, height=None, inter=None):
    """a list of the floes with these rings: derived columns from the ring (subzero_jl_amd.floe.derive), sub-floe points from
    fields.subgrid_points, every other column -- velocities, previous-step values, stresses -- copied from `like` (a list with one floe per
    ring, e.g. download_rows of the parents); inter: per floe its interaction rows (k, 7), default none"""
    from subzero_jl_amd import fields, floe as floe_mod
    n = len(rings)
    assert n_rows(like) == n
    out = {k: np.array(v) for k, v in like.items() if k not in CSR_NAMES}
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    h = out["height"] if height is None else np.broadcast_to(np.asarray(height, np.float64), (n,)).copy()
    d = floe_mod.derive(off, vx, vy, h)
    for k in ("cx", "cy", "area", "mass", "moment", "rmax", "height"):
        out[k] = d[k]
    out["id"] = np.asarray(ids, np.int64); out["ghost_id"] = np.zeros(n, np.int64)
    out["vert_off"], out["vx"], out["vy"] = off, vx, vy
    so = [0]; sxs = []; sys_ = []
    for i, r in enumerate(rings):
        sx, sy = fields.subgrid_points(r, d["cx"][i], d["cy"][i], dg)
        so.append(so[-1] + len(sx)); sxs.append(sx); sys_.append(sy)
    out["sub_off"] = np.array(so, np.int32); out["sx"] = np.concatenate(sxs); out["sy"] = np.concatenate(sys_)
    inter = [np.zeros((0, 7))] * n if inter is None else [np.asarray(r, np.float64).reshape(-1, 7) for r in inter]
    out["inter_off"] = np.concatenate([[0], np.cumsum([len(r) for r in inter])]).astype(np.int32)
    out["inter_rows"] = np.concatenate(inter).reshape(-1, 7)
    return out


def ring_of(cols, i):
    o = cols["vert_off"]
    return np.stack([cols["vx"][o[i]:o[i + 1]], cols["vy"][o[i]:o[i + 1]]], 1)


def inter_of(cols, i):
    o = cols["inter_off"]
    return cols["inter_rows"][o[i]:o[i + 1]]

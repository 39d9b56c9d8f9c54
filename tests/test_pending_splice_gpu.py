"""A ridge / raft stop as row edits: sz_ridgeraft_rows against the numpy statement of the closure rule
(tests/ridgeraft_rows_ref.py), sz_download_list_rows against the rows of a full download, and sz_splice_parents against the long path it
replaces -- the parents and their interaction lists uploaded again, as tests/test_ridgeraft_gpu.py::_edit_and_upload does it.  Every comparison
is on bits; nothing here has a tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import ridgeraft_rows_ref as rrr
import splice_ref as sp

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
STATS = ("M", "N", "n_ring_points", "n_sub_points", "n_inter_rows")
GHOST_KEYS = ("ghost_off", "ghost_idx")


def mk(ftype=np.float64, **env):
    import subzero_jl_amd
    os.environ.update(env)
    try:
        return subzero_jl_amd.World(0, ftype=ftype)
    finally:
        for k in env:
            del os.environ[k]


# ---------------------------------------------------------------- states
def _dense():
    """the 400-floe dense periodic field that tests/test_ridgeraft_gpu.py stops at tstep 10"""
    from subzero_jl_amd import fields
    return fields.make_config(n_floes=400, seed=7, subgrid_per_floe=4.0)


def _stopped(cfg, setup=None, env=None, ftype=np.float64):
    """a batch of 40 from tstep 1 with ridge / raft dt = 10, stopped before the second half of tstep 10"""
    from subzero_jl_amd import fields
    w = fields.build_world(mk(ftype, **(env or {})), cfg)
    if setup:
        setup(w, cfg)
    w.set_ridgeraft(True, dt=10)
    assert w.run(40, 1, cfg["dt"], coupling_dt=1) == 9
    assert w.ridgeraft_pending() == 10
    return w


def _by_hand(cfg, ftype=np.float64):
    """9 steps, then add_ghosts + timestep_collisions by hand: the same list, nothing pending"""
    from subzero_jl_amd import fields
    w = fields.build_world(mk(ftype), cfg)
    assert w.run(9, 1, cfg["dt"], coupling_dt=1) == 9
    w.add_ghosts(); w.timestep_collisions(cfg["n_floes"], cfg["dt"])
    return w


def _full_list(w):
    """everything downloadable of the WHOLE list, one entry per list row, in the layout of download_list_rows: the columns, the rings, the
    sub-floe points (a ghost row has none), floe.interactions and the ghost lists"""
    from subzero_jl_amd import capi
    w._push_interactions()
    w._host_stale = True
    c = {n: w.get(n) for n in capi.DCOLS}
    for n, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        c[n] = np.stack([w.get(pre + q) for q in ("11", "12", "21", "22")], 1)
    c["id"], c["ghost_id"], c["status"] = w.ids()
    m = len(c["id"])
    off, x, y = w.rings()
    c["vert_off"], c["vx"], c["vy"] = off.copy(), x.copy(), y.copy()
    so, sx, sy = w.subpoints()
    c["sub_off"] = np.concatenate([so, np.full(m - (len(so) - 1), so[-1])]).astype(np.int32)
    c["sx"], c["sy"] = sx.copy(), sy.copy()
    io, ir = w.interactions()
    c["inter_off"], c["inter_rows"] = io.copy(), ir.copy().reshape(-1, 7)
    gl = w.ghosts()
    c["ghost_off"] = np.concatenate([[0], np.cumsum([len(g) for g in gl])]).astype(np.int32)
    c["ghost_idx"] = np.array([g for l in gl for g in l], np.int32)
    assert len(c["vert_off"]) == len(c["inter_off"]) == len(c["ghost_off"]) == m + 1
    return c


def _state(w):
    c = _full_list(w)
    st = w.stats()
    c["stats"] = np.array([st[k] for k in STATS], np.int64)
    c["origin"] = w.origin()
    c["pending"] = np.array([w.ridgeraft_pending()], np.int64)
    return c


def _assert_bit_equal(a, b, where=""):
    assert sorted(a) == sorted(b), where
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (where, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        if a[k].size == 0:
            continue
        x, y = (np.ascontiguousarray(v).reshape(len(v), -1).view(np.uint8) for v in (a[k], b[k]))
        assert np.array_equal(x, y), (where, k, "first entries that differ:", list(np.nonzero(np.any(x != y, axis=1))[0][:8]), "of", len(x))


def _no_ghost_lists(c):
    return {k: v for k, v in c.items() if k not in GHOST_KEYS}


def _table(w):
    i, j, _, _, _ = w.ridgeraft_candidates()
    return list(zip(i.tolist(), j.tolist()))


@pytest.fixture(scope="module")
def pending():
    """one context at the pending stop, its full download and its table -- shared by the tests that only read"""
    cfg = _dense()
    w = _stopped(cfg)
    full = _full_list(w)
    assert w.M > cfg["n_floes"], "the periodic field has no ghosts in its list"
    return w, cfg, full, _table(w)


# ---------------------------------------------------------------- 1. sz_ridgeraft_rows
def test_rows_at_the_pending_stop(pending):
    w, cfg, full, table = pending
    want = rrr.closure(full["id"], cfg["n_floes"], full["ghost_off"], full["ghost_idx"], table)
    got = w.ridgeraft_rows()
    print("pending stop: %d table entries, closure of %d rows (%d ghosts) in a list of %d" % (len(table), len(got), int(np.sum(got >= cfg["n_floes"])), w.M))
    assert got.dtype == np.int32 and len(table) > 0 and len(got) > 0
    assert np.array_equal(got, want)
    assert np.all(np.diff(got) > 0) and got[0] >= 0 and got[-1] < w.M
    assert np.array_equal(w.ridgeraft_rows(), got), "two calls"
    assert _table(w) == table and w.ridgeraft_pending() == 10
    _assert_bit_equal(_full_list(w), full, "the call changes nothing")


def test_rows_on_a_list_made_by_hand(pending):
    w, cfg, full, table = pending
    b = _by_hand(cfg)
    b.set_ridgeraft(True, dt=10)
    assert _table(b) == table
    got = b.ridgeraft_rows()
    assert np.array_equal(got, rrr.closure_of_world(b, table))
    assert np.array_equal(got, w.ridgeraft_rows())


def _square(cx, cy, side=4e3):
    h = side / 2
    return np.array([[cx - h, cy - h], [cx - h, cy + h], [cx + h, cy + h], [cx + h, cy - h], [cx - h, cy - h]])


L_HAND = 1e5
# parents (centres), then ghosts as (parent, shift in domain lengths): 2 and 6 have one ghost, 4 -- in the corner -- three, 5 two (a list no ghost
# maker produces, but an upload may bring)
HAND_PARENTS = [(5.0e4, 5.0e4), (5.3e4, 5.0e4), (1.5e3, 3.0e4), (4.5e3, 3.0e4), (1.5e3, 1.5e3), (3.0e4, 1.5e3), (9.85e4, 3.0e4), (5.0e4, 9.75e4),
                (5.3e4, 2.0e4)]
HAND_GHOSTS = [(2, 1, 0), (4, 1, 0), (4, 1, 1), (4, 0, 1), (5, 0, 1), (5, 1, 0), (6, -1, 0)]          # list rows 9 .. 15
HAND_TOPO = (5.0e4, 2.0e4)


def _hand_list_world():
    """the hand-made list uploaded WITH its ghosts (ghost_off / ghost_idx), all four walls periodic, one topography square; every floe a square
    of height 0.25, which passes every height gate of the default settings"""
    from subzero_jl_amd import capi, floe as floe_mod
    n = len(HAND_PARENTS)
    centres = list(HAND_PARENTS) + [(HAND_PARENTS[p][0] + dx * L_HAND, HAND_PARENTS[p][1] + dy * L_HAND) for p, dx, dy in HAND_GHOSTS]
    rings = [_square(x, y) for x, y in centres]
    m = len(rings)
    off = (5 * np.arange(m + 1)).astype(np.int32)
    xy = np.concatenate(rings)
    d = floe_mod.derive(off, xy[:, 0].copy(), xy[:, 1].copy(), np.full(m, 0.25))
    ids = np.array([i + 1 for i in range(n)] + [p + 1 for p, _, _ in HAND_GHOSTS], np.int64)
    gid = np.zeros(m, np.int64)
    lists = [[] for _ in range(m)]
    for k, (p, _, _) in enumerate(HAND_GHOSTS):
        lists[p].append(n + k); gid[n + k] = len(lists[p])
    w = mk()
    w.set_consts(); w.set_settings()
    w.set_domain([capi.PERIODIC] * 4, 0.0, L_HAND, 0.0, L_HAND)
    w.set_topography([_square(*HAND_TOPO)])
    w.load_columns(dict(cx=d["cx"], cy=d["cy"], rmax=d["rmax"], area=d["area"], height=d["height"], mass=d["mass"], moment=d["moment"],
                        id=ids, ghost_id=gid, vert_off=off, vx=xy[:, 0].copy(), vy=xy[:, 1].copy(),
                        ghost_off=np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32),
                        ghost_idx=np.array([g for l in lists for g in l], np.int32)), N=n)
    w.set_ridgeraft(True, dt=10)
    return w, d["area"]


# name -> (interaction rows as {list row i: [partner j as the rows name it, ...]}, the table they must give, the closure by hand)
HAND_CASES = {
    "two parents without ghosts": ({0: [2]}, [(0, 2)], [0, 1]),
    "a parent with one ghost": ({2: [4]}, [(2, 4)], [2, 3, 9]),
    "a parent with two ghosts (boundary partner)": ({5: [-2]}, [(5, -2)], [5, 13, 14]),
    "the corner floe's three ghosts (boundary partner)": ({4: [-4]}, [(4, -4)], [4, 10, 11, 12]),
    "i is a ghost (boundary partner)": ({12: [-1], 15: [-4]}, [(12, -1), (15, -4)], [4, 6, 10, 11, 12, 15]),
    "j is a ghost": ({6: [10]}, [(6, 10)], [2, 6, 9, 15]),
    "a topography partner": ({8: [-5]}, [(8, -5)], [8]),
    "one floe in many entries": ({2: [4, 16, -4], 6: [10, -3], 0: [2]}, [(0, 2), (2, 4), (2, 16), (2, -4), (6, 10), (6, -3)], [0, 1, 2, 3, 6, 9, 15]),
    "rows that fail the window: an empty table": ({0: [(2, 2.0)], 2: [(4, 2.0)]}, [], []),
}


def test_rows_on_hand_made_lists():
    w, area = _hand_list_world()
    m, n = len(area), len(HAND_PARENTS)
    assert w.M == m and w.N == n
    ids, gl = w.ids()[0], w.ghosts()
    assert [len(g) for g in gl[:n]] == [0, 0, 1, 0, 3, 2, 1, 0, 0] and gl[4] == [10, 11, 12] and gl[5] == [13, 14]
    for name, (rows, table, by_hand) in HAND_CASES.items():
        for i in range(m):
            r = []
            for e in rows.get(i, []):
                j, frac = e if isinstance(e, tuple) else (e, 0.01)
                r.append([float(j), 0.0, 0.0, 0.0, 0.0, 0.0, frac * (min(area[i], area[j - 1]) if j > 0 else area[i])])
            w.set_interactions(i, np.array(r).reshape(-1, 7))
        assert _table(w) == table, name
        got = w.ridgeraft_rows()
        assert got.tolist() == by_hand, (name, got.tolist())
        assert np.array_equal(got, rrr.closure_of_world(w, table)), name
        assert np.array_equal(w.ridgeraft_rows(), got), (name, "two calls")


def test_rows_repeats_the_refusals_of_the_candidates():
    from subzero_jl_amd import capi, fields
    cfg = fields.make_config(n_floes=400, seed=80, subgrid_per_floe=4.0)
    w = fields.build_world(mk(), cfg)
    w._push()
    L, h = w.L, w.h
    n = C.c_int32(5)
    assert L.sz_ridgeraft_rows(h, C.byref(n), 0, None) == E_STATE and n.value == 0 and b"sz_set_ridgeraft" in L.sz_last_error(h)          # not set
    w.set_ridgeraft(True, dt=10)
    assert L.sz_ridgeraft_rows(h, C.byref(n), 0, None) == E_STATE                                # a ghost-free list
    assert L.sz_ridgeraft_rows(h, None, 0, None) == E_ARG
    assert w.run(3, 1, cfg["dt"], coupling_dt=1) == 3
    assert L.sz_ridgeraft_rows(h, C.byref(n), 0, None) == E_STATE                                # ... after a batch too
    w.add_ghosts(); w.timestep_collisions(cfg["n_floes"], cfg["dt"])
    assert L.sz_ridgeraft_rows(h, C.byref(n), 0, None) == 0 and n.value > 1
    one = np.zeros(1, np.int32)
    assert L.sz_ridgeraft_rows(h, C.byref(n), 1, capi.ptr(one, capi._ip)) == E_ARG and n.value > 1          # room for fewer rows than the closure
    assert L.sz_ridgeraft_rows_f32(h, C.byref(n), 0, None) == 0 and n.value == len(w.ridgeraft_rows())
    w.remove_ghosts()
    assert w.run(2, 4, cfg["dt"], coupling_dt=1) == 2
    gidx = np.arange(w.N, dtype=np.int64)
    assert L.sz_tile_enable(h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    assert L.sz_ridgeraft_rows(h, C.byref(n), 0, None) == E_STATE and b"tiled" in L.sz_last_error(h)


# ---------------------------------------------------------------- 2. sz_download_list_rows
def _mixed_selection(m, n, k, seed):
    """k rows of a list of m with n parents, ghosts and parents in turn as long as there are ghosts, shuffled"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = rng.permutation(np.arange(n, m))[:k // 2]
    p = rng.permutation(n)[:k - len(g)]
    return rng.permutation(np.concatenate([g, p]))


def test_list_rows_of_the_closure_and_of_the_whole_list(pending):
    w, cfg, full, table = pending
    rows = w.ridgeraft_rows()
    _assert_bit_equal(w.download_list_rows(rows), rrr.take_list(full, rows), "closure")
    rev = np.arange(w.M)[::-1]
    _assert_bit_equal(w.download_list_rows(rev), rrr.take_list(full, rev), "all rows, reversed")
    _assert_bit_equal(w.download_list_rows([]), rrr.take_list(full, []), "no row")
    _assert_bit_equal(_full_list(w), full, "a download changes nothing")


@pytest.mark.parametrize("k", [1, 63, 64, 65, 257])
def test_list_rows_mixing_parents_and_ghosts(pending, k):
    w, cfg, full, table = pending
    n, m = cfg["n_floes"], w.M
    assert m >= 257
    rows = [m - 1] if k == 1 else _mixed_selection(m, n, k, k)
    assert len(rows) == k and any(r >= n for r in rows) and (k == 1 or any(r < n for r in rows))
    _assert_bit_equal(w.download_list_rows(rows), rrr.take_list(full, rows), k)


def test_list_rows_of_ghosts_alone_ghost_lists_and_empty_point_spans(pending):
    w, cfg, full, table = pending
    n, m = cfg["n_floes"], w.M
    ghosts = np.arange(n, m)
    got = w.download_list_rows(ghosts)
    _assert_bit_equal(got, rrr.take_list(full, ghosts), "ghosts alone")
    assert np.all(got["ghost_id"] > 0) and not got["sub_off"].any() and got["sx"].size == 0 and not got["ghost_off"].any() and got["ghost_idx"].size == 0
    assert got["inter_off"][-1] > 0, "no ghost of the stop has interaction rows"
    owners = np.array([i for i in range(n) if full["ghost_off"][i + 1] > full["ghost_off"][i]])
    got = w.download_list_rows(owners[::-1])
    _assert_bit_equal(got, rrr.take_list(full, owners[::-1]), "the parents that have ghosts")
    assert got["ghost_off"][-1] == m - n and sorted(got["ghost_idx"].tolist()) == ghosts.tolist() and np.all(np.diff(got["sub_off"]) > 0)
    for k, p in enumerate(owners[::-1]):
        assert np.all(full["id"][got["ghost_idx"][got["ghost_off"][k]:got["ghost_off"][k + 1]]] == full["id"][p])


def test_list_rows_on_the_walls_and_topography_field():
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=400, seed=3, walls=True, topography=True, ocean="strait", subgrid_per_floe=4.0)
    w = fields.build_world(mk(), cfg)
    assert w.run(20, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 20
    full = _full_list(w)
    assert full["inter_off"][-1] > 0
    rows = [399, 0, 17, 64, 63]
    _assert_bit_equal(w.download_list_rows(rows), rrr.take_list(full, rows))


def test_list_rows_f32_twin():
    """a Floe{Float32} host at the same point of the step, by hand: the values come down rounded as its full download rounds them"""
    cfg = _dense()
    w = _by_hand(cfg, ftype=np.float32)
    full = _full_list(w)
    n, m = cfg["n_floes"], w.M
    assert m > n
    rows = _mixed_selection(m, n, 65, 1)
    _assert_bit_equal(w.download_list_rows(rows), rrr.take_list(full, rows), "f32")


def _refused(w, call, code, needle, *args):
    from subzero_jl_amd.capi import SzError
    before = _state(w)
    with pytest.raises(SzError) as e:
        call(*args)
    msg = str(e.value)
    head = "libsubzero_hip error %d: " % code
    assert msg.startswith(head) and len(msg) > len(head) + 8 and needle in msg, msg
    _assert_bit_equal(_state(w), before, "a refusal changes nothing")


def test_list_rows_refusals_and_download_rows_as_before(pending):
    w, cfg, full, table = pending
    from subzero_jl_amd import capi
    n, m = cfg["n_floes"], w.M
    _refused(w, w.download_list_rows, E_ARG, "outside", [0, m])
    _refused(w, w.download_list_rows, E_ARG, "outside", [-1])
    _refused(w, w.download_list_rows, E_ARG, "repeats", [m - 1, 3, m - 1])
    # sz_download_rows: parents only, the bits of the full download, zeros in ghost_off
    _refused(w, w.download_rows, E_ARG, "outside", [n])
    rows = [n - 1, 0, 64, 63, 200]
    _assert_bit_equal(w.download_rows(rows), _no_ghost_lists(rrr.take_list(full, rows)), "download_rows")
    f = capi.SzFloeColumns()
    owner = int(np.nonzero(np.diff(full["ghost_off"][:n + 1]))[0][0])          # (a parent that has ghosts among the rows asked for)
    r32 = np.array([r for r in rows if r != owner] + [owner], np.int32)
    goff = np.full(len(r32) + 1, 7, np.int32); gidx = np.full(3 * len(r32), 7, np.int32)
    f.ghost_off = capi.ptr(goff, capi._ip); f.ghost_idx = capi.ptr(gidx, capi._ip)
    assert w.L.sz_download_rows(w.h, len(r32), capi.ptr(r32, capi._ip), C.byref(f), None, None, None) == 0
    assert not goff.any() and np.all(gidx == 7), "sz_download_rows writes zeros in ghost_off and leaves ghost_idx alone"


# ---------------------------------------------------------------- 3. sz_splice_parents against the long path
def _ridge_edit(w, n, dg):
    """what a host's ridging would send back, made from download_list_rows of the closure: every parent of the closure replaced -- the first two
    by the left half of their ring, the others with the volume add_floe_volume! would give them --, the two right halves appended as new floes.
    Returns (rows replaced, their floes, the appended floes)."""
    rows = w.ridgeraft_rows()
    sel = _no_ghost_lists(w.download_list_rows(rows))
    parents = [int(r) for r in rows if r < n]
    assert len(parents) >= 3 and len(parents) < len(rows), "the closure has no ghost, or too few parents"
    where = {int(r): k for k, r in enumerate(rows)}
    next_id = int(w.ids()[0].max()) + 1
    rep, app = [], []
    for q, p in enumerate(parents):
        one = sp.take(sel, [where[p]])
        if q < 2:
            left, right = sp.halves(sp.ring_of(one, 0))
            app.append(sp._split(sp.floes_from([right], one, [next_id + q], dg))[0])
            one = sp.floes_from([left], one, one["id"], dg, inter=[sp.inter_of(one, 0)])
        else:
            vol = 0.05 * one["area"][0] * one["height"][0]
            one["height"][0] = (one["height"][0] * one["area"][0] + vol) / one["area"][0]
            one["mass"][0] = one["area"][0] * one["height"][0] * 920.0
        rep.append(sp._split(one)[0])
    return parents, sp._join(rep, sel), sp._join(app, sel)


def _long_path(w, n, rep_rows, rep, app):
    """the route of tests/test_ridgeraft_gpu.py::_edit_and_upload: the whole list and its rows come down, the parents are edited on the host and
    go up alone, with their sub-floe points and their interaction lists"""
    full = _no_ghost_lists(rrr.take_list(_full_list(w), np.arange(n)))
    edited = sp.apply(full, (), (rep_rows, rep) if len(rep_rows) else None, app)
    w.load_columns({k: v for k, v in edited.items() if k not in ("sub_off", "sx", "sy", "inter_off", "inter_rows")})
    w.set_subpoints_csr(edited["sub_off"], edited["sx"], edited["sy"])
    for i in range(sp.n_rows(edited)):
        w.set_interactions(i, sp.inter_of(edited, i))
    w._push_interactions()


def _mixed(w, cfg):
    w.set_precision("mixed")


PATHS = {"pipelined": (None, None), "three_launch": (None, {"SZ_PIPELINE": "0"}), "mixed": (_mixed, None)}


@pytest.mark.parametrize("path", list(PATHS))
def test_splice_parents_equals_the_long_path(path):
    setup, env = PATHS[path]
    cfg = _dense()
    n, dt = cfg["n_floes"], cfg["dt"]
    A, B = _stopped(cfg, setup, env), _stopped(cfg, setup, env)
    _assert_bit_equal(_state(A), _state(B), "two contexts at the same pending step")
    rep_rows, rep, app = _ridge_edit(B, n, cfg["dg"])
    assert sp.n_rows(app) == 2
    _long_path(A, n, rep_rows, rep, app)
    B.splice_parents((), (rep_rows, rep), app)
    for w in (A, B):
        assert w.ridgeraft_pending() == 10 and w.stats()["M"] == w.stats()["N"] == n + 2
    _assert_bit_equal(_state(A), _state(B), (path, "edited"))
    for w in (A, B):
        w.finish_step(10, dt, coupling_dt=1)
    _assert_bit_equal(_state(A), _state(B), (path, "finished"))
    for w in (A, B):
        w.set_ridgeraft(False)
        assert w.run(20, 11, dt, coupling_dt=1, stop_on_tags=False) == 20
    assert A.pipelined() == B.pipelined() and bool(A.pipelined()) == (path != "three_launch" and (path == "pipelined" or bool(A.pipelined())))
    _assert_bit_equal(_state(A), _state(B), (path, "20 steps on"))


def _overlapping_hand_cfg():
    """three hand-made floes in a periodic domain with room for 2 200: the first crosses the west wall (it gets a ghost), the second overlaps it"""
    import test_splice_gpu as tsg
    from subzero_jl_amd import fields, floe as floe_mod
    cfg = dict(tsg._hand_cfg(3, room=2200))
    off, vx, vy = cfg["vert_off"], cfg["vx"].copy(), cfg["vy"].copy()
    vx[off[0]:off[1]] -= 7.0e3
    vx[off[1]:off[2]] -= 2.0e4
    cfg["vx"] = vx
    d = cfg["derived"] = floe_mod.derive(off, vx, vy, cfg["height"])
    so, sxs, sys_ = [0], [], []
    for i in range(3):
        sx, sy = fields.subgrid_points(np.stack([vx[off[i]:off[i + 1]], vy[off[i]:off[i + 1]]], 1), d["cx"][i], d["cy"][i], cfg["dg"])
        so.append(so[-1] + len(sx)); sxs.append(sx); sys_.append(sy)
    cfg["sub_off"] = np.array(so, np.int32); cfg["sx"] = np.concatenate(sxs); cfg["sy"] = np.concatenate(sys_)
    return cfg


def test_growth_of_rows_rings_and_points_at_once_while_pending():
    """3 floes stopped at their first ridge / raft step, 2 100 triangles appended: rows, ring points and the sub-floe pool all outgrow the upload's"""
    import test_splice_gpu as tsg
    from subzero_jl_amd import fields
    cfg = _overlapping_hand_cfg()
    worlds = []
    for _ in range(2):
        w = fields.build_world(mk(), cfg)
        w.set_ridgeraft(True, dt=2)
        assert w.run(10, 1, cfg["dt"], coupling_dt=1) == 1 and w.ridgeraft_pending() == 2
        worlds.append(w)
    A, B = worlds
    assert B.M > 3 and len(B.ridgeraft_rows()) >= 3
    like = _no_ghost_lists(B.download_list_rows([k % 3 for k in range(3)]))
    new = [tsg._hand_ring(k, cfg["n_side"], cfg["spacing"], cfg["side"], triangle=True) for k in range(3, 2103)]
    app = sp.floes_from(new, sp.take(like, [k % 3 for k in range(2100)]), np.arange(10, 2110), cfg["dg"])
    _long_path(A, 3, [], None, app)
    B.splice_parents(append=app)
    assert B.stats()["N"] == B.stats()["M"] == 2103 and B.ridgeraft_pending() == 2
    _assert_bit_equal(_state(A), _state(B), "grown")
    for w in (A, B):
        w.finish_step(2, cfg["dt"], coupling_dt=1)
        w.set_ridgeraft(False)
        assert w.run(5, 3, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 5
    _assert_bit_equal(_state(A), _state(B), "grown, finished, 5 steps on")


def _settled_pair():
    import test_splice_gpu as tsg
    (D1, cfg), (D2, _) = tsg._settled("periodic"), tsg._settled("periodic")
    edit = tsg._edit("ridge", tsg._full(D1), cfg)
    return D1, D2, cfg, edit


def test_ghosts_by_hand_without_a_pending_step_equals_remove_ghosts_and_splice():
    D1, D2, cfg, edit = _settled_pair()
    for w in (D1, D2):
        w.add_ghosts()
        assert w.stats()["M"] > w.stats()["N"]
    D1.splice_parents(*edit)
    D2.remove_ghosts(); D2.splice(*edit)
    _assert_bit_equal(_state(D1), _state(D2), "by hand")
    for w in (D1, D2):
        assert w.run(10, 20, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 10
    _assert_bit_equal(_state(D1), _state(D2), "by hand, 10 steps on")


def test_without_ghosts_it_is_splice():
    D1, D2, cfg, edit = _settled_pair()
    D1.splice_parents(*edit)
    D2.splice(*edit)
    _assert_bit_equal(_state(D1), _state(D2), "no ghosts")
    for w in (D1, D2):
        assert w.run(10, 20, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 10
    _assert_bit_equal(_state(D1), _state(D2), "no ghosts, 10 steps on")


def test_refusals_leave_the_ghosts_in_the_list():
    cfg = _dense()
    n = cfg["n_floes"]
    w = _stopped(cfg)
    m = w.M
    sel = _no_ghost_lists(w.download_list_rows([50, 60]))
    ok, two = sp.take(sel, [0]), sel
    _refused(w, w.splice_parents, E_ARG, "ascending", [5, 3], None, None)
    _refused(w, w.splice_parents, E_ARG, "repeats", [5, 5], None, None)
    _refused(w, w.splice_parents, E_ARG, "outside", [n], None, None)          # (a ghost row: the rows number the parents)
    _refused(w, w.splice_parents, E_ARG, "outside", [-1], None, None)
    _refused(w, w.splice_parents, E_ARG, "outside", (), ([m], ok), None)
    _refused(w, w.splice_parents, E_ARG, "ascending", (), ([60, 50], two), None)
    _refused(w, w.splice_parents, E_ARG, "both deleted and replaced", [50], ([50], ok), None)
    _refused(w, w.splice_parents, E_ARG, "no floe", list(range(n)), None, None)
    opened = {k: v.copy() for k, v in ok.items()}
    opened["vx"][-1] += 1.0
    _refused(w, w.splice_parents, E_ARG, "open ring", (), ([50], opened), None)
    th = np.linspace(0.0, -2.0 * np.pi, 300)
    ring = np.stack([ok["cx"][0] + 5e3 * np.cos(th), ok["cy"][0] + 5e3 * np.sin(th)], 1); ring[-1] = ring[0]
    long_ = sp.floes_from([ring], ok, [7000], cfg["dg"])
    _refused(w, w.splice_parents, E_ARG, "255", (), ([50], long_), None)
    _refused(w, w.splice_parents, E_ARG, "255", (), None, long_)
    # sz_splice_floes still refuses this state, and names the way out
    _refused(w, w.splice, E_STATE, "sz_step_finish", [0], None, None)
    # the all-empty edit is no edit: nothing changes, the ghosts stay
    before = _state(w)
    w.splice_parents()
    _assert_bit_equal(_state(w), before, "the all-empty edit")
    assert w.stats()["M"] == m > n and w.ridgeraft_pending() == 10
    # ... and the context still takes a good edit and finishes its step
    w.splice_parents((), ([50], ok), None)
    assert w.stats()["M"] == w.stats()["N"] == n and w.ridgeraft_pending() == 10
    w.finish_step(10, cfg["dt"], coupling_dt=1)
    assert w.ridgeraft_pending() == -1


def test_refused_on_a_tiled_context():
    import test_splice_gpu as tsg
    from subzero_jl_amd import tiles
    from subzero_jl_amd.capi import SzError
    cfg = tsg._cfg("periodic")
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=20)
    before = tsg._full(tw.world)
    with pytest.raises(SzError) as e:
        tw.world.splice_parents([0], None, None)
    assert str(e.value).startswith("libsubzero_hip error -4: ") and "tiled" in str(e.value)
    tsg._assert_bit_equal(tsg._full(tw.world), before)

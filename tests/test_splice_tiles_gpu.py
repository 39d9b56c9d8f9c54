"""Rows down, rows back on tiled contexts, by global number (csrc/sz_splice_tile.hpp): TiledWorld.download_rows and
TiledWorld.splice_global against the SINGLE context -- World.download_rows and World.splice of the same edit on the undivided list, themselves
held to a fresh upload by tests/test_splice_gpu.py.  Ranks are spawned processes that share the one GPU and trade through gloo (backend
"library-host"), as in tests/test_tiles_gpu.py; at most 4 of them.  Every comparison is on bits: each rank's owned columns, rings, sub-floe
points, ids and statuses against the single context's rows named by the rank's new gidx, and that gidx against tests/splice_tiles_ref.py.  The
steps that follow an edit show a stale key, box or cache.  The rank processes build their edits from download_rows of the whole list."""
import datetime
import os

import numpy as np
import pytest

import remove_tiles_ref as rt
import splice_ref as sp
import splice_tiles_ref as st
from test_remove_gpu import _cols
from test_remove_tiles_gpu import _rank_cols
from test_splice_gpu import SHAPES, _assert_bit_equal, _cfg, _changed, _edit, _full, _hand_ring, _pieces, _removal, _settled, mk
from test_tiles_gpu import _collect, _free_port, _guard

pytestmark = pytest.mark.gpu

E_ARG, E_CAPACITY, E_STATE = -2, -3, -4
RUN = dict(coupling_dt=1)
EDITS = [s for s in SHAPES if s != "del_all_but_one"] + ["cross_fuse"]


# ---------------------------------------------------------------- fields and edits
def _owners(cfg, world):
    from subzero_jl_amd import tiles
    return tiles.assign_tiles(cfg["derived"]["cx"], cfg["derived"]["cy"], cfg["L"], world)


def _cross_pair(cfg, world=2):
    """(a, b): the first two floes, in list order, that different ranks own, a < b -- for 2 and for 4 ranks alike where possible"""
    o2, o4 = _owners(cfg, 2), _owners(cfg, 4)
    for a in range(20, 60):
        for b in range(a + 1, a + 40):
            if o2[a] != o2[b] and o4[a] != o4[b]:
                return a, b
    raise AssertionError("no such pair")


def _the_edit(name, full, cfg):
    if name == "cross_fuse":          # the replacement on one rank, the deletion on another
        a, b = _cross_pair(cfg)
        return [b], ([a], _changed(full, [a], ["resampled"], cfg["dg"], int(full["id"].max()) + 1)), None
    return _edit(name, full, cfg)


def _app_owner(edit, cfg, world):
    """TiledWorld.splice_global's default: the tile that holds the appended centroid"""
    from subzero_jl_amd import tiles
    app = edit[2]
    if app is None:
        return None
    return tiles.assign_tiles(app["cx"] % cfg["L"], app["cy"] % cfg["L"], cfg["L"], world)


def _cells_cfg(cells, room):
    """test_splice_gpu._hand_cfg with the floes in the lattice cells `cells` (so that both halves of the domain hold some)"""
    from subzero_jl_amd import fields, floe as floe_mod
    spacing, side = 2.0e4, 8.0e3
    n = len(cells)
    n_side = max(2, int(np.ceil(np.sqrt(room))))
    L = n_side * spacing
    rings = [_hand_ring(k, n_side, spacing, side) for k in cells]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    rng = np.random.Generator(np.random.PCG64(5))
    Nx = Ny = 4 * n_side
    z = np.zeros((Nx + 1, Ny + 1))
    cfg = dict(n_floes=n, L=L, kinds=["periodic"] * 4, vert_off=off, vx=vx, vy=vy, height=np.full(n, 0.25), u=rng.uniform(-0.1, 0.1, n),
               v=rng.uniform(-0.1, 0.1, n), xi=rng.uniform(-1e-6, 1e-6, n), dt=20, Nx=Nx, Ny=Ny, uo=z + 0.1, vo=z, hf=z, ua=z, va=z, topography=[],
               dg=side / 2.0, E=6e6, n_side=n_side, spacing=spacing, side=side)
    d = cfg["derived"] = floe_mod.derive(off, vx, vy, cfg["height"])
    so = [0]; sxs = []; sys_ = []
    for i, r in enumerate(rings):
        sx, sy = fields.subgrid_points(r, d["cx"][i], d["cy"][i], cfg["dg"])
        so.append(so[-1] + len(sx)); sxs.append(sx); sys_.append(sy)
    cfg["sub_off"] = np.array(so, np.int32); cfg["sx"] = np.concatenate(sxs); cfg["sy"] = np.concatenate(sys_)
    return cfg


def _grow_cfg():
    """12 floes, six in either half of a lattice of 47 x 47 cells"""
    return _cells_cfg([0, 1, 2, 3, 4, 5, 40, 41, 42, 43, 44, 45], 2200)


def _grow_append(full, cfg):
    """600 triangles in free cells of the WEST half (rank 0's of two): rank 0 outgrows what it was carved for, rank 1 keeps its rows"""
    ns = cfg["n_side"]
    cells = [k for k in range(ns, ns * ns) if k % ns < ns // 2 - 1][:600]
    new = [_hand_ring(k, ns, cfg["spacing"], cfg["side"], triangle=True) for k in cells]
    return sp.floes_from(new, sp.take(full, [k % 12 for k in range(600)]), np.arange(100, 700), cfg["dg"])


def _long_ring_append(full, cfg):
    """floe 10 out, and in its place a ring of 41 points whose rmax is the largest of the field"""
    r = 1.0001 * float(full["rmax"].max())
    th = np.linspace(0.0, -2.0 * np.pi, 41)
    ring = np.stack([full["cx"][10] + r * np.cos(th), full["cy"][10] + r * np.sin(th)], 1); ring[-1] = ring[0]
    return [10], None, sp.floes_from([ring], sp.take(full, [10]), [int(full["id"].max()) + 1], cfg["dg"])


def _pool_edits(full, cfg, stage):
    """test_splice_gpu.py::test_growth_of_the_point_pool_alone's two edits"""
    if stage == 0:
        return [10], None, _pieces(full, [10], cfg["dg"], 5000, cut=lambda r: [sp.scaled(r, 0.3)])
    app = _pieces(full, [20], cfg["dg"], 5001, cut=lambda r: [sp.resampled(r)])
    return (), ([20], sp.floes_from([sp.ring_of(app, 0)], sp.take(full, [20]), [5001], cfg["dg"] / 3.0)), None


# ---------------------------------------------------------------- ranks
def _tiled(cfg, rank, world, dist, ftype=np.float64):
    from subzero_jl_amd import tiles
    return tiles.TiledWorld(cfg, rank, world, 0, dist, host_staging=True, backend="library-host", rebox_every=3, drift_margin=3000.0, ftype=ftype)


def _settled_tile(name, rank, world, dist, steps=20, setup=None, ftype=np.float64):
    cfg = _cfg(name) if isinstance(name, str) else name
    tw = _tiled(cfg, rank, world, dist, ftype)
    if setup:
        setup(tw)
    if steps:
        assert tw.run(steps, 0, cfg["dt"], **RUN) == steps
    return tw, cfg


def _snap(tw):
    return dict(gidx=np.array(tw.gidx), cols=_rank_cols(tw))


def _same(a, b):
    if sorted(a) != sorted(b):
        return False
    return all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def _own_inter(tw, which, got):
    """the interaction rows of the floes this rank found against its own full download"""
    io, ir = tw.world.interactions()
    ir = np.asarray(ir).reshape(-1, 7)
    loc = {int(g): i for i, g in enumerate(tw.gidx)}
    return all(np.array_equal(sp.inter_of(got, k).view(np.uint8), np.ascontiguousarray(ir[io[loc[g]]:io[loc[g] + 1]]).view(np.uint8)) for k, g in enumerate(which))


def _inter_by_name(tw):
    """this rank's full download of the interaction rows, per owned global number"""
    io, ir = tw.world.interactions()
    ir = np.asarray(ir, np.float64).reshape(-1, 7)
    return {int(g): np.array(ir[io[i]:io[i + 1]]) for i, g in enumerate(tw.gidx)}


def _inter_as_promised(tw, old_gidx, before, edit, owner, rank, n_global):
    """the interaction rows behind an edit: a kept floe's are what this rank's download reported before it (partner numbers as they stood), a
    staged floe's are the uploaded ones; the rows a rank holds behind its share are splice_tiles_ref's"""
    s = st.share(old_gidx, edit, owner, rank, n_global)
    staged = st.staged_floes(edit)
    rep = {int(r): int(j) for r, j in zip(s["rep_rows"], s["staged"])}          # (the replacements this rank takes come first among its staged floes, by row)
    want = [sp.inter_of(staged, rep[r]) if r in rep else before[int(old_gidx[r])] for r in range(len(old_gidx)) if r not in set(map(int, s["del_rows"]))]
    want += [sp.inter_of(staged, int(j)) for j in s["staged"][len(s["rep_rows"]):]]
    after = _inter_by_name(tw)
    got = [after[int(g)] for g in tw.gidx]
    bits = lambda a: np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 7)).view(np.uint8)
    return len(got) == len(want) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))


def _s_rows_down(rank, world, dist):
    tw, cfg = _settled_tile("periodic", rank, world, dist)
    n = cfg["n_floes"]
    rng = np.random.Generator(np.random.PCG64(2))
    sels = {"empty": [], "one": [n // 3], "all_reversed": list(range(n))[::-1], "random_37": list(rng.permutation(n)[:37]),
            "one_rank": list(np.nonzero(_owners(cfg, world) == 0)[0][::-1][:50])}
    before = _snap(tw)
    out = dict(gidx=np.array(tw.gidx), inter_ok={}, rows={}, n_inter=0)
    for name, sel in sels.items():
        which, mine = tw.download_rows_local(sel)
        assert all(int(sel[k]) in set(tw.gidx) for k in which) and len(which) == len(set(map(int, sel)) & set(map(int, tw.gidx)))
        out["inter_ok"][name] = bool(_own_inter(tw, [int(sel[k]) for k in which], mine))
        out["n_inter"] += int(mine["inter_off"][-1])
        got = tw.download_rows(sel)
        if rank == 0:
            out["rows"][name] = (sel, got)
    out["unchanged"] = _same(before["cols"], _snap(tw)["cols"])
    return out


def _s_edits(rank, world, dist, names):
    out = {}
    for name in names:
        tw, cfg = _settled_tile("periodic", rank, world, dist)
        full = tw.download_rows(np.arange(cfg["n_floes"]))
        edit = _the_edit(name, full, cfg)
        old_gidx, inter0 = np.array(tw.gidx), _inter_by_name(tw)
        ng, no = tw.splice_global(*edit)
        o = dict(counts=(ng, no), after=_snap(tw), hints=(tw._max_ring, tw._max_rmax))
        o["inter_ok"] = bool(_inter_as_promised(tw, old_gidx, inter0, edit, _app_owner(edit, cfg, world), rank, cfg["n_floes"]))
        o["n_inter"] = int(sum(len(v) for v in inter0.values()))
        assert tw.run(20, 20, cfg["dt"], **RUN) == 20
        o["later"] = _snap(tw)
        out[name] = o
    return out


def _s_one(rank, world, dist, what):
    """one scenario of the edges: (field, steps before, edits one after the other, what follows, steps after)"""
    f32 = what == "f32"
    field = _grow_cfg() if what == "grow" else "periodic"
    tw, cfg = _settled_tile(field, rank, world, dist, steps=3 if what == "grow" else 20, ftype=np.float32 if f32 else np.float64,
                            setup=(lambda t: t.set_removal(True, max_vertices=2**31 - 1, min_floe_area=1e6, min_floe_height=0.1)) if what == "remove" else None)
    out = dict(hints0=(tw._max_ring, tw._max_rmax))
    n = cfg["n_floes"]
    full = tw.download_rows(np.arange(n))
    if what == "grow":
        tw.splice_global((), None, _grow_append(full, cfg))
    elif what == "long_ring":
        tw.splice_global(*_long_ring_append(full, cfg))
    elif what == "pool":
        tw.splice_global(*_pool_edits(full, cfg, 0))
        out["first"] = _snap(tw)
        full = tw.download_rows(np.arange(n))
        tw.splice_global(*_pool_edits(full, cfg, 1))
    elif what in ("migrate", "f32"):
        tw.splice_global(*_edit("fracture", full, cfg))
    elif what == "remove":
        from subzero_jl_amd import capi
        e1 = _edit("fracture", full, cfg)
        tw.splice_global(*e1)
        one = tw.download_rows(np.arange(n - 3 + 9))
        rep = _changed(one, [12], ["scaled"], cfg["dg"], 9000)
        rep["status"][:] = capi.REMOVE
        tw.splice_global([3], ([12], rep), None)
    out["after"] = _snap(tw); out["hints"] = (tw._max_ring, tw._max_rmax)
    if what == "migrate":
        L = cfg["L"]
        out["moved"] = tw.migrate(owner_fn=lambda cx, cy: (cy > 0.5 * L).astype(int))
        out["migrated"] = _snap(tw)
    if what == "remove":
        out["verdict"] = tw.remove_floes()
        out["removed"] = _snap(tw)
    steps = {"grow": 10, "long_ring": 20, "pool": 10, "migrate": 10, "remove": 0, "f32": 0}[what]
    if steps:
        assert tw.run(steps, 3 if what == "grow" else 20, cfg["dt"], **RUN) == steps
        out["later"] = _snap(tw)
    return out


def _code(fn):
    from subzero_jl_amd.capi import SzError
    try:
        fn()
    except SzError as e:
        msg = str(e)
        assert msg.startswith("libsubzero_hip error ") and len(msg) > 40, msg
        return int(msg.split()[2].rstrip(":")), msg
    return 0, ""


def _s_refusals(rank, world, dist):
    from subzero_jl_amd import capi
    tw, cfg = _settled_tile("periodic", rank, world, dist)
    n = cfg["n_floes"]
    full = tw.download_rows(np.arange(n))
    ok = _changed(full, [50], ["scaled"], cfg["dg"], 7000)
    two = _changed(full, [50, 60], ["scaled", "scaled"], cfg["dg"], 7000)
    opened = {k: v.copy() for k, v in ok.items()}; opened["vx"][-1] += 1.0
    th = np.linspace(0.0, -2.0 * np.pi, 300)
    ring = np.stack([full["cx"][50] + 5e3 * np.cos(th), full["cy"][50] + 5e3 * np.sin(th)], 1); ring[-1] = ring[0]
    long_ = sp.floes_from([ring], sp.take(full, [50]), [7000], cfg["dg"])
    many = {k: v.copy() for k, v in ok.items()}
    many["inter_off"] = np.array([0, 600], np.int32); many["inter_rows"] = np.ones((600, 7))
    mine = [int(g) for g in tw.gidx]
    others0 = [g for g in range(n) if _owners(cfg, world)[g] != 0]
    cases = {
        "unsorted": (([5, 3], None, None), E_ARG, "ascending"), "repeated": (([5, 5], None, None), E_ARG, "repeats"), "negative": (([-1], None, None), E_ARG, "start at 0"),
        "rep_unsorted": (((), ([60, 50], two), None), E_ARG, "ascending"), "both": (([50], ([50], ok), None), E_ARG, "both deleted and replaced"),
        "out_of_range": (([n], None, None), E_ARG, "outside"), "rep_out_of_range": (((), ([n + 7], ok), None), E_ARG, "outside"),
        "owner": (((), None, ok, [world]), E_ARG, "app_owner"), "owner_negative": (((), None, ok, [-1]), E_ARG, "app_owner"),
        "open": (((), ([50], opened), None), E_ARG, "open ring"), "long": (((), None, long_, [0]), E_ARG, "255"),
        "no_floe": ((list(range(n)), None, None), E_ARG, "no floe"), "del_all_but_one": (_edit("del_all_but_one", full, cfg), E_ARG, "no floe on rank"),
        "rank_emptied": ((others0, None, None), E_ARG, "no floe on rank"), "rows": (((), ([50], many), None), E_CAPACITY, "interaction rows"),
    }
    before = _snap(tw)
    out = dict(codes={}, same={})
    for name, (edit, code, needle) in cases.items():
        got, msg = _code(lambda: tw.splice_global(*edit))
        out["codes"][name] = (got, code, needle in msg, msg)
        out["same"][name] = _same(before["cols"], _snap(tw)["cols"]) and np.array_equal(before["gidx"], tw.gidx)
    # ghosts in the list of ONE rank: every rank returns the same code
    if rank == world - 1:
        tw.world.add_ghosts()
    got, msg = _code(lambda: tw.splice_global([5], None, None))
    out["codes"]["ghosts"] = (got, E_STATE, "ghosts" in msg, msg)
    got2, msg2 = _code(lambda: tw.download_rows_local([5])) if rank == world - 1 else (E_STATE, "ghosts")
    out["codes"]["ghosts_down"] = (got2, E_STATE, "ghosts" in msg2, msg2)
    if rank == world - 1:
        tw.world.remove_ghosts()
    out["same"]["ghosts"] = _same(before["cols"], _snap(tw)["cols"])
    # bad names of a download
    for name, sel, needle in (("down_negative", [3, -2], "start at 0"), ("down_repeated", [3, 9, 3], "repeats")):
        got, msg = _code(lambda: tw.download_rows_local(sel))
        out["codes"][name] = (got, E_ARG, needle in msg, msg)
    which, none = tw.download_rows_local([n + 5, n + 6])
    out["nowhere"] = (len(which), sp.n_rows(none))
    # the all-empty edit issues no collective: only rank 0 calls
    if rank == 0:
        out["empty_edit"] = tw.splice_global((), None, None)
    out["same"]["end"] = _same(before["cols"], _snap(tw)["cols"])
    # and the context still takes a good edit
    tw.splice_global((), ([50], ok), None)
    out["good"] = _snap(tw)
    return out


def _s_pending(rank, world, dist):
    from test_ridgeraft_gpu import _dense
    cfg = _dense()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_ridgeraft(True, dt=10)
    out = dict(ran=tw.run(40, 1, cfg["dt"], coupling_dt=1, stop_on_tags=True), pending=tw.ridgeraft_pending())
    io0, ir0 = tw.world.interactions()
    st0 = tw.world.stats()
    out["splice"] = _code(lambda: tw.splice_global([5], None, None))
    out["down"] = _code(lambda: tw.download_rows_local([5]))
    io1, ir1 = tw.world.interactions()
    out["same"] = tw.ridgeraft_pending() == out["pending"] and tw.world.stats() == st0 and np.array_equal(io0, io1) and np.array_equal(np.asarray(ir0).view(np.uint8), np.asarray(ir1).view(np.uint8))
    tw.finish_step(out["pending"], cfg["dt"], coupling_dt=1)
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_rows_down, _s_edits, _s_one, _s_refusals, _s_pending)}


def _worker(rank, world, port, scenario, args, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        q.put((rank, SCENARIOS[scenario](rank, world, dist, *args)))
    finally:
        dist.destroy_process_group()


def _run_worker(*a):
    _guard(_worker)(*a)


def _ranks(scenario, world, *args):
    """the scenario on `world` spawned ranks: their results by rank"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_run_worker, args=(r, world, port, scenario, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = _collect(q, world)
        for p in procs:
            p.join(60)
        assert all(p.exitcode == 0 for p in procs)
    finally:
        for p in procs:          # a rank left waiting in a collective by a failed peer
            if p.is_alive():
                p.terminate()
    return [out for _, out in sorted(res, key=lambda r: r[0])]


# ---------------------------------------------------------------- the yardstick
def _assert_ranks_equal_single(snaps, single, where):
    """every rank's floes are the single context's rows its gidx names, all of them exactly once; single: the World, or its _cols"""
    ref = single if isinstance(single, dict) else _cols(single)
    seen = np.concatenate([s["gidx"] for s in snaps])
    assert sorted(seen) == list(range(len(ref["cx"]))), (where, len(seen), len(ref["cx"]))
    for r, s in enumerate(snaps):
        assert np.all(np.diff(s["gidx"]) > 0), (where, r)
        _assert_bit_equal(s["cols"], rt.take_rows(ref, s["gidx"]), f"{where}, rank {r}")


def _ref_gidx(cfg_or_owner, world, edits, n0, apps_owner=None):
    """splice_tiles_ref: the ranks' numbers behind the edits, from the owners at the start"""
    own = np.asarray(cfg_or_owner)
    gidx = [np.nonzero(own == r)[0] for r in range(world)]
    n = n0
    for edit, ao in edits:
        assert st.verdict(gidx, edit, ao) is None
        gidx = [st.share(g, edit, ao, r, n)["gidx"] for r, g in enumerate(gidx)]
        n = n - len(edit[0]) + st.n_staged(edit)[1]
    return gidx


@pytest.fixture(scope="module")
def single20():
    D, cfg = _settled("periodic")
    return D, _full(D), cfg


# ---------------------------------------------------------------- 1. rows down
@pytest.fixture(scope="module", params=[2, 4])
def rows_down(request):
    return request.param, _ranks("rows_down", request.param)


@pytest.mark.parametrize("sel", ["empty", "one", "all_reversed", "random_37", "one_rank"])
def test_download_rows_equals_the_single_contexts(rows_down, single20, sel):
    world, res = rows_down
    D, full, cfg = single20
    names, got = res[0]["rows"][sel]
    want = D.download_rows(names)
    drop = ("inter_off", "inter_rows")          # (partner numbers are a tiled context's: compared against the rank's own full download)
    _assert_bit_equal({k: v for k, v in got.items() if k not in drop}, {k: v for k, v in want.items() if k not in drop}, (world, sel))
    assert np.array_equal(got["inter_off"], want["inter_off"]), "the same number of interaction rows per floe"
    assert all(r["inter_ok"][sel] for r in res) and all(r["unchanged"] for r in res)
    assert sum(r["n_inter"] for r in res) > 0, "the ranks compared interaction rows that exist"
    if sel not in ("empty", "one"):          # (no floe, or one that may be at rest)
        assert np.count_nonzero(got["stress_accum"]) > 0
    if sel == "one_rank":
        assert set(names) <= set(res[0]["gidx"])


# ---------------------------------------------------------------- 2. every edit shape
@pytest.fixture(scope="module", params=[2, 4])
def edits(request):
    return request.param, _ranks("edits", request.param, EDITS)


SINGLE = {}


def _single_edit(shape):
    """the single context's side of an edit, once for both rank counts: (edit, columns behind it, columns 20 steps on)"""
    if shape not in SINGLE:
        D, cfg = _settled("periodic")
        edit = _the_edit(shape, _full(D), cfg)
        D.splice(*edit)
        after = _cols(D)
        assert D.run(20, 20, cfg["dt"], stop_on_tags=False, **RUN) == 20
        SINGLE[shape] = (edit, after, _cols(D))
    return SINGLE[shape]


@pytest.mark.parametrize("shape", EDITS)
def test_splice_global_equals_splice_of_the_undivided_list(edits, shape):
    world, res = edits
    cfg = _cfg("periodic")
    edit, after, later = _single_edit(shape)
    ao = _app_owner(edit, cfg, world)
    want = _ref_gidx(_owners(cfg, world), world, [(edit, ao)], cfg["n_floes"])
    for r in range(world):
        assert np.array_equal(res[r][shape]["after"]["gidx"], want[r]), (shape, r)
    if shape != "noop":
        assert all(res[r][shape]["counts"] == (len(after["cx"]), len(want[r])) for r in range(world))
    if shape == "cross_fuse":
        a, b = _cross_pair(cfg)
        o = _owners(cfg, world)
        assert o[a] != o[b], "the replacement on one rank, the deletion on another"
    _assert_ranks_equal_single([res[r][shape]["after"] for r in range(world)], after, (world, shape))
    assert all(res[r][shape]["inter_ok"] for r in range(world)), "interaction rows: kept floes as the rank reported them before, staged floes as uploaded"
    assert sum(res[r][shape]["n_inter"] for r in range(world)) > 0, "the field has interaction rows to keep"
    _assert_ranks_equal_single([res[r][shape]["later"] for r in range(world)], later, (world, shape, "20 steps on"))


# ---------------------------------------------------------------- 3. one rank
@pytest.mark.parametrize("shape", ["fracture", "everything"])
def test_one_rank_as_a_tiled_context_equals_world_splice(shape):
    from subzero_jl_amd import tiles
    cfg = _cfg("periodic")
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    assert tw.run(20, 0, cfg["dt"], **RUN) == 20
    D, _ = _settled("periodic")
    full = _full(D)
    n = cfg["n_floes"]
    got = tw.download_rows(np.arange(n)[::-1])
    drop = ("inter_off", "inter_rows")
    _assert_bit_equal({k: v for k, v in got.items() if k not in drop}, {k: v for k, v in D.download_rows(np.arange(n)[::-1]).items() if k not in drop})
    edit = _edit(shape, full, cfg)
    assert tw.splice_global(*_edit(shape, tw.download_rows(np.arange(n)), cfg)) == (n - len(edit[0]) + sp.n_rows(edit[2]), n - len(edit[0]) + sp.n_rows(edit[2]))
    D.splice(*edit)
    assert np.array_equal(tw.gidx, np.arange(D.N))
    _assert_ranks_equal_single([_snap(tw)], D, shape)
    for w in (tw, D):
        assert w.run(20, 20, cfg["dt"], **({"stop_on_tags": False} if w is D else {}), **RUN) == 20
    _assert_ranks_equal_single([_snap(tw)], D, shape + ", 20 steps on")


def test_a_request_longer_than_one_round_of_the_scan():
    """The length of a request is the caller's, not one of the context's capacities: sz_tile_download_rows searches and compacts the names 2^20 at
    a time.  2^20 + 5000 names, 400 of them floes -- at the first and last position of either round and at random ones between -- bring the rows
    that the 400 names alone bring, at those positions."""
    from subzero_jl_amd import tiles
    cfg = _cfg("periodic")
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    assert tw.run(20, 0, cfg["dt"], **RUN) == 20
    n, one = cfg["n_floes"], 1 << 20
    big = one + 5000
    assert n == 400
    rng = np.random.Generator(np.random.PCG64(3))
    pos = np.sort(np.concatenate([[0, one - 1, one, big - 1], 1 + rng.choice(one - 2, 198, replace=False), one + 1 + rng.choice(4998, 198, replace=False)]))
    assert len(np.unique(pos)) == n
    floes = rng.permutation(n)
    names = np.arange(n, n + big, dtype=np.int64)          # (no rank owns these)
    names[pos] = floes
    which, got = tw.download_rows_local(names)
    assert np.array_equal(which, pos)
    which1, want = tw.download_rows_local(floes)
    assert np.array_equal(which1, np.arange(n))
    _assert_bit_equal(got, want, "two rounds")


# ---------------------------------------------------------------- 4. edges
def test_an_appended_long_ring_with_the_largest_rmax_raises_the_hints(single20):
    D0, full, cfg = single20
    res = _ranks("one", 2, "long_ring")
    D, _ = _settled("periodic")
    edit = _long_ring_append(_full(D), cfg)
    D.splice(*edit)
    for r in res:
        assert r["hints0"][0] < 41 <= r["hints"][0] and r["hints"][1] == float(edit[2]["rmax"][0]) > r["hints0"][1]
    _assert_ranks_equal_single([r["after"] for r in res], D, "long ring")
    assert D.run(20, 20, cfg["dt"], stop_on_tags=False, **RUN) == 20
    _assert_ranks_equal_single([r["later"] for r in res], D, "long ring, 20 steps on")


def test_one_rank_outgrows_its_capacities_and_the_other_does_not():
    """12 floes, 600 appended to rank 0: its 6 + 600 rows are beyond an eighth more than it was carved for, rank 1's 6 are not"""
    from subzero_jl_amd import fields
    res = _ranks("one", 2, "grow")
    cfg = _grow_cfg()
    assert list(np.bincount(_owners(cfg, 2))) == [6, 6]
    D = fields.build_world(mk(), cfg)
    assert D.run(3, 0, cfg["dt"], stop_on_tags=False, **RUN) == 3
    app = _grow_append(_full(D), cfg)
    assert set(_app_owner(((), None, app), cfg, 2)) == {0}
    D.splice((), None, app)
    assert D.N == 612 and [len(r["after"]["gidx"]) for r in res] == [606, 6]
    _assert_ranks_equal_single([r["after"] for r in res], D, "grown")
    assert D.run(10, 3, cfg["dt"], stop_on_tags=False, **RUN) == 10
    _assert_ranks_equal_single([r["later"] for r in res], D, "grown, 10 steps on")


def test_growth_of_the_point_pool_alone():
    res = _ranks("one", 2, "pool")
    D, cfg = _settled("periodic")
    D.splice(*_pool_edits(_full(D), cfg, 0))
    _assert_ranks_equal_single([r["first"] for r in res], D, "first")
    pool = D.stats()["n_sub_points"]
    D.splice(*_pool_edits(_full(D), cfg, 1))
    assert D.stats()["n_sub_points"] > pool
    _assert_ranks_equal_single([r["after"] for r in res], D, "pool")
    assert D.run(10, 20, cfg["dt"], stop_on_tags=False, **RUN) == 10
    _assert_ranks_equal_single([r["later"] for r in res], D, "pool, 10 steps on")


def test_migrate_behind_a_splice():
    res = _ranks("one", 2, "migrate")
    D, cfg = _settled("periodic")
    D.splice(*_edit("fracture", _full(D), cfg))
    _assert_ranks_equal_single([r["after"] for r in res], D, "spliced")
    assert sum(r["moved"] for r in res) > 50
    _assert_ranks_equal_single([r["migrated"] for r in res], D, "migrated")
    assert D.run(10, 20, cfg["dt"], stop_on_tags=False, **RUN) == 10
    _assert_ranks_equal_single([r["later"] for r in res], D, "migrated, 10 steps on")


def test_remove_floes_behind_two_splices_the_numbers_compose():
    from subzero_jl_amd import capi
    res = _ranks("one", 2, "remove")
    D, cfg = _settled("periodic", _removal)
    full = _full(D)
    e1 = _edit("fracture", full, cfg)
    D.splice(*e1)
    one = _full(D)
    rep = _changed(one, [12], ["scaled"], cfg["dg"], 9000)
    rep["status"][:] = capi.REMOVE
    e2 = ([3], ([12], rep), None)
    D.splice(*e2)
    want = _ref_gidx(_owners(cfg, 2), 2, [(e1, _app_owner(e1, cfg, 2)), (e2, None)], cfg["n_floes"])
    for r in range(2):
        assert np.array_equal(res[r]["after"]["gidx"], want[r])
    _assert_ranks_equal_single([r["after"] for r in res], D, "twice")
    assert D.remove_floes() == (True, 1, 0) and all(r["verdict"] == (True, 1, 0) for r in res)
    gone = 11          # (row 12 of the list before the deletion of row 3)
    for r in range(2):
        assert np.array_equal(res[r]["removed"]["gidx"], np.array([g - (g > gone) for g in want[r] if g != gone]))
    _assert_ranks_equal_single([r["removed"] for r in res], D, "twice, then the pass")


def test_f32_twins_fracture_edit():
    res = _ranks("one", 2, "f32")
    D, cfg = _settled("periodic", ftype=np.float32)
    D.splice(*_edit("fracture", _full(D), cfg))
    _assert_ranks_equal_single([r["after"] for r in res], D, "f32")


# ---------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("world", [2])
def test_refusals_leave_every_rank_as_it_was_with_the_same_code(world):
    res = _ranks("refusals", world)
    for name in res[0]["codes"]:
        got = [r["codes"][name] for r in res]
        assert all(g[0] == g[1] and g[2] for g in got), (name, got)
    for r in res:
        assert all(r["same"].values()), r["same"]
        assert r["nowhere"] == (0, 0)
    assert res[0]["empty_edit"] == (None, len(res[0]["good"]["gidx"]))
    D, cfg = _settled("periodic")
    full = _full(D)
    D.splice((), ([50], _changed(full, [50], ["scaled"], cfg["dg"], 7000)), None)
    _assert_ranks_equal_single([r["good"] for r in res], D, "a good edit behind the refusals")


def test_refused_at_a_pending_ridge_raft_stop():
    res = _ranks("pending", 2)
    for r in res:
        assert r["pending"] >= 0, "the dense field did not stop at a ridge / raft step"
        assert r["splice"][0] == E_STATE and "sz_tile_step_finish" in r["splice"][1]
        assert r["down"][0] == E_STATE and "sz_tile_step_finish" in r["down"][1]
        assert r["same"]


def test_refused_without_tiling_setup_or_ascending_numbers():
    """in this process: a single context, a context that is tiled but has no set-up and no communicator (the torch-exchange backend), and one
    rank whose numbers sz_tile_enable was given in descending order"""
    import ctypes as C
    from subzero_jl_amd import capi, fields, tiles
    cfg = _cfg("periodic")
    one = np.array([0], np.int64); nm = C.c_int32(0); which = np.zeros(1, np.int32)

    def calls(w):
        down = w.L.sz_tile_download_rows(w.h, 1, capi.ptr(one, capi._lp), C.byref(nm), capi.ptr(which, capi._ip), None, None, None, None)
        msg_down = w.L.sz_last_error(w.h).decode()
        up = w.L.sz_tile_splice_floes(w.h, 1, capi.ptr(one, capi._lp), 0, None, 0, None, None, None, None, None, None)
        return down, msg_down, up, w.L.sz_last_error(w.h).decode()
    D = fields.build_world(mk(), cfg)
    D._push()
    before = _full(D)
    down, msg_down, up, msg_up = calls(D)
    assert down == E_STATE and "sz_tile_enable" in msg_down and up == E_STATE and "sz_tile_enable" in msg_up
    _assert_bit_equal(_full(D), before, "a single context")
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="torch")
    before = _full(tw.world)
    down, msg_down, up, msg_up = calls(tw.world)
    assert down == 0 and nm.value == 1, "the download is local: it needs no set-up"
    assert up == E_STATE and "sz_tile_setup" in msg_up
    with pytest.raises(capi.SzError):
        tw.splice_global([0], None, None)
    _assert_bit_equal(_full(tw.world), before, "tiled, no set-up")
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    w = tw.world
    g = np.ascontiguousarray(tw.gidx[::-1], np.int64)
    w._chk(w.L.sz_tile_enable(w.h, capi.ptr(g, capi._lp), tw._max_ring, tw._max_rmax))
    before = _full(w)
    down, msg_down, up, msg_up = calls(w)
    assert down == E_STATE and "ascending" in msg_down and up == E_STATE and "ascending" in msg_up
    _assert_bit_equal(_full(w), before, "numbers not ascending")

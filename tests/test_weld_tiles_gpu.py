"""Welding overlaps on tiled contexts (csrc/sz_weld_tile.hpp; sz_tile_weld_overlaps, sz_tile_run with welding set): ranks are spawned processes
that share the one GPU and trade through gloo (backend "library-host"), as in tests/test_remove_tiles_gpu.py.  The yardstick is the single
context -- World.set_welding, World.weld_overlaps and World.run, held to the reference by tests/test_weld_gpu.py -- and every comparison is bit
for bit: both sides run the same clipper on the same ring bits, so there is no tolerance and no tie exclusion."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

import remove_tiles_ref as rt
import weld_ref as wr
from test_remove_gpu import _assert_bit_equal, _cols, mk
from test_fracture_tiles_gpu import _retile
from test_remove_tiles_gpu import _rank_cols, _tiled
from test_tiles_gpu import _collect, _free_port, _guard, _tag_cfg
from test_weld_gpu import FIELDS, _tip_and_wall

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
SHAPES = ((1, 1), (3, 2), (7, 5))
PARITY = dict(FIELDS, voronoi500=dict(n_floes=500, seed=7, subgrid_per_floe=4.0, shape="voronoi"))
BOX_L, BOX_DT = 1.2e5, 20
NEVER_STEPS = 24
TAG_STEPS = 12


# ---------------------------------------------------------------- fields
def _rings_cfg(rings, L, kinds, ngrid, u=None, dt=10, E=6e6, height=0.5):
    """a hand-made field as a config (fields.build_world and TiledWorld both take it)"""
    from subzero_jl_amd import floe as floe_mod
    n = len(rings)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(r) for r in rings])
    vx = np.concatenate([np.asarray(r, float)[:, 0] for r in rings]); vy = np.concatenate([np.asarray(r, float)[:, 1] for r in rings])
    h = np.full(n, float(height))
    z = np.zeros((ngrid + 1, ngrid + 1))
    return dict(n_floes=n, L=L, kinds=list(kinds), vert_off=off, vx=vx, vy=vy, height=h, u=np.zeros(n) if u is None else np.array(u, float), v=np.zeros(n),
                xi=np.zeros(n), dt=dt, Nx=ngrid, Ny=ngrid, uo=z, vo=z, hf=z, ua=z, va=z, topography=[], E=E, derived=floe_mod.derive(off, vx, vy, h),
                sub_off=np.zeros(n + 1, np.int32), sx=np.zeros(0), sy=np.zeros(0), seed=0)


def _box_cfg(pair, u01=(0.0, 0.0)):
    """the box world of tests/test_weld_gpu.py (_box_world) as a config: `pair` first, then some thirty stars at rest far from one another"""
    rings = [pair[0], pair[1]]
    rng = np.random.default_rng(3)
    for gy in range(6):
        for gx in range(6):
            cx, cy = 1.5e4 + gx * 1.8e4, 1.5e4 + gy * 1.8e4
            if abs(cy - 6.1e4) < 1.2e4 and 3.0e4 < cx < 8.0e4:
                continue
            th = ((2 * np.pi / 7) * (np.arange(7) + rng.uniform(-0.3, 0.3, 7)))[::-1]
            r = 2500.0 * (0.7 + 0.3 * rng.uniform(0, 1, 7))
            ring = np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1)
            rings.append(np.concatenate([ring, ring[:1]]))
    u = np.zeros(len(rings)); u[0], u[1] = u01
    return _rings_cfg(rings, BOX_L, ["collision"] * 4, 12, u=u, dt=BOX_DT)


def _straddle_cfg(big):
    """the two overlapping quadrilaterals of test_a_step_with_two_sets_takes_the_first, centroids either side of x = L / 2; big: the eastern one
    is a 40-gon instead (more points than the small clip working set holds)"""
    a = np.array([[5.2e4, 5.0e4], [5.3e4, 5.9e4], [6.05e4, 5.8e4], [6.1e4, 5.1e4], [5.2e4, 5.0e4]])
    b = np.array([[5.95e4, 5.2e4], [6.0e4, 5.7e4], [6.8e4, 5.8e4], [6.9e4, 5.1e4], [5.95e4, 5.2e4]])
    if big:
        th = (2 * np.pi / 40) * np.arange(40)[::-1]          # clockwise
        r = 4.6e3 * (1.0 + 0.04 * np.cos(5 * th + 0.3))
        ring = np.stack([6.42e4 + r * np.cos(th), 5.45e4 + 0.8 * r * np.sin(th)], 1)
        b = np.concatenate([ring, ring[:1]])
    return _box_cfg((a, b))


def _closing_cfg():
    """the closing pair of _box_world (10 m per step across a 125 m gap), moved east so that its floes lie either side of x = L / 2"""
    return _box_cfg(_tip_and_wall(5.8e4, 6.1e4, 125.0), u01=(0.25, -0.25))


def _break_cfg():
    """the golden bin_floes rings with the out-of-bounds floe in the middle of the list, as test_bins_of_the_reference_floes has them"""
    g = wr.golden()
    rings = g["bin_floes"]["rings"]
    gr = g["grid"]
    assert gr["x0"] == 0.0 and gr["y0"] == 0.0 and gr["xf"] == gr["yf"]
    return _rings_cfg(rings[:3] + [rings[6]] + rings[3:6], gr["xf"], g["domains"]["open"], gr["nx"], height=g["bin_floes"]["height"])


def _tag_listed_cfg():
    """_tag_cfg("open") -- a floe of rank 1 drifts into the open east boundary, rank 0 knows nothing of it -- and a 24-gon at rest on rank 0: a ring
    over 20 points, so sz_tile_run takes its list-based driver with collisions on"""
    base = _tag_cfg("open")
    off = base["vert_off"]
    rings = [np.stack([base["vx"][off[i]:off[i + 1]], base["vy"][off[i]:off[i + 1]]], 1) for i in range(base["n_floes"])]
    th = (2 * np.pi / 24) * np.arange(24)[::-1]
    ring = np.stack([2.0e4 + 4e3 * np.cos(th), 8.0e4 + 4e3 * np.sin(th)], 1)
    rings.append(np.concatenate([ring, ring[:1]]))
    return _rings_cfg(rings, base["L"], base["kinds"], 10, u=list(base["u"]) + [0.0], dt=base["dt"], E=base["E"])


def _many_point_cfg():
    """500 stars of 22 .. 36 points each, by make_config's own recipe (jittered angles, radii of 0.6 .. 1 r0 about the centres of its star field, its
    velocities, ocean and sub-floe spacing): every ring is over the 20 points of the one-launch integrator, so sz_tile_run takes its list-based
    driver, and the rings that cross ranks fill the small and the large clip working set"""
    from subzero_jl_amd import fields
    from subzero_jl_amd import floe as floe_mod
    cfg = fields.make_config(n_floes=500, seed=7, subgrid_per_floe=4.0)
    n = cfg["n_floes"]
    d0 = cfg["derived"]
    r0 = 2.0e4 * np.sqrt(0.8 / (0.6533 * np.pi))          # (make_config's radius at its default spacing and concentration)
    rng = np.random.default_rng(29)
    nv = rng.integers(22, 37, n)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum(nv + 1)
    vx = np.zeros(off[-1]); vy = np.zeros(off[-1])
    for i in range(n):
        k = nv[i]
        th = ((2 * np.pi / k) * (np.arange(k) + rng.uniform(-0.35, 0.35, k) + rng.uniform(0, 1)))[::-1]          # descending: clockwise
        rad = r0 * (0.6 + 0.4 * rng.uniform(0, 1, k))
        x = d0["cx"][i] + rad * np.cos(th); y = d0["cy"][i] + rad * np.sin(th)
        o = off[i]
        vx[o:o + k] = x; vy[o:o + k] = y; vx[o + k] = x[0]; vy[o + k] = y[0]
    d = floe_mod.derive(off, vx, vy, cfg["height"])
    so = np.zeros(n + 1, np.int32); sxs = []; sys_ = []
    for i in range(n):
        ring = np.stack([vx[off[i]:off[i + 1]], vy[off[i]:off[i + 1]]], 1)
        sx, sy = fields.subgrid_points(ring, d["cx"][i], d["cy"][i], cfg["dg"])
        so[i + 1] = so[i] + len(sx); sxs.append(sx); sys_.append(sy)
    return dict(cfg, vert_off=off, vx=vx, vy=vy, derived=d, sub_off=so, sx=np.concatenate(sxs), sy=np.concatenate(sys_))


def _parity_cfg(name):
    from subzero_jl_amd import fields
    return _many_point_cfg() if name == "stars22to36" else fields.make_config(**PARITY[name])


def _star_cfg(seed=7):
    from subzero_jl_amd import fields
    return fields.make_config(**dict(FIELDS["star"], seed=seed))


def _single(cfg):
    from subzero_jl_amd import fields
    return fields.build_world(mk(), cfg)


def _bits(t):
    """a table as comparable python values: numbers, and the areas as bit patterns"""
    i, j, a = t
    return [int(x) for x in i], [int(x) for x in j], np.asarray(a, np.float64).view(np.uint64).tolist()


# ---------------------------------------------------------------- ranks
def _snap(tw):
    return dict(gidx=np.array(tw.gidx), cols=_rank_cols(tw))


def _s_straddle(rank, world, dist, big):
    from subzero_jl_amd import capi
    tw = _tiled(_straddle_cfg(big), rank, world, dist)
    out = dict(gidx=np.array(tw.gidx))
    for nx in (1, 2):
        out[nx] = _bits(tw.weld_overlaps(nx, 1, 2e9)); out[f"pairs{nx}"] = tw.weld_candidate_pairs()
    # a cap under the table: SZ_E_ARG on every rank, and the context goes on
    w = tw.world
    n = C.c_int32(0)
    i0 = np.zeros(1, np.int64); a0 = np.zeros(1)
    out["rc_cap"] = w.L.sz_tile_weld_overlaps(w.h, 1, 1, 2e9, C.byref(n), 0, capi.ptr(i0, capi._lp), capi.ptr(i0, capi._lp), capi.ptr(a0))
    out["n_cap"] = n.value
    out["after"] = _bits(tw.weld_overlaps(1, 1, 2e9))
    return out


def _s_break(rank, world, dist):
    from subzero_jl_amd import tiles
    cfg = _break_cfg()
    tw = _tiled(cfg, rank, world, dist)
    L = cfg["L"]
    # the out-of-bounds floe (the only centroid under y = 0) to rank 0; the floes behind it in the list stay rank 1's
    tw.migrate(owner_fn=lambda cx, cy: np.where(cy < 0.0, 0, tiles.assign_tiles(cx, cy, L, world)))
    return dict(gidx=np.array(tw.gidx), bins=tw.weld_bins(2, 2), table=_bits(tw.weld_overlaps(2, 2, 1e300)))


LISTED_RING_HINT = 24.0          # over the 20 points the one-launch integrator holds: sz_tile_run then takes its list-based driver


def _s_parity(rank, world, dist, name, mx_median):
    cfg = _parity_cfg(name)
    tw = _tiled(cfg, rank, world, dist)
    if name == "voronoi500":
        # the cells of this generator have at most 12 points, so the bound on the ring sizes of all ranks that sz_tile_enable takes is what
        # sends these steps down the list-based driver
        tw._max_ring = LISTED_RING_HINT
        _retile(tw)
    out = dict(ran=tw.run(30, 0, cfg["dt"], coupling_dt=1))
    out["gidx"] = np.array(tw.gidx)
    for nx, ny in SHAPES:
        for mx in (1e300, mx_median):
            t = _bits(tw.weld_overlaps(nx, ny, mx))
            out[(nx, ny, mx)] = dict(table=t, pairs=tw.weld_candidate_pairs(), again=_bits(tw.weld_overlaps(nx, ny, mx)))
    return out


def _s_stops(rank, world, dist):
    cfg = _star_cfg()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_welding([8], [3], [2], 1e300)
    out = dict(done=tw.run(40, 1, cfg["dt"], coupling_dt=1, stop_on_tags=True))
    out["stop"] = _snap(tw); out["table"] = _bits(tw.weld_overlaps(3, 2, 1e300))
    out["more"] = tw.run(32, 9, cfg["dt"], coupling_dt=1, stop_on_tags=True)
    return out


def _closing_run(w):
    w.set_welding([5], [1], [1], 2e9)
    return w.run(40, 0, BOX_DT, coupling_dt=1, coupling_on=False, stop_on_tags=True)


def _s_cut(rank, world, dist, done):
    """the first overlap's step as the last step of a sz_tile_run call, then as the first step of the next one"""
    out = {}
    for name, every in (("last", done), ("first", done - 1)):
        tw = _tiled(_closing_cfg(), rank, world, dist)
        tw.repartition_every = every
        out[name] = _closing_run(tw)
        out[name + "_table"] = _bits(tw.weld_overlaps(1, 1, 2e9))
    return out


def _s_never_and_through(rank, world, dist):
    cfg = _star_cfg()          # (seed 7: no floe is tagged in these steps, test_welding_never_met_and_run_through_do_not_perturb)
    tiny = 0.5 * float(np.min(cfg["derived"]["area"]))
    out = {}
    for name, stop, mx in (("off", True, None), ("never", True, tiny), ("off2", False, None), ("met", False, 1e300)):
        tw = _tiled(cfg, rank, world, dist)
        if mx is not None:
            tw.set_welding([8], [1], [1], mx)
        out["ran_" + name] = tw.run(NEVER_STEPS, 0, cfg["dt"], coupling_dt=1, stop_on_tags=stop)
        out[name] = _snap(tw)
        if mx is not None:
            out["n_" + name] = len(tw.weld_overlaps(1, 1, mx)[0])
    return out


def _fracture_first_run(w, cfg):
    from subzero_jl_amd import capi
    w.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=1.0, min_floe_area=1e6)
    w.set_welding([5], [1], [1], 1e300)
    return w.run(20, 1, cfg["dt"], coupling_dt=1, stop_on_tags=True)          # tsteps 1 .. 5: tstep 5 is a fracture step and a welding step


def _s_fracture_first(rank, world, dist):
    cfg = _star_cfg()
    tw = _tiled(cfg, rank, world, dist)
    out = dict(done=_fracture_first_run(tw, cfg))
    out["cand"] = tw.fracture_candidates(); out["n_table"] = len(tw.weld_overlaps(1, 1, 1e300)[0]); out["end"] = _snap(tw)
    return out


def _tag_run(w, cfg, weld_dt):
    if weld_dt:
        w.set_welding([weld_dt], [1], [1], 2e9)
    return w.run(TAG_STEPS, 0, cfg["dt"], coupling_dt=10, coupling_on=False, stop_on_tags=True)


def _s_tag_from_one_rank(rank, world, dist, weld_dt):
    cfg = _tag_listed_cfg()
    tw = _tiled(cfg, rank, world, dist)
    out = dict(gidx=np.array(tw.gidx), done=_tag_run(tw, cfg, weld_dt))
    tw.sync()
    out["status"] = tw.world.ids()[2][:len(tw.gidx)].copy()
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_straddle, _s_break, _s_parity, _s_stops, _s_cut, _s_never_and_through, _s_fracture_first, _s_tag_from_one_rank)}


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
    """the scenario on `world` spawned ranks: their results by rank.  A rank that does not answer in _collect's time fails the test; what is
    left waiting in a collective is ended"""
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
        for p in procs:
            if p.is_alive():
                p.terminate()
    return [out for _, out in sorted(res, key=lambda r: r[0])]


def _owner_of(res, n):
    owner = np.full(n, -1)
    for r, out in enumerate(res):
        owner[out["gidx"]] = r
    assert np.all(owner >= 0) and sum(len(o["gidx"]) for o in res) == n
    return owner


def _assert_ranks_equal_rows(snaps, ref, n, where):
    seen = np.concatenate([s["gidx"] for s in snaps])
    assert sorted(seen) == list(range(n)), (where, len(seen), n)
    for r, s in enumerate(snaps):
        _assert_bit_equal(s["cols"], rt.take_rows(ref, s["gidx"]), f"{where}, rank {r}")


# ---------------------------------------------------------------- the single context's side, once each
@pytest.fixture(scope="module")
def single_parity():
    """name -> what a single World gives after the same 30 steps: per (nx, ny, max_weld_area) the table and the candidate count"""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = _parity_cfg(name)
            hw = _single(cfg)
            assert hw.run(30, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 30
            med = float(np.median(cfg["derived"]["area"]))
            out = dict(median=med, n=hw.N, max_ring=int(np.diff(cfg["vert_off"]).max()), min_ring=int(np.diff(cfg["vert_off"]).min()))
            for nx, ny in SHAPES:
                for mx in (1e300, med):
                    out[(nx, ny, mx)] = dict(table=_bits(hw.weld_overlaps(nx, ny, mx)), pairs=hw.weld_candidate_pairs())
            cache[name] = out
        return cache[name]
    return get


@pytest.fixture(scope="module")
def single_closing():
    """the step of the first overlap, from the single context alone"""
    hw = _single(_closing_cfg())
    cx = hw.get("cx")
    assert cx[0] < BOX_L / 2 < cx[1]
    done = _closing_run(hw)
    assert 10 < done < 40 and (done - 1) % 5 == 0
    table = _bits(hw.weld_overlaps(1, 1, 2e9))
    assert table[0] == [0] and table[1] == [1]
    return dict(done=done, table=table)


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("big", [False, True], ids=["quadrilaterals", "a remote ring of 40 points"])
def test_a_pair_that_straddles_the_tile_edge(big):
    """floe 0 is rank 0's and floe 1 rank 1's: rank 0 owns the pair and clips it against the ring rank 1 sent -- through the large clip variant
    when that ring has more points than the small working set holds.  (1, 1): the single context's one entry; (2, 1): none; on both ranks"""
    cfg = _straddle_cfg(big)
    hw = _single(cfg)
    want = {nx: _bits(hw.weld_overlaps(nx, 1, 2e9)) for nx in (1, 2)}
    pairs = {}
    for nx in (1, 2):
        hw.weld_overlaps(nx, 1, 2e9); pairs[nx] = hw.weld_candidate_pairs()
    assert want[1][0] == [0] and want[1][1] == [1] and want[2] == ([], [], []) and pairs[1] >= 1
    assert (np.diff(cfg["vert_off"])[1] - 1 > 31) == big
    res = _ranks("straddle", 2, big)
    owner = _owner_of(res, cfg["n_floes"])
    assert owner[0] == 0 and owner[1] == 1, "the two floes are not owned by different ranks"
    for r, out in enumerate(res):
        for nx in (1, 2):
            assert out[nx] == want[nx], (r, nx, out[nx], want[nx])
            assert out[f"pairs{nx}"] == pairs[nx], (r, nx)
        assert out["rc_cap"] == E_ARG and out["n_cap"] == 1, (r, out["rc_cap"], out["n_cap"])
        assert out["after"] == want[1], r
    assert res[0][1] == res[1][1]


def test_the_break_reaches_across_ranks():
    """the out-of-bounds floe (number 3) lives on rank 0, the floes behind it in the list on rank 1: they are in no bin there either"""
    cfg = _break_cfg()
    hw = _single(cfg)
    want = hw.weld_bins(2, 2)
    assert want.tolist() == [0, 2, 3, -1, -1, -1, -1]
    res = _ranks("break", 2)
    owner = _owner_of(res, 7)
    assert owner[3] == 0 and set(owner[4:].tolist()) == {1}, owner
    for r, out in enumerate(res):
        assert out["bins"].tolist() == want[out["gidx"]].tolist(), (r, out["bins"], out["gidx"])
        assert out["table"] == _bits(hw.weld_overlaps(2, 2, 1e300)), r
    assert res[1]["bins"].tolist().count(-1) == 3


@pytest.mark.parametrize("name, world", [("star", 2), ("star", 4), ("voronoi500", 2), ("stars22to36", 2)])
def test_field_parity_with_the_single_context(single_parity, name, world):
    """after 30 steps, three bin shapes x two max_weld_area: table and candidate count are the single context's, twice the same bits.  The
    ranks of the 500-floe Voronoi field are told of rings over 20 points (its own have at most 12): sz_tile_run takes its list-based driver.
    The 500 stars of 22 .. 36 points take it on their own, and their rings go through the ring gather at field scale"""
    s = single_parity(name)
    if name == "stars22to36":
        assert s["min_ring"] - 1 > 20 and s["max_ring"] - 1 > 31
    res = _ranks("parity", world, name, s["median"])
    owner = _owner_of(res, s["n"])
    nonempty, cross = 0, 0
    for nx, ny in SHAPES:
        for mx in (1e300, s["median"]):
            want = s[(nx, ny, mx)]
            for r, out in enumerate(res):
                assert out["ran"] == 30
                got = out[(nx, ny, mx)]
                assert got["table"] == want["table"], (name, world, nx, ny, mx, r, len(got["table"][0]), len(want["table"][0]))
                assert got["pairs"] == want["pairs"], (name, world, nx, ny, mx, r, got["pairs"], want["pairs"])
                assert got["again"] == got["table"], (name, world, nx, ny, mx, r)
            i, j, _ = want["table"]
            nonempty += len(i) > 0
            cross += int(np.count_nonzero(owner[np.array(i, int)] != owner[np.array(j, int)])) if len(i) else 0
    assert nonempty >= 4, "the field does not exercise the table"
    assert cross >= 1, "no entry whose two floes are owned by different ranks"


def test_a_tiled_batch_stops_at_every_welding_step():
    """the dense star field with dts = [8], bins (3, 2), from tstep 1: run(40) returns 8 on every rank, as World.run does
    (test_dense_field_stops_at_every_welding_step), with the single context's state at that step; then run(32, 9) returns 8 again"""
    cfg = _star_cfg()
    hw = _single(cfg)
    hw.set_welding([8], [3], [2], 1e300)
    assert hw.run(40, 1, cfg["dt"], coupling_dt=1) == 8
    table = _bits(hw.weld_overlaps(3, 2, 1e300))
    assert len(table[0]) > 0
    ref = _cols(hw)
    res = _ranks("stops", 2)
    for r, out in enumerate(res):
        assert out["done"] == 8 and out["more"] == 8, (r, out["done"], out["more"])
        assert out["table"] == table, r
    _assert_ranks_equal_rows([o["stop"] for o in res], ref, hw.N, "at the first welding step")


def test_cut_batches_stop_on_the_step_of_the_first_overlap(single_closing):
    s = single_closing
    res = _ranks("cut", 2, s["done"])
    for r, out in enumerate(res):
        assert out["last"] == s["done"] and out["first"] == s["done"], (r, out["last"], out["first"], s["done"])
        assert out["last_table"] == s["table"] and out["first_table"] == s["table"], r


def test_never_met_and_run_through_do_not_perturb_a_tiled_run():
    """welding set with max_weld_area under every floe runs all steps bit-equal to the same tiled run with welding off; so does a batch that
    runs through (stop_on_tags=False) with welding met"""
    res = _ranks("never_and_through", 2)
    for r, out in enumerate(res):
        assert [out["ran_" + k] for k in ("off", "never", "off2", "met")] == [NEVER_STEPS] * 4, r
        assert np.array_equal(out["never"]["gidx"], out["off"]["gidx"]) and np.array_equal(out["met"]["gidx"], out["off2"]["gidx"])
        _assert_bit_equal(out["never"]["cols"], out["off"]["cols"], f"never met, rank {r}")
        _assert_bit_equal(out["met"]["cols"], out["off2"]["cols"], f"run through, rank {r}")
        assert out["n_never"] == 0 and out["n_met"] > 0


def test_a_fracture_candidate_on_a_welding_step_ends_the_batch_first():
    cfg = _star_cfg()
    hw = _single(cfg)
    done = _fracture_first_run(hw, cfg)
    cand = hw.fracture_candidates()
    assert done == 5 and len(cand) > 0 and len(hw.weld_overlaps(1, 1, 1e300)[0]) > 0
    ref = _cols(hw)
    res = _ranks("fracture_first", 2)
    for r, out in enumerate(res):
        assert out["done"] == done, (r, out["done"], done)
        assert np.array_equal(out["cand"], cand) and out["n_table"] > 0, r
    _assert_ranks_equal_rows([o["end"] for o in res], ref, hw.N, "fracture first")


def test_a_tag_one_rank_raises_on_a_welding_step_ends_the_batch():
    """rank 1's floe reaches the open boundary on a step that welding makes a segment's last: behind the list-based driver only rank 1 knows of
    the tag, and the pass's last agreement tells rank 0 -- steps_done is the single context's on both"""
    cfg = _tag_listed_cfg()
    assert int(np.diff(cfg["vert_off"]).max()) - 1 > 20
    plain = _tag_run(_single(cfg), cfg, 0)
    assert 2 < plain < TAG_STEPS
    weld_dt = plain - 1          # the tag's tstep (and tstep 0: an empty table, the batch goes on)
    hw = _single(cfg)
    assert _tag_run(hw, cfg, weld_dt) == plain
    assert len(hw.weld_overlaps(1, 1, 2e9)[0]) == 0
    res = _ranks("tag_from_one_rank", 2, weld_dt)
    tagged = [int(np.count_nonzero(out["status"] != wr.ACTIVE)) for out in res]
    assert tagged[0] == 0 and tagged[1] > 0, tagged
    for r, out in enumerate(res):
        assert out["done"] == plain, (r, out["done"], plain)


def test_new_refusals():
    from subzero_jl_amd import capi, fields, tiles
    cfg = fields.make_config(n_floes=400, seed=80, subgrid_per_floe=4.0)
    n = C.c_int32(0)
    # tiled by sz_tile_enable alone: no set-up, no communicator
    w = fields.build_world(mk(), cfg)
    w._push()
    gidx = np.arange(w.N, dtype=np.int64)
    assert w.L.sz_tile_enable(w.h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    assert w.L.sz_tile_weld_overlaps(w.h, 1, 1, 2e9, C.byref(n), 0, None, None, None) == E_STATE
    assert b"sz_tile_setup" in w.L.sz_last_error(w.h)
    # arguments
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    w = tw.world
    assert w.L.sz_tile_weld_overlaps(w.h, 0, 1, 2e9, C.byref(n), 0, None, None, None) == E_ARG
    assert w.L.sz_tile_weld_overlaps(w.h, 1, 1, -1.0, C.byref(n), 0, None, None, None) == E_ARG
    assert len(tw.weld_overlaps(1, 1, 1e300)[0]) > 0
    # two-way coupling across tiles with welding set
    tw.set_welding([5], [1], [1])
    w.set_two_way(True, dt=cfg["dt"])
    done = C.c_int32(0)
    for flags in (capi.COLLISIONS_ON, capi.COLLISIONS_ON | capi.NO_STOP):
        assert w.L.sz_tile_run(w.h, 4, 1, cfg["dt"], 1, flags, C.byref(done)) == E_STATE
        assert b"two-way" in w.L.sz_last_error(w.h) and b"welding" in w.L.sz_last_error(w.h)
    tw.backend = "torch"          # (the host-driven steps: no library channel)
    with pytest.raises(capi.SzError):
        tw.set_welding([5], [1], [1])
    with pytest.raises(capi.SzError):
        tw.weld_overlaps(1, 1)

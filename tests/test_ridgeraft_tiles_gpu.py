"""Ridge / raft candidates on tiled contexts (csrc/sz_ridgeraft_tile.hpp; sz_tile_run with ridge / raft set, sz_tile_ridgeraft_candidates,
sz_tile_list_numbers, sz_tile_step_finish; DESIGN.md §9e, "tiled contexts"): ranks are spawned processes that share the one GPU and trade through
gloo (backend "library-host"), as in tests/test_weld_tiles_gpu.py.  No tolerance appears anywhere: both sides read the same row bits.

  Tables        a tiled table is compared with the single context's table at the same pending stop, both built from the same config and driven
                by the same run(): entry for entry, kind and frac as bits, the draws equal.
  Trajectories  a tiled run with ridge / raft set is compared with the same tiled run with it off and with the single context with it off,
                whether its ridge / raft steps run through or are finished at once: bit for bit on the owned columns and ring points.
  NOT asserted  equality with a single context that has ridge / raft ON across such a step: that context's split step sums the collision totals in
                process-mode order, the tiled list-based step uses the fixed-point sums.
"""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

import remove_tiles_ref as rt
from test_remove_gpu import _assert_bit_equal, _cols, mk
from test_fracture_tiles_gpu import _retile
from test_remove_tiles_gpu import _rank_cols, _tiled
from test_ridgeraft_gpu import HAND, RUN_THROUGH, _dense, _field_heights, _square, _thick
from test_tiles_gpu import _collect, _free_port, _guard
from test_weld_tiles_gpu import LISTED_RING_HINT, _assert_ranks_equal_rows, _owner_of, _tag_listed_cfg

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
RUN = dict(coupling_dt=1, stop_on_tags=True)
OFF_STEPS = 24
TAG_STEPS = 12
# (centre x, centre y, height) of the hand-made squares of side 8 km, in list order; rank 0 owns the floes with cx < L / 2
HAND_FLOES = [(4.7e4, 5e4, 0.25), (5.4e4, 5e4, 0.25),          # 0 | 1: the pair straddles the tile edge; both can ridge and raft
              (3e3, 3e4, 1.0), (9.55e4, 3e4, 1.0),             # 2 | 3: through the periodic west / east wall; ridge only
              (3e3, 9.7e4, 0.25),                              # 4: across the west wall AND on the north collision wall: so is its ghost
              (3e4, 3.5e3, 1.0),                               # 5: on the south collision wall
              (7.7e4, 7e4, 0.1),                               # 6: on the topography square
              (2e4, 7e4, 0.1), (2.7e4, 7e4, 0.1),              # 7, 8: too thin to ridge: raft only
              (7e4, 2e4, 6.0), (7.7e4, 2e4, 0.25), (2e4, 2e4, 0.25), (2.7e4, 2e4, 6.0),          # 9 .. 12: a floe over every maximum as i, as j: none
              (1.5e4, 5e4, 0.5), (3.3e4, 8.5e4, 0.5), (6.5e4, 4.5e4, 0.5), (8.7e4, 5e4, 0.5), (8.7e4, 8.7e4, 0.5), (5.5e4, 8.7e4, 0.5), (4.5e4, 2e4, 0.5)]
HAND_TOPO = (7e4, 7e4, 8e3)


# ---------------------------------------------------------------- fields
def _hand_cfg():
    """twenty squares on the pattern of _hand_world (tests/test_ridgeraft_gpu.py): E / W periodic, N / S collision walls, one topography square"""
    from subzero_jl_amd import floe as floe_mod
    rings = [_square(x, y, 8e3) for x, y, _ in HAND_FLOES]
    n = len(rings)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(r) for r in rings])
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    h = np.array([f[2] for f in HAND_FLOES])
    z = np.zeros((11, 11))
    return dict(n_floes=n, L=1e5, kinds=["collision", "collision", "periodic", "periodic"], vert_off=off, vx=vx, vy=vy, height=h, u=np.zeros(n), v=np.zeros(n),
                xi=np.zeros(n), dt=10, Nx=10, Ny=10, uo=z, vo=z, hf=z, ua=z, va=z, topography=[_square(*HAND_TOPO)], E=6e6,
                derived=floe_mod.derive(off, vx, vy, h), sub_off=np.zeros(n + 1, np.int32), sx=np.zeros(0), sy=np.zeros(0), seed=0)


def _with_heights(cfg, h):
    from subzero_jl_amd import floe as floe_mod
    cfg["height"] = np.asarray(h, float)
    cfg["derived"] = floe_mod.derive(cfg["vert_off"], cfg["vx"], cfg["vy"], cfg["height"])
    return cfg


def _field_cfg():
    """_dense() of tests/test_ridgeraft_gpu.py, heights on both sides of every threshold"""
    cfg = _dense()
    return _with_heights(cfg, _field_heights(cfg["n_floes"]))


def _through_cfg(name):
    from subzero_jl_amd import fields
    over, h = RUN_THROUGH[name]
    cfg = fields.make_config(n_floes=400, seed=11, subgrid_per_floe=4.0, **over)
    return cfg if h is None else _with_heights(cfg, np.full(cfg["n_floes"], h))


def _tag_cfg_thick():
    """the field of _tag_listed_cfg (one rank's floe reaches the open boundary; the list-based driver) with heights over every maximum"""
    cfg = _tag_listed_cfg()
    return _with_heights(cfg, np.full(cfg["n_floes"], 6.0))


def _single(cfg):
    from subzero_jl_amd import fields
    return fields.build_world(mk(), cfg)


def _bits(t):
    """a table as comparable python values: numbers, kinds, the fracs as bit patterns, the draws"""
    i, j, k, f, nd = t
    return [int(x) for x in i], [int(x) for x in j], [int(x) for x in k], np.asarray(f, np.float64).view(np.uint64).tolist(), int(nd)


# ---------------------------------------------------------------- ranks
def _snap(tw):
    return dict(gidx=np.array(tw.gidx), cols=_rank_cols(tw))


def _launches(w):
    return {k: v[1] for k, v in w.kernel_times().items()}


def _s_hand(rank, world, dist):
    cfg = _hand_cfg()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_ridgeraft(True, dt=10, **HAND)
    out = dict(gidx=np.array(tw.gidx), ran=tw.run(1, 10, cfg["dt"], **RUN), pending=tw.ridgeraft_pending())
    out["table"] = _bits(tw.ridgeraft_candidates()); out["again"] = _bits(tw.ridgeraft_candidates())
    return out


def _s_field(rank, world, dist, listed, carry):
    from subzero_jl_amd import capi
    cfg = _field_cfg()
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    if listed:
        tw._max_ring = LISTED_RING_HINT
        _retile(tw)
    tw.set_ridgeraft(True, dt=10)
    w = tw.world
    out = dict(gidx=np.array(tw.gidx), ran=tw.run(40, 1, dt, **RUN), pending=tw.ridgeraft_pending())
    out["table"] = _bits(tw.ridgeraft_candidates()); out["again"] = _bits(tw.ridgeraft_candidates())
    # the local list at the stop: list numbers, order keys, floe.interactions of every local row
    out["nums"], out["keys"] = tw.list_numbers(), tw.list_keys()
    out["inter"] = w.interactions()
    out["M_stop"] = w.stats()["M"]
    # stop, refuse
    flags = capi.COLLISIONS_ON | capi.COUPLING_ON
    done = C.c_int32(7)
    out["rc_run"] = w.L.sz_tile_run(w.h, 5, 10, dt, 1, flags, C.byref(done)); out["done_run"] = done.value; out["msg_run"] = w.L.sz_last_error(w.h)
    sent, owned = C.c_int64(0), C.c_int64(0)
    out["rc_migrate"] = w.L.sz_tile_migrate(w.h, 2, 1, None, C.byref(sent), C.byref(owned)); out["msg_migrate"] = w.L.sz_last_error(w.h)
    out["rc_wrong_tstep"] = w.L.sz_tile_step_finish(w.h, 11, dt, 1, flags)
    n = C.c_int32(0); i1 = np.zeros(1, np.int64)
    out["rc_cap"] = w.L.sz_tile_ridgeraft_candidates(w.h, C.byref(n), 1, capi.ptr(i1, capi._lp), None, None, None, None); out["n_cap"] = n.value
    out["after_refusals"] = _bits(tw.ridgeraft_candidates())
    # finish
    tw.finish_step(10, dt, coupling_dt=1)
    st = w.stats()
    out["pending_after"], out["N_after"], out["M_after"] = tw.ridgeraft_pending(), st["N"], st["M"]
    if not carry:
        return out
    # carry on: 25 steps from tstep 1 stop at 10 and 20 and are finished at once; the same tiled run with ridge / raft off
    stops, done = [10], 10
    while done < 25:
        done += tw.run(25 - done, 1 + done, dt, **RUN)
        p = tw.ridgeraft_pending()
        if p >= 0:
            stops.append(p)
            tw.finish_step(p, dt, coupling_dt=1)
            done += 1
    out["stops"] = stops
    out["on"] = _snap(tw)
    t2 = _tiled(cfg, rank, world, dist)
    out["ran_off"] = t2.run(25, 1, dt, **RUN)
    out["off"] = _snap(t2)
    return out


def _s_through(rank, world, dist, name):
    """45 steps from tstep 1 with dt = 10 in calls of 9 (tstep 10 is the first step of a call) and of 10 (the last step of one)"""
    cfg = _through_cfg(name)
    out = {}
    for every in (9, 10):
        for rr_on in (True, False):
            tw = _tiled(cfg, rank, world, dist)
            tw.repartition_every = every
            if rr_on:
                tw.set_ridgeraft(True, dt=10)
            key = (every, rr_on)
            out[key] = dict(ran=tw.run(45, 1, cfg["dt"], **RUN), pending=tw.ridgeraft_pending(), draws=tw.ridgeraft_draws(), snap=_snap(tw))
    return out


def _tag_run(w, cfg, rr_dt):
    if rr_dt:
        w.set_ridgeraft(True, dt=rr_dt)
    return w.run(TAG_STEPS, 0, cfg["dt"], coupling_dt=10, coupling_on=False, stop_on_tags=True)


def _s_tag(rank, world, dist, rr_dt):
    cfg = _tag_cfg_thick()
    out = dict(gidx=None)
    for name, d in (("off", 0), ("on", rr_dt)):
        tw = _tiled(cfg, rank, world, dist)
        out[name] = dict(done=_tag_run(tw, cfg, d), pending=tw.ridgeraft_pending(), draws=tw.ridgeraft_draws())
        tw.sync()
        out[name]["status"] = tw.world.ids()[2][:len(tw.gidx)].copy()
        out["gidx"] = np.array(tw.gidx)
    return out


def _fracture_run(w, cfg, rr_on):
    from subzero_jl_amd import capi
    w.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=1.0, min_floe_area=1e6)
    first = w.run(4, 1, cfg["dt"], **RUN)
    if rr_on:
        w.set_ridgeraft(True, dt=5)
    return first, w.run(20, 5, cfg["dt"], **RUN), len(w.fracture_candidates()), w.ridgeraft_pending()


def _s_fracture(rank, world, dist):
    cfg = _thick(_dense())
    return {rr_on: _fracture_run(_tiled(cfg, rank, world, dist), cfg, rr_on) for rr_on in (False, True)}


def _s_off(rank, world, dist):
    cfg = _field_cfg()
    out = {}
    for name, stop, setup in (("never", True, lambda t: None), ("on_then_off", True, lambda t: (t.set_ridgeraft(True, dt=10), t.set_ridgeraft(False))),
                              ("never2", False, lambda t: None), ("no_stop", False, lambda t: t.set_ridgeraft(True, dt=10))):
        tw = _tiled(cfg, rank, world, dist)
        setup(tw)
        tw.world.profile(True)
        ran = tw.run(OFF_STEPS, 1, cfg["dt"], coupling_dt=1, stop_on_tags=stop)
        tw.sync()
        out[name] = dict(ran=ran, launches=_launches(tw.world), snap=_snap(tw), pending=tw.ridgeraft_pending())
    return out


def _s_refuse(rank, world, dist):
    from subzero_jl_amd import capi
    cfg = _field_cfg()
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_ridgeraft(True, dt=10)
    w = tw.world
    L, h = w.L, w.h
    n, nd, done = C.c_int32(0), C.c_int64(0), C.c_int32(0)
    one = np.zeros(1, np.int64)
    out = dict(
        candidates=L.sz_tile_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)),          # nothing pending
        numbers=L.sz_tile_list_numbers(h, capi.ptr(one, capi._lp), 1),
        finish=L.sz_tile_step_finish(h, 10, dt, 1, capi.COLLISIONS_ON),
        no_collisions=L.sz_tile_run(h, 3, 1, dt, 1, capi.COUPLING_ON, C.byref(done)),
        tile_step=L.sz_tile_step(h, None, world, 0, 1, dt, 1, capi.COLLISIONS_ON),
        step=L.sz_step(h, 3, 1, dt, 1, capi.COLLISIONS_ON, C.byref(done)),
        single_candidates=L.sz_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)))
    out["then"] = tw.run(3, 1, dt, **RUN)
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_hand, _s_field, _s_through, _s_tag, _s_fracture, _s_off, _s_refuse)}


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


# ---------------------------------------------------------------- the single context's side, once each
@pytest.fixture(scope="module")
def single_field():
    """the single context at its own stop (40 steps from tstep 1 with dt = 10: pending at 10), and the same field 25 steps on with ridge / raft off"""
    cfg = _field_cfg()
    A = _single(cfg)
    A.set_ridgeraft(True, dt=10)
    assert A.run(40, 1, cfg["dt"], coupling_dt=1) == 9 and A.ridgeraft_pending() == 10
    table = _bits(A.ridgeraft_candidates())
    assert len(table[0]) > 50, "the field does not exercise the table"
    off, rows = A.interactions()
    N, M = cfg["n_floes"], A.M
    root = np.arange(M)
    for i, gl in enumerate(A.ghosts()):
        for g in gl:
            root[g] = root[i]
    assert np.all(root < N) and M > N
    B = _single(cfg)
    assert B.run(25, 1, cfg["dt"], coupling_dt=1) == 25
    return dict(cfg=cfg, table=table, off=off.copy(), rows=rows.copy(), N=N, M=M, root=root, end25=_cols(B))


@pytest.fixture(scope="module")
def two_ranks():
    """test 2's run on two ranks, carried on through tests 3 and 4"""
    return _ranks("field", 2, False, True)


# ---------------------------------------------------------------- tests
def test_hand_made_field_on_two_ranks():
    """one step at tstep % dt == 0: every rank is pending, the table is the single context's entry for entry on both ranks and on a second call.
    The field: a pair that straddles the tile edge (i on rank 0, j on rank 1); a pair through the periodic wall whose floes live on different
    ranks (the entry of floe 3 names the ghost of floe 2); a ghost as i (floe 4's, on the north wall); floes on a collision wall and on the
    topography square; heights that give kind 1, 2, 3 and none"""
    cfg = _hand_cfg()
    N = cfg["n_floes"]
    hw = _single(cfg)
    hw.set_ridgeraft(True, dt=10, **HAND)
    assert hw.run(1, 10, cfg["dt"], coupling_dt=1) == 0 and hw.ridgeraft_pending() == 10
    want = _bits(hw.ridgeraft_candidates())
    tab = {(i, j): k for i, j, k in zip(*want[:3])}
    assert hw.M == N + 2
    assert tab[(0, 2)] == 3 and tab[(7, 9)] == 2 and tab[(5, -2)] == 1 and tab[(6, -5)] == 3 and tab[(4, -1)] == 3
    assert not any(i in (9, 11) for i, _ in tab), "a floe over every maximum, as i and as j"
    gj = [(i, j) for i, j in tab if j - 1 >= N]
    gi = [(i, j) for i, j in tab if i >= N]
    assert gj and gj[0][0] == 3 and tab[gj[0]] == 1 and gi and gi[0][1] == -1, (gi, gj)
    res = _ranks("hand", 2)
    owner = _owner_of(res, N)
    assert owner[0] == 0 and owner[1] == 1 and owner[2] == 0 and owner[3] == 1 and owner[4] == 0
    for r, out in enumerate(res):
        assert out["ran"] == 0 and out["pending"] == 10, (r, out["ran"], out["pending"])
        assert out["table"] == want, (r, out["table"], want)
        assert out["again"] == out["table"], r
    assert res[0]["table"] == res[1]["table"]


@pytest.mark.parametrize("world, listed", [(2, False), (4, False), (2, True)], ids=["2 ranks", "2x2 ranks", "2 ranks, list-based segments"])
def test_field_parity_with_the_single_context(single_field, two_ranks, world, listed):
    """_dense() with _field_heights, 40 steps from tstep 1 with dt = 10: run returns 9, every rank is pending at 10, and the table equals the single
    context's at its own stop.  Once more with the ring hint that sends the segments down the list-based driver"""
    s = single_field
    res = two_ranks if (world, listed) == (2, False) else _ranks("field", world, listed, False)
    owner = _owner_of(res, s["N"])
    for r, out in enumerate(res):
        assert out["ran"] == 9 and out["pending"] == 10, (r, out["ran"], out["pending"])
        assert out["table"] == s["table"], (world, listed, r, len(out["table"][0]), len(s["table"][0]))
        assert out["again"] == out["table"] and out["after_refusals"] == out["table"], r
    i, j = np.array(s["table"][0]), np.array(s["table"][1])
    root = s["root"]
    cross = int(np.count_nonzero((j > 0) & (owner[root[i]] != owner[root[np.maximum(j, 1) - 1]])))
    assert cross >= 1, "no entry whose two floes are owned by different ranks"
    assert np.any(j - 1 >= s["N"]), "no entry names a ghost"


def test_list_numbers_and_rows_at_the_stop(single_field, two_ranks):
    """each rank's interaction rows of its owned parents and of their ghosts, the partner column translated through list_numbers (by way of the
    order keys), are the single context's rows of those list rows, bit for bit and in order; every list number 0 .. M - 1 is claimed by exactly
    one rank's evaluated rows"""
    s = single_field
    N, M, root = s["N"], s["M"], s["root"]
    owner = _owner_of(two_ranks, N)
    claimed = np.zeros(M, int)
    for r, out in enumerate(two_ranks):
        nums, keys = out["nums"], out["keys"]
        off, rows = out["inter"]
        assert len(nums) == len(keys) == out["M_stop"] == len(off) - 1
        n_own = len(out["gidx"])
        assert np.array_equal(nums[:n_own], out["gidx"]) and np.array_equal(keys[:n_own], out["gidx"])
        number_of = {int(k): int(v) for k, v in zip(keys, nums)}
        for k in range(len(nums)):
            Lk = int(nums[k])
            if Lk < 0 or owner[root[Lk]] != r:
                continue
            claimed[Lk] += 1
            mine = rows[off[k]:off[k + 1]].copy()
            for row in mine:
                if row[0] > 0:
                    row[0] = float(number_of[int(row[0]) - 1] + 1)
            want = s["rows"][s["off"][Lk]:s["off"][Lk + 1]]
            assert mine.shape == want.shape and np.array_equal(mine.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (r, k, Lk)
    assert np.all(claimed == 1), (np.nonzero(claimed != 1)[0][:10], claimed[claimed != 1][:10])


def test_stop_refuse_finish_and_carry_on(single_field, two_ranks):
    s = single_field
    for r, out in enumerate(two_ranks):
        assert out["rc_run"] == E_STATE and out["done_run"] == 0 and b"sz_tile_step_finish" in out["msg_run"], (r, out["rc_run"], out["done_run"], out["msg_run"])
        assert out["rc_migrate"] == E_STATE and b"sz_tile_step_finish" in out["msg_migrate"], r
        assert out["rc_wrong_tstep"] == E_ARG and out["rc_cap"] == E_ARG and out["n_cap"] == len(s["table"][0]), r
        assert out["M_stop"] > len(out["gidx"]), "no halo rows or ghosts at the stop"
        assert out["pending_after"] == -1 and out["N_after"] == out["M_after"] == len(out["gidx"]), (r, out["N_after"], out["M_after"])
        assert out["stops"] == [10, 20] and out["ran_off"] == 25, (r, out["stops"], out["ran_off"])
        _assert_bit_equal(out["on"]["cols"], out["off"]["cols"], f"finished at once against ridge / raft off, rank {r}")
        assert np.array_equal(out["on"]["gidx"], out["off"]["gidx"])
    _assert_ranks_equal_rows([o["on"] for o in two_ranks], s["end25"], s["N"], "finished at once against the single context with ridge / raft off")


@pytest.mark.parametrize("name", list(RUN_THROUGH))
def test_run_through_empty_tables(name):
    """45 steps from tstep 1 with dt = 10, cut into calls of 9 steps (tstep 10 is a call's first step) and of 10 (its last): all steps done, nothing
    pending, the draws summed over the calls are the single context's for the same run, the state is the tiled and the single run's with the
    setting off, bit for bit.  (Not asserted: equality with a single context that has ridge / raft ON across such a step -- see the module.)"""
    cfg = _through_cfg(name)
    n = cfg["n_floes"]
    A = _single(cfg)
    A.set_ridgeraft(True, dt=10)
    assert A.run(45, 1, cfg["dt"], coupling_dt=1) == 45 and A.ridgeraft_pending() == -1
    draws = A.ridgeraft_draws()
    assert draws == (0 if name == "too_thick" else 8 * n)
    B = _single(cfg)
    assert B.run(45, 1, cfg["dt"], coupling_dt=1) == 45
    ref = _cols(B)
    res = _ranks("through", 2, name)
    for every in (9, 10):
        for r, out in enumerate(res):
            on, off = out[(every, True)], out[(every, False)]
            assert on["ran"] == off["ran"] == 45 and on["pending"] == -1, (every, r, on["ran"], off["ran"], on["pending"])
            assert on["draws"] == draws and off["draws"] == 0, (every, r, on["draws"], draws)
            assert np.array_equal(on["snap"]["gidx"], off["snap"]["gidx"])
            _assert_bit_equal(on["snap"]["cols"], off["snap"]["cols"], f"{name}, calls of {every}, rank {r}")
        _assert_ranks_equal_rows([o[(every, True)]["snap"] for o in res], ref, n, f"{name}, calls of {every}")
    if name == "too_thick":
        over = np.concatenate([o[(9, True)]["snap"]["cols"]["overarea"] for o in res])
        assert np.count_nonzero(over) > n // 4, "the dense field is not in contact"


def test_a_tag_one_rank_raises_on_an_empty_ridge_raft_step_ends_the_batch():
    """rank 1's floe reaches the open boundary on a ridge / raft step whose table is empty (heights over every maximum): the step runs through, and
    the agreement behind its second half tells rank 0 -- steps_done is that of the same run without ridge / raft on both"""
    cfg = _tag_cfg_thick()
    plain = _tag_run(_single(cfg), cfg, 0)
    assert 2 < plain < TAG_STEPS
    rr_dt = plain - 1          # the tag's tstep (and tstep 0: an empty table, the batch goes on)
    res = _ranks("tag", 2, rr_dt)
    tagged = [int(np.count_nonzero(out["on"]["status"] != 1)) for out in res]
    assert tagged[0] == 0 and tagged[1] > 0, tagged
    for r, out in enumerate(res):
        assert out["off"]["done"] == plain and out["on"]["done"] == plain, (r, out["off"]["done"], out["on"]["done"], plain)
        assert out["on"]["pending"] == -1 and out["on"]["draws"] == 0
        assert np.array_equal(out["on"]["status"], out["off"]["status"])


def test_a_fracture_candidate_on_an_empty_ridge_raft_step_ends_the_batch_first():
    res = _ranks("fracture", 2)
    for r, out in enumerate(res):
        off, on = out[False], out[True]
        assert off[0] == on[0] == 4 and off[1] == on[1] == 1 and on[2] == off[2] > 0 and on[3] == -1, (r, off, on)
    assert res[0][True] == res[1][True]


def test_off_means_off():
    """set_ridgeraft(True) then (False) against never set, and ridge / raft set under SZ_NO_STOP against not set: the state is bit-equal and the
    launched kernel classes and counts are the same"""
    res = _ranks("off", 2)
    for r, out in enumerate(res):
        for a, b in (("never", "on_then_off"), ("never2", "no_stop")):
            assert out[a]["ran"] == out[b]["ran"] == OFF_STEPS and out[b]["pending"] == -1, (r, a, out[a]["ran"], out[b]["ran"])
            assert np.array_equal(out[a]["snap"]["gidx"], out[b]["snap"]["gidx"])
            _assert_bit_equal(out[a]["snap"]["cols"], out[b]["snap"]["cols"], f"{b}, rank {r}")
            assert out[a]["launches"] == out[b]["launches"], (r, b, out[a]["launches"], out[b]["launches"])
            assert sum(out[a]["launches"].values()) > OFF_STEPS


def test_new_refusals():
    from subzero_jl_amd import capi, fields, tiles
    # on every rank of a tiled run, nothing pending; the context is usable afterwards
    for r, out in enumerate(_ranks("refuse", 2)):
        for k in ("candidates", "numbers", "finish", "no_collisions", "tile_step", "step", "single_candidates"):
            assert out[k] == E_STATE, (r, k, out[k])
        assert out["then"] == 3, (r, out["then"])
    cfg = fields.make_config(n_floes=400, seed=80, subgrid_per_floe=4.0)
    done = C.c_int32(0)
    # tiled by sz_tile_enable alone: no set-up, no communicator
    w = fields.build_world(mk(), cfg)
    w._push()
    w.set_ridgeraft(True, dt=10)
    gidx = np.arange(w.N, dtype=np.int64)
    assert w.L.sz_tile_enable(w.h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    assert w.L.sz_tile_run(w.h, 4, 1, cfg["dt"], 1, capi.COLLISIONS_ON, C.byref(done)) == E_STATE
    assert b"ridge / raft" in w.L.sz_last_error(w.h) and b"sz_tile_setup" in w.L.sz_last_error(w.h)
    # two-way coupling across tiles with ridge / raft set
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    tw.set_ridgeraft(True, dt=10)
    tw.world.set_two_way(True, dt=cfg["dt"])
    for flags in (capi.COLLISIONS_ON, capi.COLLISIONS_ON | capi.NO_STOP):
        assert tw.world.L.sz_tile_run(tw.world.h, 4, 1, cfg["dt"], 1, flags, C.byref(done)) == E_STATE
        assert b"two-way" in tw.world.L.sz_last_error(tw.world.h) and b"ridge / raft" in tw.world.L.sz_last_error(tw.world.h)
    tw.backend = "torch"          # (the host-driven steps: no library channel)
    with pytest.raises(capi.SzError):
        tw.set_ridgeraft(True, dt=10)
    with pytest.raises(capi.SzError):
        tw.ridgeraft_candidates()

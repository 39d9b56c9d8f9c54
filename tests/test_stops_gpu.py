"""The stop schedule (csrc/sz_stops.hpp; DESIGN.md, "Stop schedule") with all four reasons set at once -- a criterion, welding, ridge / raft and
removal -- on a field that never meets any of them: the batch runs through every kind of cut, counts the draws and perturbs nothing.  On the
single context (sz_step) and on two ranks (sz_tile_run, both segment drivers); ranks are spawned processes that share the one GPU and trade
through gloo, as in tests/test_ridgeraft_tiles_gpu.py.  No tolerance appears anywhere: every comparison is bit for bit.

13 steps from tstep 0 with ridge / raft Δt 3, fracture Δt 2, welding Δts [4, 6]: tsteps 0, 6 and 12 are ridge / raft, fracture and welding steps
at once (12 of both welding sets: the first), 4 is a fracture and a welding step, 3 and 9 ridge / raft steps alone, 2, 8 and 10 fracture steps."""
import datetime
import os

import numpy as np
import pytest

import fracture_ref as fr
import ridgeraft_ref as rr
import weld_ref as wr
from test_fracture_tiles_gpu import _retile
from test_remove_gpu import _assert_bit_equal, _cols, mk
from test_remove_tiles_gpu import _rank_cols, _tiled
from test_tiles_gpu import _collect, _free_port, _guard
from test_weld_tiles_gpu import LISTED_RING_HINT, _assert_ranks_equal_rows

pytestmark = pytest.mark.gpu

STEPS, RR_DT, FRAC_DT, WELD = 13, 3, 2, ([4, 6], [2, 1], [2, 1])
MAX_WELD_AREA = 2e9


def _quiet_cfg():
    """50 floes on a lattice of 8 x 8 cells between periodic walls, small enough never to touch (concentration 0.1), moved half a cell west and
    south so that the first column and row lie ON the walls: 15 of them have ghosts"""
    from subzero_jl_amd import fields, floe as floe_mod
    cfg = fields.make_config(n_floes=50, seed=11, concentration=0.1, subgrid_per_floe=4.0)
    L, off = cfg["L"], cfg["vert_off"]
    for k, c in (("vx", "cx"), ("vy", "cy")):
        shift = -1.0e4 + np.where(cfg["derived"][c] < 1.0e4, L, 0.0)
        cfg[k] = cfg[k] + np.repeat(shift, np.diff(off))
    cfg["derived"] = floe_mod.derive(off, cfg["vx"], cfg["vy"], cfg["height"])
    return cfg


def _set_all(w):
    from subzero_jl_amd import capi
    w.set_fracture(capi.FRAC_POLYGON, dt=FRAC_DT, poly=fr.huge_square(), min_floe_area=1e6)
    w.set_welding(*WELD, MAX_WELD_AREA)
    w.set_ridgeraft(True, dt=RR_DT)
    w.set_removal()
    return w


def _single(cfg):
    from subzero_jl_amd import fields
    return fields.build_world(mk(), cfg)


def _oracle_draws(cfg):
    """the reference's order on the CPU oracle: every table, flag and overlap stays empty; the per-floe draws of the ridge / raft steps"""
    from oracle import orc
    from subzero_jl_amd import fields
    n, dt, L = cfg["n_floes"], cfg["dt"], cfg["L"]
    ow = fields.build_world(orc.World(), cfg)
    per_x, per_y = wr.periodic_flags(cfg["kinds"])
    draws, ghosts = 0, 0
    for t in range(STEPS):
        ow.add_ghosts(); ow.timestep_collisions(n, dt)
        ghosts = max(ghosts, len(ow.get("height")) - n)
        if t % RR_DT == 0:
            table, nd = rr.table(ow)
            assert table == []
            draws += nd
        ow.remove_ghosts(n); ow.timestep_coupling(); ow.timestep_floe_properties(dt)
        k = next((i for i, d in enumerate(WELD[0]) if t % d == 0), -1)          # (the criterion is a polygon no σ-point leaves: nothing to walk)
        if k >= 0:
            _, areas = wr.overlaps(ow, (0.0, L, 0.0, L), per_x, per_y, WELD[1][k], WELD[2][k], MAX_WELD_AREA)
            assert not np.any(np.asarray(areas) > 0)
        assert sum(ow.simplify_check(30, 1e6, 0.1)) == 0
    assert ghosts > 0, "no floe lies across a wall"
    return draws


# ---------------------------------------------------------------- ranks
def _s_all_four(rank, world, dist):
    cfg = _quiet_cfg()
    out = {}
    for listed in (False, True):
        tw = _tiled(cfg, rank, world, dist)
        if listed:
            tw._max_ring = LISTED_RING_HINT
            _retile(tw)
        _set_all(tw)
        out[listed] = dict(ran=tw.run(STEPS, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True), pending=tw.ridgeraft_pending(), draws=tw.ridgeraft_draws(),
                           snap=dict(gidx=np.array(tw.gidx), cols=_rank_cols(tw)))
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_all_four,)}


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


# ---------------------------------------------------------------- the single context's side, once
@pytest.fixture(scope="module")
def quiet():
    cfg = _quiet_cfg()
    B = _single(cfg)
    assert B.run(STEPS, 0, cfg["dt"], coupling_dt=1) == STEPS
    return dict(cfg=cfg, draws=_oracle_draws(cfg), off=_cols(B))


def test_all_four_set_and_never_met_on_the_single_context(quiet):
    cfg = quiet["cfg"]
    A = _set_all(_single(cfg))
    assert A.run(STEPS, 0, cfg["dt"], coupling_dt=1) == STEPS and A.ridgeraft_pending() == -1
    assert A.ridgeraft_draws() == quiet["draws"] > 0
    _assert_bit_equal(_cols(A), quiet["off"], "all four set against none")


def test_all_four_set_and_never_met_on_two_ranks(quiet):
    """sz_tile_run with its inline and with its list-based segments, against the single context with nothing set: the comparison of
    tests/test_ridgeraft_tiles_gpu.py::test_run_through_empty_tables (bit for bit on the owned rows)"""
    n = quiet["cfg"]["n_floes"]
    res = _ranks("all_four", 2)
    for listed in (False, True):
        for r, out in enumerate(res):
            o = out[listed]
            assert o["ran"] == STEPS and o["pending"] == -1, (listed, r, o["ran"], o["pending"])
            assert o["draws"] == quiet["draws"], (listed, r, o["draws"], quiet["draws"])
        _assert_ranks_equal_rows([out[listed]["snap"] for out in res], quiet["off"], n, f"list-based: {listed}")

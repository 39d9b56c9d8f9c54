"""Removal and dissolution on tiled contexts (csrc/sz_remove_tile.hpp; sz_tile_remove_floes, sz_tile_run with removal set): ranks are spawned
processes that share the one GPU and trade through gloo (backend "library-host"), as in tests/test_tiles_gpu.py.  The yardstick is the single
context -- World.run with set_removal and World.remove_floes(), held to the host rebuild by tests/test_remove_gpu.py -- and every comparison
is bit for bit: every column of capi.DCOLS and capi.TCOLS, id, status, rings and sub-floe points of a rank's floes against the single
context's rows named by the rank's gidx after the run.  The two cases are tests/remove_tiles_cases.py's, walked on the CPU by
tools/removal_tile_case.py, whose output this is:

  case A: 12 floes, 16 steps; owners for 2 ranks: [7 5], for 4: [3 4 4 1]
    owners under assign_tiles(.., 2): [1 0 0 1 0 1 0 1 0 0 0 1]
    behind step 2: 2 removed, 3 dissolved (rows [4, 5] / [6, 7, 8] of the list then); ranks that lose floes: [0, 1] of 2, [0, 1, 2] of 4; dissolving floes per rank of 2: [2 1]
    behind step 3: 2 removed, 0 dissolved (rows [0, 2] / [] of the list then); ranks that lose floes: [0, 1] of 2, [0, 1] of 4
    behind step 8: 1 removed, 0 dissolved (rows [4] / [] of the list then); ranks that lose floes: [1] of 2, [1] of 4
    4 floes stay: rows [1, 3, 9, 10] of the start; per rank [3 1] for 2 ranks, [0 0 3 1] for 4
    new numbers per rank, 2 ranks: [[0, 2, 3], [1]]
    overarea of the floes that stay: [63997997.69608748 43198513.3372283  63997997.69608748 43198513.3372283 ]
    lattice from zero: [(1, 2, 9007199254740994.0)] (2^53 + 2 = 9007199254740994.0)
    events behind steps [2, 3, 8]; 8 floes leave in all; fuse tag seen: False; longest ring: 5 points
  case B: 400 floes, 40 steps; owners for 2 ranks: [200 200], for 4: [100 100 100 100]
    behind step 0: 46 removed, 0 dissolved; ranks that lose floes: [0, 1] of 2, [0, 1, 2, 3] of 4
    behind step 1: 1 removed, 0 dissolved; ranks that lose floes: [1] of 2, [3] of 4
    behind step 3: 1 removed, 0 dissolved; ranks that lose floes: [1] of 2, [3] of 4
    behind step 5: 1 removed, 0 dissolved; ranks that lose floes: [0] of 2, [0] of 4
    behind step 6: 1 removed, 0 dissolved; ranks that lose floes: [0] of 2, [2] of 4
    behind step 10: 2 removed, 0 dissolved; ranks that lose floes: [0, 1] of 2, [0, 3] of 4
    behind step 14: 2 removed, 0 dissolved; ranks that lose floes: [1] of 2, [1] of 4
    behind step 15: 1 removed, 0 dissolved; ranks that lose floes: [1] of 2, [1] of 4
    behind step 29: 1 removed, 0 dissolved; ranks that lose floes: [0] of 2, [0] of 4
    344 floes stay; per rank [173 171] for 2 ranks, [86 85 87 86] for 4
    lattice from zero: []
    events behind steps [0, 1, 3, 5, 6, 10, 14, 15, 29]; 56 floes leave in all; fuse tag seen: False; longest ring: 17 points
"""
import datetime
import os

import numpy as np
import pytest

import remove_ref as rr
import remove_tiles_cases as cases
import remove_tiles_ref as rt
from test_remove_gpu import _assert_bit_equal, _build, _cols, _rebuild, mk
from test_tiles_gpu import _collect, _field, _free_port, _guard, _tag_cfg

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- ranks
def _rank_cols(tw):
    """the owned floes of a rank as _cols gives the single context's"""
    from subzero_jl_amd import capi
    w = tw.world
    tw.sync(); w._host_stale = True
    n = len(tw.gidx)
    c = {k: w.get(k)[:n] for k in capi.DCOLS}
    for name, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        c[name] = np.stack([w.get(pre + q)[:n] for q in ("11", "12", "21", "22")], 1)
    ids = w.ids()
    c["id"], c["ghost_id"], c["status"] = ids[0][:n], ids[1][:n], ids[2][:n]
    off, x, y = w.rings()
    c["vert_off"], c["vx"], c["vy"] = off[:n + 1].copy(), x[:off[n]].copy(), y[:off[n]].copy()
    so, sx, sy = w.subpoints()
    c["sub_off"], c["sx"], c["sy"] = so[:n + 1].copy(), sx[:so[n]].copy(), sy[:so[n]].copy()
    assert w.stats()["N"] == n == w.N
    return c


def _tiled(cfg, rank, world, dist):
    from subzero_jl_amd import tiles
    return tiles.TiledWorld(cfg, rank, world, 0, dist, host_staging=True, backend="library-host", rebox_every=3, drift_margin=3000.0)


def _snap(tw):
    return dict(gidx=np.array(tw.gidx), cols=_rank_cols(tw), lattice=tw.dissolved())


def _s_one_pass(rank, world, dist):
    cfg = cases.case_a()
    tw = _tiled(cfg, rank, world, dist)
    out = dict(ran=tw.run(3, 0, cfg["dt"], stop_on_tags=True, **cases.A_RUN))
    tw.set_removal()
    out["verdict"] = tw.remove_floes()
    out["pass"] = _snap(tw)
    out["more"] = tw.run(10, 3, cfg["dt"], stop_on_tags=True, **cases.A_RUN)
    out["later"] = _snap(tw)
    return out


def _s_batch_a(rank, world, dist):
    cfg = cases.case_a()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_removal()
    return dict(ran=tw.run(cases.A_STEPS, 0, cfg["dt"], stop_on_tags=True, **cases.A_RUN), end=_snap(tw))


def _s_batch_b(rank, world, dist, migrate=False):
    cfg = cases.case_b()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_removal()
    tw.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    if not migrate:
        return dict(ran=tw.run(cases.B_STEPS, 0, cfg["dt"], stop_on_tags=True, **cases.B_RUN), end=_snap(tw))
    half = cases.B_STEPS // 2
    ran = tw.run(half, 0, cfg["dt"], stop_on_tags=True, **cases.B_RUN)
    L = cfg["L"]
    moved = tw.migrate(owner_fn=lambda cx, cy: (cy > 0.5 * L).astype(int))
    ran += tw.run(cases.B_STEPS - half, half, cfg["dt"], stop_on_tags=True, **cases.B_RUN)
    return dict(ran=ran, moved=moved, end=_snap(tw))


def _s_batch_b_migrate(rank, world, dist):
    return _s_batch_b(rank, world, dist, True)


def _hand_cfg(rings, u):
    """a hand-made field between four open boundaries, in the style of _tag_cfg("open")"""
    from subzero_jl_amd import floe as floe_mod
    n = len(rings)
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(r) for r in rings])
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    h = np.full(n, 0.5)
    z = np.zeros((11, 11))
    return dict(n_floes=n, L=1e5, kinds=["open"] * 4, vert_off=off, vx=vx, vy=vy, height=h, u=np.array(u, float), v=np.zeros(n), xi=np.zeros(n), dt=10,
                Nx=10, Ny=10, uo=z, vo=z, hf=z, ua=z, va=z, topography=[], E=1e3, derived=floe_mod.derive(off, vx, vy, h),
                sub_off=np.zeros(n + 1, np.int32), sx=np.zeros(0), sy=np.zeros(0), seed=0)


def _decline_cfg(what):
    """(config, max_vertices).  fuse -- the pair of _tag_cfg("fuse") straddles the tile edge and is tagged on both ranks; fuse_one_rank -- the same
    closing pair 2e4 m further east, both partners rank 1's, and a square at rest on rank 0: the tag that declines is one rank's alone;
    vertices -- rank 0 holds two triangles (4 points with the closing one), rank 1 a triangle at rest and the square (5 points) that drifts into
    the east boundary, max_vertices = 4: every rank keeps a floe, so the long ring is the only reason to decline; empty -- rank 0 holds one
    square at rest, rank 1 only the square that leaves"""
    sq = lambda x0, y0, s=1e4: np.array([[x0, y0], [x0, y0 + s], [x0 + s, y0 + s], [x0 + s, y0], [x0, y0]])
    tri = lambda x0, y0, s=1e4: np.array([[x0, y0], [x0, y0 + s], [x0 + s, y0], [x0, y0]])
    if what == "fuse":
        return _tag_cfg("fuse"), 30
    if what == "fuse_one_rank":
        return _hand_cfg([sq(6.2e4, 4.5e4), sq(6.61e4, 4.6e4), sq(1.0e4, 1.0e4)], [3.0, -3.0, 0.0]), 30
    if what == "vertices":
        return _hand_cfg([tri(2.0e4, 4.5e4), sq(8.9e4 + 380.0, 2.0e4), tri(3.0e4, 1.0e4), tri(6.0e4, 7.0e4)], [0.0, 20.0, 0.0, 0.0]), 4
    return _hand_cfg([sq(2.0e4, 4.5e4), sq(8.9e4 + 380.0, 2.0e4)], [0.0, 20.0]), 30


def _s_declined(rank, world, dist, what):
    cfg, maxv = _decline_cfg(what)
    off = _tiled(cfg, rank, world, dist)
    out = dict(ran_off=off.run(12, 0, 10, coupling_on=False, stop_on_tags=True), off=_snap(off))
    tw = _tiled(cfg, rank, world, dist)
    tw.set_removal(True, max_vertices=maxv)
    tw.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 2.0))
    out["ran_on"] = tw.run(12, 0, 10, coupling_on=False, stop_on_tags=True)
    fuse = lambda t: [sorted(map(int, f)) for f in t.world.fuse()][:len(t.gidx)]
    out["on"] = _snap(tw); out["fuse_on"] = fuse(tw); out["fuse_off"] = fuse(off)
    out["verdict"] = tw.remove_floes()
    out["after"] = _snap(tw); out["fuse_after"] = fuse(tw)
    out["again"] = tw.run(1, out["ran_on"], 10, coupling_on=False, stop_on_tags=True)
    return out


def _s_declined_fuse(rank, world, dist):
    return _s_declined(rank, world, dist, "fuse")


def _s_declined_fuse_one_rank(rank, world, dist):
    return _s_declined(rank, world, dist, "fuse_one_rank")


def _s_declined_vertices(rank, world, dist):
    return _s_declined(rank, world, dist, "vertices")


def _s_declined_empty(rank, world, dist):
    return _s_declined(rank, world, dist, "empty")


NEVER = (500, 77, 6)          # test_tiles_gpu.py::_field at its smallest size, steps


def _s_never_met(rank, world, dist):
    n, seed, steps = NEVER
    cfg = _field(n, seed)
    out = {}
    for name in ("off", "on"):
        tw = _tiled(cfg, rank, world, dist)
        if name == "on":
            tw.set_removal()
        out["ran_" + name] = tw.run(steps, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True)
        out[name] = _snap(tw)
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_one_pass, _s_batch_a, _s_batch_b, _s_batch_b_migrate, _s_declined_fuse, _s_declined_fuse_one_rank, _s_declined_vertices, _s_declined_empty,
                                         _s_never_met)}


def _worker(rank, world, port, scenario, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        q.put((rank, SCENARIOS[scenario](rank, world, dist)))
    finally:
        dist.destroy_process_group()


def _run_worker(*a):
    _guard(_worker)(*a)


def _ranks(scenario, world):
    """the scenario on `world` spawned ranks: their results by rank"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_run_worker, args=(r, world, port, scenario, q)) for r in range(world)]
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


def _assert_ranks_equal_single(snaps, single, lattice, where):
    """every rank's floes are the single context's rows its gidx names, all of them exactly once; every rank's lattice is the single context's"""
    ref = _cols(single)
    seen = np.concatenate([s["gidx"] for s in snaps])
    assert sorted(seen) == list(range(single.N)), (where, sorted(seen), single.N)
    for r, s in enumerate(snaps):
        _assert_bit_equal(s["cols"], rt.take_rows(ref, s["gidx"]), f"{where}, rank {r}")
        assert np.array_equal(s["lattice"].view(np.uint8), lattice.view(np.uint8)), (where, r)


# ---------------------------------------------------------------- the single context's side of case B, once
@pytest.fixture(scope="module")
def single_b():
    """case B on the single context with removal set; and the loop it replaces, to show the case has its events: (world, lattice)"""
    cfg = cases.case_b()
    start = np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125)
    D = _build(mk(), cfg)
    D.set_removal(True); D.set_dissolved(start)
    assert D.run(cases.B_STEPS, 0, cfg["dt"], **cases.B_RUN) == cases.B_STEPS
    assert D.N == 344
    H = _build(mk(), cfg)
    H.set_dissolved(start)
    t, restarts = 0, 0
    while t < cases.B_STEPS:
        t += H.run(cases.B_STEPS - t, t, cfg["dt"], **cases.B_RUN)
        if t < cases.B_STEPS:
            assert not rr.would_decline(_cols(H), 30)
            H = _rebuild(H, cfg, None, False, False)[0]
            restarts += 1
    assert restarts >= 3 and H.N == 344
    return D, D.dissolved()


# ---------------------------------------------------------------- tests
def test_one_pass_on_two_ranks():
    """case A: 3 steps with the tag stop and removal not yet set, so the batch is behind step 2 on both ranks; then the collective pass.  Rows
    4 and 5 are removed, one per rank; rows 6, 7, 8 dissolve, two on rank 0 and one on rank 1, into the one cell [1, 2] with the masses 2^53,
    1, 1 in ascending global order: 2^53 + 2 comes out only when every rank walks the merged list in descending global number (per-rank partial
    sums give 2^53).  The 7 floes that stay carry the single context's new rows as global numbers.  10 more steps -- two more events inside them,
    behind steps 3 and 8 -- show a stale key, box or record."""
    res = _ranks("one_pass", 2)
    cfg = cases.case_a()
    D = _build(mk(), cfg)
    assert D.run(3, 0, cfg["dt"], **cases.A_RUN) == 3
    D.set_removal(True)
    ids_before = D.ids()[0]
    assert D.remove_floes() == (True, 2, 3)
    for r in res:
        assert r["ran"] == 3 and r["verdict"] == (True, 2, 3), (r["ran"], r["verdict"])
    assert sorted(np.concatenate([r["pass"]["gidx"] for r in res])) == list(range(7))
    ids = D.ids()[0]
    assert list(ids) == [int(i) for i in ids_before if i not in (5, 6, 7, 8, 9)]
    for k, r in enumerate(res):
        assert np.array_equal(ids[r["pass"]["gidx"]], r["pass"]["cols"]["id"]), k
        assert np.array_equal(np.array(cases.A_OWNERS)[r["pass"]["cols"]["id"] - 1], np.full(len(r["pass"]["gidx"]), k))
    lattice = D.dissolved()
    assert lattice[1, 2] == float(2 ** 53 + 2) and np.count_nonzero(lattice) == 1
    _assert_ranks_equal_single([r["pass"] for r in res], D, lattice, "behind the pass")
    assert D.run(10, 3, cfg["dt"], **cases.A_RUN) == 10
    assert all(r["more"] == 10 for r in res)
    assert D.N == 4
    _assert_ranks_equal_single([r["later"] for r in res], D, D.dissolved(), "10 steps behind the pass")


def test_a_tiled_batch_runs_past_removals_case_a():
    """case A in one run(16) with removal set: three passes inside the batch (behind steps 2, 3 and 8), 4 floes left -- rows 1, 3, 9, 10 of the
    start, three on rank 0 and one on rank 1 -- with the pairs (1, 9) and (3, 10) in contact throughout, the second across the tile edge"""
    res = _ranks("batch_a", 2)
    cfg = cases.case_a()
    D = _build(mk(), cfg)
    D.set_removal(True)
    assert D.run(cases.A_STEPS, 0, cfg["dt"], **cases.A_RUN) == cases.A_STEPS
    assert list(D.ids()[0]) == [2, 4, 10, 11] and np.all(D.get("overarea") > 4e7)
    assert all(r["ran"] == cases.A_STEPS for r in res)
    assert [list(r["end"]["gidx"]) for r in res] == [[0, 2, 3], [1]]
    assert sorted(np.concatenate([r["end"]["cols"]["id"] for r in res])) == [2, 4, 10, 11]
    lattice = D.dissolved()
    assert lattice[1, 2] == float(2 ** 53 + 2)
    _assert_ranks_equal_single([r["end"] for r in res], D, lattice, "case A, one batch")


@pytest.mark.parametrize("world,per_rank", [(2, [173, 171]), (4, [86, 85, 87, 86])])
def test_a_tiled_batch_runs_past_removals_case_b(single_b, world, per_rank):
    """case B in one run(40) with removal set, from a lattice of 0.125 everywhere: nine passes inside the batch, 46 floes leaving all ranks behind
    step 0, both of two / ranks 0 and 3 of four losing floes behind step 10; 344 floes stay"""
    D, lattice = single_b
    res = _ranks("batch_b", world)
    assert all(r["ran"] == cases.B_STEPS for r in res)
    assert [len(r["end"]["gidx"]) for r in res] == per_rank
    _assert_ranks_equal_single([r["end"] for r in res], D, lattice, f"case B, {world} ranks")


def test_migration_behind_removals(single_b):
    """case B on 2 ranks: run(20), a migration to a split along y, run(20).  The migration orders the new tiles by the global numbers the passes
    of the first half left (tile_gidx), and the passes of the second half renumber what it made"""
    D, lattice = single_b
    res = _ranks("batch_b_migrate", 2)
    assert all(r["ran"] == cases.B_STEPS and r["moved"] > 0 for r in res)
    _assert_ranks_equal_single([r["end"] for r in res], D, lattice, "case B with a migration half way")


@pytest.mark.parametrize("what", ["fuse", "fuse_one_rank", "vertices", "empty"])
def test_declined_agreed_unchanged(what):
    """What declines the pass holds on ONE rank (fuse_one_rank: both fused floes are rank 1's; vertices: the ring over max_vertices = 4 is rank
    1's, and both ranks keep floes; empty: rank 1 alone would be left without a floe) or on both (fuse: the pair straddles the edge): the batch
    with removal set ends where it ends without, with the same steps_done on both ranks and the same state; remove_floes() is declined on both
    ranks and changes nothing; one more step runs."""
    res = _ranks("declined_" + what, 2)
    cfg, maxv = _decline_cfg(what)
    cols = [r["off"]["cols"] for r in res]
    n_over = [int(np.count_nonzero(np.diff(c["vert_off"]) > maxv)) for c in cols]
    n_fuse = [int(np.count_nonzero(c["status"] == rr.FUSE)) for c in cols]
    n_remove = [int(np.count_nonzero(c["status"] == rr.REMOVE)) for c in cols]
    stay = [int(np.count_nonzero(c["status"] != rr.REMOVE)) for c in cols]
    assert all(np.all(c["area"] >= 1e6) and np.all(c["height"] >= 0.1) for c in cols)          # nothing dissolves
    if what == "vertices":          # the long ring, and nothing else
        assert n_over == [0, 1] and n_fuse == [0, 0] and n_remove == [0, 1] and stay == [2, 1]
    elif what == "empty":
        assert n_over == [0, 0] and n_fuse == [0, 0] and n_remove == [0, 1] and stay == [1, 0]
    elif what == "fuse_one_rank":
        assert n_over == [0, 0] and n_fuse == [0, 2] and n_remove == [0, 0] and stay == [1, 2]
    else:
        assert n_over == [0, 0] and n_fuse == [1, 1] and n_remove == [0, 0] and min(stay) > 0
    assert res[0]["ran_off"] == res[1]["ran_off"] and 2 <= res[0]["ran_off"] < 12
    for k, r in enumerate(res):
        assert r["ran_on"] == r["ran_off"], (k, r["ran_on"], r["ran_off"])
        assert np.array_equal(r["on"]["gidx"], r["off"]["gidx"]) and r["fuse_on"] == r["fuse_off"]
        _assert_bit_equal(r["on"]["cols"], r["off"]["cols"], f"{what}: the batch with removal set, rank {k}")
        assert r["verdict"] == (False, 0, 0), (k, r["verdict"])
        assert np.array_equal(r["after"]["gidx"], r["on"]["gidx"]) and r["fuse_after"] == r["fuse_on"]
        _assert_bit_equal(r["after"]["cols"], r["on"]["cols"], f"{what}: declined, rank {k}")
        assert np.all(r["after"]["lattice"] == 2.0)
        assert r["again"] == 1


def test_never_met_does_not_perturb_a_tiled_run():
    """the periodic two-rank field of test_tiles_gpu.py at its smallest size: removal set and never met is removal off, bit for bit"""
    res = _ranks("never_met", 2)
    for k, r in enumerate(res):
        assert r["ran_on"] == r["ran_off"] == NEVER[2], (k, r["ran_on"], r["ran_off"])
        assert np.array_equal(r["on"]["gidx"], r["off"]["gidx"])
        _assert_bit_equal(r["on"]["cols"], r["off"]["cols"], f"rank {k}")

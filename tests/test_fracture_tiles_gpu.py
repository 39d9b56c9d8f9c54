"""Fracture criteria on tiled contexts (csrc/sz_fracture_tile.hpp; sz_tile_fracture_candidates, sz_tile_run with a criterion set): ranks are
spawned processes that share the one GPU and trade through gloo (backend "library-host"), as in tests/test_remove_tiles_gpu.py.  The
yardstick is the single context -- World with set_fracture, held to the reference by tests/test_fracture_gpu.py -- and every comparison is
bit for bit: both sides run the same expressions on the same bits, so there is no tolerance and no tie exclusion."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

import fracture_ref as fr
import fracture_tiles_ref as ft
import remove_tiles_cases as cases
import remove_tiles_ref as rt
from test_fracture_gpu import CRITERIA, _cfg, _pick_pstar
from test_remove_gpu import _assert_bit_equal, _build, _cols, mk
from test_remove_tiles_gpu import _rank_cols, _tiled
from test_tiles_gpu import _collect, _free_port, _guard

pytestmark = pytest.mark.gpu

E_STATE = -4
ALPHAS = (0.0, 0.5)
SA = ("sa11", "sa12", "sa21", "sa22")
NEVER_STEPS = 24
B_FRAC_DT, B_TSTEP0 = 11, 1          # case B from tstep 1 with Δt = 11: the only fracture step of the batch is its step 10 (tstep 11)


def _crit_args(crit, alpha=0.0, dt=5):
    return dict(kind=crit["kind"], dt=dt, pstar=crit.get("pstar", 2.25e5), c=crit.get("c", 20.0), poly=crit.get("poly"), alpha=alpha, min_floe_area=1e6)


def _bits(x):
    return np.array(x, np.float64).view(np.uint64).tolist()


# ---------------------------------------------------------------- ranks
def _snap(tw, lattice=False):
    out = dict(gidx=np.array(tw.gidx), cols=_rank_cols(tw))
    if lattice:
        out["lattice"] = tw.dissolved()
    return out


def _retile(tw, gidx=None):
    """the tiling again behind an upload (as TiledWorld.repartition does); gidx: other global numbers than the rank's own"""
    from subzero_jl_amd import capi, tiles
    w = tw.world
    w._push()
    g = np.ascontiguousarray(tw.gidx if gidx is None else gidx, np.int64)
    w._chk(w.L.sz_tile_enable(w.h, capi.ptr(g, capi._lp), tw._max_ring, tw._max_rmax))
    w._chk(w.L.sz_tile_setup(w.h, tw.L, tw.L, int(tw.per_x), int(tw.per_y), float(tw.margin), int(tw._rebox_arg)))
    px, py = tiles.tile_grid(tw.nranks)
    w._chk(w.L.sz_tile_set_center(w.h, (tw.rank % px + 0.5) * tw.L / px, (tw.rank // px + 0.5) * tw.L / py))


def _s_one_pass(rank, world, dist):
    cfg, sa, area, h = ft.one_pass_case()
    tw = _tiled(cfg, rank, world, dist)
    w, g = tw.world, tw.gidx
    w.set("area", area[g]); w.set("height", h[g])
    for k, name in enumerate(SA):
        w.set(name, sa[g, k])
    _retile(tw)
    out = []
    for _, crit in CRITERIA:
        for alpha in ALPHAS:
            tw.set_fracture(**_crit_args(crit, alpha))
            got = tw.fracture_candidates(); mean = tw.fracture_mean()
            out.append(dict(cand=got, mean=_bits(mean), again=tw.fracture_candidates(), mean_again=_bits(tw.fracture_mean())))
    return dict(n_owned=len(g), passes=out)


def _stopping_run(tw, cfg, pstar):
    from subzero_jl_amd import capi
    tw.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=pstar, min_floe_area=1e6)
    return tw.run(40, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True)


def _s_stops(rank, world, dist, pstar):
    cfg = _cfg()
    tw = _tiled(cfg, rank, world, dist)
    out = dict(done=_stopping_run(tw, cfg, pstar))
    out["cand"] = tw.fracture_candidates(); out["stop"] = _snap(tw)
    out["more"] = tw.run(40 - out["done"], out["done"], cfg["dt"], coupling_dt=1, stop_on_tags=False)
    out["end"] = _snap(tw)
    return out


def _s_cut(rank, world, dist, pstar, tfirst):
    """the first candidate's step as the last step of a sz_tile_run call, then as the first step of the next one"""
    cfg = _cfg()
    out = {}
    for name, every in (("last", tfirst + 1), ("first", tfirst)):
        tw = _tiled(cfg, rank, world, dist)
        tw.repartition_every = every
        out[name] = _stopping_run(tw, cfg, pstar)
        out[name + "_cand"] = tw.fracture_candidates()
    return out


def _s_never_and_through(rank, world, dist):
    from subzero_jl_amd import capi
    cfg = _cfg(seed=78)
    out = {}
    for name, stop, crit in (("off", True, None), ("never", True, dict(kind=capi.FRAC_POLYGON, dt=5, poly=fr.huge_square(), min_floe_area=1e6)),
                             ("off2", False, None), ("met", False, dict(kind=capi.FRAC_HIBLER, dt=5, pstar=1.0, min_floe_area=1e6))):
        tw = _tiled(cfg, rank, world, dist)
        if crit:
            tw.set_fracture(**crit)
        out["ran_" + name] = tw.run(NEVER_STEPS, 0, cfg["dt"], coupling_dt=1, stop_on_tags=stop)
        out[name] = _snap(tw)
        if crit:
            out["cand_" + name] = tw.fracture_candidates()
    return out


def _b_world(make, never):
    from subzero_jl_amd import capi
    cfg = cases.case_b()
    w = make(cfg)
    w.set_removal(True)
    w.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    if never:
        w.set_fracture(capi.FRAC_POLYGON, dt=5, poly=fr.huge_square(), min_floe_area=1e6)
        return w, w.run(cases.B_STEPS, 0, cfg["dt"], stop_on_tags=True, **cases.B_RUN)
    w.set_fracture(capi.FRAC_HIBLER, dt=B_FRAC_DT, pstar=1.0, min_floe_area=1e6)
    return w, w.run(cases.B_STEPS, B_TSTEP0, cfg["dt"], stop_on_tags=True, **cases.B_RUN)


def _s_with_removal(rank, world, dist):
    out = {}
    for name, never in (("never", True), ("met", False)):
        tw, ran = _b_world(lambda cfg: _tiled(cfg, rank, world, dist), never)
        out[name] = dict(ran=ran, end=_snap(tw, lattice=True), cand=tw.fracture_candidates())
    return out


LISTED = dict(n=500, seed=81, steps=12, tstep0=1)          # Δt = 5 from tstep 1: the batch is cut behind its step 4 (tstep 5) and step 9 (tstep 10)
LISTED_RUN = dict(coupling_dt=1, collisions_on=False)       # collisions off: sz_tile_run takes its list-based driver


def _off_origin_square():
    """a fixed criterion polygon that does not cover the unstressed floes' σ-point (0, 0): every floe over min_floe_area is a candidate"""
    return np.array([1e3, 2e3, 2e3, 1e3, 1e3]), np.array([1e3, 1e3, 2e3, 2e3, 1e3])


def _listed_runs(make):
    """name -> (steps run, world) for: criterion off, never met, met on the first fracture step"""
    from subzero_jl_amd import capi
    cfg = _cfg(n=LISTED["n"], seed=LISTED["seed"])
    out = {}
    for name, poly in (("off", None), ("never", fr.huge_square()), ("met", _off_origin_square())):
        w = make(cfg)
        if poly is not None:
            w.set_fracture(capi.FRAC_POLYGON, dt=5, poly=poly, min_floe_area=1e6)
        out[name] = (w.run(LISTED["steps"], LISTED["tstep0"], cfg["dt"], stop_on_tags=True, **LISTED_RUN), w)
    return out


def _s_listed(rank, world, dist):
    out = {}
    for name, (ran, tw) in _listed_runs(lambda cfg: _tiled(cfg, rank, world, dist)).items():
        out[name] = dict(ran=ran, end=_snap(tw), cand=tw.fracture_candidates() if name != "off" else None)
    return out


def _s_duplicate(rank, world, dist):
    """rank 1 holds its first global number twice (and its second not at all): every rank returns the same error, none waits for another"""
    from subzero_jl_amd import capi
    cfg = cases.case_b()
    tw = _tiled(cfg, rank, world, dist)
    g = np.array(tw.gidx)
    if rank == 1:
        g[1] = g[0]
    _retile(tw, g)
    tw.set_fracture(capi.FRAC_HIBLER, dt=5)
    w = tw.world
    ng, no = C.c_int32(0), C.c_int32(0)
    rc = w.L.sz_tile_fracture_candidates(w.h, C.byref(ng), C.byref(no), None, None)
    msg = w.L.sz_last_error(w.h).decode()
    try:
        tw.fracture_candidates()
        raised = False
    except capi.SzError:
        raised = True
    return dict(rc=rc, msg=msg, raised=raised, n=ng.value)


SCENARIOS = {f.__name__[3:]: f for f in (_s_one_pass, _s_stops, _s_cut, _s_never_and_through, _s_with_removal, _s_listed, _s_duplicate)}


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


def fields_world(cfg):
    from subzero_jl_amd import fields
    return fields.build_world(mk(), cfg)


def _assert_ranks_equal_rows(snaps, ref, n, where):
    """every rank's floes are the rows of `ref` (the single context's columns) its gidx names, all n of them exactly once"""
    seen = np.concatenate([s["gidx"] for s in snaps])
    assert sorted(seen) == list(range(n)), (where, len(seen), n)
    for r, s in enumerate(snaps):
        _assert_bit_equal(s["cols"], rt.take_rows(ref, s["gidx"]), f"{where}, rank {r}")


# ---------------------------------------------------------------- the single context's side, once each
@pytest.fixture(scope="module")
def single_stop():
    """the 2 000-floe field of test_fracture_gpu.py::test_batch_stops_where_the_reference_fractures on the single context"""
    from subzero_jl_amd import capi, fields
    cfg = _cfg()
    pstar, tfirst = _pick_pstar(cfg)
    hw = fields.build_world(mk(), cfg)
    hw.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=pstar, min_floe_area=1e6)
    done = hw.run(40, 0, cfg["dt"], coupling_dt=1)
    assert done == tfirst + 1 and tfirst % 5 == 0 and 0 < done < 40
    cand = hw.fracture_candidates()
    assert len(cand) > 0
    stop = _cols(hw)
    assert hw.run(40 - done, done, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 40 - done
    return dict(pstar=pstar, tfirst=tfirst, done=done, cand=cand, stop=stop, end=_cols(hw), n=hw.N)


@pytest.fixture(scope="module")
def single_one_pass():
    from subzero_jl_amd import fields
    cfg, sa, area, h = ft.one_pass_case()
    hw = fields.build_world(mk(), cfg)
    hw.set("area", area); hw.set("height", h)
    for k, name in enumerate(SA):
        hw.set(name, sa[:, k])
    out = []
    for _, crit in CRITERIA:
        for alpha in ALPHAS:
            hw.set_fracture(**_crit_args(crit, alpha))
            out.append(dict(cand=hw.fracture_candidates(), mean=_bits(hw.fracture_mean())))
    return out, h, cfg


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("world", [2, 4])
def test_one_pass_is_the_single_contexts(single_one_pass, world):
    """1 500 floes (threads of the criterion kernel sum two rows), the ranks' rows interleaved in global order, three criteria x two α: the
    candidates and the mean height / p of every rank are the single context's, the means as bits -- which per-rank sums added over the ranks
    would not give on this field (tests/test_fracture_tiles_cpu.py)"""
    want, h, cfg = single_one_pass
    res = _ranks("one_pass", world)
    assert sum(r["n_owned"] for r in res) == ft.ONE_PASS_N and min(r["n_owned"] for r in res) > 0
    for nr in (2, 4):
        assert ft.reduced_mean(h, ft.one_pass_owners(cfg, nr), nr) != ft.kernel_mean(h)
    k = 0
    for name, crit in CRITERIA:
        for alpha in ALPHAS:
            w = want[k]
            assert 0 < len(w["cand"]) < ft.ONE_PASS_N, (name, alpha, len(w["cand"]))
            if crit["kind"] == 1:
                assert w["mean"][0] == _bits(ft.kernel_mean(h))
            for r, out in enumerate(res):
                got = out["passes"][k]
                assert got["cand"].dtype.kind == "i" and np.array_equal(got["cand"], w["cand"]), (name, alpha, r)
                assert got["mean"] == w["mean"], (name, alpha, r, got["mean"], w["mean"])
                assert np.array_equal(got["again"], got["cand"]) and got["mean_again"] == got["mean"], (name, alpha, r)
            k += 1


@pytest.mark.parametrize("world", [2, 4])
def test_a_tiled_batch_stops_where_the_single_context_fractures(single_stop, world):
    s = single_stop
    res = _ranks("stops", world, s["pstar"])
    for r, out in enumerate(res):
        assert out["done"] == s["done"], (r, out["done"], s["done"])
        assert np.array_equal(out["cand"], s["cand"]), r
        assert out["more"] == 40 - s["done"], r
    _assert_ranks_equal_rows([o["stop"] for o in res], s["stop"], s["n"], f"at the stop, {world} ranks")
    _assert_ranks_equal_rows([o["end"] for o in res], s["end"], s["n"], f"at the end, {world} ranks")


def test_cut_batches_stop_on_the_same_step(single_stop):
    s = single_stop
    res = _ranks("cut", 2, s["pstar"], s["tfirst"])
    for r, out in enumerate(res):
        assert out["last"] == s["done"] and out["first"] == s["done"], (r, out["last"], out["first"], s["done"])
        assert np.array_equal(out["last_cand"], s["cand"]) and np.array_equal(out["first_cand"], s["cand"]), r


def test_never_met_and_run_through_do_not_perturb_a_tiled_run():
    """a criterion that is never met runs all steps bit-equal to the same tiled run with the criterion off; so does a batch that runs through
    (stop_on_tags=False) with a criterion that is met, and the candidates are there afterwards"""
    res = _ranks("never_and_through", 2)
    for r, out in enumerate(res):
        assert [out["ran_" + k] for k in ("off", "never", "off2", "met")] == [NEVER_STEPS] * 4, r
        assert np.array_equal(out["never"]["gidx"], out["off"]["gidx"]) and np.array_equal(out["met"]["gidx"], out["off2"]["gidx"])
        _assert_bit_equal(out["never"]["cols"], out["off"]["cols"], f"never met, rank {r}")
        _assert_bit_equal(out["met"]["cols"], out["off2"]["cols"], f"run through, rank {r}")
        assert len(out["cand_never"]) == 0 and len(out["cand_met"]) > 0


def test_with_removal_in_the_single_contexts_order():
    """case B (leavers behind steps 0, 1, 3, 5, 6, 10, 14, 15, 29) with removal set, on 2 ranks.  A never-met criterion with Δt = 5: the tags of
    steps 0, 5, 10 and 15 are raised on a segment's last step, known to their rank alone until the pass's agreement -- everything is the
    single context's, the lattice included.  A criterion met on step 10: not with Δt = 5 and a pstar first met there (case B's floes are
    stressed from step 0 on; a pstar that holds at steps 0 and 5 and fails at 10 clear of ties was not searched for) but with Δt = 11 from tstep 1 and
    pstar = 1, so that the batch's step 10 (tstep 11) is its only fracture step and surely has candidates.  No fracture segment without a
    candidate comes before the stop here -- the never-met half and the stopping tests have those.  Fracture comes before simplify: both sides end
    behind step 10 with the floes of that step's tag still there"""
    res = _ranks("with_removal", 2)
    for name, never in (("never", True), ("met", False)):
        D, ran = _b_world(lambda cfg: _build(mk(), cfg), never)
        assert ran == (cases.B_STEPS if never else 11), (name, ran)
        ref, lattice, cand = _cols(D), D.dissolved(), D.fracture_candidates()
        if never:
            assert D.N == 344 and len(cand) == 0
        else:
            assert len(cand) > 0 and np.count_nonzero(ref["status"] == 2) > 0          # (REMOVE: step 10's leavers, not yet removed)
        for r, out in enumerate(res):
            assert out[name]["ran"] == ran, (name, r, out[name]["ran"], ran)
            assert np.array_equal(out[name]["cand"], cand), (name, r)
            assert np.array_equal(out[name]["end"]["lattice"].view(np.uint8), lattice.view(np.uint8)), (name, r)
        _assert_ranks_equal_rows([o[name]["end"] for o in res], ref, D.N, f"case B, {name}")


def test_the_list_based_driver_cuts_and_stops_too():
    """collisions off, so sz_tile_run takes its list-based steps (the driver of rings over 20 points and of fields without a static grid): with
    a criterion never met the 12 steps -- cut behind two fracture steps, a pass behind each -- are the criterion off and the single context, bit
    for bit; with a polygon that leaves (0, 0) uncovered the batch ends behind its first fracture step, tstep 5, where World.run ends"""
    res = _ranks("listed", 2)
    single = _listed_runs(lambda cfg: fields_world(cfg))
    assert single["off"][0] == single["never"][0] == LISTED["steps"] and single["met"][0] == 5
    for name in ("never", "met"):
        ran, D = single[name]
        cand, ref = D.fracture_candidates(), _cols(D)
        assert (len(cand) == 0) if name == "never" else (0 < len(cand) <= D.N)
        for r, out in enumerate(res):
            assert out[name]["ran"] == ran, (name, r, out[name]["ran"], ran)
            assert np.array_equal(out[name]["cand"], cand), (name, r)
        _assert_ranks_equal_rows([o[name]["end"] for o in res], ref, D.N, f"list-based driver, {name}")
    for r, out in enumerate(res):
        assert out["off"]["ran"] == LISTED["steps"]
        _assert_bit_equal(out["never"]["end"]["cols"], out["off"]["end"]["cols"], f"list-based driver, never met against off, rank {r}")


def test_one_forced_tiled_rank_stops_where_the_single_context_stops(single_stop):
    from subzero_jl_amd import tiles
    s = single_stop
    cfg = _cfg()
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    assert _stopping_run(tw, cfg, s["pstar"]) == s["done"]
    assert np.array_equal(tw.fracture_candidates(), s["cand"])
    _assert_ranks_equal_rows([_snap(tw)], s["stop"], s["n"], "one rank")


def test_refusals_that_stay():
    from subzero_jl_amd import capi, tiles
    cfg = cases.case_b()
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    tw.set_fracture(capi.FRAC_HIBLER, dt=5)
    w = tw.world
    assert w.L.sz_tile_step(w.h, None, 1, 0, 0, cfg["dt"], 1, capi.COLLISIONS_ON) == E_STATE
    assert b"sz_tile_step" in w.L.sz_last_error(w.h)
    done = C.c_int32(0)
    assert w.L.sz_tile_run(w.h, 4, 0, cfg["dt"], 1, capi.COLLISIONS_ON, C.byref(done)) == 0 and done.value == 1          # (case B tags floes on step 0)
    w.set_two_way(True, dt=cfg["dt"])
    for flags in (capi.COLLISIONS_ON, capi.COLLISIONS_ON | capi.NO_STOP):
        assert w.L.sz_tile_run(w.h, 4, 1, cfg["dt"], 1, flags, C.byref(done)) == E_STATE
        assert b"two-way" in w.L.sz_last_error(w.h) and b"fracture" in w.L.sz_last_error(w.h)
    tw.backend = "torch"          # (the host-driven steps: no library channel)
    with pytest.raises(capi.SzError):
        tw.set_fracture(capi.FRAC_HIBLER, dt=5)


def test_a_duplicated_global_number_is_the_same_error_on_every_rank():
    res = _ranks("duplicate", 2)
    for r, out in enumerate(res):
        assert out["rc"] == E_STATE and out["raised"] and out["n"] == 0, (r, out["rc"], out["raised"])
        assert "held twice" in out["msg"], (r, out["msg"])
    assert res[0]["msg"] == res[1]["msg"]

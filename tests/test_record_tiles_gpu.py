"""Output frames of tiled runs (csrc/sz_record_tile.hpp, tile_record; DESIGN.md §9i, "Tiled contexts"): ranks are spawned processes that share the
one GPU and trade through gloo (backend "library-host"), as in tests/test_tiles_gpu.py.  The yardstick is the single context's recorder (held to
the hand cut by tests/test_record_gpu.py) on the 300-floe fields of that file; the merge is also held to tests/record_tiles_ref.py.  Floe frames
and states are compared bit for bit.  Grid frames are sums over the ranks: against the single context they are held to 1e-11 x each output's
scale, the bound tests/test_tiles_gpu.py holds the existing tiled averages to; at two ranks they are bit-equal to TiledWorld.write_grid_data of
the same run cut by hand (a two-term sum does not depend on the all-reduce's order).  Measured on the MI355X: the largest grid error over its
scale is 5.8e-16 (periodic, 2 ranks), 7.2e-16 (periodic, 4 ranks), 6.4e-16 (walls, 2 and 4 ranks)."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

import record_tiles_ref as rec
import remove_tiles_cases as cases
from test_record_gpu import KINDS, THREE, _cfg, _grid, _same, _world, mk
from test_remove_gpu import _assert_bit_equal, _build
from test_remove_tiles_gpu import _assert_ranks_equal_single, _snap, _tiled
from test_tiles_gpu import _collect, _free_port, _guard

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -4
RUN = dict(coupling_dt=1, stop_on_tags=True)
OUT5, OUT7 = (5, 10, 15, 20, 25), (7, 14, 21)
RM_COLUMNS = ["cx", "id", "status", "rings"]


def _grids(cfg):
    return _grid(cfg, 10, 7), _grid(cfg, 12, 12)


def _set_three_writers(w, cfg):
    g1, g2 = _grids(cfg)
    w.set_floe_output(0, 5)
    w.set_grid_output(0, 5, *g1)
    w.set_grid_output(2, 7, *g2, outputs=THREE)


def _frames(tw, writer=0, local=True):
    """every floe frame of a writer: merged (collective), and this rank's own"""
    n = tw.output_frames()[0][writer]
    return [tw.floe_frame(writer, k) for k in range(n)], [tw.floe_frame_local(writer, k) for k in range(n)] if local else None


def _tsteps(tw, writer=0):
    return [tw.world.floe_frame(writer, k, members=[])["tstep"] for k in range(tw.output_frames()[0][writer])]


# ---------------------------------------------------------------- ranks
def _s_recorded(rank, world, dist, kind):
    cfg = _cfg(kind)
    dt = cfg["dt"]
    g1, g2 = _grids(cfg)
    tw = _tiled(cfg, rank, world, dist)
    _set_three_writers(tw, cfg)
    out = dict(gidx=np.array(tw.gidx), ran=tw.run(24, 3, dt, **RUN), frames=tw.output_frames())
    out["merged"], out["local"] = _frames(tw)
    out["grid0"] = [tw.grid_frame(0, k) for k in range(out["frames"][1][0])]
    out["grid2"] = [tw.grid_frame(2, k) for k in range(out["frames"][1][2])]
    out["end"] = _snap(tw)
    if world == 2:          # the same run cut by hand in the same rank processes
        h = _tiled(cfg, rank, world, dist)
        t, out["hand0"], out["hand2"] = 3, [], []
        for s in sorted(set(OUT5 + OUT7)):
            assert h.run(s - t, t, dt, **RUN) == s - t
            t = s
            if s % 5 == 0:
                out["hand0"].append(h.write_grid_data(*g1))
            if s % 7 == 0:
                out["hand2"].append(h.write_grid_data(*g2, THREE))
    return out


def _s_hand_cut(rank, world, dist):
    """recorded (R), cut by hand at every output step (H) and with no writer (P); R and P in the same calls, which end at 10, 20 and 27"""
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    g1 = _grids(cfg)[0]
    R, H, P = (_tiled(cfg, rank, world, dist) for _ in range(3))
    R.set_floe_output(0, 5); R.set_grid_output(0, 5, *g1)
    out = dict(R=[], H=[], P=[])
    t = 3
    for end in (10, 20, 27):
        assert R.run(end - t, t, dt, **RUN) == end - t and P.run(end - t, t, dt, **RUN) == end - t
        th = t
        for s in [u for u in OUT5 if th <= u < end] + [end]:          # (the cut at a call's end step is made where the next call begins the step)
            assert H.run(s - th, th, dt, **RUN) == s - th
            th = s
            if s % 5 == 0 and s < end:
                H.write_grid_data(*g1)          # add_ghosts, the partial sums, remove_ghosts
        t = end
        for name, w in (("R", R), ("H", H), ("P", P)):
            out[name].append(_snap(w))
    out["tsteps"] = _tsteps(R)
    return out


def _s_ends(rank, world, dist):
    from subzero_jl_amd import capi
    from test_fracture_tiles_gpu import _retile
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    out = {}
    # tagged before: the batch ends after its first step
    tw = _tiled(cfg, rank, world, dist)
    tw.set_floe_output(0, 5, ["cx", "id"])
    st = np.full(len(tw.gidx), capi.ACTIVE, np.int32); st[tw.gidx == 17] = capi.FUSE
    tw.world.set_status(st)
    _retile(tw)          # (an upload and the tiling again: the writer stays)
    out["tagged"] = [(tw.run(8, 4, dt, **RUN), _tsteps(tw)), (tw.run(8, 5, dt, **RUN), _tsteps(tw))]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_floe_output(1, 5, ["cx", "id"])
    out["calls"] = [(tw.run(5, 0, dt, **RUN), _tsteps(tw, 1)), (tw.run(5, 5, dt, **RUN), _tsteps(tw, 1))]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_floe_output(0, 5, ["cx", "id"])
    out["through"] = (tw.run(12, 0, dt, coupling_dt=1, stop_on_tags=False), _tsteps(tw))
    # full: room for two frames on rank 0 only
    p = _tiled(cfg, rank, world, dist)
    p.set_floe_output(0, 3)
    out["room"] = (p.run(12, 0, dt, **RUN), _tsteps(p))
    mask = p.world.frame_mask(None)
    sizes = []
    for k in range(2):
        fr = p.floe_frame_local(0, k, members=[])
        V = C.c_int64(0)
        assert p.world.L.sz_floe_frame_info(p.world.h, 0, k, None, None, None, C.byref(V), None) == 0
        sizes.append(p.world.frame_bytes(mask, fr["M"], fr["N"], int(V.value)) + 8 * fr["M"])
    q = _tiled(cfg, rank, world, dist)
    q.set_floe_output(0, 3, arena_bytes=sizes[0] + sizes[1] if rank == 0 else 1 << 26)
    out["full"] = (q.run(12, 0, dt, **RUN), _tsteps(q), q.output_frames()[2])
    out["full_merged"] = _frames(q, local=False)[0]; out["room_merged"] = _frames(p, local=False)[0][:2]
    q.clear_frames()
    out["cleared"] = q.output_frames()
    out["rest"] = (q.run(6, 6, dt, **RUN), _tsteps(q), q.output_frames()[2])
    out["q"], out["p"] = _snap(q), _snap(p)
    return out


def _s_removal(rank, world, dist):
    cfg = cases.case_b()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_removal()
    tw.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    tw.set_floe_output(0, 5, RM_COLUMNS)
    out = dict(ran=tw.run(cases.B_STEPS, 0, cfg["dt"], stop_on_tags=True, **cases.B_RUN))
    out["merged"], out["local"] = _frames(tw)
    out["end"] = _snap(tw)
    return out


def _s_pending(rank, world, dist):
    from test_ridgeraft_gpu import _dense
    cfg = _dense()
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_ridgeraft(True, dt=10)
    tw.set_floe_output(0, 10)
    out = dict(ran=tw.run(40, 1, dt, **RUN), pending=tw.ridgeraft_pending(), tsteps=_tsteps(tw))
    out["merged"] = _frames(tw, local=False)[0]
    tw.finish_step(10, dt, coupling_dt=1)
    out["more"] = tw.run(5, 11, dt, **RUN)
    out["tsteps_after"] = _tsteps(tw)
    return out


def _s_migration(rank, world, dist):
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    L = cfg["L"]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_floe_output(0, 5)
    out = dict(first=tw.run(10, 0, dt, **RUN), gidx_before=np.array(tw.gidx))
    out["before"] = tw.floe_frame(0, 1)          # (merged before the migration, and again behind it)
    out["moved"] = tw.migrate(owner_fn=lambda cx, cy: (cy > 0.5 * L).astype(int))
    out["second"] = tw.run(10, 10, dt, **RUN)
    out["merged"], out["local"] = _frames(tw)
    out["gidx_after"] = np.array(tw.gidx)
    out["end"] = _snap(tw)
    return out


def _launches(w):
    return {k: v[1] for k, v in w.kernel_times().items()}


def _s_refuse(rank, world, dist):
    from subzero_jl_amd import capi
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    g = _grids(cfg)[0]
    xg, yg = (np.ascontiguousarray(a) for a in g)
    codes = np.array([0, 5], np.int32)
    tw = _tiled(cfg, rank, world, dist)
    w = tw.world
    L, h = w.L, w.h
    out = dict(bad=[])
    for writer, dto in ((4, 5), (-1, 5), (0, -1)):
        out["bad"].append(L.sz_tile_set_floe_output(h, writer, dto, 1, 1 << 20))
        out["bad"].append(L.sz_tile_set_grid_output(h, writer, dto, 10, 7, capi.ptr(xg), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4))
    uneven = np.array([0.0, 1.0, 3.0])
    out["bad"].append(L.sz_tile_set_grid_output(h, 0, 5, 2, 7, capi.ptr(uneven), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4))
    out["bad"].append(L.sz_tile_set_floe_output(h, 0, 5, 1 << 33, 1 << 20))
    out["bad"].append(L.sz_tile_set_floe_output(h, 0, 5, 0, 1 << 20))
    out["single_setters"] = (L.sz_set_floe_output(h, 0, 5, 1, 1 << 20), L.sz_set_grid_output(h, 0, 5, 10, 7, capi.ptr(xg), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4))
    # the ranks disagree on an interval
    before = _snap(tw)
    tw.set_floe_output(0, 5 if rank == 0 else 7, ["cx"])
    flags = capi.COLLISIONS_ON | capi.COUPLING_ON
    done = C.c_int32(7)
    out["differ"] = (L.sz_tile_run(h, 8, 0, dt, 1, flags, C.byref(done)), done.value, L.sz_last_error(h).decode())
    out["differ_unchanged"] = (before, _snap(tw))
    # sz_step with a tile writer set
    tw.set_floe_output(0, 5, ["cx"])
    done = C.c_int32(7)
    out["step"] = (L.sz_step(h, 3, 0, dt, 1, flags, C.byref(done)), done.value, L.sz_last_error(h).decode())
    out["then"] = (tw.run(6, 0, dt, **RUN), _tsteps(tw))
    # two-way coupling with a tile writer set
    t2 = _tiled(cfg, rank, world, dist)
    t2.set_two_way(0.5, -8.0, dt)
    t2.set_floe_output(0, 5, ["cx"])
    done = C.c_int32(7)
    out["two_way"] = (t2.world.L.sz_tile_run(t2.world.h, 8, 0, dt, 1, flags, C.byref(done)), done.value)
    # set and turned off again: the launches and the bits of a fresh tiled world
    for name, setup in (("fresh", lambda t: None),
                        ("off", lambda t: (_set_three_writers(t, cfg), t.set_floe_output(0, 0), t.set_grid_output(0, 0), t.set_grid_output(2, 0)))):
        t3 = _tiled(cfg, rank, world, dist)
        setup(t3)
        t3.world.profile(True)
        ran = t3.run(12, 0, dt, **RUN)
        t3.sync()
        out[name] = dict(ran=ran, launches=_launches(t3.world), snap=_snap(t3), frames=t3.output_frames())
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_recorded, _s_hand_cut, _s_ends, _s_removal, _s_pending, _s_migration, _s_refuse)}


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
        for p in procs:
            if p.is_alive():
                p.terminate()
    return [out for _, out in sorted(res, key=lambda r: r[0])]


# ---------------------------------------------------------------- the single context's side, once per field
@pytest.fixture(scope="module", params=list(KINDS))
def single_recorded(request):
    """the single context's recorded run(24, 3) with the three writers of the tiled runs, and a fourth that records every output on the second
    grid: the scales of the bound on its stress group"""
    kind = request.param
    cfg = _cfg(kind)
    A = _world(cfg)
    _set_three_writers(A, cfg)
    A.set_grid_output(1, 7, *_grids(cfg)[1])
    assert A.run(24, 3, cfg["dt"], coupling_dt=1, stop_on_tags=True) == 24
    nf, ng, full = A.output_frames()
    assert nf == [5, 0, 0, 0] and ng == [5, 3, 3, 0] and not full
    return dict(kind=kind, cfg=cfg, world=A, floe=[A.floe_frame(0, k) for k in range(5)], grid0=[A.grid_frame(0, k) for k in range(5)],
                grid2=[A.grid_frame(2, k) for k in range(3)], all2=[A.grid_frame(1, k)[1] for k in range(3)])


def _scales(names, full, all_names):
    """per output of `names` the scale of tests/test_tiles_gpu.py's bound: its own largest value, for a stress or strain output its tensor group's"""
    out = []
    for n in names:
        grp = [j for j, o in enumerate(all_names) if o.split("_")[0] == n.split("_")[0]] if n.startswith(("stress", "strain")) else [all_names.index(n)]
        out.append(max(np.abs(full[j]).max() for j in grp))
    return out


def _assert_grid_within_bound(got, want, scales, where):
    worst = 0.0
    for k, s in enumerate(scales):
        err = np.abs(got[k] - want[k]).max()
        print(where, "output", k, "scale", s, "err", err)
        worst = max(worst, err / s if s > 0 else (0.0 if err == 0 else np.inf))
        assert err <= 1e-11 * s, (where, k, err, s)
    return worst


def _assert_local_rows(local, gidx, where):
    """a rank's rows are its gidx, then the ghosts of those"""
    N = local["N"]
    assert N == len(gidx) and np.array_equal(local["key"][:N], gidx), where
    gk = local["key"][N:]
    assert np.all(gk >= rec.GHOST), where
    parent_key = (gk & (rec.GHOST - 1)) >> 2
    assert np.all(np.isin(parent_key, gidx)), where
    off, idx = local["ghost_off"], local["ghost_idx"]
    assert off[N] == off[local["M"]] == len(idx) == local["M"] - N, where
    for i in range(N):
        for g in idx[off[i]:off[i + 1]]:
            assert ((local["key"][g] & (rec.GHOST - 1)) >> 2) == gidx[i], where


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("world", [2, 4])
def test_recorded_tiled_batch_against_the_single_recorder(single_recorded, world):
    S = single_recorded
    kind, cfg, A = S["kind"], S["cfg"], S["world"]
    res = _ranks("recorded", world, kind)
    names = list(A.EUL_OUTPUTS)
    ghost_ranks, most = set(), 0
    for r, out in enumerate(res):
        assert out["ran"] == 24 and out["frames"] == ([5, 0, 0, 0], [5, 0, 3, 0], False), (r, out["ran"], out["frames"])
    for k, s in enumerate(OUT5):
        want = S["floe"][k]
        assert want["tstep"] == s
        for r, out in enumerate(res):
            rec.assert_frames_equal(out["merged"][k], want, (kind, world, "merged frame", s, "rank", r))
            _assert_local_rows(out["local"][k], out["gidx"], (kind, world, "local rows", s, r))
            if out["local"][k]["M"] > out["local"][k]["N"]:
                ghost_ranks.add(r)
        rec.assert_frames_equal(rec.merge([out["local"][k] for out in res]), want, (kind, world, "reference merge", s))
        most = max(most, int(np.diff(want["ghost_off"]).max()))
        # every list number is claimed by exactly one rank
        keys = np.sort(np.concatenate([out["local"][k]["key"] for out in res]))
        assert len(np.unique(keys)) == len(keys) == want["M"] and np.array_equal(keys[:want["N"]], np.arange(want["N"]))
    if kind == "periodic":
        assert len(ghost_ranks) >= 2 and most == 3
    worst = 0.0
    for k, s in enumerate(OUT5):
        t, ref = S["grid0"][k]
        for r, out in enumerate(res):
            assert out["grid0"][k][0] == t == s and _same(out["grid0"][k][1], res[0]["grid0"][k][1]), (kind, world, "grid frames differ between ranks", s, r)
        worst = max(worst, _assert_grid_within_bound(res[0]["grid0"][k][1], ref, _scales(names, ref, names), (kind, world, "grid writer 0", s)))
        if world == 2:
            assert all(_same(out["grid0"][k][1], out["hand0"][k]) for out in res), (kind, "grid frame against the hand cut", s)
    for k, s in enumerate(OUT7):
        t, ref = S["grid2"][k]
        for r, out in enumerate(res):
            assert out["grid2"][k][0] == t == s and _same(out["grid2"][k][1], res[0]["grid2"][k][1]), (kind, world, "second grid writer differs between ranks", s, r)
        worst = max(worst, _assert_grid_within_bound(res[0]["grid2"][k][1], ref, _scales(THREE, S["all2"][k], names), (kind, world, "grid writer 2", s)))
        assert np.abs(ref).max() > 0
        if world == 2:
            assert all(_same(out["grid2"][k][1], out["hand2"][k]) for out in res), (kind, "second grid writer against the hand cut", s)
    print(kind, world, "ranks: largest grid error over its bound's scale:", worst)
    _assert_ranks_equal_single([out["end"] for out in res], A, A.dissolved(), (kind, world, "final state"))


def test_hand_cut_equals_recorded_on_tiles():
    res = _ranks("hand_cut", 2)
    for r, out in enumerate(res):
        assert out["tsteps"] == list(OUT5), (r, out["tsteps"])
        for k, end in enumerate((10, 20, 27)):
            for other in ("H", "P"):
                assert np.array_equal(out["R"][k]["gidx"], out[other][k]["gidx"])
                _assert_bit_equal(out["R"][k]["cols"], out[other][k]["cols"], f"rank {r}, behind step {end}: recorded against {other}")


def test_ends_and_full_on_tiles():
    res = _ranks("ends", 2)
    for r, out in enumerate(res):
        assert out["tagged"] == [(1, []), (1, [5])], (r, out["tagged"])          # (ends at step 5, which it did not begin; then begins it)
        assert out["calls"] == [(5, [0]), (5, [0, 5])], (r, out["calls"])          # none for 10: the next call's
        assert out["through"] == (12, [0, 5, 10]), (r, out["through"])
        assert out["room"] == (12, [0, 3, 6, 9]), (r, out["room"])
        assert out["full"] == (6, [0, 3], True), (r, out["full"])
        for a, b in zip(out["full_merged"], out["room_merged"]):
            rec.assert_frames_equal(a, b, (r, "frames in front of the full stop"))
        assert out["cleared"] == ([0] * 4, [0] * 4, False)
        assert out["rest"] == (6, [6, 9], False), (r, out["rest"])
        assert np.array_equal(out["q"]["gidx"], out["p"]["gidx"])
        _assert_bit_equal(out["q"]["cols"], out["p"]["cols"], f"rank {r}: after a full stop and a clear")


def test_removal_between_frames_on_tiles():
    cfg = cases.case_b()
    start = np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125)

    def single(record):
        w = _build(mk(), cfg)
        w.set_removal(True); w.set_dissolved(start)
        if record:
            w.set_floe_output(0, 5, RM_COLUMNS)
        assert w.run(cases.B_STEPS, 0, cfg["dt"], **cases.B_RUN) == cases.B_STEPS
        return w
    D, F = single(True), single(False)
    want = [D.floe_frame(0, k) for k in range(D.output_frames()[0][0])]
    ns = [f["N"] for f in want]
    assert len(want) == 8 and ns[0] == cfg["n_floes"] and ns[-1] < ns[0] and len(set(ns)) >= 4
    res = _ranks("removal", 2)
    for r, out in enumerate(res):
        assert out["ran"] == cases.B_STEPS and len(out["merged"]) == 8
        for k, f in enumerate(want):
            rec.assert_frames_equal(out["merged"][k], f, ("removal", "merged frame", k, "rank", r))
            assert np.array_equal(np.sort(np.concatenate([o["local"][k]["key"] for o in res])), np.arange(f["N"]))          # the global numbers of their step
    _assert_ranks_equal_single([out["end"] for out in res], F, F.dissolved(), "against the single run without a recorder")


def test_a_pending_ridge_raft_step_has_its_frame_on_tiles():
    import test_ridgeraft_gpu as trr
    from subzero_jl_amd import fields
    cfg = trr._dense()
    A = trr._set(fields.build_world(mk(), cfg), dt=10)
    A.set_floe_output(0, 10)
    assert A.run(40, 1, cfg["dt"], coupling_dt=1) == 9 and A.ridgeraft_pending() == 10
    want = A.floe_frame(0, 0)
    res = _ranks("pending", 2)
    for r, out in enumerate(res):
        assert (out["ran"], out["pending"], out["tsteps"]) == (9, 10, [10]), (r, out["ran"], out["pending"], out["tsteps"])
        rec.assert_frames_equal(out["merged"][0], want, ("the frame of the pending step", r))
        assert out["more"] == 5 and out["tsteps_after"] == [10]


def test_frames_survive_a_migration():
    cfg = _cfg("periodic")
    A = _world(cfg)
    A.set_floe_output(0, 5)
    assert A.run(20, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True) == 20
    want = [A.floe_frame(0, k) for k in range(4)]
    assert [f["tstep"] for f in want] == [0, 5, 10, 15]
    res = _ranks("migration", 2)
    assert sum(out["moved"] for out in res) > 50
    for r, out in enumerate(res):
        assert out["first"] == 10 and out["second"] == 10 and not np.array_equal(out["gidx_before"], out["gidx_after"])
        rec.assert_frames_equal(out["before"], want[1], ("merged before the migration", r))
        for k, f in enumerate(want):
            rec.assert_frames_equal(out["merged"][k], f, ("merged behind the migration", k, r))
            rec.assert_frames_equal(rec.merge([o["local"][k] for o in res]), f, ("reference merge", k))
            assert np.array_equal(out["local"][k]["key"][:out["local"][k]["N"]], out["gidx_before"] if k < 2 else out["gidx_after"]), (r, k)
    _assert_ranks_equal_single([out["end"] for out in res], A, A.dissolved(), "behind the migration")


def test_refusals_and_off_on_tiles(single_recorded):
    from subzero_jl_amd import capi, tiles
    S = single_recorded
    kind, cfg = S["kind"], S["cfg"]
    if kind == "periodic":
        # the tile setters want a tiled context
        w = _world(cfg)
        w._push()
        xg, yg = (np.ascontiguousarray(a) for a in _grids(cfg)[0])
        codes = np.array([0, 5], np.int32)
        assert w.L.sz_tile_set_floe_output(w.h, 0, 5, 1, 1 << 20) == E_STATE and b"sz_set_floe_output" in w.L.sz_last_error(w.h)
        assert w.L.sz_tile_set_grid_output(w.h, 0, 5, 10, 7, capi.ptr(xg), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4) == E_STATE
        assert w.L.sz_tile_set_floe_output(w.h, 4, 5, 1, 1 << 20) == E_ARG
        res = _ranks("refuse", 2)
        for r, out in enumerate(res):
            assert out["bad"] == [E_ARG] * len(out["bad"]) and out["single_setters"] == (E_STATE, E_STATE), (r, out["bad"], out["single_setters"])
            rc, done, msg = out["differ"]
            assert rc == E_STATE and done == 0 and "floe output writer 0" in msg, (r, out["differ"])
            _assert_bit_equal(out["differ_unchanged"][0]["cols"], out["differ_unchanged"][1]["cols"], f"rank {r}: refused, nothing ran")
            assert out["step"][:2] == (E_STATE, 0) and "sz_tile_run" in out["step"][2], (r, out["step"])
            assert out["then"] == (6, [0, 5]), (r, out["then"])
            assert out["two_way"] == (E_STATE, 0), (r, out["two_way"])
            assert out["off"]["ran"] == out["fresh"]["ran"] == 12 and out["off"]["frames"] == ([0] * 4, [0] * 4, False)
            assert out["off"]["launches"] == out["fresh"]["launches"], (r, out["off"]["launches"], out["fresh"]["launches"])
            _assert_bit_equal(out["off"]["snap"]["cols"], out["fresh"]["snap"]["cols"], f"rank {r}: writers set and turned off")
    # one rank as a tiled context
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    _set_three_writers(tw, cfg)
    assert tw.run(24, 3, cfg["dt"], **RUN) == 24 and tw.output_frames() == ([5, 0, 0, 0], [5, 0, 3, 0], False)
    names = list(S["world"].EUL_OUTPUTS)
    for k in range(5):
        rec.assert_frames_equal(tw.floe_frame(0, k), S["floe"][k], (kind, "one rank, merged", k))
        local = tw.floe_frame_local(0, k)
        rec.assert_frames_equal({n: v for n, v in local.items() if n != "key"}, S["floe"][k], (kind, "one rank, local", k))
        t, d = tw.grid_frame(0, k)
        assert t == S["grid0"][k][0]
        _assert_grid_within_bound(d, S["grid0"][k][1], _scales(names, S["grid0"][k][1], names), (kind, "one rank, grid writer 0", k))
    for k in range(3):
        t, d = tw.grid_frame(2, k)
        assert t == S["grid2"][k][0]
        _assert_grid_within_bound(d, S["grid2"][k][1], _scales(THREE, S["all2"][k], names), (kind, "one rank, grid writer 2", k))

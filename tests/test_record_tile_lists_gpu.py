"""floe.interactions and the sub-floe points in the frames of tiled runs (sz_tile_set_floe_output_lists; csrc/sz_record_tile.hpp, tile_record;
DESIGN.md §9i, "Tiled contexts", the lists).  Ranks are spawned processes that share the one GPU and trade through gloo (backend "library-host"),
with the helpers of tests/test_record_tiles_gpu.py.  The yardstick is the single context's recorder with lists (held to the hand cut and to the
oracle by tests/test_record_lists_gpu.py) on the 300-floe fields of tests/test_record_gpu.py; the merge is also held to the numpy rule of
tests/record_tile_lists_ref.py.  Same kernels on the same floes: every comparison is bit for bit."""
import ctypes as C
import datetime
import os

import numpy as np
import pytest

import record_lists_ref as lref
import record_tile_lists_ref as tl
import record_tiles_ref as rec
import remove_tiles_cases as cases
from test_record_gpu import KINDS, _cfg, _world, mk
from test_record_tiles_gpu import RM_COLUMNS, RUN, _assert_local_rows, _frames, _tsteps
from test_remove_gpu import _assert_bit_equal, _build
from test_remove_tiles_gpu import _assert_ranks_equal_single, _snap, _tiled
from test_tiles_gpu import _collect, _free_port, _guard

pytestmark = pytest.mark.gpu

LISTS = ["interactions", "subpoints"]
OUT5 = (5, 10, 15, 20, 25)
E_ARG, E_STATE = -2, -4


def _with_lists(tw, writer=0, dt_out=5, columns=None, lists=LISTS, **kw):
    tw.set_floe_output(writer, dt_out, columns, **kw)
    tw.set_floe_output_lists(writer, lists)


def _same_frames(a, b):
    return sorted(a) == sorted(b) and all(rec.same(a[n], b[n]) if isinstance(a[n], np.ndarray) else a[n] == b[n] for n in a)


# ---------------------------------------------------------------- ranks
def _s_recorded(rank, world, dist, kind):
    cfg = _cfg(kind)
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    _with_lists(tw)
    out = dict(gidx=np.array(tw.gidx), ran=tw.run(24, 3, dt, **RUN), frames=tw.output_frames())
    out["merged"], out["local"] = _frames(tw)
    n = len(out["merged"])
    out["again"] = [tw.floe_frame(0, k) for k in range(n)]          # a second merge of every frame
    out["tables"] = [tw.frame_list_keys(0, k) for k in range(n)]
    out["info"] = [tw.floe_frame_lists_info(0, k) for k in range(n)]
    out["rows_only"] = tw.floe_frame(0, 1, members=["inter_off", "inter_rows"] if rank == 0 else ["inter_off"])
    out["end"] = _snap(tw)
    # the same run with a writer without lists: today's frames, and the state the lists must not change
    p = _tiled(cfg, rank, world, dist)
    p.set_floe_output(0, 5)
    out["plain_ran"] = p.run(24, 3, dt, **RUN)
    out["plain_merged"] = [p.floe_frame(0, k) for k in range(p.output_frames()[0][0])]
    out["plain_info"] = p.floe_frame_lists_info(0, 0)
    out["plain_table"] = p.frame_list_keys(0, 0)
    out["plain_end"] = _snap(p)
    return out


def _s_migration(rank, world, dist):
    from subzero_jl_amd import capi
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    L = cfg["L"]
    tw = _tiled(cfg, rank, world, dist)
    _with_lists(tw)
    out = dict(first=tw.run(10, 0, dt, **RUN))
    out["before"] = tw.floe_frame(0, 1)          # (merged before the migration, and again behind it)
    out["moved"] = tw.migrate(owner_fn=lambda cx, cy: (cy > 0.5 * L).astype(int))
    out["second"] = tw.run(10, 10, dt, **RUN)          # its first act: the frame of step 10, behind the migration
    out["merged"], out["local"] = _frames(tw)
    out["info"] = [tw.floe_frame_lists_info(0, k) for k in range(4)]
    try:
        tw.floe_frame(0, 2, members=["inter_off", "inter_rows"])
        out["asked"] = None
    except capi.SzError as e:
        out["asked"] = str(e)
    out["end"] = _snap(tw)
    return out


def _s_removal(rank, world, dist):
    cfg = cases.case_b()
    tw = _tiled(cfg, rank, world, dist)
    tw.set_removal()
    tw.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    _with_lists(tw, columns=RM_COLUMNS)
    out = dict(ran=tw.run(cases.B_STEPS, 0, cfg["dt"], stop_on_tags=True, **cases.B_RUN))
    out["merged"] = _frames(tw, local=False)[0]
    out["end"] = _snap(tw)
    return out


def _s_pending(rank, world, dist):
    from test_ridgeraft_gpu import _dense
    cfg = _dense()
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_ridgeraft(True, dt=10)
    _with_lists(tw, dt_out=10)
    out = dict(ran=tw.run(40, 1, dt, **RUN), pending=tw.ridgeraft_pending(), tsteps=_tsteps(tw))
    out["merged"] = _frames(tw, local=False)[0]
    return out


def _s_behind_rr(rank, world, dist):
    """a frame recorded as the first act behind a ridge / raft step: the step in front of it was list-based"""
    from subzero_jl_amd import capi
    from test_ridgeraft_gpu import _dense
    cfg = _dense()
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    tw.set_ridgeraft(True, dt=10)
    _with_lists(tw, dt_out=11)
    out = dict(ran=tw.run(40, 1, dt, **RUN), pending=tw.ridgeraft_pending(), tsteps=_tsteps(tw))
    tw.finish_step(10, dt, coupling_dt=1)
    out["more"] = tw.run(5, 11, dt, **RUN)
    out["tsteps_after"] = _tsteps(tw)
    out["merged"] = tw.floe_frame(0, 0)
    out["local"] = tw.floe_frame_local(0, 0)
    out["info"] = tw.floe_frame_lists_info(0, 0)
    try:
        tw.floe_frame(0, 0, members=["inter_off"])
        out["asked"] = None
    except capi.SzError as e:
        out["asked"] = str(e)
    return out


def _local_sizes(tw, mask, k):
    """the size of this rank's tile frame k by the Python mirror, from the local counts"""
    w = tw.world
    fr = tw.floe_frame_local(0, k, members=[])
    V = C.c_int64(0); tot = [C.c_int64(0), C.c_int64(0)]
    assert w.L.sz_floe_frame_info(w.h, 0, k, None, None, None, C.byref(V), None) == 0
    assert w.L.sz_floe_frame_lists_info(w.h, 0, k, C.byref(tot[0]), C.byref(tot[1])) == 0
    return tw.tile_frame_bytes(mask, fr["M"], fr["N"], int(V.value), LISTS, int(tot[0].value), int(tot[1].value), len(tw.frame_list_keys(0, k)))


def _s_room(rank, world, dist):
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    p = _tiled(cfg, rank, world, dist)
    _with_lists(p, dt_out=3)
    out = dict(room=(p.run(12, 0, dt, **RUN), _tsteps(p)))
    mask = p.world.frame_mask(None)
    sizes = [_local_sizes(p, mask, k) for k in range(2)]
    out["table_lengths"] = [len(p.frame_list_keys(0, k)) for k in range(4)]
    every = [None] * world
    dist.all_gather_object(every, sizes[0] + sizes[1])
    fullest = int(np.argmax(every))
    out["fullest"] = (fullest, every)
    for name, less in (("full", 0), ("one_less", 1)):
        q = _tiled(cfg, rank, world, dist)
        _with_lists(q, dt_out=3, arena_bytes=every[fullest] - less if rank == fullest else 1 << 26)
        out[name] = (q.run(12, 0, dt, **RUN), _tsteps(q), q.output_frames()[2])
        if not less:
            out["full_merged"] = _frames(q, local=False)[0]; out["room_merged"] = _frames(p, local=False)[0][:2]
    return out


def _s_refuse(rank, world, dist):
    from subzero_jl_amd import capi
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    tw = _tiled(cfg, rank, world, dist)
    L, h = tw.world.L, tw.world.h
    out = dict(off=L.sz_tile_set_floe_output_lists(h, 0, 1))
    tw.set_floe_output(0, 5, ["cx"])
    out["bad"] = [L.sz_tile_set_floe_output_lists(h, 0, 4), L.sz_tile_set_floe_output_lists(h, 0, 7), L.sz_tile_set_floe_output_lists(h, 4, 1),
                  L.sz_tile_set_floe_output_lists(h, -1, 1)]
    out["other_off"] = L.sz_tile_set_floe_output_lists(h, 1, 1)
    # the pinned refusals of the single setter on a tiled context, and of TiledWorld.set_floe_output
    out["pinned"] = (L.sz_set_floe_output_lists(h, 0, 1), L.sz_last_error(h).decode(), L.sz_set_floe_output_lists(h, 0, 8))
    try:
        tw.set_floe_output(0, 5, ["cx"], lists=["interactions"])
        out["tiled_world"] = None
    except capi.SzError as e:
        out["tiled_world"] = str(e)
    # the lists are set behind the writer, free its frames, and are reset by setting the writer again
    assert tw.run(6, 0, dt, **RUN) == 6
    out["held"] = tw.output_frames()[0][0]
    tw.set_floe_output_lists(0, ["subpoints"])
    out["freed"] = tw.output_frames()[0][0]
    assert tw.run(1, 10, dt, **RUN) == 1
    out["sub_only"] = sorted(tw.floe_frame(0, 0))
    out["sub_only_asked"] = L.sz_tile_download_floe_frame_interactions(h, 0, 0, None, None)          # (collective: every rank takes part and is refused)
    tw.set_floe_output(0, 5, ["cx"])
    assert tw.run(1, 15, dt, **RUN) == 1
    out["reset"] = (sorted(tw.floe_frame(0, 0)), tw.floe_frame_lists_info(0, 0))
    # the ranks disagree on the lists
    t2 = _tiled(cfg, rank, world, dist)
    t2.set_floe_output(0, 5, ["cx"])
    t2.set_floe_output_lists(0, ["interactions"] if rank == 0 else LISTS)
    before = _snap(t2)
    done = C.c_int32(7)
    flags = capi.COLLISIONS_ON | capi.COUPLING_ON
    out["differ"] = (t2.world.L.sz_tile_run(t2.world.h, 8, 0, dt, 1, flags, C.byref(done)), done.value, t2.world.L.sz_last_error(t2.world.h).decode())
    out["differ_unchanged"] = (before, _snap(t2))
    return out


SCENARIOS = {f.__name__[3:]: f for f in (_s_recorded, _s_migration, _s_removal, _s_pending, _s_behind_rr, _s_room, _s_refuse)}


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
    kind = request.param
    cfg = _cfg(kind)
    A = _world(cfg)
    A.set_floe_output(0, 5, lists=LISTS)
    A.set_floe_output(1, 1, ["ghost_links"])          # every step's ghost list: what a partner above N of the NEXT step's rows counts in
    assert A.run(24, 3, cfg["dt"], coupling_dt=1, stop_on_tags=True) == 24
    assert A.output_frames() == ([5, 24, 0, 0], [0] * 4, False)
    links = {f["tstep"]: f for f in (A.floe_frame(1, k) for k in range(24))}
    return dict(kind=kind, cfg=cfg, world=A, floe=[A.floe_frame(0, k) for k in range(5)], links=links)


def _merged_equals(got, want, where, lists=3):
    got = dict(got)
    assert got.pop("lists") == lists, (where, "the frame's lists word")
    rec.assert_frames_equal(got, want, where)


def _ghost_table(tables):
    """the sorted distinct ghost keys of all ranks' key tables: the single context's ghost list of the last step"""
    t = np.concatenate(tables)
    return np.unique(t[t >= tl.GHOST])


# ---------------------------------------------------------------- tests
@pytest.mark.parametrize("world", [2, 4])
def test_recorded_tiled_batch_with_lists_against_the_single_recorder(single_recorded, world):
    S = single_recorded
    kind, A = S["kind"], S["world"]
    res = _ranks("recorded", world, kind)
    owner = np.full(A.N, -1)
    for r, out in enumerate(res):
        assert out["ran"] == 24 and out["frames"] == ([5, 0, 0, 0], [0] * 4, False), (r, out["ran"], out["frames"])
        owner[out["gidx"]] = r
    assert np.all(owner >= 0)
    cross_floe = cross_ghost = False
    for k, s in enumerate(OUT5):
        want = S["floe"][k]
        N, M = want["N"], want["M"]
        assert want["tstep"] == s
        ghosts = _ghost_table([out["tables"][k] for out in res])
        for r, out in enumerate(res):
            where = (kind, world, "step", s, "rank", r)
            _merged_equals(out["merged"][k], want, where + ("merged frame",))
            assert _same_frames(out["merged"][k], out["again"][k]), where + ("two merges of one frame",)
            assert out["info"][k] == (3, len(want["inter_rows"]), len(want["sx"])), where
            # this rank's own frame: its owned rows' spans are the single frame's spans of those rows
            loc = out["local"][k]
            assert loc["lists"] == 3
            _assert_local_rows(loc, out["gidx"], where + ("local rows",))
            rows = lref.renumbered(loc["inter_rows"], ghosts, N)
            assert np.all(loc["inter_off"][loc["N"]:] == loc["inter_off"][loc["N"]]), where
            for j, g in enumerate(out["gidx"]):
                a, b = loc["inter_off"][j], loc["inter_off"][j + 1]
                assert rec.same(rows[a:b], want["inter_rows"][want["inter_off"][g]:want["inter_off"][g + 1]]), where + ("rows of floe", g)
                a, b = loc["sub_off"][j], loc["sub_off"][j + 1]
                assert rec.same(loc["sx"][a:b], want["sx"][want["sub_off"][g]:want["sub_off"][g + 1]]), where + ("points of floe", g)
                assert rec.same(loc["sy"][a:b], want["sy"][want["sub_off"][g]:want["sub_off"][g + 1]]), where + ("points of floe", g)
            # untranslated: a partner above N is a key + 1, never a list number
            idx = loc["inter_rows"][:, 0]
            assert not np.any((idx > N) & (idx <= tl.LIMIT)), where
        # the library's merge against the numpy rule
        tiles = [dict(out["local"][k], lkeys=out["tables"][k]) for out in res]
        rec.assert_frames_equal(tl.merge(tiles), want, (kind, world, "reference merge", s))
        # what the single context's frame must exercise
        idx = want["inter_rows"][:, 0]
        floe = np.repeat(np.arange(M), np.diff(want["inter_off"]))
        assert not np.any(idx > tl.LIMIT), (kind, s, "a partner left as an order key")
        assert np.any(np.diff(want["inter_off"][:N + 1]) == 0)
        if kind == "periodic" and k > 0:
            assert np.any(idx > N), (kind, s, "no partner that was a ghost")
        if kind == "walls":
            assert np.any(idx < 0), (kind, s, "no boundary / topography partner")
        p = (idx > 0) & (idx <= N)
        cross_floe = cross_floe or bool(np.any(owner[idx[p].astype(np.int64) - 1] != owner[floe[p]]))
        g = idx > N
        if np.any(g):
            # the ghost's parent, from the single context's own ghost list of the step before (its frame of that step)
            last = S["links"][s - 1]
            assert last["M"] - last["N"] >= int(idx[g].max()) - N
            parent = lref.parents_of(last["ghost_off"], last["ghost_idx"], last["N"], last["M"])[idx[g].astype(np.int64) - 1]
            assert np.all(parent >= 0) and np.all(parent < N)
            cross_ghost = cross_ghost or bool(np.any(owner[parent] != owner[floe[g]]))
            assert np.array_equal(parent, (ghosts[idx[g].astype(np.int64) - N - 1] & (tl.GHOST - 1)) >> 2), (kind, s, "the key tables name other parents")
    assert cross_floe, (kind, world, "no row whose partner floe another rank owns")
    if kind == "periodic":
        assert cross_ghost, (kind, world, "no ghost partner whose parent another rank owns")
    # only a rank that asks takes the rows
    assert rec.same(res[0]["rows_only"]["inter_rows"], S["floe"][1]["inter_rows"]) and "inter_rows" not in res[1]["rows_only"]
    assert all(rec.same(out["rows_only"]["inter_off"], S["floe"][1]["inter_off"]) for out in res)
    # a writer without lists: today's frame
    for r, out in enumerate(res):
        assert out["plain_ran"] == 24 and out["plain_info"] == (0, 0, 0) and len(out["plain_table"]) == 0
        for k, want in enumerate(S["floe"]):
            rec.assert_frames_equal(out["plain_merged"][k], {n: v for n, v in want.items() if n not in tl.LISTS}, (kind, world, "without lists", k, r))
        assert np.array_equal(out["end"]["gidx"], out["plain_end"]["gidx"])
        _assert_bit_equal(out["end"]["cols"], out["plain_end"]["cols"], f"rank {r}: final state against the tiled run without lists")
    _assert_ranks_equal_single([out["end"] for out in res], A, A.dissolved(), (kind, world, "final state"))


def test_frames_with_lists_and_a_migration():
    cfg = _cfg("periodic")
    A = _world(cfg)
    A.set_floe_output(0, 5, lists=LISTS)
    assert A.run(20, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True) == 20
    want = [A.floe_frame(0, k) for k in range(4)]
    assert [f["tstep"] for f in want] == [0, 5, 10, 15] and len(want[2]["inter_rows"]) > 0
    res = _ranks("migration", 2)
    assert sum(out["moved"] for out in res) > 50
    for r, out in enumerate(res):
        assert out["first"] == 10 and out["second"] == 10
        _merged_equals(out["before"], want[1], ("merged before the migration", r))
        for k in (0, 1, 3):          # (0, 1: recorded before the migration, merged behind it; 3: the next output step, complete again)
            _merged_equals(out["merged"][k], want[k], ("merged behind the migration", k, r))
            assert out["info"][k] == (3, len(want[k]["inter_rows"]), len(want[k]["sx"]))
        # the frame recorded as the first act behind the migration: no rows of a last step on any rank, the points all the same
        lost = {n: v for n, v in want[2].items() if n not in ("inter_off", "inter_rows")}
        _merged_equals(out["merged"][2], lost, ("the frame behind the migration", r), lists=2)
        assert out["info"][2] == (2, 0, len(want[2]["sx"])) and out["local"][2]["lists"] == 2 and "inter_off" not in out["local"][2]
        assert out["asked"] is not None and "sz_tile_migrate" in out["asked"], out["asked"]
    _assert_ranks_equal_single([out["end"] for out in res], A, A.dissolved(), "behind the migration")


def test_removal_between_frames_with_lists():
    cfg = cases.case_b()
    w = _build(mk(), cfg)
    w.set_removal(True); w.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    w.set_floe_output(0, 5, RM_COLUMNS, lists=LISTS)
    assert w.run(cases.B_STEPS, 0, cfg["dt"], **cases.B_RUN) == cases.B_STEPS
    want = [w.floe_frame(0, k) for k in range(w.output_frames()[0][0])]
    ns = [f["N"] for f in want]
    assert len(want) == 8 and ns[-1] < ns[0] and len(set(ns)) >= 4 and sum(len(f["inter_rows"]) for f in want) > 0
    res = _ranks("removal", 2)
    for r, out in enumerate(res):
        assert out["ran"] == cases.B_STEPS and len(out["merged"]) == 8
        for k, f in enumerate(want):
            _merged_equals(out["merged"][k], f, ("removal", "merged frame", k, "rank", r))
    _assert_ranks_equal_single([out["end"] for out in res], w, w.dissolved(), "against the single run with lists")


def test_a_pending_ridge_raft_step_has_its_frame_with_lists():
    import test_ridgeraft_gpu as trr
    from subzero_jl_amd import fields
    cfg = trr._dense()
    A = trr._set(fields.build_world(mk(), cfg), dt=10)
    A.set_floe_output(0, 10, lists=LISTS)
    assert A.run(40, 1, cfg["dt"], coupling_dt=1) == 9 and A.ridgeraft_pending() == 10
    want = A.floe_frame(0, 0)
    assert len(want["inter_rows"]) > 0
    res = _ranks("pending", 2)
    for r, out in enumerate(res):
        assert (out["ran"], out["pending"], out["tsteps"]) == (9, 10, [10]), (r, out["ran"], out["pending"], out["tsteps"])
        _merged_equals(out["merged"][0], want, ("the frame of the pending step", r))


def test_a_frame_right_behind_a_ridge_raft_step_has_points_and_no_interactions():
    """the ridge / raft step of a tile is list-based: its rows name ghosts by key and no table of them is kept, so the frame recorded before the
    next step has the interactions bit cleared on every rank, as behind a migration; the points are the single context's.  The pending table
    is not empty and no host ridges here, so the state columns behind the step are not what this file is about: the frame's columns are held
    to the numpy merge of the ranks' own frames, its rows and points to the single context's frame"""
    import test_ridgeraft_gpu as trr
    from subzero_jl_amd import fields
    cfg = trr._dense()
    A = trr._set(fields.build_world(mk(), cfg), dt=10)
    A.set_floe_output(0, 11, lists=LISTS)
    assert A.run(40, 1, cfg["dt"], coupling_dt=1) == 9 and A.ridgeraft_pending() == 10
    A.finish_step(10, cfg["dt"], coupling_dt=1)
    assert A.run(5, 11, cfg["dt"], coupling_dt=1) == 5
    want = A.floe_frame(0, 0)
    assert want["tstep"] == 11
    res = _ranks("behind_rr", 2)
    for r, out in enumerate(res):
        assert (out["ran"], out["pending"], out["tsteps"], out["more"], out["tsteps_after"]) == (9, 10, [], 5, [11]), (r, out["ran"], out["pending"], out["tsteps"])
        got = out["merged"]
        assert got["lists"] == 2 and "inter_off" not in got and (got["tstep"], got["M"], got["N"]) == (11, want["M"], want["N"])
        assert all(rec.same(got[n], want[n]) for n in ("sub_off", "sx", "sy", "id", "ghost_id")), (r, "points of the frame behind the ridge / raft step")
        _merged_equals(got, tl.merge([o["local"] for o in res]), ("the frame behind the ridge / raft step against the reference merge", r), lists=2)
        assert out["info"] == (2, 0, len(want["sx"])) and out["local"]["lists"] == 2 and "inter_off" not in out["local"]
        assert out["asked"] is not None and "list-based" in out["asked"], out["asked"]


def test_room_counts_the_lists_on_tiles():
    res = _ranks("room", 2)
    fullest, every = res[0]["fullest"]
    for r, out in enumerate(res):
        assert out["fullest"] == (fullest, every)
        assert out["room"] == (12, [0, 3, 6, 9]), (r, out["room"])
        assert out["table_lengths"][0] == 0 and min(out["table_lengths"][1:]) > 0, (r, out["table_lengths"])
        assert out["full"] == (6, [0, 3], True), (r, out["full"])          # the third output step is not taken on any rank
        assert out["one_less"] == (3, [0], True), (r, out["one_less"])          # one byte less on the fullest rank: the second finds no room
        for a, b in zip(out["full_merged"], out["room_merged"]):
            assert _same_frames(a, b), (r, "frames in front of the full stop")


def test_refusals_of_the_tile_lists(single_recorded):
    from subzero_jl_amd import capi, tiles
    S = single_recorded
    kind, cfg = S["kind"], S["cfg"]
    # one rank as a tiled context: merged and local frames are the single context's
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    _with_lists(tw)
    assert tw.run(24, 3, cfg["dt"], **RUN) == 24 and tw.output_frames() == ([5, 0, 0, 0], [0] * 4, False)
    for k in range(5):
        _merged_equals(tw.floe_frame(0, k), S["floe"][k], (kind, "one rank, merged", k))
        assert tw.floe_frame_lists_info(0, k) == (3, len(S["floe"][k]["inter_rows"]), len(S["floe"][k]["sx"]))
    if kind != "periodic":
        return
    # a writer set through the single setter, on a single context
    w = _world(cfg)
    w._push()
    assert w.L.sz_tile_set_floe_output_lists(w.h, 0, 1) == E_STATE          # off
    w.set_floe_output(0, 1, ["cx"])
    assert w.L.sz_tile_set_floe_output_lists(w.h, 0, 1) == E_STATE and b"sz_set_floe_output_lists" in w.L.sz_last_error(w.h)
    assert w.L.sz_tile_set_floe_output_lists(w.h, 0, 4) == E_ARG
    res = _ranks("refuse", 2)
    for r, out in enumerate(res):
        assert out["off"] == E_STATE and out["bad"] == [E_ARG] * 4 and out["other_off"] == E_STATE, (r, out["off"], out["bad"], out["other_off"])
        assert out["pinned"][0] == E_STATE and "tile frames record no lists yet" in out["pinned"][1] and out["pinned"][2] == E_ARG, (r, out["pinned"])
        assert out["tiled_world"] is not None
        assert out["held"] == 2 and out["freed"] == 0
        assert out["sub_only"] == ["M", "N", "cx", "lists", "sub_off", "sx", "sy", "tstep"] and out["sub_only_asked"] == E_ARG, (r, out["sub_only"], out["sub_only_asked"])
        assert out["reset"] == (["M", "N", "cx", "tstep"], (0, 0, 0)), (r, out["reset"])
        rc, done, msg = out["differ"]
        assert rc == E_STATE and done == 0 and "floe output writer 0" in msg, (r, out["differ"])
        _assert_bit_equal(out["differ_unchanged"][0]["cols"], out["differ_unchanged"][1]["cols"], f"rank {r}: refused, nothing ran")

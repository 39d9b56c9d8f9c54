"""Output frames on the device (csrc/sz_record.hpp): a batch that records its output steps against the same batch cut by hand
at every output step -- run up to the step, add_ghosts, a column download, eulerian_data, remove_ghosts.  Same kernels on the same state:
every frame comparison is bit for bit.

The fields are the small ones of tests/test_batch_paths_gpu.py: 300 floes at concentration 0.8, seed 31, coupled every step -- periodic
(ghosts; on the CPU oracle that field holds two corner floes with three ghosts each at every output step used here) and between walls with
topography (no ghosts, topography inside the cells)."""
import ctypes as C

import numpy as np
import pytest

import cases
from test_batch_paths_gpu import N_FLOES, WALLS, _tagged_before
from test_ridgeraft_gpu import _assert_bit_equal, _state

pytestmark = pytest.mark.gpu

KINDS = {"periodic": {}, "walls": WALLS}
OWN = ("cx", "cy", "ghost_id", "vert_off", "vx", "vy", "ghost_off", "ghost_idx")          # a ghost row's own; the rest is its parent's
THREE = ["mass_grid", "u_grid", "stress_eig_grid"]


def mk():
    import subzero_jl_amd
    return subzero_jl_amd.World(0)


def _cfg(kind):
    from subzero_jl_amd import fields
    return fields.make_config(n_floes=N_FLOES, seed=31, concentration=0.8, **KINDS[kind])


def _world(cfg):
    from subzero_jl_amd import fields
    return fields.build_world(mk(), cfg)


def _grid(cfg, nx, ny):
    return np.linspace(0, cfg["L"], nx + 1), np.linspace(0, cfg["L"], ny + 1)


def _by_hand(w):
    """the floe frame of the list as it is, cut by hand: add_ghosts, every column down; the ghosts stay in the list for the caller"""
    w.add_ghosts()
    w._pull()
    f = {k: np.array(v) for k, v in w.col.items() if k not in ("sub_off", "sx", "sy")}
    f.update(M=w._M, N=w.N)
    return f


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_frame_is_hand_cut(got, want, where):
    """M, N; every recorded column on the parent rows; cx, cy, ring, id, ghost_id and ghost links on the ghost rows"""
    assert (got["M"], got["N"]) == (want["M"], want["N"]), where
    N = got["N"]
    for k, v in want.items():
        if k in ("M", "N"):
            continue
        if k in OWN or k == "id":
            assert _same(got[k], v), (where, k)
        else:
            assert _same(got[k][:N], v[:N]), (where, k)


@pytest.fixture(scope="module", params=list(KINDS))
def recorded_and_hand_cut(request):
    """World A: one recorded run(24, 3); World B: the same batch cut by hand at the output steps.  Kept for the tests that read the frames."""
    kind = request.param
    cfg = _cfg(kind)
    dt = cfg["dt"]
    g1, g2 = _grid(cfg, 10, 7), _grid(cfg, 12, 12)
    A = _world(cfg)
    A.set_floe_output(0, 5)
    A.set_grid_output(0, 5, *g1)
    A.set_grid_output(2, 7, *g2, outputs=THREE)
    done = A.run(24, 3, dt, coupling_dt=1)
    pipelined = A.pipelined()
    B = _world(cfg)
    t, hand = 3, {}
    for s in [u for u in range(3, 27) if u % 5 == 0 or u % 7 == 0]:
        assert B.run(s - t, t, dt, coupling_dt=1) == s - t
        t = s
        fl = _by_hand(B)
        hand[s] = (fl if s % 5 == 0 else None, B.eulerian_data(*g1) if s % 5 == 0 else None, B.eulerian_data(*g2, THREE) if s % 7 == 0 else None)
        B.remove_ghosts()
    assert B.run(27 - t, t, dt, coupling_dt=1) == 27 - t
    return kind, cfg, A, B, done, pipelined, hand


def test_recorded_batch_is_the_batch_cut_by_hand(recorded_and_hand_cut):
    kind, cfg, A, B, done, pipelined, hand = recorded_and_hand_cut
    assert done == 24
    assert pipelined          # its segments of 4 or more steps stay on the timed path
    nf, ng, full = A.output_frames()
    assert nf == [5, 0, 0, 0] and ng == [5, 0, 3, 0] and not full
    for k, s in enumerate((5, 10, 15, 20, 25)):
        fr = A.floe_frame(0, k)
        assert fr["tstep"] == s
        _assert_frame_is_hand_cut(fr, hand[s][0], (kind, "floe frame", s))
        assert (fr["M"] > fr["N"]) == (kind == "periodic")
        t, d = A.grid_frame(0, k)
        assert t == s and _same(d, hand[s][1]), (kind, "grid frame", s)
    for k, s in enumerate((7, 14, 21)):
        t, d = A.grid_frame(2, k)
        assert t == s and _same(d, hand[s][2]), (kind, "second grid writer", s)
        assert np.abs(d).max() > 0
    _assert_bit_equal(_state(A, rows=False), _state(B, rows=False), (kind, "final state"))


def test_ghost_rows_are_deep_copies(recorded_and_hand_cut):
    kind, cfg, A, B, done, pipelined, hand = recorded_and_hand_cut
    if kind != "periodic":
        assert A.floe_frame(0, 0)["M"] == N_FLOES          # (between walls there is no ghost to look at)
        return
    most = 0
    for k in range(5):
        fr = A.floe_frame(0, k)
        M, N = fr["M"], fr["N"]
        off, idx = fr["ghost_off"], fr["ghost_idx"]
        assert off[N] == off[M] == len(idx) == M - N          # every ghost on one parent's list, no list on a ghost row
        parent = np.full(M, -1)
        for i in range(N):
            parent[idx[off[i]:off[i + 1]]] = i
            most = max(most, off[i + 1] - off[i])
        g = np.arange(N, M)
        assert np.all(parent[g] >= 0) and np.all(fr["ghost_id"][g] > 0) and not np.any(fr["ghost_id"][:N])
        for name, v in fr.items():
            if name in OWN or name in ("tstep", "M", "N"):
                continue
            assert _same(v[g], v[parent[g]]), (k, name)
        assert np.any(fr["cx"][g] != fr["cx"][parent[g]]) and np.any(fr["cy"][g] != fr["cy"][parent[g]])
    assert most == 3          # a corner floe: three ghosts


@pytest.mark.parametrize("kind", list(KINDS))
def test_first_frame_against_the_oracle(kind):
    """run(1, 0) with Δtout = 1 records step 0 before anything moved.  The comparison is tests/test_output.py::test_eulerian_random's: per
    output (per tensor for stress and strain) |got - ref| < 1e-9 x the largest reference value; an output that is identically zero in the
    oracle at step 0 (nothing has collided or accelerated yet) must be identically zero in the frame."""
    from subzero_jl_amd import fields
    from oracle import orc
    cfg = _cfg(kind)
    hw, ow = _world(cfg), fields.build_world(orc.World(), cfg)
    g = _grid(cfg, 10, 7)
    hw.set_floe_output(0, 1, ["cx", "id", "ghost_id"])
    hw.set_grid_output(0, 1, *g)
    assert hw.run(1, 0, cfg["dt"], coupling_dt=1) == 1
    assert hw.output_frames() == ([1, 0, 0, 0], [1, 0, 0, 0], False)
    ow.add_ghosts()
    fr = hw.floe_frame(0, 0)
    oi, og, _ = ow.ids()
    assert fr["tstep"] == 0 and fr["M"] == ow.M and fr["N"] == N_FLOES
    assert np.array_equal(fr["ghost_id"], og) and np.array_equal(fr["id"], oi)
    t, got = hw.grid_frame(0, 0)
    ref = ow.eulerian_data(*g)
    names = orc.EUL_OUTPUTS
    assert t == 0 and np.count_nonzero(ref[names.index("area_grid")]) > 0.5 * 70
    for k, n in enumerate(names):
        grp = [j for j, o in enumerate(names) if o.split("_")[0] == n.split("_")[0]] if n.startswith(("stress", "strain")) else [k]
        scale = max(np.abs(ref[j]).max() for j in grp)
        print(kind, n, "scale", scale, "err", np.abs(got[k] - ref[k]).max())
        if scale == 0:
            assert not got[k].any(), n
        else:
            assert np.abs(got[k] - ref[k]).max() < 1e-9 * scale, n


def _tsteps(w, writer=0):
    return [w.floe_frame(writer, k, members=[])["tstep"] for k in range(w.output_frames()[0][writer])]


def test_the_rule_at_the_ends():
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    w = _world(cfg)
    w.set_floe_output(0, 5, ["cx", "id"])
    _tagged_before(w, cfg)
    assert w.run(8, 4, dt, coupling_dt=1) == 1 and _tsteps(w) == []          # (ends at step 5, which it did not begin)
    assert w.run(8, 5, dt, coupling_dt=1) == 1 and _tsteps(w) == [5]
    w = _world(cfg)
    w.set_floe_output(1, 5, ["cx", "id"])
    assert w.run(5, 0, dt, coupling_dt=1) == 5 and _tsteps(w, 1) == [0]
    assert w.run(5, 5, dt, coupling_dt=1) == 5 and _tsteps(w, 1) == [0, 5]          # none for 10: the next call's
    w = _world(cfg)
    w.set_floe_output(0, 5, ["cx", "id"])
    assert w.run(12, 0, dt, coupling_dt=1, stop_on_tags=False) == 12 and _tsteps(w) == [0, 5, 10]
    assert w.pipelined()


def test_full_ends_the_batch_in_front_of_the_step():
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    g = _grid(cfg, 10, 7)
    w = _world(cfg)
    w.set_grid_output(0, 3, *g, outputs=THREE, max_frames=2)
    assert w.run(12, 0, dt, coupling_dt=1) == 6
    assert w.output_frames() == ([0, 0, 0, 0], [2, 0, 0, 0], True)
    assert [w.grid_frame(0, k)[0] for k in range(2)] == [0, 3]
    w.clear_frames()
    assert w.output_frames() == ([0, 0, 0, 0], [0, 0, 0, 0], False)
    assert w.run(6, 6, dt, coupling_dt=1) == 6
    assert w.output_frames() == ([0, 0, 0, 0], [2, 0, 0, 0], False)
    assert [w.grid_frame(0, k)[0] for k in range(2)] == [6, 9]
    # the same for a floe arena sized for exactly two frames of that field (sized from a run with room)
    mask = w.frame_mask(None)
    p = _world(cfg)
    p.set_floe_output(0, 3)
    assert p.run(12, 0, dt, coupling_dt=1) == 12 and _tsteps(p) == [0, 3, 6, 9]
    sizes = []
    for k in range(4):
        info = [C.c_int64(0) for _ in range(5)]
        assert p.L.sz_floe_frame_info(p.h, 0, k, *(C.byref(v) for v in info)) == 0
        t, M, N, V, G = (v.value for v in info)
        assert G == M - N
        sizes.append(p.frame_bytes(mask, M, N, V))
    q = _world(cfg)
    q.set_floe_output(0, 3, arena_bytes=sizes[0] + sizes[1])
    assert q.run(12, 0, dt, coupling_dt=1) == 6 and _tsteps(q) == [0, 3] and q.output_frames()[2]
    for k in range(2):
        a, b = q.floe_frame(0, k), p.floe_frame(0, k)
        assert all(_same(a[n], b[n]) for n in a if n not in ("tstep", "M", "N"))
    q.clear_frames()
    assert q.run(6, 6, dt, coupling_dt=1) == 6 and _tsteps(q) == [6, 9] and not q.output_frames()[2]
    _assert_bit_equal(_state(q, rows=False), _state(p, rows=False), "after a full stop and a clear")


def test_frames_either_side_of_a_removal_pass():
    """the outflow scenario of tests/test_remove_gpu.py: floes are removed behind steps 1, 10, 11, 14, 15, 25, 29 and 30 of 40"""
    import test_remove_gpu as trm
    cfg, extent = trm.outflow_case()
    dt = cfg["dt"]

    def world(record):
        w = trm._build(mk(), cfg, extent)
        w.set_removal(True)
        w.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
        if record:
            w.set_floe_output(0, 5, ["cx", "id", "status", "rings"])
        return w
    D, F, E = world(True), world(False), world(False)
    assert D.run(trm.NSTEPS, 0, dt, coupling_dt=1) == trm.NSTEPS
    assert F.run(trm.NSTEPS, 0, dt, coupling_dt=1) == trm.NSTEPS
    want = []          # the list at the start of every output step, from a run cut there by hand
    for t in range(0, trm.NSTEPS, 5):
        E._pull()
        want.append((E.N, E.col["id"].copy(), E.col["cx"].copy()))
        assert E.run(5, t, dt, coupling_dt=1) == 5
        assert E.remove_floes()[0]          # (a batch does not look at its own last step: simplify_floes! behind it is the caller's)
    assert D.output_frames()[0][0] == len(want) == 8
    ns = []
    for k, (n, ids, cx) in enumerate(want):
        fr = D.floe_frame(0, k)
        assert fr["tstep"] == 5 * k and fr["N"] == fr["M"] == n and len(fr["vert_off"]) == n + 1
        assert _same(fr["id"], ids) and _same(fr["cx"], cx), k
        ns.append(n)
    assert ns[0] == cfg["n_floes"] and ns[-1] < ns[0] and len(set(ns)) >= 4
    assert D.N == F.N < cfg["n_floes"]
    trm._assert_bit_equal(trm._cols(D), trm._cols(F), "against the run without a recorder")
    assert np.array_equal(D.dissolved(), F.dissolved()) and np.array_equal(D.origin(), F.origin())


def test_a_pending_ridge_raft_step_has_its_frame():
    """the scenario of tests/test_ridgeraft_gpu.py: a batch of 40 from tstep 1 with ridge / raft Δt = 10 stops in the middle of tstep 10"""
    import test_ridgeraft_gpu as trr
    from subzero_jl_amd import fields
    cfg = trr._dense()
    dt = cfg["dt"]
    A = trr._set(fields.build_world(mk(), cfg), dt=10)
    A.set_floe_output(0, 10)
    assert A.run(40, 1, dt, coupling_dt=1) == 9          # (steps_done does not count the pending step)
    assert A.ridgeraft_pending() == 10 and len(trr._table(A)[0]) > 0
    assert _tsteps(A) == [10]
    fr = A.floe_frame(0, 0)
    B = fields.build_world(mk(), cfg)
    assert B.run(9, 1, dt, coupling_dt=1) == 9
    _assert_frame_is_hand_cut(fr, _by_hand(B), "the frame of the pending step")
    B.timestep_collisions(cfg["n_floes"], dt)
    _assert_bit_equal(_state(A), _state(B), "pending")          # the stop is the one without a recorder
    A.finish_step(10, dt, coupling_dt=1)
    assert A.run(5, 11, dt, coupling_dt=1) == 5
    assert _tsteps(A) == [10]          # the next run starts behind the step: nothing more for it


def test_refusals_and_off():
    from subzero_jl_amd import capi
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    g = _grid(cfg, 10, 7)
    w = _world(cfg)
    xg, yg = (np.ascontiguousarray(a) for a in g)
    codes = np.array([0, 5], np.int32)
    L, h = w.L, w.h
    for writer, dto in ((4, 5), (-1, 5), (0, -1)):
        assert L.sz_set_floe_output(h, writer, dto, 1, 1 << 20) == -2
        assert L.sz_set_grid_output(h, writer, dto, 10, 7, capi.ptr(xg), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4) == -2
    uneven = np.array([0.0, 1.0, 3.0])
    assert L.sz_set_grid_output(h, 0, 5, 2, 7, capi.ptr(uneven), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4) == -2
    assert L.sz_set_floe_output(h, 0, 5, 1 << 33, 1 << 20) == -2
    assert w.output_frames() == ([0] * 4, [0] * 4, False)
    w.set_floe_output(0, 1, ["cx", "rings"])
    assert w.run(1, 0, dt, coupling_dt=1) == 1
    assert sorted(k for k in w.floe_frame(0, 0) if k not in ("tstep", "M", "N")) == ["cx", "vert_off", "vx", "vy"]
    for member in ("cy", "ghost_off", "status", "sx"):
        with pytest.raises(capi.SzError):
            w.floe_frame(0, 0, members=["cx", member])
    with pytest.raises(capi.SzError):
        w.floe_frame(0, 1)
    with pytest.raises(capi.SzError):
        w.floe_frame(1, 0)
    # single contexts only: a context with a writer set does not become a tile, a tile takes no writer
    tile = _world(cfg)
    tile._push()
    gidx = np.arange(N_FLOES, dtype=np.int64)
    tile.set_floe_output(0, 5, ["cx"], arena_bytes=1 << 20)
    assert L.sz_tile_enable(tile.h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == -4
    tile.set_floe_output(0, 0)
    assert L.sz_tile_enable(tile.h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    assert L.sz_set_floe_output(tile.h, 0, 5, 1, 1 << 20) == -4
    assert L.sz_set_grid_output(tile.h, 0, 5, 10, 7, capi.ptr(xg), capi.ptr(yg), 2, capi.ptr(codes, capi._ip), 4) == -4
    # set and turned off again: the path and the state of a fresh world
    off = _world(cfg)
    off.set_floe_output(0, 5)
    off.set_grid_output(1, 7, *g)
    off.set_floe_output(0, 0)
    off.set_grid_output(1, 0)
    fresh = _world(cfg)
    assert off.run(8, 0, dt, coupling_dt=1) == fresh.run(8, 0, dt, coupling_dt=1) == 8
    assert off.pipelined() and fresh.pipelined() and off.narrow_kernel_name() == fresh.narrow_kernel_name()
    assert off.output_frames() == ([0] * 4, [0] * 4, False)
    _assert_bit_equal(_state(off), _state(fresh), "recorder off")

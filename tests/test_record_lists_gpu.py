"""The lists of a floe frame (csrc/sz_record.hpp, "THE LISTS"): floe.interactions and the sub-floe points recorded on the device
against the same batch cut by hand -- interactions() BEFORE add_ghosts, then add_ghosts, the columns, subpoints() -- through the rule of
tests/record_lists_ref.py; against the CPU oracle's list behind add_ghosts!; and a fresh World restarted from a frame.  Same kernels on the
same state: every comparison with the hand cut is bit for bit.

The fields are the 300-floe fields of tests/test_record_gpu.py (periodic: ghosts, partners that were ghosts of the step before; between walls
with topography: boundary and topography partners, no ghosts).  The tests assert that the fields still exercise those paths."""
import ctypes as C

import numpy as np
import pytest

import parity
import record_lists_ref as ref
from test_batch_paths_gpu import N_FLOES
from test_record_gpu import KINDS, _assert_frame_is_hand_cut, _by_hand, _cfg, _same, _tsteps, _world
from test_ridgeraft_gpu import _assert_bit_equal, _state

pytestmark = pytest.mark.gpu

LISTS = ["interactions", "subpoints"]
LIST_KEYS = ("inter_off", "inter_rows", "sub_off", "sx", "sy")
OUT_STEPS = (5, 10, 15, 20, 25)
E_ARG, E_STATE = -2, -4


def _lists_info(w, writer, k):
    tot = [C.c_int64(0), C.c_int64(0)]
    assert w.L.sz_floe_frame_lists_info(w.h, writer, k, *(C.byref(v) for v in tot)) == 0
    return tot[0].value, tot[1].value


@pytest.fixture(scope="module", params=list(KINDS))
def recorded_and_hand_cut(request):
    """World A: one recorded run(24, 3) with both lists; World C: the same with no lists; World B: the batch cut by hand at the output steps"""
    kind = request.param
    cfg = _cfg(kind)
    dt = cfg["dt"]
    A = _world(cfg)
    A.set_floe_output(0, 5, lists=LISTS)
    done = A.run(24, 3, dt, coupling_dt=1)
    pipelined = A.pipelined()
    Cw = _world(cfg)
    Cw.set_floe_output(0, 5)
    assert Cw.run(24, 3, dt, coupling_dt=1) == 24
    B = _world(cfg)
    t, hand = 3, {}
    for s in OUT_STEPS:
        assert B.run(s - t, t, dt, coupling_dt=1) == s - t
        t = s
        io, ir = B.interactions()          # (before add_ghosts, which forgets how the last step's ghosts were numbered)
        io, ir = io.copy(), ir.copy()
        fl = _by_hand(B)
        so, sx, sy = B.subpoints()
        hand[s] = (fl, (io, ir), (so.copy(), sx.copy(), sy.copy()))
        B.remove_ghosts()
    assert B.run(27 - t, t, dt, coupling_dt=1) == 27 - t
    frames = [A.floe_frame(0, k) for k in range(A.output_frames()[0][0])]
    return kind, cfg, A, B, Cw, done, pipelined, hand, frames


def test_recorded_lists_are_the_batch_cut_by_hand(recorded_and_hand_cut):
    kind, cfg, A, B, Cw, done, pipelined, hand, frames = recorded_and_hand_cut
    assert done == 24 and pipelined
    assert A.output_frames() == ([5, 0, 0, 0], [0] * 4, False) and Cw.output_frames() == ([5, 0, 0, 0], [0] * 4, False)
    for k, s in enumerate(OUT_STEPS):
        fr = frames[k]
        fl, (io, ir), (so, sx, sy) = hand[s]
        M, N = fr["M"], fr["N"]
        assert fr["tstep"] == s and N == N_FLOES and (M > N) == (kind == "periodic")
        # the interactions: the parents' rows to the bit, nothing on a ghost row
        assert len(io) == N + 1 and _same(fr["inter_off"][:N + 1], io), (kind, s)
        assert np.all(fr["inter_off"][N:] == io[N]), (kind, s)
        assert _same(fr["inter_rows"], ir[:io[N]].reshape(-1, 7)), (kind, s)
        want = ref.inter_section(io, ir, N, M)
        assert _same(fr["inter_off"], want[0]) and _same(fr["inter_rows"], want[1]), (kind, s)
        assert _lists_info(A, 0, k) == (len(fr["inter_rows"]), len(fr["sx"]))
        # what the field must exercise
        idx = fr["inter_rows"][:, 0]
        assert np.any(np.diff(fr["inter_off"][:N + 1]) == 0), (kind, s, "no parent without rows")
        assert not np.any(idx > ref.GHOST_KEY_LIMIT), (kind, s, "a partner left as an order key")
        if kind == "periodic":
            assert np.any(idx > N), (kind, s, "no partner that was a ghost")
            assert np.all(idx[idx > N] <= N + 3 * N)
        else:
            assert np.any(idx < 0), (kind, s, "no boundary / topography partner")
        # the sub-floe points: the parents' own, a ghost row its parent's
        assert _same(fr["sub_off"][:N + 1], so) and _same(fr["sx"][:so[N]], sx) and _same(fr["sy"][:so[N]], sy), (kind, s)
        parent = ref.parents_of(fr["ghost_off"], fr["ghost_idx"], N, M)
        assert np.all(parent >= 0)
        wo, wx, wy = ref.sub_section(so, sx, sy, parent)
        assert _same(fr["sub_off"], wo) and _same(fr["sx"], wx) and _same(fr["sy"], wy), (kind, s)
        for g in range(N, M):
            a, b, p = fr["sub_off"][g], fr["sub_off"][g + 1], parent[g]
            assert _same(fr["sx"][a:b], sx[so[p]:so[p + 1]]) and _same(fr["sy"][a:b], sy[so[p]:so[p + 1]]), (kind, s, g)
        # the fixed columns: as without lists
        cols = {n: v for n, v in fr.items() if n not in LIST_KEYS}
        _assert_frame_is_hand_cut(cols, fl, (kind, "floe frame", s))
        plain = Cw.floe_frame(0, k)
        assert sorted(plain) == sorted(cols)
        assert all(_same(plain[n], cols[n]) for n in plain if n not in ("tstep", "M", "N")) and plain["tstep"] == s, (kind, s)
    sa = _state(A)
    _assert_bit_equal(sa, _state(B), (kind, "final state against the hand cut"))
    _assert_bit_equal(sa, _state(Cw), (kind, "final state against the run without lists"))


class _FrameAsWorld:
    """a frame's interactions behind the interface parity.compare_interactions reads"""

    def __init__(self, fr):
        self.fr = fr

    def interactions(self):
        return self.fr["inter_off"], self.fr["inter_rows"]


def test_frames_against_the_oracle(recorded_and_hand_cut):
    """steps 5 and 10 of the periodic field: row counts and partner numbers of the frame equal the oracle's list behind add_ghosts! exactly,
    the values hold to parity.compare_interactions' rule at rtol = 1e-10 (the figure the resident steps are held to); ghost spans are empty on
    both sides"""
    kind, cfg, A, B, Cw, done, pipelined, hand, frames = recorded_and_hand_cut
    if kind != "periodic":
        return
    from subzero_jl_amd import fields
    from oracle import orc
    ow = fields.build_world(orc.World(), cfg)
    t = 3
    for k, s in ((0, 5), (1, 10)):
        for q in range(t, s):
            ow.timestep_sim(q, cfg["dt"], coupling_dt=1)
        t = s
        ow.add_ghosts()
        fr = frames[k]
        ooff, orows = ow.interactions()
        assert ow.M == fr["M"] and fr["M"] > fr["N"]
        assert np.all(np.diff(ooff[N_FLOES:]) == 0) and np.all(np.diff(fr["inter_off"][N_FLOES:]) == 0)
        assert np.array_equal(fr["inter_off"], ooff), s
        assert np.array_equal(fr["inter_rows"][:, 0], orows[:, 0]), s
        assert np.any(orows[:, 0] > N_FLOES)
        errs = parity.compare_interactions(_FrameAsWorld(fr), ow, 1e-10)
        print("step", s, "worst ratios", errs)
        ow.remove_ghosts(N_FLOES)


def test_restart_from_a_frame(recorded_and_hand_cut):
    """the parents of frame 3 (step 20) -- columns, sub-floe points, interactions -- loaded into a fresh World: run(7, 20) gives A's final state"""
    kind, cfg, A, B, Cw, done, pipelined, hand, frames = recorded_and_hand_cut
    fr = frames[3]
    N = fr["N"]
    assert fr["tstep"] == 20
    V, S = fr["vert_off"][N], fr["sub_off"][N]
    c = {}
    for n, v in fr.items():
        if n in LIST_KEYS or n in ("tstep", "M", "N", "ghost_off", "ghost_idx"):
            continue
        c[n] = v[:N + 1].copy() if n == "vert_off" else v[:V].copy() if n in ("vx", "vy") else v[:N].copy()
    H = _world(cfg)
    H.load_columns(c)
    H.set_subpoints_csr(fr["sub_off"][:N + 1], fr["sx"][:S], fr["sy"][:S])
    io, ir = fr["inter_off"], fr["inter_rows"]
    for i in range(N):
        if io[i + 1] > io[i]:
            H.set_interactions(i, ir[io[i]:io[i + 1]])
    H._push_interactions()
    assert H.run(7, 20, cfg["dt"], coupling_dt=1) == 7
    _assert_bit_equal(_state(A), _state(H), (kind, "restarted from the frame of step 20"))


def test_rows_the_host_gave_are_kept_as_they_are():
    cfg = _cfg("periodic")
    w = _world(cfg)
    w.set_floe_output(0, 1, ["cx", "id"], lists=["interactions"])
    N = N_FLOES
    w.set_interactions(0, [[N + 3, 1.5, -2.5, 100.0, 200.0, 3.25, 10.0], [5, 0.5, 0.25, 1.0, 2.0, -4.0, 7.0]])
    w.set_interactions(2, [[-2, 9.0, 8.0, 7.0, 6.0, 5.0, 4.0]])
    w.set_interactions(7, [[N + 1, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], [N + 40, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0], [9, 0.125, 0.0, 0.0, 0.0, 0.0, 1.0]])
    w._push_interactions()
    off, rows = w.interactions()
    off, rows = off.copy(), rows.copy()
    assert off[N] == 6 and rows[0, 0] == N + 3 and rows[2, 0] == -2
    assert w.run(1, 0, cfg["dt"], coupling_dt=1) == 1
    fr = w.floe_frame(0, 0)
    assert fr["tstep"] == 0 and fr["N"] == N and fr["M"] > N
    assert _same(fr["inter_off"][:N + 1], off[:N + 1]) and np.all(fr["inter_off"][N:] == 6)
    assert _same(fr["inter_rows"], rows.reshape(-1, 7))
    assert sorted(k for k in fr if k not in ("tstep", "M", "N")) == ["cx", "id", "inter_off", "inter_rows"]


def test_room_counts_the_lists():
    """an arena of exactly two frames by World.frame_bytes: the third output step is not taken (and the Python layout mirror is the library's)"""
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    p = _world(cfg)
    mask = p.frame_mask(None)
    p.set_floe_output(0, 3, lists=LISTS)
    assert p.run(12, 0, dt, coupling_dt=1) == 12 and _tsteps(p) == [0, 3, 6, 9]
    sizes, plain = [], []
    for k in range(4):
        info = [C.c_int64(0) for _ in range(5)]
        assert p.L.sz_floe_frame_info(p.h, 0, k, *(C.byref(v) for v in info)) == 0
        t, M, N, V, G = (v.value for v in info)
        R, S = _lists_info(p, 0, k)
        assert S > 0 and (R > 0) == (k > 0)
        sizes.append(p.frame_bytes(mask, M, N, V, LISTS, R, S))
        plain.append(p.frame_bytes(mask, M, N, V))
        assert sizes[-1] == plain[-1] + 2 * ((4 * (M + 1) + 7) // 8 * 8) + 56 * R + 16 * S
    q = _world(cfg)
    q.set_floe_output(0, 3, arena_bytes=sizes[0] + sizes[1], lists=LISTS)
    assert q.run(12, 0, dt, coupling_dt=1) == 6 and _tsteps(q) == [0, 3] and q.output_frames()[2]
    for k in range(2):
        a, b = q.floe_frame(0, k), p.floe_frame(0, k)
        assert sorted(a) == sorted(b) and all(_same(a[n], b[n]) for n in a if n not in ("tstep", "M", "N"))
    q.clear_frames()
    assert q.run(3, 6, dt, coupling_dt=1) == 3 and _tsteps(q) == [6] and not q.output_frames()[2]
    # one byte less and the second frame finds no room
    r = _world(cfg)
    r.set_floe_output(0, 3, arena_bytes=sizes[0] + sizes[1] - 1, lists=LISTS)
    assert r.run(12, 0, dt, coupling_dt=1) == 3 and _tsteps(r) == [0] and r.output_frames()[2]


def test_refusals_and_unchanged_defaults():
    from subzero_jl_amd import capi, tiles
    cfg = _cfg("periodic")
    dt = cfg["dt"]
    w = _world(cfg)
    L, h = w.L, w.h
    w._push()
    assert L.sz_set_floe_output_lists(h, 0, 1) == E_STATE          # the writer is off
    w.set_floe_output(0, 1, ["cx", "rings"])
    assert L.sz_set_floe_output_lists(h, 0, 4) == E_ARG and L.sz_set_floe_output_lists(h, 0, 7) == E_ARG
    assert L.sz_set_floe_output_lists(h, 4, 1) == E_ARG and L.sz_set_floe_output_lists(h, -1, 1) == E_ARG
    assert L.sz_set_floe_output_lists(h, 1, 1) == E_STATE
    with pytest.raises(capi.SzError):
        w.set_floe_output(0, 1, ["cx"], lists=["fuse_idx"])
    # a writer without lists: today's frame, today's refusals
    w.set_floe_output(0, 1, ["cx", "rings"])
    assert w.run(1, 0, dt, coupling_dt=1) == 1
    assert sorted(k for k in w.floe_frame(0, 0) if k not in ("tstep", "M", "N")) == ["cx", "vert_off", "vx", "vy"]
    for member in ("sx", "sub_off", "inter_off", "inter_rows"):
        with pytest.raises(capi.SzError):
            w.floe_frame(0, 0, members=["cx", member])
    assert _lists_info(w, 0, 0) == (0, 0)
    off = np.zeros(w.floe_frame(0, 0)["M"] + 1, np.int32)
    assert L.sz_download_floe_frame_interactions(h, 0, 0, capi.ptr(off, capi._ip), None) == E_ARG
    assert L.sz_download_floe_frame_interactions(h, 0, 1, capi.ptr(off, capi._ip), None) == E_ARG
    # the lists are set behind the writer, free its frames, and are reset by setting the writer again
    assert L.sz_set_floe_output_lists(h, 0, 2) == 0 and w.output_frames()[0][0] == 0
    w._floe_lists[0] = 2
    assert w.run(1, 1, dt, coupling_dt=1) == 1
    fr = w.floe_frame(0, 0)
    assert sorted(k for k in fr if k not in ("tstep", "M", "N")) == ["cx", "sub_off", "sx", "sy", "vert_off", "vx", "vy"] and fr["tstep"] == 1
    assert L.sz_download_floe_frame_interactions(h, 0, 0, capi.ptr(off, capi._ip), None) == E_ARG          # (only the points were asked for)
    w.set_floe_output(0, 1, ["cx", "rings"])
    assert w.run(1, 2, dt, coupling_dt=1) == 1
    assert _lists_info(w, 0, 0) == (0, 0)
    assert sorted(k for k in w.floe_frame(0, 0) if k not in ("tstep", "M", "N")) == ["cx", "vert_off", "vx", "vy"]
    with pytest.raises(capi.SzError):
        w.floe_frame(0, 0, members=["cx", "sx"])
    # tile frames record no lists yet: a tiled context and a writer of the tile setter refuse, and so does TiledWorld
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=3, drift_margin=3000.0)
    with pytest.raises(capi.SzError):
        tw.set_floe_output(0, 5, ["cx"], lists=["interactions"])
    th = tw.world.h
    assert L.sz_set_floe_output_lists(th, 0, 1) == E_STATE and "tile frames record no lists yet" in L.sz_last_error(th).decode()
    tw.set_floe_output(0, 5, ["cx"])
    assert L.sz_set_floe_output_lists(th, 0, 1) == E_STATE and "tile frames record no lists yet" in L.sz_last_error(th).decode()
    assert L.sz_set_floe_output_lists(th, 0, 8) == E_ARG

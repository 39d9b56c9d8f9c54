"""Ridge / raft candidates on the device (csrc/sz_ridgeraft.hpp): the table against the restatement of the rule
(tests/ridgeraft_ref.py, held to the reference's loop by tests/test_ridgeraft_cpu.py), resident batches that stop in the middle of a ridge /
raft step with candidates and run through the others, and batches ridge / raft must not perturb."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import parity
import ridgeraft_ref as rr

pytestmark = pytest.mark.gpu

TIE_REL = 1e-9           # a frac this close (relative) to a window edge, on either side, is a tie: the row contract against the oracle is 1e-10
TIE_CAP = 0.01           # ties: at most 1 % of the oracle's table
EDGES = (1e-6, 0.95)


def mk(**env):
    import subzero_jl_amd
    for k, v in env.items():
        os.environ[k] = v
    try:
        return subzero_jl_amd.World(0)
    finally:
        for k in env:
            del os.environ[k]


def _state(w, rows=True):
    """every column a step writes, rings, status; with rows: floe.interactions, the ghost lists and the fuse lists too"""
    from subzero_jl_amd import capi
    out = {n: w.get(n) for n in capi.DCOLS}
    for k in ("sa11", "sa12", "sa21", "sa22", "si11", "si12", "si21", "si22", "e11", "e12", "e21", "e22"):
        out[k] = w.get(k)
    off, x, y = w.rings()
    out["vert_off"], out["vx"], out["vy"] = off.copy(), x.copy(), y.copy()
    ids, gids, st = w.ids()
    out["id"], out["ghost_id"], out["status"] = ids, gids, st
    if rows:
        io, ir = w.interactions()
        out["inter_off"], out["inter_rows"] = io.copy(), ir.copy()
        out["ghosts"] = np.array([g for gl in w.ghosts() for g in [len(gl)] + list(gl)], np.int64)
        out["fuse"] = np.array([g for gl in w.fuse() for g in [len(gl)] + list(gl)], np.int64)
    return out


def _assert_bit_equal(a, b, where=""):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (where, k)


def _table(w):
    i, j, k, f, nd = w.ridgeraft_candidates()
    return list(zip(i.tolist(), j.tolist(), k.tolist(), f.tolist())), nd


def _assert_same_table(got, want, where=""):
    """entry for entry, in order, kind and frac as bits"""
    (gt, gd), (wt, wd) = got, want
    assert gd == wd, (where, "draws", gd, wd)
    assert [e[:3] for e in gt] == [e[:3] for e in wt], (where, len(gt), len(wt))
    assert np.array_equal(np.array([e[3] for e in gt]).view(np.uint64), np.array([e[3] for e in wt]).view(np.uint64)), (where, "frac")


def _set(w, **s):
    w.set_ridgeraft(True, **s)
    return w


# ---------------------------------------------------------------- 1. hand-made rows
HAND = dict(min_ridge_height=0.2, max_floe_ridge_height=5.0, max_domain_ridge_height=1.25, max_floe_raft_height=0.3, max_domain_raft_height=0.25)


def _square(cx, cy, side):
    h = side / 2
    return np.array([[cx - h, cy - h], [cx - h, cy + h], [cx + h, cy + h], [cx + h, cy - h], [cx - h, cy - h]])


def _overlap_for(frac, min_area):
    """an overlap whose quotient by min_area is `frac` to the bit"""
    o = frac * min_area
    for _ in range(64):
        q = o / min_area
        if q == frac:
            return o
        o = np.nextafter(o, np.inf if q < frac else -np.inf)
    raise AssertionError("no overlap gives that quotient")


def _hand_world():
    """17 floes in two clusters (every pair of a cluster passes potential_interaction) and two across the west wall, which get ghosts; N / S
    collision walls, E / W periodic walls, one topography square; rmax, heights and status set by hand so that every gate is met from both sides.  Returns the world after add_ghosts, before any rows."""
    from subzero_jl_amd import capi, floe as floe_mod
    up = lambda v: float(np.nextafter(v, np.inf))
    dn = lambda v: float(np.nextafter(v, -np.inf))
    w = mk()
    w.set_consts(); w.set_settings()
    w.set_domain([capi.COLLISION, capi.COLLISION, capi.PERIODIC, capi.PERIODIC], 0.0, 1e5, 0.0, 1e5)
    w.set_topography([_square(8e3, 8e3, 4e3)])
    rings = [_square(4.0e3 + 450.0 * (k % 4), 4.0e3 + 500.0 * (k // 4), 4e3 + 10.0 * k) for k in range(12)]
    rings += [_square(9.5e4 + 300.0 * (k % 2), 9.5e4 + 300.0 * (k // 2), 4e3 + 10.0 * k) for k in range(5)]
    rings += [_square(1.5e3, 3.0e4, 4e3), _square(1.5e3, 3.3e4, 4.1e3)]          # 17 / 18: their rings cross the periodic west wall
    off = np.zeros(len(rings) + 1, np.int32); off[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate(rings)
    height = np.array([0.2, 0.25, 0.3, 0.1, dn(0.2), 5.0, 0.25, up(5.0),          # 7: over every floe maximum (and it gets no rows)
                       0.25, 0.1, 1.25, up(0.3),                                  # 8 / 9: S inside / outside, 10 / 11: W inside / outside
                       up(0.25), 0.1, 0.1, 0.1, up(1.25), 0.25, 0.25])            # 12 / 13: N inside / outside, 14 / 15: E inside / outside, 16: N inside
    d = floe_mod.derive(off, xy[:, 0].copy(), xy[:, 1].copy(), height)
    rmax = d["rmax"].copy()
    cx, cy = d["cx"], d["cy"]
    rmax[8], rmax[9] = up(cy[8]), cy[9]                          # |cy - 0| < rmax: just inside, just outside (strict)
    rmax[10], rmax[11] = up(cx[10]), cx[11]
    rmax[12], rmax[13] = up(1e5 - cy[12]), 1e5 - cy[13]
    rmax[14], rmax[15] = up(1e5 - cx[14]), 1e5 - cx[15]
    rmax[16] = up(1e5 - cy[16])
    status = np.full(19, capi.ACTIVE, np.int32); status[6] = capi.FUSE
    w.load_columns(dict(cx=cx, cy=cy, rmax=rmax, area=d["area"], height=height, mass=d["mass"], moment=d["moment"], status=status,
                        vert_off=off, vx=xy[:, 0].copy(), vy=xy[:, 1].copy()))
    w.add_ghosts()
    return w


def _row(j, overlap):
    return [float(j), 0.0, 0.0, 0.0, 0.0, 0.0, float(overlap)]


def test_hand_made_rows_exact():
    w = _set(_hand_world(), dt=10, **HAND)
    M, N = w.M, 19
    assert M == N + 2, "the two floes across the west wall have one ghost each"
    area = w.get("area")
    ma = lambda i, j: min(area[i], area[j])
    up = lambda v: float(np.nextafter(v, np.inf))
    dn = lambda v: float(np.nextafter(v, -np.inf))
    special = {(0, 1): 1e-6, (0, 2): up(1e-6), (0, 3): 0.95, (0, 4): dn(0.95)}
    rows = {}
    for i in range(7):                                           # (7 has no rows)
        rows[i] = [_row(j + 1, _overlap_for(special.get((i, j), 0.01 + 0.001 * j), ma(i, j))) for j in range(i + 1, 12)]
    rows[1] = [_row(4, 2.0 * ma(1, 3))] + rows[1] + [_row(4, 0.03 * ma(1, 3))]          # three rows for j = 4: too large, passing, a duplicate
    rows[2].append(_row(-5, 0.01 * area[2]))                     # the topography square
    rows[3].append(_row(-6, 0.01 * area[3]))                     # a topography element that does not exist
    rows[5].insert(0, _row(3, 0.01 * ma(5, 2)))                  # i > j
    for i, j in ((8, -2), (9, -2), (10, -4), (11, -4), (12, -1), (13, -1), (14, -3), (15, -3), (16, -1)):
        rows[i] = [_row(j, 0.02 * area[i])]
    rows[0].append(_row(-4, 0.02 * area[0]))                     # (not within rmax of the west wall)
    for g in range(N, M):                                        # ghost rows: a wall, and the next ghost where there is one
        rows[g] = [_row(-3, 0.02 * area[g]), _row(-4, 0.02 * area[g])] + ([_row(g + 2, 0.05 * ma(g, g + 1))] if g + 1 < M else [])
    for i, r in rows.items():
        w.set_interactions(i, np.array(r))
    got = _table(w)
    want = rr.table(w, HAND, [_square(8e3, 8e3, 4e3)])
    _assert_same_table(got, want, "hand-made rows")
    tab = {(i, j): (k, f) for i, j, k, f in got[0]}          # (j as the rows name it: 1-based)
    assert len(tab) == len(got[0]) > 32, "the table does not outgrow its first arrays"
    both = rr.RIDGE | rr.RAFT
    # the window is open at both ends
    assert (0, 2) not in tab and (0, 4) not in tab and tab[(0, 3)][1] == up(1e-6) and tab[(0, 5)][1] == dn(0.95)
    assert tab[(1, 4)][1] == 0.01 + 0.001 * 3                              # three rows for one j: the first PASSING row, once
    assert not any(j == 7 for _, j in tab) and not any(i == 6 for i, _ in tab)          # a partner tagged fuse; a floe that is not active
    assert (5, 3) not in tab and not any(i == 7 for i, _ in tab)          # i > j; a floe without rows
    assert tab[(2, -5)][0] == rr.RIDGE and (3, -6) not in tab              # the topography square; an element that does not exist
    # heights on the thresholds (inclusive): min_ridge_height 0.2, max_floe_ridge_height 5.0, max_floe_raft_height 0.3
    assert tab[(0, 5)][0] == both and tab[(3, 5)][0] == rr.RAFT            # 0.2 with 0.2 - ulp; 0.1 with 0.2 - ulp: neither can ridge
    assert tab[(3, 6)][0] == rr.RIDGE and (3, 8) not in tab                # 0.1 with 5.0; with 5.0 + ulp
    assert tab[(1, 3)][0] == both and tab[(1, 12)][0] == rr.RIDGE          # 0.25 with 0.3; with 0.3 + ulp
    # the walls: strict < against rmax; the domain maxima 1.25 / 0.25 are inclusive
    assert tab[(8, -2)][0] == both and (9, -2) not in tab and (0, -4) not in tab
    assert tab[(10, -4)][0] == rr.RIDGE and (11, -4) not in tab
    assert tab[(12, -1)][0] == rr.RIDGE and (13, -1) not in tab
    assert tab[(14, -3)][0] == both and (15, -3) not in tab
    assert (16, -1) not in tab                                             # inside, but one ulp over max_domain_ridge_height
    assert any(i >= N for i, _ in tab), "no entry of a ghost row"
    assert got[1] == rr.n_draws(w.get("height"), HAND)
    _assert_same_table(_table(w), got, "two calls")


# ---------------------------------------------------------------- 2. field parity with the oracle
def _field_cfg(name):
    from subzero_jl_amd import fields
    if name == "star":
        return fields.make_config(n_floes=2000, seed=7, subgrid_per_floe=4.0)
    cfg = fields.make_config(n_floes=1500, seed=7, subgrid_per_floe=4.0, shape="voronoi", walls=True)
    L = cfg["L"]
    cfg["topography"] = [_square(0.37 * L, 0.61 * L, 0.06 * L)]
    return cfg


def _field_heights(n):
    return np.random.default_rng(5).choice([0.1, 0.2, 0.25, 0.3, 1.0, 1.25, 2.0, 5.0, 6.0], n)


def _near_edge(f):
    return any(abs(f - e) <= TIE_REL * e for e in EDGES)


def _all_fracs(w, topo):
    """frac of every row that passes valid_interaction, by (i, j): what can tip over a window edge"""
    v = rr._View(w, topo)
    out = {}
    for i in range(v.M):
        for r in v.rows[v.off[i]:v.off[i + 1]]:
            j = int(r[0])
            if v.valid(i, j):
                out.setdefault((i, j), []).append(float(v.frac(i, j, r[6])))
    return out


@pytest.mark.parametrize("name", ["star", "voronoi"])
def test_field_parity(name):
    """30 resident steps, then add_ghosts + timestep_collisions on the engine and on the oracle restarted from the engine's state: the draws are
    equal, and the tables are equal as sets of (i, j, kind) outside ties.  Checked on the CPU (the oracle's own 30 steps of these seeds, heights
    as here): star 2 193 rows that pass valid_interaction (1 644 table entries), voronoi 2 015 (1 571 entries, 16 floes tagged by the
    topography), none within a relative 1e-9 of a window edge -- the nearest lie a relative 0.82 (star) and 2.5e-2 (voronoi) away, so no tie
    is expected on either side."""
    from subzero_jl_amd import fields
    cfg = _field_cfg(name)
    topo = cfg["topography"]
    hw = fields.build_world(mk(), cfg)
    assert hw.run(30, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 30
    ow = parity.oracle_from(hw, cfg)
    hs = _field_heights(cfg["n_floes"])
    n = cfg["n_floes"]
    for w in (hw, ow):
        w.set("height", hs)
        w.add_ghosts()
        w.timestep_collisions(n, cfg["dt"])
    assert hw.M == ow.M
    hw.set_ridgeraft(True, dt=10)
    got, gd = _table(hw)
    want, wd = rr.table(ow, rr.SETTINGS, topo)
    assert gd == wd == rr.n_draws(ow.get("height"), rr.SETTINGS)
    hf, of = _all_fracs(hw, topo), _all_fracs(ow, topo)
    ties = {p for p in set(hf) | set(of) if any(_near_edge(f) for f in hf.get(p, []) + of.get(p, []))}
    gs = {(i, j, k) for i, j, k, _ in got if (i, j) not in ties}
    ws = {(i, j, k) for i, j, k, _ in want if (i, j) not in ties}
    print(f"ridge/raft field parity {name}: {len(want)} oracle entries, {len(got)} device entries, {len(ties)} ties, {gd} draws over {hw.M} rows")
    assert gs == ws, sorted(gs ^ ws)[:5]
    assert len(want) > 100, "the field does not exercise the table"
    assert len(ties) <= TIE_CAP * len(want)
    # the device against the rule on its OWN rows: entry for entry, to the bit
    _assert_same_table((got, gd), rr.table(hw, rr.SETTINGS, topo), name)


# ---------------------------------------------------------------- 3. the stop, 5. a host edit
def _dense(seed=7, n=400):
    from subzero_jl_amd import fields
    return fields.make_config(n_floes=n, seed=seed, subgrid_per_floe=4.0)


def _stopped(cfg):
    """a batch of 40 from tstep 1 with dt = 10, stopped before the second half of tstep 10"""
    from subzero_jl_amd import fields
    A = _set(fields.build_world(mk(), cfg), dt=10)
    assert A.run(40, 1, cfg["dt"], coupling_dt=1) == 9
    assert A.ridgeraft_pending() == 10
    return A


def _by_hand(cfg):
    """9 steps, then add_ghosts + timestep_collisions by hand; ridge / raft never set"""
    from subzero_jl_amd import fields
    B = fields.build_world(mk(), cfg)
    assert B.run(9, 1, cfg["dt"], coupling_dt=1) == 9
    B.add_ghosts(); B.timestep_collisions(cfg["n_floes"], cfg["dt"])
    return B


def test_stop_in_the_middle_of_the_step():
    cfg = _dense()
    A, B = _stopped(cfg), _by_hand(cfg)
    assert A.M == B.M > cfg["n_floes"]
    _assert_bit_equal(_state(A), _state(B), "pending")
    t1 = _table(A)
    assert len(t1[0]) > 0 and t1[1] == rr.n_draws(A.get("height"), rr.SETTINGS)
    _assert_same_table(t1, rr.table(A, rr.SETTINGS, None), "the table that ended the batch")
    B.set_ridgeraft(True, dt=10)
    _assert_same_table(_table(B), t1, "by hand")
    done = C.c_int32(7)
    from subzero_jl_amd import capi
    assert A.L.sz_step(A.h, 5, 10, cfg["dt"], 1, capi.COLLISIONS_ON | capi.COUPLING_ON, C.byref(done)) == -4 and done.value == 0
    assert b"sz_step_finish" in A.L.sz_last_error(A.h)
    A.finish_step(10, cfg["dt"], coupling_dt=1)
    assert A.ridgeraft_pending() == -1
    B.set_ridgeraft(False)
    B.remove_ghosts(); B.timestep_coupling(); B.timestep_floe_properties(cfg["dt"])
    assert A.M == cfg["n_floes"]
    _assert_bit_equal(_state(A), _state(B), "finished")
    assert A.run(5, 11, cfg["dt"], coupling_dt=1) == 5
    assert B.run(5, 11, cfg["dt"], coupling_dt=1) == 5
    _assert_bit_equal(_state(A, rows=False), _state(B, rows=False), "on from tstep 11")


def _edit_and_upload(w, n, k):
    """at a pending stop: the parents and their rows come down, parent k gains volume as add_floe_volume! would give it, the parents go up alone"""
    from subzero_jl_amd import capi
    w._pull()
    off, rows = w.interactions()
    col = w.col
    cols = {c: col[c][:n].copy() for c in capi.DCOLS + capi.TCOLS + ["id", "ghost_id", "status"]}
    vo = col["vert_off"]
    cols.update(vert_off=vo[:n + 1].copy(), vx=col["vx"][:vo[n]].copy(), vy=col["vy"][:vo[n]].copy())
    vol = 0.05 * cols["area"][k] * cols["height"][k]
    cols["height"][k] = (cols["height"][k] * cols["area"][k] + vol) / cols["area"][k]
    cols["mass"][k] = cols["area"][k] * cols["height"][k] * 920.0
    sub = w.subpoints()
    w.load_columns(cols)
    w.set_subpoints_csr(*sub)
    for i in range(n):
        w.set_interactions(i, rows[off[i]:off[i + 1]])


def test_host_edit_at_a_pending_stop():
    cfg = _dense()
    n = cfg["n_floes"]
    A, B = _stopped(cfg), _by_hand(cfg)
    k = next(i for i, _, _, _ in _table(A)[0] if i < n)
    _edit_and_upload(A, n, k)
    A.finish_step(10, cfg["dt"], coupling_dt=1)
    _edit_and_upload(B, n, k)
    B._push_interactions()
    B.timestep_coupling(); B.timestep_floe_properties(cfg["dt"])
    _assert_bit_equal(_state(A, rows=False), _state(B, rows=False), "edited")
    C0 = _by_hand(cfg)
    C0.remove_ghosts(); C0.timestep_coupling(); C0.timestep_floe_properties(cfg["dt"])
    assert A.get("height")[k] != C0.get("height")[k] and A.get("u")[k] != C0.get("u")[k], "the step did not use the uploaded values"


# ---------------------------------------------------------------- 4. run-through
RUN_THROUGH = {"sparse": (dict(concentration=0.1), None), "too_thick": ({}, 6.0)}


@pytest.mark.parametrize("name", list(RUN_THROUGH))
def test_run_through_empty_tables(name):
    """45 steps from tstep 1 with dt = 10 in one call; against a context that makes tsteps 10, 20, 30, 40 by hand through the process calls and
    the rest by batches, bit for bit; each hand-made step against the oracle restarted from the engine's state, to the 1e-10 step contract.
    (A split step is NOT asserted bit-equal to a resident three-launch step: DESIGN.md §9e.)"""
    from subzero_jl_amd import fields
    over, h = RUN_THROUGH[name]
    cfg = fields.make_config(n_floes=400, seed=11, subgrid_per_floe=4.0, **over)
    if h is not None:
        cfg["height"] = np.full(cfg["n_floes"], h)
        from subzero_jl_amd import floe as floe_mod
        cfg["derived"] = floe_mod.derive(cfg["vert_off"], cfg["vx"], cfg["vy"], cfg["height"])
    n, dt = cfg["n_floes"], cfg["dt"]
    A = _set(fields.build_world(mk(), cfg), dt=10)
    assert A.run(45, 1, dt, coupling_dt=1) == 45
    assert A.ridgeraft_pending() == -1
    B = fields.build_world(mk(), cfg)
    draws, t = 0, 1
    while t <= 45:
        if t % 10 == 0:
            ow = parity.oracle_from(B, cfg)
            B.add_ghosts(); B.timestep_collisions(n, dt)
            B.set_ridgeraft(True, dt=10)
            tab, nd = _table(B)
            B.set_ridgeraft(False)
            assert tab == []
            draws += nd
            ow.add_ghosts(); ow.timestep_collisions(n, dt)
            parity.compare_pairs(B, ow)
            B.remove_ghosts(); B.timestep_coupling(); B.timestep_floe_properties(dt)
            ow.remove_ghosts(n); ow.timestep_coupling(); ow.timestep_floe_properties(dt)
            parity.compare_worlds(B, ow, rtol=1e-10, check_pairs=False)
            t += 1
        else:
            k = min(10 - t % 10, 46 - t)
            assert B.run(k, t, dt, coupling_dt=1) == k
            t += k
    assert A.ridgeraft_draws() == draws == (0 if name == "too_thick" else 8 * n)
    _assert_bit_equal(_state(A, rows=False), _state(B, rows=False), name)
    if name == "too_thick":
        assert np.count_nonzero(A.get("overarea")) > n // 4, "the dense field is not in contact"
    assert A.run(3, 46, dt, coupling_dt=1) == 3 and A.ridgeraft_draws() == 0


# ---------------------------------------------------------------- 6. order with the other stops
def _thick(cfg):
    from subzero_jl_amd import floe as floe_mod
    cfg["height"] = np.full(cfg["n_floes"], 6.0)
    cfg["derived"] = floe_mod.derive(cfg["vert_off"], cfg["vx"], cfg["vy"], cfg["height"])
    return cfg


def test_fracture_candidate_on_an_empty_ridge_raft_step_ends_the_batch():
    from subzero_jl_amd import capi, fields
    cfg = _thick(_dense())
    out = []
    for rr_on in (False, True):
        w = fields.build_world(mk(), cfg)
        w.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=1.0, min_floe_area=1e6)
        assert w.run(4, 1, cfg["dt"], coupling_dt=1) == 4
        if rr_on:
            w.set_ridgeraft(True, dt=5)
        out.append((w.run(20, 5, cfg["dt"], coupling_dt=1), len(w.fracture_candidates()), w.ridgeraft_pending()))
    assert out[0][0] == out[1][0] == 1 and out[1][1] == out[0][1] > 0 and out[1][2] == -1, out


def test_tag_on_an_empty_ridge_raft_step_ends_the_batch():
    from subzero_jl_amd import capi, fields
    cfg = _thick(cases.floe_onto_island(fields.make_config(n_floes=400, seed=3, walls=True, topography=True, ocean="strait", subgrid_per_floe=4.0)))
    out = []
    for rr_on in (False, True):
        w = fields.build_world(mk(), cfg)
        if rr_on:
            w.set_ridgeraft(True, dt=5)
        done = w.run(20, 5, cfg["dt"], coupling_dt=1)
        out.append((done, w.ids()[2].copy(), w.ridgeraft_pending(), w.ridgeraft_draws()))
    assert out[0][0] == out[1][0] == 1, (out[0][0], out[1][0])
    assert np.array_equal(out[0][1], out[1][1]) and out[1][1][0] == capi.REMOVE
    assert out[1][2] == -1 and out[1][3] == 0


# ---------------------------------------------------------------- 7. off means off
def test_off_means_off():
    from subzero_jl_amd import fields
    cfg = _dense()

    def run(setup, **kw):
        w = fields.build_world(mk(), cfg)
        setup(w)
        w.profile(True)
        assert w.run(40, 1, cfg["dt"], coupling_dt=1, **kw) == 40
        return _state(w), {k: v[1] for k, v in w.kernel_times().items()}, w.pipelined()
    never = run(lambda w: None)
    off = run(lambda w: (w.set_ridgeraft(True, dt=10), w.set_ridgeraft(False)))
    _assert_bit_equal(never[0], off[0], "set_ridgeraft(on=False)")
    assert never[1] == off[1] and never[2] == off[2]
    never2 = run(lambda w: None, stop_on_tags=False)
    through = run(lambda w: w.set_ridgeraft(True, dt=10), stop_on_tags=False)
    _assert_bit_equal(never2[0], through[0], "SZ_NO_STOP")
    assert never2[1] == through[1] and never2[2] == through[2]


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    from subzero_jl_amd import capi, fields
    E_ARG, E_STATE = -2, -4
    cfg = fields.make_config(n_floes=400, seed=80, subgrid_per_floe=4.0)
    w = fields.build_world(mk(), cfg)
    w._push()
    L, h = w.L, w.h
    assert L.sz_set_ridgeraft(h, 1, 0, 0.2, 5.0, 1.25, 0.25, 0.25) == E_ARG
    assert L.sz_set_ridgeraft(h, 1, -3, 0.2, 5.0, 1.25, 0.25, 0.25) == E_ARG
    assert L.sz_set_ridgeraft(h, 0, 0, 0.2, 5.0, 1.25, 0.25, 0.25) == 0
    n = C.c_int32(0); nd = C.c_int64(0)
    assert L.sz_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)) == E_STATE          # not set
    w.set_ridgeraft(True, dt=10)
    assert L.sz_step_finish(h, 10, cfg["dt"], 1, capi.COLLISIONS_ON) == E_STATE                                 # nothing pending
    assert w.ridgeraft_pending() == -1
    assert L.sz_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)) == E_STATE          # a ghost-free list
    assert w.run(3, 1, cfg["dt"], coupling_dt=1) == 3
    assert L.sz_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)) == E_STATE          # ... after a batch too
    done = C.c_int32(0)
    assert L.sz_step(h, 3, 4, cfg["dt"], 1, capi.COUPLING_ON, C.byref(done)) == E_STATE                          # collisions off
    # a table larger than the room given
    w.add_ghosts(); w.timestep_collisions(cfg["n_floes"], cfg["dt"])
    assert L.sz_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)) == 0 and n.value > 1
    i1 = np.zeros(1, np.int32)
    assert L.sz_ridgeraft_candidates(h, C.byref(n), 1, capi.ptr(i1, capi._ip), None, None, None, None) == E_ARG
    w.remove_ghosts()
    # the context is still usable; a tiled context with ridge / raft set is refused
    assert w.run(2, 4, cfg["dt"], coupling_dt=1) == 2
    gidx = np.arange(w.N, dtype=np.int64)
    assert L.sz_tile_enable(h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    assert L.sz_tile_run(h, 4, 6, cfg["dt"], 1, capi.COLLISIONS_ON, C.byref(done)) == E_STATE
    assert b"ridge" in L.sz_last_error(h)
    assert L.sz_tile_step(h, None, 1, 0, 6, cfg["dt"], 1, capi.COLLISIONS_ON) == E_STATE
    assert L.sz_step(h, 4, 6, cfg["dt"], 1, capi.COLLISIONS_ON, C.byref(done)) == E_STATE
    assert L.sz_ridgeraft_candidates(h, C.byref(n), 0, None, None, None, None, C.byref(nd)) == E_STATE

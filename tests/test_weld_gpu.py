"""Welding overlaps on the device (csrc/sz_weld.hpp): bins and the overlap table against the restatement of the reference's loops
(tests/weld_ref.py, pinned by the reference's own test values), resident batches that end on the first welding step with an overlap, against
the oracle's trajectory, and batches welding must not perturb."""
import ctypes as C
import os

import numpy as np
import pytest

import parity
import weld_ref as wr

pytestmark = pytest.mark.gpu

AREA_REL = 1e-9          # |hip - ref| <= AREA_REL * min(area_i, area_j): the clip-area contract of DESIGN.md §9
TIE_CAP = 0.01           # pairs under that band on both sides (a sliver one clipper sees and the other may not): at most 1 % of the table


def mk(**env):
    import subzero_jl_amd
    for k, v in env.items():
        os.environ[k] = v
    try:
        return subzero_jl_amd.World(0)
    finally:
        for k in env:
            del os.environ[k]


def _state(w):
    """every column a step writes, rings included"""
    from subzero_jl_amd import capi
    out = {n: w.get(n) for n in capi.DCOLS}
    for k in ("sa11", "sa12", "sa21", "sa22", "si11", "si12", "si21", "si22", "e11", "e12", "e21", "e22"):
        out[k] = w.get(k)
    off, x, y = w.rings()
    out["vert_off"], out["vx"], out["vy"] = off.copy(), x.copy(), y.copy()
    out["status"] = w.ids()[2]
    return out


def _assert_bit_equal(a, b):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def _grid(g):
    gr = g["grid"]
    return gr["x0"], gr["xf"], gr["y0"], gr["yf"]


def _compare_tables(got, cand, areas, area, label, report=None):
    """the device's table (i, j, inter_area) against the reference's candidates with their areas.  Ties -- pairs whose larger inter_area of the
    two sides (0 where absent) is under AREA_REL * min(area_i, area_j) -- are left out of the set comparison; every other pair must be in both
    tables, in the same order, with areas to AREA_REL of the smaller floe."""
    gi, gj, ga = got
    hip = {(int(i), int(j)): float(a) for i, j, a in zip(gi, gj, ga)}
    assert len(hip) == len(gi), "a pair twice in the table"
    assert np.all(ga > 0), "an entry without area"
    ref = {(i, j): float(a) for (_, i, j), a in zip(cand, areas) if a > 0}
    cset = {(i, j) for _, i, j in cand}
    assert set(hip) <= cset, (label, "the table holds a pair that is no candidate", sorted(set(hip) - cset)[:5])
    band = lambda p: AREA_REL * min(area[p[0]], area[p[1]])
    ties = {p for p in set(hip) | set(ref) if max(hip.get(p, 0.0), ref.get(p, 0.0)) < band(p)}
    ref_order = [(i, j) for (_, i, j), a in zip(cand, areas) if a > 0 and (i, j) not in ties]
    hip_order = [(int(i), int(j)) for i, j in zip(gi, gj) if (int(i), int(j)) not in ties]
    assert hip_order == ref_order, (label, len(hip_order), len(ref_order), sorted(set(hip_order) ^ set(ref_order))[:5])
    worst = 0.0
    for p in ref_order:
        worst = max(worst, abs(hip[p] - ref[p]) / min(area[p[0]], area[p[1]]))
    print(f"weld table {label}: {len(ref)} reference entries of {len(cand)} candidates, {len(hip)} device entries, {len(ties)} ties, "
          f"max |hip - ref| / min(area) = {worst:.3e}")
    assert worst <= AREA_REL, (label, worst)
    assert len(ties) <= TIE_CAP * max(len(ref), 1), (label, len(ties), len(ref))
    if report is not None:
        report["worst"] = max(report.get("worst", 0.0), worst); report["ties"] = max(report.get("ties", 0), len(ties))
    return len(ties), worst


def test_bins_of_the_reference_floes():
    """test_welding.jl "Bin floes" on the device, bit-exact, and the break rule with the out-of-bounds floe in the middle of the list"""
    g = wr.golden()
    for case in g["bin_floes"]["cases"]:
        w = wr.golden_world(mk(), g, "bin_floes", case["domain"])
        b = w.weld_bins(case["nx"], case["ny"])
        for want in case["bins"]:
            k = (want["yidx"] - 1) * case["nx"] + (want["xidx"] - 1)
            assert (np.nonzero(b == k)[0] + 1).tolist() == want["members"], (case["domain"], case["nx"], case["ny"], want, b.tolist())
        assert int(np.sum(b >= 0)) == sum(x["nfloes"] for x in case["bins"])
    rings = g["bin_floes"]["rings"]
    g2 = dict(g, bin_floes=dict(g["bin_floes"], rings=rings[:3] + [rings[6]] + rings[3:6]))
    w = wr.golden_world(mk(), g2, "bin_floes", "open")
    assert w.weld_bins(2, 2).tolist() == [0, 2, 3, -1, -1, -1, -1]
    from oracle import orc
    ow = wr.golden_world(orc.World(), g2, "bin_floes", "open")
    assert wr.bins(ow, _grid(g), False, False, 2, 2).tolist() == [0, 2, 3, -1, -1, -1, -1]


def test_table_of_the_reference_floes():
    """test_welding.jl "Weld floes": the three rings overlap by 1e9 (1, 2) and 1e8 (1, 3)"""
    g = wr.golden()
    w = wr.golden_world(mk(), g, "weld_floes", g["weld_floes"]["domain"])
    area = w.get("area")

    def table(nx, ny, mx):
        i, j, a = w.weld_overlaps(nx, ny, mx)
        return list(zip(i.tolist(), j.tolist())), a
    p, a = table(1, 1, 1e10)
    assert p == [(0, 1), (0, 2)]
    assert abs(a[0] - 1e9) <= AREA_REL * min(area[0], area[1]) and abs(a[1] - 1e8) <= AREA_REL * min(area[0], area[2])
    p, a = table(1, 2, 1e10)
    assert p == [(0, 1)] and abs(a[0] - 1e9) <= AREA_REL * min(area[0], area[1])
    assert table(2, 2, 1e10)[0] == []
    assert table(1, 1, 2e9)[0] == []


def test_contained_floe_gives_the_smaller_area():
    from subzero_jl_amd import capi
    w = mk()
    w.set_domain([capi.OPEN] * 4, 0.0, 1e5, 0.0, 1e5)
    z = np.zeros((11, 11))
    w.set_grid_fields(10, 10, 0.0, 1e5, 0.0, 1e5, z, z, z, z, z)
    w.add_floe(np.array([[1e4, 1e4], [1.2e4, 6e4], [6.1e4, 6.3e4], [6e4, 1.1e4], [1e4, 1e4]]), 0.5)
    w.add_floe(np.array([[3e4, 3e4], [3.1e4, 4e4], [4.2e4, 4.1e4], [4e4, 3.05e4], [3e4, 3e4]]), 0.5)
    i, j, a = w.weld_overlaps(1, 1, 1e12)
    assert i.tolist() == [0] and j.tolist() == [1]
    assert abs(a[0] - w.get("area")[1]) <= AREA_REL * w.get("area")[1]


FIELDS = {"star": dict(n_floes=2000, seed=7, subgrid_per_floe=4.0), "voronoi": dict(n_floes=1500, seed=7, subgrid_per_floe=4.0, shape="voronoi")}


@pytest.mark.parametrize("name", ["star", "voronoi"])
def test_field_parity(name):
    """after 30 resident steps, against weld_ref on the oracle restarted from the engine's own state: bins and the candidate pair set bit-exact,
    inter_area to 1e-9 of the smaller floe, ties at most 1 % of the table, and the same bits on a second call"""
    from oracle import orc
    from subzero_jl_amd import fields
    cfg = fields.make_config(**FIELDS[name])
    hw = fields.build_world(mk(), cfg)
    assert hw.run(30, 0, cfg["dt"], coupling_dt=1) == 30
    ow = parity.oracle_from(hw, cfg)
    L = cfg["L"]
    grid = (0.0, L, 0.0, L)
    per_x, per_y = wr.periodic_flags(cfg["kinds"])
    area = ow.get("area")
    cache = {}

    def clip(a, b):
        key = (a.tobytes(), b.tobytes())
        if key not in cache:
            cache[key] = orc.clip(a, b)
        return cache[key]
    report = {}
    nonempty = 0
    for nx, ny in ((1, 1), (3, 2), (7, 5)):
        assert np.array_equal(hw.weld_bins(nx, ny), wr.bins(ow, grid, per_x, per_y, nx, ny)), (nx, ny)
        for mx in (1e300, float(np.median(area))):
            cand, areas = wr.overlaps(ow, grid, per_x, per_y, nx, ny, mx, clip=clip)
            got = hw.weld_overlaps(nx, ny, mx)
            assert hw.weld_candidate_pairs() == len(cand), (nx, ny, mx, hw.weld_candidate_pairs(), len(cand))
            _compare_tables(got, cand, areas, area, f"{name} ({nx}, {ny}) max_weld_area {mx:.3g}", report)
            again = hw.weld_overlaps(nx, ny, mx)
            for x, y in zip(got, again):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), "two calls, two tables"
            nonempty += len(got[0]) > 0
    assert nonempty >= 4, "the field does not exercise the table"
    print(f"weld field parity {name}: worst area deviation {report['worst']:.3e}, most ties in one table {report['ties']}")


# ---------------------------------------------------------------- batches
def _tip_and_wall(cx, cy, gap):
    """two floes on one line: a pentagon whose tip points east and, `gap` metres east of the tip, a quadrilateral with a long, slightly slanted
    west side -- the first overlap is the tip entering that side (a generic crossing: no collinear edges, no vertex on an edge)"""
    a = np.array([[cx - 1900.0, cy - 1500.0], [cx - 2100.0, cy + 1400.0], [cx + 300.0, cy + 1700.0], [cx + 2000.0, cy + 3.0],
                  [cx + 250.0, cy - 1650.0], [cx - 1900.0, cy - 1500.0]])
    x0 = cx + 2000.0 + gap
    b = np.array([[x0 - 20.0, cy - 1800.0], [x0 + 20.0, cy + 1750.0], [x0 + 3900.0, cy + 1500.0], [x0 + 4100.0, cy - 1600.0], [x0 - 20.0, cy - 1800.0]])
    return a, b


def _box_world(w, extra=None):
    """a few dozen floes at rest in a collision-walled box, far from one another, and one pair (the first two floes) closing at 0.5 m/s:
    10 m per 20 s step across a 125 m gap"""
    from subzero_jl_amd import capi
    L = 1.2e5
    w.set_consts()
    w.set_settings()
    w.set_domain([capi.COLLISION] * 4, 0.0, L, 0.0, L)
    z = np.zeros((13, 13))
    w.set_grid_fields(12, 12, 0.0, L, 0.0, L, z, z, z, z, z)
    a, b = _tip_and_wall(5.0e4, 6.1e4, 125.0) if extra is None else extra
    w.add_floe(a, 0.5); w.add_floe(b, 0.5)
    rng = np.random.default_rng(3)
    n = 2
    for gy in range(6):
        for gx in range(6):
            cx, cy = 1.5e4 + gx * 1.8e4, 1.5e4 + gy * 1.8e4
            if abs(cy - 6.1e4) < 1.2e4 and 3.0e4 < cx < 8.0e4:
                continue          # (room for the pair)
            th = ((2 * np.pi / 7) * (np.arange(7) + rng.uniform(-0.3, 0.3, 7)))[::-1]          # descending: clockwise, star-shaped about the centre
            r = 2500.0 * (0.7 + 0.3 * rng.uniform(0, 1, 7))
            ring = np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1)
            w.add_floe(np.concatenate([ring, ring[:1]]), 0.5)
            n += 1
    u = np.zeros(n)
    if extra is None:
        u[0], u[1] = 0.25, -0.25
    w.set("u", u)
    return w, L


def test_batch_stops_where_the_reference_would_first_weld():
    """dts = [5] from tstep 0: the pair is apart after tsteps 0, 5 and 10 and overlaps after tstep 15; run(40) returns after that step, with the
    oracle's state and the reference's table.  tfirst comes from the ORACLE's trajectory."""
    from oracle import orc
    dt = 20
    ow, L = _box_world(orc.World())
    grid = (0.0, L, 0.0, L)
    tfirst, seen = None, {}
    for t in range(40):
        ow.timestep_sim(t, dt, coupling_dt=1, coupling_on=False)
        assert np.all(ow.ids()[2] == wr.ACTIVE), f"a floe was tagged in tstep {t}"
        if t % 5 == 0:
            cand, areas = wr.overlaps(ow, grid, False, False, 1, 1, 2e9)
            seen[t] = float(areas.max()) if len(areas) else 0.0
            if np.any(areas > 0):
                tfirst = t
                break
    assert tfirst is not None and 10 < tfirst < 40, (tfirst, seen)
    area = ow.get("area")
    assert all(v == 0.0 for t, v in seen.items() if t < tfirst) and seen[tfirst] > 1e4 * wr_band(area), seen          # far above the tie band
    hw, _ = _box_world(mk())
    hw.set_welding([5], [1], [1], 2e9)
    done = hw.run(40, 0, dt, coupling_dt=1, coupling_on=False)
    assert done == tfirst + 1, (done, tfirst, seen)
    got = hw.weld_overlaps(1, 1, 2e9)
    assert len(got[0]) > 0
    _compare_tables(got, cand, areas, area, "box")
    parity.compare_worlds(hw, ow, rtol=1e-9)
    # the caller did not weld: the rest of the batch ends at the next welding step
    assert hw.run(40 - done, done, dt, coupling_dt=1, coupling_on=False) == 5


def wr_band(area):
    return AREA_REL * float(np.min(area))


def test_a_step_with_two_sets_takes_the_first():
    """dts = [6, 4], nxs = [1, 2]: two floes that overlap across the middle of the box share the bin of set 0 only; tstep 8 (set 1) finds nothing,
    tstep 12 is a step of both sets and uses set 0 (findfirst, simulation.jl:186-189)"""
    L = 1.2e5
    a = np.array([[5.2e4, 5.0e4], [5.3e4, 5.9e4], [6.05e4, 5.8e4], [6.1e4, 5.1e4], [5.2e4, 5.0e4]])          # centroid west of L / 2 = 6e4
    b = np.array([[5.95e4, 5.2e4], [6.0e4, 5.7e4], [6.8e4, 5.8e4], [6.9e4, 5.1e4], [5.95e4, 5.2e4]])         # ... east of it
    hw, _ = _box_world(mk(), extra=(a, b))
    cx = hw.get("cx")
    assert cx[0] < L / 2 < cx[1]
    assert len(hw.weld_overlaps(1, 1, 2e9)[0]) == 1 and len(hw.weld_overlaps(2, 1, 2e9)[0]) == 0
    hw.set_welding([6, 4], [1, 2], [1, 1], 2e9)
    assert hw.run(20, 7, 10, coupling_dt=1, coupling_on=False) == 6          # tsteps 7 .. 12
    assert len(hw.weld_overlaps(1, 1, 2e9)[0]) == 1
    assert np.all(hw.ids()[2] == wr.ACTIVE)


def _cfg(seed=7):
    from subzero_jl_amd import fields
    return fields.make_config(**dict(FIELDS["star"], seed=seed))


def test_welding_never_met_and_run_through_do_not_perturb():
    """welding set but never met (max_weld_area under every floe): 65 steps from tstep 0 with dts = [8], bit-equal to welding off, still on the
    two-launch steps; the same for a batch that runs through on the dense field"""
    from subzero_jl_amd import fields
    cfg = _cfg()
    off = fields.build_world(mk(), cfg)
    assert off.run(65, 0, cfg["dt"], coupling_dt=1) == 65 and off.pipelined()
    ref = _state(off)
    never = fields.build_world(mk(), cfg)
    never.set_welding([8], [1], [1], max_weld_area=0.5 * float(np.min(never.get("area"))))
    assert never.run(65, 0, cfg["dt"], coupling_dt=1) == 65
    assert never.pipelined()
    _assert_bit_equal(ref, _state(never))
    assert len(never.weld_overlaps(1, 1, 0.5 * float(np.min(never.get("area"))))[0]) == 0

    off2 = fields.build_world(mk(), cfg)
    assert off2.run(65, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 65 and off2.pipelined()
    met = fields.build_world(mk(), cfg)
    met.set_welding([8], [1], [1], 1e300)
    assert met.run(65, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 65
    assert met.pipelined()
    _assert_bit_equal(_state(off2), _state(met))
    assert len(met.weld_overlaps(1, 1, 1e300)[0]) > 0


def test_dense_field_stops_at_every_welding_step():
    from subzero_jl_amd import fields
    cfg = _cfg()
    hw = fields.build_world(mk(), cfg)
    hw.set_welding([8], [3], [2], 1e300)
    assert hw.run(40, 1, cfg["dt"], coupling_dt=1) == 8          # tsteps 1 .. 8
    t1 = hw.weld_overlaps(3, 2, 1e300)
    assert len(t1[0]) > 0 and np.all(hw.ids()[2] == wr.ACTIVE)
    assert hw.run(32, 9, cfg["dt"], coupling_dt=1) == 8          # the caller did not weld: tsteps 9 .. 16
    assert len(hw.weld_overlaps(3, 2, 1e300)[0]) > 0
    # welding off again: the batch runs to its end
    hw.set_welding([], [], [])
    assert hw.run(12, 17, cfg["dt"], coupling_dt=1) == 12


def test_refusals():
    from subzero_jl_amd import capi, fields
    E_ARG, E_STATE = -2, -4
    one = np.array([5], np.int32); zero = np.array([0], np.int32); neg = np.array([-5], np.int32)
    ip = lambda a: capi.ptr(a, capi._ip)
    n = C.c_int32(0)
    # no grid set
    w0 = mk()
    w0.set_domain([capi.OPEN] * 4, 0.0, 1e5, 0.0, 1e5)
    w0.add_floe(np.array([[1e4, 1e4], [1e4, 2e4], [2e4, 2e4], [2e4, 1e4], [1e4, 1e4]]), 0.5)
    w0._push()
    assert w0.L.sz_weld_overlaps(w0.h, 1, 1, 2e9, C.byref(n), 0, None, None, None) == E_STATE
    assert b"grid" in w0.L.sz_last_error(w0.h)
    cfg = fields.make_config(n_floes=400, seed=80, subgrid_per_floe=4.0)
    # no floes
    w1 = mk()
    assert w1.L.sz_weld_overlaps(w1.h, 1, 1, 2e9, C.byref(n), 0, None, None, None) == E_STATE
    w = fields.build_world(mk(), cfg)
    w._push()
    L, h = w.L, w.h
    assert L.sz_set_welding(h, 1, ip(zero), ip(one), ip(one), 2e9) == E_ARG
    assert L.sz_set_welding(h, 1, ip(neg), ip(one), ip(one), 2e9) == E_ARG
    assert L.sz_set_welding(h, 1, ip(one), ip(zero), ip(one), 2e9) == E_ARG
    assert L.sz_set_welding(h, 1, ip(one), ip(one), ip(zero), 2e9) == E_ARG
    assert L.sz_set_welding(h, 1, ip(one), ip(one), ip(one), 0.0) == E_ARG
    assert L.sz_set_welding(h, 1, ip(one), ip(one), ip(one), float("nan")) == E_ARG
    assert L.sz_set_welding(h, 1, None, ip(one), ip(one), 2e9) == E_ARG
    assert L.sz_set_welding(h, -1, ip(one), ip(one), ip(one), 2e9) == E_ARG
    assert L.sz_weld_overlaps(h, 0, 1, 2e9, C.byref(n), 0, None, None, None) == E_ARG
    assert L.sz_weld_overlaps(h, 1, 0, 2e9, C.byref(n), 0, None, None, None) == E_ARG
    assert L.sz_weld_overlaps(h, 1, 1, -1.0, C.byref(n), 0, None, None, None) == E_ARG
    b = np.zeros(w.N, np.int32)
    assert L.sz_debug_weld_bins(h, 0, 1, ip(b)) == E_ARG
    # a table larger than the room given
    assert L.sz_weld_overlaps(h, 1, 1, 1e300, C.byref(n), 0, None, None, None) == 0 and n.value > 1
    i1 = np.zeros(1, np.int32); a1 = np.zeros(1)
    assert L.sz_weld_overlaps(h, 1, 1, 1e300, C.byref(n), 1, ip(i1), ip(i1), capi.ptr(a1)) == E_ARG
    # the context is still usable
    assert w.run(4, 0, cfg["dt"], coupling_dt=1) == 4
    assert len(w.weld_overlaps(1, 1, 1e300)[0]) > 0
    # a tiled context with welding set
    gidx = np.arange(w.N, dtype=np.int64)
    assert L.sz_tile_enable(h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    w.set_welding([5], [1], [1])
    done = C.c_int32(0)
    assert L.sz_tile_run(h, 4, 0, cfg["dt"], 1, capi.COLLISIONS_ON, C.byref(done)) == E_STATE
    assert b"welding" in L.sz_last_error(h)
    assert L.sz_tile_step(h, None, 1, 0, 0, cfg["dt"], 1, capi.COLLISIONS_ON) == E_STATE
    assert L.sz_weld_overlaps(h, 1, 1, 2e9, C.byref(n), 0, None, None, None) == E_STATE

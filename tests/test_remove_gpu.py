"""Removal and dissolution on the device (csrc/sz_remove.hpp).  The yardstick throughout is the HOST REBUILD, which is what a resident run
did before: download the state, apply tests/remove_ref.py (remove_floes! restated), load the columns with their sub-floe points into a fresh
World (set_dissolved for the lattice), go on from there.  tests/test_shadow_gpu.py holds that a downloaded and re-uploaded state steps on bit
for bit; everything here is compared bit for bit."""
import numpy as np
import pytest

import cases
import remove_ref as rr

pytestmark = pytest.mark.gpu


def mk():
    import subzero_jl_amd
    return subzero_jl_amd.World(0)


def _build(w, cfg, extent=None):
    """fields.build_world; extent = (x0, xf, y0, yf): the domain and the grid over that box instead of [0, L]^2"""
    from subzero_jl_amd import fields
    fields.build_world(w, cfg)
    if extent is not None:
        x0, xf, y0, yf = extent
        w.set_domain([fields.KIND[k] for k in cfg["kinds"]], x0, xf, y0, yf)
        w.set_grid_fields(cfg["Nx"], cfg["Ny"], x0, xf, y0, yf, cfg["uo"], cfg["vo"], cfg["hf"], cfg["ua"], cfg["va"])
    return w


def _grid(cfg, extent=None):
    x0, xf, y0, yf = extent if extent is not None else (0.0, cfg["L"], 0.0, cfg["L"])
    return (cfg["Nx"], cfg["Ny"], x0, xf, y0, yf)


def _cols(w):
    """the state as sz_upload_floes takes it: what remove_ref works on and load_columns / set_subpoints_csr put back"""
    from subzero_jl_amd import capi
    w._push()                      # (a world that was only loaded so far: its columns through the device, like every other)
    w._host_stale = True
    c = {n: w.get(n) for n in capi.DCOLS}
    for n, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        c[n] = np.stack([w.get(pre + q) for q in ("11", "12", "21", "22")], 1)
    c["id"], c["ghost_id"], c["status"] = w.ids()
    off, x, y = w.rings()
    c["vert_off"], c["vx"], c["vy"] = off.copy(), x.copy(), y.copy()
    so, sx, sy = w.subpoints()
    c["sub_off"], c["sx"], c["sy"] = so.copy(), sx.copy(), sy.copy()
    assert len(c["cx"]) == w.N == len(off) - 1 == len(so) - 1 and not np.any(c["ghost_id"])
    return c


def _assert_bit_equal(a, b, where=""):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (where, k)


def _rebuild(w, cfg, extent, per_e, per_n, min_area=1e6, min_height=0.1):
    """the host rebuild of w's state: (fresh World, kept rows, n_removed, n_dissolved, lattice)"""
    d = w.dissolved()
    new, kept, nr, nd = rr.remove_ref(_cols(w), _grid(cfg, extent), per_e, per_n, d, min_area, min_height)
    H = _build(mk(), cfg, extent)
    sub = [new.pop(k) for k in ("sub_off", "sx", "sy")]
    H.load_columns(new)
    H.set_subpoints_csr(*sub)
    H.set_dissolved(d)
    return H, kept, nr, nd, d


# ---------------------------------------------------------------- one pass
def _long_ring_cfg():
    """200 star floes; floe 77 gets a ring of 40 points (41 with the closing one) about its centroid"""
    from subzero_jl_amd import fields, floe as floe_mod
    cfg = fields.make_config(n_floes=200, seed=9, subgrid_per_floe=4.0)
    k = 77
    off, vx, vy = cfg["vert_off"], cfg["vx"], cfg["vy"]
    cx, cy, r = cfg["derived"]["cx"][k], cfg["derived"]["cy"][k], 0.6 * cfg["derived"]["rmax"][k]
    th = (2 * np.pi / 40) * np.arange(40)[::-1]                    # descending: clockwise
    rad = r * (0.8 + 0.2 * np.cos(5 * th))
    x = cx + rad * np.cos(th); y = cy + rad * np.sin(th)
    x, y = np.append(x, x[0]), np.append(y, y[0])
    o0, o1 = off[k], off[k + 1]
    cfg["vx"] = np.concatenate([vx[:o0], x, vx[o1:]]); cfg["vy"] = np.concatenate([vy[:o0], y, vy[o1:]])
    noff = off.copy(); noff[k + 1:] += 41 - (o1 - o0)
    cfg["vert_off"] = noff
    cfg["derived"] = floe_mod.derive(noff, cfg["vx"], cfg["vy"], cfg["height"])
    so = cfg["sub_off"]
    sx, sy = fields.subgrid_points(np.stack([x, y], 1), cfg["derived"]["cx"][k], cfg["derived"]["cy"][k], cfg["dg"])
    cfg["sx"] = np.concatenate([cfg["sx"][:so[k]], sx, cfg["sx"][so[k + 1]:]]); cfg["sy"] = np.concatenate([cfg["sy"][:so[k]], sy, cfg["sy"][so[k + 1]:]])
    nso = so.copy(); nso[k + 1:] += len(sx) - (so[k + 1] - so[k])
    cfg["sub_off"] = nso
    return cfg


PATTERNS = {"none": lambda n: [], "ends": lambda n: [0, n - 1], "wavefront": lambda n: list(range(64, 128)), "all_but_first": lambda n: list(range(1, n))}


@pytest.fixture(scope="module")
def long_ring_cfg():
    return _long_ring_cfg()


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_pass_equals_host_rebuild(long_ring_cfg, pattern):
    cfg = long_ring_cfg
    n = cfg["n_floes"]
    D = _build(mk(), cfg)
    assert D.run(5, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 5          # stress, strain and the previous-step columns are not zero
    assert np.count_nonzero(D.get("sa11")) > 0 and np.count_nonzero(D.get("e11")) > n // 2 and np.count_nonzero(D.get("p_dudt")) > n // 2
    st = np.full(n, rr.ACTIVE, np.int32); st[PATTERNS[pattern](n)] = rr.REMOVE
    D.set_status(st)
    D.set_removal(True, max_vertices=64)
    D.set_dissolved(np.linspace(0.5, 1.5, (cfg["Nx"] + 1) * (cfg["Ny"] + 1)).reshape(cfg["Nx"] + 1, cfg["Ny"] + 1))
    D._push()
    H, kept, nr, nd, lattice = _rebuild(D, cfg, None, True, True)
    assert nr == len(PATTERNS[pattern](n)) and nd == 0
    assert D.remove_floes() == (True, nr, 0)
    assert D.N == n - nr == len(kept)
    assert np.array_equal(D.origin(), kept)
    _assert_bit_equal(_cols(D), _cols(H), "after the pass")
    assert np.array_equal(D.dissolved(), lattice)
    if pattern == "none":
        assert np.array_equal(D.origin(), np.arange(n))
    # any stale cache (collision records, boxes, trig, links) shows in the steps that follow
    for w in (D, H):
        assert w.run(20, 5, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 20
    _assert_bit_equal(_cols(D), _cols(H), "20 steps behind the pass")


def test_dissolve_order_and_quirks():
    """thin floes: three in one cell with masses 2^53, 1, 1 by ascending row (the sum is 2^53 + 2 in descending order only), one whose
    centroid lies south of the grid (nowhere), one beyond xf between the periodic east / west pair (wraps to the first column); on top of a
    non-zero lattice.  Then a 2 x 6 grid on which the reference's [yidx, xidx] leaves its 3 x 7 matrix: declined."""
    from subzero_jl_amd import capi, fields
    cfg = fields.make_config(n_floes=200, seed=4, subgrid_per_floe=4.0)
    cfg["kinds"] = ["collision", "collision", "periodic", "periodic"]          # N, S, E, W
    n, L, Nx = cfg["n_floes"], cfg["L"], cfg["Nx"]
    dx = L / Nx
    D = _build(mk(), cfg)
    h, m, cx, cy = D.get("height"), D.get("mass"), D.get("cx"), D.get("cy")
    rows = [10, 70, 150]
    big = float(2 ** 53)
    for r, mass, fx, fy in zip(rows, (big, 1.0, 1.0), (0.5, 0.2, 0.9), (0.3, 0.8, 0.1)):
        h[r] = 0.01; m[r] = mass; cx[r] = (17 + fx) * dx; cy[r] = (5 + fy) * dx          # cell xidx = 18, yidx = 6
    h[33] = 0.01; cy[33] = -0.5 * dx                                                      # south of the grid
    h[199] = 0.01; cx[199] = L + 0.3 * dx; cy[199] = 2.5 * dx                             # wraps to xidx = 1, yidx = 3
    st = np.full(n, rr.ACTIVE, np.int32); st[120] = rr.REMOVE; st[150 - 1] = rr.REMOVE
    h[120] = 0.01                                                                         # tagged and thin: removed, its mass goes nowhere
    for name, v in (("height", h), ("mass", m), ("cx", cx), ("cy", cy)):
        D.set(name, v)
    D.set_status(st)
    rng = np.random.default_rng(2)
    D.set_dissolved(rng.uniform(0.0, 1.0, (Nx + 1, Nx + 1)))
    D.set_removal(True, max_vertices=30)
    D._push()
    H, kept, nr, nd, lattice = _rebuild(D, cfg, None, True, False)
    assert (nr, nd) == (2, 5)
    before = D.dissolved()
    assert lattice[5, 17] == (before[5, 17] + 1.0 + 1.0) + big and lattice[5, 17] != ((before[5, 17] + big) + 1.0) + 1.0
    assert lattice[2, 0] == before[2, 0] + m[199] and np.count_nonzero(lattice != before) == 2
    assert D.remove_floes() == (True, 2, 5)
    got = D.dissolved()
    assert np.array_equal(got.view(np.uint8), lattice.view(np.uint8))
    assert np.array_equal(D.origin(), kept) and D.N == n - 7
    _assert_bit_equal(_cols(D), _cols(H), "after the pass")
    # a non-square grid on which the quirk index leaves the matrix
    w = mk()
    w.set_consts(); w.set_settings()
    w.set_domain([capi.OPEN] * 4, 0.0, 2e4, 0.0, 6e4)
    z = np.zeros((3, 7))
    w.set_grid_fields(2, 6, 0.0, 2e4, 0.0, 6e4, z, z, z, z, z)
    sq = lambda x, y, s: np.array([[x - s, y - s], [x - s, y + s], [x + s, y + s], [x + s, y - s], [x - s, y - s]])
    w.add_floe(sq(0.5e4, 0.5e4, 2e3), 0.5); w.add_floe(sq(0.5e4, 4.5e4, 2e3), 0.01); w.add_floe(sq(1.5e4, 2.5e4, 2e3), 0.5)
    w.set_dissolved(np.full((3, 7), 0.25))
    w.set_removal(True)
    w._push()
    with pytest.raises(IndexError):
        rr.remove_ref(_cols(w), (2, 6, 0.0, 2e4, 0.0, 6e4), False, False, w.dissolved())
    before = _cols(w)
    assert w.remove_floes() == (False, 0, 0)
    _assert_bit_equal(_cols(w), before, "declined: the index quirk")
    assert np.array_equal(w.dissolved(), np.full((3, 7), 0.25)) and np.array_equal(w.origin(), [0, 1, 2])
    # the same floe one cell lower (yidx = 3 = Nx + 1, the matrix's last row) dissolves
    cyw = w.get("cy"); cyw[1] = 2.5e4; w.set("cy", cyw)
    assert w.remove_floes() == (True, 0, 1)
    assert w.dissolved()[2, 0] == 0.25 + before["mass"][1] and np.array_equal(w.origin(), [0, 2])


def test_declined():
    from subzero_jl_amd import SzError, fields
    cfg = fields.make_config(n_floes=200, seed=4, subgrid_per_floe=4.0)
    n = cfg["n_floes"]
    for what in ("fuse", "vertices", "nothing left"):
        D = _build(mk(), cfg)
        st = np.full(n, rr.ACTIVE, np.int32); st[[3, 140]] = rr.REMOVE
        maxv = 30
        if what == "fuse":
            st[199] = rr.FUSE
        elif what == "vertices":
            maxv = 12
            assert np.any(np.diff(cfg["vert_off"]) > 12)
        else:
            st[:] = rr.REMOVE
        D.set_status(st)
        D.set_removal(True, max_vertices=maxv)
        D.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 2.0))
        D._push()
        before = _cols(D)
        assert D.remove_floes() == (False, 0, 0), what
        _assert_bit_equal(_cols(D), before, what)
        assert D.N == n and np.array_equal(D.origin(), np.arange(n)) and np.all(D.dissolved() == 2.0)
    # ghosts in the list
    D = _build(mk(), cfg)
    D.set_removal(True)
    D.add_ghosts()
    assert D.M > n
    with pytest.raises(SzError, match="ghosts"):
        D.remove_floes()
    D.remove_ghosts()
    assert D.remove_floes() == (True, 0, 0)


# ---------------------------------------------------------------- batches
U_OUT, XF_MARGIN, NSTEPS = 5.0, 25.0, 40


def outflow_case():
    """400 star floes between four open boundaries, the uniform ocean; the west, south and north boundaries far away, the east one
    XF_MARGIN metres beyond the easternmost vertex, every floe U_OUT m/s faster eastwards: floes reach the east boundary one after another"""
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=400, seed=11, subgrid_per_floe=4.0)
    cfg["kinds"] = ["open"] * 4
    cfg["u"] = cfg["u"] + U_OUT
    L = cfg["L"]
    extent = (-1.0e5, float(cfg["vx"].max()) + XF_MARGIN, -1.0e5, L + 1.0e5)
    return cfg, extent


def test_batch_runs_past_removals():
    """World H is the loop a resident run made before: run(), on a stop pull, remove_ref, load into a fresh World, go on.  World D: set_removal(),
    one run(NSTEPS).  The case was chosen on the CPU, with the oracle stepping and remove_ref deleting (tools/removal_case.py --steps 40):
    in 40 steps floes are removed behind steps 1, 10, 11, 14, 15, 25, 29 and 30 (0-based), two of them behind step 14, nine in all; no fuse
    tag appears and the longest ring has 17 points."""
    cfg, extent = outflow_case()
    dt, n = cfg["dt"], cfg["n_floes"]
    D = _build(mk(), cfg, extent)
    D.set_removal(True)
    D.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    assert D.run(NSTEPS, 0, dt, coupling_dt=1) == NSTEPS
    H = _build(mk(), cfg, extent)
    H.set_dissolved(np.full((cfg["Nx"] + 1, cfg["Ny"] + 1), 0.125))
    orig, t, restarts, removed_at, most = np.arange(n), 0, 0, [], 0
    while t < NSTEPS:
        t += H.run(NSTEPS - t, t, dt, coupling_dt=1)
        if t < NSTEPS:
            assert not rr.would_decline(_cols(H), 30)
            H, kept, nr, nd, _ = _rebuild(H, cfg, extent, False, False)
            assert nr + nd > 0
            orig = orig[kept]; restarts += 1; removed_at.append(t - 1); most = max(most, nr + nd)
    print(f"removals behind steps {removed_at}, at most {most} on one step, {n - len(orig)} in all")
    assert restarts >= 3 and most >= 2
    assert D.N == H.N == len(orig) < n
    _assert_bit_equal(_cols(D), _cols(H), "after the batch")
    assert np.array_equal(D.dissolved(), H.dissolved())
    assert np.array_equal(D.origin(), orig)


def _island_cfg():
    from subzero_jl_amd import fields
    return cases.floe_onto_island(fields.make_config(n_floes=900, seed=3, walls=True, topography=True, ocean="strait"))


def test_stops_where_the_host_is_needed():
    from subzero_jl_amd import capi
    cfg = _island_cfg()
    dt, n = cfg["dt"], cfg["n_floes"]
    assert np.any(np.diff(cfg["vert_off"]) > 12) and not np.any(np.diff(cfg["vert_off"]) > 30)
    # rings over max_vertices = 12: the pass is declined, the batch ends at step 0 as without removal
    off = _build(mk(), cfg)
    assert off.run(10, 0, dt, coupling_dt=1) == 1
    ref = _cols(off)
    assert ref["status"][0] == rr.REMOVE and not np.any(ref["status"] == rr.FUSE)
    D = _build(mk(), cfg)
    D.set_removal(True, max_vertices=12)
    assert D.run(10, 0, dt, coupling_dt=1) == 1
    _assert_bit_equal(_cols(D), ref, "declined inside a batch")
    # max_vertices = 30: the batch goes on past step 0
    D = _build(mk(), cfg)
    D.set_removal(True, max_vertices=30)
    done = D.run(10, 0, dt, coupling_dt=1)
    assert done > 1 and D.N < n and 0 not in D.origin()
    # a welding step that coincides with the tag ends the batch as it does without removal: the weld comes before simplify_floes!
    c = 1e12
    far = (np.array([c - 1, c + 1, c + 1, c - 1, c - 1]), np.array([c - 1, c - 1, c + 1, c + 1, c - 1]))
    for what, prepare in (("a welding step", lambda w: w.set_welding([1], [1], [1])),
                          # ... and so does a fracture step with a candidate: a criterion polygon far from every stress point
                          ("a fracture step with candidates", lambda w: w.set_fracture(capi.FRAC_POLYGON, dt=1, poly=far))):
        W0 = _build(mk(), cfg)
        prepare(W0)
        assert W0.run(10, 0, dt, coupling_dt=1) == 1, what
        D = _build(mk(), cfg)
        D.set_removal(True, max_vertices=30)
        prepare(D)
        assert D.run(10, 0, dt, coupling_dt=1) == 1, what
        assert D.N == n and D.ids()[2][0] == rr.REMOVE
        _assert_bit_equal(_cols(D), _cols(W0), what)
        if what.startswith("a fracture"):
            assert len(D.fracture_candidates()) > 0


def test_never_met_does_not_perturb():
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=400, seed=7, subgrid_per_floe=4.0)
    off = _build(mk(), cfg)
    assert off.run(40, 0, cfg["dt"], coupling_dt=1) == 40 and off.pipelined()
    on = _build(mk(), cfg)
    on.set_removal(True)
    assert on.run(40, 0, cfg["dt"], coupling_dt=1) == 40 and on.pipelined()
    _assert_bit_equal(_cols(on), _cols(off), "removal set and never met")
    assert np.array_equal(on.origin(), np.arange(cfg["n_floes"]))

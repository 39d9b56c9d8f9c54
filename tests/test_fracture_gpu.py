"""Fracture criteria on the device (csrc/sz_fracture.hpp): determine_fractures against the numpy restatement (tests/fracture_ref.py,
pinned by the reference's own test values), resident batches that end on the first fracture step with a candidate, against the oracle,
and batches the criterion must not perturb."""
import ctypes as C
import os

import numpy as np
import pytest

import fracture_ref as fr
import parity

pytestmark = pytest.mark.gpu

TIE_REL = 1e-9          # σ-points this close to the polygon boundary (relative to p / |σc|) are left out of comparisons


def mk(**env):
    import subzero_jl_amd
    for k, v in env.items():
        os.environ[k] = v
    try:
        return subzero_jl_amd.World(0)
    finally:
        for k in env:
            del os.environ[k]


def _cores():
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(quota) // int(period)))
    except Exception:
        pass
    return n


def _sa(w, n):
    return np.stack([w.get(k)[:n] for k in ("sa11", "sa12", "sa21", "sa22")], 1)


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


def test_reference_floes_fracture_as_in_the_reference():
    """test_fractures.jl:107-184: the four floes, frac_stress, HiblerYieldCurve() defaults, min_floe_area = 1e6 -> floes 1 and 2"""
    from subzero_jl_amd import capi
    g = fr.golden()
    d = g["determine_fractures"]
    rings, h, sa, _ = fr.fixture_floes(g)
    w = mk()
    w.set_domain([capi.COLLISION] * 4, -1e5, 1e5, -1e5, 1e5)
    for r, hi in zip(rings, h):
        w.add_floe(r, hi)
    for k, name in enumerate(("sa11", "sa12", "sa21", "sa22")):
        w.set(name, sa[:, k])
    w.set_fracture(capi.FRAC_HIBLER, dt=75, pstar=d["pstar"], c=d["c"], min_floe_area=d["min_floe_area"])
    assert list(w.fracture_candidates()) == [i - 1 for i in d["expected_1based"]]
    mean, p = w.fracture_mean()
    assert mean == 0.25 and p == d["pstar"] * 0.25


def _random_world(n, seed):
    """n parents with random symmetric stress_accum, heights and areas (a fifth under min_floe_area); rings are small squares on a lattice"""
    from subzero_jl_amd import capi
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(n)))
    L = side * 1e3
    ix, iy = np.arange(n) % side, np.arange(n) // side
    cx, cy = (ix + 0.5) * 1e3, (iy + 0.5) * 1e3
    q = np.array([[-100, -100], [100, -100], [100, 100], [-100, 100], [-100, -100]], float)
    vx = (cx[:, None] + q[None, :, 0]).ravel(); vy = (cy[:, None] + q[None, :, 1]).ravel()
    area = np.where(rng.random(n) < 0.2, rng.uniform(1e4, 1e6, n), rng.uniform(1e6, 1e9, n))
    height = rng.uniform(0.1, 1.5, n)
    s11, s22, s12 = rng.normal(0, 6e4, n) - 2e4, rng.normal(0, 6e4, n) - 2e4, rng.normal(0, 3e4, n)
    sa = np.stack([s11, s12, s12, s22], 1)
    w = mk()
    w.set_domain([capi.COLLISION] * 4, 0.0, L, 0.0, L)
    w.load_columns(dict(cx=cx, cy=cy, rmax=np.full(n, 150.0), area=area, height=height, mass=area * height * 920.0,
                        moment=np.ones(n), stress_accum=sa, vert_off=np.arange(0, 5 * n + 1, 5, dtype=np.int32), vx=vx, vy=vy,
                        sub_off=np.zeros(n + 1, np.int32), sx=np.zeros(0), sy=np.zeros(0)))
    return w, sa, area, height


CRITERIA = [("hibler", dict(kind=1, pstar=2.25e5, c=20.0)), ("hibler_tight", dict(kind=1, pstar=2.0e4, c=20.0)),
            ("mohr", dict(kind=2, poly=fr.calculate_mohrs()))]


@pytest.mark.parametrize("n", [1000, 100000])
def test_criteria_sweep_matches_numpy(n):
    w, sa, area, height = _random_world(n, seed=n)
    seen = 0
    for name, crit in CRITERIA:
        for alpha in (0.0, 0.5, -0.5):
            w.set_fracture(crit["kind"], dt=5, pstar=crit.get("pstar", 2.25e5), c=crit.get("c", 20.0), poly=crit.get("poly"),
                           alpha=alpha, min_floe_area=1e6)
            got = w.fracture_candidates()
            mean1 = w.fracture_mean()
            want, poly, scale = fr.determine_fractures(sa, area, height, crit["kind"], pstar=crit.get("pstar", 2.25e5),
                                                       c=crit.get("c", 20.0), poly=crit.get("poly"), alpha=alpha, min_floe_area=1e6)
            tie = fr.ties(sa, area, poly, scale, alpha, 1e6, TIE_REL)
            assert tie.sum() < 10e-6 * n, (name, alpha, int(tie.sum()))
            assert np.all(np.diff(got) > 0), "not ascending"
            g, wn = set(got.tolist()), set(want.tolist())
            assert {i for i in g ^ wn if not tie[i]} == set(), (name, alpha)
            assert 0 < len(want) < n, (name, alpha, len(want))          # the field exercises both outcomes
            seen += len(want)
            # the same field again: the same mean (a fixed-order reduction) and the same list
            again = w.fracture_candidates()
            assert np.array_equal(again, got)
            m2 = w.fracture_mean()
            assert m2[0] == mean1[0] and m2[1] == mean1[1]
            if crit["kind"] == 1:
                assert np.isclose(mean1[0], np.mean(height), rtol=1e-13, atol=0)
    assert seen > 0


def _cfg(n=2000, seed=77):
    from subzero_jl_amd import fields
    return fields.make_config(n_floes=n, seed=seed)


def _pick_pstar(cfg, nsteps=40, dt_frac=5):
    """pstar such that the first fracture step with a candidate of the oracle's own trajectory falls inside the batch, clear of ties:
    -> (pstar, first fracture tstep)"""
    from oracle import orc
    from subzero_jl_amd import fields
    ow = fields.build_world(orc.World(), cfg); ow.set_threads(_cores())
    snaps = []
    for t in range(nsteps):
        ow.timestep_sim(t, cfg["dt"], coupling_dt=1)
        if t % dt_frac == 0:
            n = ow.M          # (parents: timestep_sim! leaves no ghosts)
            snaps.append((t, _sa(ow, n), ow.get("area")[:n].copy(), ow.get("height")[:n].copy()))
    best = None
    for pstar in np.geomspace(1e1, 1e8, 400):
        first, clean = None, True
        for t, sa, area, h in snaps:
            idx, poly, scale = fr.determine_fractures(sa, area, h, 1, pstar=pstar, min_floe_area=1e6)
            stressed = np.any(sa != 0, axis=1)
            if (fr.ties(sa, area, poly, scale, 0.0, 1e6, 1e-6) & stressed).any() or \
                    (not stressed.all() and not fr.zero_point_covered_robustly(float(np.mean(h)), pstar)):
                clean = False
                break
            if len(idx):
                first = t
                break
        if clean and first is not None and 10 <= first <= 30:
            if best is None or abs(first - 20) < abs(best[1] - 20):
                best = (float(pstar), first)
    assert best is not None, "no pstar puts the first fracture inside the batch"
    return best


def test_batch_stops_where_the_reference_fractures():
    """configs[1]-style field, collisions and coupling on: World.run(40) ends after the first fracture step (dt = 5) on which the oracle's
    trajectory has a candidate; the candidates and the state there match the oracle"""
    from oracle import orc
    from subzero_jl_amd import capi, fields
    cfg = _cfg()
    pstar, tfirst = _pick_pstar(cfg)
    hw = fields.build_world(mk(), cfg)
    hw.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=pstar, min_floe_area=1e6)
    done = hw.run(40, 0, cfg["dt"], coupling_dt=1)
    assert done == tfirst + 1, (done, tfirst, pstar)
    ow = fields.build_world(orc.World(), cfg); ow.set_threads(_cores())
    for t in range(done):
        ow.timestep_sim(t, cfg["dt"], coupling_dt=1)
    n = ow.M          # (parents: timestep_sim! leaves no ghosts)
    want, poly, scale = fr.determine_fractures(_sa(ow, n), ow.get("area")[:n], ow.get("height")[:n], 1, pstar=pstar, min_floe_area=1e6)
    got = hw.fracture_candidates()
    assert len(want) > 0 and np.array_equal(got, want)
    parity.compare_worlds(hw, ow, rtol=1e-9)
    assert np.array_equal(hw.warn_counts(), ow.warn_counts())
    # the rest of the batch resumes from there
    more = hw.run(40 - done, done, cfg["dt"], coupling_dt=1, stop_on_tags=False)
    assert more == 40 - done


def test_criterion_never_met_and_run_through_do_not_perturb():
    """a criterion that is never met (a polygon no σ-point leaves: a Hibler ring of any size has the unstressed floes' (0, 0) on its
    boundary, covered or not by rounding) runs all steps bit-equal to SZ_FRAC_OFF; SZ_NO_STOP with a met criterion too (the reference those
    batches are held to: the three-launch steps, SZ_PIPELINE=0)"""
    from subzero_jl_amd import capi, fields
    cfg = _cfg(seed=78)
    nsteps = 24
    off = fields.build_world(mk(SZ_PIPELINE="0"), cfg)
    assert off.run(nsteps, 0, cfg["dt"], coupling_dt=1) == nsteps
    ref = _state(off)
    never = fields.build_world(mk(), cfg)
    never.set_fracture(capi.FRAC_POLYGON, dt=5, poly=fr.huge_square(), min_floe_area=1e6)
    assert never.run(nsteps, 0, cfg["dt"], coupling_dt=1) == nsteps
    assert not never.pipelined()
    _assert_bit_equal(ref, _state(never))
    assert len(never.fracture_candidates()) == 0

    off2 = fields.build_world(mk(SZ_PIPELINE="0"), cfg)
    assert off2.run(nsteps, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == nsteps
    met = fields.build_world(mk(), cfg)
    met.set_fracture(capi.FRAC_HIBLER, dt=5, pstar=1.0, min_floe_area=1e6)
    assert met.run(nsteps, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == nsteps
    _assert_bit_equal(_state(off2), _state(met))
    assert len(met.fracture_candidates()) > 0


def test_fracture_setting_does_not_leak_into_pipelining():
    from subzero_jl_amd import capi, fields
    cfg = _cfg(seed=79)
    a = fields.build_world(mk(), cfg)
    assert a.run(8, 0, cfg["dt"], coupling_dt=1) == 8
    assert a.pipelined()
    b = fields.build_world(mk(), cfg)
    b.set_fracture(capi.FRAC_POLYGON, dt=5, poly=fr.huge_square())
    assert b.run(8, 0, cfg["dt"], coupling_dt=1) == 8 and not b.pipelined()
    b.set_fracture(capi.FRAC_OFF)
    assert b.run(8, 8, cfg["dt"], coupling_dt=1) == 8 and b.pipelined()


def test_refusals():
    from subzero_jl_amd import capi, fields
    cfg = _cfg(n=400, seed=80)
    w = fields.build_world(mk(), cfg)
    w._push()
    L, h = w.L, w.h
    E_ARG, E_STATE = -2, -4
    px = np.zeros(129); py = np.zeros(129)
    assert L.sz_set_fracture(h, 3, 5, 2.25e5, 20.0, 0, None, None, 0.0, 1e6) == E_ARG
    assert L.sz_set_fracture(h, -1, 5, 2.25e5, 20.0, 0, None, None, 0.0, 1e6) == E_ARG
    assert L.sz_set_fracture(h, capi.FRAC_POLYGON, 5, 0.0, 0.0, 129, capi.ptr(px), capi.ptr(py), 0.0, 1e6) == E_ARG
    assert L.sz_set_fracture(h, capi.FRAC_HIBLER, 0, 2.25e5, 20.0, 0, None, None, 0.0, 1e6) == E_ARG
    assert L.sz_set_fracture(h, capi.FRAC_HIBLER, -5, 2.25e5, 20.0, 0, None, None, 0.0, 1e6) == E_ARG
    n = C.c_int32(0)
    assert L.sz_fracture_candidates(h, C.byref(n), None) == E_STATE          # no criterion set
    # a tiled context with a criterion set
    N = w.N
    gidx = np.arange(N, dtype=np.int64)
    assert L.sz_tile_enable(h, capi.ptr(gidx, capi._lp), 0.0, 0.0) == 0
    w.set_fracture(capi.FRAC_HIBLER, dt=5)
    done = C.c_int32(0)
    assert L.sz_tile_run(h, 4, 0, cfg["dt"], 1, capi.COLLISIONS_ON, C.byref(done)) == E_STATE
    assert b"fracture" in L.sz_last_error(h)
    assert L.sz_tile_step(h, None, 1, 0, 0, cfg["dt"], 1, capi.COLLISIONS_ON) == E_STATE

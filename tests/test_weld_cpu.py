"""Welding, CPU side: the restatement of bin_floe_centroids / timestep_welding! (tests/weld_ref.py) against the reference's own test values
(tests/golden/welding.json), the sufficiency of an overlap table computed once per call, and the header <-> capi.py <-> Julia mirror of the
welding entry points."""
import itertools
import os
import re

import numpy as np

import weld_ref as wr
from subzero_jl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(g):
    gr = g["grid"]
    return gr["x0"], gr["xf"], gr["y0"], gr["yf"]


def test_bins_match_the_reference_tests():
    """test_welding.jl "Bin floes": members and counts of the five cases, incl. nfloes == 6 in the open domain (the floe whose centroid is out)"""
    from oracle import orc
    g = wr.golden()
    for case in g["bin_floes"]["cases"]:
        ow = wr.golden_world(orc.World(), g, "bin_floes", case["domain"])
        per_x, per_y = wr.periodic_flags(g["domains"][case["domain"]])
        b = wr.bins(ow, _grid(g), per_x, per_y, case["nx"], case["ny"])
        seen = 0
        for want in case["bins"]:
            k = (want["yidx"] - 1) * case["nx"] + (want["xidx"] - 1)
            members = (np.nonzero(b == k)[0] + 1).tolist()
            assert members == want["members"] and len(members) == want["nfloes"], (case["domain"], case["nx"], case["ny"], want, members)
            seen += len(members)
        assert seen == int(np.sum(b >= 0)), "a floe sits in a bin the fixture does not list"


def test_break_leaves_the_floes_behind_an_out_of_bounds_centroid_unbinned():
    """welding.jl:38 is a `break`: with the out-of-bounds floe moved to the front of the list nothing is binned in the open domain"""
    from oracle import orc
    g = wr.golden()
    rings = g["bin_floes"]["rings"]
    g2 = dict(g, bin_floes=dict(g["bin_floes"], rings=[rings[0], rings[6]] + rings[1:6]))
    ow = wr.golden_world(orc.World(), g2, "bin_floes", "open")
    b = wr.bins(ow, _grid(g), False, False, 2, 2)
    assert b.tolist() == [0, -1, -1, -1, -1, -1, -1]


def test_plan_reproduces_the_reference_welds():
    """test_welding.jl "Weld floes": removed floes and the area of floe 1 for the six settings (welding_coeff = 1000: every draw passes)"""
    from oracle import orc
    g = wr.golden()
    wf = g["weld_floes"]
    ow = wr.golden_world(orc.World(), g, "weld_floes", wf["domain"])
    area = ow.get("area")
    assert np.allclose(area, wf["areas"], rtol=1e-14, atol=0)
    cand, areas = wr.overlaps(ow, _grid(g), False, False, 1, 1, 1e10)
    got = [(i + 1, j + 1) for (_, i, j), a in zip(cand, areas) if a > 0]
    assert got == [(i, j) for i, j, _ in wf["overlaps_1based"]]
    assert np.allclose([a for a in areas if a > 0], [a for _, _, a in wf["overlaps_1based"]], rtol=1e-12, atol=0)
    for case in wf["cases"]:
        cand, areas = wr.overlaps(ow, _grid(g), False, False, case["nx"], case["ny"], case["max_weld_area"])
        fuses, ndraws, new_area, status = wr.plan(wr.table_of(cand, areas), area, ow.ids()[2], case, itertools.repeat(0.5))
        removed = (np.nonzero(status == wr.REMOVE)[0] + 1).tolist()
        assert removed == case["removed"], (case, removed)
        assert np.isclose(new_area[0], case["area1"], rtol=1e-12, atol=0), (case, new_area[0])
        assert np.array_equal(new_area[1:], area[1:])
        assert ndraws == len(wr.table_of(cand, areas))


def test_a_table_computed_once_serves_the_whole_call():
    """Replay sufficiency: 300-floe star field after 20 oracle steps; the loop driven by the table of the state at the START of the call makes the
    same fuses with the same number of draws as the loop that clips every pair when it reaches it."""
    from oracle import orc
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=300, seed=7, subgrid_per_floe=4.0)
    ow = fields.build_world(orc.World(), cfg)
    for t in range(20):
        ow.timestep_sim(t, cfg["dt"], coupling_dt=1)
    n = ow.M
    assert not np.any(ow.ids()[1]), "ghosts left behind a step"
    L = cfg["L"]
    grid = (0.0, L, 0.0, L)
    area, status = ow.get("area")[:n], ow.ids()[2][:n]
    rings = [ow.ring(i) for i in range(n)]
    total = 0
    for (nx, ny), coeff, mx in (((1, 1), 1000.0, 4.0 * float(np.median(area))), ((3, 2), 1000.0, 1e12), ((1, 1), 30.0, 3.0 * float(np.median(area)))):
        s = dict(welding_coeff=coeff, min_weld_area=1e6, max_weld_area=mx)
        b = wr.bins(ow, grid, True, True, nx, ny)
        cand, areas = wr.overlaps(ow, grid, True, True, nx, ny, mx)
        table = wr.table_of(cand, areas)
        draws = np.random.default_rng(5).random(10 * len(cand) + 10)
        f1, d1, a1, s1 = wr.plan(table, area, status, s, draws)
        f2, d2, a2, s2, asked = wr.plan_live(b, ow.get("cx"), ow.get("cy"), ow.get("rmax"), rings, area, status, s, draws, orc.clip)
        assert f1 == f2 and d1 == d2, ((nx, ny), len(f1), len(f2), d1, d2)
        assert np.array_equal(a1, a2) and np.array_equal(s1, s2)
        # the live loop never asks for a pair the start-of-call candidates do not hold
        assert set(asked) <= {(i, j) for _, i, j in cand}
        assert len(f1) > 0 and len(table) > 0
        total += len(f1)
    assert total > 0


def test_welding_entry_points_mirror_header_capi_and_julia():
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    for fn, nargs, in_julia in (("sz_set_welding", 6, True), ("sz_weld_overlaps", 9, True), ("sz_debug_weld_bins", 4, False)):
        d = re.search(rf"int {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        if in_julia:
            assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    L = capi.load()
    assert len(L.sz_set_welding.argtypes) == 6 and len(L.sz_weld_overlaps.argtypes) == 9 and len(L.sz_debug_weld_bins.argtypes) == 4
    for name in ("function set_welding!", "function weld_overlaps", "function timestep_welding!"):
        assert name in jl, name
    # run_resident! takes weld_on now: its guard refuses ridging / rafting alone
    body = jl[jl.index("function run_resident!"):]
    body = body[:body.index("\nend\n")]
    guard = re.search(r"\n\s*([^\n]*?)&&\s*\n?\s*error\(\"run_resident!", body)
    assert guard, "run_resident! lost its guard"
    assert "ridge_raft_on" in guard.group(1) and "weld_on" not in guard.group(1)
    assert "set_welding!(eng, sim)" in body and "timestep_welding!(" in body and "sim.weld_settings.weld_on" in body


def test_default_paths_do_not_read_the_welding_code():
    """bench.py, smoke() and the C example run with welding off: none of them names it"""
    for name in ("bench.py", "__graft_entry__.py", os.path.join("examples", "minimal.c")):
        assert "weld" not in open(os.path.join(ROOT, name)).read().lower(), name

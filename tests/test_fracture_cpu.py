"""Fracture criteria, CPU side: the numpy restatement of determine_fractures (tests/fracture_ref.py) against the reference's own
test values (tests/golden/fractures.json), and the header <-> capi.py <-> Julia mirror of the fracture entry points."""
import os
import re

import numpy as np

import fracture_ref as fr
from subzero_jl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hibler_polygon_matches_the_reference_tests():
    g = fr.golden()
    for h in g["hibler"]:
        px, py, _ = fr.calculate_hibler(h["mean_height"], h["pstar"], h["c"])
        assert len(px) == 100 and px[0] == px[-1] and py[0] == py[-1]
        area, cx, cy = fr.ring_area_centroid(px, py)
        assert np.isclose(area, h["area"], rtol=h["area_rtol"], atol=0)
        assert np.allclose([cx, cy], h["centroid"], rtol=0, atol=h["centroid_atol"])
        assert np.allclose([px.min(), px.max()], h["x_extrema"], rtol=0, atol=h["extrema_atol"])
        assert np.allclose([py.min(), py.max()], h["y_extrema"], rtol=0, atol=h["extrema_atol"])


def test_mohrs_cone_matches_the_reference_tests():
    for m in fr.golden()["mohrs"]:
        px, py = fr.calculate_mohrs(m["q"], m["sigma_c"], m["sigma11"])
        assert np.allclose(np.c_[px, py], np.array(m["vertices"]), rtol=0, atol=m["atol"])


def test_determine_fractures_on_the_reference_floes():
    g = fr.golden()
    d = g["determine_fractures"]
    _, h, sa, area = fr.fixture_floes(g)
    idx, _, _ = fr.determine_fractures(sa, area, h, 1, pstar=d["pstar"], c=d["c"], min_floe_area=d["min_floe_area"])
    assert list(idx + 1) == d["expected_1based"]


def test_covered_by_counts_the_boundary_as_covered():
    px, py = np.array([0.0, 1.0, 1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0, 1.0, 0.0])
    assert list(fr.covered(px, py, [0.5, 1.0, 0.0, 1.5, 0.5], [0.5, 0.5, 0.0, 0.5, -1e-12])) == [True, True, True, False, False]


def test_fracture_entry_points_mirror_header_capi_and_julia():
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    m = re.search(r"enum\s*\{\s*SZ_FRAC_OFF\s*=\s*(\d+),\s*SZ_FRAC_HIBLER\s*=\s*(\d+),\s*SZ_FRAC_POLYGON\s*=\s*(\d+)\s*\}", hdr)
    assert m, "SZ_FRAC_* enum missing from the header"
    vals = tuple(int(v) for v in m.groups())
    assert (capi.FRAC_OFF, capi.FRAC_HIBLER, capi.FRAC_POLYGON) == vals
    for name, v in zip(("SZ_FRAC_OFF", "SZ_FRAC_HIBLER", "SZ_FRAC_POLYGON"), vals):
        assert re.search(rf"const {name} = Int32\({v}\)", jl), name
    for fn, nargs in (("sz_set_fracture", 10), ("sz_fracture_candidates", 3)):
        d = re.search(rf"int {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    L = capi.load()
    assert len(L.sz_set_fracture.argtypes) == 10 and len(L.sz_fracture_candidates.argtypes) == 3
    # run_resident! accepts fractures now and still refuses ridging and welding
    body = jl[jl.index("function run_resident!"):]
    body = body[:body.index("\nend\n")]
    assert "fracture_settings.fractures_on ||" not in body
    assert "ridge_raft_on" in body and "weld_on" in body and "fracture_floes!" in body

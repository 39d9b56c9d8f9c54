"""The grid paths' floe-in-cell areas where rings touch grid lines, on the device (tests/grid_cells_cases.py has the family, the exact reference
and the derived bound; tests/test_grid_cells_cpu.py holds the oracle to the same reference).  Without topography the areas come from the
rectangle pipeline (sz_k_eul_area_rect, sz_k_tw_area_rect), with an element present from sz_k_eul_area / sz_k_eul_cell_area.  Areas are held
to the exact reference under rect_bound -- cells of exact area 0 to 0.0 --, all outputs to the oracle at 1e-9 of the output's scale.  The two
capacities of these paths (FC_CAP centre cells per floe, EU_CAP ring points of the floe-against-element clip) are met at and one past:
answered exactly, or refused by name -- never a truncated field or a silent zero.
Needs a real MI355X: run with -m gpu."""
import re
from fractions import Fraction as Fr

import numpy as np
import pytest

import grid_cells_cases as G

pytestmark = pytest.mark.gpu


def mk():
    import subzero_jl_amd
    return subzero_jl_amd.World(0)


def omk():
    from oracle import orc
    return orc.World()


def _names():
    from oracle import orc
    return orc.EUL_OUTPUTS


def _capacity_bits(exc):
    """the error word of a capacity error (ring = 1 ... cells = 2048); the message lists every bit's name, the word says which are set"""
    m = re.search(r"capacity/consistency error bits 0x([0-9a-f]+)", str(exc))
    assert type(exc).__name__ == "SzError" and m, repr(exc)
    return int(m.group(1), 16)


def _assert_outputs_near(got, ref, who):
    """all 18 grids at 1e-9 of the output's scale (one scale per tensor, as tests/test_output.py); an output the oracle leaves 0 stays 0"""
    names = _names()
    for k, n in enumerate(names):
        grp = [j for j, o in enumerate(names) if o.split("_")[0] == n.split("_")[0]] if n.startswith(("stress", "strain")) else [k]
        scale = max(np.abs(ref[j]).max() for j in grp)
        assert np.abs(got[k] - ref[k]).max() <= 1e-9 * scale, (who, n, np.abs(got[k] - ref[k]).max(), scale)
        assert np.array_equal(got[k] != 0, ref[k] != 0), (who, n)


def _eulerian(rings, xg, yg, who, topo=None, ref=None, free=None):
    """one world of the rings on the device and in the oracle: areas against the exact reference, everything against the oracle, and
    write_grid_data giving the same numbers; returns the largest area error / bound"""
    hw = G.output_world(mk(), rings, xg, yg, topo=topo); ow = G.output_world(omk(), rings, xg, yg, topo=topo)
    xa, ya = np.array(xg, float), np.array(yg, float)
    d = hw.eulerian_data(xa, ya); o = ow.eulerian_data(xa, ya)
    k = _names().index
    mpa = float(ow.get("mass")[0] / ow.get("area")[0])
    if ref is None:
        nx, ny = len(xg) - 1, len(yg) - 1
        area = np.empty((nx, ny), object); area[:] = Fr(0); bound = np.zeros((nx, ny))
        for r in rings:
            a, b = G.cell_reference(r, xg, yg)
            area = area + a; bound = bound + b
        ref = (area, bound)
    print(who, "area_grid sum", d[k("area_grid")].sum(), "exact", float(sum(ref[0].ravel())))
    worst = G.assert_areas_exact(d[k("area_grid")], d[k("si_frac_grid")], d[k("mass_grid")], ref, xg, yg, mpa, who, cell_free=free)
    _assert_outputs_near(d, o, who)
    n0 = hw.M
    assert np.array_equal(hw.write_grid_data(xa, ya), d) and hw.M == n0, who
    return worst


def _two_way(ring, periodic, who, offset=0):
    hw, area, bound = G.two_way_world(mk(), ring, periodic, offset)
    ow, _, _ = G.two_way_world(omk(), ring, periodic, offset)
    got, ref = hw.ocean_stress(), ow.ocean_stress()
    worst = G.assert_si_frac_exact(got[2], area, bound, who)
    for name, g, r in zip(("tau_x", "tau_y", "si_frac", "hflx_factor"), got, ref):
        assert np.abs(g - r).max() <= 1e-9 * np.abs(r).max(), (who, name)
    return worst


# ---------------------------------------------------------------- no topography: the rectangle pipeline
@pytest.mark.parametrize("orient", G.ORIENTATIONS)
def test_eulerian_family(orient):
    worst = 0.0
    for name in G.FAMILY:
        ring, xg, yg = G.case(name, orient)
        worst = max(worst, _eulerian([ring], xg, yg, (name, orient)))
    print("worst area error / bound:", worst)


def test_eulerian_family_far_from_the_origin():
    worst = 0.0
    for name in G.FAMILY:
        ring, xg, yg = G.case(name, "cw", G.FAR)
        worst = max(worst, _eulerian([ring], xg, yg, (name, "far")))
    print("worst area error / bound:", worst)


@pytest.mark.parametrize("M", G.ROWS)
def test_eulerian_rows(M):
    rings, xg, yg = G.rows_world(M)
    print("worst area error / bound:", _eulerian(rings, xg, yg, ("rows", M)))


@pytest.mark.parametrize("periodic", (True, False), ids=("periodic", "walled"))
@pytest.mark.parametrize("orient", G.ORIENTATIONS)
def test_two_way_family(orient, periodic):
    worst = 0.0
    for name in G.FAMILY:
        ring, _, _ = G.case(name, orient)
        worst = max(worst, _two_way(ring, periodic, (name, orient, periodic)))
    print("worst si_frac error / bound:", worst)


def test_two_way_family_far_from_the_origin():
    worst = 0.0
    for name in G.FAMILY:
        ring, _, _ = G.case(name, "cw", G.FAR)
        worst = max(worst, _two_way(ring, True, (name, "far"), G.FAR))
    print("worst si_frac error / bound:", worst)


# ---------------------------------------------------------------- topography: sz_k_eul_area / sz_k_eul_cell_area
@pytest.mark.parametrize("orient", G.ORIENTATIONS)
def test_eulerian_family_with_an_element_away(orient):
    """an element off the grid and off the floe selects the topography kernels and changes no answer"""
    worst = 0.0
    for name in G.FAMILY:
        ring, xg, yg = G.case(name, orient)
        worst = max(worst, _eulerian([ring], xg, yg, (name, orient, "topo"), topo=[G.TOPO_AWAY]))
    print("worst area error / bound:", worst)


@pytest.mark.parametrize("name", tuple(G.TOPO_CASES))
def test_eulerian_element_in_the_cells(name):
    floe, topo, common = G.TOPO_CASES[name]
    area, bound, free = G.topo_reference(floe, common, topo, G.XG, G.YG)
    hw = G.output_world(mk(), [floe], G.XG, G.YG, topo=[topo])
    _eulerian([floe], G.XG, G.YG, name, topo=[topo], ref=(area, bound), free=free)
    if name == "element-covers-cell":
        d = hw.eulerian_data(np.array(G.XG, float), np.array(G.YG, float))
        assert free[3, 1] == 0 and np.all(d[:, 3, 1] == 0.0)


# ---------------------------------------------------------------- FC_CAP
def test_centre_cells_per_floe_at_and_past_the_capacity():
    cap = G.capacities()["FC_CAP"]
    hw, area, bound = G.fc_world(mk(), cap)
    hw.timestep_coupling()
    assert len(area) == cap
    print("worst si_frac error / bound:", G.assert_si_frac_exact(hw.ocean_stress()[2], area, bound, "at FC_CAP", cell=G.FC_D * G.FC_D))
    ow, _, _ = G.fc_world(omk(), cap)
    ow.timestep_coupling()
    for g, r in zip(hw.ocean_stress(), ow.ocean_stress()):
        assert np.abs(g - r).max() <= 1e-9 * np.abs(r).max()
    hw, area, _ = G.fc_world(mk(), cap + 1)
    with pytest.raises(Exception) as e:
        hw.timestep_coupling()
    assert _capacity_bits(e.value) == 2048 and f"more than {cap} distinct centre cells" in str(e.value), str(e.value)


# ---------------------------------------------------------------- EU_CAP
@pytest.mark.parametrize("topo", ("plain", "element-away", "element-met"))
def test_large_rings_are_answered_or_refused_by_name(topo):
    """rings of EU_CAP, EU_CAP + 1 and 255 points: exact, or the ring capacity by name.  Only a floe whose box meets an element's is held in
    the topography kernel's working set; every other ring of any size must be answered"""
    from subzero_jl_amd.capi import SzError
    caps = G.capacities()
    _, xg, yg = G.case("one-cell")
    for n in G.ring_sizes(caps):
        ring = G.polygon_ring(n)
        kw = {}
        if topo == "element-away":
            kw = dict(topo=[G.TOPO_AWAY])
        elif topo == "element-met":
            area, bound, free = G.ring_element_reference(ring, xg, yg)
            kw = dict(topo=[G.ring_element()], ref=(area, bound), free=free)
        try:
            worst = _eulerian([ring], xg, yg, ("ring", n, topo), **kw)
        except SzError as e:
            assert topo == "element-met" and n > caps["EU_CAP"] and _capacity_bits(e) == 1, (n, topo, str(e))
            print(n, "ring points,", topo, ": refused:", str(e))
        else:
            print(n, "ring points,", topo, ": worst area error / bound:", worst)

"""Removal and dissolution, CPU side: the restatement of remove_floes! / dissolve_floe! (tests/remove_ref.py) on hand-made cases whose outcome
is written out here, the summation order of two floes that dissolve into one cell, and the header <-> capi.py <-> Julia mirror of the entry
points."""
import os
import re

import numpy as np
import pytest

import remove_ref as rr
from subzero_jl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID = (4, 4, 0.0, 4e4, 0.0, 4e4)          # Nx, Ny, x0, xf, y0, yf: cells of 1e4


def _cols(cx, cy, area, height, mass, status):
    """n square floes of 5 ring points and 2 sub-floe points each; the ring and the points carry the row number"""
    n = len(cx)
    c = {k: np.zeros(n) for k in capi.DCOLS}
    for k in capi.TCOLS:
        c[k] = np.arange(4.0 * n).reshape(n, 4)
    c.update(cx=np.array(cx, float), cy=np.array(cy, float), area=np.array(area, float), height=np.array(height, float), mass=np.array(mass, float),
             status=np.array(status, np.int32), id=np.arange(1, n + 1, dtype=np.int64), ghost_id=np.zeros(n, np.int64),
             u=np.arange(n) * 0.5)
    c["vert_off"] = (5 * np.arange(n + 1)).astype(np.int32)
    c["vx"] = np.repeat(np.arange(n, dtype=float), 5); c["vy"] = -c["vx"]
    c["sub_off"] = (2 * np.arange(n + 1)).astype(np.int32)
    c["sx"] = np.repeat(np.arange(n, dtype=float), 2) + 0.25; c["sy"] = c["sx"] + 100.0
    return c


def _five():
    A, R = rr.ACTIVE, rr.REMOVE
    #            0 tagged      1 thin, inside    2 small, south of the grid   3 thin, beyond xf    4 tagged and thin
    return _cols(cx=[2.5e4, 1.5e4, 0.5e4, 4.5e4, 3.5e4],
                 cy=[2.5e4, 2.5e4, -0.5e4, 0.5e4, 3.5e4],
                 area=[4e6, 4e6, 5e5, 4e6, 4e6],
                 height=[0.5, 0.05, 0.5, 0.05, 0.05],
                 mass=[10.0, 20.0, 30.0, 40.0, 50.0],
                 status=[R, A, A, A, R])


@pytest.mark.parametrize("periodic_east", [False, True])
def test_five_floes(periodic_east):
    """0 and 4 are removed (4 is thin as well: removed, not dissolved); 1 dissolves into cell (xidx, yidx) = (2, 3), which the reference
    writes at dissolved[3, 2]; 2 lies south of the grid and its mass goes nowhere; 3 lies one cell east of xf: nowhere between
    non-periodic boundaries, cell xidx = 5 - 4 = 1, yidx = 1 between a periodic pair"""
    d = np.zeros((5, 5)); d[2, 1] = 0.5
    cols, kept, n_removed, n_dissolved = rr.remove_ref(_five(), GRID, periodic_east, False, d)
    assert kept.tolist() == [] and (n_removed, n_dissolved) == (2, 3)
    assert len(cols["cx"]) == 0 and cols["vert_off"].tolist() == [0] and len(cols["vx"]) == 0 and len(cols["sx"]) == 0
    want = np.zeros((5, 5)); want[2, 1] = 20.5
    if periodic_east:
        want[0, 0] = 40.0
    assert np.array_equal(d, want)


def test_kept_rows_move_up_with_their_ragged_fields():
    c = _five()
    c["status"][:] = [rr.REMOVE, rr.ACTIVE, rr.FUSE, rr.ACTIVE, rr.ACTIVE]
    c["height"][:] = 0.5; c["area"][:] = 4e6
    d = np.zeros((5, 5))
    cols, kept, n_removed, n_dissolved = rr.remove_ref(c, GRID, False, False, d, 1e6, 0.1)
    assert kept.tolist() == [1, 2, 3, 4] and (n_removed, n_dissolved) == (1, 0) and not d.any()
    assert cols["status"].tolist() == [rr.ACTIVE] * 4          # continuing floes are reset, a fuse tag too
    assert cols["id"].tolist() == [2, 3, 4, 5] and cols["u"].tolist() == [0.5, 1.0, 1.5, 2.0]
    assert cols["vert_off"].tolist() == [0, 5, 10, 15, 20] and cols["vx"].tolist() == np.repeat([1.0, 2.0, 3.0, 4.0], 5).tolist()
    assert cols["sub_off"].tolist() == [0, 2, 4, 6, 8] and cols["sx"].tolist() == (np.repeat([1.0, 2.0, 3.0, 4.0], 2) + 0.25).tolist()
    assert np.array_equal(cols["stress_accum"], np.arange(20.0).reshape(5, 4)[1:])
    assert rr.would_decline(c, 30) and not rr.would_decline(cols, 5) and rr.would_decline(cols, 4)


def test_two_floes_in_one_cell_sum_in_descending_row_order():
    """m = [2^53, 1, 1] by ascending row: reverse(eachindex(floes)) adds 1 + 1 + 2^53 = 2^53 + 2; ascending it would be 2^53"""
    big = float(2 ** 53)
    c = _cols(cx=[1.5e4, 1.2e4, 1.9e4, 3.5e4], cy=[0.5e4, 0.1e4, 0.9e4, 3.5e4], area=[4e6] * 4, height=[0.05, 0.05, 0.05, 0.5],
              mass=[big, 1.0, 1.0, 7.0], status=[rr.ACTIVE] * 3 + [rr.FUSE])
    d = np.zeros((5, 5))
    cols, kept, n_removed, n_dissolved = rr.remove_ref(c, GRID, False, False, d)
    assert kept.tolist() == [3] and (n_removed, n_dissolved) == (0, 3) and cols["status"].tolist() == [rr.ACTIVE]
    assert (big + 1.0) + 1.0 == big                  # the order matters
    assert d[0, 1] == big + 2.0
    assert np.count_nonzero(d) == 1


def test_index_quirk_outside_the_matrix_raises():
    """Nx = 2, Ny = 6: a floe in cell yidx = 5 would be written at dissolved[5, xidx] of a 3 x 7 matrix"""
    grid = (2, 6, 0.0, 2e4, 0.0, 6e4)
    c = _cols(cx=[0.5e4], cy=[4.5e4], area=[4e6], height=[0.05], mass=[3.0], status=[rr.ACTIVE])
    with pytest.raises(IndexError):
        rr.remove_ref(c, grid, False, False, np.zeros((3, 7)))
    c["cy"][0] = 2.5e4          # yidx = 3 = Nx + 1: the last row of the matrix
    d = np.zeros((3, 7))
    rr.remove_ref(c, grid, False, False, d)
    assert d[2, 0] == 3.0


def test_removal_entry_points_mirror_header_capi_and_julia():
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    want = (("sz_set_removal", 5), ("sz_remove_floes", 4), ("sz_upload_dissolved", 2), ("sz_download_dissolved", 2), ("sz_download_origin", 2))
    L = capi.load()
    for fn, nargs in want:
        d = re.search(rf"int {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        assert len(getattr(L, fn).argtypes) == nargs, fn
        assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    for name in ("function set_removal!", "function remove_floes!", "function origin", "function pull_state!"):
        assert name in jl, name
    body = jl[jl.index("function run_resident!"):]
    body = body[:body.index("\nend\n")]
    assert "set_removal!(eng, sim)" in body and "remove_floes!(" in body
    assert "todo[2] == 0 && todo[3] == 0" in body
    guard = re.search(r"\n\s*([^\n]*?)&&\s*\n?\s*error\(\"run_resident!", body)
    assert guard and "ridge_raft_on" in guard.group(1), "run_resident! lost its ridging guard"
    assert "set_welding!(eng, sim)" in body and "timestep_welding!(" in body and "simplify_floes!" in body
    pull = jl[jl.index("function pull_state!"):]
    pull = pull[:pull.index("\nend\n")]
    assert "origin(eng)" in pull and "pull_dissolved!" in pull


def test_default_paths_do_not_read_the_removal_code():
    """bench.py, smoke() and the C example run with removal off: none of them names it (bench.py's description of a timestep speaks of the
    "ghost removal" of simulation.jl:138-144: that phrase, and nothing else, is taken out before the search)"""
    for name in ("bench.py", "__graft_entry__.py", os.path.join("examples", "minimal.c")):
        text = re.sub(r"ghost\s+removal", "", open(os.path.join(ROOT, name)).read().lower())
        for word in ("removal", "remove_floes", "dissolved"):
            assert word not in text, (name, word)

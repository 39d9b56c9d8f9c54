"""The cross-rank part of a tiled removal pass (csrc/sz_remove_tile.hpp), restated in tests/remove_tiles_ref.py, against tests/remove_ref.py run
over the undivided list: merged leaving lists, global renumbering, one lattice walked in descending global number.  No GPU."""
import os
import re
import sys

import numpy as np

import remove_ref as rr
import remove_tiles_cases as cases
import remove_tiles_ref as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hold_to_undivided(cols, owner, nranks, grid, per_e, per_n, lattice0):
    """tile_remove_ref over `owner` against remove_ref over the whole list: every rank holds the single list's rows it owns, under the single
    list's new numbers, and the one lattice is the single list's to the bit"""
    want_lat = lattice0.copy()
    want, kept, nr, nd = rr.remove_ref(cols, grid, per_e, per_n, want_lat)
    got_lat = lattice0.copy()
    done, gr, gd, ranks = rt.tile_remove_ref(cols, owner, nranks, grid, per_e, per_n, got_lat)
    stay = np.bincount(np.asarray(owner)[kept], minlength=nranks)
    if np.any(stay == 0):
        assert not done and np.array_equal(got_lat, lattice0)
        return False
    assert done and (gr, gd) == (nr, nd)
    assert np.array_equal(got_lat.view(np.uint8), want_lat.view(np.uint8))
    seen = np.concatenate([g for _, g in ranks])
    assert sorted(seen) == list(range(len(kept)))
    for r, (c, g) in enumerate(ranks):
        assert np.array_equal(np.asarray(owner)[kept[g]], np.full(len(g), r))          # new number g is old number kept[g]: this rank's floe
        ref = rt.take_rows(want, g)
        assert sorted(c) == sorted(ref)
        for k in c:
            assert np.array_equal(c[k], ref[k]), (r, k)
    return True


def test_case_a_behind_step_2_with_its_owners():
    """tools/removal_tile_case.py --case a: behind step 2, rows 4 and 5 are removed (one per rank) and rows 6, 7, 8 dissolve (2 on rank 0, 1 on
    rank 1) into one cell; 2^53, 1, 1 in ascending global order sum to 2^53 + 2 only in the descending order of the undivided list"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import removal_tile_case as tool
    from subzero_jl_amd import tiles
    cfg = cases.case_a()
    owner = tiles.assign_tiles(cfg["derived"]["cx"], cfg["derived"]["cy"], cfg["L"], 2)
    assert list(owner) == cases.A_OWNERS
    t, cols, lattice = next(tool.walk(cfg, cases.A_STEPS, cases.A_RUN, upto=2))
    assert t == 2 and list(np.nonzero(cols["status"] == rr.REMOVE)[0]) == [4, 5] and not np.any(cols["status"] == rr.FUSE)
    grid = (5, 5, 0.0, 1e5, 0.0, 1e5)
    assert _hold_to_undivided(cols, owner, 2, grid, False, False, np.zeros((6, 6)))
    lat = np.zeros((6, 6))
    done, nr, nd, ranks = rt.tile_remove_ref(cols, owner, 2, grid, False, False, lat)
    assert (done, nr, nd) == (True, 2, 3)
    assert lat[1, 2] == float(2 ** 53 + 2) and np.count_nonzero(lat) == 1
    assert [list(g) for _, g in ranks] == [[1, 2, 4, 5], [0, 3, 6]]          # old rows 1, 2, 9, 10 | 0, 3, 11
    # per-rank partial sums added afterwards lose the two units
    part = [np.zeros((6, 6)), np.zeros((6, 6))]
    for r in range(2):
        rr.remove_ref(rt.take_rows(cols, np.nonzero(owner == r)[0]), grid, False, False, part[r])
    assert (part[0] + part[1])[1, 2] == float(2 ** 53)


def _random_list(rng, n=64):
    L = 1e5
    side = rng.uniform(500.0, 3000.0, n)                                # areas 2.5e5 .. 9e6 against min_floe_area = 1e6
    x0, y0 = rng.uniform(-0.1 * L, 1.05 * L, n), rng.uniform(-0.1 * L, 1.05 * L, n)          # some centroids outside the grid
    cols = {k: rng.normal(size=n) for k in rr.capi.DCOLS}
    for k in rr.capi.TCOLS:
        cols[k] = rng.normal(size=(n, 4))
    cols["cx"], cols["cy"], cols["area"] = x0 + 0.5 * side, y0 + 0.5 * side, side * side
    cols["height"] = np.where(rng.random(n) < 0.15, 0.05, 0.5)
    cols["mass"] = np.where(rng.random(n) < 0.2, 2.0 ** 53, rng.integers(1, 4, n).astype(float))          # sums whose order shows
    cols["id"] = rng.permutation(n).astype(np.int64) + 1; cols["ghost_id"] = np.zeros(n, np.int64)
    cols["status"] = np.where(rng.random(n) < 0.25, rr.REMOVE, rr.ACTIVE).astype(np.int32)
    cols["vert_off"] = (5 * np.arange(n + 1)).astype(np.int32)
    cols["vx"] = np.concatenate([[a, a, a + s, a + s, a] for a, s in zip(x0, side)]); cols["vy"] = np.concatenate([[b, b + s, b + s, b, b] for b, s in zip(y0, side)])
    ns = rng.integers(0, 4, n)
    cols["sub_off"] = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    cols["sx"], cols["sy"] = rng.normal(size=int(ns.sum())), rng.normal(size=int(ns.sum()))
    return cols


def test_random_owners_equal_the_undivided_list():
    rng = np.random.default_rng(20)
    grid = (4, 4, 0.0, 1e5, 0.0, 1e5)          # 2.5e4 m cells: several dissolving floes per cell
    went = 0
    for trial in range(50):
        cols = _random_list(rng)
        nranks = int(rng.integers(2, 5))
        owner = rng.integers(0, nranks, 64)
        per_e, per_n = bool(trial & 1), bool(trial & 2)
        went += _hold_to_undivided(cols, owner, nranks, grid, per_e, per_n, rng.uniform(0.0, 1.0, (5, 5)))
    assert went >= 45


def test_declined_cases_change_nothing():
    rng = np.random.default_rng(21)
    grid = (4, 4, 0.0, 1e5, 0.0, 1e5)
    cols = _random_list(rng)
    owner = np.arange(64) % 2
    lat = np.full((5, 5), 0.5)
    fused = dict(cols, status=cols["status"].copy()); fused["status"][7] = rr.FUSE          # on rank 1 only
    assert rt.tile_remove_ref(fused, owner, 2, grid, False, False, lat)[0] is False
    assert rt.tile_remove_ref(cols, owner, 2, grid, False, False, lat, max_vertices=4)[0] is False
    lone = np.zeros(64, int); lone[3] = 1
    gone = dict(cols, status=cols["status"].copy()); gone["status"][3] = rr.REMOVE; gone["area"] = cols["area"].copy(); gone["area"][3] = 4e6; gone["height"] = np.full(64, 0.5)
    assert rt.tile_remove_ref(gone, lone, 2, grid, False, False, lat)[0] is False          # rank 1 would be left without a floe
    assert np.all(lat == 0.5)
    # the index quirk (tests/test_remove_cpu.py: Nx = 2, Ny = 6, a floe in cell yidx = 5): met by one thin floe of rank 0, declined for both
    thin = dict(cols, cx=np.full(64, 0.5e4), cy=np.full(64, 4.5e4), area=np.full(64, 4e6), height=np.full(64, 0.5), status=np.full(64, rr.ACTIVE, np.int32))
    thin["height"][10] = 0.05
    lat = np.full((3, 7), 0.25)
    assert rt.tile_remove_ref(thin, owner, 2, (2, 6, 0.0, 2e4, 0.0, 6e4), False, False, lat)[0] is False and np.all(lat == 0.25)
    thin["cy"][10] = 2.5e4          # yidx = 3 = Nx + 1: the last row of the matrix
    assert rt.tile_remove_ref(thin, owner, 2, (2, 6, 0.0, 2e4, 0.0, 6e4), False, False, lat)[:3] == (True, 0, 1) and lat[2, 0] == 0.25 + thin["mass"][10]


def test_the_tiled_entry_point_in_header_capi_and_refusal():
    from subzero_jl_amd import capi
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    d = re.search(r"int sz_tile_remove_floes\(([^;]*?)\);", hdr)
    assert d and d.group(1).count(",") + 1 == 4
    assert "sz_tile_remove_floes" in capi.EXPORTS
    L = capi.load()
    assert len(L.sz_tile_remove_floes.argtypes) == 4 and hasattr(L, "sz_tile_remove_floes")
    api = open(os.path.join(ROOT, "subzero.jl_amd", "csrc", "sz_api.hip")).read()
    checks = api[api.index("int removal_checks("):]
    checks = checks[:checks.index("\n}\n")]
    refusal = [l for l in checks.splitlines() if "S.tiled" in l]
    assert len(refusal) == 1 and "SZ_E_STATE" in refusal[0] and "sz_tile_remove_floes" in refusal[0]
    from subzero_jl_amd import tiles
    for name in ("set_removal", "remove_floes", "dissolved", "set_dissolved"):
        assert callable(getattr(tiles.TiledWorld, name)), name

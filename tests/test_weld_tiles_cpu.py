"""The partition rule of the tiled welding pass on the CPU (tests/weld_tiles_ref.py over tests/weld_ref.py), and the mirrors of its entry point."""
import os
import re

import numpy as np
import pytest

import weld_ref as wr
import weld_tiles_ref as wt
from subzero_jl_amd import capi, fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 300


@pytest.fixture(scope="module")
def field():
    """300 star floes, 4 x 3 bins; floes 201 and 250 have their centroids out of bounds, a tenth of the floes is not active"""
    cfg = fields.make_config(n_floes=N, seed=5, subgrid_per_floe=4.0)
    d, L = cfg["derived"], cfg["L"]
    cx, cy, rmax, area = d["cx"].copy(), d["cy"].copy(), d["rmax"].copy(), d["area"].copy()
    rng = np.random.default_rng(17)
    status = np.where(rng.uniform(size=N) < 0.1, wr.REMOVE, wr.ACTIVE)
    in_bounds = np.ones(N, bool); in_bounds[[201, 250]] = False
    nx, ny = 4, 3
    xi = np.clip(np.floor(cx / (L / nx)).astype(int), 0, nx - 1); yi = np.clip(np.floor(cy / (L / ny)).astype(int), 0, ny - 1)
    raw = (yi * nx + xi).astype(np.int32)
    return dict(cx=cx, cy=cy, rmax=1.3 * rmax, area=area, status=status, in_bounds=in_bounds, raw=raw, max_area=float(np.quantile(area, 0.9)))


def _owners(nranks, seed):
    return np.random.default_rng(seed).integers(0, nranks, N)


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_partition_rule_gives_the_single_lists_order(field, nranks):
    f = field
    for seed in range(nranks):          # 2, 3 and 4 random ownerships
        owner = _owners(nranks, 100 * nranks + seed)
        first, per_rank = wt.break_number(f["in_bounds"], owner, nranks)
        assert first == 201 and first == min(per_rank) and sorted(set(per_rank) - {N}) == sorted({201, 250} if owner[201] != owner[250] else {201})
        bin_ = np.where(np.arange(N) < first, f["raw"], -1).astype(np.int32)
        want = wr.candidates(bin_, f["cx"], f["cy"], f["rmax"], f["area"], f["status"], f["max_area"])
        assert len(want) > 50 and all(j < first for _, _, j in want)
        work = [wt.rank_work(r, owner, bin_, f["cx"], f["cy"], f["rmax"], f["area"], f["status"], f["max_area"], N) for r in range(nranks)]
        keys = [w[0] for w in work]
        assert sum(len(k) for k in keys) == len(set(k for ks in keys for k in ks)), "a pair owned twice"
        assert wt.merge(keys, N) == want
        # what each rank marks wanted on its own is what the owners of the cross-rank pairs will ask it for
        cross = 0
        for r in range(nranks):
            asked = {j for q in range(nranks) if q != r for (_, i, j) in wt.merge([keys[q]], N) if owner[j] == r}
            assert work[r][1] == asked, (nranks, seed, r)
            cross += len(asked)
        assert cross > 0


def test_the_verdict_does_not_depend_on_the_order_of_its_floes(field):
    f = field
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, N, 20000), rng.integers(0, N, 20000)
    v1, v2 = wt.verdict(f["cx"], f["cy"], f["rmax"], a, b), wt.verdict(f["cx"], f["cy"], f["rmax"], b, a)
    assert np.array_equal(v1, v2) and 0 < np.count_nonzero(v1) < len(v1)
    # to the bit: the two sides of the comparison, not only its outcome
    for s in (1, -1):
        ddx, ddy = s * (f["cx"][a] - f["cx"][b]), s * (f["cy"][a] - f["cy"][b])
        ex, ey = f["cx"][b] - f["cx"][a], f["cy"][b] - f["cy"][a]
        assert np.array_equal((ddx * ddx + ddy * ddy).view(np.uint64), (ex * ex + ey * ey).view(np.uint64))
    assert np.array_equal((f["rmax"][a] + f["rmax"][b]).view(np.uint64), (f["rmax"][b] + f["rmax"][a]).view(np.uint64))


def test_tiled_welding_entry_point_mirrors_header_capi_and_julia():
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    for fn, nargs, in_julia in (("sz_tile_weld_overlaps", 9, True), ("sz_tile_debug_weld_bins", 4, False), ("sz_tile_debug_weld_npairs", 2, False)):
        d = re.search(rf"int {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        if in_julia:
            assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    assert "int64_t *idx_i, int64_t *idx_j" in re.search(r"int sz_tile_weld_overlaps\(([^;]*?)\);", hdr).group(1)
    L = capi.load()
    assert len(L.sz_tile_weld_overlaps.argtypes) == 9 and L.sz_tile_weld_overlaps.argtypes[6] is capi._lp
    assert len(L.sz_tile_debug_weld_bins.argtypes) == 4 and len(L.sz_tile_debug_weld_npairs.argtypes) == 2
    assert "function tile_weld_overlaps" in jl
    from subzero_jl_amd import tiles
    for name in ("set_welding", "weld_overlaps", "weld_candidate_pairs"):
        assert callable(getattr(tiles.TiledWorld, name)), name

"""The partition and merge rule of the tiled ridge / raft candidate pass (tests/ridgeraft_tiles_ref.py; DESIGN.md §9e, "tiled contexts") over
ridgeraft_ref.table on the oracle, and the mirror check of the new entry points."""
import os
import re

import numpy as np
import pytest

import ridgeraft_ref as rr
import ridgeraft_tiles_ref as rt
from test_ridgeraft_cpu import field, stepped

pytestmark = pytest.mark.filterwarnings("ignore")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def periodic_field():
    """the 300-floe periodic field of tests/test_ridgeraft_cpu.py, thirty steps in, heights on both sides of every threshold"""
    cfg = field("periodic")
    rng = np.random.default_rng(5)
    w = stepped(cfg, heights=lambda h: rng.choice([0.1, 0.2, 0.25, 0.3, 1.0, 1.25, 2.0, 5.0, 6.0], len(h)))
    n = cfg["n_floes"]
    assert w.M > n, "no ghosts in the list"
    key, root = rt.keys(w, n)
    return dict(w=w, n=n, view=rr._View(w, None), key=key, root=root, want=rr.table(w, rr.SETTINGS, None))


@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_partition_and_merge_give_the_single_table(periodic_field, nranks):
    """random ownerships, shuffled local lists, keys in place of positions: no list row is evaluated twice, every one once; the merged, renamed table
    is ridgeraft_ref.table entry for entry (frac to the bit); the draws add up"""
    F = periodic_field
    v, key, root, n = F["view"], F["key"], F["root"], F["n"]
    want, want_draws = F["want"]
    assert len(want) > 20 and sum(j - 1 >= n for _, j, _, _ in want) >= 5, "the field does not exercise ghost rows"
    for seed in range(3):
        rng = np.random.default_rng(100 * nranks + seed)
        owner = rng.integers(0, nranks, n)
        lists = rt.rank_lists(v, key, root, owner, nranks, rng)
        tables, claimed, draws, gkeys = [], [], 0, []
        for r in range(nranks):
            t, ev, d, gk = rt.local_table(v, key, root, owner, r, lists[r], rr.SETTINGS, 0)
            tables.append(t); claimed += ev; draws += d; gkeys.append(gk)
        assert sorted(claimed) == list(range(v.M)), "a list row is evaluated twice, or by no rank"
        assert draws == want_draws == rr.n_draws(v.h, rr.SETTINGS)
        got = rt.merge(tables, gkeys, n)
        assert [e[:3] for e in got] == [e[:3] for e in want], (nranks, seed, len(got), len(want))
        assert np.array_equal(np.array([e[3] for e in got]).view(np.uint64), np.array([e[3] for e in want]).view(np.uint64))
        # the gate is a comparison of keys: local positions say something else for many pairs
        flipped = 0
        for r in range(nranks):
            pos = {int(k): p for p, k in enumerate(key[lists[r]["glob"]])}
            flipped += sum(1 for ki, kj, _, _ in tables[r] if kj >= 0 and pos[ki] > pos[kj])
        assert flipped > 0, "the shuffle never put j in front of i"


def test_tiled_ridgeraft_entry_points_mirror_header_capi_and_julia():
    from subzero_jl_amd import capi
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    L = capi.load()
    for fn, nargs in (("sz_tile_ridgeraft_candidates", 8), ("sz_tile_list_numbers", 3), ("sz_tile_list_keys", 3), ("sz_tile_step_finish", 5)):
        d = re.search(rf"\nint {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        assert len(getattr(L, fn).argtypes) == nargs, fn
        assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    assert "int64_t *idx_i, int64_t *idx_j" in re.search(r"int sz_tile_ridgeraft_candidates\(([^;]*?)\);", hdr).group(1)
    a = L.sz_tile_ridgeraft_candidates.argtypes
    assert a[3] is capi._lp and a[4] is capi._lp and a[5] is capi._ip and a[6] is capi._dp and a[7] is capi._lp
    assert L.sz_tile_list_numbers.argtypes[1] is capi._lp and L.sz_tile_list_keys.argtypes[1] is capi._lp
    for name in ("function tile_set_ridgeraft!", "function tile_ridgeraft_candidates", "function tile_list_numbers", "function tile_list_keys", "function tile_step_finish!"):
        assert name in jl, name
    from subzero_jl_amd import tiles
    for name in ("set_ridgeraft", "ridgeraft_candidates", "ridgeraft_pending", "ridgeraft_draws", "list_numbers", "list_keys", "finish_step"):
        assert callable(getattr(tiles.TiledWorld, name)), name

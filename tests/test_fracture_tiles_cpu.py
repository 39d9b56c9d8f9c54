"""The cross-rank part of a tiled criterion pass (csrc/sz_fracture_tile.hpp), restated in tests/fracture_tiles_ref.py: heights gathered by
global number give the undivided list's mean to the bit; per-rank sums added afterwards do not, on the very field the GPU tests use.  And the
entry point through header, binding and refusals.  No GPU."""
import os
import re

import numpy as np

import fracture_tiles_ref as ft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_restated_mean_is_the_kernels_order():
    """1 500 rows: threads 0 .. 475 sum two rows (t, then t + 1024), the others one; then the tree.  Against the same additions spelled out"""
    h = ft.one_pass_case()[3]
    sh = [0.0] * 1024
    for t in range(1024):
        s = 0.0
        for i in range(t, len(h), 1024):
            s += float(h[i])
        sh[t] = s
    w = 512
    while w > 0:
        for t in range(w):
            sh[t] += sh[t + w]
        w >>= 1
    assert _bits(ft.kernel_sum(h)) == _bits(sh[0])
    assert _bits(ft.kernel_mean(h)) == _bits(sh[0] / 1500.0)
    assert np.isclose(ft.kernel_mean(h), np.mean(h), rtol=1e-13, atol=0)
    assert ft.kernel_mean(np.zeros(0)) == 0.0


def test_the_case_tells_the_gathered_order_from_a_reduce_of_rank_sums():
    cfg, _, _, h = ft.one_pass_case()
    want = ft.kernel_mean(h)
    rng = np.random.default_rng(7)
    for trial in range(50):
        nranks = int(rng.integers(2, 9))
        owner = rng.integers(0, nranks, len(h))
        assert _bits(ft.gathered_mean(h, owner, nranks)) == _bits(want), trial
    for nranks in (2, 4):
        owner = ft.one_pass_owners(cfg, nranks)
        counts = np.bincount(owner, minlength=nranks)
        assert counts.min() > 0 and counts.sum() == len(h)
        # the ranks' rows interleave in global order: no rank holds one contiguous block
        assert np.count_nonzero(np.diff(owner)) > nranks
        assert _bits(ft.gathered_mean(h, owner, nranks)) == _bits(want)
        assert _bits(ft.reduced_mean(h, owner, nranks)) != _bits(want), nranks          # the GPU case can tell the two apart
        assert np.isclose(ft.reduced_mean(h, owner, nranks), want, rtol=1e-13, atol=0)


def test_the_tiled_entry_point_in_header_capi_and_refusals():
    from subzero_jl_amd import capi, tiles
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    d = re.search(r"int sz_tile_fracture_candidates\(([^;]*?)\);", hdr)
    assert d and d.group(1).count(",") + 1 == 5
    assert "sz_tile_fracture_candidates" in capi.EXPORTS
    L = capi.load()
    assert hasattr(L, "sz_tile_fracture_candidates")
    assert L.sz_tile_fracture_candidates.argtypes == [capi.C.c_void_p, capi._ip, capi._ip, capi._ip, capi._lp]
    # what still refuses a criterion on a tiled context: sz_tile_step, a context without set-up or communicator, two-way coupling
    api = "".join(open(os.path.join(ROOT, "subzero.jl_amd", "csrc", f)).read() for f in ("sz_api.hip", "sz_tile_host.hpp"))      # (the tiled entry points)
    refusals = [l for l in api.splitlines() if "frac_kind != SZ_FRAC_OFF" in l and "SZ_E_STATE" in l]
    assert len(refusals) == 2
    step = api[api.index("int sz_tile_step("):]
    step = step[:step.index("\n}\n")]
    assert refusals[0] in step and "sz_tile_step does not evaluate fracture criteria" in refusals[0]
    run = api[api.index("int sz_tile_run("):]
    run = run[:run.index("\n}\n")]
    assert refusals[1] in run and "c->comm_n < 1 || c->tile_margin <= 0" in refusals[1] and "fracture" in refusals[1]
    two_way = [l for l in run.splitlines() if "c->two_way" in l and "SZ_E_STATE" in l]
    assert len(two_way) == 1 and "frac" in two_way[0] and "fracture" in two_way[0]
    assert "mean height needs an all-reduce" not in api
    for name in ("set_fracture", "fracture_candidates", "fracture_mean"):
        assert callable(getattr(tiles.TiledWorld, name)), name

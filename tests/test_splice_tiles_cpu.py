"""A rank's share of a global row edit, stated in numpy (tests/splice_tiles_ref.py), held to tests/splice_ref.py's `apply` over the undivided
list: for any assignment of the floes to ranks, the ranks' lists behind their shares, put in the order of their new global numbers, ARE the edited
list.  The edits are the shapes of tests/test_splice_gpu.py::_edit with the rows of a 64-floe hand list.  No device."""
import os
import re

import numpy as np
import pytest

import splice_ref as sp
import splice_tiles_ref as st
from test_splice_gpu import SHAPES, _hand_cfg          # (the shapes the GPU tests run; importing that module touches no device)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64


@pytest.fixture(scope="module")
def hand():
    """(config, the 64 floes in the layout of World.download_rows): every column distinct per floe, interaction rows on every fifth floe"""
    from subzero_jl_amd import capi
    cfg = _hand_cfg(N, room=N + 40)
    d = cfg["derived"]
    rng = np.random.Generator(np.random.PCG64(17))
    full = {k: rng.uniform(-1.0, 1.0, N) for k in capi.DCOLS}
    for k in ("cx", "cy", "rmax", "area", "height", "mass", "moment"):
        full[k] = np.array(d[k], np.float64)
    for k in capi.TCOLS:
        full[k] = rng.uniform(-1.0, 1.0, (N, 4))
    full["id"] = np.arange(1, N + 1, dtype=np.int64); full["ghost_id"] = np.zeros(N, np.int64); full["status"] = np.ones(N, np.int32)
    full["vert_off"], full["vx"], full["vy"] = cfg["vert_off"].copy(), cfg["vx"].copy(), cfg["vy"].copy()
    full["sub_off"], full["sx"], full["sy"] = cfg["sub_off"].copy(), cfg["sx"].copy(), cfg["sy"].copy()
    cnt = np.array([2 if i % 5 == 0 else 0 for i in range(N)])
    full["inter_off"] = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    full["inter_rows"] = rng.uniform(0.0, 9.0, (int(cnt.sum()), 7))
    return cfg, full


def _new(full, cfg, like, how, next_id):
    """one new floe per entry of `like`, shaped from that floe's ring: scaled / more (points) / fewer / piece (a small copy)"""
    fn = {"scaled": lambda r: sp.scaled(r, 0.9), "more": sp.resampled, "fewer": lambda r: np.concatenate([r[:3], r[:1]]), "piece": lambda r: sp.scaled(r, 0.3)}
    rings = [fn[h](sp.ring_of(full, i)) for i, h in zip(like, how)]
    return sp.floes_from(rings, sp.take(full, like), np.arange(next_id, next_id + len(like)), cfg["dg"], inter=[sp.inter_of(full, i) for i in like])


def _edit64(name, full, cfg):
    """test_splice_gpu._edit's shapes on 64 floes"""
    n, nid = N, 1000
    if name == "noop":
        return (), None, None
    if name.startswith("del_"):
        return {"del_first": [0], "del_last": [n - 1], "del_adjacent": [16, 17], "del_all_but_one": [i for i in range(n) if i != 7]}[name], None, None
    if name.startswith("rep_"):
        rows, how = {"rep_same": ([8], ["scaled"]), "rep_fewer": ([8], ["fewer"]), "rep_more": ([8], ["more"]), "rep_first": ([0], ["more"]),
                     "rep_last": ([n - 1], ["fewer"])}[name]
        return (), (rows, _new(full, cfg, rows, how, nid)), None
    if name == "append":
        return (), None, _new(full, cfg, [10, 10], ["piece", "piece"], nid)
    if name == "fracture":
        return [10, 32, n - 1], None, _new(full, cfg, [10] * 3 + [32] * 3 + [n - 1] * 3, ["piece"] * 9, nid)
    if name == "fuse":
        return [21, 49], ([20, 48], _new(full, cfg, [20, 48], ["more", "scaled"], nid)), None
    if name == "ridge":
        rows = [30, 31, 40, 41]
        return (), (rows, _new(full, cfg, rows, ["fewer", "scaled", "fewer", "more"], nid)), _new(full, cfg, [30, 40], ["piece", "piece"], nid + 4)
    if name == "everything":
        rows = [7, 16, n - 1]
        return [5, 6, 60], (rows, _new(full, cfg, rows, ["more", "fewer", "scaled"], nid)), _new(full, cfg, [5, 5, 60, 60], ["piece"] * 4, nid + 3)
    raise KeyError(name)


def _owners(rng, nranks, n):
    while True:
        o = rng.integers(0, nranks, n)
        if len(set(o)) == nranks:
            return o


def _ranks_equal_apply(full, gidx_by_rank, edit, owner):
    """every rank applies its share to its own rows; concatenated by new number the results are splice_ref.apply of the undivided list"""
    want = sp.apply(full, *edit)
    shares = [st.share(g, edit, owner, r, sp.n_rows(full)) for r, g in enumerate(gidx_by_rank)]
    lists = [st.apply_share(sp.take(full, g), s, edit) for g, s in zip(gidx_by_rank, shares)]
    new = np.concatenate([s["gidx"] for s in shares])
    assert sorted(new) == list(range(sp.n_rows(want))), "every new number once"
    for s, l in zip(shares, lists):
        assert sp.n_rows(l) == len(s["gidx"]) and np.all(np.diff(s["gidx"]) > 0), "a rank's rows stay ascending by number"
    whole = lists[0]
    for l in lists[1:]:
        whole = sp.apply(whole, append=l)
    got = sp.take(whole, np.argsort(new, kind="stable"))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), k
    return shares


@pytest.mark.parametrize("shape", [s for s in SHAPES if s != "del_all_but_one"])
def test_shares_over_random_owners_equal_apply(hand, shape):
    cfg, full = hand
    edit = _edit64(shape, full, cfg)
    n_app = st.n_staged(edit)[1]
    rng = np.random.Generator(np.random.PCG64(SHAPES.index(shape)))
    for trial in range(50):
        nranks = 2 + trial % 3
        own = _owners(rng, nranks, N)
        gidx = [np.nonzero(own == r)[0] for r in range(nranks)]
        app_owner = rng.integers(0, nranks, n_app) if n_app else None
        v = st.verdict(gidx, edit, app_owner)
        if v is not None:          # (a random assignment may leave a rank nothing but deleted floes: then that is the verdict, and the only one)
            assert v[0] == st.E_ARG and "without a floe" in v[1], (shape, trial, v)
            continue
        _ranks_equal_apply(full, gidx, edit, app_owner)


def test_an_edit_that_touches_one_rank_only(hand):
    cfg, full = hand
    gidx = [np.arange(0, 32), np.arange(32, 64)]
    edit = ([3], ([5], _new(full, cfg, [5], ["more"], 500)), _new(full, cfg, [9], ["piece"], 501))
    assert st.verdict(gidx, edit, [0]) is None
    s0, s1 = _ranks_equal_apply(full, gidx, edit, [0])
    assert len(s1["del_rows"]) == len(s1["rep_rows"]) == len(s1["staged"]) == 0
    assert np.array_equal(s1["gidx"], np.arange(31, 63)), "the untouched rank's numbers still move"
    assert np.array_equal(s0["gidx"], np.concatenate([np.arange(31), [63]])) and list(s0["staged"]) == [0, 1]


def test_a_cross_rank_fuse(hand):
    """the replacement on one rank, the deletion on another"""
    cfg, full = hand
    own = np.arange(N) % 2
    gidx = [np.nonzero(own == r)[0] for r in range(2)]
    edit = ([41], ([20], _new(full, cfg, [20], ["more"], 500)), None)
    assert st.verdict(gidx, edit, None) is None
    s0, s1 = _ranks_equal_apply(full, gidx, edit, None)
    assert list(s0["rep_rows"]) == [10] and len(s0["del_rows"]) == 0 and list(s0["staged"]) == [0]
    assert list(s1["del_rows"]) == [20] and len(s1["rep_rows"]) == 0 and len(s1["staged"]) == 0
    assert s0["gidx"][-1] == 61 and s1["gidx"][-1] == 62


def test_every_refusal_rule(hand):
    cfg, full = hand
    gidx = [np.arange(0, 40), np.arange(40, 64)]
    ok = _new(full, cfg, [8], ["scaled"], 700)
    two = _new(full, cfg, [8, 9], ["scaled", "scaled"], 700)
    app = _new(full, cfg, [9], ["piece"], 800)
    refused = lambda edit, owner=None, **kw: st.verdict(gidx, edit, owner, **kw)
    assert refused(([5, 3], None, None)) == (st.E_ARG, "del not ascending")
    assert refused(([5, 5], None, None)) == (st.E_ARG, "del repeats")
    assert refused(([-1], None, None)) == (st.E_ARG, "del negative")
    assert refused(((), ([9, 8], two), None)) == (st.E_ARG, "rep not ascending")
    assert refused(([8], ([8], ok), None)) == (st.E_ARG, "both deleted and replaced")
    assert refused(((), None, app), [2]) == (st.E_ARG, "app_owner out of range")
    assert refused(((), None, app), [-1]) == (st.E_ARG, "app_owner out of range")
    assert refused(((), None, app), None) == (st.E_ARG, "app_owner missing")
    opened = {k: v.copy() for k, v in ok.items()}; opened["vx"][-1] += 1.0
    assert refused(((), ([8], opened), None)) == (st.E_ARG, "open ring")
    th = np.linspace(0.0, -2.0 * np.pi, 300)
    ring = np.stack([full["cx"][8] + 3e3 * np.cos(th), full["cy"][8] + 3e3 * np.sin(th)], 1); ring[-1] = ring[0]
    long_ = sp.floes_from([ring], sp.take(full, [8]), [900], cfg["dg"])
    assert refused(((), None, long_), [0]) == (st.E_ARG, "ring over 255 points")
    # what only the agreement shows
    assert refused(([N], None, None)) == (st.E_ARG, "a name out of range or owned twice")
    assert refused(((), ([N + 3], ok), None)) == (st.E_ARG, "a name out of range or owned twice")
    assert st.verdict([np.arange(0, 40), np.arange(39, 64)], ([39], None, None), None) == (st.E_ARG, "a name out of range or owned twice")
    assert refused((list(range(N)), None, None)) == (st.E_ARG, "the edit leaves no floe")
    assert refused((list(range(40, 64)), None, None)) == (st.E_ARG, "the edit leaves rank 1 without a floe")
    assert refused((list(range(40, 64)), None, app), [0]) == (st.E_ARG, "the edit leaves rank 1 without a floe")
    assert refused((list(range(40, 64)), None, app), [1]) is None, "the appended floe keeps the rank alive"
    assert refused(([i for i in range(N) if i != 7], None, None)) == (st.E_ARG, "the edit leaves rank 1 without a floe")          # del_all_but_one
    for bit, code in (("ghosts", st.E_STATE), ("order", st.E_STATE), ("error", st.E_CAPACITY), ("rowcap", st.E_CAPACITY)):
        assert refused(([3], None, None), state_bits=[None, bit]) == (code, bit)
    assert st.verdict([np.arange(0, 64), np.zeros(0, int)], ([3], None, None), None) == (st.E_STATE, "a rank holds no floe")
    # the all-empty edit: nothing to agree on, whatever the ranks' state
    assert refused(((), None, None), state_bits=["ghosts", "error"]) is None


def test_new_names_in_header_bindings_and_julia():
    from subzero_jl_amd import capi, tiles
    hdr = open(os.path.join(ROOT, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(ROOT, "julia", "SubzeroHIP.jl")).read()
    L = capi.load()
    for fn, nargs in (("sz_tile_download_rows", 9), ("sz_tile_splice_floes", 12), ("sz_tile_download_rows_f32", 9), ("sz_tile_splice_floes_f32", 12)):
        d = re.search(rf"\nint {fn}\(([^;]*?)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        assert len(getattr(L, fn).argtypes) == nargs, fn
        assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    for name in ("function tile_download_rows!", "function tile_splice!"):
        assert name in jl, name
    assert "const int64_t *gidx" in re.search(r"int sz_tile_download_rows\(([^;]*?)\);", hdr).group(1)
    assert tiles.TiledWorld.download_rows and tiles.TiledWorld.splice_global and tiles.TiledWorld.splice

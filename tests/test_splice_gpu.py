"""Rows down, rows back (csrc/sz_splice.hpp): World.download_rows against a full download, World.splice against a FRESH World
with identical settings that is loaded with the edited list (tests/splice_ref.py: apply, then load_columns + set_subpoints_csr +
set_interactions) -- what a host did before these calls existed.  Every comparison is on bits and covers every downloadable item: columns,
rings, sub-floe points, interaction rows, origin and the counts of stats(); the steps that follow an edit show a stale derived buffer."""
import os

import numpy as np
import pytest

import fracture_ref as fr
import splice_ref as sp

pytestmark = pytest.mark.gpu

STATS = ("M", "N", "n_ring_points", "n_sub_points", "n_inter_rows")          # (the counts an upload sets)


def mk(ftype=np.float64, **env):
    import subzero_jl_amd
    os.environ.update(env)
    try:
        return subzero_jl_amd.World(0, ftype=ftype)
    finally:
        for k in env:
            del os.environ[k]


# ---------------------------------------------------------------- fields
def _hand_cfg(n, room=None):
    """n well-separated floes, triangles and squares in turn, on a lattice with room for `room` floes; periodic, uniform ocean"""
    from subzero_jl_amd import fields, floe as floe_mod
    spacing, side = 2.0e4, 8.0e3
    n_side = max(2, int(np.ceil(np.sqrt(room or n))))
    L = n_side * spacing
    rings = [_hand_ring(k, n_side, spacing, side) for k in range(n)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    rng = np.random.Generator(np.random.PCG64(5))
    Nx = Ny = 4 * n_side
    z = np.zeros((Nx + 1, Ny + 1))
    cfg = dict(n_floes=n, L=L, kinds=["periodic"] * 4, vert_off=off, vx=vx, vy=vy, height=np.full(n, 0.25), u=rng.uniform(-0.1, 0.1, n),
               v=rng.uniform(-0.1, 0.1, n), xi=rng.uniform(-1e-6, 1e-6, n), dt=20, Nx=Nx, Ny=Ny, uo=z + 0.1, vo=z, hf=z, ua=z, va=z, topography=[],
               dg=side / 2.0, E=6e6, n_side=n_side, spacing=spacing, side=side)
    d = cfg["derived"] = floe_mod.derive(off, vx, vy, cfg["height"])
    so = [0]; sxs = []; sys_ = []
    for i, r in enumerate(rings):
        sx, sy = fields.subgrid_points(r, d["cx"][i], d["cy"][i], cfg["dg"])
        so.append(so[-1] + len(sx)); sxs.append(sx); sys_.append(sy)
    cfg["sub_off"] = np.array(so, np.int32); cfg["sx"] = np.concatenate(sxs); cfg["sy"] = np.concatenate(sys_)
    return cfg


def _hand_ring(k, n_side, spacing, side, triangle=None):
    """clockwise, closed: a square (even k) or a triangle (odd k, or asked for) in lattice cell k"""
    cx, cy, h = (k % n_side + 0.5) * spacing, (k // n_side + 0.5) * spacing, side / 2
    if not (k % 2 if triangle is None else triangle):
        return np.array([[cx - h, cy - h], [cx - h, cy + h], [cx + h, cy + h], [cx + h, cy - h], [cx - h, cy - h]])
    return np.array([[cx - h, cy - h], [cx, cy + h], [cx + h, cy - h], [cx - h, cy - h]])


CFG = {}


def _cfg(name):
    from subzero_jl_amd import fields
    if name not in CFG:
        if name == "periodic":
            CFG[name] = fields.make_config(n_floes=400, seed=11, subgrid_per_floe=4.0)
        elif name == "walls":
            CFG[name] = fields.make_config(n_floes=400, seed=3, walls=True, topography=True, ocean="strait", subgrid_per_floe=4.0)
        else:
            kind, n = name.split("-")[:2]
            CFG[name] = _hand_cfg(int(n), room=2200 if name.endswith("-roomy") else int(n) + 2)
    return CFG[name]


def _settings(w, cfg, setup=None):
    """fields.build_world without its floes: constants, domain, topography, fields, then what the variant sets"""
    from subzero_jl_amd import fields
    w.set_consts(E=cfg["E"]); w.set_settings()
    L = cfg["L"]
    w.set_domain([fields.KIND[k] for k in cfg["kinds"]], 0.0, L, 0.0, L)
    if cfg["topography"]:
        w.set_topography(cfg["topography"])
    w.set_grid_fields(cfg["Nx"], cfg["Ny"], 0.0, L, 0.0, L, cfg["uo"], cfg["vo"], cfg["hf"], cfg["ua"], cfg["va"])
    if setup:
        setup(w, cfg)
    return w


def _settled(name, setup=None, env=None, steps=20, ftype=np.float64):
    """the field stepped `steps` steps: interaction rows exist, the previous-step columns and the stresses are not zero"""
    from subzero_jl_amd import fields
    cfg = _cfg(name)
    w = fields.build_world(mk(ftype, **(env or {})), cfg)
    if setup:
        setup(w, cfg)
    if steps:
        assert w.run(steps, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == steps
    return w, cfg


def _full(w):
    """everything downloadable, as a floe list in the layout of download_rows (all rows of the list, ghosts included if there are any)"""
    from subzero_jl_amd import capi
    w._push_interactions()
    w._host_stale = True
    c = {n: w.get(n) for n in capi.DCOLS}
    for n, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        c[n] = np.stack([w.get(pre + q) for q in ("11", "12", "21", "22")], 1)
    c["id"], c["ghost_id"], c["status"] = w.ids()
    off, x, y = w.rings()
    c["vert_off"], c["vx"], c["vy"] = off.copy(), x.copy(), y.copy()
    so, sx, sy = w.subpoints()
    c["sub_off"], c["sx"], c["sy"] = so.copy(), sx.copy(), sy.copy()
    io, ir = w.interactions()
    c["inter_off"], c["inter_rows"] = io.copy(), ir.copy().reshape(-1, 7)
    return c


def _state(w):
    c = _full(w)
    st = w.stats()
    c["stats"] = np.array([st[k] for k in STATS], np.int64)
    c["origin"] = w.origin()
    return c


def _assert_bit_equal(a, b, where=""):
    assert sorted(a) == sorted(b), where
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (where, k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
        if a[k].size == 0:
            continue
        x, y = (np.ascontiguousarray(v).reshape(len(v), -1).view(np.uint8) for v in (a[k], b[k]))
        assert np.array_equal(x, y), (where, k, "first entries that differ:", list(np.nonzero(np.any(x != y, axis=1))[0][:8]), "of", len(x))


def _fresh(cfg, cols, setup=None, env=None, ftype=np.float64):
    """the oracle: a fresh World with identical settings, loaded with the list `cols`"""
    H = _settings(mk(ftype, **(env or {})), cfg, setup)
    c = {k: v for k, v in cols.items() if k not in ("sub_off", "sx", "sy", "inter_off", "inter_rows")}
    H.load_columns(c)
    H.set_subpoints_csr(cols["sub_off"], cols["sx"], cols["sy"])
    for i in range(sp.n_rows(cols)):
        H.set_interactions(i, sp.inter_of(cols, i))
    H._push_interactions()
    return H


# ---------------------------------------------------------------- edits
def _thinned(ring):
    """every other vertex of the ring (at least three stay)"""
    r = ring[:-1][::2]
    assert len(r) >= 3
    return np.concatenate([r, r[:1]])


def _changed(full, rows, how, dg, next_id):
    """the floes `rows` with their rings changed: how[k] in scaled / thinned / resampled / left (the left half of a cut); they keep their
    interaction rows"""
    fn = {"scaled": lambda r: sp.scaled(r, 0.9), "thinned": _thinned, "resampled": sp.resampled, "left": lambda r: sp.halves(r)[0]}
    rings = [fn[h](sp.ring_of(full, i)) for i, h in zip(rows, how)]
    return sp.floes_from(rings, sp.take(full, rows), np.arange(next_id, next_id + len(rows)), dg, inter=[sp.inter_of(full, i) for i in rows])


def _pieces(full, rows, dg, next_id, cut=sp.pieces3):
    rings, like = [], []
    for i in rows:
        p = cut(sp.ring_of(full, i))
        rings += p; like += [i] * len(p)
    return sp.floes_from(rings, sp.take(full, like), np.arange(next_id, next_id + len(rings)), dg)


def _tiny(full, i, dg, next_id):
    """two floes under min_floe_area = 1e6 inside floe i's outline (the floe itself is deleted by the edits that use this): the first is
    tagged `remove` -- the tag ends the batch's first step, and the removal pass that follows removes it and dissolves the second"""
    from subzero_jl_amd import capi
    t = sp.floes_from([sp.scaled(h, 0.05) for h in sp.halves(sp.ring_of(full, i))], sp.take(full, [i, i]), [next_id, next_id + 1], dg)
    t["status"][0] = capi.REMOVE
    assert np.all(t["area"] < 1e6)
    return t


def _join(*lists):
    lists = [l for l in lists if l is not None]
    return sp.apply(lists[0], append=None) if len(lists) == 1 else sp.apply(lists[0], append=_join(*lists[1:]))


def _edit(name, full, cfg, tiny=False):
    """(delete, replace, append) of the named edit on a list of at least 400 floes"""
    n, dg = sp.n_rows(full), cfg["dg"]
    nid = int(full["id"].max()) + 1
    right = lambda i: sp.halves(sp.ring_of(full, i))[1:]
    if name == "noop":
        e = ((), None, None)
    elif name.startswith("del_"):
        e = ({"del_first": [0], "del_last": [n - 1], "del_adjacent": [100, 101], "del_all_but_one": [i for i in range(n) if i != 7]}[name], None, None)
    elif name.startswith("rep_"):
        rows, how = {"rep_same": ([50], ["scaled"]), "rep_fewer": ([50], ["thinned"]), "rep_more": ([50], ["resampled"]), "rep_first": ([0], ["resampled"]),
                     "rep_last": ([n - 1], ["thinned"])}[name]
        e = ((), (rows, _changed(full, rows, how, dg, nid)), None)
    elif name == "append":
        e = ((), None, _pieces(full, [10], dg, nid, cut=lambda r: [sp.scaled(h, 0.5) for h in sp.halves(r)]))
    elif name == "fracture":
        e = ([10, 200, n - 1], None, _pieces(full, [10, 200, n - 1], dg, nid))
    elif name == "fuse":
        e = ([21, 301], ([20, 300], _changed(full, [20, 300], ["resampled", "scaled"], dg, nid)), None)
    elif name == "ridge":
        rows = [30, 31, 250, 251]
        e = ((), (rows, _changed(full, rows, ["left", "scaled", "left", "resampled"], dg, nid)), _pieces(full, [30, 250], dg, nid + 4, cut=lambda r: sp.halves(r)[1:]))
    elif name == "everything":
        rows = [7, 100, n - 1]
        e = ([5, 6, 390], (rows, _changed(full, rows, ["resampled", "thinned", "scaled"], dg, nid)), _pieces(full, [5, 390], dg, nid + 3, cut=sp.halves))
    else:
        raise KeyError(name)
    if tiny:          # (no edit above touches row 40)
        e = (sorted(list(e[0]) + [40]), e[1], _join(e[2], _tiny(full, 40, dg, nid + 50)))
    return e


SHAPES = ["noop", "del_first", "del_last", "del_adjacent", "del_all_but_one", "rep_same", "rep_fewer", "rep_more", "rep_first", "rep_last", "append",
          "fracture", "fuse", "ridge", "everything"]


def _spliced_and_fresh(field, shape, setup=None, env=None, tiny=False):
    D, cfg = _settled(field, setup, env)
    full = _full(D)
    delete, replace, append = _edit(shape, full, cfg, tiny)
    H = _fresh(cfg, sp.apply(full, delete, replace, append), setup, env)
    D.splice(delete, replace, append)
    return D, H, cfg


# ---------------------------------------------------------------- 1. rows down
SELECT = {"empty": lambda n, rng: [], "one": lambda n, rng: [n // 3], "all_reversed": lambda n, rng: list(range(n))[::-1],
          "random_37": lambda n, rng: list(rng.permutation(n)[:37]), "wavefront_edge": lambda n, rng: [63, 64, 65]}


@pytest.fixture(scope="module")
def settled_periodic():
    D, cfg = _settled("periodic")
    return D, _full(D)


@pytest.mark.parametrize("sel", list(SELECT))
def test_download_rows_equals_the_rows_of_a_full_download(settled_periodic, sel):
    D, full = settled_periodic
    assert full["inter_off"][-1] > 0 and np.count_nonzero(full["stress_accum"]) > 0
    rows = SELECT[sel](sp.n_rows(full), np.random.Generator(np.random.PCG64(2)))
    got = D.download_rows(rows)
    _assert_bit_equal(got, sp.take(full, rows), sel)
    _assert_bit_equal(_full(D), full, "a download changes nothing")


def test_download_rows_on_the_walls_field():
    D, cfg = _settled("walls")
    full = _full(D)
    rows = [399, 0, 17, 64, 63]
    _assert_bit_equal(D.download_rows(rows), sp.take(full, rows))


# ---------------------------------------------------------------- 2. every edit shape
@pytest.mark.parametrize("shape", SHAPES)
def test_splice_equals_upload_of_the_edited_list(shape):
    D, H, cfg = _spliced_and_fresh("periodic", shape)
    _assert_bit_equal(_state(D), _state(H), shape)


@pytest.mark.parametrize("shape", ["fracture", "everything"])
def test_splice_on_the_walls_field(shape):
    D, H, cfg = _spliced_and_fresh("walls", shape)
    _assert_bit_equal(_state(D), _state(H), shape)
    for w in (D, H):
        assert w.run(10, 20, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 10
    _assert_bit_equal(_state(D), _state(H), shape + ", 10 steps on")


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 256, 257])
def test_hand_lists_at_wavefront_and_workgroup_edges(n):
    """replace the last row by a ring of more points, delete the first (where there is more than one), append two floes in free lattice cells"""
    D, cfg = _settled("hand-%d" % n, steps=3)
    full = _full(D)
    _assert_bit_equal(D.download_rows(list(range(n))[::-1]), sp.take(full, list(range(n))[::-1]), "rows down")
    rep = _changed(full, [n - 1], ["resampled"], cfg["dg"], 1000)
    new = [_hand_ring(k, cfg["n_side"], cfg["spacing"], cfg["side"]) for k in (n, n + 1)]
    app = sp.floes_from(new, sp.take(full, [0, 0]), [2000, 2001], cfg["dg"])
    delete = [0] if n > 1 else []
    H = _fresh(cfg, sp.apply(full, delete, ([n - 1], rep), app))
    D.splice(delete, ([n - 1], rep), app)
    _assert_bit_equal(_state(D), _state(H), n)
    for w in (D, H):
        assert w.run(5, 3, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 5
    _assert_bit_equal(_state(D), _state(H), "%d, 5 steps on" % n)


# ---------------------------------------------------------------- 3. the steps behind an edit
def _mixed(w, cfg):
    w.set_precision("mixed")


def _two_way(w, cfg):
    w.set_two_way(True, dt=cfg["dt"]); w.set_temps(0.0, 0.0)


def _never_fractures(w, cfg):
    from subzero_jl_amd import capi
    w.set_fracture(capi.FRAC_POLYGON, dt=5, poly=fr.huge_square(), min_floe_area=1e6)


def _welding(w, cfg):
    w.set_welding([7], [2], [2])


def _removal(w, cfg):
    w.set_removal(True, max_vertices=2**31 - 1, min_floe_area=1e6, min_floe_height=0.1)


def _ridgeraft(w, cfg):
    w.set_ridgeraft(True, dt=10)


VARIANTS = {"pipelined": (None, None), "pipeline_off": (None, {"SZ_PIPELINE": "0"}), "mixed": (_mixed, None), "two_way": (_two_way, None),
            "fracture_never": (_never_fractures, None), "welding": (_welding, None), "removal": (_removal, None), "ridgeraft": (_ridgeraft, None)}


@pytest.mark.parametrize("shape", ["fracture", "fuse", "ridge"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_steps_behind_a_splice(variant, shape):
    """20 steps on both contexts (stops allowed: the same step count on both), everything compared again.  With removal set two appended floes
    lie under min_floe_area, one of them tagged `remove`, so a removal pass runs on spliced rows."""
    setup, env = VARIANTS[variant]
    D, H, cfg = _spliced_and_fresh("periodic", shape, setup, env, tiny=variant == "removal")
    _assert_bit_equal(_state(D), _state(H), (variant, shape))
    n0 = D.stats()["N"]
    done = [w.run(20, 21, cfg["dt"], coupling_dt=1) for w in (D, H)]
    print(variant, shape, "steps", done, "floes", n0, "->", D.stats()["N"], "pending", D.ridgeraft_pending())
    assert done[0] == done[1] and D.ridgeraft_pending() == H.ridgeraft_pending()
    if variant == "removal":
        assert D.stats()["N"] == n0 - 2, "no removal pass ran on the spliced rows"
    if variant in ("pipelined", "pipeline_off", "mixed", "two_way", "fracture_never"):
        assert done[0] == 20
    _assert_bit_equal(_state(D), _state(H), (variant, shape, "behind"))


# ---------------------------------------------------------------- 4. growth
def test_growth_of_rows_rings_and_points_at_once():
    """3 floes (2051 rows after the upload), 2100 triangles appended: rows, ring points and the sub-floe pool all outgrow the upload's"""
    D, cfg = _settled("hand-3-roomy", steps=3)
    full = _full(D)
    assert 2103 <= cfg["n_side"] ** 2
    new = [_hand_ring(k, cfg["n_side"], cfg["spacing"], cfg["side"], triangle=True) for k in range(3, 2103)]
    app = sp.floes_from(new, sp.take(full, [k % 3 for k in range(2100)]), np.arange(10, 2110), cfg["dg"])
    H = _fresh(cfg, sp.apply(full, append=app))
    D.splice(append=app)
    assert D.stats()["N"] == 2103
    _assert_bit_equal(_state(D), _state(H), "grown")
    for w in (D, H):
        assert w.run(5, 3, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 5
    _assert_bit_equal(_state(D), _state(H), "grown, 5 steps on")


def test_growth_of_the_point_pool_alone():
    D, cfg = _settled("periodic")
    full = _full(D)
    pool = full["sub_off"][-1]
    app = _pieces(full, [10], cfg["dg"], 5000, cut=lambda r: [sp.scaled(r, 0.3)])
    H = _fresh(cfg, sp.apply(full, [10], None, app))
    D.splice([10], None, app)           # one floe out, a smaller one in: rows and ring points fit ...
    _assert_bit_equal(_state(D), _state(H), "first")
    full = _full(D)
    app = _pieces(full, [20], cfg["dg"], 5001, cut=lambda r: [sp.resampled(r)])
    rep = sp.floes_from([sp.ring_of(app, 0)], sp.take(full, [20]), [5001], cfg["dg"] / 3.0)           # ... and one floe with nine times the points: the pool does not
    H = _fresh(cfg, sp.apply(full, (), ([20], rep), None))
    D.splice((), ([20], rep), None)
    assert D.stats()["n_sub_points"] > pool, "the pool of the upload still holds the points"
    _assert_bit_equal(_state(D), _state(H), "pool")
    for w in (D, H):
        assert w.run(10, 20, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 10
    _assert_bit_equal(_state(D), _state(H), "pool, 10 steps on")


# ---------------------------------------------------------------- 5. twice, then a removal pass
def test_two_splices_then_a_removal_pass_origin_composes():
    """origin is the identity behind a splice, as behind an upload; the pass then composes from there"""
    from subzero_jl_amd import capi
    D, cfg = _settled("periodic", _removal)
    full = _full(D)
    e1 = _edit("fracture", full, cfg)
    D.splice(*e1)
    one = sp.apply(full, *e1)
    assert np.array_equal(D.origin(), np.arange(sp.n_rows(one)))
    rep = _changed(one, [12], ["scaled"], cfg["dg"], 9000)
    rep["status"][:] = capi.REMOVE
    D.splice([3], ([12], rep), None)
    two = sp.apply(one, [3], ([12], rep), None)
    H = _fresh(cfg, two, _removal)
    _assert_bit_equal(_state(D), _state(H), "twice")
    n = sp.n_rows(two)
    assert np.array_equal(D.origin(), np.arange(n))
    for w in (D, H):
        assert w.remove_floes() == (True, 1, 0)
    assert np.array_equal(D.origin(), np.array([i for i in range(n) if i != 11]))          # (row 12 of the list before the deletion of row 3)
    _assert_bit_equal(_state(D), _state(H), "twice, then the pass")


# ---------------------------------------------------------------- 6. refusals
def _refused(w, code, needle, *edit):
    from subzero_jl_amd.capi import SzError
    before = _full(w)
    with pytest.raises(SzError) as e:
        w.splice(*edit)
    msg = str(e.value)
    head = "libsubzero_hip error %d: " % code
    assert msg.startswith(head) and len(msg) > len(head) + 8 and needle in msg, msg
    _assert_bit_equal(_full(w), before, "a refusal changes nothing")


def test_refusals_of_bad_edits():
    D, cfg = _settled("periodic")
    full = _full(D)
    n = sp.n_rows(full)
    ok = _changed(full, [50], ["scaled"], cfg["dg"], 7000)
    two = _changed(full, [50, 60], ["scaled", "scaled"], cfg["dg"], 7000)
    E_ARG = -2
    _refused(D, E_ARG, "ascending", [5, 3], None, None)
    _refused(D, E_ARG, "repeats", [5, 5], None, None)
    _refused(D, E_ARG, "outside", [n], None, None)
    _refused(D, E_ARG, "outside", [-1], None, None)
    _refused(D, E_ARG, "outside", (), ([n], ok), None)
    _refused(D, E_ARG, "ascending", (), ([60, 50], two), None)
    _refused(D, E_ARG, "both deleted and replaced", [50], ([50], ok), None)
    _refused(D, E_ARG, "no floe", list(range(n)), None, None)
    opened = {k: v.copy() for k, v in ok.items()}
    opened["vx"][-1] += 1.0
    _refused(D, E_ARG, "open ring", (), ([50], opened), None)
    th = np.linspace(0.0, -2.0 * np.pi, 300)
    ring = np.stack([full["cx"][50] + 5e3 * np.cos(th), full["cy"][50] + 5e3 * np.sin(th)], 1); ring[-1] = ring[0]
    long_ = sp.floes_from([ring], sp.take(full, [50]), [7000], cfg["dg"])
    _refused(D, E_ARG, "255", (), ([50], long_), None)
    _refused(D, E_ARG, "255", (), None, long_)
    # and the context still takes a good edit
    H = _fresh(cfg, sp.apply(full, (), ([50], ok), None))
    D.splice((), ([50], ok), None)
    _assert_bit_equal(_state(D), _state(H))


def test_refused_with_ghosts_in_the_list():
    D, cfg = _settled("periodic")
    D.add_ghosts()
    assert D.stats()["n_ghosts"] > 0
    _refused(D, -4, "sz_remove_ghosts", [0], None, None)


def test_refused_at_a_pending_ridge_raft_stop():
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=400, seed=7, subgrid_per_floe=4.0)
    w = fields.build_world(mk(), cfg)
    w.set_ridgeraft(True, dt=10)
    w.run(30, 1, cfg["dt"], coupling_dt=1)
    assert w.ridgeraft_pending() >= 0, "the dense field did not stop at a ridge / raft step"
    _refused(w, -4, "sz_step_finish", [0], None, None)


def test_refused_on_a_tiled_context():
    from subzero_jl_amd import tiles
    from subzero_jl_amd.capi import SzError
    cfg = _cfg("periodic")
    tw = tiles.TiledWorld(cfg, 0, 1, 0, None, backend="library", rebox_every=20)
    before = _full(tw.world)
    with pytest.raises(SzError) as e:
        tw.splice([0], None, None)
    assert str(e.value).startswith("libsubzero_hip error -4: ") and "tiled" in str(e.value)
    _assert_bit_equal(_full(tw.world), before)


# ---------------------------------------------------------------- 7. Float32 hosts
def test_f32_twins_fracture_edit():
    """a Floe{Float32} host: rows down and the fracture edit back through the _f32 twins, against the _f32 upload of the edited list"""
    D, cfg = _settled("periodic", ftype=np.float32)
    full = _full(D)
    rows = [10, 200, 399]
    _assert_bit_equal(D.download_rows(rows), sp.take(full, rows), "rows down")
    delete, replace, append = _edit("fracture", full, cfg)
    H = _fresh(cfg, sp.apply(full, delete, replace, append), ftype=np.float32)          # (both worlds round the new floes to Float32 on the way in)
    D.splice(delete, replace, append)
    _assert_bit_equal(_state(D), _state(H), "f32")          # (as a Float32 host sees both; the rows a splice keeps stay doubles on the device, an upload rounds all)

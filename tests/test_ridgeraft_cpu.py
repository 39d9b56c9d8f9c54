"""The ridge / raft candidate rule (tests/ridgeraft_ref.py) on the oracle: the reference's own scenarios land in the table with the
kind its test expects, the literal loop of ridge_raft.jl:687-753 never lists a pair the table lacks, and an empty table means a call that is
nothing but the per-floe draws."""
import numpy as np
import pytest

import cases
import ridgeraft_ref as rr

pytestmark = pytest.mark.filterwarnings("ignore")


def _oracle():
    from oracle import orc
    return orc.World()


def golden_world(w, g, group):
    """the floes of a fixture group after add_ghosts! + timestep_collisions!, all active (test_ridge_raft.jl:28-62)"""
    G = g[group]
    dom = g[G["domain"]]
    w.set_consts()
    w.set_settings(floe_floe_max_overlap=g["floe_floe_max_overlap"])
    cases.set_domain(w, dom["kinds"], g["grid"], dom["topography"])
    shift = G.get("shift", [[0.0, 0.0]] * len(G["coords"]))
    for c, s in zip(G["coords"], shift):
        w.add_floe(cases.closed(c) + np.array(s), G["initial_height"])
    w.add_ghosts()
    w.timestep_collisions(len(G["coords"]), g["dt"])
    w.set_status(np.full(w.M, rr.ACTIVE, np.int32))
    return w, dom["topography"]


def _with_heights(w, heights):
    h = w.get("height")
    h[:len(heights)] = heights
    w.set("height", h)


def check_golden(mk):
    g = rr.golden()
    G = g["floe_floe"]
    w, topo = golden_world(mk(), g, "floe_floe")
    pair = tuple(G["pair"])
    for sc in G["scenarios"]:
        s = dict(g["defaults"], **sc["settings"])
        _with_heights(w, sc["heights"])
        tab = {(i, j): k for i, j, k, _ in rr.table(w, s, topo)[0]}
        if sc["expects"] == "ridge":
            assert tab.get(pair, 0) & rr.RIDGE, sc["name"]
        elif sc["expects"] == "raft":
            assert tab.get(pair, 0) & rr.RAFT, sc["name"]
        else:
            assert not tab.get(pair, 0) & rr.RIDGE, sc["name"]
            s2 = dict(s, **sc["rafting_impossible_by_height"])
            assert pair not in {(i, j) for i, j, _, _ in rr.table(w, s2, topo)[0]}, sc["name"]
    G = g["floe_domain"]
    w, topo = golden_world(mk(), g, "floe_domain")
    for sc in G["scenarios"]:
        s = dict(g["defaults"], **sc["settings"])
        _with_heights(w, sc["heights"])
        tab = {(i, j): k for i, j, k, _ in rr.table(w, s, topo)[0]}
        for p in map(tuple, G["pairs"]):
            k = tab.get(p, 0)
            if sc["expects"] == "ridge":
                assert k & rr.RIDGE, (sc["name"], p)
            elif sc["expects"] == "raft":
                assert k & rr.RAFT, (sc["name"], p)
            elif sc["expects"] == "no ridge":
                assert not k & rr.RIDGE, (sc["name"], p)
            else:
                assert not k & rr.RAFT, (sc["name"], p)


def test_golden_scenarios():
    check_golden(_oracle)


def field(kind, n=300, seed=11, **over):
    from subzero_jl_amd import fields
    if kind == "periodic":
        return fields.make_config(n_floes=n, seed=seed, subgrid_per_floe=4.0, **over)
    return fields.make_config(n_floes=n, seed=seed, subgrid_per_floe=4.0, walls=True, topography=True, ocean="strait", **over)


def stepped(cfg, nsteps=30, heights=None):
    """an oracle `nsteps` into the field, then add_ghosts! + timestep_collisions!: the state timestep_ridging_rafting! is called on"""
    from subzero_jl_amd import fields
    w = fields.build_world(_oracle(), cfg)
    for t in range(nsteps):
        w.timestep_sim(t, cfg["dt"], coupling_dt=1)
    n = w.M
    if heights is not None:
        w.set("height", heights(w.get("height")))
    w.add_ghosts()
    w.timestep_collisions(n, cfg["dt"])
    return w


@pytest.mark.parametrize("kind", ["periodic", "walled"])
def test_literal_loop_lists_a_subset(kind):
    cfg = field(kind)
    rng = np.random.default_rng(5)
    # heights on both sides of the thresholds, so that every kind and the empty kind occur
    w = stepped(cfg, heights=lambda h: rng.choice([0.1, 0.2, 0.25, 0.3, 1.0, 1.25, 2.0, 5.0, 6.0], len(h)))
    if kind == "periodic":
        assert w.M > cfg["n_floes"], "no ghosts in the list"
    topo = cfg["topography"]
    tab, nd = rr.table(w, rr.SETTINGS, topo)
    tset = {(i, j, k) for i, j, k, _ in tab}
    assert len(tset) == len(tab) > 20
    lists, stale, ndraws = rr.literal_lists(w, rr.SETTINGS, topo, draw=lambda: 0.0)
    assert ndraws == nd
    acted = set(rr.acted_on(w, lists, rr.SETTINGS, topo))
    assert acted <= tset
    extra = {(i, j) for i, j, _ in tset - acted}
    assert extra <= set(stale), sorted(extra - set(stale))[:5]
    # with real draws the loop acts on no more
    for seed in range(5):
        r = np.random.default_rng(seed)
        lists, _, ndraws = rr.literal_lists(w, rr.SETTINGS, topo, draw=r.random)
        assert ndraws == nd
        kinds = {(i, j): k for i, j, k in tset}
        assert all(kinds.get((i, j), 0) & k == k for i, j, k in rr.acted_on(w, lists, rr.SETTINGS, topo))
    print(f"{kind}: {len(tab)} table entries, {len(extra)} of them behind a stale buffer entry, {nd} draws over {w.M} rows")


EMPTY = {"sparse": (dict(concentration=0.1), None), "too_thick": ({}, lambda h: np.full(len(h), 6.0))}


@pytest.mark.parametrize("name", list(EMPTY))
def test_empty_table_means_only_the_draws(name):
    over, heights = EMPTY[name]
    cfg = field("periodic", **over)
    w = stepped(cfg, heights=heights)
    tab, nd = rr.table(w, rr.SETTINGS, None)
    assert tab == []
    assert nd == rr.n_draws(w.get("height"), rr.SETTINGS) == (0 if name == "too_thick" else 2 * w.M)
    if name == "too_thick":
        assert w.interactions()[0][-1] > 100, "the dense field has no rows"
    for seed in range(20):
        r = np.random.default_rng(seed)
        lists, _, ndraws = rr.literal_lists(w, rr.SETTINGS, None, draw=r.random)
        assert ndraws == nd
        assert rr.acted_on(w, lists, rr.SETTINGS, None) == []
        assert all(len(v) == 0 for v in lists.values())


def test_ridgeraft_entry_points_mirror_header_capi_and_julia():
    """every new entry point is declared in the header, exported by the ctypes binding with the header's argument count, and bound in Julia"""
    import os
    import re
    from subzero_jl_amd import capi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "subzero_hip.h")).read()
    jl = open(os.path.join(root, "julia", "SubzeroHIP.jl")).read()
    L = capi.load()
    for fn, nargs in (("sz_set_ridgeraft", 8), ("sz_ridgeraft_candidates", 8), ("sz_ridgeraft_pending", 2), ("sz_ridgeraft_draws", 2),
                      ("sz_step_finish", 5)):
        d = re.search(rf"\nint {fn}\(([^;]*)\);", hdr)
        assert d and d.group(1).count(",") + 1 == nargs, fn
        assert fn in capi.EXPORTS, fn
        assert len(getattr(L, fn).argtypes) == nargs, fn
        assert re.search(rf"@ccall lib\.{fn}\(", jl), fn
    body = jl[jl.index("function run_resident!"):]
    body = body[:body.index("\nend\n")]
    assert "set_ridgeraft!(eng, sim)" in body and "sz_step_finish" in body and "timestep_ridging_rafting!" in body
    assert body.index("ridgeraft_draws(eng)") < body.index("fracture_floes!"), "sim.rng is advanced before the host processes use it"

#!/usr/bin/env python3
"""The outflow case of tests/test_remove_gpu.py::test_batch_runs_past_removals, walked on the CPU: the oracle steps, tests/remove_ref.py
deletes, and the steps on which floes leave are printed.  The test needs removals on at least three different steps within 80, at least
one step that removes two or more floes, no fuse tag and no ring over 30 points; its docstring quotes what this prints.  No GPU.

    python tools/removal_case.py [--steps 60]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def oracle_from_cols(cols, cfg, extent):
    """a fresh oracle holding the columns (tests/parity.oracle_from, from a dict instead of a world)"""
    from oracle import orc
    from subzero_jl_amd import fields
    none = np.zeros(0)
    ow = fields.build_world(orc.World(), dict(cfg, n_floes=0, u=none, v=none, xi=none))
    x0, xf, y0, yf = extent
    ow.set_domain([fields.KIND[k] for k in cfg["kinds"]], x0, xf, y0, yf)
    ow.set_grid_fields(cfg["Nx"], cfg["Ny"], x0, xf, y0, yf, cfg["uo"], cfg["vo"], cfg["hf"], cfg["ua"], cfg["va"])
    off, so = cols["vert_off"], cols["sub_off"]
    n = len(cols["cx"])
    for i in range(n):
        ow.add_floe(np.stack([cols["vx"][off[i]:off[i + 1]], cols["vy"][off[i]:off[i + 1]]], 1), cols["height"][i])
        ow.set_subpoints(i, cols["sx"][so[i]:so[i + 1]], cols["sy"][so[i]:so[i + 1]])
    for f in orc.FIELDS:
        for pre, full in (("sa", "stress_accum"), ("si", "stress_instant"), ("e", "strain")):
            if f.startswith(pre) and f[len(pre):] in ("11", "12", "21", "22"):
                ow.set(f, cols[full][:, ("11", "12", "21", "22").index(f[len(pre):])])
                break
        else:
            ow.set(f, cols[f])
    ow.set_ids(cols["id"]); ow.set_status(cols["status"])
    return ow


def cols_of(ow, sub):
    from oracle import orc
    from subzero_jl_amd import capi
    c = {n: ow.get(n) for n in capi.DCOLS}
    for pre, full in (("sa", "stress_accum"), ("si", "stress_instant"), ("e", "strain")):
        c[full] = np.stack([ow.get(pre + q) for q in ("11", "12", "21", "22")], 1)
    c["id"], c["ghost_id"], c["status"] = ow.ids()
    off, x, y = ow.rings()
    c["vert_off"], c["vx"], c["vy"] = off, x, y
    c["sub_off"], c["sx"], c["sy"] = sub
    assert not np.any(c["ghost_id"]) and set(orc.FIELDS) >= set(capi.DCOLS)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    import parity
    import remove_ref as rr
    import test_remove_gpu as T
    cfg, extent = T.outflow_case()
    d = cfg["derived"]
    cols = dict(cx=d["cx"], cy=d["cy"], rmax=d["rmax"], area=d["area"], height=d["height"], mass=d["mass"], moment=d["moment"], u=cfg["u"], v=cfg["v"],
                xi=cfg["xi"], vert_off=cfg["vert_off"], vx=cfg["vx"], vy=cfg["vy"], sub_off=cfg["sub_off"], sx=cfg["sx"], sy=cfg["sy"])
    n = cfg["n_floes"]
    from subzero_jl_amd import capi
    for k in capi.DCOLS:
        cols.setdefault(k, np.zeros(n))
    for k in capi.TCOLS:
        cols[k] = np.zeros((n, 4))
    cols["id"] = np.arange(1, n + 1, dtype=np.int64); cols["status"] = np.full(n, rr.ACTIVE, np.int32)
    ow = oracle_from_cols(cols, cfg, extent); ow.set_threads(parity.cores())
    sub = (cols["sub_off"], cols["sx"], cols["sy"])
    grid = (cfg["Nx"], cfg["Ny"]) + tuple(extent)
    lattice = np.zeros((cfg["Nx"] + 1, cfg["Ny"] + 1))
    events, fuse_seen, longest = [], False, int(np.diff(cols["vert_off"]).max())
    for t in range(args.steps):
        ow.timestep_sim(t, cfg["dt"], coupling_dt=1)
        st = ow.ids()[2]
        if np.all(st == rr.ACTIVE):
            continue
        fuse_seen = fuse_seen or bool(np.any(st == rr.FUSE))
        c = cols_of(ow, sub)
        longest = max(longest, int(np.diff(c["vert_off"]).max()))
        if t == args.steps - 1:
            print(f"step {t}: tags on the batch's own last step are left to the caller")
            break
        new, kept, nr, nd = rr.remove_ref(c, grid, False, False, lattice)
        events.append((t, nr, nd))
        print(f"step {t}: {nr} removed, {nd} dissolved, {len(kept)} floes stay")
        sub = (new["sub_off"], new["sx"], new["sy"])
        ow = oracle_from_cols(new, cfg, extent); ow.set_threads(parity.cores())
    print(f"{len(events)} steps with removals in {args.steps}: {[e[0] for e in events]}; most on one step: {max([e[1] + e[2] for e in events], default=0)}; "
          f"{sum(e[1] + e[2] for e in events)} floes in all; fuse tag seen: {fuse_seen}; longest ring: {longest} points; U_OUT = {T.U_OUT}, XF_MARGIN = {T.XF_MARGIN}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The two cases of tests/test_remove_tiles_gpu.py (tests/remove_tiles_cases.py), walked on the CPU: the oracle steps the ONE global floe list,
tests/remove_ref.py deletes, and per event the step, the counts and the ranks that own the leaving floes are printed -- a floe's owner is the
tile of tiles.assign_tiles that held its centroid at the start (a TiledWorld keeps its floes unless it is told to migrate), for 2 and for 4
ranks.  The tests' docstrings quote what this prints.  No GPU.

    python tools/removal_tile_case.py [--case a|b|both]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))


def start_cols(cfg):
    from subzero_jl_amd import capi
    import remove_ref as rr
    d, n = cfg["derived"], cfg["n_floes"]
    cols = dict(cx=d["cx"], cy=d["cy"], rmax=d["rmax"], area=d["area"], height=d["height"], mass=d["mass"], moment=d["moment"], u=cfg["u"], v=cfg["v"],
                xi=cfg["xi"], vert_off=cfg["vert_off"], vx=cfg["vx"], vy=cfg["vy"], sub_off=cfg["sub_off"], sx=cfg["sx"], sy=cfg["sy"])
    for k in capi.DCOLS:
        cols.setdefault(k, np.zeros(n))
    for k in capi.TCOLS:
        cols[k] = np.zeros((n, 4))
    cols["id"] = np.arange(1, n + 1, dtype=np.int64); cols["status"] = np.full(n, rr.ACTIVE, np.int32)
    return cols


def walk(cfg, steps, run, upto=None):
    """yields (step, columns with the tags of that step, lattice before the pass) per event; applies remove_ref and goes on.  The generator's
    return value is not used: the last columns are yielded as (None, columns, lattice)."""
    import parity
    import remove_ref as rr
    from removal_case import cols_of, oracle_from_cols
    extent = (0.0, cfg["L"], 0.0, cfg["L"])
    grid = (cfg["Nx"], cfg["Ny"]) + extent
    cols = start_cols(cfg)
    ow = oracle_from_cols(cols, cfg, extent); ow.set_threads(parity.cores())
    sub = (cols["sub_off"], cols["sx"], cols["sy"])
    lattice = np.zeros((cfg["Nx"] + 1, cfg["Ny"] + 1))
    for t in range(steps):
        ow.timestep_sim(t, cfg["dt"], **run)
        st = ow.ids()[2]
        if np.all(st == rr.ACTIVE) or t == steps - 1:
            continue
        c = cols_of(ow, sub)
        yield t, c, lattice
        if upto is not None and t >= upto:
            return
        new, kept, nr, nd = rr.remove_ref(c, grid, False, False, lattice)
        sub = (new["sub_off"], new["sx"], new["sy"])
        ow = oracle_from_cols(new, cfg, extent); ow.set_threads(parity.cores())
    yield None, cols_of(ow, sub), lattice


def report(name, cfg, steps, run):
    import remove_ref as rr
    import remove_tiles_ref as rt
    from subzero_jl_amd import tiles
    d = cfg["derived"]
    own = {w: tiles.assign_tiles(d["cx"], d["cy"], cfg["L"], w) for w in (2, 4)}
    print(f"case {name}: {cfg['n_floes']} floes, {steps} steps; owners for 2 ranks: {np.bincount(own[2], minlength=2)}, for 4: {np.bincount(own[4], minlength=4)}")
    if cfg["n_floes"] <= 16:
        print(f"  owners under assign_tiles(.., 2): {own[2]}")
    events, fuse, longest, total = [], False, int(np.diff(cfg["vert_off"]).max()), 0
    for t, c, lattice in walk(cfg, steps, run):
        longest = max(longest, int(np.diff(c["vert_off"]).max()))
        if t is None:
            ids = c["id"] - 1
            print(f"  {len(ids)} floes stay" + (f": rows {[int(i) for i in ids]} of the start" if len(ids) <= 16 else "") +
                  f"; per rank {np.bincount(own[2][ids], minlength=2)} for 2 ranks, {np.bincount(own[4][ids], minlength=4)} for 4")
            if len(ids) <= 16:
                print(f"  new numbers per rank, 2 ranks: {[[int(i) for i in np.nonzero(own[2][ids] == r)[0]] for r in range(2)]}")
                print(f"  overarea of the floes that stay: {c['overarea']}")
            nz = np.nonzero(lattice)
            print(f"  lattice from zero: {[(int(i), int(j), float(lattice[i, j])) for i, j in zip(*nz)][:8]}" + (f" (2^53 + 2 = {float(2 ** 53 + 2)})" if name == "A" else ""))
            break
        fuse = fuse or bool(np.any(c["status"] == rr.FUSE))
        dis, rem = rt.flags(c, 1e6, 0.1)
        ids = c["id"] - 1
        events.append(t); total += int(dis.sum() + rem.sum())
        who = lambda w, m: sorted(set(int(o) for o in own[w][ids[m]]))
        print(f"  behind step {t}: {int(rem.sum())} removed, {int(dis.sum())} dissolved" +
              (f" (rows {[int(i) for i in np.nonzero(rem)[0]]} / {[int(i) for i in np.nonzero(dis)[0]]} of the list then)" if cfg["n_floes"] <= 16 else "") +
              f"; ranks that lose floes: {who(2, dis | rem)} of 2, {who(4, dis | rem)} of 4" +
              (f"; dissolving floes per rank of 2: {np.bincount(own[2][ids[dis]], minlength=2)}" if dis.any() else ""))
    print(f"  events behind steps {events}; {total} floes leave in all; fuse tag seen: {fuse}; longest ring: {longest} points")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["a", "b", "both"])
    args = ap.parse_args()
    import remove_tiles_cases as cases
    if args.case in ("a", "both"):
        report("A", cases.case_a(), cases.A_STEPS, cases.A_RUN)
    if args.case in ("b", "both"):
        report("B", cases.case_b(), cases.B_STEPS, cases.B_RUN)


if __name__ == "__main__":
    main()

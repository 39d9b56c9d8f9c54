"""Cost of a removal event in resident batches (sz_set_removal; csrc/sz_remove.hpp) against the host loop it replaces, on the configs[1] field
at n floes between four open boundaries with an outflow: the east boundary a few metres beyond the easternmost vertex, every floe `u_out` m/s
faster eastwards, so that floes reach the boundary one after another and are tagged `remove` (collisions.jl:436-439).
Two arms, each from a fresh upload of the same field, timed in alternating rounds of `steps` steps (wall clock around the whole loop):
  host     the loop a resident run made before: run(); on a stop download the state (columns, rings, sub-floe points), delete the tagged rows
           with numpy (one vectorised pass: cheaper than simplify_floes!), upload again; go on
  device   set_removal(), then run() -- the batch goes on past every removal
and on one relaxed state with `k` floes tagged by hand: the wall time of one remove_floes() call (its kernels alone: run this tool under a kernel
trace) beside the wall time of the download, delete and upload of the same state.  The comparison is between the two arms of the same run.
Prints one JSON line.
usage: python tools/removal_overhead.py [n_floes] [steps] [rounds] [u_out]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import subzero_jl_amd  # noqa: E402
from subzero_jl_amd import capi, fields  # noqa: E402


def build(cfg, extent):
    w = fields.build_world(subzero_jl_amd.World(0), cfg)
    x0, xf, y0, yf = extent
    w.set_domain([fields.KIND[k] for k in cfg["kinds"]], x0, xf, y0, yf)
    w.set_grid_fields(cfg["Nx"], cfg["Ny"], x0, xf, y0, yf, cfg["uo"], cfg["vo"], cfg["hf"], cfg["ua"], cfg["va"])
    return w


def pull(w):
    w._host_stale = True
    c = {n: w.get(n) for n in capi.DCOLS}
    for n, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        c[n] = np.stack([w.get(pre + q) for q in ("11", "12", "21", "22")], 1)
    c["id"], c["ghost_id"], c["status"] = w.ids()
    c["vert_off"], c["vx"], c["vy"] = w.rings()
    c["sub_off"], c["sx"], c["sy"] = w.subpoints()
    return c


def delete_rows(c, keep):
    """the rows of `keep` (a mask) with their rings and sub-floe points, every status active"""
    out = {k: v[keep] for k, v in c.items() if k not in ("vert_off", "vx", "vy", "sub_off", "sx", "sy")}
    out["status"] = np.full(int(keep.sum()), capi.ACTIVE, np.int32)
    for off, members in (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy"))):
        cnt = np.diff(c[off])
        pts = np.repeat(keep, cnt)
        for m in members:
            out[m] = c[m][pts]
        out[off] = np.concatenate([[0], np.cumsum(cnt[keep])]).astype(np.int32)
    return out


def host_rebuild(w):
    c = pull(w)
    keep = c["status"] != capi.REMOVE
    new = delete_rows(c, keep)
    sub = [new.pop(k) for k in ("sub_off", "sx", "sy")]
    w.load_columns(new); w.set_subpoints_csr(*sub)
    w._push()
    return int((~keep).sum())


def run_host(w, steps, dt):
    t, events, removed = 0, 0, 0
    a = time.perf_counter()
    while t < steps:
        t += max(w.run(steps - t, t, dt, coupling_dt=1), 1)
        if t < steps:
            removed += host_rebuild(w); events += 1
    return time.perf_counter() - a, events, removed


def run_device(w, steps, dt):
    n0 = w.N
    a = time.perf_counter()
    t = 0
    while t < steps:          # (a batch still ends where the host is needed: a fuse tag)
        t += max(w.run(steps - t, t, dt, coupling_dt=1), 1)
        if t < steps:
            host_rebuild(w)
    return time.perf_counter() - a, n0 - w.N


def main():
    args = sys.argv[1:]
    n = int(args[0]) if len(args) > 0 else 10000
    steps = int(args[1]) if len(args) > 1 else 600
    rounds = int(args[2]) if len(args) > 2 else 5
    u_out = float(args[3]) if len(args) > 3 else 5.0
    cfg = fields.make_config(n_floes=n, seed=12345)
    cfg["kinds"] = ["open"] * 4
    cfg["u"] = cfg["u"] + u_out
    L = cfg["L"]
    extent = (-L, float(cfg["vx"].max()) + 25.0, -L, 2.0 * L)
    dt = cfg["dt"]
    ms = {"host": [], "device": []}
    events, removed = [], {"host": [], "device": []}
    for r in range(rounds + 1):                      # round 0 warms up (code objects, first batches) and is not counted
        for arm in ("host", "device"):
            w = build(cfg, extent)
            if arm == "device":
                w.set_removal(True, max_vertices=30)
            w._push(); w.stats()
            if arm == "host":
                s, ev, rm = run_host(w, steps, dt)
            else:
                s, rm = run_device(w, steps, dt); ev = None
            if r:
                ms[arm].append(1e3 * s / steps); removed[arm].append(rm)
                if ev is not None:
                    events.append(ev)
            del w
    med = {k: float(np.median(v)) for k, v in ms.items()}
    ev_med = float(np.median(events)) if events else 0.0
    # one pass against one host rebuild on the same relaxed state, k floes tagged by hand
    k = 4
    per = {"pass_us": [], "host_rebuild_us": []}
    for rep in range(6):
        for arm in ("pass_us", "host_rebuild_us"):
            w = build(cfg, extent)
            w.set_removal(True, max_vertices=30)
            w.run(20, 0, dt, coupling_dt=1, stop_on_tags=False)
            st = w.ids()[2]; st[:] = capi.ACTIVE; st[np.linspace(0, w.N - 1, k).astype(int)] = capi.REMOVE
            w.set_status(st); w._push(); w.stats()
            a = time.perf_counter()
            if arm == "pass_us":
                done = w.remove_floes()
                assert done[0] and done[1] == k
            else:
                assert host_rebuild(w) == k
                w.stats()
            if rep:
                per[arm].append(1e6 * (time.perf_counter() - a))
            del w
    out = dict(n_floes=n, steps_per_round=steps, rounds=rounds, u_out=u_out, ms_per_step_median=med,
               ms_per_step_all={a: [round(x, 5) for x in v] for a, v in ms.items()}, host_events_median=ev_med, floes_removed=removed,
               per_event_saving_us=(1e3 * (med["host"] - med["device"]) * steps / ev_med) if ev_med else None,
               one_pass_wall_us_median=float(np.median(per["pass_us"])), one_host_rebuild_wall_us_median=float(np.median(per["host_rebuild_us"])),
               floes_tagged_in_the_one_pass=k)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Cost of ridge / raft in resident batches (sz_set_ridgeraft; csrc/sz_ridgeraft.hpp), configs[1] field (periodic box, uniform flow) at n floes
after 50 relaxation steps.  Three arms on the same field, timed in alternating rounds of `steps` steps (wall clock around sz_step, which
returns after its device synchronise):
  off       ridge / raft off, the default path (pipelined steps)
  empty     dt = 150 with maxima under every height (every table is empty): the cut before the ridge / raft step, the split step through the
            process calls and the candidate pass -- what ridge / raft costs a run between two stops
  default   dt = 150 with the reference's default thresholds.  A stop is answered as a host without work would: finish_step, and on (the
            host's ridging itself is not timed: it is the reference's)
and the share of stopping steps: the default thresholds with dt = `share_dt` (default 10) over `share_steps` more steps -- how many ridge / raft
steps had a non-empty table, and the table sizes.  Prints one JSON line.
usage: python tools/ridgeraft_overhead.py [n_floes] [steps] [rounds] [share_dt] [share_steps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import subzero_jl_amd  # noqa: E402
from subzero_jl_amd import fields  # noqa: E402


def run(w, steps, t0, dt, tables=None):
    """steps timestep_sim! from tstep t0 -> seconds.  Batches end on tags (the rest is run as the next batch) and in the middle of ridge / raft
    steps with candidates (finished at once; tables, if given, collects their sizes)"""
    a = time.perf_counter()
    done = 0
    while done < steps:
        k = w.run(steps - done, t0 + done, dt, coupling_dt=1)
        done += k
        p = w.ridgeraft_pending()
        if p >= 0:
            if tables is not None:
                tables.append(int(len(w.ridgeraft_candidates()[0])))
            w.finish_step(p, dt, coupling_dt=1)
            done += 1
        elif k == 0:
            done += 1          # (a batch that could not start: do not spin)
    return time.perf_counter() - a


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 10000
    steps = int(args[1]) if len(args) > 1 else 300
    rounds = int(args[2]) if len(args) > 2 else 5
    share_dt = int(args[3]) if len(args) > 3 else 10
    share_steps = int(args[4]) if len(args) > 4 else 300
    cfg = fields.make_config(n_floes=n, seed=12345)
    arms = {k: fields.build_world(subzero_jl_amd.World(0), cfg) for k in ("off", "empty", "default")}
    below = 0.5 * float(np.min(cfg["height"]))
    arms["empty"].set_ridgeraft(True, dt=150, min_ridge_height=below, max_floe_ridge_height=below, max_domain_ridge_height=below,
                                max_floe_raft_height=below, max_domain_raft_height=below)
    arms["default"].set_ridgeraft(True, dt=150)
    t = {}
    for k, w in arms.items():                      # relaxation (and warm-up: code objects, lists, first batch); tsteps 1 .. 50
        run(w, 50, 1, cfg["dt"]); t[k] = 51
    ms = {k: [] for k in arms}
    tables = {k: [] for k in arms}
    for _ in range(rounds):
        for k, w in arms.items():
            s = run(w, steps, t[k], cfg["dt"], tables[k]); t[k] += steps
            ms[k].append(1e3 * s / steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    # the share of ridge / raft steps that stop, on the relaxed dense field
    w = arms["default"]
    w.set_ridgeraft(True, dt=share_dt)
    sizes = []
    first = t["default"]
    run(w, share_steps, first, cfg["dt"], sizes)
    n_rr = len([s for s in range(first, first + share_steps) if s % share_dt == 0])
    out = dict(n_floes=n, steps_per_round=steps, rounds=rounds, ridgeraft_dt=150, ms_per_step_median=med,
               ms_per_step_all={k: [round(x, 5) for x in v] for k, v in ms.items()},
               empty_overhead_pct=100.0 * (med["empty"] / med["off"] - 1.0), default_overhead_pct=100.0 * (med["default"] / med["off"] - 1.0),
               default_stops=len(tables["default"]), default_table_sizes=tables["default"], empty_stops=len(tables["empty"]),
               share=dict(dt=share_dt, steps=share_steps, ridgeraft_steps=n_rr, stopped=len(sizes),
                          table_min=int(min(sizes)) if sizes else 0, table_median=float(np.median(sizes)) if sizes else 0.0,
                          table_max=int(max(sizes)) if sizes else 0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

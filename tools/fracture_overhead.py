"""Cost of a fracture criterion in resident batches (sz_set_fracture; csrc/sz_fracture.hpp), configs[1] field (periodic box,
uniform flow) at n floes, FractureSettings.Δt = 75, a criterion that is never met (pstar = 1e30: every batch runs to its end).
Three contexts on the same field, timed in alternating rounds of `steps` steps (wall clock around sz_step, which returns after
its device synchronise):
  off_pipe   SZ_FRAC_OFF, the default path (pipelined steps where eligible)
  off_3l     SZ_FRAC_OFF with SZ_PIPELINE=0: the three-launch steps
  hibler     HIBLER set: the three-launch steps + the criterion launches every Δt steps
hibler - off_3l isolates the fracture launches; hibler - off_pipe is what a criterion costs a user, falling back to three-launch
steps included.  Prints one JSON line.
usage: python tools/fracture_overhead.py [n_floes] [steps] [rounds]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import subzero_jl_amd  # noqa: E402
from subzero_jl_amd import capi, fields  # noqa: E402


def world(cfg, **env):
    for k, v in env.items():
        os.environ[k] = v
    try:
        return fields.build_world(subzero_jl_amd.World(0), cfg)
    finally:
        for k in env:
            del os.environ[k]


BATCHES = {}


def run(w, steps, t0, dt):
    """steps timestep_sim! from tstep t0 (batches end on tags: the rest is run as the next batch) -> seconds"""
    a = time.perf_counter()
    done = 0
    while done < steps:
        k = w.run(steps - done, t0 + done, dt, coupling_dt=1)
        done += max(k, 1)
        BATCHES[id(w)] = BATCHES.get(id(w), 0) + 1
    return time.perf_counter() - a


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    cfg = fields.make_config(n_floes=n, seed=12345)
    arms = {"off_pipe": world(cfg), "off_3l": world(cfg, SZ_PIPELINE="0"), "hibler": world(cfg)}
    # (an unstressed floe's σ-point (0, 0) is the Hibler ring's first vertex up to rounding: covered or not by the last bits of p -- the
    #  pstar is nudged until the device finds no candidate on the field)
    pstar = 1e30
    for _ in range(100):
        arms["hibler"].set_fracture(capi.FRAC_HIBLER, dt=75, pstar=pstar, min_floe_area=1e6)
        if len(arms["hibler"].fracture_candidates()) == 0:
            break
        pstar *= 1.001
    t = {k: 0 for k in arms}
    for k, w in arms.items():                      # warm-up: code objects, lists, first batch
        run(w, 20, 0, cfg["dt"]); t[k] = 20
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, w in arms.items():
            s = run(w, steps, t[k], cfg["dt"]); t[k] += steps
            ms[k].append(1e3 * s / steps)
    pipelined = {k: bool(w.pipelined()) for k, w in arms.items()}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = dict(n_floes=n, steps_per_round=steps, rounds=rounds, frac_dt=75, pstar=pstar,
               batches={k: BATCHES.get(id(w), 0) for k, w in arms.items()}, ms_per_step_median=med,
               ms_per_step_all={k: [round(x, 5) for x in v] for k, v in ms.items()}, pipelined=pipelined,
               fracture_launch_overhead_pct=100.0 * (med["hibler"] / med["off_3l"] - 1.0),
               vs_default_path_pct=100.0 * (med["hibler"] / med["off_pipe"] - 1.0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

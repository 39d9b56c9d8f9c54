"""Cost of welding in resident batches (sz_set_welding; csrc/sz_weld.hpp), configs[1] field (periodic box, uniform flow) at n floes after 50
relaxation steps.  Three measurements on the same field, the first two timed in alternating rounds of `steps` steps (wall clock around sz_step,
which returns after its device synchronise):
  off      welding off, the default path (pipelined steps)
  never    dts = [100] with a max_weld_area under every floe: every welding step runs the pass's bins and search, finds no candidate pair, and the
           batch goes on -- what welding costs a run between two welds (the segments, one host round trip per welding step)
  pass     sz_weld_overlaps on the dense state, unlimited max_weld_area, count only: bins, search, sort, clips, table and the two host
           synchronisations of one pass, wall clock per call (the kernels alone: run this tool under a kernel trace)
and, with --host, what the host side of the same table costs on this machine's CPU: the oracle's intersect_polys port (orc.clip) over the same
candidate pairs, one thread, clip calls only -- a C port's clip, not Julia's.  Prints one JSON line.
usage: python tools/weld_overhead.py [n_floes] [steps] [rounds] [--host]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import subzero_jl_amd  # noqa: E402
from subzero_jl_amd import fields  # noqa: E402


def run(w, steps, t0, dt):
    """steps timestep_sim! from tstep t0 (batches end on tags: the rest is run as the next batch) -> seconds"""
    a = time.perf_counter()
    done = 0
    while done < steps:
        done += max(w.run(steps - done, t0 + done, dt, coupling_dt=1), 1)
    return time.perf_counter() - a


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if len(args) > 0 else 10000
    steps = int(args[1]) if len(args) > 1 else 200
    rounds = int(args[2]) if len(args) > 2 else 5
    cfg = fields.make_config(n_floes=n, seed=12345)
    arms = {"off": fields.build_world(subzero_jl_amd.World(0), cfg), "never": fields.build_world(subzero_jl_amd.World(0), cfg)}
    tiny = 0.5 * float(np.min(cfg["derived"]["area"]))
    arms["never"].set_welding([100], [1], [1], max_weld_area=tiny)
    t = {}
    for k, w in arms.items():                      # relaxation (and warm-up: code objects, lists, first batch)
        run(w, 50, 0, cfg["dt"]); t[k] = 50
    ms = {k: [] for k in arms}
    for _ in range(rounds):
        for k, w in arms.items():
            s = run(w, steps, t[k], cfg["dt"]); t[k] += steps
            ms[k].append(1e3 * s / steps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    w = arms["off"]
    calls = []
    for _ in range(21):
        a = time.perf_counter()
        i, j, area = w.weld_overlaps(1, 1, 1e300)
        calls.append(1e6 * (time.perf_counter() - a) / 2)          # (World.weld_overlaps asks twice: the count, then the columns)
    out = dict(n_floes=n, steps_per_round=steps, rounds=rounds, weld_dt=100, ms_per_step_median=med,
               ms_per_step_all={k: [round(x, 5) for x in v] for k, v in ms.items()}, pipelined={k: bool(x.pipelined()) for k, x in arms.items()},
               never_met_overhead_pct=100.0 * (med["never"] / med["off"] - 1.0),
               pass_us_median=float(np.median(calls[1:])), pass_candidate_pairs=w.weld_candidate_pairs(), pass_table_entries=int(len(i)))
    if "--host" in sys.argv:
        import parity
        import weld_ref as wr
        ow = parity.oracle_from(w, cfg)
        timer = dict(clock=time.perf_counter, s=0.0)
        per_x, per_y = wr.periodic_flags(cfg["kinds"])
        cand, areas = wr.overlaps(ow, (0.0, cfg["L"], 0.0, cfg["L"]), per_x, per_y, 1, 1, 1e300, timer=timer)
        out.update(host_clip_ms=1e3 * timer["s"], host_candidate_pairs=len(cand), host_table_entries=int(np.sum(areas > 0)))
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of a fracture criterion in a tiled run (sz_tile_run with sz_set_fracture; csrc/sz_fracture_tile.hpp) on the configs[1]-type field
with the ranks sharing ONE GPU over gloo -- a rehearsal of the flow, not a multi-GPU number.  Per rank:
    off / never   ms/step of run(steps) with the criterion off and with a criterion that is never met (a huge fixed polygon, Δt = 75: the
                  batch is cut and the collective pass runs behind every fracture step), alternating rounds, the median
    cut           the criterion off, the same steps as one run() per segment the criterion's loop makes: what ending a tiled batch and starting
                  the next costs without any pass
    pass          wall of one sz_tile_fracture_candidates (the pass of a batch plus the compaction and the count gather), and how much of it
                  the host's all-gathers take (timed inside the transport); the rest is kernels, copies and synchronisations
Prints one line per rank.

    python tools/fracture_tile_overhead.py [n_floes] [steps] [rounds] [ranks]
"""
import ctypes as C
import datetime
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAC_DT = 75


class TimedDist:
    """torch.distributed with the wall time of its all_gather calls added up (the library's all-gathers over the host transport)"""

    def __init__(self, dist):
        self._d = dist; self.t_gather = 0.0; self.n_gather = 0

    def __getattr__(self, name):
        return getattr(self._d, name)

    def all_gather(self, *a, **k):
        t0 = time.perf_counter()
        try:
            return self._d.all_gather(*a, **k)
        finally:
            self.t_gather += time.perf_counter() - t0; self.n_gather += 1


def _worker(rank, world, port, n, steps, rounds, q):
    import torch.distributed as dist
    import fracture_ref as fr
    from subzero_jl_amd import capi, fields, tiles
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        cfg = fields.make_config(n_floes=n, seed=12345)
        td = TimedDist(dist)

        def fresh(criterion):
            tw = tiles.TiledWorld(cfg, rank, world, 0, td, host_staging=True, backend="library-host")
            if criterion:
                tw.set_fracture(capi.FRAC_POLYGON, dt=FRAC_DT, poly=fr.huge_square(), min_floe_area=1e6)
            tw.run(8, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True)          # warm-up
            tw.sync(); dist.barrier()
            return tw

        per = {"off": [], "cut": [], "never": []}; ran = []
        # the calls of the `cut` arm: the criterion off, one run() per segment the criterion's loop would make (each ends on a fracture step)
        ends = [t + 1 for t in range(8, 8 + steps - 1) if t % FRAC_DT == 0] + [8 + steps]
        for _ in range(rounds):
            for name in ("off", "cut", "never"):
                tw = fresh(name == "never")
                t0 = time.perf_counter()
                if name == "cut":
                    done, t = 0, 8
                    for e in ends:
                        got = tw.run(e - t, t, cfg["dt"], coupling_dt=1, stop_on_tags=True); done += got
                        if got < e - t:
                            break
                        t = e
                else:
                    done = tw.run(steps, 8, cfg["dt"], coupling_dt=1, stop_on_tags=True)          # (a tag ends all arms on the same step)
                tw.sync()
                per[name].append(1e3 * (time.perf_counter() - t0) / max(done, 1)); ran.append(done)
        tw = fresh(True)
        w = tw.world
        ng, no = C.c_int32(0), C.c_int32(0)
        walls, gathers = [], []
        for _ in range(5):
            dist.barrier()
            g0, k0 = td.t_gather, td.n_gather
            t0 = time.perf_counter()
            w._chk(w.L.sz_tile_fracture_candidates(w.h, C.byref(ng), C.byref(no), None, None))
            walls.append(1e3 * (time.perf_counter() - t0)); gathers.append(1e3 * (td.t_gather - g0)); ngath = td.n_gather - k0
        k = int(np.argsort(walls)[len(walls) // 2])
        fmt = lambda v: f"{np.median(v):.4f} (all: {' '.join(f'{x:.4f}' for x in v)})"
        q.put(f"rank {rank} of {world}, {n} floes ({len(tw.gidx)} owned), {min(ran)}..{max(ran)} of {steps} steps run, Δt = {FRAC_DT}: ms/step off {fmt(per['off'])}; off, cut into {len(ends)} calls {fmt(per['cut'])}; never met {fmt(per['never'])}; "
              f"one fracture_candidates pass {walls[k]:.3f} ms, of which {gathers[k]:.3f} ms in {ngath} host all-gathers, {walls[k] - gathers[k]:.3f} ms kernels, copies and "
              f"synchronisations (median of 5 by wall; walls: {' '.join(f'{x:.3f}' for x in walls)})")
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    a = [int(x) for x in sys.argv[1:]]
    n, steps, rounds, world = (a + [10000, 150, 5, 2][len(a):])[:4]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, steps, rounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for _ in range(world):
            print(q.get(timeout=540), flush=True)
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()


if __name__ == "__main__":
    main()

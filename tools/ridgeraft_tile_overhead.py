#!/usr/bin/env python3
"""Cost of ridge / raft in a tiled run (sz_tile_run with sz_set_ridgeraft; csrc/sz_ridgeraft_tile.hpp) on the configs[1]-type field with the
ranks sharing ONE GPU over gloo -- wall times of a rehearsal of the flow, not a multi-GPU number: the kernels' share and RCCL between real
peers are not in them.  After `relax` steps, per rank:
    pass          wall of one sz_tile_ridgeraft_candidates at a pending stop (the pass that stopped the batch, run again: the key sort, the
                  status, count, scan and write kernels, the gathers, the rename, the merge), and how much of it the host's all-gathers take
                  (timed inside the transport); median of 5
    off / empty   ms/step of run(steps) with ridge / raft off and with Δt = 150 and thresholds no floe meets (every table empty: the batch is cut
                  before each ridge / raft step, which runs split, with the two-collective pass in the middle), alternating rounds, the median
`off-only` measures the off arm alone: the figure a commit without the tiled pass can give.  Prints one line per rank.

    python tools/ridgeraft_tile_overhead.py [n_floes] [steps] [rounds] [ranks] [relax] [off-only]
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

RR_DT = 150


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


def _worker(rank, world, port, n, steps, rounds, relax, off_only, q):
    import torch.distributed as dist
    from subzero_jl_amd import fields, tiles
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        cfg = fields.make_config(n_floes=n, seed=12345)
        td = TimedDist(dist)

        def fresh():
            tw = tiles.TiledWorld(cfg, rank, world, 0, td, host_staging=True, backend="library-host")
            tw.repartition_every = 10 ** 9          # (one sz_tile_run per run(): no ownership check between the arms' steps)
            got = tw.run(relax, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True)
            tw.sync(); dist.barrier()
            return tw, got

        per = {"off": [], "empty": []}; ran = []
        for _ in range(rounds):
            for name in ("off",) if off_only else ("off", "empty"):
                tw, t = fresh()
                if name == "empty":
                    tw.set_ridgeraft(True, dt=RR_DT, max_floe_ridge_height=-1.0, max_floe_raft_height=-1.0)
                t0 = time.perf_counter()
                done = tw.run(steps, t, cfg["dt"], coupling_dt=1, stop_on_tags=True)          # (a tag ends both arms on the same step)
                tw.sync()
                per[name].append(1e3 * (time.perf_counter() - t0) / max(done, 1)); ran.append(done)
        fmt = lambda v: f"{np.median(v):.4f} (all: {' '.join(f'{x:.4f}' for x in v)})"
        line = f"rank {rank} of {world}, {n} floes, {relax} relaxation steps, {min(ran)}..{max(ran)} of {steps} steps run: ms/step off {fmt(per['off'])}"
        if not off_only:
            n_rr = len([s for s in range(relax, relax + steps) if s % RR_DT == 0])
            line += f"; Δt = {RR_DT}, every table empty ({n_rr} ridge / raft steps) {fmt(per['empty'])}"
            # one pass at a pending stop: Δt = 1 makes the next step a ridge / raft step, the default heights let the field's contacts in
            tw, t = fresh()
            tw.set_ridgeraft(True, dt=1)
            got = tw.run(1, t, cfg["dt"], coupling_dt=1, stop_on_tags=True)
            if tw.ridgeraft_pending() < 0:
                line += f"; no pending stop at tstep {t} (run returned {got}): no pass timed"
            else:
                w = tw.world
                nt, nd = C.c_int32(0), C.c_int64(0)
                walls, gathers = [], []
                for _ in range(5):
                    dist.barrier()
                    g0, k0 = td.t_gather, td.n_gather
                    t0 = time.perf_counter()
                    w._chk(w.L.sz_tile_ridgeraft_candidates(w.h, C.byref(nt), 0, None, None, None, None, C.byref(nd)))
                    walls.append(1e3 * (time.perf_counter() - t0)); gathers.append(1e3 * (td.t_gather - g0)); ngath = td.n_gather - k0
                k = int(np.argsort(walls)[len(walls) // 2])
                line += (f"; one pass at tstep {t}: {nt.value} entries, {nd.value} draws, {w.stats()['M']} local rows ({len(tw.gidx)} owned), {walls[k]:.3f} ms, of which "
                         f"{gathers[k]:.3f} ms in {ngath} host all-gathers, {walls[k] - gathers[k]:.3f} ms kernels, copies, sorts and synchronisations "
                         f"(median of 5 by wall; walls: {' '.join(f'{x:.3f}' for x in walls)})")
                tw.finish_step(t, cfg["dt"], coupling_dt=1)
        q.put(line)
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    off_only = "off-only" in sys.argv[1:]
    a = [int(x) for x in sys.argv[1:] if x != "off-only"]
    n, steps, rounds, world, relax = (a + [10000, 300, 3, 2, 50][len(a):])[:5]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, steps, rounds, relax, off_only, q)) for r in range(world)]
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

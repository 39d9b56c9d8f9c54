#!/usr/bin/env python3
"""Cost of the welding overlap table in a tiled run (sz_tile_run with sz_set_welding, sz_tile_weld_overlaps; csrc/sz_weld_tile.hpp) at n floes of
the configs[1] field after 50 relaxation steps, with the ranks sharing ONE GPU over gloo -- a rehearsal of the flow, not a multi-GPU number: the
collectives of a pass go through the host's channel here, and RCCL with real peers has not run it.  Per rank:
    off / never   ms/step of run(steps) with welding off and with dts = [100] and a max_weld_area under every floe (every welding step runs the
                  collective pass, finds no candidate pair, and the batch goes on), in alternating rounds, with the median
    pass          wall of one sz_tile_weld_overlaps on the dense state (bins (1, 1), unlimited max_weld_area, count only): kernels, copies, the
                  host synchronisations and the collectives of one pass (the kernels alone: run this tool under a kernel trace)
Prints one line per rank.

    python tools/weld_tile_overhead.py [n_floes] [steps] [rounds] [ranks]
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


def _worker(rank, world, port, n, steps, rounds, q):
    import torch.distributed as dist
    from subzero_jl_amd import fields, tiles
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    try:
        cfg = fields.make_config(n_floes=n, seed=12345)
        mk = lambda: tiles.TiledWorld(cfg, rank, world, 0, dist, host_staging=True, backend="library-host")
        arms = {"off": mk(), "never": mk()}
        arms["never"].set_welding([100], [1], [1], max_weld_area=0.5 * float(np.min(cfg["derived"]["area"])))
        t = {}
        for k, tw in arms.items():          # relaxation and warm-up
            assert tw.run(50, 0, cfg["dt"], coupling_dt=1, stop_on_tags=True) == 50
            tw.sync(); t[k] = 50
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, tw in arms.items():
                dist.barrier()
                a = time.perf_counter()
                assert tw.run(steps, t[k], cfg["dt"], coupling_dt=1, stop_on_tags=True) == steps
                tw.sync()
                ms[k].append(1e3 * (time.perf_counter() - a) / steps); t[k] += steps
        tw = arms["off"]; w = tw.world
        nt = C.c_int32(0)
        calls = []
        for _ in range(11):
            dist.barrier()
            a = time.perf_counter()
            w._chk(w.L.sz_tile_weld_overlaps(w.h, 1, 1, 1e300, C.byref(nt), 0, None, None, None))
            calls.append(1e3 * (time.perf_counter() - a))
        pairs = tw.weld_candidate_pairs()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        q.put(f"rank {rank} of {world}, {n} floes ({len(tw.gidx)} owned): welding off {med['off']:.4f} ms/step, dts=[100] never met {med['never']:.4f} ms/step "
              f"({100.0 * (med['never'] / med['off'] - 1.0):+.1f} %; rounds off: {' '.join(f'{x:.4f}' for x in ms['off'])}; never: {' '.join(f'{x:.4f}' for x in ms['never'])}); "
              f"one pass {float(np.median(calls[1:])):.2f} ms wall (median of {len(calls) - 1}; min {min(calls[1:]):.2f}), {pairs} candidate pairs, {nt.value} table entries")
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    a = sys.argv[1:]
    n = int(a[0]) if len(a) > 0 else 10000
    steps = int(a[1]) if len(a) > 1 else 200
    rounds = int(a[2]) if len(a) > 2 else 3
    world = int(a[3]) if len(a) > 3 else 2
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

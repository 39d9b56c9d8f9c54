#!/usr/bin/env python3
"""Cost of removal events in a tiled run (sz_tile_run with sz_set_removal; csrc/sz_remove_tile.hpp) against the loop they replace, on case B of
tests/remove_tiles_cases.py (400 floes, 40 steps, nine events) with the ranks sharing ONE GPU over gloo -- a rehearsal of the flow, not a
multi-GPU number.  Per rank and round:
    batch    wall of one run(40) with removal set
    loop     wall of the same 40 steps without it: on every stop all ranks gather their whole state (all_gather_object), each deletes on the
             host (tests/remove_ref.py over the merged list) and builds a fresh TiledWorld from what stays -- positions, velocities, rings and
             sub-floe points only: enough for the cost of a rebuild, not for a bit-equal trajectory
    pass     wall of one remove_floes() behind step 0 (46 floes leave)
Prints one line per rank.

    python tools/removal_tile_overhead.py [ranks] [rounds]
"""
import datetime
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _state_cfg(cfg, parts):
    """a config for TiledWorld from the gathered per-rank states, in global order, minus what remove_ref deletes"""
    import remove_ref as rr
    from subzero_jl_amd import capi
    order = np.argsort(np.concatenate([p["gidx"] for p in parts]), kind="stable")
    cat = lambda k: np.concatenate([p[k] for p in parts])
    cols = {k: cat(k)[order] for k in capi.DCOLS + ["id", "status"]}
    for off, members in (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy"))):
        cnt = np.concatenate([np.diff(p[off]) for p in parts]); start = np.concatenate([[0], np.cumsum(cnt)])
        sel = np.concatenate([np.arange(start[i], start[i + 1]) for i in order])
        cols[off] = np.concatenate([[0], np.cumsum(cnt[order])]).astype(np.int32)
        for m in members:
            cols[m] = cat(m)[sel]
    new = rr.remove_ref(cols, (cfg["Nx"], cfg["Ny"], 0.0, cfg["L"], 0.0, cfg["L"]), False, False, np.zeros((cfg["Nx"] + 1, cfg["Ny"] + 1)))[0]
    d = {k: new[k] for k in ("cx", "cy", "rmax", "area", "height", "mass", "moment")}
    return dict(cfg, n_floes=len(new["cx"]), derived=d, height=new["height"], u=new["u"], v=new["v"], xi=new["xi"], vert_off=new["vert_off"], vx=new["vx"],
                vy=new["vy"], sub_off=new["sub_off"], sx=new["sx"], sy=new["sy"])


def _worker(rank, world, port, rounds, q):
    import torch.distributed as dist
    import remove_tiles_cases as cases
    from subzero_jl_amd import capi, tiles
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        cfg0 = cases.case_b()
        mk = lambda cfg: tiles.TiledWorld(cfg, rank, world, 0, dist, host_staging=True, backend="library-host", rebox_every=3, drift_margin=3000.0)
        t_batch, t_loop, t_pass, stops = [], [], [], 0
        for _ in range(rounds):
            tw = mk(cfg0); tw.set_removal(); tw.sync(); dist.barrier()
            t0 = time.perf_counter(); assert tw.run(cases.B_STEPS, 0, cfg0["dt"], stop_on_tags=True, **cases.B_RUN) == cases.B_STEPS; tw.sync()
            t_batch.append(time.perf_counter() - t0)
            tw = mk(cfg0); tw.sync(); dist.barrier()
            t0 = time.perf_counter(); t = 0; stops = 0
            while t < cases.B_STEPS:
                t += tw.run(cases.B_STEPS - t, t, cfg0["dt"], stop_on_tags=True, **cases.B_RUN)
                if t < cases.B_STEPS:
                    w = tw.world; n = len(tw.gidx)
                    mine = {k: w.get(k)[:n] for k in capi.DCOLS}
                    ids = w.ids(); mine["id"], mine["status"] = ids[0][:n], ids[2][:n]
                    off, x, y = w.rings(); mine["vert_off"], mine["vx"], mine["vy"] = off[:n + 1], x[:off[n]], y[:off[n]]
                    so, sx, sy = w.subpoints(); mine["sub_off"], mine["sx"], mine["sy"] = so[:n + 1], sx[:so[n]], sy[:so[n]]
                    mine["gidx"] = tw.gidx
                    parts = [None] * world
                    dist.all_gather_object(parts, mine)
                    tw = mk(_state_cfg(cfg0, parts)); stops += 1
            tw.sync(); t_loop.append(time.perf_counter() - t0)
            tw = mk(cfg0); tw.set_removal(False)
            assert tw.run(3, 0, cfg0["dt"], stop_on_tags=True, **cases.B_RUN) == 1
            tw.set_removal(); tw.sync(); dist.barrier()
            t0 = time.perf_counter(); verdict = tw.remove_floes(); tw.sync(); t_pass.append(time.perf_counter() - t0)
            assert verdict == (True, 46, 0), verdict
        ms = lambda v: f"{1e3 * min(v):.1f} ms (best of {len(v)}; all: {' '.join(f'{1e3 * x:.1f}' for x in v)})"
        q.put(f"rank {rank} of {world}: run(40) with removal set {ms(t_batch)}; host loop with {stops} rebuilds {ms(t_loop)}; one remove_floes() {ms(t_pass)}")
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    world = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, rounds, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        for _ in range(world):
            print(q.get(timeout=240), flush=True)
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()


if __name__ == "__main__":
    main()

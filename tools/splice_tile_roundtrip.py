#!/usr/bin/env python3
"""Cost of a host edit at a stop of a tiled run: TiledWorld.download_rows + TiledWorld.splice_global (sz_tile_download_rows /
sz_tile_splice_floes; csrc/sz_splice_tile.hpp) against the path a tiled run had before them, on the 400-floe periodic field of
tests/test_splice_gpu.py with the ranks sharing ONE GPU over gloo -- a rehearsal of the flow, not a multi-GPU number.  At each of `stops` stops,
5 steps apart, 3 floes fracture into 9 pieces (tests/splice_ref.py: pieces3); the first stop is a warm-up and is dropped.  Per rank and stop:
    edit     wall of download_rows(the 3 floes) + splice_global(3 deleted, 9 appended) on a world that lives through all stops
    rebuild  wall of the same edit as it was done: all ranks gather their whole state (all_gather_object), each applies the edit to the merged
             list on the host and builds a fresh TiledWorld from the result -- positions, velocities, rings and sub-floe points only: enough for
             the cost of a rebuild, not for a bit-equal trajectory
Making the pieces (host geometry) is common to both and outside both.  Prints one line per rank.

    python tools/splice_tile_roundtrip.py [ranks] [stops]
"""
import datetime
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))


def _pieces(parents, dg, next_id):
    """every floe of `parents` cut into three; the pieces take their parent's velocities and stresses"""
    import splice_ref as sp
    rings, like = [], []
    for i in range(sp.n_rows(parents)):
        p = sp.pieces3(sp.ring_of(parents, i))
        rings += p; like += [i] * len(p)
    return sp.floes_from(rings, sp.take(parents, like), np.arange(next_id, next_id + len(rings)), dg)


def _merged(parts):
    """the gathered per-rank states as one list in global order, in the layout of World.download_rows (no interaction rows)"""
    from subzero_jl_amd import capi
    order = np.argsort(np.concatenate([p["gidx"] for p in parts]), kind="stable")
    cat = lambda k: np.concatenate([p[k] for p in parts])
    cols = {k: cat(k)[order] for k in capi.DCOLS + capi.TCOLS + ["id", "ghost_id", "status"]}
    for off, members in (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy"))):
        cnt = np.concatenate([np.diff(p[off]) for p in parts]); start = np.concatenate([[0], np.cumsum(cnt)])
        sel = np.concatenate([np.arange(start[i], start[i + 1]) for i in order])
        cols[off] = np.concatenate([[0], np.cumsum(cnt[order])]).astype(np.int32)
        for m in members:
            cols[m] = cat(m)[sel]
    cols["inter_off"] = np.zeros(len(order) + 1, np.int32); cols["inter_rows"] = np.zeros((0, 7))
    return cols


def _cfg_of(cfg, new):
    d = {k: new[k] for k in ("cx", "cy", "rmax", "area", "height", "mass", "moment")}
    return dict(cfg, n_floes=len(new["cx"]), derived=d, height=new["height"], u=new["u"], v=new["v"], xi=new["xi"], vert_off=new["vert_off"], vx=new["vx"],
                vy=new["vy"], sub_off=new["sub_off"], sx=new["sx"], sy=new["sy"])


def _state(tw):
    from subzero_jl_amd import capi
    w = tw.world; n = len(tw.gidx)
    tw.sync(); w._host_stale = True
    mine = {k: w.get(k)[:n] for k in capi.DCOLS}
    for name, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        mine[name] = np.stack([w.get(pre + q)[:n] for q in ("11", "12", "21", "22")], 1)
    ids = w.ids(); mine["id"], mine["ghost_id"], mine["status"] = ids[0][:n], ids[1][:n], ids[2][:n]
    off, x, y = w.rings(); mine["vert_off"], mine["vx"], mine["vy"] = off[:n + 1], x[:off[n]], y[:off[n]]
    so, sx, sy = w.subpoints(); mine["sub_off"], mine["sx"], mine["sy"] = so[:n + 1], sx[:so[n]], sy[:so[n]]
    mine["gidx"] = tw.gidx
    return mine


def _worker(rank, world, port, stops, q):
    import torch.distributed as dist
    import splice_ref as sp
    from subzero_jl_amd import fields, tiles
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        cfg0 = fields.make_config(n_floes=400, seed=11, subgrid_per_floe=4.0)
        mk = lambda cfg: tiles.TiledWorld(cfg, rank, world, 0, dist, host_staging=True, backend="library-host", rebox_every=3, drift_margin=3000.0)
        A, B = mk(cfg0), mk(cfg0)
        cfgB, t = cfg0, 0
        t_edit, t_rebuild, n_floes = [], [], []
        for stop in range(stops):
            for tw in (A, B):
                assert tw.run(5, t, cfg0["dt"], coupling_dt=1) == 5
            t += 5
            n = 400 + 6 * stop
            rows = [10 + stop, 200 + stop, 380 - 3 * stop]          # (floes of the start at every stop: the pieces go behind them)
            # ---- the row edit
            A.sync(); dist.barrier()
            t0 = time.perf_counter()
            parents = A.download_rows(rows)
            t1 = time.perf_counter()
            new = _pieces(parents, cfg0["dg"], 10000 + 9 * stop)
            t2 = time.perf_counter()
            ng, _ = A.splice_global(rows, None, new)
            A.sync()
            t_edit.append((t1 - t0) + (time.perf_counter() - t2))
            assert ng == n + 6, (ng, n)
            # ---- the rebuild
            B.sync(); dist.barrier()
            t0 = time.perf_counter()
            parts = [None] * world
            dist.all_gather_object(parts, _state(B))
            whole = _merged(parts)
            t1 = time.perf_counter()
            new = _pieces(sp.take(whole, rows), cfg0["dg"], 10000 + 9 * stop)
            t2 = time.perf_counter()
            cfgB = _cfg_of(cfgB, sp.apply(whole, rows, None, new))
            B = mk(cfgB); B.sync()
            t_rebuild.append((t1 - t0) + (time.perf_counter() - t2))
            n_floes.append((n + 6, len(A.gidx), len(B.gidx)))
        ms = lambda v: f"{1e3 * float(np.median(v)):.2f} ms (median of {len(v)}; all: {' '.join(f'{1e3 * x:.2f}' for x in v)})"
        q.put(f"rank {rank} of {world}: edit (download_rows + splice_global) {ms(t_edit[1:])}; rebuild (gather, host edit, new TiledWorld) {ms(t_rebuild[1:])}; "
              f"floes (global, owned by the edited world, owned by the rebuilt one) per stop: {n_floes}")
    finally:
        dist.destroy_process_group()


def main():
    import torch.multiprocessing as mp
    world = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    stops = (int(sys.argv[2]) if len(sys.argv) > 2 else 7) + 1
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, stops, q)) for r in range(world)]
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

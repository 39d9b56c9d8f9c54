#!/usr/bin/env python3
"""Cost of an output step in a tiled run (sz_tile_run with sz_tile_set_floe_output / sz_tile_set_grid_output; csrc/sz_record_tile.hpp) with two
ranks sharing ONE GPU over gloo -- wall times of a rehearsal of the flow, not a multi-GPU number: every collective goes through the host
here, and RCCL between real peers is not in them.  Per rank, on the bench field (periodic, coupled every 10 steps), after WARM steps:
    plain     one run() per block of NB steps, no output
    hand      the block cut by hand at every output step (every DT_OUT steps): run() up to the step, add_ghosts, a download of every column,
              remove_ghosts, write_grid_data (100 x 100, all outputs; it adds and removes the ghosts itself)
    recorded  one run() per block with a floe writer (all column groups) and a grid writer (100 x 100, all outputs) set
    drain     per output step of the block: the merged floe frame through the library (collective) and the grid frame, then clear_frames
The cost of ONE output step is (block - plain block) / output steps in the block.  The blocks alternate between the worlds; the first repeat
warms every shape and is not counted; every repeat is printed, then the median.
`--off-rounds R --parent-tree PATH`: ms/step of a run with NO writer set, on this tree and on another built checkout (the parent commit's:
its package and library), in fresh rank processes each, alternating, R rounds: the writer-off path must cost what it cost before.
`--off-writer`: the same with a floe writer WITHOUT lists set (all column groups, an output step every DT_OUT steps): the recorded step of a
writer without lists must cost what it cost before, too.
`--lists`: the arm with both lists (sz_tile_set_floe_output_lists) instead of the arms above, floe writers only, in the same repeats:
    plain      no output
    recorded   a floe writer without lists
    lists      a floe writer with interactions and sub-floe points (arena 256 MiB: the block must not end `full`)
    hand       the cut by hand that also downloads interactions (before add_ghosts) and sub-floe points on every rank
    drain / drain_lists   per frame: the merged download of the frame without / with lists; with lists two collectives, timed apart too: the
                          columns with the points, and the interactions (which gathers only the keys, the key tables and the rows)

    python tools/record_tile_bench.py [--floes 10000] [--repeats 5] [--lists] [--off-rounds 0] [--off-writer] [--parent-tree PATH] [--off-steps 200]
"""
import argparse
import datetime
import os
import socket
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NB, DT_OUT, WARM, WORLD = 40, 10, 40, 2
RUN = dict(coupling_dt=10, stop_on_tags=False)


def _tiled(cfg, rank, dist):
    from subzero_jl_amd import tiles
    tw = tiles.TiledWorld(cfg, rank, WORLD, 0, dist, host_staging=True, backend="library-host")
    tw.repartition_every = 10 ** 9          # (one sz_tile_run per run(): no ownership check inside a block)
    assert tw.run(WARM, 0, cfg["dt"], **RUN) == WARM
    tw.sync()
    return tw


def _worker_steps(rank, port, floes, repeats, q):
    import torch.distributed as dist
    from subzero_jl_amd import fields
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=300))
    try:
        cfg = fields.make_config(n_floes=floes, seed=12345)
        dt, L = cfg["dt"], cfg["L"]
        xg = yg = np.linspace(0, L, 101)
        P, H, R = (_tiled(cfg, rank, dist) for _ in range(3))
        R.set_floe_output(0, DT_OUT, arena_bytes=1 << 28)
        R.set_grid_output(0, DT_OUT, xg, yg, max_frames=NB // DT_OUT)
        nout = NB // DT_OUT

        def timed(fn):
            dist.barrier()
            t0 = time.perf_counter(); fn(); return time.perf_counter() - t0

        def hand(t):
            for s in range(t, t + NB, DT_OUT):          # (t is an output step: every segment starts on one)
                H.sync(); H.world.add_ghosts(); H.world._host_stale = True; H.world._pull(); H.world.remove_ghosts()
                H.write_grid_data(xg, yg)
                assert H.run(DT_OUT, s, dt, **RUN) == DT_OUT
            H.sync()

        def drain():
            nf, ng, full = R.output_frames()
            assert nf[0] == ng[0] == nout and not full
            for k in range(nout):
                R.floe_frame(0, k); R.grid_frame(0, k)
            R.clear_frames()

        rows, t = [], WARM
        for rep in range(repeats + 1):
            tp = timed(lambda: (P.run(NB, t, dt, **RUN), P.sync()))
            th = timed(lambda: hand(t))
            tr = timed(lambda: (R.run(NB, t, dt, **RUN), R.sync()))
            td = timed(drain)
            t += NB
            if rep == 0:
                continue
            rows.append(dict(plain_ms_per_step=tp / NB * 1e3, hand_step_ms=(th - tp) / nout * 1e3, recorded_step_ms=(tr - tp) / nout * 1e3,
                             merged_download_ms_per_frame_pair=td / nout * 1e3))
            q.put(f"rank {rank} repeat {rep}: " + "  ".join(f"{k} {v:.3f}" for k, v in rows[-1].items()))
        same = all(np.array_equal(P.owned(n), R.owned(n)) and np.array_equal(P.owned(n), H.owned(n)) for n in ("cx", "cy", "u", "v", "xi"))
        q.put(f"rank {rank} of {WORLD} sharing one GPU over the host channel (wall times of a rehearsal), {floes} floes ({len(P.gidx)} owned), grid 100x100, "
              f"{repeats} repeats of {NB} steps with {nout} output steps each; median: "
              + "  ".join(f"{k} {statistics.median(r[k] for r in rows):.3f}" for k in rows[0]) + f"; final states equal: {same}")
        q.put(None)
    finally:
        dist.destroy_process_group()


def _worker_lists(rank, port, floes, repeats, q):
    import torch.distributed as dist
    from subzero_jl_amd import fields
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=300))
    try:
        cfg = fields.make_config(n_floes=floes, seed=12345)
        dt = cfg["dt"]
        P, H, R0, RL, X = (_tiled(cfg, rank, dist) for _ in range(5))          # (X: see below)
        R0.set_floe_output(0, DT_OUT, arena_bytes=1 << 28)
        RL.set_floe_output(0, DT_OUT, arena_bytes=1 << 28)
        RL.set_floe_output_lists(0, ["interactions", "subpoints"])
        nout = NB // DT_OUT

        def timed(fn):
            dist.barrier()
            t0 = time.perf_counter(); fn(); return time.perf_counter() - t0

        def hand(t):
            for s in range(t, t + NB, DT_OUT):
                H.sync(); H.world.interactions()
                H.world.add_ghosts(); H.world._host_stale = True; H.world._pull(); H.world.subpoints(); H.world.remove_ghosts()
                assert H.run(DT_OUT, s, dt, **RUN) == DT_OUT
            H.sync()

        ROWS = ["inter_off", "inter_rows"]

        def drain(w, split=None):
            """every frame down, merged; split: the seconds of the column-and-points call and of the interactions call, each a collective"""
            nf, ng, full = w.output_frames()
            assert nf[0] == nout and not full, (nf, full)
            sizes = []
            for k in range(nout):
                if split is None:
                    fr = w.floe_frame(0, k)
                else:
                    t0 = time.perf_counter()
                    fr = w.floe_frame(0, k, members=COLS)
                    t1 = time.perf_counter()
                    fr.update(w.floe_frame(0, k, members=ROWS))
                    split[0] += t1 - t0; split[1] += time.perf_counter() - t1
                sizes.append(sum(v.nbytes for v in fr.values() if isinstance(v, np.ndarray)))
            w.clear_frames()
            return sizes

        from subzero_jl_amd import capi
        COLS = [m for g in capi.FRAME_BITS for m in capi.FRAME_MEMBERS.get(g, [g])] + capi.FRAME_LIST_MEMBERS["subpoints"]

        rows, t, bytes0, bytesL = [], WARM, 0, 0
        for rep in range(repeats + 1):
            # the block that follows the drain of the large frames runs at a third of its speed whichever world it is (§9i: the single-context
            # arm saw the same): a world that is not measured takes it
            X.run(NB, t, dt, **RUN); X.sync()
            tp = timed(lambda: (P.run(NB, t, dt, **RUN), P.sync()))
            t0 = timed(lambda: (R0.run(NB, t, dt, **RUN), R0.sync()))
            tl = timed(lambda: (RL.run(NB, t, dt, **RUN), RL.sync()))
            th = timed(lambda: hand(t))
            box = {}
            td0 = timed(lambda: box.update(a=drain(R0)))
            split = [0.0, 0.0]
            tdl = timed(lambda: box.update(b=drain(RL, split)))
            bytes0, bytesL = max(box["a"]), max(box["b"])
            t += NB
            if rep == 0:
                continue
            rows.append(dict(plain_ms_per_step=tp / NB * 1e3, recorded_step_ms=(t0 - tp) / nout * 1e3, lists_step_ms=(tl - tp) / nout * 1e3,
                             hand_lists_step_ms=(th - tp) / nout * 1e3, merged_download_ms=td0 / nout * 1e3, merged_download_lists_ms=tdl / nout * 1e3,
                             of_it_columns_and_points_ms=split[0] / nout * 1e3, of_it_interactions_ms=split[1] / nout * 1e3))
            q.put(f"rank {rank} repeat {rep}: " + "  ".join(f"{k} {v:.3f}" for k, v in rows[-1].items()))
        same = all(np.array_equal(P.owned(n), w.owned(n)) for w in (R0, RL, H) for n in ("cx", "cy", "u", "v", "xi"))
        q.put(f"rank {rank} of {WORLD} sharing one GPU over the host channel (wall times of a rehearsal), {floes} floes ({len(P.gidx)} owned), "
              f"{repeats} repeats of {NB} steps with {nout} output steps each; merged frame {bytes0} bytes without lists, {bytesL} with; median (min .. max): "
              + "  ".join(f"{k} {statistics.median(r[k] for r in rows):.3f} ({min(r[k] for r in rows):.3f} .. {max(r[k] for r in rows):.3f})" for k in rows[0])
              + f"; final states equal: {same}")
        q.put(None)
    finally:
        dist.destroy_process_group()


def _worker_off(rank, port, floes, steps, tree, writer, q):
    if tree:
        sys.path.insert(0, tree)          # (in front of this tree: the other checkout's package and the library beside it)
    import torch.distributed as dist
    from subzero_jl_amd import fields
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD, timeout=datetime.timedelta(seconds=300))
    try:
        cfg = fields.make_config(n_floes=floes, seed=12345)
        tw = _tiled(cfg, rank, dist)
        if writer:
            tw.set_floe_output(0, DT_OUT, arena_bytes=1 << 29)
        dist.barrier()
        t0 = time.perf_counter()
        assert tw.run(steps, WARM, cfg["dt"], **RUN) == steps
        tw.sync()
        q.put(1e3 * (time.perf_counter() - t0) / steps)
        q.put(None)
    finally:
        dist.destroy_process_group()


def _ranks(target, *args):
    """the worker on WORLD spawned ranks; what they put on the queue until each has put None"""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, port) + args + (q,)) for r in range(WORLD)]
    for p in procs:
        p.start()
    out, ended = [], 0
    try:
        while ended < WORLD:
            v = q.get(timeout=540)
            if v is None:
                ended += 1
            else:
                out.append(v)
                if isinstance(v, str):
                    print(v, flush=True)
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--floes", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--off-rounds", type=int, default=0)
    ap.add_argument("--off-steps", type=int, default=200)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--lists", action="store_true")
    ap.add_argument("--off-writer", action="store_true")
    ap.add_argument("--alternate-order", action="store_true", help="--off-rounds: the tree that runs first changes from round to round")
    ap.add_argument("--parent-first", action="store_true", help="--off-rounds: the parent's tree runs first in every round (the order is a suspect of its own)")
    a = ap.parse_args()
    if a.repeats > 0:
        _ranks(_worker_lists if a.lists else _worker_steps, a.floes, a.repeats)
    if a.off_rounds > 0:
        arms = {"this build": "", "parent build": os.path.abspath(a.parent_tree)} if a.parent_tree else {"this build": ""}
        if a.parent_first:
            arms = dict(reversed(list(arms.items())))
        got = {k: [] for k in arms}
        for rnd in range(a.off_rounds):
            for name, tree in (list(arms.items()) if not (a.alternate_order and rnd % 2) else list(arms.items())[::-1]):
                got[name].append(max(_ranks(_worker_off, a.floes, a.off_steps, tree, a.off_writer)))          # (the slower rank: the ranks step together)
        what = f"a floe writer without lists set (an output step every {DT_OUT} steps)" if a.off_writer else "no writer set"
        for name, v in got.items():
            print(f"{what}, {name}: ms/step over {a.off_steps} steps, {WORLD} ranks sharing one GPU (wall times of a rehearsal), median {statistics.median(v):.4f} "
                  f"(all: {' '.join(f'{x:.4f}' for x in v)})", flush=True)


if __name__ == "__main__":
    main()

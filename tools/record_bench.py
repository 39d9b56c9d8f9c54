"""Cost of an output step at the bench field (10 000 floes, periodic): recorded on the device (a floe frame with all column groups plus a
100 x 100 grid frame of all 18 outputs) against the same step cut by hand -- add_ghosts, a download of the same columns, eulerian_data,
remove_ghosts.  Three worlds step through the same NB-step blocks with an output step every DT_OUT steps:
    plain     one run() per block, no output
    hand      a run() up to each output step, then the four calls
    recorded  one run() per block with the writers set, then the frames drained (downloaded) and cleared
Two more worlds take the ragged members too (sz_set_floe_output_lists: floe.interactions and the sub-floe points):
    hand+lists      the hand cut, with interactions() in front of add_ghosts and subpoints() behind the column download
    recorded+lists  the recorded run with both lists set; its drain downloads the list sections too
Each block ends in a device synchronise (run() returns after one), so the host clock around a block is its wall time; the cost of ONE output
step is (block - plain block) / output steps in the block, which includes what the cut itself costs the batch.  The blocks alternate between
the worlds and are repeated; every repeat is printed, then the median.
The hand-cut arm runs the entry points a host used before the recorder existed (sz_add_ghosts, sz_download_floes, sz_eulerian_data,
sz_remove_ghosts), in the same process and on the same field as the recorded arm.
usage: python tools/record_bench.py [--floes 10000] [--repeats 7]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import subzero_jl_amd
from subzero_jl_amd import fields

NB, DT_OUT, WARM = 40, 10, 40

ap = argparse.ArgumentParser()
ap.add_argument("--floes", type=int, default=10000)
ap.add_argument("--repeats", type=int, default=7)
args = ap.parse_args()

cfg = fields.make_config(n_floes=args.floes, seed=12345)
dt, L = cfg["dt"], cfg["L"]
xg = yg = np.linspace(0, L, 101)
run = dict(coupling_dt=10, stop_on_tags=False)


def world():
    w = fields.build_world(subzero_jl_amd.World(0), cfg)
    assert w.run(WARM, 0, dt, **run) == WARM
    return w


def block_plain(w, t):
    assert w.run(NB, t, dt, **run) == NB


def block_hand(w, t):
    calls = 0.0
    for s in range(t, t + NB, DT_OUT):          # (t is an output step: every segment starts on one)
        t0 = time.perf_counter()
        w.add_ghosts()
        w._pull()
        w.eulerian_data(xg, yg)
        w.remove_ghosts()
        calls += time.perf_counter() - t0
        assert w.run(DT_OUT, s, dt, **run) == DT_OUT
    return calls


def block_hand_lists(w, t):
    for s in range(t, t + NB, DT_OUT):
        w.interactions()          # (before add_ghosts, which forgets how the last step's ghosts were numbered)
        w.add_ghosts()
        w._pull()
        w.subpoints()
        w.eulerian_data(xg, yg)
        w.remove_ghosts()
        assert w.run(DT_OUT, s, dt, **run) == DT_OUT


def block_recorded(w, t):
    assert w.run(NB, t, dt, **run) == NB


def drain(w, sizes=None):
    nf, ng, full = w.output_frames()
    assert nf[0] == ng[0] == NB // DT_OUT and not full
    for k in range(nf[0]):
        fr = w.floe_frame(0, k)
        w.grid_frame(0, k)
        if sizes is not None:
            sizes.append(w.frame_bytes(w.frame_mask(None), fr["M"], fr["N"], len(fr["vx"]), LISTS, len(fr["inter_rows"]), len(fr["sx"])))
    w.clear_frames()


P, H = world(), world()
R = world()
R.set_floe_output(0, DT_OUT, arena_bytes=1 << 28)
R.set_grid_output(0, DT_OUT, xg, yg, max_frames=NB // DT_OUT)
LISTS = ["interactions", "subpoints"]
HL, RL = world(), world()
RL.set_floe_output(0, DT_OUT, arena_bytes=1 << 28, lists=LISTS)          # (4 frames of ~20 MB each a block: the default arena of 64 MiB ends `full` at the 4th)
RL.set_grid_output(0, DT_OUT, xg, yg, max_frames=NB // DT_OUT)
nout = NB // DT_OUT
rows, frame_sizes = [], []
t = WARM
for rep in range(args.repeats + 1):          # (the first repeat warms every shape of the timed window and is not counted)
    t0 = time.perf_counter(); block_plain(P, t); tp = time.perf_counter() - t0
    t0 = time.perf_counter(); calls = block_hand(H, t); th = time.perf_counter() - t0
    t0 = time.perf_counter(); block_recorded(R, t); tr = time.perf_counter() - t0
    t0 = time.perf_counter(); drain(R); td = time.perf_counter() - t0
    t0 = time.perf_counter(); block_hand_lists(HL, t); thl = time.perf_counter() - t0
    t0 = time.perf_counter(); block_recorded(RL, t); trl = time.perf_counter() - t0
    t0 = time.perf_counter(); drain(RL, frame_sizes); tdl = time.perf_counter() - t0
    t += NB
    if rep == 0:
        continue
    row = dict(plain_ms_per_step=tp / NB * 1e3, hand_step_ms=(th - tp) / nout * 1e3, hand_calls_ms=calls / nout * 1e3,
               recorded_step_ms=(tr - tp) / nout * 1e3, drain_ms_per_frame_pair=td / nout * 1e3,
               hand_lists_step_ms=(thl - tp) / nout * 1e3, recorded_lists_step_ms=(trl - tp) / nout * 1e3, drain_lists_ms_per_frame_pair=tdl / nout * 1e3)
    rows.append(row)
    print(f"repeat {rep}: " + "  ".join(f"{k} {v:.3f}" for k, v in row.items()), flush=True)
print(f"floes {args.floes}, grid 100x100, {args.repeats} repeats of {NB} steps with {nout} output steps each; median:")
for k in rows[0]:
    print(f"  {k}: {statistics.median(r[k] for r in rows):.3f}")
print(f"  floe frame with both lists: {statistics.median(frame_sizes) / 1e6:.2f} MB (median of {len(frame_sizes)})")
# the ways end in the same state
from subzero_jl_amd import capi
same = all(np.array_equal(P.get(n), W.get(n)) for n in capi.DCOLS for W in (R, H, HL, RL))
print("final states equal:", same)
assert same

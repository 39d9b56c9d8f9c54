"""Round trip of a stop: what it costs to take k floes to the host, fracture each into three pieces and put the result back, on the configs[1]
field (periodic box, uniform flow) at n floes after 20 relaxation steps.  Two contexts hold the same list and get the same edits in
alternating rounds; wall clock (time.perf_counter) around the C calls alone -- the host's own work between them (here numpy, in a Julia host
the packing of the ragged columns) is not in the figures:
  A  sz_download_floes + sz_download_interactions, then sz_upload_floes + sz_upload_interactions of the edited list (what a host did before)
  B  sz_download_rows of the k floes, then sz_splice_floes (delete k, append 3 k)
Prints one JSON line with the medians and the raw rounds, per stage, for every k asked for.
usage: python tools/splice_roundtrip.py [n_floes] [rounds] [k ...]        (default 10000 7 3 300)"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import splice_ref as sp  # noqa: E402
import subzero_jl_amd  # noqa: E402
from subzero_jl_amd import capi, fields  # noqa: E402

I32, I64 = np.int32, np.int64


def timed(fn, *a):
    t = time.perf_counter()
    rc = fn(*a)
    dt = time.perf_counter() - t
    if rc != 0:
        raise capi.SzError("rc %d" % rc)
    return 1e3 * dt


def mirror(w):
    """the list as the host holds it: every column, rings, sub-floe points, interactions"""
    w._host_stale = True
    c = {n: w.get(n) for n in capi.DCOLS}
    for n, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        c[n] = np.stack([w.get(pre + q) for q in ("11", "12", "21", "22")], 1)
    c["id"], c["ghost_id"], c["status"] = w.ids()
    off, x, y = w.rings()
    c["vert_off"], c["vx"], c["vy"] = off.copy(), x.copy(), y.copy()
    so, sx, sy = w.subpoints()
    c["sub_off"], c["sx"], c["sy"] = so.copy(), sx.copy(), sy.copy()
    io, ir = w.interactions()
    c["inter_off"], c["inter_rows"] = io.copy(), ir.copy().reshape(-1, 7)
    return c


def struct_of(w, col, keep):
    return w._columns_struct({k: v for k, v in col.items() if k not in ("inter_off", "inter_rows")}, keep)


def path_a(w, full, rows, pieces):
    """-> (ms down, ms up, the edited list)"""
    L, h = w.L, w.h
    st = w.stats()
    M, V = st["M"], st["n_ring_points"]
    buf = {n: np.zeros(M) for n in capi.DCOLS}
    for n in capi.TCOLS:
        buf[n] = np.zeros((M, 4))
    buf["id"] = np.zeros(M, I64); buf["ghost_id"] = np.zeros(M, I64); buf["status"] = np.zeros(M, I32)
    buf["vert_off"] = np.zeros(M + 1, I32); buf["vx"] = np.zeros(V); buf["vy"] = np.zeros(V)
    ioff = np.zeros(M + 1, I32); irows = np.zeros((max(st["n_inter_rows"], 1), 7))
    keep = []
    f = struct_of(w, buf, keep)
    down = timed(L.sz_download_floes, h, C.byref(f)) + timed(L.sz_download_interactions, h, capi.ptr(ioff, capi._ip), capi.ptr(irows))
    assert np.array_equal(buf["cx"], full["cx"]) and np.array_equal(ioff, full["inter_off"])
    new = sp.apply(full, rows, None, pieces)
    keep = []
    f = struct_of(w, new, keep)
    n = sp.n_rows(new)
    io = np.ascontiguousarray(new["inter_off"], I32); ir = np.ascontiguousarray(new["inter_rows"] if len(new["inter_rows"]) else np.zeros((1, 7)))
    up = timed(L.sz_upload_floes, h, n, n, C.byref(f)) + timed(L.sz_upload_interactions, h, capi.ptr(io, capi._ip), capi.ptr(ir))
    w.N = w._M = n; w._host_stale = True
    return down, up, new


def path_b(w, rows):
    """-> (ms down, the rows)"""
    L, h = w.L, w.h
    rows = np.ascontiguousarray(rows, I32)
    n = len(rows)
    sizes = np.zeros(3, I64)
    down = timed(L.sz_download_rows, h, n, capi.ptr(rows, capi._ip), None, None, None, capi.ptr(sizes, capi._lp))
    V, NS, R = (int(v) for v in sizes)
    col = {k: np.zeros(n) for k in capi.DCOLS}
    for k in capi.TCOLS:
        col[k] = np.zeros((n, 4))
    col["id"] = np.zeros(n, I64); col["ghost_id"] = np.zeros(n, I64); col["status"] = np.zeros(n, I32)
    col["vert_off"] = np.zeros(n + 1, I32); col["vx"] = np.zeros(V); col["vy"] = np.zeros(V)
    col["sub_off"] = np.zeros(n + 1, I32); col["sx"] = np.zeros(NS); col["sy"] = np.zeros(NS)
    ioff = np.zeros(n + 1, I32); irows = np.zeros((max(R, 1), 7))
    keep = []
    f = struct_of(w, col, keep)
    down += timed(L.sz_download_rows, h, n, capi.ptr(rows, capi._ip), C.byref(f), capi.ptr(ioff, capi._ip), capi.ptr(irows), None)
    col["inter_off"] = ioff; col["inter_rows"] = irows[:R]
    return down, col


def splice_b(w, rows, pieces):
    L, h = w.L, w.h
    rows = np.ascontiguousarray(rows, I32)
    keep = []
    f = struct_of(w, pieces, keep)
    io = np.ascontiguousarray(pieces["inter_off"], I32)
    up = timed(L.sz_splice_floes, h, len(rows), capi.ptr(rows, capi._ip), 0, None, sp.n_rows(pieces), C.byref(f), capi.ptr(io, capi._ip), None)
    w.N = w._M = w.stats()["N"]; w._host_stale = True
    return up


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    ks = [int(a) for a in sys.argv[3:]] or [3, 300]
    cfg = fields.make_config(n_floes=n, seed=12345)
    A = fields.build_world(subzero_jl_amd.World(0), cfg)
    B = fields.build_world(subzero_jl_amd.World(0), cfg)
    for w in (A, B):
        assert w.run(20, 0, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 20
    full = mirror(A)
    fb = mirror(B)
    assert all(np.array_equal(full[k], fb[k]) for k in full)
    rng = np.random.Generator(np.random.PCG64(1))
    unused = list(rng.permutation(np.arange(1, n + 1)))          # ids of floes not fractured yet
    next_id = n + 1
    out = dict(n_floes=n, rounds=rounds, edits={})
    for k in ks:
        ms = {s: [] for s in ("A_down", "A_up", "B_down", "B_up")}
        for r in range(rounds + 1):                              # (round 0 warms both paths up and is dropped)
            ids = [unused.pop() for _ in range(k)]
            rows = np.sort(np.nonzero(np.isin(full["id"], ids))[0]).astype(I32)
            assert len(rows) == k
            bd, got = path_b(B, rows)
            want = sp.take(full, rows)
            assert all(np.array_equal(got[c], want[c]) for c in want), "rows down differ from the host's list"
            rings, like = [], []
            for j, i in enumerate(rows):
                p = sp.pieces3(sp.ring_of(got, j))
                rings += p; like += [j] * len(p)
            pieces = sp.floes_from(rings, sp.take(got, like), np.arange(next_id, next_id + len(rings)), cfg["dg"])
            next_id += len(rings)
            bu = splice_b(B, rows, pieces)
            ad, au, full = path_a(A, full, rows, pieces)
            if r:
                for s, v in zip(("A_down", "A_up", "B_down", "B_up"), (ad, au, bd, bu)):
                    ms[s].append(round(v, 4))
        fb = mirror(B)
        assert all(np.array_equal(full[c].view(np.uint8), fb[c].view(np.uint8)) for c in full), "the two paths left different lists"
        med = {s: float(np.median(v)) for s, v in ms.items()}
        out["edits"][str(k)] = dict(floes_after=sp.n_rows(full), median_ms=med, A_total_ms=med["A_down"] + med["A_up"], B_total_ms=med["B_down"] + med["B_up"],
                                    A_over_B=(med["A_down"] + med["A_up"]) / (med["B_down"] + med["B_up"]), rounds_ms=ms)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

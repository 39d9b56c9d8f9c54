"""Round trip of a ridge / raft stop: what the host's side of a pending stop costs on the configs[1] field (periodic box, uniform flow) at n
floes, relaxed, with ridge / raft Δt = 10 and the reference's default thresholds.  Two contexts run the same trajectory and get the same edit at
every pending stop; wall clock (time.perf_counter) around the C calls alone -- the host's own work between them is not in the figures:
  A  sz_download_floes + sz_download_subpoints + sz_download_interactions of the whole list, then sz_upload_floes + sz_upload_interactions of
     the edited parents (what a host did before)
  B  sz_ridgeraft_rows, sz_download_list_rows of the closure, then sz_splice_parents
The edit is a fixed stand-in for the host's ridging: every parent of the closure replaced unchanged, and one small new floe appended per table
entry (a copy of row i's ring scaled to 2 % about its centroid).  The first stop warms both paths up and is dropped.
Behind the timed edit the pieces are taken out again, untimed and by the same call on both contexts, so the field goes on undisturbed and every
stop is one the relaxed field itself reaches.  With `keep` they stay: they lie inside their parents, the overlaps tag the parents, and the
later stops have tables of a few entries in a list twice as long -- the small-closure end of the comparison.
Prints one JSON line: medians per stage, the raw rounds, and the table / closure sizes of every stop.
usage: python tools/ridgeraft_roundtrip.py [n_floes] [stops] [keep]        (default 10000 7)"""
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
RR_DT, RELAX = 10, 50
CSR = (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy")), ("inter_off", ("inter_rows",)))
CSR_NAMES = {n for off, vals in CSR for n in (off,) + vals}


def timed(fn, *a):
    t = time.perf_counter()
    rc = fn(*a)
    dt = time.perf_counter() - t
    if rc != 0:
        raise capi.SzError("rc %d" % rc)
    return 1e3 * dt


def struct_of(w, col, keep):
    return w._columns_struct({k: v for k, v in col.items() if k not in ("inter_off", "inter_rows")}, keep)


def rows_buffers(n, V, NS, R):
    col = {k: np.zeros(n) for k in capi.DCOLS}
    for k in capi.TCOLS:
        col[k] = np.zeros((n, 4))
    col["id"] = np.zeros(n, I64); col["ghost_id"] = np.zeros(n, I64); col["status"] = np.zeros(n, I32)
    col["vert_off"] = np.zeros(n + 1, I32); col["vx"] = np.zeros(V); col["vy"] = np.zeros(V)
    col["sub_off"] = np.zeros(n + 1, I32); col["sx"] = np.zeros(NS); col["sy"] = np.zeros(NS)
    return col, np.zeros(n + 1, I32), np.zeros((max(R, 1), 7))


def concat(a, b):
    """list b behind list a"""
    out = {k: np.concatenate([a[k], b[k]]) for k in a if k not in CSR_NAMES}
    for off, vals in CSR:
        out[off] = np.concatenate([a[off], a[off][-1] + b[off][1:] - b[off][0]]).astype(I32)
        for v in vals:
            out[v] = np.concatenate([a[v][:a[off][-1]], b[v][b[off][0]:b[off][-1]]])
    return out


def b_down(w):
    """-> (ms rows, ms download, the closure's list rows, their floes)"""
    L, h = w.L, w.h
    n = C.c_int32(0)
    t_rows = timed(L.sz_ridgeraft_rows, h, C.byref(n), 0, None)
    rows = np.zeros(max(n.value, 1), I32)
    t_rows += timed(L.sz_ridgeraft_rows, h, C.byref(n), len(rows), capi.ptr(rows, capi._ip))
    rows = rows[:n.value]
    k = len(rows)
    sizes = np.zeros(3, I64)
    t_down = timed(L.sz_download_list_rows, h, k, capi.ptr(rows, capi._ip), None, None, None, capi.ptr(sizes, capi._lp))
    col, ioff, irows = rows_buffers(k, *(int(v) for v in sizes))
    col["ghost_off"] = np.zeros(k + 1, I32); col["ghost_idx"] = np.zeros(max(3 * k, 1), I32)
    keep = []
    f = struct_of(w, col, keep)
    t_down += timed(L.sz_download_list_rows, h, k, capi.ptr(rows, capi._ip), C.byref(f), capi.ptr(ioff, capi._ip), capi.ptr(irows), None)
    del col["ghost_off"], col["ghost_idx"]
    col["inter_off"] = ioff; col["inter_rows"] = irows[:ioff[-1]]
    return t_rows, t_down, rows, col


def b_up(w, rep_rows, staged, n_app):
    L, h = w.L, w.h
    rep_rows = np.ascontiguousarray(rep_rows, I32)
    keep = []
    f = struct_of(w, staged, keep)
    io = np.ascontiguousarray(staged["inter_off"], I32)
    ir = np.ascontiguousarray(staged["inter_rows"] if len(staged["inter_rows"]) else np.zeros((1, 7)))
    up = timed(L.sz_splice_parents, h, 0, None, len(rep_rows), capi.ptr(rep_rows, capi._ip), int(n_app), C.byref(f), capi.ptr(io, capi._ip), capi.ptr(ir))
    w.N = w._M = w.stats()["N"]; w._sub_on_device = True; w._sub = {}; w._host_stale = True
    return up


def a_down(w):
    """-> (ms, the parents of the list with their sub-floe points and interaction lists)"""
    L, h = w.L, w.h
    st = w.stats()
    M, N, V = st["M"], st["N"], st["n_ring_points"]
    col, ioff, irows = rows_buffers(M, V, 0, st["n_inter_rows"])
    col["ghost_off"] = np.zeros(M + 1, I32); col["ghost_idx"] = np.zeros(max(3 * M, 1), I32)
    del col["sub_off"], col["sx"], col["sy"]
    keep = []
    f = struct_of(w, col, keep)
    ms = timed(L.sz_download_floes, h, C.byref(f))
    so = np.zeros(N + 1, I32)
    ms += timed(L.sz_download_subpoints, h, capi.ptr(so, capi._ip), None, None)
    sx = np.zeros(max(int(so[N]), 1)); sy = np.zeros(max(int(so[N]), 1))
    ms += timed(L.sz_download_subpoints, h, capi.ptr(so, capi._ip), capi.ptr(sx), capi.ptr(sy))
    ms += timed(L.sz_download_interactions, h, capi.ptr(ioff, capi._ip), capi.ptr(irows))
    par = {k: v[:N] for k, v in col.items() if k not in CSR_NAMES and k not in ("ghost_off", "ghost_idx")}
    vo = col["vert_off"]
    par.update(vert_off=vo[:N + 1], vx=col["vx"][:vo[N]], vy=col["vy"][:vo[N]], sub_off=so, sx=sx[:so[N]], sy=sy[:so[N]],
               inter_off=ioff[:N + 1], inter_rows=irows[:ioff[N]])
    return ms, par


def a_up(w, new):
    L, h = w.L, w.h
    keep = []
    f = struct_of(w, new, keep)
    n = sp.n_rows(new)
    io = np.ascontiguousarray(new["inter_off"], I32); ir = np.ascontiguousarray(new["inter_rows"] if len(new["inter_rows"]) else np.zeros((1, 7)))
    up = timed(L.sz_upload_floes, h, n, n, C.byref(f)) + timed(L.sz_upload_interactions, h, capi.ptr(io, capi._ip), capi.ptr(ir))
    w.N = w._M = n; w._sub_on_device = True; w._sub = {}; w._host_stale = True
    return up


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    stops = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    keep_pieces = len(sys.argv) > 3 and sys.argv[3] == "keep"
    cfg = fields.make_config(n_floes=n, seed=12345)
    dt = cfg["dt"]
    A = fields.build_world(subzero_jl_amd.World(0), cfg)
    B = fields.build_world(subzero_jl_amd.World(0), cfg)
    for w in (A, B):
        assert w.run(RELAX, 0, dt, coupling_dt=1, stop_on_tags=False) == RELAX
        w.set_ridgeraft(True, dt=RR_DT)
    t, next_id = RELAX, 10 * n
    ms = {s: [] for s in ("A_down", "A_up", "B_rows", "B_down", "B_splice")}
    sizes = []
    while len(sizes) < stops + 1:
        done = [w.run(4 * RR_DT, t, dt, coupling_dt=1) for w in (A, B)]
        assert done[0] == done[1], done
        t += done[0]
        pend = [w.ridgeraft_pending() for w in (A, B)]
        assert pend[0] == pend[1], pend
        if pend[0] < 0:          # (a tag ended the batch: this tool has no simplification, the run goes on)
            assert done[0] > 0
            continue
        assert pend[0] == t
        ti, tj, _, _, _ = B.ridgeraft_candidates()
        t_rows, t_down, rows, sel = b_down(B)
        st0 = B.stats(); N, M = st0["N"], st0["M"]
        where = {int(r): k for k, r in enumerate(rows)}
        parents = [int(r) for r in rows if r < N]
        rep = sp.take(sel, [where[p] for p in parents])
        like = sp.take(sel, [where[int(i)] for i in ti])
        rings = [sp.scaled(sp.ring_of(like, k), 0.02) for k in range(len(ti))]
        app = sp.floes_from(rings, like, np.arange(next_id, next_id + len(ti)), cfg["dg"])
        next_id += len(ti)
        ad, par = a_down(A)
        assert all(np.array_equal(np.asarray(par[c])[parents].view(np.uint8), rep[c].view(np.uint8)) for c in ("cx", "u", "stress_accum", "id")), "the two contexts differ"
        au = a_up(A, concat(par, app))
        bs = b_up(B, parents, concat(rep, app), len(ti))
        assert A.stats()["N"] == B.stats()["N"] == N + len(ti)
        sizes.append(dict(tstep=int(t), floes=int(N), list_rows=int(M), table=int(len(ti)), closure=int(len(rows)), closure_parents=len(parents)))
        if len(sizes) > 1:
            for s, v in zip(("A_down", "A_up", "B_rows", "B_down", "B_splice"), (ad, au, t_rows, t_down, bs)):
                ms[s].append(round(v, 4))
        if not keep_pieces and len(ti):
            gone = np.arange(N, N + len(ti), dtype=I32)
            for w in (A, B):
                w._chk(w.L.sz_splice_parents(w.h, len(gone), capi.ptr(gone, capi._ip), 0, None, 0, None, None, None))
                w.N = w._M = w.stats()["N"]; w._sub_on_device = True; w._sub = {}; w._host_stale = True
                assert w.N == N
        for w in (A, B):
            w.finish_step(t, dt, coupling_dt=1)
        t += 1
    a, b = (A.get(c) for c in ("cx",)), (B.get(c) for c in ("cx",))
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b)), "the two paths left different lists"
    med = {s: float(np.median(v)) for s, v in ms.items()}
    at, bt = med["A_down"] + med["A_up"], med["B_rows"] + med["B_down"] + med["B_splice"]
    print(json.dumps(dict(n_floes=n, stops=stops, pieces="kept" if keep_pieces else "taken out again behind the timed edit", ridge_raft_dt=RR_DT, relax_steps=RELAX, median_ms=med, A_total_ms=at, B_total_ms=bt, A_over_B=at / bt,
                          stops_measured=sizes[1:], warm_up=sizes[0], rounds_ms=ms)))


if __name__ == "__main__":
    main()

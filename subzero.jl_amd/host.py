"""Host-side mirror of the reference's process API for the hot path, on top of the C-ABI.

`World` keeps the hot columns of the reference's StructArray{Floe} as numpy arrays, hands them to
libsubzero_hip.so, and exposes one method per reference function (same names, argument meaning
and mutation contract):

    add_ghosts!                  -> World.add_ghosts()                 collisions.jl:1060
    timestep_collisions!         -> World.timestep_collisions(n_init, dt)          :734
    floe_floe_interaction!       -> World.floe_floe_interaction(i, j, dt, max_overlap)  :347
    floe_domain_interaction!     -> World.floe_domain_interaction(i, dt, max_overlap)   :594
    timestep_coupling!           -> World.timestep_coupling()          coupling.jl:1705
    timestep_floe_properties!    -> World.timestep_floe_properties(dt) update_floe.jl:469
    timestep_sim!                -> World.timestep_sim(tstep, dt, ...) / World.run(nsteps, ...)  simulation.jl:94

All arithmetic of those calls happens in HIP kernels; this module only packs and unpacks
columns.  Without the built library and a HIP device every call raises (no CPU fallback).
"""
import ctypes as C

import numpy as np

from . import capi, floe as floe_mod
from .capi import SzError

_I32 = np.int32
_I64 = np.int64


class World:
    def __init__(self, device=0, ftype=np.float64):
        """ftype = numpy.float32: a Floe{Float32} host -- the columns cross the boundary as floats (sz_*_f32); the engine computes in double
        all the same, and this class keeps its own copies as float64 holding the rounded values"""
        self._ft = np.dtype(ftype)
        assert self._ft in (np.dtype(np.float64), np.dtype(np.float32))
        self.L = capi.load()
        self.h = self.L.sz_create(int(device))
        if not self.h:
            raise SzError("sz_create failed: no HIP device available (the HIP engine has no CPU fallback)")
        self.h = C.c_void_p(self.h)
        self._params = dict(E=6e6, nu=0.3, mu=0.2, rho_o=1027.0, rho_a=1.2, Cd_io=3e-3, Cd_ia=1e-3, f=1.4e-4,
                            turn_theta=15 * np.pi / 180, floe_floe_max_overlap=0.55, floe_domain_max_overlap=0.75,
                            rho_i=920.0, max_floe_height=10.0, maximum_xi=1e-5, lam=0.2, coupling_dd=1)
        self._rings = []          # host rings of floes added with add_floe
        self._sub = {}            # i -> (sx, sy)
        self.col = {}             # host columns (valid when not _host_stale)
        self.N = 0
        self._M = 0
        self._dirty = True        # host columns changed since the last upload
        self._host_stale = False  # device columns changed since the last download
        self._inter = {}          # hand-set interaction matrices waiting for upload
        self._have_domain = False
        self._domain = None
        self._topo = []

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.sz_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------ helpers
    def _chk(self, rc):
        if rc != 0:
            raise SzError(f"libsubzero_hip error {rc}: {self.L.sz_last_error(self.h).decode()}")

    def _push_params(self):
        p = capi.SzParams(**self._params, _pad=0)
        self._chk(self.L.sz_set_params(self.h, C.byref(p)))

    # ------------------------------------------------------------------ static inputs
    def set_consts(self, E=6e6, nu=0.3, mu=0.2, rho_o=1027.0, rho_a=1.2, Cd_io=3e-3, Cd_ia=1e-3, f=1.4e-4,
                   turn_theta=15 * np.pi / 180):
        self._params.update(E=E, nu=nu, mu=mu, rho_o=rho_o, rho_a=rho_a, Cd_io=Cd_io, Cd_ia=Cd_ia, f=f,
                            turn_theta=turn_theta)
        self._push_params()

    def set_settings(self, floe_floe_max_overlap=0.55, floe_domain_max_overlap=0.75, rho_i=920.0,
                     max_floe_height=10.0, maximum_xi=1e-5, lam=0.2, coupling_dd=1):
        self._params.update(floe_floe_max_overlap=floe_floe_max_overlap, floe_domain_max_overlap=floe_domain_max_overlap,
                            rho_i=rho_i, max_floe_height=max_floe_height, maximum_xi=maximum_xi, lam=lam,
                            coupling_dd=int(coupling_dd))
        self._push_params()

    def set_domain(self, kinds, x0, xf, y0, yf, bu=None, bv=None):
        rects, vals = floe_mod.boundary_rects(x0, xf, y0, yf)
        self.set_domain_raw(kinds, vals, rects, bu, bv)
        self._extent = (x0, xf, y0, yf)

    def set_domain_raw(self, kinds, vals, rects, bu=None, bv=None):
        k = np.ascontiguousarray(kinds, _I32)
        vals = np.ascontiguousarray(vals, np.float64); rects = np.ascontiguousarray(rects, np.float64)
        bu = np.ascontiguousarray(bu if bu is not None else np.zeros(4), np.float64)
        bv = np.ascontiguousarray(bv if bv is not None else np.zeros(4), np.float64)
        self._chk(self.L.sz_set_domain(self.h, capi.ptr(k, capi._ip), capi.ptr(vals), capi.ptr(rects), capi.ptr(bu), capi.ptr(bv)))
        self._have_domain = True
        self._domain = (k, vals, rects, bu, bv)
        self._push_params()

    def set_topography(self, rings):
        rings = [floe_mod.valid_ring(r) for r in rings]
        off = np.zeros(len(rings) + 1, _I32)
        props = []
        for i, r in enumerate(rings):
            off[i + 1] = off[i] + len(r)
            props.append(floe_mod.topography_props(r))
        xy = np.concatenate(rings, 0) if rings else np.zeros((0, 2))
        x = np.ascontiguousarray(xy[:, 0]); y = np.ascontiguousarray(xy[:, 1])
        cx = np.array([p[0] for p in props], np.float64); cy = np.array([p[1] for p in props], np.float64)
        rm = np.array([p[2] for p in props], np.float64)
        self._chk(self.L.sz_set_topography(self.h, len(rings), capi.ptr(off, capi._ip), capi.ptr(x), capi.ptr(y),
                                           capi.ptr(cx), capi.ptr(cy), capi.ptr(rm)))

    def set_grid_fields(self, Nx, Ny, x0, xf, y0, yf, uo, vo, hflx, ua, va):
        arrs = [np.ascontiguousarray(np.broadcast_to(a, (Nx + 1, Ny + 1)), self._ft) for a in (uo, vo, hflx, ua, va)]
        f32 = self._ft == np.float32
        fn = self.L.sz_set_fields_f32 if f32 else self.L.sz_set_fields
        self._chk(fn(self.h, int(Nx), int(Ny), float(x0), float(xf), float(y0), float(yf), *(capi.ptr(a, capi._fp if f32 else capi._dp) for a in arrs)))
        self._grid = (int(Nx), int(Ny))

    def set_precision(self, mode):
        """"f64" (default) or "mixed": the per-point arithmetic of the forcings in fp32 (BASELINE configs[4])"""
        self._chk(self.L.sz_set_precision(self.h, {"f64": 0, "mixed": 1}[mode]))

    # ---- two-way coupling (coupling.jl:1617-1680); off by default like CouplingSettings()
    def set_two_way(self, on=True, Cd_ao=1.25e-3, k=2.14, L=2.93e5, dt=10):
        self._chk(self.L.sz_set_two_way(self.h, int(on), float(Cd_ao), float(k), float(L), int(dt)))

    def set_temps(self, t_ocn, t_atm):
        Nx, Ny = self._grid
        a, b = (np.ascontiguousarray(np.broadcast_to(t, (Nx + 1, Ny + 1)), np.float64) for t in (t_ocn, t_atm))
        self._chk(self.L.sz_set_temps(self.h, capi.ptr(a), capi.ptr(b)))

    def ocean_stress(self):
        """tau_x, tau_y, si_frac, hflx_factor on the (Nx+1) x (Ny+1) grid-line lattice"""
        Nx, Ny = self._grid
        out = [np.zeros((Nx + 1, Ny + 1)) for _ in range(4)]
        self._chk(self.L.sz_download_ocean_stress(self.h, *(capi.ptr(a) for a in out)))
        return out

    # ------------------------------------------------------------------ floe setup (host side)
    def add_floe(self, coords, height):
        """Floe(coords, hmean, 0): appends a parent floe; derived columns as the reference computes them."""
        self._pull()
        ring = floe_mod.valid_ring(coords)
        d = floe_mod.derive(np.array([0, len(ring)]), ring[:, 0].copy(), ring[:, 1].copy(), height,
                            self._params["rho_i"])
        i = self.N
        if not self.col:
            self.col = {n: np.zeros(0) for n in capi.DCOLS}
            for n in capi.TCOLS:
                self.col[n] = np.zeros((0, 4))
            self.col["id"] = np.zeros(0, _I64); self.col["ghost_id"] = np.zeros(0, _I64)
            self.col["status"] = np.zeros(0, _I32)
            self.col["vert_off"] = np.zeros(1, _I32); self.col["vx"] = np.zeros(0); self.col["vy"] = np.zeros(0)
        assert self._M == self.N, "add_floe while ghosts exist"
        for n in capi.DCOLS:
            self.col[n] = np.append(self.col[n], d[n][0] if n in d else 0.0)
        for n in capi.TCOLS:
            self.col[n] = np.vstack([self.col[n], np.zeros((1, 4))])
        self.col["id"] = np.append(self.col["id"], _I64(i + 1))
        self.col["ghost_id"] = np.append(self.col["ghost_id"], _I64(0))
        self.col["status"] = np.append(self.col["status"], _I32(capi.ACTIVE))
        self.col["vert_off"] = np.append(self.col["vert_off"], _I32(self.col["vert_off"][-1] + len(ring)))
        self.col["vx"] = np.append(self.col["vx"], ring[:, 0]); self.col["vy"] = np.append(self.col["vy"], ring[:, 1])
        self.N += 1; self._M += 1
        self._dirty = True
        return i

    def load_columns(self, cols, N=None):
        """Bulk initialisation from ready-made columns (dict with the sz_floe_columns names)."""
        self.col = {k: np.ascontiguousarray(v) for k, v in cols.items()}
        M = len(self.col["cx"])
        self.N = M if N is None else int(N); self._M = M
        for n in capi.DCOLS:
            self.col.setdefault(n, np.zeros(M))
        for n in capi.TCOLS:
            self.col.setdefault(n, np.zeros((M, 4)))
        self.col.setdefault("id", np.arange(1, M + 1, dtype=_I64))
        self.col.setdefault("ghost_id", np.zeros(M, _I64))
        self.col.setdefault("status", np.full(M, capi.ACTIVE, _I32))
        self._sub = {}; self._sub_on_device = False
        self._dirty = True; self._host_stale = False
        self._new_field = True    # a different field: the interaction rows the device may still hold are not its rows

    def set_subpoints(self, i, sx, sy):
        self._sub[int(i)] = (np.ascontiguousarray(sx, np.float64), np.ascontiguousarray(sy, np.float64))
        self._dirty = True

    def set_subpoints_csr(self, sub_off, sx, sy):
        self._sub_on_device = False
        self.col["sub_off"] = np.ascontiguousarray(sub_off, _I32)
        self.col["sx"] = np.ascontiguousarray(sx, np.float64); self.col["sy"] = np.ascontiguousarray(sy, np.float64)
        self._dirty = True

    # ------------------------------------------------------------------ host <-> device
    def _columns_struct(self, col, keep):
        f32 = self._ft == np.float32
        f = capi.SzFloeColumnsF32() if f32 else capi.SzFloeColumns()
        pt = capi._fp if f32 else capi._dp
        for n in capi.DCOLS + ["vx", "vy", "sx", "sy"]:
            a = col.get(n)
            if a is not None:
                a = np.ascontiguousarray(a, self._ft); keep.append(a); setattr(f, n, capi.ptr(a, pt))
        for n in capi.TCOLS:
            a = col.get(n)
            if a is not None:
                a = np.ascontiguousarray(a, self._ft).reshape(-1); keep.append(a); setattr(f, n, capi.ptr(a, pt))
        for n in ("id", "ghost_id"):
            a = col.get(n)
            if a is not None:
                a = np.ascontiguousarray(a, _I64); keep.append(a); setattr(f, n, capi.ptr(a, capi._lp))
        for n in ("status", "vert_off", "sub_off", "ghost_off", "ghost_idx"):
            a = col.get(n)
            if a is not None:
                a = np.ascontiguousarray(a, _I32); keep.append(a); setattr(f, n, capi.ptr(a, capi._ip))
        return f

    def subpoints(self):
        """(offsets, sx, sy) of the sub-floe points as the library holds them (sz_download_subpoints): the caller's points in the caller's order"""
        self._push()
        n = self.N
        off = np.zeros(n + 1, _I32)
        self._chk(self.L.sz_download_subpoints(self.h, capi.ptr(off, capi._ip), None, None))
        sx = np.zeros(max(int(off[n]), 1)); sy = np.zeros(max(int(off[n]), 1))
        self._chk(self.L.sz_download_subpoints(self.h, capi.ptr(off, capi._ip), capi.ptr(sx), capi.ptr(sy)))
        return off, sx[:off[n]], sy[:off[n]]

    def _fetch_subpoints(self):
        """after a migration of a tiled run (tiles.TiledWorld.migrate) the sub-floe points of the tile are the library's: fetched when needed"""
        if not getattr(self, "_sub_on_device", False):
            return
        n = self.N
        off = np.zeros(n + 1, _I32)
        self._chk(self.L.sz_download_subpoints(self.h, capi.ptr(off, capi._ip), None, None))
        sx = np.zeros(max(int(off[n]), 1)); sy = np.zeros(max(int(off[n]), 1))
        self._chk(self.L.sz_download_subpoints(self.h, capi.ptr(off, capi._ip), capi.ptr(sx), capi.ptr(sy)))
        self.col["sub_off"], self.col["sx"], self.col["sy"] = off, sx[:off[n]], sy[:off[n]]
        self._sub_on_device = False

    def _push(self):
        if not self._dirty:
            return
        if not self._have_domain:
            raise SzError("set_domain must be called before the first process call")
        self._fetch_subpoints()
        col = dict(self.col)
        if "sub_off" not in col or self._sub:
            off = np.zeros(self.N + 1, _I32); xs = []; ys = []
            for i in range(self.N):
                sx, sy = self._sub.get(i, (np.zeros(0), np.zeros(0)))
                if "sub_off" in self.col and i not in self._sub:
                    o0, o1 = self.col["sub_off"][i], self.col["sub_off"][i + 1]
                    sx, sy = self.col["sx"][o0:o1], self.col["sy"][o0:o1]
                off[i + 1] = off[i] + len(sx); xs.append(sx); ys.append(sy)
            col["sub_off"] = off
            col["sx"] = np.concatenate(xs) if xs else np.zeros(0)
            col["sy"] = np.concatenate(ys) if ys else np.zeros(0)
            self.col["sub_off"], self.col["sx"], self.col["sy"] = col["sub_off"], col["sx"], col["sy"]
            self._sub = {}
        keep = []
        f = self._columns_struct(col, keep)
        self._chk((self.L.sz_upload_floes_f32 if self._ft == np.float32 else self.L.sz_upload_floes)(self.h, int(self._M), int(self.N), C.byref(f)))
        self._dirty = False; self._host_stale = False
        if getattr(self, "_new_field", False):
            off = np.zeros(self._M + 1, _I32)
            self._chk(self.L.sz_upload_interactions(self.h, capi.ptr(off, capi._ip), None))
            self._new_field = False

    def crec_mismatches(self):
        """test hook: parts of the collision records (the per-floe cache of the columns the neighbour search and the narrow phase read) that differ
        from the columns after the last resident batch; -1: that batch did not run on records"""
        n = C.c_int64(0)
        self._chk(self.L.sz_debug_crec_mismatches(self.h, C.byref(n)))
        return int(n.value)

    def find_key(self, slot, key):
        """diagnosis: the ghost / halo row with order key `key` of the last resident step that used ghost allocator `slot` (sz_debug_find_key)"""
        out = np.zeros(56)
        self._chk(self.L.sz_debug_find_key(self.h, int(slot), int(key), capi.ptr(out)))
        n = int(out[13])
        return None if out[0] < 0 else {"row": int(out[0]), "cx": out[1], "cy": out[2], "u": out[3], "v": out[4], "xi": out[5], "rmax": out[6], "area": out[7],
                                        "height": out[8], "box": out[9:13].copy(), "parent": int(out[14]), "status": int(out[15]),
                                        "x": out[16:16 + n].copy(), "y": out[36:36 + n].copy()}

    def pairs_of_ids(self, slot, id_a, id_b):
        """diagnosis: (owner key, partner key, contact rows, owner row, partner row) of the last resident step's pair items between instances of two ids"""
        out = np.zeros(61)
        self._chk(self.L.sz_debug_pairs_of_ids(self.h, int(slot), int(id_a), int(id_b), capi.ptr(out)))
        return [tuple(int(v) for v in out[1 + 5 * k:6 + 5 * k]) for k in range(min(int(out[0]), 12))]

    def stats(self):
        s = capi.SzStats()
        self._chk(self.L.sz_get_stats(self.h, C.byref(s)))
        return {n: int(getattr(s, n)) for n, _ in capi.SzStats._fields_}

    def _follow_count(self, st=None):
        """a removal pass compacted the parents (remove_floes, run with set_removal): N is the device's, the sub-floe points are the library's"""
        st = self.stats() if st is None else st
        if st["N"] != self.N:
            self.N = st["N"]; self._sub_on_device = "sub_off" in self.col or bool(self._sub); self._sub = {}
            self._host_stale = True

    def _pull(self):
        if not self._host_stale:
            return
        st = self.stats()
        M, V = st["M"], st["n_ring_points"]
        self._follow_count(st)
        col = {n: np.zeros(M, self._ft) for n in capi.DCOLS}
        for n in capi.TCOLS:
            col[n] = np.zeros((M, 4), self._ft)
        col["id"] = np.zeros(M, _I64); col["ghost_id"] = np.zeros(M, _I64); col["status"] = np.zeros(M, _I32)
        col["vert_off"] = np.zeros(M + 1, _I32); col["vx"] = np.zeros(V, self._ft); col["vy"] = np.zeros(V, self._ft)
        col["ghost_off"] = np.zeros(M + 1, _I32); col["ghost_idx"] = np.zeros(max(3 * M, 1), _I32)
        keep = []
        f = self._columns_struct(col, keep)
        self._chk((self.L.sz_download_floes_f32 if self._ft == np.float32 else self.L.sz_download_floes)(self.h, C.byref(f)))
        if self._ft == np.float32:          # (this class keeps float64 copies: the rounded values)
            for n in list(col):
                if col[n].dtype == np.float32:
                    col[n] = col[n].astype(np.float64)
        self._fetch_subpoints()
        for n in ("sub_off", "sx", "sy"):
            if n in self.col:
                col[n] = self.col[n]
        col["ghost_idx"] = col["ghost_idx"][:col["ghost_off"][M]]
        self.col = col
        self._M = M
        self._host_stale = False

    # ------------------------------------------------------------------ state access (oracle-compatible)
    @property
    def M(self):
        self._pull()
        return self._M

    def get(self, name):
        self._pull()
        m = {"sa": "stress_accum", "si": "stress_instant", "e": "strain"}
        for pre, full in m.items():
            if name.startswith(pre) and name[len(pre):] in ("11", "12", "21", "22"):
                return self.col[full][:, ("11", "12", "21", "22").index(name[len(pre):])].copy()
        return self.col[name].copy()

    def set(self, name, vals):
        self._pull()
        v = np.ascontiguousarray(np.broadcast_to(vals, (self._M,)), np.float64).copy()
        for pre, full in {"sa": "stress_accum", "si": "stress_instant", "e": "strain"}.items():
            if name.startswith(pre) and name[len(pre):] in ("11", "12", "21", "22"):
                self.col[full][:, ("11", "12", "21", "22").index(name[len(pre):])] = v
                break
        else:
            self.col[name] = v
        self._dirty = True

    def ids(self):
        self._pull()
        return self.col["id"].copy(), self.col["ghost_id"].copy(), self.col["status"].copy()

    def set_ids(self, ids):
        self._pull(); self.col["id"] = np.ascontiguousarray(ids, _I64); self._dirty = True

    def set_status(self, st):
        self._pull(); self.col["status"] = np.ascontiguousarray(st, _I32); self._dirty = True

    def rings(self):
        self._pull()
        return self.col["vert_off"], self.col["vx"], self.col["vy"]

    def ring(self, i):
        off, x, y = self.rings()
        return np.stack([x[off[i]:off[i + 1]], y[off[i]:off[i + 1]]], 1)

    def interactions(self):
        self._push()
        st = self.stats()
        off = np.zeros(st["M"] + 1, _I32); rows = np.zeros((max(st["n_inter_rows"], 1), 7), self._ft)
        if self._ft == np.float32:
            self._chk(self.L.sz_download_interactions_f32(self.h, capi.ptr(off, capi._ip), capi.ptr(rows, capi._fp)))
            rows = rows.astype(np.float64)
        else:
            self._chk(self.L.sz_download_interactions(self.h, capi.ptr(off, capi._ip), capi.ptr(rows)))
        return off, rows[:off[-1]]

    def inter(self, i):
        off, rows = self.interactions()
        return rows[off[i]:off[i + 1]]

    def ghosts(self):
        self._pull()
        if "ghost_off" not in self.col:
            return [[] for _ in range(self._M)]
        o, g = self.col["ghost_off"], self.col["ghost_idx"]
        return [list(g[o[i]:o[i + 1]]) for i in range(self._M)]

    def fuse(self):
        self._push()
        M = self.stats()["M"]
        off = np.zeros(M + 1, _I32)
        self._chk(self.L.sz_download_fuse(self.h, capi.ptr(off, capi._ip), None))
        idx = np.zeros(max(off[-1], 1), _I32)
        self._chk(self.L.sz_download_fuse(self.h, capi.ptr(off, capi._ip), capi.ptr(idx, capi._ip)))
        return [list(idx[off[i]:off[i + 1]]) for i in range(M)]

    def pairs(self):
        n = self.stats()["n_pairs"]
        pi = np.zeros(max(n, 1), _I32); pj = np.zeros(max(n, 1), _I32)
        self._chk(self.L.sz_download_pairs(self.h, capi.ptr(pi, capi._ip), capi.ptr(pj, capi._ip)))
        return pi[:n], pj[:n]

    def boundary_vals(self):
        v = np.zeros(4)
        self._chk(self.L.sz_get_boundary_vals(self.h, capi.ptr(v)))
        return v

    def boundary_polys(self):
        """the four boundary polygons (N, S, E, W) as (5, 2) arrays, as _make_bounding_box_polygon orders them"""
        r = np.zeros(16)
        self._chk(self.L.sz_get_boundary_rects(self.h, capi.ptr(r)))
        out = []
        for k in range(4):
            x0, x1, y0, y1 = r[4 * k:4 * k + 4]
            out.append(np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0], [x0, y0]]))
        return out

    def which_vertices_match_points(self, points, region):
        """which_vertices_match_points(points, region) (floe_utils.jl:331-352) by the narrow phase's device routine: sorted
        1-based vertex indices"""
        p = np.ascontiguousarray(points, np.float64); r = np.ascontiguousarray(region, np.float64)
        px, py = np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])
        rx, ry = np.ascontiguousarray(r[:, 0]), np.ascontiguousarray(r[:, 1])
        idx = np.zeros(max(len(px), 1), _I32); n = C.c_int32(0)
        self._chk(self.L.sz_debug_match_vertices(self.h, len(px), capi.ptr(px), capi.ptr(py), len(rx), capi.ptr(rx), capi.ptr(ry),
                                                 capi.ptr(idx, capi._ip), C.byref(n)))
        return [int(v) + 1 for v in idx[:n.value]]

    def sample_fields(self, x, y):
        """the forcing kernels' in-bounds test and lattice sample at points (x, y): rows [in_bounds, uocn, vocn, hflx, uatm, vatm, line west, east,
        south, north (1-based), tx, ty]"""
        x = np.ascontiguousarray(x, np.float64); y = np.ascontiguousarray(y, np.float64)
        out = np.zeros((len(x), 12))
        self._chk(self.L.sz_debug_sample_fields(self.h, len(x), capi.ptr(x), capi.ptr(y), capi.ptr(out)))
        return out

    def pipelined(self):
        """the last run() batch ran as pipelined steps (two launches per timestep)"""
        return bool(self.L.sz_debug_pipelined(self.h))

    def totals_mode(self):
        """where the last run() batch took the collision totals from: 0 serial double sums, 1 / 2 the fixed-point totals (sz_debug_totals_mode)"""
        return int(self.L.sz_debug_totals_mode(self.h))

    def fx_totals(self, v, e=0, mode=0, area=1.0, height=1.0, rmax=1.0, perm=None, nthreads=1):
        """test hook (sz_debug_fx_totals): the values v split and added to one pair of fixed-point words by nthreads threads in the order perm;
        mode 0: at exponent e, 1: fx_force_exp(kexp=e, area, height), 2: + fx_lever_exp(rmax), 3: fx_area_exp(area), 4: fx_lever_exp(rmax);
        + 8: kexp from this world's E and mu.  Returns (hi, lo, bad, exponent, joined value)."""
        v = np.ascontiguousarray(v, np.float64)
        perm = np.ascontiguousarray(np.arange(len(v)) if perm is None else perm, _I32)
        words = np.zeros(2, _I64); flags = np.zeros(2, _I32); joined = np.zeros(1)
        self._chk(self.L.sz_debug_fx_totals(self.h, len(v), capi.ptr(v), capi.ptr(perm, capi._ip), int(nthreads), int(mode), int(e), float(area),
                                            float(height), float(rmax), capi.ptr(words, capi._lp), capi.ptr(flags, capi._ip), capi.ptr(joined)))
        return int(words[0]), int(words[1]), int(flags[0]), int(flags[1]), float(joined[0])

    def fx_word(self, row5, sign, cx, cy, eF, eA, eL):
        """test hook (sz_debug_fx_word): the seven high and seven low words one row {fx, fy, px, py, overlap} adds to a floe's totals, and the range flag"""
        row = np.ascontiguousarray(row5, np.float64); assert row.shape == (5,)
        words = np.zeros(14, _I64); bad = C.c_int32(0)
        self._chk(self.L.sz_debug_fx_word(self.h, capi.ptr(row), float(sign), float(cx), float(cy), int(eF), int(eA), int(eL), capi.ptr(words, capi._lp), C.byref(bad)))
        return [int(w) for w in words[:7]], [int(w) for w in words[7:]], int(bad.value)

    def warn_counts(self):
        s = self.stats()
        return np.array([s["warn_height"], s["warn_force"], s["warn_vel"], s["warn_xi"]], _I64)

    # ------------------------------------------------------------------ the reference's process API
    # ------------------------------------------------------------------ output path
    EUL_OUTPUTS = [
        "u_grid", "v_grid", "dudt_grid", "dvdt_grid", "overarea_grid", "mass_grid", "area_grid", "height_grid",
        "si_frac_grid", "stress_xx_grid", "stress_yx_grid", "stress_xy_grid", "stress_yy_grid", "stress_eig_grid",
        "strain_ux_grid", "strain_vx_grid", "strain_uy_grid", "strain_vy_grid",
    ]

    def eulerian_data(self, xg, yg, outputs=None):
        """calc_eulerian_data! (output.jl:793-914) over the rows the context holds: array [len(outputs), nx, ny]
        (writer.data[ix + 1, iy + 1, k + 1]); outputs: names out of EUL_OUTPUTS (get_known_grid_outputs), default all."""
        self._push()
        names = list(self.EUL_OUTPUTS if outputs is None else outputs)
        for n in names:
            if n not in self.EUL_OUTPUTS:
                raise SzError(f"{n} is not a known grid output")
        codes = np.array([self.EUL_OUTPUTS.index(n) for n in names], _I32)
        xg = np.ascontiguousarray(xg, np.float64); yg = np.ascontiguousarray(yg, np.float64)
        nx, ny = len(xg) - 1, len(yg) - 1
        out = np.zeros((max(len(names), 1), nx, ny))
        self._chk(self.L.sz_eulerian_data(self.h, nx, ny, capi.ptr(xg), capi.ptr(yg), len(names), capi.ptr(codes, capi._ip),
                                          capi.ptr(out)))
        return out[:len(names)]

    def write_grid_data(self, xg, yg, outputs=None):
        """write_grid_data! as timestep_sim! reaches it (simulation.jl:102-105): ghosts on, averages, ghosts off"""
        self.add_ghosts()
        try:
            return self.eulerian_data(xg, yg, outputs)
        finally:
            self.remove_ghosts()

    # ---- output frames on the device (sz_set_floe_output / sz_set_grid_output): run() cuts before the writers' output steps, records what they
    # would take -- the list as add_ghosts! leaves it -- into device memory and goes on; the frames are drained afterwards
    @staticmethod
    def frame_mask(columns=None):
        """the columns_mask of set_floe_output for group names out of capi.FRAME_BITS (None: all)"""
        names = capi.FRAME_BITS if columns is None else list(columns)
        for n in names:
            if n not in capi.FRAME_BITS:
                raise SzError(f"{n} is not a column group of a floe frame")
        return sum(1 << capi.FRAME_BITS.index(n) for n in set(names))

    @staticmethod
    def frame_lists(lists=None):
        """the `lists` word of sz_set_floe_output_lists for names out of capi.FRAME_LISTS (None: none; a ready word passes through)"""
        if lists is None or isinstance(lists, int):
            return int(lists or 0)
        for n in lists:
            if n not in capi.FRAME_LISTS:
                raise SzError(f"{n} is not a list of a floe frame")
        return sum(1 << capi.FRAME_LISTS.index(n) for n in set(lists))

    @staticmethod
    def frame_bytes(mask, M, N, V, lists=0, R=0, S=0):
        """what a floe frame of M rows (N parents) and V ring points takes of its writer's arena (FrameLayout, csrc/sz_record.hpp): a header of
        64 bytes, then the selected sections, each padded to 8 bytes; behind them the lists (ListLayout): R interaction rows, S sub-floe points"""
        def pad(b):
            return (b + 7) // 8 * 8
        total = 64
        for b, n in enumerate(capi.FRAME_BITS):
            if not mask >> b & 1:
                continue
            if n in capi.DCOLS or n in ("id", "ghost_id"):
                total += 8 * M
            elif n in capi.TCOLS:
                total += 32 * M
            elif n == "status":
                total += pad(4 * M)
            elif n == "rings":
                total += pad(4 * (M + 1)) + 16 * V
            else:
                total += pad(4 * (M + 1)) + pad(4 * (M - N))
        lists = World.frame_lists(lists)
        if lists & 1:
            total += pad(4 * (M + 1)) + 56 * R
        if lists & 2:
            total += pad(4 * (M + 1)) + 16 * S
        return total

    def set_floe_output(self, writer, dt_out, columns=None, arena_bytes=1 << 26, _tile=False, lists=None):
        """a FloeOutputWriter with Δtout = dt_out (0: off) that records the column groups `columns` (names out of capi.FRAME_BITS, or a ready
        mask; None: all) into an arena of arena_bytes on the device, and the ragged members `lists` (names out of capi.FRAME_LISTS; None: none)
        behind them.  (_tile: through the setter of tiled contexts -- TiledWorld's call.)"""
        mask = columns if isinstance(columns, int) else self.frame_mask(columns)
        word = self.frame_lists(lists)
        fn = self.L.sz_tile_set_floe_output if _tile else self.L.sz_set_floe_output
        self._chk(fn(self.h, int(writer), int(dt_out), int(mask), int(arena_bytes)))
        self._floe_masks = getattr(self, "_floe_masks", {})
        self._floe_masks[int(writer)] = int(mask)
        self._floe_lists = getattr(self, "_floe_lists", {})
        self._floe_lists[int(writer)] = 0
        self._floe_tile = getattr(self, "_floe_tile", {})
        self._floe_tile[int(writer)] = bool(_tile)
        if word:
            self._chk(self.L.sz_set_floe_output_lists(self.h, int(writer), word))
            self._floe_lists[int(writer)] = word

    def set_grid_output(self, writer, dt_out, xg=None, yg=None, outputs=None, max_frames=64, _tile=False):
        """a GridOutputWriter with Δtout = dt_out (0: off) on the grid lines xg, yg for the outputs named (EUL_OUTPUTS, default all), with room
        for max_frames frames on the device.  (_tile: through the setter of tiled contexts -- TiledWorld's call.)"""
        names = list(self.EUL_OUTPUTS if outputs is None else outputs)
        for n in names:
            if n not in self.EUL_OUTPUTS:
                raise SzError(f"{n} is not a known grid output")
        codes = np.array([self.EUL_OUTPUTS.index(n) for n in names], _I32)
        xg = np.ascontiguousarray(xg if xg is not None else [0.0, 1.0], np.float64); yg = np.ascontiguousarray(yg if yg is not None else [0.0, 1.0], np.float64)
        fn = self.L.sz_tile_set_grid_output if _tile else self.L.sz_set_grid_output
        self._chk(fn(self.h, int(writer), int(dt_out), len(xg) - 1, len(yg) - 1, capi.ptr(xg), capi.ptr(yg), len(names), capi.ptr(codes, capi._ip), int(max_frames)))
        self._grid_writers = getattr(self, "_grid_writers", {})
        self._grid_writers[int(writer)] = (len(names), len(xg) - 1, len(yg) - 1)

    def output_frames(self):
        """(frames held per floe writer, frames held per grid writer, full): full = the last run() ended in front of an output step whose
        frame found no room"""
        nf = np.zeros(capi.REC_WRITERS, _I32); ng = np.zeros(capi.REC_WRITERS, _I32); full = C.c_int32(0)
        self._chk(self.L.sz_output_frames(self.h, capi.ptr(nf, capi._ip), capi.ptr(ng, capi._ip), C.byref(full)))
        return [int(v) for v in nf], [int(v) for v in ng], bool(full.value)

    def floe_frame(self, writer, k, members=None, _merged=False):
        """floe frame k of a writer: a dict with tstep, M, N and the recorded columns as arrays in the layout of load_columns (the rings as
        vert_off, vx, vy; the ghost links as ghost_off, ghost_idx; of a writer with lists inter_off, inter_rows [R, 7] and sub_off, sx, sy).
        members: struct members (and inter_off / inter_rows) to ask for instead of everything recorded.
        (_merged: the merged frame of a tiled run, collectively -- TiledWorld.floe_frame's call.)"""
        info = [C.c_int64(0) for _ in range(5)]
        info_fn, down_fn = (self.L.sz_tile_floe_frame_info, self.L.sz_tile_download_floe_frame) if _merged else (self.L.sz_floe_frame_info, self.L.sz_download_floe_frame)
        rc = info_fn(self.h, int(writer), int(k), *(C.byref(v) for v in info))
        if rc and _merged:
            down_fn(self.h, int(writer), int(k), None)          # (the peers are in the collective: take part, so that every rank raises)
        self._chk(rc)
        tstep, M, N, V, G = (int(v.value) for v in info)
        tot = [C.c_int64(0), C.c_int64(0)]
        lists = getattr(self, "_floe_lists", {}).get(int(writer), 0)
        if _merged:          # (the lists a tile frame really holds: a frame behind a migration has lost its interactions)
            word = C.c_uint32(0)
            self._chk(self.L.sz_tile_floe_frame_lists_info(self.h, int(writer), int(k), C.byref(word), *(C.byref(v) for v in tot)))
            lists = int(word.value)
        else:
            if getattr(self, "_floe_tile", {}).get(int(writer)):
                word = C.c_uint32(0)
                self._chk(self.L.sz_tile_floe_frame_lists_info(self.h, int(writer), int(k), C.byref(word), None, None))
                lists = int(word.value)
            self._chk(self.L.sz_floe_frame_lists_info(self.h, int(writer), int(k), *(C.byref(v) for v in tot)))
        R, S = (int(v.value) for v in tot)
        if members is None:
            members = []
            for b, n in enumerate(capi.FRAME_BITS):
                if self._floe_masks[int(writer)] >> b & 1:
                    members += capi.FRAME_MEMBERS.get(n, [n])
            for b, n in enumerate(capi.FRAME_LISTS):
                if lists >> b & 1:
                    members += capi.FRAME_LIST_MEMBERS[n]
        inter = [n for n in members if n in ("inter_off", "inter_rows")]
        col = {}
        for n in members:
            if n in inter:
                continue
            if n in capi.DCOLS:
                col[n] = np.zeros(M)
            elif n in capi.TCOLS:
                col[n] = np.zeros((M, 4))
            elif n in ("id", "ghost_id"):
                col[n] = np.zeros(M, _I64)
            elif n == "status":
                col[n] = np.zeros(M, _I32)
            elif n in ("vert_off", "ghost_off", "sub_off"):
                col[n] = np.zeros(M + 1, _I32)
            elif n in ("vx", "vy"):
                col[n] = np.zeros(max(V, 1))
            elif n in ("sx", "sy"):
                col[n] = np.zeros(max(S, 1))
            elif n == "ghost_idx":
                col[n] = np.zeros(max(G, 1), _I32)
            else:
                raise SzError(f"{n} is not a member of sz_floe_columns")
        keep = []
        f = capi.SzFloeColumns()
        for n, a in col.items():
            keep.append(a)
            setattr(f, n, capi.ptr(a.reshape(-1), capi._lp if a.dtype == _I64 else capi._ip if a.dtype == _I32 else capi._dp))
        if col or not (_merged and inter):          # (a merged call for the interactions alone is ONE collective: no gather of the whole frames in front of it)
            self._chk(down_fn(self.h, int(writer), int(k), C.byref(f)))
        for n in ("vx", "vy"):
            if n in col:
                col[n] = col[n][:V]
        for n in ("sx", "sy"):
            if n in col:
                col[n] = col[n][:S]
        if inter:
            off = np.zeros(M + 1, _I32); rows = np.zeros((max(R, 1), 7))
            inter_fn = self.L.sz_tile_download_floe_frame_interactions if _merged else self.L.sz_download_floe_frame_interactions
            self._chk(inter_fn(self.h, int(writer), int(k), capi.ptr(off, capi._ip), capi.ptr(rows) if "inter_rows" in inter else None))
            if "inter_off" in inter:
                col["inter_off"] = off
            if "inter_rows" in inter:
                col["inter_rows"] = rows[:R]
        if "ghost_idx" in col:
            col["ghost_idx"] = col["ghost_idx"][:G]
        col.update(tstep=tstep, M=M, N=N)
        if getattr(self, "_floe_tile", {}).get(int(writer)) and self._floe_lists.get(int(writer), 0):
            col["lists"] = lists          # (a tile frame of a writer with lists: the frame's own word -- TiledWorld.floe_frame, floe_frame_local)
        return col

    def grid_frame(self, writer, k):
        """grid frame k of a writer: (tstep, array [nout, nx, ny])"""
        nout, nx, ny = self._grid_writers[int(writer)]
        t = C.c_int32(0); out = np.zeros((nout, nx, ny))
        self._chk(self.L.sz_download_grid_frame(self.h, int(writer), int(k), C.byref(t), capi.ptr(out)))
        return int(t.value), out

    def clear_frames(self):
        self._chk(self.L.sz_clear_frames(self.h))

    def simplify_check(self, max_vertices=30, min_floe_area=1e6, min_floe_height=0.1):
        """counts of what simplify_floes! (simplification.jl:339-378) would act on: remove, fuse, rings over
        max_vertices, floes under the minimum area / height; all zero = the pass is a no-op"""
        self._push()
        out = np.zeros(4, _I64)
        self._chk(self.L.sz_simplify_check(self.h, int(max_vertices), float(min_floe_area), float(min_floe_height),
                                           capi.ptr(out, capi._lp)))
        return dict(zip(("remove", "fuse", "over_max_vertices", "dissolve"), (int(v) for v in out)))

    def add_ghosts(self):
        self._push()
        self._chk(self.L.sz_add_ghosts(self.h)); self._host_stale = True

    def remove_ghosts(self, n_init=None):
        self._push()
        self._chk(self.L.sz_remove_ghosts(self.h)); self._host_stale = True

    def timestep_collisions(self, n_init, dt):
        self._push()
        self._chk(self.L.sz_timestep_collisions(self.h, int(n_init), int(dt))); self._host_stale = True

    def floe_floe_interaction(self, i, j, dt, max_overlap):
        self.collide_pairs([i], [j], dt, max_overlap)

    def collide_pairs(self, pi, pj, dt, max_overlap):
        self._push()
        pi = np.ascontiguousarray(pi, _I32); pj = np.ascontiguousarray(pj, _I32)
        self._chk(self.L.sz_collide_pairs(self.h, len(pi), capi.ptr(pi, capi._ip), capi.ptr(pj, capi._ip), int(dt),
                                          float(max_overlap)))
        self._host_stale = True

    def floe_domain_interaction(self, i, dt, max_overlap):
        self._push()
        self._chk(self.L.sz_collide_domain(self.h, int(dt), float(max_overlap))); self._host_stale = True

    def set_interactions(self, i, rows):
        """floe.interactions of floe i = rows (k x 7), set by hand as the reference's calc_stress! test does"""
        self._inter[int(i)] = np.ascontiguousarray(rows, np.float64).reshape(-1, 7)

    def _push_interactions(self):
        self._push()
        if not self._inter:
            return
        M = self._M
        off = np.zeros(M + 1, _I32)
        for i in range(M):
            off[i + 1] = off[i] + len(self._inter.get(i, ()))
        rows = np.concatenate([self._inter[i] for i in range(M) if i in self._inter]) if off[M] else np.zeros((1, 7))
        self._chk(self.L.sz_upload_interactions(self.h, capi.ptr(off, capi._ip), capi.ptr(rows)))
        self._inter = {}

    def calc_stress(self):
        self._push_interactions()
        self._chk(self.L.sz_calc_stress(self.h)); self._host_stale = True

    def calc_strain(self):
        self._push_interactions()
        self._chk(self.L.sz_calc_strain(self.h)); self._host_stale = True

    def calc_torque(self, i):
        """calc_torque! is fused into the interaction-list kernel; nothing to do."""

    def timestep_coupling(self):
        self._push()
        self._chk(self.L.sz_timestep_coupling(self.h)); self._host_stale = True

    def timestep_floe_properties(self, dt):
        self._push()
        self._chk(self.L.sz_timestep_floe_properties(self.h, int(dt))); self._host_stale = True

    def run(self, nsteps, tstep0, dt, coupling_dt=10, collisions_on=True, coupling_on=True, stop_on_tags=True):
        """nsteps x timestep_sim! with the state resident in HBM.  Returns the number of steps run: the batch ends
        after the first step that tags a floe remove / fuse (the reference runs simplify_floes! after every step,
        simulation.jl:205-214), or -- with a criterion set (set_fracture) -- after the first fracture step on which a floe would
        fracture (fracture_floes! is the host's), or -- with welding set (set_welding) -- after the first welding step on which two floes that
        could weld overlap (weld_overlaps() then gives the table timestep_welding! works from; the fuse is the host's);
        or -- with ridge / raft set (set_ridgeraft) -- BEFORE the second half of the first ridge / raft step (tstep % dt == 0) whose candidate
        table is not empty: that step is not counted, ridgeraft_pending() names it, the state is the reference's between timestep_collisions!
        and timestep_ridging_rafting! (ghosts in the list), ridgeraft_candidates() gives the table, and finish_step() runs the rest of the step
        after the host's ridging and rafting; ridge / raft steps with an empty table are run through, and ridgeraft_draws() says by how many
        rand(rng, FT) calls the host's rng has to advance for them;
        stop_on_tags=False runs on regardless (measurement / soak runs).
        With an output writer set (set_floe_output, set_grid_output) the batch is also cut BEFORE each of its output steps, the frames are
        recorded on the device and the batch goes on: every output step at which the batch begins a step has one frame per due writer, its end
        step has none (the next run() records it); a frame that finds no room ends the batch in front of that step (output_frames()[2])."""
        self._push()
        flags = self._flags(collisions_on, coupling_on)
        if not stop_on_tags:
            flags |= capi.NO_STOP
        done = C.c_int32(0)
        self._chk(self.L.sz_step(self.h, int(nsteps), int(tstep0), int(dt), int(coupling_dt), flags, C.byref(done)))
        self._host_stale = True
        if getattr(self, "_removal_on", False) and stop_on_tags:
            self._follow_count()
        return int(done.value)

    @staticmethod
    def _flags(collisions_on, coupling_on):
        return (capi.COLLISIONS_ON if collisions_on else 0) | (capi.COUPLING_ON if coupling_on else 0)

    # ---- ridge / raft candidates on the device (timestep_ridging_rafting!, ridge_raft.jl:676-837)
    def set_ridgeraft(self, on=True, dt=150, min_ridge_height=0.2, max_floe_ridge_height=5.0, max_domain_ridge_height=1.25,
                      max_floe_raft_height=0.25, max_domain_raft_height=0.25):
        """RidgeRaftSettings(ridge_raft_on = on, Δt = dt, ...) with the reference's default heights.  run() then stops in the middle of a ridge /
        raft step whose candidate table is not empty (see run())."""
        self._chk(self.L.sz_set_ridgeraft(self.h, int(bool(on)), int(dt), float(min_ridge_height), float(max_floe_ridge_height),
                                          float(max_domain_ridge_height), float(max_floe_raft_height), float(max_domain_raft_height)))

    def ridgeraft_candidates(self):
        """the candidate table of the list as it is -- after add_ghosts() + timestep_collisions(), hand-made rows on such a list, or at a pending
        stop: (i, j, kind, frac, n_draws).  i: 0-based list row; j: the partner as the interaction rows name it (1-based list row, -1..-4 for the
        N/S/E/W boundary, -(4 + k) for topography element k); kind: bit 1 ridge, bit 2 raft; frac = overlap / min_area; n_draws: the per-floe
        draws of the call (all list rows).  Ascending i, then first-passing-row order."""
        self._push_interactions()
        n = C.c_int32(0); nd = C.c_int64(0)
        self._chk(self.L.sz_ridgeraft_candidates(self.h, C.byref(n), 0, None, None, None, None, C.byref(nd)))
        cap = max(int(n.value), 1)
        i = np.zeros(cap, _I32); j = np.zeros(cap, _I32); k = np.zeros(cap, _I32); f = np.zeros(cap)
        self._chk(self.L.sz_ridgeraft_candidates(self.h, C.byref(n), cap, capi.ptr(i, capi._ip), capi.ptr(j, capi._ip), capi.ptr(k, capi._ip),
                                                 capi.ptr(f), C.byref(nd)))
        m = int(n.value)
        return i[:m].copy(), j[:m].copy(), k[:m].copy(), f[:m].copy(), int(nd.value)

    def ridgeraft_rows(self):
        """the list rows the host's ridging and rafting can touch (sz_ridgeraft_rows), where ridgeraft_candidates() is valid: for every table
        entry row i and, for a floe partner, row j - 1, each with its root parent and every ghost on that parent's ghost list -- ascending
        0-based list rows, each once; empty for an empty table"""
        self._push_interactions()
        fn = self.L.sz_ridgeraft_rows_f32 if self._ft == np.float32 else self.L.sz_ridgeraft_rows
        n = C.c_int32(0)
        self._chk(fn(self.h, C.byref(n), 0, None))
        cap = max(int(n.value), 1)
        rows = np.zeros(cap, _I32)
        self._chk(fn(self.h, C.byref(n), cap, capi.ptr(rows, capi._ip)))
        return rows[:int(n.value)].copy()

    def ridgeraft_pending(self):
        """the timestep whose ridge / raft step is pending (run() stopped in its middle), or -1"""
        t = C.c_int32(-1)
        self._chk(self.L.sz_ridgeraft_pending(self.h, C.byref(t)))
        return int(t.value)

    def ridgeraft_draws(self):
        """per-floe draws of the ridge / raft steps the last run() ran through with an empty table"""
        n = C.c_int64(0)
        self._chk(self.L.sz_ridgeraft_draws(self.h, C.byref(n)))
        return int(n.value)

    def finish_step(self, tstep, dt, coupling_dt=10, collisions_on=True, coupling_on=True):
        """the second half of the pending ridge / raft step on the state the device holds now (floes and interactions the host changed are
        uploaded first): remove_ghosts, timestep_coupling when due, timestep_floe_properties"""
        self._push_interactions()
        self._chk(self.L.sz_step_finish(self.h, int(tstep), int(dt), int(coupling_dt), self._flags(collisions_on, coupling_on)))
        self._host_stale = True

    def set_fracture(self, kind, dt=75, pstar=2.25e5, c=20.0, poly=None, alpha=0.0, min_floe_area=1e6):
        """FractureSettings(fractures_on, criteria, Δt = dt) with FloeSettings.min_floe_area and DecayAreaScaledCalculator.α:
        kind capi.FRAC_HIBLER (HiblerYieldCurve(pstar, c), rebuilt from the mean height on every fracture step), capi.FRAC_POLYGON
        (poly = (px, py), a fixed closed ring, e.g. MohrsCone's) or capi.FRAC_OFF.  run() then ends a batch after the first fracture step
        (tstep % dt == 0) on which determine_fractures finds a floe, as it ends one on a tag (stop_on_tags)."""
        px = py = None
        npts = 0
        if poly is not None:
            px = np.ascontiguousarray(poly[0], np.float64); py = np.ascontiguousarray(poly[1], np.float64)
            npts = len(px)
            if len(py) != npts:
                raise SzError("poly: x and y differ in length")
        self._chk(self.L.sz_set_fracture(self.h, int(kind), int(dt), float(pstar), float(c), int(npts), capi.ptr(px), capi.ptr(py),
                                         float(alpha), float(min_floe_area)))

    def fracture_candidates(self):
        """determine_fractures (fractures.jl:269-280) on the state as it is: 0-based indices of the parents that would fracture"""
        self._push()
        n = C.c_int32(0)
        self._chk(self.L.sz_fracture_candidates(self.h, C.byref(n), None))
        idx = np.zeros(max(self.N, 1), _I32)
        self._chk(self.L.sz_fracture_candidates(self.h, C.byref(n), capi.ptr(idx, capi._ip)))
        return idx[:n.value].copy()

    def fracture_mean(self):
        """(mean parent height, Hibler p) of the last evaluation of the criterion"""
        m, p = C.c_double(0), C.c_double(0)
        self._chk(self.L.sz_debug_fracture_mean(self.h, C.byref(m), C.byref(p)))
        return m.value, p.value

    def set_welding(self, dts, nxs, nys, max_weld_area=2e9):
        """WeldSettings(weld_on, Δts = dts, Nxs = nxs, Nys = nys, max_weld_area) in the reference's order (sorted by Δt, largest first; the set of a
        step is the first with tstep % dt == 0); empty lists turn it off.  run() then ends a batch after the first welding step whose overlap
        table is not empty."""
        d, x, y = (np.ascontiguousarray(a, _I32).ravel() for a in (dts, nxs, nys))
        if not (len(d) == len(x) == len(y)):
            raise SzError("set_welding: dts, nxs and nys differ in length")
        self._chk(self.L.sz_set_welding(self.h, len(d), capi.ptr(d, capi._ip), capi.ptr(x, capi._ip), capi.ptr(y, capi._ip), float(max_weld_area)))

    def weld_overlaps(self, nx, ny, max_weld_area=2e9):
        """the welding overlap table of the state as it is (welding.jl:91-152): (i, j, inter_area), 0-based parents i < j that share a bin of the
        nx x ny welding grid, are active and under max_weld_area, pass potential_interaction and overlap; in the reference's visiting order"""
        self._push()
        n = C.c_int32(0)
        self._chk(self.L.sz_weld_overlaps(self.h, int(nx), int(ny), float(max_weld_area), C.byref(n), 0, None, None, None))
        cap = max(int(n.value), 1)
        i = np.zeros(cap, _I32); j = np.zeros(cap, _I32); a = np.zeros(cap)
        self._chk(self.L.sz_weld_overlaps(self.h, int(nx), int(ny), float(max_weld_area), C.byref(n), cap, capi.ptr(i, capi._ip), capi.ptr(j, capi._ip),
                                          capi.ptr(a)))
        return i[:n.value].copy(), j[:n.value].copy(), a[:n.value].copy()

    def weld_bins(self, nx, ny):
        """bin_floe_centroids (welding.jl:23-55): per parent the 0-based bin number (yidx - 1) * nx + (xidx - 1), or -1 for the floes at and behind
        the first centroid that is out of bounds"""
        self._push()
        b = np.zeros(max(self.N, 1), _I32)
        self._chk(self.L.sz_debug_weld_bins(self.h, int(nx), int(ny), capi.ptr(b, capi._ip)))
        return b[:self.N].copy()

    def weld_candidate_pairs(self):
        """pairs the last table pass clipped (the reference's candidates before intersect_polys)"""
        n = C.c_int32(0)
        self._chk(self.L.sz_debug_weld_npairs(self.h, C.byref(n)))
        return int(n.value)

    # ---- removal and dissolution on the device (remove_floes!, simplification.jl:279-314)
    def set_removal(self, on=True, max_vertices=30, min_floe_area=1e6, min_floe_height=0.1):
        """SimplificationSettings.max_vertices (2**31 - 1 with smooth_vertices_on == false) and FloeSettings' minimum area / height.  run() then
        goes on past a step that tagged a floe `remove`: the floes are removed (or dissolved into dissolved()) on the device, unless the host is
        needed -- a `fuse` tag, a ring over max_vertices, a fracture candidate or a welding step on that step -- where the batch ends as before."""
        self._chk(self.L.sz_set_removal(self.h, int(bool(on)), int(min(int(max_vertices), 2**31 - 1)), float(min_floe_area), float(min_floe_height)))
        self._removal_on = bool(on)

    def remove_floes(self):
        """one pass of remove_floes! on the state as it is: (done, n_removed, n_dissolved); done == False: declined, nothing changed"""
        self._push()
        d, nr, nd = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._chk(self.L.sz_remove_floes(self.h, C.byref(d), C.byref(nr), C.byref(nd)))
        if d.value and (nr.value or nd.value):
            self._follow_count()
        return bool(d.value), int(nr.value), int(nd.value)

    def dissolved(self):
        """the running ocean.dissolved lattice, (Nx+1) x (Ny+1)"""
        Nx, Ny = self._grid
        a = np.zeros((Nx + 1, Ny + 1))
        self._chk(self.L.sz_download_dissolved(self.h, capi.ptr(a)))
        return a

    def set_dissolved(self, a):
        Nx, Ny = self._grid
        a = np.ascontiguousarray(np.broadcast_to(a, (Nx + 1, Ny + 1)), np.float64)
        self._chk(self.L.sz_upload_dissolved(self.h, capi.ptr(a)))

    def origin(self):
        """per parent the row it had at the last upload (the identity until a removal pass compacts the rows)"""
        self._push()
        n = self.stats()["N"]
        o = np.zeros(max(n, 1), _I32)
        self._chk(self.L.sz_download_origin(self.h, capi.ptr(o, capi._ip)))
        return o[:n].copy()

    # ---- rows down, rows back (sz_download_rows / sz_splice_floes): the host's side of a stop edits a few floes, the others stay on the device
    ROW_INT = {"id": _I64, "ghost_id": _I64, "status": _I32}

    def download_rows(self, rows):
        """the parents `rows` (0-based, any order, none twice) as a dict in the layout of load_columns: every column with len(rows) entries in
        that order, the rings (vert_off, vx, vy), the sub-floe points (sub_off, sx, sy) and floe.interactions (inter_off, inter_rows k x 7) as
        CSR -- each value as a full download gives it"""
        return self._download_rows(rows, False)

    def download_list_rows(self, rows):
        """download_rows over the whole list (sz_download_list_rows): `rows` may name any list row, ghosts included; the dict of download_rows
        plus ghost_off / ghost_idx -- a parent's ghost list in list numbers, an empty one for a ghost row (whose sub_off span is empty too)"""
        return self._download_rows(rows, True)

    def _download_rows(self, rows, whole_list):
        self._push_interactions()
        f32 = self._ft == np.float32
        rows = np.ascontiguousarray(rows, _I32).ravel()
        n = len(rows)
        if whole_list:
            fn = self.L.sz_download_list_rows_f32 if f32 else self.L.sz_download_list_rows
        else:
            fn = self.L.sz_download_rows_f32 if f32 else self.L.sz_download_rows
        return self._rows_down(lambda f, ioff, irows, sizes: fn(self.h, n, capi.ptr(rows, capi._ip), f, ioff, irows, sizes), lambda: n, whole_list)

    def _rows_down(self, call, count, whole_list=False):
        """the two calls of a row download through call(cols, inter_off, inter_rows, sizes3) -- the sizes, then the columns; count(): the rows
        that come back, asked behind the first call (tiles.TiledWorld.download_rows learns it there)"""
        f32 = self._ft == np.float32
        sizes = np.zeros(3, _I64)
        self._chk(call(None, None, None, capi.ptr(sizes, capi._lp)))
        n = count()
        V, NS, R = (int(v) for v in sizes)
        col = {k: np.zeros(n, self._ft) for k in capi.DCOLS}
        for k in capi.TCOLS:
            col[k] = np.zeros((n, 4), self._ft)
        for k, t in self.ROW_INT.items():
            col[k] = np.zeros(n, t)
        col["vert_off"] = np.zeros(n + 1, _I32); col["vx"] = np.zeros(V, self._ft); col["vy"] = np.zeros(V, self._ft)
        col["sub_off"] = np.zeros(n + 1, _I32); col["sx"] = np.zeros(NS, self._ft); col["sy"] = np.zeros(NS, self._ft)
        ioff = np.zeros(n + 1, _I32); irows = np.zeros((R, 7), self._ft)
        if whole_list:
            col["ghost_off"] = np.zeros(n + 1, _I32); col["ghost_idx"] = np.zeros(max(3 * n, 1), _I32)
        keep = []
        f = self._columns_struct(col, keep)
        self._chk(call(C.byref(f), capi.ptr(ioff, capi._ip), capi.ptr(irows, capi._fp if f32 else capi._dp), None))
        if whole_list:
            col["ghost_idx"] = col["ghost_idx"][:col["ghost_off"][n]].copy()
        if f32:
            col = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in col.items()}
            irows = irows.astype(np.float64)
        col["inter_off"] = ioff; col["inter_rows"] = irows
        return col

    @staticmethod
    def _staged(parts):
        """dicts in the layout of download_rows, one behind the other (missing columns: zeros, as an upload reads a NULL column)"""
        parts = [p for p in parts if p is not None and len(p["vert_off"]) > 1]
        if not parts:
            return None, None, None, 0
        ns = [len(p["vert_off"]) - 1 for p in parts]
        col = {}
        for k in capi.DCOLS + capi.TCOLS + list(World.ROW_INT):
            if any(k in p for p in parts):
                shape = (4,) if k in capi.TCOLS else ()
                t = World.ROW_INT.get(k, np.float64)
                fill = capi.ACTIVE if k == "status" else 0
                if k == "id" and not all(k in p for p in parts):
                    raise SzError("splice: id given for some of the floes only")
                col[k] = np.concatenate([np.asarray(p[k], t).reshape((m,) + shape) if k in p else np.full((m,) + shape, fill, t) for p, m in zip(parts, ns)])

        def csr(off_name, val_names, width=None):
            off = [np.zeros(1, _I64)]; vals = {v: [] for v in val_names}
            for p, m in zip(parts, ns):
                o = np.asarray(p[off_name], _I64) if off_name in p else np.zeros(m + 1, _I64)
                off.append(off[-1][-1] + (o[1:] - o[0]))
                for v in val_names:
                    a = np.asarray(p[v], np.float64) if off_name in p else np.zeros((0,) if width is None else (0, width))
                    vals[v].append(a[o[0]:o[-1]])
            return np.concatenate(off).astype(_I32), {v: np.concatenate(a) for v, a in vals.items()}
        col["vert_off"], xy = csr("vert_off", ("vx", "vy")); col.update(xy)
        if any("sub_off" in p for p in parts):
            col["sub_off"], xy = csr("sub_off", ("sx", "sy")); col.update(xy)
        ioff, ir = csr("inter_off", ("inter_rows",), 7)
        return col, ioff, np.ascontiguousarray(ir["inter_rows"].reshape(-1, 7)), sum(ns)

    def splice(self, delete=(), replace=None, append=None):
        """edits the resident list in place (sz_splice_floes): `delete` -- ascending rows that vanish; replace = (rows, floes) -- ascending rows
        (of the list as it is, before the deletion) overwritten by the floes of a dict in the layout of download_rows; append = such a dict of
        floes that go behind the last kept row, in their order.  Afterwards the device holds what an upload of the edited list and its interaction
        lists would have left; this object's copy of the columns is fetched again when it is next looked at."""
        self._splice(delete, replace, append, False)

    def splice_parents(self, delete=(), replace=None, append=None):
        """splice on a list that still holds its ghosts (sz_splice_parents) -- a pending ridge / raft stop, or add_ghosts by hand: the ghosts are
        dropped as remove_ghosts drops them, then the edit is applied to the parents; rows number the parents as they are, ghost columns of the
        floes are ignored, a pending step stays pending (finish_step runs its second half).  An all-empty edit changes nothing and keeps the
        ghosts.  With no ghosts and nothing pending it is splice."""
        self._splice(delete, replace, append, True)

    def _splice(self, delete, replace, append, parents):
        self._push_interactions()
        f32 = self._ft == np.float32
        dele = np.ascontiguousarray(delete, _I32).ravel()
        rep_rows, rep_cols = (np.zeros(0, _I32), None) if replace is None else (np.ascontiguousarray(replace[0], _I32).ravel(), replace[1])
        if rep_cols is not None and len(rep_cols["vert_off"]) - 1 != len(rep_rows):
            raise SzError("splice: replace names %d rows and gives %d floes" % (len(rep_rows), len(rep_cols["vert_off"]) - 1))
        col, ioff, irows, ns = self._staged([rep_cols, append])
        n_app = ns - len(rep_rows)
        keep = []
        f = self._columns_struct(col, keep) if col is not None else None
        if irows is not None:
            irows = np.ascontiguousarray(irows, self._ft)
        if parents:
            fn = self.L.sz_splice_parents_f32 if f32 else self.L.sz_splice_parents
        else:
            fn = self.L.sz_splice_floes_f32 if f32 else self.L.sz_splice_floes
        self._chk(fn(self.h, len(dele), capi.ptr(dele, capi._ip), len(rep_rows), capi.ptr(rep_rows, capi._ip), int(n_app),
                     C.byref(f) if f is not None else None, capi.ptr(ioff, capi._ip) if ioff is not None else None,
                     capi.ptr(irows, capi._fp if f32 else capi._dp) if irows is not None and len(irows) else None))
        if len(dele) + ns:          # the mirror follows: count from the device, columns and sub-floe points fetched on demand
            self.N = self._M = self.stats()["N"]
            self._sub_on_device = "sub_off" in self.col or bool(self._sub); self._sub = {}
            self._host_stale = True

    def timestep_sim(self, tstep, dt, coupling_dt=10, collisions_on=True, coupling_on=True):
        self.run(1, tstep, dt, coupling_dt, collisions_on, coupling_on)

    # ------------------------------------------------------------------ measurement
    def profile(self, on=True, only=None):
        """event-time the kernel classes (all, or the one named `only`, e.g. "narrow") from now on."""
        mode = (2 << capi.KERNEL_CLASS_NAMES.index(only)) if (on and only) else int(bool(on))
        self._chk(self.L.sz_profile_enable(self.h, mode)); self._chk(self.L.sz_profile_reset(self.h))

    def forcing_launch(self):
        """0 / 1 / 2: the forcings of the last resident batch ran in their own / the neighbour / the narrow launch (-1: none yet)"""
        w = np.zeros(1, np.int32)
        self._chk(self.L.sz_forcing_launch(self.h, w.ctypes.data_as(C.POINTER(C.c_int32))))
        return int(w[0])

    def narrow_kernel_name(self):
        """the dominant kernel's instantiation as a kernel trace names it, for the last batch"""
        buf = C.create_string_buffer(128)
        self._chk(self.L.sz_narrow_kernel_name(self.h, buf, 128))
        return buf.value.decode()

    def kernel_times(self):
        out = {}
        for k, name in enumerate(capi.KERNEL_CLASS_NAMES):
            ms = C.c_double(0); n = C.c_int64(0)
            self._chk(self.L.sz_kernel_time_ms(self.h, k, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

"""Multi-GPU sharding of the floe population by spatial tile with a ghost-floe halo.

One process per GPU.  The domain box is cut into px x py tiles; a rank OWNS the floes whose
centroid lies in its tile at partition time and keeps them for the whole run (floes move metres
per step against tile sizes of hundreds of kilometres; `repartition()` is a rare host-side
operation).  Every step each rank

  1. packs, on the device, the owned floes that any other rank may need: those whose centroid --
     or a periodic image of it -- lies inside the other rank's owned bounding box expanded by the
     interaction range 2*max(rmax) (+ a drift margin);
  2. trades them with ONE all-to-all-v (`all_to_all_single` with split sizes: RCCL over xGMI; the
     messages are KB-scale, the exchange is latency-bound);
  3. appends the received records as extra floes and runs the ordinary single-GPU timestep on
     owned + halo floes.  Order-dependent rules (which floe of a pair is p1, the Dict rule, row
     order) use the floes' GLOBAL indices, so every pair is evaluated with the same roles on
     every rank that sees it and the owned floes get bit-identical contact rows to a single-GPU
     run; cross-tile pairs are evaluated on both sides instead of shipping rows back.
  4. Only owned floes are integrated; the halo is dropped and rebuilt next step.

The periodic ghost floes of the reference (collisions.jl:881-1047) are created locally from the
local parents (owned or halo) by the same kernels as in the single-GPU path.
"""
import ctypes as C

import numpy as np

from . import capi
from .host import World


def tile_grid(world):
    """px x py with px >= py and px*py == world: 1x1, 2x1, 2x2, 4x2, ..."""
    py = int(np.floor(np.sqrt(world)))
    while world % py:
        py -= 1
    return world // py, py


def assign_tiles(cx, cy, L, world):
    px, py = tile_grid(world)
    ix = np.clip((cx / L * px).astype(int), 0, px - 1)
    iy = np.clip((cy / L * py).astype(int), 0, py - 1)
    return iy * px + ix


def select_halo(cx, cy, box, Lx, Ly, per_x, per_y):
    """Host-side statement of the pack rule (used by the CPU tests): mask of floes whose centroid
    or one of its periodic images lies inside `box` = (xmin, xmax, ymin, ymax)."""
    hit = np.zeros(len(cx), bool)
    for kx in ((-1, 0, 1) if per_x else (0,)):
        for ky in ((-1, 0, 1) if per_y else (0,)):
            x = cx + kx * Lx; y = cy + ky * Ly
            hit |= (box[0] <= x) & (x <= box[1]) & (box[2] <= y) & (y <= box[3])
    return hit


def expanded_box(b5, margin):
    """b5 = xmin, xmax, ymin, ymax, rmax of the owned floes -> box expanded by 2*rmax + margin."""
    r = 2.0 * b5[4] + margin
    return np.array([b5[0] - r, b5[1] + r, b5[2] - r, b5[3] + r])


def subset_config(cfg, idx):
    """The columns of a fields.make_config() scenario restricted to the floes `idx` (sorted)."""
    off = cfg["vert_off"]; so = cfg["sub_off"]
    nv = np.diff(off)[idx]; ns = np.diff(so)[idx]
    voff = np.zeros(len(idx) + 1, np.int32); voff[1:] = np.cumsum(nv)
    soff = np.zeros(len(idx) + 1, np.int32); soff[1:] = np.cumsum(ns)
    vsel = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, int)
    ssel = np.concatenate([np.arange(so[i], so[i + 1]) for i in idx]) if len(idx) else np.zeros(0, int)
    d = cfg["derived"]
    cols = dict(cx=d["cx"][idx], cy=d["cy"][idx], rmax=d["rmax"][idx], area=d["area"][idx], height=d["height"][idx],
                mass=d["mass"][idx], moment=d["moment"][idx], u=cfg["u"][idx], v=cfg["v"][idx], xi=cfg["xi"][idx],
                vert_off=voff, vx=cfg["vx"][vsel], vy=cfg["vy"][vsel],
                id=(np.asarray(idx) + 1).astype(np.int64))
    return cols, soff, cfg["sx"][ssel], cfg["sy"][ssel]


_ROW_CSR = (("vert_off", ("vx", "vy")), ("sub_off", ("sx", "sy")), ("inter_off", ("inter_rows",)))
_ROW_CSR_NAMES = {n for off, vals in _ROW_CSR for n in (off,) + vals}


def _concat_rows(parts):
    """floe lists in the layout of World.download_rows (the same keys in each), one behind the other"""
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0] if k not in _ROW_CSR_NAMES}
    for off, vals in _ROW_CSR:
        n = np.concatenate([np.diff(np.asarray(p[off], np.int64)) for p in parts])
        out[off] = np.concatenate([[0], np.cumsum(n)]).astype(parts[0][off].dtype)
        for v in vals:
            out[v] = np.concatenate([p[v] for p in parts])
    return out


def _take_rows(col, idx):
    """the floes idx of such a list, in that order, as a list of their own"""
    idx = np.asarray(idx, np.int64)
    out = {k: v[idx] for k, v in col.items() if k not in _ROW_CSR_NAMES}
    for off, vals in _ROW_CSR:
        o = np.asarray(col[off], np.int64)
        n = np.diff(o)[idx]
        out[off] = np.concatenate([[0], np.cumsum(n)]).astype(col[off].dtype)
        sel = np.concatenate([np.arange(o[i], o[i + 1]) for i in idx]).astype(np.int64) if len(idx) else np.zeros(0, np.int64)
        for v in vals:
            out[v] = col[v][sel]
    return out


def host_transport(dist, rank, world):
    """sz_host_transport over torch.distributed collectives on HOST tensors (gloo, or any backend that takes CPU tensors):
    the three collectives the library calls when the tiled run was set up with sz_comm_init_host."""
    import torch

    def view(p, nbytes):
        return torch.frombuffer((C.c_char * nbytes).from_address(p), dtype=torch.uint8) if nbytes else torch.zeros(0, dtype=torch.uint8)

    def allgather(user, send, recv, nbytes):
        try:
            out = view(recv, nbytes * world)
            dist.all_gather(list(out.split(nbytes)), view(send, nbytes).clone())
            return 0
        except Exception:                      # noqa: BLE001  (an exception must not cross the C frames)
            import traceback; traceback.print_exc()
            return 1

    def sendrecv(user, npeers, peer, send, send_bytes, recv, recv_bytes):
        try:
            ops = []
            for k in range(npeers):
                if recv_bytes[k]:
                    ops.append(dist.P2POp(dist.irecv, view(recv[k], recv_bytes[k]), int(peer[k])))
                if send_bytes[k]:
                    ops.append(dist.P2POp(dist.isend, view(send[k], send_bytes[k]), int(peer[k])))
            for r in (dist.batch_isend_irecv(ops) if ops else []):
                r.wait()
            return 0
        except Exception:                      # noqa: BLE001
            import traceback; traceback.print_exc()
            return 1

    def allreduce(user, buf, n):
        try:
            dist.all_reduce(torch.frombuffer((C.c_double * n).from_address(C.addressof(buf.contents)), dtype=torch.float64))
            return 0
        except Exception:                      # noqa: BLE001
            import traceback; traceback.print_exc()
            return 1

    t = capi.SzHostTransport(None, capi._AG(allgather), capi._SR(sendrecv), capi._AR(allreduce))
    t._keep = (allgather, sendrecv, allreduce)
    return t


class TileSetupError(capi.SzError):
    """the exchange could not be set up -- raised on EVERY rank together (the ranks agree on it before any collective that
    one of them would miss), so that a caller may fall back to another backend on all ranks at once"""


class TiledWorld:
    """One rank of a tiled run.  `dist` is torch.distributed (initialised) or None for world == 1."""

    def __init__(self, cfg, rank, world, device, dist, drift_margin=None, rebox_every=50, host_staging=False,
                 always_exchange=False, backend="torch", ftype=np.float64):
        """backend: "library" -- the exchange runs inside libsubzero_hip.so (sz_comm_init / sz_tile_setup / sz_tile_run: RCCL
        bound by the library, grouped send / receive with the neighbouring tiles only; `dist` is then only used to hand the
        communicator id to the ranks); "torch" -- one torch.distributed all_to_all_single per step on buffers the library
        packs and unpacks (and, with host_staging, through the host: the gloo tests); "library-host" -- sz_tile_run as
        with "library", but over the host's channel (sz_comm_init_host: `dist` collectives on host buffers, e.g. gloo) --
        the library's multi-rank exchange without an RCCL communicator, which ranks sharing one GPU cannot open.
        ftype: World's -- numpy.float32 for a Floe{Float32} host (the columns cross the boundary through the _f32 twins)."""
        import torch
        self.torch = torch
        self.cfg, self.rank, self.nranks, self.dist = cfg, rank, world, dist
        self.backend = backend
        self.host_staging = host_staging          # gloo: exchange through CPU tensors
        self.world_device = device
        self.always_exchange = always_exchange    # run the collectives even with one rank (tests)
        self.L = cfg["L"]
        self.per_x = cfg["kinds"][2] == "periodic"; self.per_y = cfg["kinds"][0] == "periodic"
        owner = assign_tiles(cfg["derived"]["cx"], cfg["derived"]["cy"], self.L, world)
        self.gidx = np.nonzero(owner == rank)[0]
        cols, soff, sx, sy = subset_config(cfg, self.gidx)
        from . import fields
        w = World(device, ftype=ftype)
        w.set_consts(E=cfg["E"]); w.set_settings()
        w.set_domain([fields.KIND[k] for k in cfg["kinds"]], 0.0, self.L, 0.0, self.L)
        if cfg["topography"]:
            w.set_topography(cfg["topography"])
        w.set_grid_fields(cfg["Nx"], cfg["Ny"], 0.0, self.L, 0.0, self.L, cfg["uo"], cfg["vo"], cfg["hf"], cfg["ua"], cfg["va"])
        w.load_columns(cols); w.set_subpoints_csr(soff, sx, sy)
        w._push()
        g = np.ascontiguousarray(self.gidx, np.int64)
        max_ring = float(np.diff(cfg["vert_off"]).max())        # over ALL floes: halo floes arrive unseen
        max_rmax = float(cfg["derived"]["rmax"].max())          # over ALL floes, like max_ring
        self._max_ring, self._max_rmax = max_ring, max_rmax
        if drift_margin is None:
            # metres an owned floe may move between two box gathers (half of it, strictly): half the largest floe radius keeps the
            # extra halo small against the 2 x rmax interaction range (+ 25 % of a strip that holds ~6 % of a tile's floes at 8 tiles
            # of the 100 k field) and the gathers -- a handful of host synchronisations each -- a hundred steps apart at metres per step
            drift_margin = max(2000.0, 0.5 * max_rmax)
        w._chk(w.L.sz_tile_enable(w.h, capi.ptr(g, capi._lp), max_ring, max_rmax))
        self.world = w
        self.REC = w.L.sz_halo_record_doubles_ctx(w.h)          # (follows the largest ring of all ranks: 12 + 2 x ring capacity)
        self.dev = torch.device("cuda", device)
        self.cap = 0                                          # record slots per peer, sized from a counting pass
        self.send = self.recv = None
        if backend == "library":
            # Every step below that can fail on ONE rank is agreed on before the next collective: a rank that raised while its
            # peers waited in a broadcast or inside ncclCommInitRank would hang the job (no JSON line, no error message).
            uid = (C.c_char * 128)()
            if world > 1:
                self._agree(w.L.sz_comm_available() == 0, "RCCL cannot be bound by libsubzero_hip.so on some rank (librccl missing, or SZ_RCCL_DISABLE)")
                ok = True
                if rank == 0:
                    ok = w.L.sz_comm_unique_id(C.cast(uid, C.c_void_p)) == 0
                box = [bytes(uid) if ok else None]
                dist.broadcast_object_list(box, src=0)          # any host channel does: the id is 128 opaque bytes (None: rank 0 could not make one)
                if box[0] is None:
                    raise TileSetupError("ncclGetUniqueId failed on rank 0")
                uid = (C.c_char * 128).from_buffer_copy(box[0])
            rc = w.L.sz_comm_init(w.h, world, rank, C.cast(uid, C.c_void_p))
            self._agree(rc == 0, f"sz_comm_init failed on some rank ({w.L.sz_last_error(w.h).decode() if rc else 'not this one'})")
        elif backend == "library-host":
            self._transport = host_transport(dist, rank, world)          # (kept alive: the library calls into it)
            w._chk(w.L.sz_comm_init_host(w.h, world, rank, C.byref(self._transport)))
        if backend in ("library", "library-host"):
            w._chk(w.L.sz_tile_setup(w.h, self.L, self.L, int(self.per_x), int(self.per_y), float(drift_margin), int(rebox_every)))
            px, py = tile_grid(world)          # (the tile rule of assign_tiles: rank = iy * px + ix)
            w._chk(w.L.sz_tile_set_center(w.h, (rank % px + 0.5) * self.L / px, (rank // px + 0.5) * self.L / py))
        elif not host_staging:
            # kernels and RCCL collectives are ordered by ONE stream: no host sync inside a step
            w._chk(w.L.sz_set_stream(w.h, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)))
        self.margin, self.rebox_every = drift_margin, min(abs(rebox_every), 8)
        self._dt = 0
        self.rebox_every_max = abs(rebox_every)
        self._rebox_arg = rebox_every
        self._ref = None                                      # owned centroids at the last box gather (drift check)
        self.repartition_every = 500                          # steps between ownership checks (run())
        self.repartition_fraction = 0.1                       # ... re-tile when this share of the floes has left its tile
        self._since_check = 0
        self.boxes = None
        self.steps_since_box = 0
        self.tw_buf = None                                    # per-cell partial sums of the two-way coupling
        self._frac_dt = 0                                     # Δt of the criterion set through set_fracture (0: none): run() asks at its own cuts
        self._weld = None                                     # (dts, nxs, nys, max_weld_area) set through set_welding (None: off): run() asks at its own cuts
        self._rr_draws = 0                                    # per-floe draws of the ridge / raft steps the last run() ran through (sum over its calls)

    def _agree(self, ok, what):
        """collective: raise TileSetupError on every rank when `ok` is false on any of them"""
        if self.dist is None or self.nranks == 1:
            if not ok:
                raise TileSetupError(what)
            return
        t = self.torch.tensor([0 if ok else 1], dtype=self.torch.int32, device="cpu" if self.host_staging else self.torch.device("cuda", self.world_device))
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        if int(t.item()):
            raise TileSetupError(what)

    # ---- collectives
    def _drift_since_last_gather(self):
        """largest centroid displacement of an owned floe since the last box gather, over all ranks (collective).  The
        halo selection is only valid while 2 x that stays under the drift margin built into the boxes: beyond it a
        contact across a tile edge could be missed silently, so it is an error; the gather interval adapts to the
        measured speed (40 % of the margin)."""
        w = self.world
        w._host_stale = True
        n = len(self.gidx)
        cx, cy = w.get("cx")[:n].copy(), w.get("cy")[:n].copy()
        d = 0.0
        if self._ref is not None and len(self._ref[0]) == n and n:
            dx, dy = np.abs(cx - self._ref[0]), np.abs(cy - self._ref[1])
            if self.per_x: dx = np.minimum(dx, np.abs(dx - self.L))       # a parent the ghost pass wrapped around
            if self.per_y: dy = np.minimum(dy, np.abs(dy - self.L))
            d = float(max(dx.max(), dy.max()))
        vmax = float(max(np.abs(w.get("u")[:n]).max(), np.abs(w.get("v")[:n]).max())) if n else 0.0
        t = self.torch.tensor([d, vmax], dtype=self.torch.float64, device="cpu" if self.host_staging else self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        d, vmax = float(t[0].item()), float(t[1].item())
        if 2.0 * d > self.margin:
            raise capi.SzError(f"halo drift: a floe moved {d:.1f} m in {self.steps_since_box} steps, the margin is {self.margin:.1f} m "
                               f"(gather the boxes more often or widen the margin)")
        # the faster of the measured displacement per step and the largest velocity component now may use 30 % of the margin before the
        # next gather; the interval at most doubles from one gather to the next (floes that start from rest speed up)
        per_step = max(d / self.steps_since_box if self.steps_since_box > 0 else 0.0, vmax * abs(self._dt))
        if per_step > 0:
            self.rebox_every = int(max(1, min(self.rebox_every_max, 2 * self.rebox_every if self.steps_since_box > 0 else self.rebox_every,
                                              0.3 * self.margin / per_step)))
        self._ref = (cx, cy)

    def _allgather_boxes(self):
        w = self.world
        b5 = np.zeros(5)
        w._chk(w.L.sz_sync(w.h))
        self._drift_since_last_gather()
        w._chk(w.L.sz_owned_box(w.h, capi.ptr(b5)))
        t = self.torch.tensor(b5, dtype=self.torch.float64, device="cpu" if self.host_staging else self.dev)
        out = [self.torch.zeros_like(t) for _ in range(self.nranks)]
        self.dist.all_gather(out, t)
        allb = np.stack([o.cpu().numpy() for o in out])
        allb[:, 4] = allb[:, 4].max()
        self.boxes = np.ascontiguousarray(np.stack([expanded_box(b, self.margin) for b in allb]))
        w._chk(w.L.sz_halo_set_boxes(w.h, self.nranks, capi.ptr(self.boxes)))
        self.steps_since_box = 0
        # size the exchange buffers: counting pass, largest count over all ranks and peers, 50 % head room
        # (the all-to-all uses equal splits, so every rank must use the same number of slots)
        w._chk(w.L.sz_halo_pack(w.h, self.nranks, self.rank, self.L, self.L, int(self.per_x), int(self.per_y), None, 1))
        counts = np.zeros(self.nranks, np.int32)
        w._chk(w.L.sz_halo_counts(w.h, self.nranks, capi.ptr(counts, capi._ip)))
        t = self.torch.tensor([int(counts.max())], dtype=self.torch.int64, device="cpu" if self.host_staging else self.dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        cap = int(t.item()) * 3 // 2 + 32
        if cap > self.cap:
            self.cap = cap
            n = self.nranks * (self.cap + 1) * self.REC
            self.send = self.torch.zeros(n, dtype=self.torch.float64, device=self.dev)
            self.recv = self.torch.zeros(n, dtype=self.torch.float64, device=self.dev)

    def exchange(self, between=None):
        """steps 1-2 of the module docstring, asynchronous on the device: fills self.recv.  `between` is enqueued
        after the pack kernel and before the wait for the collective: work that does not need the halo (the
        forcings of the owned floes) then runs beside the exchange."""
        torch, dist, w = self.torch, self.dist, self.world
        if self.boxes is None or self.steps_since_box >= self.rebox_every:
            self._allgather_boxes()
        self.steps_since_box += 1
        w._chk(w.L.sz_halo_pack(w.h, self.nranks, self.rank, self.L, self.L, int(self.per_x), int(self.per_y),
                                C.c_void_p(self.send.data_ptr()), self.cap))
        # (this path sizes every region alike and has no per-step drift check: after a box gather the floes may move
        #  margin / 2 -- _allgather_boxes measures what they really moved and shortens the interval when needed)
        if self.host_staging:                       # gloo: through the host
            if between:
                between()
            w._chk(w.L.sz_sync(w.h))
            sb = self.send.cpu(); rb = torch.zeros_like(sb)
            dist.all_to_all_single(rb, sb)
            self.recv.copy_(rb)
            torch.cuda.synchronize()
        else:                                       # RCCL: equal splits, device to device
            work = dist.all_to_all_single(self.recv, self.send, async_op=True)
            if between:
                between()
            work.wait()                             # stream-level: the kernels enqueued next wait for the collective

    def step(self, tstep, dt, coupling_dt=10, collisions_on=True, coupling_on=True):
        w = self.world
        self._dt = dt
        flags = (capi.COLLISIONS_ON if collisions_on else 0) | (capi.COUPLING_ON if coupling_on else 0)
        peers = self.nranks > 1 or self.always_exchange
        if peers:
            self.exchange(lambda: w._chk(w.L.sz_tile_forcing(w.h, int(tstep), int(coupling_dt), flags)))
        w._chk(w.L.sz_tile_step(w.h, C.c_void_p(self.recv.data_ptr()) if peers else None, self.nranks if peers else 0,
                                self.cap, int(tstep), int(dt), int(coupling_dt), flags))
        if self.tw_buf is not None and coupling_on and coupling_dt > 0 and tstep % coupling_dt == 0:
            self._two_way_reduce(dt)
        w._host_stale = True

    # ---- two-way coupling across tiles
    def set_two_way(self, t_ocn, t_atm, dt, Cd_ao=1.25e-3, k=2.14, L=2.93e5):
        """calc_two_way_coupling! (coupling.jl:1617-1680) in a tiled run: every rank sums the ice stress per centre
        cell over the floes it owns, the partial fields are added up with one all-reduce per coupling step, and
        every rank finishes the cells (so every rank holds the full ocean fields, like the single-process run)."""
        w = self.world
        w.set_two_way(True, Cd_ao=Cd_ao, k=k, L=L, dt=dt); w.set_temps(t_ocn, t_atm)
        Nx, Ny = w._grid
        self.tw_buf = self.torch.zeros(3 * (Nx + 1) * (Ny + 1), dtype=self.torch.float64, device=self.dev)

    def _two_way_reduce(self, dt):
        w, torch = self.world, self.torch
        w._chk(w.L.sz_two_way_partial(w.h, C.c_void_p(self.tw_buf.data_ptr())))
        if self.nranks > 1:
            if self.host_staging:
                w._chk(w.L.sz_sync(w.h))
                hb = self.tw_buf.cpu(); self.dist.all_reduce(hb); self.tw_buf.copy_(hb); torch.cuda.synchronize()
            else:
                self.dist.all_reduce(self.tw_buf)
        w._chk(w.L.sz_two_way_finish(w.h, C.c_void_p(self.tw_buf.data_ptr()), int(dt)))

    # ---- grid output across tiles
    def write_grid_data(self, xg, yg, outputs=None):
        """write_grid_data! (output.jl:588-605) in a tiled run: every rank sums what its own floes and their ghosts
        put into each output cell, one all-reduce adds the partial fields up, every rank finishes the averages
        (array [len(outputs), nx, ny] on every rank, as World.write_grid_data gives it)."""
        w, torch = self.world, self.torch
        names = list(w.EUL_OUTPUTS if outputs is None else outputs)
        codes = np.array([w.EUL_OUTPUTS.index(n) for n in names], np.int32)
        xg = np.ascontiguousarray(xg, np.float64); yg = np.ascontiguousarray(yg, np.float64)
        nx, ny = len(xg) - 1, len(yg) - 1
        buf = torch.zeros(capi.EUL_PARTIAL * nx * ny, dtype=torch.float64, device=self.dev)
        self.sync()
        w.add_ghosts()
        try:
            w._chk(w.L.sz_eulerian_partial(w.h, nx, ny, capi.ptr(xg), capi.ptr(yg), C.c_void_p(buf.data_ptr())))
        finally:
            w.remove_ghosts()
        if self.nranks > 1:
            if self.host_staging:
                hb = buf.cpu(); self.dist.all_reduce(hb); buf.copy_(hb)
            else:
                self.dist.all_reduce(buf)
            torch.cuda.synchronize()
        out = np.zeros((max(len(names), 1), nx, ny))
        w._chk(w.L.sz_eulerian_finish(w.h, nx, ny, capi.ptr(xg), capi.ptr(yg), C.c_void_p(buf.data_ptr()), len(names),
                                      capi.ptr(codes, capi._ip), capi.ptr(out)))
        return out[:len(names)]

    # ---- migration: rare, host-side
    def repartition(self, owner_fn=None):
        """Re-assign every floe to the tile its centroid lies in now and move the floes that changed tile to
        their new owner with their complete state (all columns incl. the previous-step tendencies, tensors,
        status, ring, sub-floe points), so that the run continues exactly as it would have.  Floes move metres per
        step against tiles of hundreds of kilometres: this is a rare operation, done on the host (download,
        all_gather_object of the movers, upload).  Returns the number of floes this rank gave away.
        owner_fn(cx, cy) -> rank array overrides the tile rule (tests)."""
        w, dist, rank = self.world, self.dist, self.rank
        self.sync(); w._host_stale = True; w._pull()
        col = w.col; n = len(self.gidx)
        assert w._M == n, "repartition needs a ghost-free state"
        cx, cy = col["cx"].copy(), col["cy"].copy()
        if self.per_x: cx %= self.L
        if self.per_y: cy %= self.L
        owner = np.asarray(owner_fn(cx, cy) if owner_fn else assign_tiles(cx, cy, self.L, self.nranks))
        mv = np.nonzero(owner != rank)[0]; keep = np.nonzero(owner == rank)[0]

        def pick(idx):
            """the rows `idx` of the local columns as one record batch"""
            off = col["vert_off"]; so = col["sub_off"]
            rec = {"gidx": self.gidx[idx], "owner": owner[idx]}
            for k in capi.DCOLS + capi.TCOLS + ["id", "status"]:
                rec[k] = col[k][idx]
            rec["nv"] = np.diff(off)[idx]; rec["ns"] = np.diff(so)[idx]
            sel = np.concatenate([np.arange(off[i], off[i + 1]) for i in idx]) if len(idx) else np.zeros(0, int)
            ssel = np.concatenate([np.arange(so[i], so[i + 1]) for i in idx]) if len(idx) else np.zeros(0, int)
            rec["vx"], rec["vy"] = col["vx"][sel], col["vy"][sel]
            rec["sx"], rec["sy"] = col["sx"][ssel], col["sy"][ssel]
            return rec

        out = pick(mv)
        gathered = [None] * self.nranks
        dist.all_gather_object(gathered, out)
        parts = [pick(keep)]
        for r, rec in enumerate(gathered):
            if r == rank or len(rec["gidx"]) == 0:
                continue
            m = np.nonzero(rec["owner"] == rank)[0]
            if len(m) == 0:
                continue
            vo = np.concatenate([[0], np.cumsum(rec["nv"])]); so = np.concatenate([[0], np.cumsum(rec["ns"])])
            sub = {k: rec[k][m] for k in rec if k not in ("vx", "vy", "sx", "sy")}
            vs = np.concatenate([np.arange(vo[i], vo[i + 1]) for i in m]); ss = np.concatenate([np.arange(so[i], so[i + 1]) for i in m])
            sub["vx"], sub["vy"], sub["sx"], sub["sy"] = rec["vx"][vs], rec["vy"][vs], rec["sx"][ss], rec["sy"][ss]
            parts.append(sub)
        total_moved = int(sum(len(g["gidx"]) for g in gathered))
        if total_moved == 0:
            return 0
        # merge, ordered by global index (any fixed order would do: order-dependent rules use the global index)
        g_all = np.concatenate([p_["gidx"] for p_ in parts]); order = np.argsort(g_all, kind="stable")
        nv_all = np.concatenate([p_["nv"] for p_ in parts]); ns_all = np.concatenate([p_["ns"] for p_ in parts])
        vstart = np.concatenate([[0], np.cumsum(nv_all)]); sstart = np.concatenate([[0], np.cumsum(ns_all)])
        vx_all = np.concatenate([p_["vx"] for p_ in parts]); vy_all = np.concatenate([p_["vy"] for p_ in parts])
        sx_all = np.concatenate([p_["sx"] for p_ in parts]); sy_all = np.concatenate([p_["sy"] for p_ in parts])
        cols = {k: np.concatenate([p_[k] for p_ in parts])[order] for k in capi.DCOLS + capi.TCOLS + ["id", "status"]}
        nv = nv_all[order]; ns = ns_all[order]
        cols["vert_off"] = np.concatenate([[0], np.cumsum(nv)]).astype(np.int32)
        vsel = np.concatenate([np.arange(vstart[i], vstart[i + 1]) for i in order]) if len(order) else np.zeros(0, int)
        ssel = np.concatenate([np.arange(sstart[i], sstart[i + 1]) for i in order]) if len(order) else np.zeros(0, int)
        cols["vx"], cols["vy"] = vx_all[vsel], vy_all[vsel]
        soff = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        self.gidx = g_all[order]
        w.load_columns(cols); w.set_subpoints_csr(soff, sx_all[ssel], sy_all[ssel])
        w._push()
        g = np.ascontiguousarray(self.gidx, np.int64)
        w._chk(w.L.sz_tile_enable(w.h, capi.ptr(g, capi._lp), self._max_ring, self._max_rmax))
        if self.backend in ("library", "library-host"):
            w._chk(w.L.sz_tile_setup(w.h, self.L, self.L, int(self.per_x), int(self.per_y), float(self.margin), int(self._rebox_arg)))
        self.boxes = None                      # owned boxes and halo capacity are re-established at the next exchange
        self._ref = None
        return len(mv)

    def migrate(self, owner_fn=None):
        """Migration inside the library (sz_tile_migrate: library backends): every owned floe goes to the tile that holds its centroid now
        (or to owner_fn(cx, cy)), with its complete state, over the library's own channel (RCCL / the host transport); the context is
        rebuilt from the kept and received floes ordered by global index.  Collective.  Returns the number of floes this rank gave away."""
        w = self.world
        self.sync()
        ov = None
        if owner_fn is not None:
            w._host_stale = True
            n = len(self.gidx)
            cx, cy = w.get("cx")[:n].copy(), w.get("cy")[:n].copy()
            if self.per_x: cx %= self.L
            if self.per_y: cy %= self.L
            ov = np.ascontiguousarray(owner_fn(cx, cy), np.int32)
        px, py = tile_grid(self.nranks)
        sent = C.c_int64(0); owned = C.c_int64(0)
        w._chk(w.L.sz_tile_migrate(w.h, int(px), int(py), capi.ptr(ov, capi._ip) if ov is not None else None, C.byref(sent), C.byref(owned)))
        # the host's copies of the columns are stale now: the columns come back with the next get() (World._pull), the sub-floe points when
        # something asks for them (World._fetch_subpoints) -- a migration itself moves no floe data to the host
        n = int(owned.value)
        w.N = n; w._M = n; w._dirty = False; w._host_stale = True; w._sub = {}; w._sub_on_device = True
        g = np.zeros(max(n, 1), np.int64)
        w._chk(w.L.sz_tile_owned_gidx(w.h, capi.ptr(g, capi._lp), int(g.size)))
        self.gidx = g[:n].copy()
        self.migrate_path = int(w.L.sz_debug_migrate_path(w.h))          # 1: packed on the device, 2: host-staged
        self.boxes = None; self._ref = None
        return int(sent.value)

    # ---- removal and dissolution across tiles (sz_tile_remove_floes: library backends)
    def set_removal(self, on=True, max_vertices=30, min_floe_area=1e6, min_floe_height=0.1):
        """World.set_removal for this rank's tile (the same arguments on every rank).  run(..., stop_on_tags=True) then goes on past a step that
        tagged a floe `remove` on any rank: the collective pass of remove_floes() follows it, unless it is declined -- where the batch ends as before."""
        self.world.set_removal(on, max_vertices, min_floe_area, min_floe_height)

    def _after_pass(self):
        """a removal pass may have compacted the tile and renumbered its floes: N, the global indices and the host's caches follow, as in migrate()"""
        w = self.world
        n = w.stats()["N"]
        g = np.zeros(max(n, 1), np.int64)
        w._chk(w.L.sz_tile_owned_gidx(w.h, capi.ptr(g, capi._lp), int(g.size)))
        if n == len(self.gidx) and np.array_equal(g[:n], self.gidx):
            return
        w.N = n; w._M = n; w._dirty = False; w._host_stale = True; w._sub = {}; w._sub_on_device = True
        self.gidx = g[:n].copy()
        self.boxes = None; self._ref = None

    def remove_floes(self):
        """one pass of remove_floes! over the global floe list (collective): (done, n_removed, n_dissolved) with GLOBAL counts, the same on every
        rank; done == False: declined on every rank, nothing changed.  The floes that stay carry the single context's new numbers (self.gidx)."""
        if self.backend not in ("library", "library-host"):
            raise capi.SzError("TiledWorld.remove_floes needs a library backend (the pass is collective inside libsubzero_hip.so)")
        w = self.world
        d, nr, nd = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        w._chk(w.L.sz_tile_remove_floes(w.h, C.byref(d), C.byref(nr), C.byref(nd)))
        if d.value and (nr.value or nd.value):
            self._after_pass()
        return bool(d.value), int(nr.value), int(nd.value)

    def dissolved(self):
        """this rank's replica of the running ocean.dissolved lattice: the same matrix on every rank"""
        return self.world.dissolved()

    def set_dissolved(self, a):
        """the lattice to go on from: the same matrix on every rank"""
        self.world.set_dissolved(a)

    # ---- fracture criteria across tiles (sz_tile_fracture_candidates, sz_tile_run with a criterion set: library backends)
    def _library_only(self, what):
        if self.backend not in ("library", "library-host"):
            raise capi.SzError(f"TiledWorld.{what} needs a library backend (the pass is collective inside libsubzero_hip.so)")

    def set_fracture(self, kind, dt=75, pstar=2.25e5, c=20.0, poly=None, alpha=0.0, min_floe_area=1e6):
        """World.set_fracture for this rank's tile (the same arguments on every rank).  run(..., stop_on_tags=True) then ends after the first
        fracture step on which a floe of ANY rank would fracture -- the same step on every rank, the step World.run ends on for the undivided list.
        Set it here, not on `self.world`: run() must know Δt to ask at its own cuts."""
        self._library_only("set_fracture")
        self.world.set_fracture(kind, dt, pstar, c, poly, alpha, min_floe_area)
        self._frac_dt = int(dt) if kind != capi.FRAC_OFF else 0

    def _fracture_pass(self, want_rows):
        """one collective criterion pass: (global count, global numbers of this rank's candidates, ascending by local row)"""
        self._library_only("fracture_candidates")
        w = self.world
        ng, no = C.c_int32(0), C.c_int32(0)
        g = np.zeros(max(len(self.gidx), 1), np.int64) if want_rows else None
        w._chk(w.L.sz_tile_fracture_candidates(w.h, C.byref(ng), C.byref(no), None, capi.ptr(g, capi._lp) if want_rows else None))
        return int(ng.value), (g[:no.value].copy() if want_rows else None)

    def fracture_candidates(self):
        """determine_fractures over the global floe list (collective): the 0-based GLOBAL numbers of the floes that would fracture, ascending and
        complete, identical on every rank -- what World.fracture_candidates() returns for the undivided list"""
        ng, mine = self._fracture_pass(True)
        if self.dist is None or self.nranks == 1:
            return np.sort(mine)
        parts = [None] * self.nranks
        self.dist.all_gather_object(parts, mine)
        out = np.sort(np.concatenate(parts))
        assert len(out) == ng, (len(out), ng)
        return out

    def fracture_mean(self):
        """(mean height over the global list, Hibler p) of the last evaluation: the single context's, to the bit, on every rank"""
        return self.world.fracture_mean()

    # ---- welding overlaps across tiles (sz_tile_weld_overlaps, sz_tile_run with welding set: library backends)
    def set_welding(self, dts, nxs, nys, max_weld_area=2e9):
        """World.set_welding for this rank's tile (the same arguments on every rank).  run(..., stop_on_tags=True) then ends after the first
        welding step on which two floes of the global list that could weld overlap -- the same step on every rank, the step World.run ends on
        for the undivided list.  Set it here, not on `self.world`: run() must know the sets to ask at its own cuts."""
        self._library_only("set_welding")
        self.world.set_welding(dts, nxs, nys, max_weld_area)
        d = [int(x) for x in np.ravel(dts)]
        self._weld = (d, [int(x) for x in np.ravel(nxs)], [int(x) for x in np.ravel(nys)], float(max_weld_area)) if d else None

    def _weld_set_at(self, tstep):
        """(nx, ny) of the first welding set with tstep % dt == 0, or None"""
        if self._weld:
            for dt, nx, ny in zip(*self._weld[:3]):
                if tstep % dt == 0:
                    return nx, ny
        return None

    def weld_overlaps(self, nx, ny, max_weld_area=2e9):
        """the welding overlap table of the global floe list (collective): (i, j, inter_area) with 0-based GLOBAL numbers i < j (int64), the whole
        table on every rank -- the rows World.weld_overlaps() returns for the undivided list, in its order, areas to the bit"""
        self._library_only("weld_overlaps")
        w = self.world
        n = C.c_int32(0)
        w._chk(w.L.sz_tile_weld_overlaps(w.h, int(nx), int(ny), float(max_weld_area), C.byref(n), 0, None, None, None))
        cap = max(int(n.value), 1)
        i = np.zeros(cap, np.int64); j = np.zeros(cap, np.int64); a = np.zeros(cap)
        w._chk(w.L.sz_tile_weld_overlaps(w.h, int(nx), int(ny), float(max_weld_area), C.byref(n), cap, capi.ptr(i, capi._lp), capi.ptr(j, capi._lp), capi.ptr(a)))
        return i[:n.value].copy(), j[:n.value].copy(), a[:n.value].copy()

    def weld_bins(self, nx, ny):
        """per owned floe (self.gidx) the 0-based bin of the global list's bin_floe_centroids, or -1 at and behind its first out-of-bounds
        centroid, on whichever rank that floe lives (collective)"""
        self._library_only("weld_bins")
        w = self.world
        b = np.zeros(max(len(self.gidx), 1), np.int32)
        w._chk(w.L.sz_tile_debug_weld_bins(w.h, int(nx), int(ny), capi.ptr(b, capi._ip)))
        return b[:len(self.gidx)].copy()

    def weld_candidate_pairs(self):
        """pairs the last table pass clipped, over all ranks (collective): World.weld_candidate_pairs() of the undivided list"""
        self._library_only("weld_candidate_pairs")
        w = self.world
        n = C.c_int64(0)
        w._chk(w.L.sz_tile_debug_weld_npairs(w.h, C.byref(n)))
        return int(n.value)

    # ---- ridge / raft candidates across tiles (sz_tile_run with ridge / raft set, sz_tile_ridgeraft_candidates: library backends)
    def set_ridgeraft(self, on=True, dt=150, min_ridge_height=0.2, max_floe_ridge_height=5.0, max_domain_ridge_height=1.25,
                      max_floe_raft_height=0.25, max_domain_raft_height=0.25):
        """World.set_ridgeraft for this rank's tile (the same arguments on every rank).  run(..., stop_on_tags=True) then stops on every rank in the
        middle of the first ridge / raft step (tstep % dt == 0) whose candidate table of the global list is not empty -- the step World.run stops
        in for the undivided list: that step is not counted, ridgeraft_pending() names it, the lists keep their halo rows and ghosts,
        ridgeraft_candidates() gives the table and finish_step() runs the rest of the step.  Steps with an empty table are run through."""
        self._library_only("set_ridgeraft")
        self.world.set_ridgeraft(on, dt, min_ridge_height, max_floe_ridge_height, max_domain_ridge_height, max_floe_raft_height, max_domain_raft_height)

    def ridgeraft_pending(self):
        """the timestep whose ridge / raft step is pending, or -1"""
        return self.world.ridgeraft_pending()

    def splice(self, delete=(), replace=None, append=None):
        """World.splice on this rank's context: a tiled context refuses it (its rows carry global numbers and its list is one rank's share), and
        the library's message is raised"""
        return self.world.splice(delete, replace, append)

    # ---- rows down, rows back by global number (sz_tile_download_rows / sz_tile_splice_floes: library backends)
    def download_rows_local(self, gidx):
        """the floes of `gidx` (global numbers, any order, none twice) that THIS rank owns: (which, floes) -- their positions in gidx, ascending,
        and a dict in the layout of World.download_rows with the floes in that order.  Local: no rank waits for another."""
        self._library_only("download_rows_local")
        w = self.world
        w._push_interactions()
        f32 = w._ft == np.float32
        g = np.ascontiguousarray(gidx, np.int64).ravel()
        n = len(g)
        which = np.zeros(max(n, 1), np.int32); nm = C.c_int32(0)
        fn = w.L.sz_tile_download_rows_f32 if f32 else w.L.sz_tile_download_rows
        col = w._rows_down(lambda f, ioff, irows, sizes: fn(w.h, n, capi.ptr(g, capi._lp), C.byref(nm), capi.ptr(which, capi._ip), f, ioff, irows, sizes),
                           lambda: int(nm.value))
        return which[:nm.value].copy(), col

    def download_rows(self, gidx):
        """World.download_rows over the global floe list: the floes `gidx` (global numbers, any order, none twice) in that order, on every rank.
        Collective in Python only -- the local call, then one all_gather_object of what each rank found: the template for a host with its own
        channel (MPI).  Raises when a name was found on no rank."""
        g = np.ascontiguousarray(gidx, np.int64).ravel()
        which, col = self.download_rows_local(g)
        parts = [(which, col)]
        if self.dist is not None and self.nranks > 1:
            parts = [None] * self.nranks
            self.dist.all_gather_object(parts, (which, col))
        pos = np.concatenate([p[0] for p in parts]).astype(np.int64)
        missing = np.setdiff1d(np.arange(len(g)), pos)
        if len(missing) or len(pos) != len(g):
            raise capi.SzError("TiledWorld.download_rows: no rank owns the floes %s (or a floe is owned twice)" % list(g[missing][:8]))
        return _take_rows(_concat_rows([p[1] for p in parts]), np.argsort(pos, kind="stable"))

    def splice_global(self, delete=(), replace=None, append=None, owner=None):
        """World.splice over the global floe list (sz_tile_splice_floes; collective, the same arguments on every rank): `delete` and the rows of
        replace = (rows, floes) are ascending GLOBAL numbers of the list as it is, `append` goes behind the last kept floe of the global list;
        owner[k]: the rank that takes appended floe k (default: the tile that holds its centroid, assign_tiles).  Every rank applies its share;
        afterwards self.gidx holds the single context's new numbers of the floes this rank owns.  Returns (N_global, N_owned)."""
        self._library_only("splice_global")
        w = self.world
        w._push_interactions()
        f32 = w._ft == np.float32
        dele = np.ascontiguousarray(delete, np.int64).ravel()
        rep_rows, rep_cols = (np.zeros(0, np.int64), None) if replace is None else (np.ascontiguousarray(replace[0], np.int64).ravel(), replace[1])
        if rep_cols is not None and len(rep_cols["vert_off"]) - 1 != len(rep_rows):
            raise capi.SzError("splice_global: replace names %d rows and gives %d floes" % (len(rep_rows), len(rep_cols["vert_off"]) - 1))
        col, ioff, irows, ns = World._staged([rep_cols, append])
        n_app = ns - len(rep_rows)
        if n_app and owner is None:
            cx, cy = np.array(col["cx"][len(rep_rows):], float), np.array(col["cy"][len(rep_rows):], float)
            if self.per_x: cx %= self.L
            if self.per_y: cy %= self.L
            owner = assign_tiles(cx, cy, self.L, self.nranks)
        own = np.ascontiguousarray(owner if n_app else np.zeros(0), np.int32).ravel()
        if len(own) != n_app:
            raise capi.SzError("splice_global: %d appended floes and %d owners" % (n_app, len(own)))
        keep = []
        f = w._columns_struct(col, keep) if col is not None else None
        if irows is not None:
            irows = np.ascontiguousarray(irows, w._ft)
        fn = w.L.sz_tile_splice_floes_f32 if f32 else w.L.sz_tile_splice_floes
        ng, no = C.c_int64(0), C.c_int64(0)
        w._chk(fn(w.h, len(dele), capi.ptr(dele, capi._lp), len(rep_rows), capi.ptr(rep_rows, capi._lp), int(n_app), capi.ptr(own, capi._ip) if n_app else None,
                  C.byref(f) if f is not None else None, capi.ptr(ioff, capi._ip) if ioff is not None else None,
                  capi.ptr(irows, capi._fp if f32 else capi._dp) if irows is not None and len(irows) else None, C.byref(ng), C.byref(no)))
        if len(dele) + ns == 0:
            return None, len(self.gidx)
        # the mirror follows, as in _after_pass: count and numbers from the library, columns and sub-floe points fetched on demand; the maxima
        # given to sz_tile_enable cover the staged floes of the whole edit, as the library raised them
        n = int(no.value)
        w.N = n; w._M = n; w._dirty = False; w._host_stale = True; w._sub = {}; w._sub_on_device = True
        g = np.zeros(max(n, 1), np.int64)
        w._chk(w.L.sz_tile_owned_gidx(w.h, capi.ptr(g, capi._lp), int(g.size)))
        self.gidx = g[:n].copy()
        self.boxes = None; self._ref = None
        self.REC = w.L.sz_halo_record_doubles_ctx(w.h)
        if ns:
            if self._max_ring > 0:
                self._max_ring = max(self._max_ring, float(np.diff(col["vert_off"]).max()))
            if self._max_rmax > 0 and "rmax" in col:
                self._max_rmax = max(self._max_rmax, float(np.max(col["rmax"])))
        return int(ng.value), n

    # ---- output frames of a tiled run (sz_tile_set_floe_output / sz_tile_set_grid_output, sz_tile_download_floe_frame: library backends)
    def set_floe_output(self, writer, dt_out, columns=None, arena_bytes=1 << 26, lists=None):
        """World.set_floe_output for this rank's tile (the same arguments on every rank).  run() then goes on past the writer's output steps and
        records there: every rank keeps the frame of its own rows -- its owned floes and their ghosts -- with their order keys.  `lists` is
        refused here: the lists of a tile writer are set through set_floe_output_lists, behind this call."""
        self._library_only("set_floe_output")
        if lists:
            raise capi.SzError("tile frames record no lists yet through set_floe_output: set_floe_output_lists(writer, lists) behind it sets them")
        self.world.set_floe_output(writer, dt_out, columns, arena_bytes, _tile=True)

    def set_floe_output_lists(self, writer, lists):
        """the ragged members (names out of capi.FRAME_LISTS; the same on every rank) a tile writer records behind its columns: called after
        set_floe_output, which resets them; frees the writer's frames.  The merged frame then holds inter_off, inter_rows, sub_off, sx, sy as
        World.floe_frame of a single context's writer with the same lists does, bit for bit"""
        self._library_only("set_floe_output_lists")
        w = self.world
        word = w.frame_lists(lists)
        w._chk(w.L.sz_tile_set_floe_output_lists(w.h, int(writer), word))
        w._floe_lists[int(writer)] = word

    @staticmethod
    def tile_frame_bytes(mask, M, N, V, lists=0, R=0, S=0, K=0):
        """what a tile frame of M local rows (N owned parents), V ring points takes of its writer's arena (TileFrameLayout / TileListLayout,
        csrc/sz_record_tile.hpp): World.frame_bytes, the M order keys, and with lists the K entries of the last step's key table (interactions
        only) and the list sections of R interaction rows and S sub-floe points"""
        lists = World.frame_lists(lists)
        plain = World.frame_bytes(mask, M, N, V)
        return plain + 8 * M + (8 * K if lists & 1 else 0) + World.frame_bytes(mask, M, N, V, lists, R, S) - plain

    def frame_list_keys(self, writer, k):
        """the key table of this rank's tile frame k (local): the sorted order keys of the rows the last step had behind the owned parents"""
        w = self.world
        n = C.c_int64(0)
        w._chk(w.L.sz_tile_floe_frame_list_keys(w.h, int(writer), int(k), C.byref(n), None))
        keys = np.zeros(max(int(n.value), 1), np.int64)
        w._chk(w.L.sz_tile_floe_frame_list_keys(w.h, int(writer), int(k), C.byref(n), capi.ptr(keys, capi._lp)))
        return keys[:int(n.value)].copy()

    def floe_frame_lists_info(self, writer, k):
        """(lists word, interaction rows, sub-floe points) of the MERGED frame k (local: from the counts kept with the frame)"""
        w = self.world
        word = C.c_uint32(0); tot = [C.c_int64(0), C.c_int64(0)]
        w._chk(w.L.sz_tile_floe_frame_lists_info(w.h, int(writer), int(k), C.byref(word), *(C.byref(v) for v in tot)))
        return int(word.value), int(tot[0].value), int(tot[1].value)

    def set_grid_output(self, writer, dt_out, xg=None, yg=None, outputs=None, max_frames=64):
        """World.set_grid_output for this rank's tile (the same arguments on every rank): every rank holds every grid frame, summed over the ranks"""
        self._library_only("set_grid_output")
        self.world.set_grid_output(writer, dt_out, xg, yg, outputs, max_frames, _tile=True)

    def output_frames(self):
        """World.output_frames: the same numbers on every rank (`full` is agreed between the ranks)"""
        return self.world.output_frames()

    def clear_frames(self):
        self.world.clear_frames()

    def floe_frame_local(self, writer, k, members=None):
        """this rank's tile frame k of a writer (local): World.floe_frame over its own rows -- M, N and ghost_idx are local -- plus `key`, the
        order key of every row: a parent's global number, a ghost's (pass << 40) + 4 * parent key + k.  Of a writer with lists also this rank's
        own lists -- the partner column of inter_rows untranslated: global number + 1, or order key + 1 of a ghost of the last step -- and
        `lists`, the word of the lists the frame holds"""
        w = self.world
        fr = w.floe_frame(writer, k, members)
        key = np.zeros(max(fr["M"], 1), np.int64)
        w._chk(w.L.sz_tile_floe_frame_keys(w.h, int(writer), int(k), capi.ptr(key, capi._lp)))
        fr["key"] = key[:fr["M"]].copy()
        return fr

    def floe_frame(self, writer, k, members=None):
        """floe frame k of a writer over the global list (collective: every rank calls it alike): the rows of all ranks merged by order key inside
        the library -- World.floe_frame of the single context's recorded run, bit for bit in every member, the lists of a writer with lists
        included; such a frame also has `lists`, the word of the lists it holds (a frame recorded right behind migrate() has lost its interactions)"""
        self._library_only("floe_frame")
        return self.world.floe_frame(writer, k, members, _merged=True)

    def grid_frame(self, writer, k):
        """grid frame k of a writer: (tstep, array [nout, nx, ny]), the same on every rank"""
        return self.world.grid_frame(writer, k)

    def ridgeraft_draws(self):
        """the per-floe draws of the ridge / raft steps the last run() ran through, over the global list: the same number on every rank"""
        return self._rr_draws

    def ridgeraft_candidates(self):
        """at a pending stop (collective): (i, j, kind, frac, n_draws) of the global list, the whole table on every rank -- what
        World.ridgeraft_candidates() returns for the undivided list, in its numbering and order (int64 numbers), kind and frac to the bit"""
        self._library_only("ridgeraft_candidates")
        w = self.world
        n = C.c_int32(0); nd = C.c_int64(0)
        w._chk(w.L.sz_tile_ridgeraft_candidates(w.h, C.byref(n), 0, None, None, None, None, C.byref(nd)))
        cap = max(int(n.value), 1)
        i = np.zeros(cap, np.int64); j = np.zeros(cap, np.int64); k = np.zeros(cap, np.int32); f = np.zeros(cap)
        w._chk(w.L.sz_tile_ridgeraft_candidates(w.h, C.byref(n), cap, capi.ptr(i, capi._lp), capi.ptr(j, capi._lp), capi.ptr(k, capi._ip), capi.ptr(f), C.byref(nd)))
        m = int(n.value)
        return i[:m].copy(), j[:m].copy(), k[:m].copy(), f[:m].copy(), int(nd.value)

    def _list_column(self, fn):
        w = self.world
        cap = int(w.stats()["M"])
        out = np.zeros(max(cap, 1), np.int64)
        w._chk(fn(w.h, capi.ptr(out, capi._lp), cap))
        return out[:cap].copy()

    def list_numbers(self):
        """at a pending stop: the single context's list number of every local row -- owned floes, halo floes, the ghosts of both, in local order"""
        self._library_only("list_numbers")
        return self._list_column(self.world.L.sz_tile_list_numbers)

    def list_keys(self):
        """at a pending stop: the order key of every local row, in local order; the partner column of a downloaded interaction row holds key + 1"""
        self._library_only("list_keys")
        return self._list_column(self.world.L.sz_tile_list_keys)

    def finish_step(self, tstep, dt, coupling_dt=10, collisions_on=True, coupling_on=True):
        """the second half of the pending ridge / raft step on what the device holds (collective): the halo rows and ghosts are dropped behind it"""
        self._library_only("finish_step")
        w = self.world
        flags = (capi.COLLISIONS_ON if collisions_on else 0) | (capi.COUPLING_ON if coupling_on else 0)
        w._chk(w.L.sz_tile_step_finish(w.h, int(tstep), int(dt), int(coupling_dt), flags))
        w._host_stale = True

    def maybe_repartition(self):
        """Ownership is static between calls of repartition(); floes drift.  Collective: re-tile when more than
        `repartition_fraction` of all floes has left the tile that owns it (cheap test: the owned centroids against the
        tile rule).  Returns the number of floes this rank gave away (0: nothing done)."""
        self.sync(); w = self.world; w._host_stale = True
        n = len(self.gidx)
        cx, cy = w.get("cx")[:n].copy(), w.get("cy")[:n].copy()
        if self.per_x: cx %= self.L
        if self.per_y: cy %= self.L
        away = int(np.count_nonzero(assign_tiles(cx, cy, self.L, self.nranks) != self.rank)) if n else 0
        t = self.torch.tensor([away, n], dtype=self.torch.int64, device="cpu" if self.host_staging else self.dev)
        self.dist.all_reduce(t)
        if int(t[0]) <= self.repartition_fraction * max(int(t[1]), 1):
            return 0
        return self.migrate() if self.backend in ("library", "library-host") else self.repartition()

    def run(self, nsteps, tstep0, dt, coupling_dt=10, collisions_on=True, coupling_on=True, stop_on_tags=False):
        """nsteps x timestep_sim! of the tiled run (collective).  Returns the steps run.  stop_on_tags (library backends): the batch ends
        after the first step that leaves a floe tagged remove / fuse on ANY rank -- the same step on every rank -- as World.run does
        for the single context (the reference runs simplify_floes! after every step, simulation.jl:205-214).  With set_removal() the batch
        goes on past such a step where the collective removal pass is done, and ends there where it is declined.  With set_fracture() it
        ends after the first fracture step (tstep % dt == 0) on which a floe of any rank would fracture, however the batch is cut: with more
        than one rank a batch is cut into calls of `repartition_every` steps (500), the last step of a call is a batch's own last step,
        which sz_tile_run does not look at -- so when that step is a fracture step, run asks for the global candidate count itself and ends
        there if it is positive: run(n) returns what World.run(n) returns.  With set_welding() it likewise ends after the first welding step
        whose overlap table of the global list is not empty, and asks for the table itself where a call's last step is a welding step.  A limit that stays: a floe TAGGED on exactly the last step of a
        call is removed behind the first step of the next call, one step later than World.run(n) would; a caller that needs the single
        context's timing there keeps nsteps within one call or calls remove_floes() itself.  With set_ridgeraft() it returns at a pending
        stop (ridgeraft_pending() >= 0) with the steps before that step, and does not repartition there."""
        done = 0
        self._rr_draws = 0
        while done < nsteps:
            k = min(nsteps - done, self.repartition_every - self._since_check) if self.nranks > 1 else nsteps - done
            if self.backend in ("library", "library-host"):
                w = self.world
                flags = (capi.COLLISIONS_ON if collisions_on else 0) | (capi.COUPLING_ON if coupling_on else 0) | (0 if stop_on_tags else capi.NO_STOP)
                ran = C.c_int32(0)
                w._chk(w.L.sz_tile_run(w.h, int(k), int(tstep0 + done), int(dt), int(coupling_dt), flags, C.byref(ran)))
                w._host_stale = True
                self._rr_draws += w.ridgeraft_draws()
                if stop_on_tags and getattr(w, "_removal_on", False):
                    self._after_pass()
                if ran.value < k:
                    return done + int(ran.value)
                fdt = self._frac_dt
                if stop_on_tags and fdt > 0 and done + k < nsteps and (tstep0 + done + k - 1) % fdt == 0 and self._fracture_pass(False)[0] > 0:
                    self._since_check += k
                    return done + k
                wset = self._weld_set_at(tstep0 + done + k - 1) if stop_on_tags and done + k < nsteps else None
                if wset is not None:          # (behind the fracture pass, as in timestep_sim!)
                    nt = C.c_int32(0)
                    w._chk(w.L.sz_tile_weld_overlaps(w.h, wset[0], wset[1], self._weld[3], C.byref(nt), 0, None, None, None))
                    if nt.value > 0:
                        self._since_check += k
                        return done + k
            else:
                for s in range(k):
                    self.step(tstep0 + done + s, dt, coupling_dt, collisions_on, coupling_on)
                self.sync()
            done += k; self._since_check += k
            if self.nranks > 1 and self._since_check >= self.repartition_every:
                self._since_check = 0
                self.maybe_repartition()
        return done

    def sync(self):
        self.world._chk(self.world.L.sz_sync(self.world.h))

    @property
    def n_halo_last(self):
        self.sync()
        return self.world.stats().get("n_halo", 0)

    def owned(self, name):
        """column `name` of the owned floes (global indices in self.gidx)."""
        return self.world.get(name)[:len(self.gidx)]

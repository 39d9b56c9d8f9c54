"""Column identity (csrc/sz_columns.hpp): every way the engine moves a floe row walks a table of the floe columns, and two entries swapped or one
missing in any of them moves a floe with the wrong values in silence.  Here every column of every floe holds a value that names the column, and
each row mover -- upload and full download, download_rows, splice, their Float32 twins, and a tiled migration on either path -- must hand every
column back as itself, bit for bit.  No step is run, so the values need not be physical.

The field: six squares that do not touch in a periodic domain, floe 1 with sub-floe points.  cx, cy, rmax, area and the rings are the real ones;
every other scalar column k (in capi.DCOLS order) of floe i holds 8 k + i + 0.5, component q of tensor t holds 1000 + 100 t + 8 q + i + 0.5 --
distinct per column and exact in Float32 (what is not, a real rmax or sub-floe point, is compared as the value rounded once)."""
import datetime
import os

import numpy as np
import pytest

import splice_ref as sp
from test_fracture_tiles_gpu import _retile
from test_remove_tiles_gpu import _rank_cols
from test_splice_gpu import _assert_bit_equal, _full, _hand_ring, mk
from test_splice_tiles_gpu import _assert_ranks_equal_single, _tiled
from test_tiles_gpu import _collect, _free_port, _guard

pytestmark = pytest.mark.gpu

CELLS = [0, 1, 2, 3, 4, 6]          # of a 4 x 4 lattice: the west half (rank 0 of two) holds floes 0, 1, 4, the east half 2, 3, 5
REAL = ("cx", "cy", "rmax", "area")
WITH_POINTS = 1


def _field():
    """(cfg for tiles.TiledWorld, the floe list in the layout of World.download_rows)"""
    from subzero_jl_amd import capi, fields, floe as floe_mod
    n, n_side, spacing, side = len(CELLS), 4, 2.0e4, 8.0e3
    L = n_side * spacing
    rings = [_hand_ring(k, n_side, spacing, side, triangle=False) for k in CELLS]
    off = (5 * np.arange(n + 1)).astype(np.int32)
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    d = floe_mod.derive(off, vx, vy, np.full(n, 0.25))
    i = np.arange(n, dtype=np.float64)
    cols = {name: (d[name].copy() if name in REAL else 8.0 * k + i + 0.5) for k, name in enumerate(capi.DCOLS)}
    for t, name in enumerate(capi.TCOLS):
        cols[name] = 1000.0 + 100.0 * t + 8.0 * np.arange(4.0)[None, :] + i[:, None] + 0.5
    cols["id"] = (101 + 7 * np.arange(n)).astype(np.int64); cols["ghost_id"] = np.zeros(n, np.int64); cols["status"] = np.full(n, capi.ACTIVE, np.int32)
    cols["vert_off"], cols["vx"], cols["vy"] = off, vx, vy
    sx, sy = fields.subgrid_points(rings[WITH_POINTS], d["cx"][WITH_POINTS], d["cy"][WITH_POINTS], side / 2.0)
    assert len(sx) > 0
    cols["sub_off"] = np.where(np.arange(n + 1) > WITH_POINTS, len(sx), 0).astype(np.int32); cols["sx"], cols["sy"] = sx, sy
    cols["inter_off"] = np.zeros(n + 1, np.int32); cols["inter_rows"] = np.zeros((0, 7))
    flat = np.concatenate([cols[k].ravel() for k in capi.DCOLS + capi.TCOLS if k not in REAL])
    assert len(set(flat.tolist())) == flat.size and np.array_equal(flat, flat.astype(np.float32)), "a value per column and floe, exact in Float32"
    Nx = Ny = 4 * n_side
    z = np.zeros((Nx + 1, Ny + 1))
    cfg = dict(n_floes=n, L=L, kinds=["periodic"] * 4, vert_off=off, vx=vx, vy=vy, height=np.full(n, 0.25), u=np.zeros(n), v=np.zeros(n), xi=np.zeros(n),
               dt=20, Nx=Nx, Ny=Ny, uo=z, vo=z, hf=z, ua=z, va=z, topography=[], E=6e6, derived=d, sub_off=cols["sub_off"], sx=sx, sy=sy)
    return cfg, cols


def _as(ftype, cols):
    """the list as a host of this float type holds it: every float column rounded once"""
    return {k: (v.astype(ftype).astype(np.float64) if v.dtype == np.float64 else v) for k, v in cols.items()}


def _load(w, cols, L):
    from subzero_jl_amd import capi
    w.set_consts(); w.set_settings()
    w.set_domain([capi.PERIODIC] * 4, 0.0, L, 0.0, L)
    w.load_columns({k: v for k, v in cols.items() if k not in ("sub_off", "sx", "sy", "inter_off", "inter_rows")})
    w.set_subpoints_csr(cols["sub_off"], cols["sx"], cols["sy"])
    w._push()
    return w


@pytest.mark.parametrize("ftype", [np.float64, np.float32], ids=["f64", "f32"])
def test_every_column_comes_back_as_itself(ftype):
    cfg, cols = _field()
    want = _as(ftype, cols)
    w = _load(mk(ftype), cols, cfg["L"])
    _assert_bit_equal(_full(w), want, "upload, then a full download")
    _assert_bit_equal(w.download_rows([4, 1]), sp.take(want, [4, 1]), "download_rows([4, 1])")
    edit = ((), ([2], sp.take(want, [5])), sp.take(want, [0]))
    w.splice(*edit)
    _assert_bit_equal(_full(w), sp.apply(want, *edit), "row 2 replaced by row 5's floe, row 0's appended")


# ---------------------------------------------------------------- two ranks on the one GPU: a migration on either path
def _swap_row_0(L):
    """the floes of the lattice's first row change tiles: two of each rank's three"""
    return lambda cx, cy: np.where(cy < 2.0e4, cx < 0.5 * L, cx > 0.5 * L).astype(int)


def _home(L):
    return lambda cx, cy: (cx > 0.5 * L).astype(int)


def _migrations(rank, world, dist):
    cfg, cols = _field()
    tw = _tiled(cfg, rank, world, dist)
    w, g = tw.world, tw.gidx
    mine = sp.take(cols, g)
    w.load_columns({k: v for k, v in mine.items() if k not in ("sub_off", "sx", "sy", "inter_off", "inter_rows")})
    w.set_subpoints_csr(mine["sub_off"], mine["sx"], mine["sy"])
    _retile(tw)
    out = []
    for env, owner in ((None, _swap_row_0(cfg["L"])), ("1", _home(cfg["L"]))):
        if env:
            os.environ["SZ_MIGRATE_HOST"] = env
        sent = tw.migrate(owner_fn=owner)
        out.append(dict(sent=sent, path=tw.migrate_path, gidx=np.array(tw.gidx), cols=_rank_cols(tw)))
    return out


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        q.put((rank, _migrations(rank, world, dist)))
    finally:
        dist.destroy_process_group()


def _run_worker(*a):
    _guard(_worker)(*a)


def test_a_migration_moves_every_column_as_itself_on_either_path():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue(); port = _free_port()
    procs = [ctx.Process(target=_run_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [out for _, out in sorted(_collect(q, 2), key=lambda r: r[0])]
        for p in procs:
            p.join(60)
        assert all(p.exitcode == 0 for p in procs)
    finally:
        for p in procs:          # a rank left waiting in a collective by a failed peer
            if p.is_alive():
                p.terminate()
    _, cols = _field()
    ref = {k: v for k, v in cols.items() if k not in ("inter_off", "inter_rows")}
    for k, (path, owned) in enumerate(((1, ([2, 3, 4], [0, 1, 5])), (2, ([0, 1, 4], [2, 3, 5])))):
        snaps = [r[k] for r in res]
        assert [s["path"] for s in snaps] == [path, path] and [s["sent"] for s in snaps] == [2, 2], (k, [(s["path"], s["sent"]) for s in snaps])
        assert [list(s["gidx"]) for s in snaps] == [list(o) for o in owned]
        _assert_ranks_equal_single(snaps, ref, "device-packed" if path == 1 else "host-staged")

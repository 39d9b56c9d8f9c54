"""The two scenarios of tests/test_remove_tiles_gpu.py, tests/test_remove_tiles_cpu.py and tools/removal_tile_case.py (which walks them on the
CPU oracle and prints what the tests' docstrings quote)."""
import numpy as np

A_STEPS, B_STEPS = 16, 40


def case_a():
    """12 squares between four open boundaries on [0, 1e5]^2, a 5 x 5 grid of zero fields, no sub-floe points, dt = 10, E = 1e3, coupling off.
    Rows 0, 2, 4, 5, 11 drift into a boundary at 20 m/s; rows 6, 7, 8 (side 900 m: under min_floe_area) carry the masses 2^53, 1, 1 and lie in
    grid cell (xidx, yidx) = (3, 2), which straddles the edge x = 5e4 between two tiles; pairs (1, 9) and (3, 10) are in contact throughout."""
    from subzero_jl_amd import floe as floe_mod
    sq = lambda x0, y0, s=1e4: np.array([[x0, y0], [x0, y0 + s], [x0 + s, y0 + s], [x0 + s, y0], [x0, y0]])
    rings = [sq(8.9e4 + 380, 2.0e4), sq(2.0e4, 6.0e4), sq(650, 1.0e4), sq(4.98e4, 7.0e4), sq(3.0e4, 8.9e4 + 700), sq(7.0e4, 450),
             sq(4.4e4, 3.0e4, 900), sq(5.5e4, 3.1e4, 900), sq(4.6e4, 3.3e4, 900), sq(2.95e4, 6.2e4), sq(4.01e4, 7.1e4), sq(8.8e4 + 400, 4.0e4)]
    n = len(rings)
    u = np.zeros(n); v = np.zeros(n)
    u[0] = 20.0; u[2] = -20.0; v[4] = 20.0; v[5] = -20.0; u[11] = 20.0
    off = np.zeros(n + 1, np.int32); off[1:] = np.cumsum([len(r) for r in rings])
    vx = np.concatenate([r[:, 0] for r in rings]); vy = np.concatenate([r[:, 1] for r in rings])
    h = np.full(n, 0.5)
    z = np.zeros((6, 6))
    cfg = dict(n_floes=n, L=1e5, kinds=["open"] * 4, vert_off=off, vx=vx, vy=vy, height=h, u=u, v=v, xi=np.zeros(n), dt=10,
               Nx=5, Ny=5, uo=z, vo=z, hf=z, ua=z, va=z, topography=[], E=1e3, derived=floe_mod.derive(off, vx, vy, h),
               sub_off=np.zeros(n + 1, np.int32), sx=np.zeros(0), sy=np.zeros(0), seed=0)
    cfg["derived"]["mass"][6:9] = [2.0 ** 53, 1.0, 1.0]
    return cfg


A_RUN = dict(coupling_dt=10, coupling_on=False)
A_OWNERS = [1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 1]


def case_b():
    """400 star floes between four open boundaries on [0, L]^2, every floe 5 m/s faster away from the line x = L / 2: floes leave through the
    west and the east boundary, on every tile of a 2 x 1 and of a 2 x 2 tiling"""
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=400, seed=11, subgrid_per_floe=4.0)
    cfg["kinds"] = ["open"] * 4
    cfg["u"] = cfg["u"] + 5.0 * np.sign(cfg["derived"]["cx"] - 0.5 * cfg["L"])
    return cfg


B_RUN = dict(coupling_dt=1)

"""The HIP engine shadowed step by step by the oracle along long, relaxed trajectories (the state the bench times: a compressed contact
network with multi-region contacts, many neighbours per floe, deep overlaps, limiters that fire).

Two long trajectories cannot be compared tightly: over a few steps a stiff contact network amplifies the round-off by which any two
evaluations differ by orders of magnitude (test_pipelined_batch_full_size_oracle_parity).  So every check here starts the oracle from
the engine's own state (parity.oracle_from, lossless: test_shadow_cpu.py) and takes ONE step on each side: a defect shows at once,
amplification has no steps in which to grow, and the step is held to the 1e-10 contract (parity.compare_worlds: pair list bit-exact,
ids / status, interaction rows and per-floe totals per element, state columns, vertices; the guards that fired equal).
Needs a real MI355X: run with -m gpu."""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

RTOL = 1e-10
ROWS = ("xforce", "yforce", "torque", "overlap", "point", "coll_fx", "coll_fy", "coll_trq")     # compare_worlds reports these as a ratio to the tolerance


def mk():
    import subzero_jl_amd
    return subzero_jl_amd.World(0)


class Shadow:
    """the one-step check, and the largest deviation it met (printed: DESIGN.md quotes it)"""

    def __init__(self, case, cfg):
        self.case, self.cfg, self.worst, self.n = case, cfg, (0.0, None, None), 0

    def step(self, B, k):
        """B holds the state after k steps: restart the oracle from it, step both once (step k), compare"""
        cfg = self.cfg
        ow = parity.oracle_from(B, cfg); ow.set_threads(parity.cores())
        assert B.run(1, k, cfg["dt"], coupling_dt=1, stop_on_tags=False) == 1
        ow.timestep_sim(k, cfg["dt"], coupling_dt=1)
        try:
            res = parity.compare_worlds(B, ow, rtol=RTOL)
            assert np.array_equal(B.warn_counts(), ow.warn_counts()), ("guards that fired", B.warn_counts(), ow.warn_counts())
        except AssertionError as e:
            raise AssertionError(f"{self.case}: step {k} from the engine's state: {e}") from None
        for f, v in res.items():
            d = v * RTOL if f in ROWS else v
            if f != "n_pairs" and d > self.worst[0]:
                self.worst = (d, f, k)
        self.n += 1
        return res

    def report(self):
        d, f, k = self.worst
        print(f"\nSHADOW {self.case}: {self.n} single steps, largest deviation {d:.3e} ({f}, step {k})")


def _assert_bit_equal(a, b, where):
    from oracle import orc
    for f in orc.FIELDS:
        assert np.array_equal(a.get(f), b.get(f)), (where, f)
    for x, y in zip(a.rings(), b.rings()):
        assert np.array_equal(x, y), (where, "rings")
    for x, y in zip(a.interactions(), b.interactions()):
        assert np.array_equal(x, y), (where, "interactions")
    for x, y in zip(a.ids(), b.ids()):
        assert np.array_equal(x, y), (where, "ids / status")
    for x, y in zip(a.pairs(), b.pairs()):
        assert np.array_equal(x, y), (where, "pairs")


@pytest.mark.parametrize("workload", ["configs1", "configs3"])
def test_bench_window_shadowed_and_pipelined_equal(workload):
    """The bench's fields over its whole timed window (steps 55-255 behind 50 relaxation steps).  Context A steps as the bench's runner
    does (pipelined 20-step batches that run through); context B in one-step batches, shadowed at every step 0-59 and every 10th step
    60-250.  Every 20 steps A equals B bit for bit: "pipelined = three-launch" over 260 steps, and through B the pipelined path is held
    to the oracle along the window."""
    from subzero_jl_amd import fields
    cfg = parity.bench_cfg(workload)
    dt = cfg["dt"]
    A = fields.build_world(mk(), cfg); B = fields.build_world(mk(), cfg)
    sh = Shadow(workload, cfg)
    for k in range(260):
        if k % 20 == 0:
            if k:
                _assert_bit_equal(A, B, f"{workload}: pipelined A against one-step B at step {k}")
            assert A.run(20, k, dt, coupling_dt=1, stop_on_tags=False) == 20
            assert A.pipelined()
        if k < 60 or k % 10 == 0:
            sh.step(B, k)
        else:
            assert B.run(1, k, dt, coupling_dt=1, stop_on_tags=False) == 1
    _assert_bit_equal(A, B, f"{workload}: pipelined A against one-step B at step 260")
    assert np.count_nonzero(B.get("overarea")) > cfg["n_floes"] // 2          # the network is in contact
    sh.report()


def test_relaxed_state_uploads_losslessly():
    """run_resident! resumes after host-side fracturing by uploading the state it downloaded: at step 50 of configs[1], B's downloaded
    state uploaded into a fresh context steps like B, one step and then a 20-step pipelined batch, bit for bit."""
    from subzero_jl_amd import capi, fields
    cfg = parity.bench_cfg("configs1")
    dt = cfg["dt"]
    B = fields.build_world(mk(), cfg)
    assert B.run(50, 0, dt, coupling_dt=1, stop_on_tags=False) == 50
    cols = {n: B.get(n) for n in capi.DCOLS}
    for n, pre in (("stress_accum", "sa"), ("stress_instant", "si"), ("strain", "e")):
        cols[n] = np.stack([B.get(pre + c) for c in ("11", "12", "21", "22")], 1)
    ids, gids, status = B.ids()
    off, x, y = B.rings()
    assert B.M == cfg["n_floes"] and not np.any(gids)
    cols.update(id=ids, ghost_id=gids, status=status, vert_off=off.copy(), vx=x.copy(), vy=y.copy())
    C = fields.build_world(mk(), cfg)
    C.load_columns(cols)
    C.set_subpoints_csr(*B.subpoints())
    for w in (B, C):
        assert w.run(1, 50, dt, coupling_dt=1, stop_on_tags=False) == 1
    _assert_bit_equal(B, C, "one step after the upload")
    for w in (B, C):
        assert w.run(20, 51, dt, coupling_dt=1, stop_on_tags=False) == 20
        assert w.pipelined()
    _assert_bit_equal(B, C, "a pipelined batch after the upload")
    assert np.array_equal(B.warn_counts(), C.warn_counts())


def test_voronoi_field_shadowed():
    """The reference's own field generator: Voronoi cells that touch along whole edges, so every contact starts degenerate (collinear
    edges, shared vertices, zero-area overlaps) and becomes a sliver.  test_voronoi_field_touching_cells can hold such a trajectory only
    to 1e-6; each of its steps, taken from the engine's state, to 1e-10."""
    from subzero_jl_amd import fields
    cfg = fields.make_config(n_floes=1500, seed=5, spacing=1.0e4, shape="voronoi", ocean="shear", concentration=1.0)
    B = fields.build_world(mk(), cfg)
    sh = Shadow("voronoi", cfg)
    for k in range(41):
        sh.step(B, k)
    assert np.count_nonzero(B.get("overarea")) > cfg["n_floes"] // 4
    sh.report()


def test_configs2_100k_shadowed():
    """configs[2], 100 000 floes in one context: the three-launch steps of a field above the pipelining limit, with the forcings in a
    launch of their own (above 65 536 floes), shadowed at steps 0, 20 and 40."""
    cfg = parity.bench_cfg("configs2")
    from subzero_jl_amd import fields
    dt = cfg["dt"]
    B = fields.build_world(mk(), cfg)
    sh = Shadow("configs2", cfg)
    for k in (0, 20, 40):
        sh.step(B, k)
        if k < 40:
            assert B.run(19, k + 1, dt, coupling_dt=1, stop_on_tags=False) == 19
            assert not B.pipelined()
    sh.report()

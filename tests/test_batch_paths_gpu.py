"""Which driver a resident batch takes, as a decision table (csrc/sz_api.hip: plan_batch, pipeline_eligible), observed through the hooks a
profile reader has: World.pipelined(), World.forcing_launch(), World.narrow_kernel_name() and the step count run() returns.

One small field per row: 300 floes at concentration 0.8, periodic unless the row says otherwise, coupled every step, one run() of the
stated length with the tag stop on unless the row says otherwise.

The path column follows from pipeline_eligible: pipelined batches need pipe_min_steps = 4 steps or more, no SZ_PIPELINE=0, fp64, one-way
coupling, no fracture criterion, collisions on, and either inline ghosts (periodic walls) or walls that do not move.  A parent that is tagged
before the batch and SZ_NO_STOP do not change the path.

The launch column was recorded once from the commit before plan_batch existed, on the GPU.  The rules that give it:
 - forcing_launch: forcing_fuse_mode -- with collisions on and one-way coupling the forcings of a field this small ride in the narrow
   launch's tail (2) on either path; two-way coupling and steps without collisions give them a launch of their own (0);
 - narrow_kernel_name: sz_k_narrow<.., FRC, GEO> -- FRC is the flavour of the forcing tail (0 none, 1 fp64, 2 mixed precision), GEO = 1 is
   the pipelined first launch (narrow | GEO | forcings)."""
import os

import numpy as np
import pytest

import cases
import fracture_ref as fr

pytestmark = pytest.mark.gpu

N_FLOES = 300
WALLS = dict(walls=True, topography=True, ocean="strait")


def _mixed(w, cfg):
    w.set_precision("mixed")


def _two_way(w, cfg):
    w.set_two_way(True, dt=cfg["dt"]); w.set_temps(0.0, 0.0)


def _never_fractures(w, cfg):
    from subzero_jl_amd import capi
    w.set_fracture(capi.FRAC_POLYGON, dt=5, poly=fr.huge_square(), min_floe_area=1e6)


def _tagged_before(w, cfg):
    st = np.full(cfg["n_floes"], cases.ACTIVE, np.int32); st[17] = cases.FUSE
    w.set_status(st)


# id: (steps, environment at create, make_config arguments, setup, run() arguments), (steps returned, pipelined, forcing_launch, narrow_kernel_name)
NARROW = "sz_k_narrow<%s,%d,%d>"
ROWS = {
    "3-steps":          ((3, {}, {}, None, {}),                           (3, False, 2, (1, 0))),
    "4-steps":          ((4, {}, {}, None, {}),                           (4, True, 2, (1, 1))),
    "pipeline-off":     ((8, {"SZ_PIPELINE": "0"}, {}, None, {}),         (8, False, 2, (1, 0))),
    "mixed-precision":  ((8, {}, {}, _mixed, {}),                         (8, False, 2, (2, 0))),
    "two-way":          ((8, {}, {}, _two_way, {}),                       (8, False, 0, (0, 0))),
    "fracture-set":     ((8, {}, {}, _never_fractures, {}),               (8, False, 2, (1, 0))),
    "collisions-off":   ((8, {}, {}, None, {"collisions_on": False}),     (8, False, 0, (0, 0))),
    "walls-topography": ((8, {}, WALLS, None, {}),                        (8, True, 2, (1, 1))),
    "tagged-before":    ((8, {}, {}, _tagged_before, {}),                 (1, True, 2, (1, 1))),          # (the tagged parent ends the batch at its first step)
    "run-through":      ((8, {}, {}, None, {"stop_on_tags": False}),      (8, True, 2, (1, 1))),
}
NARROW_HEAD = "8,18,8,16,4,64,0,0,3"          # the arguments of sz_k_narrow before FRC and GEO (NARROW_FIRST_ARGS): the same in every row


def observe(row_id):
    """(steps returned, pipelined, forcing_launch, narrow_kernel_name) of one row's batch"""
    import subzero_jl_amd
    from subzero_jl_amd import fields
    (nsteps, env, cfg_args, setup, run_args), _ = ROWS[row_id]
    cfg = fields.make_config(n_floes=N_FLOES, seed=31, concentration=0.8, **cfg_args)
    os.environ.update(env)
    try:
        w = subzero_jl_amd.World(0)
    finally:
        for k in env:
            del os.environ[k]
    fields.build_world(w, cfg)
    if setup:
        setup(w, cfg)
    done = w.run(nsteps, 0, cfg["dt"], coupling_dt=1, **run_args)
    return done, w.pipelined(), w.forcing_launch(), w.narrow_kernel_name()


@pytest.mark.parametrize("row_id", list(ROWS))
def test_batch_takes_the_planned_path(row_id):
    done, pipelined, forcing, name = observe(row_id)
    print(row_id, done, pipelined, forcing, name)
    want_done, want_pipelined, want_forcing, (frc, geo) = ROWS[row_id][1]
    assert pipelined is want_pipelined
    assert done == want_done
    assert forcing == want_forcing
    assert name == NARROW % (NARROW_HEAD, frc, geo)

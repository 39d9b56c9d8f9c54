"""stops_ref.segments with the output steps of registered writers: write_data! runs at the START of a step, right behind add_ghosts!
(simulation.jl:102-105), so an output step is a visit of the host in front of the step -- as a ridge / raft step is, whose first half is not
the earlier steps' either."""
import stops_ref


def is_output_step(out_dts, t):
    return any(d and t % d == 0 for d in out_dts)


def segments(tstep0, nsteps, rr_dt, frac_dt, weld_dts, cut_on_fracture, out_dts):
    """[(first step, last step, is a ridge / raft step)]: the runs of steps between two visits of the host"""
    out, first, end = [], tstep0, tstep0 + nsteps
    for t in range(tstep0, end):
        middle = bool(rr_dt) and t % rr_dt == 0
        behind = stops_ref.weld_set(weld_dts, t) >= 0 or (cut_on_fracture and bool(frac_dt) and t % frac_dt == 0)
        if (middle or is_output_step(out_dts, t)) and first < t:          # an output step t with first < t ends the run at t - 1
            out.append((first, t - 1, False))
            first = t
        if middle or behind or t == end - 1:
            out.append((first, t, middle))
            first = t + 1
    return out


def frames(tstep0, steps_done, pending, out_dts):
    """the output steps a batch that ran steps_done steps from tstep0 has recorded: those at which it BEGAN a step -- a ridge / raft step left
    pending (not counted in steps_done) included, the batch's end step not"""
    return [t for t in range(tstep0, tstep0 + steps_done + (1 if pending else 0)) if is_output_step(out_dts, t)]

"""Where a resident batch needs the host, walked step by step from the reference's order inside a timestep (simulation.jl:121-136, 172-214):
timestep_ridging_rafting! stands in the middle of its step, fracture_floes! and timestep_welding! behind theirs."""


def weld_set(weld_dts, t):
    """findfirst(x -> mod(tstep, x) == 0, Δts), 0-based, or -1"""
    return next((k for k, d in enumerate(weld_dts) if t % d == 0), -1)


def segments(tstep0, nsteps, rr_dt, frac_dt, weld_dts, cut_on_fracture):
    """[(first step, last step, is a ridge / raft step)]: the runs of steps between two visits of the host"""
    out, first, end = [], tstep0, tstep0 + nsteps
    for t in range(tstep0, end):
        middle = bool(rr_dt) and t % rr_dt == 0
        behind = weld_set(weld_dts, t) >= 0 or (cut_on_fracture and bool(frac_dt) and t % frac_dt == 0)
        if middle and first < t:          # the steps before it end here: its first half is not theirs
            out.append((first, t - 1, False))
            first = t
        if middle or behind or t == end - 1:
            out.append((first, t, middle))
            first = t + 1
    return out

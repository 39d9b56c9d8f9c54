"""The cutter of the stop schedule (csrc/sz_stops.hpp: next_segment, which sz_step and sz_tile_run share) against a step-by-step walk of the
reference's order (stops_ref.py), exhaustively over small settings.  No context, no device call: sz_debug_next_segment."""
import ctypes
import itertools

from subzero_jl_amd import capi

import stops_ref

DTS = range(0, 6)                                   # rr_dt, frac_dt: 0 = off
WELDS = [[]] + [[k] for k in range(1, 6)] + [[j, k] for j in range(1, 6) for k in range(1, 6)]
TSTEP0S = range(0, 11)
NSTEPS = range(0, 12)


def _cutter():
    L = capi.load()
    out = (ctypes.c_int32 * 4)()

    def cut(t, remaining, rr_dt, frac_dt, cof, n_weld, dts):
        assert L.sz_debug_next_segment(t, remaining, rr_dt, frac_dt, cof, n_weld, dts, out) == 0
        return out[0], out[1], out[2], out[3]
    return cut


def test_two_sets_on_one_step_give_the_first():
    cut = _cutter()
    dts = (ctypes.c_int32 * 2)(6, 4)
    assert cut(11, 5, 0, 0, 0, 2, dts) == (0, 2, 0, 0)          # tstep 12: both divide it
    assert cut(7, 5, 0, 0, 0, 2, dts) == (0, 2, 0, 1)           # tstep 8: only the second
    assert cut(11, 2, 0, 0, 0, 2, dts) == (0, 2, 0, 0)          # (the batch's last step: no cut, described all the same)


def test_segments_against_the_reference_order():
    cut = _cutter()
    n_calls = 0
    for weld, rr_dt, frac_dt, cof in itertools.product(WELDS, DTS, DTS, (0, 1)):
        dts = (ctypes.c_int32 * max(len(weld), 1))(*weld)
        what = f"rr_dt={rr_dt} frac_dt={frac_dt} weld={weld} cut_on_fracture={cof}"
        is_rr = [bool(rr_dt) and t % rr_dt == 0 for t in range(32)]
        is_f = [bool(frac_dt) and t % frac_dt == 0 for t in range(32)]
        wset = [stops_ref.weld_set(weld, t) for t in range(32)]
        memo = {}
        for tstep0, nsteps in itertools.product(TSTEP0S, NSTEPS):
            end = tstep0 + nsteps
            segs, t = [], tstep0
            while t < end:
                g = memo.get((t, end))
                if g is None:          # (the cutter keeps no state: a call is checked once for each setting)
                    g = memo[(t, end)] = cut(t, end - t, rr_dt, frac_dt, cof, len(weld), dts)
                    n_calls += 1
                    rr, ln, fstep, ws = g
                    assert ln >= 1, (what, t, end, g)
                    last = t + ln - 1
                    # the segments tile the batch; a ridge / raft step is a segment of its own and lies in no other
                    assert last < end, (what, t, end, g)
                    assert bool(rr) == is_rr[t] and (not rr or ln == 1), (what, t, end, g)
                    assert not any(is_rr[t + 1:last + 1]), (what, t, end, g)
                    # a welding step (a fracture step where those cut) before the batch's last step is a segment's last step
                    assert not any(wset[u] >= 0 or (cof and is_f[u]) for u in range(t, last)), (what, t, end, g)
                    # the last step is described: the first matching set
                    assert bool(fstep) == is_f[last] and ws == wset[last], (what, t, end, g)
                segs.append((t, t + g[1] - 1, bool(g[0])))
                t += g[1]
            if nsteps == 0:
                assert cut(t, 0, rr_dt, frac_dt, cof, len(weld), dts) == (0, 0, 0, -1), (what, t)
            # ... and each is as long as the walk allows
            assert segs == stops_ref.segments(tstep0, nsteps, rr_dt, frac_dt, weld, bool(cof)), (what, tstep0, nsteps)
    assert n_calls > 100000

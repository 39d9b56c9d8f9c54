"""The cutter of the stop schedule with output intervals (csrc/sz_stops.hpp: next_segment with StopRules::out_dts, through
sz_debug_next_segment_out) against the step-by-step walk of stops_out_ref.py, exhaustively over the settings tests/test_stops_cpu.py uses and
out_dts in OUTS.  No context, no device call."""
import ctypes
import itertools
import os
import re

import pytest

from subzero_jl_amd import capi

import stops_out_ref
import stops_ref
from test_stops_cpu import DTS, NSTEPS, TSTEP0S, WELDS

OUTS = [[], [1], [3], [4], [2, 5]]


def _arr(v):
    return (ctypes.c_int32 * max(len(v), 1))(*v)


@pytest.mark.parametrize("outs", OUTS, ids=lambda o: "out_dts=" + "-".join(map(str, o)))
def test_segments_with_output_steps_against_the_reference_order(outs):
    L = capi.load()
    out4, old4 = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    n_calls = 0
    for weld, rr_dt, frac_dt, cof in itertools.product(WELDS, DTS, DTS, (0, 1)):
        dts, odts = _arr(weld), _arr(outs)
        what = f"rr_dt={rr_dt} frac_dt={frac_dt} weld={weld} cut_on_fracture={cof} out_dts={outs}"
        memo = {}
        for tstep0, nsteps in itertools.product(TSTEP0S, NSTEPS):
            end = tstep0 + nsteps
            segs, t = [], tstep0
            while t < end:
                g = memo.get((t, end))
                if g is None:          # (the cutter keeps no state: a call is made once for each setting)
                    assert L.sz_debug_next_segment_out(t, end - t, rr_dt, frac_dt, cof, len(weld), dts, len(outs), odts, out4) == 0
                    g = memo[(t, end)] = tuple(out4)
                    n_calls += 1
                    rr, ln, fstep, ws = g
                    assert ln >= 1 and t + ln <= end, (what, t, end, g)
                    last = t + ln - 1
                    # no output step inside a segment behind its first step; the last step is described as before
                    assert not any(stops_out_ref.is_output_step(outs, u) for u in range(t + 1, last + 1)), (what, t, end, g)
                    assert bool(fstep) == (bool(frac_dt) and last % frac_dt == 0) and ws == stops_ref.weld_set(weld, last), (what, t, end, g)
                    if not outs:       # no writer: the answers of the cutter as it was
                        assert L.sz_debug_next_segment(t, end - t, rr_dt, frac_dt, cof, len(weld), dts, old4) == 0
                        assert tuple(old4) == g, (what, t, end)
                segs.append((t, t + g[1] - 1, bool(g[0])))
                t += g[1]
            assert segs == stops_out_ref.segments(tstep0, nsteps, rr_dt, frac_dt, weld, bool(cof), outs), (what, tstep0, nsteps)
            if not outs:
                assert segs == stops_ref.segments(tstep0, nsteps, rr_dt, frac_dt, weld, bool(cof)), (what, tstep0, nsteps)
    assert n_calls > 100000


def test_a_writer_that_is_off_cuts_nothing_and_bad_arguments_are_refused():
    L = capi.load()
    a, b = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    none = _arr([])
    assert L.sz_debug_next_segment_out(3, 20, 0, 0, 0, 0, none, 3, _arr([0, 0, 0]), a) == 0 and tuple(a) == (0, 20, 0, -1)
    assert L.sz_debug_next_segment_out(3, 20, 0, 0, 0, 0, none, 3, _arr([0, 7, 0]), a) == 0 and tuple(a) == (0, 4, 0, -1)
    # a ridge / raft step that is also an output step stays a one-step segment; the step in front of it ends its segment once
    assert L.sz_debug_next_segment_out(10, 20, 5, 0, 0, 0, none, 1, _arr([5]), a) == 0 and tuple(a) == (1, 1, 0, -1)
    assert L.sz_debug_next_segment_out(6, 20, 5, 0, 0, 0, none, 1, _arr([5]), a) == 0
    assert L.sz_debug_next_segment(6, 20, 5, 0, 0, 0, none, b) == 0 and tuple(a) == tuple(b) == (0, 4, 0, -1)
    assert L.sz_debug_next_segment_out(0, 5, 0, 0, 0, 0, none, 1, _arr([-2]), a) == -2
    assert L.sz_debug_next_segment_out(0, 5, 0, 0, 0, 0, none, 1, None, a) == -2


def test_frame_bits_are_the_struct_order():
    """the mask bits the header publishes (sz_debug_frame_bits) are the binding's list: the double columns as sz_debug_column_names orders
    them, then id, ghost_id, status, rings, ghost_links"""
    L = capi.load()
    bits = L.sz_debug_frame_bits().decode().split()
    assert bits == capi.FRAME_BITS and len(bits) == 33
    assert bits[:28] == L.sz_debug_column_names().decode().split()
    fields = [n for n, _ in capi.SzFloeColumns._fields_]
    members = [m for b in bits for m in capi.FRAME_MEMBERS.get(b, [b])]
    assert members == [f for f in fields if f not in ("sub_off", "sx", "sy")]          # struct order, the sub-floe points left out
    # ... and the list julia/SubzeroHIP.jl keeps by hand, with the groups its FloeOutputWriter outputs ask for
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "julia", "SubzeroHIP.jl")).read()
    jl = re.search(r"^const FRAME_BITS = \((.*?)\)$", src, re.S | re.M).group(1)
    assert re.findall(r":(\w+)", jl) == bits
    outputs = re.search(r"^const FRAME_OUTPUTS = Dict\{Symbol, Vector\{Symbol\}\}\((.*?)\)$", src, re.S | re.M).group(1)
    groups = {g for lst in re.findall(r"=> \[(.*?)\]", outputs) for g in re.findall(r":(\w+)", lst)}
    assert groups and groups <= set(bits)

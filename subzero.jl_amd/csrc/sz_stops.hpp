// The stop schedule of resident batches: where sz_step and sz_tile_run cut a batch into segments and what follows a segment, stated once.
// Host-only C++, no HIP and no sz_ctx (the contexts come in as template arguments).  DESIGN.md, "Stop schedule", has the table of hooks.
//
// The rule is the reference's order inside a timestep: timestep_ridging_rafting! runs in the MIDDLE of the step (simulation.jl:121-136); BEHIND
// it come fracture_floes!, timestep_welding! for the first set k with tstep % Δts[k] == 0, then simplify_floes! (simulation.jl:172-214).  Each
// needs the host only where it would change a floe, so a batch stops only there:
//   - a ridge / raft step is a one-step segment, split around the candidate pass.  Table not empty: the batch ends with the step PENDING
//     (steps_done does not count it; sz_step_finish / sz_tile_step_finish runs the second half).  Empty: the reference's call would change no
//     floe and draw exactly the per-floe draws (sz_ridgeraft_draws); the second half runs and the step ends as any segment's last step does;
//   - every other segment is an ordinary batch, the longest that holds no later ridge / raft step and ends on the first welding step -- or
//     fracture step, where the criterion runs behind the segment (cut_on_fracture);
//   - behind a segment whose last step t ran, in that order: a fracture candidate ends the batch (steps_done counts t); on a welding step a tag
//     ends it, removal set or not (the caller works through the step and removes the floes itself), and so does an overlap table that is not
//     empty; elsewhere a tag goes to the removal pass, and ends the batch where removal is not set or the pass declines; else on at t + 1;
//   - the batch's own last step is never looked at: the caller sees what kind of step the batch ended on and asks;
//   - an output step of a registered writer (StopRules::out_dts, the recorder of sz_record.hpp) is a cut BEFORE the step, as in front of a
//     ridge / raft step: write_data! runs at the start of a step, right behind add_ghosts! (simulation.jl:102-105).  record() takes the frames
//     in front of the segment that starts there; the passes behind the segment that ends there run as behind any other cut.
// Output frames: every output step at which a batch BEGINS A STEP has exactly one frame per due writer, taken before the step -- the batch's
// first step and a ridge / raft step that is left pending included (its frame belongs to the start of the step; the next batch starts behind
// it).  The batch's end step, tstep0 + steps_done, has none: the next call records it.  A frame that finds no room ends the batch there with
// SZ_OK, the step not begun.
// What differs between the two contexts is in the rules and the ops, nowhere else:
//   - the single context's three-launch driver evaluates the criterion inside the batch, and a candidate arrives as a stop, as a tag does
//     (SingleStops::fracture asks which only where a tag alone would let the batch go on).  On tiles the pass is collective, behind a cut;
//   - on tiles `tag` is every rank's knowledge only once `settled`: a tag of a segment's last step is, behind the list-based driver, this rank's
//     own word (the peers would hear of it in the unpack of a step that does not come).  The next pass carries it in its agreement and returns
//     the ranks' OR; where the step has no pass -- a cut before a ridge / raft step -- settle() agrees on it;
//   - a tag that the second half of a tiled ridge / raft step has agreed counts as not settled all the same: it still goes through that step's
//     welding pass before it ends the batch (the single context returns without the pass).  Kept as it was; only settle() skips it.
// Collective calls on tiles: every hook but a settle() behind a ridge / raft step is one, so every rank must make the same calls in the same
// order.  nsteps, tstep0 and the rules are the same everywhere (sz_tile_run's contract), so next_segment() cuts alike; both tile drivers end a
// segment at the same `ran` on every rank (a stop before its last step is agreed inside them), so t, fstep, weld_set and settled are the same;
// pending, cand, the table's length, ok and a returned tag are agreed inside their hooks, an error of one rank is every rank's
// (comm_agree_bits).  No branch below reads anything else -- never a tag that is not settled.
#pragma once
#include "../../include/subzero_hip.h"

namespace sz {
struct StopRules {
  int rr_dt, frac_dt;                   // RidgeRaftSettings.Δt (0: off), FractureSettings.Δt (0: no criterion)
  const int* weld_dts; int n_weld;      // WeldSettings.Δts, in the reference's order
  bool cut_on_fracture;                 // tiles: the passes are collective, the criterion's runs behind a segment, not inside the batch
  bool removal;                         // a tag goes to the removal pass
  const int* out_dts = nullptr; int n_out = 0;      // the Δtout of the registered output writers (an entry <= 0: that writer is off); none by default
};
// the two call sites (sz_step on a tiled context has no pass for any of the four: removal is not engaged there, the others are refused)
template <class Ctx> StopRules single_stop_rules(const Ctx& c) {
  return { c.rr_on ? c.rr_dt : 0, c.frac_kind != SZ_FRAC_OFF ? c.frac_dt : 0, c.weld_dts.data(), (int)c.weld_dts.size(), false, c.rm_on && !c.S.tiled };
}
template <class Ctx> StopRules tile_stop_rules(const Ctx& c) { StopRules r = single_stop_rules(c); r.cut_on_fracture = true; r.removal = c.rm_on; return r; }

inline bool step_due(int dt, int tstep) { return dt > 0 && tstep % dt == 0; }
inline bool is_fracture_step(int frac_dt, int tstep) { return step_due(frac_dt, tstep); }
// an output step of any registered writer
inline bool is_output_step(const StopRules& r, int tstep) {
  for (int k = 0; k < r.n_out; k++) if (step_due(r.out_dts[k], tstep)) return true;
  return false;
}
// the welding set of timestep tstep: the FIRST k with tstep % dts[k] == 0 (findfirst, simulation.jl:186-189), or -1
inline int weld_set_at(const StopRules& r, int tstep) {
  for (int k = 0; k < r.n_weld; k++) if (tstep % r.weld_dts[k] == 0) return k;
  return -1;
}

struct Segment { bool rr_step; int len; bool fstep; int weld_set; };          // fstep, weld_set: of its last step
// The segment that starts at tstep with `remaining` steps of the batch left.  A cut is only made where the batch goes on behind it.
inline Segment next_segment(const StopRules& r, int tstep, int remaining) {
  Segment g = { false, remaining > 0 ? remaining : 0, false, -1 };
  if (g.len == 0) return g;
  if (step_due(r.rr_dt, tstep)) { g.rr_step = true; g.len = 1; }
  else for (int s = 0; s + 1 < remaining; s++)
    if (weld_set_at(r, tstep + s) >= 0 || (r.cut_on_fracture && is_fracture_step(r.frac_dt, tstep + s)) || step_due(r.rr_dt, tstep + s + 1) ||
        is_output_step(r, tstep + s + 1)) { g.len = s + 1; break; }
  g.fstep = is_fracture_step(r.frac_dt, tstep + g.len - 1); g.weld_set = weld_set_at(r, tstep + g.len - 1);
  return g;
}

// The batch [tstep0, tstep0 + nsteps) in segments.  Every hook of ops returns an SZ_* code, which ends the batch; flags are 0 / 1.  tag: a stop
// request ended the segment early or was raised on its last step; fracture() and weld() take this rank's and return the settled one; last: the
// batch's last step, nothing behind it is looked at; ok: the removal pass is done, the batch may go on; full: a frame of the output step found
// no room, the batch ends in front of that step.
template <class Ops>
int run_with_stops(const StopRules& r, Ops& ops, int nsteps, int tstep0, int32_t* steps_done) {
  for (int done = 0; done < nsteps;) {
    int ran = 0, rc = SZ_OK, pending = 0, tag = 0, full = 0;
    if (is_output_step(r, tstep0 + done) && ((rc = ops.record(tstep0 + done, &full)) || full)) return rc;          // write_data!
    Segment g = next_segment(r, tstep0 + done, nsteps - done);
    if (g.rr_step) {
      if ((rc = ops.rr_step(tstep0 + done, done + 1 == nsteps, &pending, &tag)) || pending) return rc;
      ran = 1;
    } else rc = ops.segment(g.len, tstep0 + done, &ran, &tag);
    done += ran;
    if (steps_done) *steps_done = done;
    if (rc || done >= nsteps || ran < 1) return rc;
    const int t = tstep0 + done - 1;
    bool settled = !r.cut_on_fracture || ran < g.len;
    if (ran < g.len) { g.fstep = is_fracture_step(r.frac_dt, t); g.weld_set = weld_set_at(r, t); }          // (a stop ended the segment early, at t)
    if (g.fstep && (r.cut_on_fracture || tag)) {          // fracture_floes! (inside the batch a candidate can only hide in a stop)
      int cand = 0;
      if ((rc = ops.fracture(t, g.weld_set, &cand, &tag)) || cand) return rc;
      settled = true;
    }
    if (g.weld_set >= 0) {                                // timestep_welding!
      int nt = 0;
      if ((settled && tag) || (rc = ops.weld(g.weld_set, &nt, &tag)) || tag || nt > 0) return rc;
      settled = true;
    }
    if (!settled && (rc = ops.settle(&tag))) return rc;          // simplify_floes!
    if (!tag) continue;
    int ok = 0;
    if (!r.removal || (rc = ops.remove(&ok)) || !ok) return rc;
  }
  return SZ_OK;
}
}  // namespace sz

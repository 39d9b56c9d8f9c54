// stops_out_check.cpp — the cutter of the stop schedule (csrc/sz_stops.hpp: next_segment with output intervals) against a step-by-step walk, as
// a stand-alone host program: sz_stops.hpp is host-only C++, so it can run under the host sanitizers.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/stops_out_check.cpp -o stops_out_check && ./stops_out_check
// The grid is that of tests/test_output_stops_cpu.py: rr_dt, frac_dt in 0..5, the welding sets {}, {k}, {j, k} for j, k in 1..5, cut_on_fracture
// 0 / 1, out_dts in {}, {1}, {3}, {4}, {2, 5}, tstep0 in 0..10, nsteps in 0..11.  Exit status 0 and a count when every batch is cut as the walk says.
#include <cstdio>
#include <vector>
#include "../subzero.jl_amd/csrc/sz_stops.hpp"

using namespace sz;

struct Run { int first, last; bool rr; bool operator==(const Run& o) const { return first == o.first && last == o.last && rr == o.rr; } };

// the runs of steps between two visits of the host, walked step by step (tests/stops_out_ref.py)
static std::vector<Run> walk(const StopRules& r, int tstep0, int nsteps) {
  std::vector<Run> out;
  int first = tstep0;
  const int end = tstep0 + nsteps;
  for (int t = tstep0; t < end; t++) {
    const bool middle = step_due(r.rr_dt, t);
    const bool behind = weld_set_at(r, t) >= 0 || (r.cut_on_fracture && step_due(r.frac_dt, t));
    if ((middle || is_output_step(r, t)) && first < t) { out.push_back({ first, t - 1, false }); first = t; }
    if (middle || behind || t == end - 1) { out.push_back({ first, t, middle }); first = t + 1; }
  }
  return out;
}

int main() {
  std::vector<std::vector<int>> welds = { {} }, outs = { {}, { 1 }, { 3 }, { 4 }, { 2, 5 } };
  for (int k = 1; k <= 5; k++) welds.push_back({ k });
  for (int j = 1; j <= 5; j++) for (int k = 1; k <= 5; k++) welds.push_back({ j, k });
  long long batches = 0, cuts = 0;
  for (const auto& w : welds) for (const auto& o : outs) for (int rr_dt = 0; rr_dt <= 5; rr_dt++) for (int frac_dt = 0; frac_dt <= 5; frac_dt++) for (int cof = 0; cof <= 1; cof++) {
    // (exact-size copies on the heap: a read past the end of either list is the sanitizer's to find)
    const std::vector<int> wd(w), od(o);
    StopRules r = { rr_dt, frac_dt, wd.data(), (int)wd.size(), cof != 0, false };
    r.out_dts = od.data(); r.n_out = (int)od.size();
    for (int tstep0 = 0; tstep0 <= 10; tstep0++) for (int nsteps = 0; nsteps <= 11; nsteps++) {
      std::vector<Run> got;
      for (int done = 0; done < nsteps;) {
        const Segment g = next_segment(r, tstep0 + done, nsteps - done);
        if (g.len < 1 || done + g.len > nsteps) { printf("bad length %d at %d of %d\n", g.len, tstep0 + done, nsteps); return 1; }
        const int last = tstep0 + done + g.len - 1;
        if (g.fstep != is_fracture_step(frac_dt, last) || g.weld_set != weld_set_at(r, last)) { printf("last step %d described wrongly\n", last); return 1; }
        got.push_back({ tstep0 + done, last, g.rr_step });
        done += g.len; cuts++;
      }
      if (!(got == walk(r, tstep0, nsteps))) {
        printf("rr_dt %d frac_dt %d cut_on_fracture %d welds %zu outs %zu tstep0 %d nsteps %d: cut differs from the walk\n", rr_dt, frac_dt, cof, wd.size(), od.size(), tstep0, nsteps);
        return 1;
      }
      if (next_segment(r, tstep0, 0).len != 0) { printf("an empty batch has a segment\n"); return 1; }
      batches++;
    }
  }
  printf("%lld batches, %lld segments: every cut is the walk's\n", batches, cuts);
  return 0;
}

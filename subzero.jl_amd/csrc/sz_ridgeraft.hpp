// sz_ridgeraft.hpp — the ridge / raft candidate table (timestep_ridging_rafting!, ridge_raft.jl:676-837) on the list WITH its ghosts, as the
// reference calls it between timestep_collisions! and the ghost removal (simulation.jl:121-136).  The ridging and rafting themselves
// (remove_floe_overlap!, add_floe_volume!, replace_floe!, the pieces, sim.rng) are serial, topology-changing host work and stay there; the device
// evaluates what tells whether the host has anything to do:
//   the per-floe draws   every row i draws once if height <= max_floe_ridge_height, then once if height <= max_floe_raft_height (:694-697), before
//                        anything else is looked at: with nothing to act on the whole call is exactly these draws -> n_draws, an integer sum
//   the gates            :698-753 and :757-831 with every draw assumed to pass: row i active with rows; a row naming j that passes valid_interaction
//                        as written there; 1e-6 < overlap / min_area < 0.95; heights that allow an action that changes state or draws (the kind bits)
// The table is a SUPERSET of what the reference acts on (the probabilities are left out, and so are the stale entries of its never-cleared
// interactions_list buffer); only true duplicates go: one entry per (i, j), from the first passing row.  An empty table means the call changes no
// floe and draws exactly n_draws numbers.
//   sz_k_rr_count   per list row the number of its entries, and the draws (per-wavefront sums added as integers: no order to depend on)
//   sz_k_rr_scan    ONE workgroup: exclusive offsets of the counts, the total
//   sz_k_rr_write   the entries at their offsets: ascending i, then first-passing-row order -- columns i, j (the reference's numbering of rows:
//                   partner index, -1..-4, -(4 + k)), kind, frac.  No atomic decides a position: the same table on every run
//   sz_k_rr_mark,   sz_ridgeraft_rows: the rows of the table's entries with their root parents and those parents' ghosts, flagged,
//   sz_k_rr_compact then compacted into ascending list rows (at the end of this file)
// The gates are stated once, in rr_row, which takes a policy for how a list names its rows: RrSingle here, RrTiled in sz_ridgeraft_tile.hpp.
// A dependent-load chain over the rows of floe.interactions (ROWCAP rows of 7 doubles per floe), one thread per list row.  fp64 in every precision mode.
#pragma once
#include "sz_kernels.hpp"

namespace sz {

constexpr int RR_TPB = 1024;          // the single-workgroup scan
constexpr int RR_CAP0 = 32;           // entries the table holds at first (it grows to what a pass counted, and the pass runs again)
enum { RR_RIDGE = 1, RR_RAFT = 2 };   // kind bits

struct RrDev { unsigned long long draws; int total, pad; };

struct RrArgs {
  RrDev* d;
  int *cnt, *off;                     // per list row: entries, exclusive offsets
  int *ti, *tj, *tk; double* tf;      // the table
  int m, cap;                         // list rows (parents and ghosts), capacity of the table
  double min_ridge_h, max_floe_ridge_h, max_domain_ridge_h, max_floe_raft_h, max_domain_raft_h;
};

// How a list names its rows.  The single context: a row's number is its position, the partner column of floe.interactions holds position + 1, and
// every row is evaluated.  The tiled policy (sz_ridgeraft_tile.hpp) names rows by their order keys instead.  A policy gives:
//   J                     the type of a partner number as the rows hold it (and as emit() is handed it)
//   evaluated(S, i)       does this context evaluate list row i at all?
//   partner(S, A, i, j)   the local row the positive partner number j names, or -1 (a row that names no list row: the reference would throw)
//   before(S, i, p)       the reference's i < j gate for local rows i and p
//   active(S, i)          is local row i `active` behind this step's timestep_collisions!?
struct RrSingle {
  using J = int;
  __device__ __forceinline__ bool evaluated(const State&, int) const { return true; }
  __device__ __forceinline__ int partner(const State&, const RrArgs& A, int, int j) const { return j > A.m ? -1 : j - 1; }
  __device__ __forceinline__ bool before(const State&, int i, int p) const { return i < p; }
  __device__ __forceinline__ bool active(const State& S, int i) const { return S.status[i] == SZ_ACTIVE; }
};

// The entries of list row i, in row order, handed to emit(j, kind, frac); returns the row's draws (0 for a row this context does not evaluate).
template <class Pol, class Emit>
__device__ __forceinline__ int rr_row(const State& S, const RrArgs& A, const Pol& pol, int i, Emit&& emit) {
  using J = typename Pol::J;
  if (!pol.evaluated(S, i)) return 0;
  const double hi = S.height[i];
  const bool ridge = hi <= A.max_floe_ridge_h, raft = hi <= A.max_floe_raft_h;
  const int nrows = min(S.inter_cnt[i], S.rowcap);
  if ((ridge || raft) && pol.active(S, i) && nrows > 0) {
    const double* rows = S.inter_rows + (size_t)i * S.rowcap * 7;
    const double xi = S.cx[i], yi = S.cy[i], ri = S.rmax[i], ai = S.area[i];
    for (int r = 0; r < nrows; r++) {
      const J j = (J)rows[(size_t)r * 7];
      double min_area = ai, hj = 0.0;
      bool valid = false;
      if (j > 0) {
        const int p = pol.partner(S, A, i, j);
        if (p < 0) continue;
        min_area = fmin(ai, S.area[p]);
        if (pol.before(S, i, p) && pol.active(S, p)) {
          // potential_interaction (collisions.jl:705-710), the collision search's expression
          const double ddx = xi - S.cx[p], ddy = yi - S.cy[p], rr = ri + S.rmax[p];
          valid = (ddx * ddx + ddy * ddy) < rr * rr;
          hj = S.height[p];
        }
      }
      else if (j == -1) valid = fabs(yi - S.eval[SZ_NORTH]) < ri;
      else if (j == -2) valid = fabs(yi - S.eval[SZ_SOUTH]) < ri;
      else if (j == -3) valid = fabs(xi - S.eval[SZ_EAST]) < ri;
      else if (j == -4) valid = fabs(xi - S.eval[SZ_WEST]) < ri;
      else if (j < 0) {
        const int e = (int)(-j - 1);    // topography element k = -(j + 4), 1-based, behind the four boundaries
        if (e >= S.nelem) continue;
        const double ddx = xi - S.ecx[e], ddy = yi - S.ecy[e], rr = ri + S.ermax[e];
        valid = (ddx * ddx + ddy * ddy) < rr * rr;
      }
      if (!valid) continue;
      const double frac = rows[(size_t)r * 7 + 6] / min_area;
      if (!(1e-6 < frac && frac < 0.95)) continue;
      int kind = 0;
      if (j > 0) {
        if (ridge && hj <= A.max_floe_ridge_h && (hi >= A.min_ridge_h || hj >= A.min_ridge_h)) kind |= RR_RIDGE;
        if (raft && hj <= A.max_floe_raft_h) kind |= RR_RAFT;
      } else {
        if (ridge && hi <= A.max_domain_ridge_h) kind |= RR_RIDGE;
        if (raft && hi <= A.max_domain_raft_h) kind |= RR_RAFT;
      }
      if (!kind) continue;
      // one entry per (i, j): an earlier row for the same j passes or fails on its own overlap alone (everything else is the pair's)
      bool dup = false;
      for (int q = 0; q < r && !dup; q++) {
        if ((J)rows[(size_t)q * 7] != j) continue;
        const double fq = rows[(size_t)q * 7 + 6] / min_area;
        dup = 1e-6 < fq && fq < 0.95;
      }
      if (!dup) emit(j, kind, frac);
    }
  }
  return (ridge ? 1 : 0) + (raft ? 1 : 0);
}

__global__ void __launch_bounds__(256) sz_k_rr_count(State S, RrArgs A) {
  unsigned long long draws = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += gridDim.x * blockDim.x) {
    int n = 0;
    draws += (unsigned long long)rr_row(S, A, RrSingle{}, i, [&](int, int, double) { n++; });
    A.cnt[i] = n;
  }
  for (int d = 32; d >= 1; d >>= 1) draws += __shfl_xor(draws, d);
  if ((threadIdx.x & 63) == 0 && draws) atomicAdd(&A.d->draws, draws);
}

// thread t takes the contiguous chunk t of the rows
__global__ void __launch_bounds__(RR_TPB) sz_k_rr_scan(RrArgs A) {
  __shared__ int part[RR_TPB];
  const int t = threadIdx.x, chunk = (A.m + RR_TPB - 1) / RR_TPB;
  const int p0 = min(A.m, t * chunk), p1 = min(A.m, p0 + chunk);
  int s = 0;
  for (int p = p0; p < p1; p++) s += A.cnt[p];
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < RR_TPB; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = part[t] - s;
  for (int p = p0; p < p1; p++) { A.off[p] = base; base += A.cnt[p]; }
  if (t == RR_TPB - 1) A.d->total = part[t];
}

__global__ void __launch_bounds__(256) sz_k_rr_write(State S, RrArgs A) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += gridDim.x * blockDim.x) {
    if (A.cnt[i] == 0) continue;
    int o = A.off[i];
    rr_row(S, A, RrSingle{}, i, [&](int j, int kind, double frac) {
      if (o >= 0 && o < A.cap) { A.ti[o] = i; A.tj[o] = j; A.tk[o] = kind; A.tf[o] = frac; }
      o++;
    });
  }
}

// ---- sz_ridgeraft_rows: the list rows the host's ridging and rafting can touch, from the table above.  An entry (i, j) names row
// i and, where j > 0, row j - 1; each of them stands for its family -- the root parent (the row < n that its parent link leads to: the row the
// reference's findfirst over floes.id finds) and every ghost on that parent's list.
//   sz_k_rr_mark      one thread per entry: flag 1 onto the two rows and their families.  Every writer writes the same value: no atomic, no order
//   (the engine's scan of the flags)
//   sz_k_rr_compact   flagged row r -> out[off[r]]: ascending list rows, each once
__device__ __forceinline__ void rr_mark_family(const State& S, int r, int m, int n, int* flag) {
  if (r < 0 || r >= m) return;
  flag[r] = 1;
  int p = r;
  for (int hop = 0; hop < MAX_GHOSTS && p >= n && p < m; hop++) p = S.parent[p];
  if (p < 0 || p >= n) return;
  flag[p] = 1;
  const int ng = min(S.ngh[p] & 0xff, MAX_GHOSTS);
  for (int k = 0; k < ng; k++) { const int g = S.gh[p * MAX_GHOSTS + k]; if (g >= 0 && g < m) flag[g] = 1; }
}
// ti / tj: nt entries of the table; m list rows of which the first n are parents; flag: m entries, zeroed
__global__ void __launch_bounds__(256) sz_k_rr_mark(State S, const int* ti, const int* tj, int nt, int m, int n, int* flag) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < nt; e += gridDim.x * blockDim.x) {
    rr_mark_family(S, ti[e], m, n, flag);
    const int j = tj[e];
    if (j > 0) rr_mark_family(S, j - 1, m, n, flag);
  }
}
__global__ void __launch_bounds__(256) sz_k_rr_compact(const int* flag, const int* off, int m, int* out) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < m; r += gridDim.x * blockDim.x)
    if (flag[r]) { const int o = off[r]; if (o >= 0 && o < m) out[o] = r; }
}

}  // namespace sz

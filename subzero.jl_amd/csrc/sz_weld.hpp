// sz_weld.hpp — the welding overlap table (timestep_welding!, welding.jl:91-182) on the resident parents: every pair the reference's loop would
// clip, in the order it visits them, with its intersection area.  The welding itself (weld_prob > rand(rng), the union-area window, the sort by
// area, fuse_two_floes!: polygon union, replace_floe!, momentum) is serial, topology-changing host work and stays there; what the loop asks of
// the geometry is only inter_area of pairs whose floes are still as they were when the call began, so the table of the state at
// the start of the call serves the whole call.  An empty table means the call would change nothing and draw no random number.
//   sz_k_weld_oob    the smallest parent index whose centroid fails in_bounds: bin_floe_centroids (:23-55) BREAKS there (:38), the floes
//                    behind it are in no bin.  One atomic per wavefront that found one.
//   sz_k_weld_bins   per parent the bin number k = (yidx - 1) Nx + (xidx - 1) (eachindex of the Nx x Ny matrix, column-major) or -1, and the
//                    parents that can weld at all (in a bin, active, area < max_weld_area) into the pass's own search cells
//   sz_k_weld_pairs  per such parent i the j > i of the same bin with potential_interaction (:128-131; strict <, no periodic images: the ghosts
//                    are gone by then, simulation.jl:138-144) -> keys (k, i, j)
//   (radix sort)     keys ascending = the reference's visiting order: bins by eachindex, i and j in ascending list order
//   sz_k_weld_area   one lane group per pair on LDS-staged rings: sum of GO.area over ALL regions of intersect_polys (:134), in region order;
//                    a pair the small working set cannot hold is handed on to the large instantiation (second launch, device-side list)
//   sz_k_weld_table  ONE workgroup: the entries with inter_area > 0, compacted in key order -> columns i, j, inter_area and the count
// Every hand-off between workgroups is a kernel boundary.  fp64 throughout, in every precision mode (predicates stay fp64).
#pragma once
#include "sz_kernels.hpp"

namespace sz {

constexpr int WELD_TPB = 1024;        // the single-workgroup compaction
constexpr int WELD_G0 = 16, WELD_CAP0 = 32, WELD_KC0 = 16, WELD_RC0 = 80, WELD_RM0 = 6;          // small working set: four pairs per wavefront
constexpr int WELD_G1 = 64, WELD_CAP1 = 255, WELD_KC1 = 64, WELD_RC1 = 640, WELD_RM1 = 16;       // large: the sizes of the largest narrow variant

struct WeldDev { int first_oob, npairs, ntable, nretry; };

struct WeldArgs {
  WeldDev* d;
  int* bin;                           // per parent: bin number or -1
  unsigned long long *keys_in, *keys; // pair keys (k * n + i) * n + j: as found / sorted
  double* area;                       // per sorted pair: inter_area
  int* retry;                         // sorted-pair positions handed on to the large instantiation
  int *ti, *tj; double* ta;           // the table
  int n, nx, ny, cap;                 // parents, bins, capacity of the pair arrays
  double max_area;
};

// ---- bins (bin_floe_centroids)
__global__ void __launch_bounds__(256) sz_k_weld_oob(State S, WeldArgs W) {
  const int per_x = S.ekind[2] == 1, per_y = S.ekind[0] == 1;          // in_bounds(xp, yp, grid, domain.north, domain.east)
  int first = W.n;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < W.n; i += gridDim.x * blockDim.x)
    if (!point_in_bounds(S, S.cx[i], S.cy[i], per_x, per_y)) first = min(first, i);
  for (int d = 32; d >= 1; d >>= 1) first = min(first, __shfl_xor(first, d));
  if ((threadIdx.x & 63) == 0 && first < W.n) atomicMin(&W.d->first_oob, first);
}

// grid_cell_index(p, Δ, g0) = floor((p - g0) / Δ) + 1, then the two clamps of :41-45 (1-based, as the reference has it).  A value outside 1..n can only
// be left where the reference itself would index out of bounds; it is folded into the range so that nothing here does.
__device__ __forceinline__ int weld_index(double p, double g0, double gf, double d, int n) {
  double f = floor((p - g0) / d) + 1.0;
  if (p <= g0) f = 1.0;
  if (p >= gf) f = (double)n;
  if (!(f >= 1.0)) f = 1.0;
  if (f > (double)n) f = (double)n;
  return (int)f;
}

__device__ __forceinline__ bool weld_eligible(const State& S, const WeldArgs& W, int i) {
  return W.bin[i] >= 0 && S.status[i] == SZ_ACTIVE && S.area[i] < W.max_area;
}

// T: the State with the pass's own cell arrays and grid geometry in place of the collision search's
__global__ void __launch_bounds__(256) sz_k_weld_bins(State T, WeldArgs W) {
  const int first = W.d->first_oob;
  const double dx = (T.gxf - T.gx0) / (double)W.nx, dy = (T.gyf - T.gy0) / (double)W.ny;
  const GridGeo g = grid_geo(T);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < W.n; i += gridDim.x * blockDim.x) {
    const double x = T.cx[i], y = T.cy[i];
    int k = -1;
    if (i < first) k = (weld_index(y, T.gy0, T.gyf, dy, W.ny) - 1) * W.nx + (weld_index(x, T.gx0, T.gxf, dx, W.nx) - 1);
    W.bin[i] = k;
    if (k >= 0 && T.status[i] == SZ_ACTIVE && T.area[i] < W.max_area) cell_insert(T, g, i, x, y);
  }
}

// ---- pairs.  Whole wavefronts go round together: one atomic per wavefront reserves the keys of its 64 floes.
__global__ void __launch_bounds__(256) sz_k_weld_pairs(State T, WeldArgs W) {
  const GridGeo g = grid_geo(T);
  const int lane = threadIdx.x & 63;
  constexpr int LOCAL = 24;
  for (int i0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63; i0 < W.n; i0 += gridDim.x * blockDim.x) {
    const int i = i0 + lane;
    const bool act = i < W.n && weld_eligible(T, W, i);
    int found[LOCAL]; int n = 0;
    double xi = 0, yi = 0, ri = 0; int ki = -1, cix = 0, ciy = 0;
    if (act) { xi = T.cx[i]; yi = T.cy[i]; ri = T.rmax[i]; ki = W.bin[i]; cell_of(g, xi, yi, cix, ciy); }
    // two rounds: count (and keep the first LOCAL partners), reserve, then write -- a floe with more partners than LOCAL walks its cells again
    auto walk = [&](auto&& hit) {
      for (int iy = max(ciy - 1, 0); iy <= min(ciy + 1, g.ncy - 1); iy++)
        for (int ix = max(cix - 1, 0); ix <= min(cix + 1, g.ncx - 1); ix++) {
          const int c = iy * g.ncx + ix;
          const int cnt = min(T.cell_cnt[c], CELL_K);
          auto test = [&](int j) {
            if (j <= i || W.bin[j] != ki) return;
            // potential_interaction (collisions.jl:705-710): the expression of the collision search, parents as they lie
            const double ddx = xi - T.cx[j], ddy = yi - T.cy[j], rr = ri + T.rmax[j];
            if ((ddx * ddx + ddy * ddy) < rr * rr) hit(j);
          };
          for (int s = 0; s < cnt; s++) test(T.cell_slots[(size_t)c * CELL_K + s]);
          if (T.cell_cnt[c] > CELL_K) for (int j = T.cell_ovf[c] - 1; j >= 0; j = T.cell_items[j]) test(j);
        }
    };
    if (act) walk([&](int j) { if (n < LOCAL) found[n] = j; n++; });
    int inc = n;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    const int tot = __shfl(inc, 63);
    int base = 0;
    if (lane == 0 && tot) base = atomicAdd(&W.d->npairs, tot);
    base = __shfl(base, 0);
    if (n == 0 || base + inc > W.cap) continue;          // (over capacity: the host sees npairs > cap, grows the arrays and runs the pass again)
    unsigned long long* out = W.keys_in + (base + inc - n);
    const unsigned long long hi = ((unsigned long long)ki * (unsigned long long)W.n + (unsigned long long)i) * (unsigned long long)W.n;
    if (n <= LOCAL) { for (int q = 0; q < n; q++) out[q] = hi + (unsigned long long)found[q]; }
    else { int q = 0; walk([&](int j) { if (q < n) out[q] = hi + (unsigned long long)j; q++; }); }
  }
}

// ---- areas
// Where the two rings of a pair come from is the ring source's business (RS): the kernel asks it for both rings of a key and stages, clips and sums
// whatever it is given.  A ring the source cannot produce is reported with more points than any working set holds, so it ends in the capacity error
// like a ring that is too long.
struct WeldRing { const double2* p; int n, osign; Box box; };
// the single context: both floes are rows of the state, the key is in row numbers
struct WeldRowRings {
  static __device__ __forceinline__ WeldRing row(const State& S, int i) {
    const int o = S.voff[i];
    return { S.vxy + o, S.voff[i + 1] - o, (int)S.osign[i], Box{ S.bbx0[i], S.bbx1[i], S.bby0[i], S.bby1[i] } };
  }
  __device__ __forceinline__ void pair(const State& S, const WeldArgs& W, unsigned long long key, WeldRing& a, WeldRing& b) const {
    const unsigned long long n64 = (unsigned long long)W.n;
    a = row(S, (int)((key / n64) % n64)); b = row(S, (int)(key % n64));
  }
};

template <int G, int CAP, int KC, int RC, int RM, int LARGE, class RS = WeldRowRings>
__global__ void __launch_bounds__(64) sz_k_weld_area(State S, WeldArgs W, int npairs, RS rings) {
  constexpr int GPB = 64 / G;
  using Mem = GroupMem<CAP, KC, RC, RM>;
  __shared__ Mem mem[GPB];
  const int gl = threadIdx.x % G, gi = threadIdx.x / G;
  Mem& m = mem[gi];
  if (gl == 0) { m.err = 0; m.ntracefail = 0; }
  Stamps st; STAMP_INIT(st);
  int bad = 0;
  const int nitem = LARGE ? W.d->nretry : npairs;
  for (int q0 = blockIdx.x * GPB; q0 < nitem; q0 += gridDim.x * GPB) {
    const int q = q0 + gi;
    if (q >= nitem) continue;
    const int t = LARGE ? W.retry[q] : q;
    WeldRing ra, rb;
    rings.pair(S, W, W.keys[t], ra, rb);
    const int na = ra.n, nb = rb.n;
    gsync();
    bool fits = na <= CAP && nb <= CAP;
    double a = 0.0;
    if (fits) {
      for (int k = gl; k < na; k += G) { const double2 p = ra.p[k]; m.ax[k] = p.x; m.ay[k] = p.y; }
      for (int k = gl; k < nb; k += G) { const double2 p = rb.p[k]; m.bx[k] = p.x; m.by[k] = p.y; }
      gsync();
      // buffer 0: a contained ring is measured where it lies (one floe inside the other: the smaller floe's area)
      clip<G>(m, gl, 0.0, 0.0, na, ra.osign, nb, rb.osign, 0, ra.box, rb.box, st);
      gsync();
      const int e = m.err;
      if (e & (ERR_CAP_XING | ERR_CAP_REGION)) {
        fits = false;
        gsync();
        if (gl == 0) m.err = 0;
        if (LARGE) bad |= e & (ERR_CAP_XING | ERR_CAP_REGION);
      } else {
        const int nreg = m.nreg[0];
        for (int r = 0; r < nreg; r++) a += m.rarea[0][r];          // region order: the same sum on every run
      }
    } else if (LARGE) bad |= ERR_CAP_RING;
    if (gl == 0) {
      W.area[t] = fits ? a : 0.0;
      if (!fits && !LARGE) W.retry[atomicAdd(&W.d->nretry, 1)] = t;
    }
  }
  gsync();
  if (gl == 0 && bad) atomicOr(&S.cnt[C_ERR], bad);          // no variant holds the pair: the sticky capacity error, nothing is dropped silently
  if (gl == 0 && m.ntracefail) atomicAdd(&S.cnt[C_TRACE_FAIL], (int)m.ntracefail);
}

// ---- table: ascending compaction of the entries with area > 0.  ONE workgroup of 16 wavefronts: wavefront w takes the contiguous chunk w of the
// sorted pairs, 64 at a time (coalesced), positions from ballots -- a fixed order,
// the same table on every run
__global__ void __launch_bounds__(WELD_TPB) sz_k_weld_table(WeldArgs W, int npairs) {
  constexpr int NW = WELD_TPB / 64;
  __shared__ int wc[NW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int chw = ((npairs + NW - 1) / NW + 63) & ~63;
  const int p0 = min(npairs, wave * chw), p1 = min(npairs, p0 + chw);
  int cnt = 0;
  for (int q = p0; q < p1; q += 64) {
    const int p = q + lane;
    cnt += __popcll(__ballot(p < p1 && W.area[p] > 0.0));
  }
  if (lane == 0) wc[wave] = cnt;
  __syncthreads();
  int base = 0, total = 0;
  for (int w = 0; w < NW; w++) { if (w < wave) base += wc[w]; total += wc[w]; }
  const unsigned long long n64 = (unsigned long long)W.n;
  for (int q = p0; q < p1; q += 64) {
    const int p = q + lane;
    const double a = p < p1 ? W.area[p] : 0.0;
    const bool f = a > 0.0;
    const unsigned long long mask = __ballot(f);
    if (f) {
      const int o = base + __popcll(mask & ((1ull << lane) - 1ull));
      const unsigned long long key = W.keys[p];
      W.ti[o] = (int)((key / n64) % n64); W.tj[o] = (int)(key % n64); W.ta[o] = a;
    }
    base += __popcll(mask);
  }
  if (threadIdx.x == 0) W.d->ntable = total;
}

}  // namespace sz

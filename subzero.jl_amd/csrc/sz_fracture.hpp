// sz_fracture.hpp — determine_fractures (fractures.jl:269-280) on the resident state: which parents the host's fracture_floes!
// would split.  The splitting itself (Voronoi pieces, deform_floe!, momentum, new ids) is topology-changing serial work and stays
// on the host; on most fracture steps nothing fractures and the step changes nothing, so resident batches
// evaluate only the predicate and end where it finds a candidate (sz_step, the same C_STOP word as the tag stop).
//   sz_k_frac_criterion  ONE workgroup: mean(floes.height) over the parents in a fixed order (the same sums on every run, whatever the
//                        grid), then -- Hibler -- the criterion polygon as _calculate_hibler (:83-94) builds it from that mean,
//                        update_criteria! (:234-251).  A fixed polygon (MohrsCone, :170-214) was uploaded by sz_set_fracture.
//   sz_k_frac_test       per parent: the principal stresses (eigvals of the symmetric stress_accum, find_σpoint :284-288) scaled by
//                        (area / min_floe_area)^α (_scale_principal_stress!, stress_calculators.jl:127-132), the covered-by test of that
//                        point against the polygon (inside or on the boundary = covered), the area cut.  A candidate raises the stop.
//   sz_k_frac_compact    ONE workgroup, on request only (sz_fracture_candidates): the candidates as ascending 0-based indices.
// The three are separate launches: every hand-off between workgroups is a kernel boundary.
#pragma once
#include "sz_kernels.hpp"

namespace sz {

constexpr int FRAC_MAXPTS = 128;   // points of a criterion polygon (the Hibler ring has 100)
constexpr int FRAC_HIBLER_PTS = 100;
constexpr int FRAC_TPB = 1024;     // the single-workgroup launches

// device block of the criterion: the unit table of the Hibler ring (cos / sin of the points of range(0, 2π, length = 100), last =
// first, made by the host), the polygon as the last evaluation built it, its mean height and the candidate count
struct FracDev {
  double ct[FRAC_MAXPTS], st[FRAC_MAXPTS];
  double px[FRAC_MAXPTS], py[FRAC_MAXPTS];
  double mean_h, p;
  int count, pad;
};

struct FracArgs {
  FracDev* d;
  unsigned char* flag;        // per parent: 1 = candidate (the last evaluation)
  int* idx;                   // compacted candidates
  int kind, npts, n;          // SZ_FRAC_HIBLER / SZ_FRAC_POLYGON, polygon points (closed ring), parents
  double pstar, c, alpha, min_area;
  double rc, rs;              // cos(π/4), sin(π/4) as sincos gives them (Rotations.Angle2d in _move_poly)
};

// mean height and (Hibler) the polygon.  step: the batch-relative step this evaluation ends (0: on request); launches of steps the
// batch has been stopped or paused before return at once, like the other kernels of such a step (stopped_late).
__global__ void __launch_bounds__(FRAC_TPB) sz_k_frac_criterion(State S, FracArgs F) {
  if (stopped_late(S)) return;
  __shared__ double sh[FRAC_TPB];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < F.n; i += FRAC_TPB) s += S.height[i];       // thread t: its strided floes in ascending order
  sh[t] = s;
  __syncthreads();
  for (int w = FRAC_TPB / 2; w > 0; w >>= 1) {                    // fixed pairwise tree: the same additions on every run
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  const double hbar = F.n > 0 ? sh[0] / (double)F.n : 0.0;
  if (t == 0) { F.d->mean_h = hbar; F.d->count = 0; }
  if (F.kind != 1) return;
  // _calculate_hibler: p = pstar h̄ exp(-c (1 - compactness)), compactness = 1; semi-axes a = p √2 / 2, b = a / 2; the ring
  // (a cos α, b sin α) rotated by π/4 about the origin and moved by (-p/2, -p/2) (_move_poly, floe_utils.jl:74-80)
  const double p = F.pstar * hbar * exp(-F.c * (1.0 - 1.0));
  const double a = p * sqrt(2.0) / 2.0, b = a / 2.0;
  if (t < FRAC_HIBLER_PTS) {
    const double x0 = a * F.d->ct[t], y0 = b * F.d->st[t];
    const double x1 = F.rc * x0 + (-F.rs) * y0, y1 = F.rs * x0 + F.rc * y0;
    F.d->px[t] = x1 + (-p / 2.0);
    F.d->py[t] = y1 + (-p / 2.0);
  }
  if (t == 0) F.d->p = p;
}

// covered-by (GO.coveredby): on an edge, or inside by the crossing rule, of the closed ring P[0..n-1] (P[n-1] == P[0])
__device__ __forceinline__ bool frac_covered(const double* qx, const double* qy, int n, double x, double y) {
  bool in = false, on = false;
  for (int k = 0; k + 1 < n; k++) {
    const double x1 = qx[k], y1 = qy[k], x2 = qx[k + 1], y2 = qy[k + 1];
    const double cr = (x2 - x1) * (y - y1) - (y2 - y1) * (x - x1);
    if (cr == 0.0 && x >= fmin(x1, x2) && x <= fmax(x1, x2) && y >= fmin(y1, y2) && y <= fmax(y1, y2)) on = true;
    if ((y1 > y) != (y2 > y)) {
      const double xi = x1 + (y - y1) * (x2 - x1) / (y2 - y1);
      if (x < xi) in = !in;
    }
  }
  return in || on;
}

// the principal stresses of the symmetric [s11 s12; s12 s22], ascending (the order LAPACK returns them)
__device__ __forceinline__ void frac_eig(double s11, double s12, double s22, double& lo, double& hi) {
  const double m = 0.5 * (s11 + s22), h = 0.5 * (s11 - s22);
  const double r = sqrt(h * h + s12 * s12);
  lo = m - r; hi = m + r;
}

__global__ void __launch_bounds__(256) sz_k_frac_test(State S, FracArgs F) {
  if (stopped_late(S)) return;
  __shared__ double qx[FRAC_MAXPTS], qy[FRAC_MAXPTS];
  const int np = F.npts;
  for (int k = threadIdx.x; k < np; k += blockDim.x) { qx[k] = F.d->px[k]; qy[k] = F.d->py[k]; }
  __syncthreads();
  int found = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < F.n; i += gridDim.x * blockDim.x) {
    const double4 sa = *(const double4*)(S.sa + (size_t)i * 4);       // 11, 12, 21, 22
    const double area = S.area[i];
    double lo, hi;
    frac_eig(sa.x, 0.5 * (sa.y + sa.z), sa.w, lo, hi);
    if (F.alpha != 0.0) { const double m = pow(area / F.min_area, F.alpha); lo *= m; hi *= m; }
    const bool cand = !(area < F.min_area) && !frac_covered(qx, qy, np, lo, hi);
    F.flag[i] = cand ? 1 : 0;
    found += cand ? 1 : 0;
  }
  if (__ballot(found > 0) != 0ull && (threadIdx.x & 63) == 0) {
    atomicAdd(&F.d->count, 1);      // waves with a candidate: "> 0" is what a batch needs; sz_k_frac_compact writes the exact count
    request_stop(S);                // the batch ends after this step: fracture_floes! (host) has work
  }
}

// ascending compaction of the flags: thread t takes the contiguous chunk t, chunks in order
__global__ void __launch_bounds__(FRAC_TPB) sz_k_frac_compact(FracArgs F) {
  __shared__ int sc[FRAC_TPB];
  const int t = threadIdx.x;
  const int ch = (F.n + FRAC_TPB - 1) / FRAC_TPB;
  const int i0 = min(F.n, t * ch), i1 = min(F.n, i0 + ch);
  int cnt = 0;
  for (int i = i0; i < i1; i++) cnt += F.flag[i];
  sc[t] = cnt;
  __syncthreads();
  for (int w = 1; w < FRAC_TPB; w <<= 1) {           // inclusive scan (Hillis-Steele)
    const int v = t >= w ? sc[t - w] : 0;
    __syncthreads();
    sc[t] += v;
    __syncthreads();
  }
  int o = sc[t] - cnt;
  for (int i = i0; i < i1; i++) if (F.flag[i]) F.idx[o++] = i;
  if (t == FRAC_TPB - 1) F.d->count = sc[t];
}

// A fracture step inside a batch that stops on fracture is run as the last step of a batch (the integrator keeps its ghosts and makes
// none for a next step: sz_k_integrate, acc_mode bit 1) -- whether it IS the last is only known once sz_k_frac_test has run.  The batch
// goes on through these two launches, enqueued behind the test with S.step = the NEXT step, which return at once when the test (or a
// tag, or a pause) has stopped the batch: then the ghosts of the fracture step are where the rows assembled behind the batch need them.
// Otherwise they do what starting a new batch there would do -- drop the step's ghosts, make the next step's from the parents as they lie.
__global__ void sz_k_frac_resume_remove(State S) {
  if (stopped(S)) return;
  remove_ghosts(S, 0);
}
__global__ void __launch_bounds__(256) sz_k_frac_resume_seed(State S, int slot, int nh) {
  if (stopped(S)) return;
  ghost_inline_seed(S, slot, nh);
}

}  // namespace sz

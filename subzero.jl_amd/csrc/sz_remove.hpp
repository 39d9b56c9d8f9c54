// sz_remove.hpp — remove_floes! (simplification.jl:279-314) on the device, for the case in which simplify_floes! reduces to it: no floe
// tagged `fuse`, no ring over max_vertices.  The pass runs over the parents with no ghosts in the list:
//     sz_k_rm_flags     per parent, in the reference's branch order: dissolve (tag != remove and under the minimum area / height), remove
//                       (tag == remove), keep; the two kinds counted with one ballot per wavefront; what would decline the pass counted too
//     scans             keep flags -> new row numbers; ring / sub-floe points of the kept rows -> their new CSR offsets; dissolve flags ->
//                       positions on the compacted list of dissolving rows
//     sz_k_rm_rows      new row -> old row, the new offsets per new row, the dissolving rows onto their list
//     sz_k_rm_dissolve  one thread walks that list in DESCENDING row order (the reference loops reverse(eachindex(floes))): two floes that
//                       dissolve into one cell sum in the reference's order, to the bit.  It decides whether the pass is declined, and only
//                       a pass that is not declined touches the lattice
// then the host reads the verdict, and the rows move through temporaries with the migration's kernels (sz_migrate.hpp: sz_k_mig_gather,
// sz_k_mig_points, sz_k_mig_scatter -- a row's source lies at or behind it, but an in-place parallel shift races) and the two below for what
// a migration does not carry: the interaction rows and the `origin` column.  Every hand-off between workgroups is a kernel boundary.
#pragma once
#include "sz_migrate.hpp"

namespace sz {

enum { RM_DECL_FUSE = 1, RM_DECL_VERTS = 2, RM_DECL_EMPTY = 4, RM_DECL_INDEX = 8, RM_NO_LATTICE = 16 };

struct RmDev {
  int n_removed, n_dissolved, n_fuse, n_over;      // sz_k_rm_flags
  int Nn, Vn, NSn;                                 // sz_k_rm_rows: parents, ring points and sub-floe points that stay
  int declined;                                    // sz_k_rm_dissolve: RM_DECL_* bits (0: the pass goes ahead)
  int max_ring, max_sub;                           // sz_k_rm_flags: most ring / sub-floe points of a floe that stays (what an upload would find)
};

struct RmArgs {
  int n;                                           // parents
  int max_vertices; double min_area, min_height;
  int *keep, *dis, *kv, *ks;                       // per old row: stays, dissolves, its ring / sub-floe points if it stays
  int *newrow, *dpos, *ovoff, *osoff;              // their exclusive scans (n + 1 entries)
  int *src, *nvoff, *nsoff, *dlist;                // per new row: old row, new CSR offsets; the dissolving rows, ascending
  RmDev* d;
  // dissolve_floe! (simplification.jl:18-32): the grid of sz_set_fields, the running ocean.dissolved lattice, periodic east / north
  double x0, y0, dx, dy; int Nx, Ny, per_e, per_n; double* dissolved;
};

__global__ void __launch_bounds__(256) sz_k_rm_flags(State S, RmArgs A) {
  const int lane = threadIdx.x & 63;
  for (int i0 = blockIdx.x * blockDim.x; i0 < A.n; i0 += gridDim.x * blockDim.x) {
    const int i = i0 + threadIdx.x;
    bool rem = false, dis = false, fuse = false, over = false;
    int kring = 0, ksub = 0;
    if (i < A.n) {
      const int st = S.status[i], nv = S.voff[i + 1] - S.voff[i], ns = S.soff[i + 1] - S.soff[i];
      dis = st != SZ_REMOVE && (S.area[i] < A.min_area || S.height[i] < A.min_height);
      rem = !dis && st == SZ_REMOVE;
      fuse = st == SZ_FUSE; over = nv > A.max_vertices;
      const int keep = !dis && !rem;
      A.keep[i] = keep; A.dis[i] = dis;
      kring = keep ? nv : 0; ksub = keep ? ns : 0;
      A.kv[i] = kring; A.ks[i] = ksub;
    }
    for (int d = 32; d >= 1; d >>= 1) { kring = max(kring, __shfl_xor(kring, d)); ksub = max(ksub, __shfl_xor(ksub, d)); }
    const unsigned long long br = __ballot(rem), bd = __ballot(dis), bf = __ballot(fuse), bo = __ballot(over);
    if (lane == 0) {          // (counts: the order of the additions does not matter)
      if (br) atomicAdd(&A.d->n_removed, __popcll(br));
      if (bd) atomicAdd(&A.d->n_dissolved, __popcll(bd));
      if (bf) atomicAdd(&A.d->n_fuse, __popcll(bf));
      if (bo) atomicAdd(&A.d->n_over, __popcll(bo));
      if (kring) atomicMax(&A.d->max_ring, kring);
      if (ksub) atomicMax(&A.d->max_sub, ksub);
    }
  }
}

__global__ void __launch_bounds__(256) sz_k_rm_rows(RmArgs A) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += gridDim.x * blockDim.x) {
    if (A.keep[i]) { const int r = A.newrow[i]; A.src[r] = i; A.nvoff[r] = A.ovoff[i]; A.nsoff[r] = A.osoff[i]; }
    if (A.dis[i]) A.dlist[A.dpos[i]] = i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int Nn = A.newrow[A.n];
    A.nvoff[Nn] = A.ovoff[A.n]; A.nsoff[Nn] = A.osoff[A.n];
    A.d->Nn = Nn; A.d->Vn = A.ovoff[A.n]; A.d->NSn = A.osoff[A.n];
  }
}

// find_grid_cell_index (coupling.jl:440-444) and shift_cell_idx (:1154-1178) of one coordinate: the 1-based cell, or 0 for "outside" where
// the value does not fit an index
__device__ __forceinline__ long long rm_cell_idx(double p, double p0, double d, int ncells, int periodic) {
  const double f = floor((p - p0) / d) + 1.0;
  if (!(f > -1e15 && f < 1e15)) return 0;
  long long idx = (long long)f;
  if (periodic) idx = idx < 1 ? idx + ncells : ncells < idx ? idx - ncells : idx;
  return idx;
}

// The reference writes dissolved[yidx, xidx] into its (Nx + 1) x (Ny + 1) matrix: in the lattice layout (element [ix][iy] at ix (Ny + 1) + iy)
// that is element [yidx - 1][xidx - 1].  The quirk is kept; where it leaves the matrix (a BoundsError there, non-square grids only) the pass
// is declined.  The element a floe at (cx, cy) dissolves into: 1 and *elem, 0 = outside the grid (nothing is added), -1 = outside the matrix
__device__ __forceinline__ int rm_dissolve_elem(double cx, double cy, const RmArgs& A, size_t* elem) {
  const long long xidx = rm_cell_idx(cx, A.x0, A.dx, A.Nx, A.per_e), yidx = rm_cell_idx(cy, A.y0, A.dy, A.Ny, A.per_n);
  if (!(0 < xidx && xidx <= A.Nx && 0 < yidx && yidx <= A.Ny)) return 0;
  if (yidx > A.Nx + 1 || xidx > A.Ny + 1) return -1;
  *elem = (size_t)(yidx - 1) * (A.Ny + 1) + (size_t)(xidx - 1);
  return 1;
}
// The walk over nd dissolving floes in DESCENDING order, in two parts: RM_WALK_CHECK -- is any index outside the matrix -- and RM_WALK_SUM -- the
// sums; a part runs only while nothing has declined.  at(k, &cx, &cy, &mass) gives floe k of the ascending list (false: not a dissolving one).
// Returns decl with RM_DECL_INDEX / RM_NO_LATTICE added; only the sums touch the lattice.
enum { RM_WALK_CHECK = 1, RM_WALK_SUM = 2 };
template <typename At>
__device__ __forceinline__ int rm_dissolve_walk(const RmArgs& A, int decl, int nd, int any_dissolves, int parts, At at) {
  if (!decl && any_dissolves && !A.dissolved) decl = RM_NO_LATTICE;
  for (int pass = 0; pass < 2 && !decl; pass++) {
    if (!(parts >> pass & 1)) continue;
    for (int k = nd - 1; k >= 0; k--) {
      double cx, cy, mass; size_t e = 0;
      if (!at(k, &cx, &cy, &mass)) continue;
      const int in = rm_dissolve_elem(cx, cy, A, &e);
      if (in == 0) continue;
      if (pass == 0) { if (in < 0) { decl = RM_DECL_INDEX; break; } }
      else if (in > 0) A.dissolved[e] += mass;
    }
  }
  return decl;
}
__global__ void sz_k_rm_dissolve(State S, RmArgs A) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  RmDev* R = A.d;
  const int decl = (R->n_fuse ? RM_DECL_FUSE : 0) | (R->n_over ? RM_DECL_VERTS : 0) | (R->Nn == 0 ? RM_DECL_EMPTY : 0);
  const int nd = R->n_dissolved;
  R->declined = rm_dissolve_walk(A, decl, nd, nd > 0, RM_WALK_CHECK | RM_WALK_SUM, [&](int k, double* cx, double* cy, double* mass) {
    const int i = A.dlist[k];
    *cx = S.cx[i]; *cy = S.cy[i]; *mass = S.mass[i];
    return true;
  });
}

// what a migration does not carry, one wavefront per new row: the interaction rows (count and the rows in use, partner numbers as they
// are) and the row the floe had at the last upload, into temporaries ...
__global__ void __launch_bounds__(256) sz_k_rm_gather_rows(State S, int Nn, const int* src, const int* origin, int* t_origin, int* t_cnt, double* t_rows) {
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const size_t stride = (size_t)S.rowcap * 7;
  for (int r = wave; r < Nn; r += nw) {
    const int s = src[r];
    const int cnt = S.inter_cnt[s], n = min(max(cnt, 0), S.rowcap) * 7;
    if (lane == 0) { t_origin[r] = origin[s]; t_cnt[r] = cnt; }
    const double* from = S.inter_rows + stride * s;
    double* to = t_rows + stride * r;
    for (int k = lane; k < n; k += 64) to[k] = from[k];
  }
}
// ... and back; the surviving statuses are `active` (simplification.jl:308-311)
__global__ void __launch_bounds__(256) sz_k_rm_scatter_rows(State S, int Nn, int* origin, const int* t_origin, const int* t_cnt, const double* t_rows) {
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const size_t stride = (size_t)S.rowcap * 7;
  for (int r = wave; r < Nn; r += nw) {
    const int cnt = t_cnt[r], n = min(max(cnt, 0), S.rowcap) * 7;
    if (lane == 0) { origin[r] = t_origin[r]; S.inter_cnt[r] = cnt; S.status[r] = SZ_ACTIVE; S.tagA[r] = SZ_ACTIVE; }
    const double* from = t_rows + stride * r;
    double* to = S.inter_rows + stride * r;
    for (int k = lane; k < n; k += 64) to[k] = from[k];
  }
}

}  // namespace sz

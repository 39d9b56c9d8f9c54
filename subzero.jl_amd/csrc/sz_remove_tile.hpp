// sz_remove_tile.hpp — the part of remove_floes! (sz_remove.hpp) that a tiled context adds: the rows of the ONE global floe list live on several
// ranks, and every rank must end with what the single context's pass leaves, restricted to the floes it owns ("tiled contexts").
// Flags, scans and the row move are the single context's.  Between them:
//     sz_k_rmt_pack      the floes that leave this rank, in row order (= ascending global number), as records {old global number, kind, cx, cy,
//                        mass}.  The records of all ranks are all-gathered, every rank the same number of slots
//     sz_k_rmt_merge     the gathered lists -- each ascending -- into one list ordered by global number: a record's place is its place in its
//                        own list plus, per other rank, the records there with a smaller number (binary search).  Every rank builds the same list
//     sz_k_rmt_renumber  a kept row's new global number: its old one minus the leaving floes with a smaller one (binary search in the merged list)
//     sz_k_rmt_walk      one thread walks the merged list in DESCENDING global number -- the order of the reference's loop over the undivided
//                        list -- with the arithmetic of sz_k_rm_dissolve: every rank holds the same replica of ocean.dissolved, bit for bit.
//                        Two launches: the check before the ranks agree on the verdict, the sums behind the agreement
// Every hand-off between workgroups is a kernel boundary.
#pragma once
#include "sz_remove.hpp"

namespace sz {

constexpr int RMT_REC = 5;          // doubles per leaving record: old global number, kind (1: dissolves, 0: removed), cx, cy, mass

// old row i leaves: record i - newrow[i] (newrow: the exclusive scan of the keep flags = the kept rows before i)
__global__ void __launch_bounds__(256) sz_k_rmt_pack(State S, RmArgs A, double* rec) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += gridDim.x * blockDim.x) {
    if (A.keep[i]) continue;
    double* r = rec + (size_t)RMT_REC * (i - A.newrow[i]);
    r[0] = (double)S.okey[i]; r[1] = A.dis[i] ? 1.0 : 0.0; r[2] = S.cx[i]; r[3] = S.cy[i]; r[4] = S.mass[i];
  }
}

// records of `list` (cnt of them, ascending) with a global number below g
__device__ __forceinline__ int rmt_below(const double* list, int cnt, double g) {
  int lo = 0, hi = cnt;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (list[(size_t)RMT_REC * mid] < g) lo = mid + 1; else hi = mid; }
  return lo;
}

// all: nranks lists at a stride of `slots` records, cnt[r] in use; merged: the sum of cnt records, ascending
__global__ void __launch_bounds__(256) sz_k_rmt_merge(const double* all, const int* cnt, int nranks, int slots, double* merged, int total) {
  const long long n = (long long)nranks * slots;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(t / slots), k = (int)(t % slots);
    if (k >= cnt[r]) continue;
    const double* me = all + (size_t)RMT_REC * ((size_t)r * slots + k);
    int pos = k;
    for (int q = 0; q < nranks; q++) if (q != r) pos += rmt_below(all + (size_t)RMT_REC * (size_t)q * slots, cnt[q], me[0]);
    if (pos >= total) continue;          // (lists that are not what they should be: a global number twice)
    double* to = merged + (size_t)RMT_REC * pos;
    for (int j = 0; j < RMT_REC; j++) to[j] = me[j];
  }
}

// new row r (old row src[r]) -> its new global number
__global__ void __launch_bounds__(256) sz_k_rmt_renumber(State S, int Nn, const int* src, const double* merged, int total, long long* newkey) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < Nn; r += gridDim.x * blockDim.x) {
    const long long g = S.okey[src[r]];
    newkey[r] = g - rmt_below(merged, total, (double)g);
  }
}

// parts = RM_WALK_CHECK: the verdict of the walk into *declined (RM_DECL_INDEX, RM_NO_LATTICE or 0; what the counts decline, the host has decided
// before), the lattice untouched; parts = RM_WALK_SUM, behind the ranks' agreement on that verdict: the sums
__global__ void sz_k_rmt_walk(RmArgs A, const double* merged, int total, int n_dissolved, int parts, int* declined) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int decl = rm_dissolve_walk(A, 0, total, n_dissolved > 0, parts, [&](int k, double* cx, double* cy, double* mass) {
    const double* r = merged + (size_t)RMT_REC * k;
    *cx = r[2]; *cy = r[3]; *mass = r[4];
    return r[1] != 0.0;
  });
  if (parts & RM_WALK_CHECK) *declined = decl;
}

}  // namespace sz

// sz_fracture_tile.hpp — the part of determine_fractures (sz_fracture.hpp) that a tiled context adds: the Hibler polygon is built from
// mean(floes.height) over the ONE global floe list, whose rows live on several ranks, and sz_k_frac_criterion sums in a fixed order over that
// list (thread t of 1024: rows t, t + 1024, .. ascending, then a fixed tree).  Partial sums per rank, reduced over the ranks, add the same
// numbers in another order: other last bits of p, other verdicts for σ-points on the polygon's boundary.  So the heights come together in
// global order on every rank, and the single context's kernels run unchanged: the criterion over the gathered array, the test over the owned
// rows ("tiled contexts").
//     sz_k_fract_pack     {global number, height} of every owned row, in row order.  The records of all ranks are all-gathered, every rank the
//                         same number of slots
//     sz_k_fract_scatter  each gathered height to its global number in an array of length N_global (the sum of the owned counts); every slot
//                         written is marked.  A number out of range or a slot written twice raises a bit -- with N_global records for
//                         N_global slots that is also every way a slot can stay unwritten
// Every hand-off between workgroups is a kernel boundary.
#pragma once
#include "sz_fracture.hpp"

namespace sz {

constexpr int FRT_REC = 2;          // doubles per record: global number, height
constexpr int FRT_BAD_RANGE = 1, FRT_BAD_TWICE = 2;

__global__ void __launch_bounds__(256) sz_k_fract_pack(State S, int n, double* rec) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    rec[(size_t)FRT_REC * i] = (double)S.okey[i];
    rec[(size_t)FRT_REC * i + 1] = S.height[i];
  }
}

// all: nranks lists at a stride of `slots` records, cnt[r] in use; height / mark: total slots, mark zeroed by the caller
__global__ void __launch_bounds__(256) sz_k_fract_scatter(const double* all, const int* cnt, int nranks, int slots, double* height, int* mark, int total, int* bad) {
  const long long n = (long long)nranks * slots;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(t / slots), k = (int)(t % slots);
    if (k >= cnt[r]) continue;
    const double* me = all + (size_t)FRT_REC * ((size_t)r * slots + k);
    const double g = me[0];
    if (!(g >= 0.0 && g < (double)total) || g != (double)(long long)g) { atomicOr(bad, FRT_BAD_RANGE); continue; }
    const int to = (int)g;
    if (atomicAdd(&mark[to], 1) != 0) { atomicOr(bad, FRT_BAD_TWICE); continue; }
    height[to] = me[1];
  }
}

}  // namespace sz

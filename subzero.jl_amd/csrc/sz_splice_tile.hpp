// sz_splice_tile.hpp — the part of a row edit (sz_splice.hpp) that a tiled context adds: sz_tile_download_rows and sz_tile_splice_floes name rows by
// their number in the ONE global floe list, whose rows live on several ranks.  Every rank is given the whole edit and applies its
// share; the plan, the gathers and the scatters are the single context's.  In front of them:
//     sz_k_spt_find      sz_tile_download_rows: per requested name the local row (binary search in the owned order keys, S.okey[0 .. N), ascending by
//                        row) or -1 and a found flag; behind the engine's scan of the flags a second launch (pos != null) compacts the positions in
//                        the request and the local rows of the names found.  A request goes through in chunks the scan's block array covers
//     sz_k_spt_marks     sz_tile_splice_floes: per `del` / `rep` name the owned row it marks (or -1), and how many names of either kind were found --
//                        the counts the ranks gather before anything changes
//     sz_k_spt_renumber  a new row's global number: a kept or replaced row's old one minus the `del` names below it (binary search in the device copy
//                        of `del`, as sz_k_rmt_renumber searches the merged leaving list); an appended row's from N_global - n_del + k
// The searches need the order keys ascending by row: the host checks its copy (tile_gidx) before either call launches.
#pragma once
#include "sz_splice.hpp"

namespace sz {

// row of key g among keys[0 .. n), ascending, or -1
__device__ __forceinline__ int spt_row_of(const long long* keys, int n, long long g) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < g) lo = mid + 1; else hi = mid; }
  return lo < n && keys[lo] == g ? lo : -1;
}
// names of list[0 .. n), ascending, below g
__device__ __forceinline__ int spt_below(const long long* list, int n, long long g) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (list[mid] < g) lo = mid + 1; else hi = mid; }
  return lo;
}

// One chunk of a request: names[0 .. n) are its positions k0 .. k0 + n.  pos == null: loc[k] = the owned row of names[k] or -1, flag[k] = found.
// pos = the exclusive scan of flag: which[pos[k]] = k0 + k, rows[pos[k]] = loc[k] for the names found (ascending k: the order of the request);
// which / rows start where the chunks before this one ended
__global__ void __launch_bounds__(256) sz_k_spt_find(State S, int N, int n, int k0, const long long* names, int* loc, int* flag, const int* pos, int* which, int* rows) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    if (!pos) { const int r = spt_row_of(S.okey, N, names[k]); loc[k] = r; flag[k] = r >= 0; }
    else if (flag[k]) { which[pos[k]] = k0 + k; rows[pos[k]] = loc[k]; }
  }
}

// names: n_del `del` names, then n_rep `rep` names; found[0] / found[1]: the `del` / `rep` names this rank owns (zeroed by the caller)
__global__ void __launch_bounds__(256) sz_k_spt_marks(State S, int N, int n_del, int n_rep, const long long* names, int* loc, int* found) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_del + n_rep; t += gridDim.x * blockDim.x) {
    const int r = spt_row_of(S.okey, N, names[t]);
    loc[t] = r;
    if (r >= 0) atomicAdd(&found[t < n_del ? 0 : 1], 1);
  }
}

struct SptKeys {
  const long long* del; int n_del;    // the whole edit's `del` names (device), ascending
  const int* rep; int n_rep;          // this rank's replaced rows (device; staged row j < n_rep replaces old row rep[j])
  const int* app_k;                   // staged row n_rep + a is appended floe app_k[a] of the whole edit
  long long base;                     // N_global - n_del: the number of appended floe 0
};
// new row r (old row src[r], or staged row -src[r] - 1) -> its new global number
__global__ void __launch_bounds__(256) sz_k_spt_renumber(State S, int Nn, const int* src, SptKeys K, long long* newkey) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < Nn; r += gridDim.x * blockDim.x) {
    const int s = src[r], j = -s - 1;
    if (s < 0 && j >= K.n_rep) { newkey[r] = K.base + K.app_k[j - K.n_rep]; continue; }
    const long long g = S.okey[s >= 0 ? s : K.rep[j]];
    newkey[r] = g - spt_below(K.del, K.n_del, g);
  }
}

}  // namespace sz

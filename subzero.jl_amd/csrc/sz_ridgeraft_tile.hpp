// sz_ridgeraft_tile.hpp — the ridge / raft candidate table (sz_ridgeraft.hpp) over the ONE global floe list whose rows live on the ranks' tiles
// ("tiled contexts").  In the middle of a tiled step a rank's list holds its owned floes, the halo floes and the ghosts of both; every
// row carries its order key (State::okey: a parent's global number, a ghost's (pass << 40) + 4 * gid + k), and the partner column of
// floe.interactions holds key + 1.  Sorted, the distinct keys of all ranks are the single context's list order, so
//   a row is evaluated by ONE rank: the owner of its root parent (a parent: itself; a ghost: the parent that made it)
//   the reference's i < j gate is the comparison of the two keys, never of local positions
//   an entry is (key_i, key_j or the negative boundary / topography number, kind, frac), the keys as exact doubles (they stay under 2^42)
// The gates are rr_row's, through the policy RrTiled.  Kernels:
//   sz_k_rrt_iota     0 .. m - 1: the values of the key sort (rocprim::radix_sort_pairs over okey gives skey / srow, the rows by ascending key)
//   sz_k_rrt_active   which local rows are `active` behind this step's collisions: the owner's word, gathered for the rows of other ranks
//   sz_k_rrt_count    per local row the number of its entries (0 for a row another rank evaluates), the draws of the evaluated rows as
//                     per-wavefront integer sums, and the number of ghost rows whose root parent is owned
//   sz_k_rr_scan      reused: exclusive offsets, the total
//   sz_k_rrt_gscan    ONE workgroup: the ghost rows of owned root parents, their keys packed in local row order
//   sz_k_rrt_write    the records at their offsets: local row order, then first-passing-row order.  No atomic decides a position
//   sz_k_rrt_rename   a key to the single context's list number: a parent's key is its number, a ghost's is N_global + its place among the
//                     gathered, sorted, distinct ghost keys (binary search); over the gathered records and over the local rows
// fp64 in every precision mode, no FMA contraction (the library's flags).
#pragma once
#include "sz_ridgeraft.hpp"

namespace sz {

constexpr int RRT_REC = 4;                              // doubles per entry record: key_i, key_j (or the negative number), kind, frac
constexpr long long RRT_GHOST = (long long)1 << 40;     // keys from here on are ghosts'

struct RrTileDev { int nghost, ninact; };

struct RrTiled {
  using J = long long;
  const long long* skey; const int* srow;               // the local rows by ascending key
  const unsigned char* act;                             // per local row: `active` behind this step's collisions (sz_k_rrt_active)
  int m, nown, npar;                                    // local rows; owned floes; local parents (owned + halo)
  __device__ __forceinline__ int root(const State& S, int i) const { return i < npar ? i : S.parent[i]; }
  __device__ __forceinline__ bool evaluated(const State& S, int i) const { const int r = root(S, i); return r >= 0 && r < nown; }
  __device__ __forceinline__ int partner(const State&, const RrArgs&, int, long long j) const {
    const long long key = j - 1;
    int lo = 0, hi = m;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (skey[mid] < key) lo = mid + 1; else hi = mid; }
    return lo < m && skey[lo] == key ? srow[lo] : -1;
  }
  __device__ __forceinline__ bool before(const State& S, int i, int p) const { return S.okey[i] < S.okey[p]; }
  __device__ __forceinline__ bool active(const State&, int i) const { return act[i] != 0; }
};

// The status of a row behind this step's timestep_collisions! is its owner's to say.  In the middle of a tiled step the tags of an owned parent
// are still bits in its fixed-point words (word 7: the integrator turns them into status), a ghost's are resolved by the row assembly; the rows
// another rank evaluates may have met pairs this rank never saw.  So:
//   own = 1   act[i] of the rows this rank evaluates, their keys where they are not active appended to `inact` (any order: the gathered list is
//             sorted before it is searched), the count in d->ninact
//   own = 0   act[i] of the other rows: not among the gathered, sorted keys `gin` of the rows their owners found not active
__global__ void __launch_bounds__(256) sz_k_rrt_active(State S, RrTiled P, const long long* facc, int own, unsigned char* act, double* inact, int cap, RrTileDev* d,
                                                        const long long* gin, int nin) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P.m; i += gridDim.x * blockDim.x) {
    const bool mine = P.evaluated(S, i);
    if (own && mine) {
      bool a = S.status[i] == SZ_ACTIVE;
      if (a && i < P.nown && facc) a = ((int)(facc[(size_t)i * FX_WORDS + 7] & 0xffffffffll) & 7) == 0;
      act[i] = a ? 1 : 0;
      if (!a) { const int o = atomicAdd(&d->ninact, 1); if (o < cap) inact[o] = (double)S.okey[i]; }
    } else if (!own && !mine) {
      const long long key = S.okey[i];
      int lo = 0, hi = nin;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (gin[mid] < key) lo = mid + 1; else hi = mid; }
      act[i] = lo < nin && gin[lo] == key ? 0 : 1;
    }
  }
}

__global__ void __launch_bounds__(256) sz_k_rrt_iota(int* v, int m) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) v[i] = i;
}

// gflag[i] = 1 for a ghost row whose root parent is owned
__global__ void __launch_bounds__(256) sz_k_rrt_count(State S, RrArgs A, RrTiled P, int* gflag) {
  unsigned long long draws = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += gridDim.x * blockDim.x) {
    int n = 0;
    draws += (unsigned long long)rr_row(S, A, P, i, [&](long long, int, double) { n++; });
    A.cnt[i] = n;
    gflag[i] = i >= P.npar && P.evaluated(S, i) ? 1 : 0;
  }
  for (int d = 32; d >= 1; d >>= 1) draws += __shfl_xor(draws, d);
  if ((threadIdx.x & 63) == 0 && draws) atomicAdd(&A.d->draws, draws);
}

// the keys of the flagged rows, packed in local row order (thread t takes the contiguous chunk t of the rows, as sz_k_rr_scan does)
__global__ void __launch_bounds__(RR_TPB) sz_k_rrt_gscan(State S, const int* gflag, int m, double* gkeys, int cap, RrTileDev* d) {
  __shared__ int part[RR_TPB];
  const int t = threadIdx.x, chunk = (m + RR_TPB - 1) / RR_TPB;
  const int p0 = min(m, t * chunk), p1 = min(m, p0 + chunk);
  int s = 0;
  for (int p = p0; p < p1; p++) s += gflag[p];
  part[t] = s;
  __syncthreads();
  for (int k = 1; k < RR_TPB; k <<= 1) {
    const int v = t >= k ? part[t - k] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = part[t] - s;
  if (gkeys)
    for (int p = p0; p < p1; p++) if (gflag[p]) { if (base < cap) gkeys[base] = (double)S.okey[p]; base++; }
  if (t == RR_TPB - 1) d->nghost = part[t];
}

__global__ void __launch_bounds__(256) sz_k_rrt_write(State S, RrArgs A, RrTiled P, double* rec) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += gridDim.x * blockDim.x) {
    if (A.cnt[i] == 0) continue;
    int o = A.off[i];
    const double ki = (double)S.okey[i];
    rr_row(S, A, P, i, [&](long long j, int kind, double frac) {
      if (o >= 0 && o < A.cap) {
        double* r = rec + (size_t)RRT_REC * o;
        r[0] = ki; r[1] = j > 0 ? (double)(j - 1) : (double)j; r[2] = (double)kind; r[3] = frac;
      }
      o++;
    });
  }
}

// the single context's list number of a key: -1 for a ghost key no rank gathered
__device__ __forceinline__ long long rrt_number(long long key, const long long* gk, int ng, long long nglobal) {
  if (key < RRT_GHOST) return key;
  int lo = 0, hi = ng;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (gk[mid] < key) lo = mid + 1; else hi = mid; }
  return lo < ng && gk[lo] == key ? nglobal + lo : -1;
}
// The gathered records (`slots` of RRT_REC doubles per rank, cnt[r] of them used, base[r] entries before rank r's) into the merged columns ti / tj
// (list numbers; tj keeps a negative number, a partner goes back to the rows' 1-based form), tk, tf; and the list numbers of the local rows.  A key
// that cannot be renamed raises *bad.
__global__ void __launch_bounds__(256) sz_k_rrt_rename(State S, const double* all, const int* cnt, const int* base, int nranks, int slots, const long long* gk, int ng,
                                                        long long nglobal, long long* ti, long long* tj, int* tk, double* tf, long long* rownum, int m, int* bad) {
  const long long nslot = (long long)nranks * slots;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nslot + m; q += (long long)gridDim.x * blockDim.x) {
    if (q < nslot) {
      const int r = (int)(q / slots), k = (int)(q % slots);
      if (k >= cnt[r]) continue;
      const double* e = all + (size_t)RRT_REC * q;
      const int o = base[r] + k;
      const long long ni = rrt_number((long long)e[0], gk, ng, nglobal);
      long long nj = (long long)e[1];
      if (nj >= 0) { nj = rrt_number(nj, gk, ng, nglobal); if (nj < 0) atomicOr(bad, 1); nj += 1; }
      if (ni < 0) atomicOr(bad, 1);
      ti[o] = ni; tj[o] = nj; tk[o] = (int)e[2]; tf[o] = e[3];
    } else {
      const int i = (int)(q - nslot);
      rownum[i] = rrt_number(S.okey[i], gk, ng, nglobal);
    }
  }
}

}  // namespace sz

// sz_weld_tile.hpp — what a tiled context adds to the welding overlap table (sz_weld.hpp): the bins, the `break` of bin_floe_centroids and the
// candidate pairs are properties of the ONE global floe list whose rows live on several ranks, and the two floes of a pair can live on different
// ranks ("tiled contexts").  All numbers below are GLOBAL floe numbers (S.okey of an owned row), N the global count.
//     sz_k_weldt_pack    one record per owned row, in row order: number, centroid, rmax, the bin of weld_index (unchanged), and two flags -- the
//                        centroid fails in_bounds (the expression of sz_k_weld_oob), the floe can weld at all (active, area < max_weld_area).
//                        The records of all ranks are all-gathered: every rank then holds the candidates of the whole field
//     sz_k_weldt_scan    over the gathered records: every number in range and met once (as sz_k_fract_scatter), the smallest number with an
//                        out-of-bounds centroid -- welding.jl:38 breaks there, every floe with a larger number is in no bin, on whichever rank
//                        it lives -- and the largest rmax (the host sizes the search cells from it)
//     sz_k_weldt_insert  the gathered records that are in a bin and can weld into the pass's own search cells (cell_insert), by record slot
//     sz_k_weldt_pairs   per owned candidate the 3 x 3 cells: partners of the same bin that pass potential_interaction (the expression of
//                        sz_k_weld_pairs: strict <, no periodic wrap).  The rank that owns the floe with the SMALLER number owns the pair: a
//                        partner with a larger number gives a key (k N + i) N + j, a partner with a smaller number that lives on another rank
//                        marks the owned floe "wanted" -- the test is symmetric in its two floes to the bit ((a - b)^2 == (b - a)^2, + commutes),
//                        so the partner's rank reaches the same verdict on its own and will ask for this ring.  Also: the final bin of every
//                        owned row, and number -> row for the ring source
//     sz_k_weldt_rings   one record per wanted floe: number, vertex count, osign, the bounding box, the ring points.  All-gathered, the slot
//                        sized by the largest wanted ring of ANY rank
//     sz_k_weldt_src     number -> gathered ring record, for the records of the other ranks
//     (radix sort, sz_k_weld_area<.., WeldTileRings>)   the single context's clipper over this rank's pairs: ring i from the local rows, ring j
//                        from the local rows or a gathered record -- the same staging, region-order sum and capacity-error rule
//     sz_k_weldt_table   ONE workgroup: this rank's entries with inter_area > 0 as {key, area}, ascending (the ballots of sz_k_weld_table).
//                        All-gathered
//     sz_k_weldt_merge   every gathered entry to its place in key order: the per-rank lists are disjoint and ascending, so the place is the
//                        sum of its lower bounds in all of them -> columns i, j, inter_area, identical on every rank
// Every hand-off between workgroups is a kernel boundary.  fp64 throughout.  Nothing of the floes is written.
#pragma once
#include "sz_weld.hpp"

namespace sz {

constexpr int WTC_REC = 6;          // doubles per candidate record: number, cx, cy, rmax, bin, flags
constexpr int WTC_OOB = 1, WTC_CAN = 2;
constexpr int WTR_HEAD = 8;         // doubles in front of a ring record's points: number, vertex count, osign, bbx0, bbx1, bby0, bby1, (spare)
constexpr int WTT_REC = 2;          // doubles per table record: the key's bits, inter_area
constexpr int WT_BAD_RANGE = 1, WT_BAD_TWICE = 2;

struct WeldTileDev { unsigned long long rmax_bits; int first_oob, bad, nwant, maxring; };

__global__ void __launch_bounds__(256) sz_k_weldt_pack(State S, int n, int nx, int ny, double max_area, double* rec) {
  const int per_x = S.ekind[2] == 1, per_y = S.ekind[0] == 1;
  const double dx = (S.gxf - S.gx0) / (double)nx, dy = (S.gyf - S.gy0) / (double)ny;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const double x = S.cx[i], y = S.cy[i];
    double* r = rec + (size_t)WTC_REC * i;
    r[0] = (double)S.okey[i]; r[1] = x; r[2] = y; r[3] = S.rmax[i];
    r[4] = (double)((weld_index(y, S.gy0, S.gyf, dy, ny) - 1) * nx + (weld_index(x, S.gx0, S.gxf, dx, nx) - 1));
    r[5] = (double)((point_in_bounds(S, x, y, per_x, per_y) ? 0 : WTC_OOB) | (S.status[i] == SZ_ACTIVE && S.area[i] < max_area ? WTC_CAN : 0));
  }
}

// all: nranks lists at a stride of `slots` records, cnt[r] in use; mark: total ints, zeroed by the caller
__global__ void __launch_bounds__(256) sz_k_weldt_scan(const double* all, const int* cnt, int nranks, int slots, int total, int* mark, WeldTileDev* D) {
  const long long n = (long long)nranks * slots;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    if ((int)(t % slots) >= cnt[(int)(t / slots)]) continue;
    const double* r = all + (size_t)WTC_REC * t;
    const double g = r[0];
    if (!(g >= 0.0 && g < (double)total) || g != (double)(long long)g) { atomicOr(&D->bad, WT_BAD_RANGE); continue; }
    if (atomicAdd(&mark[(int)g], 1) != 0) { atomicOr(&D->bad, WT_BAD_TWICE); continue; }
    if ((int)r[5] & WTC_OOB) atomicMin(&D->first_oob, (int)g);
    if (r[3] > 0.0) atomicMax(&D->rmax_bits, (unsigned long long)__double_as_longlong(r[3]));          // (positive doubles order as their bits)
  }
}

// is the gathered record in a bin, and can it weld?  (first: the number the reference's loop breaks at)
__device__ __forceinline__ bool weldt_candidate(const double* r, int first) { return ((int)r[5] & WTC_CAN) && !((int)r[5] & WTC_OOB) && (int)r[0] < first; }

// T: the State with the pass's own cell arrays and grid geometry; the cells hold record slots
__global__ void __launch_bounds__(256) sz_k_weldt_insert(State T, const double* all, const int* cnt, int nranks, int slots, const WeldTileDev* D) {
  const int first = D->first_oob;
  const GridGeo g = grid_geo(T);
  const long long n = (long long)nranks * slots;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    if ((int)(t % slots) >= cnt[(int)(t / slots)]) continue;
    const double* r = all + (size_t)WTC_REC * t;
    if (weldt_candidate(r, first)) cell_insert(T, g, (int)t, r[1], r[2]);
  }
}

// W.n: the global count; W.keys_in / W.cap: this rank's pairs.  n_own rows, whose records are the slots me * slots + row.
// bin: per owned row the final bin or -1; wslot: per owned row its slot among this rank's wanted rings or -1; src: number -> row.
// Whole wavefronts go round together, as in sz_k_weld_pairs: one atomic per wavefront reserves the keys of its 64 floes, one its wanted slots.
__global__ void __launch_bounds__(256) sz_k_weldt_pairs(State T, WeldArgs W, const double* all, int slots, int me, int n_own, WeldTileDev* D, int* bin, int* wslot, int* src) {
  const int first = D->first_oob;
  const GridGeo g = grid_geo(T);
  const unsigned long long n64 = (unsigned long long)W.n;
  const int lane = threadIdx.x & 63;
  for (int i0 = (blockIdx.x * blockDim.x + threadIdx.x) & ~63; i0 < n_own; i0 += gridDim.x * blockDim.x) {
    const int i = i0 + lane;
    const bool row = i < n_own;
    const double* ri = all + (size_t)WTC_REC * (row ? me * slots + i : 0);
    int gi = 0, ki = -1, cix = 0, ciy = 0; double xi = 0, yi = 0, rmi = 0; bool act = false;
    if (row) {
      gi = (int)ri[0]; ki = (int)ri[4];
      src[gi] = i;
      bin[i] = !((int)ri[5] & WTC_OOB) && gi < first ? ki : -1;
      act = weldt_candidate(ri, first);
    }
    if (act) { xi = ri[1]; yi = ri[2]; rmi = ri[3]; cell_of(g, xi, yi, cix, ciy); }
    // two rounds, as in sz_k_weld_pairs: count, reserve, write
    auto walk = [&](auto&& hit) {
      for (int iy = max(ciy - 1, 0); iy <= min(ciy + 1, g.ncy - 1); iy++)
        for (int ix = max(cix - 1, 0); ix <= min(cix + 1, g.ncx - 1); ix++) {
          const int c = iy * g.ncx + ix;
          const int cnt = min(T.cell_cnt[c], CELL_K);
          auto test = [&](int tj) {
            const double* rj = all + (size_t)WTC_REC * tj;
            const int gj = (int)rj[0];
            if (gj == gi || (int)rj[4] != ki) return;
            // potential_interaction (collisions.jl:705-710), the floe with the smaller number first as in sz_k_weld_pairs
            const bool lower = gi < gj;
            const double ddx = lower ? xi - rj[1] : rj[1] - xi, ddy = lower ? yi - rj[2] : rj[2] - yi, rr = lower ? rmi + rj[3] : rj[3] + rmi;
            if ((ddx * ddx + ddy * ddy) < rr * rr) hit(gj, tj / slots);
          };
          for (int s = 0; s < cnt; s++) test(T.cell_slots[(size_t)c * CELL_K + s]);
          if (T.cell_cnt[c] > CELL_K) for (int j = T.cell_ovf[c] - 1; j >= 0; j = T.cell_items[j]) test(j);
        }
    };
    int np = 0; bool wanted = false;
    if (act) walk([&](int gj, int owner) { if (gj > gi) np++; else if (owner != me) wanted = true; });
    // the wanted rings of this wavefront: slots from a ballot, the largest ring from a butterfly
    const unsigned long long wm = __ballot(wanted);
    int wbase = 0;
    if (lane == 0 && wm) wbase = atomicAdd(&D->nwant, __popcll(wm));
    wbase = __shfl(wbase, 0);
    if (row) wslot[i] = wanted ? wbase + __popcll(wm & ((1ull << lane) - 1ull)) : -1;
    int mr = wanted ? T.voff[i + 1] - T.voff[i] : 0;
    for (int d = 32; d >= 1; d >>= 1) mr = max(mr, __shfl_xor(mr, d));
    if (lane == 0 && mr > 0) atomicMax(&D->maxring, mr);
    int inc = np;
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    const int tot = __shfl(inc, 63);
    int base = 0;
    if (lane == 0 && tot) base = atomicAdd(&W.d->npairs, tot);
    base = __shfl(base, 0);
    if (np == 0 || base + inc > W.cap) continue;          // (over capacity: the host sees npairs > cap, the ranks agree, grow and run the pass again)
    unsigned long long* out = W.keys_in + (base + inc - np);
    const unsigned long long hi = ((unsigned long long)ki * n64 + (unsigned long long)gi) * n64;
    int q = 0;
    walk([&](int gj, int) { if (gj > gi && q < np) out[q++] = hi + (unsigned long long)gj; });
  }
}

// one wavefront per wanted row; width: doubles per record (WTR_HEAD + 2 * ring capacity).  A ring over the capacity keeps its count and loses its
// points: the ring source then reports it as too long
__global__ void __launch_bounds__(256) sz_k_weldt_rings(State S, int n_own, const int* wslot, int width, double* rec) {
  const int lane = threadIdx.x & 63, nwave = gridDim.x * (blockDim.x >> 6);
  const int ringcap = (width - WTR_HEAD) / 2;
  for (int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_own; i += nwave) {
    const int s = wslot[i];
    if (s < 0) continue;
    double* r = rec + (size_t)width * s;
    const int o = S.voff[i], nv = S.voff[i + 1] - o;
    if (lane == 0) {
      r[0] = (double)S.okey[i]; r[1] = (double)nv; r[2] = (double)S.osign[i];
      r[3] = S.bbx0[i]; r[4] = S.bbx1[i]; r[5] = S.bby0[i]; r[6] = S.bby1[i]; r[7] = 0.0;
    }
    double2* p = (double2*)(r + WTR_HEAD);
    for (int k = lane; k < min(nv, ringcap); k += 64) p[k] = S.vxy[o + k];
  }
}

__global__ void __launch_bounds__(256) sz_k_weldt_src(const double* all, const int* cnt, int nranks, int slots, int width, int me, int total, int* src) {
  const long long n = (long long)nranks * slots;
  const int ringcap = (width - WTR_HEAD) / 2;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(t / slots);
    if (r == me || (int)(t % slots) >= cnt[r]) continue;
    const double* q = all + (size_t)width * t;
    const double g = q[0];
    if (!(g >= 0.0 && g < (double)total) || !(q[1] >= 0.0 && q[1] <= (double)ringcap)) continue;
    src[(int)g] = -2 - (int)t;
  }
}

// the ring source of a tiled pass: keys in global numbers; src[g] >= 0: the local row, <= -2: the gathered ring record -2 - src[g]
struct WeldTileRings {
  const int* src; const double* rec; int width;
  __device__ __forceinline__ WeldRing ring(const State& S, int g) const {
    const int s = src[g];
    if (s >= 0) return WeldRowRings::row(S, s);
    if (s == -1) return { nullptr, 0x7fffffff, 0, Box{ 0.0, 0.0, 0.0, 0.0 } };          // (nobody sent it: the capacity error, nothing is dropped silently)
    const double* r = rec + (size_t)width * (size_t)(-2 - s);
    return { (const double2*)(r + WTR_HEAD), (int)r[1], (int)r[2], Box{ r[3], r[4], r[5], r[6] } };
  }
  __device__ __forceinline__ void pair(const State& S, const WeldArgs& W, unsigned long long key, WeldRing& a, WeldRing& b) const {
    const unsigned long long n64 = (unsigned long long)W.n;
    a = ring(S, (int)((key / n64) % n64)); b = ring(S, (int)(key % n64));
  }
};

// this rank's entries with area > 0 as {key, area}, ascending: the compaction of sz_k_weld_table
__global__ void __launch_bounds__(WELD_TPB) sz_k_weldt_table(WeldArgs W, int npairs, double* rec) {
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
  for (int q = p0; q < p1; q += 64) {
    const int p = q + lane;
    const double a = p < p1 ? W.area[p] : 0.0;
    const bool f = a > 0.0;
    const unsigned long long mask = __ballot(f);
    if (f) {
      const int o = base + __popcll(mask & ((1ull << lane) - 1ull));
      rec[(size_t)WTT_REC * o] = __longlong_as_double((long long)W.keys[p]);
      rec[(size_t)WTT_REC * o + 1] = a;
    }
    base += __popcll(mask);
  }
  if (threadIdx.x == 0) W.d->ntable = total;
}

// all: nranks ascending lists at a stride of `slots` records, cnt[r] in use, no key in two lists; n_global: the N of the keys
__global__ void __launch_bounds__(256) sz_k_weldt_merge(const double* all, const int* cnt, int nranks, int slots, int n_global, long long* ti, long long* tj, double* ta) {
  const long long n = (long long)nranks * slots;
  const unsigned long long n64 = (unsigned long long)n_global;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
    if ((int)(t % slots) >= cnt[(int)(t / slots)]) continue;
    const unsigned long long key = (unsigned long long)__double_as_longlong(all[(size_t)WTT_REC * t]);
    int pos = 0;
    for (int r = 0; r < nranks; r++) {
      const double* L = all + (size_t)WTT_REC * (size_t)r * slots;
      int lo = 0, hi = cnt[r];
      while (lo < hi) { const int mid = (lo + hi) >> 1; if ((unsigned long long)__double_as_longlong(L[(size_t)WTT_REC * mid]) < key) lo = mid + 1; else hi = mid; }
      pos += lo;
    }
    ti[pos] = (long long)((key / n64) % n64); tj[pos] = (long long)(key % n64); ta[pos] = all[(size_t)WTT_REC * t + 1];
  }
}

}  // namespace sz

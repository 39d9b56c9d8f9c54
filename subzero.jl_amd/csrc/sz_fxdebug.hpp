// sz_fxdebug.hpp — test hooks for the fixed-point totals (sz_geom.hpp: fx_ilogb .. fx_word), which are __device__ only: the helpers on given
// numbers, outside every step kernel (sz_debug_fx_totals, sz_debug_fx_word; tests/test_totals_gpu.py holds them to tests/totals_ref.py).
//   sz_k_debug_fx_add    thread t of nthreads takes the values perm[t], perm[t + nthreads], ... , splits each with fx_split, sums its words and
//                        adds them to ONE pair of words -- as the narrow phase does: sums of a lane's rows, then an atomicAdd per non-zero word
//   sz_k_debug_fx_read   (behind it: a kernel boundary) the exponent used and fx_join of the pair
//   sz_k_debug_fx_word   lane w < 7: word w of one row, by fx_word
#pragma once
#include "sz_geom.hpp"

namespace sz {

// how the exponent of sz_debug_fx_totals is formed (its `mode`, bits 0..2); bit 3: kexp is the context's (force_scale_exp), not the argument
enum { FXD_GIVEN = 0, FXD_FORCE = 1, FXD_TORQUE = 2, FXD_AREA = 3, FXD_LEVER = 4, FXD_CTX_KEXP = 8 };

SZ_DEV int fxd_exp(int mode, int e, double area, double height, double rmax) {
  switch (mode) {
    case FXD_FORCE: return fx_force_exp(e, area, height);
    case FXD_TORQUE: return fx_force_exp(e, area, height) + fx_lever_exp(rmax);
    case FXD_AREA: return fx_area_exp(area);
    case FXD_LEVER: return fx_lever_exp(rmax);
    default: return e;
  }
}

// words: { hi, lo } (zero on entry); flags: { bad, e }
__global__ void __launch_bounds__(256) sz_k_debug_fx_add(int n, const double* v, const int* perm, int nthreads, int mode, int e0, double area, double height,
                                                         double rmax, long long* words, int* flags) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nthreads) return;
  const int e = fxd_exp(mode, e0, area, height, rmax);
  long long q = 0, l = 0; int bad = 0;
  for (int k = t; k < n; k += nthreads) {
    long long a = 0, b = 0;
    fx_split(v[perm[k]], e, a, b, bad);
    q += a; l += b;
  }
  unsigned long long* const w = (unsigned long long*)words;
  if (q) atomicAdd(w, (unsigned long long)q);
  if (l) atomicAdd(w + 1, (unsigned long long)l);
  if (bad) atomicOr(flags, 1);
}

__global__ void sz_k_debug_fx_read(int mode, int e0, double area, double height, double rmax, const long long* words, int* flags, double* joined) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int e = fxd_exp(mode, e0, area, height, rmax);
  flags[1] = e;
  joined[0] = fx_join(words[0], words[1], e);
}

// row5: { fx, fy, px, py, overlap }; words14: the high words 0..6, then the low words 0..6; flags[0]: bad
__global__ void sz_k_debug_fx_word(const double* row5, double sign, double cx, double cy, int eF, int eA, int eL, long long* words14, int* flags) {
  const int w = threadIdx.x;
  if (blockIdx.x != 0 || w >= 7) return;
  long long hi = 0, lo = 0; int bad = 0;
  fx_word(w, row5, sign, cx, cy, eF, eA, eL, hi, lo, bad);
  words14[w] = hi; words14[7 + w] = lo;
  if (bad) atomicOr(flags, 1);
}

}  // namespace sz

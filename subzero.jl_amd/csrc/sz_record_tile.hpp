// sz_record_tile.hpp — the merge of the ranks' tile frames into the single context's floe frame (sz_tile_download_floe_frame; DESIGN.md §9i,
// "Tiled contexts").  A tile frame is sz_record.hpp's FrameLayout over a rank's own rows -- its owned parents and their ghosts -- plus the key
// section: a parent's key is its global number, a ghost's (pass << 40) + 4 * parent key + k, so the rows of all ranks sorted by key ARE the
// single context's list of that step (§9e), ghosts included.  The frames of all ranks arrive in slots of one size (comm_allgather); rocprim
// sorts (key, gathered row) pairs; then every selected section is written at its merged place:
//   sz_k_rect_keys     per gathered row: its key, and its own number as the sort's value
//   sz_k_rect_counts   per merged row m (gathered row src[m]): pos[src[m]] = m, the row's ring points, a parent's ghost links
//                      (two exclusive scans of those counts give vert_off and ghost_off, written straight into the merged frame)
//   sz_k_rect_scatter  blockIdx.y = the pack's slices: a column is read by sorted order and written coalesced; ring points find their row by
//                      bisection in the merged vert_off; ghost_idx is pos[] of (rank, local ghost row), so no order of a rank's ghost rows is
//                      assumed; the header.
// THE LISTS (sz_tile_set_floe_output_lists; TileListLayout below).  A tile frame of a writer with lists carries, behind its key section, the
// sorted order keys of the LAST step's rows behind its owned parents (the interactions only: a rank's rows name ghost partners by key + 1, and
// the frame's own ghosts are those of the record point) and sz_record.hpp's list sections over its own rows, partners untranslated.  The merge:
//   sz_k_rect_lkeys        the ranks' key tables one behind the other; rocprim sorts them
//   sz_k_rect_kflags       per sorted entry: the first of a ghost key (>= 2^40; the halo parents' keys sort to the front and count nothing);
//                          an exclusive scan of the flags gives every entry the number of distinct ghost keys in front of it -- the union of the
//                          ranks' ghosts of a step IS the single context's ghost list of that step (§9e), so that number is the ghost's rank there
//   sz_k_rect_list_counts  per merged row its interaction rows (a ghost row: none) and sub-floe points (two exclusive scans give inter_off and
//                          sub_off, written straight into the merged frame)
//   sz_k_rect_lists        blockIdx.y = the list, element-parallel: one thread per output double / per point finds its merged row by bisection in
//                          the merged offsets, reads (rank, local row) through src[] / row0[] at the local offset of that rank's own section and
//                          stores coalesced; column 0 of an interaction row above 2^40 becomes N_global + rank of the key + 1 in the same pass
// No atomic decides a position: two merges of one frame give the same bits.  Every store is indexed by a loop variable below a count the host
// made the merged layout from; what is read out of a peer's frame as an index is clamped before it is used.
#pragma once
#include "sz_record.hpp"

namespace sz {

// a tile frame: the single layout, then the keys
struct TileFrameLayout : FrameLayout {
  long long key;
  TileFrameLayout(unsigned long long mask, long long M, long long N, long long V) : FrameLayout(mask, M, N, V) { key = total; total += M * 8; }
};

// ... of a writer with lists: behind the keys the last step's key table, int64 [K], sorted (with the interactions only), then ListLayout's sections
struct TileListLayout {
  long long lkey, base, off[FL_NSEC], total;          // base: where ListLayout's sections begin
  TileListLayout(unsigned long long mask, unsigned lists, long long M, long long N, long long V, long long R, long long S, long long K) {
    const long long keys_end = TileFrameLayout(mask, M, N, V).total;
    const bool in = lists & FR_LIST_INTER;
    lkey = in ? keys_end : -1;
    base = keys_end + (in ? K * 8 : 0);
    const ListLayout L(base, lists, M, R, S);
    for (int k = 0; k < FL_NSEC; k++) off[k] = L.off[k];
    total = L.total;
  }
};

constexpr int RECT_RANKS = 64;          // the most ranks of a communicator (Gather::RANKS)
// a rank's sections in the merge's table: the frame's, the keys, the key table of the lists, the list sections
constexpr int RS_KEY = FR_NSEC, RS_LKEY = FR_NSEC + 1, RS_LIST = FR_NSEC + 2, RECT_NSEC = RS_LIST + FL_NSEC;
// what the merge kernels are told: the gathered slots, per rank the byte offset of every section from the start of `all` (-1: not recorded)
// and its first gathered row; the sorted order and its inverse; the merged frame and its layout
struct RectArgs {
  const char* all; const long long* sec;          // sec[r * RECT_NSEC + section]
  const int* row0;                                // [nranks + 1]: gathered rows of rank r are row0[r] .. row0[r + 1] - 1, local row = gathered row - row0[r]
  const int* npar;                                // [nranks]: the parents among them
  const int* src; int* pos;                       // src[m]: the gathered row at merged place m; pos: its inverse
  int *nv, *ng;                                   // [Mg + 1] counts in merged order (entry Mg = 0)
  char* out; long long off[FR_NSEC];
  int nranks, Mg, Ng, Vg, tstep;
  // the lists (lists == 0: none of what follows is looked at)
  unsigned lists;
  const int* lcnt;                                // [3 * nranks]: {R, S, K} of rank r's frame, the host's
  const int* kbase;                               // [nranks + 1]: the entries of rank r's key table are kbase[r] .. kbase[r + 1] - 1 of the concatenation
  int *ni, *ns;                                   // [Mg + 1] counts in merged order (entry Mg = 0)
  const long long* dkeys; const int* drank;       // the sorted concatenation, and per entry the distinct ghost keys in front of it
  long long loff[FL_NSEC];                        // the merged frame's list sections
  int Kt, Rg, Sg;
  int list0;                                      // sz_k_rect_lists: the list of blockIdx.y == 0 (a call moves only the lists it returns)
};

// the ranks' first rows in LDS, and for this workgroup's slice up to three of its section offsets per rank
struct RectLds { int row0[RECT_RANKS + 1], npar[RECT_RANKS]; long long sec[RECT_RANKS][3]; };
__device__ __forceinline__ void rect_load(const RectArgs& A, RectLds& L, int s0, int s1, int s2) {
  for (int r = threadIdx.x; r <= A.nranks; r += blockDim.x) L.row0[r] = A.row0[r];
  for (int r = threadIdx.x; r < A.nranks; r += blockDim.x) {
    L.npar[r] = A.npar[r];
    const long long* t = A.sec + (size_t)r * RECT_NSEC;
    L.sec[r][0] = s0 >= 0 ? t[s0] : -1; L.sec[r][1] = s1 >= 0 ? t[s1] : -1; L.sec[r][2] = s2 >= 0 ? t[s2] : -1;
  }
  __syncthreads();
}
__device__ __forceinline__ int rect_rank(const RectLds& L, int nranks, int s) {
  int r = 0;
  while (r + 1 < nranks && s >= L.row0[r + 1]) r++;
  return r;
}

constexpr int RECT_TPB = 256;

__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_keys(RectArgs A, long long* key_in, int* val_in) {
  __shared__ RectLds L;
  rect_load(A, L, RS_KEY, -1, -1);
  for (int s = blockIdx.x * RECT_TPB + threadIdx.x; s < A.Mg; s += gridDim.x * RECT_TPB) {
    const int r = rect_rank(L, A.nranks, s);
    key_in[s] = ((const long long*)(A.all + L.sec[r][0]))[s - L.row0[r]];
    val_in[s] = s;
  }
}

__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_counts(RectArgs A) {
  __shared__ RectLds L;
  rect_load(A, L, A.off[FR_VOFF] >= 0 ? FR_VOFF : -1, A.off[FR_GOFF] >= 0 ? FR_GOFF : -1, -1);
  for (int m = blockIdx.x * RECT_TPB + threadIdx.x; m <= A.Mg; m += gridDim.x * RECT_TPB) {
    if (m == A.Mg) { A.nv[m] = 0; A.ng[m] = 0; break; }
    const int s = A.src[m], r = rect_rank(L, A.nranks, s), j = s - L.row0[r];
    A.pos[s] = m;
    int nv = 0, ng = 0;
    if (L.sec[r][0] >= 0) { const int* v = (const int*)(A.all + L.sec[r][0]); nv = max(v[j + 1] - v[j], 0); }
    if (L.sec[r][1] >= 0 && m < A.Ng) { const int* g = (const int*)(A.all + L.sec[r][1]); ng = min(max(g[j + 1] - g[j], 0), MAX_GHOSTS); }
    A.nv[m] = nv; A.ng[m] = ng;
  }
}

// grid (x, FP_SLICES): the slices of sz_k_frame_pack.  vert_off and ghost_off of the merged frame are already in place (the scans).
__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_scatter(RectArgs A) {
  __shared__ RectLds L;
  const int y = blockIdx.y, Mg = A.Mg;
  const long long t0 = (long long)blockIdx.x * RECT_TPB + threadIdx.x, stride = (long long)gridDim.x * RECT_TPB;
  if (y < MIG_NTAB || y == FR_BIT_ID || y == FR_BIT_GHOST_ID || y == FR_BIT_STATUS) {
    const int sec = y < MIG_NTAB ? y : y == FR_BIT_ID ? FR_ID : y == FR_BIT_GHOST_ID ? FR_GHOST_ID : FR_STATUS;
    if (A.off[sec] < 0) return;
    rect_load(A, L, sec, -1, -1);
    char* out = A.out + A.off[sec];
    if (y == FR_BIT_STATUS) {
      for (long long m = t0; m < Mg; m += stride) {
        const int s = A.src[m], r = rect_rank(L, A.nranks, s);
        ((int*)out)[m] = ((const int*)(A.all + L.sec[r][0]))[s - L.row0[r]];
      }
    } else if (y < MIG_NSC || y >= MIG_NTAB) {          // 8 bytes per row: a scalar column, id, ghost_id
      for (long long m = t0; m < Mg; m += stride) {
        const int s = A.src[m], r = rect_rank(L, A.nranks, s);
        ((long long*)out)[m] = ((const long long*)(A.all + L.sec[r][0]))[s - L.row0[r]];
      }
    } else {
      for (long long e = t0; e < 4ll * Mg; e += stride) {
        const int s = A.src[e >> 2], r = rect_rank(L, A.nranks, s);
        ((long long*)out)[e] = ((const long long*)(A.all + L.sec[r][0]))[4ll * (s - L.row0[r]) + (e & 3)];
      }
    }
  } else if (y == FR_BIT_RINGS) {
    if (A.off[FR_VOFF] < 0) return;
    rect_load(A, L, FR_VOFF, FR_VX, FR_VY);
    const int* voff = (const int*)(A.out + A.off[FR_VOFF]);
    double *vx = (double*)(A.out + A.off[FR_VX]), *vy = (double*)(A.out + A.off[FR_VY]);
    for (long long p = t0; p < A.Vg; p += stride) {
      int lo = 0, hi = Mg;                        // the last row m with voff[m] <= p
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (voff[mid] <= p) lo = mid; else hi = mid; }
      const int s = A.src[lo], r = rect_rank(L, A.nranks, s), j = s - L.row0[r];
      const int* lv = (const int*)(A.all + L.sec[r][0]);
      const long long q = (long long)lv[j] + (p - voff[lo]), Vr = lv[L.row0[r + 1] - L.row0[r]];
      const bool ok = q >= 0 && q < Vr;
      vx[p] = ok ? ((const double*)(A.all + L.sec[r][1]))[q] : 0.0;
      vy[p] = ok ? ((const double*)(A.all + L.sec[r][2]))[q] : 0.0;
    }
  } else {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      long long* h = (long long*)A.out;
      h[0] = A.tstep; h[1] = Mg; h[2] = A.Ng; h[3] = A.Vg; h[4] = Mg - A.Ng; h[5] = h[6] = h[7] = 0;
    }
    if (A.off[FR_GOFF] < 0) return;
    rect_load(A, L, FR_GOFF, FR_GIDX, -1);
    const int* goff = (const int*)(A.out + A.off[FR_GOFF]);
    int* gidx = (int*)(A.out + A.off[FR_GIDX]);
    const int G = Mg - A.Ng;
    for (long long i = t0; i < A.Ng; i += stride) {
      const int s = A.src[i], r = rect_rank(L, A.nranks, s), j = s - L.row0[r], Mr = L.row0[r + 1] - L.row0[r];
      const int* lg = (const int*)(A.all + L.sec[r][0]);
      const int* li = (const int*)(A.all + L.sec[r][1]);
      const int a = lg[j], n = goff[i + 1] - goff[i], o = goff[i], Gr = Mr - L.npar[r];
      for (int q = 0; q < n && o + q < G; q++) {
        const int g = a >= 0 && a + q < Gr ? li[a + q] : -1;
        gidx[o + q] = g >= 0 && g < Mr ? A.pos[L.row0[r] + g] : -1;
      }
    }
  }
}

// ---- the lists
// ... with a count of the lists per rank ({R, S, K}[which]) in place of the parents
__device__ __forceinline__ void rect_load_lists(const RectArgs& A, RectLds& L, int s0, int s1, int s2, int which) {
  rect_load(A, L, s0, s1, s2);
  for (int r = threadIdx.x; r < A.nranks; r += blockDim.x) L.npar[r] = max(A.lcnt[3 * r + which], 0);
  __syncthreads();
}

__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_lkeys(RectArgs A, long long* kcat) {
  __shared__ int kb[RECT_RANKS + 1]; __shared__ long long at[RECT_RANKS];
  for (int r = threadIdx.x; r <= A.nranks; r += blockDim.x) kb[r] = A.kbase[r];
  for (int r = threadIdx.x; r < A.nranks; r += blockDim.x) at[r] = A.sec[(size_t)r * RECT_NSEC + RS_LKEY];
  __syncthreads();
  for (int i = blockIdx.x * RECT_TPB + threadIdx.x; i < A.Kt; i += gridDim.x * RECT_TPB) {
    int r = 0;
    while (r + 1 < A.nranks && i >= kb[r + 1]) r++;
    kcat[i] = at[r] >= 0 ? ((const long long*)(A.all + at[r]))[i - kb[r]] : 0;
  }
}

// flag[i]: sorted entry i is the first of a ghost key (entry Kt: 0)
__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_kflags(const long long* ks, int* flag, int Kt) {
  for (int i = blockIdx.x * RECT_TPB + threadIdx.x; i <= Kt; i += gridDim.x * RECT_TPB)
    flag[i] = i < Kt && ks[i] >= ((long long)1 << 40) && (i == 0 || ks[i] != ks[i - 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_list_counts(RectArgs A) {
  __shared__ RectLds L;
  rect_load(A, L, A.loff[FL_IOFF] >= 0 ? RS_LIST + FL_IOFF : -1, A.loff[FL_SOFF] >= 0 ? RS_LIST + FL_SOFF : -1, -1);
  for (int m = blockIdx.x * RECT_TPB + threadIdx.x; m <= A.Mg; m += gridDim.x * RECT_TPB) {
    int ni = 0, ns = 0;
    if (m < A.Mg) {
      const int s = A.src[m], r = rect_rank(L, A.nranks, s), j = s - L.row0[r];
      if (L.sec[r][0] >= 0 && m < A.Ng) { const int* o = (const int*)(A.all + L.sec[r][0]); ni = min(max(o[j + 1] - o[j], 0), max(A.lcnt[3 * r], 0)); }
      if (L.sec[r][1] >= 0) { const int* o = (const int*)(A.all + L.sec[r][1]); ns = min(max(o[j + 1] - o[j], 0), max(A.lcnt[3 * r + 1], 0)); }
    }
    if (A.loff[FL_IOFF] >= 0) A.ni[m] = ni;
    if (A.loff[FL_SOFF] >= 0) A.ns[m] = ns;
  }
}

// grid (x, 1 or 2): list = blockIdx.y + list0.  inter_off / sub_off of the merged frame are already in place (the scans); the three spare header words become {lists, R, S},
// as sz_k_frame_lists leaves them in the single context's frame (behind sz_k_rect_scatter in the stream, which zeroes them).
__global__ void __launch_bounds__(RECT_TPB) sz_k_rect_lists(RectArgs A) {
  __shared__ RectLds L;
  const long long t0 = (long long)blockIdx.x * RECT_TPB + threadIdx.x, stride = (long long)gridDim.x * RECT_TPB;
  if (blockIdx.y + A.list0 == 0) {
    if (t0 == 0) { long long* h = (long long*)A.out; h[5] = A.lists; h[6] = A.loff[FL_IOFF] >= 0 ? A.Rg : 0; h[7] = A.loff[FL_SOFF] >= 0 ? A.Sg : 0; }
    if (A.loff[FL_IOFF] < 0 || A.Ng <= 0) return;
    rect_load_lists(A, L, RS_LIST + FL_IOFF, RS_LIST + FL_IROWS, -1, 0);
    const int* ioff = (const int*)(A.out + A.loff[FL_IOFF]);
    double* out = (double*)(A.out + A.loff[FL_IROWS]);
    const double lim = (double)((long long)1 << 40);
    for (long long e = t0; e < 7ll * A.Rg; e += stride) {
      const long long row = e / 7; const int k = (int)(e - 7 * row);
      int lo = 0, hi = A.Ng;                      // the last parent i with ioff[i] <= row: the one that owns it (empty parents share an offset)
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ioff[mid] <= row) lo = mid; else hi = mid; }
      const int s = A.src[lo], r = rect_rank(L, A.nranks, s), j = s - L.row0[r];
      double v = 0.0;
      if (L.sec[r][0] >= 0) {
        const long long q = (long long)((const int*)(A.all + L.sec[r][0]))[j] + (row - ioff[lo]);
        if (q >= 0 && q < L.npar[r]) v = ((const double*)(A.all + L.sec[r][1]))[7 * q + k];
      }
      if (k == 0 && A.Kt > 0 && v > lim) {
        const long long key = (long long)v - 1;
        int a = 0, b = A.Kt;                      // lower bound
        while (a < b) { const int mid = (a + b) >> 1; if (A.dkeys[mid] < key) a = mid + 1; else b = mid; }
        if (a < A.Kt && A.dkeys[a] == key) v = (double)((long long)A.Ng + A.drank[a] + 1);
      }
      out[e] = v;
    }
  } else {
    if (A.loff[FL_SOFF] < 0 || A.Mg <= 0) return;
    rect_load_lists(A, L, RS_LIST + FL_SOFF, RS_LIST + FL_SX, RS_LIST + FL_SY, 1);
    const int* soff = (const int*)(A.out + A.loff[FL_SOFF]);
    double *sx = (double*)(A.out + A.loff[FL_SX]), *sy = (double*)(A.out + A.loff[FL_SY]);
    for (long long p = t0; p < A.Sg; p += stride) {
      int lo = 0, hi = A.Mg;                      // the last row with soff[row] <= p
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (soff[mid] <= p) lo = mid; else hi = mid; }
      const int s = A.src[lo], r = rect_rank(L, A.nranks, s), j = s - L.row0[r];
      long long q = -1;
      if (L.sec[r][0] >= 0) q = (long long)((const int*)(A.all + L.sec[r][0]))[j] + (p - soff[lo]);
      const bool ok = q >= 0 && q < L.npar[r];
      sx[p] = ok ? ((const double*)(A.all + L.sec[r][1]))[q] : 0.0;
      sy[p] = ok ? ((const double*)(A.all + L.sec[r][2]))[q] : 0.0;
    }
  }
}

}  // namespace sz

// sz_splice.hpp — device side of sz_download_rows / sz_download_list_rows and sz_splice_floes / sz_splice_parents: a few rows of the resident list go down to the host,
// the host edits them, and the edit -- rows replaced in place, rows deleted, rows appended -- is spliced back; the other rows stay in HBM.
//
// A splice is a migration whose stream comes from the host, combined with removal's compaction.  The host packs the n_rep + n_app uploaded rows
// into ONE stream of migration records with its directory (sz_migrate.hpp: MIG_NCOL doubles, the ring as {x, y} pairs, the sub-floe points
// x.. then y..), so the rows are gathered by the migration's own kernels (sz_k_mig_gather, sz_k_mig_points: new row r from old row src[r] or
// from record -src[r] - 1) and placed by sz_k_mig_scatter.  What is new here:
//     sz_k_sp_marks        delete / replace marks onto per-row flags (0 keep, -1 delete, 1 + j replaced by staged row j)
//     sz_k_sp_flags        per old row: stays (as it is or replaced), and the ring / sub-floe points it then has -- old or staged lengths
//     scans                keep flags -> new row numbers; the lengths -> the new CSR offsets (removal's scans)
//     sz_k_sp_rows         new row -> source (a negative entry names a staged row) and its offsets; the appended rows behind the last kept one
//     sz_k_sp_limits       over the new rows: longest ring, most sub-floe points, rows whose status is not `active` (what an upload finds on the host)
//     sz_k_sp_gather_rows  what a migration does not carry, one wavefront per new row: the interaction rows, kept ones from the old rows (a partner
//     sz_k_sp_scatter_rows that was an inline ghost is renumbered as a download would), staged ones from the uploaded CSR; and back, with `origin` and
//                          the order keys as the identity (a tiled context's share of a global edit, sz_splice_tile.hpp: as the new global numbers)
//                          and the tag column equal to the status column, as sz_upload_floes leaves them
//     sz_k_sp_clear_rows   the rows a shrinking list vacates, zeroed
//     sz_k_sp_sel_len,     sz_download_rows / sz_download_list_rows: the lengths of the selected rows (scanned into the offsets of the staging buffer),
//     sz_k_sp_pack         then one wavefront per selected row packs columns, ring, sub-floe points, interaction rows and ghost list into that buffer
// Rows move through temporaries (an in-place parallel shift races: sz_remove.hpp); every hand-off between workgroups is a kernel boundary; fp64
// values move as bits.
#pragma once
#include "sz_remove.hpp"

namespace sz {

constexpr int SP_MAX_RING = 255;      // ring points of a spliced floe: what the collision record (State::crec, 8 bits) and a halo record carry
// (SP_NCOL, the doubles per row the column gather moves, and SP_PACK_NCOL, those of sz_download_rows' staging buffer -- ghost_id at SP_GHOST_ID --: sz_columns.hpp)

struct SpDev {
  int Nn, Vn, NSn;                    // sz_k_sp_rows: rows, ring points and sub-floe points of the edited list
  int max_ring, max_sub, n_tagged;    // sz_k_sp_limits
};

struct SpArgs {
  int n;                              // rows of the list before the edit
  int n_del, n_rep, n_app;
  const int *del, *rep;               // ascending old rows
  const int *svoff, *ssoff;           // CSR offsets of the staged rows' rings and sub-floe points (n_rep + n_app + 1 entries each)
  int *mark, *keep, *kv, *ks;         // per old row
  int *newrow, *ovoff, *osoff;        // their exclusive scans (n + 1 entries)
  int *src, *nvoff, *nsoff;           // per new row
  SpDev* d;
};

__global__ void __launch_bounds__(256) sz_k_sp_marks(SpArgs A) {
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < A.n_del + A.n_rep; t += gridDim.x * blockDim.x) {
    const int row = t < A.n_del ? A.del[t] : A.rep[t - A.n_del];
    if (row >= 0 && row < A.n) A.mark[row] = t < A.n_del ? -1 : 1 + (t - A.n_del);
  }
}

__global__ void __launch_bounds__(256) sz_k_sp_flags(State S, SpArgs A) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n; i += gridDim.x * blockDim.x) {
    const int m = A.mark[i], keep = m >= 0;
    int nv = S.voff[i + 1] - S.voff[i], ns = S.soff[i + 1] - S.soff[i];
    if (m > 0) { nv = A.svoff[m] - A.svoff[m - 1]; ns = A.ssoff[m] - A.ssoff[m - 1]; }
    A.keep[i] = keep; A.kv[i] = keep ? nv : 0; A.ks[i] = keep ? ns : 0;
  }
}

__global__ void __launch_bounds__(256) sz_k_sp_rows(SpArgs A) {
  const int Nk = A.newrow[A.n], V0 = A.ovoff[A.n], S0 = A.osoff[A.n], ns = A.n_rep + A.n_app;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < max(A.n, A.n_app); i += gridDim.x * blockDim.x) {
    if (i < A.n && A.keep[i]) { const int r = A.newrow[i], m = A.mark[i]; A.src[r] = m > 0 ? -m : i; A.nvoff[r] = A.ovoff[i]; A.nsoff[r] = A.osoff[i]; }
    if (i < A.n_app) {
      const int r = Nk + i, j = A.n_rep + i;
      A.src[r] = -(j + 1); A.nvoff[r] = V0 + A.svoff[j] - A.svoff[A.n_rep]; A.nsoff[r] = S0 + A.ssoff[j] - A.ssoff[A.n_rep];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int Nn = Nk + A.n_app, Vn = V0 + A.svoff[ns] - A.svoff[A.n_rep], NSn = S0 + A.ssoff[ns] - A.ssoff[A.n_rep];
    A.nvoff[Nn] = Vn; A.nsoff[Nn] = NSn;
    A.d->Nn = Nn; A.d->Vn = Vn; A.d->NSn = NSn;
  }
}

// dirs / recv: the staged stream as sz_k_mig_gather reads it (record -s - 1 of the directory; its status is double MIG_STATUS)
__global__ void __launch_bounds__(256) sz_k_sp_limits(State S, SpArgs A, int Nn, const double* dirs, const double* recv) {
  const int lane = threadIdx.x & 63;
  for (int r0 = blockIdx.x * blockDim.x; r0 < Nn; r0 += gridDim.x * blockDim.x) {
    const int r = r0 + threadIdx.x;
    int nv = 0, ns = 0; bool tagged = false;
    if (r < Nn) {
      const int s = A.src[r];
      nv = A.nvoff[r + 1] - A.nvoff[r]; ns = A.nsoff[r + 1] - A.nsoff[r];
      const int st = s >= 0 ? S.status[s] : (int)recv[(size_t)dirs[(size_t)MIG_DIR * (size_t)(-s) + 3] + MIG_STATUS];
      tagged = st != SZ_ACTIVE;
    }
    for (int d = 32; d >= 1; d >>= 1) { nv = max(nv, __shfl_xor(nv, d)); ns = max(ns, __shfl_xor(ns, d)); }
    const unsigned long long bt = __ballot(tagged);
    if (lane == 0) {
      if (nv) atomicMax(&A.d->max_ring, nv);
      if (ns) atomicMax(&A.d->max_sub, ns);
      if (bt) atomicAdd(&A.d->n_tagged, __popcll(bt));
    }
  }
}

// order key + 1 of an inline ghost (> 2^40) in column 0 of an interaction row -> the reference's 1-based number N + rank + 1 among the sorted
// keys of the last step's ghosts, as sz_download_interactions renumbers it on the host; a key that is not among them stays
__device__ __forceinline__ double sp_partner(double idx, const long long* keys, int nkeys, int N) {
  if (!(idx > (double)((long long)1 << 40)) || nkeys <= 0) return idx;
  const long long key = (long long)idx - 1;
  int lo = 0, hi = nkeys;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < key) lo = mid + 1; else hi = mid; }
  return lo < nkeys && keys[lo] == key ? (double)(N + lo + 1) : idx;
}

// t_rows at a stride of tcap rows per floe (the context's rowcap at the time of the gather); sioff / srows: CSR of the staged rows' interactions
__global__ void __launch_bounds__(256) sz_k_sp_gather_rows(State S, int Nn, const int* src, const int* sioff, const double* srows, const long long* keys, int nkeys,
                                                           int Nold, int tcap, int* t_cnt, double* t_rows) {
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  for (int r = wave; r < Nn; r += nw) {
    const int s = src[r];
    double* to = t_rows + (size_t)tcap * 7 * r;
    if (s >= 0) {
      const int cnt = S.inter_cnt[s], n = min(min(max(cnt, 0), S.rowcap), tcap) * 7;
      if (lane == 0) t_cnt[r] = cnt;
      const double* from = S.inter_rows + (size_t)S.rowcap * 7 * s;
      for (int k = lane; k < n; k += 64) { const double v = from[k]; to[k] = k % 7 == 0 ? sp_partner(v, keys, nkeys, Nold) : v; }
    } else {
      const int j = -s - 1, o = sioff ? sioff[j] : 0, cnt = sioff ? sioff[j + 1] - o : 0, n = min(max(cnt, 0), tcap) * 7;
      if (lane == 0) t_cnt[r] = cnt;
      const double* from = srows + (size_t)o * 7;
      for (int k = lane; k < n; k += 64) to[k] = from[k];
    }
  }
}
// newkey: the order keys of the new rows (a tiled context's share of a global edit: their global numbers) or null: the identity
__global__ void __launch_bounds__(256) sz_k_sp_scatter_rows(State S, int Nn, int* origin, const long long* newkey, int tcap, const int* t_cnt, const double* t_rows) {
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  for (int r = wave; r < Nn; r += nw) {
    const int cnt = t_cnt[r], n = min(min(max(cnt, 0), S.rowcap), tcap) * 7;
    if (lane == 0) { const long long key = newkey ? newkey[r] : r; origin[r] = (int)key; S.okey[r] = key; S.inter_cnt[r] = cnt; S.tagA[r] = S.status[r]; }      // (an appended floe lies in a row that held a ghost, with the ghost's order key)
    const double* from = t_rows + (size_t)tcap * 7 * r;
    double* to = S.inter_rows + (size_t)S.rowcap * 7 * r;
    for (int k = lane; k < n; k += 64) to[k] = from[k];
  }
}

// rows [from, to) of the columns -> 0: the rows a shrinking list vacates.  Nothing reads them as floes, but a ghost that is placed there keeps what the
// makers do not write (the previous-step columns), and a download shows it: a list that was uploaded afresh shows zeros
__global__ void __launch_bounds__(256) sz_k_sp_clear_rows(int from, int to, double* const* cols) {
  for (int r = from + blockIdx.x * blockDim.x + threadIdx.x; r < to; r += gridDim.x * blockDim.x) {
    for (int k = 0; k < MIG_NSC; k++) cols[k][r] = 0.0;
    for (int t = 0; t < MIG_NTEN; t++) for (int q = 0; q < 4; q++) cols[MIG_NSC + t][(size_t)4 * r + q] = 0.0;
  }
}

// ---- sz_download_rows / sz_download_list_rows
// len[a (n + 1) + k], a = 0..3: ring points, sub-floe points, interaction rows and ghost-list entries of selected row k (four arrays of n + 1
// entries).  nsub: the rows below it have sub-floe points (the parents of a list uploaded with points; 0: none) -- the points' offsets are not read
// at or beyond it, a ghost row has no points; nlist: the rows below it have a ghost list that is reported (0: sz_download_rows, which writes zeros)
__global__ void __launch_bounds__(256) sz_k_sp_sel_len(State S, int n, const int* rows, int nsub, int nlist, int* len) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
    const int i = rows[k];
    len[k] = S.voff[i + 1] - S.voff[i];
    len[n + 1 + k] = i < nsub ? S.soff[i + 1] - S.soff[i] : 0;
    len[2 * (n + 1) + k] = min(max(S.inter_cnt[i], 0), S.rowcap);
    len[3 * (n + 1) + k] = i < nlist ? min(S.ngh[i] & 0xff, MAX_GHOSTS) : 0;
  }
}
// The staging buffer, in doubles: [0, SP_PACK_NCOL n) the columns (column q of selected row k at q n + k; id, status and ghost_id as bits in a double's place),
// then the rings as {x, y} pairs, the sub-floe points x.. and y.., the interaction rows, and last the ghost lists as 32-bit list numbers (two to a
// double's place); off: the scanned lengths (4 x (n + 1)).
// cols: the device copy of state_columns(S).
__global__ void __launch_bounds__(256) sz_k_sp_pack(State S, int n, const int* rows, const int* off, double* const* cols, double* out) {
  const int lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const int* voff = off; const int* soff = off + (n + 1); const int* ioff = off + 2 * (n + 1); const int* goff = off + 3 * (n + 1);
  const size_t V = (size_t)voff[n], NS = (size_t)soff[n], R = (size_t)ioff[n];
  double* ring = out + (size_t)SP_PACK_NCOL * n;
  double* sx = ring + 2 * V; double* sy = sx + NS; double* irow = sy + NS;
  int* glist = (int*)(irow + 7 * R);
  for (int k = wave; k < n; k += nw) {
    const int i = rows[k];
    if (lane < MIG_NSC) out[(size_t)lane * n + k] = cols[lane][i];
    else if (lane < MIG_ID) { const int t = (lane - MIG_TEN) >> 2, q = (lane - MIG_TEN) & 3; out[(size_t)lane * n + k] = cols[MIG_NSC + t][(size_t)4 * i + q]; }
    else if (lane == MIG_ID) out[(size_t)MIG_ID * n + k] = __longlong_as_double(S.id[i]);
    else if (lane == MIG_STATUS) out[(size_t)MIG_STATUS * n + k] = __longlong_as_double((long long)S.status[i]);
    else if (lane == SP_GHOST_ID) out[(size_t)SP_GHOST_ID * n + k] = __longlong_as_double(S.ghost_id[i]);
    const int vo = S.voff[i], nv = voff[k + 1] - voff[k], ns = soff[k + 1] - soff[k], ni = (ioff[k + 1] - ioff[k]) * 7, ng = goff[k + 1] - goff[k];
    const int po = ns > 0 ? S.soff[i] : 0;
    const double* from = (const double*)(S.vxy + vo);
    double* to = ring + 2 * (size_t)voff[k];
    for (int q = lane; q < 2 * nv; q += 64) to[q] = from[q];
    for (int q = lane; q < ns; q += 64) { sx[soff[k] + q] = S.sx[po + q]; sy[soff[k] + q] = S.sy[po + q]; }
    const double* rf = S.inter_rows + (size_t)S.rowcap * 7 * i;
    double* rt = irow + (size_t)ioff[k] * 7;
    for (int q = lane; q < ni; q += 64) rt[q] = rf[q];
    if (lane < ng) glist[goff[k] + lane] = S.gh[i * MAX_GHOSTS + lane];
  }
}

}  // namespace sz

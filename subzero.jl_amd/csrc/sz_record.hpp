// sz_record.hpp — the output recorder: what the reference's writers take at an output step, kept in HBM until the host asks for it.
// write_data! runs at the start of a step, right behind add_ghosts! (simulation.jl:102-105).  With a writer registered (sz_set_floe_output,
// sz_set_grid_output) sz_step cuts its batch BEFORE every output step (sz_stops.hpp: StopRules::out_dts, the hook record()) and, at the cut:
// detaches ghosts a process call left attached, sz_add_ghosts, one sz_k_frame_pack launch per due floe writer, the averages of
// calc_eulerian_data! per due grid writer, sz_remove_ghosts -- and goes on.  Nothing crosses to the host but the counters.  (Tiled contexts: below.)
//
// A FLOE FRAME is the list as add_ghosts! leaves it, in the columns the writer's mask selects.  The mask has one bit per column group of
// sz_floe_columns, in struct order (frame_bit_names below): bits 0..27 the double columns (the three tensors 4 doubles per floe), 28 id,
// 29 ghost_id, 30 status, 31 the rings (vert_off + vx + vy), 32 the ghost links (ghost_off + ghost_idx).
// THE LISTS (sz_set_floe_output_lists, opt-in per writer; sz_k_frame_lists below): the ragged members of a floe, in sections BEHIND the selected
// column sections, so that the layout of a frame without them is untouched (the move TileFrameLayout made for its keys):
//   interactions  inter_off int32 [M + 1], inter_rows double [R][7].  A parent row carries floe.interactions of the last step that ran, with the
//                 bits sz_download_interactions gives at that cut BEFORE sz_add_ghosts: the floeidx column as the reference stores it -- a partner
//                 that was an inline ghost of that step is N + the rank of its order key among that step's ghost keys + 1 (the keys are sorted on
//                 the device, or the host's fetched copy is uploaded, before sz_add_ghosts clears gi_valid and reuses the key table); where that
//                 call would translate nothing (gi_valid false: a process-mode call ran, the host uploaded the rows) the rows are kept as they
//                 are.  A ghost row's span is EMPTY whatever inter_cnt says on rows >= N: deepcopy_floe (floe_utils.jl:120-161) passes no
//                 interactions, the copy gets zeros(0, 7) and num_inters = 0.
//   subpoints     sub_off int32 [M + 1], sx [S], sy [S], centred as stored.  A parent row carries its own points with the bits of
//                 sz_download_subpoints; a ghost row its root parent's (deepcopy_floe copies them; State::parent names the row).
// status.fuse_idx has no section: it is non-empty only on a row tagged `fuse` (collisions.jl:367-368, 801-806), and a batch that honours tags
// never begins a step with such a row -- a host reads the recorded status column and knows.
// The three spare header words of a frame with lists are {lists, R, S}.
// A ghost is a deep copy of its parent (collisions.jl:881-901, floe_utils.jl:138), translated: the device keeps only the collision columns on a
// ghost row, so the pack reads every column of a ghost row from the row State::parent names -- cx, cy, the ring and ghost_id apart, which are
// the ghost's own.  A ghost row has no ghost links of its own (its ghost_off span is empty), as sz_download_floes reports it.
// Layout of a frame in the writer's arena (FrameLayout): a header of 8 x int64 {tstep, M, N, n_ring_points, n_ghost_links, 0, 0, 0}, then the
// selected sections in bit order, each padded to 8 bytes: doubles [M] or [M][4]; id, ghost_id int64 [M]; status int32 [M]; vert_off int32
// [M + 1], frame-relative (vert_off[0] == 0), vx [V], vy [V] de-interleaved; ghost_off int32 [M + 1], ghost_idx int32 [M - N] in list numbers.
// A GRID FRAME is nout * nx * ny doubles in the layout of sz_eulerian_data, in a store of max_frames frames; its timestep is kept on the host.
// Limits: 4 floe and 4 grid writers; a frame that finds no room (the arena, max_frames) is not taken: the batch ends in front of that step with
// `full` set (sz_output_frames), and no writer gets a frame of a step that not all due writers have room for.
// (sz_tile_set_floe_output_lists: a tile frame's lists lie behind its key section, sz_record_tile.hpp.)
// TILED CONTEXTS (sz_tile_set_floe_output / sz_tile_set_grid_output; the record point is tile_record in sz_tile_host.hpp, the merge of the ranks'
// frames sz_record_tile.hpp): a TILE FRAME is the same layout over the rank's own rows -- its owned parents and their ghosts, ghost_idx in local
// row numbers -- with one more section behind the selected ones, so that the layout above is untouched: key, int64 [M], the row's order key
// (State::okey: a parent's global number, a ghost's (pass << 40) + 4 * parent key + k).  The three spare header words carry {N_global, rank,
// nranks}.  The rows of all ranks sorted by key are the single context's frame of that step.
#pragma once
#include "sz_kernels.hpp"
#include "sz_columns.hpp"

namespace sz {

constexpr int REC_WRITERS = 4;
// mask bits behind the double columns
constexpr int FR_BIT_ID = MIG_NTAB, FR_BIT_GHOST_ID = FR_BIT_ID + 1, FR_BIT_STATUS = FR_BIT_ID + 2, FR_BIT_RINGS = FR_BIT_ID + 3, FR_BIT_LINKS = FR_BIT_ID + 4,
              FR_NBITS = FR_BIT_ID + 5;
// sections of a frame: the double columns, then
constexpr int FR_ID = MIG_NTAB, FR_GHOST_ID = FR_ID + 1, FR_STATUS = FR_ID + 2, FR_VOFF = FR_ID + 3, FR_VX = FR_ID + 4, FR_VY = FR_ID + 5, FR_GOFF = FR_ID + 6,
              FR_GIDX = FR_ID + 7, FR_NSEC = FR_ID + 8;
constexpr size_t FR_HEADER = 8 * sizeof(long long);
static_assert(FR_NBITS == 33, "frame mask: 28 double columns, id, ghost_id, status, rings, ghost links");
// the mask bits by name, space-separated, each with a space in front (sz_debug_frame_bits)
constexpr char FRAME_BIT_TAIL[] = " id ghost_id status rings ghost_links";

// where the sections of a frame of M rows (N parents), V ring points lie: byte offsets from the frame's start, -1 = not recorded
struct FrameLayout {
  long long off[FR_NSEC]; long long total;
  FrameLayout(unsigned long long mask, long long M, long long N, long long V) {
    long long at = (long long)FR_HEADER;
    auto take = [&](int sec, bool on, long long bytes) { off[sec] = on ? at : -1; if (on) at += (bytes + 7) & ~7ll; };
    for (int k = 0; k < MIG_NTAB; k++) take(k, mask >> k & 1, (long long)col_width(k) * M * 8);
    take(FR_ID, mask >> FR_BIT_ID & 1, M * 8); take(FR_GHOST_ID, mask >> FR_BIT_GHOST_ID & 1, M * 8); take(FR_STATUS, mask >> FR_BIT_STATUS & 1, M * 4);
    const bool rings = mask >> FR_BIT_RINGS & 1, links = mask >> FR_BIT_LINKS & 1;
    take(FR_VOFF, rings, (M + 1) * 4); take(FR_VX, rings, V * 8); take(FR_VY, rings, V * 8);
    take(FR_GOFF, links, (M + 1) * 4); take(FR_GIDX, links, (M - N) * 4);
    total = at;
  }
};

// what one launch of sz_k_frame_pack is told
struct FramePack {
  const double* col[MIG_NTAB];
  long long off[FR_NSEC];
  char* dst;                      // the frame's start in the arena
  int tstep, M, N, V;             // the host's counts behind sz_add_ghosts: every store lies inside the layout made from them
  long long key_off;              // a tile frame: where its key section lies (behind FrameLayout::total), and the three spare header words
  long long spare[3];             // {N_global, rank, nranks}
};

constexpr int FP_TPB = 256;
constexpr int FP_SLICES = MIG_NTAB + 5;      // blockIdx.y: one slice per mask bit (a tile frame: one more, the keys)

// One launch gathers a frame: slice y < MIG_NTAB double column y over all rows; then id, ghost_id, status; the rings (offsets made
// frame-relative, vxy de-interleaved); the header and the ghost links (one workgroup: the offsets are a prefix sum over the parents' counts).
// KEYED (tile frames): slice FP_SLICES copies the order keys, and the header's spare words are F.spare; nothing else differs.
template <bool KEYED>
__global__ void __launch_bounds__(FP_TPB) sz_k_frame_pack(State S, FramePack F) {
  const int y = blockIdx.y, M = F.M, N = F.N;
  const long long t0 = (long long)blockIdx.x * FP_TPB + threadIdx.x, stride = (long long)gridDim.x * FP_TPB;
  if constexpr (KEYED) {
    if (y == FP_SLICES) {
      long long* out = (long long*)(F.dst + F.key_off);
      for (long long r = t0; r < M; r += stride) out[r] = S.okey[r];
      return;
    }
  }
  auto src_row = [&](int r) { if (r < N) return r; const int p = S.parent[r]; return p >= 0 && p < N ? p : r; };
  if (y < MIG_NTAB) {
    if (F.off[y] < 0) return;
    double* out = (double*)(F.dst + F.off[y]);
    const bool own = y == COL_cx || y == COL_cy;
    if (y < MIG_NSC) for (long long r = t0; r < M; r += stride) out[r] = F.col[y][own ? (int)r : src_row((int)r)];
    else for (long long e = t0; e < 4ll * M; e += stride) out[e] = F.col[y][4ll * src_row((int)(e >> 2)) + (e & 3)];
  } else if (y == FR_BIT_ID) {
    if (F.off[FR_ID] < 0) return;
    long long* out = (long long*)(F.dst + F.off[FR_ID]);
    for (long long r = t0; r < M; r += stride) out[r] = S.id[src_row((int)r)];
  } else if (y == FR_BIT_GHOST_ID) {
    if (F.off[FR_GHOST_ID] < 0) return;
    long long* out = (long long*)(F.dst + F.off[FR_GHOST_ID]);
    for (long long r = t0; r < M; r += stride) out[r] = S.ghost_id[r];
  } else if (y == FR_BIT_STATUS) {
    if (F.off[FR_STATUS] < 0) return;
    int* out = (int*)(F.dst + F.off[FR_STATUS]);
    for (long long r = t0; r < M; r += stride) out[r] = S.status[src_row((int)r)];
  } else if (y == FR_BIT_RINGS) {
    if (F.off[FR_VOFF] < 0) return;
    int* voff = (int*)(F.dst + F.off[FR_VOFF]);
    double *vx = (double*)(F.dst + F.off[FR_VX]), *vy = (double*)(F.dst + F.off[FR_VY]);
    const int v0 = S.voff[0];
    for (long long r = t0; r <= M; r += stride) voff[r] = S.voff[r] - v0;
    for (long long p = t0; p < F.V; p += stride) { const double2 q = S.vxy[v0 + p]; vx[p] = q.x; vy[p] = q.y; }
  } else if (blockIdx.x == 0) {
    const int G = M - N, t = threadIdx.x;
    if (t == 0) {
      long long* h = (long long*)F.dst;
      h[0] = F.tstep; h[1] = M; h[2] = N; h[3] = F.V; h[4] = G;
      if constexpr (KEYED) { h[5] = F.spare[0]; h[6] = F.spare[1]; h[7] = F.spare[2]; } else h[5] = h[6] = h[7] = 0;
    }
    if (F.off[FR_GOFF] < 0) return;
    int *goff = (int*)(F.dst + F.off[FR_GOFF]), *gidx = (int*)(F.dst + F.off[FR_GIDX]);
    // thread t owns the parents [lo, hi): their counts summed, the sums scanned over the workgroup, the offsets and links written
    __shared__ int part[FP_TPB];
    const int per = (N + FP_TPB - 1) / FP_TPB, lo = min(t * per, N), hi = min(lo + per, N);
    auto count = [&](int i) { const int n = S.ngh[i]; return n < 0 ? 0 : n > MAX_GHOSTS ? MAX_GHOSTS : n; };
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += count(i);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < FP_TPB; d <<= 1) {
      const int v = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    int at = part[t] - sum;
    for (int i = lo; i < hi; i++) {
      goff[i] = at;
      const int n = count(i);
      for (int k = 0; k < n; k++, at++) if (at < G) gidx[at] = S.gh[i * MAX_GHOSTS + k];
    }
    const int tot = min(part[FP_TPB - 1], G);
    for (int r = N + t; r <= M; r += FP_TPB) goff[r] = tot;          // (a ghost row has no links; entry M closes the list)
    if (t == 0 && N == 0) goff[0] = 0;
  }
}

// ---- the lists (sz_set_floe_output_lists): which, and where their sections lie -- behind FrameLayout::total, each padded to 8 bytes
constexpr unsigned FR_LIST_INTER = 1, FR_LIST_SUB = 2, FR_LIST_ALL = 3;
// a tiled context: what the partner column of its interaction rows can be translated with (sz_ctx::tile_inter_state), and why a tile frame
// lost its interactions bit (FloeFrame::inter_lost: _LISTED, _MIGRATED)
constexpr int TILE_INTER_NONE = 0, TILE_INTER_TABLE = 1, TILE_INTER_LISTED = 2, TILE_INTER_MIGRATED = 3;
constexpr int FL_IOFF = 0, FL_IROWS = 1, FL_SOFF = 2, FL_SX = 3, FL_SY = 4, FL_NSEC = 5;
struct ListLayout {
  long long off[FL_NSEC]; long long total;          // total: the whole frame's, columns included
  ListLayout(long long base, unsigned lists, long long M, long long R, long long S) {
    long long at = base;
    auto take = [&](int sec, bool on, long long bytes) { off[sec] = on ? at : -1; if (on) at += (bytes + 7) & ~7ll; };
    const bool in = lists & FR_LIST_INTER, sub = lists & FR_LIST_SUB;
    take(FL_IOFF, in, (M + 1) * 4); take(FL_IROWS, in, R * 7 * 8);
    take(FL_SOFF, sub, (M + 1) * 4); take(FL_SX, sub, S * 8); take(FL_SY, sub, S * 8);
    total = at;
  }
};

// per row of the list behind sz_add_ghosts its interaction rows and sub-floe points (entry M: 0): what the two scans turn into offsets.
// A null pointer: that list is not wanted.
__global__ void __launch_bounds__(FP_TPB) sz_k_frame_list_counts(State S, int* n_inter, int* n_sub, int M, int N) {
  for (int r = blockIdx.x * FP_TPB + threadIdx.x; r <= M; r += gridDim.x * FP_TPB) {
    if (n_inter) n_inter[r] = r < N ? min(max(S.inter_cnt[r], 0), S.rowcap) : 0;          // (a ghost row: empty, whatever inter_cnt says there)
    if (n_sub) {
      int p = r < N ? r : -1;
      if (r >= N && r < M) { const int q = S.parent[r]; p = q >= 0 && q < N ? q : -1; }
      n_sub[r] = p >= 0 ? max(S.soff[p + 1] - S.soff[p], 0) : 0;
    }
  }
}

// what one launch of sz_k_frame_lists is told
struct FrameLists {
  char* dst;                      // the frame's start in the arena
  long long off[FL_NSEC];
  const int *ioff, *soff;         // the scanned counts, M + 1 entries each (the recorder's workspace)
  const long long* keys;          // the order keys of the last step's inline ghosts, sorted; nkeys == 0: nothing is translated
  int nkeys, M, N;
  unsigned lists;
  long long R, S;                 // the host's totals, fetched with the counters: every store lies inside the layout made from them
  int keep_spare;                 // a tile frame: the spare header words stay {N_global, rank, nranks} (its totals are kept with the frame on the host)
};

// The payload of the lists, element-parallel: blockIdx.y = 0 the interactions, one thread per output double; 1 the sub-floe points, one thread
// per point.  The owning row is found by bisection in the scanned offsets, which the same slice copies into the frame; stores are coalesced,
// reads contiguous within a row.  The floeidx column (column 0) of a row whose partner was an inline ghost holds 1 + the ghost's order key
// (> 2^40): it becomes N + rank among the sorted keys + 1, as sz_download_interactions renumbers it on the host; a key that is not among them
// stays.  No atomic decides a position: two packs of one state give the same bits.
__global__ void __launch_bounds__(FP_TPB) sz_k_frame_lists(State S, FrameLists F) {
  const int M = F.M, N = F.N;
  const long long t0 = (long long)blockIdx.x * FP_TPB + threadIdx.x, stride = (long long)gridDim.x * FP_TPB;
  if (blockIdx.y == 0) {
    if (t0 == 0 && !F.keep_spare) { long long* h = (long long*)F.dst; h[5] = F.lists; h[6] = F.R; h[7] = F.S; }
    if (F.off[FL_IOFF] < 0) return;
    int* off = (int*)(F.dst + F.off[FL_IOFF]);
    double* out = (double*)(F.dst + F.off[FL_IROWS]);
    for (long long r = t0; r <= M; r += stride) off[r] = F.ioff[r];
    const double lim = (double)((long long)1 << 40);
    for (long long e = t0; e < 7 * F.R; e += stride) {
      const long long row = e / 7; const int k = (int)(e - 7 * row);
      int lo = 0, hi = N;                         // the last parent i with ioff[i] <= row: the one that owns it (empty parents share an offset)
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (F.ioff[mid] <= row) lo = mid; else hi = mid; }
      const long long q = row - F.ioff[lo];
      double v = q >= 0 && q < S.rowcap && lo < N ? S.inter_rows[((size_t)lo * S.rowcap + (size_t)q) * 7 + k] : 0.0;
      if (k == 0 && F.nkeys > 0 && v > lim) {
        const long long key = (long long)v - 1;
        int a = 0, b = F.nkeys;                   // lower bound
        while (a < b) { const int mid = (a + b) >> 1; if (F.keys[mid] < key) a = mid + 1; else b = mid; }
        if (a < F.nkeys && F.keys[a] == key) v = (double)(N + a + 1);
      }
      out[e] = v;
    }
  } else {
    if (F.off[FL_SOFF] < 0) return;
    int* off = (int*)(F.dst + F.off[FL_SOFF]);
    double *sx = (double*)(F.dst + F.off[FL_SX]), *sy = (double*)(F.dst + F.off[FL_SY]);
    for (long long r = t0; r <= M; r += stride) off[r] = F.soff[r];
    for (long long p = t0; p < F.S; p += stride) {
      int lo = 0, hi = M;                         // the last row with soff[row] <= p
      while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (F.soff[mid] <= p) lo = mid; else hi = mid; }
      int src = lo < N ? lo : -1;
      if (lo >= N && lo < M) { const int q = S.parent[lo]; src = q >= 0 && q < N ? q : -1; }
      const long long q = src >= 0 ? (long long)S.soff[src] + (p - F.soff[lo]) : -1;
      const bool ok = src >= 0 && q >= S.soff[src] && q < S.soff[src + 1] && q < S.capS;
      sx[p] = ok ? S.sx[q] : 0.0; sy[p] = ok ? S.sy[q] : 0.0;
    }
  }
}

// host side of one writer each; the device memory is the recorder's own (hipMalloc / hipFree when a writer is set, re-set or cleared away),
// so frames outlive uploads and row edits
struct FloeFrame {
  size_t at; int tstep, M, N, V;
  std::vector<int> ranks;         // a tile frame: {M, N, V} of every rank's frame of this step, as gathered at the record point
  unsigned lists = 0; long long R = 0, S = 0;          // the lists it holds, their totals: interaction rows, sub-floe points
  // a tile frame of a writer with lists (sz_tile_set_floe_output_lists): K = the entries of its key-table section; lranks = {R, S, K} of every
  // rank's frame of this step, as gathered at the record point; inter_lost = why the interactions bit of `lists` was cleared on every rank
  // (TILE_INTER_*; 0: it was not)
  long long K = 0; std::vector<int> lranks; int inter_lost = 0;
};
struct FloeWriter {
  int dt = 0; unsigned long long mask = 0; bool tile = false;      // tile: set through sz_tile_set_floe_output
  unsigned lists = 0;             // sz_set_floe_output_lists
  char* arena = nullptr; size_t bytes = 0, used = 0;
  std::vector<FloeFrame> frames;
};
struct GridWriter {
  int dt = 0, nx = 0, ny = 0, max_frames = 0; bool tile = false;      // tile: set through sz_tile_set_grid_output
  std::vector<double> xg, yg; std::vector<int> outputs;
  double* store = nullptr;        // [max_frames][nout][nx][ny]
  std::vector<int> tsteps;
};
// one device chunk that is kept and grows on demand: the persistent workspace of the recorded averages
struct RecWork { char* p = nullptr; size_t bytes = 0; };
struct Recorder {
  FloeWriter floe[REC_WRITERS]; GridWriter grid[REC_WRITERS];
  int dts[2 * REC_WRITERS] = { 0 };          // StopRules::out_dts: floe writers, then grid writers
  bool any = false, full = false;
  bool any_tile = false, any_single = false; // ... set through the tile setters / through the single context's
  RecWork grid_work, entry_work;             // EulGrid's per-cell arrays; its entries and the sort's scratch
  RecWork list_work;                         // the lists: sorted ghost keys, counts and scanned offsets, the sort's scratch (ListWork)
  RecWork part_work;                         // tile frames: the per-cell partial sums of all grid writers due at a step, one behind the other
  std::vector<char> host;                    // a frame on its way down
  void refresh() {
    any = any_tile = any_single = false;
    for (int w = 0; w < REC_WRITERS; w++) {
      dts[w] = floe[w].dt; dts[REC_WRITERS + w] = grid[w].dt;
      any_tile = any_tile || (floe[w].dt > 0 && floe[w].tile) || (grid[w].dt > 0 && grid[w].tile);
      any_single = any_single || (floe[w].dt > 0 && !floe[w].tile) || (grid[w].dt > 0 && !grid[w].tile);
    }
    any = any_tile || any_single;
  }
};

}  // namespace sz

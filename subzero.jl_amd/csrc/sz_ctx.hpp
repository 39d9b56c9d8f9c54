// sz_ctx.hpp — the context (sz_ctx) and what every other part of the host code needs first: pooled device allocations, the error-check
// macro, launch sizing, event timing of kernel classes, the counter block and the stop words, the sync that reports sticky device errors.
// Host code of the one translation unit sz_api.hip, which includes it behind the kernel headers.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/subzero_hip.h"
#include "sz_kernels.hpp"
#include "sz_pipeline.hpp"
#include "sz_fracture.hpp"
#include "sz_weld.hpp"
#include "sz_weld_tile.hpp"
#include "sz_ridgeraft.hpp"
#include "sz_ridgeraft_tile.hpp"
#include "sz_splice.hpp"
#include "sz_record.hpp"
#include "sz_record_tile.hpp"

using namespace sz;

namespace {

constexpr int NK = SZ_K_COUNT + 2;   // + large narrow variant, + the halo exchange of a tiled step (events on the communication stream)
constexpr int K_NARROW_LARGE = SZ_K_COUNT, K_EXCHANGE = SZ_K_COUNT + 1;
struct EvPair { int k; hipEvent_t a, b; };

// Device allocations of one lifetime.  The ~130 columns and work arrays are carved out of a few large chunks
// instead of one hipMalloc each: the chunks are mapped with 2 MB fragments, so a kernel that walks 60 columns
// needs a handful of TLB entries instead of several per column.
struct Pool {
  std::vector<void*> chunks; std::vector<size_t> sizes;
  size_t ci = 0;                 // chunk being carved
  char* cur = nullptr; size_t left = 0, next = 8u << 20;
  bool empty() const { return chunks.empty(); }
  void push_back(void* q) { chunks.push_back(q); sizes.push_back(0); }      // a stand-alone allocation handed to the pool
};

}  // namespace

struct sz_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = true;
  hipStream_t stream2 = nullptr;        // forcings beside the collision kernels
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  State S{};
  Params P{};
  std::string err;
  Pool allocs;        // per-upload allocations
  Pool list_allocs;   // the lists whose capacity follows the field and GROWS on demand (grow_lists): neighbour lists, pair items, item rows
  int callid = 0;     // collision calls so far (State::callid: a call run again after its lists grew adds its overlap to floe.overarea once)
  Pool inter_allocs;  // floe.interactions (inter_cnt, inter_rows): survive an upload of the same size -- a shim uploads between
                      // timestep_collisions! and timestep_floe_properties!, and calc_stress! reads the rows of the collisions
  int inter_capM = 0, inter_rowcap = 0; bool inter_any = false, inter_lost = false;
  int nb_count_max = 0;             // bounding-circle neighbours of the most crowded floe at upload (inflated circles): sizes State::maxnb
  Pool static_allocs; // domain element table
  Pool field_allocs;  // ocean / atmosphere lattices
  bool have_floes = false, have_domain = false, have_fields = false;
  int hostM = 0, hostN = 0;
  // element table (host copy, rebuilt on set_domain / set_topography)
  int h_kinds[4] = { 0, 0, 0, 0 };
  double h_vals[4] = { 0, 0, 0, 0 }, h_rects[16] = { 0 }, h_bu[4] = { 0 }, h_bv[4] = { 0 };
  std::vector<int> h_toff; std::vector<double> h_tx, h_ty, h_tcx, h_tcy, h_trmax;
  // profiling
  unsigned pmask = 0;               // bit k: kernel class k is event-timed
  std::vector<EvPair> evs; size_t ev_used = 0;
  double kms[NK] = { 0 }; long long kl[NK] = { 0 };
  // fuse bookkeeping (status.fuse_idx lives on the host: it only changes on rare fuse events)
  std::vector<std::vector<int>> fuse_lists;
  long long* d_stats = nullptr;
  int last_dt = 0;
  bool any_moving = false;
  int overlap_forcing = -1;       // -1: by size (fp64 fields above 65 536 floes, where the forcings have a launch of their own: 0.585 -> 0.567 ms/step at 100 k; not
                                  // in mixed precision: 0.181 -> 0.187 on configs[4]); SZ_OVERLAP=0|1 forces it.  SZ_OVERLAP=1: forcings on a second stream beside the broad / narrow / reduce kernels.  The fork/join
                                  // costs ~10 us; riding in the neighbour launch (fuse_forcing) is as good or better at every size
  int max_sub = 0;                  // most sub-floe points of one floe (sizes the LDS of the two-way forcing kernel)
  int max_ring = 0, max_elem_ring = 5, max_ring_tiled = 0;   // largest ring sizes (host knowledge: which narrow variants can be needed)
  int narrow_grid0 = 0;
  // mixed precision (sz_set_precision): fp32 copies for the forcing kernel, rebuilt when their sources change
  int precision = 0; bool mixed_pts_ok = false, mixed_nodes_ok = false; Pool mixed_pt_allocs, mixed_node_allocs;
  bool blk_pts_ok = false, no_block_points = false; Pool blk_pt_allocs; int pts_N = 0;      // State::sxy (ensure_block_points); pts_N: floes whose soff entries are set (upload, migration)
  // mixed precision, geometry: fp32 broad-phase records and body-frame rings (sz_state.hpp); rings_stale: resident steps ran on the
  // body rings, the world rings vx / vy are behind (rebuilt by world_rings() before anything else looks at them)
  bool mixed_geom_ok = false, rings_stale = false; Pool mixed_geom_allocs;
  // two-way coupling (off by default, like CouplingSettings())
  bool two_way = false; int tw_dt = 10; int tw_capM = 0; size_t tw_ncell = 0; bool temps_set = false;
  Pool tw_allocs, tw_field_allocs;
  // static broad-phase grid of the resident steps (fixed by the host: no bounds reduction per step)
  // inline ghosts (sz_kernels.hpp ghost_inline_make): the resident steps make a step's ghosts in the kernel that places their parents,
  // in allocation order; the reference's ghost numbers are recovered from the order keys of the last step that ran
  bool gi_valid = false;            // the interaction rows / pair lists on the device carry order keys of inline ghosts
  std::vector<long long> gi_keys;   // order key of the ghost at storage offset k (floe N + k) in the last step that ran
  bool gi_pending = false; int gi_pending_n = 0, gi_pending_slot = 0;      // ... still to be fetched from the device (gi_fetch)
  std::vector<int> gi_ref;          // ... and its number among the ghosts in the reference's order (ghost N + gi_ref[k])
  bool retry_seen = false;          // an item has needed the largest narrow variant: sz_step enqueues it in every step from now on
  bool no_lean_narrow = false;      // SZ_LEAN_NARROW=0: always enqueue it
  double* frc_alt[4] = { nullptr, nullptr, nullptr, nullptr };      // second set of the forcing outputs fxOA, fyOA, trqOA, hflx (tiled steps with peers, see sz_tile_run)
  double2* crec_buf = nullptr;      // the records' memory (State::crec points at it only inside the batches that keep it current)
  bool crec_was_live = false;       // the last resident batch ran on records (sz_debug_crec_mismatches)
  int forcing_where = -1;           // sz_forcing_launch
  int fuse_forcing_mode = 0;        // ... 1: in the neighbour launch, 2: in the narrow launch (its tail), 0: by size -- the narrow launch while the narrow phase is one
                                    // round with a long tail (measured better up to 20 k floes, even at 40 k, worse at 65 k); SZ_FUSE_FORCING=1|2 forces one
  bool fuse_forcing = true;         // forcings inside the neighbour launch (sz_k_neighbors_forcing); SZ_FUSE_FORCING=0: own launch
  double rmax_max = 0.0, rmax_hint = 0.0; bool grid_ok = false, grid_live = false; double h_grid[8] = { 0 };
  unsigned scan_epoch = 0;      // launch counter of the look-back scans (their flags carry it: no reset pass)
  // ghost-candidate lists of the resident steps (sz_k_ghost_list): gl_cur = the list the next step consumes, gl_valid = it is
  // current (kept so by the integrator / halo unpack; any process-mode call or upload makes it stale: it is then seeded again),
  // gl_est = how long it is (host estimate at upload, device count after every batch): long lists take the two-launch path
  int gl_cur = 0; bool gl_valid = false; int gl_est = 0; bool no_ghost_list = false; int gl_max = 2048;
  // tiled runs with the exchange inside the library (sz_comm_init / sz_tile_setup / sz_tile_run): the RCCL communicator, a second
  // stream for the sends / receives (the forcings of the owned floes run beside them), the exchange buffers and their layout
  void* comm = nullptr; int comm_n = 0, comm_rank = 0;
  sz_host_transport host_tr = { nullptr, nullptr, nullptr, nullptr }; bool host_transport = false;   // sz_comm_init_host: the collectives are the host's, staged through h_send / h_recv
  std::vector<double> h_send, h_recv;
  hipStream_t comm_stream = nullptr; hipEvent_t ev_packed = nullptr, ev_recv = nullptr;
  Pool comm_allocs; double *d_send = nullptr, *d_recv = nullptr, *d_ref = nullptr, *d_gather = nullptr; int* d_dcap = nullptr;
  int halo_cap = 0; std::vector<int> cap_send, cap_recv;      // slots per peer region (stride) and what is really sent to / received from each peer
  double tile_Lx = 0, tile_Ly = 0, tile_margin = 0; int tile_per_x = 0, tile_per_y = 0, tile_rebox_every = 50, tile_since_box = -1, tile_rebox_cur = 8, tile_dt = 0; bool tile_rebox_fixed = false;    // rebox_cur: the gather interval in use (<= rebox_every, from the measured drift)
  Pool tw_part_allocs; double* d_tw_partial = nullptr;
  Pool mig_allocs;                  // scratch of sz_tile_migrate (streams, directory, the gathered rows): kept between migrations
  Pool sub_allocs;                  // sub-floe points of a tile that outgrew State::capS in a migration (sz_tile_migrate): until the next upload
  int upload_M = 0, upload_V = 0;   // floes and ring points of the last sz_upload_floes (what its capacities were carved for)
  int migrate_path = 0;             // how the last sz_tile_migrate ran: 1 packed on the device, 2 staged through the host (sz_debug_migrate_path)
  std::vector<long long> tile_gidx; // global index of every owned floe (sz_tile_enable): status.fuse_idx of a tiled context is reported in global numbers
  bool tile_hdr_neighbours = false; // SZ_TILE_HEADERS=neighbours (measurement only, batches that run through): the inline steps trade with the neighbouring tiles only --
                                    // no header record to the others, hence no tag stop and no pause agreement in that arm (the largest narrow variant stays in)
  double tile_box_ctr[2] = { 0, 0 }; bool tile_box_valid = false;   // centre of this rank's owned box at the last gather (sz_k_owned_box: periodic images)
  int tile_forcing_tstep = -1;      // timestep whose forcings sz_tile_forcing has already enqueued
  bool tile_dirty = false;      // ghosts / halo floes of the last sz_tile_step still appended
  // fixed-point totals (State::facc): resident batches only.  acc_mode: what the integrator is told (bit 0: totals / stress sums / tags from facc,
  // bit 1: the batch's last step); reduce_mode: 0 sz_k_inter_fill does everything inside the step (process mode), 1 it only assembles rows inside
  // the step, 2 it is left out of the steps and runs once behind the batch (the reduce-free steps)
  long long* facc_buf = nullptr; int acc_mode = 0, reduce_mode = 0;
  int last_totals_mode = 0;         // reduce_mode of the last sz_step batch (sz_debug_totals_mode)
  // pipelined resident steps (sz_pipeline.hpp): the second set of what is double-buffered by step parity.  pb[0] is what the upload carved
  // (State::vxy, crec_buf, the cell lists, the work list, the ghost links), pb[1] its twin; gpar: the set that holds the context's state -- c->S
  // points at pb[gpar]'s buffers, the records apart: State::crec is a batch mode, the set's records are crec_buf (own_set_carved, pipe_adopt).
  StepSet pb[2] = {};
  int gpar = 0;
  bool no_pipeline = false;         // SZ_PIPELINE=0: the three-launch steps (A/B)
  int pipe_min_steps = 4;           // batches shorter than this take the three-launch steps (a pipelined batch has a prologue and an epilogue)
  int pipe_max_floes = 60000;       // larger fields keep the three-launch steps: they are throughput-bound, nothing idles beside the narrow phase (measured at 100 k: 0.486 against 0.476 ms; SZ_PIPE_MAX_FLOES)
  int last_pipelined = 0;           // the last sz_step batch ran pipelined (sz_debug_pipelined)
  bool crec_current = false;        // the collision records of set gpar hold the parents as they lie (a pipelined batch left them so; any call that moves or
                                    // re-uploads floes outside such a batch clears it) and the twin set has the static quads: the next batch seeds neither
  // fracture criterion (sz_set_fracture; sz_fracture.hpp): kind SZ_FRAC_*, FractureSettings.Δt, the device block and the per-parent buffers
  int frac_kind = 0, frac_dt = 0, frac_npts = 0, frac_cap = 0;
  double frac_pstar = 0, frac_c = 0, frac_alpha = 0, frac_min_area = 0;
  FracDev* frac_d = nullptr; unsigned char* frac_flag = nullptr; int* frac_idx = nullptr;
  Pool frac_allocs;                 // scratch of a tiled context's collective criterion pass (tile_frac_pass; sz_fracture_tile.hpp): kept between passes
  int tile_stop_raised = 0;         // the batch-relative stop step the last tile driver ended with (0: none): the list-based driver's is THIS rank's own word -- a tag of its
                                    // last step is not yet known to the peers --, the inline driver's is already the ranks' agreed one (comm_agree_steps)
  std::vector<int> frac_cnt;        // owned counts of all ranks of the last criterion pass (the source of an asynchronous upload: outlives the call)
  // welding (sz_set_welding; sz_weld.hpp): WeldSettings' Δts / Nxs / Nys in the reference's order and max_weld_area; the buffers of the overlap-table
  // pass (its own search cells, bins, pair keys, areas, table), carved for weld_capN parents, weld_cells cells and weld_cap pairs
  std::vector<int> weld_dts, weld_nxs, weld_nys; double weld_max_area = 0;
  Pool weld_allocs; int weld_capN = 0, weld_cells = 0, weld_cap = 0; void* weld_tmp = nullptr; size_t weld_tmp_bytes = 0;
  WeldArgs weld{}; int *weld_cell_cnt = nullptr, *weld_cell_slots = nullptr, *weld_cell_ovf = nullptr, *weld_cell_items = nullptr; double* weld_bounds = nullptr;
  WeldDev weld_h{}; double weld_h_grid[8] = { 0 };          // host sides of the two small uploads of a pass
  int weld_npairs = 0;              // candidate pairs of the last pass (sz_debug_weld_npairs)
  // ... on a tiled context (tile_weld_pass; sz_weld_tile.hpp): the scratch of the collective pass, kept between passes; the pair capacity a pass
  // that ran out asked for; the host sides of its small transfers; the whole table in global numbers, as every rank ends a pass with it
  Pool weldt_allocs; int weldt_need = 0, weldt_npairs = 0; int* weldt_bin = nullptr;
  WeldTileDev weldt_h{}; WeldDev weldt_hw{}; double weldt_h_grid[8] = { 0 }; std::vector<int> weldt_cnt;
  std::vector<long long> weldt_i, weldt_j; std::vector<double> weldt_a;
  // removal (sz_set_removal; sz_remove.hpp): SimplificationSettings.max_vertices (INT32_MAX: smoothing off) and FloeSettings' minimum area / height;
  // the running ocean.dissolved lattice (with the fields: zero after sz_set_fields); per parent the row it had at the last sz_upload_floes
  bool rm_on = false; int rm_max_vertices = 0x7fffffff; double rm_min_area = 0, rm_min_height = 0;
  double* dissolved = nullptr; int* origin = nullptr; Pool rm_allocs;
  Pool sp_allocs;                   // scratch of sz_download_rows / sz_download_list_rows / sz_splice_floes / sz_splice_parents (sz_splice.hpp) and of sz_ridgeraft_rows: the staged rows, the plan, the gathered rows, the closure's flags; kept between calls
  Pool spt_allocs;                  // scratch of sz_tile_download_rows / sz_tile_splice_floes in front of that (sz_splice_tile.hpp): the names, their rows, the ranks' records; kept between calls
  // ridge / raft (sz_set_ridgeraft; sz_ridgeraft.hpp): RidgeRaftSettings' Δt and the five heights the gates read; the buffers of the candidate pass,
  // carved for rr_capM list rows and rr_cap entries.  rr_pending: the timestep whose ridge / raft step stopped between timestep_collisions! and
  // timestep_ridging_rafting! (-1: none; sz_step_finish runs its second half); rr_draws: the per-floe draws of the ridge / raft steps the last
  // sz_step ran through with an empty table.  ghosts_staged / rr_rows: the list is as add_ghosts! leaves it, and floe.interactions is of that
  // list (a collision call, sz_upload_interactions) -- what the pass may be asked on
  bool rr_on = false; int rr_dt = 0; double rr_h[5] = { 0, 0, 0, 0, 0 };
  Pool rr_allocs; RrArgs rr{}; int rr_capM = 0, rr_cap = 0; RrDev rr_hd{};
  int rr_pending = -1; long long rr_draws = 0; bool ghosts_staged = false, rr_rows = false;
  // ... on a tiled context (tile_rr_pass; sz_ridgeraft_tile.hpp): the scratch of the collective pass, kept between passes; the host sides of its
  // small transfers; the whole table in the single context's list numbers, as every rank ends a pass with it, the list number and the order key of every local
  // row of that pass (sz_tile_list_numbers, sz_tile_list_keys), and the draws of all ranks.  tile_split_gl: the first half of a split step took the ghost-candidate list
  Pool rrt_allocs; RrDev rrt_hd{}; RrTileDev rrt_hg{}; int rrt_hw[4] = { 0, 0, 0, 0 }, rrt_hbad = 0; std::vector<int> rrt_cnt;
  std::vector<long long> rrt_i, rrt_j, rrt_rownum, rrt_rowkey; std::vector<int> rrt_k; std::vector<double> rrt_f;
  bool tile_split_gl = false;
  // output recorder (sz_set_floe_output / sz_set_grid_output; sz_record.hpp): the writers, their frames in HBM, the workspace of the averages
  Recorder rec;
  Pool rect_allocs;                 // scratch of sz_tile_download_floe_frame (sz_record_tile.hpp): the gathered slots, the sort's arrays, the merged frame; kept between calls
  // tile frames with lists (sz_tile_set_floe_output_lists): what the partner column of floe.interactions on this tile can be translated with.
  // TILE_INTER_NONE: the rows are as placed (an upload: nothing to translate); _TABLE: the last step was an inline tile step, its order keys are
  // tile_keys_n entries of S.gkeys' half tile_keys_slot; _LISTED: it was a list-based tile step (sz_tile_step, a ridge / raft step), whose key
  // table nobody keeps; _MIGRATED: sz_tile_migrate dropped the rows.  Set by the migration and by every collision step of a tile.
  int tile_inter_state = 0, tile_keys_n = 0, tile_keys_slot = 0;
  bool last_stopped = false;        // the last batch of resident steps ended on a stop request (tag, fracture candidate), not at its last step
  bool maybe_tagged = false;        // a parent may be non-active on the device (an upload said so, a batch ended on a tag, a process-mode call ran):
                                    // the next batch then runs its first step on its own (see sz_step)
  int last_err_bits = 0;   // device error bits the last sync_and_check found (tiled runs agree on them between the ranks)
  int dbg = 0;   // SZ_DEBUG: read by the narrow kernel of a -DSZ_STAMPS build only (dbg >> 8: the workgroup it stamps, bit 16: its first round twice)
};

namespace {

#define HIPCHK(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                  \
      return SZ_E_HIP;                                                                 \
    }                                                                                  \
  } while (0)

template <typename T>
int dalloc(sz_ctx* c, T** p, size_t n, Pool& pool) {
  const size_t bytes = (((n ? n : 1) * sizeof(T)) + 255) & ~(size_t)255;
  if (bytes > pool.left) {
    // a chunk kept from before the last reset_pool() that is large enough comes first (an upload of the same sizes
    // as the previous one then allocates nothing)
    size_t k = pool.cur ? pool.ci + 1 : 0;
    while (k < pool.chunks.size() && pool.sizes[k] < bytes) {      // too small now: will not fit later either
      (void)hipFree(pool.chunks[k]); pool.chunks.erase(pool.chunks.begin() + k); pool.sizes.erase(pool.sizes.begin() + k);
    }
    if (k < pool.chunks.size()) { pool.ci = k; pool.cur = (char*)pool.chunks[k]; pool.left = pool.sizes[k]; }
    else {
      const size_t chunk = std::max(bytes, pool.next);
      void* q = nullptr;
      HIPCHK(c, hipMalloc(&q, chunk));
      pool.chunks.push_back(q); pool.sizes.push_back(chunk); pool.ci = pool.chunks.size() - 1; pool.cur = (char*)q; pool.left = chunk;
      if (pool.next < ((size_t)256 << 20)) pool.next *= 2;
    }
    // allocations are handed out zeroed: one fill per chunk instead of one per array (~130 launches per upload)
    HIPCHK(c, hipMemsetAsync(pool.cur, 0, pool.left, c->stream));
  }
  void* q = pool.cur; pool.cur += bytes; pool.left -= bytes;
  *p = (T*)q;
  return SZ_OK;
}
void free_pool(Pool& pool) { for (void* p : pool.chunks) (void)hipFree(p); pool.chunks.clear(); pool.sizes.clear(); pool.ci = 0; pool.cur = nullptr; pool.left = 0; pool.next = 8u << 20; }
// forget the allocations, keep the memory for the next round of dalloc()s
void reset_pool(Pool& pool) { pool.ci = 0; pool.cur = nullptr; pool.left = 0; }
// after a round: chunks the round did not reach go back to the driver
void trim_pool(Pool& pool) {
  const size_t keep = pool.cur ? pool.ci + 1 : 0;
  for (size_t k = keep; k < pool.chunks.size(); k++) (void)hipFree(pool.chunks[k]);
  pool.chunks.resize(keep); pool.sizes.resize(keep);
}

struct PoolGuard { Pool v; PoolGuard() { v.next = 1u << 16; } ~PoolGuard() { free_pool(v); } };

inline int grid_for(long long n, int tpb, int maxb = 4096) {
  long long b = (n + tpb - 1) / tpb;
  if (b < 1) b = 1;
  if (b > maxb) b = maxb;
  return (int)b;
}
// timestep tstep computes the forcings (a coupling step)
inline bool coupling_at(int flags, int coupling_dt, int tstep) { return (flags & SZ_COUPLING_ON) && coupling_dt > 0 && (tstep % coupling_dt) == 0; }

struct Timed {   // RAII-free helper: begin/end a timed kernel class
  sz_ctx* c; int k; size_t idx = (size_t)-1; hipStream_t st;
  Timed(sz_ctx* c_, int k_, hipStream_t st_ = nullptr) : c(c_), k(k_), st(st_ ? st_ : c_->stream) {
    if (!(c->pmask >> k & 1u)) return;
    if (c->ev_used == c->evs.size()) {
      EvPair e; e.k = k; (void)hipEventCreate(&e.a); (void)hipEventCreate(&e.b); c->evs.push_back(e);
    }
    idx = c->ev_used++;
    c->evs[idx].k = k;
    (void)hipEventRecord(c->evs[idx].a, st);
  }
  void end() { if (idx != (size_t)-1) (void)hipEventRecord(c->evs[idx].b, st); }
};
void resolve_events(sz_ctx* c) {
  for (size_t i = 0; i < c->ev_used; i++) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, c->evs[i].a, c->evs[i].b) == hipSuccess) { c->kms[c->evs[i].k] += ms; c->kl[c->evs[i].k] += 1; }
  }
  c->ev_used = 0;
}

// after tiled steps: forget the ghosts and halo floes of the last one (simulation.jl:138-144; N := owned)
void tile_cleanup(sz_ctx* c) {
  if (!c->tile_dirty) return;
  hipLaunchKernelGGL(sz_k_remove_ghosts, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, 1);
  c->tile_dirty = false;
}
// the counter block as the stream leaves it: copied behind everything enqueued so far, and waited for
int fetch_counters(sz_ctx* c, int* h) {
  HIPCHK(c, hipMemcpyAsync(h, c->S.cnt, C_COUNT * sizeof(int), hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
// The words through which the kernels of a resident batch end or pause it (sz_state.hpp), cleared between (sub-)batches: one memset per word
// of the mask, in the order of the list below
constexpr unsigned W_STOP = 1u << C_STOP, W_RETRYSTOP = 1u << C_RETRYSTOP, W_PAUSED = 1u << C_PAUSED, W_FRCSTOP = 1u << C_FRCSTOP;
hipError_t clear_stop_words(sz_ctx* c, unsigned mask) {
  hipError_t e = hipSuccess;
  for (int w : { C_STOP, C_RETRYSTOP, C_PAUSED, C_FRCSTOP }) if (e == hipSuccess && (mask >> w & 1u)) e = hipMemsetAsync(c->S.cnt + w, 0, sizeof(int), c->stream);
  return e;
}
int sync_and_check(sz_ctx* c, int* cnt_out = nullptr) {
  tile_cleanup(c);
  int h[C_COUNT];
  if (int rc = fetch_counters(c, h)) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream2));
  if (c->pmask) resolve_events(c);
  c->hostM = h[C_M]; c->hostN = h[C_N];
  if (cnt_out) memcpy(cnt_out, h, sizeof(h));
  c->last_err_bits = h[C_ERR];
  if (h[C_ERR]) {
    char buf[400];
    snprintf(buf, sizeof(buf),
             "device capacity/consistency error bits 0x%x (ring=1 crossings=2 regions=4 rows=8 trace=16 neighbours=32 "
             "pairs=64 elems=128 inter=256 floes=512 verts=1024 cells=2048 ghosts/parent=4096 scan=8192 halo-drift=16384 fixed-point-range=32768)", h[C_ERR]);
    c->err = buf;
    if (h[C_ERR] & ERR_CAP_CELLS)
      c->err += "; cells: the sub-floe points of one floe fall into more than " + std::to_string(FC_CAP) + " distinct centre cells, or number more than the forcing kernel stages per floe";
    int z = 0; (void)hipMemcpy(c->S.cnt + C_ERR, &z, sizeof(int), hipMemcpyHostToDevice);
    return SZ_E_CAPACITY;
  }
  return SZ_OK;
}

}  // namespace

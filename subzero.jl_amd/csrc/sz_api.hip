// sz_api.hip — the one translation unit of the library: uploads and downloads, launch orchestration, the single context's batch drivers and
// passes, and the extern "C" boundary declared in include/subzero_hip.h.  The context and its allocations are sz_ctx.hpp, the channel
// between ranks sz_comm.hpp, everything tiled sz_tile_host.hpp.  Host code is plumbing; the arithmetic is in sz_kernels.hpp / sz_geom.hpp.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/subzero_hip.h"
#include "sz_kernels.hpp"
#include "sz_pipeline.hpp"
#include "sz_twoway.hpp"
#include "sz_output.hpp"
#include "sz_migrate.hpp"
#include "sz_fracture.hpp"
#include "sz_weld.hpp"
#include "sz_ridgeraft.hpp"
#include "sz_remove_tile.hpp"
#include "sz_fracture_tile.hpp"
#include "sz_weld_tile.hpp"
#include "sz_ridgeraft_tile.hpp"
#include "sz_splice.hpp"
#include "sz_splice_tile.hpp"
#include "sz_stops.hpp"
#include "sz_record.hpp"
#include "sz_fxdebug.hpp"
#include <rocprim/rocprim.hpp>      // device radix sort of the output-grid entries (sz_eulerian_data)
#include "sz_ctx.hpp"
#include "sz_comm.hpp"

namespace {

// exclusive scan of in[0..n) into out[0..n], n = cnt[ci] + add; total also to cnt[co]
constexpr int SCAN_ONE_MAX = 1 << 13;     // up to here a scan is one single-workgroup launch instead of three (measured: wins below ~5k floes)
void scan(sz_ctx* c, const int* in, int* out, int cap, int ci, int add, int co) {
  if (cap <= SCAN_ONE_MAX) { hipLaunchKernelGGL(sz_k_scan_one, dim3(1), dim3(SCAN_B), 0, c->stream, in, out, c->S.cnt, ci, add, co); return; }
  int nb = grid_for(cap, SCAN_B, 1 << 20);
  hipLaunchKernelGGL(sz_k_scan1, dim3(nb), dim3(SCAN_B), 0, c->stream, in, out, c->S.blk, c->S.cnt, ci, add);
  hipLaunchKernelGGL(sz_k_scan2, dim3(1), dim3(SCAN_B), 0, c->stream, c->S.blk, c->S.cnt, ci, add);
  hipLaunchKernelGGL(sz_k_scan3, dim3(nb), dim3(SCAN_B), 0, c->stream, in, out, c->S.blk, c->S.cnt, ci, add, co);
}
// collision records of the first n floes of T from their columns (State::crec must point at the records)
void seed_records(sz_ctx* c, const State& T, int n) { hipLaunchKernelGGL(sz_k_crec_seed, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, T, n); }

// ---------------------------------------------------------------- lists that follow the field
// floe.interactions (rows at a stride of State::rowcap per floe): kept across an upload of the same size (see sz_upload_floes)
int carve_interactions(sz_ctx* c) {
  State& S = c->S;
  if (c->inter_capM != S.capM || c->inter_rowcap != S.rowcap || c->inter_allocs.empty()) {
    free_pool(c->inter_allocs);
    int rc;
    if ((rc = dalloc(c, &S.inter_cnt, (size_t)S.capM + 1, c->inter_allocs))) return rc;
    if ((rc = dalloc(c, &S.inter_rows, (size_t)S.capM * S.rowcap * 7, c->inter_allocs))) return rc;
    HIPCHK(c, hipMemsetAsync(S.inter_cnt, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
    c->inter_capM = S.capM; c->inter_rowcap = S.rowcap; c->inter_lost = c->inter_any; c->inter_any = false;
  }
  return SZ_OK;
}
// members of the parity set were carved into c->S: the context's own set follows (c->S is set gpar's; the set's records are crec_buf)
void own_set_carved(sz_ctx* c) { StepSet& B = c->pb[c->gpar]; step_set_copy(B, c->S); B.crec = c->crec_buf; }
// neighbour lists (stride State::maxnb), the narrow phase's work list and the rows of its items (State::capPairs)
int carve_lists(sz_ctx* c) {
  State& S = c->S;
  StepSet& twin = c->pb[1 - c->gpar];
  reset_pool(c->list_allocs);
  int rc;
#define DL(field, n) if ((rc = dalloc(c, &S.field, (size_t)(n), c->list_allocs))) return rc
  DL(nb_out, (size_t)S.capM * S.maxnb); DL(nb_in, (size_t)S.capM * S.maxnb);
  DL(work, 2 * ((size_t)S.capPairs + NSEG)); DL(wq, NSEG * 32); DL(pair_i, S.capPairs); DL(pair_j, S.capPairs);
  if ((rc = dalloc(c, &twin.work, 2 * ((size_t)S.capPairs + NSEG), c->list_allocs)) || (rc = dalloc(c, &twin.wq, (size_t)NSEG * 32, c->list_allocs))) return rc;
  own_set_carved(c);
  DL(it_rows, ((size_t)S.capPairs + S.capElem) * ROWS_PER_ITEM * 5); DL(it_info, (size_t)S.capM * S.maxnb + S.capElem + 1);
#undef DL
  trim_pool(c->list_allocs);
  HIPCHK(c, hipMemsetAsync(S.wq, 0, NSEG * 32 * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(twin.wq, 0, NSEG * 32 * sizeof(int), c->stream));
  return SZ_OK;
}
// The reference's lists grow as needed (collisions.jl:290-296: vcat; the Dict of the pair loop).  A call / step that outgrew a list has
// raised the matching error bit (and, inside a resident batch, paused the batch before anything of the floes' state changed): the lists
// are carved again with the next capacity and the caller runs the call / step again.  growable: nothing but list capacities overflowed.
constexpr int GROW_BITS = ERR_CAP_NEIGH | ERR_CAP_PAIRS | ERR_CAP_INTER;
bool growable(int bits) { return bits != 0 && (bits & ~GROW_BITS) == 0; }
int grow_lists(sz_ctx* c, int bits) {
  State& S = c->S;
  int maxnb = S.maxnb, rowcap = S.rowcap; long long capPairs = S.capPairs;
  if (bits & ERR_CAP_NEIGH) {
    if (maxnb >= 256) { c->err = "a floe has more than 256 bounding-circle neighbours in one direction: beyond the engine's largest neighbour capacity"; return SZ_E_CAPACITY; }
    maxnb = maxnb <= MAXNB ? 64 : 256;
    rowcap = std::max(rowcap, maxnb <= 64 ? 128 : 512);
    capPairs = std::max(capPairs, (long long)S.capM * 16);
  }
  if (bits & ERR_CAP_INTER) rowcap *= 4;
  if (bits & ERR_CAP_PAIRS) capPairs *= 2;
  const double bytes = (double)S.capM * maxnb * 16.0 + (double)capPairs * (16.0 + 8.0 + ROWS_PER_ITEM * 40.0) + (double)S.capM * rowcap * 56.0;
  if (rowcap > 8192 || capPairs > (1LL << 30) || bytes > 64e9) { c->err = "the lists a step needs have outgrown 64 GB (neighbours / pair items / interaction rows per floe)"; return SZ_E_CAPACITY; }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (getenv("SZ_VERBOSE")) fprintf(stderr, "[subzero-hip] lists grow (bits 0x%x): neighbours %d -> %d, rows per floe %d -> %d, pair items %d -> %lld\n", bits, S.maxnb, maxnb, S.rowcap, rowcap, S.capPairs, capPairs);
  S.maxnb = maxnb; S.rowcap = rowcap; S.capPairs = (int)capPairs;
  int rc = carve_lists(c);
  if (!rc) rc = carve_interactions(c);
  if (!rc) HIPCHK(c, hipMemsetAsync(S.inter_cnt, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
  c->inter_lost = false;             // (the call that is run again provides the rows)
  return rc;
}
// The rows of a batch's last step, assembled behind the batch, outgrew the stride (ERR_CAP_INTER alone; the device word is clear): only the
// rows' memory grows (collisions.jl:290-296) and that launch runs again, on the State `rows` builds -- after the carve, which moves inter_cnt /
// inter_rows.  h: the counter block of the last try.
template <typename RowsState>
int regrow_rows(sz_ctx* c, int* h, RowsState rows) {
  for (int tries = 0; tries < 6; tries++) {
    c->S.rowcap *= 4;
    if (c->S.rowcap > 8192) { c->err = "a floe has more than 8192 interaction rows"; return SZ_E_CAPACITY; }
    if (int rc = carve_interactions(c)) return rc;
    c->inter_lost = false;
    const State R = rows();
    hipLaunchKernelGGL(sz_k_inter_fill, dim3(grid_for(R.capM, 128 / IF_G, 16384)), dim3(128), 0, c->stream, R, 1, c->hostN, 0, 1, 1);
    const int rc = sync_and_check(c, h);
    if (!(rc == SZ_E_CAPACITY && c->last_err_bits == ERR_CAP_INTER)) return rc;
  }
  return SZ_E_CAPACITY;
}

// ---------------------------------------------------------------- element table upload
int upload_elements(sz_ctx* c) {
  free_pool(c->static_allocs);
  State& S = c->S;
  int ntopo = (int)c->h_toff.size() > 0 ? (int)c->h_toff.size() - 1 : 0;
  int ne = 4 + ntopo;
  std::vector<int> eoff(ne + 1), ekind(ne), edir(ne);
  std::vector<double> ex, ey, eval(ne), eu(ne), ev(ne), ecx(ne), ecy(ne), erm(ne), erect(16);
  eoff[0] = 0;
  for (int k = 0; k < 4; k++) {
    const double* r = c->h_rects + 4 * k;   // xmin, xmax, ymin, ymax
    // _make_bounding_box_polygon, floe_utils.jl:104-108
    double px[5] = { r[0], r[0], r[1], r[1], r[0] }, py[5] = { r[2], r[3], r[3], r[2], r[2] };
    for (int q = 0; q < 5; q++) { ex.push_back(px[q]); ey.push_back(py[q]); }
    eoff[k + 1] = (int)ex.size();
    ekind[k] = c->h_kinds[k]; edir[k] = k; eval[k] = c->h_vals[k]; eu[k] = c->h_bu[k]; ev[k] = c->h_bv[k];
    ecx[k] = ecy[k] = erm[k] = 0.0;
    for (int q = 0; q < 4; q++) erect[4 * k + q] = r[q];
  }
  for (int t = 0; t < ntopo; t++) {
    for (int q = c->h_toff[t]; q < c->h_toff[t + 1]; q++) { ex.push_back(c->h_tx[q]); ey.push_back(c->h_ty[q]); }
    int e = 4 + t;
    eoff[e + 1] = (int)ex.size();
    ekind[e] = SZ_COLLISION; edir[e] = -1; eval[e] = 0.0; eu[e] = ev[e] = 0.0;
    ecx[e] = c->h_tcx[t]; ecy[e] = c->h_tcy[t]; erm[e] = c->h_trmax[t];
  }
  S.nelem = ne;
  c->max_elem_ring = 5;
  for (int e = 0; e < ne; e++) c->max_elem_ring = std::max(c->max_elem_ring, eoff[e + 1] - eoff[e]);
  int rc;
  if ((rc = dalloc(c, &S.eoff, ne + 1, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ex, ex.size(), c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ey, ey.size(), c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ekind, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.edir, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.eval, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.eu, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ev, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ecx, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ecy, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ermax, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.erect, 16, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.eosign, ne, c->static_allocs))) return rc;
  if ((rc = dalloc(c, &S.ebb, 4 * ne, c->static_allocs))) return rc;
#define H2D(dst, src, n, T) HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)(n) * sizeof(T), hipMemcpyHostToDevice, c->stream))
  H2D(S.eoff, eoff.data(), ne + 1, int); H2D(S.ex, ex.data(), ex.size(), double); H2D(S.ey, ey.data(), ey.size(), double);
  H2D(S.ekind, ekind.data(), ne, int); H2D(S.edir, edir.data(), ne, int); H2D(S.eval, eval.data(), ne, double);
  H2D(S.eu, eu.data(), ne, double); H2D(S.ev, ev.data(), ne, double); H2D(S.ecx, ecx.data(), ne, double);
  H2D(S.ecy, ecy.data(), ne, double); H2D(S.ermax, erm.data(), ne, double); H2D(S.erect, erect.data(), 16, double);
  hipLaunchKernelGGL(sz_k_elem_osign, dim3(1), dim3(256), 0, c->stream, S);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  S.any_periodic_ew = c->h_kinds[SZ_EAST] == SZ_PERIODIC && c->h_kinds[SZ_WEST] == SZ_PERIODIC;
  S.any_periodic_ns = c->h_kinds[SZ_NORTH] == SZ_PERIODIC && c->h_kinds[SZ_SOUTH] == SZ_PERIODIC;
  S.any_domain_work = ntopo > 0;
  c->any_moving = false;
  for (int k = 0; k < 4; k++) { if (c->h_kinds[k] != SZ_PERIODIC) S.any_domain_work = 1; if (c->h_kinds[k] == SZ_MOVING) c->any_moving = true; }
  c->have_domain = true;
  return SZ_OK;
}

// launch number of the look-back scans; when the counter would no longer fit beside the status bits the flags
// are cleared once and it starts over
unsigned next_epoch(sz_ctx* c) {
  if (++c->scan_epoch >= (1u << 30)) {
    (void)hipMemsetAsync(c->S.lb_flag, 0, ((size_t)c->S.capM / SCAN_B + 8) * sizeof(unsigned), c->stream);
    c->scan_epoch = 1;
  }
  return c->scan_epoch;
}

// Grid for the resident steps: the domain box cut into cells of at least 2 max(rmax) (so that touching circles
// are in adjacent cells), indices wrapped in a periodic direction and clamped otherwise (sz_kernels.hpp, GridGeo).
void setup_grid(sz_ctx* c) {
  c->grid_ok = false; c->grid_live = false;
  const double rm = std::max(c->rmax_max, c->rmax_hint);
  if (!c->have_domain || !c->have_floes || !(rm > 0.0)) return;
  const double x0 = c->h_vals[3], xf = c->h_vals[2], y0 = c->h_vals[1], yf = c->h_vals[0];     // W, E, S, N
  if (!(xf > x0) || !(yf > y0)) return;
  // cells a hair wider than 2 max(rmax): a floe binned one cell off by round-off at a cell edge (e.g. a parent
  // wrapped by exactly one domain length after it was binned) still meets every floe whose circle touches its own
  const double cmin = 2.0 * rm * (1.0 + 1e-9);
  long long ncx = std::max(1LL, (long long)std::floor((xf - x0) / cmin));
  long long ncy = std::max(1LL, (long long)std::floor((yf - y0) / cmin));
  while (ncx * ncy > (long long)c->S.capCells) { ncx = std::max(1LL, ncx / 2); ncy = std::max(1LL, ncy / 2); }
  double* g = c->h_grid;
  g[0] = x0; g[1] = y0; g[2] = (xf - x0) / (double)ncx; g[3] = (yf - y0) / (double)ncy; g[4] = (double)ncx; g[5] = (double)ncy;
  g[6] = c->S.any_periodic_ew ? 1.0 : 0.0; g[7] = c->S.any_periodic_ns ? 1.0 : 0.0;
  c->grid_ok = true;
}
// make the static grid the live one (a process-mode call may have fitted a grid to the centroids meanwhile)
void use_static_grid(sz_ctx* c) {
  if (c->grid_live) return;
  (void)hipMemcpyAsync(c->S.bounds, c->h_grid, 8 * sizeof(double), hipMemcpyHostToDevice, c->stream);
  (void)hipMemsetAsync(c->S.cell_cnt, 0, ((size_t)c->S.capCells + 1) * sizeof(int), c->stream);
  (void)hipMemsetAsync(c->S.cell_ovf, 0, ((size_t)c->S.capCells + 1) * sizeof(int), c->stream);
  hipLaunchKernelGGL(sz_k_cell_build, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, 1);
  c->grid_live = true;
}

// resident steps of mixed precision run on body-frame rings: the world rings are rebuilt before anything else looks at them
void world_rings(sz_ctx* c) {
  if (!c->rings_stale) return;
  hipLaunchKernelGGL(sz_k_world_rings, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S);
  c->rings_stale = false;
}
// every call outside the resident steps: the candidate list they keep goes stale, the world rings must be current
void leave_resident(sz_ctx* c) { c->gl_valid = false; c->S.famrec = 0; c->crec_current = false; world_rings(c); }
// The per-batch modes of State and sz_ctx (what a resident batch's kernels are told about the batch they run in) for the life of one batch
// driver, sz_step or sz_tile_run: the batch starts from their process-mode values, and every way out of it -- early returns and HIPCHK
// included -- puts them back.  What is meant to outlive a batch (candidate lists, records, pending ghost keys, tags) is no mode.
struct BatchModes {
  sz_ctx* c;
  explicit BatchModes(sz_ctx* c_) : c(c_) { clear(); }
  ~BatchModes() { clear(); }
  BatchModes(const BatchModes&) = delete;
  BatchModes& operator=(const BatchModes&) = delete;
  void clear() {
    State& S = c->S;
    S.step = 0; S.retry_stop = 0; S.stop_on_tags = 0; S.restart_on_tags = 0; S.ginline = 0; S.famrec = 0; S.body_rings = 0;
    S.crec = nullptr; S.facc = nullptr; S.goff = 0; S.gcap = 0; S.pipe = 0;
    c->acc_mode = 0; c->reduce_mode = 0;
  }
};

// the candidate list of the coming step, seeded from the parents as they lie
void use_ghost_list(sz_ctx* c) {
  if (c->gl_valid) return;
  (void)hipMemsetAsync(c->S.cnt + C_NGCAND, 0, 2 * sizeof(int), c->stream);
  c->gl_cur = 0;
  hipLaunchKernelGGL(sz_k_ghost_seed, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, 0);
  c->gl_valid = true;
}
// inline ghosts: those of the step that starts a batch (or starts it again) from the parents as they lie, in allocator `slot`
int reseed_inline_ghosts(sz_ctx* c, int slot) {
  HIPCHK(c, hipMemsetAsync(c->S.galloc, 0, 32 * sizeof(unsigned long long), c->stream));
  c->S.gslot = slot;
  hipLaunchKernelGGL(sz_k_ghost_inline_seed, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, slot, c->hostN);
  return SZ_OK;
}
bool ghost_list_wanted(const sz_ctx* c, bool sg) {
  // (the list pass gives a parent one wavefront lane per ring point: rings of up to 64 points)
  return sg && !c->no_ghost_list && (c->S.any_periodic_ew || c->S.any_periodic_ns) && c->gl_est <= c->gl_max && c->max_ring <= 64;
}

// ---------------------------------------------------------------- pipeline stages
// in_step: the previous step's ghosts are dropped by the flag kernel and the commit is done by
// the bounds kernel of the broad phase (which always follows inside a step)
// commit: the flag/scan kernel commits the new counts itself (resident steps with the static grid, where no
// bounds kernel follows); otherwise the bounds kernel (in_step) or a commit launch does
// use_list: the candidate-list pass (one launch) instead of flag/scan + fill
void stage_ghosts(sz_ctx* c, bool in_step = false, bool commit = false, bool use_list = false) {
  State& S = c->S;
  // the parents' count is the host's in resident single-context steps (nothing creates or removes floes there)
  const int nh = in_step && !S.tiled ? c->hostN : -1;
  if (!S.any_periodic_ew && !S.any_periodic_ns) return;
  S.famrec = in_step ? 1 : 0;          // (process mode: ghosts the host uploaded may be present, which have no records)
  Timed t(c, SZ_K_GHOSTS);
  if (use_list) {
    const int waves = std::min(std::max(2 * c->gl_est + 64, 256), 8192);
    hipLaunchKernelGGL(sz_k_ghost_list, dim3((waves + 3) / 4), dim3(256), 0, c->stream, S, c->gl_cur, 1, nh);
    t.end();
    return;
  }
  const int nb = grid_for(S.capM, SCAN_B, 1 << 20);
  hipLaunchKernelGGL(sz_k_ghost_flag_scan, dim3(nb), dim3(SCAN_B), 0, c->stream, S, in_step ? 1 : 0, commit ? 1 : 0, next_epoch(c), nh);
  hipLaunchKernelGGL(sz_k_ghost_fill, dim3(grid_for(S.capM, 32, 2048)), dim3(256), 0, c->stream, S, commit ? 1 : 0, commit ? 1 : 0, nh);
  if (!in_step) hipLaunchKernelGGL(sz_k_ghost_commit, dim3(1), dim3(64), 0, c->stream, S);
  t.end();
}

// workgroups of the neighbour search, on its own or as a part of a launch (sz_k_neighbors_elem, sz_k_vel_search)
int search_grid(const State& T) { return grid_for(T.capM, NB_TPB / NB_G, 8192); }
// The neighbour search of the step State T stands for; it appends the pair items to the narrow phase's work list itself (no scan, no pair-list
// launch).  The instantiation follows from T: the ones that read the collision records where T.crec says they are current in this batch (the
// default stride only), the Dict rule's family records where ghosts can exist (fam), the row stride class from T.maxnb.
// elems: the floe-element items ride in the launch's tail (fields between walls: the lean instantiation -- no ghosts, no Dict rule)
// forcing: the step's forcings ride in it (sz_k_neighbors_forcing)
void launch_search(sz_ctx* c, const State& T, bool elems = false, bool forcing = false) {
  const bool rec = T.crec != nullptr;
  if (forcing) {
    const int nbn = grid_for(T.capM, 256 / NB_G, 8192), nbf = grid_for(T.capM, 256 / FRC_PLAIN, 8192);
    const auto kern = c->precision == 1 ? (rec ? sz_k_neighbors_forcing<2, true> : sz_k_neighbors_forcing<2, false>)
                                        : (rec ? sz_k_neighbors_forcing<1, true> : sz_k_neighbors_forcing<1, false>);
    hipLaunchKernelGGL(kern, dim3(nbn + nbf), dim3(256), 0, c->stream, T, c->P, nbn);
  } else if (elems) {
    const int nbn = search_grid(T), nbe = grid_for(T.capM, NB_TPB, 1 << 20);
    const auto kern = rec ? sz_k_neighbors_elem<false, true> : sz_k_neighbors_elem<false, false>;
    hipLaunchKernelGGL(kern, dim3(nbn + nbe), dim3(NB_TPB), 0, c->stream, T, next_epoch(c), nbn);
  } else {
    const bool fam = c->hostN <= 40000 && (T.any_periodic_ew || T.any_periodic_ns);      // (no periodic wall: no ghosts, no Dict rule)
    const bool wide = T.maxnb > 64;          // (a floe with more than 64 neighbours: the capacity that keeps such a field running, 64 threads per workgroup)
    const auto kern = T.maxnb <= MAXNB ? (fam ? (rec ? sz_k_neighbors<true, MAXNB, true> : sz_k_neighbors<true, MAXNB>) : (rec ? sz_k_neighbors<false, MAXNB, true> : sz_k_neighbors<false, MAXNB>))
                      : !wide ? (fam ? sz_k_neighbors<true, 64> : sz_k_neighbors<false, 64>) : sz_k_neighbors<false, 256>;
    hipLaunchKernelGGL(kern, dim3(wide ? grid_for(T.capM, 64 / NB_G, 16384) : search_grid(T)), dim3(wide ? 64 : NB_TPB), 0, c->stream, T);
  }
}
// static_grid: the geometry in S.bounds is the host's (use_static_grid), no bounds kernel; the pair kernel does
// the housekeeping the bounds kernel would have done
void stage_broad(sz_ctx* c, bool commit_ghosts = false, bool static_grid = false, bool fuse_forcing = false, bool with_elems = false) {
  State& S = c->S;
  Timed t(c, SZ_K_BROAD);
  if (!static_grid) {          // with the static grid the cells are already current (see sz_k_cell_build)
    hipLaunchKernelGGL(sz_k_bounds, dim3(1), dim3(1024), 0, c->stream, S, commit_ghosts ? 1 : 0);
    hipLaunchKernelGGL(sz_k_cell_build, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S, 0);
    c->grid_live = false;
  }
  launch_search(c, S, with_elems, fuse_forcing);
  t.end();
}

void stage_elems(sz_ctx* c, bool enabled) {
  State& S = c->S;
  if (!enabled || !S.any_domain_work) {
    // el_off stays all-zero (allocated zeroed and never written in this mode)
    if (!S.any_domain_work) return;              // C_NELEM is 0 since the upload and nothing ever changes it
    hipLaunchKernelGGL(sz_k_zero_int, dim3(1), dim3(64), 0, c->stream, S.cnt + C_NELEM, S.cnt, -1, 1);
    if (S.any_domain_work)
      hipLaunchKernelGGL(sz_k_zero_int, dim3(grid_for(S.capM + 1, 256)), dim3(256), 0, c->stream, S.el_off, S.cnt, C_M, 1);
    return;
  }
  Timed t(c, SZ_K_BROAD);
  hipLaunchKernelGGL(sz_k_elem_scan_fill, dim3(grid_for(S.capM, SCAN_B, 1 << 20)), dim3(SCAN_B), 0, c->stream, S, next_epoch(c));
  t.end();
}

#ifndef NARROW_G
#define NARROW_G 8
#endif
#ifndef NARROW_KC0          // working set of the first narrow variant: crossings, region points
#define NARROW_KC0 8
#define NARROW_RC0 16
#endif
// The three narrow variants, by ring capacity (NARROW_CAP0 / 1 / 2, sz_kernels.hpp): every launch, the occupancy query and sz_narrow_kernel_name
// name them through these.  The first one's leading template arguments -- G, CAP, KC, RC, RM, TPB, LO, CLS, WPE -- are followed by FRC (the
// step's forcings ride in the launch: 1 fp64, 2 mixed precision) and GEO (a pipelined step: the next step's geometry rides in it).
constexpr int NARROW_TPB = 64;
#define NARROW_FIRST_ARGS NARROW_G, NARROW_CAP0, NARROW_KC0, NARROW_RC0, 4, NARROW_TPB, 0, 0, 3
template <int FRC = 0, int GEO = 0> constexpr auto narrow_first = sz_k_narrow<NARROW_FIRST_ARGS, FRC, GEO>;
constexpr decltype(narrow_first<>) narrow_first_frc[3] = { narrow_first<0>, narrow_first<1>, narrow_first<2> };          // the three-launch steps' flavours, by FRC
constexpr auto narrow_larger = sz_k_narrow<16, NARROW_CAP1, 16, 80, 6, NARROW_TPB, NARROW_CAP0, 1>;
constexpr auto narrow_last = sz_k_narrow<64, NARROW_CAP2, NARROW_KC2, NARROW_RC2, 16, NARROW_TPB, NARROW_CAP1, 2>;

// frc: the step's forcings ride in the launch of the first variant (0: no, 1: fp64, 2: mixed precision)
// rings above the first narrow variant's capacity exist (rings never change size inside the hot path, so the host knows; halo floes of a
// tiled run arrive unseen: their bound counts)
bool larger_rings(const sz_ctx* c) {
  return std::max(std::max(c->max_ring, c->max_elem_ring), c->S.tiled ? c->max_ring_tiled : 0) > NARROW_CAP0;
}
// grid of the first narrow variant: as many workgroups as the chip holds at once, so that every one of them runs the same number of rounds
int narrow_grid(sz_ctx* c) {
  int& grid = c->narrow_grid0;
  if (grid == 0) {
    int per_cu = 0, cus = 0;
    // (asked of the plain flavour for all of them: the FRC / GEO flavours are held to the same 168 registers and 16 KB of LDS per workgroup --
    //  test_hot_kernels_keep_their_register_budgets -- so a CU holds as many of their narrow workgroups)
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, narrow_first<>, NARROW_TPB, 0);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
    grid = per_cu > 0 && cus > 0 ? per_cu * cus : 2048;
    if (const char* e = getenv("SZ_NARROW_GRID")) { int v = atoi(e); if (v > 0) grid = v; }
    if (getenv("SZ_VERBOSE")) fprintf(stderr, "[subzero-hip] narrow: %d workgroups per CU x %d CUs\n", per_cu, cus);
  }
  return grid;
}
// A launch of the first narrow variant on the step State T stands for (event-timed as the class "narrow"): 168 VGPRs (3 wavefronts per SIMD) and
// 16 KB of LDS per workgroup -- 10 workgroups = 80 items in flight per CU.  kern: the flavour; frc: it has the step's forcings in its tail.
// A (a GEO flavour; pipelined steps, sz_pipeline.hpp): the geometry of the next step, for N parents, into the parity A names -- in front
void launch_narrow_first(sz_ctx* c, decltype(narrow_first<>) kern, const State& T, int dt, double ffmo, double fdmo, bool frc, const PipeAlt* A = nullptr, int N = 0) {
  const int nbn = grid_for((long long)T.capPairs + T.capElem, NARROW_TPB / NARROW_G, narrow_grid(c));
  const int nbf = frc ? grid_for(T.capM, NARROW_TPB / FRC_PLAIN, 32768) : 0, nbg = A ? grid_for(N, NARROW_TPB, 1 << 20) : 0;
  Timed t(c, SZ_K_NARROW);
  hipLaunchKernelGGL(kern, dim3(nbn + nbg + nbf), dim3(NARROW_TPB), 0, c->stream, T, c->P, dt, ffmo, fdmo, c->dbg, nbf, A ? *A : PipeAlt{}, nbg, N);
  t.end();
}
// the largest narrow variant, on the items the smaller ones hand on; maxb caps its grid (256, or 2048 where larger rings exist)
void narrow_largest(sz_ctx* c, const State& T, int dt, double ffmo, double fdmo, int maxb) {
  hipLaunchKernelGGL(narrow_last, dim3(grid_for((long long)T.capPairs + T.capElem, 1, maxb)), dim3(NARROW_TPB), 0,
                     c->stream, T, c->P, dt, ffmo, fdmo, c->dbg, 0, PipeAlt{}, 0, 0);
}
// parts: 0 everything (the largest variant is always enqueued: it takes the items the others hand on), 1 without the largest variant unless
// rings that need it exist (sz_step's retry_stop mode), 2 only the larger variants (the rest of a paused step)
void stage_narrow(sz_ctx* c, int dt, double ffmo, double fdmo, int frc = 0, int parts = 0) {
  State& S = c->S;
  long long capItems = (long long)S.capPairs + S.capElem;
  // Rings never change size inside the hot path, so the host knows whether any item can need a
  // larger variant (halo floes of a tiled run arrive unseen: then always check on the device).
  const bool larger = larger_rings(c);
  if (larger && parts != 2) hipLaunchKernelGGL(sz_k_items_clear, dim3(grid_for(capItems, 256)), dim3(256), 0, c->stream, S);
  if (parts != 2) launch_narrow_first(c, narrow_first_frc[frc], S, dt, ffmo, fdmo, frc != 0);
  {
    // larger working sets: items with larger rings (only if such rings can exist) and items the
    // smaller variant handed on; both kernels return at once when the step has no such item
    Timed t(c, K_NARROW_LARGE);
    if (parts == 1 && !larger) { t.end(); return; }
    if (larger)
      hipLaunchKernelGGL(narrow_larger, dim3(grid_for(capItems, 4, 2048)), dim3(NARROW_TPB), 0, c->stream, S, c->P, dt, ffmo, fdmo, c->dbg, 0, PipeAlt{}, 0, 0);
    narrow_largest(c, S, dt, ffmo, fdmo, larger ? 2048 : 256);
    t.end();
  }
}

// m_hint: see sz_k_inter_fill (resident steps: the parents + the ghosts the last look at the device showed, and some)
// the force scale of the fixed-point totals (sz_geom.hpp fx_force_exp): |row force| <= (1 + mu) E h sqrt(area)
int force_scale_exp(const sz_ctx* c) { const double b = (1.0 + std::max(c->P.mu, 0.0)) * c->P.E; return (b > 0.0 && b < 1e300 ? std::ilogb(b) : 0) + 1; }
// the fixed-point totals and the forcings' stop hint from zero: a batch's start, and a step that is run again (its narrow phase adds its rows again)
int clear_totals(sz_ctx* c) {
  HIPCHK(c, hipMemsetAsync(c->facc_buf, 0, (size_t)FX_WORDS * c->S.capM * sizeof(long long), c->stream));
  HIPCHK(c, clear_stop_words(c, W_FRCSTOP));
  return SZ_OK;
}
// behind: the launch that assembles the rows of a reduce-free batch's last step (parents' centroids of that step from `mot`)
void stage_reduce(sz_ctx* c, int mirror, int n_init, int dt, int m_hint = 0, bool behind = false) {
  State& S = c->S;
  Timed t(c, SZ_K_REDUCE);
  if (behind || c->reduce_mode != 2)
    hipLaunchKernelGGL(sz_k_inter_fill, dim3(grid_for(S.capM, 128 / IF_G, 16384)), dim3(128), 0, c->stream, S, mirror, n_init, m_hint, behind || c->reduce_mode == 1 ? 1 : 0, behind ? 1 : 0);
  if (!behind && mirror && c->any_moving) hipLaunchKernelGGL(sz_k_update_boundaries, dim3(1), dim3(64), 0, c->stream, S, dt);
  t.end();
}

// where a coupling step's forcings ride when nothing else rules it out (`fuse`): 0 nowhere (a launch of their own), 1 in the neighbour search's
// launch, 2 in the narrow launch's tail -- by size unless SZ_FUSE_FORCING says.  (Riding in the neighbour launch pays while both kernels leave
// the chip idle: measured better up to 40 k floes, neutral at 100 k dense, worse at 100 k sparse -- there the forcings get their own launch.)
int forcing_fuse_mode(const sz_ctx* c, bool fuse) {
  if (!fuse || (c->pmask >> SZ_K_FORCING & 1u) || !c->fuse_forcing || c->hostN > 65536) return 0;
  const int m = c->fuse_forcing_mode ? c->fuse_forcing_mode : (c->hostN <= 30000 ? 2 : 1);
  return m == 1 && c->S.maxnb > MAXNB ? 2 : m;      // (the neighbour + forcing launch exists for the default neighbour capacity only)
}
// a step of sz_step: `resume` = the rest of a step that paused after its narrow launch (see stopped_late())
void collisions_step(sz_ctx* c, int n_init, int dt, bool commit_ghosts, bool static_grid, int fuse_forcing, bool lean, bool resume) {
  if (!resume) {
    // resident steps of a field between walls: the element items are made in the tail of the neighbour search's launch
    const bool ride = static_grid && fuse_forcing != 1 && c->S.any_domain_work && !c->S.any_periodic_ew && !c->S.any_periodic_ns &&
                      c->S.maxnb <= MAXNB && !c->S.tiled;      // (a tile's neighbour launch commits the halo rows' count: the scan
                                                                                        //  would read it while it changes)
    stage_broad(c, commit_ghosts, static_grid, fuse_forcing == 1, ride);
    if (!ride) stage_elems(c, true);
  }
  stage_narrow(c, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, fuse_forcing == 2 ? (c->precision == 1 ? 2 : 1) : 0, resume ? 2 : lean ? 1 : 0);
  // (rows the step can hold at most, for the reduce's first batch of loads: a tile's halo floes are bounded by the slots of its receive regions,
  //  and any of them may bring up to three ghosts)
  int halo = 0;
  if (c->S.tiled) for (size_t r = 0; r < c->cap_recv.size(); r++) halo += std::max(c->cap_recv[r], 0);
  stage_reduce(c, 1, n_init, dt, c->hostN + halo + 3 * (c->gl_est + halo) + c->hostN / 64 + 32);
}
// fuse_forcing: the step's forcings ride in another launch: 1 the neighbour search's, 2 the narrow phase's
void collisions(sz_ctx* c, int n_init, int dt, bool commit_ghosts = false, bool static_grid = false, int fuse_forcing = 0) {
  stage_broad(c, commit_ghosts, static_grid, fuse_forcing == 1);
  stage_elems(c, true);
  stage_narrow(c, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, fuse_forcing == 2 ? (c->precision == 1 ? 2 : 1) : 0);
  stage_reduce(c, 1, n_init, dt);
}

// The forcings only read the floes' state at the start of the step and write fxOA/fyOA/trqOA/
// hflx_factor, which nothing but the integrator reads: inside a step they run on a second stream
// BESIDE the ghost / broad / narrow / reduce kernels (all of them latency-bound, the chip is far
// from full) and join before the integrator.
void stage_forcing_fork(sz_ctx* c, const State* Sp = nullptr) {
  const State& S = Sp ? *Sp : c->S;
  (void)hipEventRecord(c->ev_fork, c->stream);
  (void)hipStreamWaitEvent(c->stream2, c->ev_fork, 0);
  Timed t(c, SZ_K_FORCING, c->stream2);
  if (c->precision == 1) hipLaunchKernelGGL(sz_k_forcing_mixed, dim3(grid_for(c->S.capM, 256 / FRC_PLAIN, 8192)), dim3(256), 0, c->stream2, S, c->P);
  else hipLaunchKernelGGL(sz_k_forcing<false>, dim3(grid_for(c->S.capM, 256 / FRC_PLAIN, 8192)), dim3(256), 0, c->stream2, S, c->P, 0);
  t.end();
  (void)hipEventRecord(c->ev_join, c->stream2);
}
void stage_forcing_join(sz_ctx* c) { (void)hipStreamWaitEvent(c->stream, c->ev_join, 0); }
// the blocked copy of the sub-floe points the one-way fp64 forcing loop reads (State::sxy): made when the points or the lattice spacing changed
// (SZ_BLOCK_POINTS=0: never -- the loop then reads sx / sy in the caller's order, A/B switch)
int ensure_block_points(sz_ctx* c) {
  State& S = c->S;
  if (c->blk_pts_ok || c->no_block_points || !c->have_fields) return SZ_OK;
  int rc;
  free_pool(c->blk_pt_allocs);
  S.sxy = nullptr;
  if ((rc = dalloc(c, &S.sxy, (size_t)std::max(S.capS, 1), c->blk_pt_allocs))) return rc;
  const double q = std::min(S.gdx, S.gdy) / 4.0;
  if (c->pts_N > 0) hipLaunchKernelGGL(sz_k_block_points, dim3(grid_for(c->pts_N, 1, 1 << 16)), dim3(64), 0, c->stream, S, c->pts_N, q > 0 ? 1.0 / q : 1.0);
  c->blk_pts_ok = true;
  return SZ_OK;
}
// fp32 copies of the sub-floe points and of the lattice for the mixed-precision forcing kernel
int ensure_mixed(sz_ctx* c) {
  State& S = c->S;
  int rc;
  if (!c->mixed_pts_ok) {
    free_pool(c->mixed_pt_allocs);
    if ((rc = dalloc(c, &S.s32, (size_t)std::max(S.capS, 1), c->mixed_pt_allocs))) return rc;
    hipLaunchKernelGGL(sz_k_to_f32_points, dim3(grid_for(S.capS, 256)), dim3(256), 0, c->stream, S, S.capS);
    c->mixed_pts_ok = true;
  }
  if (!c->mixed_geom_ok) {
    world_rings(c);                 // (the body rings are made from the world rings)
    free_pool(c->mixed_geom_allocs);
    if ((rc = dalloc(c, &S.rec32, (size_t)2 * S.capM, c->mixed_geom_allocs)) || (rc = dalloc(c, &S.ring32, (size_t)std::max(S.capV, 1), c->mixed_geom_allocs)) ||
        (rc = dalloc(c, &S.rb_off, (size_t)S.capM, c->mixed_geom_allocs)) || (rc = dalloc(c, &S.rb_n, (size_t)S.capM, c->mixed_geom_allocs))) return rc;
    hipLaunchKernelGGL(sz_k_rec32_seed, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S);
    hipLaunchKernelGGL(sz_k_body_rings, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S);
    c->mixed_geom_ok = true;
  }
  if (!c->mixed_nodes_ok) {
    free_pool(c->mixed_node_allocs);
    const size_t n = (size_t)(S.Nx + 1) * (S.Ny + 1) * 8;
    if ((rc = dalloc(c, &S.nodes32, n, c->mixed_node_allocs))) return rc;
    hipLaunchKernelGGL(sz_k_to_f32_nodes, dim3(grid_for((long long)n, 256)), dim3(256), 0, c->stream, S);
    c->mixed_nodes_ok = true;
  }
  return SZ_OK;
}
// buffers of the two-way coupling: per-floe cell slots follow the floe capacity, per-cell arrays the lattice
int ensure_two_way(sz_ctx* c) {
  State& S = c->S;
  const size_t ncell = (size_t)(S.Nx + 1) * (S.Ny + 1);
  int rc;
  if (c->tw_field_allocs.empty() || c->tw_ncell != ncell) {
    free_pool(c->tw_field_allocs);
    if ((rc = dalloc(c, &S.t_ocn, ncell, c->tw_field_allocs)) || (rc = dalloc(c, &S.t_atm, ncell, c->tw_field_allocs)) ||
        (rc = dalloc(c, &S.tau_x, ncell, c->tw_field_allocs)) || (rc = dalloc(c, &S.tau_y, ncell, c->tw_field_allocs)) ||
        (rc = dalloc(c, &S.si_frac, ncell, c->tw_field_allocs)) || (rc = dalloc(c, &S.cl_cnt, ncell + 1, c->tw_field_allocs)) ||
        (rc = dalloc(c, &S.cl_off, ncell + 2, c->tw_field_allocs)) || (rc = dalloc(c, &S.cl_cur, ncell + 1, c->tw_field_allocs)))
      return rc;
    c->tw_ncell = ncell;
  }
  if (c->have_floes && (c->tw_allocs.empty() || c->tw_capM != S.capM)) {
    free_pool(c->tw_allocs);
    const size_t ne = (size_t)S.capM * FC_CAP;
    if ((rc = dalloc(c, &S.fc_key, ne, c->tw_allocs)) || (rc = dalloc(c, &S.fc_n, ne, c->tw_allocs)) ||
        (rc = dalloc(c, &S.fc_cnt, (size_t)S.capM, c->tw_allocs)) || (rc = dalloc(c, &S.fc_code, ne, c->tw_allocs)) ||
        (rc = dalloc(c, &S.fc_tx, ne, c->tw_allocs)) || (rc = dalloc(c, &S.fc_ty, ne, c->tw_allocs)) ||
        (rc = dalloc(c, &S.fc_area, ne, c->tw_allocs)) || (rc = dalloc(c, &S.cl_ent, ne, c->tw_allocs)))
      return rc;
    c->tw_capM = S.capM;
  }
  return SZ_OK;
}
void stage_forcing(sz_ctx* c, int dt = -1) {      // in-order variant (process mode, profiling)
  Timed t(c, SZ_K_FORCING);
  if (!c->two_way && c->precision == 1) {
    hipLaunchKernelGGL(sz_k_forcing_mixed, dim3(grid_for(c->S.capM, 256 / FRC_PLAIN, 8192)), dim3(256), 0, c->stream, c->S, c->P);
  } else if (!c->two_way) {
    hipLaunchKernelGGL(sz_k_forcing<false>, dim3(grid_for(c->S.capM, 256 / FRC_PLAIN, 8192)), dim3(256), 0, c->stream, c->S, c->P, 0);
  } else {
    // timestep_coupling! with two_way_coupling_on (coupling.jl:1705-1738): one-way forcings + per-floe cell slots,
    // then calc_two_way_coupling! (:1617-1680) as a counting sort by cell, one clip per (floe, cell) entry, a reduction
    State& S = c->S;
    const int ncell = (int)c->tw_ncell;
    // LDS for the largest floe's points only (capacity TW_PMAX): the kernel is bound by the floes in flight per CU
    const int pmax = std::min(TW_PMAX, std::max(32, (c->max_sub + 31) / 32 * 32));
    hipLaunchKernelGGL(sz_k_forcing<true>, dim3(grid_for(S.capM, TW_FPB, 16384)), dim3(TW_FPB * FRC_G), tw_forcing_lds(pmax), c->stream, S, c->P, pmax);
    const int ge = grid_for((long long)S.capM * FC_CAP, 256, 8192);
    hipLaunchKernelGGL(sz_k_tw_count, dim3(ge), dim3(256), 0, c->stream, S);
    scan(c, S.cl_cnt, S.cl_off, ncell, -1, ncell, C_NENT);
    hipLaunchKernelGGL(sz_k_tw_fill, dim3(ge), dim3(256), 0, c->stream, S);
    hipLaunchKernelGGL(sz_k_tw_sort, dim3(grid_for(ncell, 256)), dim3(256), 0, c->stream, S, ncell);
    hipLaunchKernelGGL(sz_k_tw_area_rect, dim3(grid_for((long long)S.capM * 16, 256, 8192)), dim3(256), 0, c->stream, S);
    // tiled runs finish the cells after the partial sums of all ranks have been added up (sz_two_way_partial / _finish)
    if (!S.tiled) hipLaunchKernelGGL(sz_k_tw_reduce, dim3(grid_for(ncell, 256)), dim3(256), 0, c->stream, S, c->P, ncell, dt >= 0 ? dt : c->tw_dt);
  }
  t.end();
}
// gl_fill: ghost-candidate list the integrator appends to (resident steps on the list path), -1: none
void stage_integrate(sz_ctx* c, int dt, bool reset_guards, bool apply_frc, bool bin = false, int gl_fill = -1, int ginl = -1, const PackInl* pack = nullptr) {
  const int nh = bin && !c->S.tiled ? c->hostN : -1;     // resident single-context steps: the host knows the count
  // the guard counters describe the last timestep_floe_properties! call (inside a step the
  // ghost-removal kernel has already cleared them)
  if (reset_guards) (void)hipMemsetAsync(c->S.warn, 0, (size_t)WARN_SLOTS * 32 * sizeof(int), c->stream);
  Timed t(c, SZ_K_INTEGRATE);
  // resident steps with small rings: one launch (thread per floe) integrates, moves the ring and bins the floe
  if (bin && c->max_ring <= MV_RING) {
    // (tiled steps: the same thread also writes the floe's halo records for the next step -- sz_k_integrate<true, true>)
    if (pack) hipLaunchKernelGGL((sz_k_integrate<true, true>), dim3(grid_for(c->S.capM, 128)), dim3(128), 0, c->stream, c->S, c->P, dt, apply_frc ? 1 : 0, 1, nh, gl_fill, ginl, *pack, c->acc_mode);
    else hipLaunchKernelGGL(sz_k_integrate<true>, dim3(grid_for(c->S.capM, 128)), dim3(128), 0, c->stream, c->S, c->P, dt, apply_frc ? 1 : 0, 1, nh, gl_fill, ginl, PackInl{}, c->acc_mode);
  } else {
    hipLaunchKernelGGL(sz_k_integrate<false>, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, c->P, dt, apply_frc ? 1 : 0, 0, nh, gl_fill, -1, PackInl{}, c->acc_mode);
    hipLaunchKernelGGL(sz_k_move_strain, dim3(grid_for(c->S.capM, 16, 8192)), dim3(256), 0, c->stream, c->S, 0, bin ? 1 : 0, gl_fill);
  }
  if (!bin) c->grid_live = false;          // floes moved without re-binning: the resident steps' cell lists are stale
  t.end();
}

// inline ghosts: the keys of the last step's ghosts from the device, and each ghost's number in the reference's order
int gi_fetch(sz_ctx* c) {
  if (!c->gi_pending) return SZ_OK;
  const int G = c->gi_pending_n;
  c->gi_keys.assign(G, 0);
  if (G > 0) HIPCHK(c, hipMemcpy(c->gi_keys.data(), c->S.gkeys + (size_t)c->gi_pending_slot * c->S.capM, (size_t)G * sizeof(long long), hipMemcpyDeviceToHost));
  std::vector<int> ord(G);
  for (int k = 0; k < G; k++) ord[k] = k;
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return c->gi_keys[a] < c->gi_keys[b]; });
  c->gi_ref.assign(G, 0);
  for (int r = 0; r < G; r++) c->gi_ref[ord[r]] = r;
  c->gi_pending = false;
  return SZ_OK;
}
// exact host replay of the fuse bookkeeping (collisions.jl:367-368 and :801-806) for the rare
// steps in which a pair exceeded max_overlap
// after_step (sz_step): the ghosts of the step have already been detached (C_M == N; their rows and the pair arrays are
// still in place) and the integrator has run since: a floe the coupling marked for removal stays `remove`
// (timestep_coupling! follows timestep_collisions! in timestep_sim!, simulation.jl:109-161)
// tkeys (tiled contexts): the order key of every local row -- owned floes, then the step's halo floes and ghosts in allocation order; the
// replay then walks the rows in the order of their keys (= the single context's floe order) and the lists come back indexed by STORAGE row
// with partners named by storage row (tile_fuse_global turns those into global floe numbers)
int host_fuse_fixup(sz_ctx* c, const int* h, bool mirror, bool after_step = false, bool coupled = false, const std::vector<long long>* tkeys = nullptr) {
  State& S = c->S;
  int M = after_step ? h[C_N] + h[C_NGHOSTS] : h[C_M];
  // A resident batch's lists describe the step that ended it, and only that step: whatever earlier batches left in them is dropped.  (The
  // reference's simplify_floes! consumes status.fuse_idx after every step; batches that run on past a fuse -- SZ_NO_STOP, measurement runs --
  // would otherwise replay lists that name the ghost numbers of older steps.)
  if (tkeys || after_step) c->fuse_lists.assign(M, {});
  if ((int)c->fuse_lists.size() < M) c->fuse_lists.resize(M);
  if (h[C_NFUSE] == 0 || M == 0) return SZ_OK;          // no pair asked for a fuse (the narrow phase counts them)
  // the pairs in the reference's serial order (i asc, j asc): per floe its sorted list of owned pairs
  const int MAXNB = S.maxnb;
  std::vector<int> nout(M), nbo((size_t)M * MAXNB); std::vector<int2> info((size_t)M * MAXNB);
  HIPCHK(c, hipMemcpy(nout.data(), S.n_out, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(nbo.data(), S.nb_out, (size_t)M * MAXNB * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(info.data(), S.it_info, (size_t)M * MAXNB * sizeof(int2), hipMemcpyDeviceToHost));
  std::vector<int> tag(M);
  HIPCHK(c, hipMemcpy(tag.data(), c->S.tagA, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
  // inline ghosts lie in allocation order: the replay walks the floes in the reference's order and the lists hold its numbers
  // (ref[storage index] / sto[reference number]; the identity otherwise)
  const int Np = h[C_N];
  if (after_step && c->gi_valid) { int rc = gi_fetch(c); if (rc) return rc; }
  const bool renum = after_step && c->gi_valid && (int)c->gi_ref.size() == M - Np;
  std::vector<int> ref(M), sto(M);
  for (int i = 0; i < M; i++) { ref[i] = i < Np || !renum ? i : Np + c->gi_ref[i - Np]; sto[ref[i]] = i; }
  if (tkeys && (int)tkeys->size() == M) {
    for (int i = 0; i < M; i++) sto[i] = i;
    std::sort(sto.begin(), sto.end(), [&](int a, int b) { return (*tkeys)[a] < (*tkeys)[b]; });
    for (int r = 0; r < M; r++) ref[sto[r]] = r;
  }
  for (int ii = 0; ii < M; ii++) {
    const int i = sto[ii];
    for (int r = 0; r < nout[i]; r++)
      if ((info[(size_t)i * MAXNB + r].x >> 8) & IT_FUSE) { const int pj = nbo[(size_t)i * MAXNB + r]; if (pj >= 0 && pj < M) c->fuse_lists[ii].push_back(ref[pj]); }
  }
  if (mirror) {
    for (int ii = 0; ii < M; ii++) {
      if (tag[sto[ii]] != SZ_FUSE) continue;
      size_t n = c->fuse_lists[ii].size();
      for (size_t k = 0; k < n; k++) {
        const int idx = c->fuse_lists[ii][k];
        if (idx < 0 || idx >= M) continue;          // (a partner number of a step whose ghosts are gone: process-mode lists accumulate like the reference's)
        tag[sto[idx]] = SZ_FUSE; c->fuse_lists[idx].push_back(ii);
      }
    }
  }
  if (after_step && coupled) {
    std::vector<int> rm(h[C_N]);
    HIPCHK(c, hipMemcpy(rm.data(), S.frc_remove, (size_t)h[C_N] * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < h[C_N]; i++) if (rm[i]) tag[i] = SZ_REMOVE;
  }
  HIPCHK(c, hipMemcpy(S.status, tag.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice));
  if (tkeys && (int)tkeys->size() == M) {          // back to storage rows (index and values)
    std::vector<std::vector<int>> byrow(M);
    for (int r = 0; r < M; r++) { byrow[sto[r]] = c->fuse_lists[r]; for (int& v : byrow[sto[r]]) v = v >= 0 && v < M ? sto[v] : v; }
    c->fuse_lists.swap(byrow);
  }
  return SZ_OK;
}

}  // namespace

// =====================================================================================================
extern "C" {

const char* sz_version(void) { return "subzero-hip 0.1 (gfx950)"; }

// SZ_BACKTRACE=1 (diagnosis of a host-side crash on a box without a debugger): SIGSEGV / SIGABRT print the C frames (module + offset: resolve with
// addr2line -e libsubzero_hip.so <offset>) before the process dies
static void sz_crash_handler(int sig) {
  signal(SIGALRM, SIG_DFL); alarm(2);          // (a handler that gets stuck -- the heap's lock may be held -- still ends the process)
  void* fr[64];
  const int n = backtrace(fr, 64);
  const char msg[] = "[subzero-hip] fatal signal, C frames:\n";
  (void)!write(2, msg, sizeof(msg) - 1);
  backtrace_symbols_fd(fr, n, 2);
  signal(sig, SIG_DFL); raise(sig);
}
sz_ctx* sz_create(int device_id) {
  if (getenv("SZ_BACKTRACE")) { void* warm[4]; (void)backtrace(warm, 4); signal(SIGSEGV, sz_crash_handler); signal(SIGABRT, sz_crash_handler); }      // (the first backtrace() loads its library: not inside a handler)
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id >= n) return nullptr;
  if (hipSetDevice(device_id) != hipSuccess) return nullptr;
  sz_ctx* c = new sz_ctx();
  c->device = device_id;
  if (const char* e = getenv("SZ_DEBUG")) c->dbg = atoi(e);
  if (const char* e = getenv("SZ_OVERLAP")) c->overlap_forcing = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("SZ_LEAN_NARROW")) c->no_lean_narrow = atoi(e) == 0;
  if (const char* e = getenv("SZ_PIPELINE")) c->no_pipeline = atoi(e) == 0;
  if (const char* e = getenv("SZ_TILE_HEADERS")) c->tile_hdr_neighbours = strcmp(e, "neighbours") == 0;
  if (const char* e = getenv("SZ_PIPE_MIN_STEPS")) c->pipe_min_steps = std::max(2, atoi(e));
  if (const char* e = getenv("SZ_PIPE_MAX_FLOES")) c->pipe_max_floes = atoi(e);
  if (const char* e = getenv("SZ_BLOCK_POINTS")) c->no_block_points = atoi(e) == 0;
  if (const char* e = getenv("SZ_FUSE_FORCING")) { c->fuse_forcing = atoi(e) != 0; if (atoi(e) > 0) c->fuse_forcing_mode = atoi(e) >= 2 ? 2 : 1; }
  if (const char* e = getenv("SZ_GHOST_LIST")) { c->no_ghost_list = atoi(e) == 0; if (atoi(e) > 1) c->gl_max = atoi(e); }
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);     // lo = least urgent, hi = most urgent
  if (hipStreamCreateWithPriority(&c->stream, hipStreamDefault, prio_hi) != hipSuccess) { delete c; return nullptr; }
  if (hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_lo) != hipSuccess) { delete c; return nullptr; }
  (void)hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming); (void)hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
  // Constants() and default settings of the reference
  Params& P = c->P;
  P.E = 6e6; P.nu = 0.3; P.mu = 0.2; P.rho_o = 1027.0; P.rho_a = 1.2; P.Cd_io = 3e-3; P.Cd_ia = 1e-3;
  P.fcor = 1.4e-4; P.turn = 15.0 * 3.14159265358979323846 / 180.0; P.ff_max_overlap = 0.55; P.fd_max_overlap = 0.75;
  P.rho_i = 920.0; P.max_h = 10.0; P.max_xi = 1e-5; P.lambda = 0.2; P.dd = 1;
  P.Cd_ao = 1.25e-3; P.k_ice = 2.14; P.L_ice = 2.93e5;
  if (hipMalloc((void**)&c->d_stats, 20 * sizeof(long long)) != hipSuccess) { delete c; return nullptr; }
  if (hipMalloc((void**)&c->S.acc, (size_t)ACC_SLOTS * 8 * sizeof(unsigned long long)) != hipSuccess) { delete c; return nullptr; }
  (void)hipMemset(c->S.acc, 0, (size_t)ACC_SLOTS * 8 * sizeof(unsigned long long));
  return c;
}

static void rec_free_all(sz_ctx* c);          // (the output recorder's frames and workspace, below)
void sz_destroy(sz_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  rec_free_all(c);
  free_pool(c->allocs); free_pool(c->list_allocs); free_pool(c->inter_allocs); free_pool(c->static_allocs); free_pool(c->field_allocs); free_pool(c->tw_allocs); free_pool(c->tw_field_allocs);
  free_pool(c->blk_pt_allocs); free_pool(c->mixed_pt_allocs); free_pool(c->mixed_node_allocs); free_pool(c->mixed_geom_allocs); free_pool(c->comm_allocs); free_pool(c->tw_part_allocs); free_pool(c->sub_allocs); free_pool(c->mig_allocs);
  (void)sz_comm_destroy(c);
  for (auto& e : c->evs) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  (void)hipFree(c->d_stats); (void)hipFree(c->S.acc);
  (void)hipFree(c->frac_d); (void)hipFree(c->frac_flag); (void)hipFree(c->frac_idx);
  free_pool(c->weld_allocs); free_pool(c->weldt_allocs); (void)hipFree(c->weld_tmp); free_pool(c->rr_allocs); free_pool(c->rrt_allocs);
  free_pool(c->rm_allocs); free_pool(c->sp_allocs); free_pool(c->spt_allocs); free_pool(c->rect_allocs);
  free_pool(c->frac_allocs);
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2);
  (void)hipEventDestroy(c->ev_fork); (void)hipEventDestroy(c->ev_join);
  delete c;
}

const char* sz_last_error(const sz_ctx* c) { return c ? c->err.c_str() : "no context (no HIP device?)"; }

int sz_set_params(sz_ctx* c, const sz_params* p) {
  if (!c || !p) return SZ_E_ARG;
  Params& P = c->P;
  P.E = p->E; P.nu = p->nu; P.mu = p->mu; P.rho_o = p->rho_o; P.rho_a = p->rho_a; P.Cd_io = p->Cd_io; P.Cd_ia = p->Cd_ia;
  P.fcor = p->f; P.turn = p->turn_theta; P.ff_max_overlap = p->floe_floe_max_overlap; P.fd_max_overlap = p->floe_domain_max_overlap;
  P.rho_i = p->rho_i; P.max_h = p->max_floe_height; P.max_xi = p->maximum_xi; P.lambda = p->lambda; P.dd = p->coupling_dd;
  return SZ_OK;
}

int sz_set_domain(sz_ctx* c, const int32_t* kinds, const double* vals, const double* rects, const double* bu, const double* bv) {
  if (!c || !kinds || !vals || !rects) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  for (int k = 0; k < 4; k++) { c->h_kinds[k] = kinds[k]; c->h_vals[k] = vals[k]; c->h_bu[k] = bu ? bu[k] : 0.0; c->h_bv[k] = bv ? bv[k] : 0.0; }
  memcpy(c->h_rects, rects, 16 * sizeof(double));
  // keep the grid fields alive across the element re-upload
  int rc = upload_elements(c);
  if (!rc) setup_grid(c);
  return rc;
}

int sz_set_topography(sz_ctx* c, int32_t ntopo, const int32_t* off, const double* x, const double* y, const double* cx,
                      const double* cy, const double* rmax) {
  if (!c || ntopo < 0) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  c->h_toff.clear(); c->h_tx.clear(); c->h_ty.clear(); c->h_tcx.clear(); c->h_tcy.clear(); c->h_trmax.clear();
  if (ntopo > 0) {
    c->h_toff.assign(off, off + ntopo + 1);
    c->h_tx.assign(x, x + off[ntopo]); c->h_ty.assign(y, y + off[ntopo]);
    c->h_tcx.assign(cx, cx + ntopo); c->h_tcy.assign(cy, cy + ntopo); c->h_trmax.assign(rmax, rmax + ntopo);
  }
  return upload_elements(c);
}

int sz_set_fields(sz_ctx* c, int32_t Nx, int32_t Ny, double x0, double xf, double y0, double yf, const double* uocn,
                  const double* vocn, const double* hflx, const double* uatm, const double* vatm) {
  if (!c || Nx < 1 || Ny < 1 || !uocn || !vocn || !hflx || !uatm || !vatm) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  State& S = c->S;
  size_t n = (size_t)(Nx + 1) * (Ny + 1);
  free_pool(c->field_allocs); c->dissolved = nullptr;
  // the ocean / atmosphere temperatures (sz_set_temps) and the stress fields stay when the lattice keeps its shape:
  // re-uploading changing currents into one context must not reset them to zero
  if (c->tw_ncell != n) { free_pool(c->tw_field_allocs); c->tw_ncell = 0; c->temps_set = false; }
  double** dst[5] = { &S.uo, &S.vo, &S.hf, &S.ua, &S.va };
  const double* src[5] = { uocn, vocn, hflx, uatm, vatm };
  for (int k = 0; k < 5; k++) {
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, n * sizeof(double)));
    HIPCHK(c, hipMemcpy(q, src[k], n * sizeof(double), hipMemcpyHostToDevice));
    c->field_allocs.push_back(q);
    *dst[k] = (double*)q;
  }
  {
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, n * 8 * sizeof(double)));
    c->field_allocs.push_back(q);
    S.nodes = (double*)q;
  }
  {          // ocean.dissolved (sz_remove.hpp): starts at zero with every new set of fields
    void* q = nullptr;
    HIPCHK(c, hipMalloc(&q, n * sizeof(double)));
    HIPCHK(c, hipMemset(q, 0, n * sizeof(double)));
    c->field_allocs.push_back(q);
    c->dissolved = (double*)q;
  }
  S.Nx = Nx; S.Ny = Ny; S.gx0 = x0; S.gxf = xf; S.gy0 = y0; S.gyf = yf; S.gdx = (xf - x0) / Nx; S.gdy = (yf - y0) / Ny; S.rdx = 1.0 / S.gdx; S.rdy = 1.0 / S.gdy;
  hipLaunchKernelGGL(sz_k_interleave_fields, dim3(grid_for((long long)n, 256)), dim3(256), 0, c->stream, S);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->have_fields = true; c->mixed_nodes_ok = false; c->blk_pts_ok = false; c->S.sxy = nullptr;
  return SZ_OK;
}

namespace {
// The largest number of bounding-circle neighbours a floe of the uploaded field has (periodic images included), with the circles
// inflated by 25 % so that the count still holds after the field has compacted somewhat: the neighbour lists of the device are sized from
// it (State::maxnb).  window_max: the most floes any 3 x 3 cell window holds (cells a little larger than the device's): the pool of the
// neighbour search's fast variant holds 96.  Fields of like-sized floes stay below 24; a field with a size spectrum -- the reference's Voronoi fields: a large
// cell among small ones -- does not, and the reference's own lists grow as needed (collisions.jl:290-296).  O(M) with a uniform grid.
int host_max_neighbours(const sz_ctx* c, const sz_floe_columns* f, int M, int* window_max) {
  *window_max = 0;
  if (!f->rmax || M < 2) return 0;
  double rm = 0.0;
  for (int i = 0; i < M; i++) rm = std::max(rm, f->rmax[i]);
  if (!(rm > 0.0)) return 0;
  const bool px = c->h_kinds[SZ_EAST] == SZ_PERIODIC && c->h_kinds[SZ_WEST] == SZ_PERIODIC;
  const bool py = c->h_kinds[SZ_NORTH] == SZ_PERIODIC && c->h_kinds[SZ_SOUTH] == SZ_PERIODIC;
  double x0 = c->h_vals[3], xf = c->h_vals[2], y0 = c->h_vals[1], yf = c->h_vals[0];     // W, E, S, N
  double bx0 = f->cx[0], bx1 = f->cx[0], by0 = f->cy[0], by1 = f->cy[0];
  for (int i = 1; i < M; i++) { bx0 = std::min(bx0, f->cx[i]); bx1 = std::max(bx1, f->cx[i]); by0 = std::min(by0, f->cy[i]); by1 = std::max(by1, f->cy[i]); }
  if (!px || !(xf > x0)) { x0 = bx0; xf = bx1 + 1e-9 * std::max(1.0, std::fabs(bx1)); }
  if (!py || !(yf > y0)) { y0 = by0; yf = by1 + 1e-9 * std::max(1.0, std::fabs(by1)); }
  const double Lx = std::max(xf - x0, 1e-300), Ly = std::max(yf - y0, 1e-300), cs = 2.5 * rm;
  const int nx = (int)std::max(1.0, std::min(2048.0, std::floor(Lx / cs))), ny = (int)std::max(1.0, std::min(2048.0, std::floor(Ly / cs)));
  auto wrap = [](double v, double lo, double L) { v = std::fmod(v - lo, L); return v < 0 ? v + L : v; };
  auto cell1 = [&](double v, double lo, double L, int n, bool per) { const double t = per ? wrap(v, lo, L) : v - lo; return std::max(0, std::min(n - 1, (int)(t / L * n))); };
  std::vector<int> head((size_t)nx * ny, -1), next(M), cxi(M), cyi(M);
  for (int i = 0; i < M; i++) {
    cxi[i] = cell1(f->cx[i], x0, Lx, nx, px); cyi[i] = cell1(f->cy[i], y0, Ly, ny, py);
    const size_t cidx = (size_t)cyi[i] * nx + cxi[i]; next[i] = head[cidx]; head[cidx] = i;
  }
  int best = 0;
  for (int i = 0; i < M; i++) {
    int cnt = 0, seen[9], ns = 0, win = 0;
    for (int oy = -1; oy <= 1; oy++)
      for (int ox = -1; ox <= 1; ox++) {
        int ax = cxi[i] + ox, ay = cyi[i] + oy;
        if (px) ax = (ax % nx + nx) % nx; else if (ax < 0 || ax >= nx) continue;
        if (py) ay = (ay % ny + ny) % ny; else if (ay < 0 || ay >= ny) continue;
        const int cidx = ay * nx + ax;
        bool dup = false;
        for (int q = 0; q < ns; q++) dup |= seen[q] == cidx;
        if (dup) continue;
        seen[ns++] = cidx;
        for (int j = head[cidx]; j >= 0; j = next[j]) {
          win++;
          if (j == i) continue;
          double dx = f->cx[i] - f->cx[j], dy = f->cy[i] - f->cy[j];
          if (px) dx -= Lx * std::nearbyint(dx / Lx);
          if (py) dy -= Ly * std::nearbyint(dy / Ly);
          const double rr = 1.25 * (f->rmax[i] + f->rmax[j]);
          cnt += (dx * dx + dy * dy) < rr * rr;
        }
      }
    best = std::max(best, cnt); *window_max = std::max(*window_max, win);
  }
  return best;
}
// A field has just been placed in the context's columns -- an upload's copies, a migration's gathered rows: N parents with G ghosts behind them,
// V ring points, sub-floe offsets set for pts_N floes.  The counter block; the per-floe counts a kernel may read before a collision call has
// written them (a re-upload carves the chunks of the previous one again: sz_k_stats walks n_out -- they must not hold what some other array
// left there); ring signs, boxes and trig; then the host's knowledge of the old field goes.  gl_est: how long the ghost-candidate list will
// be (an upper bound); rmax_max / rmax_hint: largest rmax of this field, and of all ranks' (0: unknown) -- the static grid is made from them.
int field_placed(sz_ctx* c, int N, int G, int V, int pts_N, int gl_est, double rmax_max, double rmax_hint) {
  State& S = c->S;
  int h[C_COUNT + 64 + 72] = { 0 };
  h[C_M] = N + G; h[C_N] = N; h[C_NV] = V; h[C_NGHOSTS] = G; h[C_NOWN] = N;
  c->ghosts_staged = G > 0; c->rr_rows = false;          // (ghosts the host staged itself; the rows are not known to be this list's)
  H2D(S.cnt, h, C_COUNT + 64 + 72, int);
  HIPCHK(c, hipMemsetAsync(S.over_stamp, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(S.n_out, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(S.n_in, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(S.el_off, 0, ((size_t)S.capM + 2) * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(S.warn, 0, (size_t)WARN_SLOTS * 32 * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(S.lb_flag, 0, ((size_t)S.capM / 128 + 8) * sizeof(unsigned), c->stream)); c->scan_epoch = 0;      // (the look-back scans' epochs start over)
  hipLaunchKernelGGL(sz_k_osign, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S, 0);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // a new field: whatever sz_tile_enable / sz_tile_setup established belongs to the old one (exchange buffers sized for its capM, the
  // drift reference, the gather interval): sz_tile_run refuses to run until both have been called again
  S.tiled = 0; S.famrec = 0;
  c->tile_margin = 0.0; c->tile_since_box = -1; c->halo_cap = 0; c->d_send = c->d_recv = c->d_ref = nullptr; c->d_dcap = nullptr;
  c->hostM = N + G; c->hostN = N; c->have_floes = true; c->tile_dirty = false; c->mixed_pts_ok = false; c->blk_pts_ok = false; S.sxy = nullptr; c->pts_N = pts_N;
  c->gl_valid = false; c->gl_est = gl_est; c->crec_current = false;
  c->mixed_geom_ok = false; c->rings_stale = false; S.rec32 = nullptr; S.ring32 = nullptr; S.body_rings = 0;
  c->rmax_max = rmax_max; c->rmax_hint = rmax_hint;
  setup_grid(c);
  c->fuse_lists.assign(N + G, {});
  return SZ_OK;
}
}  // namespace

int sz_upload_floes(sz_ctx* c, int64_t M64, int64_t N64, const sz_floe_columns* f) {
  if (!c || !f || M64 < 0 || N64 < 0 || N64 > M64 || !f->vert_off || !f->vx || !f->vy || !f->cx || !f->cy) return SZ_E_ARG;
  if (!c->have_domain) { c->err = "sz_set_domain must be called before sz_upload_floes"; return SZ_E_STATE; }
  if (M64 > N64 && (!f->ghost_off || !f->ghost_idx || !f->ghost_id)) { c->err = "M > N needs ghost_off/ghost_idx/ghost_id"; return SZ_E_ARG; }
  {
    // Rings no kernel holds are refused here, by name, before anything of the last upload is dropped (the kernels' own guards -- ERR_CAP_RING --
    // stay behind this): ring sizes and edge indices travel as bytes, and the ghost passes copy a parent's ring in one wavefront's registers.
    int big = 0;
    for (int64_t i = 0; i < M64; i++) big = std::max(big, f->vert_off[i + 1] - f->vert_off[i]);
    if (big > NARROW_CAP2) {
      c->err = "a ring has " + std::to_string(big) + " points: more than the " + std::to_string(NARROW_CAP2) + " the narrow phase's largest variant holds";
      return SZ_E_CAPACITY;
    }
    if (big > GHOST_RING_WIDE && (c->S.any_periodic_ew || c->S.any_periodic_ns)) {
      c->err = "a ring has " + std::to_string(big) + " points in a domain with a periodic direction: the ghost passes copy rings of at most " +
               std::to_string(GHOST_RING_WIDE) + " points (rings of up to " + std::to_string(NARROW_CAP2) + " need non-periodic boundaries)";
      return SZ_E_CAPACITY;
    }
  }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->gi_pending && c->gi_valid) { int rc0 = gi_fetch(c); if (rc0) return rc0; }      // (the key tables go with the pool; the rows may stay)
  c->gi_pending = false;
  free_pool(c->sub_allocs);
  reset_pool(c->allocs);       // the chunks of the previous upload are carved again (a shim uploads before every replaced call)
  State& S = c->S;
  const int M = (int)M64, N = (int)N64;
  const int V = f->vert_off[M];
  c->max_ring = 0;
  for (int i = 0; i < M; i++) c->max_ring = std::max(c->max_ring, f->vert_off[i + 1] - f->vert_off[i]);
  const int NS = f->sub_off ? f->sub_off[N] : 0;
  // neighbour and row capacities from the field itself: like-sized floes 24 / 32, a size spectrum 64 / 128 (SZ_MAXNB=24|64 overrides)
  int window_max = 0;
  c->nb_count_max = host_max_neighbours(c, f, M, &window_max);
  S.maxnb = c->nb_count_max + 2 <= MAXNB && window_max <= 80 ? MAXNB : c->nb_count_max + 2 <= 64 ? 64 : 256;
  if (const char* e = getenv("SZ_MAXNB")) S.maxnb = atoi(e) > 64 ? 256 : atoi(e) > MAXNB ? 64 : MAXNB;
  S.rowcap = S.maxnb <= MAXNB ? ROWCAP : S.maxnb <= 64 ? 128 : 512;
  if (const char* e = getenv("SZ_ROWCAP")) S.rowcap = std::max(1, atoi(e));          // (tests of the growth path)
  S.capM = std::max(2 * M + 64, M + 2048);      // (rows for the floes, their ghosts and -- a tile -- its halo: small tiles of fast floes hold more halo floes than owned ones)
  S.capV = std::max(2 * V + 4096, V + 32768); S.capPairs = S.capM * (S.maxnb <= MAXNB ? 8 : 16); S.capElem = S.capM * 4;
  S.capRows = S.capPairs * 3 + S.capElem * 2; S.capCells = 4 * S.capM + 64; S.capS = NS;
  int rc;
#define DA(field, n) if ((rc = dalloc(c, &S.field, (size_t)(n), c->allocs))) return rc
  DA(cnt, C_COUNT + 64 + 72); DA(warn, WARN_SLOTS * 32);      // counters | 64 per-rank counts of the pack kernel | its 66 scratch words
  const ColTable<double**> dcols = state_column_slots(S);
  const ColTable<const double*> hcols = host_columns(*f);
  for (int k = 0; k < MIG_NSC; k++) {
    if ((rc = dalloc(c, dcols.p[k], S.capM, c->allocs))) return rc;
    if (hcols.p[k]) H2D(*dcols.p[k], hcols.p[k], M, double);
  }
  for (int k = MIG_NSC; k < MIG_NTAB; k++) if ((rc = dalloc(c, dcols.p[k], (size_t)4 * S.capM, c->allocs))) return rc;
  DA(mot, 4 * S.capM); DA(mot2, 2 * S.capM); DA(trig, 2 * S.capM);
  for (int k = MIG_NSC; k < MIG_NTAB; k++) if (hcols.p[k]) H2D(*dcols.p[k], hcols.p[k], 4 * M, double);
  DA(id, S.capM); DA(ghost_id, S.capM); DA(okey, S.capM); DA(status, S.capM); DA(parent, S.capM); DA(gh, MAX_GHOSTS * S.capM); DA(ngh, S.capM);
  DA(gh_save, MAX_GHOSTS * S.capM); DA(ngh_save, S.capM);
  std::vector<int> tag0;          // (tagA starts as the status column: the integrator of a resident step only rewrites it where a tag was raised)
  DA(frc_remove, S.capM); DA(osign, S.capM); DA(bbx0, S.capM); DA(bbx1, S.capM); DA(bby0, S.capM); DA(bby1, S.capM);
  {
    std::vector<long long> id(M), gid(M, 0);
    std::vector<int> st(M, SZ_ACTIVE), parent(M), gh((size_t)MAX_GHOSTS * M, -1), ngh(M, 0);
    for (int i = 0; i < M; i++) { id[i] = f->id ? f->id[i] : i + 1; if (f->ghost_id) gid[i] = f->ghost_id[i]; if (f->status) st[i] = f->status[i]; parent[i] = i; }
    if (M > N) {
      for (int i = 0; i < N; i++) {
        int n = f->ghost_off[i + 1] - f->ghost_off[i];
        if (n > MAX_GHOSTS) { c->err = "more than 3 ghosts for one parent"; return SZ_E_ARG; }
        ngh[i] = n;
        for (int k = 0; k < n; k++) { int g = f->ghost_idx[f->ghost_off[i] + k]; if (g < N || g >= M) { c->err = "ghost index out of range"; return SZ_E_ARG; } gh[(size_t)i * MAX_GHOSTS + k] = g; parent[g] = i; }
      }
    }
    { std::vector<long long> ok(S.capM); for (int i = 0; i < S.capM; i++) ok[i] = i; H2D(S.okey, ok.data(), S.capM, long long); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    H2D(S.id, id.data(), M, long long); H2D(S.ghost_id, gid.data(), M, long long); H2D(S.status, st.data(), M, int);
    tag0 = st;
    H2D(S.parent, parent.data(), M, int); H2D(S.gh, gh.data(), (size_t)MAX_GHOSTS * M, int); H2D(S.ngh, ngh.data(), M, int);
    HIPCHK(c, hipStreamSynchronize(c->stream));   // host vectors go out of scope
  }
  DA(voff, S.capM + 1); DA(vxy, S.capV);
  H2D(S.voff, f->vert_off, M + 1, int);
  {          // the rings, interleaved {x, y} on the device (State::vxy)
    std::vector<double> xy((size_t)2 * std::max(V, 1));
    for (int k = 0; k < V; k++) { xy[(size_t)2 * k] = f->vx[k]; xy[(size_t)2 * k + 1] = f->vy[k]; }
    H2D(S.vxy, xy.data(), (size_t)2 * V, double); HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  DA(soff, S.capM + 1); DA(sx, NS); DA(sy, NS);
  if (f->sub_off) { H2D(S.soff, f->sub_off, N + 1, int); H2D(S.sx, f->sx, NS, double); H2D(S.sy, f->sy, NS, double); }
  c->max_sub = 0;
  if (f->sub_off) for (int i = 0; i < N; i++) c->max_sub = std::max(c->max_sub, f->sub_off[i + 1] - f->sub_off[i]);
  DA(gplan, S.capM + 1); DA(gscan4, S.capM + 1); DA(gtot4, 4);
  DA(lb_agg, S.capM / 128 + 8); DA(lb_inc, S.capM / 128 + 8); DA(lb_flag, S.capM / 128 + 8);      // (tiles of 128 .. SCAN_B elements)
  DA(gflag, S.capM + 1); DA(gvscan, S.capM + 2); DA(gcand, (size_t)2 * S.capM); DA(galloc, 32); DA(gkeys, (size_t)2 * S.capM); DA(fam, S.capM);
  DA(crec, (size_t)8 * S.capM); c->crec_buf = S.crec; S.crec = nullptr;
  {          // the twin set of the pipelined steps' double buffers (sz_pipeline.hpp)
    StepSet& B = c->pb[1];
    if ((rc = dalloc(c, &B.vxy, (size_t)S.capV, c->allocs)) || (rc = dalloc(c, &B.crec, (size_t)8 * S.capM, c->allocs)) ||
        (rc = dalloc(c, &B.gh, (size_t)MAX_GHOSTS * S.capM, c->allocs)) || (rc = dalloc(c, &B.ngh, (size_t)S.capM, c->allocs))) return rc;
    HIPCHK(c, hipMemsetAsync(B.gh, 0xff, (size_t)MAX_GHOSTS * S.capM * sizeof(int), c->stream));
    c->gpar = 0;
  }
  DA(facc, (size_t)FX_WORDS * S.capM); c->facc_buf = S.facc; S.facc = nullptr;
  c->maybe_tagged = false;          // (what the host's status column says: a migration's floes keep what the context knew)
  if (f->status) for (int i = 0; i < N; i++) if (f->status[i] != SZ_ACTIVE) { c->maybe_tagged = true; break; }
  for (int k = 0; k < 4; k++) if ((rc = dalloc(c, &c->frc_alt[k], (size_t)S.capM, c->allocs))) return rc;
  DA(bounds, 16 + 64 * 4); DA(cell_cnt, S.capCells + 1); DA(cell_ovf, S.capCells + 1); DA(cell_slots, (size_t)S.capCells * CELL_K + 8);
  DA(cell_items, S.capM);
  {
    StepSet& B = c->pb[1];
    if ((rc = dalloc(c, &B.cell_cnt, (size_t)S.capCells + 1, c->allocs)) || (rc = dalloc(c, &B.cell_ovf, (size_t)S.capCells + 1, c->allocs)) ||
        (rc = dalloc(c, &B.cell_slots, (size_t)S.capCells * CELL_K + 8, c->allocs)) || (rc = dalloc(c, &B.cell_items, (size_t)S.capM, c->allocs))) return rc;
  }
  DA(n_out, S.capM + 1); DA(n_in, S.capM + 1); DA(over_stamp, S.capM + 1); DA(over_base, S.capM + 1);
  DA(out_off, S.capM + 2);
  DA(el_off, S.capM + 2); DA(el_floe, S.capElem); DA(el_elem, S.capElem);
  DA(inter_off, S.capM + 2);
  if (!f->sub_off) HIPCHK(c, hipMemsetAsync(S.soff, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
  // neighbour lists, pair items and their rows: in a pool of their own, carved again (larger) when a step outgrows them
  if ((rc = carve_lists(c))) return rc;
  // floe.interactions is part of the floe state, but not of sz_floe_columns (it is ragged): the rows the last
  // collision call left stay valid across an upload of the same size; after an upload of another size they are
  // gone, and sz_timestep_floe_properties / sz_calc_stress refuse to run on nothing (SZ_E_STATE) until
  // sz_upload_interactions or a collision call provides them again
  if ((rc = carve_interactions(c))) return rc;
  DA(blk, std::max(S.capCells, std::max(S.capM, 1024)) / SCAN_B + 1024);
  own_set_carved(c);          // (set 0 -- gpar above -- is what this upload carved)
  DA(tagA, S.capM + 1);
  if (!tag0.empty()) { H2D(S.tagA, tag0.data(), M, int); HIPCHK(c, hipStreamSynchronize(c->stream)); }
  if ((rc = dalloc(c, &c->origin, (size_t)S.capM, c->allocs))) return rc;
  { std::vector<int> o(std::max(M, 1)); for (int i = 0; i < M; i++) o[i] = i; H2D(c->origin, o.data(), M, int); HIPCHK(c, hipStreamSynchronize(c->stream)); }
  DA(stamps, 512 + 8 * 8000);
  trim_pool(c->allocs);
  free_pool(c->comm_allocs);          // (sized for the old field's capM; a migration keeps its capacities and these chunks with them)
  int gl_est = N;          // parents near a periodic wall: how long the ghost-candidate list will be (a superset of it)
  double rmax_max = 0.0;
  if (f->rmax) {
    const double x0 = c->h_vals[3], xf = c->h_vals[2], y0 = c->h_vals[1], yf = c->h_vals[0];
    const bool pew = c->h_kinds[SZ_EAST] == SZ_PERIODIC && c->h_kinds[SZ_WEST] == SZ_PERIODIC;
    const bool pns = c->h_kinds[SZ_NORTH] == SZ_PERIODIC && c->h_kinds[SZ_SOUTH] == SZ_PERIODIC;
    gl_est = 0;
    for (int i = 0; i < N; i++) {
      const double r = f->rmax[i];
      if ((pew && (f->cx[i] - r < x0 || f->cx[i] + r > xf)) || (pns && (f->cy[i] - r < y0 || f->cy[i] + r > yf))) gl_est++;
    }
    for (int i = 0; i < M; i++) rmax_max = std::max(rmax_max, f->rmax[i]);
  }
  // (an upload may bring ghosts, and floes without sub-floe points; its largest rmax is the host's, and no other rank's is known: no hint)
  if ((rc = field_placed(c, N, M - N, V, f->sub_off ? N : 0, gl_est, rmax_max, 0.0))) return rc;
  c->tile_inter_state = TILE_INTER_NONE;          // (whatever rows stay are the host's to answer for: nothing is translated)
  c->upload_M = M; c->upload_V = V;
  return SZ_OK;
}

int sz_get_stats(sz_ctx* c, sz_stats* out) {
  if (!c || !out || !c->have_floes) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  State& S = c->S;
  HIPCHK(c, hipMemsetAsync(c->d_stats, 0, 20 * sizeof(long long), c->stream));
  hipLaunchKernelGGL(sz_k_stats, dim3(grid_for((long long)S.capPairs + S.capElem, 256, 1024)), dim3(256), 0, c->stream, S, c->d_stats);
  int h[C_COUNT]; long long st[20];
  HIPCHK(c, hipMemcpyAsync(st, c->d_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  if (int rc = fetch_counters(c, h)) return rc;
  int soffN = 0;
  HIPCHK(c, hipMemcpy(&soffN, S.soff + h[C_N], sizeof(int), hipMemcpyDeviceToHost));
  out->M = h[C_M]; out->N = h[C_N]; out->n_ring_points = h[C_NV]; out->n_sub_points = soffN;
  out->n_pairs = st[16]; out->n_pair_ring_points = st[0]; out->n_pair_rows = st[1];
  out->n_elem_items = h[C_NELEM]; out->n_elem_rows = st[2]; out->n_inter_rows = st[3]; out->n_ghosts = h[C_NGHOSTS];
  out->warn_height = st[6]; out->warn_force = st[7]; out->warn_vel = st[8]; out->warn_xi = st[9];
  out->n_trace_fail = h[C_TRACE_FAIL];
  out->n_halo = h[C_NHALO];
  out->n_pairs_clipped = st[17];
  out->n_status_remove = st[4]; out->n_status_fuse = st[5];
  out->n_retry = h[C_NRETRY];
  out->acc_narrow_launches = st[10]; out->acc_pair_items = st[11]; out->acc_pair_ring_points = st[12];
  out->acc_pair_rows = st[13]; out->acc_elem_items = st[14]; out->acc_elem_rows = st[15];
  out->acc_dir_checks = st[18]; out->acc_dir_checks_certified = st[19];
  return SZ_OK;
}

int sz_download_floes(sz_ctx* c, sz_floe_columns* f) {
  if (!c || !f || !c->have_floes) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  world_rings(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  State& S = c->S;
  int h[C_COUNT];
  HIPCHK(c, hipMemcpy(h, S.cnt, sizeof(h), hipMemcpyDeviceToHost));
  int M = h[C_M], N = h[C_N], V = h[C_NV];
#define D2H(dst, src, n, T) if (dst) HIPCHK(c, hipMemcpy(dst, src, (size_t)(n) * sizeof(T), hipMemcpyDeviceToHost))
  const ColTable<double*> dst = host_columns(*f), src = state_columns(S);
  for (int k = 0; k < MIG_NTAB; k++) D2H(dst.p[k], src.p[k], col_width(k) * M, double);
  D2H(f->id, S.id, M, long long); D2H(f->ghost_id, S.ghost_id, M, long long); D2H(f->status, S.status, M, int);
  D2H(f->vert_off, S.voff, M + 1, int);
  if ((f->vx || f->vy) && V > 0) {
    std::vector<double> xy((size_t)2 * V);
    HIPCHK(c, hipMemcpy(xy.data(), S.vxy, (size_t)2 * V * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < V; k++) { if (f->vx) f->vx[k] = xy[(size_t)2 * k]; if (f->vy) f->vy[k] = xy[(size_t)2 * k + 1]; }
  }
  if (f->ghost_off) {
    std::vector<int> gh((size_t)MAX_GHOSTS * M), ngh(M);
    HIPCHK(c, hipMemcpy(gh.data(), S.gh, gh.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(ngh.data(), S.ngh, (size_t)M * sizeof(int), hipMemcpyDeviceToHost));
    int t = 0; f->ghost_off[0] = 0;
    for (int i = 0; i < M; i++) {
      int n = i < N ? ngh[i] : 0;
      for (int k = 0; k < n; k++) { if (f->ghost_idx) f->ghost_idx[t] = gh[(size_t)i * MAX_GHOSTS + k]; t++; }
      f->ghost_off[i + 1] = t;
    }
  }
  return SZ_OK;
}

// ---------------------------------------------------------------- Float32 hosts (include/subzero_hip.h: sz_floe_columns_f32)
// (widened on the way in, rounded on the way out: F32Up / F32Down, sz_columns.hpp)
int sz_upload_floes_f32(sz_ctx* c, int64_t M, int64_t N, const sz_floe_columns_f32* f) {
  if (!c || !f || M < 0 || N < 0 || N > M) return SZ_E_ARG;
  if (M > 0 && !f->vert_off) { c->err = "sz_upload_floes_f32: vert_off is required"; return SZ_E_ARG; }
  const size_t V = M > 0 ? (size_t)f->vert_off[M] : 0, NS = (f->sub_off && N > 0) ? (size_t)f->sub_off[N] : 0;
  const F32Up W(f, (size_t)M, V, NS);
  return sz_upload_floes(c, M, N, &W.d);
}
int sz_download_floes_f32(sz_ctx* c, sz_floe_columns_f32* f) {
  if (!c || !f) return SZ_E_ARG;
  sz_stats st;
  int rc = sz_get_stats(c, &st); if (rc) return rc;
  F32Down W(f, (size_t)st.M, (size_t)st.n_ring_points, (size_t)st.n_sub_points, F32_LEAVE_SUB);
  rc = sz_download_floes(c, &W.d); if (rc) return rc;
  W.back();
  return SZ_OK;
}
int sz_set_fields_f32(sz_ctx* c, int32_t Nx, int32_t Ny, double x0, double xf, double y0, double yf, const float* uocn, const float* vocn,
                      const float* hflx, const float* uatm, const float* vatm) {
  if (!c || Nx < 1 || Ny < 1) return SZ_E_ARG;
  const size_t n = (size_t)(Nx + 1) * (Ny + 1);
  std::vector<double> a[5]; const float* src[5] = { uocn, vocn, hflx, uatm, vatm };
  for (int k = 0; k < 5; k++) if (src[k]) { a[k].resize(n); for (size_t q = 0; q < n; q++) a[k][q] = (double)src[k][q]; }
  auto p = [&](int k) { return src[k] ? a[k].data() : (const double*)nullptr; };
  return sz_set_fields(c, Nx, Ny, x0, xf, y0, yf, p(0), p(1), p(2), p(3), p(4));
}
int sz_download_interactions_f32(sz_ctx* c, int32_t* off, float* rows) {
  if (!c || !off) return SZ_E_ARG;
  sz_stats st;
  int rc = sz_get_stats(c, &st); if (rc) return rc;
  rc = sz_download_interactions(c, off, nullptr); if (rc) return rc;          // the offsets first: off[M] = rows in all
  const size_t total = (size_t)off[st.M];
  if (!rows || total == 0) return SZ_OK;
  std::vector<double> r(total * 7);
  rc = sz_download_interactions(c, off, r.data()); if (rc) return rc;
  for (size_t k = 0; k < total * 7; k++) rows[k] = (float)r[k];
  return SZ_OK;
}

int sz_download_interactions(sz_ctx* c, int32_t* off, double* rows) {
  if (!c || !off || !c->have_floes) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  State& S = c->S;
  // rows are kept at a fixed stride on the device: compact to CSR here
  scan(c, S.inter_cnt, S.inter_off, S.capM, C_M, 0, C_NINTER);
  int h[C_COUNT];
  if (int rc = fetch_counters(c, h)) return rc;
  HIPCHK(c, hipMemcpy(off, S.inter_off, (size_t)(h[C_M] + 1) * sizeof(int), hipMemcpyDeviceToHost));
  int total = h[C_NINTER];
  if (rows && total > 0) {
    double* tmp = nullptr;
    HIPCHK(c, hipMalloc((void**)&tmp, (size_t)total * 7 * sizeof(double)));
    hipLaunchKernelGGL(sz_k_inter_compact, dim3(grid_for(S.capM, 128)), dim3(128), 0, c->stream, S, tmp);
    hipError_t e = hipMemcpyAsync(rows, tmp, (size_t)total * 7 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) { c->err = hipGetErrorString(e); return SZ_E_HIP; }
    if (c->gi_valid) { int rc2 = gi_fetch(c); if (rc2) return rc2; }
    if (c->gi_valid) {            // partners that were inline ghosts: order key -> the reference's floe number
      std::vector<long long> sorted(c->gi_keys);
      std::sort(sorted.begin(), sorted.end());
      const double lim = (double)((long long)1 << 40);
      for (int r = 0; r < total; r++) {
        const double idx = rows[(size_t)r * 7];
        if (idx <= lim) continue;
        const long long key = (long long)idx - 1;
        const auto it = std::lower_bound(sorted.begin(), sorted.end(), key);
        if (it == sorted.end() || *it != key) { c->err = "interaction row names a ghost that is not among the last step's"; return SZ_E_STATE; }
        rows[(size_t)r * 7] = (double)(c->hostN + (int)(it - sorted.begin()) + 1);
      }
    }
  }
  return SZ_OK;
}

int sz_download_pairs(sz_ctx* c, int32_t* pi, int32_t* pj) {
  if (!c || !pi || !pj || !c->have_floes) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  State& S = c->S;
  // the compact list is made here, on demand: the steps themselves only keep the per-floe sorted lists (the ghosts of the
  // last resident step own pairs too: their rows outlive their removal)
  int h[C_COUNT];
  int rc = sync_and_check(c, h);
  if (rc) return rc;
  const int mlast = std::max(h[C_M], h[C_N] + h[C_NGHOSTS]);
  scan(c, S.n_out, S.out_off, S.capM, -1, mlast, C_NPAIRS);
  hipLaunchKernelGGL(sz_k_pairs_fill, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S, mlast);
  rc = sync_and_check(c, h);
  if (rc) return rc;
  if (h[C_NPAIRS] > 0) {
    HIPCHK(c, hipMemcpy(pi, c->S.pair_i, (size_t)h[C_NPAIRS] * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(pj, c->S.pair_j, (size_t)h[C_NPAIRS] * sizeof(int), hipMemcpyDeviceToHost));
    if (c->gi_valid) { int rc2 = gi_fetch(c); if (rc2) return rc2; }
    if (c->gi_valid && (int)c->gi_ref.size() == mlast - h[C_N]) {       // inline ghosts: storage index -> the reference's number, then its serial order
      const int Np = h[C_N], np = h[C_NPAIRS];
      std::vector<std::pair<int, int>> ps(np);
      for (int k = 0; k < np; k++)
        ps[k] = { pi[k] < Np ? pi[k] : Np + c->gi_ref[pi[k] - Np], pj[k] < Np ? pj[k] : Np + c->gi_ref[pj[k] - Np] };
      std::sort(ps.begin(), ps.end());
      for (int k = 0; k < np; k++) { pi[k] = ps[k].first; pj[k] = ps[k].second; }
    }
  }
  return SZ_OK;
}

int sz_download_fuse(sz_ctx* c, int32_t* off, int32_t* idx) {
  if (!c || !off || !c->have_floes) return SZ_E_ARG;
  int M = c->hostM, t = 0;
  off[0] = 0;
  for (int i = 0; i < M; i++) {
    if (i < (int)c->fuse_lists.size())
      for (int v : c->fuse_lists[i]) { if (idx) idx[t] = v; t++; }
    off[i + 1] = t;
  }
  return SZ_OK;
}

// sub-floe points of the floes the context holds (CSR: off has N + 1 entries; call with sx == NULL for the offsets alone): after a
// migration the host's copy of these is the library's
int sz_download_subpoints(sz_ctx* c, int32_t* off, double* sx, double* sy) {
  if (!c || !c->have_floes || !off) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int N = c->hostN;
  HIPCHK(c, hipMemcpy(off, c->S.soff, ((size_t)N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (sx && sy && off[N] > 0) {
    HIPCHK(c, hipMemcpy(sx, c->S.sx, (size_t)off[N] * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(sy, c->S.sy, (size_t)off[N] * sizeof(double), hipMemcpyDeviceToHost));
  }
  return SZ_OK;
}

int sz_get_boundary_vals(sz_ctx* c, double* vals4) {
  if (!c || !vals4 || !c->have_domain) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  HIPCHK(c, hipMemcpy(vals4, c->S.eval, 4 * sizeof(double), hipMemcpyDeviceToHost));
  return SZ_OK;
}

// the four boundary rectangles as they stand: {xmin, xmax, ymin, ymax} each, order N, S, E, W (MovingBoundary walls move)
int sz_get_boundary_rects(sz_ctx* c, double* rects16) {
  if (!c || !rects16 || !c->have_domain) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  HIPCHK(c, hipMemcpy(rects16, c->S.erect, 16 * sizeof(double), hipMemcpyDeviceToHost));
  return SZ_OK;
}

// which_vertices_match_points on given points and a given region ring (the reference's test vectors for it)
int sz_debug_match_vertices(sz_ctx* c, int32_t npts, const double* px, const double* py, int32_t nr, const double* rx, const double* ry,
                            int32_t* idx, int32_t* n_out) {
  if (!c || npts < 0 || npts > NARROW_KC2 || nr < 1 || nr > NARROW_RC2 || !idx || !n_out) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  PoolGuard pool;
  double *dpx, *dpy, *drx, *dry; int* dout;
  int rc;
  if ((rc = dalloc(c, &dpx, npts, pool.v)) || (rc = dalloc(c, &dpy, npts, pool.v)) || (rc = dalloc(c, &drx, nr, pool.v)) ||
      (rc = dalloc(c, &dry, nr, pool.v)) || (rc = dalloc(c, &dout, npts + 1, pool.v))) return rc;
  H2D(dpx, px, npts, double); H2D(dpy, py, npts, double); H2D(drx, rx, nr, double); H2D(dry, ry, nr, double);
  hipLaunchKernelGGL(sz_k_debug_match_vertices, dim3(1), dim3(64), 0, c->stream, npts, dpx, dpy, nr, drx, dry, dout);
  std::vector<int> h(npts + 1);
  HIPCHK(c, hipMemcpyAsync(h.data(), dout, (size_t)(npts + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_out = h[0];
  for (int k = 0; k < h[0]; k++) idx[k] = h[1 + k];
  return SZ_OK;
}

// the forcing kernels' in-bounds test and lattice sample at given points (the reference's vectors for in_bounds / find_interp_knots)
int sz_debug_sample_fields(sz_ctx* c, int32_t n, const double* x, const double* y, double* out12) {
  if (!c || n < 0 || (n > 0 && (!x || !y || !out12))) return SZ_E_ARG;
  if (!c->have_fields || !c->have_domain) { c->err = "sz_debug_sample_fields needs sz_set_domain and sz_set_fields"; return SZ_E_STATE; }
  if (n == 0) return SZ_OK;
  (void)hipSetDevice(c->device);
  PoolGuard pool;
  double *dx, *dy, *dout;
  int rc;
  if ((rc = dalloc(c, &dx, n, pool.v)) || (rc = dalloc(c, &dy, n, pool.v)) || (rc = dalloc(c, &dout, (size_t)12 * n, pool.v))) return rc;
  H2D(dx, x, n, double); H2D(dy, y, n, double);
  hipLaunchKernelGGL(sz_k_debug_sample, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, c->S, n, dx, dy, dout);
  HIPCHK(c, hipMemcpyAsync(out12, dout, (size_t)12 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}

// the fixed-point totals' own arithmetic on given numbers (sz_fxdebug.hpp): no floe, no step kernel
int sz_debug_fx_totals(sz_ctx* c, int32_t n, const double* v, const int32_t* perm, int32_t nthreads, int32_t mode, int32_t e, double area, double height,
                       double rmax, int64_t* words2, int32_t* flags2, double* joined) {
  const int how = mode & 7;
  if (!c || n < 0 || n > 4096 || nthreads < 1 || nthreads > 1024 || (n > 0 && (!v || !perm)) || (mode & ~15) || how > FXD_LEVER || !words2 || !flags2 || !joined) return SZ_E_ARG;
  for (int k = 0; k < n; k++) if (perm[k] < 0 || perm[k] >= n) return SZ_E_ARG;
  if (mode & FXD_CTX_KEXP) e = force_scale_exp(c);
  (void)hipSetDevice(c->device);
  PoolGuard pool;
  double *dv, *dj; int *dp, *df; long long* dw;
  int rc;
  if ((rc = dalloc(c, &dv, n, pool.v)) || (rc = dalloc(c, &dp, n, pool.v)) || (rc = dalloc(c, &dw, 2, pool.v)) || (rc = dalloc(c, &df, 2, pool.v)) ||
      (rc = dalloc(c, &dj, 1, pool.v))) return rc;
  if (n > 0) { H2D(dv, v, n, double); H2D(dp, perm, n, int); }
  HIPCHK(c, hipMemsetAsync(dw, 0, 2 * sizeof(long long), c->stream));
  HIPCHK(c, hipMemsetAsync(df, 0, 2 * sizeof(int), c->stream));
  hipLaunchKernelGGL(sz_k_debug_fx_add, dim3(grid_for(nthreads, 256)), dim3(256), 0, c->stream, n, dv, dp, nthreads, how, e, area, height, rmax, dw, df);
  hipLaunchKernelGGL(sz_k_debug_fx_read, dim3(1), dim3(64), 0, c->stream, how, e, area, height, rmax, dw, df, dj);
  long long hw[2]; int hf[2];
  HIPCHK(c, hipMemcpyAsync(hw, dw, sizeof(hw), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hf, df, sizeof(hf), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(joined, dj, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  words2[0] = hw[0]; words2[1] = hw[1]; flags2[0] = hf[0]; flags2[1] = hf[1];
  return SZ_OK;
}

int sz_debug_fx_word(sz_ctx* c, const double* row5, double sign, double cx, double cy, int32_t eF, int32_t eA, int32_t eL, int64_t* words14, int32_t* bad) {
  if (!c || !row5 || !words14 || !bad) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  PoolGuard pool;
  double* dr; long long* dw; int* df;
  int rc;
  if ((rc = dalloc(c, &dr, 5, pool.v)) || (rc = dalloc(c, &dw, 14, pool.v)) || (rc = dalloc(c, &df, 1, pool.v))) return rc;
  H2D(dr, row5, 5, double);
  HIPCHK(c, hipMemsetAsync(df, 0, sizeof(int), c->stream));
  hipLaunchKernelGGL(sz_k_debug_fx_word, dim3(1), dim3(64), 0, c->stream, dr, sign, cx, cy, eF, eA, eL, dw, df);
  long long hw[14]; int hb = 0;
  HIPCHK(c, hipMemcpyAsync(hw, dw, sizeof(hw), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&hb, df, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 14; k++) words14[k] = hw[k];
  *bad = hb;
  return SZ_OK;
}

// ---------------------------------------------------------------- processes
int sz_add_ghosts(sz_ctx* c) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  c->gi_valid = false;         // (what follows numbers its ghosts by storage position)
  leave_resident(c);            // a process-mode call: the resident steps' ghost-candidate list is stale, the world rings must be current
  int oldM = c->hostM;
  stage_ghosts(c);
  int rc = sync_and_check(c);
  if (rc) return rc;
  // deepcopy_floe copies status.fuse_idx (floe_utils.jl:138)
  if (c->hostM > oldM) {
    std::vector<int> parent(c->hostM);
    HIPCHK(c, hipMemcpy(parent.data(), c->S.parent, (size_t)c->hostM * sizeof(int), hipMemcpyDeviceToHost));
    c->fuse_lists.resize(c->hostM);
    for (int g = oldM; g < c->hostM; g++) c->fuse_lists[g] = c->fuse_lists[parent[g]];
  }
  c->ghosts_staged = true; c->rr_rows = false;
  return SZ_OK;
}

int sz_remove_ghosts(sz_ctx* c) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  leave_resident(c);            // a process-mode call: the resident steps' ghost-candidate list is stale, the world rings must be current
  hipLaunchKernelGGL(sz_k_remove_ghosts, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, 0);
  int rc = sync_and_check(c);
  if (rc) return rc;
  c->fuse_lists.resize(c->hostM);
  c->ghosts_staged = false; c->rr_rows = false;
  return SZ_OK;
}

int sz_timestep_collisions(sz_ctx* c, int64_t n_init, int32_t dt) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  c->maybe_tagged = true;
  (void)hipSetDevice(c->device);
  c->gi_valid = false;         // (what follows numbers its ghosts by storage position)
  leave_resident(c);            // a process-mode call: the resident steps' ghost-candidate list is stale, the world rings must be current
  c->S.callid = ++c->callid;
  int h[C_COUNT];
  for (;;) {
    collisions(c, (int)n_init, dt);
    c->inter_any = true; c->inter_lost = false;
    int rc = sync_and_check(c, h);
    // a list outgrown (neighbours per floe, pair items, rows per floe): larger lists, the call again -- the reference's lists grow (collisions.jl:290-296)
    if (rc == SZ_E_CAPACITY && growable(c->last_err_bits)) { if ((rc = grow_lists(c, c->last_err_bits))) return rc; continue; }
    if (rc) return rc;
    break;
  }
  c->rr_rows = true;
  return host_fuse_fixup(c, h, true);
}

int sz_collide_pairs(sz_ctx* c, int64_t np, const int32_t* pi, const int32_t* pj, int32_t dt, double max_overlap) {
  if (!c || !c->have_floes || np < 0 || (np > 0 && (!pi || !pj))) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  c->gi_valid = false;         // (what follows numbers its ghosts by storage position)
  leave_resident(c);
  State& S = c->S;
  if (np > S.capPairs) { c->err = "too many explicit pairs"; return SZ_E_CAPACITY; }
  c->maybe_tagged = true;
  std::vector<std::pair<int, int>> ps(np);
  for (int64_t k = 0; k < np; k++) {
    if (pi[k] < 0 || pj[k] < 0 || pi[k] >= c->hostM || pj[k] >= c->hostM || pi[k] == pj[k]) { c->err = "pair index out of range"; return SZ_E_ARG; }
    ps[k] = { pi[k], pj[k] };
  }
  std::sort(ps.begin(), ps.end());
  std::vector<int> hi(np), hj(np);
  for (int64_t k = 0; k < np; k++) { hi[k] = ps[k].first; hj[k] = ps[k].second; }
  if (np) { H2D(S.pair_i, hi.data(), np, int); H2D(S.pair_j, hj.data(), np, int); }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  S.callid = ++c->callid;
  hipLaunchKernelGGL(sz_k_pairs_explicit, dim3(grid_for(S.capM + 1, 256)), dim3(256), 0, c->stream, S, (int)np);
  stage_elems(c, false);
  stage_narrow(c, dt, max_overlap, c->P.fd_max_overlap);
  stage_reduce(c, 0, c->hostN, dt);
  c->inter_any = true; c->inter_lost = false;
  int h[C_COUNT];
  int rc = sync_and_check(c, h);
  if (rc) return rc;
  return host_fuse_fixup(c, h, false);
}

int sz_collide_domain(sz_ctx* c, int32_t dt, double max_overlap) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  c->maybe_tagged = true;
  (void)hipSetDevice(c->device);
  c->gi_valid = false;         // (what follows numbers its ghosts by storage position)
  leave_resident(c);            // a process-mode call: the resident steps' ghost-candidate list is stale, the world rings must be current
  State& S = c->S;
  S.callid = ++c->callid;
  hipLaunchKernelGGL(sz_k_pairs_explicit, dim3(grid_for(S.capM + 1, 256)), dim3(256), 0, c->stream, S, 0);
  stage_elems(c, true);
  stage_narrow(c, dt, c->P.ff_max_overlap, max_overlap);
  stage_reduce(c, 0, c->hostN, dt);
  c->inter_any = true; c->inter_lost = false;
  return sync_and_check(c);
}

int sz_timestep_coupling(sz_ctx* c) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (!c->have_fields) { c->err = "sz_set_fields must be called before sz_timestep_coupling"; return SZ_E_STATE; }
  c->maybe_tagged = true;
  (void)hipSetDevice(c->device);
  leave_resident(c);            // a process-mode call: the resident steps' ghost-candidate list is stale, the world rings must be current
  if (c->two_way) { if (c->S.tiled) { c->err = "tiled contexts couple through sz_tile_step + sz_two_way_partial / sz_two_way_finish"; return SZ_E_STATE; } int rc = ensure_two_way(c); if (rc) return rc; }
  if (c->precision == 1 && !c->two_way) { int rc = ensure_mixed(c); if (rc) return rc; }
  if (c->precision == 0 && !c->two_way) { int rc = ensure_block_points(c); if (rc) return rc; }
  stage_forcing(c);
  hipLaunchKernelGGL(sz_k_apply_frc, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S);
  return sync_and_check(c);
}

// ---- precision of the forcings: 0 = fp64 (default), 1 = mixed (per-point arithmetic in fp32, sz_kernels.hpp)
int sz_set_precision(sz_ctx* c, int32_t mode) {
  if (!c || mode < 0 || mode > 1) return SZ_E_ARG;
  if (mode == 0 && c->precision == 1 && c->have_floes) {        // back to fp64: the world rings are the state again
    (void)hipSetDevice(c->device);
    world_rings(c);
    c->S.rec32 = nullptr; c->S.body_rings = 0; c->mixed_geom_ok = false;
  }
  c->precision = mode;
  return SZ_OK;
}
// ---- two-way coupling (coupling.jl:1617-1680; CouplingSettings(two_way_coupling_on = true))
int sz_set_two_way(sz_ctx* c, int32_t on, double Cd_ao, double k, double L, int32_t dt) {
  if (!c) return SZ_E_ARG;
  c->two_way = on != 0; c->P.Cd_ao = Cd_ao; c->P.k_ice = k; c->P.L_ice = L; c->tw_dt = dt;
  return SZ_OK;
}
int sz_set_temps(sz_ctx* c, const double* t_ocn, const double* t_atm) {
  if (!c || !t_ocn || !t_atm) return SZ_E_ARG;
  if (!c->have_fields) { c->err = "sz_set_fields must be called before sz_set_temps"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  int rc = ensure_two_way(c); if (rc) return rc;
  H2D(c->S.t_ocn, t_ocn, c->tw_ncell, double); H2D(c->S.t_atm, t_atm, c->tw_ncell, double);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->temps_set = true;
  return SZ_OK;
}
int sz_download_ocean_stress(sz_ctx* c, double* tau_x, double* tau_y, double* si_frac, double* hflx) {
  if (!c || !c->have_fields) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  int rc = ensure_two_way(c); if (rc) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t nb = c->tw_ncell * sizeof(double);
  if (tau_x) HIPCHK(c, hipMemcpy(tau_x, c->S.tau_x, nb, hipMemcpyDeviceToHost));
  if (tau_y) HIPCHK(c, hipMemcpy(tau_y, c->S.tau_y, nb, hipMemcpyDeviceToHost));
  if (si_frac) HIPCHK(c, hipMemcpy(si_frac, c->S.si_frac, nb, hipMemcpyDeviceToHost));
  if (hflx) HIPCHK(c, hipMemcpy(hflx, c->S.hf, nb, hipMemcpyDeviceToHost));
  return SZ_OK;
}

namespace {
int need_interactions(sz_ctx* c) {
  if (!c->inter_lost) return SZ_OK;
  c->err = "the interaction rows of the last collision call were dropped by an upload of another size: "
           "sz_upload_interactions (floe.interactions of every floe, possibly empty) or a collision call must come first";
  return SZ_E_STATE;
}
}  // namespace
int sz_timestep_floe_properties(sz_ctx* c, int32_t dt) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (int rc = need_interactions(c)) return rc;
  (void)hipSetDevice(c->device);
  leave_resident(c);            // a process-mode call: the resident steps' ghost-candidate list is stale, the world rings must be current
  stage_integrate(c, dt, true, false);
  return sync_and_check(c);
}

// floe.interactions of every floe replaced by hand (CSR, rows k x 7: floeidx, xforce, yforce, xpoint, ypoint,
// torque, overlap): what the reference's calc_stress! test does before calling it (test_update_floe.jl:27-30)
int sz_upload_interactions(sz_ctx* c, const int32_t* off, const double* rows) {
  if (!c || !c->have_floes || !off) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  tile_cleanup(c);
  State& S = c->S;
  const int M = c->hostM;
  if (off[M] == 0) {           // no floe has interactions (fresh floes): the counts are all there is to say
    HIPCHK(c, hipMemsetAsync(S.inter_cnt, 0, (size_t)M * sizeof(int), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->inter_any = true; c->inter_lost = false; c->rr_rows = true;
    return SZ_OK;
  }
  if (!rows) return SZ_E_ARG;
  const int ROWCAP = S.rowcap;
  std::vector<int> cnt(M); std::vector<double> buf((size_t)M * ROWCAP * 7, 0.0);
  for (int i = 0; i < M; i++) {
    int k = off[i + 1] - off[i];
    if (k < 0 || k > ROWCAP) { c->err = "more interaction rows per floe than the fixed stride holds"; return SZ_E_CAPACITY; }
    cnt[i] = k;
    if (k) memcpy(&buf[(size_t)i * ROWCAP * 7], rows + (size_t)off[i] * 7, (size_t)k * 7 * sizeof(double));
  }
  H2D(S.inter_cnt, cnt.data(), M, int);
  H2D(S.inter_rows, buf.data(), (size_t)M * ROWCAP * 7, double);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->inter_any = true; c->inter_lost = false; c->rr_rows = true;
  return SZ_OK;
}
// calc_stress! (update_floe.jl:392-414) and calc_strain! (:425-453) on their own, for every floe
int sz_calc_stress(sz_ctx* c) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (int rc = need_interactions(c)) return rc;
  (void)hipSetDevice(c->device);
  hipLaunchKernelGGL(sz_k_calc_stress, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, c->P);
  return sync_and_check(c);
}
int sz_calc_strain(sz_ctx* c) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  hipLaunchKernelGGL(sz_k_move_strain, dim3(grid_for(c->S.capM, 16, 8192)), dim3(256), 0, c->stream, c->S, 1, 0, -1);
  return sync_and_check(c);
}

namespace {
// a list of buffers to fill with one launch (sz_k_clear_many); bytes must be a multiple of 4, the value is a byte value as for memset
struct Clears {
  ClearList L{}; unsigned long long maxw = 0; sz_ctx* ctx;
  explicit Clears(sz_ctx* c) : ctx(c) {}
  void add(void* p, size_t bytes, int byte_val = 0) {
    if (L.n == CLEAR_MAX) launch(ctx);          // (a full list goes out; the order of the clears among themselves does not matter)
    const unsigned b = (unsigned)(byte_val & 0xff);
    L.p[L.n] = (unsigned*)p; L.words[L.n] = bytes / 4; L.val[L.n] = b | (b << 8) | (b << 16) | (b << 24);
    maxw = std::max(maxw, L.words[L.n]); L.n++;
  }
  void launch(sz_ctx* c) {
    if (!L.n) return;
    hipLaunchKernelGGL(sz_k_clear_many, dim3(grid_for((long long)maxw, 256, 2048)), dim3(256), 0, c->stream, L);
    L.n = 0; maxw = 0;
  }
};
// ---------------------------------------------------------------- pipelined batches (sz_pipeline.hpp)
// the State of step parity q: everything that is double-buffered points at set q; rows of the step's makers at region q
State pipe_state(sz_ctx* c, int q) {
  State S = c->S;
  step_set_copy(S, c->pb[q]);
  // rows of a step's makers: set 0 straight behind the parents (as everywhere else), set 1 from a multiple of 16 half way through the spare rows
  const int nr1 = (c->hostN + (S.capM - c->hostN) / 2 + 15) & ~15;
  S.goff = q ? nr1 - c->hostN : 0; S.gcap = q ? S.capM - nr1 : nr1 - c->hostN; S.gslot = q;
  return S;
}
PipeAlt pipe_alt(sz_ctx* c, int q, int make_ghosts) {
  const State T = pipe_state(c, q);
  PipeAlt A;
  step_set_copy(A, T); A.goff = T.goff; A.gslot = T.gslot; A.make_ghosts = make_ghosts;
  return A;
}
// make set q the context's own (c->S, crec_buf): where the state lies after a pipelined batch.  State::crec of c->S is a batch mode -- null, or
// the records the batch started on -- and stays what it is: the set's records become crec_buf
void pipe_adopt(sz_ctx* c, int q) {
  double2* const mode = c->S.crec;
  step_set_copy(c->S, c->pb[q]);
  c->crec_buf = c->S.crec; c->S.crec = mode; c->gpar = q;
}
// ---------------------------------------------------------------- what a resident batch decides (BatchPlan)
// Everything a batch driver branches on, decided once before the batch touches anything: a function of the context as the last call left it
// and of the arguments -- no rule reads what batch_enter sets up (the static grid, the ghost list, the ensure_* buffers, the world rings).
struct BatchPlan {
  // a periodic pair of walls; SZ_COLLISIONS_ON; the batch ends at the first tag (no SZ_NO_STOP)
  bool periodic, coll, user_stop;
  // static grid; ghosts from the candidate list; inline ghosts (made by the integrator); mixed precision; its steps run on body-frame rings
  bool sg, gl, gi, mixed, body;
  // collision records kept current; fixed-point totals; reduce-free steps (rows once, behind the batch); the pipelined two-launch steps; a
  // fracture criterion is evaluated in the batch
  bool cr, facc_on, rfree, pipe, frac;
  // the steps start without the largest narrow variant (a driver puts it in when an item needs it); the first step is enqueued on its own, as
  // a last step
  bool lean, first_alone;
  // the stop words the batch starts with cleared; the first inline ghosts are the driver's (a tile seeds them behind its first pack)
  unsigned stop_mask; bool own_first_ghosts;
  int reduce_mode;                     // sz_ctx::reduce_mode of the batch
  void set_rfree(bool r) { rfree = r; reduce_mode = !facc_on ? 0 : r ? 2 : 1; }
};
// what the integrator is told (sz_ctx::acc_mode): totals on, reduce-free steps, and in those: the host knows this is the batch's last step
static int integrator_acc_mode(bool facc_on, bool rfree, bool last) { return !facc_on ? 0 : 1 | (rfree ? 4 | (last ? 2 : 0) : 0); }
// the largest narrow variant only takes items the small one hands on (none in most fields): it is left out of the steps until one
// shows up -- the batch then pauses inside that step (stopped_late()) and its driver finishes it
static bool lean_wanted(const sz_ctx* c) { return !c->retry_seen && !c->no_lean_narrow && !larger_rings(c); }
// collision records (State::crec): in batches whose kernels keep them current -- the one-launch integrator, and for periodic walls the
// inline ghost maker.
// Fixed-point totals (State::facc; sz_geom.hpp): the narrow phase adds every row to both floes' totals, the integrator reads them -- no reduce
// launch inside the steps.
static void plan_records_totals(BatchPlan& p, const sz_ctx* c, int nsteps) {
  p.cr = p.coll && p.sg && c->crec_buf && c->max_ring <= MV_RING && (p.gi || !p.periodic) && nsteps > 0;
  p.facc_on = p.coll && c->facc_buf != nullptr;
}
bool pipeline_eligible(const sz_ctx* c, const BatchPlan& p, int nsteps, int flags) {
  return p.rfree && !c->no_pipeline && c->frac_kind == SZ_FRAC_OFF && p.coll && p.sg && (p.gi || !p.periodic) && p.cr && nsteps >= c->pipe_min_steps && c->hostN <= c->pipe_max_floes && c->precision == 0 && !c->two_way &&
         (!c->S.any_domain_work || (!p.periodic && !c->any_moving)) && c->S.maxnb <= MAXNB && !larger_rings(c) && c->pb[1].vxy && c->pb[1].work &&
         (c->S.capM - c->hostN) / 2 > 64 && (flags & SZ_COLLISIONS_ON);
}
static BatchPlan plan_batch(const sz_ctx* c, int nsteps, int flags) {
  BatchPlan p{};
  p.periodic = c->S.any_periodic_ew || c->S.any_periodic_ns;
  p.coll = (flags & SZ_COLLISIONS_ON) != 0;
  // the batch ends after the first step that leaves a parent tagged remove / fuse (simplify_floes!, simulation.jl:205-214,
  // is the host's): the launches of the later steps are enqueued all the same and return at once (stopped())
  p.user_stop = !(flags & SZ_NO_STOP);
  p.stop_mask = W_STOP | W_RETRYSTOP;
  p.sg = p.coll && c->grid_ok;
  p.gl = ghost_list_wanted(c, p.sg);
  // inline ghosts: no ghost launch in the steps at all (the integrator makes the next step's ghosts; needs the one-launch integrator)
  p.gi = p.gl && !c->S.tiled && c->max_ring <= MV_RING;
  p.mixed = c->precision == 1 && !c->two_way;
  // mixed precision: the steps run on body-frame rings (the integrator moves poses, not rings) when nothing else in the batch
  // needs world rings -- single context, the list path for the ghosts, rings small enough for the fused integrator
  p.body = p.mixed && p.coll && p.sg && (p.gl || !p.periodic) && !c->S.tiled && c->max_ring <= MV_RING;
  plan_records_totals(p, c, nsteps);
  // floe.interactions of the step that ended the batch is assembled once, behind the batch (stage_reduce(.., behind)): that needs the ghosts
  // of that step still in their rows, i.e. the one-launch integrator with inline ghosts (or no periodic wall), which knows when it runs a
  // batch's last step (sz_k_integrate: last_step).  The other paths keep the launch inside the step, rows only.
  p.set_rfree(p.facc_on && p.sg && (p.gi || !p.periodic) && c->max_ring <= MV_RING && !c->any_moving);
  // pipelined batches (sz_pipeline.hpp: two launches per step) run their own prologue -- records, first ghosts, first neighbour search
  p.pipe = pipeline_eligible(c, p, nsteps, flags);
  // (a tile's three-launch steps keep the variant in; the pipelined steps do not ask whether the context is tiled -- kept as found)
  p.lean = p.coll && lean_wanted(c) && (p.pipe || !c->S.tiled);
  // a parent that is already tagged ends the batch after its first step, and the integrator only finds out while it runs (the tags of a
  // step itself are raised by its narrow phase / forcings, a launch earlier): that first step is then enqueued on its own, as a last step
  p.first_alone = p.rfree && c->maybe_tagged && p.user_stop && nsteps > 1;
  // fracture criterion (sz_set_fracture): evaluated after every fracture step of a batch that stops -- one that runs through has no use for it
  p.frac = c->frac_kind != SZ_FRAC_OFF && p.user_stop && !p.pipe;
  return p;
}

// A batch of pipelined steps: L1(s) = narrow(s) | GEO(s) | forcings(s), L2(s) = VEL(s) | search(s + 1).  Same contract as the loop of sz_step
// it replaces: h = the counter block after the batch, *done = the steps that ran; the context's state is complete when it returns (rows of
// the last step assembled, strain evaluated, ghosts detached).
// *slot_out: the allocator slot of the last step's inline ghosts (the parity of its set).
// *rest_out: the lists grew past what the pipelined launches are compiled for (MAXNB); the batch handed back the state at step *done_out and the
// caller runs the rest on the three-launch steps.
// It runs inside sz_step's BatchModes scope (the modes batch_enter has set from the plan are the batch's) and opens none of its own.
int step_batch_pipelined(sz_ctx* c, const BatchPlan& plan, int nsteps, int tstep0, int dt, int coupling_dt, int flags, int* h, int* done_out, int* slot_out, bool* rest_out) {
  State& S0 = c->S;
  const int N = c->hostN;
  const bool fam = N <= 40000 && plan.periodic;
  const bool elems = S0.any_domain_work != 0;          // (eligible only without a periodic pair: no ghosts, the floe count is the host's)
  const int q0 = c->gpar;
  auto par = [&](int s) { return (q0 + s) & 1; };
  S0.restart_on_tags = plan.user_stop ? 0 : 1;
  bool lean = plan.lean;
  Clears clr(c);          // (the batch's clears go out with the first prologue's, in one launch)
  clr.add(c->facc_buf, (size_t)FX_WORDS * S0.capM * sizeof(long long));
  clr.add(S0.cnt + C_FRCSTOP, sizeof(int));
  const int callid0 = c->callid; c->callid += nsteps;
  // ---- the prologue of a (sub-)batch that starts at step s: cells, records, ghosts and the neighbour search of that step, from the floes as they lie
  bool first_start = true;
  auto prologue = [&](int s) {
    const int q = par(s);
    pipe_adopt(c, q);                                   // (the geometry of step s is in set q: the context's own from here on)
    S0.step = 0; S0.goff = 0; S0.gcap = 0;
    if (!first_start) c->grid_live = false;             // (a restart: the cells hold ghosts of a step that is started afresh)
    use_static_grid(c);                                 // cells[q] <- the parents (unless they are: the last batch's update binned them)
    const StepSet& O = c->pb[1 - q];
    clr.add(O.cell_cnt, ((size_t)S0.capCells + 1) * sizeof(int));
    clr.add(O.cell_ovf, ((size_t)S0.capCells + 1) * sizeof(int));
    clr.add(c->pb[0].wq, NSEG * 32 * sizeof(int)); clr.add(c->pb[1].wq, NSEG * 32 * sizeof(int));
    clr.add(c->pb[0].ngh, (size_t)S0.capM * sizeof(int));          // (no links: a restart after a tag comes with those GEO made for a step that is now started afresh)
    clr.add(c->pb[1].ngh, (size_t)S0.capM * sizeof(int));
    clr.add(S0.galloc, 32 * sizeof(unsigned long long));
    clr.launch(c);
    // the records of both sets from the columns (the static quads of the twin; its geometry quads are GEO's) -- unless the last batch left them current
    if (!(first_start && c->crec_current))
      for (int b = 0; b < 2; b++) { State T = pipe_state(c, b); T.step = 0; seed_records(c, T, N); }
    first_start = false;
    State T = pipe_state(c, q); T.step = s + 1; T.callid = callid0 + s + 1; T.retry_stop = lean ? 1 : 0;
    if (plan.gi) hipLaunchKernelGGL(sz_k_ghost_inline_seed, dim3(grid_for(S0.capM, 256)), dim3(256), 0, c->stream, T, q, N);
    launch_search(c, T, elems);          // (between walls: the element items of the step in the tail of its search, as the three-launch steps do)
  };
  auto launch_L1 = [&](int s, bool make_ghosts) {
    State T = pipe_state(c, par(s)); T.step = s + 1; T.callid = callid0 + s + 1; T.retry_stop = lean ? 1 : 0;
    const PipeAlt A = pipe_alt(c, par(s + 1), make_ghosts ? 1 : 0);
    const bool coupling = coupling_at(flags, coupling_dt, tstep0 + s);
    const bool overlap = coupling && (c->overlap_forcing >= 0 ? c->overlap_forcing != 0 : N > 65536);
    if (overlap) stage_forcing_fork(c, &T);
    if (coupling) c->forcing_where = overlap ? 0 : 2;
    // (event-timed classes of a pipelined step: "narrow" = L1, "integrate" = L2)
    const bool frc = coupling && !overlap;          // (pipelined batches are fp64: pipeline_eligible)
    launch_narrow_first(c, frc ? narrow_first<1, 1> : narrow_first<0, 1>, T, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, frc, &A, N);
    if (!lean) narrow_largest(c, T, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, 256);          // (it takes what the small one hands on)
    return overlap;
  };
  auto launch_L2 = [&](int s, bool with_search, bool host_last, bool joined) {
    if (joined) stage_forcing_join(c);
    State T = pipe_state(c, par(s + 1)); T.step = s + 2; T.callid = callid0 + s + 2; T.retry_stop = lean ? 1 : 0;
    const PipeAlt A = pipe_alt(c, par(s), 0);
    const int nbv = grid_for(N, NB_TPB, 1 << 20), nbs = with_search ? search_grid(T) : 0;
    const int nbe = with_search && elems ? grid_for(N, NB_TPB, 1 << 20) : 0;
    const unsigned ep = nbe ? next_epoch(c) : 0u;
    const int am = 1 | 4 | (host_last ? 2 : 0);
    Timed tm(c, SZ_K_INTEGRATE);
    if (fam) hipLaunchKernelGGL((sz_k_vel_search<true>), dim3(nbv + nbs + nbe), dim3(NB_TPB), 0, c->stream, T, c->P, A, dt, coupling_at(flags, coupling_dt, tstep0 + s) ? 1 : 0, nbv, N, am, nbe, ep);
    else hipLaunchKernelGGL((sz_k_vel_search<false>), dim3(nbv + nbs + nbe), dim3(NB_TPB), 0, c->stream, T, c->P, A, dt, coupling_at(flags, coupling_dt, tstep0 + s) ? 1 : 0, nbv, N, am, nbe, ep);
    tm.end();
  };
  // what lies behind the last step `last` (0-based) of the batch: parents un-swapped after a tag stop, strain, the step's rows, rows home, ghosts off
  auto epilogue = [&](int last, bool after_device_stop) {
    const int q = par(last + 1);                          // the geometry of the state that is handed back
    pipe_adopt(c, q);
    if (after_device_stop) {
      State T = pipe_state(c, q); T.step = 0;
      hipLaunchKernelGGL(sz_k_unswap, dim3(grid_for(N, 128)), dim3(128), 0, c->stream, T, pipe_alt(c, 1 - q, 0), N);
      c->grid_live = false;
    }
    State T = pipe_state(c, q); T.step = 0; T.goff = 0;
    hipLaunchKernelGGL(sz_k_move_strain, dim3(grid_for(S0.capM, 16, 8192)), dim3(256), 0, c->stream, T, 1, 0, -1);      // calc_strain! of the state handed back
    // the rows of step `last`: its links and row region are parity par(last)'s; the parents' centroids of that step are in mot
    State R = pipe_state(c, par(last)); R.step = 0; R.vxy = T.vxy;
    hipLaunchKernelGGL(sz_k_inter_fill, dim3(grid_for(S0.capM, 128 / IF_G, 16384)), dim3(128), 0, c->stream, R, 1, N, 0, 1, 2 + last);      // (2 + last: behind, for 1-based step last + 1)
  };
  int s_end = plan.first_alone ? 1 : nsteps;
  int s0 = 0, done = 0; bool need_prologue = true;
  for (;;) {
    S0.retry_stop = lean ? 1 : 0;
    if (need_prologue) { prologue(s0); need_prologue = false; }
    for (int s = s0; s < s_end; s++) {
      const bool host_last = s + 1 == s_end;
      const bool joined = launch_L1(s, !host_last);
      launch_L2(s, !host_last, host_last, joined);
    }
    // the epilogue of the case "all steps ran" goes out with the steps: its launches look at the counters and return when the batch ended early
    // (sz_k_inter_fill: behind-mode guard; the strain launch is harmless either way and is repeated below)
    S0.step = 0;
    epilogue(s_end - 1, false);
    if (int rc = fetch_counters(c, h)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    if (h[C_ERR] & ~ERR_CAP_INTER) {          // (the rows' stride, ERR_CAP_INTER, is dealt with behind the loop: the bit stays up until then)
      const int bits = h[C_ERR] & ~ERR_CAP_INTER;
      if (growable(bits) && h[C_RETRYSTOP] > 0) {
        // a list of step sr outgrown (neighbours, pair items): the batch paused there before the step changed anything -- larger lists, then that
        // step and the rest again (as sz_step)
        int z = 0; (void)hipMemcpy(S0.cnt + C_ERR, &z, sizeof(int), hipMemcpyHostToDevice);
        const int sr = h[C_RETRYSTOP] - 1;
        pipe_adopt(c, par(sr));
        int rc = grow_lists(c, bits & (ERR_CAP_NEIGH | ERR_CAP_PAIRS)); if (rc) return rc;
        (void)clear_stop_words(c, W_RETRYSTOP); (void)clear_stop_words(c, W_STOP);
        if ((rc = clear_totals(c))) return rc;
        if (S0.maxnb > MAXNB) {
          // the prologue's and the L2 launch's neighbour search are instantiated for MAXNB-wide rows (neighbors_body's row stride): with the
          // wider lists the steps from sr on are the three-launch ones.  The state of step sr is set par(sr)'s (adopted above); the ghost links
          // GEO(sr - 1) made go, the caller's batch seeds its own from the parents as they lie (as sz_step does after growing its lists)
          Clears cl(c);
          for (int b = 0; b < 2; b++) { cl.add(c->pb[b].ngh, (size_t)S0.capM * sizeof(int)); cl.add(c->pb[b].gh, (size_t)MAX_GHOSTS * S0.capM * sizeof(int), 0xff); }
          cl.launch(c);
          HIPCHK(c, hipStreamSynchronize(c->stream));
          if (getenv("SZ_VERBOSE")) fprintf(stderr, "[subzero-hip] pipelined batch: lists outgrew its neighbour capacity in step %d of %d, the rest on the three-launch steps\n", sr + 1, nsteps);
          c->grid_live = false; c->crec_current = false; c->callid = callid0 + sr;
          *done_out = sr; *rest_out = true;
          return SZ_OK;
        }
        s0 = sr; need_prologue = true;
        continue;
      }
      (void)sync_and_check(c, h);          // (sets the error text, clears the word)
      return SZ_E_CAPACITY;
    }
    if (lean && h[C_RETRYSTOP] > 0) {
      // paused inside step sr: an item for the largest narrow variant.  That variant on the step's own State, the step's second launch again, on
      // with the steps behind it (the variant stays in from now on)
      const int sr = h[C_RETRYSTOP] - 1;
      c->retry_seen = true; lean = false;
      (void)clear_stop_words(c, W_RETRYSTOP | W_PAUSED);
      State T = pipe_state(c, par(sr)); T.step = sr + 1; T.callid = callid0 + sr + 1; T.retry_stop = 0;
      narrow_largest(c, T, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, 256);
      const bool host_last = sr + 1 == s_end;
      S0.retry_stop = 0;
      launch_L2(sr, !host_last, host_last, false);
      s0 = sr + 1;
      if (s0 >= s_end) {          // it was the last step: only the epilogue is left
        S0.step = 0;
        epilogue(s_end - 1, false);
        if (int rc = fetch_counters(c, h)) return rc;
        if (h[C_ERR] & ~ERR_CAP_INTER) { (void)sync_and_check(c, h); return SZ_E_CAPACITY; }
        done = s_end;
        break;
      }
      continue;
    }
    if (h[C_STOP] > 0 && h[C_STOP] < s_end) {
      // a tag ended the enqueued steps after step k: the state behind it (GEO(k) has run ahead: parents un-swapped), then either the end of
      // the batch (the caller's stop) or -- a batch that runs through -- the rest of it, started like a batch (the ghosts know the tag now)
      const int k = h[C_STOP] - 1;
      if (plan.user_stop) { epilogue(k, true); done = k + 1; if (int rc = fetch_counters(c, h)) return rc; break; }
      pipe_adopt(c, par(k + 1));
      { State T = pipe_state(c, par(k + 1)); T.step = 0; hipLaunchKernelGGL(sz_k_unswap, dim3(grid_for(N, 128)), dim3(128), 0, c->stream, T, pipe_alt(c, par(k), 0), N); }
      (void)clear_stop_words(c, W_STOP | W_FRCSTOP);
      s0 = k + 1; need_prologue = true;
      continue;
    }
    if (s_end < nsteps && h[C_STOP] == 0) {          // the first step ran on its own (a parent might have been tagged before the batch): the rest
      s0 = s_end; s_end = nsteps; need_prologue = true;
      continue;
    }
    done = h[C_STOP] > 0 ? std::min(h[C_STOP], nsteps) : s_end;
    break;
  }
  // ---- the batch is over: state in set par(done); rows of step done - 1 assembled (region par(done - 1))
  const int qlast = par(done - 1);
  if (h[C_ERR] & ERR_CAP_INTER) {          // a floe of the last step has more rows than the stride holds
    int z = 0; (void)hipMemcpy(S0.cnt + C_ERR, &z, sizeof(int), hipMemcpyHostToDevice);
    if (int rc = regrow_rows(c, h, [&] { State R = pipe_state(c, qlast); R.step = 0; R.vxy = S0.vxy; return R; })) return rc;
  }
  {          // the per-row results of the last step to the rows straight behind the parents; its links become the context's; ghosts off
    const State R = pipe_state(c, qlast);
    const int G = h[C_NGHOSTS];
    if (R.goff != 0 && G > 0) {
      State T = c->S; T.gh = R.gh; T.ngh = R.ngh; T.step = 0;
      hipLaunchKernelGGL(sz_k_rows_home, dim3(grid_for((long long)G * S0.maxnb, 256)), dim3(256), 0, c->stream, T, N, G, R.goff);
      hipLaunchKernelGGL(sz_k_rows_rename, dim3(grid_for((long long)(N + G) * S0.maxnb, 256, 8192)), dim3(256), 0, c->stream, T, N, G, R.goff);
    }
    // (the links of the last step are set qlast's; the context's own set is par(done)'s: sz_k_remove_ghosts saves and clears what it is given)
    State T = c->S; T.gh = R.gh; T.ngh = R.ngh; T.step = 0; T.retry_stop = 0;
    hipLaunchKernelGGL(sz_k_remove_ghosts, dim3(grid_for(S0.capM, 256)), dim3(256), 0, c->stream, T, 0);
    Clears tail(c);
    tail.add(c->pb[1 - qlast].ngh, (size_t)S0.capM * sizeof(int));
    tail.add(c->pb[1 - qlast].gh, (size_t)MAX_GHOSTS * S0.capM * sizeof(int), 0xff);
    tail.launch(c);
  }
  {
    const int keepG = h[C_NGHOSTS];
    int rc = sync_and_check(c, h);
    h[C_NGHOSTS] = keepG;
    if (rc) return rc;
  }
  *done_out = done; *slot_out = qlast;
  // (h[C_STOP]: the caller's view -- a batch that ran through ended at nsteps)
  if (!plan.user_stop) h[C_STOP] = 0;
  return SZ_OK;
}
}  // namespace


// ---------------------------------------------------------------- fracture criteria (sz_fracture.hpp)
int sz_set_fracture(sz_ctx* c, int32_t kind, int32_t dt, double pstar, double cc, int32_t npts, const double* px, const double* py,
                    double alpha, double min_floe_area) {
  if (!c) return SZ_E_ARG;
  if (kind != SZ_FRAC_OFF && kind != SZ_FRAC_HIBLER && kind != SZ_FRAC_POLYGON) { c->err = "sz_set_fracture: kind is not an SZ_FRAC_* value"; return SZ_E_ARG; }
  if (kind == SZ_FRAC_OFF) { c->frac_kind = SZ_FRAC_OFF; return SZ_OK; }
  if (dt <= 0) { c->err = "sz_set_fracture: dt (FractureSettings.Δt) must be positive"; return SZ_E_ARG; }
  if (kind == SZ_FRAC_POLYGON && (npts < 4 || npts > FRAC_MAXPTS || !px || !py)) {
    c->err = "sz_set_fracture: a criterion polygon is a closed ring of 4 to 128 points"; return SZ_E_ARG;
  }
  if (!(min_floe_area > 0.0)) { c->err = "sz_set_fracture: min_floe_area must be positive"; return SZ_E_ARG; }
  (void)hipSetDevice(c->device);
  if (!c->frac_d) HIPCHK(c, hipMalloc(&c->frac_d, sizeof(FracDev)));
  FracDev h{};
  if (kind == SZ_FRAC_HIBLER) {
    // the points of range(0, 2π, length = 100): k (2π) / 99 rounded once (extended precision here; Julia's range computes them in
    // twice-precision arithmetic), and ring_coords[end] = ring_coords[1]
    const long double two_pi = (long double)(2.0 * M_PI);
    for (int k = 0; k < FRAC_HIBLER_PTS; k++) {
      const double a = k == FRAC_HIBLER_PTS - 1 ? 0.0 : (double)(two_pi * k / (long double)(FRAC_HIBLER_PTS - 1));
      h.ct[k] = cos(a); h.st[k] = sin(a);
    }
    npts = FRAC_HIBLER_PTS;
  } else {
    for (int k = 0; k < npts; k++) { h.px[k] = px[k]; h.py[k] = py[k]; }
  }
  HIPCHK(c, hipMemcpyAsync(c->frac_d, &h, sizeof(FracDev), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->frac_kind = kind; c->frac_dt = dt; c->frac_npts = npts;
  c->frac_pstar = pstar; c->frac_c = cc; c->frac_alpha = alpha; c->frac_min_area = min_floe_area;
  return SZ_OK;
}
// the per-parent buffers for the field as it is (hostN parents)
static int frac_ensure(sz_ctx* c) {
  if (c->frac_cap >= c->hostN && c->frac_flag) return SZ_OK;
  (void)hipFree(c->frac_flag); (void)hipFree(c->frac_idx); c->frac_flag = nullptr; c->frac_idx = nullptr; c->frac_cap = 0;
  const int cap = std::max(c->hostN, 1);
  HIPCHK(c, hipMalloc(&c->frac_flag, (size_t)cap));
  HIPCHK(c, hipMalloc(&c->frac_idx, (size_t)cap * sizeof(int)));
  c->frac_cap = cap;
  return SZ_OK;
}
static FracArgs frac_args(const sz_ctx* c) {
  FracArgs F;
  F.d = c->frac_d; F.flag = c->frac_flag; F.idx = c->frac_idx;
  F.kind = c->frac_kind; F.npts = c->frac_npts; F.n = c->hostN;
  F.pstar = c->frac_pstar; F.c = c->frac_c; F.alpha = c->frac_alpha; F.min_area = c->frac_min_area;
  F.rc = cos(M_PI / 4); F.rs = sin(M_PI / 4);
  return F;
}
// ASYNC: one evaluation of the criterion on the parents; T.step = the batch-relative step it ends (a candidate stops the batch there)
static void frac_launch(sz_ctx* c, const State& T) {
  const FracArgs F = frac_args(c);
  hipLaunchKernelGGL(sz_k_frac_criterion, dim3(1), dim3(FRAC_TPB), 0, c->stream, T, F);
  hipLaunchKernelGGL(sz_k_frac_test, dim3(grid_for(std::max(c->hostN, 1), 256, 2048)), dim3(256), 0, c->stream, T, F);
}
int sz_fracture_candidates(sz_ctx* c, int32_t* n, int32_t* idx) {
  if (n) *n = 0;
  if (!c || !n) return SZ_E_ARG;
  if (!c->have_floes) { c->err = "sz_fracture_candidates: no floes uploaded"; return SZ_E_STATE; }
  if (c->frac_kind == SZ_FRAC_OFF) { c->err = "sz_fracture_candidates: no fracture criterion set (sz_set_fracture)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  if (int rc = frac_ensure(c)) return rc;
  State T = c->S; T.step = 0;
  frac_launch(c, T);
  hipLaunchKernelGGL(sz_k_frac_compact, dim3(1), dim3(FRAC_TPB), 0, c->stream, frac_args(c));
  int cnt = 0;
  HIPCHK(c, hipMemcpyAsync(&cnt, &c->frac_d->count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  int rc = sync_and_check(c);
  if (rc) return rc;
  if (cnt < 0 || cnt > c->hostN) { c->err = "sz_fracture_candidates: bad candidate count"; return SZ_E_HIP; }
  if (idx && cnt > 0) {
    HIPCHK(c, hipMemcpyAsync(idx, c->frac_idx, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *n = cnt;
  return SZ_OK;
}
int sz_debug_fracture_mean(sz_ctx* c, double* mean_h, double* p) {
  if (!c || !c->frac_d) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  double h2[2];
  HIPCHK(c, hipMemcpyAsync(h2, &c->frac_d->mean_h, sizeof(h2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (mean_h) *mean_h = h2[0];
  if (p) *p = h2[1];
  return SZ_OK;
}

int sz_debug_pipelined(sz_ctx* c) { return c ? c->last_pipelined : 0; }
int sz_debug_totals_mode(sz_ctx* c) { return c ? c->last_totals_mode : 0; }

// The side effects of a batch's start, from the plan: the stop words, the cells, the ghosts' form, the buffers and rings the steps read, the
// records and totals.  The per-batch modes it sets are put back by the caller's BatchModes scope.  *gl0: the candidate list the batch starts on.
static int batch_enter(sz_ctx* c, const BatchPlan& p, int* gl0) {
  c->S.stop_on_tags = p.user_stop ? 1 : 0;
  HIPCHK(c, clear_stop_words(c, p.stop_mask));
  if (p.sg) use_static_grid(c);
  // (ghosts a process-mode sz_add_ghosts left attached are dropped first: the list pass only visits the parents that get new ones)
  if (p.gl && p.periodic && c->hostM != c->hostN) hipLaunchKernelGGL(sz_k_remove_ghosts, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, 0);
  if (p.gl && !p.gi) use_ghost_list(c); else c->gl_valid = false;
  *gl0 = c->gl_cur;
  c->S.ginline = p.gi ? 1 : 0; if (p.gi) c->S.famrec = 1;
  if (c->gi_pending && c->gi_valid && !p.coll) { int rc = gi_fetch(c); if (rc) return rc; }      // (the key tables are about to be reused)
  c->gi_pending = false; if (p.coll) c->gi_valid = false;    // (this batch's rows replace the old ones; batch_leave sets it again if they carry order keys of inline ghosts)
  if (p.mixed) { int rc = ensure_mixed(c); if (rc) return rc; }
  if (c->precision == 0 && !c->two_way && c->have_fields) { int rc = ensure_block_points(c); if (rc) return rc; }
  if (!p.body) world_rings(c);
  c->S.body_rings = p.body ? 1 : 0;
  // the records are seeded here from the columns (before the ghost seed: the maker updates the records of the parents it visits)
  c->S.crec = p.cr ? c->crec_buf : nullptr; c->crec_was_live = p.cr;
  c->last_pipelined = 0;
  if (!p.pipe) c->crec_current = false;          // (the three-launch steps seed the records they use; they may not keep the twin set's)
  if (p.cr && !p.pipe) seed_records(c, c->S, c->hostN);
  // the ghosts of the first step, from the parents as they lie (after the rings are in the batch's form)
  if (p.gi && !p.pipe && !p.own_first_ghosts) { if (int rc = reseed_inline_ghosts(c, 0)) return rc; }
  c->S.facc = p.facc_on ? c->facc_buf : nullptr; c->S.kexp = force_scale_exp(c); c->reduce_mode = p.reduce_mode; c->last_totals_mode = p.reduce_mode;
  if (p.facc_on && !p.pipe) { if (int rc = clear_totals(c)) return rc; }          // (a pipelined batch clears them with the rest of its prologue: one launch)
  if (p.frac) { if (int rc = frac_ensure(c)) return rc; }
  return SZ_OK;
}

// A batch of three-launch steps (neighbour search, narrow phase, integrator).  The contract of step_batch_pipelined: h = the counter block after
// the batch, *done = the steps that ran, *slot_out = the allocator slot of the last step's inline ghosts; the context's state is complete when
// it returns (rows of the last step assembled, ghosts detached).  It starts again from inside: lists grown, the first step alone, a pause for
// the largest narrow variant.
static int step_batch_three_launch(sz_ctx* c, const BatchPlan& p, int gl0, int nsteps, int tstep0, int dt, int coupling_dt, int flags, int* h, int* done_out, int* slot_out) {
  const bool periodic = p.periodic, coll = p.coll, sg = p.sg, gl = p.gl, gi = p.gi, cr = p.cr, facc_on = p.facc_on, rfree = p.rfree, frac = p.frac;
  bool lean = p.lean;
  int s_end = p.first_alone ? 1 : nsteps;
  const int callid0 = c->callid; c->callid += nsteps;          // (step s of this batch is collision call callid0 + s + 1, also when it is run again)
  for (int s0 = 0, mid = 0;;) {
    c->S.retry_stop = lean ? 1 : 0;
    for (int s = s0; s < s_end; s++) {
      int tstep = tstep0 + s;
      c->S.step = s + 1; c->S.callid = callid0 + s + 1;
      const bool resume = mid && s == s0;
      const bool coupling = coupling_at(flags, coupling_dt, tstep);
      const bool overlap = coupling && !c->two_way && (c->overlap_forcing >= 0 ? c->overlap_forcing != 0 : (c->hostN > 65536 && c->precision == 0 && coll));
      // with collisions on, the ghosts of step s are detached by the ghost kernels of step s+1 (nothing
      // in between looks past the parents) and committed by the bounds kernel: two launches less
      // The forcings only read the floes' state at the start of the step (after the ghost pass has wrapped the parents that left the
      // domain) and write columns nothing reads before the update: they can run beside the collision kernels (second stream, fork
      // after the ghost pass) or inside one of their launches.
      const int fmode = forcing_fuse_mode(c, coupling && !overlap && coll && !c->two_way);
      if (!resume) {          // (a paused step has all of this behind it)
        if (coll && !gi) stage_ghosts(c, true, sg, gl);
        // (after the ghost pass, like the reference's timestep_coupling!: a parent that has just swapped with its ghost is sampled where it
        //  now lies -- the same lattice values as at its image, but the interpolation weights come from other coordinates)
        if (coupling && !overlap && !fmode) stage_forcing(c, dt);
        if (overlap) stage_forcing_fork(c);
        if (coupling) c->forcing_where = fmode;
      }
      c->S.gslot = s & 1;
      // (the totals of the rows the inline makers allocated for this step are cleared by its neighbour search when it runs on collision records;
      //  without them -- lists wider than MAXNB -- here)
      if (facc_on && gi && !(cr && c->S.maxnb <= MAXNB) && !resume) (void)hipMemsetAsync(c->facc_buf + (size_t)FX_WORDS * c->hostN, 0, (size_t)FX_WORDS * (c->S.capM - c->hostN) * sizeof(long long), c->stream);
      if (coll) collisions_step(c, c->hostN, dt, periodic && !sg, sg, resume ? 0 : fmode, lean, resume);
      if (overlap && !resume) stage_forcing_join(c);
      // (inline ghosts: the last step of the batch makes none -- there is no step to make them for, and the cell lists stay the parents')
      // a fracture step (fracture_floes!, simulation.jl:172-183) ends the batch when the criterion finds a candidate -- known only after the
      // update: the step runs as a batch's last one (its ghosts stay, none are made for a next step), and the next step is started behind
      // the test by launches that return at once when it has stopped the batch (sz_fracture.hpp)
      const bool fstep = is_fracture_step(frac ? c->frac_dt : 0, tstep);
      const bool fcut = fstep && s + 1 < s_end;
      c->acc_mode = integrator_acc_mode(facc_on, rfree, s + 1 == s_end || fcut);
      stage_integrate(c, dt, !coll, coupling, sg, gl && !gi ? 1 - c->gl_cur : -1, gi && s + 1 < s_end && !fcut ? 1 - (s & 1) : -1);
      if (gl && !gi) c->gl_cur ^= 1;
      if (fstep) {
        frac_launch(c, c->S);
        if (fcut && gi) {
          State T = c->S; T.step = s + 2;
          if (coll && periodic) hipLaunchKernelGGL(sz_k_frac_resume_remove, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, T);
          (void)hipMemsetAsync(c->S.galloc + ((s + 1) & 1) * 16, 0, 2 * sizeof(unsigned long long), c->stream);
          hipLaunchKernelGGL(sz_k_frac_resume_seed, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, T, (s + 1) & 1, c->hostN);
        }
      }
    }
    c->S.step = 0;
    // floe.interactions of the step that ended the batch (reduce-free steps): one launch for the whole batch
    if (rfree) stage_reduce(c, 1, c->hostN, dt, c->hostN + 3 * c->gl_est + c->hostN / 64 + 32, true);
    if (coll && periodic) hipLaunchKernelGGL(sz_k_remove_ghosts, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, 0);
    int rc = sync_and_check(c, h);
    if (rfree && rc == SZ_E_CAPACITY && c->last_err_bits == ERR_CAP_INTER && h[C_RETRYSTOP] == 0) {
      // a floe of that last step has more rows than the stride holds: the launch runs again on the parents with the ghost links
      // sz_k_remove_ghosts has put aside
      int h2[C_COUNT];
      rc = regrow_rows(c, h2, [&] { State R = c->S; R.ngh = c->S.ngh_save; R.gh = c->S.gh_save; return R; });
    }
    if (rc == SZ_E_CAPACITY && growable(c->last_err_bits) && h[C_RETRYSTOP] > 0 && coll) {
      // A list outgrown inside step h[C_RETRYSTOP] (neighbours per floe, pair items, rows per floe): the batch paused there before anything
      // of the floes' state changed (capacity_stop()).  Larger lists, then that step and the rest of the batch again, from the parents as
      // they lie -- exactly as a batch that starts at that step would (cells, the step's ghosts): the reference's lists grow (collisions.jl:290-296).
      if ((rc = grow_lists(c, c->last_err_bits))) return rc;
      s0 = h[C_RETRYSTOP] - 1; mid = 0;
      (void)clear_stop_words(c, W_RETRYSTOP); (void)clear_stop_words(c, W_STOP);
      if (facc_on && (rc = clear_totals(c))) return rc;
      c->grid_live = false; use_static_grid(c);
      if (cr) seed_records(c, c->S, c->hostN);
      if (gi) { if ((rc = reseed_inline_ghosts(c, s0 & 1))) return rc; }
      else if (gl) { c->gl_valid = false; use_ghost_list(c); }
      continue;
    }
    if (rc) return rc;
    if ((!lean || h[C_RETRYSTOP] == 0) && s_end < nsteps && h[C_STOP] == 0) {
      // the first step ran on its own (a parent might have been tagged already) and nothing ended the batch: the rest of it, from the floes
      // as they lie -- the cells hold the parents (the step made no ghosts), the ghosts of the next step are seeded as at a batch's start
      s0 = s_end; s_end = nsteps; mid = 0;
      if (gi && (rc = reseed_inline_ghosts(c, s0 & 1))) return rc;
      continue;
    }
    if (!lean || h[C_RETRYSTOP] == 0) break;
    // paused after the narrow launch of step h[C_RETRYSTOP]: that variant is in from now on
    c->retry_seen = true; lean = false;
    s0 = h[C_RETRYSTOP] - 1; mid = 1;
    if (gl && !gi) c->gl_cur = (gl0 + s0) & 1;
    (void)clear_stop_words(c, W_RETRYSTOP);
  }
  *done_out = h[C_STOP] > 0 ? std::min(h[C_STOP], nsteps) : nsteps; *slot_out = (*done_out - 1) & 1;
  return SZ_OK;
}

// What a batch leaves behind, and who reads it:
//   maybe_tagged      a parent may carry a tag: the next plan's first_alone
//   last_stopped      a tag ended the batch
//   last_pipelined    sz_debug_pipelined, sz_narrow_kernel_name
//   crec_current      the records of both sets follow the columns: the next pipelined prologue does not seed them (every call outside the
//                     resident steps drops it: leave_resident).  After a tag stop the un-swap rewrote a few: seeded again next time
//   rings_stale       the world rings lag the poses: world_rings, before anything reads them
//   inter_any / inter_lost   floe.interactions on the device is the batch's: need_interactions, the downloads
//   gl_cur / gl_est   the candidate list the last step that RAN has filled, and how long it is: use_ghost_list, ghost_list_wanted, the list pass
//   gi_pending, gi_pending_n, gi_pending_slot, gi_valid   the order keys of the last step's inline ghosts, not fetched yet: gi_fetch
//   grid_live         the cells hold the parents as they lie: use_static_grid
//   fuse_lists, gl_valid   status.fuse_idx of the step that ended the batch, replayed on the host; the replay may change tags
static int batch_leave(sz_ctx* c, const BatchPlan& p, int gl0, const int* h, int done, int slot, int nsteps, int tstep0, int coupling_dt, int flags) {
  if (p.coll && (h[C_STOP] > 0 || !p.user_stop)) c->maybe_tagged = true;
  c->last_stopped = h[C_STOP] > 0;
  c->last_pipelined = p.pipe; c->crec_current = p.pipe && done == nsteps;
  if (p.body && nsteps > 0) c->rings_stale = true;
  if (p.coll) { c->inter_any = true; c->inter_lost = false; }
  if (p.gl && !p.gi) { c->gl_cur = (gl0 + done) & 1; c->gl_est = h[C_NGCAND + c->gl_cur]; }
  if (p.gi) {               // the order keys of the last step's ghosts are what the host needs to number them as the reference does:
    // they are fetched when somebody asks for numbers (gi_fetch: downloads, the fuse replay) -- most batches end without
    c->gi_pending_n = done > 0 ? h[C_NGHOSTS] : 0; c->gi_pending_slot = slot; c->gi_pending = true;
    if (p.coll) c->gi_valid = done > 0;
    c->gl_est = std::max(c->gl_est, c->gi_pending_n);        // (sizes the list pass should the next batch use it)
  }
  // stopped early: the step that ended the batch has binned ghosts (inline makers, the pipelined update) for a step that did not come
  if ((p.gi || p.pipe) && done < nsteps) c->grid_live = false;
  // status.fuse_idx of the step that ended the batch: the reference's serial propagation, replayed on the host as
  // sz_timestep_collisions does (only that step can have produced fuse pairs: the batch stops on the first tag)
  int rc = SZ_OK;
  if (p.coll && done > 0 && (h[C_STOP] > 0 || !p.user_stop)) {
    rc = host_fuse_fixup(c, h, true, true, coupling_at(flags, coupling_dt, tstep0 + done - 1));
    c->fuse_lists.resize(c->hostM);
    c->gl_valid = false;          // the replay may have changed status tags
  }
  return rc;
}

// One batch of resident steps (sz_step without welding, or one of the segments sz_step cuts a batch with welding into): checks, plan, enter,
// one driver, leave
static int step_segment(sz_ctx* c, int32_t nsteps, int32_t tstep0, int32_t dt, int32_t coupling_dt, int32_t flags, int32_t* steps_done) {
  if (steps_done) *steps_done = 0;
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (nsteps < 0) return SZ_E_ARG;
  if ((flags & SZ_COUPLING_ON) && !c->have_fields) { c->err = "sz_set_fields must be called before coupling"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  if (c->two_way && (flags & SZ_COUPLING_ON)) {
    if (c->S.tiled) { c->err = "tiled contexts couple through sz_tile_step + sz_two_way_partial / sz_two_way_finish"; return SZ_E_STATE; }
    if (!c->temps_set) { c->err = "two-way coupling needs sz_set_temps (after the sz_set_fields that fixed the lattice shape)"; return SZ_E_STATE; }
    int rc = ensure_two_way(c); if (rc) return rc;
  }
  if (!(flags & SZ_COLLISIONS_ON)) { if (int rc = need_interactions(c)) return rc; }
  c->ghosts_staged = false; c->rr_rows = false;          // (a batch detaches the ghosts it finds and leaves its own last step's rows)
  const BatchPlan plan = plan_batch(c, nsteps, flags);
  BatchModes modes(c);
  int h[C_COUNT], gl0 = 0, done = 0, slot = 0; bool rest = false;
  if (int rc = batch_enter(c, plan, &gl0)) return rc;
  if (plan.pipe) {
    if (int rc = step_batch_pipelined(c, plan, nsteps, tstep0, dt, coupling_dt, flags, h, &done, &slot, &rest)) return rc;
    if (rest) {          // the lists outgrew the pipelined launches in step `done`: the rest of the batch as a batch of its own (not eligible now;
                         //  its scope starts from the process-mode values)
      int more = 0;
      const int rc = step_segment(c, nsteps - done, tstep0 + done, dt, coupling_dt, flags, &more);
      if (steps_done) *steps_done = done + more;
      return rc;
    }
  } else if (int rc = step_batch_three_launch(c, plan, gl0, nsteps, tstep0, dt, coupling_dt, flags, h, &done, &slot)) return rc;
  if (steps_done) *steps_done = done;
  return batch_leave(c, plan, gl0, h, done, slot, nsteps, tstep0, coupling_dt, flags);
}

// ---------------------------------------------------------------- welding overlap table (sz_weld.hpp)
int sz_set_welding(sz_ctx* c, int32_t n, const int32_t* dts, const int32_t* nxs, const int32_t* nys, double max_weld_area) {
  if (!c) return SZ_E_ARG;
  if (n == 0) { c->weld_dts.clear(); c->weld_nxs.clear(); c->weld_nys.clear(); return SZ_OK; }
  if (n < 0 || !dts || !nxs || !nys) { c->err = "sz_set_welding: n sets need dts, nxs and nys"; return SZ_E_ARG; }
  for (int k = 0; k < n; k++) {
    if (dts[k] <= 0) { c->err = "sz_set_welding: every dt (WeldSettings.Δts) must be positive"; return SZ_E_ARG; }
    if (nxs[k] < 1 || nys[k] < 1) { c->err = "sz_set_welding: every Nx, Ny must be at least 1 (bin_floe_centroids asserts it)"; return SZ_E_ARG; }
  }
  if (!(max_weld_area > 0.0)) { c->err = "sz_set_welding: max_weld_area must be positive"; return SZ_E_ARG; }
  c->weld_dts.assign(dts, dts + n); c->weld_nxs.assign(nxs, nxs + n); c->weld_nys.assign(nys, nys + n);
  c->weld_max_area = max_weld_area;
  return SZ_OK;
}

namespace {
// the pass's buffers for the parents as they are, `need` pairs and `cells` search cells
int weld_ensure(sz_ctx* c, int need, int cells) {
  const int N = std::max(c->hostN, 1);
  if (c->weld.d && N <= c->weld_capN && cells <= c->weld_cells && need <= c->weld_cap) return SZ_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_pool(c->weld_allocs);
  c->weld = WeldArgs{}; c->weld_capN = c->weld_cells = c->weld_cap = 0;
  const size_t cap = (size_t)std::max((long long)need, 8LL * N + 1024);
  if (cap > (size_t)1 << 30) { c->err = "welding: candidate pair count overflow"; return SZ_E_CAPACITY; }
  Pool& P = c->weld_allocs; WeldArgs& W = c->weld; int rc;
  if ((rc = dalloc(c, &W.d, 1, P)) || (rc = dalloc(c, &W.bin, N, P)) || (rc = dalloc(c, &c->weld_bounds, 8, P)) ||
      (rc = dalloc(c, &c->weld_cell_cnt, (size_t)cells + 1, P)) || (rc = dalloc(c, &c->weld_cell_ovf, (size_t)cells + 1, P)) ||
      (rc = dalloc(c, &c->weld_cell_slots, (size_t)cells * CELL_K, P)) || (rc = dalloc(c, &c->weld_cell_items, N, P)) ||
      (rc = dalloc(c, &W.keys_in, cap, P)) || (rc = dalloc(c, &W.keys, cap, P)) || (rc = dalloc(c, &W.area, cap, P)) || (rc = dalloc(c, &W.retry, cap, P)) ||
      (rc = dalloc(c, &W.ti, cap, P)) || (rc = dalloc(c, &W.tj, cap, P)) || (rc = dalloc(c, &W.ta, cap, P))) { W.d = nullptr; return rc; }
  c->weld_capN = N; c->weld_cells = cells; c->weld_cap = (int)cap; W.cap = (int)cap;
  return SZ_OK;
}
// The overlap table of the parents as they lie, for nx x ny bins: *ntable entries in c->weld.ti / tj / ta.  Synchronous; reads the floes' columns and
// rings, writes nothing but its own buffers (a batch that goes on behind it finds the state as the steps left it).
int weld_pass(sz_ctx* c, int nx, int ny, double max_area, int* ntable) {
  *ntable = 0;
  State& S = c->S;
  const int N = c->hostN;
  if (N <= 0) { c->err = "welding: no floes"; return SZ_E_STATE; }
  // (k n + i) n + j must fit an unsigned 64-bit key
  if ((long double)nx * (long double)ny * (long double)N * (long double)N >= 9.0e18L) { c->err = "welding: Nx * Ny * N^2 does not fit the 64-bit pair key"; return SZ_E_ARG; }
  const double rm = std::max(c->rmax_max, c->rmax_hint);
  if (!(rm > 0.0) || !(S.gxf > S.gx0) || !(S.gyf > S.gy0)) { c->err = "welding: needs the floes' rmax and the grid extents (sz_set_fields)"; return SZ_E_STATE; }
  // search cells over the grid's box, at least 2 max(rmax) wide (setup_grid's rule), indices clamped: no periodic wrap in this search
  const double cmin = 2.0 * rm * (1.0 + 1e-9);
  long long ncx = std::max(1LL, (long long)std::floor(std::min((S.gxf - S.gx0) / cmin, 1e6)));
  long long ncy = std::max(1LL, (long long)std::floor(std::min((S.gyf - S.gy0) / cmin, 1e6)));
  const long long cell_max = std::max(4LL * N, 1024LL);
  while (ncx * ncy > cell_max) { ncx = std::max(1LL, ncx / 2); ncy = std::max(1LL, ncy / 2); }
  const int cells = (int)(ncx * ncy);
  double* g = c->weld_h_grid;
  g[0] = S.gx0; g[1] = S.gy0; g[2] = (S.gxf - S.gx0) / (double)ncx; g[3] = (S.gyf - S.gy0) / (double)ncy; g[4] = (double)ncx; g[5] = (double)ncy; g[6] = 0.0; g[7] = 0.0;
  world_rings(c);
  int need = 0;
  for (int round = 0;; round++) {
    if (int rc = weld_ensure(c, need, cells)) return rc;
    WeldArgs& W = c->weld;
    W.n = N; W.nx = nx; W.ny = ny; W.max_area = max_area;
    State T = S; T.step = 0;
    T.bounds = c->weld_bounds; T.cell_cnt = c->weld_cell_cnt; T.cell_slots = c->weld_cell_slots; T.cell_ovf = c->weld_cell_ovf; T.cell_items = c->weld_cell_items;
    c->weld_h = WeldDev{ N, 0, 0, 0 };
    HIPCHK(c, hipMemcpyAsync(W.d, &c->weld_h, sizeof(WeldDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->weld_bounds, g, 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->weld_cell_cnt, 0, ((size_t)cells + 1) * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->weld_cell_ovf, 0, ((size_t)cells + 1) * sizeof(int), c->stream));
    const int nb = grid_for(N, 256, 2048);
    hipLaunchKernelGGL(sz_k_weld_oob, dim3(nb), dim3(256), 0, c->stream, T, W);
    hipLaunchKernelGGL(sz_k_weld_bins, dim3(nb), dim3(256), 0, c->stream, T, W);
    hipLaunchKernelGGL(sz_k_weld_pairs, dim3(nb), dim3(256), 0, c->stream, T, W);
    HIPCHK(c, hipMemcpyAsync(&c->weld_h, W.d, sizeof(WeldDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int P = c->weld_h.npairs;
    if (P < 0) { c->err = "welding: candidate pair count overflow"; return SZ_E_CAPACITY; }
    if (P > W.cap) {          // the pair arrays grow like the other lists; nothing is truncated
      if (round > 0) { c->err = "welding: the pair arrays did not grow enough"; return SZ_E_CAPACITY; }
      need = P + P / 4;
      continue;
    }
    c->weld_npairs = P;
    if (P > 0) {
      const unsigned long long top = (unsigned long long)nx * ny * (unsigned long long)N * (unsigned long long)N;
      unsigned bits = 1; while (bits < 64 && (top >> bits)) bits++;
      size_t tmp_bytes = 0;
      HIPCHK(c, rocprim::radix_sort_keys(nullptr, tmp_bytes, W.keys_in, W.keys, (size_t)P, 0u, bits, c->stream));
      if (tmp_bytes > c->weld_tmp_bytes) {
        (void)hipFree(c->weld_tmp); c->weld_tmp = nullptr; c->weld_tmp_bytes = 0;
        HIPCHK(c, hipMalloc(&c->weld_tmp, tmp_bytes + tmp_bytes / 2));
        c->weld_tmp_bytes = tmp_bytes + tmp_bytes / 2;
      }
      HIPCHK(c, rocprim::radix_sort_keys(c->weld_tmp, tmp_bytes, W.keys_in, W.keys, (size_t)P, 0u, bits, c->stream));
      hipLaunchKernelGGL((sz_k_weld_area<WELD_G0, WELD_CAP0, WELD_KC0, WELD_RC0, WELD_RM0, 0>), dim3(grid_for(P, 64 / WELD_G0, 1 << 16)), dim3(64), 0, c->stream, S, W, P, WeldRowRings{});
      // (what the small working set handed on; its count lives on the device: a fixed grid, most of it returns at once)
      hipLaunchKernelGGL((sz_k_weld_area<WELD_G1, WELD_CAP1, WELD_KC1, WELD_RC1, WELD_RM1, 1>), dim3(grid_for(P, 1, 512)), dim3(64), 0, c->stream, S, W, P, WeldRowRings{});
      hipLaunchKernelGGL(sz_k_weld_table, dim3(1), dim3(WELD_TPB), 0, c->stream, W, P);
      HIPCHK(c, hipMemcpyAsync(&c->weld_h, W.d, sizeof(WeldDev), hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc = sync_and_check(c)) return rc;
    if (c->weld_h.ntable < 0 || c->weld_h.ntable > P) { c->err = "welding: bad table count"; return SZ_E_HIP; }
    *ntable = c->weld_h.ntable;
    return SZ_OK;
  }
}
int weld_query_checks(sz_ctx* c, const char* who, int32_t nx, int32_t ny) {
  if (!c) return SZ_E_ARG;
  if (nx < 1 || ny < 1) { c->err = std::string(who) + ": Nx and Ny must be at least 1"; return SZ_E_ARG; }
  if (!c->have_floes) { c->err = std::string(who) + ": no floes uploaded"; return SZ_E_STATE; }
  if (!c->have_domain || !c->have_fields) { c->err = std::string(who) + ": the bins need the domain's boundary kinds and the grid extents (sz_set_domain, sz_set_fields)"; return SZ_E_STATE; }
  if (c->S.tiled) { c->err = std::string(who) + ": tiled contexts do not compute welding overlaps (the bins span ranks)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  return sync_and_check(c);          // hostN current, nothing pending
}
}  // namespace

int sz_weld_overlaps(sz_ctx* c, int32_t nx, int32_t ny, double max_weld_area, int32_t* n, int32_t cap, int32_t* idx_i, int32_t* idx_j, double* inter_area) {
  if (n) *n = 0;
  if (!c || !n) return SZ_E_ARG;
  if (!(max_weld_area > 0.0)) { c->err = "sz_weld_overlaps: max_weld_area must be positive"; return SZ_E_ARG; }
  if (int rc = weld_query_checks(c, "sz_weld_overlaps", nx, ny)) return rc;
  int nt = 0;
  if (int rc = weld_pass(c, nx, ny, max_weld_area, &nt)) return rc;
  *n = nt;
  if (!idx_i && !idx_j && !inter_area) return SZ_OK;
  if (cap < nt) { c->err = "sz_weld_overlaps: cap is smaller than the table (*n)"; return SZ_E_ARG; }
  if (nt > 0) {
    if (idx_i) HIPCHK(c, hipMemcpyAsync(idx_i, c->weld.ti, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (idx_j) HIPCHK(c, hipMemcpyAsync(idx_j, c->weld.tj, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (inter_area) HIPCHK(c, hipMemcpyAsync(inter_area, c->weld.ta, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return SZ_OK;
}
int sz_debug_weld_bins(sz_ctx* c, int32_t nx, int32_t ny, int32_t* bin) {
  if (!c || !bin) return SZ_E_ARG;
  if (int rc = weld_query_checks(c, "sz_debug_weld_bins", nx, ny)) return rc;
  int nt = 0;
  if (int rc = weld_pass(c, nx, ny, INFINITY, &nt)) return rc;
  HIPCHK(c, hipMemcpy(bin, c->weld.bin, (size_t)c->hostN * sizeof(int), hipMemcpyDeviceToHost));
  return SZ_OK;
}
int sz_debug_weld_npairs(sz_ctx* c, int32_t* n) {
  if (!c || !n) return SZ_E_ARG;
  *n = c->weld_npairs;
  return SZ_OK;
}

// ---------------------------------------------------------------- removal and dissolution on the device (sz_remove.hpp)
int sz_set_removal(sz_ctx* c, int32_t on, int32_t max_vertices, double min_floe_area, double min_floe_height) {
  if (!c) return SZ_E_ARG;
  if (on && (max_vertices < 0 || !(min_floe_area >= 0.0) || !(min_floe_height >= 0.0))) { c->err = "sz_set_removal: max_vertices, min_floe_area and min_floe_height must not be negative"; return SZ_E_ARG; }
  c->rm_on = on != 0;
  if (on) { c->rm_max_vertices = max_vertices; c->rm_min_area = min_floe_area; c->rm_min_height = min_floe_height; }
  return SZ_OK;
}

namespace {
// The first half of a removal pass over the N parents as they lie, single context and tile alike: the arrays of RmArgs carved from the context's
// scratch, the flags, the scans and what sz_k_rm_rows derives from them -- A.d then holds the counts (not yet a verdict).
int rm_flag_rows(sz_ctx* c, int N, RmArgs& A) {
  State& S = c->S;
  int rc;
  world_rings(c);
  Pool& P = c->rm_allocs;
  reset_pool(P);
  A = RmArgs{};
  A.n = N; A.max_vertices = c->rm_max_vertices; A.min_area = c->rm_min_area; A.min_height = c->rm_min_height;
  const size_t n1 = (size_t)N + 2;
  if ((rc = dalloc(c, &A.d, 1, P)) || (rc = dalloc(c, &A.keep, n1, P)) || (rc = dalloc(c, &A.dis, n1, P)) || (rc = dalloc(c, &A.kv, n1, P)) || (rc = dalloc(c, &A.ks, n1, P)) ||
      (rc = dalloc(c, &A.newrow, n1, P)) || (rc = dalloc(c, &A.dpos, n1, P)) || (rc = dalloc(c, &A.ovoff, n1, P)) || (rc = dalloc(c, &A.osoff, n1, P)) ||
      (rc = dalloc(c, &A.src, n1, P)) || (rc = dalloc(c, &A.nvoff, n1, P)) || (rc = dalloc(c, &A.nsoff, n1, P)) || (rc = dalloc(c, &A.dlist, n1, P))) return rc;
  if (c->have_fields && c->dissolved) {
    A.x0 = S.gx0; A.y0 = S.gy0; A.dx = S.gdx; A.dy = S.gdy; A.Nx = S.Nx; A.Ny = S.Ny; A.dissolved = c->dissolved;
    A.per_e = c->h_kinds[SZ_EAST] == SZ_PERIODIC; A.per_n = c->h_kinds[SZ_NORTH] == SZ_PERIODIC;
  }
  HIPCHK(c, hipMemsetAsync(A.d, 0, sizeof(RmDev), c->stream));
  const int nb = grid_for(N, 256, 2048);
  hipLaunchKernelGGL(sz_k_rm_flags, dim3(nb), dim3(256), 0, c->stream, S, A);
  scan(c, A.keep, A.newrow, N, C_N, 0, -1);
  scan(c, A.dis, A.dpos, N, C_N, 0, -1);
  scan(c, A.kv, A.ovoff, N, C_N, 0, -1);
  scan(c, A.ks, A.osoff, N, C_N, 0, -1);
  hipLaunchKernelGGL(sz_k_rm_rows, dim3(nb), dim3(256), 0, c->stream, A);
  return SZ_OK;
}
// The second half, behind a verdict that lets the pass go ahead: the N parents compacted to the R.Nn that stay, through temporaries, and what is
// derived from the rows rebuilt as a migration rebuilds it (field_placed: as sz_upload_floes leaves it -- a tile is a plain context behind it,
// as behind any new field).  The capacities the context was carved with stay.
int rm_move_rows(sz_ctx* c, int N, const RmArgs& A, const RmDev& R) {
  State& S = c->S;
  Pool& P = c->rm_allocs;
  const int Nn = R.Nn, Vn = R.Vn, NSn = R.NSn;
  int rc;
  if (c->gi_pending && c->gi_valid) { if ((rc = gi_fetch(c))) return rc; }
  c->gi_pending = false;
  // ---- the rows into their new places, gathered beside the old ones first
  double** d_cols = nullptr; double *d_tmp = nullptr, *d_tsx = nullptr, *d_tsy = nullptr, *d_trows = nullptr; double2* d_tv = nullptr; int *d_torigin = nullptr, *d_tcnt = nullptr;
  if ((rc = dalloc(c, &d_cols, MIG_TAB_CAP, P)) || (rc = dalloc(c, &d_tmp, (size_t)MIG_NGATHER * Nn, P)) || (rc = dalloc(c, &d_tv, (size_t)Vn, P)) || (rc = dalloc(c, &d_tsx, (size_t)NSn, P)) ||
      (rc = dalloc(c, &d_tsy, (size_t)NSn, P)) || (rc = dalloc(c, &d_torigin, (size_t)Nn, P)) || (rc = dalloc(c, &d_tcnt, (size_t)Nn, P)) ||
      (rc = dalloc(c, &d_trows, (size_t)Nn * S.rowcap * 7, P))) return rc;
  const ColTable<double*> hcols = state_columns(S);
  HIPCHK(c, hipMemcpyAsync(d_cols, hcols.p, sizeof(hcols.p), hipMemcpyHostToDevice, c->stream));
  const int nbw = grid_for((long long)Nn * 64, 256, 4096);
  hipLaunchKernelGGL(sz_k_mig_gather, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, (const double*)nullptr, (const double*)nullptr,
                     (double* const*)d_cols, d_tmp);
  hipLaunchKernelGGL(sz_k_mig_points, dim3(nbw), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, (const double*)nullptr, (const double*)nullptr,
                     (const int*)A.nvoff, (const int*)A.nsoff, d_tv, d_tsx, d_tsy);
  hipLaunchKernelGGL(sz_k_rm_gather_rows, dim3(nbw), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, (const int*)c->origin, d_torigin, d_tcnt, d_trows);
  hipLaunchKernelGGL(sz_k_mig_scatter, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (double* const*)d_cols, (const double*)d_tmp);
  hipLaunchKernelGGL(sz_k_rm_scatter_rows, dim3(nbw), dim3(256), 0, c->stream, S, Nn, c->origin, (const int*)d_torigin, (const int*)d_tcnt, (const double*)d_trows);
  if (N > Nn) HIPCHK(c, hipMemsetAsync(S.inter_cnt + Nn, 0, (size_t)(N - Nn) * sizeof(int), c->stream));
  if (Vn) HIPCHK(c, hipMemcpyAsync(S.vxy, d_tv, (size_t)Vn * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(S.voff, A.nvoff, ((size_t)Nn + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  if (c->pts_N) {
    if (NSn) {
      HIPCHK(c, hipMemcpyAsync(S.sx, d_tsx, (size_t)NSn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(S.sy, d_tsy, (size_t)NSn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(S.soff, A.nsoff, ((size_t)Nn + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  }
  // ---- the field is placed: as behind the copies of sz_upload_floes (the estimates and bounds the context held still bound the floes that stay)
  const bool inter_any = c->inter_any, inter_lost = c->inter_lost;
  if ((rc = field_placed(c, Nn, 0, Vn, c->pts_N ? Nn : 0, std::min(Nn, c->gl_est), c->rmax_max, c->rmax_hint))) return rc;
  c->inter_any = inter_any; c->inter_lost = inter_lost;
  c->maybe_tagged = false; c->grid_live = false;
  c->max_ring = R.max_ring; if (c->pts_N) c->max_sub = R.max_sub;          // (as an upload of the floes that stay would find them)
  return SZ_OK;
}
// remove_floes! on the parents as they lie (no ghosts in the list, a single context).  *done = 0: declined, nothing has changed.  Two host
// synchronisations: the verdict (counts, what stays), then the end of the pass.
int remove_pass(sz_ctx* c, int* done, int* n_removed, int* n_dissolved) {
  *done = 0; *n_removed = 0; *n_dissolved = 0;
  const int N = c->hostN;
  int rc;
  if (N <= 0) return SZ_OK;          // (no floe would be left)
  RmArgs A;
  if ((rc = rm_flag_rows(c, N, A))) return rc;
  hipLaunchKernelGGL(sz_k_rm_dissolve, dim3(1), dim3(64), 0, c->stream, c->S, A);
  RmDev R{};
  HIPCHK(c, hipMemcpyAsync(&R, A.d, sizeof(RmDev), hipMemcpyDeviceToHost, c->stream));
  if ((rc = sync_and_check(c))) return rc;
  if (R.declined & RM_NO_LATTICE) { c->err = "sz_remove_floes: a floe dissolves, and the ocean.dissolved lattice needs the grid (sz_set_fields)"; return SZ_E_STATE; }
  if (R.declined) return SZ_OK;
  if (R.Nn <= 0 || R.Nn > N || R.Nn + R.n_removed + R.n_dissolved != N || R.Vn < 0 || R.NSn < 0) { c->err = "sz_remove_floes: bad counts"; return SZ_E_HIP; }
  *done = 1; *n_removed = R.n_removed; *n_dissolved = R.n_dissolved;
  if (R.Nn == N) return SZ_OK;          // nothing leaves, and every status is `active` already (no tag but remove / fuse exists)
  return rm_move_rows(c, N, A, R);
}
int removal_checks(sz_ctx* c, const char* who) {
  if (!c->have_floes) { c->err = std::string(who) + ": no floes uploaded"; return SZ_E_STATE; }
  if (c->S.tiled) { c->err = std::string(who) + ": the rows of a tiled context carry global numbers, and its pass is collective: sz_tile_remove_floes"; return SZ_E_STATE; }
  return SZ_OK;
}
}  // namespace

int sz_remove_floes(sz_ctx* c, int32_t* done, int32_t* n_removed, int32_t* n_dissolved) {
  if (done) *done = 0;
  if (n_removed) *n_removed = 0;
  if (n_dissolved) *n_dissolved = 0;
  if (!c || !done) return SZ_E_ARG;
  if (int rc = removal_checks(c, "sz_remove_floes")) return rc;
  (void)hipSetDevice(c->device);
  if (int rc = sync_and_check(c)) return rc;          // hostM / hostN current, nothing pending
  if (c->hostM != c->hostN) { c->err = "sz_remove_floes: ghosts are in the list (sz_remove_ghosts first): the pass runs over the parents alone"; return SZ_E_STATE; }
  leave_resident(c);
  int d = 0, nr = 0, nd = 0;
  if (int rc = remove_pass(c, &d, &nr, &nd)) return rc;
  *done = d;
  if (n_removed) *n_removed = nr;
  if (n_dissolved) *n_dissolved = nd;
  return SZ_OK;
}
int sz_upload_dissolved(sz_ctx* c, const double* dissolved) {
  if (!c || !dissolved) return SZ_E_ARG;
  if (!c->have_fields || !c->dissolved) { c->err = "sz_upload_dissolved: the lattice comes with the fields (sz_set_fields)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->dissolved, dissolved, (size_t)(c->S.Nx + 1) * (c->S.Ny + 1) * sizeof(double), hipMemcpyHostToDevice));
  return SZ_OK;
}
int sz_download_dissolved(sz_ctx* c, double* dissolved) {
  if (!c || !dissolved) return SZ_E_ARG;
  if (!c->have_fields || !c->dissolved) { c->err = "sz_download_dissolved: the lattice comes with the fields (sz_set_fields)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(dissolved, c->dissolved, (size_t)(c->S.Nx + 1) * (c->S.Ny + 1) * sizeof(double), hipMemcpyDeviceToHost));
  return SZ_OK;
}
int sz_download_origin(sz_ctx* c, int32_t* origin) {
  if (!c || !origin) return SZ_E_ARG;
  if (!c->have_floes || !c->origin) { c->err = "sz_download_origin: no floes uploaded"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  if (int rc = sync_and_check(c)) return rc;
  if (c->hostN > 0) HIPCHK(c, hipMemcpy(origin, c->origin, (size_t)c->hostN * sizeof(int), hipMemcpyDeviceToHost));
  return SZ_OK;
}

// ---------------------------------------------------------------- rows down, rows back (sz_splice.hpp)
namespace {
// rows[0..n): in [0, N), ascending without repeats (sorted) or merely without repeats
int sp_check_rows(sz_ctx* c, const char* who, const char* what, int n, const int32_t* rows, int N, bool sorted, const char* of = "parents") {
  std::vector<int> tmp;
  const int32_t* r = rows;
  if (!sorted && n > 1) { tmp.assign(rows, rows + n); std::sort(tmp.begin(), tmp.end()); r = tmp.data(); }
  for (int k = 0; k < n; k++) {
    if (r[k] < 0 || r[k] >= N) { c->err = std::string(who) + ": " + what + " names row " + std::to_string(r[k]) + ", outside the " + std::to_string(N) + " " + of; return SZ_E_ARG; }
    if (k && r[k] <= r[k - 1]) { c->err = std::string(who) + ": " + what + (r[k] == r[k - 1] ? " repeats row " + std::to_string(r[k]) : std::string(" is not ascending")); return SZ_E_ARG; }
  }
  return SZ_OK;
}
// order keys of the last step's inline ghosts, sorted (what an interaction row may name in place of a list number), fetched if pending
int sp_ghost_keys(sz_ctx* c, std::vector<long long>& sorted) {
  sorted.clear();
  if (!c->gi_valid) return SZ_OK;
  if (int rc = gi_fetch(c)) return rc;
  if (c->gi_valid) { sorted = c->gi_keys; std::sort(sorted.begin(), sorted.end()); }
  return SZ_OK;
}
}  // namespace

namespace {
// sz_download_rows (list = false: parents, ghost_off zeros) and sz_download_list_rows (list = true: any row of the list, the ghost lists with it)
int sp_download(sz_ctx* c, const char* who, bool list, int32_t n, const int32_t* rows, sz_floe_columns* f, int32_t* inter_off, double* inter_rows, int64_t* sizes3) {
  if (!c || n < 0 || (n > 0 && !rows)) return SZ_E_ARG;
  if (!c->have_floes) { c->err = std::string(who) + ": no floes uploaded"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = sync_and_check(c))) return rc;          // hostM / hostN current, nothing pending
  const int N = c->hostN, lim = list ? c->hostM : N;
  if ((rc = sp_check_rows(c, who, "rows", n, rows, lim, false, list ? "rows of the list" : "parents"))) return rc;
  world_rings(c);
  State& S = c->S;
  const size_t n1 = (size_t)n + 1;
  std::vector<int> off(4 * n1, 0);
  Pool& P = c->sp_allocs;
  reset_pool(P);
  int *d_rows = nullptr, *d_len = nullptr, *d_off = nullptr; double** d_cols = nullptr; double* d_out = nullptr;
  if (n > 0) {
    if ((rc = dalloc(c, &d_rows, n1, P)) || (rc = dalloc(c, &d_len, 4 * n1, P)) || (rc = dalloc(c, &d_off, 4 * n1, P)) || (rc = dalloc(c, &d_cols, MIG_TAB_CAP, P))) return rc;
    H2D(d_rows, rows, n, int);
    hipLaunchKernelGGL(sz_k_sp_sel_len, dim3(grid_for(n, 256)), dim3(256), 0, c->stream, S, (int)n, (const int*)d_rows, c->pts_N > 0 ? N : 0, list ? N : 0, d_len);
    for (int k = 0; k < 4; k++) scan(c, d_len + k * n1, d_off + k * n1, n, -1, n, -1);
    HIPCHK(c, hipMemcpyAsync(off.data(), d_off, 4 * n1 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  const size_t V = (size_t)off[n], NS = (size_t)off[n1 + n], R = (size_t)off[2 * n1 + n], G = (size_t)off[3 * n1 + n];
  if (sizes3) { sizes3[0] = (int64_t)V; sizes3[1] = (int64_t)NS; sizes3[2] = (int64_t)R; }
  if (!f) return SZ_OK;
  if (f->vert_off) for (size_t k = 0; k < n1; k++) f->vert_off[k] = off[k];
  if (f->sub_off) for (size_t k = 0; k < n1; k++) f->sub_off[k] = off[n1 + k];
  if (f->ghost_off) for (size_t k = 0; k < n1; k++) f->ghost_off[k] = off[3 * n1 + k];          // (zeros where the ghost lists are not asked for)
  if (inter_off) for (size_t k = 0; k < n1; k++) inter_off[k] = off[2 * n1 + k];
  if (n == 0) return SZ_OK;
  const size_t total = (size_t)SP_PACK_NCOL * n + 2 * V + 2 * NS + 7 * R + (G + 1) / 2;
  if ((rc = dalloc(c, &d_out, total, P))) return rc;
  const ColTable<double*> hcols = state_columns(S);
  HIPCHK(c, hipMemcpyAsync(d_cols, hcols.p, sizeof(hcols.p), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(sz_k_sp_pack, dim3(grid_for((long long)n * 64, 256, 4096)), dim3(256), 0, c->stream, S, (int)n, (const int*)d_rows, (const int*)d_off, (double* const*)d_cols, d_out);
  std::vector<double> out(total);
  HIPCHK(c, hipMemcpyAsync(out.data(), d_out, total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const ColTable<double*> dst = host_columns(*f);
  for (int q = 0; q < MIG_NSC; q++) if (dst.p[q]) memcpy(dst.p[q], &out[(size_t)q * n], (size_t)n * sizeof(double));
  for (int t = 0; t < MIG_NTEN; t++) if (double* td = dst.p[MIG_NSC + t]) for (int k = 0; k < n; k++) for (int q = 0; q < 4; q++) td[(size_t)4 * k + q] = out[(size_t)(MIG_TEN + 4 * t + q) * n + k];
  for (int k = 0; k < n; k++) {
    long long b;
    if (f->id) { memcpy(&b, &out[(size_t)MIG_ID * n + k], 8); f->id[k] = b; }
    if (f->status) { memcpy(&b, &out[(size_t)MIG_STATUS * n + k], 8); f->status[k] = (int32_t)b; }
    if (f->ghost_id) { memcpy(&b, &out[(size_t)SP_GHOST_ID * n + k], 8); f->ghost_id[k] = b; }
  }
  const double* ring = out.data() + (size_t)SP_PACK_NCOL * n;
  for (size_t k = 0; k < V; k++) { if (f->vx) f->vx[k] = ring[2 * k]; if (f->vy) f->vy[k] = ring[2 * k + 1]; }
  const double *sx = ring + 2 * V, *sy = sx + NS, *ir = sy + NS;
  if (f->sx && NS) memcpy(f->sx, sx, NS * sizeof(double));
  if (f->sy && NS) memcpy(f->sy, sy, NS * sizeof(double));
  if (f->ghost_idx && G) memcpy(f->ghost_idx, ir + 7 * R, G * sizeof(int32_t));
  if (inter_rows && R) {
    memcpy(inter_rows, ir, 7 * R * sizeof(double));
    std::vector<long long> sorted;
    if ((rc = sp_ghost_keys(c, sorted))) return rc;
    if (!sorted.empty()) {            // partners that were inline ghosts: order key -> the reference's floe number (sz_download_interactions)
      const double lim = (double)((long long)1 << 40);
      for (size_t r = 0; r < R; r++) {
        const double idx = inter_rows[r * 7];
        if (idx <= lim) continue;
        const long long key = (long long)idx - 1;
        const auto it = std::lower_bound(sorted.begin(), sorted.end(), key);
        if (it == sorted.end() || *it != key) { c->err = "interaction row names a ghost that is not among the last step's"; return SZ_E_STATE; }
        inter_rows[r * 7] = (double)(c->hostN + (int)(it - sorted.begin()) + 1);
      }
    }
  }
  return SZ_OK;
}
}  // namespace

int sz_download_rows(sz_ctx* c, int32_t n, const int32_t* rows, sz_floe_columns* f, int32_t* inter_off, double* inter_rows, int64_t* sizes3) {
  return sp_download(c, "sz_download_rows", false, n, rows, f, inter_off, inter_rows, sizes3);
}
int sz_download_list_rows(sz_ctx* c, int32_t n, const int32_t* rows, sz_floe_columns* f, int32_t* inter_off, double* inter_rows, int64_t* sizes3) {
  return sp_download(c, "sz_download_list_rows", true, n, rows, f, inter_off, inter_rows, sizes3);
}

namespace {
// The uploaded floes of a row edit, checked before anything changes: closed rings the row-moving kernels carry, offsets that ascend, interaction rows
// that fit the stride; *stream_len: the doubles of their migration records.  bits == null: the first fault is returned.  A tiled context's share
// (sz_tile_splice_floes) gives `bits`: what depends on this rank's context alone -- SPT_BIT_ROWCAP, SPT_BIT_POINTS -- is then noted there for the
// ranks' agreement and the walk goes on; what the arguments alone decide is returned as ever, the same on every rank.
constexpr int SPT_BIT_ERR = 1, SPT_BIT_GHOSTS = 2, SPT_BIT_ORDER = 4, SPT_BIT_ROWCAP = 8, SPT_BIT_POINTS = 16, SPT_BIT_NONE = 32, SPT_BIT_MEM = 64;
int sp_check_staged(sz_ctx* c, const std::string& who, int ns, const sz_floe_columns* f, const int32_t* ioff, const double* irows, bool* with_sub_out, size_t* stream_len_out,
                    int* bits = nullptr) {
  const State& S = c->S;
  const bool with_sub = ns > 0 && f->sub_off != nullptr;
  if (with_sub && (!f->sx || !f->sy) && f->sub_off[ns] != f->sub_off[0]) { c->err = who + ": sub_off without sx / sy"; return SZ_E_ARG; }
  size_t stream_len = 0;
  for (int j = 0; j < ns; j++) {
    const int o = f->vert_off[j], nv = f->vert_off[j + 1] - o, sp = with_sub ? f->sub_off[j + 1] - f->sub_off[j] : 0, ni = ioff ? ioff[j + 1] - ioff[j] : 0;
    if (nv < 4 || o < 0 || !(f->vx[o] == f->vx[o + nv - 1] && f->vy[o] == f->vy[o + nv - 1])) { c->err = who + ": uploaded row " + std::to_string(j) + " has an open ring (a ring is closed: its first point repeated, at least 4 points)"; return SZ_E_ARG; }
    if (nv > SP_MAX_RING) { c->err = who + ": uploaded row " + std::to_string(j) + " has a ring of " + std::to_string(nv) + " points: the row-moving kernels carry " + std::to_string(SP_MAX_RING); return SZ_E_ARG; }
    if (sp < 0 || ni < 0) { c->err = who + ": offsets of uploaded row " + std::to_string(j) + " descend"; return SZ_E_ARG; }
    if (sp > 0 && c->pts_N == 0) { if (bits) *bits |= SPT_BIT_POINTS; else { c->err = who + ": the list was uploaded without sub-floe points"; return SZ_E_ARG; } }
    if (ni > S.rowcap) { if (bits) *bits |= SPT_BIT_ROWCAP; else { c->err = "more interaction rows per floe than the fixed stride holds"; return SZ_E_CAPACITY; } }
    if (ni > 0 && !irows) { c->err = who + ": inter_off without inter_rows"; return SZ_E_ARG; }
    stream_len += (size_t)MIG_NCOL + 2 * (size_t)nv + 2 * (size_t)sp;
  }
  if (stream_len > 0x7fffffffull) { c->err = who + ": the uploaded rows are too long for one stream"; return SZ_E_ARG; }
  *with_sub_out = with_sub; *stream_len_out = stream_len;
  return SZ_OK;
}

// What a tiled context's share of a global edit gives the body of a splice: how sz_k_spt_renumber numbers the new rows, the new global number of
// every staged floe (a floe uploaded without an id gets it + 1), and where the new numbers of all new rows go on the host.
struct SpTile { SptKeys keys; const long long* staged_num; std::vector<long long>* newkey; };

int sp_splice_rows(sz_ctx* c, const std::string& who, bool parents, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns* f,
                   const int32_t* ioff, const double* irows, bool with_sub, size_t stream_len, const SpTile* tile);

// sz_splice_floes (parents = false: a ghost-free list with nothing pending) and sz_splice_parents (parents = true: the ghosts of the list are dropped
// first, as sz_remove_ghosts drops them, and a pending mark stays) -- every check comes before the first change
int sp_splice(sz_ctx* c, const char* who_, bool parents, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns* f,
              const int32_t* ioff, const double* irows) {
  const std::string who(who_);
  if (!c || n_del < 0 || n_rep < 0 || n_app < 0 || (n_del && !del) || (n_rep && !rep)) return SZ_E_ARG;
  const long long ns64 = (long long)n_rep + n_app;
  if (ns64 > 0x3fffffff) return SZ_E_ARG;
  const int ns = (int)ns64;
  if (ns > 0 && (!f || !f->vert_off || !f->vx || !f->vy || !f->cx || !f->cy)) { c->err = who + ": replaced / appended rows need vert_off, vx, vy, cx and cy"; return SZ_E_ARG; }
  if (!c->have_floes) { c->err = who + ": no floes uploaded"; return SZ_E_STATE; }
  if (c->S.tiled) { c->err = who + ": the rows of a tiled context carry global numbers and its list is one rank's share: not supported on tiled contexts (sz_tile_splice_floes edits them by global number)"; return SZ_E_STATE; }
  if (!parents && c->rr_pending >= 0) { c->err = who + ": a ridge / raft step is pending with its ghosts in the list (sz_step_finish first)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = sync_and_check(c))) return rc;          // hostM / hostN current, nothing pending
  if (!parents && c->hostM != c->hostN) { c->err = who + ": ghosts are in the list (sz_remove_ghosts first): the edit is of the parents alone"; return SZ_E_STATE; }
  const int N = c->hostN;
  // ---- the edit itself: rows, then the uploaded floes
  if ((rc = sp_check_rows(c, who_, "del", n_del, del, N, true)) || (rc = sp_check_rows(c, who_, "rep", n_rep, rep, N, true))) return rc;
  for (int a = 0, b = 0; a < n_del && b < n_rep;) {
    if (del[a] == rep[b]) { c->err = who + ": row " + std::to_string(del[a]) + " is both deleted and replaced"; return SZ_E_ARG; }
    if (del[a] < rep[b]) a++; else b++;
  }
  const long long Nn64 = (long long)N - n_del + n_app;
  if (Nn64 <= 0) { c->err = who + ": the edit leaves no floe"; return SZ_E_ARG; }
  if (Nn64 > 0x3fffffff) { c->err = who + ": too many floes"; return SZ_E_ARG; }
  bool with_sub = false; size_t stream_len = 0;
  if ((rc = sp_check_staged(c, who, ns, f, ioff, irows, &with_sub, &stream_len))) return rc;
  if (n_del + ns == 0) return SZ_OK;          // nothing to do, nothing touched
  return sp_splice_rows(c, who, parents, n_del, del, n_rep, rep, n_app, f, ioff, irows, with_sub, stream_len, nullptr);
}

// The body of a splice, behind the checks: rows del / rep of this context's list, the ns = n_rep + n_app uploaded floes.  tile: this context's share of
// a global edit (sz_tile_splice_floes, which has agreed it with the other ranks and establishes the tiling again behind it) -- the new rows then take
// the global numbers of sz_k_spt_renumber as order keys and origin instead of the identity.
int sp_splice_rows(sz_ctx* c, const std::string& who, bool parents, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns* f,
                   const int32_t* ioff, const double* irows, bool with_sub, size_t stream_len, const SpTile* tile) {
  int rc;
  State& S = c->S;
  const int N = c->hostN, ns = n_rep + n_app, Nn = N - n_del + n_app;
  // ---- from here on the state changes
  const int Mold = c->hostM;          // (the rows the list's ghosts held are vacated too)
  if (parents && (Mold != N || c->ghosts_staged)) { if ((rc = sz_remove_ghosts(c))) return rc; }
  leave_resident(c);
  std::vector<long long> keys;
  if ((rc = sp_ghost_keys(c, keys))) return rc;
  c->gi_pending = false;
  Pool& P = c->sp_allocs;
  reset_pool(P);
  // ---- the uploaded rows as one stream of migration records with its directory (sz_migrate.hpp), their CSR offsets, the marks
  std::vector<double> stream(std::max<size_t>(stream_len, 1)), dirs((size_t)MIG_DIR * (1 + (size_t)ns), 0.0);
  std::vector<int> ints(3 * ((size_t)ns + 1) + (size_t)n_del + n_rep + 1, 0);
  int *h_svoff = ints.data(), *h_ssoff = h_svoff + ns + 1, *h_sioff = h_ssoff + ns + 1, *h_del = h_sioff + ns + 1, *h_rep = h_del + n_del;
  double staged_rmax = 0.0;
  {
    static const sz_floe_columns none{};
    const ColTable<const double*> src = host_columns(f ? *f : none);
    dirs[0] = (double)ns;
    size_t at = 0; int dbelow = 0;
    for (int j = 0; j < ns; j++) {
      const int o = f->vert_off[j], nv = f->vert_off[j + 1] - o, so = with_sub ? f->sub_off[j] : 0, sp = with_sub ? f->sub_off[j + 1] - so : 0;
      // the row this floe takes in the edited list (the id an upload gives a floe without one is its row + 1)
      int newrow;
      if (j < n_rep) { while (dbelow < n_del && del[dbelow] < rep[j]) dbelow++; newrow = rep[j] - dbelow; }
      else newrow = N - n_del + (j - n_rep);
      double* rec = &stream[at];
      for (int q = 0; q < MIG_NSC; q++) rec[q] = src.p[q] ? src.p[q][j] : 0.0;
      for (int t = 0; t < MIG_NTEN; t++) for (int q = 0; q < 4; q++) rec[MIG_TEN + 4 * t + q] = src.p[MIG_NSC + t] ? src.p[MIG_NSC + t][(size_t)4 * j + q] : 0.0;
      rec[MIG_ID] = (double)(f->id ? f->id[j] : (tile ? tile->staged_num[j] : (long long)newrow) + 1); rec[MIG_STATUS] = (double)(f->status ? f->status[j] : SZ_ACTIVE); rec[MIG_GIDX] = 0.0;
      rec[MIG_NV] = (double)nv; rec[MIG_NS] = (double)sp;
      for (int k = 0; k < nv; k++) { rec[MIG_NCOL + 2 * k] = f->vx[o + k]; rec[MIG_NCOL + 2 * k + 1] = f->vy[o + k]; }
      double* sub = rec + MIG_NCOL + 2 * (size_t)nv;
      for (int k = 0; k < sp; k++) { sub[k] = f->sx[so + k]; sub[sp + k] = f->sy[so + k]; }
      double* e = &dirs[(size_t)MIG_DIR * (1 + (size_t)j)];
      e[0] = 0.0; e[1] = (double)nv; e[2] = (double)sp; e[3] = (double)at; e[4] = rec[COL_rmax]; e[5] = rec[COL_cx]; e[6] = rec[COL_cy];
      staged_rmax = std::max(staged_rmax, rec[COL_rmax]);
      h_svoff[j + 1] = h_svoff[j] + nv; h_ssoff[j + 1] = h_ssoff[j] + sp; h_sioff[j + 1] = h_sioff[j] + (ioff ? ioff[j + 1] - ioff[j] : 0);
      at += (size_t)MIG_NCOL + 2 * (size_t)nv + 2 * (size_t)sp;
    }
    for (int k = 0; k < n_del; k++) h_del[k] = del[k];
    for (int k = 0; k < n_rep; k++) h_rep[k] = rep[k];
  }
  const int n_irows = h_sioff[ns];
  double *d_stream = nullptr, *d_dirs = nullptr, *d_irows = nullptr; int* d_ints = nullptr; long long* d_keys = nullptr;
  SpArgs A{};
  const size_t o1 = (size_t)N + 2, r1 = (size_t)Nn + 2;
  if ((rc = dalloc(c, &d_stream, stream.size(), P)) || (rc = dalloc(c, &d_dirs, dirs.size(), P)) || (rc = dalloc(c, &d_ints, ints.size(), P)) ||
      (rc = dalloc(c, &d_irows, (size_t)std::max(n_irows, 1) * 7, P)) || (rc = dalloc(c, &d_keys, std::max<size_t>(keys.size(), 1), P)) ||
      (rc = dalloc(c, &A.d, 1, P)) || (rc = dalloc(c, &A.mark, o1, P)) || (rc = dalloc(c, &A.keep, o1, P)) || (rc = dalloc(c, &A.kv, o1, P)) || (rc = dalloc(c, &A.ks, o1, P)) ||
      (rc = dalloc(c, &A.newrow, o1, P)) || (rc = dalloc(c, &A.ovoff, o1, P)) || (rc = dalloc(c, &A.osoff, o1, P)) ||
      (rc = dalloc(c, &A.src, r1, P)) || (rc = dalloc(c, &A.nvoff, r1, P)) || (rc = dalloc(c, &A.nsoff, r1, P))) return rc;
  H2D(d_stream, stream.data(), stream.size(), double); H2D(d_dirs, dirs.data(), dirs.size(), double); H2D(d_ints, ints.data(), ints.size(), int);
  if (n_irows) H2D(d_irows, irows + (size_t)ioff[0] * 7, (size_t)n_irows * 7, double);
  if (!keys.empty()) H2D(d_keys, keys.data(), keys.size(), long long);
  A.n = N; A.n_del = n_del; A.n_rep = n_rep; A.n_app = n_app;
  A.svoff = d_ints; A.ssoff = d_ints + ns + 1; A.del = d_ints + 3 * ((size_t)ns + 1); A.rep = A.del + n_del;
  const int* d_sioff = d_ints + 2 * ((size_t)ns + 1);
  // ---- the plan: marks, flags, removal's scans over old-or-staged lengths, the new rows' sources and offsets, what an upload would find of them
  HIPCHK(c, hipMemsetAsync(A.mark, 0, o1 * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(A.d, 0, sizeof(SpDev), c->stream));
  const int nb = grid_for(std::max(N, n_app), 256, 2048);
  if (n_del + n_rep) hipLaunchKernelGGL(sz_k_sp_marks, dim3(grid_for(n_del + n_rep, 256, 2048)), dim3(256), 0, c->stream, A);
  hipLaunchKernelGGL(sz_k_sp_flags, dim3(nb), dim3(256), 0, c->stream, S, A);
  scan(c, A.keep, A.newrow, N, C_N, 0, -1);
  scan(c, A.kv, A.ovoff, N, C_N, 0, -1);
  scan(c, A.ks, A.osoff, N, C_N, 0, -1);
  hipLaunchKernelGGL(sz_k_sp_rows, dim3(nb), dim3(256), 0, c->stream, A);
  long long* d_newkey = nullptr;
  if (tile) {
    if ((rc = dalloc(c, &d_newkey, (size_t)Nn + 1, P))) return rc;
    hipLaunchKernelGGL(sz_k_spt_renumber, dim3(grid_for(Nn, 256, 2048)), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, tile->keys, d_newkey);
    tile->newkey->assign((size_t)Nn, 0);
    HIPCHK(c, hipMemcpyAsync(tile->newkey->data(), d_newkey, (size_t)Nn * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  }
  hipLaunchKernelGGL(sz_k_sp_limits, dim3(grid_for(Nn, 256, 2048)), dim3(256), 0, c->stream, S, A, Nn, (const double*)d_dirs, (const double*)d_stream);
  SpDev R{};
  HIPCHK(c, hipMemcpyAsync(&R, A.d, sizeof(SpDev), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (R.Nn != Nn || R.Vn < 0 || R.NSn < 0) { c->err = who + ": bad counts"; return SZ_E_HIP; }
  const int Vn = R.Vn, NSn = R.NSn, tcap = S.rowcap;
  // ---- the rows of the edited list, gathered beside the old ones: kept rows from the list, the others from the stream
  double** d_cols = nullptr; double *d_tmp = nullptr, *d_tsx = nullptr, *d_tsy = nullptr, *d_trows = nullptr; double2* d_tv = nullptr; int* d_tcnt = nullptr;
  if ((rc = dalloc(c, &d_cols, MIG_TAB_CAP, P)) || (rc = dalloc(c, &d_tmp, (size_t)SP_NCOL * Nn, P)) || (rc = dalloc(c, &d_tv, (size_t)Vn, P)) || (rc = dalloc(c, &d_tsx, (size_t)NSn, P)) ||
      (rc = dalloc(c, &d_tsy, (size_t)NSn, P)) || (rc = dalloc(c, &d_tcnt, (size_t)Nn, P)) || (rc = dalloc(c, &d_trows, (size_t)Nn * tcap * 7, P))) return rc;
  ColTable<double*> hcols = state_columns(S);
  HIPCHK(c, hipMemcpyAsync(d_cols, hcols.p, sizeof(hcols.p), hipMemcpyHostToDevice, c->stream));
  const int nbw = grid_for((long long)Nn * 64, 256, 4096);
  hipLaunchKernelGGL(sz_k_mig_gather, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, (const double*)d_dirs, (const double*)d_stream,
                     (double* const*)d_cols, d_tmp);
  hipLaunchKernelGGL(sz_k_mig_points, dim3(nbw), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, (const double*)d_dirs, (const double*)d_stream,
                     (const int*)A.nvoff, (const int*)A.nsoff, d_tv, d_tsx, d_tsy);
  hipLaunchKernelGGL(sz_k_sp_gather_rows, dim3(nbw), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, d_sioff, (const double*)d_irows, (const long long*)d_keys,
                     (int)keys.size(), N, tcap, d_tcnt, d_trows);
  // does the edited list fit what the context was carved for?  The rule of a migration's receive path: an eighth more than the upload held is let in.
  const bool fits = Nn <= c->upload_M + c->upload_M / 8 && Vn <= c->upload_V + c->upload_V / 8 && Nn <= S.capM && Vn <= S.capV;
  const int pts = c->pts_N ? Nn : 0;
  int gl_est = std::min(Nn, c->gl_est + ns); double rmax_max = std::max(c->rmax_max, staged_rmax), rmax_hint = c->rmax_hint;
  Pool old_sub;
  if (!fits) {
    // ---- the pools grow: the context is carved anew for the edited list by the upload itself -- given the small host columns its sizing reads (centroids,
    // rmax, ids, statuses, offsets: fetched from the gathered rows) and rings / points of zeros --, then the gathered rows are placed as below
    std::vector<double> h3((size_t)3 * Nn), hid((size_t)2 * Nn), zv((size_t)std::max(Vn, 1), 0.0), zs((size_t)std::max(NSn, 1), 0.0);
    std::vector<int> hvoff((size_t)Nn + 1), hsoff((size_t)Nn + 1), hst((size_t)Nn); std::vector<long long> hidl((size_t)Nn);
    static_assert(COL_cx == 0 && COL_cy == 1 && COL_rmax == 2 && MIG_STATUS == MIG_ID + 1, "fetched as two runs of the gathered columns: cx, cy, rmax and id, status");
    HIPCHK(c, hipMemcpyAsync(h3.data(), d_tmp, h3.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hid.data(), d_tmp + (size_t)MIG_ID * Nn, hid.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hvoff.data(), A.nvoff, hvoff.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hsoff.data(), A.nsoff, hsoff.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < Nn; r++) { hidl[r] = (long long)hid[r]; hst[r] = (int)hid[(size_t)Nn + r]; }
    sz_floe_columns d; memset(&d, 0, sizeof(d));
    d.cx = h3.data(); d.cy = h3.data() + Nn; d.rmax = h3.data() + (size_t)2 * Nn; d.id = (int64_t*)hidl.data(); d.status = hst.data();
    d.vert_off = hvoff.data(); d.vx = zv.data(); d.vy = zv.data();
    if (c->pts_N) { d.sub_off = hsoff.data(); d.sx = zs.data(); d.sy = zs.data(); }
    if ((rc = sz_upload_floes(c, Nn, Nn, &d))) return rc;
    if (S.rowcap < tcap) { S.rowcap = tcap; if ((rc = carve_interactions(c))) return rc; }      // (a kept floe may hold more rows than a fresh stride)
    hcols = state_columns(S);
    HIPCHK(c, hipMemcpyAsync(d_cols, hcols.p, sizeof(hcols.p), hipMemcpyHostToDevice, c->stream));
    gl_est = c->gl_est; rmax_max = c->rmax_max; rmax_hint = 0.0;          // (the upload's own, of the edited list)
  } else if (NSn > S.capS) {          // the sub-floe points have no slack at upload: a new pair, as for a tile that gained points in a migration
    old_sub = c->sub_allocs; c->sub_allocs = Pool();
    S.capS = NSn + NSn / 4;
    if ((rc = dalloc(c, &S.sx, (size_t)S.capS, c->sub_allocs)) || (rc = dalloc(c, &S.sy, (size_t)S.capS, c->sub_allocs))) return rc;
  }
  // ---- and into their places, with the links of a freshly placed ghost-free field (as sz_upload_floes leaves them)
  hipLaunchKernelGGL(sz_k_mig_scatter, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (double* const*)d_cols, (const double*)d_tmp);
  hipLaunchKernelGGL(sz_k_sp_scatter_rows, dim3(nbw), dim3(256), 0, c->stream, S, Nn, c->origin, (const long long*)d_newkey, tcap, (const int*)d_tcnt, (const double*)d_trows);
  const int top = std::min(std::max(N, Mold), S.capM);
  if (fits && top > Nn) hipLaunchKernelGGL(sz_k_sp_clear_rows, dim3(grid_for(top - Nn, 256, 2048)), dim3(256), 0, c->stream, Nn, top, (double* const*)d_cols);
  if (top > Nn) HIPCHK(c, hipMemsetAsync(S.inter_cnt + Nn, 0, (size_t)(top - Nn) * sizeof(int), c->stream));
  if (Vn) HIPCHK(c, hipMemcpyAsync(S.vxy, d_tv, (size_t)Vn * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(S.voff, A.nvoff, ((size_t)Nn + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  if (c->pts_N) {
    if (NSn) {
      HIPCHK(c, hipMemcpyAsync(S.sx, d_tsx, (size_t)NSn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(c, hipMemcpyAsync(S.sy, d_tsy, (size_t)NSn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(S.soff, A.nsoff, ((size_t)Nn + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  }
  // ---- the field is placed: everything derived as behind the copies of sz_upload_floes; the rows as behind sz_upload_interactions
  if ((rc = field_placed(c, Nn, 0, Vn, pts, gl_est, rmax_max, rmax_hint))) return rc;
  free_pool(old_sub);
  c->inter_any = true; c->inter_lost = false; c->rr_rows = true;
  c->maybe_tagged = R.n_tagged > 0; c->grid_live = false;
  c->max_ring = R.max_ring; if (c->pts_N) c->max_sub = R.max_sub;          // (as an upload of the edited list finds them)
  return SZ_OK;
}
}  // namespace

int sz_splice_floes(sz_ctx* c, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns* f,
                    const int32_t* ioff, const double* irows) {
  return sp_splice(c, "sz_splice_floes", false, n_del, del, n_rep, rep, n_app, f, ioff, irows);
}
int sz_splice_parents(sz_ctx* c, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns* f,
                      const int32_t* ioff, const double* irows) {
  return sp_splice(c, "sz_splice_parents", true, n_del, del, n_rep, rep, n_app, f, ioff, irows);
}

// ... for Float32 hosts: widened on the way in, rounded on the way out, exactly as sz_upload_floes_f32 / sz_download_floes_f32 do
namespace {
using sp_download_fn = int (*)(sz_ctx*, int32_t, const int32_t*, sz_floe_columns*, int32_t*, double*, int64_t*);
using sp_splice_fn = int (*)(sz_ctx*, int32_t, const int32_t*, int32_t, const int32_t*, int32_t, const sz_floe_columns*, const int32_t*, const double*);
// Float64 room for the n rows a download brings (sz: the sizes its sizing call gave -- ring points, sub-floe points, interaction rows)
struct SpF32Down : F32Down {
  SpF32Down(size_t n, const int64_t* sz, sz_floe_columns_f32* f, float* inter_rows) : F32Down(f, n, (size_t)sz[0], (size_t)sz[1], F32_STAGE_SUB, inter_rows, 7 * (size_t)sz[2]) {}
};
// the M = n_rep + n_app uploaded floes of a splice, widened
struct SpF32Up : F32Up {
  SpF32Up(size_t M, const sz_floe_columns_f32* f, const int32_t* ioff, const float* irows) : F32Up(f, M, (size_t)f->vert_off[M], f->sub_off ? (size_t)f->sub_off[M] : 0, irows, ioff ? 7 * (size_t)ioff[M] : 0) {}
};
int sp_download_f32(sp_download_fn down, sz_ctx* c, int32_t n, const int32_t* rows, sz_floe_columns_f32* f, int32_t* inter_off, float* inter_rows, int64_t* sizes3) {
  if (!c || n < 0) return SZ_E_ARG;
  int64_t sz[3] = { 0, 0, 0 };
  int rc = down(c, n, rows, nullptr, nullptr, nullptr, sz); if (rc) return rc;
  if (sizes3) { sizes3[0] = sz[0]; sizes3[1] = sz[1]; sizes3[2] = sz[2]; }
  if (!f) return SZ_OK;
  SpF32Down W((size_t)n, sz, f, inter_rows);
  rc = down(c, n, rows, &W.d, inter_off, W.ir, nullptr); if (rc) return rc;
  W.back();
  return SZ_OK;
}
int sp_splice_f32(sp_splice_fn splice, const char* who, sz_ctx* c, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app,
                  const sz_floe_columns_f32* f, const int32_t* ioff, const float* irows) {
  if (!c || n_rep < 0 || n_app < 0) return SZ_E_ARG;
  const size_t M = (size_t)n_rep + (size_t)n_app;
  if (M == 0 || !f) return splice(c, n_del, del, n_rep, rep, n_app, nullptr, ioff, nullptr);
  if (!f->vert_off) { c->err = std::string(who) + ": vert_off is required"; return SZ_E_ARG; }
  const SpF32Up W(M, f, ioff, irows);
  return splice(c, n_del, del, n_rep, rep, n_app, &W.d, ioff, W.ir);
}
}  // namespace
int sz_download_rows_f32(sz_ctx* c, int32_t n, const int32_t* rows, sz_floe_columns_f32* f, int32_t* inter_off, float* inter_rows, int64_t* sizes3) {
  return sp_download_f32(sz_download_rows, c, n, rows, f, inter_off, inter_rows, sizes3);
}
int sz_download_list_rows_f32(sz_ctx* c, int32_t n, const int32_t* rows, sz_floe_columns_f32* f, int32_t* inter_off, float* inter_rows, int64_t* sizes3) {
  return sp_download_f32(sz_download_list_rows, c, n, rows, f, inter_off, inter_rows, sizes3);
}
int sz_splice_floes_f32(sz_ctx* c, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns_f32* f,
                        const int32_t* ioff, const float* irows) {
  return sp_splice_f32(sz_splice_floes, "sz_splice_floes_f32", c, n_del, del, n_rep, rep, n_app, f, ioff, irows);
}
int sz_splice_parents_f32(sz_ctx* c, int32_t n_del, const int32_t* del, int32_t n_rep, const int32_t* rep, int32_t n_app, const sz_floe_columns_f32* f,
                          const int32_t* ioff, const float* irows) {
  return sp_splice_f32(sz_splice_parents, "sz_splice_parents_f32", c, n_del, del, n_rep, rep, n_app, f, ioff, irows);
}

// ---------------------------------------------------------------- ridge / raft candidates (sz_ridgeraft.hpp)
int sz_set_ridgeraft(sz_ctx* c, int32_t on, int32_t dt, double min_ridge_height, double max_floe_ridge_height, double max_domain_ridge_height,
                     double max_floe_raft_height, double max_domain_raft_height) {
  if (!c) return SZ_E_ARG;
  if (!on) { c->rr_on = false; return SZ_OK; }
  if (dt <= 0) { c->err = "sz_set_ridgeraft: dt (RidgeRaftSettings.Δt) must be positive"; return SZ_E_ARG; }
  const double h[5] = { min_ridge_height, max_floe_ridge_height, max_domain_ridge_height, max_floe_raft_height, max_domain_raft_height };
  for (double v : h) if (v != v) { c->err = "sz_set_ridgeraft: a height is NaN"; return SZ_E_ARG; }
  c->rr_on = true; c->rr_dt = dt;
  for (int k = 0; k < 5; k++) c->rr_h[k] = h[k];
  return SZ_OK;
}

namespace {
int rr_ensure(sz_ctx* c, int M, int need) {
  if (c->rr.d && M <= c->rr_capM && need <= c->rr_cap) return SZ_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_pool(c->rr_allocs);
  c->rr = RrArgs{}; c->rr_capM = c->rr_cap = 0;
  const size_t capM = (size_t)std::max(M, c->S.capM), cap = (size_t)std::max(need, RR_CAP0);
  Pool& P = c->rr_allocs; RrArgs& A = c->rr; int rc;
  if ((rc = dalloc(c, &A.d, 1, P)) || (rc = dalloc(c, &A.cnt, capM + 1, P)) || (rc = dalloc(c, &A.off, capM + 1, P)) ||
      (rc = dalloc(c, &A.ti, cap, P)) || (rc = dalloc(c, &A.tj, cap, P)) || (rc = dalloc(c, &A.tk, cap, P)) || (rc = dalloc(c, &A.tf, cap, P))) return rc;
  c->rr_capM = (int)capM; c->rr_cap = (int)cap;
  return SZ_OK;
}
// what the pass may be asked on: the list as add_ghosts! leaves it, with the rows of a collision call (or hand-made ones) on that list
int rr_state_checks(sz_ctx* c, const char* who) {
  if (!c->have_floes) { c->err = std::string(who) + ": no floes uploaded"; return SZ_E_STATE; }
  if (c->S.tiled) { c->err = std::string(who) + ": a tiled list is one rank's share of the table: sz_tile_ridgeraft_candidates (collective, at a pending stop of sz_tile_run)"; return SZ_E_STATE; }
  if (!c->ghosts_staged || !c->rr_rows || !c->inter_any || c->inter_lost || c->gi_valid) {
    c->err = std::string(who) + ": needs the list with its ghosts and this step's interaction rows (sz_add_ghosts + sz_timestep_collisions, or a pending ridge / raft stop)";
    return SZ_E_STATE;
  }
  return SZ_OK;
}
// The candidate table of the list as it lies (hostM rows, current): *nt entries in c->rr.ti / tj / tk / tf, *draws per-floe draws.  One host
// synchronisation (two when the table outgrew its arrays); reads the floes' columns and rows only.
int rr_pass(sz_ctx* c, const double* h5, int* nt, long long* draws) {
  *nt = 0; *draws = 0;
  const int M = c->hostM;
  if (M <= 0) return SZ_OK;
  int need = c->rr_cap;
  for (int round = 0;; round++) {
    if (int rc = rr_ensure(c, M, need)) return rc;
    RrArgs A = c->rr;
    A.m = M; A.cap = c->rr_cap;
    A.min_ridge_h = h5[0]; A.max_floe_ridge_h = h5[1]; A.max_domain_ridge_h = h5[2]; A.max_floe_raft_h = h5[3]; A.max_domain_raft_h = h5[4];
    HIPCHK(c, hipMemsetAsync(A.d, 0, sizeof(RrDev), c->stream));
    const int nb = grid_for(M, 256, 2048);
    hipLaunchKernelGGL(sz_k_rr_count, dim3(nb), dim3(256), 0, c->stream, c->S, A);
    hipLaunchKernelGGL(sz_k_rr_scan, dim3(1), dim3(RR_TPB), 0, c->stream, A);
    hipLaunchKernelGGL(sz_k_rr_write, dim3(nb), dim3(256), 0, c->stream, c->S, A);
    HIPCHK(c, hipMemcpyAsync(&c->rr_hd, A.d, sizeof(RrDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int T = c->rr_hd.total;
    if (T < 0 || (long long)T > (long long)M * c->S.rowcap) { c->err = "ridge / raft candidates: bad table count"; return SZ_E_HIP; }
    if (T > c->rr_cap) {          // more than the arrays hold: larger arrays, the pass again -- nothing is truncated
      if (round > 0) { c->err = "ridge / raft candidates: the table did not grow enough"; return SZ_E_CAPACITY; }
      need = std::max(T, 2 * c->rr_cap);
      continue;
    }
    *nt = T; *draws = (long long)c->rr_hd.draws;
    return SZ_OK;
  }
}
// the second half of a timestep whose first half (add_ghosts!, timestep_collisions!) has run: sz_remove_ghosts; sz_timestep_coupling when due;
// sz_timestep_floe_properties
int rr_second_half(sz_ctx* c, int tstep, int dt, int coupling_dt, int flags) {
  if (int rc = sz_remove_ghosts(c)) return rc;
  if (coupling_at(flags, coupling_dt, tstep)) { if (int rc = sz_timestep_coupling(c)) return rc; }
  return sz_timestep_floe_properties(c, dt);
}
}  // namespace

int sz_ridgeraft_candidates(sz_ctx* c, int32_t* n, int32_t cap, int32_t* idx_i, int32_t* idx_j, int32_t* kind, double* frac, int64_t* n_draws) {
  if (n) *n = 0;
  if (n_draws) *n_draws = 0;
  if (!c || !n) return SZ_E_ARG;
  if (!c->rr_on) { c->err = "sz_ridgeraft_candidates: ridge / raft is not set (sz_set_ridgeraft)"; return SZ_E_STATE; }
  if (int rc = rr_state_checks(c, "sz_ridgeraft_candidates")) return rc;
  (void)hipSetDevice(c->device);
  if (int rc = sync_and_check(c)) return rc;          // hostM current
  int nt = 0; long long nd = 0;
  if (int rc = rr_pass(c, c->rr_h, &nt, &nd)) return rc;
  *n = nt;
  if (n_draws) *n_draws = nd;
  if (!idx_i && !idx_j && !kind && !frac) return SZ_OK;
  if (cap < nt) { c->err = "sz_ridgeraft_candidates: cap is smaller than the table (*n)"; return SZ_E_ARG; }
  if (nt > 0) {
    if (idx_i) HIPCHK(c, hipMemcpyAsync(idx_i, c->rr.ti, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (idx_j) HIPCHK(c, hipMemcpyAsync(idx_j, c->rr.tj, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (kind) HIPCHK(c, hipMemcpyAsync(kind, c->rr.tk, (size_t)nt * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (frac) HIPCHK(c, hipMemcpyAsync(frac, c->rr.tf, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return SZ_OK;
}
// The closure of the table (sz_ridgeraft.hpp): the rows of its entries, their root parents and those parents' ghosts, ascending, each once.
int sz_ridgeraft_rows(sz_ctx* c, int32_t* n, int32_t cap, int32_t* rows) {
  if (n) *n = 0;
  if (!c || !n) return SZ_E_ARG;
  if (!c->rr_on) { c->err = "sz_ridgeraft_rows: ridge / raft is not set (sz_set_ridgeraft)"; return SZ_E_STATE; }
  if (int rc = rr_state_checks(c, "sz_ridgeraft_rows")) return rc;
  (void)hipSetDevice(c->device);
  if (int rc = sync_and_check(c)) return rc;          // hostM / hostN current
  int nt = 0; long long nd = 0;
  if (int rc = rr_pass(c, c->rr_h, &nt, &nd)) return rc;
  if (nt == 0) return SZ_OK;
  const int M = c->hostM, N = c->hostN;
  Pool& P = c->sp_allocs;
  reset_pool(P);
  int *flag = nullptr, *off = nullptr, *out = nullptr, rc;
  if ((rc = dalloc(c, &flag, (size_t)M + 1, P)) || (rc = dalloc(c, &off, (size_t)M + 2, P)) || (rc = dalloc(c, &out, (size_t)M + 1, P))) return rc;
  HIPCHK(c, hipMemsetAsync(flag, 0, ((size_t)M + 1) * sizeof(int), c->stream));
  hipLaunchKernelGGL(sz_k_rr_mark, dim3(grid_for(nt, 256, 2048)), dim3(256), 0, c->stream, c->S, (const int*)c->rr.ti, (const int*)c->rr.tj, nt, M, N, flag);
  scan(c, flag, off, M, -1, M, -1);
  hipLaunchKernelGGL(sz_k_rr_compact, dim3(grid_for(M, 256, 2048)), dim3(256), 0, c->stream, (const int*)flag, (const int*)off, M, out);
  int total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, off + M, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (total < 0 || total > M) { c->err = "sz_ridgeraft_rows: bad row count"; return SZ_E_HIP; }
  *n = total;
  if (!rows) return SZ_OK;
  if (cap < total) { c->err = "sz_ridgeraft_rows: cap is smaller than the closure (*n)"; return SZ_E_ARG; }
  if (total > 0) HIPCHK(c, hipMemcpy(rows, out, (size_t)total * sizeof(int), hipMemcpyDeviceToHost));
  return SZ_OK;
}
// (a Float32 host's name for the same call: no floating-point value crosses it)
int sz_ridgeraft_rows_f32(sz_ctx* c, int32_t* n, int32_t cap, int32_t* rows) { return sz_ridgeraft_rows(c, n, cap, rows); }
int sz_ridgeraft_pending(sz_ctx* c, int32_t* tstep) {
  if (!c || !tstep) return SZ_E_ARG;
  *tstep = c->rr_pending;
  return SZ_OK;
}
int sz_ridgeraft_draws(sz_ctx* c, int64_t* n) {
  if (!c || !n) return SZ_E_ARG;
  *n = c->rr_draws;
  return SZ_OK;
}
int sz_step_finish(sz_ctx* c, int32_t tstep, int32_t dt, int32_t coupling_dt, int32_t flags) {
  if (!c) return SZ_E_ARG;
  if (c->rr_pending < 0) { c->err = "sz_step_finish: no ridge / raft step is pending"; return SZ_E_STATE; }
  if (tstep != c->rr_pending) { c->err = "sz_step_finish: tstep is not the pending timestep (sz_ridgeraft_pending)"; return SZ_E_ARG; }
  if ((flags & SZ_COUPLING_ON) && !c->have_fields) { c->err = "sz_set_fields must be called before coupling"; return SZ_E_STATE; }
  if (int rc = rr_second_half(c, tstep, dt, coupling_dt, flags)) return rc;
  c->rr_pending = -1;
  return SZ_OK;
}

static int rec_record(sz_ctx* c, int tstep, int* full);          // (the recorder: behind the output path, below)
namespace {
// The passes of the stop schedule (sz_stops.hpp) on the single context.  Every value is this process's own: a tag is always settled.
struct SingleStops {
  sz_ctx* c; int dt, coupling_dt, flags; int pipelined = 0;
  // write_data! of an output step (sz_record.hpp): the frames of the list as add_ghosts! leaves it, the ghosts detached again
  int record(int tstep, int* full) { return rec_record(c, tstep, full); }
  // an ordinary batch: its last step keeps its ghosts, the rows come home behind it, segments of pipe_min_steps or more stay pipelined
  int segment(int len, int t0, int* ran, int* tag) {
    const int rc = step_segment(c, len, t0, dt, coupling_dt, flags, ran);
    *tag = !(flags & SZ_NO_STOP) && (*ran < len || c->last_stopped);          // (a batch that runs through is only cut and recorded: no tag is looked at)
    pipelined |= c->last_pipelined;
    return rc;
  }
  // through the process calls, with the candidate pass of sz_ridgeraft.hpp (one host synchronisation) in the middle; pending = the state is the
  // reference's between timestep_collisions! and timestep_ridging_rafting!, and sz_ridgeraft_candidates gives the same table again
  int rr_step(int tstep, bool last, int* pending, int* tag) {
    int rc, nt = 0, nc = 0; long long nd = 0; int64_t todo[4] = { 0, 0, 0, 0 };
    (void)hipSetDevice(c->device);
    if (c->ghosts_staged && (rc = sz_remove_ghosts(c))) return rc;          // (ghosts a process-mode call left attached: a batch drops them too)
    if ((rc = sz_add_ghosts(c)) || (rc = sz_timestep_collisions(c, c->hostN, dt)) || (rc = rr_pass(c, c->rr_h, &nt, &nd))) return rc;
    if (nt > 0) { c->rr_pending = tstep; *pending = 1; return SZ_OK; }
    c->rr_draws += nd;
    if ((rc = rr_second_half(c, tstep, dt, coupling_dt, flags))) return rc;
    // ... which ends as a segment's last step does: a tag, or a fracture candidate on a fracture step, is a stop request
    if (!last && (rc = sz_simplify_check(c, 0x7fffffff, 0.0, 0.0, todo))) return rc;
    c->last_stopped = todo[0] + todo[1] > 0;
    if (!last && !c->last_stopped && is_fracture_step(c->frac_kind != SZ_FRAC_OFF ? c->frac_dt : 0, tstep)) {
      if ((rc = sz_fracture_candidates(c, &nc, nullptr))) return rc;
      c->last_stopped = nc > 0;
    }
    *tag = c->last_stopped;
    return SZ_OK;
  }
  // only asked behind a stop, which is a tag or a candidate: where a tag alone ends the batch -- no removal, a welding step -- nobody asks which
  int fracture(int, int weld_set, int* cand, int*) { *cand = 1; return c->rm_on && weld_set < 0 ? sz_fracture_candidates(c, cand, nullptr) : SZ_OK; }
  // (not empty: sz_weld_overlaps gives the caller the same table again)
  int weld(int set, int* nt, int*) { return weld_pass(c, c->weld_nxs[set], c->weld_nys[set], c->weld_max_area, nt); }
  int settle(int*) { return SZ_OK; }
  // the pass of sz_remove.hpp on the parents alone (the segment's ghosts are detached by then, as at the start of a new batch)
  int remove(int* ok) {
    int nr = 0, nd = 0;
    if (!c->last_stopped || c->hostM != c->hostN) return SZ_OK;
    leave_resident(c);
    const int rc = remove_pass(c, ok, &nr, &nd);
    if (!rc && *ok) c->last_stopped = false;
    return rc;
  }
};
}  // namespace

// nsteps x timestep_sim!.  With ridge / raft (sz_set_ridgeraft), welding (sz_set_welding) or removal (sz_set_removal) set the batch runs in
// segments that stop only where the host is needed: the schedule is sz_stops.hpp's, SingleStops its passes.  Batches that run through
// (SZ_NO_STOP) and contexts with none of the three set take the driver as it is.
// With an output writer registered (sz_set_floe_output, sz_set_grid_output) every batch takes the schedule, which then also cuts before the
// output steps and records their frames; a batch that runs through (SZ_NO_STOP) carries the output intervals alone in its rules -- no pass
// runs, no tag is looked at.  sz_debug_pipelined then says whether ANY segment ran pipelined: the cuts leave short segments between long ones.
int sz_step(sz_ctx* c, int32_t nsteps, int32_t tstep0, int32_t dt, int32_t coupling_dt, int32_t flags, int32_t* steps_done) {
  if (c && c->rr_pending >= 0) {
    if (steps_done) *steps_done = 0;
    c->err = "sz_step: a ridge / raft step is pending (sz_ridgeraft_pending): sz_step_finish runs its second half first";
    return SZ_E_STATE;
  }
  if (c) c->rr_draws = 0;
  if (c && c->rr_on && c->S.tiled) {
    if (steps_done) *steps_done = 0;
    c->err = "sz_step on a tiled context has no ridge / raft candidate pass (a tile's rows are named by order keys, its ghosts' partners live on other ranks): sz_tile_run, or sz_set_ridgeraft(0)";
    return SZ_E_STATE;
  }
  if (c && c->rec.any_tile) {
    if (steps_done) *steps_done = 0;
    c->err = "sz_step: an output writer of a tiled context is set (sz_tile_set_floe_output / sz_tile_set_grid_output): its record point is collective, sz_tile_run takes it";
    return SZ_E_STATE;
  }
  const bool rec = c && c->rec.any && !c->S.tiled;
  const bool through = (flags & SZ_NO_STOP) != 0;
  const bool weld = c && !through && !c->weld_dts.empty(), rem = c && !through && c->rm_on && !c->S.tiled, rr = c && !through && c->rr_on;
  if (c) c->rec.full = false;
  if (!c || (!weld && !rem && !rr && !rec) || nsteps <= 0) return step_segment(c, nsteps, tstep0, dt, coupling_dt, flags, steps_done);
  if (steps_done) *steps_done = 0;
  if (!c->have_floes) return SZ_E_STATE;
  if (weld) {
    if (c->S.tiled) { c->err = "tiled contexts do not compute welding overlaps (the bins span ranks): sz_set_welding(0)"; return SZ_E_STATE; }
    if (!c->have_domain || !c->have_fields) { c->err = "sz_step with welding set: the bins need the grid extents (sz_set_fields)"; return SZ_E_STATE; }
  }
  if (rr && !(flags & SZ_COLLISIONS_ON)) { c->err = "sz_step with ridge / raft set: the candidates are read from this step's interaction rows (SZ_COLLISIONS_ON)"; return SZ_E_STATE; }
  if (rr && (flags & SZ_COUPLING_ON) && !c->have_fields) { c->err = "sz_set_fields must be called before coupling"; return SZ_E_STATE; }
  SingleStops ops = { c, dt, coupling_dt, flags };
  StopRules rules = through ? StopRules{ 0, 0, nullptr, 0, false, false } : single_stop_rules(*c);
  if (rec) { rules.out_dts = c->rec.dts; rules.n_out = 2 * REC_WRITERS; }
  const int rc = run_with_stops(rules, ops, nsteps, tstep0, steps_done);
  if (rec) c->last_pipelined = ops.pipelined;
  return rc;
}
int sz_debug_next_segment(int32_t tstep, int32_t remaining, int32_t rr_dt, int32_t frac_dt, int32_t cut_on_fracture, int32_t n_weld, const int32_t* dts, int32_t* out4) {
  if (!out4 || tstep < 0 || rr_dt < 0 || frac_dt < 0 || n_weld < 0 || (n_weld > 0 && !dts)) return SZ_E_ARG;
  for (int k = 0; k < n_weld; k++) if (dts[k] <= 0) return SZ_E_ARG;
  const StopRules r = { rr_dt, frac_dt, dts, n_weld, cut_on_fracture != 0, false };
  const Segment g = next_segment(r, tstep, remaining);
  out4[0] = g.rr_step; out4[1] = g.len; out4[2] = g.fstep; out4[3] = g.weld_set;
  return SZ_OK;
}
int sz_debug_next_segment_out(int32_t tstep, int32_t remaining, int32_t rr_dt, int32_t frac_dt, int32_t cut_on_fracture, int32_t n_weld, const int32_t* dts,
                              int32_t n_out, const int32_t* out_dts, int32_t* out4) {
  if (!out4 || tstep < 0 || rr_dt < 0 || frac_dt < 0 || n_weld < 0 || (n_weld > 0 && !dts) || n_out < 0 || (n_out > 0 && !out_dts)) return SZ_E_ARG;
  for (int k = 0; k < n_weld; k++) if (dts[k] <= 0) return SZ_E_ARG;
  for (int k = 0; k < n_out; k++) if (out_dts[k] < 0) return SZ_E_ARG;
  StopRules r = { rr_dt, frac_dt, dts, n_weld, cut_on_fracture != 0, false };
  r.out_dts = out_dts; r.n_out = n_out;
  const Segment g = next_segment(r, tstep, remaining);
  out4[0] = g.rr_step; out4[1] = g.len; out4[2] = g.fstep; out4[3] = g.weld_set;
  return SZ_OK;
}
const char* sz_debug_frame_bits(void) {
  static const std::string names = std::string(COLUMN_NAMES + 1) + FRAME_BIT_TAIL;
  return names.c_str();
}
const char* sz_debug_column_names(void) { return COLUMN_NAMES + 1; }

int sz_profile_enable(sz_ctx* c, int32_t on) {
  if (!c) return SZ_E_ARG;
  c->pmask = on == 1 ? ~0u : on > 1 ? (unsigned)on >> 1 : 0u;
  return SZ_OK;
}
// the instantiation of the dominant kernel as the kernel trace names it (the first narrow variant; its last template argument says whether
// the step's forcings rode in the launch in the last batch): what a profile reader has to look for, derived from the code that ran
int sz_narrow_kernel_name(sz_ctx* c, char* buf, int32_t n) {
  if (!c || !buf || n < 8) return SZ_E_ARG;
  const int frc = c->forcing_where == 2 ? (c->precision == 1 ? 2 : 1) : 0;
  const int args[] = { NARROW_FIRST_ARGS, frc, c->last_pipelined ? 1 : 0 };          // narrow_first<FRC, GEO>, argument by argument
  std::string name = "sz_k_narrow<";
  for (int a : args) name += std::to_string(a) + ",";
  name.back() = '>';
  snprintf(buf, (size_t)n, "%s", name.c_str());
  return SZ_OK;
}
int sz_forcing_launch(sz_ctx* c, int32_t* where) {
  if (!c || !where) return SZ_E_ARG;
  *where = c->forcing_where;
  return SZ_OK;
}
int sz_profile_reset(sz_ctx* c) {
  if (!c) return SZ_E_ARG;
  for (int k = 0; k < NK; k++) { c->kms[k] = 0; c->kl[k] = 0; }
  c->ev_used = 0;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemsetAsync(c->S.acc, 0, (size_t)ACC_SLOTS * 8 * sizeof(unsigned long long), c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
int sz_kernel_time_ms(sz_ctx* c, int32_t k, double* ms, int64_t* launches) {
  if (!c || k < 0 || k >= NK) return SZ_E_ARG;
  if (ms) *ms = c->kms[k];
  if (launches) *launches = c->kl[k];
  return SZ_OK;
}

}  // extern "C"
// ---------------------------------------------------------------- tiled contexts: behind the batch drivers and passes they call into
#include "sz_tile_host.hpp"
extern "C" {

// ---------------------------------------------------------------- debug hooks
// test hook: quads of the collision records (State::crec) of the owned parents that differ from the columns they cache; *n_bad = -1 when the last
// resident batch did not run on records
int sz_debug_crec_mismatches(sz_ctx* c, int64_t* n_bad) {
  if (!c || !c->have_floes || !n_bad) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  if (!c->crec_buf || !c->crec_was_live) { *n_bad = -1; return SZ_OK; }
  int h[C_COUNT];
  int rc = sync_and_check(c, h); if (rc) return rc;
  unsigned long long* d = (unsigned long long*)(c->S.cnt + C_COUNT + 64 + 68);      // (two spare words of the counter block)
  HIPCHK(c, hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(sz_k_crec_check, dim3(grid_for(c->hostN, 256)), dim3(256), 0, c->stream, c->S, (const double2*)c->crec_buf, c->hostN, d);
  unsigned long long v = 0;
  HIPCHK(c, hipMemcpyAsync(&v, d, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *n_bad = (int64_t)v;
  return SZ_OK;
}
// diagnosis: the ghost / halo row that carried order key `key` in the last resident step that used ghost allocator `slot` (step s of a batch,
// 0-based: s & 1), as the collision kernels saw it: out[0] = row (-1: none), cx, cy, u, v, xi, rmax, area, height, box, ring points, parent,
// status, ring x (20) and y (20) -- 56 doubles
int sz_debug_find_key(sz_ctx* c, int32_t slot, int64_t key, double* out56) {
  if (!c || !c->have_floes || !out56 || slot < 0 || slot > 1) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  double* d = nullptr;
  HIPCHK(c, hipMalloc((void**)&d, 56 * sizeof(double)));
  hipLaunchKernelGGL(sz_k_debug_find_key, dim3(1), dim3(64), 0, c->stream, c->S, slot, (long long)key, c->hostN, d);
  HIPCHK(c, hipMemcpyAsync(out56, d, 56 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipFree(d);
  return SZ_OK;
}
// diagnosis: the pair items of the last resident step (ghost allocator `slot`) between the instances of two floe ids: out[0] = entries (at most 12
// returned), then {owner key, partner key, contact rows, owner row, partner row} each -- 61 doubles
int sz_debug_pairs_of_ids(sz_ctx* c, int32_t slot, int64_t id_a, int64_t id_b, double* out61) {
  if (!c || !c->have_floes || !out61 || slot < 0 || slot > 1) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  double* d = nullptr;
  HIPCHK(c, hipMalloc((void**)&d, 61 * sizeof(double)));
  HIPCHK(c, hipMemsetAsync(d, 0, 61 * sizeof(double), c->stream));
  hipLaunchKernelGGL(sz_k_debug_pairs_of_ids, dim3(1), dim3(64), 0, c->stream, c->S, slot, (long long)id_a, (long long)id_b, c->hostN, d, 12);
  HIPCHK(c, hipMemcpyAsync(out61, d, 61 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipFree(d);
  return SZ_OK;
}
// diagnostic build only: cycles per narrow-phase stage, summed over groups (zeros otherwise)
int sz_debug_stamps(sz_ctx* c, long long* out16) {
  if (!c || !c->have_floes || !out16) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpy(out16, c->S.stamps, (512 + 8 * 8000) * sizeof(long long), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemset(c->S.stamps, 0, (512 + 8 * 8000) * sizeof(long long)));
  return SZ_OK;
}

// ---------------------------------------------------------------- output path

// shared front of the grid-output calls: argument checks, grid lines to the device, cell areas
// (the memory comes from `pool`: a call's own, freed behind it, or the recorder's workspace, which stays -- eul_grid_bytes / eul_fill_bytes say how
//  much a pool of one chunk must hold)
int eul_check_lines(sz_ctx* c, int32_t nx, int32_t ny, const double* xg, const double* yg) {
  if (nx < 1 || ny < 1 || !xg || !yg) return SZ_E_ARG;
  const double dx = xg[1] - xg[0], dy = yg[1] - yg[0];
  if (!(dx > 0) || !(dy > 0)) { c->err = "grid lines must ascend"; return SZ_E_ARG; }
  for (int k = 0; k <= nx; k++) if (fabs(xg[k] - (xg[0] + k * dx)) > 1e-6 * dx) { c->err = "x grid lines must be evenly spaced"; return SZ_E_ARG; }
  for (int k = 0; k <= ny; k++) if (fabs(yg[k] - (yg[0] + k * dy)) > 1e-6 * dy) { c->err = "y grid lines must be evenly spaced"; return SZ_E_ARG; }
  return SZ_OK;
}
static size_t pool_bytes(size_t n, size_t size) { return ((n ? n : 1) * size + 255) & ~(size_t)255; }          // (what dalloc carves for n elements)
size_t eul_grid_bytes(int nx, int ny) {
  const size_t ncell = (size_t)nx * ny;
  return pool_bytes(nx + 1, 8) + pool_bytes(ny + 1, 8) + pool_bytes(1, sizeof(int)) + pool_bytes(ncell, 8) + pool_bytes((size_t)EUL_COUNT * ncell, 8);
}
int eul_grid(sz_ctx* c, int32_t nx, int32_t ny, const double* xg, const double* yg, Pool& pool, EulGrid& E) {
  if (int rc = eul_check_lines(c, nx, ny, xg, yg)) return rc;
  (void)hipSetDevice(c->device);
  world_rings(c);
  int rc = sync_and_check(c);          // hostM current, nothing pending
  if (rc) return rc;
  const int ncell = nx * ny;
  E = EulGrid{};
  E.nx = nx; E.ny = ny; E.M = c->hostM > 0 ? c->hostM : 1;
  double *d_xg, *d_yg;
  if ((rc = dalloc(c, &d_xg, nx + 1, pool)) || (rc = dalloc(c, &d_yg, ny + 1, pool)) || (rc = dalloc(c, &E.count, 1, pool)) ||
      (rc = dalloc(c, &E.cell_area, ncell, pool)) || (rc = dalloc(c, &E.data, (size_t)EUL_COUNT * ncell, pool))) return rc;
  H2D(d_xg, xg, nx + 1, double); H2D(d_yg, yg, ny + 1, double);
  E.xg = d_xg; E.yg = d_yg;
  hipLaunchKernelGGL(sz_k_eul_cell_area, dim3(grid_for(ncell, 256, 8192)), dim3(256), 0, c->stream, c->S, E);
  return SZ_OK;
}
// entries: counted ...
int eul_count(sz_ctx* c, EulGrid& E, int& nent) {
  hipLaunchKernelGGL(sz_k_eul_entries, dim3(grid_for(c->S.capM, 256)), dim3(256), 0, c->stream, c->S, E, 0);
  nent = 0;
  HIPCHK(c, hipMemcpyAsync(&nent, E.count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (nent < 0) { c->err = "output grid: entry count overflow"; return SZ_E_CAPACITY; }
  return SZ_OK;
}
static unsigned eul_key_bits(const EulGrid& E) {
  unsigned long long top = (unsigned long long)E.nx * E.ny * (unsigned long long)E.M;
  unsigned bits = 1; while (bits < 64 && (top >> bits)) bits++;
  return bits;
}
int eul_fill_bytes(sz_ctx* c, const EulGrid& E, int nent, size_t* bytes) {
  size_t tmp_bytes = 0;
  if (nent > 0) HIPCHK(c, rocprim::radix_sort_keys(nullptr, tmp_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (size_t)nent, 0u, eul_key_bits(E), c->stream));
  *bytes = 3 * pool_bytes(nent, 8) + pool_bytes(tmp_bytes, 1);
  return SZ_OK;
}
// ... then sized, filled and sorted, and the area of every entry
int eul_fill(sz_ctx* c, Pool& pool, EulGrid& E, int nent) {
  State& S = c->S;
  int rc;
  unsigned long long* keys_in = nullptr;
  E.cap = nent;
  if ((rc = dalloc(c, &keys_in, nent, pool)) || (rc = dalloc(c, &E.keys, nent, pool)) || (rc = dalloc(c, &E.pic, nent, pool))) return rc;
  if (nent == 0) return SZ_OK;
  HIPCHK(c, hipMemsetAsync(E.count, 0, sizeof(int), c->stream));
  EulGrid Ein = E; Ein.keys = keys_in;
  hipLaunchKernelGGL(sz_k_eul_entries, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S, Ein, 1);
  const unsigned bits = eul_key_bits(E);
  size_t tmp_bytes = 0;
  HIPCHK(c, rocprim::radix_sort_keys(nullptr, tmp_bytes, keys_in, E.keys, (size_t)nent, 0u, bits, c->stream));
  char* tmp = nullptr;
  if ((rc = dalloc(c, &tmp, tmp_bytes, pool))) return rc;
  HIPCHK(c, rocprim::radix_sort_keys((void*)tmp, tmp_bytes, keys_in, E.keys, (size_t)nent, 0u, bits, c->stream));
  if (S.nelem > 4) hipLaunchKernelGGL(sz_k_eul_area, dim3(grid_for(nent, 64 / EU_G, 1 << 16)), dim3(64), 0, c->stream, S, E, nent);
  else hipLaunchKernelGGL(sz_k_eul_area_rect, dim3(grid_for(nent, 256, 1 << 16)), dim3(256), 0, c->stream, S, E, nent);
  return SZ_OK;
}
int eul_entries(sz_ctx* c, Pool& pool, EulGrid& E, int& nent) {
  if (int rc = eul_count(c, E, nent)) return rc;
  return eul_fill(c, pool, E, nent);
}
int eul_check_outputs(sz_ctx* c, int32_t nout, const int32_t* outputs, const double* data) {
  if (nout < 0 || (nout > 0 && (!outputs || !data))) return SZ_E_ARG;
  for (int k = 0; k < nout; k++) if (outputs[k] < 0 || outputs[k] >= EUL_COUNT) { c->err = "unknown grid output"; return SZ_E_ARG; }
  return SZ_OK;
}
int eul_copy_out(sz_ctx* c, const EulGrid& E, int32_t nout, const int32_t* outputs, double* data) {
  const size_t ncell = (size_t)E.nx * E.ny;
  for (int k = 0; k < nout; k++)
    HIPCHK(c, hipMemcpyAsync(data + (size_t)k * ncell, E.data + (size_t)outputs[k] * ncell, ncell * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  return sync_and_check(c);
}

// calc_eulerian_data! (output.jl:793-914) on the rows the context holds (parents and, if the caller ran
// sz_add_ghosts, ghosts -- write_data! runs after add_ghosts!, simulation.jl:102-105)
int sz_eulerian_data(sz_ctx* c, int32_t nx, int32_t ny, const double* xg, const double* yg, int32_t nout,
                     const int32_t* outputs, double* data) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  int rc = eul_check_outputs(c, nout, outputs, data);
  if (rc) return rc;
  if (c->S.tiled) { c->err = "tiled contexts: sz_eulerian_partial, all-reduce, sz_eulerian_finish"; return SZ_E_STATE; }
  PoolGuard pool; EulGrid E; int nent = 0;
  if ((rc = eul_grid(c, nx, ny, xg, yg, pool.v, E)) || (rc = eul_entries(c, pool.v, E, nent))) return rc;
  hipLaunchKernelGGL(sz_k_eul_reduce, dim3(grid_for(nx * ny, 64)), dim3(64), 0, c->stream, c->S, E, nent);
  return eul_copy_out(c, E, nout, outputs, data);
}
// tiled runs, first half: this rank's per-cell sums into d_partial (SZ_EUL_PARTIAL * nx * ny doubles on the device)
int sz_eulerian_partial(sz_ctx* c, int32_t nx, int32_t ny, const double* xg, const double* yg, void* d_partial) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (!d_partial) return SZ_E_ARG;
  PoolGuard pool; EulGrid E; int nent = 0, rc;
  if ((rc = eul_grid(c, nx, ny, xg, yg, pool.v, E)) || (rc = eul_entries(c, pool.v, E, nent))) return rc;
  hipLaunchKernelGGL(sz_k_eul_partial, dim3(grid_for(nx * ny, 64)), dim3(64), 0, c->stream, c->S, E, nent, (double*)d_partial);
  return sync_and_check(c);
}
// second half: the summed buffer -> the averages
int sz_eulerian_finish(sz_ctx* c, int32_t nx, int32_t ny, const double* xg, const double* yg, const void* d_partial, int32_t nout,
                       const int32_t* outputs, double* data) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (!d_partial) return SZ_E_ARG;
  int rc = eul_check_outputs(c, nout, outputs, data);
  if (rc) return rc;
  PoolGuard pool; EulGrid E;
  if ((rc = eul_grid(c, nx, ny, xg, yg, pool.v, E))) return rc;
  hipLaunchKernelGGL(sz_k_eul_finish, dim3(grid_for(nx * ny, 64)), dim3(64), 0, c->stream, E, (const double*)d_partial);
  return eul_copy_out(c, E, nout, outputs, data);
}

// ---------------------------------------------------------------- output recorder (sz_record.hpp)
// a workspace chunk as a pool of one chunk for the eul_* helpers; work_keep() takes back whatever the round left (the same chunk, when it was
// reserved large enough)
static int work_reserve(sz_ctx* c, RecWork& w, size_t need) {
  if (w.bytes >= need) return SZ_OK;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  (void)hipFree(w.p); w.p = nullptr; w.bytes = 0;
  need = (need + need / 4 + 255) & ~(size_t)255;          // (a quarter to spare: the entry count wanders from frame to frame)
  HIPCHK(c, hipMalloc((void**)&w.p, need));
  w.bytes = need;
  return SZ_OK;
}
static Pool work_pool(const RecWork& w) { Pool p; p.chunks.push_back(w.p); p.sizes.push_back(w.bytes); return p; }
static void work_keep(RecWork& w, Pool& p) {
  for (size_t k = 1; k < p.chunks.size(); k++) (void)hipFree(p.chunks[k]);
  w.p = p.chunks.empty() ? nullptr : (char*)p.chunks[0]; w.bytes = p.chunks.empty() ? 0 : p.sizes[0];
  p.chunks.clear(); p.sizes.clear();
}
static void rec_free_floe(FloeWriter& w) { (void)hipFree(w.arena); w = FloeWriter{}; }
static void rec_free_grid(GridWriter& g) { (void)hipFree(g.store); g = GridWriter{}; }
static void rec_free_all(sz_ctx* c) {
  for (int w = 0; w < REC_WRITERS; w++) { rec_free_floe(c->rec.floe[w]); rec_free_grid(c->rec.grid[w]); }
  (void)hipFree(c->rec.grid_work.p); (void)hipFree(c->rec.entry_work.p); (void)hipFree(c->rec.part_work.p);
  (void)hipFree(c->rec.list_work.p);
  c->rec = Recorder{};
}
// the setters of the single context (tile = false) and of a tiled one (sz_tile_set_*): the same arguments and checks, each kind refuses the other's context
static int rec_setter_checks(sz_ctx* c, int32_t writer, int32_t dt_out, bool tile) {
  if (!c) return SZ_E_ARG;
  if (writer < 0 || writer >= REC_WRITERS) { c->err = "output writer index out of range (0..3)"; return SZ_E_ARG; }
  if (dt_out < 0) { c->err = "output interval must not be negative (0 turns the writer off)"; return SZ_E_ARG; }
  if (c->S.tiled && !tile) { c->err = "sz_set_floe_output / sz_set_grid_output serve single contexts only: a tiled context takes sz_tile_set_floe_output / sz_tile_set_grid_output"; return SZ_E_STATE; }
  if (!c->S.tiled && tile) { c->err = "sz_tile_set_floe_output / sz_tile_set_grid_output need a tiled context (sz_tile_enable): a single context takes sz_set_floe_output / sz_set_grid_output"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
static int rec_set_floe(sz_ctx* c, int32_t writer, int32_t dt_out, uint64_t columns_mask, int64_t arena_bytes, bool tile) {
  if (int rc = rec_setter_checks(c, writer, dt_out, tile)) return rc;
  if (dt_out > 0 && (columns_mask == 0 || (columns_mask >> FR_NBITS) != 0)) { c->err = "sz_set_floe_output: the mask selects no column group, or one that does not exist (sz_debug_frame_bits)"; return SZ_E_ARG; }
  if (dt_out > 0 && arena_bytes < (int64_t)FR_HEADER) { c->err = "sz_set_floe_output: the arena holds no frame"; return SZ_E_ARG; }
  FloeWriter& w = c->rec.floe[writer];
  rec_free_floe(w);
  if (dt_out > 0) {
    HIPCHK(c, hipMalloc((void**)&w.arena, (size_t)arena_bytes));
    w.dt = dt_out; w.mask = columns_mask; w.bytes = (size_t)arena_bytes; w.tile = tile;
  }
  c->rec.refresh();
  return SZ_OK;
}
static int rec_set_grid(sz_ctx* c, int32_t writer, int32_t dt_out, int32_t nx, int32_t ny, const double* xg, const double* yg, int32_t nout,
                        const int32_t* outputs, int32_t max_frames, bool tile);
int sz_set_floe_output(sz_ctx* c, int32_t writer, int32_t dt_out, uint64_t columns_mask, int64_t arena_bytes) { return rec_set_floe(c, writer, dt_out, columns_mask, arena_bytes, false); }
int sz_tile_set_floe_output(sz_ctx* c, int32_t writer, int32_t dt_out, uint64_t columns_mask, int64_t arena_bytes) { return rec_set_floe(c, writer, dt_out, columns_mask, arena_bytes, true); }
int sz_set_floe_output_lists(sz_ctx* c, int32_t writer, uint32_t lists) {
  if (!c) return SZ_E_ARG;
  if (writer < 0 || writer >= REC_WRITERS) { c->err = "output writer index out of range (0..3)"; return SZ_E_ARG; }
  if (lists & ~FR_LIST_ALL) { c->err = "sz_set_floe_output_lists: a list that does not exist (SZ_FRAME_INTERACTIONS | SZ_FRAME_SUBPOINTS)"; return SZ_E_ARG; }
  FloeWriter& w = c->rec.floe[writer];
  if (c->S.tiled || w.tile) { c->err = "sz_set_floe_output_lists: tile frames record no lists yet (single contexts, writers of sz_set_floe_output) through this setter: a writer of sz_tile_set_floe_output takes sz_tile_set_floe_output_lists"; return SZ_E_STATE; }
  if (w.dt == 0) { c->err = "sz_set_floe_output_lists: the writer is off (sz_set_floe_output first)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  w.frames.clear(); w.used = 0; w.lists = lists;
  return SZ_OK;
}
// the lists of a tiled context's writer (behind sz_tile_set_floe_output, which resets them; the same word on every rank: tile_rec_agree_settings)
int sz_tile_set_floe_output_lists(sz_ctx* c, int32_t writer, uint32_t lists) {
  if (!c) return SZ_E_ARG;
  if (writer < 0 || writer >= REC_WRITERS) { c->err = "output writer index out of range (0..3)"; return SZ_E_ARG; }
  if (lists & ~FR_LIST_ALL) { c->err = "sz_tile_set_floe_output_lists: a list that does not exist (SZ_FRAME_INTERACTIONS | SZ_FRAME_SUBPOINTS)"; return SZ_E_ARG; }
  FloeWriter& w = c->rec.floe[writer];
  if (w.dt == 0) { c->err = "sz_tile_set_floe_output_lists: the writer is off (sz_tile_set_floe_output first)"; return SZ_E_STATE; }
  if (!c->S.tiled || !w.tile) { c->err = "sz_tile_set_floe_output_lists: not a writer of sz_tile_set_floe_output (a single context's writer takes sz_set_floe_output_lists)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  w.frames.clear(); w.used = 0; w.lists = lists;
  return SZ_OK;
}
int sz_set_grid_output(sz_ctx* c, int32_t writer, int32_t dt_out, int32_t nx, int32_t ny, const double* xg, const double* yg, int32_t nout,
                       const int32_t* outputs, int32_t max_frames) { return rec_set_grid(c, writer, dt_out, nx, ny, xg, yg, nout, outputs, max_frames, false); }
int sz_tile_set_grid_output(sz_ctx* c, int32_t writer, int32_t dt_out, int32_t nx, int32_t ny, const double* xg, const double* yg, int32_t nout,
                            const int32_t* outputs, int32_t max_frames) { return rec_set_grid(c, writer, dt_out, nx, ny, xg, yg, nout, outputs, max_frames, true); }
static int rec_set_grid(sz_ctx* c, int32_t writer, int32_t dt_out, int32_t nx, int32_t ny, const double* xg, const double* yg, int32_t nout,
                        const int32_t* outputs, int32_t max_frames, bool tile) {
  if (int rc = rec_setter_checks(c, writer, dt_out, tile)) return rc;
  if (dt_out > 0) {
    if (int rc = eul_check_lines(c, nx, ny, xg, yg)) return rc;
    if (nout < 1 || !outputs || max_frames < 1) return SZ_E_ARG;
    for (int k = 0; k < nout; k++) if (outputs[k] < 0 || outputs[k] >= EUL_COUNT) { c->err = "unknown grid output"; return SZ_E_ARG; }
  }
  GridWriter& g = c->rec.grid[writer];
  rec_free_grid(g);
  if (dt_out > 0) {
    HIPCHK(c, hipMalloc((void**)&g.store, (size_t)max_frames * nout * nx * ny * sizeof(double)));
    g.dt = dt_out; g.nx = nx; g.ny = ny; g.max_frames = max_frames; g.tile = tile;
    g.xg.assign(xg, xg + nx + 1); g.yg.assign(yg, yg + ny + 1); g.outputs.assign(outputs, outputs + nout);
    if (int rc = work_reserve(c, c->rec.grid_work, eul_grid_bytes(nx, ny))) return rc;
  }
  c->rec.refresh();
  return SZ_OK;
}
// one floe frame: the layout from the host's counts, one launch
static int rec_pack(sz_ctx* c, FloeWriter& w, int tstep, int V) {
  const int M = c->hostM, N = c->hostN;
  const FrameLayout L(w.mask, M, N, V);
  FramePack F;
  const ColTable<double*> src = state_columns(c->S);
  for (int k = 0; k < MIG_NTAB; k++) F.col[k] = src.p[k];
  for (int k = 0; k < FR_NSEC; k++) F.off[k] = L.off[k];
  F.dst = w.arena + w.used; F.tstep = tstep; F.M = M; F.N = N; F.V = V;
  F.key_off = 0; F.spare[0] = F.spare[1] = F.spare[2] = 0;
  const long long widest = std::max<long long>(4ll * M, V);
  hipLaunchKernelGGL(sz_k_frame_pack<false>, dim3(grid_for(widest, FP_TPB, 256), FP_SLICES), dim3(FP_TPB), 0, c->stream, c->S, F);
  w.frames.push_back({ w.used, tstep, M, N, V, {} });
  w.used += (size_t)L.total;
  return SZ_OK;
}
// one grid frame: the averages of sz_eulerian_data in the recorder's workspace, the wanted outputs copied into the store on the device
static int rec_grid(sz_ctx* c, GridWriter& g, int tstep) {
  Recorder& R = c->rec;
  EulGrid E; int nent = 0, rc;
  if ((rc = work_reserve(c, R.grid_work, eul_grid_bytes(g.nx, g.ny)))) return rc;
  Pool gp = work_pool(R.grid_work);
  rc = eul_grid(c, g.nx, g.ny, g.xg.data(), g.yg.data(), gp, E);
  work_keep(R.grid_work, gp);
  size_t need = 0;
  if (rc || (rc = eul_count(c, E, nent)) || (rc = eul_fill_bytes(c, E, nent, &need)) || (rc = work_reserve(c, R.entry_work, need))) return rc;
  Pool ep = work_pool(R.entry_work);
  rc = eul_fill(c, ep, E, nent);
  work_keep(R.entry_work, ep);
  if (rc) return rc;
  const size_t ncell = (size_t)g.nx * g.ny, nout = g.outputs.size();
  hipLaunchKernelGGL(sz_k_eul_reduce, dim3(grid_for((long long)ncell, 64)), dim3(64), 0, c->stream, c->S, E, nent);
  double* dst = g.store + g.tsteps.size() * nout * ncell;
  for (size_t k = 0; k < nout; k++)
    HIPCHK(c, hipMemcpyAsync(dst + k * ncell, E.data + (size_t)g.outputs[k] * ncell, ncell * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  g.tsteps.push_back(tstep);
  return SZ_OK;
}
// The workspace of the lists (Recorder::list_work), carved for a context of capM rows: the sorted keys, the keys on their way up, the counts and
// the scanned offsets of both lists, the sort's scratch.  Sized by the capacity, not by the counts, so that what is sorted before sz_add_ghosts
// stays where it is when the counts are known.
struct ListWork {
  long long *keys, *keys_in; int *n_inter, *n_sub, *ioff, *soff; void* tmp; size_t tmp_bytes;
};
static int rec_list_work(sz_ctx* c, ListWork& W) {
  const size_t cap = (size_t)c->S.capM + 2, ints = (cap * sizeof(int) + 7) & ~(size_t)7;
  size_t tb = 0;
  HIPCHK(c, rocprim::radix_sort_keys(nullptr, tb, (long long*)nullptr, (long long*)nullptr, cap, 0, 64, c->stream));
  tb = (tb + 255) & ~(size_t)255;
  if (int rc = work_reserve(c, c->rec.list_work, 2 * cap * sizeof(long long) + 4 * ints + tb)) return rc;
  char* p = c->rec.list_work.p;
  W.keys = (long long*)p; p += cap * sizeof(long long); W.keys_in = (long long*)p; p += cap * sizeof(long long);
  W.n_inter = (int*)p; p += ints; W.n_sub = (int*)p; p += ints; W.ioff = (int*)p; p += ints; W.soff = (int*)p; p += ints;
  W.tmp = p; W.tmp_bytes = tb;
  return SZ_OK;
}
// the order keys of the last step's inline ghosts, sorted, into the workspace: what the interactions section translates partners with.  To be
// called BEFORE sz_add_ghosts, which clears gi_valid and reuses the key table.  Keys not fetched yet are sorted where they are, on the device
// (gi_pending stays: nothing is fetched); keys the host holds already are uploaded.  *nkeys == 0: nothing to translate, as
// sz_download_interactions would translate nothing.
static int rec_list_keys(sz_ctx* c, int* nkeys) {
  *nkeys = 0;
  if (!c->gi_valid) return SZ_OK;
  ListWork W;
  if (int rc = rec_list_work(c, W)) return rc;
  const int G = c->gi_pending ? c->gi_pending_n : (int)c->gi_keys.size();
  if (G <= 0 || G > c->S.capM) return SZ_OK;
  const long long* src = c->S.gkeys + (size_t)c->gi_pending_slot * c->S.capM;
  if (!c->gi_pending) {
    HIPCHK(c, hipMemcpyAsync(W.keys_in, c->gi_keys.data(), (size_t)G * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    src = W.keys_in;
  }
  size_t tb = 0;
  HIPCHK(c, rocprim::radix_sort_keys(nullptr, tb, src, W.keys, (size_t)G, 0, 64, c->stream));
  if (tb > W.tmp_bytes) { c->err = "the recorder's key sort needs more scratch than its workspace holds"; return SZ_E_STATE; }
  HIPCHK(c, rocprim::radix_sort_keys(W.tmp, tb, src, W.keys, (size_t)G, 0, 64, c->stream));
  *nkeys = G;
  return SZ_OK;
}
// the counts of both lists over the rows behind sz_add_ghosts and their scans; the totals go into two spare words of the counter block and
// reach the host with the counter fetch the record point does anyway
static int rec_list_scans(sz_ctx* c, unsigned lists) {
  ListWork W;
  if (int rc = rec_list_work(c, W)) return rc;
  const int M = c->hostM, N = c->hostN;
  hipLaunchKernelGGL(sz_k_frame_list_counts, dim3(grid_for(M + 1, FP_TPB, 256)), dim3(FP_TPB), 0, c->stream, c->S, lists & FR_LIST_INTER ? W.n_inter : nullptr,
                     lists & FR_LIST_SUB ? W.n_sub : nullptr, M, N);
  if (lists & FR_LIST_INTER) scan(c, W.n_inter, W.ioff, M, -1, M, C_SCRATCH0);
  if (lists & FR_LIST_SUB) scan(c, W.n_sub, W.soff, M, -1, M, C_SCRATCH1);
  return SZ_OK;
}
// the list sections of the frame rec_pack has just appended to w: one launch
static int rec_pack_lists(sz_ctx* c, FloeWriter& w, long long R, long long S, int nkeys) {
  ListWork W;
  if (int rc = rec_list_work(c, W)) return rc;
  FloeFrame& fr = w.frames.back();
  const long long base = FrameLayout(w.mask, fr.M, fr.N, fr.V).total;
  fr.lists = w.lists; fr.R = w.lists & FR_LIST_INTER ? R : 0; fr.S = w.lists & FR_LIST_SUB ? S : 0;
  const ListLayout L(base, fr.lists, fr.M, fr.R, fr.S);
  FrameLists F;
  for (int k = 0; k < FL_NSEC; k++) F.off[k] = L.off[k];
  F.dst = w.arena + fr.at; F.ioff = W.ioff; F.soff = W.soff; F.keys = W.keys; F.nkeys = nkeys; F.M = fr.M; F.N = fr.N; F.lists = fr.lists; F.R = fr.R; F.S = fr.S; F.keep_spare = 0;
  const long long widest = std::max<long long>(std::max<long long>(7 * fr.R, fr.S), fr.M + 1);
  hipLaunchKernelGGL(sz_k_frame_lists, dim3(grid_for(widest, FP_TPB, 256), 2), dim3(FP_TPB), 0, c->stream, c->S, F);
  w.used = fr.at + (size_t)L.total;
  return SZ_OK;
}
// write_data! of output step tstep, in front of the segment that starts there (run_with_stops).  *full: a due writer has no room for its
// frame -- nothing is recorded for this step, the batch ends in front of it.
static int rec_record(sz_ctx* c, int tstep, int* full) {
  Recorder& R = c->rec;
  *full = 0;
  bool fdue[REC_WRITERS], gdue[REC_WRITERS], any = false;
  for (int w = 0; w < REC_WRITERS; w++) { fdue[w] = step_due(R.floe[w].dt, tstep); gdue[w] = step_due(R.grid[w].dt, tstep); any = any || fdue[w] || gdue[w]; }
  if (!any) return SZ_OK;
  for (int w = 0; w < REC_WRITERS; w++) if (gdue[w] && (int)R.grid[w].tsteps.size() >= R.grid[w].max_frames) { *full = 1; R.full = true; return SZ_OK; }
  int rc, h[C_COUNT], nkeys = 0;
  (void)hipSetDevice(c->device);
  unsigned lists = 0;          // the lists some due writer records: a writer without lists adds no launch, no scan and no synchronisation
  for (int w = 0; w < REC_WRITERS; w++) if (fdue[w]) lists |= R.floe[w].lists;
  if ((lists & FR_LIST_INTER) && (rc = rec_list_keys(c, &nkeys))) return rc;
  const char* const keys_in = R.list_work.p;
  if ((c->ghosts_staged || c->hostM != c->hostN) && (rc = sz_remove_ghosts(c))) return rc;          // (ghosts a process-mode call left attached: a batch drops them too)
  if ((rc = sz_add_ghosts(c)) || (lists && (rc = rec_list_scans(c, lists))) || (rc = fetch_counters(c, h))) return rc;
  if (nkeys > 0 && R.list_work.p != keys_in) { c->err = "the recorder's workspace moved under the sorted ghost keys (sz_add_ghosts grew the list)"; return SZ_E_STATE; }
  const int V = h[C_NV];
  const long long nR = lists & FR_LIST_INTER ? h[C_SCRATCH0] : 0, nS = lists & FR_LIST_SUB ? h[C_SCRATCH1] : 0;
  auto frame_total = [&](const FloeWriter& fw) {
    const long long base = FrameLayout(fw.mask, c->hostM, c->hostN, V).total;
    return (size_t)(fw.lists ? ListLayout(base, fw.lists, c->hostM, nR, nS).total : base);
  };
  for (int w = 0; w < REC_WRITERS; w++)
    if (fdue[w] && R.floe[w].used + frame_total(R.floe[w]) > R.floe[w].bytes) { *full = 1; R.full = true; }
  for (int w = 0; w < REC_WRITERS && !*full; w++)
    if (fdue[w] && ((rc = rec_pack(c, R.floe[w], tstep, V)) || (R.floe[w].lists && (rc = rec_pack_lists(c, R.floe[w], nR, nS, nkeys))))) return rc;
  for (int w = 0; w < REC_WRITERS && !*full; w++) if (gdue[w] && (rc = rec_grid(c, R.grid[w], tstep))) return rc;
  return sz_remove_ghosts(c);
}
int sz_output_frames(sz_ctx* c, int32_t* n_floe, int32_t* n_grid, int32_t* full) {
  if (!c) return SZ_E_ARG;
  for (int w = 0; w < REC_WRITERS; w++) { if (n_floe) n_floe[w] = (int32_t)c->rec.floe[w].frames.size(); if (n_grid) n_grid[w] = (int32_t)c->rec.grid[w].tsteps.size(); }
  if (full) *full = c->rec.full;
  return SZ_OK;
}
static const FloeFrame* rec_floe_frame(sz_ctx* c, int32_t writer, int32_t k) {
  if (!c) return nullptr;
  if (writer < 0 || writer >= REC_WRITERS || k < 0 || k >= (int)c->rec.floe[writer].frames.size()) { c->err = "no such floe frame (sz_output_frames)"; return nullptr; }
  return &c->rec.floe[writer].frames[k];
}
int sz_floe_frame_info(sz_ctx* c, int32_t writer, int32_t k, int64_t* tstep, int64_t* M, int64_t* N, int64_t* n_ring_points, int64_t* n_ghost_links) {
  const FloeFrame* f = rec_floe_frame(c, writer, k);
  if (!f) return SZ_E_ARG;
  if (tstep) *tstep = f->tstep;
  if (M) *M = f->M;
  if (N) *N = f->N;
  if (n_ring_points) *n_ring_points = f->V;
  if (n_ghost_links) *n_ghost_links = f->M - f->N;
  return SZ_OK;
}
// a frame of M rows (N parents), V ring points in layout L at d_frame: down in one copy, its sections into the non-NULL members of f
// LL (a frame with the sub-floe points section): sub_off, sx, sy come down too, S points, in copies of their own
static int rec_frame_down(sz_ctx* c, const char* who, const FrameLayout& L, long long M, long long N, long long V, const char* d_frame, sz_floe_columns* f,
                          const ListLayout* LL = nullptr, long long S = 0) {
  const long long G = M - N;
  struct Part { void* dst; int sec; long long bytes; };
  std::vector<Part> parts;
  const ColTable<double*> dst = host_columns(*f);
  for (int q = 0; q < MIG_NTAB; q++) parts.push_back({ dst.p[q], q, (long long)col_width(q) * M * 8 });
  parts.push_back({ f->id, FR_ID, M * 8 }); parts.push_back({ f->ghost_id, FR_GHOST_ID, M * 8 }); parts.push_back({ f->status, FR_STATUS, M * 4 });
  parts.push_back({ f->vert_off, FR_VOFF, (M + 1) * 4 }); parts.push_back({ f->vx, FR_VX, V * 8 }); parts.push_back({ f->vy, FR_VY, V * 8 });
  parts.push_back({ f->ghost_off, FR_GOFF, (M + 1) * 4 }); parts.push_back({ f->ghost_idx, FR_GIDX, G * 4 });
  for (const Part& p : parts) if (p.dst && L.off[p.sec] < 0) { c->err = std::string(who) + ": a member is asked for that the writer's mask did not record"; return SZ_E_ARG; }
  const bool subs = LL && LL->off[FL_SOFF] >= 0;
  if ((f->sub_off || f->sx || f->sy) && !subs) { c->err = std::string(who) + ": this frame did not record the sub-floe points (sz_set_floe_output_lists)"; return SZ_E_ARG; }
  if (!d_frame) return SZ_OK;          // (the members were only checked)
  (void)hipSetDevice(c->device);
  // the frame comes down in one copy
  std::vector<char>& host = c->rec.host;
  host.resize((size_t)L.total);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host.data(), d_frame, (size_t)L.total, hipMemcpyDeviceToHost));
  for (const Part& p : parts) if (p.dst && p.bytes > 0) memcpy(p.dst, host.data() + L.off[p.sec], (size_t)p.bytes);
  if (subs) {
    if (f->sub_off) HIPCHK(c, hipMemcpy(f->sub_off, d_frame + LL->off[FL_SOFF], (size_t)(M + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (f->sx && S > 0) HIPCHK(c, hipMemcpy(f->sx, d_frame + LL->off[FL_SX], (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
    if (f->sy && S > 0) HIPCHK(c, hipMemcpy(f->sy, d_frame + LL->off[FL_SY], (size_t)S * sizeof(double), hipMemcpyDeviceToHost));
  }
  return SZ_OK;
}
// where the list sections of a frame lie: behind the columns; in a tile frame behind its keys and its key table
static ListLayout rec_list_layout(const FloeWriter& w, const FloeFrame& fr) {
  if (w.tile && !fr.ranks.empty()) {
    return ListLayout(TileListLayout(w.mask, fr.lists, fr.M, fr.N, fr.V, fr.R, fr.S, fr.K).base, fr.lists, fr.M, fr.R, fr.S);
  }
  return ListLayout(FrameLayout(w.mask, fr.M, fr.N, fr.V).total, fr.lists, fr.M, fr.R, fr.S);
}
int sz_download_floe_frame(sz_ctx* c, int32_t writer, int32_t k, sz_floe_columns* f) {
  const FloeFrame* fr = rec_floe_frame(c, writer, k);
  if (!fr || !f) return SZ_E_ARG;
  const FloeWriter& w = c->rec.floe[writer];
  const FrameLayout L(w.mask, fr->M, fr->N, fr->V);
  const ListLayout LL = rec_list_layout(w, *fr);
  return rec_frame_down(c, "sz_download_floe_frame", L, fr->M, fr->N, fr->V, w.arena + fr->at, f, &LL, fr->S);
}
int sz_floe_frame_lists_info(sz_ctx* c, int32_t writer, int32_t k, int64_t* n_inter_rows, int64_t* n_sub_points) {
  const FloeFrame* f = rec_floe_frame(c, writer, k);
  if (!f) return SZ_E_ARG;
  if (n_inter_rows) *n_inter_rows = f->R;
  if (n_sub_points) *n_sub_points = f->S;
  return SZ_OK;
}
int sz_download_floe_frame_interactions(sz_ctx* c, int32_t writer, int32_t k, int32_t* off, double* rows) {
  const FloeFrame* fr = rec_floe_frame(c, writer, k);
  if (!fr || !off) return SZ_E_ARG;
  if (!(fr->lists & FR_LIST_INTER)) { c->err = "sz_download_floe_frame_interactions: this frame did not record the interactions (sz_set_floe_output_lists)"; return SZ_E_ARG; }
  const FloeWriter& w = c->rec.floe[writer];
  const ListLayout LL = rec_list_layout(w, *fr);
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(off, w.arena + fr->at + LL.off[FL_IOFF], (size_t)(fr->M + 1) * sizeof(int), hipMemcpyDeviceToHost));
  if (rows && fr->R > 0) HIPCHK(c, hipMemcpy(rows, w.arena + fr->at + LL.off[FL_IROWS], (size_t)fr->R * 7 * sizeof(double), hipMemcpyDeviceToHost));
  return SZ_OK;
}
int sz_download_grid_frame(sz_ctx* c, int32_t writer, int32_t k, int32_t* tstep, double* data) {
  if (!c) return SZ_E_ARG;
  if (writer < 0 || writer >= REC_WRITERS || k < 0 || k >= (int)c->rec.grid[writer].tsteps.size()) { c->err = "no such grid frame (sz_output_frames)"; return SZ_E_ARG; }
  const GridWriter& g = c->rec.grid[writer];
  const size_t n = g.outputs.size() * g.nx * g.ny;
  if (tstep) *tstep = g.tsteps[k];
  if (!data) return SZ_OK;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(data, g.store + (size_t)k * n, n * sizeof(double), hipMemcpyDeviceToHost));
  return SZ_OK;
}
int sz_clear_frames(sz_ctx* c) {
  if (!c) return SZ_E_ARG;
  for (int w = 0; w < REC_WRITERS; w++) { c->rec.floe[w].frames.clear(); c->rec.floe[w].used = 0; c->rec.grid[w].tsteps.clear(); }
  c->rec.full = false;
  return SZ_OK;
}

}  // extern "C"
// ---------------------------------------------------------------- output recorder on tiled contexts (sz_record_tile.hpp; DESIGN.md §9i, "Tiled contexts")
// Host code of the tiled recorder, here and not in sz_tile_host.hpp because it is built from the helpers above (the workspace chunks, eul_*,
// rec_frame_down); TileStops::record and sz_tile_run reach tile_record / tile_rec_agree_settings through the declarations there.
namespace {
constexpr int REC_BIT_FULL = 1 << 30;          // beside the device error bits in the word of the record point's gather
// k ints of every rank on every rank, rank-major (k <= 8; the count-matrix area of d_gather, as comm_sizes borrows it between box gathers)
int tile_gather_ints(sz_ctx* c, const int* local, int k, int* all) {
  const int n = c->comm_n;
  if (n == 1) { memcpy(all, local, (size_t)k * sizeof(int)); return SZ_OK; }
  int *d_row = (int*)(c->d_gather + Gather::MAT), *d_all = d_row + Gather::RANKS;
  HIPCHK(c, hipMemcpyAsync(d_row, local, (size_t)k * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (const int rc = comm_allgather(c, d_row, d_all, (size_t)k, NCCL_INT32, sizeof(int))) return rc;
  HIPCHK(c, hipMemcpyAsync(all, d_all, (size_t)k * n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
static_assert(2 * REC_WRITERS <= 8 && Gather::RANKS + 8 * Gather::RANKS <= Gather::RANKS * Gather::RANKS, "tile_gather_ints would leave the count-matrix area");
// FNV-1a over what a writer was set with
struct Digest {
  unsigned h = 2166136261u;
  void add(const void* p, size_t n) { for (size_t k = 0; k < n; k++) { h ^= ((const unsigned char*)p)[k]; h *= 16777619u; } }
  template <class T> void val(const T& v) { add(&v, sizeof(T)); }
};
}  // namespace
// The first act of a tiled batch with writers set, before any other collective: one gather of a digest of every writer's settings (interval, mask, lists;
// interval, grid lines, output codes, max_frames).  Ranks that were set differently would cut their batches differently and wait for each other
// in different collectives: every rank returns SZ_E_STATE instead, naming the first writer that differs.
static int tile_rec_agree_settings(sz_ctx* c) {
  const Recorder& R = c->rec;
  int mine[2 * REC_WRITERS], all[2 * REC_WRITERS * Gather::RANKS];
  for (int w = 0; w < REC_WRITERS; w++) {
    Digest f, g;
    f.val(R.floe[w].dt); f.val(R.floe[w].mask); f.val(R.floe[w].tile); f.val(R.floe[w].lists);
    const GridWriter& G = R.grid[w];
    g.val(G.dt); g.val(G.nx); g.val(G.ny); g.val(G.max_frames); g.val(G.tile);
    g.add(G.xg.data(), G.xg.size() * sizeof(double)); g.add(G.yg.data(), G.yg.size() * sizeof(double)); g.add(G.outputs.data(), G.outputs.size() * sizeof(int));
    mine[w] = (int)f.h; mine[REC_WRITERS + w] = (int)g.h;
  }
  if (const int rc = tile_gather_ints(c, mine, 2 * REC_WRITERS, all)) return rc;
  for (int w = 0; w < 2 * REC_WRITERS; w++)
    for (int r = 1; r < c->comm_n; r++)
      if (all[2 * REC_WRITERS * r + w] != all[w]) {
        c->err = std::string("sz_tile_run: ") + (w < REC_WRITERS ? "floe" : "grid") + " output writer " + std::to_string(w % REC_WRITERS) + " is set differently on rank " + std::to_string(r) +
                 " than on rank 0 (sz_tile_set_floe_output / sz_tile_set_grid_output are to be called alike on every rank): no step was run";
        return SZ_E_STATE;
      }
  return SZ_OK;
}
namespace {
// one tile frame: the single frame's launch with the key slice behind it
int tile_rec_pack(sz_ctx* c, FloeWriter& w, int tstep, int V, const std::vector<int>& ranks, long long n_global) {
  const int M = c->hostM, N = c->hostN;
  const TileFrameLayout L(w.mask, M, N, V);
  FramePack F;
  const ColTable<double*> src = state_columns(c->S);
  for (int k = 0; k < MIG_NTAB; k++) F.col[k] = src.p[k];
  for (int k = 0; k < FR_NSEC; k++) F.off[k] = L.off[k];
  F.dst = w.arena + w.used; F.tstep = tstep; F.M = M; F.N = N; F.V = V;
  F.key_off = L.key; F.spare[0] = n_global; F.spare[1] = c->comm_rank; F.spare[2] = c->comm_n;
  const long long widest = std::max<long long>(4ll * M, V);
  hipLaunchKernelGGL(sz_k_frame_pack<true>, dim3(grid_for(widest, FP_TPB, 256), FP_SLICES + 1), dim3(FP_TPB), 0, c->stream, c->S, F);
  w.frames.push_back({ w.used, tstep, M, N, V, ranks });
  w.used += (size_t)L.total;
  return SZ_OK;
}
// The lists of a tile frame (sz_tile_set_floe_output_lists).  The order keys of the last step's rows behind the owned parents -- its halo floes,
// their ghosts and the owned floes' ghosts, as the inline tile steps leave them in S.gkeys -- sorted into the recorder's workspace: what the
// merge translates ghost partners with.  Called BEFORE sz_add_ghosts, as rec_list_keys is.  *nkeys == 0: nothing to translate.
int tile_rec_list_keys(sz_ctx* c, int* nkeys) {
  *nkeys = 0;
  if (c->tile_inter_state != TILE_INTER_TABLE) return SZ_OK;
  ListWork W;
  if (int rc = rec_list_work(c, W)) return rc;
  const int G = c->tile_keys_n;
  if (G <= 0 || G > c->S.capM) return SZ_OK;
  const long long* src = c->S.gkeys + (size_t)c->tile_keys_slot * c->S.capM;
  size_t tb = 0;
  HIPCHK(c, rocprim::radix_sort_keys(nullptr, tb, src, W.keys, (size_t)G, 0, 64, c->stream));
  if (tb > W.tmp_bytes) { c->err = "the recorder's key sort needs more scratch than its workspace holds"; return SZ_E_STATE; }
  HIPCHK(c, rocprim::radix_sort_keys(W.tmp, tb, src, W.keys, (size_t)G, 0, 64, c->stream));
  *nkeys = G;
  return SZ_OK;
}
// the list sections of the tile frame tile_rec_pack has just appended to w: the key table copied, one launch of the single frame's list kernel
// with nothing translated.  lists: the writer's, without the interactions where some rank's rows were not the last step's (lost: why);
// lranks: {R, S, K} of every rank for the union of the due writers' lists
int tile_rec_pack_lists(sz_ctx* c, FloeWriter& w, unsigned lists, int nkeys, const std::vector<int>& lranks, int lost) {
  ListWork W;
  if (int rc = rec_list_work(c, W)) return rc;
  FloeFrame& fr = w.frames.back();
  const bool in = lists & FR_LIST_INTER, sub = lists & FR_LIST_SUB;
  const int me = c->comm_rank;
  fr.lists = lists; fr.inter_lost = (w.lists & FR_LIST_INTER) ? lost : 0;
  fr.lranks = lranks;
  for (size_t r = 0; r < fr.lranks.size() / 3; r++) { if (!in) fr.lranks[3 * r] = fr.lranks[3 * r + 2] = 0; if (!sub) fr.lranks[3 * r + 1] = 0; }
  fr.R = fr.lranks[3 * me]; fr.S = fr.lranks[3 * me + 1]; fr.K = in ? nkeys : 0;
  const TileListLayout L(w.mask, lists, fr.M, fr.N, fr.V, fr.R, fr.S, fr.K);
  char* dst = w.arena + fr.at;
  if (fr.K > 0) HIPCHK(c, hipMemcpyAsync(dst + L.lkey, W.keys, (size_t)fr.K * sizeof(long long), hipMemcpyDeviceToDevice, c->stream));
  if (lists) {
    FrameLists F;
    for (int k = 0; k < FL_NSEC; k++) F.off[k] = L.off[k];
    F.dst = dst; F.ioff = W.ioff; F.soff = W.soff; F.keys = nullptr; F.nkeys = 0; F.M = fr.M; F.N = fr.N; F.lists = lists; F.R = fr.R; F.S = fr.S; F.keep_spare = 1;
    const long long widest = std::max<long long>(std::max<long long>(7 * fr.R, fr.S), fr.M + 1);
    hipLaunchKernelGGL(sz_k_frame_lists, dim3(grid_for(widest, FP_TPB, 256), 2), dim3(FP_TPB), 0, c->stream, c->S, F);
  }
  w.used = fr.at + (size_t)L.total;
  return SZ_OK;
}
}  // namespace
// write_data! of output step tstep on a tiled context, collectively (TileStops::record): halo rows and ghosts dropped, sz_add_ghosts -- the
// ghosts of the owned parents, which depend on each parent alone --, the counters, ONE gather of {error / full bits, M, N, V} per rank (with lists due also
// {R, S, key-table entries, rows-lost}: the key table is sorted in front of sz_add_ghosts, the counts and scans of the lists run behind it; an error
// or a full writer of one rank is every rank's; the counts stay with the frame: the merge needs no collective to size its slots), one keyed
// pack launch per due floe writer; per due grid writer this rank's per-cell sums into one buffer, ONE all-reduce over it, the averages, the
// selected outputs into the store; sz_remove_ghosts.  A failure of the runtime itself (SZ_E_HIP) is returned alone, as everywhere on tiles.
static int tile_record(sz_ctx* c, int tstep, int* full) {
  Recorder& R = c->rec;
  *full = 0;
  bool fdue[REC_WRITERS], gdue[REC_WRITERS], any = false, any_grid = false;
  for (int w = 0; w < REC_WRITERS; w++) {
    fdue[w] = step_due(R.floe[w].dt, tstep); gdue[w] = step_due(R.grid[w].dt, tstep);
    any = any || fdue[w] || gdue[w]; any_grid = any_grid || gdue[w];
  }
  if (!any) return SZ_OK;
  const int n = c->comm_n;
  (void)hipSetDevice(c->device);
  int h[C_COUNT] = { 0 };
  // the lists some due writer records (the same word on every rank: the settings were agreed).  A writer without lists adds no launch, no scan,
  // no synchronisation, and the gather carries its four words
  unsigned lists = 0;
  for (int w = 0; w < REC_WRITERS; w++) if (fdue[w]) lists |= R.floe[w].lists;
  int rc = SZ_OK, nkeys = 0, lost = 0;
  if (lists & FR_LIST_INTER) {
    lost = c->tile_inter_state == TILE_INTER_MIGRATED || c->tile_inter_state == TILE_INTER_LISTED ? c->tile_inter_state : 0;
    if (!lost && (rc = tile_rec_list_keys(c, &nkeys)) == SZ_E_HIP) return rc;
  }
  const char* const keys_in = R.list_work.p;
  tile_cleanup(c);
  if (!rc) rc = sz_add_ghosts(c);
  if (rc == SZ_E_HIP) return rc;
  if (!rc && lists && (rc = rec_list_scans(c, lost ? lists & ~FR_LIST_INTER : lists)) == SZ_E_HIP) return rc;
  if (!rc && nkeys > 0 && R.list_work.p != keys_in) {
    (void)sz_remove_ghosts(c);          // (the ghosts are in the list: an error return leaves the parents alone, as the other ways out do)
    c->err = "the recorder's workspace moved under the sorted ghost keys (sz_add_ghosts grew the list)"; rc = SZ_E_STATE;
  }
  const int err_bits = rc ? (c->last_err_bits ? c->last_err_bits & ~REC_BIT_FULL : 1) : 0;
  if (!rc && (rc = fetch_counters(c, h))) return rc;
  const int M = c->hostM, N = c->hostN, V = h[C_NV];
  const int nR = (lists & FR_LIST_INTER) && !lost ? h[C_SCRATCH0] : 0, nS = lists & FR_LIST_SUB ? h[C_SCRATCH1] : 0;
  auto frame_total = [&](const FloeWriter& fw) {
    if (!fw.lists) return (size_t)TileFrameLayout(fw.mask, M, N, V).total;
    return (size_t)TileListLayout(fw.mask, lost ? fw.lists & ~FR_LIST_INTER : fw.lists, M, N, V, nR, nS, nkeys).total;
  };
  // (the local full size: where only a PEER's rows are lost the frame will be smaller than checked -- conservative; the migration and the
  //  drivers set the state alike on every rank, so in practice the ranks agree on `lost` before the gather says so)
  bool room = true;
  for (int w = 0; w < REC_WRITERS && !err_bits; w++) {
    if (fdue[w] && R.floe[w].used + frame_total(R.floe[w]) > R.floe[w].bytes) room = false;
    if (gdue[w] && (int)R.grid[w].tsteps.size() >= R.grid[w].max_frames) room = false;
  }
  const int nw = lists ? 8 : 4;
  const int mine[8] = { err_bits | (room ? 0 : REC_BIT_FULL), M, N, V, nR, nS, nkeys, lost };
  std::vector<int> all((size_t)nw * Gather::RANKS, 0), ranks((size_t)3 * n), lranks(lists ? (size_t)3 * n : 0, 0);          // (without lists: what was allocated before)
  if ((rc = tile_gather_ints(c, mine, nw, all.data()))) return rc;
  int bits = 0, who = -1; long long n_global = 0;
  for (int r = 0; r < n; r++) {
    if ((all[nw * r] & ~REC_BIT_FULL) && who < 0) who = r;
    bits |= all[nw * r];
    for (int q = 0; q < 3; q++) ranks[3 * r + q] = all[nw * r + 1 + q];
    n_global += all[nw * r + 2];
    if (lists) { for (int q = 0; q < 3; q++) lranks[3 * r + q] = all[nw * r + 4 + q]; if (!lost) lost = all[nw * r + 7]; }
  }
  // (rows that are not the last step's on one rank: no rank records the interactions of this frame -- the points stay)
  if (lost) { nkeys = 0; for (int r = 0; r < n; r++) lranks[3 * r] = lranks[3 * r + 2] = 0; }
  if (bits & ~REC_BIT_FULL) {
    if (!err_bits) {          // (else this rank's own message stands)
      (void)sz_remove_ghosts(c);
      c->err = "rank " + std::to_string(who) + " of the tiled run reported device error bits at an output step (this rank is clean; all ranks stop together)";
    }
    return SZ_E_CAPACITY;
  }
  c->err.clear();
  if (bits & REC_BIT_FULL) { *full = 1; R.full = true; return sz_remove_ghosts(c); }
  for (int w = 0; w < REC_WRITERS; w++) {
    if (!fdue[w]) continue;
    if ((rc = tile_rec_pack(c, R.floe[w], tstep, V, ranks, n_global))) return rc;
    if (R.floe[w].lists && (rc = tile_rec_pack_lists(c, R.floe[w], lost ? R.floe[w].lists & ~FR_LIST_INTER : R.floe[w].lists, nkeys, lranks, lost))) return rc;
  }
  if (any_grid) {
    size_t need_grid = 0, need_part = 0;
    for (int w = 0; w < REC_WRITERS; w++) if (gdue[w]) { need_grid += eul_grid_bytes(R.grid[w].nx, R.grid[w].ny); need_part += (size_t)EUL_PARTIAL * R.grid[w].nx * R.grid[w].ny * sizeof(double); }
    if ((rc = work_reserve(c, R.grid_work, need_grid)) || (rc = work_reserve(c, R.part_work, need_part))) return rc;
    // every due writer's grid arrays out of the one workspace chunk (they live until the averages are made), its sums behind the last writer's
    EulGrid E[REC_WRITERS]; double* part[REC_WRITERS] = { nullptr };
    Pool gp = work_pool(R.grid_work);
    size_t at = 0;
    for (int w = 0; w < REC_WRITERS && !rc; w++) {
      if (!gdue[w]) continue;
      const GridWriter& g = R.grid[w];
      int nent = 0; size_t need = 0;
      if ((rc = eul_grid(c, g.nx, g.ny, g.xg.data(), g.yg.data(), gp, E[w])) || (rc = eul_count(c, E[w], nent)) || (rc = eul_fill_bytes(c, E[w], nent, &need)) ||
          (rc = work_reserve(c, R.entry_work, need))) break;
      Pool ep = work_pool(R.entry_work);
      rc = eul_fill(c, ep, E[w], nent);
      work_keep(R.entry_work, ep);
      if (rc) break;
      const int ncell = g.nx * g.ny;
      part[w] = (double*)R.part_work.p + at; at += (size_t)EUL_PARTIAL * ncell;
      hipLaunchKernelGGL(sz_k_eul_partial, dim3(grid_for(ncell, 64)), dim3(64), 0, c->stream, c->S, E[w], nent, part[w]);
    }
    work_keep(R.grid_work, gp);
    if (rc) return rc;
    if ((rc = sz_comm_allreduce(c, R.part_work.p, (int64_t)at))) return rc;
    for (int w = 0; w < REC_WRITERS; w++) {
      if (!gdue[w]) continue;
      GridWriter& g = R.grid[w];
      const size_t ncell = (size_t)g.nx * g.ny, nout = g.outputs.size();
      hipLaunchKernelGGL(sz_k_eul_finish, dim3(grid_for((long long)ncell, 64)), dim3(64), 0, c->stream, E[w], (const double*)part[w]);
      double* dst = g.store + g.tsteps.size() * nout * ncell;
      for (size_t k = 0; k < nout; k++)
        HIPCHK(c, hipMemcpyAsync(dst + k * ncell, E[w].data + (size_t)g.outputs[k] * ncell, ncell * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
      g.tsteps.push_back(tstep);
    }
  }
  return sz_remove_ghosts(c);
}
extern "C" {
static const FloeFrame* tile_floe_frame(sz_ctx* c, int32_t writer, int32_t k, const char* who) {
  const FloeFrame* fr = rec_floe_frame(c, writer, k);
  if (fr && (!c->rec.floe[writer].tile || fr->ranks.empty())) { c->err = std::string(who) + ": not a frame of a tiled context's writer (sz_tile_set_floe_output)"; return nullptr; }
  return fr;
}
int sz_tile_floe_frame_keys(sz_ctx* c, int32_t writer, int32_t k, int64_t* keys) {
  const FloeFrame* fr = tile_floe_frame(c, writer, k, "sz_tile_floe_frame_keys");
  if (!fr || !keys) return SZ_E_ARG;
  const FloeWriter& w = c->rec.floe[writer];
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (fr->M > 0) HIPCHK(c, hipMemcpy(keys, w.arena + fr->at + TileFrameLayout(w.mask, fr->M, fr->N, fr->V).key, (size_t)fr->M * sizeof(long long), hipMemcpyDeviceToHost));
  return SZ_OK;
}
int sz_tile_floe_frame_info(sz_ctx* c, int32_t writer, int32_t k, int64_t* tstep, int64_t* M, int64_t* N, int64_t* n_ring_points, int64_t* n_ghost_links) {
  const FloeFrame* fr = tile_floe_frame(c, writer, k, "sz_tile_floe_frame_info");
  if (!fr) return SZ_E_ARG;
  long long tot[3] = { 0, 0, 0 };
  for (size_t r = 0; r < fr->ranks.size() / 3; r++) for (int q = 0; q < 3; q++) tot[q] += fr->ranks[3 * r + q];
  if (tstep) *tstep = fr->tstep;
  if (M) *M = tot[0];
  if (N) *N = tot[1];
  if (n_ring_points) *n_ring_points = tot[2];
  if (n_ghost_links) *n_ghost_links = tot[0] - tot[1];
  return SZ_OK;
}
// The merged frame (collective): what each rank prepares alone -- the frame, the members asked for, the scratch -- is agreed first, so that nobody
// is left in the gather; every rank's frame k in slots of the largest frame's size (known from the counts kept with the frame); the merge of
// sz_record_tile.hpp on the ranks that asked for the frame; one copy down.  inter: the call is sz_tile_download_floe_frame_interactions, and
// off / rows take the merged interactions instead of f the columns and points.  A rank that passes neither only takes part.
static int tile_frame_merged(sz_ctx* c, const char* who, int32_t writer, int32_t k, sz_floe_columns* f, bool inter, int32_t* off, double* rows) {
  if (!c) return SZ_E_ARG;
  if (int rc = tiled_ready(c, who)) return rc;
  (void)hipSetDevice(c->device);
  const int n = c->comm_n, me = c->comm_rank;
  const bool take = inter ? off != nullptr : f != nullptr;
  int rc = SZ_OK;
  const FloeFrame* fr = tile_floe_frame(c, writer, k, who);
  if (!fr) rc = SZ_E_ARG;
  else if ((int)fr->ranks.size() != 3 * n || (fr->lists && (int)fr->lranks.size() != 3 * n)) { c->err = std::string(who) + ": the frame was recorded by another number of ranks"; rc = SZ_E_STATE; }
  else if (inter && !(fr->lists & FR_LIST_INTER)) {
    if (fr->inter_lost == TILE_INTER_MIGRATED) { c->err = std::string(who) + ": this frame holds no interactions: it was recorded behind sz_tile_migrate, which drops the rows, before a collision step had made new ones"; rc = SZ_E_STATE; }
    else if (fr->inter_lost == TILE_INTER_LISTED) { c->err = std::string(who) + ": this frame holds no interactions: the step in front of it was a list-based tile step (sz_tile_step, a ridge / raft step), whose ghost keys are not kept"; rc = SZ_E_STATE; }
    else { c->err = std::string(who) + ": this frame did not record the interactions (sz_tile_set_floe_output_lists)"; rc = SZ_E_ARG; }
  }
  // ---- this rank alone: the layouts of all ranks' frames and of the merged one, the scratch
  const unsigned lists = fr && !rc ? fr->lists : 0;
  long long slot = 8, Mg = 0, Ng = 0, Vg = 0, Rg = 0, Sg = 0, Kt = 0;
  std::vector<long long> sec((size_t)n * RECT_NSEC, -1); std::vector<int> row0((size_t)n + 1, 0), npar((size_t)n, 0), lcnt((size_t)3 * n, 0), kbase((size_t)n + 1, 0);
  const unsigned long long mask = fr ? c->rec.floe[writer].mask : 1;
  if (!rc) {
    auto layout = [&](int r) { return TileListLayout(mask, lists, fr->ranks[3 * r], fr->ranks[3 * r + 1], fr->ranks[3 * r + 2], lists ? fr->lranks[3 * r] : 0, lists ? fr->lranks[3 * r + 1] : 0, lists ? fr->lranks[3 * r + 2] : 0); };
    // What travels: the whole frame -- or, for the interactions, only the part of it that call reads: the keys, the key table, inter_off and the
    // rows lie one behind the other in a tile frame (TileFrameLayout::key .. the end of ListLayout's FL_IROWS), in front of the points
    auto part = [&](int r, long long* from, long long* to) {
      const TileListLayout T = layout(r);
      *from = inter ? TileFrameLayout(mask, fr->ranks[3 * r], fr->ranks[3 * r + 1], fr->ranks[3 * r + 2]).key : 0;
      *to = inter ? T.off[FL_IROWS] + 56ll * std::max(fr->lranks[3 * r], 0) : T.total;
    };
    for (int r = 0; r < n; r++) { long long a, b; part(r, &a, &b); slot = std::max(slot, b - a); }
    for (int r = 0; r < n; r++) {
      const TileFrameLayout L(mask, fr->ranks[3 * r], fr->ranks[3 * r + 1], fr->ranks[3 * r + 2]);
      long long* t = &sec[(size_t)r * RECT_NSEC];
      long long from, to; part(r, &from, &to);
      auto at = [&](long long off) { return off < from || off >= to ? -1 : r * slot + off - from; };
      for (int s = 0; s < FR_NSEC; s++) t[s] = L.off[s] < 0 ? -1 : at(L.off[s]);
      t[RS_KEY] = at(L.key);
      if (lists) {
        const TileListLayout T = layout(r);
        t[RS_LKEY] = T.lkey < 0 ? -1 : at(T.lkey);
        for (int s = 0; s < FL_NSEC; s++) t[RS_LIST + s] = T.off[s] < 0 ? -1 : at(T.off[s]);
        for (int q = 0; q < 3; q++) lcnt[3 * r + q] = std::max(fr->lranks[3 * r + q], 0);
        Rg += lcnt[3 * r]; Sg += lcnt[3 * r + 1];
      }
      kbase[r] = (int)Kt; Kt += lcnt[3 * r + 2];
      row0[r] = (int)Mg; npar[r] = fr->ranks[3 * r + 1];
      Mg += fr->ranks[3 * r]; Ng += fr->ranks[3 * r + 1]; Vg += fr->ranks[3 * r + 2];
    }
    row0[n] = (int)Mg; kbase[n] = (int)Kt;
    if (Mg > 0x7fffffffll || Vg > 0x7fffffffll || 7 * Rg > 0x7fffffffll || Sg > 0x7fffffffll || Kt > 0x7fffffffll) { c->err = std::string(who) + ": the merged frame has more rows, ring points or list entries than an int holds"; rc = SZ_E_CAPACITY; }
    else if (fr->M != fr->ranks[3 * me] || fr->N != fr->ranks[3 * me + 1] || fr->V != fr->ranks[3 * me + 2]) { c->err = std::string(who) + ": the frame was recorded by another rank of the communicator"; rc = SZ_E_STATE; }
  }
  const FrameLayout Lg(mask, Mg, Ng, Vg);
  const ListLayout LLg(Lg.total, lists, Mg, Rg, Sg);
  if (!rc && f && !inter) rc = rec_frame_down(c, who, Lg, Mg, Ng, Vg, nullptr, f, &LLg, Sg);          // (the members asked for: checked before anybody gathers)
  Pool& P = c->rect_allocs;
  reset_pool(P);
  char *d_own = nullptr, *d_all = nullptr, *d_out = nullptr, *d_tmp = nullptr;
  long long *d_sec = nullptr, *key_in = nullptr, *key_out = nullptr, *kcat = nullptr, *ksort = nullptr;
  int *d_row0 = nullptr, *d_npar = nullptr, *val_in = nullptr, *src = nullptr, *pos = nullptr, *nv = nullptr, *ng = nullptr, *d_lcnt = nullptr, *d_kbase = nullptr, *ni = nullptr, *ns = nullptr,
      *kflag = nullptr, *drank = nullptr;
  size_t tmp_bytes = 0;
  const size_t Mc = (size_t)std::max<long long>(Mg, 1), Kc = (size_t)std::max<long long>(Kt, 1);
  if (!rc) (void)((rc = dalloc(c, &d_own, (size_t)slot, P)) || (rc = dalloc(c, &d_all, (size_t)slot * n, P)));
  if (!rc && take) {
    size_t b1 = 0, b2 = 0, b3 = 0;
    if (hipSuccess != rocprim::radix_sort_pairs(nullptr, b1, (const long long*)nullptr, (long long*)nullptr, (const int*)nullptr, (int*)nullptr, Mc, 0u, 43u, c->stream) ||
        hipSuccess != rocprim::exclusive_scan(nullptr, b2, (const int*)nullptr, (int*)nullptr, 0, std::max(Mc, lists ? Kc : 0) + 1, rocprim::plus<int>(), c->stream) ||
        (lists && hipSuccess != rocprim::radix_sort_keys(nullptr, b3, (const long long*)nullptr, (long long*)nullptr, Kc, 0u, 64u, c->stream))) { c->err = std::string(who) + ": rocprim would not size its scratch"; rc = SZ_E_HIP; }
    tmp_bytes = std::max(std::max(b1, b2), b3);
    if (!rc) (void)((rc = dalloc(c, &d_out, (size_t)LLg.total, P)) || (rc = dalloc(c, &d_tmp, tmp_bytes, P)) || (rc = dalloc(c, &d_sec, sec.size(), P)) || (rc = dalloc(c, &d_row0, row0.size(), P)) ||
                    (rc = dalloc(c, &d_npar, npar.size(), P)) || (rc = dalloc(c, &key_in, Mc, P)) || (rc = dalloc(c, &key_out, Mc, P)) || (rc = dalloc(c, &val_in, Mc, P)) ||
                    (rc = dalloc(c, &src, Mc, P)) || (rc = dalloc(c, &pos, Mc, P)) || (rc = dalloc(c, &nv, Mc + 1, P)) || (rc = dalloc(c, &ng, Mc + 1, P)));
    if (!rc && lists) (void)((rc = dalloc(c, &d_lcnt, lcnt.size(), P)) || (rc = dalloc(c, &d_kbase, kbase.size(), P)) || (rc = dalloc(c, &ni, Mc + 1, P)) || (rc = dalloc(c, &ns, Mc + 1, P)) ||
                             (rc = dalloc(c, &kcat, Kc, P)) || (rc = dalloc(c, &ksort, Kc, P)) || (rc = dalloc(c, &kflag, Kc + 1, P)) || (rc = dalloc(c, &drank, Kc + 1, P)));
  }
  // ---- the agreement on what each prepared alone, then the gather
  int first = 0;
  if (const int rc2 = comm_agree_rc(c, who, rc, &first)) return rc2;
  if (first) return rc ? rc : first;
  const FloeWriter& w = c->rec.floe[writer];
  const TileListLayout Tm(mask, lists, fr->M, fr->N, fr->V, fr->R, fr->S, fr->K);
  const long long mine_from = inter ? TileFrameLayout(mask, fr->M, fr->N, fr->V).key : 0, mine_to = inter ? Tm.off[FL_IROWS] + 56ll * fr->R : Tm.total;
  if (mine_to > mine_from) HIPCHK(c, hipMemcpyAsync(d_own, w.arena + fr->at + mine_from, (size_t)(mine_to - mine_from), hipMemcpyDeviceToDevice, c->stream));
  if ((rc = comm_allgather(c, d_own, d_all, (size_t)slot / 8, NCCL_FLOAT64, sizeof(double)))) return rc;
  if (!take) return SZ_OK;
  // ---- the merge
  HIPCHK(c, hipMemcpyAsync(d_sec, sec.data(), sec.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_row0, row0.data(), row0.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_npar, npar.data(), npar.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  RectArgs A{};
  A.all = d_all; A.sec = d_sec; A.row0 = d_row0; A.npar = d_npar; A.src = src; A.pos = pos; A.nv = nv; A.ng = ng; A.out = d_out;
  for (int s = 0; s < FR_NSEC; s++) A.off[s] = Lg.off[s];
  A.nranks = n; A.Mg = (int)Mg; A.Ng = (int)Ng; A.Vg = (int)Vg; A.tstep = fr->tstep;
  const int nb = grid_for(Mg + 1, RECT_TPB, 2048);
  if (Mg > 0) {
    hipLaunchKernelGGL(sz_k_rect_keys, dim3(nb), dim3(RECT_TPB), 0, c->stream, A, key_in, val_in);
    HIPCHK(c, rocprim::radix_sort_pairs((void*)d_tmp, tmp_bytes, (const long long*)key_in, key_out, (const int*)val_in, src, (size_t)Mg, 0u, 43u, c->stream));
  }
  // (a call moves what it returns: the interactions call neither the columns nor the points, the column call neither the key tables nor the rows)
  if (!inter) hipLaunchKernelGGL(sz_k_rect_counts, dim3(nb), dim3(RECT_TPB), 0, c->stream, A);
  if (!inter && Lg.off[FR_VOFF] >= 0) HIPCHK(c, rocprim::exclusive_scan((void*)d_tmp, tmp_bytes, (const int*)nv, (int*)(d_out + Lg.off[FR_VOFF]), 0, (size_t)Mg + 1, rocprim::plus<int>(), c->stream));
  if (!inter && Lg.off[FR_GOFF] >= 0) HIPCHK(c, rocprim::exclusive_scan((void*)d_tmp, tmp_bytes, (const int*)ng, (int*)(d_out + Lg.off[FR_GOFF]), 0, (size_t)Mg + 1, rocprim::plus<int>(), c->stream));
  if (!inter) hipLaunchKernelGGL(sz_k_rect_scatter, dim3(grid_for(std::max<long long>(4 * Mg, Vg), RECT_TPB, 256), FP_SLICES), dim3(RECT_TPB), 0, c->stream, A);
  const bool want_in = inter && (lists & FR_LIST_INTER), want_sub = !inter && (lists & FR_LIST_SUB) && f && (f->sub_off || f->sx || f->sy);
  if (want_in || want_sub) {
    HIPCHK(c, hipMemcpyAsync(d_lcnt, lcnt.data(), lcnt.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_kbase, kbase.data(), kbase.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    A.lists = lists; A.lcnt = d_lcnt; A.kbase = d_kbase; A.ni = ni; A.ns = ns; A.dkeys = ksort; A.drank = drank;
    for (int s = 0; s < FL_NSEC; s++) A.loff[s] = LLg.off[s];
    if (!want_in) A.loff[FL_IOFF] = A.loff[FL_IROWS] = -1;
    if (!want_sub) A.loff[FL_SOFF] = A.loff[FL_SX] = A.loff[FL_SY] = -1;
    A.Kt = want_in ? (int)Kt : 0; A.Rg = (int)Rg; A.Sg = (int)Sg; A.list0 = want_in ? 0 : 1;
    if (A.Kt > 0) {
      hipLaunchKernelGGL(sz_k_rect_lkeys, dim3(grid_for(Kt, RECT_TPB, 2048)), dim3(RECT_TPB), 0, c->stream, A, kcat);
      HIPCHK(c, rocprim::radix_sort_keys((void*)d_tmp, tmp_bytes, (const long long*)kcat, ksort, (size_t)Kt, 0u, 64u, c->stream));
      hipLaunchKernelGGL(sz_k_rect_kflags, dim3(grid_for(Kt + 1, RECT_TPB, 2048)), dim3(RECT_TPB), 0, c->stream, (const long long*)ksort, kflag, (int)Kt);
      HIPCHK(c, rocprim::exclusive_scan((void*)d_tmp, tmp_bytes, (const int*)kflag, drank, 0, (size_t)Kt + 1, rocprim::plus<int>(), c->stream));
    }
    hipLaunchKernelGGL(sz_k_rect_list_counts, dim3(nb), dim3(RECT_TPB), 0, c->stream, A);
    if (want_in) HIPCHK(c, rocprim::exclusive_scan((void*)d_tmp, tmp_bytes, (const int*)ni, (int*)(d_out + LLg.off[FL_IOFF]), 0, (size_t)Mg + 1, rocprim::plus<int>(), c->stream));
    if (want_sub) HIPCHK(c, rocprim::exclusive_scan((void*)d_tmp, tmp_bytes, (const int*)ns, (int*)(d_out + LLg.off[FL_SOFF]), 0, (size_t)Mg + 1, rocprim::plus<int>(), c->stream));
    hipLaunchKernelGGL(sz_k_rect_lists, dim3(grid_for(want_in ? 7 * Rg : Sg, RECT_TPB, 256), 1), dim3(RECT_TPB), 0, c->stream, A);
  }
  if (!inter) rc = rec_frame_down(c, who, Lg, Mg, Ng, Vg, d_out, f, &LLg, Sg);
  else {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(off, d_out + LLg.off[FL_IOFF], (size_t)(Mg + 1) * sizeof(int), hipMemcpyDeviceToHost));
    if (rows && Rg > 0) HIPCHK(c, hipMemcpy(rows, d_out + LLg.off[FL_IROWS], (size_t)Rg * 7 * sizeof(double), hipMemcpyDeviceToHost));
  }
  trim_pool(P);
  return rc;
}
int sz_tile_download_floe_frame(sz_ctx* c, int32_t writer, int32_t k, sz_floe_columns* f) { return tile_frame_merged(c, "sz_tile_download_floe_frame", writer, k, f, false, nullptr, nullptr); }
int sz_tile_download_floe_frame_interactions(sz_ctx* c, int32_t writer, int32_t k, int32_t* off, double* rows) {
  return tile_frame_merged(c, "sz_tile_download_floe_frame_interactions", writer, k, nullptr, true, off, rows);
}
// the lists of the MERGED frame and their totals, from the counts kept with the frame (local)
int sz_tile_floe_frame_lists_info(sz_ctx* c, int32_t writer, int32_t k, uint32_t* lists, int64_t* n_inter_rows, int64_t* n_sub_points) {
  const FloeFrame* fr = tile_floe_frame(c, writer, k, "sz_tile_floe_frame_lists_info");
  if (!fr) return SZ_E_ARG;
  long long tot[2] = { 0, 0 };
  for (size_t r = 0; r < fr->lranks.size() / 3; r++) for (int q = 0; q < 2; q++) tot[q] += fr->lranks[3 * r + q];
  if (lists) *lists = fr->lists;
  if (n_inter_rows) *n_inter_rows = tot[0];
  if (n_sub_points) *n_sub_points = tot[1];
  return SZ_OK;
}
// the key table of tile frame k (local): *n its entries, keys (may be NULL) the sorted order keys of the last step's rows behind the owned parents
int sz_tile_floe_frame_list_keys(sz_ctx* c, int32_t writer, int32_t k, int64_t* n, int64_t* keys) {
  const FloeFrame* fr = tile_floe_frame(c, writer, k, "sz_tile_floe_frame_list_keys");
  if (!fr || !n) return SZ_E_ARG;
  *n = fr->K;
  if (!keys || fr->K <= 0) return SZ_OK;
  const FloeWriter& w = c->rec.floe[writer];
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(keys, w.arena + fr->at + TileListLayout(w.mask, fr->lists, fr->M, fr->N, fr->V, fr->R, fr->S, fr->K).lkey, (size_t)fr->K * sizeof(long long), hipMemcpyDeviceToHost));
  return SZ_OK;
}

// what simplify_floes! (simplification.jl:339-378) would find to do, without downloading a floe
int sz_simplify_check(sz_ctx* c, int32_t max_vertices, double min_floe_area, double min_floe_height, int64_t* out4) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (!out4) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  PoolGuard pool;
  unsigned long long* d = nullptr;
  int rc = dalloc(c, &d, 4, pool.v);
  if (rc) return rc;
  hipLaunchKernelGGL(sz_k_simplify_check, dim3(grid_for(c->S.capM, 256, 1024)), dim3(256), 0, c->stream, c->S, max_vertices,
                     min_floe_area, min_floe_height, d);
  unsigned long long h[4];
  HIPCHK(c, hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  rc = sync_and_check(c);
  if (rc) return rc;
  for (int k = 0; k < 4; k++) out4[k] = (int64_t)h[k];
  return SZ_OK;
}

// waits for everything enqueued so far and reports sticky device errors
int sz_sync(sz_ctx* c) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  int h[C_COUNT];
  int rc = sync_and_check(c, h);
  if (rc) return rc;
  c->fuse_lists.resize(c->hostM);
  return SZ_OK;
}

// run on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream) instead of the
// library's own, so that collectives enqueued by the host framework order with the kernels
int sz_set_stream(sz_ctx* c, void* hip_stream) {
  if (!c) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->own_stream) { (void)hipStreamDestroy(c->stream); c->own_stream = false; }
  c->stream = (hipStream_t)hip_stream;
  return SZ_OK;
}

}  // extern "C"

// sz_tile_host.hpp — the host code of tiled (multi-GPU) contexts: set-up, the steps a host drives itself (sz_halo_* / sz_tile_step), the box
// gather and the halo exchange, migration, the collective removal, row edits by global number, the fracture, welding and ridge / raft passes, and the batch drivers of sz_tile_run.  Host code of
// the one translation unit sz_api.hip, which includes it behind the single context's batch drivers and passes: a tile's steps are theirs.
#pragma once
#include "sz_comm.hpp"

// ---------------------------------------------------------------- set-up, and the steps a host drives itself (multi-GPU halo API)
namespace {
// is this context ready for a collective tiled call?  (`who`: the entry point, for the message)
int tiled_ready(sz_ctx* c, const char* who) {
  if (c->have_floes && c->S.tiled && c->comm_n >= 1 && c->tile_margin > 0) return SZ_OK;
  c->err = std::string(who) + " needs sz_tile_enable and sz_tile_setup after the last sz_upload_floes";
  return SZ_E_STATE;
}
// The pack launch (sz_k_halo_pack): the owned floes that reach into a peer's expanded box, as records in that peer's region of `send` (`cap`
// slots each, at most dcap[d] used; record 0 = header with the count), the counts per destination behind the counter block; ref / margin: the
// drift check against the positions of the last box gather.  A null `send` only counts.  The tiling is the caller's: the context's own
// (tile_geo) or the arguments of a host that drives its steps itself.
struct TileGeo { int nranks, me; double Lx, Ly; int per_x, per_y; };
TileGeo tile_geo(const sz_ctx* c) { return { c->comm_n, c->comm_rank, c->tile_Lx, c->tile_Ly, c->tile_per_x, c->tile_per_y }; }
void halo_pack(sz_ctx* c, const TileGeo& g, double* send, int cap, const int* dcap, const double* ref, double margin) {
  State& S = c->S;
  hipLaunchKernelGGL(sz_k_halo_pack, dim3(grid_for(std::max(c->hostN, 1), PACK_TPB)), dim3(PACK_TPB), 0, c->stream, S, g.nranks, g.me, S.bounds + 16, g.Lx, g.Ly,
                     g.per_x, g.per_y, send, cap, S.cnt + C_COUNT, dcap, ref, margin);      // (the counts: 64 ints reserved behind the counter block)
}
int tile_forcing(sz_ctx* c) {
  if (!c->have_fields) { c->err = "sz_set_fields must be called before coupling"; return SZ_E_STATE; }
  if (c->two_way) { int rc = ensure_two_way(c); if (rc) return rc; }
  else if (c->precision == 1) { int rc = ensure_mixed(c); if (rc) return rc; }
  else { int rc = ensure_block_points(c); if (rc) return rc; }
  stage_forcing(c);
  return SZ_OK;
}

// one list-based tiled step: the body of the public sz_tile_step below, and the step of sz_tile_run's list-based driver (tile_run_listed), which
// has checked the context and evaluates a criterion itself, between its segments.
// halves: TILE_STEP_WHOLE is the step as it always was.  A ridge / raft step of sz_tile_run is split where timestep_ridging_rafting! stands
// (simulation.jl:121-136): TILE_STEP_FIRST = unpack, ghosts, collisions -- the list then holds the owned floes, the halo floes and the ghosts of
// both, with this step's floe.interactions -- and TILE_STEP_SECOND = the forcings of a coupling step (behind the host's possible edits, as
// timestep_coupling! comes after the ridging) and the integrator.  Nothing between the halves changes what the second reads, and both set the
// modes their kernels are told, so anything may run between them.
enum { TILE_STEP_FIRST = 1, TILE_STEP_SECOND = 2, TILE_STEP_WHOLE = 3 };
static int tile_step_body(sz_ctx* c, const void* d_recv, int32_t nranks, int32_t cap, int32_t tstep, int32_t dt, int32_t coupling_dt, int32_t flags, int halves = TILE_STEP_WHOLE) {
  (void)hipSetDevice(c->device);
  State& S = c->S;
  const bool first = (halves & TILE_STEP_FIRST) != 0, second = (halves & TILE_STEP_SECOND) != 0, whole = first && second;
  const bool coll = (flags & SZ_COLLISIONS_ON) != 0;
  const bool sg = coll && c->grid_ok;
  if (sg && first) use_static_grid(c);
  const bool gl = whole ? ghost_list_wanted(c, sg) : first ? (c->tile_split_gl = ghost_list_wanted(c, sg)) : c->tile_split_gl;
  if (first) { if (gl) use_ghost_list(c); else c->gl_valid = false; }
  if (first && d_recv && nranks > 0) {
    // halo floes join the candidate list of THIS step (the owned floes were appended by the last integrator)
    hipLaunchKernelGGL(sz_k_halo_unpack, dim3(1), dim3(1024), 0, c->stream, S, (const double*)d_recv, nranks, cap, sg ? 1 : 0, gl ? c->gl_cur : -1);
  }
  const bool coupling = coupling_at(flags, coupling_dt, tstep);
  const bool periodic = S.any_periodic_ew || S.any_periodic_ns;
  // the forcings of this step: already enqueued by sz_tile_forcing (beside the exchange), else now -- in either
  // case before the ghost pass, like sz_step (a split step: in its second half)
  if (whole || second) {
    if (coupling && c->tile_forcing_tstep != tstep) { int rc = tile_forcing(c); if (rc) return rc; }
    c->tile_forcing_tstep = -1;
  }
  // As in sz_step, the ghosts of the previous step are detached by this step's flag kernel and the new ones
  // committed by the flag/scan kernel; the halo of the previous step was overwritten by the unpack kernel.  Nothing
  // between two steps looks past the owned floes, so no clean-up launch is needed per step: the ghosts and halo
  // floes of the LAST step are dropped when the host next looks at the state (tile_cleanup).
  // n_init = every local parent (owned + halo): totals of halo floes are computed and then ignored
  if (first) S.callid = ++c->callid;
  // (fixed-point totals as in the resident steps of sz_step, so that a tile and the single context give the same bits; the reduce launch stays
  //  inside the step here, assembling rows only)
  const bool facc_on = coll && c->facc_buf != nullptr;
  S.facc = facc_on ? c->facc_buf : nullptr; S.kexp = force_scale_exp(c); c->reduce_mode = facc_on ? 1 : 0; c->acc_mode = facc_on ? 1 : 0;
  if (first && coll) c->tile_inter_state = TILE_INTER_LISTED;          // (the rows name this step's ghosts by order key, and no table of them is kept)
  if (first && coll) stage_ghosts(c, true, sg, gl);
  if (first && coll) collisions(c, -1, dt, periodic && !sg, sg);
  if (second) {
    stage_integrate(c, dt, false, coupling, sg, gl ? 1 - c->gl_cur : -1);
    if (gl) { c->gl_cur ^= 1; c->gl_est = std::max(c->gl_est, 64); }
    c->tile_dirty = true;
  }
  S.facc = nullptr; c->reduce_mode = 0; c->acc_mode = 0;
  return SZ_OK;
}
}  // namespace

int sz_tile_enable(sz_ctx* c, const int64_t* gidx, double halo_capacity_factor, double max_rmax) {
  if (!c || !c->have_floes || !gidx) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  leave_resident(c);
  State& S = c->S;
  if (c->hostM != c->hostN) { c->err = "sz_tile_enable needs a ghost-free upload"; return SZ_E_STATE; }
  if (c->rec.any_single) { c->err = "sz_tile_enable: an output writer of a single context is set (sz_set_floe_output / sz_set_grid_output with dt_out = 0 turn it off; a tiled context takes sz_tile_set_floe_output / sz_tile_set_grid_output)"; return SZ_E_STATE; }
  std::vector<long long>& ok = c->tile_gidx;
  ok.assign(c->hostN, 0);
  for (int i = 0; i < c->hostN; i++) ok[i] = gidx[i];
  H2D(S.okey, ok.data(), c->hostN, long long);
  if (c->facc_buf) HIPCHK(c, hipMemsetAsync(c->facc_buf, 0, (size_t)FX_WORDS * S.capM * sizeof(long long), c->stream));      // (rows change hands in a migration: no stale totals)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  S.tiled = 1;
  // largest ring among ALL ranks' floes (halo floes arrive unseen): decides which narrow variants can be needed
  c->max_ring_tiled = halo_capacity_factor > 0 ? (int)halo_capacity_factor : HALO_RING;
  // the halo records have room for the largest ring of ANY rank's floes (Floe rings are unbounded, floe.jl:24-77; the engine's narrow phase
  // takes 255 points, and so do the tiles): 12 + 2 * halo_ring doubles per record
  if (c->max_ring_tiled > NARROW_CAP2) { c->err = "a ring has more than 255 points: beyond the narrow phase's largest variant"; return SZ_E_CAPACITY; }
  S.halo_ring = std::max(HALO_RING, (std::max(c->max_ring_tiled, c->max_ring) + 3) & ~3);
  // largest rmax among ALL ranks' floes: the static broad-phase grid must hold for halo floes too (0: unknown ->
  // the grid is fitted to the centroids every step instead)
  c->rmax_hint = max_rmax; c->rmax_max = max_rmax > 0 ? c->rmax_max : 0.0;
  setup_grid(c);
  return SZ_OK;
}

int sz_owned_box(sz_ctx* c, double* out5) {
  if (!c || !c->have_floes || !out5) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  hipLaunchKernelGGL(sz_k_owned_box, dim3(1), dim3(1024), 0, c->stream, c->S, c->S.bounds + 8, (const double*)nullptr, 0.0, 0.0, 0, 0);
  HIPCHK(c, hipMemcpyAsync(out5, c->S.bounds + 8, 5 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}

int sz_halo_record_doubles(void) { return HALO_REC; }
int sz_halo_record_doubles_ctx(sz_ctx* c) { return c ? halo_rec(c->S) : HALO_REC; }

// boxes: nranks x {xmin, xmax, ymin, ymax}, already expanded by the interaction range (rarely changes)
int sz_halo_set_boxes(sz_ctx* c, int32_t nranks, const double* boxes) {
  if (!c || !c->have_floes || nranks < 1 || nranks > 64 || !boxes) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(c->S.bounds + 16, boxes, (size_t)nranks * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}

// asynchronous: fills d_send (nranks regions of (cap + 1) records, record 0 = header with the count)
int sz_halo_pack(sz_ctx* c, int32_t nranks, int32_t me, double Lx, double Ly, int32_t per_x, int32_t per_y, void* d_send,
                 int32_t cap) {
  if (!c || !c->have_floes || nranks < 1 || nranks > 64 || cap < 1) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  halo_pack(c, { nranks, me, Lx, Ly, per_x, per_y }, (double*)d_send, cap, nullptr, nullptr, 0.0);
  return SZ_OK;
}
// counts of the last sz_halo_pack per destination rank (synchronises); used to size the exchange buffers
int sz_halo_counts(sz_ctx* c, int32_t nranks, int32_t* counts_out) {
  if (!c || !c->have_floes || nranks < 1 || nranks > 64 || !counts_out) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  HIPCHK(c, hipMemcpyAsync(counts_out, c->S.cnt + C_COUNT, (size_t)nranks * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}

// asynchronous: unpack d_recv (same layout, region r = records from rank r) and run one timestep_sim!
// on owned + halo floes; only owned floes are integrated, the halo is dropped afterwards
int sz_tile_step(sz_ctx* c, const void* d_recv, int32_t nranks, int32_t cap, int32_t tstep, int32_t dt, int32_t coupling_dt,
                 int32_t flags) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  if (c->frac_kind != SZ_FRAC_OFF) { c->err = "sz_tile_step does not evaluate fracture criteria (the host drives its steps: no library channel to gather the mean height over): sz_tile_run, or sz_set_fracture(SZ_FRAC_OFF)"; return SZ_E_STATE; }
  if (!c->weld_dts.empty()) { c->err = "sz_tile_step does not compute welding overlaps (the host drives its steps: no library channel to gather the candidates over): sz_tile_run, or sz_set_welding(0)"; return SZ_E_STATE; }
  if (c->rr_on) { c->err = "sz_tile_step has no ridge / raft candidate pass (the host drives its steps: no library channel to gather the ghost keys and the entries over): sz_tile_run, or sz_set_ridgeraft(0)"; return SZ_E_STATE; }
  return tile_step_body(c, d_recv, nranks, cap, tstep, dt, coupling_dt, flags);
}

// Two-way coupling across tiles.  After a tiled coupling step: sz_two_way_partial writes this rank's per-cell sums
// (3 x (Nx+1)(Ny+1) doubles: stress numerators x / y, ice area) to a DEVICE buffer of the caller, the caller adds
// the buffers of all ranks up (all-reduce), sz_two_way_finish turns the sums into the ocean fields on every rank.
int sz_two_way_partial(sz_ctx* c, void* d_partial) {
  if (!c || !c->have_floes || !c->two_way || !d_partial) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  const int ncell = (int)c->tw_ncell;
  hipLaunchKernelGGL(sz_k_tw_partial, dim3(grid_for(ncell, 256)), dim3(256), 0, c->stream, c->S, ncell, (double*)d_partial);
  return SZ_OK;
}
int sz_two_way_finish(sz_ctx* c, const void* d_partial, int32_t dt) {
  if (!c || !c->have_floes || !c->two_way || !d_partial) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  const int ncell = (int)c->tw_ncell;
  hipLaunchKernelGGL(sz_k_tw_finish, dim3(grid_for(ncell, 256)), dim3(256), 0, c->stream, c->S, c->P, ncell, dt, (const double*)d_partial);
  return SZ_OK;
}

// ASYNC: the forcings of step `tstep` (owned floes only; they need nothing from the halo), to be enqueued between
// sz_halo_pack and the collective so that they run beside the exchange; sz_tile_step(tstep) then skips them
int sz_tile_forcing(sz_ctx* c, int32_t tstep, int32_t coupling_dt, int32_t flags) {
  if (!c || !c->have_floes) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  const bool coupling = coupling_at(flags, coupling_dt, tstep);
  if (!coupling) return SZ_OK;
  int rc = tile_forcing(c); if (rc) return rc;
  c->tile_forcing_tstep = tstep;
  return SZ_OK;
}

int sz_tile_setup(sz_ctx* c, double Lx, double Ly, int32_t per_x, int32_t per_y, double drift_margin, int32_t rebox_every) {
  if (!c || !c->have_floes || !c->S.tiled || c->comm_n < 1 || !(drift_margin > 0) || rebox_every == 0) {
    if (c) c->err = "sz_tile_setup needs sz_upload_floes, sz_tile_enable and sz_comm_init first, a positive drift margin and rebox interval";
    return SZ_E_STATE;
  }
  (void)hipSetDevice(c->device);
  c->tile_Lx = Lx; c->tile_Ly = Ly; c->tile_per_x = per_x; c->tile_per_y = per_y; c->tile_margin = drift_margin; c->tile_rebox_every = std::abs(rebox_every); c->tile_rebox_fixed = rebox_every < 0;
  c->tile_since_box = -1; c->halo_cap = 0; c->d_send = nullptr; c->tile_rebox_cur = rebox_every < 0 ? -rebox_every : std::min(rebox_every, 8);
  c->tile_box_valid = false;
  if (!c->d_gather) HIPCHK(c, hipMalloc((void**)&c->d_gather, Gather::TOTAL * sizeof(double)));          // (lives as long as the communicator)
  return SZ_OK;
}
// the centre of this rank's tile (optional, after sz_tile_setup): in a periodic direction the owned box of the FIRST gather then takes every
// centroid at its image nearest to it, as the later gathers do with the centre of the box before (sz_k_owned_box)
int sz_tile_set_center(sz_ctx* c, double x, double y) {
  if (!c || !c->S.tiled || c->tile_margin <= 0) { if (c) c->err = "sz_tile_set_center needs sz_tile_setup"; return SZ_E_STATE; }
  c->tile_box_ctr[0] = x; c->tile_box_ctr[1] = y; c->tile_box_valid = true;
  return SZ_OK;
}

// ---------------------------------------------------------------- agreement on errors, the box gather, the exchange of a step
namespace {
// the agreement on this rank's sync_and_check status rc
static int tile_agree(sz_ctx* c, int rc) {
  int all = 0;
  if (const int rc2 = comm_agree_bits(c, rc ? (c->last_err_bits ? c->last_err_bits : 1) : 0, &all)) return rc2;
  return all ? SZ_E_CAPACITY : SZ_OK;
}
// sync + sticky device errors of THIS rank + agreement: SZ_OK on every rank or the same error code on every rank
int tile_sync_agree(sz_ctx* c, int* cnt_out = nullptr) {
  const int rc = sync_and_check(c, cnt_out);
  return rc == SZ_E_HIP ? rc : tile_agree(c, rc);              // (the runtime itself failed: nothing to agree on)
}

// do the expanded box of rank d and the (margin-expanded) owned box of rank s meet, periodic images included?
bool tiles_adjacent(const double* owned_s, const double* expanded_d, double margin, double Lx, double Ly, int per_x, int per_y) {
  for (int kx = (per_x ? -1 : 0); kx <= (per_x ? 1 : 0); kx++)
    for (int ky = (per_y ? -1 : 0); ky <= (per_y ? 1 : 0); ky++) {
      const double x0 = owned_s[0] - margin + kx * Lx, x1 = owned_s[1] + margin + kx * Lx;
      const double y0 = owned_s[2] - margin + ky * Ly, y1 = owned_s[3] + margin + ky * Ly;
      if (!(x1 < expanded_d[0] || expanded_d[1] < x0 || y1 < expanded_d[2] || expanded_d[3] < y0)) return true;
    }
  return false;
}

// collective: owned boxes of all ranks -> expanded boxes on the device, neighbour relation, per-pair slot counts, buffers,
// reference positions of the drift check.  Synchronises (it runs once per rebox_every steps).
int tile_rebox(sz_ctx* c) {
  State& S = c->S;
  const int n = c->comm_n, me = c->comm_rank;
  int rc = tile_sync_agree(c); if (rc) return rc;
  // (every gather after the first: centroids at their periodic image nearest to the centre of the last box)
  double* d_ctr = c->d_gather + Gather::CTR;
  if (c->tile_box_valid) {
    const double ctr[2] = { c->tile_box_ctr[0], c->tile_box_ctr[1] };
    HIPCHK(c, hipMemcpyAsync(d_ctr, ctr, sizeof(ctr), hipMemcpyHostToDevice, c->stream));
  }
  hipLaunchKernelGGL(sz_k_owned_box, dim3(1), dim3(1024), 0, c->stream, S, c->d_gather + Gather::OWN, c->tile_box_valid ? (const double*)d_ctr : (const double*)nullptr,
                     c->tile_Lx, c->tile_Ly, c->tile_per_x, c->tile_per_y);
  constexpr int GB = Gather::GB;      // doubles per rank in the gather: box, rmax, drift, speed, (spare)
  std::vector<double> all((size_t)GB * n);
  if ((rc = comm_allgather(c, c->d_gather + Gather::OWN, c->d_gather + Gather::ALL, GB, NCCL_FLOAT64, sizeof(double)))) return rc;
  HIPCHK(c, hipMemcpyAsync(all.data(), c->d_gather + Gather::ALL, all.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tile_box_ctr[0] = 0.5 * (all[GB * me] + all[GB * me + 1]); c->tile_box_ctr[1] = 0.5 * (all[GB * me + 2] + all[GB * me + 3]); c->tile_box_valid = true;
  double rmax = 0.0, drift = 0.0, speed = 0.0;
  for (int r = 0; r < n; r++) { rmax = std::max(rmax, all[GB * r + 4]); drift = std::max(drift, all[GB * r + 5]); speed = std::max(speed, all[GB * r + 6]); }
  // the gather interval follows the floes (every rank computes the same number): at the faster of the measured displacement per step since
  // the last gather and the largest velocity component now, they may use 30 % of the margin before the next gather (half of it is the
  // error threshold); the interval at most doubles from one gather to the next, and a new setup starts with a short one -- floes that
  // start from rest are slower in their first steps than later
  {
    const double per_step = std::max(c->tile_since_box > 0 ? drift / c->tile_since_box : 0.0, speed * std::fabs((double)c->tile_dt));
    int want = per_step > 0.0 ? (int)std::max(1.0, std::min((double)c->tile_rebox_every, 0.3 * c->tile_margin / per_step)) : c->tile_rebox_every;
    if (c->tile_since_box > 0) want = std::min(want, 2 * c->tile_rebox_cur);
    else want = std::min(want, c->tile_rebox_cur);
    c->tile_rebox_cur = c->tile_rebox_fixed ? c->tile_rebox_every : std::max(1, want);
  }
  const double reach = 2.0 * rmax + c->tile_margin;
  std::vector<double> boxes((size_t)4 * n);
  for (int r = 0; r < n; r++) { boxes[4 * r] = all[GB * r] - reach; boxes[4 * r + 1] = all[GB * r + 1] + reach; boxes[4 * r + 2] = all[GB * r + 2] - reach; boxes[4 * r + 3] = all[GB * r + 3] + reach; }
  HIPCHK(c, hipMemcpyAsync(S.bounds + 16, boxes.data(), boxes.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  // counting pass, then the count matrix of all ranks (row s: what s sends to every d)
  halo_pack(c, tile_geo(c), nullptr, 1, nullptr, nullptr, 0.0);
  int *dcnt = S.cnt + C_COUNT, *d_mat = (int*)(c->d_gather + Gather::MAT);
  std::vector<int> mat((size_t)n * n);
  if ((rc = comm_allgather(c, dcnt, d_mat, (size_t)n, NCCL_INT32, sizeof(int)))) return rc;
  HIPCHK(c, hipMemcpyAsync(mat.data(), d_mat, mat.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // slots per ordered pair: neighbours get 1.5 x the present count + 32, the others nothing (every rank computes the same table)
  c->cap_send.assign(n, 0); c->cap_recv.assign(n, 0);
  int cap = 32;
  for (int s = 0; s < n; s++)
    for (int d = 0; d < n; d++) {
      if (s == d) continue;
      const bool adj = tiles_adjacent(&all[GB * s], &boxes[4 * d], c->tile_margin, c->tile_Lx, c->tile_Ly, c->tile_per_x, c->tile_per_y);
      const int k = adj || mat[(size_t)s * n + d] > 0 ? mat[(size_t)s * n + d] * 3 / 2 + 32 : 0;
      if (s == me) c->cap_send[d] = k;
      if (d == me) c->cap_recv[s] = k;
      cap = std::max(cap, k);
    }
  if (cap > c->halo_cap || !c->d_send) {
    reset_pool(c->comm_allocs);          // (chunks that are large enough are carved again: a set-up after a migration allocates nothing)
    c->halo_cap = cap;
    const size_t nd = (size_t)n * (cap + 1) * halo_rec(c->S);
    if ((rc = dalloc(c, &c->d_send, nd, c->comm_allocs)) || (rc = dalloc(c, &c->d_recv, nd, c->comm_allocs)) ||
        (rc = dalloc(c, &c->d_ref, (size_t)2 * S.capM, c->comm_allocs)) || (rc = dalloc(c, &c->d_dcap, 64, c->comm_allocs))) return rc;
    trim_pool(c->comm_allocs);
  }
  // regions of ranks that send nothing keep a zero count in their header record
  HIPCHK(c, hipMemsetAsync(c->d_recv, 0, (size_t)n * (c->halo_cap + 1) * halo_rec(c->S) * sizeof(double), c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_dcap, c->cap_send.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_ref, S.cx, (size_t)c->hostN * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_ref + S.capM, S.cy, (size_t)c->hostN * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->tile_since_box = 0;
  return SZ_OK;
}
// a gather of the boxes is due: none since the set-up, or the interval in use has run out
bool rebox_due(const sz_ctx* c) { return c->tile_since_box < 0 || c->tile_since_box >= c->tile_rebox_cur; }
int rebox_if_due(sz_ctx* c) { return rebox_due(c) ? tile_rebox(c) : (int)SZ_OK; }

// The exchange of one step: the regions of d_send to the peers, theirs into d_recv, on the communication stream behind the pack kernel
// (ev_packed) -- ev_recv is recorded when the halo is in.  all_ranks: every rank gets at least the header record (the stop agreement of the
// inline steps reads the flags of ALL ranks); otherwise only the neighbouring tiles take part.
int tile_exchange(sz_ctx* c, bool all_ranks) {
  const int n = c->comm_n, me = c->comm_rank;
  if (n <= 1) return SZ_OK;
  const int HREC = halo_rec(c->S);
  const size_t stride = (size_t)(c->halo_cap + 1) * HREC;
  HIPCHK(c, hipEventRecord(c->ev_packed, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->comm_stream, c->ev_packed, 0));
  if (c->host_transport) {
    Timed tx(c, K_EXCHANGE, c->comm_stream);
    c->h_send.resize((size_t)n * stride); c->h_recv.resize((size_t)n * stride);
    HostTrade tr;
    for (int d = 0; d < n; d++) {
      if (d == me || (!all_ranks && c->cap_send[d] <= 0 && c->cap_recv[d] <= 0)) continue;
      const size_t ns = (all_ranks || c->cap_send[d] > 0) ? (size_t)(c->cap_send[d] + 1) * HREC : 0;
      const size_t nr = (all_ranks || c->cap_recv[d] > 0) ? (size_t)(c->cap_recv[d] + 1) * HREC : 0;
      if (ns) HIPCHK(c, hipMemcpyAsync(c->h_send.data() + d * stride, c->d_send + d * stride, ns * sizeof(double), hipMemcpyDeviceToHost, c->comm_stream));
      tr.add(d, c->h_send.data() + d * stride, ns * sizeof(double), c->h_recv.data() + d * stride, nr * sizeof(double));
    }
    HIPCHK(c, hipStreamSynchronize(c->comm_stream));
    if (int rc = tr.run(c)) return rc;
    for (size_t k = 0; k < tr.peer.size(); k++)
      if (tr.rb[k]) HIPCHK(c, hipMemcpyAsync(c->d_recv + tr.peer[k] * stride, tr.rp[k], (size_t)tr.rb[k], hipMemcpyHostToDevice, c->comm_stream));
    HIPCHK(c, hipStreamSynchronize(c->comm_stream));       // (h_recv is reused by the next step)
    tx.end();
  } else {
    Timed tx(c, K_EXCHANGE, c->comm_stream);          // (class "exchange" of sz_kernel_time_ms: the grouped send / receive on the communication stream)
    NCCLCHK(c, g_rccl.GroupStart());
    for (int d = 0; d < n; d++) {
      if (d == me) continue;
      if (all_ranks || c->cap_send[d] > 0) NCCLCHK(c, g_rccl.Send(c->d_send + d * stride, (size_t)(c->cap_send[d] + 1) * HREC, NCCL_FLOAT64, d, c->comm, c->comm_stream));
      if (all_ranks || c->cap_recv[d] > 0) NCCLCHK(c, g_rccl.Recv(c->d_recv + d * stride, (size_t)(c->cap_recv[d] + 1) * HREC, NCCL_FLOAT64, d, c->comm, c->comm_stream));
    }
    NCCLCHK(c, g_rccl.GroupEnd());
    tx.end();
  }
  HIPCHK(c, hipEventRecord(c->ev_recv, c->comm_stream));
  return SZ_OK;
}
// what a pack is given (sz_k_halo_pack; the integrator of a tiled step that packs for the next one: sz_k_integrate<true, true>)
PackInl tile_pack_args(sz_ctx* c) {
  State& S = c->S;
  PackInl a;
  a.send = c->d_send; a.boxes = S.bounds + 16; a.dcap = c->d_dcap; a.ref = c->d_ref; a.counts = S.cnt + C_COUNT;
  a.Lx = c->tile_Lx; a.Ly = c->tile_Ly; a.margin = c->tile_margin;
  a.nranks = c->comm_n; a.me = c->comm_rank; a.cap = c->halo_cap; a.per_x = c->tile_per_x; a.per_y = c->tile_per_y;
  return a;
}
void tile_pack(sz_ctx* c) { halo_pack(c, tile_geo(c), c->d_send, c->halo_cap, c->d_dcap, c->d_ref, c->tile_margin); }

// ---------------------------------------------------------------- migration
// Floes drift; ownership follows the tile that holds the centroid.  sz_tile_migrate re-assigns every owned floe (collective): the floes
// that changed tile travel with their COMPLETE state -- every column incl. the previous-step tendencies and the stress / strain tensors,
// status, ring, sub-floe points -- over the library's own channel (RCCL send / receive between device buffers, or the host's transport),
// and every rank's context is rebuilt from the floes it keeps and the ones it received, ordered by global index, through the same path an
// upload takes (capacities, neighbour counts, grid, ghost-candidate estimate are all re-derived).  The re-assignment is host-staged inside
// the library -- a rare operation (floes move metres per step against tiles of hundreds of km) whose cost is a download and an upload of
// the tile; the in-reference analogue is the parent / ghost swap of collisions.jl:942-950.  floe.interactions of the last collision call do
// not travel (the next step's collision call rebuilds them before anything reads them).
// The tiling of a context, taken before a migration replaces its field (the new field forgets it, as after any upload) and established again
// behind it with the same parameters: collective.  px > 0: the tiles are the px x py boxes of the domain, and the owned box of the first gather
// takes its centroids at the image nearest to this rank's box centre (sz_tile_set_center).
struct Retile {
  double Lx, Ly, margin, ring_hint, rmax_hint; int per_x, per_y, rebox, precision;
  explicit Retile(const sz_ctx* c) : Lx(c->tile_Lx), Ly(c->tile_Ly), margin(c->tile_margin), ring_hint((double)c->max_ring_tiled), rmax_hint(c->rmax_hint), per_x(c->tile_per_x),
                                     per_y(c->tile_per_y), rebox(c->tile_rebox_fixed ? -c->tile_rebox_every : c->tile_rebox_every), precision(c->precision) {}
  int again(sz_ctx* c, const long long* gidx, int px, int py) const {
    if (int rc = sz_tile_enable(c, (const int64_t*)gidx, ring_hint, rmax_hint)) return rc;
    if (int rc = sz_tile_setup(c, Lx, Ly, per_x, per_y, margin, rebox)) return rc;
    const double x0 = c->h_vals[3], y0 = c->h_vals[1], DLx = c->h_vals[2] - c->h_vals[3], DLy = c->h_vals[0] - c->h_vals[1];
    const int me = c->comm_rank;
    if (px > 0) (void)sz_tile_set_center(c, x0 + ((me % px) + 0.5) * DLx / px, y0 + ((me / px) + 0.5) * DLy / py);
    c->precision = precision;
    return SZ_OK;
  }
};
// sz_tile_migrate with the movers packed on the device (sz_migrate.hpp): owners, pack, exchange device to device, merge of the directories, the
// rows gathered into the new order, then what sz_upload_floes does behind its copies (counters, ring signs and boxes, cleared per-floe counts).
// The capacities the context was carved with stay; *fell_back = 1 (and nothing has changed) when some rank's new tile would crowd them --
// every rank then takes the host-staged path below, which carves anew.  The host reads the owner and offset columns (ints) and the merged
// directory; no floe column, ring or sub-floe point crosses to the host (a host transport stages the movers' streams).
int tile_migrate_device(sz_ctx* c, int px, int py, const int32_t* owner_override, int64_t* n_sent, int64_t* n_owned, int* fell_back) {
  State& S = c->S;
  const int n = c->comm_n, me = c->comm_rank, N = c->hostN;
  *fell_back = 0;
  int rc;
  if (c->gi_pending && c->gi_valid) { if ((rc = gi_fetch(c))) return rc; }
  c->gi_pending = false;
  struct Scratch { Pool& v; } pool{ c->mig_allocs };      // (the scratch of the last migration is carved again: no allocation in the common case)
  reset_pool(pool.v);
  // ---- owners, and how much goes where
  int *d_owner = nullptr, *d_override = nullptr, *d_bad = nullptr, *d_cntd = nullptr;
  unsigned long long *d_tally = nullptr, *d_cur = nullptr; long long *d_base = nullptr, *d_rbase = nullptr, *d_rsize = nullptr; double** d_cols = nullptr;
  if ((rc = dalloc(c, &d_owner, (size_t)N + 1, pool.v)) || (rc = dalloc(c, &d_tally, 128, pool.v)) || (rc = dalloc(c, &d_cur, 128, pool.v)) ||
      (rc = dalloc(c, &d_base, 64, pool.v)) || (rc = dalloc(c, &d_rbase, 64, pool.v)) || (rc = dalloc(c, &d_rsize, 64, pool.v)) ||
      (rc = dalloc(c, &d_cntd, 64, pool.v)) || (rc = dalloc(c, &d_bad, 1, pool.v)) || (rc = dalloc(c, &d_cols, MIG_TAB_CAP, pool.v))) return rc;
  if (owner_override) {
    if ((rc = dalloc(c, &d_override, (size_t)N + 1, pool.v))) return rc;
    if (N) HIPCHK(c, hipMemcpyAsync(d_override, owner_override, (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  const double x0 = c->h_vals[3], y0 = c->h_vals[1], Lx = c->h_vals[2] - c->h_vals[3], Ly = c->h_vals[0] - c->h_vals[1];
  hipLaunchKernelGGL(sz_k_mig_owner, dim3(grid_for(std::max(N, 1), 256)), dim3(256), 0, c->stream, S, N, (const int*)d_override, x0, y0, Lx, Ly, px, py,
                     c->tile_per_x, c->tile_per_y, me, n, d_owner, d_tally, d_bad);
  unsigned long long tally[128]; int bad = 0;
  std::vector<int> owner((size_t)N + 1), voff((size_t)N + 1), soff((size_t)N + 1);
  HIPCHK(c, hipMemcpyAsync(tally, d_tally, sizeof(tally), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (N) HIPCHK(c, hipMemcpyAsync(owner.data(), d_owner, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(voff.data(), S.voff, ((size_t)N + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(soff.data(), S.soff, ((size_t)N + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int any_bad = 0;
  if ((rc = comm_agree_bits(c, bad ? 1 : 0, &any_bad))) return rc;
  if (any_bad) { c->err = "sz_tile_migrate: owner out of range"; return SZ_E_ARG; }
  // ---- the movers' records, one stream per destination
  std::vector<int> mine(n, 0), all, cntd(64, 0); std::vector<long long> base(64, 0);
  size_t ts = 0; int nmove = 0; bool too_long = false;
  for (int d = 0; d < n; d++) {
    const unsigned long long cnt = tally[2 * d];
    if (d == me || !cnt) continue;
    const unsigned long long sz = 1 + (unsigned long long)MIG_DIR * cnt + tally[2 * d + 1];
    if (sz > 0x7fffffffull) { too_long = true; break; }
    mine[d] = (int)sz; base[d] = (long long)ts; ts += (size_t)sz; cntd[d] = (int)cnt; nmove += (int)cnt;
  }
  if (too_long) { for (int d = 0; d < n; d++) { mine[d] = 0; cntd[d] = 0; } ts = 0; }      // (says so in the agreement below; nothing is sent)
  double* d_sendb = nullptr;
  if ((rc = dalloc(c, &d_sendb, ts, pool.v))) return rc;
  const ColTable<double*> hcols = state_columns(S);
  HIPCHK(c, hipMemcpyAsync(d_cols, hcols.p, sizeof(hcols.p), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_base, base.data(), 64 * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_cntd, cntd.data(), 64 * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (ts) hipLaunchKernelGGL(sz_k_mig_pack, dim3(grid_for((long long)N * 64, 256, 2048)), dim3(256), 0, c->stream, S, N, (const int*)d_owner, me, d_sendb,
                             (const long long*)d_base, (const int*)d_cntd, d_cur, (double* const*)d_cols);
  // ---- sizes, then the streams: device to device (a host transport: staged, the movers only)
  if ((rc = comm_sizes(c, mine, all))) return rc;
  std::vector<long long> rbase(64, 0), rsize(64, 0);
  size_t tr = 0;
  for (int s2 = 0; s2 < n; s2++) { if (s2 == me) continue; rbase[s2] = (long long)tr; rsize[s2] = all[(size_t)s2 * n + me]; tr += (size_t)rsize[s2]; }
  double* d_recvb = nullptr;
  if ((rc = dalloc(c, &d_recvb, tr, pool.v))) return rc;
  if (n > 1 && c->host_transport) {
    std::vector<double> hs(std::max<size_t>(ts, 1)), hr(std::max<size_t>(tr, 1));
    if (ts) HIPCHK(c, hipMemcpyAsync(hs.data(), d_sendb, ts * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HostTrade trade;
    for (int d = 0; d < n; d++) if (d != me) trade.add(d, hs.data() + base[d], (size_t)mine[d] * sizeof(double), hr.data() + rbase[d], (size_t)rsize[d] * sizeof(double));
    if ((rc = trade.run(c))) return rc;
    if (tr) HIPCHK(c, hipMemcpyAsync(d_recvb, hr.data(), tr * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else if (n > 1) {
    NCCLCHK(c, g_rccl.GroupStart());
    for (int d = 0; d < n; d++) {
      if (d == me) continue;
      if (mine[d]) NCCLCHK(c, g_rccl.Send(d_sendb + base[d], (size_t)mine[d], NCCL_FLOAT64, d, c->comm, c->stream));
      if (rsize[d]) NCCLCHK(c, g_rccl.Recv(d_recvb + rbase[d], (size_t)rsize[d], NCCL_FLOAT64, d, c->comm, c->stream));
    }
    NCCLCHK(c, g_rccl.GroupEnd());
  }
  // ---- what arrived: the merged directory is all the host reads of it
  const int dcap = (int)(tr / (size_t)(MIG_DIR + MIG_NCOL)) + 1;
  double* d_dirs = nullptr;
  if ((rc = dalloc(c, &d_dirs, (size_t)MIG_DIR * (1 + (size_t)dcap), pool.v))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_rbase, rbase.data(), 64 * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_rsize, rsize.data(), 64 * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(sz_k_mig_dirs, dim3(1), dim3(256), 0, c->stream, (const double*)d_recvb, (const long long*)d_rbase, (const long long*)d_rsize, n, d_dirs, dcap);
  std::vector<double> dirs((size_t)MIG_DIR * (1 + (size_t)dcap));
  HIPCHK(c, hipMemcpyAsync(dirs.data(), d_dirs, dirs.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int R = (int)dirs[0];
  // ---- the new tile: kept floes + received ones, ordered by global index
  struct Src { long long g; int s; };
  std::vector<Src> src;
  for (int i = 0; i < N; i++) if (owner[i] == me) src.push_back({ c->tile_gidx[i], i });
  for (int e = 0; e < R; e++) src.push_back({ (long long)dirs[(size_t)MIG_DIR * (1 + e)], -(e + 1) });
  std::sort(src.begin(), src.end(), [](const Src& a, const Src& b2) { return a.g < b2.g; });
  const int Nn = (int)src.size();
  std::vector<int> hsrc((size_t)Nn + 1), nvoff((size_t)Nn + 1, 0), nsoff((size_t)Nn + 1, 0); std::vector<long long> ngid((size_t)Nn + 1);
  int ring_in = 0, sub_in = 0; double rmax_in = 0.0;
  for (int r = 0; r < Nn; r++) {
    const int s2 = src[r].s;
    int nv, ns;
    if (s2 >= 0) { nv = voff[s2 + 1] - voff[s2]; ns = soff[s2 + 1] - soff[s2]; }
    else {
      const double* e = dirs.data() + (size_t)MIG_DIR * (size_t)(-s2);
      nv = (int)e[1]; ns = (int)e[2]; ring_in = std::max(ring_in, nv); sub_in = std::max(sub_in, ns); rmax_in = std::max(rmax_in, e[4]);
    }
    hsrc[r] = s2; ngid[r] = src[r].g; nvoff[r + 1] = nvoff[r] + nv; nsoff[r + 1] = nsoff[r] + ns;
  }
  const int Vn = nvoff[Nn], NSn = nsoff[Nn];
  // does it fit what the context was carved for (sz_upload_floes: at least 2 M + 64 rows and 2 V + 4096 ring points, for the owned floes, their
  // ghosts and the halo)?  An eighth more than the upload held is let in.
  const bool fits = Nn <= c->upload_M + c->upload_M / 8 && Vn <= c->upload_V + c->upload_V / 8 && !too_long;
  int bits = (nmove > 0 ? 1 : 0) | (fits ? 0 : 2) | (Nn == 0 ? 4 : 0) | (R < 0 ? 8 : 0), allb = 0;
  if ((rc = comm_agree_bits(c, bits, &allb))) return rc;
  if (allb & 8) { c->err = "sz_tile_migrate: a stream of movers arrived inconsistent"; return SZ_E_STATE; }
  if (n_sent) *n_sent = nmove;
  if (!(allb & 1)) { c->err.clear(); if (n_owned) *n_owned = N; return SZ_OK; }
  if (allb & 4) { c->err = "sz_tile_migrate: a tile without floes (every rank must own at least one)"; return SZ_E_STATE; }
  if (allb & 2) { c->err.clear(); *fell_back = 1; return SZ_OK; }
  c->err.clear();
  // ---- the rows into their new order: gathered beside the old ones first (a row's source may lie on either side of it)
  int *d_src = nullptr, *d_nvoff = nullptr, *d_nsoff = nullptr; double *d_tmp = nullptr, *d_tsx = nullptr, *d_tsy = nullptr; double2* d_tv = nullptr;
  if ((rc = dalloc(c, &d_src, (size_t)Nn + 1, pool.v)) || (rc = dalloc(c, &d_nvoff, (size_t)Nn + 1, pool.v)) || (rc = dalloc(c, &d_nsoff, (size_t)Nn + 1, pool.v)) ||
      (rc = dalloc(c, &d_tmp, (size_t)MIG_NGATHER * Nn, pool.v)) || (rc = dalloc(c, &d_tv, (size_t)Vn, pool.v)) ||
      (rc = dalloc(c, &d_tsx, (size_t)NSn, pool.v)) || (rc = dalloc(c, &d_tsy, (size_t)NSn, pool.v))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_src, hsrc.data(), (size_t)Nn * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_nvoff, nvoff.data(), ((size_t)Nn + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_nsoff, nsoff.data(), ((size_t)Nn + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(sz_k_mig_gather, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (const int*)d_src, (const double*)d_dirs, (const double*)d_recvb,
                     (double* const*)d_cols, d_tmp);
  hipLaunchKernelGGL(sz_k_mig_points, dim3(grid_for((long long)Nn * 64, 256, 4096)), dim3(256), 0, c->stream, S, Nn, (const int*)d_src, (const double*)d_dirs,
                     (const double*)d_recvb, (const int*)d_nvoff, (const int*)d_nsoff, d_tv, d_tsx, d_tsy);
  hipLaunchKernelGGL(sz_k_mig_scatter, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (double* const*)d_cols, (const double*)d_tmp);
  if (Vn) HIPCHK(c, hipMemcpyAsync(S.vxy, d_tv, (size_t)Vn * sizeof(double2), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(S.voff, d_nvoff, ((size_t)Nn + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  Pool old_sub;
  if (NSn > S.capS) {          // the sub-floe points have no slack at upload (they are the largest array of a field): a tile that gained points gets a new pair
    old_sub = c->sub_allocs; c->sub_allocs = Pool();
    S.capS = NSn + NSn / 4;
    if ((rc = dalloc(c, &S.sx, (size_t)S.capS, c->sub_allocs)) || (rc = dalloc(c, &S.sy, (size_t)S.capS, c->sub_allocs))) return rc;
  }
  if (NSn) {
    HIPCHK(c, hipMemcpyAsync(S.sx, d_tsx, (size_t)NSn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.sy, d_tsy, (size_t)NSn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipMemcpyAsync(S.soff, d_nsoff, ((size_t)Nn + 1) * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  // ---- the field is placed: as behind the copies of sz_upload_floes (no ghosts; every floe's sub-floe offsets are set; the estimates and bounds the
  // context held still bound the floes it kept, those of the floes that arrived come on top).  No interaction rows until the next collision call
  // -- an upload keeps those of a field of the same size.
  HIPCHK(c, hipMemsetAsync(S.inter_cnt, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));
  const Retile tiling(c);
  if ((rc = field_placed(c, Nn, 0, Vn, Nn, std::min(Nn, c->gl_est + R), std::max(c->rmax_max, rmax_in), c->rmax_hint))) return rc;
  free_pool(old_sub);
  c->max_ring = std::max(c->max_ring, ring_in); c->max_sub = std::max(c->max_sub, sub_in);
  c->inter_lost = false; c->inter_any = true;
  c->tile_inter_state = TILE_INTER_MIGRATED;          // (a tile frame with lists says so: no rows of a last step to record)
  if ((rc = tiling.again(c, ngid.data(), owner_override ? 0 : px, py))) return rc;
  trim_pool(pool.v);
  if (n_owned) *n_owned = Nn;
  return SZ_OK;
}
int tile_migrate_host(sz_ctx* c, int32_t px, int32_t py, const int32_t* owner_override, int64_t* n_sent, int64_t* n_owned) {
  State& S = c->S;
  const int n = c->comm_n, me = c->comm_rank;
  int rc;
  const int N = c->hostN;
  // ---- the tile's state on the host
  const ColTable<double*> dcol = state_columns(S);
  std::vector<std::vector<double>> col(MIG_NTAB);
  std::vector<long long> id((size_t)N); std::vector<int> status((size_t)N), voff((size_t)N + 1), soff((size_t)N + 1);
  for (int k = 0; k < MIG_NTAB; k++) {
    col[k].resize(col_width(k) * N);
    if (N) HIPCHK(c, hipMemcpy(col[k].data(), dcol.p[k], col[k].size() * sizeof(double), hipMemcpyDeviceToHost));
  }
  if (N) { HIPCHK(c, hipMemcpy(id.data(), S.id, (size_t)N * sizeof(long long), hipMemcpyDeviceToHost)); HIPCHK(c, hipMemcpy(status.data(), S.status, (size_t)N * sizeof(int), hipMemcpyDeviceToHost)); }
  HIPCHK(c, hipMemcpy(voff.data(), S.voff, ((size_t)N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(soff.data(), S.soff, ((size_t)N + 1) * sizeof(int), hipMemcpyDeviceToHost));
  const int V = voff[N], NS = soff[N];
  std::vector<double> vx((size_t)std::max(V, 1)), vy((size_t)std::max(V, 1)), sx((size_t)std::max(NS, 1)), sy((size_t)std::max(NS, 1));
  if (V) {
    std::vector<double> xy((size_t)2 * V);
    HIPCHK(c, hipMemcpy(xy.data(), S.vxy, (size_t)2 * V * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < V; k++) { vx[k] = xy[(size_t)2 * k]; vy[k] = xy[(size_t)2 * k + 1]; }
  }
  if (NS) { HIPCHK(c, hipMemcpy(sx.data(), S.sx, (size_t)NS * sizeof(double), hipMemcpyDeviceToHost)); HIPCHK(c, hipMemcpy(sy.data(), S.sy, (size_t)NS * sizeof(double), hipMemcpyDeviceToHost)); }
  // ---- who owns what now: the tile that holds the centroid (periodic: of its image inside the domain), px x py tiles over the domain
  const double x0 = c->h_vals[3], y0 = c->h_vals[1], Lx = c->h_vals[2] - c->h_vals[3], Ly = c->h_vals[0] - c->h_vals[1];
  std::vector<int> owner((size_t)N);
  for (int i = 0; i < N; i++) {
    if (owner_override) { owner[i] = owner_override[i]; if (owner[i] < 0 || owner[i] >= n) { c->err = "sz_tile_migrate: owner out of range"; return SZ_E_ARG; } continue; }
    double x = col[COL_cx][i] - x0, y = col[COL_cy][i] - y0;
    if (c->tile_per_x) { x = std::fmod(x, Lx); if (x < 0) x += Lx; }
    if (c->tile_per_y) { y = std::fmod(y, Ly); if (y < 0) y += Ly; }
    const int ix = std::max(0, std::min(px - 1, (int)(x / Lx * px))), iy = std::max(0, std::min(py - 1, (int)(y / Ly * py)));
    owner[i] = iy * px + ix;
  }
  // ---- movers, one stream of doubles per destination: the MIG_NCOL doubles of a record (sz_columns.hpp), then ring x.. / y.., then sub-floe points
  // x.. / y.. of every floe
  std::vector<std::vector<double>> sendv(n), recvv;
  int nmove = 0;
  for (int i = 0; i < N; i++) {
    if (owner[i] == me) continue;
    nmove++;
    std::vector<double>& b = sendv[owner[i]];
    const int nv = voff[i + 1] - voff[i], ns = soff[i + 1] - soff[i];
    double rec[MIG_NCOL];
    for (int k = 0; k < MIG_NSC; k++) rec[k] = col[k][i];
    for (int t = 0; t < MIG_NTEN; t++) for (int q = 0; q < 4; q++) rec[MIG_TEN + 4 * t + q] = col[MIG_NSC + t][(size_t)4 * i + q];
    rec[MIG_ID] = (double)id[i]; rec[MIG_STATUS] = (double)status[i]; rec[MIG_GIDX] = (double)c->tile_gidx[i]; rec[MIG_NV] = (double)nv; rec[MIG_NS] = (double)ns;
    b.insert(b.end(), rec, rec + MIG_NCOL);
    b.insert(b.end(), vx.begin() + voff[i], vx.begin() + voff[i + 1]); b.insert(b.end(), vy.begin() + voff[i], vy.begin() + voff[i + 1]);
    b.insert(b.end(), sx.begin() + soff[i], sx.begin() + soff[i + 1]); b.insert(b.end(), sy.begin() + soff[i], sy.begin() + soff[i + 1]);
  }
  if ((rc = comm_alltoallv(c, sendv, recvv))) return rc;
  // did anything move anywhere?  (every rank must take the same branch: the rebuild below ends in collective set-up calls)
  int moved_all = 0;
  if ((rc = comm_agree_bits(c, nmove > 0 ? 1 : 0, &moved_all))) return rc;
  if (n_sent) *n_sent = nmove;
  if (!moved_all) { if (n_owned) *n_owned = N; return SZ_OK; }
  // ---- the new tile: kept floes + received ones, ordered by global index
  struct Src { long long g; int from; size_t at; };          // from < 0: local row `at`; else stream `from`, offset `at`
  std::vector<Src> src;
  for (int i = 0; i < N; i++) if (owner[i] == me) src.push_back({ c->tile_gidx[i], -1, (size_t)i });
  for (int s2 = 0; s2 < n; s2++) {
    const std::vector<double>& b = recvv[s2];
    for (size_t at = 0; at < b.size();) {
      if (at + MIG_NCOL > b.size()) { c->err = "sz_tile_migrate: truncated record"; return SZ_E_STATE; }
      const int nv = (int)b[at + MIG_NV], ns = (int)b[at + MIG_NS];
      src.push_back({ (long long)b[at + MIG_GIDX], s2, at });
      at += (size_t)MIG_NCOL + 2 * (size_t)nv + 2 * (size_t)ns;
    }
  }
  std::sort(src.begin(), src.end(), [](const Src& a, const Src& b2) { return a.g < b2.g; });
  const int Nn = (int)src.size();
  if (Nn == 0) { c->err = "sz_tile_migrate: a tile without floes (every rank must own at least one)"; return SZ_E_STATE; }
  std::vector<std::vector<double>> ncol(MIG_NTAB);
  for (int k = 0; k < MIG_NTAB; k++) ncol[k].resize(col_width(k) * Nn);
  std::vector<long long> nid((size_t)Nn), ngid((size_t)Nn); std::vector<int> nstatus((size_t)Nn), nvoff((size_t)Nn + 1, 0), nsoff((size_t)Nn + 1, 0);
  std::vector<double> nvx, nvy, nsx, nsy;
  for (int r = 0; r < Nn; r++) {
    const Src& q = src[r];
    ngid[r] = q.g;
    if (q.from < 0) {
      const size_t i = q.at;
      for (int k = 0; k < MIG_NTAB; k++) std::copy_n(&col[k][col_width(k) * i], col_width(k), &ncol[k][col_width(k) * r]);
      nid[r] = id[i]; nstatus[r] = status[i];
      nvx.insert(nvx.end(), vx.begin() + voff[i], vx.begin() + voff[i + 1]); nvy.insert(nvy.end(), vy.begin() + voff[i], vy.begin() + voff[i + 1]);
      nsx.insert(nsx.end(), sx.begin() + soff[i], sx.begin() + soff[i + 1]); nsy.insert(nsy.end(), sy.begin() + soff[i], sy.begin() + soff[i + 1]);
    } else {
      const double* b = recvv[q.from].data() + q.at;
      for (int k = 0; k < MIG_NSC; k++) ncol[k][r] = b[k];
      for (int t = 0; t < MIG_NTEN; t++) std::copy_n(b + MIG_TEN + 4 * t, 4, &ncol[MIG_NSC + t][(size_t)4 * r]);
      nid[r] = (long long)b[MIG_ID]; nstatus[r] = (int)b[MIG_STATUS];
      const int nv = (int)b[MIG_NV], ns = (int)b[MIG_NS];
      const double* p = b + MIG_NCOL;
      nvx.insert(nvx.end(), p, p + nv); nvy.insert(nvy.end(), p + nv, p + 2 * nv);
      p += 2 * (size_t)nv;
      nsx.insert(nsx.end(), p, p + ns); nsy.insert(nsy.end(), p + ns, p + 2 * ns);
    }
    nvoff[r + 1] = (int)nvx.size(); nsoff[r + 1] = (int)nsx.size();
  }
  if (nvx.empty()) { nvx.push_back(0.0); nvy.push_back(0.0); }
  if (nsx.empty()) { nsx.push_back(0.0); nsy.push_back(0.0); }
  // ---- rebuild through the upload path, then the tile set-up again
  const Retile tiling(c);
  sz_floe_columns f; memset(&f, 0, sizeof(f));
  const ColTable<double**> fcol = host_column_slots(f);
  for (int k = 0; k < MIG_NTAB; k++) *fcol.p[k] = ncol[k].data();
  f.id = (int64_t*)nid.data(); f.status = nstatus.data(); f.vert_off = nvoff.data(); f.vx = nvx.data(); f.vy = nvy.data(); f.sub_off = nsoff.data(); f.sx = nsx.data(); f.sy = nsy.data();
  if ((rc = sz_upload_floes(c, Nn, Nn, &f))) return rc;
  c->inter_lost = false; c->inter_any = true;
  c->tile_inter_state = TILE_INTER_MIGRATED;          // (a tile frame with lists says so: no rows of a last step to record)
  HIPCHK(c, hipMemsetAsync(S.inter_cnt, 0, ((size_t)S.capM + 1) * sizeof(int), c->stream));          // (no rows until the next collision call)
  if ((rc = tiling.again(c, ngid.data(), owner_override ? 0 : px, py))) return rc;
  if (n_owned) *n_owned = Nn;
  return SZ_OK;
}
}  // namespace

int sz_tile_migrate(sz_ctx* c, int32_t px, int32_t py, const int32_t* owner_override, int64_t* n_sent, int64_t* n_owned) {
  if (n_sent) *n_sent = 0;
  if (c && c->rr_pending >= 0) { c->err = "sz_tile_migrate: a ridge / raft step is pending (sz_ridgeraft_pending): sz_tile_step_finish runs its second half first"; return SZ_E_STATE; }
  if (!c || tiled_ready(c, "sz_tile_migrate") || px < 1 || py < 1 || (!owner_override && px * py != c->comm_n)) {
    if (c) c->err = "sz_tile_migrate needs a tiled context after sz_tile_setup, and px * py == the number of ranks";
    return SZ_E_STATE;
  }
  (void)hipSetDevice(c->device);
  int rc = tile_sync_agree(c); if (rc) return rc;             // (ghosts and halo floes of the last step are dropped: the state is the owned floes)
  world_rings(c);
  c->migrate_path = 0;
  const char* e = getenv("SZ_MIGRATE_HOST");                  // (A/B switch, the same on every rank: the host-staged path only)
  if (!(e && atoi(e) != 0)) {
    int fell_back = 0;
    rc = tile_migrate_device(c, px, py, owner_override, n_sent, n_owned, &fell_back);
    if (rc) return rc;
    if (!fell_back) { c->migrate_path = 1; return SZ_OK; }
  }
  rc = tile_migrate_host(c, px, py, owner_override, n_sent, n_owned);
  if (rc == SZ_OK) c->migrate_path = 2;
  return rc;
}
// how the last sz_tile_migrate ran: 1 = movers packed on the device, 2 = staged through the host (0: it did not get that far)
int sz_debug_migrate_path(sz_ctx* c) { return c ? c->migrate_path : 0; }
// global indices of the owned floes (sz_tile_enable; after sz_tile_migrate: of the new tile), n_cap >= the number of owned floes
int sz_tile_owned_gidx(sz_ctx* c, int64_t* out, int64_t n_cap) {
  if (!c || !c->have_floes || !c->S.tiled || !out || n_cap < (int64_t)c->tile_gidx.size()) return SZ_E_ARG;
  for (size_t i = 0; i < c->tile_gidx.size(); i++) out[i] = c->tile_gidx[i];
  return SZ_OK;
}

// ---------------------------------------------------------------- removal and dissolution on a tiled context (sz_remove_tile.hpp)
namespace {
// remove_floes! over the ONE global floe list whose rows live on the ranks' tiles: collective.  Every rank ends with what the single context's
// pass (remove_pass) leaves for that list, restricted to the floes it owns, numbered as the single context numbers them; *done = 0: declined on
// EVERY rank, nothing has changed on any.  The counts are global.  The collectives, the same on every rank whatever it holds:
//   1. the agreement on this rank's state (device error bits, ghosts in the list)
//   2. the all-gather of the counts (RmDev of every rank): the verdict they allow -- a fuse tag, a ring over max_vertices, a rank or the world
//      left without a floe -- is the same on every rank, and so is "nothing leaves"; both end the pass here, on all ranks
//   3. the all-gather of the leaving records, as many slots per rank as the longest list needs
//   4. the agreement on the verdict of the walk (the index quirk) and on this rank's counts, BEFORE the lattice or a row changes
// In front of 2 and of 3 the ranks gather the code of what each prepared alone (scratch memory: N differs per rank), so a rank that fails there
// takes the others with it instead of leaving them in the gather.  A failure of the HIP runtime or of the channel itself (SZ_E_HIP out of a
// copy, a launch or a collective) is returned at once, as everywhere in the library: there is nothing left to agree over.
// An empty tile is not a state the tile drivers are tested in: a pass that would leave one is declined.
int tile_remove_pass(sz_ctx* c, int* done, int* n_removed, int* n_dissolved) {
  constexpr int BIT_GHOSTS = 1 << 30, BIT_NONE = 1 << 29;          // the word of agreement 1 ...
  constexpr int BIT_ERR = 1, BIT_COUNTS = 2, BIT_INDEX = 4, BIT_LATTICE = 8, BIT_WENT = 16;          // ... and of agreement 4
  *done = 0; *n_removed = 0; *n_dissolved = 0;
  State& S = c->S;
  const int n = c->comm_n, me = c->comm_rank;
  int rc, all = 0;
  constexpr const char* who = "sz_tile_remove_floes";
  // ---- 1
  rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  const int state = rc ? (c->last_err_bits ? c->last_err_bits & ~(BIT_GHOSTS | BIT_NONE) : 1) : c->hostM != c->hostN ? BIT_GHOSTS : c->hostN <= 0 ? BIT_NONE : 0;
  if ((rc = comm_agree_bits(c, state, &all))) return rc;
  if (all & ~(BIT_GHOSTS | BIT_NONE)) return SZ_E_CAPACITY;
  if (all & BIT_GHOSTS) { c->err = "sz_tile_remove_floes: ghosts are in the list on some rank: the pass runs over the parents alone"; return SZ_E_STATE; }
  c->err.clear();
  if (all) return SZ_OK;          // (a rank without floes: declined)
  const int N = c->hostN;
  leave_resident(c);
  // ---- 2
  RmArgs A;
  Pool& P = c->rm_allocs;
  constexpr int RW = (int)(sizeof(RmDev) / sizeof(int));
  int *d_counts = nullptr, *d_decl = nullptr, first = 0;
  (void)((rc = rm_flag_rows(c, N, A)) || (rc = dalloc(c, &d_counts, (size_t)RW * 64, P)) || (rc = dalloc(c, &d_decl, 1, P)));
  if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
  if (first) return first;
  if ((rc = comm_allgather(c, A.d, d_counts, RW, NCCL_INT32, sizeof(int)))) return rc;
  std::vector<RmDev> Rs(n);
  HIPCHK(c, hipMemcpyAsync(Rs.data(), d_counts, (size_t)n * sizeof(RmDev), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const RmDev R = Rs[me];
  int decl = 0, nr = 0, nd = 0, left = 0;
  std::vector<int> cnt(64, 0);
  for (int r = 0; r < n; r++) {
    decl |= (Rs[r].n_fuse ? RM_DECL_FUSE : 0) | (Rs[r].n_over ? RM_DECL_VERTS : 0) | (Rs[r].Nn <= 0 ? RM_DECL_EMPTY : 0);
    cnt[r] = Rs[r].n_removed + Rs[r].n_dissolved;
    nr += Rs[r].n_removed; nd += Rs[r].n_dissolved; left += Rs[r].Nn;
  }
  if (decl || left <= 0) return SZ_OK;
  ListGather LG(c, cnt.data(), RMT_REC, 0);
  const int slots = LG.slots, total = (int)LG.total;
  if (total == 0) { *done = 1; return SZ_OK; }          // nothing leaves anywhere, and every status is `active` already
  // ---- 3
  const int Nn = std::max(R.Nn, 0);
  double* d_merged = nullptr; long long* d_newkey = nullptr;
  (void)((rc = LG.carve(c, P)) || (rc = dalloc(c, &d_merged, (size_t)RMT_REC * total, P)) || (rc = dalloc(c, &d_newkey, (size_t)Nn + 1, P)));
  if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
  if (first) return first;
  HIPCHK(c, hipMemsetAsync(LG.d_rec, 0, (size_t)RMT_REC * slots * sizeof(double), c->stream));
  HIPCHK(c, hipMemsetAsync(d_merged, 0, (size_t)RMT_REC * total * sizeof(double), c->stream));
  if ((rc = LG.upload_counts(c, cnt.data()))) return rc;
  const bool counts_ok = Nn > 0 && Nn <= N && Nn + cnt[me] == N && R.Vn >= 0 && R.NSn >= 0;      // (the records go where the scans say: not with bad counts)
  if (counts_ok) hipLaunchKernelGGL(sz_k_rmt_pack, dim3(grid_for(N, 256, 2048)), dim3(256), 0, c->stream, S, A, LG.d_rec);
  if ((rc = LG.gather(c))) return rc;
  hipLaunchKernelGGL(sz_k_rmt_merge, dim3(grid_for((long long)n * slots, 256)), dim3(256), 0, c->stream, (const double*)LG.d_all, (const int*)LG.d_cnt, n, slots, d_merged, total);
  if (counts_ok) hipLaunchKernelGGL(sz_k_rmt_renumber, dim3(grid_for(Nn, 256)), dim3(256), 0, c->stream, S, Nn, (const int*)A.src, (const double*)d_merged, total, d_newkey);
  hipLaunchKernelGGL(sz_k_rmt_walk, dim3(1), dim3(64), 0, c->stream, A, (const double*)d_merged, total, nd, (int)RM_WALK_CHECK, d_decl);
  // ---- 4 (nothing has changed so far, on any rank: the walk has only looked)
  int walk = 0;
  std::vector<long long> newkey((size_t)Nn + 1, 0);
  HIPCHK(c, hipMemcpyAsync(&walk, d_decl, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (counts_ok) HIPCHK(c, hipMemcpyAsync(newkey.data(), d_newkey, (size_t)Nn * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  const int mine = (rc ? BIT_ERR : 0) | (counts_ok ? 0 : BIT_COUNTS) | (walk & RM_DECL_INDEX ? BIT_INDEX : 0) | (walk & RM_NO_LATTICE ? BIT_LATTICE : 0) | (walk ? 0 : BIT_WENT);
  if ((rc = comm_agree_bits(c, mine, &all))) return rc;
  if (all & BIT_ERR) return SZ_E_CAPACITY;
  if (all & BIT_COUNTS) { c->err = "sz_tile_remove_floes: bad counts on some rank"; return SZ_E_HIP; }
  if (all & BIT_LATTICE) { c->err = "sz_tile_remove_floes: a floe dissolves, and the ocean.dissolved lattice needs the grid (sz_set_fields)"; return SZ_E_STATE; }
  if ((all & BIT_INDEX) && (all & BIT_WENT)) { c->err = "sz_tile_remove_floes: the ranks walked the same list to different ends: their grids (sz_set_fields) differ"; return SZ_E_STATE; }
  c->err.clear();
  if (all & BIT_INDEX) return SZ_OK;
  *done = 1; *n_removed = nr; *n_dissolved = nd;
  // ---- the pass goes ahead on every rank: the sums of the walk, then the rows move as in the single context -- on every rank, one that loses no
  // floe included: its numbers change with the floes that left before them, and the next batch gathers the boxes anew on all ranks or on none.
  // The tiling is taken before the new field forgets it and established again behind it, with the new numbers (S.okey, tile_gidx) and the
  // centre the owned box was last gathered around.  Boxes, halo capacities and peers: the next exchange
  if (nd > 0) hipLaunchKernelGGL(sz_k_rmt_walk, dim3(1), dim3(64), 0, c->stream, A, (const double*)d_merged, total, nd, (int)RM_WALK_SUM, d_decl);
  const Retile tiling(c);
  const bool ctr_valid = c->tile_box_valid; const double ctr[2] = { c->tile_box_ctr[0], c->tile_box_ctr[1] };
  if ((rc = rm_move_rows(c, N, A, R))) return rc;
  if ((rc = tiling.again(c, newkey.data(), 0, 0))) return rc;
  if (ctr_valid) (void)sz_tile_set_center(c, ctr[0], ctr[1]);
  return SZ_OK;
}
}  // namespace
int sz_tile_remove_floes(sz_ctx* c, int32_t* done, int32_t* n_removed, int32_t* n_dissolved) {
  if (done) *done = 0;
  if (n_removed) *n_removed = 0;
  if (n_dissolved) *n_dissolved = 0;
  if (!c || !done) return SZ_E_ARG;
  if (int rc = tiled_ready(c, "sz_tile_remove_floes")) return rc;
  (void)hipSetDevice(c->device);
  int d = 0, nr = 0, nd = 0;
  if (int rc = tile_remove_pass(c, &d, &nr, &nd)) return rc;
  *done = d;
  if (n_removed) *n_removed = nr;
  if (n_dissolved) *n_dissolved = nd;
  return SZ_OK;
}

// ---------------------------------------------------------------- row edits by global number (sz_splice_tile.hpp)
namespace {
// names[0 .. n): no negative one, none twice; sorted: ascending as given
int spt_check_names(sz_ctx* c, const std::string& who, const char* what, int n, const int64_t* names, bool sorted) {
  std::vector<int64_t> tmp;
  const int64_t* g = names;
  if (!sorted && n > 1) { tmp.assign(names, names + n); std::sort(tmp.begin(), tmp.end()); g = tmp.data(); }
  for (int k = 0; k < n; k++) {
    if (g[k] < 0) { c->err = who + ": " + what + " names floe " + std::to_string((long long)g[k]) + ": global numbers start at 0"; return SZ_E_ARG; }
    if (k && g[k] <= g[k - 1]) { c->err = who + ": " + what + (g[k] == g[k - 1] ? " repeats floe " + std::to_string((long long)g[k]) : std::string(" is not ascending")); return SZ_E_ARG; }
  }
  return SZ_OK;
}
// the binary searches of sz_k_spt_* need the owned numbers ascending by row: TiledWorld, sz_tile_migrate and sz_tile_remove_floes leave them so,
// sz_tile_enable takes any order
bool spt_ascending(const sz_ctx* c) {
  const std::vector<long long>& g = c->tile_gidx;
  for (size_t i = 1; i < g.size(); i++) if (g[i] <= g[i - 1]) return false;
  return true;
}
// names per find and scan of sz_tile_download_rows.  The engine's three-launch scan notes one total per SCAN_B elements in S.blk, which is sized by the
// context's capacities and holds at least 1024 of them whatever those are: a request of any length stays inside it in rounds of this size
constexpr int SPT_CHUNK = 1024 * SCAN_B;
constexpr const char* SPT_ORDER_MSG = ": the global numbers of the owned floes are not ascending by row (sz_tile_enable takes any order; rows are found by binary search)";

// the staged floes `sel` (ascending positions among the ns = n_rep + n_app uploaded floes) as a list of their own: this rank's share
struct SptSubset {
  std::vector<std::vector<double>> keep; std::vector<int64_t> id; std::vector<int32_t> status, voff, soff, ioff;
  std::vector<double> vx, vy, sx, sy, irows;
  sz_floe_columns f;
  SptSubset(const sz_floe_columns* a, const int32_t* a_ioff, const double* a_irows, const std::vector<int>& sel) {
    memset(&f, 0, sizeof(f));
    const size_t m = sel.size();
    if (!a || m == 0) return;
    auto pick = [&](const double* src, int w) -> double* {
      if (!src) return nullptr;
      keep.emplace_back(m * w);
      for (size_t k = 0; k < m; k++) for (int q = 0; q < w; q++) keep.back()[k * w + q] = src[(size_t)sel[k] * w + q];
      return keep.back().data();
    };
#define X(host, state) f.host = pick(a->host, (int)col_width(COL_##host));
    SZ_ALL_COLUMNS(X)
#undef X
    if (a->id) { for (int j : sel) id.push_back(a->id[j]); f.id = id.data(); }
    if (a->status) { for (int j : sel) status.push_back(a->status[j]); f.status = status.data(); }
    voff.assign(1, 0); soff.assign(1, 0); ioff.assign(1, 0);
    for (int j : sel) {
      for (int q = a->vert_off[j]; q < a->vert_off[j + 1]; q++) { vx.push_back(a->vx[q]); vy.push_back(a->vy[q]); }
      voff.push_back((int32_t)vx.size());
      if (a->sub_off) { for (int q = a->sub_off[j]; q < a->sub_off[j + 1]; q++) { sx.push_back(a->sx[q]); sy.push_back(a->sy[q]); } soff.push_back((int32_t)sx.size()); }
      if (a_ioff) { for (size_t q = (size_t)a_ioff[j] * 7; q < (size_t)a_ioff[j + 1] * 7; q++) irows.push_back(a_irows[q]); ioff.push_back((int32_t)(irows.size() / 7)); }
    }
    vx.push_back(0.0); vy.push_back(0.0); sx.push_back(0.0); sy.push_back(0.0); irows.push_back(0.0);          // (never NULL where the offsets are given)
    f.vert_off = voff.data(); f.vx = vx.data(); f.vy = vy.data();
    if (a->sub_off) { f.sub_off = soff.data(); f.sx = sx.data(); f.sy = sy.data(); }
  }
};
}  // namespace

// The rows `gidx` of the global list that this rank owns: local, not collective.  sz_k_spt_find and the engine's scan name them; the rows come through
// sp_download, the path of sz_download_rows (one staging buffer, one copy).
int sz_tile_download_rows(sz_ctx* c, int32_t n, const int64_t* gidx, int32_t* n_mine, int32_t* which, sz_floe_columns* f, int32_t* inter_off, double* inter_rows, int64_t* sizes3) {
  const std::string who = "sz_tile_download_rows";
  if (n_mine) *n_mine = 0;
  if (!c || n < 0 || !n_mine || (n > 0 && (!gidx || !which))) return SZ_E_ARG;
  if (!c->have_floes || !c->S.tiled) { c->err = who + " needs sz_tile_enable after the last sz_upload_floes: on a single context sz_download_rows names the rows"; return SZ_E_STATE; }
  if (c->rr_pending >= 0) { c->err = who + ": a ridge / raft step is pending with halo rows and ghosts in the list (sz_tile_step_finish first)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  int rc;
  if ((rc = sync_and_check(c))) return rc;          // hostM / hostN current; the halo rows and ghosts of the last step are dropped
  if (c->hostM != c->hostN) { c->err = who + ": ghosts are in the list (sz_remove_ghosts first): the rows are the parents'"; return SZ_E_STATE; }
  if (!spt_ascending(c)) { c->err = who + SPT_ORDER_MSG; return SZ_E_STATE; }
  if ((rc = spt_check_names(c, who, "gidx", n, gidx, false))) return rc;
  const int N = c->hostN;
  std::vector<int> hw((size_t)n + 1, 0), hr((size_t)n + 1, 0);
  int cnt = 0;
  if (n > 0) {
    Pool& P = c->spt_allocs;
    reset_pool(P);
    long long* d_names = nullptr; int *d_loc = nullptr, *d_flag = nullptr, *d_pos = nullptr, *d_which = nullptr, *d_rows = nullptr;
    const size_t n1 = (size_t)n + 1, c1 = (size_t)std::min((int)n, SPT_CHUNK) + 1;
    if ((rc = dalloc(c, &d_names, n1, P)) || (rc = dalloc(c, &d_loc, c1, P)) || (rc = dalloc(c, &d_flag, c1, P)) || (rc = dalloc(c, &d_pos, c1 + 1, P)) ||
        (rc = dalloc(c, &d_which, n1, P)) || (rc = dalloc(c, &d_rows, n1, P))) return rc;
    H2D(d_names, gidx, n, long long);
    // n is the caller's, not one of the context's capacities: the names go through the find and the scan SPT_CHUNK at a time (one round for any
    // request a run makes), and every round appends what it found behind the rounds before it
    for (int k0 = 0; k0 < n; k0 += SPT_CHUNK) {
      const int m = std::min(SPT_CHUNK, (int)n - k0), nb = grid_for(m, 256, 2048);
      int got = -1;
      hipLaunchKernelGGL(sz_k_spt_find, dim3(nb), dim3(256), 0, c->stream, c->S, N, m, k0, (const long long*)d_names + k0, d_loc, d_flag, (const int*)nullptr, d_which + cnt, d_rows + cnt);
      scan(c, d_flag, d_pos, m, -1, m, -1);
      hipLaunchKernelGGL(sz_k_spt_find, dim3(nb), dim3(256), 0, c->stream, c->S, N, m, k0, (const long long*)d_names + k0, d_loc, d_flag, (const int*)d_pos, d_which + cnt, d_rows + cnt);
      HIPCHK(c, hipMemcpyAsync(&got, d_pos + m, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(hw.data() + cnt, d_which + cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));          // (cnt <= k0: the m entries lie inside the n)
      HIPCHK(c, hipMemcpyAsync(hr.data() + cnt, d_rows + cnt, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      if (got < 0 || got > m) { c->err = who + ": bad counts"; return SZ_E_HIP; }
      cnt += got;
    }
    for (int k = 0; k < cnt; k++) if (hr[k] < 0 || hr[k] >= N || hw[k] < 0 || hw[k] >= n) { c->err = who + ": bad rows"; return SZ_E_HIP; }
  }
  for (int k = 0; k < cnt; k++) which[k] = hw[k];
  *n_mine = cnt;
  return sp_download(c, who.c_str(), false, cnt, hr.data(), f, inter_off, inter_rows, sizes3);
}

// One edit of the global list, stated in global numbers with the same arguments on every rank: collective.  Every rank applies the share that
// concerns the rows it owns -- no floe data crosses between the ranks; the one collective is the all-gather of a per-rank record {error bits, rows
// owned, `del` names found, `rep` names found, appended floes taken} in front of the change, from which every rank derives N_global and the same
// verdict.  Behind it the rows move through the body of sz_splice_floes (sp_splice_rows) with local rows, the staged floes this rank takes and the
// new global numbers (sz_k_spt_renumber), and the tiling is established again as behind tile_remove_pass.
int sz_tile_splice_floes(sz_ctx* c, int32_t n_del, const int64_t* del, int32_t n_rep, const int64_t* rep, int32_t n_app, const int32_t* app_owner, const sz_floe_columns* f,
                         const int32_t* ioff, const double* irows, int64_t* n_global, int64_t* n_owned) {
  const std::string who = "sz_tile_splice_floes";
  if (n_global) *n_global = -1;
  if (n_owned) *n_owned = -1;
  if (!c || n_del < 0 || n_rep < 0 || n_app < 0 || (n_del && !del) || (n_rep && !rep)) return SZ_E_ARG;
  const long long ns64 = (long long)n_rep + n_app;
  if (ns64 > 0x3fffffff || (long long)n_del + n_rep > 0x3fffffff) return SZ_E_ARG;
  const int ns = (int)ns64, nn = n_del + n_rep;
  if (n_app > 0 && !app_owner) { c->err = who + ": appended floes need app_owner, the rank that takes each"; return SZ_E_ARG; }
  if (ns > 0 && (!f || !f->vert_off || !f->vx || !f->vy || !f->cx || !f->cy)) { c->err = who + ": replaced / appended rows need vert_off, vx, vy, cx and cy"; return SZ_E_ARG; }
  int rc;
  if ((rc = tiled_ready(c, who.c_str()))) return rc;
  if (c->rr_pending >= 0) { c->err = who + ": a ridge / raft step is pending with halo rows and ghosts in the list (sz_tile_step_finish first)"; return SZ_E_STATE; }
  const int n = c->comm_n, me = c->comm_rank;
  // ---- what the arguments alone decide: the same verdict on every rank, no collective needed
  if ((rc = spt_check_names(c, who, "del", n_del, del, true)) || (rc = spt_check_names(c, who, "rep", n_rep, rep, true))) return rc;
  for (int a = 0, b = 0; a < n_del && b < n_rep;) {
    if (del[a] == rep[b]) { c->err = who + ": floe " + std::to_string((long long)del[a]) + " is both deleted and replaced"; return SZ_E_ARG; }
    if (del[a] < rep[b]) a++; else b++;
  }
  int app_mine = 0;
  for (int k = 0; k < n_app; k++) {
    if (app_owner[k] < 0 || app_owner[k] >= n) { c->err = who + ": app_owner[" + std::to_string(k) + "] = " + std::to_string(app_owner[k]) + ", outside the " + std::to_string(n) + " ranks"; return SZ_E_ARG; }
    app_mine += app_owner[k] == me;
  }
  int bits = 0; bool with_sub = false; size_t stream_len = 0;
  if ((rc = sp_check_staged(c, who, ns, f, ioff, irows, &with_sub, &stream_len, &bits))) return rc;
  if (n_del + ns == 0) { if (n_owned) *n_owned = (int64_t)c->tile_gidx.size(); return SZ_OK; }          // nothing to do, nothing touched, no collective (*n_global stays -1: it takes one)
  // ---- this rank's state and its share of the names
  (void)hipSetDevice(c->device);
  rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  if (rc) bits |= SPT_BIT_ERR;
  const int N = c->hostN;
  if (!rc) bits |= c->hostM != N ? SPT_BIT_GHOSTS : N <= 0 ? SPT_BIT_NONE : !spt_ascending(c) ? SPT_BIT_ORDER : 0;
  Pool& P = c->spt_allocs;
  reset_pool(P);
  constexpr int RW = 5;          // the record: error bits, rows owned, `del` names found, `rep` names found, appended floes taken
  int *d_rec = nullptr, *d_all = nullptr, *d_loc = nullptr, *d_found = nullptr, *d_lrep = nullptr, *d_appk = nullptr; long long* d_names = nullptr;
  if ((rc = dalloc(c, &d_rec, 8, P)) || (rc = dalloc(c, &d_all, (size_t)RW * Gather::RANKS, P))) return rc;          // (the record's own two words: without them there is no gathering, as with a failed channel)
  // the scratch of the names: a rank that cannot have it says so in its record and goes into the gather, instead of leaving the others there
  // (tile_remove_pass agrees such a code with comm_agree_rc; here the record is the agreement)
  if (dalloc(c, &d_loc, (size_t)nn + 1, P) || dalloc(c, &d_found, 2, P) || dalloc(c, &d_names, (size_t)nn + 1, P) || dalloc(c, &d_lrep, (size_t)n_rep + 1, P) ||
      dalloc(c, &d_appk, (size_t)n_app + 1, P)) bits |= SPT_BIT_MEM;
  std::vector<int> loc((size_t)nn + 1, -1);
  int found[2] = { 0, 0 };
  if (!bits && nn > 0) {
    if (n_del) H2D(d_names, del, n_del, long long);
    if (n_rep) H2D(d_names + n_del, rep, n_rep, long long);
    HIPCHK(c, hipMemsetAsync(d_found, 0, 2 * sizeof(int), c->stream));
    hipLaunchKernelGGL(sz_k_spt_marks, dim3(grid_for(nn, 256, 2048)), dim3(256), 0, c->stream, c->S, N, (int)n_del, (int)n_rep, (const long long*)d_names, d_loc, d_found);
    HIPCHK(c, hipMemcpyAsync(loc.data(), d_loc, (size_t)nn * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(found, d_found, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // ---- the agreement, before anything changes
  const int rec[RW] = { bits, N, found[0], found[1], app_mine };
  std::vector<int> all((size_t)RW * n, 0);
  H2D(d_rec, rec, RW, int);
  if ((rc = comm_allgather(c, d_rec, d_all, RW, NCCL_INT32, sizeof(int)))) return rc;
  HIPCHK(c, hipMemcpyAsync(all.data(), d_all, all.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  long long Ng = 0; int allbits = 0, fdel = 0, frep = 0, empty_rank = -1;
  for (int r = 0; r < n; r++) {
    const int* a = &all[(size_t)RW * r];
    allbits |= a[0]; Ng += a[1]; fdel += a[2]; frep += a[3];
    if (empty_rank < 0 && (long long)a[1] - a[2] + a[4] <= 0) empty_rank = r;
  }
  const std::string some = bits ? " (this rank among them)" : " (not this one; all ranks return together)";
  if (allbits & SPT_BIT_MEM) { if (!(bits & SPT_BIT_MEM)) c->err = who + ": a rank of the tiled run could not allocate the scratch of the names" + some; return SZ_E_HIP; }
  if (allbits & SPT_BIT_ERR) { if (!(bits & SPT_BIT_ERR)) c->err = who + ": a rank of the tiled run reported device error bits" + some; return SZ_E_CAPACITY; }
  if (allbits & SPT_BIT_GHOSTS) { c->err = who + ": ghosts are in the list on some rank" + some + ": the edit is of the parents alone (sz_remove_ghosts first)"; return SZ_E_STATE; }
  if (allbits & SPT_BIT_NONE) { c->err = who + ": some rank holds no floe" + some; return SZ_E_STATE; }
  if (allbits & SPT_BIT_ORDER) { c->err = who + SPT_ORDER_MSG + ", on some rank" + some; return SZ_E_STATE; }
  if (allbits & SPT_BIT_POINTS) { c->err = who + ": an uploaded floe has sub-floe points, and some rank's list was uploaded without" + some; return SZ_E_ARG; }
  if (allbits & SPT_BIT_ROWCAP) { c->err = "more interaction rows per floe than the fixed stride holds on some rank" + some; return SZ_E_CAPACITY; }
  if (fdel != n_del || frep != n_rep) {
    c->err = who + ": the ranks own " + std::to_string(fdel) + " of the " + std::to_string(n_del) + " del names and " + std::to_string(frep) + " of the " + std::to_string(n_rep) +
             " rep names: a name outside the " + std::to_string(Ng) + " floes of the global list, or owned twice";
    return SZ_E_ARG;
  }
  const long long Nng = Ng - n_del + n_app;
  if (Nng <= 0) { c->err = who + ": the edit leaves no floe"; return SZ_E_ARG; }
  if (Nng > 0x3fffffff) { c->err = who + ": too many floes"; return SZ_E_ARG; }
  if (empty_rank >= 0) { c->err = who + ": the edit leaves no floe on rank " + std::to_string(empty_rank) + " (an empty tile is not a state the tile drivers run in)"; return SZ_E_ARG; }
  c->err.clear();
  // ---- the share: local rows, the staged floes this rank takes, their new global numbers
  std::vector<int32_t> ldel, lrep; std::vector<int> sel, appk; std::vector<long long> num;
  for (int t = 0; t < n_del; t++) if (loc[t] >= 0) ldel.push_back(loc[t]);
  for (int j = 0, below = 0; j < n_rep; j++) {
    while (below < n_del && del[below] < rep[j]) below++;
    if (loc[n_del + j] >= 0) { lrep.push_back(loc[n_del + j]); sel.push_back(j); num.push_back((long long)rep[j] - below); }
  }
  for (int k = 0; k < n_app; k++) if (app_owner[k] == me) { sel.push_back(n_rep + k); appk.push_back(k); num.push_back(Ng - n_del + k); }
  if ((int)ldel.size() != found[0] || (int)lrep.size() != found[1]) { c->err = who + ": bad counts"; return SZ_E_HIP; }
  const SptSubset mine(f, ioff, irows, sel);
  bool sub2 = false; size_t len2 = 0;
  if ((rc = sp_check_staged(c, who, (int)sel.size(), &mine.f, ioff ? mine.ioff.data() : nullptr, mine.irows.data(), &sub2, &len2))) return rc;          // (its sizes; the verdict is known)
  if (!lrep.empty()) H2D(d_lrep, lrep.data(), lrep.size(), int);
  if (!appk.empty()) H2D(d_appk, appk.data(), appk.size(), int);
  std::vector<long long> newkey;
  SpTile T{ SptKeys{ d_names, (int)n_del, d_lrep, (int)lrep.size(), d_appk, Ng - n_del }, num.data(), &newkey };
  // ---- the tiling before, with hints that cover every staged floe of the whole edit (every rank sees the same edit: the same maxima, no exchange)
  Retile tiling(c);
  for (int j = 0; j < ns; j++) {
    if (tiling.ring_hint > 0) tiling.ring_hint = std::max(tiling.ring_hint, (double)(f->vert_off[j + 1] - f->vert_off[j]));
    if (tiling.rmax_hint > 0 && f->rmax) tiling.rmax_hint = std::max(tiling.rmax_hint, f->rmax[j]);
  }
  const bool ctr_valid = c->tile_box_valid; const double ctr[2] = { c->tile_box_ctr[0], c->tile_box_ctr[1] };
  if ((rc = sp_splice_rows(c, who, false, (int32_t)ldel.size(), ldel.data(), (int32_t)lrep.size(), lrep.data(), (int32_t)appk.size(), sel.empty() ? nullptr : &mine.f,
                           ioff && !sel.empty() ? mine.ioff.data() : nullptr, mine.irows.data(), sub2, len2, &T))) return rc;
  if ((rc = tiling.again(c, newkey.data(), 0, 0))) return rc;
  if (ctr_valid) (void)sz_tile_set_center(c, ctr[0], ctr[1]);
  if (n_global) *n_global = Nng;
  if (n_owned) *n_owned = c->hostN;
  return SZ_OK;
}

int sz_tile_download_rows_f32(sz_ctx* c, int32_t n, const int64_t* gidx, int32_t* n_mine, int32_t* which, sz_floe_columns_f32* f, int32_t* inter_off, float* inter_rows, int64_t* sizes3) {
  if (!c || !n_mine) return SZ_E_ARG;
  int64_t sz[3] = { 0, 0, 0 };
  if (int rc = sz_tile_download_rows(c, n, gidx, n_mine, which, nullptr, nullptr, nullptr, sz)) return rc;          // (*n_mine and the sizes: the room the rows need)
  if (sizes3) { sizes3[0] = sz[0]; sizes3[1] = sz[1]; sizes3[2] = sz[2]; }
  if (!f) return SZ_OK;
  SpF32Down W((size_t)*n_mine, sz, f, inter_rows);
  if (int rc = sz_tile_download_rows(c, n, gidx, n_mine, which, &W.d, inter_off, W.ir, nullptr)) return rc;
  W.back();
  return SZ_OK;
}
int sz_tile_splice_floes_f32(sz_ctx* c, int32_t n_del, const int64_t* del, int32_t n_rep, const int64_t* rep, int32_t n_app, const int32_t* app_owner, const sz_floe_columns_f32* f,
                             const int32_t* ioff, const float* irows, int64_t* n_global, int64_t* n_owned) {
  if (!c || n_rep < 0 || n_app < 0) return SZ_E_ARG;
  const size_t M = (size_t)n_rep + (size_t)n_app;
  if (M == 0 || !f) return sz_tile_splice_floes(c, n_del, del, n_rep, rep, n_app, app_owner, nullptr, ioff, nullptr, n_global, n_owned);
  if (!f->vert_off) { c->err = "sz_tile_splice_floes_f32: vert_off is required"; return SZ_E_ARG; }
  const SpF32Up W(M, f, ioff, irows);
  return sz_tile_splice_floes(c, n_del, del, n_rep, rep, n_app, app_owner, &W.d, ioff, W.ir, n_global, n_owned);
}

// ---------------------------------------------------------------- fracture criteria on a tiled context (sz_fracture_tile.hpp)
namespace {
// determine_fractures over the ONE global floe list whose rows live on the ranks' tiles: collective, over the parents with ghosts detached (as
// behind a segment of sz_tile_run).  Every rank ends with the mean height, p and polygon of the single context, to the bit -- the heights of all
// ranks gathered by global number, then sz_k_frac_criterion over that array, unchanged -- and with the flags of the rows it owns (sz_k_frac_test
// over hostN rows; halo rows are never tested).  The collectives, the same on every rank whatever it holds:
//   1. the gather of the owned counts; a rank that cannot take part (device error bits, ghosts in the list) sends its error code in place of its
//      count, and all ranks return it together
//   2. the all-gather of the {global number, height} records, as many slots per rank as the longest list needs
//   3. the agreement (comm_agree_bits) on: a global number out of range or met twice, a device error, "I have a candidate", and my_tag -- "my stop
//      word stood at the segment's last step".  Behind the list-based driver that is news to the peers: they would hear of such a tag in the unpack
//      of a step that does not come.  The inline driver has agreed its stop step already (comm_agree_steps), and every rank sends the same bit
// Nothing of the floes changes in a pass; what 3 refuses has only written the pass's scratch and the criterion block.  A failure of the HIP runtime
// or of the channel itself is returned at once, as everywhere in the library.  compact: the owned candidates as ascending rows in frac_idx and
// their exact number in *n_owned (otherwise *n_owned is only zero or not).
constexpr int FRT_BIT_RANGE = 1, FRT_BIT_TWICE = 2, FRT_BIT_ERR = 4, FRT_BIT_CAND = 8, FRT_BIT_TAG = 16;          // the word of agreement 3
int tile_frac_pass(sz_ctx* c, bool my_tag, bool compact, int* any_cand, int* any_tag, int* n_owned) {
  *any_cand = 0; *any_tag = 0; *n_owned = 0;
  State& S = c->S;
  const int n = c->comm_n;
  // ---- 1
  int rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  if ((rc = rc ? rc : c->hostM != c->hostN ? (int)SZ_E_STATE : frac_ensure(c)) == SZ_E_HIP) return rc;
  const int N = c->hostN;
  c->frac_cnt.assign(64, 0);
  int* const cnt = c->frac_cnt.data();
  if (const int r2 = comm_gather_int(c, rc ? rc : N, cnt)) return r2;
  for (int r = 0; r < n; r++) if (cnt[r] < 0) {
    if (cnt[r] == SZ_E_STATE) c->err = "tiled fracture criteria: ghosts are in the list on rank " + std::to_string(r) + ": the pass runs over the parents alone";
    else if (!rc) c->err = "tiled fracture criteria: rank " + std::to_string(r) + " reported a device error (this rank is clean; all ranks return together)";
    return cnt[r];
  }
  ListGather LG(c, cnt, FRT_REC, 1);
  if (LG.total > 0x7fffffff) { c->err = "tiled fracture criteria: more than 2^31 floes"; return SZ_E_CAPACITY; }          // (the same sum on every rank)
  const int slots = LG.slots, total = (int)LG.total;
  // ---- 2
  Pool& P = c->frac_allocs;
  reset_pool(P);
  double* d_h = nullptr; int *d_mark = nullptr, *d_bad = nullptr;
  if ((rc = LG.carve(c, P)) || (rc = dalloc(c, &d_h, (size_t)total, P)) || (rc = dalloc(c, &d_mark, (size_t)total, P)) || (rc = dalloc(c, &d_bad, 1, P))) return rc;
  HIPCHK(c, hipMemsetAsync(d_mark, 0, (size_t)std::max(total, 1) * sizeof(int), c->stream));
  HIPCHK(c, hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
  if ((rc = LG.upload_counts(c, cnt))) return rc;
  if (N > 0) hipLaunchKernelGGL(sz_k_fract_pack, dim3(grid_for(N, 256, 2048)), dim3(256), 0, c->stream, S, N, LG.d_rec);
  if ((rc = LG.gather(c))) return rc;
  hipLaunchKernelGGL(sz_k_fract_scatter, dim3(grid_for((long long)n * slots, 256)), dim3(256), 0, c->stream, (const double*)LG.d_all, (const int*)LG.d_cnt, n, slots, d_h, d_mark, total, d_bad);
  // ---- the single context's kernels: the criterion over the gathered heights, the test over the owned rows
  State T = S; T.step = 0;
  FracArgs F = frac_args(c);
  State G = T; G.height = d_h;
  FracArgs Fg = F; Fg.n = total;
  hipLaunchKernelGGL(sz_k_frac_criterion, dim3(1), dim3(FRAC_TPB), 0, c->stream, G, Fg);
  hipLaunchKernelGGL(sz_k_frac_test, dim3(grid_for(std::max(N, 1), 256, 2048)), dim3(256), 0, c->stream, T, F);
  if (compact) hipLaunchKernelGGL(sz_k_frac_compact, dim3(1), dim3(FRAC_TPB), 0, c->stream, F);
  int found = 0, bad = 0;
  HIPCHK(c, hipMemcpyAsync(&found, &c->frac_d->count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  // ---- 3
  if (found < 0 || found > N) rc = SZ_E_CAPACITY;
  const int mine = (bad & FRT_BAD_RANGE ? FRT_BIT_RANGE : 0) | (bad & FRT_BAD_TWICE ? FRT_BIT_TWICE : 0) | (rc ? FRT_BIT_ERR : 0) | (found > 0 ? FRT_BIT_CAND : 0) | (my_tag ? FRT_BIT_TAG : 0);
  int all = 0;
  if ((rc = comm_agree_bits(c, mine, &all))) return rc;
  if (all & (FRT_BIT_RANGE | FRT_BIT_TWICE)) {
    c->err = std::string("tiled fracture criteria: the global numbers of the ranks (sz_tile_enable) are not 0 .. N_global - 1 once each: ") +
             (all & FRT_BIT_RANGE ? "one is out of range" : "one is held twice") + " (all ranks return together)";
    return SZ_E_STATE;
  }
  if (all & FRT_BIT_ERR) { if (!(mine & FRT_BIT_ERR)) c->err = "tiled fracture criteria: a rank reported a device error (this rank is clean; all ranks return together)"; return SZ_E_CAPACITY; }
  c->err.clear();
  *any_cand = (all & FRT_BIT_CAND) != 0; *any_tag = (all & FRT_BIT_TAG) != 0; *n_owned = found;
  return SZ_OK;
}
}  // namespace
int sz_tile_fracture_candidates(sz_ctx* c, int32_t* n_global, int32_t* n_owned, int32_t* rows, int64_t* gidx) {
  if (n_global) *n_global = 0;
  if (n_owned) *n_owned = 0;
  if (!c || !n_global || !n_owned) return SZ_E_ARG;
  if (int rc = tiled_ready(c, "sz_tile_fracture_candidates")) return rc;
  if (c->frac_kind == SZ_FRAC_OFF) { c->err = "sz_tile_fracture_candidates: no fracture criterion set (sz_set_fracture)"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  int any = 0, tag = 0, mine = 0, per_rank[64] = { 0 };
  if (int rc = tile_frac_pass(c, false, true, &any, &tag, &mine)) return rc;
  if (int rc = comm_gather_int(c, mine, per_rank)) return rc;
  long long total = 0;
  for (int r = 0; r < c->comm_n; r++) total += per_rank[r];
  if (mine > 0 && (rows || gidx)) {
    std::vector<int> h((size_t)mine);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->frac_idx, (size_t)mine * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < mine; k++) {
      if (h[k] < 0 || h[k] >= (int)c->tile_gidx.size()) { c->err = "sz_tile_fracture_candidates: bad candidate row"; return SZ_E_HIP; }
      if (rows) rows[k] = h[k];
      if (gidx) gidx[k] = c->tile_gidx[h[k]];
    }
  }
  *n_global = (int32_t)total; *n_owned = mine;
  return SZ_OK;
}

// ---------------------------------------------------------------- the welding overlap table on a tiled context (sz_weld_tile.hpp)
namespace {
// The overlap table (weld_pass) over the ONE global floe list whose rows live on the ranks' tiles: collective, over the parents with ghosts
// detached.  Every rank ends with the single context's whole table in global numbers (c->weldt_i / _j / _a), to the bit.  The collectives, the
// same on every rank whatever it holds:
//   1. the gather of the owned counts; a rank that cannot take part (device error bits, ghosts in the list, no grid) sends its error code in
//      place of its count, and all ranks return it together
//   2. the all-gather of the candidate records, one per owned row (ListGather)
//   3. the agreement on: a global number out of range or met twice, a device error, "my pair arrays are too small" -- all ranks then grow what
//      they must and run the pass again together
//   4. the gather of {wanted rings, largest wanted ring} per rank, then the all-gather of the ring records, the slot sized by the largest
//      wanted ring of any rank (not by a rank's own max_ring: ADVICE.md, the halo_ring item)
//   5. the gather of the table counts (an error code in place of the count, as in 1), then the all-gather of the {key, area} entries
//   6. the agreement on: a device error, "the table is not empty", and my_tag -- "my stop word stood at the segment's last step", news to
//      the peers behind the list-based driver (see tile_frac_pass)
// In front of 2, 4 and 5's all-gather the ranks gather the code of what each prepared alone (scratch memory), so a rank that fails there takes the
// others with it instead of leaving them in the gather.  A failure of the HIP runtime or of the channel itself is returned at once, as everywhere
// in the library.  Nothing of the floes changes in a pass: it writes its own scratch (c->weldt_allocs, kept between passes) and the sort's.
constexpr int WT_BIT_RANGE = 1, WT_BIT_TWICE = 2, WT_BIT_ERR = 4, WT_BIT_GROW = 8, WT_BIT_TABLE = 16, WT_BIT_TAG = 32;
int tile_weld_pass(sz_ctx* c, int nx, int ny, double max_area, bool my_tag, int* ntable, int* any_tag) {
  *ntable = 0; *any_tag = 0;
  State& S = c->S;
  const int n = c->comm_n, me = c->comm_rank;
  constexpr const char* who = "tiled welding overlaps";
  // ---- 1
  int rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  if (!rc && c->hostM != c->hostN) rc = SZ_E_STATE;
  if (!rc && (!c->have_domain || !c->have_fields || !(S.gxf > S.gx0) || !(S.gyf > S.gy0))) { c->err = "tiled welding overlaps: the bins need the domain's boundary kinds and the grid extents (sz_set_domain, sz_set_fields)"; rc = SZ_E_STATE; }
  const int N = c->hostN;
  c->weldt_cnt.assign(64, 0);
  int* const cnt = c->weldt_cnt.data();
  if (const int r2 = comm_gather_int(c, rc ? rc : N, cnt)) return r2;
  for (int r = 0; r < n; r++) if (cnt[r] < 0) {
    if (cnt[r] == SZ_E_STATE && !(rc && r == c->comm_rank && c->hostM == c->hostN)) c->err = "tiled welding overlaps: rank " + std::to_string(r) + " has ghosts in its list (the pass runs over the parents alone) or no grid";
    else if (!rc) c->err = "tiled welding overlaps: rank " + std::to_string(r) + " reported a device error (this rank is clean; all ranks return together)";
    return cnt[r];
  }
  long long Ng64 = 0;
  for (int r = 0; r < n; r++) Ng64 += cnt[r];
  // (the same sums on every rank)
  if (Ng64 <= 0) { c->err = "tiled welding overlaps: no floes"; return SZ_E_STATE; }
  if (Ng64 > 0x3fffffff) { c->err = "tiled welding overlaps: more than 2^30 floes"; return SZ_E_CAPACITY; }
  const int Ng = (int)Ng64;
  if ((long double)nx * (long double)ny * (long double)Ng * (long double)Ng >= 9.0e18L) { c->err = "tiled welding overlaps: Nx * Ny * N^2 does not fit the 64-bit pair key"; return SZ_E_ARG; }
  world_rings(c);
  Pool& P = c->weldt_allocs;
  for (int round = 0;; round++) {
    reset_pool(P);
    // ---- 2: the scratch of this rank (the search cells take the most a field of Ng floes can need), then the candidates of the whole field
    ListGather LG(c, cnt, WTC_REC, 1);
    const int slots = LG.slots;
    const long long nslot = (long long)n * slots;
    const long long cell_max = std::max(4LL * Ng, 1024LL);
    const size_t cap = (size_t)std::max((long long)c->weldt_need, 8LL * N + 1024);
    int first = 0;
    WeldArgs W{};
    WeldTileDev* d_dev = nullptr; int *d_mark = nullptr, *d_wslot = nullptr, *d_src = nullptr, *cell_cnt = nullptr, *cell_ovf = nullptr, *cell_slots = nullptr, *cell_items = nullptr;
    double *d_bounds = nullptr, *d_trec = nullptr;
    rc = nslot > 0x3fffffff || cap > ((size_t)1 << 30) ? (int)SZ_E_CAPACITY : (int)SZ_OK;
    (void)(rc || (rc = LG.carve(c, P)) || (rc = dalloc(c, &d_dev, 1, P)) || (rc = dalloc(c, &W.d, 1, P)) || (rc = dalloc(c, &d_mark, (size_t)Ng, P)) || (rc = dalloc(c, &d_src, (size_t)Ng, P)) ||
           (rc = dalloc(c, &W.bin, (size_t)N + 1, P)) || (rc = dalloc(c, &d_wslot, (size_t)N + 1, P)) || (rc = dalloc(c, &d_bounds, 8, P)) ||
           (rc = dalloc(c, &cell_cnt, (size_t)cell_max + 1, P)) || (rc = dalloc(c, &cell_ovf, (size_t)cell_max + 1, P)) || (rc = dalloc(c, &cell_slots, (size_t)cell_max * CELL_K, P)) ||
           (rc = dalloc(c, &cell_items, (size_t)nslot + 1, P)) || (rc = dalloc(c, &W.keys_in, cap, P)) || (rc = dalloc(c, &W.keys, cap, P)) || (rc = dalloc(c, &W.area, cap, P)) ||
           (rc = dalloc(c, &W.retry, cap, P)) || (rc = dalloc(c, &d_trec, (size_t)WTT_REC * cap, P)));
    if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
    if (first) return first;
    c->weldt_bin = W.bin;
    W.n = Ng; W.nx = nx; W.ny = ny; W.cap = (int)cap; W.max_area = max_area;
    c->weldt_h = WeldTileDev{ 0ull, Ng, 0, 0, 0 }; c->weldt_hw = WeldDev{ Ng, 0, 0, 0 };
    HIPCHK(c, hipMemcpyAsync(d_dev, &c->weldt_h, sizeof(WeldTileDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(W.d, &c->weldt_hw, sizeof(WeldDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_mark, 0, (size_t)Ng * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(d_src, 0xff, (size_t)Ng * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(LG.d_rec, 0, (size_t)WTC_REC * slots * sizeof(double), c->stream));
    if ((rc = LG.upload_counts(c, cnt))) return rc;
    if (N > 0) hipLaunchKernelGGL(sz_k_weldt_pack, dim3(grid_for(N, 256, 2048)), dim3(256), 0, c->stream, S, N, nx, ny, max_area, LG.d_rec);
    if ((rc = LG.gather(c))) return rc;
    hipLaunchKernelGGL(sz_k_weldt_scan, dim3(grid_for(nslot, 256, 2048)), dim3(256), 0, c->stream, (const double*)LG.d_all, (const int*)LG.d_cnt, n, slots, Ng, d_mark, d_dev);
    HIPCHK(c, hipMemcpyAsync(&c->weldt_h, d_dev, sizeof(WeldTileDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int bad = c->weldt_h.bad;
    // ---- the pair search: cells of at least 2 max(rmax) over the gathered records (setup_grid's rule), indices clamped: no periodic wrap
    int npairs = 0, nwant = 0, maxring = 0;
    if (!bad) {
      double rm; { const long long b = (long long)c->weldt_h.rmax_bits; memcpy(&rm, &b, sizeof(rm)); }
      if (!(rm > 0.0)) rm = std::max(S.gxf - S.gx0, S.gyf - S.gy0);          // (no rmax anywhere: one cell)
      const double cmin = 2.0 * rm * (1.0 + 1e-9);
      long long ncx = std::max(1LL, (long long)std::floor(std::min((S.gxf - S.gx0) / cmin, 1e6)));
      long long ncy = std::max(1LL, (long long)std::floor(std::min((S.gyf - S.gy0) / cmin, 1e6)));
      while (ncx * ncy > cell_max) { ncx = std::max(1LL, ncx / 2); ncy = std::max(1LL, ncy / 2); }
      const int cells = (int)(ncx * ncy);
      double* g = c->weldt_h_grid;
      g[0] = S.gx0; g[1] = S.gy0; g[2] = (S.gxf - S.gx0) / (double)ncx; g[3] = (S.gyf - S.gy0) / (double)ncy; g[4] = (double)ncx; g[5] = (double)ncy; g[6] = 0.0; g[7] = 0.0;
      State T = S; T.step = 0;
      T.bounds = d_bounds; T.cell_cnt = cell_cnt; T.cell_slots = cell_slots; T.cell_ovf = cell_ovf; T.cell_items = cell_items;
      HIPCHK(c, hipMemcpyAsync(d_bounds, g, 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
      HIPCHK(c, hipMemsetAsync(cell_cnt, 0, ((size_t)cells + 1) * sizeof(int), c->stream));
      HIPCHK(c, hipMemsetAsync(cell_ovf, 0, ((size_t)cells + 1) * sizeof(int), c->stream));
      hipLaunchKernelGGL(sz_k_weldt_insert, dim3(grid_for(nslot, 256, 2048)), dim3(256), 0, c->stream, T, (const double*)LG.d_all, (const int*)LG.d_cnt, n, slots, (const WeldTileDev*)d_dev);
      if (N > 0) hipLaunchKernelGGL(sz_k_weldt_pairs, dim3(grid_for(N, 256, 2048)), dim3(256), 0, c->stream, T, W, (const double*)LG.d_all, slots, me, N, d_dev, W.bin, d_wslot, d_src);
      HIPCHK(c, hipMemcpyAsync(&c->weldt_h, d_dev, sizeof(WeldTileDev), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(&c->weldt_hw, W.d, sizeof(WeldDev), hipMemcpyDeviceToHost, c->stream));
    }
    rc = sync_and_check(c);
    if (rc == SZ_E_HIP) return rc;
    if (!bad) { npairs = c->weldt_hw.npairs; nwant = c->weldt_h.nwant; maxring = c->weldt_h.maxring; }
    if (npairs < 0 || nwant < 0 || nwant > N || nwant >= (1 << 22) || maxring < 0) rc = SZ_E_CAPACITY;
    const bool grow = !rc && npairs > (int)cap;
    // ---- 3
    const int mine = (bad & WT_BAD_RANGE ? WT_BIT_RANGE : 0) | (bad & WT_BAD_TWICE ? WT_BIT_TWICE : 0) | (rc ? WT_BIT_ERR : 0) | (grow ? WT_BIT_GROW : 0);
    int all = 0;
    if ((rc = comm_agree_bits(c, mine, &all))) return rc;
    if (all & (WT_BIT_RANGE | WT_BIT_TWICE)) {
      c->err = std::string("tiled welding overlaps: the global numbers of the ranks (sz_tile_enable) are not 0 .. N_global - 1 once each: ") +
               (all & WT_BIT_RANGE ? "one is out of range" : "one is held twice") + " (all ranks return together)";
      return SZ_E_STATE;
    }
    if (all & WT_BIT_ERR) { if (!(mine & WT_BIT_ERR)) c->err = "tiled welding overlaps: a rank reported a device error (this rank is clean; all ranks return together)"; return SZ_E_CAPACITY; }
    c->err.clear();
    if (all & WT_BIT_GROW) {          // the pair arrays grow like the other lists; nothing is truncated
      if (round > 0) { c->err = "tiled welding overlaps: the pair arrays did not grow enough"; return SZ_E_CAPACITY; }
      if (grow) c->weldt_need = npairs + npairs / 4;
      continue;
    }
    // ---- 4: the rings the owners of cross-rank pairs asked for
    int word[64] = { 0 }, wcnt[64] = { 0 }, ringcap = 4;
    if ((rc = comm_gather_int(c, nwant << 8 | std::min(maxring, 255), word))) return rc;
    for (int r = 0; r < n; r++) { wcnt[r] = word[r] >> 8; ringcap = std::max(ringcap, ((word[r] & 255) + 1) & ~1); }
    const int RW = WTR_HEAD + 2 * ringcap;
    ListGather LR(c, wcnt, RW, 1);
    rc = (long long)n * LR.slots > 0x3fffffff ? (int)SZ_E_CAPACITY : LR.carve(c, P);
    if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
    if (first) return first;
    if ((rc = LR.upload_counts(c, wcnt))) return rc;
    if (nwant > 0) hipLaunchKernelGGL(sz_k_weldt_rings, dim3(grid_for((long long)N * 64, 256, 2048)), dim3(256), 0, c->stream, S, N, (const int*)d_wslot, RW, LR.d_rec);
    if ((rc = LR.gather(c))) return rc;
    hipLaunchKernelGGL(sz_k_weldt_src, dim3(grid_for((long long)n * LR.slots, 256, 2048)), dim3(256), 0, c->stream, (const double*)LR.d_all, (const int*)LR.d_cnt, n, LR.slots, RW, me, Ng, d_src);
    // ---- the clip: the single context's kernels over this rank's pairs, sorted by key
    c->weldt_hw.ntable = 0;
    if (npairs > 0) {
      const int Pn = npairs;
      const WeldTileRings RS{ d_src, LR.d_all, RW };
      const unsigned long long top = (unsigned long long)nx * ny * (unsigned long long)Ng * (unsigned long long)Ng;
      unsigned bits = 1; while (bits < 64 && (top >> bits)) bits++;
      size_t tmp_bytes = 0;
      HIPCHK(c, rocprim::radix_sort_keys(nullptr, tmp_bytes, W.keys_in, W.keys, (size_t)Pn, 0u, bits, c->stream));
      if (tmp_bytes > c->weld_tmp_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->weld_tmp); c->weld_tmp = nullptr; c->weld_tmp_bytes = 0;
        HIPCHK(c, hipMalloc(&c->weld_tmp, tmp_bytes + tmp_bytes / 2));
        c->weld_tmp_bytes = tmp_bytes + tmp_bytes / 2;
      }
      HIPCHK(c, rocprim::radix_sort_keys(c->weld_tmp, tmp_bytes, W.keys_in, W.keys, (size_t)Pn, 0u, bits, c->stream));
      hipLaunchKernelGGL((sz_k_weld_area<WELD_G0, WELD_CAP0, WELD_KC0, WELD_RC0, WELD_RM0, 0, WeldTileRings>), dim3(grid_for(Pn, 64 / WELD_G0, 1 << 16)), dim3(64), 0, c->stream, S, W, Pn, RS);
      hipLaunchKernelGGL((sz_k_weld_area<WELD_G1, WELD_CAP1, WELD_KC1, WELD_RC1, WELD_RM1, 1, WeldTileRings>), dim3(grid_for(Pn, 1, 512)), dim3(64), 0, c->stream, S, W, Pn, RS);
      hipLaunchKernelGGL(sz_k_weldt_table, dim3(1), dim3(WELD_TPB), 0, c->stream, W, Pn, d_trec);
      HIPCHK(c, hipMemcpyAsync(&c->weldt_hw, W.d, sizeof(WeldDev), hipMemcpyDeviceToHost, c->stream));
    }
    rc = sync_and_check(c);
    if (rc == SZ_E_HIP) return rc;
    const int nt = c->weldt_hw.ntable;
    if (!rc && (nt < 0 || nt > npairs)) rc = SZ_E_CAPACITY;
    // ---- 5: one table everywhere
    int tcnt[64] = { 0 };
    if (const int r2 = comm_gather_int(c, rc ? rc : nt, tcnt)) return r2;
    for (int r = 0; r < n; r++) if (tcnt[r] < 0) {
      if (!rc) c->err = "tiled welding overlaps: rank " + std::to_string(r) + " reported a device error (this rank is clean; all ranks return together)";
      return tcnt[r];
    }
    ListGather LT(c, tcnt, WTT_REC, 1);
    const long long total = LT.total;
    long long *d_ti = nullptr, *d_tj = nullptr; double* d_ta = nullptr;
    rc = total > 0x3fffffff || (long long)n * LT.slots > 0x3fffffff ? (int)SZ_E_CAPACITY : (int)SZ_OK;
    (void)(rc || (rc = LT.carve(c, P)) || (rc = dalloc(c, &d_ti, (size_t)total + 1, P)) || (rc = dalloc(c, &d_tj, (size_t)total + 1, P)) || (rc = dalloc(c, &d_ta, (size_t)total + 1, P)));
    if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
    if (first) return first;
    if ((rc = LT.upload_counts(c, tcnt))) return rc;
    if (nt > 0) HIPCHK(c, hipMemcpyAsync(LT.d_rec, d_trec, (size_t)WTT_REC * nt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = LT.gather(c))) return rc;
    c->weldt_i.assign((size_t)total, 0); c->weldt_j.assign((size_t)total, 0); c->weldt_a.assign((size_t)total, 0.0);
    if (total > 0) {
      hipLaunchKernelGGL(sz_k_weldt_merge, dim3(grid_for((long long)n * LT.slots, 256, 2048)), dim3(256), 0, c->stream, (const double*)LT.d_all, (const int*)LT.d_cnt, n, LT.slots, Ng, d_ti, d_tj, d_ta);
      HIPCHK(c, hipMemcpyAsync(c->weldt_i.data(), d_ti, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(c->weldt_j.data(), d_tj, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipMemcpyAsync(c->weldt_a.data(), d_ta, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    rc = sync_and_check(c);
    if (rc == SZ_E_HIP) return rc;
    // ---- 6
    const int last = (rc ? WT_BIT_ERR : 0) | (total > 0 ? WT_BIT_TABLE : 0) | (my_tag ? WT_BIT_TAG : 0);
    if ((rc = comm_agree_bits(c, last, &all))) return rc;
    if (all & WT_BIT_ERR) { if (!(last & WT_BIT_ERR)) c->err = "tiled welding overlaps: a rank reported a device error (this rank is clean; all ranks return together)"; return SZ_E_CAPACITY; }
    c->err.clear();
    trim_pool(P);
    c->weldt_npairs = npairs;
    *ntable = (int)total; *any_tag = (all & WT_BIT_TAG) != 0;
    return SZ_OK;
  }
}
}  // namespace
int sz_tile_weld_overlaps(sz_ctx* c, int32_t nx, int32_t ny, double max_weld_area, int32_t* n, int32_t cap, int64_t* idx_i, int64_t* idx_j, double* inter_area) {
  if (n) *n = 0;
  if (!c || !n) return SZ_E_ARG;
  if (nx < 1 || ny < 1) { c->err = "sz_tile_weld_overlaps: Nx and Ny must be at least 1"; return SZ_E_ARG; }
  if (!(max_weld_area > 0.0)) { c->err = "sz_tile_weld_overlaps: max_weld_area must be positive"; return SZ_E_ARG; }
  if (int rc = tiled_ready(c, "sz_tile_weld_overlaps")) return rc;
  (void)hipSetDevice(c->device);
  int nt = 0, tag = 0;
  if (int rc = tile_weld_pass(c, nx, ny, max_weld_area, false, &nt, &tag)) return rc;
  *n = nt;
  if (!idx_i && !idx_j && !inter_area) return SZ_OK;
  if (cap < nt) { c->err = "sz_tile_weld_overlaps: cap is smaller than the table (*n)"; return SZ_E_ARG; }          // (the same table on every rank: with the same cap, the same answer)
  for (int k = 0; k < nt; k++) {
    if (idx_i) idx_i[k] = c->weldt_i[k];
    if (idx_j) idx_j[k] = c->weldt_j[k];
    if (inter_area) inter_area[k] = c->weldt_a[k];
  }
  return SZ_OK;
}
// per owned row the 0-based bin or -1, with the `break` of the global list (collective: it runs a pass)
int sz_tile_debug_weld_bins(sz_ctx* c, int32_t nx, int32_t ny, int32_t* bin) {
  if (!c || !bin || nx < 1 || ny < 1) return SZ_E_ARG;
  if (int rc = tiled_ready(c, "sz_tile_debug_weld_bins")) return rc;
  (void)hipSetDevice(c->device);
  int nt = 0, tag = 0;
  if (int rc = tile_weld_pass(c, nx, ny, INFINITY, false, &nt, &tag)) return rc;
  if (c->hostN > 0) HIPCHK(c, hipMemcpy(bin, c->weldt_bin, (size_t)c->hostN * sizeof(int), hipMemcpyDeviceToHost));
  return SZ_OK;
}
// the candidate pairs (before the clip) of the last pass, over all ranks (collective)
int sz_tile_debug_weld_npairs(sz_ctx* c, int64_t* n) {
  if (!c || !n) return SZ_E_ARG;
  *n = 0;
  if (int rc = tiled_ready(c, "sz_tile_debug_weld_npairs")) return rc;
  (void)hipSetDevice(c->device);
  int per_rank[64] = { 0 };
  if (int rc = comm_gather_int(c, c->weldt_npairs, per_rank)) return rc;
  for (int r = 0; r < c->comm_n; r++) *n += per_rank[r];
  return SZ_OK;
}

// ---------------------------------------------------------------- ridge / raft candidates on a tiled context (sz_ridgeraft_tile.hpp)
namespace {
// The candidate table (rr_pass) over the ONE global floe list whose rows live on the ranks' tiles: collective, in the MIDDLE of a step -- behind the
// first half of a split step (tile_step_body), the local list holding the owned floes, the halo floes and the ghosts of both with this step's
// rows.  Every rank ends with the single context's whole table in the single context's list numbers and order (c->rrt_i / _j / _k / _f), to the bit,
// with the draws of all ranks as an exact integer sum, and with the list number of each of its local rows (c->rrt_rownum).  DESIGN.md §9e, "tiled
// contexts": the owner of a row's root parent evaluates it; i < j is the comparison of the order keys.  The collectives, the same on every rank
// whatever it holds:
//   1. the all-gather of {error code, rows this rank found not active, owned floes}: a rank that cannot take part (device error bits) sends its
//      code and all ranks return it together.  Only where some rank has a row that is not active: the agreement on what each prepared alone, then
//      the all-gather of those rows' keys (the status of a row behind this step's collisions is its owner's word)
//   2. the all-gather of {error code, entries, ghost rows of owned root parents, draws}.  All counts zero entries: the table is empty on every
//      rank and the pass ends here -- two collectives on the path a step runs through
//   3. the agreement on what each prepared alone (scratch memory)
//   4. the all-gather of the ghost keys: sorted, they number the single context's ghosts (N_global + place)
//   5. the all-gather of the entry records, renamed on every rank (sz_k_rrt_rename) and ordered by ascending i, then by the emitting rank's row
//      order -- the single context's order, as one rank emits all the entries of a list row
//   6. the agreement on: a device error, a key that could not be renamed
// The entries are counted before their memory is carved: nothing is truncated, no second round.  Nothing of the floes changes in a pass.
int tile_rr_pass(sz_ctx* c, int* ntable, long long* draws) {
  *ntable = 0; *draws = 0;
  State& S = c->S;
  const int n = c->comm_n, me = c->comm_rank;
  constexpr const char* who = "tiled ridge / raft candidates";
  int h[C_COUNT] = { 0 };
  int rc = sync_and_check(c, h);
  if (rc == SZ_E_HIP) return rc;
  const int M = h[C_M], nown = h[C_NOWN], npar = h[C_N];
  if (!rc && (M < npar || npar < nown || nown < 0 || M > S.capM)) { c->err = "tiled ridge / raft candidates: bad list counts"; rc = SZ_E_HIP; }
  Pool& P = c->rrt_allocs;
  reset_pool(P);
  // ---- this rank alone: the rows by ascending key, the status of the rows it evaluates
  RrArgs A{}; RrTiled T{};
  RrTileDev* d_g = nullptr; long long* skey = nullptr; int *srow = nullptr, *iota = nullptr, *gflag = nullptr, *d_w = nullptr, *d_wall = nullptr;
  unsigned char* act = nullptr; double *inact = nullptr, *gkeys = nullptr;
  const size_t Mc = (size_t)std::max(M, 1);
  if (const int r2 = dalloc(c, &d_w, 4, P)) return r2;          // (the words of gathers 1 and 2: without them there is nothing to agree over)
  if (const int r2 = dalloc(c, &d_wall, 4 * 64, P)) return r2;
  if (!rc) (void)((rc = dalloc(c, &A.d, 1, P)) || (rc = dalloc(c, &A.cnt, Mc + 1, P)) || (rc = dalloc(c, &A.off, Mc + 1, P)) || (rc = dalloc(c, &d_g, 1, P)) ||
                  (rc = dalloc(c, &skey, Mc, P)) || (rc = dalloc(c, &srow, Mc, P)) || (rc = dalloc(c, &iota, Mc, P)) || (rc = dalloc(c, &gflag, Mc, P)) ||
                  (rc = dalloc(c, &act, Mc, P)) || (rc = dalloc(c, &inact, Mc, P)) || (rc = dalloc(c, &gkeys, Mc, P)));
  const int nb = grid_for(std::max(M, 1), 256, 2048);
  c->rrt_hg = RrTileDev{ 0, 0 };
  if (!rc) {
    A.m = M; A.cap = 0;
    A.min_ridge_h = c->rr_h[0]; A.max_floe_ridge_h = c->rr_h[1]; A.max_domain_ridge_h = c->rr_h[2]; A.max_floe_raft_h = c->rr_h[3]; A.max_domain_raft_h = c->rr_h[4];
    T.skey = skey; T.srow = srow; T.act = act; T.m = M; T.nown = nown; T.npar = npar;
    HIPCHK(c, hipMemsetAsync(A.d, 0, sizeof(RrDev), c->stream));
    HIPCHK(c, hipMemsetAsync(d_g, 0, sizeof(RrTileDev), c->stream));
    if (M > 0) {
      hipLaunchKernelGGL(sz_k_rrt_iota, dim3(nb), dim3(256), 0, c->stream, iota, M);
      size_t tmp_bytes = 0;
      HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const long long*)S.okey, skey, (const int*)iota, srow, (size_t)M, 0u, 43u, c->stream));
      if (tmp_bytes > c->weld_tmp_bytes) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->weld_tmp); c->weld_tmp = nullptr; c->weld_tmp_bytes = 0;
        HIPCHK(c, hipMalloc(&c->weld_tmp, tmp_bytes + tmp_bytes / 2));
        c->weld_tmp_bytes = tmp_bytes + tmp_bytes / 2;
      }
      HIPCHK(c, rocprim::radix_sort_pairs(c->weld_tmp, tmp_bytes, (const long long*)S.okey, skey, (const int*)iota, srow, (size_t)M, 0u, 43u, c->stream));
      hipLaunchKernelGGL(sz_k_rrt_active, dim3(nb), dim3(256), 0, c->stream, S, T, (const long long*)c->facc_buf, 1, act, inact, M, d_g, (const long long*)nullptr, 0);
    }
    HIPCHK(c, hipMemcpyAsync(&c->rrt_hg, d_g, sizeof(RrTileDev), hipMemcpyDeviceToHost, c->stream));
    rc = sync_and_check(c);
    if (rc == SZ_E_HIP) return rc;
    if (!rc && (c->rrt_hg.ninact < 0 || c->rrt_hg.ninact > M)) { c->err = "tiled ridge / raft candidates: bad count of rows that are not active"; rc = SZ_E_CAPACITY; }
  }
  // ---- 1
  std::vector<int> words((size_t)4 * 64, 0);
  auto gather_words = [&](int w0, int w1, int w2, int w3) -> int {
    int* hw = c->rrt_hw; hw[0] = w0; hw[1] = w1; hw[2] = w2; hw[3] = w3;
    HIPCHK(c, hipMemcpyAsync(d_w, hw, 4 * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (const int r2 = comm_allgather(c, d_w, d_wall, 4, NCCL_INT32, sizeof(int))) return r2;
    HIPCHK(c, hipMemcpyAsync(words.data(), d_wall, (size_t)4 * n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SZ_OK;
  };
  if (const int r2 = gather_words(rc, rc ? 0 : c->rrt_hg.ninact, nown, 0)) return r2;
  auto first_code = [&]() -> int {
    for (int r = 0; r < n; r++) if (words[(size_t)4 * r] < 0) {
      if (!rc) c->err = std::string(who) + ": rank " + std::to_string(r) + " reported a device error (this rank is clean; all ranks return together)";
      return words[(size_t)4 * r];
    }
    return 0;
  };
  if (const int code = first_code()) return code;
  long long Ng = 0, nin_all = 0;
  int icnt[64] = { 0 };
  for (int r = 0; r < n; r++) { icnt[r] = words[(size_t)4 * r + 1]; nin_all += icnt[r]; Ng += words[(size_t)4 * r + 2]; }
  int first = 0;
  long long* d_gin = nullptr;
  if (nin_all > 0) {
    ListGather LI(c, icnt, 1, 1);
    rc = nin_all > 0x3fffffff ? (int)SZ_E_CAPACITY : LI.carve(c, P);
    if (!rc) rc = dalloc(c, &d_gin, (size_t)nin_all, P);
    if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
    if (first) return first;
    if (icnt[me] > 0) HIPCHK(c, hipMemcpyAsync(LI.d_rec, inact, (size_t)icnt[me] * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = LI.gather(c))) return rc;
    std::vector<double> hall((size_t)LI.slots * n);
    HIPCHK(c, hipMemcpyAsync(hall.data(), LI.d_all, hall.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<long long> gin;
    for (int r = 0; r < n; r++) for (int k = 0; k < icnt[r]; k++) gin.push_back((long long)hall[(size_t)r * LI.slots + k]);
    std::sort(gin.begin(), gin.end());
    HIPCHK(c, hipMemcpyAsync(d_gin, gin.data(), gin.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (gin leaves the scope)
  }
  // ---- the count pass over the rows this rank evaluates
  c->rrt_hd = RrDev{ 0ull, 0, 0 };
  if (M > 0) {
    hipLaunchKernelGGL(sz_k_rrt_active, dim3(nb), dim3(256), 0, c->stream, S, T, (const long long*)c->facc_buf, 0, act, inact, M, d_g, (const long long*)d_gin, (int)nin_all);
    hipLaunchKernelGGL(sz_k_rrt_count, dim3(nb), dim3(256), 0, c->stream, S, A, T, gflag);
    hipLaunchKernelGGL(sz_k_rr_scan, dim3(1), dim3(RR_TPB), 0, c->stream, A);
    hipLaunchKernelGGL(sz_k_rrt_gscan, dim3(1), dim3(RR_TPB), 0, c->stream, S, (const int*)gflag, M, gkeys, M, d_g);
    HIPCHK(c, hipMemcpyAsync(&c->rrt_hd, A.d, sizeof(RrDev), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&c->rrt_hg, d_g, sizeof(RrTileDev), hipMemcpyDeviceToHost, c->stream));
  }
  rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  const int Tn = c->rrt_hd.total, Gn = c->rrt_hg.nghost;
  if (!rc && (Tn < 0 || (long long)Tn > (long long)M * S.rowcap || Gn < 0 || Gn > M || c->rrt_hd.draws > 2ull * (unsigned long long)std::max(M, 0))) {
    c->err = "tiled ridge / raft candidates: bad table count"; rc = SZ_E_CAPACITY;
  }
  // ---- 2
  if (const int r2 = gather_words(rc, rc ? 0 : Tn, rc ? 0 : Gn, rc ? 0 : (int)c->rrt_hd.draws)) return r2;
  if (const int code = first_code()) return code;
  c->err.clear();
  int tcnt[64] = { 0 }, gcnt[64] = { 0 }, tbase[64] = { 0 };
  long long total = 0, gtotal = 0, dsum = 0;
  for (int r = 0; r < n; r++) { tcnt[r] = words[(size_t)4 * r + 1]; gcnt[r] = words[(size_t)4 * r + 2]; tbase[r] = (int)std::min(total, (long long)0x3fffffff); total += tcnt[r]; gtotal += gcnt[r]; dsum += words[(size_t)4 * r + 3]; }
  *draws = dsum;
  c->rrt_i.clear(); c->rrt_j.clear(); c->rrt_k.clear(); c->rrt_f.clear(); c->rrt_rownum.clear(); c->rrt_rowkey.clear();
  if (total == 0) { trim_pool(P); return SZ_OK; }
  // ---- 3
  ListGather LK(c, gcnt, 1, 1), LE(c, tcnt, RRT_REC, 1);
  long long *d_gk = nullptr, *d_ti = nullptr, *d_tj = nullptr, *d_rownum = nullptr; int *d_tk = nullptr, *d_base = nullptr, *d_bad = nullptr; double* d_tf = nullptr;
  rc = total > 0x3fffffff || gtotal > 0x3fffffff || (long long)n * LE.slots > 0x3fffffff ? (int)SZ_E_CAPACITY : (int)SZ_OK;
  (void)(rc || (rc = LK.carve(c, P)) || (rc = LE.carve(c, P)) || (rc = dalloc(c, &d_gk, (size_t)gtotal + 1, P)) || (rc = dalloc(c, &d_ti, (size_t)total, P)) ||
         (rc = dalloc(c, &d_tj, (size_t)total, P)) || (rc = dalloc(c, &d_tk, (size_t)total, P)) || (rc = dalloc(c, &d_tf, (size_t)total, P)) ||
         (rc = dalloc(c, &d_rownum, Mc, P)) || (rc = dalloc(c, &d_base, 64, P)) || (rc = dalloc(c, &d_bad, 1, P)));
  if (const int r2 = comm_agree_rc(c, who, rc, &first)) return r2;
  if (first) return first;
  // ---- 4
  if (Gn > 0) HIPCHK(c, hipMemcpyAsync(LK.d_rec, gkeys, (size_t)Gn * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if ((rc = LK.gather(c))) return rc;
  {
    std::vector<double> hall((size_t)LK.slots * n);
    HIPCHK(c, hipMemcpyAsync(hall.data(), LK.d_all, hall.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<long long> gk;
    for (int r = 0; r < n; r++) for (int k = 0; k < gcnt[r]; k++) gk.push_back((long long)hall[(size_t)r * LK.slots + k]);
    std::sort(gk.begin(), gk.end());
    gk.erase(std::unique(gk.begin(), gk.end()), gk.end());          // (distinct already: one rank owns a ghost's root parent)
    gtotal = (long long)gk.size();
    if (gtotal) HIPCHK(c, hipMemcpyAsync(d_gk, gk.data(), gk.size() * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // ---- 5
  if ((rc = LE.upload_counts(c, tcnt))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_base, tbase, 64 * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_bad, 0, sizeof(int), c->stream));
  A.cap = Tn;
  if (Tn > 0) hipLaunchKernelGGL(sz_k_rrt_write, dim3(nb), dim3(256), 0, c->stream, S, A, T, LE.d_rec);
  if ((rc = LE.gather(c))) return rc;
  hipLaunchKernelGGL(sz_k_rrt_rename, dim3(grid_for((long long)n * LE.slots + M, 256, 2048)), dim3(256), 0, c->stream, S, (const double*)LE.d_all, (const int*)LE.d_cnt, (const int*)d_base, n, LE.slots,
                     (const long long*)d_gk, (int)gtotal, Ng, d_ti, d_tj, d_tk, d_tf, d_rownum, M, d_bad);
  std::vector<long long> ti((size_t)total), tj((size_t)total); std::vector<int> tk((size_t)total); std::vector<double> tf((size_t)total);
  c->rrt_rownum.assign((size_t)M, -1); c->rrt_hbad = 0;
  HIPCHK(c, hipMemcpyAsync(ti.data(), d_ti, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tj.data(), d_tj, (size_t)total * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tk.data(), d_tk, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tf.data(), d_tf, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (M > 0) HIPCHK(c, hipMemcpyAsync(c->rrt_rownum.data(), d_rownum, (size_t)M * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  c->rrt_rowkey.assign((size_t)M, 0);
  if (M > 0) HIPCHK(c, hipMemcpyAsync(c->rrt_rowkey.data(), S.okey, (size_t)M * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&c->rrt_hbad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  rc = sync_and_check(c);
  if (rc == SZ_E_HIP) return rc;
  // ---- 6
  int all = 0;
  if (const int r2 = comm_agree_bits(c, (rc ? 1 : 0) | (c->rrt_hbad ? 2 : 0), &all)) return r2;
  if (all & 1) { if (!rc) c->err = std::string(who) + ": a rank reported a device error (this rank is clean; all ranks return together)"; return SZ_E_CAPACITY; }
  if (all & 2) { c->err = std::string(who) + ": an entry names a ghost no rank owns (the ranks do not hold the same floes' bits)"; return SZ_E_STATE; }
  c->err.clear();
  // ascending i, then the emitting rank's row order (the gathered order: a stable sort keeps it)
  std::vector<int> ord((size_t)total);
  for (int k = 0; k < (int)total; k++) ord[k] = k;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return ti[a] < ti[b]; });
  c->rrt_i.resize((size_t)total); c->rrt_j.resize((size_t)total); c->rrt_k.resize((size_t)total); c->rrt_f.resize((size_t)total);
  for (int k = 0; k < (int)total; k++) { c->rrt_i[k] = ti[ord[k]]; c->rrt_j[k] = tj[ord[k]]; c->rrt_k[k] = tk[ord[k]]; c->rrt_f[k] = tf[ord[k]]; }
  trim_pool(P);
  *ntable = (int)total;
  return SZ_OK;
}
}  // namespace

// ---------------------------------------------------------------- the batch drivers of sz_tile_run
namespace {
// status.fuse_idx of a tiled context, in GLOBAL floe numbers: the order keys of the local rows of the step that ended the batch (owned
// floes: their global index; halo floes and ghosts: the step's key table), the replay of host_fuse_fixup in key order, and the partners
// renamed -- a ghost by its parent
int tile_fuse_replay(sz_ctx* c, const int* h, bool last_coupled) {
  int rc = gi_fetch(c); if (rc) return rc;
  const int M = h[C_N] + h[C_NGHOSTS];
  std::vector<long long> keys(M, 0);
  for (int i = 0; i < M; i++) keys[i] = i < c->hostN ? c->tile_gidx[i] : (i - c->hostN < (int)c->gi_keys.size() ? c->gi_keys[i - c->hostN] : ((long long)3 << 40) + i);
  rc = host_fuse_fixup(c, h, true, true, last_coupled, &keys);
  if (rc) return rc;
  const long long lim = (long long)1 << 40;
  for (int i = 0; i < c->hostN && i < (int)c->fuse_lists.size(); i++)
    for (int& v : c->fuse_lists[i]) { if (v < 0 || v >= (int)keys.size()) continue; long long key = keys[v]; if (key >= lim) key = (key & (lim - 1)) >> 2; v = (int)key; }
  return SZ_OK;
}
// The plan of a tiled batch of inline steps (sz_tile_run has checked what they need: collisions, the static grid, rings that fit the one-launch
// integrator, no two-way coupling).  The ghosts are made by whoever places the parent (integrator: owned floes, unpack: halo floes): inline
// ghosts without a candidate list.  Records and totals: plan_batch's rules.  A tile's own:
//  - rfree.  With peers and the tag stop a rank learns that a step was the batch's last only in the unpack of the NEXT one -- after its
//    integrator has made that step's ghosts over the rows of this one -- so the rows are then assembled inside every step (rows only); alone,
//    or in batches that run through (SZ_NO_STOP), once behind the batch.  (Moving walls do not enter the rule.)
//  - lean.  Not under SZ_SYNC_DEBUG (dbgsync: the stages run one by one), and not without the all-pairs headers (hdr_all): a pause must
//    reach every rank.
static BatchPlan plan_tile_batch(const sz_ctx* c, int nsteps, int flags, bool hdr_all, bool dbgsync) {
  BatchPlan p{};
  p.periodic = c->S.any_periodic_ew || c->S.any_periodic_ns;
  p.coll = p.sg = p.gi = true;
  p.user_stop = !(flags & SZ_NO_STOP);
  p.stop_mask = W_STOP | W_RETRYSTOP | W_PAUSED; p.own_first_ghosts = true;
  p.mixed = c->precision == 1;
  plan_records_totals(p, c, nsteps);
  p.set_rfree(p.facc_on && !(c->comm_n > 1 && p.user_stop));
  p.lean = lean_wanted(c) && !dbgsync && hdr_all;
  return p;
}
// sz_tile_run on the list-based steps of sz_tile_step
static int tile_run_listed(sz_ctx* c, int nsteps, int tstep0, int dt, int coupling_dt, int flags, int32_t* steps_done) {
  State& S = c->S; const int n = c->comm_n;
  // The tag stop of these steps (one-way coupling): the pack kernel's header records carry every rank's stop word to EVERY rank, the unpack
  // kernel of the next step reads them before that step has touched anything and ends the batch there (sz_k_halo_unpack), as in the inline
  // steps.  The forcings then run behind the unpack instead of beside the exchange: a rank must not compute the forcings of a step its
  // peers have already called off.  Two-way coupling across tiles (round 4): the same stop -- the steps behind it are enqueued and return at
  // once; their all-reduces of the per-cell sums still run on every rank (collectives must), on the sums of the step that ended the
  // batch, and sz_two_way_finish writes the ocean fields of that step once more: the same values.
  const bool stopping = !(flags & SZ_NO_STOP);
  S.stop_on_tags = stopping ? 1 : 0;
  HIPCHK(c, clear_stop_words(c, W_STOP | W_RETRYSTOP));
  for (int s = 0; s < nsteps; s++) {
    const int tstep = tstep0 + s;
    c->tile_dt = dt;
    S.step = stopping ? s + 1 : 0;
    if (int rc = rebox_if_due(c)) return rc;
    c->tile_since_box++;
    const bool coupling = coupling_at(flags, coupling_dt, tstep);
    tile_pack(c);
    // (the host's channel blocks: the forcings go to the device first and run while the host trades the regions)
    if (coupling && !stopping && n > 1 && c->host_transport) { int rc = sz_tile_forcing(c, tstep, coupling_dt, flags); if (rc) return rc; }
    { int rc = tile_exchange(c, stopping); if (rc) return rc; }
    // the forcings of the owned floes need nothing from the halo: they run beside the exchange
    if (coupling && !stopping && !(n > 1 && c->host_transport)) { int rc = sz_tile_forcing(c, tstep, coupling_dt, flags); if (rc) return rc; }
    if (n > 1 && hipStreamWaitEvent(c->stream, c->ev_recv, 0) != hipSuccess) { c->err = "hipStreamWaitEvent (halo exchange)"; return SZ_E_HIP; }
    int rc = tile_step_body(c, c->d_recv, n, c->halo_cap, tstep, dt, coupling_dt, flags); if (rc) return rc;
    if (c->two_way && coupling) {       // ice-on-ocean stress: per-cell partial sums, summed over the ranks, finished on every rank
      const size_t nc = 3 * c->tw_ncell;
      if (!c->d_tw_partial) { int r2 = dalloc(c, &c->d_tw_partial, nc, c->tw_part_allocs); if (r2) return r2; }
      if ((rc = sz_two_way_partial(c, c->d_tw_partial)) || (rc = sz_comm_allreduce(c, c->d_tw_partial, (int64_t)nc)) ||
          (rc = sz_two_way_finish(c, c->d_tw_partial, dt))) return rc;
    }
  }
  // (the ranks agree on the error word: a rank with a device error and a clean one return the same code)
  S.step = 0;
  int hl[C_COUNT] = { 0 };
  const int rce = tile_sync_agree(c, hl);
  c->fuse_lists.resize(c->hostM);
  const int done = stopping && hl[C_STOP] > 0 ? std::min(hl[C_STOP], (int)nsteps) : nsteps;
  c->tile_stop_raised = stopping ? hl[C_STOP] : 0;
  if (done < nsteps) { c->grid_live = false; c->gl_valid = false; }          // stopped early: cells and ghost-candidate lists belong to steps that did not come
  if (steps_done) *steps_done = done;
  return rce;
}
// sz_tile_run on the inline steps: the single context's (step_batch_three_launch with inline ghosts), plus the pack and unpack kernels and the
// exchange, and the restarts the ranks agree on
static int tile_run_inline(sz_ctx* c, int nsteps, int tstep0, int dt, int coupling_dt, int flags, int32_t* steps_done) {
  State& S = c->S; const int n = c->comm_n, me = c->comm_rank;
  // SZ_SYNC_DEBUG=1 (diagnosis of a faulting kernel): wait after every stage of every step and say so on stderr -- the last line names the stage
  const bool dbgsync = getenv("SZ_SYNC_DEBUG") != nullptr;
  const bool hdr_all = !(c->tile_hdr_neighbours && (flags & SZ_NO_STOP));      // (the A/B arm without the all-pairs headers: see tile_hdr_neighbours)
  const BatchPlan plan = plan_tile_batch(c, nsteps, flags, hdr_all, dbgsync);
  const bool periodic = plan.periodic, facc_on = plan.facc_on, rfree = plan.rfree;
  tile_cleanup(c);                                  // (the halo floes / ghosts a list-based call may have left attached)
  // the start of a batch as in sz_step, from the plan: stop words, cells, buffers, rings, the collision records of the owned floes (the halo
  // floes get theirs from the unpack kernel, ghosts from their maker), totals.  The periodic ghosts of the owned floes for the first step, and
  // the swap of parents that lie outside the domain, are this driver's: in the loop, BEHIND the first pack -- see there
  int gl0 = 0;
  if (int rc = batch_enter(c, plan, &gl0)) return rc;
  HIPCHK(c, hipMemsetAsync(S.galloc, 0, 32 * sizeof(unsigned long long), c->stream));
  // the forcing output set in use (see `beside` below): a way out before the end of the batch takes the columns back to set 0, as at entry
  struct FrcSets {
    sz_ctx* c; int cur; bool keep;
    void use(int set) { if (set != cur) { std::swap(c->S.fxOA, c->frc_alt[0]); std::swap(c->S.fyOA, c->frc_alt[1]); std::swap(c->S.trqOA, c->frc_alt[2]); std::swap(c->S.hflx, c->frc_alt[3]); cur = set; } }
    ~FrcSets() { if (!keep) use(0); }
  } frc{ c, 0, false };
  auto stage_done = [&](int s, const char* what) {
    if (!dbgsync) return;
    const hipError_t e = hipStreamSynchronize(c->stream);
    int h4[C_COUNT]; (void)hipMemcpy(h4, S.cnt, sizeof(h4), hipMemcpyDeviceToHost);
    fprintf(stderr, "[sz rank %d] step %d: %s done (%s) M=%d N=%d own=%d halo=%d ghosts=%d err=0x%x\n", me, s, what, hipGetErrorString(e), h4[C_M], h4[C_N], h4[C_NOWN], h4[C_NHALO], h4[C_NGHOSTS], h4[C_ERR]);
    fflush(stderr);
  };
  stage_done(-1, "seed");
  std::vector<signed char> fset((size_t)std::max(nsteps, 1), (signed char)-1);      // the output set the forcings of step s wrote (-1: none of this kind)
  auto last_set = [&](int upto) { int set = 0; for (int s2 = 0; s2 < upto; s2++) if (fset[s2] >= 0) set = fset[s2]; return set; };      // (of steps [0, upto); 0: as at entry)
  // The largest narrow variant is left out of the steps until an item needs it, as in sz_step (-4 us and a launch boundary per step).  A
  // rank whose narrow phase meets such an item pauses inside that step (C_RETRYSTOP); its pause rides in the header records of the next
  // exchange (sz_k_halo_pack hdr[2]), whose unpack kernel stops every other rank before that step has touched anything.  After the sync
  // all ranks know the step: the rank that paused finishes it (the variant, the reduce, the integrator), and everybody runs the rest of
  // the batch again from the step after it, as a batch that starts there (cells, ghosts, records seeded anew) with the variant in.
  bool lean = plan.lean;
  std::vector<int> callid_of((size_t)std::max(nsteps, 1), 0);
  int h[C_COUNT]; int rc = SZ_OK;
  // The halo records of step s + 1 are written by the integrator of step s: the thread that has just placed the floe holds all a record
  // carries, and it packs the floe as the update left it, BEFORE the swap of a parent that left the domain -- the receiving rank makes
  // the ghosts with the routine the owner runs on the same values (see sz_k_integrate<true, true>).  A pack launch remains for the first
  // step of a batch (and the step a paused batch is taken up again at): it runs BEFORE the launch that makes the owned floes' first
  // ghosts and swaps the parents that lie outside, for the same reason.  New boxes for step s + 1 are therefore gathered before the
  // integrator of step s (from the positions that step started with; the drift margin covers the step in between).
  // fresh: this rank starts the (sub-)batch from its parents as they lie -- boxes, the first pack, the first ghosts.  After a pause only the
  // rank that paused does: it finished its step without making anything for the next one.  The others have that step behind them as any other
  // -- their integrator has made the next step's ghosts (from the parents BEFORE their swap, like the single context and the reference:
  // collisions.jl:942-950) and packed the halo records -- and simply take up the steps where the pause stopped them.
  bool fresh = true;
  for (int s_begin = 0;;) {
    S.retry_stop = lean ? 1 : 0;
    for (int s = s_begin; s < nsteps; s++) {
      const int tstep = tstep0 + s;
      S.step = s + 1; S.gslot = s & 1;
      c->tile_dt = dt;
      if (s == s_begin && s_begin == 0) {
        if (int rc = rebox_if_due(c)) return rc;
        stage_done(s, "rebox");
      }
      if (s == s_begin && fresh) {
        tile_pack(c);
        if (periodic) hipLaunchKernelGGL(sz_k_ghost_inline_seed, dim3(grid_for(S.capM, 256)), dim3(256), 0, c->stream, S, s & 1, c->hostN);
      }
      c->tile_since_box++;
      const bool coupling = coupling_at(flags, coupling_dt, tstep);
      stage_done(s, "pack");
      // With peers the forcings of the owned floes (they need nothing from the halo) run BESIDE the exchange -- on the main stream while the
      // communication stream trades the regions, before the host's channel blocks -- and the narrow launch carries no forcing tail; without
      // peers there is nothing to hide them behind and they ride in the narrow launch's tail as in sz_step.
      const bool beside = coupling && n > 1 && !(c->pmask >> SZ_K_FORCING & 1u);
      // (these forcings run before this rank knows whether a peer has asked for the batch to end at the previous step -- the unpack kernel
      //  below finds out.  They therefore write a SECOND set of the four output columns, alternating step by step, and the set the last
      //  step that really ran has written is made the context's at the end of the call: a batch that ends early leaves fxOA .. hflx of the
      //  step it ended with, as sz_step does.)
      if (beside) { frc.use(frc.cur ^ 1); fset[s] = (signed char)frc.cur; }
      if (beside && c->host_transport) stage_forcing(c, dt);
      { int rc = tile_exchange(c, hdr_all); if (rc) return rc; }
      if (beside && !c->host_transport) stage_forcing(c, dt);
      if (n > 1) {
        if (hipStreamWaitEvent(c->stream, c->ev_recv, 0) != hipSuccess) { c->err = "hipStreamWaitEvent (halo exchange)"; return SZ_E_HIP; }
        const long long slots = (long long)n * c->halo_cap;
        hipLaunchKernelGGL(sz_k_halo_unpack_inline, dim3(grid_for(slots, UNPACK_TPB, 1 << 20)), dim3(UNPACK_TPB), 0, c->stream, S, (const double*)c->d_recv, n, me, c->halo_cap,
                           S.gslot, c->hostN);
      }
      stage_done(s, "exchange + unpack");
      // the forcings that did not run beside the exchange: where sz_step puts them (forcing_fuse_mode)
      const int fmode = forcing_fuse_mode(c, coupling && !beside);
      if (coupling && !fmode && !beside) stage_forcing(c, dt);
      if (coupling) c->forcing_where = fmode;
      S.callid = ++c->callid; callid_of[s] = S.callid;
      if (facc_on && !(S.crec && S.maxnb <= MAXNB)) (void)hipMemsetAsync(c->facc_buf + (size_t)FX_WORDS * c->hostN, 0, (size_t)FX_WORDS * (S.capM - c->hostN) * sizeof(long long), c->stream);      // (see sz_step)
      if (dbgsync) {          // (the stages of collisions_step one by one)
        stage_broad(c, false, true, fmode == 1, false); stage_done(s, "neighbour search");
        stage_elems(c, true); stage_done(s, "element items");
        stage_narrow(c, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, fmode == 2 ? (c->precision == 1 ? 2 : 1) : 0, 0); stage_done(s, "narrow phase");
        stage_reduce(c, 1, -1, dt, 0); stage_done(s, "reduce");
      } else collisions_step(c, -1, dt, false, true, fmode, lean, false);
      const bool pack_next = s + 1 < nsteps;
      // (synchronises: once per gather interval; tile_since_box was incremented in this step, from 0 or more: the first step of the batch gathered if none had)
      if (pack_next) { if (int rc = rebox_if_due(c)) return rc; }
      const PackInl pk = tile_pack_args(c);
      c->acc_mode = integrator_acc_mode(facc_on, rfree, s + 1 == nsteps);
      stage_integrate(c, dt, false, coupling, true, -1, periodic && s + 1 < nsteps ? 1 - (s & 1) : -1, pack_next ? &pk : nullptr);
      stage_done(s, "integrate");
    }
    S.step = 0;
    if (rfree && nsteps > 0) stage_reduce(c, 1, -1, dt, 0, true);          // floe.interactions of the step that ended the batch
    c->tile_dirty = nsteps > 0;
    rc = sync_and_check(c, h);                     // (drops the halo floes and ghosts of the last step: tile_cleanup -- unless a step is paused)
    if (rc == SZ_E_HIP) return rc;
    // (the ranks agree on the error word BEFORE anybody decides to run steps again: a rank leaving on its own would hang the others)
    if (const int ra = tile_agree(c, rc)) return ra;
    // the step that was paused (here or on a peer) and the step a tag ended the batch at, as every rank sees them (comm_agree_steps)
    int sp = h[C_RETRYSTOP], st_all = h[C_STOP];
    { const int rc3 = comm_agree_steps(c, h[C_STOP], h[C_RETRYSTOP], &st_all, &sp); if (rc3) return rc3; }
    if (st_all > 0) h[C_STOP] = st_all;
    if (!lean || sp <= 0 || (st_all > 0 && st_all < sp)) break;
    // ---- a pause for the largest narrow variant in step sp
    const bool coupling_sp = coupling_at(flags, coupling_dt, tstep0 + sp - 1);
    HIPCHK(c, clear_stop_words(c, W_RETRYSTOP | W_PAUSED));
    S.retry_stop = 0; c->retry_seen = true; lean = false;
    // the forcing outputs as of step sp (the steps after it are run again).  BEFORE that step is finished: its integrator reads them, and
    // the steps enqueued behind it have gone on alternating the sets on the host while their forcing kernels returned at once
    frc.use(last_set(sp));
    for (int s2 = sp; s2 < nsteps; s2++) fset[s2] = -1;
    if (h[C_PAUSED] == sp) {          // this rank's step: the variant, then what the pause held back
      S.step = sp; S.gslot = (sp - 1) & 1; S.callid = callid_of[sp - 1];
      stage_narrow(c, dt, c->P.ff_max_overlap, c->P.fd_max_overlap, 0, 2);
      stage_reduce(c, 1, -1, dt, 0);
      c->acc_mode = integrator_acc_mode(facc_on, rfree, sp >= nsteps);
      stage_integrate(c, dt, false, coupling_sp, true, -1, -1);
      S.step = 0;
      if (rfree && sp >= nsteps) stage_reduce(c, 1, -1, dt, 0, true);
    }
    c->tile_dirty = true;
    if (sp >= nsteps || (st_all > 0 && st_all <= sp)) {               // (the last step of the batch -- or a peer tagged a floe in this very step: the batch ends with it -- nothing is run again)
      rc = sync_and_check(c, h);
      if (rc == SZ_E_HIP) return rc;
      if (st_all > 0) h[C_STOP] = h[C_STOP] > 0 ? std::min(h[C_STOP], st_all) : st_all;
      break;
    }
    // the rest of the batch again.  The rank that paused: from its floes as they lie after step sp (sz_step's capacity restart does the same);
    // the others: on from where the pause stopped them (see `fresh`)
    fresh = h[C_PAUSED] == sp;
    if (fresh) {
      tile_cleanup(c);
      c->grid_live = false; use_static_grid(c);
      HIPCHK(c, hipMemsetAsync(S.galloc, 0, 32 * sizeof(unsigned long long), c->stream));
      if (plan.cr) seed_records(c, S, c->hostN);
    } else {
      c->tile_dirty = false;          // (nothing to drop: the rows behind the owned floes are the NEXT step's ghosts)
      // the header records this rank's last pack left say "paused" (the launches enqueued behind the pause wrote the word there): not any more
      const size_t hstride = (size_t)(c->halo_cap + 1) * halo_rec(S);
      for (int d = 0; d < n; d++) HIPCHK(c, hipMemsetAsync(c->d_send + (size_t)d * hstride + 2, 0, sizeof(double), c->stream));
    }
    s_begin = sp;          // (the ghosts of that step: behind its pack, at the top of the loop)
  }
  if (const int ra = tile_agree(c, rc)) return ra;
  const int done = h[C_STOP] > 0 ? std::min(h[C_STOP], (int)nsteps) : nsteps;
  c->tile_stop_raised = plan.user_stop ? h[C_STOP] : 0;
  if (steps_done) *steps_done = done;
  frc.use(last_set(done)); frc.keep = true;          // the forcing outputs of the last step that ran (see `beside` above)
  if (done < nsteps) c->grid_live = false;          // stopped early: cells hold floes of a step that did not come
  c->inter_any = true; c->inter_lost = false;
  if (done > 0) { c->tile_inter_state = TILE_INTER_TABLE; c->tile_keys_n = h[C_NGHOSTS]; c->tile_keys_slot = (done - 1) & 1; }      // (the rows' ghost partners: that step's key table)
  // status.fuse_idx of the step that ended the batch (as sz_step: only that step can have produced fuse pairs)
  if (done > 0 && (h[C_STOP] > 0 || (flags & SZ_NO_STOP))) {
    c->gi_pending_n = h[C_NGHOSTS]; c->gi_pending_slot = (done - 1) & 1; c->gi_pending = true;
    rc = tile_fuse_replay(c, h, coupling_at(flags, coupling_dt, tstep0 + done - 1));
    c->gi_pending = false;
  }
  c->fuse_lists.resize(c->hostM);
  return rc;
}
// The second half of a split step (tile_step_body) and what settles it: the integrator, the halo rows and ghosts dropped, and the ranks' agreement
// on the error word and on "a floe of mine was tagged in this step" (*any_tag: of any rank)
static int tile_rr_second_half(sz_ctx* c, int tstep, int dt, int coupling_dt, int flags, int* any_tag) {
  State& S = c->S;
  *any_tag = 0;
  c->hostN = (int)c->tile_gidx.size();          // (the pass looked at the whole list; the host-side count of a tile is its owned floes)
  S.stop_on_tags = 1; S.step = 1;
  if (int rc = tile_step_body(c, nullptr, 0, 0, tstep, dt, coupling_dt, flags, TILE_STEP_SECOND)) return rc;
  S.step = 0;
  int hl[C_COUNT] = { 0 };
  const int rc = sync_and_check(c, hl);
  if (rc == SZ_E_HIP) return rc;
  int all = 0;
  if (const int rc2 = comm_agree_bits(c, (rc ? (c->last_err_bits ? c->last_err_bits & ~RRS_BIT_TAG : 1) : 0) | (hl[C_STOP] > 0 ? RRS_BIT_TAG : 0), &all)) return rc2;
  if (all & ~RRS_BIT_TAG) return SZ_E_CAPACITY;
  c->err.clear();
  *any_tag = (all & RRS_BIT_TAG) != 0;
  c->fuse_lists.resize(c->hostM);
  c->inter_any = true; c->inter_lost = false;
  return SZ_OK;
}
// A ridge / raft step of sz_tile_run (tstep % rr_dt == 0), a one-step segment of its own whichever driver runs the segments around it: pack,
// exchange, the first half of the list-based step, the candidate pass (tile_rr_pass: it starts with the agreement on the error word).  Empty
// table: the draws go to the batch's counter, the second half runs, *any_tag says whether a floe of any rank was tagged in the step.  Not empty:
// *pending = 1, the list keeps its halo rows and ghosts, and sz_tile_step_finish runs the second half.
static int tile_rr_step(sz_ctx* c, int tstep, int dt, int coupling_dt, int flags, int* pending, int* any_tag) {
  State& S = c->S; const int n = c->comm_n;
  *pending = 0; *any_tag = 0;
  BatchModes modes(c);
  world_rings(c);
  tile_cleanup(c);          // (halo rows and ghosts a host-driven step may have left attached)
  S.stop_on_tags = 1;
  HIPCHK(c, clear_stop_words(c, W_STOP | W_RETRYSTOP));
  c->tile_dt = dt;
  S.step = 1;
  if (int rc = rebox_if_due(c)) return rc;
  c->tile_since_box++;
  tile_pack(c);
  if (int rc = tile_exchange(c, true)) return rc;
  if (n > 1 && hipStreamWaitEvent(c->stream, c->ev_recv, 0) != hipSuccess) { c->err = "hipStreamWaitEvent (halo exchange)"; return SZ_E_HIP; }
  if (int rc = tile_step_body(c, c->d_recv, n, c->halo_cap, tstep, dt, coupling_dt, flags, TILE_STEP_FIRST)) return rc;
  S.step = 0;
  c->tile_dirty = false;          // (the pass must see the whole list: nothing is dropped before the second half)
  int nt = 0; long long nd = 0;
  if (int rc = tile_rr_pass(c, &nt, &nd)) { c->tile_dirty = true; return rc; }
  if (nt > 0) { *pending = 1; c->inter_any = true; c->inter_lost = false; return SZ_OK; }
  c->rr_draws += nd;
  return tile_rr_second_half(c, tstep, dt, coupling_dt, flags, any_tag);
}
}  // namespace
// the tiled recorder (sz_api.hip, behind the single context's: it is built from the same helpers): the record point, and the agreement on the
// writers' settings in front of a batch
static int tile_record(sz_ctx* c, int tstep, int* full);
static int tile_rec_agree_settings(sz_ctx* c);
namespace {
// The passes of the stop schedule (sz_stops.hpp) on a tiled context: collective, each agrees what it returns.  The only reader of tile_stop_raised.
struct TileStops {
  sz_ctx* c; int dt, coupling_dt, flags;
  bool agreed = false;          // the second half of a ridge / raft step has agreed the tag: settle() has nothing left to do
  // The steps of a tile are the single context's (sz_step): ghosts made by whoever places the parent (integrator: owned floes, unpack:
  // halo floes), forcings in the tail of the narrow launch, no ghost launch -- plus the pack and unpack kernels and the exchange.
  // Needs what the inline ghost maker needs (rings that fit the one-launch integrator, the static grid).  Otherwise: the list-based steps
  // of sz_tile_step.
  // Either driver runs under one scope of its own per segment; the ring maxima may shrink behind a removal pass, so each segment asks again.
  int drive(int len, int t0, int32_t* ran) {
    const bool inl = (flags & SZ_COLLISIONS_ON) && c->grid_ok && !c->two_way &&
                     std::max(c->max_ring, c->max_ring_tiled) <= MV_RING && ((flags & SZ_COUPLING_ON) == 0 || c->have_fields);
    BatchModes modes(c);
    return inl ? tile_run_inline(c, len, t0, dt, coupling_dt, flags, ran) : tile_run_listed(c, len, t0, dt, coupling_dt, flags, ran);
  }
  // a stop before the segment's last step is the same step on every rank; one on it is the driver's own word (sz_ctx.hpp, tile_stop_raised)
  int segment(int len, int t0, int* ran, int* tag) {
    c->tile_stop_raised = 0; agreed = false;
    const int rc = drive(len, t0, ran);
    *tag = !(flags & SZ_NO_STOP) && (*ran < len || c->tile_stop_raised == len);          // (a batch that runs through is only cut and recorded: no tag is looked at)
    return rc;
  }
  // pending = the lists keep their halo rows and ghosts, sz_tile_step_finish runs the rest
  int rr_step(int tstep, bool, int* pending, int* tag) {
    c->tile_stop_raised = 0;
    if (int rc = tile_rr_step(c, tstep, dt, coupling_dt, flags, pending, tag)) return rc;
    if (*pending) c->rr_pending = tstep;
    c->tile_stop_raised = *tag; agreed = true;          // (yet a welding pass of this step still runs: sz_stops.hpp)
    return SZ_OK;
  }
  int fracture(int, int, int* cand, int* tag) { int mine = 0; return tile_frac_pass(c, *tag != 0, false, cand, tag, &mine); }
  int weld(int set, int* nt, int* tag) { return tile_weld_pass(c, c->weld_nxs[set], c->weld_nys[set], c->weld_max_area, *tag != 0, nt, tag); }
  int settle(int* tag) {
    if (agreed) return SZ_OK;
    const int rc = comm_agree_bits(c, *tag ? RRS_BIT_TAG : 0, tag);
    if (!rc) c->err.clear();
    return rc;
  }
  // done = the next segment starts from the compacted tiles (boxes, halo capacities and peers are gathered again at its first exchange)
  int remove(int* ok) { int nr = 0, nd = 0; return tile_remove_pass(c, ok, &nr, &nd); }
  // write_data! of an output step (sz_record.hpp, "tiled contexts"): every rank's tile frame of its owned rows, the grid frames summed over the ranks
  int record(int tstep, int* full) { return tile_record(c, tstep, full); }
};
}  // namespace

// nsteps x timestep_sim! of a tiled run, collectively on every rank (same arguments everywhere)
int sz_tile_run(sz_ctx* c, int32_t nsteps, int32_t tstep0, int32_t dt, int32_t coupling_dt, int32_t flags, int32_t* steps_done) {
  if (steps_done) *steps_done = 0;
  if (c && !c->weld_dts.empty() && (c->comm_n < 1 || c->tile_margin <= 0)) { c->err = "tiled welding overlaps gather the candidates and rings over the ranks: needs sz_tile_setup and a communicator"; return SZ_E_STATE; }
  if (c && c->frac_kind != SZ_FRAC_OFF && (c->comm_n < 1 || c->tile_margin <= 0)) { c->err = "tiled fracture criteria gather the mean height over the ranks: needs sz_tile_setup and a communicator"; return SZ_E_STATE; }
  if (!c) return SZ_E_STATE;
  if (c->rr_pending >= 0) { c->err = "sz_tile_run: a ridge / raft step is pending (sz_ridgeraft_pending): sz_tile_step_finish runs its second half first"; return SZ_E_STATE; }
  if (c->rr_on && (c->comm_n < 1 || c->tile_margin <= 0)) { c->err = "tiled ridge / raft candidates gather the ghost keys and the entries over the ranks: needs sz_tile_setup and a communicator"; return SZ_E_STATE; }
  if (c->rec.any_tile && (c->comm_n < 1 || c->tile_margin <= 0)) { c->err = "tiled output writers gather the ranks' frame counts and sum the grid frames over the ranks: needs sz_tile_setup and a communicator"; return SZ_E_STATE; }
  if (int rc = tiled_ready(c, "sz_tile_run")) return rc;
  if (nsteps < 0) return SZ_E_ARG;
  c->rr_draws = 0;
  const bool frac = c->frac_kind != SZ_FRAC_OFF;
  const bool weld = !c->weld_dts.empty();
  const bool rr = c->rr_on && !(flags & SZ_NO_STOP) && nsteps > 0;
  if (rr && !(flags & SZ_COLLISIONS_ON)) { c->err = "sz_tile_run with ridge / raft set: the candidates are read from this step's interaction rows (SZ_COLLISIONS_ON)"; return SZ_E_STATE; }
  if (rr && (flags & SZ_COUPLING_ON) && !c->have_fields) { c->err = "sz_set_fields must be called before coupling"; return SZ_E_STATE; }
  if ((frac || weld || c->rr_on) && c->two_way) { c->err = std::string("tiled two-way coupling with ") + (frac ? "a fracture criterion set: its per-step all-reduce path has no tested stop: sz_set_fracture(SZ_FRAC_OFF)" : weld ? "welding set: its per-step all-reduce path has no tested stop: sz_set_welding(0)" : "ridge / raft set: its per-step all-reduce path has no tested stop: sz_set_ridgeraft(0)"); return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  // In batches that stop, with a criterion, welding, ridge / raft or removal set: the schedule of sz_stops.hpp over the passes of TileStops.
  // Two-way coupling across tiles has no tag stop of its own to hang a pass on: removal is not engaged there, the other three
  // refused above.  SZ_NO_STOP batches and contexts with none of the four set take the drivers as they are.
  TileStops ops = { c, dt, coupling_dt, flags };
  const bool rec = c->rec.any_tile && nsteps > 0;
  c->rec.full = false;
  if (rec) {
    // With an output writer set every batch takes the schedule, which then also cuts before the output steps and records their frames; a batch
    // that runs through (SZ_NO_STOP) carries the output intervals alone in its rules, as on the single context.
    const bool two_way = c->two_way;
    if (two_way) { c->err = "tiled two-way coupling with an output writer set: its per-step all-reduce path has no tested cut: sz_tile_set_floe_output / sz_tile_set_grid_output with dt_out = 0"; return SZ_E_STATE; }
    if (int rc = tile_rec_agree_settings(c)) return rc;
    StopRules rules = (flags & SZ_NO_STOP) ? StopRules{ 0, 0, nullptr, 0, false, false } : tile_stop_rules(*c);
    rules.out_dts = c->rec.dts; rules.n_out = 2 * REC_WRITERS;
    return run_with_stops(rules, ops, nsteps, tstep0, steps_done);
  }
  if ((!c->rm_on && !frac && !weld && !rr) || (flags & SZ_NO_STOP) || c->two_way || nsteps <= 0) return ops.drive(nsteps, tstep0, steps_done);
  return run_with_stops(tile_stop_rules(*c), ops, nsteps, tstep0, steps_done);
}

// ---------------------------------------------------------------- ridge / raft on a tiled context: the entry points of a pending stop
namespace {
int tile_rr_pending_ready(sz_ctx* c, const char* who) {
  if (int rc = tiled_ready(c, who)) return rc;
  if (!c->rr_on) { c->err = std::string(who) + ": ridge / raft is not set (sz_set_ridgeraft)"; return SZ_E_STATE; }
  if (c->rr_pending < 0) { c->err = std::string(who) + ": no ridge / raft step is pending (sz_tile_run stops there; sz_ridgeraft_pending)"; return SZ_E_STATE; }
  return SZ_OK;
}
}  // namespace
// the table of the pending step (collective: it runs the pass again), in the numbering and order of sz_ridgeraft_candidates
int sz_tile_ridgeraft_candidates(sz_ctx* c, int32_t* n, int32_t cap, int64_t* idx_i, int64_t* idx_j, int32_t* kind, double* frac, int64_t* n_draws) {
  if (n) *n = 0;
  if (n_draws) *n_draws = 0;
  if (!c || !n) return SZ_E_ARG;
  if (int rc = tile_rr_pending_ready(c, "sz_tile_ridgeraft_candidates")) return rc;
  (void)hipSetDevice(c->device);
  int nt = 0; long long nd = 0;
  if (int rc = tile_rr_pass(c, &nt, &nd)) return rc;
  *n = nt;
  if (n_draws) *n_draws = nd;
  if (!idx_i && !idx_j && !kind && !frac) return SZ_OK;
  if (cap < nt) { c->err = "sz_tile_ridgeraft_candidates: cap is smaller than the table (*n)"; return SZ_E_ARG; }          // (the same table on every rank: with the same cap, the same answer)
  for (int k = 0; k < nt; k++) {
    if (idx_i) idx_i[k] = c->rrt_i[k];
    if (idx_j) idx_j[k] = c->rrt_j[k];
    if (kind) kind[k] = c->rrt_k[k];
    if (frac) frac[k] = c->rrt_f[k];
  }
  return SZ_OK;
}
// the single context's list number of every local row of the pending step -- owned floes, halo floes, the ghosts of both (-1: a ghost no rank owns)
int sz_tile_list_numbers(sz_ctx* c, int64_t* out, int64_t cap) {
  if (!c || !out) return SZ_E_ARG;
  if (int rc = tile_rr_pending_ready(c, "sz_tile_list_numbers")) return rc;
  if (cap < (int64_t)c->rrt_rownum.size()) { c->err = "sz_tile_list_numbers: cap is smaller than the local list"; return SZ_E_ARG; }
  for (size_t k = 0; k < c->rrt_rownum.size(); k++) out[k] = c->rrt_rownum[k];
  return SZ_OK;
}
// ... and its order key (the partner column of a downloaded row holds key + 1)
int sz_tile_list_keys(sz_ctx* c, int64_t* out, int64_t cap) {
  if (!c || !out) return SZ_E_ARG;
  if (int rc = tile_rr_pending_ready(c, "sz_tile_list_keys")) return rc;
  if (cap < (int64_t)c->rrt_rowkey.size()) { c->err = "sz_tile_list_keys: cap is smaller than the local list"; return SZ_E_ARG; }
  for (size_t k = 0; k < c->rrt_rowkey.size(); k++) out[k] = c->rrt_rowkey[k];
  return SZ_OK;
}
// the second half of the pending step on what the device holds, collectively
int sz_tile_step_finish(sz_ctx* c, int32_t tstep, int32_t dt, int32_t coupling_dt, int32_t flags) {
  if (!c) return SZ_E_ARG;
  if (c->rr_pending < 0) { c->err = "sz_tile_step_finish: no ridge / raft step is pending"; return SZ_E_STATE; }
  if (tstep != c->rr_pending) { c->err = "sz_tile_step_finish: tstep is not the pending timestep (sz_ridgeraft_pending)"; return SZ_E_ARG; }
  if (int rc = tiled_ready(c, "sz_tile_step_finish")) return rc;
  if ((flags & SZ_COUPLING_ON) && !c->have_fields) { c->err = "sz_set_fields must be called before coupling"; return SZ_E_STATE; }
  (void)hipSetDevice(c->device);
  BatchModes modes(c);
  int tag = 0;
  if (int rc = tile_rr_second_half(c, tstep, dt, coupling_dt, flags, &tag)) return rc;
  c->rr_pending = -1;
  c->tile_stop_raised = tag ? 1 : 0;
  return SZ_OK;
}

/*
 * subzero_hip.h — C-ABI of libsubzero_hip.so, the MI355X (gfx950) engine for Subzero.jl's
 * per-timestep collision / forcing / rigid-body-update path.
 *
 * This is the drop-in boundary: a Julia shim or any other host
 * binds exactly these symbols with @ccall / ctypes / cgo.  Plain pointers and sizes only; no
 * exceptions cross the boundary.  Every int-returning call returns 0 on success and a negative
 * SZ_E_* code on failure (text via sz_last_error).  All calls are synchronous at return and
 * must come from one host thread per context.  The caller owns every host buffer; the library
 * keeps no host pointer after a call returns.
 *
 * Reference interfaces replaced (paths relative to the Subzero.jl repository):
 *   sz_add_ghosts                 <- add_ghosts!(floes, domain)            src/physical_processes/collisions.jl:1060-1174
 *   sz_timestep_collisions        <- timestep_collisions!(floes, n_init_floes, domain, consts, Δt,
 *                                    collision_settings, spinlock)          collisions.jl:734-864
 *   sz_collide_pairs              <- floe_floe_interaction!(ifloe, i, jfloe, j, consts, Δt,
 *                                    max_overlap)                           collisions.jl:347-408
 *   sz_collide_domain             <- floe_domain_interaction!(floe, domain, consts, Δt,
 *                                    max_overlap)                           collisions.jl:594-662
 *   sz_remove_ghosts              <- ghost-row deletion in timestep_sim!    src/simulation_components/simulation.jl:138-144
 *   sz_remove_floes               <- remove_floes!(floes, grid, domain, dissolved, floe_settings), where simplify_floes!
 *                                    reduces to it                         src/physical_processes/simplification.jl:279-314
 *   sz_download_rows /            <- what the host-side topology changes do to the floe list: deleteat!, assignment in place,
 *   sz_splice_floes                  append! (fracture_floes!, fuse / replace_floe!, ridging and rafting, smoothing), on the rows
 *                                    they name; the floes themselves are still made by the reference on the host
 *   sz_tile_download_rows /       <- the same list edits on a tiled (multi-GPU) context, stated once in global floe numbers
 *   sz_tile_splice_floes             with the same arguments on every rank
 *   sz_ridgeraft_rows /           <- the rows timestep_ridging_rafting! can touch, and what timestep_sim! does to the list behind it:
 *   sz_download_list_rows /          deleteat!(floes, n_init_floes + 1 : end), append!(floes, pieces)
 *   sz_splice_parents                                                       src/simulation_components/simulation.jl:121-147
 *   sz_timestep_coupling          <- timestep_coupling!(model, Δt, consts, coupling_settings,
 *                                    floe_settings), one-way part           src/physical_processes/coupling.jl:1705-1738
 *   sz_timestep_floe_properties   <- timestep_floe_properties!(floes, tstep, Δt, floe_settings)
 *                                                                           src/physical_processes/update_floe.jl:469-551
 *   sz_step                       <- timestep_sim!(sim, tstep), hot-path processes only,
 *                                    state resident in HBM between steps   simulation.jl:94-170
 *   sz_params                     <- Constants (simulation.jl:5-18), CollisionSettings
 *                                    (process_settings.jl:183-187), FloeSettings (:25-32),
 *                                    DecayAreaScaledCalculator.λ (stress_calculators.jl:82),
 *                                    CouplingSettings.Δd (process_settings.jl:133-137)
 *   sz_floe_columns               <- the hot columns of StructArray{Floe{Float64}} (src/simulation_components/floe.jl:24-77)
 *
 * Index conventions: all indices in this API are 0-based, EXCEPT the `floeidx` column (column 0)
 * of interaction rows, which holds the partner exactly as the reference stores it
 * (collisions.jl:297): 1-based floe index as a double, -1/-2/-3/-4 for the N/S/E/W boundary,
 * -(4+k) for topography element k (1-based).
 * Interaction rows are 7 doubles, row-major: floeidx, xforce, yforce, xpoint, ypoint, torque,
 * overlap (floe.jl:102-110).
 * 2x2 tensors are 4 doubles per floe in the order 11, 12, 21, 22.
 */
#ifndef SUBZERO_HIP_H
#define SUBZERO_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sz_ctx sz_ctx;

enum { SZ_OK = 0, SZ_E_HIP = -1, SZ_E_ARG = -2, SZ_E_CAPACITY = -3, SZ_E_STATE = -4, SZ_E_NODEVICE = -5 };
enum { SZ_OPEN = 0, SZ_PERIODIC = 1, SZ_COLLISION = 2, SZ_MOVING = 3 };       /* boundary kinds  */
enum { SZ_NORTH = 0, SZ_SOUTH = 1, SZ_EAST = 2, SZ_WEST = 3 };                /* boundary order  */
enum { SZ_ACTIVE = 1, SZ_REMOVE = 2, SZ_FUSE = 3 };                           /* floe.jl:8-12    */
/* process switches for sz_step (CollisionSettings.collisions_on, CouplingSettings.coupling_on) */
enum { SZ_COLLISIONS_ON = 1, SZ_COUPLING_ON = 2,
       SZ_NO_STOP = 4 };   /* sz_step: run all nsteps even when a floe gets tagged remove / fuse (departs from the reference,
                              which runs simplify_floes! after every step: measurement and soak runs only) */

typedef struct {
  double E, nu, mu, rho_o, rho_a, Cd_io, Cd_ia, f, turn_theta;
  double floe_floe_max_overlap, floe_domain_max_overlap;
  double rho_i, max_floe_height, maximum_xi, lambda;
  int32_t coupling_dd;
  int32_t _pad;
} sz_params;

/* Host-side view of the floe columns.  Scalar columns have one entry per floe (M entries);
   ragged columns are CSR.  Rings are closed (last point == first).  NULL columns are read as
   zeros on upload and skipped on download. */
typedef struct {
  double *cx, *cy, *rmax, *area, *height, *mass, *moment, *alpha, *u, *v, *xi;
  double *p_dxdt, *p_dydt, *p_dalphadt, *p_dudt, *p_dvdt, *p_dxidt;
  double *fxOA, *fyOA, *trqOA, *hflx_factor, *overarea;
  double *coll_fx, *coll_fy, *coll_trq;
  double *stress_accum, *stress_instant, *strain;        /* 4 per floe */
  int64_t *id, *ghost_id;
  int32_t *status;
  int32_t *vert_off;  double *vx, *vy;                   /* M+1 offsets, closed rings   */
  int32_t *sub_off;   double *sx, *sy;                   /* sub-floe points, centred    */
  int32_t *ghost_off; int32_t *ghost_idx;                /* parent -> ghost rows        */
} sz_floe_columns;

typedef struct {
  int64_t M, N;                 /* floes incl. ghosts / parents                              */
  int64_t n_ring_points;        /* V_M                                                       */
  int64_t n_sub_points;         /* S                                                         */
  int64_t n_pairs;              /* P: pairs that reached the narrow phase in the last step   */
  int64_t n_pair_ring_points;   /* sum over the pairs the narrow phase ran of both rings' point counts */
  int64_t n_pair_rows;          /* C: floe-floe contact rows before mirroring                */
  int64_t n_elem_items;         /* floe-boundary / floe-topography clips                     */
  int64_t n_elem_rows;          /* C_b                                                       */
  int64_t n_inter_rows;         /* total interaction rows after mirror + ghost fold          */
  int64_t n_ghosts;             /* G                                                         */
  int64_t warn_height, warn_force, warn_vel, warn_xi;   /* update_floe.jl guards             */
  int64_t n_trace_fail;         /* clip traces abandoned (self-intersecting input / round-off), cumulative */
  int64_t n_halo;               /* halo floes received in the last tiled step */
  int64_t n_pairs_clipped;      /* pairs with overlapping ring boxes: the pair items the narrow phase ran */
  int64_t n_status_remove;      /* floes tagged remove / fuse: when both are zero the host-side simplify_floes!  */
  int64_t n_status_fuse;        /* (simulation.jl:206) has no removal or fusion to do and needs no download       */
  int64_t n_retry;              /* narrow-phase items redone by the largest kernel variant (working set overflow), cumulative */
  /* cumulative since the last sz_profile_reset: what the narrow phase did over a window of steps (bench.py prices the
     dominant kernel's algorithmic bytes with the counts of the very launches whose time it averages) */
  int64_t acc_narrow_launches;  /* launches of the first narrow variant (= collision steps)                    */
  int64_t acc_pair_items;       /* pair items run (pairs whose ring boxes overlap)                              */
  int64_t acc_pair_ring_points; /* sum over those items of both rings' point counts                              */
  int64_t acc_pair_rows;        /* floe-floe contact rows before mirroring                                       */
  int64_t acc_elem_items;       /* floe-boundary / floe-topography items run                                     */
  int64_t acc_elem_rows;
  int64_t acc_dir_checks;       /* direction checks of calc_normal_force (collisions.jl:58-68) run ...                          */
  int64_t acc_dir_checks_certified; /* ... of which settled from the crossing detection of the translated polygon alone (no second clip) */
} sz_stats;

/* kernel classes for sz_kernel_time_ms */
enum { SZ_K_GHOSTS = 0, SZ_K_BROAD = 1, SZ_K_NARROW = 2, SZ_K_REDUCE = 3, SZ_K_FORCING = 4,
       SZ_K_INTEGRATE = 5, SZ_K_COUNT = 6 };

/* ---- lifetime */
sz_ctx     *sz_create(int device_id);            /* NULL if no HIP device / allocation failure */
void        sz_destroy(sz_ctx *ctx);
const char *sz_last_error(const sz_ctx *ctx);
const char *sz_version(void);

/* ---- static inputs */
int sz_set_params(sz_ctx *ctx, const sz_params *p);
/* boundaries in the order N, S, E, W: kind, wall coordinate `val`, rectangle
   {xmin, xmax, ymin, ymax} (boundaries.jl:29-150) and velocity (MovingBoundary only) */
int sz_set_domain(sz_ctx *ctx, const int32_t *kinds, const double *vals, const double *rects,
                  const double *bu, const double *bv);
/* topography elements: closed rings (CSR) with centroid and rmax (topography.jl:5-9) */
int sz_set_topography(sz_ctx *ctx, int32_t ntopo, const int32_t *off, const double *x,
                      const double *y, const double *cx, const double *cy, const double *rmax);
/* grid (grids.jl:106) and the (Nx+1)x(Ny+1) ocean/atmosphere lattices, element [ix][iy] at
   ix*(Ny+1)+iy (oceans.jl:74, atmos.jl:4) */
int sz_set_fields(sz_ctx *ctx, int32_t Nx, int32_t Ny, double x0, double xf, double y0, double yf,
                  const double *uocn, const double *vocn, const double *hflx_factor,
                  const double *uatm, const double *vatm);

/* ---- floe state */
/* M rows, of which the first N are parents; M > N only when the caller ran add_ghosts!
   itself, in which case ghost_off/ghost_idx must be given.
   floe.interactions is ragged and not part of the column struct: the rows the last collision call left on the
   device stay valid across an upload of the same M (the shim's re-upload between timestep_collisions! and
   timestep_floe_properties!, whose calc_stress! reads them); an upload of another size drops them, and
   sz_timestep_floe_properties / sz_calc_stress then fail with SZ_E_STATE until sz_upload_interactions (the
   matrices the host holds, possibly empty) or a collision call provides rows again.  A context that is given
   a DIFFERENT field of the same size must be told so with sz_upload_interactions. */
int sz_upload_floes(sz_ctx *ctx, int64_t M, int64_t N, const sz_floe_columns *cols);
int sz_get_stats(sz_ctx *ctx, sz_stats *out);
/* copies every non-NULL column (sized from sz_get_stats) */
int sz_download_floes(sz_ctx *ctx, sz_floe_columns *cols);
/* interactions of all M floes: off has M+1 entries, rows has n_inter_rows*7 doubles */
int sz_download_interactions(sz_ctx *ctx, int32_t *off, double *rows);
/* ---- the same boundary for hosts whose floes are Floe{Float32} (floe.jl:24: the struct is generic in its float type FT; SURVEY section 8b
   "two instantiations: _f64, _f32").  documentation.md:25 supports and tests Float64 only, so there are no Float32 answers to reproduce: the
   engine computes in double (or mixed precision, sz_set_precision) whatever the host's FT -- these entry points widen the columns on the
   way in and round them on the way out (a run from Float32 columns therefore equals the run from the same values held as doubles, rounded
   once at the end).  Integer columns and the CSR offsets are the same types as above. */
typedef struct {
  float *cx, *cy, *rmax, *area, *height, *mass, *moment, *alpha, *u, *v, *xi;
  float *p_dxdt, *p_dydt, *p_dalphadt, *p_dudt, *p_dvdt, *p_dxidt;
  float *fxOA, *fyOA, *trqOA, *hflx_factor, *overarea;
  float *coll_fx, *coll_fy, *coll_trq;
  float *stress_accum, *stress_instant, *strain;         /* 4 per floe */
  int64_t *id, *ghost_id;
  int32_t *status;
  int32_t *vert_off;  float *vx, *vy;
  int32_t *sub_off;   float *sx, *sy;
  int32_t *ghost_off; int32_t *ghost_idx;
} sz_floe_columns_f32;
int sz_upload_floes_f32(sz_ctx *ctx, int64_t M, int64_t N, const sz_floe_columns_f32 *cols);
int sz_download_floes_f32(sz_ctx *ctx, sz_floe_columns_f32 *cols);
int sz_set_fields_f32(sz_ctx *ctx, int32_t Nx, int32_t Ny, double x0, double xf, double y0, double yf,
                      const float *uocn, const float *vocn, const float *hflx_factor, const float *uatm, const float *vatm);
int sz_download_interactions_f32(sz_ctx *ctx, int32_t *off, float *rows);
/* the pairs that reached the narrow phase, in the reference's serial (i asc, j asc) order */
int sz_download_pairs(sz_ctx *ctx, int32_t *pi, int32_t *pj);
/* status.fuse_idx after the mirror pass (collisions.jl:801-806): off M+1, idx; call with
   idx == NULL to get only the offsets (off[M] = total) */
int sz_download_fuse(sz_ctx *ctx, int32_t *off, int32_t *idx);
int sz_get_boundary_vals(sz_ctx *ctx, double *vals4);
/* the boundary rectangles as they stand, {xmin, xmax, ymin, ymax} for N, S, E, W (MovingBoundary walls move with
   update_boundaries!, collisions.jl:565-571) */
int sz_get_boundary_rects(sz_ctx *ctx, double *rects16);

/* ---- processes (each mirrors one reference function, see the header comment) */
int sz_add_ghosts(sz_ctx *ctx);
int sz_remove_ghosts(sz_ctx *ctx);
int sz_timestep_collisions(sz_ctx *ctx, int64_t n_init, int32_t dt);
/* floe_floe_interaction! on explicit (i, j) pairs: only floe i of each pair is updated */
int sz_collide_pairs(sz_ctx *ctx, int64_t npairs, const int32_t *pi, const int32_t *pj, int32_t dt,
                     double max_overlap);
/* floe_domain_interaction! for every floe */
int sz_collide_domain(sz_ctx *ctx, int32_t dt, double max_overlap);
int sz_timestep_coupling(sz_ctx *ctx);
int sz_timestep_floe_properties(sz_ctx *ctx, int32_t dt);
/* ---- precision (BASELINE configs[4]): 0 = fp64 (default); 1 = mixed.  Mixed: the per-point arithmetic of
   calc_one_way_coupling! in fp32 on fp32 copies of the sub-floe points and the lattice; the broad phase on 32-byte fp32
   records with fp64 confirmation of the bounding-circle test (pair list bit-exact); in resident batches of single-context
   runs the rings as fp32 offsets in the floe's body frame + fp64 pose, world coordinates rebuilt in fp64 for the
   narrow-phase predicates.  Absolute positions, predicates, contact rows and per-floe totals stay
   fp64.  The reference has no Float32 answers (documentation.md:25); the acceptance criterion against the fp64 path is
   stated in tests/test_hip_parity.py.  Two-way coupling keeps its fp64 forcing kernel. */
int sz_set_precision(sz_ctx *ctx, int32_t mode);
/* ---- two-way coupling: calc_two_way_coupling! (coupling.jl:1617-1680) with floe_to_grid_info! (:1417-1454),
   center_cell_coords (:1116-1140) and shift_cell_idx (:1154-1178).  Off by default like CouplingSettings().
   With it on, every coupling step (sz_timestep_coupling, sz_step) also produces the ice+atmosphere stress on the
   ocean, the sea-ice fraction and the heat-flux factor per centre cell ((Nx+1) x (Ny+1) values, element
   [ix][iy] at ix*(Ny+1)+iy); the heat-flux factor replaces the hflx lattice given to sz_set_fields, as
   ocean.hflx_factor is overwritten in the reference.  Cd_ao, k, L: Constants() (simulation.jl:10-14); dt is the
   timestep used for the heat-flux factor by sz_timestep_coupling (sz_step uses its own).
   Tiled (multi-GPU) runs: a floe only contributes on the rank that owns it, so after a tiled coupling step every
   rank calls sz_two_way_partial (its per-cell sums -> a device buffer of 3 (Nx+1)(Ny+1) doubles: stress numerators
   x, y and ice area), the host adds the buffers up across the ranks (all-reduce) and sz_two_way_finish turns the
   sums into the ocean fields on every rank (both ASYNC on the context's stream). */
int sz_set_two_way(sz_ctx *ctx, int32_t on, double Cd_ao, double k, double L, int32_t dt);
int sz_set_temps(sz_ctx *ctx, const double *t_ocn, const double *t_atm);
int sz_download_ocean_stress(sz_ctx *ctx, double *tau_x, double *tau_y, double *si_frac, double *hflx);
int sz_two_way_partial(sz_ctx *ctx, void *d_partial);
int sz_two_way_finish(sz_ctx *ctx, const void *d_partial, int32_t dt);
/* calc_stress! (update_floe.jl:392-414, with _update_stress_accum!, stress_calculators.jl:118-122) and
   calc_strain! (update_floe.jl:425-453) on their own, for every floe, as the reference's tests call them
   (test_update_floe.jl:10-39).  sz_upload_interactions replaces floe.interactions of every floe by hand-made
   matrices first (CSR offsets, rows of 7: floeidx, xforce, yforce, xpoint, ypoint, torque, overlap). */
int sz_upload_interactions(sz_ctx *ctx, const int32_t *inter_off, const double *rows);
int sz_calc_stress(sz_ctx *ctx);
int sz_calc_strain(sz_ctx *ctx);
/* nsteps x timestep_sim! with the state resident in HBM; tstep counts from tstep0.
   The reference runs simplify_floes! (host work: fuse, remove, smooth, simulation.jl:205-214) at the end of EVERY
   step.  The batch therefore ends after the first step that leaves a parent tagged remove or fuse: the launches of
   the remaining steps are already enqueued and return at once.  *steps_done (may be NULL) = steps actually run
   (== nsteps when nothing was tagged); the state is that of the reference after steps_done steps, status.fuse_idx
   (sz_download_fuse) included, and the host resumes with sz_step(nsteps - steps_done, tstep0 + steps_done, ...) after
   its simplify_floes! (and the upload that follows it).  Floes already tagged at entry end the batch after one
   step.  SZ_NO_STOP in flags runs all steps regardless. */
int sz_step(sz_ctx *ctx, int32_t nsteps, int32_t tstep0, int32_t dt, int32_t coupling_dt,
            int32_t flags, int32_t *steps_done);

/* ---- fracture criteria on the device: determine_fractures (src/physical_processes/fractures.jl:269-280) on the resident state.
   fracture_floes! (fractures.jl:461) splits floes on the host -- topology-changing serial work -- but only on fracture steps where
   determine_fractures returns a floe; the device evaluates that predicate and a resident batch ends where it does.
   FractureSettings + the criterion + FloeSettings.min_floe_area + DecayAreaScaledCalculator.α:
     SZ_FRAC_HIBLER   HiblerYieldCurve(pstar, c): the 100-point polygon of _calculate_hibler (:83-94) rebuilt from the parents' mean
                      height on every fracture step (update_criteria!, :234-251); px / py unused
     SZ_FRAC_POLYGON  a fixed closed ring of npts <= 128 points in principal-stress space (MohrsCone.poly, or any criterion that does not
                      update); pstar / c unused
   dt = FractureSettings.Δt (> 0).  A floe is a candidate when area >= min_floe_area and the point (λmin, λmax) of its stress_accum, times
   (area / min_floe_area)^alpha when alpha != 0, is not covered by the polygon (inside or on the boundary counts as covered).
   sz_step with a criterion set (kind != SZ_FRAC_OFF): after every step with tstep % dt == 0 the criterion is evaluated on the device, and a
   candidate ends the batch after that step exactly as a tag does (*steps_done counts the step; the state is the reference's just before
   fracture_floes!; the launches of the later steps return at once; no host synchronisation per step).  SZ_NO_STOP runs through.
   Batches with a criterion set run the three-launch steps, never the pipelined ones (csrc/sz_pipeline.hpp): the mean height is a
   grid-wide dependency between a step's update and the next step's neighbour search, which the pipelined launches overlap.
   Tiled contexts: sz_tile_run evaluates the criterion collectively behind segments that end on fracture steps, sz_tile_fracture_candidates on
   request (both below); sz_tile_step, the host-driven step, returns SZ_E_STATE with a criterion set.
   SZ_FRAC_OFF (the default) adds nothing to a step, not even a launch. */
enum { SZ_FRAC_OFF = 0, SZ_FRAC_HIBLER = 1, SZ_FRAC_POLYGON = 2 };
int sz_set_fracture(sz_ctx *ctx, int32_t kind, int32_t dt, double pstar, double c, int32_t npts,
                    const double *px, const double *py, double alpha, double min_floe_area);
/* determine_fractures on the resident state as it is now: *n candidates, idx (may be NULL; room for N) = their 0-based parent indices,
   ascending.  Needs a criterion set. */
int sz_fracture_candidates(sz_ctx *ctx, int32_t *n, int32_t *idx);
/* test hook: the mean parent height and (Hibler) the polygon's p of the last evaluation (sz_fracture_candidates or a batch's fracture step) */
int sz_debug_fracture_mean(sz_ctx *ctx, double *mean_h, double *p);

/* ---- welding overlaps on the device: the geometry of timestep_welding! (src/physical_processes/welding.jl:91-182) on the resident state.
   The reference clips every pair of floes that share a welding bin (bin_floe_centroids, :23-55), pass potential_interaction (:128-131; parents
   only, no periodic images) and are active and under max_weld_area (:116-127), and welds on inter_area (:134), a random draw and an area
   window (:140-145); the fuse itself (fuse_two_floes!, :161-168) is topology-changing serial host work.  The device computes the OVERLAP TABLE:
   every such pair i < j with inter_area > 0, ordered as the reference visits them -- bins in eachindex order (k = (yidx - 1) Nx + xidx - 1), then i,
   then j ascending -- with inter_area = the sum of GO.area over all regions of intersect_polys.  The loop only ever asks for pairs whose two floes
   are still as they were when the call began, so the table of the state at the start serves the whole call; an empty table means
   the call changes nothing and draws no random number.
   sz_set_welding: WeldSettings (process_settings.jl:526-533).  n = 0 turns it off (the default: nothing changes, not even a launch).  dts / nxs / nys
   in the order the reference keeps them (sorted by Δt, largest first); the set of a step is the FIRST k with tstep % dts[k] == 0
   (simulation.jl:186-189).
   sz_step with welding set, in batches that stop: the batch ends after the first welding step whose table (for that step's Nx, Ny) is not empty;
   *steps_done counts that step, the state is the reference's just before timestep_welding!, and sz_weld_overlaps then gives the same table, bit
   for bit.  A tag or a fracture candidate on the same step ends the batch first (fracture_floes! runs before the welding).  The table of the batch's
   own last step is left to the caller.  The steps between two welding steps run as ordinary batches (pipelined where those are); one host
   synchronisation per welding step.  SZ_NO_STOP runs through and evaluates nothing.
   Tiled contexts: sz_tile_run computes the table collectively behind segments that end on welding steps, sz_tile_weld_overlaps on request (both
   below); sz_tile_step, the host-driven step, and sz_weld_overlaps on a tiled context return SZ_E_STATE.
   Limits: Nx * Ny * N^2 < 9e18 (the 64-bit pair key); rings of up to 254 vertices (the largest clip working set; beyond it SZ_E_CAPACITY). */
int sz_set_welding(sz_ctx *ctx, int32_t n, const int32_t *dts, const int32_t *nxs, const int32_t *nys, double max_weld_area);
/* the table of the state as it is now: *n entries; idx_i / idx_j (0-based parents) / inter_area have room for cap entries, or are all NULL to
   ask for *n only.  Needs the domain and the grid extents (sz_set_domain, sz_set_fields); two calls on the same state give the same bits. */
int sz_weld_overlaps(sz_ctx *ctx, int32_t nx, int32_t ny, double max_weld_area,
                     int32_t *n, int32_t cap, int32_t *idx_i, int32_t *idx_j, double *inter_area);
/* test hooks: per parent (room for N) the 0-based bin number of bin_floe_centroids or -1 (not binned: at or behind the first floe whose centroid
   is out of bounds, welding.jl:38 breaks there); the candidate pairs (before the clip) of the last table pass */
int sz_debug_weld_bins(sz_ctx *ctx, int32_t nx, int32_t ny, int32_t *bin);
int sz_debug_weld_npairs(sz_ctx *ctx, int32_t *n);

/* ---- removal and dissolution on the device (csrc/sz_remove.hpp): remove_floes! (simplification.jl:279-314) where simplify_floes!
   reduces to it -- no floe tagged fuse and no ring over max_vertices, so the pass needs no polygon union, no smoothing and no random number.
   sz_remove_floes runs the pass once on the state as it is, over the parents (ghosts in the list: SZ_E_STATE; a tiled context: SZ_E_STATE, its
   pass is the collective sz_tile_remove_floes below): in the reference's branch order a floe that is not tagged remove and lies under min_floe_area or min_floe_height
   dissolves, a floe tagged remove is removed (not dissolved as well), the others stay, in their order, with status active.  Every column
   sz_upload_floes takes moves to its new row, with the rings, the sub-floe points and the per-floe interaction rows (partner numbers left as they
   are, as the reference leaves them); everything derived is as sz_upload_floes leaves it.  *n_removed / *n_dissolved count the two kinds.
   *done = 0: the pass is DECLINED and nothing has changed -- a floe is tagged fuse, a ring has more than max_vertices points (GI.npoint counts
   the closing point, as sz_simplify_check), no floe would be left, or a dissolving floe's cell index leaves the matrix (below).  Not an error:
   the host's simplify_floes! takes over.
   The dissolved mass goes to the RUNNING ocean.dissolved lattice the context holds, (Nx + 1) (Ny + 1) doubles in the layout of
   sz_download_ocean_stress, zero after sz_set_fields: the host uploads the matrix it has (sz_upload_dissolved) and later overwrites its own with
   sz_download_dissolved -- deltas would change the summation order.  The dissolving floes are walked in descending row order, as
   reverse(eachindex(floes)) does: sums into one cell agree to the bit.  dissolve_floe! (simplification.jl:18-32) indexes its matrix as
   [yidx, xidx]; the quirk is kept (lattice element [yidx - 1][xidx - 1]).  Where that index lies outside the matrix the reference throws a
   BoundsError (non-square grids only): the pass is declined.
   sz_set_removal(on, SimplificationSettings.max_vertices -- INT32_MAX with smooth_vertices_on == false --, FloeSettings.min_floe_area,
   min_floe_height): off by default.  sz_step with removal set, in batches that stop: a tag that ends a segment before the batch's last step is
   followed by the pass; done = the batch goes on at the next step (*steps_done counts on), declined = it ends there as without removal.  On a
   fracture step with a candidate, or a welding step of a context with welding set, the batch ends as before (simulation.jl:172-214: fracture,
   weld, then simplify) and the caller calls sz_remove_floes itself.  The batch's own last step is not looked at.  SZ_NO_STOP batches and
   contexts without removal set run as before: not a launch more.
   sz_download_origin: per parent the row it had at the last sz_upload_floes (the identity after an upload, composed through the passes). */
int sz_set_removal(sz_ctx *ctx, int32_t on, int32_t max_vertices, double min_floe_area, double min_floe_height);
int sz_remove_floes(sz_ctx *ctx, int32_t *done, int32_t *n_removed, int32_t *n_dissolved);
int sz_upload_dissolved(sz_ctx *ctx, const double *dissolved);
int sz_download_dissolved(sz_ctx *ctx, double *dissolved);
int sz_download_origin(sz_ctx *ctx, int32_t *origin);

/* ---- rows down, rows back (csrc/sz_splice.hpp): the host's side of a stop -- fracture_floes!, the fuse of timestep_welding!, ridging
   and rafting, smoothing -- changes a few floes; these two calls move those floes alone, and the others do not leave HBM.
   sz_download_rows: `rows` holds n 0-based parent rows in any order, none twice (SZ_E_ARG: out of range or repeated).  With cols == NULL only
   sizes3 = {ring points, sub-floe points, interaction rows} of the selection is written, so that the caller can size its buffers.  Otherwise every
   non-NULL column receives n entries in the order of `rows` (the CSR offsets vert_off / sub_off / inter_off n + 1 entries, starting at 0; ghost_off
   zeros; ghost_idx is not written), each value with the bits sz_download_floes, sz_download_subpoints or sz_download_interactions give for that
   row.  One pack kernel writes the selection into one staging buffer, which comes down in one copy.  Works on any context that holds floes.
   sz_splice_floes: `del` (n_del) and `rep` (n_rep) are ascending 0-based parent rows of the list AS IT IS, without repeats, no row in both.  cols
   holds n_rep + n_app floes in the layout of sz_upload_floes (vert_off, vx, vy, cx, cy required; NULL columns are read as zeros, a NULL id as
   row + 1, a NULL status as active; ghost columns are ignored): the first n_rep overwrite the rows `rep`, the other n_app are appended behind the
   last kept row in the order given.  Deleted rows vanish, kept rows keep their order, as deleteat! / append! do.  inter_off (n_rep + n_app + 1) /
   inter_rows (k x 7) give floe.interactions of the uploaded floes (NULL: none); kept floes keep theirs, partner numbers untouched, as the removal
   pass leaves them (a partner that was a ghost of the last resident step is stored as the number sz_download_interactions reports for it).
   Afterwards the context is the one that sz_upload_floes(N', N', edited list) + sz_upload_interactions(edited lists) would have left in this same
   context: bit for bit in everything downloadable (columns, rings, sub-floe points, interaction rows, the counts of sz_get_stats, sz_download_origin
   = the identity), and everything derived is as sz_upload_floes leaves it (made again on demand: collision records, the fp32 copies of mixed
   precision, the blocked points of the forcing kernel, the static grid and the ghost-candidate list, the stop words, the per-capacity scratch of
   fracture, welding, removal, ridge / raft and two-way coupling).  Settings, domain, fields, the ocean.dissolved lattice and moving walls are left
   alone; the neighbour capacity keeps its value (it grows on demand).  An edit the capacities of the last upload cannot take (an eighth more rows or
   ring points than it held) is not refused: the context is carved anew on the device for the edited list and the rows move there; the sub-floe
   point pool, which an upload gives no slack, grows by itself.  The result is the same.
   Refusals leave the state untouched: ghosts in the list (sz_remove_ghosts first) or a pending ridge / raft step (sz_step_finish first) and tiled
   contexts (sz_tile_splice_floes below edits those, by global number): SZ_E_STATE; rows unsorted, repeated, out of range or both deleted and replaced, an edit that leaves no floe, an uploaded ring that is
   open (first point != last, or under 4 points) or longer than 255 points (what the row-moving kernels and the collision record carry): SZ_E_ARG;
   more interaction rows for a floe than the stride holds: SZ_E_CAPACITY, as sz_upload_interactions.  n_del = n_rep = n_app = 0 changes nothing.
   The _f32 twins widen and round exactly as sz_upload_floes_f32 / sz_download_floes_f32 / sz_download_interactions_f32 do. */
int sz_download_rows(sz_ctx *ctx, int32_t n, const int32_t *rows, sz_floe_columns *cols, int32_t *inter_off, double *inter_rows, int64_t *sizes3);
int sz_splice_floes(sz_ctx *ctx, int32_t n_del, const int32_t *del, int32_t n_rep, const int32_t *rep, int32_t n_app, const sz_floe_columns *cols,
                    const int32_t *inter_off, const double *inter_rows);
int sz_download_rows_f32(sz_ctx *ctx, int32_t n, const int32_t *rows, sz_floe_columns_f32 *cols, int32_t *inter_off, float *inter_rows, int64_t *sizes3);
int sz_splice_floes_f32(sz_ctx *ctx, int32_t n_del, const int32_t *del, int32_t n_rep, const int32_t *rep, int32_t n_app, const sz_floe_columns_f32 *cols,
                        const int32_t *inter_off, const float *inter_rows);

/* ---- ridge / raft candidates on the device (csrc/sz_ridgeraft.hpp): what tells whether timestep_ridging_rafting!
   (src/physical_processes/ridge_raft.jl:676-837) has anything to do.  The reference calls it on the list WITH its ghosts, between
   timestep_collisions! and the ghost removal, on every step with tstep % Δt == 0 (simulation.jl:121-136); the ridging and rafting themselves are
   serial, topology-changing host work that consumes sim.rng.  The device evaluates
     the per-floe draws: every list row draws once if height <= max_floe_ridge_height, then once if height <= max_floe_raft_height (:694-697);
       *n_draws is their count over all rows, ghosts included;
     the CANDIDATE TABLE: the gates of :698-753 and :757-831 with every draw assumed to pass.  (i, j) is an entry when row i is active and has
       interaction rows, one of them names j and passes valid_interaction as written there (j > 0: i < j, j active, potential_interaction;
       -1..-4: the boundary distance against rmax; below -4: the topography test), 1e-6 < overlap / min_area < 0.95 (both strict; min_area =
       min(area_i, area_j) for a floe partner, area_i otherwise), and the heights allow an action that changes state or draws: kind bit 1
       (ridge) for a floe partner = both heights <= max_floe_ridge_height and one of them >= min_ridge_height, for a domain partner = h_i <=
       min(max_floe_ridge_height, max_domain_ridge_height); bit 2 (raft) = both <= max_floe_raft_height, resp. h_i <= min(max_floe_raft_height,
       max_domain_raft_height).  One entry per (i, j), from the first passing row.
   The table is a superset of what the reference acts on: the probabilities are left out, and so is its never-cleared interactions_list buffer,
   which can only suppress entries.  An EMPTY table means the call changes no floe and draws exactly *n_draws numbers rand(rng, FT).
   sz_set_ridgeraft: RidgeRaftSettings (process_settings.jl).  Off by default: nothing changes, not even a launch.  dt <= 0 with on: SZ_E_ARG.
   sz_ridgeraft_candidates: the table of the state as it is, which must be the list with its ghosts and this step's rows (after sz_add_ghosts +
   sz_timestep_collisions, or sz_upload_interactions on such a list) or a pending stop -- SZ_E_STATE otherwise.  *n entries in ascending i, then
   row order: idx_i (0-based list row), idx_j (the partner as the rows name it: 1-based list row, -1..-4, -(4 + k)), kind, frac = overlap /
   min_area; the arrays have room for cap entries, or are all NULL to ask for the counts only.  Two calls on one state give the same bits.
   sz_step with ridge / raft set, in batches that stop (SZ_COLLISIONS_ON required): the batch is cut into segments that end BEFORE a ridge /
   raft step; that step runs through the process calls (sz_add_ghosts, sz_timestep_collisions), then the pass, one host synchronisation.
     Empty table: the draws are added to the batch's counter (sz_ridgeraft_draws: the sum over the ridge / raft steps the LAST sz_step ran
       through; the host advances its rng by that many rand(rng, FT)), the step is finished as sz_step_finish finishes it, and it ends as a
       segment's last step does -- a tag, a fracture candidate, a welding table, removal, in the reference's order.
     Non-empty table: the batch ends, *steps_done does NOT count the step, the context is PENDING at that timestep (sz_ridgeraft_pending: the
       timestep, or -1) and holds the reference's state between timestep_collisions! and timestep_ridging_rafting!: ghosts in the list; rows, fuse
       lists and ghost lists downloadable; sz_ridgeraft_candidates gives the same table, bit for bit.  While pending, sz_step returns SZ_E_STATE.
   sz_step_finish: the second half of the pending step on whatever state the device holds now (the host may have uploaded the floes its
   timestep_ridging_rafting! left, with their interactions): exactly sz_remove_ghosts; sz_timestep_coupling when flags and tstep % coupling_dt
   say so; sz_timestep_floe_properties -- and the pending mark is cleared.  SZ_E_STATE when nothing is pending; the batch goes on with
   sz_step(.., tstep + 1, ..) after the host's end-of-step processes.
   SZ_NO_STOP batches run through and evaluate nothing.  Tiled contexts: sz_tile_run stops the same way, collectively (sz_tile_ridgeraft_candidates,
   sz_tile_list_numbers and sz_tile_step_finish below); sz_tile_step, sz_step and sz_ridgeraft_candidates on a tiled context with ridge / raft set
   return SZ_E_STATE. */
int sz_set_ridgeraft(sz_ctx *ctx, int32_t on, int32_t dt, double min_ridge_height, double max_floe_ridge_height,
                     double max_domain_ridge_height, double max_floe_raft_height, double max_domain_raft_height);
int sz_ridgeraft_candidates(sz_ctx *ctx, int32_t *n, int32_t cap, int32_t *idx_i, int32_t *idx_j, int32_t *kind, double *frac,
                            int64_t *n_draws);
int sz_ridgeraft_pending(sz_ctx *ctx, int32_t *tstep);
int sz_ridgeraft_draws(sz_ctx *ctx, int64_t *n);
int sz_step_finish(sz_ctx *ctx, int32_t tstep, int32_t dt, int32_t coupling_dt, int32_t flags);

/* ---- a ridge / raft stop as row edits (csrc/sz_ridgeraft.hpp, csrc/sz_splice.hpp).  timestep_ridging_rafting! changes floes in
   place, parents and ghosts alike, and collects new pieces; timestep_sim! then deletes every row behind n_init_floes and appends the pieces
   (simulation.jl:137-147).  What goes on is "the parents, some replaced, pieces appended": the ghosts are read by the host and never sent back.
   sz_ridgeraft_rows: the rows the host's ridging and rafting can touch.  Valid where sz_ridgeraft_candidates is valid, with the same refusals.
   The candidate pass runs; for every table entry (i, j) row i and, where j > 0, row j - 1 are taken, each with its root parent (the row < N with
   the same id, found through the device's parent link) and every ghost on that parent's ghost list.  *n rows, ascending 0-based list rows, each
   once; rows has room for cap entries (cap < *n: SZ_E_ARG), or is NULL to ask for *n only.  An empty table gives *n = 0; two calls on one state
   give the same bits.
   sz_download_list_rows: sz_download_rows over the whole list.  `rows` may name any of the M list rows, ghosts included, in any order, none twice
   (SZ_E_ARG otherwise, the state untouched).  Every value has the bits sz_download_floes, sz_download_subpoints and sz_download_interactions give
   for that row; ghost_off (n + 1 entries) / ghost_idx are written -- a parent's ghost list in list numbers, as sz_download_floes gives it, an
   empty list for a ghost row (ghost_idx needs room for 3 entries per selected row).  A ghost row has no sub-floe points: its sub_off span is
   empty.  The same staging buffer and the same single copy down as sz_download_rows; the ghost lists travel in it.
   sz_splice_parents: sz_splice_floes on a list that still holds its ghosts.  Arguments and checks are those of sz_splice_floes; rows number the
   parents as they are; ghost columns of cols are ignored.  With ghosts in the list -- a pending ridge / raft step, or sz_add_ghosts by hand -- the
   ghosts are dropped as sz_remove_ghosts drops them and the edit is applied as sz_splice_floes applies it, both capacity paths included.  A
   pending mark stays: sz_step_finish then runs the second half and finds no ghost to remove.  With no ghosts and nothing pending it is
   sz_splice_floes.  Afterwards the context is, bit for bit in everything downloadable and with everything derived as sz_splice_floes states it,
   the one that sz_remove_ghosts followed by sz_upload_floes of the edited parents and sz_upload_interactions of their lists leaves in this same
   context.  Kept rows keep their partner numbers untouched: a kept row may go on naming a ghost's old list number, as in the reference behind
   simulation.jl:138-147.  Every check comes before the first change, so a refused call leaves the ghosts in the list: tiled contexts SZ_E_STATE;
   every edit sz_splice_floes refuses, with its code.  n_del = n_rep = n_app = 0 changes nothing and drops no ghost.
   The _f32 twins widen and round as those of sz_download_rows / sz_splice_floes do; sz_ridgeraft_rows_f32 is sz_ridgeraft_rows (no floating-point
   value crosses it; a Float32 host finds every call of the stop under one suffix). */
int sz_ridgeraft_rows(sz_ctx *ctx, int32_t *n, int32_t cap, int32_t *rows);
int sz_ridgeraft_rows_f32(sz_ctx *ctx, int32_t *n, int32_t cap, int32_t *rows);
int sz_download_list_rows(sz_ctx *ctx, int32_t n, const int32_t *rows, sz_floe_columns *cols, int32_t *inter_off, double *inter_rows, int64_t *sizes3);
int sz_splice_parents(sz_ctx *ctx, int32_t n_del, const int32_t *del, int32_t n_rep, const int32_t *rep, int32_t n_app, const sz_floe_columns *cols,
                      const int32_t *inter_off, const double *inter_rows);
int sz_download_list_rows_f32(sz_ctx *ctx, int32_t n, const int32_t *rows, sz_floe_columns_f32 *cols, int32_t *inter_off, float *inter_rows,
                              int64_t *sizes3);
int sz_splice_parents_f32(sz_ctx *ctx, int32_t n_del, const int32_t *del, int32_t n_rep, const int32_t *rep, int32_t n_app,
                          const sz_floe_columns_f32 *cols, const int32_t *inter_off, const float *inter_rows);

/* ---- measurement: HIP-event time per kernel class, accumulated since the last reset, on the
   stream the kernels are launched on; launches = number of timed launches of that class.
   on = 0: off; 1: every class; otherwise a mask, bit (k+1) = class k (e.g. 2 << SZ_K_NARROW: only
   the dominant kernel -- every event pair costs a few microseconds of a ~250 us step) */
int sz_profile_enable(sz_ctx *ctx, int32_t on);
int sz_profile_reset(sz_ctx *ctx);
int sz_kernel_time_ms(sz_ctx *ctx, int32_t kclass, double *ms, int64_t *launches);
/* which launch evaluated the forcings (timestep_coupling!, coupling.jl:1705) in the steps of the last sz_step: 0 their own,
   1 the neighbour search's, 2 the narrow phase's first variant (class SZ_K_NARROW then times both: a small field's narrow
   phase is one round with a long tail, and the forcings run in that tail), -1 no coupling step yet */
int sz_forcing_launch(sz_ctx *ctx, int32_t *where);
/* name of the dominant kernel's instantiation as a kernel trace (rocprofv3) prints it, for the last batch: buf gets at most n bytes */
int sz_narrow_kernel_name(sz_ctx *ctx, char *buf, int32_t n);

/* ---- multi-GPU halo support (no counterpart in the single-process reference:
   its periodic ghost floes, collisions.jl:881-1047, are the same pattern inside one address
   space).  One context per rank owns a fixed subset of the floes; every step the ranks trade
   ghost-floe records (sz_halo_record_doubles() doubles each) through buffers in DEVICE memory
   that the host hands to RCCL (torch.distributed all_to_all_single).
     sz_tile_enable   after sz_upload_floes of the owned floes: gidx[i] = global index of owned
                      floe i; all order-dependent rules then use global indices.  max_ring = largest
                      ring (points) over the floes of ALL ranks, 0 if unknown; max_rmax = largest rmax
                      over the floes of ALL ranks (the resident steps' fixed broad-phase grid must hold
                      for halo floes too), 0 if unknown (the grid is then fitted every step)
     sz_owned_box     bounding box of the owned centroids + largest rmax: xmin,xmax,ymin,ymax,rmax
     sz_halo_set_boxes  nranks x {xmin,xmax,ymin,ymax}, already expanded by the interaction range
     sz_halo_pack     ASYNC. Exchange buffers have one region per peer: 1 header record (count in
                      double [0]) + cap record slots.  Fills d_send with the owned floes whose
                      centroid, or a periodic image of it, lies in the peer's box
     sz_tile_forcing  ASYNC, optional.  The forcings of step tstep (they need nothing from the halo); called between
                      sz_halo_pack and the collective they run beside the exchange, and sz_tile_step(tstep)
                      skips them
     sz_tile_step     ASYNC. Appends the records of d_recv (same layout, region r = from rank r) as
                      halo floes, runs one timestep_sim! on owned + halo floes; only owned floes are
                      integrated, the halo is dropped at the end.  d_recv may be NULL (no peers)
     sz_sync          waits for everything enqueued, reports sticky device errors
     sz_set_stream    enqueue on the caller's HIP stream (torch.cuda.current_stream().cuda_stream) so
                      that the framework's collectives order with the kernels without host syncs */
int sz_tile_enable(sz_ctx *ctx, const int64_t *gidx, double max_ring, double max_rmax);
int sz_owned_box(sz_ctx *ctx, double *out5);
int sz_halo_record_doubles(void);
/* ... of THIS context after sz_tile_enable: the records have room for the largest ring of all ranks' floes (12 + 2 x ring capacity, at
   least the value above; rings of up to 255 points, as in a single context -- Floe rings are unbounded, floe.jl:24-77) */
int sz_halo_record_doubles_ctx(sz_ctx *ctx);
int sz_halo_set_boxes(sz_ctx *ctx, int32_t nranks, const double *boxes);
int sz_halo_pack(sz_ctx *ctx, int32_t nranks, int32_t my_rank, double Lx, double Ly, int32_t periodic_x,
                 int32_t periodic_y, void *d_send, int32_t cap);
int sz_halo_counts(sz_ctx *ctx, int32_t nranks, int32_t *counts_out);   /* of the last pack; d_send NULL = count only */
int sz_tile_forcing(sz_ctx *ctx, int32_t tstep, int32_t coupling_dt, int32_t flags);
int sz_tile_step(sz_ctx *ctx, const void *d_recv, int32_t nranks, int32_t cap, int32_t tstep, int32_t dt,
                 int32_t coupling_dt, int32_t flags);
int sz_sync(sz_ctx *ctx);
int sz_set_stream(sz_ctx *ctx, void *hip_stream);

/* ---- the same halo exchange INSIDE the library: RCCL over xGMI, one process per GPU, no Python / torch involved.
   (The single-process reference has no counterpart: it keeps all floes in one address space, and its periodic ghost floes
   -- collisions.jl:881-1047, folded back at :830-850 -- are the pattern this generalises to tiles.)
     sz_comm_unique_id   on ONE rank: 128 bytes (an ncclUniqueId) that the host passes to every rank by its own channel
                         (MPI broadcast, a file, ...)
     sz_comm_init        on every rank, collectively: the communicator of this context (nranks == 1: no RCCL needed)
     sz_tile_setup       after sz_upload_floes + sz_tile_enable: domain lengths and periodicity, the drift margin (metres a
                         floe may move between two box gathers, on top of the interaction range) and the LONGEST gather
                         interval: the library starts with 8 steps and sizes every following interval from the displacement
                         it measured and the largest velocity now (30 % of the margin), at most doubling it.  rebox_every < 0:
                         exactly every |rebox_every| steps, no adaptation (tests of the drift error)
     sz_tile_run         nsteps x timestep_sim! of the tiled run, collectively, same arguments on every rank.  Per step:
                         grouped ncclSend / ncclRecv (whole regions with the neighbouring tiles, real counts in the header
                         records, slots per pair sized at the last gather; the header record with every rank), forcings of
                         the owned floes beside the exchange, unpack + step; the halo records of the next step are written by
                         the step's integrator (a pack launch starts a batch), each floe as the update left it, before a swap
                         with its ghost -- the receiving rank swaps it with the owner's routine, so a floe's instances are the
                         same bits with the same ghost numbers on every rank.  Two-way coupling partial sums are all-reduced
                         (those batches run to their end: no tag stop).  A floe that moves further than half
                         the margin between two gathers is an error (halo-drift bit), never a silently missed contact.
                         As with sz_step the batch ends after the first step that leaves a floe tagged remove / fuse ON ANY RANK
                         (simplify_floes!, simulation.jl:205-214, runs after every step and is the host's): every rank's header
                         record carries its stop request to every other rank with the next exchange, whose unpack kernel ends the
                         batch there before that step has touched anything.  *steps_done (may be NULL) is the same number on every
                         rank; status.fuse_idx (sz_download_fuse) of a tiled context names partners by GLOBAL floe index.
                         SZ_NO_STOP runs all steps.
                         With a criterion set (sz_set_fracture) and without SZ_NO_STOP the batch is cut into segments that end on a
                         fracture step (tstep % dt == 0); behind a segment whose last step ran, the ranks evaluate the criterion over
                         the ONE global list (sz_tile_fracture_candidates below: the same pass) and a candidate ON ANY RANK ends the
                         batch on every rank, *steps_done counting the fracture step -- where sz_step ends it for the undivided list.
                         A tag raised on that step ends the batch there too when no floe fractures (with removal set: the removal
                         pass, and on).  The batch's own last step is not looked at: the caller asks.  SZ_NO_STOP batches and
                         contexts without a criterion launch and gather nothing for it.  Needs sz_tile_setup and a communicator
                         (SZ_E_STATE without); with two-way coupling across tiles a criterion is refused (SZ_E_STATE: those batches
                         have no tested stop).
                         With welding set (sz_set_welding) and without SZ_NO_STOP the segments also end on welding steps (the first k
                         with tstep % dts[k] == 0 gives Nx, Ny).  Behind a segment whose last step ran the order is the single
                         context's: the fracture pass on a fracture step, then the collective overlap table (sz_tile_weld_overlaps
                         below: the same pass), then removal.  A table that is not empty ends the batch on every rank, *steps_done
                         counting the welding step; an empty one lets the next segment start.  A tag or a fracture candidate on that
                         step ends the batch first, where sz_step ends it, with removal set too.  The batch's own last step is not
                         looked at.  SZ_NO_STOP batches and contexts without welding launch and gather nothing for it.  Needs
                         sz_tile_setup and a communicator; refused with two-way coupling across tiles, like a criterion.
                         With ridge / raft set (sz_set_ridgeraft) and without SZ_NO_STOP (SZ_COLLISIONS_ON required) the segments also end
                         BEFORE a ridge / raft step (tstep % dt == 0), and that step is a segment of its own: pack, exchange, the first
                         half of the step (unpack, ghosts, collisions), then the collective candidate pass over the ONE global list
                         (sz_tile_ridgeraft_candidates below: the same pass).  An empty table: the draws of all ranks go to the batch's
                         counter (sz_ridgeraft_draws: the same sum on every rank), the second half runs, and the step ends as a
                         segment's last step does -- a tag ANY rank raised, the fracture pass, the welding pass, removal.  A table that
                         is not empty ends the batch on every rank with the step PENDING (sz_ridgeraft_pending): *steps_done does NOT
                         count it, the lists keep their halo rows and ghosts, and sz_tile_run and sz_tile_migrate return SZ_E_STATE
                         until sz_tile_step_finish has run.  SZ_NO_STOP batches and contexts without ridge / raft launch and gather
                         nothing for it.  Needs sz_tile_setup and a communicator; refused with two-way coupling across tiles.
                         Device errors are per rank; the ranks agree on them at every box gather and at the end of the call,
                         so that EVERY rank returns the same code at the same step (a rank leaving on its own would hang the
                         others: RCCL has no timeout).  A new sz_upload_floes invalidates sz_tile_enable / sz_tile_setup.
     sz_comm_allreduce   sum of n doubles in device memory over the ranks, in place (sz_eulerian_partial / sz_two_way_partial) */
int sz_comm_available(void);   /* SZ_OK when RCCL can be bound in this process; ask on every rank and agree before sz_comm_init (collective) */
int sz_comm_unique_id(void *id128);
int sz_comm_init(sz_ctx *ctx, int32_t nranks, int32_t rank, const void *id128);
/* The same tiled run over the HOST's own channel between its ranks, for hosts whose ranks cannot open an RCCL communicator
   (an MPI.jl build that is not device-aware, several ranks sharing one GPU -- RCCL refuses that, so this is also how the
   library's multi-rank exchange is rehearsed on a one-GPU box): sz_comm_init_host instead of sz_comm_init, everything else
   as above.  The library stages the regions through host memory and calls the three collectives below with HOST pointers;
   they block, return 0 on success, and are called by every rank in the same order.
     allgather          `bytes` from every rank into recv (nranks x bytes, in rank order)
     sendrecv           npeers point-to-point transfers in each direction, all of them in flight together:
                        send[k] / send_bytes[k] to rank peer[k], recv[k] / recv_bytes[k] from rank peer[k]
                        (a peer's send_bytes to this rank equals this rank's recv_bytes for it; either may be 0)
     allreduce_sum_f64  element-wise sum of n doubles over the ranks, in place */
typedef struct sz_host_transport {
  void *user;
  int (*allgather)(void *user, const void *send, void *recv, int64_t bytes);
  int (*sendrecv)(void *user, int32_t npeers, const int32_t *peer, const void *const *send, const int64_t *send_bytes,
                  void *const *recv, const int64_t *recv_bytes);
  int (*allreduce_sum_f64)(void *user, double *buf, int64_t n);
} sz_host_transport;
int sz_comm_init_host(sz_ctx *ctx, int32_t nranks, int32_t rank, const sz_host_transport *transport);
int sz_comm_destroy(sz_ctx *ctx);
/* one-rank self test of the RCCL binding (run-time loading, communicator of one rank, all-gather, all-reduce, grouped
   send / receive to self with the stream hand-shake of sz_tile_run): what of the exchange can run on a one-GPU box */
int sz_comm_selftest(sz_ctx *ctx);
int sz_comm_allreduce(sz_ctx *ctx, void *d_buf, int64_t n);
int sz_tile_setup(sz_ctx *ctx, double Lx, double Ly, int32_t periodic_x, int32_t periodic_y, double drift_margin,
                  int32_t rebox_every);
/* optional, after sz_tile_setup: the centre of this rank's tile.  The bounding box of the owned floes -- what the peers select this rank's
   halo with -- takes every centroid at its periodic image nearest to that point at the first gather (later gathers use the centre of the
   box before), so that a parent the ghost pass has wrapped to the far side of the domain does not stretch the box across the domain */
int sz_tile_set_center(sz_ctx *ctx, double x, double y);
int sz_tile_run(sz_ctx *ctx, int32_t nsteps, int32_t tstep0, int32_t dt, int32_t coupling_dt, int32_t flags, int32_t *steps_done);
/* Migration (collective, between two sz_tile_run calls): every owned floe is re-assigned to the tile that holds its centroid -- px x py
   tiles over the domain of sz_set_domain, tile (ix, iy) = rank iy * px + ix; owner_override (may be NULL; one entry per owned floe, in
   the order of the last upload) names the new owner rank instead.  Floes that change tile travel with their complete state (all columns,
   tensors, status, ring, sub-floe points) over the library's channel (RCCL or the host transport); the context is then rebuilt from the
   kept and the received floes, ordered by global index, exactly as an upload + sz_tile_enable + sz_tile_setup (same parameters) would.
   The movers are packed on the device, one stream per destination, travel device to device (RCCL grouped send / receive; a host
   transport stages those streams only) and the rows are gathered into their new order on the device: the host sees the owner and
   offset columns and a directory of what arrived, no floe data (csrc/sz_migrate.hpp).  The capacities of the last upload stay; a
   tile that would crowd them (more than 1/8 above what that upload held, on any rank) is rebuilt through a download and an upload
   instead -- the host-staged path, on every rank (SZ_MIGRATE_HOST=1 forces it; sz_debug_migrate_path: 1 device, 2 host-staged).
   *n_sent = floes this rank gave away, *n_owned = floes it owns now (sz_tile_owned_gidx names them; the host's own copies of the
   columns are stale).  floe.interactions do not travel.
   sz_download_subpoints: the sub-floe points of the floes the context holds (off: N + 1 entries; sx == NULL: offsets only). */
int sz_tile_migrate(sz_ctx *ctx, int32_t px, int32_t py, const int32_t *owner_override, int64_t *n_sent, int64_t *n_owned);
int sz_tile_owned_gidx(sz_ctx *ctx, int64_t *gidx, int64_t n_cap);
/* Removal and dissolution on a tiled context (csrc/sz_remove_tile.hpp; DESIGN.md §9d, "tiled contexts"): sz_remove_floes over the ONE global floe
   list whose rows live on the ranks' tiles.  Collective, between two sz_tile_run calls: it needs sz_tile_enable + sz_tile_setup and the
   communicator (RCCL, the host transport, or one rank), the parents alone in the list, and the parameters of sz_set_removal.  Every rank is left
   with what the single context's pass leaves for the same global list, restricted to the floes it owns:
     - a floe that stays gets the global number the single context gives it -- its old one minus the floes that left, on ANY rank, with a smaller
       number -- as its order key; sz_tile_owned_gidx reports the new numbers;
     - the dissolving floes of all ranks are walked in descending global number on every rank, so every rank holds the same replica of
       ocean.dissolved, bit for bit the single context's (sz_upload_dissolved: the same matrix on every rank; sz_download_dissolved: any rank's);
     - the rows move and everything derived is rebuilt as in sz_remove_floes; owned boxes, halo capacities and peers are gathered again at the
       next exchange, as after sz_tile_migrate; the ring / rmax maxima given to sz_tile_enable are kept.
   *n_removed / *n_dissolved are GLOBAL counts, the same on every rank.  *done = 0: declined on EVERY rank and nothing has changed on any -- a fuse
   tag or a ring over max_vertices on any rank, the index quirk of sz_remove_floes, no floe left, or ANY RANK left without a floe (a limit: the
   tile drivers are not tested on empty tiles; the host's path takes over).  Every rank issues the same collectives whatever it holds, and an
   error one rank finds -- device error bits, scratch memory it could not get, counts that do not add up -- is agreed on before the next
   collective: all ranks return the same code, with the lattice and every row as they were.  A failure of the HIP runtime or of the channel
   itself (SZ_E_HIP) is returned at once, as everywhere in the library.
   sz_tile_run with removal set (sz_set_removal) and without SZ_NO_STOP: a segment that a tag ends before the batch's last step is followed by
   this pass; done = the next segment starts at the following step and *steps_done counts on, declined = the batch ends there as without removal.
   The batch's own last step is not looked at.  Tiled two-way coupling has no tag stop to hang the pass on: removal is not engaged there. */
int sz_tile_remove_floes(sz_ctx *ctx, int32_t *done, int32_t *n_removed, int32_t *n_dissolved);
/* Rows down, rows back on a tiled context, by GLOBAL number (csrc/sz_splice_tile.hpp): sz_download_rows / sz_splice_floes over the ONE
   global floe list whose rows live on the ranks' tiles (library backends; sz_download_rows / sz_splice_floes themselves stay single-context calls).
   The collective passes give every rank the same table, so every rank's host makes the same decisions: the edit is stated once, in global numbers,
   and every rank calls with identical arguments and applies the share that concerns the rows it owns.  No floe data crosses between the ranks.
   Both calls need sz_tile_enable, the parents alone in the list (ghosts: SZ_E_STATE), no pending ridge / raft step (SZ_E_STATE: sz_tile_step_finish
   first) and the owned global numbers ASCENDING BY ROW (SZ_E_STATE otherwise: the rows are found by binary search in the order keys; sz_tile_migrate
   and sz_tile_remove_floes leave them so, sz_tile_enable takes any order).
   sz_tile_download_rows: LOCAL, not collective.  gidx holds n global numbers in any order, none negative, none twice (SZ_E_ARG).  which[0 .. *n_mine)
   receives the positions in gidx of the floes this rank owns, ascending (which has room for n entries); a name no rank owns is found nowhere.
   n has no limit of the context's: the names are searched and compacted 2^20 at a time, so a request may be longer than any of its capacities.
   The rows come back in that order with the layout, the sizes3 / cols == NULL protocol and the bits of sz_download_rows -- the same staging buffer
   and single copy; partner numbers are as sz_download_interactions reports them on this tiled context.
   sz_tile_splice_floes: COLLECTIVE, the same arguments on every rank; it also needs sz_tile_setup and the communicator (RCCL, the host transport,
   or one rank).  del / rep: ascending global numbers of the list AS IT IS, without repeats, none in both.  cols, inter_off, inter_rows: the n_rep
   replacements, then the n_app appended floes, in the layout of sz_splice_floes; app_owner[k] (required with n_app > 0) is the rank that takes
   appended floe k.  Afterwards every rank holds what the single context holds after sz_splice_floes with the same edit on the undivided list,
   restricted to the floes the rank owns:
     - a kept floe's global number is its old one minus the deleted floes, on ANY rank, with a smaller number; appended floe k gets
       N_global - n_del + k; a replaced floe stays with its owner (the next sz_tile_migrate moves it if it must); a floe uploaded without an id gets
       its new global number + 1;
     - the new numbers are the order keys and what sz_tile_owned_gidx reports; columns, rings, sub-floe points and statuses of owned floes equal the
       single context's rows of those numbers, bit for bit; everything derived is as sz_splice_floes leaves it, both capacity paths included;
     - interaction rows of kept floes are what this rank's download reported before the edit, staged floes get the uploaded rows;
     - the tiling is established again on every rank (one whose rows did not change included: its numbers still move) with the new numbers, the
       centre kept, and the ring / rmax maxima given to sz_tile_enable raised to cover every staged floe of the whole edit (a maximum of 0 stays 0);
       owned boxes, halo capacities and peers come with the next exchange, as after sz_tile_remove_floes.
   *n_global / *n_owned: the new counts (either may be NULL).  The one collective is a small all-gather in front of the change: per rank the error
   bits, the rows owned, the del and rep names found, the appended floes taken.  From it every rank derives N_global and refuses alike, with the
   state untouched: names that do not add up to n_del / n_rep -- one out of range or owned twice -- (SZ_E_ARG); an edit that leaves no floe, or
   leaves ANY rank without a floe, as sz_tile_remove_floes declines (SZ_E_ARG); ghosts, an empty rank or unsorted numbers on any rank (SZ_E_STATE);
   device error bits on any rank, or more interaction rows for a floe than some rank's stride holds (SZ_E_CAPACITY).  What the arguments alone
   decide is refused before the collective, on every rank alike: names unsorted, repeated, negative or both deleted and replaced, app_owner out of
   range, open rings or rings over 255 points (SZ_E_ARG).  A failure of the HIP runtime or of the channel itself (SZ_E_HIP) is returned at once.
   n_del = n_rep = n_app = 0 changes nothing and issues no collective (*n_global = -1: the global count takes one; *n_owned = the rows owned).
   The _f32 twins widen and round as those of sz_download_rows / sz_splice_floes do. */
int sz_tile_download_rows(sz_ctx *ctx, int32_t n, const int64_t *gidx, int32_t *n_mine, int32_t *which, sz_floe_columns *cols, int32_t *inter_off,
                          double *inter_rows, int64_t *sizes3);
int sz_tile_splice_floes(sz_ctx *ctx, int32_t n_del, const int64_t *del, int32_t n_rep, const int64_t *rep, int32_t n_app, const int32_t *app_owner,
                         const sz_floe_columns *cols, const int32_t *inter_off, const double *inter_rows, int64_t *n_global, int64_t *n_owned);
int sz_tile_download_rows_f32(sz_ctx *ctx, int32_t n, const int64_t *gidx, int32_t *n_mine, int32_t *which, sz_floe_columns_f32 *cols, int32_t *inter_off,
                              float *inter_rows, int64_t *sizes3);
int sz_tile_splice_floes_f32(sz_ctx *ctx, int32_t n_del, const int64_t *del, int32_t n_rep, const int64_t *rep, int32_t n_app, const int32_t *app_owner,
                             const sz_floe_columns_f32 *cols, const int32_t *inter_off, const float *inter_rows, int64_t *n_global, int64_t *n_owned);
/* Fracture criteria on a tiled context (csrc/sz_fracture_tile.hpp; DESIGN.md §9b, "tiled contexts"): determine_fractures over the ONE global
   floe list whose rows live on the ranks' tiles, on the state as it is.  Collective: it needs sz_tile_enable + sz_tile_setup, the communicator
   (RCCL, the host transport, or one rank), the parents alone in the list and a criterion (sz_set_fracture, the same on every rank).  The heights
   of all ranks are gathered by global number, and the single context's kernels run unchanged -- the mean and the polygon over the gathered
   array, in the single context's order of additions (a reduce of per-rank sums would add in another order: other last bits of p), the test
   over the owned rows -- so every rank holds the single context's mean, p and verdicts to the bit (sz_debug_fracture_mean).
   *n_global = candidates on all ranks, the same number on every rank; *n_owned = this rank's; rows / gidx (each may be NULL: counts only;
   room for the owned floes) = their local rows, ascending, and their global numbers.  The global numbers of the ranks must be
   0 .. N_global - 1 once each: one out of range or held twice is SZ_E_STATE on EVERY rank, as is any error one rank finds (device error
   bits: SZ_E_CAPACITY) -- the ranks agree before they return, and nothing of the floes has changed.  A failure of the HIP runtime or of the
   channel itself (SZ_E_HIP) is returned at once. */
int sz_tile_fracture_candidates(sz_ctx *ctx, int32_t *n_global, int32_t *n_owned, int32_t *rows, int64_t *gidx);
/* Welding overlaps on a tiled context (csrc/sz_weld_tile.hpp; DESIGN.md §9c, "tiled contexts"): the table of sz_weld_overlaps over the ONE global
   floe list whose rows live on the ranks' tiles, on the state as it is.  Collective: it needs sz_tile_enable + sz_tile_setup, the communicator
   (RCCL, the host transport, or one rank), the parents alone in the list, the domain and the grid extents.  The bins, the break at the first
   out-of-bounds centroid (the smallest such global number over all ranks) and the candidate pairs are those of the global list; the rank that
   owns the floe with the smaller number clips the pair, with the other floe's ring sent over when it lives elsewhere, by the single context's
   clipper on the same ring bits.  Every rank gets the WHOLE table: *n entries, idx_i / idx_j in GLOBAL numbers (i < j), inter_area -- the rows of
   the single context's table in its order, areas to the bit, identical on every rank.  n, cap and SZ_E_ARG for a cap under *n as in
   sz_weld_overlaps (the same cap on every rank).  The global numbers of the ranks must be 0 .. N_global - 1 once each (SZ_E_STATE on EVERY rank
   otherwise), and any error one rank finds (device error bits, scratch memory) is agreed on before the next collective: all ranks return the
   same code, and nothing of the floes has changed.  A failure of the HIP runtime or of the channel itself (SZ_E_HIP) is returned at once.
   Limits: Nx * Ny * N_global^2 < 9e18; rings of up to 254 vertices.
   Test hooks (collective): per OWNED row the 0-based bin or -1, with the break of the global list; the candidate pairs of the last pass, summed
   over the ranks. */
int sz_tile_weld_overlaps(sz_ctx *ctx, int32_t nx, int32_t ny, double max_weld_area,
                          int32_t *n, int32_t cap, int64_t *idx_i, int64_t *idx_j, double *inter_area);
int sz_tile_debug_weld_bins(sz_ctx *ctx, int32_t nx, int32_t ny, int32_t *bin);
int sz_tile_debug_weld_npairs(sz_ctx *ctx, int64_t *n);
/* Ridge / raft candidates on a tiled context (csrc/sz_ridgeraft_tile.hpp; DESIGN.md §9e, "tiled contexts"), at a PENDING stop of sz_tile_run: the
   local list holds the owned floes, the halo floes and the ghosts of both, with this step's rows.  Every local row has an order key (a parent: its
   global number; a ghost: (pass << 40) + 4 gid + k); sorted, the distinct keys of all ranks are the single context's list order.  A list row is
   evaluated by ONE rank, the owner of its root parent, and the reference's i < j gate is the comparison of the keys.
   sz_tile_ridgeraft_candidates (collective: it runs the pass again): the WHOLE table of sz_ridgeraft_candidates for the undivided list on every
   rank, in its numbering (idx_i: 0-based list row -- a parent's global number, a ghost's N_global + its place among the ghosts; idx_j: the partner
   as the rows name it, 1-based list row or the negative boundary / topography number) and its order, kind and frac to the bit; *n_draws is the
   exact integer sum over the ranks.  Two calls give the same bits.  A cap under *n: SZ_E_ARG on every rank (the same cap everywhere), and the
   context goes on.  Any error one rank finds is agreed on before the next collective: all ranks return the same code.
   sz_tile_list_numbers: the single context's list number of every LOCAL row -- owned floes, halo floes, ghosts, in local order (-1: a ghost of a
   halo floe that its owner does not hold) -- of the pass that stopped the batch or of the last sz_tile_ridgeraft_candidates: with it a host reads
   the partner column of downloaded rows: the column holds order key + 1, and sz_tile_list_keys gives the order key of every local row in the
   same order (every partner a row names is a local row).
   sz_tile_step_finish (collective): the second half of the pending step on what the device holds -- the forcings of a coupling step, the
   integrator -- then the halo rows and ghosts are dropped and the mark is cleared.  SZ_E_ARG for a tstep that is not the pending one, SZ_E_STATE
   when nothing is pending.  What an upload does to a pending tiled context is not defined yet. */
int sz_tile_ridgeraft_candidates(sz_ctx *ctx, int32_t *n, int32_t cap, int64_t *idx_i, int64_t *idx_j, int32_t *kind, double *frac,
                                 int64_t *n_draws);
int sz_tile_list_numbers(sz_ctx *ctx, int64_t *out, int64_t cap);
int sz_tile_list_keys(sz_ctx *ctx, int64_t *out, int64_t cap);
int sz_tile_step_finish(sz_ctx *ctx, int32_t tstep, int32_t dt, int32_t coupling_dt, int32_t flags);
int sz_debug_migrate_path(sz_ctx *ctx);
/* diagnosis: the ghost / halo row that carried order key `key` in the last resident step that used ghost allocator `slot` (0-based step & 1), as the
   collision kernels saw it -- out56: row (-1: none), cx, cy, u, v, xi, rmax, area, height, box x0 x1 y0 y1, ring points, parent, status, ring x[20], y[20] */
int sz_debug_find_key(sz_ctx *ctx, int32_t slot, int64_t key, double *out56);
/* diagnosis: pair items of the last resident step between the instances (parent, ghosts) of two floe ids -- out61: entries, then {owner key, partner
   key, contact rows, owner row, partner row} for up to 12 of them */
int sz_debug_pairs_of_ids(sz_ctx *ctx, int32_t slot, int64_t id_a, int64_t id_b, double *out61);
int sz_download_subpoints(sz_ctx *ctx, int32_t *off, double *sx, double *sy);

/* ---- output path on the resident state
   sz_eulerian_data: calc_eulerian_data! (output.jl:793-914), the GridOutputWriter averages, over the rows the
   context holds -- write_data! runs after add_ghosts! (simulation.jl:102-105), so callers that step with sz_step
   bracket it with sz_add_ghosts / sz_remove_ghosts.  xg (nx + 1) and yg (ny + 1) are the writer's grid lines (evenly
   spaced, as GridOutputWriter builds them, output.jl:352-353); outputs lists nout of the SZ_EUL_* codes;
   data[k][ix][iy] at (k * nx + ix) * ny + iy is writer.data[ix + 1, iy + 1, k + 1].  Topography is taken out of
   the cells as the reference does (elements must not overlap one another).
   The FloeOutputWriter (write_floe_data!, output.jl:558-574) writes whole columns: sz_download_floes with only
   the wanted columns non-NULL is its device-side packing.
   sz_simplify_check: what simplify_floes! (simplification.jl:339-378) would find to do -- out4 = floes tagged remove,
   tagged fuse, rings with more than max_vertices points (smooth_floes!, :66) and floes under min_floe_area /
   min_floe_height that are not tagged remove (remove_floes!, :287-290).  All four zero: the pass changes nothing and
   no geometry needs to leave the device. */
enum { SZ_EUL_U = 0, SZ_EUL_V, SZ_EUL_DUDT, SZ_EUL_DVDT, SZ_EUL_OVERAREA, SZ_EUL_MASS, SZ_EUL_AREA, SZ_EUL_HEIGHT,
       SZ_EUL_SI_FRAC, SZ_EUL_STRESS_XX, SZ_EUL_STRESS_YX, SZ_EUL_STRESS_XY, SZ_EUL_STRESS_YY, SZ_EUL_STRESS_EIG,
       SZ_EUL_STRAIN_UX, SZ_EUL_STRAIN_VX, SZ_EUL_STRAIN_UY, SZ_EUL_STRAIN_VY, SZ_EUL_COUNT };
int sz_eulerian_data(sz_ctx *ctx, int32_t nx, int32_t ny, const double *xg, const double *yg, int32_t nout,
                     const int32_t *outputs, double *data);
/* tiled (multi-GPU) runs: a floe and its ghosts count on the rank that owns it.  Every rank calls
   sz_eulerian_partial (its per-cell sums -> SZ_EUL_PARTIAL * nx * ny doubles in device memory), the host adds the
   buffers up across the ranks (all-reduce), sz_eulerian_finish turns the sums into the averages on every rank. */
enum { SZ_EUL_PARTIAL = 17 };
int sz_eulerian_partial(sz_ctx *ctx, int32_t nx, int32_t ny, const double *xg, const double *yg, void *d_partial);
int sz_eulerian_finish(sz_ctx *ctx, int32_t nx, int32_t ny, const double *xg, const double *yg, const void *d_partial,
                       int32_t nout, const int32_t *outputs, double *data);
int sz_simplify_check(sz_ctx *ctx, int32_t max_vertices, double min_floe_area, double min_floe_height, int64_t *out4);

/* ---- output frames on the device (csrc/sz_record.hpp): write_data! runs at the start of every output step, right behind
   add_ghosts! (simulation.jl:102-105).  With a writer registered sz_step cuts its batch BEFORE each output step of that writer and records, at
   the cut, what the writer would take -- and goes on: ghosts a process call left attached are detached, sz_add_ghosts, one pack launch per due
   floe writer, the averages per due grid writer, sz_remove_ghosts.  The frames stay in device memory until the host drains them; nothing else
   crosses to the host at an output step.  The schedule is taken whenever a writer is set, also with nothing else set and with SZ_NO_STOP (the
   batch is then only cut and recorded: no pass runs, no tag is looked at); segments long enough stay pipelined.
   THE RULE: every output step at which a batch BEGINS A STEP has exactly one frame per due writer, taken before the step -- the batch's first
   step included, and a ridge / raft step that is left pending (*steps_done does not count it; the next sz_step starts behind it, so no step
   gets two frames).  The batch's end step, tstep0 + *steps_done, has none: the next call records it.
   Up to 4 floe writers and 4 grid writers, each with its own dt_out (FloeOutputWriter / GridOutputWriter Δtout; tstep % dt_out == 0 is an
   output step).  dt_out == 0 turns that writer off, which is the default: not a launch more, and no allocation.  dt_out < 0 or a writer
   index outside 0..3: SZ_E_ARG.  Setting a writer again frees its frames.  Single contexts only: both setters return SZ_E_STATE on a tiled
   context, sz_tile_enable returns SZ_E_STATE on a context with a writer set through them (a tiled context has setters of its own, below).
   sz_set_floe_output: columns_mask has one bit per column group of sz_floe_columns, in struct order (sz_debug_frame_bits): bits 0..27 the 28
     double columns cx .. strain (tensors 4 per floe), 28 id, 29 ghost_id, 30 status, 31 the rings (vert_off + vx + vy), 32 the ghost links
     (ghost_off + ghost_idx).  The ragged members -- floe.interactions and the sub-floe points -- are the lists of sz_set_floe_output_lists,
     below.  Frames are appended to one arena of arena_bytes in device memory.
     A FLOE FRAME is what sz_add_ghosts followed by sz_download_floes of the selected columns gives at the start of the step, with one rule made
     explicit: a ghost is a deep copy of its parent (collisions.jl:881-901, floe_utils.jl:138), so a ghost row carries the parent's bits in
     every recorded column except cx, cy, the ring and ghost_id (the device keeps only the collision columns on ghost rows; the pack reads the
     others from the parent row).  vert_off is frame-relative; a ghost row's ghost_off span is empty.
   sz_set_floe_output_lists: the ragged members floe writer `writer` records beside its columns, SZ_FRAME_INTERACTIONS | SZ_FRAME_SUBPOINTS; to be
     called after sz_set_floe_output, which resets them to 0; frees that writer's frames.  Their sections lie behind the column sections: the
     layout of a frame without lists is what it was, and a writer without lists costs no launch, scan or synchronisation more.  With the lists
     a frame is everything a Floe holds on the device at write_data! time: a fresh context can be restarted from it.
     INTERACTIONS: inter_off int32 [M + 1] and rows double [R][7].  A parent row carries floe.interactions of the last step that ran, with the
     bits sz_download_interactions gives at that cut BEFORE sz_add_ghosts: the floeidx column as the reference stores it -- a partner that was
     an inline ghost of that step is N + the rank of its order key among that step's ghost keys + 1; where that call would translate nothing
     (a process-mode call ran since, the host uploaded the rows) the rows are kept untranslated, as it would.  A ghost row's span is empty:
     deepcopy_floe (floe_utils.jl:120-161) passes no interactions, the copy gets zeros(0, 7) and num_inters = 0.
     SUB-FLOE POINTS: sub_off int32 [M + 1], sx, sy [S], centred as stored: a parent row's own points with the bits of sz_download_subpoints; a
     ghost row carries its parent's (deepcopy_floe copies them).
     status.fuse_idx has no section: it is non-empty only on a row tagged `fuse` (collisions.jl:367-368, 801-806), and a batch that honours tags
     never begins a step with such a row -- the recorded status column says so.
     Refusals: bits other than the two, SZ_E_ARG; a writer that is off, SZ_E_STATE; a tiled context or a writer of sz_tile_set_floe_output,
     SZ_E_STATE (tile frames record no lists yet through this setter: sz_tile_set_floe_output_lists, below).  The room check of a frame uses
     its full size, lists included.
   sz_set_grid_output: the arguments of sz_eulerian_data (evenly spaced grid lines, nout >= 1 of the SZ_EUL_* codes) and room for max_frames
     frames.  A GRID FRAME is the nout * nx * ny doubles sz_eulerian_data gives on the same list, bit for bit, and its timestep.  The averages run
     in a workspace the recorder keeps (sized when the writer is set, grown on demand): a recorded output step allocates nothing once warm.
   A frame that finds no room -- the arena, the max_frames + 1-th grid frame -- is not taken and no writer gets a frame of that step: the batch
   ends in front of it with SZ_OK, *steps_done not counting it, and `full` set until the next sz_step or sz_clear_frames.
   Draining: sz_output_frames: frames held per writer (n_floe, n_grid: 4 entries each, may be NULL) and full.  sz_floe_frame_info: the header of
   floe frame k {tstep, M, N, n_ring_points, n_ghost_links}.  sz_download_floe_frame: every non-NULL member of cols that was recorded is filled
   (sized from sz_floe_frame_info; ghost_idx n_ghost_links entries; sub_off M + 1 and sx, sy n_sub_points entries, when the frame recorded
   the sub-floe points); a non-NULL member that was not recorded returns SZ_E_ARG and nothing is written.  sz_floe_frame_lists_info: the totals
   of frame k's list sections (0 for a section not recorded).  sz_download_floe_frame_interactions: the signature of sz_download_interactions,
   on frame k: off M + 1 entries, rows n_inter_rows * 7 (rows may be NULL); SZ_E_ARG on a frame without the section.  sz_download_grid_frame: tstep and data[nout][nx][ny] (either may be NULL).  A frame or writer
   that does not exist: SZ_E_ARG.  Frames survive sz_upload_floes, sz_splice_floes and sz_remove_floes, so a host that edits at a stop drains
   whenever it likes; they are freed by sz_clear_frames (all writers, the writers stay set), by setting that writer again and by sz_destroy. */
int sz_set_floe_output(sz_ctx *ctx, int32_t writer, int32_t dt_out, uint64_t columns_mask, int64_t arena_bytes);
enum { SZ_FRAME_INTERACTIONS = 1, SZ_FRAME_SUBPOINTS = 2 };
int sz_set_floe_output_lists(sz_ctx *ctx, int32_t writer, uint32_t lists);
int sz_set_grid_output(sz_ctx *ctx, int32_t writer, int32_t dt_out, int32_t nx, int32_t ny, const double *xg, const double *yg,
                       int32_t nout, const int32_t *outputs, int32_t max_frames);
int sz_output_frames(sz_ctx *ctx, int32_t *n_floe, int32_t *n_grid, int32_t *full);
int sz_floe_frame_info(sz_ctx *ctx, int32_t writer, int32_t k, int64_t *tstep, int64_t *M, int64_t *N, int64_t *n_ring_points,
                       int64_t *n_ghost_links);
int sz_download_floe_frame(sz_ctx *ctx, int32_t writer, int32_t k, sz_floe_columns *cols);
int sz_floe_frame_lists_info(sz_ctx *ctx, int32_t writer, int32_t k, int64_t *n_inter_rows, int64_t *n_sub_points);
int sz_download_floe_frame_interactions(sz_ctx *ctx, int32_t writer, int32_t k, int32_t *off, double *rows);
int sz_download_grid_frame(sz_ctx *ctx, int32_t writer, int32_t k, int32_t *tstep, double *data);
int sz_clear_frames(sz_ctx *ctx);

/* ---- output frames of a tiled run (csrc/sz_record_tile.hpp; DESIGN.md §9i, "Tiled contexts"): with a writer set through the two setters below
   sz_tile_run cuts its batch before every output step and records there, collectively, and goes on -- the rule at the ends, `full`, the limits
   and the draining calls are the single context's, above.  The setters take the single setters' arguments and checks, are local, are to be
   called alike on every rank, and need a tiled context (sz_tile_enable; SZ_E_STATE otherwise: a single context takes sz_set_floe_output).
   Writers set through them do not stop sz_tile_enable, so they and their frames survive a re-tile, sz_tile_migrate, sz_tile_splice_floes and
   sz_tile_remove_floes; they are cleared and freed as on the single context.
   At a record point: halo rows and ghosts are dropped, sz_add_ghosts makes the ghosts of the OWNED parents (which ghosts a parent gets depends
   on that parent alone), ONE all-gather of {error / full bits, M, N, n_ring_points} per rank, one pack launch per due floe writer; with a grid
   writer due, ONE all-reduce over the per-cell sums of all grid writers due at that step; sz_remove_ghosts.  An error of one rank is every
   rank's.  If any rank has no room for any due frame no rank records that step: every rank ends in front of it with SZ_OK and `full` set.
   A TILE FLOE FRAME is the floe frame above over the rank's own rows -- its owned parents, then their ghosts; ghost_idx in local row numbers --
   with every row's ORDER KEY kept beside it: a parent's key is its global number, a ghost's (pass << 40) + 4 * parent key + k.  The rows of all
   ranks sorted by key are the single context's frame of that step, bit for bit in every section.  A GRID FRAME is held by every rank: the sums
   over the ranks differ from the single context's serial sums by round-off (two ranks: by the order of one addition, i.e. not at all).
   The single context's calls work on a tiled context as they are, locally: sz_output_frames, sz_floe_frame_info (local counts),
   sz_download_floe_frame (the tile frame: local rows), sz_download_grid_frame, sz_clear_frames.
   sz_tile_floe_frame_keys: the M order keys of tile frame k (local).  sz_tile_floe_frame_info: the header of the MERGED frame -- global counts,
   from the ranks' counts kept with the frame at the record point; local, no rank waits for another.  sz_tile_download_floe_frame: the merged
   frame, in the members of cols as sz_download_floe_frame fills them, sized from sz_tile_floe_frame_info.  COLLECTIVE: every rank calls it for
   the same writer and k; cols may be NULL on a rank that only takes part.  What a rank prepares alone (the frame exists, the members were
   recorded, its scratch) is agreed before the gather: an error of one rank is returned by every rank, nobody is left waiting.  The frames
   travel between device buffers (RCCL) and are merged on the device; the merged frame comes down in one copy.
   sz_tile_run refuses, with SZ_E_STATE and no step run: writers whose settings differ between the ranks (one gather of a digest, before any
   other collective: the message names the writer); two-way coupling with a tile writer set; a context without sz_tile_setup and a
   communicator.  sz_step on a context with tile writers set returns SZ_E_STATE: sz_tile_run records.
   THE LISTS IN TILE FRAMES.  sz_tile_set_floe_output_lists: sz_set_floe_output_lists for a writer of sz_tile_set_floe_output (called after it,
   which resets the lists; frees the writer's frames; the same word on every rank: it is part of the digest).  SZ_E_ARG: unknown bits, a bad
   writer; SZ_E_STATE: a writer that is off or was not set through the tile setter.  The merged frame of a tiled run with lists is the single
   context's frame with lists of the same step, bit for bit, the list sections included.  A tile frame then carries, behind its keys: the sorted
   order keys of the rows the LAST step had behind the owned parents (halo floes, their ghosts, the owned floes' ghosts; interactions only) and
   the single frame's list sections over its own rows -- a ghost row its parent's points and no interactions; the partner column UNTRANSLATED: a
   floe's global number + 1, or the order key + 1 of a ghost of the last step (> 2^40), or a negative boundary / topography code.  The merge
   turns a key + 1 into N_global + (rank of the key among the sorted DISTINCT ghost keys of all ranks' tables) + 1 -- the single context's
   number, since the union of the ranks' ghosts of a step is its ghost list of that step; a key found nowhere stays.  The record point adds
   {R, S, table entries, rows-lost} to its one all-gather, and no other collective.  WHERE THE ROWS ARE NOT THE LAST STEP'S on some rank -- a
   frame recorded behind sz_tile_migrate (which drops the rows) before a collision step has run, or behind a list-based tile step (sz_tile_step,
   a ridge / raft step: its ghost keys are not kept) -- every rank records that frame with SZ_FRAME_INTERACTIONS cleared in its `lists` word;
   the points are still recorded.  sz_tile_floe_frame_lists_info (local): the `lists` word of frame k and the MERGED frame's totals.
   sz_tile_download_floe_frame fills sub_off / sx / sy when asked for and recorded.  sz_tile_download_floe_frame_interactions: COLLECTIVE, the
   signature of sz_download_floe_frame_interactions on the merged frame (off M + 1, rows n_inter_rows * 7); off and rows may be NULL on a rank
   that only takes part; a frame whose interactions bit was cleared returns SZ_E_STATE on every rank, the message naming the migration (or the
   list-based step); a frame of a writer without the list SZ_E_ARG.  The local calls work on a tile frame with lists: sz_floe_frame_lists_info
   and sz_download_floe_frame give this rank's own totals and points, sz_download_floe_frame_interactions its rows with the partner column
   untranslated, sz_tile_floe_frame_list_keys the key table (*n entries; keys may be NULL). */
int sz_tile_set_floe_output(sz_ctx *ctx, int32_t writer, int32_t dt_out, uint64_t columns_mask, int64_t arena_bytes);
int sz_tile_set_grid_output(sz_ctx *ctx, int32_t writer, int32_t dt_out, int32_t nx, int32_t ny, const double *xg, const double *yg,
                            int32_t nout, const int32_t *outputs, int32_t max_frames);
int sz_tile_floe_frame_keys(sz_ctx *ctx, int32_t writer, int32_t k, int64_t *keys);
int sz_tile_floe_frame_info(sz_ctx *ctx, int32_t writer, int32_t k, int64_t *tstep, int64_t *M, int64_t *N, int64_t *n_ring_points,
                            int64_t *n_ghost_links);
int sz_tile_download_floe_frame(sz_ctx *ctx, int32_t writer, int32_t k, sz_floe_columns *cols);
int sz_tile_set_floe_output_lists(sz_ctx *ctx, int32_t writer, uint32_t lists);
int sz_tile_floe_frame_lists_info(sz_ctx *ctx, int32_t writer, int32_t k, uint32_t *lists, int64_t *n_inter_rows, int64_t *n_sub_points);
int sz_tile_download_floe_frame_interactions(sz_ctx *ctx, int32_t writer, int32_t k, int32_t *off, double *rows);
int sz_tile_floe_frame_list_keys(sz_ctx *ctx, int32_t writer, int32_t k, int64_t *n, int64_t *keys);

/* test hook: which_vertices_match_points(points, region) (floe_utils.jl:331-352) as the narrow phase evaluates it, on
   given points (<= 64) and a given closed region ring; idx = sorted 0-based vertex indices */
int sz_debug_match_vertices(sz_ctx *ctx, int32_t npts, const double *px, const double *py, int32_t nr, const double *rx,
                            const double *ry, int32_t *idx, int32_t *n_out);

/* test hook: the in-bounds test of calc_subfloe_values! (in_bounds, coupling.jl:494-597) and the lattice sample of mc_interpolation
   (find_interp_knots + linear_interpolation, coupling.jl:702-902) as the forcing kernels evaluate them, at n given points.
   out12[12 k ..] = in_bounds (0 / 1), uocn, vocn, hflx, uatm, vatm, the 1-based grid lines west, east, south, north the bilinear
   blend reads, its weights tx, ty.  Needs sz_set_domain and sz_set_fields. */
int sz_debug_sample_fields(sz_ctx *ctx, int32_t n, const double *x, const double *y, double *out12);

/* test hook: 1 when the last sz_step batch ran as pipelined steps (two launches per timestep: csrc/sz_pipeline.hpp), 0 otherwise; with an
   output writer set (sz_set_floe_output / sz_set_grid_output): 1 when any of the segments between its cuts did */
int sz_debug_pipelined(sz_ctx *ctx);
/* test hook: where the last sz_step batch took collision_force, collision_trq, overarea and the stress sums from: 0 the serial double sums of
   the row assembly (process mode's; batches with collisions off), 1 the fixed-point totals with the rows assembled inside every step, 2 the
   fixed-point totals with the rows of the batch's last step assembled once behind it */
int sz_debug_totals_mode(sz_ctx *ctx);
/* test hook: the arithmetic of the fixed-point totals (csrc/sz_geom.hpp: fx_force_exp, fx_lever_exp, fx_area_exp, fx_split, fx_join) on given
   numbers, by the device functions the step kernels call; no floe is needed.  Thread t of nthreads (1..1024) splits the values
   v[perm[t]], v[perm[t + nthreads]], ... (n <= 4096, perm a permutation of 0..n-1) at exponent E, sums its words and adds them to ONE pair of
   words with the narrow phase's atomics.  E by mode & 7: 0 the argument e; 1 fx_force_exp(kexp = e, area, height); 2 that + fx_lever_exp(rmax);
   3 fx_area_exp(area); 4 fx_lever_exp(rmax); with mode & 8 kexp is the context's own (from the E and mu of sz_set_params) instead of e.
   words2 = { sum of the high words, sum of the low words }, flags2 = { 1 if a value was out of range (it adds nothing), E },
   joined = fx_join(words2, E). */
int sz_debug_fx_totals(sz_ctx *ctx, int32_t n, const double *v, const int32_t *perm, int32_t nthreads, int32_t mode, int32_t e, double area,
                       double height, double rmax, int64_t *words2, int32_t *flags2, double *joined);
/* test hook: what one interaction row row5 = { xforce, yforce, xpoint, ypoint, overlap } adds to the totals of a floe with centroid (cx, cy)
   (fx_word; sign +1: the pair's first floe, -1: its second) at force, area and lever exponents eF, eA, eL: words14 = the high words
   0 xforce, 1 yforce, 2 (x-cx) fx, 3 (y-cy) fx, 4 (x-cx) fy, 5 (y-cy) fy, 6 overlap, then their seven low words; bad: 1 if one was out of range */
int sz_debug_fx_word(sz_ctx *ctx, const double *row5, double sign, double cx, double cy, int32_t eF, int32_t eA, int32_t eL, int64_t *words14,
                     int32_t *bad);
/* diagnostic build (-DSZ_STAMPS) only: stamp log of one lane group of the narrow phase
   (out512[0] = entries, then (stage << 48) | cycles since the wave started) */
int sz_debug_stamps(sz_ctx *ctx, long long *out512);
/* test hook: parts of the collision records (the per-floe 128-byte cache of the columns the neighbour search and the narrow phase read;
   DESIGN.md section 3.00) of the owned parents that differ from the columns after the last resident batch -- 0 expected; -1: that batch
   did not run on records */
int sz_debug_crec_mismatches(sz_ctx *ctx, int64_t *n_bad);
/* test hook: the cutter of the stop schedule that sz_step and sz_tile_run share (csrc/sz_stops.hpp), with no context and no device call.  The
   segment that starts at timestep tstep with `remaining` steps of the batch left, for RidgeRaftSettings.Δt rr_dt (0: off), FractureSettings.Δt
   frac_dt (0: no criterion), the n_weld WeldSettings.Δts and cut_on_fracture (1: segments end on fracture steps too, as on tiled contexts):
   out4 = { 1 if it is a ridge / raft step, its length, 1 if its last step is a fracture step, that step's welding set or -1 }. */
int sz_debug_next_segment(int32_t tstep, int32_t remaining, int32_t rr_dt, int32_t frac_dt, int32_t cut_on_fracture, int32_t n_weld,
                          const int32_t *weld_dts, int32_t *out4);
/* ... the same cutter with the output intervals of registered writers: n_out entries out_dts (0: that writer is off), a segment also ends
   BEFORE every step that is an output step of one of them.  With n_out = 0 every answer is sz_debug_next_segment's. */
int sz_debug_next_segment_out(int32_t tstep, int32_t remaining, int32_t rr_dt, int32_t frac_dt, int32_t cut_on_fracture, int32_t n_weld,
                              const int32_t *weld_dts, int32_t n_out, const int32_t *out_dts, int32_t *out4);
/* test hook: the columns of sz_floe_columns in the order the engine's tables hold them (csrc/sz_columns.hpp) -- the scalar columns, then the
   tensors, as the member names of the struct above, space-separated; no context and no device call */
const char *sz_debug_column_names(void);
/* test hook: the bits of sz_set_floe_output's columns_mask in order, bit 0 first, space-separated: the names above, then id, ghost_id, status,
   rings (vert_off + vx + vy) and ghost_links (ghost_off + ghost_idx); no context and no device call */
const char *sz_debug_frame_bits(void);

#ifdef __cplusplus
}
#endif
#endif

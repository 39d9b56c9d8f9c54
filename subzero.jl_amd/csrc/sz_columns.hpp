// sz_columns.hpp — the columns of a floe and the layout of a migration record, stated ONCE.  A column is added HERE (and to the hand-written lists
// that cannot include this file: DESIGN.md §2 names them); everything that moves floe rows -- upload, download, migration, removal, the row edits
// and their Float32 twins -- builds its tables from the two X-macros and names the slots of a record by the constants below.
//
// Needs include/subzero_hip.h and the standard library only: no HIP call, so a host program can compile it on its own (tools/columns_f32_check.cpp).
// The constants are constexpr and so usable in kernels; the table builders take the device state as a template argument (State, sz_state.hpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../include/subzero_hip.h"

// X(member of sz_floe_columns / sz_floe_columns_f32, member of State), in the order of a migration record: one double per floe ...
#define SZ_SCALAR_COLUMNS(X) \
  X(cx, cx) X(cy, cy) X(rmax, rmax) X(area, area) X(height, height) X(mass, mass) X(moment, moment) X(alpha, alpha) X(u, u) X(v, v) X(xi, xi) \
  X(p_dxdt, p_dxdt) X(p_dydt, p_dydt) X(p_dalphadt, p_dalphadt) X(p_dudt, p_dudt) X(p_dvdt, p_dvdt) X(p_dxidt, p_dxidt) \
  X(fxOA, fxOA) X(fyOA, fyOA) X(trqOA, trqOA) X(hflx_factor, hflx) X(overarea, overarea) X(coll_fx, cfx) X(coll_fy, cfy) X(coll_trq, ctrq)
// ... and the 2 x 2 tensors, four doubles per floe
#define SZ_TENSOR_COLUMNS(X) X(stress_accum, sa) X(stress_instant, si) X(strain, strain)
#define SZ_ALL_COLUMNS(X) SZ_SCALAR_COLUMNS(X) SZ_TENSOR_COLUMNS(X)

namespace sz {

#define X(host, state) + 1
constexpr int MIG_NSC = 0 SZ_SCALAR_COLUMNS(X);       // scalar columns
constexpr int MIG_NTEN = 0 SZ_TENSOR_COLUMNS(X);      // tensors
#undef X
constexpr int MIG_NTAB = MIG_NSC + MIG_NTEN;          // entries of a column table: the scalars, then the tensors
constexpr int MIG_TAB_CAP = (MIG_NTAB + 7) / 8 * 8;   // pointers of the device copy of a table (what the row movers allocate for it)

// ---- a migration record (sz_migrate.hpp), in doubles: the scalars, the tensors, then
constexpr int MIG_TEN = MIG_NSC;                      // component q of tensor t at MIG_TEN + 4 t + q
constexpr int MIG_ID = MIG_TEN + 4 * MIG_NTEN;
constexpr int MIG_STATUS = MIG_ID + 1;
constexpr int MIG_NGATHER = MIG_STATUS + 1;           // the leading doubles the column gather moves (sz_k_mig_gather / sz_k_mig_scatter): up to the status
constexpr int MIG_GIDX = MIG_NGATHER;                 // global index: the order key of the floe
constexpr int MIG_NV = MIG_GIDX + 1;                  // ring points
constexpr int MIG_NS = MIG_NV + 1;                    // sub-floe points
constexpr int MIG_NCOL = MIG_NS + 1;                  // doubles of a record before its ring
// ---- the staging buffer of sz_download_rows (sz_splice.hpp), column q of selected row k at q n + k: the gathered doubles, then
constexpr int SP_NCOL = MIG_NGATHER;
constexpr int SP_GHOST_ID = SP_NCOL;
constexpr int SP_PACK_NCOL = SP_GHOST_ID + 1;

// the wire format as it stands; a change of the layout is made on purpose, here
static_assert(MIG_NSC == 25 && MIG_ID == 37 && MIG_STATUS == 38 && MIG_GIDX == 39 && MIG_NV == 40 && MIG_NS == 41 && MIG_NCOL == 42, "migration record layout");
static_assert(SP_NCOL == 39 && SP_PACK_NCOL == 40 && MIG_TAB_CAP == 32, "staging buffer layout");
static_assert(MIG_NCOL <= 64, "one lane of a wavefront per slot of a record (sz_k_mig_pack, sz_k_sp_pack)");

// COL_cx, COL_cy, ...: the slot of a column by its host name, for the few places that read one column of a record or a table
#define X(host, state) COL_##host,
enum { SZ_ALL_COLUMNS(X) COL_END };
#undef X
// the hand-written structs of the public header hold the columns in the macros' order, from offset 0
#define X(host, state) \
  static_assert(offsetof(sz_floe_columns, host) == COL_##host * sizeof(double*), "sz_floe_columns: " #host " out of order"); \
  static_assert(offsetof(sz_floe_columns_f32, host) == COL_##host * sizeof(float*), "sz_floe_columns_f32: " #host " out of order");
SZ_ALL_COLUMNS(X)
#undef X

// the host names, scalars then tensors, each with a space in front (sz_debug_column_names)
#define X(host, state) " " #host
constexpr char COLUMN_NAMES[] = SZ_ALL_COLUMNS(X);
#undef X

// ---- column tables: entry k is column k of a record (k < MIG_NSC), tensor k - MIG_NSC behind them; col_width(k) doubles per floe
template <class T> struct ColTable { T p[MIG_NTAB]; };
constexpr size_t col_width(int k) { return k < MIG_NSC ? 1 : 4; }
#define SZ_STATE_COLUMN(host, state) S.state,          // (handed to the list with a & in front: the address of each member)
#define SZ_HOST_COLUMN(host, state) f.host,
// the device columns of a State, and where the State keeps their addresses (the allocation loop of sz_upload_floes)
template <class St> inline ColTable<double*> state_columns(const St& S) { return { { SZ_ALL_COLUMNS(SZ_STATE_COLUMN) } }; }
template <class St> inline ColTable<double**> state_column_slots(St& S) { return { { SZ_ALL_COLUMNS(&SZ_STATE_COLUMN) } }; }
// the host's columns: to read, to fill, and the members themselves
inline ColTable<const double*> host_columns(const sz_floe_columns& f) { return { { SZ_ALL_COLUMNS(SZ_HOST_COLUMN) } }; }
inline ColTable<double*> host_columns(sz_floe_columns& f) { return { { SZ_ALL_COLUMNS(SZ_HOST_COLUMN) } }; }
inline ColTable<double**> host_column_slots(sz_floe_columns& f) { return { { SZ_ALL_COLUMNS(&SZ_HOST_COLUMN) } }; }

// ---- Float32 hosts (sz_floe_columns_f32): every _f32 entry point widens on the way in and rounds on the way out through these two.
// The counts are the caller's: floes, ring points, sub-floe points, doubles of the interaction rows that go with them.  A NULL column stays NULL;
// the integer columns and the offsets pass through as they are.
struct F32Up {          // an owned Float64 copy of *f: d (and ir) go to the Float64 call
  std::vector<std::vector<double>> keep;
  sz_floe_columns d; const double* ir;
  F32Up(const sz_floe_columns_f32* f, size_t rows, size_t ring, size_t sub, const float* inter = nullptr, size_t n_inter = 0) {
    memset(&d, 0, sizeof(d));
#define X(host, state) d.host = widen(f->host, col_width(COL_##host) * rows);
    SZ_ALL_COLUMNS(X)
#undef X
    d.id = f->id; d.ghost_id = f->ghost_id; d.status = f->status; d.vert_off = f->vert_off; d.sub_off = f->sub_off; d.ghost_off = f->ghost_off; d.ghost_idx = f->ghost_idx;
    d.vx = widen(f->vx, ring); d.vy = widen(f->vy, ring); d.sx = widen(f->sx, sub); d.sy = widen(f->sy, sub);
    ir = widen(inter, n_inter);
  }
  double* widen(const float* src, size_t n) {
    if (!src) return nullptr;
    keep.emplace_back(n ? n : 1);
    for (size_t k = 0; k < n; k++) keep.back()[k] = (double)src[k];
    return keep.back().data();
  }
};
// sx / sy of a download: a row download brings them; a whole-list download does not write them (sz_download_subpoints is their way back), so they
// are not staged and the caller's buffers are left alone -- staging them handed zeros back
enum F32Sub { F32_STAGE_SUB, F32_LEAVE_SUB };
struct F32Down {        // Float64 room for what a download brings: d (and ir) go to the Float64 call, back() rounds into *f
  std::vector<std::vector<double>> keep;
  struct Back { float* dst; const double* src; size_t n; }; std::vector<Back> todo;
  sz_floe_columns d; double* ir;
  F32Down(sz_floe_columns_f32* f, size_t rows, size_t ring, size_t sub, F32Sub sub_rule, float* inter = nullptr, size_t n_inter = 0) {
    memset(&d, 0, sizeof(d));
#define X(host, state) d.host = room(f->host, col_width(COL_##host) * rows);
    SZ_ALL_COLUMNS(X)
#undef X
    d.id = f->id; d.ghost_id = f->ghost_id; d.status = f->status; d.vert_off = f->vert_off; d.sub_off = f->sub_off; d.ghost_off = f->ghost_off; d.ghost_idx = f->ghost_idx;
    d.vx = room(f->vx, ring); d.vy = room(f->vy, ring);
    if (sub_rule == F32_STAGE_SUB) { d.sx = room(f->sx, sub); d.sy = room(f->sy, sub); }
    ir = room(inter, n_inter);
  }
  double* room(float* dst, size_t n) {
    if (!dst) return nullptr;
    keep.emplace_back(n ? n : 1);
    todo.push_back({ dst, keep.back().data(), n });
    return keep.back().data();
  }
  void back() const { for (const Back& b : todo) for (size_t k = 0; k < b.n; k++) b.dst[k] = (float)b.src[k]; }
};

}  // namespace sz

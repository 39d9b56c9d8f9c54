// Host check of the Float32 helpers of csrc/sz_columns.hpp (F32Up, F32Down), with no HIP and no library: a sz_floe_columns_f32 of six floes, of no
// floe, and with columns left NULL is widened and rounded back, and every value is compared with what went in.  Meant to run under the sanitizers
// (tools/README.md has the command); exit status 0 and "ok" when everything holds.
#include <cstdio>
#include "../subzero.jl_amd/csrc/sz_columns.hpp"

using namespace sz;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { failures++; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

// a host list of n floes: 5 ring points and 2 sub-floe points a floe, 3 interaction rows in all; column k of floe i holds 8 k + i + 0.5
struct Host {
  size_t n, V, NS, R;
  std::vector<float> col[MIG_NTAB], vx, vy, sx, sy, inter;
  std::vector<int64_t> id; std::vector<int32_t> status, voff, soff;
  sz_floe_columns_f32 f;
  Host(size_t n_, bool sparse) : n(n_), V(5 * n_), NS(2 * n_), R(n_ ? 3 : 0) {
    for (int k = 0; k < MIG_NTAB; k++) { col[k].reserve(4 * n + 1); col[k].resize((k < MIG_NSC ? 1 : 4) * n); for (size_t i = 0; i < col[k].size(); i++) col[k][i] = 8.0f * k + (float)i + 0.5f; }
    // (reserve: never NULL, with no floe either)
    auto fill = [](std::vector<float>& v, size_t m, float base) { v.reserve(m + 1); v.resize(m); for (size_t i = 0; i < m; i++) v[i] = base + (float)i; };
    fill(vx, V, 1000.f); fill(vy, V, 2000.f); fill(sx, NS, 3000.f); fill(sy, NS, 4000.f); fill(inter, 7 * R, 5000.f);
    id.resize(n); status.assign(n, SZ_ACTIVE); voff.resize(n + 1); soff.resize(n + 1);
    for (size_t i = 0; i <= n; i++) { voff[i] = (int32_t)(5 * i); soff[i] = (int32_t)(2 * i); if (i < n) id[i] = 101 + 7 * (int64_t)i; }
    memset(&f, 0, sizeof(f));
    int k = 0;
#define X(host, state) f.host = (sparse && k % 3 == 1) ? nullptr : col[k].data(); k++;
    SZ_ALL_COLUMNS(X)
#undef X
    f.id = id.data(); f.status = sparse ? nullptr : status.data(); f.vert_off = voff.data(); f.vx = vx.data(); f.vy = vy.data();
    f.sub_off = soff.data(); f.sx = sx.data(); f.sy = sparse ? nullptr : sy.data();
  }
};

static void copy(double* dst, const double* src, size_t m) { if (dst && m) memcpy(dst, src, m * sizeof(double)); }
static void same(const double* d, const float* s, size_t m) {
  CHECK((d == nullptr) == (s == nullptr));
  if (d && s) for (size_t i = 0; i < m; i++) CHECK(d[i] == (double)s[i]);
}

static void round_trip(size_t n, bool sparse) {
  Host in(n, sparse), out(n, sparse);
  // ---- up: an owned Float64 copy, NULL where the host gave NULL, the integer columns passed through
  const F32Up up(&in.f, in.n, in.V, in.NS, in.inter.data(), 7 * in.R);
  const ColTable<const double*> wide = host_columns(up.d);
  int k = 0;
#define X(host, state) same(wide.p[k], in.f.host, (k < MIG_NSC ? 1 : 4) * n); CHECK(wide.p[k] == up.d.host); k++;
  SZ_ALL_COLUMNS(X)
#undef X
  same(up.d.vx, in.f.vx, in.V); same(up.d.vy, in.f.vy, in.V); same(up.d.sx, in.f.sx, in.NS); same(up.d.sy, in.f.sy, in.NS); same(up.ir, in.inter.data(), 7 * in.R);
  CHECK(up.d.id == in.f.id && up.d.status == in.f.status && up.d.vert_off == in.f.vert_off && up.d.sub_off == in.f.sub_off && up.d.ghost_off == nullptr);
  // ---- down: Float64 room that a download fills (here: with the widened values), rounded back into a host list that holds other values
  for (int q = 0; q < MIG_NTAB; q++) for (float& v : out.col[q]) v = -1.f;
  for (std::vector<float>* v : { &out.vx, &out.vy, &out.sx, &out.sy, &out.inter }) for (float& x : *v) x = -1.f;
  for (const F32Sub rule : { F32_STAGE_SUB, F32_LEAVE_SUB }) {
    F32Down down(&out.f, out.n, out.V, out.NS, rule, out.inter.data(), 7 * out.R);
    const ColTable<double*> room = host_columns(down.d);
    for (int q = 0; q < MIG_NTAB; q++) {
      CHECK((room.p[q] == nullptr) == (wide.p[q] == nullptr));
      copy(room.p[q], wide.p[q], (q < MIG_NSC ? 1 : 4) * n);
    }
    copy(down.d.vx, up.d.vx, in.V); copy(down.d.vy, up.d.vy, in.V); copy(down.ir, up.ir, 7 * in.R);
    CHECK(rule == F32_STAGE_SUB ? down.d.sx != nullptr && (down.d.sy != nullptr) == !sparse : !down.d.sx && !down.d.sy);
    copy(down.d.sx, up.d.sx, in.NS); copy(down.d.sy, up.d.sy, in.NS);
    down.back();
    for (int q = 0; q < MIG_NTAB; q++) for (size_t i = 0; i < out.col[q].size(); i++) CHECK(out.col[q][i] == (wide.p[q] ? in.col[q][i] : -1.f));
    CHECK(out.vx == in.vx && out.vy == in.vy && out.inter == in.inter);
    if (rule == F32_STAGE_SUB) {          // a row download brings the points; what the next rule must leave alone is put in their place
      CHECK(out.sx == in.sx);
      for (size_t i = 0; i < out.NS; i++) CHECK(out.sy[i] == (sparse ? -1.f : in.sy[i]));
      for (float& x : out.sx) x = -2.f;
      for (float& x : out.sy) x = -2.f;
    } else {
      for (size_t i = 0; i < out.NS; i++) CHECK(out.sx[i] == -2.f && out.sy[i] == -2.f);
    }
  }
}

int main() {
  static_assert(MIG_NSC == 25 && MIG_NTAB == 28, "the columns of include/subzero_hip.h");
  CHECK(strncmp(COLUMN_NAMES, " cx cy rmax ", 12) == 0);
  for (const bool sparse : { false, true }) { round_trip(6, sparse); round_trip(0, sparse); }
  std::printf(failures ? "%d checks failed\n" : "ok\n", failures);
  return failures ? 1 : 0;
}

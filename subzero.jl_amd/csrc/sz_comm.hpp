// sz_comm.hpp — the channel between the ranks of a tiled run: the run-time RCCL binding, the host's transport in its place, the small
// collectives built on either (all-gather, agreements, the variable-size all-to-all) with the layout of their device scratch, and the
// sz_comm_* entry points.  Host code of the one translation unit sz_api.hip; what the tiles do over the channel is sz_tile_host.hpp.
#pragma once
#include <dlfcn.h>

#include "sz_ctx.hpp"

// ---------------------------------------------------------------- the halo exchange inside the library (RCCL over xGMI)
// "library owns device buffers, streams, RCCL communicators inside the opaque sz_ctx".  A host that is not
// Python (the reference's is Julia: one process per GPU, e.g. under MPI.jl) drives a tiled run with
//     sz_comm_unique_id (rank 0)  ->  the 128 bytes to every rank by any host channel  ->  sz_comm_init
//     sz_upload_floes (the owned floes) / sz_tile_enable  ->  sz_tile_setup  ->  sz_tile_run(nsteps) on every rank.
// Per step: pack kernel -> grouped ncclSend / ncclRecv with the NEIGHBOUR tiles only (the all-to-all-v of the halo records;
// a peer's region carries its real count in the header record and is sized per pair from the counts at the last box gather)
// on a second stream, beside the forcings of the owned floes -> unpack + the ordinary step.  The boxes are gathered again
// (ncclAllGather) every `rebox_every` steps; a floe that out-runs the drift margin in between raises ERR_HALO_DRIFT.
// RCCL is bound at run time (dlopen: the library has no link-time dependency on it, and a process that already holds an
// RCCL -- torch's -- shares that copy).
namespace {
struct UId { char b[128]; };
struct Rccl {
  void* h = nullptr;
  int (*GetUniqueId)(UId*) = nullptr;
  int (*CommInitRank)(void**, int, UId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
constexpr int NCCL_INT32 = 2, NCCL_FLOAT64 = 8, NCCL_SUM = 0;
bool rccl_load(std::string& err) {
  if (g_rccl.h) return true;
  if (getenv("SZ_RCCL_DISABLE")) { err = "RCCL binding switched off (SZ_RCCL_DISABLE)"; return false; }     // (to rehearse the callers' fallback)
  // an RCCL the process already holds comes first (a host framework's: two RCCL builds in one process each bring their own
  // runtime threads), then the system's
  const char* names[] = { "librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1" };
  for (const char* n : names) if ((g_rccl.h = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
  if (!g_rccl.h) for (const char* n : names) if ((g_rccl.h = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
  if (!g_rccl.h) { err = std::string("RCCL not found: ") + dlerror(); return false; }
#define RSYM(field, name) g_rccl.field = (decltype(g_rccl.field))dlsym(g_rccl.h, name); if (!g_rccl.field) { err = std::string("RCCL symbol missing: ") + name; g_rccl.h = nullptr; return false; }
  RSYM(GetUniqueId, "ncclGetUniqueId") RSYM(CommInitRank, "ncclCommInitRank") RSYM(CommDestroy, "ncclCommDestroy")
  RSYM(Send, "ncclSend") RSYM(Recv, "ncclRecv") RSYM(AllGather, "ncclAllGather") RSYM(AllReduce, "ncclAllReduce")
  RSYM(GroupStart, "ncclGroupStart") RSYM(GroupEnd, "ncclGroupEnd") RSYM(GetErrorString, "ncclGetErrorString")
#undef RSYM
  return true;
}
#define NCCLCHK(ctx, call)                                                                             \
  do {                                                                                                 \
    int r_ = (call);                                                                                   \
    if (r_ != 0) { (ctx)->err = std::string(#call) + ": " + g_rccl.GetErrorString(r_); return SZ_E_HIP; } \
  } while (0)

#define HOSTCHK(ctx, call, what)                                                                        \
  do {                                                                                                 \
    int r_ = (call);                                                                                   \
    if (r_ != 0) { (ctx)->err = std::string("host transport: ") + what + " returned " + std::to_string(r_); return SZ_E_HIP; } \
  } while (0)

// all-gather of `bytes` per rank between device buffers on the context's stream (host transport: through the host, synchronous)
int comm_allgather(sz_ctx* c, const void* d_src, void* d_dst, size_t count, int nccl_type, size_t elem) {
  const int n = c->comm_n;
  if (n == 1) { HIPCHK(c, hipMemcpyAsync(d_dst, d_src, count * elem, hipMemcpyDeviceToDevice, c->stream)); return SZ_OK; }
  if (!c->host_transport) { NCCLCHK(c, g_rccl.AllGather(d_src, d_dst, count, nccl_type, c->comm, c->stream)); return SZ_OK; }
  std::vector<char> hs(count * elem), hr(count * elem * n);
  HIPCHK(c, hipMemcpyAsync(hs.data(), d_src, hs.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HOSTCHK(c, c->host_tr.allgather(c->host_tr.user, hs.data(), hr.data(), (int64_t)hs.size()), "allgather");
  HIPCHK(c, hipMemcpyAsync(d_dst, hr.data(), hr.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}

// The device scratch of the small collectives, c->d_gather (sz_tile_setup allocates it; it lives as long as the communicator), in doubles:
//   OWN    this rank's record of the box gather (tile_rebox: box, rmax, drift, speed, spare)
//   ALL    the records of all ranks
//   MAT    the count matrix of the box gather (RANKS x RANKS ints; row s: what s sends to every d).  comm_sizes borrows this area between box
//          gathers: its own row at the start, the rows of all ranks RANKS ints behind it -- with 64 ranks the last of them runs into the words
//          of comm_gather_int, which are free while it runs, and ends short of the box centre
//   SPARE  64 doubles: the word of comm_gather_int (int 0), the words of all ranks (from int 32), the box centre of tile_rebox (double 48)
struct Gather {
  static constexpr int RANKS = 64, GB = 8;          // the most ranks of a communicator; doubles per rank in the box gather
  static constexpr int OWN = 0, ALL = OWN + GB, MAT = ALL + GB * RANKS, SPARE = MAT + RANKS * RANKS / 2, TOTAL = SPARE + 64;
  static constexpr int WORD = 2 * SPARE, WORDS = WORD + 32, CTR = SPARE + 48;          // (int*)d_gather + WORD / WORDS; d_gather + CTR
};
static_assert(Gather::ALL + Gather::GB * Gather::RANKS <= Gather::MAT && 2 * Gather::MAT + Gather::RANKS * Gather::RANKS <= 2 * Gather::SPARE, "the areas of d_gather overlap");
static_assert(Gather::WORD < Gather::WORDS && Gather::WORDS + Gather::RANKS <= 2 * Gather::CTR && Gather::CTR + 2 <= Gather::TOTAL, "the sub-uses of the spare doubles overlap");
static_assert(2 * Gather::MAT + Gather::RANKS + Gather::RANKS * Gather::RANKS <= 2 * Gather::CTR, "comm_sizes would reach the box centre");
static_assert(Gather::TOTAL == 8 + 8 * 64 + 64 * 64 / 2 + 64, "the size of d_gather has changed");

// one int of every rank (n <= 64), on every rank
int comm_gather_int(sz_ctx* c, int local, int* all64) {
  const int n = c->comm_n;
  all64[0] = local;
  if (n == 1) return SZ_OK;
  int *d = (int*)c->d_gather + Gather::WORD, *d_all = (int*)c->d_gather + Gather::WORDS;
  HIPCHK(c, hipMemcpyAsync(d, &local, sizeof(int), hipMemcpyHostToDevice, c->stream));
  int rc = comm_allgather(c, d, d_all, 1, NCCL_INT32, sizeof(int));
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(all64, d_all, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
// Collective: the OR of a word over the ranks.  Device errors (capacity bits, halo drift) are per rank and sticky; a rank that returned
// on its own while its peers went on into the next collective would leave them waiting forever (RCCL has no timeout).  Every point
// at which sz_tile_run looks at the error word therefore agrees on it first: all ranks return the same code at the same step.
int comm_agree_bits(sz_ctx* c, int local, int* all) {
  int h[64];
  if (const int rc = comm_gather_int(c, local, h)) return rc;
  int bits = 0, who = -1;
  for (int r = 0; r < c->comm_n; r++) { if (h[r] && who < 0) who = r; bits |= h[r]; }
  *all = bits;
  if (bits && !local) {
    char buf[200];
    snprintf(buf, sizeof(buf), "rank %d of the tiled run reported device error bits 0x%x (this rank is clean; all ranks stop together)", who, bits);
    c->err = buf;
  }
  return SZ_OK;
}
// "a floe of mine was tagged in this step", where an agreement carries it beside the error bits or on its own (the stop schedule, sz_stops.hpp)
constexpr int RRS_BIT_TAG = 1 << 30;
// The two words that decide how a tiled batch goes on -- the step a tag ended it at (C_STOP) and the step that paused for the largest narrow
// variant or a list that outgrew its capacity (C_RETRYSTOP) -- as ALL ranks must see them before anyone branches: the smallest non-zero
// value of each.  A rank's own counters are not enough: a pause on one rank and a tag on another in the SAME step are not heard by either
// (the unpack kernels of the next step return at their stop test before they read the peers' headers), and ranks that then take
// different branches wait for each other in different collectives.
int comm_agree_steps(sz_ctx* c, int stop_local, int pause_local, int* stop_all, int* pause_all) {
  int a[64], b[64];
  int rc = comm_gather_int(c, stop_local, a); if (rc) return rc;
  rc = comm_gather_int(c, pause_local, b); if (rc) return rc;
  int s = 0, p = 0;
  for (int r = 0; r < c->comm_n; r++) { if (a[r] > 0 && (s == 0 || a[r] < s)) s = a[r]; if (b[r] > 0 && (p == 0 || b[r] < p)) p = b[r]; }
  *stop_all = s; *pause_all = p;
  return SZ_OK;
}
// What a rank did on its own since the last collective came back with `local`: the first code a rank reports, in rank order, on EVERY rank
// (0: none) -- a rank that returned alone would leave its peers waiting in the next gather.  who: the caller, for the message.
// (tile_frac_pass sends its code in the slot of its owned count instead: one collective fewer.)
int comm_agree_rc(sz_ctx* c, const char* who, int local, int* first) {
  int h[64];
  if (const int r2 = comm_gather_int(c, local, h)) return r2;
  *first = 0;
  for (int r = 0; r < c->comm_n && !*first; r++) if (h[r]) { *first = h[r]; if (!local) c->err = std::string(who) + ": rank " + std::to_string(r) + " could not prepare the pass (all ranks return together)"; }
  return SZ_OK;
}
// One trade over the host's transport: per peer what goes out and what comes in (pointer and bytes each; a site names a peer with neither, or
// leaves it out, as the transport's pairing of the calls on both sides needs).  The five parallel arrays sz_host_transport::sendrecv takes.
struct HostTrade {
  std::vector<int32_t> peer; std::vector<const void*> sp; std::vector<void*> rp; std::vector<int64_t> sb, rb;
  void add(int d, const void* s, size_t s_bytes, void* r, size_t r_bytes) {
    peer.push_back(d);
    sp.push_back(s); sb.push_back((int64_t)s_bytes);
    rp.push_back(r); rb.push_back((int64_t)r_bytes);
  }
  int run(sz_ctx* c) {
    HOSTCHK(c, c->host_tr.sendrecv(c->host_tr.user, (int32_t)peer.size(), peer.data(), sp.data(), sb.data(), rp.data(), rb.data()), "sendrecv");
    return SZ_OK;
  }
};
// sizes of a variable-size all-to-all: mine[d] doubles go to rank d; all[s * n + d] = what rank s sends to rank d
int comm_sizes(sz_ctx* c, const std::vector<int>& mine, std::vector<int>& all) {
  const int n = c->comm_n;
  all.assign((size_t)n * n, 0);
  if (n == 1) { all[0] = mine[0]; return SZ_OK; }
  int* d_row = (int*)(c->d_gather + Gather::MAT);          // (the count-matrix area of the box gather: free between gathers)
  HIPCHK(c, hipMemcpyAsync(d_row, mine.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  int* d_all = d_row + Gather::RANKS;
  int rc = comm_allgather(c, d_row, d_all, (size_t)n, NCCL_INT32, sizeof(int));
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(all.data(), d_all, all.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
// variable-size all-to-all of doubles between the ranks: sendv[d] to rank d, recvv[s] (sized here) from rank s
int comm_alltoallv(sz_ctx* c, const std::vector<std::vector<double>>& sendv, std::vector<std::vector<double>>& recvv) {
  const int n = c->comm_n, me = c->comm_rank;
  recvv.assign(n, {});
  if (n == 1) return SZ_OK;
  // sizes first: every rank's row of the size matrix
  std::vector<int> mine(n), all;
  for (int d = 0; d < n; d++) mine[d] = (int)sendv[d].size();
  int rc = comm_sizes(c, mine, all);
  if (rc) return rc;
  for (int s2 = 0; s2 < n; s2++) if (s2 != me) recvv[s2].assign((size_t)all[(size_t)s2 * n + me], 0.0);
  if (c->host_transport) {
    HostTrade tr;
    for (int d = 0; d < n; d++) if (d != me) tr.add(d, sendv[d].data(), sendv[d].size() * sizeof(double), recvv[d].data(), recvv[d].size() * sizeof(double));
    return tr.run(c);
  }
  // RCCL: device staging buffers, one grouped send / receive
  size_t ts = 0, tr = 0;
  for (int d = 0; d < n; d++) { if (d == me) continue; ts += sendv[d].size(); tr += recvv[d].size(); }
  PoolGuard pool; double *ds = nullptr, *dr = nullptr;
  if ((rc = dalloc(c, &ds, ts, pool.v)) || (rc = dalloc(c, &dr, tr, pool.v))) return rc;
  size_t os = 0;
  for (int d = 0; d < n; d++) { if (d == me || sendv[d].empty()) continue; HIPCHK(c, hipMemcpyAsync(ds + os, sendv[d].data(), sendv[d].size() * sizeof(double), hipMemcpyHostToDevice, c->stream)); os += sendv[d].size(); }
  NCCLCHK(c, g_rccl.GroupStart());
  os = 0; size_t orr = 0;
  for (int d = 0; d < n; d++) {
    if (d == me) continue;
    if (!sendv[d].empty()) { NCCLCHK(c, g_rccl.Send(ds + os, sendv[d].size(), NCCL_FLOAT64, d, c->comm, c->stream)); os += sendv[d].size(); }
    if (!recvv[d].empty()) { NCCLCHK(c, g_rccl.Recv(dr + orr, recvv[d].size(), NCCL_FLOAT64, d, c->comm, c->stream)); orr += recvv[d].size(); }
  }
  NCCLCHK(c, g_rccl.GroupEnd());
  orr = 0;
  for (int d = 0; d < n; d++) { if (d == me || recvv[d].empty()) continue; HIPCHK(c, hipMemcpyAsync(recvv[d].data(), dr + orr, recvv[d].size() * sizeof(double), hipMemcpyDeviceToHost, c->stream)); orr += recvv[d].size(); }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SZ_OK;
}
// The record lists of all ranks, on every rank: cnt[r] records of `width` doubles from rank r, in as many slots per rank as the longest list
// needs (at least min_slots).  The caller carves, zeroes what its kernels expect zeroed, uploads the counts, packs d_rec, and gathers.
struct ListGather {
  int width, slots; long long total = 0;          // total: the records of all ranks
  double *d_rec = nullptr, *d_all = nullptr; int* d_cnt = nullptr;          // this rank's slots, those of all ranks, the 64 counts
  ListGather(const sz_ctx* c, const int* cnt, int width_, int min_slots) : width(width_), slots(min_slots) {
    for (int r = 0; r < c->comm_n; r++) { slots = std::max(slots, cnt[r]); total += cnt[r]; }
  }
  int carve(sz_ctx* c, Pool& P) {
    int rc;
    (void)((rc = dalloc(c, &d_rec, (size_t)width * slots, P)) || (rc = dalloc(c, &d_all, (size_t)width * slots * c->comm_n, P)) || (rc = dalloc(c, &d_cnt, 64, P)));
    return rc;
  }
  int upload_counts(sz_ctx* c, const int* cnt64) { HIPCHK(c, hipMemcpyAsync(d_cnt, cnt64, 64 * sizeof(int), hipMemcpyHostToDevice, c->stream)); return SZ_OK; }
  int gather(sz_ctx* c) { return comm_allgather(c, d_rec, d_all, (size_t)width * slots, NCCL_FLOAT64, sizeof(double)); }
};
}  // namespace

// can the RCCL binding be made in this process (run-time loading)?  Hosts ask on EVERY rank and agree on the answer over their own
// channel before the collective sz_comm_init: a rank that cannot bind would leave the others waiting inside ncclCommInitRank
int sz_comm_available(void) {
  std::string err;
  return rccl_load(err) ? SZ_OK : SZ_E_STATE;
}
int sz_comm_unique_id(void* id128) {
  std::string err;
  if (!id128 || !rccl_load(err)) return SZ_E_STATE;
  return g_rccl.GetUniqueId((UId*)id128) == 0 ? SZ_OK : SZ_E_HIP;
}
int sz_comm_init(sz_ctx* c, int32_t nranks, int32_t rank, const void* id128) {
  if (!c || nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks || (nranks > 1 && !id128)) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  (void)sz_comm_destroy(c);
  if (nranks > 1) {
    if (!rccl_load(c->err)) return SZ_E_STATE;
    UId id; memcpy(&id, id128, sizeof(id));
    NCCLCHK(c, g_rccl.CommInitRank(&c->comm, nranks, id, rank));
  }
  c->comm_n = nranks; c->comm_rank = rank;
  HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_recv, hipEventDisableTiming));
  return SZ_OK;
}
// the host's own channel instead of RCCL (include/subzero_hip.h: sz_host_transport)
int sz_comm_init_host(sz_ctx* c, int32_t nranks, int32_t rank, const sz_host_transport* t) {
  if (!c || nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks) return SZ_E_ARG;
  if (nranks > 1 && (!t || !t->allgather || !t->sendrecv || !t->allreduce_sum_f64)) { c->err = "sz_comm_init_host: the transport needs all three collectives"; return SZ_E_ARG; }
  (void)hipSetDevice(c->device);
  (void)sz_comm_destroy(c);
  if (nranks > 1) { c->host_tr = *t; c->host_transport = true; }
  c->comm_n = nranks; c->comm_rank = rank;
  HIPCHK(c, hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming));
  HIPCHK(c, hipEventCreateWithFlags(&c->ev_recv, hipEventDisableTiming));
  return SZ_OK;
}
// One-rank self test of the RCCL binding (the build box has one GPU, so the multi-rank exchange cannot run there): the
// run-time binding, ncclGetUniqueId / ncclCommInitRank with the id passed by value, an all-gather, an all-reduce and a
// grouped send / receive to self on the communication stream with the event hand-shake sz_tile_run uses.  Returns SZ_OK
// when every buffer holds what it should.
int sz_comm_selftest(sz_ctx* c) {
  if (!c) return SZ_E_ARG;
  (void)hipSetDevice(c->device);
  if (!rccl_load(c->err)) return SZ_E_STATE;
  UId id;
  NCCLCHK(c, g_rccl.GetUniqueId(&id));
  void* comm = nullptr;
  NCCLCHK(c, g_rccl.CommInitRank(&comm, 1, id, 0));
  hipStream_t cs = nullptr; hipEvent_t e0 = nullptr, e1 = nullptr;
  HIPCHK(c, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  HIPCHK(c, hipEventCreateWithFlags(&e0, hipEventDisableTiming)); HIPCHK(c, hipEventCreateWithFlags(&e1, hipEventDisableTiming));
  const int n = 4096;
  double* d = nullptr;
  HIPCHK(c, hipMalloc((void**)&d, (size_t)4 * n * sizeof(double)));
  std::vector<double> h((size_t)4 * n, 0.0);
  for (int k = 0; k < n; k++) h[k] = 1.0 + k;
  HIPCHK(c, hipMemcpyAsync(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(e0, c->stream));
  HIPCHK(c, hipStreamWaitEvent(cs, e0, 0));
  int rc = SZ_OK;
  NCCLCHK(c, g_rccl.GroupStart());
  NCCLCHK(c, g_rccl.Send(d, (size_t)n, NCCL_FLOAT64, 0, comm, cs));
  NCCLCHK(c, g_rccl.Recv(d + n, (size_t)n, NCCL_FLOAT64, 0, comm, cs));
  NCCLCHK(c, g_rccl.GroupEnd());
  HIPCHK(c, hipEventRecord(e1, cs));
  HIPCHK(c, hipStreamWaitEvent(c->stream, e1, 0));
  NCCLCHK(c, g_rccl.AllGather(d + n, d + 2 * n, (size_t)n, NCCL_FLOAT64, comm, c->stream));
  NCCLCHK(c, g_rccl.AllReduce(d + 2 * n, d + 3 * n, (size_t)n, NCCL_FLOAT64, NCCL_SUM, comm, c->stream));
  HIPCHK(c, hipMemcpyAsync(h.data(), d, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < n && rc == SZ_OK; k++)
    if (h[n + k] != 1.0 + k || h[2 * n + k] != 1.0 + k || h[3 * n + k] != 1.0 + k) { c->err = "RCCL self test: wrong data"; rc = SZ_E_HIP; }
  (void)hipFree(d); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipStreamDestroy(cs);
  (void)g_rccl.CommDestroy(comm);
  return rc;
}
int sz_comm_destroy(sz_ctx* c) {
  if (!c) return SZ_E_ARG;
  if (c->comm) { (void)g_rccl.CommDestroy(c->comm); c->comm = nullptr; }
  if (c->comm_stream) { (void)hipStreamDestroy(c->comm_stream); c->comm_stream = nullptr; }
  if (c->ev_packed) { (void)hipEventDestroy(c->ev_packed); c->ev_packed = nullptr; }
  if (c->ev_recv) { (void)hipEventDestroy(c->ev_recv); c->ev_recv = nullptr; }
  c->host_transport = false; c->host_tr = sz_host_transport{ nullptr, nullptr, nullptr, nullptr };
  c->comm_n = 0; c->d_send = c->d_recv = c->d_ref = nullptr; c->d_dcap = nullptr; c->halo_cap = 0; c->tile_since_box = -1;
  if (c->d_gather) { (void)hipFree(c->d_gather); c->d_gather = nullptr; }
  free_pool(c->comm_allocs);
  return SZ_OK;
}
// sum of n doubles in device memory over all ranks, in place, on the context's stream (per-cell partial sums of the
// two-way coupling and of the grid output)
int sz_comm_allreduce(sz_ctx* c, void* d_buf, int64_t n) {
  if (!c || !d_buf || n < 0 || c->comm_n < 1) return SZ_E_STATE;
  (void)hipSetDevice(c->device);
  if (c->comm_n > 1 && c->host_transport) {
    std::vector<double> h((size_t)n);
    HIPCHK(c, hipMemcpyAsync(h.data(), d_buf, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HOSTCHK(c, c->host_tr.allreduce_sum_f64(c->host_tr.user, h.data(), n), "allreduce_sum_f64");
    HIPCHK(c, hipMemcpyAsync(d_buf, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  } else if (c->comm_n > 1) NCCLCHK(c, g_rccl.AllReduce(d_buf, d_buf, (size_t)n, NCCL_FLOAT64, NCCL_SUM, c->comm, c->stream));
  return SZ_OK;
}

// prv_comm_api.inc -- the multi-GPU half of the C ABI; compiled as part of prv_api.cpp (shares its context types).
//
// One process per GPU (RANK / WORLD_SIZE / LOCAL_RANK as torchrun exports them).  The candidate views of a scoring
// round are dealt to the ranks, every rank renders + scores its shard with the whole ensemble, and ONE all-gather of
// the 16-byte score records gives every rank the whole round (SURVEY 8e).  The reference has nothing like it: its
// loops over the candidates are serial (main.cpp:2045-2094, 2105-2158; run.py:293).
//
// transport "rccl": ncclAllGather / ncclBroadcast on device buffers over xGMI, on the context's stream.  librccl is
//   resolved at run time: the copy the process has ALREADY mapped when there is one (a host program that brought up
//   torch.distributed's "nccl" backend: ONE RCCL per process), else the soname search (comm_load_rccl); rank 0's
//   ncclUniqueId reaches the others through the TCP star of prv_star.hpp.
// transport "socket": the same calls staged through host memory and that star -- for two ranks that share ONE GPU
//   (RCCL refuses that) in the tests.  Never the default when every rank has its own device.
#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>

#include "prv_star.hpp"

// a communicator that outlives its context (interpreter shutdown order) becomes an inert handle: every entry point
// checks ctx, prv_comm_destroy then only frees host memory
struct prv_comm : prv_handle {
  using prv_handle::prv_handle;
  ~prv_comm() override {
    if (ctx) detach();
  }
  void detach() override {
    if (nccl && CommDestroy) (void)CommDestroy(nccl);
    nccl = nullptr;
    send.reset();
    recv.reset();
  }
  int rank = 0, world = 1;
  bool rccl = false;
  prvstar::Star star;
  // RCCL entry points (dlsym)
  void* lib = nullptr;
  ncclComm_t nccl = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string lib_path, lib_how; // the librccl file the entry points resolve to, and how it was found (prv_comm_library)
  int lib_version = 0;           // ncclGetVersion
  Buffer send, recv;             // device staging of the record gather
  std::vector<prv_score_record> host_records; // ... and its host end (grows with them)
  std::vector<uint8_t> host_a, host_b; // socket transport staging
};

namespace {

#define NCCLCHK(cm, expr)                                                                                        \
  do {                                                                                                           \
    ncclResult_t r__ = (expr);                                                                                   \
    if (r__ != ncclSuccess)                                                                                      \
      return fail((cm)->ctx, PRV_E_HIP, "%s failed: %s", #expr, (cm)->GetErrorString ? (cm)->GetErrorString(r__) : "?"); \
  } while (0)

// the librccl this process has ALREADY mapped (torch.distributed's bundled copy when the host program brought its "nccl"
// backend up first): path of the first loaded object whose file name starts with "librccl.so"
static int find_mapped_rccl(struct dl_phdr_info* info, size_t, void* out) {
  const char* name = info->dlpi_name;
  if (!name || !*name) return 0;
  const char* base = strrchr(name, '/');
  base = base ? base + 1 : name;
  if (strncmp(base, "librccl.so", 10) != 0) return 0;
  *static_cast<std::string*>(out) = name;
  return 1; // stop
}

int comm_load_rccl(prv_comm* cm) {
  prv_ctx* c = cm->ctx;
  // ONE RCCL per process.  Order: an explicit PRV_RCCL_LIB; the copy the process has already mapped (RTLD_NOLOAD: the
  // same handle torch's communicator runs on -- a second, different build of the library bringing up a second set of
  // transports over the same GPUs is what this avoids); only then the soname search.
  if (const char* n = getenv("PRV_RCCL_LIB"); n && *n) {
    cm->lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    cm->lib_how = "PRV_RCCL_LIB";
  }
  if (!cm->lib) {
    std::string mapped;
    dl_iterate_phdr(find_mapped_rccl, &mapped);
    if (!mapped.empty() && (cm->lib = dlopen(mapped.c_str(), RTLD_NOW | RTLD_NOLOAD))) cm->lib_how = "already mapped by the process";
  }
  if (!cm->lib) {
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
    for (const char* n : names) {
      cm->lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
      if (cm->lib) break;
    }
    cm->lib_how = "soname search";
  }
  if (!cm->lib) return fail(c, PRV_E_IO, "cannot load librccl (%s): set PRV_RCCL_LIB, or use the socket transport", dlerror());
  struct { void** fn; const char* name; } syms[] = {
      {(void**)&cm->GetUniqueId, "ncclGetUniqueId"}, {(void**)&cm->CommInitRank, "ncclCommInitRank"},
      {(void**)&cm->CommDestroy, "ncclCommDestroy"}, {(void**)&cm->AllGather, "ncclAllGather"},
      {(void**)&cm->Broadcast, "ncclBroadcast"},     {(void**)&cm->GroupStart, "ncclGroupStart"},
      {(void**)&cm->GroupEnd, "ncclGroupEnd"},       {(void**)&cm->GetErrorString, "ncclGetErrorString"}};
  for (auto& s : syms)
    if (!(*s.fn = dlsym(cm->lib, s.name))) return fail(c, PRV_E_IO, "librccl has no %s", s.name);
  Dl_info where{};
  if (dladdr((void*)cm->CommInitRank, &where) && where.dli_fname) cm->lib_path = where.dli_fname; // the file the calls really land in
  if (auto get_version = (ncclResult_t(*)(int*))dlsym(cm->lib, "ncclGetVersion")) (void)get_version(&cm->lib_version);
  g_rccl_loaded.store(true);
  return PRV_OK;
}

// device buffers; recv = world blocks of `bytes` in rank order.  Enqueued on the context's stream (rccl) or done by
// the time it returns (socket).
int comm_all_gather(prv_comm* cm, const void* send_dev, size_t bytes, void* recv_dev) {
  prv_ctx* c = cm->ctx;
  if (cm->rccl) { // also with one rank: the same call path a multi-GPU job takes
    NCCLCHK(cm, cm->AllGather(send_dev, recv_dev, bytes, ncclUint8, cm->nccl, c->stream));
    return PRV_OK;
  }
  if (cm->world == 1) {
    if (recv_dev != send_dev) HIPCHK(c, hipMemcpyAsync(recv_dev, send_dev, bytes, hipMemcpyDeviceToDevice, c->stream));
    return PRV_OK;
  }
  cm->host_a.resize(bytes);
  cm->host_b.resize(bytes * (size_t)cm->world);
  HIPCHK(c, hipMemcpyAsync(cm->host_a.data(), send_dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!cm->star.all_gather(cm->host_a.data(), bytes, cm->host_b.data())) return fail(c, PRV_E_IO, "socket all-gather: %s", cm->star.error.c_str());
  HIPCHK(c, hipMemcpyAsync(recv_dev, cm->host_b.data(), cm->host_b.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream)); // the staging vector is reused by the next call
  return PRV_OK;
}

int comm_broadcast(prv_comm* cm, void* buf_dev, size_t bytes, int root) {
  prv_ctx* c = cm->ctx;
  if (cm->rccl) {
    NCCLCHK(cm, cm->Broadcast(buf_dev, buf_dev, bytes, ncclUint8, root, cm->nccl, c->stream));
    return PRV_OK;
  }
  if (cm->world == 1) return PRV_OK;
  cm->host_a.resize(bytes);
  if (cm->rank == root) {
    HIPCHK(c, hipMemcpyAsync(cm->host_a.data(), buf_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  if (!cm->star.broadcast(cm->host_a.data(), bytes, root)) return fail(c, PRV_E_IO, "socket broadcast: %s", cm->star.error.c_str());
  if (cm->rank != root) {
    HIPCHK(c, hipMemcpyAsync(buf_dev, cm->host_a.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return PRV_OK;
}

} // namespace

extern "C" {

int prv_shard_views(int n_views, int rank, int world, int interleaved, int* ids_out, int* n_mine) {
  if (n_views < 0 || world < 1 || rank < 0 || rank >= world) return PRV_E_INVALID;
  const int per = (n_views + world - 1) / world;
  int n = 0;
  if (interleaved) {
    for (int v = rank; v < n_views; v += world, n++)
      if (ids_out) ids_out[n] = v;
  } else {
    const int lo = std::min(n_views, rank * per), hi = std::min(n_views, lo + per);
    for (int v = lo; v < hi; v++, n++)
      if (ids_out) ids_out[n] = v;
  }
  if (n_mine) *n_mine = n;
  return per;
}

int prv_comm_create(prv_ctx* c, int rank, int world, const char* transport, const char* rendezvous, prv_comm** out) try {
  if (!c) return PRV_E_INVALID;
  if (!out) return fail(c, PRV_E_INVALID, "out is NULL");
  *out = nullptr;
  if (world < 1 || rank < 0 || rank >= world) return fail(c, PRV_E_INVALID, "rank %d / world %d make no sense", rank, world);
  std::string tr = transport && *transport ? transport : (getenv("PRV_COMM") ? getenv("PRV_COMM") : "rccl");
  if (tr != "rccl" && tr != "socket") return fail(c, PRV_E_INVALID, "unknown transport '%s' (rccl | socket)", tr.c_str());
  std::unique_ptr<prv_comm> cm(new prv_comm(c));
  cm->rank = rank;
  cm->world = world;
  cm->rccl = tr == "rccl";
  std::string addr;
  int port = 0;
  if (rendezvous && *rendezvous) { // "host:port"
    const std::string rv = rendezvous;
    const size_t colon = rv.rfind(':');
    addr = colon == std::string::npos ? rv : rv.substr(0, colon);
    port = colon == std::string::npos ? 0 : atoi(rv.c_str() + colon + 1);
  }
  if (!cm->star.open(rank, world, addr, port)) return fail(c, PRV_E_IO, "rendezvous: %s", cm->star.error.c_str());
  if (cm->rccl && world > 1) {
    // RCCL wants one physical GPU per rank: two ranks on the same device make ncclCommInitRank fail late or hang.  Every
    // rank tells the others which GPU it sits on (host name + PCI bus id through the star) and ALL of them refuse
    // together, with the ranks and the device named, before anything of RCCL is touched.
    char me[128] = {0};
    if (gethostname(me, 63) != 0) me[0] = 0;
    me[63] = 0;
    const size_t at = strlen(me);
    me[at] = '|';
    HIPCHK(c, hipSetDevice(c->device));
    if (hipDeviceGetPCIBusId(me + at + 1, (int)(sizeof(me) - at - 2), c->device) != hipSuccess) snprintf(me + at + 1, sizeof(me) - at - 1, "device%d", c->device);
    std::vector<char> where((size_t)world * sizeof(me));
    if (!cm->star.all_gather(me, sizeof(me), where.data())) return fail(c, PRV_E_IO, "rendezvous: %s", cm->star.error.c_str());
    for (int a = 0; a < world; a++)
      for (int b = a + 1; b < world; b++)
        if (strncmp(&where[(size_t)a * sizeof(me)], &where[(size_t)b * sizeof(me)], sizeof(me)) == 0)
          return fail(c, PRV_E_INVALID, "ranks %d and %d share one GPU (%s): the rccl transport needs a device per rank -- give every rank its "
                      "own LOCAL_RANK / device, or use transport \"socket\" (PRV_COMM=socket) for ranks that share a GPU", a, b,
                      &where[(size_t)a * sizeof(me)]);
  }
  if (cm->rccl) {
    int rc = comm_load_rccl(cm.get());
    if (rc != PRV_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memset(&id, 0, sizeof(id));
    if (rank == 0) NCCLCHK(cm.get(), cm->GetUniqueId(&id));
    if (!cm->star.broadcast(&id, sizeof(id), 0)) return fail(c, PRV_E_IO, "rendezvous: %s", cm->star.error.c_str());
    NCCLCHK(cm.get(), cm->CommInitRank(&cm->nccl, world, id, rank));
  }
  *out = cm.release();
  return PRV_OK;
} catch (...) { return caught(c); }

// (librccl stays loaded: unloading a library that owns device state at exit is asking for trouble)
void prv_comm_destroy(prv_comm* cm) { destroy_handle(cm); }

int prv_comm_rank(const prv_comm* cm) { return cm ? cm->rank : PRV_E_INVALID; }
int prv_comm_world(const prv_comm* cm) { return cm ? cm->world : PRV_E_INVALID; }
const char* prv_comm_transport(const prv_comm* cm) { return !cm ? "" : cm->rccl ? "rccl" : "socket"; }

int prv_comm_library(const prv_comm* cm, char* path_out, int path_cap, int* version_out, char* how_out, int how_cap) {
  if (!cm) return PRV_E_INVALID;
  if (path_out && path_cap > 0) snprintf(path_out, (size_t)path_cap, "%s", cm->lib_path.c_str());
  if (how_out && how_cap > 0) snprintf(how_out, (size_t)how_cap, "%s", cm->lib_how.c_str());
  if (version_out) *version_out = cm->lib_version;
  return PRV_OK;
}

int prv_comm_all_gather(prv_comm* cm, const void* send_dev, size_t bytes_per_rank, void* recv_dev) try {
  if (!cm || !cm->ctx) return PRV_E_INVALID;
  prv_ctx* c = cm->ctx;
  if (!send_dev || !recv_dev || bytes_per_rank == 0) return fail(c, PRV_E_INVALID, "bad argument");
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = check_device_ptr(c, send_dev, "send_dev")) != PRV_OK || (rc = check_device_ptr(c, recv_dev, "recv_dev")) != PRV_OK) return rc;
  return comm_all_gather(cm, send_dev, bytes_per_rank, recv_dev);
} catch (...) { return caught(cm ? cm->ctx : nullptr); }

int prv_comm_barrier(prv_comm* cm) try {
  if (!cm || !cm->ctx) return PRV_E_INVALID; // also: a communicator whose context has been destroyed
  HIPCHK(cm->ctx, hipStreamSynchronize(cm->ctx->stream));
  if (!cm->star.barrier()) return fail(cm->ctx, PRV_E_IO, "barrier: %s", cm->star.error.c_str());
  return PRV_OK;
} catch (...) { return caught(cm ? cm->ctx : nullptr); }

/* The sharded scoring round: prv_score_views on this rank's shard of views [0, n_views_total), ONE all-gather of
 * ceil(N / world) records per rank, un-permuted into view order: every rank ends with the same n_views_total
 * records (and so, through prv_rank / prv_argmax, with the same ranking).  cm == NULL = one rank. */
int prv_score_views_sharded(prv_ctx* c, prv_comm* cm, int method, const int* model_slots, int n_models, const prv_camset* cs,
                            int n_views_total, int interleaved, const prv_render_opts* o, const float* gt_shard_dev,
                            prv_score_record* records_host, prv_stats* st) try {
  if (!c) return PRV_E_INVALID;
  if (cm && cm->ctx != c) return fail(c, PRV_E_INVALID, "communicator belongs to another (or a destroyed) context");
  if (n_views_total < 0 || !records_host) return fail(c, PRV_E_INVALID, "bad argument");
  const int world = cm ? cm->world : 1, rank = cm ? cm->rank : 0;
  std::vector<int> ids((size_t)std::max(1, (n_views_total + world - 1) / world));
  int n_mine = 0;
  const int per = prv_shard_views(n_views_total, rank, world, interleaved, ids.data(), &n_mine);
  if (n_views_total == 0) return PRV_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Buffer local_send, local_recv; // one-rank case: no communicator to keep them in
  Buffer& send = cm ? cm->send : local_send;
  Buffer& recv = cm ? cm->recv : local_recv;
  // Everything that can fail BEFORE the collective -- the staging buffers (they grow on the first round and when the
  // view count changes; the same on every rank, the call sequence being the same) and the host vector -- is done first,
  // and when it involved an allocation the ranks agree (one byte each through the star) that all of them got theirs:
  // a rank that could not is never waited for inside the all-gather.
  const size_t need_send = (size_t)per * sizeof(prv_score_record), need_recv = need_send * (size_t)world;
  std::vector<prv_score_record> local_all;
  std::vector<prv_score_record>& all = cm ? cm->host_records : local_all;
  // `grows` depends on nothing but the call sequence (the same on every rank): it alone decides whether the ranks meet
  // in the agreement round, so no rank can enter it alone.  Nothing is allocated when nothing grows.
  const bool grows = !send.p || send.bytes < need_send || !recv.p || recv.bytes < need_recv || all.size() < (size_t)per * world;
  int rc = PRV_OK;
  if (grows) {
    rc = ensure(c, send, need_send);
    if (rc == PRV_OK) rc = ensure(c, recv, need_recv);
    if (rc == PRV_OK) {
      try {
        if (all.size() < (size_t)per * world) all.resize((size_t)per * world);
      } catch (const std::bad_alloc&) {
        rc = fail(c, PRV_E_INTERNAL, "host memory for %zu records", (size_t)per * world);
      }
    }
  }
  if (cm && world > 1 && grows) {
    const std::string why = c->err;
    std::vector<char> ok((size_t)world, 0);
    const char mine = rc == PRV_OK ? 1 : 0;
    if (!cm->star.all_gather(&mine, 1, ok.data())) rc = fail(c, PRV_E_IO, "scoring round: %s", cm->star.error.c_str());
    else if (rc != PRV_OK) c->err = why;
    else
      for (int r = 0; r < world; r++)
        if (!ok[(size_t)r]) rc = fail(c, PRV_E_STATE, "rank %d could not allocate its buffers for the round", r);
  }
  if (rc != PRV_OK) return rc;
  hipError_t e = hipMemsetAsync(send.p, 0, (size_t)per * sizeof(prv_score_record), c->stream); // padding slots of a ragged shard
  if (e != hipSuccess) rc = fail(c, PRV_E_HIP, "memset: %s", hipGetErrorString(e));
  if (rc == PRV_OK)
    rc = prv_score_views(c, method, model_slots, n_models, cs, ids.data(), n_mine, o, gt_shard_dev, nullptr, (prv_score_record*)send.p, st);
  // A rank whose shard failed must not leave its peers alone in the collective: it still takes part, with a block of
  // all-ones bytes (no score record looks like that: psnr and coverage would both be the all-ones NaN), and EVERY rank
  // then fails the round together, naming the rank that could not score its views.
  const int shard_rc = rc;
  const std::string shard_err = c->err;
  if (cm && world > 1 && shard_rc != PRV_OK) rc = hipMemsetAsync(send.p, 0xff, (size_t)per * sizeof(prv_score_record), c->stream) == hipSuccess ? PRV_OK : shard_rc;
  if (rc == PRV_OK) rc = cm ? comm_all_gather(cm, send.p, (size_t)per * sizeof(prv_score_record), recv.p)
                            : (hipMemcpyAsync(recv.p, send.p, (size_t)per * sizeof(prv_score_record), hipMemcpyDeviceToDevice, c->stream) == hipSuccess ? PRV_OK : PRV_E_HIP);
  if (rc == PRV_OK) {
    e = hipMemcpyAsync(all.data(), recv.p, (size_t)per * world * sizeof(prv_score_record), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, PRV_E_HIP, "record copy: %s", hipGetErrorString(e));
  }
  if (shard_rc != PRV_OK) {
    c->err = shard_err; // this rank's own failure is the message its caller wants
    return shard_rc;
  }
  if (rc != PRV_OK) return rc;
  for (int r = 0; r < world; r++) // a peer's poisoned block (every record of it, not just the first): the round failed there
    for (int k = 0; k < per; k++) {
      uint32_t bits[2];
      memcpy(bits, &all[(size_t)r * per + (size_t)k].psnr, sizeof(bits));
      if (bits[0] == 0xffffffffu && bits[1] == 0xffffffffu) return fail(c, PRV_E_STATE, "rank %d could not score its shard of the round", r);
    }
  for (int v = 0; v < n_views_total; v++) // slot r*per + k holds view k*world + r (interleaved) or r*per + k (blocks)
    records_host[v] = interleaved ? all[(size_t)(v % world) * per + (size_t)(v / world)] : all[(size_t)v];
  return PRV_OK;
} catch (...) { return caught(c); }

/* The exchange step of a multi-GPU NBV iteration (main.cpp:2041-2043 trains the members one after another in one
 * process): member e has just been trained in slot e of rank e % world; afterwards slot e of EVERY rank holds it,
 * bit for bit -- every rank needs the whole ensemble to score its shard of views.  Device to device: one group of
 * ncclBroadcast calls on the slots' own canonical buffers (fp16 table | fp16 MLP | occupancy words), no host copy. */
int prv_model_exchange_slots(prv_ctx* c, prv_comm* cm, int n_members, const int* slots, const int* owners, const prv_field_desc* desc) try {
  if (!c) return PRV_E_INVALID;
  if (!cm || cm->ctx != c) return fail(c, PRV_E_INVALID, "bad communicator");
  if (n_members < 1 || n_members > PRV_MAX_MODELS || !desc || !slots || !owners) return fail(c, PRV_E_INVALID, "bad argument");
  for (int e = 0; e < n_members; e++) {
    if (slots[e] < 0 || slots[e] >= PRV_MAX_SLOTS) return fail(c, PRV_E_INVALID, "model slot %d out of range", slots[e]);
    if (owners[e] < 0 || owners[e] >= cm->world) return fail(c, PRV_E_INVALID, "member %d: owner rank %d of %d", e, owners[e], cm->world);
    for (int f = 0; f < e; f++)
      if (slots[f] == slots[e]) return fail(c, PRV_E_INVALID, "model slot %d listed twice", slots[e]);
  }
  HostLevel lv[kMaxLevels];
  uint64_t total = 0;
  if (compute_levels(*desc, lv, &total) != 0) return fail(c, PRV_E_INVALID, "invalid field descriptor");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize()); // trainers step on their own streams
  const uint64_t table_halfs = total * (uint64_t)desc->n_features, R = (uint64_t)desc->occ_res, occ_words = (R * R * R + 31) / 32;
  // every rank checks its own members and makes room for the others' FIRST, then the ranks agree (one byte each through
  // the star) that all of them can go on: nobody enters the broadcasts alone, and nothing has been overwritten yet when
  // a rank has to refuse
  int rc = PRV_OK;
  std::string why;
  for (int e = 0; e < n_members && rc == PRV_OK; e++) {
    Model& m = c->models[slots[e]];
    if (owners[e] == cm->rank) { // mine: it must be there, and be this field
      if ((rc = model_present(c, slots[e])) == PRV_OK && memcmp(&m.desc, desc, sizeof(*desc)) != 0)
        rc = fail(c, PRV_E_STATE, "member %d (slot %d) is not the field being exchanged", e, slots[e]);
    } else if ((rc = ensure(c, m.table, table_halfs * 2)) == PRV_OK && (rc = ensure(c, m.occ, occ_words * 4)) == PRV_OK) { // somebody else's: room for it
      rc = ensure(c, m.mlp, PRV_MLP_HALFS * 2);
    }
  }
  if (rc != PRV_OK) why = c->err;
  {
    std::vector<char> ok((size_t)cm->world, 0);
    const char mine = rc == PRV_OK ? 1 : 0;
    if (!cm->star.all_gather(&mine, 1, ok.data())) return fail(c, PRV_E_IO, "model exchange: %s", cm->star.error.c_str());
    if (rc != PRV_OK) {
      c->err = why;
      return rc;
    }
    for (int r = 0; r < cm->world; r++)
      if (!ok[(size_t)r]) return fail(c, PRV_E_STATE, "model exchange: rank %d can not take part (its members are not in place)", r);
  }
  for (int e = 0; e < n_members; e++) // from here on the receiving slots' arrays are being overwritten: they hold no model
    if (owners[e] != cm->rank) c->models[slots[e]].loaded = false; // until the new one has arrived and been republished
  if (cm->rccl) NCCLCHK(cm, cm->GroupStart());
  for (int e = 0; e < n_members && rc == PRV_OK; e++) {
    Model& m = c->models[slots[e]];
    const int root = owners[e];
    if ((rc = comm_broadcast(cm, m.table.p, table_halfs * 2, root)) == PRV_OK && (rc = comm_broadcast(cm, m.mlp.p, PRV_MLP_HALFS * 2, root)) == PRV_OK)
      rc = comm_broadcast(cm, m.occ.p, occ_words * 4, root);
  }
  if (rc != PRV_OK) why = c->err;
  if (cm->rccl) { // the group is closed on the error path too: an open group would leave the communicator unusable
    const ncclResult_t g = cm->GroupEnd();
    if (g != ncclSuccess && rc == PRV_OK) rc = fail(c, PRV_E_HIP, "ncclGroupEnd failed: %s", cm->GetErrorString ? cm->GetErrorString(g) : "?");
  }
  if (rc != PRV_OK) {
    if (!why.empty()) c->err = why;
    return rc;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int e = 0; e < n_members; e++) { // the data has arrived: only now do the received slots change hands
    if (owners[e] == cm->rank) continue;
    Model& m = c->models[slots[e]];
    m.loaded = false;
    m.desc = *desc;
    m.table_halfs = table_halfs;
    m.occ_words = occ_words;
    if ((rc = republish_model(c, slots[e])) != PRV_OK) return rc; // derived render state from the arrays that just arrived
    m.generation++;
  }
  return PRV_OK;
} catch (...) { return caught(c); }


/* member e in slot e, trained by rank e % world: the views-sharded planner's rule */
int prv_model_exchange(prv_ctx* c, prv_comm* cm, int n_members, const prv_field_desc* desc) try {
  if (!c) return PRV_E_INVALID;
  if (!cm || cm->ctx != c) return fail(c, PRV_E_INVALID, "bad communicator");
  if (n_members < 1 || n_members > PRV_MAX_MODELS) return fail(c, PRV_E_INVALID, "bad argument");
  int slots[PRV_MAX_MODELS], owners[PRV_MAX_MODELS];
  for (int e = 0; e < n_members; e++) {
    slots[e] = e;
    owners[e] = e % cm->world;
  }
  return prv_model_exchange_slots(c, cm, n_members, slots, owners, desc);
} catch (...) { return caught(c); }

} // extern "C"

// nid_multi.inc -- include/nid/nid_multi.h: cell shards over the GPUs of one node, in C++ behind the C-ABI.
// Part of the nid_capi.hip translation unit (it drives the shard contexts through their internals: streams,
// slots, the batched launcher).  Reference anchors: there is no multi-GPU code in the reference; the callers this
// serves are NID_pose_estimation.cpp:253-351 and optimization_algorithm_levenberg.cpp:98,173 (SURVEY 8e).
#include <dlfcn.h>
#include <rccl/rccl.h>

#include "nid/nid_multi.h"

namespace {

// librccl is loaded on first use: a single-GPU process never pays for it
struct RcclApi {
  void *handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::string error, path;
  bool load() {
    if (handle) return true;
    // The RCCL that belongs to the HIP / HSA runtime this process is ALREADY running on: a process that imported
    // PyTorch runs on the ROCm libraries bundled in torch/lib (they were loaded first and own the sonames), any
    // other process on /opt/rocm/lib -- and an RCCL from the other tree would bring up a second HSA runtime
    // ("no ROCm-capable device is detected").  So: the directory libamdhip64 was loaded from, first.
    std::vector<std::string> names;
    if (const char *forced = getenv("NID_RCCL_LIBRARY")) {  // deployment override: exactly this library, nothing else
      handle = dlopen(forced, RTLD_NOW | RTLD_LOCAL);
      if (!handle) { error = std::string("dlopen(NID_RCCL_LIBRARY=") + forced + "): " + dlerror(); return false; }
      path = forced;
    } else if (void *sym = dlsym(RTLD_DEFAULT, "hipGetDeviceCount")) {
      Dl_info info;
      if (dladdr(sym, &info) && info.dli_fname) {
        std::string dir(info.dli_fname);
        const size_t slash = dir.rfind('/');
        if (slash != std::string::npos) {
          dir.resize(slash);
          names.push_back(dir + "/librccl.so.1");
          names.push_back(dir + "/librccl.so");
        }
      }
    }
    if (!handle) {
      names.push_back("librccl.so.1");
      names.push_back("librccl.so");
      names.push_back("/opt/rocm/lib/librccl.so.1");
      for (const std::string &name : names) {
        handle = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (handle) { path = name; break; }
      }
    }
    if (!handle) { error = std::string("dlopen(librccl): ") + dlerror(); return false; }
    auto sym = [&](const char *n) { void *p = dlsym(handle, n); if (!p) error = std::string("librccl lacks ") + n; return p; };
    GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(sym("ncclGetUniqueId"));
    CommInitRank = reinterpret_cast<decltype(CommInitRank)>(sym("ncclCommInitRank"));
    CommInitAll = reinterpret_cast<decltype(CommInitAll)>(sym("ncclCommInitAll"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
    CommCount = reinterpret_cast<decltype(CommCount)>(sym("ncclCommCount"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
    GroupStart = reinterpret_cast<decltype(GroupStart)>(sym("ncclGroupStart"));
    GroupEnd = reinterpret_cast<decltype(GroupEnd)>(sym("ncclGroupEnd"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
    if (!GetUniqueId || !CommInitRank || !CommInitAll || !CommDestroy || !CommCount || !AllReduce || !GroupStart ||
        !GroupEnd || !GetErrorString) { dlclose(handle); handle = nullptr; return false; }
    return true;
  }
};
RcclApi g_rccl;

constexpr int kGroupRing = 2;  // nid_multi_run_sequence: groups in flight

struct ShardBuf {  // (released on the shard's device, before its context: nid_multi_destroy)
  Stream comm_stream;
  DevBuf<double> part_dev;    // [NID_SLOTS][32] partial blocks of launches in RCCL mode
  DevBuf<double> cells_dev;   // [ncell][kCellExch] per-cell exchange across processes
  Event fence[2];             // compute streams -> comm stream
  DevBuf<double> ring_dev[kGroupRing];  // run_sequence: each at least [group*batch][32]
  Event ring_free[kGroupRing];          // this shard's exchange of the group in ring_dev[i] is over
  bool ring_used[kGroupRing] = {false, false};
};
constexpr int kCellExch = 9;  // Htarget, Hjoint, err, der[6]

}  // namespace

// RCCL communicator(s) of this process: one per local device.  Separate from nid_multi so that one communicator
// serves every nid_multi a process creates on the same devices (e.g. the levels of the coarse-to-fine schedule).
struct nid_comm {
  std::vector<ncclComm_t> comm;
  std::vector<int> device;
  int rank = 0, world = 1;  // process level
};

struct nid_multi {
  std::vector<nid_ctx *> sh;
  std::vector<ShardBuf> buf;
  std::vector<ncclComm_t> comm;  // borrowed from `attached`: one per shard once a communicator is live
  nid_comm *attached = nullptr;
  bool owns_comm = false;
  nid_exchange_fn hook = nullptr;  // NID_REDUCE_HOOK
  void *hook_user = nullptr;
  int batch_n[NID_SLOTS];          // NID_REDUCE_HOOK: poses of the batch that starts at this slot, 0 once exchanged
  nid_config cfg{};
  int ncell = 0;
  int rank = 0, world = 1;      // process level; a single-process nid_multi has world == 1
  int reduce_mode = NID_REDUCE_HOST;
  bool comm_live = false;
  // RCCL mode: results of batched launches land here (pinned), one event per batch
  PinnedBuf<double> part_host;   // [NID_SLOTS][32]
  PinnedBuf<double> cells_host;  // [ncell][kCellExch]
  PinnedBuf<double> ring_host[kGroupRing];  // each at least [shards * group*batch][32]
  Event ring_done[kGroupRing];
  Event batch_done[NID_SLOTS];
  int batch_of[NID_SLOTS];       // first slot of the batch a pending slot belongs to, -1 = not pending
  std::string last_error;
};

namespace {

#define NIDM_HIP(m, expr)                                                      \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      (m)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);     \
      return _e == hipErrorOutOfMemory ? NID_ERR_NOMEM : NID_ERR_HIP;          \
    }                                                                          \
  } while (0)
#define NIDM_NCCL(m, expr)                                                     \
  do {                                                                         \
    ncclResult_t _r = (expr);                                                  \
    if (_r != ncclSuccess) {                                                   \
      (m)->last_error = std::string(#expr) + ": " + g_rccl.GetErrorString(_r); \
      return NID_ERR_HIP;                                                      \
    }                                                                          \
  } while (0)
#define NIDM_SHARDS(m, call)                                                   \
  do {                                                                         \
    for (size_t _k = 0; _k < (m)->sh.size(); _k++) {                           \
      nid_ctx *ctx = (m)->sh[_k];                                              \
      int _rc = (call);                                                        \
      if (_rc != NID_OK) { (m)->last_error = nid_last_error(ctx); return _rc; }\
    }                                                                          \
  } while (0)

bool rccl_needed(const nid_multi *m) { return m->reduce_mode == NID_REDUCE_RCCL; }

int multi_check(nid_multi *m) {
  if (!m) return NID_ERR_INVALID_ARG;
  if (m->world > 1 && !m->comm_live && !m->hook) {
    m->last_error = "a multi-process nid_multi needs nid_multi_comm_init (or an exchange hook) before it can evaluate";
    return NID_ERR_STATE;
  }
  return NID_OK;
}

int multi_alloc(nid_multi *m) {
  const size_t K = m->sh.size();
  m->buf.resize(K);
  for (int s = 0; s < NID_SLOTS; s++) { m->batch_of[s] = -1; m->batch_n[s] = 0; }
  for (size_t k = 0; k < K; k++) {
    NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device));
    ShardBuf &B = m->buf[k];
    NIDM_HIP(m, B.part_dev.alloc((size_t)NID_SLOTS * kReducedLen));
    NIDM_HIP(m, B.cells_dev.alloc((size_t)m->ncell * kCellExch));
    NIDM_HIP(m, B.comm_stream.create());
    for (Event &e : B.fence) NIDM_HIP(m, e.create(hipEventDisableTiming));
    for (Event &e : B.ring_free) NIDM_HIP(m, e.create(hipEventDisableTiming));
  }
  NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
  NIDM_HIP(m, m->part_host.alloc((size_t)NID_SLOTS * kReducedLen));
  NIDM_HIP(m, m->cells_host.alloc((size_t)m->ncell * kCellExch));
  for (Event &e : m->batch_done) NIDM_HIP(m, e.create(hipEventDisableTiming));
  for (Event &e : m->ring_done) NIDM_HIP(m, e.create(hipEventDisableTiming));
  return NID_OK;
}

// sum of `count` doubles at `dev[k]` (same offset on every shard) over every shard of the job, in place, on
// stream[k]; the caller has ordered stream[k] after the producers
int multi_allreduce(nid_multi *m, const std::vector<double *> &dev, size_t count, const std::vector<hipStream_t> &st) {
  if (!m->comm_live) { m->last_error = "no communicator"; return NID_ERR_STATE; }
  const size_t K = m->sh.size();
  if (K > 1) NIDM_NCCL(m, g_rccl.GroupStart());
  for (size_t k = 0; k < K; k++) {
    NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device));
    NIDM_NCCL(m, g_rccl.AllReduce(dev[k], dev[k], count, ncclDouble, ncclSum, m->comm[k], st[k]));
  }
  if (K > 1) NIDM_NCCL(m, g_rccl.GroupEnd());
  return NID_OK;
}

// per-cell arrays of the whole image across PROCESSES: vals[ncell][kCellExch], zero outside this process's cells
int multi_exchange_cells(nid_multi *m) {
  if (m->reduce_mode == NID_REDUCE_HOOK) {
    if (m->hook(m->cells_host, (int64_t)m->ncell * kCellExch, m->hook_user) != 0) { m->last_error = "exchange hook failed"; return NID_ERR_HIP; }
    return NID_OK;
  }
  if (m->sh.size() > 1) { m->last_error = "per-cell exchange across processes supports one shard per process"; return NID_ERR_UNSUPPORTED; }
  nid_ctx *c0 = m->sh[0];
  ShardBuf &B = m->buf[0];
  NIDM_HIP(m, hipSetDevice(c0->cfg.device));
  const size_t bytes = (size_t)m->ncell * kCellExch * sizeof(double);
  NIDM_HIP(m, hipMemcpyAsync(B.cells_dev, m->cells_host, bytes, hipMemcpyHostToDevice, B.comm_stream));
  std::vector<double *> dev{B.cells_dev};
  std::vector<hipStream_t> st{B.comm_stream};
  int rc = multi_allreduce(m, dev, (size_t)m->ncell * kCellExch, st);
  if (rc) return rc;
  NIDM_HIP(m, hipMemcpyAsync(m->cells_host, B.cells_dev, bytes, hipMemcpyDeviceToHost, B.comm_stream));
  NIDM_HIP(m, hipStreamSynchronize(B.comm_stream));
  return NID_OK;
}

int multi_href_finish(nid_multi *m, std::vector<int32_t> &cnt, std::vector<double> &href, int32_t *bs_counter, double *Href);
int multi_href(nid_multi *m, const double *pose, bool matrix, int32_t *bs_counter, double *Href, double *bs_value,
               int32_t *bs_index) {
  if (!m || !pose) return NID_ERR_INVALID_ARG;
  std::vector<int32_t> cnt(m->ncell, 0);
  std::vector<double> href(m->ncell, 0.0);
  for (nid_ctx *ctx : m->sh) {
    int rc = matrix ? nid_compute_href_matrix(ctx, pose, cnt.data(), href.data(), bs_value, bs_index)
                    : nid_compute_href(ctx, pose, cnt.data(), href.data(), bs_value, bs_index);
    if (rc) { m->last_error = nid_last_error(ctx); return rc; }
  }
  return multi_href_finish(m, cnt, href, bs_counter, Href);
}

// the per-cell counts and reference entropies of this process's shards -> every cell of the image (across the ranks)
int multi_href_finish(nid_multi *m, std::vector<int32_t> &cnt, std::vector<double> &href, int32_t *bs_counter, double *Href) {
  if (m->world > 1) {
    int rc = multi_check(m);
    if (rc) return rc;
    std::memset(m->cells_host, 0, (size_t)m->ncell * kCellExch * sizeof(double));
    for (nid_ctx *ctx : m->sh)
      for (int cl = 0, c = ctx->g.cell_begin; cl < ctx->g.nloc; cl++, c += ctx->g.cell_stride) {
        m->cells_host[(size_t)c * kCellExch] = (double)cnt[c];
        m->cells_host[(size_t)c * kCellExch + 1] = href[c];  // NaN = inactive survives the sum
      }
    rc = multi_exchange_cells(m);
    if (rc) return rc;
    for (int c = 0; c < m->ncell; c++) {
      cnt[c] = (int32_t)m->cells_host[(size_t)c * kCellExch];
      href[c] = m->cells_host[(size_t)c * kCellExch + 1];
    }
  }
  for (int c = 0; c < m->ncell; c++) {
    if (bs_counter) bs_counter[c] = cnt[c];
    if (Href) Href[c] = href[c];
  }
  return NID_OK;
}

int multi_evaluate(nid_multi *m, const double *pose, bool matrix, int want_jac, double *Ht, double *Hj, double *err,
                   double *der) {
  int rc = multi_check(m);
  if (rc) return rc;
  if (!pose) return NID_ERR_INVALID_ARG;
  if (m->world == 1) {  // every shard writes its own cell range of the caller's arrays
    for (nid_ctx *ctx : m->sh) {
      rc = matrix ? nid_evaluate_matrix(ctx, pose, want_jac, Ht, Hj, err, der) : nid_evaluate(ctx, pose, want_jac, Ht, Hj, err, der);
      if (rc) { m->last_error = nid_last_error(ctx); return rc; }
    }
    return NID_OK;
  }
  std::vector<double> ht(m->ncell, 0.0), hj(m->ncell, 0.0), er(m->ncell, 0.0), dr((size_t)6 * m->ncell, 0.0);
  for (nid_ctx *ctx : m->sh) {
    rc = matrix ? nid_evaluate_matrix(ctx, pose, want_jac, ht.data(), hj.data(), er.data(), dr.data())
                : nid_evaluate(ctx, pose, want_jac, ht.data(), hj.data(), er.data(), dr.data());
    if (rc) { m->last_error = nid_last_error(ctx); return rc; }
  }
  for (int c = 0; c < m->ncell; c++) {
    double *row = m->cells_host + (size_t)c * kCellExch;
    row[0] = ht[c]; row[1] = hj[c]; row[2] = er[c];
    for (int n = 0; n < 6; n++) row[3 + n] = dr[6 * (size_t)c + n];
  }
  rc = multi_exchange_cells(m);
  if (rc) return rc;
  for (int c = 0; c < m->ncell; c++) {
    const double *row = m->cells_host + (size_t)c * kCellExch;
    if (Ht) Ht[c] = row[0];
    if (Hj) Hj[c] = row[1];
    if (err) err[c] = row[2];
    if (der && want_jac) for (int n = 0; n < 6; n++) der[6 * (size_t)c + n] = row[3 + n];
  }
  return NID_OK;
}

void sum_block(double *acc, const double *part) {
  for (int i = 0; i < kReducedLen; i++) acc[i] += part[i];
}

}  // namespace

extern "C" {

int nid_multi_cell_range(int32_t k, int32_t n, int32_t ncell, int32_t *lo, int32_t *hi) {
  if (n < 1 || k < 0 || k >= n || ncell < n || !lo || !hi) return NID_ERR_INVALID_ARG;
  *lo = (int32_t)((int64_t)k * ncell / n);
  *hi = (int32_t)((int64_t)(k + 1) * ncell / n);
  return NID_OK;
}

int nid_multi_cell_partition(int32_t k, int32_t n, int32_t ncell, int32_t partition, int32_t *begin, int32_t *end, int32_t *stride) {
  if (!begin || !end || !stride) return NID_ERR_INVALID_ARG;
  if (partition == NID_PARTITION_INTERLEAVED) {
    if (n < 1 || k < 0 || k >= n || ncell < n) return NID_ERR_INVALID_ARG;
    *begin = k; *end = ncell; *stride = n;  // cells k, k + n, ...
    return NID_OK;
  }
  if (partition != NID_PARTITION_CONTIGUOUS) return NID_ERR_INVALID_ARG;
  *stride = 1;
  return nid_multi_cell_range(k, n, ncell, begin, end);
}

static int multi_create_common(const nid_config *cfg, const int32_t *devices, int32_t n, int32_t rank, int32_t world,
                               int32_t partition, nid_multi **out) {
  if (!cfg || !out || !devices || n < 1 || n > NID_MAX_SHARDS || world < 1 || rank < 0 || rank >= world) return NID_ERR_INVALID_ARG;
  if (partition != NID_PARTITION_CONTIGUOUS && partition != NID_PARTITION_INTERLEAVED) return NID_ERR_INVALID_ARG;
  *out = nullptr;
  const int ncell = cfg->cell_num * cfg->cell_num;
  const int total = n * world;  // shards in the job: `world` processes with n each (n == 1 when world > 1)
  if (cfg->cell_num < 1 || total > ncell) return NID_ERR_INVALID_ARG;
  nid_multi *m = new (std::nothrow) nid_multi();
  if (!m) return NID_ERR_NOMEM;
  m->cfg = *cfg; m->ncell = ncell; m->rank = rank; m->world = world;
  for (int k = 0; k < n; k++) {
    nid_config c = *cfg;
    c.device = devices[k];
    int32_t lo, hi, stride = 1;
    { int prc = nid_multi_cell_partition(rank * n + k, total, ncell, partition, &lo, &hi, &stride); if (prc != NID_OK) { nid_multi_destroy(m); return prc; } }
    c.cell_begin = lo; c.cell_end = hi;
    nid_ctx *ctx = nullptr;
    int rc = nid_create_strided(&c, stride, &ctx);
    if (rc != NID_OK) { nid_multi_destroy(m); return rc; }
    m->sh.push_back(ctx);
  }
  int rc = multi_alloc(m);
  if (rc != NID_OK) { nid_multi_destroy(m); return rc; }
  *out = m;
  return NID_OK;
}

int nid_multi_create(const nid_config *cfg, const int32_t *devices, int32_t n, nid_multi **out) {
  return multi_create_common(cfg, devices, n, 0, 1, NID_PARTITION_CONTIGUOUS, out);
}

int nid_multi_create_rank(const nid_config *cfg, int32_t device, int32_t rank, int32_t world, nid_multi **out) {
  return multi_create_common(cfg, &device, 1, rank, world, NID_PARTITION_CONTIGUOUS, out);
}

int nid_multi_create_partitioned(const nid_config *cfg, const int32_t *devices, int32_t n, int32_t rank, int32_t world,
                                 int32_t partition, nid_multi **out) {
  if (world > 1 && n != 1) return NID_ERR_INVALID_ARG;  // one shard per process in a multi-process job
  return multi_create_common(cfg, devices, n, rank, world, partition, out);
}

int nid_multi_destroy(nid_multi *m) {
  if (!m) return NID_OK;
  // resident evaluators first: every release below synchronises the device, i.e. would wait for a resident kernel to
  // leave by itself (its 200 ms idle limit) instead of being told to
  for (nid_ctx *ctx : m->sh) (void)nid_set_resident(ctx, 0);
  for (size_t k = 0; k < m->sh.size() && k < m->buf.size(); k++) {  // a shard's buffers on its device, behind its comm stream
    (void)hipSetDevice(m->sh[k]->cfg.device);
    if (m->buf[k].comm_stream) (void)hipStreamSynchronize(m->buf[k].comm_stream);
    m->buf[k] = ShardBuf();
  }
  const int dev0 = m->sh.empty() ? -1 : m->sh[0]->cfg.device;
  if (m->owns_comm && m->attached) nid_comm_destroy(m->attached);
  for (nid_ctx *ctx : m->sh) nid_destroy(ctx);
  if (dev0 >= 0) (void)hipSetDevice(dev0);  // (the pinned landing zones and the events are the first shard's device's)
  delete m;
  return NID_OK;
}

const char *nid_multi_last_error(const nid_multi *m) { return m ? m->last_error.c_str() : ""; }
int nid_multi_shards(const nid_multi *m) { return m ? (int)m->sh.size() : 0; }
nid_ctx *nid_multi_shard(nid_multi *m, int32_t k) { return (m && k >= 0 && k < (int)m->sh.size()) ? m->sh[k] : nullptr; }
int nid_multi_world(const nid_multi *m, int32_t *rank, int32_t *world) {
  if (!m) return NID_ERR_INVALID_ARG;
  if (rank) *rank = m->rank;
  if (world) *world = m->world;
  return NID_OK;
}

// ---- RCCL ------------------------------------------------------------------------------------------------
int nid_multi_comm_unique_id(uint8_t id[NID_RCCL_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) == NID_RCCL_ID_BYTES, "ncclUniqueId size");
  if (!id) return NID_ERR_INVALID_ARG;
  if (!g_rccl.load()) return NID_ERR_UNSUPPORTED;
  ncclUniqueId u;
  if (g_rccl.GetUniqueId(&u) != ncclSuccess) return NID_ERR_HIP;
  std::memcpy(id, &u, sizeof(u));
  return NID_OK;
}

int nid_comm_create_rank(const uint8_t id[NID_RCCL_ID_BYTES], int32_t rank, int32_t world, int32_t device, nid_comm **out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world) return NID_ERR_INVALID_ARG;
  *out = nullptr;
  if (!g_rccl.load()) return NID_ERR_UNSUPPORTED;
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  if (hipSetDevice(device) != hipSuccess) return NID_ERR_NO_DEVICE;
  nid_comm *c = new (std::nothrow) nid_comm();
  if (!c) return NID_ERR_NOMEM;
  c->comm.assign(1, nullptr); c->device.assign(1, device); c->rank = rank; c->world = world;
  if (g_rccl.CommInitRank(&c->comm[0], world, u, rank) != ncclSuccess) { delete c; return NID_ERR_HIP; }
  *out = c;
  return NID_OK;
}

int nid_comm_create_local(const int32_t *devices, int32_t n, nid_comm **out) {
  if (!devices || !out || n < 1 || n > NID_MAX_SHARDS) return NID_ERR_INVALID_ARG;
  *out = nullptr;
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++)
      if (devices[a] == devices[b]) return NID_ERR_UNSUPPORTED;  // RCCL: one rank per device
  if (!g_rccl.load()) return NID_ERR_UNSUPPORTED;
  nid_comm *c = new (std::nothrow) nid_comm();
  if (!c) return NID_ERR_NOMEM;
  c->comm.assign(n, nullptr); c->device.assign(devices, devices + n);
  if (g_rccl.CommInitAll(c->comm.data(), n, c->device.data()) != ncclSuccess) { delete c; return NID_ERR_HIP; }
  *out = c;
  return NID_OK;
}

int nid_comm_destroy(nid_comm *c) {
  if (!c) return NID_OK;
  for (size_t k = 0; k < c->comm.size(); k++)
    if (c->comm[k]) { (void)hipSetDevice(c->device[k]); (void)g_rccl.CommDestroy(c->comm[k]); }
  delete c;
  return NID_OK;
}

int nid_comm_ranks(const nid_comm *c, int32_t *nranks) {
  if (!c || !nranks || c->comm.empty()) return NID_ERR_INVALID_ARG;
  int n = 0;
  if (g_rccl.CommCount(c->comm[0], &n) != ncclSuccess) return NID_ERR_HIP;
  *nranks = n;
  return NID_OK;
}

int nid_multi_attach_comm(nid_multi *m, nid_comm *c) {
  if (!m || !c) return NID_ERR_INVALID_ARG;
  if (m->comm_live) return NID_ERR_STATE;
  if (c->comm.size() != m->sh.size() || c->world != m->world || c->rank != m->rank) {
    m->last_error = "communicator and nid_multi disagree on shards / rank / world";
    return NID_ERR_INVALID_ARG;
  }
  for (size_t k = 0; k < m->sh.size(); k++)
    if (c->device[k] != m->sh[k]->cfg.device) { m->last_error = "communicator and nid_multi disagree on devices"; return NID_ERR_INVALID_ARG; }
  m->comm = c->comm;
  m->attached = c;
  m->comm_live = true;
  m->reduce_mode = NID_REDUCE_RCCL;
  return NID_OK;
}

int nid_multi_comm_init(nid_multi *m, const uint8_t id[NID_RCCL_ID_BYTES]) {
  if (!m || !id) return NID_ERR_INVALID_ARG;
  if (m->sh.size() != 1) { m->last_error = "nid_multi_comm_init: one shard per process (nid_multi_create_rank)"; return NID_ERR_STATE; }
  if (m->comm_live) return NID_ERR_STATE;
  nid_comm *c = nullptr;
  int rc = nid_comm_create_rank(id, m->rank, m->world, m->sh[0]->cfg.device, &c);
  if (rc) { m->last_error = g_rccl.error.empty() ? "ncclCommInitRank failed" : g_rccl.error; return rc; }
  rc = nid_multi_attach_comm(m, c);
  if (rc) { nid_comm_destroy(c); return rc; }
  m->owns_comm = true;
  return NID_OK;
}

int nid_multi_comm_init_local(nid_multi *m) {
  if (!m) return NID_ERR_INVALID_ARG;
  if (m->world != 1 || m->comm_live) return NID_ERR_STATE;
  std::vector<int32_t> devs(m->sh.size());
  for (size_t k = 0; k < m->sh.size(); k++) devs[k] = m->sh[k]->cfg.device;
  nid_comm *c = nullptr;
  int rc = nid_comm_create_local(devs.data(), (int32_t)devs.size(), &c);
  if (rc) {
    m->last_error = rc == NID_ERR_UNSUPPORTED && g_rccl.handle ? "RCCL needs one device per shard (two shards share a device: use NID_REDUCE_HOST)"
                                                               : (g_rccl.error.empty() ? "ncclCommInitAll failed" : g_rccl.error);
    return rc;
  }
  rc = nid_multi_attach_comm(m, c);
  if (rc) { nid_comm_destroy(c); return rc; }
  m->owns_comm = true;
  return NID_OK;
}

int nid_multi_comm_ranks(const nid_multi *m, int32_t *nranks) {
  if (!m || !nranks || !m->comm_live) return NID_ERR_STATE;
  int n = 0;
  if (g_rccl.CommCount(m->comm[0], &n) != ncclSuccess) return NID_ERR_HIP;
  *nranks = n;
  return NID_OK;
}

int nid_multi_set_reduce_mode(nid_multi *m, int mode) {
  if (!m || (mode != NID_REDUCE_HOST && mode != NID_REDUCE_RCCL && mode != NID_REDUCE_HOOK)) return NID_ERR_INVALID_ARG;
  if (mode == NID_REDUCE_HOOK && !m->hook) { m->last_error = "no exchange hook: nid_multi_set_exchange_hook first"; return NID_ERR_STATE; }
  if (mode == NID_REDUCE_RCCL && !m->comm_live) { m->last_error = "no communicator: nid_multi_comm_init[_local] first"; return NID_ERR_STATE; }
  if (mode == NID_REDUCE_HOST && m->world > 1) { m->last_error = "NID_REDUCE_HOST sums inside one process only"; return NID_ERR_STATE; }
  m->reduce_mode = mode;
  return NID_OK;
}

int nid_multi_set_exchange_hook(nid_multi *m, nid_exchange_fn fn, void *user) {
  if (!m || !fn) return NID_ERR_INVALID_ARG;
  m->hook = fn; m->hook_user = user;
  m->reduce_mode = NID_REDUCE_HOOK;
  return NID_OK;
}

// ---- broadcast calls -----------------------------------------------------------------------------------------
int nid_multi_set_options(nid_multi *m, int jb, int xf) { if (!m) return NID_ERR_INVALID_ARG; NIDM_SHARDS(m, nid_set_options(ctx, jb, xf)); return NID_OK; }
int nid_multi_set_href_nan_markers(nid_multi *m, int on) { if (!m) return NID_ERR_INVALID_ARG; NIDM_SHARDS(m, nid_set_href_nan_markers(ctx, on)); return NID_OK; }
int nid_multi_set_math_mode(nid_multi *m, int mode) { if (!m) return NID_ERR_INVALID_ARG; NIDM_SHARDS(m, nid_set_math_mode(ctx, mode)); return NID_OK; }
int nid_multi_set_block_threads(nid_multi *m, int t) { if (!m) return NID_ERR_INVALID_ARG; NIDM_SHARDS(m, nid_set_block_threads(ctx, t)); return NID_OK; }
int nid_multi_set_launch_shape(nid_multi *m, int j, int c) { if (!m) return NID_ERR_INVALID_ARG; NIDM_SHARDS(m, nid_set_launch_shape(ctx, j, c)); return NID_OK; }
int nid_multi_set_resident(nid_multi *m, int on) {
  if (!m) return NID_ERR_INVALID_ARG;
  for (size_t k = 0; k < m->sh.size(); k++) {
    nid_ctx *ctx = m->sh[k];
    int same = 0;
    for (nid_ctx *o : m->sh) same += o->cfg.device == ctx->cfg.device;
    int rc = nid_set_resident(ctx, on && same == 1);
    if (rc) { m->last_error = nid_last_error(ctx); return rc; }
  }
  return NID_OK;
}
int nid_multi_resident_pause(nid_multi *m) {
  if (!m) return NID_ERR_INVALID_ARG;
  NIDM_SHARDS(m, nid_resident_pause(ctx));
  return NID_OK;
}
int nid_multi_set_reference_depth(nid_multi *m, const double *d, const uint8_t *im0, const double *T) {
  if (!m) return NID_ERR_INVALID_ARG;
  NIDM_SHARDS(m, nid_set_reference_depth(ctx, d, im0, T));
  return NID_OK;
}
int nid_multi_set_reference_points(nid_multi *m, const double *p, const uint8_t *im0) {
  if (!m) return NID_ERR_INVALID_ARG;
  NIDM_SHARDS(m, nid_set_reference_points(ctx, p, im0));
  return NID_OK;
}
int nid_multi_set_target_u8(nid_multi *m, const uint8_t *im1) {
  if (!m) return NID_ERR_INVALID_ARG;
  NIDM_SHARDS(m, nid_set_target_u8(ctx, im1));
  return NID_OK;
}
int nid_multi_set_pair_u16(nid_multi *m, const uint16_t *depth_u16, double depth_factor, const uint8_t *im0, const uint8_t *im1,
                           const double *Twc, const double *pose0_7, const double *pose0_colmajor16, int32_t *bs_counter, double *Href) {
  if (!m || !depth_u16 || !im0 || !im1 || !Twc || (pose0_7 == nullptr) == (pose0_colmajor16 == nullptr)) return NID_ERR_INVALID_ARG;
  // every shard's uploads and kernels are in flight before the first one is waited for
  for (nid_ctx *ctx : m->sh) {
    NIDM_HIP(m, hipSetDevice(ctx->cfg.device));
    Pose p;
    if (pose0_7) pose_from_pose7(pose0_7, ctx->xform, &p); else pose_from_matrix16(pose0_colmajor16, &p);
    int rc = pair_u16_enqueue(ctx, depth_u16, depth_factor, im0, im1, Twc, p);
    if (rc) { m->last_error = nid_last_error(ctx); return rc; }
  }
  std::vector<int32_t> cnt(m->ncell, 0);
  std::vector<double> href(m->ncell, 0.0);
  for (nid_ctx *ctx : m->sh) {
    int rc = pair_u16_collect(ctx, cnt.data(), href.data());
    if (rc) { m->last_error = nid_last_error(ctx); return rc; }
  }
  return multi_href_finish(m, cnt, href, bs_counter, Href);
}
int nid_multi_set_href_state(nid_multi *m, const int32_t *cnt, const double *Href, const double *bsv, const int32_t *bsi) {
  if (!m) return NID_ERR_INVALID_ARG;
  NIDM_SHARDS(m, nid_set_href_state(ctx, cnt, Href, bsv, bsi));
  return NID_OK;
}
int nid_multi_compute_href(nid_multi *m, const double *pose7, int32_t *cnt, double *Href, double *bsv, int32_t *bsi) {
  return multi_href(m, pose7, false, cnt, Href, bsv, bsi);
}
int nid_multi_compute_href_matrix(nid_multi *m, const double *p16, int32_t *cnt, double *Href, double *bsv, int32_t *bsi) {
  return multi_href(m, p16, true, cnt, Href, bsv, bsi);
}
int nid_multi_evaluate(nid_multi *m, const double *pose7, int want_jac, double *Ht, double *Hj, double *err, double *der) {
  return multi_evaluate(m, pose7, false, want_jac, Ht, Hj, err, der);
}
int nid_multi_evaluate_matrix(nid_multi *m, const double *p16, int want_jac, double *Ht, double *Hj, double *err, double *der) {
  return multi_evaluate(m, p16, true, want_jac, Ht, Hj, err, der);
}

// ---- fused evaluations ---------------------------------------------------------------------------------------
int nid_multi_launch_batch(nid_multi *m, int first_slot, int n, const double *poses7, int want_jac, double delta) {
  int rc = multi_check(m);
  if (rc) return rc;
  if (!poses7 || n < 1 || n > kMaxBatchExt || first_slot < 0 || first_slot + n > NID_SLOTS) return NID_ERR_INVALID_ARG;
  for (int k = 0; k < n; k++)
    if (m->batch_of[first_slot + k] >= 0) { m->last_error = "slot still pending: nid_multi_wait() it first"; return NID_ERR_STATE; }
  if (!rccl_needed(m)) {
    NIDM_SHARDS(m, nid_launch_batch(ctx, first_slot, n, poses7, want_jac, delta));
  } else {
    std::vector<double *> dev(m->sh.size());
    std::vector<hipStream_t> st(m->sh.size());
    for (size_t k = 0; k < m->sh.size(); k++) {
      nid_ctx *ctx = m->sh[k];
      dev[k] = m->buf[k].part_dev + (size_t)first_slot * kReducedLen;
      st[k] = ctx->stream;
      rc = nid_launch_batch_to(ctx, first_slot, n, poses7, want_jac, delta, dev[k]);
      if (rc) { m->last_error = nid_last_error(ctx); return rc; }
    }
    rc = multi_allreduce(m, dev, (size_t)n * kReducedLen, st);  // in-stream, behind each shard's kernel
    if (rc) return rc;
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipMemcpyAsync(m->part_host + (size_t)first_slot * kReducedLen, dev[0], (size_t)n * kReducedLen * sizeof(double),
                               hipMemcpyDeviceToHost, st[0]));
    NIDM_HIP(m, hipEventRecord(m->batch_done[first_slot], st[0]));
  }
  for (int k = 0; k < n; k++) m->batch_of[first_slot + k] = first_slot;
  m->batch_n[first_slot] = n;
  return NID_OK;
}

int nid_multi_launch_chain(nid_multi *m, int first_slot, int n, const double *poses7, int n_jac, double delta) {
  int rc = multi_check(m);
  if (rc) return rc;
  if (!poses7 || n < 1 || n > kMaxBatchExt || n_jac < 0 || n_jac > n || first_slot < 0 || first_slot + n > NID_SLOTS)
    return NID_ERR_INVALID_ARG;
  for (int k = 0; k < n; k++)
    if (m->batch_of[first_slot + k] >= 0) { m->last_error = "slot still pending: nid_multi_wait() it first"; return NID_ERR_STATE; }
  if (!rccl_needed(m)) {
    NIDM_SHARDS(m, nid_launch_chain(ctx, first_slot, n, poses7, n_jac, delta));
  } else {
    // the all-reduce is ordered behind BOTH launches: they share the shard's main stream
    std::vector<double *> dev(m->sh.size());
    std::vector<hipStream_t> st(m->sh.size());
    for (size_t k = 0; k < m->sh.size(); k++) {
      nid_ctx *ctx = m->sh[k];
      dev[k] = m->buf[k].part_dev + (size_t)first_slot * kReducedLen;
      st[k] = ctx->stream;
      rc = NID_OK;
      if (n_jac > 0) rc = nid_launch_batch_to(ctx, first_slot, n_jac, poses7, 1, delta, dev[k]);
      if (rc == NID_OK && n_jac < n)
        rc = nid_launch_batch_to(ctx, first_slot + n_jac, n - n_jac, poses7 + 7 * (size_t)n_jac, 0, delta,
                                 dev[k] + (size_t)n_jac * kReducedLen);
      if (rc) { m->last_error = nid_last_error(ctx); return rc; }
    }
    rc = multi_allreduce(m, dev, (size_t)n * kReducedLen, st);
    if (rc) return rc;
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipMemcpyAsync(m->part_host + (size_t)first_slot * kReducedLen, dev[0], (size_t)n * kReducedLen * sizeof(double),
                               hipMemcpyDeviceToHost, st[0]));
    NIDM_HIP(m, hipEventRecord(m->batch_done[first_slot], st[0]));
  }
  for (int k = 0; k < n; k++) m->batch_of[first_slot + k] = first_slot;
  m->batch_n[first_slot] = n;
  return NID_OK;
}

int nid_multi_wait(nid_multi *m, int slot, double *H36, double *b6, double *chi2, int32_t *n_active) {
  if (!m || slot < 0 || slot >= NID_SLOTS) return NID_ERR_INVALID_ARG;
  if (m->batch_of[slot] < 0) return NID_ERR_STATE;
  double acc[kReducedLen];
  if (m->reduce_mode == NID_REDUCE_HOOK) {
    // the whole batch is exchanged at once, on the first wait of any of its slots
    const int first = m->batch_of[slot], n = m->batch_n[first];
    if (n > 0) {
      for (int q = 0; q < n; q++) {
        double *dst = m->part_host + (size_t)(first + q) * kReducedLen;
        for (int i = 0; i < kReducedLen; i++) dst[i] = 0.0;
        for (nid_ctx *ctx : m->sh) {
          int rc = nid_wait(ctx, first + q, nullptr, nullptr, nullptr, nullptr);
          if (rc) { m->last_error = nid_last_error(ctx); return rc; }
          sum_block(dst, ctx->slots[first + q].reduced_host);
        }
      }
      if (m->hook(m->part_host + (size_t)first * kReducedLen, (int64_t)n * kReducedLen, m->hook_user) != 0) {
        m->last_error = "exchange hook failed";
        return NID_ERR_HIP;
      }
      m->batch_n[first] = 0;
    }
    std::memcpy(acc, m->part_host + (size_t)slot * kReducedLen, sizeof(acc));
  } else if (!rccl_needed(m)) {
    for (int i = 0; i < kReducedLen; i++) acc[i] = 0.0;
    for (nid_ctx *ctx : m->sh) {  // fixed order: shard 0, 1, ... -> bitwise reproducible
      int rc = nid_wait(ctx, slot, nullptr, nullptr, nullptr, nullptr);
      if (rc) { m->last_error = nid_last_error(ctx); return rc; }
      sum_block(acc, ctx->slots[slot].reduced_host);
    }
  } else {
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipEventSynchronize(m->batch_done[m->batch_of[slot]]));
    for (nid_ctx *ctx : m->sh) {  // the shard slots only carry an event now: clear their pending marks
      int rc = nid_wait(ctx, slot, nullptr, nullptr, nullptr, nullptr);
      if (rc) { m->last_error = nid_last_error(ctx); return rc; }
    }
    std::memcpy(acc, m->part_host + (size_t)slot * kReducedLen, sizeof(acc));
  }
  m->batch_of[slot] = -1;
  return nid_unpack_reduced(acc, H36, b6, chi2, n_active);
}

int nid_multi_normal_equations(nid_multi *m, const double *pose7, int want_jac, double delta, double *H36, double *b6,
                               double *chi2, int32_t *n_active) {
  int rc = nid_multi_launch_batch(m, 0, 1, pose7, want_jac, delta);
  if (rc) return rc;
  return nid_multi_wait(m, 0, H36, b6, chi2, n_active);
}

int64_t nid_multi_contract_bytes(const nid_multi *m) {
  if (!m) return 0;
  int64_t s = 0;
  for (nid_ctx *ctx : m->sh) s += nid_contract_bytes(ctx);
  return s;
}

// Pipelined throughput loop.  A group = `group` launches of `batch` poses on every shard, alternating between the
// shard's two compute streams (each with its own `batch` result slots; a stream runs its launches in order, so
// the slots are reused launch after launch), every launch writing its partial blocks into the group's device
// buffer; then ONE exchange for the whole group -- RCCL all-reduce of [group*batch, 32] doubles on the shard's
// comm stream + copy to pinned host memory, or (NID_REDUCE_HOST) the copies alone and a host sum -- while the
// compute streams already work on the next group.  Two groups in flight.
static int multi_run_sequence_impl(nid_multi *m, const double *poses7, int n, int batch, int group, int want_jac, double delta,
                                   double *reduced_out);

int nid_multi_time_exchange(nid_multi *m, int blocks, int repeats, float *ms_per_exchange) {
  // `repeats` exchanges of `blocks` 32-double blocks back to back on the comm stream(s) between two events: what ONE
  // exchange of the pipelined loop costs when nothing else runs (RCCL mode; collective: every rank calls it)
  int rc = multi_check(m);
  if (rc) return rc;
  if (!ms_per_exchange || blocks < 1 || repeats < 1) return NID_ERR_INVALID_ARG;
  if (!rccl_needed(m)) { *ms_per_exchange = 0.0f; return NID_OK; }  // host sum / hook: no device-side exchange
  const size_t K = m->sh.size(), count = (size_t)blocks * kReducedLen;
  std::vector<double *> dev(K, nullptr);
  std::vector<hipStream_t> st(K, nullptr);
  std::vector<DevBuf<double>> own(K);
  Event e0, e1;
  // every exit path releases what was created: each buffer on its device, behind its stream
  auto body = [&]() -> int {
    for (size_t k = 0; k < K; k++) {
      NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device));
      NIDM_HIP(m, own[k].alloc(count));
      dev[k] = own[k];
      st[k] = m->buf[k].comm_stream;
      NIDM_HIP(m, hipMemsetAsync(dev[k], 0, count * sizeof(double), st[k]));
    }
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, e0.create());
    NIDM_HIP(m, e1.create());
    int r2 = multi_allreduce(m, dev, count, st);  // warm
    if (r2 != NID_OK) return r2;
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipEventRecord(e0, st[0]));
    for (int r = 0; r < repeats; r++) {
      r2 = multi_allreduce(m, dev, count, st);
      if (r2 != NID_OK) return r2;
    }
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipEventRecord(e1, st[0]));
    NIDM_HIP(m, hipEventSynchronize(e1));
    float ms = 0.f;
    NIDM_HIP(m, hipEventElapsedTime(&ms, e0, e1));
    *ms_per_exchange = ms / (float)repeats;
    return NID_OK;
  };
  rc = body();
  for (size_t k = 0; k < K; k++) {
    (void)hipSetDevice(m->sh[k]->cfg.device);
    if (st[k]) (void)hipStreamSynchronize(st[k]);
    own[k].reset();
  }
  return rc;
}

int nid_multi_run_sequence(nid_multi *m, const double *poses7, int n, int batch, int group, int want_jac, double delta,
                           double *reduced_out) {
  const int rc = multi_run_sequence_impl(m, poses7, n, batch, group, want_jac, delta, reduced_out);
  if (rc != NID_OK && rc != NID_ERR_INVALID_ARG && rc != NID_ERR_STATE && m) {
    // an error in the middle of the pipeline (a failed hook, a HIP or RCCL error) leaves launches in flight on the ring
    // buffers and the shard slots marked pending: let everything that was enqueued finish and clear the marks, so that
    // the handle stays usable (the error itself is in nid_multi_last_error)
    const std::string why = m->last_error;
    for (size_t k = 0; k < m->sh.size(); k++) {
      nid_ctx *ctx = m->sh[k];
      (void)hipSetDevice(ctx->cfg.device);
      (void)hipStreamSynchronize(ctx->stream);
      if (ctx->aux_stream) (void)hipStreamSynchronize(ctx->aux_stream);
      if (m->buf[k].comm_stream) (void)hipStreamSynchronize(m->buf[k].comm_stream);
      (void)hipGetLastError();
      for (int s = 0; s < NID_SLOTS; s++) {
        Slot &S = ctx->slots[s];
        if (S.pending && S.delivery == Delivery::Event) S.pending = false;
      }
      for (int i = 0; i < kGroupRing; i++) m->buf[k].ring_used[i] = false;
    }
    m->last_error = why;
  }
  return rc;
}

static int multi_run_sequence_impl(nid_multi *m, const double *poses7, int n, int batch, int group, int want_jac, double delta,
                                   double *reduced_out) {
  int rc = multi_check(m);
  if (rc) return rc;
  if (!poses7 || n < 0 || batch < 1 || batch > kMaxBatchExt || 2 * batch > NID_SLOTS || group < 1) return NID_ERR_INVALID_ARG;
  for (int s = 0; s < NID_SLOTS; s++) if (m->batch_of[s] >= 0) return NID_ERR_STATE;
  const size_t K = m->sh.size();
  const size_t gcap = (size_t)group * batch;
  const bool rccl = rccl_needed(m);
  const size_t host_blocks = rccl ? gcap : gcap * K;  // host mode: every shard's partial blocks come home
  for (size_t k = 0; k < K; k++) {
    ShardBuf &B = m->buf[k];
    if (ring_size(B.ring_dev) < gcap * kReducedLen) {
      NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device));
      NIDM_HIP(m, ring_grow(B.ring_dev, gcap * kReducedLen));
    }
  }
  NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
  NIDM_HIP(m, ring_grow(m->ring_host, gcap * K * kReducedLen));  // pinned landing zones: kept across calls, grown on demand
  (void)host_blocks;
  for (size_t k = 0; k < K; k++) for (int i = 0; i < kGroupRing; i++) m->buf[k].ring_used[i] = false;
  Pose p[kMaxBatchExt];
  const int ngroups = (n + (int)gcap - 1) / (int)gcap;
  auto deliver = [&](int j) -> int {  // group j has landed in ring_host[j % ring]: sum (host mode) and hand out
    const int gi = j % kGroupRing;
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipEventSynchronize(m->ring_done[gi]));
    if (!rccl)  // the D2H copies of shards 1.. ran on their own comm streams
      for (size_t k = 1; k < K; k++) { NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device)); NIDM_HIP(m, hipStreamSynchronize(m->buf[k].comm_stream)); }
    const int cnt = std::min((int)gcap, n - j * (int)gcap);
    double *home = m->ring_host[gi];  // shard 0's region doubles as the place of the summed blocks
    if (!rccl) {
      for (int q = 0; q < cnt; q++) {
        double acc[kReducedLen];
        for (int i = 0; i < kReducedLen; i++) acc[i] = 0.0;
        for (size_t k = 0; k < K; k++) sum_block(acc, m->ring_host[gi] + (k * gcap + (size_t)q) * kReducedLen);
        std::memcpy(home + (size_t)q * kReducedLen, acc, sizeof(acc));
      }
      if (m->reduce_mode == NID_REDUCE_HOOK && m->hook(home, (int64_t)cnt * kReducedLen, m->hook_user) != 0) {
        m->last_error = "exchange hook failed";
        return NID_ERR_HIP;
      }
    }
    if (reduced_out) std::memcpy(reduced_out + (size_t)j * gcap * kReducedLen, home, (size_t)cnt * kReducedLen * sizeof(double));
    return NID_OK;
  };
  for (int j = 0; j < ngroups; j++) {
    const int gi = j % kGroupRing;
    if (j >= kGroupRing) { rc = deliver(j - kGroupRing); if (rc) return rc; }
    const int cnt = std::min((int)gcap, n - j * (int)gcap);
    const int nl = (cnt + batch - 1) / batch;
    for (size_t k = 0; k < K; k++) {  // the group that last used this ring entry must have left this shard's buffer
      ShardBuf &B = m->buf[k];
      if (!B.ring_used[gi]) continue;
      nid_ctx *ctx = m->sh[k];
      NIDM_HIP(m, hipSetDevice(ctx->cfg.device));
      NIDM_HIP(m, hipStreamWaitEvent(ctx->stream, B.ring_free[gi], 0));
      if (!ctx->external_stream) NIDM_HIP(m, hipStreamWaitEvent(ctx->aux_stream, B.ring_free[gi], 0));
    }
    for (int l = 0; l < nl; l++) {
      const int nb = std::min(batch, cnt - l * batch);
      const size_t first = (size_t)j * gcap + (size_t)l * batch;
      for (size_t k = 0; k < K; k++) {
        nid_ctx *ctx = m->sh[k];
        for (int q = 0; q < nb; q++) pose_from_pose7(poses7 + 7 * (first + q), ctx->xform, &p[q]);
        rc = launch_batch(ctx, (l & 1) * batch, nb, p, want_jac, delta, m->buf[k].ring_dev[gi] + (size_t)l * batch * kReducedLen,
                          /*on_aux_stream=*/(l & 1) != 0, /*relaunch_ok=*/true);
        if (rc) { m->last_error = nid_last_error(ctx); return rc; }
      }
    }
    // comm streams wait for the group's launches, exchange, copy home
    std::vector<double *> dev(K);
    std::vector<hipStream_t> st(K);
    for (size_t k = 0; k < K; k++) {
      nid_ctx *ctx = m->sh[k];
      ShardBuf &B = m->buf[k];
      NIDM_HIP(m, hipSetDevice(ctx->cfg.device));
      NIDM_HIP(m, hipEventRecord(B.fence[0], ctx->stream));
      NIDM_HIP(m, hipStreamWaitEvent(B.comm_stream, B.fence[0], 0));
      if (nl > 1 && !ctx->external_stream) {
        NIDM_HIP(m, hipEventRecord(B.fence[1], ctx->aux_stream));
        NIDM_HIP(m, hipStreamWaitEvent(B.comm_stream, B.fence[1], 0));
      }
      dev[k] = B.ring_dev[gi];
      st[k] = B.comm_stream;
    }
    if (rccl) {
      rc = multi_allreduce(m, dev, (size_t)cnt * kReducedLen, st);
      if (rc) return rc;
      NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
      NIDM_HIP(m, hipMemcpyAsync(m->ring_host[gi], dev[0], (size_t)cnt * kReducedLen * sizeof(double), hipMemcpyDeviceToHost, st[0]));
    } else {
      for (size_t k = 0; k < K; k++) {
        NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device));
        NIDM_HIP(m, hipMemcpyAsync(m->ring_host[gi] + k * gcap * kReducedLen, dev[k], (size_t)cnt * kReducedLen * sizeof(double),
                                   hipMemcpyDeviceToHost, st[k]));
      }
    }
    for (size_t k = 0; k < K; k++) {
      NIDM_HIP(m, hipSetDevice(m->sh[k]->cfg.device));
      NIDM_HIP(m, hipEventRecord(m->buf[k].ring_free[gi], st[k]));
      m->buf[k].ring_used[gi] = true;
    }
    NIDM_HIP(m, hipSetDevice(m->sh[0]->cfg.device));
    NIDM_HIP(m, hipEventRecord(m->ring_done[gi], st[0]));
  }
  for (int j = std::max(0, ngroups - kGroupRing); j < ngroups; j++) { rc = deliver(j); if (rc) return rc; }
  // the shard slots used above only carry events: clear their pending marks
  for (nid_ctx *ctx : m->sh)
    for (int s = 0; s < 2 * batch && s < NID_SLOTS; s++)
      if (ctx->slots[s].pending) { rc = nid_wait(ctx, s, nullptr, nullptr, nullptr, nullptr); if (rc) { m->last_error = nid_last_error(ctx); return rc; } }
  return NID_OK;
}

}  // extern "C"

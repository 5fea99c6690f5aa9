// nid_pyr.inc -- a device-built, resident image pyramid and the coarse-to-fine loop over its levels (include/nid/nid_pyr.h).
// Part of nid_capi.hip's translation unit (included behind nid_multistart.inc): it works on the level contexts' internals.
//
// A level is an ordinary context from nid_create(nid_pyr_level_config(...)).  nid_pyr_set_pair_u16 enqueues EVERYTHING --
// level 0's uploads (pair_u16_upload), levels - 1 k_pyr_down launches, every level's set-up chain (pair_u16_device) -- on
// ONE stream, level 0's, in dependency order, and synchronises it once before it marks any level ready: a level's later
// launches run on that level's own streams, and nothing of this call is in flight by then.  What a level's own streams may
// still be running when the call begins (k_repair behind a collected launch) is put in front of it with one event per
// stream, on the device.  That opening and the close are the frame (pyr_open / pyr_close, below) in which every later call
// that rewrites a level's inputs stands as well; the reference's way from level 0's depth plane down is pyr_ref_tail.
// nid_pyr_multistart_lm calls nid_compute_href and nid_multistart_lm as they are: it fills no record and launches nothing
// of its own; the survivors of a level are a handful of comparisons on the host (lm::rank_chains).

struct nid_pyr {
  int levels = 0;
  nid_ctx *ctx[NID_PYR_MAX_LEVELS] = {};
  Event idle[NID_PYR_MAX_LEVELS][2];  // a level's stream / aux_stream have reached this call
  bool have_pair = false;  // a reference is resident on every level (nid_pyr_set_pair_u16, or a promoted target: nid_pyr_stream.inc)
  // nid_keyframe.inc: the resident target's depth at level 0 (made with the pyramid), and the depth check's buffers
  // (made on its first call): the poses' matrices and the totals through one pinned block, the cell records
  DevBuf<uint16_t> tdepth_dev;
  bool have_tdepth = false;  // cleared by whatever replaces the target
  double tdepth_factor = 0;
  struct DepthCheck {
    DevBuf<double> M_dev;                    // [NID_MAX_BATCH][12]
    DevBuf<unsigned long long> totals_dev;   // [NID_MAX_BATCH][8]
    DevBuf<nid_depth_cell> cells_dev;        // [NID_MAX_BATCH][cells of level 0]
    PinnedBuf<unsigned long long> stage;     // the matrices (as doubles), then the totals
    PinnedBuf<nid_depth_cell> cells_host;    // grown to what a call with cells != NULL asks for
  } dc;
  // nid_refmask.inc: the reference's depth factor (remembered by whatever makes a reference), and the mask's state and
  // buffers -- made by the first masking call behind a new reference (have_pristine), never by a caller who does not mask
  struct RefMask {
    double ref_factor = 0;
    bool have_pristine = false;  // pristine_dev / mask_dev belong to the resident reference
    bool any_masked = false;     // a byte of mask_dev is non-zero
    DevBuf<uint16_t> pristine_dev;           // level 0's reference depth as it was made
    DevBuf<uint8_t> mask_dev, work_dev;      // the plane; the classified bytes of the call under way
    DevBuf<unsigned long long> counts_dev;   // [8]
    PinnedBuf<unsigned long long> counts_host;
    PinnedBuf<uint8_t> plane_host;           // nid_pyr_set_reference_mask_u8's plane on its way up
    // nid_reffill.inc: the fill's state and buffers -- made by the first fill behind a new reference (have_uploaded), never
    // by a caller who does not fill.  With have_uploaded, pristine_dev holds fill ? fill : uploaded
    struct Fill {
      bool have_uploaded = false;  // uploaded_dev / fill_dev belong to the resident reference
      bool any_filled = false;     // an entry of fill_dev is non-zero
      DevBuf<uint16_t> uploaded_dev, fill_dev;  // level 0's reference depth as it was made; the plane
      DevBuf<uint32_t> zbuf_dev;                // the z-buffer of the call under way
      DevBuf<unsigned long long> counts_dev;    // [8]: nid_reffill_counts
      PinnedBuf<unsigned long long> counts_host;
    } fill;
    // nid_reffuse.inc: the fusion's state and buffers -- made by the first fusion behind a new reference (have_state, which
    // implies fill.have_uploaded), never by a caller who does not fuse.  With have_state, base_dev holds fused ? fused :
    // uploaded, pristine_dev fill ? fill : base, and the fill reads base_dev where it read uploaded_dev
    struct Fuse {
      bool have_state = false;  // sum_dev / obs_dev / fused_dev / base_dev belong to the resident reference
      bool any_fused = false;   // an entry of obs_dev is non-zero
      DevBuf<uint32_t> sum_dev;             // S
      DevBuf<uint8_t> obs_dev;              // k
      DevBuf<uint16_t> fused_dev, base_dev;
    } fuse;
    // a new reference starts unmasked, unfilled and unfused
    void new_reference(double factor) {
      ref_factor = factor;
      have_pristine = any_masked = fill.have_uploaded = fill.any_filled = fuse.have_state = fuse.any_fused = false;
    }
  } rm;
};

namespace {

int pyr_fail(nid_pyr *p, int rc, const std::string &why) {
  p->ctx[0]->last_error = why;
  return rc;
}

// THE FRAME of every call that rewrites the levels' inputs (nid_pyr_set_pair_u16; nid_pyr_stream.inc's, nid_keyframe.inc's
// and nid_refmask.inc's): pyr_open, the call's own operations on level 0's stream in dependency order, pyr_close -- over
// the PARTS the call owns.  A part's ready flags are down from pyr_open to a pyr_close that returned NID_OK.
enum : unsigned { kPyrRef = 1, kPyrTarget = 2, kPyrTdepth = 4 };

void pyr_mark(nid_pyr *p, unsigned parts, bool ready) {
  for (int l = 0; l < p->levels; l++) {
    nid_ctx *ctx = p->ctx[l];
    if (parts & kPyrRef) {
      ctx->have_ref = ready;
      if (ready) ctx->ref_from_depth = true;  // (have_href stays false: the reference stage is the caller's)
      else ctx->have_href = false;
    }
    if (parts & kPyrTarget) ctx->have_target = ready;
  }
  if (parts & kPyrRef) p->have_pair = ready;
  if (parts & kPyrTdepth) p->have_tdepth = ready;
}

// REFUSE: NID_ERR_STATE, and nothing changed, while a level has an uncollected launch.
int pyr_refuse_pending(nid_pyr *p, const char *what) {
  for (int l = 0; l < p->levels; l++)
    if (any_pending(p->ctx[l])) return pyr_fail(p, NID_ERR_STATE, std::string(what) + ": a launch is pending on level " + std::to_string(l) + ": nid_wait() it first");
  return NID_OK;
}

// OPEN: the refusal; the parts' flags cleared -- from here on they are being overwritten -- and, where the call makes a NEW
// reference (new_ref_factor: its depth factor) and not the resident one again, its mask and fill forgotten (nid_refmask.h);
// then the device selected, resident evaluators retired, and what the levels' own streams still run -- it reads the
// buffers the call rewrites -- put in front of level 0's stream, on the device, with one event per stream.
int pyr_open(nid_pyr *p, const char *what, unsigned parts, const double *new_ref_factor = nullptr) {
  const int rc = pyr_refuse_pending(p, what);
  if (rc) return rc;
  pyr_mark(p, parts, false);
  if (new_ref_factor) p->rm.new_reference(*new_ref_factor);
  nid_ctx *c0 = p->ctx[0];
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  for (int l = 0; l < p->levels; l++) resident_retire(p->ctx[l]);
  const hipStream_t st = c0->stream;
  for (int l = 0; l < p->levels; l++) {
    nid_ctx *ctx = p->ctx[l];
    const hipStream_t own[2] = {ctx->stream, ctx->aux_stream};
    for (int s = 0; s < 2; s++) {
      if (!own[s] || own[s] == st) continue;
      NID_HIP(c0, hipEventRecord(p->idle[l][s], own[s]));
      NID_HIP(c0, hipStreamWaitEvent(st, p->idle[l][s], 0));
    }
  }
  return NID_OK;
}

// an error behind pyr_open drains the stream: nothing of the call stays in flight
int pyr_drain(nid_pyr *p, int rc) {
  (void)hipStreamSynchronize(p->ctx[0]->stream);
  return rc;
}

// CLOSE: hipGetLastError behind the last launch, ONE synchronisation, and only then the parts' flags set.
int pyr_close(nid_pyr *p, const char *what, unsigned parts) {
  nid_ctx *c0 = p->ctx[0];
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, std::string(what) + ": a launch failed: " + hipGetErrorString(e)));
  NID_HIP(c0, hipStreamSynchronize(c0->stream));
  pyr_mark(p, parts, true);
  return NID_OK;
}

unsigned pyr_down_blocks(const nid_ctx *dst) {
  const long threads = (long)dst->g.rows * ((dst->g.cols + kPyrRun - 1) / kPyrRun);
  return (unsigned)((threads + 255) / 256);
}

// THE REFERENCE TAIL behind level 0's depth plane: the coarser levels' depth, then every level's points and tiles.
void pyr_ref_tail(nid_pyr *p, double factor, hipStream_t st) {
  for (int l = 1; l < p->levels; l++) {
    nid_ctx *src = p->ctx[l - 1], *dst = p->ctx[l];
    hipLaunchKernelGGL(k_pyr_down_depth, dim3(pyr_down_blocks(dst)), dim3(256), 0, st, dst->g.rows, dst->g.cols, src->depth16_dev, factor,
                       dst->depth16_dev);
  }
  for (int l = 0; l < p->levels; l++) pair_u16_device_ref(p->ctx[l], factor, st);
}

}  // namespace

extern "C" {

int nid_pyr_level_config(const nid_config *cfg0, int level, nid_config *out) {
  if (!cfg0 || !out || level < 0 || level >= NID_PYR_MAX_LEVELS) return NID_ERR_INVALID_ARG;
  if (cfg0->cell_begin != 0 || cfg0->cell_end != 0) return NID_ERR_INVALID_ARG;  // shards are out of scope
  if (cfg0->rows < 1 || cfg0->cols < 1 || cfg0->cell_num < 1) return NID_ERR_INVALID_ARG;
  const int d = 1 << level;  // (the rule of nid_host_run_pyramid_lm)
  if ((cfg0->rows % d) || (cfg0->cols % d) || (cfg0->cell_num % d) || (cfg0->cell_num >> level) < 1) return NID_ERR_INVALID_ARG;
  nid_config c = *cfg0;
  for (int l = 0; l < level; l++) {  // host/nid_pyramid.cpp's operations, in its order
    c.rows = c.rows / 2; c.cols = c.cols / 2; c.cell_num = c.cell_num / 2;
    c.fx = c.fx / 2; c.fy = c.fy / 2; c.cx = (c.cx - 0.5) / 2; c.cy = (c.cy - 0.5) / 2;
  }
  *out = c;
  return NID_OK;
}

int nid_pyr_destroy(nid_pyr *p) {
  if (!p) return NID_OK;
  for (int l = 0; l < p->levels; l++) (void)nid_destroy(p->ctx[l]);  // (each selects the device: the one of every level)
  delete p;  // (the idle events)
  return NID_OK;
}

int nid_pyr_create(const nid_config *cfg0, int levels, nid_pyr **out) {
  if (!cfg0 || !out) return NID_ERR_INVALID_ARG;
  *out = nullptr;
  if (levels < 1 || levels > NID_PYR_MAX_LEVELS) return NID_ERR_INVALID_ARG;
  nid_config c;
  int rc = nid_pyr_level_config(cfg0, levels - 1, &c);
  if (rc) return rc;
  nid_pyr *p = new (std::nothrow) nid_pyr();
  if (!p) return NID_ERR_NOMEM;
  p->levels = levels;
  auto fail = [&](int code) { nid_pyr_destroy(p); return code; };
  for (int l = 0; l < levels; l++) {
    if ((rc = nid_pyr_level_config(cfg0, l, &c))) return fail(rc);
    if ((rc = nid_create(&c, &p->ctx[l]))) return fail(rc);
    // (here, not on the first pair: hipMalloc waits for the whole device)
    nid_ctx *ctx = p->ctx[l];
    if (ctx->depth16_dev.alloc((size_t)c.rows * c.cols) != hipSuccess) return fail(NID_ERR_NOMEM);
    for (Event &e : p->idle[l])
      if (e.create(hipEventDisableTiming) != hipSuccess) return fail(NID_ERR_HIP);
  }
  if (p->tdepth_dev.alloc((size_t)cfg0->rows * cfg0->cols) != hipSuccess) return fail(NID_ERR_NOMEM);
  *out = p;
  return NID_OK;
}

int nid_pyr_levels(const nid_pyr *p) { return p ? p->levels : 0; }

nid_ctx *nid_pyr_level(nid_pyr *p, int level) { return (p && level >= 0 && level < p->levels) ? p->ctx[level] : nullptr; }

int nid_pyr_set_pair_u16(nid_pyr *p, const uint16_t *depth_u16, double depth_factor, const uint8_t *im0, const uint8_t *im1,
                         const double *Twc) {
  if (!p || !depth_u16 || !im0 || !im1 || !Twc) return NID_ERR_INVALID_ARG;
  // (a pair's target comes without a depth of its own: that flag stays down)
  int rc = pyr_open(p, "nid_pyr_set_pair_u16", kPyrRef | kPyrTarget | kPyrTdepth, &depth_factor);
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const hipStream_t st = c0->stream;
  if ((rc = pair_u16_upload(c0, depth_u16, im0, im1, Twc, st))) return pyr_drain(p, rc);
  const PairStage L0 = pair_stage_layout(c0->g);
  for (int l = 1; l < p->levels; l++) {
    nid_ctx *src = p->ctx[l - 1], *dst = p->ctx[l];
    if (hipMemcpyAsync(dst->Twc_dev, c0->pair_stage + L0.twc, 16 * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess)
      return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, "nid_pyr_set_pair_u16: hipMemcpyAsync(T_wc0)"));
    hipLaunchKernelGGL(k_pyr_down, dim3(pyr_down_blocks(dst)), dim3(256), 0, st, dst->g.rows, dst->g.cols, src->im0_dev, src->im1_dev,
                       src->depth16_dev, depth_factor, dst->im0_dev, dst->im1_dev, dst->depth16_dev);
  }
  for (int l = 0; l < p->levels; l++) pair_u16_device(p->ctx[l], depth_factor, st);
  return pyr_close(p, "nid_pyr_set_pair_u16", kPyrRef | kPyrTarget);
}

int nid_pyr_get_level_inputs(nid_pyr *p, int level, uint16_t *depth_u16, uint8_t *im0, uint8_t *im1) {
  if (!p || level < 0 || level >= p->levels) return NID_ERR_INVALID_ARG;
  nid_ctx *ctx = p->ctx[level];
  if (!p->have_pair) { ctx->last_error = "nid_pyr_get_level_inputs: no pair set"; return NID_ERR_STATE; }
  NID_HIP(ctx, hipSetDevice(ctx->cfg.device));
  resident_retire(ctx);
  const size_t N = (size_t)ctx->g.rows * ctx->g.cols;
  if (depth_u16) NID_HIP(ctx, hipMemcpyAsync(depth_u16, ctx->depth16_dev, N * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
  if (im0) NID_HIP(ctx, hipMemcpyAsync(im0, ctx->im0_dev, N, hipMemcpyDeviceToHost, ctx->stream));
  if (im1) NID_HIP(ctx, hipMemcpyAsync(im1, ctx->im1_dev, N, hipMemcpyDeviceToHost, ctx->stream));
  NID_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return NID_OK;
}

int nid_pyr_multistart_lm(nid_pyr *p, const double *poses7_in, int n, const double *pose_ref7, int iterations, double delta,
                          const int32_t *keep, nid_ms_result *results, int32_t *origin, int32_t *rounds, int *best_origin,
                          double *best_pose7) {
  if (!p || !poses7_in || !results || !origin || n < 1 || n > kMaxBatchExt || iterations < 1) return NID_ERR_INVALID_ARG;
  const int L = p->levels;
  int kp[NID_PYR_MAX_LEVELS];
  for (int l = 0; l < L; l++) kp[l] = keep ? keep[l] : n;
  if (kp[L - 1] != n) return pyr_fail(p, NID_ERR_INVALID_ARG, "nid_pyr_multistart_lm: keep[levels-1] must be n");
  for (int l = 0; l + 1 < L; l++)
    if (kp[l] < 1 || kp[l] > kp[l + 1]) return pyr_fail(p, NID_ERR_INVALID_ARG, "nid_pyr_multistart_lm: 1 <= keep[l] <= keep[l+1]");
  if (!p->have_pair) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_multistart_lm: no pair set");
  if (int rc = pyr_refuse_pending(p, "nid_pyr_multistart_lm")) return rc;
  std::memset(results, 0, (size_t)L * n * sizeof(nid_ms_result));
  std::fill(origin, origin + (size_t)L * n, (int32_t)-1);
  if (rounds) std::fill(rounds, rounds + L, (int32_t)0);
  if (best_origin) *best_origin = -1;

  std::vector<double> cur(poses7_in, poses7_in + 7 * (size_t)n), next;
  std::vector<int32_t> cur_origin(n), next_origin;
  for (int k = 0; k < n; k++) cur_origin[k] = k;
  std::vector<int> order;
  int m = n;  // chains of the running level
  for (int l = L - 1; l >= 0; l--) {
    nid_ctx *ctx = p->ctx[l];
    nid_ms_result *res = results + (size_t)(L - 1 - l) * n;
    auto failed = [&](int rc) { if (l) p->ctx[0]->last_error = "level " + std::to_string(l) + ": " + ctx->last_error; return rc; };
    int rc = nid_compute_href(ctx, (l == L - 1 && pose_ref7) ? pose_ref7 : cur.data(), nullptr, nullptr, nullptr, nullptr);
    if (rc) return failed(rc);
    int r = 0;
    if ((rc = nid_multistart_lm(ctx, cur.data(), m, iterations, delta, 0, res, nullptr, nullptr, &r))) return failed(rc);
    if (rounds) rounds[L - 1 - l] = r;
    std::copy(cur_origin.begin(), cur_origin.begin() + m, origin + (size_t)(L - 1 - l) * n);
    lm::rank_chains(res, m, order);
    if (order.empty()) return NID_OK;  // (*best_origin is -1, the finer levels' rows are zero)
    if (l == 0) {
      if (best_origin) *best_origin = cur_origin[order[0]];
      if (best_pose7) std::memcpy(best_pose7, res[order[0]].pose7, 7 * sizeof(double));
      break;
    }
    m = std::min(kp[l - 1], (int)order.size());
    next.resize(7 * (size_t)m);
    next_origin.resize(m);
    for (int k = 0; k < m; k++) {
      std::memcpy(next.data() + 7 * (size_t)k, res[order[k]].pose7, 7 * sizeof(double));
      next_origin[k] = cur_origin[order[k]];
    }
    cur.swap(next);
    cur_origin.swap(next_origin);
  }
  return NID_OK;
}

}  // extern "C"

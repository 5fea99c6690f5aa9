// nid_pyr_stream.inc -- frame streams on the resident pyramid (include/nid/nid_pyr_stream.h): a new target alone, the
// resident target promoted to the reference, the pose helpers' C entry points and the tracker.
// Part of nid_capi.hip's translation unit (included behind nid_pyr.inc): it works on the pyramid's and the levels' internals.
//
// The two frame operations stand in nid_pyr.inc's frame (pyr_open over the part being overwritten, everything on level 0's
// stream in dependency order, pyr_close) and enqueue the halves of nid_pyr_set_pair_u16's chain: the TARGET half (upload,
// k_pyr_down_u8 per coarser level, pair_u16_device_target per level) or the REFERENCE half (im1 -> im0 on the device, depth
// upload, T_wc, pyr_ref_tail).  The tracker is a composition of these calls and nid_pyr_multistart_lm: it fills no pose
// record and launches no evaluation.

struct nid_track {
  nid_pyr *pyr = nullptr;
  int iterations = 10;
  double delta = 0.97467943448089633;  // sqrt(0.95)
  bool have_keep = false;
  int32_t keep[NID_PYR_MAX_LEVELS] = {};
  std::vector<double> twists;  // n x 6
  bool have_prev = false;  // the velocity is known: prev is the pose of the frame before cur's
  double cur[7] = {0, 0, 0, 1, 0, 0, 0}, prev[7] = {0, 0, 0, 1, 0, 0, 0};
  int32_t frame = 0;  // pushes that returned NID_OK
  std::vector<nid_ms_result> results;
  std::vector<int32_t> origin;
  // nid_keyframe.h (nid_keyframe.inc): the policy, the frames tracked OK on the keyframe, and what the last push checked
  nid_track_policy policy = {0, 0, 0, 0, 0.0, 0.0, 0.01, 0.02};
  int32_t age = 0, n_checked = 0;
  nid_depth_counts chosen = {};
  // nid_refmask.h (nid_refmask.inc): the classes masked behind a frame tracked on the keyframe (0: masking is off), the
  // dilation, and the counts of the last push's step 5e
  int32_t mask_classes = 0, mask_dilate = 0;
  nid_refmask_counts last_mask = {}, push_mask = {};  // (push_mask: of the push under way, kept when it returns NID_OK)
  // nid_reffill.h (nid_reffill.inc): whether a frame tracked on the keyframe fills its depth holes, the guard, and the
  // counts of the last push's fill
  bool fill_on = false;
  int32_t fill_guard = 0, fill_guard_abs = 0, fill_guard_rel_1024 = 0;
  nid_reffill_counts last_fill = {}, push_fill = {};  // (push_fill: as push_mask)
  // nid_reffuse.h (nid_reffuse.inc): whether such a frame refines the keyframe's valid depth, the gate, the cap, and the
  // counts of the last push's fusion
  bool fuse_on = false;
  int32_t fuse_gate_abs = 0, fuse_gate_rel_1024 = 0, fuse_max_obs = 1;
  nid_reffuse_counts last_fusion = {}, push_fusion = {};  // (push_fusion: as push_mask)
  // nid_refgather.h (nid_refgather.inc): where such a fusion takes its observations from, the tap gate of a bilinear one, and
  // the counts of the last push's gather
  int32_t fuse_sampling = NID_REFFUSE_NEAREST, fuse_tap_abs = 0, fuse_tap_rel_1024 = 0;
  nid_refgather_counts last_gather = {}, push_gather = {};  // (push_gather: as push_mask)
};

namespace {

// A later frame with depth under an active policy (nid_keyframe.inc, behind this file): steps 5a - 5d of nid_keyframe.h
// (and, with masking set, step 5e of nid_refmask.h) on the chains nid_pyr_multistart_lm left in t->results / t->origin.  It moves cur / prev as nid_track_push_u16 does, behind
// its last call that can fail; the age and the last check's record are nid_track_push_u16's to keep.
int track_finish_with_policy(nid_track *t, int n, nid_track_result *R, nid_depth_counts *chosen, int32_t *n_checked);

// The REFERENCE half for nid_pyr_promote_target_u16 (depth_u16: the caller's map, uploaded) and nid_pyr_promote_target
// (depth_u16 == NULL: the resident target depth, copied on the device); `what` names the call in an error.
int pyr_promote(nid_pyr *p, const uint16_t *depth_u16, double depth_factor, const double *Twc, const char *what) {
  for (int l = 0; l < p->levels; l++)
    if (!p->ctx[l]->have_target) return pyr_fail(p, NID_ERR_STATE, std::string(what) + ": no target on level " + std::to_string(l));
  if (!depth_u16 && !p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, std::string(what) + ": the target has no depth: nid_pyr_set_target_depth_u16() first");
  int rc = pyr_open(p, what, kPyrRef, &depth_factor);
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const hipStream_t st = c0->stream;
  if ((rc = pair_stage_ensure(c0))) return rc;  // (nothing enqueued yet)
  const PairStage L0 = pair_stage_layout(c0->g);
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  if (depth_u16) std::memcpy(c0->pair_stage + L0.depth, depth_u16, 2 * N);
  std::memcpy(c0->pair_stage + L0.twc, Twc, 16 * sizeof(double));
  auto copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) { return hipMemcpyAsync(dst, src, bytes, kind, st) == hipSuccess; };
  bool ok = depth_u16 ? copy(c0->depth16_dev, c0->pair_stage + L0.depth, 2 * N, hipMemcpyHostToDevice)
                      : copy(c0->depth16_dev, p->tdepth_dev, 2 * N, hipMemcpyDeviceToDevice);
  for (int l = 0; ok && l < p->levels; l++) {
    nid_ctx *ctx = p->ctx[l];
    ok = copy(ctx->im0_dev, ctx->im1_dev, (size_t)ctx->g.rows * ctx->g.cols, hipMemcpyDeviceToDevice) &&
         copy(ctx->Twc_dev, c0->pair_stage + L0.twc, 16 * sizeof(double), hipMemcpyHostToDevice);
  }
  if (!ok) return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, std::string(what) + ": hipMemcpyAsync"));
  pyr_ref_tail(p, depth_factor, st);
  return pyr_close(p, what, kPyrRef);
}

}  // namespace

extern "C" {

int nid_pyr_set_target_u8(nid_pyr *p, const uint8_t *im1) {
  if (!p || !im1) return NID_ERR_INVALID_ARG;
  int rc = pyr_open(p, "nid_pyr_set_target_u8", kPyrTarget | kPyrTdepth);  // (nid_keyframe.h: a target's depth belongs to its image)
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const hipStream_t st = c0->stream;
  if ((rc = pair_stage_ensure(c0))) return rc;  // (nothing enqueued yet)
  const PairStage L0 = pair_stage_layout(c0->g);
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  std::memcpy(c0->pair_stage + L0.im1, im1, N);
  if (hipMemcpyAsync(c0->im1_dev, c0->pair_stage + L0.im1, N, hipMemcpyHostToDevice, st) != hipSuccess)
    return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, "nid_pyr_set_target_u8: hipMemcpyAsync(im1)"));
  for (int l = 1; l < p->levels; l++) {
    nid_ctx *src = p->ctx[l - 1], *dst = p->ctx[l];
    hipLaunchKernelGGL(k_pyr_down_u8, dim3(pyr_down_blocks(dst)), dim3(256), 0, st, dst->g.rows, dst->g.cols, src->im1_dev, dst->im1_dev);
  }
  for (int l = 0; l < p->levels; l++) pair_u16_device_target(p->ctx[l], st);
  return pyr_close(p, "nid_pyr_set_target_u8", kPyrTarget);
}

int nid_pyr_promote_target_u16(nid_pyr *p, const uint16_t *depth_u16, double depth_factor, const double *Twc) {
  if (!p || !depth_u16 || !Twc) return NID_ERR_INVALID_ARG;
  return pyr_promote(p, depth_u16, depth_factor, Twc, "nid_pyr_promote_target_u16");
}

// ---- pose helpers (csrc/nid_track_pose.h) ---------------------------------------------------------------------------
int nid_track_pose_inverse(const double *pose7, double *out7) {
  if (!pose7 || !out7) return NID_ERR_INVALID_ARG;
  track::pose_inverse(pose7, out7);
  return NID_OK;
}

int nid_track_pose_compose(const double *a7, const double *b7, double *out7) {
  if (!a7 || !b7 || !out7) return NID_ERR_INVALID_ARG;
  track::pose_compose(a7, b7, out7);
  return NID_OK;
}

int nid_track_pose_perturb(const double *pose7, const double *twist6, double *out7) {
  if (!pose7 || !twist6 || !out7) return NID_ERR_INVALID_ARG;
  track::pose_perturb(pose7, twist6, out7);
  return NID_OK;
}

int nid_track_pose_to_Twc16(const double *pose7_cw, double *T16) {
  if (!pose7_cw || !T16) return NID_ERR_INVALID_ARG;
  track::pose_to_Twc16(pose7_cw, T16);
  return NID_OK;
}

int nid_track_pose_from_Twc16(const double *T16, double *pose7_cw) {
  if (!T16 || !pose7_cw) return NID_ERR_INVALID_ARG;
  track::pose_from_Twc16(T16, pose7_cw);
  return NID_OK;
}

// ---- the tracker ----------------------------------------------------------------------------------------------------
int nid_track_destroy(nid_track *t) {
  if (!t) return NID_OK;
  (void)nid_pyr_destroy(t->pyr);
  delete t;
  return NID_OK;
}

int nid_track_create(const nid_config *cfg0, int levels, nid_track **out) {
  if (!cfg0 || !out) return NID_ERR_INVALID_ARG;
  *out = nullptr;
  nid_track *t = new (std::nothrow) nid_track();
  if (!t) return NID_ERR_NOMEM;
  const int rc = nid_pyr_create(cfg0, levels, &t->pyr);  // (its argument checks come before any device)
  if (rc) { delete t; return rc; }
  *out = t;
  return NID_OK;
}

nid_pyr *nid_track_pyramid(nid_track *t) { return t ? t->pyr : nullptr; }

int nid_track_set_lm(nid_track *t, int iterations, double huber_delta, const int32_t *keep) {
  if (!t || iterations < 1) return NID_ERR_INVALID_ARG;
  const int L = t->pyr->levels;
  if (keep)
    for (int l = 0; l < L; l++)
      if (keep[l] < 1 || (l + 1 < L && keep[l] > keep[l + 1])) return NID_ERR_INVALID_ARG;
  t->iterations = iterations;
  t->delta = huber_delta;
  t->have_keep = keep != nullptr;
  if (keep) std::copy(keep, keep + L, t->keep);
  return NID_OK;
}

int nid_track_set_twists(nid_track *t, const double *twists6, int n) {
  if (!t || n < 0 || n > NID_MAX_BATCH - 2 || (n > 0 && !twists6)) return NID_ERR_INVALID_ARG;
  t->twists.assign(twists6, twists6 + 6 * (size_t)n);
  return NID_OK;
}

int nid_track_set_pose(nid_track *t, const double *pose7) {
  if (!t || !pose7) return NID_ERR_INVALID_ARG;
  std::memcpy(t->cur, pose7, sizeof(t->cur));
  t->have_prev = false;
  return NID_OK;
}

int nid_track_push_u16(nid_track *t, const uint16_t *depth_u16, double depth_factor, const uint8_t *im, const double *Twc_first,
                       nid_track_result *out) {
  if (!t || !im || !out) return NID_ERR_INVALID_ARG;
  nid_pyr *p = t->pyr;
  const bool first = !p->have_pair;  // no reference yet (also after a promotion that failed)
  if (first && !depth_u16) return NID_ERR_INVALID_ARG;
  nid_track_result R = {};
  R.best_origin = -1;
  R.frame = t->frame;
  nid_depth_counts chosen = {};  // (nid_keyframe.h: what this push checked, kept with the poses when it returns NID_OK)
  int32_t n_checked = 0;
  t->push_mask = nid_refmask_counts();  // (nid_refmask.h: step 5e's counts, if this push runs it)
  t->push_fill = nid_reffill_counts();  // (nid_reffill.h: the fill's counts, likewise)
  t->push_fusion = nid_reffuse_counts();  // (nid_reffuse.h: the fusion's)
  t->push_gather = nid_refgather_counts();  // (nid_refgather.h: the gather's)
  int rc = nid_pyr_set_target_u8(p, im);
  if (rc) return rc;
  if (first) {
    static const double identity16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const double *Twc = Twc_first ? Twc_first : identity16;
    if ((rc = nid_pyr_promote_target_u16(p, depth_u16, depth_factor, Twc))) return rc;
    track::pose_from_Twc16(Twc, t->cur);
    t->have_prev = false;
    R.status = NID_TRACK_FIRST;
    R.promoted = 1;
  } else {
    const int n = 2 + (int)(t->twists.size() / 6), L = p->levels;
    double starts[NID_MAX_BATCH * 7];
    double *pred = starts, *cur = starts + 7;
    std::memcpy(cur, t->cur, sizeof(t->cur));
    if (t->have_prev) {
      double inv[7], vel[7];
      track::pose_inverse(t->prev, inv);
      track::pose_compose(t->cur, inv, vel);
      track::pose_compose(vel, t->cur, pred);
    } else {
      std::memcpy(pred, t->cur, sizeof(t->cur));
    }
    for (int k = 2; k < n; k++) track::pose_perturb(pred, t->twists.data() + 6 * (size_t)(k - 2), starts + 7 * (size_t)k);
    t->results.resize((size_t)L * n);
    t->origin.resize((size_t)L * n);
    int best = -1;
    double best_pose[7];
    // (nid_keyframe.h: an active policy and a frame with depth -- the depth stays on the device for the check and the promotion)
    const bool with_policy = depth_u16 && dc::policy_active(t->policy);
    if (with_policy && (rc = nid_pyr_set_target_depth_u16(p, depth_u16, depth_factor))) return rc;
    if ((rc = nid_pyr_multistart_lm(p, starts, n, nullptr, t->iterations, t->delta, t->have_keep ? t->keep : nullptr, t->results.data(),
                                    t->origin.data(), R.rounds, &best, best_pose)))
      return rc;
    R.best_origin = best;
    if (with_policy && best >= 0) {
      if ((rc = track_finish_with_policy(t, n, &R, &chosen, &n_checked))) return rc;
    } else if (best >= 0) {
      if (depth_u16) {
        double Twc[16];
        track::pose_to_Twc16(best_pose, Twc);
        if ((rc = nid_pyr_promote_target_u16(p, depth_u16, depth_factor, Twc))) return rc;
        R.promoted = 1;
      }
      const nid_ms_result *row = t->results.data() + (size_t)(L - 1) * n;  // level 0's chains
      const int32_t *org = t->origin.data() + (size_t)(L - 1) * n;
      for (int k = 0; k < n; k++)
        if (org[k] == best) { R.chi2 = row[k].chi2; R.n_active = row[k].n_active; break; }
      std::memcpy(t->prev, t->cur, sizeof(t->cur));
      std::memcpy(t->cur, best_pose, sizeof(t->cur));
      t->have_prev = true;
      R.status = NID_TRACK_OK;
    } else {
      t->have_prev = false;
      R.status = NID_TRACK_LOST;
    }
  }
  std::memcpy(R.pose7, t->cur, sizeof(t->cur));
  if (R.promoted) t->age = 0;  // frames tracked OK on the keyframe since it was promoted
  else if (R.status == NID_TRACK_OK) t->age++;
  t->chosen = chosen;
  t->n_checked = n_checked;
  t->last_mask = t->push_mask;
  t->last_fill = t->push_fill;
  t->last_fusion = t->push_fusion;
  t->last_gather = t->push_gather;
  t->frame++;
  *out = R;
  return NID_OK;
}

}  // extern "C"

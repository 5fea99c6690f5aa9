// nid_refmask.inc -- the per-pixel mask on the resident pyramid's reference and the tracker's use of it
// (include/nid/nid_refmask.h).  Part of nid_capi.hip's translation unit (included behind nid_keyframe.inc).
//
// The three masking calls are ONE chain on level 0's stream with three ways to its front: the pristine copy and a zero
// plane if this is the first call behind a new reference; the classified bytes into work_dev -- the caller's plane
// uploaded (nid_pyr_set_reference_mask_u8), zeros (nid_pyr_clear_reference_mask) or k_refmask_classify
// (nid_pyr_mask_occluded) --; then k_refmask_dilate_apply (the final plane, level 0's masked depth, the counts), the
// REFERENCE half of a promotion from there on (k_pyr_down_depth per coarser level, pair_u16_device_ref per level:
// nid_pyr_stream.inc) and the counts' way home.  They open and close like the frame operations and leave every level as a
// promotion does.  No evaluation kernel is launched, no SlotArgs filled, no slot touched.
// nid_reffill.inc (behind this file) runs the same chain with a fourth front -- the plane as it is -- and its own kernels
// between the pristine copy and the front (RmBefore): there the pristine depth is what a fill makes of the uploaded one.

namespace {

enum class RmFront { kCallerPlane, kZeros, kClassify, kKeep };  // (kKeep: the plane as it is -- nid_reffill.inc's front)

// what a call puts between the pristine copy and the front (nid_reffill.inc: the kernels that rewrite pristine_dev)
struct RmBefore {
  int (*enqueue)(nid_pyr *p, const void *arg, hipStream_t st, const char *what);  // NID_OK, or the error behind pyr_fail
  const void *arg;
};

int rm_ensure(nid_pyr *p, bool plane_host) {
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask &R = p->rm;
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  NID_HIP(c0, R.pristine_dev.grow(N));
  NID_HIP(c0, R.mask_dev.grow(N));
  NID_HIP(c0, R.work_dev.grow(N));
  NID_HIP(c0, R.counts_dev.grow(8));
  NID_HIP(c0, R.counts_host.grow(8));
  if (plane_host) NID_HIP(c0, R.plane_host.grow(N));
  return NID_OK;
}

// the state errors every masking call shares (nothing changed behind one)
int rm_refuse(nid_pyr *p, const char *what) {
  if (!p->have_pair || !p->ctx[0]->have_ref) return pyr_fail(p, NID_ERR_STATE, std::string(what) + ": no reference");
  return pyr_refuse_pending(p, what);
}

// the chain; A: k_refmask_classify's arguments but the planes (kClassify only), caller: the plane of kCallerPlane
int rm_run(nid_pyr *p, RmFront front, const RefMaskArgs *A, const uint8_t *caller, int dilate, nid_refmask_counts *out, const char *what,
           const RmBefore *before = nullptr) {
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask &R = p->rm;
  // from here on the reference is being overwritten: no level has one until the stream has drained
  p->have_pair = false;
  for (int l = 0; l < p->levels; l++) p->ctx[l]->have_ref = p->ctx[l]->have_href = false;
  int rc = pyr_front(p);
  if (rc) return rc;
  if ((rc = rm_ensure(p, front == RmFront::kCallerPlane))) return rc;  // (nothing enqueued yet)
  const hipStream_t st = c0->stream;
  const Geometry &g = c0->g;
  const size_t N = (size_t)g.rows * g.cols;
  auto failed = [&](const char *step) { return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, std::string(what) + ": " + step)); };
  if (!R.have_pristine) {
    if (hipMemcpyAsync(R.pristine_dev, c0->depth16_dev, 2 * N, hipMemcpyDeviceToDevice, st) != hipSuccess) return failed("hipMemcpyAsync(pristine)");
    if (hipMemsetAsync(R.mask_dev, 0, N, st) != hipSuccess) return failed("hipMemsetAsync(mask)");
  }
  if (hipMemsetAsync(R.counts_dev, 0, 8 * sizeof(unsigned long long), st) != hipSuccess) return failed("hipMemsetAsync(counts)");
  if (before && (rc = before->enqueue(p, before->arg, st, what))) return pyr_drain(p, rc);
  if (front == RmFront::kCallerPlane) {
    uint8_t *h = R.plane_host;
    for (size_t i = 0; i < N; i++) h[i] = caller[i] ? NID_REFMASK_CALLER : 0;
    if (hipMemcpyAsync(R.work_dev, h, N, hipMemcpyHostToDevice, st) != hipSuccess) return failed("hipMemcpyAsync(mask)");
  } else if (front == RmFront::kZeros) {
    if (hipMemsetAsync(R.work_dev, 0, N, st) != hipSuccess) return failed("hipMemsetAsync(work)");
  } else if (front == RmFront::kKeep) {  // (a final plane through dc::mask_final with dilate 0 is itself)
    if (hipMemcpyAsync(R.work_dev, R.mask_dev, N, hipMemcpyDeviceToDevice, st) != hipSuccess) return failed("hipMemcpyAsync(work)");
  } else {
    RefMaskArgs a = *A;
    a.d0 = R.pristine_dev; a.Twc = c0->Twc_dev; a.d1 = p->tdepth_dev;
    a.factor0 = R.ref_factor; a.factor1 = p->tdepth_factor;
    hipLaunchKernelGGL(k_refmask_classify, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, g, a, R.mask_dev.get(), R.work_dev.get());
  }
  hipLaunchKernelGGL(k_refmask_dilate_apply, dim3((unsigned)((g.cols + kRmTileW - 1) / kRmTileW), (unsigned)((g.rows + kRmTileH - 1) / kRmTileH)), dim3(256),
                     0, st, g.rows, g.cols, dilate, R.work_dev.get(), R.pristine_dev.get(), R.ref_factor, R.mask_dev.get(), c0->depth16_dev.get(),
                     R.counts_dev.get());
  for (int l = 1; l < p->levels; l++) {
    nid_ctx *src = p->ctx[l - 1], *dst = p->ctx[l];
    hipLaunchKernelGGL(k_pyr_down_depth, dim3(pyr_down_blocks(dst)), dim3(256), 0, st, dst->g.rows, dst->g.cols, src->depth16_dev, R.ref_factor,
                       dst->depth16_dev);
  }
  for (int l = 0; l < p->levels; l++) pair_u16_device_ref(p->ctx[l], R.ref_factor, st);
  if (hipGetLastError() != hipSuccess) return failed("a launch failed");
  if (hipMemcpyAsync(R.counts_host, R.counts_dev, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) return failed("hipMemcpyAsync(counts)");
  if ((rc = pyr_finish(p, what))) return rc;
  for (int l = 0; l < p->levels; l++) {
    nid_ctx *ctx = p->ctx[l];
    ctx->have_ref = true;  // (have_href stays false: the reference stage is the caller's)
    ctx->ref_from_depth = true;
  }
  p->have_pair = true;
  R.have_pristine = true;
  const unsigned long long *n = R.counts_host;
  R.any_masked = n[kRmCountWords - 1] != 0;
  if (out) {
    *out = nid_refmask_counts();
    std::memcpy(out, n, 6 * sizeof(int64_t));
  }
  return NID_OK;
}

}  // namespace

extern "C" {

int nid_pyr_set_reference_mask_u8(nid_pyr *p, const uint8_t *mask) {
  if (!p || !mask) return NID_ERR_INVALID_ARG;
  const int rc = rm_refuse(p, "nid_pyr_set_reference_mask_u8");
  if (rc) return rc;
  return rm_run(p, RmFront::kCallerPlane, nullptr, mask, 0, nullptr, "nid_pyr_set_reference_mask_u8");
}

int nid_pyr_mask_occluded(nid_pyr *p, const double *pose7, double tol_abs, double tol_rel, int classes, int dilate, int accumulate,
                          nid_refmask_counts *out) {
  if (!p || !pose7 || !dc::refmask_args_ok(tol_abs, tol_rel, classes, dilate)) return NID_ERR_INVALID_ARG;
  int rc = rm_refuse(p, "nid_pyr_mask_occluded");
  if (rc) return rc;
  if (!p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_mask_occluded: the target has no depth: nid_pyr_set_target_depth_u16() first");
  RefMaskArgs A = {};
  double q7[7];
  int32_t mode;
  lm::pose_record(pose7, p->ctx[0]->xform, q7, A.M, &mode);
  A.tol_abs = tol_abs; A.tol_rel = tol_rel;
  A.classes = classes; A.accumulate = accumulate != 0;
  return rm_run(p, RmFront::kClassify, &A, nullptr, dilate, out, "nid_pyr_mask_occluded");
}

int nid_pyr_clear_reference_mask(nid_pyr *p) {
  if (!p) return NID_ERR_INVALID_ARG;
  const int rc = rm_refuse(p, "nid_pyr_clear_reference_mask");
  if (rc) return rc;
  if (!p->rm.have_pristine || !p->rm.any_masked) return NID_OK;  // nothing is masked
  return rm_run(p, RmFront::kZeros, nullptr, nullptr, 0, nullptr, "nid_pyr_clear_reference_mask");
}

int nid_pyr_get_reference_mask_u8(nid_pyr *p, uint8_t *out) {
  if (!p || !out) return NID_ERR_INVALID_ARG;
  const int rc = rm_refuse(p, "nid_pyr_get_reference_mask_u8");
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  if (!p->rm.have_pristine) {  // a new reference starts unmasked
    std::memset(out, 0, N);
    return NID_OK;
  }
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  resident_retire(c0);
  NID_HIP(c0, hipMemcpyAsync(out, p->rm.mask_dev, N, hipMemcpyDeviceToHost, c0->stream));
  NID_HIP(c0, hipStreamSynchronize(c0->stream));
  return NID_OK;
}

int nid_refmask_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *Twc, const uint16_t *depth1_u16,
                     double factor1, const double *pose7, double tol_abs, double tol_rel, int classes, int dilate, int accumulate,
                     uint8_t *mask_inout, nid_refmask_counts *counts) {
  if (!cfg || !depth0_u16 || !Twc || !depth1_u16 || !pose7 || !mask_inout || !dc::refmask_args_ok(tol_abs, tol_rel, classes, dilate)) return NID_ERR_INVALID_ARG;
  if (cfg->rows < 1 || cfg->cols < 1 || (int64_t)cfg->rows * cfg->cols > INT32_MAX) return NID_ERR_INVALID_ARG;
  dc::View V;
  double q7[7];
  int32_t mode;
  lm::pose_record(pose7, NID_XFORM_QUAT, q7, V.M, &mode);
  V.fx = cfg->fx; V.fy = cfg->fy; V.cx = cfg->cx; V.cy = cfg->cy;
  V.rows = cfg->rows; V.cols = cfg->cols;
  V.d1 = depth1_u16; V.factor = factor1; V.tol_abs = tol_abs; V.tol_rel = tol_rel;
  const dc::Keyframe K = {depth0_u16, factor0, Twc};
  dc::refmask_host(V, K, classes, dilate, accumulate != 0, mask_inout, counts);
  return NID_OK;
}

int nid_track_set_masking(nid_track *t, int classes, int dilate) {
  if (!t || !dc::refmask_args_ok(0.0, 0.0, classes, dilate)) return NID_ERR_INVALID_ARG;
  t->mask_classes = classes;
  t->mask_dilate = dilate;
  return NID_OK;
}

int nid_track_last_mask(const nid_track *t, nid_refmask_counts *counts) {
  if (!t || !counts) return NID_ERR_INVALID_ARG;
  *counts = t->last_mask;
  return NID_OK;
}

}  // extern "C"

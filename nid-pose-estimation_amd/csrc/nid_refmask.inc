// nid_refmask.inc -- the per-pixel mask on the resident pyramid's reference and the tracker's use of it
// (include/nid/nid_refmask.h).  Part of nid_capi.hip's translation unit (included behind nid_keyframe.inc).
//
// A masking call is straight-line code on level 0's stream in nid_pyr.inc's frame: rm_begin (pyr_open over the reference;
// the pristine copy and a zero plane if this is the first call behind a new reference; the counts zeroed), the call's own
// MIDDLE -- the classified bytes into work_dev: the caller's plane uploaded (nid_pyr_set_reference_mask_u8), zeros
// (nid_pyr_clear_reference_mask) or k_refmask_classify (nid_pyr_mask_occluded) --, and rm_finish (k_refmask_dilate_apply:
// the final plane, level 0's masked depth, the counts; pyr_ref_tail; the counts' way home; pyr_close), which leaves every
// level as a promotion does.  No evaluation kernel is launched, no SlotArgs filled, no slot touched.
// nid_reffill.inc (behind this file) puts its own operations between the same two: there the pristine depth is what a fill
// makes of the uploaded one, and the plane goes into work_dev as it is.

namespace {

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

// an error between rm_begin and rm_finish: nothing of the call stays in flight
int rm_failed(nid_pyr *p, const char *what, const char *step) {
  return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, std::string(what) + ": " + step));
}

int rm_begin(nid_pyr *p, const char *what, bool plane_host = false) {
  int rc = pyr_open(p, what, kPyrRef);  // (the resident reference made again, not a new one: its mask and fill stay)
  if (rc) return rc;
  if ((rc = rm_ensure(p, plane_host))) return rc;  // (nothing enqueued yet)
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask &R = p->rm;
  const hipStream_t st = c0->stream;
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  if (!R.have_pristine) {
    if (hipMemcpyAsync(R.pristine_dev, c0->depth16_dev, 2 * N, hipMemcpyDeviceToDevice, st) != hipSuccess) return rm_failed(p, what, "hipMemcpyAsync(pristine)");
    if (hipMemsetAsync(R.mask_dev, 0, N, st) != hipSuccess) return rm_failed(p, what, "hipMemsetAsync(mask)");
  }
  if (hipMemsetAsync(R.counts_dev, 0, 8 * sizeof(unsigned long long), st) != hipSuccess) return rm_failed(p, what, "hipMemsetAsync(counts)");
  return NID_OK;
}

// work_dev holds the call's classified bytes, in stream order
int rm_finish(nid_pyr *p, const char *what, int dilate, nid_refmask_counts *out) {
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask &R = p->rm;
  const hipStream_t st = c0->stream;
  const Geometry &g = c0->g;
  hipLaunchKernelGGL(k_refmask_dilate_apply, dim3((unsigned)((g.cols + kRmTileW - 1) / kRmTileW), (unsigned)((g.rows + kRmTileH - 1) / kRmTileH)), dim3(256),
                     0, st, g.rows, g.cols, dilate, R.work_dev.get(), R.pristine_dev.get(), R.ref_factor, R.mask_dev.get(), c0->depth16_dev.get(),
                     R.counts_dev.get());
  pyr_ref_tail(p, R.ref_factor, st);
  if (hipGetLastError() != hipSuccess) return rm_failed(p, what, "a launch failed");
  if (hipMemcpyAsync(R.counts_host, R.counts_dev, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) return rm_failed(p, what, "hipMemcpyAsync(counts)");
  const int rc = pyr_close(p, what, kPyrRef);
  if (rc) return rc;
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
  const char *what = "nid_pyr_set_reference_mask_u8";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  if ((rc = rm_begin(p, what, true))) return rc;
  nid_pyr::RefMask &R = p->rm;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  uint8_t *h = R.plane_host;
  for (size_t i = 0; i < N; i++) h[i] = mask[i] ? NID_REFMASK_CALLER : 0;
  if (hipMemcpyAsync(R.work_dev, h, N, hipMemcpyHostToDevice, p->ctx[0]->stream) != hipSuccess) return rm_failed(p, what, "hipMemcpyAsync(mask)");
  return rm_finish(p, what, 0, nullptr);
}

int nid_pyr_mask_occluded(nid_pyr *p, const double *pose7, double tol_abs, double tol_rel, int classes, int dilate, int accumulate,
                          nid_refmask_counts *out) {
  if (!p || !pose7 || !dc::refmask_args_ok(tol_abs, tol_rel, classes, dilate)) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_mask_occluded";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  if (!p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_mask_occluded: the target has no depth: nid_pyr_set_target_depth_u16() first");
  if ((rc = rm_begin(p, what))) return rc;
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask &R = p->rm;
  RefMaskArgs A = {};
  double q7[7];
  int32_t mode;
  lm::pose_record(pose7, c0->xform, q7, A.M, &mode);
  A.d0 = R.pristine_dev; A.Twc = c0->Twc_dev; A.d1 = p->tdepth_dev;
  A.factor0 = R.ref_factor; A.factor1 = p->tdepth_factor; A.tol_abs = tol_abs; A.tol_rel = tol_rel;
  A.classes = classes; A.accumulate = accumulate != 0;
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  hipLaunchKernelGGL(k_refmask_classify, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c0->stream, c0->g, A, R.mask_dev.get(), R.work_dev.get());
  return rm_finish(p, what, dilate, out);
}

int nid_pyr_clear_reference_mask(nid_pyr *p) {
  if (!p) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_clear_reference_mask";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  if (!p->rm.have_pristine || !p->rm.any_masked) return NID_OK;  // nothing is masked
  if ((rc = rm_begin(p, what))) return rc;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  if (hipMemsetAsync(p->rm.work_dev, 0, N, p->ctx[0]->stream) != hipSuccess) return rm_failed(p, what, "hipMemsetAsync(work)");
  return rm_finish(p, what, 0, nullptr);
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
  double q7[7], M[12];
  int32_t mode;
  lm::pose_record(pose7, NID_XFORM_QUAT, q7, M, &mode);
  const dc::View V = dc::make_view(*cfg, M, depth1_u16, factor1, tol_abs, tol_rel);
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

// nid_reffill.inc -- depth for the holes of the resident pyramid's reference from tracked frames, and the tracker's use of
// it (include/nid/nid_reffill.h).  Part of nid_capi.hip's translation unit (included behind nid_refmask.inc).
//
// A fill call is a masking call (nid_refmask.inc's rm_begin ... rm_finish) that keeps the plane and rewrites the PRISTINE
// depth in its middle.  rf_begin: behind rm_begin's own pristine copy come, on the same stream, the uploaded copy and a
// zero fill plane if this is the first fill behind a new reference, and the fill's counts zeroed.  The call's own part:
// the z-buffer's 0xFF bytes, k_reffill_splat and k_reffill_apply (the fill plane, pristine = fill ? fill : uploaded, the
// counts) -- or, for nid_pyr_clear_reference_fill, zeros into the plane and the uploaded copy back into the pristine depth.
// (Behind a fusion of nid_reffuse.h, "uploaded" in both is its BASE plane: rf_base.)
// rf_finish: the counts' way home, the mask plane as it is into work_dev -- a final plane through dc::mask_final with
// dilate 0 is itself --, and rm_finish, which makes the effective reference of it and closes the call with its one
// synchronisation.  No evaluation kernel is launched, no SlotArgs filled, no slot touched.

namespace {

// the fill's buffers, made before anything of the call changes the pyramid
int rf_ensure(nid_pyr *p) {
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask::Fill &F = p->rm.fill;
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  NID_HIP(c0, F.uploaded_dev.grow(N));
  NID_HIP(c0, F.fill_dev.grow(N));
  NID_HIP(c0, F.zbuf_dev.grow(N));
  NID_HIP(c0, F.counts_dev.grow(8));
  NID_HIP(c0, F.counts_host.grow(8));
  return NID_OK;
}

// a fill call that fails behind rf_ensure: the planes may be half made (the reference is not ready either); the fusion's
// state (nid_reffuse.inc) stands on them
int rf_failed(nid_pyr *p, int rc) {
  p->rm.fill.have_uploaded = p->rm.fill.any_filled = p->rm.fuse.have_state = p->rm.fuse.any_fused = false;
  return rc;
}

int rf_failed(nid_pyr *p, const char *what, const char *step) { return rf_failed(p, rm_failed(p, what, step)); }

// behind it pristine_dev is the reference's pristine depth, in stream order
int rf_begin(nid_pyr *p, const char *what) {
  int rc = rf_ensure(p);
  if (rc) return rc;
  if ((rc = rm_begin(p, what))) return rf_failed(p, rc);
  nid_pyr::RefMask &R = p->rm;
  nid_pyr::RefMask::Fill &F = R.fill;
  const hipStream_t st = p->ctx[0]->stream;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  if (!F.have_uploaded) {  // (nothing is filled yet: the pristine depth is the uploaded one)
    if (hipMemcpyAsync(F.uploaded_dev, R.pristine_dev, 2 * N, hipMemcpyDeviceToDevice, st) != hipSuccess) return rf_failed(p, what, "hipMemcpyAsync(uploaded)");
    if (hipMemsetAsync(F.fill_dev, 0, 2 * N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(fill)");
  }
  if (hipMemsetAsync(F.counts_dev, 0, 8 * sizeof(unsigned long long), st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(fill counts)");
  return NID_OK;
}

// part A's arguments for pose7 against the resident target depth (on the host: nothing is enqueued)
RefFillArgs rf_splat_args(nid_pyr *p, const double *pose7) {
  nid_ctx *c0 = p->ctx[0];
  RefFillArgs A = {};
  double Twc[16];  // the host's copy of the keyframe's matrix: where whatever made the reference staged it
  std::memcpy(Twc, c0->pair_stage + pair_stage_layout(c0->g).twc, sizeof(Twc));
  rf::target_to_keyframe(Twc, pose7, A.M);
  A.d1 = p->tdepth_dev;
  A.factor1 = p->tdepth_factor;
  A.factor0 = p->rm.ref_factor;
  return A;
}

// part A behind rf_begin: the z-buffer's 0xFF bytes and k_reffill_splat (words 0 and 1 of the call's totals)
int rf_splat(nid_pyr *p, const char *what, const RefFillArgs &A) {
  nid_pyr::RefMask::Fill &F = p->rm.fill;
  const hipStream_t st = p->ctx[0]->stream;
  const Geometry &g = p->ctx[0]->g;
  const size_t N = (size_t)g.rows * g.cols;
  if (hipMemsetAsync(F.zbuf_dev, 0xFF, 4 * N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(zbuf)");
  hipLaunchKernelGGL(k_reffill_splat, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, g, A, F.zbuf_dev.get(), F.counts_dev.get());
  return NID_OK;
}

// the keyframe's own samples as a fill reads them: the BASE plane of nid_reffuse.h once a fusion state exists, else the
// uploaded copy
const uint16_t *rf_base(nid_pyr *p) { return p->rm.fuse.have_state ? p->rm.fuse.base_dev.get() : p->rm.fill.uploaded_dev.get(); }

// the close of a fill call and of a fusion call (nid_reffuse.inc): behind it counts_host holds the call's eight totals
int rf_close(nid_pyr *p, const char *what) {
  nid_pyr::RefMask &R = p->rm;
  nid_pyr::RefMask::Fill &F = R.fill;
  const hipStream_t st = p->ctx[0]->stream;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  if (hipMemcpyAsync(F.counts_host, F.counts_dev, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) return rf_failed(p, what, "hipMemcpyAsync(fill counts)");
  if (hipMemcpyAsync(R.work_dev, R.mask_dev, N, hipMemcpyDeviceToDevice, st) != hipSuccess) return rf_failed(p, what, "hipMemcpyAsync(work)");
  const int rc = rm_finish(p, what, 0, nullptr);
  if (rc) return rf_failed(p, rc);
  F.have_uploaded = true;
  return NID_OK;
}

int rf_finish(nid_pyr *p, const char *what, nid_reffill_counts *out) {
  nid_pyr::RefMask::Fill &F = p->rm.fill;
  const int rc = rf_close(p, what);
  if (rc) return rc;
  static_assert(sizeof(nid_reffill_counts) == 8 * sizeof(unsigned long long), "the totals are the record");
  nid_reffill_counts n;
  std::memcpy(&n, F.counts_host.host(), sizeof(n));
  F.any_filled = n.n_filled != 0;
  if (out) *out = n;
  return NID_OK;
}

}  // namespace

extern "C" {

int nid_pyr_fill_reference_depth(nid_pyr *p, const double *pose7, int guard, int guard_abs, int guard_rel_1024, int accumulate,
                                 nid_reffill_counts *out) {
  if (!p || !pose7 || !rf::args_ok(guard, guard_abs, guard_rel_1024)) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_fill_reference_depth";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  if (!p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_fill_reference_depth: the target has no depth: nid_pyr_set_target_depth_u16() first");
  nid_pyr::RefMask &R = p->rm;
  nid_pyr::RefMask::Fill &F = R.fill;
  const RefFillArgs A = rf_splat_args(p, pose7);
  if ((rc = rf_begin(p, what))) return rc;
  if ((rc = rf_splat(p, what, A))) return rc;
  const hipStream_t st = p->ctx[0]->stream;
  const Geometry &g = p->ctx[0]->g;
  hipLaunchKernelGGL(k_reffill_apply, dim3((unsigned)((g.cols + kRmTileW - 1) / kRmTileW), (unsigned)((g.rows + kRmTileH - 1) / kRmTileH)), dim3(256),
                     0, st, g.rows, g.cols, guard, guard_abs, guard_rel_1024, (int)(accumulate != 0), F.zbuf_dev.get(), rf_base(p),
                     R.ref_factor, F.fill_dev.get(), R.pristine_dev.get(), F.counts_dev.get());
  return rf_finish(p, what, out);
}

int nid_pyr_clear_reference_fill(nid_pyr *p) {
  if (!p) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_clear_reference_fill";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  nid_pyr::RefMask &R = p->rm;
  nid_pyr::RefMask::Fill &F = R.fill;
  if (!F.have_uploaded || !F.any_filled) return NID_OK;  // nothing is filled
  if ((rc = rf_begin(p, what))) return rc;
  const hipStream_t st = p->ctx[0]->stream;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  if (hipMemsetAsync(F.fill_dev, 0, 2 * N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(fill)");
  if (hipMemcpyAsync(R.pristine_dev, rf_base(p), 2 * N, hipMemcpyDeviceToDevice, st) != hipSuccess) return rf_failed(p, what, "hipMemcpyAsync(pristine)");
  return rf_finish(p, what, nullptr);
}

int nid_pyr_get_reference_fill_u16(nid_pyr *p, uint16_t *out) {
  if (!p || !out) return NID_ERR_INVALID_ARG;
  const int rc = rm_refuse(p, "nid_pyr_get_reference_fill_u16");
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  if (!p->rm.fill.have_uploaded) {  // a new reference starts unfilled
    std::memset(out, 0, 2 * N);
    return NID_OK;
  }
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  resident_retire(c0);
  NID_HIP(c0, hipMemcpyAsync(out, p->rm.fill.fill_dev, 2 * N, hipMemcpyDeviceToHost, c0->stream));
  NID_HIP(c0, hipStreamSynchronize(c0->stream));
  return NID_OK;
}

int nid_reffill_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *Twc, const uint16_t *depth1_u16,
                     double factor1, const double *pose7, int guard, int guard_abs, int guard_rel_1024, int accumulate, uint16_t *fill_inout,
                     nid_reffill_counts *counts) {
  if (!cfg || !depth0_u16 || !Twc || !depth1_u16 || !pose7 || !fill_inout || !rf::args_ok(guard, guard_abs, guard_rel_1024)) return NID_ERR_INVALID_ARG;
  if (cfg->rows < 1 || cfg->cols < 1 || (int64_t)cfg->rows * cfg->cols > INT32_MAX) return NID_ERR_INVALID_ARG;
  double M[12];
  rf::target_to_keyframe(Twc, pose7, M);
  const rf::Splat S = rf::make_splat(*cfg, M, depth1_u16, factor1, factor0);
  std::vector<uint32_t> zbuf;
  try {
    zbuf.resize((size_t)cfg->rows * (size_t)cfg->cols);
  } catch (const std::bad_alloc &) {
    return NID_ERR_NOMEM;
  }
  rf::reffill_host(S, depth0_u16, guard, guard_abs, guard_rel_1024, accumulate != 0, fill_inout, zbuf.data(), counts);
  return NID_OK;
}

int nid_track_set_filling(nid_track *t, int on, int guard, int guard_abs, int guard_rel_1024) {
  if (!t || !rf::args_ok(guard, guard_abs, guard_rel_1024)) return NID_ERR_INVALID_ARG;
  t->fill_on = on != 0;
  t->fill_guard = guard;
  t->fill_guard_abs = guard_abs;
  t->fill_guard_rel_1024 = guard_rel_1024;
  return NID_OK;
}

int nid_track_last_fill(const nid_track *t, nid_reffill_counts *counts) {
  if (!t || !counts) return NID_ERR_INVALID_ARG;
  *counts = t->last_fill;
  return NID_OK;
}

}  // extern "C"

// nid_reffuse.inc -- the reference's valid depth refined from tracked frames, and the tracker's use of it
// (include/nid/nid_reffuse.h).  Part of nid_capi.hip's translation unit (included behind nid_reffill.inc).
//
// A fusion call is a fill call (nid_reffill.inc's rf_begin ... rf_close) with another second kernel.  ru_begin: behind
// rf_begin -- which makes the uploaded copy and a zero fill plane if neither a fill nor a fusion came before -- zeros into S
// and k if this is the first fusion behind a new reference.  The
// call's own part: rf_splat (the z-buffer, k_reffill_splat) and k_reffuse_apply (S, k, fused, base, pristine = fill ? fill :
// base, the counts) -- or, for nid_pyr_clear_reference_fusion, zeros into S and k and the same kernel over a z-buffer
// nothing has hit, which makes fused 0, base = uploaded and pristine = fill ? fill : uploaded.  rf_close: the counts' way
// home, the mask plane as it is, the masking calls' chain and the call's one synchronisation.

namespace {

// the fusion's buffers, made before anything of the call changes the pyramid
int ru_ensure(nid_pyr *p) {
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask::Fuse &U = p->rm.fuse;
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  NID_HIP(c0, U.sum_dev.grow(N));
  NID_HIP(c0, U.obs_dev.grow(N));
  NID_HIP(c0, U.fused_dev.grow(N));
  NID_HIP(c0, U.base_dev.grow(N));
  return NID_OK;
}

// behind it the fusion's four planes belong to the reference, in stream order
int ru_begin(nid_pyr *p, const char *what) {
  int rc = ru_ensure(p);
  if (rc) return rc;
  if ((rc = rf_begin(p, what))) return rc;
  nid_pyr::RefMask::Fuse &U = p->rm.fuse;
  const hipStream_t st = p->ctx[0]->stream;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  if (!U.have_state) {
    if (hipMemsetAsync(U.sum_dev, 0, 4 * N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(sum)");
    if (hipMemsetAsync(U.obs_dev, 0, N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(obs)");
  }  // (the FUSED and the BASE plane are written whole by every call's k_reffuse_apply)
  return NID_OK;
}

// k_reffuse_apply over the z-buffer as it stands, then the close; the call's totals into *n
int ru_apply_finish(nid_pyr *p, const char *what, int gate_abs, int gate_rel_1024, int max_obs, nid_reffuse_counts *n) {
  nid_pyr::RefMask &R = p->rm;
  nid_pyr::RefMask::Fill &F = R.fill;
  nid_pyr::RefMask::Fuse &U = R.fuse;
  const long N = (long)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  hipLaunchKernelGGL(k_reffuse_apply, dim3((unsigned)((N + kRuSpan - 1) / kRuSpan)), dim3(256), 0, p->ctx[0]->stream, N, gate_abs, gate_rel_1024, max_obs,
                     F.zbuf_dev.get(), F.uploaded_dev.get(), R.ref_factor, F.fill_dev.get(), U.sum_dev.get(), U.obs_dev.get(), U.fused_dev.get(),
                     U.base_dev.get(), R.pristine_dev.get(), F.counts_dev.get());
  const int rc = rf_close(p, what);
  if (rc) return rc;
  static_assert(sizeof(nid_reffuse_counts) == 8 * sizeof(unsigned long long), "the totals are the record");
  std::memcpy(n, F.counts_host.host(), sizeof(*n));
  U.have_state = true;
  return NID_OK;
}

}  // namespace

extern "C" {

int nid_pyr_fuse_reference_depth(nid_pyr *p, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs, nid_reffuse_counts *out) {
  if (!p || !pose7 || !rfu::args_ok(gate_abs, gate_rel_1024, max_obs)) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_fuse_reference_depth";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  if (!p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_fuse_reference_depth: the target has no depth: nid_pyr_set_target_depth_u16() first");
  const RefFillArgs A = rf_splat_args(p, pose7);
  if ((rc = ru_begin(p, what))) return rc;
  if ((rc = rf_splat(p, what, A))) return rc;
  nid_reffuse_counts n;
  if ((rc = ru_apply_finish(p, what, gate_abs, gate_rel_1024, max_obs, &n))) return rc;
  p->rm.fuse.any_fused |= n.n_fused != 0;
  if (out) *out = n;
  return NID_OK;
}

int nid_pyr_clear_reference_fusion(nid_pyr *p) {
  if (!p) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_clear_reference_fusion";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  nid_pyr::RefMask::Fuse &U = p->rm.fuse;
  if (!U.have_state || !U.any_fused) return NID_OK;  // nothing is fused
  if ((rc = ru_begin(p, what))) return rc;
  const hipStream_t st = p->ctx[0]->stream;
  const size_t N = (size_t)p->ctx[0]->g.rows * p->ctx[0]->g.cols;
  if (hipMemsetAsync(U.sum_dev, 0, 4 * N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(sum)");
  if (hipMemsetAsync(U.obs_dev, 0, N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(obs)");
  if (hipMemsetAsync(p->rm.fill.zbuf_dev, 0xFF, 4 * N, st) != hipSuccess) return rf_failed(p, what, "hipMemsetAsync(zbuf)");
  nid_reffuse_counts n;
  if ((rc = ru_apply_finish(p, what, 0, 0, 1, &n))) return rc;  // (no pixel is hit: the gate and the cap decide nothing)
  U.any_fused = false;
  return NID_OK;
}

int nid_pyr_get_reference_fused_u16(nid_pyr *p, uint16_t *out) {
  if (!p || !out) return NID_ERR_INVALID_ARG;
  const int rc = rm_refuse(p, "nid_pyr_get_reference_fused_u16");
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  if (!p->rm.fuse.have_state) {  // a new reference starts unfused
    std::memset(out, 0, 2 * N);
    return NID_OK;
  }
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  resident_retire(c0);
  NID_HIP(c0, hipMemcpyAsync(out, p->rm.fuse.fused_dev, 2 * N, hipMemcpyDeviceToHost, c0->stream));
  NID_HIP(c0, hipStreamSynchronize(c0->stream));
  return NID_OK;
}

int nid_pyr_get_reference_fusion_obs_u8(nid_pyr *p, uint8_t *out) {
  if (!p || !out) return NID_ERR_INVALID_ARG;
  const int rc = rm_refuse(p, "nid_pyr_get_reference_fusion_obs_u8");
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  if (!p->rm.fuse.have_state) {
    std::memset(out, 0, N);
    return NID_OK;
  }
  NID_HIP(c0, hipSetDevice(c0->cfg.device));
  resident_retire(c0);
  NID_HIP(c0, hipMemcpyAsync(out, p->rm.fuse.obs_dev, N, hipMemcpyDeviceToHost, c0->stream));
  NID_HIP(c0, hipStreamSynchronize(c0->stream));
  return NID_OK;
}

int nid_reffuse_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *Twc, const uint16_t *depth1_u16,
                     double factor1, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs, uint32_t *sum_inout, uint8_t *obs_inout,
                     uint16_t *fused_out, nid_reffuse_counts *counts) {
  if (!cfg || !depth0_u16 || !Twc || !depth1_u16 || !pose7 || !sum_inout || !obs_inout || !fused_out || !rfu::args_ok(gate_abs, gate_rel_1024, max_obs))
    return NID_ERR_INVALID_ARG;
  if (cfg->rows < 1 || cfg->cols < 1 || (int64_t)cfg->rows * cfg->cols > INT32_MAX) return NID_ERR_INVALID_ARG;
  const size_t N = (size_t)cfg->rows * (size_t)cfg->cols;
  for (size_t i = 0; i < N; i++)
    if (!rfu::state_ok(sum_inout[i], obs_inout[i])) return NID_ERR_INVALID_ARG;
  double M[12];
  rf::target_to_keyframe(Twc, pose7, M);
  const rf::Splat S = rf::make_splat(*cfg, M, depth1_u16, factor1, factor0);
  std::vector<uint32_t> zbuf;
  try {
    zbuf.resize(N);
  } catch (const std::bad_alloc &) {
    return NID_ERR_NOMEM;
  }
  rfu::reffuse_host(S, depth0_u16, gate_abs, gate_rel_1024, max_obs, sum_inout, obs_inout, fused_out, nullptr, zbuf.data(), counts);
  return NID_OK;
}

int nid_track_set_fusing(nid_track *t, int on, int gate_abs, int gate_rel_1024, int max_obs) {
  if (!t || !rfu::args_ok(gate_abs, gate_rel_1024, max_obs)) return NID_ERR_INVALID_ARG;
  t->fuse_on = on != 0;
  t->fuse_gate_abs = gate_abs;
  t->fuse_gate_rel_1024 = gate_rel_1024;
  t->fuse_max_obs = max_obs;
  return NID_OK;
}

int nid_track_last_fusion(const nid_track *t, nid_reffuse_counts *counts) {
  if (!t || !counts) return NID_ERR_INVALID_ARG;
  *counts = t->last_fusion;
  return NID_OK;
}

}  // extern "C"

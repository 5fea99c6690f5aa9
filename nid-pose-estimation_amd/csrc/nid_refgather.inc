// nid_refgather.inc -- bilinear depth samples fused into the reference, and the tracker's use of them
// (include/nid/nid_refgather.h).  Part of nid_capi.hip's translation unit (included behind nid_reffuse.inc).
//
// A gather call is a fusion call (nid_reffuse.inc's ru_begin ... rf_close) with ONE kernel of its own in its middle:
// k_refgather_apply reads the target's depth where each keyframe pixel projects and writes S, k, fused, base, pristine =
// fill ? fill : base and the call's eight totals.  No splat is launched and the z-buffer is not filled.  The fusion's
// state is shared: have_state and any_fused are set as a fusion sets them, so nid_pyr_clear_reference_fusion and the two
// getters serve a gather unchanged.

extern "C" {

int nid_pyr_fuse_reference_depth_bilinear(nid_pyr *p, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs, int tap_abs,
                                          int tap_rel_1024, nid_refgather_counts *out) {
  if (!p || !pose7 || !rg::args_ok(gate_abs, gate_rel_1024, max_obs, tap_abs, tap_rel_1024)) return NID_ERR_INVALID_ARG;
  const char *what = "nid_pyr_fuse_reference_depth_bilinear";
  int rc = rm_refuse(p, what);
  if (rc) return rc;
  if (!p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_fuse_reference_depth_bilinear: the target has no depth: nid_pyr_set_target_depth_u16() first");
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::RefMask &R = p->rm;
  nid_pyr::RefMask::Fill &F = R.fill;
  nid_pyr::RefMask::Fuse &U = R.fuse;
  RefGatherArgs A = {};
  double Twc[16];  // the host's copy of the keyframe's matrix: where whatever made the reference staged it
  std::memcpy(Twc, c0->pair_stage + pair_stage_layout(c0->g).twc, sizeof(Twc));
  rf::keyframe_to_target(Twc, pose7, A.K);
  rf::target_to_keyframe(Twc, pose7, A.M);
  A.d1 = p->tdepth_dev;
  A.factor1 = p->tdepth_factor;
  A.factor0 = R.ref_factor;
  A.tap_abs = tap_abs;
  A.tap_rel_1024 = tap_rel_1024;
  if ((rc = ru_begin(p, what))) return rc;
  const Geometry &g = c0->g;
  const long N = (long)g.rows * g.cols;
  hipLaunchKernelGGL(k_refgather_apply, dim3((unsigned)((N + kRuSpan - 1) / kRuSpan)), dim3(256), 0, c0->stream, g, A, N, gate_abs, gate_rel_1024, max_obs,
                     F.uploaded_dev.get(), F.fill_dev.get(), U.sum_dev.get(), U.obs_dev.get(), U.fused_dev.get(), U.base_dev.get(),
                     R.pristine_dev.get(), F.counts_dev.get());
  if ((rc = rf_close(p, what))) return rc;
  static_assert(sizeof(nid_refgather_counts) == 8 * sizeof(unsigned long long), "the totals are the record");
  nid_refgather_counts n;
  std::memcpy(&n, F.counts_host.host(), sizeof(n));
  U.have_state = true;
  U.any_fused |= n.n_fused != 0;
  if (out) *out = n;
  return NID_OK;
}

int nid_refgather_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *Twc, const uint16_t *depth1_u16,
                       double factor1, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs, int tap_abs, int tap_rel_1024,
                       uint32_t *sum_inout, uint8_t *obs_inout, uint16_t *fused_out, nid_refgather_counts *counts) {
  if (!cfg || !depth0_u16 || !Twc || !depth1_u16 || !pose7 || !sum_inout || !obs_inout || !fused_out ||
      !rg::args_ok(gate_abs, gate_rel_1024, max_obs, tap_abs, tap_rel_1024))
    return NID_ERR_INVALID_ARG;
  if (cfg->rows < 1 || cfg->cols < 1 || (int64_t)cfg->rows * cfg->cols > INT32_MAX) return NID_ERR_INVALID_ARG;
  const size_t N = (size_t)cfg->rows * (size_t)cfg->cols;
  for (size_t i = 0; i < N; i++)
    if (!rfu::state_ok(sum_inout[i], obs_inout[i])) return NID_ERR_INVALID_ARG;
  double K[12], M[12];
  rf::keyframe_to_target(Twc, pose7, K);
  rf::target_to_keyframe(Twc, pose7, M);
  const rg::Gather A = rg::make_gather(*cfg, K, M, depth1_u16, factor1, factor0, tap_abs, tap_rel_1024);
  rg::refgather_host(A, depth0_u16, gate_abs, gate_rel_1024, max_obs, sum_inout, obs_inout, fused_out, nullptr, counts);
  return NID_OK;
}

int nid_track_set_fusion_sampling(nid_track *t, int mode, int tap_abs, int tap_rel_1024) {
  if (!t || (mode != NID_REFFUSE_NEAREST && mode != NID_REFFUSE_BILINEAR) || !rg::args_ok(0, 0, 1, tap_abs, tap_rel_1024)) return NID_ERR_INVALID_ARG;
  t->fuse_sampling = mode;
  t->fuse_tap_abs = tap_abs;
  t->fuse_tap_rel_1024 = tap_rel_1024;
  return NID_OK;
}

int nid_track_last_gather(const nid_track *t, nid_refgather_counts *counts) {
  if (!t || !counts) return NID_ERR_INVALID_ARG;
  *counts = t->last_gather;
  return NID_OK;
}

}  // extern "C"

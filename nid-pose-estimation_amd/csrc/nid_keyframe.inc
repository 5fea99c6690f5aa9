// nid_keyframe.inc -- the depth-consistency check on the resident pyramid and the tracker's keyframe policy
// (include/nid/nid_keyframe.h).  Part of nid_capi.hip's translation unit (included behind nid_pyr_stream.inc).
//
// The target's depth is a level-0 plane of the pyramid's own (nid_pyr::tdepth_dev).  nid_pyr_set_target_depth_u16 stands
// in nid_pyr.inc's frame over that part; nid_pyr_promote_target is nid_pyr_stream.inc's pyr_promote with the depth copied
// on the device.  nid_pyr_depth_check rewrites nothing -- the frame over no part -- and runs k_depth_check
// (nid_setup_kernels.hip.h) on level 0's tiles, on level 0's stream: the poses' matrices go up from the pyramid's pinned block in-stream -- one path for every n --, the per-pose
// totals are 64-bit integer atomics behind the workgroups' reductions and come home through the same block, the cell
// records only when asked for.  It launches no evaluation kernel, fills no SlotArgs and touches no slot.
// The tracker's part is the back half of a frame under an active policy: one check, two decisions (nid_depth_check.h).

namespace {

bool dc_tolerances_ok(double tol_abs, double tol_rel) { return dc::finite_nonneg(tol_abs) && dc::finite_nonneg(tol_rel); }

constexpr size_t kDcStageM = (size_t)kMaxBatchExt * 12, kDcStageTotals = (size_t)kMaxBatchExt * 8;  // 8-byte words of the pinned block

// the check's buffers, made on its first call (a hipMalloc waits for the whole device: never on a later one)
int dc_ensure(nid_pyr *p, size_t cells_host) {
  nid_ctx *c0 = p->ctx[0];
  nid_pyr::DepthCheck &D = p->dc;
  NID_HIP(c0, D.M_dev.grow(kDcStageM));
  NID_HIP(c0, D.totals_dev.grow(kDcStageTotals));
  NID_HIP(c0, D.cells_dev.grow((size_t)kMaxBatchExt * c0->g.nloc));
  NID_HIP(c0, D.stage.grow(kDcStageM + kDcStageTotals));
  if (cells_host) NID_HIP(c0, D.cells_host.grow(cells_host));
  return NID_OK;
}

int track_finish_with_policy(nid_track *t, int n, nid_track_result *R, nid_depth_counts *chosen, int32_t *n_checked) {
  nid_pyr *p = t->pyr;
  const int L = p->levels;
  const nid_track_policy &P = t->policy;
  const nid_ms_result *row = t->results.data() + (size_t)(L - 1) * n;  // level 0's chains
  const int32_t *org = t->origin.data() + (size_t)(L - 1) * n;
  // 5a. the candidates in rank order (the rule of nid_pyr_multistart_lm's survivors)
  std::vector<int> order;
  lm::rank_chains(row, n, order);
  // 5b. one check, over as many of them as the choice reads
  const int m = dc::candidates_to_check(P, (int)order.size());
  std::vector<double> poses(7 * (size_t)m);
  std::vector<nid_depth_counts> counts(m);
  for (int k = 0; k < m; k++) std::memcpy(poses.data() + 7 * (size_t)k, row[order[k]].pose7, 7 * sizeof(double));
  int rc = nid_pyr_depth_check(p, poses.data(), m, P.tol_abs, P.tol_rel, counts.data(), nullptr);
  if (rc) return rc;
  const int pick = dc::choose_candidate(P, counts.data(), m);
  R->best_origin = org[order[0]];
  if (pick < 0) {  // 5c.
    t->have_prev = false;
    R->status = NID_TRACK_REJECTED;
    *chosen = counts[0];
    *n_checked = m;
    return NID_OK;
  }
  // 5d.
  const nid_ms_result &best = row[order[pick]];
  if (dc::promote(P, counts[pick], t->age + 1)) {
    double Twc[16];
    track::pose_to_Twc16(best.pose7, Twc);
    if ((rc = nid_pyr_promote_target(p, Twc))) return rc;
    R->promoted = 1;
  } else {
    // (nid_reffill.h): the keyframe stays, with this frame's depth where it has none; the first fill of a pixel stays
    if (t->fill_on && (rc = nid_pyr_fill_reference_depth(p, best.pose7, t->fill_guard, t->fill_guard_abs, t->fill_guard_rel_1024, 1, &t->push_fill))) return rc;
    // (nid_reffuse.h): ... and this frame's depth averaged into the samples it has, where it passes their gate
    // (nid_refgather.h): ... from bilinear samples of it where the caller asked for them
    if (t->fuse_on && t->fuse_sampling == NID_REFFUSE_BILINEAR) {
      if ((rc = nid_pyr_fuse_reference_depth_bilinear(p, best.pose7, t->fuse_gate_abs, t->fuse_gate_rel_1024, t->fuse_max_obs, t->fuse_tap_abs,
                                                      t->fuse_tap_rel_1024, &t->push_gather)))
        return rc;
    } else if (t->fuse_on && (rc = nid_pyr_fuse_reference_depth(p, best.pose7, t->fuse_gate_abs, t->fuse_gate_rel_1024, t->fuse_max_obs, &t->push_fusion))) return rc;
    // 5e. (nid_refmask.h): ... without what this frame no longer sees of it
    if (t->mask_classes && (rc = nid_pyr_mask_occluded(p, best.pose7, P.tol_abs, P.tol_rel, t->mask_classes, t->mask_dilate, 0, &t->push_mask))) return rc;
  }
  R->best_origin = org[order[pick]];
  R->chi2 = best.chi2;
  R->n_active = best.n_active;
  std::memcpy(t->prev, t->cur, sizeof(t->cur));
  std::memcpy(t->cur, best.pose7, sizeof(t->cur));
  t->have_prev = true;
  R->status = NID_TRACK_OK;
  *chosen = counts[pick];
  *n_checked = m;
  return NID_OK;
}

}  // namespace

extern "C" {

int nid_pyr_set_target_depth_u16(nid_pyr *p, const uint16_t *depth_u16, double depth_factor) {
  if (!p || !depth_u16) return NID_ERR_INVALID_ARG;
  for (int l = 0; l < p->levels; l++)
    if (!p->ctx[l]->have_target) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_set_target_depth_u16: no target on level " + std::to_string(l));
  int rc = pyr_open(p, "nid_pyr_set_target_depth_u16", kPyrTdepth);
  if (rc) return rc;
  nid_ctx *c0 = p->ctx[0];
  if ((rc = pair_stage_ensure(c0))) return rc;  // (nothing enqueued yet)
  const PairStage L0 = pair_stage_layout(c0->g);
  const size_t N = (size_t)c0->g.rows * c0->g.cols;
  std::memcpy(c0->pair_stage + L0.depth, depth_u16, 2 * N);
  if (hipMemcpyAsync(p->tdepth_dev, c0->pair_stage + L0.depth, 2 * N, hipMemcpyHostToDevice, c0->stream) != hipSuccess)
    return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, "nid_pyr_set_target_depth_u16: hipMemcpyAsync(depth)"));
  if ((rc = pyr_close(p, "nid_pyr_set_target_depth_u16", kPyrTdepth))) return rc;
  p->tdepth_factor = depth_factor;
  return NID_OK;
}

int nid_pyr_promote_target(nid_pyr *p, const double *Twc) {
  if (!p || !Twc) return NID_ERR_INVALID_ARG;
  return pyr_promote(p, nullptr, p->tdepth_factor, Twc, "nid_pyr_promote_target");
}

int nid_pyr_depth_check(nid_pyr *p, const double *poses7, int n, double tol_abs, double tol_rel, nid_depth_counts *totals,
                        nid_depth_cell *cells) {
  if (!p || !poses7 || !totals || n < 1 || n > kMaxBatchExt || !dc_tolerances_ok(tol_abs, tol_rel)) return NID_ERR_INVALID_ARG;
  nid_ctx *c0 = p->ctx[0];
  if (!p->have_pair || !c0->have_ref) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_depth_check: no reference");
  if (!p->have_tdepth) return pyr_fail(p, NID_ERR_STATE, "nid_pyr_depth_check: the target has no depth: nid_pyr_set_target_depth_u16() first");
  int rc = pyr_open(p, "nid_pyr_depth_check", 0);  // (it rewrites nothing: no part's flags go down)
  if (rc) return rc;
  const Geometry &g = c0->g;
  const size_t ncell = (size_t)g.nloc, nrec = (size_t)n * ncell;
  if ((rc = dc_ensure(p, cells ? nrec : 0))) return rc;
  nid_pyr::DepthCheck &D = p->dc;
  const hipStream_t st = c0->stream;
  double *M_host = reinterpret_cast<double *>(D.stage.host());
  unsigned long long *totals_host = D.stage.host() + kDcStageM;
  for (int k = 0; k < n; k++) {
    double q7[7];
    int32_t mode;
    lm::pose_record(poses7 + 7 * (size_t)k, c0->xform, q7, M_host + 12 * (size_t)k, &mode);
  }
  auto failed = [&](const char *what) { return pyr_drain(p, pyr_fail(p, NID_ERR_HIP, std::string("nid_pyr_depth_check: ") + what)); };
  if (hipMemcpyAsync(D.M_dev, M_host, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) return failed("hipMemcpyAsync(poses)");
  if (hipMemsetAsync(D.totals_dev, 0, (size_t)n * 8 * sizeof(unsigned long long), st) != hipSuccess) return failed("hipMemsetAsync(totals)");
  DepthCheckArgs A;
  A.M = D.M_dev; A.d1 = p->tdepth_dev; A.factor = p->tdepth_factor; A.tol_abs = tol_abs; A.tol_rel = tol_rel;
  A.cells = D.cells_dev; A.totals = D.totals_dev;
  hipLaunchKernelGGL(k_depth_check, dim3((unsigned)nrec), dim3(256), 0, st, g, c0->t, A);
  if (hipGetLastError() != hipSuccess) return failed("the launch failed");
  if (hipMemcpyAsync(totals_host, D.totals_dev, (size_t)n * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st) != hipSuccess) return failed("hipMemcpyAsync(totals)");
  if (cells && hipMemcpyAsync(D.cells_host, D.cells_dev, nrec * sizeof(nid_depth_cell), hipMemcpyDeviceToHost, st) != hipSuccess) return failed("hipMemcpyAsync(cells)");
  if ((rc = pyr_close(p, "nid_pyr_depth_check", 0))) return rc;
  std::memcpy(totals, totals_host, (size_t)n * sizeof(nid_depth_counts));
  if (cells) {
    // the device's records are in the context's own cell order: cell cell_begin + cl * cell_stride (a pyramid owns all cells: cl itself)
    for (int k = 0; k < n; k++)
      for (size_t cl = 0; cl < ncell; cl++) cells[(size_t)k * ncell + (size_t)(g.cell_begin + (int)cl * g.cell_stride)] = D.cells_host[(size_t)k * ncell + cl];
  }
  return NID_OK;
}

int nid_depth_check_host(const nid_config *cfg, const double *points3d, const uint16_t *depth1_u16, double depth_factor,
                         const double *pose7, double tol_abs, double tol_rel, nid_depth_counts *total, nid_depth_cell *cells) {
  if (!cfg || !points3d || !depth1_u16 || !pose7 || (!total && !cells) || !dc_tolerances_ok(tol_abs, tol_rel)) return NID_ERR_INVALID_ARG;
  if (cfg->rows < 1 || cfg->cols < 1 || cfg->cell_num < 1 || cfg->cell_begin != 0 || cfg->cell_end != 0) return NID_ERR_INVALID_ARG;
  if ((int64_t)cfg->rows * cfg->cols > INT32_MAX) return NID_ERR_INVALID_ARG;
  double q7[7], M[12];
  int32_t mode;
  lm::pose_record(pose7, NID_XFORM_QUAT, q7, M, &mode);
  const dc::View V = dc::make_view(*cfg, M, depth1_u16, depth_factor, tol_abs, tol_rel);
  const int cn = cfg->cell_num, rb = cfg->rows / cn, cb = cfg->cols / cn;  // k_tile's cell map
  nid_depth_counts sum = {};
  for (int ci = 0; ci < cn; ci++)
    for (int cj = 0; cj < cn; cj++) {
      nid_depth_cell a = {};
      for (int r = ci * rb; r < (ci + 1) * rb; r++)
        for (int c = cj * cb; c < (cj + 1) * cb; c++) {
          const double *P = points3d + 3 * ((size_t)r * cfg->cols + c);
          dc::sample(V, P[0], P[1], P[2], &a);
        }
      if (cells) cells[(size_t)ci * cn + cj] = a;
      dc::add_cell(&sum, a);
    }
  if (total) *total = sum;
  return NID_OK;
}

int nid_track_policy_default(nid_track_policy *out) {
  if (!out) return NID_ERR_INVALID_ARG;
  *out = nid_track_policy();
  out->tol_abs = 0.01;
  out->tol_rel = 0.02;
  return NID_OK;
}

int nid_track_set_policy(nid_track *t, const nid_track_policy *policy) {
  if (!t || !policy || !dc::policy_valid(*policy)) return NID_ERR_INVALID_ARG;
  t->policy = *policy;
  return NID_OK;
}

int nid_track_last_check(const nid_track *t, nid_depth_counts *chosen, int32_t *n_checked, int32_t *age) {
  if (!t) return NID_ERR_INVALID_ARG;
  if (chosen) *chosen = t->chosen;
  if (n_checked) *n_checked = t->n_checked;
  if (age) *age = t->age;
  return NID_OK;
}

}  // extern "C"

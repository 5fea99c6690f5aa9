// lm_eval_stub.cpp -- everything host/g2o_min.cpp calls outward, answered without a GPU from ONE analytic per-cell
// model, so that the LM flows of g2o_min.cpp (fused 0..4 of nid_pose_problem) run on the CPU under a sanitizer
// (tests/test_lm_flows_cpu.py, tests/cpp/lm_flows_caller.cpp).
//
// The model: 3x3 cells, cell 2 inactive (Href NaN).  With z = (the antisymmetric part of R, t) of the pose -- zero at
// the identity, additive in the LM's update to first order -- and d = z - z*, every active cell c has a residual
//   e_c = gain * (a_c . d) + r_c + wall * (|z|^2)^2
// and answers  Hjoint = h_c + (|z|^2 / blow_r2)^1024,  Htarget = h_c * (2 - e_c) - Href,  so that the edge's
// (2 Hj - Href - Hc) / Hj is e_c up to rounding where the second term of Hjoint vanishes and NaN where it overflows;
// der_c = (der_scale + der_slope * z[3]) * a_c.  Polynomials only: no libm, the same bits everywhere.
// CudaComputeH hands these per-cell values out; the fused entry points form H, b, chi2 and n_active from the same
// values with the edge's own operations in edge order (computeError, robustify, constructQuadraticForm).
// An evaluation at a pose with |d|^2 < fail_r2 fails: the fused entry points return NID_ERR_HIP, CudaComputeH (void,
// "prints and carries on") leaves NaN in every cell.
// Every call is logged: which launches a flow issues is its speed.
#include "lm_eval_stub.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "g2o_min/g2o_min.h"
#include "nid/legacy_ops.h"
#include "nid/nid_multi.h"

struct nid_multi { int unused; };

namespace {

constexpr int kCellNum = 3, kCells = kCellNum * kCellNum, kInactive = 2, kSlots = 16;
const double kNaN = std::numeric_limits<double>::quiet_NaN();

struct Model {
  const char *name;
  double zstar[6];
  double gain;       // slope of the residuals in the pose; 0: the cost is flat
  double der_scale;  // 1: the Jacobian is the residuals' slope; < 1: Gauss-Newton overshoots; < 0: it points uphill
  double der_slope;  // the Jacobian's scale changes along z[3]
  double wall;       // a cost the Jacobian does not know about
  double blow_r2;    // > 0: Hjoint overflows where |z|^2 reaches about twice this (NaN chi2) ...
  bool blow_target;  // ... or Htarget does (infinite chi2)
  int rank;          // < 6: the cells' Jacobian rows are multiples of this many rows, H is singular
  double fail_r2;    // an evaluation fails where |z - z*|^2 is below this
};

#define ZSTAR {0.01, -0.02, 0.015, 0.05, -0.03, 0.04}
const Model kModels[] = {
    // name              zstar  gain scale slope  wall blow_r2 target rank fail_r2
    {"well_posed",       ZSTAR, 1.0, 1.0,  0.0,   0.0, 0.0,    false, 9,   0.0},   // first trials accepted, then three flat iterations
    {"overshoot",        ZSTAR, 1.0, 0.1,  0.0,   0.0, 0.0,    false, 9,   0.0},   // seven trials first, then one or two per iteration
    {"uphill",           ZSTAR, 1.0, -1.0, 0.0,   0.0, 0.0,    false, 9,   0.0},   // every trial rejected
    {"flat",             ZSTAR, 0.0, 1.0,  0.0,   0.0, 0.0,    false, 9,   0.0},   // rho == 0
    {"nan_cost",         ZSTAR, 1.0, 0.5,  0.0,   0.0, 0.008,  false, 9,   0.0},   // a NaN trial chi2 ends a chain
    {"inf_cost",         ZSTAR, 1.0, 0.1,  0.0,   0.0, 0.008,  true,  9,   0.0},   // an infinite one is rejected; long chains later on
    {"slope",            ZSTAR, 1.0, 1.0,  -19.8, 0.0, 0.0,    false, 9,   0.0},   // accepted at once, then ten rejections
    {"wall",             ZSTAR, 1.0, 1.0,  0.0,   1e4, 0.0,    false, 9,   0.0},
    // a singular H that grows by many orders of magnitude past the first step: lambda drowns in its rounding, LDLT fails
    {"ldlt_first_trial", ZSTAR, 1.0, 1.0,  1e8,   0.0, 0.0,    false, 2,   0.0},
    {"ldlt_later_trial", ZSTAR, 1.0, 1.0,  1e9,   0.0, 0.0,    false, 3,   0.0},
    {"ldlt_stale_step",  ZSTAR, 1.0, 1.0,  1e7,   0.0, 0.0,    false, 3,   0.0},   // where the flows differ in the x they keep
    {"fail_start",       ZSTAR, 1.0, 1.0,  0.0,   0.0, 0.0,    false, 9,   1.0},
    {"fail_trial",       ZSTAR, 1.0, 0.1,  0.0,   0.0, 0.0,    false, 9,   2e-3},
};
const Model *g_model = &kModels[0];
std::vector<std::string> g_log;
double g_last_pose[16];
bool g_have_last = false;

struct Cell { double Hc, Hj, der[6]; };

double row(int c, int i) { return ((c * 7 + i * 3 + c * i) % 11 - 5) * 0.25; }

// false: the evaluation fails
bool model(const double *M /* column-major 4x4 */, Cell cells[kCells], bool may_fail = true) {
  const Model &m = *g_model;
  const double z[6] = {(M[1 * 4 + 2] - M[2 * 4 + 1]) * 0.5, (M[2 * 4 + 0] - M[0 * 4 + 2]) * 0.5, (M[0 * 4 + 1] - M[1 * 4 + 0]) * 0.5,
                       M[12], M[13], M[14]};
  double d[6], s0 = 0, s = 0;
  for (int i = 0; i < 6; i++) { d[i] = z[i] - m.zstar[i]; s0 += z[i] * z[i]; s += d[i] * d[i]; }
  if (may_fail && s < m.fail_r2) return false;
  double blow = 0;
  if (m.blow_r2 > 0) {
    blow = s0 / m.blow_r2;
    for (int k = 0; k < 10; k++) blow *= blow;
  }
  const double k_der = m.der_scale + m.der_slope * z[3];
  for (int c = 0; c < kCells; c++) {
    Cell &o = cells[c];
    if (c == kInactive) {
      o.Hc = o.Hj = kNaN;
      for (int i = 0; i < 6; i++) o.der[i] = kNaN;
      continue;
    }
    const double h = 1.0 + 0.125 * c, r = ((c % 3) - 1) * 0.05;
    double lin = 0;
    const double mult = m.rank < 6 ? 1.0 + c / 3.0 : 1.0;
    for (int i = 0; i < 6; i++) lin += mult * row(c % m.rank, i) * d[i];
    const double e = m.gain * lin + r + m.wall * (s0 * s0);
    o.Hj = m.blow_target ? h : h + blow;
    o.Hc = h * (2.0 - e) - lm_stub_href(c) + (m.blow_target ? blow : 0.0);
    for (int i = 0; i < 6; i++) o.der[i] = k_der * (mult * row(c % m.rank, i));
  }
  return true;
}

const char *repeat_mark(const double *M) {  // the pose of the evaluation before this one, bit for bit: an LM step that did not move
  const bool same = g_have_last && std::memcmp(M, g_last_pose, sizeof(g_last_pose)) == 0;
  std::memcpy(g_last_pose, M, sizeof(g_last_pose));
  g_have_last = true;
  return same ? " same_pose" : "";
}

struct Reduced { int status; double H[36], b[6], chi2; int32_t n_active; };

// The whole image at one pose, the way the per-edge flow forms it (SparseOptimizer::computeActiveErrors,
// activeRobustChi2, BlockSolver_6_X::buildSystem), on edges of its own.
Reduced reduce(const double *pose7, bool want_jac, double huber_delta, const char **mark, bool may_fail = true) {
  Reduced r{};
  const g2o::Matrix4d M = g2o::SE3Quat::fromPose7(pose7).to_homogeneous_matrix();
  if (mark) *mark = repeat_mark(M.data());
  Cell cells[kCells];
  if (!model(M.data(), cells, may_fail)) { r.status = NID_ERR_HIP; return r; }
  g2o::VertexSE3Expmap v;
  v.clearQuadraticForm();
  g2o::EdgeSE3ProjectIntensityOnlyPoseNID edges[kCells];
  for (int c = 0; c < kCells; c++) {
    if (c == kInactive) continue;
    g2o::EdgeSE3ProjectIntensityOnlyPoseNID &e = edges[c];
    g2o::RobustKernelHuber *rk = new g2o::RobustKernelHuber;
    rk->setDelta(huber_delta);
    e.setRobustKernel(rk);
    e.setVertex(0, &v);
    e.setInformation(1.0);
    e.set_href(lm_stub_href(c));
    e.set_h(cells[c].Hc, cells[c].Hj);
    e.computeError();
    double rho[3];
    rk->robustify(e.chi2(), rho);
    r.chi2 += rho[0];
    r.n_active++;
  }
  if (want_jac)
    for (int c = 0; c < kCells; c++) {
      if (c == kInactive) continue;
      const double *j = cells[c].der;
      edges[c].set_j(j[0], j[1], j[2], j[3], j[4], j[5]);
      edges[c].linearizeOplus();
      edges[c].constructQuadraticForm();
    }
  std::memcpy(r.H, v.H, sizeof(r.H));
  std::memcpy(r.b, v.b, sizeof(r.b));
  return r;
}

Reduced g_slot[kSlots];
bool g_slot_jac[kSlots];

void log_line(const char *fmt, int a, int b, int c, const char *tail) {
  char buf[96];
  std::snprintf(buf, sizeof(buf), fmt, a, b, c);
  g_log.push_back(std::string(buf) + tail);
}

}  // namespace

int lm_stub_case_count() { return (int)(sizeof(kModels) / sizeof(kModels[0])); }
const char *lm_stub_select_case(int k) {
  g_model = &kModels[k];
  g_log.clear();
  g_have_last = false;
  return g_model->name;
}
int lm_stub_cell_num() { return kCellNum; }
double lm_stub_href(int cell) { return cell == kInactive ? kNaN : 0.5 + 0.0625 * cell; }
nid_multi *lm_stub_pair() { static nid_multi pair; return &pair; }
const std::vector<std::string> &lm_stub_call_log() { return g_log; }
void lm_stub_system(const double *pose7, double huber_delta, double *H36, double *b6) {
  const Reduced r = reduce(pose7, true, huber_delta, nullptr, false);
  std::memcpy(H36, r.H, sizeof(r.H));
  std::memcpy(b6, r.b, sizeof(r.b));
}

namespace g2o {
void CudaComputeH(bool calculate_der, double *, double *, double *, int *, double *, int *, double *pose, double *, int, int,
                  int cell_num, int, int, double *, double *, double *, double *Htarget, double *Hjoint, double *der) {
  const char *mark = repeat_mark(pose);
  Cell cells[kCells];
  const bool ok = cell_num == kCellNum && model(pose, cells);
  for (int c = 0; c < kCells; c++) {
    Htarget[c] = ok ? cells[c].Hc : kNaN;
    Hjoint[c] = ok ? cells[c].Hj : kNaN;
    if (calculate_der && der)
      for (int i = 0; i < 6; i++) der[6 * c + i] = ok ? cells[c].der[i] : kNaN;
  }
  log_line("CudaComputeH der=%d", calculate_der ? 1 : 0, 0, 0, (std::string(ok ? "" : " failed") + mark).c_str());
}
}  // namespace g2o

extern "C" {

nid_multi *nid_legacy_multi(void) {
  g_log.push_back("nid_legacy_multi");
  return nullptr;
}

nid_multi *nid_legacy_prepare(double *, double *, double *, int *, double *, int *, double *, int, int, int, int, int, double *) {
  g_log.push_back("nid_legacy_prepare");  // never reached: the fused flows run with native_pair_ set
  return nullptr;
}

int nid_multi_normal_equations(nid_multi *, const double *pose7, int want_jac, double huber_delta, double *H36, double *b6, double *chi2,
                               int32_t *n_active) {
  const char *mark = "";
  const Reduced r = reduce(pose7, want_jac != 0, huber_delta, &mark);
  std::string tail = mark;
  if (r.status != NID_OK) tail += " failed";
  else if (!std::isfinite(r.chi2)) tail += " nonfinite";
  log_line("normal_equations want_jac=%d", want_jac, 0, 0, tail.c_str());
  if (r.status != NID_OK) return r.status;
  if (H36) std::memcpy(H36, r.H, sizeof(r.H));
  if (b6) std::memcpy(b6, r.b, sizeof(r.b));
  if (chi2) *chi2 = r.chi2;
  if (n_active) *n_active = r.n_active;
  return NID_OK;
}

int nid_multi_launch_chain(nid_multi *, int first_slot, int n, const double *poses7, int n_jac, double huber_delta) {
  std::string tail;
  if (first_slot < 0 || n < 1 || first_slot + n > kSlots) return NID_ERR_INVALID_ARG;
  for (int k = 0; k < n; k++) {
    const char *mark = "";
    g_slot[first_slot + k] = reduce(poses7 + 7 * k, k < n_jac, huber_delta, &mark);
    g_slot_jac[first_slot + k] = k < n_jac;
    const Reduced &r = g_slot[first_slot + k];
    if (mark[0] || r.status != NID_OK || !std::isfinite(r.chi2)) {
      char buf[48];
      std::snprintf(buf, sizeof(buf), " [%d%s%s]", k, mark, r.status != NID_OK ? " failed" : !std::isfinite(r.chi2) ? " nonfinite" : "");
      tail += buf;
    }
  }
  log_line("launch_chain n=%d n_jac=%d slot=%d", n, n_jac, first_slot, tail.c_str());
  return NID_OK;
}

int nid_multi_wait(nid_multi *, int slot, double *H36, double *b6, double *chi2, int32_t *n_active) {
  if (slot < 0 || slot >= kSlots) return NID_ERR_INVALID_ARG;
  const Reduced &r = g_slot[slot];
  log_line("wait slot=%d jac=%d", slot, H36 ? 1 : 0, 0, r.status != NID_OK ? " failed" : "");
  if (r.status != NID_OK) return r.status;
  if (H36 && !g_slot_jac[slot]) return NID_ERR_STATE;
  if (H36) std::memcpy(H36, r.H, sizeof(r.H));
  if (b6) std::memcpy(b6, r.b, sizeof(r.b));
  if (chi2) *chi2 = r.chi2;
  if (n_active) *n_active = r.n_active;
  return NID_OK;
}

}  // extern "C"

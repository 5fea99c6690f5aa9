// nid_lm_step.h -- one step of one Levenberg-Marquardt chain: the ONE definition the device (k_lm_step in
// nid_multistart.inc) and the host (nid_lm_step_host) are compiled from.  See include/nid/nid_multistart.h for the rule.
//
// Bitwise agreement of the two compilations: everything here is IEEE + - * / sqrt and comparisons on doubles, integer
// arithmetic and selects.  No libm: the cube is y*y*y, sin / cos are written out below, the 6x6 LDLT is this file's.
// Both sides are compiled with -ffp-contract=off and without fast-math, so no operation is fused, reassociated or
// replaced.  No HIP-only construct: a plain C++ translation unit can include this file.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "nid/nid_multistart.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NID_LM_HD __host__ __device__ inline
#else
#define NID_LM_HD inline
#endif

namespace nid {
namespace lm {

constexpr double kDblMax = 1.7976931348623157e308;   // DBL_MAX
constexpr double kDblMin = 2.2250738585072014e-308;  // DBL_MIN
constexpr int kMaxTrials = 10;                       // _maxTrialsAfterFailure
constexpr double kTau = 1e-5, kGoodLower = 1. / 3., kGoodUpper = 2. / 3.;

NID_LM_HD double dabs(double v) { return v < 0 ? -v : v; }
NID_LM_HD bool finite(double v) { return dabs(v) <= kDblMax; }  // (false for NaN and the infinities)

// sin and cos of theta >= 0: Cody-Waite reduction by pi/2 in four pieces (the first three have 33 significant bits: their
// products with k < 2^20 are exact), then the classic degree-13 / degree-14 minimax polynomials on [-pi/4, pi/4].
// Within 4 ulp of sinl / cosl for theta <= 1e6 (the bound: three rounded subtractions in the reduction behind an exact
// first one, at most 1.5 ulp of r, plus the polynomial and the final sum); measured worst 2.35 ulp (cos, at
// 0x1.461c749ba6759p+19) and 2.28 ulp (sin) over 6 M random arguments, 1.00 ulp at the doubles next to k pi/2 for every
// k <= 636 619 (tests/cpp/lm_step_math_check.cpp, profiles/lm_step_edges.txt).  Beyond 1e6 (no LM step is a million
// radians) both are NaN, like for a NaN or an infinite argument.  THAT they are NaN is the same on both sides; the bits of
// a NaN that ARITHMETIC produced are not -- IEEE fixes neither its sign nor its payload, and x86 and gfx950 do differ: a
// generated one (0 / 0 here, inf - inf elsewhere) is 0xfff8000000000000 on x86 and 0x7ff8000000000000 on gfx950, and a NaN
// chi2 comes out of the subtraction in rho with its sign kept on x86 and turned on gfx950.  1642 fields of the 106 steps
// built to make NaNs in tests/lm_step_cases.py are NaN on both sides with other bits.  Everything else -- every number, and
// every NaN merely copied -- has the same bits on both sides, in every field of every step of that corpus, which reaches
// every branch of this file (tests/test_lm_step_gpu.py).
NID_LM_HD void sincos_pos(double theta, double *s, double *c) {
  if (!(theta <= 1.0e6)) {
    const double z = theta - theta;
    *s = *c = z / z;
    return;
  }
  constexpr double kInvPio2 = 0x1.45F306DC9C883p-1;
  constexpr double kP1 = 0x1.921FB54400000p+0, kP2 = 0x1.0B4611A600000p-34, kP3 = 0x1.3198A2E000000p-69, kP4 = 0x1.B839A252049C1p-104;
  constexpr double kRound = 0x1.8p52;  // adding and subtracting it rounds to the nearest integer
  const double kd = (theta * kInvPio2 + kRound) - kRound;
  double r = theta - kd * kP1;
  r = r - kd * kP2;
  r = r - kd * kP3;
  r = r - kd * kP4;
  const int quadrant = (int)kd & 3;
  const double z = r * r;
  constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                   S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                   C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double ps = S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6))));
  const double pc = C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6))));
  const double sr = r + (r * z) * ps;
  const double cr = (1.0 - 0.5 * z) + (z * z) * pc;
  switch (quadrant) {
    case 0: *s = sr; *c = cr; break;
    case 1: *s = cr; *c = -sr; break;
    case 2: *s = -sr; *c = -cr; break;
    default: *s = -cr; *c = sr; break;
  }
}

// (H + lambda I) x = b by an LDL^T with diagonal pivoting (the idea of LinearSolverDense::solve: the largest remaining
// |diagonal| next, "positive or fail").  H21: upper triangle row-major.  false -- and x untouched -- when a pivot is
// negative or NaN; a zero pivot gives a zero component.
NID_LM_HD bool ldlt6_solve(const double *H21, double lambda, const double *b, double *x) {
  enum { n = 6 };
  double A[n][n];
  {
    int k = 0;
    for (int i = 0; i < n; i++)
      for (int j = i; j < n; j++, k++) { A[i][j] = H21[k]; A[j][i] = H21[k]; }
    for (int i = 0; i < n; i++) A[i][i] = A[i][i] + lambda;
  }
  int perm[n];
  double y[n], d[n];
  for (int i = 0; i < n; i++) { perm[i] = i; y[i] = b[i]; }
  bool positive = true;
  for (int k = 0; k < n; k++) {
    int p = k;
    double best = dabs(A[k][k]);
    for (int i = k + 1; i < n; i++)
      if (dabs(A[i][i]) > best) { best = dabs(A[i][i]); p = i; }
    if (p != k) {  // symmetric exchange of rows and columns k and p (finished columns of L included), and of the right-hand side
      for (int j = 0; j < n; j++) { const double t = A[k][j]; A[k][j] = A[p][j]; A[p][j] = t; }
      for (int i = 0; i < n; i++) { const double t = A[i][k]; A[i][k] = A[i][p]; A[i][p] = t; }
      { const int t = perm[k]; perm[k] = perm[p]; perm[p] = t; }
      { const double t = y[k]; y[k] = y[p]; y[p] = t; }
    }
    const double dk = A[k][k];
    d[k] = dk;
    if (!(dk >= 0)) positive = false;
    const bool usable = dabs(dk) > kDblMin;
    for (int i = k + 1; i < n; i++) A[i][k] = usable ? A[i][k] / dk : 0.0;  // L(i, k)
    for (int i = k + 1; i < n; i++)
      for (int j = k + 1; j < n; j++) A[i][j] = A[i][j] - (A[i][k] * dk) * A[j][k];
  }
  if (!positive) return false;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < i; j++) y[i] = y[i] - A[i][j] * y[j];
  for (int i = 0; i < n; i++) y[i] = dabs(d[i]) > kDblMin ? y[i] / d[i] : 0.0;
  for (int i = n - 1; i >= 0; i--)
    for (int j = i + 1; j < n; j++) y[i] = y[i] - A[j][i] * y[j];
  for (int i = 0; i < n; i++) x[perm[i]] = y[i];
  return true;
}

// SE3Quat::normalizeRotation (se3quat.h:280-285) on q = {x, y, z, w}
NID_LM_HD void normalize_rotation(double *q) {
  if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double nrm = __builtin_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] = q[0] / nrm; q[1] = q[1] / nrm; q[2] = q[2] / nrm; q[3] = q[3] / nrm;
}

// SE3Quat::exp (se3quat.h:223-257): update = (omega, upsilon) -> pose7 {qx, qy, qz, qw, tx, ty, tz}
NID_LM_HD void se3_exp(const double *u, double *out7) {
  const double o0 = u[0], o1 = u[1], o2 = u[2];
  const double theta = __builtin_sqrt(o0 * o0 + o1 * o1 + o2 * o2);
  double Om[9] = {0, -o2, o1, o2, 0, -o0, -o1, o0, 0}, Om2[9], R[9], V[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s = s + Om[i * 3 + k] * Om[k * 3 + j];
      Om2[i * 3 + j] = s;
    }
  if (theta < 0.00001) {
    for (int i = 0; i < 9; i++) { const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0; R[i] = id + Om[i] + Om2[i]; V[i] = R[i]; }
  } else {
    double sn, cs;
    sincos_pos(theta, &sn, &cs);
    const double a = sn / theta;
    const double b = (1 - cs) / (theta * theta);
    const double c = (theta - sn) / (theta * theta * theta);
    for (int i = 0; i < 9; i++) {
      const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
      R[i] = id + a * Om[i] + b * Om2[i];
      V[i] = id + b * Om[i] + c * Om2[i];
    }
  }
  // Quaterniond(R): Eigen's quaternion from a rotation matrix
  double q[4];
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = __builtin_sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[2 * 3 + 1] - R[1 * 3 + 2]) * t;
    q[1] = (R[0 * 3 + 2] - R[2 * 3 + 0]) * t;
    q[2] = (R[1 * 3 + 0] - R[0 * 3 + 1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = __builtin_sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
  normalize_rotation(q);
  out7[0] = q[0]; out7[1] = q[1]; out7[2] = q[2]; out7[3] = q[3];
  for (int i = 0; i < 3; i++) out7[4 + i] = V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5];
}

// SE3Quat::operator* (se3quat.h:106-112): out = a * b
NID_LM_HD void se3_mul(const double *a, const double *b, double *out7) {
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
  // a's rotation applied to b's translation (Eigen QuaternionBase::_transformVector)
  const double v0 = b[4], v1 = b[5], v2 = b[6];
  double uvx = ay * v2 - az * v1, uvy = az * v0 - ax * v2, uvz = ax * v1 - ay * v0;
  uvx = uvx + uvx; uvy = uvy + uvy; uvz = uvz + uvz;
  const double cx = ay * uvz - az * uvy, cy = az * uvx - ax * uvz, cz = ax * uvy - ay * uvx;
  const double r0 = v0 + aw * uvx + cx, r1 = v1 + aw * uvy + cy, r2 = v2 + aw * uvz + cz;
  const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
  double q[4];
  q[3] = aw * bw - ax * bx - ay * by - az * bz;
  q[0] = aw * bx + ax * bw + ay * bz - az * by;
  q[1] = aw * by + ay * bw + az * bx - ax * bz;
  q[2] = aw * bz + az * bw + ax * by - ay * bx;
  normalize_rotation(q);
  out7[0] = q[0]; out7[1] = q[1]; out7[2] = q[2]; out7[3] = q[3];
  out7[4] = a[4] + r0; out7[5] = a[5] + r1; out7[6] = a[6] + r2;
}

// The pose record the evaluation kernels read (Pose in nid_kernels.hip.h: q[7], M[12], mode) for a pose7: what the
// host's pose_from_pose7 uploads (to_homogeneous_matrix, se3quat.h:270-278 = Eigen toRotationMatrix).
NID_LM_HD void pose_record(const double *p, int mode, double *q7, double *M, int32_t *mode_out) {
  for (int i = 0; i < 7; i++) q7[i] = p[i];
  const double x = p[0], y = p[1], z = p[2], w = p[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  M[0] = 1 - (tyy + tzz); M[1] = txy - twz;       M[2] = txz + twy;        M[3] = p[4];
  M[4] = txy + twz;       M[5] = 1 - (txx + tzz); M[6] = tyz - twx;        M[7] = p[5];
  M[8] = txz - twy;       M[9] = tyz + twx;       M[10] = 1 - (txx + tyy); M[11] = p[6];
  *mode_out = mode;
}

// One step of chain S with the reduced block r ([0] chi2, [1..6] b, [7..27] H upper, [28] n_active) of the pose it
// asked for.  Returns true while the chain is running.
NID_LM_HD bool lm_step(nid_ms_state *S, const double *r) {
  if (S->status != NID_MS_RUNNING) return false;  // frozen
  int flags = 0;
  auto adopt = [&]() {
    for (int i = 0; i < 6; i++) S->b[i] = r[1 + i];
    for (int i = 0; i < 21; i++) S->H[i] = r[7 + i];
    S->n_active = (int32_t)r[28];
  };
  S->trial_chi2 = r[0];
  if (!S->started) {
    S->started = 1;
    flags = NID_MS_F_FIRST;
    adopt();
    S->chi2 = r[0];
    double maxd = 0.;  // computeLambdaInit: tau * max |H_jj|
    for (int j = 0, k = 0; j < 6; k += 6 - j, j++) { const double a = dabs(S->H[k]); maxd = a > maxd ? a : maxd; }
    S->lambda = kTau * maxd;
    S->ni = 2;
    S->n_bad = 0;
    S->trials = 0;
    S->ini_chi2 = S->chi2;
    S->rho = 0;
    for (int j = 0; j < 6; j++) S->x[j] = 0;
  } else {
    const double trial = r[0];
    const double temp = S->solve_ok ? trial : kDblMax;
    double scale = 0.;
    for (int j = 0; j < 6; j++) scale = scale + S->x[j] * (S->lambda * S->x[j] + S->b[j]);
    scale = scale + 1e-3;
    const double rho = (S->chi2 - temp) / scale;
    S->rho = rho;
    S->trials++;
    S->trials_total++;
    double rule_chi2 = S->chi2;  // what the nBad rule compares with (the sequential loop's currentChi)
    const bool accept = rho > 0 && finite(temp);
    if (accept) {
      flags |= NID_MS_F_ACCEPT;
      const double y = 2 * rho - 1;
      double alpha = 1. - y * y * y;
      alpha = alpha < kGoodUpper ? alpha : kGoodUpper;
      const double factor = kGoodLower > alpha ? kGoodLower : alpha;
      S->lambda = S->lambda * factor;
      S->ni = 2;
      for (int i = 0; i < 7; i++) S->pose7[i] = S->trial7[i];
      adopt();
      rule_chi2 = temp;
      S->chi2 = trial;  // (the next outer iteration's evaluation of this pose)
    } else {
      flags |= NID_MS_F_REJECT;
      S->lambda = S->lambda * S->ni;
      S->ni = S->ni * 2;
    }
    if (accept || !(rho < 0) || S->trials >= kMaxTrials) {
      flags |= NID_MS_F_OUTER_END;
      S->outer_done++;
      if (S->trials >= kMaxTrials) S->status = NID_MS_TRIALS_EXHAUSTED;
      else if (rho == 0) S->status = NID_MS_RHO_NOT_NEGATIVE;
      else {
        if ((S->ini_chi2 - rule_chi2) * 1e3 < S->ini_chi2) S->n_bad++;
        else S->n_bad = 0;
        if (S->n_bad >= 3) S->status = NID_MS_NBAD;
        else if (S->outer_done >= S->iterations) S->status = NID_MS_ITERATIONS;
      }
      S->ini_chi2 = S->chi2;
      S->trials = 0;
    }
  }
  if (S->status == NID_MS_RUNNING) {
    const bool ok = ldlt6_solve(S->H, S->lambda, S->b, S->x);
    S->solve_ok = ok ? 1 : 0;
    if (!ok) flags |= NID_MS_F_SOLVE_FAILED;
    double e7[7];
    se3_exp(S->x, e7);
    se3_mul(e7, S->pose7, S->trial7);
    pose_record(S->trial7, S->xform_mode, S->rec_q, S->rec_M, &S->rec_mode);
  } else {
    flags |= NID_MS_F_FINISHED;
  }
  S->flags = flags;
  return S->status == NID_MS_RUNNING;
}

// a fresh chain from its start pose (what nid_multistart_lm does for every chain; the start pose's record)
NID_LM_HD void lm_init(nid_ms_state *S, const double *pose7, int iterations, int xform_mode) {
  *S = nid_ms_state();
  for (int i = 0; i < 7; i++) { S->pose7[i] = pose7[i]; S->trial7[i] = pose7[i]; }
  S->iterations = iterations;
  S->xform_mode = xform_mode;
  pose_record(pose7, xform_mode, S->rec_q, S->rec_M, &S->rec_mode);
}

NID_LM_HD void lm_trace(const nid_ms_state *S, nid_ms_trace *T) {
  T->trial_chi2 = S->trial_chi2;
  T->lambda = S->lambda;
  T->rho = S->rho;
  for (int i = 0; i < 7; i++) T->pose7[i] = S->pose7[i];
  T->flags = S->flags;
  T->status = S->status;
}

// THE RANK RULE of a batch of finished chains (host only): the eligible ones -- n_active > 0 and a finite chi2 -- by
// chi2 / n_active ascending, the lower index winning ties.  order[0] is nid_multistart_lm's *best; nid_pyr_multistart_lm's
// survivors and the tracker's candidates (nid_keyframe.h, step 5a) are its front.
inline void rank_chains(const nid_ms_result *res, int m, std::vector<int> &order) {
  order.clear();
  for (int k = 0; k < m; k++)
    if (res[k].n_active > 0 && finite(res[k].chi2)) order.push_back(k);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return res[a].chi2 / (double)res[a].n_active < res[b].chi2 / (double)res[b].n_active;
  });
}

}  // namespace lm
}  // namespace nid

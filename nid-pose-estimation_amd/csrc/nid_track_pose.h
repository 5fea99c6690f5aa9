// nid_track_pose.h -- the pose arithmetic of a frame sequence (include/nid/nid_pyr_stream.h): inverse, composition, the
// LM chains' update exp(twist) o pose, and the world -> camera pose7 <-> camera -> world matrix pair.  No HIP in it: a
// plain C++ translation unit can include this file alone (tests/cpp/track_pose_check.cpp does).
//
// Everything goes through nid_lm_step.h's SE(3) text -- se3_exp, se3_mul, normalize_rotation, pose_record: there is ONE
// exponential and ONE product in the library --, so it is IEEE + - * / sqrt only and, compiled without contraction like
// the step itself, gives the bits the chains' own updates give.  Every output quaternion is unit with w >= 0.
#pragma once

#include "nid_lm_step.h"

namespace nid {
namespace track {

// inverse: rotation conj(q), translation -(conj(q) t) -- as the product {conj(q), 0} o {identity, -t}
inline void pose_inverse(const double *p, double *out7) {
  const double a[7] = {-p[0], -p[1], -p[2], p[3], 0.0, 0.0, 0.0};
  const double b[7] = {0.0, 0.0, 0.0, 1.0, -p[4], -p[5], -p[6]};
  lm::se3_mul(a, b, out7);
}

// a o b (b applied first)
inline void pose_compose(const double *a, const double *b, double *out7) {
  double o[7];
  lm::se3_mul(a, b, o);
  for (int i = 0; i < 7; i++) out7[i] = o[i];
}

// exp(twist) o pose, twist = (omega, upsilon): the last three lines of lm_step()
inline void pose_perturb(const double *p, const double *twist6, double *out7) {
  double e7[7], o[7];
  lm::se3_exp(twist6, e7);
  lm::se3_mul(e7, p, o);
  for (int i = 0; i < 7; i++) out7[i] = o[i];
}

// world -> camera pose7 -> column-major 4x4 camera -> world
inline void pose_to_Twc16(const double *pose_cw, double *T16) {
  double inv[7], q7[7], M[12];
  int32_t mode;
  pose_inverse(pose_cw, inv);
  lm::pose_record(inv, 0, q7, M, &mode);  // M: 3x4 row-major
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 4; c++) T16[4 * c + r] = M[4 * r + c];
  T16[3] = 0.0; T16[7] = 0.0; T16[11] = 0.0; T16[15] = 1.0;
}

// column-major 4x4 camera -> world -> world -> camera pose7: R_cw = R_wc^T, t_cw = -(R_wc^T t_wc); the quaternion of
// R_cw by Eigen's Quaterniond(R), the branch se3_exp takes for its own rotation
inline void pose_from_Twc16(const double *T16, double *pose_cw) {
  double R[9];  // R_cw row-major: R[i * 3 + j] = R_wc(j, i) = T16[4 * i + j]
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = T16[4 * i + j];
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
  lm::normalize_rotation(q);
  pose_cw[0] = q[0]; pose_cw[1] = q[1]; pose_cw[2] = q[2]; pose_cw[3] = q[3];
  for (int i = 0; i < 3; i++) pose_cw[4 + i] = 0.0 - (R[i * 3] * T16[12] + R[i * 3 + 1] * T16[13] + R[i * 3 + 2] * T16[14]);
}

}  // namespace track
}  // namespace nid

// nid_reffill_rule.h -- the rule of the reference fill (include/nid/nid_reffill.h) on the terms of nid_depth_check.h, its
// sibling: the ONE definition the device (k_reffill_splat / k_reffill_apply in nid_setup_kernels.hip.h) and the host
// (rf::reffill_host behind nid_reffill_host) are compiled from -- a target pixel's way into the keyframe's z-buffer, the
// surface a keyframe pixel shows, the guard's comparison, a pixel's fill and its counts -- and the one helper that makes
// the matrix both sides read.
//
// Bitwise agreement of the two compilations: IEEE + - * / on doubles, comparisons, floor and integer arithmetic; both
// sides are compiled with -ffp-contract=off and without fast-math.  Every result is an integer and the z-buffer keeps a
// minimum, so neither the order of the pixels nor how they are spread over lanes shows.  No HIP-only construct: a plain
// C++ translation unit can include this file (tests/cpp/reffill_check.cpp, under the host sanitizers: no conversion or
// index here is reachable out of range).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "nid/nid_reffill.h"
#include "nid_depth_check.h"
#include "nid_track_pose.h"

namespace nid {
namespace rf {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // a z-buffer entry nothing has hit; a pixel that shows no surface

// what one call's target pixels share
struct Splat {
  double M[12];  // rows of [R|t], target camera -> keyframe camera (target_to_keyframe)
  double fx, fy, cx, cy;
  int rows, cols;
  const uint16_t *d1;  // the target's depth, rows x cols
  double factor1, factor0;
};

// the Splat of a call's matrix M, an image geometry g (Geometry on the device, nid_config on the host) and its arguments
template <class G>
NID_DC_HD Splat make_splat(const G &g, const double *M, const uint16_t *d1, double factor1, double factor0) {
  Splat S;
  for (int k = 0; k < 12; k++) S.M[k] = M[k];
  S.fx = g.fx; S.fy = g.fy; S.cx = g.cx; S.cy = g.cy;
  S.rows = g.rows; S.cols = g.cols;
  S.d1 = d1; S.factor1 = factor1; S.factor0 = factor0;
  return S;
}

// M: x_k = T_cw(keyframe) T_wc(target) x_t from the keyframe's column-major camera -> world matrix and the target's
// world -> camera pose7.  Host only, once per call: the device call and the host twin read the same twelve doubles.
inline void target_to_keyframe(const double *Twc16, const double *pose7, double *M) {
  double kf[7], inv[7], rel[7], q7[7];
  int32_t mode;
  track::pose_from_Twc16(Twc16, kf);
  track::pose_inverse(pose7, inv);
  track::pose_compose(kf, inv, rel);
  lm::pose_record(rel, 0, q7, M, &mode);
}

// K: the composition the other way round, x_t = T_cw(target) T_wc(keyframe) x_k (nid_refgather_rule.h projects the
// keyframe's pixels with it).  Host only, once per call, on the same terms.
inline void keyframe_to_target(const double *Twc16, const double *pose7, double *K) {
  double kf[7], inv[7], rel[7], q7[7];
  int32_t mode;
  track::pose_from_Twc16(Twc16, kf);
  track::pose_inverse(kf, inv);
  track::pose_compose(pose7, inv, rel);
  lm::pose_record(rel, 0, q7, K, &mode);
}

// Part A for target pixel (r1, c1).  0: its depth is not valid; 1: valid, and it ends before the z-buffer; 2: a splat of
// count *q onto keyframe pixel *idx (row-major, inside the image).
NID_DC_HD int splat(const Splat &S, int r1, int c1, size_t *idx, uint32_t *q) {
  const double zt = (double)S.d1[(size_t)r1 * (size_t)S.cols + (size_t)c1] * S.factor1;  // 1.
  if (zt < 0.01 || zt > 100) return 0;
  const double x = zt * (c1 - S.cx) / S.fx;  // 2. (dc::backproject's operations in its order)
  const double y = zt * (r1 - S.cy) / S.fy;
  const double *M = S.M;
  const double xk = ((M[0] * x + M[1] * y) + M[2] * zt) + M[3];  // 3. (summed as dc::classify sums)
  const double yk = ((M[4] * x + M[5] * y) + M[6] * zt) + M[7];
  const double zk = ((M[8] * x + M[9] * y) + M[10] * zt) + M[11];
  if (!(zk > 0)) return 1;
  const double u = (S.fx * xk) / zk + S.cx;  // 4.
  const double v = (S.fy * yk) / zk + S.cy;
  const double c = __builtin_floor(u + 0.5), r = __builtin_floor(v + 0.5);
  if (!(c >= 0 && c <= (double)(S.cols - 1) && r >= 0 && r <= (double)(S.rows - 1))) return 1;  // (NaN and the infinities fail)
  const double qd = __builtin_floor(zk / S.factor0 + 0.5);  // 5.
  if (!(qd >= 1 && qd <= 65535)) return 1;
  const uint32_t qi = (uint32_t)qd;  // (in range: decided above)
  if (!dc::depth_valid((uint16_t)qi, S.factor0)) return 1;
  *idx = (size_t)(int)r * (size_t)S.cols + (size_t)(int)c;  // (in range: decided in step 4)
  *q = qi;
  return 2;
}

// Part B.  S(p): the z-buffer's entry if p was hit, else the uploaded count if it is valid, else none
NID_DC_HD uint32_t surface(uint32_t z, uint16_t uploaded, double factor0) {
  return z != kNone ? z : (dc::depth_valid(uploaded, factor0) ? (uint32_t)uploaded : kNone);
}

// a hit of count q lies behind a neighbour's surface qn (64-bit integers: in metres the comparison lands on its threshold)
NID_DC_HD bool behind(uint32_t q, uint32_t qn, int guard_abs, int guard_rel_1024) {
  return ((int64_t)q - (int64_t)qn) * 1024 > (int64_t)guard_abs * 1024 + (int64_t)guard_rel_1024 * (int64_t)qn;
}

// the pixels whose fill the guard decides: a hole without a kept fill that was hit
NID_DC_HD bool guard_decides(bool uploaded_valid, uint16_t old, bool hit, int accumulate) {
  return !uploaded_valid && !(accumulate && old) && hit;
}

// Part C for one keyframe pixel, counted: its fill from the fill before it (`refused` is read where guard_decides)
NID_DC_HD uint16_t apply(bool uploaded_valid, uint16_t old, uint32_t z, bool refused, int accumulate, nid_reffill_counts *n) {
  const bool hit = z != kNone;
  uint16_t f = 0;
  n->n_hit += hit;
  if (!uploaded_valid) {
    n->n_holes++;
    if (accumulate && old) f = old;  // the first fill wins
    else if (hit) {
      if (refused) n->n_refused++;
      else f = (uint16_t)z;  // (a z-buffer entry is a count of step 5: 1 ... 65535)
    }
  }
  n->n_new += old == 0 && f != 0;
  n->n_filled += f != 0;
  return f;
}

NID_DC_HD bool args_ok(int guard, int guard_abs, int guard_rel_1024) {
  return guard >= 0 && guard <= NID_REFFILL_MAX_GUARD && guard_abs >= 0 && guard_abs <= 65535 && guard_rel_1024 >= 0 && guard_rel_1024 <= 1024;
}

// Part A over the whole target on the host (the fill's and, in nid_reffuse_rule.h, the fusion's): zbuf, rows x cols words of
// the caller's, overwritten; the part's two counts
inline void splat_host(const Splat &S, uint32_t *zbuf, int64_t *n_target_valid, int64_t *n_splat) {
  const int rows = S.rows, cols = S.cols;
  const size_t N = (size_t)rows * (size_t)cols;
  int64_t valid = 0, splats = 0;
  for (size_t i = 0; i < N; i++) zbuf[i] = kNone;
  for (int r1 = 0; r1 < rows; r1++)
    for (int c1 = 0; c1 < cols; c1++) {
      size_t idx = 0;
      uint32_t q = 0;
      const int k = splat(S, r1, c1, &idx, &q);
      valid += k >= 1;
      if (k != 2) continue;
      splats++;
      if (q < zbuf[idx]) zbuf[idx] = q;  // 6.
    }
  *n_target_valid = valid;
  *n_splat = splats;
}

// nid_reffill_host behind its argument checks: THE RULE over the whole plane, in place.  d0: the keyframe's uploaded depth;
// zbuf: rows x cols words of the caller's, overwritten.
inline void reffill_host(const Splat &S, const uint16_t *d0, int guard, int guard_abs, int guard_rel_1024, int accumulate, uint16_t *fill,
                         uint32_t *zbuf, nid_reffill_counts *counts) {
  const int rows = S.rows, cols = S.cols;
  nid_reffill_counts n = {};
  splat_host(S, zbuf, &n.n_target_valid, &n.n_splat);
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) {
      const size_t i = (size_t)r * (size_t)cols + (size_t)c;
      const bool valid = dc::depth_valid(d0[i], S.factor0);
      bool refused = false;
      if (guard > 0 && guard_decides(valid, fill[i], zbuf[i] != kNone, accumulate)) {
        const int r0 = r - guard < 0 ? 0 : r - guard, r1 = r + guard > rows - 1 ? rows - 1 : r + guard;
        const int c0 = c - guard < 0 ? 0 : c - guard, c1 = c + guard > cols - 1 ? cols - 1 : c + guard;
        for (int rr = r0; rr <= r1 && !refused; rr++)
          for (int cc = c0; cc <= c1; cc++) {
            if (rr == r && cc == c) continue;
            const size_t j = (size_t)rr * (size_t)cols + (size_t)cc;
            const uint32_t qn = surface(zbuf[j], d0[j], S.factor0);
            if (qn != kNone && behind(zbuf[i], qn, guard_abs, guard_rel_1024)) { refused = true; break; }
          }
      }
      fill[i] = apply(valid, fill[i], zbuf[i], refused, accumulate, &n);
    }
  if (counts) *counts = n;
}

}  // namespace rf
}  // namespace nid

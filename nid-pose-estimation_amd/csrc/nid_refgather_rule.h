// nid_refgather_rule.h -- the rule of the bilinear gather (include/nid/nid_refgather.h) on the terms of nid_reffill_rule.h
// and nid_reffuse_rule.h, which it includes and reuses (rf::target_to_keyframe, rf::keyframe_to_target, dc::depth_valid,
// rfu::fuse as it is): the ONE definition the device (k_refgather_apply in nid_setup_kernels.hip.h) and the host
// (rg::refgather_host behind nid_refgather_host) are compiled from -- a keyframe pixel's way into the target, the four taps
// and their gate, the interpolated depth's way back, and the pixel's counts.
//
// Bitwise agreement of the two compilations: IEEE + - * / on doubles, comparisons, floor and integer arithmetic; both
// sides are compiled with -ffp-contract=off and without fast-math.  A pixel reads the target's depth and its own entries
// alone, so neither the order of the pixels nor how they are spread over lanes shows.  No HIP-only construct: a plain C++
// translation unit can include this file (tests/cpp/refgather_check.cpp, under the host sanitizers: no conversion or
// index here is reachable out of range).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "nid/nid_refgather.h"
#include "nid_reffill_rule.h"
#include "nid_reffuse_rule.h"

namespace nid {
namespace rg {

// what one call's keyframe pixels share
struct Gather {
  double K[12];  // rows of [R|t], keyframe camera -> target camera (rf::keyframe_to_target)
  double M[12];  // rows of [R|t], target camera -> keyframe camera (rf::target_to_keyframe)
  double fx, fy, cx, cy;
  int rows, cols;
  const uint16_t *d1;  // the target's depth, rows x cols
  double factor1, factor0;
  int tap_abs, tap_rel_1024;
};

// the Gather of a call's matrices, an image geometry g (Geometry on the device, nid_config on the host) and its arguments
template <class G>
NID_DC_HD Gather make_gather(const G &g, const double *K, const double *M, const uint16_t *d1, double factor1, double factor0, int tap_abs,
                             int tap_rel_1024) {
  Gather A;
  for (int k = 0; k < 12; k++) {
    A.K[k] = K[k];
    A.M[k] = M[k];
  }
  A.fx = g.fx; A.fy = g.fy; A.cx = g.cx; A.cy = g.cy;
  A.rows = g.rows; A.cols = g.cols;
  A.d1 = d1; A.factor1 = factor1; A.factor0 = factor0;
  A.tap_abs = tap_abs; A.tap_rel_1024 = tap_rel_1024;
  return A;
}

// the four taps lie within the tap gate of the smallest of them (64-bit integers)
NID_DC_HD bool taps_within(uint16_t t00, uint16_t t01, uint16_t t10, uint16_t t11, int tap_abs, int tap_rel_1024) {
  uint16_t lo = t00, hi = t00;
  lo = t01 < lo ? t01 : lo; hi = t01 > hi ? t01 : hi;
  lo = t10 < lo ? t10 : lo; hi = t10 > hi ? t10 : hi;
  lo = t11 < lo ? t11 : lo; hi = t11 > hi ? t11 : hi;
  return ((int64_t)hi - (int64_t)lo) * 1024 <= (int64_t)tap_abs * 1024 + (int64_t)tap_rel_1024 * (int64_t)lo;
}

enum Outcome : int { kSampled = 0, kOutside = 1, kTapRefused = 2 };

// Steps G.1 - G.6 for keyframe pixel (r, c) with the VALID uploaded count u: the outcome, and *q, a count of 1 ... 65535,
// where it is kSampled.  *tap (may be null): the first tap's row-major index of a pixel that reached G.4
NID_DC_HD Outcome observe(const Gather &A, int r, int c, uint16_t u, uint32_t *q, size_t *tap = nullptr) {
  const double zk = (double)u * A.factor0;  // G.1 (dc::backproject's operations in its order)
  const double x = zk * (c - A.cx) / A.fx;
  const double y = zk * (r - A.cy) / A.fy;
  const double *K = A.K;
  const double xt = ((K[0] * x + K[1] * y) + K[2] * zk) + K[3];  // G.2 (summed as rf::splat sums)
  const double yt = ((K[4] * x + K[5] * y) + K[6] * zk) + K[7];
  const double zt = ((K[8] * x + K[9] * y) + K[10] * zk) + K[11];
  if (!(zt > 0)) return kOutside;
  const double ut = (A.fx * xt) / zt + A.cx;  // G.3
  const double vt = (A.fy * yt) / zt + A.cy;
  const double c0 = __builtin_floor(ut), r0 = __builtin_floor(vt);
  if (!(c0 >= 0 && c0 <= (double)(A.cols - 2) && r0 >= 0 && r0 <= (double)(A.rows - 2))) return kOutside;  // (NaN and the infinities fail)
  const double a = ut - c0, b = vt - r0;
  const size_t i00 = (size_t)(int)r0 * (size_t)A.cols + (size_t)(int)c0;  // G.4 (in range, with the row and the column behind it: decided above)
  if (tap) *tap = i00;
  const uint16_t t00 = A.d1[i00], t01 = A.d1[i00 + 1], t10 = A.d1[i00 + (size_t)A.cols], t11 = A.d1[i00 + (size_t)A.cols + 1];
  if (!(dc::depth_valid(t00, A.factor1) && dc::depth_valid(t01, A.factor1) && dc::depth_valid(t10, A.factor1) && dc::depth_valid(t11, A.factor1)))
    return kTapRefused;
  if (!taps_within(t00, t01, t10, t11, A.tap_abs, A.tap_rel_1024)) return kTapRefused;
  const double top = (double)t00 + a * ((double)t01 - (double)t00);  // G.5
  const double bot = (double)t10 + a * ((double)t11 - (double)t10);
  const double zo = (top + b * (bot - top)) * A.factor1;
  const double xo = zo * (ut - A.cx) / A.fx;  // G.6
  const double yo = zo * (vt - A.cy) / A.fy;
  const double *M = A.M;
  const double zk2 = ((M[8] * xo + M[9] * yo) + M[10] * zo) + M[11];
  const double qd = __builtin_floor(zk2 / A.factor0 + 0.5);
  if (!(qd >= 1 && qd <= 65535)) return kOutside;
  const uint32_t qi = (uint32_t)qd;  // (in range: decided above)
  if (!dc::depth_valid((uint16_t)qi, A.factor0)) return kOutside;
  *q = qi;
  return kSampled;
}

// THE RULE for one keyframe pixel, counted: *S and *k before / after; *base: the pixel's BASE count behind the call.
// Returns the FUSED plane's entry.  Part B is rfu::fuse on the observation, or on a z-buffer entry nothing has hit
NID_DC_HD uint16_t gather(const Gather &A, int r, int c, uint16_t u, int gate_abs, int gate_rel_1024, int max_obs, uint32_t *S, uint8_t *k,
                          uint16_t *base, nid_refgather_counts *n) {
  const bool valid = dc::depth_valid(u, A.factor0);
  uint32_t q = rf::kNone;
  if (valid) {  // G.0
    const Outcome o = observe(A, r, c, u, &q);
    n->n_sampled += o == kSampled;
    n->n_outside += o == kOutside;
    n->n_tap_refused += o == kTapRefused;
    if (o != kSampled) q = rf::kNone;
  }
  nid_reffuse_counts f = {};
  const uint16_t e = rfu::fuse(valid, u, q, gate_abs, gate_rel_1024, max_obs, S, k, base, &f);
  n->n_valid += f.n_valid;
  n->n_fused += f.n_fused;
  n->n_gated += f.n_gated;
  n->n_saturated += f.n_saturated;
  n->n_changed += f.n_changed;
  return e;
}

NID_DC_HD bool args_ok(int gate_abs, int gate_rel_1024, int max_obs, int tap_abs, int tap_rel_1024) {
  return rfu::args_ok(gate_abs, gate_rel_1024, max_obs) && tap_abs >= 0 && tap_abs <= 65535 && tap_rel_1024 >= 0 && tap_rel_1024 <= 1024;
}

// nid_refgather_host behind its argument checks: THE RULE over the whole plane, in place.  d0: the keyframe's uploaded
// depth; base: rows x cols of the caller's or null.
inline void refgather_host(const Gather &A, const uint16_t *d0, int gate_abs, int gate_rel_1024, int max_obs, uint32_t *sum, uint8_t *obs,
                           uint16_t *fused, uint16_t *base, nid_refgather_counts *counts) {
  nid_refgather_counts n = {};
  for (int r = 0; r < A.rows; r++)
    for (int c = 0; c < A.cols; c++) {
      const size_t i = (size_t)r * (size_t)A.cols + (size_t)c;
      uint16_t b = 0;
      fused[i] = gather(A, r, c, d0[i], gate_abs, gate_rel_1024, max_obs, sum + i, obs + i, &b, &n);
      if (base) base[i] = b;
    }
  if (counts) *counts = n;
}

}  // namespace rg
}  // namespace nid

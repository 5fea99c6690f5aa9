// nid_depth_check.h -- the per-sample rule of the depth-consistency check and the tracker's two decisions
// (include/nid/nid_keyframe.h): the ONE definition the device (k_depth_check in nid_setup_kernels.hip.h) and the host
// (nid_depth_check_host; the tracker in nid_keyframe.inc) are compiled from.
//
// Bitwise agreement of the two compilations: IEEE + - * / on doubles, comparisons, floor and integer arithmetic; both
// sides are compiled with -ffp-contract=off and without fast-math.  Every result is an integer, so neither the order of
// the samples nor how they are spread over lanes shows.  No HIP-only construct: a plain C++ translation unit can include
// this file (tests/cpp/depth_check_check.cpp, under the host sanitizers: no conversion here is reachable out of range).
#pragma once

#include <stdint.h>

#include "nid/nid_keyframe.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NID_DC_HD __host__ __device__ inline
#else
#define NID_DC_HD inline
#endif

namespace nid {
namespace dc {

constexpr double kUmSaturated = 9223372036854775808.0;  // 2^63: what a |dz| too large for the sum (or a NaN) adds

// what one pose's samples share
struct View {
  double M[12];  // rows of [R|t] (lm::pose_record)
  double fx, fy, cx, cy;
  int rows, cols;
  const uint16_t *d1;  // rows x cols
  double factor, tol_abs, tol_rel;
};

// One reference sample into the running counts `a` (steps 1 - 5 of nid_keyframe.h).
NID_DC_HD void sample(const View &V, double X, double Y, double Z, nid_depth_cell *a) {
  if (X != X) return;  // 1. no reference sample
  a->n_ref++;
  const double *M = V.M;
  const double xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3];  // 2.
  const double yc = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7];
  const double zc = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11];
  if (!(zc > 0)) return;
  const double u = (V.fx * xc) / zc + V.cx;  // 3.
  const double v = (V.fy * yc) / zc + V.cy;
  const double c = __builtin_floor(u + 0.5), r = __builtin_floor(v + 0.5);
  if (!(c >= 0 && c <= (double)(V.cols - 1) && r >= 0 && r <= (double)(V.rows - 1))) return;  // (NaN and the infinities fail)
  a->n_inframe++;
  const int ci = (int)c, ri = (int)r;  // (in range: decided above)
  const double zt = (double)V.d1[(size_t)ri * (size_t)V.cols + (size_t)ci] * V.factor;  // 4.
  if (zt < 0.01 || zt > 100) return;
  a->n_both++;
  const double tol = V.tol_abs + V.tol_rel * zt;  // 5.
  const double dz = zc - zt;
  if (dz > tol) { a->n_occluded++; return; }
  if (dz < -tol) { a->n_through++; return; }
  a->n_consistent++;
  const double um = (dz < 0 ? -dz : dz) * 1e6 + 0.5;
  a->sum_abs_um += um < kUmSaturated ? (uint64_t)um : (uint64_t)1 << 63;  // (um >= 0.5, or NaN -- a NaN factor --: the second arm)
}

NID_DC_HD void add_cell(nid_depth_counts *t, const nid_depth_cell &c) {
  t->n_ref += c.n_ref; t->n_inframe += c.n_inframe; t->n_both += c.n_both;
  t->n_consistent += c.n_consistent; t->n_occluded += c.n_occluded; t->n_through += c.n_through;
  t->sum_abs_um += c.sum_abs_um;
}

NID_DC_HD bool finite_nonneg(double v) { return v >= 0 && v <= 1.7976931348623157e308; }  // (false for NaN)

// nid_track_set_policy's argument rule
NID_DC_HD bool policy_valid(const nid_track_policy &P) {
  return (P.keyframe_mode == 0 || P.keyframe_mode == 1) && P.max_age >= 0 && P.min_samples >= 0 && P.reserved == 0 &&
         P.min_overlap >= 0 && P.min_overlap <= 1 && P.min_consistent >= 0 && P.min_consistent <= 1 &&
         finite_nonneg(P.tol_abs) && finite_nonneg(P.tol_rel);
}

// the default policy needs no check: the tracker then runs the schedule of nid_pyr_stream.h
NID_DC_HD bool policy_active(const nid_track_policy &P) { return P.keyframe_mode != 0 || P.min_consistent > 0; }

NID_DC_HD bool candidate_passes(const nid_track_policy &P, const nid_depth_counts &c) {
  return c.n_both >= (int64_t)P.min_samples && (double)c.n_consistent >= P.min_consistent * (double)c.n_both;
}

// candidates the tracker has checked for n candidates in rank order: all of them with verification on, the top one else
NID_DC_HD int candidates_to_check(const nid_track_policy &P, int n) { return P.min_consistent > 0 ? n : (n < 1 ? n : 1); }

// THE CHOICE among the candidates' counts (rank order): verification on -- the first that passes, -1 if none does;
// verification off -- the top candidate
NID_DC_HD int choose_candidate(const nid_track_policy &P, const nid_depth_counts *counts, int n) {
  if (n < 1) return -1;
  if (!(P.min_consistent > 0)) return 0;
  for (int k = 0; k < n; k++)
    if (candidate_passes(P, counts[k])) return k;
  return -1;
}

// THE PROMOTION RULE for a frame tracked OK: `chosen` the chosen candidate's counts, `age` the frames tracked OK on the
// keyframe, this one included
NID_DC_HD bool promote(const nid_track_policy &P, const nid_depth_counts &chosen, int32_t age) {
  if (P.keyframe_mode == 0) return true;
  if ((double)chosen.n_inframe < P.min_overlap * (double)chosen.n_ref) return true;
  return P.max_age > 0 && age >= P.max_age;
}

}  // namespace dc
}  // namespace nid

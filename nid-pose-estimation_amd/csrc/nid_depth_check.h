// nid_depth_check.h -- the per-sample rule of the depth-consistency check and the tracker's two decisions
// (include/nid/nid_keyframe.h): the ONE definition the device (k_depth_check in nid_setup_kernels.hip.h) and the host
// (nid_depth_check_host; the tracker in nid_keyframe.inc) are compiled from.  Behind them the rule of the reference mask
// (include/nid/nid_refmask.h) on the same terms: the set-up's back-projection (k_tile calls it), a pixel's byte from its
// class, the dilation's outcome and the counts -- k_refmask_classify / k_refmask_dilate_apply on the device,
// dc::refmask_host (nid_refmask_host) on the host.
//
// Bitwise agreement of the two compilations: IEEE + - * / on doubles, comparisons, floor and integer arithmetic; both
// sides are compiled with -ffp-contract=off and without fast-math.  Every result is an integer, so neither the order of
// the samples nor how they are spread over lanes shows.  No HIP-only construct: a plain C++ translation unit can include
// this file (tests/cpp/depth_check_check.cpp, under the host sanitizers: no conversion here is reachable out of range).
#pragma once

#include <stdint.h>

#include "nid/nid_keyframe.h"
#include "nid/nid_refmask.h"

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

// the View of one pose's matrix M, an image geometry g (Geometry on the device, nid_config on the host) and a call's arguments
template <class G>
NID_DC_HD View make_view(const G &g, const double *M, const uint16_t *d1, double factor, double tol_abs, double tol_rel) {
  View V;
  for (int k = 0; k < 12; k++) V.M[k] = M[k];
  V.fx = g.fx; V.fy = g.fy; V.cx = g.cx; V.cy = g.cy;
  V.rows = g.rows; V.cols = g.cols;
  V.d1 = d1; V.factor = factor; V.tol_abs = tol_abs; V.tol_rel = tol_rel;
  return V;
}

// The class of one reference sample (steps 1 - 5 of nid_keyframe.h), in the order the steps decide it
enum Class : int {
  kNone = 0,           // 1. no reference sample
  kNotInView = 1,      // 2. / 3. behind the camera or out of the frame
  kNoTargetDepth = 2,  // 4. the target's depth there is not valid
  kConsistent = 3,     // 5.
  kOccluded = 4,
  kThrough = 5
};

// THE RULE for one sample; *dz (may be null) is zc - zt of a sample that reached step 5
NID_DC_HD Class classify(const View &V, double X, double Y, double Z, double *dz_out = nullptr) {
  if (X != X) return kNone;  // 1. no reference sample
  const double *M = V.M;
  const double xc = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3];  // 2.
  const double yc = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7];
  const double zc = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11];
  if (!(zc > 0)) return kNotInView;
  const double u = (V.fx * xc) / zc + V.cx;  // 3.
  const double v = (V.fy * yc) / zc + V.cy;
  const double c = __builtin_floor(u + 0.5), r = __builtin_floor(v + 0.5);
  if (!(c >= 0 && c <= (double)(V.cols - 1) && r >= 0 && r <= (double)(V.rows - 1))) return kNotInView;  // (NaN and the infinities fail)
  const int ci = (int)c, ri = (int)r;  // (in range: decided above)
  const double zt = (double)V.d1[(size_t)ri * (size_t)V.cols + (size_t)ci] * V.factor;  // 4.
  if (zt < 0.01 || zt > 100) return kNoTargetDepth;
  const double tol = V.tol_abs + V.tol_rel * zt;  // 5.
  const double dz = zc - zt;
  if (dz_out) *dz_out = dz;
  if (dz > tol) return kOccluded;
  if (dz < -tol) return kThrough;
  return kConsistent;
}

// One reference sample into the running counts `a`: the class, counted.
NID_DC_HD void sample(const View &V, double X, double Y, double Z, nid_depth_cell *a) {
  double dz = 0;
  const Class k = classify(V, X, Y, Z, &dz);
  if (k == kNone) return;
  a->n_ref++;
  if (k == kNotInView) return;
  a->n_inframe++;
  if (k == kNoTargetDepth) return;
  a->n_both++;
  if (k == kOccluded) { a->n_occluded++; return; }
  if (k == kThrough) { a->n_through++; return; }
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


// ---- nid_refmask.h --------------------------------------------------------------------------------------------------------
// The set-up's back-projection of one pixel (k_tile calls it: ITS operations in its order): z in metres, the validity
// test, x0, y0, the three rows of the column-major T_wc.  false -- and X, Y, Z untouched -- where the depth is not valid.
NID_DC_HD bool backproject(double z, int r, int col, double fx, double fy, double cx, double cy, const double *Twc, double *X,
                           double *Y, double *Z) {
  if (z < 0.01 || z > 100) return false;  // CudaPoints3d.cu:12
  const double x0 = z * (col - cx) / fx;
  const double y0 = z * (r - cy) / fy;
  *X = Twc[0] * x0 + Twc[4] * y0 + Twc[8] * z + Twc[12];
  *Y = Twc[1] * x0 + Twc[5] * y0 + Twc[9] * z + Twc[13];
  *Z = Twc[2] * x0 + Twc[6] * y0 + Twc[10] * z + Twc[14];
  return true;
}

// what one masking call's pixels share besides the View of the target
struct Keyframe {
  const uint16_t *d0;  // the pristine depth, rows x cols
  double factor;
  const double *Twc;  // column-major 16
};

// Steps 1 - 3 of nid_refmask.h for pixel (r, col): the byte behind the classification, from the byte before it.
NID_DC_HD uint8_t mask_classified(const View &V, const Keyframe &K, int r, int col, uint8_t old, int classes, int accumulate) {
  uint8_t b = (uint8_t)(old & (accumulate ? 15 : NID_REFMASK_CALLER));
  double X, Y, Z;
  if (!backproject((double)K.d0[(size_t)r * (size_t)V.cols + (size_t)col] * K.factor, r, col, V.fx, V.fy, V.cx, V.cy, K.Twc, &X, &Y, &Z)) return b;
  const Class k = classify(V, X, Y, Z);
  if (k == kOccluded && (classes & NID_REFMASK_OCCLUDED)) b |= NID_REFMASK_OCCLUDED;
  if (k == kThrough && (classes & NID_REFMASK_THROUGH)) b |= NID_REFMASK_THROUGH;
  return b;
}

constexpr int kClassBits = NID_REFMASK_OCCLUDED | NID_REFMASK_THROUGH;

// Step 4 for one pixel: the final byte from the classified byte and whether a pixel of S lies in its window.
NID_DC_HD uint8_t mask_final(uint8_t classified, bool near_S) {
  if (classified & kClassBits) return (uint8_t)(classified & ~NID_REFMASK_DILATED);
  return near_S ? (uint8_t)(classified | NID_REFMASK_DILATED) : classified;
}

// one pixel of the final plane into the counts
NID_DC_HD void mask_count(uint8_t b, bool valid, nid_refmask_counts *n) {
  n->n_valid += valid;
  n->n_caller += (b & NID_REFMASK_CALLER) != 0;
  n->n_occluded += (b & NID_REFMASK_OCCLUDED) != 0;
  n->n_through += (b & NID_REFMASK_THROUGH) != 0;
  n->n_dilated += (b & NID_REFMASK_DILATED) != 0;
  n->n_masked += valid && b;
}

NID_DC_HD bool depth_valid(uint16_t d, double factor) {
  const double z = (double)d * factor;
  return !(z < 0.01 || z > 100);
}

// nid_refmask_host behind its argument checks: THE RULE over the whole plane, in place.  The window of step 4 is searched
// pixel by pixel (the device's dilation is separable: two ways to the same set).
inline void refmask_host(const View &V, const Keyframe &K, int classes, int dilate, int accumulate, uint8_t *mask, nid_refmask_counts *counts) {
  const int rows = V.rows, cols = V.cols;
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) {
      uint8_t &b = mask[(size_t)r * (size_t)cols + (size_t)c];
      b = mask_classified(V, K, r, c, b, classes, accumulate);
    }
  // (step 4 changes bit 8 alone, S is read from bits 2 and 4: the plane can be finished in place)
  nid_refmask_counts n = {};
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) {
      const size_t i = (size_t)r * (size_t)cols + (size_t)c;
      bool near_S = false;
      if (dilate > 0 && !(mask[i] & kClassBits)) {
        const int r0 = r - dilate < 0 ? 0 : r - dilate, r1 = r + dilate > rows - 1 ? rows - 1 : r + dilate;
        const int c0 = c - dilate < 0 ? 0 : c - dilate, c1 = c + dilate > cols - 1 ? cols - 1 : c + dilate;
        for (int rr = r0; rr <= r1 && !near_S; rr++)
          for (int cc = c0; cc <= c1; cc++)
            if (mask[(size_t)rr * (size_t)cols + (size_t)cc] & kClassBits) { near_S = true; break; }
      }
      mask[i] = mask_final(mask[i], near_S);
      mask_count(mask[i], depth_valid(K.d0[i], K.factor), &n);
    }
  if (counts) *counts = n;
}

NID_DC_HD bool refmask_args_ok(double tol_abs, double tol_rel, int classes, int dilate) {
  return finite_nonneg(tol_abs) && finite_nonneg(tol_rel) && (classes & ~kClassBits) == 0 && dilate >= 0 && dilate <= NID_REFMASK_MAX_DILATE;
}

}  // namespace dc
}  // namespace nid

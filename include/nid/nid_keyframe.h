/*
 * nid_keyframe.h -- a depth-consistency check on the resident pyramid of nid_pyr.h and a keyframe policy for the tracker
 * of nid_pyr_stream.h (libnid_hip.so).
 *
 * THE CHECK.  For a candidate pose, every 3-D point of the keyframe (level 0's tiles) is projected into the current
 * camera and compared with the current frame's depth map there.  Per sample (csrc/nid_depth_check.h: ONE text, compiled
 * for the device -- k_depth_check -- and for the host -- nid_depth_check_host --, IEEE + - * /, comparisons and floor,
 * no contraction), with M[12] the rows of [R|t] of the pose (what the evaluations' pose record holds), the level's
 * fx, fy, cx, cy, rows, cols, the target depth d1 (u16) and its factor:
 *   1. a NaN in X: the slot is no reference sample (padding, invalid depth), nothing is counted.  Otherwise n_ref++.
 *   2. xc = ((M[0] X + M[1] Y) + M[2] Z) + M[3], yc and zc likewise from rows 1 and 2.  !(zc > 0) ends the sample.
 *   3. u = (fx xc) / zc + cx, v = (fy yc) / zc + cy; c = floor(u + 0.5), r = floor(v + 0.5) as doubles; in frame iff
 *      0 <= c <= cols - 1 and 0 <= r <= rows - 1 (compared as doubles: NaN and the infinities fail).  n_inframe++.
 *   4. zt = (double)d1[r cols + c] * factor; zt < 0.01 || zt > 100 (the validity test of the back-projection) ends the
 *      sample.  Otherwise n_both++.
 *   5. tol = tol_abs + tol_rel zt, dz = zc - zt.  dz > tol: n_occluded++ (the keyframe's point lies behind what the
 *      camera sees now); dz < -tol: n_through++ (the camera sees through the place where the point should be); else
 *      n_consistent++ and sum_abs_um += (uint64)(|dz| 1e6 + 0.5) -- a value of 2^63 or more, or a NaN, adds 2^63.
 * Everything is an integer: the counts do not depend on the order of the samples, on the workgroup shape or on what else
 * is in the batch, and the device and the host give the same.
 *
 * THE TRACKER'S POLICY.  With the default policy (nid_track_policy_default, or none ever set) nid_track_push_u16 is the
 * schedule of nid_pyr_stream.h, call for call.  A policy is ACTIVE when keyframe_mode != 0 or min_consistent > 0.  With
 * an active policy the FIRST frame and a later frame WITHOUT depth are as in nid_pyr_stream.h (nothing is checked, the
 * keyframe stays); a later frame WITH depth is, with cur / prev as there:
 *     1. nid_pyr_set_target_u8(im); nid_pyr_set_target_depth_u16(depth, factor);
 *     2. - 4. the prediction, the starts and nid_pyr_multistart_lm as in nid_pyr_stream.h;
 *     best_origin < 0: NID_TRACK_LOST as in nid_pyr_stream.h (n_checked = 0).  Otherwise
 *     5a. the candidates: level 0's chains with finite chi2 and n_active > 0 in rank order, chi2 / n_active ascending,
 *         the lower index first (nid_pyr.h step 3);
 *     5b. ONE nid_pyr_depth_check(poses, m, tol_abs, tol_rel) -- with min_consistent > 0 (verification on) over all
 *         candidates' poses in rank order, the frame's pose being the first candidate with n_both >= min_samples and
 *         (double)n_consistent >= min_consistent * (double)n_both; with verification off over the top candidate alone,
 *         which is the frame's pose;
 *     5c. no candidate passes: status NID_TRACK_REJECTED, cur unchanged, the velocity forgotten, no promotion,
 *         best_origin the top candidate's origin, chi2 = 0, n_active = 0, the call returns NID_OK; nid_track_last_check
 *         gives the top candidate's counts;
 *     5d. a candidate is chosen: prev = cur, cur = its pose, status NID_TRACK_OK, best_origin / chi2 / n_active that
 *         chain's; age = age + 1.  Promotion: keyframe_mode 0 always; keyframe_mode 1 iff
 *         (double)n_inframe < min_overlap * (double)n_ref (the chosen candidate's counts) or (max_age > 0 and
 *         age >= max_age).  A promotion is nid_pyr_promote_target(nid_track_pose_to_Twc16(cur)) and sets age = 0.
 * age is 0 after the first frame.  Errors of composed calls are returned as they are, as in nid_pyr_stream.h.
 *
 * Out of scope: cell shards and several devices, a target depth on the coarser levels, a host-layer wrapper, an
 * asynchronous push.  Per-pixel masks on the reference, fed back into the evaluation, are nid_refmask.h, which lists
 * masks on the target, shards and masks on several devices as out of scope.
 */
#ifndef NID_KEYFRAME_H
#define NID_KEYFRAME_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_pyr.h"
#include "nid/nid_pyr_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one cell's counts for one pose / the exact sum of a pose's cells */
typedef struct {
  int32_t n_ref, n_inframe, n_both, n_consistent, n_occluded, n_through;
  uint64_t sum_abs_um; /* sum of |dz| over the consistent samples, in micrometres, each rounded half up */
} nid_depth_cell;      /* 32 bytes */
typedef struct {
  int64_t n_ref, n_inframe, n_both, n_consistent, n_occluded, n_through;
  uint64_t sum_abs_um, reserved;
} nid_depth_counts; /* 64 bytes */

/* ---- on a nid_pyr ------------------------------------------------------------------------------------------------------ */

/* The depth map of the RESIDENT TARGET, kept on the device at level 0 (rows x cols of level 0).  Opens and closes like
 * the frame operations of nid_pyr_stream.h (NID_ERR_STATE and nothing changed while a level has an uncollected launch;
 * one stream, one synchronisation).  NID_ERR_STATE without a target.  nid_pyr_set_target_u8 and nid_pyr_set_pair_u16
 * drop the target depth: it belongs to the image it came with. */
int nid_pyr_set_target_depth_u16(nid_pyr *p, const uint16_t *depth_u16, double depth_factor);

/* nid_pyr_promote_target_u16(the resident target depth, its factor, T_wc) without the upload: the depth is copied on the
 * device.  Every level holds the same bytes afterwards; the target, its margins and its depth stay.  NID_ERR_STATE
 * without a target depth (and then nothing changed: a reference that was evaluable still is). */
int nid_pyr_promote_target(nid_pyr *p, const double *T_wc_colmajor16);

/* The check at the head of this file on level 0's tiles against the resident target depth, for n poses (pose7, world ->
 * camera) at once, 1 <= n <= NID_MAX_BATCH.  totals[n]; cells (may be NULL): n x (cells of level 0), pose-major, cell
 * c = ci * cell_num + cj.  Blocking.  NID_ERR_INVALID_ARG for a null pointer, n out of range or a tolerance that is
 * negative or not finite -- checked before any device is touched.  NID_ERR_STATE without a reference, without a target
 * depth or while a level has an uncollected launch.  The public slots and the reference stage are not touched: a level
 * stays evaluable across the call. */
int nid_pyr_depth_check(nid_pyr *p, const double *poses7, int n, double tol_abs, double tol_rel,
                        nid_depth_counts *totals, nid_depth_cell *cells);

/* The same text compiled for the host, over nid_get_points3d's layout (3 doubles per pixel, image order), grouped into
 * cells as the tiles are (cell c = ci * cell_num + cj owns rows ci * (rows / cell_num) ..., columns cj * (cols /
 * cell_num) ...; pixels of no cell are not counted).  One pose; total and cells (cell_num^2 records) may each be NULL,
 * not both.  Never touches a device.  NID_ERR_INVALID_ARG for a null pointer, a cfg with rows, cols or cell_num < 1 or
 * that does not own all cells, or a tolerance that is negative or not finite. */
int nid_depth_check_host(const nid_config *cfg, const double *points3d, const uint16_t *depth1_u16, double depth_factor,
                         const double *pose7, double tol_abs, double tol_rel, nid_depth_counts *total,
                         nid_depth_cell *cells);

/* ---- the tracker's policy ---------------------------------------------------------------------------------------------- */
#define NID_TRACK_REJECTED 3 /* chains were eligible, none passed the depth verification */
typedef struct {
  int32_t keyframe_mode;  /* 0 = promote every frame with depth, 1 = promote on demand */
  int32_t max_age;        /* on demand: promote once this many frames were tracked on the keyframe; 0 = no limit */
  int32_t min_samples;    /* a candidate with n_both below this cannot be verified */
  int32_t reserved;       /* 0 */
  double min_overlap;     /* on demand: promote when n_inframe / n_ref falls below this */
  double min_consistent;  /* > 0: verification on; a candidate passes iff n_both >= min_samples and
                             (double)n_consistent >= min_consistent * (double)n_both */
  double tol_abs, tol_rel; /* metres, and a fraction of the observed depth */
} nid_track_policy;

/* keyframe_mode 0, max_age 0, min_samples 0, min_overlap 0, min_consistent 0 (not active: the tracker of
 * nid_pyr_stream.h), tol_abs 0.01 m, tol_rel 0.02 -- the tolerances are design choices: a centimetre of quantisation and
 * pose error near the camera, and two per cent for a sensor whose depth noise grows with the distance. */
int nid_track_policy_default(nid_track_policy *out);
/* NID_ERR_INVALID_ARG for a null pointer, keyframe_mode other than 0 / 1, a negative max_age or min_samples, reserved
 * != 0, min_overlap or min_consistent outside [0, 1] or not finite, a tolerance that is negative or not finite. */
int nid_track_set_policy(nid_track *t, const nid_track_policy *policy);
/* Of the last push that returned NID_OK: the counts of the chosen candidate (REJECTED: the top candidate's; nothing
 * checked: zeros), the number of poses that were checked, and the age after it -- frames tracked OK on the keyframe
 * since it was promoted.  Any pointer but t may be NULL. */
int nid_track_last_check(const nid_track *t, nid_depth_counts *chosen, int32_t *n_checked, int32_t *age);

#ifdef __cplusplus
}
#endif
#endif

/*
 * nid_pyr_stream.h -- frame streams on the resident pyramid of nid_pyr.h (libnid_hip.so): the two frame operations a
 * sequence needs beside nid_pyr_set_pair_u16, the pose arithmetic of a sequence, and a small tracker on top of them.
 *
 * Frame k+1 of a video is the target of pair (k, k+1) and the reference of pair (k+1, k+2).  nid_pyr_set_target_u8
 * replaces the target alone on every level; nid_pyr_promote_target_u16 makes the resident target the reference, with
 * its depth and its pose in the world.  An image crosses to the device once and its pyramid is built once; a keyframe
 * tracker (one reference, many targets) repeats nothing of the reference side.
 *
 * Poses: pose7 = {qx, qy, qz, qw, tx, ty, tz} of nid_c.h, a unit quaternion with w >= 0; a frame's pose is its
 * WORLD -> CAMERA transform (what the evaluations take), T_wc is the column-major 4x4 CAMERA -> WORLD matrix the set-up
 * kernels take.
 *
 * nid_track_push_u16 is a composition of the calls of this header and nid_pyr_multistart_lm, stated exactly so that it
 * can be restated and compared bit for bit.  With cur / prev the poses of the last two tracked frames:
 *   FIRST frame (no reference yet):
 *     nid_pyr_set_target_u8(im); nid_pyr_promote_target_u16(depth, factor, T_wc_first) -- depth == NULL is
 *     NID_ERR_INVALID_ARG, T_wc_first == NULL the identity --; cur = nid_track_pose_from_Twc16(T_wc_first); no
 *     velocity; status NID_TRACK_FIRST, promoted = 1.
 *   every LATER frame:
 *     1. nid_pyr_set_target_u8(im);
 *     2. the prediction: pred = (cur o inverse(prev)) o cur if both are known (nid_track_pose_inverse, then
 *        nid_track_pose_compose twice), else pred = cur;
 *     3. the starts, n = 2 + n_twists of them: [pred, cur, perturb(pred, twist_0), perturb(pred, twist_1), ...];
 *     4. nid_pyr_multistart_lm(starts, n, pose_ref7 = NULL, iterations, huber_delta, keep, ...);
 *     5. best_origin >= 0: prev = cur, cur = the best pose, status NID_TRACK_OK; chi2 / n_active are those of level 0's
 *        chain of that origin.  If depth != NULL: nid_pyr_promote_target_u16(depth, factor,
 *        nid_track_pose_to_Twc16(cur)), promoted = 1.  With depth == NULL the keyframe stays (intensity-only frames);
 *     6. best_origin < 0 (no eligible chain on some level): status NID_TRACK_LOST, cur unchanged, the velocity
 *        forgotten (prev unknown), no promotion -- the old keyframe stays the reference --, chi2 = 0, n_active = 0, and
 *        the call returns NID_OK.
 * An error of a composed call is returned as it is; the tracker's poses and frame count are then those from before the
 * call, while the pyramid's target is the new image (or not ready, if the error was nid_pyr_set_target_u8's), and its
 * reference is not ready if the error was the promotion's.
 *
 * Out of scope: cell shards or several devices, an asynchronous push, a host-layer wrapper.  Keyframe selection policies
 * and a check of a result against the frame's depth are a header of their own: nid/nid_keyframe.h; without a policy set
 * there, the tracker is exactly the schedule above.
 */
#ifndef NID_PYR_STREAM_H
#define NID_PYR_STREAM_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_pyr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- frame operations on a nid_pyr ---------------------------------------------------------------------------------
 * Both follow nid_pyr_set_pair_u16's discipline: NID_ERR_STATE (and nothing changed) while a level context has an
 * uncollected launch; everything enqueued on ONE stream (level 0's) with one synchronisation at the end, before
 * anything is marked ready; an error leaves the side that was being overwritten not ready. */

/* A new target on every level: level 0's image uploaded, every coarser level made on the device (k_pyr_down_u8: the
 * 2x2 box mean of nid_pyr_set_pair_u16's levels, byte for byte), every level's margins.  Tiles, reference image, depth
 * and the reference stage of every level are untouched: a level on which nid_compute_href has run stays evaluable.  May
 * be called before any pair exists: the pyramid then has a target and no reference. */
int nid_pyr_set_target_u8(nid_pyr *p, const uint8_t *im1);

/* The resident target becomes the reference: on every level the target image is copied to the reference image on the
 * device, the depth goes up to level 0 and down the levels on the device (k_pyr_down_depth), back-projection and tiles
 * are made with T_wc.  The target and its margins stay.  Afterwards every level is in the state
 * nid_pyr_set_pair_u16(depth, im, im, T_wc) leaves (href not set).  NID_ERR_STATE if the pyramid has no target. */
int nid_pyr_promote_target_u16(nid_pyr *p, const uint16_t *depth_u16, double depth_factor,
                               const double *T_wc_colmajor16);

/* ---- pose helpers: pure arithmetic, never touch a device (csrc/nid_track_pose.h) -----------------------------------
 * IEEE + - * / sqrt only, compiled without contraction; every output quaternion is renormalised with w >= 0.
 * NID_ERR_INVALID_ARG for a null pointer.  Outputs may alias inputs. */
int nid_track_pose_inverse(const double *pose7, double *out7);
int nid_track_pose_compose(const double *a7, const double *b7, double *out7); /* a o b: b applied first */
/* exp(twist) o pose, twist6 = {omega (rotation) 0..2, upsilon 3..5}: the update of nid_multistart_lm's chains
 * (VertexSE3Expmap::oplusImpl), from the same text. */
int nid_track_pose_perturb(const double *pose7, const double *twist6, double *out7);
/* world -> camera pose7 -> the column-major camera -> world matrix, and back (rotation by Eigen's Quaterniond(R)). */
int nid_track_pose_to_Twc16(const double *pose7_cw, double *T_wc_colmajor16);
int nid_track_pose_from_Twc16(const double *T_wc_colmajor16, double *pose7_cw);

/* ---- the tracker --------------------------------------------------------------------------------------------------- */
typedef struct nid_track nid_track;
#define NID_TRACK_FIRST 0 /* first frame: became the reference, nothing tracked */
#define NID_TRACK_OK 1
#define NID_TRACK_LOST 2 /* no eligible chain on some level */
typedef struct {
  double pose7[7]; /* world -> camera of this frame (LOST: the previous pose, unchanged) */
  double chi2;
  int32_t n_active, best_origin, status, promoted, frame; /* frame: 0 for the first push, counted over every push that returned NID_OK */
  int32_t rounds[NID_PYR_MAX_LEVELS]; /* coarsest first, as nid_pyr_multistart_lm's; unused entries 0 */
} nid_track_result;

/* Owns a nid_pyr (nid_pyr_create's argument rules, checked before any device is touched; NID_ERR_NO_DEVICE without a
 * device).  Defaults: 10 iterations per level, huber_delta sqrt(0.95), keep NULL, no twists (two starts). */
int nid_track_create(const nid_config *cfg0, int levels, nid_track **out);
int nid_track_destroy(nid_track *t);
/* The tracker's pyramid (NULL for a null handle); options on its level contexts are the caller's. */
nid_pyr *nid_track_pyramid(nid_track *t);
/* iterations >= 1; keep[levels] or NULL, 1 <= keep[l] <= keep[l+1] (keep[levels-1] must be 2 + n_twists when a frame
 * is pushed: nid_pyr_multistart_lm's rule). */
int nid_track_set_lm(nid_track *t, int iterations, double huber_delta, const int32_t *keep);
/* The start fan around the prediction: n x 6, 0 <= n <= NID_MAX_BATCH - 2 (twists6 may be NULL for n = 0). */
int nid_track_set_twists(nid_track *t, const double *twists6, int n);
/* Overrides the current pose (world -> camera) and forgets the velocity. */
int nid_track_set_pose(nid_track *t, const double *pose7);
/* One frame: the schedule at the head of this file.  depth_u16 may be NULL on a later frame (the keyframe stays);
 * T_wc_first16 is read on the first frame only (NULL: identity).  Blocking. */
int nid_track_push_u16(nid_track *t, const uint16_t *depth_u16, double depth_factor, const uint8_t *im,
                       const double *T_wc_first16, nid_track_result *out);

#ifdef __cplusplus
}
#endif
#endif

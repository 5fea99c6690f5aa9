/*
 * nid_reffill.h -- depth for the holes of the REFERENCE (the keyframe) of the resident pyramid of nid_pyr.h, taken from
 * tracked frames, and the tracker's use of it (libnid_hip.so).  nid_keyframe.h and nid_refmask.h can only take samples
 * away from a keyframe; a fill gives one back: a keyframe pixel whose depth sample is invalid (0, below 0.01 m, above
 * 100 m) has an intensity and no point, and every later frame with depth shows the surface behind it.
 *
 * WHAT A FILL IS.  A rebuild of the reference set-up from a completed depth plane; no evaluation kernel knows of it.  A
 * pyramid carries
 *   - a level-0 u16 FILL PLANE, rows x cols: 0 -- not filled; any other value -- the fill, in counts of the reference's
 *     depth factor.  Only pixels whose uploaded depth is invalid carry one;
 *   - an UPLOADED COPY of level 0's reference depth as it was made, taken on the first fill behind a new reference: a
 *     caller who never fills pays nothing.
 * The PRISTINE depth of nid_refmask.h becomes fill ? fill : uploaded, the effective level-0 depth
 * mask ? 0 : (fill ? fill : uploaded); coarser levels and every level's reference half follow through the masking calls'
 * own chain.  So a filled pyramid is, byte for byte and bit for bit, the pyramid of the same pair with those depth samples
 * written in.  After a fill call every level is in the state a promotion leaves (a reference, no reference stage); the
 * mask plane is unchanged byte for byte -- a mask bit on a pixel that has just become valid now masks it --, and later
 * nid_pyr_mask_occluded calls classify filled pixels like any other: they read pristine depth.  A new reference --
 * nid_pyr_set_pair_u16 and both promotions -- starts unfilled.  The calls open and close like the masking calls:
 * NID_ERR_STATE and nothing changed without a reference or while a level has an uncollected launch; one stream, one
 * synchronisation; no slot is touched and no evaluation kernel is launched.
 *
 * THE RULE of nid_pyr_fill_reference_depth / nid_reffill_host (csrc/nid_reffill_rule.h: ONE text, compiled for the device
 * and for the host; IEEE + - * /, comparisons, floor and integer arithmetic, no contraction).  M is the 3 x 4 matrix that
 * takes the target camera to the keyframe camera, x_k = T_cw(keyframe) T_wc(target) x_t, made once per call on the host:
 * the keyframe's world -> camera pose from its T_wc (nid_track_pose_from_Twc16), composed with the inverse of pose7
 * (nid_track_pose_compose, nid_track_pose_inverse), and the rows of [R|t] of that pose.
 *   A. SPLAT.  For every target pixel (r1, c1):
 *      1. zt = (double)depth1[r1 cols + c1] * factor1; zt < 0.01 || zt > 100 ends the pixel.  Otherwise n_target_valid++.
 *      2. x = zt (c1 - cx) / fx, y = zt (r1 - cy) / fy (the set-up's back-projection, operation for operation).
 *      3. xk = M[0] x + M[1] y + M[2] zt + M[3] (summed left to right), yk and zk from rows 1 and 2; !(zk > 0) ends.
 *      4. u = (fx xk) / zk + cx, v = (fy yk) / zk + cy, c = floor(u + 0.5), r = floor(v + 0.5); 0 <= c <= cols - 1 and
 *         0 <= r <= rows - 1 are decided on the doubles (NaN and the infinities fail), only then c and r become integers.
 *      5. q = floor(zk / factor0 + 0.5); as a double 1 <= q <= 65535, and (double)q * factor0 must be a valid depth.
 *         Otherwise the pixel ends.
 *      6. n_splat++ and zbuf[r, c] = min(zbuf[r, c], q).
 *   B. GUARD, in integers.  S(p), the surface at keyframe pixel p: zbuf[p] if p was hit; else the uploaded count if it is
 *      valid; else none.  A hit at p with count q is REFUSED if some pixel p' != p within Chebyshev distance `guard` (the
 *      window clipped at the image) has S(p') = q' with (q - q') 1024 > guard_abs 1024 + guard_rel_1024 q' in 64-bit
 *      integers: the hit lies behind a neighbouring surface -- the leak of a forward splat through a nearer surface's
 *      sampling gaps.  guard 0 refuses nothing.
 *   C. APPLY.  For every keyframe pixel: uploaded depth valid -- fill 0; else accumulate set and the old fill non-zero --
 *      the old fill stays (the first fill wins); else hit and not refused -- fill = zbuf; else fill 0.
 * The counts: n_target_valid and n_splat of A; n_hit the keyframe pixels with a z-buffer entry; n_holes the pixels whose
 * uploaded depth is invalid; n_refused the hole pixels without a kept fill whose hit the guard refused; n_new the pixels
 * whose fill went from 0 to non-zero in this call; n_filled the non-zero entries of the final plane.  Everything is an
 * integer and a minimum does not depend on order: the device and the host give the same counts and the same plane.
 *
 * THE TRACKER.  nid_track_set_filling(on, guard, guard_abs, guard_rel_1024); off is the default, and then the tracker is
 * nid_refmask.h's, call for call.  With filling on AND an active policy (nid_keyframe.h), a later frame with depth whose
 * step 5d chooses a candidate and does NOT promote gets, after the choice and before step 5e's mask,
 *     5d'. nid_pyr_fill_reference_depth(the chosen pose, guard, guard_abs, guard_rel_1024, accumulate = 1)
 * -- fills persist over a keyframe's life, the first one wins; the mask of step 5e is still made afresh from every frame
 * and now sees the filled pixels too.  REJECTED, LOST, depth-less and promoted frames run no fill; a promoted frame starts
 * unfilled.  An error is returned as it is and the poses have not moved.
 * A fill trusts the chosen pose: with verification off (min_consistent == 0) a frame LM loses to a false minimum writes
 * its depth into the keyframe's holes at that wrong pose, and accumulate keeps it.  Use filling with verification on
 * (min_consistent > 0).  And where the keyframe has no depth there is nothing to check a frame against: a moving object
 * seen through a hole cannot be told from the scene, and its depth is filled in like any other.
 *
 * Refining depths that are already valid is nid_reffuse.h's; once a pyramid has been fused there, "uploaded" in THE RULE
 * above reads as its BASE plane, fused ? fused : uploaded.  Out of scope: fills on the target, cell shards, several devices,
 * a fill plane on the coarser levels.
 */
#ifndef NID_REFFILL_H
#define NID_REFFILL_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_pyr.h"
#include "nid/nid_pyr_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NID_REFFILL_MAX_GUARD 2

typedef struct {
  int64_t n_target_valid; /* target pixels with a valid depth */
  int64_t n_splat;        /* ... of them, those that reached the z-buffer */
  int64_t n_hit;          /* keyframe pixels with a z-buffer entry */
  int64_t n_holes;        /* keyframe pixels whose uploaded depth is invalid */
  int64_t n_refused;      /* hole pixels without a kept fill whose hit the guard refused */
  int64_t n_new;          /* pixels whose fill went from 0 to non-zero in this call */
  int64_t n_filled;       /* non-zero entries of the final plane */
  int64_t reserved;       /* 0 */
} nid_reffill_counts; /* 64 bytes */

/* ---- on a nid_pyr ------------------------------------------------------------------------------------------------------
 * Argument errors (NID_ERR_INVALID_ARG) are reported before any device is touched: a null handle or pose, guard outside
 * 0 ... NID_REFFILL_MAX_GUARD, guard_abs outside 0 ... 65535, guard_rel_1024 outside 0 ... 1024.  NID_ERR_STATE, and nothing
 * changed, without a reference or while a level has an uncollected launch; nid_pyr_fill_reference_depth -- the one call
 * that reads it -- also without a target depth (nid_pyr_set_target_depth_u16). */

/* THE RULE at the head of this file for pose7 (world -> camera, the target's) against the resident target depth, then the
 * rebuild.  accumulate: 0 makes the plane afresh, any other value keeps the fills it has.  out may be NULL. */
int nid_pyr_fill_reference_depth(nid_pyr *p, const double *pose7, int guard, int guard_abs, int guard_rel_1024, int accumulate,
                                 nid_reffill_counts *out);

/* Every fill to 0 and the reference rebuilt: the never-filled pyramid's bits on every level (the mask stays).  A no-op
 * returning NID_OK when nothing is filled (the reference stage then stays too). */
int nid_pyr_clear_reference_fill(nid_pyr *p);

/* The plane as the device holds it (zeros behind a new reference). */
int nid_pyr_get_reference_fill_u16(nid_pyr *p, uint16_t *out);

/* The same text compiled for the host: one call of THE RULE on fill_inout (rows x cols, the plane before / after).  cfg:
 * rows, cols and the intrinsics of level 0; depth0_u16 / factor0 / T_wc_colmajor16: the keyframe's uploaded depth, its
 * factor and camera -> world matrix; depth1_u16 / factor1: the target's depth.  counts may be NULL.  Never touches a
 * device.  NID_ERR_INVALID_ARG for a null pointer, rows or cols < 1, rows x cols above INT32_MAX, or a guard argument out
 * of range. */
int nid_reffill_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *T_wc_colmajor16,
                     const uint16_t *depth1_u16, double factor1, const double *pose7, int guard, int guard_abs, int guard_rel_1024,
                     int accumulate, uint16_t *fill_inout, nid_reffill_counts *counts);

/* ---- the tracker ------------------------------------------------------------------------------------------------------- */
/* on: 0 = off (the default); the guard arguments as above (checked also when on is 0). */
int nid_track_set_filling(nid_track *t, int on, int guard, int guard_abs, int guard_rel_1024);
/* Of the last push that returned NID_OK: the counts of its fill, zeros if it ran none. */
int nid_track_last_fill(const nid_track *t, nid_reffill_counts *counts);

#ifdef __cplusplus
}
#endif
#endif

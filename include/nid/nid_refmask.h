/*
 * nid_refmask.h -- a per-pixel mask on the REFERENCE (the keyframe) of the resident pyramid of nid_pyr.h, and the tracker's
 * use of it (libnid_hip.so).  A masked keyframe pixel takes no part in any evaluation until it is unmasked or the
 * reference is replaced.
 *
 * WHAT A MASK IS.  An invalid reference sample already exists in this library: a depth of 0 -- the set-up writes a NaN
 * point and a bin index of -1 for it, and the reference stage counts it out of N_c.  A mask is therefore a rebuild of the
 * reference set-up from a masked depth plane; no evaluation kernel knows of it.  A pyramid carries
 *   - a level-0 u8 MASK PLANE, rows x cols; a pixel is masked iff its byte is non-zero.  Bits: NID_REFMASK_CALLER (set
 *     by the caller), NID_REFMASK_OCCLUDED, NID_REFMASK_THROUGH (the two classes of the depth-consistency check of
 *     nid_keyframe.h), NID_REFMASK_DILATED (near a pixel of one of the two classes);
 *   - a PRISTINE COPY of level 0's reference depth (u16) and the reference's depth factor.  The copy is taken on the
 *     first masking call behind a new reference: a caller who never masks pays nothing.
 * A new reference -- nid_pyr_set_pair_u16, nid_pyr_promote_target_u16, nid_pyr_promote_target -- starts unmasked, the
 * caller's bit included: a caller's mask belongs to the image it was drawn on.
 *
 * THE EFFECTIVE REFERENCE.  Level 0's depth is mask[i] ? 0 : pristine[i]; every coarser level's depth comes from it by the
 * pyramid's own reduction (nid_pyr.h), every level's reference half is set up again from the resident T_wc and reference
 * image.  So a masked pyramid is, byte for byte and bit for bit, the pyramid of the same pair with those depth samples
 * set to 0.  After a masking call every level is in the state a promotion leaves: it has a reference and no reference
 * stage (nid_compute_href per level, or nid_pyr_multistart_lm, which runs it).  The calls open and close like the frame
 * operations of nid_pyr_stream.h: NID_ERR_STATE and nothing changed while a level has an uncollected launch; one stream,
 * one synchronisation.  The public slots are not touched.
 *
 * THE RULE of nid_pyr_mask_occluded / nid_refmask_host (csrc/nid_depth_check.h: ONE text, compiled for the device and for
 * the host; IEEE + - * /, comparisons and floor, no contraction).  For every pixel (r, c) of level 0, in image order:
 *   1. z = (double)pristine[r cols + c] * factor0; z < 0.01 || z > 100: the pixel is not valid and gets no class.
 *      Otherwise n_valid++ and the pixel's point is the set-up's back-projection, operation for operation:
 *      x0 = z (c - cx) / fx, y0 = z (r - cy) / fy, X = T[0] x0 + T[4] y0 + T[8] z + T[12] (summed left to right), Y and Z
 *      likewise from rows 1 and 2 of the column-major T_wc.  The point comes from the PRISTINE depth: a pixel that is
 *      masked now is classified again, and pixels that belong to no cell are classified too.
 *   2. steps 2 - 5 of nid_keyframe.h for (X, Y, Z) against the target depth with tol_abs and tol_rel give the class:
 *      not in view, no target depth, consistent, occluded or through.
 *   3. byte = old & (accumulate ? 15 : NID_REFMASK_CALLER); occluded and (classes & 2): byte |= 2; through and
 *      (classes & 4): byte |= 4.
 *   4. with S the set of pixels whose byte now carries bit 2 or 4: a pixel of S loses bit 8; a pixel outside S gets bit 8
 *      iff dilate > 0 and a pixel of S lies within Chebyshev distance dilate of it (the window is clipped at the image),
 *      and otherwise keeps the bit 8 it had (which step 3 left only under accumulate).
 * The counts are over the final plane: n_caller, n_occluded, n_through, n_dilated the pixels that carry the bit, n_masked
 * the VALID pixels with a non-zero byte.  Everything is an integer: the device and the host give the same.
 *
 * THE TRACKER.  nid_track_set_masking(classes, dilate); classes == 0 is off and the default, and then the tracker is
 * nid_keyframe.h's, call for call.  With masking on AND an active policy (nid_keyframe.h), a later frame with depth whose
 * step 5d chooses a candidate and does NOT promote gets, between the choice and the move of cur / prev,
 *     5e. nid_pyr_mask_occluded(the chosen pose, P.tol_abs, P.tol_rel, classes, dilate, accumulate = 0)
 * -- the mask is made afresh from every such frame; a pixel an occluder has left comes back.  A promoted frame starts
 * unmasked (the rule above).  REJECTED, LOST and depth-less frames, and every frame under a policy that is not active,
 * leave the mask as it is.  An error of 5e is returned as it is and the poses have not moved.
 * From then on the check's n_ref counts the UNMASKED samples only (the check reads level 0's tiles), so min_overlap is a
 * ratio over what is still in use, and a keyframe that is mostly masked is not promoted for that alone.
 * Step 5e trusts the chosen pose: with verification off (min_consistent == 0) a frame LM loses to a false minimum is
 * masked at that wrong pose, and most of the keyframe can go with it.  Use masking with verification on.
 *
 * Out of scope: masks on the target (they would have to reach into the evaluation kernels' pixel loops), cell shards,
 * masks on several devices, a mask plane on the coarser levels.
 */
#ifndef NID_REFMASK_H
#define NID_REFMASK_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_keyframe.h"
#include "nid/nid_pyr.h"
#include "nid/nid_pyr_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NID_REFMASK_CALLER 1
#define NID_REFMASK_OCCLUDED 2
#define NID_REFMASK_THROUGH 4
#define NID_REFMASK_DILATED 8
#define NID_REFMASK_MAX_DILATE 8

typedef struct {
  int64_t n_valid;    /* pixels whose pristine depth is valid */
  int64_t n_caller, n_occluded, n_through, n_dilated; /* pixels of the final plane that carry the bit */
  int64_t n_masked;   /* valid pixels with a non-zero byte: the samples the mask takes out of the evaluation */
  int64_t reserved[2]; /* 0 */
} nid_refmask_counts; /* 64 bytes */

/* ---- on a nid_pyr ------------------------------------------------------------------------------------------------------
 * Argument errors (NID_ERR_INVALID_ARG) are reported before any device is touched.  NID_ERR_STATE, and nothing changed,
 * without a reference or while a level has an uncollected launch; nid_pyr_mask_occluded -- the one call that reads it --
 * also without a target depth (nid_pyr_set_target_depth_u16). */

/* Bit 1 of every pixel from mask[i] != 0 (rows x cols of level 0), the derived bits 2, 4 and 8 cleared, the reference
 * rebuilt. */
int nid_pyr_set_reference_mask_u8(nid_pyr *p, const uint8_t *mask);

/* THE RULE at the head of this file for pose7 (world -> camera) against the resident target depth, then the rebuild.
 * classes: a subset of 2 | 4; dilate: 0 ... NID_REFMASK_MAX_DILATE; accumulate: 0 clears the derived bits first, any other
 * value keeps them; a tolerance negative or not finite is an argument error.  out may be NULL. */
int nid_pyr_mask_occluded(nid_pyr *p, const double *pose7, double tol_abs, double tol_rel, int classes, int dilate,
                          int accumulate, nid_refmask_counts *out);

/* Every bit to 0 and the reference rebuilt: the never-masked pyramid's bits on every level.  A no-op returning NID_OK when
 * no byte of the plane is set (the reference stage then stays too). */
int nid_pyr_clear_reference_mask(nid_pyr *p);

/* The plane as the device holds it (zeros behind a new reference). */
int nid_pyr_get_reference_mask_u8(nid_pyr *p, uint8_t *out);

/* The same text compiled for the host: one call of THE RULE on mask_inout (rows x cols, the plane before / after).  cfg:
 * rows, cols and the intrinsics of level 0; depth0_u16 / factor0 / T_wc_colmajor16: the keyframe's pristine depth, its
 * factor and camera -> world matrix; depth1_u16 / factor1: the target's depth.  counts may be NULL.  Never touches a
 * device.  NID_ERR_INVALID_ARG for a null pointer, rows or cols < 1, classes, dilate or a tolerance out of range. */
int nid_refmask_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *T_wc_colmajor16,
                     const uint16_t *depth1_u16, double factor1, const double *pose7, double tol_abs, double tol_rel,
                     int classes, int dilate, int accumulate, uint8_t *mask_inout, nid_refmask_counts *counts);

/* ---- the tracker ------------------------------------------------------------------------------------------------------- */
/* classes: a subset of 2 | 4, 0 = off (the default); dilate: 0 ... NID_REFMASK_MAX_DILATE. */
int nid_track_set_masking(nid_track *t, int classes, int dilate);
/* Of the last push that returned NID_OK: the counts of its step 5e, zeros if it ran none. */
int nid_track_last_mask(const nid_track *t, nid_refmask_counts *counts);

#ifdef __cplusplus
}
#endif
#endif

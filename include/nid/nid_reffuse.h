/*
 * nid_reffuse.h -- the VALID depth samples of the REFERENCE (the keyframe) of the resident pyramid of nid_pyr.h refined from
 * tracked frames, and the tracker's use of it (libnid_hip.so).  nid_reffill.h gives a keyframe depth where it has none;
 * where it has a sample, that sample stays what the sensor delivered in one shot for as long as the keyframe lives, and
 * its noise is geometry noise in every evaluation of every later frame.  Every frame tracked on the keyframe with depth
 * measures the same surfaces again: a fusion averages those measurements into the keyframe's own.
 *
 * WHAT A FUSION IS.  A rebuild of the reference set-up from a changed level-0 depth plane; no evaluation kernel knows of
 * it.  The state lives at level 0 only and belongs to the resident reference; the first fusion behind a new reference makes
 * it, and a caller who never fuses pays nothing:
 *   - a SUM plane, u32, rows x cols: S, the sum of the fused observations of a pixel, in counts of the reference's depth
 *     factor;
 *   - an OBS plane, u8: k, the number of fused observations, 0 ... max_obs;
 *   - a FUSED plane, u16: 0 -- not refined (k == 0); any other value -- the refined count e below;
 *   - the UPLOADED COPY of nid_reffill.h, made together with a zero fill plane by whichever of the first fill or the first
 *     fusion behind a new reference comes first.
 * With u the uploaded count of a pixel,
 *     e = (2 (u + S) + (k + 1)) / (2 (k + 1))   in integer division:
 * the round-half-up mean of the sensor's own sample and the fused ones; k == 0 gives e == u; the numerator stays below
 * 2^26 (k <= 255 and every observation <= 65535).  e lies between the smallest and the largest of its k + 1 observations,
 * all of which are counts of valid depths, and the validity test is an interval of counts: e is a valid depth.
 * The BASE depth is fused ? fused : uploaded.  The PRISTINE depth of nid_refmask.h becomes fill ? fill : base, the
 * effective level-0 depth mask ? 0 : (fill ? fill : base); everything behind level 0's depth plane is the masking calls'
 * chain, unchanged.  So a refined pyramid is, byte for byte and bit for bit, the pyramid of the same pair with the refined
 * samples written into its depth map.  A new reference -- nid_pyr_set_pair_u16 and both promotions -- starts unfused.  A
 * fusion call opens and closes like a fill call: NID_ERR_STATE and nothing changed without a reference or while a level has
 * an uncollected launch; one stream, one synchronisation; every level left as a promotion leaves it; the mask plane and the
 * fill plane stay byte for byte; no slot is touched and no evaluation kernel is launched.
 *
 * THE RULE of nid_pyr_fuse_reference_depth / nid_reffuse_host (csrc/nid_reffuse_rule.h: ONE text, compiled for the device
 * and for the host on the terms of csrc/nid_reffill_rule.h, which it includes and reuses).
 *   A. SPLAT.  Parts A.1 - 6 of nid_reffill.h as they are: the matrix M, the target's pixels into the keyframe's u32
 *      z-buffer, the minimum.  n_target_valid, n_splat and n_hit have the fill's meanings.
 *   B. FUSE, in integers, for every keyframe pixel with uploaded count u.  u invalid: nothing happens -- holes and their
 *      fills are nid_reffill.h's business --, fused = 0, S and k untouched.  Otherwise n_valid++, and if the pixel was hit
 *      with count q:
 *        k >= max_obs                                               n_saturated++, nothing else;
 *        |q - u| 1024 <= gate_abs 1024 + gate_rel_1024 u  (64 bit)  S += q, k += 1, n_fused++;
 *        else                                                       n_gated++.
 *      Then fused = k ? e : 0, and n_changed counts the pixels whose BASE value differs from the one before the call.
 * The gate is taken against the UPLOADED count, not against the running mean: every accepted observation lies within the
 * gate of the sensor's own sample, so e never leaves that gate (of the widest gate used on the pixel), and a chain of wrong
 * poses cannot walk a depth away.  The gate is also what rejects hits from another surface: occluders, and a forward
 * splat's leak through a nearer surface's sampling gaps.  The splat is to the nearest pixel: on a slanted surface the
 * observation is the depth up to half a pixel away; that error is accepted here.
 * Everything is an integer and a minimum does not depend on order: the device and the host give the same planes and counts.
 *
 * THE FILL READS BASE.  Once a fusion state exists, nid_pyr_fill_reference_depth takes the BASE plane where it took the
 * uploaded copy -- for the guard's surfaces and for pristine = fill ? fill : base -- and nid_pyr_clear_reference_fill copies
 * BASE back: a fill on a fused pyramid is nid_reffill_host with depth0 = where(fused, fused, uploaded).  Without a fusion
 * nothing changes.  For the same target depth and pose, fill-then-fuse and fuse-then-fill leave the same planes: the fusion
 * changes BASE only at hit pixels, where the guard's surface is the z-buffer's entry either way; it never touches holes,
 * and the fill never touches valid pixels.
 *
 * THE TRACKER.  nid_track_set_fusing(on, gate_abs, gate_rel_1024, max_obs); off is the default, and then the tracker is
 * nid_reffill.h's, call for call.  With fusing on AND an active policy (nid_keyframe.h), a later frame with depth whose
 * step 5d chooses a candidate and does NOT promote gets, after the fill (step 5d', if on) and before step 5e's mask,
 *     5d''. nid_pyr_fuse_reference_depth(the chosen pose, gate_abs, gate_rel_1024, max_obs)
 * REJECTED, LOST, depth-less and promoted frames run no fusion; a promoted frame starts unfused.  An error is returned as it
 * is and the poses have not moved.
 * A fusion trusts the chosen pose as a fill does: with verification off (min_consistent == 0) a frame LM loses to a false
 * minimum is averaged into the keyframe at that wrong pose wherever it passes the gate.  Use fusing with verification on
 * (min_consistent > 0).  And an observation is only as good as the pose and the splat that bring it: it carries the pose's
 * error along the viewing ray and, on a surface whose depth changes by s counts per pixel, up to s / 2 counts from the
 * nearest-pixel splat.  Where those exceed the sensor's noise a fusion makes the keyframe's depth worse, not better
 * (profiles/reffuse_cost.txt has such a sequence); the gate bounds the damage, it does not prevent it.
 *
 * A bilinear sample of the target's depth where the keyframe pixel projects, in the place of the nearest-pixel splat, is
 * nid_refgather.h's: the same state, gate and cap, another source of the observation.
 *
 * Out of scope: refining fills (only sensor-valid pixels are refined), confidence weights beyond the observation cap, one
 * shared splat and rebuild for a frame's fill, fusion and mask (today three chains), cell shards, several devices, planes on
 * the coarser levels.
 */
#ifndef NID_REFFUSE_H
#define NID_REFFUSE_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_pyr.h"
#include "nid/nid_pyr_stream.h"
#include "nid/nid_reffill.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NID_REFFUSE_MAX_OBS 255

typedef struct {
  int64_t n_target_valid; /* target pixels with a valid depth */
  int64_t n_splat;        /* ... of them, those that reached the z-buffer */
  int64_t n_hit;          /* keyframe pixels with a z-buffer entry */
  int64_t n_valid;        /* keyframe pixels whose uploaded depth is valid */
  int64_t n_fused;        /* ... of them, hit within the gate below the cap: an observation more */
  int64_t n_gated;        /* ... hit outside the gate */
  int64_t n_saturated;    /* ... hit with max_obs observations already */
  int64_t n_changed;      /* pixels whose BASE value differs from the one before the call */
} nid_reffuse_counts; /* 64 bytes */

/* ---- on a nid_pyr ------------------------------------------------------------------------------------------------------
 * Argument errors (NID_ERR_INVALID_ARG) are reported before any device is touched: a null handle or pointer, gate_abs
 * outside 0 ... 65535, gate_rel_1024 outside 0 ... 1024, max_obs outside 1 ... NID_REFFUSE_MAX_OBS.  NID_ERR_STATE, and nothing
 * changed, without a reference or while a level has an uncollected launch; nid_pyr_fuse_reference_depth -- the one call
 * that reads it -- also without a target depth (nid_pyr_set_target_depth_u16). */

/* THE RULE at the head of this file for pose7 (world -> camera, the target's) against the resident target depth, then the
 * rebuild.  out may be NULL. */
int nid_pyr_fuse_reference_depth(nid_pyr *p, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs, nid_reffuse_counts *out);

/* S, k and fused to 0, BASE back to uploaded and the reference rebuilt: the bits of the never-fused pyramid with the same
 * fill and mask.  A no-op returning NID_OK when nothing is fused (the reference stage then stays too). */
int nid_pyr_clear_reference_fusion(nid_pyr *p);

/* The FUSED and the OBS plane as the device holds them (zeros behind a new reference). */
int nid_pyr_get_reference_fused_u16(nid_pyr *p, uint16_t *out);
int nid_pyr_get_reference_fusion_obs_u8(nid_pyr *p, uint8_t *out);

/* The same text compiled for the host: one call of THE RULE on sum_inout / obs_inout (rows x cols each, the planes before /
 * after); fused_out (rows x cols) is written.  cfg, depth0_u16 (the UPLOADED depth), factor0, T_wc_colmajor16, depth1_u16,
 * factor1, pose7: as nid_reffill_host's.  counts may be NULL.  Never touches a device.  NID_ERR_INVALID_ARG for a null
 * pointer, rows or cols < 1, rows x cols above INT32_MAX, a gate or cap out of range, or planes that no sequence of calls
 * leaves: a pixel with sum_inout > 65535 obs_inout. */
int nid_reffuse_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *T_wc_colmajor16,
                     const uint16_t *depth1_u16, double factor1, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs,
                     uint32_t *sum_inout, uint8_t *obs_inout, uint16_t *fused_out, nid_reffuse_counts *counts);

/* ---- the tracker ------------------------------------------------------------------------------------------------------- */
/* on: 0 = off (the default); the gate and the cap as above (checked also when on is 0). */
int nid_track_set_fusing(nid_track *t, int on, int gate_abs, int gate_rel_1024, int max_obs);
/* Of the last push that returned NID_OK: the counts of its fusion, zeros if it ran none. */
int nid_track_last_fusion(const nid_track *t, nid_reffuse_counts *counts);

#ifdef __cplusplus
}
#endif
#endif

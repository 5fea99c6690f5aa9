/*
 * nid_refgather.h -- a second source of observations for the fusion of nid_reffuse.h (libnid_hip.so): the target's depth
 * SAMPLED BILINEARLY where a keyframe pixel projects, instead of splatted forward to the nearest keyframe pixel.
 * nid_reffuse.h's observation is the target's depth up to half a pixel away; on a surface whose depth changes by s counts
 * per pixel that is a bias of up to s / 2 counts, which the gate bounds and the mean does not remove
 * (profiles/reffuse_cost.txt).  Here each valid keyframe pixel is projected into the target at the pose, the target's depth
 * is interpolated there between its four neighbours, and the sampled point is brought back into the keyframe: projective
 * data association.
 *
 * WHAT STAYS.  The state of nid_reffuse.h -- the SUM plane S, the OBS plane k, FUSED, BASE --, the refined count e, the
 * gate against the uploaded count, the cap, the rebuild behind level 0 and the composition with the fill and the mask.
 * Only where the observation q of a pixel comes from is new.  A gather needs no z-buffer, no atomics on the planes and no
 * 0xFF fill: a call is ONE kernel in front of the masking calls' chain where a fusion has two and a memset.  Nearest-splat
 * and bilinear observations may be mixed on one keyframe: they share S, k and the cap, and
 * nid_pyr_clear_reference_fusion, nid_pyr_get_reference_fused_u16 and nid_pyr_get_reference_fusion_obs_u8 serve both.
 *
 * THE RULE of nid_pyr_fuse_reference_depth_bilinear / nid_refgather_host (csrc/nid_refgather_rule.h: ONE text, compiled
 * for the device and for the host on the terms of csrc/nid_reffill_rule.h and csrc/nid_reffuse_rule.h, which it includes
 * and reuses: IEEE + - * / on doubles, comparisons, floor and integer arithmetic, no contraction).  K: the twelve doubles
 * of [R|t] keyframe camera -> target camera, M: target camera -> keyframe camera (parts A.1 of nid_reffill.h), both made
 * once per call on the host.  For keyframe pixel (r, c) with uploaded count u:
 *   G.0  u is not a valid depth: nothing happens -- holes stay nid_reffill.h's business --, S and k untouched, fused = 0.
 *        Otherwise n_valid++.
 *   G.1  zk = u factor0; x = zk (c - cx) / fx, y = zk (r - cy) / fy.  The UPLOADED count, not BASE: where a pixel looks
 *        does not depend on what was fused before.
 *   G.2  xt = ((K[0] x + K[1] y) + K[2] zk) + K[3], yt and zt likewise.  !(zt > 0): n_outside++, no observation.
 *   G.3  ut = (fx xt) / zt + cx, vt = (fy yt) / zt + cy; c0 = floor(ut), r0 = floor(vt).  Unless 0 <= c0 <= cols - 2 and
 *        0 <= r0 <= rows - 2 (NaN and the infinities fail): n_outside++.  a = ut - c0, b = vt - r0.
 *   G.4  the taps t00, t01, t10, t11: the target's depth at rows r0, r0 + 1 and columns c0, c0 + 1.  One of them not a
 *        valid depth: n_tap_refused++.  Their spread, in 64-bit integers:
 *            (max - min) 1024 <= tap_abs 1024 + tap_rel_1024 min,   else n_tap_refused++.
 *        This is what keeps a sample from being interpolated across a depth edge.
 *   G.5  top = t00 + a (t01 - t00), bot = t10 + a (t11 - t10), zo = (top + b (bot - top)) factor1, in doubles, in this order.
 *   G.6  the sampled point on the target's ray through (ut, vt): xo = zo (ut - cx) / fx, yo = zo (vt - cy) / fy; its
 *        keyframe depth zk' = ((M[8] xo + M[9] yo) + M[10] zo) + M[11]; qd = floor(zk' / factor0 + 0.5).  Unless
 *        1 <= qd <= 65535 and the count is a valid depth: n_outside++.  Else n_sampled++: the pixel has the observation q.
 *   B.   Part B of nid_reffuse.h as it is, on q or on no hit: the cap before the gate, the gate against the uploaded
 *        count, e, FUSED, BASE, n_fused / n_gated / n_saturated / n_changed.
 * So n_valid = n_sampled + n_outside + n_tap_refused and n_sampled = n_fused + n_gated + n_saturated.  A pixel's new state
 * hangs on its own entries and on the target's depth alone: the device and the host give the same planes and counts.
 *
 * WHAT IS ACCEPTED.
 *   - The sampled point lies on the TARGET's ray through (ut, vt), not on the keyframe pixel's: where zo differs from the
 *     keyframe's own depth it projects beside the pixel, by the parallax of that depth difference.  The error is second
 *     order in the baseline (the difference times the baseline over the depth) and is accepted.
 *   - A target pixel that shows another surface -- an occluder in front of the keyframe's, or what a disocclusion
 *     uncovers -- gives a q far from u.  That is the gate's business, as in a fusion.
 *   - A keyframe pixel that projects onto the target's last row or last column gets no observation (c0 <= cols - 2,
 *     r0 <= rows - 2: the four taps are always inside the image).
 *   - The interpolation is of depth along the target's rays, linear in the image: exact on a plane only to first order.
 *
 * FILL AND GATHER DO NOT COMMUTE in general, unlike fill and fusion: a gather moves BASE at pixels the fill's z-buffer did
 * not hit, and the fill's guard reads BASE there.  What holds is nid_reffuse.h's "the fill reads BASE": a fill behind a
 * gather is nid_reffill_host with depth0 = where(fused, fused, uploaded).
 *
 * THE TRACKER.  nid_track_set_fusion_sampling(mode, tap_abs, tap_rel_1024): NID_REFFUSE_NEAREST is the default, and then
 * the tracker is nid_reffuse.h's, call for call.  With NID_REFFUSE_BILINEAR, step 5d'' of a frame that fuses
 * (nid_track_set_fusing on) runs
 *     nid_pyr_fuse_reference_depth_bilinear(the chosen pose, nid_track_set_fusing's gate and cap, tap_abs, tap_rel_1024)
 * in the place of nid_pyr_fuse_reference_depth; nid_track_last_fusion then reads zeros and nid_track_last_gather the counts.
 * Nothing about how the tracker finds its poses changes: an observation is still only as good as the pose that brings it
 * (profiles/refgather_cost.txt).
 *
 * Out of scope: refining fills, weights beyond the cap, normals or slope-aware gates, one shared rebuild for a frame's
 * fill, fusion and mask, cell shards, several devices, planes on the coarser levels.
 */
#ifndef NID_REFGATHER_H
#define NID_REFGATHER_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_pyr.h"
#include "nid/nid_pyr_stream.h"
#include "nid/nid_reffuse.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NID_REFFUSE_NEAREST 0  /* step 5d'' splats: nid_pyr_fuse_reference_depth */
#define NID_REFFUSE_BILINEAR 1 /* step 5d'' gathers: nid_pyr_fuse_reference_depth_bilinear */

typedef struct {
  int64_t n_valid;       /* keyframe pixels whose uploaded depth is valid */
  int64_t n_sampled;     /* ... of them, those with an observation (G.6) */
  int64_t n_outside;     /* ... behind the target, off its frame or on its last row or column, or sampled out of range */
  int64_t n_tap_refused; /* ... with an invalid tap or taps spread beyond the tap gate */
  int64_t n_fused;       /* sampled within the gate below the cap: an observation more */
  int64_t n_gated;       /* sampled outside the gate */
  int64_t n_saturated;   /* sampled with max_obs observations already */
  int64_t n_changed;     /* pixels whose BASE value differs from the one before the call */
} nid_refgather_counts; /* 64 bytes */

/* Argument errors (NID_ERR_INVALID_ARG) are reported before any device is touched: a null handle or pointer, gate_abs or
 * tap_abs outside 0 ... 65535, gate_rel_1024 or tap_rel_1024 outside 0 ... 1024, max_obs outside 1 ... NID_REFFUSE_MAX_OBS. */

/* THE RULE at the head of this file for pose7 (world -> camera, the target's) against the resident target depth, then the
 * rebuild.  NID_ERR_STATE, and nothing changed, under nid_pyr_fuse_reference_depth's conditions: no reference, no target
 * depth, a level with an uncollected launch.  Opens and closes as that call does: one stream, one synchronisation, the mask
 * and the fill plane byte for byte, no slot touched, no evaluation kernel launched.  out may be NULL. */
int nid_pyr_fuse_reference_depth_bilinear(nid_pyr *p, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs, int tap_abs,
                                          int tap_rel_1024, nid_refgather_counts *out);

/* The same text compiled for the host: nid_reffuse_host's arguments, checks and planes, and the two tap arguments.  Never
 * touches a device. */
int nid_refgather_host(const nid_config *cfg, const uint16_t *depth0_u16, double factor0, const double *T_wc_colmajor16,
                       const uint16_t *depth1_u16, double factor1, const double *pose7, int gate_abs, int gate_rel_1024, int max_obs,
                       int tap_abs, int tap_rel_1024, uint32_t *sum_inout, uint8_t *obs_inout, uint16_t *fused_out,
                       nid_refgather_counts *counts);

/* ---- the tracker ------------------------------------------------------------------------------------------------------- */
/* mode: NID_REFFUSE_NEAREST (the default) or NID_REFFUSE_BILINEAR; the tap gate as above (checked in either mode). */
int nid_track_set_fusion_sampling(nid_track *t, int mode, int tap_abs, int tap_rel_1024);
/* Of the last push that returned NID_OK: the counts of its gather, zeros if it ran none. */
int nid_track_last_gather(const nid_track *t, nid_refgather_counts *counts);

#ifdef __cplusplus
}
#endif
#endif

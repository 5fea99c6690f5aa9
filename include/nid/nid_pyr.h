/*
 * nid_pyr.h -- a device-built, resident image pyramid and coarse-to-fine multi-start LM on it (libnid_hip.so).
 *
 * A nid_pyr owns one nid_ctx per pyramid level, all on one device.  nid_pyr_set_pair_u16 uploads level 0 once (what
 * nid_set_pair_u16 uploads), makes every coarser level ON THE DEVICE (k_pyr_down: the arithmetic of
 * host/nid_pyramid.cpp -- 2x2 box mean of the images rounded half up, mean of the VALID depth samples rounded half up
 * in u16 counts, 0 if none is valid -- so the levels are the host route's, byte for byte) and runs every level's
 * back-projection, tiling and target margins.  Every level stays resident; a level context is an ordinary nid_ctx
 * (nid_pyr_level) in the state nid_set_reference_depth + nid_set_target_u8 leave: the reference stage
 * (nid_compute_href) is the caller's, at the pose the level starts from.
 *
 * nid_pyr_multistart_lm is a composition of public calls, stated exactly so that it can be restated and compared bit
 * for bit: for level l = levels-1 (coarsest) down to 0
 *   1. nid_compute_href on level l's context at the level's reference pose: on the coarsest level pose_ref7 (NULL:
 *      start 0), on every finer level the start pose of that level's first chain;
 *   2. nid_multistart_lm on level l's context from the level's start poses, with `iterations`, huber_delta,
 *      max_rounds = 0, no trace;
 *   3. the chains with finite chi2 and n_active > 0, ranked by chi2 / n_active ascending (the lower index winning
 *      ties: the rule of *best in nid_multistart.h); the first keep[l-1] of them -- fewer if fewer are eligible --
 *      start level l-1 from their result poses, in rank order.
 * No eligible chain on a level: the call ends there with NID_OK and *best_origin = -1.
 *
 * Out of scope: cell shards (cfg0 must own all cells), levels on different devices, a device-side selection of the
 * survivors (a handful of comparisons on the host between two blocking calls), and a reference stage inside
 * nid_pyr_set_pair_u16.
 *
 * Frame streams on the same object -- a new target alone, the target promoted to the reference, a tracker -- are a header
 * of their own: nid/nid_pyr_stream.h.
 */
#ifndef NID_PYR_H
#define NID_PYR_H

#include <stdint.h>

#include "nid/nid_c.h"
#include "nid/nid_multistart.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nid_pyr nid_pyr;
#define NID_PYR_MAX_LEVELS 8

/* Geometry of level `level` (0 = cfg0 itself): per level rows / 2, cols / 2, cell_num / 2, fx / 2, fy / 2,
 * (cx - 0.5) / 2, (cy - 0.5) / 2 -- the operations of host/nid_pyramid.cpp in its order --, everything else copied.
 * Pure arithmetic: never touches a device.  NID_ERR_INVALID_ARG for a null pointer, level outside 0 ... 7, rows, cols
 * or cell_num not divisible by 2^level, a level with cell_num < 1, or a cfg0 that does not own all cells
 * (cell_begin / cell_end other than 0, 0). */
int nid_pyr_level_config(const nid_config *cfg0, int level, nid_config *out);

/* One nid_ctx per level (nid_create of nid_pyr_level_config), all on cfg0->device.  NID_ERR_INVALID_ARG for a null
 * pointer, levels outside 1 ... NID_PYR_MAX_LEVELS or a cfg0 nid_pyr_level_config refuses for level levels-1 -- all
 * checked before any device is touched; then whatever nid_create returns (NID_ERR_NO_DEVICE without a device). */
int nid_pyr_create(const nid_config *cfg0, int levels, nid_pyr **out);
int nid_pyr_destroy(nid_pyr *p);
int nid_pyr_levels(const nid_pyr *p);
/* Level `level`'s context (NULL: no such level).  Owned by the pyramid: never nid_destroy it.  Options set on it
 * (nid_set_options, nid_set_math_mode, nid_set_launch_shape) are the caller's and survive nid_pyr_set_pair_u16. */
nid_ctx *nid_pyr_level(nid_pyr *p, int level);

/* Level 0 uploaded once (what nid_set_pair_u16 uploads); every coarser level built on the device; every level's
 * back-projection, tiles and target margins made.  NO reference stage: afterwards each level context is in the state
 * nid_set_reference_depth + nid_set_target_u8 leave (href not set).  Everything is enqueued on ONE stream (level 0's)
 * with one synchronisation at the end, before any level is marked ready.  NID_ERR_STATE while a level context has an
 * uncollected launch; an error leaves every level without a pair. */
int nid_pyr_set_pair_u16(nid_pyr *p, const uint16_t *depth_u16, double depth_factor, const uint8_t *im0,
                         const uint8_t *im1, const double *T_wc0_colmajor16);

/* A level's inputs as the device holds them (tests, debugging): rows x cols of that level each; any pointer may be
 * NULL.  NID_ERR_STATE before the first nid_pyr_set_pair_u16. */
int nid_pyr_get_level_inputs(nid_pyr *p, int level, uint16_t *depth_u16, uint8_t *im0, uint8_t *im1);

/* Coarse-to-fine multi-start LM: the schedule at the head of this file.  poses7_in: n x 7, 1 <= n <= NID_MAX_BATCH.
 * keep[levels] (NULL: n on every level): keep[l] chains start on level l; keep[levels-1] == n and
 * 1 <= keep[l] <= keep[l+1].  results and origin: levels x n, coarsest level first -- results[(levels-1-l) * n + k]
 * is chain k of level l, origin[...] its index into poses7_in; unused rows are zero / -1.  rounds[levels] (may be
 * NULL): the rounds nid_multistart_lm took per level, coarsest first.  *best_origin / best_pose7[7] (may be NULL):
 * origin and pose of level 0's best chain by the ranking above; -1 and untouched if a level had no eligible chain.
 * Blocking.  The public slots of the level contexts are not touched.  Errors as nid_multistart_lm's. */
int nid_pyr_multistart_lm(nid_pyr *p, const double *poses7_in, int n, const double *pose_ref7, int iterations,
                          double huber_delta, const int32_t *keep, nid_ms_result *results, int32_t *origin,
                          int32_t *rounds, int *best_origin, double *best_pose7);

#ifdef __cplusplus
}
#endif
#endif

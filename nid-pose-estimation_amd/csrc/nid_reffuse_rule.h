// nid_reffuse_rule.h -- the rule of the reference fusion (include/nid/nid_reffuse.h) on the terms of nid_reffill_rule.h, which
// it includes and whose part A it reuses as it is (rf::target_to_keyframe, rf::make_splat, rf::splat, the u32 z-buffer's
// minimum): the ONE definition the device (k_reffuse_apply in nid_setup_kernels.hip.h, behind k_reffill_splat) and the host
// (rfu::reffuse_host behind nid_reffuse_host) are compiled from -- the refined count, the gate's comparison, a pixel's new
// state and its counts.
//
// Part B is integer arithmetic alone; part A's agreement is nid_reffill_rule.h's (-ffp-contract=off, no fast-math).  No
// HIP-only construct: a plain C++ translation unit can include this file (tests/cpp/reffuse_check.cpp, under the host
// sanitizers: no conversion or index here is reachable out of range).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "nid/nid_reffuse.h"
#include "nid_reffill_rule.h"

namespace nid {
namespace rfu {

// e: the round-half-up mean of the uploaded count u and the k fused observations whose sum is S.  S <= 65535 k and
// k <= 255 keep the numerator below 2^26; k == 0 gives u
NID_DC_HD uint32_t refined(uint16_t u, uint32_t S, uint32_t k) { return (2u * ((uint32_t)u + S) + (k + 1u)) / (2u * (k + 1u)); }

// a hit of count q lies within the gate of the uploaded count u (64-bit integers)
NID_DC_HD bool within(uint32_t q, uint16_t u, int gate_abs, int gate_rel_1024) {
  const int64_t d = (int64_t)q - (int64_t)u;
  return (d < 0 ? -d : d) * 1024 <= (int64_t)gate_abs * 1024 + (int64_t)gate_rel_1024 * (int64_t)u;
}

// a state no sequence of calls leaves (nid_reffuse_host refuses it: refined()'s numerator is sized for the others)
NID_DC_HD bool state_ok(uint32_t S, uint32_t k) { return S <= 65535u * k; }

// Part B for one keyframe pixel, counted: *S and *k before / after; *base: the pixel's BASE count behind the call (fused or
// uploaded).  Returns the FUSED plane's entry.  z: the z-buffer's entry (rf::kNone: not hit)
NID_DC_HD uint16_t fuse(bool uploaded_valid, uint16_t u, uint32_t z, int gate_abs, int gate_rel_1024, int max_obs, uint32_t *S, uint8_t *k,
                        uint16_t *base, nid_reffuse_counts *n) {
  const bool hit = z != rf::kNone;
  n->n_hit += hit;
  *base = u;
  if (!uploaded_valid) return 0;  // (a hole: nid_reffill.h's business)
  n->n_valid++;
  uint32_t s = *S, kk = *k;
  const uint32_t before = refined(u, s, kk);
  if (hit) {
    if (kk >= (uint32_t)max_obs) n->n_saturated++;
    else if (within(z, u, gate_abs, gate_rel_1024)) {
      s += z;  // (a z-buffer entry is a count of step A.5: 1 ... 65535)
      kk++;
      n->n_fused++;
    } else n->n_gated++;
  }
  const uint32_t e = refined(u, s, kk);  // (between the smallest and the largest of its observations: a count)
  n->n_changed += e != before;
  *S = s;
  *k = (uint8_t)kk;  // (kk <= max_obs <= 255, or the caller's own k)
  *base = (uint16_t)e;
  return kk ? (uint16_t)e : (uint16_t)0;
}

NID_DC_HD bool args_ok(int gate_abs, int gate_rel_1024, int max_obs) {
  return gate_abs >= 0 && gate_abs <= 65535 && gate_rel_1024 >= 0 && gate_rel_1024 <= 1024 && max_obs >= 1 && max_obs <= NID_REFFUSE_MAX_OBS;
}

// nid_reffuse_host behind its argument checks: THE RULE over the whole plane, in place.  d0: the keyframe's uploaded depth;
// zbuf: rows x cols words of the caller's, overwritten; base: rows x cols of the caller's or null.
inline void reffuse_host(const rf::Splat &S, const uint16_t *d0, int gate_abs, int gate_rel_1024, int max_obs, uint32_t *sum, uint8_t *obs,
                         uint16_t *fused, uint16_t *base, uint32_t *zbuf, nid_reffuse_counts *counts) {
  const size_t N = (size_t)S.rows * (size_t)S.cols;
  nid_reffuse_counts n = {};
  rf::splat_host(S, zbuf, &n.n_target_valid, &n.n_splat);  // A.
  for (size_t i = 0; i < N; i++) {
    uint16_t b = 0;
    fused[i] = fuse(dc::depth_valid(d0[i], S.factor0), d0[i], zbuf[i], gate_abs, gate_rel_1024, max_obs, sum + i, obs + i, &b, &n);
    if (base) base[i] = b;
  }
  if (counts) *counts = n;
}

}  // namespace rfu
}  // namespace nid

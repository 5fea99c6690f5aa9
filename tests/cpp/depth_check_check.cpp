// The per-sample rule of the depth-consistency check and the tracker's two decisions (csrc/nid_depth_check.h: plain
// arithmetic, no HIP) in a program of their own.  Built with -fsanitize=address,undefined,float-cast-overflow by
// tests/test_keyframe_cpu.py.  Exit code 0: all as expected.
//
// 1. The rule over LCG inputs in which every quantity -- point, pose matrix, intrinsics, factor, tolerances -- is now and
//    then +-inf, NaN, +-1e300 or a subnormal: whatever comes in, no conversion to an integer and no index may be out of
//    range (the sanitizers say so), and the counts keep their invariants: n_ref >= n_inframe >= n_both = consistent +
//    occluded + through.
// 2. The decision functions against tables written by hand.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "nid_depth_check.h"

namespace {

uint64_t g_state = 20240611ull;
uint64_t next_u64() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return g_state >> 11;
}
double uniform() { return (double)next_u64() * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }  // [-1, 1)

int g_special = 0;
// an ordinary value of the given scale, or -- one time in `one_in` -- one of the special ones
double draw(double scale, int one_in, bool *special) {
  static const double kSpecial[] = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                                    std::numeric_limits<double>::quiet_NaN(), 1e300, -1e300, 4.9e-324, -4.9e-324, 2.2e-308 / 4, 0.0, -0.0};
  if (next_u64() % (uint64_t)one_in == 0) {
    *special = true;
    return kSpecial[next_u64() % (sizeof(kSpecial) / sizeof(kSpecial[0]))];
  }
  return uniform() * scale;
}

int g_failures = 0;
void expect(bool ok, const char *what, int k) {
  if (!ok) { g_failures++; std::printf("FAILED: %s (%d)\n", what, k); }
}

nid_depth_counts counts(int64_t n_ref, int64_t n_inframe, int64_t n_both, int64_t n_consistent) {
  nid_depth_counts c = {};
  c.n_ref = n_ref; c.n_inframe = n_inframe; c.n_both = n_both; c.n_consistent = n_consistent;
  c.n_occluded = n_both - n_consistent;
  return c;
}

}  // namespace

int main() {
  using namespace nid;
  // ---- 1. the rule --------------------------------------------------------------------------------------------------------
  const int rows = 12, cols = 20;
  std::vector<uint16_t> d1((size_t)rows * cols);
  long samples = 0, in_frame = 0, saturated = 0;
  for (int batch = 0; batch < 400; batch++) {
    for (uint16_t &d : d1) d = (uint16_t)(next_u64() % 4 == 0 ? next_u64() % 65536 : 8000 + next_u64() % 4000);
    dc::View V;
    bool sp = false;
    const bool plain = batch % 4 == 0;  // a camera that sees the points: identity-like, so that samples reach step 5
    for (int k = 0; k < 12; k++) V.M[k] = plain ? ((k == 0 || k == 5 || k == 10) ? 1.0 : 0.01 * uniform()) : draw(1.0, 6, &sp);
    V.fx = plain ? 10.0 : draw(20.0, 8, &sp); V.fy = plain ? -10.0 : draw(20.0, 8, &sp);
    V.cx = plain ? 9.5 : draw(20.0, 8, &sp); V.cy = plain ? 5.5 : draw(20.0, 8, &sp);
    V.rows = rows; V.cols = cols; V.d1 = d1.data();
    V.factor = batch % 3 ? 1.0 / 5000 : draw(1.0, 2, &sp);
    V.tol_abs = batch % 5 ? 0.01 : draw(1.0, 2, &sp);
    V.tol_rel = batch % 7 ? 0.02 : draw(1.0, 2, &sp);
    nid_depth_cell a = {};
    for (int s = 0; s < 600; s++) {
      bool sp_point = sp;
      const double X = draw(2.0, 10, &sp_point), Y = draw(1.0, 10, &sp_point), Z = plain && s % 3 ? 1.5 + uniform() : draw(4.0, 10, &sp_point);
      const uint64_t before = a.sum_abs_um;
      dc::sample(V, X, Y, Z, &a);
      if (a.sum_abs_um - before >= ((uint64_t)1 << 63)) saturated++;
      g_special += sp_point;
      samples++;
    }
    in_frame += a.n_inframe;
    expect(a.n_ref <= 600 && a.n_inframe <= a.n_ref && a.n_both <= a.n_inframe, "the counts nest", batch);
    expect(a.n_consistent + a.n_occluded + a.n_through == a.n_both, "every sample with both depths is classified once", batch);
    expect(a.n_consistent > 0 || a.sum_abs_um == 0, "a sum without a consistent sample", batch);
  }
  {  // a |dz| too large for the sum adds 2^63 and converts nothing out of range
    dc::View V = {};
    V.M[0] = V.M[5] = V.M[10] = 1.0;
    V.fx = 10; V.fy = -10; V.cx = 9.5; V.cy = 5.5; V.rows = rows; V.cols = cols; V.d1 = d1.data();
    d1[5 * cols + 9] = 10000; d1[6 * cols + 10] = 10000; d1[5 * cols + 10] = 10000; d1[6 * cols + 9] = 10000;
    V.factor = 1.0 / 5000; V.tol_abs = 1e300; V.tol_rel = 0;
    nid_depth_cell a = {};
    dc::sample(V, 0.0, 0.0, 1e299, &a);
    expect(a.n_consistent == 1 && a.sum_abs_um == (uint64_t)1 << 63, "a saturated sum", 0);
    saturated += a.sum_abs_um == (uint64_t)1 << 63;
    V.factor = std::numeric_limits<double>::quiet_NaN(); V.tol_abs = 0.01;  // zt is NaN: passes the validity test as in k_tile, neither comparison holds
    a = nid_depth_cell();
    dc::sample(V, 0.0, 0.0, 2.0, &a);
    expect(a.n_both == 1 && a.n_consistent == 1 && a.sum_abs_um == (uint64_t)1 << 63, "a NaN factor", 0);
  }

  // ---- 2. the decisions ---------------------------------------------------------------------------------------------------
  int decisions = 0;
  nid_track_policy P = {};
  P.tol_abs = 0.01; P.tol_rel = 0.02;
  expect(dc::policy_valid(P) && !dc::policy_active(P), "the default policy is valid and not active", 0);
  {
    // the choice: {n_ref, n_inframe, n_both, n_consistent}
    const nid_depth_counts list[4] = {counts(1000, 900, 800, 399), counts(1000, 900, 40, 40), counts(1000, 900, 800, 400), counts(1000, 900, 800, 800)};
    P.min_consistent = 0.5; P.min_samples = 50;
    expect(dc::policy_active(P), "verification makes a policy active", 0);
    expect(dc::choose_candidate(P, list, 4) == 2, "rank 0 fails (399 of 800), rank 1 has too few samples, rank 2 passes exactly on min_consistent", decisions++);
    expect(dc::candidates_to_check(P, 4) == 4 && dc::candidates_to_check(P, 0) == 0, "verification reads every candidate", decisions++);
    expect(dc::choose_candidate(P, list, 2) == -1, "none of the first two passes", decisions++);
    expect(dc::choose_candidate(P, list, 0) == -1, "no candidate", decisions++);
    expect(!dc::candidate_passes(P, list[0]) && !dc::candidate_passes(P, list[1]) && dc::candidate_passes(P, list[2]), "the three alone", decisions++);
    P.min_samples = 40;
    expect(dc::choose_candidate(P, list, 4) == 1, "n_both == min_samples is enough", decisions++);
    P.min_samples = 41;
    expect(dc::choose_candidate(P, list, 4) == 2, "n_both < min_samples is not", decisions++);
    P.min_consistent = 1.0;
    expect(dc::choose_candidate(P, list, 4) == 3, "min_consistent 1: every sample must agree", decisions++);
    P.min_consistent = 0.0;
    expect(dc::choose_candidate(P, list, 4) == 0 && dc::candidates_to_check(P, 4) == 1, "verification off: the top candidate, checked alone", decisions++);
    const nid_depth_counts empty = counts(1000, 0, 0, 0);
    P.min_consistent = 0.5; P.min_samples = 0;
    expect(dc::candidate_passes(P, empty), "0 >= 0.5 * 0: min_samples is what refuses an empty overlap", decisions++);
    P.min_samples = 1;
    expect(!dc::candidate_passes(P, empty), "... and does", decisions++);
  }
  {
    // the promotion
    P = nid_track_policy();
    expect(dc::promote(P, counts(1000, 1000, 1000, 1000), 1), "mode 0 promotes always", decisions++);
    P.keyframe_mode = 1; P.min_overlap = 0.75; P.max_age = 0;
    expect(dc::policy_active(P), "on demand is an active policy", 0);
    expect(!dc::promote(P, counts(1000, 750, 700, 700), 1000000), "an overlap exactly on min_overlap is not below it; max_age 0 is no limit", decisions++);
    expect(dc::promote(P, counts(1000, 749, 700, 700), 1), "one sample fewer is", decisions++);
    expect(!dc::promote(P, counts(1000, 751, 700, 700), 1), "one more is not", decisions++);
    expect(dc::promote(P, counts(0, 0, 0, 0), 1) == false, "no reference sample: 0 < 0 is false", decisions++);
    P.max_age = 3;
    expect(!dc::promote(P, counts(1000, 1000, 900, 900), 2), "age below max_age", decisions++);
    expect(dc::promote(P, counts(1000, 1000, 900, 900), 3), "max_age hit exactly", decisions++);
    expect(dc::promote(P, counts(1000, 1000, 900, 900), 4), "and beyond", decisions++);
    P.min_overlap = 0.0;
    expect(!dc::promote(P, counts(1000, 0, 0, 0), 1), "min_overlap 0 never promotes on overlap", decisions++);
  }
  {
    // the argument rule
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto with = [](void (*change)(nid_track_policy &, double), double v) {
      nid_track_policy Q = {};
      Q.tol_abs = 0.01; Q.tol_rel = 0.02;
      change(Q, v);
      return dc::policy_valid(Q);
    };
    expect(with([](nid_track_policy &Q, double v) { Q.keyframe_mode = (int)v; }, 1) && !with([](nid_track_policy &Q, double v) { Q.keyframe_mode = (int)v; }, 2) &&
               !with([](nid_track_policy &Q, double v) { Q.keyframe_mode = (int)v; }, -1), "keyframe_mode", decisions++);
    expect(!with([](nid_track_policy &Q, double v) { Q.max_age = (int)v; }, -1) && !with([](nid_track_policy &Q, double v) { Q.min_samples = (int)v; }, -1) &&
               !with([](nid_track_policy &Q, double v) { Q.reserved = (int)v; }, 1), "max_age, min_samples, reserved", decisions++);
    for (double bad : {nan, inf, -inf, -1e-9, 1.0000001}) {
      expect(!with([](nid_track_policy &Q, double v) { Q.min_overlap = v; }, bad), "min_overlap", decisions++);
      expect(!with([](nid_track_policy &Q, double v) { Q.min_consistent = v; }, bad), "min_consistent", decisions++);
    }
    for (double bad : {nan, inf, -inf, -1e-9}) {
      expect(!with([](nid_track_policy &Q, double v) { Q.tol_abs = v; }, bad), "tol_abs", decisions++);
      expect(!with([](nid_track_policy &Q, double v) { Q.tol_rel = v; }, bad), "tol_rel", decisions++);
    }
    expect(with([](nid_track_policy &Q, double v) { Q.min_overlap = v; }, 1.0) && with([](nid_track_policy &Q, double v) { Q.tol_abs = v; }, 0.0) &&
               with([](nid_track_policy &Q, double v) { Q.tol_rel = v; }, 1e300), "the ends of the ranges are inside", decisions++);
  }
  std::printf("depth check: %ld samples (%d with a special value, %ld in frame, %ld saturated sums), %d decisions, %d failures\n", samples, g_special,
              in_frame, saturated, decisions, g_failures);
  return g_failures ? 1 : 0;
}

// The rule of the bilinear gather (csrc/nid_refgather_rule.h: rg::observe, rg::taps_within, rg::gather and the host's loop
// rg::refgather_host on top of nid_reffill_rule.h's matrices and nid_reffuse_rule.h's part B -- plain arithmetic, no HIP) in
// a program of its own.  Built with -fsanitize=address,undefined,float-cast-overflow by tests/test_refgather_cpu.py.  Exit
// code 0: all as expected.
//
// Sequences of rg::refgather_host calls on one state over LCG inputs in which every quantity -- the keyframe's matrix, the
// pose, the intrinsics, both depth factors -- is now and then +-inf, NaN, +-1e300, a subnormal or zero, depth maps full of
// special counts, every gate, tap gate and cap, 2 x 2, 1 x N and N x 1 images among them: no conversion and no index out of
// range (the sanitizers say so; the depth maps are exactly rows x cols, so a tap beyond them is a heap overflow), and on
// every pixel behind every call: the four taps inside the image; the numerator of e below 2^26; e between the smallest and
// the largest of its observations; e a valid depth; e within the widest gate the pixel has seen of its uploaded count; a
// hole untouched; the counts those of the planes and the header's two identities.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nid_refgather_rule.h"

namespace {

uint64_t g_state = 20261023ull;
uint64_t next_u64() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return g_state >> 11;
}
double uniform() { return (double)next_u64() * (1.0 / 9007199254740992.0) * 2.0 - 1.0; }  // [-1, 1)

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
void expect(bool ok, const char *what, long k) {
  if (!ok) { g_failures++; std::printf("FAILED: %s (%ld)\n", what, k); }
}

uint16_t special_count() {
  static const uint16_t kCounts[] = {0, 1, 49, 50, 51, 65535, 65534, 32768};
  return next_u64() % 9 == 0 ? kCounts[next_u64() % 8] : (uint16_t)(6000 + next_u64() % 400);
}

// what the checker itself keeps of a pixel: the extremes of its observations and the widest gate it has seen
struct Seen {
  uint32_t lo, hi;
  int gate_abs, gate_rel;
};

long g_sampled = 0, g_outside = 0, g_tap_refused = 0, g_fused = 0, g_gated = 0, g_saturated = 0, g_changed = 0;

// one call on the state, and every invariant behind it
void call_and_check(const nid::rg::Gather &A, const std::vector<uint16_t> &d0, int gate_abs, int gate_rel, int max_obs, std::vector<uint32_t> &sum,
                    std::vector<uint8_t> &obs, std::vector<Seen> &seen, long tag) {
  using namespace nid;
  const size_t N = d0.size();
  std::vector<uint32_t> sum0 = sum;
  std::vector<uint8_t> obs0 = obs;
  std::vector<uint16_t> fused(N, 0xABAB), base(N, 0xABAB);
  nid_refgather_counts n;
  std::memset(&n, 0xAB, sizeof(n));
  expect(rg::args_ok(gate_abs, gate_rel, max_obs, A.tap_abs, A.tap_rel_1024), "args_ok", tag);
  rg::refgather_host(A, d0.data(), gate_abs, gate_rel, max_obs, sum.data(), obs.data(), fused.data(), base.data(), &n);
  long valid = 0, sampled = 0, outside = 0, tap_refused = 0, fusedn = 0, changed = 0;
  for (size_t i = 0; i < N; i++) {
    const uint16_t u = d0[i];
    if (!dc::depth_valid(u, A.factor0)) {
      expect(fused[i] == 0 && base[i] == u && sum[i] == sum0[i] && obs[i] == obs0[i], "a hole was touched", tag);
      continue;
    }
    valid++;
    uint32_t q = 0xABABABABu;
    size_t tap = (size_t)-1;
    const rg::Outcome o = rg::observe(A, (int)(i / (size_t)A.cols), (int)(i % (size_t)A.cols), u, &q, &tap);
    sampled += o == rg::kSampled;
    outside += o == rg::kOutside;
    tap_refused += o == rg::kTapRefused;
    if (tap != (size_t)-1) {  // the pixel reached G.4: its four taps are tap, tap + 1, tap + cols, tap + cols + 1
      expect(A.rows >= 2 && A.cols >= 2 && tap % (size_t)A.cols <= (size_t)A.cols - 2 && tap / (size_t)A.cols <= (size_t)A.rows - 2 &&
                 tap + (size_t)A.cols + 1 < N,
             "a tap outside the image", tag);
    } else {
      expect(o == rg::kOutside, "a pixel without taps that is not outside", tag);
    }
    if (o == rg::kSampled) expect(q >= 1 && q <= 65535 && dc::depth_valid((uint16_t)q, A.factor0), "an observation that is no valid count", tag);
    const uint32_t before = rfu::refined(u, sum0[i], obs0[i]);
    const bool took = obs[i] != obs0[i];
    if (took) {
      expect(o == rg::kSampled && obs[i] == obs0[i] + 1 && sum[i] == sum0[i] + q && obs0[i] < max_obs, "an observation that is not the sample's", tag);
      expect(rfu::within(q, u, gate_abs, gate_rel), "an observation outside the gate", tag);
      fusedn++;
      Seen &s = seen[i];
      if (q < s.lo) s.lo = q;
      if (q > s.hi) s.hi = q;
      if (gate_abs > s.gate_abs) s.gate_abs = gate_abs;
      if (gate_rel > s.gate_rel) s.gate_rel = gate_rel;
    } else {
      expect(sum[i] == sum0[i], "a sum moved without an observation", tag);
    }
    const uint64_t numerator = 2ull * ((uint64_t)u + sum[i]) + (obs[i] + 1ull);
    expect(numerator < (1ull << 26) && rfu::state_ok(sum[i], obs[i]), "the numerator's range", tag);
    const uint32_t e = rfu::refined(u, sum[i], obs[i]);
    expect(numerator / (2ull * (obs[i] + 1ull)) == e, "e in 32 bits is not e", tag);
    expect(e >= seen[i].lo && e <= seen[i].hi, "e outside its observations", tag);
    expect(e <= 65535 && dc::depth_valid((uint16_t)e, A.factor0), "e is no valid depth", tag);
    expect(rfu::within(e, u, seen[i].gate_abs, seen[i].gate_rel), "e left the gate of its uploaded sample", tag);
    expect(base[i] == e && fused[i] == (obs[i] ? e : 0), "the planes are not e", tag);
    expect(obs[i] != 0 || e == u, "k == 0 and e != u", tag);
    changed += e != before;
  }
  expect(n.n_valid == valid && n.n_sampled == sampled && n.n_outside == outside && n.n_tap_refused == tap_refused && n.n_fused == fusedn &&
             n.n_changed == changed,
         "the counts are not the planes'", tag);
  expect(n.n_valid == n.n_sampled + n.n_outside + n.n_tap_refused, "n_valid != n_sampled + n_outside + n_tap_refused", tag);
  expect(n.n_sampled == n.n_fused + n.n_gated + n.n_saturated && n.n_gated >= 0 && n.n_saturated >= 0, "n_sampled != n_fused + n_gated + n_saturated", tag);
  expect(n.n_changed <= n.n_fused && n.n_valid <= (int64_t)N, "a pixel changed without an observation", tag);
  g_sampled += n.n_sampled; g_outside += n.n_outside; g_tap_refused += n.n_tap_refused;
  g_fused += n.n_fused; g_gated += n.n_gated; g_saturated += n.n_saturated; g_changed += n.n_changed;
}

}  // namespace

int main() {
  using namespace nid;
  const int shapes[][2] = {{12, 20}, {2, 2}, {1, 17}, {9, 1}, {5, 7}, {16, 64}, {3, 3}, {1, 1}};
  long planes = 0, special = 0;
  for (int batch = 0; batch < 800; batch++) {
    const int rows = shapes[batch % 8][0], cols = shapes[batch % 8][1];
    const size_t N = (size_t)rows * cols;
    std::vector<uint16_t> d0(N), d1(N);
    std::vector<uint32_t> sum(N, 0);
    std::vector<uint8_t> obs(N, 0);
    std::vector<Seen> seen(N);
    for (size_t i = 0; i < N; i++) {
      d0[i] = next_u64() % 6 == 0 ? (uint16_t)(next_u64() % 50) : special_count();
      seen[i] = Seen{d0[i], d0[i], 0, 0};
    }
    bool sp = false;
    const bool plain = batch % 4 != 3;  // a pair of cameras that see each other's surface, so that samples land
    struct { double fx, fy, cx, cy; int rows, cols; } g;
    g.rows = rows; g.cols = cols;
    const double factor0 = batch % 11 ? 1.0 / 5000 : draw(1.0, 2, &sp);
    for (int call = 0; call < 6; call++) {
      for (size_t i = 0; i < N; i++) d1[i] = special_count();
      double Twc[16], pose7[7], K[12], M[12];
      for (int k = 0; k < 16; k++) Twc[k] = (k % 5 == 0 ? 1.0 : 0.0) + (plain ? 0.002 * uniform() : draw(1.0, 6, &sp));
      for (int k = 0; k < 7; k++) pose7[k] = (k == 3 ? 1.0 : 0.0) + (plain ? 0.003 * uniform() : draw(1.0, 6, &sp));
      if (plain && call == 3) pose7[6] = 0.7;  // the target further back: the keyframe's pixels crowd into its middle
      rf::keyframe_to_target(Twc, pose7, K);
      rf::target_to_keyframe(Twc, pose7, M);
      if (!plain && call % 2) {  // ... and matrices that are no rigid motion at all
        for (int k = 0; k < 12; k++) {
          K[k] = draw(2.0, 5, &sp);
          M[k] = draw(2.0, 5, &sp);
        }
      }
      g.fx = plain ? 10.0 : draw(20.0, 8, &sp); g.fy = plain ? -10.0 : draw(20.0, 8, &sp);
      g.cx = plain ? 0.5 * (cols - 1) : draw(20.0, 8, &sp); g.cy = plain ? 0.5 * (rows - 1) : draw(20.0, 8, &sp);
      const double factor1 = (batch + call) % 5 ? 1.0 / 5000 : draw(1.0, 2, &sp);
      const int gate_abs = (batch + call) % 13 == 0 ? 65535 : (int)(next_u64() % 200), gate_rel = (batch + call) % 17 == 0 ? 1024 : (int)(next_u64() % 64);
      const int tap_abs = (batch + call) % 3 == 0 ? 65535 : (int)(next_u64() % 600), tap_rel = (batch + call) % 7 == 0 ? 1024 : (int)(next_u64() % 64);
      const int max_obs = call < 2 ? 1 + (int)(next_u64() % 2) : (call == 5 ? 255 : 1 + (int)(next_u64() % 4));
      const rg::Gather A = rg::make_gather(g, K, M, d1.data(), factor1, factor0, tap_abs, tap_rel);
      call_and_check(A, d0, gate_abs, gate_rel, max_obs, sum, obs, seen, batch * 10 + call);
      planes++;
    }
    special += sp;
  }
  // the tap gate's comparison and the argument rule at their edges
  expect(rg::taps_within(1000, 1050, 1020, 1000, 50, 0) && !rg::taps_within(1000, 1051, 1020, 1000, 50, 0), "taps_within: the absolute bound", 0);
  expect(rg::taps_within(2048 + 40, 2048, 2060, 2050, 0, 20) && !rg::taps_within(2048 + 41, 2048, 2060, 2050, 0, 20), "taps_within: the relative bound, of the smallest tap", 0);
  expect(rg::taps_within(7, 7, 7, 7, 0, 0) && !rg::taps_within(7, 7, 8, 7, 0, 0) && rg::taps_within(1, 65535, 1, 1, 65534, 0) && !rg::taps_within(1, 65535, 1, 1, 65533, 0),
         "taps_within: the counts' extremes", 0);
  expect(!rg::args_ok(0, 0, 1, -1, 0) && !rg::args_ok(0, 0, 1, 65536, 0) && !rg::args_ok(0, 0, 1, 0, -1) && !rg::args_ok(0, 0, 1, 0, 1025) &&
             !rg::args_ok(0, 0, 0, 0, 0) && !rg::args_ok(-1, 0, 1, 0, 0) && rg::args_ok(65535, 1024, 255, 65535, 1024) && rg::args_ok(0, 0, 1, 0, 0),
         "args_ok's bounds", 0);
  std::printf("refgather: %ld planes (%ld with a special value), %ld sampled, %ld outside, %ld tap-refused, %ld fused, %ld gated, %ld saturated, %ld changed, %d failures\n",
              planes, special, g_sampled, g_outside, g_tap_refused, g_fused, g_gated, g_saturated, g_changed, g_failures);
  return g_failures ? 1 : 0;
}

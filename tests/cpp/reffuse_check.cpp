// The rule of the reference fusion (csrc/nid_reffuse_rule.h: rfu::refined, rfu::within, rfu::fuse and the host's loop
// rfu::reffuse_host on top of nid_reffill_rule.h's part A -- plain arithmetic, no HIP) in a program of its own.  Built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_reffuse_cpu.py.  Exit code 0: all as expected.
//
// Sequences of rfu::reffuse_host calls on one state over LCG inputs in which every quantity -- the keyframe's matrix, the
// pose, the intrinsics, both depth factors -- is now and then +-inf, NaN, +-1e300, a subnormal or zero, depth maps full of
// special counts, every gate and cap, 1 x 1 and one-row images among them: no conversion and no index out of range (the
// sanitizers say so), and on every pixel behind every call: the numerator of e below 2^26; e between the smallest and the
// largest of its observations; e a valid depth; e within the widest gate the pixel has seen of its uploaded count; a hole
// untouched; the counts those of the planes.  Then the cap: max_obs 255 with every observation 65535.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nid_reffuse_rule.h"

namespace {

uint64_t g_state = 20261022ull;
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
  return next_u64() % 5 == 0 ? kCounts[next_u64() % 8] : (uint16_t)(6000 + next_u64() % 400);
}

// what the checker itself keeps of a pixel: the extremes of its observations and the widest gate it has seen
struct Seen {
  uint32_t lo, hi;
  int gate_abs, gate_rel;
};

long g_fused = 0, g_gated = 0, g_saturated = 0, g_changed = 0;

// one call on the state, and every invariant behind it
void call_and_check(const nid::rf::Splat &S, const std::vector<uint16_t> &d0, int gate_abs, int gate_rel, int max_obs, std::vector<uint32_t> &sum,
                    std::vector<uint8_t> &obs, std::vector<Seen> &seen, long tag) {
  using namespace nid;
  const size_t N = d0.size();
  std::vector<uint32_t> sum0 = sum, zbuf(N);
  std::vector<uint8_t> obs0 = obs;
  std::vector<uint16_t> fused(N, 0xABAB), base(N, 0xABAB);
  nid_reffuse_counts n;
  std::memset(&n, 0xAB, sizeof(n));
  expect(rfu::args_ok(gate_abs, gate_rel, max_obs), "args_ok", tag);
  rfu::reffuse_host(S, d0.data(), gate_abs, gate_rel, max_obs, sum.data(), obs.data(), fused.data(), base.data(), zbuf.data(), &n);
  long valid = 0, hits = 0, on_valid = 0, fusedn = 0, changed = 0;
  for (size_t i = 0; i < N; i++) {
    const uint16_t u = d0[i];
    const bool hit = zbuf[i] != rf::kNone;
    hits += hit;
    if (hit) expect(zbuf[i] >= 1 && zbuf[i] <= 65535 && dc::depth_valid((uint16_t)zbuf[i], S.factor0), "a z-buffer entry that is no valid count", tag);
    if (!dc::depth_valid(u, S.factor0)) {
      expect(fused[i] == 0 && base[i] == u && sum[i] == sum0[i] && obs[i] == obs0[i], "a hole was touched", tag);
      continue;
    }
    valid++;
    on_valid += hit;
    const uint32_t before = rfu::refined(u, sum0[i], obs0[i]);
    const bool took = obs[i] != obs0[i];
    if (took) {
      expect(hit && obs[i] == obs0[i] + 1 && sum[i] == sum0[i] + zbuf[i] && obs0[i] < max_obs, "an observation that is not the hit's", tag);
      expect(rfu::within(zbuf[i], u, gate_abs, gate_rel), "an observation outside the gate", tag);
      fusedn++;
      Seen &s = seen[i];
      if (zbuf[i] < s.lo) s.lo = zbuf[i];
      if (zbuf[i] > s.hi) s.hi = zbuf[i];
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
    expect(e <= 65535 && dc::depth_valid((uint16_t)e, S.factor0), "e is no valid depth", tag);  // (a NaN factor makes count 0 valid)
    expect(rfu::within(e, u, seen[i].gate_abs, seen[i].gate_rel), "e left the gate of its uploaded sample", tag);
    expect(base[i] == e && fused[i] == (obs[i] ? e : 0), "the planes are not e", tag);
    expect(obs[i] != 0 || e == u, "k == 0 and e != u", tag);
    changed += e != before;
  }
  expect(n.n_valid == valid && n.n_hit == hits && n.n_fused == fusedn && n.n_changed == changed, "the counts are not the planes'", tag);
  expect(n.n_fused + n.n_gated + n.n_saturated == on_valid && n.n_gated >= 0 && n.n_saturated >= 0, "fused + gated + saturated != hits on valid pixels", tag);
  expect(n.n_hit <= n.n_splat && n.n_splat <= n.n_target_valid && n.n_target_valid <= (int64_t)N, "n_hit <= n_splat <= n_target_valid", tag);
  expect(n.n_changed <= n.n_fused, "a pixel changed without an observation", tag);
  g_fused += n.n_fused; g_gated += n.n_gated; g_saturated += n.n_saturated; g_changed += n.n_changed;
}

}  // namespace

int main() {
  using namespace nid;
  const int shapes[][2] = {{12, 20}, {1, 1}, {1, 17}, {9, 1}, {5, 7}, {16, 64}, {3, 3}};
  long planes = 0, special = 0;
  for (int batch = 0; batch < 700; batch++) {
    const int rows = shapes[batch % 7][0], cols = shapes[batch % 7][1];
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
    const bool plain = batch % 4 != 3;  // a pair of cameras that see each other's surface, so that splats land
    rf::Splat S;
    S.rows = rows; S.cols = cols; S.d1 = d1.data();
    S.factor0 = batch % 11 ? 1.0 / 5000 : draw(1.0, 2, &sp);
    for (int call = 0; call < 6; call++) {
      for (size_t i = 0; i < N; i++) d1[i] = special_count();
      double Twc[16], pose7[7];
      for (int k = 0; k < 16; k++) Twc[k] = (k % 5 == 0 ? 1.0 : 0.0) + (plain ? 0.002 * uniform() : draw(1.0, 6, &sp));
      for (int k = 0; k < 7; k++) pose7[k] = (k == 3 ? 1.0 : 0.0) + (plain ? 0.003 * uniform() : draw(1.0, 6, &sp));
      if (plain && call == 3) pose7[6] = 0.7;  // backwards: several target pixels onto one keyframe pixel
      rf::target_to_keyframe(Twc, pose7, S.M);
      S.fx = plain ? 10.0 : draw(20.0, 8, &sp); S.fy = plain ? -10.0 : draw(20.0, 8, &sp);
      S.cx = plain ? 0.5 * (cols - 1) : draw(20.0, 8, &sp); S.cy = plain ? 0.5 * (rows - 1) : draw(20.0, 8, &sp);
      S.factor1 = (batch + call) % 5 ? 1.0 / 5000 : draw(1.0, 2, &sp);
      const int gate_abs = (batch + call) % 13 == 0 ? 65535 : (int)(next_u64() % 200), gate_rel = (batch + call) % 17 == 0 ? 1024 : (int)(next_u64() % 64);
      const int max_obs = call < 2 ? 1 + (int)(next_u64() % 2) : (call == 5 ? 255 : 1 + (int)(next_u64() % 4));
      call_and_check(S, d0, gate_abs, gate_rel, max_obs, sum, obs, seen, batch * 10 + call);
      planes++;
    }
    special += sp;
  }
  // the cap: identical cameras, a target pixel on its own index; the keyframe at extreme counts, every observation 65535, the
  // widest gate, max_obs 255 -- 255 observations, then saturation, the sum at its largest
  {
    const int rows = 3, cols = 5;
    const size_t N = (size_t)rows * cols;
    std::vector<uint16_t> d0(N), d1(N, 65535);
    for (size_t i = 0; i < N; i++) d0[i] = i % 3 == 0 ? 65535 : (i % 3 == 1 ? 51 : (uint16_t)(1000 * i));
    std::vector<uint32_t> sum(N, 0);
    std::vector<uint8_t> obs(N, 0);
    std::vector<Seen> seen(N);
    for (size_t i = 0; i < N; i++) seen[i] = Seen{d0[i], d0[i], 0, 0};
    const double Twc[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, pose7[7] = {0, 0, 0, 1, 0, 0, 0};
    rf::Splat S;
    rf::target_to_keyframe(Twc, pose7, S.M);
    S.fx = 10; S.fy = -10; S.cx = 2; S.cy = 1; S.rows = rows; S.cols = cols; S.d1 = d1.data(); S.factor0 = S.factor1 = 1.0 / 5000;
    const long before = g_saturated;
    for (int call = 0; call < 258; call++) call_and_check(S, d0, 65535, 1024, 255, sum, obs, seen, 100000 + call);
    for (size_t i = 0; i < N; i++) expect(obs[i] == 255 && sum[i] == 255u * 65535u, "the cap was not reached with the largest sum", (long)i);
    expect(g_saturated - before == 3 * (long)N, "three calls beyond the cap are three saturated hits a pixel", 0);
    expect(rfu::refined(65535, 255u * 65535u, 255) == 65535 && rfu::refined(1, 255u * 65535u, 255) == 65279, "e at the largest sum", 0);
  }
  // e's rounding and the gate's comparison at their edges
  expect(rfu::refined(8192, 0, 0) == 8192 && rfu::refined(8192, 8200, 1) == 8196 && rfu::refined(8192, 8200 + 8201, 2) == 8198, "e: the header's examples", 0);
  expect(rfu::refined(8192, 8193, 1) == 8193 && rfu::refined(8193, 8192, 1) == 8193 && rfu::refined(0, 1, 1) == 1, "e rounds a half up", 0);
  expect(rfu::within(1050, 1000, 50, 0) && !rfu::within(1051, 1000, 50, 0) && rfu::within(950, 1000, 50, 0) && !rfu::within(949, 1000, 50, 0), "within: the absolute bound", 0);
  expect(rfu::within(2048 + 40, 2048, 0, 20) && !rfu::within(2048 + 41, 2048, 0, 20) && rfu::within(2048 - 40, 2048, 0, 20) && !rfu::within(2048 - 41, 2048, 0, 20),
         "within: the relative bound", 0);
  expect(rfu::within(65535, 1, 65534, 0) && !rfu::within(65535, 1, 65533, 0) && rfu::within(1, 65535, 65535, 1024) && rfu::within(7, 7, 0, 0) && !rfu::within(8, 7, 0, 0),
         "within: the counts' extremes", 0);
  expect(!rfu::args_ok(-1, 0, 1) && !rfu::args_ok(65536, 0, 1) && !rfu::args_ok(0, -1, 1) && !rfu::args_ok(0, 1025, 1) && !rfu::args_ok(0, 0, 0) &&
             !rfu::args_ok(0, 0, 256) && rfu::args_ok(65535, 1024, 255) && rfu::args_ok(0, 0, 1), "args_ok's bounds", 0);
  std::printf("reffuse: %ld planes (%ld with a special value), %ld fused, %ld gated, %ld saturated, %ld changed, %d failures\n", planes, special, g_fused,
              g_gated, g_saturated, g_changed, g_failures);
  return g_failures ? 1 : 0;
}

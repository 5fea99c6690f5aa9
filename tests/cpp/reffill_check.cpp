// The rule of the reference fill (csrc/nid_reffill_rule.h: rf::target_to_keyframe, rf::splat, the guard and the host's loop
// rf::reffill_host -- plain arithmetic, no HIP) in a program of its own.  Built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_reffill_cpu.py.  Exit code 0: all as expected.
//
// rf::reffill_host over LCG inputs in which every quantity -- the keyframe's matrix, the pose, the intrinsics, both depth
// factors -- is now and then +-inf, NaN, +-1e300, a subnormal or zero, depth maps full of special counts, old fill planes
// with entries on valid pixels, every guard, both accumulate values, 1 x 1 and one-row images among them: no conversion
// and no index out of range (the sanitizers say so); a fill stands only on a hole; n_filled <= n_holes; n_hit <= n_splat
// <= n_target_valid; the counts are those of the planes; under accumulate an old fill on a hole stays; and rf::splat alone
// never names a pixel outside the image or a count outside 1 ... 65535.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nid_reffill_rule.h"

namespace {

uint64_t g_state = 20261021ull;
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
  return next_u64() % 3 == 0 ? kCounts[next_u64() % 8] : (uint16_t)(6000 + next_u64() % 6000);
}

}  // namespace

int main() {
  using namespace nid;
  const int shapes[][2] = {{12, 20}, {1, 1}, {1, 17}, {9, 1}, {5, 7}, {16, 64}, {3, 3}};
  long planes = 0, special = 0, splats = 0, filled = 0, refused = 0, kept = 0;
  for (int batch = 0; batch < 1400; batch++) {
    const int rows = shapes[batch % 7][0], cols = shapes[batch % 7][1];
    const size_t N = (size_t)rows * cols;
    std::vector<uint16_t> d0(N), d1(N), fill(N), before(N);
    std::vector<uint32_t> zbuf(N);
    for (size_t i = 0; i < N; i++) {
      d0[i] = next_u64() % 3 == 0 ? (uint16_t)(next_u64() % 50) : special_count();
      d1[i] = special_count();
      fill[i] = next_u64() % 4 == 0 ? (uint16_t)(next_u64() % 65536) : (uint16_t)0;  // (also on valid pixels: the rule takes them off)
    }
    before = fill;
    bool sp = false;
    const bool plain = batch % 4 != 3;  // a pair of cameras that see each other's surface, so that splats land
    double Twc[16], pose7[7];
    for (int k = 0; k < 16; k++) Twc[k] = (k % 5 == 0 ? 1.0 : 0.0) + (plain ? 0.002 * uniform() : draw(1.0, 6, &sp));
    for (int k = 0; k < 7; k++) pose7[k] = (k == 3 ? 1.0 : 0.0) + (plain ? 0.003 * uniform() : draw(1.0, 6, &sp));
    if (plain && batch % 8 == 0) pose7[6] = 0.7;  // backwards: several target pixels onto one keyframe pixel
    rf::Splat S;
    rf::target_to_keyframe(Twc, pose7, S.M);
    S.fx = plain ? 10.0 : draw(20.0, 8, &sp); S.fy = plain ? -10.0 : draw(20.0, 8, &sp);
    S.cx = plain ? 0.5 * (cols - 1) : draw(20.0, 8, &sp); S.cy = plain ? 0.5 * (rows - 1) : draw(20.0, 8, &sp);
    S.rows = rows; S.cols = cols; S.d1 = d1.data();
    S.factor1 = batch % 5 ? 1.0 / 5000 : draw(1.0, 2, &sp);
    S.factor0 = batch % 11 ? 1.0 / 5000 : draw(1.0, 2, &sp);
    special += sp;
    const int guard = batch % 3, accumulate = (batch / 3) % 2;
    const int guard_abs = batch % 13 == 0 ? 65535 : (int)(next_u64() % 100), guard_rel = batch % 17 == 0 ? 1024 : (int)(next_u64() % 64);
    expect(rf::args_ok(guard, guard_abs, guard_rel), "args_ok", batch);
    // rf::splat alone: what it names is inside the image and a count
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < cols; c++) {
        size_t idx = N;
        uint32_t q = 0;
        const int k = rf::splat(S, r, c, &idx, &q);
        expect(k >= 0 && k <= 2, "splat's outcome", batch);
        if (k == 2) expect(idx < N && q >= 1 && q <= 65535 && dc::depth_valid((uint16_t)q, S.factor0), "a splat outside the image or the counts", batch);
      }
    nid_reffill_counts n;
    std::memset(&n, 0xAB, sizeof(n));
    rf::reffill_host(S, d0.data(), guard, guard_abs, guard_rel, accumulate, fill.data(), zbuf.data(), &n);
    planes++;
    long holes = 0, nz = 0, hits = 0, fresh = 0;
    for (size_t i = 0; i < N; i++) {
      const bool valid = dc::depth_valid(d0[i], S.factor0);
      holes += !valid;
      nz += fill[i] != 0;
      hits += zbuf[i] != rf::kNone;
      fresh += before[i] == 0 && fill[i] != 0;
      if (fill[i]) expect(!valid, "a fill on a pixel whose uploaded depth is valid", batch);
      if (!valid && accumulate && before[i]) { expect(fill[i] == before[i], "accumulate lost a fill", batch); kept++; }
      if (fill[i] && !(accumulate && before[i])) expect(zbuf[i] == fill[i], "a new fill that is not the z-buffer's entry", batch);
      if (zbuf[i] != rf::kNone) expect(zbuf[i] >= 1 && zbuf[i] <= 65535, "a z-buffer entry that is no count", batch);
    }
    expect(n.n_holes == holes && n.n_filled == nz && n.n_hit == hits && n.n_new == fresh && n.reserved == 0, "the counts are not the planes'", batch);
    expect(n.n_filled <= n.n_holes, "n_filled > n_holes", batch);
    expect(n.n_hit <= n.n_splat && n.n_splat <= n.n_target_valid && n.n_target_valid <= (int64_t)N, "n_hit <= n_splat <= n_target_valid", batch);
    expect(n.n_refused >= 0 && n.n_refused + n.n_filled <= n.n_holes && (guard > 0 || n.n_refused == 0), "n_refused", batch);
    splats += n.n_splat;
    filled += n.n_filled;
    refused += n.n_refused;
    // a null counts pointer is allowed, and a second call under accumulate changes nothing that is filled
    std::vector<uint16_t> again = fill;
    rf::reffill_host(S, d0.data(), guard, guard_abs, guard_rel, 1, again.data(), zbuf.data(), nullptr);
    for (size_t i = 0; i < N; i++)
      if (fill[i]) expect(again[i] == fill[i], "a second accumulating call moved a fill", batch);
  }
  // the guard's comparison at its edges, in 64-bit integers
  expect(!rf::behind(1000, 950, 50, 0) && rf::behind(1001, 950, 50, 0), "behind: the absolute tolerance's edge", 0);
  expect(!rf::behind(2048 + 40, 2048, 0, 20) && rf::behind(2048 + 41, 2048, 0, 20), "behind: the relative tolerance's edge", 0);
  expect(!rf::behind(1, 65535, 0, 0) && rf::behind(65535, 1, 65534, 0) == false && rf::behind(65535, 1, 65533, 0), "behind: the counts' extremes", 0);
  expect(!rf::args_ok(-1, 0, 0) && !rf::args_ok(3, 0, 0) && !rf::args_ok(0, -1, 0) && !rf::args_ok(0, 65536, 0) && !rf::args_ok(0, 0, -1) &&
             !rf::args_ok(0, 0, 1025) && rf::args_ok(2, 65535, 1024), "args_ok's bounds", 0);
  std::printf("reffill: %ld planes (%ld with a special value), %ld splats, %ld fills, %ld refused, %ld kept, %d failures\n", planes, special, splats,
              filled, refused, kept, g_failures);
  return g_failures ? 1 : 0;
}

// The rule of the reference mask (csrc/nid_depth_check.h: dc::classify, dc::backproject and the host's masking loop
// dc::refmask_host -- plain arithmetic, no HIP) in a program of its own.  Built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_refmask_cpu.py.  Exit code 0: all as expected.
//
// 1. dc::classify plus counting against dc::sample, sample by sample, over LCG inputs in which every quantity -- point,
//    pose matrix, intrinsics, factor, tolerances -- is now and then +-inf, NaN, +-1e300 or a subnormal, and over
//    degenerate samples written by hand: the counts a restatement makes from the class are dc::sample's.
// 2. dc::refmask_host over random planes, depth maps full of special counts, degenerate matrices and every dilation,
//    1 x 1 and one-row images among them: no index out of range (the sanitizers say so), the caller's bit kept, bit 8
//    never beside bit 2 or 4, the counts those of the plane, and the dilation equal to a search written here.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "nid_depth_check.h"

namespace {

uint64_t g_state = 20250917ull;
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

// the counts of one sample from its class alone (nid_keyframe.h's steps, read off the class)
void count_class(nid::dc::Class k, nid_depth_cell *a) {
  using namespace nid::dc;
  if (k >= kNotInView) a->n_ref++;
  if (k >= kNoTargetDepth) a->n_inframe++;
  if (k >= kConsistent) a->n_both++;
  if (k == kConsistent) a->n_consistent++;
  if (k == kOccluded) a->n_occluded++;
  if (k == kThrough) a->n_through++;
}

bool same_counts(const nid_depth_cell &a, const nid_depth_cell &b) {
  return a.n_ref == b.n_ref && a.n_inframe == b.n_inframe && a.n_both == b.n_both && a.n_consistent == b.n_consistent &&
         a.n_occluded == b.n_occluded && a.n_through == b.n_through;
}

}  // namespace

int main() {
  using namespace nid;
  // ---- 1. classify + counting == sample ---------------------------------------------------------------------------------
  const int rows = 12, cols = 20;
  std::vector<uint16_t> d1((size_t)rows * cols);
  long samples = 0, special = 0, step5 = 0;
  for (int batch = 0; batch < 400; batch++) {
    for (uint16_t &d : d1) d = (uint16_t)(next_u64() % 4 == 0 ? next_u64() % 65536 : 8000 + next_u64() % 4000);
    dc::View V;
    bool sp = false;
    const bool plain = batch % 4 == 0;  // a camera that sees the points, so that samples reach step 5
    for (int k = 0; k < 12; k++) V.M[k] = plain ? ((k == 0 || k == 5 || k == 10) ? 1.0 : 0.01 * uniform()) : draw(1.0, 6, &sp);
    V.fx = plain ? 10.0 : draw(20.0, 8, &sp); V.fy = plain ? -10.0 : draw(20.0, 8, &sp);
    V.cx = plain ? 9.5 : draw(20.0, 8, &sp); V.cy = plain ? 5.5 : draw(20.0, 8, &sp);
    V.rows = rows; V.cols = cols; V.d1 = d1.data();
    V.factor = batch % 3 ? 1.0 / 5000 : draw(1.0, 2, &sp);
    V.tol_abs = batch % 5 ? 0.01 : draw(1.0, 2, &sp);
    V.tol_rel = batch % 7 ? 0.02 : draw(1.0, 2, &sp);
    nid_depth_cell by_sample = {}, by_class = {};
    for (int s = 0; s < 600; s++) {
      bool sp_point = sp;
      const double X = draw(2.0, 10, &sp_point), Y = draw(1.0, 10, &sp_point), Z = plain && s % 3 ? 1.5 + uniform() : draw(4.0, 10, &sp_point);
      nid_depth_cell one = {}, one_class = {};
      dc::sample(V, X, Y, Z, &one);
      double dz = -12345.0;
      const dc::Class k = dc::classify(V, X, Y, Z, &dz);
      count_class(k, &one_class);
      expect(same_counts(one, one_class), "a sample's counts from its class", samples);
      expect(dc::classify(V, X, Y, Z) == k, "the class without dz", samples);
      expect(k >= dc::kConsistent || dz == -12345.0, "dz is written at step 5 alone", samples);
      if (k == dc::kConsistent) {  // the sum's term from the dz classify gives
        const double um = (dz < 0 ? -dz : dz) * 1e6 + 0.5;
        expect(one.sum_abs_um == (um < dc::kUmSaturated ? (uint64_t)um : (uint64_t)1 << 63), "sum_abs_um from classify's dz", samples);
      } else {
        expect(one.sum_abs_um == 0, "a sum without a consistent sample", samples);
      }
      dc::sample(V, X, Y, Z, &by_sample);
      count_class(k, &by_class);
      step5 += k >= dc::kConsistent;
      special += sp_point;
      samples++;
    }
    expect(same_counts(by_sample, by_class), "a batch's counts", batch);
  }
  {  // degenerate samples by hand
    dc::View V = {};
    V.M[0] = V.M[5] = V.M[10] = 1.0;
    V.fx = 10; V.fy = -10; V.cx = 9.5; V.cy = 5.5; V.rows = rows; V.cols = cols; V.d1 = d1.data();
    for (uint16_t &d : d1) d = 10000;  // 2 m
    V.factor = 1.0 / 5000; V.tol_abs = 0.01; V.tol_rel = 0.02;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    expect(dc::classify(V, nan, 0, 2) == dc::kNone, "a NaN X is no sample", 0);
    expect(dc::classify(V, 0, nan, 2) == dc::kNotInView && dc::classify(V, 0, 0, nan) == dc::kNotInView, "a NaN Y or Z is not in view", 0);
    expect(dc::classify(V, 0, 0, 0) == dc::kNotInView && dc::classify(V, 0, 0, -1) == dc::kNotInView, "zc <= 0", 0);
    expect(dc::classify(V, inf, 0, 2) == dc::kNotInView && dc::classify(V, 0, 0, inf) == dc::kNotInView, "infinities", 0);
    expect(dc::classify(V, 100, 0, 2) == dc::kNotInView, "out of the frame", 0);
    expect(dc::classify(V, 0, 0, 2) == dc::kConsistent && dc::classify(V, 0, 0, 2.5) == dc::kOccluded && dc::classify(V, 0, 0, 1.5) == dc::kThrough, "the three classes", 0);
    d1[5 * cols + 9] = d1[5 * cols + 10] = d1[6 * cols + 9] = d1[6 * cols + 10] = 0;
    expect(dc::classify(V, 0, 0, 2) == dc::kNoTargetDepth, "no target depth", 0);
    // the back-projection: invalid depths leave the point alone
    double X = 7, Y = 8, Z = 9;
    const double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.5, -0.25, 2, 1};
    expect(!dc::backproject(0.0, 3, 4, 10, -10, 9.5, 5.5, T, &X, &Y, &Z) && X == 7 && Y == 8 && Z == 9, "z = 0", 0);
    expect(!dc::backproject(100.5, 3, 4, 10, -10, 9.5, 5.5, T, &X, &Y, &Z) && !dc::backproject(-1.0, 3, 4, 10, -10, 9.5, 5.5, T, &X, &Y, &Z), "z out of range", 0);
    expect(dc::backproject(2.0, 3, 4, 10, -10, 9.5, 5.5, T, &X, &Y, &Z) && X == 2.0 * (4 - 9.5) / 10 + 0.5 && Y == 2.0 * (3 - 5.5) / -10 - 0.25 && Z == 4.0, "a valid pixel", 0);
  }

  // ---- 2. the masking loop ----------------------------------------------------------------------------------------------
  long planes = 0, bits = 0;
  static const int kShapes[][2] = {{1, 1}, {1, 37}, {23, 1}, {7, 9}, {17, 40}, {33, 70}};
  for (int it = 0; it < 240; it++) {
    const int R = kShapes[it % 6][0], C = kShapes[it % 6][1];
    const size_t N = (size_t)R * C;
    std::vector<uint16_t> a(N), b(N);
    static const uint16_t kCounts[] = {0, 1, 49, 50, 51, 65535, 10000, 5000, 20000};
    for (size_t i = 0; i < N; i++) {
      a[i] = next_u64() % 8 == 0 ? kCounts[next_u64() % 9] : (uint16_t)(9000 + next_u64() % 2000);
      b[i] = next_u64() % 3 == 0 ? kCounts[next_u64() % 9] : (uint16_t)(9000 + next_u64() % 2000);
    }
    dc::View V;
    bool sp = false;
    const bool plain = it % 3 != 2;
    for (int k = 0; k < 12; k++) V.M[k] = plain ? ((k == 0 || k == 5 || k == 10) ? 1.0 : 0.002 * uniform()) : draw(1.0, 6, &sp);
    V.fx = plain ? 20.0 : draw(20.0, 8, &sp); V.fy = plain ? -20.0 : draw(20.0, 8, &sp);
    V.cx = (C - 1) / 2.0; V.cy = (R - 1) / 2.0;
    V.rows = R; V.cols = C; V.d1 = b.data();
    V.factor = it % 5 == 4 ? draw(1.0, 2, &sp) : 1.0 / 5000;
    V.tol_abs = 0.01; V.tol_rel = it % 7 == 6 ? draw(1.0, 2, &sp) : 0.02;
    double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (!plain) for (int k = 0; k < 16; k++) T[k] = draw(1.0, 6, &sp);
    const dc::Keyframe K = {a.data(), it % 11 == 10 ? draw(1.0, 2, &sp) : 1.0 / 5000, T};
    const int classes = (int)(next_u64() % 4) * 2, dilate = it % (NID_REFMASK_MAX_DILATE + 1), accumulate = (int)(next_u64() % 2);
    std::vector<uint8_t> before(N), m(N);
    for (size_t i = 0; i < N; i++) before[i] = (uint8_t)(next_u64() % 5 == 0 ? next_u64() % 16 : 0);
    m = before;
    nid_refmask_counts n = {};
    dc::refmask_host(V, K, classes, dilate, accumulate, m.data(), &n);
    nid_refmask_counts want = {};
    for (int r = 0; r < R; r++)
      for (int c = 0; c < C; c++) {
        const size_t i = (size_t)r * C + c;
        const uint8_t v = m[i];
        expect((v & 1) == (before[i] & 1), "the caller's bit stays", it);
        expect(!((v & 6) && (v & 8)), "bit 8 beside a class bit", it);
        expect((v & 6 & ~classes) == (accumulate ? (before[i] & 6 & ~classes) : 0), "a class that was not selected", it);
        expect(dc::depth_valid(a[i], K.factor) || (v & 6) == (accumulate ? (before[i] & 6) : 0), "an invalid pixel got a class", it);
        bool near = false;  // the window, searched here
        for (int rr = r - dilate; rr <= r + dilate; rr++)
          for (int cc = c - dilate; cc <= c + dilate; cc++)
            if (rr >= 0 && rr < R && cc >= 0 && cc < C && (m[(size_t)rr * C + cc] & 6)) near = true;
        if (!(v & 6)) expect(((v & 8) != 0) == ((dilate > 0 && near) || (accumulate && (before[i] & 8))), "bit 8", it);
        const bool valid = dc::depth_valid(a[i], K.factor);
        want.n_valid += valid; want.n_caller += v & 1; want.n_occluded += (v >> 1) & 1; want.n_through += (v >> 2) & 1;
        want.n_dilated += (v >> 3) & 1; want.n_masked += valid && v;
        bits += v != 0;
      }
    expect(std::memcmp(&n, &want, sizeof(n)) == 0, "the counts are the plane's", it);
    planes++;
  }
  std::printf("refmask: %ld samples (%ld with a special value, %ld classified at step 5), %ld planes (%ld bits set), %d failures\n", samples, special, step5,
              planes, bits, g_failures);
  return g_failures ? 1 : 0;
}

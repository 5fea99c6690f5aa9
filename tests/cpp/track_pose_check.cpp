// The pose helpers of include/nid/nid_pyr_stream.h (csrc/nid_track_pose.h: plain arithmetic on nid_lm_step.h's SE(3) text,
// no HIP) against the 4x4-matrix route with libm's sin / cos, over a few thousand LCG poses of the size of
// synth.make_pair's (rotations up to ~0.1 rad about a random axis, translations up to ~0.3 m).  Built with
// -fsanitize=address,undefined by tests/test_pyr_stream_cpu.py.  Exit code 0: all as expected.
//
// Bounds.  kTol = 1e-14 per component: a few tens of ulps of O(1) quantities, the order two sin / cos implementations
// differ by.  The exponential adds two terms of its own, both properties of SE3Quat::exp's formulas and not of this code:
//   * above the small-angle switch (theta >= 1e-5) b = (1 - cos theta) / theta^2 divides a difference of two numbers near
//     1 that two correctly rounded cosines may give one ulp apart: a relative eps / theta^2 in b, i.e. eps |upsilon| / theta
//     in the translation V upsilon (4 x that allowed); the rotation's term b Om^2 moves by eps only;
//   * below it R = I + Om + Om^2 is a rotation only to theta^2, so the unit quaternion made from it and the matrix route,
//     which carries R as it is, differ by that order (2 theta^2 allowed).
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "nid_track_pose.h"

namespace {

constexpr double kTol = 1e-14, kEps = 2.220446049250313e-16;

uint64_t g_state = 20211003ull;
double uniform() {  // [-1, 1)
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

struct M4 { double m[4][4]; };

M4 mul(const M4 &a, const M4 &b) {
  M4 o{};
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 4; k++) o.m[i][j] += a.m[i][k] * b.m[k][j];
  return o;
}

M4 matrix(const double *p) {  // to_homogeneous_matrix (synth.pose7_to_matrix)
  const double x = p[0], y = p[1], z = p[2], w = p[3];
  M4 o{};
  o.m[0][0] = 1 - 2 * (y * y + z * z); o.m[0][1] = 2 * (x * y - z * w);     o.m[0][2] = 2 * (x * z + y * w);     o.m[0][3] = p[4];
  o.m[1][0] = 2 * (x * y + z * w);     o.m[1][1] = 1 - 2 * (x * x + z * z); o.m[1][2] = 2 * (y * z - x * w);     o.m[1][3] = p[5];
  o.m[2][0] = 2 * (x * z - y * w);     o.m[2][1] = 2 * (y * z + x * w);     o.m[2][2] = 1 - 2 * (x * x + y * y); o.m[2][3] = p[6];
  o.m[3][3] = 1;
  return o;
}

M4 rigid_inverse(const M4 &a) {
  M4 o{};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o.m[i][j] = a.m[j][i];
    o.m[i][3] = -(a.m[0][i] * a.m[0][3] + a.m[1][i] * a.m[1][3] + a.m[2][i] * a.m[2][3]);
  }
  o.m[3][3] = 1;
  return o;
}

M4 exp_matrix(const double *u) {  // SE3Quat::exp with libm, the switch included (synth.perturb_pose7)
  const double th = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double Om[3][3] = {{0, -u[2], u[1]}, {u[2], 0, -u[0]}, {-u[1], u[0], 0}};
  double Om2[3][3] = {};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      for (int k = 0; k < 3; k++) Om2[i][j] += Om[i][k] * Om[k][j];
  double a = 1, b = 1, c = 1;  // below the switch: R = V = I + Om + Om^2
  if (!(th < 0.00001)) { a = std::sin(th) / th; b = (1 - std::cos(th)) / (th * th); c = (th - std::sin(th)) / (th * th * th); }
  M4 o{};
  double V[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const double id = i == j ? 1.0 : 0.0;
      o.m[i][j] = id + a * Om[i][j] + b * Om2[i][j];
      V[i][j] = id + b * Om[i][j] + c * Om2[i][j];
    }
  for (int i = 0; i < 3; i++) o.m[i][3] = V[i][0] * u[3] + V[i][1] * u[4] + V[i][2] * u[5];
  o.m[3][3] = 1;
  return o;
}

int g_bad = 0;
void fail(const char *what, int k, double d, double tol) {
  if (g_bad < 20) std::printf("%s, case %d: %.3e > %.3e\n", what, k, d, tol);
  g_bad++;
}

double max_diff(const M4 &a, const M4 &b) {
  double d = 0;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 4; j++) d = std::fmax(d, std::fabs(a.m[i][j] - b.m[i][j]));
  return d;
}

double max_diff7(const double *a, const double *b) {
  double d = 0;
  for (int i = 0; i < 7; i++) d = std::fmax(d, std::fabs(a[i] - b[i]));
  return d;
}

void check_unit(const char *what, int k, const double *p) {
  const double n2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
  if (!(p[3] >= 0)) fail(what, k, p[3], 0.0);
  if (!(std::fabs(std::sqrt(n2) - 1.0) <= 4 * kEps)) fail(what, k, std::fabs(std::sqrt(n2) - 1.0), 4 * kEps);
}

void random_pose(double angle, double shift, double *p) {
  double ax[3] = {uniform(), uniform(), uniform()};
  const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-300, th = angle * uniform();
  double q[4] = {ax[0] / n * std::sin(th / 2), ax[1] / n * std::sin(th / 2), ax[2] / n * std::sin(th / 2), std::cos(th / 2)};
  nid::lm::normalize_rotation(q);
  for (int i = 0; i < 4; i++) p[i] = q[i];
  for (int i = 0; i < 3; i++) p[4 + i] = shift * uniform();
}

}  // namespace

int main() {
  using namespace nid::track;
  int cases = 0, below = 0, above = 0, flipped = 0;
  for (int k = 0; k < 4000; k++, cases++) {
    // every fourth pose a large rotation: the raw quaternion product of two of them has w < 0 about as often as not
    const double angle = (k % 4 == 3) ? 3.1 : 0.1;
    double a[7], b[7], o[7], o2[7], T[16];
    random_pose(angle, 0.3, a);
    random_pose(angle, 0.3, b);
    const M4 Ma = matrix(a), Mb = matrix(b);
    // inverse
    pose_inverse(a, o);
    check_unit("inverse: quaternion", k, o);
    double d = max_diff(matrix(o), rigid_inverse(Ma));
    if (!(d <= kTol)) fail("inverse against the matrix route", k, d, kTol);
    pose_inverse(o, o2);
    if (!((d = max_diff7(o2, a)) <= kTol)) fail("inverse(inverse(p)) - p", k, d, kTol);
    // composition
    pose_compose(a, b, o);
    check_unit("compose: quaternion", k, o);
    if (a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2] < 0) flipped++;
    if (!((d = max_diff(matrix(o), mul(Ma, Mb))) <= kTol)) fail("compose against the matrix route", k, d, kTol);
    pose_inverse(a, o2);
    pose_compose(o2, o, o2);  // (output aliasing an input) a^-1 o (a o b) = b
    if (!((d = max_diff(matrix(o2), Mb)) <= kTol)) fail("inverse(a) o (a o b) - b", k, d, kTol);
    // T_wc and back
    pose_to_Twc16(a, T);
    M4 Mt{};
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) Mt.m[r][c] = T[4 * c + r];
    if (!((d = max_diff(Mt, rigid_inverse(Ma))) <= kTol) || T[3] != 0 || T[7] != 0 || T[11] != 0 || T[15] != 1) fail("to_Twc16 against the matrix route", k, d, kTol);
    pose_from_Twc16(T, o);
    check_unit("from_Twc16: quaternion", k, o);
    if (!((d = max_diff7(o, a)) <= kTol)) fail("from_Twc16(to_Twc16(p)) - p", k, d, kTol);
    // exp(twist) o pose: rotation sizes from 1e-9 to 0.5 rad, the switch at 1e-5 straddled closely every eighth case
    double tw[6];
    double th = std::pow(10.0, -9.0 + 8.7 * (0.5 + 0.5 * uniform()));
    if (k % 8 == 0) th = 0.00001 * (1.0 - 1e-3);
    if (k % 8 == 1) th = 0.00001 * (1.0 + 1e-3);
    {
      double ax[3] = {uniform(), uniform(), uniform()};
      const double n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-300;
      for (int i = 0; i < 3; i++) { tw[i] = ax[i] / n * th; tw[3 + i] = 0.05 * uniform(); }
    }
    const double th_is = std::sqrt(tw[0] * tw[0] + tw[1] * tw[1] + tw[2] * tw[2]);
    const double ups = std::sqrt(tw[3] * tw[3] + tw[4] * tw[4] + tw[5] * tw[5]);
    const bool small = th_is < 0.00001;
    (small ? below : above)++;
    const double tol = small ? kTol + 2 * th_is * th_is : kTol + 4 * kEps * ups / th_is;
    pose_perturb(a, tw, o);
    check_unit("perturb: quaternion", k, o);
    if (!((d = max_diff(matrix(o), mul(exp_matrix(tw), Ma))) <= tol)) fail("perturb against the matrix route", k, d, tol);
  }
  // fixed points
  {
    const double id[7] = {0, 0, 0, 1, 0, 0, 0}, zero[6] = {0, 0, 0, 0, 0, 0}, I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double o[7], T[16];
    pose_inverse(id, o);
    if (max_diff7(o, id) != 0) fail("inverse(identity)", 0, max_diff7(o, id), 0);
    pose_perturb(id, zero, o);
    if (max_diff7(o, id) != 0) fail("perturb(identity, 0)", 0, max_diff7(o, id), 0);
    pose_from_Twc16(I16, o);
    if (max_diff7(o, id) != 0) fail("from_Twc16(identity)", 0, max_diff7(o, id), 0);
    pose_to_Twc16(id, T);
    for (int i = 0; i < 16; i++)
      if (T[i] != I16[i]) fail("to_Twc16(identity)", i, T[i], I16[i]);
  }
  std::printf("track pose: %d cases (%d twists below the small-angle switch, %d above, %d compositions with a raw w < 0), %d failures\n", cases,
              below, above, flipped, g_bad);
  return g_bad ? 1 : 0;
}

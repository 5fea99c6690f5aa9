// The arithmetic of csrc/nid_lm_step.h against long-double references, alone in a program of its own: sincos_pos against
// sinl / cosl, se3_exp against a long-double restatement of the same formulas branch for branch, se3_mul and pose_record
// against long double, ldlt6_solve against long-double Gaussian elimination with full pivoting.  Built with
// -ffp-contract=off -fsanitize=address,undefined and run by tests/test_lm_step_cpu.py, which parses the lines
//   <name>: <N> cases, worst <W> <unit>, <F> failures
// Exit code 0: no failures.  The bounds and where they come from stand at each check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "nid_lm_step.h"

namespace {

using nid::lm::kDblMin;
typedef long double ld;
const double kEps = std::numeric_limits<double>::epsilon();
const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();
const ld kPiL = 3.14159265358979323846264338327950288419716939937510L;

uint64_t g_state = 20240521ull;
uint64_t draw64() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  uint64_t z = g_state;
  z ^= z >> 33; z *= 0xff51afd7ed558ccdull; z ^= z >> 33;
  return z;
}
double uniform() { return (double)(draw64() >> 11) * 0x1p-53; }  // [0, 1)
double uniform(double a, double b) { return a + (b - a) * uniform(); }
double log_uniform(double a, double b) { return std::exp(uniform(std::log(a), std::log(b))); }
double normal() {
  const double u = 1.0 - uniform(), v = uniform();
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

int g_failures = 0;

struct Stat {
  long cases = 0, failures = 0;
  double worst = 0;
  void add(double v, double bound, const char *what, double at) {
    cases++;
    if (v > worst) worst = v;
    if (!(v <= bound)) {
      if (failures < 5) std::printf("  FAIL %s: %.6g > %.6g at %a\n", what, v, bound, at);
      failures++;
    }
  }
  void fail(const char *what, double at) {
    if (failures < 5) std::printf("  FAIL %s at %a\n", what, at);
    failures++;
  }
  void print(const char *name, const char *unit) {
    std::printf("%s: %ld cases, worst %.4g %s, %ld failures\n", name, cases, worst, unit, failures);
    g_failures += failures != 0;
  }
};

// ---- sincos_pos ---------------------------------------------------------------------------------------------------
// |got - ref| in units in the last place of the (long-double) reference value
double ulps(double got, ld ref) {
  if (ref == 0) return got == 0 ? 0.0 : kInf;
  const ld ulp = ldexpl(1.0L, ilogbl(fabsl(ref)) - 52);
  return (double)(fabsl((ld)got - ref) / ulp);
}

constexpr int kDecLo = -8, kDecHi = 5;
double g_dec_sin[kDecHi - kDecLo + 1], g_dec_cos[kDecHi - kDecLo + 1];
double g_worst_sin = 0, g_worst_cos = 0, g_at_sin = 0, g_at_cos = 0;

// The bound: 4 ulp of the reference value.  The reduction's first subtraction is exact (kd * kP1 is, and it cancels),
// the three behind it round, each to within half an ulp of r: at most 1.5 ulp of r, which the polynomial passes on
// (|d sin| <= |d r|, |d cos| <= |r| |d r|); the polynomial's own error and the final sum add about one more.
void check_sincos(double theta, Stat &st) {
  double s, c;
  nid::lm::sincos_pos(theta, &s, &c);
  const double es = ulps(s, sinl((ld)theta)), ec = ulps(c, cosl((ld)theta));
  st.add(es, 4.0, "sin", theta);
  st.add(ec, 4.0, "cos", theta);
  st.cases--;  // (one case, two figures)
  if (es > g_worst_sin) { g_worst_sin = es; g_at_sin = theta; }
  if (ec > g_worst_cos) { g_worst_cos = ec; g_at_cos = theta; }
  if (theta > 0) {
    int d = (int)std::floor(std::log10(theta));
    d = d < kDecLo ? kDecLo : d > kDecHi ? kDecHi : d;
    if (es > g_dec_sin[d - kDecLo]) g_dec_sin[d - kDecLo] = es;
    if (ec > g_dec_cos[d - kDecLo]) g_dec_cos[d - kDecLo] = ec;
  }
}

void sincos_all() {
  {
    Stat st;
    for (int i = 0; i < 2000000; i++) check_sincos(uniform(0.0, 10.0), st);
    st.print("sincos [0, 10]", "ulp");
  }
  {
    Stat st;
    for (int i = 0; i < 2000000; i++) check_sincos(uniform(0.0, 1e6), st);
    st.print("sincos [0, 1e6]", "ulp");
  }
  {
    Stat st;
    for (int i = 0; i < 2000000; i++) check_sincos(log_uniform(1e-8, 1e6), st);
    st.print("sincos log-uniform", "ulp");
  }
  {  // the double nearest k pi/2 and two neighbours on each side: where the reduction cancels most
    Stat st;
    for (int k = 1; k <= 636619; k++) {
      const double t = (double)((ld)k * (kPiL / 2));
      double lo = t, hi = t;
      check_sincos(t, st);
      for (int j = 0; j < 2; j++) {
        lo = std::nextafter(lo, 0.0); hi = std::nextafter(hi, kInf);
        check_sincos(lo, st);
        if (hi <= 1.0e6) check_sincos(hi, st); else st.cases++;
      }
    }
    st.print("sincos k pi/2", "ulp");
  }
  {
    Stat st;
    check_sincos(0.0, st);
    check_sincos(1.0e6, st);
    double s, c;
    nid::lm::sincos_pos(0.0, &s, &c);
    if (!(s == 0.0 && c == 1.0)) st.fail("sincos(0) is not (0, 1)", 0.0);
    st.print("sincos ends", "ulp");
  }
  {  // above 1e6, NaN, inf: both NaN
    Stat st;
    const double beyond[6] = {std::nextafter(1.0e6, kInf), 1.0e7, 1.0e300, kInf, kNaN, -kNaN};
    for (double t : beyond) {
      double s = 0, c = 0;
      nid::lm::sincos_pos(t, &s, &c);
      st.cases++;
      if (!(std::isnan(s) && std::isnan(c))) st.fail("not NaN beyond 1e6", t);
    }
    st.print("sincos beyond", "(both NaN)");
  }
  std::printf("sincos worst: sin %.3f ulp at %a, cos %.3f ulp at %a\n", g_worst_sin, g_at_sin, g_worst_cos, g_at_cos);
  for (int d = kDecLo; d <= kDecHi; d++)
    std::printf("sincos decade 1e%+03d: worst sin %.3f cos %.3f ulp\n", d, g_dec_sin[d - kDecLo], g_dec_cos[d - kDecLo]);
}

// ---- se3_exp ------------------------------------------------------------------------------------------------------
void normalize_l(ld *q) {
  if (q[3] < 0) for (int i = 0; i < 4; i++) q[i] = -q[i];
  const ld n = sqrtl(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= n;
}

// se3_exp's formulas in long double, branch for branch.  theta is the DOUBLE the code computes (a long-double theta would
// charge the code theta * eps of argument rounding: 3e5 eps at 1e6); below 1e-5 it is I + Om + Om^2 as written, not the
// true exponential.
void se3_exp_l(const double *u, double theta, ld *out7) {
  const ld o0 = u[0], o1 = u[1], o2 = u[2], th = theta;
  const ld Om[9] = {0, -o2, o1, o2, 0, -o0, -o1, o0, 0};
  ld Om2[9], R[9], V[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      ld s = 0;
      for (int k = 0; k < 3; k++) s += Om[i * 3 + k] * Om[k * 3 + j];
      Om2[i * 3 + j] = s;
    }
  ld a = 1, b = 1, c = 1;
  if (!(theta < 0.00001)) {
    const ld sn = sinl(th), cs = cosl(th);
    a = sn / th; b = (1 - cs) / (th * th); c = (th - sn) / (th * th * th);
  }
  for (int i = 0; i < 9; i++) {
    const ld id = (i == 0 || i == 4 || i == 8) ? 1 : 0;
    R[i] = id + a * Om[i] + b * Om2[i];
    V[i] = theta < 0.00001 ? R[i] : id + b * Om[i] + c * Om2[i];
  }
  ld q[4], t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrtl(t + 1);
    q[3] = t / 2;
    t = 0.5L / t;
    q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrtl(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1);
    q[i] = t / 2;
    t = 0.5L / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
  normalize_l(q);
  for (int i = 0; i < 4; i++) out7[i] = q[i];
  for (int i = 0; i < 3; i++) out7[4 + i] = V[i * 3] * u[3] + V[i * 3 + 1] * u[4] + V[i * 3 + 2] * u[5];
}

struct ExpClass { const char *name; long cases; double worst_q, worst_t, worst_t_of_bound; };

// Quaternion, up to sign: 16 eps absolute.  Translation: (16 + 2 / theta) eps max(1, |t_ref|_inf) for theta >= 1e-5 -- the
// 1 / theta term is the cancellation of (1 - cos) / theta^2 in double, which the reference's own formula has -- and 16 eps
// max(1, |t_ref|_inf) below.
void check_exp(const double *u, Stat &st, ExpClass &cl) {
  double got[7];
  nid::lm::se3_exp(u, got);
  const double theta = __builtin_sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  ld ref[7];
  se3_exp_l(u, theta, ref);
  ld dp = 0, dm = 0, dt = 0, tmax = 1;
  for (int i = 0; i < 4; i++) {
    dp = fmaxl(dp, fabsl((ld)got[i] - ref[i]));
    dm = fmaxl(dm, fabsl((ld)got[i] + ref[i]));
  }
  for (int i = 4; i < 7; i++) {
    dt = fmaxl(dt, fabsl((ld)got[i] - ref[i]));
    tmax = fmaxl(tmax, fabsl(ref[i]));
  }
  const double eq = (double)(fminl(dp, dm) / kEps), et = (double)(dt / (kEps * tmax));
  const double tb = theta < 0.00001 ? 16.0 : 16.0 + 2.0 / theta;
  st.add(eq / 16.0, 1.0, "se3_exp quaternion (of 16 eps)", theta);
  st.add(et / tb, 1.0, "se3_exp translation (of its bound)", theta);
  st.cases--;
  if (!(got[3] >= 0)) st.fail("se3_exp: w < 0", theta);
  cl.cases++;
  if (eq > cl.worst_q) cl.worst_q = eq;
  if (et > cl.worst_t) cl.worst_t = et;
  if (et / tb > cl.worst_t_of_bound) cl.worst_t_of_bound = et / tb;
}

void axis_of(int kind, double *ax) {  // kind 0..2: +x, +y, +z; 3..5: -x, -y, -z; else random
  if (kind < 6) {
    ax[0] = ax[1] = ax[2] = 0;
    ax[kind % 3] = kind < 3 ? 1.0 : -1.0;
    return;
  }
  double n;
  do {
    for (int i = 0; i < 3; i++) ax[i] = normal();
    n = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  } while (!(n > 1e-3));
  for (int i = 0; i < 3; i++) ax[i] /= n;
}

void se3_exp_all() {
  Stat st;
  ExpClass classes[] = {{"zero", 0, 0, 0, 0},        {"1e-8 .. 1e-5", 0, 0, 0, 0}, {"at 1e-5", 0, 0, 0, 0},     {"1e-5 .. 1e-2", 0, 0, 0, 0},
                        {"1e-2 .. 10", 0, 0, 0, 0},  {"at k pi/2", 0, 0, 0, 0},    {"2.0 .. 2.2", 0, 0, 0, 0},  {"3.0 .. 3.3", 0, 0, 0, 0},
                        {"10 .. 1e6", 0, 0, 0, 0},   {"40, 1e3, 1e6", 0, 0, 0, 0}};
  const int ncl = (int)(sizeof(classes) / sizeof(classes[0]));
  const double fixed[3] = {40.0, 1.0e3, 1.0e6};
  for (long n = 0; n < 4000000; n++) {
    const int cl = n < 100 ? 0 : (int)(draw64() % (uint64_t)(ncl - 1)) + 1;
    const int kind = (int)(draw64() % 12);  // half axis-aligned (theta is then exactly the double asked for), half random
    double theta = 0, ax[3], u[6];
    switch (cl) {
      case 1: theta = log_uniform(1e-8, 1e-5); break;
      case 2: {
        theta = 1e-5;
        const int steps = (int)(draw64() % 9) - 4;
        for (int j = 0; j < std::abs(steps); j++) theta = std::nextafter(theta, steps < 0 ? 0.0 : 1.0);
        break;
      }
      case 3: theta = log_uniform(1e-5, 1e-2); break;
      case 4: theta = log_uniform(1e-2, 10.0); break;
      case 5: {
        theta = (double)((ld)(1 + draw64() % 8) * (kPiL / 2));
        const int steps = (int)(draw64() % 5) - 2;
        for (int j = 0; j < std::abs(steps); j++) theta = std::nextafter(theta, steps < 0 ? 0.0 : 100.0);
        break;
      }
      case 6: theta = uniform(2.0, 2.2); break;
      case 7: theta = uniform(3.0, 3.3); break;
      case 8: theta = log_uniform(10.0, 1.0e6); break;
      case 9: theta = fixed[draw64() % 3]; break;  // (1e6 about the coordinate axes only: a random axis can round it past the range)
      default: break;
    }
    axis_of(cl == 9 ? kind % 6 : kind, ax);
    for (int i = 0; i < 3; i++) { u[i] = ax[i] * theta; u[3 + i] = normal(); }
    check_exp(u, st, classes[cl]);
  }
  {  // past the range: everything of the rotation is NaN
    const double u[6] = {0, 2.0e6, 0, 0.1, 0.2, 0.3};
    double got[7];
    nid::lm::se3_exp(u, got);
    for (int i = 0; i < 4; i++)
      if (!std::isnan(got[i])) st.fail("se3_exp beyond 1e6 is not NaN", 2.0e6);
  }
  for (int k = 0; k < ncl; k++)
    std::printf("se3_exp class %s: %ld, worst quaternion %.3g eps, translation %.4g eps = %.3g of its bound\n", classes[k].name,
                classes[k].cases, classes[k].worst_q, classes[k].worst_t, classes[k].worst_t_of_bound);
  st.print("se3_exp", "of the bound");
}

// ---- se3_mul, pose_record -----------------------------------------------------------------------------------------
void random_pose(double *p) {  // a unit quaternion (to rounding) with w >= 0, a translation in [-1, 1]^3
  double n;
  do {
    for (int i = 0; i < 4; i++) p[i] = normal();
    n = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
  } while (!(n > 1e-3));
  for (int i = 0; i < 4; i++) p[i] /= p[3] < 0 ? -n : n;
  if (draw64() % 16 == 0) p[3] = (double)(draw64() % 3) * 5e-17;  // w within 1e-16 of zero
  for (int i = 4; i < 7; i++) p[i] = uniform(-1.0, 1.0);
}

// Unit quaternions, translations in [-1, 1]^3: 16 eps absolute on every component (a dozen roundings of terms below 3, the
// normalisation's two).  The sign of the result is the flip's: compared as it stands unless the true w is within 1e-14 of 0.
void se3_mul_all() {
  Stat st, flip;
  for (int n = 0; n < 200000; n++) {
    double a[7], b[7], got[7];
    random_pose(a);
    random_pose(b);
    nid::lm::se3_mul(a, b, got);
    ld q[4], t[3];
    const ld ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    q[3] = aw * bw - ax * bx - ay * by - az * bz;
    q[0] = aw * bx + ax * bw + ay * bz - az * by;
    q[1] = aw * by + ay * bw + az * bx - ax * bz;
    q[2] = aw * bz + az * bw + ax * by - ay * bx;
    const ld w_raw = q[3];
    normalize_l(q);
    // a's rotation of b's translation, from the rotation matrix of the UNNORMALISED double a (what the vector formula computes
    // is v + 2 w (u x v) + 2 u x (u x v), u = (ax, ay, az))
    const ld v[3] = {b[4], b[5], b[6]}, uv[3] = {ay * v[2] - az * v[1], az * v[0] - ax * v[2], ax * v[1] - ay * v[0]};
    const ld uuv[3] = {ay * uv[2] - az * uv[1], az * uv[0] - ax * uv[2], ax * uv[1] - ay * uv[0]};
    for (int i = 0; i < 3; i++) t[i] = (ld)a[4 + i] + v[i] + 2 * aw * uv[i] + 2 * uuv[i];
    ld dp = 0, dm = 0, dt = 0;
    for (int i = 0; i < 4; i++) {
      dp = fmaxl(dp, fabsl((ld)got[i] - q[i]));
      dm = fmaxl(dm, fabsl((ld)got[i] + q[i]));
    }
    for (int i = 0; i < 3; i++) dt = fmaxl(dt, fabsl((ld)got[4 + i] - t[i]));
    const ld dq = fabsl(w_raw) < 1e-14L ? fminl(dp, dm) : dp;
    const double e = (double)(fmaxl(dq, dt) / kEps);
    st.add(e, 16.0, "se3_mul", (double)w_raw);
    if (!(got[3] >= 0)) st.fail("se3_mul: w < 0", (double)w_raw);
    if (w_raw < -1e-3L) flip.add(e, 16.0, "se3_mul (flipped)", (double)w_raw);
  }
  st.print("se3_mul", "eps");
  flip.print("se3_mul flip", "eps");
}

// 8 eps absolute on the rotation's entries (three roundings of terms below 2 each); the translation is copied
void pose_record_all() {
  Stat st;
  for (int n = 0; n < 100000; n++) {
    double p[7], q7[7], M[12];
    int32_t mode = -1;
    random_pose(p);
    nid::lm::pose_record(p, n & 1, q7, M, &mode);
    const ld x = p[0], y = p[1], z = p[2], w = p[3];
    const ld R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                     2 * (y * z - w * x),     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
    ld d = 0;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) d = fmaxl(d, fabsl((ld)M[4 * r + c] - R[3 * r + c]));
    st.add((double)(d / kEps), 8.0, "pose_record", p[3]);
    if (std::memcmp(q7, p, sizeof(q7)) != 0 || M[3] != p[4] || M[7] != p[5] || M[11] != p[6] || mode != (n & 1)) st.fail("pose_record: q, t or mode", p[3]);
  }
  st.print("pose_record", "eps");
}

// ---- ldlt6_solve --------------------------------------------------------------------------------------------------
void unpack(const double *H21, double lambda, ld A[6][6]) {
  int k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++, k++) A[i][j] = A[j][i] = H21[k];
  for (int i = 0; i < 6; i++) A[i][i] = (ld)(H21[i * 6 - i * (i - 1) / 2] + lambda);  // (the damped diagonal as the double the code forms)
}
void pack(const double A[6][6], double *H21) {
  int k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++, k++) H21[k] = A[i][j];
}

// Gaussian elimination with full pivoting in long double: the largest remaining |entry| next, a diagonal one before an
// off-diagonal one and the lower index before the higher among equals; a remaining block that is zero (at most `tiny`)
// gives zero components.  On the positive semi-definite matrices used here the largest entry is on the diagonal, so this is
// the order "largest remaining |diagonal|, ties to the lower index" -- in exact arithmetic on the integer cases.
void gauss_full(const ld A0[6][6], const double *b, ld tiny, ld *x) {
  ld A[6][6], y[6];
  int col[6];
  for (int i = 0; i < 6; i++) { col[i] = i; y[i] = b[i]; for (int j = 0; j < 6; j++) A[i][j] = A0[i][j]; }
  int rank = 6;
  for (int k = 0; k < 6; k++) {
    int pi = k, pj = k;
    ld best = fabsl(A[k][k]);
    for (int i = k + 1; i < 6; i++)
      if (fabsl(A[i][i]) > best) { best = fabsl(A[i][i]); pi = pj = i; }
    for (int i = k; i < 6; i++)
      for (int j = k; j < 6; j++)
        if (fabsl(A[i][j]) > best) { best = fabsl(A[i][j]); pi = i; pj = j; }
    if (!(best > tiny)) { rank = k; break; }
    for (int j = 0; j < 6; j++) { const ld t = A[k][j]; A[k][j] = A[pi][j]; A[pi][j] = t; }
    { const ld t = y[k]; y[k] = y[pi]; y[pi] = t; }
    for (int i = 0; i < 6; i++) { const ld t = A[i][k]; A[i][k] = A[i][pj]; A[i][pj] = t; }
    { const int t = col[k]; col[k] = col[pj]; col[pj] = t; }
    for (int i = k + 1; i < 6; i++) {
      const ld f = A[i][k] / A[k][k];
      for (int j = k; j < 6; j++) A[i][j] -= f * A[k][j];
      y[i] -= f * y[k];
    }
  }
  ld z[6] = {0, 0, 0, 0, 0, 0};
  for (int i = rank - 1; i >= 0; i--) {
    ld s = y[i];
    for (int j = i + 1; j < rank; j++) s -= A[i][j] * z[j];
    z[i] = s / A[i][i];
  }
  for (int i = 0; i < 6; i++) x[col[i]] = z[i];
}

// the project's residual bound (check_solve_and_trial of tests/test_multistart_cpu.py): 64 eps (|A|_inf |x|_inf + |b|_inf)
double residual_of_bound(const ld A[6][6], const double *b, const double *x) {
  ld res = 0, an = 0, xn = 0, bn = 0;
  for (int i = 0; i < 6; i++) {
    ld s = -(ld)b[i], row = 0;
    for (int j = 0; j < 6; j++) { s += A[i][j] * x[j]; row += fabsl(A[i][j]); }
    res = fmaxl(res, fabsl(s)); an = fmaxl(an, row); xn = fmaxl(xn, fabsl((ld)x[i])); bn = fmaxl(bn, fabsl((ld)b[i]));
  }
  const ld bound = 64 * (ld)kEps * (an * xn + bn);
  return bound > 0 ? (double)(res / bound) : (res == 0 ? 0.0 : kInf);
}

void random_orthogonal(ld Q[6][6]) {  // Gram-Schmidt (twice) on normal columns
  for (int j = 0; j < 6; j++) {
    for (int i = 0; i < 6; i++) Q[i][j] = normal();
    for (int pass = 0; pass < 2; pass++)
      for (int k = 0; k < j; k++) {
        ld d = 0;
        for (int i = 0; i < 6; i++) d += Q[i][j] * Q[i][k];
        for (int i = 0; i < 6; i++) Q[i][j] -= d * Q[i][k];
      }
    ld n = 0;
    for (int i = 0; i < 6; i++) n += Q[i][j] * Q[i][j];
    n = sqrtl(n);
    for (int i = 0; i < 6; i++) Q[i][j] /= n;
  }
}

const double kSentinel = 7.5;
bool untouched(const double *x) {
  for (int i = 0; i < 6; i++)
    if (x[i] != kSentinel) return false;
  return true;
}

void ldlt_all() {
  {  // SPD, condition 1 .. 1e12, scale 1e-300 .. 1e300, lambda 0 or 1e-5 of the largest diagonal: success, the residual within the
     // project's bound, and x within 6 * 64 eps * cond of the reference's (backward error times the condition number; 6: norms;
     // damped, the condition is at most 6e5: lambda = 1e-5 max diagonal >= 1e-5 / 6 of the largest eigenvalue)
    Stat st, fwd;
    for (int n = 0; n < 20000; n++) {
      const double cond = std::pow(10.0, (double)(draw64() % 13)), scale = std::pow(10.0, (double)((int)(draw64() % 13) - 6) * 50.0);
      ld Q[6][6];
      random_orthogonal(Q);
      double Ad[6][6], H21[21], b[6], x[6];
      for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) {
          ld s = 0;
          for (int k = 0; k < 6; k++) {
            const ld ev = powl((ld)cond, (ld)k / 5) * (scale * cond < 1e301 ? 1.0L : 1.0L / cond);
            s += Q[i][k] * ev * Q[j][k];
          }
          Ad[i][j] = Ad[j][i] = (double)(s * scale);
        }
      pack(Ad, H21);
      double maxd = 0;
      for (int i = 0; i < 6; i++) { b[i] = normal() * scale; x[i] = kSentinel; if (Ad[i][i] > maxd) maxd = Ad[i][i]; }
      const double lambda = (n & 1) ? 1e-5 * maxd : 0.0;
      const bool ok = nid::lm::ldlt6_solve(H21, lambda, b, x);
      ld A[6][6], xr[6];
      unpack(H21, lambda, A);
      if (!ok) { st.fail("ldlt6_solve failed on an SPD matrix", cond); st.cases++; continue; }
      st.add(residual_of_bound(A, b, x), 1.0, "ldlt residual (of 64 eps (|A||x| + |b|))", cond);
      gauss_full(A, b, 0, xr);
      ld d = 0, xn = 0;
      for (int i = 0; i < 6; i++) { d = fmaxl(d, fabsl((ld)x[i] - xr[i])); xn = fmaxl(xn, fabsl(xr[i])); }
      fwd.add((double)(d / (6 * 64 * (ld)kEps * (lambda > 0 ? fminl(cond, 6e5L) : cond) * xn)), 1.0, "ldlt x against the reference", cond);
    }
    st.print("ldlt residual", "of the bound");
    fwd.print("ldlt forward error", "of the bound");
  }
  {  // every order of six distinct diagonals (every pivot-exchange pattern), small off-diagonals
    Stat st;
    int perm[6] = {0, 1, 2, 3, 4, 5};
    for (int n = 0; n < 720; n++) {
      double Ad[6][6], H21[21], b[6], x[6];
      for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) Ad[i][j] = Ad[j][i] = i == j ? 1.0 + perm[i] : 0.05 * normal();
      pack(Ad, H21);
      for (int i = 0; i < 6; i++) { b[i] = normal(); x[i] = kSentinel; }
      ld A[6][6], xr[6];
      unpack(H21, 6e-5, A);
      if (!nid::lm::ldlt6_solve(H21, 6e-5, b, x)) st.fail("ldlt6_solve failed on a diagonally dominant matrix", n);
      st.add(residual_of_bound(A, b, x), 1.0, "ldlt residual", n);
      gauss_full(A, b, 0, xr);
      for (int i = 0; i < 6; i++)
        if (!(fabsl((ld)x[i] - xr[i]) <= 64 * 6 * 10 * (ld)kEps)) st.fail("ldlt x against the reference", n);  // (cond < 10, |x| < 6)
      std::next_permutation(perm, perm + 6);
    }
    st.print("ldlt exchanges", "of the bound");
  }
  {  // equal diagonals on singular integer matrices, where the ORDER decides which basic solution comes out: the tie goes to
     // the lower index, so the zero components sit at the higher ones.  Exact arithmetic on both sides: x must be EQUAL.
    Stat st;
    // (every pivot met is a power of two: no division rounds)
    const int v1[6] = {1, 1, 1, 1, 1, 1}, v2[6] = {1, -1, 1, -1, 1, -1}, v3[6] = {1, 1, 1, 0, 0, 0}, v4[6] = {0, 0, 0, 1, 1, 1};
    const int h1[6] = {1, 1, 1, 1, 0, 0}, h2[6] = {1, -1, 1, -1, 0, 0}, h3[6] = {0, 0, 0, 0, 1, 1}, h4[6] = {0, 0, 0, 0, 1, -1};
    const int *sets[6][4] = {{v1, nullptr, nullptr, nullptr}, {v1, v2, nullptr, nullptr}, {v3, v4, nullptr, nullptr},
                             {v2, nullptr, nullptr, nullptr}, {h1, h2, h3, h4},           {h1, h2, h3, nullptr}};
    const double scales[3] = {1.0, 0.5, 1024.0};
    for (int c = 0; c < 6; c++)
      for (double s : scales) {
        double Ad[6][6] = {}, H21[21], b[6], x[6];
        for (int m = 0; m < 4 && sets[c][m]; m++)
          for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) Ad[i][j] += s * sets[c][m][i] * sets[c][m][j];
        const double xs[6] = {1, 2, 3, -1, -2, 4};
        for (int i = 0; i < 6; i++) { b[i] = 0; x[i] = kSentinel; for (int j = 0; j < 6; j++) b[i] += Ad[i][j] * xs[j]; }
        pack(Ad, H21);
        ld A[6][6], xr[6];
        unpack(H21, 0.0, A);
        gauss_full(A, b, 0, xr);
        st.cases++;
        if (!nid::lm::ldlt6_solve(H21, 0.0, b, x)) { st.fail("ldlt ties: failed", c); continue; }
        for (int i = 0; i < 6; i++)
          if ((ld)x[i] != xr[i]) { st.fail("ldlt ties: x differs from the lower-index basic solution", c); break; }
        if (residual_of_bound(A, b, x) != 0.0) st.fail("ldlt ties: residual", c);
      }
    {  // the plainest one, spelled out: ones(6, 6) x = ones has the basic solutions e_k; the tie rule picks e_0
      double Ad[6][6], H21[21], b[6] = {1, 1, 1, 1, 1, 1}, x[6];
      for (int i = 0; i < 6; i++) { x[i] = kSentinel; for (int j = 0; j < 6; j++) Ad[i][j] = 1.0; }
      pack(Ad, H21);
      st.cases++;
      if (!nid::lm::ldlt6_solve(H21, 0.0, b, x) || x[0] != 1.0 || x[1] != 0 || x[2] != 0 || x[3] != 0 || x[4] != 0 || x[5] != 0)
        st.fail("ldlt ties: ones(6, 6) x = ones is not e_0", 0);
    }
    st.print("ldlt ties", "(exact)");
  }
  {  // a negative or NaN pivot first met at k = 0 .. 5: false, x untouched
    Stat st;
    for (int k = 0; k < 6; k++)
      for (int what = 0; what < 3; what++) {
        double Ad[6][6], H21[21], b[6], x[6];
        for (int i = 0; i < 6; i++)
          for (int j = i; j < 6; j++) Ad[i][j] = Ad[j][i] = i == j ? 6.0 - i : (what == 2 ? 0.05 * normal() : 0.0);
        Ad[k][k] = what == 1 ? kNaN : -Ad[k][k];
        pack(Ad, H21);
        for (int i = 0; i < 6; i++) { b[i] = normal(); x[i] = kSentinel; }
        st.cases++;
        if (nid::lm::ldlt6_solve(H21, 6e-5, b, x)) st.fail("a negative / NaN pivot did not fail", k);
        if (!untouched(x)) st.fail("a failed solve touched x", k);
      }
    st.print("ldlt negative pivot", "(false and x untouched)");
  }
  {  // a zero or denormal pivot (|d| <= DBL_MIN): a zero component, and true
    Stat st;
    const double diags[8][6] = {{0, 0, 0, 0, 0, 0},         {1, 0, 2, 0, 3, 0},        {1e-310, 1e-310, 1e-310, 1e-310, 1e-310, 1e-310},
                                {1, 1e-310, 2, 5e-324, 3, kDblMin}, {kDblMin, 4 * kDblMin, 1, 0, 1e-320, 2}, {0, 0, 0, 0, 0, 1e300},
                                {1e-300, 0, 1e-300, 0, 1e-305, 0},  {2, 2, 0, 0, 2, 2}};
    for (int c = 0; c < 8; c++) {
      double Ad[6][6] = {}, H21[21], b[6], x[6];
      for (int i = 0; i < 6; i++) { Ad[i][i] = diags[c][i]; b[i] = (1.0 + i) * (diags[c][i] > 0 && diags[c][i] < 1e-290 ? 1e-300 : 1.0); x[i] = kSentinel; }
      pack(Ad, H21);
      st.cases++;
      if (!nid::lm::ldlt6_solve(H21, 0.0, b, x)) { st.fail("a zero pivot failed the solve", c); continue; }
      for (int i = 0; i < 6; i++) {
        const double want = std::fabs(diags[c][i]) > kDblMin ? b[i] / diags[c][i] : 0.0;
        if (!(x[i] == want)) st.fail("a zero / denormal pivot's component", c);
      }
    }
    st.print("ldlt zero pivot", "(a zero component and true)");
  }
}

}  // namespace

int main() {
  sincos_all();
  se3_exp_all();
  se3_mul_all();
  pose_record_all();
  ldlt_all();
  std::printf("%s\n", g_failures ? "FAILED" : "all within their bounds");
  return g_failures ? 1 : 0;
}

// tests/cpp/direct_sum_check.cpp -- csrc/nid_direct_sum.h (the host's half of a DIRECT launch: Huber weights, per-cell
// quadratic forms, the two cursors and the order of the additions) driven through DirectSum's non-blocking step against
// a reference written out independently below: every cell's 32-double block formed the way the evaluation kernel's tail
// forms it, then sum_blocks_w0's rule applied twice, literally -- from +0.0 the even-numbered blocks in ascending order,
// the odd-numbered ones likewise, the two added -- per group of cells and then over the groups.  All 29 entries must
// have the same bits and entries 29..31 must be +0.0, whatever order the records arrive in, down to single words.
// Built with AddressSanitizer + UndefinedBehaviorSanitizer and run by tests/test_host_cpu.py; no GPU involved.
// Exit code 0 and one summary line = everything identical.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nid_direct_sum.h"

namespace {

struct alignas(64) Rec { double w[8]; };
static_assert(sizeof(Rec) == nid::kDirectRec * sizeof(double), "one record is one 64-byte line");

uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

// ---- the reference ------------------------------------------------------------------------------------------------
// one cell's block, entry by entry: [0] rho0 | [1..6] 0 - (rho1 J[n]) err | [7..27] (J[a] rho1) J[b], a <= b, row-major
// | [28] 1 | [29..31] 0; a level-1 edge (active == 0): all +0.0
void ref_block(double err, double active, const double *J, double delta, double *blk) {
  for (int v = 0; v < 32; v++) blk[v] = 0.0;
  if (active == 0.0) return;
  const float dsqr = (float)(delta * delta);
  const double e2 = err * err;
  double rho0 = e2, rho1 = 1.0;
  if (!(e2 <= dsqr)) {
    const double s = std::sqrt(e2);
    rho0 = 2 * s * delta - dsqr;
    rho1 = delta / s;
  }
  for (int v = 0; v < 32; v++) {
    if (v == 0) blk[v] = rho0;
    else if (v == 28) blk[v] = 1.0;
    else if (v < 7) blk[v] = 0.0 - (rho1 * J[v - 1]) * err;
    else if (v < 28) {
      int k = v - 7, a = 0, len = 6;  // which (a, b) of the upper triangle
      while (k >= len) { k -= len; a++; len--; }
      blk[v] = (J[a] * rho1) * J[a + k];
    }
  }
}

// sum_blocks_w0's rule over `count` blocks of 32 doubles
void ref_sum(const double *blocks, int count, double *out) {
  for (int v = 0; v < 32; v++) {
    double even = 0.0, odd = 0.0;
    for (int c = 0; c < count; c += 2) even += blocks[(size_t)c * 32 + v];
    for (int c = 1; c < count; c += 2) odd += blocks[(size_t)c * 32 + v];
    out[v] = even + odd;
  }
}

struct Cells {
  int nloc = 0;
  std::vector<double> err, active, J;  // [nloc], [nloc], [nloc][6]
};

void reference(const Cells &C, int gs, bool jac, double delta, double *out) {
  const int ngroups = (C.nloc + gs - 1) / gs;
  std::vector<double> blocks((size_t)C.nloc * 32), groups((size_t)ngroups * 32);
  const double noJ[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // a cost-only launch has no Jacobian
  for (int c = 0; c < C.nloc; c++) ref_block(C.err[c], C.active[c], jac ? &C.J[6 * (size_t)c] : noJ, delta, &blocks[(size_t)c * 32]);
  for (int g = 0; g < ngroups; g++) ref_sum(&blocks[(size_t)g * gs * 32], std::min(gs, C.nloc - g * gs), &groups[(size_t)g * 32]);
  ref_sum(groups.data(), ngroups, out);
}

// ---- the cases ----------------------------------------------------------------------------------------------------
enum Inactive { kNone, kScattered, kWholeGroup, kAll, kInactiveModes };
enum Order { kAllPresent, kCellOrder, kJacobianFirst, kWordByWord, kOrders };

Cells make_cells(int nloc, int gs, Inactive inactive, double delta, std::mt19937_64 &rng) {
  Cells C;
  C.nloc = nloc;
  C.err.resize(nloc); C.active.resize(nloc); C.J.resize((size_t)6 * nloc);
  const float dsqr = (float)(delta * delta);
  // residuals on both sides of the Huber threshold, one ulp either side of it, and exactly on it: err * err == dsqr
  double on = std::sqrt((double)dsqr);
  for (int k = 0; k < 16 && on * on != (double)dsqr; k++) on = std::nextafter(on, on * on < (double)dsqr ? 2.0 : 0.0);
  const double below = std::nextafter(on, 0.0), above = std::nextafter(on, 2.0);
  std::uniform_real_distribution<double> uni(-1.0, 1.0);
  const int ngroups = (nloc + gs - 1) / gs;
  const int dead_group = ngroups > 1 ? 1 : 0;
  for (int c = 0; c < nloc; c++) {
    double e;
    switch (rng() % 8) {
      case 0: e = on; break;
      case 1: e = -on; break;
      case 2: e = below; break;
      case 3: e = above; break;
      case 4: e = uni(rng) * 30.0; break;   // far above the threshold
      case 5: e = uni(rng) * 1e-9; break;   // tiny
      default: e = uni(rng) * 1.5; break;   // around it
    }
    C.err[c] = e;
    bool act = true;
    if (inactive == kAll) act = false;
    if (inactive == kScattered || inactive == kWholeGroup) act = rng() % 5 != 0;
    if (inactive == kWholeGroup && c / gs == dead_group) act = false;
    C.active[c] = act ? 1.0 : 0.0;
    const int kind = (int)(rng() % 6);
    for (int n = 0; n < 6; n++) {
      double x = uni(rng);
      if (kind == 1) x = std::ldexp(x, (int)(rng() % 300) - 150);  // 300 binades; products and sums stay finite
      if (kind == 2 && n % 2) x = 0.0;
      if (kind == 3 && n % 3 == 0) x = -0.0;
      if (kind == 4) x = (n & 1) ? -0.0 : 0.0;
      C.J[6 * (size_t)c + n] = x;
    }
  }
  if (on * on != (double)dsqr) C.nloc = -1;  // (no residual sits exactly on the threshold: reported as a failure)
  return C;
}

struct Wire {  // the records as the device would write them, and how many words of each have been delivered
  const Cells &C;
  bool jac;
  std::vector<Rec> &rec;
  std::vector<int> delivered;
  Wire(const Cells &C, bool jac, std::vector<Rec> &rec) : C(C), jac(jac), rec(rec), delivered(rec.size(), 0) {}
  double word(int r, int w) const {
    if (r < C.nloc) return w == 0 ? C.err[r] : (w == 1 ? C.active[r] : 0.0);
    return w < 6 ? C.J[6 * (size_t)(r - C.nloc) + w] : 0.0;
  }
  void put_word(int r, int w) { rec[r].w[w] = word(r, w); delivered[r]++; }
  void put(int r) { for (int w = 0; w < 8; w++) put_word(r, w); }
};

long g_failures = 0;
void fail(const char *what, int nloc, bool jac, int inactive, int order, bool vec) {
  if (g_failures++ < 10) std::printf("FAIL %s: nloc %d %s inactive-mode %d order %d %s\n", what, nloc, jac ? "cost+Jacobian" : "cost", inactive, order, vec ? "avx512" : "scalar");
}

void run_case(const Cells &C, int gs, bool jac, double delta, Inactive inactive, Order order, bool vec, std::mt19937_64 &rng) {
  const int nloc = C.nloc, nrec = 2 * nloc;
  std::vector<Rec> rec((size_t)nrec);
  nid::fill_sentinel(rec[0].w, (size_t)nrec * 8);
  std::vector<double> hub((size_t)3 * nloc);
  Wire wire(C, jac, rec);
  nid::DirectSum::Blocks blocks;
  nid::DirectSum sum(blocks, rec[0].w, nloc, gs, jac, delta, jac ? hub.data() : nullptr, vec, 24);
  int m1 = 0, m2 = jac ? 0 : nloc;  // the cursors, mirrored: which record a step may have taken
  bool ok = true;
  // one step; whatever it takes must be a record every word of which has been delivered, in cursor order
  auto step = [&]() {
    const nid::DirectSum::Took t = sum.step();
    if (t == nid::DirectSum::kResidual) { if (m1 >= nloc || wire.delivered[m1] != 8) ok = false; m1++; }
    if (t == nid::DirectSum::kJacobian) { if (m2 >= m1 || wire.delivered[nloc + m2] != 8) ok = false; m2++; }
    return t;
  };
  auto drain = [&]() { while (step() != nid::DirectSum::kNothing) {} };
  if (step() != nid::DirectSum::kNothing) ok = false;  // nothing has arrived yet
  switch (order) {
    case kAllPresent:
      for (int r = 0; r < (jac ? nrec : nloc); r++) wire.put(r);
      while (!sum.done()) if (step() == nid::DirectSum::kNothing) { ok = false; break; }
      break;
    case kCellOrder:
      for (int c = 0; c < nloc; c++) {
        wire.put(c);
        if (step() != nid::DirectSum::kResidual) ok = false;
        if (jac) { wire.put(nloc + c); if (step() != nid::DirectSum::kJacobian) ok = false; }
        if (!sum.done() && step() != nid::DirectSum::kNothing) ok = false;
      }
      break;
    case kJacobianFirst:
      for (int c = 0; c < nloc; c++) {
        if (jac) { wire.put(nloc + c); if (step() != nid::DirectSum::kNothing) ok = false; }  // the Jacobian cursor never passes the residual one
        wire.put(c);
        if (step() != nid::DirectSum::kResidual) ok = false;
        if (jac && step() != nid::DirectSum::kJacobian) ok = false;
      }
      break;
    case kWordByWord: {
      std::vector<int> words;
      for (int r = 0; r < (jac ? nrec : nloc); r++) for (int w = 0; w < 8; w++) words.push_back(r * 8 + w);
      std::shuffle(words.begin(), words.end(), rng);
      for (int x : words) { wire.put_word(x / 8, x % 8); drain(); }
      break;
    }
    default: break;
  }
  if (!ok) fail("a step took or refused the wrong record", nloc, jac, inactive, order, vec);
  if (!sum.done() || m1 != nloc || m2 != nloc) { fail("not done", nloc, jac, inactive, order, vec); return; }
  if (sum.step() != nid::DirectSum::kNothing) fail("a step behind the end", nloc, jac, inactive, order, vec);
  double got[32], want[32];
  for (double &g : got) g = -1.0;
  sum.finish(got);
  reference(C, gs, jac, delta, want);
  for (int v = 0; v < 32; v++) {
    const bool same = v < 29 ? bits(got[v]) == bits(want[v]) : bits(got[v]) == 0;
    if (!same) {
      if (g_failures < 10) std::printf("entry %d: got %a, reference %a\n", v, got[v], want[v]);
      fail("sums differ", nloc, jac, inactive, order, vec);
      break;
    }
  }
  for (int r = 0; r < nrec; r++)
    for (int w = 0; w < 8; w++)
      if (bits(rec[r].w[w]) != nid::kHostSentinel) { fail("a record was not re-armed", nloc, jac, inactive, order, vec); return; }
}

}  // namespace

int main() {
  const double delta = std::sqrt(0.95);
  const int sizes[] = {1, 2, 3, 16, 17, 255, 256, 400, 1024};
  const bool have512 = nid_hostsum_have_avx512() != 0;
  std::mt19937_64 rng(20240607);
  long cases = 0, partial = 0;
  for (int nloc : sizes) {
    const int gs = nid::direct_group_size(nloc);
    if (gs < 1 || (long)gs * gs < nloc || (gs > 1 && (long)(gs - 1) * (gs - 1) >= nloc)) fail("group size rule", nloc, false, 0, 0, false);
    if (nloc % gs) partial++;
    for (int inactive = 0; inactive < kInactiveModes; inactive++) {
      const Cells C = make_cells(nloc, gs, (Inactive)inactive, delta, rng);
      if (C.nloc != nloc) { fail("no residual exactly on the Huber threshold", nloc, false, inactive, 0, false); continue; }
      for (int jac = 1; jac >= 0; jac--)
        for (int order = 0; order < kOrders; order++)
          for (int vec = 0; vec <= (have512 ? 1 : 0); vec++, cases++) run_case(C, gs, jac != 0, delta, (Inactive)inactive, (Order)order, vec != 0, rng);
    }
  }
  std::printf("direct sum: %ld cases (%ld sizes with a partial last group, %s), %ld failures\n", cases, partial,
              have512 ? "scalar and AVX-512" : "scalar only: no AVX-512 on this CPU", g_failures);
  return g_failures ? 1 : 0;
}

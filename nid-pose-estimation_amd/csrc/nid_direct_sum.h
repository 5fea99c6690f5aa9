// nid_direct_sum.h -- the HOST's half of a DIRECT launch: the record layout, the sentinel protocol, the Huber weights,
// one cell's quadratic form, and the order in which the cells' forms are added up.  Plain arithmetic, no HIP:
// nid_kernels.hip.h takes the layout constants from here, nid_capi.hip's wait_direct / wait_groups are loops around
// DirectSum::step / add_block, and tests/cpp/direct_sum_check.cpp compiles it alone against a reference written out
// independently.
//
// Every cell's workgroup writes its record -- err, J[6], an active flag: 64 bytes -- straight to pinned host memory and
// the HOST forms the Huber-weighted quadratic forms (RobustKernelHuber::robustify robust_kernel_impl.cpp:77-91 with the
// float dsqr, constructQuadraticForm base_unary_edge.hpp:56-63: the kernel's operations in the kernel's order, all IEEE)
// and adds them up in the order the in-launch reduction uses (sum_blocks_w0 twice: per group the even-numbered cells in
// ascending order plus the odd-numbered ones, then the groups likewise), so the 6x6 system has the same bits either
// way.  No word is ordered against any other: the host pre-fills the records with a sentinel no arithmetic produces and
// polls every word; a consumed record is reset on the spot.
// Every product and sum here is an operation of its own: translation units that include this header are built with
// -ffp-contract=off or for a target without fused multiply-add.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

// add_record_jac's sums with AVX-512 (nid_hostsum.cpp: host-only C++ next to this file; the same operations lane by lane)
extern "C" __attribute__((visibility("hidden"))) int nid_hostsum_have_avx512(void);
extern "C" __attribute__((visibility("hidden"))) void nid_hostsum_jac_avx512(const double *rec, double err, double rho1, double *acc);
extern "C" __attribute__((visibility("hidden"))) int nid_hostsum_take_jac_avx512(double *rec, unsigned long long sentinel, int active, double err,
                                                                                  double rho1, double *acc);

namespace nid {

// every function here is part of the latency path's one loop (wait_direct): none is to become a call
#define NID_SUM_INLINE __attribute__((always_inline)) inline

// The bit pattern the host fills a DIRECT launch's result words with before the launch (a signalling-NaN payload no
// arithmetic produces: NaN results are the canonical quiet NaN); a word that still holds it has not arrived.
constexpr unsigned long long kHostSentinel = 0x7FF4DEADBEEF5A5Aull;
// A cell's records of a DIRECT launch, one 64-byte line each, every line written by ONE store instruction (a line
// written in two instalments sat in a write combiner for ~30 us):
//   residual record [cl]:        err | 1.0 active / 0.0 level-1 edge | 0 x 6   -- sent when the cost phase is over
//   Jacobian record [nloc + cl]: J[6] | 0 | 0                                   -- cost + Jacobian launches only
constexpr int kDirectRec = 8;
// a per-cell block, a group sum and a result block: [0] chi2 | [1..6] b | [7..27] H upper, row-major | [28] count | [29..31] 0
constexpr int kSumBlock = 32, kSumChi2 = 0, kSumB = 1, kSumH = 7, kSumCount = 28, kSumUsed = 29;

// cells per first-level group of the two-level sums (the in-launch reduction's and the host's)
NID_SUM_INLINE int direct_group_size(int nloc) { return std::max(1, (int)std::ceil(std::sqrt((double)nloc))); }

NID_SUM_INLINE void fill_sentinel(double *p, size_t n) {
  unsigned long long *q = reinterpret_cast<unsigned long long *>(p);
  for (size_t i = 0; i < n; i++) q[i] = kHostSentinel;
}

// true when all `n` words at p have arrived
NID_SUM_INLINE bool words_arrived(const double *p, int n) {
  const volatile unsigned long long *q = reinterpret_cast<const volatile unsigned long long *>(p);
  for (int i = 0; i < n; i++)
    if (q[i] == kHostSentinel) return false;
  return true;
}

// One cell's quadratic form, from its record, ADDED to acc[0..28] -- exactly the 32-double block k_eval2's tail forms
// (residual_and_huber + constructQuadraticForm: the same IEEE operations on the same values) and the same addition
// sum_blocks_w0 performs.  Terms that are +0.0 by construction (an inactive cell's block, the b and H entries of a
// cost-only block) are not added: an accumulator that starts at +0.0 never holds -0.0, so x + 0.0 is x, bit for bit.
NID_SUM_INLINE void huber_weights(double err, double delta, float dsqr, double &rho0, double &rho1) {
  const double e2 = err * err;  // robust_kernel_impl.cpp:77-91 (float dsqr)
  rho0 = e2; rho1 = 1.0;
  if (!(e2 <= dsqr)) {
    const double sqrte = std::sqrt(e2);
    rho0 = 2 * sqrte * delta - dsqr;
    rho1 = delta / sqrte;
  }
}

// first half, from the record's early words (err, active flag): chi2 and the count; returns rho1 (0 for a level-1 edge)
NID_SUM_INLINE double add_record_cost(const double *rec, double delta, float dsqr, double *acc) {
  if (rec[1] == 0.0) return 0.0;  // level-1 edge
  double rho0, rho1;
  huber_weights(rec[0], delta, dsqr, rho0, rho1);
  acc[kSumChi2] += rho0;
  acc[kSumCount] += 1.0;
  return rho1;
}
// second half, from the Jacobian words: b and the upper triangle of H
NID_SUM_INLINE void add_record_jac(const double *J, double err, double rho1, double *acc) {
  for (int n = 0; n < 6; n++) acc[kSumB + n] += 0.0 - (rho1 * J[n]) * err;
  int idx = kSumH;
  for (int a = 0; a < 6; a++)
    for (int b = a; b < 6; b++, idx++) acc[idx] += (J[a] * rho1) * J[b];
}

// sum_blocks_w0's rule for blocks met in ascending order: block `index` is added to the even or to the odd half (each
// starts at +0.0), and the sum is the even half plus the odd one.  Entries [lo, hi) of the blocks.
NID_SUM_INLINE void add_block(double (*halves)[kSumBlock], int index, const double *blk, int lo, int hi) {
  double *t = halves[index & 1];
  for (int v = lo; v < hi; v++) t[v] += blk[v];
}
NID_SUM_INLINE void sum_halves(const double (*halves)[kSumBlock], int lo, int hi, double *out) {
  for (int v = lo; v < hi; v++) out[v] = halves[0][v] + halves[1][v];
}

// The sums of one DIRECT launch.  Two cursors over the cells, each in cell order.  c1: residual records (a cost +
// Jacobian kernel sends them BEFORE its Jacobian phase, so this work -- a square root and a division per cell -- is
// done while the device is still busy) -> Huber weights, chi2 (entry 0), count (entry 28).  c2 <= c1: Jacobian records
// -> b, H (entries 1..27).  Every entry has its own chain of additions, in sum_blocks_w0's order, whichever cursor
// performs it: per group the even-numbered cells in ascending order plus the odd-numbered ones, then the groups
// likewise.
struct DirectSum {
  enum Took { kNothing = 0, kResidual = 1, kJacobian = 2 };
  // The running sums: the groups' (even / odd) and, within the open group, the cells' (even / odd; chi2 and the count,
  // which the residual cursor adds, apart: g00 / g28).  The caller's, next to its DirectSum and not inside it: they are
  // indexed by a cell's parity and the AVX-512 routine is handed a pointer into them, so they live in memory -- and would
  // keep the cursors and everything else of a DirectSum there with them instead of in registers.
  struct Blocks {
    alignas(64) double top[2][kSumBlock] = {}, grp[2][kSumBlock] = {};
    double g00[2] = {0.0, 0.0}, g28[2] = {0.0, 0.0};
  };

  // records: [2][nloc][kDirectRec], 64-byte aligned; hub: 3 * nloc doubles of the caller's (per cell rho1, err, active;
  // cost + Jacobian only); vec512: nid_hostsum_take_jac_avx512 instead of the scalar loop; ahead: every consumed record
  // asks for the line `ahead` records further on (a record is a line the device has just written, i.e. a miss to memory)
  NID_SUM_INLINE DirectSum(Blocks &sums, double *records, int nloc, int group_size, bool jac, double delta, double *hub, bool vec512, int ahead)
      : sums(sums), base(records), hub(hub), nloc(nloc), gs(group_size), ahead(ahead), jac(jac), vec512(vec512), delta(delta),
        dsqr((float)(delta * delta)),  // RobustKernelHuber::setDelta (robust_kernel_impl.h:84)
        c2(jac ? 0 : nloc) {}

  NID_SUM_INLINE bool done() const { return c1 >= nloc && c2 >= nloc; }

  // consume the next record that has fully arrived, if any (never waits); says which kind it took
  NID_SUM_INLINE Took step() {
    if (c1 < nloc) {
      double *rec = base + (size_t)c1 * kDirectRec;
      if (words_arrived(rec, kDirectRec)) {
        if (c1 + ahead < nloc) __builtin_prefetch(rec + (size_t)ahead * kDirectRec, 0, 3);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);  // (the words were read as volatile; keep the plain reads below behind them)
        const int i = c1 % gs, gq = c1 / gs;
        double acc[kSumBlock];
        acc[kSumChi2] = sums.g00[i & 1]; acc[kSumCount] = sums.g28[i & 1];
        const double r1 = add_record_cost(rec, delta, dsqr, acc);
        sums.g00[i & 1] = acc[kSumChi2]; sums.g28[i & 1] = acc[kSumCount];
        if (jac) { double *w = hub + 3 * (size_t)c1; w[0] = r1; w[1] = rec[0]; w[2] = rec[1]; }
        fill_sentinel(rec, kDirectRec);
        c1++;
        if (i == gs - 1 || c1 == nloc) {  // the group is complete
          sums.top[gq & 1][kSumChi2] += sums.g00[0] + sums.g00[1];
          sums.top[gq & 1][kSumCount] += sums.g28[0] + sums.g28[1];
          sums.g00[0] = sums.g00[1] = sums.g28[0] = sums.g28[1] = 0.0;
        }
        return kResidual;
      }
    }
    if (c2 < c1) {
      double *rec = base + (size_t)(nloc + c2) * kDirectRec;
      const int i = c2 % gs, gq = c2 / gs;
      const double *w = hub + 3 * (size_t)c2;
      bool took;
      if (vec512) {  // arrival test, sums and re-arming on one load of the line (nid_hostsum.cpp)
        took = nid_hostsum_take_jac_avx512(rec, kHostSentinel, w[2] != 0.0, w[1], w[0], sums.grp[i & 1]) != 0;
        if (took && c2 + ahead < nloc) __builtin_prefetch(rec + (size_t)ahead * kDirectRec, 0, 3);
      } else {
        took = words_arrived(rec, kDirectRec);
        if (took) {
          if (c2 + ahead < nloc) __builtin_prefetch(rec + (size_t)ahead * kDirectRec, 0, 3);
          __atomic_thread_fence(__ATOMIC_ACQUIRE);
          if (w[2] != 0.0) add_record_jac(rec, w[1], w[0], sums.grp[i & 1]);
          fill_sentinel(rec, kDirectRec);
        }
      }
      if (took) {
        c2++;
        if (i == gs - 1 || c2 == nloc) {
          double g[kSumBlock];
          sum_halves(sums.grp, kSumB, kSumCount, g);
          add_block(sums.top, gq, g, kSumB, kSumCount);
          std::memset(sums.grp, 0, sizeof(sums.grp));
        }
        return kJacobian;
      }
    }
    return kNothing;
  }

  NID_SUM_INLINE void finish(double *out32) const {
    sum_halves(sums.top, 0, kSumUsed, out32);
    for (int v = kSumUsed; v < kSumBlock; v++) out32[v] = 0.0;
  }

 private:
  Blocks &sums;
  double *base, *hub;
  int nloc, gs, ahead;
  bool jac, vec512;
  double delta;
  float dsqr;
  int c1 = 0, c2;
};

}  // namespace nid

// nid_eval_launch.h -- the evaluation kernels' launch entry points, one translation unit per workgroup shape and
// kernel kind (nid_eval_tu.inc, built in parallel by __graft_entry__.build(): the ~120 instantiations of k_eval2 /
// k_resident in one translation unit took five minutes to compile, split over eight they take one).
// Plain host functions.  Each kernel is compiled in exactly one unit: two code objects with the same kernel would both
// register it, and which copy the runtime serves would be a matter of module order.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

#include "nid_kernels.hip.h"

namespace nid {

struct ResidentCtl;  // nid_resident_kernels.hip.h

// which family of k_eval2 instantiations a launch takes (launch_eval2 in nid_capi.hip decides)
enum EvalFamily {
  kFamLoop = 0,       // bin-specialised (8 / 10) or generic; EXT when P.slots_ext is set (128 / 256 threads)
  kFamDbg = 1,        // per-pixel dump / phase stamps compiled in (128 / 256 threads, generic bin count)
  kFamBig = 2,        // cells of more than 32 * NT slots (FAST, generic bin count)
  kFamLat = 3,        // the latency form (512 / 1024 threads, FAST, <= kMaxBatch poses)
  kFamStampsLat = 4,  // ... with phase stamps (generic bin count)
};

// k_repair's workgroup shape (round 6): a queued cell is redone by ONE workgroup, whose time is its number of rounds, so the
// 128-thread launches repair with kRepairThreads: five rounds of a 1200-pixel cell instead of ten (profiles/r06_flash_ab.txt).
// A repaired cell's six Jacobian sums are then added in that shape's order: within 1e-15 of the launch shape's, not its bits.
constexpr int kRepairThreads = 256;
constexpr int repair_threads(int nt) { return nt < kRepairThreads ? kRepairThreads : nt; }

// the bin count a kernel is specialised for (8, 10; 0: generic), and f(std::integral_constant<int, that count>())
constexpr int nb_spec(int nb) { return nb == 8 || nb == 10 ? nb : 0; }
template <class F> void with_nb_spec(int nb, F &&f) {
  if (nb_spec(nb) == 8) f(std::integral_constant<int, 8>());
  else if (nb_spec(nb) == 10) f(std::integral_constant<int, 10>());
  else f(std::integral_constant<int, 0>());
}

// lds_repair: the dynamic LDS of k_repair's workgroup shape (repair_threads(NT))
// eval_end: null, or an event recorded right behind k_eval2 -- in front of k_repair -- (timed launches: nid_time_kernel)
#define NID_DECLARE_EVAL_TU(NT, KIND) \
  void launch_eval_##NT##_##KIND(const EvalParams &P, int family, bool strict, size_t lds, size_t lds_repair, hipStream_t s, int batch, hipEvent_t eval_end);
NID_DECLARE_EVAL_TU(128, jac) NID_DECLARE_EVAL_TU(128, cost)
NID_DECLARE_EVAL_TU(256, jac) NID_DECLARE_EVAL_TU(256, cost)
NID_DECLARE_EVAL_TU(512, jac) NID_DECLARE_EVAL_TU(512, cost)
NID_DECLARE_EVAL_TU(1024, jac) NID_DECLARE_EVAL_TU(1024, cost)
#undef NID_DECLARE_EVAL_TU

// k_repair<kRepairThreads, ...> behind the loop-form launches of 128 and 256 threads: built by the 128-thread unit of the kind
void launch_repair_jac(const EvalParams &P, bool strict, size_t lds, hipStream_t s, int batch);
void launch_repair_cost(const EvalParams &P, bool strict, size_t lds, hipStream_t s, int batch);

// k_resident<512, NB, 3> (nid_resident_tu.hip): sets the kernel's dynamic LDS limit and launches it
void launch_resident(const EvalParams &P, int nt, size_t lds, unsigned grid, hipStream_t s, const ResidentCtl *ctl,
                         unsigned long long word0, long long idle_ticks, int xform_mode);

}  // namespace nid

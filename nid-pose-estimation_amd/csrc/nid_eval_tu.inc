// nid_eval_tu.inc -- one translation unit of evaluation kernels: workgroup shape NID_TU_NT, cost + Jacobian
// (NID_TU_JAC 1) or cost-only (0).  Included by nid_eval_nt*_*.hip; see nid_eval_launch.h.
#include "nid_eval_launch.h"

namespace nid {
namespace {

constexpr int NT = NID_TU_NT;
constexpr bool JAC = NID_TU_JAC != 0;
constexpr int RNT = repair_threads(NT);

inline dim3 eval_grid(const EvalParams &P, int batch) { return dim3((unsigned)(((P.g.nloc + 7) / 8) * 8 * batch)); }
// k_repair's grid: what fills the chip once at its two waves per SIMD, never more than the launch itself has
inline dim3 repair_grid(const EvalParams &P, int batch) {
  const unsigned launch = (unsigned)P.g.nloc * (unsigned)batch;
  const unsigned fill = 256u * 8u * 64u / (unsigned)RNT;
  return dim3(launch < fill ? launch : fill);
}

// f(NB, STRICT, EXT) for a loop-form launch: bin-specialised or generic, FAST or STRICT, records in the kernel arguments or
// (EXT: more than kMaxBatch poses, 128 / 256 threads) in device memory
template <class F>
void with_loop_kernel(const EvalParams &P, bool strict, F &&f) {
  with_nb_spec(P.g.nb, [&](auto nb) {
    auto placed = [&](auto ext) {
      if (strict) f(nb, std::true_type(), ext);
      else f(nb, std::false_type(), ext);
    };
    if constexpr (NT <= 256) { if (P.slots_ext) return placed(std::true_type()); }
    placed(std::false_type());
  });
}

// the loop form, and behind it on the same stream the kernel that does what it left in the repair queue (k_repair; usually nothing)
void launch_loop(const EvalParams &P, bool strict, size_t lds, size_t lds_repair, hipStream_t s, int batch, hipEvent_t eval_end) {
  with_loop_kernel(P, strict, [&](auto nb, auto st, auto ext) {
    hipLaunchKernelGGL((k_eval2<NT, JAC, st, nb, false, ext>), eval_grid(P, batch), dim3(NT), lds, s, P);
    if (eval_end) (void)hipEventRecord(eval_end, s);
    if constexpr (NT == kRepairThreads) (JAC ? launch_repair_jac : launch_repair_cost)(P, strict, lds_repair, s, batch);
    else hipLaunchKernelGGL((k_repair<RNT, JAC, st, nb, ext>), repair_grid(P, batch), dim3(RNT), lds_repair, s, P);
  });
}

}  // namespace

#define NID_TU_NAME2(nt, kind) launch_eval_##nt##_##kind
#define NID_TU_NAME(nt, kind) NID_TU_NAME2(nt, kind)
#if NID_TU_JAC
#define NID_TU_KIND jac
#define NID_TU_REPAIR launch_repair_jac
#else
#define NID_TU_KIND cost
#define NID_TU_REPAIR launch_repair_cost
#endif

void NID_TU_NAME(NID_TU_NT, NID_TU_KIND)(const EvalParams &P, int family, bool strict, size_t lds, size_t lds_repair, hipStream_t s, int batch, hipEvent_t eval_end) {
  const dim3 grid = eval_grid(P, batch), block(NT);
  constexpr int LAT = NT == 512 ? 3 : 2;
  switch (family) {
    case kFamLoop:
      launch_loop(P, strict, lds, lds_repair, s, batch, eval_end);
      return;  // (eval_end recorded in front of k_repair)
    case kFamDbg:  // the loop form's kernel of this shape with the diagnostics compiled in; it repairs inline, in this shape
      if constexpr (NT <= 256) {
        if (strict) hipLaunchKernelGGL((k_eval2<NT, JAC, true, 0, true>), grid, block, lds, s, P);
        else hipLaunchKernelGGL((k_eval2<NT, JAC, false, 0, true>), grid, block, lds, s, P);
      }
      break;
    case kFamBig:  // cells of more than 32 * NT slots (test geometries): FAST, generic bin count
      if constexpr (NT <= 256) {
        if (P.slots_ext) { hipLaunchKernelGGL((k_eval2<NT, JAC, false, 0, false, true, 0, true>), grid, block, lds, s, P); break; }
      }
      hipLaunchKernelGGL((k_eval2<NT, JAC, false, 0, false, false, 0, true>), grid, block, lds, s, P);
      break;
    case kFamLat:  // the latency form: 512- / 1024-thread workgroups whose LAT rounds cover the cell (FAST)
      if constexpr (NT >= 512)
        with_nb_spec(P.g.nb, [&](auto nb) { hipLaunchKernelGGL((k_eval2<NT, JAC, false, nb, false, false, LAT>), grid, block, lds, s, P); });
      break;
    case kFamStampsLat:
      if constexpr (NT >= 512) hipLaunchKernelGGL((k_eval2<NT, JAC, false, 0, true, false, LAT>), grid, block, lds, s, P);
      break;
    default:
      break;
  }
  if (eval_end) (void)hipEventRecord(eval_end, s);  // (these families repair inline: the kernel is the whole launch)
}

#if NID_TU_NT == 128
// k_repair<kRepairThreads, ...> of the 128- and 256-thread launches: this unit's code (nid_eval_launch.h)
static_assert(RNT == kRepairThreads && NT < RNT, "the unit that builds k_repair<kRepairThreads>");
void NID_TU_REPAIR(const EvalParams &P, bool strict, size_t lds, hipStream_t s, int batch) {
  with_loop_kernel(P, strict, [&](auto nb, auto st, auto ext) {
    hipLaunchKernelGGL((k_repair<RNT, JAC, st, nb, ext>), repair_grid(P, batch), dim3(RNT), lds, s, P);
  });
}
#endif

}  // namespace nid

#ifdef NID_CENSUS
#if NID_TU_NT == 128 && NID_TU_JAC
extern "C" int nid_census_read(unsigned long long *out64, int reset) {
  if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(nid::g_census), 64 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[64] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(nid::g_census), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
#endif

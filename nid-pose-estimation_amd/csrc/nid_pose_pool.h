// nid_pose_pool.h -- sizes of what ONE pose of a grid needs besides the context's shared tiles, and the memory budget of
// nid_run_sequence's fused grids.  Plain arithmetic, no HIP: nid_capi.hip's PosePool allocates by it, and
// tests/cpp/pose_pool_check.cpp compiles it alone.
#pragma once

#include <algorithm>
#include <cstddef>

namespace nid {

constexpr int kPoseBlock = 32;  // doubles of a per-cell block, a group sum and a result block (kQuad, kReducedLen)

// per pose: per-cell quadratic-form blocks and group sums (doubles), tickets ([0] top, [1 + g] groups, padded; 32-bit words)
struct PoseSizes { size_t quad, gpart, ticket; };
constexpr PoseSizes pose_sizes(int nloc, int ngroups) {
  return {(size_t)nloc * kPoseBlock, (size_t)ngroups * kPoseBlock, ((size_t)ngroups + 4 + 3) & ~(size_t)3};
}

// ---- fused grids of the pipelined loop: how many batches per grid, how many grids in flight -------------------------
// kSeqPoolBudget caps the device memory of the pipeline's pool.  Per pose: quad nloc x 32 doubles, gpart ngroups x 32
// doubles, tickets, a result block and a record (~0.5 KB together).
//   config A (640x480, 256 cells, 16 groups): 64 KB + 4 KB + 0.5 KB = 68.5 KB; a 1024-pose grid 68.5 MB; 4 in flight 274 MB
//   config B (1280x960, 1024 cells, 32 groups): 256 KB + 8 KB + 0.6 KB = 264.6 KB; a 1024-pose grid 264.6 MB; 4 in flight
//     1058 MB is over, 3 in flight 794 MB
// (the public slots of config B hold 1024 x (256 KB quad + 80 KB cellout + 8 KB gpart) = 344 MB).  Over budget at two
// grids in flight, F goes down instead -- to 1, the unfused pipeline, at worst.
constexpr int kSeqGridLimit = 1024;  // the most poses of one grid (kSeqGridMax of the kernels' header)
constexpr size_t kSeqPoolBudget = (size_t)1 << 30;
constexpr int kSeqPoolMinDepth = 2, kSeqPoolMaxDepth = 4;  // grids in flight (two streams: at least one each)

constexpr size_t seq_pool_bytes_per_pose(int nloc, int ngroups, size_t record_bytes) {
  return ((size_t)nloc + (size_t)ngroups + 1) * kPoseBlock * sizeof(double) + pose_sizes(nloc, ngroups).ticket * sizeof(unsigned) + record_bytes;
}

// batches per grid of a long sequence (1: not fused) and how many such grids are in flight
inline int seq_fusion(int nloc, int ngroups, size_t record_bytes, int batch, int *depth) {
  int F = std::max(1, kSeqGridLimit / batch);
  const size_t per_pose = seq_pool_bytes_per_pose(nloc, ngroups, record_bytes);
  while (F > 1 && (size_t)kSeqPoolMinDepth * F * batch * per_pose > kSeqPoolBudget) F--;
  *depth = (int)std::min<size_t>(kSeqPoolMaxDepth, std::max<size_t>(kSeqPoolMinDepth, kSeqPoolBudget / ((size_t)F * batch * per_pose)));
  return F;
}

}  // namespace nid

// The budget rule of nid_run_sequence's fused grids (csrc/nid_pose_pool.h: plain arithmetic, no HIP) against values
// worked out by hand from the rule's comment, for a 224-byte argument record (nid_capi.hip asserts that size):
//   per pose = (nloc + ngroups + 1) x 32 doubles (per-cell blocks, group sums, one result block)
//            + ((ngroups + 4 + 3) & ~3) ticket words + the record
//   F = 1024 / batch, lowered until two grids of F x batch poses fit 2^30 bytes (never below 1)
//   grids in flight = 2^30 / (F x batch x per pose), kept within [2, 4]
// Exit code 0: all as expected.
#include <cstdio>

#include "nid_pose_pool.h"

int main() {
  constexpr size_t kRecord = 224, kBudget = (size_t)1 << 30;
  int bad = 0;
  struct Case { int nloc, ngroups; size_t bytes; int batch, F, depth; };
  const Case cases[] = {
      // config A, 256 cells in 16 groups: 273 x 256 + 20 x 4 + 224
      {256, 16, 70192, 256, 4, 4},   // 2 x 1024 x 70192 = 144 MB fits; 2^30 / (1024 x 70192) = 14 -> 4
      {256, 16, 70192, 16, 64, 4},   // the same 1024-pose grid from 64 batches
      // config B, 1024 cells in 32 groups: 1057 x 256 + 36 x 4 + 224
      {1024, 32, 270960, 256, 4, 3},  // 2 x 1024 x 270960 = 555 MB fits; 2^30 / (1024 x 270960) = 3.87 -> 3
      // 4096 cells in 64 groups: 4161 x 256 + 68 x 4 + 224
      {4096, 64, 1065712, 256, 1, 3},  // two 512-pose grids are 1091 MB: over; F = 1; 2^30 / (256 x 1065712) = 3.94 -> 3
      {4096, 64, 1065712, 64, 7, 2},   // 2 x F x 64 x 1065712 <= 2^30 up to F = 7 (8: 1091 MB); 2^30 / (448 x 1065712) = 2.25 -> 2
  };
  for (const Case &c : cases) {
    const size_t bytes = nid::seq_pool_bytes_per_pose(c.nloc, c.ngroups, kRecord);
    int depth = -1;
    const int F = nid::seq_fusion(c.nloc, c.ngroups, kRecord, c.batch, &depth);
    if (bytes != c.bytes || F != c.F || depth != c.depth) {
      std::printf("nloc %d ngroups %d batch %d: %zu bytes per pose, F %d, %d in flight; expected %zu, %d, %d\n", c.nloc, c.ngroups, c.batch,
                  bytes, F, depth, c.bytes, c.F, c.depth);
      bad++;
    }
  }
  // the sizes the pools allocate by are the terms of the per-pose figure
  {
    const nid::PoseSizes z = nid::pose_sizes(256, 16);
    if (z.quad != 256 * 32 || z.gpart != 16 * 32 || z.ticket != 20) { std::printf("pose_sizes(256, 16): %zu %zu %zu\n", z.quad, z.gpart, z.ticket); bad++; }
    if (nid::pose_sizes(1, 1).ticket != 8 || nid::pose_sizes(4096, 64).ticket != 68) { std::printf("ticket words\n"); bad++; }
  }
  // invariants over a sweep of geometries (square grids of 1 .. 100^2 cells, groups of ~sqrt(nloc) cells as nid_create
  // forms them) and every batch a call may pass
  for (int side = 1; side <= 100; side += (side < 20 ? 1 : 7)) {
    const int nloc = side * side;
    int gs = 1;
    while (gs * gs < nloc) gs++;
    const int ngroups = (nloc + gs - 1) / gs;
    const size_t bytes = nid::seq_pool_bytes_per_pose(nloc, ngroups, kRecord);
    for (int batch = 1; batch <= 256; batch++) {
      int depth = -1;
      const int F = nid::seq_fusion(nloc, ngroups, kRecord, batch, &depth);
      const bool ok = F >= 1 && F * batch <= 1024 && depth >= 2 && depth <= 4 && (F == 1 || (size_t)2 * F * batch * bytes <= kBudget) &&
                      (depth == 2 || (size_t)depth * F * batch * bytes <= kBudget);
      if (!ok) {
        if (bad < 20) std::printf("nloc %d ngroups %d batch %d: F %d, %d in flight (%zu bytes per pose)\n", nloc, ngroups, batch, F, depth, bytes);
        bad++;
      }
    }
  }
  if (bad == 0) std::printf("pose pool rule ok\n");
  return bad ? 1 : 0;
}

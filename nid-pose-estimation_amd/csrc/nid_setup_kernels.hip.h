// nid_setup_kernels.hip.h -- the once-per-pair kernels: back-projection + tiling, the target image's margins, the reference
// stage at the initial pose (k_href), the plain-histogram program (k_plain_nid), untiling of the per-pixel outputs, the
// next pyramid level (k_pyr_down; one plane of it: k_pyr_down_u8, k_pyr_down_depth), the depth-consistency check of the
// keyframe's points against the target's depth (k_depth_check), the reference mask (k_refmask_classify,
// k_refmask_dilate_apply), the reference fill (k_reffill_splat, k_reffill_apply), the reference fusion (k_reffuse_apply), the
// bilinear gather of the same fusion (k_refgather_apply).
// Streaming kernels, not on the iteration path.  Included by ONE translation unit (nid_capi.hip), which launches them.
#pragma once

#include "nid_depth_check.h"
#include "nid_kernels.hip.h"
#include "nid_reffill_rule.h"
#include "nid_reffuse_rule.h"
#include "nid_refgather_rule.h"

namespace nid {

// ---------------------------------------------------------------------------
// Setup: back-projection + tiling.  Calculate3DpointKernel (CudaPoints3d.cu:5-32)
// == Get3dPointAndIntensity (NID_pose_estimation.cpp:401-432) folded into the
// cell-major tile writer.  One thread per tile slot.
__global__ void k_tile(Geometry g, const double *__restrict__ depth,
                       const double *__restrict__ points_in, const uint8_t *__restrict__ im0,
                       const double *__restrict__ Twc /*col-major 16*/, Tiles t,
                       double *__restrict__ points_out /*3N or null*/) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)g.nloc * g.pstride;
  if (gid >= total) return;
  const int cl = (int)(gid / g.pstride);
  const int s = (int)(gid % g.pstride);
  double X = NAN, Y = NAN, Z = NAN;
  int jr = -1;
  uint8_t i0 = 0;
  if (s < g.ps) {
    const int c = g.cell_begin + cl * g.cell_stride;
    const int ci = c / g.cell_num, cj = c % g.cell_num;
    const int r = ci * g.rb + s / g.cb;
    const int col = cj * g.cb + s % g.cb;
    const long id = (long)r * g.cols + col;
    i0 = im0[id];
    bool valid;
    if (depth) {
      valid = dc::backproject(depth[id], r, col, g.fx, g.fy, g.cx, g.cy, Twc, &X, &Y, &Z);  // (shared with nid_refmask.h's rule)
      if (points_out) {
        points_out[3 * id] = X; points_out[3 * id + 1] = Y; points_out[3 * id + 2] = Z;
      }
    } else {
      X = points_in[3 * id]; Y = points_in[3 * id + 1]; Z = points_in[3 * id + 2];
      valid = !(isnan(X) || isnan(Y) || isnan(Z));  // computeH.cu:145
      if (!valid) { X = NAN; Y = NAN; Z = NAN; }
    }
    if (valid) {
      double obs = (double)i0;  // types_six_dof_expmap.cpp:553-559
      if (obs >= 255) obs = 254.999;
      const double bin_pos_ref = obs * (double)g.S / 255.0;
      jr = (int)floor(bin_pos_ref);
    }
  }
  t.X[gid] = X; t.Y[gid] = Y; t.Z[gid] = Z;
  t.JR[gid] = (int8_t)jr;
  t.I0[gid] = i0;
}

// The driver's depth map as it comes off the disk: u16 at 1/5000 m (NID_pose_estimation.cpp:73,106:
// depth.convertTo(depth, CV_64F, depth_factor) -- one IEEE multiplication per pixel, no contraction) -> the f64 metres
// k_tile / k_backproject_plain read.  nid_set_pair_u16: 0.6 MB cross PCIe instead of 2.5 MB.
__global__ void k_depth_u16(long n, const uint16_t *__restrict__ src, double factor, double *__restrict__ dst) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id < n) dst[id] = (double)src[id] * factor;
}

// Target image for the evaluation kernel: int16 copy of the u8 image with the extrapolated top / left margin
// (see Win).  dst is (rows + 1) x stride; one thread per destination element of the first `cols + 1` columns.
__global__ void k_im1_margins(int rows, int cols, int stride, const uint8_t *__restrict__ src, int16_t *__restrict__ dst) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)(rows + 1) * (cols + 1)) return;
  const int r = (int)(gid / (cols + 1)) - 1, c = (int)(gid % (cols + 1)) - 1;
  auto at = [&](int rr, int cc) { return (int)src[(size_t)rr * cols + cc]; };
  auto col_m1 = [&](int rr) { return cols > 1 ? 2 * at(rr, 0) - at(rr, 1) : at(rr, 0); };
  int v;
  if (r >= 0 && c >= 0) v = at(r, c);
  else if (r >= 0) v = col_m1(r);
  else if (c >= 0) v = rows > 1 ? 2 * at(0, c) - at(1, c) : at(0, c);
  else v = rows > 1 ? 2 * col_m1(0) - col_m1(1) : col_m1(0);  // corner: never read with a non-zero weight
  dst[(size_t)(r + 1) * stride + (c + 1)] = (int16_t)v;
}

// Pyramid level l+1 from level l on the device (nid_pyr.h): all three planes in one launch, the arithmetic of
// nid_pyr_down_u8 / nid_pyr_down_depth_u16 (host/nid_pyramid.cpp) operation for operation -- images (a + b + c + d + 2) >> 2;
// depth: the mean of the VALID samples (metres = (double)count * factor, one IEEE product, valid as in k_tile) rounded
// half up in unsigned integers, 0 if none is valid -- so the planes are the host's, byte for byte.  The source is
// (2 rows2) x (2 cols2).  One thread makes kPyrRun adjacent output pixels of every plane: 8 source bytes of two image
// rows, 16 of two depth rows, one 4-byte and one 8-byte store per plane; the last pixels of a row whose width is no
// multiple of kPyrRun are made one by one.  Rows of a level are cols2 elements apart -- a multiple of nothing --, so every
// wide access goes through memcpy with the element's alignment and the compiler picks the instruction.
constexpr int kPyrRun = 4;
__device__ inline uint16_t pyr_depth_mean(const uint16_t v[4], double factor) {
  unsigned sum = 0, n = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double z = (double)v[k] * factor;
    if (!(z < 0.01 || z > 100)) { sum += v[k]; n++; }
  }
  return n ? (uint16_t)((2 * sum + n) / (2 * n)) : (uint16_t)0;
}

// kPyrRun image pixels of one plane: 8 bytes of each of the two source rows a and b -> 4 packed output bytes
__device__ inline unsigned pyr_box4(const uint8_t *a, const uint8_t *b) {
  unsigned long long ra, rb;
  __builtin_memcpy(&ra, a, 8);
  __builtin_memcpy(&rb, b, 8);
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < kPyrRun; k++) {
    const unsigned s = (unsigned)((ra >> (16 * k)) & 0xff) + (unsigned)((ra >> (16 * k + 8)) & 0xff) +
                       (unsigned)((rb >> (16 * k)) & 0xff) + (unsigned)((rb >> (16 * k + 8)) & 0xff);
    o |= ((s + 2) >> 2) << (8 * k);
  }
  return o;
}

__global__ void __launch_bounds__(256) k_pyr_down(int rows2, int cols2, const uint8_t *__restrict__ im0, const uint8_t *__restrict__ im1,
                                                  const uint16_t *__restrict__ depth, double factor, uint8_t *__restrict__ o_im0,
                                                  uint8_t *__restrict__ o_im1, uint16_t *__restrict__ o_depth) {
  const int runs = (cols2 + kPyrRun - 1) / kPyrRun;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)rows2 * runs) return;
  const int r = (int)(gid / runs), c0 = (int)(gid % runs) * kPyrRun;
  const size_t cols = 2 * (size_t)cols2;
  const size_t top = (size_t)(2 * r) * cols + 2 * (size_t)c0;  // source: rows 2r and 2r + 1, from column 2 c0
  const size_t out = (size_t)r * cols2 + c0;
  if (c0 + kPyrRun <= cols2) {
    const unsigned p0 = pyr_box4(im0 + top, im0 + top + cols), p1 = pyr_box4(im1 + top, im1 + top + cols);
    __builtin_memcpy(o_im0 + out, &p0, 4);
    __builtin_memcpy(o_im1 + out, &p1, 4);
    uint16_t da[2 * kPyrRun], db[2 * kPyrRun], od[kPyrRun];
    __builtin_memcpy(da, depth + top, sizeof(da));
    __builtin_memcpy(db, depth + top + cols, sizeof(db));
#pragma unroll
    for (int k = 0; k < kPyrRun; k++) {
      const uint16_t v[4] = {da[2 * k], da[2 * k + 1], db[2 * k], db[2 * k + 1]};
      od[k] = pyr_depth_mean(v, factor);
    }
    __builtin_memcpy(o_depth + out, od, sizeof(od));
  } else {
    for (int k = 0; c0 + k < cols2; k++) {
      const size_t s = top + 2 * (size_t)k;
      o_im0[out + k] = (uint8_t)((im0[s] + im0[s + 1] + im0[s + cols] + im0[s + cols + 1] + 2) >> 2);
      o_im1[out + k] = (uint8_t)((im1[s] + im1[s + 1] + im1[s + cols] + im1[s + cols + 1] + 2) >> 2);
      const uint16_t v[4] = {depth[s], depth[s + 1], depth[s + cols], depth[s + cols + 1]};
      o_depth[out + k] = pyr_depth_mean(v, factor);
    }
  }
}

// The one-plane forms of k_pyr_down (nid_pyr_stream.h: a new target alone, a new reference's depth alone): the same thread
// map, arithmetic and access form, plane for plane.  The source is (2 rows2) x (2 cols2).
__global__ void __launch_bounds__(256) k_pyr_down_u8(int rows2, int cols2, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst) {
  const int runs = (cols2 + kPyrRun - 1) / kPyrRun;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)rows2 * runs) return;
  const int r = (int)(gid / runs), c0 = (int)(gid % runs) * kPyrRun;
  const size_t cols = 2 * (size_t)cols2;
  const size_t top = (size_t)(2 * r) * cols + 2 * (size_t)c0;
  const size_t out = (size_t)r * cols2 + c0;
  if (c0 + kPyrRun <= cols2) {
    const unsigned p = pyr_box4(src + top, src + top + cols);
    __builtin_memcpy(dst + out, &p, 4);
  } else {
    for (int k = 0; c0 + k < cols2; k++) {
      const size_t s = top + 2 * (size_t)k;
      dst[out + k] = (uint8_t)((src[s] + src[s + 1] + src[s + cols] + src[s + cols + 1] + 2) >> 2);
    }
  }
}

__global__ void __launch_bounds__(256) k_pyr_down_depth(int rows2, int cols2, const uint16_t *__restrict__ depth, double factor,
                                                        uint16_t *__restrict__ o_depth) {
  const int runs = (cols2 + kPyrRun - 1) / kPyrRun;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)rows2 * runs) return;
  const int r = (int)(gid / runs), c0 = (int)(gid % runs) * kPyrRun;
  const size_t cols = 2 * (size_t)cols2;
  const size_t top = (size_t)(2 * r) * cols + 2 * (size_t)c0;
  const size_t out = (size_t)r * cols2 + c0;
  if (c0 + kPyrRun <= cols2) {
    uint16_t da[2 * kPyrRun], db[2 * kPyrRun], od[kPyrRun];
    __builtin_memcpy(da, depth + top, sizeof(da));
    __builtin_memcpy(db, depth + top + cols, sizeof(db));
#pragma unroll
    for (int k = 0; k < kPyrRun; k++) {
      const uint16_t v[4] = {da[2 * k], da[2 * k + 1], db[2 * k], db[2 * k + 1]};
      od[k] = pyr_depth_mean(v, factor);
    }
    __builtin_memcpy(o_depth + out, od, sizeof(od));
  } else {
    for (int k = 0; c0 + k < cols2; k++) {
      const size_t s = top + 2 * (size_t)k;
      const uint16_t v[4] = {depth[s], depth[s + 1], depth[s + cols], depth[s + cols + 1]};
      o_depth[out + k] = pyr_depth_mean(v, factor);
    }
  }
}

// The depth-consistency check (nid/nid_keyframe.h): ONE workgroup per (cell, pose), pose-major -- with a cell count that is
// a multiple of the XCDs, a cell's tile is read by one XCD for every pose and can stay in its L2 --, 256 lanes striding over
// the cell's pstride slots (a multiple of 64, not of 256: the loop is bounded on the slot).  X / Y / Z are coalesced f64
// reads, the u16 depth gather stays inside the cell's footprint moved by the pose.  Each lane runs dc::sample
// (nid_depth_check.h: the host's text) into six 32-bit counts and one 64-bit sum; the wave sums them with shuffles, the
// four waves meet in LDS, lanes 0 .. 6 write the cell's 32-byte record with plain stores and add their sum to the pose's
// totals with ONE 64-bit INTEGER atomic each (exact and order-independent: no float is summed anywhere).
struct DepthCheckArgs {
  const double *M;              // [n][12]: rows of [R|t] per pose (lm::pose_record)
  const uint16_t *d1;           // level 0's target depth, rows x cols
  double factor, tol_abs, tol_rel;
  nid_depth_cell *cells;        // [n][nloc]
  unsigned long long *totals;   // [n][8]: nid_depth_counts, zero before the launch
};
static_assert(sizeof(nid_depth_cell) == 32 && sizeof(nid_depth_counts) == 64, "nid_keyframe.h's records");
static_assert(offsetof(nid_depth_cell, n_through) == 20 && offsetof(nid_depth_cell, sum_abs_um) == 24, "six counts, then the sum");
static_assert(offsetof(nid_depth_counts, sum_abs_um) == 48, "a total is the cell record's members widened, in its order");

__global__ void __launch_bounds__(256) k_depth_check(Geometry g, Tiles t, DepthCheckArgs A) {
  __shared__ unsigned long long part[4][8];
  const int cl = (int)(blockIdx.x % (unsigned)g.nloc), pose = (int)(blockIdx.x / (unsigned)g.nloc), tid = threadIdx.x;
  const dc::View V = dc::make_view(g, A.M + (size_t)pose * 12, A.d1, A.factor, A.tol_abs, A.tol_rel);
  nid_depth_cell a = {};
  const size_t base = (size_t)cl * g.pstride;
  for (int s = tid; s < g.pstride; s += 256) dc::sample(V, t.X[base + s], t.Y[base + s], t.Z[base + s], &a);
  int cnt[6] = {a.n_ref, a.n_inframe, a.n_both, a.n_consistent, a.n_occluded, a.n_through};
  unsigned long long um = a.sum_abs_um;
#pragma unroll
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int k = 0; k < 6; k++) cnt[k] += __shfl_down(cnt[k], o, 64);
    um += __shfl_down(um, o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 6; k++) part[tid >> 6][k] = (unsigned long long)cnt[k];
    part[tid >> 6][6] = um;
  }
  __syncthreads();
  if (tid < 7) {
    const unsigned long long s = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
    nid_depth_cell *out = A.cells + ((size_t)pose * g.nloc + cl);
    if (tid < 6) reinterpret_cast<int32_t *>(out)[tid] = (int32_t)s;
    else out->sum_abs_um = s;
    atomicAdd(A.totals + (size_t)pose * 8 + tid, s);
  }
}

// The int counts of a 256-lane workgroup into a call's totals (the mask's and the fill's kernels): each of a lane's K counts
// summed over the wave with shuffles, the four waves' sums through `part` in LDS behind ONE barrier -- every lane of the
// workgroup calls this --, and lanes 0 .. K - 1 add the workgroup's sums to words Off .. Off + K - 1 of `totals` with ONE
// 64-bit INTEGER atomic each (exact, order-independent).  The counts come as scalar arguments: behind a reference to an
// array of them the compiler kept the callers' pixel-loop counters in 64 bits (7 and 4 more VGPRs).
template <int Off, int W, class... Ints>
__device__ __forceinline__ void counts_to_totals(unsigned long long (&part)[4][W], int tid, unsigned long long *totals, Ints... counts) {
  constexpr int K = (int)sizeof...(Ints);
  int cnt[K] = {counts...};
  static_assert(K <= W && Off + K <= 8, "a wave's row of part, the totals' eight words");
#pragma unroll
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; k++) cnt[k] += __shfl_down(cnt[k], o, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++) part[tid >> 6][k] = (unsigned long long)cnt[k];
  }
  __syncthreads();
  if (tid < K) atomicAdd(totals + Off + tid, part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid]);
}

// The reference mask (nid/nid_refmask.h), two kernels behind each other on one stream.
//
// k_refmask_classify: image order, one lane per pixel of level 0 -- the pristine u16 depth and the u8 plane are read and
// the classified byte is written at the lane's own index (coalesced); the one gather is the target depth where the
// pixel's point projects.  Each lane runs dc::mask_classified (nid_depth_check.h: the host's text): the set-up's
// back-projection of the PRISTINE depth, the check's class, the byte.  `work` is a plane of its own: the next kernel reads
// neighbours' bytes of it while it writes the final plane.
struct RefMaskArgs {
  double M[12];         // rows of [R|t] of the pose (lm::pose_record)
  const uint16_t *d0;   // the keyframe's pristine depth, rows x cols
  const double *Twc;    // its camera -> world matrix, column-major 16
  const uint16_t *d1;   // the target's depth, rows x cols
  double factor0, factor1, tol_abs, tol_rel;
  int classes, accumulate;
};
static_assert(sizeof(nid_refmask_counts) == 64, "nid_refmask.h's record");

__global__ void __launch_bounds__(256) k_refmask_classify(Geometry g, RefMaskArgs A, const uint8_t *__restrict__ mask, uint8_t *__restrict__ work) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)g.rows * g.cols) return;
  const dc::View V = dc::make_view(g, A.M, A.d1, A.factor1, A.tol_abs, A.tol_rel);
  const dc::Keyframe K = {A.d0, A.factor0, A.Twc};
  work[id] = dc::mask_classified(V, K, (int)(id / g.cols), (int)(id % g.cols), mask[id], A.classes, A.accumulate);
}

// k_refmask_dilate_apply: ONE workgroup per kRmTileH x kRmTileW image tile (a wave is one tile row: its byte and u16
// accesses are 64 adjacent elements).  The flags "the classified byte carries bit 2 or 4" of the tile and its halo of
// NID_REFMASK_MAX_DILATE -- zero outside the image, which clips the window -- go to LDS; the dilation is separable: rows
// (every tile row and halo row), then columns.  Each lane then makes four pixels: the final byte (dc::mask_final), the
// masked depth pristine-or-0 of level 0 in the same pass, and the pixel's counts (dc::mask_count).  The counts -- six of
// nid_refmask_counts and the non-zero bytes -- are summed over the wave with shuffles, over the four waves in LDS, and
// lanes 0 .. 6 add them to the call's totals with ONE 64-bit INTEGER atomic each (exact, order-independent).
constexpr int kRmTileW = 64, kRmTileH = 16, kRmHalo = NID_REFMASK_MAX_DILATE;
constexpr int kRmCountWords = 7;  // n_valid, n_caller, n_occluded, n_through, n_dilated, n_masked, non-zero bytes
static_assert(kRmTileW * 4 == 256 && kRmTileH % 4 == 0, "256 lanes: a wave per tile row, four passes");

__global__ void __launch_bounds__(256) k_refmask_dilate_apply(int rows, int cols, int dilate, const uint8_t *__restrict__ work,
                                                              const uint16_t *__restrict__ pristine, double factor,
                                                              uint8_t *__restrict__ mask, uint16_t *__restrict__ depth,
                                                              unsigned long long *__restrict__ totals /*[8], zero before the launch*/) {
  constexpr int SW = kRmTileW + 2 * kRmHalo, SH = kRmTileH + 2 * kRmHalo;
  __shared__ uint8_t src[SH][SW];
  __shared__ uint8_t rowd[SH][kRmTileW];
  __shared__ unsigned long long part[4][8];
  const int tid = threadIdx.x;
  const int r0 = (int)blockIdx.y * kRmTileH, c0 = (int)blockIdx.x * kRmTileW;
  const int d = dilate < 0 ? 0 : (dilate > kRmHalo ? kRmHalo : dilate);
  for (int e = tid; e < SH * SW; e += 256) {
    const int lr = e / SW, lc = e % SW;
    const int r = r0 - kRmHalo + lr, c = c0 - kRmHalo + lc;
    uint8_t f = 0;
    if (r >= 0 && r < rows && c >= 0 && c < cols) f = (work[(size_t)r * cols + c] & dc::kClassBits) ? 1 : 0;
    src[lr][lc] = f;
  }
  __syncthreads();
  for (int e = tid; e < SH * kRmTileW; e += 256) {
    const int lr = e / kRmTileW, lc = e % kRmTileW;
    uint8_t f = 0;
    for (int k = -d; k <= d; k++) f |= src[lr][lc + kRmHalo + k];
    rowd[lr][lc] = f;
  }
  __syncthreads();
  nid_refmask_counts n = {};
  int nonzero = 0;
  for (int e = tid; e < kRmTileH * kRmTileW; e += 256) {
    const int lr = e / kRmTileW, lc = e % kRmTileW;
    const int r = r0 + lr, c = c0 + lc;
    if (r >= rows || c >= cols) continue;
    uint8_t f = 0;
    for (int k = -d; k <= d; k++) f |= rowd[lr + kRmHalo + k][lc];
    const size_t i = (size_t)r * cols + c;
    const uint8_t b = dc::mask_final(work[i], d > 0 && f);
    const uint16_t z = pristine[i];
    mask[i] = b;
    depth[i] = b ? (uint16_t)0 : z;
    dc::mask_count(b, dc::depth_valid(z, factor), &n);
    nonzero += b != 0;
  }
  counts_to_totals<0>(part, tid, totals, (int)n.n_valid, (int)n.n_caller, (int)n.n_occluded, (int)n.n_through, (int)n.n_dilated, (int)n.n_masked, nonzero);
}

// The reference fill (nid/nid_reffill.h), two kernels behind each other on one stream, in front of the masking calls' chain.
//
// k_reffill_splat: image order, one lane per TARGET pixel of level 0 -- the u16 depth is read at the lane's own index
// (coalesced); the one scatter is a 32-bit atomicMin into the keyframe's z-buffer (0xFF bytes before the launch) where
// rf::splat (nid_reffill_rule.h: the host's text) sends the pixel.  n_target_valid and n_splat are summed over the wave with
// shuffles, over the four waves in LDS, and lanes 0 and 1 add them to the call's totals with ONE 64-bit INTEGER atomic
// each.  Every lane reaches the shuffles: a lane past the image counts nothing.
struct RefFillArgs {
  double M[12];        // rows of [R|t], target camera -> keyframe camera (rf::target_to_keyframe)
  const uint16_t *d1;  // the target's depth, rows x cols
  double factor1, factor0;
};
static_assert(sizeof(nid_reffill_counts) == 64 && offsetof(nid_reffill_counts, n_hit) == 16, "nid_reffill.h's record: the splat's two counts, then the apply's five");

__global__ void __launch_bounds__(256) k_reffill_splat(Geometry g, RefFillArgs A, uint32_t *__restrict__ zbuf,
                                                       unsigned long long *__restrict__ totals /*[8], zero before the launch*/) {
  __shared__ unsigned long long part[4][2];
  const int tid = threadIdx.x;
  const long id = (long)blockIdx.x * blockDim.x + tid;
  int cnt[2] = {0, 0};
  if (id < (long)g.rows * g.cols) {
    const rf::Splat S = rf::make_splat(g, A.M, A.d1, A.factor1, A.factor0);
    size_t idx = 0;
    uint32_t q = 0;
    const int k = rf::splat(S, (int)(id / g.cols), (int)(id % g.cols), &idx, &q);
    cnt[0] = k >= 1;
    cnt[1] = k == 2;
    if (k == 2) atomicMin(zbuf + idx, q);  // (idx < rows cols: rf::splat's frame test)
  }
  counts_to_totals<0>(part, tid, totals, cnt[0], cnt[1]);
}

// k_reffill_apply: ONE workgroup per kRmTileH x kRmTileW image tile, a wave per tile row, as k_refmask_dilate_apply.  The
// surface counts S(p) (rf::surface) of the tile and its halo of NID_REFFILL_MAX_GUARD -- none outside the image, which
// clips the window -- go to LDS as 32-bit words.  Each lane then makes four pixels: the guard's window where the pixel's
// fill hangs on it (rf::guard_decides, rf::behind), the fill (rf::apply) written over the plane's old value, the new
// pristine depth fill-or-uploaded for the masking chain behind this kernel, and the pixel's five counts -- summed like the
// mask's and added to words 2 .. 6 of the call's totals with ONE 64-bit INTEGER atomic each.
constexpr int kRfHalo = NID_REFFILL_MAX_GUARD;

__global__ void __launch_bounds__(256) k_reffill_apply(int rows, int cols, int guard, int guard_abs, int guard_rel_1024, int accumulate,
                                                       const uint32_t *__restrict__ zbuf, const uint16_t *__restrict__ uploaded, double factor0,
                                                       uint16_t *__restrict__ fill, uint16_t *__restrict__ pristine,
                                                       unsigned long long *__restrict__ totals /*[8]: words 2 .. 6*/) {
  constexpr int SW = kRmTileW + 2 * kRfHalo, SH = kRmTileH + 2 * kRfHalo;
  __shared__ uint32_t surf[SH][SW];
  __shared__ unsigned long long part[4][8];
  const int tid = threadIdx.x;
  const int r0 = (int)blockIdx.y * kRmTileH, c0 = (int)blockIdx.x * kRmTileW;
  const int d = guard < 0 ? 0 : (guard > kRfHalo ? kRfHalo : guard);
  for (int e = tid; e < SH * SW; e += 256) {
    const int lr = e / SW, lc = e % SW;
    const int r = r0 - kRfHalo + lr, c = c0 - kRfHalo + lc;
    uint32_t s = rf::kNone;
    if (r >= 0 && r < rows && c >= 0 && c < cols) {
      const size_t i = (size_t)r * cols + c;
      s = rf::surface(zbuf[i], uploaded[i], factor0);
    }
    surf[lr][lc] = s;
  }
  __syncthreads();
  nid_reffill_counts n = {};
  for (int e = tid; e < kRmTileH * kRmTileW; e += 256) {
    const int lr = e / kRmTileW, lc = e % kRmTileW;
    const int r = r0 + lr, c = c0 + lc;
    if (r >= rows || c >= cols) continue;
    const size_t i = (size_t)r * cols + c;
    const uint32_t z = zbuf[i];
    const uint16_t up = uploaded[i], old = fill[i];
    const bool valid = dc::depth_valid(up, factor0);
    bool refused = false;
    if (d > 0 && rf::guard_decides(valid, old, z != rf::kNone, accumulate)) {
      for (int dr = -d; dr <= d; dr++)
        for (int dc_ = -d; dc_ <= d; dc_++) {
          if (dr == 0 && dc_ == 0) continue;
          const uint32_t qn = surf[lr + kRfHalo + dr][lc + kRfHalo + dc_];
          refused |= qn != rf::kNone && rf::behind(z, qn, guard_abs, guard_rel_1024);
        }
    }
    const uint16_t f = rf::apply(valid, old, z, refused, accumulate, &n);
    fill[i] = f;
    pristine[i] = f ? f : up;
  }
  counts_to_totals<2>(part, tid, totals, (int)n.n_hit, (int)n.n_holes, (int)n.n_refused, (int)n.n_new, (int)n.n_filled);
}

// The reference fusion (nid/nid_reffuse.h): k_reffill_splat as it is, then
//
// k_reffuse_apply: image order, no halo -- a pixel's new state hangs on its own entries alone.  A lane makes kRuPerLane
// CONSECUTIVE pixels: the z-buffer's and the SUM plane's entries as one 16-byte access each, the u16 planes' as 8 bytes, the
// OBS plane's as 4 (the planes come from hipMalloc and a lane's first index is a multiple of 4: aligned); a wave's accesses
// are adjacent.  The lane whose four pixels cross the plane's end makes the ones inside it one by one.  Each pixel runs
// rfu::fuse (nid_reffuse_rule.h: the host's text): S and k written back, the FUSED plane, the BASE plane fused-or-uploaded
// and the new pristine depth fill-or-base for the masking chain behind this kernel.  n_hit and the rule's five counts are
// summed like the fill's and added to words 2 .. 7 of the call's totals with ONE 64-bit INTEGER atomic each; every lane
// reaches the shuffles.  No float is summed.
constexpr int kRuPerLane = 4, kRuSpan = 256 * kRuPerLane;
static_assert(sizeof(nid_reffuse_counts) == 64 && offsetof(nid_reffuse_counts, n_hit) == 16 && offsetof(nid_reffuse_counts, n_changed) == 56,
              "nid_reffuse.h's record: the splat's two counts, then this kernel's six");

__global__ void __launch_bounds__(256) k_reffuse_apply(long N, int gate_abs, int gate_rel_1024, int max_obs, const uint32_t *__restrict__ zbuf,
                                                       const uint16_t *__restrict__ uploaded, double factor0, const uint16_t *__restrict__ fill,
                                                       uint32_t *__restrict__ sum, uint8_t *__restrict__ obs, uint16_t *__restrict__ fused,
                                                       uint16_t *__restrict__ base, uint16_t *__restrict__ pristine,
                                                       unsigned long long *__restrict__ totals /*[8]: words 2 .. 7*/) {
  __shared__ unsigned long long part[4][8];
  const int tid = threadIdx.x;
  const long i0 = ((long)blockIdx.x * 256 + tid) * kRuPerLane;
  nid_reffuse_counts n = {};
  if (i0 + kRuPerLane <= N) {
    const uint4 z4 = *reinterpret_cast<const uint4 *>(zbuf + i0);
    const ushort4 u4 = *reinterpret_cast<const ushort4 *>(uploaded + i0);
    const ushort4 f4 = *reinterpret_cast<const ushort4 *>(fill + i0);
    uint4 s4 = *reinterpret_cast<const uint4 *>(sum + i0);
    uchar4 k4 = *reinterpret_cast<const uchar4 *>(obs + i0);
    ushort4 e4, b4, p4;
#define NID_RU_PIXEL(m)                                                                                                              \
  e4.m = rfu::fuse(dc::depth_valid(u4.m, factor0), u4.m, z4.m, gate_abs, gate_rel_1024, max_obs, &s4.m, &k4.m, &b4.m, &n); \
  p4.m = f4.m ? f4.m : b4.m;
    NID_RU_PIXEL(x) NID_RU_PIXEL(y) NID_RU_PIXEL(z) NID_RU_PIXEL(w)
#undef NID_RU_PIXEL
    *reinterpret_cast<uint4 *>(sum + i0) = s4;
    *reinterpret_cast<uchar4 *>(obs + i0) = k4;
    *reinterpret_cast<ushort4 *>(fused + i0) = e4;
    *reinterpret_cast<ushort4 *>(base + i0) = b4;
    *reinterpret_cast<ushort4 *>(pristine + i0) = p4;
  } else {
    for (long i = i0; i < N; i++) {  // (at most kRuPerLane - 1 pixels of one lane of the grid)
      uint32_t s = sum[i];
      uint8_t k = obs[i];
      uint16_t b = 0;
      const uint16_t u = uploaded[i], f = fill[i];
      fused[i] = rfu::fuse(dc::depth_valid(u, factor0), u, zbuf[i], gate_abs, gate_rel_1024, max_obs, &s, &k, &b, &n);
      sum[i] = s;
      obs[i] = k;
      base[i] = b;
      pristine[i] = f ? f : b;
    }
  }
  counts_to_totals<2>(part, tid, totals, (int)n.n_hit, (int)n.n_valid, (int)n.n_fused, (int)n.n_gated, (int)n.n_saturated, (int)n.n_changed);
}

// The bilinear gather (nid/nid_refgather.h): ONE kernel in the place of k_reffill_splat, the z-buffer's fill and
// k_reffuse_apply.
//
// k_refgather_apply: image order, k_reffuse_apply's shape -- a lane makes kRuPerLane CONSECUTIVE pixels, the SUM plane's
// entries as one 16-byte access, the u16 planes' as 8 bytes, the OBS plane's as 4; the lane whose four pixels cross the
// plane's end makes the ones inside it one by one.  Each pixel runs rg::gather (nid_refgather_rule.h: the host's text):
// the f64 chain G.1 - G.6 -- seven divisions, none of them in a loop -- and four 2-byte reads of the target's depth where
// the pixel projects.  Neighbouring keyframe pixels project onto neighbouring target pixels, so a wave's taps fall into a
// few rows' worth of lines and the plane (tens of kilobytes) stays in L2; the kernel's time is the f64 VALU chain's, not
// the reads'.  The eight counts are summed like the fusion's and added to the call's eight totals with ONE 64-bit INTEGER
// atomic each; every lane reaches the shuffles.  No float is summed, no atomic touches a plane.
struct RefGatherArgs {
  double K[12];        // rows of [R|t], keyframe camera -> target camera (rf::keyframe_to_target)
  double M[12];        // rows of [R|t], target camera -> keyframe camera (rf::target_to_keyframe)
  const uint16_t *d1;  // the target's depth, rows x cols
  double factor1, factor0;
  int tap_abs, tap_rel_1024;
};
static_assert(sizeof(nid_refgather_counts) == 64 && offsetof(nid_refgather_counts, n_changed) == 56, "nid_refgather.h's record: this kernel's eight counts");

__global__ void __launch_bounds__(256) k_refgather_apply(Geometry g, RefGatherArgs A, long N, int gate_abs, int gate_rel_1024, int max_obs,
                                                         const uint16_t *__restrict__ uploaded, const uint16_t *__restrict__ fill,
                                                         uint32_t *__restrict__ sum, uint8_t *__restrict__ obs, uint16_t *__restrict__ fused,
                                                         uint16_t *__restrict__ base, uint16_t *__restrict__ pristine,
                                                         unsigned long long *__restrict__ totals /*[8], zero before the launch*/) {
  __shared__ unsigned long long part[4][8];
  const int tid = threadIdx.x;
  const long i0 = ((long)blockIdx.x * 256 + tid) * kRuPerLane;
  nid_refgather_counts n = {};
  const rg::Gather G = rg::make_gather(g, A.K, A.M, A.d1, A.factor1, A.factor0, A.tap_abs, A.tap_rel_1024);
  int r = (int)(i0 / g.cols), c = (int)(i0 % g.cols);  // (the lane's first pixel; the next ones step along the row)
  if (i0 + kRuPerLane <= N) {
    const ushort4 u4 = *reinterpret_cast<const ushort4 *>(uploaded + i0);
    const ushort4 f4 = *reinterpret_cast<const ushort4 *>(fill + i0);
    uint4 s4 = *reinterpret_cast<const uint4 *>(sum + i0);
    uchar4 k4 = *reinterpret_cast<const uchar4 *>(obs + i0);
    ushort4 e4, b4, p4;
#define NID_RG_PIXEL(m)                                                                                 \
  e4.m = rg::gather(G, r, c, u4.m, gate_abs, gate_rel_1024, max_obs, &s4.m, &k4.m, &b4.m, &n); \
  p4.m = f4.m ? f4.m : b4.m;                                                                            \
  if (++c == g.cols) { c = 0; r++; }
    NID_RG_PIXEL(x) NID_RG_PIXEL(y) NID_RG_PIXEL(z) NID_RG_PIXEL(w)
#undef NID_RG_PIXEL
    *reinterpret_cast<uint4 *>(sum + i0) = s4;
    *reinterpret_cast<uchar4 *>(obs + i0) = k4;
    *reinterpret_cast<ushort4 *>(fused + i0) = e4;
    *reinterpret_cast<ushort4 *>(base + i0) = b4;
    *reinterpret_cast<ushort4 *>(pristine + i0) = p4;
  } else {
    for (long i = i0; i < N; i++) {  // (at most kRuPerLane - 1 pixels of one lane of the grid)
      uint32_t s = sum[i];
      uint8_t k = obs[i];
      uint16_t b = 0;
      const uint16_t f = fill[i];
      fused[i] = rg::gather(G, r, c, uploaded[i], gate_abs, gate_rel_1024, max_obs, &s, &k, &b, &n);
      sum[i] = s;
      obs[i] = k;
      base[i] = b;
      pristine[i] = f ? f : b;
      if (++c == g.cols) { c = 0; r++; }
    }
  }
  counts_to_totals<0>(part, tid, totals, (int)n.n_valid, (int)n.n_sampled, (int)n.n_outside, (int)n.n_tap_refused, (int)n.n_fused, (int)n.n_gated,
                      (int)n.n_saturated, (int)n.n_changed);
}

// depth pixels that belong to no cell (rows/cols not divisible by cell_num, Q11)
// still need Calculate3Dpoint's output when the caller asks for points3d.
__global__ void k_backproject_plain(Geometry g, const double *__restrict__ depth,
                                    const double *__restrict__ Twc, double *__restrict__ pts) {
  const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long)g.rows * g.cols) return;
  const int r = (int)(id / g.cols), col = (int)(id % g.cols);
  const double z = depth[id];
  double X = NAN, Y = NAN, Z = NAN;
  if (!(z < 0.01 || z > 100)) {
    const double x0 = z * (col - g.cx) / g.fx;
    const double y0 = z * (r - g.cy) / g.fy;
    X = Twc[0] * x0 + Twc[4] * y0 + Twc[8] * z + Twc[12];
    Y = Twc[1] * x0 + Twc[5] * y0 + Twc[9] * z + Twc[13];
    Z = Twc[2] * x0 + Twc[6] * y0 + Twc[10] * z + Twc[14];
  }
  pts[3 * id] = X; pts[3 * id + 1] = Y; pts[3 * id + 2] = Z;
}

// The reference stage's per-pixel outputs in the caller's layout (CudaComputeHref's bs_value / bs_index, image order):
// one thread per tile slot writes its pixel's four weights (the sign of the first is the evaluation kernel's knot flag:
// stripped) and its bin index.  Pixels of no cell of this context are not written.
__global__ void k_untile_bs(Geometry g, Tiles t, double *__restrict__ bsv /*4N or null*/, int *__restrict__ bsi /*N or null*/, int nan_rows) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)g.nloc * g.pstride) return;
  const int cl = (int)(gid / g.pstride), s = (int)(gid % g.pstride);
  if (s >= g.ps) return;
  const int c = g.cell_begin + cl * g.cell_stride;
  const long id = (long)((c / g.cell_num) * g.rb + s / g.cb) * g.cols + (c % g.cell_num) * g.cb + s % g.cb;
  if (bsv) {
    const double4 w = *reinterpret_cast<const double4 *>(t.W + 4 * gid);
    // nan_rows (nid_set_href_nan_markers): the legacy operators' convention -- a pixel that is invalid or out of frame at
    // this pose reads NaN, NaN, NaN, NaN (CudaComputeHref.cu:82-87, 126-130); in-frame weights sum to 1, so an all-zero
    // row is exactly that set
    const bool none = nan_rows && w.x == 0.0 && w.y == 0.0 && w.z == 0.0 && w.w == 0.0;
    *reinterpret_cast<double4 *>(bsv + 4 * id) = none ? make_double4(NAN, NAN, NAN, NAN) : make_double4(fabs(w.x), w.y, w.z, w.w);
  }
  if (bsi) bsi[id] = (int)t.JR[gid];
}

// ---------------------------------------------------------------------------
// Setup: reference stage at the initial pose -- computeHref
// (types_six_dof_expmap.cpp:655-725) / CalculateHrefKernel
// (CudaComputeHref.cu:33-135) for one cell per workgroup.
template <int NT>
__global__ __launch_bounds__(NT) void k_href(Geometry g, Pose pose, Tiles t, int *__restrict__ Nc,
                                             double *__restrict__ Href, double hist_scale,
                                             double hist_inv_scale) {
  __shared__ unsigned long long hist[kMaxBins * kHistCopies];
  __shared__ double red[2 * (NT / 64)];
  const int cl = blockIdx.x, tid = threadIdx.x;
  const int copy = tid & (kHistCopies - 1);
  for (int i = tid; i < g.nb * kHistCopies; i += NT) hist[i] = 0ull;
  __syncthreads();
  const size_t base = (size_t)cl * g.pstride;
  int count = 0;
  for (int s = tid; s < g.pstride; s += NT) {
    const size_t gi = base + s;
    const int jr = t.JR[gi];
    double w[4] = {0.0, 0.0, 0.0, 0.0};
    if (jr >= 0) {
      double qx, qy, qz;
      xform_point(pose, t.X[gi], t.Y[gi], t.Z[gi], qx, qy, qz);
      const double u = g.fx * qx / qz + g.cx;
      const double v = g.fy * qy / qz + g.cy;
      if (u >= 0 && u + 3 <= g.cols && v >= 0 && v + 3 <= g.rows) {
        count++;
        double obs = (double)t.I0[gi];
        if (obs >= 255) obs = 254.999;
        const double bin_pos_ref = obs * (double)g.S / 255.0;
        double d[4];
        bspline4<false>(bin_pos_ref, jr, g.S, w, d);
#pragma unroll
        for (int k = 0; k < 4; k++) atomicAdd(&hist[(jr + k) * kHistCopies + copy], fx_encode(w[k], hist_scale));
      }
    }
    // the evaluation kernel's "tiny non-zero reference weights" flag rides in the sign of the first weight (hist_add)
    {
      const double wmin = fmin(w[0], w[3]);
      if (wmin < kTinyW && wmin != 0.0) w[0] = -w[0];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) t.W[4 * gi + k] = w[k];  // slot-major: see load_tile_w
  }
  double v2[2] = {(double)count, 0.0};
  block_sum<NT, 2>(v2, red, tid);
  const int n_c = (int)v2[0];
  __syncthreads();
  // entropy of the reference histogram
  double term = 0.0;
  if (tid < g.nb) {
    unsigned long long acc = 0;
    for (int c = 0; c < kHistCopies; c++) acc += hist[tid * kHistCopies + ((c + tid) & (kHistCopies - 1))];
    const double p = ((double)(long long)acc * hist_inv_scale) / (double)n_c;
    if (!(p < kSigma)) term = p * log2(p);
  }
  double v1[2] = {term, 0.0};
  block_sum<NT, 2>(v1, red, tid);
  if (tid == 0) {
    Nc[cl] = n_c;
    Href[cl] = (n_c < 300) ? NAN : (0.0 - v1[0]);  // CudaComputeHref.cu:206-209
  }
}

// ---------------------------------------------------------------------------
// Plain-histogram NID of one cell per workgroup: NID::ComputeHref + NID::ComputeH of the reference's
// second program (NID_standard_property.cpp:342-485) -- same warp and bilinear sample, HARD binning
// floor(I * bins / 255), no B-spline, no Jacobian.  Counts are integers (u32 LDS atomics), so the
// histograms are exact; the entropies are summed by one thread in the reference's bin order.
// out[cell*6 + {0..5}] = H_ref, H_current, H_joint, nid, MI, n_in.  Cells with fewer than 300 in-frame
// pixels get NaN for H_current / H_joint / nid / MI (the reference returns early there and then reads an
// uninitialised nid_: not reproduced).
template <int NT>
__global__ __launch_bounds__(NT) void k_plain_nid(Geometry g, Pose pose, Tiles t, const uint8_t *__restrict__ im1,
                                                  int bins, double *__restrict__ out) {
  __shared__ unsigned h_ref[kMaxPlainBins], h_cur[kMaxPlainBins], h_joint[kMaxPlainBins * kMaxPlainBins];
  __shared__ unsigned n_in_s;
  const int cl = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < bins; i += NT) { h_ref[i] = 0u; h_cur[i] = 0u; }
  for (int i = tid; i < bins * bins; i += NT) h_joint[i] = 0u;
  if (tid == 0) n_in_s = 0u;
  __syncthreads();
  const size_t base = (size_t)cl * g.pstride;
  for (int s = tid; s < g.pstride; s += NT) {
    const size_t gi = base + s;
    if (t.JR[gi] < 0) continue;  // invalid depth / padding: Get3dPointAndIntensity skips the pixel (:226-227)
    double qx, qy, qz;
    xform_point(pose, t.X[gi], t.Y[gi], t.Z[gi], qx, qy, qz);
    const double u = g.fx * qx / qz + g.cx;  // :357-358
    const double v = g.fy * qy / qz + g.cy;
    if (!(u >= 0 && u + 3 <= g.cols && v >= 0 && v + 3 <= g.rows)) continue;  // ob++
    double i0 = (double)t.I0[gi];
    if (i0 >= 255) i0 = 254.999;  // :370-373
    const int br = (int)floor(i0 * bins / 255.0);
    double ic = bilinear_u8(im1, g.cols, u, v);
    if (ic >= 255) ic = 254.999;  // :432-435
    if (ic < 0) ic = 0.0;
    const int bc = (int)floor(ic * bins / 255.0);
    atomicAdd(&h_ref[br], 1u);
    atomicAdd(&h_cur[bc], 1u);
    atomicAdd(&h_joint[br * bins + bc], 1u);
    atomicAdd(&n_in_s, 1u);
  }
  __syncthreads();
  if (tid == 0) {
    const unsigned n_in = n_in_s;
    const double n = (double)n_in;
    double Href = 0.0, Hc = 0.0, Hj = 0.0;
    for (int i = 0; i < bins; i++) {
      const double p = (double)h_ref[i] / n;
      if (p < kSigma) continue;
      Href -= p * log2(p);
    }
    double nid = NAN, mi = NAN;
    if (n_in >= 300u) {
      for (int i = 0; i < bins; i++) {
        const double p = (double)h_cur[i] / n;
        if (p < kSigma) continue;
        Hc -= p * log2(p);
      }
      for (int i = 0; i < bins * bins; i++) {
        const double p = (double)h_joint[i] / n;
        if (p < kSigma) continue;
        Hj -= p * log2(p);
      }
      nid = (2 * Hj - Href - Hc) / Hj;  // :469-470
      mi = Href + Hc - Hj;
      if (Href == 0.0 && Hc == 0.0 && Hj == 0.0) { mi = 0.0; nid = 0.0; }  // :474-477
    } else {
      Hc = NAN; Hj = NAN;
    }
    double *o = out + (size_t)cl * 6;
    o[0] = Href; o[1] = Hc; o[2] = Hj; o[3] = nid; o[4] = mi; o[5] = n;
  }
}

}  // namespace nid

// What the streaming-kernel files share (batchnorm.hip, reduce.hip, planes_split.hip, criterion.hip, optim.hip,
// pose_feed.hip): their workgroup size, the float4 access of a lane, and the two fixed-order workgroup sums.
// (Not in pl_internal.h: small_layer.hip, gemm_thin.hip and others have an NTHR, ld4 and st4 of their own.)
#pragma once
#include "pl_internal.h"

namespace pl {

constexpr int NTHR = 256;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// -------------------------------------------------------------------------------------
// Small fixed-order column reductions.  Shape of all three: block = 256 threads = 16 columns
// x 16 row-parts, grid = ceil(H/16): every thread sums a strided 1/16 of the partial rows
// (loads coalesce to 64 B per part), then the 16 parts are combined through LDS in a fixed
// order.  (A first version used 64 columns x 4 parts on 16 workgroups: 128 dependent-free
// loads per thread on 16 CUs took 13-31 us per call, 10 % of a step.)
// -------------------------------------------------------------------------------------
constexpr int RCOLS = 16, RPARTS = 16;

__device__ __forceinline__ float parts_sum(float v, float (*red)[RCOLS], int cl, int part) {
  red[part][cl] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < RPARTS; ++q) t += red[q][cl];
  __syncthreads();
  return t;
}

// the sum of v over the workgroup (any whole number of waves), in wave order; sm: one float per wave
__device__ __forceinline__ float block_sum(float v, float* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  float t = 0.f;
  const int nw = blockDim.x >> 6;
  for (int w = 0; w < nw; ++w) t += sm[w];
  __syncthreads();
  return t;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace pl

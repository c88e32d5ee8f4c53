// Global L2 norm of the active part of a flat gradient arena and the clip record the flat AdamW step reads
// (pl_grad_norm_clip): nn.utils.clip_grad_norm(model.parameters(), max_norm=1) of phase1_lifting/main.py:465-470 without
// rewriting the gradient and without a host decision.  One streaming pass over a buffer AdamW reads anyway.
//   stage 1  norm_partial_kernel: up to kChunk ranges per launch, each swept in float4 steps by the whole grid (lo is a
//            multiple of 4; the up-to-3 floats of a ragged tail go to one thread); g^2 summed in fp64 -- the product of two
//            fp32 values is exact there, so only the summation rounds -- per thread, then per workgroup, one double each
//   stage 2  norm_final_kernel: one workgroup sums the partials in a fixed order and writes the record
// No atomics: a repeated call gives the same bits.
#include <math.h>

#include "pl_internal.h"

namespace pl {
namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 64;          // ranges per stage-1 launch (kernel arguments: 1 KiB of ranges)
constexpr int kMaxBlocks = 1024;    // 4 workgroups per CU; 16 KiB of float4 loads per workgroup pass

struct NormRanges {
  int n;
  int64_t lo[kChunk], hi[kChunk];
};

// sum over the workgroup, valid in thread 0; the same tree on every call
__device__ __forceinline__ double block_sum_f64(double x, double* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) sm[w] = x;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < kThreads / 64; ++q) t += sm[q];
  }
  return t;
}

__device__ __forceinline__ void sq4(double (&a)[4], const float4 v) {
  a[0] += (double)v.x * (double)v.x;
  a[1] += (double)v.y * (double)v.y;
  a[2] += (double)v.z * (double)v.z;
  a[3] += (double)v.w * (double)v.w;
}

__global__ __launch_bounds__(kThreads) void norm_partial_kernel(const float* __restrict__ g, NormRanges R,
                                                                double* __restrict__ part) {
  __shared__ double sm[kThreads / 64];
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  const int64_t t0 = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
  for (int r = 0; r < R.n; ++r) {
    const float* __restrict__ base = g + R.lo[r];                   // 16-byte aligned: g is, lo % 4 == 0
    const int64_t len = R.hi[r] - R.lo[r], n4 = len >> 2;
    int64_t i = t0;
    for (; i + 3 * stride < n4; i += 4 * stride) {                  // four loads in flight per thread
      const float4 v0 = *reinterpret_cast<const float4*>(base + 4 * i);
      const float4 v1 = *reinterpret_cast<const float4*>(base + 4 * (i + stride));
      const float4 v2 = *reinterpret_cast<const float4*>(base + 4 * (i + 2 * stride));
      const float4 v3 = *reinterpret_cast<const float4*>(base + 4 * (i + 3 * stride));
      sq4(a, v0); sq4(a, v1); sq4(a, v2); sq4(a, v3);
    }
    for (; i < n4; i += stride) sq4(a, *reinterpret_cast<const float4*>(base + 4 * i));
    if (t0 == 0) {
      for (int64_t e = n4 << 2; e < len; ++e) a[0] += (double)base[e] * (double)base[e];
    }
  }
  const double t = block_sum_f64((a[0] + a[1]) + (a[2] + a[3]), sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(kThreads) void norm_final_kernel(const double* __restrict__ part, int np, float gscale,
                                                              int clip, float max_norm, const float* __restrict__ max_norm_dev,
                                                              int skip_nonfinite, PLClipRecord* __restrict__ rec) {
  __shared__ double sm[kThreads / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < np; i += kThreads) acc += part[i];
  const double s = block_sum_f64(acc, sm);
  if (threadIdx.x == 0) {
    const float norm = (float)(fabs((double)gscale) * sqrt(s));
    float coef = 1.0f;
    if (clip) {                                                     // torch: clamp(max_norm / (total_norm + 1e-6), max=1)
      const float c = (max_norm_dev ? max_norm_dev[0] : max_norm) / (norm + 1e-6f);
      coef = c > 1.0f ? 1.0f : c;                                   // (a NaN stays a NaN, as torch.clamp leaves it)
    }
    const bool fin = isfinite(norm);
    const bool skip = skip_nonfinite && !fin;
    rec->norm = norm;
    rec->coef = coef;
    rec->finite = fin ? 1u : 0u;
    rec->skip = skip ? 1u : 0u;
    if (skip) rec->skipped += 1;
  }
}

inline int chunks_of(int nranges) { return (nranges + kChunk - 1) / kChunk; }

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" size_t pl_grad_norm_scratch_bytes(int nranges) {
  if (nranges < 1 || nranges > PL_GRAD_NORM_MAX_RANGES) return 0;
  return (size_t)chunks_of(nranges) * kMaxBlocks * sizeof(double);
}

extern "C" int pl_grad_norm_clip(const float* g, int64_t n, const PLGradRange* ranges, int nranges, float grad_scale,
                                 int clip, float max_norm, const float* max_norm_dev, int skip_nonfinite,
                                 PLClipRecord* record, void* scratch, void* stream) {
  if (!g || !ranges || !record || !scratch) PL_FAIL(PL_EINVAL, "pl_grad_norm_clip: null pointer");
  if ((reinterpret_cast<uintptr_t>(g) & 15) || (reinterpret_cast<uintptr_t>(record) & 7) ||
      (reinterpret_cast<uintptr_t>(scratch) & 7))
    PL_FAIL(PL_EINVAL, "pl_grad_norm_clip: misaligned arena (16), record or scratch (8)");
  if (n <= 0 || nranges < 1 || nranges > PL_GRAD_NORM_MAX_RANGES)
    PL_FAIL(PL_ESHAPE, "pl_grad_norm_clip: n=%lld nranges=%d (1..%d)", (long long)n, nranges, PL_GRAD_NORM_MAX_RANGES);
  if (clip && !max_norm_dev && !(max_norm >= 0.f))                  // (negative or NaN)
    PL_FAIL(PL_EINVAL, "pl_grad_norm_clip: max_norm = %g", (double)max_norm);
  int64_t prev = 0;
  for (int r = 0; r < nranges; ++r) {
    const int64_t lo = ranges[r].lo, hi = ranges[r].hi;
    if (lo < prev || hi <= lo || hi > n)
      PL_FAIL(PL_ESHAPE, "pl_grad_norm_clip: range %d = [%lld, %lld) of %lld floats (ascending, disjoint, inside)", r,
              (long long)lo, (long long)hi, (long long)n);
    if (lo & 3) PL_FAIL(PL_EINVAL, "pl_grad_norm_clip: misaligned range %d: lo = %lld is no multiple of 4", r, (long long)lo);
    prev = hi;
  }
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(scratch);
  int np = 0;
  for (int c = 0; c < chunks_of(nranges); ++c) {
    NormRanges R = {};
    int64_t work = 0;                                               // float4 steps of this chunk
    for (int r = c * kChunk; r < nranges && r < (c + 1) * kChunk; ++r) {
      R.lo[R.n] = ranges[r].lo; R.hi[R.n] = ranges[r].hi; ++R.n;
      work += (ranges[r].hi - ranges[r].lo + 3) >> 2;
    }
    int64_t blocks = (work + kThreads - 1) / kThreads;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(norm_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, g, R, part + np);
    PL_CHECK_LAUNCH("grad_norm_partial");
    np += (int)blocks;
  }
  hipLaunchKernelGGL(norm_final_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)part, np, grad_scale, clip, max_norm,
                     max_norm_dev, skip_nonfinite, record);
  PL_CHECK_LAUNCH("grad_norm_final");
  return PL_OK;
}

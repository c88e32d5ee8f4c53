// The fixed-order sums of the lifter path: split-K slabs (with and without the bias), partial rows of the bias and
// weight gradients -- several problems per launch -- partial column sums, and the fill.
//
// They replace nothing on the reference path by themselves: they are the second stage of the sums its addmm / mm backward
// and the split-K GEMMs here leave (phase1_lifting/baselineModel.py:35-37,92-94).
//
// Common shape: a (B x H) fp32 activation is walked with one float4 per lane, a
// wavefront covering 256 consecutive columns of one row (1 KiB per wave-instruction,
// fully coalesced).  Every column reduction is a fixed-order two-stage sum (per-block
// partials, then a small finalize kernel): results are bitwise reproducible, no float
// atomics anywhere.
#include "pl_internal.h"
#include "streaming.h"

namespace pl {
namespace {

// out[c] = sum_r part[r][c]: the column-parallel form of reduce_slabs for many short slabs
__global__ __launch_bounds__(NTHR) void reduce_rows_kernel(const float* __restrict__ part, int R, int H,
                                                           float* __restrict__ out) {
  __shared__ float red[RPARTS][RCOLS];
  const int cl = threadIdx.x & (RCOLS - 1), p = threadIdx.x / RCOLS;
  const int c = blockIdx.x * RCOLS + cl;
  float a = 0.f;
  if (c < H)
#pragma unroll 8
    for (int k = p; k < R; k += RPARTS) a += part[(size_t)k * H + c];
  const float t = parts_sum(a, red, cl, p);
  if (p == 0 && c < H) out[c] = t;
}

__global__ void reduce_slabs_kernel(const float* __restrict__ slabs, int nslab, int64_t n,
                                    float* __restrict__ out, int vec) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (; i < n4; i += stride) {
      float4 a = ld4(slabs + 4 * i);
      int s = 1;
      for (; s + 4 <= nslab; s += 4) {                   // four slabs' loads in flight, added in slab order
        float4 b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) b[u] = ld4(slabs + (size_t)(s + u) * n + 4 * i);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) { a.x += b[u].x; a.y += b[u].y; a.z += b[u].z; a.w += b[u].w; }
      }
      for (; s < nslab; ++s) {
        const float4 b = ld4(slabs + (size_t)s * n + 4 * i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      st4(out + 4 * i, a);
    }
  } else {
    for (; i < n; i += stride) {
      float a = slabs[i];
      for (int s = 1; s < nslab; ++s) a += slabs[(size_t)s * n + i];
      out[i] = a;
    }
  }
}

// out[r][c] = bias[c] + sum_s slabs[s][r][c]   (split-K forward of the skinny output layer)
__global__ void reduce_slabs_bias_kernel(const float* __restrict__ slabs, int nslab, int64_t n, int cols,
                                         const float* __restrict__ bias, float* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float a = bias ? bias[i % cols] : 0.f;
    for (int s = 0; s < nslab; ++s) a += slabs[(size_t)s * n + i];
    out[i] = a;
  }
}

// block = 4 row-lanes x 64 column-lanes; fixed-order combine through LDS
__global__ __launch_bounds__(NTHR) void colsum_partial_kernel(const float* __restrict__ X, int rows,
                                                              int cols, int rpc, float* __restrict__ part) {
  __shared__ float sm[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int r0 = blockIdx.x * rpc, r1 = min(rows, r0 + rpc);
  for (int c0 = 0; c0 < cols; c0 += 64) {
    const int c = c0 + cl;
    float s = 0.f;
    if (c < cols)
      for (int r = r0 + rl; r < r1; r += 4) s += X[(size_t)r * cols + c];
    sm[rl][cl] = s;
    __syncthreads();
    if (rl == 0 && c < cols) part[(size_t)blockIdx.x * cols + c] = (sm[0][cl] + sm[1][cl]) + (sm[2][cl] + sm[3][cl]);
    __syncthreads();
  }
}

// several independent reduce_rows problems in one launch: blockIdx.y = job
// Every fixed-order partial-sum combine of one backward range in ONE launch (blockIdx.y = job): the bias gradients
// (many partial rows, few columns: 16 columns x 16 row-parts per workgroup, as reduce_rows_kernel), the skinny
// layers' weight-gradient partials (transK: the transposed store of dW0), and the split-K slabs of the 1024-wide weight
// gradients (few slabs, 1M outputs: streamed as float4, slab by slab in order -- kind 1).
constexpr int kMaxRowJobs = 16;
struct RowJobs { const float* part[kMaxRowJobs]; float* out[kMaxRowJobs]; int R[kMaxRowJobs]; int H[kMaxRowJobs];
                 int kind[kMaxRowJobs]; int transK[kMaxRowJobs]; float inv_n; uint64_t* tick; };
__global__ __launch_bounds__(NTHR) void reduce_rows_multi_kernel(RowJobs j) {
  __shared__ float red[RPARTS][RCOLS];
  const int job = blockIdx.y;
  const int R = j.R[job], H = j.H[job];
  const float* __restrict__ part = j.part[job];
  if (j.kind[job] == 2) {                    // the MSE loss of the fused train step: mse_final_kernel's sum, bit for bit
    if (blockIdx.x) return;
    float acc = 0.f;
    for (int i = threadIdx.x; i < R; i += blockDim.x) acc += part[i];
    const float t = block_sum(acc, &red[0][0]);
    if (threadIdx.x == 0) {
      j.out[job][0] = t * j.inv_n;
      if (j.tick) j.tick[0] += 1;
    }
    return;
  }
  if (j.kind[job] == 1) {                    // H % 4 == 0, 16-byte aligned (checked on the host)
    const int n4 = H >> 2;
    if (R == 4) {
      // the four split-K slabs of a 1024-wide weight gradient: all four loads in flight, added in slab order (with the
      // slab count a run-time loop bound every load waited for the one before it)
      for (int i = blockIdx.x * NTHR + threadIdx.x; i < n4; i += gridDim.x * NTHR) {
        const float* __restrict__ q = part + 4 * (size_t)i;
        float4 a = ld4(q);
        const float4 b1 = ld4(q + (size_t)H), b2 = ld4(q + 2 * (size_t)H), b3 = ld4(q + 3 * (size_t)H);
        a.x += b1.x; a.y += b1.y; a.z += b1.z; a.w += b1.w;
        a.x += b2.x; a.y += b2.y; a.z += b2.z; a.w += b2.w;
        a.x += b3.x; a.y += b3.y; a.z += b3.z; a.w += b3.w;
        st4(j.out[job] + 4 * (size_t)i, a);
      }
      return;
    }
    for (int i = blockIdx.x * NTHR + threadIdx.x; i < n4; i += gridDim.x * NTHR) {
      float4 a = ld4(part + 4 * (size_t)i);
      for (int sl = 1; sl < R; ++sl) {
        const float4 b = ld4(part + (size_t)sl * H + 4 * (size_t)i);
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      st4(j.out[job] + 4 * (size_t)i, a);
    }
    return;
  }
  if (blockIdx.x * RCOLS >= H) return;
  const int cl = threadIdx.x & (RCOLS - 1), p = threadIdx.x / RCOLS;
  const int c = blockIdx.x * RCOLS + cl;
  float a = 0.f;
  if (c < H)
#pragma unroll 8
    for (int k = p; k < R; k += RPARTS) a += part[(size_t)k * H + c];
  const float t = parts_sum(a, red, cl, p);
  if (p == 0 && c < H) {
    const int K = j.transK[job];
    if (K > 0) {                             // c = k * (H / K) + col  ->  out[col][k]
      const int Hc = H / K, k = c / Hc, col = c - k * Hc;
      j.out[job][(size_t)col * K + k] = t;
    } else {
      j.out[job][c] = t;
    }
  }
}

__global__ void fill_kernel(float* p, int64_t n, float v) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

}  // namespace

// =====================================================================================
// launchers
// =====================================================================================
int launch_reduce_slabs(const float* slabs, int nslab, int64_t n, float* out, hipStream_t s) {
  if (nslab >= 8 && n <= 65536) {   // many short slabs: parallelise over the slab index too
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(((int)n + RCOLS - 1) / RCOLS), dim3(NTHR), 0, s, slabs, nslab,
                       (int)n, out);
    PL_CHECK_LAUNCH("reduce_rows");
    return PL_OK;
  }
  const int vec = ((n & 3) == 0) && aligned16(slabs) && aligned16(out);
  const int64_t work = vec ? (n >> 2) : n;
  int blocks = (int)((work + NTHR - 1) / NTHR);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3(blocks), dim3(NTHR), 0, s, slabs, nslab, n, out, vec);
  PL_CHECK_LAUNCH("reduce_slabs");
  return PL_OK;
}

int launch_reduce_slabs_bias(const float* slabs, int nslab, int rows, int cols, const float* bias,
                             float* out, hipStream_t s) {
  const int64_t n = (int64_t)rows * cols;
  int blocks = (int)((n + NTHR - 1) / NTHR);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(reduce_slabs_bias_kernel, dim3(blocks), dim3(NTHR), 0, s, slabs, nslab, n, cols, bias, out);
  PL_CHECK_LAUNCH("reduce_slabs_bias");
  return PL_OK;
}

int launch_reduce_rows_multi(const RowJob* jobs, int njobs, float loss_inv_n, uint64_t* loss_tick, hipStream_t s) {
  for (int base = 0; base < njobs; base += kMaxRowJobs) {
    RowJobs j = {};
    j.inv_n = loss_inv_n; j.tick = loss_tick;
    const int n = njobs - base < kMaxRowJobs ? njobs - base : kMaxRowJobs;
    int gx = 1;
    for (int k = 0; k < n; ++k) {
      const RowJob& q = jobs[base + k];
      j.part[k] = q.part; j.out[k] = q.out; j.R[k] = q.R; j.H[k] = q.H; j.kind[k] = q.kind; j.transK[k] = q.transK;
      int need;
      if (q.kind == 1) {
        if ((q.H & 3) || !aligned16(q.part) || !aligned16(q.out)) PL_FAIL(PL_EINVAL, "reduce_rows_multi: slab job alignment");
        need = ((q.H >> 2) + NTHR - 1) / NTHR;
        if (need > 1024) need = 1024;
      } else if (q.kind == 2) {
        need = 1;
      } else {
        need = (q.H + RCOLS - 1) / RCOLS;
      }
      if (need > gx) gx = need;
    }
    hipLaunchKernelGGL(reduce_rows_multi_kernel, dim3(gx, n), dim3(NTHR), 0, s, j);
    PL_CHECK_LAUNCH("reduce_rows_multi");
  }
  return PL_OK;
}

int colsum_chunks(int rows) {
  int rc = (rows + 63) / 64;
  if (rc > 64) rc = 64;
  return rc < 1 ? 1 : rc;
}

int launch_colsum_partial(const float* X, int rows, int cols, float* part, hipStream_t s) {
  const int rc = colsum_chunks(rows);
  const int rpc = (rows + rc - 1) / rc;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3(rc), dim3(NTHR), 0, s, X, rows, cols, rpc, part);
  PL_CHECK_LAUNCH("colsum_partial");
  return PL_OK;
}

int launch_fill(float* p, int64_t n, float v, hipStream_t s) {
  if (n <= 0) return PL_OK;
  int blocks = (int)((n + NTHR - 1) / NTHR);
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(NTHR), 0, s, p, n, v);
  PL_CHECK_LAUNCH("fill");
  return PL_OK;
}

}  // namespace pl

// MyViT, the transformer lifter (reference phase1_lifting/baselineModel.py:220-362): every non-GEMM part of its
// forward and backward.  The Linears run on the library's GEMMs (pl_gemm_f32 / pl_gemm_planes_raw); this file holds
//   vit_embed_fwd / _bwd     x = x2d W^T + b + pos (K = in_d is 2 or 3: not a GEMM shape); dW, db, dpos, dx2d
//   vit_ln_fwd / _bwd        one or two chained LayerNorms per row (norm1 -> mhsa.norm), the residual add in front
//   vit_attn_fwd / _bwd      short-sequence multi-head attention, one workgroup per sample, all heads
//   vit_gelu_fwd / _bwd      exact (erf) GELU and its derivative
//   vit_head_fwd / _bwd      ReLU + the last Linear of the token head (H/2 -> out_d, out_d <= 4)
//   vit_amax / vit_split     fp16 operand planes of an activation or gradient with a power-of-two scale chosen
//                            on the device from its max |x| (PL_F16X3 mode)
//   vit_bf16_pack            fp32 -> bf16 carrier (the one "bf16p" operand no producer here writes: the head's dx)
// "bf16p" mode: the producers of the block GEMMs' operands (LayerNorm forward / backward, attention forward / backward,
// GELU forward / backward) also take a bf16 CARRIER of their output, [rows_pad][cols] row-major with the rows past T
// zero (the padded contraction of the TN weight gradients).  Each carrier element is the kernel's own fp32 result
// rounded once at the store (__bf16 cast: v_cvt_pk_bf16_f32, round to nearest even, NaN stays NaN).  The kernels take
// it as a template flag: the <false> instantiations are the fp32 kernels, launched as before.
// Every parameter gradient is reduced in a fixed order: per-chunk partial sums, then one ordered pass over the
// chunks (vit_reduce_chunks).  No float atomics anywhere: a repeated step is bitwise equal.
#include <math.h>

#include <algorithm>

#include "pl_internal.h"

namespace pl {
namespace {

constexpr int NT = 256;          // threads of every kernel here
constexpr int kChunkRows = 256;  // rows per partial-sum chunk of the parameter-gradient reductions
constexpr int kMaxSeq = 32;
constexpr int kDimHead = 64;
constexpr int kLnMaxV = 4;       // float4s per lane of a LayerNorm row: H <= 1024
constexpr int kHeadMaxOut = 4;
constexpr int kHeadMaxK = 256;
constexpr int kAmaxBlocks = 512;
constexpr size_t kLdsMax = 160 * 1024;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
  return v;
}

inline int blocks_for(int64_t n, int per) { return (int)((n + per - 1) / per); }
inline int64_t chunks_of(int64_t T) { return (T + kChunkRows - 1) / kChunkRows; }

typedef __bf16 vb4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned short bf16_bits(float v) {
  const __bf16 q = (__bf16)v;
  return __builtin_bit_cast(unsigned short, q);
}

// 4 consecutive carrier elements (8-byte aligned)
__device__ __forceinline__ void st_bf16x4(unsigned short* p, float4 v) {
  vb4 q;
  q[0] = (__bf16)v.x; q[1] = (__bf16)v.y; q[2] = (__bf16)v.z; q[3] = (__bf16)v.w;
  *reinterpret_cast<vb4*>(p) = q;
}

// rows T .. rows_pad-1 of a [rows_pad][cols] carrier (cols % 4 == 0) to zero, by every thread of the calling workgroup
__device__ __forceinline__ void zero_pad_rows(unsigned short* c, int64_t T, int64_t rows_pad, int64_t cols) {
  const int64_t e1 = rows_pad * cols / 4;
  for (int64_t e = T * cols / 4 + threadIdx.x; e < e1; e += NT) reinterpret_cast<uint2*>(c)[e] = make_uint2(0u, 0u);
}

// out[c] = sum over k = 0 .. nchunks-1 of part[k][c], in that order per quarter (k = q mod 4), quarters summed 0..3
__global__ void __launch_bounds__(NT) vit_reduce_chunks(const float* __restrict__ part, int nchunks, int ncols,
                                                        float* __restrict__ out) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
  float s = 0.f;
  if (c < ncols)
    for (int k = q; k < nchunks; k += 4) s += part[(size_t)k * ncols + c];
  red[q][threadIdx.x & 63] = s;
  __syncthreads();
  if (q == 0 && c < ncols) out[c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

int launch_reduce(const float* part, int64_t nchunks, int64_t ncols, float* out, hipStream_t s) {
  hipLaunchKernelGGL(vit_reduce_chunks, dim3(blocks_for(ncols, 64)), dim3(NT), 0, s, part, (int)nchunks, (int)ncols, out);
  PL_CHECK_LAUNCH("vit_reduce_chunks");
  return PL_OK;
}

// ---------------------------------------------------------------------------------------------- embedding
__global__ void __launch_bounds__(NT) vit_embed_fwd(const float* __restrict__ x2d, int T, int in_d, int seq,
                                                    const float* __restrict__ W, const float* __restrict__ b,
                                                    const float* __restrict__ pos, int H, float* __restrict__ x) {
  const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (int64_t)T * H) return;
  const int t = (int)(idx / H), j = (int)(idx % H);
  float v = 0.f;
  for (int i = 0; i < in_d; ++i) v = fmaf(x2d[(size_t)t * in_d + i], W[j * in_d + i], v);
  x[idx] = (v + b[j]) + pos[(t % seq) * H + j];
}

// partial[chunk][H*in_d + H]: dW in the parameter's [H][in_d] layout, then db
__global__ void __launch_bounds__(NT) vit_embed_bwd_part(const float* __restrict__ dx, const float* __restrict__ x2d, int T,
                                                         int in_d, int H, float* __restrict__ part) {
  const int r0 = blockIdx.x * kChunkRows, r1 = min(T, r0 + kChunkRows);
  float* p = part + (size_t)blockIdx.x * (H * in_d + H);
  for (int j = threadIdx.x; j < H; j += NT) {
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, db = 0.f;
    for (int t = r0; t < r1; ++t) {
      const float g = dx[(size_t)t * H + j];
      db += g;
      for (int i = 0; i < in_d; ++i) acc[i] = fmaf(g, x2d[(size_t)t * in_d + i], acc[i]);
    }
    for (int i = 0; i < in_d; ++i) p[j * in_d + i] = acc[i];
    p[H * in_d + j] = db;
  }
}

// dpos[n][j] = sum over samples of dx[b*seq + n][j], samples in order
__global__ void __launch_bounds__(NT) vit_embed_dpos(const float* __restrict__ dx, int B, int seq, int H,
                                                     float* __restrict__ dpos) {
  const int idx = blockIdx.x * NT + threadIdx.x;
  if (idx >= seq * H) return;
  const int n = idx / H, j = idx % H;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += dx[((size_t)b * seq + n) * H + j];
  dpos[idx] = s;
}

// dx2d[t][i] = sum_j dx[t][j] W[j][i]: one wave per row
__global__ void __launch_bounds__(NT) vit_embed_dinput(const float* __restrict__ dx, const float* __restrict__ W, int T,
                                                       int in_d, int H, float* __restrict__ dx2d) {
  const int t = blockIdx.x * (NT / kWave) + threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (t >= T) return;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = lane; j < H; j += kWave) {
    const float g = dx[(size_t)t * H + j];
    for (int i = 0; i < in_d; ++i) acc[i] = fmaf(g, W[j * in_d + i], acc[i]);
  }
  for (int i = 0; i < in_d; ++i) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) dx2d[(size_t)t * in_d + i] = s;
  }
}

// ---------------------------------------------------------------------------------------------- LayerNorm
// One wave per row; lane l holds float4s l, l + 64, ... of the row in registers.  Statistics are two-pass over the
// registers and taken about the row's first element (shift): d = x - shift is exact for a row with a large mean and a
// small spread, and so is the mean of d -- the mean itself, rounded to fp32, would cost the normalised row its low bits.
// Saved per row: mean of (x - shift), 1/std; the backward re-reads the shift from the row.
struct LnRow {
  float4 v[kLnMaxV];
};

__device__ __forceinline__ float row_shift(const LnRow& r) { return __shfl(r.v[0].x, 0, kWave); }

__device__ __forceinline__ void ln_stats(const LnRow& r, int nv4, int H, float eps, float shift, float& mean, float& rstd) {
  const int lane = threadIdx.x % kWave;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < kLnMaxV; ++k)
    if (lane + k * kWave < nv4) s += ((r.v[k].x - shift) + (r.v[k].y - shift)) + ((r.v[k].z - shift) + (r.v[k].w - shift));
  mean = wave_sum(s) / (float)H;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < kLnMaxV; ++k)
    if (lane + k * kWave < nv4) {
      const float a = (r.v[k].x - shift) - mean, b = (r.v[k].y - shift) - mean, c = (r.v[k].z - shift) - mean,
                  d = (r.v[k].w - shift) - mean;
      q += (a * a + b * b) + (c * c + d * d);
    }
  rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
}

__device__ __forceinline__ float4 ln_xhat4(float4 x, float shift, float mean, float rstd) {
  return make_float4(((x.x - shift) - mean) * rstd, ((x.y - shift) - mean) * rstd, ((x.z - shift) - mean) * rstd,
                     ((x.w - shift) - mean) * rstd);
}

__device__ __forceinline__ float4 ln_apply4(float4 x, float shift, float mean, float rstd, float4 g, float4 b) {
  const float4 h = ln_xhat4(x, shift, mean, rstd);
  return make_float4(fmaf(h.x, g.x, b.x), fmaf(h.y, g.y, b.y), fmaf(h.z, g.z, b.z), fmaf(h.w, g.w, b.w));
}

// x_out = x + add (add optional); y = LN_nnorm(... LN_1(x_out)); stats [nnorm][2][T] = mean, rstd of each LayerNorm
// kBf: y also (or only: y may be NULL) as the bf16 carrier yb [rows_pad][H]; the grid covers rows_pad rows
template <bool kBf>
__global__ void __launch_bounds__(NT) vit_ln_fwd(const float* __restrict__ x, const float* __restrict__ add, int T, int H,
                                                 int nnorm, const float* __restrict__ g1, const float* __restrict__ b1,
                                                 const float* __restrict__ g2, const float* __restrict__ b2, float eps,
                                                 float* __restrict__ x_out, float* __restrict__ y, float* __restrict__ stats,
                                                 unsigned short* __restrict__ yb, int rows_pad) {
  const int t = blockIdx.x * (NT / kWave) + threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int nv4 = H / 4;
  if (kBf && t >= T && t < rows_pad) {
    for (int c = lane; c < nv4; c += kWave) reinterpret_cast<uint2*>(yb + (size_t)t * H)[c] = make_uint2(0u, 0u);
    return;
  }
  if (t >= T) return;
  const float4* xr = reinterpret_cast<const float4*>(x + (size_t)t * H);
  const float4* ar = add ? reinterpret_cast<const float4*>(add + (size_t)t * H) : nullptr;
  LnRow r;
#pragma unroll
  for (int k = 0; k < kLnMaxV; ++k) {
    const int c = lane + k * kWave;
    if (c < nv4) {
      float4 v = xr[c];
      if (ar) {
        const float4 a = ar[c];
        v = make_float4(v.x + a.x, v.y + a.y, v.z + a.z, v.w + a.w);
        reinterpret_cast<float4*>(x_out + (size_t)t * H)[c] = v;
      }
      r.v[k] = v;
    }
  }
  for (int n = 0; n < nnorm; ++n) {
    float mean, rstd;
    const float shift = row_shift(r);
    ln_stats(r, nv4, H, eps, shift, mean, rstd);
    if (lane == 0) {
      stats[(size_t)(2 * n) * T + t] = mean;
      stats[(size_t)(2 * n + 1) * T + t] = rstd;
    }
    const float4* g = reinterpret_cast<const float4*>(n == 0 ? g1 : g2);
    const float4* b = reinterpret_cast<const float4*>(n == 0 ? b1 : b2);
#pragma unroll
    for (int k = 0; k < kLnMaxV; ++k) {
      const int c = lane + k * kWave;
      if (c < nv4) r.v[k] = ln_apply4(r.v[k], shift, mean, rstd, g[c], b[c]);
    }
  }
  if (nnorm > 0) {
#pragma unroll
    for (int k = 0; k < kLnMaxV; ++k) {
      const int c = lane + k * kWave;
      if (c < nv4) {
        if (kBf) {
          st_bf16x4(yb + (size_t)t * H + 4 * c, r.v[k]);
          if (y) reinterpret_cast<float4*>(y + (size_t)t * H)[c] = r.v[k];
        } else {
          reinterpret_cast<float4*>(y + (size_t)t * H)[c] = r.v[k];
        }
      }
    }
  }
}

// LayerNorm backward of one row held as (xhat, dy) in registers: returns dx in dy's place, accumulates dgamma / dbeta
__device__ __forceinline__ void ln_row_bwd(LnRow& xh, LnRow& dy, const float4* g, float rstd, int nv4, int H, LnRow& dg,
                                           LnRow& db) {
  const int lane = threadIdx.x % kWave;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < kLnMaxV; ++k) {
    const int c = lane + k * kWave;
    if (c < nv4) {
      const float4 gg = g[c], d = dy.v[k], h = xh.v[k];
      dg.v[k].x = fmaf(d.x, h.x, dg.v[k].x); dg.v[k].y = fmaf(d.y, h.y, dg.v[k].y);
      dg.v[k].z = fmaf(d.z, h.z, dg.v[k].z); dg.v[k].w = fmaf(d.w, h.w, dg.v[k].w);
      db.v[k].x += d.x; db.v[k].y += d.y; db.v[k].z += d.z; db.v[k].w += d.w;
      const float4 e = make_float4(d.x * gg.x, d.y * gg.y, d.z * gg.z, d.w * gg.w);   // d xhat
      dy.v[k] = e;
      s1 += (e.x + e.y) + (e.z + e.w);
      s2 += (e.x * h.x + e.y * h.y) + (e.z * h.z + e.w * h.w);
    }
  }
  const float m1 = wave_sum(s1) / (float)H, m2 = wave_sum(s2) / (float)H;
#pragma unroll
  for (int k = 0; k < kLnMaxV; ++k) {
    const int c = lane + k * kWave;
    if (c < nv4) {
      const float4 e = dy.v[k], h = xh.v[k];
      dy.v[k] = make_float4(rstd * (e.x - m1 - h.x * m2), rstd * (e.y - m1 - h.y * m2), rstd * (e.z - m1 - h.z * m2),
                            rstd * (e.w - m1 - h.w * m2));
    }
  }
}

// dx = dres + LN_1'( ... LN_nnorm'(dy)); x is the first LayerNorm's input; partial[chunk][nnorm][2][H] = dgamma, dbeta
// kBf: dx also (or only: dx may be NULL) as the bf16 carrier dxb [rows_pad][H]; the last workgroup zeroes its padding
template <bool kBf>
__global__ void __launch_bounds__(NT) vit_ln_bwd(const float* __restrict__ dy, const float* __restrict__ dres,
                                                 const float* __restrict__ x, const float* __restrict__ stats, int T, int H,
                                                 int nnorm, const float* __restrict__ g1, const float* __restrict__ b1,
                                                 const float* __restrict__ g2, float* __restrict__ dx,
                                                 float* __restrict__ part, unsigned short* __restrict__ dxb, int rows_pad) {
  extern __shared__ float4 red4[];              // [NT / kWave][2 * nnorm * H]
  float* red = reinterpret_cast<float*>(red4);
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave, nv4 = H / 4, ncols = 2 * nnorm * H;
  LnRow dg[2], db[2];
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int k = 0; k < kLnMaxV; ++k) dg[n].v[k] = db[n].v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int r0 = blockIdx.x * kChunkRows, r1 = min(T, r0 + kChunkRows);
  for (int t = r0 + w; t < r1; t += NT / kWave) {
    const float4* xr = reinterpret_cast<const float4*>(x + (size_t)t * H);
    const float4* dr = reinterpret_cast<const float4*>(dy + (size_t)t * H);
    LnRow h1, h2, d;
    const float mean1 = stats[t], rstd1 = stats[(size_t)T + t], shift1 = x[(size_t)t * H];
#pragma unroll
    for (int k = 0; k < kLnMaxV; ++k) {
      const int c = lane + k * kWave;
      if (c < nv4) {
        h1.v[k] = ln_xhat4(xr[c], shift1, mean1, rstd1);
        d.v[k] = dr[c];
      }
    }
    if (nnorm == 2) {
      // the second LayerNorm's input y1 = xhat1 g1 + b1 (as the forward computed it), its xhat2
      const float mean2 = stats[(size_t)2 * T + t], rstd2 = stats[(size_t)3 * T + t];
      const float4* gg = reinterpret_cast<const float4*>(g1);
      const float4* bb = reinterpret_cast<const float4*>(b1);
      LnRow y1;
#pragma unroll
      for (int k = 0; k < kLnMaxV; ++k) {
        const int c = lane + k * kWave;
        if (c < nv4) y1.v[k] = ln_apply4(xr[c], shift1, mean1, rstd1, gg[c], bb[c]);
      }
      const float shift2 = row_shift(y1);
#pragma unroll
      for (int k = 0; k < kLnMaxV; ++k) {
        const int c = lane + k * kWave;
        if (c < nv4) h2.v[k] = ln_xhat4(y1.v[k], shift2, mean2, rstd2);
      }
      ln_row_bwd(h2, d, reinterpret_cast<const float4*>(g2), rstd2, nv4, H, dg[1], db[1]);
    }
    ln_row_bwd(h1, d, reinterpret_cast<const float4*>(g1), rstd1, nv4, H, dg[0], db[0]);
    const float4* rr = dres ? reinterpret_cast<const float4*>(dres + (size_t)t * H) : nullptr;
#pragma unroll
    for (int k = 0; k < kLnMaxV; ++k) {
      const int c = lane + k * kWave;
      if (c < nv4) {
        float4 v = d.v[k];
        if (rr) {
          const float4 q = rr[c];
          v = make_float4(v.x + q.x, v.y + q.y, v.z + q.z, v.w + q.w);
        }
        if (kBf) {
          st_bf16x4(dxb + (size_t)t * H + 4 * c, v);
          if (dx) reinterpret_cast<float4*>(dx + (size_t)t * H)[c] = v;
        } else {
          reinterpret_cast<float4*>(dx + (size_t)t * H)[c] = v;
        }
      }
    }
  }
  if (kBf && blockIdx.x == gridDim.x - 1) zero_pad_rows(dxb, T, rows_pad, H);
  // waves -> LDS -> one ordered sum per column
  for (int n = 0; n < nnorm; ++n)
#pragma unroll
    for (int k = 0; k < kLnMaxV; ++k) {
      const int c = lane + k * kWave;
      if (c < nv4) {
        reinterpret_cast<float4*>(red + w * ncols + (2 * n) * H)[c] = dg[n].v[k];
        reinterpret_cast<float4*>(red + w * ncols + (2 * n + 1) * H)[c] = db[n].v[k];
      }
    }
  __syncthreads();
  float* p = part + (size_t)blockIdx.x * ncols;
  for (int c = threadIdx.x; c < ncols; c += NT)
    p[c] = ((red[c] + red[ncols + c]) + red[2 * ncols + c]) + red[3 * ncols + c];
}

// ---------------------------------------------------------------------------------------------- attention
// qkv [B*seq][3*HD] (HD = heads * 64; q | k | v, head h at columns h*64 .. h*64+63 of each); one workgroup per sample.
// LDS: the sample's qkv with rows padded by one float (the score loop's consecutive threads read consecutive key rows).
// kBf: o only as the bf16 carrier ob [rows_pad][HD] (o may be NULL then); the last workgroup zeroes its padding
template <bool kBf>
__global__ void __launch_bounds__(NT) vit_attn_fwd(const float* __restrict__ qkv, int seq, int heads, float scale,
                                                   float* __restrict__ o, float* __restrict__ lse,
                                                   unsigned short* __restrict__ ob, int rows_pad) {
  extern __shared__ float lds[];
  const int HD = heads * kDimHead, ld = 3 * HD + 1;
  float* sq = lds;                          // [seq][ld]
  float* sc = lds + seq * ld;               // [heads][seq][kMaxSeq]
  const int b = blockIdx.x;
  const float* src = qkv + (size_t)b * seq * 3 * HD;
  for (int e = threadIdx.x; e < seq * 3 * HD / 4; e += NT) {
    const float4 v = reinterpret_cast<const float4*>(src)[e];
    const int r = (4 * e) / (3 * HD), c = (4 * e) % (3 * HD);
    float* d = sq + r * ld + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < heads * seq * seq; it += NT) {
    const int h = it / (seq * seq), i = (it / seq) % seq, j = it % seq;
    const float* q = sq + i * ld + h * kDimHead;
    const float* k = sq + j * ld + HD + h * kDimHead;
    float s = 0.f;
#pragma unroll 16
    for (int d = 0; d < kDimHead; ++d) s = fmaf(q[d], k[d], s);
    sc[(h * seq + i) * kMaxSeq + j] = s * scale;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < heads * seq; r += NT) {
    float* row = sc + r * kMaxSeq;
    float m = -INFINITY;
    for (int j = 0; j < seq; ++j) m = fmaxf(m, row[j]);
    float sum = 0.f;
    for (int j = 0; j < seq; ++j) {
      const float e = expf(row[j] - m);
      row[j] = e;
      sum += e;
    }
    const float inv = 1.0f / sum;
    for (int j = 0; j < seq; ++j) row[j] *= inv;
    lse[(size_t)b * heads * seq + r] = m + logf(sum);
  }
  __syncthreads();
  for (int it = threadIdx.x; it < seq * HD; it += NT) {
    const int i = it / HD, c = it % HD, h = c / kDimHead;
    const float* p = sc + (h * seq + i) * kMaxSeq;
    float acc = 0.f;
    for (int j = 0; j < seq; ++j) acc = fmaf(p[j], sq[j * ld + 2 * HD + c], acc);
    if (kBf) {
      ob[((size_t)b * seq + i) * HD + c] = bf16_bits(acc);
      if (o) o[((size_t)b * seq + i) * HD + c] = acc;
    } else {
      o[((size_t)b * seq + i) * HD + c] = acc;
    }
  }
  if (kBf && b == (int)gridDim.x - 1) zero_pad_rows(ob, (int64_t)gridDim.x * seq, rows_pad, HD);
}

// P = exp(scale q k^T - lse) recomputed; dP = dO V^T; D = rowsum(P * dP) (= rowsum(dO * O): O = P V);
// dS = P (dP - D) scale; dQ = dS K, dK = dS^T Q, dV = P^T dO -> dqkv [B*seq][3*HD]
// kBf: dqkv also (or only: dqkv may be NULL) as the bf16 carrier dqb [rows_pad][3*HD]
template <bool kBf>
__global__ void __launch_bounds__(NT) vit_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ lse,
                                                   const float* __restrict__ dout, int seq, int heads, float scale,
                                                   float* __restrict__ dqkv, unsigned short* __restrict__ dqb, int rows_pad) {
  extern __shared__ float lds[];
  const int HD = heads * kDimHead, ld = 3 * HD + 1, ldo = HD + 1;
  float* sq = lds;                                   // [seq][ld]
  float* sd = sq + seq * ld;                         // [seq][ldo]  dO
  float* sp = sd + seq * ldo;                        // [heads][seq][kMaxSeq]  P
  float* ss = sp + heads * seq * kMaxSeq;            // [heads][seq][kMaxSeq]  dP, then dS
  const int b = blockIdx.x;
  const float* src = qkv + (size_t)b * seq * 3 * HD;
  for (int e = threadIdx.x; e < seq * 3 * HD / 4; e += NT) {
    const float4 v = reinterpret_cast<const float4*>(src)[e];
    const int r = (4 * e) / (3 * HD), c = (4 * e) % (3 * HD);
    float* d = sq + r * ld + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  const float* dsrc = dout + (size_t)b * seq * HD;
  for (int e = threadIdx.x; e < seq * HD / 4; e += NT) {
    const float4 v = reinterpret_cast<const float4*>(dsrc)[e];
    const int r = (4 * e) / HD, c = (4 * e) % HD;
    float* d = sd + r * ldo + c;
    d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < heads * seq * seq; it += NT) {
    const int h = it / (seq * seq), i = (it / seq) % seq, j = it % seq;
    const float* q = sq + i * ld + h * kDimHead;
    const float* k = sq + j * ld + HD + h * kDimHead;
    const float* v = sq + j * ld + 2 * HD + h * kDimHead;
    const float* g = sd + i * ldo + h * kDimHead;
    float s = 0.f, dp = 0.f;
#pragma unroll 16
    for (int d = 0; d < kDimHead; ++d) {
      s = fmaf(q[d], k[d], s);
      dp = fmaf(g[d], v[d], dp);
    }
    const int at = (h * seq + i) * kMaxSeq + j;
    sp[at] = expf(s * scale - lse[(size_t)b * heads * seq + h * seq + i]);
    ss[at] = dp;
  }
  __syncthreads();
  for (int r = threadIdx.x; r < heads * seq; r += NT) {
    const float* p = sp + r * kMaxSeq;
    float* d = ss + r * kMaxSeq;
    float D = 0.f;
    for (int j = 0; j < seq; ++j) D = fmaf(p[j], d[j], D);
    for (int j = 0; j < seq; ++j) d[j] = p[j] * (d[j] - D) * scale;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < seq * 3 * HD; it += NT) {
    const int i = it / (3 * HD), c = it % (3 * HD), part = c / HD, cc = c % HD, h = cc / kDimHead;
    float acc = 0.f;
    if (part == 0) {            // dq_i = sum_j dS_ij k_j
      const float* ds = ss + (h * seq + i) * kMaxSeq;
      for (int j = 0; j < seq; ++j) acc = fmaf(ds[j], sq[j * ld + HD + cc], acc);
    } else if (part == 1) {     // dk_i = sum_q dS_qi q_q
      for (int r = 0; r < seq; ++r) acc = fmaf(ss[(h * seq + r) * kMaxSeq + i], sq[r * ld + cc], acc);
    } else {                    // dv_i = sum_q P_qi dO_q
      for (int r = 0; r < seq; ++r) acc = fmaf(sp[(h * seq + r) * kMaxSeq + i], sd[r * ldo + cc], acc);
    }
    if (kBf) {
      dqb[((size_t)b * seq + i) * 3 * HD + c] = bf16_bits(acc);
      if (dqkv) dqkv[((size_t)b * seq + i) * 3 * HD + c] = acc;
    } else {
      dqkv[((size_t)b * seq + i) * 3 * HD + c] = acc;
    }
  }
  if (kBf && b == (int)gridDim.x - 1) zero_pad_rows(dqb, (int64_t)gridDim.x * seq, rows_pad, 3 * HD);
}

size_t attn_fwd_lds(int seq, int heads) {
  return sizeof(float) * ((size_t)seq * (3 * heads * kDimHead + 1) + (size_t)heads * seq * kMaxSeq);
}
size_t attn_bwd_lds(int seq, int heads) {
  return sizeof(float) * ((size_t)seq * (3 * heads * kDimHead + 1) + (size_t)seq * (heads * kDimHead + 1) +
                          2 * (size_t)heads * seq * kMaxSeq);
}

// ---------------------------------------------------------------------------------------------- GELU (exact)
__device__ __forceinline__ float gelu_of(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

__device__ __forceinline__ float gelu_grad_of(float v, float g) {
  const float cdf = 0.5f * (1.0f + erff(v * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * expf(-0.5f * v * v);
  return g * (cdf + v * pdf);
}

// kBf: the result also (or only: y may be NULL) as the bf16 carrier yb of n_pad elements, zero past n
template <bool kBf>
__global__ void __launch_bounds__(NT) vit_gelu_fwd(const float* __restrict__ u, int64_t n, float* __restrict__ y,
                                                   unsigned short* __restrict__ yb, int64_t n_pad) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < (kBf ? n_pad : n); i += (int64_t)gridDim.x * NT) {
    if (kBf) {
      if (i >= n) {
        yb[i] = 0;
        continue;
      }
      const float r = gelu_of(u[i]);
      yb[i] = bf16_bits(r);
      if (y) y[i] = r;
    } else {
      y[i] = gelu_of(u[i]);
    }
  }
}

template <bool kBf>
__global__ void __launch_bounds__(NT) vit_gelu_bwd(const float* __restrict__ u, const float* __restrict__ dy, int64_t n,
                                                   float* __restrict__ du, unsigned short* __restrict__ dub, int64_t n_pad) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < (kBf ? n_pad : n); i += (int64_t)gridDim.x * NT) {
    if (kBf) {
      if (i >= n) {
        dub[i] = 0;
        continue;
      }
      const float r = gelu_grad_of(u[i], dy[i]);
      dub[i] = bf16_bits(r);
      if (du) du[i] = r;
    } else {
      du[i] = gelu_grad_of(u[i], dy[i]);
    }
  }
}

// fp32 [n] (n % 4 == 0) -> bf16 carrier [n_pad], zero past n
__global__ void __launch_bounds__(NT) vit_bf16_pack(const float* __restrict__ x, int64_t n, int64_t n_pad,
                                                    unsigned short* __restrict__ out) {
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n_pad / 4; e += (int64_t)gridDim.x * NT) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * e < n) v = reinterpret_cast<const float4*>(x)[e];
    st_bf16x4(out + 4 * e, v);
  }
}

// ---------------------------------------------------------------------------------------------- token head, last layer
// y[t][o] = b[o] + sum_k relu(z[t][k]) W[o][k]: one wave per row
__global__ void __launch_bounds__(NT) vit_head_fwd(const float* __restrict__ z, int T, int K, const float* __restrict__ W,
                                                   const float* __restrict__ bias, int out_d, float* __restrict__ y) {
  const int t = blockIdx.x * (NT / kWave) + threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (t >= T) return;
  float acc[kHeadMaxOut] = {0.f, 0.f, 0.f, 0.f};
  for (int k = lane; k < K; k += kWave) {
    const float r = relu_f(z[(size_t)t * K + k]);
    for (int o = 0; o < out_d; ++o) acc[o] = fmaf(r, W[o * K + k], acc[o]);
  }
  for (int o = 0; o < out_d; ++o) {
    const float s = wave_sum(acc[o]);
    if (lane == 0) y[(size_t)t * out_d + o] = s + bias[o];
  }
}

// dz[t][k] = [z > 0 or NaN] sum_o dy[t][o] W[o][k]; partial[chunk] = dW [out_d][K], then db [out_d]
__global__ void __launch_bounds__(NT) vit_head_bwd(const float* __restrict__ dy, const float* __restrict__ z, int T, int K,
                                                   const float* __restrict__ W, int out_d, float* __restrict__ dz,
                                                   float* __restrict__ part) {
  __shared__ float red[NT / kWave][kHeadMaxOut * kHeadMaxK + kHeadMaxOut];
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  float dw[kHeadMaxOut][kHeadMaxK / kWave], db[kHeadMaxOut];
#pragma unroll
  for (int o = 0; o < kHeadMaxOut; ++o) {
    db[o] = 0.f;
#pragma unroll
    for (int m = 0; m < kHeadMaxK / kWave; ++m) dw[o][m] = 0.f;
  }
  const int r0 = blockIdx.x * kChunkRows, r1 = min(T, r0 + kChunkRows);
  for (int t = r0 + w; t < r1; t += NT / kWave) {
    float g[kHeadMaxOut];
#pragma unroll
    for (int o = 0; o < kHeadMaxOut; ++o) {
      g[o] = o < out_d ? dy[(size_t)t * out_d + o] : 0.f;
      db[o] += g[o];
    }
#pragma unroll
    for (int m = 0; m < kHeadMaxK / kWave; ++m) {
      const int k = lane + m * kWave;
      if (k < K) {
        const float zz = z[(size_t)t * K + k], r = relu_f(zz);
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < kHeadMaxOut; ++o)
          if (o < out_d) {
            s = fmaf(g[o], W[o * K + k], s);
            dw[o][m] = fmaf(g[o], r, dw[o][m]);
          }
        dz[(size_t)t * K + k] = relu_on(zz) ? s : 0.f;
      }
    }
  }
#pragma unroll
  for (int o = 0; o < kHeadMaxOut; ++o) {
    if (o >= out_d) continue;
#pragma unroll
    for (int m = 0; m < kHeadMaxK / kWave; ++m) {
      const int k = lane + m * kWave;
      if (k < K) red[w][o * K + k] = dw[o][m];
    }
    if (lane == 0) red[w][out_d * K + o] = db[o];
  }
  __syncthreads();
  const int ncols = out_d * K + out_d;
  float* p = part + (size_t)blockIdx.x * ncols;
  for (int c = threadIdx.x; c < ncols; c += NT) p[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

// ---------------------------------------------------------------------------------------------- dynamic-scale planes
__global__ void __launch_bounds__(NT) vit_amax(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
  __shared__ float red[NT / kWave];
  float m = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) m = fmaxf(m, fabsf(x[i]));
  m = wave_max(m);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

typedef _Float16 vh4 __attribute__((ext_vector_type(4)));

// S = the power of two that maps max |x| into [2^13, 2^14) (1 for a zero or non-finite max); scale = {S, 1/S,
// other[1] / S} (the last: the dyn_inv of a GEMM whose other operand has dynamic planes too).  Planes: h = fp16(S x),
// l = fp16((S x - h) 2048), rows_pad * cols elements each, the rows past `rows` zero.
__global__ void __launch_bounds__(NT) vit_split(const float* __restrict__ x, int64_t rows, int64_t cols, int64_t rows_pad,
                                                const float* __restrict__ part, int nparts, const float* __restrict__ other,
                                                float* __restrict__ scale, unsigned short* __restrict__ planes) {
  __shared__ float red[NT / kWave];
  float m = 0.f;
  for (int i = threadIdx.x; i < nparts; i += NT) m = fmaxf(m, part[i]);
  m = wave_max(m);
  if (threadIdx.x % kWave == 0) red[threadIdx.x / kWave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float S = 1.0f;
  if (m > 0.f && isfinite(m)) {
    int ex;
    frexpf(m, &ex);                                   // m in [2^(ex-1), 2^ex)
    S = ldexpf(1.0f, min(100, max(-100, 14 - ex)));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    scale[0] = S;
    scale[1] = 1.0f / S;
    scale[2] = other ? other[1] / S : 1.0f / S;
  }
  const int64_t n4 = rows_pad * cols / 4, valid = rows * cols;
  unsigned short* hp = planes;
  unsigned short* lp = planes + rows_pad * cols;
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < n4; e += (int64_t)gridDim.x * NT) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (4 * e < valid) v = reinterpret_cast<const float4*>(x)[e];
    const float a[4] = {v.x * S, v.y * S, v.z * S, v.w * S};
    vh4 hh, ll;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hh[j] = (_Float16)a[j];
      ll[j] = (_Float16)((a[j] - (float)hh[j]) * 2048.0f);
    }
    reinterpret_cast<vh4*>(hp)[e] = hh;
    reinterpret_cast<vh4*>(lp)[e] = ll;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace pl

using namespace pl;

// ---------------------------------------------------------------------------------------------- C ABI
extern "C" int pl_vit_embed_fwd(const float* x2d, int64_t T, int in_d, int seq, const float* W, const float* b,
                                const float* pos, int H, float* x, void* stream) {
  if (!x2d || !W || !b || !pos || !x) PL_FAIL(PL_EINVAL, "pl_vit_embed_fwd: null pointer");
  if (T <= 0 || T > INT32_MAX / 1024 || in_d < 1 || in_d > 8 || seq <= 0 || T % seq || H <= 0 || H > 4096)
    PL_FAIL(PL_ESHAPE, "pl_vit_embed_fwd: T=%lld in_d=%d seq=%d H=%d", (long long)T, in_d, seq, H);
  hipLaunchKernelGGL(vit_embed_fwd, dim3(blocks_for(T * H, NT)), dim3(NT), 0, (hipStream_t)stream, x2d, (int)T, in_d, seq, W,
                     b, pos, H, x);
  PL_CHECK_LAUNCH("vit_embed_fwd");
  return PL_OK;
}

extern "C" size_t pl_vit_embed_bwd_scratch_bytes(int64_t T, int in_d, int H) {
  if (T <= 0 || in_d <= 0 || H <= 0) return 0;
  return sizeof(float) * (size_t)chunks_of(T) * (size_t)(H * in_d + H);
}

extern "C" int pl_vit_embed_bwd(const float* dx, const float* x2d, int64_t T, int in_d, int seq, int H, const float* W,
                                float* dW, float* dpos, float* dx2d, void* scratch, void* stream) {
  if (!dx || !x2d || !dW || !scratch || (dx2d && !W)) PL_FAIL(PL_EINVAL, "pl_vit_embed_bwd: null pointer");
  if (T <= 0 || T > INT32_MAX / 1024 || in_d < 1 || in_d > 8 || seq <= 0 || T % seq || H <= 0 || H > 4096)
    PL_FAIL(PL_ESHAPE, "pl_vit_embed_bwd: T=%lld in_d=%d seq=%d H=%d", (long long)T, in_d, seq, H);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nch = chunks_of(T);
  hipLaunchKernelGGL(vit_embed_bwd_part, dim3((unsigned)nch), dim3(NT), 0, s, dx, x2d, (int)T, in_d, H,
                     static_cast<float*>(scratch));
  PL_CHECK_LAUNCH("vit_embed_bwd_part");
  PL_TRY(launch_reduce(static_cast<const float*>(scratch), nch, (int64_t)H * in_d + H, dW, s));
  if (dpos) {
    hipLaunchKernelGGL(vit_embed_dpos, dim3(blocks_for((int64_t)seq * H, NT)), dim3(NT), 0, s, dx, (int)(T / seq), seq, H,
                       dpos);
    PL_CHECK_LAUNCH("vit_embed_dpos");
  }
  if (dx2d) {
    hipLaunchKernelGGL(vit_embed_dinput, dim3(blocks_for(T, NT / kWave)), dim3(NT), 0, s, dx, W, (int)T, in_d, H, dx2d);
    PL_CHECK_LAUNCH("vit_embed_dinput");
  }
  return PL_OK;
}

// ---------------------------------------------------------------------------------------------- the carrier kernels
// LayerNorm, attention and GELU, forward and backward: ONE checked launcher per kernel.  It takes the optional bf16 carrier
// of the kernel's output ([rows_pad][cols], rows past T zero; "bf16p") and the name of the entry point for its messages.
// Both exported forms are calls of it: the plain form passes no carrier, the _bf16 form its own arguments.  Without a
// carrier the <false> kernel runs and the fp32 output is required; with one it may be NULL.  Everything is checked before
// any HIP call.
static int carrier_check(const void* c, int64_t T, int64_t rows_pad, int64_t cols, const char* who) {
  if (!c) return PL_OK;
  if (rows_pad < T || rows_pad % 32 || rows_pad > INT32_MAX / 1024 || cols % 4 || rows_pad * cols > ((int64_t)1 << 40))
    PL_FAIL(PL_ESHAPE, "%s: carrier rows_pad=%lld for T=%lld rows of %lld (rows_pad >= T, rows_pad %% 32 == 0, cols %% 4 == 0)",
            who, (long long)rows_pad, (long long)T, (long long)cols);
  if (!aligned16(c)) PL_FAIL(PL_EINVAL, "%s: the bf16 carrier must be 16-byte aligned", who);
  return PL_OK;
}

static int ln_shape_ok(int64_t T, int H, int nnorm) {
  return T > 0 && T <= INT32_MAX / 1024 && H > 0 && H % 4 == 0 && H <= 4 * kLnMaxV * kWave && nnorm >= 0 && nnorm <= 2;
}

static int ln_fwd(const char* who, const float* x, const float* add, int64_t T, int H, int nnorm, const float* g1,
                  const float* b1, const float* g2, const float* b2, float eps, float* x_out, float* y, void* y_bf16,
                  int64_t rows_pad, float* stats, void* stream) {
  if (!ln_shape_ok(T, H, nnorm)) PL_FAIL(PL_ESHAPE, "%s: T=%lld H=%d nnorm=%d", who, (long long)T, H, nnorm);
  if (!x || (add && !x_out) || (nnorm >= 1 && (!g1 || !b1 || !(y || y_bf16) || !stats)) || (nnorm == 2 && (!g2 || !b2)) ||
      (nnorm == 0 && (!add || y_bf16)))
    PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (!aligned16(x) || (add && (!aligned16(add) || !aligned16(x_out))) || (y && !aligned16(y)) ||
      (g1 && !aligned16(g1)) || (b1 && !aligned16(b1)) || (g2 && !aligned16(g2)) || (b2 && !aligned16(b2)))
    PL_FAIL(PL_EINVAL, "%s: x / add / x_out / y / g1 / b1 / g2 / b2 must be 16-byte aligned", who);
  PL_TRY(carrier_check(y_bf16, T, rows_pad, H, who));
  const int64_t rows = y_bf16 ? rows_pad : T;      // (the carrier kernel also zeroes the padding rows)
  hipLaunchKernelGGL(y_bf16 ? vit_ln_fwd<true> : vit_ln_fwd<false>, dim3(blocks_for(rows, NT / kWave)), dim3(NT), 0,
                     (hipStream_t)stream, x, add, (int)T, H, nnorm, g1, b1, g2, b2, eps, x_out, y, stats,
                     static_cast<unsigned short*>(y_bf16), (int)rows);
  PL_CHECK_LAUNCH("vit_ln_fwd");
  return PL_OK;
}

extern "C" int pl_vit_ln_fwd(const float* x, const float* add, int64_t T, int H, int nnorm, const float* g1,
                             const float* b1, const float* g2, const float* b2, float eps, float* x_out, float* y,
                             float* stats, void* stream) {
  return ln_fwd("pl_vit_ln_fwd", x, add, T, H, nnorm, g1, b1, g2, b2, eps, x_out, y, nullptr, 0, stats, stream);
}

extern "C" int pl_vit_ln_fwd_bf16(const float* x, const float* add, int64_t T, int H, int nnorm, const float* g1,
                                  const float* b1, const float* g2, const float* b2, float eps, float* x_out, float* y,
                                  void* y_bf16, int64_t rows_pad, float* stats, void* stream) {
  return ln_fwd("pl_vit_ln_fwd_bf16", x, add, T, H, nnorm, g1, b1, g2, b2, eps, x_out, y, y_bf16, rows_pad, stats, stream);
}

extern "C" size_t pl_vit_ln_bwd_scratch_bytes(int64_t T, int H, int nnorm) {
  if (T <= 0 || H <= 0 || nnorm <= 0) return 0;
  return sizeof(float) * (size_t)chunks_of(T) * (size_t)(2 * nnorm * H);
}

static int ln_bwd(const char* who, const float* dy, const float* dres, const float* x, const float* stats, int64_t T, int H,
                  int nnorm, const float* g1, const float* b1, const float* g2, float* dx, void* dx_bf16, int64_t rows_pad,
                  float* dgb, void* scratch, void* stream) {
  if (!ln_shape_ok(T, H, nnorm) || nnorm < 1) PL_FAIL(PL_ESHAPE, "%s: T=%lld H=%d nnorm=%d", who, (long long)T, H, nnorm);
  if (!dy || !x || !stats || !g1 || !(dx || dx_bf16) || !dgb || !scratch || (nnorm == 2 && (!b1 || !g2)))
    PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (!aligned16(dy) || !aligned16(x) || (dx && !aligned16(dx)) || (dres && !aligned16(dres)) || !aligned16(g1) ||
      (b1 && !aligned16(b1)) || (g2 && !aligned16(g2)))
    PL_FAIL(PL_EINVAL, "%s: dy / x / dx / dres / g1 / b1 / g2 must be 16-byte aligned", who);
  PL_TRY(carrier_check(dx_bf16, T, rows_pad, H, who));
  hipStream_t s = (hipStream_t)stream;
  const int64_t nch = chunks_of(T);
  hipLaunchKernelGGL(dx_bf16 ? vit_ln_bwd<true> : vit_ln_bwd<false>, dim3((unsigned)nch), dim3(NT),
                     sizeof(float) * (NT / kWave) * 2 * nnorm * H, s, dy, dres, x, stats, (int)T, H, nnorm, g1, b1, g2, dx,
                     static_cast<float*>(scratch), static_cast<unsigned short*>(dx_bf16), (int)(dx_bf16 ? rows_pad : T));
  PL_CHECK_LAUNCH("vit_ln_bwd");
  return launch_reduce(static_cast<const float*>(scratch), nch, 2 * nnorm * H, dgb, s);
}

extern "C" int pl_vit_ln_bwd(const float* dy, const float* dres, const float* x, const float* stats, int64_t T, int H,
                             int nnorm, const float* g1, const float* b1, const float* g2, float* dx, float* dgb,
                             void* scratch, void* stream) {
  return ln_bwd("pl_vit_ln_bwd", dy, dres, x, stats, T, H, nnorm, g1, b1, g2, dx, nullptr, 0, dgb, scratch, stream);
}

extern "C" int pl_vit_ln_bwd_bf16(const float* dy, const float* dres, const float* x, const float* stats, int64_t T, int H,
                                  int nnorm, const float* g1, const float* b1, const float* g2, float* dx, void* dx_bf16,
                                  int64_t rows_pad, float* dgb, void* scratch, void* stream) {
  return ln_bwd("pl_vit_ln_bwd_bf16", dy, dres, x, stats, T, H, nnorm, g1, b1, g2, dx, dx_bf16, rows_pad, dgb, scratch,
                stream);
}

static int attn_check(int64_t B, int seq, int heads, int dim_head, size_t lds, const char* what) {
  if (B <= 0 || B > INT32_MAX / 4096 || seq < 1 || seq > kMaxSeq || heads < 1 || dim_head != kDimHead || lds > kLdsMax)
    PL_FAIL(PL_ESHAPE, "%s: B=%lld seq=%d heads=%d dim_head=%d (seq <= %d, dim_head %d, LDS %zu of %zu bytes)", what,
            (long long)B, seq, heads, dim_head, kMaxSeq, kDimHead, lds, kLdsMax);
  return PL_OK;
}

extern "C" int pl_vit_attn_supported(int seq, int heads, int dim_head) {
  return seq >= 1 && seq <= kMaxSeq && heads >= 1 && dim_head == kDimHead && attn_bwd_lds(seq, heads) <= kLdsMax;
}

static int attn_fwd(const char* who, const float* qkv, int64_t B, int seq, int heads, int dim_head, float scale, float* o,
                    void* o_bf16, int64_t rows_pad, float* lse, void* stream) {
  if (!qkv || !(o || o_bf16) || !lse) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  const size_t lds = attn_fwd_lds(seq, heads);
  PL_TRY(attn_check(B, seq, heads, dim_head, lds, who));
  if (!aligned16(qkv)) PL_FAIL(PL_EINVAL, "%s: qkv must be 16-byte aligned", who);
  PL_TRY(carrier_check(o_bf16, B * seq, rows_pad, (int64_t)heads * kDimHead, who));
  hipLaunchKernelGGL(o_bf16 ? vit_attn_fwd<true> : vit_attn_fwd<false>, dim3((unsigned)B), dim3(NT), lds,
                     (hipStream_t)stream, qkv, seq, heads, scale, o, lse, static_cast<unsigned short*>(o_bf16),
                     (int)(o_bf16 ? rows_pad : 0));
  PL_CHECK_LAUNCH("vit_attn_fwd");
  return PL_OK;
}

extern "C" int pl_vit_attn_fwd(const float* qkv, int64_t B, int seq, int heads, int dim_head, float scale, float* o,
                               float* lse, void* stream) {
  return attn_fwd("pl_vit_attn_fwd", qkv, B, seq, heads, dim_head, scale, o, nullptr, 0, lse, stream);
}

extern "C" int pl_vit_attn_fwd_bf16(const float* qkv, int64_t B, int seq, int heads, int dim_head, float scale, float* o,
                                    void* o_bf16, int64_t rows_pad, float* lse, void* stream) {
  return attn_fwd("pl_vit_attn_fwd_bf16", qkv, B, seq, heads, dim_head, scale, o, o_bf16, rows_pad, lse, stream);
}

static int attn_bwd(const char* who, const float* qkv, const float* lse, const float* dout, int64_t B, int seq, int heads,
                    int dim_head, float scale, float* dqkv, void* dqkv_bf16, int64_t rows_pad, void* stream) {
  if (!qkv || !lse || !dout || !(dqkv || dqkv_bf16)) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  const size_t lds = attn_bwd_lds(seq, heads);
  PL_TRY(attn_check(B, seq, heads, dim_head, lds, who));
  if (!aligned16(qkv) || !aligned16(dout)) PL_FAIL(PL_EINVAL, "%s: qkv / dout must be 16-byte aligned", who);
  PL_TRY(carrier_check(dqkv_bf16, B * seq, rows_pad, 3 * (int64_t)heads * kDimHead, who));
  hipLaunchKernelGGL(dqkv_bf16 ? vit_attn_bwd<true> : vit_attn_bwd<false>, dim3((unsigned)B), dim3(NT), lds,
                     (hipStream_t)stream, qkv, lse, dout, seq, heads, scale, dqkv, static_cast<unsigned short*>(dqkv_bf16),
                     (int)(dqkv_bf16 ? rows_pad : 0));
  PL_CHECK_LAUNCH("vit_attn_bwd");
  return PL_OK;
}

extern "C" int pl_vit_attn_bwd(const float* qkv, const float* lse, const float* dout, int64_t B, int seq, int heads,
                               int dim_head, float scale, float* dqkv, void* stream) {
  return attn_bwd("pl_vit_attn_bwd", qkv, lse, dout, B, seq, heads, dim_head, scale, dqkv, nullptr, 0, stream);
}

extern "C" int pl_vit_attn_bwd_bf16(const float* qkv, const float* lse, const float* dout, int64_t B, int seq, int heads,
                                    int dim_head, float scale, float* dqkv, void* dqkv_bf16, int64_t rows_pad, void* stream) {
  return attn_bwd("pl_vit_attn_bwd_bf16", qkv, lse, dout, B, seq, heads, dim_head, scale, dqkv, dqkv_bf16, rows_pad, stream);
}

static unsigned grid_stride_blocks(int64_t n) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(1, (n + NT - 1) / NT), 8192);
}

static int rows_cols_ok(int64_t rows, int64_t cols) {
  return rows > 0 && cols > 0 && cols % 4 == 0 && rows <= INT32_MAX / 1024 && rows * cols <= ((int64_t)1 << 40);
}

// GELU is elementwise.  The plain forms take a count (plain: `rows` elements, any n > 0), the _bf16 forms [rows][cols]
// with cols % 4 == 0, which a carrier needs.
static int gelu_shape(const char* who, int64_t rows, int64_t cols, bool plain) {
  if (plain && rows <= 0) PL_FAIL(PL_ESHAPE, "%s: n=%lld", who, (long long)rows);
  if (!plain && !rows_cols_ok(rows, cols)) PL_FAIL(PL_ESHAPE, "%s: rows=%lld cols=%lld", who, (long long)rows, (long long)cols);
  return PL_OK;
}

static int gelu_fwd(const char* who, bool plain, const float* u, int64_t rows, int64_t cols, int64_t rows_pad, float* y,
                    void* y_bf16, void* stream) {
  if (!u || !(y || y_bf16)) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PL_TRY(gelu_shape(who, rows, cols, plain));
  PL_TRY(carrier_check(y_bf16, rows, rows_pad, cols, who));
  const int64_t n = plain ? rows : rows * cols, n_pad = y_bf16 ? rows_pad * cols : n;
  hipLaunchKernelGGL(y_bf16 ? vit_gelu_fwd<true> : vit_gelu_fwd<false>, dim3(grid_stride_blocks(n_pad)), dim3(NT), 0,
                     (hipStream_t)stream, u, n, y, static_cast<unsigned short*>(y_bf16), n_pad);
  PL_CHECK_LAUNCH("vit_gelu_fwd");
  return PL_OK;
}

extern "C" int pl_vit_gelu_fwd(const float* u, int64_t n, float* y, void* stream) {
  return gelu_fwd("pl_vit_gelu_fwd", true, u, n, 0, 0, y, nullptr, stream);
}

extern "C" int pl_vit_gelu_fwd_bf16(const float* u, int64_t rows, int64_t cols, int64_t rows_pad, float* y, void* y_bf16,
                                    void* stream) {
  return gelu_fwd("pl_vit_gelu_fwd_bf16", false, u, rows, cols, rows_pad, y, y_bf16, stream);
}

static int gelu_bwd(const char* who, bool plain, const float* u, const float* dy, int64_t rows, int64_t cols,
                    int64_t rows_pad, float* du, void* du_bf16, void* stream) {
  if (!u || !dy || !(du || du_bf16)) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PL_TRY(gelu_shape(who, rows, cols, plain));
  PL_TRY(carrier_check(du_bf16, rows, rows_pad, cols, who));
  const int64_t n = plain ? rows : rows * cols, n_pad = du_bf16 ? rows_pad * cols : n;
  hipLaunchKernelGGL(du_bf16 ? vit_gelu_bwd<true> : vit_gelu_bwd<false>, dim3(grid_stride_blocks(n_pad)), dim3(NT), 0,
                     (hipStream_t)stream, u, dy, n, du, static_cast<unsigned short*>(du_bf16), n_pad);
  PL_CHECK_LAUNCH("vit_gelu_bwd");
  return PL_OK;
}

extern "C" int pl_vit_gelu_bwd(const float* u, const float* dy, int64_t n, float* du, void* stream) {
  return gelu_bwd("pl_vit_gelu_bwd", true, u, dy, n, 0, 0, du, nullptr, stream);
}

extern "C" int pl_vit_gelu_bwd_bf16(const float* u, const float* dy, int64_t rows, int64_t cols, int64_t rows_pad, float* du,
                                    void* du_bf16, void* stream) {
  return gelu_bwd("pl_vit_gelu_bwd_bf16", false, u, dy, rows, cols, rows_pad, du, du_bf16, stream);
}

static int head_shape_ok(int64_t T, int K, int out_d) {
  return T > 0 && T <= INT32_MAX / 1024 && K > 0 && K <= kHeadMaxK && out_d >= 1 && out_d <= kHeadMaxOut;
}

extern "C" int pl_vit_head_fwd(const float* z, int64_t T, int K, const float* W, const float* b, int out_d, float* y,
                               void* stream) {
  if (!z || !W || !b || !y) PL_FAIL(PL_EINVAL, "pl_vit_head_fwd: null pointer");
  if (!head_shape_ok(T, K, out_d)) PL_FAIL(PL_ESHAPE, "pl_vit_head_fwd: T=%lld K=%d out_d=%d", (long long)T, K, out_d);
  hipLaunchKernelGGL(vit_head_fwd, dim3(blocks_for(T, NT / kWave)), dim3(NT), 0, (hipStream_t)stream, z, (int)T, K, W, b,
                     out_d, y);
  PL_CHECK_LAUNCH("vit_head_fwd");
  return PL_OK;
}

extern "C" size_t pl_vit_head_bwd_scratch_bytes(int64_t T, int K, int out_d) {
  if (T <= 0 || K <= 0 || out_d <= 0) return 0;
  return sizeof(float) * (size_t)chunks_of(T) * (size_t)(out_d * K + out_d);
}

extern "C" int pl_vit_head_bwd(const float* dy, const float* z, int64_t T, int K, const float* W, int out_d, float* dz,
                               float* dWb, void* scratch, void* stream) {
  if (!dy || !z || !W || !dz || !dWb || !scratch) PL_FAIL(PL_EINVAL, "pl_vit_head_bwd: null pointer");
  if (!head_shape_ok(T, K, out_d)) PL_FAIL(PL_ESHAPE, "pl_vit_head_bwd: T=%lld K=%d out_d=%d", (long long)T, K, out_d);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nch = chunks_of(T);
  hipLaunchKernelGGL(vit_head_bwd, dim3((unsigned)nch), dim3(NT), 0, s, dy, z, (int)T, K, W, out_d, dz,
                     static_cast<float*>(scratch));
  PL_CHECK_LAUNCH("vit_head_bwd");
  return launch_reduce(static_cast<const float*>(scratch), nch, (int64_t)out_d * K + out_d, dWb, s);
}

extern "C" size_t pl_vit_planes_scratch_bytes(void) { return sizeof(float) * kAmaxBlocks; }

extern "C" int pl_vit_planes_dyn(const float* x, int64_t rows, int64_t cols, int64_t rows_pad, const float* other_scale,
                                 float* scale, void* planes, void* scratch, void* stream) {
  if (!x || !scale || !planes || !scratch) PL_FAIL(PL_EINVAL, "pl_vit_planes_dyn: null pointer");
  if (rows <= 0 || cols <= 0 || cols % 4 || rows_pad < rows || rows_pad * cols > ((int64_t)1 << 40))
    PL_FAIL(PL_ESHAPE, "pl_vit_planes_dyn: rows=%lld cols=%lld rows_pad=%lld", (long long)rows, (long long)cols,
            (long long)rows_pad);
  if (!aligned16(x) || (reinterpret_cast<uintptr_t>(planes) & 7) || ((rows_pad * cols) & 3))
    PL_FAIL(PL_EINVAL, "pl_vit_planes_dyn: misaligned operand (x must be 16-byte aligned, planes 8-byte, rows_pad * cols %% 4 == 0)");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = rows * cols;
  const int nb = (int)std::min<int64_t>(kAmaxBlocks, std::max<int64_t>(1, (n + 4 * NT - 1) / (4 * NT)));
  hipLaunchKernelGGL(vit_amax, dim3(nb), dim3(NT), 0, s, x, n, static_cast<float*>(scratch));
  PL_CHECK_LAUNCH("vit_amax");
  hipLaunchKernelGGL(vit_split, dim3(grid_stride_blocks(rows_pad * cols / 4)), dim3(NT), 0, s, x, rows, cols, rows_pad,
                     static_cast<const float*>(scratch), nb, other_scale, scale, static_cast<unsigned short*>(planes));
  PL_CHECK_LAUNCH("vit_split");
  return PL_OK;
}

extern "C" int pl_vit_bf16_pack(const float* x, int64_t rows, int64_t cols, int64_t rows_pad, void* out, void* stream) {
  if (!x || !out) PL_FAIL(PL_EINVAL, "pl_vit_bf16_pack: null pointer");
  if (!rows_cols_ok(rows, cols)) PL_FAIL(PL_ESHAPE, "pl_vit_bf16_pack: rows=%lld cols=%lld", (long long)rows, (long long)cols);
  PL_TRY(carrier_check(out, rows, rows_pad, cols, "pl_vit_bf16_pack"));
  if (!aligned16(x)) PL_FAIL(PL_EINVAL, "pl_vit_bf16_pack: x must be 16-byte aligned");
  hipLaunchKernelGGL(vit_bf16_pack, dim3(grid_stride_blocks(rows_pad * cols / 4)), dim3(NT), 0, (hipStream_t)stream, x,
                     rows * cols, rows_pad * cols, static_cast<unsigned short*>(out));
  PL_CHECK_LAUNCH("vit_bf16_pack");
  return PL_OK;
}

// One hidden layer of the lifter per launch, for SMALL batches (B <= 64 rows: the reference's own batch_size = 64,
// phase1_lifting/train_1.py:194) -- and, in evaluation, for every batch off the tile grid (M <= 512).
//
// At this size every kernel of the step is launch latency (4.5-9 us each for 256 KB of data) and a hidden layer was four of
// them forward (split-K GEMM, its reduce, BatchNorm statistics + apply) and four backward.  BatchNorm is what forces the
// boundaries -- its statistics need every row of a column -- so here a workgroup OWNS 16 columns for ALL rows:
//   small_first_fwd_kernel   the first layer (34 / 51 inputs: contraction on the vector unit), then the forward tail
//   small_fwd_kernel         z = a W^T + b on its columns -- K split over the workgroup's eight waves, row-contiguous loads
//                            through a wave-private LDS image, exact-fp32 v_mfma_f32_16x16x4_f32 or (PL_F16X3) three
//                            v_mfma_f32_16x16x32_f16 on fp16 planes, wave partials through LDS in wave order -- then, the
//                            columns being complete, the forward tail: batch statistics, running statistics, scale / shift,
//                            ReLU, dropout, the residual add, the ReLU & keep bitmap (Linear + BatchNorm1d + ReLU + Dropout
//                            (+ skip), baselineModel.py:33-37 / 39-45 / 79-95); evaluation: the fold on the running
//                            statistics instead, grid also over 64-row blocks; the last layer also leaves the slabs of the
//                            output Linear
//   small_mse_kernel         y = bias + slabs, MSE forward + backward (or, evaluation, y alone)
//   small_top_bwd_kernel     g = dy W2, BatchNorm backward of the top hidden layer, dW2, db2, loss, step counter
//   small_bwd_kernel         three roles by workgroup: g = dz W (+ skip gradient) on its columns and the BatchNorm backward
//                            of the layer BELOW (+ the first layer's weight gradient); the layer's own weight gradient
//                            dz^T a, one 128 x 64 tile each; a slice of the AdamW step
// (the autograd of the same modules, train_1.py:95-96).  64 column workgroups at H = 1024: column ownership caps the
// parallelism, and every one of them reads all of the activations -- what a launch waits for is its 320 KB of operands through
// one CU's vector memory unit and LDS, then (exact fp32) 3.4 us of MFMA issue.  DESIGN.md 3.7 has the measurements.
//
// Bitmap of the layers produced here ("tile format", private to the small path: written by the forward tail, read by the
// backward tail and by bn_small_bwd_kernel<.., true>): element (r, c) is bit (r & 15) * 4 + ((c >> 2) & 3) of word
// (c >> 4) * 16 + (r >> 4) * 4 + (c & 3) -- what a ballot over the tail's lanes yields.
#include <stdlib.h>

#include <algorithm>

#include "adamw.h"
#include "bn_pieces.h"
#include "philox.h"
#include "pl_internal.h"
#include "plane_store.h"

namespace pl {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int NTHR = 512, NWAVE = 8, COLS = 16, ROWS = 64;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float comp(const float4& v, int e) { return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w)); }

// the workgroup's 16 columns: column blocks in XCD-contiguous runs (workgroup b runs on XCD b % 8), so that the two blocks
// sharing a 128-byte line of W (NN) fetch it into one L2
__device__ __forceinline__ int col_block(int b, int nb) {
  if (nb & 7) return b;
  return (b & 7) * (nb >> 3) + (b >> 3);
}

// part[wave][64 x 16] = A[:, wave's k range] * B[that range, c0 .. c0+15]; wave's range = STEPS * 32 k.
//   B_KS = false: B [N][K] k-contiguous (forward, W rows);  true: B [K][N] (backward: dz W, 64-byte segments of W's rows)
// The MFMA wants its 16 rows on adjacent lanes; memory has k on adjacent addresses.  (First version: every lane fetched the
// 32 bytes of its own row straight into its fragment -- 64 separate requests per instruction: 8.5 us of a 15 us kernel for
// 320 KB, measured with the MFMAs removed.)  So the global loads are row-contiguous -- eight lanes per 128-byte row piece, all
// of the wave's 40 in flight at once -- and each 32-k step passes through a wave-private LDS image [row][36 floats] (the pad
// makes both the b128 writes and the fragment reads conflict-free); no barrier: one wave's DS operations execute in order.
// Rows >= M read row M - 1 (valid memory); their results are never used.
constexpr int LDR = 36;                                   // floats per row of the step image
constexpr int LDH = 40;                                   // halves per row of one PLANE's step image (f16x3 form below)
// per wave: 64 rows of A, 16 of B -- fp32 rows of LDR floats, or two fp16 planes of LDH halves each (the larger of the two)
constexpr int STAGE = (ROWS + COLS) * (LDR > LDH ? LDR : LDH);
template <int STEPS, bool B_KS>
__device__ __forceinline__ void contract(const float* __restrict__ A, int lda, int M, const float* __restrict__ Bm, int ldb,
                                         int c0, float* __restrict__ part, float* __restrict__ stage) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int kb = wave * STEPS * 32;
  float* img = stage + wave * STAGE;
  float4 ga[STEPS][8], gb[STEPS][2];
  {
    const int rr = lane >> 3, q4 = 4 * (lane & 7);
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ga[s][j] = ld4(A + (size_t)min(8 * j + rr, M - 1) * lda + kb + 32 * s + q4);
      if (!B_KS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) gb[s][j] = ld4(Bm + (size_t)(c0 + 8 * j + rr) * ldb + kb + 32 * s + q4);
      } else {
#pragma unroll
        for (int j = 0; j < 2; ++j) gb[s][j] = ld4(Bm + (size_t)(kb + 32 * s + 16 * j + (lane >> 2)) * ldb + c0 + 4 * (lane & 3));
      }
      __builtin_amdgcn_sched_barrier(0);                  // (all 40 loads leave before anything below, in step order: one round trip)
    }
  }
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    {
      const int rr = lane >> 3, q4 = 4 * (lane & 7);
#pragma unroll
      for (int j = 0; j < 8; ++j) st4(img + (8 * j + rr) * LDR + q4, ga[s][j]);
      if (!B_KS) {
#pragma unroll
        for (int j = 0; j < 2; ++j) st4(img + (ROWS + 8 * j + rr) * LDR + q4, gb[s][j]);
      } else {
        // a lane holds four columns of one k: transposed into the [column][k] image
        const int kr = lane >> 2, cq = 4 * (lane & 3);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          img[(ROWS + cq + 0) * LDR + 16 * j + kr] = gb[s][j].x;
          img[(ROWS + cq + 1) * LDR + 16 * j + kr] = gb[s][j].y;
          img[(ROWS + cq + 2) * LDR + 16 * j + kr] = gb[s][j].z;
          img[(ROWS + cq + 3) * LDR + 16 * j + kr] = gb[s][j].w;
        }
      }
    }
    float4 a[4][2], b[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      a[t][0] = ld4(img + (16 * t + i) * LDR + 8 * kq);
      a[t][1] = ld4(img + (16 * t + i) * LDR + 8 * kq + 4);
    }
    b[0] = ld4(img + (ROWS + i) * LDR + 8 * kq);
    b[1] = ld4(img + (ROWS + i) * LDR + 8 * kq + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
      for (int t = 0; t < 4; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(comp(a[t][e >> 2], e & 3), comp(b[e >> 2], e & 3), acc[t], 0, 0, 0);
  }
  float* mine = part + wave * (ROWS * COLS);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) mine[(16 * t + 4 * kq + v) * COLS + i] = acc[t][v];
}

// The same contraction on fp16 operand planes (PL_F16X3 descriptors, forward): A arrives as the two planes the producing
// launch's tail wrote (h = fp16(x), l = fp16((x - h) 2048): plane_store.h), B = W is split on the fly (16 rows per workgroup:
// 32 elements per thread), and a 32-k step is three v_mfma_f32_16x16x32_f16 per row tile on two accumulators -- main = Ah Bh,
// low = Ah Bl + Al Bh, result (main + low / 2048) / (S_a S_w) -- 192 MFMA cycles per step instead of the 1,024 of the exact
// fp32 form: the 3.8 us of MFMA issue that a forward launch was waiting for becomes 0.7.  The fp32-grade arithmetic of the
// bench's large batches (gemm_planes.h), not exact fp32: only descriptors that ask for it take it.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4h __attribute__((ext_vector_type(4)));
template <int STEPS>
__device__ __forceinline__ void contract_f16(const unsigned short* __restrict__ Ah, size_t a_plane, int lda, int M,
                                             const float* __restrict__ Bm, int ldb, int c0, float w_scale, float out_scale,
                                             float* __restrict__ part, float* __restrict__ stage, uint32_t* range) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int kb = wave * STEPS * 32;
  _Float16* img = reinterpret_cast<_Float16*>(stage + wave * STAGE);
  _Float16* iAh = img;
  _Float16* iAl = img + ROWS * LDH;
  _Float16* iBh = img + 2 * ROWS * LDH;
  _Float16* iBl = iBh + COLS * LDH;
  uint4 gah[STEPS][4], gal[STEPS][4];
  float4 gb[STEPS][2];
  {
    const int rr = lane >> 2, q8 = 8 * (lane & 3);          // A planes: four lanes per 64-byte row piece, 16 rows per instruction
    const int br = lane >> 3, bq = 4 * (lane & 7);          // B fp32: eight lanes per 128-byte row piece
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned short* q = Ah + (size_t)min(16 * j + rr, M - 1) * lda + kb + 32 * s + q8;
        gah[s][j] = *reinterpret_cast<const uint4*>(q);
        gal[s][j] = *reinterpret_cast<const uint4*>(q + a_plane);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) gb[s][j] = ld4(Bm + (size_t)(c0 + 8 * j + br) * ldb + kb + 32 * s + bq);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  f32x4 acc0[4], acc1[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { acc0[t] = f32x4{0.f, 0.f, 0.f, 0.f}; acc1[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  float w_over = 0.f;                       // range guard of the weight split below: flushed once behind the loop
#pragma unroll
  for (int s = 0; s < STEPS; ++s) {
    {
      const int rr = lane >> 2, q8 = 8 * (lane & 3);
      const int br = lane >> 3, bq = 4 * (lane & 7);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *reinterpret_cast<uint4*>(iAh + (16 * j + rr) * LDH + q8) = gah[s][j];
        *reinterpret_cast<uint4*>(iAl + (16 * j + rr) * LDH + q8) = gal[s][j];
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (range) w_over = range_over4(w_over, gb[s][j], w_scale);
        const float a[4] = {gb[s][j].x * w_scale, gb[s][j].y * w_scale, gb[s][j].z * w_scale, gb[s][j].w * w_scale};
        f16x4h hh, ll;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          hh[e] = (_Float16)a[e];
          ll[e] = (_Float16)((a[e] - (float)hh[e]) * 2048.0f);
        }
        *reinterpret_cast<f16x4h*>(iBh + (8 * j + br) * LDH + bq) = hh;
        *reinterpret_cast<f16x4h*>(iBl + (8 * j + br) * LDH + bq) = ll;
      }
    }
    f16x8 ah[4], al[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      ah[t] = *reinterpret_cast<const f16x8*>(iAh + (16 * t + i) * LDH + 8 * kq);
      al[t] = *reinterpret_cast<const f16x8*>(iAl + (16 * t + i) * LDH + 8 * kq);
    }
    const f16x8 bh = *reinterpret_cast<const f16x8*>(iBh + i * LDH + 8 * kq);
    const f16x8 bl = *reinterpret_cast<const f16x8*>(iBl + i * LDH + 8 * kq);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bh, acc0[t], 0, 0, 0);
      acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[t], bl, acc1[t], 0, 0, 0);
      acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[t], bh, acc1[t], 0, 0, 0);
    }
  }
  float* mine = part + wave * (ROWS * COLS);
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v)
      mine[(16 * t + 4 * kq + v) * COLS + i] = fmaf(acc1[t][v], 1.0f / 2048.0f, acc0[t][v]) * out_scale;
  if (range) range_flush(range, PL_RANGE_SITE_LIFTER_WEIGHT, w_over);
}

// the epilogue's element of thread tid < 256: row tid >> 2 (= 16 wave + (lane >> 2)), columns c0 + 4 (tid & 3) .. + 3
__device__ __forceinline__ float4 gather_part(const float* __restrict__ part) {
  const int tid = threadIdx.x;
  float4 v = ld4(part + tid * 4);
#pragma unroll
  for (int w = 1; w < NWAVE; ++w) {
    const float4 u = ld4(part + w * (ROWS * COLS) + tid * 4);
    v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
  }
  return v;
}

// dst[idx] = src(idx) for idx < n, by the whole workgroup: BATCH loads per thread requested before the first is stored (an
// element loop keeps ONE 4-byte load in flight per thread: 5-7 dependent round trips for the 2-3 K floats staged here)
template <int BATCH, class F>
__device__ __forceinline__ void fill_lds(float* dst, int n, F src) {
  for (int base = threadIdx.x; base < n; base += BATCH * NTHR) {
    float v[BATCH];
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const int idx = base + u * NTHR;
      v[u] = src(min(idx, n - 1));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      const int idx = base + u * NTHR;
      if (idx < n) dst[idx] = v[u];
    }
  }
}

// column sums over the 64 rows of NV float4 values per thread (threads >= 256 pass zeros and get garbage): the wave's 16 rows
// by butterfly over lanes l ^ 4, 8, 16, 32, the four epilogue waves through LDS in wave order
template <int NV>
__device__ __forceinline__ void colsum(float4 (&v)[NV], float4 (*sm)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cq = lane & 3;
#pragma unroll
  for (int n = 0; n < NV; ++n)
#pragma unroll
    for (int o = 4; o <= 32; o <<= 1) {
      v[n].x += __shfl_xor(v[n].x, o); v[n].y += __shfl_xor(v[n].y, o);
      v[n].z += __shfl_xor(v[n].z, o); v[n].w += __shfl_xor(v[n].w, o);
    }
  if (wave < 4 && lane < 4) {
#pragma unroll
    for (int n = 0; n < NV; ++n) sm[n * 4 + wave][lane] = v[n];
  }
  __syncthreads();
#pragma unroll
  for (int n = 0; n < NV; ++n) {
    float4 t = sm[n * 4][cq];
#pragma unroll
    for (int w = 1; w < 4; ++w) { const float4 x = sm[n * 4 + w][cq]; t.x += x.x; t.y += x.y; t.z += x.z; t.w += x.w; }
    v[n] = t;
  }
  __syncthreads();
}

struct FwdArgs {
  const float *a, *W, *bias, *gamma, *beta, *resid;
  float *rm, *rv, *mean, *rstd, *z, *act;
  int64_t* nbt;
  uint64_t* bits;
  const uint64_t *inject, *step_dev;
  float eps, momentum, kscale;
  int B, H, K, mode;
  uint32_t thr, k0, k1, c3, layer, seed_hi;
  // the last hidden layer of a fused train step: this workgroup's share of the output Linear, ypart[blk][B][64] (columns < O) =
  // act[:, its 16 columns] W2[:, those columns]^T -- the slabs small_mse_kernel adds up (no launch for the output layer)
  const float* W2;
  float* ypart;
  int O;
  // evaluation (model.eval(), train_1.py:112-126): BatchNorm on the running statistics, Dropout the identity, nothing saved.
  // No statistic ties the rows together, so the grid also runs over 64-row blocks (blockIdx.y; Mtot rows in all): every row
  // sees the same contraction order whatever the batch, i.e. the same bits.
  int eval, Mtot;
  // PL_F16X3 descriptors: the input as fp16 planes [rows][K] (h, then l a_plane elements behind: what the launch before left in
  // outp), this layer's output also as planes for the next launch (outp; NULL: nobody reads them)
  const unsigned short* ap;
  unsigned short* outp;
  size_t a_plane, o_plane;
  // the range guard's record or NULL (pl_internal.h range_record): outp is noted at slot `site`, the weight split of the
  // planes contraction at the weight slot
  uint32_t* range;
  int site;
  // the Linear alone, for training batches of 65 ... 512 rows (stats = 1): z = a W^T + b and partial BatchNorm statistics in the
  // layout of a tile GEMM's epilogue (per 64-row group: column sums, and plain sums of squares about the group mean -- stat_sum / stat_m2
  // [groups][H], zeros for groups past the last row; NULL: none); the grid runs over the groups like an evaluation's
  int stats;
  float *stat_sum, *stat_m2;
};

// the launch's row block: blockIdx.y * 64 .. + 63 of Mtot rows (evaluation; training launches have one block of B rows)
__device__ __forceinline__ FwdArgs row_block(FwdArgs p) {
  if (!p.eval && !p.stats) { p.Mtot = p.B; return p; }
  const int r0 = blockIdx.y * ROWS;
  p.B = min(ROWS, p.Mtot - r0);
  if (p.stats) p.z += (size_t)r0 * p.H;
  p.a += (size_t)r0 * p.K;
  if (p.ap) p.ap += (size_t)r0 * p.K;
  if (p.outp) p.outp += (size_t)r0 * p.H;
  if (p.resid) p.resid += (size_t)r0 * p.H;
  p.act += (size_t)r0 * p.H;
  if (p.ypart) p.ypart += (size_t)r0 * 64;
  return p;
}

// everything behind the Linear: z (bias NOT yet added; thread tid < 256 holds row tid >> 2, columns c .. c + 3 of block blk)
// what the tail reads from memory besides z: requested BEFORE the contraction, so that its round trip is not the tail's
struct FwdPre { float4 bias, ga, be, rv, rmean, rvar; };
__device__ __forceinline__ FwdPre fwd_prefetch(const FwdArgs& p, int c) {
  const int tid = threadIdx.x, r = tid >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  FwdPre q = {zero, zero, zero, zero, zero, zero};
  if (tid < 256) {
    q.bias = ld4(p.bias + c);
    if (!p.stats) { q.ga = ld4(p.gamma + c); q.be = ld4(p.beta + c); }
    if (p.resid && r < p.B) q.rv = ld4(p.resid + (size_t)r * p.H + c);
    if (p.eval) { q.rmean = ld4(p.rm + c); q.rvar = ld4(p.rv + c); }
  }
  return q;
}
// the evaluation tail: y = relu(z s + t) (+ residual) with s = gamma / sqrt(running_var + eps), t = (bias - running_mean) s +
// beta -- bn_fold_eval_kernel's fold and the GEMM epilogue's order (batchnorm.hip, gemm_epilogue.h)
__device__ __forceinline__ float4 eval_tail(const FwdArgs& p, float4 z, const FwdPre& q, int c) {
  const int tid = threadIdx.x, r = tid >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid >= 256 || r >= p.B) return zero;
  const float sx = q.ga.x * (1.0f / sqrtf(q.rvar.x + p.eps)), sy = q.ga.y * (1.0f / sqrtf(q.rvar.y + p.eps));
  const float sz = q.ga.z * (1.0f / sqrtf(q.rvar.z + p.eps)), sw = q.ga.w * (1.0f / sqrtf(q.rvar.w + p.eps));
  float4 y;
  y.x = relu_f(fmaf(z.x, sx, fmaf(q.bias.x - q.rmean.x, sx, q.be.x))) + q.rv.x;
  y.y = relu_f(fmaf(z.y, sy, fmaf(q.bias.y - q.rmean.y, sy, q.be.y))) + q.rv.y;
  y.z = relu_f(fmaf(z.z, sz, fmaf(q.bias.z - q.rmean.z, sz, q.be.z))) + q.rv.z;
  y.w = relu_f(fmaf(z.w, sw, fmaf(q.bias.w - q.rmean.w, sw, q.be.w))) + q.rv.w;
  st4(p.act + (size_t)r * p.H + c, y);
  if (p.outp) store_planes4(PlaneDst{p.outp, p.outp + p.o_plane, kActPlaneScale, 2, 0, p.range, p.site}, (size_t)r * p.H + c, y);
  return y;
}
// Returns the thread's four outputs (zeros outside the batch and for threads >= 256).
__device__ __forceinline__ float4 fwd_tail(const FwdArgs& p, float4 z, const FwdPre& pre, int blk, int c, float4 (*sm)[4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 2;
  const bool live = tid < 256 && r < p.B;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 ga = pre.ga, be = pre.be, rv = pre.rv;
  z.x += pre.bias.x; z.y += pre.bias.y; z.z += pre.bias.z; z.w += pre.bias.w;
  if (!live) z = zero;
  if (live) st4(p.z + (size_t)r * p.H + c, z);
  const float Bt = (float)p.B;
  float4 s[1] = {z};
  colsum<1>(s, sm);
  const float4 mean = make_float4(s[0].x / Bt, s[0].y / Bt, s[0].z / Bt, s[0].w / Bt);
  float4 q[1] = {zero};
  if (live) {
    const float dx = z.x - mean.x, dy = z.y - mean.y, dz = z.z - mean.z, dw = z.w - mean.w;
    q[0] = make_float4(dx * dx, dy * dy, dz * dz, dw * dw);
  }
  colsum<1>(q, sm);
  if (tid >= 256) return zero;
  const float var[4] = {q[0].x / Bt, q[0].y / Bt, q[0].z / Bt, q[0].w / Bt};
  const float mu[4] = {mean.x, mean.y, mean.z, mean.w};
  const float g4[4] = {ga.x, ga.y, ga.z, ga.w}, b4[4] = {be.x, be.y, be.z, be.w};
  float rs[4], sc[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rs[j] = 1.0f / sqrtf(var[j] + p.eps);
    sc[j] = g4[j] * rs[j];
    sh[j] = bn_shift_of(b4[j], mu[j], sc[j]);
  }
  if (tid < 4) {
    st4(p.mean + c, mean);
    st4(p.rstd + c, make_float4(rs[0], rs[1], rs[2], rs[3]));
    if (p.rm) {
      float4 m = ld4(p.rm + c), v = ld4(p.rv + c);
      bn_running_update(m.x, v.x, mu[0], var[0], Bt, p.momentum);
      bn_running_update(m.y, v.y, mu[1], var[1], Bt, p.momentum);
      bn_running_update(m.z, v.z, mu[2], var[2], Bt, p.momentum);
      bn_running_update(m.w, v.w, mu[3], var[3], Bt, p.momentum);
      st4(p.rm + c, m); st4(p.rv + c, v);
    }
  }
  if (p.nbt && blockIdx.x == 0 && tid == 0) p.nbt[0] += 1;
  // ReLU, dropout, bitmap, residual (element order of bn_apply_row, batchnorm.hip)
  uint32_t c3 = p.c3, k1 = p.k1;
  dropout_replay_step(c3, k1, p.seed_hi, p.step_dev);
  const int mode = p.mode & 7;
  const bool norelu = (p.mode & 8) != 0;
  const float zv[4] = {z.x, z.y, z.z, z.w};
  float y[4];
  bool keep[4] = {true, true, true, true};
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = fmaf(zv[j], sc[j], sh[j]);
  if (live) {
    if (mode == 1) {
      const uint64_t g = ((uint64_t)r * (uint64_t)p.H + (uint64_t)c) >> 2;
      const Philox4 u = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), p.layer, c3, p.k0, k1);
#pragma unroll
      for (int j = 0; j < 4; ++j) keep[j] = u.v[j] >= p.thr;
    } else if (mode == 2) {
      const int wpr = (((p.H + 255) >> 8) * 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) keep[j] = (p.inject[(size_t)r * wpr + (c >> 8) * 4 + j] >> ((c >> 2) & 63)) & 1ull;
    } else if (mode == 3) {
#pragma unroll
      for (int j = 0; j < 4; ++j) keep[j] = false;
    }
  }
  float o[4];
  uint64_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool on = live && keep[j] && (norelu || relu_on(y[j]));
    o[j] = on ? y[j] * p.kscale : 0.f;
    const uint64_t bal = __ballot(on);
    if (lane == j) word = bal;
  }
  if (lane < 4) p.bits[(size_t)blk * 16 + wave * 4 + lane] = word;
  const float4 out = make_float4(o[0] + rv.x, o[1] + rv.y, o[2] + rv.z, o[3] + rv.w);
  if (live) {
    st4(p.act + (size_t)r * p.H + c, out);
    if (p.outp) store_planes4(PlaneDst{p.outp, p.outp + p.o_plane, kActPlaneScale, 2, 0, p.range, p.site}, (size_t)r * p.H + c, out);
  }
  return live ? out : zero;
}

// the workgroup's slab of the output Linear (FwdArgs.ypart): hs = the act tile [64][16] from the threads' registers, ws = the
// 16 columns of W2 [O][17] (odd stride: lanes walk o); thread t handles (row idx >> 6, output idx & 63), an fmaf chain over the
// 16 columns in order.  Every thread of the workgroup calls it.
__device__ __forceinline__ void head_slab(const FwdArgs& p, float4 out, int blk, int c0, float* hs, float* ws) {
  const int tid = threadIdx.x;
  if (tid < 256) st4(hs + tid * 4, out);
  {
    float v[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = min(tid + u * NTHR, p.O * COLS - 1);
      v[u] = p.W2[(size_t)(idx >> 4) * p.H + c0 + (idx & 15)];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + u * NTHR;
      if (idx < p.O * COLS) ws[(idx >> 4) * 17 + (idx & 15)] = v[u];
    }
  }
  __syncthreads();
  float* mine = p.ypart + (size_t)blk * p.Mtot * 64;
  for (int idx = tid; idx < p.B * 64; idx += NTHR) {
    const int r = idx >> 6, o = idx & 63;
    if (o >= p.O) continue;
    float acc = 0.f;
#pragma unroll
    for (int cc = 0; cc < COLS; ++cc) acc = fmaf(hs[r * COLS + cc], ws[o * 17 + cc], acc);
    mine[idx] = acc;
  }
}

// the tail of the Linear-alone form: z (+ bias) stored, the group's partial statistics (every thread of the workgroup calls it)
__device__ __forceinline__ void stats_tail(const FwdArgs& p, float4 z, const FwdPre& pre, int c, float4 (*sm)[4]) {
  const int tid = threadIdx.x, r = tid >> 2;
  const bool live = tid < 256 && r < p.B;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  z.x += pre.bias.x; z.y += pre.bias.y; z.z += pre.bias.z; z.w += pre.bias.w;
  if (!live) z = zero;
  if (live) st4(p.z + (size_t)r * p.H + c, z);
  if (!p.stat_sum) return;                                   // (kernel-uniform)
  float4 s[1] = {z};
  colsum<1>(s, sm);
  const float cnt = (float)p.B;
  float4 q[1] = {zero};
  if (live) {
    const float dx = z.x - s[0].x / cnt, dy = z.y - s[0].y / cnt, dz = z.z - s[0].z / cnt, dw = z.w - s[0].w / cnt;
    q[0] = make_float4(dx * dx, dy * dy, dz * dz, dw * dw);
  }
  colsum<1>(q, sm);
  if (tid < 4) {
    st4(p.stat_sum + (size_t)blockIdx.y * p.H + c, s[0]);
    st4(p.stat_m2 + (size_t)blockIdx.y * p.H + c, q[0]);
  }
}

template <int STEPS>
__global__ __launch_bounds__(NTHR) void small_fwd_kernel(FwdArgs p_in) {
  __shared__ float part[NWAVE * ROWS * COLS];
  __shared__ float stage[NWAVE * STAGE];
  __shared__ float4 sm[4][4];
  const FwdArgs p = row_block(p_in);
  const int blk = col_block(blockIdx.x, gridDim.x);
  const int c0 = blk * COLS;
  const int tid = threadIdx.x;
  const int c = c0 + 4 * (tid & 3);
  if (p.stats && p.B <= 0) {                                 // a statistics group past the last row: zeros (workgroup-uniform)
    if (p.stat_sum && tid < 4) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      st4(p.stat_sum + (size_t)blockIdx.y * p.H + c, zero);
      st4(p.stat_m2 + (size_t)blockIdx.y * p.H + c, zero);
    }
    return;
  }
  const FwdPre pre = fwd_prefetch(p, c);
  if (p.ap)
    contract_f16<STEPS>(p.ap, p.a_plane, p.K, p.B, p.W, p.K, c0, kWeightPlaneScale, 1.0f / (kActPlaneScale * kWeightPlaneScale), part,
                        stage, p.range);
  else contract<STEPS, false>(p.a, p.K, p.B, p.W, p.K, c0, part, stage);
  __syncthreads();
  float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < 256) z = gather_part(part);
  if (p.stats) { stats_tail(p, z, pre, c, sm); return; }
  const float4 out = p.eval ? eval_tail(p, z, pre, c) : fwd_tail(p, z, pre, blk, c, sm);
  if (p.ypart) {
    if (p.eval) __syncthreads();                             // (every thread is done with part)
    head_slab(p, out, blk, c0, part, stage);                 // (part and stage are free behind the barriers of fwd_tail)
  }
}

// The FIRST hidden layer (LinearModel.w1: in_dim = 34 or 51 inputs, baselineModel.py:76,90-94): the contraction is 34 steps,
// so x (all rows) and the workgroup's 16 rows of W1 sit in LDS and a thread forms its four outputs on the vector unit (an fmaf
// chain over k in index order); the tail is the other layers'.  K <= kFirstMaxK.
constexpr int kFirstMaxK = 256;                        // (64 + 16) rows of K floats in the stage array
__global__ __launch_bounds__(NTHR) void small_first_fwd_kernel(FwdArgs p_in) {
  __shared__ float stage[NWAVE * STAGE];
  __shared__ float4 sm[4][4];
  const FwdArgs p = row_block(p_in);
  static_assert((ROWS + COLS) * kFirstMaxK <= NWAVE * STAGE, "stage array");
  const int blk = col_block(blockIdx.x, gridDim.x);
  const int c0 = blk * COLS;
  const int tid = threadIdx.x, K = p.K;
  const FwdPre pre = fwd_prefetch(p, c0 + 4 * (tid & 3));
  float* xs = stage;
  float* ws = stage + ROWS * K;
  {
    const float* __restrict__ xa = p.a;
    const float* __restrict__ wa = p.W + (size_t)c0 * K;
    const int nx = p.B * K;
    fill_lds<8>(xs, ROWS * K, [&](int idx) { return idx < nx ? xa[idx] : 0.f; });
    fill_lds<2>(ws, COLS * K, [&](int idx) { return wa[idx]; });
  }
  __syncthreads();
  const int c = c0 + 4 * (tid & 3);
  float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < 256) {
    const float* xr = xs + (tid >> 2) * K;
    const float* w0 = ws + 4 * (tid & 3) * K;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < K; ++k) {
      const float xv = xr[k];
      a0 = fmaf(xv, w0[k], a0); a1 = fmaf(xv, w0[K + k], a1); a2 = fmaf(xv, w0[2 * K + k], a2); a3 = fmaf(xv, w0[3 * K + k], a3);
    }
    z = make_float4(a0, a1, a2, a3);
  }
  const float4 out = p.eval ? eval_tail(p, z, pre, c) : fwd_tail(p, z, pre, blk, c, sm);
  if (p.ypart) {                                             // (num_stage = 0: the first layer is the last)
    if (p.eval) __syncthreads();                             // (every thread is done with xs / ws)
    head_slab(p, out, blk, c0, stage, stage + ROWS * COLS);
  }
}

// The weight gradient of the same layer rides in the backward launch as extra workgroups (it needs dz and the layer's input,
// both complete when the launch starts): dW [N][Kin] = dz^T a over the B <= 64 rows, one 128 x 64 tile per workgroup; wave w
// owns rows 32 (w & 3) .. + 31 and columns 32 (w >> 2) .. + 31 of the tile: 2 x 2 MFMA tiles, sixteen 4-row steps.
__device__ __forceinline__ void dw_tile(const float* __restrict__ dz, const float* __restrict__ a, float* __restrict__ dW, int B,
                                        int N, int Kin, int tile) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int tpr = Kin >> 6;                              // tiles per row of tiles
  const int n0 = (tile / tpr) * 128 + 32 * (wave & 3), k0 = (tile % tpr) * 64 + 32 * (wave >> 2);
  float av[16][2], bv[16][2];
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const int r = 4 * st + kq;
    const int rc = min(r, B - 1);
    const float* pa = dz + (size_t)rc * N + n0 + i;
    const float* pb = a + (size_t)rc * Kin + k0 + i;
    av[st][0] = pa[0]; av[st][1] = pa[16];
    bv[st][0] = pb[0]; bv[st][1] = pb[16];
    if (r >= B) av[st][0] = av[st][1] = 0.f;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < 16; ++st)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[st][x], bv[st][y], acc[x][y], 0, 0, 0);
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int v = 0; v < 4; ++v) dW[(size_t)(n0 + 16 * x + 4 * kq + v) * Kin + k0 + 16 * y + i] = acc[x][y][v];
}

// BatchNorm backward of one layer on the workgroup's columns, from the layer's incoming gradient g (thread tid < 256: row
// tid >> 2, columns c .. c + 3 of block blk): sum dy, sum dy zhat, the coefficients, dz (stored, and returned: zeros outside the
// batch), dgamma, dbeta and the gradient of the bias in front of the BatchNorm.  Every thread of the workgroup calls it.
struct BnLo {
  const float *z, *mean, *rstd, *gamma;
  const uint64_t* bits;
  float *dz, *dgamma, *dbeta, *dbias;
  float kscale;
  int B, H, rowbits;                      // rowbits: the bitmap is in the row format of bn_apply_row (batchnorm.hip)
};
// what the tail reads from memory besides g: requested before the contraction that produces g
struct BnPre { float4 zl, mu, rs, ga; uint64_t bw[4]; int bit; };
__device__ __forceinline__ BnPre bn_prefetch(const BnLo& p, int blk, int c) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = tid >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  BnPre q = {zero, zero, zero, zero, {0, 0, 0, 0}, lane};
  if (tid < 256) {
    q.mu = ld4(p.mean + c); q.rs = ld4(p.rstd + c); q.ga = ld4(p.gamma + c);
    if (r < p.B) {
      q.zl = ld4(p.z + (size_t)r * p.H + c);
      const uint64_t* w = p.bits + (size_t)blk * 16 + wave * 4;
      if (p.rowbits) {
        w = p.bits + (size_t)r * (((p.H + 255) >> 8) * 4) + (c >> 8) * 4;
        q.bit = (c >> 2) & 63;
      }
      const ulonglong2 b01 = *reinterpret_cast<const ulonglong2*>(w), b23 = *reinterpret_cast<const ulonglong2*>(w + 2);
      q.bw[0] = b01.x; q.bw[1] = b01.y; q.bw[2] = b23.x; q.bw[3] = b23.y;
    }
  }
  return q;
}
__device__ __forceinline__ float4 bnbwd_tail(const BnLo& p, float4 g, const BnPre& pre, int blk, int c, float4 (*sm)[4]) {
  const int tid = threadIdx.x;
  const int r = tid >> 2;
  const bool live = tid < 256 && r < p.B;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 zl = pre.zl, mu = pre.mu, rs = pre.rs, ga = pre.ga;
  const uint64_t bw[4] = {pre.bw[0], pre.bw[1], pre.bw[2], pre.bw[3]};
  const int bit = pre.bit;
  float4 dv = zero, zh = zero;
  if (live) {
    dv.x = ((bw[0] >> bit) & 1ull) ? g.x * p.kscale : 0.f;
    dv.y = ((bw[1] >> bit) & 1ull) ? g.y * p.kscale : 0.f;
    dv.z = ((bw[2] >> bit) & 1ull) ? g.z * p.kscale : 0.f;
    dv.w = ((bw[3] >> bit) & 1ull) ? g.w * p.kscale : 0.f;
    zh = make_float4((zl.x - mu.x) * rs.x, (zl.y - mu.y) * rs.y, (zl.z - mu.z) * rs.z, (zl.w - mu.w) * rs.w);
  }
  float4 s[3];
  s[0] = dv;
  s[1] = make_float4(dv.x * zh.x, dv.y * zh.y, dv.z * zh.z, dv.w * zh.w);
  s[2] = zh;
  colsum<3>(s, sm);
  const float Bt = (float)p.B;
  const float4 s1 = s[0], s2 = s[1], sz = s[2];
  const float4 k0 = make_float4(ga.x * rs.x, ga.y * rs.y, ga.z * rs.z, ga.w * rs.w);
  const float4 k1 = make_float4(s1.x / Bt, s1.y / Bt, s1.z / Bt, s1.w / Bt);
  const float4 k2 = make_float4(s2.x / Bt, s2.y / Bt, s2.z / Bt, s2.w / Bt);
  if (tid < 4) {
    st4(p.dgamma + c, s2); st4(p.dbeta + c, s1);
    // (the bias in front of BatchNorm: true gradient 0; formed from the three sums as in bn_small_bwd_kernel)
    float4 db;
    db.x = k0.x * ((s1.x - Bt * k1.x) - k2.x * sz.x); db.y = k0.y * ((s1.y - Bt * k1.y) - k2.y * sz.y);
    db.z = k0.z * ((s1.z - Bt * k1.z) - k2.z * sz.z); db.w = k0.w * ((s1.w - Bt * k1.w) - k2.w * sz.w);
    st4(p.dbias + c, db);
  }
  float4 d = zero;
  if (live) {
    d.x = k0.x * (dv.x - k1.x - zh.x * k2.x); d.y = k0.y * (dv.y - k1.y - zh.y * k2.y);
    d.z = k0.z * (dv.z - k1.z - zh.z * k2.z); d.w = k0.w * (dv.w - k1.w - zh.w * k2.w);
    st4(p.dz + (size_t)r * p.H + c, d);
  }
  return d;
}

struct BwdArgs {
  const float *a_in;                      // the layer's input [B][H] and
  float* dW;                              //   its weight gradient [K][H] = dz^T a_in (extra workgroups), or NULL
  int nblk_dx;                            // workgroups of the dX part (H / 16)
  const float *dz, *W, *addend;           // g = dz W (+ addend) on the workgroup's columns
  float* gout;                            // g is kept here when something later reads it (the skip gradient), or NULL
  BnLo lo;                                // the layer below
  // the layer below is the FIRST layer: its weight gradient dW1 [H][K1] = dz_lo^T x follows in the same workgroup, or NULL
  const float* x1;
  float* dW1;
  int K1;
  int B, H, K;
  // a slice of the AdamW step (parameters whose gradients earlier launches finished and which nothing reads any more) on
  // nblk_adam further workgroups behind the weight-gradient ones: HBM streaming beside the latency-bound layer work
  AdamWRide adam;
  int nblk_dw, nblk_adam;
};

// dW [16 columns of this workgroup][K1] = d^T x over the rows: d (this workgroup's dz of the first layer, from the threads'
// registers) and x through LDS; thread o handles (column o / K1, input o % K1), an fmaf chain over the rows in order
__device__ __forceinline__ void first_wgrad(float4 d, const float* __restrict__ x, float* __restrict__ dW1, int B, int K1, int c0,
                                            float* ds, float* xs) {
  const int tid = threadIdx.x;
  if (tid < 256) st4(ds + tid * 4, d);                   // [row][16]
  fill_lds<8>(xs, B * K1, [&](int idx) { return x[idx]; });
  __syncthreads();
  for (int o = tid; o < COLS * K1; o += NTHR) {
    const int cc = o / K1, k = o - cc * K1;
    float acc = 0.f;
    for (int r = 0; r < B; ++r) acc = fmaf(ds[r * COLS + cc], xs[r * K1 + k], acc);
    dW1[(size_t)(c0 + cc) * K1 + k] = acc;
  }
}

// EMA: the AdamW slice's workgroups keep the averaged weights too (PLEma, adamw.h); EMA = false takes an empty EmaArg and is
// the kernel as it was.
template <int STEPS, bool EMA>
__global__ __launch_bounds__(NTHR) void small_bwd_kernel(BwdArgs p, EmaArg<EMA> ema) {
  __shared__ float part[NWAVE * ROWS * COLS];
  __shared__ float stage[NWAVE * STAGE];
  __shared__ float4 sm[12][4];
  if ((int)blockIdx.x >= p.nblk_dx + p.nblk_dw) {       // (workgroup-uniform)
    const AdamWK k = adamw_consts(p.adam);
    if constexpr (EMA)
      adamw_span<true>(p.adam.p, p.adam.g, p.adam.m, p.adam.v, p.adam.n >> 2,
                       (int64_t)(blockIdx.x - p.nblk_dx - p.nblk_dw) * NTHR + threadIdx.x, (int64_t)p.nblk_adam * NTHR, k,
                       ema.v.e, ema_omd(p.adam, nullptr, ema.v));
    else
      adamw_span(p.adam.p, p.adam.g, p.adam.m, p.adam.v, p.adam.n >> 2,
                 (int64_t)(blockIdx.x - p.nblk_dx - p.nblk_dw) * NTHR + threadIdx.x, (int64_t)p.nblk_adam * NTHR, k);
    return;
  }
  if ((int)blockIdx.x >= p.nblk_dx) {
    dw_tile(p.dz, p.a_in, p.dW, p.B, p.K, p.H, blockIdx.x - p.nblk_dx);
    return;
  }
  const int blk = col_block(blockIdx.x, p.nblk_dx);
  const int c0 = blk * COLS;
  const int tid = threadIdx.x;
  const int r = tid >> 2, c = c0 + 4 * (tid & 3);
  const bool live = tid < 256 && r < p.B;
  const BnPre pre = bn_prefetch(p.lo, blk, c);
  float4 add = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p.addend && live) add = ld4(p.addend + (size_t)r * p.H + c);
  contract<STEPS, true>(p.dz, p.K, p.B, p.W, p.H, c0, part, stage);
  __syncthreads();
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < 256) {
    g = gather_part(part);
    g.x += add.x; g.y += add.y; g.z += add.z; g.w += add.w;
    if (p.gout && live) st4(p.gout + (size_t)r * p.H + c, g);
  }
  const float4 d = bnbwd_tail(p.lo, g, pre, blk, c, sm);
  // (part and stage are free: every thread is past the barriers of bnbwd_tail)
  if (p.dW1) first_wgrad(d, p.x1, p.dW1, p.B, p.K1, c0, part, stage);
}

// The TOP of the backward pass: the output Linear (LinearModel.w2, out_dim = 51 or 34 outputs) and the BatchNorm backward of
// the last hidden layer, from dy [B][O]:  g = dy W2 on the workgroup's 16 columns (O steps on the vector unit, dy and the W2
// columns in LDS; kept in gout: it is also the skip gradient of the last residual block), the BatchNorm backward of the top
// layer, dW2[:, columns] = dy^T h, and -- workgroup 0 -- the output bias gradient = column sums of dy.   O <= 64.
struct TopArgs {
  const float *dy, *W2, *h;
  float *gout, *dW2, *db2;
  BnLo lo;
  int B, H, O;
  // the fused train step: the MSE loss = inv_n * (sum of the np partials, in order), and the device step counter ticks here
  // (every dropout kernel of the forward ran before this launch, AdamW runs after it) -- mse_final_kernel's job
  const float* mpart;
  float* loss;
  uint64_t* tick;
  float inv_n;
  int np;
};
__global__ __launch_bounds__(NTHR) void small_top_bwd_kernel(TopArgs p) {
  __shared__ float stage[ROWS * 64 + 64 * COLS + ROWS * COLS];
  __shared__ float4 sm[12][4];
  const int blk = col_block(blockIdx.x, gridDim.x);
  const int c0 = blk * COLS;
  const int tid = threadIdx.x, O = p.O;
  const BnPre pre = bn_prefetch(p.lo, blk, c0 + 4 * (tid & 3));
  float* dys = stage;                    // [64][O]
  float* ws = stage + ROWS * 64;         // [O][16]
  float* hs = ws + 64 * COLS;            // [64][16]
  {
    // (everything the workgroup stages is requested before the first LDS store: 8 + 2 + 2 loads per thread, one round trip)
    const int nd = p.B * O;
    float vd[8], vw[2], vh[2];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + u * NTHR;
      vd[u] = idx < nd ? p.dy[idx] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int iw = min(tid + u * NTHR, O * COLS - 1), ih = tid + u * NTHR;
      vw[u] = p.W2[(size_t)(iw >> 4) * p.H + c0 + (iw & 15)];
      vh[u] = (ih >> 4) < p.B ? p.h[(size_t)(ih >> 4) * p.H + c0 + (ih & 15)] : 0.f;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int idx = tid + u * NTHR;
      if (idx < ROWS * O) dys[idx] = vd[u];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + u * NTHR;
      if (idx < O * COLS) ws[idx] = vw[u];
      hs[idx] = vh[u];
    }
  }
  __syncthreads();
  const int r = tid >> 2, c = c0 + 4 * (tid & 3);
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < 256) {
    const float* dr = dys + r * O;
    const float* w0 = ws + 4 * (tid & 3);
    for (int o = 0; o < O; ++o) {
      const float dv = dr[o];
      const float4 wv = ld4(w0 + o * COLS);
      g.x = fmaf(dv, wv.x, g.x); g.y = fmaf(dv, wv.y, g.y); g.z = fmaf(dv, wv.z, g.z); g.w = fmaf(dv, wv.w, g.w);
    }
    if (r < p.B) st4(p.gout + (size_t)r * p.H + c, g);
  } else {
    // (waves 4-7 have no element of the tail: the weight-gradient columns are theirs, beside the g loop of waves 0-3)
    for (int o = tid - 256; o < O * COLS; o += 256) {
      const int oo = o >> 4, cc = o & 15;
      float acc = 0.f;
      for (int rr = 0; rr < p.B; ++rr) acc = fmaf(dys[rr * O + oo], hs[rr * COLS + cc], acc);
      p.dW2[(size_t)oo * p.H + c0 + cc] = acc;
    }
  }
  (void)bnbwd_tail(p.lo, g, pre, blk, c, sm);
  if (blockIdx.x == 0 && tid < O) {
    float acc = 0.f;
    for (int rr = 0; rr < p.B; ++rr) acc += dys[rr * O + tid];
    p.db2[tid] = acc;
  }
  if (p.loss && blockIdx.x == 0 && tid == 64) {
    float acc = 0.f;
    for (int i = 0; i < p.np; ++i) acc += p.mpart[i];
    p.loss[0] = acc * p.inv_n;
    if (p.tick) p.tick[0] += 1;
  }
}

// y = bias + the NS slabs of the output Linear (FwdArgs.ypart: [NS][B][64]), dpred = coef (y - t), and per workgroup the
// partial sum of (y - t)^2: the MSE forward + backward of the fused train step at small batch (nn.MSELoss, train_1.py:64-66).
// Four lanes per element, a quarter of the slabs each (all of a lane's loads in flight: one round trip), combined in a fixed
// order: (q0 + q1) + (q2 + q3).  64 elements per workgroup.
// C, W (pose_criterion.h): the criterion in MSE's place and its weights (one element, one weight per lane group; kWRow:
// k.rw[i / G], loaded by lane 0 of the group in front of the slab loads); <Pointwise<PL_CRIT_MSE>, kWNone> is the kernel as
// it always was.
constexpr int kMseElems = 64;
template <class C, int W>
__global__ __launch_bounds__(256) void small_mse_kernel(const float* __restrict__ ypart, int NS, int B, int O,
                                                        const float* __restrict__ bias, const float* __restrict__ tgt, CritK k,
                                                        float* __restrict__ y, float* __restrict__ dpred, float* __restrict__ mpart) {
  __shared__ float red[4];
  const int n = B * O, tid = threadIdx.x;
  const int i = blockIdx.x * kMseElems + (tid >> 2), q = tid & 3;
  const bool ok = i < n;
  const int r = ok ? i / O : 0, o = ok ? i - r * O : 0;
  const size_t slab = (size_t)B * 64;
  const int per = (NS + 3) >> 2;
  const float* src = ypart + (size_t)r * 64 + o + (size_t)(q * per) * slab;
  float rwv = 0.f, wjv = 0.f;                                // (kWRow: loads only here; their product where it is used)
  if constexpr (W == kWRow) {
    if (ok && q == 0 && tgt) { rwv = k.rw[i / k.G]; wjv = joint_weight_or_one(k, o / k.G); }
  }
  float a = 0.f;
  for (int s0 = 0; s0 < per; s0 += 16) {
    float u[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) u[j] = (ok && s0 + j < per && q * per + s0 + j < NS) ? src[(size_t)(s0 + j) * slab] : 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) a += u[j];
  }
  a += __shfl_xor(a, 1);
  a += __shfl_xor(a, 2);
  float acc = 0.f;
  if (ok && q == 0) {
    if (bias) a += bias[o];
    y[i] = a;
    if (tgt) {
      const float d = a - tgt[i];
      if constexpr (W == kWRow) {
        const float w = wjv * rwv;
        acc = C::add_w(0.f, d, w, k);
        dpred[i] = C::grad(d, k) * w;
      } else if constexpr (W == kWJoint) {
        const float w = k.w[o / k.G];
        acc = C::add_w(0.f, d, w, k);
        dpred[i] = C::grad(d, k) * w;
      } else {
        acc = C::first(d, k);
        dpred[i] = C::grad(d, k);
      }
    }
  }
  if (!tgt) return;                                          // (evaluation: y is all there is; kernel-uniform)
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) acc += __shfl_xor(acc, w);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) mpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The grouped kind (mpjpe) with an element map of its own: four lanes per JOINT, 64 joints per workgroup (no joint is shared
// between workgroups).  Each lane sums a quarter of the slabs of all G coordinates -- G x 16 loads in flight per pass, one round
// trip -- and the quarters combine per coordinate in small_mse_kernel's order, (q0 + q1) + (q2 + q3), + bias: y has the bits
// the pointwise map gives it.  Lane 0 of the group then holds the whole joint.  ceil(B J / 64) <= 64 partials.
template <int G, int W>
__global__ __launch_bounds__(256) void small_mpjpe_kernel(const float* __restrict__ ypart, int NS, int B, int O,
                                                          const float* __restrict__ bias, const float* __restrict__ tgt, CritK k,
                                                          float* __restrict__ y, float* __restrict__ dpred, float* __restrict__ mpart) {
  __shared__ float red[4];
  const int J = O / G, nj = B * J, tid = threadIdx.x;
  const int i = blockIdx.x * kMseElems + (tid >> 2), q = tid & 3;
  const bool ok = i < nj;
  const int r = ok ? i / J : 0, j = ok ? i - r * J : 0;
  const size_t slab = (size_t)B * 64;
  const int per = (NS + 3) >> 2;
  const float* src = ypart + (size_t)r * 64 + j * G + (size_t)(q * per) * slab;
  float rwv = 0.f, wjv = 0.f;                                // (kWRow: the joint's weights, loaded in front of the slab loads)
  if constexpr (W == kWRow) {
    if (ok && q == 0) { rwv = k.rw[i]; wjv = joint_weight_or_one(k, j); }
  }
  float a[G];
#pragma unroll
  for (int c = 0; c < G; ++c) a[c] = 0.f;
  for (int s0 = 0; s0 < per; s0 += 16) {
    float u[G][16];
#pragma unroll
    for (int c = 0; c < G; ++c)
#pragma unroll
      for (int m = 0; m < 16; ++m) u[c][m] = (ok && s0 + m < per && q * per + s0 + m < NS) ? src[(size_t)(s0 + m) * slab + c] : 0.f;
#pragma unroll
    for (int c = 0; c < G; ++c)
#pragma unroll
      for (int m = 0; m < 16; ++m) a[c] += u[c][m];
  }
#pragma unroll
  for (int c = 0; c < G; ++c) {
    a[c] += __shfl_xor(a[c], 1);
    a[c] += __shfl_xor(a[c], 2);
  }
  float acc = 0.f;
  if (ok && q == 0) {
    float d[G], g[G];
#pragma unroll
    for (int c = 0; c < G; ++c) {
      if (bias) a[c] += bias[j * G + c];
      y[i * G + c] = a[c];
      d[c] = a[c] - tgt[i * G + c];
    }
    float w;
    if constexpr (W == kWRow) w = wjv * rwv;
    else w = W ? k.w[j] : 1.f;
    const float nr = joint_norm_grad<G>(d, W ? k.coef * w : k.coef, g);
    acc = W ? w * nr : nr;
#pragma unroll
    for (int c = 0; c < G; ++c) dpred[i * G + c] = g[c];
  }
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) acc += __shfl_xor(acc, w);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) mpart[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

inline bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// workgroups of the AdamW slice a backward launch carries: ~2 K float4 per workgroup pass, 1 M parameters on 64 workgroups
constexpr int kSmallAdamBlocks = 64;

}  // namespace

// shapes the layer kernels take: B rows in one tile, 16-column blocks, K split over eight waves in 32-k steps
bool small_layer_ok(int B, int H, int K) {
  if (B < 2 || B > ROWS || (H & 15) || H < 16) return false;
  const int steps = K / (NWAVE * 32);
  return K % (NWAVE * 32) == 0 && (steps == 1 || steps == 2 || steps == 4);
}
// ... and the first layer (K = in_dim inputs) / the output layer (O = out_dim outputs) beside such hidden layers
bool small_first_ok(int K) {
  return K >= 1 && K <= kFirstMaxK;
}
bool small_top_ok(int O) {
  return O >= 1 && O <= 64;
}

// the output Linear of an evaluation forward from the slabs the last hidden layer's launch left: y = bias + sum of slabs
int launch_small_out(const SmallHeadArgs& a, hipStream_t s) {
  if (!a.ypart || !a.y || a.NS < 1 || a.B < 1 || !small_top_ok(a.O)) PL_FAIL(PL_EINVAL, "small_out: bad arguments");
  hipLaunchKernelGGL((small_mse_kernel<Pointwise<PL_CRIT_MSE>, kWNone>), dim3((a.B * a.O + kMseElems - 1) / kMseElems), dim3(256), 0,
                     s, a.ypart, a.NS, a.B, a.O, a.bias, (const float*)nullptr, CritK{}, a.y, (float*)nullptr, (float*)nullptr);
  PL_CHECK_LAUNCH("small_out");
  return PL_OK;
}

namespace {
// what launch_small_layer_fwd / _eval share: the kernel's arguments from the fields both read (rows: all rows of the
// launch), and the launch itself (grid.y = row_blocks 64-row blocks)
int fill_layer_fwd(FwdArgs& p, const SmallLayerFwdArgs& a, int rows, const char* who) {
  p.a = a.a; p.W = a.W; p.bias = a.bias; p.resid = a.resid; p.act = a.act;
  p.gamma = a.bn.gamma; p.beta = a.bn.beta; p.eps = a.bn.eps; p.rm = a.bn.running_mean; p.rv = a.bn.running_var;
  p.H = a.H; p.K = a.K;
  if (a.ypart) {
    if (!a.W2 || !small_top_ok(a.O)) PL_FAIL(PL_EINVAL, "%s: output-layer slabs (O=%d)", who, a.O);
    p.W2 = a.W2; p.ypart = a.ypart; p.O = a.O;
  }
  if ((a.a_planes && (a.first || !al16(a.a_planes))) || !al16(a.out_planes)) PL_FAIL(PL_EINVAL, "%s: operand planes", who);
  p.ap = a.a_planes; p.a_plane = (size_t)rows * a.K; p.outp = a.out_planes; p.o_plane = (size_t)rows * a.H;
  p.range = range_record(); p.site = range_site_act(a.layer);
  return PL_OK;
}
int run_layer_fwd(const FwdArgs& p, bool first, int rows, int row_blocks, const char* who, hipStream_t s) {
  const dim3 grid(p.H / COLS, row_blocks), block(NTHR);
  void* prof = prof_begin_flops(2.0 * rows * p.H * p.K, s);
  if (first) hipLaunchKernelGGL(small_first_fwd_kernel, grid, block, 0, s, p);
  else switch (p.K / (NWAVE * 32)) {
    case 1: hipLaunchKernelGGL(small_fwd_kernel<1>, grid, block, 0, s, p); break;
    case 2: hipLaunchKernelGGL(small_fwd_kernel<2>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(small_fwd_kernel<4>, grid, block, 0, s, p); break;
  }
  prof_end(prof, s);
  PL_CHECK_LAUNCH(who);
  return PL_OK;
}
}  // namespace

// hidden layer l of an evaluation forward of a.B rows (any number: the grid runs over 64-row blocks): act = relu(bn_eval(a W^T
// + b)) (+ resid); first: the K-input first layer; ypart != NULL: + the output Linear's slabs [H / 16][B][64]
int launch_small_layer_eval(const SmallLayerFwdArgs& a, hipStream_t s) {
  const int M = a.B;
  if (a.first ? !(small_layer_ok(2, a.H, a.H) && small_first_ok(a.K)) : !small_layer_ok(2, a.H, a.K))
    PL_FAIL(PL_ESHAPE, "small_layer_eval: H=%d K=%d first=%d", a.H, a.K, (int)a.first);
  if (!a.a || !a.W || !a.bias || !a.bn.gamma || !a.bn.beta || !a.bn.running_mean || !a.bn.running_var || !a.act || M < 1)
    PL_FAIL(PL_EINVAL, "small_layer_eval: bad arguments");
  if ((!a.first && (!al16(a.a) || !al16(a.W))) || !al16(a.bias) || !al16(a.bn.gamma) || !al16(a.bn.beta) ||
      !al16(a.bn.running_mean) || !al16(a.bn.running_var) || !al16(a.act) || !al16(a.resid))
    PL_FAIL(PL_EINVAL, "small_layer_eval: 16-byte alignment");
  FwdArgs p = {};
  PL_TRY(fill_layer_fwd(p, a, M, "small_layer_eval"));
  p.B = ROWS; p.eval = 1; p.Mtot = M;
  return run_layer_fwd(p, a.first, M, (M + ROWS - 1) / ROWS, "small_layer_eval", s);
}

// z [M][H] = a W^T + bias for M <= 512 rows (any M; one 64-row block x 16 columns per workgroup) and, stat_sum != NULL, the
// groups partial BatchNorm statistics of a tile GEMM's epilogue ([groups][H] each; groups >= ceil(M / 64): the rest zeros).
// a_planes != NULL: the input as fp16 planes [M][K] (h, l), contraction as three fp16 MFMAs per product; else a fp32, exact.
int launch_small_linear_stats(const SmallLinearStatsArgs& q, hipStream_t s) {
  const int M = q.M, H = q.H, K = q.K;
  if (!small_layer_ok(2, H, K) || M < 1 || q.groups < (M + ROWS - 1) / ROWS)
    PL_FAIL(PL_ESHAPE, "small_linear_stats: M=%d H=%d K=%d groups=%d", M, H, K, q.groups);
  if ((!q.a && !q.a_planes) || !q.W || !q.bias || !q.z || (q.stat_sum != nullptr) != (q.stat_m2 != nullptr))
    PL_FAIL(PL_EINVAL, "small_linear_stats: bad arguments");
  if (!al16(q.a) || !al16(q.a_planes) || !al16(q.W) || !al16(q.bias) || !al16(q.z) || !al16(q.stat_sum) || !al16(q.stat_m2))
    PL_FAIL(PL_EINVAL, "small_linear_stats: 16-byte alignment");
  FwdArgs p = {};
  p.a = q.a; p.W = q.W; p.bias = q.bias; p.z = q.z; p.B = ROWS; p.H = H; p.K = K; p.Mtot = M; p.stats = 1;
  p.stat_sum = q.stat_sum; p.stat_m2 = q.stat_m2;
  p.ap = q.a_planes; p.a_plane = (size_t)M * K; p.range = range_record();
  if (!q.a) p.a = reinterpret_cast<const float*>(q.a_planes);     // (never read: the planes form is taken)
  return run_layer_fwd(p, false, M, q.stat_sum ? q.groups : (M + ROWS - 1) / ROWS, "small_linear_stats", s);
}

int launch_small_layer_fwd(const SmallLayerFwdArgs& a, hipStream_t s) {
  const int B = a.B;
  const BnSaved& sv = a.saved;
  if (a.first ? !(small_layer_ok(B, a.H, a.H) && small_first_ok(a.K)) : !small_layer_ok(B, a.H, a.K))
    PL_FAIL(PL_ESHAPE, "small_layer_fwd: B=%d H=%d K=%d first=%d", B, a.H, a.K, (int)a.first);
  if (!a.a || !a.W || !a.bias || !a.bn.gamma || !a.bn.beta || !sv.mean || !sv.rstd || !sv.z || !a.act || !sv.bits ||
      (a.bn.running_mean != nullptr) != (a.bn.running_var != nullptr))
    PL_FAIL(PL_EINVAL, "small_layer_fwd: bad arguments");
  if ((!a.first && (!al16(a.a) || !al16(a.W))) || !al16(a.bias) || !al16(a.bn.gamma) || !al16(a.bn.beta) || !al16(sv.mean) ||
      !al16(sv.rstd) || !al16(sv.z) || !al16(a.act) || !al16(a.resid) || !al16(a.bn.running_mean) || !al16(a.bn.running_var) ||
      !al16(sv.bits))
    PL_FAIL(PL_EINVAL, "small_layer_fwd: 16-byte alignment");
  FwdArgs p = {};
  PL_TRY(fill_layer_fwd(p, a, B, "small_layer_fwd"));
  const DropKey& k = a.drop;
  p.momentum = a.bn.momentum; p.nbt = a.bn.batches; p.mean = sv.mean; p.rstd = sv.rstd; p.z = sv.z; p.bits = sv.bits; p.B = B;
  p.mode = k.mode; p.thr = k.thr; p.kscale = k.kscale; p.k0 = k.k0; p.k1 = k.k1; p.c3 = k.c3; p.layer = k.layer;
  p.seed_hi = k.seed_hi; p.inject = k.inject; p.step_dev = k.step_dev;
  return run_layer_fwd(p, a.first, B, 1, "small_layer_fwd", s);
}

namespace {
// the BatchNorm backward a launch ends with: every field of the layer checked in this one place
int fill_lo(BnLo& lo, const SmallBnLayer& b, int B, int H, float kscale, float* dz_lo, const char* who) {
  const BnSaved& v = b.saved;
  if (!v.z || !v.bits || !v.mean || !v.rstd || !b.gamma || !dz_lo || !b.dgamma || !b.dbeta || !b.dbias)
    PL_FAIL(PL_EINVAL, "%s: bad arguments (layer below)", who);
  if (!al16(v.z) || !al16(v.bits) || !al16(v.mean) || !al16(v.rstd) || !al16(b.gamma) || !al16(dz_lo) || !al16(b.dgamma) ||
      !al16(b.dbeta) || !al16(b.dbias))
    PL_FAIL(PL_EINVAL, "%s: 16-byte alignment (layer below)", who);
  lo.z = v.z; lo.mean = v.mean; lo.rstd = v.rstd; lo.gamma = b.gamma; lo.bits = v.bits; lo.dz = dz_lo;
  lo.dgamma = b.dgamma; lo.dbeta = b.dbeta; lo.dbias = b.dbias; lo.kscale = kscale; lo.B = B; lo.H = H; lo.rowbits = v.tile_bits ? 0 : 1;
  return PL_OK;
}
}  // namespace

int launch_small_layer_bwd(const SmallLayerBwdArgs& a, hipStream_t s) {
  const int B = a.B, H = a.H, K = a.K;
  if (!small_layer_ok(B, H, K)) PL_FAIL(PL_ESHAPE, "small_layer_bwd: B=%d H=%d K=%d", B, H, K);
  if (!a.dz || !a.W || a.dz_lo == a.dz) PL_FAIL(PL_EINVAL, "small_layer_bwd: bad arguments");
  if (!al16(a.dz) || !al16(a.W) || !al16(a.addend) || !al16(a.gout)) PL_FAIL(PL_EINVAL, "small_layer_bwd: 16-byte alignment");
  BwdArgs p = {};
  PL_TRY(fill_lo(p.lo, a.below, B, H, a.kscale, a.dz_lo, "small_layer_bwd"));
  p.dz = a.dz; p.W = a.W; p.addend = a.addend; p.gout = a.gout;
  p.B = B; p.H = H; p.K = K;
  p.nblk_dx = H / COLS;
  int extra = 0;
  if (a.dW) {
    if (!a.a_in || !al16(a.a_in) || !al16(a.dW) || (K & 127) || (H & 63))
      PL_FAIL(PL_EINVAL, "small_layer_bwd: weight-gradient part (K=%d H=%d)", K, H);
    p.a_in = a.a_in; p.dW = a.dW;
    extra = (K / 128) * (H / 64);
  }
  if (a.dW1) {
    if (!a.x1 || !small_first_ok(a.K1)) PL_FAIL(PL_EINVAL, "small_layer_bwd: first-layer weight gradient (K1=%d)", a.K1);
    p.x1 = a.x1; p.dW1 = a.dW1; p.K1 = a.K1;
  }
  p.nblk_dw = extra;
  if (a.adam && a.adam->n > 0) {
    const AdamWRide& r = *a.adam;
    if (!r.p || !r.g || !r.m || !r.v || (r.n & 3) || !al16(r.p) || !al16(r.g) || !al16(r.m) || !al16(r.v) ||
        (r.lr_dev != nullptr) != (r.t_dev != nullptr))
      PL_FAIL(PL_EINVAL, "small_layer_bwd: AdamW slice");
    p.adam = r;
    p.nblk_adam = (int)std::min<int64_t>(kSmallAdamBlocks, (r.n / 4 + NTHR - 1) / NTHR);
    extra += p.nblk_adam;
  }
  const bool ema = a.ema && p.nblk_adam > 0;           // (no slice: nothing to average in this launch)
  if (ema) PL_TRY(check_ema(*a.ema, "small_layer_bwd"));
  const dim3 grid(H / COLS + extra), block(NTHR);
  void* prof = prof_begin_flops(2.0 * B * H * K * (a.dW ? 2 : 1), s);
  const EmaArg<false> off = {};
  const EmaArg<true> on = {ema ? *a.ema : PLEma{}};
  if (ema) {
    switch (K / (NWAVE * 32)) {
      case 1: hipLaunchKernelGGL((small_bwd_kernel<1, true>), grid, block, 0, s, p, on); break;
      case 2: hipLaunchKernelGGL((small_bwd_kernel<2, true>), grid, block, 0, s, p, on); break;
      default: hipLaunchKernelGGL((small_bwd_kernel<4, true>), grid, block, 0, s, p, on); break;
    }
  } else switch (K / (NWAVE * 32)) {
    case 1: hipLaunchKernelGGL((small_bwd_kernel<1, false>), grid, block, 0, s, p, off); break;
    case 2: hipLaunchKernelGGL((small_bwd_kernel<2, false>), grid, block, 0, s, p, off); break;
    default: hipLaunchKernelGGL((small_bwd_kernel<4, false>), grid, block, 0, s, p, off); break;
  }
  prof_end(prof, s);
  PL_CHECK_LAUNCH("small_layer_bwd");
  return PL_OK;
}

int small_mse_partials(int B, int O) { return (B * O + kMseElems - 1) / kMseElems; }

int small_loss_partials(const Crit& c, int B, int O) {
  return c.kind == PL_CRIT_MPJPE ? (B * (O / c.G) + kMseElems - 1) / kMseElems : small_mse_partials(B, O);
}

int launch_small_mse(const SmallHeadArgs& a, hipStream_t s) {
  const Crit& c = a.crit;
  if (!a.ypart || !a.tgt || !a.y || !a.dpred || !a.mpart || a.NS < 1 || a.B < 1 || a.B > ROWS || !small_top_ok(a.O) || c.G < 1 ||
      a.O % c.G != 0 || (c.kind == PL_CRIT_MPJPE && c.G > kCritMaxGroup))
    PL_FAIL(PL_EINVAL, "small_mse: bad arguments");
  const dim3 grid(small_loss_partials(c, a.B, a.O)), block(256);
  const CritK k = crit_consts(c, a.grad_scale, (int64_t)a.B * a.O, a.O);
  if (c.kind == PL_CRIT_MPJPE) {
    group_dispatch(c, [&](auto g, auto w) {
      hipLaunchKernelGGL((small_mpjpe_kernel<decltype(g)::value, decltype(w)::value>), grid, block, 0, s, a.ypart, a.NS, a.B, a.O,
                         a.bias, a.tgt, k, a.y, a.dpred, a.mpart);
      return 0;
    });
  } else {
    crit_dispatch(c, [&](auto crit, auto w) {
      using C = decltype(crit);
      if constexpr (!C::grouped)
        hipLaunchKernelGGL((small_mse_kernel<C, decltype(w)::value>), grid, block, 0, s, a.ypart, a.NS, a.B, a.O, a.bias, a.tgt, k,
                           a.y, a.dpred, a.mpart);
      return 0;
    });
  }
  PL_CHECK_LAUNCH("small_mse");
  return PL_OK;
}

int launch_small_top_bwd(const SmallTopBwdArgs& a, hipStream_t s) {
  if (!small_layer_ok(a.B, a.H, a.H) || !small_top_ok(a.O)) PL_FAIL(PL_ESHAPE, "small_top_bwd: B=%d H=%d O=%d", a.B, a.H, a.O);
  if (!a.dy || !a.W2 || !a.h || !a.gout || !a.dW2 || !a.db2 || !al16(a.gout) || !al16(a.h))
    PL_FAIL(PL_EINVAL, "small_top_bwd: bad arguments");
  TopArgs p = {};
  PL_TRY(fill_lo(p.lo, a.top, a.B, a.H, a.kscale, a.dz_top, "small_top_bwd"));
  p.dy = a.dy; p.W2 = a.W2; p.h = a.h; p.gout = a.gout; p.dW2 = a.dW2; p.db2 = a.db2; p.B = a.B; p.H = a.H; p.O = a.O;
  if (a.loss) {
    if (!a.mpart || a.np < 1) PL_FAIL(PL_EINVAL, "small_top_bwd: loss partials");
    p.mpart = a.mpart; p.np = a.np; p.inv_n = a.inv_n; p.loss = a.loss; p.tick = a.tick;
  }
  hipLaunchKernelGGL(small_top_bwd_kernel, dim3(a.H / COLS), dim3(NTHR), 0, s, p);
  PL_CHECK_LAUNCH("small_top_bwd");
  return PL_OK;
}

}  // namespace pl

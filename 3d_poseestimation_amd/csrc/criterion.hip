// The train criterion (MSE, L1, smooth-L1, MPJPE; per-joint weights) forward + backward, directly and from the output
// Linear's split-K slabs, the L1 terms of the cycle step, and the MPJPE metric.
//
// They replace, on the reference path, mse_loss (train_1.py:37,94) and loss_MPJPE (train_1.py:19-23).
#include "pl_internal.h"
#include "pose_table.h"
#include "skeleton_terms.h"
#include "streaming.h"

namespace pl {
namespace {

// ---- the criterion (mean) forward + backward: MSE, and the other pointwise kinds of pose_criterion.h ------------------------
// C: the criterion type, W: the weights (pose_criterion.h) -- kWJoint: k.w[(i mod O) / G]; kWRow: k.rw[i / G], loaded with
// the element's operands (n <= INT32_MAX there), times k.w[...] when there are joint weights too.
// <Pointwise<PL_CRIT_MSE>, kWNone> is the MSE kernel as it always was: d, fmaf(d, d, acc), d * coef, block_sum.
template <class C, int W>
__global__ __launch_bounds__(NTHR) void mse_partial_kernel(const float* __restrict__ pred,
                                                           const float* __restrict__ tgt, int64_t n,
                                                           CritK k, float* __restrict__ dpred,
                                                           float* __restrict__ part) {
  __shared__ float sm[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    float rwv = 0.f, wj = 0.f;                          // (kWRow: both weight loads issued with pred and tgt, before d)
    if constexpr (W == kWRow) { rwv = k.rw[(int)i / k.G]; wj = joint_weight_or_one(k, (int)i % k.O / k.G); }
    const float d = pred[i] - tgt[i];
    if constexpr (W == kWRow) {
      const float w = wj * rwv;
      acc = C::add_w(acc, d, w, k);
      if (dpred) dpred[i] = C::grad(d, k) * w;
    } else if constexpr (W == kWJoint) {
      const float w = k.w[(int)(i % k.O) / k.G];
      acc = C::add_w(acc, d, w, k);
      if (dpred) dpred[i] = C::grad(d, k) * w;
    } else {
      acc = C::add(acc, d, k);
      if (dpred) dpred[i] = C::grad(d, k);
    }
  }
  const float t = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// The grouped kind (mpjpe) has an element map of its own: a thread takes whole joints -- the G coordinates of joint i are
// elements i G .. i G + G - 1 of the flat [B][O] tensors -- so no joint is shared between threads, let alone workgroups.
// nj = B J joints, J joints per row (the weight of joint i is k.w[i mod J]; kWRow: k.rw[i], times k.w[i mod J] if any).
template <int G, int W>
__global__ __launch_bounds__(NTHR) void mpjpe_loss_partial_kernel(const float* __restrict__ pred,
                                                                  const float* __restrict__ tgt, int64_t nj, int J,
                                                                  CritK k, float* __restrict__ dpred,
                                                                  float* __restrict__ part) {
  __shared__ float sm[4];
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nj; i += stride) {
    float p[G], t[G], d[G], g[G];
#pragma unroll
    for (int c = 0; c < G; ++c) { p[c] = pred[i * G + c]; t[c] = tgt[i * G + c]; }
    float w, wj = 1.f;
    if constexpr (W == kWRow) { w = k.rw[i]; wj = joint_weight_or_one(k, (int)i % J); }
    else w = W ? k.w[(int)(i % J)] : 1.f;
#pragma unroll
    for (int c = 0; c < G; ++c) d[c] = p[c] - t[c];
    if constexpr (W == kWRow) w = wj * w;
    const float r = joint_norm_grad<G>(d, W ? k.coef * w : k.coef, g);
    acc = W ? fmaf(w, r, acc) : acc + r;
    if (dpred) {
#pragma unroll
      for (int c = 0; c < G; ++c) dpred[i * G + c] = g[c];
    }
  }
  const float tsum = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = tsum;
}

// mse_partial_kernel with pred[i] formed on the fly from the output Linear's split-K slabs (part[s][r][64 padded columns]) and
// stored: y[i] = bias[n] + slabs in order -- skinny_narrow_out_reduce_kernel's sum -- then the same d, fmaf and block_sum on the
// same thread -> element map: y, dpred and the partials equal the two-launch route's bit for bit.  NS slabs, N columns.
// C, W: the criterion and its weights as in mse_partial_kernel (the weight of each element loaded with its slabs; kWRow:
// k.rw[r J + c / G] and, with joint weights, k.w[c / G], both in that first group of loads, their product formed once).
template <int NS, int N, class C, int W>
__global__ __launch_bounds__(NTHR) void mse_partial_from_slabs_kernel(const float* __restrict__ part, int B,
                                                                      const float* __restrict__ bias,
                                                                      const float* __restrict__ tgt, CritK k,
                                                                      float* __restrict__ y, float* __restrict__ dpred,
                                                                      float* __restrict__ mpart) {
  __shared__ float sm[4];
  const int64_t n = (int64_t)B * N;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const size_t slab = (size_t)B * 64;
  float acc = 0.f;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n; i0 += 4 * stride) {
    float u[4][NS], t[4], bs[4], wq[4], wj[4];
    int64_t idx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                       // up to four elements of this thread: every load issued first
      idx[q] = i0 + q * stride;
      const bool ok = idx[q] < n;
      const int r = ok ? (int)(idx[q] / N) : 0, c = ok ? (int)(idx[q] - (int64_t)r * N) : 0;
      const float* p = part + (size_t)r * 64 + c;
#pragma unroll
      for (int s = 0; s < NS; ++s) u[q][s] = ok ? p[(size_t)s * slab] : 0.f;
      t[q] = ok ? tgt[idx[q]] : 0.f;
      bs[q] = (ok && bias) ? bias[c] : 0.f;
      if constexpr (W == kWRow) { wq[q] = ok ? k.rw[r * (N / k.G) + c / k.G] : 0.f; wj[q] = joint_weight_or_one(k, c / k.G); }
      else if constexpr (W == kWJoint) wq[q] = k.w[c / k.G];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (idx[q] >= n) continue;
      float a = bs[q];
#pragma unroll
      for (int s = 0; s < NS; ++s) a += u[q][s];
      y[idx[q]] = a;
      const float d = a - t[q];
      if constexpr (W == kWRow) wq[q] = wj[q] * wq[q];
      if constexpr (W != kWNone) {
        acc = C::add_w(acc, d, wq[q], k);
        dpred[idx[q]] = C::grad(d, k) * wq[q];
      } else {
        acc = C::add(acc, d, k);
        dpred[idx[q]] = C::grad(d, k);
      }
    }
  }
  const float tsum = block_sum(acc, sm);
  if (threadIdx.x == 0) mpart[blockIdx.x] = tsum;
}

// The grouped kind on the slabs, with its own element map: a thread takes whole joints (two per pass; the 2 G NS slab
// loads, the targets, the biases and the weights all issued before the first add), y[i] = bias + slabs in the same order.
template <int NS, int N, int G, int W>
__global__ __launch_bounds__(NTHR) void mpjpe_partial_from_slabs_kernel(const float* __restrict__ part, int B,
                                                                        const float* __restrict__ bias,
                                                                        const float* __restrict__ tgt, CritK k,
                                                                        float* __restrict__ y, float* __restrict__ dpred,
                                                                        float* __restrict__ mpart) {
  static_assert(N % G == 0, "whole joints per row");
  constexpr int J = N / G, Q = 2;
  __shared__ float sm[4];
  const int64_t nj = (int64_t)B * J;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const size_t slab = (size_t)B * 64;
  float acc = 0.f;
  for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < nj; i0 += Q * stride) {
    float u[Q][G][NS], t[Q][G], bs[Q][G], wq[Q], wj[Q];
    int64_t idx[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      idx[q] = i0 + q * stride;
      const bool ok = idx[q] < nj;
      const int r = ok ? (int)(idx[q] / J) : 0, j = ok ? (int)(idx[q] - (int64_t)r * J) : 0;
      const float* p = part + (size_t)r * 64 + j * G;
#pragma unroll
      for (int c = 0; c < G; ++c) {
#pragma unroll
        for (int s = 0; s < NS; ++s) u[q][c][s] = ok ? p[(size_t)s * slab + c] : 0.f;
        t[q][c] = ok ? tgt[idx[q] * G + c] : 0.f;
        bs[q][c] = (ok && bias) ? bias[j * G + c] : 0.f;
      }
      if constexpr (W == kWRow) { wq[q] = ok ? k.rw[idx[q]] : 0.f; wj[q] = joint_weight_or_one(k, j); }
      else wq[q] = W ? k.w[j] : 1.f;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      if (idx[q] >= nj) continue;
      float d[G], g[G];
#pragma unroll
      for (int c = 0; c < G; ++c) {
        float a = bs[q][c];
#pragma unroll
        for (int s = 0; s < NS; ++s) a += u[q][c][s];
        y[idx[q] * G + c] = a;
        d[c] = a - t[q][c];
      }
      if constexpr (W == kWRow) wq[q] = wj[q] * wq[q];
      const float r = joint_norm_grad<G>(d, W ? k.coef * wq[q] : k.coef, g);
      acc = W ? fmaf(wq[q], r, acc) : acc + r;
#pragma unroll
      for (int c = 0; c < G; ++c) dpred[idx[q] * G + c] = g[c];
    }
  }
  const float tsum = block_sum(acc, sm);
  if (threadIdx.x == 0) mpart[blockIdx.x] = tsum;
}

__global__ __launch_bounds__(NTHR) void mse_final_kernel(const float* __restrict__ part, int np,
                                                         float inv_n, float* __restrict__ loss, uint64_t* tick) {
  __shared__ float sm[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < np; i += blockDim.x) acc += part[i];
  const float t = block_sum(acc, sm);
  if (threadIdx.x == 0) {
    loss[0] = t * inv_n;
    // graph replay: one training step is complete as far as its readers of the counter go (every dropout kernel of the
    // forward ran before this kernel, AdamW runs after it)
    if (tick) tick[0] += 1;
  }
}

// ---- L1(mean) terms, forward + backward, several (a, b) pairs per launch -----------------------
constexpr int L1_BLOCKS = 64;
struct L1Terms { PLL1Term t[PL_L1_MAX_TERMS]; };

__global__ __launch_bounds__(NTHR) void l1_partial_kernel(L1Terms T, float grad_scale, float* __restrict__ part) {
  __shared__ float sm[4];
  const PLL1Term q = T.t[blockIdx.y];
  const float coef = grad_scale / (float)q.n;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x; i < q.n; i += (int64_t)L1_BLOCKS * NTHR) {
    const float d = q.a[i] - q.b[i];
    acc += fabsf(d);
    const float g = d > 0.f ? coef : (d < 0.f ? -coef : 0.f);
    if (q.da) q.da[i] = g;
    if (q.db) q.db[i] = -g;
  }
  const float t = block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.y * L1_BLOCKS + blockIdx.x] = t;
}

__global__ __launch_bounds__(64) void l1_final_kernel(const float* __restrict__ part, L1Terms T,
                                                      float* __restrict__ losses) {
  float v = part[blockIdx.x * L1_BLOCKS + threadIdx.x];       // L1_BLOCKS == 64 == one wavefront
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if (threadIdx.x == 0) losses[blockIdx.x] = v / (float)T.t[blockIdx.x].n;
}

// ---- loss_MPJPE --------------------------------------------------------------------------
// XF (pl_mpjpe_accum_t): both tensors are taken out of the model's space as they are loaded, x = y div[c] + sub[c] over
// the 3 J columns of a pose (pose_table.h invert1); XF = false is the kernel as it was.
template <bool XF>
__global__ void mpjpe_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                     int B, int J, int rpc, float* __restrict__ part, const float* __restrict__ sub,
                                     const float* __restrict__ div) {
  const int r0 = blockIdx.x * rpc, r1 = min(B, r0 + rpc);
  for (int j = threadIdx.x; j < J; j += blockDim.x) {
    float s = 0.f;
    float sb[3] = {0.f, 0.f, 0.f}, dv[3] = {1.f, 1.f, 1.f};
    if constexpr (XF) {
      for (int d = 0; d < 3; ++d) { sb[d] = sub[3 * j + d]; dv[d] = div[3 * j + d]; }
    }
    for (int r = r0; r < r1; ++r) {
      const size_t o = ((size_t)r * J + j) * 3;
      float dx, dy, dz;
      if constexpr (XF) {
        dx = pt::invert1(pred[o], sb[0], dv[0]) - pt::invert1(tgt[o], sb[0], dv[0]);
        dy = pt::invert1(pred[o + 1], sb[1], dv[1]) - pt::invert1(tgt[o + 1], sb[1], dv[1]);
        dz = pt::invert1(pred[o + 2], sb[2], dv[2]) - pt::invert1(tgt[o + 2], sb[2], dv[2]);
      } else {
        dx = pred[o] - tgt[o]; dy = pred[o + 1] - tgt[o + 1]; dz = pred[o + 2] - tgt[o + 2];
      }
      s += sqrtf(fmaf(dx, dx, fmaf(dy, dy, dz * dz)));
    }
    part[(size_t)blockIdx.x * J + j] = s;
  }
}

__global__ void mpjpe_final_kernel(const float* __restrict__ part, int np, int J,
                                   float* __restrict__ metric) {
  for (int j = threadIdx.x; j < J; j += blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < np; ++k) s += part[(size_t)k * J + j];
    metric[j] += s;
  }
}

int mse_blocks(int64_t n) {
  int64_t b = (n + NTHR * 4 - 1) / (NTHR * 4);
  if (b > 1024) b = 1024;
  return b < 1 ? 1 : (int)b;
}

template <int N>
void launch_from_slabs(const Crit& c, const CritK& k, dim3 grid, hipStream_t s, const float* part, int B, const float* bias,
                       const float* tgt, float* y, float* dpred, float* mpart) {
  const dim3 block(NTHR);
  if (c.kind == PL_CRIT_MPJPE) {
    group_dispatch(c, [&](auto g, auto w) {
      constexpr int G = decltype(g)::value;
      if constexpr (N % G == 0)
        hipLaunchKernelGGL((mpjpe_partial_from_slabs_kernel<8, N, G, decltype(w)::value>), grid, block, 0, s, part, B, bias, tgt, k, y,
                           dpred, mpart);
      return 0;
    });
  } else {
    crit_dispatch(c, [&](auto crit, auto w) {
      using C = decltype(crit);
      if constexpr (!C::grouped)
        hipLaunchKernelGGL((mse_partial_from_slabs_kernel<8, N, C, decltype(w)::value>), grid, block, 0, s, part, B, bias, tgt, k, y,
                           dpred, mpart);
      return 0;
    });
  }
}

int mpjpe_chunks(int64_t B) {
  int64_t c = (B + 63) / 64;
  if (c > 256) c = 256;
  return c < 1 ? 1 : (int)c;
}

// mpjpe_partial_kernel's only launch site; sub == nullptr: the plain instantiation
int launch_mpjpe(const char* fn, const float* pred, const float* tgt, int64_t B, int64_t joints, const float* sub,
                 const float* div, float* metric, void* scratch, void* stream) {
  if (!pred || !tgt || !metric || !scratch) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (B <= 0 || joints <= 0 || joints > 1024) PL_FAIL(PL_ESHAPE, "%s: B=%lld joints=%lld", fn, (long long)B, (long long)joints);
  hipStream_t s = (hipStream_t)stream;
  const int nc = mpjpe_chunks(B);
  const int rpc = (int)((B + nc - 1) / nc);
  if (sub)
    hipLaunchKernelGGL(mpjpe_partial_kernel<true>, dim3(nc), dim3(64), 0, s, pred, tgt, (int)B, (int)joints, rpc,
                       (float*)scratch, sub, div);
  else
    hipLaunchKernelGGL(mpjpe_partial_kernel<false>, dim3(nc), dim3(64), 0, s, pred, tgt, (int)B, (int)joints, rpc,
                       (float*)scratch, (const float*)nullptr, (const float*)nullptr);
  PL_CHECK_LAUNCH("mpjpe_partial");
  hipLaunchKernelGGL(mpjpe_final_kernel, dim3(1), dim3(64), 0, s, (const float*)scratch, nc, (int)joints,
                     metric);
  PL_CHECK_LAUNCH("mpjpe_final");
  return PL_OK;
}

}  // namespace

int crit_resolve(const PLCriterion* crit, int64_t B, int64_t O, Crit& out, const char* who) {
  out = Crit{};
  if (!crit) return PL_OK;
  // (a kind outside the four, -1 included, is refused before anything past PLCriterion is read: no negative kind has a flag)
  constexpr int flags = PL_CRIT_HAS_SKELETON | PL_CRIT_HAS_ROW_WEIGHTS;
  const int kind = crit->kind > 0 && (crit->kind & flags) ? crit->kind & ~flags : crit->kind;
  if (kind < PL_CRIT_MSE || kind > PL_CRIT_MPJPE) PL_FAIL(PL_EINVAL, "%s: criterion kind %d", who, (int)crit->kind);
  if (kind == PL_CRIT_SMOOTH_L1 && !(crit->beta > 0.f && crit->beta <= 3.0e38f))
    PL_FAIL(PL_EINVAL, "%s: smooth_l1 needs a finite beta > 0 (beta = 0 is l1), got %g", who, (double)crit->beta);
  if (crit->group < 1 || O % crit->group != 0)
    PL_FAIL(PL_ESHAPE, "%s: %lld outputs are not whole joints of %d coordinates", who, (long long)O, (int)crit->group);
  if (kind == PL_CRIT_MPJPE && crit->group > kCritMaxGroup)
    PL_FAIL(PL_ESHAPE, "%s: mpjpe takes joints of at most %d coordinates, got %d", who, kCritMaxGroup, (int)crit->group);
  out.kind = kind; out.G = crit->group; out.w = crit->weights;
  out.beta = kind == PL_CRIT_SMOOTH_L1 ? crit->beta : 1.0f;
  if (crit->kind > 0 && (crit->kind & PL_CRIT_HAS_ROW_WEIGHTS)) {
    if (!(out.rw = crit_row_weights(crit))) PL_FAIL(PL_EINVAL, "%s: PL_CRIT_HAS_ROW_WEIGHTS with a null row_weights", who);
    if (crit->kind & PL_CRIT_HAS_SKELETON)
      PL_FAIL(PL_EINVAL, "%s: row weights together with the skeleton terms are not built (the bone terms have no per-pose weights yet)", who);
    if (B < 1 || B > INT32_MAX / O)
      PL_FAIL(PL_ESHAPE, "%s: row weights index B O = %lld x %lld elements in 32 bits", who, (long long)B, (long long)O);
  }
  if (const PLSkeleton* sk = crit_skeleton(crit)) {
    PL_TRY(skeleton_check(sk, O, crit->group, who));
    out.has_sk = true; out.sk = *sk;
  }
  return PL_OK;
}

// the first half of loss_fwd_bwd_tick: dpred and the per-workgroup partial sums (loss_partials of them); the loss itself is
// summed later by a kind-2 job of launch_reduce_rows_multi (inv_n = crit_inv_n)
int loss_partials(const Crit& c, int64_t B, int64_t O) { return mse_blocks(c.kind == PL_CRIT_MPJPE ? B * O / c.G : B * O); }
int loss_partial_only(const float* pred, const float* tgt, int64_t B, int64_t O, const Crit& c, float grad_scale, float* dpred,
                      void* scratch, void* stream, const char* who) {
  if (!pred || !tgt || !scratch) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  const int64_t n = B * O;
  if (n <= 0) PL_FAIL(PL_ESHAPE, "%s: n = %lld", who, (long long)n);
  // (the weight index of element i is (i mod O) / G in 32-bit arithmetic; the plain MSE call passes its n as O and reads none)
  if ((c.w || c.kind == PL_CRIT_MPJPE) && O > INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: O = %lld", who, (long long)O);
  const CritK k = crit_consts(c, grad_scale, n, O > INT32_MAX ? 1 : (int)O);
  const dim3 grid(loss_partials(c, B, O)), block(NTHR);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)scratch;
  if (c.kind == PL_CRIT_MPJPE) {
    const int J = (int)(O / c.G);
    group_dispatch(c, [&](auto g, auto w) {
      hipLaunchKernelGGL((mpjpe_loss_partial_kernel<decltype(g)::value, decltype(w)::value>), grid, block, 0, s, pred, tgt, n / c.G, J,
                         k, dpred, part);
      return 0;
    });
  } else {
    crit_dispatch(c, [&](auto crit, auto w) {
      using C = decltype(crit);
      if constexpr (!C::grouped)
        hipLaunchKernelGGL((mse_partial_kernel<C, decltype(w)::value>), grid, block, 0, s, pred, tgt, n, k, dpred, part);
      return 0;
    });
  }
  PL_CHECK_LAUNCH("mse_partial");
  return PL_OK;
}

// y = bias + slabs, dpred, loss partials in one launch (mse_partial_from_slabs_kernel); false: shape not specialised
bool mse_from_slabs_supported(int splits, int N) { return splits == 8 && (N == 51 || N == 34); }
int loss_partial_from_slabs(const float* part, int splits, int B, int N, const float* bias, const float* tgt, const Crit& c,
                            float grad_scale, float* y, float* dpred, void* scratch, void* stream) {
  if (!part || !tgt || !y || !dpred || !scratch) PL_FAIL(PL_EINVAL, "mse_partial_from_slabs: null pointer");
  if (!mse_from_slabs_supported(splits, N) || B < 1 || N % c.G != 0)
    PL_FAIL(PL_ESHAPE, "mse_partial_from_slabs: splits=%d N=%d group=%d", splits, N, c.G);
  const int64_t n = (int64_t)B * N;
  const CritK k = crit_consts(c, grad_scale, n, N);
  // (the grouped kind runs the same number of workgroups over its B J joints: the same count of partials either way)
  const dim3 grid(mse_blocks(n));
  if (N == 51) launch_from_slabs<51>(c, k, grid, (hipStream_t)stream, part, B, bias, tgt, y, dpred, (float*)scratch);
  else launch_from_slabs<34>(c, k, grid, (hipStream_t)stream, part, B, bias, tgt, y, dpred, (float*)scratch);
  PL_CHECK_LAUNCH("mse_partial_from_slabs");
  return PL_OK;
}

int loss_fwd_bwd_tick(const float* pred, const float* tgt, int64_t B, int64_t O, const Crit& c, float grad_scale, float* dpred,
                      float* loss_out, void* scratch, uint64_t* tick, void* stream, const char* who) {
  if (!loss_out) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PL_TRY(loss_partial_only(pred, tgt, B, O, c, grad_scale, dpred, scratch, stream, who));
  int np = loss_partials(c, B, O);
  if (c.has_sk) {
    PL_TRY(launch_skeleton_terms(c, pred, tgt, B, O, grad_scale, crit_inv_n(c, B * O), dpred, (float*)scratch + np, stream, who));
    np += skeleton_partials(B);
  }
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(NTHR), 0, (hipStream_t)stream, (const float*)scratch, np,
                     crit_inv_n(c, B * O), loss_out, tick);
  PL_CHECK_LAUNCH("mse_final");
  return PL_OK;
}

}  // namespace pl

extern "C" size_t pl_mse_scratch_bytes(int64_t n) { return (size_t)pl::mse_blocks(n > 0 ? n : 1) * sizeof(float); }

extern "C" size_t pl_pose_loss_scratch_bytes(int64_t B, int64_t O, const PLCriterion* crit) {
  // (the grouped kind's B J joints need no more workgroups than B O elements do; the skeleton pass appends its partials)
  return pl_mse_scratch_bytes(B > 0 && O > 0 ? B * O : 1) + (pl::crit_skeleton(crit) ? pl::sk::kMaxGroups * sizeof(float) : 0);
}

extern "C" int pl_mse_fwd_bwd(const float* pred, const float* tgt, int64_t n, float grad_scale,
                              float* dpred, float* loss_out, void* scratch, void* stream) {
  if (n <= 0) PL_FAIL(PL_ESHAPE, "pl_mse_fwd_bwd: n = %lld", (long long)n);
  return pl::loss_fwd_bwd_tick(pred, tgt, 1, n, pl::Crit{}, grad_scale, dpred, loss_out, scratch, nullptr, stream, "pl_mse_fwd_bwd");
}

extern "C" int pl_pose_loss_fwd_bwd(const float* pred, const float* tgt, int64_t B, int64_t O, const PLCriterion* crit,
                                    float grad_scale, float* dpred, float* loss, void* scratch, void* stream) {
  if (B <= 0 || O <= 0) PL_FAIL(PL_ESHAPE, "pl_pose_loss_fwd_bwd: B=%lld O=%lld", (long long)B, (long long)O);
  pl::Crit c;
  PL_TRY(pl::crit_resolve(crit, B, O, c, "pl_pose_loss_fwd_bwd"));
  return pl::loss_fwd_bwd_tick(pred, tgt, B, O, c, grad_scale, dpred, loss, scratch, nullptr, stream, "pl_pose_loss_fwd_bwd");
}

extern "C" size_t pl_mpjpe_scratch_bytes(int64_t B, int64_t joints) {
  return (size_t)pl::mpjpe_chunks(B) * (size_t)(joints > 0 ? joints : 1) * sizeof(float);
}

extern "C" int pl_mpjpe_accum(const float* pred, const float* tgt, int64_t B, int64_t joints,
                              float* metric, void* scratch, void* stream) {
  return pl::launch_mpjpe("pl_mpjpe_accum", pred, tgt, B, joints, nullptr, nullptr, metric, scratch, stream);
}

extern "C" int pl_mpjpe_accum_t(const float* pred, const float* tgt, int64_t B, int64_t joints, const float* sub_or_null,
                                const float* div_or_null, float* metric, void* scratch, void* stream) {
  if ((sub_or_null != nullptr) != (div_or_null != nullptr)) PL_FAIL(PL_EINVAL, "pl_mpjpe_accum_t: sub and div come together");
  if (sub_or_null && joints > pl::pt::kMaxJoints) PL_FAIL(PL_ESHAPE, "pl_mpjpe_accum_t: joints=%lld with a transform (at most %d)", (long long)joints, pl::pt::kMaxJoints);
  return pl::launch_mpjpe("pl_mpjpe_accum_t", pred, tgt, B, joints, sub_or_null, div_or_null, metric, scratch, stream);
}

extern "C" size_t pl_l1_scratch_bytes(int nterms) {
  return (size_t)(nterms > 0 ? nterms : 1) * pl::L1_BLOCKS * sizeof(float);
}

extern "C" int pl_l1_terms_fwd_bwd(const PLL1Term* terms, int nterms, float grad_scale, float* losses,
                                   void* scratch, void* stream) {
  if (!terms || !losses || !scratch) PL_FAIL(PL_EINVAL, "pl_l1_terms_fwd_bwd: null pointer");
  if (nterms < 1 || nterms > PL_L1_MAX_TERMS) PL_FAIL(PL_EINVAL, "pl_l1_terms_fwd_bwd: nterms=%d", nterms);
  pl::L1Terms T = {};
  for (int t = 0; t < nterms; ++t) {
    if (!terms[t].a || !terms[t].b || terms[t].n <= 0)
      PL_FAIL(PL_EINVAL, "pl_l1_terms_fwd_bwd: term %d has a null operand or n <= 0", t);
    T.t[t] = terms[t];
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pl::l1_partial_kernel, dim3(pl::L1_BLOCKS, nterms), dim3(pl::NTHR), 0, s, T, grad_scale, (float*)scratch);
  PL_CHECK_LAUNCH("l1_partial");
  hipLaunchKernelGGL(pl::l1_final_kernel, dim3(nterms), dim3(64), 0, s, (const float*)scratch, T, losses);
  PL_CHECK_LAUNCH("l1_final");
  return PL_OK;
}

// The flat AdamW step's device pieces, shared by the optimizer kernel (optim.hip) and the small-batch backward launches
// that carry a slice of the step (small_layer.hip): torch.optim.AdamW's single-tensor update order
// (phase1_lifting/train_1.py:39 optimizer, :89 step).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/poselift.h"

namespace pl {

struct AdamWK {
  float decay;       // 1 - lr*wd
  float one_m_b1, b2, one_m_b2;
  float step_size;   // lr / (1 - b1^t)
  float bc2_sqrt;    // sqrt(1 - b2^t)
  float eps, gscale;
};

// What the step is given; the per-step constants are derived ON THE DEVICE (every thread, once: two double pow),
// so that a captured graph advances them by itself: t = t_base + *t_dev, lr = *lr_dev when the pointers are set
// (the eager call passes them by value through the same code, hence the same bits).
struct AdamWIn {
  float lr, beta1, beta2, eps, wd, gscale;
  int64_t t;
  const float* lr_dev;
  const uint64_t* t_dev;
  // GEMM operand planes of the 1024-wide weight matrices, refreshed by the step that changes them (PLAdamWPlanes):
  // the forward then needs no split pass of its own
  int nseg, kind;
  float pscale;
  int64_t seg_off[PL_ADAMW_MAX_SEGS], seg_n[PL_ADAMW_MAX_SEGS];
  unsigned short* seg_h[PL_ADAMW_MAX_SEGS];
  unsigned short* seg_l[PL_ADAMW_MAX_SEGS];
  uint32_t* range;   // the range guard's record or NULL (fp16 planes at pscale: the weight slot)
  // pl_grad_norm_clip's record or NULL (gradnorm.hip): gscale *= coef, t -= skipped, no update when skip
  const PLClipRecord* clip;
};

// a slice [p, p + n) of the step carried by another kernel's spare workgroups (small_layer.hip): same fields, same constants
struct AdamWRide {
  float *p, *m, *v;
  const float* g;
  int64_t n;                 // floats; n % 4 == 0, the four pointers 16-byte aligned
  float lr, beta1, beta2, eps, wd, gscale;
  int64_t t;
  const float* lr_dev;
  const uint64_t* t_dev;
};

template <class A>
__device__ __forceinline__ AdamWK adamw_consts(const A& a) {
  const double lr = a.lr_dev ? (double)a.lr_dev[0] : (double)a.lr;
  const double t = (double)(a.t + (a.t_dev ? (int64_t)a.t_dev[0] : 0));
  const double bc1 = 1.0 - pow((double)a.beta1, t);
  const double bc2 = 1.0 - pow((double)a.beta2, t);
  AdamWK k;
  k.decay = (float)(1.0 - lr * (double)a.wd);
  k.one_m_b1 = (float)(1.0 - (double)a.beta1);
  k.b2 = a.beta2;
  k.one_m_b2 = (float)(1.0 - (double)a.beta2);
  k.step_size = (float)(lr / bc1);
  k.bc2_sqrt = (float)sqrt(bc2);
  k.eps = a.eps;
  k.gscale = a.gscale;
  return k;
}

// The same constants behind pl_grad_norm_clip's record (the clipping forms of the optimizer kernel): a skipped step does not
// count in the bias corrections (t - skipped: what a loop that does not call optimizer.step() gives), and the clipping
// coefficient folds into the gradient scale as ONE fp32 product.  (Its own copy rather than a parameter of adamw_consts:
// the constants of the step without a record compile to the code they always did.)
__device__ __forceinline__ AdamWK adamw_consts_clip(const AdamWIn& a, const PLClipRecord* clip) {
  const double lr = a.lr_dev ? (double)a.lr_dev[0] : (double)a.lr;
  const double t = (double)(a.t + (a.t_dev ? (int64_t)a.t_dev[0] : 0) - (int64_t)clip->skipped);
  const double bc1 = 1.0 - pow((double)a.beta1, t);
  const double bc2 = 1.0 - pow((double)a.beta2, t);
  AdamWK k;
  k.decay = (float)(1.0 - lr * (double)a.wd);
  k.one_m_b1 = (float)(1.0 - (double)a.beta1);
  k.b2 = a.beta2;
  k.one_m_b2 = (float)(1.0 - (double)a.beta2);
  k.step_size = (float)(lr / bc1);
  k.bc2_sqrt = (float)sqrt(bc2);
  k.eps = a.eps;
  k.gscale = a.gscale * clip->coef;
  return k;
}

// ---- averaged (EMA) weights: e <- e + (p_new - e) (1 - d_n), kept by the launch that holds the new p in registers ----------
// PLEma (poselift.h) is what the kernels are given.  n = t_taken - t0 is the 1-based count of this EMA update, from the
// inputs the bias corrections use (t + *t_dev, minus the record's skipped count behind pl_grad_norm_clip), so a captured graph
// advances it by itself; d_n = decay, or min(decay, (1 + n) / (10 + n)) with warmup; 1 - d_n is formed in double and
// rounded once.  A skipped step never gets here (e stays bitwise, like p, m, v) and so does not count in n.
template <class A>
__device__ __forceinline__ float ema_omd(const A& a, const PLClipRecord* clip, const PLEma& ema) {
  const int64_t taken = a.t + (a.t_dev ? (int64_t)a.t_dev[0] : 0) - (clip ? (int64_t)clip->skipped : 0);
  const double n = (double)(taken - ema.t0);
  double d = (double)ema.decay;
  if (ema.warmup) d = fmin(d, (1.0 + n) / (10.0 + n));
  return (float)(1.0 - d);
}

// the kernel argument of a kernel templated on whether it keeps the average: nothing, or the PLEma
template <bool EMA>
struct EmaArg {};
template <>
struct EmaArg<true> {
  PLEma v;
};

// fp32, exactly two roundings (the difference, the fused multiply-add), on every route
__device__ __forceinline__ void ema_one(float& e, float p_new, float omd) { e = __fmaf_rn(p_new - e, omd, e); }

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, const AdamWK& k) {
  g *= k.gscale;
  p *= k.decay;
  m = m + (g - m) * k.one_m_b1;
  v = v * k.b2 + (k.one_m_b2 * g) * g;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p - k.step_size * (m / denom);
}


// p, m, v (and g read) of elements [4 i0, n) in float4 steps of `stride` threads: the loop of adamw_kernel without the planes.
// EMA: the average e beside them, from the registers that hold the new p (EMA = false is the loop as it was: e, omd unused)
template <bool EMA = false>
__device__ __forceinline__ void adamw_span(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                           float* __restrict__ v, int64_t n4, int64_t i0, int64_t stride, const AdamWK& k,
                                           float* __restrict__ e = nullptr, float omd = 0.f) {
  for (int64_t i = i0; i < n4; i += stride) {
    float4 pv = *reinterpret_cast<const float4*>(p + 4 * i), mv = *reinterpret_cast<const float4*>(m + 4 * i);
    float4 vv = *reinterpret_cast<const float4*>(v + 4 * i);
    const float4 gv = *reinterpret_cast<const float4*>(g + 4 * i);
    adamw_one(pv.x, gv.x, mv.x, vv.x, k);
    adamw_one(pv.y, gv.y, mv.y, vv.y, k);
    adamw_one(pv.z, gv.z, mv.z, vv.z, k);
    adamw_one(pv.w, gv.w, mv.w, vv.w, k);
    *reinterpret_cast<float4*>(p + 4 * i) = pv;
    *reinterpret_cast<float4*>(m + 4 * i) = mv;
    *reinterpret_cast<float4*>(v + 4 * i) = vv;
    if constexpr (EMA) {
      float4 ev = *reinterpret_cast<const float4*>(e + 4 * i);
      ema_one(ev.x, pv.x, omd);
      ema_one(ev.y, pv.y, omd);
      ema_one(ev.z, pv.z, omd);
      ema_one(ev.w, pv.w, omd);
      *reinterpret_cast<float4*>(e + 4 * i) = ev;
    }
  }
}

}  // namespace pl

// The pointwise part of the lifter's training criterion (include/poselift.h PLCriterion) as compile-time
// types: every loss kernel is written once over a criterion type and a weights state (none, per joint, per pose and
// joint: DESIGN 3d.2b), the kind is chosen at the launch, and no element loop branches on it.
// d = prediction - target (fp32), w = the joint's (effective) weight, k = CritK.
//
//   kind        accumulated term                         gradient of the element
//   mse         fmaf(d, d, acc)   [fmaf(w d, d, acc)]    d * coef                       coef = s * 2 / n
//   l1          acc + |d|         [fmaf(w, |d|, acc)]    d > 0 ? coef : d < 0 ? -coef : 0            coef = s / n
//   smooth_l1   acc + rho(d)      [fmaf(w, rho, acc)]    |d| >= beta ? (d > 0 ? coef : -coef) : d * cb   cb = coef / beta
//               rho = |d| >= beta ? |d| - hb : d * d * qb          hb = beta / 2, qb = 0.5 / beta
//   mpjpe       acc + r           [fmaf(w, r, acc)]      ss == 0 ? 0 : d_g * (cw / r)   coef = s / (B J), cw = coef [* w]
//               ss = d_0 d_0, then fmaf(d_g, d_g, ss); r = sqrtf(ss)
// The weighted gradient of the three pointwise kinds is (the unweighted one) * w.  The MSE entries are the expressions the
// MSE kernels always had: that instantiation's bits do not move.  A NaN d takes the `else` arm of every comparison: L1's
// gradient is 0, smooth-L1's d * cb = NaN, MPJPE's whole joint NaN (ss is NaN, not 0) -- torch's sets.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/poselift.h"
#include "skeleton_terms.h"

namespace pl {

// A criterion resolved against a shape [B][O]: what the launchers hand their kernels (crit_resolve, criterion.hip).
struct Crit {
  int kind = PL_CRIT_MSE;
  int G = 1;                    // coordinates per joint; O = J * G
  float beta = 1.0f;
  const float* w = nullptr;     // J device floats, or NULL = all ones
  const float* rw = nullptr;    // [B][J] device floats, the per-pose joint weights (PL_CRIT_HAS_ROW_WEIGHTS), or NULL
  bool has_sk = false;          // the skeleton terms (skeleton.hip) follow the loss pass: one launch more
  PLSkeleton sk = {};           // ... a validated copy
};
// the skeleton a criterion carries (PL_CRIT_HAS_SKELETON in kind, PLSkeletonCriterion), or NULL
inline const PLSkeleton* crit_skeleton(const PLCriterion* crit) {
  return crit && (crit->kind & PL_CRIT_HAS_SKELETON) ? reinterpret_cast<const PLSkeletonCriterion*>(crit)->skeleton : nullptr;
}
// The skeleton pass on [B][O] tensors after the base loss pass wrote dpred and its partials: adds into dpred (NULL: the value
// only) and writes skeleton_partials(B) partial sums to part, pre-scaled so that their sum times inv_n (the base criterion's
// crit_inv_n) is lambda_bone L_bone + lambda_sym L_sym.  skeleton_terms_kernel's only launch site.
int skeleton_partials(int64_t B);
int launch_skeleton_terms(const Crit& c, const float* pred, const float* tgt, int64_t B, int64_t O, float grad_scale, float inv_n,
                          float* dpred, float* part, void* stream, const char* who);
// PL_ESHAPE / PL_EINVAL as include/poselift.h lists them; G = the criterion's group
int skeleton_check(const PLSkeleton* sk, int64_t O, int G, const char* who);
// the row weights a criterion carries (PL_CRIT_HAS_ROW_WEIGHTS in kind, PLRowWeightsCriterion), or NULL
inline const float* crit_row_weights(const PLCriterion* crit) {
  return crit && (crit->kind & PL_CRIT_HAS_ROW_WEIGHTS) ? reinterpret_cast<const PLRowWeightsCriterion*>(crit)->row_weights : nullptr;
}
// crit == NULL: plain MSE.  PL_EINVAL: unknown kind, beta <= 0 or not finite on smooth_l1; PL_ESHAPE: group < 1, O % group,
// group > kCritMaxGroup on mpjpe (a joint's coordinates live in one thread's registers).  Row weights: PL_EINVAL when NULL
// under their flag or together with a skeleton, PL_ESHAPE when B O > INT32_MAX.
constexpr int kCritMaxGroup = 4;
int crit_resolve(const PLCriterion* crit, int64_t B, int64_t O, Crit& out, const char* who);

// the constants of one launch, computed once on the host in fp32
struct CritK {
  float coef, cb, beta, hb, qb;
  const float* w;
  int O, G;
  const float* rw;
};
inline CritK crit_consts(const Crit& c, float grad_scale, int64_t n /* = B O */, int O) {
  CritK k = {};
  switch (c.kind) {
    case PL_CRIT_MSE: k.coef = grad_scale * 2.0f / (float)n; break;
    case PL_CRIT_MPJPE: k.coef = grad_scale / (float)(n / c.G); break;
    default: k.coef = grad_scale / (float)n; break;
  }
  k.beta = c.beta; k.cb = k.coef / c.beta; k.hb = 0.5f * c.beta; k.qb = 0.5f / c.beta;
  k.w = c.w; k.O = O; k.G = c.G; k.rw = c.rw;
  return k;
}
// what the summed partials are multiplied by: 1 / (B O), for mpjpe 1 / (B J)
inline float crit_inv_n(const Crit& c, int64_t n /* = B O */) { return 1.0f / (float)(c.kind == PL_CRIT_MPJPE ? n / c.G : n); }

template <int KIND>
struct Pointwise;
template <>
struct Pointwise<PL_CRIT_MSE> {
  static constexpr bool grouped = false;
  static __device__ __forceinline__ float first(float d, const CritK&) { return d * d; }
  static __device__ __forceinline__ float add(float acc, float d, const CritK&) { return fmaf(d, d, acc); }
  static __device__ __forceinline__ float add_w(float acc, float d, float w, const CritK&) { return fmaf(w * d, d, acc); }
  static __device__ __forceinline__ float grad(float d, const CritK& k) { return d * k.coef; }
};
template <>
struct Pointwise<PL_CRIT_L1> {
  static constexpr bool grouped = false;
  static __device__ __forceinline__ float first(float d, const CritK&) { return fabsf(d); }
  static __device__ __forceinline__ float add(float acc, float d, const CritK&) { return acc + fabsf(d); }
  static __device__ __forceinline__ float add_w(float acc, float d, float w, const CritK&) { return fmaf(w, fabsf(d), acc); }
  static __device__ __forceinline__ float grad(float d, const CritK& k) { return d > 0.f ? k.coef : (d < 0.f ? -k.coef : 0.f); }
};
template <>
struct Pointwise<PL_CRIT_SMOOTH_L1> {
  static constexpr bool grouped = false;
  static __device__ __forceinline__ float first(float d, const CritK& k) {
    const float a = fabsf(d);
    return a >= k.beta ? a - k.hb : d * d * k.qb;
  }
  static __device__ __forceinline__ float add(float acc, float d, const CritK& k) { return acc + first(d, k); }
  static __device__ __forceinline__ float add_w(float acc, float d, float w, const CritK& k) { return fmaf(w, first(d, k), acc); }
  static __device__ __forceinline__ float grad(float d, const CritK& k) {
    return fabsf(d) >= k.beta ? (d > 0.f ? k.coef : -k.coef) : d * k.cb;
  }
};
template <>
struct Pointwise<PL_CRIT_MPJPE> {
  static constexpr bool grouped = true;
};

// one joint of the grouped kind: d[G] in, gradient g[G] out, returns r = ||d||
template <int G>
__device__ __forceinline__ float joint_norm_grad(const float (&d)[G], float cw, float (&g)[G]) {
  float ss = d[0] * d[0];
#pragma unroll
  for (int c = 1; c < G; ++c) ss = fmaf(d[c], d[c], ss);
  const float r = sqrtf(ss);
  const float q = cw / r;
#pragma unroll
  for (int c = 0; c < G; ++c) g[c] = ss == 0.f ? 0.f : d[c] * q;
  return r;
}

// The weights of a launch, the W template parameter of every loss kernel: none, one per joint (k.w[j]), or one per pose and
// joint (k.rw[b J + j], times k.w[j] when the criterion has joint weights too: a kernel-argument test, the same in every
// lane -- the row-weight instantiation serves both, so the old two keep their text).
constexpr int kWNone = 0, kWJoint = 1, kWRow = 2;
template <int W>
using WeightsC = std::integral_constant<int, W>;
// The effective weight W_bj of the row-weight instantiation in two steps, so that no product (and with it no wait for a
// load) stands between the loads of an element: joint_weight_or_one is issued with the element's other loads -- only the
// load is under the kernel-uniform test -- and the one fp32 product w_j * rw[b][j] is formed where the weight is first
// used.  Without joint weights w_j = 1 and fl(1 * r) = r: the bits of the row weight itself.
__device__ __forceinline__ float joint_weight_or_one(const CritK& k, int j) { return k.w ? k.w[j] : 1.f; }

// (kind, weights) -> f(Pointwise<kind>{}, WeightsC<W>{}): the one place a launch turns the run-time kind into types
template <class F, class P>
inline int weights_dispatch(const Crit& c, F&& f, P p) {
  return c.rw ? f(p, WeightsC<kWRow>{}) : c.w ? f(p, WeightsC<kWJoint>{}) : f(p, WeightsC<kWNone>{});
}
template <class F>
inline int crit_dispatch(const Crit& c, F&& f) {
  switch (c.kind) {
    case PL_CRIT_MSE: return weights_dispatch(c, f, Pointwise<PL_CRIT_MSE>{});
    case PL_CRIT_L1: return weights_dispatch(c, f, Pointwise<PL_CRIT_L1>{});
    case PL_CRIT_SMOOTH_L1: return weights_dispatch(c, f, Pointwise<PL_CRIT_SMOOTH_L1>{});
    default: return weights_dispatch(c, f, Pointwise<PL_CRIT_MPJPE>{});
  }
}
// ... and the group size of the grouped kind: f(std::integral_constant<int, G>{}, WeightsC<W>{}), G = 1 .. kCritMaxGroup
template <class F>
inline int group_dispatch(const Crit& c, F&& f) {
  switch (c.G) {
    case 1: return weights_dispatch(c, f, std::integral_constant<int, 1>{});
    case 2: return weights_dispatch(c, f, std::integral_constant<int, 2>{});
    case 3: return weights_dispatch(c, f, std::integral_constant<int, 3>{});
    default: return weights_dispatch(c, f, std::integral_constant<int, 4>{});
  }
}

}  // namespace pl

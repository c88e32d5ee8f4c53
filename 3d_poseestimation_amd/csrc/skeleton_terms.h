// The bone-length and left/right symmetry terms of the train criterion (include/poselift.h PLSkeleton): the
// arithmetic of one pose, written once for the device and the host.  skeleton.hip: skeleton_terms_kernel, bone_lengths_kernel
// and the test hook pl_skeleton_terms_host run this text.
//
// One pose: p, t are its rows of the prediction and the target, J joints of G coordinates, already in raw units (raw1 below,
// applied as the rows are staged).  In fp32, every operation rounded once, nothing contracted but the fmaf written out:
//
//   bone k = (c, q)          d_g = p[c G + g] - p[q G + g];  ss = d_0 d_0, then ss = fmaf(d_g, d_g, ss);  lh_k = sqrtf(ss)
//                            the target's l_k likewise from t
//   bone term                e = lh_k - l_k;       l1: sb = sb + |e|,  u_k = e > 0 ? wb : e < 0 ? -wb : 0
//                                                  mse: sb = fmaf(e, e, sb),  u_k = e * (2 wb)
//   pair m = (a, b)          e = lh_a - lh_b;      l1: sp = sp + |e|,  v = e > 0 ? ws : e < 0 ? -ws : 0
//   (in pair order)                                mse: sp = fmaf(e, e, sp),  v = e * (2 ws);    u_a = u_a + v,  u_b = u_b - v
//   gradient, bones in order r_k = lh_k == 0 ? 0 : u_k / lh_k;   x = d_g * r_k   (d_g recomputed from p: the same bits)
//                            with a transform  g[c G + g] += x * div[c G + g],  g[q G + g] -= x * div[q G + g]
//                            without           g[c G + g] += x,                 g[q G + g] -= x
//   the pose's value         (lwb * sb) + (lws * sp)
//   constants (host, fp32)   cb = s / (float)(B K), cs = s / (float)(B S);  lb = 1 / ((float)(B K) * inv_n), ls likewise, inv_n
//                            the factor the finaliser multiplies the summed partials by;  device: wb = lambda_bone * cb,
//                            ws = lambda_sym * cs, lwb = lambda_bone * lb, lws = lambda_sym * ls
//
// A NaN e takes the last arm of l1's comparisons (u = 0) and 0 / NaN, 0 * NaN are NaN: a NaN coordinate of the prediction
// reaches every coordinate of both joints of each bone that touches it, a NaN in the target alone reaches none under l1.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SK_HD __host__ __device__ inline
#else
#define SK_HD inline
#endif

namespace pl {
namespace sk {

constexpr int kMaxJoints = 32, kMaxBones = 31, kMaxPairs = 16;
constexpr int kPoses = 64;          // poses per workgroup = lanes of its one wavefront
constexpr int kMaxGroups = 64;      // workgroups (= partial sums) of one launch at most

// the launch constants computed once on the host
struct Consts { float cb, cs, lb, ls; };
inline Consts consts(int64_t B, int K, int S, float grad_scale, float inv_n) {
  Consts c = {};
  const float nb = (float)(B * K);
  c.cb = grad_scale / nb;
  c.lb = 1.0f / (nb * inv_n);
  if (S > 0) {
    const float ns = (float)(B * S);
    c.cs = grad_scale / ns;
    c.ls = 1.0f / (ns * inv_n);
  }
  return c;
}

// a coordinate of the model's space back in raw units: two roundings, and a NaN stays one where div == 0
SK_HD float raw1(float y, float sub, float div) {
#pragma clang fp contract(off)
  const float t = y * div;
  return t + sub;
}

template <int G>
SK_HD float bone_len(const float* x, int c, int q, float (&d)[G]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int g = 0; g < G; ++g) d[g] = x[c * G + g] - x[q * G + g];
  float ss = d[0] * d[0];
#pragma unroll
  for (int g = 1; g < G; ++g) ss = fmaf(d[g], d[g], ss);
  return sqrtf(ss);
}

// RHO: 0 = l1, 1 = mse
template <int RHO>
SK_HD float rho_add(float acc, float e) {
#pragma clang fp contract(off)
  return RHO == 0 ? acc + fabsf(e) : fmaf(e, e, acc);
}
template <int RHO>
SK_HD float rho_grad(float e, float w) {
#pragma clang fp contract(off)
  return RHO == 0 ? (e > 0.f ? w : (e < 0.f ? -w : 0.f)) : e * (2.0f * w);
}

// The tables as pose_terms reads them: child(k), parent(k) of bone k < K, pa(m), pb(m) the bone indices of pair m < S, div [J G]
// with a transform.  A bone joins two different joints and a pair two different bones.
struct Tables {                                     // plain arrays (the host hook)
  int K, S;
  const int32_t* c_; const int32_t* q_; const int32_t* a_; const int32_t* b_;
  const float* div;
  int child(int k) const { return c_[k]; }
  int parent(int k) const { return q_[k]; }
  int pa(int m) const { return a_[m]; }
  int pb(int m) const { return b_[m]; }
};
#if defined(__HIPCC__)
// One wavefront: lane k keeps entry k of each table in a register (K <= 31, S <= 16 < 64 lanes) and a wave-uniform index
// fetches it with a lane read -- no memory latency inside the per-bone loops.  Fill cv .. bv with every lane active.
struct LaneTables {
  int K, S;
  int cv, qv, av, bv;
  const float* div;
  __device__ int child(int k) const { return __builtin_amdgcn_readlane(cv, k); }
  __device__ int parent(int k) const { return __builtin_amdgcn_readlane(qv, k); }
  __device__ int pa(int m) const { return __builtin_amdgcn_readlane(av, m); }
  __device__ int pb(int m) const { return __builtin_amdgcn_readlane(bv, m); }
};
#endif

// One pose.  p: the prediction's row; t: the target's row on entry, and -- grad -- the pose's gradient row on return (W =
// J G floats); lh, u: K floats of scratch each (lh returns the prediction's bone lengths).  Returns the pose's value.
template <int RHO, int G, bool XF, class TB>
SK_HD float pose_terms(const float* p, float* t, float* lh, float* u, int W, const TB& T, float wb, float ws, float lwb,
                       float lws, bool grad) {
#pragma clang fp contract(off)
  float d[G];
  float sb = 0.f, sp = 0.f;
  for (int k = 0; k < T.K; ++k) {
    const int c = T.child(k), q = T.parent(k);
    const float l = bone_len<G>(t, c, q, d);
    const float h = bone_len<G>(p, c, q, d);
    const float e = h - l;
    sb = rho_add<RHO>(sb, e);
    lh[k] = h;
    u[k] = rho_grad<RHO>(e, wb);
  }
  for (int m = 0; m < T.S; ++m) {
    const int a = T.pa(m), b = T.pb(m);
    const float e = lh[a] - lh[b];
    sp = rho_add<RHO>(sp, e);
    const float v = rho_grad<RHO>(e, ws);
    u[a] = u[a] + v;
    u[b] = u[b] - v;
  }
  if (grad) {
    for (int i = 0; i < W; ++i) t[i] = 0.f;
    for (int k = 0; k < T.K; ++k) {
      const int c = T.child(k), q = T.parent(k);
      bone_len<G>(p, c, q, d);
      const float h = lh[k];
      const float r = h == 0.f ? 0.f : u[k] / h;
      float gc[G], gq[G];                 // (c != q: both joints' entries are read before either is written)
#pragma unroll
      for (int g = 0; g < G; ++g) { gc[g] = t[c * G + g]; gq[g] = t[q * G + g]; }
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const float x = d[g] * r;
        if constexpr (XF) {
          gc[g] = gc[g] + x * T.div[c * G + g];
          gq[g] = gq[g] - x * T.div[q * G + g];
        } else {
          gc[g] = gc[g] + x;
          gq[g] = gq[g] - x;
        }
      }
#pragma unroll
      for (int g = 0; g < G; ++g) { t[c * G + g] = gc[g]; t[q * G + g] = gq[g]; }
    }
  }
  return (lwb * sb) + (lws * sp);
}

}  // namespace sk
}  // namespace pl

// The skeleton terms of the train criterion: bone lengths and left/right symmetry (include/poselift.h PLSkeleton; DESIGN
// 3d.2).  One launch after the base loss pass adds the terms' gradient into dpred and appends their partial sums to the
// pass's own; pl_bone_lengths serves evaluation.  The per-pose arithmetic is skeleton_terms.h, shared with
// pl_skeleton_terms_host.
#include <string.h>

#include "pl_internal.h"
#include "skeleton_terms.h"
#include "streaming.h"

namespace pl {
namespace {

constexpr int kWide = 4, kNarrow = 8;      // float4 / float loads of each tensor a lane issues before it uses the first

struct SkArgs {
  int J, K, S;
  const int32_t* child; const int32_t* parent; const int32_t* pa; const int32_t* pb;
  const float* tw; const float* sub; const float* div;
  sk::Consts c;
};

// One lane per pose, 64 poses per one-wave workgroup, in the shape of pose_errors_kernel (metrics.hip): the workgroup brings
// its poses of both tensors into LDS coalesced (16 bytes a lane where both pointers allow it), a pose's row padded to an odd
// number of floats so the 64 lanes, each walking its own row, fall on distinct banks.  pose_terms() leaves the pose's
// gradient in the target's row; the workgroup then adds the rows into dy coalesced (read, add, store; an element whose
// gradient is 0 is not touched, so a lambda of 0 leaves every bit of dy alone).  Lane k keeps entry k of each table in a register (sk::LaneTables);
// div in the gradient and the two lambdas are read at wave-uniform addresses.  Workgroups stride over the 64-pose chunks; a lane sums its poses' values
// in chunk order, the wave adds the lanes in a fixed tree: one partial per workgroup, no atomics.
template <int RHO, int G, bool XF>
__global__ __launch_bounds__(sk::kPoses) void skeleton_terms_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                    int64_t B, SkArgs a, float* __restrict__ dy,
                                                                    float* __restrict__ part) {
  extern __shared__ __align__(16) float lds[];
  const int W = a.J * G, RS = W | 1, KS = a.K | 1;
  float* lp = lds;
  float* lt = lp + sk::kPoses * RS;
  float* lh = lt + sk::kPoses * RS;
  float* lu = lh + sk::kPoses * KS;
  const int tid = threadIdx.x;
  const float lam_b = a.tw[0], lam_s = a.tw[1];
  const float wb = lam_b * a.c.cb, ws = lam_s * a.c.cs, lwb = lam_b * a.c.lb, lws = lam_s * a.c.ls;
  const sk::LaneTables T = {a.K, a.S, tid < a.K ? a.child[tid] : 0, tid < a.K ? a.parent[tid] : 0, tid < a.S ? a.pa[tid] : 0,
                            tid < a.S ? a.pb[tid] : 0, a.div};
  // (a chunk starts 256 W bytes into each tensor: its alignment is the tensor's)
  const bool wide = ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt)) & 15) == 0;
  const int64_t chunks = (B + sk::kPoses - 1) / sk::kPoses;
  const int drow = 256 / W, dcol = 256 % W;                // 64 lanes x 4 floats further on
  float acc = 0.f;
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t b0 = ch * sk::kPoses;
    const int nb = (int)((B - b0) < sk::kPoses ? (B - b0) : sk::kPoses);
    const int n = nb * W, n4 = wide ? n >> 2 : 0;          // floats (and whole float4s) of this chunk
    const float* gp = pred + b0 * W;
    const float* gt = tgt + b0 * W;
    // (every load of a batch is issued before its first use: a lane keeps 8 wide or 16 narrow loads in flight)
    int row = (4 * tid) / W, col = 4 * tid - row * W;
    for (int q0 = tid; q0 < n4; q0 += kWide * sk::kPoses) {
      float4 vp[kWide], vt[kWide];
#pragma unroll
      for (int u = 0; u < kWide; ++u) {
        const int q = q0 + u * sk::kPoses;
        if (q < n4) {
          vp[u] = reinterpret_cast<const float4*>(gp)[q];
          vt[u] = reinterpret_cast<const float4*>(gt)[q];
        }
      }
#pragma unroll
      for (int u = 0; u < kWide; ++u) {
        if (q0 + u * sk::kPoses >= n4) break;
        const float ep[4] = {vp[u].x, vp[u].y, vp[u].z, vp[u].w}, et[4] = {vt[u].x, vt[u].y, vt[u].z, vt[u].w};
        int r = row, c = col;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if constexpr (XF) {
            lp[r * RS + c] = sk::raw1(ep[k], a.sub[c], a.div[c]);
            lt[r * RS + c] = sk::raw1(et[k], a.sub[c], a.div[c]);
          } else {
            lp[r * RS + c] = ep[k];
            lt[r * RS + c] = et[k];
          }
          if (++c == W) { c = 0; ++r; }
        }
        row += drow; col += dcol;
        if (col >= W) { col -= W; ++row; }
      }
    }
    // at most 3 floats, or all of them off 16-byte alignment
    for (int i0 = 4 * n4 + tid; i0 < n; i0 += kNarrow * sk::kPoses) {
      float ep[kNarrow], et[kNarrow];
#pragma unroll
      for (int u = 0; u < kNarrow; ++u) {
        const int i = i0 + u * sk::kPoses;
        if (i < n) { ep[u] = gp[i]; et[u] = gt[i]; }
      }
#pragma unroll
      for (int u = 0; u < kNarrow; ++u) {
        const int i = i0 + u * sk::kPoses;
        if (i >= n) break;
        const int r = i / W, c = i - r * W;
        if constexpr (XF) {
          lp[r * RS + c] = sk::raw1(ep[u], a.sub[c], a.div[c]);
          lt[r * RS + c] = sk::raw1(et[u], a.sub[c], a.div[c]);
        } else {
          lp[r * RS + c] = ep[u];
          lt[r * RS + c] = et[u];
        }
      }
    }
    __syncthreads();
    // (every lane runs it, so the lane reads of the tables happen with all lanes active; a lane past the batch works on
    // whatever its own rows hold and its value and gradient row are dropped)
    const float v = sk::pose_terms<RHO, G, XF>(lp + tid * RS, lt + tid * RS, lh + tid * KS, lu + tid * KS, W, T, wb, ws, lwb, lws,
                                               dy != nullptr);
    if (tid < nb) acc += v;
    __syncthreads();
    if (dy) {
      float* gd = dy + b0 * W;
      const int erow = sk::kPoses / W, ecol = sk::kPoses % W;          // 64 floats further on
      int r = tid / W, c = tid - r * W;
      for (int i0 = tid; i0 < n; i0 += kNarrow * sk::kPoses) {
        float v[kNarrow], g[kNarrow];
#pragma unroll
        for (int u = 0; u < kNarrow; ++u) {
          const int i = i0 + u * sk::kPoses;
          if (i < n) {
            v[u] = gd[i];
            g[u] = lt[r * RS + c];
          }
          r += erow; c += ecol;
          if (c >= W) { c -= W; ++r; }
        }
#pragma unroll
        for (int u = 0; u < kNarrow; ++u) {
          const int i = i0 + u * sk::kPoses;
          if (i < n && g[u] != 0.f) gd[i] = v[u] + g[u];
        }
      }
    }
    __syncthreads();                                       // the next chunk is staged over these rows
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (tid == 0) part[blockIdx.x] = acc;
}

// lengths [B][K] of poses [B][J][G]: a thread per bone of a pose
template <int G, bool XF>
__global__ __launch_bounds__(NTHR) void bone_lengths_kernel(const float* __restrict__ poses, int64_t B, int J, int K,
                                                            const int32_t* __restrict__ child, const int32_t* __restrict__ parent,
                                                            const float* __restrict__ sub, const float* __restrict__ div,
                                                            float* __restrict__ out) {
  const int64_t n = B * K, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int64_t b = i / K;
    const int k = (int)(i - b * K);
    const int c = child[k], q = parent[k];
    const float* row = poses + b * J * G;
    float x[2 * G], d[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      x[g] = XF ? sk::raw1(row[c * G + g], sub[c * G + g], div[c * G + g]) : row[c * G + g];
      x[G + g] = XF ? sk::raw1(row[q * G + g], sub[q * G + g], div[q * G + g]) : row[q * G + g];
    }
    out[i] = sk::bone_len<G>(x, 0, 1, d);
  }
}

// (rho, G, has transform) -> f(integral constants): the one place a launch turns the run-time skeleton into types
template <class F>
int sk_dispatch(int rho, int G, bool xf, F&& f) {
  auto g = [&](auto R) {
    if (G == 2) return xf ? f(R, std::integral_constant<int, 2>{}, std::true_type{}) : f(R, std::integral_constant<int, 2>{}, std::false_type{});
    return xf ? f(R, std::integral_constant<int, 3>{}, std::true_type{}) : f(R, std::integral_constant<int, 3>{}, std::false_type{});
  };
  return rho == 0 ? g(std::integral_constant<int, 0>{}) : g(std::integral_constant<int, 1>{});
}

int check_bones(const PLSkeleton* s, int G, const char* who) {
  if (!s) PL_FAIL(PL_EINVAL, "%s: skeleton is NULL", who);
  if (G != 2 && G != 3) PL_FAIL(PL_ESHAPE, "%s: a skeleton takes joints of 2 or 3 coordinates, got %d", who, G);
  if (s->joints < 2 || s->joints > sk::kMaxJoints)
    PL_FAIL(PL_ESHAPE, "%s: skeleton joints=%d outside 2..%d", who, (int)s->joints, sk::kMaxJoints);
  if (s->bones < 1 || s->bones > sk::kMaxBones)
    PL_FAIL(PL_ESHAPE, "%s: skeleton bones=%d outside 1..%d", who, (int)s->bones, sk::kMaxBones);
  if (!s->bone_child || !s->bone_parent) PL_FAIL(PL_EINVAL, "%s: skeleton bone table is NULL", who);
  if ((s->sub != nullptr) != (s->div != nullptr)) PL_FAIL(PL_EINVAL, "%s: skeleton sub and div come together", who);
  return PL_OK;
}

}  // namespace

int skeleton_check(const PLSkeleton* s, int64_t O, int G, const char* who) {
  PL_TRY(check_bones(s, G, who));
  if ((int64_t)s->joints * G != O)
    PL_FAIL(PL_ESHAPE, "%s: a skeleton of %d joints of %d coordinates on %lld outputs", who, (int)s->joints, G, (long long)O);
  if (s->pairs < 0 || s->pairs > sk::kMaxPairs)
    PL_FAIL(PL_ESHAPE, "%s: skeleton pairs=%d outside 0..%d", who, (int)s->pairs, sk::kMaxPairs);
  if (s->pairs > 0 && (!s->pair_a || !s->pair_b)) PL_FAIL(PL_EINVAL, "%s: skeleton pair table is NULL", who);
  if (!s->term_weights) PL_FAIL(PL_EINVAL, "%s: skeleton term_weights is NULL", who);
  if (s->rho != 0 && s->rho != 1) PL_FAIL(PL_EINVAL, "%s: skeleton rho %d (0 = l1, 1 = mse)", who, (int)s->rho);
  return PL_OK;
}

int skeleton_partials(int64_t B) {
  const int64_t c = (B + sk::kPoses - 1) / sk::kPoses;
  return c > sk::kMaxGroups ? sk::kMaxGroups : (c < 1 ? 1 : (int)c);
}

int launch_skeleton_terms(const Crit& c, const float* pred, const float* tgt, int64_t B, int64_t O, float grad_scale, float inv_n,
                          float* dpred, float* part, void* stream, const char* who) {
  if (!c.has_sk) PL_FAIL(PL_EINVAL, "%s: no skeleton", who);
  if (!pred || !tgt || !part) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (B <= 0 || B > INT32_MAX || O != (int64_t)c.sk.joints * c.G) PL_FAIL(PL_ESHAPE, "%s: B=%lld O=%lld", who, (long long)B, (long long)O);
  const PLSkeleton& s = c.sk;
  SkArgs a = {s.joints, s.bones, s.pairs, s.bone_child, s.bone_parent, s.pair_a, s.pair_b, s.term_weights, s.sub, s.div,
              sk::consts(B, s.bones, s.pairs, grad_scale, inv_n)};
  const int RS = (s.joints * c.G) | 1, KS = s.bones | 1;
  const size_t lds = (size_t)sk::kPoses * (2 * RS + 2 * KS) * sizeof(float);       // 65,536 B at J = 32, G = 3, K = 31
  const dim3 grid(skeleton_partials(B)), block(sk::kPoses);
  sk_dispatch(s.rho, c.G, s.sub != nullptr, [&](auto R, auto G, auto X) {
    hipLaunchKernelGGL((skeleton_terms_kernel<decltype(R)::value, decltype(G)::value, decltype(X)::value>), grid, block, lds,
                       (hipStream_t)stream, pred, tgt, B, a, dpred, part);
    return 0;
  });
  PL_CHECK_LAUNCH("skeleton_terms");
  return PL_OK;
}

}  // namespace pl

using namespace pl;

extern "C" int pl_bone_lengths(const float* poses, int64_t B, int32_t group, const PLSkeleton* s, float* lengths, void* stream) {
  PL_TRY(check_bones(s, group, "pl_bone_lengths"));
  if (!poses || !lengths) PL_FAIL(PL_EINVAL, "pl_bone_lengths: null pointer");
  if (B <= 0 || B > INT32_MAX) PL_FAIL(PL_ESHAPE, "pl_bone_lengths: B=%lld outside 1..2^31-1", (long long)B);
  int64_t blocks = (B * s->bones + NTHR - 1) / NTHR;
  if (blocks > 1024) blocks = 1024;
  sk_dispatch(0, group, s->sub != nullptr, [&](auto, auto G, auto X) {
    hipLaunchKernelGGL((bone_lengths_kernel<decltype(G)::value, decltype(X)::value>), dim3((unsigned)blocks), dim3(NTHR), 0,
                       (hipStream_t)stream, poses, B, (int)s->joints, (int)s->bones, s->bone_child, s->bone_parent, s->sub, s->div,
                       lengths);
    return 0;
  });
  PL_CHECK_LAUNCH("bone_lengths");
  return PL_OK;
}

extern "C" int pl_skeleton_terms_host(const float* pred, const float* tgt, int64_t B, int32_t group, const PLSkeleton* s,
                                      float grad_scale, float* dpred, float* loss, float* lengths) {
  const char* who = "pl_skeleton_terms_host";
  if (!s) PL_FAIL(PL_EINVAL, "%s: skeleton is NULL", who);
  PL_TRY(skeleton_check(s, (int64_t)s->joints * group, group, who));
  if (!pred || !tgt || !loss) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (B <= 0 || B > INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: B=%lld outside 1..2^31-1", who, (long long)B);
  const int W = s->joints * group, K = s->bones;
  const sk::Consts c = sk::consts(B, K, s->pairs, grad_scale, 1.0f);
  const float lam_b = s->term_weights[0], lam_s = s->term_weights[1];
  const float wb = lam_b * c.cb, ws = lam_s * c.cs, lwb = lam_b * c.lb, lws = lam_s * c.ls;
  const sk::Tables T = {K, s->pairs, s->bone_child, s->bone_parent, s->pair_a, s->pair_b, s->div};
  double total = 0.0;
  sk_dispatch(s->rho, group, s->sub != nullptr, [&](auto R, auto G, auto X) {
    constexpr bool XF = decltype(X)::value;
    float p[3 * sk::kMaxJoints], t[3 * sk::kMaxJoints], lh[sk::kMaxBones], u[sk::kMaxBones];
    for (int64_t b = 0; b < B; ++b) {
      for (int i = 0; i < W; ++i) {
        p[i] = XF ? sk::raw1(pred[b * W + i], s->sub[i], s->div[i]) : pred[b * W + i];
        t[i] = XF ? sk::raw1(tgt[b * W + i], s->sub[i], s->div[i]) : tgt[b * W + i];
      }
      total += (double)sk::pose_terms<decltype(R)::value, decltype(G)::value, XF>(p, t, lh, u, W, T, wb, ws, lwb, lws,
                                                                                  dpred != nullptr);
      if (dpred)
        for (int i = 0; i < W; ++i)
          if (t[i] != 0.f) dpred[b * W + i] += t[i];
      if (lengths) memcpy(lengths + b * K, lh, K * sizeof(float));
    }
    return 0;
  });
  loss[0] = (float)total;
  return PL_OK;
}

extern "C" size_t pl_skeleton_abi_bytes(int which) {
  return which == 0 ? sizeof(PLCriterion) : which == 1 ? sizeof(PLSkeleton) : which == 2 ? sizeof(PLSkeletonCriterion) : 0;
}

extern "C" size_t pl_criterion_abi_bytes(int which) {
  return which == 3 ? sizeof(PLRowWeightsCriterion) : which >= 0 && which < 3 ? pl_skeleton_abi_bytes(which) : 0;
}

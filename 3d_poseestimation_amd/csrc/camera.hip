// Cameras on the device (camera.py): projection, its backward, per-joint reprojection errors, the reprojection loss with its
// gradient, and the per-pose root translation fitted to a 2-D track.  camera.h has the definitions; the _host entry points
// run the same text.  Nothing here reads or writes wider than 4 bytes: rows are 3 J, 2 J and J floats and a caller's tensor
// may start anywhere.
#include "camera.h"
#include "pl_internal.h"

#pragma clang fp contract(off)

namespace pl {
namespace {

constexpr int CM_THREADS = 256;

// what the loss reads besides the scene
struct LossArgs {
  const float* w;           // [B][J] or nullptr
  int kind;
  float div_w, div_h, coef;
};

// One lane per (pose, joint): two floats out.
__global__ __launch_bounds__(CM_THREADS) void camera_project_kernel(const float* __restrict__ X, int64_t B, int J, cm::Scene s,
                                                                    float* __restrict__ uv) {
  const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
  if (i >= B * J) return;
  const int64_t b = i / J;
  cm::Cam c;
  cm::pose_cam(s, b, &c);
  float o[2];
  cm::project_joint(s, c, X, J, b, (int)(i - b * J), o, nullptr, nullptr);
  uv[2 * i] = o[0];
  uv[2 * i + 1] = o[1];
}

// One lane per (pose, joint): one float out.
__global__ __launch_bounds__(CM_THREADS) void camera_reproj_errors_kernel(const float* __restrict__ X,
                                                                          const float* __restrict__ tgt, int64_t B, int J,
                                                                          cm::Scene s, float div_w, float div_h,
                                                                          float* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * CM_THREADS + threadIdx.x;
  if (i >= B * J) return;
  const int64_t b = i / J;
  cm::Cam c;
  cm::pose_cam(s, b, &c);
  float o[2], du, dv;
  cm::project_joint(s, c, X, J, b, (int)(i - b * J), o, nullptr, nullptr);
  cm::residual(o, tgt + 2 * i, div_w, div_h, &du, &dv);
  err[i] = cm::pixel_error(du, dv);
}

// A workgroup owns P = 256 / J whole poses, lane l < P J the joint at float offset (tile P J + l) of the arrays, so every
// access is a contiguous piece.  kLoss: (du_bar, dv_bar) come from the loss and the joint's value is reduced too; else
// they are the incoming duv.  Per joint: dX.  Per pose (dT != nullptr / kLoss): the joints' g and value leave through LDS
// and lane p < P adds pose p's in joint order (in fp64, g rounded to fp32 once); lane 0 then adds the poses' values in pose
// order into part[tile].
template <bool kLoss>
__global__ __launch_bounds__(cm::kTileThreads) void camera_bwd_tile_kernel(const float* __restrict__ X,
                                                                           const float* __restrict__ duv_or_tgt, int64_t B, int J,
                                                                           cm::Scene s, LossArgs a, float* __restrict__ dX,
                                                                           float* __restrict__ dT, double* __restrict__ part) {
  __shared__ float sm[4][cm::kTileThreads];
  __shared__ double ps[cm::kTileThreads];
  const int tid = threadIdx.x, P = cm::tile_poses(J);
  const int pl = tid / J;
  const int64_t b0 = (int64_t)blockIdx.x * P, b = b0 + pl;
  const bool on = pl < P && b < B;
  float v = 0.f, g[3] = {0.f, 0.f, 0.f};
  if (on) {
    const int j = tid - pl * J;
    const int64_t i = b * J + j;
    cm::Cam c;
    cm::pose_cam(s, b, &c);
    float o[2], ju[3], jv[3], ub, vb;
    cm::project_joint(s, c, X, J, b, j, o, ju, jv);
    if constexpr (kLoss) {
      float du, dv;
      cm::residual(o, duv_or_tgt + 2 * i, a.div_w, a.div_h, &du, &dv);
      v = cm::joint_loss(a.kind, du, dv, a.w ? a.w + i : nullptr, a.coef, a.div_w, a.div_h, &ub, &vb);
    } else {
      ub = duv_or_tgt[2 * i];
      vb = duv_or_tgt[2 * i + 1];
    }
    cm::joint_grad(ub, vb, ju, jv, g);
    if (dX) {
      float dx[3];
      cm::chain_point(s, j, g, dx);
      dX[3 * i] = dx[0];
      dX[3 * i + 1] = dx[1];
      dX[3 * i + 2] = dx[2];
    }
  }
  if (!kLoss && !dT) return;
  sm[0][tid] = v;
  if (dT) {
    sm[1][tid] = g[0];
    sm[2][tid] = g[1];
    sm[3][tid] = g[2];
  }
  __syncthreads();
  if (tid < P && b0 + tid < B) {
    const int base = tid * J;
    if (dT) {
      for (int d = 0; d < 3; ++d) {
        double acc = 0.0;
        for (int j = 0; j < J; ++j) acc = acc + (double)sm[1 + d][base + j];
        dT[3 * (b0 + tid) + d] = (float)acc;
      }
    }
    if constexpr (kLoss) {
      double acc = 0.0;
      for (int j = 0; j < J; ++j) acc = acc + (double)sm[0][base + j];
      ps[tid] = acc;
    }
  }
  if constexpr (kLoss) {
    __syncthreads();
    if (tid == 0) {
      const int np = B - b0 < P ? (int)(B - b0) : P;
      double acc = 0.0;
      for (int p = 0; p < np; ++p) acc = acc + ps[p];
      part[blockIdx.x] = acc;
    }
  }
}

// loss = final_sum(part) / elements (camera.h), fp64, rounded to fp32 once.  Eight partials are loaded before they are added,
// in the same order.
constexpr int kFinalLoads = 8;
__global__ __launch_bounds__(cm::kFinalThreads) void camera_loss_final_kernel(const double* __restrict__ part, int64_t np,
                                                                               double elements, float* __restrict__ loss) {
  __shared__ double sm[cm::kFinalThreads];
  const int tid = threadIdx.x;
  double acc = 0.0;
  int64_t i = tid;
  for (; i + (int64_t)(kFinalLoads - 1) * cm::kFinalThreads < np; i += (int64_t)kFinalLoads * cm::kFinalThreads) {
    double v[kFinalLoads];
#pragma unroll
    for (int u = 0; u < kFinalLoads; ++u) v[u] = part[i + (int64_t)u * cm::kFinalThreads];
#pragma unroll
    for (int u = 0; u < kFinalLoads; ++u) acc = acc + v[u];
  }
  for (; i < np; i += cm::kFinalThreads) acc = acc + part[i];
  sm[tid] = acc;
  __syncthreads();
  for (int h = cm::kFinalThreads / 2; h > 0; h >>= 1) {
    if (tid < h) sm[tid] = sm[tid] + sm[tid + h];
    __syncthreads();
  }
  if (tid == 0) loss[0] = (float)(sm[0] / elements);
}

// A workgroup of one wave owns 64 consecutive poses, a lane a pose.  The poses' rows of X (through the transform), of the
// target and of the weights are brought into LDS as they lie in memory -- consecutive lanes on consecutive floats -- into
// rows of odd stride, then every lane walks its own row: (iters + 2) passes over its joints, all out of LDS.
__global__ __launch_bounds__(cm::kFitPoses) void camera_fit_kernel(const float* __restrict__ X, const float* __restrict__ tgt,
                                                                   const float* __restrict__ w, int64_t B, int J, cm::Scene s,
                                                                   int iters, float* __restrict__ t, float* __restrict__ rms) {
  extern __shared__ __align__(16) float lds[];
  const int lane = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * cm::kFitPoses;
  const int np = B - b0 < cm::kFitPoses ? (int)(B - b0) : cm::kFitPoses;
  const int sq = cm::odd_stride(3 * J), su = cm::odd_stride(2 * J), sw = cm::odd_stride(J);
  float* qs = lds;
  float* us = qs + cm::kFitPoses * sq;
  float* ws = us + cm::kFitPoses * su;
  {
    // element e = lane, lane + 64, ... of a piece of np rows of W floats goes to row e / W, column e % W: (row, column) are
    // stepped, not divided
    auto stage = [&](const float* src, int W, int stride, float* dst, bool points) {
      const int n = np * W, q64 = cm::kFitPoses / W, r64 = cm::kFitPoses % W;
      int row = lane / W, col = lane % W;
      for (int e = lane; e < n; e += cm::kFitPoses) {
        float v = src[e];
        if (points && s.sub) v = pt::invert1(v, s.sub[col], s.div[col]);
        dst[row * stride + col] = v;
        row += q64;
        col += r64;
        if (col >= W) {
          col -= W;
          ++row;
        }
      }
    };
    stage(X + b0 * (3 * J), 3 * J, sq, qs, true);
    stage(tgt + b0 * (2 * J), 2 * J, su, us, false);
    if (w) stage(w + b0 * J, J, sw, ws, false);
  }
  __syncthreads();
  if (lane >= np) return;
  const int64_t b = b0 + lane;
  cm::Cam c;
  float o[3], e;
  if (cm::pose_cam(s, b, &c)) {
    cm::fit_pose(c, qs + lane * sq, us + lane * su, w ? ws + lane * sw : nullptr, J, iters, o, &e);
  } else {
    o[0] = o[1] = o[2] = e = pt::nan_f();
  }
  t[3 * b] = o[0];
  t[3 * b + 1] = o[1];
  t[3 * b + 2] = o[2];
  rms[b] = e;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }

// the checks every entry shares, and the scene
int scene_args(const char* fn, const float* X, int64_t B, int64_t J, const float* cams, int64_t C, const int32_t* cam_ids,
               const float* t, const float* sub, const float* div, cm::Scene* s) {
  if (!X || !cams) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (B <= 0 || B > (int64_t)INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: B=%lld poses", fn, (long long)B);
  if (J < 1 || J > cm::kMaxJoints) PL_FAIL(PL_ESHAPE, "%s: J=%lld joints (1..%d)", fn, (long long)J, cm::kMaxJoints);
  if (C < 1 || C > (int64_t)INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: C=%lld cameras", fn, (long long)C);
  if ((sub != nullptr) != (div != nullptr)) PL_FAIL(PL_EINVAL, "%s: sub and div come together", fn);
  *s = cm::Scene{cams, (int)C, cam_ids, t, sub, div};
  return PL_OK;
}

int div_args(const char* fn, float div_w, float div_h) {
  if (!(div_w > 0.f) || !(div_h > 0.f) || !finite_f(div_w) || !finite_f(div_h))
    PL_FAIL(PL_EINVAL, "%s: div=(%g, %g) must be positive and finite", fn, (double)div_w, (double)div_h);
  return PL_OK;
}

int project_args(const char* fn, const float* X, int64_t B, int64_t J, const float* uv) {
  if (!uv) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (overlap(X, (size_t)(B * J) * 12, uv, (size_t)(B * J) * 8)) PL_FAIL(PL_EINVAL, "%s: the output overlaps the poses", fn);
  return PL_OK;
}

int bwd_args(const char* fn, const float* X, const float* duv, int64_t B, int64_t J, const float* t, const float* dX,
             const float* dT) {
  if (!duv || !dX) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (dT && !t) PL_FAIL(PL_EINVAL, "%s: dT without a translation", fn);
  const size_t n3 = (size_t)(B * J) * 12, n2 = (size_t)(B * J) * 8, nt = (size_t)B * 12;
  if (overlap(X, n3, dX, n3) || overlap(duv, n2, dX, n3) || overlap(X, n3, dT, nt) || overlap(duv, n2, dT, nt) ||
      overlap(dX, n3, dT, nt) || overlap(t, nt, dT, nt) || overlap(t, nt, dX, n3))
    PL_FAIL(PL_EINVAL, "%s: the outputs overlap an input or each other", fn);
  return PL_OK;
}

int errors_args(const char* fn, const float* X, const float* tgt, int64_t B, int64_t J, float div_w, float div_h,
                const float* err) {
  if (!tgt || !err) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  PL_TRY(div_args(fn, div_w, div_h));
  const size_t n3 = (size_t)(B * J) * 12, n2 = (size_t)(B * J) * 8, n1 = (size_t)(B * J) * 4;
  if (overlap(X, n3, err, n1) || overlap(tgt, n2, err, n1)) PL_FAIL(PL_EINVAL, "%s: the output overlaps an input", fn);
  return PL_OK;
}

int loss_args(const char* fn, const float* X, const float* tgt, int64_t B, int64_t J, const float* t, const float* w, int kind,
              float div_w, float div_h, float grad_scale, const float* dX, const float* dT, const float* loss,
              const void* scratch, LossArgs* a) {
  if (!tgt || !loss || !scratch) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (kind != cm::kL1 && kind != cm::kMse && kind != cm::kL2) PL_FAIL(PL_EINVAL, "%s: kind=%d", fn, kind);
  PL_TRY(div_args(fn, div_w, div_h));
  if (dT && !t) PL_FAIL(PL_EINVAL, "%s: dT without a translation", fn);
  if (dT && !dX) PL_FAIL(PL_EINVAL, "%s: dT without dX", fn);
  if ((uintptr_t)scratch & 7) PL_FAIL(PL_EINVAL, "%s: scratch not 8-byte aligned", fn);
  const size_t n3 = (size_t)(B * J) * 12, n2 = (size_t)(B * J) * 8, nt = (size_t)B * 12;
  if (overlap(X, n3, dX, n3) || overlap(tgt, n2, dX, n3) || overlap(X, n3, dT, nt) || overlap(tgt, n2, dT, nt) ||
      overlap(dX, n3, dT, nt) || overlap(t, nt, dT, nt) || overlap(t, nt, dX, n3) || overlap(w, (size_t)(B * J) * 4, dX, n3) ||
      overlap(w, (size_t)(B * J) * 4, dT, nt))
    PL_FAIL(PL_EINVAL, "%s: the outputs overlap an input or each other", fn);
  *a = LossArgs{w, kind, div_w, div_h, grad_scale / (float)(kind == cm::kL2 ? B * J : B * J * 2)};
  return PL_OK;
}

int fit_args(const char* fn, const float* X, const float* tgt, int64_t B, int64_t J, int iters, const float* t,
             const float* rms) {
  if (!tgt || !t || !rms) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (iters < 0 || iters > cm::kMaxIters) PL_FAIL(PL_EINVAL, "%s: iters=%d is outside 0..%d", fn, iters, cm::kMaxIters);
  const size_t n3 = (size_t)(B * J) * 12, n2 = (size_t)(B * J) * 8, nt = (size_t)B * 12, nr = (size_t)B * 4;
  if (overlap(X, n3, t, nt) || overlap(X, n3, rms, nr) || overlap(tgt, n2, t, nt) || overlap(tgt, n2, rms, nr) ||
      overlap(t, nt, rms, nr))
    PL_FAIL(PL_EINVAL, "%s: the outputs overlap an input or each other", fn);
  return PL_OK;
}

double loss_elements(int kind, int64_t B, int64_t J) { return (double)(kind == cm::kL2 ? B * J : B * J * 2); }

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + CM_THREADS - 1) / CM_THREADS); }

// the backward of a tile of poses on the host, in the kernel's order; returns the tile's partial
template <bool kLoss>
double bwd_tile_host(const float* X, const float* duv_or_tgt, int64_t B, int J, const cm::Scene& s, const LossArgs& a, float* dX,
                    float* dT, int64_t tile) {
  const int P = cm::tile_poses(J);
  const int64_t b0 = tile * P;
  double partial = 0.0;
  for (int p = 0; p < P && b0 + p < B; ++p) {
    const int64_t b = b0 + p;
    cm::Cam c;
    cm::pose_cam(s, b, &c);
    double value = 0.0, gt[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < J; ++j) {
      const int64_t i = b * J + j;
      float o[2], ju[3], jv[3], ub, vb, v = 0.f, g[3];
      cm::project_joint(s, c, X, J, b, j, o, ju, jv);
      if constexpr (kLoss) {
        float du, dv;
        cm::residual(o, duv_or_tgt + 2 * i, a.div_w, a.div_h, &du, &dv);
        v = cm::joint_loss(a.kind, du, dv, a.w ? a.w + i : nullptr, a.coef, a.div_w, a.div_h, &ub, &vb);
      } else {
        ub = duv_or_tgt[2 * i];
        vb = duv_or_tgt[2 * i + 1];
      }
      cm::joint_grad(ub, vb, ju, jv, g);
      if (dX) cm::chain_point(s, j, g, dX + 3 * i);
      for (int d = 0; d < 3; ++d) gt[d] = gt[d] + (double)g[d];
      value = value + (double)v;
    }
    if (dT)
      for (int d = 0; d < 3; ++d) dT[3 * b + d] = (float)gt[d];
    partial = partial + value;
  }
  return partial;
}

// camera_loss_final_kernel's order on the host
float final_sum_host(const double* part, int64_t np, double elements) {
  static thread_local double sm[cm::kFinalThreads];
  for (int tid = 0; tid < cm::kFinalThreads; ++tid) {
    double acc = 0.0;
    for (int64_t i = tid; i < np; i += cm::kFinalThreads) acc = acc + part[i];
    sm[tid] = acc;
  }
  for (int h = cm::kFinalThreads / 2; h > 0; h >>= 1)
    for (int tid = 0; tid < h; ++tid) sm[tid] = sm[tid] + sm[tid + h];
  return (float)(sm[0] / elements);
}

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" int pl_camera_project(const float* X, int64_t B, int64_t J, const float* cams, int64_t C,
                                 const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                 const float* div_or_null, float* uv, void* stream) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_project", X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(project_args("pl_camera_project", X, B, J, uv));
  hipLaunchKernelGGL(camera_project_kernel, dim3(blocks_of(B * J)), dim3(CM_THREADS), 0, (hipStream_t)stream, X, B, (int)J, s, uv);
  PL_CHECK_LAUNCH("camera_project");
  return PL_OK;
}

extern "C" int pl_camera_project_host(const float* X, int64_t B, int64_t J, const float* cams, int64_t C,
                                      const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                      const float* div_or_null, float* uv) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_project_host", X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(project_args("pl_camera_project_host", X, B, J, uv));
  for (int64_t b = 0; b < B; ++b) {
    cm::Cam c;
    cm::pose_cam(s, b, &c);
    for (int j = 0; j < (int)J; ++j) cm::project_joint(s, c, X, (int)J, b, j, uv + 2 * (b * J + j), nullptr, nullptr);
  }
  return PL_OK;
}

extern "C" int pl_camera_project_bwd(const float* X, const float* duv, int64_t B, int64_t J, const float* cams, int64_t C,
                                     const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                     const float* div_or_null, float* dX, float* dT_or_null, void* stream) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_project_bwd", X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(bwd_args("pl_camera_project_bwd", X, duv, B, J, t_or_null, dX, dT_or_null));
  hipLaunchKernelGGL(camera_bwd_tile_kernel<false>, dim3((unsigned)cm::loss_tiles(B, (int)J)), dim3(cm::kTileThreads), 0,
                     (hipStream_t)stream, X, duv, B, (int)J, s, LossArgs{}, dX, dT_or_null, (double*)nullptr);
  PL_CHECK_LAUNCH("camera_project_bwd");
  return PL_OK;
}

extern "C" int pl_camera_project_bwd_host(const float* X, const float* duv, int64_t B, int64_t J, const float* cams, int64_t C,
                                          const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                          const float* div_or_null, float* dX, float* dT_or_null) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_project_bwd_host", X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(bwd_args("pl_camera_project_bwd_host", X, duv, B, J, t_or_null, dX, dT_or_null));
  for (int64_t tile = 0; tile < cm::loss_tiles(B, (int)J); ++tile)
    bwd_tile_host<false>(X, duv, B, (int)J, s, LossArgs{}, dX, dT_or_null, tile);
  return PL_OK;
}

extern "C" int pl_camera_reproj_errors(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                                       const int32_t* cam_ids_or_null, const float* t_or_null, const float* sub_or_null,
                                       const float* div_or_null, float div_w, float div_h, float* err, void* stream) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_reproj_errors", X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(errors_args("pl_camera_reproj_errors", X, target, B, J, div_w, div_h, err));
  hipLaunchKernelGGL(camera_reproj_errors_kernel, dim3(blocks_of(B * J)), dim3(CM_THREADS), 0, (hipStream_t)stream, X, target, B,
                     (int)J, s, div_w, div_h, err);
  PL_CHECK_LAUNCH("camera_reproj_errors");
  return PL_OK;
}

extern "C" int pl_camera_reproj_errors_host(const float* X, const float* target, int64_t B, int64_t J, const float* cams,
                                            int64_t C, const int32_t* cam_ids_or_null, const float* t_or_null,
                                            const float* sub_or_null, const float* div_or_null, float div_w, float div_h,
                                            float* err) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_reproj_errors_host", X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(errors_args("pl_camera_reproj_errors_host", X, target, B, J, div_w, div_h, err));
  for (int64_t b = 0; b < B; ++b) {
    cm::Cam c;
    cm::pose_cam(s, b, &c);
    for (int j = 0; j < (int)J; ++j) {
      const int64_t i = b * J + j;
      float o[2], du, dv;
      cm::project_joint(s, c, X, (int)J, b, j, o, nullptr, nullptr);
      cm::residual(o, target + 2 * i, div_w, div_h, &du, &dv);
      err[i] = cm::pixel_error(du, dv);
    }
  }
  return PL_OK;
}

extern "C" size_t pl_camera_reproj_loss_scratch_bytes(int64_t B, int64_t J) {
  if (B <= 0 || B > (int64_t)INT32_MAX || J < 1 || J > cm::kMaxJoints) return 0;
  return (size_t)cm::loss_tiles(B, (int)J) * sizeof(double);
}

extern "C" int pl_camera_reproj_loss_fwd_bwd(const float* X, const float* target, int64_t B, int64_t J, const float* cams,
                                             int64_t C, const int32_t* cam_ids_or_null, const float* t_or_null,
                                             const float* sub_or_null, const float* div_or_null, const float* weights_or_null,
                                             int kind, float div_w, float div_h, float grad_scale, float* dX_or_null,
                                             float* dT_or_null, float* loss, void* scratch, void* stream) {
  const char* fn = "pl_camera_reproj_loss_fwd_bwd";
  cm::Scene s;
  LossArgs a;
  PL_TRY(scene_args(fn, X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(loss_args(fn, X, target, B, J, t_or_null, weights_or_null, kind, div_w, div_h, grad_scale, dX_or_null, dT_or_null, loss,
                   scratch, &a));
  const int64_t tiles = cm::loss_tiles(B, (int)J);
  hipLaunchKernelGGL(camera_bwd_tile_kernel<true>, dim3((unsigned)tiles), dim3(cm::kTileThreads), 0, (hipStream_t)stream, X, target,
                     B, (int)J, s, a, dX_or_null, dT_or_null, (double*)scratch);
  PL_CHECK_LAUNCH("camera_reproj_loss");
  hipLaunchKernelGGL(camera_loss_final_kernel, dim3(1), dim3(cm::kFinalThreads), 0, (hipStream_t)stream, (const double*)scratch,
                     tiles, loss_elements(kind, B, J), loss);
  PL_CHECK_LAUNCH("camera_loss_final");
  return PL_OK;
}

extern "C" int pl_camera_reproj_loss_fwd_bwd_host(const float* X, const float* target, int64_t B, int64_t J, const float* cams,
                                                  int64_t C, const int32_t* cam_ids_or_null, const float* t_or_null,
                                                  const float* sub_or_null, const float* div_or_null,
                                                  const float* weights_or_null, int kind, float div_w, float div_h,
                                                  float grad_scale, float* dX_or_null, float* dT_or_null, float* loss,
                                                  void* scratch) {
  const char* fn = "pl_camera_reproj_loss_fwd_bwd_host";
  cm::Scene s;
  LossArgs a;
  PL_TRY(scene_args(fn, X, B, J, cams, C, cam_ids_or_null, t_or_null, sub_or_null, div_or_null, &s));
  PL_TRY(loss_args(fn, X, target, B, J, t_or_null, weights_or_null, kind, div_w, div_h, grad_scale, dX_or_null, dT_or_null, loss,
                   scratch, &a));
  const int64_t tiles = cm::loss_tiles(B, (int)J);
  double* part = (double*)scratch;
  for (int64_t tile = 0; tile < tiles; ++tile)
    part[tile] = bwd_tile_host<true>(X, target, B, (int)J, s, a, dX_or_null, dT_or_null, tile);
  loss[0] = final_sum_host(part, tiles, loss_elements(kind, B, J));
  return PL_OK;
}

extern "C" int pl_camera_fit_translation(const float* X, const float* target, int64_t B, int64_t J, const float* cams, int64_t C,
                                         const int32_t* cam_ids_or_null, const float* weights_or_null, const float* sub_or_null,
                                         const float* div_or_null, int iters, float* t, float* rms, void* stream) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_fit_translation", X, B, J, cams, C, cam_ids_or_null, nullptr, sub_or_null, div_or_null, &s));
  PL_TRY(fit_args("pl_camera_fit_translation", X, target, B, J, iters, t, rms));
  const int j = (int)J;
  const size_t lds = (size_t)cm::kFitPoses * (cm::odd_stride(3 * j) + cm::odd_stride(2 * j) + cm::odd_stride(j)) * sizeof(float);
  hipLaunchKernelGGL(camera_fit_kernel, dim3((unsigned)((B + cm::kFitPoses - 1) / cm::kFitPoses)), dim3(cm::kFitPoses), lds,
                     (hipStream_t)stream, X, target, weights_or_null, B, j, s, iters, t, rms);
  PL_CHECK_LAUNCH("camera_fit");
  return PL_OK;
}

extern "C" int pl_camera_fit_translation_host(const float* X, const float* target, int64_t B, int64_t J, const float* cams,
                                              int64_t C, const int32_t* cam_ids_or_null, const float* weights_or_null,
                                              const float* sub_or_null, const float* div_or_null, int iters, float* t,
                                              float* rms) {
  cm::Scene s;
  PL_TRY(scene_args("pl_camera_fit_translation_host", X, B, J, cams, C, cam_ids_or_null, nullptr, sub_or_null, div_or_null, &s));
  PL_TRY(fit_args("pl_camera_fit_translation_host", X, target, B, J, iters, t, rms));
  for (int64_t b = 0; b < B; ++b) {
    cm::Cam c;
    if (!cm::pose_cam(s, b, &c)) {
      t[3 * b] = t[3 * b + 1] = t[3 * b + 2] = rms[b] = pt::nan_f();
      continue;
    }
    float q[3 * cm::kMaxJoints];
    for (int j = 0; j < (int)J; ++j) cm::raw_point(s, X + (b * J + j) * 3, j, q + 3 * j);
    cm::fit_pose(c, q, target + b * J * 2, weights_or_null ? weights_or_null + b * J : nullptr, (int)J, iters, t + 3 * b, rms + b);
  }
  return PL_OK;
}

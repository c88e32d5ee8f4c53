// Pose tables on the device (pose_table.py): prepare (joint pick, camera view, root-centring), per-column statistics and
// the per-column transform.  pose_table.h has the definitions; the _host entry points run the same text.
#include "pose_table.h"
#include "pl_internal.h"

namespace pl {
namespace {

constexpr int PT_THREADS = 256;

// One thread per output joint (n, j): D consecutive floats, consecutive lanes consecutive joints.  Under root-centring a
// thread makes joint 0 of its row again (pick + camera view) and subtracts it: the row's 4 Jsrc D bytes are in the
// cache for all its J threads, and the fp64 quaternion products are far below what the loads cost.
__global__ __launch_bounds__(PT_THREADS) void pose_prepare_kernel(const float* __restrict__ raw, int64_t N,
                                                                  const int32_t* __restrict__ cam_id,
                                                                  const double* __restrict__ cams, float* __restrict__ out,
                                                                  pt::Prepare a) {
  const int64_t t = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
  if (t >= N * a.j) return;
  const int64_t n = t / a.j;
  const int j = (int)(t - n * a.j);
  float o[3];
  pt::prepare_joint(a, raw + n * a.jsrc * a.d, cams, a.has_cam ? cam_id[n] : 0, j, o);
  float* dst = out + t * a.d;
  for (int d = 0; d < a.d; ++d) dst[d] = o[d];
}

// ---- statistics: two passes of (per-chunk partials, one thread per column over the chunks); pose_table.h fixes the order ----
// Workgroup = one chunk of kChunkRows rows.  Thread t < H W is phase h = t / W of column c = t % W: the H W threads of an
// iteration read H whole rows, one contiguous piece.  Partials: part[chunk][3][W] fp64 (sum or squares, min, max).
template <bool SQ>
__global__ __launch_bounds__(pt::kStatThreads) void pose_stats_partial_kernel(const float* __restrict__ x, int64_t N, int W,
                                                                              const double* __restrict__ mean,
                                                                              double* __restrict__ part) {
  __shared__ double ss[pt::kStatThreads], slo[pt::kStatThreads], shi[pt::kStatThreads];
  const int H = pt::stat_phases(W), t = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * pt::kChunkRows, r1 = r0 + pt::kChunkRows < N ? r0 + pt::kChunkRows : N;
  if (t < H * W) {
    const int h = t / W, c = t - h * W;
    if constexpr (SQ) ss[t] = pt::phase_sq(x, r0, r1, W, H, h, c, mean[c]);
    else pt::phase_sum(x, r0, r1, W, H, h, c, &ss[t], &slo[t], &shi[t]);
  }
  __syncthreads();
  if (t < W) {
    double s = ss[t], lo = 0.0, hi = 0.0;
    if constexpr (!SQ) { lo = slo[t]; hi = shi[t]; }
    for (int h = 1; h < H; ++h) {
      s += ss[h * W + t];
      if constexpr (!SQ) { lo = pt::min_nan(lo, slo[h * W + t]); hi = pt::max_nan(hi, shi[h * W + t]); }
    }
    double* p = part + (size_t)blockIdx.x * 3 * W;
    p[t] = s;
    if constexpr (!SQ) { p[W + t] = lo; p[2 * W + t] = hi; }
  }
}

// One thread per column: the chunks in order.  out [4][W]: mean, std, min, max.
template <bool SQ>
__global__ void pose_stats_final_kernel(const double* __restrict__ part, int64_t nc, int W, int64_t N, double* __restrict__ out) {
  const int c = threadIdx.x;
  if (c >= W) return;
  double s = part[c], lo = 0.0, hi = 0.0;
  if constexpr (!SQ) { lo = part[W + c]; hi = part[2 * W + c]; }
  constexpr int U = 8;                                     // chunks loaded before they are added, in the same order
  int64_t k = 1;
  for (; k + U <= nc; k += U) {
    double vs[U], vlo[U], vhi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double* p = part + (size_t)(k + u) * 3 * W;
      vs[u] = p[c];
      if constexpr (!SQ) { vlo[u] = p[W + c]; vhi[u] = p[2 * W + c]; }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s += vs[u];
      if constexpr (!SQ) { lo = pt::min_nan(lo, vlo[u]); hi = pt::max_nan(hi, vhi[u]); }
    }
  }
  for (; k < nc; ++k) {
    const double* p = part + (size_t)k * 3 * W;
    s += p[c];
    if constexpr (!SQ) { lo = pt::min_nan(lo, p[W + c]); hi = pt::max_nan(hi, p[2 * W + c]); }
  }
  if constexpr (SQ) out[W + c] = pt::std_of(s, N);
  else { out[c] = pt::mean_of(s, lo, hi, N); out[2 * W + c] = lo; out[3 * W + c] = hi; }
}

// y = (x - sub) / div or x = y div + sub, one thread per element; in place allowed (an element is read once, by its writer)
template <bool INVERT>
__global__ __launch_bounds__(PT_THREADS) void pose_affine_kernel(const float* x, int64_t n, int W, const float* __restrict__ sub,
                                                                 const float* __restrict__ div, float* y) {
  const int64_t i = (int64_t)blockIdx.x * PT_THREADS + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % W);
  y[i] = INVERT ? pt::invert1(x[i], sub[c], div[c]) : pt::apply1(x[i], sub[c], div[c]);
}

int prepare_args(const char* fn, const float* raw, int64_t N, int64_t Jsrc, int64_t D, const int32_t* pick, int64_t J,
                 const int32_t* cam_id, const double* cams, int64_t C, int zero_centre, const float* out, pt::Prepare* a) {
  if (!raw || !out) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (N <= 0 || (D != 2 && D != 3) || Jsrc < 1 || Jsrc > pt::kMaxSrcJoints || J < 1 || J > pt::kMaxJoints ||
      N > INT64_MAX / (4 * pt::kMaxSrcJoints * 3))
    PL_FAIL(PL_ESHAPE, "%s: N=%lld Jsrc=%lld J=%lld D=%lld", fn, (long long)N, (long long)Jsrc, (long long)J, (long long)D);
  if (!pick && J != Jsrc) PL_FAIL(PL_ESHAPE, "%s: no joint list, yet J=%lld differs from Jsrc=%lld", fn, (long long)J, (long long)Jsrc);
  if ((cams != nullptr) != (cam_id != nullptr)) PL_FAIL(PL_EINVAL, "%s: cameras and cam_id come together", fn);
  if (cams && D != 3) PL_FAIL(PL_ESHAPE, "%s: the camera view is for D = 3, got D=%lld", fn, (long long)D);
  if (cams && (C < 1 || C > INT32_MAX)) PL_FAIL(PL_ESHAPE, "%s: C=%lld cameras", fn, (long long)C);
  const uintptr_t r0 = (uintptr_t)raw, r1 = r0 + (uintptr_t)(N * Jsrc * D * 4), o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)(N * J * D * 4);
  if (r0 < o1 && o0 < r1) PL_FAIL(PL_EINVAL, "%s: the output overlaps the raw table", fn);
  *a = pt::Prepare{(int)Jsrc, (int)J, (int)D, pick != nullptr, cams != nullptr, zero_centre != 0, (int)C, {}};
  for (int64_t j = 0; pick && j < J; ++j) {
    if (pick[j] < 0 || pick[j] >= Jsrc) PL_FAIL(PL_ESHAPE, "%s: pick[%lld]=%d is outside [0, %lld)", fn, (long long)j, (int)pick[j], (long long)Jsrc);
    a->pick[j] = (uint8_t)pick[j];
  }
  return PL_OK;
}

int stats_args(const char* fn, const float* x, int64_t N, int64_t W, const double* out) {
  if (!x || !out) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (N <= 0 || W < 1 || W > pt::kMaxCols || N > (int64_t)INT32_MAX * (pt::kChunkRows / 2))
    PL_FAIL(PL_ESHAPE, "%s: N=%lld W=%lld (W in 1..%d)", fn, (long long)N, (long long)W, pt::kMaxCols);
  if ((uintptr_t)out & 7) PL_FAIL(PL_EINVAL, "%s: the record is not 8-byte aligned", fn);
  return PL_OK;
}

int affine_args(const char* fn, const float* x, int64_t N, int64_t W, const float* sub, const float* div, const float* y) {
  if (!x || !sub || !div || !y) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (N <= 0 || W < 1 || W > pt::kMaxCols || N > (int64_t)INT32_MAX * 2)
    PL_FAIL(PL_ESHAPE, "%s: N=%lld W=%lld (W in 1..%d)", fn, (long long)N, (long long)W, pt::kMaxCols);
  if (x != y) {
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)(N * W * 4), y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)(N * W * 4);
    if (x0 < y1 && y0 < x1) PL_FAIL(PL_EINVAL, "%s: y overlaps x without being x", fn);
  }
  return PL_OK;
}

int64_t stat_chunks(int64_t N) { return (N + pt::kChunkRows - 1) / pt::kChunkRows; }

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" int pl_pose_prepare(const float* raw, int64_t N, int64_t Jsrc, int64_t D, const int32_t* pick, int64_t J,
                               const int32_t* cam_id, const double* cameras, int64_t C, int zero_centre, float* out,
                               void* stream) {
  pt::Prepare a;
  PL_TRY(prepare_args("pl_pose_prepare", raw, N, Jsrc, D, pick, J, cam_id, cameras, C, zero_centre, out, &a));
  const int64_t threads = N * J;
  if ((threads + PT_THREADS - 1) / PT_THREADS > INT32_MAX) PL_FAIL(PL_ESHAPE, "pl_pose_prepare: table too large");
  hipLaunchKernelGGL(pose_prepare_kernel, dim3((unsigned)((threads + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0,
                     (hipStream_t)stream, raw, N, cam_id, cameras, out, a);
  PL_CHECK_LAUNCH("pose_prepare");
  return PL_OK;
}

extern "C" int pl_pose_prepare_host(const float* raw, int64_t N, int64_t Jsrc, int64_t D, const int32_t* pick, int64_t J,
                                    const int32_t* cam_id, const double* cameras, int64_t C, int zero_centre, float* out) {
  pt::Prepare a;
  PL_TRY(prepare_args("pl_pose_prepare_host", raw, N, Jsrc, D, pick, J, cam_id, cameras, C, zero_centre, out, &a));
  for (int64_t n = 0; n < N; ++n)
    for (int j = 0; j < a.j; ++j)
      pt::prepare_joint(a, raw + n * a.jsrc * a.d, cameras, a.has_cam ? cam_id[n] : 0, j, out + (n * a.j + j) * a.d);
  return PL_OK;
}

extern "C" int64_t pl_pose_stats_chunk_rows(void) { return pt::kChunkRows; }

extern "C" size_t pl_pose_stats_scratch_bytes(int64_t N, int64_t W) {
  if (N <= 0 || W < 1 || W > pt::kMaxCols) return 0;
  return (size_t)stat_chunks(N) * 3 * (size_t)W * sizeof(double);
}

extern "C" int pl_pose_stats(const float* x, int64_t N, int64_t W, double* out, void* scratch, void* stream) {
  PL_TRY(stats_args("pl_pose_stats", x, N, W, out));
  if (!scratch || ((uintptr_t)scratch & 7)) PL_FAIL(PL_EINVAL, "pl_pose_stats: scratch is null or not 8-byte aligned");
  const int64_t nc = stat_chunks(N);
  double* part = (double*)scratch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(pose_stats_partial_kernel<false>, dim3((unsigned)nc), dim3(pt::kStatThreads), 0, s, x, N, (int)W,
                     (const double*)nullptr, part);
  PL_CHECK_LAUNCH("pose_stats_partial");
  hipLaunchKernelGGL(pose_stats_final_kernel<false>, dim3(1), dim3(128), 0, s, (const double*)part, nc, (int)W, N, out);
  PL_CHECK_LAUNCH("pose_stats_final");
  hipLaunchKernelGGL(pose_stats_partial_kernel<true>, dim3((unsigned)nc), dim3(pt::kStatThreads), 0, s, x, N, (int)W,
                     (const double*)out, part);
  PL_CHECK_LAUNCH("pose_stats_partial_sq");
  hipLaunchKernelGGL(pose_stats_final_kernel<true>, dim3(1), dim3(128), 0, s, (const double*)part, nc, (int)W, N, out);
  PL_CHECK_LAUNCH("pose_stats_final_sq");
  return PL_OK;
}

extern "C" int pl_pose_stats_host(const float* x, int64_t N, int64_t W_, double* out) {
  PL_TRY(stats_args("pl_pose_stats_host", x, N, W_, out));
  const int W = (int)W_, H = pt::stat_phases(W);
  const int64_t nc = stat_chunks(N);
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < W; ++c) {
      double s = 0.0, lo = 0.0, hi = 0.0;
      for (int64_t k = 0; k < nc; ++k) {
        const int64_t r0 = k * pt::kChunkRows, r1 = r0 + pt::kChunkRows < N ? r0 + pt::kChunkRows : N;
        double cs = 0.0, clo = 0.0, chi = 0.0;
        for (int h = 0; h < H; ++h) {
          double ps, plo = 0.0, phi = 0.0;
          if (pass) ps = pt::phase_sq(x, r0, r1, W, H, h, c, out[c]);
          else pt::phase_sum(x, r0, r1, W, H, h, c, &ps, &plo, &phi);
          if (h == 0) { cs = ps; clo = plo; chi = phi; }
          else { cs += ps; clo = pt::min_nan(clo, plo); chi = pt::max_nan(chi, phi); }
        }
        if (k == 0) { s = cs; lo = clo; hi = chi; }
        else { s += cs; lo = pt::min_nan(lo, clo); hi = pt::max_nan(hi, chi); }
      }
      if (pass) out[W + c] = pt::std_of(s, N);
      else { out[c] = pt::mean_of(s, lo, hi, N); out[2 * W + c] = lo; out[3 * W + c] = hi; }
    }
  return PL_OK;
}

extern "C" int pl_pose_affine(const float* x, int64_t N, int64_t W, const float* sub, const float* div, int invert, float* y,
                              void* stream) {
  PL_TRY(affine_args("pl_pose_affine", x, N, W, sub, div, y));
  const int64_t n = N * W;
  const dim3 grid((unsigned)((n + PT_THREADS - 1) / PT_THREADS)), block(PT_THREADS);
  if (invert) hipLaunchKernelGGL(pose_affine_kernel<true>, grid, block, 0, (hipStream_t)stream, x, n, (int)W, sub, div, y);
  else hipLaunchKernelGGL(pose_affine_kernel<false>, grid, block, 0, (hipStream_t)stream, x, n, (int)W, sub, div, y);
  PL_CHECK_LAUNCH("pose_affine");
  return PL_OK;
}

extern "C" int pl_pose_affine_host(const float* x, int64_t N, int64_t W, const float* sub, const float* div, int invert,
                                   float* y) {
  PL_TRY(affine_args("pl_pose_affine_host", x, N, W, sub, div, y));
  for (int64_t i = 0; i < N * W; ++i) {
    const int c = (int)(i % W);
    y[i] = invert ? pt::invert1(x[i], sub[c], div[c]) : pt::apply1(x[i], sub[c], div[c]);
  }
  return PL_OK;
}

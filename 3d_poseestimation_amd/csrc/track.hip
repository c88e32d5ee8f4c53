// Video tracks on the device (sequence.py): joint remap, track preparation (scale, validity, gap fill), the
// confidence-weighted temporal FIR and the velocity / acceleration errors.  track.h has the definitions; the _host entry
// points run the same text.
#include "track.h"
#include "pl_internal.h"

namespace pl {
namespace {

constexpr int TK_THREADS = 256;
constexpr int kTileFrames = 64;                 // frames of a filter workgroup; halved where tile + halo would pass kTileLdsBytes
constexpr size_t kTileLdsBytes = 60 * 1024;

// One thread per (t, j) of the H36M-17 row: three floats.
__global__ __launch_bounds__(TK_THREADS) void track_remap_kernel(const float* __restrict__ det, int64_t T, int layout,
                                                                 float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= T * tk::kJoints) return;
  const int64_t t = i / tk::kJoints;
  float o[3];
  tk::remap_joint(det + t * (tk::kJoints * 3), layout, (int)(i - t * tk::kJoints), o);
  out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

// One thread per (t, j).  A valid sample (nine in ten on recorded tracks) costs its own row's sources; an invalid one walks
// up to G frames each way through rows its neighbours in the wave are reading too.
__global__ __launch_bounds__(TK_THREADS) void track_prepare_kernel(const float* __restrict__ det, int64_t T,
                                                                   const int32_t* __restrict__ seq, float* __restrict__ xy,
                                                                   float* __restrict__ w, uint8_t* __restrict__ state,
                                                                   tk::Prepare a) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= T * tk::kJoints) return;
  const int64_t t = i / tk::kJoints;
  float o[2], ww;
  uint8_t st;
  tk::prepare_joint(a, det, seq, T, t, (int)(i - t * tk::kJoints), o, &ww, &st);
  xy[2 * i] = o[0]; xy[2 * i + 1] = o[1];
  w[i] = ww;
  state[i] = st;
}

// A workgroup owns tf consecutive frames and all W = J D columns.  It brings rows [t0 - h, t0 + tf + h) of x (and of w, and
// of seq) into LDS as they lie in memory -- one contiguous piece each, 4 bytes a lane: rows are 34 or 51 floats and a
// caller's tensor may start anywhere, so nothing wider is aligned -- then one thread per frame finds the frame's window
// inside its sequence, then one thread per (t, j) runs the taps out of LDS.  Thread i reads x at float (i D + d) + o W of
// the image: for D = 3 a stride coprime with the banks.
template <int D>
__global__ __launch_bounds__(TK_THREADS) void track_filter_kernel(const float* __restrict__ x, int64_t T, int J,
                                                                  const float* __restrict__ w, const int32_t* __restrict__ seq,
                                                                  float* __restrict__ y, tk::Taps taps, int tf) {
  extern __shared__ __align__(16) float lds[];
  const int W = J * D, h = taps.k / 2, tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * tf;
  const int64_t t1 = t0 + tf < T ? t0 + tf : T;
  const int64_t r0 = t0 - h > 0 ? t0 - h : 0, r1 = t1 + h < T ? t1 + h : T;
  const int rows = (int)(r1 - r0), nf = (int)(t1 - t0), cap = tf + 2 * h;
  float* xs = lds;
  float* ws = xs + cap * W;
  int32_t* ss = (int32_t*)(ws + (w ? cap * J : 0));
  int* win = ss + (seq ? cap : 0);                           // [tf][2]
  {
    const float* gx = x + r0 * W;
    for (int i = tid; i < rows * W; i += TK_THREADS) xs[i] = gx[i];
    if (w) {
      const float* gw = w + r0 * J;
      for (int i = tid; i < rows * J; i += TK_THREADS) ws[i] = gw[i];
    }
    if (seq)
      for (int i = tid; i < rows; i += TK_THREADS) ss[i] = seq[r0 + i];
  }
  __syncthreads();
  if (tid < nf) {
    int lo, hi;
    tk::seq_window(seq ? ss : nullptr, r0, T, t0 + tid, h, &lo, &hi);
    win[2 * tid] = lo;
    win[2 * tid + 1] = hi;
  }
  __syncthreads();
  const int first = (int)(t0 - r0);
  for (int i = tid; i < nf * J; i += TK_THREADS) {
    const int tl = i / J, j = i - tl * J, row = first + tl;
    float o[D];
    tk::fir_joint<D>(xs + row * W + j * D, W, w ? ws + row * J + j : nullptr, J, taps, win[2 * tl], win[2 * tl + 1], o);
    float* dst = y + (t0 + tl) * W + j * D;
#pragma unroll
    for (int d = 0; d < D; ++d) dst[d] = o[d];
  }
}

// One thread per (t, j); the thread of joint 0 writes the frame's count.
__global__ __launch_bounds__(TK_THREADS) void track_velocity_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                    int64_t T, int J, const int32_t* __restrict__ seq, int order,
                                                                    const float* __restrict__ sub, const float* __restrict__ div,
                                                                    float* __restrict__ out, uint8_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * TK_THREADS + threadIdx.x;
  if (i >= T * J) return;
  const int64_t t = i / J;
  const int j = (int)(i - t * J);
  const bool has = tk::vel_has_stencil(seq, T, t, order);
  out[i] = has ? tk::vel_error(pred + 3 * i, tgt + 3 * i, 3 * J, order, sub, div, j) : 0.f;
  if (j == 0) count[t] = has ? 1 : 0;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

int frames_ok(const char* fn, int64_t T) {
  if (T <= 0 || T > (int64_t)INT32_MAX * 8) PL_FAIL(PL_ESHAPE, "%s: T=%lld frames", fn, (long long)T);
  return PL_OK;
}

int remap_args(const char* fn, const float* det, int64_t T, int layout, const float* out) {
  if (!det || !out) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  PL_TRY(frames_ok(fn, T));
  if (layout != tk::kLayoutCoco17 && layout != tk::kLayoutH36m17) PL_FAIL(PL_EINVAL, "%s: layout=%d", fn, layout);
  const size_t n = (size_t)T * tk::kJoints * 3 * 4;
  if (overlap(det, n, out, n)) PL_FAIL(PL_EINVAL, "%s: the output overlaps the detections", fn);
  return PL_OK;
}

int prepare_args(const char* fn, const float* det, int64_t T, int layout, float div_w, float div_h, float conf_thr, int max_gap,
                 float fill_conf, const float* xy, const float* w, const uint8_t* state, tk::Prepare* a) {
  if (!det || !xy || !w || !state) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  PL_TRY(frames_ok(fn, T));
  if (layout != tk::kLayoutCoco17 && layout != tk::kLayoutH36m17) PL_FAIL(PL_EINVAL, "%s: layout=%d", fn, layout);
  if (!(div_w > 0.f) || !(div_h > 0.f) || !tk::finite_f(div_w) || !tk::finite_f(div_h))
    PL_FAIL(PL_EINVAL, "%s: div=(%g, %g) must be positive and finite", fn, (double)div_w, (double)div_h);
  if (conf_thr != conf_thr) PL_FAIL(PL_EINVAL, "%s: conf_thr is NaN", fn);
  if (!(fill_conf >= 0.f) || !tk::finite_f(fill_conf)) PL_FAIL(PL_EINVAL, "%s: fill_conf=%g", fn, (double)fill_conf);
  if (max_gap < 0 || max_gap > tk::kMaxGap) PL_FAIL(PL_EINVAL, "%s: max_gap=%d is outside 0..%d", fn, max_gap, tk::kMaxGap);
  const size_t nd = (size_t)T * tk::kJoints * 3 * 4, nxy = (size_t)T * tk::kJoints * 2 * 4, nw = (size_t)T * tk::kJoints * 4,
               ns = (size_t)T * tk::kJoints;
  if (overlap(det, nd, xy, nxy) || overlap(det, nd, w, nw) || overlap(det, nd, state, ns) || overlap(xy, nxy, w, nw) ||
      overlap(xy, nxy, state, ns) || overlap(w, nw, state, ns))
    PL_FAIL(PL_EINVAL, "%s: the outputs overlap the detections or each other", fn);
  *a = tk::Prepare{layout, max_gap, div_w, div_h, conf_thr, fill_conf};
  return PL_OK;
}

int filter_tile_frames(int64_t J, int64_t D, int K) {
  const size_t cap = (size_t)kTileFrames + 2 * (size_t)(K / 2);
  return (cap * (size_t)(J * D + J + 1) + 2 * kTileFrames) * 4 <= kTileLdsBytes ? kTileFrames : kTileFrames / 2;
}

int filter_args(const char* fn, const float* x, int64_t T, int64_t J, int64_t D, const float* w, const float* taps, int K,
                const float* y, tk::Taps* tp) {
  if (!x || !y || !taps) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  PL_TRY(frames_ok(fn, T));
  if ((D != 2 && D != 3) || J < 1 || J > tk::kMaxJoints) PL_FAIL(PL_ESHAPE, "%s: J=%lld D=%lld", fn, (long long)J, (long long)D);
  if (K < 1 || K > tk::kMaxTaps || K % 2 == 0) PL_FAIL(PL_EINVAL, "%s: K=%d taps (odd, at most %d)", fn, K, tk::kMaxTaps);
  tp->k = K;
  for (int k = 0; k < tk::kMaxTaps; ++k) tp->v[k] = 0.f;
  for (int k = 0; k < K; ++k) {
    if (!(taps[k] >= 0.f) || !tk::finite_f(taps[k])) PL_FAIL(PL_EINVAL, "%s: taps[%d]=%g is negative or not finite", fn, k, (double)taps[k]);
    tp->v[k] = taps[k];
  }
  const size_t nx = (size_t)(T * J * D) * 4;
  if (overlap(x, nx, y, nx) || (w && overlap(w, (size_t)(T * J) * 4, y, nx)))
    PL_FAIL(PL_EINVAL, "%s: the output overlaps an input", fn);
  return PL_OK;
}

int velocity_args(const char* fn, const float* pred, const float* tgt, int64_t T, int64_t J, int order, const float* sub,
                  const float* div, const float* out, const uint8_t* count) {
  if (!pred || !tgt || !out || !count) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  PL_TRY(frames_ok(fn, T));
  if (J < 1 || J > tk::kMaxJoints) PL_FAIL(PL_ESHAPE, "%s: J=%lld", fn, (long long)J);
  if (order != 1 && order != 2) PL_FAIL(PL_EINVAL, "%s: order=%d", fn, order);
  if ((sub != nullptr) != (div != nullptr)) PL_FAIL(PL_EINVAL, "%s: sub and div come together", fn);
  const size_t np = (size_t)(T * J) * 12, no = (size_t)(T * J) * 4;
  if (overlap(pred, np, out, no) || overlap(tgt, np, out, no) || overlap(pred, np, count, (size_t)T) ||
      overlap(tgt, np, count, (size_t)T) || overlap(out, no, count, (size_t)T))
    PL_FAIL(PL_EINVAL, "%s: the outputs overlap an input or each other", fn);
  return PL_OK;
}

unsigned blocks_of(int64_t threads) { return (unsigned)((threads + TK_THREADS - 1) / TK_THREADS); }

template <int D>
void filter_host(const float* x, int64_t T, int J, const float* w, const int32_t* seq, const tk::Taps& tp, float* y) {
  const int W = J * D;
  for (int64_t t = 0; t < T; ++t) {
    int lo, hi;
    tk::seq_window(seq, 0, T, t, tp.k / 2, &lo, &hi);
    for (int j = 0; j < J; ++j)
      tk::fir_joint<D>(x + t * W + j * D, W, w ? w + t * J + j : nullptr, J, tp, lo, hi, y + t * W + j * D);
  }
}

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" int pl_track_remap(const float* det, int64_t T, int layout, float* out, void* stream) {
  PL_TRY(remap_args("pl_track_remap", det, T, layout, out));
  hipLaunchKernelGGL(track_remap_kernel, dim3(blocks_of(T * tk::kJoints)), dim3(TK_THREADS), 0, (hipStream_t)stream, det, T, layout,
                     out);
  PL_CHECK_LAUNCH("track_remap");
  return PL_OK;
}

extern "C" int pl_track_remap_host(const float* det, int64_t T, int layout, float* out) {
  PL_TRY(remap_args("pl_track_remap_host", det, T, layout, out));
  for (int64_t t = 0; t < T; ++t)
    for (int j = 0; j < tk::kJoints; ++j) tk::remap_joint(det + t * (tk::kJoints * 3), layout, j, out + (t * tk::kJoints + j) * 3);
  return PL_OK;
}

extern "C" int pl_track_prepare(const float* det, int64_t T, int layout, float div_w, float div_h, float conf_thr, int max_gap,
                                float fill_conf, const int32_t* seq_ids_or_null, float* xy, float* w, uint8_t* state,
                                void* stream) {
  tk::Prepare a;
  PL_TRY(prepare_args("pl_track_prepare", det, T, layout, div_w, div_h, conf_thr, max_gap, fill_conf, xy, w, state, &a));
  hipLaunchKernelGGL(track_prepare_kernel, dim3(blocks_of(T * tk::kJoints)), dim3(TK_THREADS), 0, (hipStream_t)stream, det, T,
                     seq_ids_or_null, xy, w, state, a);
  PL_CHECK_LAUNCH("track_prepare");
  return PL_OK;
}

extern "C" int pl_track_prepare_host(const float* det, int64_t T, int layout, float div_w, float div_h, float conf_thr,
                                     int max_gap, float fill_conf, const int32_t* seq_ids_or_null, float* xy, float* w,
                                     uint8_t* state) {
  tk::Prepare a;
  PL_TRY(prepare_args("pl_track_prepare_host", det, T, layout, div_w, div_h, conf_thr, max_gap, fill_conf, xy, w, state, &a));
  for (int64_t t = 0; t < T; ++t)
    for (int j = 0; j < tk::kJoints; ++j) {
      const int64_t i = t * tk::kJoints + j;
      tk::prepare_joint(a, det, seq_ids_or_null, T, t, j, xy + 2 * i, w + i, state + i);
    }
  return PL_OK;
}

extern "C" int pl_track_filter_tile_frames(int64_t J, int64_t D, int K) {
  if ((D != 2 && D != 3) || J < 1 || J > tk::kMaxJoints || K < 1 || K > tk::kMaxTaps) return 0;
  return filter_tile_frames(J, D, K);
}

extern "C" int pl_track_filter(const float* x, int64_t T, int64_t J, int64_t D, const float* w_or_null,
                               const int32_t* seq_ids_or_null, const float* taps, int K, float* y, void* stream) {
  tk::Taps tp;
  PL_TRY(filter_args("pl_track_filter", x, T, J, D, w_or_null, taps, K, y, &tp));
  const int tf = filter_tile_frames(J, D, K);
  const size_t cap = (size_t)tf + 2 * (size_t)(K / 2);
  const size_t lds = (cap * (size_t)(J * D + (w_or_null ? J : 0) + (seq_ids_or_null ? 1 : 0)) + 2 * (size_t)tf) * 4;
  const dim3 grid((unsigned)((T + tf - 1) / tf)), block(TK_THREADS);
  if (D == 3)
    hipLaunchKernelGGL(track_filter_kernel<3>, grid, block, lds, (hipStream_t)stream, x, T, (int)J, w_or_null, seq_ids_or_null, y,
                       tp, tf);
  else
    hipLaunchKernelGGL(track_filter_kernel<2>, grid, block, lds, (hipStream_t)stream, x, T, (int)J, w_or_null, seq_ids_or_null, y,
                       tp, tf);
  PL_CHECK_LAUNCH("track_filter");
  return PL_OK;
}

extern "C" int pl_track_filter_host(const float* x, int64_t T, int64_t J, int64_t D, const float* w_or_null,
                                    const int32_t* seq_ids_or_null, const float* taps, int K, float* y) {
  tk::Taps tp;
  PL_TRY(filter_args("pl_track_filter_host", x, T, J, D, w_or_null, taps, K, y, &tp));
  if (D == 3) filter_host<3>(x, T, (int)J, w_or_null, seq_ids_or_null, tp, y);
  else filter_host<2>(x, T, (int)J, w_or_null, seq_ids_or_null, tp, y);
  return PL_OK;
}

extern "C" int pl_track_velocity_errors(const float* pred, const float* tgt, int64_t T, int64_t J,
                                        const int32_t* seq_ids_or_null, int order, const float* sub_or_null,
                                        const float* div_or_null, float* out, uint8_t* count, void* stream) {
  PL_TRY(velocity_args("pl_track_velocity_errors", pred, tgt, T, J, order, sub_or_null, div_or_null, out, count));
  hipLaunchKernelGGL(track_velocity_kernel, dim3(blocks_of(T * J)), dim3(TK_THREADS), 0, (hipStream_t)stream, pred, tgt, T, (int)J,
                     seq_ids_or_null, order, sub_or_null, div_or_null, out, count);
  PL_CHECK_LAUNCH("track_velocity");
  return PL_OK;
}

extern "C" int pl_track_velocity_errors_host(const float* pred, const float* tgt, int64_t T, int64_t J,
                                             const int32_t* seq_ids_or_null, int order, const float* sub_or_null,
                                             const float* div_or_null, float* out, uint8_t* count) {
  PL_TRY(velocity_args("pl_track_velocity_errors_host", pred, tgt, T, J, order, sub_or_null, div_or_null, out, count));
  for (int64_t t = 0; t < T; ++t) {
    const bool has = tk::vel_has_stencil(seq_ids_or_null, T, t, order);
    count[t] = has ? 1 : 0;
    for (int64_t j = 0; j < J; ++j) {
      const int64_t i = t * J + j;
      out[i] = has ? tk::vel_error(pred + 3 * i, tgt + 3 * i, 3 * (int)J, order, sub_or_null, div_or_null, (int)j) : 0.f;
    }
  }
  return PL_OK;
}

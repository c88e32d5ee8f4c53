// The flat optimizer step: AdamW over the parameter arena with the clip record, the averaged (EMA) weights and the operand
// planes of the weights in the same launch; the weight <-> average swap; the device step counter.
//
// They replace, on the reference path, AdamW.step (train_1.py:39,96).
#include <algorithm>

#include "adamw.h"
#include "pl_internal.h"
#include "plane_store.h"
#include "streaming.h"

namespace pl {
namespace {

// ---- flat AdamW (torch single-tensor update order): AdamWIn, adamw_consts, adamw_one in adamw.h ---------
// CLIP: the step behind pl_grad_norm_clip (in.clip set).  A skipped step writes no p, m, v; it still writes the operand
// planes, from the unchanged parameters -- the host marks them current after every launch (optim.FlatAdamW._launch), and
// they may have been stale before it (load_state_dict).  CLIP = false is the kernel as it was.
// EMA: the averaged weights e (PLEma, the parameter arena's layout) follow from the registers that hold the new p -- float4
// beside p, m, v, the scalar tail likewise; a skipped step leaves e alone.  EMA = false takes an empty EmaArg and is the kernel
// as it was.
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(NTHR) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v,
                                                     int64_t n, AdamWIn in, int vec, EmaArg<EMA> ema) {
  if constexpr (CLIP) {
    if (in.clip->skip) {
      if (!in.nseg) return;
      const int64_t stride = (int64_t)gridDim.x * blockDim.x, n4 = n >> 2;
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        const int64_t e = 4 * i;
#pragma unroll 1
        for (int q = 0; q < in.nseg; ++q) {
          const int64_t r = e - in.seg_off[q];
          if (r >= 0 && r < in.seg_n[q]) {
            const PlaneDst d = {in.seg_h[q], in.seg_l[q], in.pscale, in.kind, 0, in.range, PL_RANGE_SITE_LIFTER_WEIGHT};
            store_planes4(d, (size_t)r, ld4(p + e));
            break;
          }
        }
      }
      return;
    }
  }
  const AdamWK k = [&] { if constexpr (CLIP) return adamw_consts_clip(in, in.clip); else return adamw_consts(in); }();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  float* __restrict__ e = nullptr;
  float omd = 0.f;
  if constexpr (EMA) {
    e = ema.v.e;
    omd = ema_omd(in, CLIP ? in.clip : nullptr, ema.v);
  }
  if (vec) {
    const int64_t n4 = n >> 2;
    for (; i < n4; i += stride) {
      float4 pv = ld4(p + 4 * i), mv = ld4(m + 4 * i), vv = ld4(v + 4 * i);
      const float4 gv = ld4(g + 4 * i);
      adamw_one(pv.x, gv.x, mv.x, vv.x, k);
      adamw_one(pv.y, gv.y, mv.y, vv.y, k);
      adamw_one(pv.z, gv.z, mv.z, vv.z, k);
      adamw_one(pv.w, gv.w, mv.w, vv.w, k);
      st4(p + 4 * i, pv); st4(m + 4 * i, mv); st4(v + 4 * i, vv);
      if constexpr (EMA) {
        float4 ev = ld4(e + 4 * i);
        ema_one(ev.x, pv.x, omd);
        ema_one(ev.y, pv.y, omd);
        ema_one(ev.z, pv.z, omd);
        ema_one(ev.w, pv.w, omd);
        st4(e + 4 * i, ev);
      }
      if (in.nseg) {                      // segment starts and lengths are multiples of 4: a float4 lies inside one
        const int64_t e = 4 * i;
#pragma unroll 1
        for (int q = 0; q < in.nseg; ++q) {
          const int64_t r = e - in.seg_off[q];
          if (r >= 0 && r < in.seg_n[q]) {
            const PlaneDst d = {in.seg_h[q], in.seg_l[q], in.pscale, in.kind, 0, in.range, PL_RANGE_SITE_LIFTER_WEIGHT};
            store_planes4(d, (size_t)r, pv);
            break;
          }
        }
      }
    }
    i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  }
  for (; i < n; i += stride) {
    adamw_one(p[i], g[i], m[i], v[i], k);
    if constexpr (EMA) ema_one(e[i], p[i], omd);
  }
}

// a <-> b over n floats, in place: float4 body, scalar tail (optim.FlatOptimizer.averaged_weights: parameters <-> their average)
__global__ __launch_bounds__(NTHR) void swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n, int vec) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (vec) {
    const int64_t n4 = n >> 2;
    for (; i < n4; i += stride) {
      const float4 av = ld4(a + 4 * i), bv = ld4(b + 4 * i);
      st4(a + 4 * i, bv); st4(b + 4 * i, av);
    }
    i = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  }
  for (; i < n; i += stride) {
    const float t = a[i];
    a[i] = b[i];
    b[i] = t;
  }
}

// (same-box sweep, B = 64 step: 256 / 512 / 1024 / 2048 blocks -> 0.1297 / 0.1289 / 0.1295 / 0.1304 ms; B = 4096: no difference)
constexpr int kAdamBlocks = 512;

// PLAdamWPlanes (NULL or no segment: nothing) -> the plane fields of a.in, checked against a's arenas
int adamw_planes(const PLAdamWPlanes* planes, AdamWArgs& a) {
  if (!planes || planes->nseg <= 0) return PL_OK;
  AdamWIn& in = a.in;
  if (planes->nseg > PL_ADAMW_MAX_SEGS || (planes->kind != 1 && planes->kind != 2) || !(planes->scale > 0.f))
    PL_FAIL(PL_EINVAL, "pl_adamw_flat_planes: bad plane description");
  if (!(aligned16(a.p) && aligned16(a.g) && aligned16(a.m) && aligned16(a.v)) || (a.n & 3))
    PL_FAIL(PL_EINVAL, "pl_adamw_flat_planes: arenas must be 16-byte aligned, n %% 4 == 0");
  in.nseg = planes->nseg; in.kind = planes->kind; in.pscale = planes->scale;
  in.range = planes->kind == 2 ? range_record() : nullptr;
  for (int q = 0; q < planes->nseg; ++q) {
    const PLAdamWSeg& sg = planes->seg[q];
    if (sg.offset < 0 || sg.numel <= 0 || (sg.offset & 3) || (sg.numel & 3) || sg.offset + sg.numel > a.n || !sg.h ||
        (planes->kind == 2 && !sg.l) || (reinterpret_cast<uintptr_t>(sg.h) & 7) || (reinterpret_cast<uintptr_t>(sg.l) & 7))
      PL_FAIL(PL_EINVAL, "pl_adamw_flat_planes: segment %d", q);
    in.seg_off[q] = sg.offset; in.seg_n[q] = sg.numel;
    in.seg_h[q] = static_cast<unsigned short*>(sg.h); in.seg_l[q] = static_cast<unsigned short*>(sg.l);
  }
  return PL_OK;
}

}  // namespace

// PLEma as every entry that takes one checks it, before anything is launched
int check_ema(const PLEma& ema, const char* who) {
  if (!ema.e || !aligned16(ema.e)) PL_FAIL(PL_EINVAL, "%s: ema: e is null or not 16-byte aligned", who);
  if (!(ema.decay >= 0.f && ema.decay < 1.f)) PL_FAIL(PL_EINVAL, "%s: ema: decay=%g is outside [0, 1)", who, (double)ema.decay);
  if (ema.t0 < 0) PL_FAIL(PL_EINVAL, "%s: ema: t0=%lld < 0", who, (long long)ema.t0);
  return PL_OK;
}

int launch_adamw(const AdamWArgs& a, hipStream_t s) {
  const AdamWIn& in = a.in;
  if (!a.p || !a.g || !a.m || !a.v) PL_FAIL(PL_EINVAL, "pl_adamw_flat: null pointer");
  if (a.n <= 0 || in.t < (in.t_dev ? 0 : 1)) PL_FAIL(PL_ESHAPE, "pl_adamw_flat: n=%lld t=%lld", (long long)a.n, (long long)in.t);
  if (reinterpret_cast<uintptr_t>(in.clip) & 7) PL_FAIL(PL_EINVAL, "pl_adamw_flat: clip record must be 8-byte aligned");
  if (a.ema) PL_TRY(check_ema(*a.ema, "pl_adamw_flat"));
  const int vec = aligned16(a.p) && aligned16(a.g) && aligned16(a.m) && aligned16(a.v);
  int64_t work = vec ? (a.n >> 2) : a.n;
  int blocks = (int)((work + NTHR - 1) / NTHR);
  if (blocks > kAdamBlocks) blocks = kAdamBlocks;
  if (blocks < 1) blocks = 1;
  const EmaArg<false> off = {};
  const EmaArg<true> on = {a.ema ? *a.ema : PLEma{}};
  const dim3 grid(blocks), block(NTHR);
  if (a.ema && in.clip) hipLaunchKernelGGL((adamw_kernel<true, true>), grid, block, 0, s, a.p, a.g, a.m, a.v, a.n, in, vec, on);
  else if (a.ema) hipLaunchKernelGGL((adamw_kernel<false, true>), grid, block, 0, s, a.p, a.g, a.m, a.v, a.n, in, vec, on);
  else if (in.clip) hipLaunchKernelGGL((adamw_kernel<true, false>), grid, block, 0, s, a.p, a.g, a.m, a.v, a.n, in, vec, off);
  else hipLaunchKernelGGL((adamw_kernel<false, false>), grid, block, 0, s, a.p, a.g, a.m, a.v, a.n, in, vec, off);
  PL_CHECK_LAUNCH("adamw");
  return PL_OK;
}

}  // namespace pl

// The six entry points: the three _clip ones fill an AdamWArgs (the AdamWIn fields they do not name stay zero), the plain
// ones are their _clip twin with no record.
extern "C" int pl_adamw_flat_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, int64_t t, float grad_scale,
                                  const PLClipRecord* clip, void* stream) {
  pl::AdamWArgs a = {p, g, m, v, n, {lr, beta1, beta2, eps, weight_decay, grad_scale, t}};
  a.in.clip = clip;
  return pl::launch_adamw(a, (hipStream_t)stream);
}

extern "C" int pl_adamw_flat(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int64_t t,
                             float grad_scale, void* stream) {
  return pl_adamw_flat_clip(p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, t, grad_scale, nullptr, stream);
}

extern "C" int pl_adamw_flat_dev_clip(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev,
                                      float beta1, float beta2, float eps, float weight_decay, int64_t t_base,
                                      const uint64_t* t_dev, float grad_scale, const PLClipRecord* clip, void* stream) {
  if (!lr_dev || !t_dev) PL_FAIL(PL_EINVAL, "pl_adamw_flat_dev: null lr / t pointer");
  pl::AdamWArgs a = {p, g, m, v, n, {0.f, beta1, beta2, eps, weight_decay, grad_scale, t_base, lr_dev, t_dev}};
  a.in.clip = clip;
  return pl::launch_adamw(a, (hipStream_t)stream);
}

extern "C" int pl_adamw_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_dev,
                                 float beta1, float beta2, float eps, float weight_decay, int64_t t_base,
                                 const uint64_t* t_dev, float grad_scale, void* stream) {
  return pl_adamw_flat_dev_clip(p, g, m, v, n, lr_dev, beta1, beta2, eps, weight_decay, t_base, t_dev, grad_scale, nullptr,
                                stream);
}

extern "C" int pl_adamw_flat_planes_clip(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                                         const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                         int64_t t, const uint64_t* t_dev, float grad_scale, const PLAdamWPlanes* planes,
                                         const PLClipRecord* clip, void* stream) {
  if ((lr_dev != nullptr) != (t_dev != nullptr)) PL_FAIL(PL_EINVAL, "pl_adamw_flat_planes: lr_dev and t_dev go together");
  pl::AdamWArgs a = {p, g, m, v, n, {lr, beta1, beta2, eps, weight_decay, grad_scale, t, lr_dev, t_dev}};
  a.in.clip = clip;
  PL_TRY(pl::adamw_planes(planes, a));
  return pl::launch_adamw(a, (hipStream_t)stream);
}

extern "C" int pl_adamw_flat_planes_clip_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                                             const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                                             int64_t t, const uint64_t* t_dev, float grad_scale, const PLAdamWPlanes* planes,
                                             const PLClipRecord* clip, const PLEma* ema, void* stream) {
  if (!ema)
    return pl_adamw_flat_planes_clip(p, g, m, v, n, lr, lr_dev, beta1, beta2, eps, weight_decay, t, t_dev, grad_scale, planes, clip,
                                     stream);
  if ((lr_dev != nullptr) != (t_dev != nullptr)) PL_FAIL(PL_EINVAL, "pl_adamw_flat_planes: lr_dev and t_dev go together");
  PL_TRY(pl::check_ema(*ema, "pl_adamw_flat_planes_clip_ema"));
  if (n < 0) PL_FAIL(PL_EINVAL, "pl_adamw_flat_planes_clip_ema: n=%lld", (long long)n);
  pl::AdamWArgs a = {p, g, m, v, n, {lr, beta1, beta2, eps, weight_decay, grad_scale, t, lr_dev, t_dev}};
  a.in.clip = clip;
  a.ema = ema;
  PL_TRY(pl::adamw_planes(planes, a));
  return pl::launch_adamw(a, (hipStream_t)stream);
}

extern "C" int pl_swap_f32(float* a, float* b, int64_t n, void* stream) {
  if (!a || !b || a == b) PL_FAIL(PL_EINVAL, "pl_swap_f32: null or aliased pointers");
  if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(b) & 3))
    PL_FAIL(PL_EINVAL, "pl_swap_f32: pointers must be 4-byte aligned");
  if (n < 0) PL_FAIL(PL_EINVAL, "pl_swap_f32: n=%lld", (long long)n);
  if ((a < b ? b - a : a - b) < n) PL_FAIL(PL_EINVAL, "pl_swap_f32: the two ranges overlap");
  if (n == 0) return PL_OK;
  const int vec = pl::aligned16(a) && pl::aligned16(b);
  const int64_t work = vec ? (n >> 2) + (n & 3) : n;
  int blocks = (int)std::min<int64_t>(pl::kAdamBlocks, (work + pl::NTHR - 1) / pl::NTHR);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(pl::swap_f32_kernel, dim3(blocks), dim3(pl::NTHR), 0, (hipStream_t)stream, a, b, n, vec);
  PL_CHECK_LAUNCH("swap_f32");
  return PL_OK;
}

extern "C" int pl_adamw_flat_planes(float* p, const float* g, float* m, float* v, int64_t n, float lr, const float* lr_dev,
                                    float beta1, float beta2, float eps, float weight_decay, int64_t t,
                                    const uint64_t* t_dev, float grad_scale, const PLAdamWPlanes* planes, void* stream) {
  return pl_adamw_flat_planes_clip(p, g, m, v, n, lr, lr_dev, beta1, beta2, eps, weight_decay, t, t_dev, grad_scale, planes,
                                   nullptr, stream);
}

// *counter += delta, one thread: the step counter of an optimizer whose step is replayed from a hipGraph (pl_adamw_flat_dev
// reads t = t_base + *t_dev; this ticks it behind the update)
// (at global scope, as it always was: the kernel keeps its symbol name)
__global__ void counter_add_kernel(uint64_t* counter, int64_t delta) { counter[0] = (uint64_t)((int64_t)counter[0] + delta); }
extern "C" int pl_counter_add(uint64_t* counter, int64_t delta, void* stream) {
  if (!counter) PL_FAIL(PL_EINVAL, "pl_counter_add: null counter");
  hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, delta);
  PL_CHECK_LAUNCH("counter_add");
  return PL_OK;
}

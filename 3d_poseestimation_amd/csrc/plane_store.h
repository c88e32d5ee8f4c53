// Writers / readers of GEMM operand planes for the streaming kernels (PlaneOut, pl_internal.h): the kernel that produces a
// tensor stores it as the planes the planes GEMM stages by LDS-DMA.
#pragma once
#include "pl_internal.h"

namespace pl {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
// range / site: the range guard's record and slot (PlaneOut), NULL for planes whose scale is chosen on the device
struct PlaneDst { unsigned short* h; unsigned short* l; float scale; int kind; int nt; uint32_t* range; int site; };

__device__ __forceinline__ PlaneDst plane_dst(const PlaneOut& o) {
  PlaneDst d = {o.h, o.l, o.scale, o.kind, o.nt, o.range, o.site};
  if (o.kind == 2 && o.dyn) { d.scale = o.dyn[0]; d.range = nullptr; }
  return d;
}

// ---- range guard (poselift.h pl_range_monitor): EVERY static-scale fp16 conversion of the library goes through here ----
// v: four fp32 values about to be stored as fp16(scale * v).  A lane is "over" when a value is finite and |scale * v| > 65504
// (inf / NaN sources are not this arithmetic's doing).  Nothing is over in a model inside the contract, so the common path is
// the compares and one wave-uniform branch; behind it the over-lanes' largest |v| is reduced to one value per wave by lane
// reads (only the active lanes of the caller's control flow take part: the mask comes from their ballot) and ONE lane issues
// one atomic maximum on the slot -- the bits of a non-negative float order like the float.  The stored planes do not change.
// Two pieces, so that a kernel with many stores in straight-line code (a GEMM epilogue's 16, the staging loop of
// small_layer.hip) collects in one register and branches once: range_over4 folds four values into the lane's maximum m
// (0 = nothing over), range_flush is the wave-uniform branch.  range_note4 = both, for a single store.
__device__ __forceinline__ float range_over4(float m, float4 v, float scale) {
  const float s[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = fabsf(s[j]);
    m = (a * scale > 65504.0f && a < __builtin_inff()) ? fmaxf(m, a) : m;
  }
  return m;
}
__device__ __forceinline__ void range_flush(uint32_t* rec, int site, float m) {
  unsigned long long over = __ballot(m != 0.f);
  if (over) {
    const int first = __ffsll(over) - 1;
    const uint32_t mine = __float_as_uint(m);
    uint32_t top = 0;
    do {
      const int src = __ffsll(over) - 1;
      const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)mine, src);
      top = t > top ? t : top;
      over &= over - 1;
    } while (over);
    if ((int)__lane_id() == first) atomicMax(rec + site, top);
  }
}
__device__ __forceinline__ void range_note4(uint32_t* rec, int site, float4 v, float scale) {
  if (rec) range_flush(rec, site, range_over4(0.f, v, scale));
}

// over (optional): the caller collects the range guard's lane maximum there and calls range_flush(d.range, d.site, *over)
// itself, once, where every lane that stored arrives (d.range != NULL only)
__device__ __forceinline__ void store_planes4(const PlaneDst& d, size_t off, float4 v, float* over = nullptr) {
  if (d.kind == 2) {
    if (over) { if (d.range) *over = range_over4(*over, v, d.scale); }
    else range_note4(d.range, d.site, v, d.scale);
    const float a[4] = {v.x * d.scale, v.y * d.scale, v.z * d.scale, v.w * d.scale};
    f16x4 hh, ll;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      hh[j] = (_Float16)a[j];
      ll[j] = (_Float16)((a[j] - (float)hh[j]) * 2048.0f);
    }
    if (d.nt) {
      __builtin_nontemporal_store(hh, reinterpret_cast<f16x4*>(d.h + off));
      __builtin_nontemporal_store(ll, reinterpret_cast<f16x4*>(d.l + off));
    } else {
      *reinterpret_cast<f16x4*>(d.h + off) = hh;
      *reinterpret_cast<f16x4*>(d.l + off) = ll;
    }
  } else if (d.kind == 1) {
    bf16x4 q;
    q[0] = (__bf16)v.x; q[1] = (__bf16)v.y; q[2] = (__bf16)v.z; q[3] = (__bf16)v.w;
    if (d.nt) __builtin_nontemporal_store(q, reinterpret_cast<bf16x4*>(d.h + off));
    else *reinterpret_cast<bf16x4*>(d.h + off) = q;
  }
}

typedef float f32x4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void st4_nt(float* p, float4 v, int nt) {
  if (nt) {
    const f32x4s q = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(q, reinterpret_cast<f32x4s*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}

// x[off .. off+3] back from its planes, times inv (1 / S): kind 2 -> (h + l / 2048) * inv, kind 1 -> the bf16 values
__device__ __forceinline__ float4 load_planes4(int kind, const unsigned short* h, const unsigned short* l, size_t off, float inv) {
  if (kind == 2) {
    const f16x4 hh = *reinterpret_cast<const f16x4*>(h + off), ll = *reinterpret_cast<const f16x4*>(l + off);
    return make_float4(fmaf((float)ll[0], 1.0f / 2048.0f, (float)hh[0]) * inv, fmaf((float)ll[1], 1.0f / 2048.0f, (float)hh[1]) * inv,
                       fmaf((float)ll[2], 1.0f / 2048.0f, (float)hh[2]) * inv, fmaf((float)ll[3], 1.0f / 2048.0f, (float)hh[3]) * inv);
  }
  const bf16x4 q = *reinterpret_cast<const bf16x4*>(h + off);
  return make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
}

}  // namespace pl

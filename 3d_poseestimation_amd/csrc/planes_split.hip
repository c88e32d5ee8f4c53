// fp32 tensors -> the 16-bit operand planes of the planes GEMM (gemm_planes.hip), for tensors no producer kernel writes
// as planes itself: contiguous, and a strided 4-D view (a convolution weight in the layout its GEMM wants).
//
// On the reference path this is the .to(dtype) / .permute().contiguous() / .flip() in front of a matmul or convolution.
#include "pl_internal.h"
#include "plane_store.h"
#include "streaming.h"

namespace pl {
namespace {

// ---- GEMM operand planes written by the kernel that produces the tensor (pl_internal.h PlaneOut) ----------
// Four consecutive elements per lane: one 8-byte store per plane (512 B per wave instruction).
__global__ __launch_bounds__(256) void split_planes_kernel(const float* __restrict__ x, int64_t n4, PlaneOut o) {
  const PlaneDst d = plane_dst(o);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride)
    store_planes4(d, (size_t)i * 4, ld4(x + 4 * i));
}

// The same from a STRIDED 4-D view of the source (signed element strides; output contiguous [d0][d1][d2][d3], d3 % 4 == 0): a
// convolution weight in the layout a GEMM wants -- OIHW -> OHWI, its transpose, its spatial flip -- goes from the parameter
// to planes in ONE launch instead of a layout copy (+ a flip) + a split.  Weights are small: the gathers do not matter.
struct Strided4 { int d1, d2, d3; int64_t s0, s1, s2, s3; };
__global__ __launch_bounds__(256) void split_planes_strided_kernel(const float* __restrict__ x, Strided4 v, int64_t n4, PlaneOut o) {
  const PlaneDst d = plane_dst(o);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int q3 = v.d3 >> 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    const int i3 = (int)(i % q3) * 4;
    int64_t r = i / q3;
    const int i2 = (int)(r % v.d2); r /= v.d2;
    const int i1 = (int)(r % v.d1);
    const int64_t i0 = r / v.d1;
    const float* p = x + i0 * v.s0 + i1 * v.s1 + i2 * v.s2 + (int64_t)i3 * v.s3;
    store_planes4(d, (size_t)i * 4, make_float4(p[0], p[v.s3], p[2 * v.s3], p[3 * v.s3]));
  }
}

// the range guard's slot of a caller-scaled split: the conv path's two scales are named, anything else is "a split"
int split_site(float scale) {
  return scale == kConvActPlaneScale ? PL_RANGE_SITE_CONV_ACT : scale == kWeightPlaneScale ? PL_RANGE_SITE_CONV_WEIGHT : PL_RANGE_SITE_SPLIT;
}

}  // namespace

int launch_split_planes(const float* x, int64_t n, const PlaneOut& out, hipStream_t s) {
  if (!x || !out.h || (out.kind == 2 && !out.l) || out.kind < 1 || out.kind > 2) PL_FAIL(PL_EINVAL, "split_planes: bad arguments");
  if ((n & 3) || !aligned16(x) || (reinterpret_cast<uintptr_t>(out.h) & 7) || (reinterpret_cast<uintptr_t>(out.l) & 7))
    PL_FAIL(PL_EINVAL, "split_planes: n %% 4 and alignment");
  const int64_t n4 = n >> 2;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(split_planes_kernel, dim3(blocks), dim3(256), 0, s, x, n4, out);
  PL_CHECK_LAUNCH("split_planes");
  return PL_OK;
}

// operand planes of a [n]-element tensor for the planes GEMM: mode PL_F16X3 -> [2][n] fp16 (h, l), PL_BF16 -> [n] bf16
int plane_out_of(int mode, void* planes, int64_t n, float scale, const float* dyn, PlaneOut* po, const char* who) {
  *po = PlaneOut{nullptr, nullptr, scale, dyn, 0};
  if (!planes) return PL_OK;
  if (mode != PL_F16X3 && mode != PL_BF16) PL_FAIL(PL_EDTYPE, "%s: planes want PL_F16X3 or PL_BF16 (mode %d)", who, mode);
  if ((reinterpret_cast<uintptr_t>(planes) & 15) || (n & 7)) PL_FAIL(PL_EINVAL, "%s: planes misaligned", who);
  po->h = static_cast<unsigned short*>(planes);
  po->l = po->h + n;
  po->kind = mode == PL_F16X3 ? 2 : 1;
  return PL_OK;
}

}  // namespace pl

extern "C" float pl_conv_act_plane_scale(void) { return pl::kConvActPlaneScale; }

extern "C" int pl_planes_split(const float* x, int64_t n, int mode, float scale, void* planes, void* stream) {
  if (!x || !planes || n <= 0 || !(scale > 0.f)) PL_FAIL(PL_EINVAL, "pl_planes_split: bad arguments");
  PL_REQUIRE_ALIGNED16("pl_planes_split", x);                // (split_planes_kernel reads float4; planes: plane_out_of)
  pl::PlaneOut po;
  PL_TRY(pl::plane_out_of(mode, planes, n, scale, nullptr, &po, "pl_planes_split"));
  pl::range_watch(po, pl::split_site(scale));
  return pl::launch_split_planes(x, n, po, (hipStream_t)stream);
}

// planes of a strided 4-D view: element (i0, i1, i2, i3) of the (contiguous) result is x[i0 s0 + i1 s1 + i2 s2 + i3 s3] -- x already
// points at element (0, 0, 0, 0) of the view, strides in elements and signed (a flipped axis: negative).  dims[3] % 4 == 0.
extern "C" int pl_planes_split_strided(const float* x, const int64_t* dims, const int64_t* strides, int mode, float scale,
                                       void* planes, void* stream) {
  if (!x || !dims || !strides || !planes || !(scale > 0.f)) PL_FAIL(PL_EINVAL, "pl_planes_split_strided: bad arguments");
  for (int i = 0; i < 4; ++i)
    if (dims[i] <= 0 || dims[i] > INT32_MAX) PL_FAIL(PL_ESHAPE, "pl_planes_split_strided: dims[%d] = %lld", i, (long long)dims[i]);
  if (dims[3] & 3) PL_FAIL(PL_ESHAPE, "pl_planes_split_strided: innermost extent %lld is not a multiple of 4", (long long)dims[3]);
  const int64_t n = dims[0] * dims[1] * dims[2] * dims[3];
  pl::PlaneOut po;
  PL_TRY(pl::plane_out_of(mode, planes, n, scale, nullptr, &po, "pl_planes_split_strided"));
  pl::range_watch(po, pl::split_site(scale));
  const pl::Strided4 v = {(int)dims[1], (int)dims[2], (int)dims[3], strides[0], strides[1], strides[2], strides[3]};
  const int64_t n4 = n >> 2;
  int blocks = (int)((n4 + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pl::split_planes_strided_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, v, n4, po);
  PL_CHECK_LAUNCH("split_planes_strided");
  return PL_OK;
}

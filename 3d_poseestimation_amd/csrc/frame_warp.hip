// Frame feed (data.py FrameFeeder, augment_frames): gather + bilinear resize + scale + the pose augmentation's flip, rotation,
// scale and shift of a batch of frames in one launch.  frame_warp.h has the definition; the host entry point runs the same text.
#include "frame_crop.h"
#include "frame_warp.h"
#include "pl_internal.h"

namespace pl {
namespace {

// Grid (pixel tiles, n): a workgroup serves one sample, so the source frame, the row's two Philox calls, sincosf and the
// inverse transform's coefficients depend on blockIdx.y alone -- the same in every lane, made once per thread in front of
// the pixel loop.  The output is the dominant traffic (201 MB at B = 256 into 256 x 256 against at most 3 MB of uint8 source
// per frame, read with 2-D locality through the caches): a lane owns a quad, 4 consecutive output pixels of a row = 12
// floats, written as three 16-byte stores; consecutive lanes own consecutive quads, so a wave-iteration writes 3 KiB in one
// piece.  VEC = false (Wo % 4 != 0 or an output that is not 16-byte aligned) is the tail path: the last quad of a row is
// short, rows start at any float, stores are single floats.  No LDS, no atomics.  Offsets inside a frame fit 32 bits (the
// launcher checks); the frame's and the sample's bases are 64-bit.
constexpr int FW_THREADS = 256;
constexpr int FW_QUADS = 4;   // quads per thread: the per-sample set-up is spread over 16 pixels

// uint8 tables: the two horizontal taps of a row are six neighbouring bytes.  Read one by one they are six loads that each
// touch the same cache lines; the packed path reads the three aligned dwords around them and shifts them into place
// (base 4-byte aligned; offsets in bytes from it).  A quad takes it when none of its eight dword triples reaches past the
// table's end -- all but the quads that read the last bytes of the last frame, which take frame_warp.h's own loads -- and
// then issues all its loads before it waits for any: taps_of clamps the taps of an outside pixel into the frame, so no
// load hangs on a lane's branch.
struct TapWords {
  uint32_t d0, d1, d2;
};
__device__ __forceinline__ bool taps_packable(int64_t off, int64_t total) { return (off & ~(int64_t)3) + 12 <= total; }
__device__ __forceinline__ TapWords load_tap_words(const uint8_t* __restrict__ base, int64_t off) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(base + (off & ~(int64_t)3));
  return TapWords{q[0], q[1], q[2]};
}
// the bytes at off .. off + 5 as the three channels of tap x0 (p0) and of tap x1 = x0 + dx (p1)
__device__ __forceinline__ void unpack_taps(const TapWords& w, int64_t off, int dx, float p0[3], float p1[3]) {
  const uint32_t sh = (uint32_t)(off & 3);
  const uint32_t w0 = __builtin_amdgcn_alignbyte(w.d1, w.d0, sh), w1 = __builtin_amdgcn_alignbyte(w.d2, w.d1, sh);
  p0[0] = (float)(w0 & 0xffu); p0[1] = (float)((w0 >> 8) & 0xffu); p0[2] = (float)((w0 >> 16) & 0xffu);
  p1[0] = dx ? (float)(w0 >> 24) : p0[0];
  p1[1] = dx ? (float)(w1 & 0xffu) : p0[1];
  p1[2] = dx ? (float)((w1 >> 8) & 0xffu) : p0[2];
}

// PACKED (uint8 tables whose base is 4-byte aligned): the packed tap loads above; otherwise frame_warp.h's own loads.  A source
// index outside [0, N) reads frame 0 and writes a NaN frame.
// CROP (pl_frame_warp_gather_crop): the per-sample preamble also computes the row's box from its source 2-D pose,
// x2d[s][34] (row 0 for a bad index), with fc::box_of_pose -- the text the pose launch's box comes from, so the two launches
// agree bit for bit without talking to each other.  Every thread reads the 34 floats itself: their address depends on
// blockIdx.y and kernel arguments alone, so they are workgroup-uniform loads (136 bytes per workgroup out of L2) and need
// neither LDS nor a barrier.  The source position is then fc::source_position; the border rule, the taps and the packed
// path's guard are unchanged, and a NaN box writes a NaN frame like a bad index.  CROP = false is the kernel as it was and
// reads neither x2d nor crop.
template <typename T, bool VEC, bool PACKED, bool CROP>
__global__ __launch_bounds__(FW_THREADS) void frame_warp_gather_kernel(const T* __restrict__ src, int64_t N,
                                                                       const int64_t* __restrict__ src_idx,
                                                                       const int64_t* __restrict__ row_id,
                                                                       float* __restrict__ out, fw::Geom g, pa::Plan p,
                                                                       const float* __restrict__ x2d, fc::Spec crop) {
  static_assert(!PACKED || sizeof(T) == 1, "packed taps are bytes");
  const int64_t k = blockIdx.y;
  const int64_t s = src_idx ? src_idx[k] : k;
  bool ok = s >= 0 && s < N;
  const bool draws = pa::needs_call(p, 0) || pa::needs_call(p, 1);
  const pa::Pose q = fw::pose_of(p, draws ? (uint64_t)row_id[k] : 0);
  fc::Box box = {0.f, 0.f, 1.f};
  if constexpr (CROP) {
    box = fc::box_of_pose(crop, x2d + (ok ? s : 0) * pa::kWA);
    ok = ok && fc::box_ok(box);
  }
  const int64_t frame_elems = (int64_t)g.Hs * g.Ws * 3, frame_off = (ok ? s : 0) * frame_elems;
  float* o = out + k * ((int64_t)g.Ho * g.Wo * 3);
  const int wq = (g.Wo + 3) >> 2, nquad = g.Ho * wq;
  const float bad = __int_as_float(0x7fc00000);
#pragma unroll 1
  for (int it = 0; it < FW_QUADS; ++it) {
    const int quad = ((int)blockIdx.x * FW_QUADS + it) * FW_THREADS + (int)threadIdx.x;
    if (quad >= nquad) return;
    const int i = quad / wq, j0 = (quad - i * wq) * 4;
    float v[12];
    fw::Taps tp[4];
    int64_t off0[4], off1[4];
    bool packed = PACKED;
#pragma unroll
    for (int t = 0; t < 4; ++t) {         // a pixel past the row's end (tail path) is computed as the row's last and not stored
      float xs, ys;
      const int j = VEC || j0 + t < g.Wo ? j0 + t : g.Wo - 1;
      if constexpr (CROP) fc::source_position(p, q, g, box, i, j, xs, ys);
      else fw::source_position(p, q, g, i, j, xs, ys);
      tp[t] = fw::taps_of(g, xs, ys);
      if constexpr (PACKED) {
        off0[t] = frame_off + (tp[t].y0 * g.Ws + tp[t].x0) * 3;
        off1[t] = frame_off + (tp[t].y1 * g.Ws + tp[t].x0) * 3;
        packed = packed && taps_packable(off0[t], N * frame_elems) && taps_packable(off1[t], N * frame_elems);
      }
    }
    if constexpr (PACKED) {
      if (packed) {
        TapWords w0[4], w1[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) { w0[t] = load_tap_words(src, off0[t]); w1[t] = load_tap_words(src, off1[t]); }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          float p00[3], p01[3], p10[3], p11[3];
          unpack_taps(w0[t], off0[t], tp[t].x1 - tp[t].x0, p00, p01);
          unpack_taps(w1[t], off1[t], tp[t].x1 - tp[t].x0, p10, p11);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * t + c] = fw::blend(g, tp[t], p00[c], p01[c], p10[c], p11[c]);
        }
      }
    }
    if (!packed) {
#pragma unroll
      for (int t = 0; t < 4; ++t) fw::sample_taps(src + frame_off, g, tp[t], v + 3 * t);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float f = ok ? g.fill : bad;
      const bool keep = ok && tp[t].inside;
      v[3 * t] = keep ? v[3 * t] : f; v[3 * t + 1] = keep ? v[3 * t + 1] : f; v[3 * t + 2] = keep ? v[3 * t + 2] : f;
    }
    float* d = o + (i * g.Wo + j0) * 3;
    if constexpr (VEC) {
      float4* d4 = reinterpret_cast<float4*>(d);
      d4[0] = make_float4(v[0], v[1], v[2], v[3]);
      d4[1] = make_float4(v[4], v[5], v[6], v[7]);
      d4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (j0 + t < g.Wo) { d[3 * t] = v[3 * t]; d[3 * t + 1] = v[3 * t + 1]; d[3 * t + 2] = v[3 * t + 2]; }
      }
    }
  }
}

// what a crop adds to a launch: the source poses and the spec; x2d null = no crop
struct WarpCrop {
  const float* x2d;
  fc::Spec spec;
};

// frame_warp_gather_kernel's only launch site
template <typename T, bool VEC, bool PACKED>
void launch_frame_warp(const PLFrameWarp& a, const fw::Geom& g, const pa::Plan& p, const WarpCrop& c, hipStream_t s) {
  const int wq = (g.Wo + 3) >> 2, nquad = g.Ho * wq, per = FW_THREADS * FW_QUADS;
  auto kernel = c.x2d ? frame_warp_gather_kernel<T, VEC, PACKED, true> : frame_warp_gather_kernel<T, VEC, PACKED, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((nquad + per - 1) / per), (unsigned)a.n), dim3(FW_THREADS), 0, s, (const T*)a.src,
                     a.N, a.src_idx, a.row_id, a.out, g, p, c.x2d, c.spec);
}

template <typename T>
void warp_host(const PLFrameWarp& a, const fw::Geom& g, const pa::Plan& p, const WarpCrop& c) {
  const bool draws = pa::needs_call(p, 0) || pa::needs_call(p, 1);
  for (int64_t k = 0; k < a.n; ++k) {
    const int64_t s = a.src_idx ? a.src_idx[k] : k;
    const pa::Pose q = fw::pose_of(p, draws ? (uint64_t)a.row_id[k] : 0);
    const T* frame = (const T*)a.src + s * ((int64_t)g.Hs * g.Ws * 3);
    float* o = a.out + k * ((int64_t)g.Ho * g.Wo * 3);
    fc::Box box = {0.f, 0.f, 1.f};
    if (c.x2d) box = fc::box_of_pose(c.spec, c.x2d + s * pa::kWA);
    for (int i = 0; i < g.Ho; ++i)
      for (int j = 0; j < g.Wo; ++j) {
        float xs, ys;
        float* px = o + (i * g.Wo + j) * 3;
        if (!c.x2d) fw::source_position(p, q, g, i, j, xs, ys);
        else if (fc::box_ok(box)) fc::source_position(p, q, g, box, i, j, xs, ys);
        else { px[0] = NAN; px[1] = NAN; px[2] = NAN; continue; }
        fw::sample(frame, g, xs, ys, px);
      }
  }
}

// Argument checks shared by pl_frame_warp_gather and pl_frame_warp_host; on success *g and *plan are what the transform reads.
int frame_warp_args(const char* fn, const PLFrameWarp* a, fw::Geom* g, pa::Plan* plan) {
  if (!a) PL_FAIL(PL_EINVAL, "%s: null argument struct", fn);
  if (!a->src || !a->out) PL_FAIL(PL_EINVAL, "%s: null pointer (table or output)", fn);
  if (a->src_dtype != PL_FRAME_U8 && a->src_dtype != PL_FRAME_F32) PL_FAIL(PL_EINVAL, "%s: src_dtype=%d", fn, (int)a->src_dtype);
  if (a->C != 3) PL_FAIL(PL_ESHAPE, "%s: C=%d, frames have 3 channels", fn, (int)a->C);
  if (a->N <= 0 || a->Hs <= 0 || a->Ws <= 0 || a->Ho <= 0 || a->Wo <= 0 || a->n <= 0)
    PL_FAIL(PL_ESHAPE, "%s: N=%lld Hs=%lld Ws=%lld Ho=%lld Wo=%lld n=%lld", fn, (long long)a->N, (long long)a->Hs, (long long)a->Ws,
            (long long)a->Ho, (long long)a->Wo, (long long)a->n);
  // offsets inside one frame are 32-bit; pixel indices are exact in fp32 (step 1 and step 5 of the definition)
  constexpr int64_t kSide = 1 << 22, kFrame = INT32_MAX / 4;
  if (a->Hs > kSide || a->Ws > kSide || a->Ho > kSide || a->Wo > kSide || a->Hs * a->Ws * 3 > kFrame ||
      a->Ho * a->Wo * 3 > kFrame)
    PL_FAIL(PL_ESHAPE, "%s: a frame of %lld x %lld or %lld x %lld is too large", fn, (long long)a->Hs, (long long)a->Ws,
            (long long)a->Ho, (long long)a->Wo);
  if (a->n > 65535) PL_FAIL(PL_ESHAPE, "%s: n=%lld exceeds 65535 samples per launch", fn, (long long)a->n);
  const int64_t frame = a->Hs * a->Ws * 3, esz = a->src_dtype == PL_FRAME_U8 ? 1 : 4;
  if (a->N > INT64_MAX / (frame * esz)) PL_FAIL(PL_ESHAPE, "%s: N=%lld frames overflow the address space", fn, (long long)a->N);
  if (!a->src_idx && a->n > a->N)
    PL_FAIL(PL_ESHAPE, "%s: n=%lld exceeds the %lld frames of an ungathered batch", fn, (long long)a->n, (long long)a->N);
  const uintptr_t s0 = (uintptr_t)a->src, s1 = s0 + (uintptr_t)(a->N * frame * esz);
  const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + (uintptr_t)(a->n * a->Ho * a->Wo * 3 * 4);
  if (s0 < o1 && o0 < s1) PL_FAIL(PL_EINVAL, "%s: aliased pointers (the output overlaps the table)", fn);
  if (!(fabsf(a->scale) <= 3.402823466e38f) || !(fabsf(a->fill) <= 3.402823466e38f))
    PL_FAIL(PL_EINVAL, "%s: scale or fill is not finite", fn);
  const PLPoseAug none = {0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 0.5f, 0.5f, 0};
  PL_TRY(pose_aug_plan(fn, a->aug ? a->aug : &none, a->epoch, plan));
  if (a->aug && a->aug->p_flip > 0.f && a->aug->flip_offset != 1.f)
    PL_FAIL(PL_EINVAL, "%s: flip_offset=%g: a frame flip mirrors about the image centre (flip_offset 1)", fn,
            (double)a->aug->flip_offset);
  if ((pa::needs_call(*plan, 0) || pa::needs_call(*plan, 1)) && !a->row_id)
    PL_FAIL(PL_EINVAL, "%s: null pointer (row_id)", fn);
  *g = fw::Geom{(int)a->Hs, (int)a->Ws, (int)a->Ho, (int)a->Wo, a->scale, a->fill};
  return PL_OK;
}

// the crop's part of the checks, behind frame_warp_args; crop null: *c says "no crop"
int frame_crop_args(const char* fn, const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d, WarpCrop* c) {
  *c = WarpCrop{};
  if (!crop) return PL_OK;
  if (!x2d) PL_FAIL(PL_EINVAL, "%s: null pointer (x2d)", fn);
  PL_TRY(crop_spec(fn, crop, a->aug, &c->spec));
  if (crop->Hs != a->Hs || crop->Ws != a->Ws)
    PL_FAIL(PL_ESHAPE, "%s: the crop's frame is %lld x %lld, the table's %lld x %lld", fn, (long long)crop->Hs,
            (long long)crop->Ws, (long long)a->Hs, (long long)a->Ws);
  const uintptr_t x0 = (uintptr_t)x2d, x1 = x0 + (uintptr_t)((a->src_idx ? a->N : a->n) * pa::kWA * 4);
  const uintptr_t o0 = (uintptr_t)a->out, o1 = o0 + (uintptr_t)(a->n * a->Ho * a->Wo * 3 * 4);
  if (x0 < o1 && o0 < x1) PL_FAIL(PL_EINVAL, "%s: aliased pointers (the output overlaps x2d)", fn);
  c->x2d = x2d;
  return PL_OK;
}

// the body of both device entry points
int frame_warp_gather(const char* fn, const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d, void* stream) {
  fw::Geom g;
  pa::Plan plan;
  WarpCrop c;
  PL_TRY(frame_warp_args(fn, a, &g, &plan));
  PL_TRY(frame_crop_args(fn, a, crop, x2d, &c));
  const bool vec = (g.Wo & 3) == 0 && ((uintptr_t)a->out & 15) == 0;
  const bool u8 = a->src_dtype == PL_FRAME_U8;
  hipStream_t s = (hipStream_t)stream;
  if (!u8) vec ? launch_frame_warp<float, true, false>(*a, g, plan, c, s) : launch_frame_warp<float, false, false>(*a, g, plan, c, s);
  else if (((uintptr_t)a->src & 3) == 0)
    vec ? launch_frame_warp<uint8_t, true, true>(*a, g, plan, c, s) : launch_frame_warp<uint8_t, false, true>(*a, g, plan, c, s);
  else vec ? launch_frame_warp<uint8_t, true, false>(*a, g, plan, c, s) : launch_frame_warp<uint8_t, false, false>(*a, g, plan, c, s);
  PL_CHECK_LAUNCH("frame_warp_gather");
  return PL_OK;
}

int frame_warp_host(const char* fn, const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d) {
  fw::Geom g;
  pa::Plan plan;
  WarpCrop c;
  PL_TRY(frame_warp_args(fn, a, &g, &plan));
  PL_TRY(frame_crop_args(fn, a, crop, x2d, &c));
  for (int64_t k = 0; k < a->n; ++k) {
    const int64_t s = a->src_idx ? a->src_idx[k] : k;
    if (s < 0 || s >= a->N) PL_FAIL(PL_EINVAL, "%s: src_idx[%lld]=%lld is outside the table", fn, (long long)k, (long long)s);
  }
  if (a->src_dtype == PL_FRAME_U8) warp_host<uint8_t>(*a, g, plan, c);
  else warp_host<float>(*a, g, plan, c);
  return PL_OK;
}

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" int pl_frame_warp_gather(const PLFrameWarp* a, void* stream) {
  return frame_warp_gather("pl_frame_warp_gather", a, nullptr, nullptr, stream);
}

extern "C" int pl_frame_warp_host(const PLFrameWarp* a) { return frame_warp_host("pl_frame_warp_host", a, nullptr, nullptr); }

extern "C" int pl_frame_warp_gather_crop(const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d, void* stream) {
  return frame_warp_gather("pl_frame_warp_gather_crop", a, crop, x2d, stream);
}

extern "C" int pl_frame_warp_host_crop(const PLFrameWarp* a, const PLPoseCrop* crop, const float* x2d) {
  return frame_warp_host("pl_frame_warp_host_crop", a, crop, x2d);
}

// Fused softmax + integral soft-argmax.
//
// Replaces the tail of Model_3D.forward (phase4_joined/Model.py:94-133: norm_heatmap softmax over
// D*H*W voxels per joint, the no-op renormalisation, three marginal sums, arange expectation,
// (c/dim - 0.5)*2) and of Model_2D.forward (phase5_loop/Model_2d.py:96-134: depth 1, c/dim).
// The reference materialises the normalised (B,17,64,64,64) heat-map 3-4 times (17.8 MB per
// frame each); here one pass streams the logits once with an online softmax that carries the
// three coordinate expectations along, and the backward streams them once more:
//   forward : read logits                      -> coords (B,J,3|2) + per-(b,j) {max, sum, Ex, Ey, Ez}
//   backward: read logits, write dlogits       dl = p * sum_a g_a * c_a * (idx_a - E_a)
// HBM-bound: 4 B read per voxel forward, 4 B read + 4 B written backward.
//
// Heat-map supervision (the _hm entry points; HM = true below): the squared error of the normalised heat-map p against the
// Gaussian target g of heatmap_target.h rides in the same two passes, neither p nor g ever stored:
//   sum_v (p - g)^2 = sum p^2 - 2 sum_win p g + sum_win g^2
//   d/dl_v          = 2 w p_v (p_v - g_v - (sum p^2 - sum_win p g)),   w = the upstream gradient of that (b, j)'s sum
// sum e^2 and sum_win e g are two more online accumulators (e^2 rescales by f^2), sum_win g^2 a plain sum; the backward
// gains one fma per voxel.  Same bytes as the plain kernels.  The kernels are written once: the <false> instantiations are
// the plain kernels, instruction for instruction what they were before the template.
#include "heatmap_target.h"
#include "pl_internal.h"
#include "plane_store.h"

namespace pl {
namespace {

constexpr int NTHR = 256;

struct Acc { float m, s, x, y, z; };

__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
  const float m = fmaxf(a.m, b.m);
  const float fa = (a.m == -INFINITY) ? 0.f : __expf(a.m - m);
  const float fb = (b.m == -INFINITY) ? 0.f : __expf(b.m - m);
  a.s = a.s * fa + b.s * fb;
  a.x = a.x * fa + b.x * fb;
  a.y = a.y * fa + b.y * fb;
  a.z = a.z * fa + b.z * fb;
  a.m = m;
}

// the heat-map accumulators of the same partial softmax: q = sum e^2, g = sum_win e * target (both relative to a.m)
struct AccH { float q, g; };

__device__ __forceinline__ void merge_hm(Acc& a, AccH& ah, const Acc& b, const AccH& bh) {
  const float m = fmaxf(a.m, b.m);
  const float fa = (a.m == -INFINITY) ? 0.f : __expf(a.m - m);
  const float fb = (b.m == -INFINITY) ? 0.f : __expf(b.m - m);
  ah.q = ah.q * (fa * fa) + bh.q * (fb * fb);
  ah.g = ah.g * fa + bh.g * fb;
  merge(a, b);
}

// what the HM instantiations read besides the plain arguments (the <false> ones are launched with an empty one)
struct HmIn {
  const float* target;     // [BJ][ncoord]
  plh::Law law;
};

// the four target values of one float4 of a row (w0 .. w0 + 3 at height hh, depth dd); false: the row misses the window
__device__ __forceinline__ bool hm_row4(const plh::Map& mp, const plh::Law& L, float w0, float hh, float dd, float (&g)[4]) {
  g[0] = g[1] = g[2] = g[3] = 0.f;
  if (!(plh::in_window(hh, mp.c[1], L.half) && plh::in_window(dd, mp.c[2], L.half) && w0 + 3.f >= mp.c[0] - L.half &&
        w0 <= mp.c[0] + L.half))
    return false;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (plh::in_window(w0 + (float)k, mp.c[0], L.half)) g[k] = plh::gauss_at(mp, L, w0 + (float)k, hh, dd);
  return true;
}

// the end of both forward kernels: thread 0 of the workgroup, t the map's merged accumulators
template <bool HM>
__device__ __forceinline__ void fwd_finish(const Acc& t, const AccH& th, float gg, bool bad, int D, int H, int W, int centred,
                                           int ncoord, float* __restrict__ coords, float* __restrict__ stats,
                                           float* __restrict__ sq) {
  const float inv = 1.0f / t.s;
  const float ex = t.x * inv, ey = t.y * inv, ez = t.z * inv;
  float* st = stats + (size_t)blockIdx.x * (HM ? 8 : 5);
  st[0] = t.m; st[1] = t.s; st[2] = ex; st[3] = ey; st[4] = ez;
  if (HM) {
    const float nan = __builtin_nanf("");
    const float p2 = bad ? nan : th.q * inv * inv, pg = bad ? nan : th.g * inv;
    st[5] = p2; st[6] = pg; st[7] = bad ? nan : gg;
    sq[blockIdx.x] = (p2 - 2.f * pg) + gg;
  }
  float* c = coords + (size_t)blockIdx.x * ncoord;
  if (centred) {
    c[0] = (ex / (float)W - 0.5f) * 2.f;
    c[1] = (ey / (float)H - 0.5f) * 2.f;
    if (ncoord > 2) c[2] = (ez / (float)D - 0.5f) * 2.f;
  } else {
    c[0] = ex / (float)W;
    c[1] = ey / (float)H;
    if (ncoord > 2) c[2] = ez / (float)D;
  }
}

// one workgroup per (batch, joint) heat-map of n = D*H*W logits; W % 4 == 0
template <bool HM>
__global__ __launch_bounds__(NTHR) void softargmax_fwd_kernel(const float* __restrict__ logits, int D, int H, int W,
                                                              int centred, float* __restrict__ coords, int ncoord,
                                                              float* __restrict__ stats, HmIn hm, float* __restrict__ sq) {
  __shared__ Acc sm[NTHR / 64];
  __shared__ float smh[HM ? NTHR / 64 : 1][3];
  AccH ah = {0.f, 0.f};
  float gg = 0.f;                        // sum_win g^2: no logit in it, so it is summed before the -inf skip
  plh::Map mp = {};
  if (HM) mp = plh::map_of(hm.target + (size_t)blockIdx.x * ncoord, ncoord, D, hm.law);
  const int n4 = (D * H * W) >> 2;
  const float4* __restrict__ src = reinterpret_cast<const float4*>(logits + (size_t)blockIdx.x * D * H * W);
  Acc a = {-INFINITY, 0.f, 0.f, 0.f, 0.f};
  const int w4 = W >> 2;
  for (int i = threadIdx.x; i < n4; i += NTHR) {
    const float4 v = src[i];
    const int wq = i % w4, hd = i / w4;
    const float w0 = (float)(wq * 4), hh = (float)(hd % H), dd = (float)(hd / H);
    const float mx = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    float g[4];
    bool win = false;
    if (HM) {
      win = hm_row4(mp, hm.law, w0, hh, dd, g);
      if (win) gg += (g[0] * g[0] + g[1] * g[1]) + (g[2] * g[2] + g[3] * g[3]);
    }
    if (mx == -INFINITY) continue;       // weight exactly 0 (and with a.m still -inf, v - a.m would be NaN)
    if (mx > a.m) {                      // rescale what this lane has so far
      const float f = (a.m == -INFINITY) ? 0.f : __expf(a.m - mx);
      a.s *= f; a.x *= f; a.y *= f; a.z *= f;
      if (HM) { ah.q *= f * f; ah.g *= f; }
      a.m = mx;
    }
    const float e0 = __expf(v.x - a.m), e1 = __expf(v.y - a.m), e2 = __expf(v.z - a.m), e3 = __expf(v.w - a.m);
    const float es = (e0 + e1) + (e2 + e3);
    if (HM) {
      ah.q += (e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3);
      if (win) ah.g += (e0 * g[0] + e1 * g[1]) + (e2 * g[2] + e3 * g[3]);
    }
    a.s += es;
    a.x += e0 * w0 + e1 * (w0 + 1.f) + e2 * (w0 + 2.f) + e3 * (w0 + 3.f);
    a.y = fmaf(es, hh, a.y);
    a.z = fmaf(es, dd, a.z);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Acc b;
    b.m = __shfl_xor(a.m, o); b.s = __shfl_xor(a.s, o); b.x = __shfl_xor(a.x, o);
    b.y = __shfl_xor(a.y, o); b.z = __shfl_xor(a.z, o);
    if (HM) {
      AccH bh;
      bh.q = __shfl_xor(ah.q, o); bh.g = __shfl_xor(ah.g, o);
      gg += __shfl_xor(gg, o);
      merge_hm(a, ah, b, bh);
    } else {
      merge(a, b);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sm[wave] = a;
    if (HM) { smh[wave][0] = ah.q; smh[wave][1] = ah.g; smh[wave][2] = gg; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc t = sm[0];
    AccH th = {0.f, 0.f};
    float tg = 0.f;
    if (HM) {
      th.q = smh[0][0]; th.g = smh[0][1]; tg = smh[0][2];
      for (int w = 1; w < NTHR / 64; ++w) {
        const AccH bh = {smh[w][0], smh[w][1]};
        tg += smh[w][2];
        merge_hm(t, th, sm[w], bh);
      }
    } else {
      for (int w = 1; w < NTHR / 64; ++w) merge(t, sm[w]);
    }
    fwd_finish<HM>(t, th, tg, HM && plh::map_bad(mp), D, H, W, centred, ncoord, coords, stats, sq);
  }
}

// The same forward on NHWC logits [B][H*W][J*64] (depth 64 = one lane per depth slice): what the conv
// path's final 1x1 convolution writes, so Model_3D inference needs no NHWC -> NCHW pass (1.1 GB read + written
// at B = 64).  One workgroup per (batch, joint); a wavefront reads one pixel's 64 depths (256 B) per load.
template <bool HM>
__global__ __launch_bounds__(NTHR) void softargmax_nhwc_fwd_kernel(const float* __restrict__ logits, int J, int H, int W,
                                                                   float* __restrict__ coords, float* __restrict__ stats,
                                                                   HmIn hm, float* __restrict__ sq) {
  __shared__ Acc sm[NTHR / 64];
  __shared__ float smh[HM ? NTHR / 64 : 1][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / J, j = blockIdx.x - b * J;
  const int P = H * W, C = J * 64;
  const float* __restrict__ src = logits + (size_t)b * P * C + j * 64 + lane;
  Acc a = {-INFINITY, 0.f, 0.f, 0.f, 0.f};
  AccH ah = {0.f, 0.f};
  float gg = 0.f;
  plh::Map mp = {};
  bool lane_in = false;                      // this lane's depth inside the window
  if (HM) {
    mp = plh::map_of(hm.target + (size_t)blockIdx.x * 3, 3, 64, hm.law);
    lane_in = plh::in_window((float)lane, mp.c[2], hm.law.half);
  }
  for (int p0 = wave; p0 < P; p0 += 4 * (NTHR / 64)) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = p0 + q * (NTHR / 64);
      v[q] = p < P ? src[(size_t)p * C] : -INFINITY;
    }
    const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (HM) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int p = p0 + q * (NTHR / 64);
        const float fw = (float)(p % W), fh = (float)(p / W);
        if (p < P && lane_in && plh::in_window(fw, mp.c[0], hm.law.half) && plh::in_window(fh, mp.c[1], hm.law.half)) {
          g[q] = plh::gauss_at(mp, hm.law, fw, fh, (float)lane);
          gg = fmaf(g[q], g[q], gg);
        }
      }
    }
    if (mx == -INFINITY) continue;             // as above
    if (mx > a.m) {
      const float f = (a.m == -INFINITY) ? 0.f : __expf(a.m - mx);
      a.s *= f; a.x *= f; a.y *= f; a.z *= f;
      if (HM) { ah.q *= f * f; ah.g *= f; }
      a.m = mx;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p = p0 + q * (NTHR / 64);
      if (p < P) {
        const float e = __expf(v[q] - a.m);
        a.s += e;
        a.x = fmaf(e, (float)(p % W), a.x);
        a.y = fmaf(e, (float)(p / W), a.y);
        if (HM) { ah.q = fmaf(e, e, ah.q); ah.g = fmaf(e, g[q], ah.g); }
      }
    }
  }
  a.z = a.s * (float)lane;                   // this lane's depth index, weight = its whole mass
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Acc t;
    t.m = __shfl_xor(a.m, o); t.s = __shfl_xor(a.s, o); t.x = __shfl_xor(a.x, o);
    t.y = __shfl_xor(a.y, o); t.z = __shfl_xor(a.z, o);
    if (HM) {
      AccH th;
      th.q = __shfl_xor(ah.q, o); th.g = __shfl_xor(ah.g, o);
      gg += __shfl_xor(gg, o);
      merge_hm(a, ah, t, th);
    } else {
      merge(a, t);
    }
  }
  if (lane == 0) {
    sm[wave] = a;
    if (HM) { smh[wave][0] = ah.q; smh[wave][1] = ah.g; smh[wave][2] = gg; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc t = sm[0];
    AccH th = {0.f, 0.f};
    float tg = 0.f;
    if (HM) {
      th.q = smh[0][0]; th.g = smh[0][1]; tg = smh[0][2];
      for (int w = 1; w < NTHR / 64; ++w) {
        const AccH bh = {smh[w][0], smh[w][1]};
        tg += smh[w][2];
        merge_hm(t, th, sm[w], bh);
      }
    } else {
      for (int w = 1; w < NTHR / 64; ++w) merge(t, sm[w]);
    }
    fwd_finish<HM>(t, th, tg, HM && plh::map_bad(mp), 64, H, W, 1, 3, coords, stats, sq);
  }
}

// a b + c d as the plain backward kernels compile it: two products and a sum, nothing fused.  The HM instantiations say so
// explicitly, because whether the compiler contracts such an expression depends on the code around it, and with gsq == 0
// they owe the plain kernels' values bit for bit.
__device__ __forceinline__ float mul_add_unfused(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float x = a * b, y = c * d;
  return x + y;
}

// one voxel's dlogit with the heat-map term: 2 w p (p - g - hk) on top of the coordinate term p * ct in ONE fma whose addend
// is the plain kernel's expression: w2 = 0 gives the plain kernel's values
__device__ __forceinline__ float dlogit_hm(float p, float ct, float w2, float g, float hk) {
  return fmaf(w2 * p, (p - g) - hk, p * ct);
}

// grid = (chunks, BJ): dlogit = p * (gx*cx*(w-Ex) + gy*cy*(h-Ey) + gz*cz*(d-Ez))
template <bool HM>
__global__ __launch_bounds__(NTHR) void softargmax_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ stats,
                                                              const float* __restrict__ gcoords, int D, int H, int W,
                                                              int centred, int ncoord, float* __restrict__ dlogits, HmIn hm,
                                                              const float* __restrict__ gsq) {
  const int bj = blockIdx.y;
  const int n4 = (D * H * W) >> 2;
  const float* st = stats + (size_t)bj * (HM ? 8 : 5);
  plh::Map mp = {};
  float w2 = 0.f, hk = 0.f;                  // a bad target left NaN in st[5], st[6]: hk, and with it every dlogit, is NaN
  if (HM) {
    mp = plh::map_of(hm.target + (size_t)bj * ncoord, ncoord, D, hm.law);
    w2 = 2.f * gsq[bj];
    hk = st[5] - st[6];
  }
  const float m = st[0], inv = 1.0f / st[1], ex = st[2], ey = st[3], ez = st[4];
  const float k = centred ? 2.f : 1.f;
  const float* g = gcoords + (size_t)bj * ncoord;
  const float gx = g[0] * k / (float)W, gy = g[1] * k / (float)H, gz = ncoord > 2 ? g[2] * k / (float)D : 0.f;
  const float4* __restrict__ src = reinterpret_cast<const float4*>(logits + (size_t)bj * D * H * W);
  float4* __restrict__ dst = reinterpret_cast<float4*>(dlogits + (size_t)bj * D * H * W);
  const int w4 = W >> 2;
  for (int i = blockIdx.x * NTHR + threadIdx.x; i < n4; i += gridDim.x * NTHR) {
    const float4 v = src[i];
    const int wq = i % w4, hd = i / w4;
    const float w0 = (float)(wq * 4) - ex;
    const float base = HM ? mul_add_unfused(gy, (float)(hd % H) - ey, gz, (float)(hd / H) - ez)
                          : gy * ((float)(hd % H) - ey) + gz * ((float)(hd / H) - ez);
    float tg[4] = {0.f, 0.f, 0.f, 0.f};
    if (HM) hm_row4(mp, hm.law, (float)(wq * 4), (float)(hd % H), (float)(hd / H), tg);
    float4 o;
    if (HM) {
      o.x = dlogit_hm(__expf(v.x - m) * inv, fmaf(gx, w0, base), w2, tg[0], hk);
      o.y = dlogit_hm(__expf(v.y - m) * inv, fmaf(gx, w0 + 1.f, base), w2, tg[1], hk);
      o.z = dlogit_hm(__expf(v.z - m) * inv, fmaf(gx, w0 + 2.f, base), w2, tg[2], hk);
      o.w = dlogit_hm(__expf(v.w - m) * inv, fmaf(gx, w0 + 3.f, base), w2, tg[3], hk);
    } else {
      o.x = __expf(v.x - m) * inv * fmaf(gx, w0, base);
      o.y = __expf(v.y - m) * inv * fmaf(gx, w0 + 1.f, base);
      o.z = __expf(v.z - m) * inv * fmaf(gx, w0 + 2.f, base);
      o.w = __expf(v.w - m) * inv * fmaf(gx, w0 + 3.f, base);
    }
    dst[i] = o;
  }
}

// backward on the NHWC layout: one float4 = four consecutive depths of one (pixel, joint); pure streaming
// (4 B read + 4 B written per voxel, every access a whole 16-byte vector of a contiguous row)
template <bool HM>
__global__ __launch_bounds__(NTHR) void softargmax_nhwc_bwd_kernel(const float* __restrict__ logits,
                                                                   const float* __restrict__ stats,
                                                                   const float* __restrict__ gcoords, int J, int H, int W,
                                                                   int64_t n4, float* __restrict__ dlogits, PlaneOut po, HmIn hm,
                                                                   const float* __restrict__ gsq) {
  const int64_t t = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (t >= n4) return;
  const PlaneDst pd = plane_dst(po);
  const int c4 = J * 16;                           // float4s per pixel
  const int q = (int)(t % c4);
  const int64_t bp = t / c4;
  const int P = H * W;
  const int p = (int)(bp % P);
  const int64_t b = bp / P;
  const int j = q >> 4, d0 = (q & 15) * 4;
  const float* st = stats + ((size_t)b * J + j) * (HM ? 8 : 5);
  const float* g = gcoords + ((size_t)b * J + j) * 3;
  const float m = st[0], inv = 1.0f / st[1];
  const float gx = g[0] * 2.f / (float)W, gy = g[1] * 2.f / (float)H, gz = g[2] * 2.f / 64.f;
  const float base = HM ? mul_add_unfused(gx, (float)(p % W) - st[2], gy, (float)(p / W) - st[3])
                        : gx * ((float)(p % W) - st[2]) + gy * ((float)(p / W) - st[3]);
  const float z0 = (float)d0 - st[4];
  const float4 v = reinterpret_cast<const float4*>(logits)[t];
  float tg[4] = {0.f, 0.f, 0.f, 0.f};
  float w2 = 0.f, hk = 0.f;
  if (HM) {
    const plh::Law& L = hm.law;
    const plh::Map mp = plh::map_of(hm.target + ((size_t)b * J + j) * 3, 3, 64, L);
    w2 = 2.f * gsq[(size_t)b * J + j];
    hk = st[5] - st[6];
    const float fw = (float)(p % W), fh = (float)(p / W);
    if (plh::in_window(fw, mp.c[0], L.half) && plh::in_window(fh, mp.c[1], L.half)) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (plh::in_window((float)(d0 + k), mp.c[2], L.half)) tg[k] = plh::gauss_at(mp, L, fw, fh, (float)(d0 + k));
    }
  }
  float4 o;
  if (HM) {
    o.x = dlogit_hm(__expf(v.x - m) * inv, fmaf(gz, z0, base), w2, tg[0], hk);
    o.y = dlogit_hm(__expf(v.y - m) * inv, fmaf(gz, z0 + 1.f, base), w2, tg[1], hk);
    o.z = dlogit_hm(__expf(v.z - m) * inv, fmaf(gz, z0 + 2.f, base), w2, tg[2], hk);
    o.w = dlogit_hm(__expf(v.w - m) * inv, fmaf(gz, z0 + 3.f, base), w2, tg[3], hk);
  } else {
    o.x = __expf(v.x - m) * inv * fmaf(gz, z0, base);
    o.y = __expf(v.y - m) * inv * fmaf(gz, z0 + 1.f, base);
    o.z = __expf(v.z - m) * inv * fmaf(gz, z0 + 2.f, base);
    o.w = __expf(v.w - m) * inv * fmaf(gz, z0 + 3.f, base);
  }
  if (dlogits) reinterpret_cast<float4*>(dlogits)[t] = o;
  if (pd.kind) store_planes4(pd, (size_t)t * 4, o);        // the final convolution's gradient GEMMs read planes
}

// ---- the host side: one launcher per kernel (its checks, its grid, both instantiations' launch); the extern "C" entry points
// fill its argument struct and pass their own name, which every message starts with.
// The dims of every NCHW entry point -- w4: the soft-argmax kernels read float4 rows, the dense target does not; max_bj: BJ is
// grid.x (65535 * 64; the backward, where it is grid.y, then answers with a message of its own) or the target's grid.y
int check_dims(const char* who, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord, bool w4, int64_t max_bj) {
  if (BJ <= 0 || BJ > max_bj || D <= 0 || H <= 0 || W <= 0 || (w4 && (W & 3)) || D * H * W > (int64_t)1 << 30)
    PL_FAIL(PL_ESHAPE, "%s: bad dims BJ=%lld D=%lld H=%lld W=%lld%s", who, (long long)BJ, (long long)D, (long long)H,
            (long long)W, w4 ? " (W % 4 == 0)" : "");
  if (ncoord != 2 && ncoord != 3) PL_FAIL(PL_ESHAPE, "%s: ncoord=%d", who, ncoord);
  if (ncoord == 2 && D != 1) PL_FAIL(PL_ESHAPE, "%s: 2 coordinates need depth 1", who);
  return PL_OK;
}

// the dense target [BJ][D][H][W] (visualisation, tests): grid = (chunks, BJ), one voxel per thread and step; a bad pair's
// map is NaN throughout
__global__ __launch_bounds__(NTHR) void heatmap_gaussian_kernel(const float* __restrict__ target, int D, int H, int W,
                                                                int ncoord, plh::Law law, float* __restrict__ out) {
  const int bj = blockIdx.y;
  const int n = D * H * W;
  const plh::Map mp = plh::map_of(target + (size_t)bj * ncoord, ncoord, D, law);
  const bool bad = plh::map_bad(mp);
  float* __restrict__ dst = out + (size_t)bj * n;
  for (int i = blockIdx.x * NTHR + threadIdx.x; i < n; i += gridDim.x * NTHR) {
    const int w = i % W, hd = i / W;
    dst[i] = bad ? __builtin_nanf("") : plh::value_at(mp, law, (float)w, (float)(hd % H), (float)(hd / H));
  }
}

// the host's half of every _hm entry point: sigma -> window and 1 / (2 sigma^2), law[6] = {alpha x, y, z, gamma x, y, z}
int heat_law_of(const char* who, float sigma, const float* law, plh::Law* L) {
  if (!law) PL_FAIL(PL_EINVAL, "%s: null law", who);
  const int half = plh::half_of_sigma(sigma);
  if (half < 0) PL_FAIL(PL_EINVAL, "%s: sigma=%g is not a positive finite number", who, (double)sigma);
  if (half > plh::kMaxHalf)
    PL_FAIL(PL_ESHAPE, "%s: sigma=%g needs a window of half-width %d > %d", who, (double)sigma, half, plh::kMaxHalf);
  for (int a = 0; a < 3; ++a) {
    if (!plh::finite1(law[a]) || !plh::finite1(law[3 + a])) PL_FAIL(PL_EINVAL, "%s: law[%d] is not finite", who, a);
    L->alpha[a] = law[a];
    L->gamma[a] = law[3 + a];
  }
  L->half = (float)half;
  L->k = 1.0 / (2.0 * (double)sigma * (double)sigma);
  return PL_OK;
}

// what an _hm entry point receives besides the plain arguments, unchecked: the launchers check it where the entry points
// always did (target among the pointers, sigma and law after the dims), so a call that is wrong twice answers as it used to
struct HmArgs { const float* target; float sigma; const float* law; };

// the kernels' heat-map input; hm == NULL: the empty one that the <false> instantiations are launched with
int hm_in_of(const char* who, const HmArgs* hm, HmIn* in) {
  *in = HmIn{};
  if (!hm) return PL_OK;
  if (!hm->target) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  in->target = hm->target;
  return heat_law_of(who, hm->sigma, hm->law, &in->law);
}

struct FwdArgs {
  const float* logits;
  int64_t BJ, D, H, W;
  int ncoord, centred;
  float *coords, *stats, *sq;                       // sq: with hm
};

int launch_softargmax_fwd(const FwdArgs& a, const char* who, const HmArgs* hm, hipStream_t s) {
  if (!a.logits || !a.coords || !a.stats || (hm && (!hm->target || !a.sq))) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (reinterpret_cast<uintptr_t>(a.logits) & 15) PL_FAIL(PL_EINVAL, "%s: logits not 16-byte aligned", who);
  PL_TRY(check_dims(who, a.BJ, a.D, a.H, a.W, a.ncoord, true, 65535 * 64));
  HmIn in;
  PL_TRY(hm_in_of(who, hm, &in));
  hipLaunchKernelGGL((hm ? softargmax_fwd_kernel<true> : softargmax_fwd_kernel<false>), dim3((unsigned)a.BJ), dim3(NTHR), 0, s,
                     a.logits, (int)a.D, (int)a.H, (int)a.W, a.centred, a.coords, a.ncoord, a.stats, in, hm ? a.sq : nullptr);
  PL_CHECK_LAUNCH(who);
  return PL_OK;
}

struct BwdArgs {
  const float *logits, *stats, *gcoords, *gsq;      // gsq: with hm
  int64_t BJ, D, H, W;
  int ncoord, centred;
  float* dlogits;
};

int launch_softargmax_bwd(const BwdArgs& a, const char* who, const HmArgs* hm, hipStream_t s) {
  if (!a.logits || !a.stats || !a.gcoords || !a.dlogits || (hm && (!hm->target || !a.gsq)))
    PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(a.logits) | reinterpret_cast<uintptr_t>(a.dlogits)) & 15)
    PL_FAIL(PL_EINVAL, "%s: logits / dlogits not 16-byte aligned", who);
  PL_TRY(check_dims(who, a.BJ, a.D, a.H, a.W, a.ncoord, true, 65535 * 64));
  if (a.BJ > 65535) PL_FAIL(PL_ESHAPE, "%s: BJ=%lld > 65535 (split the batch)", who, (long long)a.BJ);
  HmIn in;
  PL_TRY(hm_in_of(who, hm, &in));
  const int64_t n4 = (a.D * a.H * a.W) >> 2;
  int chunks = (int)((n4 + NTHR * 8 - 1) / (NTHR * 8));      // 8 float4 per thread
  if (chunks < 1) chunks = 1;
  if (chunks > 64) chunks = 64;
  hipLaunchKernelGGL((hm ? softargmax_bwd_kernel<true> : softargmax_bwd_kernel<false>), dim3(chunks, (unsigned)a.BJ), dim3(NTHR),
                     0, s, a.logits, a.stats, a.gcoords, (int)a.D, (int)a.H, (int)a.W, a.centred, a.ncoord, a.dlogits, in,
                     hm ? a.gsq : nullptr);
  PL_CHECK_LAUNCH(who);
  return PL_OK;
}

int check_nhwc_dims(const char* who, int64_t B, int64_t J, int64_t H, int64_t W) {
  if (B <= 0 || J <= 0 || H <= 0 || W <= 0 || B * J > 0x7fffffff || H * W > (1 << 24)) PL_FAIL(PL_ESHAPE, "%s: bad dims", who);
  return PL_OK;
}

struct NhwcFwdArgs {
  const float* logits;
  int64_t B, J, H, W;
  float *coords, *stats, *sq;                       // sq: with hm
};

int launch_softargmax_nhwc_fwd(const NhwcFwdArgs& a, const char* who, const HmArgs* hm, hipStream_t s) {
  if (!a.logits || !a.coords || !a.stats || (hm && (!hm->target || !a.sq))) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PL_TRY(check_nhwc_dims(who, a.B, a.J, a.H, a.W));
  HmIn in;
  PL_TRY(hm_in_of(who, hm, &in));
  hipLaunchKernelGGL((hm ? softargmax_nhwc_fwd_kernel<true> : softargmax_nhwc_fwd_kernel<false>), dim3((unsigned)(a.B * a.J)),
                     dim3(NTHR), 0, s, a.logits, (int)a.J, (int)a.H, (int)a.W, a.coords, a.stats, in, hm ? a.sq : nullptr);
  PL_CHECK_LAUNCH(who);
  return PL_OK;
}

// dl_planes (optional): dlogits also / only (dlogits == NULL) as operand planes for the final convolution's gradient GEMMs.
// PL_F16X3: the planes hold dl_scale[0] * dlogits -- dl_scale = {S, 1/S} on the device, S a power of two that the CALLER
// derives from the bound on |dlogit| (pl_softargmax_dl_scale; with hm pl_softargmax_hm_dl_scale, the bound grows by 4 |gsq|)
struct NhwcBwdArgs {
  const float *logits, *stats, *gcoords, *gsq;      // gsq [B*J], with hm: the upstream gradient of sq
  int64_t B, J, H, W;
  float* dlogits;
  void* dl_planes;
  int planes_mode;
  const float* dl_scale;
};

int launch_softargmax_nhwc_bwd(const NhwcBwdArgs& a, const char* who, const HmArgs* hm, hipStream_t s) {
  if (!a.logits || !a.stats || !a.gcoords || (!a.dlogits && !a.dl_planes) || (hm && (!hm->target || !a.gsq)))
    PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if ((reinterpret_cast<uintptr_t>(a.logits) | reinterpret_cast<uintptr_t>(a.dlogits)) & 15)
    PL_FAIL(PL_EINVAL, "%s: logits / dlogits not 16-byte aligned", who);
  PL_TRY(check_nhwc_dims(who, a.B, a.J, a.H, a.W));
  const int64_t n4 = a.B * a.H * a.W * a.J * 16;
  if (n4 > (int64_t)INT32_MAX * NTHR) PL_FAIL(PL_ESHAPE, "%s: too large", who);
  const bool f16 = a.planes_mode == PL_F16X3;
  if (a.dl_planes && f16 && !a.dl_scale) PL_FAIL(PL_EINVAL, "%s: fp16 planes need dl_scale", who);
  HmIn in;
  PL_TRY(hm_in_of(who, hm, &in));
  PlaneOut po;
  PL_TRY(plane_out_of(a.planes_mode, a.dl_planes, n4 * 4, 1.0f, f16 ? a.dl_scale : nullptr, &po, who));
  hipLaunchKernelGGL((hm ? softargmax_nhwc_bwd_kernel<true> : softargmax_nhwc_bwd_kernel<false>),
                     dim3((unsigned)((n4 + NTHR - 1) / NTHR)), dim3(NTHR), 0, s, a.logits, a.stats, a.gcoords, (int)a.J, (int)a.H,
                     (int)a.W, n4, a.dlogits, po, in, hm ? a.gsq : nullptr);
  PL_CHECK_LAUNCH(who);
  return PL_OK;
}

}  // namespace
}  // namespace pl

using namespace pl;

extern "C" int pl_softargmax_fwd(const float* logits, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord,
                                 int centred, float* coords, float* stats, void* stream) {
  return launch_softargmax_fwd({logits, BJ, D, H, W, ncoord, centred, coords, stats, nullptr}, "pl_softargmax_fwd", nullptr,
                               (hipStream_t)stream);
}

extern "C" int pl_softargmax_hm_fwd(const float* logits, const float* target, int64_t BJ, int64_t D, int64_t H, int64_t W,
                                    int ncoord, int centred, float sigma, const float* law, float* coords, float* sq,
                                    float* stats, void* stream) {
  const HmArgs hm = {target, sigma, law};
  return launch_softargmax_fwd({logits, BJ, D, H, W, ncoord, centred, coords, stats, sq}, "pl_softargmax_hm_fwd", &hm,
                               (hipStream_t)stream);
}

extern "C" int pl_softargmax_bwd(const float* logits, const float* stats, const float* gcoords, int64_t BJ,
                                 int64_t D, int64_t H, int64_t W, int ncoord, int centred, float* dlogits,
                                 void* stream) {
  return launch_softargmax_bwd({logits, stats, gcoords, nullptr, BJ, D, H, W, ncoord, centred, dlogits}, "pl_softargmax_bwd",
                               nullptr, (hipStream_t)stream);
}

extern "C" int pl_softargmax_hm_bwd(const float* logits, const float* target, const float* stats, const float* gcoords,
                                    const float* gsq, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord, int centred,
                                    float sigma, const float* law, float* dlogits, void* stream) {
  const HmArgs hm = {target, sigma, law};
  return launch_softargmax_bwd({logits, stats, gcoords, gsq, BJ, D, H, W, ncoord, centred, dlogits}, "pl_softargmax_hm_bwd", &hm,
                               (hipStream_t)stream);
}

extern "C" int pl_softargmax3d_nhwc_fwd(const float* logits, int64_t B, int64_t J, int64_t H, int64_t W,
                                        float* coords, float* stats, void* stream) {
  return launch_softargmax_nhwc_fwd({logits, B, J, H, W, coords, stats, nullptr}, "pl_softargmax3d_nhwc_fwd", nullptr,
                                    (hipStream_t)stream);
}

extern "C" int pl_softargmax3d_nhwc_hm_fwd(const float* logits, const float* target, int64_t B, int64_t J, int64_t H,
                                           int64_t W, float sigma, const float* law, float* coords, float* sq, float* stats,
                                           void* stream) {
  const HmArgs hm = {target, sigma, law};
  return launch_softargmax_nhwc_fwd({logits, B, J, H, W, coords, stats, sq}, "pl_softargmax3d_nhwc_hm_fwd", &hm,
                                    (hipStream_t)stream);
}

extern "C" int pl_softargmax3d_nhwc_bwd(const float* logits, const float* stats, const float* gcoords, int64_t B,
                                        int64_t J, int64_t H, int64_t W, float* dlogits, void* stream) {
  const char* who = "pl_softargmax3d_nhwc_bwd";
  if (!dlogits) PL_FAIL(PL_EINVAL, "%s: null pointer", who);          // (no planes to write instead)
  return launch_softargmax_nhwc_bwd({logits, stats, gcoords, nullptr, B, J, H, W, dlogits, nullptr, 0, nullptr}, who, nullptr,
                                    (hipStream_t)stream);
}

extern "C" int pl_softargmax3d_nhwc_bwd_ex(const float* logits, const float* stats, const float* gcoords, int64_t B,
                                           int64_t J, int64_t H, int64_t W, float* dlogits, void* dl_planes, int planes_mode,
                                           const float* dl_scale, void* stream) {
  return launch_softargmax_nhwc_bwd({logits, stats, gcoords, nullptr, B, J, H, W, dlogits, dl_planes, planes_mode, dl_scale},
                                    "pl_softargmax3d_nhwc_bwd_ex", nullptr, (hipStream_t)stream);
}

extern "C" int pl_softargmax3d_nhwc_hm_bwd_ex(const float* logits, const float* target, const float* stats,
                                              const float* gcoords, const float* gsq, int64_t B, int64_t J, int64_t H,
                                              int64_t W, float sigma, const float* law, float* dlogits, void* dl_planes,
                                              int planes_mode, const float* dl_scale, void* stream) {
  const HmArgs hm = {target, sigma, law};
  return launch_softargmax_nhwc_bwd({logits, stats, gcoords, gsq, B, J, H, W, dlogits, dl_planes, planes_mode, dl_scale},
                                    "pl_softargmax3d_nhwc_hm_bwd_ex", &hm, (hipStream_t)stream);
}

extern "C" int pl_heatmap_gaussian(const float* target, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord, float sigma,
                                   const float* law, float* out, void* stream) {
  if (!target || !out) PL_FAIL(PL_EINVAL, "pl_heatmap_gaussian: null pointer");
  PL_TRY(check_dims("pl_heatmap_gaussian", BJ, D, H, W, ncoord, false, 65535));
  plh::Law L;
  PL_TRY(heat_law_of("pl_heatmap_gaussian", sigma, law, &L));
  const int64_t n = D * H * W;
  int chunks = (int)((n + NTHR * 16 - 1) / (NTHR * 16));
  if (chunks > 64) chunks = 64;
  hipLaunchKernelGGL(heatmap_gaussian_kernel, dim3(chunks, (unsigned)BJ), dim3(NTHR), 0, (hipStream_t)stream, target, (int)D,
                     (int)H, (int)W, ncoord, L, out);
  PL_CHECK_LAUNCH("heatmap_gaussian");
  return PL_OK;
}

extern "C" int pl_heatmap_gaussian_host(const float* target, int64_t BJ, int64_t D, int64_t H, int64_t W, int ncoord,
                                        float sigma, const float* law, float* out) {
  if (!target || !out) PL_FAIL(PL_EINVAL, "pl_heatmap_gaussian_host: null pointer");
  PL_TRY(check_dims("pl_heatmap_gaussian_host", BJ, D, H, W, ncoord, false, 65535));
  plh::Law L;
  PL_TRY(heat_law_of("pl_heatmap_gaussian_host", sigma, law, &L));
  for (int64_t bj = 0; bj < BJ; ++bj) {
    const plh::Map mp = plh::map_of(target + bj * ncoord, ncoord, (int)D, L);
    const bool bad = plh::map_bad(mp);
    float* dst = out + bj * D * H * W;
    for (int64_t d = 0; d < D; ++d)
      for (int64_t h = 0; h < H; ++h)
        for (int64_t w = 0; w < W; ++w)
          dst[(d * H + h) * W + w] = bad ? __builtin_nanf("") : plh::value_at(mp, L, (float)w, (float)h, (float)d);
  }
  return PL_OK;
}

// {S, 1/S} for the fp16 planes of dlogits: S the power of two that maps the bound 2 max_(b,j) sum_c |g_c| >= max |dlogit|
// into (2^13, 2^14] (softmax weights <= 1, index offsets < the map size); bound 0 / inf / nan -> 1.  One workgroup.
// HM: the heat-map term adds 2 |w| p |p - g - (sum p^2 - sum p g)| <= 4 |w| (p <= 1, |p - g| <= 1, the bracket's last part in
// [-1, 1]): the bound is 2 max_(b,j) (sum_c |g_c| + 2 |gsq|)
template <bool HM>
__device__ __forceinline__ void softargmax_dl_scale_body(const float* __restrict__ g, const float* __restrict__ gsq,
                                                         int64_t rows, int ncoord, float* __restrict__ out) {
  __shared__ float sm[2 * (NTHR / 64)];
  float m = 0.f, bad = 0.f;                           // bad: a row sum that is inf / nan (fmaxf would drop a nan)
  for (int64_t r = threadIdx.x; r < rows; r += NTHR) {
    float a = 0.f;
    for (int c = 0; c < ncoord; ++c) a += fabsf(g[r * ncoord + c]);
    if (HM) a += 2.f * fabsf(gsq[r]);
    if (!(a < 3.0e38f)) bad = 1.f;
    m = fmaxf(m, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o)); bad = fmaxf(bad, __shfl_xor(bad, o)); }
  if ((threadIdx.x & 63) == 0) { sm[2 * (threadIdx.x >> 6)] = m; sm[2 * (threadIdx.x >> 6) + 1] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < NTHR / 64; ++w) { m = fmaxf(m, sm[2 * w]); bad = fmaxf(bad, sm[2 * w + 1]); }
    if (bad > 0.f) m = 0.f;
    const float bound = 2.0f * m;
    float S = 1.0f, Si = 1.0f;
    if (bound > 0.f && bound < 3.0e38f) {
      int e = 0;
      (void)frexpf(bound, &e);
      e = min(max(14 - e, -100), 100);
      S = ldexpf(1.0f, e); Si = ldexpf(1.0f, -e);
    }
    out[0] = S; out[1] = Si;
  }
}

__global__ __launch_bounds__(NTHR) void softargmax_dl_scale_kernel(const float* __restrict__ g, int64_t rows, int ncoord,
                                                                   float* __restrict__ out) {
  softargmax_dl_scale_body<false>(g, nullptr, rows, ncoord, out);
}

__global__ __launch_bounds__(NTHR) void softargmax_hm_dl_scale_kernel(const float* __restrict__ g, const float* __restrict__ gsq,
                                                                      int64_t rows, int ncoord, float* __restrict__ out) {
  softargmax_dl_scale_body<true>(g, gsq, rows, ncoord, out);
}

namespace pl {
namespace {

struct DlScaleArgs {
  const float *gcoords, *gsq;           // gsq: with the heat-map term
  int64_t rows;
  int ncoord;
  float* scale2;
};

int launch_softargmax_dl_scale(const DlScaleArgs& a, const char* who, bool hm, hipStream_t s) {
  if (!a.gcoords || !a.scale2 || (hm && !a.gsq)) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (a.rows <= 0 || a.ncoord <= 0 || a.ncoord > 3) PL_FAIL(PL_ESHAPE, "%s: bad dims", who);
  if (hm)
    hipLaunchKernelGGL(softargmax_hm_dl_scale_kernel, dim3(1), dim3(NTHR), 0, s, a.gcoords, a.gsq, a.rows, a.ncoord, a.scale2);
  else
    hipLaunchKernelGGL(softargmax_dl_scale_kernel, dim3(1), dim3(NTHR), 0, s, a.gcoords, a.rows, a.ncoord, a.scale2);
  PL_CHECK_LAUNCH(who);
  return PL_OK;
}

}  // namespace
}  // namespace pl

extern "C" int pl_softargmax_dl_scale(const float* gcoords, int64_t rows, int ncoord, float* scale2, void* stream) {
  return launch_softargmax_dl_scale({gcoords, nullptr, rows, ncoord, scale2}, "pl_softargmax_dl_scale", false,
                                    (hipStream_t)stream);
}

extern "C" int pl_softargmax_hm_dl_scale(const float* gcoords, const float* gsq, int64_t rows, int ncoord, float* scale2,
                                         void* stream) {
  return launch_softargmax_dl_scale({gcoords, gsq, rows, ncoord, scale2}, "pl_softargmax_hm_dl_scale", true,
                                    (hipStream_t)stream);
}

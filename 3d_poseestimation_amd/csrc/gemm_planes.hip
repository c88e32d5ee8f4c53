// GEMMs on pre-split 16-bit operand planes (gemm_planes.h): the 1024-wide Linears of the lifter in the
// PL_F16X3 (fp32-grade, three fp16 MFMAs per product term) and PL_BF16 (bf16 storage) modes.
//
// Replaces the ATen addmm calls behind nn.Linear forward / backward (reference phase1_lifting/baselineModel.py:33,39
// and their autograd), like gemm_f32.hip; same 128x128 tile per workgroup, the element order of its register epilogue
// (gemm_epilogue.h) in an epilogue of its own (staged_epilogue below: bias, training-mode BatchNorm partial statistics,
// eval-mode BN fold + ReLU + skip, residual-gradient addend, split-K slabs).  512 threads: wavefronts 0-3 compute,
// wavefronts 4-7 drive the LDS-DMA.
#include "gemm_planes16.h"
#include "pl_internal.h"
#include "plane_store.h"

namespace pl {
namespace {

struct PlanesKern {
  plp::PlanesArgs p;
  GemmArgs e;
  float out_scale;
  const float* dyn_inv;
  int nt_store;            // C leaves with nontemporal stores (an output far larger than the caches, read next from HBM anyway)
};

// x_l + x_(l ^ 16) and x_l + x_(l ^ 32) in every lane, by ONE vector instruction each (gfx950: v_permlane16_swap /
// v_permlane32_swap exchange 16- / 32-lane rows of two registers) instead of a ds_bpermute round trip through the LDS
// crossbar.  IEEE addition commutes, so the sums are bit for bit those of `x += __shfl_xor(x, 16 | 32)`.
__device__ __forceinline__ float xadd16(const float v) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float xadd32(const float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float4 xadd_rows(float4 s) {       // the four lanes l, l^16, l^32, l^48: fixed order (16, then 32)
  s.x = xadd32(xadd16(s.x)); s.y = xadd32(xadd16(s.y)); s.z = xadd32(xadd16(s.z)); s.w = xadd32(xadd16(s.w));
  return s;
}

// ---- the epilogue on the wave's 64x64 block staged in its own 17 KB of LDS (row stride 68 floats: conflict-free both
// ways), everything as 16-byte accesses on 256-byte row segments.  Lane (lr = lane >> 4, lc = 4 (lane & 15)) owns columns
// col0 .. col0+3 of rows lr, lr+4, ..., lr+60.  Same operation order per element as gemm_epilogue (bias, skip-gradient
// addend, eval-BN fold, ReLU, residual, ReLU); statistics and the BatchNorm-backward sums per 64-row block in a fixed order.
template <bool EDGE>
__device__ __forceinline__ void staged_epilogue(const PlanesKern& k, float* __restrict__ C, float4 (&v)[16],
                                                const int m0, const int n0, const int wm, const int wn, const int lane) {
  const GemmArgs& e = k.e;
  const int lr = lane >> 4, lc = (lane & 15) * 4;
  const int row0 = m0 + wm * 64 + lr, col0 = n0 + wn * 64 + lc;
  const size_t o0 = (size_t)row0 * e.ldc + col0;
  const bool plain = e.split_k > 1;              // split-K slab: the bare partial product
  // EDGE: rows >= M / columns >= N of an overhanging tile hold garbage: never loaded for, never stored, never counted
  const int nrows = EDGE ? e.M - (m0 + wm * 64) : 64;          // valid rows of this wave's block (may be <= 0)
  const bool cok = !EDGE || col0 < e.N;
  auto ok = [&](int it) { return !EDGE || (cok && lr + 4 * it < nrows); };
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  // (Tried: requesting bnr_z's sixteen float4 here, ahead of the addend, so that both arrive in one round trip instead of two in
  //  a row.  Same-box A/B over five interleaved runs: dual launch 63.1 us against 62.4 us as it is -- the epilogue's burst is
  //  bandwidth, not latency; more of it in flight at once only lengthens the queue.  Not kept.)
  if (!plain) {
    if (e.bias) {
      const float4 b = cok ? *reinterpret_cast<const float4*>(e.bias + col0) : zero4;
#pragma unroll
      for (int it = 0; it < 16; ++it) { v[it].x += b.x; v[it].y += b.y; v[it].z += b.z; v[it].w += b.w; }
    }
    if (e.addend) {
      float4 q[16];
#pragma unroll
      for (int it = 0; it < 16; ++it) q[it] = ok(it) ? *reinterpret_cast<const float4*>(e.addend + o0 + (size_t)it * 4 * e.ldc) : zero4;
#pragma unroll
      for (int it = 0; it < 16; ++it) { v[it].x += q[it].x; v[it].y += q[it].y; v[it].z += q[it].z; v[it].w += q[it].w; }
    }
    if (e.col_scale) {
      const float4 sc = cok ? *reinterpret_cast<const float4*>(e.col_scale + col0) : zero4;
      const float4 sh = cok ? *reinterpret_cast<const float4*>(e.col_shift + col0) : zero4;
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        v[it].x = fmaf(v[it].x, sc.x, sh.x); v[it].y = fmaf(v[it].y, sc.y, sh.y);
        v[it].z = fmaf(v[it].z, sc.z, sh.z); v[it].w = fmaf(v[it].w, sc.w, sh.w);
      }
    }
    if (e.relu == 1) {
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        v[it].x = relu_f(v[it].x); v[it].y = relu_f(v[it].y); v[it].z = relu_f(v[it].z); v[it].w = relu_f(v[it].w);
      }
    }
    if (e.resid) {
      float4 q[16];
#pragma unroll
      for (int it = 0; it < 16; ++it) q[it] = ok(it) ? *reinterpret_cast<const float4*>(e.resid + o0 + (size_t)it * 4 * e.ldc) : zero4;
#pragma unroll
      for (int it = 0; it < 16; ++it) { v[it].x += q[it].x; v[it].y += q[it].y; v[it].z += q[it].z; v[it].w += q[it].w; }
    }
    if (e.relu == 2) {
#pragma unroll
      for (int it = 0; it < 16; ++it) {
        v[it].x = relu_f(v[it].x); v[it].y = relu_f(v[it].y); v[it].z = relu_f(v[it].z); v[it].w = relu_f(v[it].w);
      }
    }
  }
  // the result as the next GEMM's operand planes
  const PlaneDst cpd = {e.cpl_h, e.cpl_l, e.cpl_scale, plain ? 0 : e.cpl_kind, k.nt_store, e.cpl_range, e.cpl_site};
  float cpl_over = 0.f;                          // range guard of those planes: one flush behind the stores (plane_store.h)
  if (EDGE && e.scat_on) {                       // one output parity of a transposed convolution (GemmArgs::scat_*)
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      if (!ok(it)) continue;
      const int m = row0 + 4 * it;
      const int c = m % e.conv_wo, t = m / e.conv_wo;
      const int a = t % e.conv_ho, b = t / e.conv_ho;
      const size_t orow = ((size_t)b * 2 * e.conv_ho + 2 * a + e.scat_ph) * 2 * e.conv_wo + 2 * c + e.scat_pw;
      if (C) *reinterpret_cast<float4*>(C + orow * e.ldc + col0) = v[it];
      if (cpd.kind) store_planes4(cpd, orow * e.ldc + col0, v[it], &cpl_over);
    }
    if (cpd.kind == 2 && cpd.range) range_flush(cpd.range, cpd.site, cpl_over);
    return;
  }
  if (k.nt_store && C) {
    typedef float f4v __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int it = 0; it < 16; ++it)
      if (ok(it)) {
        const f4v q = {v[it].x, v[it].y, v[it].z, v[it].w};
        __builtin_nontemporal_store(q, reinterpret_cast<f4v*>(C + o0 + (size_t)it * 4 * e.ldc));
        if (cpd.kind) store_planes4(cpd, o0 + (size_t)it * 4 * e.ldc, v[it], &cpl_over);
      }
  } else {
#pragma unroll
  for (int it = 0; it < 16; ++it)
    if (ok(it)) {
      if (C) *reinterpret_cast<float4*>(C + o0 + (size_t)it * 4 * e.ldc) = v[it];
      if (cpd.kind) store_planes4(cpd, o0 + (size_t)it * 4 * e.ldc, v[it], &cpl_over);
    }
  }
  if (cpd.kind == 2 && cpd.range) range_flush(cpd.range, cpd.site, cpl_over);
  if (plain) return;
  if (e.stat_sum) {
    // training-mode BatchNorm partial statistics of this 64-row block (sum and M2 about the block's own mean); lanes l,
    // l^16, l^32, l^48 hold the same four columns: fixed-order butterfly
    if (EDGE) {
#pragma unroll
      for (int it = 0; it < 16; ++it)
        if (!ok(it)) v[it] = zero4;
    }
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int it = 0; it < 16; ++it) { s.x += v[it].x; s.y += v[it].y; s.z += v[it].z; s.w += v[it].w; }
    s = xadd_rows(s);
    const int cnt = EDGE ? max(0, min(64, nrows)) : 64;
    const float inv = cnt > 0 ? 1.0f / (float)cnt : 0.f;
    const float4 mean = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
    // corrected two-pass form (Chan, Golub, LeVeque): the fp32 mean misses the true one by a rounding d0, which adds
    // cnt d0^2 to the plain sum of squares -- all there is on a constant column; (sum d)^2 / cnt takes it out again.
    // Only here: pl_gemm_planes_raw hands these partials to its caller, and they are held to an M2 floor of their own
    // (K 2^-24 n s^2 u, tests/test_gpu_bn_conditioning.py c.).  The fp32 routes' partials (gemm_epilogue.h, gemm_thin.hip,
    // skinny.hip, small_layer.hip) keep the plain sum about the group mean: they only feed the finalize, where cnt d0^2 is
    // second order -- d0 <~ 2^-24 |mean| rounding units, so d0^2 / s^2 ~ u^2 against the stated u for mean, rstd and zhat.
    float4 m2 = make_float4(0.f, 0.f, 0.f, 0.f), sd = m2;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      if (EDGE && !ok(it)) continue;
      const float dx = v[it].x - mean.x, dy = v[it].y - mean.y, dz = v[it].z - mean.z, dw = v[it].w - mean.w;
      m2.x = fmaf(dx, dx, m2.x); m2.y = fmaf(dy, dy, m2.y); m2.z = fmaf(dz, dz, m2.z); m2.w = fmaf(dw, dw, m2.w);
      sd.x += dx; sd.y += dy; sd.z += dz; sd.w += dw;
    }
    m2 = xadd_rows(m2);
    sd = xadd_rows(sd);
    m2.x = relu_f(fmaf(-sd.x * inv, sd.x, m2.x)); m2.y = relu_f(fmaf(-sd.y * inv, sd.y, m2.y));
    m2.z = relu_f(fmaf(-sd.z * inv, sd.z, m2.z)); m2.w = relu_f(fmaf(-sd.w * inv, sd.w, m2.w));
    // (the consumers walk 2 ceil(M / 128) groups, empty ones included -- gemm_stat_groups; a wave block of a 256-row tile
    //  below that has no group)
    if (lr == 0 && cok && (!EDGE || (m0 >> 6) + wm < 2 * ((e.M + 127) >> 7))) {
      const size_t o = (size_t)((m0 >> 6) + wm) * e.N + col0;
      *reinterpret_cast<float4*>(e.stat_sum + o) = s;
      *reinterpret_cast<float4*>(e.stat_m2 + o) = m2;
    }
  }
  if (e.bnr_z) {
    // BatchNorm-backward pass 1 of the layer below on the block just produced (GemmArgs::bnr_*): the separate pass read
    // g (16.8 MB) back from HBM, here it is in registers.  One partial row per 64-row block, in a fixed order.
    const int N = e.N;
    const int wpr = ((N + 255) >> 8) * 4;
    const int strip = col0 >> 8, bit = (col0 & 255) >> 2;
    const float4 mu = *reinterpret_cast<const float4*>(e.bnr_mean + col0);
    const float4 rs = *reinterpret_cast<const float4*>(e.bnr_rstd + col0);
    const float ks = e.bnr_kscale;
    float4 zz[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) zz[it] = *reinterpret_cast<const float4*>(e.bnr_z + o0 + (size_t)it * 4 * e.ldc);
    float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
    float mxd = 0.f, mxz = 0.f;
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const uint64_t* bw = e.bnr_bits + (size_t)(row0 + 4 * it) * wpr + strip * 4;
      const ulonglong2 w01 = *reinterpret_cast<const ulonglong2*>(bw), w23 = *reinterpret_cast<const ulonglong2*>(bw + 2);
      const float d0 = ((w01.x >> bit) & 1ull) ? v[it].x * ks : 0.f;
      const float d1 = ((w01.y >> bit) & 1ull) ? v[it].y * ks : 0.f;
      const float d2 = ((w23.x >> bit) & 1ull) ? v[it].z * ks : 0.f;
      const float d3 = ((w23.y >> bit) & 1ull) ? v[it].w * ks : 0.f;
      const float z0 = (zz[it].x - mu.x) * rs.x, z1 = (zz[it].y - mu.y) * rs.y;
      const float z2 = (zz[it].z - mu.z) * rs.z, z3 = (zz[it].w - mu.w) * rs.w;
      s1.x += d0; s1.y += d1; s1.z += d2; s1.w += d3;
      s2.x = fmaf(d0, z0, s2.x); s2.y = fmaf(d1, z1, s2.y); s2.z = fmaf(d2, z2, s2.z); s2.w = fmaf(d3, z3, s2.w);
      mxd = fmaxf(fmaxf(mxd, fmaxf(fabsf(d0), fabsf(d1))), fmaxf(fabsf(d2), fabsf(d3)));
      mxz = fmaxf(fmaxf(mxz, fmaxf(fabsf(z0), fabsf(z1))), fmaxf(fabsf(z2), fabsf(z3)));
    }
    s1 = xadd_rows(s1);
    s2 = xadd_rows(s2);
    const int rg = (m0 >> 6) + wm;                   // 64-row block of the whole matrix
    if (lr == 0) {
      *reinterpret_cast<float4*>(e.bnr_part_dy + (size_t)rg * N + col0) = s1;
      *reinterpret_cast<float4*>(e.bnr_part_dyz + (size_t)rg * N + col0) = s2;
    }
    if (e.bnr_amax) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { mxd = fmaxf(mxd, __shfl_xor(mxd, o)); mxz = fmaxf(mxz, __shfl_xor(mxz, o)); }
      if (lane == 0) {
        float* q = e.bnr_amax + ((size_t)rg * (N >> 6) + (n0 >> 6) + wn) * 2;
        q[0] = mxd; q[1] = mxz;
      }
    }
  }
}

// The 16x16x32 main loop (gemm_planes16.h) and the staged epilogue for everything.
// EDGE: M / N need not be multiples of 128 -- the conv path's 64-wide layers and ragged pixel counts
// CONV: 1 = A gathered as a convolution input (NT), 2 = B gathered for the weight gradient (TN)
// PERSIST: the workgroup walks a run of work items, operands streaming across the item boundaries (gemm_planes16.h); the
// epilogue then stages through LDS of its own behind the three-stage ring.
template <int MODE, int NST = 3> constexpr int ring_bytes() { return plp::PlanesCfg<32, plp::ModeCfg<MODE>::NPL, NST>::LDS; }
// the 256 x 64 tile (gemm_planes16.h T64): A image 256 rows, B image 64 rows of 64 B per plane and stage, three stages
template <int MODE> constexpr int t64_ring_bytes() { return 3 * plp::ModeCfg<MODE>::NPL * (256 + 64) * 64; }
// the staged epilogue takes the wave's 64x64 block through LDS in 64 / ER passes of ER rows x 68 floats per wave
template <int ER> constexpr int stage_bytes() { return 4 * ER * 68 * 4; }
// ring depth of the persistent form.  (Measured with 4 stages + 16-row staging passes for f16x3, 6 for bf16: the K = 64
// layer 372 us against 379 us with 3 -- the ring is not what those launches wait for)
template <int MODE> constexpr int persist_nst() { return 3; }
constexpr int kPersistRows = 32;
template <int MODE> constexpr int wide_ring_bytes() { return plp::WideCfg<plp::ModeCfg<MODE>::NPL>::LDS; }
constexpr int kWidePersistRows = 16;              // 2 x 64 KB of pair-stages leave 32 KB: the staged epilogue in 16-row passes
template <int MODE, bool PERSIST = false, bool WIDE = false, bool T64 = false>
constexpr int lds_bytes() {
  if (T64) return PERSIST ? t64_ring_bytes<MODE>() + stage_bytes<kPersistRows>()
                          : (t64_ring_bytes<MODE>() > stage_bytes<32>() ? t64_ring_bytes<MODE>() : stage_bytes<32>());
  if (WIDE) return PERSIST ? wide_ring_bytes<MODE>() + stage_bytes<kWidePersistRows>()
                           : (wide_ring_bytes<MODE>() > stage_bytes<32>() ? wide_ring_bytes<MODE>() : stage_bytes<32>());
  if (PERSIST) return ring_bytes<MODE, persist_nst<MODE>()>() + stage_bytes<kPersistRows>();
  // the operand ring, and never less than 4 x 17 KB (a whole 64x64 block per wave: what the removed 32x32x16 loop's
  // epilogue staged; the one-item kernels' LDS, and with it their occupancy, is kept as measured)
  return ring_bytes<MODE>() > 4 * 64 * 68 * 4 ? ring_bytes<MODE>() : 4 * 64 * 68 * 4;
}
static_assert(lds_bytes<plp::kF16x3, true>() <= 160 * 1024 && lds_bytes<plp::kBf16, true>() <= 160 * 1024, "LDS per CU");
static_assert(lds_bytes<plp::kF16x3, true, true>() <= 160 * 1024 && lds_bytes<plp::kF16x3, false, true>() <= 160 * 1024, "LDS per CU");
static_assert(lds_bytes<plp::kF16x3, true, false, true>() <= 160 * 1024, "LDS per CU");

template <bool A_KS, bool B_KS, int MODE, bool EDGE = false, int CONV = 0, bool PERSIST = false, bool WIDE = false,
          bool T64 = false>
__device__ __forceinline__ void planes_body(const PlanesKern& k, const int block_id, const int nblocks, const int nwork, char* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = T64 ? (wave & 3) : (wave & 3) >> 1, wn = T64 ? 0 : (wave & 1);
  // main + low / 2048, then back from the operands' power-of-two scales (exact unless the result under/overflows)
  const float os = MODE == plp::kF16x3 ? (k.dyn_inv ? k.out_scale * k.dyn_inv[0] : k.out_scale) : 1.f;
  // the wave's 64x64 block goes through ER rows x 68 floats of LDS in 64 / ER passes: the lane that owned accumulator
  // elements leaves with float4 rows (v[it] = row 4 it + (lane >> 4), columns 4 (lane & 15) ..)
  constexpr int NST = PERSIST ? persist_nst<MODE>() : 3;
  constexpr int ER = PERSIST ? (WIDE ? kWidePersistRows : kPersistRows) : 32;
  constexpr int RING = T64 ? t64_ring_bytes<MODE>() : (WIDE ? wide_ring_bytes<MODE>() : ring_bytes<MODE, NST>());
  float* ldsw = reinterpret_cast<float*>(lds + (PERSIST ? RING : 0)) + (wave & 3) * ER * 68;
  const int q = lane >> 4, c = lane & 15, lc = c * 4;
  auto epi = [&](plp::f32x4v (&acc)[plp::ModeCfg<MODE>::NACC][4][4], const int m0, const int n0, const int slice) {
    if (!PERSIST) __syncthreads();                     // every computing wave is done reading operand tiles (the staging
                                                       // rows alias the ring); PERSIST: a region of its own, wave-private
    float4 v[16];
#pragma unroll
    for (int pass = 0; pass < 64 / ER; ++pass) {
#pragma unroll
      for (int r2 = 0; r2 < ER / 16; ++r2)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float x = acc[0][pass * (ER / 16) + r2][ct][r];
            if constexpr (MODE == plp::kF16x3) x = fmaf(acc[1][pass * (ER / 16) + r2][ct][r], 1.0f / plp::kF16LoScale, x) * os;
            ldsw[(r2 * 16 + 4 * q + r) * 68 + ct * 16 + c] = x;
          }
#pragma unroll
      for (int it = 0; it < ER / 4; ++it)
        v[pass * (ER / 4) + it] = *reinterpret_cast<const float4*>(ldsw + (it * 4 + q) * 68 + lc);
    }
    float* C = k.e.C ? k.e.C + (k.e.split_k > 1 ? (size_t)slice * k.e.M * k.e.ldc : 0) : nullptr;
    staged_epilogue<EDGE>(k, C, v, m0, n0, wm, wn, lane);
  };
  if constexpr (WIDE) plp::planes_run16w<A_KS, B_KS, MODE, EDGE, CONV, PERSIST>(k.p, block_id, nblocks, nwork, lds, epi);
  else plp::planes_run16<A_KS, B_KS, MODE, EDGE, CONV, PERSIST, NST, T64>(k.p, block_id, nblocks, nwork, lds, epi);
}

template <bool A_KS, bool B_KS, int MODE, bool EDGE = false, int CONV = 0>
__global__ __launch_bounds__(512) void planes_gemm_kernel(PlanesKern k) {
  __shared__ __attribute__((aligned(16))) char lds[lds_bytes<MODE>()];
  planes_body<A_KS, B_KS, MODE, EDGE, CONV>(k, blockIdx.x, gridDim.x, gridDim.x, lds);
}

// one workgroup per CU, each walking nwork / gridDim.x consecutive work items (NT, 16x16x32 loop)
template <int MODE, bool EDGE, int CONV>
__global__ __launch_bounds__(512) void planes_gemm_persistent_kernel(PlanesKern k, int nwork) {
  __shared__ __attribute__((aligned(16))) char lds[lds_bytes<MODE, true>()];
  planes_body<false, false, MODE, EDGE, CONV, true>(k, blockIdx.x, gridDim.x, nwork, lds);
}

// NT on 256-row x 64-column tiles (gemm_planes16.h T64): the 64-channel layers
template <int MODE, bool EDGE, int CONV, bool PERSIST>
__global__ __launch_bounds__(512) void planes_gemm_t64_kernel(PlanesKern k, int nwork) {
  __shared__ __attribute__((aligned(16))) char lds[lds_bytes<MODE, PERSIST, false, true>()];
  planes_body<false, false, MODE, EDGE, CONV, PERSIST, false, true>(k, blockIdx.x, gridDim.x, nwork, lds);
}

// NT with the k-tiles staged in pairs (whole 128-byte lines of both k-contiguous operands: gemm_planes16.h, WIDE);
// PERSIST: nwork items over gridDim.x workgroups, else one item per workgroup (nwork == gridDim.x)
template <int MODE, bool EDGE, int CONV, bool PERSIST>
__global__ __launch_bounds__(512) void planes_gemm_wide_kernel(PlanesKern k, int nwork) {
  __shared__ __attribute__((aligned(16))) char lds[lds_bytes<MODE, PERSIST, true>()];
  planes_body<false, false, MODE, EDGE, CONV, PERSIST, true>(k, blockIdx.x, gridDim.x, nwork, lds);
}

// the wave's 64x64 accumulator block -> float4 rows through ER rows x 68 floats of LDS (64 / ER passes), then the staged epilogue
template <int MODE, int ER, bool EDGE>
__device__ __forceinline__ void acc_epilogue(const PlanesKern& k, plp::f32x4v (&acc)[plp::ModeCfg<MODE>::NACC][4][4], float* ldsw,
                                             const int m0, const int n0, const int slice, const int wm, const int wn, const int lane) {
  const float os = MODE == plp::kF16x3 ? (k.dyn_inv ? k.out_scale * k.dyn_inv[0] : k.out_scale) : 1.f;
  const int q = lane >> 4, c = lane & 15, lc = c * 4;
  float4 v[16];
#pragma unroll
  for (int pass = 0; pass < 64 / ER; ++pass) {
#pragma unroll
    for (int r2 = 0; r2 < ER / 16; ++r2)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = acc[0][pass * (ER / 16) + r2][ct][r];
          if constexpr (MODE == plp::kF16x3) x = fmaf(acc[1][pass * (ER / 16) + r2][ct][r], 1.0f / plp::kF16LoScale, x) * os;
          ldsw[(r2 * 16 + 4 * q + r) * 68 + ct * 16 + c] = x;
        }
#pragma unroll
    for (int it = 0; it < ER / 4; ++it)
      v[pass * (ER / 4) + it] = *reinterpret_cast<const float4*>(ldsw + (it * 4 + q) * 68 + lc);
  }
  float* C = k.e.C ? k.e.C + (k.e.split_k > 1 ? (size_t)slice * k.e.M * k.e.ldc : 0) : nullptr;
  staged_epilogue<EDGE>(k, C, v, m0, n0, wm, wn, lane);
}

// dX's epilogue of the chained pair, handed from computing wave w to loader wave 4 + w (gemm_planes16.h HAND-OFF): what
// staged_epilogue<false> does for a dX problem -- skip-gradient addend, the g store, BatchNorm-backward pass 1 of the layer
// below (the host takes this form for nothing else: chain_hand_ok) -- one row-quad `it` at a time.  `blk` is the 64 x 64
// block of the wave this lane writes (computing) or stands in for (loader); lane (lr = lane >> 4, lc = 4 (lane & 15)) of the
// loader owns what staged_epilogue's lane owns, every element sees the same operations in the same order, the column sums run
// over it = 0 .. 15 in registers and leave through the same butterfly.
// ADD / BNR: addend / bnr_* present -- compile-time, so that every step issues a fixed number of vector-memory operations.
struct NoHand { static constexpr bool kOn = false; };
template <int MODE, bool ADD, bool BNR>
struct ChainHand {
  static constexpr bool kOn = true;
  static constexpr int D = plp::kChainAhead;
  // vector-memory operations of chunk(J): the loads of row-quad J, the g store of row-quad J - D
  static constexpr int vm_ops(int j) {
    return (j >= 0 && j < plp::kChainChunks ? (ADD ? 1 : 0) + (BNR ? 3 : 0) : 0) + (j >= D && j - D < plp::kChainChunks ? 1 : 0);
  }
  const PlanesKern& k;
  float* blk;
  int lane;
  size_t o0 = 0;
  int rg = 0, cb = 0, col0 = 0, wpr = 0, bit = 0;
  const uint64_t* bw0 = nullptr;
  float4 mu, rs, s1, s2;
  float mxd = 0.f, mxz = 0.f;
  float4 qa[D], zz[D];                             // row-quads in flight (slot = row-quad % D; the indices are compile-time):
  ulonglong2 w01[D], w23[D];                       // addend, saved z, the bitmap's four words

  __device__ __forceinline__ ChainHand(const PlanesKern& k_, float* blk_, int lane_) : k(k_), blk(blk_), lane(lane_) {}

  // computing wave: the block as acc_epilogue stages it, in the accumulator layout (row 16 rt + 4 q + r, column 16 ct + c)
  __device__ __forceinline__ void put(plp::f32x4v (&acc)[plp::ModeCfg<MODE>::NACC][4][4]) const {
    const float os = MODE == plp::kF16x3 ? (k.dyn_inv ? k.out_scale * k.dyn_inv[0] : k.out_scale) : 1.f;
    const int q = lane >> 4, c = lane & 15;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float x = acc[0][rt][ct][r];
          if constexpr (MODE == plp::kF16x3) x = fmaf(acc[1][rt][ct][r], 1.0f / plp::kF16LoScale, x) * os;
          blk[plp::hand_idx(rt * 16 + 4 * q + r, ct * 16 + c)] = x;
        }
  }

  // loader wave, before item 1's first step
  __device__ __forceinline__ void begin(const int m0, const int n0, const int wm, const int wn) {
    const GemmArgs& e = k.e;
    const int lr = lane >> 4, lc = (lane & 15) * 4;
    const int row0 = m0 + wm * 64 + lr;
    col0 = n0 + wn * 64 + lc;
    o0 = (size_t)row0 * e.ldc + col0;
    rg = (m0 >> 6) + wm;                           // 64-row block of the whole matrix
    cb = (n0 >> 6) + wn;
    s1 = make_float4(0.f, 0.f, 0.f, 0.f); s2 = s1;
    if constexpr (BNR) {
      wpr = ((e.N + 255) >> 8) * 4;
      bit = (col0 & 255) >> 2;
      bw0 = e.bnr_bits + (size_t)row0 * wpr + (col0 >> 8) * 4;
      mu = *reinterpret_cast<const float4*>(e.bnr_mean + col0);
      rs = *reinterpret_cast<const float4*>(e.bnr_rstd + col0);
    }
  }

  template <int J>
  __device__ __forceinline__ void chunk(std::integral_constant<int, J>) {
    const GemmArgs& e = k.e;
    float4 nq, nz;
    ulonglong2 n01, n23;
    if constexpr (J < plp::kChainChunks) {
      const size_t o = o0 + (size_t)J * 4 * e.ldc;
      if constexpr (ADD) nq = *reinterpret_cast<const float4*>(e.addend + o);
      if constexpr (BNR) {
        nz = *reinterpret_cast<const float4*>(e.bnr_z + o);
        const uint64_t* bw = bw0 + (size_t)(4 * J) * wpr;
        n01 = *reinterpret_cast<const ulonglong2*>(bw);
        n23 = *reinterpret_cast<const ulonglong2*>(bw + 2);
      }
    }
    if constexpr (J >= D && J - D < plp::kChainChunks) {
      constexpr int it = J - D, sl = it % D;
      // (the read as an instruction of its own: hipcc lets no LDS load it knows of pass an LDS-DMA that might alias it -- it put
      //  vmcnt(loads of this step) in front of a plain load, i.e. waited for the k-tile issued a moment ago, every step)
      plp::f32x4v hv;
      const uint32_t ha = (uint32_t)(size_t)(__attribute__((address_space(3))) float*)(blk + plp::hand_idx(4 * it + (lane >> 4), (lane & 15) * 4));
      asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(hv) : "v"(ha) : "memory");
      float4 v = make_float4(hv[0], hv[1], hv[2], hv[3]);
      if constexpr (ADD) { v.x += qa[sl].x; v.y += qa[sl].y; v.z += qa[sl].z; v.w += qa[sl].w; }
      float* dst = e.C + o0 + (size_t)it * 4 * e.ldc;
      if (k.nt_store) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f4v q = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(q, reinterpret_cast<f4v*>(dst));
      } else {
        *reinterpret_cast<float4*>(dst) = v;
      }
      if constexpr (BNR) {
        const float ks = e.bnr_kscale;
        const float d0 = ((w01[sl].x >> bit) & 1ull) ? v.x * ks : 0.f;
        const float d1 = ((w01[sl].y >> bit) & 1ull) ? v.y * ks : 0.f;
        const float d2 = ((w23[sl].x >> bit) & 1ull) ? v.z * ks : 0.f;
        const float d3 = ((w23[sl].y >> bit) & 1ull) ? v.w * ks : 0.f;
        const float z0 = (zz[sl].x - mu.x) * rs.x, z1 = (zz[sl].y - mu.y) * rs.y;
        const float z2 = (zz[sl].z - mu.z) * rs.z, z3 = (zz[sl].w - mu.w) * rs.w;
        s1.x += d0; s1.y += d1; s1.z += d2; s1.w += d3;
        s2.x = fmaf(d0, z0, s2.x); s2.y = fmaf(d1, z1, s2.y); s2.z = fmaf(d2, z2, s2.z); s2.w = fmaf(d3, z3, s2.w);
        mxd = fmaxf(fmaxf(mxd, fmaxf(fabsf(d0), fabsf(d1))), fmaxf(fabsf(d2), fabsf(d3)));
        mxz = fmaxf(fmaxf(mxz, fmaxf(fabsf(z0), fabsf(z1))), fmaxf(fabsf(z2), fabsf(z3)));
        // the sums are read after the loop only: without this hipcc sinks the whole chain down there and keeps sixteen
        // row-quads of loaded z and bitmap words alive for it (23-31 VGPRs spilled: scratch traffic inside the counted steps)
        asm volatile("" : "+v"(s1.x), "+v"(s1.y), "+v"(s1.z), "+v"(s1.w), "+v"(s2.x), "+v"(s2.y), "+v"(s2.z), "+v"(s2.w),
                          "+v"(mxd), "+v"(mxz));
      }
    }
    if constexpr (J < plp::kChainChunks) {
      if constexpr (ADD) qa[J % D] = nq;
      if constexpr (BNR) { zz[J % D] = nz; w01[J % D] = n01; w23[J % D] = n23; }
    }
  }

  // loader wave, after the last barrier: one partial row per 64-row block, in staged_epilogue's order
  __device__ __forceinline__ void finish() {
    if constexpr (BNR) {
      const GemmArgs& e = k.e;
      const int N = e.N;
      s1 = xadd_rows(s1);
      s2 = xadd_rows(s2);
      if ((lane >> 4) == 0) {
        *reinterpret_cast<float4*>(e.bnr_part_dy + (size_t)rg * N + col0) = s1;
        *reinterpret_cast<float4*>(e.bnr_part_dyz + (size_t)rg * N + col0) = s2;
      }
      if (e.bnr_amax) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mxd = fmaxf(mxd, __shfl_xor(mxd, o)); mxz = fmaxf(mxz, __shfl_xor(mxz, o)); }
        if (lane == 0) {
          float* q = e.bnr_amax + ((size_t)rg * (N >> 6) + cb) * 2;
          q[0] = mxd; q[1] = mxz;
        }
      }
    }
  }
};

// the backward pair chained in one workgroup per CU (gemm_planes16.h CHAIN): grid = the number of dX tiles = dW items.
// HAND: dX's epilogue on the loader waves, under dW's MFMAs (ADD / BNR: what that epilogue holds); else both epilogues on the
// computing waves, staged through 34 KB behind the ring.
template <int MODE, bool HAND, bool ADD = false, bool BNR = false>
__global__ __launch_bounds__(512) void planes_gemm_chain_kernel(PlanesKern k0, PlanesKern k1, plp::SlabRide ride) {
  constexpr int BEHIND = HAND ? plp::kHandBytes : stage_bytes<32>();
  static_assert(ring_bytes<MODE>() + BEHIND <= 160 * 1024 && stage_bytes<32>() <= plp::kHandBytes, "LDS per CU");
  __shared__ __attribute__((aligned(16))) char lds[ring_bytes<MODE>() + BEHIND];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave & 3) >> 1, wn = wave & 1;
  // (HAND: dW's epilogue stages through the hand-off blocks, which the loaders left before the loop's last barriers)
  float* ldsw = reinterpret_cast<float*>(lds + ring_bytes<MODE>()) + (wave & 3) * 32 * 68;
  auto epi0 = [&](plp::f32x4v (&acc)[plp::ModeCfg<MODE>::NACC][4][4], const int m0, const int n0, const int slice) {
    if constexpr (!HAND) acc_epilogue<MODE, 32, false>(k0, acc, ldsw, m0, n0, slice, wm, wn, lane);
  };
  auto epi1 = [&](plp::f32x4v (&acc)[plp::ModeCfg<MODE>::NACC][4][4], const int m0, const int n0, const int slice) {
    acc_epilogue<MODE, 32, false>(k1, acc, ldsw, m0, n0, slice, wm, wn, lane);
  };
  if constexpr (HAND) {
    ChainHand<MODE, ADD, BNR> hand(k0, reinterpret_cast<float*>(lds + ring_bytes<MODE>()) + (wave & 3) * 64 * 64, lane);
    plp::planes_run16_chain<MODE>(k0.p, k1.p, ride, blockIdx.x, gridDim.x, lds, hand, epi0, epi1);
  } else {
    NoHand hand;
    plp::planes_run16_chain<MODE>(k0.p, k1.p, ride, blockIdx.x, gridDim.x, lds, hand, epi0, epi1);
  }
}

// backward pair of one layer in one launch: workgroups [0, n0) run dX = dz W (NN), the rest dW = dz^T a (TN, split-K
// slabs).  One workgroup per CU at a time (96 KB of LDS each): what the single launch saves is the launch boundary
// and the tail of the first problem, which the second one's workgroups fill.
// (Tried: alternating the two problems in groups of 8 workgroups, so that half the CUs run dX's heavy epilogues beside the
//  other half's main loops -- same-box A/B 0.688 vs 0.629 ms per step: two working sets per XCD L2 cost far more.)
// (Tried in round 3: the two problems taking turns PER XCD -- XCDs 0-3 run their share
//  of dX first and of dW second, XCDs 4-7 the other way round (blocks b and b + 8 share an XCD and are dispatched in order), so
//  that each L2 still holds ONE problem's working set at a time while dX's 50 MB epilogue burst comes in two halves, each
//  beside the other half's main loops.  Same-box A/B over three interleaved runs: 68.5 us per dual launch against 65.1 us,
//  0.650 against 0.638 ms per step.  Not kept -- the burst is not what a half-chip of main loops can hide.)
template <int MODE>
__global__ __launch_bounds__(512) void planes_gemm_dual_kernel(PlanesKern k0, PlanesKern k1, int n0) {
  __shared__ __attribute__((aligned(16))) char lds[lds_bytes<MODE>()];
  const int b = blockIdx.x;
  if (b < n0)
    planes_body<false, true, MODE>(k0, b, n0, n0, lds);
  else
    planes_body<true, true, MODE>(k1, b - n0, gridDim.x - n0, gridDim.x - n0, lds);
}

PlanesKern kern_of(const PlanesGemmArgs& a) {
  PlanesKern k = {};
  k.p.A = reinterpret_cast<const __bf16*>(a.A);
  k.p.B = reinterpret_cast<const __bf16*>(a.B);
  k.p.C = a.e.C;
  k.p.M = a.e.M; k.p.N = a.e.N; k.p.K = a.e.K;
  k.p.lda = a.lda; k.p.ldb = a.ldb; k.p.ldc = a.e.ldc;
  k.p.split_k = a.e.split_k;
  k.p.a_plane = (size_t)a.a_plane; k.p.b_plane = (size_t)a.b_plane;
  k.e = a.e;
  k.p.cv_cin = a.e.conv_cin; k.p.cv_h = a.e.conv_h; k.p.cv_w = a.e.conv_w; k.p.cv_ho = a.e.conv_ho; k.p.cv_wo = a.e.conv_wo;
  k.p.cv_kw = a.e.conv_kw; k.p.cv_stride = a.e.conv_stride; k.p.cv_pad_h = a.e.conv_pad_h; k.p.cv_pad_w = a.e.conv_pad_w;
  k.p.cv_stride_w = a.e.conv_stride_w > 0 ? a.e.conv_stride_w : a.e.conv_stride;
  k.out_scale = a.out_scale;
  k.dyn_inv = a.dyn_inv;
  k.nt_store = (int64_t)a.e.M * a.e.N * 4 >= kNontemporalBytes ? 1 : 0;
  return k;
}

// CUs of the current device (the persistent form launches one workgroup per CU)
int cu_count() {
  static int cached[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  if (!cached[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

int splits_of(const GemmArgs& e) { return e.split_k > 1 ? e.split_k : 1; }
int grid_of(const PlanesGemmArgs& a) { return ((a.e.M + 127) / 128) * ((a.e.N + 127) / 128) * splits_of(a.e); }
bool is_edge(const PlanesGemmArgs& a) { return (a.e.M % 128) != 0 || (a.e.N % 128) != 0; }

// One planes GEMM as planes_route decided it: every kernel template is named here and nowhere else.
template <int MODE>
int launch_routed(GemmLayout layout, const PlanesRoute& r, const PlanesKern& k, hipStream_t s) {
  const dim3 grid(r.grid), block(512);
  // the (EDGE, CONV) forms of the NT families: whole <false, 0>, overhanging <true, 0>, gathered A <true, 1>
  auto nt_form = [&](auto launch) {
    if (r.conv) launch(Bool<true>{}, Int<1>{});
    else if (r.edge) launch(Bool<true>{}, Int<0>{});
    else launch(Bool<false>{}, Int<0>{});
  };
  auto persist_form = [&](auto launch) {
    if (r.persist) launch(Bool<true>{}); else launch(Bool<false>{});
  };
  switch (r.family) {
    case PlanesFamily::T64:
      nt_form([&](auto E, auto C) {
        persist_form([&](auto P) {
          hipLaunchKernelGGL((planes_gemm_t64_kernel<MODE, decltype(E)::value, decltype(C)::value, decltype(P)::value>), grid, block,
                             0, s, k, r.nwork);
        });
      });
      return PL_OK;
    case PlanesFamily::Wide:
      nt_form([&](auto E, auto C) {
        persist_form([&](auto P) {
          hipLaunchKernelGGL((planes_gemm_wide_kernel<MODE, decltype(E)::value, decltype(C)::value, decltype(P)::value>), grid, block,
                             0, s, k, r.nwork);
        });
      });
      return PL_OK;
    case PlanesFamily::Persistent:
      nt_form([&](auto E, auto C) {
        hipLaunchKernelGGL((planes_gemm_persistent_kernel<MODE, decltype(E)::value, decltype(C)::value>), grid, block, 0, s, k,
                           r.nwork);
      });
      return PL_OK;
    case PlanesFamily::OneItem: break;
  }
  // one item per workgroup, any layout: whole or overhanging, and the layout's gathered form GATHER (NT 1, TN 2, NN none)
  auto one_item = [&](auto AKS, auto BKS, auto GATHER) {
    auto launch = [&](auto E, auto C) {
      hipLaunchKernelGGL((planes_gemm_kernel<decltype(AKS)::value, decltype(BKS)::value, MODE, decltype(E)::value, decltype(C)::value>),
                         grid, block, 0, s, k);
    };
    if constexpr (decltype(GATHER)::value != 0) {
      if (r.conv) return launch(Bool<true>{}, GATHER);
    }
    if (r.edge) launch(Bool<true>{}, Int<0>{}); else launch(Bool<false>{}, Int<0>{});
  };
  switch (layout) {
    case kNT: one_item(Bool<false>{}, Bool<false>{}, Int<1>{}); break;
    case kNN: one_item(Bool<false>{}, Bool<true>{}, Int<0>{}); break;
    case kTN: one_item(Bool<true>{}, Bool<true>{}, Int<2>{}); break;
    default: PL_FAIL(PL_EINVAL, "gemm_planes: bad layout %d", (int)layout);
  }
  return PL_OK;
}

// the backward pair: chained (one workgroup per dX tile that goes on to a dW item, operands streaming across) or side by side
// ChainHand: the chained kernel with dX's epilogue on the loader waves (gemm_planes16.h HAND-OFF)
enum class PairRoute { Chain, ChainHand, Dual };
// what ChainHand's epilogue covers: a plain g store with, at most, the skip-gradient addend and BatchNorm-backward pass 1
bool chain_hand_ok(const GemmArgs& e) {
  return e.C && splits_of(e) == 1 && !e.bias && !e.col_scale && !e.relu && !e.resid && !e.cpl_kind && !e.stat_sum && !e.scat_on;
}
PairRoute pair_route(const PlanesGemmArgs& nn, const PlanesGemmArgs& tn) {
  const int ts = splits_of(tn.e);
  const bool chain = grid_of(nn) == grid_of(tn) && nn.e.K % 32 == 0 && nn.e.K >= 64 && tn.e.K % (32 * ts) == 0 && tn.e.K >= 32 * ts;
  if (!chain) return PairRoute::Dual;
  // the hand-off spreads dX's epilogue over k-steps 2 .. 2 + kChainChunks of every dW slice and must be done before the
  // slice's last step: nk1 = K1 / (32 splits) >= kChainMinNk1 (20: H >= 640 in the lifter); shorter slices keep the epilogue
  // on the computing waves
  const int nk1 = tn.e.K / (32 * ts);
  return nk1 >= plp::kChainMinNk1 && chain_hand_ok(nn.e) ? PairRoute::ChainHand : PairRoute::Chain;
}
// Can the pair's launch carry a split-K sum -- `slabs` slabs of n floats -- on its loader waves (gemm_planes16.h SLAB RIDE)?
// Only the hand-off form has the ride; its arithmetic exists for four slabs; the float4s are dealt kRideChunks to a loader
// lane over grid x 4 waves x 64 lanes, exactly (which, chained, means B = H x 4: the lifter's H = 1024 at B = 4096); and
// the ride's kRideChunks + kChainAhead steps, from loader iteration kRideFirst on, must lie within dX's nk0 - 2 iterations.
bool pair_carries_slab_sum(const PlanesGemmArgs& nn, const PlanesGemmArgs& tn, int slabs, int64_t n) {
  if (pair_route(nn, tn) != PairRoute::ChainHand) return false;
  const int nk0 = nn.e.K / 32;
  return slabs == plp::kRideSlabs && n == (int64_t)plp::kRideChunks * 4 * 64 * 4 * grid_of(nn) && nk0 >= plp::kRideMinNk0;
}
template <int MODE>
void launch_pair(PairRoute r, const PlanesKern& k0, const PlanesKern& k1, const plp::SlabRide& ride, int g0, int g1, hipStream_t s) {
  const dim3 block(512);
  if (r == PairRoute::ChainHand) {
    auto launch = [&](auto ADD, auto BNR) {
      hipLaunchKernelGGL((planes_gemm_chain_kernel<MODE, true, decltype(ADD)::value, decltype(BNR)::value>), dim3(g0), block, 0, s, k0, k1,
                         ride);
    };
    auto with_bnr = [&](auto ADD) { if (k0.e.bnr_z) launch(ADD, Bool<true>{}); else launch(ADD, Bool<false>{}); };
    if (k0.e.addend) with_bnr(Bool<true>{}); else with_bnr(Bool<false>{});
  } else if (r == PairRoute::Chain) {
    hipLaunchKernelGGL((planes_gemm_chain_kernel<MODE, false>), dim3(g0), block, 0, s, k0, k1, plp::SlabRide{});
  } else {
    hipLaunchKernelGGL((planes_gemm_dual_kernel<MODE>), dim3(g0 + g1), block, 0, s, k0, k1, g0);
  }
}

}  // namespace

// whole 128x128 tiles, every K slice a whole number of 32-k tiles, 16-byte aligned plane rows, and every byte
// offset the DMA's 32-bit scalar offset has to hold below 2^31
bool planes_gemm_ok(GemmLayout layout, const PlanesGemmArgs& a) {
  const GemmArgs& e = a.e;
  const int splits = splits_of(e);
  if (a.mode != plp::kBf16 && a.mode != plp::kF16x3) return false;
  if (!a.A || !a.B || (!e.C && !e.cpl_kind) || e.M <= 0 || e.N <= 0 || e.K <= 0) return false;
  if (e.cpl_kind && (splits > 1 || !e.cpl_h || (e.cpl_kind == 2 && !e.cpl_l) ||
                     ((reinterpret_cast<uintptr_t>(e.cpl_h) | reinterpret_cast<uintptr_t>(e.cpl_l)) & 7)))
    return false;
  if (e.K % (32 * splits)) return false;
  if (e.conv_cin) {
    // implicit-GEMM convolution: NT with A gathered (forward / data gradient) or TN with B gathered (weight gradient);
    // the gathered tensor's bytes (every plane) must fit the DMA's 32-bit offsets
    if ((layout != kNT && layout != kTN) || e.bnr_z) return false;
    if (e.conv_h <= 0 || e.conv_w <= 0 || e.conv_ho <= 0 || e.conv_wo <= 0 || e.conv_kw <= 0 || e.conv_stride <= 0) return false;
    const int64_t pixels = layout == kNT ? e.M : e.K;
    if (pixels % ((int64_t)e.conv_ho * e.conv_wo)) return false;
    const int64_t xb = pixels / ((int64_t)e.conv_ho * e.conv_wo) * e.conv_h * e.conv_w * e.conv_cin * 2;
    if (xb >= 0x7fffffe0ll) return false;
    // (8 channels: four taps of a kernel row per 32-k tile -- the stem on pixel pairs; one K slice, no pair staging)
    const bool cin8 = e.conv_cin == 8 && e.conv_kw % 4 == 0 && e.split_k <= 1;
    if (layout == kNT && !cin8 && ((e.conv_cin & 31) || e.K % e.conv_cin)) return false;
    if (e.scat_on && (layout != kNT || e.split_k > 1 || e.addend || e.resid || e.relu == 2 || e.stat_sum)) return false;
    if (layout == kTN && ((e.conv_cin & 7) || e.N % e.conv_cin)) return false;
  }
  if (e.M % 128 || e.N % 128) {
    // overhanging tiles (guarded epilogue): the source of an overhanging lane is clamped to the last valid
    // row / 8-column chunk, so a k-strided operand's extent must be a multiple of 8; no BatchNorm-backward epilogue there
    if ((e.N & 7) || (layout == kTN && (e.M & 7)) || e.bnr_z) return false;
  }
  if ((a.lda & 7) || (a.ldb & 7)) return false;
  if ((reinterpret_cast<uintptr_t>(a.A) | reinterpret_cast<uintptr_t>(a.B)) & 15) return false;
  if (((a.a_plane | a.b_plane) & 7) != 0) return false;
  const bool a_ks = layout == kTN, b_ks = layout != kNT;
  // byte offsets inside ONE plane and ONE K slice, from the tile origin (plane stride and slice origin are in the
  // descriptor's 64-bit base)
  const int64_t ks = e.K / splits;
  const int64_t a_ext = a_ks ? ks * a.lda * 2 : (int64_t)128 * a.lda * 2 + ks * 2;
  const int64_t b_ext = b_ks ? ks * a.ldb * 2 : (int64_t)128 * a.ldb * 2 + ks * 2;
  if (a_ext >= (1ll << 31) || b_ext >= (1ll << 31)) return false;
  if ((e.stat_sum != nullptr) != (e.stat_m2 != nullptr)) return false;
  if ((e.col_scale != nullptr) != (e.col_shift != nullptr)) return false;
  // the staged epilogue moves everything as 16-byte accesses
  if (e.ldc & 3) return false;
  const uintptr_t al = reinterpret_cast<uintptr_t>(e.C) | reinterpret_cast<uintptr_t>(e.bias) | reinterpret_cast<uintptr_t>(e.addend) |
                       reinterpret_cast<uintptr_t>(e.resid) | reinterpret_cast<uintptr_t>(e.col_scale) |
                       reinterpret_cast<uintptr_t>(e.col_shift) | reinterpret_cast<uintptr_t>(e.stat_sum) |
                       reinterpret_cast<uintptr_t>(e.stat_m2) | reinterpret_cast<uintptr_t>(e.bnr_z) |
                       reinterpret_cast<uintptr_t>(e.bnr_mean) | reinterpret_cast<uintptr_t>(e.bnr_rstd) |
                       reinterpret_cast<uintptr_t>(e.bnr_part_dy) | reinterpret_cast<uintptr_t>(e.bnr_part_dyz);
  if (al & 15) return false;
  return true;
}

// Which kernel family runs a problem that planes_gemm_ok accepted, in which form and on what grid.  The first
// family whose conditions hold takes it; a gathered operand (conv) implies the edge form in every family -- the gathered
// kernels exist as <EDGE = true> only.
PlanesRoute planes_route(GemmLayout layout, const PlanesGemmArgs& a, int ncu) {
  const GemmArgs& e = a.e;
  const bool nt = layout == kNT, one_slice = splits_of(e) == 1;
  PlanesRoute r = {};
  r.conv = !e.conv_cin ? 0 : nt ? 1 : 2;     // 1: A gathered as a convolution input (NT), 2: B gathered, weight gradient (TN)
  r.nwork = grid_of(a);                      // 128 x 128 tiles x K slices
  r.edge = is_edge(a) || r.conv;
  if (nt && e.N <= 64 && one_slice && !e.scat_on) {
    // 64-channel outputs: 256-row x 64-column tiles (half of a 128-wide tile would be padding)
    r.family = PlanesFamily::T64;
    r.nwork = ((e.M + 255) / 256) * ((e.N + 63) / 64);
    r.edge = (e.M % 256) != 0 || (e.N % 64) != 0 || r.conv;
  } else if (nt && one_slice && e.K % 64 == 0 && e.K >= 1024 && (e.conv_cin == 0 || e.conv_cin % 64 == 0)) {
    // pair-staged k-tiles: every K slice a whole number of 64-k pairs, a gathered pair inside one filter tap -- and a long
    // contraction: measured same-box (tools/bench_conv_gemm.py, bench.py) K = 1024 / 2048 take 4-6 % less time (the lifter's
    // forward GEMM 33.2 -> 32.7 us in the step), K <= 512 0-3 % MORE (a pair is a coarser unit at an item boundary)
    r.family = PlanesFamily::Wide;
  } else if (nt && r.nwork >= 2 * ncu) {
    // persistent form (round 3): NT problems with at least two work items per CU -- the conv path's 1x1 / 3x3 / transposed
    // convolutions over 16K .. 1M pixels
    r.family = PlanesFamily::Persistent;
  } else {
    r.family = PlanesFamily::OneItem;
  }
  // the NT families walk their items with one workgroup per CU from two items per CU on
  r.persist = r.family != PlanesFamily::OneItem && r.nwork >= 2 * ncu;
  r.grid = r.persist ? ncu : r.nwork;
  return r;
}

int launch_gemm_planes(GemmLayout layout, const PlanesGemmArgs& a, hipStream_t s) {
  if (!planes_gemm_ok(layout, a)) PL_FAIL(PL_ESHAPE, "gemm_planes: unsupported problem %dx%dx%d (layout %d, mode %d)", a.e.M, a.e.N, a.e.K, (int)layout, a.mode);
  const PlanesKern k = kern_of(a);
  const PlanesRoute r = planes_route(layout, a, cu_count());
  void* prof = prof_begin_flops(2.0 * a.e.M * a.e.N * a.e.K, s);
  PL_TRY(a.mode == plp::kF16x3 ? launch_routed<plp::kF16x3>(layout, r, k, s) : launch_routed<plp::kBf16>(layout, r, k, s));
  prof_end(prof, s);
  PL_CHECK_LAUNCH("gemm_planes");
  return PL_OK;
}

bool planes_pair_carries_slab_sum(const PlanesGemmArgs& nn, const PlanesGemmArgs& tn, int slabs, int64_t n) {
  return pair_carries_slab_sum(nn, tn, slabs, n);
}

int launch_gemm_planes_pair(const PlanesGemmArgs& nn, const PlanesGemmArgs& tn, const SlabSum* sum, hipStream_t s) {
  if (!planes_gemm_ok(kNN, nn) || !planes_gemm_ok(kTN, tn) || nn.mode != tn.mode || is_edge(nn) || is_edge(tn))
    PL_FAIL(PL_ESHAPE, "gemm_planes_pair: unsupported problems");
  const PlanesKern k0 = kern_of(nn), k1 = kern_of(tn);
  const PairRoute r = pair_route(nn, tn);
  plp::SlabRide ride = {};
  if (sum) {
    // the caller asked planes_pair_carries_slab_sum first: a sum this launch cannot carry is an error, not a silent drop
    if (!sum->part || !sum->out || !pair_carries_slab_sum(nn, tn, sum->slabs, sum->n))
      PL_FAIL(PL_ESHAPE, "gemm_planes_pair: cannot carry a sum of %d slabs of %lld floats", sum->slabs, (long long)sum->n);
    if ((reinterpret_cast<uintptr_t>(sum->part) | reinterpret_cast<uintptr_t>(sum->out)) & 15)
      PL_FAIL(PL_EINVAL, "gemm_planes_pair: slab sum alignment");
    ride.part = sum->part; ride.out = sum->out; ride.stride = sum->n; ride.R = sum->slabs; ride.n4 = (int)(sum->n / 4);
  }
  void* prof = prof_begin_flops(2.0 * nn.e.M * nn.e.N * nn.e.K + 2.0 * tn.e.M * tn.e.N * tn.e.K, s);
  if (nn.mode == plp::kF16x3) launch_pair<plp::kF16x3>(r, k0, k1, ride, grid_of(nn), grid_of(tn), s);
  else launch_pair<plp::kBf16>(r, k0, k1, ride, grid_of(nn), grid_of(tn), s);
  prof_end(prof, s);
  PL_CHECK_LAUNCH(r == PairRoute::Dual ? "gemm_planes_dual" : "gemm_planes_chain");
  return PL_OK;
}

}  // namespace pl

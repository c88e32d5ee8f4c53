// BatchNorm of the lifter path and of the conv path: statistics, apply (+ ReLU, dropout, residual add), backward, the
// eval-mode fold, and the Bottleneck's residual join.
//
// They replace, on the reference path, native_batch_norm(+backward), relu_, dropout, add
// (phase1_lifting/baselineModel.py:35-37,41-45,92-94) and, as stand-alone entry points, BatchNorm2d and the residual join of
// the conv path (Resnet.py:81-91).
//
// Common shape: a (B x H) fp32 activation is walked with one float4 per lane, a
// wavefront covering 256 consecutive columns of one row (1 KiB per wave-instruction,
// fully coalesced).  Every column reduction is a fixed-order two-stage sum (per-block
// partials, then a small finalize kernel): results are bitwise reproducible, no float
// atomics anywhere.
#include <algorithm>

#include "bn_pieces.h"
#include "pl_internal.h"
#include "plane_store.h"
#include "streaming.h"

namespace pl {
namespace {

// Pieces of the statistics finalize.  Floating-point contraction is OFF inside them: "SyncBN == one process on the
// concatenated batch, bit for bit" is a tested property, and it must not depend on what the compiler contracts.
__device__ __forceinline__ float bn_m2_term(float gsum, float gm2, float fn, float mean) {
#pragma clang fp contract(off)
  const float d = gsum / fn - mean;
  return gm2 + fn * d * d;
}
// (bn_shift_of, bn_running_update: bn_pieces.h)

// BatchNorm statistics finalize: Chan merge of (sum, M2) over 64-row groups.
// stat = [world][2][G][H] (rank-major: G rows of sums, then G rows of M2); Br rows per rank.  Walking
// the world*G partials in rank-major order is walking the concatenated batch's groups in row order,
// so the result is the one a single process gets on the concatenated batch (when Br % 128 == 0 even
// bit for bit: same partials, same order).
__global__ __launch_bounds__(NTHR) void bn_finalize_kernel(
    const float* __restrict__ stat, int G, int world, int Br, int H, int gs,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
    float* running_mean, float* running_var, int64_t* batches, float* mean_out, float* rstd_out,
    float* scale_out, float* shift_out) {
  __shared__ float red[RPARTS][RCOLS];
  const int cl = threadIdx.x & (RCOLS - 1), part = threadIdx.x / RCOLS;
  const int c = blockIdx.x * RCOLS + cl;
  const bool ok = c < H;
  const int GT = G * world;
  const float Bt = (float)Br * (float)world;
  const size_t GH = (size_t)G * H;
  // This kernel is pure latency (16,384 threads): everything it will need is requested up front -- the partials of
  // both passes (the lifter has 4 per thread: held in registers) and the per-column parameters -- so that it pays
  // ONE memory round trip instead of four dependent ones (6.6 -> ~3.5 us per launch, five launches per step).
  constexpr int KEEP = 4;
  float ks[KEEP], km[KEEP];
  const bool keep = GT <= KEEP * RPARTS;
#pragma unroll
  for (int q = 0; q < KEEP; ++q) {
    const int g = part + q * RPARTS;
    ks[q] = km[q] = 0.f;
    if (ok && keep && g < GT) {
      const int r = g / G, gl = g - r * G;
      const size_t at = (size_t)r * 2 * GH + (size_t)gl * H + c;
      ks[q] = stat[at]; km[q] = stat[at + GH];
    }
  }
  float ga = 0.f, be = 0.f, rm0 = 0.f, rv0 = 0.f;
  if (part == 0 && ok) {
    ga = gamma[c]; be = beta[c];
    if (running_mean) { rm0 = running_mean[c]; rv0 = running_var[c]; }
  }
  float s = 0.f;
  if (ok) {
    if (keep) {
#pragma unroll
      for (int q = 0; q < KEEP; ++q) s += ks[q];         // (absent groups hold 0)
    } else {
      // (many groups -- the conv path's maps: up to 2048): eight loads in flight per trip, at clamped addresses so that no
      // branch sits between them; added in group order.  One load per trip made this kernel 29 us on those maps.
      for (int g0 = part; g0 < GT; g0 += 8 * RPARTS) {
        float sv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int g = g0 + u * RPARTS, gg = min(g, GT - 1);
          const int r = gg / G, gl = gg - r * G;
          const float v = stat[(size_t)r * 2 * GH + (size_t)gl * H + c];
          sv[u] = g < GT ? v : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);     // (all eight requested before the first is waited for)
#pragma unroll
        for (int u = 0; u < 8; ++u) s += sv[u];
      }
    }
  }
  const float mean = parts_sum(s, red, cl, part) / Bt;
  float m2 = 0.f;
  if (ok) {
    if (keep) {
#pragma unroll
      for (int q = 0; q < KEEP; ++q) {
        const int g = part + q * RPARTS;
        if (g < GT) {
          const int gl = g % G;
          const int n = max(0, min(gs, Br - gl * gs));
          if (n > 0) m2 += bn_m2_term(ks[q], km[q], (float)n, mean);
        }
      }
    } else {
      for (int g0 = part; g0 < GT; g0 += 8 * RPARTS) {
        float sv[8], qv[8];
        int nv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int g = g0 + u * RPARTS, gg = min(g, GT - 1);
          const int r = gg / G, gl = gg - r * G;
          const size_t at = (size_t)r * 2 * GH + (size_t)gl * H + c;
          sv[u] = stat[at]; qv[u] = stat[at + GH];
          nv[u] = g < GT ? max(0, min(gs, Br - gl * gs)) : 0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (nv[u] > 0) m2 += bn_m2_term(sv[u], qv[u], (float)nv[u], mean);
      }
    }
  }
  const float m2t = parts_sum(m2, red, cl, part);
  if (part == 0 && ok) {
    const float var = m2t / Bt;  // biased
    const float rstd = 1.0f / sqrtf(var + eps);
    const float sc = ga * rstd;
    mean_out[c] = mean;
    rstd_out[c] = rstd;
    scale_out[c] = sc;
    shift_out[c] = bn_shift_of(be, mean, sc);
    if (running_mean) {
      bn_running_update(rm0, rv0, mean, var, Bt, momentum);
      running_mean[c] = rm0; running_var[c] = rv0;
    }
  }
  if (batches && blockIdx.x == 0 && threadIdx.x == 0) batches[0] += 1;
}

// block-level combine of per-wave float4 column partials; wave 0 returns the total
__device__ __forceinline__ float4 combine4(float4 v, float4 (*sm)[64], int wave, int lane) {
  sm[wave][lane] = v;
  __syncthreads();
  float4 t = sm[0][lane];
  if (wave == 0) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float4 u = sm[w][lane];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
  }
  __syncthreads();
  return t;
}

// Column statistics of a [B][H] matrix in the layout bn_finalize merges: per 64-row group the column sums
// and the sums of squares about the group mean (what the GEMM epilogue emits for the lifter; the conv path's
// BatchNorm2d over [B*H*W][C] computes them here).  grid = (ceil(H/256), ceil(B/64)).
// Narrow maps (C = 64, 128): the caller views [rows][C] as [rows/R][R*C] so that every lane of a 256-column strip
// works; virtual column vc is replica vc / Hc of real column vc % Hc, and the partials are written replica-major
// ([R][2][G][Hc]) -- exactly the [world][2][G][H] layout bn_finalize merges, with the replicas in the role of ranks.
// One pass over z: a workgroup's gs rows are taken 64 at a time, each wave holding its 16 rows of the sub-group in
// registers (16 loads in flight per lane) for the sum AND the squares about the sub-group mean; the sub-groups are
// merged pairwise in order (Chan et al.) into the one partial per gs rows.  (The first version re-read the group
// from memory for the second moment: 2x the traffic on maps far larger than the L2.)
__global__ __launch_bounds__(NTHR) void bn_colstats_kernel(const float* __restrict__ z, int B, int H, int gs, int Hc,
                                                           float* __restrict__ stat) {
  __shared__ float4 sm[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const bool active = c < H;
  const int r0 = blockIdx.y * gs, r1 = min(B, r0 + gs);
  float4 tsum = make_float4(0, 0, 0, 0), tm2 = tsum;       // merged so far (wave 0)
  float ndone = 0.f;
  for (int q0 = r0; q0 < r1; q0 += 64) {
    const int q1 = min(r1, q0 + 64);
    float4 v[16];
    float4 s = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = q0 + wave + 4 * i;
      v[i] = (active && r < q1) ? ld4(z + (size_t)r * H + c) : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) { s.x += v[i].x; s.y += v[i].y; s.z += v[i].z; s.w += v[i].w; }
    float4 t = combine4(s, sm, wave, lane);
    if (wave == 0) sm[0][lane] = t;
    __syncthreads();
    t = sm[0][lane];
    __syncthreads();
    const float nb = (float)(q1 - q0), inv = 1.0f / nb;
    const float4 mu = make_float4(t.x * inv, t.y * inv, t.z * inv, t.w * inv);
    float4 m2 = make_float4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (q0 + wave + 4 * i < q1) {
        const float dx = v[i].x - mu.x, dy = v[i].y - mu.y, dz = v[i].z - mu.z, dw = v[i].w - mu.w;
        m2.x = fmaf(dx, dx, m2.x); m2.y = fmaf(dy, dy, m2.y); m2.z = fmaf(dz, dz, m2.z); m2.w = fmaf(dw, dw, m2.w);
      }
    const float4 q = combine4(m2, sm, wave, lane);
    if (ndone == 0.f) { tsum = t; tm2 = q; }
    else {
      const float w = ndone * nb / (ndone + nb), ia = 1.0f / ndone;
      const float dx = mu.x - tsum.x * ia, dy = mu.y - tsum.y * ia, dz = mu.z - tsum.z * ia, dw = mu.w - tsum.w * ia;
      tm2.x += q.x + dx * dx * w; tm2.y += q.y + dy * dy * w; tm2.z += q.z + dz * dz * w; tm2.w += q.w + dw * dw * w;
      tsum.x += t.x; tsum.y += t.y; tsum.z += t.z; tsum.w += t.w;
    }
    ndone += nb;
  }
  if (wave == 0 && active) {
    const int rep = c / Hc, cc = c - rep * Hc;
    const size_t GH = (size_t)gridDim.y * Hc;
    float* base = stat + (size_t)rep * 2 * GH + (size_t)blockIdx.y * Hc + cc;
    st4(base, tsum);
    st4(base + GH, tm2);
  }
}

// out = relu(a + b), bitmap of relu_on(out) (positive or NaN): the residual join of a Bottleneck (Resnet.py:90-91) in training mode
__global__ __launch_bounds__(NTHR) void add_relu_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ out, uint64_t* __restrict__ bits, int B,
                                                        int H, PlaneOut po) {
  const PlaneDst pd = plane_dst(po);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x;
  const int c = strip * 256 + lane * 4;
  const bool active = c < H;
  const int wpr = ((H + 255) >> 8) * 4;
  for (int r = blockIdx.y * 4 + wave; r < B; r += gridDim.y * 4) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
      const float4 u = ld4(a + (size_t)r * H + c), v = ld4(b + (size_t)r * H + c);
      o[0] = u.x + v.x; o[1] = u.y + v.y; o[2] = u.z + v.z; o[3] = u.w + v.w;
    }
    uint64_t word = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool on = active && relu_on(o[j]);
      o[j] = on ? o[j] : 0.f;
      const uint64_t m = __ballot(on);
      if (lane == j) word = m;
    }
    if (lane < 4) bits[(size_t)r * wpr + strip * 4 + lane] = word;
    if (active) {
      const float4 v = make_float4(o[0], o[1], o[2], o[3]);
      st4(out + (size_t)r * H + c, v);
      if (pd.kind) store_planes4(pd, (size_t)r * H + c, v);
    }
  }
}

// dx = g where the bitmap says the forward output was positive, else 0 (backward of add_relu: both inputs get it)
__global__ __launch_bounds__(NTHR) void mask_by_bits_kernel(const float* __restrict__ g, const uint64_t* __restrict__ bits,
                                                            float* __restrict__ dx, int B, int H, const float* __restrict__ g2) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x;
  const int c = strip * 256 + lane * 4;
  if (c >= H) return;
  const int wpr = ((H + 255) >> 8) * 4;
  for (int r = blockIdx.y * 4 + wave; r < B; r += gridDim.y * 4) {
    float4 v = ld4(g + (size_t)r * H + c);
    if (g2) { const float4 u = ld4(g2 + (size_t)r * H + c); v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w; }
    const uint64_t* bw = bits + (size_t)r * wpr + strip * 4;
    float4 d;
    d.x = ((bw[0] >> lane) & 1ull) ? v.x : 0.f;
    d.y = ((bw[1] >> lane) & 1ull) ? v.y : 0.f;
    d.z = ((bw[2] >> lane) & 1ull) ? v.z : 0.f;
    d.w = ((bw[3] >> lane) & 1ull) ? v.w : 0.f;
    st4(dx + (size_t)r * H + c, d);
  }
}

// -------------------------------------------------------------------------------------
// act = [resid +] dropout(relu(z*scale + shift)); bitmap of (positive & kept).
// grid = (ceil(H/256), gy), block = 256: wave w walks rows blockIdx.y*4+w, +4*gy, ...
// Bitmap layout: row r, 256-column strip q, word j (0..3): bit l <-> column 256q + 4l + j.
// -------------------------------------------------------------------------------------
// the row loop of bn_apply_kernel (sc, sh: the lane's four columns).
// (Round 2 tried folding the statistics finalize into this kernel -- every workgroup re-deriving mean / rstd of its
//  256-column strip from the 64 partials -- to drop the 6.6 us finalize launch per layer; likewise for the backward
//  pass.  Same-box A/B, B = 4096: 0.7095 ms per step unfused against 0.80 (64 rows per workgroup), 0.80 (32), 0.92
//  (128), 0.90 (16): the 128 KB prologue per workgroup costs more than the launch it removes.  Not kept.
//  Also tried: two rows per trip with both rows' loads issued first (here and in bn_bwd_dz_rows): 0.6543 / 0.6524 ms
//  against 0.6446 / 0.6446 for one row per trip, same box -- eight short waves per CU already overlap their round trips.
//  Tried again on the conv path's maps (up to 1 GB, far beyond the caches; bn_apply, bn_bwd_dz and bn_bwd_reduce with two rows'
//  operands AND bitmap words requested up front): Model_3D step at B = 256 92.9 / 92.8 ms against 91.9 / 91.6 ms for one row per
//  trip, interleaved on one box -- these passes are not short of requests in flight.)
// RESID (is there a residual / join operand) is a template parameter for the same reason as bn_bwd_dz_rows' BN: its load leaves
// with z's instead of after the wait for it.
// one row of bn_apply: the lane's four columns c .. c+3 of row r (v = z, rv = the residual / join operand)
template <bool RESID>
__device__ __forceinline__ void bn_apply_row(
    const int r, const int c, const bool active, const float4 v, const float4 rv, const float4 sc, const float4 sh, float* act,
    uint64_t* __restrict__ bits, int H, int mode, bool norelu, uint32_t thr, float kscale, uint32_t k0,
    uint32_t k1, uint32_t c3, uint32_t layer, const uint64_t* __restrict__ inject, const PlaneDst& pd, bool resid_first) {
  const int lane = threadIdx.x & 63;
  const int strip = c >> 8;
  const int wpr = ((H + 255) >> 8) * 4;
  const size_t off = (size_t)r * H + c;
  float y[4] = {0.f, 0.f, 0.f, 0.f};
  bool keep[4] = {true, true, true, true};
  if (active) {
    y[0] = fmaf(v.x, sc.x, sh.x); y[1] = fmaf(v.y, sc.y, sh.y);
    y[2] = fmaf(v.z, sc.z, sh.z); y[3] = fmaf(v.w, sc.w, sh.w);
    if (RESID && resid_first) { y[0] += rv.x; y[1] += rv.y; y[2] += rv.z; y[3] += rv.w; }
    if (mode == 1) {
      const uint64_t g = ((uint64_t)r * (uint64_t)H + (uint64_t)c) >> 2;
      const Philox4 u = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), layer, c3, k0, k1);
#pragma unroll
      for (int j = 0; j < 4; ++j) keep[j] = u.v[j] >= thr;
    } else if (mode == 2) {
#pragma unroll
      for (int j = 0; j < 4; ++j) keep[j] = (inject[(size_t)r * wpr + strip * 4 + j] >> lane) & 1ull;
    } else if (mode == 3) {
#pragma unroll
      for (int j = 0; j < 4; ++j) keep[j] = false;
    }
  }
  bool on[4];
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    on[j] = active && keep[j] && (norelu || relu_on(y[j]));
    o[j] = on[j] ? y[j] * kscale : 0.f;
  }
  uint64_t word = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint64_t b = __ballot(on[j]);
    if (lane == j) word = b;
  }
  if (lane < 4) bits[(size_t)r * wpr + strip * 4 + lane] = word;
  if (active) {
    float4 out = make_float4(o[0], o[1], o[2], o[3]);
    if (RESID && !resid_first) { out.x += rv.x; out.y += rv.y; out.z += rv.z; out.w += rv.w; }
    if (act) st4_nt(act + off, out, pd.nt);
    if (pd.kind) store_planes4(pd, off, out);
  }
}

template <bool RESID>
__device__ __forceinline__ void bn_apply_rows(
    const float* __restrict__ z, const float4 sc, const float4 sh, const float* resid, float* act,
    uint64_t* __restrict__ bits, int B, int H, int mode, bool norelu, uint32_t thr, float kscale, uint32_t k0,
    uint32_t k1, uint32_t c3, uint32_t layer, const uint64_t* __restrict__ inject, const PlaneDst& pd,
    bool resid_first = false) {
  // resid_first: resid joins BEFORE the ReLU -- relu(bn(z) + resid), the Bottleneck's join (Resnet.py:90-91) -- instead of
  // after it (the lifter's block: x + relu(bn(z)))
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const bool active = c < H;
  for (int r = blockIdx.y * 4 + wave; r < B; r += gridDim.y * 4) {
    const size_t off = (size_t)r * H + c;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f), rv = v;
    if (active) {
      v = ld4(z + off);
      if constexpr (RESID) rv = ld4(resid + off);
    }
    bn_apply_row<RESID>(r, c, active, v, rv, sc, sh, act, bits, H, mode, norelu, thr, kscale, k0, k1, c3, layer, inject, pd,
                        resid_first);
  }
}

// The statistics finalize inside the apply launch (BnFin::stat != NULL; local statistics, at most 16 groups -- BnApplyArgs::fin
// in pl_internal.h says what is routed here): every workgroup re-derives mean / rstd / scale / shift of its four columns per
// lane from the partials -- with <= 16 groups bn_finalize_kernel's part p holds group p alone, so its result is the sum over
// the groups in order, which is what is done here, bit for bit -- and the workgroups with blockIdx.y == 0 write mean, rstd and
// the running statistics.  At B = 4096 (64 groups, 128 KB of partials per workgroup) this cost more than the launch it
// removes (round 2); at 128 ... 256 rows the prologue is 2 ... 4 float4 pairs per lane and the 4.9 us finalize launch is a
// twentieth of the step.
// (the kernel's own copy of BnFinalizeArgs: only what it reads, so that the kernel's argument block stays as small as it was)
struct BnFin {
  const float* stat;            // [2][G][H]
  const float *gamma, *beta;
  float *running_mean, *running_var, *mean_out, *rstd_out;
  int64_t* batches;
  float eps, momentum;
  int G, Br, gs;
};

__global__ __launch_bounds__(NTHR) void bn_apply_kernel(
    const float* __restrict__ z, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* resid, float* act, uint64_t* __restrict__ bits, int B, int H, int mode,
    uint32_t thr, float kscale, uint32_t k0, uint32_t k1, uint32_t c3, uint32_t layer,
    const uint64_t* __restrict__ inject, int Hc, PlaneOut po, const uint64_t* __restrict__ step_dev,
    uint32_t seed_hi, BnFin fin) {
  const PlaneDst pd = plane_dst(po);
  dropout_replay_step(c3, k1, seed_hi, step_dev);
  // Hc: real columns behind the H virtual ones (bn_colstats_kernel); Hc == H for the lifter
  // mode: 0 keep all, 1 philox, 2 injected bitmap, 3 drop all; + 8: no ReLU (BatchNorm alone; bitmap all ones)
  const bool norelu = (mode & 8) != 0, resid_first = (mode & 32) != 0;      // + 32: the residual joins before the ReLU
  mode &= 7;
  const int c = blockIdx.x * 256 + (threadIdx.x & 63) * 4;
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
  if (fin.stat) {                                           // (kernel-uniform; Hc == H on this route)
    if (c < H) {
      const size_t GH = (size_t)fin.G * H;
      float4 ks[16], km[16];
#pragma unroll
      for (int g = 0; g < 16; ++g)
        if (g < fin.G) { ks[g] = ld4(fin.stat + (size_t)g * H + c); km[g] = ld4(fin.stat + GH + (size_t)g * H + c); }
      const float4 ga = ld4(fin.gamma + c), be = ld4(fin.beta + c);
      const float Bt = (float)fin.Br;
      float s4[4] = {0.f, 0.f, 0.f, 0.f}, m4[4] = {0.f, 0.f, 0.f, 0.f}, mean4[4];
#pragma unroll
      for (int g = 0; g < 16; ++g)
        if (g < fin.G) { s4[0] += ks[g].x; s4[1] += ks[g].y; s4[2] += ks[g].z; s4[3] += ks[g].w; }
#pragma unroll
      for (int j = 0; j < 4; ++j) mean4[j] = s4[j] / Bt;
#pragma unroll
      for (int g = 0; g < 16; ++g)
        if (g < fin.G) {
          const int n = max(0, min(fin.gs, fin.Br - g * fin.gs));
          if (n > 0) {
            m4[0] += bn_m2_term(ks[g].x, km[g].x, (float)n, mean4[0]); m4[1] += bn_m2_term(ks[g].y, km[g].y, (float)n, mean4[1]);
            m4[2] += bn_m2_term(ks[g].z, km[g].z, (float)n, mean4[2]); m4[3] += bn_m2_term(ks[g].w, km[g].w, (float)n, mean4[3]);
          }
        }
      const float g4[4] = {ga.x, ga.y, ga.z, ga.w}, b4[4] = {be.x, be.y, be.z, be.w};
      float var4[4], rs4[4], sc4[4], sh4[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        var4[j] = m4[j] / Bt;
        rs4[j] = 1.0f / sqrtf(var4[j] + fin.eps);
        sc4[j] = g4[j] * rs4[j];
        sh4[j] = bn_shift_of(b4[j], mean4[j], sc4[j]);
      }
      sc = make_float4(sc4[0], sc4[1], sc4[2], sc4[3]);
      sh = make_float4(sh4[0], sh4[1], sh4[2], sh4[3]);
      if (blockIdx.y == 0 && threadIdx.x < 64) {
        st4(fin.mean_out + c, make_float4(mean4[0], mean4[1], mean4[2], mean4[3]));
        st4(fin.rstd_out + c, make_float4(rs4[0], rs4[1], rs4[2], rs4[3]));
        if (fin.running_mean) {
          float4 rm = ld4(fin.running_mean + c), rv = ld4(fin.running_var + c);
          bn_running_update(rm.x, rv.x, mean4[0], var4[0], Bt, fin.momentum);
          bn_running_update(rm.y, rv.y, mean4[1], var4[1], Bt, fin.momentum);
          bn_running_update(rm.z, rv.z, mean4[2], var4[2], Bt, fin.momentum);
          bn_running_update(rm.w, rv.w, mean4[3], var4[3], Bt, fin.momentum);
          st4(fin.running_mean + c, rm); st4(fin.running_var + c, rv);
        }
      }
    }
    if (fin.batches && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) fin.batches[0] += 1;
  } else if (c < H && scale) { sc = ld4(scale + c % Hc); sh = ld4(shift + c % Hc); }
  if (resid) bn_apply_rows<true>(z, sc, sh, resid, act, bits, B, H, mode, norelu, thr, kscale, k0, k1, c3, layer, inject, pd, resid_first);
  else bn_apply_rows<false>(z, sc, sh, resid, act, bits, B, H, mode, norelu, thr, kscale, k0, k1, c3, layer, inject, pd, resid_first);
}

// -------------------------------------------------------------------------------------
// Small batches (B <= kBnSmallRows: the reference's own batch of 64, train_1.py:194): the three launches of a hidden layer's
// forward tail -- statistics finalize, apply -- and of its backward head -- pass 1, finalize, dz -- are launch latency and
// nothing else at this size (5 us each for 256 KB of data).  Here ONE workgroup owns a 256-column strip for ALL rows:
// statistics straight from z (no partials, no Chan merge: two passes over rows that sit in L2), then the apply loop itself.
// -------------------------------------------------------------------------------------
// every wave gets the strip total of a per-wave float4 partial (fixed order); NW waves
template <int NW>
__device__ __forceinline__ float4 allwaves4(float4 v, float4 (*sm)[64], int wave, int lane) {
  sm[wave][lane] = v;
  __syncthreads();
  float4 t = sm[0][lane];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const float4 u = sm[w][lane];
    t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
  }
  __syncthreads();
  return t;
}

// 512 threads: wave w holds rows w, w + 8, ... (RU of them: 8 for B <= 64, 16 for B <= 128) of the strip IN REGISTERS -- one
// memory round trip for the whole kernel: statistics, the apply and the bitmap all work on the registers.
// (First version: 256 threads streaming the rows twice for the statistics and a third time for the apply, four rows in
//  flight: 0.313 ms per step at B = 64 against 0.304 for the three separate launches -- a dozen dependent round trips in
//  four workgroups cost more than two launch boundaries.)
constexpr int kSmallThreads = 512;
template <int RU, bool RESID>
__global__ __launch_bounds__(kSmallThreads) void bn_small_fwd_kernel(
    const float* __restrict__ z, const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
    float* running_mean, float* running_var, int64_t* batches, float* __restrict__ mean_out, float* __restrict__ rstd_out,
    const float* resid, float* act, uint64_t* __restrict__ bits, int B, int H, int mode, uint32_t thr, float kscale,
    uint32_t k0, uint32_t k1, uint32_t c3, uint32_t layer, const uint64_t* __restrict__ inject,
    const uint64_t* __restrict__ step_dev, uint32_t seed_hi) {
  __shared__ float4 sm[8][64];
  dropout_replay_step(c3, k1, seed_hi, step_dev);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const bool active = c < H;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 zv[RU], rv[RESID ? RU : 1];
  float4 ga = zero, be = zero, rm = zero, rvar = zero;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int r = wave + 8 * u;
    const bool ok = active && r < B;
    zv[u] = ok ? ld4(z + (size_t)r * H + c) : zero;
    if constexpr (RESID) rv[u] = ok ? ld4(resid + (size_t)r * H + c) : zero;
  }
  if (active) {
    ga = ld4(gamma + c); be = ld4(beta + c);
    if (running_mean && wave == 0) { rm = ld4(running_mean + c); rvar = ld4(running_var + c); }
  }
  float4 s = zero;
#pragma unroll
  for (int u = 0; u < RU; ++u) { s.x += zv[u].x; s.y += zv[u].y; s.z += zv[u].z; s.w += zv[u].w; }
  s = allwaves4<8>(s, sm, wave, lane);
  const float Bt = (float)B;
  const float4 mean = make_float4(s.x / Bt, s.y / Bt, s.z / Bt, s.w / Bt);
  float4 q = zero;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    if (wave + 8 * u >= B) continue;
    const float dx = zv[u].x - mean.x, dy = zv[u].y - mean.y, dz = zv[u].z - mean.z, dw = zv[u].w - mean.w;
    q.x = fmaf(dx, dx, q.x); q.y = fmaf(dy, dy, q.y); q.z = fmaf(dz, dz, q.z); q.w = fmaf(dw, dw, q.w);
  }
  q = allwaves4<8>(q, sm, wave, lane);
  float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = zero;
  if (active) {
    const float var[4] = {q.x / Bt, q.y / Bt, q.z / Bt, q.w / Bt};
    const float mu[4] = {mean.x, mean.y, mean.z, mean.w};
    const float g4[4] = {ga.x, ga.y, ga.z, ga.w}, b4[4] = {be.x, be.y, be.z, be.w};
    float rs[4], scv[4], shv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      rs[j] = 1.0f / sqrtf(var[j] + eps);
      scv[j] = g4[j] * rs[j];
      shv[j] = bn_shift_of(b4[j], mu[j], scv[j]);
    }
    sc = make_float4(scv[0], scv[1], scv[2], scv[3]);
    sh = make_float4(shv[0], shv[1], shv[2], shv[3]);
    if (wave == 0) {
      st4(mean_out + c, mean);
      st4(rstd_out + c, make_float4(rs[0], rs[1], rs[2], rs[3]));
      if (running_mean) {
        bn_running_update(rm.x, rvar.x, mu[0], var[0], Bt, momentum);
        bn_running_update(rm.y, rvar.y, mu[1], var[1], Bt, momentum);
        bn_running_update(rm.z, rvar.z, mu[2], var[2], Bt, momentum);
        bn_running_update(rm.w, rvar.w, mu[3], var[3], Bt, momentum);
        st4(running_mean + c, rm); st4(running_var + c, rvar);
      }
    }
  }
  if (batches && blockIdx.x == 0 && threadIdx.x == 0) batches[0] += 1;
  const bool norelu = (mode & 8) != 0;
  const PlaneDst pd = {nullptr, nullptr, 1.f, 0, 0};
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int r = wave + 8 * u;
    if (r >= B) break;                                 // (wave-uniform)
    bn_apply_row<RESID>(r, c, active, zv[u], RESID ? rv[u] : zero, sc, sh, act, bits, H, mode & 7, norelu, thr, kscale, k0, k1,
                        c3, layer, inject, pd, false);
  }
}

// backward head of one hidden layer for a small batch: pass 1 (sum dy, sum dy zhat), the coefficients, dz = c0 (dy - c1 -
// zhat c2), the bias gradient and dgamma / dbeta -- one workgroup per strip, the rows (masked dy and zhat) in registers
// TILE: the bitmap is in the tile format of small_layer.hip (the layer's forward ran there)
template <int RU, bool TILE>
__global__ __launch_bounds__(kSmallThreads) void bn_small_bwd_kernel(
    const float* __restrict__ g, const uint64_t* __restrict__ bits, const float* __restrict__ z,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ gamma, float kscale, int B, int H,
    float* __restrict__ dz, float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ dbias) {
  __shared__ float4 sm[8][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x;
  const int c = strip * 256 + lane * 4;
  const bool active = c < H;
  const int wpr = ((H + 255) >> 8) * 4;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 mu = zero, rs = zero, ga = zero;
  float4 dv[RU], zh[RU];                                // masked, scaled dy and zhat of the wave's rows
  {
    float4 gv[RU], zv[RU];
    ulonglong2 b01[RU], b23[RU];
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const int r = min(wave + 8 * u, B - 1);
      gv[u] = active ? ld4(g + (size_t)r * H + c) : zero;
      zv[u] = active ? ld4(z + (size_t)r * H + c) : zero;
      const uint64_t* bw = TILE ? bits + (size_t)(c >> 4) * 16 + (r >> 4) * 4 : bits + (size_t)r * wpr + strip * 4;
      b01[u] = *reinterpret_cast<const ulonglong2*>(bw);
      b23[u] = *reinterpret_cast<const ulonglong2*>(bw + 2);
    }
    if (active) { mu = ld4(mean + c); rs = ld4(rstd + c); ga = ld4(gamma + c); }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < RU; ++u) {
      const bool ok = wave + 8 * u < B;
      const int bit = TILE ? ((min(wave + 8 * u, B - 1) & 15) * 4 + (lane & 3)) : lane;
      dv[u].x = (ok && ((b01[u].x >> bit) & 1ull)) ? gv[u].x * kscale : 0.f;
      dv[u].y = (ok && ((b01[u].y >> bit) & 1ull)) ? gv[u].y * kscale : 0.f;
      dv[u].z = (ok && ((b23[u].x >> bit) & 1ull)) ? gv[u].z * kscale : 0.f;
      dv[u].w = (ok && ((b23[u].y >> bit) & 1ull)) ? gv[u].w * kscale : 0.f;
      zh[u] = ok ? make_float4((zv[u].x - mu.x) * rs.x, (zv[u].y - mu.y) * rs.y, (zv[u].z - mu.z) * rs.z, (zv[u].w - mu.w) * rs.w) : zero;
    }
  }
  float4 s1 = zero, s2 = zero, sz = zero;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    s1.x += dv[u].x; s1.y += dv[u].y; s1.z += dv[u].z; s1.w += dv[u].w;
    s2.x = fmaf(dv[u].x, zh[u].x, s2.x); s2.y = fmaf(dv[u].y, zh[u].y, s2.y);
    s2.z = fmaf(dv[u].z, zh[u].z, s2.z); s2.w = fmaf(dv[u].w, zh[u].w, s2.w);
    sz.x += zh[u].x; sz.y += zh[u].y; sz.z += zh[u].z; sz.w += zh[u].w;
  }
  s1 = allwaves4<8>(s1, sm, wave, lane);
  s2 = allwaves4<8>(s2, sm, wave, lane);
  sz = allwaves4<8>(sz, sm, wave, lane);
  const float Bt = (float)B;
  const float4 c0 = make_float4(ga.x * rs.x, ga.y * rs.y, ga.z * rs.z, ga.w * rs.w);
  const float4 c1 = make_float4(s1.x / Bt, s1.y / Bt, s1.z / Bt, s1.w / Bt);
  const float4 c2 = make_float4(s2.x / Bt, s2.y / Bt, s2.z / Bt, s2.w / Bt);
  if (wave == 0 && active) {
    st4(dgamma + c, s2); st4(dbeta + c, s1);
    // bias gradient = sum_r dz_r = c0 (sum d - B c1 - c2 sum zhat): its true value is 0 (a bias in front of BatchNorm); formed
    // from the three sums it carries a few ulps of them, where the sum of B rounded dz values carries sqrt(B) ulps of |dz|
    float4 db;
    db.x = c0.x * ((s1.x - Bt * c1.x) - c2.x * sz.x); db.y = c0.y * ((s1.y - Bt * c1.y) - c2.y * sz.y);
    db.z = c0.z * ((s1.z - Bt * c1.z) - c2.z * sz.z); db.w = c0.w * ((s1.w - Bt * c1.w) - c2.w * sz.w);
    st4(dbias + c, db);
  }
  if (!active) return;
#pragma unroll
  for (int u = 0; u < RU; ++u) {
    const int r = wave + 8 * u;
    if (r >= B) break;
    float4 d;
    d.x = c0.x * (dv[u].x - c1.x - zh[u].x * c2.x); d.y = c0.y * (dv[u].y - c1.y - zh[u].y * c2.y);
    d.z = c0.z * (dv[u].z - c1.z - zh[u].z * c2.z); d.w = c0.w * (dv[u].w - c1.w - zh[u].w * c2.w);
    st4(dz + (size_t)r * H + c, d);
  }
}

// -------------------------------------------------------------------------------------
// BN backward pass 1: per-block partial column sums of dy and dy*zhat.
// -------------------------------------------------------------------------------------
// join_g2 / join_dx (the Bottleneck's bn3 + residual join, pl_bn_join_bwd): the incoming gradient is g + join_g2 (join_g2 may be
// NULL) and the masked value is also stored to join_dx -- the residual join's backward (mask_by_bits_kernel) folded into this pass.
__global__ __launch_bounds__(NTHR) void bn_bwd_reduce_kernel(
    const float* __restrict__ g, const uint64_t* __restrict__ bits, const float* __restrict__ z,
    const float* __restrict__ mean, const float* __restrict__ rstd, float kscale, int B, int H,
    float* __restrict__ part_dy, float* __restrict__ part_dyz, int Hc, float* __restrict__ part_amax,
    const float* __restrict__ join_g2, float* __restrict__ join_dx) {
  __shared__ float4 sm[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x;
  const int c = strip * 256 + lane * 4;
  const bool active = c < H;
  const int wpr = ((H + 255) >> 8) * 4;
  float4 mu = make_float4(0, 0, 0, 0), rs = mu, s1 = mu, s2 = mu;
  float mxd = 0.f, mxz = 0.f;                     // max |dy|, max |zhat| seen by this lane (part_amax)
  if (active) { mu = ld4(mean + c % Hc); rs = ld4(rstd + c % Hc); }
  for (int r = blockIdx.y * 4 + wave; r < B; r += gridDim.y * 4) {
    if (!active) continue;
    const size_t off = (size_t)r * H + c;
    float4 gv = ld4(g + off);
    const float4 zv = ld4(z + off);
    if (join_g2) { const float4 u = ld4(join_g2 + off); gv.x += u.x; gv.y += u.y; gv.z += u.z; gv.w += u.w; }
    const uint64_t* bw = bits + (size_t)r * wpr + strip * 4;
    const float d0 = ((bw[0] >> lane) & 1ull) ? gv.x * kscale : 0.f;
    const float d1 = ((bw[1] >> lane) & 1ull) ? gv.y * kscale : 0.f;
    const float d2 = ((bw[2] >> lane) & 1ull) ? gv.z * kscale : 0.f;
    const float d3 = ((bw[3] >> lane) & 1ull) ? gv.w * kscale : 0.f;
    if (join_dx) st4(join_dx + off, make_float4(d0, d1, d2, d3));
    s1.x += d0; s1.y += d1; s1.z += d2; s1.w += d3;
    const float z0 = (zv.x - mu.x) * rs.x, z1 = (zv.y - mu.y) * rs.y, z2 = (zv.z - mu.z) * rs.z, z3 = (zv.w - mu.w) * rs.w;
    s2.x = fmaf(d0, z0, s2.x);
    s2.y = fmaf(d1, z1, s2.y);
    s2.z = fmaf(d2, z2, s2.z);
    s2.w = fmaf(d3, z3, s2.w);
    if (part_amax) {
      mxd = fmaxf(fmaxf(mxd, fmaxf(fabsf(d0), fabsf(d1))), fmaxf(fabsf(d2), fabsf(d3)));
      mxz = fmaxf(fmaxf(mxz, fmaxf(fabsf(z0), fabsf(z1))), fmaxf(fabsf(z2), fabsf(z3)));
    }
  }
  const float4 t1 = combine4(s1, sm, wave, lane);
  const float4 t2 = combine4(s2, sm, wave, lane);
  if (part_amax) {                                 // wave-uniform; one pair per workgroup, no atomics
    sm[wave][lane] = make_float4(mxd, mxz, 0.f, 0.f);
    __syncthreads();
    if (wave == 0) {
      float a = 0.f, b = 0.f;
#pragma unroll
      for (int w = 0; w < 4; ++w) { a = fmaxf(a, sm[w][lane].x); b = fmaxf(b, sm[w][lane].y); }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) { a = fmaxf(a, __shfl_xor(a, o)); b = fmaxf(b, __shfl_xor(b, o)); }
      if (lane == 0) {
        float* q = part_amax + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 2;
        q[0] = a; q[1] = b;
      }
    }
    __syncthreads();
  }
  if (wave == 0 && active) {
    // replica-major when Hc < H: [R][2][RC][Hc] (part_dyz = part_dy + RC*Hc); plain [2][RC][H] otherwise
    const int rep = c / Hc, cc = c - rep * Hc;
    const size_t off = (size_t)rep * 2 * gridDim.y * Hc + (size_t)blockIdx.y * Hc + cc;
    st4(part_dy + off, t1);
    st4(part_dyz + off, t2);
  }
}

// part = [world][2][RC][H] (rank-major: RC rows of sum dy, then RC rows of sum dy*zhat).  The dz
// coefficients use every rank's partials (the statistics were global, so is their gradient); dgamma
// and dbeta are this rank's own sums -- the gradient all-reduce adds the other ranks'.
__global__ __launch_bounds__(NTHR) void bn_bwd_finalize_kernel(
    const float* __restrict__ part_all, int RC, int world, int rank, int Br, int H,
    const float* __restrict__ gamma, const float* __restrict__ rstd, float* __restrict__ coef,
    float* __restrict__ dgamma, float* __restrict__ dbeta, const float* __restrict__ part_amax, int n_amax,
    float* __restrict__ dz_scale, int eval_mode, long long rstride, int amax_world) {
  // rstride: floats between two ranks' slabs (0: the dense 2 RC H); amax_world > 1: every rank's slab carries its n_amax
  // {max|dy|, max|zhat|} pairs behind its partial sums (part_amax points at rank 0's) -- under SyncBN the batch means in dz
  // are global, so the range bound of dz needs the GLOBAL maxima
  __shared__ float red[RPARTS][RCOLS];
  if (dz_scale && blockIdx.x == gridDim.x - 1) {
    // the extra workgroup: range bound of dz = c0 (dy - c1 - zhat c2), |c1| <= max|dy|, |c2| <= max|dy| (mean |zhat| <= 1):
    //   |dz| <= max|c0| max|dy| (2 + max|zhat|)  ->  S = the power of two that maps the bound into (2^13, 2^14]
    float a = 0.f, b = 0.f, c0 = 0.f;
    // (this one workgroup is the kernel's critical path: its loads go out eight at a time, at clamped indices -- a maximum does
    //  not care about repeats -- instead of one dependent round trip per trip)
    for (int r = 0; r < max(amax_world, 1); ++r) {
      const float2* pa = reinterpret_cast<const float2*>(part_amax + (size_t)r * rstride);
      for (int k0 = threadIdx.x; k0 < n_amax; k0 += 8 * NTHR) {
        float2 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = pa[min(k0 + u * NTHR, n_amax - 1)];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u) { a = fmaxf(a, t[u].x); b = fmaxf(b, t[u].y); }
      }
    }
    for (int k0 = threadIdx.x; k0 < H; k0 += 4 * NTHR) {
      float gv[4], rv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { const int k = min(k0 + u * NTHR, H - 1); gv[u] = gamma[k]; rv[u] = rstd[k]; }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) c0 = fmaxf(c0, fabsf(gv[u] * rv[u]));
    }
    float* sm = &red[0][0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      a = fmaxf(a, __shfl_xor(a, o)); b = fmaxf(b, __shfl_xor(b, o)); c0 = fmaxf(c0, __shfl_xor(c0, o));
    }
    if (lane == 0) { sm[wave * 3] = a; sm[wave * 3 + 1] = b; sm[wave * 3 + 2] = c0; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < 4; ++w) { a = fmaxf(a, sm[w * 3]); b = fmaxf(b, sm[w * 3 + 1]); c0 = fmaxf(c0, sm[w * 3 + 2]); }
      const float bound = c0 * a * (2.0f + b);
      int e = 0;
      float S = 1.0f, Si = 1.0f;
      if (bound > 0.f && bound < 3.0e38f) {          // zero / inf / nan gradients: scale 1 (they stay what they are)
        (void)frexpf(bound, &e);                     // bound = m 2^e, 0.5 <= m < 1
        e = min(max(14 - e, -100), 100);
        S = ldexpf(1.0f, e); Si = ldexpf(1.0f, -e);
      }
      dz_scale[0] = S; dz_scale[1] = Si;
    }
    return;
  }
  const int cl = threadIdx.x & (RCOLS - 1), part = threadIdx.x / RCOLS;
  const int c = blockIdx.x * RCOLS + cl;
  const bool ok = c < H;
  const size_t RH = (size_t)RC * H;
  const size_t RS = rstride > 0 ? (size_t)rstride : 2 * RH;
  // rank < 0: the "ranks" are replicas of a narrow map (bn_colstats_kernel): every partial is this process's own
  const float* mine = part_all + (size_t)max(rank, 0) * RS;
  float gac = 0.f, rsc = 0.f;               // requested with the partials: one memory round trip, not two
  if (part == 0 && ok) { gac = gamma[c]; rsc = rstd[c]; }
  float a = 0.f, b = 0.f;
  if (ok && rank >= 0)                    // a replica view only needs the totals below
    for (int k0 = part; k0 < RC; k0 += 8 * RPARTS) {        // eight row-chunks' loads in flight (as bn_finalize_kernel)
      float av[8], bv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u * RPARTS, kk = min(k, RC - 1);
        const float x = mine[(size_t)kk * H + c], y = mine[RH + (size_t)kk * H + c];
        av[u] = k < RC ? x : 0.f; bv[u] = k < RC ? y : 0.f;
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int u = 0; u < 8; ++u) { a += av[u]; b += bv[u]; }
    }
  const float sdy = parts_sum(a, red, cl, part);
  const float sdyz = parts_sum(b, red, cl, part);
  float tdy = sdy, tdyz = sdyz;
  if (world > 1) {                        // fixed rank-major order: every rank computes the same totals
    a = 0.f; b = 0.f;
    if (ok)
      for (int k0 = part; k0 < RC * world; k0 += 8 * RPARTS) {
        float av[8], bv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + u * RPARTS, kk = min(k, RC * world - 1);
          const int r = kk / RC, kl = kk - r * RC;
          const float x = part_all[(size_t)r * RS + (size_t)kl * H + c], y = part_all[(size_t)r * RS + RH + (size_t)kl * H + c];
          av[u] = k < RC * world ? x : 0.f; bv[u] = k < RC * world ? y : 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 8; ++u) { a += av[u]; b += bv[u]; }
      }
    tdy = parts_sum(a, red, cl, part);
    tdyz = parts_sum(b, red, cl, part);
  }
  if (part == 0 && ok) {
    const float Bt = (float)Br * (float)world;
    coef[c] = gac * rsc;
    // eval mode (running statistics are constants of the graph): dz = gamma rstd dy, no batch-mean terms
    coef[H + c] = eval_mode ? 0.f : tdy / Bt;
    coef[2 * H + c] = eval_mode ? 0.f : tdyz / Bt;
    dgamma[c] = rank < 0 ? tdyz : sdyz;
    dbeta[c] = rank < 0 ? tdy : sdy;
  }
}

// -------------------------------------------------------------------------------------
// BN backward pass 2: dz = c0*(dy - c1 - zhat*c2) (or dz = dy without BN) + db partials.
// -------------------------------------------------------------------------------------
// the row loop of bn_bwd_dz_kernel
// BN is a template parameter so that the z load sits in the same basic block as the g load: behind a run-time `if (bn)` it was
// issued only after the wait for g -- two dependent round trips per row.
template <bool BN>
__device__ __forceinline__ void bn_bwd_dz_rows(
    const float* __restrict__ g, const uint64_t* __restrict__ bits, const float* __restrict__ z, const float4 mu,
    const float4 rs, const float4 c0, const float4 c1, const float4 c2, float kscale, int B, int H,
    float* __restrict__ dz, float* __restrict__ part_db, const PlaneDst& pd, float4 (*sm)[64]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int strip = blockIdx.x;
  const int c = strip * 256 + lane * 4;
  const bool active = c < H;
  const int wpr = ((H + 255) >> 8) * 4;
  float4 sdb = make_float4(0, 0, 0, 0);
  for (int r = blockIdx.y * 4 + wave; r < B; r += gridDim.y * 4) {
    if (!active) continue;
    const size_t off = (size_t)r * H + c;
    const float4 gv = ld4(g + off);
    float4 zv = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (BN) zv = ld4(z + off);
    const uint64_t* bw = bits + (size_t)r * wpr + strip * 4;
    float4 d;
    d.x = ((bw[0] >> lane) & 1ull) ? gv.x * kscale : 0.f;
    d.y = ((bw[1] >> lane) & 1ull) ? gv.y * kscale : 0.f;
    d.z = ((bw[2] >> lane) & 1ull) ? gv.z * kscale : 0.f;
    d.w = ((bw[3] >> lane) & 1ull) ? gv.w * kscale : 0.f;
    if constexpr (BN) {
      d.x = c0.x * (d.x - c1.x - (zv.x - mu.x) * rs.x * c2.x);
      d.y = c0.y * (d.y - c1.y - (zv.y - mu.y) * rs.y * c2.y);
      d.z = c0.z * (d.z - c1.z - (zv.z - mu.z) * rs.z * c2.z);
      d.w = c0.w * (d.w - c1.w - (zv.w - mu.w) * rs.w * c2.w);
    }
    if (dz) st4_nt(dz + off, d, pd.nt);
    if (pd.kind) store_planes4(pd, off, d);
    sdb.x += d.x; sdb.y += d.y; sdb.z += d.z; sdb.w += d.w;
  }
  const float4 t = combine4(sdb, sm, wave, lane);
  if (wave == 0 && active) st4(part_db + (size_t)blockIdx.y * H + c, t);
}

__global__ __launch_bounds__(NTHR) void bn_bwd_dz_kernel(
    const float* __restrict__ g, const uint64_t* __restrict__ bits, const float* __restrict__ z,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ coef,
    float kscale, int bn, int B, int H, float* __restrict__ dz, float* __restrict__ part_db, int Hc, PlaneOut po) {
  __shared__ float4 sm[4][64];
  const PlaneDst pd = plane_dst(po);
  const int c = blockIdx.x * 256 + (threadIdx.x & 63) * 4;
  float4 zero = make_float4(0, 0, 0, 0);
  float4 mu = zero, rs = zero, c0 = zero, c1 = zero, c2 = zero;
  if (c < H && bn) {
    const int cc = c % Hc;
    mu = ld4(mean + cc); rs = ld4(rstd + cc);
    c0 = ld4(coef + cc); c1 = ld4(coef + Hc + cc); c2 = ld4(coef + 2 * Hc + cc);
  }
  if (bn) bn_bwd_dz_rows<true>(g, bits, z, mu, rs, c0, c1, c2, kscale, B, H, dz, part_db, pd, sm);
  else bn_bwd_dz_rows<false>(g, bits, z, mu, rs, c0, c1, c2, kscale, B, H, dz, part_db, pd, sm);
}

__global__ void bn_fold_eval_kernel(const float* __restrict__ bias, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, const float* __restrict__ rm,
                                    const float* __restrict__ rv, float eps, int bn, int H,
                                    float* __restrict__ scale, float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= H) return;
  if (bn) {
    const float s = gamma[c] * (1.0f / sqrtf(rv[c] + eps));
    scale[c] = s;
    shift[c] = fmaf(bias[c] - rm[c], s, beta[c]);
  } else {
    scale[c] = 1.f;
    shift[c] = bias[c];
  }
}

// eval-mode BatchNorm as the training kernels see it: "batch" statistics := the running ones
__global__ void bn_eval_stats_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ rm, const float* __restrict__ rv, float eps, int H,
                                     float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ scale,
                                     float* __restrict__ shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= H) return;
  const float r = 1.0f / sqrtf(rv[c] + eps), sc = gamma[c] * r;
  mean[c] = rm[c]; rstd[c] = r; scale[c] = sc; shift[c] = bn_shift_of(beta[c], rm[c], sc);
}

inline int stream_rows_grid(int B, int strips) {
  // ~2048 workgroups in flight (8 per CU), 4 rows per workgroup pass
  int gy = (2048 + strips - 1) / strips;
  const int need = (B + 3) / 4;
  if (gy > need) gy = need;
  return gy < 1 ? 1 : gy;
}

}  // namespace

// (sum, M2) partials over 64-row groups (what a GEMM epilogue emits) merged F at a time, in group order (Chan et al.), into
// the [2][Gp][H] layout bn_finalize walks with group_rows = 64 F: a 1M-pixel map has 16384 such partials per column.
// (in namespace pl itself, as it always was: the kernel keeps its symbol name)
__global__ __launch_bounds__(NTHR) void bn_merge_groups_kernel(const float* __restrict__ in, int G, int rows, int H, int F,
                                                               float* __restrict__ out, int Gp) {
  const int c = blockIdx.x * NTHR + threadIdx.x;
  if (c >= H) return;
  const int gp = blockIdx.y;
  const size_t GH = (size_t)G * H;
  float S = 0.f, Q = 0.f, na = 0.f;
  for (int f0 = 0; f0 < F; f0 += 8) {
    float s[8], q[8], n[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {                       // eight groups' loads in flight
      const int g = gp * F + f0 + u;
      n[u] = (f0 + u < F && g < G) ? (float)max(0, min(64, rows - 64 * g)) : 0.f;
      s[u] = q[u] = 0.f;
      if (n[u] > 0.f) { s[u] = in[(size_t)g * H + c]; q[u] = in[GH + (size_t)g * H + c]; }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (n[u] == 0.f) continue;
      if (na == 0.f) { S = s[u]; Q = q[u]; na = n[u]; continue; }
      const float d = s[u] / n[u] - S / na;
      Q += q[u] + d * d * (na * n[u] / (na + n[u]));
      S += s[u];
      na += n[u];
    }
  }
  out[(size_t)gp * H + c] = S;
  out[(size_t)Gp * H + (size_t)gp * H + c] = Q;
}

// =====================================================================================
// launchers
// =====================================================================================
int launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((a.H + RCOLS - 1) / RCOLS), dim3(NTHR), 0, s, a.stat, a.G, a.world, a.B,
                     a.H, a.group_rows, a.bn.gamma, a.bn.beta, a.bn.eps, a.bn.momentum, a.bn.running_mean, a.bn.running_var,
                     a.bn.batches, a.mean, a.rstd, a.scale, a.shift);
  PL_CHECK_LAUNCH("bn_finalize");
  return PL_OK;
}

int launch_bn_apply(const BnApplyArgs& a, hipStream_t s) {
  const int B = a.B, H = a.H;
  PlaneOut po = a.planes;
  po.nt = (int64_t)B * H * 4 >= kNontemporalBytes ? 1 : 0;
  if (!a.act && !po.kind) PL_FAIL(PL_EINVAL, "bn_apply: nothing to write");
  // the kernel's mode word: the dropout mode (0 .. 3) + 8: no ReLU + 32: the residual joins before the ReLU
  const int mode = a.drop.mode | (a.no_relu ? 8 : 0) | (a.resid_before_relu ? 32 : 0);
  const int strips = (H + 255) / 256;
  dim3 grid(strips, stream_rows_grid(B, strips));
  BnFin fin = {};
  if (a.fin.stat) {
    const BnFinalizeArgs& f = a.fin;
    if (!f.bn.gamma || !f.bn.beta || !f.mean || !f.rstd || f.G < 1 || f.G > 16 || (H & 3) ||
        (f.bn.running_mean != nullptr) != (f.bn.running_var != nullptr))
      PL_FAIL(PL_EINVAL, "bn_apply: statistics finalize (G=%d)", f.G);
    fin = BnFin{f.stat, f.bn.gamma, f.bn.beta, f.bn.running_mean, f.bn.running_var, f.mean, f.rstd, f.bn.batches, f.bn.eps,
                f.bn.momentum, f.G, B, f.group_rows};
  }
  const DropKey& k = a.drop;
  hipLaunchKernelGGL(bn_apply_kernel, grid, dim3(NTHR), 0, s, a.z, a.scale, a.shift, a.resid, a.act, a.bits, B, H,
                     mode, k.thr, k.kscale, k.k0, k.k1, k.c3, k.layer, k.inject, a.Hc > 0 ? a.Hc : H, po, k.step_dev, k.seed_hi,
                     fin);
  PL_CHECK_LAUNCH("bn_apply");
  return PL_OK;
}

int launch_bn_small_fwd(const BnSmallFwdArgs& a, hipStream_t s) {
  const int B = a.B, H = a.H;
  if (!a.saved.z || !a.act || !a.saved.bits || !a.saved.mean || !a.saved.rstd || B < 2 || (H & 3))
    PL_FAIL(PL_EINVAL, "bn_small_fwd: bad arguments");
  if (B > kBnSmallRows) PL_FAIL(PL_ESHAPE, "bn_small_fwd: B=%d", B);
  const dim3 grid((H + 255) / 256), block(kSmallThreads);
  const DropKey& k = a.drop;
#define PL_SMALL_FWD(RU, RES)                                                                                              \
  hipLaunchKernelGGL((bn_small_fwd_kernel<RU, RES>), grid, block, 0, s, a.saved.z, a.bn.gamma, a.bn.beta, a.bn.eps,        \
                     a.bn.momentum, a.bn.running_mean, a.bn.running_var, a.bn.batches, a.saved.mean, a.saved.rstd, a.resid, \
                     a.act, a.saved.bits, B, H, k.mode, k.thr, k.kscale, k.k0, k.k1, k.c3, k.layer, k.inject, k.step_dev,   \
                     k.seed_hi)
  if (a.resid) PL_SMALL_FWD(8, true); else PL_SMALL_FWD(8, false);
#undef PL_SMALL_FWD
  PL_CHECK_LAUNCH("bn_small_fwd");
  return PL_OK;
}

int launch_bn_small_bwd(const BnSmallBwdArgs& a, hipStream_t s) {
  const SmallBnLayer& l = a.layer;
  const int B = a.B, H = a.H;
  if (!a.g || !l.saved.bits || !l.saved.z || !a.dz || !l.dgamma || !l.dbeta || !l.dbias || B < 1 || (H & 3))
    PL_FAIL(PL_EINVAL, "bn_small_bwd: bad arguments");
  if (B > kBnSmallRows) PL_FAIL(PL_ESHAPE, "bn_small_bwd: B=%d", B);
  const dim3 grid((H + 255) / 256), block(kSmallThreads);
  if (l.saved.tile_bits && (H & 255)) PL_FAIL(PL_ESHAPE, "bn_small_bwd: tile-format bitmap with H=%d", H);
#define PL_SMALL_BWD(TILE)                                                                                              \
  hipLaunchKernelGGL((bn_small_bwd_kernel<8, TILE>), grid, block, 0, s, a.g, l.saved.bits, l.saved.z, l.saved.mean,     \
                     l.saved.rstd, l.gamma, a.keep_scale, B, H, a.dz, l.dgamma, l.dbeta, l.dbias)
  if (l.saved.tile_bits) PL_SMALL_BWD(true); else PL_SMALL_BWD(false);
#undef PL_SMALL_BWD
  PL_CHECK_LAUNCH("bn_small_bwd");
  return PL_OK;
}

// Row chunks of the two backward streaming passes over a [B][H] matrix (grid.y; one partial row per chunk).
// 32 rows per chunk, capped so that strips x chunks stays near 1024 workgroups (4 per CU) and never below 128:
// a 256-column map of the conv path (one strip, 131072 rows) ran 128 workgroups on 256 CUs with the old flat cap;
// 2048 made the two streaming passes no faster and the finalize kernel (serial over the chunks) twice as slow.
int bwd_row_chunks(int B, int H) {
  const int strips = (H + 255) / 256;
  int cap = 1024 / strips;
  if (cap < 128) cap = 128;
  int rc = (B + 31) / 32;
  if (rc > cap) rc = cap;
  return rc < 1 ? 1 : rc;
}

int launch_bn_bwd_reduce(const BnBwdReduceArgs& a, hipStream_t s) {
  dim3 grid((a.H + 255) / 256, a.rc > 0 ? a.rc : bwd_row_chunks(a.B, a.H));
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, grid, dim3(NTHR), 0, s, a.g, a.saved.bits, a.saved.z, a.saved.mean, a.saved.rstd,
                     a.keep_scale, a.B, a.H, a.part_dy, a.part_dyz, a.Hc > 0 ? a.Hc : a.H, a.part_amax, a.join_g2, a.join_dx);
  PL_CHECK_LAUNCH("bn_bwd_reduce");
  return PL_OK;
}

int launch_bn_bwd_finalize(const BnBwdFinalizeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((a.H + RCOLS - 1) / RCOLS + (a.dz_scale ? 1 : 0)), dim3(NTHR), 0, s, a.part,
                     a.RC, a.world, a.rank, a.B, a.H, a.gamma, a.rstd, a.coef, a.dgamma, a.dbeta, a.part_amax, a.n_amax,
                     a.dz_scale, a.eval_mode, (long long)a.rstride, a.amax_world > 0 ? a.amax_world : 1);
  PL_CHECK_LAUNCH("bn_bwd_finalize");
  return PL_OK;
}

int launch_bn_bwd_dz(const BnBwdDzArgs& a, hipStream_t s) {
  dim3 grid((a.H + 255) / 256, a.rc > 0 ? a.rc : bwd_row_chunks(a.B, a.H));
  PlaneOut po = a.planes;
  po.nt = (int64_t)a.B * a.H * 4 >= kNontemporalBytes ? 1 : 0;
  if (!a.dz && !po.kind) PL_FAIL(PL_EINVAL, "bn_bwd_dz: nothing to write");
  hipLaunchKernelGGL(bn_bwd_dz_kernel, grid, dim3(NTHR), 0, s, a.g, a.saved.bits, a.saved.z, a.saved.mean, a.saved.rstd, a.coef,
                     a.keep_scale, a.bn, a.B, a.H, a.dz, a.part_db, a.Hc > 0 ? a.Hc : a.H, po);
  PL_CHECK_LAUNCH("bn_bwd_dz");
  return PL_OK;
}

int launch_bn_fold_eval(const float* bias, const BnParams* bn, int H, float* scale, float* shift, hipStream_t s) {
  const BnParams b = bn ? *bn : BnParams{};
  hipLaunchKernelGGL(bn_fold_eval_kernel, dim3((H + NTHR - 1) / NTHR), dim3(NTHR), 0, s, bias, b.gamma, b.beta,
                     (const float*)b.running_mean, (const float*)b.running_var, b.eps, bn ? 1 : 0, H, scale, shift);
  PL_CHECK_LAUNCH("bn_fold_eval");
  return PL_OK;
}

int launch_bn_eval_stats(const BnFinalizeArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(bn_eval_stats_kernel, dim3((a.H + NTHR - 1) / NTHR), dim3(NTHR), 0, s, a.bn.gamma, a.bn.beta,
                     (const float*)a.bn.running_mean, (const float*)a.bn.running_var, a.bn.eps, a.H, a.mean, a.rstd, a.scale,
                     a.shift);
  PL_CHECK_LAUNCH("bn_eval_stats");
  return PL_OK;
}

// =====================================================================================
// BatchNorm over the rows of a [rows][C] matrix as stand-alone entry points (the conv path: an NHWC feature
// map IS that matrix, BatchNorm2d = BatchNorm1d over its rows).  Same kernels as the lifter's layers.
// =====================================================================================
namespace {
// rows per statistics group: 64 (the GEMM epilogue's unit) up to 16 K rows, then 256 -- a 131072-row map would
// otherwise hand the finalize kernel 2048 partials per column (38 us per layer)
// (1024 for maps so large that 256-row groups would leave > 1024 partials per column: the statistics kernel merges
//  its 64-row sub-groups itself, so longer groups only cost workgroup count)
int bn_group_rows(int64_t rows) { return rows > 262144 ? 1024 : (rows > 16384 ? 256 : 64); }
int bn_groups(int64_t rows) { const int gs = bn_group_rows(rows); return (int)((rows + gs - 1) / gs); }
// replicas of a narrow map: [rows][C] is worked on as [rows/R][R*C] (bn_colstats_kernel)
// (static: tests/test_conv_planes_host.py ties conv.py's copy to this function's text)
static int bn_replicas(int64_t rows, int64_t C) {
  int r = C <= 64 ? 4 : (C <= 128 ? 2 : 1);
  while (r > 1 && (rows % r != 0 || rows / r < 2)) r >>= 1;
  return r;
}

// The view the streaming kernels take of a [rows][C] map -- [B = rows / R][H = R C], Hc = C real columns -- and where
// the conv-path entry points keep what in their scratch buffer (float offsets; pl_bn_train_scratch_bytes sizes it for both
// directions).
//   forward:  stat [2][R G][Hc] | scale [Hc] | shift [Hc]        (a GEMM's statistics merged first: [2][<= 512][Hc] | ...)
//   backward: part [2][R RC][Hc] | coef [3][Hc] | part_db [RC R][Hc] | amax [strips RC][2] (the dz range maxima)
struct BnScratch {
  int R, B, H, Hc;
  int G, gs;                     // forward: statistics groups of gs rows
  int RC, n_amax;                // backward: row chunks; workgroups of pass 1
  size_t scale;                  // forward: scale at this offset, shift Hc behind it
  size_t coef, part_db, amax;    // backward
  size_t fwd_floats, bwd_floats;
};
BnScratch bn_scratch(int64_t rows, int64_t C) {
  BnScratch q = {};
  q.R = bn_replicas(rows, C);
  q.B = (int)(rows / q.R); q.H = (int)C * q.R; q.Hc = (int)C;
  q.G = bn_groups(q.B); q.gs = bn_group_rows(q.B);
  q.RC = bwd_row_chunks(q.B, q.H);
  q.n_amax = ((q.H + 255) / 256) * q.RC;
  q.scale = (size_t)2 * q.R * q.G * q.Hc;
  q.fwd_floats = std::max(q.scale, (size_t)2 * 512 * q.Hc) + 2 * (size_t)q.Hc;
  q.coef = (size_t)2 * q.R * q.RC * q.Hc;
  q.part_db = q.coef + 3 * (size_t)q.Hc;
  q.amax = q.part_db + (size_t)q.RC * q.R * q.Hc;
  q.bwd_floats = q.amax + (size_t)2 * q.n_amax + 16;
  return q;
}

// BatchNorm backward of a [rows][C] map in three launches -- pass 1, the finalize, dz -- on the scratch layout above.
// join_dx != NULL (pl_bn_join_bwd): pass 1 first forms the incoming gradient, (g + join_g2) where the bitmap is set, and
// writes it to join_dx; dz then reads it from there.
struct ConvBnBwd {
  const float* g;
  const float* join_g2;
  float* join_dx;
  BnSaved saved;
  const float* gamma;
  float *dz, *dgamma, *dbeta;
  PlaneOut planes;              // dz also / only (dz == NULL) as operand planes
  float* dz_scale;              // fp16 planes: receives {S, 1/S} (bn_bwd_finalize_kernel)
};
// (BnSaved is written by a forward and read here: the C ABI hands the backward const pointers)
BnSaved conv_saved(const float* z, const uint64_t* bits, const float* mean, const float* rstd) {
  return BnSaved{const_cast<float*>(z), const_cast<uint64_t*>(bits), const_cast<float*>(mean), const_cast<float*>(rstd), false};
}
int conv_bn_bwd(const ConvBnBwd& a, int64_t rows, int64_t C, void* scratch, hipStream_t s) {
  const BnScratch q = bn_scratch(rows, C);
  float* part = static_cast<float*>(scratch);
  float* amax = a.dz_scale ? part + q.amax : nullptr;
  BnBwdReduceArgs r = {};
  r.g = a.g; r.saved = a.saved; r.keep_scale = 1.0f; r.B = q.B; r.H = q.H; r.Hc = q.Hc;
  r.part_dy = part; r.part_dyz = part + (size_t)q.RC * q.Hc; r.part_amax = amax;
  r.join_g2 = a.join_g2; r.join_dx = a.join_dx;
  PL_TRY(launch_bn_bwd_reduce(r, s));
  BnBwdFinalizeArgs f = {};
  f.part = part; f.RC = q.RC; f.world = q.R; f.rank = q.R > 1 ? -1 : 0; f.B = q.B; f.H = q.Hc;
  f.gamma = a.gamma; f.rstd = a.saved.rstd; f.coef = part + q.coef; f.dgamma = a.dgamma; f.dbeta = a.dbeta;
  f.part_amax = amax; f.n_amax = q.n_amax; f.dz_scale = a.dz_scale;
  PL_TRY(launch_bn_bwd_finalize(f, s));
  BnBwdDzArgs d = {};
  d.g = a.join_dx ? a.join_dx : a.g; d.saved = a.saved; d.coef = f.coef; d.keep_scale = 1.0f; d.bn = 1;
  d.B = q.B; d.H = q.H; d.Hc = q.Hc; d.dz = a.dz; d.part_db = part + q.part_db; d.planes = a.planes;
  return launch_bn_bwd_dz(d, s);
}

}  // namespace
}  // namespace pl

extern "C" size_t pl_bn_train_scratch_bytes(int64_t rows, int64_t C) {
  if (rows <= 0 || C <= 0) return 0;
  const pl::BnScratch q = pl::bn_scratch(rows, C);
  return std::max(q.fwd_floats, q.bwd_floats) * sizeof(float);
}

extern "C" int pl_bn_train_fwd(const float* z, int64_t rows, int64_t C, const float* gamma, const float* beta, float eps,
                               float momentum, float* running_mean, float* running_var, int64_t* batches, int relu,
                               float* y, uint64_t* bits, float* mean, float* rstd, void* scratch, void* stream) {
  if (!y) PL_FAIL(PL_EINVAL, "pl_bn_train_fwd: null pointer");
  return pl_bn_train_fwd_ex(z, rows, C, gamma, beta, eps, momentum, running_mean, running_var, batches, relu, y, bits, mean,
                            rstd, scratch, nullptr, 0, nullptr, nullptr, stream);
}

// + y_planes (optional): the output also / only (y == NULL) as operand planes of the next 1x1 convolution's planes GEMM
extern "C" int pl_bn_train_fwd_ex(const float* z, int64_t rows, int64_t C, const float* gamma, const float* beta, float eps,
                                  float momentum, float* running_mean, float* running_var, int64_t* batches, int relu,
                                  float* y, uint64_t* bits, float* mean, float* rstd, void* scratch, void* y_planes,
                                  int planes_mode, const float* gemm_stat, const float* join, void* stream) {
  if (!z || !gamma || !beta || (!y && !y_planes) || !bits || !mean || !rstd || !scratch) PL_FAIL(PL_EINVAL, "pl_bn_train_fwd: null pointer");
  // the streaming kernels take z, join and y as float4 and the bitmap as 64-bit words (bn_colstats_kernel, bn_apply_rows);
  // gamma, beta, mean, rstd and the running statistics only meet element code (bn_finalize_kernel)
  PL_REQUIRE_ALIGNED16("pl_bn_train_fwd", z);
  PL_REQUIRE_ALIGNED16("pl_bn_train_fwd", y);
  PL_REQUIRE_ALIGNED16("pl_bn_train_fwd", bits);
  PL_REQUIRE_ALIGNED16("pl_bn_train_fwd", join);
  pl::PlaneOut ypo;
  PL_TRY(pl::plane_out_of(planes_mode, y_planes, rows * C, pl::kConvActPlaneScale, nullptr, &ypo, "pl_bn_train_fwd_ex"));
  pl::range_watch(ypo, PL_RANGE_SITE_CONV_ACT);
  if (rows < 2 || rows > INT32_MAX || C <= 0 || (C & 3)) PL_FAIL(rows < 2 ? PL_EBATCH : PL_ESHAPE, "pl_bn_train_fwd: rows=%lld C=%lld (C %% 4 == 0, rows >= 2)", (long long)rows, (long long)C);
  hipStream_t s = (hipStream_t)stream;
  const pl::BnScratch q = pl::bn_scratch(rows, C);
  float* stat = static_cast<float*>(scratch);
  pl::BnFinalizeArgs f = {};
  f.bn = pl::BnParams{gamma, beta, eps, momentum, running_mean, running_var, batches};
  f.H = q.Hc; f.mean = mean; f.rstd = rstd;
  if (gemm_stat) {
    // the convolution's GEMM epilogue already left (sum, M2) per 64-row group and column: [2][gemm_stat_groups(rows)][C]
    // -- no pass over z for the statistics; more than 512 groups are merged F at a time first
    const int G64 = pl::gemm_stat_groups((int)rows);
    f.stat = gemm_stat; f.G = G64; f.group_rows = 64; f.world = 1; f.B = (int)rows;
    f.scale = stat + q.scale;
    if (G64 > 512) {
      const int F = (G64 + 511) / 512;
      f.G = (G64 + F - 1) / F; f.group_rows = 64 * F;
      f.stat = stat;                                     // (the merged partials: scratch >= 2 * 512 * C floats)
      f.scale = stat + (size_t)2 * f.G * q.Hc;
      hipLaunchKernelGGL(pl::bn_merge_groups_kernel, dim3((q.Hc + pl::NTHR - 1) / pl::NTHR, f.G), dim3(pl::NTHR), 0, s, gemm_stat, G64, (int)rows,
                         q.Hc, F, stat, f.G);
      PL_CHECK_LAUNCH("bn_merge_groups");
    }
  } else {
    hipLaunchKernelGGL(pl::bn_colstats_kernel, dim3((q.H + 255) / 256, q.G), dim3(pl::NTHR), 0, s, z, q.B, q.H, q.gs, q.Hc, stat);
    PL_CHECK_LAUNCH("bn_colstats");
    f.stat = stat; f.G = q.G; f.group_rows = q.gs; f.world = q.R; f.B = q.B;
    f.scale = stat + q.scale;
  }
  f.shift = f.scale + q.Hc;
  PL_TRY(pl::launch_bn_finalize(f, s));
  // join (optional): y = relu(bn(z) + join) in this one pass -- the Bottleneck's bn3 and residual join (needs relu != 0)
  if (join && !relu) PL_FAIL(PL_EINVAL, "pl_bn_train_fwd_ex: a join without its ReLU");
  pl::BnApplyArgs ap = {};
  ap.z = z; ap.scale = f.scale; ap.shift = f.shift; ap.resid = join; ap.act = y; ap.bits = bits;
  ap.B = q.B; ap.H = q.H; ap.Hc = q.Hc;
  ap.no_relu = !relu; ap.resid_before_relu = join != nullptr;
  ap.drop = pl::dropout_key(0.f, 0, 0, 0, nullptr, nullptr);
  ap.planes = ypo;
  return pl::launch_bn_apply(ap, s);
}

extern "C" int pl_bn_train_bwd(const float* dy, const uint64_t* bits, const float* z, const float* mean, const float* rstd,
                               const float* gamma, int64_t rows, int64_t C, float* dz, float* dgamma, float* dbeta,
                               void* scratch, void* stream) {
  if (!dz) PL_FAIL(PL_EINVAL, "pl_bn_train_bwd: null pointer");
  return pl_bn_train_bwd_ex(dy, bits, z, mean, rstd, gamma, rows, C, dz, dgamma, dbeta, scratch, nullptr, 0, nullptr, stream);
}

// + dz_planes (optional): dz also / only (dz == NULL) as operand planes of the 1x1 convolution's dgrad / wgrad planes GEMMs.
// PL_F16X3: the fp16 planes hold S * dz with S the power of two from the range bound of the lifter's layers
// (bn_bwd_finalize_kernel); dz_scale (device, 2 floats) receives {S, 1/S} -- the GEMMs take &dz_scale[1] as dyn_inv.
extern "C" int pl_bn_train_bwd_ex(const float* dy, const uint64_t* bits, const float* z, const float* mean, const float* rstd,
                                  const float* gamma, int64_t rows, int64_t C, float* dz, float* dgamma, float* dbeta,
                                  void* scratch, void* dz_planes, int planes_mode, float* dz_scale, void* stream) {
  if (!dy || !bits || !z || !mean || !rstd || !gamma || (!dz && !dz_planes) || !dgamma || !dbeta || !scratch)
    PL_FAIL(PL_EINVAL, "pl_bn_train_bwd: null pointer");
  // float4 / 64-bit in bn_bwd_reduce_kernel and bn_bwd_dz_kernel (mean and rstd: four columns per lane); gamma, dgamma and
  // dbeta only meet element code (bn_bwd_finalize_kernel)
  PL_REQUIRE_ALIGNED16("pl_bn_train_bwd", dy);
  PL_REQUIRE_ALIGNED16("pl_bn_train_bwd", bits);
  PL_REQUIRE_ALIGNED16("pl_bn_train_bwd", z);
  PL_REQUIRE_ALIGNED16("pl_bn_train_bwd", mean);
  PL_REQUIRE_ALIGNED16("pl_bn_train_bwd", rstd);
  PL_REQUIRE_ALIGNED16("pl_bn_train_bwd", dz);
  if (rows < 2 || rows > INT32_MAX || C <= 0 || (C & 3)) PL_FAIL(PL_ESHAPE, "pl_bn_train_bwd: rows=%lld C=%lld", (long long)rows, (long long)C);
  const bool scaled = dz_planes && planes_mode == PL_F16X3;
  if (scaled && !dz_scale) PL_FAIL(PL_EINVAL, "pl_bn_train_bwd_ex: fp16 planes of dz need dz_scale");
  pl::ConvBnBwd a = {};
  PL_TRY(pl::plane_out_of(planes_mode, dz_planes, rows * C, 1.0f, scaled ? dz_scale : nullptr, &a.planes, "pl_bn_train_bwd_ex"));
  a.g = dy; a.saved = pl::conv_saved(z, bits, mean, rstd); a.gamma = gamma; a.dz = dz; a.dgamma = dgamma; a.dbeta = dbeta;
  a.dz_scale = scaled ? dz_scale : nullptr;
  return pl::conv_bn_bwd(a, rows, C, scratch, (hipStream_t)stream);
}

// Backward of the Bottleneck's bn3 + residual join (pl_bn_train_fwd_ex with `join`; Resnet.py:81-91) in three launches: dx = (g + g2)
// where the join's bitmap is set (the identity's gradient AND bn3's dy; g2 may be NULL) written by the same pass that takes
// BatchNorm-backward's column sums of it (no separate pl_mask_add_by_bits pass and no re-read of dx for the sums), the finalize,
// then dz (fp32 and / or planes as pl_bn_train_bwd_ex).  C >= 256 (no column replication: the bitmap is per (row, channel)).
extern "C" int pl_bn_join_bwd(const float* g, const float* g2, const uint64_t* bits, const float* z, const float* mean,
                              const float* rstd, const float* gamma, int64_t rows, int64_t C, float* dx, float* dz, float* dgamma,
                              float* dbeta, void* scratch, void* dz_planes, int planes_mode, float* dz_scale, void* stream) {
  if (!g || !bits || !z || !mean || !rstd || !gamma || !dx || (!dz && !dz_planes) || !dgamma || !dbeta || !scratch)
    PL_FAIL(PL_EINVAL, "pl_bn_join_bwd: null pointer");
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", g);                 // (as pl_bn_train_bwd_ex; g2 and dx: bn_bwd_reduce_kernel's join)
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", g2);
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", bits);
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", z);
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", mean);
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", rstd);
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", dx);
  PL_REQUIRE_ALIGNED16("pl_bn_join_bwd", dz);
  if (rows < 2 || rows > INT32_MAX || C <= 0 || (C & 3)) PL_FAIL(PL_ESHAPE, "pl_bn_join_bwd: rows=%lld C=%lld", (long long)rows, (long long)C);
  if (pl::bn_replicas(rows, C) != 1) PL_FAIL(PL_ESHAPE, "pl_bn_join_bwd: C=%lld is narrower than one 256-column strip", (long long)C);
  const bool scaled = dz_planes && planes_mode == PL_F16X3;
  if (scaled && !dz_scale) PL_FAIL(PL_EINVAL, "pl_bn_join_bwd: fp16 planes of dz need dz_scale");
  pl::ConvBnBwd a = {};
  PL_TRY(pl::plane_out_of(planes_mode, dz_planes, rows * C, 1.0f, scaled ? dz_scale : nullptr, &a.planes, "pl_bn_join_bwd"));
  a.g = g; a.join_g2 = g2; a.join_dx = dx;
  a.saved = pl::conv_saved(z, bits, mean, rstd); a.gamma = gamma; a.dz = dz; a.dgamma = dgamma; a.dbeta = dbeta;
  a.dz_scale = scaled ? dz_scale : nullptr;
  return pl::conv_bn_bwd(a, rows, C, scratch, (hipStream_t)stream);
}

extern "C" int pl_add_relu_fwd(const float* a, const float* b, int64_t rows, int64_t C, float* out, uint64_t* bits,
                               void* stream) {
  return pl_add_relu_fwd_ex(a, b, rows, C, out, bits, nullptr, 0, stream);
}

// + out_planes (optional): the block output also as operand planes (the next block's 1x1 convolutions read those)
extern "C" int pl_add_relu_fwd_ex(const float* a, const float* b, int64_t rows, int64_t C, float* out, uint64_t* bits,
                                  void* out_planes, int planes_mode, void* stream) {
  if (!a || !b || !out || !bits) PL_FAIL(PL_EINVAL, "pl_add_relu_fwd: null pointer");
  PL_REQUIRE_ALIGNED16("pl_add_relu_fwd", a);                // (add_relu_kernel: float4 rows, 64-bit bitmap words)
  PL_REQUIRE_ALIGNED16("pl_add_relu_fwd", b);
  PL_REQUIRE_ALIGNED16("pl_add_relu_fwd", out);
  PL_REQUIRE_ALIGNED16("pl_add_relu_fwd", bits);
  if (rows <= 0 || rows > INT32_MAX || C <= 0 || (C & 3)) PL_FAIL(PL_ESHAPE, "pl_add_relu_fwd: rows=%lld C=%lld", (long long)rows, (long long)C);
  pl::PlaneOut po;
  PL_TRY(pl::plane_out_of(planes_mode, out_planes, rows * C, pl::kConvActPlaneScale, nullptr, &po, "pl_add_relu_fwd_ex"));
  pl::range_watch(po, PL_RANGE_SITE_CONV_ACT);
  const int strips = ((int)C + 255) / 256;
  dim3 grid(strips, pl::stream_rows_grid((int)rows, strips));
  hipLaunchKernelGGL(pl::add_relu_kernel, grid, dim3(pl::NTHR), 0, (hipStream_t)stream, a, b, out, bits, (int)rows, (int)C, po);
  PL_CHECK_LAUNCH("add_relu");
  return PL_OK;
}

extern "C" int pl_mask_by_bits(const float* g, const uint64_t* bits, int64_t rows, int64_t C, float* dx, void* stream) {
  return pl_mask_add_by_bits(g, nullptr, bits, rows, C, dx, stream);
}

// dx = (g + g2) where the bitmap is set, else 0: the residual join's backward with the sum of the two gradients that
// reach the block output (through the next join and through the next block's convolutions) folded in (g2 may be NULL)
extern "C" int pl_mask_add_by_bits(const float* g, const float* g2, const uint64_t* bits, int64_t rows, int64_t C, float* dx,
                                   void* stream) {
  if (!g || !bits || !dx) PL_FAIL(PL_EINVAL, "pl_mask_by_bits: null pointer");
  PL_REQUIRE_ALIGNED16("pl_mask_by_bits", g);                // (mask_by_bits_kernel: float4 rows, 64-bit bitmap words)
  PL_REQUIRE_ALIGNED16("pl_mask_by_bits", g2);
  PL_REQUIRE_ALIGNED16("pl_mask_by_bits", bits);
  PL_REQUIRE_ALIGNED16("pl_mask_by_bits", dx);
  if (rows <= 0 || rows > INT32_MAX || C <= 0 || (C & 3)) PL_FAIL(PL_ESHAPE, "pl_mask_by_bits: rows=%lld C=%lld", (long long)rows, (long long)C);
  const int strips = ((int)C + 255) / 256;
  dim3 grid(strips, pl::stream_rows_grid((int)rows, strips));
  hipLaunchKernelGGL(pl::mask_by_bits_kernel, grid, dim3(pl::NTHR), 0, (hipStream_t)stream, g, bits, dx, (int)rows, (int)C, g2);
  PL_CHECK_LAUNCH("mask_by_bits");
  return PL_OK;
}

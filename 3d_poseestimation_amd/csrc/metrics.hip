// Evaluation on the device: per-pose MPJPE / N-MPJPE / P-MPJPE (pl_pose_errors) and their per-group, per-joint sums and
// PCK counts (pl_pose_metrics_accum).  The per-pose arithmetic is pose_metrics.h, shared with pl_pose_errors_host.
#include <string.h>

#include "pl_internal.h"
#include "pose_metrics.h"
#include "pose_table.h"

namespace pl {
namespace {

constexpr int kPoseBlock = 64;        // poses per workgroup = lanes of its one wavefront

// One lane per pose.  The workgroup first brings its 64 poses of both tensors into LDS with coalesced 16-byte loads (a lane
// reading its own pose from global memory would stride 12 J bytes between lanes); a pose's row is padded to an odd number
// of floats so the 64 lanes, each walking its own row, fall on distinct banks.  pose_errors_one() leaves the aligned pose
// in the prediction's row and e[j][m] in the target's row; both leave the LDS coalesced again.
// XF (pl_pose_errors_t): both tensors are in a model's space; column c of a pose is taken back, x = y div[c] + sub[c]
// (pose_table.h invert1), on its way into the LDS.  XF = false is the kernel as it was and reads neither pointer.
// WT (pl_pose_errors_w): the workgroup's 64 x J slab of per-joint weights comes into a third LDS slab the same way (its
// row stride J | 1 is odd for the same reason; weights need only be 4-byte aligned, so up to three leading floats go
// singly before the 16-byte loads start) and the lane runs pose_errors_one_weighted().  WT = false reads no weight and is
// the instruction stream it was: the new parameter is the last one.
template <bool XF, bool WT>
__global__ __launch_bounds__(kPoseBlock) void pose_errors_kernel(const float* __restrict__ pred, const float* __restrict__ tgt,
                                                                 int64_t B, int J, float* __restrict__ err,
                                                                 float* __restrict__ aligned, const float* __restrict__ sub,
                                                                 const float* __restrict__ div,
                                                                 const float* __restrict__ weights) {
  extern __shared__ __align__(16) float lds[];
  const int W = 3 * J, S = W | 1;
  float* lp = lds;
  float* lt = lds + kPoseBlock * S;
  [[maybe_unused]] float* lw = lds + 2 * kPoseBlock * S;
  [[maybe_unused]] const int SJ = J | 1;
  const int tid = threadIdx.x;
  const int64_t b0 = (int64_t)blockIdx.x * kPoseBlock;
  const int nb = (int)((B - b0) < kPoseBlock ? (B - b0) : kPoseBlock);
  const int n = nb * W, n4 = n >> 2;                       // floats (and whole float4s) of this workgroup's slab
  const float* gp = pred + b0 * W;                         // 16-byte aligned: b0 * W * 4 is a multiple of 256
  const float* gt = tgt + b0 * W;
  const int drow = 256 / W, dcol = 256 % W;                // 64 lanes x 4 floats further on
  {
    int row = (4 * tid) / W, col = 4 * tid - row * W;
    for (int q = tid; q < n4; q += kPoseBlock) {
      const float4 vp = reinterpret_cast<const float4*>(gp)[q];
      const float4 vt = reinterpret_cast<const float4*>(gt)[q];
      const float ep[4] = {vp.x, vp.y, vp.z, vp.w}, et[4] = {vt.x, vt.y, vt.z, vt.w};
      int r = row, c = col;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if constexpr (XF) {
          lp[r * S + c] = pt::invert1(ep[k], sub[c], div[c]);
          lt[r * S + c] = pt::invert1(et[k], sub[c], div[c]);
        } else {
          lp[r * S + c] = ep[k];
          lt[r * S + c] = et[k];
        }
        if (++c == W) { c = 0; ++r; }
      }
      row += drow; col += dcol;
      if (col >= W) { col -= W; ++row; }
    }
    for (int i = 4 * n4 + tid; i < n; i += kPoseBlock) {   // at most 3 floats
      const int r = i / W, c = i - r * W;
      if constexpr (XF) {
        lp[r * S + c] = pt::invert1(gp[i], sub[c], div[c]);
        lt[r * S + c] = pt::invert1(gt[i], sub[c], div[c]);
      } else {
        lp[r * S + c] = gp[i];
        lt[r * S + c] = gt[i];
      }
    }
  }
  if constexpr (WT) {
    const int nw = nb * J;                                   // floats of this workgroup's slab of weights
    const float* gw = weights + b0 * J;
    int lead = (int)((0u - (unsigned)(reinterpret_cast<uintptr_t>(gw) >> 2)) & 3u);      // floats up to a 16-byte boundary
    lead = lead < nw ? lead : nw;
    const int nw4 = (nw - lead) >> 2;
    const float4* gw4 = reinterpret_cast<const float4*>(gw + lead);
    const int drw = 256 / J, dcw = 256 % J;
    int row = (lead + 4 * tid) / J, col = lead + 4 * tid - row * J;
    for (int q = tid; q < nw4; q += kPoseBlock) {
      const float4 v = gw4[q];
      const float e[4] = {v.x, v.y, v.z, v.w};
      int r = row, c = col;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        lw[r * SJ + c] = e[k];
        if (++c == J) { c = 0; ++r; }
      }
      row += drw; col += dcw;
      if (col >= J) { col -= J; ++row; }
    }
    if (tid < lead) lw[tid] = gw[tid];                       // lead <= 3 < J: row 0
    for (int i = lead + 4 * nw4 + tid; i < nw; i += kPoseBlock) {       // at most 3 floats
      const int r = i / J, c = i - r * J;
      lw[r * SJ + c] = gw[i];
    }
  }
  __syncthreads();
  if constexpr (WT) {
    if (tid < nb) plm::pose_errors_one_weighted(lp + tid * S, lt + tid * S, lw + tid * SJ, J);
  } else {
    if (tid < nb) plm::pose_errors_one(lp + tid * S, lt + tid * S, J);
  }
  __syncthreads();
  {
    const int ne = nb * J, dl = kPoseBlock / J, dj = kPoseBlock % J;
    int l = tid / J, j = tid - l * J;
    float* e0 = err + b0 * J;
    for (int i = tid; i < ne; i += kPoseBlock) {
      const float* src = lt + l * S + 3 * j;
      e0[i] = src[0];
      e0[(size_t)B * J + i] = src[1];
      e0[(size_t)2 * B * J + i] = src[2];
      l += dl; j += dj;
      if (j >= J) { j -= J; ++l; }
    }
  }
  if (aligned) {
    float* ga = aligned + b0 * W;
    int row = (4 * tid) / W, col = 4 * tid - row * W;
    for (int q = tid; q < n4; q += kPoseBlock) {
      float v[4];
      int r = row, c = col;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = lp[r * S + c];
        if (++c == W) { c = 0; ++r; }
      }
      reinterpret_cast<float4*>(ga)[q] = make_float4(v[0], v[1], v[2], v[3]);
      row += drow; col += dcol;
      if (col >= W) { col -= W; ++row; }
    }
    for (int i = 4 * n4 + tid; i < n; i += kPoseBlock) {
      const int r = i / W, c = i - r * W;
      ga[i] = lp[r * S + c];
    }
  }
}

// ---- accumulation: two stages, no atomics, a fixed order of every sum ---------------------------------------------------
// Stage 1, workgroup (chunk c of rows, metric m, job tt): tt < T counts errors <= thr[tt], tt == T sums errors; either way
// into one 32-bit cell per (group, joint): part[c][m][tt][g][j].  Lane (h, j) = (tid / 32, tid % 32) takes the rows of its
// parity h and owns column j of the LDS table acc[h][.][j], so no two lanes ever touch a cell.  The (0, T) workgroup of a
// chunk also counts the chunk's poses per group, lane k owning group k (k == G: ids outside [0, G)).
// Stage 2, one thread per output cell: the chunks' partials in order, then += into the accumulator.
constexpr int kAccMaxGroups = 32, kAccMaxThr = 32, kAccLanesJ = 32;
constexpr int kAccMinRows = 128, kAccMaxChunks = 64;

// WT (pl_pose_metrics_accum_w): weights [B][J] mask every entry, w > 0 or the entry is in no sum and no count; the weight is
// loaded beside the error it gates and acts as a select (the entry is skipped), so a NaN error behind a zero weight is in
// nothing.  The grid gets one more job, tt == T + 1 of metric 0: the visible entries per (group, joint), a count that reads
// no error (the weights stand in for it); a chunk's partial grows by those G J cells, which follow its 3 (T + 1) G J.  WT = false is the code as it was.
struct AccumShape {
  int nc, rows;       // chunks, rows per chunk
  size_t cells;       // 32-bit cells of one chunk's sums-and-counts partial: 3 (T + 1) G J
  size_t bytes;
};

AccumShape accum_shape(int64_t B, int64_t J, int G, int T, bool weighted = false) {
  AccumShape s;
  int64_t rows = (B + kAccMaxChunks - 1) / kAccMaxChunks;
  if (rows < kAccMinRows) rows = kAccMinRows;
  s.rows = (int)rows;
  s.nc = (int)((B + rows - 1) / rows);
  s.cells = (size_t)3 * (size_t)(T + 1) * (size_t)G * (size_t)J;
  s.bytes = (size_t)s.nc * (s.cells + (weighted ? (size_t)G * (size_t)J : 0) + (size_t)(G + 1)) * 4;
  return s;
}

template <bool WT>
__global__ __launch_bounds__(64) void pose_metrics_partial_kernel(const float* __restrict__ err, int B, int J,
                                                                  const int32_t* __restrict__ group, int G,
                                                                  const float* __restrict__ thr, int T, int rows,
                                                                  uint32_t* __restrict__ part, int32_t* __restrict__ part_n,
                                                                  const float* __restrict__ weights) {
  __shared__ uint32_t acc[2][kAccMaxGroups][kAccLanesJ];
  const int c = blockIdx.x, m = blockIdx.y, tt = blockIdx.z;
  [[maybe_unused]] const bool valid = WT && tt == T + 1;   // the visible-entry count
  if constexpr (WT) {
    if (valid && m != 0) return;                           // (uniform over the workgroup, before any barrier)
  }
  const int tid = threadIdx.x, h = tid >> 5, j = tid & 31;
  const int64_t r0 = (int64_t)c * rows, r1 = (r0 + rows < B) ? r0 + rows : (int64_t)B;
  const bool sums = tt == T;
  for (int g = 0; g < G; ++g) acc[h][g][j] = 0u;           // 0 is 0.0f too; the owner zeroes its own column
  if (j < J) {
    float bound;
    if constexpr (WT) bound = sums ? 0.f : (valid ? INFINITY : thr[tt]);       // 0 <= inf: every visible entry counts
    else bound = sums ? 0.f : thr[tt];
    const float* e = err + (size_t)m * B * J + j;
    if constexpr (WT) e = valid ? weights + j : e;         // the visible count reads no error: its "error" is the weight, <= inf
    // eight rows' loads in flight before their (ordered, possibly same-cell) LDS updates: the loop is latency-bound
    constexpr int U = 8;
    for (int64_t r = r0 + h; r < r1; r += 2 * U) {
      int g[U];
      float v[U];
      [[maybe_unused]] float w[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t rr = r + 2 * u;
        const bool in = rr < r1;
        g[u] = in ? (group ? group[rr] : 0) : -1;
        v[u] = in ? e[(size_t)rr * J] : 0.f;
        if constexpr (WT) w[u] = in ? weights[(size_t)rr * J + j] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((unsigned)g[u] >= (unsigned)G) continue;
        if constexpr (WT) {
          if (!(w[u] > 0.0f)) continue;                      // not visible (zero, negative, NaN): in no sum and no count
        }
        if (sums) acc[h][g[u]][j] = __float_as_uint(__uint_as_float(acc[h][g[u]][j]) + v[u]);
        else acc[h][g[u]][j] += (v[u] <= bound) ? 1u : 0u;
      }
    }
  }
  __syncthreads();
  if (j < J) {
    uint32_t* out;
    if constexpr (WT)            // job m (T + 1) + tt of the chunk's 3 (T + 1) + 1; the visible-entry count is the last
      out = part + (((size_t)c * (3 * (T + 1) + 1) + (valid ? 3 * (T + 1) : m * (T + 1) + tt)) * G) * J + j;
    else
      out = part + ((((size_t)c * 3 + m) * (T + 1) + tt) * G) * J + j;
    for (int g = h; g < G; g += 2) {
      const uint32_t a = acc[0][g][j], b = acc[1][g][j];
      out[(size_t)g * J] = sums ? __float_as_uint(__uint_as_float(a) + __uint_as_float(b)) : a + b;
    }
  }
  if (sums && m == 0 && tid <= G) {
    int n = 0;
    for (int64_t r = r0; r < r1; ++r) {
      const int g = group ? group[r] : 0;
      n += (tid < G) ? (g == tid) : ((unsigned)g >= (unsigned)G);
    }
    part_n[(size_t)c * (G + 1) + tid] = n;
  }
}

__global__ void pose_metrics_final_kernel(const uint32_t* __restrict__ part, const int32_t* __restrict__ part_n, int nc,
                                          int J, int G, int T, float* __restrict__ sums, int64_t* __restrict__ counts,
                                          int64_t* __restrict__ n_poses) {
  const int64_t cells = (int64_t)3 * (T + 1) * G * J;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cells) {                                         // i = ((m (T + 1) + tt) G + g) J + j, a chunk's own order
    const int j = (int)(i % J);
    const int g = (int)((i / J) % G);
    const int tt = (int)((i / ((int64_t)J * G)) % (T + 1));
    const int m = (int)(i / ((int64_t)J * G * (T + 1)));
    if (tt == T) {
      float s = 0.f;
#pragma unroll 8
      for (int c = 0; c < nc; ++c) s += __uint_as_float(part[(size_t)c * cells + i]);
      sums[((size_t)g * 3 + m) * J + j] += s;
    } else {
      int64_t s = 0;
#pragma unroll 8
      for (int c = 0; c < nc; ++c) s += part[(size_t)c * cells + i];
      counts[(((size_t)g * 3 + m) * T + tt) * J + j] += s;
    }
  } else if (i < cells + G + 1) {
    const int k = (int)(i - cells);
    int64_t s = 0;
    for (int c = 0; c < nc; ++c) s += part_n[(size_t)c * (G + 1) + k];
    n_poses[k] += s;
  }
}

// The same for pl_pose_metrics_accum_w, a kernel of its own so that the one above stays the text (and the instruction stream)
// it was: a chunk's partial is cells + G J long here, and the threads behind the pose counts add the chunks' visible-entry
// cells into n_valid.
__global__ void pose_metrics_final_weighted_kernel(const uint32_t* __restrict__ part, const int32_t* __restrict__ part_n, int nc,
                                                   int J, int G, int T, float* __restrict__ sums,
                                                   int64_t* __restrict__ counts, int64_t* __restrict__ n_poses,
                                                   int64_t* __restrict__ n_valid) {
  const int64_t cells = (int64_t)3 * (T + 1) * G * J;
  const int64_t stride = cells + (int64_t)G * J;           // 32-bit cells from one chunk's partial to the next
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cells) {                                         // i = ((m (T + 1) + tt) G + g) J + j, a chunk's own order
    const int j = (int)(i % J);
    const int g = (int)((i / J) % G);
    const int tt = (int)((i / ((int64_t)J * G)) % (T + 1));
    const int m = (int)(i / ((int64_t)J * G * (T + 1)));
    if (tt == T) {
      float s = 0.f;
#pragma unroll 8
      for (int c = 0; c < nc; ++c) s += __uint_as_float(part[(size_t)c * stride + i]);
      sums[((size_t)g * 3 + m) * J + j] += s;
    } else {
      int64_t s = 0;
#pragma unroll 8
      for (int c = 0; c < nc; ++c) s += part[(size_t)c * stride + i];
      counts[(((size_t)g * 3 + m) * T + tt) * J + j] += s;
    }
  } else if (i < cells + G + 1) {
    const int k = (int)(i - cells);
    int64_t s = 0;
    for (int c = 0; c < nc; ++c) s += part_n[(size_t)c * (G + 1) + k];
    n_poses[k] += s;
  } else if (i < cells + G + 1 + (int64_t)G * J) {
    const int64_t k = i - (cells + G + 1);                 // = g J + j, n_valid's own order
    int64_t s = 0;
#pragma unroll 8
    for (int c = 0; c < nc; ++c) s += part[(size_t)c * stride + cells + k];
    n_valid[k] += s;
  }
}

int check_pose_args(const char* who, const float* pred, const float* tgt, int64_t B, int64_t J, const float* err,
                    const float* aligned) {
  if (!pred || !tgt || !err) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  if (B <= 0 || B > INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: B=%lld outside 1..2^31-1", who, (long long)B);
  if (J < plm::kMinJoints || J > plm::kMaxJoints)
    PL_FAIL(PL_ESHAPE, "%s: J=%lld outside %d..%d", who, (long long)J, plm::kMinJoints, plm::kMaxJoints);
  if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(tgt) | reinterpret_cast<uintptr_t>(aligned)) & 15)
    PL_FAIL(PL_EINVAL, "%s: pred / tgt / aligned not 16-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(err) & 3) PL_FAIL(PL_EINVAL, "%s: err not 4-byte aligned", who);
  return PL_OK;
}

}  // namespace
}  // namespace pl

using namespace pl;

// pose_errors_kernel's only launch site; sub == nullptr / weights == nullptr: the instantiations without them
static int launch_pose_errors(const char* who, const float* pred, const float* tgt, int64_t B, int64_t J, float* err,
                              float* aligned_or_null, const float* sub, const float* div, const float* weights, void* stream) {
  PL_TRY(check_pose_args(who, pred, tgt, B, J, err, aligned_or_null));
  if (reinterpret_cast<uintptr_t>(weights) & 3) PL_FAIL(PL_EINVAL, "%s: weights not 4-byte aligned", who);
  const int S = (3 * (int)J) | 1;
  // 49,664 B at J = 32; with the weights' slab of 64 (J | 1) floats 58,112 B: under the 64 KB a launch may ask for without
  // a function attribute
  const size_t lds = ((size_t)2 * kPoseBlock * S + (weights ? (size_t)kPoseBlock * ((int)J | 1) : 0)) * sizeof(float);
  const unsigned grid = (unsigned)((B + kPoseBlock - 1) / kPoseBlock);
  const float* none = nullptr;
  if (weights && sub)
    hipLaunchKernelGGL((pose_errors_kernel<true, true>), dim3(grid), dim3(kPoseBlock), lds, (hipStream_t)stream, pred, tgt, B,
                       (int)J, err, aligned_or_null, sub, div, weights);
  else if (weights)
    hipLaunchKernelGGL((pose_errors_kernel<false, true>), dim3(grid), dim3(kPoseBlock), lds, (hipStream_t)stream, pred, tgt, B,
                       (int)J, err, aligned_or_null, none, none, weights);
  else if (sub)
    hipLaunchKernelGGL((pose_errors_kernel<true, false>), dim3(grid), dim3(kPoseBlock), lds, (hipStream_t)stream, pred, tgt, B,
                       (int)J, err, aligned_or_null, sub, div, none);
  else
    hipLaunchKernelGGL((pose_errors_kernel<false, false>), dim3(grid), dim3(kPoseBlock), lds, (hipStream_t)stream, pred, tgt, B,
                       (int)J, err, aligned_or_null, none, none, none);
  PL_CHECK_LAUNCH("pose_errors");
  return PL_OK;
}

extern "C" int pl_pose_errors(const float* pred, const float* tgt, int64_t B, int64_t J, float* err,
                              float* aligned_or_null, void* stream) {
  return launch_pose_errors("pl_pose_errors", pred, tgt, B, J, err, aligned_or_null, nullptr, nullptr, nullptr, stream);
}

extern "C" int pl_pose_errors_t(const float* pred, const float* tgt, int64_t B, int64_t J, const float* sub_or_null,
                                const float* div_or_null, float* err, float* aligned_or_null, void* stream) {
  if ((sub_or_null != nullptr) != (div_or_null != nullptr)) PL_FAIL(PL_EINVAL, "pl_pose_errors_t: sub and div come together");
  return launch_pose_errors("pl_pose_errors_t", pred, tgt, B, J, err, aligned_or_null, sub_or_null, div_or_null, nullptr, stream);
}

extern "C" int pl_pose_errors_w(const float* pred, const float* tgt, int64_t B, int64_t J, const float* weights_or_null,
                                const float* sub_or_null, const float* div_or_null, float* err, float* aligned_or_null,
                                void* stream) {
  if ((sub_or_null != nullptr) != (div_or_null != nullptr)) PL_FAIL(PL_EINVAL, "pl_pose_errors_w: sub and div come together");
  return launch_pose_errors("pl_pose_errors_w", pred, tgt, B, J, err, aligned_or_null, sub_or_null, div_or_null, weights_or_null,
                            stream);
}

// the host entries: weights / (sub, div) == nullptr run the text without them, as the launch above picks its instantiation
static int pose_errors_host(const char* who, const float* pred, const float* tgt, int64_t B, int64_t J, const float* weights,
                            const float* sub, const float* div, float* err, float* aligned_or_null) {
  PL_TRY(check_pose_args(who, pred, tgt, B, J, err, aligned_or_null));
  if (reinterpret_cast<uintptr_t>(weights) & 3) PL_FAIL(PL_EINVAL, "%s: weights not 4-byte aligned", who);
  const int W = 3 * (int)J;
  float p[3 * plm::kMaxJoints], t[3 * plm::kMaxJoints];
  for (int64_t b = 0; b < B; ++b) {
    memcpy(p, pred + b * W, W * sizeof(float));
    memcpy(t, tgt + b * W, W * sizeof(float));
    if (sub)
      for (int c = 0; c < W; ++c) {
        p[c] = pt::invert1(p[c], sub[c], div[c]);
        t[c] = pt::invert1(t[c], sub[c], div[c]);
      }
    if (weights) plm::pose_errors_one_weighted(p, t, weights + b * J, (int)J);
    else plm::pose_errors_one(p, t, (int)J);
    for (int j = 0; j < J; ++j)
      for (int m = 0; m < 3; ++m) err[((size_t)m * B + b) * J + j] = t[3 * j + m];
    if (aligned_or_null) memcpy(aligned_or_null + b * W, p, W * sizeof(float));
  }
  return PL_OK;
}

extern "C" int pl_pose_errors_host(const float* pred, const float* tgt, int64_t B, int64_t J, float* err,
                                   float* aligned_or_null) {
  return pose_errors_host("pl_pose_errors_host", pred, tgt, B, J, nullptr, nullptr, nullptr, err, aligned_or_null);
}

extern "C" int pl_pose_errors_w_host(const float* pred, const float* tgt, int64_t B, int64_t J, const float* weights_or_null,
                                     const float* sub_or_null, const float* div_or_null, float* err, float* aligned_or_null) {
  if ((sub_or_null != nullptr) != (div_or_null != nullptr)) PL_FAIL(PL_EINVAL, "pl_pose_errors_w_host: sub and div come together");
  return pose_errors_host("pl_pose_errors_w_host", pred, tgt, B, J, weights_or_null, sub_or_null, div_or_null, err,
                          aligned_or_null);
}

static int check_accum_shape(const char* who, int64_t B, int64_t J, int groups, int n_thr) {
  if (B <= 0 || B > INT32_MAX) PL_FAIL(PL_ESHAPE, "%s: B=%lld outside 1..2^31-1", who, (long long)B);
  if (J < plm::kMinJoints || J > plm::kMaxJoints)
    PL_FAIL(PL_ESHAPE, "%s: J=%lld outside %d..%d", who, (long long)J, plm::kMinJoints, plm::kMaxJoints);
  if (groups < 1 || groups > kAccMaxGroups) PL_FAIL(PL_ESHAPE, "%s: groups=%d outside 1..%d", who, groups, kAccMaxGroups);
  if (n_thr < 0 || n_thr > kAccMaxThr) PL_FAIL(PL_ESHAPE, "%s: n_thr=%d outside 0..%d", who, n_thr, kAccMaxThr);
  return PL_OK;
}

extern "C" size_t pl_pose_metrics_scratch_bytes(int64_t B, int64_t J, int groups, int n_thr) {
  if (check_accum_shape("pl_pose_metrics_scratch_bytes", B, J, groups, n_thr) != PL_OK) return 0;
  return accum_shape(B, J, groups, n_thr).bytes;
}

extern "C" size_t pl_pose_metrics_w_scratch_bytes(int64_t B, int64_t J, int groups, int n_thr) {
  if (check_accum_shape("pl_pose_metrics_w_scratch_bytes", B, J, groups, n_thr) != PL_OK) return 0;
  return accum_shape(B, J, groups, n_thr, true).bytes;
}

// the accumulation kernels' only launch sites; weights == nullptr: the kernels without them (n_valid unread)
static int launch_accum(const char* who, const float* err, const float* weights, int64_t B, int64_t J,
                        const int32_t* group_or_null, int groups, const float* thr_or_null, int n_thr, float* sums,
                        int64_t* counts, int64_t* n_poses, int64_t* n_valid, void* scratch, void* stream) {
  const AccumShape a = accum_shape(B, J, groups, n_thr, weights != nullptr);
  uint32_t* part = (uint32_t*)scratch;
  const size_t chunk = a.cells + (weights ? (size_t)groups * (size_t)J : 0);
  int32_t* part_n = (int32_t*)(part + (size_t)a.nc * chunk);
  hipStream_t s = (hipStream_t)stream;
  if (weights)
    hipLaunchKernelGGL(pose_metrics_partial_kernel<true>, dim3(a.nc, 3, n_thr + 2), dim3(64), 0, s, err, (int)B, (int)J,
                       group_or_null, groups, thr_or_null, n_thr, a.rows, part, part_n, weights);
  else
    hipLaunchKernelGGL(pose_metrics_partial_kernel<false>, dim3(a.nc, 3, n_thr + 1), dim3(64), 0, s, err, (int)B, (int)J,
                       group_or_null, groups, thr_or_null, n_thr, a.rows, part, part_n, (const float*)nullptr);
  PL_CHECK_LAUNCH("pose_metrics_partial");
  const int64_t threads = (int64_t)chunk + groups + 1;
  if (weights)
    hipLaunchKernelGGL(pose_metrics_final_weighted_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                       (const uint32_t*)part, (const int32_t*)part_n, a.nc, (int)J, groups, n_thr, sums, counts, n_poses, n_valid);
  else
    hipLaunchKernelGGL(pose_metrics_final_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s,
                       (const uint32_t*)part, (const int32_t*)part_n, a.nc, (int)J, groups, n_thr, sums, counts, n_poses);
  PL_CHECK_LAUNCH("pose_metrics_final");
  return PL_OK;
}

extern "C" int pl_pose_metrics_accum(const float* err, int64_t B, int64_t J, const int32_t* group_or_null, int groups,
                                     const float* thr_or_null, int n_thr, float* sums, int64_t* counts, int64_t* n_poses,
                                     void* scratch, void* stream) {
  const char* who = "pl_pose_metrics_accum";
  if (!err || !sums || !n_poses || !scratch) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PL_TRY(check_accum_shape(who, B, J, groups, n_thr));
  if (n_thr > 0 && (!thr_or_null || !counts)) PL_FAIL(PL_EINVAL, "%s: null thresholds / counts with n_thr=%d", who, n_thr);
  if ((reinterpret_cast<uintptr_t>(err) | reinterpret_cast<uintptr_t>(group_or_null) | reinterpret_cast<uintptr_t>(thr_or_null) |
       reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(scratch)) & 3)
    PL_FAIL(PL_EINVAL, "%s: err / group / thr / sums / scratch not 4-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(n_poses)) & 7)
    PL_FAIL(PL_EINVAL, "%s: counts / n_poses not 8-byte aligned", who);
  return launch_accum(who, err, nullptr, B, J, group_or_null, groups, thr_or_null, n_thr, sums, counts, n_poses, nullptr, scratch,
                      stream);
}

extern "C" int pl_pose_metrics_accum_w(const float* err, const float* weights, int64_t B, int64_t J,
                                       const int32_t* group_or_null, int groups, const float* thr_or_null, int n_thr,
                                       float* sums, int64_t* counts, int64_t* n_poses, int64_t* n_valid, void* scratch,
                                       void* stream) {
  const char* who = "pl_pose_metrics_accum_w";
  if (!err || !weights || !sums || !n_poses || !n_valid || !scratch) PL_FAIL(PL_EINVAL, "%s: null pointer", who);
  PL_TRY(check_accum_shape(who, B, J, groups, n_thr));
  if (n_thr > 0 && (!thr_or_null || !counts)) PL_FAIL(PL_EINVAL, "%s: null thresholds / counts with n_thr=%d", who, n_thr);
  if (reinterpret_cast<uintptr_t>(weights) & 3) PL_FAIL(PL_EINVAL, "%s: weights not 4-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(err) | reinterpret_cast<uintptr_t>(group_or_null) | reinterpret_cast<uintptr_t>(thr_or_null) |
       reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(scratch)) & 3)
    PL_FAIL(PL_EINVAL, "%s: err / group / thr / sums / scratch not 4-byte aligned", who);
  if (reinterpret_cast<uintptr_t>(n_valid) & 7) PL_FAIL(PL_EINVAL, "%s: n_valid not 8-byte aligned", who);
  if ((reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(n_poses)) & 7)
    PL_FAIL(PL_EINVAL, "%s: counts / n_poses not 8-byte aligned", who);
  return launch_accum(who, err, weights, B, J, group_or_null, groups, thr_or_null, n_thr, sums, counts, n_poses, n_valid, scratch,
                      stream);
}

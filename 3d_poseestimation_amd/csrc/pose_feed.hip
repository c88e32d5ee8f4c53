// The pose feed: flip_pose and the flip test-time augmentation's pack / merge, the batch gather, the seeded augmentation
// (with the person-centred crop and the columns' transform) applied where the row is read, crop boxes, and poses between
// image and crop coordinates -- each with its host reference twin where it has one.
//
// They replace, on the reference path, flip_pose (phase3_direct/my_HybrIK/utils.py:372-396), the two forward passes of the
// flip test (train_1.py:128-134) and the DataLoader's batch assembly.
#include "frame_crop.h"
#include "pl_internal.h"
#include "pose_augment.h"
#include "pose_table.h"
#include "streaming.h"

namespace pl {
namespace {

// ---- flip_pose (phase3_direct/my_HybrIK/utils.py:372-396) -----------------------------------
// horizontal flip of (B, 17, D) poses: x -> 1-x (D = 2, image-normalised) or -x (D = 3), then
// left joints [4,5,6,11,12,13] <-> right joints [1,2,3,14,15,16]
__global__ void flip_pose_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = (int)(i % D);
  const int64_t bj = i / D;
  const int j = (int)(bj % 17);
  const int64_t b = bj / 17;
  // source joint of destination joint j
  const int src = (j >= 1 && j <= 3) ? j + 3 : (j >= 4 && j <= 6) ? j - 3
                : (j >= 11 && j <= 13) ? j + 3 : (j >= 14 && j <= 16) ? j - 3 : j;
  float v = in[(b * 17 + src) * D + d];
  if (d == 0) v = (D == 2) ? 1.0f - v : -v;
  out[i] = v;
}

// Flip test-time augmentation around ONE forward of 2B rows (eval-mode BatchNorm is row-wise, so the
// two passes the reference makes, train_5 copy.py:160-171 / train_1.py:128-134, are one batch):
//   pack : xx[0:B) = x, xx[B:2B) = flip(x)
//   merge: y = (yy[0:B) + flip(yy[B:2B))) / 2
__device__ __forceinline__ int flip_src_joint(int j) {
  return (j >= 1 && j <= 3) ? j + 3 : (j >= 4 && j <= 6) ? j - 3
       : (j >= 11 && j <= 13) ? j + 3 : (j >= 14 && j <= 16) ? j - 3 : j;
}

__global__ void flip_tta_pack_kernel(const float* __restrict__ x, float* __restrict__ xx, int64_t n, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = (int)(i % D);
  const int64_t bj = i / D;
  const int j = (int)(bj % 17);
  const int64_t b = bj / 17;
  float v = x[(b * 17 + flip_src_joint(j)) * D + d];
  if (d == 0) v = (D == 2) ? 1.0f - v : -v;
  xx[i] = x[i];
  xx[n + i] = v;
}

__global__ void flip_tta_merge_kernel(const float* __restrict__ yy, float* __restrict__ y, int64_t n, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = (int)(i % D);
  const int64_t bj = i / D;
  const int j = (int)(bj % 17);
  const int64_t b = bj / 17;
  float v = yy[n + (b * 17 + flip_src_joint(j)) * D + d];
  if (d == 0) v = (D == 2) ? 1.0f - v : -v;
  y[i] = (v + yy[i]) / 2.0f;
}

// The training-mode Flip branch of the phase5 cycle step (train_5 copy.py:174-199) composes flip_pose with an average:
//   y = (flip_pose(a) + b) / 2, and its backward  da = flip_pose'(g) / 2  (x negated, joints swapped: no 1 - x offset).
// out = (x_offset_if_d0 - / + in[src joint]) [+ addend] ) * scale in ONE pass.
__global__ void flip_pose_ex_kernel(const float* __restrict__ in, const float* __restrict__ addend, float* __restrict__ out,
                                    int64_t n, int D, float x_offset, float scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int d = (int)(i % D);
  const int64_t bj = i / D;
  const int j = (int)(bj % 17);
  const int64_t b = bj / 17;
  float v = in[(b * 17 + flip_src_joint(j)) * D + d];
  if (d == 0) v = x_offset - v;
  if (addend) v += addend[i];
  out[i] = v * scale;
}

// torch.flip(frame, (W,)) of NHWC frames (train_5 copy.py:176 flips the NCHW frame along dim 3 = width): one element per
// thread, writes coalesced, reads reversed in groups of C
__global__ void flip_w_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t n, int W, int C) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (int)(i % C);
  const int64_t p = i / C;
  const int w = (int)(p % W);
  const int64_t row = p / W;
  out[i] = in[(row * W + (W - 1 - w)) * C + c];
}

// ---- batch gather (data.py PoseFeeder): rows idx[0..n) of two resident row-major tables ----------
// oa[i][:] = a[idx[i]][:] (wa floats), ob[i][:] = b[idx[i]][:] (wb floats); one thread per output float
__global__ void gather_rows2_kernel(const float* __restrict__ a, int wa, const float* __restrict__ b, int wb,
                                    const int64_t* __restrict__ idx, int64_t n, float* __restrict__ oa,
                                    float* __restrict__ ob) {
  const int w = wa + wb;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * w) return;
  const int64_t i = t / w;
  const int c = (int)(t - i * w);
  const int64_t r = idx[i];
  if (c < wa) oa[i * wa + c] = a[r * wa + c];
  else ob[i * wb + (c - wa)] = b[r * wb + (c - wa)];
}

// ---- augmented batch gather (data.py PoseFeeder(augment=...), augment_poses): pose_augment.h applied where the row is read ----
// 32 lanes share a pose (two poses per wave, eight per workgroup).  The pose's Philox calls are spread over the group, one
// call per lane: lane 0 turns c2 = 0 into the flip bit, sin / cos and the scale, lane 1 c2 = 1 into the shift, lanes 2..10
// one call each into four noise values; the group then reads them with shuffles of width 32, so no draw, sincosf or logf is
// made twice for a pose.  Output element e = lane, lane + 32, lane + 64 (< 85; the first 34 are a's, the rest b's):
// consecutive lanes store consecutive floats, and load them too unless the pose is flipped (then joints swap inside the
// 340-byte row).  Every stage test is on a kernel argument, the same in all lanes; with all stages off the kernel is
// gather_rows2's copy.  A source index outside [0, table_rows) reads nothing and yields a NaN pose.
// XF (pl_pose_augment_gather_t): every output element goes through its column's transform (pose_table.h apply1) after
// the augmentation, a's 34 columns by (xf.sa, xf.da), b's 51 by (xf.sb, xf.db), either pair nullable.  XF = false is the
// kernel as it was and reads no field of xf.
// CROP (the _crop entry points): the person-centred crop of frame_crop.h in front of the augmentation.  Lane e of a group
// holds elements e and e + 32 of the SOURCE row a (even elements x, odd y), so the extent of the pose is a min / max
// reduction over the lanes of one parity -- xor shuffles of width 32 by 2, 4, 8, 16 -- and one exchange by 1 for the other
// coordinate's; the finiteness of all 34 is an AND over all 32 lanes.  Every lane then holds the same box
// (fc::box_from_extent, the text the frame warp and the host run), crops the source coordinates elem2d reads, and lanes
// 0..3 write boxes[k][4] = (x0, y0, side, side).  A bad source index: NaN box.  CROP = false is the kernel as it was and
// reads no field of crop.
constexpr int PA_LANES = 32;
struct PoseXf {
  const float *sa, *da, *sb, *db;
};
struct PoseCrop {
  fc::Spec spec;
  float* boxes;
};
template <bool XF, bool CROP>
__global__ __launch_bounds__(NTHR) void pose_augment_gather_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const int64_t* __restrict__ src_idx,
                                                                   const int64_t* __restrict__ row_id, int64_t n,
                                                                   int64_t table_rows, float* __restrict__ oa,
                                                                   float* __restrict__ ob, pa::Plan p, PoseXf xf,
                                                                   PoseCrop crop) {
  const int gl = threadIdx.x & (PA_LANES - 1);
  const int64_t k = (int64_t)blockIdx.x * (NTHR / PA_LANES) + (threadIdx.x / PA_LANES);
  if (k >= n) return;                                   // a whole group leaves; no shuffle below crosses a group
  const int64_t src = src_idx ? src_idx[k] : k;
  const uint64_t row = (uint64_t)row_id[k];
  const bool ok = src >= 0 && src < table_rows;
  const float* ar = a + (ok ? src : 0) * pa::kWA;
  const float* br = b + (ok ? src : 0) * pa::kWB;

  const bool any0 = pa::needs_call(p, 0), any1 = pa::needs_call(p, 1), any2 = pa::needs_call(p, 2);
  pa::Pose q = {p.flip_mode == 2, 1.f, 0.f, 1.f, 0.f, 0.f};
  float nz[4] = {0.f, 0.f, 0.f, 0.f};
  if (gl < pa::kCalls && pa::needs_call(p, gl)) {
    uint32_t w[4];
    pa::draw(p, row, gl, w);
    if (gl == 0) pa::decide0(p, w, q);
    else if (gl == 1) pa::decide1(p, w, q);
    else pa::noise4(p, w, nz);
  }
  if (any0) {
    q.flip = __shfl(q.flip, 0, PA_LANES);
    q.cs = __shfl(q.cs, 0, PA_LANES);
    q.sn = __shfl(q.sn, 0, PA_LANES);
    q.sc = __shfl(q.sc, 0, PA_LANES);
  }
  if (any1) {
    q.tx = __shfl(q.tx, 1, PA_LANES);
    q.ty = __shfl(q.ty, 1, PA_LANES);
  }
  float nz_lo = 0.f, nz_hi = 0.f;                       // noise of a's elements gl and gl + 32 (the latter: lanes 0, 1)
  if (any2) {
    const int from = 2 + (gl >> 2);
    const float t0 = __shfl(nz[0], from, PA_LANES), t1 = __shfl(nz[1], from, PA_LANES);
    const float t2 = __shfl(nz[2], from, PA_LANES), t3 = __shfl(nz[3], from, PA_LANES);
    nz_lo = (gl & 2) ? ((gl & 1) ? t3 : t2) : ((gl & 1) ? t1 : t0);
    const float u0 = __shfl(nz[0], 2 + (32 >> 2), PA_LANES), u1 = __shfl(nz[1], 2 + (32 >> 2), PA_LANES);
    nz_hi = (gl & 1) ? u1 : u0;
  }

  const bool rot = p.max_rot != 0.f;
  const float bad = __int_as_float(0x7fc00000);
  fc::Box box = {bad, bad, bad};
  if constexpr (CROP) {
    const float e0 = ar[gl], e1 = gl < pa::kWA - PA_LANES ? ar[gl + PA_LANES] : e0;
    float lo = fminf(e0, e1), hi = fmaxf(e0, e1);
    int fin = fc::finite1(e0) && fc::finite1(e1);
#pragma unroll
    for (int m = 2; m < PA_LANES; m <<= 1) {
      lo = fminf(lo, __shfl_xor(lo, m, PA_LANES));
      hi = fmaxf(hi, __shfl_xor(hi, m, PA_LANES));
    }
#pragma unroll
    for (int m = 1; m < PA_LANES; m <<= 1) fin &= __shfl_xor(fin, m, PA_LANES);
    const float lo2 = __shfl_xor(lo, 1, PA_LANES), hi2 = __shfl_xor(hi, 1, PA_LANES);   // the other coordinate's extent
    const float rx = __shfl(e0, 0, PA_LANES), ry = __shfl(e0, 1, PA_LANES);
    const bool isx = (gl & 1) == 0;
    if (ok) box = fc::box_from_extent(crop.spec, isx ? lo : lo2, isx ? hi : hi2, isx ? lo2 : lo, isx ? hi2 : hi, rx, ry, fin != 0);
    if (gl < 4) crop.boxes[k * 4 + gl] = gl == 0 ? box.x0 : gl == 1 ? box.y0 : box.side;
  }
  float* oar = oa + k * pa::kWA;
  float* obr = ob + k * pa::kWB;
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int e = gl + PA_LANES * it;
    if (e < pa::kWA) {
      const int j = e >> 1, d = e & 1, sj = q.flip ? pa::flip_src_joint(j) : j;
      float v = bad;
      if (ok) {
        float sv = ar[sj * 2 + d], su = rot ? ar[sj * 2 + (d ^ 1)] : 0.f;
        if constexpr (CROP) {
          sv = fc::crop1(crop.spec, box, d, sv);
          if (rot) su = fc::crop1(crop.spec, box, d ^ 1, su);
        }
        v = pa::elem2d(p, q, d, sv, su, it == 0 ? nz_lo : nz_hi);
      }
      if constexpr (XF) {
        if (xf.sa) v = pt::apply1(v, xf.sa[e], xf.da[e]);
      }
      oar[e] = v;
    } else if (e < pa::kRow) {
      const int c = e - pa::kWA, j = c / 3, d = c - 3 * j, sj = q.flip ? pa::flip_src_joint(j) : j;
      float v = bad;
      if (ok) {
        v = br[sj * 3 + d];
        if (d != 2) v = pa::elem3d(p, q, d, v, rot ? br[sj * 3 + (d ^ 1)] : 0.f);
      }
      if constexpr (XF) {
        if (xf.sb) v = pt::apply1(v, xf.sb[c], xf.db[c]);
      }
      obr[c] = v;
    }
  }
}

// ---- the per-pose joint weights of a batch (data.py PoseFeeder(weights=), gather_row_weights): the weights follow the joints ----
// out[k][j] = w[s][flipped_k ? flip_src_joint(j) : j].  p is the batch's plan with every stage but the flip switched off, so
// decide0 -- the function the pose gather's lane 0 runs on the same words -- returns the flip bit and nothing else is
// computed.  One thread per output float, one draw per pose and wavefront (shared by a shuffle); rw_flipped and rw_elem are
// written once for the kernel and the host entry point.
PLA_HD bool rw_flipped(const pa::Plan& p, uint64_t row) {
  pa::Pose q = {p.flip_mode == 2, 1.f, 0.f, 1.f, 0.f, 0.f};
  if (pa::needs_call(p, 0)) {
    uint32_t w[4];
    pa::draw(p, row, 0, w);
    pa::decide0(p, w, q);
  }
  return q.flip != 0;
}
PLA_HD float rw_elem(const float* w, int64_t s, int J, int j, bool flipped) {
  return w[s * J + (flipped ? pa::flip_src_joint(j) : j)];
}
__global__ __launch_bounds__(NTHR) void row_weights_gather_kernel(const float* __restrict__ w, const int64_t* __restrict__ src_idx,
                                                                  const int64_t* __restrict__ row_id, int64_t n,
                                                                  int64_t table_rows, int J, float* __restrict__ out,
                                                                  pa::Plan p) {
  const int64_t t = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  const bool in = t < n * J;                            // (nobody leaves before the shuffle)
  const int64_t k = in ? t / J : 0;
  const int j = (int)(t - k * J);
  bool flipped = p.flip_mode == 2;
  if (p.flip_mode == 1) {                               // a kernel argument: the same in every lane
    // one draw per pose and wavefront: the pose's first element inside the wavefront makes it, the others read it
    const int64_t wave0 = t - (threadIdx.x & (warpSize - 1));
    const int64_t first = k * J > wave0 ? k * J : wave0;
    int f = 0;
    if (in && t == first) f = rw_flipped(p, (uint64_t)row_id[k]);
    flipped = __shfl(f, (int)(first - wave0)) != 0;
  }
  if (!in) return;
  const int64_t s = src_idx ? src_idx[k] : k;
  float v = __int_as_float(0x7fc00000);
  if (s >= 0 && s < table_rows) v = rw_elem(w, s, J, j, flipped);
  out[t] = v;
}

// the checks both entry points share; on success *plan holds the flip and nothing else
bool pa_overlap(const float* x, int64_t nx, const float* y, int64_t ny);
int row_weights_args(const char* fn, const float* w, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                     int64_t table_rows, int64_t J, float* out, const PLPoseAug* aug, uint64_t epoch, pa::Plan* plan) {
  if (!w || !out) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (n <= 0 || table_rows <= 0 || J < 1 || J > 4096 || n > (int64_t)INT32_MAX * NTHR / J || table_rows > INT64_MAX / (4 * J))
    PL_FAIL(PL_ESHAPE, "%s: n=%lld rows=%lld J=%lld", fn, (long long)n, (long long)table_rows, (long long)J);
  if (!src_idx && n > table_rows)
    PL_FAIL(PL_ESHAPE, "%s: n=%lld exceeds the %lld rows of an ungathered batch", fn, (long long)n, (long long)table_rows);
  if (pa_overlap(out, n * J, w, table_rows * J)) PL_FAIL(PL_EINVAL, "%s: aliased pointers (out overlaps the table)", fn);
  PLPoseAug off = {};
  PL_TRY(pose_aug_plan(fn, aug ? aug : &off, epoch, plan));
  plan->max_rot = plan->scale_range = plan->max_shift = plan->sigma = 0.f;
  if (plan->flip_mode != 0 && J != 17) PL_FAIL(PL_ESHAPE, "%s: a flip swaps the left and right of 17 joints, J=%lld", fn, (long long)J);
  if (plan->flip_mode == 1 && !row_id) PL_FAIL(PL_EINVAL, "%s: null pointer (row_id)", fn);
  return PL_OK;
}

// ---- crop boxes and poses between image and crop coordinates (data.py crop_boxes, crop_poses, uncrop_poses): frame_crop.h ----
// one thread per pose: its 34 floats, fc::box_of_pose, boxes[k][4] = (x0, y0, side, side)
__global__ __launch_bounds__(NTHR) void pose_crop_boxes_kernel(const float* __restrict__ a, int64_t n, fc::Spec c,
                                                               float* __restrict__ boxes) {
  const int64_t k = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (k >= n) return;
  const fc::Box b = fc::box_of_pose(c, a + k * pa::kWA);
  float* o = boxes + k * 4;
  o[0] = b.x0; o[1] = b.y0; o[2] = b.side; o[3] = b.side;
}

// one thread per coordinate of p [n][17][2] with boxes [n][4].  INV = false: image-normalised -> crop-normalised (fc::crop1);
// INV = true: back (fc::uncrop1).  offset = 0 drops x0 / y0: both maps are affine per element, so the backward pass of
// either is the same instantiation with offset = 0 on the incoming gradient.
template <bool INV>
__global__ __launch_bounds__(NTHR) void crop_poses_kernel(const float* __restrict__ p, const float* __restrict__ boxes,
                                                          int64_t total, fc::Spec c, int offset, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i >= total) return;
  const float* bx = boxes + (i / pa::kWA) * 4;
  const fc::Box b = {bx[0], bx[1], bx[2]};
  const int d = (int)(i & 1);
  out[i] = INV ? fc::uncrop1(c, b, d, p[i], offset != 0) : fc::crop1(c, b, d, p[i], offset != 0);
}

// Argument checks shared by pl_pose_augment_gather and pl_pose_augment_host; on success *plan is what the transform reads.
// pose_aug_plan is the part about the PLPoseAug itself, which the frame warp (frame_warp.hip) reads too.
bool pa_overlap(const float* x, int64_t nx, const float* y, int64_t ny) {
  const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)nx * sizeof(float);
  const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)ny * sizeof(float);
  return x0 < y1 && y0 < x1;
}
int pose_augment_args(const char* fn, const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                      int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                      pa::Plan* plan) {
  if (!a || !b || !row_id || !oa || !ob || !aug) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (n <= 0 || table_rows <= 0 || n > (int64_t)INT32_MAX * (NTHR / PA_LANES) || table_rows > INT64_MAX / (4 * pa::kRow))
    PL_FAIL(PL_ESHAPE, "%s: n=%lld rows=%lld", fn, (long long)n, (long long)table_rows);
  if (!src_idx && n > table_rows)
    PL_FAIL(PL_ESHAPE, "%s: n=%lld exceeds the %lld rows of an ungathered batch", fn, (long long)n, (long long)table_rows);
  if (pa_overlap(oa, n * pa::kWA, ob, n * pa::kWB) || pa_overlap(oa, n * pa::kWA, a, table_rows * pa::kWA) ||
      pa_overlap(oa, n * pa::kWA, b, table_rows * pa::kWB) || pa_overlap(ob, n * pa::kWB, a, table_rows * pa::kWA) ||
      pa_overlap(ob, n * pa::kWB, b, table_rows * pa::kWB))
    PL_FAIL(PL_EINVAL, "%s: aliased pointers (the outputs overlap each other or a source)", fn);
  return pose_aug_plan(fn, aug, epoch, plan);
}

int pose_crop_args(const char* fn, const PLPoseCrop* crop, const PLPoseAug* aug, const float* a, int64_t table_rows,
                   const float* oa, const float* ob, int64_t n, float* boxes, PoseCrop* pc) {
  pc->boxes = nullptr;
  if (!crop) return PL_OK;
  if (!boxes) PL_FAIL(PL_EINVAL, "%s: null pointer (boxes)", fn);
  if (!aug) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  PL_TRY(crop_spec(fn, crop, aug, &pc->spec));
  if (pa_overlap(boxes, n * 4, oa, n * pa::kWA) || pa_overlap(boxes, n * 4, ob, n * pa::kWB) ||
      pa_overlap(boxes, n * 4, a, table_rows * pa::kWA))
    PL_FAIL(PL_EINVAL, "%s: aliased pointers (boxes overlaps an output or the source)", fn);
  pc->boxes = boxes;
  return PL_OK;
}

// pose_augment_gather_kernel's only launch site; no transform and no crop at all: the plain instantiation
int launch_pose_augment(const char* fn, const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                        int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                        const PoseXf& xf, const PLPoseCrop* crop, float* boxes, void* stream) {
  pa::Plan plan;
  PoseCrop pc = {};
  PL_TRY(pose_augment_args(fn, a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch, &plan));
  PL_TRY(pose_crop_args(fn, crop, aug, a, table_rows, oa, ob, n, boxes, &pc));
  constexpr int per = NTHR / PA_LANES;
  const dim3 grid((unsigned)((n + per - 1) / per));
  const bool t = xf.sa || xf.sb;
  auto kernel = pc.boxes ? (t ? pose_augment_gather_kernel<true, true> : pose_augment_gather_kernel<false, true>)
                         : (t ? pose_augment_gather_kernel<true, false> : pose_augment_gather_kernel<false, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(NTHR), 0, (hipStream_t)stream, a, b, src_idx, row_id, n, table_rows, oa, ob, plan, xf,
                     pc);
  PL_CHECK_LAUNCH("pose_augment_gather");
  return PL_OK;
}

int pose_xf_args(const char* fn, const float* sub_a, const float* div_a, const float* sub_b, const float* div_b) {
  if ((sub_a != nullptr) != (div_a != nullptr) || (sub_b != nullptr) != (div_b != nullptr))
    PL_FAIL(PL_EINVAL, "%s: a transform is a (sub, div) pair", fn);
  return PL_OK;
}

// the host reference of launch_pose_augment, pose by pose: pa:: / fc::augment_pose, then the columns' transform.  fn: the
// name argument errors are reported under
int pose_augment_host(const char* fn, const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                      int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                      const PoseXf& xf, const PLPoseCrop* crop, float* boxes) {
  pa::Plan plan;
  PoseCrop pc = {};
  PL_TRY(pose_augment_args(fn, a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch, &plan));
  PL_TRY(pose_crop_args(fn, crop, aug, a, table_rows, oa, ob, n, boxes, &pc));
  for (int64_t k = 0; k < n; ++k) {
    const int64_t src = src_idx ? src_idx[k] : k;
    if (src < 0 || src >= table_rows)
      PL_FAIL(PL_EINVAL, "%s: src_idx[%lld]=%lld is outside the table", fn, (long long)k, (long long)src);
  }
  for (int64_t k = 0; k < n; ++k) {
    const int64_t src = src_idx ? src_idx[k] : k;
    const float *ar = a + src * pa::kWA, *br = b + src * pa::kWB;
    float *oar = oa + k * pa::kWA, *obr = ob + k * pa::kWB;
    if (pc.boxes) {
      fc::Box box;
      fc::augment_pose(pc.spec, plan, (uint64_t)row_id[k], ar, br, oar, obr, &box);
      float* o = boxes + k * 4;
      o[0] = box.x0; o[1] = box.y0; o[2] = box.side; o[3] = box.side;
    } else {
      pa::augment_pose(plan, (uint64_t)row_id[k], ar, br, oar, obr);
    }
    for (int e = 0; xf.sa && e < pa::kWA; ++e) oar[e] = pt::apply1(oar[e], xf.sa[e], xf.da[e]);
    for (int e = 0; xf.sb && e < pa::kWB; ++e) obr[e] = pt::apply1(obr[e], xf.sb[e], xf.db[e]);
  }
  return PL_OK;
}

int crop_boxes_args(const char* fn, const float* x2d, int64_t n, const PLPoseCrop* crop, float* boxes, fc::Spec* spec) {
  if (!x2d || !boxes || !crop) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (n <= 0 || n > (int64_t)INT32_MAX * NTHR / pa::kWA) PL_FAIL(PL_ESHAPE, "%s: n=%lld", fn, (long long)n);
  if (pa_overlap(boxes, n * 4, x2d, n * pa::kWA)) PL_FAIL(PL_EINVAL, "%s: aliased pointers (boxes overlaps the poses)", fn);
  return crop_spec(fn, crop, nullptr, spec);
}

int crop_poses_args(const char* fn, const float* p, const float* boxes, int64_t n, int64_t Hs, int64_t Ws, float* out,
                    fc::Spec* spec) {
  if (!p || !boxes || !out) PL_FAIL(PL_EINVAL, "%s: null pointer", fn);
  if (n <= 0 || n > (int64_t)INT32_MAX * NTHR / pa::kWA) PL_FAIL(PL_ESHAPE, "%s: n=%lld", fn, (long long)n);
  if (Hs <= 0 || Ws <= 0 || Hs > (1 << 22) || Ws > (1 << 22))
    PL_FAIL(PL_ESHAPE, "%s: frame size Hs=%lld Ws=%lld", fn, (long long)Hs, (long long)Ws);
  if (pa_overlap(out, n * pa::kWA, boxes, n * 4) || pa_overlap(out, n * pa::kWA, p, n * pa::kWA))
    PL_FAIL(PL_EINVAL, "%s: aliased pointers (out overlaps boxes or p)", fn);
  *spec = fc::Spec{1.f, 1.f, (float)Hs, (float)Ws, 0};
  return PL_OK;
}

}  // namespace

int pose_aug_plan(const char* fn, const PLPoseAug* aug, uint64_t epoch, pa::Plan* plan) {
  const struct { const char* name; float v; bool nonneg; } par[] = {
      {"p_flip", aug->p_flip, true},         {"flip_offset", aug->flip_offset, false},   {"max_rot", aug->max_rot, true},
      {"scale_range", aug->scale_range, true}, {"max_shift", aug->max_shift, true},      {"jitter_sigma", aug->jitter_sigma, true},
      {"cx", aug->cx, false},                {"cy", aug->cy, false}};
  for (const auto& q : par) {
    if (!(fabsf(q.v) <= 3.402823466e38f)) PL_FAIL(PL_EINVAL, "%s: %s is not finite", fn, q.name);
    if (q.nonneg && q.v < 0.f) PL_FAIL(PL_EINVAL, "%s: %s=%g is negative", fn, q.name, (double)q.v);
  }
  if (aug->scale_range >= 1.f) PL_FAIL(PL_EINVAL, "%s: scale_range=%g must be below 1", fn, (double)aug->scale_range);
  *plan = pa::plan_of(aug->p_flip, dropout_threshold(aug->p_flip), aug->flip_offset, aug->max_rot, aug->scale_range,
                      aug->max_shift, aug->jitter_sigma, aug->cx, aug->cy, aug->seed, epoch);
  return PL_OK;
}

// The checks of a PLPoseCrop (fn: the entry point named in the message) and the spec frame_crop.h reads; the frame warp
// (frame_warp.hip) reads it too.  A crop's flip mirrors about the crop's centre, so it carries the frame warp's flip check.
int crop_spec(const char* fn, const PLPoseCrop* c, const PLPoseAug* aug, fc::Spec* spec) {
  if (!(fabsf(c->margin) <= 3.402823466e38f) || c->margin <= 0.f)
    PL_FAIL(PL_EINVAL, "%s: crop margin=%g must be finite and > 0", fn, (double)c->margin);
  if (!(c->min_side >= 1.f) || c->min_side > fc::kMaxSide || c->min_side != floorf(c->min_side))
    PL_FAIL(PL_EINVAL, "%s: crop min_side=%g must be an integer in [1, 2^20]", fn, (double)c->min_side);
  if (c->centre != PL_CROP_BBOX && c->centre != PL_CROP_ROOT) PL_FAIL(PL_EINVAL, "%s: crop centre=%d", fn, (int)c->centre);
  if (c->Hs <= 0 || c->Ws <= 0 || c->Hs > (1 << 22) || c->Ws > (1 << 22))
    PL_FAIL(PL_ESHAPE, "%s: crop frame size Hs=%lld Ws=%lld", fn, (long long)c->Hs, (long long)c->Ws);
  if (aug && aug->p_flip > 0.f && aug->flip_offset != 1.f)
    PL_FAIL(PL_EINVAL, "%s: flip_offset=%g: a flip of a cropped pose mirrors about the crop's centre (flip_offset 1)", fn,
            (double)aug->flip_offset);
  *spec = fc::Spec{c->margin, c->min_side, (float)c->Hs, (float)c->Ws, c->centre == PL_CROP_ROOT};
  return PL_OK;
}

}  // namespace pl

extern "C" int pl_flip_pose(const float* in, float* out, int64_t B, int64_t joints, int64_t D, void* stream) {
  if (!in || !out || in == out) PL_FAIL(PL_EINVAL, "pl_flip_pose: null or aliased pointers");
  if (B <= 0 || joints != 17 || (D != 2 && D != 3)) PL_FAIL(PL_ESHAPE, "pl_flip_pose: expects (B, 17, 2|3)");
  const int64_t n = B * joints * D;
  hipLaunchKernelGGL(pl::flip_pose_kernel, dim3((unsigned)((n + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0, (hipStream_t)stream,
                     in, out, n, (int)D);
  PL_CHECK_LAUNCH("flip_pose");
  return PL_OK;
}

extern "C" int pl_flip_tta_pack(const float* x, float* xx, int64_t B, int64_t joints, int64_t D, void* stream) {
  if (!x || !xx) PL_FAIL(PL_EINVAL, "pl_flip_tta_pack: null pointer");
  if (B <= 0 || joints != 17 || (D != 2 && D != 3)) PL_FAIL(PL_ESHAPE, "pl_flip_tta_pack: expects (B, 17, 2|3)");
  const int64_t n = B * joints * D;
  hipLaunchKernelGGL(pl::flip_tta_pack_kernel, dim3((unsigned)((n + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0,
                     (hipStream_t)stream, x, xx, n, (int)D);
  PL_CHECK_LAUNCH("flip_tta_pack");
  return PL_OK;
}

extern "C" int pl_flip_tta_merge(const float* yy, float* y, int64_t B, int64_t joints, int64_t D, void* stream) {
  if (!yy || !y) PL_FAIL(PL_EINVAL, "pl_flip_tta_merge: null pointer");
  if (B <= 0 || joints != 17 || (D != 2 && D != 3)) PL_FAIL(PL_ESHAPE, "pl_flip_tta_merge: expects (B, 17, 2|3)");
  const int64_t n = B * joints * D;
  hipLaunchKernelGGL(pl::flip_tta_merge_kernel, dim3((unsigned)((n + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0,
                     (hipStream_t)stream, yy, y, n, (int)D);
  PL_CHECK_LAUNCH("flip_tta_merge");
  return PL_OK;
}

extern "C" int pl_flip_pose_ex(const float* in, const float* addend, float* out, int64_t B, int64_t joints, int64_t D,
                               float x_offset, float scale, void* stream) {
  if (!in || !out || in == out || addend == out) PL_FAIL(PL_EINVAL, "pl_flip_pose_ex: null or aliased pointers");
  if (B <= 0 || joints != 17 || (D != 2 && D != 3)) PL_FAIL(PL_ESHAPE, "pl_flip_pose_ex: expects (B, 17, 2|3)");
  const int64_t n = B * joints * D;
  hipLaunchKernelGGL(pl::flip_pose_ex_kernel, dim3((unsigned)((n + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0, (hipStream_t)stream,
                     in, addend, out, n, (int)D, x_offset, scale);
  PL_CHECK_LAUNCH("flip_pose_ex");
  return PL_OK;
}

extern "C" int pl_flip_w_nhwc(const float* in, float* out, int64_t B, int64_t H, int64_t W, int64_t C, void* stream) {
  if (!in || !out || in == out) PL_FAIL(PL_EINVAL, "pl_flip_w_nhwc: null or aliased pointers");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || W > (1 << 30) || C > (1 << 30)) PL_FAIL(PL_ESHAPE, "pl_flip_w_nhwc: bad shape");
  const int64_t n = B * H * W * C;
  if ((n + pl::NTHR - 1) / pl::NTHR > 0x7fffffffLL) PL_FAIL(PL_ESHAPE, "pl_flip_w_nhwc: tensor too large");
  hipLaunchKernelGGL(pl::flip_w_nhwc_kernel, dim3((unsigned)((n + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0, (hipStream_t)stream,
                     in, out, n, (int)W, (int)C);
  PL_CHECK_LAUNCH("flip_w_nhwc");
  return PL_OK;
}

extern "C" int pl_gather_rows2(const float* a, int64_t wa, const float* b, int64_t wb, const int64_t* idx,
                               int64_t n, int64_t table_rows, float* oa, float* ob, void* stream) {
  if (!a || !b || !idx || !oa || !ob) PL_FAIL(PL_EINVAL, "pl_gather_rows2: null pointer");
  if (n <= 0 || wa <= 0 || wb <= 0 || wa + wb > 4096 || table_rows <= 0)
    PL_FAIL(PL_ESHAPE, "pl_gather_rows2: n=%lld wa=%lld wb=%lld rows=%lld", (long long)n, (long long)wa,
            (long long)wb, (long long)table_rows);
  const int64_t total = n * (wa + wb);
  if (total > (int64_t)INT32_MAX * pl::NTHR) PL_FAIL(PL_ESHAPE, "pl_gather_rows2: batch too large");
  hipLaunchKernelGGL(pl::gather_rows2_kernel, dim3((unsigned)((total + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0,
                     (hipStream_t)stream, a, (int)wa, b, (int)wb, idx, n, oa, ob);
  PL_CHECK_LAUNCH("gather_rows2");
  return PL_OK;
}

extern "C" int pl_pose_augment_gather(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                                      int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug,
                                      uint64_t epoch, void* stream) {
  return pl::launch_pose_augment("pl_pose_augment_gather", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                             pl::PoseXf{nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr, stream);
}

extern "C" int pl_row_weights_gather(const float* w, const int64_t* src_idx, const int64_t* row_id, int64_t n, int64_t table_rows,
                                     int64_t J, float* out, const PLPoseAug* aug, uint64_t epoch, void* stream) {
  pl::pa::Plan plan;
  PL_TRY(pl::row_weights_args("pl_row_weights_gather", w, src_idx, row_id, n, table_rows, J, out, aug, epoch, &plan));
  const int64_t total = n * J;
  hipLaunchKernelGGL(pl::row_weights_gather_kernel, dim3((unsigned)((total + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0,
                     (hipStream_t)stream, w, src_idx, row_id, n, table_rows, (int)J, out, plan);
  PL_CHECK_LAUNCH("row_weights_gather");
  return PL_OK;
}

extern "C" int pl_row_weights_gather_host(const float* w, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                                          int64_t table_rows, int64_t J, float* out, const PLPoseAug* aug, uint64_t epoch) {
  pl::pa::Plan plan;
  PL_TRY(pl::row_weights_args("pl_row_weights_gather_host", w, src_idx, row_id, n, table_rows, J, out, aug, epoch, &plan));
  for (int64_t k = 0; k < n; ++k) {
    const int64_t s = src_idx ? src_idx[k] : k;
    if (s < 0 || s >= table_rows)
      PL_FAIL(PL_EINVAL, "pl_row_weights_gather_host: src_idx[%lld]=%lld is outside the table", (long long)k, (long long)s);
  }
  for (int64_t k = 0; k < n; ++k) {
    const bool flipped = pl::rw_flipped(plan, plan.flip_mode == 1 ? (uint64_t)row_id[k] : 0);
    for (int j = 0; j < (int)J; ++j) out[k * J + j] = pl::rw_elem(w, src_idx ? src_idx[k] : k, (int)J, j, flipped);
  }
  return PL_OK;
}

extern "C" int pl_pose_augment_gather_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                                        int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug,
                                        uint64_t epoch, const float* sub_a, const float* div_a, const float* sub_b,
                                        const float* div_b, void* stream) {
  PL_TRY(pl::pose_xf_args("pl_pose_augment_gather_t", sub_a, div_a, sub_b, div_b));
  return pl::launch_pose_augment("pl_pose_augment_gather_t", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                             pl::PoseXf{sub_a, div_a, sub_b, div_b}, nullptr, nullptr, stream);
}

extern "C" int pl_pose_augment_host(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                                    int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch) {
  return pl::pose_augment_host("pl_pose_augment_host", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                           pl::PoseXf{nullptr, nullptr, nullptr, nullptr}, nullptr, nullptr);
}

// (argument errors behind the transform's own are reported under pl_pose_augment_host's name, as they always were)
extern "C" int pl_pose_augment_host_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id, int64_t n,
                                      int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug, uint64_t epoch,
                                      const float* sub_a, const float* div_a, const float* sub_b, const float* div_b) {
  PL_TRY(pl::pose_xf_args("pl_pose_augment_host_t", sub_a, div_a, sub_b, div_b));
  return pl::pose_augment_host("pl_pose_augment_host", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                           pl::PoseXf{sub_a, div_a, sub_b, div_b}, nullptr, nullptr);
}

extern "C" int pl_pose_augment_gather_crop(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                                           int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug,
                                           uint64_t epoch, const PLPoseCrop* crop, float* boxes, void* stream) {
  return pl::launch_pose_augment("pl_pose_augment_gather_crop", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                             pl::PoseXf{nullptr, nullptr, nullptr, nullptr}, crop, boxes, stream);
}

extern "C" int pl_pose_augment_gather_crop_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                                             int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug,
                                             uint64_t epoch, const float* sub_a, const float* div_a, const float* sub_b,
                                             const float* div_b, const PLPoseCrop* crop, float* boxes, void* stream) {
  PL_TRY(pl::pose_xf_args("pl_pose_augment_gather_crop_t", sub_a, div_a, sub_b, div_b));
  return pl::launch_pose_augment("pl_pose_augment_gather_crop_t", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                             pl::PoseXf{sub_a, div_a, sub_b, div_b}, crop, boxes, stream);
}

extern "C" int pl_pose_augment_host_crop(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                                         int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug,
                                         uint64_t epoch, const PLPoseCrop* crop, float* boxes) {
  return pl::pose_augment_host("pl_pose_augment_host_crop", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                           pl::PoseXf{nullptr, nullptr, nullptr, nullptr}, crop, boxes);
}

extern "C" int pl_pose_augment_host_crop_t(const float* a, const float* b, const int64_t* src_idx, const int64_t* row_id,
                                           int64_t n, int64_t table_rows, float* oa, float* ob, const PLPoseAug* aug,
                                           uint64_t epoch, const float* sub_a, const float* div_a, const float* sub_b,
                                           const float* div_b, const PLPoseCrop* crop, float* boxes) {
  PL_TRY(pl::pose_xf_args("pl_pose_augment_host_crop_t", sub_a, div_a, sub_b, div_b));
  return pl::pose_augment_host("pl_pose_augment_host_crop_t", a, b, src_idx, row_id, n, table_rows, oa, ob, aug, epoch,
                           pl::PoseXf{sub_a, div_a, sub_b, div_b}, crop, boxes);
}

extern "C" int pl_pose_crop_boxes(const float* x2d, int64_t n, const PLPoseCrop* crop, float* boxes, void* stream) {
  pl::fc::Spec spec;
  PL_TRY(pl::crop_boxes_args("pl_pose_crop_boxes", x2d, n, crop, boxes, &spec));
  hipLaunchKernelGGL(pl::pose_crop_boxes_kernel, dim3((unsigned)((n + pl::NTHR - 1) / pl::NTHR)), dim3(pl::NTHR), 0, (hipStream_t)stream, x2d,
                     n, spec, boxes);
  PL_CHECK_LAUNCH("pose_crop_boxes");
  return PL_OK;
}

extern "C" int pl_pose_crop_boxes_host(const float* x2d, int64_t n, const PLPoseCrop* crop, float* boxes) {
  pl::fc::Spec spec;
  PL_TRY(pl::crop_boxes_args("pl_pose_crop_boxes_host", x2d, n, crop, boxes, &spec));
  for (int64_t k = 0; k < n; ++k) {
    const pl::fc::Box b = pl::fc::box_of_pose(spec, x2d + k * pl::pa::kWA);
    float* o = boxes + k * 4;
    o[0] = b.x0; o[1] = b.y0; o[2] = b.side; o[3] = b.side;
  }
  return PL_OK;
}

extern "C" int pl_crop_poses(const float* p, const float* boxes, int64_t n, int64_t Hs, int64_t Ws, int invert, int offset,
                             float* out, void* stream) {
  pl::fc::Spec spec;
  PL_TRY(pl::crop_poses_args("pl_crop_poses", p, boxes, n, Hs, Ws, out, &spec));
  const int64_t total = n * pl::pa::kWA;
  const dim3 grid((unsigned)((total + pl::NTHR - 1) / pl::NTHR));
  auto kernel = invert ? pl::crop_poses_kernel<true> : pl::crop_poses_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(pl::NTHR), 0, (hipStream_t)stream, p, boxes, total, spec, offset, out);
  PL_CHECK_LAUNCH("crop_poses");
  return PL_OK;
}

extern "C" int pl_crop_poses_host(const float* p, const float* boxes, int64_t n, int64_t Hs, int64_t Ws, int invert, int offset,
                                  float* out) {
  pl::fc::Spec spec;
  PL_TRY(pl::crop_poses_args("pl_crop_poses_host", p, boxes, n, Hs, Ws, out, &spec));
  for (int64_t i = 0; i < n * pl::pa::kWA; ++i) {
    const float* bx = boxes + (i / pl::pa::kWA) * 4;
    const pl::fc::Box b = {bx[0], bx[1], bx[2]};
    const int d = (int)(i & 1);
    out[i] = invert ? pl::fc::uncrop1(spec, b, d, p[i], offset != 0) : pl::fc::crop1(spec, b, d, p[i], offset != 0);
  }
  return PL_OK;
}

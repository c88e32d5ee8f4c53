// Pose tables: what makes one from raw joint arrays (joint pick, camera view, root-centring), its per-column statistics,
// and the per-column transform (standardise / normalise and the way back), written once for the device kernels and the
// host entry points: pl_pose_prepare / pl_pose_stats / pl_pose_affine and their _host forms run this text, and so do the
// transform stages of pl_pose_augment_gather_t, pl_pose_errors_t and pl_mpjpe_accum_t.
// The reference does this per frame and per joint in Python (phase3_direct/my_HybrIK/H36_dataset.py:303-379 read_data:
// 17 of 32 joints, `tmp - translation/1000`, qv_mult; :205-300 process_data: root-centre, mean / std / min / max of the
// training set, standardise or normalise) and undoes it before it measures (phase1_lifting/main.py:473-474).
//
// Prepare, raw [N][Jsrc][D] -> out [N][J][D], stages in the reference's order, a stage that is off not run at all:
//   pick     out[n][j] = raw[n][pick[j]]
//   camera   (D = 3)  v = q (0, (double)p - t) q*, camera row (t0, t1, t2, w, x, y, z) of cam[cam_id[n]], both Hamilton
//            products term by term in utils.py:328-335's order, in fp64, rounded to fp32 once.  A cam_id outside [0, C)
//            reads no camera: every element of the row is NaN.
//   centre   joints 1..J-1 minus joint 0 in fp32; joint 0 becomes +0 (H36_dataset.py:209-211, 288-289)
//
// Statistics of the W = J D columns over N rows, fp64 throughout: mean = sum / N, std = sqrt(sum (x - mean)^2 / N), min, max.
// Order of every sum, a function of (N, W) alone: rows go in chunks of kChunkRows; inside a chunk, H = kStatThreads / W
// sub-sums, sub-sum h taking rows h, h + H, h + 2 H ... of the chunk in order; a chunk's value is the sub-sums added in
// order h = 0 .. H-1; a column's value the chunks added in order.  No atomics.  min / max carry a NaN (min_nan / max_nan),
// so a NaN in a column makes all four of its values NaN.  A column whose min == max gets mean = that value exactly, and
// hence std = +0.
//
// Transform, per column (sub, div) in fp32:  apply  y = (x - sub) / div  (a correctly rounded division),  invert
// x = y div + sub (two roundings).  A column with div == 0 applies to 0 and inverts to sub.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLT_HD __host__ __device__ inline
#else
#define PLT_HD inline
#endif

namespace pl {
namespace pt {

constexpr int kMaxSrcJoints = 64, kMaxJoints = 32, kMaxCols = 96;
constexpr int kChunkRows = 1024;      // rows of a first-stage workgroup
constexpr int kStatThreads = 256;     // its threads: H = kStatThreads / W row phases of W columns each

// what a prepare pass reads besides the tables; built on the host, passed by value
struct Prepare {
  int jsrc, j, d;
  int has_pick, has_cam, centre;
  int n_cam;
  uint8_t pick[kMaxJoints];
};

PLT_HD float nan_f() {
  union { uint32_t u; float f; } c;
  c.u = 0x7fc00000u;
  return c.f;
}

// q (0, p - t) q* with cam = (t0, t1, t2, w, x, y, z); utils.py:328-340 with q2 = (0, v) and q_conjugate(q1) spelled out
PLT_HD void camera_view(const double* cam, const float p[3], float out[3]) {
#pragma clang fp contract(off)
  const double w1 = cam[3], x1 = cam[4], y1 = cam[5], z1 = cam[6];
  const double w2 = 0.0, x2 = (double)p[0] - cam[0], y2 = (double)p[1] - cam[1], z2 = (double)p[2] - cam[2];
  const double w = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
  const double x = w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2;
  const double y = w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2;
  const double z = w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2;
  const double w3 = w1, x3 = -x1, y3 = -y1, z3 = -z1;
  const double ox = w * x3 + x * w3 + y * z3 - z * y3;
  const double oy = w * y3 + y * w3 + z * x3 - x * z3;
  const double oz = w * z3 + z * w3 + x * y3 - y * x3;
  out[0] = (float)ox; out[1] = (float)oy; out[2] = (float)oz;
}

// joint j of row n before root-centring: the pick and the camera view.  cam = the row's camera or nullptr
PLT_HD void picked_joint(const Prepare& a, const float* raw_row, const double* cam, int j, float v[3]) {
  const float* s = raw_row + (a.has_pick ? (int)a.pick[j] : j) * a.d;
  for (int d = 0; d < a.d; ++d) v[d] = s[d];
  if (cam) camera_view(cam, v, v);
}

// output joint j of one row; o [D].  cam_id is read only when the camera view is on
PLT_HD void prepare_joint(const Prepare& a, const float* raw_row, const double* cams, int32_t cam_id, int j, float* o) {
#pragma clang fp contract(off)
  const double* cam = nullptr;
  if (a.has_cam) {
    if (cam_id < 0 || cam_id >= a.n_cam) {
      for (int d = 0; d < a.d; ++d) o[d] = nan_f();
      return;
    }
    cam = cams + (int64_t)cam_id * 7;
  }
  float v[3];
  if (a.centre && j == 0) {
    for (int d = 0; d < a.d; ++d) o[d] = 0.f;
    return;
  }
  picked_joint(a, raw_row, cam, j, v);
  if (a.centre) {
    float r[3];
    picked_joint(a, raw_row, cam, 0, r);
    for (int d = 0; d < a.d; ++d) v[d] = v[d] - r[d];
  }
  for (int d = 0; d < a.d; ++d) o[d] = v[d];
}

// ---- statistics ----------------------------------------------------------------------------------------------------------
PLT_HD double min_nan(double a, double b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
PLT_HD double max_nan(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
PLT_HD int stat_phases(int W) { return kStatThreads / W; }

// sub-sum h of a chunk, first pass: rows r0 + h, r0 + h + H, ... < r1 of column c -> (sum, min, max).  kStatLoads rows
// are loaded before they are added, in the same order: the loop waits on memory, not on its own additions.
constexpr int kStatLoads = 8;
PLT_HD void phase_sum(const float* x, int64_t r0, int64_t r1, int W, int H, int h, int c, double* s, double* lo, double* hi) {
  double acc = 0.0, mn = INFINITY, mx = -INFINITY;
  int64_t r = r0 + h;
  for (; r + (int64_t)(kStatLoads - 1) * H < r1; r += (int64_t)kStatLoads * H) {
    float v[kStatLoads];
#pragma unroll
    for (int u = 0; u < kStatLoads; ++u) v[u] = x[(r + (int64_t)u * H) * W + c];
#pragma unroll
    for (int u = 0; u < kStatLoads; ++u) {
      acc += (double)v[u];
      mn = min_nan(mn, (double)v[u]);
      mx = max_nan(mx, (double)v[u]);
    }
  }
  for (; r < r1; r += H) {
    const double v = (double)x[r * W + c];
    acc += v;
    mn = min_nan(mn, v);
    mx = max_nan(mx, v);
  }
  *s = acc; *lo = mn; *hi = mx;
}

// second pass: the squared deviations from the column's mean
PLT_HD double phase_sq(const float* x, int64_t r0, int64_t r1, int W, int H, int h, int c, double mean) {
#pragma clang fp contract(off)
  double acc = 0.0;
  int64_t r = r0 + h;
  for (; r + (int64_t)(kStatLoads - 1) * H < r1; r += (int64_t)kStatLoads * H) {
    float v[kStatLoads];
#pragma unroll
    for (int u = 0; u < kStatLoads; ++u) v[u] = x[(r + (int64_t)u * H) * W + c];
#pragma unroll
    for (int u = 0; u < kStatLoads; ++u) {
      const double dv = (double)v[u] - mean;
      const double sq = dv * dv;
      acc += sq;
    }
  }
  for (; r < r1; r += H) {
    const double dv = (double)x[r * W + c] - mean;
    const double sq = dv * dv;
    acc += sq;
  }
  return acc;
}

// a column's mean from its sum; a constant column's mean is its value
PLT_HD double mean_of(double sum, double lo, double hi, int64_t N) { return lo == hi ? lo : sum / (double)N; }
PLT_HD double std_of(double sq, int64_t N) { return sqrt(sq / (double)N); }

// ---- transform -----------------------------------------------------------------------------------------------------------
PLT_HD float apply1(float x, float sub, float div) {
#pragma clang fp contract(off)
  if (div == 0.f) return 0.f;
  const float t = x - sub;
  return t / div;
}

PLT_HD float invert1(float y, float sub, float div) {
#pragma clang fp contract(off)
  if (div == 0.f) return sub;
  const float t = y * div;
  return t + sub;
}

}  // namespace pt
}  // namespace pl

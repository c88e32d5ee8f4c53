// Cameras: the pinhole projection with radial and tangential distortion of a camera-frame pose, its analytic Jacobian, the
// reprojection residual and loss against a 2-D target, and the per-pose root translation that best explains a 2-D track,
// written once for the device kernels and the host entry points: pl_camera_project / pl_camera_project_bwd /
// pl_camera_reproj_errors / pl_camera_reproj_loss_fwd_bwd / pl_camera_fit_translation and their _host forms run this text.
// The reference carries the Human3.6M intrinsics (phase3_direct/my_HybrIK/utils.py:131-172: focal length, centre, three
// radial and two tangential coefficients per camera) and returns one field per sample, but never projects with them
// (Model.py:185-189 is commented out): PARITY UNPINNED, the form below is the one in common use for these coefficients.
//
// Camera row, nine fp32 values: fx, fy, cx, cy, k1, k2, k3, p1, p2.  cam_ids [B] int32 or none: without them every pose uses
// row 0; an id outside [0, C) reads no row: its camera is nine NaN, and every value of its pose that depends on the camera
// is NaN (the gradient of a column whose div == 0 stays 0).
//
// Point of joint j of pose b, fp32, each step rounded:  q = X[b][j]  ->  with (sub, div) [J][3]  q = q div + sub
// (pose_table.h invert1; a column with div == 0 is the constant sub)  ->  with t [B][3]  p = q + t[b].
//
// Projection of p = (X, Y, Z), fp32, every operation rounded by itself in this order, divisions correctly rounded:
//   x = X / Z,  y = Y / Z,  r2 = x*x + y*y
//   rad = 1 + r2*(k1 + r2*(k2 + r2*k3))
//   tan = p1*x + p2*y
//   u = fx * (x*(rad + tan) + p1*r2) + cx
//   v = fy * (y*(rad + tan) + p2*r2) + cy
// No clamp and no special case for Z <= 0: the values are what IEEE arithmetic gives.  With k1 = k2 = k3 = p1 = p2 = 0 this
// is fx*(X/Z) + cx bit for bit (x*(1 + 0) + 0).
//
// Jacobian of (u, v) by (X, Y, Z), fp32, written once (project_point): with s = rad + tan, dr = k1 + r2*(2 k2 + 3 k3 r2),
// gx = dr*2x + p1, gy = dr*2y + p2:
//   a = d u'/dx = s + x*gx + p1*2x     b = d u'/dy = x*gy + p1*2y
//   c = d v'/dx = y*gx + p2*2x         d = d v'/dy = s + y*gy + p2*2y
//   du/d(X, Y, Z) = fx (a, b, -(a x + b y)) / Z,   dv/d(X, Y, Z) = fy (c, d, -(c x + d y)) / Z,
// six correctly rounded divisions by Z (a product with 1/Z would carry the reciprocal's rounding into every entry).
// The gradient of a joint is g = du_bar ju + dv_bar jv; dX = g div through a transform (0 where div == 0), and the
// translation's gradient is the sum of its pose's g in joint order, added in fp64 and rounded to fp32 once.
//
// Residual of a joint against a target (tu, tv):  du = (u - tu) / div_w,  dv = (v - tv) / div_h  (div defaults to (1, 1): the
// convention of the track preparation).  Error = sqrtf(du*du + dv*dv).  Loss kinds: l1 = |du| + |dv| over B J 2 elements,
// mse = du*du + dv*dv over B J 2, l2 = the error over B J.  A weight MULTIPLIES the joint's value (0 * NaN = NaN); the
// normaliser stays the element count.
//
// Fit of a pose's translation (fit_pose).  A joint takes part iff its weight is > 0 (weights SELECT here; none = all).
//   initialisation  without distortion, n = ((u - cx)/fx, (v - cy)/fy) in fp32: each joint gives  tx - n_x tz = n_x Z - X,
//                   ty - n_y tz = n_y Z - Y;  weighted 3 x 3 normal equations, closed form (cofactors).
//   iters steps     Gauss-Newton on the distorted model: sum w (ju ju^T + jv jv^T) delta = sum w (ju ru + jv rv),
//                   r = target - projection.  The count is fixed: no convergence test.
//   rms             sqrt(sum w (ru^2 + rv^2) / sum w) after the last step.
// The whole fit runs in FP64 on its fp32 inputs -- the 3 x 3 systems, their solution, and the projection and Jacobian of the
// steps (project_point<double>) -- and t and rms are rounded to fp32 once.  Why: the normal matrix of a pose at 5 m has a
// condition number of a few hundred, and the depth is the weak direction (du/dtz is some 10 px/m over a body's width), so an
// fp32 projection's rounding, 3e-5 px at u = 1000, alone moves tz by about one fp32 ulp of 5 m and fp32 sums by more.
// Measured maxima against the float64 restatement over the fit cases of tests/test_camera_host.py: the all-fp32 restatement
// 1.43e-6 m in t, this text with fp64 sums but fp32 projections 2.95e-6 m, this form 3.94e-7 m (one ulp of 5 m is 4.8e-7;
// DESIGN.md 3g.2).  A pose is degenerate -- t and rms NaN -- when fewer than two joints take part or a
// system's determinant is not > kDetFloor times the product of its diagonal (a determinant that is not > 0, up to the
// rounding of the fp64 determinant itself, which is 1e-16 of that product; a NaN fails the comparison).
#pragma once
#include <math.h>
#include <stdint.h>

#include "pose_table.h"

namespace pl {
namespace cm {

constexpr int kCamFloats = 9, kMaxJoints = 32, kMaxIters = 8;
constexpr int kL1 = 0, kMse = 1, kL2 = 2;
constexpr double kDetFloor = 1e-12;
constexpr int kTileThreads = 256;     // a loss / backward workgroup: kTileThreads / J whole poses, one lane per (pose, joint)
constexpr int kFinalThreads = 1024;   // the loss's second launch
constexpr int kFitPoses = 64;         // poses (= lanes) of a fit workgroup

struct Cam {
  float fx, fy, cx, cy, k1, k2, k3, p1, p2;
};

// what an entry reads besides the poses; built on the host, passed by value
struct Scene {
  const float* cams;        // [C][9]
  int n_cam;
  const int32_t* cam_ids;   // [B] or nullptr
  const float* t;           // [B][3] or nullptr
  const float* sub;         // [J][3] or nullptr, with div
  const float* div;
};

PLT_HD Cam load_cam(const float* r) { return Cam{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]}; }

PLT_HD Cam nan_cam() {
  const float n = pt::nan_f();
  return Cam{n, n, n, n, n, n, n, n, n};
}

// the camera of pose b: row 0 without ids (a uniform address); a row is never loaded for an id outside [0, C)
PLT_HD bool pose_cam(const Scene& s, int64_t b, Cam* c) {
  if (!s.cam_ids) {
    *c = load_cam(s.cams);
    return true;
  }
  const int32_t id = s.cam_ids[b];
  if (id < 0 || id >= s.n_cam) {
    *c = nan_cam();
    return false;
  }
  *c = load_cam(s.cams + (int64_t)id * kCamFloats);
  return true;
}

// q of joint j from xj = &X[b][j][0]: through the transform when there is one
PLT_HD void raw_point(const Scene& s, const float* xj, int j, float q[3]) {
  for (int d = 0; d < 3; ++d) q[d] = s.sub ? pt::invert1(xj[d], s.sub[3 * j + d], s.div[3 * j + d]) : xj[d];
}

// p = q + t[b]
PLT_HD void cam_point(const Scene& s, const float* xj, int64_t b, int j, float p[3]) {
#pragma clang fp contract(off)
  raw_point(s, xj, j, p);
  if (s.t)
    for (int d = 0; d < 3; ++d) p[d] = p[d] + s.t[3 * b + d];
}

// uv of p and, ju != nullptr, the rows ju = du/d(X, Y, Z), jv = dv/d(X, Y, Z).  T = float everywhere but in the fit, which
// runs this text in double on the same fp32 camera row.
template <typename T>
PLT_HD void project_point(const Cam& cam, const T p[3], T uv[2], T* ju, T* jv) {
#pragma clang fp contract(off)
  const struct { T fx, fy, cx, cy, k1, k2, k3, p1, p2; } c = {(T)cam.fx, (T)cam.fy, (T)cam.cx, (T)cam.cy, (T)cam.k1,
                                                              (T)cam.k2, (T)cam.k3, (T)cam.p1, (T)cam.p2};
  const T x = p[0] / p[2], y = p[1] / p[2];
  const T xx = x * x, yy = y * y;
  const T r2 = xx + yy;
  const T r3 = r2 * c.k3;
  const T r23 = c.k2 + r3;
  const T r22 = r2 * r23;
  const T r12 = c.k1 + r22;
  const T r11 = r2 * r12;
  const T rad = (T)1 + r11;
  const T tx = c.p1 * x, ty = c.p2 * y;
  const T tan = tx + ty;
  const T s = rad + tan;
  const T xs = x * s, ys = y * s;
  const T pr1 = c.p1 * r2, pr2 = c.p2 * r2;
  const T ud = xs + pr1, vd = ys + pr2;
  const T fu = c.fx * ud, fv = c.fy * vd;
  uv[0] = fu + c.cx;
  uv[1] = fv + c.cy;
  if (!ju) return;
  const T k3r = (T)3 * c.k3;
  const T d0 = k3r * r2;
  const T k22 = (T)2 * c.k2;
  const T d1 = k22 + d0;
  const T d2 = d1 * r2;
  const T dr = c.k1 + d2;
  const T x2 = (T)2 * x, y2 = (T)2 * y;
  const T gx0 = dr * x2, gy0 = dr * y2;
  const T gx = gx0 + c.p1, gy = gy0 + c.p2;
  const T xgx = x * gx, xgy = x * gy, ygx = y * gx, ygy = y * gy;
  const T p1x2 = c.p1 * x2, p1y2 = c.p1 * y2, p2x2 = c.p2 * x2, p2y2 = c.p2 * y2;
  const T a0 = s + xgx;
  const T a = a0 + p1x2;
  const T b = xgy + p1y2;
  const T cc = ygx + p2x2;
  const T e0 = s + ygy;
  const T e = e0 + p2y2;
  const T ax = a * x, by = b * y, cx = cc * x, ey = e * y;
  const T az = ax + by, cz = cx + ey;
  const T fa = c.fx * a, fb = c.fx * b, fz = c.fx * az;
  const T fc = c.fy * cc, fe = c.fy * e, fw = c.fy * cz;
  ju[0] = fa / p[2];
  ju[1] = fb / p[2];
  ju[2] = -(fz / p[2]);
  jv[0] = fc / p[2];
  jv[1] = fe / p[2];
  jv[2] = -(fw / p[2]);
}

// g = du_bar ju + dv_bar jv
PLT_HD void joint_grad(float du_bar, float dv_bar, const float ju[3], const float jv[3], float g[3]) {
#pragma clang fp contract(off)
  for (int d = 0; d < 3; ++d) {
    const float a = du_bar * ju[d], b = dv_bar * jv[d];
    g[d] = a + b;
  }
}

// dX of joint j from its g: through the transform's div when there is one
PLT_HD void chain_point(const Scene& s, int j, const float g[3], float dx[3]) {
#pragma clang fp contract(off)
  for (int d = 0; d < 3; ++d) {
    if (!s.div) {
      dx[d] = g[d];
    } else {
      const float dv = s.div[3 * j + d];
      dx[d] = dv == 0.f ? 0.f : g[d] * dv;
    }
  }
}

// (du, dv) of a joint
PLT_HD void residual(const float uv[2], const float* tgt, float div_w, float div_h, float* du, float* dv) {
#pragma clang fp contract(off)
  const float a = uv[0] - tgt[0], b = uv[1] - tgt[1];
  *du = a / div_w;
  *dv = b / div_h;
}

PLT_HD float pixel_error(float du, float dv) {
#pragma clang fp contract(off)
  const float a = du * du, b = dv * dv;
  return sqrtf(a + b);
}

PLT_HD float sign_nan(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : v); }      // +-0 and NaN pass

// The value of a joint (times its weight) and (du_bar, dv_bar) = coef d value / d(u, v); coef = grad_scale / elements
PLT_HD float joint_loss(int kind, float du, float dv, const float* w, float coef, float div_w, float div_h, float* du_bar,
                        float* dv_bar) {
#pragma clang fp contract(off)
  float e, gu, gv;
  if (kind == kL1) {
    e = fabsf(du) + fabsf(dv);
    gu = sign_nan(du);
    gv = sign_nan(dv);
  } else if (kind == kMse) {
    const float a = du * du, b = dv * dv;
    e = a + b;
    gu = 2.f * du;
    gv = 2.f * dv;
  } else {
    e = pixel_error(du, dv);
    gu = e == 0.f ? 0.f : du / e;
    gv = e == 0.f ? 0.f : dv / e;
  }
  const float cw = w ? coef * *w : coef;
  const float gu1 = gu * cw, gv1 = gv * cw;
  *du_bar = gu1 / div_w;
  *dv_bar = gv1 / div_h;
  return w ? *w * e : e;
}

// uv of joint (b, j) of X [B][J][3]; the Jacobian rows when ju != nullptr.  A pose with a bad camera id: all NaN
PLT_HD void project_joint(const Scene& s, const Cam& c, const float* X, int J, int64_t b, int j, float uv[2], float* ju,
                          float* jv) {
  float p[3];
  cam_point(s, X + (b * J + j) * 3, b, j, p);
  project_point<float>(c, p, uv, ju, jv);
}

// ---- loss: the order of its sums, a function of (B, J) alone ------------------------------------------------------------
// The joints' fp32 values are added in FP64 (a mean over B J values must not carry the rounding of B J fp32 additions):
// a workgroup owns tile_poses(J) consecutive poses; a pose's value is its joints' added in joint order; a workgroup's partial
// its poses' added in pose order; the loss the partials added by final_sum: lane i of kFinalThreads adds partials i,
// i + kFinalThreads, ... in order, then the lanes are halved (lane i += lane i + h, h = 512 .. 1), then one division by the
// element count and one rounding to fp32.
PLT_HD int tile_poses(int J) { return kTileThreads / J; }
PLT_HD int64_t loss_tiles(int64_t B, int J) { return (B + tile_poses(J) - 1) / tile_poses(J); }

// ---- fit ------------------------------------------------------------------------------------------------------------------
// x of the symmetric system m = (m00, m01, m02, m11, m12, m22), m x = b, by cofactors; false when the determinant is not
// > kDetFloor times the diagonal's product
PLT_HD bool solve3(const double m[6], const double b[3], double x[3]) {
#pragma clang fp contract(off)
  const double c00 = m[3] * m[5] - m[4] * m[4];
  const double c01 = m[2] * m[4] - m[1] * m[5];
  const double c02 = m[1] * m[4] - m[2] * m[3];
  const double c11 = m[0] * m[5] - m[2] * m[2];
  const double c12 = m[1] * m[2] - m[0] * m[4];
  const double c22 = m[0] * m[3] - m[1] * m[1];
  const double det = (m[0] * c00 + m[1] * c01) + m[2] * c02;
  const double scale = (m[0] * m[3]) * m[5];
  x[0] = ((c00 * b[0] + c01 * b[1]) + c02 * b[2]) / det;
  x[1] = ((c01 * b[0] + c11 * b[1]) + c12 * b[2]) / det;
  x[2] = ((c02 * b[0] + c12 * b[1]) + c22 * b[2]) / det;
  return det > kDetFloor * scale;
}

// One pose.  q [J][3] its root-relative joints (already through the transform), uv [J][2] the target in pixels, w [J] or
// nullptr: rows of the caller's arrays or of a workgroup's staging.  t [3] and rms out; NaN for a degenerate pose.
PLT_HD void fit_pose(const Cam& c, const float* q, const float* uv, const float* w, int J, int iters, float t[3], float* rms) {
#pragma clang fp contract(off)
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0}, x[3];
  int n = 0;
  for (int j = 0; j < J; ++j) {
    const float wf = w ? w[j] : 1.f;
    if (!(wf > 0.f)) continue;
    ++n;
    const double wj = (double)wf;
    const float ux = uv[2 * j] - c.cx, vy = uv[2 * j + 1] - c.cy;
    const double nx = (double)(ux / c.fx), ny = (double)(vy / c.fy);
    const double X = (double)q[3 * j], Y = (double)q[3 * j + 1], Z = (double)q[3 * j + 2];
    const double rx = nx * Z - X, ry = ny * Z - Y;
    m[0] += wj;
    m[2] -= wj * nx;
    m[4] -= wj * ny;
    m[5] += wj * (nx * nx + ny * ny);
    r[0] += wj * rx;
    r[1] += wj * ry;
    r[2] -= wj * (nx * rx + ny * ry);
  }
  m[3] = m[0];
  bool ok = n >= 2;
  ok = solve3(m, r, x) && ok;
  double td[3] = {x[0], x[1], x[2]};
  double se = 0.0, sw = 0.0;
  for (int it = 0; it <= iters; ++it) {                  // the pass after the last step only measures
    for (int k = 0; k < 6; ++k) m[k] = 0.0;
    r[0] = r[1] = r[2] = 0.0;
    se = sw = 0.0;
    for (int j = 0; j < J; ++j) {
      const float wf = w ? w[j] : 1.f;
      if (!(wf > 0.f)) continue;
      const double wj = (double)wf;
      double p[3], pu[2], ju[3], jv[3];
      for (int d = 0; d < 3; ++d) p[d] = (double)q[3 * j + d] + td[d];
      project_point<double>(c, p, pu, ju, jv);
      const double ru = (double)uv[2 * j] - pu[0], rv = (double)uv[2 * j + 1] - pu[1];
      const double a0 = ju[0], a1 = ju[1], a2 = ju[2], b0 = jv[0], b1 = jv[1], b2 = jv[2];
      m[0] += wj * (a0 * a0 + b0 * b0);
      m[1] += wj * (a0 * a1 + b0 * b1);
      m[2] += wj * (a0 * a2 + b0 * b2);
      m[3] += wj * (a1 * a1 + b1 * b1);
      m[4] += wj * (a1 * a2 + b1 * b2);
      m[5] += wj * (a2 * a2 + b2 * b2);
      r[0] += wj * (a0 * ru + b0 * rv);
      r[1] += wj * (a1 * ru + b1 * rv);
      r[2] += wj * (a2 * ru + b2 * rv);
      se += wj * (ru * ru + rv * rv);
      sw += wj;
    }
    if (it == iters) break;
    ok = solve3(m, r, x) && ok;
    for (int d = 0; d < 3; ++d) td[d] = td[d] + x[d];
  }
  const float bad = pt::nan_f();
  for (int d = 0; d < 3; ++d) t[d] = ok ? (float)td[d] : bad;
  *rms = ok ? (float)sqrt(se / sw) : bad;
}

// a staged row's stride: odd, so that lanes walking their own rows fall on different banks
PLT_HD int odd_stride(int n) { return n | 1; }

}  // namespace cm
}  // namespace pl

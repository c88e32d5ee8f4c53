// Video tracks: what turns a detector's per-frame keypoints into a track a lifter can read (joint remap, scaling, validity,
// gap fill), the confidence-weighted temporal FIR over a track, and the velocity / acceleration errors of a 3-D track,
// written once for the device kernels and the host entry points: pl_track_remap / pl_track_prepare / pl_track_filter /
// pl_track_velocity_errors and their _host forms run this text.
// The reference runs openpifpaf on the frames, maps COCO-17 to the H36M-17 layout and keeps one (17, 3) [x, y, confidence]
// row per frame, all zeros where nothing was detected (phase1_lifting/video2keypoints.py:14-57, :83-98).
//
// Sequences.  seq [T] int32 or none; the frames of one video are contiguous.  Frame s is in frame t's sequence when every
// frame from t to s carries seq[t]; without seq all T frames are one sequence.  Nothing reads across a sequence boundary.
//
// Remap (COCO17), fp32, video2keypoints.py:40-56 in its order: a midpoint is (a + b) * 0.5f, joint 7 is made from the
// computed joints 0 and 8.  The confidence of a derived joint is the minimum of its sources' (joint 7: four sources), a
// NaN confidence winning.  H36M17 copies the row.
//
// Prepare, per (t, j): s = (x / div_w, y / div_h), two correctly rounded divisions.  The sample is VALID when
// conf >= conf_thr and both scaled coordinates are finite.  An invalid sample looks on each side for the nearest valid
// sample of joint j, visiting t -+ i for i = 1 .. G; a side's search LEAVES the sequence when one of those frames is
// outside it.
//   state 0  valid                                                  xy = s                             w = conf
//   state 1  found a < t < b and b - a - 1 <= G                     xy = s_a + (s_b - s_a) * ((float)(t - a) / (float)(b - a))
//                                                                                                      w = fill_conf * min(conf_a, conf_b)
//   state 2  one side found, the other side's search left the sequence   xy = s_side                   w = fill_conf * conf_side
//   state 3  anything else                                          xy = s where finite, else +0       w = +0
// Every choice is a select: a NaN in an invalid sample reaches no output.
//
// Filter, per (t, j), taps [K], K odd, h = K / 2:  y = (sum_k c_k x[s_k]) / (sum_k c_k),  c_k = taps[k] * w[s_k][j],
// s_k = t + k - h, over the s_k inside t's sequence, in increasing k, fp32, product and sum rounded separately; the first
// term starts each sum.  A sample with w == 0 is skipped; without w the weight is 1.  One correctly rounded division per
// element.  A denominator that is not > 0 (no sample left, or a NaN weight) gives y = x[t], the bits copied.
//
// Velocity errors, per (t, j), 3-D: order 1  || (p[t] - p[t-1]) - (g[t] - g[t-1]) ||, order 2 the same with
// (q[t+1] - 2 q[t]) + q[t-1]; differences, squares and their sum (x, y, z in order) rounded one by one, sqrtf correctly
// rounded.  count[t] = 1 where the stencil lies inside t's sequence; elsewhere the error is +0.  With (sub, div) the poses
// are taken back first, q = v div[c] + sub[c] (pose_table.h invert1).
#pragma once
#include <math.h>
#include <stdint.h>

#include "pose_table.h"

namespace pl {
namespace tk {

constexpr int kJoints = 17;           // of a detector row
constexpr int kMaxGap = 64, kMaxTaps = 65, kMaxJoints = 32;
constexpr int kLayoutCoco17 = 0, kLayoutH36m17 = 1;
constexpr int kValid = 0, kInterpolated = 1, kHeld = 2, kLost = 3;

struct Prepare {
  int layout, max_gap;
  float div_w, div_h, conf_thr, fill_conf;
};

struct Taps {
  int k;
  float v[kMaxTaps];
};

PLT_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e+38f; }        // false for NaN
PLT_HD float min_nan(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }

// COCO sources of an H36M joint: one joint (b < 0) or the midpoint of two; joint 7 is special
PLT_HD void coco_sources(int j, int* a, int* b) {
  // a switch, not a table: a table indexed per lane would live in private memory
  int s = 0, m = -1;
  switch (j) {
    case 0: s = 11; m = 12; break;
    case 1: s = 12; break;
    case 2: s = 14; break;
    case 3: s = 16; break;
    case 4: s = 11; break;
    case 5: s = 13; break;
    case 6: s = 15; break;
    case 8: s = 5; m = 6; break;
    case 9: s = 0; break;
    case 10: s = 1; m = 2; break;
    case 11: s = 5; break;
    case 12: s = 7; break;
    case 13: s = 9; break;
    case 14: s = 6; break;
    case 15: s = 8; break;
    case 16: s = 10; break;
    default: break;
  }
  *a = s;
  *b = m;
}

PLT_HD void coco_mid(const float* row, int a, int b, float o[3]) {
#pragma clang fp contract(off)
  const float* p = row + 3 * a;
  const float* q = row + 3 * b;
  o[0] = (p[0] + q[0]) * 0.5f;
  o[1] = (p[1] + q[1]) * 0.5f;
  o[2] = min_nan(p[2], q[2]);
}

// joint j of a detector row [17][3] in the H36M-17 layout: (x, y, conf)
PLT_HD void remap_joint(const float* row, int layout, int j, float o[3]) {
#pragma clang fp contract(off)
  if (layout == kLayoutH36m17) {
    o[0] = row[3 * j]; o[1] = row[3 * j + 1]; o[2] = row[3 * j + 2];
    return;
  }
  if (j == 7) {
    float r[3], n[3];
    coco_mid(row, 11, 12, r);
    coco_mid(row, 5, 6, n);
    o[0] = (r[0] + n[0]) * 0.5f;
    o[1] = (r[1] + n[1]) * 0.5f;
    o[2] = min_nan(r[2], n[2]);
    return;
  }
  int a, b;
  coco_sources(j, &a, &b);
  if (b < 0) {
    o[0] = row[3 * a]; o[1] = row[3 * a + 1]; o[2] = row[3 * a + 2];
  } else {
    coco_mid(row, a, b, o);
  }
}

// the scaled sample of (t, j) and whether it is valid; s = (x / div_w, y / div_h, conf)
PLT_HD bool scaled_sample(const Prepare& a, const float* det, int64_t t, int j, float s[3]) {
#pragma clang fp contract(off)
  float o[3];
  remap_joint(det + t * (kJoints * 3), a.layout, j, o);
  s[0] = o[0] / a.div_w;
  s[1] = o[1] / a.div_h;
  s[2] = o[2];
  return s[2] >= a.conf_thr && finite_f(s[0]) && finite_f(s[1]);
}

// One side of the search of an invalid (t, j): frames t + dir i, i = 1 .. G.  Returns the distance of the nearest valid
// sample (its values in s), 0 when none was found; *left = the search met a frame outside the sequence.
PLT_HD int search_side(const Prepare& a, const float* det, const int32_t* seq, int64_t T, int64_t t, int j, int dir, float s[3],
                       bool* left) {
  *left = false;
  for (int i = 1; i <= a.max_gap; ++i) {
    const int64_t u = t + (int64_t)dir * i;
    if (u < 0 || u >= T || (seq && seq[u] != seq[t])) {
      *left = true;
      return 0;
    }
    if (scaled_sample(a, det, u, j, s)) return i;
  }
  return 0;
}

// output of (t, j): xy [2], w, state
PLT_HD void prepare_joint(const Prepare& a, const float* det, const int32_t* seq, int64_t T, int64_t t, int j, float* xy,
                          float* w, uint8_t* state) {
#pragma clang fp contract(off)
  float s[3];
  if (scaled_sample(a, det, t, j, s)) {
    xy[0] = s[0]; xy[1] = s[1];
    *w = s[2];
    *state = (uint8_t)kValid;
    return;
  }
  float sa[3], sb[3];
  bool left_a, left_b;
  const int da = search_side(a, det, seq, T, t, j, -1, sa, &left_a);
  const int db = search_side(a, det, seq, T, t, j, +1, sb, &left_b);
  if (da > 0 && db > 0 && da + db - 1 <= a.max_gap) {
    const float f = (float)da / (float)(da + db);
    for (int d = 0; d < 2; ++d) {
      const float span = sb[d] - sa[d];
      const float step = span * f;
      xy[d] = sa[d] + step;
    }
    *w = a.fill_conf * min_nan(sa[2], sb[2]);
    *state = (uint8_t)kInterpolated;
    return;
  }
  if ((da > 0) != (db > 0) && (da > 0 ? left_b : left_a)) {
    xy[0] = da > 0 ? sa[0] : sb[0];
    xy[1] = da > 0 ? sa[1] : sb[1];
    *w = a.fill_conf * (da > 0 ? sa[2] : sb[2]);
    *state = (uint8_t)kHeld;
    return;
  }
  xy[0] = finite_f(s[0]) ? s[0] : 0.f;
  xy[1] = finite_f(s[1]) ? s[1] : 0.f;
  *w = 0.f;
  *state = (uint8_t)kLost;
}

// ---- filter ----------------------------------------------------------------------------------------------------------------
// [lo, hi], -h <= lo <= 0 <= hi <= h: the offsets s - t of the frames of t's sequence within h of t.  seq (or nullptr) is
// indexed seq[s - seq0].
PLT_HD void seq_window(const int32_t* seq, int64_t seq0, int64_t T, int64_t t, int h, int* lo, int* hi) {
  int l = 0, r = 0;
  while (l > -h && t + l - 1 >= 0 && (!seq || seq[t + l - 1 - seq0] == seq[t - seq0])) --l;
  while (r < h && t + r + 1 < T && (!seq || seq[t + r + 1 - seq0] == seq[t - seq0])) ++r;
  *lo = l;
  *hi = r;
}

// y [D] of one (t, j).  xt = &x[t][j][0] with frames xstride floats apart, wt = &w[t][j] (or nullptr) with frames wstride apart.
template <int D>
PLT_HD void fir_joint(const float* xt, int xstride, const float* wt, int wstride, const Taps& taps, int lo, int hi, float* y) {
#pragma clang fp contract(off)
  const int h = taps.k / 2;
  float num[3] = {0.f, 0.f, 0.f}, den = 0.f;
  bool any = false;
  for (int k = 0; k < taps.k; ++k) {
    const int o = k - h;
    if (o < lo || o > hi) continue;
    const float ws = wt ? wt[o * wstride] : 1.f;
    if (ws == 0.f) continue;
    const float c = taps.v[k] * ws;
    const float* xs = xt + o * xstride;
    for (int d = 0; d < D; ++d) {
      const float p = c * xs[d];
      num[d] = any ? num[d] + p : p;
    }
    den = any ? den + c : c;
    any = true;
  }
  const bool ok = any && den > 0.f;
  for (int d = 0; d < D; ++d) y[d] = ok ? num[d] / den : xt[d];
}

// ---- velocity ----------------------------------------------------------------------------------------------------------------
// element d of joint j of frame t, taken back through (sub, div) when given; q = &v[t][j][0], c0 = 3 j
PLT_HD float vel_load(const float* q, int d, const float* sub, const float* div, int c0) {
  return sub ? pt::invert1(q[d], sub[c0 + d], div[c0 + d]) : q[d];
}

// the order-th difference of a track at t, element d; stride = floats between frames
PLT_HD float vel_stencil(const float* q, int stride, int order, int d, const float* sub, const float* div, int c0) {
#pragma clang fp contract(off)
  const float v0 = vel_load(q, d, sub, div, c0), vm = vel_load(q - stride, d, sub, div, c0);
  if (order == 1) return v0 - vm;
  const float vp = vel_load(q + stride, d, sub, div, c0);
  const float two = 2.f * v0;
  const float a = vp - two;
  return a + vm;
}

// whether frame t has its stencil inside its sequence
PLT_HD bool vel_has_stencil(const int32_t* seq, int64_t T, int64_t t, int order) {
  if (t < 1 || (seq && seq[t - 1] != seq[t])) return false;
  if (order == 2 && (t + 1 >= T || (seq && seq[t + 1] != seq[t]))) return false;
  return true;
}

// error of (t, j) where the stencil exists; p, g = &pred[t][j][0], &tgt[t][j][0]
PLT_HD float vel_error(const float* p, const float* g, int stride, int order, const float* sub, const float* div, int j) {
#pragma clang fp contract(off)
  float acc = 0.f;
  for (int d = 0; d < 3; ++d) {
    const float e = vel_stencil(p, stride, order, d, sub, div, 3 * j) - vel_stencil(g, stride, order, d, sub, div, 3 * j);
    const float sq = e * e;
    acc = d == 0 ? sq : acc + sq;
  }
  return sqrtf(acc);
}

}  // namespace tk
}  // namespace pl

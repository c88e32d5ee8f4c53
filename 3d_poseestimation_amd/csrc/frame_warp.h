// Frame augmentation that follows the pose augmentation (pose_augment.h): the frame of a dataset row is flipped, turned,
// scaled and shifted by the very draws its 2-D pose gets, inside the launch that gathers, resizes and normalises the batch.
// Written once for the device kernel and the host entry point: pl_frame_warp_gather and pl_frame_warp_host run this text.
// The reference resizes per sample on DataLoader workers (phase3_direct/my_HybrIK/H36_dataset.py:129-131
// `cv2.resize(frame,(256,256))`, `frame/256.0`) and leaves the paired augmentation commented out (:98-117, `cv2.flip(frame,1)`
// next to flip_pose).
//
// Source: a table src[N][Hs][Ws][3], uint8 or fp32.  Output: out[n][Ho][Wo][3], fp32.  The decisions flip, cs, sn, sc, tx, ty of
// a row are pa::decide0 / pa::decide1 on pa::draw(plan, row, 0 / 1): nothing is restated here.  jitter_sigma is pose noise and
// does not touch a frame.
//
// Output pixel (i, j) of a sample, every stage whose parameter is 0 skipped as in pose_augment.h:
//   1. u = (j + 0.5) / Wo, v = (i + 0.5) / Ho: image-normalised coordinates at pixel centres, x right and y down -- the 2-D
//      pose's coordinates.
//   2. undo the pose transform (flip, rotate about (cx, cy) by [[c, -s], [s, c]], scale about (cx, cy), translate) in reverse:
//        u -= tx, v -= ty;   u = (u - cx) / sc + cx, v = (v - cy) / sc + cy;
//        du = u - cx, dv = v - cy: u = (c du + s dv) + cx, v = (-s du + c dv) + cy;   if flipped, u = 1 - u.
//   3. xs = u Ws - 0.5, ys = v Hs - 0.5.
//   4. xs outside [-0.5, Ws - 0.5] or ys outside [-0.5, Hs - 0.5]: the pixel is `fill` on all three channels.
//   5. otherwise clamp xs to [0, Ws - 1], ys to [0, Hs - 1]; x0 = floor(xs), x1 = min(x0 + 1, Ws - 1), fx = xs - x0; y likewise.
//   6. value = scale * ((1 - fy) * ((1 - fx) p00 + fx p01) + fy * ((1 - fx) p10 + fx p11)), uint8 taps converted to fp32 first.
// With every stage off this is bilinear resampling in the half-pixel convention (cv2.resize INTER_LINEAR,
// F.interpolate(align_corners=False)); there is no antialiasing.
//
// Arithmetic.  Every product, quotient and sum is rounded on its own (contraction is off in every function below), so
// configurations without sincosf give the same bits on the host, on the device and in a numpy fp32 restatement.  Two steps
// are evaluated in an algebraically equal form, because the literal one is not exact in fp32 where exactness is wanted
// (((j + 0.5) / 28) * 28 - 0.5 is 15 - 2^-20 at j = 15; 1 - u moves 5 of 20 columns of a 20-wide frame off their integers):
//   - the flip is taken on the source position: xs = (Ws - 1) - xs  (= (1 - u) Ws - 0.5), so a flipped integer stays one;
//   - with shift, scale and rotation all off, u and v are never formed: xs = (j + 0.5) * (Ws / Wo) - 0.5, ys likewise -- the
//     form cv2.resize and F.interpolate use.  A same-size resize then copies scale * p, a flip mirrors it, and halving a
//     frame has weights of exactly 0.5.
#pragma once
#include "pose_augment.h"

namespace pl {
namespace fw {

struct Geom {
  int Hs, Ws, Ho, Wo;
  float scale, fill;
};

// The decisions of a row that a frame reads: pose_augment.h's calls c2 = 0 and c2 = 1, as augment_pose makes them.
PLA_HD pa::Pose pose_of(const pa::Plan& p, uint64_t row) {
  uint32_t w[4];
  pa::Pose q = {0, 1.f, 0.f, 1.f, 0.f, 0.f};
  if (pa::needs_call(p, 0)) { pa::draw(p, row, 0, w); pa::decide0(p, w, q); }
  else q.flip = p.flip_mode == 2;
  if (pa::needs_call(p, 1)) { pa::draw(p, row, 1, w); pa::decide1(p, w, q); }
  return q;
}

// steps 1-3: the source position of output pixel (i, j)
PLA_HD void source_position(const pa::Plan& p, const pa::Pose& q, const Geom& g, int i, int j, float& xs, float& ys) {
#pragma clang fp contract(off)
  if (p.max_shift == 0.f && p.scale_range == 0.f && p.max_rot == 0.f) {
    xs = ((float)j + 0.5f) * ((float)g.Ws / (float)g.Wo) - 0.5f;
    ys = ((float)i + 0.5f) * ((float)g.Hs / (float)g.Ho) - 0.5f;
  } else {
    float u = ((float)j + 0.5f) / (float)g.Wo;
    float v = ((float)i + 0.5f) / (float)g.Ho;
    if (p.max_shift != 0.f) { u = u - q.tx; v = v - q.ty; }
    if (p.scale_range != 0.f) {
      u = (u - p.cx) / q.sc + p.cx;
      v = (v - p.cy) / q.sc + p.cy;
    }
    if (p.max_rot != 0.f) {
      const float du = u - p.cx, dv = v - p.cy;
      u = (q.cs * du + q.sn * dv) + p.cx;
      v = ((-q.sn) * du + q.cs * dv) + p.cy;
    }
    xs = u * (float)g.Ws - 0.5f;
    ys = v * (float)g.Hs - 0.5f;
  }
  if (q.flip) xs = (float)(g.Ws - 1) - xs;
}

// steps 4-5: where a source position reads.  inside = false: the pixel is `fill`; the taps are then those of the position
// clamped into the frame (of pixel (0, 0) for a NaN position), legal to load and never used.
struct Taps {
  bool inside;
  int x0, x1, y0, y1;
  float fx, fy;
};
PLA_HD Taps taps_of(const Geom& g, float xs, float ys) {
#pragma clang fp contract(off)
  Taps t;
  const float wmax = (float)(g.Ws - 1), hmax = (float)(g.Hs - 1);
  t.inside = xs >= -0.5f && xs <= wmax + 0.5f && ys >= -0.5f && ys <= hmax + 0.5f;
  xs = fminf(fmaxf(xs, 0.f), wmax);
  ys = fminf(fmaxf(ys, 0.f), hmax);
  const float xf = floorf(xs), yf = floorf(ys);
  t.fx = xs - xf; t.fy = ys - yf;
  t.x0 = (int)xf; t.y0 = (int)yf;
  t.x1 = t.x0 + 1 < g.Ws ? t.x0 + 1 : g.Ws - 1;
  t.y1 = t.y0 + 1 < g.Hs ? t.y0 + 1 : g.Hs - 1;
  return t;
}

// step 6: one channel from its four taps
PLA_HD float blend(const Geom& g, const Taps& t, float p00, float p01, float p10, float p11) {
#pragma clang fp contract(off)
  const float gx = 1.0f - t.fx, gy = 1.0f - t.fy;
  const float top = gx * p00 + t.fx * p01;
  const float bot = gx * p10 + t.fx * p11;
  return g.scale * (gy * top + t.fy * bot);
}

// step 6 on all three channels, the taps read one by one from `frame` [Hs][Ws][3]
template <typename T>
PLA_HD void sample_taps(const T* frame, const Geom& g, const Taps& t, float o[3]) {
  const T* r0 = frame + t.y0 * (g.Ws * 3);
  const T* r1 = frame + t.y1 * (g.Ws * 3);
  for (int c = 0; c < 3; ++c)
    o[c] = blend(g, t, (float)r0[t.x0 * 3 + c], (float)r0[t.x1 * 3 + c], (float)r1[t.x0 * 3 + c], (float)r1[t.x1 * 3 + c]);
}

// steps 4-6: the three channels of a pixel whose source position in `frame` [Hs][Ws][3] is (xs, ys)
template <typename T>
PLA_HD void sample(const T* frame, const Geom& g, float xs, float ys, float o[3]) {
  const Taps t = taps_of(g, xs, ys);
  if (t.inside) sample_taps(frame, g, t, o);
  else { o[0] = g.fill; o[1] = g.fill; o[2] = g.fill; }
}

}  // namespace fw
}  // namespace pl

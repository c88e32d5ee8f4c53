// Person-centred crop taken from each row's 2-D pose, written once for the device kernels and the host entry points: the
// crop forms of pl_pose_augment_gather and pl_frame_warp_gather, pl_pose_crop_boxes, pl_crop_poses and their _host forms
// run this text.  The reference sketches it ("cropping using the gt 2d as bounding box",
// phase3_direct/my_HybrIK/H36_dataset.py:120-126) with a slice min(0, ...) : max(1000, ...) that always selects the whole
// frame; here the box is real, square, and rides in the two launches that build a batch (pose_augment.h, frame_warp.h).
//
// Box of a row.  a[17][2] its SOURCE 2-D pose, image-normalised, x right and y down (frame_warp.h step 1); (Hs, Ws) the source
// frame; spec {margin > 0, centre in {bbox, root}, min_side >= 1, integer-valued}:
//   xmin, xmax, ymin, ymax over the 17 joints
//   ex = (xmax - xmin) Ws,  ey = (ymax - ymin) Hs                          pixels
//   side = max(ceil(margin max(ex, ey)), min_side)                         an integer; the box is square in source pixels
//   bbox: ccx = (0.5 (xmin + xmax)) Ws, ccy = (0.5 (ymin + ymax)) Hs;      root: ccx = a[0][0] Ws, ccy = a[0][1] Hs  (:126)
//   x0 = rint(ccx - 0.5 side),  y0 = rint(ccy - 0.5 side)                  ties to even; may be negative or past the frame
// A non-finite coordinate anywhere in the pose makes the whole box NaN (fminf / fmaxf would drop a NaN, so the test is
// explicit), and so does a side above 2^20.  min and max are exact and the finiteness test is an AND, so the box does not
// depend on the order the joints are visited in: the pose kernel reduces over lanes, the frame kernel and the host loop.
// (fminf(-0, +0) may be either zero; the zero's sign reaches no result, side >= 1 keeps ccx - 0.5 side off it.)
//
// Pose in crop coordinates, in front of every augmentation stage: a'x = (ax Ws - x0) / side, a'y = (ay Hs - y0) / side.
// pose_augment.h then runs unchanged on a': (cx, cy) = (0.5, 0.5) is the crop's centre, a flip mirrors about it
// (flip_offset 1).  The 3-D pose is untouched (weak perspective, as for scale and shift).  Back: ax = (a'x side + x0) / Ws.
//
// Frame.  Steps 1-2 of frame_warp.h unchanged, (u, v) now crop-normalised; step 3 goes through the crop-local position:
//   xl = u side - 0.5;   shift, scale and rotation all off: xl = (j + 0.5) (side / Wo) - 0.5;   flipped: xl = (side - 1) - xl;
//   xs = xl + x0     (ys likewise with Ho and y0; no flip)
// and steps 4-6 are frame_warp.h's, against the FRAME: the part of a box outside the frame is `fill`.  Integer boxes and this
// order make three cases exact in fp32: side == Wo == Ho copies scale * frame[y0:y0+Ho, x0:x0+Wo]; with a flip its mirror
// image; side == 2 Wo == 2 Ho is the 2 x 2 block mean with weights of exactly 0.5.  A NaN box is a NaN frame and a NaN 2-D
// pose.  xs reaches fw::taps_of unclamped, NaN or huge, and is clamped there before it becomes an int.
//
// Arithmetic: contraction off in every function, each product, quotient and sum rounded on its own (pose_augment.h).
#pragma once
#include "frame_warp.h"

namespace pl {
namespace fc {

constexpr float kMaxSide = 1048576.f;   // 2^20

// What the crop needs besides the pose: built on the host (crop_spec), passed by value.
struct Spec {
  float margin, min_side, Hs, Ws;
  int root;                             // centre: 0 bbox, 1 root joint
};

struct Box {
  float x0, y0, side;
};

PLA_HD bool finite1(float v) { return fabsf(v) <= 3.402823466e38f; }
PLA_HD bool box_ok(const Box& b) { return b.side == b.side; }

// the box from the pose's extent, its root joint (rx, ry) and whether every coordinate was finite
PLA_HD Box box_from_extent(const Spec& c, float xmin, float xmax, float ymin, float ymax, float rx, float ry, bool finite) {
#pragma clang fp contract(off)
  const float ex = (xmax - xmin) * c.Ws, ey = (ymax - ymin) * c.Hs;
  const float side = fmaxf(ceilf(c.margin * fmaxf(ex, ey)), c.min_side);
  float ccx, ccy;
  if (c.root) { ccx = rx * c.Ws; ccy = ry * c.Hs; }
  else { ccx = (0.5f * (xmin + xmax)) * c.Ws; ccy = (0.5f * (ymin + ymax)) * c.Hs; }
  const float h = 0.5f * side;
  Box b = {rintf(ccx - h), rintf(ccy - h), side};
  if (!finite || !(side <= kMaxSide)) {
    const float bad = NAN;
    b.x0 = bad; b.y0 = bad; b.side = bad;
  }
  return b;
}

// one whole pose a[34], one joint after the other
PLA_HD Box box_of_pose(const Spec& c, const float* a) {
  float xmin = a[0], xmax = a[0], ymin = a[1], ymax = a[1];
  bool finite = finite1(a[0]) && finite1(a[1]);
  for (int j = 1; j < 17; ++j) {
    const float x = a[2 * j], y = a[2 * j + 1];
    xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
    ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
    finite = finite && finite1(x) && finite1(y);
  }
  return box_from_extent(c, xmin, xmax, ymin, ymax, a[0], a[1], finite);
}

// coordinate d (0 = x, 1 = y) of a 2-D joint: image-normalised -> crop-normalised.  offset = false drops x0 / y0: the map's
// factor alone, which is how a gradient goes back through it.
PLA_HD float crop1(const Spec& c, const Box& b, int d, float v, bool offset = true) {
#pragma clang fp contract(off)
  const float t = v * (d == 0 ? c.Ws : c.Hs);
  const float s = offset ? t - (d == 0 ? b.x0 : b.y0) : t;
  return s / b.side;
}

// crop-normalised -> image-normalised; offset = false as in crop1
PLA_HD float uncrop1(const Spec& c, const Box& b, int d, float v, bool offset = true) {
#pragma clang fp contract(off)
  const float t = v * b.side;
  const float s = offset ? t + (d == 0 ? b.x0 : b.y0) : t;
  return s / (d == 0 ? c.Ws : c.Hs);
}

// steps 1-3 with a crop: the source position, in the frame, of output pixel (i, j)
PLA_HD void source_position(const pa::Plan& p, const pa::Pose& q, const fw::Geom& g, const Box& b, int i, int j, float& xs,
                            float& ys) {
#pragma clang fp contract(off)
  float xl, yl;
  if (p.max_shift == 0.f && p.scale_range == 0.f && p.max_rot == 0.f) {
    xl = ((float)j + 0.5f) * (b.side / (float)g.Wo) - 0.5f;
    yl = ((float)i + 0.5f) * (b.side / (float)g.Ho) - 0.5f;
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
    xl = u * b.side - 0.5f;
    yl = v * b.side - 0.5f;
  }
  if (q.flip) xl = (b.side - 1.0f) - xl;
  xs = xl + b.x0;
  ys = yl + b.y0;
}

// One whole pose with the crop in front of the augmentation: pa::augment_pose on the cropped 2-D pose.  *box is the row's.
PLA_HD void augment_pose(const Spec& c, const pa::Plan& p, uint64_t row, const float* a, const float* b, float* oa, float* ob,
                         Box* box) {
  *box = box_of_pose(c, a);
  float ac[pa::kWA];
  for (int k = 0; k < pa::kWA; ++k) ac[k] = crop1(c, *box, k & 1, a[k]);
  pa::augment_pose(p, row, ac, b, oa, ob);
}

}  // namespace fc
}  // namespace pl

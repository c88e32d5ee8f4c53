// Train-time pose augmentation (horizontal flip, in-plane rotation, 2-D scale, 2-D shift, 2-D Gaussian jitter), written
// once for the device kernel and the host entry point: pl_pose_augment_gather and pl_pose_augment_host run this text.
// The reference sketches it per sample in DataLoader workers and leaves it commented out
// (phase3_direct/my_HybrIK/H36_dataset.py:98-117 flip / translate / rotate / scale stubs with flip_pose on both tensors;
// phase1_lifting/train_1.py:83-84 `y1 + 0.05*randn`); here it rides in the launch that gathers the batch.
//
// A pose is 17 joints: a = 2-D [17][2], b = 3-D [17][3].  Conventions: image x points right and y down; the 3-D target is
// in the camera frame, root-relative, x right and y down, so one in-plane angle turns both.  2-D scale and shift leave the
// root-relative 3-D target alone (weak perspective).  A zero root row of b stays zero (flip and rotation are linear).
//
// Draws: a pure function of (seed, epoch, row), row = the pose's index in the dataset table (NOT its place in the batch):
//   key     = (seed & 0xffffffff, (seed >> 32) ^ (epoch >> 32) ^ 0x41554721)        the tag keeps it off the dropout stream
//   counter = (row & 0xffffffff, row >> 32, c2, epoch & 0xffffffff)
//   f(w) = (w >> 8) * 2^-24 in [0, 1),  g(w) = ((w >> 8) + 1) * 2^-24 in (0, 1]     both exact in fp32
//   c2 = 0: (w0, w1, w2, w3): flip iff w0 < thr(p_flip) (thr = dropout_threshold; p_flip >= 1 always, <= 0 never),
//           theta = (2 f(w1) - 1) * max_rot,  s = 1 + (2 f(w2) - 1) * scale_range,  w3 reserved
//   c2 = 1: tx = (2 f(w0) - 1) * max_shift,  ty = (2 f(w1) - 1) * max_shift
//   c2 = 2 + (k >> 2), k = joint * 2 + coord of the OUTPUT element, 0..33: lane k & 3 of that call; lanes (0, 1) from
//           (v0, v1), lanes (2, 3) from (v2, v3): r = sqrtf(-2 logf(g(v_even))), phi = 2 pi f(v_odd),
//           z_even = r cos(phi), z_odd = r sin(phi); noise_k = jitter_sigma * z
//
// Order.  2-D: flip (joint swap [4,5,6,11,12,13] <-> [1,2,3,14,15,16], x -> flip_offset - x), rotate about (cx, cy) by
// [[c, -s], [s, c]], scale about (cx, cy), translate, add noise.  3-D: flip (same swap, x -> -x), rotate (x, y) by the
// same matrix; z untouched.
//
// Arithmetic.  A stage whose parameter is 0 is skipped, not multiplied by 1 or added 0: the all-default transform copies
// bits.  Every product and sum is rounded on its own (contraction is off in every function below), so configurations
// without sincosf / logf give the same bits on the host, on the device and in a numpy fp32 restatement.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLA_HD __host__ __device__ inline
#else
#define PLA_HD inline
#endif

namespace pl {
namespace pa {

constexpr int kWA = 34, kWB = 51, kRow = kWA + kWB;   // floats of a, of b, of a pose
constexpr int kCalls = 11;                            // Philox calls of a pose: c2 = 0, 1, and 2..10 for the 34 noise values
constexpr uint32_t kStreamTag = 0x41554721u;

// What the transform needs besides the pose and its row: built on the host (plan_of), passed by value.
struct Plan {
  uint32_t k0, k1, c3;                // Philox key and the epoch's low word
  uint32_t thr;                       // flip iff w0 < thr (flip_mode 1)
  int flip_mode;                      // 0 never, 1 by the draw, 2 always
  float flip_offset, max_rot, scale_range, max_shift, sigma, cx, cy;
};

// The decisions of one pose.
struct Pose {
  int flip;
  float cs, sn, sc, tx, ty;
};

inline Plan plan_of(float p_flip, uint32_t thr, float flip_offset, float max_rot, float scale_range, float max_shift,
                    float sigma, float cx, float cy, uint64_t seed, uint64_t epoch) {
  Plan p;
  p.k0 = (uint32_t)seed;
  p.k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(epoch >> 32) ^ kStreamTag;
  p.c3 = (uint32_t)epoch;
  p.thr = thr;
  p.flip_mode = p_flip >= 1.f ? 2 : (p_flip > 0.f ? 1 : 0);
  p.flip_offset = flip_offset; p.max_rot = max_rot; p.scale_range = scale_range; p.max_shift = max_shift;
  p.sigma = sigma; p.cx = cx; p.cy = cy;
  return p;
}

// which of a pose's calls a configuration reads: c2 = 0, c2 = 1, c2 >= 2
PLA_HD bool needs_call(const Plan& p, int c2) {
  if (c2 == 0) return p.flip_mode == 1 || p.max_rot != 0.f || p.scale_range != 0.f;
  if (c2 == 1) return p.max_shift != 0.f;
  return p.sigma != 0.f;
}

// Philox4x32-10 (csrc/philox.h, oracle/philox.py) with the products written in 64 bits, so the host compiles it too
PLA_HD void philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t w[4]) {
  const uint64_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = M0 * c0, p1 = M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

PLA_HD void draw(const Plan& p, uint64_t row, int c2, uint32_t w[4]) {
  philox((uint32_t)row, (uint32_t)(row >> 32), (uint32_t)c2, p.c3, p.k0, p.k1, w);
}

PLA_HD float unit_co(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }           // f: [0, 1)
PLA_HD float unit_oc(uint32_t w) { return (float)((w >> 8) + 1u) * 5.9604644775390625e-8f; }    // g: (0, 1]
// 2 f(w) - 1 in [-1, 1): exact in fp32 (a multiple of 2^-23 of magnitude <= 1)
PLA_HD float signed_unit(uint32_t w) {
#pragma clang fp contract(off)
  return 2.0f * unit_co(w) - 1.0f;
}

// the c2 = 0 words -> flip bit, rotation, scale; a stage that is off leaves its identity value, which nobody reads
PLA_HD void decide0(const Plan& p, const uint32_t w[4], Pose& o) {
#pragma clang fp contract(off)
  o.flip = p.flip_mode == 2 || (p.flip_mode == 1 && w[0] < p.thr);
  o.cs = 1.f; o.sn = 0.f; o.sc = 1.f;
  if (p.max_rot != 0.f) {
    const float theta = signed_unit(w[1]) * p.max_rot;
    sincosf(theta, &o.sn, &o.cs);
  }
  if (p.scale_range != 0.f) {
    const float d = signed_unit(w[2]) * p.scale_range;
    o.sc = 1.0f + d;
  }
}

// the c2 = 1 words -> translation
PLA_HD void decide1(const Plan& p, const uint32_t w[4], Pose& o) {
#pragma clang fp contract(off)
  o.tx = signed_unit(w[0]) * p.max_shift;
  o.ty = signed_unit(w[1]) * p.max_shift;
}

// the words of call c2 >= 2 -> the noise of output elements k = 4 (c2 - 2) .. + 3
PLA_HD void noise4(const Plan& p, const uint32_t w[4], float nz[4]) {
#pragma clang fp contract(off)
  for (int h = 0; h < 2; ++h) {
    const float r = sqrtf(-2.0f * logf(unit_oc(w[2 * h])));
    const float phi = 6.28318530717958647692f * unit_co(w[2 * h + 1]);
    float s, c;
    sincosf(phi, &s, &c);
    const float z0 = r * c, z1 = r * s;
    nz[2 * h] = p.sigma * z0;
    nz[2 * h + 1] = p.sigma * z1;
  }
}

// source joint of output joint j under flip_pose's swap
PLA_HD int flip_src_joint(int j) {
  return (j >= 1 && j <= 3) ? j + 3 : (j >= 4 && j <= 6) ? j - 3 : (j >= 11 && j <= 13) ? j + 3 : (j >= 14 && j <= 16) ? j - 3 : j;
}

// Output coordinate d (0 = x, 1 = y) of a 2-D joint.  v = that coordinate of the SOURCE joint, u = the source joint's other
// coordinate (read only when the rotation is on), nz = the output element's noise (read only when sigma != 0).
PLA_HD float elem2d(const Plan& p, const Pose& q, int d, float v, float u, float nz) {
#pragma clang fp contract(off)
  const float cv = d == 0 ? p.cx : p.cy;
  if (q.flip) {
    if (d == 0) v = p.flip_offset - v;
    else u = p.flip_offset - u;
  }
  if (p.max_rot != 0.f) {
    const float cu = d == 0 ? p.cy : p.cx;
    const float dv = v - cv, du = u - cu;
    // x' = c dx - s dy,  y' = s dx + c dy
    const float t = d == 0 ? q.cs * dv - q.sn * du : q.sn * du + q.cs * dv;
    v = t + cv;
  }
  if (p.scale_range != 0.f) v = q.sc * (v - cv) + cv;
  if (p.max_shift != 0.f) v = v + (d == 0 ? q.tx : q.ty);
  if (p.sigma != 0.f) v = v + nz;
  return v;
}

// Output coordinate d (0 = x, 1 = y; z is a copy and never comes here) of a 3-D joint; v, u as above.
PLA_HD float elem3d(const Plan& p, const Pose& q, int d, float v, float u) {
#pragma clang fp contract(off)
  if (q.flip) {
    if (d == 0) v = -v;
    else u = -u;
  }
  if (p.max_rot != 0.f) v = d == 0 ? q.cs * v - q.sn * u : q.sn * u + q.cs * v;
  return v;
}

// One whole pose, one element after the other: the host entry point, and the definition the kernel's lanes divide up.
// a [34], b [51] the source rows; oa, ob the outputs (no overlap with the sources).
PLA_HD void augment_pose(const Plan& p, uint64_t row, const float* a, const float* b, float* oa, float* ob) {
  uint32_t w[4];
  Pose q = {0, 1.f, 0.f, 1.f, 0.f, 0.f};
  if (needs_call(p, 0)) { draw(p, row, 0, w); decide0(p, w, q); }
  else q.flip = p.flip_mode == 2;
  if (needs_call(p, 1)) { draw(p, row, 1, w); decide1(p, w, q); }
  const bool rot = p.max_rot != 0.f;
  for (int k4 = 0; k4 < kWA; k4 += 4) {
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (needs_call(p, 2)) { draw(p, row, 2 + (k4 >> 2), w); noise4(p, w, nz); }
    for (int k = k4; k < k4 + 4 && k < kWA; ++k) {
      const int j = k >> 1, d = k & 1, sj = q.flip ? flip_src_joint(j) : j;
      oa[k] = elem2d(p, q, d, a[sj * 2 + d], rot ? a[sj * 2 + (d ^ 1)] : 0.f, nz[k & 3]);
    }
  }
  for (int k = 0; k < kWB; ++k) {
    const int j = k / 3, d = k - 3 * j, sj = q.flip ? flip_src_joint(j) : j;
    const float v = b[sj * 3 + d];
    ob[k] = d == 2 ? v : elem3d(p, q, d, v, rot ? b[sj * 3 + (d ^ 1)] : 0.f);
  }
}

}  // namespace pa
}  // namespace pl

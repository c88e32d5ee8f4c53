// The Gaussian heat-map target of the reference's dataset (phase3_direct/my_HybrIK/H36_dataset.py:148-194), written once
// for the device kernels and the host entry point: pl_heatmap_gaussian, pl_heatmap_gaussian_host and the fused heat-map
// loss of softargmax.hip run this text.  The target is never stored by the loss kernels: a voxel's value is a function of the
// (b, j) pair's target coordinate, evaluated where the voxel is streamed.
//
// Per axis a (0 = x <-> W, 1 = y <-> H, 2 = z <-> D; a depth-1 map has no z factor):
//   mu_a = alpha_a * (t_a + gamma_a)      the continuous centre index: an affine law of the target coordinate t_a, evaluated
//                                         in fp32 in the dataset's own order of operations (31.5 * (1 + t)), so the centre
//                                         and its rounding tie fall where the dataset's fall
//   c_a  = rint(mu_a), ties to even       (np.rint; mu = 31.5 -> 32)
//   half = size / 2, size = ceil(6 sigma) made odd
//   g    = exp(-sum_a (idx_a - mu_a)^2 / (2 sigma^2))   where |idx_a - c_a| <= half on every axis, 0 elsewhere
// Unnormalised; the window is clipped by the map simply because only the map's voxels are ever asked for.
//
// The window test is a float comparison against c_a: no centre, however far off the map or non-finite, is ever turned into an
// index.  A window wholly outside the map gives an all-zero target.  A non-finite centre makes the pair BAD (map_bad):
// its dense target, its loss and its heat-map gradient are NaN (the callers' business, one select each); the comparisons
// are false for NaN, so nothing else is evaluated for such a pair.
//
// The exponent is formed in fp64 (idx - mu is exact there, the three squares and the division lose nothing that fp32 would
// see) and handed to expf as a fp32 head and a first-order tail: the value is within a few ulps of the fp64 exp rounded to
// fp32 even at the window's corners (exponent -13.5 at sigma 0.5), where an fp32 exponent would cost 20 ulps.  Only voxels
// inside the window pay for it: 27 of 262144 at sigma 0.5.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PLH_HD __host__ __device__ inline
#else
#define PLH_HD inline
#endif

namespace pl {
namespace plh {

constexpr int kMaxHalf = 8;           // supported window: 17 voxels per axis (sigma <= 2.83)

// What a kernel needs besides the target coordinates; built on the host (heat_law_of), passed by value.
struct Law {
  float alpha[3], gamma[3];           // mu_a = alpha_a * (t_a + gamma_a)
  float half;                         // window half-width, an integer value
  double k;                           // 1 / (2 sigma^2)
};

// half-width of the reference's window for sigma, or -1 when sigma is not a positive finite number
inline int half_of_sigma(float sigma) {
  if (!(sigma > 0.f) || !(sigma < 1.0e6f)) return -1;
  int size = (int)ceil(6.0 * (double)sigma);
  if (!(size & 1)) ++size;
  return size / 2;
}

struct Map {
  float mu[3], c[3];                  // an unused axis (ncoord 2, depth 1) has mu = c = 0: index 0 is inside, its factor is 1
};

PLH_HD Map map_of(const float* t, int ncoord, int D, const Law& L) {
  Map m;
  m.mu[0] = L.alpha[0] * (t[0] + L.gamma[0]);
  m.mu[1] = L.alpha[1] * (t[1] + L.gamma[1]);
  m.mu[2] = (ncoord > 2 && D > 1) ? L.alpha[2] * (t[2] + L.gamma[2]) : 0.f;
  m.c[0] = rintf(m.mu[0]);
  m.c[1] = rintf(m.mu[1]);
  m.c[2] = rintf(m.mu[2]);
  return m;
}

PLH_HD bool finite1(float x) { return fabsf(x) <= 3.402823466e38f; }          // false for inf and NaN
PLH_HD bool map_bad(const Map& m) { return !(finite1(m.mu[0]) && finite1(m.mu[1]) && finite1(m.mu[2])); }

// index i (as a float) inside the window of an axis centred at c
PLH_HD bool in_window(float i, float c, float half) { return fabsf(i - c) <= half; }

// the value at (x, y, z) = (w, h, d) indices; the CALLER has tested the window on every axis
PLH_HD float gauss_at(const Map& m, const Law& L, float x, float y, float z) {
  const double dx = (double)x - (double)m.mu[0], dy = (double)y - (double)m.mu[1], dz = (double)z - (double)m.mu[2];
  const double e = -(dx * dx + dy * dy + dz * dz) * L.k;
  const float eh = (float)e;
  const float el = (float)(e - (double)eh);
  return expf(eh) * (1.0f + el);
}

// the target's value at a voxel of a map that is not bad: window test + value
PLH_HD float value_at(const Map& m, const Law& L, float x, float y, float z) {
  if (!(in_window(x, m.c[0], L.half) && in_window(y, m.c[1], L.half) && in_window(z, m.c[2], L.half))) return 0.f;
  return gauss_at(m, L, x, y, z);
}

}  // namespace plh
}  // namespace pl

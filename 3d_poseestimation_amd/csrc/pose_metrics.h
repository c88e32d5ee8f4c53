// Per-pose evaluation arithmetic (MPJPE, N-MPJPE, P-MPJPE), written once for the device kernel and the host entry point of
// metrics.hip: pl_pose_errors and pl_pose_errors_host run this text.
//
// One pose pair is 3J floats of prediction P and 3J floats of target T ([J][3] each).  pose_errors_one() works IN PLACE:
//   P[3j .. 3j+2] <- the Procrustes-aligned prediction  a R (P_j - muP) + muT
//   T[3j + m]     <- e_m[j], m = 0 MPJPE, 1 N-MPJPE, 2 P-MPJPE
// (joint j's three target floats are dead once its errors are known, so the errors take their place: no third buffer.)
//
// P-MPJPE by Horn's closed form (J. Opt. Soc. Am. A 4, 1987): with M = P0^T T0 of the centred poses, the best PROPER rotation
// is R(q) of the unit eigenvector q of the largest eigenvalue lambda of the symmetric 4x4 matrix N(M), and
// max tr(R M) = lambda, so the best scale is lambda / ||P0||^2.  No SVD, no determinant fix, no branch on rank; a mirrored
// prediction stays mirrored.  The eigenproblem: cyclic Jacobi, a fixed number of sweeps, every index a compile-time constant.
//
// Degenerate rules (part of the definition): sum P.P == 0 -> N-MPJPE scale 0; ||P0||^2 == 0 -> Procrustes scale 0 (a
// collapsed prediction is scored against the target's centroid; a collapsed target has M = 0, lambda = 0, scale 0, error
// 0).  The tests are `== 0` selects, so a NaN anywhere in the pose reaches every output of that pose that depends on the
// whole pose: N-MPJPE, P-MPJPE and the aligned pose.  (MPJPE is per joint: NaN at the joints that hold one.)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PLM_HD __host__ __device__ inline
#else
#define PLM_HD inline
#endif

namespace pl {
namespace plm {

constexpr int kMinJoints = 3, kMaxJoints = 32;
constexpr int kJacobiSweeps = 6;      // 4x4, quadratic convergence: converged after 4 in fp32; 6 leaves two spare

// One Jacobi rotation of the symmetric a (both triangles kept) in the (p, q) plane, accumulated into the columns of v.
template <int p, int q>
PLM_HD void jacobi_rotate(float (&a)[4][4], float (&v)[4][4]) {
  const float apq = a[p][q];
  const float theta = (a[q][q] - a[p][p]) / (2.0f * apq);
  // tan of the smaller rotation angle; theta = +-inf (or its square overflowing) gives 0, apq == 0 is no rotation
  const float tt = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.0f));
  const float t = (apq == 0.0f) ? 0.0f : tt;
  const float c = 1.0f / sqrtf(t * t + 1.0f), s = t * c, tau = s / (1.0f + c);
  a[p][p] -= t * apq;
  a[q][q] += t * apq;
  a[p][q] = a[q][p] = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != p && r != q) {
      const float arp = a[r][p], arq = a[r][q];
      a[r][p] = a[p][r] = arp - s * (arq + tau * arp);
      a[r][q] = a[q][r] = arq + s * (arp - tau * arq);
    }
    const float vrp = v[r][p], vrq = v[r][q];
    v[r][p] = vrp - s * (vrq + tau * vrp);
    v[r][q] = vrq + s * (vrp - tau * vrq);
  }
}

// Largest eigenvalue of the symmetric 4x4 a and its unit eigenvector (a is destroyed).
PLM_HD void sym4_largest(float (&a)[4][4], float (&q)[4], float& lambda) {
  float v[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[i][k] = (i == k) ? 1.0f : 0.0f;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<0, 3>(a, v);
    jacobi_rotate<1, 2>(a, v);
    jacobi_rotate<1, 3>(a, v);
    jacobi_rotate<2, 3>(a, v);
  }
  lambda = a[0][0];
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = v[i][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    const bool up = a[k][k] > lambda;       // false for NaN: column 0 stays, and it is NaN too
    lambda = up ? a[k][k] : lambda;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = up ? v[i][k] : q[i];
  }
  const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] *= inv;
}

PLM_HD void pose_errors_one(float* P, float* T, int J) {
  // Everything centred is formed from differences to joint 0 first: exact for a collapsed pose (every difference is 0, so
  // the centred pose is 0 and not round-off of a mean), and a prediction 1000 m away loses nothing to its offset.
  const float px0 = P[0], py0 = P[1], pz0 = P[2], tx0 = T[0], ty0 = T[1], tz0 = T[2];
  float pt = 0.f, pp = 0.f;
  float sp[3] = {0.f, 0.f, 0.f}, st[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < J; ++j) {
    const float px = P[3 * j], py = P[3 * j + 1], pz = P[3 * j + 2];
    const float tx = T[3 * j], ty = T[3 * j + 1], tz = T[3 * j + 2];
    pt += px * tx + py * ty + pz * tz;
    pp += px * px + py * py + pz * pz;
    sp[0] += px - px0; sp[1] += py - py0; sp[2] += pz - pz0;
    st[0] += tx - tx0; st[1] += ty - ty0; st[2] += tz - tz0;
  }
  const float s = (pp == 0.0f) ? 0.0f : pt / pp;
  const float invJ = 1.0f / (float)J;
  const float mp[3] = {sp[0] * invJ, sp[1] * invJ, sp[2] * invJ};     // centroid - joint 0
  const float mt[3] = {st[0] * invJ, st[1] * invJ, st[2] * invJ};
  float M[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  float pp0 = 0.f;
  for (int j = 0; j < J; ++j) {
    const float a[3] = {(P[3 * j] - px0) - mp[0], (P[3 * j + 1] - py0) - mp[1], (P[3 * j + 2] - pz0) - mp[2]};
    const float b[3] = {(T[3 * j] - tx0) - mt[0], (T[3 * j + 1] - ty0) - mt[1], (T[3 * j + 2] - tz0) - mt[2]};
    pp0 += a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) M[x][y] += a[x] * b[y];
  }
  float N[4][4];
  N[0][0] = M[0][0] + M[1][1] + M[2][2];
  N[1][1] = M[0][0] - M[1][1] - M[2][2];
  N[2][2] = -M[0][0] + M[1][1] - M[2][2];
  N[3][3] = -M[0][0] - M[1][1] + M[2][2];
  N[0][1] = N[1][0] = M[1][2] - M[2][1];
  N[0][2] = N[2][0] = M[2][0] - M[0][2];
  N[0][3] = N[3][0] = M[0][1] - M[1][0];
  N[1][2] = N[2][1] = M[0][1] + M[1][0];
  N[1][3] = N[3][1] = M[2][0] + M[0][2];
  N[2][3] = N[3][2] = M[1][2] + M[2][1];
  float q[4], lambda;
  sym4_largest(N, q, lambda);
  const float scale = (pp0 == 0.0f) ? 0.0f : lambda / pp0;
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  // scale * R(q), rows
  const float R[3][3] = {
      {scale * (1.0f - 2.0f * (y * y + z * z)), scale * 2.0f * (x * y - w * z), scale * 2.0f * (x * z + w * y)},
      {scale * 2.0f * (x * y + w * z), scale * (1.0f - 2.0f * (x * x + z * z)), scale * 2.0f * (y * z - w * x)},
      {scale * 2.0f * (x * z - w * y), scale * 2.0f * (y * z + w * x), scale * (1.0f - 2.0f * (x * x + y * y))}};
  const float ct[3] = {tx0 + mt[0], ty0 + mt[1], tz0 + mt[2]};        // the target's centroid
  for (int j = 0; j < J; ++j) {
    const float p[3] = {P[3 * j], P[3 * j + 1], P[3 * j + 2]};
    const float t[3] = {T[3 * j], T[3 * j + 1], T[3 * j + 2]};
    const float a[3] = {(p[0] - px0) - mp[0], (p[1] - py0) - mp[1], (p[2] - pz0) - mp[2]};
    const float b[3] = {(t[0] - tx0) - mt[0], (t[1] - ty0) - mt[1], (t[2] - tz0) - mt[2]};
    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float d0 = p[k] - t[k], d1 = s * p[k] - t[k];
      const float yk = R[k][0] * a[0] + R[k][1] * a[1] + R[k][2] * a[2];
      const float d2 = yk - b[k];
      e0 += d0 * d0; e1 += d1 * d1; e2 += d2 * d2;
      P[3 * j + k] = yk + ct[k];
    }
    T[3 * j] = sqrtf(e0);
    T[3 * j + 1] = sqrtf(e1);
    T[3 * j + 2] = sqrtf(e2);
  }
}

// The same with per-joint weights w [J] (visibility): V = {j : w_j > 0}; a weight that is not > 0 (zero, negative, NaN) is
// "not visible".  Every whole-pose sum runs over V with weight w_j, as a SELECT: an invisible joint's coordinates are not
// read into s, the centroids, M or ||P0||^2, so a NaN there reaches only that joint's own three errors and its aligned
// coordinates.  The anchor of the differences is the FIRST visible joint (joint 0 may be the missing one), which keeps both
// exactness properties above.  Errors and the aligned pose are written for every joint: an invisible one is carried by the
// transform fitted on the visible ones.  No visible joint: s = 0, a = 0, both centroids 0.  One visible joint: every
// centred visible coordinate is exactly 0, so a = 0 and that joint's P-MPJPE is 0.
// A function of its own, so pose_errors_one() above compiles to what it compiled to before this one existed.
PLM_HD void pose_errors_one_weighted(float* P, float* T, const float* w, int J) {
  int ja = -1;
  for (int j = J - 1; j >= 0; --j) ja = (w[j] > 0.0f) ? j : ja;
  const bool any = ja >= 0;
  const int jr = any ? ja : 0;
  const float px0 = any ? P[3 * jr] : 0.f, py0 = any ? P[3 * jr + 1] : 0.f, pz0 = any ? P[3 * jr + 2] : 0.f;
  const float tx0 = any ? T[3 * jr] : 0.f, ty0 = any ? T[3 * jr + 1] : 0.f, tz0 = any ? T[3 * jr + 2] : 0.f;
  float pt = 0.f, pp = 0.f, sw = 0.f;
  float sp[3] = {0.f, 0.f, 0.f}, st[3] = {0.f, 0.f, 0.f};
  for (int j = 0; j < J; ++j) {
    const float wj = w[j];
    const bool vis = wj > 0.0f;
    const float px = P[3 * j], py = P[3 * j + 1], pz = P[3 * j + 2];
    const float tx = T[3 * j], ty = T[3 * j + 1], tz = T[3 * j + 2];
    pt += vis ? wj * (px * tx + py * ty + pz * tz) : 0.f;
    pp += vis ? wj * (px * px + py * py + pz * pz) : 0.f;
    sw += vis ? wj : 0.f;
    sp[0] += vis ? wj * (px - px0) : 0.f; sp[1] += vis ? wj * (py - py0) : 0.f; sp[2] += vis ? wj * (pz - pz0) : 0.f;
    st[0] += vis ? wj * (tx - tx0) : 0.f; st[1] += vis ? wj * (ty - ty0) : 0.f; st[2] += vis ? wj * (tz - tz0) : 0.f;
  }
  const float s = (pp == 0.0f) ? 0.0f : pt / pp;
  const float invW = any ? 1.0f / sw : 0.0f;
  const float mp[3] = {sp[0] * invW, sp[1] * invW, sp[2] * invW};     // weighted centroid - anchor
  const float mt[3] = {st[0] * invW, st[1] * invW, st[2] * invW};
  float M[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
  float pp0 = 0.f;
  for (int j = 0; j < J; ++j) {
    const float wj = w[j];
    const bool vis = wj > 0.0f;
    const float a[3] = {(P[3 * j] - px0) - mp[0], (P[3 * j + 1] - py0) - mp[1], (P[3 * j + 2] - pz0) - mp[2]};
    const float b[3] = {(T[3 * j] - tx0) - mt[0], (T[3 * j + 1] - ty0) - mt[1], (T[3 * j + 2] - tz0) - mt[2]};
    pp0 += vis ? wj * (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]) : 0.f;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
      const float wa = wj * a[x];
#pragma unroll
      for (int y = 0; y < 3; ++y) M[x][y] += vis ? wa * b[y] : 0.f;
    }
  }
  float N[4][4];
  N[0][0] = M[0][0] + M[1][1] + M[2][2];
  N[1][1] = M[0][0] - M[1][1] - M[2][2];
  N[2][2] = -M[0][0] + M[1][1] - M[2][2];
  N[3][3] = -M[0][0] - M[1][1] + M[2][2];
  N[0][1] = N[1][0] = M[1][2] - M[2][1];
  N[0][2] = N[2][0] = M[2][0] - M[0][2];
  N[0][3] = N[3][0] = M[0][1] - M[1][0];
  N[1][2] = N[2][1] = M[0][1] + M[1][0];
  N[1][3] = N[3][1] = M[2][0] + M[0][2];
  N[2][3] = N[3][2] = M[1][2] + M[2][1];
  float q[4], lambda;
  sym4_largest(N, q, lambda);
  const float scale = (pp0 == 0.0f) ? 0.0f : lambda / pp0;
  const float qw = q[0], x = q[1], y = q[2], z = q[3];
  // scale * R(q), rows
  const float R[3][3] = {
      {scale * (1.0f - 2.0f * (y * y + z * z)), scale * 2.0f * (x * y - qw * z), scale * 2.0f * (x * z + qw * y)},
      {scale * 2.0f * (x * y + qw * z), scale * (1.0f - 2.0f * (x * x + z * z)), scale * 2.0f * (y * z - qw * x)},
      {scale * 2.0f * (x * z - qw * y), scale * 2.0f * (y * z + qw * x), scale * (1.0f - 2.0f * (x * x + y * y))}};
  const float ct[3] = {tx0 + mt[0], ty0 + mt[1], tz0 + mt[2]};        // the target's weighted centroid
  for (int j = 0; j < J; ++j) {
    const float p[3] = {P[3 * j], P[3 * j + 1], P[3 * j + 2]};
    const float t[3] = {T[3 * j], T[3 * j + 1], T[3 * j + 2]};
    const float a[3] = {(p[0] - px0) - mp[0], (p[1] - py0) - mp[1], (p[2] - pz0) - mp[2]};
    const float b[3] = {(t[0] - tx0) - mt[0], (t[1] - ty0) - mt[1], (t[2] - tz0) - mt[2]};
    float e0 = 0.f, e1 = 0.f, e2 = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float d0 = p[k] - t[k], d1 = s * p[k] - t[k];
      const float yk = R[k][0] * a[0] + R[k][1] * a[1] + R[k][2] * a[2];
      const float d2 = yk - b[k];
      e0 += d0 * d0; e1 += d1 * d1; e2 += d2 * d2;
      P[3 * j + k] = yk + ct[k];
    }
    T[3 * j] = sqrtf(e0);
    T[3 * j + 1] = sqrtf(e1);
    T[3 * j + 2] = sqrtf(e2);
  }
}

}  // namespace plm
}  // namespace pl

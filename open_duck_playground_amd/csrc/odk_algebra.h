// odk_algebra.h -- per-lane arithmetic, no cross-lane traffic and no model: the numerical constants, 3-vector / quaternion / spatial
// 6-vector algebra, the manifold's area measure (area0, AREA_TIE: shared by odk_convex.h and the contact routines), and the threefry RNG.
// Bottom layer: stands on the HIP runtime header alone.
#pragma once
#include <hip/hip_runtime.h>

namespace odk {

constexpr float MINVAL_F = 1e-15f;
constexpr float PI_F = 3.14159265358979323846f;

__device__ __forceinline__ void cross3(float* r, const float* a, const float* b) {
  float x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z;
}
__device__ __forceinline__ float dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void qmul(float* r, const float* a, const float* b) {
  float w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  float x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  float y = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
  float z = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}
__device__ __forceinline__ void qnormalize(float* q) {   // v_rsq_f32 (1 ulp) instead of IEEE sqrt + division (~20 instructions)
  const float n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (n2 < MINVAL_F * MINVAL_F) { q[0] = 1; q[1] = q[2] = q[3] = 0; return; }
  const float inv = __builtin_amdgcn_rsqf(n2);
  q[0] *= inv; q[1] *= inv; q[2] *= inv; q[3] *= inv;
}
__device__ __forceinline__ void qrot(float* r, const float* q, const float* v) {  // r = R(q) v
  float t[3], u[3] = {q[1], q[2], q[3]}, c[3];
  cross3(t, u, v);
  t[0] *= 2; t[1] *= 2; t[2] *= 2;
  cross3(c, u, t);
  r[0] = v[0] + q[0] * t[0] + c[0]; r[1] = v[1] + q[0] * t[1] + c[1]; r[2] = v[2] + q[0] * t[2] + c[2];
}
__device__ __forceinline__ void q2mat(float* m, const float* q) {
  float w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = w * w + x * x - y * y - z * z; m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = w * w - x * x + y * y - z * z; m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = w * w - x * x - y * y + z * z;
}
// spatial inertia (10: Ixx Iyy Izz Ixy Ixz Iyz mcx mcy mcz m) times motion [ang; lin] (mju_mulInertVec)
__device__ __forceinline__ void inert_mul(float* res, const float* i, const float* v) {
  res[0] = i[0] * v[0] + i[3] * v[1] + i[4] * v[2] - i[8] * v[4] + i[7] * v[5];
  res[1] = i[3] * v[0] + i[1] * v[1] + i[5] * v[2] + i[8] * v[3] - i[6] * v[5];
  res[2] = i[4] * v[0] + i[5] * v[1] + i[2] * v[2] - i[7] * v[3] + i[6] * v[4];
  res[3] = i[8] * v[1] - i[7] * v[2] + i[9] * v[3];
  res[4] = i[6] * v[2] - i[8] * v[0] + i[9] * v[4];
  res[5] = i[7] * v[0] - i[6] * v[1] + i[9] * v[5];
}
__device__ __forceinline__ void cross_motion(float* res, const float* vel, const float* v) {  // mju_crossMotion
  float a[3], b[3];
  cross3(res, vel, v);
  cross3(a, vel, v + 3);
  cross3(b, vel + 3, v);
  res[3] = a[0] + b[0]; res[4] = a[1] + b[1]; res[5] = a[2] + b[2];
}

// area measures below 1e-7 m^2 count as zero (oracle manifold_points AREA0: collinear / coincident candidates tie like in exact
// arithmetic instead of by rounding residue)
__device__ __forceinline__ float area0(float v) { return v < 1e-7f ? 0.0f : v; }
// last manifold point: values within AREA_TIE of the maximum count as the maximum, the lowest index wins (oracle manifold_points)
constexpr float AREA_TIE = 1e-7f;

// ---- RNG: threefry2x32-20, stream definition shared with oracle/odk_oracle_env.c
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ inline void threefry2x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t& o0, uint32_t& o1) {
  const int R[8] = {13, 15, 26, 6, 17, 29, 16, 24};
  uint32_t ks[3] = {k0, k1, 0x1BD11BDAu ^ k0 ^ k1};
  uint32_t x0 = c0 + ks[0], x1 = c1 + ks[1];
#pragma unroll
  for (int blk = 0; blk < 5; blk++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      x0 += x1;
      x1 = rotl32(x1, R[(blk & 1) * 4 + r]);
      x1 ^= x0;
    }
    x0 += ks[(blk + 1) % 3];
    x1 += ks[(blk + 2) % 3] + (uint32_t)(blk + 1);
  }
  o0 = x0; o1 = x1;
}
__device__ inline float rng_uniform(uint32_t k0, uint32_t k1, uint32_t ctr, uint32_t idx) {
  uint32_t a, b;
  threefry2x32(k0, k1, ctr, idx >> 1, a, b);
  return (float)(((idx & 1) ? b : a) >> 8) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ int randint3(float u) { int i = (int)(u * 3.0f); return i > 2 ? 2 : i; }

}  // namespace odk

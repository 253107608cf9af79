// Train-BatchNorm arithmetic shared by the two-launch kernels (bn_train.hip)
// and the one-launch kernels (bn_onepass.hip).
//
// Both families must give the same bits, so every floating-point expression
// of the per-channel chain lives here once and both compile from this text:
// the stripe accumulation, the statistics, the running-stat update, the
// normalisation and the dx formula.  Summation ORDER is the callers' job and
// is described at bn_nslab().
#pragma once

#include "common.h"

namespace flreid {

constexpr int BN_STRIPES = 16;   // row stripes per slab
constexpr int BN_CG = 64;        // channels per block of the two-launch pair

// Row slabs of the reduction.  Stripe g = slab·16 + r sums rows g, g+S, …
// (S = nslab·16) in row order; a slab sums its 16 stripes in order from 0.f;
// the total sums the slabs in order from 0.f.
inline int bn_nslab(int64_t M, int C) {
  // target ≈256 blocks (one wave over the 8 XCDs); never more slabs than
  // 16-row stripes available
  const int cg = C / BN_CG;
  int ns = 256 / cg;
  const int max_rows = (int)((M + BN_STRIPES - 1) / BN_STRIPES);
  if (ns > max_rows) ns = max_rows;
  if (ns > 64) ns = 64;
  if (ns < 1) ns = 1;
  return ns;
}

__device__ __forceinline__ void bn_unpack4(const ushort4 t, float v[4]) {
  v[0] = __bfloat162float(*(const __hip_bfloat16*)&t.x);
  v[1] = __bfloat162float(*(const __hip_bfloat16*)&t.y);
  v[2] = __bfloat162float(*(const __hip_bfloat16*)&t.z);
  v[3] = __bfloat162float(*(const __hip_bfloat16*)&t.w);
}

template <typename T>
__device__ __forceinline__ void bn_load4(const T* p, float v[4]);

template <>
__device__ __forceinline__ void bn_load4<float>(const float* p, float v[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

template <>
__device__ __forceinline__ void bn_load4<__hip_bfloat16>(
    const __hip_bfloat16* p, float v[4]) {
  bn_unpack4(*reinterpret_cast<const ushort4*>(p), v);
}

template <typename T>
__device__ __forceinline__ void bn_store4(T* p, const float v[4]);

template <>
__device__ __forceinline__ void bn_store4<float>(float* p, const float v[4]) {
  *reinterpret_cast<float4*>(p) = float4{v[0], v[1], v[2], v[3]};
}

template <>
__device__ __forceinline__ void bn_store4<__hip_bfloat16>(
    __hip_bfloat16* p, const float v[4]) {
  ushort4 t;
  __hip_bfloat16 b;
  b = __float2bfloat16(v[0]); t.x = *(const unsigned short*)&b;
  b = __float2bfloat16(v[1]); t.y = *(const unsigned short*)&b;
  b = __float2bfloat16(v[2]); t.z = *(const unsigned short*)&b;
  b = __float2bfloat16(v[3]); t.w = *(const unsigned short*)&b;
  *reinterpret_cast<ushort4*>(p) = t;
}

// ---- arithmetic ------------------------------------------------------------
// Which multiply feeds a fused multiply-add decides the last bit, and left to
// the compiler that choice moves with the surrounding code and the build
// flags.  So contraction is off in these helpers and every fma is written
// out, in the form the two-launch kernels have always compiled to (the
// running-stat update has none).

__device__ __forceinline__ void bn_fwd_accum(float& sa, float& sb, float x) {
#pragma clang fp contract(off)
  sa = sa + x;
  sb = __builtin_fmaf(x, x, sb);
}

// the fused ReLU zeroed this element's output (its dy is masked)
__device__ __forceinline__ bool bn_relu_off(float x, float sc, float sh) {
  return __builtin_fmaf(x, sc, sh) <= 0.f;
}

__device__ __forceinline__ void bn_bwd_accum(float& sa, float& sb, float dy,
                                             float x, float mn, float iv) {
#pragma clang fp contract(off)
  sa = sa + dy;
  const float t = dy * (x - mn);
  sb = __builtin_fmaf(t, iv, sb);
}

// ---- per-channel scalar chain ----------------------------------------------
__device__ __forceinline__ void bn_fwd_stats(float ta, float tb, int64_t M,
                                             float eps, float& mean,
                                             float& var, float& inv) {
#pragma clang fp contract(off)
  const float inv_m = 1.f / (float)M;
  mean = ta * inv_m;
  const float ex2 = tb * inv_m;
  var = fmaxf(__builtin_fmaf(-mean, mean, ex2), 0.f);
  inv = rsqrtf(var + eps);
}

__device__ __forceinline__ void bn_running_update(float& rmean, float& rvar,
                                                  float momentum, float mean,
                                                  float var, float unbiased) {
#pragma clang fp contract(off)
  const float keep = 1.f - momentum;
  const float a = keep * rmean;
  const float b = momentum * mean;
  rmean = a + b;
  const float c = keep * rvar;
  const float d = momentum * var * unbiased;
  rvar = c + d;
}

__device__ __forceinline__ void bn_scale_shift(float gamma, float beta,
                                               float mean, float inv,
                                               float& scale, float& shift) {
#pragma clang fp contract(off)
  scale = gamma * inv;
  shift = __builtin_fmaf(-mean, scale, beta);
}

__device__ __forceinline__ float bn_normalize(float v, float scale,
                                              float shift, int relu) {
  v = __builtin_fmaf(v, scale, shift);
  if (relu) v = fmaxf(v, 0.f);
  return v;
}

// ---- residual epilogue -----------------------------------------------------
// relu(bn(x) + res) as the three-kernel chain forms it: the BN output rounded
// to bf16, the add in fp32 rounded to bf16, the ReLU last.
__device__ __forceinline__ float bn_round_bf16(float v) {
  return __bfloat162float(__float2bfloat16(v));
}

__device__ __forceinline__ float bn_add_relu(float y, float res) {
#pragma clang fp contract(off)
  const float z = bn_round_bf16(bn_round_bf16(y) + res);
  return fmaxf(z, 0.f);
}

// threshold_backward on raw bf16 quads: dz where z > 0, +0 where z <= 0
__device__ __forceinline__ ushort4 bn_relu_mask4(const ushort4 dz,
                                                 const ushort4 z) {
  float zf[4];
  bn_unpack4(z, zf);
  ushort4 d;
  d.x = zf[0] <= 0.f ? (unsigned short)0 : dz.x;
  d.y = zf[1] <= 0.f ? (unsigned short)0 : dz.y;
  d.z = zf[2] <= 0.f ? (unsigned short)0 : dz.z;
  d.w = zf[3] <= 0.f ? (unsigned short)0 : dz.w;
  return d;
}

// Σ/M of the two backward sums
__device__ __forceinline__ void bn_bwd_means(float tdy, float tdyx, int64_t M,
                                             float& mdy, float& mdyx) {
#pragma clang fp contract(off)
  const float inv_m = 1.f / (float)M;
  mdy = tdy * inv_m;
  mdyx = tdyx * inv_m;
}

// dx = γ·invstd·(d − Σdy/M − x̂·Σ(dy·x̂)/M), d = dy or 0 under the ReLU mask
__device__ __forceinline__ float bn_bwd_dx(float x, float dy, float mn,
                                           float iv, float g_iv, float sh,
                                           float mdy, float mdyx, int relu) {
#pragma clang fp contract(off)
  const float xhat = (x - mn) * iv;
  float d = dy;
  if (relu && bn_relu_off(x, g_iv, sh)) d = 0.f;
  const float e = d - mdy;
  return g_iv * __builtin_fmaf(-xhat, mdyx, e);
}

}  // namespace flreid

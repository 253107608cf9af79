// Device helpers shared by the two MFMA window-attention files for windows of
// up to 64 tokens (window_attn_qkv.hip: rows of a [BW][N][3·C] tensor;
// window_attn_map.hip: rows of the [B][Hi][Wi][3·C] feature map): fragment
// types, the transposed LDS copies, the strip products and the bias loads.
// What differs between the two, how a token's row is found and where the
// shift mask comes from, stays in each file.  The design is described at the
// top of window_attn_qkv.hip.
#pragma once

#include "common.h"

namespace flreid {
namespace wq {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;
using u16x4 = __attribute__((ext_vector_type(4))) unsigned short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int WQ_D = 32;        // head dim
// Windows per backward workgroup (two per wave).  One [N][N] fp32 partial
// per run keeps the partials at 1/8 of a full dS tensor.  Stage 0 of
// swin-tiny at batch 64 (BW = 4096, H = 3) gives 1536 workgroups, six per
// CU of a 256-CU part; stage 2 (BW = 256, H = 12) still 384 and stage 3
// (BW = 64, H = 24) 192, where 16 would leave a third of the CUs idle.
constexpr int WQ_GROUP = 8;

// transposed [d][token] row stride in elements: NT rounded up to even tiles
// plus 8 (20 or 36 dwords: the 16 rows of an 8-byte read land apart)
constexpr int wq_ts(int NT) { return 32 * ((NT + 1) / 2) + 8; }

// LDS of one backward wave in elements: two transposed copies and the
// 3 × 64 fp32 row statistics
constexpr int wq_bwd_wave_elems(int NT) { return 2 * WQ_D * wq_ts(NT) + 384; }

// round-to-nearest-even; every value rounded here is finite
__device__ __forceinline__ unsigned short wq_bf16(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

__device__ __forceinline__ f32x4 wq_mfma(u16x8 a, u16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
      0);
}

// Orders this wave's LDS traffic: what other lanes wrote before is visible
// after.  No instruction — a wave's LDS operations complete in order — but
// the compiler may not move LDS accesses across it.
__device__ __forceinline__ void wq_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// base + a 32-bit BYTE offset: with a wave-uniform base this is one scalar
// register pair, one offset register and an immediate; an element index
// would be widened to a 64-bit address per access, and the compiler keeps
// those across the loops.
template <typename T>
__device__ __forceinline__ T* wq_at(T* base, int elems) {
  return (T*)((char*)base + (unsigned)(elems * (int)sizeof(T)));
}
template <typename T>
__device__ __forceinline__ const T* wq_at(const T* base, int elems) {
  return (const T*)((const char*)base + (unsigned)(elems * (int)sizeof(T)));
}

// A wave-uniform index the optimiser cannot see through.  The backward
// forms its bases from such indices once per window: otherwise every address
// of the window loop is hoisted out of it as a 64-bit register pair.
__device__ __forceinline__ int wq_opaque(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

// lT[d][token] = the matrix whose fragments are f; the tile past an odd NT
// is written as zeros (its partner operand is zero, but 0·NaN is not).
template <int NT>
__device__ __forceinline__ void wq_put_transposed(unsigned short* lT,
                                                  const u16x8 (&f)[NT],
                                                  int lane) {
  constexpr int NTE = 2 * ((NT + 1) / 2), TS = wq_ts(NT);
  const int fr = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int t = 0; t < NTE; ++t) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      lT[(kg * 8 + e) * TS + t * 16 + fr] =
          t < NT ? f[t][e] : (unsigned short)0;
    }
  }
}

// p[row / N][j0..j0+3] of an [N][N] fp32 matrix, row = N·min(i, N − 1).
// Branch-free: in the last key tile (`last`) a key past the matrix is clamped
// into it, and the caller discards what such an element returns.  Four
// dword loads whatever N is: N = 49 allows no wider one.
__device__ __forceinline__ f32x4 wq_load4(const float* __restrict__ p, int row,
                                          int j0, int N, bool last) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[e] = *wq_at(p, row + (last ? min(j0 + e, N - 1) : j0 + e));
  }
  return r;
}

// p[i0 + r][j], r = 0..3, both indices clamped into the matrix
__device__ __forceinline__ f32x4 wq_load_col(const float* __restrict__ p,
                                             int i0, int j, int N) {
  f32x4 r;
  const int jc = min(j, N - 1);
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = *wq_at(p, min(i0 + e, N - 1) * N + jc);
  return r;
}

__device__ __forceinline__ void wq_store4(float* __restrict__ p, int i, int j0,
                                          int N, bool vec4, f32x4 v) {
  if (i < N && j0 < N) {
    float* q = wq_at(p, i * N + j0);
    if (vec4) {
      *(f32x4*)q = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (j0 + e < N) q[e] = v[e];
      }
    }
  }
}

// Xᵀ[d][x] = Σ_c Mᵀ[d][c]·W[x][c] for this lane's x (lane & 15), the
// contraction index c running over NT tiles of 16; W is given as bf16 bits,
// w[ct][r] = W[x][16·ct + 4·kg + r]; mT is the transposed copy of M
// ([32][wq_ts(NT)]).  Returns the two d tiles: out[dt][r] is d = 16·dt +
// 4·kg + r.
template <int NT>
__device__ __forceinline__ void wq_strip_times(const u16x4 (&w)[NT],
                                               const unsigned short* mT,
                                               int lane, f32x4 (&out)[2]) {
  constexpr int TS = wq_ts(NT);
  const int fr = lane & 15, kg = lane >> 4;
  out[0] = f32x4{0.f, 0.f, 0.f, 0.f};
  out[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < (NT + 1) / 2; ++u) {
    const u16x4 lo = w[2 * u];
    u16x4 hi = {0, 0, 0, 0};                 // the zero tile of an odd NT
    if (2 * u + 1 < NT) hi = w[2 * u + 1];
    const u16x8 wf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const unsigned short* row = mT + (dt * 16 + fr) * TS + kg * 4;
      const u16x4 a0 = *(const u16x4*)(row + (2 * u) * 16);
      const u16x4 a1 = *(const u16x4*)(row + (2 * u + 1) * 16);
      const u16x8 af = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      out[dt] = wq_mfma(af, wf, out[dt]);
    }
  }
}

}  // namespace wq
}  // namespace flreid

// MFMA Swin window attention for windows of 65..144 tokens (ws 9..12),
// head dim 32, bf16 — forward and backward.  window_attn.hip (VALU, fp32
// LDS) keeps N <= 64; its [N][N+1] fp32 score array does not fit at N = 144.
//
//   S = scale·Q·Kᵀ + bias[h] (+ mask[bw % nW]),  P = softmax_rows(S),  O = P·V
//   dV = Pᵀ·dO, dP = dO·Vᵀ, dS = P∘(dP − rowsum(dP∘P)),
//   dQ = scale·dS·K, dK = scale·dSᵀ·Q, dbias = Σ_windows dS
//
// Design (v_mfma_f32_16x16x32_bf16 throughout; NT = ⌈N/16⌉ tiles, a kernel
// instance per NT = 5..9 so every tile loop unrolls into registers):
//  - one workgroup of 4 waves per (window, head).  Q, K (V, dO) are staged
//    once into LDS as bf16 rows of 40 elements (80 B = 20 dwords: the 16
//    rows of a 16-byte fragment read land on 16 distinct 4-bank groups);
//    rows N..16·NT−1 are zero.
//  - a wave owns query tiles qt = wave, wave+4, (wave+8) and computes the
//    TRANSPOSED strip Sᵀ = K·Qᵀ, one MFMA per 16×16 tile (D = 32 is one
//    instruction).  The accumulator layout then gives each lane ONE query
//    (lane & 15) and, per key tile, the 4 keys 4·(lane >> 4) + r: scale,
//    bias and mask are applied in fp32 on the accumulators (float4 reads
//    from L2 when N % 4 == 0), keys >= N are −inf, and the row max / sum are
//    an in-lane reduction plus two shuffles (xor 16, 32).  No [N][N] array.
//  - P·V contracts over keys.  Two key tiles (2u, 2u+1) of one lane are the
//    8 values an MFMA operand wants, so P is rounded to bf16 in registers
//    and fed straight back as the B operand; the contraction index is
//    thereby permuted (slot (kg, e) = key 16·(2u + e/4) + 4·kg + e%4), and
//    V is read with the same permutation from a TRANSPOSED copy Vᵀ[d][key]
//    (two 8-byte reads; row stride 168 = 84 dwords).  P never touches LDS.
//    An odd NT pairs its last tile with a zero tile (Vᵀ is zero to key 160).
//    The result tile is Oᵀ: a lane holds one query and 4 consecutive d, an
//    8-byte store.  dQ = scale·dS·K takes the same route with Kᵀ.
//  - 9 query tiles over 4 waves is 3/2/2/2.  Accepted: a finer split would
//    break "one lane = one query row", which is what keeps the softmax and
//    the P operand in registers.
//  - backward: dPᵀ = V·dOᵀ shares the Sᵀ layout, so dS is formed in fp32
//    registers.  dV and dK contract over QUERIES, which a lane has one of:
//    P and dS are rounded to bf16 once (the same rounded dS feeds dQ) and
//    written to two LDS tiles [key][query] (row stride 144 = 72 dwords);
//    after a barrier the 2·NT (dV | dK, key tile) units are dealt over the
//    waves, reading Qᵀ / dOᵀ [d][query] copies.  A chunk of 32 queries
//    past 16·NT uses a zero operand.
//  - bias gradient: a workgroup walks a run of WM_GROUP = 8 consecutive
//    windows of one head and keeps the fp32, unrounded dS sum in registers
//    (dsacc, 27 float4 on wave 0); it writes one [N][N] partial, the
//    wrapper sums the [⌈BW/8⌉, H, N, N] partials.  No atomics, no
//    [BW,H,N,N] tensor.
//  - P is recomputed in the backward (no saved log-sum-exp: the max / sum
//    is two shuffles here).
//
// Resources, from the compiler's resource summary (hipcc -O3, gfx950,
// packed fp32 off), smallest and largest instance:
//   fwd NT = 5: 128 VGPRs + 20 AGPRs, no spill, 23 552 B static LDS
//   fwd NT = 9: 208 VGPRs + 36 AGPRs, no spill, 33 792 B static LDS
//               (2 waves / SIMD)
//   bwd NT = 5: 256 VGPRs + 40 AGPRs, no spill, 102 656 B dynamic LDS
//   bwd NT = 9: 256 VGPRs + 256 AGPRs, 95 VGPRs spilled (384 B scratch per
//               lane), 161 280 B dynamic LDS
// The backward runs one workgroup per CU (LDS) and needs the raised
// dynamic-LDS attribute.  Its NT = 9 instance holds 27 float4 of dsacc next
// to a strip's S, dP, bias and mask quads; NT <= 8 does not spill.

#include "common.h"
#include "ops.h"

#include <initializer_list>

namespace flreid {

namespace {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;
using u16x4 = __attribute__((ext_vector_type(4))) unsigned short;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int WM_D = 32;        // head dim
constexpr int WM_RS = 40;       // row-major LDS row stride (elements)
constexpr int WM_TS = 168;      // transposed [d][token] row stride
constexpr int WM_TCOLS = 160;   // transposed columns written (zero past N)
constexpr int WM_PS = 144;      // P / dS tile [key][query] row stride
constexpr int WM_GROUP = 8;     // windows per backward workgroup

// round-to-nearest-even; every value rounded here is finite
__device__ __forceinline__ unsigned short wm_bf16(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}

__device__ __forceinline__ f32x4 wm_mfma(u16x8 a, u16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      __builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
      0);
}

// p[row / N][j0..j0+3] of an [N][N] fp32 matrix, row = N·min(i, N − 1).
// Branch-free: in the last key tile (`last`) a key past the matrix is clamped
// into it, and the caller discards what such an element returns (keys >= N
// become -inf, queries >= N get probability zero).  p is wave-uniform and
// the offset 32-bit: one scalar base, one offset register, an immediate.
__device__ __forceinline__ f32x4 wm_load4(const float* __restrict__ p, int row,
                                          int j0, int N, bool vec4,
                                          bool last) {
  if (vec4) return *(const f32x4*)(p + (row + (last ? min(j0, N - 4) : j0)));
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    r[e] = p[row + (last ? min(j0 + e, N - 1) : j0 + e)];
  }
  return r;
}

__device__ __forceinline__ void wm_store4(float* __restrict__ p, int i, int j0,
                                          int N, bool vec4, f32x4 v) {
  if (i < N && j0 < N) {
    float* q = p + (int64_t)i * N + j0;
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

// One 16-byte chunk (8 bf16 of row `row`, d = 8·part..) of a [N][32] matrix
// into the row-major copy (rows < NP) and / or the transposed copy
// (columns < WM_TCOLS); rows >= N are zero.
template <int NP, bool ROWMAJOR, bool TRANSPOSED>
__device__ __forceinline__ void wm_stage(const __hip_bfloat16* __restrict__ g,
                                         unsigned short* lrow,
                                         unsigned short* ltr, int N, int tid) {
  for (int c = tid; c < WM_TCOLS * 4; c += 256) {
    const int row = c >> 2, part = c & 3;
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < N) v = *(const u16x8*)(g + (int64_t)c * 8);
    if (ROWMAJOR && row < NP) *(u16x8*)(lrow + row * WM_RS + part * 8) = v;
    if (TRANSPOSED) {
#pragma unroll
      for (int e = 0; e < 8; ++e) ltr[(part * 8 + e) * WM_TS + row] = v[e];
    }
  }
}

// The normalised probabilities of query tile qt, transposed-strip layout:
// p[kt][r] = P[i][kt·16 + 4·kg + r], i = qt·16 + (lane & 15); zero for
// i >= N or key >= N.
template <int NT>
__device__ __forceinline__ void wm_probs(const unsigned short* lq,
                                         const unsigned short* lk,
                                         const float* __restrict__ brow,
                                         const float* __restrict__ mrow, int N,
                                         int qt, int lane, float scale,
                                         bool vec4, f32x4 (&p)[NT]) {
  const int fr = lane & 15, kg = lane >> 4;
  const int i = qt * 16 + fr;
  const u16x8 qf = *(const u16x8*)(lq + i * WM_RS + kg * 8);
  const int row = min(i, N - 1) * N;
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    const u16x8 kf = *(const u16x8*)(lk + (kt * 16 + fr) * WM_RS + kg * 8);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 acc = wm_mfma(kf, qf, zero);
    const int j0 = kt * 16 + kg * 4;
    const f32x4 b = wm_load4(brow, row, j0, N, vec4, kt == NT - 1);
    f32x4 mk = {0.f, 0.f, 0.f, 0.f};
    if (mrow) mk = wm_load4(mrow, row, j0, N, vec4, kt == NT - 1);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = acc[r] * scale + b[r];
      s += mk[r];
      s = (j0 + r < N) ? s : -INFINITY;
      p[kt][r] = s;
      m = fmaxf(m, s);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float se = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __expf(p[kt][r] - m);
      p[kt][r] = e;
      se += e;
    }
  }
  se += __shfl_xor(se, 16, 64);
  se += __shfl_xor(se, 32, 64);
  const float inv = (i < N) ? 1.0f / se : 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[kt][r] *= inv;
  }
}

// Xᵀ[d][i] = Σ_key Mᵀ[d][key]·W[i][key] for this lane's query tile, W given
// as bf16 bits in the strip layout (w[kt][r]); mT is the transposed copy of
// M ([32][WM_TS]).  Returns the two d tiles: out[dt][r] is d = 16·dt +
// 4·kg + r of query (lane & 15).
template <int NT>
__device__ __forceinline__ void wm_strip_times(const u16x4 (&w)[NT],
                                               const unsigned short* mT,
                                               int lane, f32x4 (&out)[2]) {
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
      const unsigned short* row = mT + (dt * 16 + fr) * WM_TS + kg * 4;
      const u16x4 a0 = *(const u16x4*)(row + (2 * u) * 16);
      const u16x4 a1 = *(const u16x4*)(row + (2 * u + 1) * 16);
      const u16x8 af = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      out[dt] = wm_mfma(af, wf, out[dt]);
    }
  }
}

// out[dt][0..3] · mul -> G[i][16·dt + 4·kg ..] as bf16 (8-byte stores)
__device__ __forceinline__ void wm_store_rows(__hip_bfloat16* __restrict__ g,
                                              int i, int N, int kg,
                                              const f32x4 (&out)[2],
                                              float mul) {
  if (i >= N) return;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    u16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = wm_bf16(out[dt][r] * mul);
    *(u16x4*)(g + (int64_t)i * WM_D + dt * 16 + kg * 4) = o;
  }
}

template <int NT>
__global__ __launch_bounds__(256) void window_attn_mfma_fwd_kernel(
    const __hip_bfloat16* __restrict__ Q, const __hip_bfloat16* __restrict__ K,
    const __hip_bfloat16* __restrict__ V, const float* __restrict__ bias,
    const float* __restrict__ mask, __hip_bfloat16* __restrict__ O, int H,
    int N, int nW, float scale) {
  constexpr int NP = NT * 16;
  __shared__ __attribute__((aligned(16))) unsigned short lq[NP * WM_RS];
  __shared__ __attribute__((aligned(16))) unsigned short lk[NP * WM_RS];
  __shared__ __attribute__((aligned(16))) unsigned short lvT[WM_D * WM_TS];

  const int64_t wh = blockIdx.x;
  const int64_t bw = wh / H;
  const int h = (int)(wh % H);
  const int64_t base = wh * (int64_t)N * WM_D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  wm_stage<NP, true, false>(Q + base, lq, nullptr, N, tid);
  wm_stage<NP, true, false>(K + base, lk, nullptr, N, tid);
  wm_stage<NP, false, true>(V + base, nullptr, lvT, N, tid);
  __syncthreads();

  const float* brow = bias + (int64_t)h * N * N;
  const float* mrow = mask ? mask + (int64_t)(bw % nW) * N * N : nullptr;
  const bool vec4 = (N & 3) == 0;

#pragma unroll 1
  for (int qt = wave; qt < NT; qt += 4) {
    f32x4 p[NT];
    wm_probs<NT>(lq, lk, brow, mrow, N, qt, lane, scale, vec4, p);
    u16x4 pb[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pb[kt][r] = wm_bf16(p[kt][r]);
    }
    f32x4 o[2];
    wm_strip_times<NT>(pb, lvT, lane, o);
    wm_store_rows(O + base, qt * 16 + (lane & 15), N, lane >> 4, o, 1.0f);
  }
}

// dynamic LDS of the backward, in elements (unsigned short)
constexpr int wm_bwd_lds_elems(int NT) {
  return 4 * NT * 16 * WM_RS + 3 * WM_D * WM_TS + 2 * NT * 16 * WM_PS;
}

template <int NT>
__global__ __launch_bounds__(256) void window_attn_mfma_bwd_kernel(
    const __hip_bfloat16* __restrict__ Q, const __hip_bfloat16* __restrict__ K,
    const __hip_bfloat16* __restrict__ V, const float* __restrict__ bias,
    const float* __restrict__ mask, const __hip_bfloat16* __restrict__ DO,
    __hip_bfloat16* __restrict__ DQ, __hip_bfloat16* __restrict__ DK,
    __hip_bfloat16* __restrict__ DV, float* __restrict__ DBP, int64_t BW,
    int H, int N, int nW, float scale) {
  constexpr int NP = NT * 16;
  constexpr int NS = (NT + 3) / 4;          // query tiles of wave 0
  constexpr int NC = (NP + 31) / 32;        // 32-query contraction chunks
  extern __shared__ __attribute__((aligned(16))) unsigned char wm_smem[];
  unsigned short* lq = (unsigned short*)wm_smem;
  unsigned short* lk = lq + NP * WM_RS;
  unsigned short* lv = lk + NP * WM_RS;
  unsigned short* ldo = lv + NP * WM_RS;
  unsigned short* lqT = ldo + NP * WM_RS;
  unsigned short* lkT = lqT + WM_D * WM_TS;
  unsigned short* ldoT = lkT + WM_D * WM_TS;
  unsigned short* lp = ldoT + WM_D * WM_TS;   // bf16 P  [key][query]
  unsigned short* lds = lp + NP * WM_PS;      // bf16 dS [key][query]

  const int h = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, kg = lane >> 4;
  const float* brow = bias + (int64_t)h * N * N;
  const bool vec4 = (N & 3) == 0;

  f32x4 dsacc[NS][NT];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) dsacc[s][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int g = 0; g < WM_GROUP; ++g) {
    const int64_t bw = (int64_t)blockIdx.x * WM_GROUP + g;
    if (bw >= BW) break;                      // block-uniform
    const int64_t base = (bw * H + h) * (int64_t)N * WM_D;
    const float* mrow = mask ? mask + (int64_t)(bw % nW) * N * N : nullptr;

    wm_stage<NP, true, true>(Q + base, lq, lqT, N, tid);
    wm_stage<NP, true, true>(K + base, lk, lkT, N, tid);
    wm_stage<NP, true, false>(V + base, lv, nullptr, N, tid);
    wm_stage<NP, true, true>(DO + base, ldo, ldoT, N, tid);
    __syncthreads();

    // P, dP, dS of this wave's query tiles; dQ straight from registers
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int qt = wave + 4 * s;
      // keep the strips apart: hoisting the next strip's bias / mask loads
      // over this one's arithmetic costs more registers than there are
      __builtin_amdgcn_sched_barrier(0);
      if (qt < NT) {
        const int i = qt * 16 + fr;
        f32x4 p[NT];
        wm_probs<NT>(lq, lk, brow, mrow, N, qt, lane, scale, vec4, p);
        const u16x8 dof = *(const u16x8*)(ldo + i * WM_RS + kg * 8);
        f32x4 dp[NT];
        float rd = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          const u16x8 vf =
              *(const u16x8*)(lv + (kt * 16 + fr) * WM_RS + kg * 8);
          dp[kt] = wm_mfma(vf, dof, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) rd += dp[kt][r] * p[kt][r];
        }
        rd += __shfl_xor(rd, 16, 64);
        rd += __shfl_xor(rd, 32, 64);
        u16x4 dsb[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float ds = p[kt][r] * (dp[kt][r] - rd);
            dsacc[s][kt][r] += ds;
            dsb[kt][r] = wm_bf16(ds);
            const int j = kt * 16 + kg * 4 + r;
            lp[j * WM_PS + i] = wm_bf16(p[kt][r]);
            lds[j * WM_PS + i] = dsb[kt][r];
          }
        }
        f32x4 dq[2];
        wm_strip_times<NT>(dsb, lkT, lane, dq);
        wm_store_rows(DQ + base, i, N, kg, dq, scale);
      }
    }
    __syncthreads();

    // dV = Pᵀ·dO and dK = scale·dSᵀ·Q: units (which, key tile) over waves
    for (int unit = wave; unit < 2 * NT; unit += 4) {
      const bool is_dk = unit >= NT;
      const int jt = is_dk ? unit - NT : unit;
      const unsigned short* tile = (is_dk ? lds : lp) + (jt * 16 + fr) * WM_PS;
      const unsigned short* opT = is_dk ? lqT : ldoT;
      f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int i0 = c * 32 + kg * 8;
        u16x8 tf = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i0 < NP) tf = *(const u16x8*)(tile + i0);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const u16x8 af = *(const u16x8*)(opT + (dt * 16 + fr) * WM_TS + i0);
          acc[dt] = wm_mfma(af, tf, acc[dt]);
        }
      }
      wm_store_rows((is_dk ? DK : DV) + base, jt * 16 + fr, N, kg, acc,
                    is_dk ? scale : 1.0f);
    }
    __syncthreads();
  }

  float* part = DBP + ((int64_t)blockIdx.x * H + h) * (int64_t)N * N;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int qt = wave + 4 * s;
    if (qt < NT) {
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        wm_store4(part, qt * 16 + fr, kt * 16 + kg * 4, N, vec4, dsacc[s][kt]);
      }
    }
  }
}

void wm_check(const char* who, int64_t BW, int H, int N, int D, int nW,
              std::initializer_list<const void*> ptrs) {
  if (D != WM_D || N <= 64 || N > 144) {
    throw std::runtime_error(std::string(who) +
                             ": needs D == 32 and 64 < N <= 144");
  }
  if (BW <= 0 || H <= 0 || nW <= 0 || H > 65535 ||
      BW * H > (int64_t)0x7fffffff) {
    throw std::runtime_error(std::string(who) + ": bad BW / H / nW");
  }
  for (const void* p : ptrs) {
    if ((uintptr_t)p & 15) {
      throw std::runtime_error(std::string(who) +
                               ": pointers must be 16-byte aligned");
    }
  }
}

}  // namespace

extern "C" int flreid_window_attn_mfma_group() { return WM_GROUP; }

extern "C" void flreid_window_attn_mfma_fwd(const void* q, const void* k,
                                            const void* v, const float* bias,
                                            const float* mask, void* out,
                                            int64_t BW, int H, int N, int D,
                                            int nW, float scale,
                                            hipStream_t stream) {
  wm_check("window_attn_mfma_fwd", BW, H, N, D, nW,
           {q, k, v, bias, mask, out});
  dim3 grid((unsigned)(BW * H)), block(256);
  switch ((N + 15) / 16) {
#define FLREID_WM_CASE(NT)                                                    \
  case NT:                                                                    \
    hipLaunchKernelGGL((window_attn_mfma_fwd_kernel<NT>), grid, block, 0,     \
                       stream, (const __hip_bfloat16*)q,                      \
                       (const __hip_bfloat16*)k, (const __hip_bfloat16*)v,    \
                       bias, mask, (__hip_bfloat16*)out, H, N, nW, scale);    \
    break;
    FLREID_WM_CASE(5)
    FLREID_WM_CASE(6)
    FLREID_WM_CASE(7)
    FLREID_WM_CASE(8)
    FLREID_WM_CASE(9)
#undef FLREID_WM_CASE
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_window_attn_mfma_bwd(
    const void* q, const void* k, const void* v, const float* bias,
    const float* mask, const void* dout, void* dq, void* dk, void* dv,
    float* dbias_part, int64_t BW, int H, int N, int D, int nW, float scale,
    hipStream_t stream) {
  wm_check("window_attn_mfma_bwd", BW, H, N, D, nW,
           {q, k, v, bias, mask, dout, dq, dk, dv, dbias_part});
  dim3 grid((unsigned)((BW + WM_GROUP - 1) / WM_GROUP), (unsigned)H);
  dim3 block(256);
  switch ((N + 15) / 16) {
#define FLREID_WM_CASE(NT)                                                    \
  case NT: {                                                                  \
    constexpr int lds_bytes = wm_bwd_lds_elems(NT) * 2;                       \
    HIP_CHECK(hipFuncSetAttribute(                                            \
        (const void*)window_attn_mfma_bwd_kernel<NT>,                         \
        hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));              \
    hipLaunchKernelGGL((window_attn_mfma_bwd_kernel<NT>), grid, block,        \
                       lds_bytes, stream, (const __hip_bfloat16*)q,           \
                       (const __hip_bfloat16*)k, (const __hip_bfloat16*)v,    \
                       bias, mask, (const __hip_bfloat16*)dout,               \
                       (__hip_bfloat16*)dq, (__hip_bfloat16*)dk,              \
                       (__hip_bfloat16*)dv, dbias_part, BW, H, N, nW, scale); \
    break;                                                                    \
  }
    FLREID_WM_CASE(5)
    FLREID_WM_CASE(6)
    FLREID_WM_CASE(7)
    FLREID_WM_CASE(8)
    FLREID_WM_CASE(9)
#undef FLREID_WM_CASE
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

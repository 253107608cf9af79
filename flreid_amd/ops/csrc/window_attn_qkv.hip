// Packed-QKV MFMA Swin window attention for windows of 1..64 tokens (ws <= 8;
// 49 tokens at 224² / window 7), head dim 32, bf16 — forward and backward,
// straight on the projection output qkv [BW][N][3·C], C = H·32, last axis
// ordered (q|k|v, head, d).  The result is [BW][N][C], ready for `proj`; the
// backward writes one dqkv [BW][N][3·C].  No q/k/v copies, no transposes of
// the output, no [BW,H,N,N] tensor.
//
//   S = scale·Q·Kᵀ + bias[h] (+ mask[bw % nW]),  P = softmax_rows(S),  O = P·V
//   dV = Pᵀ·dO, dP = dO·Vᵀ, dS = P∘(dP − rowsum(dP∘P)),
//   dQ = scale·dS·K, dK = scale·dSᵀ·Q, dbias = Σ_windows dS
//
// The helpers that do not depend on how a token's row is found (wq_at,
// wq_opaque, the transposed copies, the strip products, the bias loads) are
// in window_attn_wq.h, shared with window_attn_map.hip, which runs the same
// attention on the feature map.
//
// Design (v_mfma_f32_16x16x32_bf16 throughout; NT = ⌈N/16⌉ tiles, a kernel
// instance per NT = 1..4 and per mask / no mask so every tile loop unrolls
// into registers and nothing branches on the mask pointer):
//  - one WAVE serves one (window, head); a workgroup is 4 independent waves.
//    The ragged last tile (N = 49: one valid row of 16) costs idle MFMA
//    slots only.  All LDS is wave-private; the only __syncthreads are around
//    the bias-gradient reduction at the end of the backward.
//  - operands straight from the packed tensor: a Q, K, V or dO fragment is 16
//    bytes of one token row (lane (fr, kg) reads row[16·t + fr][8·kg..+7])
//    loaded from global memory into the operand registers with the packed
//    row stride 3·C (C for dO); rows >= N are zero.  A head's 64-byte row
//    segment is half a 128-byte line: in the forward adjacent waves take
//    adjacent heads of one window, in the backward grid y = head, so the
//    other half is wanted by a neighbour at the same time.
//  - forward: the TRANSPOSED strip Sᵀ = K·Qᵀ gives a lane ONE query
//    (lane & 15) and, per key tile, the 4 keys 4·(lane >> 4) + r.  Scale,
//    bias and mask are applied in fp32 on the accumulators, keys >= N are
//    −inf, max and sum are an in-lane reduction plus two shuffles (xor 16,
//    32).  P is rounded to bf16 in registers and fed back as the B operand;
//    two key tiles of a lane are the 8 values it wants, which permutes the
//    contraction index (slot (kg, e) = key 16·(2u + e/4) + 4·kg + e%4), and V
//    is read with the same permutation from a wave-private transposed copy
//    Vᵀ[d][key] in LDS, written from the V fragments (row stride 16·NTE + 8
//    elements, NTE = NT rounded up to even; the tile past an odd NT is
//    zero).  The result is Oᵀ: a lane holds one query and 4 consecutive d,
//    an 8-byte store.  4 608 B of LDS per wave at NT = 3, 4.
//  - backward, two passes, no P / dS tiles in LDS (at one wave per window
//    those two [key][query] tiles would be 16 KB a wave):
//    pass 1, transposed layout as the forward: P, dPᵀ = V·dOᵀ, rd =
//    rowsum(dP∘P) and dS in fp32 registers; the unrounded dS goes into the
//    wave's dbias accumulator; dQ = scale·dS·K from registers against Kᵀ in
//    LDS.  The row max, 1/sum and rd of each query go to a 3 × 64-float
//    wave-private array.
//    pass 2, untransposed: S = Q·Kᵀ and dP = dO·Vᵀ with the operands
//    swapped, so a lane owns ONE key (lane & 15) and 4 queries per query
//    tile; P and dS are formed again from the saved row statistics.  Two
//    query tiles of a lane are then the 8 values a B operand wants for a
//    contraction over queries: dVᵀ = dOᵀ·P and dKᵀ = scale·Qᵀ·dS run from
//    registers against dOᵀ / Qᵀ copies in LDS (Qᵀ overwrites Kᵀ, which
//    pass 1 has finished with).  Cost: 2·NT² extra MFMAs and a second exp
//    pass per window.  9 984 B of LDS per wave at NT = 3, 4.  K and V
//    fragments are resident through pass 1 only, Q and dO fragments through
//    pass 2 only; the other pair is read per tile from global memory again.
//    Bias and mask are read with dword loads at 32-bit byte offsets from a
//    scalar base (wq_at), and the per-window bases are formed from opaque
//    indices (wq_opaque), or the compiler carries every address of the
//    window loop as a 64-bit pair.
//  - bias gradient: a backward workgroup is (run of WQ_GROUP windows, head);
//    wave w walks windows w, w + 4, .. of the run and keeps the fp32 dS sum
//    in registers (NT² float4).  At the end waves 1, 2, 3 hand their sums to
//    wave 0 through LDS in that order — no atomics, the same bits every
//    run — and wave 0 writes one [N][N] partial; the wrapper sums the
//    [⌈BW/WQ_GROUP⌉, H, N, N] partials.
//
// Resources, from the compiler's resource summary (hipcc -O3, gfx950,
// packed fp32 off), masked instances:
//   fwd NT = 1:  34 VGPRs +   8 AGPRs, no spill, 10 240 B static LDS
//   fwd NT = 4:  84 VGPRs +   8 AGPRs, no spill, 18 432 B static LDS
//               (5 waves / SIMD)
//   bwd NT = 1:  82 VGPRs +  12 AGPRs, no spill, 23 552 B static LDS
//   bwd NT = 4: 256 VGPRs + 191 AGPRs, no spill, 39 936 B static LDS
//               (1 wave / SIMD)
// The NT = 4 backward is the weak point: next to the 64 registers of dsacc
// and 32 of fragments the unrolled strips keep about 350 more alive, so a
// SIMD holds one wave.  Bounding it to 256 registers (two waves) spills 185
// VGPRs, which is worse; the kept form has none.  It is still 6× the
// unpacked route (profiles/README.md); a second wave is the open gain.

#include "common.h"
#include "ops.h"
#include "window_attn_wq.h"

#include <initializer_list>

namespace flreid {

namespace {

using namespace wq;             // the helpers shared with window_attn_map.hip

// The NT fragments of one [N][32] matrix whose rows lie `stride` elements
// apart (g is wave-uniform; the byte offset fits 32 bits: 64 rows of at most
// 3·65535·32 elements): f[t] = g[16·t + fr][8·kg .. 8·kg + 7], zero for rows >= N.
template <int NT>
__device__ __forceinline__ void wq_load_frags(
    const __hip_bfloat16* __restrict__ g, int stride, int N, int lane,
    u16x8 (&f)[NT]) {
  const int fr = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int row = t * 16 + fr;
    f[t] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (row < N) f[t] = *(const u16x8*)wq_at(g, row * stride + kg * 8);
  }
}

// The normalised probabilities of the query tile whose fragment is qf,
// transposed-strip layout: p[kt][r] = P[i][kt·16 + 4·kg + r], i = the tile's
// row (lane & 15); zero for i >= N or key >= N.  m is the row max of S and
// inv the reciprocal of the row's exp sum (zero for i >= N).
template <int NT, bool MASK>
__device__ __forceinline__ void wq_probs(u16x8 qf, const u16x8 (&kf)[NT],
                                         const float* __restrict__ brow,
                                         const float* __restrict__ mrow, int N,
                                         int i, int lane, float scale,
                                         f32x4 (&p)[NT], float& m,
                                         float& inv) {
  const int kg = lane >> 4;
  const int row = min(i, N - 1) * N;
  m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    const f32x4 acc = wq_mfma(kf[kt], qf, f32x4{0.f, 0.f, 0.f, 0.f});
    const int j0 = kt * 16 + kg * 4;
    const f32x4 b = wq_load4(brow, row, j0, N, kt == NT - 1);
    f32x4 mk = {0.f, 0.f, 0.f, 0.f};
    if (MASK) mk = wq_load4(mrow, row, j0, N, kt == NT - 1);
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
  inv = (i < N) ? 1.0f / se : 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[kt][r] *= inv;
  }
}

// out[dt][0..3] · mul -> g[i][16·dt + 4·kg ..] as bf16 (8-byte stores), rows
// `stride` elements apart
__device__ __forceinline__ void wq_store_rows(__hip_bfloat16* __restrict__ g,
                                              int stride, int i, int N,
                                              int kg, const f32x4 (&out)[2],
                                              float mul) {
  if (i >= N) return;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    u16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = wq_bf16(out[dt][r] * mul);
    *(u16x4*)wq_at(g, i * stride + dt * 16 + kg * 4) = o;
  }
}

template <int NT, bool MASK>
__global__ __launch_bounds__(256) void window_attn_qkv_fwd_kernel(
    const __hip_bfloat16* __restrict__ QKV, const float* __restrict__ bias,
    const float* __restrict__ mask, __hip_bfloat16* __restrict__ O,
    int64_t WH, int H, int N, int nW, float scale) {
  constexpr int TB = WQ_D * wq_ts(NT);
  __shared__ __attribute__((aligned(16))) unsigned short lds[4 * TB];

  const int lane = threadIdx.x & 63;
  // uniform to the compiler too: the bases below are scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wh = (int64_t)blockIdx.x * 4 + wave;
  if (wh >= WH) return;                       // wave-uniform; no barriers
  const int64_t bw = wh / H;
  const int h = (int)(wh % H);
  const int C = H * WQ_D;
  const __hip_bfloat16* q0 = QKV + bw * N * 3 * C + h * WQ_D;
  unsigned short* lvT = lds + wave * TB;
  const int fr = lane & 15, kg = lane >> 4;

  u16x8 kf[NT], vf[NT];
  wq_load_frags<NT>(q0 + C, 3 * C, N, lane, kf);
  wq_load_frags<NT>(q0 + 2 * C, 3 * C, N, lane, vf);
  wq_put_transposed<NT>(lvT, vf, lane);
  wq_wave_sync();

  const float* brow = bias + (int64_t)h * N * N;
  const float* mrow = MASK ? mask + (int64_t)(bw % nW) * N * N : nullptr;
  __hip_bfloat16* o0 = O + bw * N * C + h * WQ_D;

#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
    const int i = qt * 16 + fr;
    u16x8 qf = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < N) qf = *(const u16x8*)wq_at(q0, i * 3 * C + kg * 8);
    f32x4 p[NT];
    float m, inv;
    wq_probs<NT, MASK>(qf, kf, brow, mrow, N, i, lane, scale, p, m, inv);
    u16x4 pb[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pb[kt][r] = wq_bf16(p[kt][r]);
    }
    f32x4 o[2];
    wq_strip_times<NT>(pb, lvT, lane, o);
    wq_store_rows(o0, C, i, N, kg, o, 1.0f);
  }
}

template <int NT, bool MASK>
__global__ __launch_bounds__(256) void window_attn_qkv_bwd_kernel(
    const __hip_bfloat16* __restrict__ QKV, const float* __restrict__ bias,
    const float* __restrict__ mask, const __hip_bfloat16* __restrict__ DO,
    __hip_bfloat16* __restrict__ DQKV, float* __restrict__ DBP, int64_t BW,
    int H, int N, int nW, float scale) {
  constexpr int TB = WQ_D * wq_ts(NT);
  constexpr int WE = wq_bwd_wave_elems(NT);
  __shared__ __attribute__((aligned(16))) unsigned short lds[4 * WE];
  // the dbias reduction passes one wave's NT² float4 per lane through it
  static_assert(4 * WE * 2 >= NT * NT * 64 * 16, "reduction needs the LDS");

  const int h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, kg = lane >> 4;
  const int C = H * WQ_D;
  unsigned short* lA = lds + wave * WE;       // Kᵀ in pass 1, Qᵀ in pass 2
  unsigned short* lB = lA + TB;               // dOᵀ
  float* stat = (float*)(lB + TB);            // [3][64]: max, 1/sum, rd
  const bool vec4 = (N & 3) == 0;

  f32x4 dsacc[NT][NT];
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) dsacc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

#pragma unroll 1
  for (int g = wave; g < WQ_GROUP; g += 4) {
    const int64_t bw = (int64_t)blockIdx.x * WQ_GROUP + wq_opaque(g);
    if (bw >= BW) break;                      // wave-uniform; no barriers
    const int hq = wq_opaque(h);
    const __hip_bfloat16* q0 = QKV + bw * N * 3 * C + hq * WQ_D;
    const __hip_bfloat16* do0 = DO + bw * N * C + hq * WQ_D;
    __hip_bfloat16* dq0 = DQKV + bw * N * 3 * C + hq * WQ_D;
    const float* brow = bias + (int64_t)hq * N * N;
    const float* mrow = MASK ? mask + (int64_t)(bw % nW) * N * N : nullptr;

    // Registers: K and V fragments live through pass 1, Q and dO fragments
    // through pass 2; the other pair comes per tile from global memory (L2
    // hits).  All four resident next to dsacc would spill at NT = 4.
    u16x8 kf[NT], vf[NT];
    wq_load_frags<NT>(q0 + C, 3 * C, N, lane, kf);
    wq_load_frags<NT>(q0 + 2 * C, 3 * C, N, lane, vf);
    wq_wave_sync();                           // the last window's reads
    wq_put_transposed<NT>(lA, kf, lane);
    {
      u16x8 dof[NT];
      wq_load_frags<NT>(do0, C, N, lane, dof);
      wq_put_transposed<NT>(lB, dof, lane);
    }
    wq_wave_sync();

    // pass 1: lane = one query, 4 keys per key tile
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
      // keep the strips apart: hoisting the next strip's bias / mask loads
      // over this one's arithmetic costs more registers than there are
      __builtin_amdgcn_sched_barrier(0);
      const int i = qt * 16 + fr;
      u16x8 qfi = {0, 0, 0, 0, 0, 0, 0, 0}, dofi = qfi;
      if (i < N) {
        qfi = *(const u16x8*)wq_at(q0, i * 3 * C + kg * 8);
        dofi = *(const u16x8*)wq_at(do0, i * C + kg * 8);
      }
      f32x4 p[NT];
      float m, inv;
      wq_probs<NT, MASK>(qfi, kf, brow, mrow, N, i, lane, scale, p, m,
                         inv);
      f32x4 dp[NT];
      float rd = 0.f;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        dp[kt] = wq_mfma(vf[kt], dofi, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) rd += dp[kt][r] * p[kt][r];
      }
      rd += __shfl_xor(rd, 16, 64);
      rd += __shfl_xor(rd, 32, 64);
      if (kg == 0) {
        stat[i] = m;
        stat[64 + i] = inv;
        stat[128 + i] = rd;
      }
      u16x4 dsb[NT];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ds = p[kt][r] * (dp[kt][r] - rd);
          dsacc[qt][kt][r] += ds;
          dsb[kt][r] = wq_bf16(ds);
        }
      }
      f32x4 dq[2];
      wq_strip_times<NT>(dsb, lA, lane, dq);
      wq_store_rows(dq0, 3 * C, i, N, kg, dq, scale);
    }
    wq_wave_sync();                           // Kᵀ is done with
    // (the opaque zero keeps these loads from being merged with pass 1's)
    u16x8 qf[NT], dof[NT];
    wq_load_frags<NT>(q0 + wq_opaque(0), 3 * C, N, lane, qf);
    wq_load_frags<NT>(do0 + wq_opaque(0), C, N, lane, dof);
    wq_put_transposed<NT>(lA, qf, lane);
    wq_wave_sync();

    // pass 2: lane = one key, 4 queries per query tile.  A rolled loop:
    // the key tile's K and V fragments come from global memory again (L2
    // hits) so that nothing is indexed by kt.
#pragma unroll 1
    for (int kt = 0; kt < NT; ++kt) {
      const int j = kt * 16 + fr;
      u16x8 kfj = {0, 0, 0, 0, 0, 0, 0, 0}, vfj = kfj;
      if (j < N) {
        kfj = *(const u16x8*)wq_at(q0 + C, j * 3 * C + kg * 8);
        vfj = *(const u16x8*)wq_at(q0 + 2 * C, j * 3 * C + kg * 8);
      }
      u16x4 pb[NT], dsb[NT];
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
        __builtin_amdgcn_sched_barrier(0);    // as in pass 1
        const int i0 = qt * 16 + kg * 4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 s = wq_mfma(qf[qt], kfj, zero);
        const f32x4 dp = wq_mfma(dof[qt], vfj, zero);
        const f32x4 b = wq_load_col(brow, i0, j, N);
        f32x4 mk = {0.f, 0.f, 0.f, 0.f};
        if (MASK) mk = wq_load_col(mrow, i0, j, N);
        const f32x4 m4 = *(const f32x4*)(stat + i0);
        const f32x4 inv4 = *(const f32x4*)(stat + 64 + i0);
        const f32x4 rd4 = *(const f32x4*)(stat + 128 + i0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv = s[r] * scale + b[r];
          sv += mk[r];
          sv = (j < N) ? sv : -INFINITY;
          // a query >= N has inv = 0 and a finite max: P = 0
          const float pv = __expf(sv - m4[r]) * inv4[r];
          pb[qt][r] = wq_bf16(pv);
          dsb[qt][r] = wq_bf16(pv * (dp[r] - rd4[r]));
        }
      }
      f32x4 dv[2], dk[2];
      wq_strip_times<NT>(pb, lB, lane, dv);
      wq_store_rows(dq0 + 2 * C, 3 * C, j, N, kg, dv, 1.0f);
      wq_strip_times<NT>(dsb, lA, lane, dk);
      wq_store_rows(dq0 + C, 3 * C, j, N, kg, dk, scale);
    }
  }

  // dbias partial of the run: waves 1, 2, 3 into wave 0, in that order
  f32x4* red = (f32x4*)lds;
  __syncthreads();
#pragma unroll 1
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          red[(qt * NT + kt) * 64 + lane] = dsacc[qt][kt];
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          dsacc[qt][kt] += red[(qt * NT + kt) * 64 + lane];
        }
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* part = DBP + ((int64_t)blockIdx.x * H + h) * (int64_t)N * N;
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        wq_store4(part, qt * 16 + fr, kt * 16 + kg * 4, N, vec4,
                  dsacc[qt][kt]);
      }
    }
  }
}

void wq_check(const char* who, int64_t BW, int H, int N, int nW,
              std::initializer_list<const void*> ptrs) {
  if (N < 1 || N > 64) {
    throw std::runtime_error(std::string(who) + ": needs 1 <= N <= 64");
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

extern "C" int flreid_window_attn_qkv_group() { return WQ_GROUP; }

extern "C" void flreid_window_attn_qkv_fwd(const void* qkv, const float* bias,
                                           const float* mask, void* out,
                                           int64_t BW, int H, int N, int nW,
                                           float scale, hipStream_t stream) {
  wq_check("window_attn_qkv_fwd", BW, H, N, nW, {qkv, bias, mask, out});
  const int64_t WH = BW * H;
  dim3 grid((unsigned)((WH + 3) / 4)), block(256);
  switch ((N + 15) / 16) {
#define FLREID_WQ_CASE(NT)                                                    \
  case NT:                                                                    \
    if (mask) {                                                               \
      hipLaunchKernelGGL((window_attn_qkv_fwd_kernel<NT, true>), grid, block, \
                         0, stream, (const __hip_bfloat16*)qkv, bias, mask,   \
                         (__hip_bfloat16*)out, WH, H, N, nW, scale);          \
    } else {                                                                  \
      hipLaunchKernelGGL((window_attn_qkv_fwd_kernel<NT, false>), grid,       \
                         block, 0, stream, (const __hip_bfloat16*)qkv, bias,  \
                         mask, (__hip_bfloat16*)out, WH, H, N, nW, scale);    \
    }                                                                         \
    break;
    FLREID_WQ_CASE(1)
    FLREID_WQ_CASE(2)
    FLREID_WQ_CASE(3)
    FLREID_WQ_CASE(4)
#undef FLREID_WQ_CASE
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_window_attn_qkv_bwd(const void* qkv, const float* bias,
                                           const float* mask, const void* dout,
                                           void* dqkv, float* dbias_part,
                                           int64_t BW, int H, int N, int nW,
                                           float scale, hipStream_t stream) {
  wq_check("window_attn_qkv_bwd", BW, H, N, nW,
           {qkv, bias, mask, dout, dqkv, dbias_part});
  dim3 grid((unsigned)((BW + WQ_GROUP - 1) / WQ_GROUP), (unsigned)H);
  dim3 block(256);
  switch ((N + 15) / 16) {
#define FLREID_WQ_CASE(NT)                                                    \
  case NT:                                                                    \
    if (mask) {                                                               \
      hipLaunchKernelGGL((window_attn_qkv_bwd_kernel<NT, true>), grid, block, \
                         0, stream, (const __hip_bfloat16*)qkv, bias, mask,   \
                         (const __hip_bfloat16*)dout, (__hip_bfloat16*)dqkv,  \
                         dbias_part, BW, H, N, nW, scale);                    \
    } else {                                                                  \
      hipLaunchKernelGGL((window_attn_qkv_bwd_kernel<NT, false>), grid,       \
                         block, 0, stream, (const __hip_bfloat16*)qkv, bias,  \
                         mask, (const __hip_bfloat16*)dout,                   \
                         (__hip_bfloat16*)dqkv, dbias_part, BW, H, N, nW,     \
                         scale);                                              \
    }                                                                         \
    break;
    FLREID_WQ_CASE(1)
    FLREID_WQ_CASE(2)
    FLREID_WQ_CASE(3)
    FLREID_WQ_CASE(4)
#undef FLREID_WQ_CASE
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

// Fused FedWeIT weight composition, forward and backward
// (models/decomposed.py::DecomposedBase.composed_weight):
//
//   θ[r,j] = thr(mask[r], λ_mask)·sw[r,j] + thr(aw[r,j], λ_l1)
//            + Σ_k atten[k]·aw_kb[r,j,k]          thr(w, λ) = w·1[|w| > λ]
//
// (thresholds only when training).  The eager chain writes and re-reads an
// aw_kb-sized temporary in both directions and reduces it with a stride-KB
// pattern; here every operand is read exactly once — (KB+3) floats per
// element forward, (KB+4) backward — and no temporary reaches HBM.
//
// Data view.  rows = sw.shape[0] (one mask entry per row), inner = C·S
// elements per row, aw_kb is always logical-contiguous [rows][inner][KB].
// sw / aw / θ / dθ share one dense layout: logical-contiguous, or
// channels-last [rows][S][C] for 4-D weights with S = kh·kw > 1 and C > 1.
//
// Work decomposition.  The unit of work is one WAVE (64 lanes); a 256-thread
// block is four independent wave tasks, so short rows share a block and long
// rows spread over several:
//   contiguous   : task = (row, chunk of 512 consecutive elements);
//                  (8000, 2048) -> 32000 tasks, (2048, 512) -> 2048 tasks.
//                  Lanes take 4 consecutive elements each (float4 on every
//                  operand, KB float4 on aw_kb) when inner % 4 == 0 and the
//                  pointers are 16-byte aligned, else 1 element each.
//   channels-last: task = (row, tile of 64 channels × ≤16 taps);
//                  (512, 512, 3, 3) -> 4096 tasks.  The two sides of a tile
//                  are each other's transpose: aw_kb holds it as [c][s]·KB
//                  (one contiguous run when S ≤ 16, read as float4 quads),
//                  sw/aw/θ/dθ hold it as S runs of 64 consecutive channels
//                  (one run per wave instruction).  The tile crosses through
//                  LDS: float tile[64][pitch], pitch = taps | 1 (odd).  The
//                  [c][s]-order side touches it in runs of consecutive
//                  words; the transposed side has lane = channel, stride =
//                  pitch words, and an odd pitch maps the 64 lanes onto the
//                  64 distinct 4-byte banks.  Forward stages the KB-reduced
//                  tile, backward stages the dθ tile.  4 waves × 64 × 17
//                  floats = 17 KiB of LDS per block.
//
// Reductions are deterministic — no floating-point atomics.  d_mask: each
// task writes one partial into dmask_part[rows][tasks_per_row]; d_atten:
// each block combines its four waves in a fixed order and writes KB
// partials into datten_part[blocks][KB].  The wrapper finishes both with a
// torch sum over the partial axis (as drift_fwd does).  Workspaces come
// from the wrapper; nothing here allocates or synchronises, so both kernels
// are safe under hipGraph capture.
//
// KB is a runtime value: 1…8 are template instances (fully unrolled, atten
// and the d_atten accumulators in registers); any other KB runs a generic
// loop (the backward in passes of 8 accumulators).

#include "common.h"
#include "ops.h"

namespace flreid {

constexpr int DC_BLOCK = 256;
constexpr int DC_WAVES = DC_BLOCK / kWave;
constexpr int DC_CHUNK = 512;  // elements per wave task, contiguous layout
constexpr int DC_CT = 64;      // channels per tile, channels-last layout
constexpr int DC_ST = 16;      // taps per tile (upper bound)
constexpr int DC_PITCH = DC_ST | 1;
constexpr int DC_KMAX = 8;     // largest templated KB / generic pass width

__device__ __forceinline__ float dc_thr(float w, float lam, bool train) {
  return (!train || fabsf(w) > lam) ? w : 0.f;
}

template <int VEC>
__device__ __forceinline__ void dc_load_f32(const float* __restrict__ p,
                                            float (&o)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {
    o[0] = p[0];
  }
}

template <int VEC>
__device__ __forceinline__ void dc_store_f32(float* __restrict__ p,
                                             const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// θ / dθ are fp32 or bf16 (wave-uniform runtime flag); i is an element index
template <int VEC>
__device__ __forceinline__ void dc_load_any(const void* __restrict__ base,
                                            int64_t i, bool bf16,
                                            float (&o)[VEC]) {
  if (!bf16) {
    dc_load_f32<VEC>(reinterpret_cast<const float*>(base) + i, o);
  } else {
    const uint16_t* p = reinterpret_cast<const uint16_t*>(base) + i;
    if constexpr (VEC == 4) {
      const uint2 v = *reinterpret_cast<const uint2*>(p);
      o[0] = __uint_as_float(v.x << 16);
      o[1] = __uint_as_float(v.x & 0xffff0000u);
      o[2] = __uint_as_float(v.y << 16);
      o[3] = __uint_as_float(v.y & 0xffff0000u);
    } else {
      o[0] = __uint_as_float((uint32_t)p[0] << 16);
    }
  }
}

template <int VEC>
__device__ __forceinline__ void dc_store_any(void* __restrict__ base,
                                             int64_t i, bool bf16,
                                             const float (&v)[VEC]) {
  if (!bf16) {
    dc_store_f32<VEC>(reinterpret_cast<float*>(base) + i, v);
  } else {
    __hip_bfloat16 h[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) h[e] = __float2bfloat16(v[e]);  // RNE
    __builtin_memcpy(reinterpret_cast<__hip_bfloat16*>(base) + i, h,
                     sizeof(h));
  }
}

// VEC·KB consecutive aw_kb floats starting at p (16-byte aligned for VEC 4)
template <int KB_T, int VEC>
__device__ __forceinline__ void dc_load_kb(const float* __restrict__ p,
                                           float (&flat)[VEC * KB_T]) {
  if constexpr (VEC == 4) {
#pragma unroll
    for (int q = 0; q < KB_T; ++q) {
      const float4 v = reinterpret_cast<const float4*>(p)[q];
      flat[4 * q] = v.x; flat[4 * q + 1] = v.y;
      flat[4 * q + 2] = v.z; flat[4 * q + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < KB_T; ++k) flat[k] = p[k];
  }
}

// out[e] = Σ_k atten[k]·aw_kb[e][k] for VEC consecutive elements at p
template <int KB_T, int VEC>
__device__ __forceinline__ void dc_kb_dot(const float* __restrict__ p,
                                          const float* at_reg,
                                          const float* __restrict__ atten,
                                          int KB, float (&out)[VEC]) {
  if constexpr (KB_T > 0) {
    float flat[VEC * KB_T];
    dc_load_kb<KB_T, VEC>(p, flat);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < KB_T; ++k) s = fmaf(at_reg[k], flat[e * KB_T + k], s);
      out[e] = s;
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float s = 0.f;
      for (int k = 0; k < KB; ++k) s = fmaf(atten[k], p[(int64_t)e * KB + k], s);
      out[e] = s;
    }
  }
}

// acc[k] += Σ_e g[e]·aw_kb[e][k0+k] for VEC consecutive elements at p
template <int KB_T, int VEC>
__device__ __forceinline__ void dc_kb_acc(const float* __restrict__ p,
                                          const float (&g)[VEC], int KB,
                                          int k0, int kc,
                                          float (&acc)[DC_KMAX]) {
  if constexpr (KB_T > 0) {
    float flat[VEC * KB_T];
    dc_load_kb<KB_T, VEC>(p, flat);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
#pragma unroll
      for (int k = 0; k < KB_T; ++k)
        acc[k] = fmaf(g[e], flat[e * KB_T + k], acc[k]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
#pragma unroll
      for (int k = 0; k < DC_KMAX; ++k) {
        if (k < kc) acc[k] = fmaf(g[e], p[(int64_t)e * KB + k0 + k], acc[k]);
      }
    }
  }
}

// wave sums of acc[0..kc) -> fixed-order sum over the block's waves ->
// datten_part[block][k0..k0+kc).  Called by every thread of the block.
__device__ __forceinline__ void dc_block_atten_partial(
    float (&acc)[DC_KMAX], int k0, int kc, int KB,
    float (*red)[DC_KMAX], float* __restrict__ datten_part) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = threadIdx.x / kWave;
#pragma unroll
  for (int k = 0; k < DC_KMAX; ++k) {
    if (k < kc) {
      const float s = wave_reduce_sum(acc[k]);
      if (lane == 0) red[wid][k] = s;
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < kc) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < DC_WAVES; ++w) s += red[w][threadIdx.x];
    datten_part[(int64_t)blockIdx.x * KB + k0 + threadIdx.x] = s;
  }
  __syncthreads();
}

struct DcClTask {
  bool valid;
  int row, c0, ct_n, s0, st_n, pitch;
};

__device__ __forceinline__ DcClTask dc_cl_task(int rows, int C, int S,
                                               int nct, int nst) {
  DcClTask t;
  const int64_t task =
      (int64_t)blockIdx.x * DC_WAVES + (int)(threadIdx.x / kWave);
  const int tpr = nct * nst;
  t.valid = task < (int64_t)rows * tpr;
  t.row = t.valid ? (int)(task / tpr) : 0;
  const int rem = t.valid ? (int)(task - (int64_t)t.row * tpr) : 0;
  const int ct = rem / nst, st = rem - ct * nst;
  t.c0 = ct * DC_CT;
  t.ct_n = min(DC_CT, C - t.c0);
  t.s0 = st * DC_ST;
  t.st_n = min(DC_ST, S - t.s0);
  t.pitch = t.st_n | 1;
  return t;
}

// LDS word of logical tile element l = cc·st_n + ss
__device__ __forceinline__ int dc_tile_word(int l, int st_n, int pitch) {
  if (pitch == st_n) return l;  // odd tap count (3×3): no padding
  const int cc = l / st_n;
  return cc * pitch + (l - cc * st_n);
}

// aw_kb element index of logical tile element l.  VEC 4 implies one tap
// tile per row (s0 == 0, st_n == S): the whole tile is one contiguous run.
template <int VEC>
__device__ __forceinline__ int64_t dc_cl_kb_elem(const DcClTask& t, int l,
                                                 int C, int S) {
  if constexpr (VEC == 4) {
    return ((int64_t)t.row * C + t.c0) * S + l;
  } else {
    const int cc = l / t.st_n;
    const int ss = l - cc * t.st_n;
    return ((int64_t)t.row * C + t.c0 + cc) * S + t.s0 + ss;
  }
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

template <int KB_T, int VEC>
__global__ __launch_bounds__(DC_BLOCK) void decomposed_fwd_contig_kernel(
    const float* __restrict__ sw, const float* __restrict__ mask,
    const float* __restrict__ aw, const float* __restrict__ aw_kb,
    const float* __restrict__ atten, void* __restrict__ out, int rows,
    int inner, int KB, int cpr, bool train, float l1, float lm,
    bool out_bf16) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t task =
      (int64_t)blockIdx.x * DC_WAVES + (int)(threadIdx.x / kWave);
  if (task >= (int64_t)rows * cpr) return;  // no block barrier below
  const int row = (int)(task / cpr);
  const int j0 = (int)(task - (int64_t)row * cpr) * DC_CHUNK;
  const int n = min(DC_CHUNK, inner - j0);
  const int64_t e0 = (int64_t)row * inner + j0;

  float at[KB_T > 0 ? KB_T : 1];
  if constexpr (KB_T > 0) {
#pragma unroll
    for (int k = 0; k < KB_T; ++k) at[k] = atten[k];
  }
  const float m = dc_thr(mask[row], lm, train);

#pragma unroll 2
  for (int jj = lane * VEC; jj < n; jj += kWave * VEC) {
    const int64_t e = e0 + jj;
    float s[VEC], a[VEC], kb[VEC], r[VEC];
    dc_load_f32<VEC>(sw + e, s);
    dc_load_f32<VEC>(aw + e, a);
    dc_kb_dot<KB_T, VEC>(aw_kb + e * KB, at, atten, KB, kb);
#pragma unroll
    for (int i = 0; i < VEC; ++i)
      r[i] = fmaf(m, s[i], dc_thr(a[i], l1, train)) + kb[i];
    dc_store_any<VEC>(out, e, out_bf16, r);
  }
}

template <int KB_T, int VEC>
__global__ __launch_bounds__(DC_BLOCK) void decomposed_fwd_cl_kernel(
    const float* __restrict__ sw, const float* __restrict__ mask,
    const float* __restrict__ aw, const float* __restrict__ aw_kb,
    const float* __restrict__ atten, void* __restrict__ out, int rows, int C,
    int S, int KB, int nct, int nst, bool train, float l1, float lm,
    bool out_bf16) {
  __shared__ float tile[DC_WAVES][DC_CT * DC_PITCH];
  const int lane = threadIdx.x & (kWave - 1);
  float* t = tile[threadIdx.x / kWave];
  const DcClTask tk = dc_cl_task(rows, C, S, nct, nst);

  float at[KB_T > 0 ? KB_T : 1];
  if constexpr (KB_T > 0) {
#pragma unroll
    for (int k = 0; k < KB_T; ++k) at[k] = atten[k];
  }

  // phase 1: KB-reduce the tile in aw_kb's [c][s] order, stage it in LDS
  if (tk.valid) {
    const int n = tk.ct_n * tk.st_n;
    for (int l = lane * VEC; l < n; l += kWave * VEC) {
      float kb[VEC];
      dc_kb_dot<KB_T, VEC>(aw_kb + dc_cl_kb_elem<VEC>(tk, l, C, S) * KB, at,
                           atten, KB, kb);
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        t[dc_tile_word(l + i, tk.st_n, tk.pitch)] = kb[i];
    }
  }
  __syncthreads();
  // phase 2: one 64-channel run of sw/aw/θ per tap, lane = channel
  if (tk.valid && lane < tk.ct_n) {
    const float m = dc_thr(mask[tk.row], lm, train);
    for (int ss = 0; ss < tk.st_n; ++ss) {
      const int64_t p =
          ((int64_t)tk.row * S + tk.s0 + ss) * C + tk.c0 + lane;
      float r[1];
      r[0] = fmaf(m, sw[p], dc_thr(aw[p], l1, train)) +
             t[lane * tk.pitch + ss];
      dc_store_any<1>(out, p, out_bf16, r);
    }
  }
}

// ---------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------

template <int KB_T, int VEC>
__global__ __launch_bounds__(DC_BLOCK) void decomposed_bwd_contig_kernel(
    const void* __restrict__ g, bool g_bf16, const float* __restrict__ sw,
    const float* __restrict__ mask, const float* __restrict__ aw,
    const float* __restrict__ aw_kb, float* __restrict__ d_aw,
    float* __restrict__ dmask_part, float* __restrict__ datten_part, int rows,
    int inner, int KB, int cpr, bool train, float l1, float lm, bool need_aw,
    bool need_mask, bool need_atten) {
  __shared__ float red[DC_WAVES][DC_KMAX];
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t task =
      (int64_t)blockIdx.x * DC_WAVES + (int)(threadIdx.x / kWave);
  const bool valid = task < (int64_t)rows * cpr;
  const int row = valid ? (int)(task / cpr) : 0;
  const int j0 = valid ? (int)(task - (int64_t)row * cpr) * DC_CHUNK : 0;
  const int n = valid ? min(DC_CHUNK, inner - j0) : 0;
  const int64_t e0 = (int64_t)row * inner + j0;

  float dm = 0.f;
  // one pass for templated KB (or when d_atten is not wanted); the generic
  // KB re-reads dθ once per 8 accumulators
  const int npass = (KB_T > 0 || !need_atten) ? 1 : (KB + DC_KMAX - 1) / DC_KMAX;
  for (int pass = 0; pass < npass; ++pass) {
    const int k0 = pass * DC_KMAX;
    const int kc = KB_T > 0 ? KB_T : min(DC_KMAX, KB - k0);
    float acc[DC_KMAX];
#pragma unroll
    for (int k = 0; k < DC_KMAX; ++k) acc[k] = 0.f;

#pragma unroll 2
    for (int jj = lane * VEC; jj < n; jj += kWave * VEC) {
      const int64_t e = e0 + jj;
      float gv[VEC];
      dc_load_any<VEC>(g, e, g_bf16, gv);
      if (pass == 0) {
        if (need_aw) {
          float da[VEC];
          if (train) {
            float a[VEC];
            dc_load_f32<VEC>(aw + e, a);
#pragma unroll
            for (int i = 0; i < VEC; ++i)
              da[i] = fabsf(a[i]) > l1 ? gv[i] : 0.f;
          } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) da[i] = gv[i];
          }
          dc_store_f32<VEC>(d_aw + e, da);
        }
        if (need_mask) {
          float s[VEC];
          dc_load_f32<VEC>(sw + e, s);
#pragma unroll
          for (int i = 0; i < VEC; ++i) dm = fmaf(gv[i], s[i], dm);
        }
      }
      if (need_atten)
        dc_kb_acc<KB_T, VEC>(aw_kb + e * KB, gv, KB, k0, kc, acc);
    }
    if (need_atten)
      dc_block_atten_partial(acc, k0, kc, KB, red, datten_part);
  }
  if (need_mask) {
    dm = wave_reduce_sum(dm);
    if (valid && lane == 0) {
      const bool keep = !train || fabsf(mask[row]) > lm;
      dmask_part[task] = keep ? dm : 0.f;
    }
  }
}

template <int KB_T, int VEC>
__global__ __launch_bounds__(DC_BLOCK) void decomposed_bwd_cl_kernel(
    const void* __restrict__ g, bool g_bf16, const float* __restrict__ sw,
    const float* __restrict__ mask, const float* __restrict__ aw,
    const float* __restrict__ aw_kb, float* __restrict__ d_aw,
    float* __restrict__ dmask_part, float* __restrict__ datten_part, int rows,
    int C, int S, int KB, int nct, int nst, bool train, float l1, float lm,
    bool need_aw, bool need_mask, bool need_atten) {
  __shared__ float tile[DC_WAVES][DC_CT * DC_PITCH];
  __shared__ float red[DC_WAVES][DC_KMAX];
  const int lane = threadIdx.x & (kWave - 1);
  float* t = tile[threadIdx.x / kWave];
  const DcClTask tk = dc_cl_task(rows, C, S, nct, nst);

  // phase 1: dθ/sw/aw in their own layout (lane = channel): d_aw, the
  // d_mask partial, and the dθ tile staged in LDS
  float dm = 0.f;
  if (tk.valid && lane < tk.ct_n) {
    for (int ss = 0; ss < tk.st_n; ++ss) {
      const int64_t p =
          ((int64_t)tk.row * S + tk.s0 + ss) * C + tk.c0 + lane;
      float gv[1];
      dc_load_any<1>(g, p, g_bf16, gv);
      if (need_aw)
        d_aw[p] = (!train || fabsf(aw[p]) > l1) ? gv[0] : 0.f;
      if (need_mask) dm = fmaf(gv[0], sw[p], dm);
      if (need_atten) t[lane * tk.pitch + ss] = gv[0];
    }
  }
  if (need_mask) {
    dm = wave_reduce_sum(dm);
    if (tk.valid && lane == 0) {
      const bool keep = !train || fabsf(mask[tk.row]) > lm;
      const int64_t task =
          (int64_t)blockIdx.x * DC_WAVES + (int)(threadIdx.x / kWave);
      dmask_part[task] = keep ? dm : 0.f;
    }
  }
  if (!need_atten) return;  // block-uniform
  __syncthreads();

  // phase 2: aw_kb in its [c][s] order against the staged dθ tile
  const int n = tk.valid ? tk.ct_n * tk.st_n : 0;
  const int npass = KB_T > 0 ? 1 : (KB + DC_KMAX - 1) / DC_KMAX;
  for (int pass = 0; pass < npass; ++pass) {
    const int k0 = pass * DC_KMAX;
    const int kc = KB_T > 0 ? KB_T : min(DC_KMAX, KB - k0);
    float acc[DC_KMAX];
#pragma unroll
    for (int k = 0; k < DC_KMAX; ++k) acc[k] = 0.f;
    for (int l = lane * VEC; l < n; l += kWave * VEC) {
      float gv[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i)
        gv[i] = t[dc_tile_word(l + i, tk.st_n, tk.pitch)];
      dc_kb_acc<KB_T, VEC>(aw_kb + dc_cl_kb_elem<VEC>(tk, l, C, S) * KB, gv,
                           KB, k0, kc, acc);
    }
    dc_block_atten_partial(acc, k0, kc, KB, red, datten_part);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

static bool dc_aligned16(const void* p) {
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

struct DcPlan {
  int inner, nct, nst, tpr;
  int64_t blocks;
};

static DcPlan dc_plan(int64_t rows, int64_t C, int64_t S, int channels_last) {
  if (rows < 1 || C < 1 || S < 1 || C * S >= (int64_t)1 << 31 ||
      rows >= (int64_t)1 << 31)
    throw std::runtime_error("decomposed: shape out of range");
  DcPlan p;
  p.inner = (int)(C * S);
  p.nct = (int)((C + DC_CT - 1) / DC_CT);
  p.nst = (int)((S + DC_ST - 1) / DC_ST);
  const int64_t tpr = channels_last ? (int64_t)p.nct * p.nst
                                    : (p.inner + DC_CHUNK - 1) / DC_CHUNK;
  const int64_t blocks = (rows * tpr + DC_WAVES - 1) / DC_WAVES;
  if (blocks >= (int64_t)1 << 31)
    throw std::runtime_error("decomposed: grid too large");
  p.tpr = (int)tpr;
  p.blocks = blocks;
  return p;
}

// workspace geometry for the wrapper: dmask_part is [rows][tasks_per_row],
// datten_part is [blocks][KB]
extern "C" void flreid_decomposed_plan(int64_t rows, int64_t C, int64_t S,
                                       int channels_last,
                                       int64_t* tasks_per_row,
                                       int64_t* blocks) {
  const DcPlan p = dc_plan(rows, C, S, channels_last);
  *tasks_per_row = p.tpr;
  *blocks = p.blocks;
}

#define DC_KB_SWITCH(KB, CALL)                       \
  switch (KB) {                                      \
    case 1: CALL(1); break;                          \
    case 2: CALL(2); break;                          \
    case 3: CALL(3); break;                          \
    case 4: CALL(4); break;                          \
    case 5: CALL(5); break;                          \
    case 6: CALL(6); break;                          \
    case 7: CALL(7); break;                          \
    case 8: CALL(8); break;                          \
    default: CALL(0); break;                         \
  }

extern "C" void flreid_decomposed_fwd(
    const float* sw, const float* mask, const float* aw, const float* aw_kb,
    const float* atten, void* out, int64_t rows, int64_t C, int64_t S,
    int64_t KB, int channels_last, int train, float lambda_l1,
    float lambda_mask, int out_dtype, hipStream_t stream) {
  if (KB < 1 || KB >= (int64_t)1 << 31)
    throw std::runtime_error("decomposed_fwd: KB out of range");
  if (out_dtype != kF32 && out_dtype != kBF16)
    throw std::runtime_error("decomposed_fwd: unsupported output dtype");
  const DcPlan p = dc_plan(rows, C, S, channels_last);
  const dim3 grid((unsigned)p.blocks), block(DC_BLOCK);
  const bool bf16 = out_dtype == kBF16;
  const int kb = (int)KB;
  if (!channels_last) {
    const bool vec = p.inner % 4 == 0 && dc_aligned16(sw) &&
                     dc_aligned16(aw) && dc_aligned16(aw_kb) &&
                     dc_aligned16(out);
#define DC_CALL(K)                                                           \
  if (vec)                                                                   \
    hipLaunchKernelGGL((decomposed_fwd_contig_kernel<K, 4>), grid, block, 0, \
                       stream, sw, mask, aw, aw_kb, atten, out, (int)rows,   \
                       p.inner, kb, p.tpr, train != 0, lambda_l1,            \
                       lambda_mask, bf16);                                   \
  else                                                                       \
    hipLaunchKernelGGL((decomposed_fwd_contig_kernel<K, 1>), grid, block, 0, \
                       stream, sw, mask, aw, aw_kb, atten, out, (int)rows,   \
                       p.inner, kb, p.tpr, train != 0, lambda_l1,            \
                       lambda_mask, bf16)
    DC_KB_SWITCH(kb, DC_CALL)
#undef DC_CALL
  } else {
    const bool vec = p.nst == 1 && C % 4 == 0 && dc_aligned16(aw_kb);
#define DC_CALL(K)                                                           \
  if (vec)                                                                   \
    hipLaunchKernelGGL((decomposed_fwd_cl_kernel<K, 4>), grid, block, 0,     \
                       stream, sw, mask, aw, aw_kb, atten, out, (int)rows,   \
                       (int)C, (int)S, kb, p.nct, p.nst, train != 0,         \
                       lambda_l1, lambda_mask, bf16);                        \
  else                                                                       \
    hipLaunchKernelGGL((decomposed_fwd_cl_kernel<K, 1>), grid, block, 0,     \
                       stream, sw, mask, aw, aw_kb, atten, out, (int)rows,   \
                       (int)C, (int)S, kb, p.nct, p.nst, train != 0,         \
                       lambda_l1, lambda_mask, bf16)
    DC_KB_SWITCH(kb, DC_CALL)
#undef DC_CALL
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_decomposed_bwd(
    const void* g, int g_dtype, const float* sw, const float* mask,
    const float* aw, const float* aw_kb, float* d_aw, float* dmask_part,
    float* datten_part, int64_t rows, int64_t C, int64_t S, int64_t KB,
    int channels_last, int train, float lambda_l1, float lambda_mask,
    int need_aw, int need_mask, int need_atten, hipStream_t stream) {
  if (KB < 1 || KB >= (int64_t)1 << 31)
    throw std::runtime_error("decomposed_bwd: KB out of range");
  if (g_dtype != kF32 && g_dtype != kBF16)
    throw std::runtime_error("decomposed_bwd: unsupported grad dtype");
  if ((need_aw && !d_aw) || (need_mask && !dmask_part) ||
      (need_atten && !datten_part))
    throw std::runtime_error("decomposed_bwd: missing output buffer");
  if (!need_aw && !need_mask && !need_atten) return;
  const DcPlan p = dc_plan(rows, C, S, channels_last);
  const dim3 grid((unsigned)p.blocks), block(DC_BLOCK);
  const bool bf16 = g_dtype == kBF16;
  const int kb = (int)KB;
  if (!channels_last) {
    const bool vec = p.inner % 4 == 0 && dc_aligned16(g) &&
                     dc_aligned16(sw) && dc_aligned16(aw) &&
                     dc_aligned16(aw_kb) && dc_aligned16(d_aw);
#define DC_CALL(K)                                                           \
  if (vec)                                                                   \
    hipLaunchKernelGGL((decomposed_bwd_contig_kernel<K, 4>), grid, block, 0, \
                       stream, g, bf16, sw, mask, aw, aw_kb, d_aw,           \
                       dmask_part, datten_part, (int)rows, p.inner, kb,      \
                       p.tpr, train != 0, lambda_l1, lambda_mask,            \
                       need_aw != 0, need_mask != 0, need_atten != 0);       \
  else                                                                       \
    hipLaunchKernelGGL((decomposed_bwd_contig_kernel<K, 1>), grid, block, 0, \
                       stream, g, bf16, sw, mask, aw, aw_kb, d_aw,           \
                       dmask_part, datten_part, (int)rows, p.inner, kb,      \
                       p.tpr, train != 0, lambda_l1, lambda_mask,            \
                       need_aw != 0, need_mask != 0, need_atten != 0)
    DC_KB_SWITCH(kb, DC_CALL)
#undef DC_CALL
  } else {
    const bool vec = p.nst == 1 && C % 4 == 0 && dc_aligned16(aw_kb);
#define DC_CALL(K)                                                           \
  if (vec)                                                                   \
    hipLaunchKernelGGL((decomposed_bwd_cl_kernel<K, 4>), grid, block, 0,     \
                       stream, g, bf16, sw, mask, aw, aw_kb, d_aw,           \
                       dmask_part, datten_part, (int)rows, (int)C, (int)S,   \
                       kb, p.nct, p.nst, train != 0, lambda_l1, lambda_mask, \
                       need_aw != 0, need_mask != 0, need_atten != 0);       \
  else                                                                       \
    hipLaunchKernelGGL((decomposed_bwd_cl_kernel<K, 1>), grid, block, 0,     \
                       stream, g, bf16, sw, mask, aw, aw_kb, d_aw,           \
                       dmask_part, datten_part, (int)rows, (int)C, (int)S,   \
                       kb, p.nct, p.nst, train != 0, lambda_l1, lambda_mask, \
                       need_aw != 0, need_mask != 0, need_atten != 0)
    DC_KB_SWITCH(kb, DC_CALL)
#undef DC_CALL
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

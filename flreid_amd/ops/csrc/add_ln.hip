// K4b: residual add + LayerNorm for the Swin blocks, forward and backward.
//
// models/swin.py runs, between its attention and MLP GEMMs, the row passes
//   s = a + b,  y = LN(s)·γ + β
// where the stream a is fp32 under bf16 autocast (LayerNorm is an fp32 op),
// the branch b is the bf16 output of a Linear and y feeds the next Linear,
// which wants bf16.  Eager torch moves the stream through an add kernel, an
// fp32 LN and a cast; here one pass reads a and b once, writes s in a's dtype
// and y in the dtype its consumer reads, and saves mean / rstd.  The backward
// is one pass too: ds = ds_in + LNbwd(dy), dγ / dβ as per-block partials.
//
// Geometry.  The unit is a CHUNK of 8 consecutive columns: one 16-byte access
// of a bf16 tensor, two of an fp32 one, so a lane owns the same columns of
// every operand whatever the dtypes.  A row of NC = C / 8 chunks goes to a
// group of G = 8, 16, 32 or 64 lanes, the narrowest with ceil(NC / G) <= 3;
// lane l of the group holds chunks l, l + G, l + 2G in registers (K of them,
// at most 24 values) from the load to the last store: nothing is read twice.
//   C =  96: G =  8, K = 2, 8 rows a wave      C =  768: G = 32, K = 3
//   C = 192: G =  8, K = 3                     C = 1536: G = 64, K = 3
//   C = 384: G = 16, K = 3
// A 256-thread block covers 256 / G rows per step of a grid-stride loop; the
// grid is capped (flreid_add_ln_blocks) so γ, β and the backward's dγ / dβ
// accumulators are loaded / reduced once per block and not once per row.
// Row reductions are xor butterflies inside the group (every lane ends with
// the sum, no broadcast).  Variance is that of the centred values, see
// patch_merge.hip.
//
// dγ / dβ: lane l of EVERY group holds the same columns, so a lane adds its
// rows' terms in registers, a second xor butterfly (offsets G .. 32) adds the
// groups of a wave, the four waves meet in LDS and are added in wave order:
// one [C] partial per block, no atomics, the same bits every run.
//
// dtypes are runtime tags, not template parameters: the branch is uniform
// over the launch and costs nothing beside the memory traffic, and 12
// (G, K) instances per direction stand in for 144.

#include <initializer_list>

#include "common.h"
#include "ops.h"

namespace flreid {

namespace {

constexpr int kAlnBlock = 256;
constexpr int kAlnMaxC = 1536;
constexpr int kAlnGridCap = 1024;   // 4 blocks on each of 256 CUs

__device__ __forceinline__ float aln_bf16_lo(uint32_t w) {
  return __uint_as_float(w << 16);
}
__device__ __forceinline__ float aln_bf16_hi(uint32_t w) {
  return __uint_as_float(w & 0xffff0000u);
}
__device__ __forceinline__ float aln_round_bf16(float v) {
  return __bfloat162float(__float2bfloat16(v));
}
// two values that ARE bf16 numbers (aln_round_bf16) into one word
__device__ __forceinline__ uint32_t aln_pack(float lo, float hi) {
  return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u);
}

// columns [off, off + 8) of a row-major tensor, off % 8 == 0
__device__ __forceinline__ void aln_load8(const void* p, int dtype,
                                          int64_t off, float (&v)[8]) {
  if (dtype == kF32) {
    const float4* q =
        reinterpret_cast<const float4*>(static_cast<const float*>(p) + off);
    const float4 a = q[0], b = q[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
    const uint4 r = *reinterpret_cast<const uint4*>(
        static_cast<const uint16_t*>(p) + off);
    v[0] = aln_bf16_lo(r.x); v[1] = aln_bf16_hi(r.x);
    v[2] = aln_bf16_lo(r.y); v[3] = aln_bf16_hi(r.y);
    v[4] = aln_bf16_lo(r.z); v[5] = aln_bf16_hi(r.z);
    v[6] = aln_bf16_lo(r.w); v[7] = aln_bf16_hi(r.w);
  }
}

// bf16: rounds to nearest even on the way out
__device__ __forceinline__ void aln_store8(void* p, int dtype, int64_t off,
                                           const float (&v)[8]) {
  if (dtype == kF32) {
    float4* q = reinterpret_cast<float4*>(static_cast<float*>(p) + off);
    q[0] = make_float4(v[0], v[1], v[2], v[3]);
    q[1] = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    float r[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = aln_round_bf16(v[i]);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(p) + off) =
        make_uint4(aln_pack(r[0], r[1]), aln_pack(r[2], r[3]),
                   aln_pack(r[4], r[5]), aln_pack(r[6], r[7]));
  }
}

// sum over the G lanes of a group; every lane receives it
template <int G>
__device__ __forceinline__ float aln_group_sum(float v) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// sum over the lanes of a wave that hold the same columns (l, l + G, ...)
template <int G>
__device__ __forceinline__ float aln_across_groups(float v) {
#pragma unroll
  for (int off = G; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int G, int K>
__global__ __launch_bounds__(kAlnBlock) void add_ln_fwd_kernel(
    const void* __restrict__ A, const void* __restrict__ B,
    const float* __restrict__ GAMMA, const float* __restrict__ BETA,
    void* __restrict__ S, void* __restrict__ Y, float* __restrict__ MEAN,
    float* __restrict__ RSTD, int64_t rows, int C, float eps, int a_dtype,
    int b_dtype, int y_dtype) {
  constexpr int RPB = kAlnBlock / G;
  const int lane = threadIdx.x % G;
  const int grp = threadIdx.x / G;
  const int nc = C >> 3;
  const float fc = (float)C;

  bool on[K];
  float gam[K][8], bet[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = lane + k * G;
    on[k] = ch < nc;
    if (on[k]) {
      aln_load8(GAMMA, kF32, (int64_t)ch * 8, gam[k]);
      aln_load8(BETA, kF32, (int64_t)ch * 8, bet[k]);
    }
  }

  for (int64_t base = (int64_t)blockIdx.x * RPB; base < rows;
       base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + grp;
    const bool live = row < rows;
    const int64_t roff = row * C;
    float x[K][8];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t off = roff + (int64_t)(lane + k * G) * 8;
      if (live && on[k]) {
        aln_load8(A, a_dtype, off, x[k]);
        if (B != nullptr) {
          float b[8];
          aln_load8(B, b_dtype, off, b);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            x[k][i] += b[i];
            // the statistics are those of the STORED stream
            if (a_dtype == kBF16) x[k][i] = aln_round_bf16(x[k][i]);
          }
          aln_store8(S, a_dtype, off, x[k]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) x[k][i] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) sum += x[k][i];
    }
    const float mean = aln_group_sum<G>(sum) / fc;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        x[k][i] = on[k] ? x[k][i] - mean : 0.f;
        sq += x[k][i] * x[k][i];
      }
    }
    const float rstd = rsqrtf(aln_group_sum<G>(sq) / fc + eps);
    if (live && lane == 0 && MEAN != nullptr) {
      MEAN[row] = mean;
      RSTD[row] = rstd;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (live && on[k]) {
        float y[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          y[i] = x[k][i] * rstd * gam[k][i] + bet[k][i];
        aln_store8(Y, y_dtype, roff + (int64_t)(lane + k * G) * 8, y);
      }
    }
  }
}

// S is the saved stream (a's dtype), DY the gradient of y (y's dtype, may be
// null), DS_IN the gradient that reaches s directly (a's dtype, may be null).
// DS receives the sum in a's dtype, DS_B (may be null) the same values in
// b_dtype.  AFFINE: DG_PART / DB_PART [gridDim.x][C].
template <int G, int K, bool AFFINE>
__global__ __launch_bounds__(kAlnBlock) void add_ln_bwd_kernel(
    const void* __restrict__ S, const float* __restrict__ GAMMA,
    const float* __restrict__ MEAN, const float* __restrict__ RSTD,
    const void* __restrict__ DY, const void* __restrict__ DS_IN,
    void* __restrict__ DS, void* __restrict__ DS_B,
    float* __restrict__ DG_PART, float* __restrict__ DB_PART, int64_t rows,
    int C, int a_dtype, int b_dtype, int y_dtype) {
  constexpr int RPB = kAlnBlock / G;
  __shared__ float red[AFFINE ? (kAlnBlock / kWave) * kAlnMaxC : 1];
  const int lane = threadIdx.x % G;
  const int grp = threadIdx.x / G;
  const int nc = C >> 3;
  const float fc = (float)C;

  bool on[K];
  float gam[K][8], dg[K][8], db[K][8];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int ch = lane + k * G;
    on[k] = ch < nc;
    if (on[k]) aln_load8(GAMMA, kF32, (int64_t)ch * 8, gam[k]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (!on[k]) gam[k][i] = 0.f;
      dg[k][i] = 0.f;
      db[k][i] = 0.f;
    }
  }

  for (int64_t base = (int64_t)blockIdx.x * RPB; base < rows;
       base += (int64_t)gridDim.x * RPB) {
    const int64_t row = base + grp;
    const bool live = row < rows;
    const int64_t roff = row * C;
    const float mean = live ? MEAN[row] : 0.f;
    const float rstd = live ? RSTD[row] : 0.f;
    float xh[K][8], dy[K][8];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t off = roff + (int64_t)(lane + k * G) * 8;
#pragma unroll
      for (int i = 0; i < 8; ++i) xh[k][i] = dy[k][i] = 0.f;
      if (live && on[k]) {
        aln_load8(S, a_dtype, off, xh[k]);
        if (DY != nullptr) aln_load8(DY, y_dtype, off, dy[k]);
#pragma unroll
        for (int i = 0; i < 8; ++i) xh[k][i] = (xh[k][i] - mean) * rstd;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float g = gam[k][i] * dy[k][i];
        m1 += g;
        m2 += g * xh[k][i];
        if (AFFINE) {
          dg[k][i] += dy[k][i] * xh[k][i];
          db[k][i] += dy[k][i];
        }
      }
    }
    m1 = aln_group_sum<G>(m1) / fc;
    m2 = aln_group_sum<G>(m2) / fc;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (!(live && on[k])) continue;
      const int64_t off = roff + (int64_t)(lane + k * G) * 8;
      float d[8];
#pragma unroll
      for (int i = 0; i < 8; ++i)
        d[i] = (gam[k][i] * dy[k][i] - m1 - xh[k][i] * m2) * rstd;
      if (DS_IN != nullptr) {
        float r[8];
        aln_load8(DS_IN, a_dtype, off, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] += r[i];
      }
      aln_store8(DS, a_dtype, off, d);
      if (DS_B != nullptr) aln_store8(DS_B, b_dtype, off, d);
    }
  }

  if (AFFINE) {
    // groups of a wave by butterfly, then the waves through LDS in wave
    // order; dγ first, dβ through the same buffer
    const int wave = threadIdx.x / kWave;
    const int wl = threadIdx.x % kWave;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          t[i] = aln_across_groups<G>(pass == 0 ? dg[k][i] : db[k][i]);
        if (wl < G && on[k]) {
          float4* q = reinterpret_cast<float4*>(red + wave * kAlnMaxC +
                                                (lane + k * G) * 8);
          q[0] = make_float4(t[0], t[1], t[2], t[3]);
          q[1] = make_float4(t[4], t[5], t[6], t[7]);
        }
      }
      __syncthreads();
      float* out = (pass == 0 ? DG_PART : DB_PART) + (int64_t)blockIdx.x * C;
      for (int v = threadIdx.x; v < (C >> 2); v += kAlnBlock) {
        float4 acc = reinterpret_cast<const float4*>(red)[v];
#pragma unroll
        for (int w = 1; w < kAlnBlock / kWave; ++w) {
          const float4 o =
              reinterpret_cast<const float4*>(red + w * kAlnMaxC)[v];
          acc.x += o.x; acc.y += o.y; acc.z += o.z; acc.w += o.w;
        }
        reinterpret_cast<float4*>(out)[v] = acc;
      }
      __syncthreads();
    }
  }
}

int aln_group(int C) {
  const int nc = C >> 3;
  for (int g = 8; g < 64; g <<= 1)
    if ((nc + g - 1) / g <= 3) return g;
  return 64;
}

void aln_check(const char* what, int64_t rows, int C,
               std::initializer_list<const void*> ptrs,
               std::initializer_list<int> dtypes) {
  if (rows < 1 || C < 8 || C > kAlnMaxC || C % 8)
    throw std::runtime_error(std::string(what) +
                             ": needs rows >= 1, C % 8 == 0, 8 <= C <= 1536");
  for (const void* p : ptrs)
    if (reinterpret_cast<uintptr_t>(p) % 16)
      throw std::runtime_error(std::string(what) +
                               ": pointers must be 16-byte aligned");
  for (int d : dtypes)
    if (d != kF32 && d != kBF16)
      throw std::runtime_error(std::string(what) + ": dtype tag");
}

}  // namespace

// (G, K) from C; `call` is instantiated for the 12 pairs
#define ALN_DISPATCH(C, call)                                         \
  do {                                                                \
    const int g_ = aln_group(C);                                      \
    const int k_ = ((C >> 3) + g_ - 1) / g_;                          \
    switch (g_ * 4 + k_) {                                            \
      case 8 * 4 + 1: call(8, 1); break;                              \
      case 8 * 4 + 2: call(8, 2); break;                              \
      case 8 * 4 + 3: call(8, 3); break;                              \
      case 16 * 4 + 1: call(16, 1); break;                            \
      case 16 * 4 + 2: call(16, 2); break;                            \
      case 16 * 4 + 3: call(16, 3); break;                            \
      case 32 * 4 + 1: call(32, 1); break;                            \
      case 32 * 4 + 2: call(32, 2); break;                            \
      case 32 * 4 + 3: call(32, 3); break;                            \
      case 64 * 4 + 1: call(64, 1); break;                            \
      case 64 * 4 + 2: call(64, 2); break;                            \
      case 64 * 4 + 3: call(64, 3); break;                            \
      default: throw std::runtime_error("add_ln: no instance");       \
    }                                                                 \
  } while (0)

extern "C" int flreid_add_ln_blocks(int64_t rows, int C) {
  if (rows < 1 || C < 8 || C > kAlnMaxC || C % 8) return 0;
  const int rpb = kAlnBlock / aln_group(C);
  const int64_t need = (rows + rpb - 1) / rpb;
  return (int)(need < kAlnGridCap ? need : kAlnGridCap);
}

extern "C" void flreid_add_ln_fwd(const void* a, const void* b,
                                  const float* gamma, const float* beta,
                                  void* s, void* y, float* mean, float* rstd,
                                  int64_t rows, int C, float eps, int a_dtype,
                                  int b_dtype, int y_dtype,
                                  hipStream_t stream) {
  aln_check("add_ln_fwd", rows, C, {a, b, gamma, beta, s, y},
            {a_dtype, b_dtype, y_dtype});
  if (a == nullptr || y == nullptr || gamma == nullptr || beta == nullptr ||
      (b != nullptr && s == nullptr) || (mean == nullptr) != (rstd == nullptr))
    throw std::runtime_error("add_ln_fwd: missing operand");
  dim3 grid((unsigned)flreid_add_ln_blocks(rows, C)), block(kAlnBlock);
#define ALN_FWD(G, K)                                                      \
  hipLaunchKernelGGL((add_ln_fwd_kernel<G, K>), grid, block, 0, stream, a, \
                     b, gamma, beta, s, y, mean, rstd, rows, C, eps,       \
                     a_dtype, b_dtype, y_dtype)
  ALN_DISPATCH(C, ALN_FWD);
#undef ALN_FWD
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_add_ln_bwd(const void* s, const float* gamma,
                                  const float* mean, const float* rstd,
                                  const void* dy, const void* ds_in, void* ds,
                                  void* ds_b, float* dg_part, float* db_part,
                                  int64_t rows, int C, int a_dtype,
                                  int b_dtype, int y_dtype, int affine,
                                  hipStream_t stream) {
  aln_check("add_ln_bwd", rows, C, {s, gamma, dy, ds_in, ds, ds_b, dg_part,
                                    db_part},
            {a_dtype, b_dtype, y_dtype});
  if (s == nullptr || gamma == nullptr || mean == nullptr ||
      rstd == nullptr || ds == nullptr ||
      (affine && (dg_part == nullptr || db_part == nullptr)))
    throw std::runtime_error("add_ln_bwd: missing operand");
  dim3 grid((unsigned)flreid_add_ln_blocks(rows, C)), block(kAlnBlock);
#define ALN_BWD_(G, K, AFF)                                                  \
  hipLaunchKernelGGL((add_ln_bwd_kernel<G, K, AFF>), grid, block, 0, stream, \
                     s, gamma, mean, rstd, dy, ds_in, ds, ds_b, dg_part,     \
                     db_part, rows, C, a_dtype, b_dtype, y_dtype)
#define ALN_BWD_ON(G, K) ALN_BWD_(G, K, true)
#define ALN_BWD_OFF(G, K) ALN_BWD_(G, K, false)
  if (affine) {
    ALN_DISPATCH(C, ALN_BWD_ON);
  } else {
    ALN_DISPATCH(C, ALN_BWD_OFF);
  }
#undef ALN_BWD_ON
#undef ALN_BWD_OFF
#undef ALN_BWD_
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

// Fused elementwise / row-reduction kernels for the ReID hot path.
//
//  - l2norm_rows:  y = x / max(||x||, eps) rowwise (K11 in SURVEY.md §2.9;
//                  replaces F.normalize in the eval feature path,
//                  ref:methods/fedavg.py:158-168)
//  - ce_label_smooth: fused log-softmax + smoothed NLL + analytic grad in one
//                  pass over the [B, C] score matrix (K6; the reference
//                  round-tripped a one-hot through the host every batch,
//                  ref:criterions/cross_entropy.py:36-38)
//  - adaptive_compose: theta = atten (bcast over last dim) * gw + aw (the
//                  FedSTIL composition, K1-prologue candidate; standalone
//                  fused form saves two full tensor passes vs mul+add)
//  - importance_sq/abs: F += g^2 or |g| (K9, EWC/MAS accumulation)
//
// All kernels: fp32 compute; bf16 or fp32 I/O.

#include "common.h"
#include "ops.h"

namespace flreid {

// --------------------------------------------------------------------------
// rowwise L2 normalize
// --------------------------------------------------------------------------

template <typename T, int BLOCK>
__global__ void l2norm_rows_kernel(const T* __restrict__ x, T* __restrict__ y,
                                   int64_t rows, int64_t cols, float eps) {
  __shared__ float scratch[BLOCK / kWave];
  const int64_t row = blockIdx.x;
  if (row >= rows) return;
  const T* xr = x + row * cols;
  T* yr = y + row * cols;

  float ss = 0.f;
  for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
    const float v = load_as_float(xr, c);
    ss += v * v;
  }
  const float total = block_reduce_sum<BLOCK>(ss, scratch);
  const float inv = 1.0f / fmaxf(sqrtf(total), eps);
  for (int64_t c = threadIdx.x; c < cols; c += BLOCK) {
    store_from_float(yr, c, load_as_float(xr, c) * inv);
  }
}

extern "C" void flreid_l2norm_rows(const void* x, void* y, int64_t rows,
                                   int64_t cols, int dtype, float eps,
                                   hipStream_t stream) {
  constexpr int BLOCK = 256;
  dim3 grid((unsigned)rows), block(BLOCK);
  if (dtype == kF32) {
    hipLaunchKernelGGL((l2norm_rows_kernel<float, BLOCK>), grid, block, 0,
                       stream, (const float*)x, (float*)y, rows, cols, eps);
  } else {
    hipLaunchKernelGGL((l2norm_rows_kernel<__hip_bfloat16, BLOCK>), grid,
                       block, 0, stream, (const __hip_bfloat16*)x,
                       (__hip_bfloat16*)y, rows, cols, eps);
  }
  HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------
// fused label-smooth CE: per-row loss + grad
//   loss_b = sum_c -t_bc * logp_bc,  t = (1-eps)*onehot + eps/C
//   grad_bc = (softmax_bc - t_bc) / B          (d(mean_b sum_c)/dscore)
// --------------------------------------------------------------------------

template <typename T, int BLOCK>
__global__ void ce_smooth_kernel(const T* __restrict__ score,
                                 const int64_t* __restrict__ target,
                                 float* __restrict__ row_loss,
                                 T* __restrict__ grad, int64_t B, int64_t C,
                                 float eps_smooth, float inv_B) {
  __shared__ float scratch[BLOCK / kWave];
  const int64_t b = blockIdx.x;
  if (b >= B) return;
  const T* s = score + b * C;
  T* g = grad + b * C;
  const int64_t y = target[b];
  const float uni = eps_smooth / (float)C;
  const float on = 1.0f - eps_smooth;

  // pass 1: max
  float m = -INFINITY;
  for (int64_t c = threadIdx.x; c < C; c += BLOCK) {
    m = fmaxf(m, load_as_float(s, c));
  }
  m = block_reduce_max(m, scratch, BLOCK);

  // pass 2: sum exp
  float se = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += BLOCK) {
    se += __expf(load_as_float(s, c) - m);
  }
  se = block_reduce_sum<BLOCK>(se, scratch);
  const float log_z = __logf(se) + m;
  const float inv_se = 1.0f / se;

  // pass 3: loss + grad
  float loss = 0.f;
  for (int64_t c = threadIdx.x; c < C; c += BLOCK) {
    const float sv = load_as_float(s, c);
    const float logp = sv - log_z;
    const float p = __expf(sv - m) * inv_se;
    const float t = uni + (c == y ? on : 0.0f);
    loss += -t * logp;
    store_from_float(g, c, (p - t) * inv_B);
  }
  loss = block_reduce_sum<BLOCK>(loss, scratch);
  if (threadIdx.x == 0) row_loss[b] = loss;
}

extern "C" void flreid_ce_smooth(const void* score, const int64_t* target,
                                 float* row_loss, void* grad, int64_t B,
                                 int64_t C, int dtype, float eps_smooth,
                                 hipStream_t stream) {
  constexpr int BLOCK = 256;
  dim3 grid((unsigned)B), block(BLOCK);
  const float inv_B = 1.0f / (float)B;
  if (dtype == kF32) {
    hipLaunchKernelGGL((ce_smooth_kernel<float, BLOCK>), grid, block, 0,
                       stream, (const float*)score, target, row_loss,
                       (float*)grad, B, C, eps_smooth, inv_B);
  } else {
    hipLaunchKernelGGL((ce_smooth_kernel<__hip_bfloat16, BLOCK>), grid, block,
                       0, stream, (const __hip_bfloat16*)score, target,
                       row_loss, (__hip_bfloat16*)grad, B, C, eps_smooth,
                       inv_B);
  }
  HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------
// FedSTIL composition: theta = atten * gw + aw (atten over the last dim)
// --------------------------------------------------------------------------

// compose2: layout-aware + mixed-dtype composition.  atten broadcasts over
// the LOGICAL last weight dim; for channels-last conv weights the physical
// index of that dim is (i / inner) % L (inner = C for [K][kh][kw][C]
// storage, 1 for linear weights).  Tout=bf16 with Tin=f32 produces the
// bf16 θ the MFMA conv/GEMM kernels consume directly — no autocast cast
// pass, θ never exists in fp32 HBM.
template <typename Tin, typename Tout>
__global__ void compose2_kernel(const Tin* __restrict__ gw,
                                const float* __restrict__ atten,
                                const Tin* __restrict__ aw,
                                Tout* __restrict__ out, int64_t numel,
                                int64_t L, int64_t inner) {
  // 4 elements per thread (vectorized when the 4-run stays inside one
  // atten-broadcast segment — always true for inner % 4 == 0 or L == 1):
  // the scalar form measured 0.37 TB/s in the bench trace (launch+issue
  // bound on the 13 per-step compositions)
  const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i0 >= numel) return;
  // linear weights (inner==1, atten over the contiguous last dim): the
  // 4-run reads 4 consecutive atten entries — vectorize those too
  if (i0 + 4 <= numel && atten && inner == 1 && L % 4 == 0 && L > 1) {
    const float4 a4 = *(const float4*)(atten + (i0 % L));
    float4 g, w = {0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(Tin) == 4) {
      g = *(const float4*)(gw + i0);
      if (aw) w = *(const float4*)(aw + i0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        (&g.x)[e] = load_as_float(gw, i0 + e);
        if (aw) (&w.x)[e] = load_as_float(aw, i0 + e);
      }
    }
    Tout v4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float r = fmaf((&a4.x)[e], (&g.x)[e], (&w.x)[e]);
      if constexpr (sizeof(Tout) == 4) {
        v4[e] = r;
      } else {
        v4[e] = __float2bfloat16(r);
      }
    }
    __builtin_memcpy(out + i0, v4, sizeof(v4));
    return;
  }
  if (i0 + 4 <= numel && (L == 1 || !atten || (inner % 4 == 0))) {
    const float a = atten ? atten[(i0 / inner) % L] : 1.0f;
    float4 g, w = {0.f, 0.f, 0.f, 0.f};
    if constexpr (sizeof(Tin) == 4) {
      g = *(const float4*)(gw + i0);
      if (aw) w = *(const float4*)(aw + i0);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        (&g.x)[e] = load_as_float(gw, i0 + e);
        if (aw) (&w.x)[e] = load_as_float(aw, i0 + e);
      }
    }
    Tout v4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float r = fmaf(a, (&g.x)[e], (&w.x)[e]);
      if constexpr (sizeof(Tout) == 4) {
        v4[e] = r;
      } else {
        v4[e] = __float2bfloat16(r);
      }
    }
    __builtin_memcpy(out + i0, v4, sizeof(v4));
    return;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int64_t i = i0 + e;
    if (i >= numel) return;
    const float a = atten ? atten[(i / inner) % L] : 1.0f;
    const float v = fmaf(a, load_as_float(gw, i),
                         aw ? load_as_float(aw, i) : 0.0f);
    store_from_float(out, i, v);
  }
}

extern "C" void flreid_compose2(const void* gw, const float* atten,
                                const void* aw, void* out, int64_t numel,
                                int64_t L, int64_t inner, int in_dtype,
                                int out_dtype, hipStream_t stream) {
  constexpr int BLOCK = 256;
  dim3 grid((unsigned)((numel + BLOCK * 4 - 1) / (BLOCK * 4))), block(BLOCK);
  if (in_dtype == kF32 && out_dtype == kBF16) {
    hipLaunchKernelGGL((compose2_kernel<float, __hip_bfloat16>), grid, block,
                       0, stream, (const float*)gw, atten, (const float*)aw,
                       (__hip_bfloat16*)out, numel, L, inner);
  } else if (in_dtype == kF32 && out_dtype == kF32) {
    hipLaunchKernelGGL((compose2_kernel<float, float>), grid, block, 0,
                       stream, (const float*)gw, atten, (const float*)aw,
                       (float*)out, numel, L, inner);
  } else if (in_dtype == kBF16 && out_dtype == kBF16) {
    hipLaunchKernelGGL((compose2_kernel<__hip_bfloat16, __hip_bfloat16>),
                       grid, block, 0, stream, (const __hip_bfloat16*)gw,
                       atten, (const __hip_bfloat16*)aw,
                       (__hip_bfloat16*)out, numel, L, inner);
  } else {
    throw std::runtime_error("compose2: unsupported dtype combination");
  }
  HIP_CHECK(hipGetLastError());
}

// --------------------------------------------------------------------------
// EWC/MAS importance accumulation: F += g*g (sq) or F += |g| * scale
// --------------------------------------------------------------------------

template <typename T, bool SQ>
__global__ void importance_kernel(float* __restrict__ F,
                                  const T* __restrict__ g, int64_t numel,
                                  float scale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numel) return;
  const float gv = load_as_float(g, i);
  F[i] += SQ ? gv * gv * scale : fabsf(gv) * scale;
}

extern "C" void flreid_importance(float* F, const void* g, int64_t numel,
                                  int dtype, int sq, float scale,
                                  hipStream_t stream) {
  constexpr int BLOCK = 256;
  dim3 grid((unsigned)((numel + BLOCK - 1) / BLOCK)), block(BLOCK);
  if (dtype == kF32) {
    if (sq)
      hipLaunchKernelGGL((importance_kernel<float, true>), grid, block, 0,
                         stream, F, (const float*)g, numel, scale);
    else
      hipLaunchKernelGGL((importance_kernel<float, false>), grid, block, 0,
                         stream, F, (const float*)g, numel, scale);
  } else {
    if (sq)
      hipLaunchKernelGGL((importance_kernel<__hip_bfloat16, true>), grid,
                         block, 0, stream, F, (const __hip_bfloat16*)g, numel,
                         scale);
    else
      hipLaunchKernelGGL((importance_kernel<__hip_bfloat16, false>), grid,
                         block, 0, stream, F, (const __hip_bfloat16*)g, numel,
                         scale);
  }
  HIP_CHECK(hipGetLastError());
}


// --------------------------------------------------------------------------
// eval-mode BatchNorm2d: y = (x − μ[c])·rsqrt(σ²[c]+eps)·γ[c] + β[c]
// One bandwidth-bound pass (MIOpen's inference kernel measured ~0.3 TB/s on
// ReID shapes; this is a plain coalesced elementwise).  layout 0 = NCHW
// (c = i/(HW) % C), 1 = NHWC/channels-last (c = i % C).
// --------------------------------------------------------------------------

template <typename T, bool NHWC>
__global__ void bn_eval_kernel(const T* __restrict__ x, T* __restrict__ y,
                               const float* __restrict__ gamma,
                               const float* __restrict__ beta,
                               const float* __restrict__ mean,
                               const float* __restrict__ var, int64_t numel,
                               int C, int64_t HW, float eps, int relu) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= numel) return;
  const int c = NHWC ? (int)(i % C) : (int)((i / HW) % C);
  const float inv = __frsqrt_rn(var[c] + eps);
  float v = (load_as_float(x, i) - mean[c]) * inv * gamma[c] + beta[c];
  if (relu) v = fmaxf(v, 0.f);
  store_from_float(y, i, v);
}

extern "C" void flreid_bn_eval(const void* x, void* y, const float* gamma,
                               const float* beta, const float* mean,
                               const float* var, int64_t numel, int C,
                               int64_t HW, float eps, int nhwc, int relu,
                               int dtype, hipStream_t stream) {
  constexpr int BLOCK = 256;
  dim3 grid((unsigned)((numel + BLOCK - 1) / BLOCK)), block(BLOCK);
  if (dtype == kF32) {
    if (nhwc)
      hipLaunchKernelGGL((bn_eval_kernel<float, true>), grid, block, 0, stream,
                         (const float*)x, (float*)y, gamma, beta, mean, var,
                         numel, C, HW, eps, relu);
    else
      hipLaunchKernelGGL((bn_eval_kernel<float, false>), grid, block, 0,
                         stream, (const float*)x, (float*)y, gamma, beta, mean,
                         var, numel, C, HW, eps, relu);
  } else {
    if (nhwc)
      hipLaunchKernelGGL((bn_eval_kernel<__hip_bfloat16, true>), grid, block,
                         0, stream, (const __hip_bfloat16*)x,
                         (__hip_bfloat16*)y, gamma, beta, mean, var, numel, C,
                         HW, eps, relu);
    else
      hipLaunchKernelGGL((bn_eval_kernel<__hip_bfloat16, false>), grid, block,
                         0, stream, (const __hip_bfloat16*)x,
                         (__hip_bfloat16*)y, gamma, beta, mean, var, numel, C,
                         HW, eps, relu);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

// Fused training-mode BatchNorm2d over NHWC rows (K1-adjacent hot op): the
// two-launch pair.  bn_onepass.hip does the same arithmetic (bn_train.h) in
// one launch per direction where the rows fit in registers; this pair is the
// path for larger M and fp32, and the reference the one-launch kernels are
// tested against bit for bit.
//
// MIOpen's train BN on the FedSTIL head-epoch shapes (M = N·H·W = 2048 rows,
// C ∈ {512, 1024, 2048}) costs 5 kernels per layer per direction
// (MeanVariance, FinalMeanVariance, Norm / DScaleDBias, DX) plus
// SubTensorOp casts and an fp32 autocast round-trip of the activation —
// measured ≈900 µs per training step for the 10 layer4 BNs
// (profiles/README.md).  This replaces each direction with TWO kernels:
//
//   k1  partial:   grid (C/64, NSLAB) — every block reduces its row slab to
//                  64-channel partial sums (LDS tree), written densely to a
//                  workspace [NSLAB, C] (no atomics → deterministic, and no
//                  zeroing pass: every slot is overwritten every call).
//   k2  finalize:  same grid — every block re-reduces the (tiny) partial
//                  array for its channel group, then normalizes its own
//                  slab; the slab-0 block additionally writes save_mean /
//                  save_invstd and the running-stat update (fused — no
//                  SubTensorOp casts).  bf16 activations never round-trip
//                  through fp32 HBM copies.
//
// A first single-kernel version (one block per 64 channels doing the whole
// column reduction) filled only C/64 ≤ 32 of the 256 CUs and measured SLOWER
// than the MIOpen chain — the split-row grid is the fix: C/64 × NSLAB blocks
// cover the chip and every traversal runs at full bandwidth.
//
// Layout: x viewed as [M, C] NHWC rows; each thread owns 4 consecutive
// channels (8 B vector loads) × its block's row stripes.
//
// Semantics match torch.nn.BatchNorm2d(train): biased batch var for the
// normalisation, unbiased (·M/(M−1)) for the running-var update
// (ref models the same torch module family: ref:models/resnet.py).

#include "bn_train.h"
#include "common.h"
#include "ops.h"

namespace flreid {

// Two per-channel f32 accumulators reduced across a block's stripes:
// fwd uses (Σx, Σx²); bwd uses (Σdy, Σ dy·x̂).
template <typename T, bool IS_BWD>
__global__ __launch_bounds__(256) void bn_partial_kernel(
    const T* __restrict__ X, const T* __restrict__ DY,
    const float* __restrict__ smean, const float* __restrict__ sinv,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ part_a, float* __restrict__ part_b, int64_t M,
    int C, int relu) {
  const int c0 = blockIdx.x * BN_CG;
  const int q = threadIdx.x & 15;       // channel quad within the group
  const int r = threadIdx.x >> 4;       // stripe within the block
  const int c = c0 + q * 4;
  const int S = gridDim.y * BN_STRIPES; // total stripes across slabs
  const int g = blockIdx.y * BN_STRIPES + r;

  __shared__ float la[BN_STRIPES][BN_CG + 4];
  __shared__ float lb[BN_STRIPES][BN_CG + 4];

  float mn[4], iv[4], sc[4], sh[4];
  if (IS_BWD) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mn[j] = smean[c + j];
      iv[j] = sinv[c + j];
      if (relu)                      // recompute pre-relu output sign
        bn_scale_shift(gamma[c + j], beta[c + j], mn[j], iv[j], sc[j], sh[j]);
    }
  }

  float sa[4] = {0.f, 0.f, 0.f, 0.f};
  float sb[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t row = g; row < M; row += S) {
    float x[4];
    bn_load4(X + row * C + c, x);
    if (IS_BWD) {
      float dy[4];
      bn_load4(DY + row * C + c, dy);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (relu && bn_relu_off(x[j], sc[j], sh[j])) continue;  // dy masked
        bn_bwd_accum(sa[j], sb[j], dy[j], x[j], mn[j], iv[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) bn_fwd_accum(sa[j], sb[j], x[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    la[r][q * 4 + j] = sa[j];
    lb[r][q * 4 + j] = sb[j];
  }
  __syncthreads();
  if (threadIdx.x < BN_CG) {
    float ta = 0.f, tb = 0.f;
#pragma unroll
    for (int i = 0; i < BN_STRIPES; ++i) {
      ta += la[i][threadIdx.x];
      tb += lb[i][threadIdx.x];
    }
    const int64_t w = (int64_t)blockIdx.y * C + c0 + threadIdx.x;
    part_a[w] = ta;
    part_b[w] = tb;
  }
}

// ---------------------------------------------------------------- forward
template <typename T>
__global__ __launch_bounds__(256) void bn_finalize_fwd_kernel(
    const T* __restrict__ X, T* __restrict__ Y,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ rmean, float* __restrict__ rvar,
    float* __restrict__ smean, float* __restrict__ sinv,
    const float* __restrict__ part_a, const float* __restrict__ part_b,
    unsigned long long* __restrict__ nbt, int64_t M, int C, float momentum,
    float eps, float unbiased, int relu) {
  const int c0 = blockIdx.x * BN_CG;
  const int q = threadIdx.x & 15;
  const int r = threadIdx.x >> 4;
  const int c = c0 + q * 4;
  const int S = gridDim.y * BN_STRIPES;
  const int g = blockIdx.y * BN_STRIPES + r;
  const int nslab = gridDim.y;

  // num_batches_tracked update fused in (torch increments it per train call)
  if (nbt != nullptr && blockIdx.x == 0 && blockIdx.y == 0 &&
      threadIdx.x == 0) {
    ++(*nbt);
  }

  __shared__ float lmean[BN_CG], linv[BN_CG];
  if (threadIdx.x < BN_CG) {
    float ta = 0.f, tb = 0.f;
    for (int s = 0; s < nslab; ++s) {
      ta += part_a[(int64_t)s * C + c0 + threadIdx.x];
      tb += part_b[(int64_t)s * C + c0 + threadIdx.x];
    }
    float mean, var, inv;
    bn_fwd_stats(ta, tb, M, eps, mean, var, inv);
    lmean[threadIdx.x] = mean;
    linv[threadIdx.x] = inv;
    if (blockIdx.y == 0) {
      const int gc = c0 + threadIdx.x;
      smean[gc] = mean;
      sinv[gc] = inv;
      if (rmean != nullptr)
        bn_running_update(rmean[gc], rvar[gc], momentum, mean, var, unbiased);
    }
  }
  __syncthreads();

  float scale[4], shift[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    bn_scale_shift(gamma[c + j], beta[c + j], lmean[q * 4 + j],
                   linv[q * 4 + j], scale[j], shift[j]);
  for (int64_t row = g; row < M; row += S) {
    float v[4];
    bn_load4(X + row * C + c, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = bn_normalize(v[j], scale[j], shift[j], relu);
    bn_store4(Y + row * C + c, v);
  }
}

// --------------------------------------------------------------- backward
// dx = γ·invstd·(dy − Σdy/M − x̂·Σ(dy·x̂)/M);  dγ = Σ(dy·x̂);  dβ = Σdy
template <typename T>
__global__ __launch_bounds__(256) void bn_finalize_bwd_kernel(
    const T* __restrict__ X, const T* __restrict__ DY, T* __restrict__ DX,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ smean, const float* __restrict__ sinv,
    float* __restrict__ dgamma, float* __restrict__ dbeta,
    const float* __restrict__ part_a, const float* __restrict__ part_b,
    int64_t M, int C, int relu) {
  const int c0 = blockIdx.x * BN_CG;
  const int q = threadIdx.x & 15;
  const int r = threadIdx.x >> 4;
  const int c = c0 + q * 4;
  const int S = gridDim.y * BN_STRIPES;
  const int g = blockIdx.y * BN_STRIPES + r;
  const int nslab = gridDim.y;

  __shared__ float lmdy[BN_CG], lmdyx[BN_CG];
  if (threadIdx.x < BN_CG) {
    float tdy = 0.f, tdyx = 0.f;
    for (int s = 0; s < nslab; ++s) {
      tdy += part_a[(int64_t)s * C + c0 + threadIdx.x];
      tdyx += part_b[(int64_t)s * C + c0 + threadIdx.x];
    }
    if (blockIdx.y == 0) {
      const int gc = c0 + threadIdx.x;
      dgamma[gc] = tdyx;
      dbeta[gc] = tdy;
    }
    bn_bwd_means(tdy, tdyx, M, lmdy[threadIdx.x], lmdyx[threadIdx.x]);
  }
  __syncthreads();

  float g_iv[4], mn[4], iv[4], mdy[4], mdyx[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mn[j] = smean[c + j];
    iv[j] = sinv[c + j];
    bn_scale_shift(gamma[c + j], beta[c + j], mn[j], iv[j], g_iv[j], sh[j]);
    mdy[j] = lmdy[q * 4 + j];
    mdyx[j] = lmdyx[q * 4 + j];
  }
  for (int64_t row = g; row < M; row += S) {
    float x[4], dy[4], dx[4];
    bn_load4(X + row * C + c, x);
    bn_load4(DY + row * C + c, dy);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      dx[j] = bn_bwd_dx(x[j], dy[j], mn[j], iv[j], g_iv[j], sh[j], mdy[j],
                        mdyx[j], relu);
    bn_store4(DX + row * C + c, dx);
  }
}

// ----------------------------------------------------------------- launch
extern "C" int flreid_bn_train_nslab(int64_t M, int C) {
  return bn_nslab(M, C);
}

extern "C" void flreid_bn_train_fwd(const void* X, void* Y, const float* gamma,
                                    const float* beta, float* rmean,
                                    float* rvar, float* smean, float* sinv,
                                    float* part_a, float* part_b,
                                    unsigned long long* nbt, int64_t M, int C,
                                    float momentum, float eps, float unbiased,
                                    int relu, int dtype, hipStream_t stream) {
  if (C % BN_CG != 0) throw std::runtime_error("bn_train: C % 64 != 0");
  dim3 grid(C / BN_CG, bn_nslab(M, C)), block(256);
  if (dtype == kBF16) {
    hipLaunchKernelGGL((bn_partial_kernel<__hip_bfloat16, false>), grid,
                       block, 0, stream, (const __hip_bfloat16*)X, nullptr,
                       nullptr, nullptr, nullptr, nullptr, part_a, part_b, M,
                       C, 0);
    hipLaunchKernelGGL(bn_finalize_fwd_kernel<__hip_bfloat16>, grid, block, 0,
                       stream, (const __hip_bfloat16*)X, (__hip_bfloat16*)Y,
                       gamma, beta, rmean, rvar, smean, sinv, part_a, part_b,
                       nbt, M, C, momentum, eps, unbiased, relu);
  } else {
    hipLaunchKernelGGL((bn_partial_kernel<float, false>), grid, block, 0,
                       stream, (const float*)X, nullptr, nullptr, nullptr,
                       nullptr, nullptr, part_a, part_b, M, C, 0);
    hipLaunchKernelGGL(bn_finalize_fwd_kernel<float>, grid, block, 0, stream,
                       (const float*)X, (float*)Y, gamma, beta, rmean, rvar,
                       smean, sinv, part_a, part_b, nbt, M, C, momentum, eps,
                       unbiased, relu);
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_bn_train_bwd(const void* X, const void* DY, void* DX,
                                    const float* gamma, const float* beta,
                                    const float* smean, const float* sinv,
                                    float* dgamma, float* dbeta,
                                    float* part_a, float* part_b, int64_t M,
                                    int C, int relu, int dtype,
                                    hipStream_t stream) {
  if (C % BN_CG != 0) throw std::runtime_error("bn_train: C % 64 != 0");
  dim3 grid(C / BN_CG, bn_nslab(M, C)), block(256);
  if (dtype == kBF16) {
    hipLaunchKernelGGL((bn_partial_kernel<__hip_bfloat16, true>), grid, block,
                       0, stream, (const __hip_bfloat16*)X,
                       (const __hip_bfloat16*)DY, smean, sinv, gamma, beta,
                       part_a, part_b, M, C, relu);
    hipLaunchKernelGGL(bn_finalize_bwd_kernel<__hip_bfloat16>, grid, block, 0,
                       stream, (const __hip_bfloat16*)X,
                       (const __hip_bfloat16*)DY, (__hip_bfloat16*)DX, gamma,
                       beta, smean, sinv, dgamma, dbeta, part_a, part_b, M, C,
                       relu);
  } else {
    hipLaunchKernelGGL((bn_partial_kernel<float, true>), grid, block, 0,
                       stream, (const float*)X, (const float*)DY, smean, sinv,
                       gamma, beta, part_a, part_b, M, C, relu);
    hipLaunchKernelGGL(bn_finalize_bwd_kernel<float>, grid, block, 0, stream,
                       (const float*)X, (const float*)DY, (float*)DX, gamma,
                       beta, smean, sinv, dgamma, dbeta, part_a, part_b, M, C,
                       relu);
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

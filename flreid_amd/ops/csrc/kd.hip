// K7: fused knowledge-distillation losses.
//
// 1) kd_fwd — temperature-softmax KL (ref:criterions/kd_loss.py:10-27):
//      L = (T²/B) · Σ_b Σ_i p_t·(log p_t − log p_s),
//      p_s = softmax(z_s/T), p_t = softmax(z_t/T)
//    One block per row; three strided passes over the row (max, sumexp,
//    loss+grad) — the tensors are 64×C and L2-resident, so re-reading beats
//    register caching at arbitrary C.  The gradient
//      dL/dz_s = (T/B)·(p_s − p_t)
//    is produced in the same pass (the eager chain is 5 kernels + the
//    backward graph; this is 1 fwd + a scale in bwd).
//
// 2) icarl_distill — the iCaRL distillation step's TWO BCE-with-logits
//    losses fused into one pass (ref:methods/icarl.py:216-236):
//      clf     = mean_{b,c}  bce(x[b,c], onehot(target)[b,c])
//      distill = mean_{b,c<P} bce(x[b,c], sigmoid(prev[b,c]))
//    with the combined gradient written in the same pass:
//      g[b,c] = (σ(x)−y)/(B·C) + [c<P]·(σ(x)−σ(prev)))/(B·P)
//    bce(x,y) = max(x,0) − x·y + log1p(exp(−|x|)) (the stable form torch
//    uses).  Row-combined losses land in row_loss[b]; the wrapper sums.
//
// All inputs fp32 (the iCaRL pass upcasts under autocast; DistillKL logits
// are head outputs) — fp32 here is bit-comparable with the eager reference.

#include "common.h"
#include "ops.h"

namespace flreid {

constexpr int KD_BLOCK = 256;

__global__ __launch_bounds__(KD_BLOCK) void kd_fwd_kernel(
    const float* __restrict__ ZS, const float* __restrict__ ZT,
    float* __restrict__ ROW_LOSS, float* __restrict__ GRAD, int64_t C,
    float inv_t, float t_sq_over_b, float t_over_b) {
  __shared__ float scratch[KD_BLOCK / kWave];
  const int64_t row = blockIdx.x;
  const float* zs = ZS + row * C;
  const float* zt = ZT + row * C;
  float* grad = GRAD + row * C;

  float max_s = -INFINITY, max_t = -INFINITY;
  for (int64_t i = threadIdx.x; i < C; i += KD_BLOCK) {
    max_s = fmaxf(max_s, zs[i] * inv_t);
    max_t = fmaxf(max_t, zt[i] * inv_t);
  }
  max_s = block_reduce_max(max_s, scratch, KD_BLOCK);
  max_t = block_reduce_max(max_t, scratch, KD_BLOCK);

  float sum_s = 0.f, sum_t = 0.f;
  for (int64_t i = threadIdx.x; i < C; i += KD_BLOCK) {
    sum_s += __expf(zs[i] * inv_t - max_s);
    sum_t += __expf(zt[i] * inv_t - max_t);
  }
  sum_s = block_reduce_sum<KD_BLOCK>(sum_s, scratch);
  sum_t = block_reduce_sum<KD_BLOCK>(sum_t, scratch);
  const float log_sum_s = __logf(sum_s), log_sum_t = __logf(sum_t);
  const float rcp_s = 1.f / sum_s, rcp_t = 1.f / sum_t;

  float loss = 0.f;
  for (int64_t i = threadIdx.x; i < C; i += KD_BLOCK) {
    const float ls = zs[i] * inv_t - max_s;           // log p_s + log_sum_s
    const float lt = zt[i] * inv_t - max_t;
    const float p_s = __expf(ls) * rcp_s;
    const float p_t = __expf(lt) * rcp_t;
    loss += p_t * ((lt - log_sum_t) - (ls - log_sum_s));
    grad[i] = t_over_b * (p_s - p_t);
  }
  loss = block_reduce_sum<KD_BLOCK>(loss, scratch);
  if (threadIdx.x == 0) ROW_LOSS[row] = loss * t_sq_over_b;
}

extern "C" void flreid_kd_fwd(const float* zs, const float* zt,
                              float* row_loss, float* grad, int64_t B,
                              int64_t C, float temperature,
                              hipStream_t stream) {
  const float inv_t = 1.0f / temperature;
  const float t_sq_over_b = temperature * temperature / (float)B;
  const float t_over_b = temperature / (float)B;
  hipLaunchKernelGGL(kd_fwd_kernel, dim3((uint32_t)B), dim3(KD_BLOCK), 0,
                     stream, zs, zt, row_loss, grad, C, inv_t, t_sq_over_b,
                     t_over_b);
  HIP_CHECK(hipGetLastError());
}

__device__ __forceinline__ float bce_logits(float x, float y) {
  return fmaxf(x, 0.f) - x * y + log1pf(__expf(-fabsf(x)));
}

__global__ __launch_bounds__(KD_BLOCK) void icarl_distill_kernel(
    const float* __restrict__ SCORE, const int64_t* __restrict__ TARGET,
    const float* __restrict__ PREV, float* __restrict__ ROW_LOSS,
    float* __restrict__ GRAD, int64_t C, int64_t P, float inv_bc,
    float inv_bp) {
  __shared__ float scratch[KD_BLOCK / kWave];
  const int64_t row = blockIdx.x;
  const float* x = SCORE + row * C;
  const float* prev = PREV + row * P;
  float* grad = GRAD + row * C;
  const int64_t tgt = TARGET[row];

  float clf = 0.f, dis = 0.f;
  for (int64_t i = threadIdx.x; i < C; i += KD_BLOCK) {
    const float xi = x[i];
    const float sig_x = 1.f / (1.f + __expf(-xi));
    const float y = (i == tgt) ? 1.f : 0.f;
    clf += bce_logits(xi, y);
    float g = (sig_x - y) * inv_bc;
    if (i < P) {
      const float yt = 1.f / (1.f + __expf(-prev[i]));   // sigmoid(prev)
      dis += bce_logits(xi, yt);
      g += (sig_x - yt) * inv_bp;
    }
    grad[i] = g;
  }
  clf = block_reduce_sum<KD_BLOCK>(clf, scratch);
  dis = block_reduce_sum<KD_BLOCK>(dis, scratch);
  if (threadIdx.x == 0) ROW_LOSS[row] = clf * inv_bc + dis * inv_bp;
}

extern "C" void flreid_icarl_distill(const float* score, const int64_t* target,
                                     const float* prev, float* row_loss,
                                     float* grad, int64_t B, int64_t C,
                                     int64_t P, hipStream_t stream) {
  const float inv_bc = 1.0f / (float)(B * C);
  const float inv_bp = 1.0f / (float)(B * P);
  hipLaunchKernelGGL(icarl_distill_kernel, dim3((uint32_t)B), dim3(KD_BLOCK),
                     0, stream, score, target, prev, row_loss, grad, C, P,
                     inv_bc, inv_bp);
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

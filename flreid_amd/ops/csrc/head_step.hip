// One-pass FedSTIL head update: L1-drift gradient + Adam + next-step θ.
//
// Every head-training step used to walk the ~31 M fp32 adaptive weights
// many times: drift forward (read aw, aw0), drift backward (write a
// weight-sized sign buffer), AccumulateGrad (task grad + drift grad), torch's
// fused Adam (read aw/g/m/v, write aw/m/v) and — next step — compose2
// (read gw/aw, write bf16 θ).  Here each element is visited once:
//
//   d   = aw − aw0
//   g   = float(dw) + (d>0 ? λ : d<0 ? −λ : 0)          fp32, as AccumulateGrad
//   Adam, ORIGINAL mode, expression for expression as torch's
//   ATen/native/cuda/fused_adam_utils.cuh::adam_math<float> (the scalars are
//   double there, so the element math promotes to double and truncates to
//   float at each assignment; bias corrections are truncated to float)
//   θ   = bf16(fmaf(atten[(i/inner)%L], gw, aw_new))     as compose2_kernel
//   partial[block] = Σ|d|                                 pre-update weights
//
// The tensor table crosses BY VALUE as the kernel argument (like torch's
// multi-tensor apply): gradient buffers move from step to step in eager mode
// and are fixed capture-pool addresses inside a captured hipGraph, and a
// by-value table is right in both cases with no host→device copy inside
// capture.  The step count is a device float per tensor (torch's capturable
// layout), so a replayed graph advances it.
//
// Grid: 16 K-element chunks, 256 threads, 64 elements per thread — 31 M
// elements are ~1900 blocks, i.e. every block of the launch is resident at
// once on 256 CUs × 8 blocks (no second wave, no 64 K-chunk tail), and the
// two double pow() of the bias corrections amortise over 64 elements.
// The drift partial is accumulated and stored in double: the sum of the
// partials is then the correctly rounded drift, whatever the chunking.

#include "common.h"
#include "ops.h"

#include <vector>

namespace flreid {

constexpr int HS_BLOCK = 256;
constexpr int HS_CHUNK = 1 << 14;
constexpr int HS_MAX_TENSORS = 32;

enum HeadStepFlags : int {
  kHsGradBf16 = 1,   // dw is bf16 (else fp32)
  kHsVec = 2,        // 16 B rows: float4 path
  kHsTheta = 4,      // gw/atten/theta present: emit θ
  kHsAttenVec = 8,   // linear weight with L % 4 == 0: float4 atten
};

struct HeadStepTensor {
  float* aw;
  const float* aw0;
  const void* dw;
  const float* gw;
  const float* atten;
  float* m;
  float* v;
  __hip_bfloat16* theta;
  const float* step;
  int64_t numel;
  int L;
  int inner;
  int flags;
  int block_end;     // exclusive prefix of blocks in this launch
  int partial0;      // index of this tensor's first partial
  int pad_;
};

struct HeadStepArgs {
  HeadStepTensor t[HS_MAX_TENSORS];
  double* partials;
  double lr, beta1, beta2, weight_decay, eps;
  float lambda;
  int n_tensors;
};
static_assert(sizeof(HeadStepArgs) <= 4096, "kernel argument limit");

struct HeadStepScalars {
  double lr, beta1, beta2, weight_decay, eps;
  float bias_correction1, bias_correction2_sqrt, lambda;
};

// one element; mirrors adam_math<float, float, 4, ORIGINAL, false>
__device__ __forceinline__ void head_step_elem(const HeadStepScalars& s,
                                               float& param, float aw0,
                                               float dw, float& exp_avg,
                                               float& exp_avg_sq,
                                               double& drift) {
  const float d = param - aw0;
  drift += fabs((double)param - (double)aw0);
  const float sgn = d > 0.f ? s.lambda : (d < 0.f ? -s.lambda : 0.f);
  float grad = dw + sgn;
  if (s.weight_decay != 0) {
    grad += param * s.weight_decay;
  }
  exp_avg = s.beta1 * exp_avg + (1 - s.beta1) * grad;
  exp_avg_sq = s.beta2 * exp_avg_sq + (1 - s.beta2) * grad * grad;
  const float step_size = s.lr / s.bias_correction1;
  float denom = (sqrtf(exp_avg_sq) / s.bias_correction2_sqrt) + s.eps;
  param -= step_size * exp_avg / denom;
}

__device__ __forceinline__ float bf16_bits_to_float(unsigned short b) {
  return __uint_as_float((unsigned)b << 16);
}

__global__ __launch_bounds__(HS_BLOCK) void head_step_kernel(
    const HeadStepArgs args) {
  // block -> (tensor, chunk): linear search over the (≤ 32) block prefixes
  int ti = 0;
  while (ti < args.n_tensors - 1 && (int)blockIdx.x >= args.t[ti].block_end)
    ++ti;
  const HeadStepTensor& t = args.t[ti];
  const int block0 = ti ? args.t[ti - 1].block_end : 0;
  const int chunk = (int)blockIdx.x - block0;
  const int64_t base = (int64_t)chunk * HS_CHUNK;
  const int64_t rest = t.numel - base;
  const int len = rest < HS_CHUNK ? (int)rest : HS_CHUNK;

  HeadStepScalars s;
  s.lr = args.lr;
  s.beta1 = args.beta1;
  s.beta2 = args.beta2;
  s.weight_decay = args.weight_decay;
  s.eps = args.eps;
  s.lambda = args.lambda;
  {
    const float step_count = *t.step;
    const double bc1 = 1 - ::pow(args.beta1, (double)step_count);
    const double bc2 = 1 - ::pow(args.beta2, (double)step_count);
    s.bias_correction1 = (float)bc1;
    s.bias_correction2_sqrt = (float)::sqrt(bc2);
  }

  float* aw = t.aw + base;
  const float* aw0 = t.aw0 + base;
  float* m = t.m + base;
  float* v = t.v + base;
  const bool g16 = t.flags & kHsGradBf16;
  const bool has_theta = t.flags & kHsTheta;
  const float* dw32 = reinterpret_cast<const float*>(t.dw) + base;
  const unsigned short* dw16 =
      reinterpret_cast<const unsigned short*>(t.dw) + base;
  const float* gw = has_theta ? t.gw + base : nullptr;
  __hip_bfloat16* theta = has_theta ? t.theta + base : nullptr;
  const int64_t L = t.L, inner = t.inner;

  double drift = 0.0;

  if (t.flags & kHsVec) {
    const int q4 = len >> 2;
    const bool atten_vec = t.flags & kHsAttenVec;
#pragma unroll 2
    for (int q = threadIdx.x; q < q4; q += HS_BLOCK) {
      const int i0 = q << 2;
      float4 p = *reinterpret_cast<const float4*>(aw + i0);
      const float4 p0 = *reinterpret_cast<const float4*>(aw0 + i0);
      float4 em = *reinterpret_cast<const float4*>(m + i0);
      float4 ev = *reinterpret_cast<const float4*>(v + i0);
      float4 g;
      if (g16) {
        const uint2 raw = *reinterpret_cast<const uint2*>(dw16 + i0);
        g.x = __uint_as_float(raw.x << 16);
        g.y = __uint_as_float(raw.x & 0xffff0000u);
        g.z = __uint_as_float(raw.y << 16);
        g.w = __uint_as_float(raw.y & 0xffff0000u);
      } else {
        g = *reinterpret_cast<const float4*>(dw32 + i0);
      }
      float4 gwv = {0.f, 0.f, 0.f, 0.f}, a4 = {0.f, 0.f, 0.f, 0.f};
      if (has_theta) {
        gwv = *reinterpret_cast<const float4*>(gw + i0);
        if (atten_vec) {
          a4 = *reinterpret_cast<const float4*>(t.atten + ((base + i0) % L));
        } else {
          const float a = t.atten[((base + i0) / inner) % L];
          a4 = {a, a, a, a};
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        head_step_elem(s, (&p.x)[e], (&p0.x)[e], (&g.x)[e], (&em.x)[e],
                       (&ev.x)[e], drift);
      }
      *reinterpret_cast<float4*>(aw + i0) = p;
      *reinterpret_cast<float4*>(m + i0) = em;
      *reinterpret_cast<float4*>(v + i0) = ev;
      if (has_theta) {
        __hip_bfloat16 th[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          th[e] = __float2bfloat16(fmaf((&a4.x)[e], (&gwv.x)[e], (&p.x)[e]));
        }
        __builtin_memcpy(theta + i0, th, sizeof(th));
      }
    }
    // ragged tail of the tensor's last chunk (< 4 elements)
    for (int i = (q4 << 2) + threadIdx.x; i < len; i += HS_BLOCK) {
      float p = aw[i], em = m[i], ev = v[i];
      const float g = g16 ? bf16_bits_to_float(dw16[i]) : dw32[i];
      head_step_elem(s, p, aw0[i], g, em, ev, drift);
      aw[i] = p;
      m[i] = em;
      v[i] = ev;
      if (has_theta) {
        const float a = t.atten[((base + i) / inner) % L];
        theta[i] = __float2bfloat16(fmaf(a, gw[i], p));
      }
    }
  } else {
    // scalar path: unaligned rows, or an atten broadcast that a 4-run crosses
    for (int i = threadIdx.x; i < len; i += HS_BLOCK) {
      float p = aw[i], em = m[i], ev = v[i];
      const float g = g16 ? bf16_bits_to_float(dw16[i]) : dw32[i];
      head_step_elem(s, p, aw0[i], g, em, ev, drift);
      aw[i] = p;
      m[i] = em;
      v[i] = ev;
      if (has_theta) {
        const float a = t.atten[((base + i) / inner) % L];
        theta[i] = __float2bfloat16(fmaf(a, gw[i], p));
      }
    }
  }

  // block sum of the drift partial, in double
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) drift += __shfl_down(drift, off, 64);
  __shared__ double lds[HS_BLOCK / kWave];
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x / kWave] = drift;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < HS_BLOCK / kWave; ++w) total += lds[w];
    args.partials[t.partial0 + chunk] = total;
  }
}

extern "C" int flreid_head_step_chunk() { return HS_CHUNK; }

// rows: n × kHeadStepFields (ops.h) int64 — aw, aw0, dw, gw, atten, m, v,
// theta, step (device addresses), numel, L, inner, flags, partial0.
// Validates every row, then launches (several launches when the table
// exceeds the argument limit).  Throws before the first launch on any violated check.
extern "C" void flreid_head_step(const int64_t* rows, int n_rows,
                                 double* partials, int64_t n_partials,
                                 double lr, double beta1, double beta2,
                                 double weight_decay, double eps,
                                 float lambda, hipStream_t stream) {
  if (n_rows <= 0) throw std::runtime_error("head_step: empty tensor table");
  if (!partials) throw std::runtime_error("head_step: null partials");
  for (int r = 0; r < n_rows; ++r) {
    const int64_t* row = rows + (int64_t)r * kHeadStepFields;
    const int flags = (int)row[12];
    const bool th = flags & kHsTheta;
    const int64_t numel = row[9], L = row[10], inner = row[11];
    const char* names[9] = {"aw", "aw0", "dw", "gw", "atten",
                            "m",  "v",   "theta", "step"};
    for (int k = 0; k < 9; ++k) {
      const bool theta_only = (k == 3 || k == 4 || k == 7);
      if (row[k] == 0 && (th || !theta_only))
        throw std::runtime_error(std::string("head_step: null pointer '") +
                                 names[k] + "' in row " + std::to_string(r));
    }
    if (numel <= 0 || L <= 0 || inner <= 0)
      throw std::runtime_error("head_step: bad numel/L/inner in row " +
                               std::to_string(r));
    const int64_t nchunks = (numel + HS_CHUNK - 1) / HS_CHUNK;
    if (row[13] < 0 || row[13] + nchunks > n_partials)
      throw std::runtime_error("head_step: partial range out of bounds");
    if (flags & kHsVec) {
      const int64_t galign = (flags & kHsGradBf16) ? 8 : 16;
      bool ok = row[0] % 16 == 0 && row[1] % 16 == 0 && row[5] % 16 == 0 &&
                row[6] % 16 == 0 && row[2] % galign == 0;
      if (th) {
        ok = ok && row[3] % 16 == 0 && row[7] % 8 == 0;
        if (flags & kHsAttenVec)
          ok = ok && inner == 1 && L % 4 == 0 && row[4] % 16 == 0;
        else
          ok = ok && (L == 1 || inner % 4 == 0);
      }
      if (!ok)
        throw std::runtime_error(
            "head_step: float4 path requested for an unaligned row " +
            std::to_string(r));
    }
  }

  int r = 0;
  while (r < n_rows) {
    HeadStepArgs args;
    int n = 0, blocks = 0;
    for (; r < n_rows && n < HS_MAX_TENSORS; ++r, ++n) {
      const int64_t* row = rows + (int64_t)r * kHeadStepFields;
      HeadStepTensor& t = args.t[n];
      t.aw = reinterpret_cast<float*>(row[0]);
      t.aw0 = reinterpret_cast<const float*>(row[1]);
      t.dw = reinterpret_cast<const void*>(row[2]);
      t.gw = reinterpret_cast<const float*>(row[3]);
      t.atten = reinterpret_cast<const float*>(row[4]);
      t.m = reinterpret_cast<float*>(row[5]);
      t.v = reinterpret_cast<float*>(row[6]);
      t.theta = reinterpret_cast<__hip_bfloat16*>(row[7]);
      t.step = reinterpret_cast<const float*>(row[8]);
      t.numel = row[9];
      t.L = (int)row[10];
      t.inner = (int)row[11];
      t.flags = (int)row[12];
      t.partial0 = (int)row[13];
      t.pad_ = 0;
      blocks += (int)((row[9] + HS_CHUNK - 1) / HS_CHUNK);
      t.block_end = blocks;
    }
    for (int k = n; k < HS_MAX_TENSORS; ++k) args.t[k] = HeadStepTensor{};
    args.partials = partials;
    args.lr = lr;
    args.beta1 = beta1;
    args.beta2 = beta2;
    args.weight_decay = weight_decay;
    args.eps = eps;
    args.lambda = lambda;
    args.n_tensors = n;
    hipLaunchKernelGGL(head_step_kernel, dim3(blocks), dim3(HS_BLOCK), 0,
                       stream, args);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace flreid

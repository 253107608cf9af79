// Fused multi-tensor quadratic penalty: Σ_n Σ_s F_s[n]·(p[n] − a_s[n])² over
// a parameter list and S (anchor, importance) sets — the per-step regulariser
// of EWC / MAS (S = 1), FedCurv (S = 1 + #other clients) and FedProx (S = 1,
// unit importance), ref:methods/ewc.py:80-85, ref:methods/fedprox.py:52-57.
//
// The eager chain runs sub, pow, mul, sum and a scalar add per tensor and
// per set, plus the mirror chain backward.  Here: ONE forward pass reads p
// once and every present (a_s, F_s) and accumulates the value into per-chunk
// partials (summed by a tiny torch reduction — no atomics, bit-reproducible);
// ONE backward pass reads them again and writes the gradient into one flat
// buffer, 4S + 3 weight-sized passes per step in all.
//
// The backward reproduces the eager chain's gradient BIT FOR BIT: per set
// fl(fl(g·F_s) · (2·d_s)) — autograd's mul backward, then pow backward — and
// fl(g · (2·d_s)) for unit importance, the sets added from the last to the
// first, which is the order in which autograd's engine sums them into a
// leaf.  Training amplifies a last-bit difference in a gradient into
// visibly different weights within a few rounds, so a form that rounds
// differently (saving the unscaled Σ_s F_s·2·d_s in the forward and scaling
// it by g afterwards: 2S + 4 passes) would change every trajectory.  The
// gradient term is compiled with floating-point contraction off, so that
// no product and sum of it become one fused multiply-add.
//
// The tensor list crosses as two device tables:
//   ptrs   int64 [n_tensors, 1 + 2·S] — p, a_0, F_0, a_1, F_1, …
//          a_s == 0: set s has no entry for this tensor (skipped);
//          F_s == 0 with a_s != 0: unit importance
//   chunks int32 [n_chunks, 4] — (tensor, elem_offset, len, flat_offset)
// one chunk of at most PENALTY_CHUNK elements per workgroup.  Every tensor
// is walked in storage order, so p, a_s and F_s must share one dense layout;
// all bases and every tensor's flat_offset are 16-byte aligned (the python
// wrapper's eligibility test), so the float4 body never straddles.

#include "common.h"
#include "ops.h"

namespace flreid {

constexpr int PENALTY_BLOCK = 256;
constexpr int PENALTY_CHUNK = 1 << 16;
constexpr int PENALTY_UNROLL = 4;      // quads in flight per thread and stream

// forward, one set's term for one element: acc += F·d·d
__device__ __forceinline__ void penalty_value(float p, float a, float f,
                                              float& acc) {
  const float d = p - a;
  acc += f * d * d;
}

// backward, one set's term for one element, in the eager chain's rounding:
// w = fl(g·F) (g itself for unit importance), term = fl(w · 2d); the first
// present set initialises the sum, as autograd's input buffer does
__device__ __forceinline__ void penalty_grad(float p, float a, float w,
                                             bool first, float& g) {
  // the product must round before the add: no fused multiply-add here
#pragma clang fp contract(off)
  const float t = w * (2.f * (p - a));
  g = first ? t : g + t;
}

// U float4 quads of one thread, PENALTY_BLOCK quads apart: quad i + u·BLOCK
// for u < U.  The caller guarantees all of them lie inside the chunk.
// BWD: write the gradient to `out` (scaled by gs); else accumulate the value.
template <int ST, int U, bool BWD>
__device__ __forceinline__ void penalty_quads(const float* p,
                                              const int64_t* __restrict__ row,
                                              int off, int S, int i, float gs,
                                              float* out, float& acc) {
  const float4* p4 = reinterpret_cast<const float4*>(p);
  float4 pv[U], g[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    pv[u] = p4[i + u * PENALTY_BLOCK];
    g[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  bool first = true;
  // constant trip count for ST > 0 (fully unrolled), runtime S otherwise;
  // last set first (the backward's summation order, immaterial forward)
  for (int s = (ST > 0 ? ST : S) - 1; s >= 0; --s) {
    const float* a = reinterpret_cast<const float*>(row[1 + 2 * s]);
    if (a == nullptr) continue;       // wave-uniform: per tensor
    const float* f = reinterpret_cast<const float*>(row[2 + 2 * s]);
    const float4* a4 = reinterpret_cast<const float4*>(a + off);
    float4 av[U], fv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) av[u] = a4[i + u * PENALTY_BLOCK];
    if (f != nullptr) {
      const float4* f4 = reinterpret_cast<const float4*>(f + off);
#pragma unroll
      for (int u = 0; u < U; ++u) fv[u] = f4[i + u * PENALTY_BLOCK];
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) fv[u] = make_float4(1.f, 1.f, 1.f, 1.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (BWD) {
        // fl(gs·1) == gs: unit importance needs no case of its own
        penalty_grad(pv[u].x, av[u].x, gs * fv[u].x, first, g[u].x);
        penalty_grad(pv[u].y, av[u].y, gs * fv[u].y, first, g[u].y);
        penalty_grad(pv[u].z, av[u].z, gs * fv[u].z, first, g[u].z);
        penalty_grad(pv[u].w, av[u].w, gs * fv[u].w, first, g[u].w);
      } else {
        penalty_value(pv[u].x, av[u].x, fv[u].x, acc);
        penalty_value(pv[u].y, av[u].y, fv[u].y, acc);
        penalty_value(pv[u].z, av[u].z, fv[u].z, acc);
        penalty_value(pv[u].w, av[u].w, fv[u].w, acc);
      }
    }
    first = false;
  }
  if (BWD) {
    float4* o4 = reinterpret_cast<float4*>(out);
#pragma unroll
    for (int u = 0; u < U; ++u) o4[i + u * PENALTY_BLOCK] = g[u];
  }
}

// ST > 0: S is the compile-time ST (set loop unrolled, table row hoisted);
// ST == 0: S is the runtime argument.  One chunk per workgroup.
// BWD == false: partials[chunk] = the chunk's value;
// BWD == true:  flat_grad[flat_offset + i] = d(*gscale · value)/dp.
template <int ST, bool BWD>
__global__ __launch_bounds__(PENALTY_BLOCK) void penalty_kernel(
    const int64_t* __restrict__ ptrs, const int* __restrict__ chunks,
    int s_rt, float* __restrict__ partials,
    const float* __restrict__ gscale, float* __restrict__ flat_grad) {
  const int S = ST > 0 ? ST : s_rt;
  const int* ch = chunks + (int64_t)blockIdx.x * 4;
  const int64_t* row = ptrs + (int64_t)ch[0] * (1 + 2 * S);
  const int off = ch[1];
  const int len = ch[2];
  const float* p = reinterpret_cast<const float*>(row[0]) + off;
  float* out = BWD ? flat_grad + ch[3] : nullptr;
  const float gs = BWD ? *gscale : 0.f;

  float acc = 0.f;
  const int q4 = len >> 2;            // full float4 quads
  int i = threadIdx.x;
  // U quads per trip: the set branches are per tensor, outside the batch,
  // so a thread keeps U independent 16-byte loads in flight per stream
  for (; i + (PENALTY_UNROLL - 1) * PENALTY_BLOCK < q4;
       i += PENALTY_UNROLL * PENALTY_BLOCK)
    penalty_quads<ST, PENALTY_UNROLL, BWD>(p, row, off, S, i, gs, out, acc);
  for (; i < q4; i += PENALTY_BLOCK)
    penalty_quads<ST, 1, BWD>(p, row, off, S, i, gs, out, acc);
  for (i = (q4 << 2) + threadIdx.x; i < len; i += PENALTY_BLOCK) {
    const float pv = p[i];
    float g = 0.f;
    bool first = true;
    for (int s = S - 1; s >= 0; --s) {
      const float* a = reinterpret_cast<const float*>(row[1 + 2 * s]);
      if (a == nullptr) continue;
      const float* f = reinterpret_cast<const float*>(row[2 + 2 * s]);
      const float fv = f != nullptr ? f[off + i] : 1.f;
      if (BWD) {
        penalty_grad(pv, a[off + i], gs * fv, first, g);
        first = false;
      } else {
        penalty_value(pv, a[off + i], fv, acc);
      }
    }
    if (BWD) out[i] = g;
  }
  if (!BWD) {
    __shared__ float lds[PENALTY_BLOCK / kWave];
    acc = block_reduce_sum<PENALTY_BLOCK>(acc, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
  }
}

extern "C" int flreid_penalty_chunk() { return PENALTY_CHUNK; }
extern "C" int flreid_penalty_block() { return PENALTY_BLOCK; }

template <bool BWD>
static void penalty_launch(const int64_t* ptrs, const int* chunks, int S,
                           float* partials, const float* gscale,
                           float* flat_grad, int n_chunks,
                           hipStream_t stream) {
  const dim3 grid(n_chunks), block(PENALTY_BLOCK);
#define FLREID_PENALTY_LAUNCH(ST)                                       \
  hipLaunchKernelGGL((penalty_kernel<ST, BWD>), grid, block, 0, stream, \
                     ptrs, chunks, S, partials, gscale, flat_grad)
  switch (S) {
    case 1: FLREID_PENALTY_LAUNCH(1); break;
    case 2: FLREID_PENALTY_LAUNCH(2); break;
    case 3: FLREID_PENALTY_LAUNCH(3); break;
    case 4: FLREID_PENALTY_LAUNCH(4); break;
    default: FLREID_PENALTY_LAUNCH(0); break;
  }
#undef FLREID_PENALTY_LAUNCH
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_penalty_fwd(const int64_t* ptrs, const int* chunks,
                                   int S, float* partials, int n_chunks,
                                   hipStream_t stream) {
  if (ptrs == nullptr || chunks == nullptr || partials == nullptr)
    throw std::invalid_argument("penalty_fwd: null table or partials");
  if (S < 1 || n_chunks < 1)
    throw std::invalid_argument("penalty_fwd: needs S >= 1 and n_chunks >= 1");
  penalty_launch<false>(ptrs, chunks, S, partials, nullptr, nullptr, n_chunks,
                        stream);
}

// gscale: the upstream gradient, one float on the device (no host sync)
extern "C" void flreid_penalty_bwd(const int64_t* ptrs, const int* chunks,
                                   int S, const float* gscale,
                                   float* flat_grad, int n_chunks,
                                   hipStream_t stream) {
  if (ptrs == nullptr || chunks == nullptr || gscale == nullptr ||
      flat_grad == nullptr)
    throw std::invalid_argument("penalty_bwd: null table, scale or gradient");
  if (S < 1 || n_chunks < 1)
    throw std::invalid_argument("penalty_bwd: needs S >= 1 and n_chunks >= 1");
  if (reinterpret_cast<uintptr_t>(flat_grad) % 16 != 0)
    throw std::invalid_argument("penalty_bwd: flat_grad not 16-byte aligned");
  penalty_launch<true>(ptrs, chunks, S, nullptr, gscale, flat_grad, n_chunks,
                       stream);
}

}  // namespace flreid

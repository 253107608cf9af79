// One-launch training-mode BatchNorm over NHWC rows (bf16), bit-identical to
// the two-launch pair of bn_train.hip.
//
// The two-launch pair reads its inputs twice (partial, then finalize), goes
// through a global [nslab][C] workspace and pays two launches for tensors of
// 0.25–8 MB that are launch- and latency-bound.  A channel's statistics
// depend on that channel's column alone, so here ONE block owns a group of
// W = 4·QUADS channels over ALL rows:
//
//   1. every thread loads its rows × 4 channels once and keeps them in
//      registers (raw bf16);
//   2. it forms the stripe sums in the pair's order (bn_train.h: stripe g sums
//      rows g, g+S, … sequentially) and puts them in LDS;
//   3. slab sums (16 stripes in order from 0.f) and totals (slabs in order
//      from 0.f) are formed in LDS exactly as partial / finalize form them;
//   4. W threads run the scalar chain and write the stats block (save_mean,
//      save_invstd, running stats / dgamma, dbeta) — this block owns them;
//   5. every thread normalises its own rows from registers and stores them.
//
// One read of x (and dy), one write of y (or dx), one launch, no workspace.
// Blocks never wait for each other.  All arithmetic comes from bn_train.h,
// the text the two-launch kernels compile from.
//
// Residual epilogue (RESID instantiations): a block's last BatchNorm is
// followed by relu(y + identity).  Forward reads the identity's quad in step 5
// and stores relu(bf16(y) + res) — the bits of the add and clamp kernels it
// replaces; statistics are untouched.  Backward masks dy with the saved
// output z as it loads it (threshold_backward), stores the masked value as
// the identity's gradient, and runs the plain backward on it.
//
// Thread mapping <QUADS, P, SPT, RPS>: thread = (row-thread p, quad q), P
// row-threads; row-thread p owns stripes p, p+P, … (SPT of them) and up to
// RPS rows of each, so a shape fits when SPT·P ≥ S and RPS ≥ ceil(M/S).
// Shapes that fit no instantiation stay on the two-launch pair.
//
// Channel groups are handed out so that the blocks of one XCD (workgroups
// are dealt round-robin over the 8 XCDs) cover one contiguous channel range:
// a 128 B line of a row is then fetched by one XCD's L2 and not by all eight.

#include "bn_train.h"
#include "common.h"
#include "ops.h"

namespace flreid {

constexpr int BN_OP_PAD = 4;          // floats; staggers the 16 stripe rows

// LDS, sized for the most slabs the instantiation can take (NS = SPT·P/16):
// la, lb [16][ld] stripe sums (stripe g at row g%16, slab g/16, ld =
// nslab·W + PAD); sla, slb [nslab][W] slab sums; two [W] arrays broadcast
// the channel scalars.  Static, like every other kernel the head-step graph
// captures.
template <int W, int NS>
struct BnOpLds {
  float la[BN_STRIPES * (NS * W + BN_OP_PAD)];
  float lb[BN_STRIPES * (NS * W + BN_OP_PAD)];
  float sla[NS * W];
  float slb[NS * W];
  float c0[W];
  float c1[W];
};

__device__ __forceinline__ int bn_op_group(int b, int nb, int swz) {
  return (swz && nb % 8 == 0) ? (b % 8) * (nb / 8) + b / 8 : b;
}

// Stripe sums (already in la / lb) → slab sums → totals of channel
// threadIdx.x (valid for threadIdx.x < W), in the two-launch order.
template <int W>
__device__ __forceinline__ void bn_op_reduce(const float* la, const float* lb,
                                             float* sla, float* slb,
                                             int nslab, int ld, float& ta,
                                             float& tb) {
  __syncthreads();
  for (int t = threadIdx.x; t < nslab * W; t += blockDim.x) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < BN_STRIPES; ++i) {
      a += la[i * ld + t];
      b += lb[i * ld + t];
    }
    sla[t] = a;
    slb[t] = b;
  }
  __syncthreads();
  ta = 0.f;
  tb = 0.f;
  if (threadIdx.x < W) {
    for (int s = 0; s < nslab; ++s) {
      ta += sla[s * W + threadIdx.x];
      tb += slb[s * W + threadIdx.x];
    }
  }
}

// ---------------------------------------------------------------- forward
template <int QUADS, int P, int SPT, int RPS, bool RESID>
__global__ __launch_bounds__(QUADS* P) void bn_onepass_fwd_kernel(
    const __hip_bfloat16* __restrict__ X,
    const __hip_bfloat16* __restrict__ RES, __hip_bfloat16* __restrict__ Y,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    float* __restrict__ rmean, float* __restrict__ rvar,
    float* __restrict__ smean, float* __restrict__ sinv,
    unsigned long long* __restrict__ nbt, int64_t M, int C, int nslab,
    float momentum, float eps, float unbiased, int relu, int swz) {
  constexpr int W = QUADS * 4;
  __shared__ BnOpLds<W, SPT * P / BN_STRIPES> lds;
  const int S = nslab * BN_STRIPES;
  const int ld = nslab * W + BN_OP_PAD;
  float* la = lds.la;
  float* lb = lds.lb;
  float* sla = lds.sla;
  float* slb = lds.slb;
  float* lmean = lds.c0;
  float* linv = lds.c1;

  const int q = threadIdx.x % QUADS;
  const int p = threadIdx.x / QUADS;
  const int c0 = bn_op_group(blockIdx.x, gridDim.x, swz) * W;
  const int c = c0 + q * 4;

  if (nbt != nullptr && blockIdx.x == 0 && threadIdx.x == 0) ++(*nbt);

  ushort4 raw[SPT][RPS];
#pragma unroll
  for (int a = 0; a < SPT; ++a) {
    const int g = p + a * P;
#pragma unroll
    for (int k = 0; k < RPS; ++k) {
      const int64_t row = g + (int64_t)k * S;
      raw[a][k] = make_ushort4(0, 0, 0, 0);
      if (g < S && row < M)
        raw[a][k] = *reinterpret_cast<const ushort4*>(X + row * C + c);
    }
  }
#pragma unroll
  for (int a = 0; a < SPT; ++a) {
    const int g = p + a * P;
    if (g < S) {
      float sa[4] = {0.f, 0.f, 0.f, 0.f};
      float sb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < RPS; ++k) {
        if (g + (int64_t)k * S < M) {
          float x[4];
          bn_unpack4(raw[a][k], x);
#pragma unroll
          for (int j = 0; j < 4; ++j) bn_fwd_accum(sa[j], sb[j], x[j]);
        }
      }
      const int o = (g % BN_STRIPES) * ld + (g / BN_STRIPES) * W + q * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        la[o + j] = sa[j];
        lb[o + j] = sb[j];
      }
    }
  }

  float ta, tb;
  bn_op_reduce<W>(la, lb, sla, slb, nslab, ld, ta, tb);
  if (threadIdx.x < W) {
    float mean, var, inv;
    bn_fwd_stats(ta, tb, M, eps, mean, var, inv);
    lmean[threadIdx.x] = mean;
    linv[threadIdx.x] = inv;
    const int gc = c0 + threadIdx.x;
    smean[gc] = mean;
    sinv[gc] = inv;
    if (rmean != nullptr)
      bn_running_update(rmean[gc], rvar[gc], momentum, mean, var, unbiased);
  }
  __syncthreads();

  float scale[4], shift[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    bn_scale_shift(gamma[c + j], beta[c + j], lmean[q * 4 + j],
                   linv[q * 4 + j], scale[j], shift[j]);
#pragma unroll
  for (int a = 0; a < SPT; ++a) {
    const int g = p + a * P;
#pragma unroll
    for (int k = 0; k < RPS; ++k) {
      const int64_t row = g + (int64_t)k * S;
      if (g < S && row < M) {
        float v[4];
        bn_unpack4(raw[a][k], v);
        if constexpr (RESID) {
          float r[4];
          bn_load4(RES + row * C + c, r);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = bn_add_relu(bn_normalize(v[j], scale[j], shift[j], 0),
                               r[j]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            v[j] = bn_normalize(v[j], scale[j], shift[j], relu);
        }
        bn_store4(Y + row * C + c, v);
      }
    }
  }
}

// --------------------------------------------------------------- backward
template <int QUADS, int P, int SPT, int RPS, bool RESID>
__global__ __launch_bounds__(QUADS* P) void bn_onepass_bwd_kernel(
    const __hip_bfloat16* __restrict__ X,
    const __hip_bfloat16* __restrict__ DY,
    const __hip_bfloat16* __restrict__ Z, __hip_bfloat16* __restrict__ DRES,
    __hip_bfloat16* __restrict__ DX,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ smean, const float* __restrict__ sinv,
    float* __restrict__ dgamma, float* __restrict__ dbeta, int64_t M, int C,
    int nslab, int relu, int swz) {
  constexpr int W = QUADS * 4;
  __shared__ BnOpLds<W, SPT * P / BN_STRIPES> lds;
  const int S = nslab * BN_STRIPES;
  const int ld = nslab * W + BN_OP_PAD;
  float* la = lds.la;
  float* lb = lds.lb;
  float* sla = lds.sla;
  float* slb = lds.slb;
  float* lmdy = lds.c0;
  float* lmdyx = lds.c1;

  const int q = threadIdx.x % QUADS;
  const int p = threadIdx.x / QUADS;
  const int c0 = bn_op_group(blockIdx.x, gridDim.x, swz) * W;
  const int c = c0 + q * 4;

  ushort4 rx[SPT][RPS], rdy[SPT][RPS];
#pragma unroll
  for (int a = 0; a < SPT; ++a) {
    const int g = p + a * P;
#pragma unroll
    for (int k = 0; k < RPS; ++k) {
      const int64_t row = g + (int64_t)k * S;
      rx[a][k] = make_ushort4(0, 0, 0, 0);
      rdy[a][k] = make_ushort4(0, 0, 0, 0);
      if (g < S && row < M) {
        rx[a][k] = *reinterpret_cast<const ushort4*>(X + row * C + c);
        rdy[a][k] = *reinterpret_cast<const ushort4*>(DY + row * C + c);
        if constexpr (RESID) {
          // the ReLU behind the add masks dy as it arrives; the masked value
          // is the identity branch's gradient
          rdy[a][k] = bn_relu_mask4(
              rdy[a][k], *reinterpret_cast<const ushort4*>(Z + row * C + c));
          if (DRES != nullptr)
            *reinterpret_cast<ushort4*>(DRES + row * C + c) = rdy[a][k];
        }
      }
    }
  }

  float mn[4], iv[4], g_iv[4], sh[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mn[j] = smean[c + j];
    iv[j] = sinv[c + j];
    bn_scale_shift(gamma[c + j], beta[c + j], mn[j], iv[j], g_iv[j], sh[j]);
  }

#pragma unroll
  for (int a = 0; a < SPT; ++a) {
    const int g = p + a * P;
    if (g < S) {
      float sa[4] = {0.f, 0.f, 0.f, 0.f};
      float sb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < RPS; ++k) {
        if (g + (int64_t)k * S < M) {
          float x[4], dy[4];
          bn_unpack4(rx[a][k], x);
          bn_unpack4(rdy[a][k], dy);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (relu && bn_relu_off(x[j], g_iv[j], sh[j])) continue;
            bn_bwd_accum(sa[j], sb[j], dy[j], x[j], mn[j], iv[j]);
          }
        }
      }
      const int o = (g % BN_STRIPES) * ld + (g / BN_STRIPES) * W + q * 4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        la[o + j] = sa[j];
        lb[o + j] = sb[j];
      }
    }
  }

  float tdy, tdyx;
  bn_op_reduce<W>(la, lb, sla, slb, nslab, ld, tdy, tdyx);
  if (threadIdx.x < W) {
    const int gc = c0 + threadIdx.x;
    dgamma[gc] = tdyx;
    dbeta[gc] = tdy;
    bn_bwd_means(tdy, tdyx, M, lmdy[threadIdx.x], lmdyx[threadIdx.x]);
  }
  __syncthreads();

  float mdy[4], mdyx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mdy[j] = lmdy[q * 4 + j];
    mdyx[j] = lmdyx[q * 4 + j];
  }
#pragma unroll
  for (int a = 0; a < SPT; ++a) {
    const int g = p + a * P;
#pragma unroll
    for (int k = 0; k < RPS; ++k) {
      const int64_t row = g + (int64_t)k * S;
      if (g < S && row < M) {
        float x[4], dy[4], dx[4];
        bn_unpack4(rx[a][k], x);
        bn_unpack4(rdy[a][k], dy);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dx[j] = bn_bwd_dx(x[j], dy[j], mn[j], iv[j], g_iv[j], sh[j], mdy[j],
                            mdyx[j], relu);
        bn_store4(DX + row * C + c, dx);
      }
    }
  }
}

// ----------------------------------------------------------------- launch
struct BnOpCfg {
  int quads, p, spt, rps;
};

// The instantiations (id, QUADS, P, SPT, RPS); a variant's low byte is the
// id.  A 32-channel, 1024-thread tile for 16 rows per stripe is left out: its
// backward kernel does not fit 128 VGPRs and spills to scratch.
#define BN_OP_CFGS(X) \
  X(0, 1, 512, 1, 4)  \
  X(1, 2, 256, 2, 4)  \
  X(2, 2, 512, 1, 4)  \
  X(3, 2, 128, 1, 16) \
  X(4, 4, 128, 1, 16) \
  X(5, 2, 128, 1, 1)  \
  X(6, 4, 128, 1, 1)  \
  X(7, 8, 128, 1, 1)

static const BnOpCfg kBnOpCfgs[] = {
#define BN_OP_ROW(id, q, p, spt, rps) {q, p, spt, rps},
    BN_OP_CFGS(BN_OP_ROW)
#undef BN_OP_ROW
};
constexpr int kBnOpNumCfgs = sizeof(kBnOpCfgs) / sizeof(kBnOpCfgs[0]);

static bool bn_op_fits(int cfg, int64_t M, int C) {
  if (cfg < 0 || cfg >= kBnOpNumCfgs || M < 2 || C < BN_CG || C % BN_CG != 0)
    return false;
  const BnOpCfg& k = kBnOpCfgs[cfg];
  const int W = k.quads * 4;
  const int nslab = bn_nslab(M, C);
  const int64_t S = (int64_t)nslab * BN_STRIPES;
  return C % W == 0 && (int64_t)k.spt * k.p >= S && (int64_t)k.rps * S >= M;
}

// Per-shape choice, measured on MI355X (profiles/README.md, "One-launch
// train BN"); the first entry that fits wins.
static const int kBnOpPrefFwd[] = {5, 2, 4, 6, 7, 1, 0, 3};
static const int kBnOpPrefBwd[] = {5, 2, 4, 6, 7, 1, 0, 3};

static int bn_op_pick(const int* pref, int64_t M, int C) {
  for (int i = 0; i < kBnOpNumCfgs; ++i)
    if (bn_op_fits(pref[i], M, C)) return pref[i];
  return -1;
}

// variant < 0: the table's choice.  Otherwise low byte = instantiation,
// bit 8 = plain block→group order (no XCD grouping); for the benchmark.
static void bn_op_resolve(int variant, const int* pref, int64_t M, int C,
                          int* cfg, int* swz) {
  *swz = 1;
  if (variant < 0) {
    *cfg = bn_op_pick(pref, M, C);
  } else {
    *cfg = variant & 0xff;
    *swz = (variant & 0x100) ? 0 : 1;
    if (!bn_op_fits(*cfg, M, C)) *cfg = -1;
  }
  if (*cfg < 0)
    throw std::runtime_error(
        "bn_onepass: shape outside the one-launch regime (M=" +
        std::to_string(M) + ", C=" + std::to_string(C) + ")");
}

extern "C" int flreid_bn_onepass_config(int64_t M, int C) {
  const int f = bn_op_pick(kBnOpPrefFwd, M, C);
  const int b = bn_op_pick(kBnOpPrefBwd, M, C);
  return (f < 0 || b < 0) ? -1 : f;
}

// RESID picks the residual instantiation: res (forward) and z (backward) are
// then read, and the BN's own ReLU is off.
template <bool RESID>
static void bn_op_launch_fwd(const void* X, const void* RES, void* Y,
                             const float* gamma, const float* beta,
                             float* rmean, float* rvar, float* smean,
                             float* sinv, unsigned long long* nbt, int64_t M,
                             int C, float momentum, float eps, float unbiased,
                             int relu, int variant, hipStream_t stream) {
  int cfg, swz;
  bn_op_resolve(variant, kBnOpPrefFwd, M, C, &cfg, &swz);
  const int nslab = bn_nslab(M, C);
  switch (cfg) {
#define BN_OP_CASE(id, Q, P, SPT, RPS)                                        \
  case id:                                                                    \
    hipLaunchKernelGGL((bn_onepass_fwd_kernel<Q, P, SPT, RPS, RESID>),        \
                       dim3(C / (Q * 4)), dim3(Q * P), 0, stream,             \
                       (const __hip_bfloat16*)X, (const __hip_bfloat16*)RES,  \
                       (__hip_bfloat16*)Y, gamma, beta, rmean, rvar, smean,   \
                       sinv, nbt, M, C, nslab, momentum, eps, unbiased, relu, \
                       swz);                                                  \
    break;
    BN_OP_CFGS(BN_OP_CASE)
#undef BN_OP_CASE
  }
  HIP_CHECK(hipGetLastError());
}

template <bool RESID>
static void bn_op_launch_bwd(const void* X, const void* DY, const void* Z,
                             void* DRES, void* DX, const float* gamma,
                             const float* beta, const float* smean,
                             const float* sinv, float* dgamma, float* dbeta,
                             int64_t M, int C, int relu, int variant,
                             hipStream_t stream) {
  int cfg, swz;
  bn_op_resolve(variant, kBnOpPrefBwd, M, C, &cfg, &swz);
  const int nslab = bn_nslab(M, C);
  switch (cfg) {
#define BN_OP_CASE(id, Q, P, SPT, RPS)                                        \
  case id:                                                                    \
    hipLaunchKernelGGL((bn_onepass_bwd_kernel<Q, P, SPT, RPS, RESID>),        \
                       dim3(C / (Q * 4)), dim3(Q * P), 0, stream,             \
                       (const __hip_bfloat16*)X, (const __hip_bfloat16*)DY,   \
                       (const __hip_bfloat16*)Z, (__hip_bfloat16*)DRES,       \
                       (__hip_bfloat16*)DX, gamma, beta, smean, sinv, dgamma, \
                       dbeta, M, C, nslab, relu, swz);                        \
    break;
    BN_OP_CFGS(BN_OP_CASE)
#undef BN_OP_CASE
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_bn_onepass_fwd(const void* X, void* Y,
                                      const float* gamma, const float* beta,
                                      float* rmean, float* rvar, float* smean,
                                      float* sinv, unsigned long long* nbt,
                                      int64_t M, int C, float momentum,
                                      float eps, float unbiased, int relu,
                                      int variant, hipStream_t stream) {
  bn_op_launch_fwd<false>(X, nullptr, Y, gamma, beta, rmean, rvar, smean, sinv,
                          nbt, M, C, momentum, eps, unbiased, relu, variant,
                          stream);
}

extern "C" void flreid_bn_onepass_bwd(const void* X, const void* DY, void* DX,
                                      const float* gamma, const float* beta,
                                      const float* smean, const float* sinv,
                                      float* dgamma, float* dbeta, int64_t M,
                                      int C, int relu, int variant,
                                      hipStream_t stream) {
  bn_op_launch_bwd<false>(X, DY, nullptr, nullptr, DX, gamma, beta, smean,
                          sinv, dgamma, dbeta, M, C, relu, variant, stream);
}

extern "C" void flreid_bn_onepass_res_fwd(
    const void* X, const void* RES, void* Y, const float* gamma,
    const float* beta, float* rmean, float* rvar, float* smean, float* sinv,
    unsigned long long* nbt, int64_t M, int C, float momentum, float eps,
    float unbiased, int variant, hipStream_t stream) {
  if (RES == nullptr)
    throw std::invalid_argument("bn_onepass_res_fwd: no residual");
  bn_op_launch_fwd<true>(X, RES, Y, gamma, beta, rmean, rvar, smean, sinv, nbt,
                         M, C, momentum, eps, unbiased, 0, variant, stream);
}

extern "C" void flreid_bn_onepass_res_bwd(
    const void* X, const void* DZ, const void* Z, void* DRES, void* DX,
    const float* gamma, const float* beta, const float* smean,
    const float* sinv, float* dgamma, float* dbeta, int64_t M, int C,
    int variant, hipStream_t stream) {
  if (Z == nullptr)
    throw std::invalid_argument("bn_onepass_res_bwd: no saved output");
  bn_op_launch_bwd<true>(X, DZ, Z, DRES, DX, gamma, beta, smean, sinv, dgamma,
                         dbeta, M, C, 0, variant, stream);
}

}  // namespace flreid

// Triplet loss in Gram form, every mining / margin / metric mode (K5b in
// SURVEY.md §2.9; triplet.hip keeps the batch-hard euclidean margin mode).
//
// With G = F·Fᵀ both metrics are functions of G alone,
//
//   euclid: d_ij = G_ii + G_jj − 2·G_ij
//   cosine: d_ij = 1 − G_ij·r_i·r_j,           r_i = 1 / max(√G_ii, 1e-12)
//
// and with C_ij = ∂(Σ_i row_loss_i)/∂d_ij, S = C + Cᵀ, every gradient is
//
//   dF_i = (upstream / N)·(Σ_k W_ik·F_k + e_i·F_i)
//   euclid: W_ik = −2·S_ik,          e_i = 2·Σ_k S_ik          = −Σ_k W_ik
//   cosine: W_ik = −S_ik·r_i·r_k,    e_i = r_i²·Σ_k S_ik·cos_ik = −r_i²·Σ_k W_ik·G_ik
//
// so the loss is two small fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32, nothing
// rounded: G feeds arg-max decisions and differences of large numbers)
// around an O(N²) mining step.  Three launches, no atomics, no host
// synchronisation; every output element is written once, so loss and
// gradient have the same bits on every run.  1 ≤ N ≤ 512, any D ≥ 1.
//
// Gram phase (tg_gram_kernel): grid = (upper-triangle 64×64 tiles, KS).  A
//   workgroup is four waves, one 32×32 quadrant each, on K slice blockIdx.y
//   = [s·kc, min(D, (s+1)·kc)), kc a multiple of the 32-wide K panel.  KS is
//   chosen on the host so that tiles·KS fills the chip (N = 64, D = 2048:
//   one tile × 32 slices of 64).  The A and B panels are staged through LDS
//   with row stride 33 (conflict-free) while the next panel is prefetched
//   into registers; rows ≥ N and columns ≥ the slice end are staged as
//   zeros, so a slice past the end of D stores a slab of zeros.  Each slice
//   stores its partial tile into its own slab of the workspace at [r][c] and
//   [c][r] (r ≤ c), so the slabs are symmetric bit for bit.  The wave of a
//   diagonal tile that lies below the diagonal skips its MFMAs.
// Mining phase (tg_mine_kernel): one wave per anchor i, four anchors per
//   workgroup, lane l owning columns l, l+64, ….  The wave sums row i and
//   the diagonal of the slabs in slice order 0, 1, … (the fixed-order K
//   reduction: G_ij and G_ji, and G_jj seen from any row, are the same
//   bits), forms the distances, mines (batch-hard with first-index ties, or
//   the softmax weights with their max shift and +1e-6), evaluates the row
//   loss (hinge, or log1p(exp(−x)) in fp32 — it overflows where the fp32
//   eager chain does — plus the 0.3 hinge the soft-margin mode falls back
//   to) and writes row i of C for the loss and for the fallback.  C is the
//   derivative autograd takes of the eager chain: through the weights,
//   through the max shift (−ap·1e-6/z on the arg-max column when that column
//   is not masked) and, batch-hard, through the selected column only.  All
//   wave reductions are xor butterflies.  The cosine mode also writes the
//   reduced row of G and r_i for the gradient phase.
// Gradient phase (tg_grad_kernel): grid = (⌈D/64⌉, ⌈N/32⌉), two waves, each
//   a 32×32 tile of dF; K is N in panels of 32.  The W panel is formed while
//   it is staged: C[i][k] is read row-wise and stored, C[k][i] is read
//   row-wise as well and added through the transposed LDS address (stride
//   33, conflict-free both ways).  Thread r < 32 accumulates e_r from the
//   staged panel in k order.  The F panel is prefetched into registers.  The
//   soft-margin mode picks C or the fallback's C by a device flag; upstream
//   is read from device memory.

#include <algorithm>
#include <climits>

#include "common.h"
#include "ops.h"

namespace flreid {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int TG_MAX_N = 512;     // largest batch served
constexpr int TG_CPL = TG_MAX_N / 64;
constexpr int TG_T = 64;          // Gram tile
constexpr int TG_BK = 32;         // K panel, both GEMMs
constexpr int TG_PS = TG_BK + 1;  // its LDS row stride (odd: conflict-free)
constexpr int TG_MAX_KS = 32;     // most K slices
constexpr int TG_FILL = 256;      // workgroups that fill the chip
constexpr int TG_GC = 64;         // dF columns per gradient workgroup
constexpr float TG_FB_MARGIN = 0.3f;

// four floats at p; element e is read when e < nvalid, else 0.  VEC: p is
// 16-byte aligned and nvalid is 0 or ≥ 4.
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* p, int nvalid) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (VEC) {
    if (nvalid > 0) v = *(const float4*)p;
  } else {
    if (nvalid > 0) v.x = p[0];
    if (nvalid > 1) v.y = p[1];
    if (nvalid > 2) v.z = p[2];
    if (nvalid > 3) v.w = p[3];
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void tg_gram_kernel(
    const float* __restrict__ F, float* __restrict__ slabs, int N, int D,
    int kc) {
  __shared__ float pa[TG_T][TG_PS];
  __shared__ float pb[TG_T][TG_PS];
  // blockIdx.x-th tile (bi ≤ bj) of the upper triangle, row-major
  const int T = (N + TG_T - 1) / TG_T;
  int bi = 0, idx = blockIdx.x;
  while (idx >= T - bi) { idx -= T - bi; ++bi; }
  const int bj = bi + idx;
  const int r0 = bi * TG_T, c0 = bj * TG_T;
  const int kbeg = min(D, (int)blockIdx.y * kc);
  const int kend = min(D, kbeg + kc);
  float* P = slabs + (size_t)blockIdx.y * N * N;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int fr = lane & 31, fk = lane >> 5;

  // staging: 8 lanes cover one 32-float panel row, 32 rows per pass
  const int lrow = tid >> 3;
  const int lcol = (tid & 7) * 4;
  const float *ra[2], *rb[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int ar = r0 + p * 32 + lrow, br = c0 + p * 32 + lrow;
    ra[p] = ar < N ? F + (int64_t)ar * D + lcol : nullptr;
    rb[p] = br < N ? F + (int64_t)br * D + lcol : nullptr;
  }
  float4 va[2], vb[2];
  auto fetch = [&](int k0) {
    const int nv = kend - (k0 + lcol);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      va[p] = load4<VEC>(ra[p] + k0, ra[p] != nullptr ? nv : 0);
      vb[p] = load4<VEC>(rb[p] + k0, rb[p] != nullptr ? nv : 0);
    }
  };

  const bool below = bi == bj && wr > wc;   // nothing of this quadrant is kept
  f32x16 acc = {};
  fetch(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += TG_BK) {
    __syncthreads();   // the previous panel has been read
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float* da = &pa[p * 32 + lrow][lcol];
      float* db = &pb[p * 32 + lrow][lcol];
      da[0] = va[p].x; da[1] = va[p].y; da[2] = va[p].z; da[3] = va[p].w;
      db[0] = vb[p].x; db[1] = vb[p].y; db[2] = vb[p].z; db[3] = vb[p].w;
    }
    __syncthreads();
    if (k0 + TG_BK < kend) fetch(k0 + TG_BK);
    if (!below) {
#pragma unroll
      for (int kk = 0; kk < TG_BK; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(
            pa[wr + fr][kk + fk], pb[wc + fr][kk + fk], acc, 0, 0, 0);
    }
  }

  // C/D mapping: col = lane & 31, row = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5)
  const int c = c0 + wc + fr;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = r0 + wr + (reg & 3) + 8 * (reg >> 2) + 4 * fk;
    if (r <= c && c < N) {
      P[(int64_t)r * N + c] = acc[reg];
      P[(int64_t)c * N + r] = acc[reg];
    }
  }
}

// wave arg-max of (v, j): the largest v, the lowest j among equals
__device__ __forceinline__ void wave_argmax(float& v, int& j) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(v, off, 64);
    const int oj = __shfl_xor(j, off, 64);
    if (ov > v || (ov == v && oj < j)) { v = ov; j = oj; }
  }
}

__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// CPL·64 ≥ N.  margin is read in the hinge mode (soft == 0) only.
template <int CPL>
__global__ __launch_bounds__(256) void tg_mine_kernel(
    const float* __restrict__ slabs, int KS,
    const int64_t* __restrict__ labels, float* __restrict__ G,
    float* __restrict__ rinv, float* __restrict__ C, float* __restrict__ Cfb,
    float* __restrict__ row_loss, float* __restrict__ row_fb, int N,
    int cosine, int hard, int soft, float margin) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= N) return;   // a whole wave; the kernel has no block barrier
  const size_t NN = (size_t)N * N;

  // the K slices in the order 0, 1, …: row i, the diagonal, G_ii
  float g[CPL], gd[CPL];
  float gii = 0.f;
  for (int s = 0; s < KS; ++s) gii += slabs[s * NN + (size_t)i * N + i];
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    const int j = lane + 64 * t;
    g[t] = 0.f; gd[t] = 0.f;
    if (j < N) {
      for (int s = 0; s < KS; ++s) {
        g[t] += slabs[s * NN + (size_t)i * N + j];
        gd[t] += slabs[s * NN + (size_t)j * N + j];
      }
    }
  }

  const int64_t li = labels[i];
  const float ri = 1.0f / fmaxf(sqrtf(gii), 1e-12f);
  float d[CPL];
  bool in[CPL], pos[CPL];
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    const int j = lane + 64 * t;
    in[t] = j < N;
    pos[t] = in[t] && labels[in[t] ? j : i] == li;
    if (cosine) {
      const float rj = 1.0f / fmaxf(sqrtf(gd[t]), 1e-12f);
      d[t] = 1.0f - g[t] * ri * rj;
    } else {
      d[t] = (gii + gd[t]) - 2.0f * g[t];
    }
  }
  if (cosine) {
#pragma unroll
    for (int t = 0; t < CPL; ++t)
      if (in[t]) G[(size_t)i * N + lane + 64 * t] = g[t];
    if (lane == 0) rinv[i] = ri;
  }

  // dap[t] = ∂ap/∂d_j on positives, dan[t] = ∂an/∂d_j on negatives
  float ap, an, dap[CPL], dan[CPL];
  // max of d·pos (masked columns count as 0) and of −d·neg, first index
  float mp = -INFINITY, mn = -INFINITY;
  int jp = INT_MAX, jn = INT_MAX;
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    const int j = lane + 64 * t;
    if (!in[t]) continue;
    const float a = pos[t] ? d[t] : 0.0f;
    // batch-hard: −(d·neg + 1e9·pos), so that the min becomes a max
    const float b = pos[t] ? (hard ? -1e9f : 0.0f) : -d[t];
    if (a > mp) { mp = a; jp = j; }
    if (b > mn) { mn = b; jn = j; }
  }
  wave_argmax(mp, jp);
  wave_argmax(mn, jn);
  if (hard) {
    ap = mp;
    an = -mn;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int j = lane + 64 * t;
      dap[t] = j == jp ? 1.0f : 0.0f;
      dan[t] = j == jn ? 1.0f : 0.0f;
    }
  } else {
    float ep[CPL], en[CPL];
    float zp = 0.f, zn = 0.f;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      ep[t] = pos[t] ? expf(d[t] - mp) : 0.0f;
      en[t] = (in[t] && !pos[t]) ? expf(-d[t] - mn) : 0.0f;
      zp += ep[t];
      zn += en[t];
    }
    zp = wave_sum_all(zp) + 1e-6f;
    zn = wave_sum_all(zn) + 1e-6f;
    float sp = 0.f, sn = 0.f;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      ep[t] = ep[t] / zp;   // the weights
      en[t] = en[t] / zn;
      sp += d[t] * ep[t];   // 0 weight on masked columns
      sn += d[t] * en[t];
    }
    ap = wave_sum_all(sp);
    an = wave_sum_all(sn);
    const float shp = ap * 1e-6f / zp, shn = an * 1e-6f / zn;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int j = lane + 64 * t;
      dap[t] = ep[t] * (1.0f + d[t] - ap) - (j == jp ? shp : 0.0f);
      dan[t] = en[t] * (1.0f - d[t] + an) + (j == jn ? shn : 0.0f);
    }
  }

  // row loss and its derivative by ap (that by an is its negative)
  float loss, gp, loss_fb = 0.f, gp_fb = 0.f;
  if (soft) {
    const float z = expf(-(an - ap));
    loss = log1pf(z);
    gp = z / (1.0f + z);
    const float h = TG_FB_MARGIN + ap - an;
    loss_fb = fmaxf(h, 0.0f);
    gp_fb = h >= 0.0f ? 1.0f : 0.0f;
  } else {
    const float h = margin + ap - an;
    loss = fmaxf(h, 0.0f);
    gp = h >= 0.0f ? 1.0f : 0.0f;   // clamp_min passes the gradient at 0
  }
  if (lane == 0) {
    row_loss[i] = loss;
    if (soft) row_fb[i] = loss_fb;
  }
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    if (!in[t]) continue;
    const size_t o = (size_t)i * N + lane + 64 * t;
    const float dd = pos[t] ? dap[t] : -dan[t];
    C[o] = gp * dd;
    if (soft) Cfb[o] = gp_fb * dd;
  }
}

template <bool VEC>
__global__ __launch_bounds__(128) void tg_grad_kernel(
    const float* __restrict__ F, const float* __restrict__ C,
    const float* __restrict__ Cfb, const int* __restrict__ use_fb,
    const float* __restrict__ G, const float* __restrict__ rinv,
    const float* __restrict__ gscale, float* __restrict__ dF, int N, int D,
    int cosine) {
  __shared__ float Ws[32][TG_PS];
  __shared__ float Gs[32][TG_PS];
  __shared__ __attribute__((aligned(16))) float Fs[TG_BK][TG_GC];
  __shared__ float es[32];
  const float* Cs = (use_fb != nullptr && *use_fb != 0) ? Cfb : C;
  const int c0 = blockIdx.x * TG_GC, r0 = blockIdx.y * 32;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wc = (tid >> 6) * 32;
  const int fr = lane & 31, fk = lane >> 5;

  // W staging: 32 lanes cover one panel row, 4 rows per pass
  const int sk = tid & 31, sr = tid >> 5;
  // F staging: 16 lanes cover one 64-float panel row, 8 rows per pass
  const int frow = tid >> 4, fcol = (tid & 15) * 4;
  float4 vf[4];
  auto fetch = [&](int k0) {
    const int nv = D - (c0 + fcol);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int k = k0 + p * 8 + frow;
      // rows ≥ N read row N − 1's address and are zeroed by nvalid = 0
      vf[p] = load4<VEC>(F + (int64_t)min(k, N - 1) * D + c0 + fcol,
                         k < N ? nv : 0);
    }
  };

  const float ri_row = (cosine && r0 + sk < N) ? rinv[r0 + sk] : 1.0f;
  float e_acc = 0.f;   // threads 0..31: row r0 + tid
  f32x16 acc = {};
  fetch(0);
  for (int k0 = 0; k0 < N; k0 += TG_BK) {
    __syncthreads();   // the previous panel has been read
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int ii = sr + 4 * p;
      const int i = r0 + ii, k = k0 + sk;
      const bool live = i < N && k < N;
      float w = 0.f, gv = 0.f;
      if (live) {
        const float fac = cosine ? -(rinv[i] * rinv[k]) : -2.0f;
        w = fac * Cs[(size_t)i * N + k];
        if (cosine) gv = G[(size_t)i * N + k];
      }
      Ws[ii][sk] = w;
      Gs[ii][sk] = gv;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *(float4*)&Fs[p * 8 + frow][fcol] = vf[p];
    __syncthreads();
    // + fac·C[k][i], read row-wise, through the transposed address
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const int kk = sr + 4 * p;
      const int k = k0 + kk, i = r0 + sk;
      if (i < N && k < N) {
        const float fac = cosine ? -(ri_row * rinv[k]) : -2.0f;
        Ws[sk][kk] += fac * Cs[(size_t)k * N + i];
      }
    }
    __syncthreads();
    if (k0 + TG_BK < N) fetch(k0 + TG_BK);
    if (tid < 32) {
#pragma unroll
      for (int kk = 0; kk < TG_BK; ++kk)
        e_acc -= Ws[tid][kk] * (cosine ? Gs[tid][kk] : 1.0f);
    }
#pragma unroll
    for (int kk = 0; kk < TG_BK; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(
          Ws[fr][kk + fk], Fs[kk + fk][wc + fr], acc, 0, 0, 0);
  }
  if (tid < 32) es[tid] = cosine ? e_acc * ri_row * ri_row : e_acc;
  __syncthreads();

  const float scale = *gscale / (float)N;
  const int col = c0 + wc + fr;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = (reg & 3) + 8 * (reg >> 2) + 4 * fk;
    const int i = r0 + r;
    if (i < N && col < D) {
      const size_t o = (size_t)i * D + col;
      dF[o] = scale * (acc[reg] + es[r] * F[o]);
    }
  }
}

int tg_tiles(int N) {
  const int T = (N + TG_T - 1) / TG_T;
  return T * (T + 1) / 2;
}

bool tg_vec(const float* F, int D) {
  return D % 4 == 0 && (reinterpret_cast<uintptr_t>(F) & 15) == 0;
}

}  // namespace

extern "C" int flreid_triplet_gram_max_n() { return TG_MAX_N; }

extern "C" int flreid_triplet_gram_slices(int N, int D) {
  if (N < 1 || N > TG_MAX_N || D < 1)
    throw std::invalid_argument("triplet_gram: needs 1 <= N <= " +
                                std::to_string(TG_MAX_N) + " and D >= 1");
  const int fill = std::max(1, TG_FILL / tg_tiles(N));
  return std::min(std::min(fill, TG_MAX_KS), (D + TG_BK - 1) / TG_BK);
}

extern "C" void flreid_triplet_gram_fwd(
    const float* F, const int64_t* labels, float* slabs, float* G,
    float* rinv, float* C, float* C_fb, float* row_loss, float* row_fb, int N,
    int D, int cosine, int hard, int soft, float margin, hipStream_t stream) {
  const int KS = flreid_triplet_gram_slices(N, D);
  if (F == nullptr || labels == nullptr || slabs == nullptr || C == nullptr
      || row_loss == nullptr || (cosine && (G == nullptr || rinv == nullptr))
      || (soft && (C_fb == nullptr || row_fb == nullptr)))
    throw std::invalid_argument("triplet_gram_fwd: null pointer");
  if (!soft && !(margin > 0.0f))
    throw std::invalid_argument("triplet_gram_fwd: the hinge needs margin > 0");
  // K per slice: a multiple of the panel
  const int kc = ((D + KS - 1) / KS + TG_BK - 1) / TG_BK * TG_BK;
  const dim3 ggrid((unsigned)tg_tiles(N), (unsigned)KS);
  if (tg_vec(F, D))
    hipLaunchKernelGGL(tg_gram_kernel<true>, ggrid, dim3(256), 0, stream, F,
                       slabs, N, D, kc);
  else
    hipLaunchKernelGGL(tg_gram_kernel<false>, ggrid, dim3(256), 0, stream, F,
                       slabs, N, D, kc);
  HIP_CHECK(hipGetLastError());

  const dim3 mgrid((unsigned)((N + 3) / 4));
#define TG_MINE(CPL)                                                          \
  hipLaunchKernelGGL(tg_mine_kernel<CPL>, mgrid, dim3(256), 0, stream,        \
                     (const float*)slabs, KS, labels, G, rinv, C, C_fb,       \
                     row_loss, row_fb, N, cosine, hard, soft, margin)
  if (N <= 64) TG_MINE(1);
  else if (N <= 128) TG_MINE(2);
  else if (N <= 256) TG_MINE(4);
  else TG_MINE(TG_CPL);
#undef TG_MINE
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_triplet_gram_bwd(
    const float* F, const float* C, const float* C_fb, const int* use_fb,
    const float* G, const float* rinv, const float* gscale, float* dF, int N,
    int D, int cosine, hipStream_t stream) {
  if (N < 1 || N > TG_MAX_N || D < 1)
    throw std::invalid_argument("triplet_gram_bwd: needs 1 <= N <= " +
                                std::to_string(TG_MAX_N) + " and D >= 1");
  if (F == nullptr || C == nullptr || gscale == nullptr || dF == nullptr
      || (cosine && (G == nullptr || rinv == nullptr))
      || ((use_fb != nullptr) != (C_fb != nullptr)))
    throw std::invalid_argument(
        "triplet_gram_bwd: null pointer, or use_fb without C_fb");
  const dim3 grid((unsigned)((D + TG_GC - 1) / TG_GC),
                  (unsigned)((N + 31) / 32));
  if (tg_vec(F, D))
    hipLaunchKernelGGL(tg_grad_kernel<true>, grid, dim3(128), 0, stream, F, C,
                       C_fb, use_fb, G, rinv, gscale, dF, N, D, cosine);
  else
    hipLaunchKernelGGL(tg_grad_kernel<false>, grid, dim3(128), 0, stream, F,
                       C, C_fb, use_fb, G, rinv, gscale, dF, N, D, cosine);
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

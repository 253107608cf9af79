// Herding exemplar selection in Gram form (K10 in SURVEY.md §2.9).
//
// Herding picks, m times per identity, argmin_j ‖μ − (f_j + Σ picked)/(i+1)‖.
// With G = F·Fᵀ, c_j = (1/n)·Σ_k G[j,k] = ⟨f_j, μ⟩ and s_j = Σ_{picked p}
// G[j,p], the quantity minimised at step i is, up to a constant in j,
//
//   score_i(j) = G[j,j] − 2·((i+1)·c_j − s_j)
//
// so after one Gram matrix per identity a step is O(n) work on three
// n-vectors and one row of G: no D-wide work, no μ, no running sum, no padded
// copy of the features.  Rows are read through `order` (the stable sort of
// the rows by identity), and `sel` receives original row indices.
//
// Gram phase: fp32-input MFMA (v_mfma_f32_32x32x2_f32), nothing rounded —
// the result feeds an argmin.  Only tiles with block-row ≤ block-column are
// computed, and of a diagonal tile only the entries with row ≤ column are
// kept; the lower triangle is a copy of the upper one, so row j of G and
// column j are the same bits.  Rows beyond n are staged as zeros and are
// never candidates.
//
//  * n ≤ 128 (herding_lds_kernel): one workgroup of four waves per identity,
//    G stays in LDS.  A 32·T-row, 64-wide K panel is staged per step (next
//    panel prefetched into registers); each fragment row block serves as A
//    and as B.  How the four waves share the T(T+1)/2 tiles:
//      T ≤ 2 (1 or 3 tiles): every wave takes every tile on its own quarter
//        of each panel (split-K ×4) — there are fewer tiles than waves, and
//        the flagship shapes (8..40 rows of 2048) live here;
//      T ≥ 3 (6 or 10 tiles): two halves of the tile list × split-K ×2 —
//        the reduction below costs one pass over the tiles per K slice, so
//        it is halved once the tile list is long enough to fill two groups.
//    The K slices are reduced in LDS in a fixed order: slice 0 stores its
//    tiles into G, then slice 1 adds its own, … with a barrier in between.
//    No partial buffer exists.  G rows have stride 32·T + 1: row reads are
//    contiguous and the mirror's column writes hit distinct banks.
//  * 128 < n ≤ 1024: G lives in the caller's workspace (n² floats per such
//    identity).  herding_gram_ws_kernel runs one workgroup per 64×64 tile of
//    a host-built table over all large identities (four waves, one 32×32
//    quadrant each, full K), storing each kept value at [r][c] and [c][r];
//    herding_select_ws_kernel then runs the same selection loop on rows of G
//    read from global memory.
//
// Selection phase: ONE wave runs all m steps with no block barrier.  Lane l
// owns candidates l, l+64, … (d_j, c_j, s_j in registers).  A step computes
// the scores, takes the wave argmin of (score, position) by xor shuffles —
// ties go to the lowest position, repeats are allowed — adds row G[pick] to
// s (contiguous, conflict-free) and writes order[position] to `sel`.

#include <climits>
#include <type_traits>

#include "common.h"
#include "ops.h"

namespace flreid {

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int HD_LDS_MAX = 128;   // largest n whose G stays in LDS
constexpr int HD_WS_MAX = 1024;   // largest n served at all
constexpr int HD_BK = 64;         // K panel of the LDS kernel
constexpr int HD_PS = HD_BK + 1;  // its row stride (odd: conflict-free)
constexpr int HD_WT = 64;         // workspace Gram tile
constexpr int HD_WK = 32;         // its K panel
constexpr int HD_TILE_FIELDS = 5; // offset, n, tile row, tile col, ws offset

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// idx-th tile (bi ≤ bj) of the upper triangle of a T×T grid, row-major
constexpr int tri_bi(int T, int idx) {
  int bi = 0;
  while (idx >= T - bi) { idx -= T - bi; ++bi; }
  return bi;
}
constexpr int tri_bj(int T, int idx) {
  int bi = 0;
  while (idx >= T - bi) { idx -= T - bi; ++bi; }
  return bi + idx;
}

// LDS floats of the LDS kernel for T row blocks: G, the K panel, c
constexpr int hd_lds_floats(int T) {
  return 32 * T * (32 * T + 1) + 32 * T * HD_PS + 32 * T;
}

// G (stride 32·T + 1, full, mirrored) of the n ≤ 32·T rows ord[0..n) of
// feats, by all 256 threads; ends on a barrier.
template <int T>
__device__ __forceinline__ void gram_lds(const float* __restrict__ feats,
                                         const int* __restrict__ ord, int n,
                                         int D, float* G, float* panel) {
  constexpr int NP = 32 * T;
  constexpr int GS = NP + 1;
  constexpr int NTILE = T * (T + 1) / 2;
  constexpr int KS = T <= 2 ? 4 : 2;          // waves along K
  constexpr int TG = 4 / KS;                  // waves along the tile list
  constexpr int TPW = (NTILE + TG - 1) / TG;  // tiles per wave
  constexpr int KW = HD_BK / KS;              // k per wave per panel
  constexpr int NLD = NP / 16;                // float4 loads per thread

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int ks = wave % KS;
  const int tg = wave / KS;
  const int fr = lane & 31;   // fragment row / col within a 32-tile
  const int fk = lane >> 5;   // fragment k (0 / 1)

  // staging: 16 lanes cover one 64-float panel row, 16 rows per pass
  const int lrow = tid >> 4;
  const int lcol = (tid & 15) * 4;
  // rows beyond n read row n − 1 again and are zeroed on their way to LDS
  const float* rp[NLD];
#pragma unroll
  for (int p = 0; p < NLD; ++p)
    rp[p] = feats + (int64_t)ord[min(p * 16 + lrow, n - 1)] * D + lcol;
  float4 pre[NLD];
  auto fetch = [&](int k0) {
    const bool kin = k0 + lcol < D;
#pragma unroll
    for (int p = 0; p < NLD; ++p)
      pre[p] = kin ? *(const float4*)(rp[p] + k0)
                   : make_float4(0.f, 0.f, 0.f, 0.f);
  };

  f32x16 acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = f32x16{};

  // tile group TGI's MFMAs on fragments a[0..T)
  float a[T];
  auto mma = [&](auto tgc) {
    static_for<0, TPW>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      constexpr int idx = decltype(tgc)::value * TPW + t;
      if constexpr (idx < NTILE) {
        constexpr int bi = tri_bi(T, idx), bj = tri_bj(T, idx);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[bi], a[bj], acc[t],
                                                      0, 0, 0);
      }
    });
  };

  fetch(0);
  for (int k0 = 0; k0 < D; k0 += HD_BK) {
    __syncthreads();   // the previous panel has been read
#pragma unroll
    for (int p = 0; p < NLD; ++p) {
      float* dst = panel + (p * 16 + lrow) * HD_PS + lcol;
      const bool live = p * 16 + lrow < n;
      dst[0] = live ? pre[p].x : 0.f; dst[1] = live ? pre[p].y : 0.f;
      dst[2] = live ? pre[p].z : 0.f; dst[3] = live ? pre[p].w : 0.f;
    }
    __syncthreads();
    if (k0 + HD_BK < D) fetch(k0 + HD_BK);
#pragma unroll
    for (int kk = 0; kk < KW; kk += 2) {
#pragma unroll
      for (int b = 0; b < T; ++b)
        a[b] = panel[(b * 32 + fr) * HD_PS + ks * KW + kk + fk];
      if (TG == 1 || tg == 0) mma(std::integral_constant<int, 0>{});
      else mma(std::integral_constant<int, TG - 1>{});
    }
  }

  // K slices into G in the fixed order 0, 1, …  A diagonal tile is stored
  // whole; the mirror below then overwrites its lower half.
  // C/D mapping: col = lane & 31, row = (reg & 3) + 8·(reg >> 2) + 4·(lane >> 5)
  auto flush = [&](auto tgc, bool first) {
    static_for<0, TPW>([&](auto tc) {
      constexpr int t = decltype(tc)::value;
      constexpr int idx = decltype(tgc)::value * TPW + t;
      if constexpr (idx < NTILE) {
        constexpr int bi = tri_bi(T, idx), bj = tri_bj(T, idx);
        const int c = bj * 32 + fr;
        static_for<0, 16>([&](auto rc) {
          constexpr int reg = decltype(rc)::value;
          const int r = bi * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * fk;
          float* g = G + r * GS + c;
          *g = first ? acc[t][reg] : *g + acc[t][reg];
        });
      }
    });
  };
#pragma unroll
  for (int pass = 0; pass < KS; ++pass) {
    if (ks == pass) {
      if (TG == 1 || tg == 0) flush(std::integral_constant<int, 0>{}, pass == 0);
      else flush(std::integral_constant<int, TG - 1>{}, pass == 0);
    }
    __syncthreads();
  }
  // lower triangle := upper triangle
  for (int i = tid; i < NP * NP; i += 256) {
    const int r = i / NP, c = i % NP;
    if (r > c) G[r * GS + c] = G[c * GS + r];
  }
  __syncthreads();
}

// The m herding steps of one identity on one wave (lanes 0..63).  G is the
// full n×n Gram matrix with row stride gs, c the row means of G; `ord` maps
// positions to original rows.  CPL·64 ≥ n.
template <int CPL>
__device__ __forceinline__ void herd_select(const float* G, int gs,
                                            const float* cvec, int n, int m,
                                            const int* __restrict__ ord,
                                            int* __restrict__ sel_row) {
  const int lane = threadIdx.x & 63;
  float d[CPL], c[CPL], s[CPL];
#pragma unroll
  for (int t = 0; t < CPL; ++t) {
    const int j = lane + 64 * t;
    d[t] = j < n ? G[j * gs + j] : 0.f;
    c[t] = j < n ? cvec[j] : 0.f;
    s[t] = 0.f;
  }
  for (int i = 0; i < m; ++i) {
    const float w = (float)(i + 1);
    float best = INFINITY;
    int bpos = INT_MAX;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int j = lane + 64 * t;
      const float sc = d[t] - 2.0f * (w * c[t] - s[t]);
      if (j < n && sc < best) { best = sc; bpos = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ob = __shfl_xor(best, off, 64);
      const int op = __shfl_xor(bpos, off, 64);
      if (ob < best || (ob == best && op < bpos)) { best = ob; bpos = op; }
    }
    bpos = __builtin_amdgcn_readfirstlane(bpos);
    // no finite score at all (NaN / inf features): keep the row read in range
    if (bpos >= n) bpos = 0;
#pragma unroll
    for (int t = 0; t < CPL; ++t) {
      const int j = lane + 64 * t;
      if (j < n) s[t] += G[bpos * gs + j];
    }
    if (lane == 0) sel_row[i] = ord[bpos];
  }
}

__global__ __launch_bounds__(256) void herding_lds_kernel(
    const float* __restrict__ feats, const int* __restrict__ order,
    const int* __restrict__ offsets, int* __restrict__ sel, int n_lds, int D,
    int m) {
  extern __shared__ __attribute__((aligned(16))) float hd_smem[];
  const int p = blockIdx.x;
  const int off = offsets[p];
  const int n = offsets[p + 1] - off;
  // n_lds sized the LDS; anything larger is the workspace kernels' identity
  if (n < 1 || n > n_lds) return;
  const int T = (n + 31) / 32;
  const int NP = 32 * T, GS = NP + 1;
  float* G = hd_smem;
  float* panel = G + NP * GS;
  float* cvec = panel + NP * HD_PS;
  const int* ord = order + off;
  switch (T) {
    case 1: gram_lds<1>(feats, ord, n, D, G, panel); break;
    case 2: gram_lds<2>(feats, ord, n, D, G, panel); break;
    case 3: gram_lds<3>(feats, ord, n, D, G, panel); break;
    default: gram_lds<4>(feats, ord, n, D, G, panel); break;
  }
  // c_j: column j top to bottom (= row j, bit for bit), then / n
  const int tid = threadIdx.x;
  if (tid < n) {
    float sum = 0.f;
    for (int k = 0; k < n; ++k) sum += G[k * GS + tid];
    cvec[tid] = sum / (float)n;
  }
  __syncthreads();
  if (tid < 64)
    herd_select<HD_LDS_MAX / 64>(G, GS, cvec, n, m, ord, sel + (int64_t)p * m);
}

// One 64×64 tile (tile row ≤ tile col) of one large identity's G, stored to
// the workspace at [r][c] and [c][r] for r ≤ c < n.
__global__ __launch_bounds__(256) void herding_gram_ws_kernel(
    const float* __restrict__ feats, const int* __restrict__ order,
    const int* __restrict__ tiles, float* __restrict__ ws, int D) {
  __shared__ float pa[HD_WT][HD_WK + 1];
  __shared__ float pb[HD_WT][HD_WK + 1];
  const int* row = tiles + (int64_t)blockIdx.x * HD_TILE_FIELDS;
  const int* ord = order + row[0];
  const int n = row[1];
  const int r0 = row[2] * HD_WT, c0 = row[3] * HD_WT;
  float* G = ws + row[4];

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
    ra[p] = ar < n ? feats + (int64_t)ord[ar] * D + lcol : nullptr;
    rb[p] = br < n ? feats + (int64_t)ord[br] * D + lcol : nullptr;
  }
  float4 va[2], vb[2];
  auto fetch = [&](int k0) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool kin = k0 + lcol < D;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      va[p] = (ra[p] != nullptr && kin) ? *(const float4*)(ra[p] + k0) : zero;
      vb[p] = (rb[p] != nullptr && kin) ? *(const float4*)(rb[p] + k0) : zero;
    }
  };

  f32x16 acc = {};
  fetch(0);
  for (int k0 = 0; k0 < D; k0 += HD_WK) {
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float* da = &pa[p * 32 + lrow][lcol];
      float* db = &pb[p * 32 + lrow][lcol];
      da[0] = va[p].x; da[1] = va[p].y; da[2] = va[p].z; da[3] = va[p].w;
      db[0] = vb[p].x; db[1] = vb[p].y; db[2] = vb[p].z; db[3] = vb[p].w;
    }
    __syncthreads();
    if (k0 + HD_WK < D) fetch(k0 + HD_WK);
#pragma unroll
    for (int kk = 0; kk < HD_WK; kk += 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(
          pa[wr + fr][kk + fk], pb[wc + fr][kk + fk], acc, 0, 0, 0);
    }
  }

  const int c = c0 + wc + fr;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int r = r0 + wr + (reg & 3) + 8 * (reg >> 2) + 4 * fk;
    if (r <= c && c < n) {
      G[(int64_t)r * n + c] = acc[reg];
      G[(int64_t)c * n + r] = acc[reg];
    }
  }
}

__global__ __launch_bounds__(256) void herding_select_ws_kernel(
    const int* __restrict__ order, const int* __restrict__ offsets,
    const int* __restrict__ ws_offsets, const float* __restrict__ ws,
    int* __restrict__ sel, int m) {
  __shared__ float cvec[HD_WS_MAX];
  const int p = blockIdx.x;
  const int off = offsets[p];
  const int n = offsets[p + 1] - off;
  if (n <= HD_LDS_MAX || n > HD_WS_MAX) return;   // the LDS kernel's identity
  const float* G = ws + ws_offsets[p];
  const int tid = threadIdx.x;
  for (int j = tid; j < n; j += 256) {
    float sum = 0.f;
    for (int k = 0; k < n; ++k) sum += G[k * n + j];
    cvec[j] = sum / (float)n;
  }
  __syncthreads();
  if (tid < 64)
    herd_select<HD_WS_MAX / 64>(G, n, cvec, n, m, order + off,
                                sel + (int64_t)p * m);
}

}  // namespace

extern "C" int flreid_herding_lds_max() { return HD_LDS_MAX; }

extern "C" void flreid_herding_select(
    const float* feats, const int* order, const int* offsets, int* sel,
    float* gram_ws, const int* ws_offsets, const int* tiles, int n_tiles,
    int n_lds, int P, int D, int m, hipStream_t stream) {
  if (P < 1 || m < 1 || D < 4 || D % 4 != 0 || n_tiles < 0 || n_lds < 0
      || n_lds > HD_LDS_MAX)
    throw std::invalid_argument(
        "herding_select: needs P >= 1, m >= 1, D a positive multiple of 4, "
        "n_lds in [0, " + std::to_string(HD_LDS_MAX) + "]");
  if (feats == nullptr || order == nullptr || offsets == nullptr
      || sel == nullptr || (reinterpret_cast<uintptr_t>(feats) & 15) != 0)
    throw std::invalid_argument(
        "herding_select: null pointer, or feats not 16-byte aligned");
  if (n_tiles > 0 && (gram_ws == nullptr || ws_offsets == nullptr
                      || tiles == nullptr))
    throw std::invalid_argument(
        "herding_select: a tile table needs gram_ws and ws_offsets");
  if (n_lds > 0) {
    const int lds_bytes = hd_lds_floats((n_lds + 31) / 32) * (int)sizeof(float);
    HIP_CHECK(hipFuncSetAttribute((const void*)herding_lds_kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize,
                                  lds_bytes));
    hipLaunchKernelGGL(herding_lds_kernel, dim3((unsigned)P), dim3(256),
                       lds_bytes, stream, feats, order, offsets, sel, n_lds, D,
                       m);
    HIP_CHECK(hipGetLastError());
  }
  if (n_tiles > 0) {
    hipLaunchKernelGGL(herding_gram_ws_kernel, dim3((unsigned)n_tiles),
                       dim3(256), 0, stream, feats, order, tiles, gram_ws, D);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(herding_select_ws_kernel, dim3((unsigned)P), dim3(256),
                       0, stream, order, offsets, ws_offsets,
                       (const float*)gram_ws, sel, m);
    HIP_CHECK(hipGetLastError());
  }
}

}  // namespace flreid

// Shifted-window MFMA attention straight on the feature map, for Swin windows
// of 1..64 tokens (ws <= 8), head dim 32, bf16 — forward and backward.  qkv
// and dqkv are [B][Hi][Wi][3·C] (C = H·32, last axis ordered (q|k|v, head,
// d)), out and dout [B][Hi][Wi][C], all in image order: the cyclic shift, the
// window partition, its reverse and the shift back are address arithmetic
// here, and the shift mask is formed from region labels in registers.
//
// Window bw = b·nW + wy·nWx + wx, token n = ny·ws + nx:
//   rolled coordinates   y' = wy·ws + ny,          x' = wx·ws + nx
//   pixel read / written y  = (y' + shift) mod Hi,  x = (x' + shift) mod Wi
//   label  3·ry + rx,    ry = (y' >= Hi − ws) + (y' >= Hi − shift), rx alike
//   S = scale·Q·Kᵀ + bias[h] + (label_i == label_j ? 0 : −100)
// which is roll(−shift), window_partition, window_attn_qkv.hip with the
// model's shift mask of window bw % nW, window_reverse, roll(+shift).  Every
// pixel belongs to one token of one window, so out and dqkv are written
// exactly once everywhere.
//
// The math, the transposed strips, the two-pass backward, the in-order dbias
// reduction and one wave per (window, head) are those of window_attn_qkv.hip
// (design notes there; shared helpers in window_attn_wq.h).  New here:
//  - row table: a lane's (ny, nx) for token `lane` never changes, so the one
//    division by ws happens once per kernel.  Per window lane n < N forms
//    token n's pixel index y·Wi + x in its image and, in the shifted
//    instances, its label, and writes them to two wave-private LDS tables
//    (64 ints, 64 bytes).  Every fragment load and row store touches token
//    16·t + fr and reads its pixel there in place of the row number; the
//    offset pixel·stride is a 32-bit byte offset from the IMAGE base (a
//    shifted window's tokens wrap, so there is no window base), which the
//    host check keeps below 2³¹.  The tables sit in LDS and not in
//    registers: the NT = 4 backward has none to spare.
//  - labels: in the transposed strip a lane holds one query (one byte read
//    per strip) and, per key tile, keys 16·kt + 4·kg + 0..3, whose labels
//    are ONE dword of the byte table.  In pass 2 the roles swap.  The mask
//    term is added in fp32 where window_attn_qkv.hip adds the loaded one.
//    shift == 0 instances hold no label code.
//
// Resources, from the compiler's resource summary (hipcc -O3, gfx950,
// packed fp32 off), shifted instances (all sixteen in profiles/README.md):
//   fwd NT = 1:  33 VGPRs +   8 AGPRs, no spill, 11 520 B static LDS
//   fwd NT = 4: 106 VGPRs +   8 AGPRs, no spill, 19 712 B static LDS
//   bwd NT = 1:  72 VGPRs +  12 AGPRs, no spill, 24 832 B static LDS
//   bwd NT = 4: 256 VGPRs + 156 AGPRs, no spill, 41 216 B static LDS
// No instance spills; the tables cost 320 B of LDS per wave.

#include "common.h"
#include "ops.h"
#include "window_attn_wq.h"

#include <initializer_list>

namespace flreid {

namespace {

using namespace wq;

// ints of one wave's tables: pixel index per token, then the label bytes
constexpr int WM_TAB = 64 + 16;

// Where this window's tokens lie.  (ny, nx) are the lane's own token's
// window coordinates; lanes >= N write zeros.
template <bool SHIFTED>
__device__ __forceinline__ void wm_put_tables(int* tab, int lane, int N, int ny,
                                              int nx, int y0, int x0, int Hi,
                                              int Wi, int ws, int shift) {
  const int yr = y0 + ny, xr = x0 + nx;       // rolled coordinates
  int y = yr, x = xr;
  if (SHIFTED) {
    y += shift;
    x += shift;
    y = y >= Hi ? y - Hi : y;
    x = x >= Wi ? x - Wi : x;
  }
  tab[lane] = lane < N ? y * Wi + x : 0;
  if (SHIFTED) {
    const int lab = 3 * ((yr >= Hi - ws) + (yr >= Hi - shift)) +
                    (xr >= Wi - ws) + (xr >= Wi - shift);
    ((unsigned char*)(tab + 64))[lane] = (unsigned char)(lane < N ? lab : 0);
  }
}

// The NT fragments of one head's [N][32] matrix on the map (g is the image
// base plus the head's column, wave-uniform; rows are `stride` elements
// apart): f[t] = g[pixel of token 16·t + fr][8·kg .. 8·kg + 7], zero for
// tokens >= N.
template <int NT>
__device__ __forceinline__ void wm_load_frags(
    const __hip_bfloat16* __restrict__ g, const int* tab, int stride, int N,
    int lane, u16x8 (&f)[NT]) {
  const int fr = lane & 15, kg = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int row = t * 16 + fr;
    f[t] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (row < N) f[t] = *(const u16x8*)wq_at(g, tab[row] * stride + kg * 8);
  }
}

// one token's fragment
__device__ __forceinline__ u16x8 wm_load_frag(
    const __hip_bfloat16* __restrict__ g, const int* tab, int stride, int N,
    int row, int kg) {
  u16x8 f = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < N) f = *(const u16x8*)wq_at(g, tab[row] * stride + kg * 8);
  return f;
}

// 0 / −100 for the four labels in the bytes of `four` against `mine`
__device__ __forceinline__ f32x4 wm_mask4(unsigned four, unsigned mine) {
  f32x4 mk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    mk[r] = ((four >> (8 * r)) & 0xffu) == mine ? 0.f : -100.f;
  }
  return mk;
}

// wq_probs of window_attn_qkv.hip with the mask from the label table
template <int NT, bool SHIFTED>
__device__ __forceinline__ void wm_probs(u16x8 qf, const u16x8 (&kf)[NT],
                                         const float* __restrict__ brow,
                                         const int* tab, int N, int i,
                                         int lane, float scale,
                                         f32x4 (&p)[NT], float& m,
                                         float& inv) {
  const int kg = lane >> 4;
  const int row = min(i, N - 1) * N;
  unsigned li = 0;
  if (SHIFTED) li = ((const unsigned char*)(tab + 64))[i];
  m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    const f32x4 acc = wq_mfma(kf[kt], qf, f32x4{0.f, 0.f, 0.f, 0.f});
    const int j0 = kt * 16 + kg * 4;
    const f32x4 b = wq_load4(brow, row, j0, N, kt == NT - 1);
    f32x4 mk = {0.f, 0.f, 0.f, 0.f};
    if (SHIFTED) mk = wm_mask4((unsigned)tab[64 + 4 * kt + kg], li);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s = acc[r] * scale + b[r];
      s += mk[r];
      s = (j0 + r < N) ? s : -INFINITY;
      p[kt][r] = s;
      m = fmaxf(m, s);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float se = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = __expf(p[kt][r] - m);
      p[kt][r] = e;
      se += e;
    }
  }
  se += __shfl_xor(se, 16, 64);
  se += __shfl_xor(se, 32, 64);
  inv = (i < N) ? 1.0f / se : 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) p[kt][r] *= inv;
  }
}

// out[dt][0..3] · mul -> g[pixel of token i][16·dt + 4·kg ..] as bf16 (8-byte
// stores), rows `stride` elements apart
__device__ __forceinline__ void wm_store_rows(__hip_bfloat16* __restrict__ g,
                                              const int* tab, int stride,
                                              int i, int N, int kg,
                                              const f32x4 (&out)[2],
                                              float mul) {
  if (i >= N) return;
  const int at = tab[i] * stride + kg * 4;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    u16x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) o[r] = wq_bf16(out[dt][r] * mul);
    *(u16x4*)wq_at(g, at + dt * 16) = o;
  }
}

// The geometry the kernels take: everything the host can divide once.
struct WmGeom {
  int Hi, Wi, ws, shift, nWx, nW, N;
};

template <int NT, bool SHIFTED>
__global__ __launch_bounds__(256) void window_attn_map_fwd_kernel(
    const __hip_bfloat16* __restrict__ QKV, const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ O, int64_t WH, int H, WmGeom gm,
    float scale) {
  constexpr int TB = WQ_D * wq_ts(NT);
  __shared__ __attribute__((aligned(16))) unsigned short lds[4 * TB];
  __shared__ int tabs[4 * WM_TAB];

  const int lane = threadIdx.x & 63;
  // uniform to the compiler too: the bases below are scalar
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t wh = (int64_t)blockIdx.x * 4 + wave;
  if (wh >= WH) return;                       // wave-uniform; no barriers
  const int bw = (int)(wh / H);
  const int h = (int)(wh % H);
  const int N = gm.N, C = H * WQ_D;
  const int b = bw / gm.nW, w = bw - b * gm.nW;
  const int wy = w / gm.nWx, wx = w - wy * gm.nWx;
  const int64_t img = (int64_t)b * (gm.Hi * gm.Wi);
  const __hip_bfloat16* q0 = QKV + img * 3 * C + h * WQ_D;
  __hip_bfloat16* o0 = O + img * C + h * WQ_D;
  unsigned short* lvT = lds + wave * TB;
  int* tab = tabs + wave * WM_TAB;
  const int fr = lane & 15, kg = lane >> 4;

  wm_put_tables<SHIFTED>(tab, lane, N, lane / gm.ws, lane % gm.ws,
                         wy * gm.ws, wx * gm.ws, gm.Hi, gm.Wi, gm.ws,
                         gm.shift);
  wq_wave_sync();

  u16x8 kf[NT], vf[NT];
  wm_load_frags<NT>(q0 + C, tab, 3 * C, N, lane, kf);
  wm_load_frags<NT>(q0 + 2 * C, tab, 3 * C, N, lane, vf);
  wq_put_transposed<NT>(lvT, vf, lane);
  wq_wave_sync();

  const float* brow = bias + (int64_t)h * N * N;

#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
    const int i = qt * 16 + fr;
    const u16x8 qf = wm_load_frag(q0, tab, 3 * C, N, i, kg);
    f32x4 p[NT];
    float m, inv;
    wm_probs<NT, SHIFTED>(qf, kf, brow, tab, N, i, lane, scale, p, m, inv);
    u16x4 pb[NT];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pb[kt][r] = wq_bf16(p[kt][r]);
    }
    f32x4 o[2];
    wq_strip_times<NT>(pb, lvT, lane, o);
    wm_store_rows(o0, tab, C, i, N, kg, o, 1.0f);
  }
}

// LDS of one backward wave in elements: that of window_attn_qkv.hip and the
// tables
constexpr int wm_bwd_wave_elems(int NT) {
  return wq_bwd_wave_elems(NT) + 2 * WM_TAB;
}

template <int NT, bool SHIFTED>
__global__ __launch_bounds__(256) void window_attn_map_bwd_kernel(
    const __hip_bfloat16* __restrict__ QKV, const float* __restrict__ bias,
    const __hip_bfloat16* __restrict__ DO, __hip_bfloat16* __restrict__ DQKV,
    float* __restrict__ DBP, int BW, int H, WmGeom gm, float scale) {
  constexpr int TB = WQ_D * wq_ts(NT);
  constexpr int WE = wm_bwd_wave_elems(NT);
  __shared__ __attribute__((aligned(16))) unsigned short lds[4 * WE];
  // the dbias reduction passes one wave's NT² float4 per lane through it
  static_assert(4 * WE * 2 >= NT * NT * 64 * 16, "reduction needs the LDS");
  static_assert(WE % 8 == 0, "a wave's LDS stays 16-byte aligned");

  const int h = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int fr = lane & 15, kg = lane >> 4;
  const int N = gm.N, C = H * WQ_D;
  unsigned short* lA = lds + wave * WE;       // Kᵀ in pass 1, Qᵀ in pass 2
  unsigned short* lB = lA + TB;               // dOᵀ
  float* stat = (float*)(lB + TB);            // [3][64]: max, 1/sum, rd
  int* tab = (int*)(stat + 192);              // pixels, labels
  const bool vec4 = (N & 3) == 0;
  const int ny = lane / gm.ws, nx = lane % gm.ws;

  f32x4 dsacc[NT][NT];
#pragma unroll
  for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) dsacc[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

#pragma unroll 1
  for (int g = wave; g < WQ_GROUP; g += 4) {
    const int bw = (int)blockIdx.x * WQ_GROUP + wq_opaque(g);
    if (bw >= BW) break;                      // wave-uniform; no barriers
    const int hq = wq_opaque(h);
    const int b = bw / gm.nW, w = bw - b * gm.nW;
    const int wy = w / gm.nWx, wx = w - wy * gm.nWx;
    const int64_t img = (int64_t)b * (gm.Hi * gm.Wi);
    const __hip_bfloat16* q0 = QKV + img * 3 * C + hq * WQ_D;
    const __hip_bfloat16* do0 = DO + img * C + hq * WQ_D;
    __hip_bfloat16* dq0 = DQKV + img * 3 * C + hq * WQ_D;
    const float* brow = bias + (int64_t)hq * N * N;

    wq_wave_sync();                           // the last window's reads
    wm_put_tables<SHIFTED>(tab, lane, N, ny, nx, wy * gm.ws, wx * gm.ws,
                           gm.Hi, gm.Wi, gm.ws, gm.shift);
    wq_wave_sync();

    // Registers: K and V fragments live through pass 1, Q and dO fragments
    // through pass 2; the other pair comes per tile from global memory (L2
    // hits).  All four resident next to dsacc would spill at NT = 4.
    u16x8 kf[NT], vf[NT];
    wm_load_frags<NT>(q0 + C, tab, 3 * C, N, lane, kf);
    wm_load_frags<NT>(q0 + 2 * C, tab, 3 * C, N, lane, vf);
    wq_put_transposed<NT>(lA, kf, lane);
    {
      u16x8 dof[NT];
      wm_load_frags<NT>(do0, tab, C, N, lane, dof);
      wq_put_transposed<NT>(lB, dof, lane);
    }
    wq_wave_sync();

    // pass 1: lane = one query, 4 keys per key tile
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
      // keep the strips apart: hoisting the next strip's bias loads over
      // this one's arithmetic costs more registers than there are
      __builtin_amdgcn_sched_barrier(0);
      const int i = qt * 16 + fr;
      const u16x8 qfi = wm_load_frag(q0, tab, 3 * C, N, i, kg);
      const u16x8 dofi = wm_load_frag(do0, tab, C, N, i, kg);
      f32x4 p[NT];
      float m, inv;
      wm_probs<NT, SHIFTED>(qfi, kf, brow, tab, N, i, lane, scale, p, m,
                            inv);
      f32x4 dp[NT];
      float rd = 0.f;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        dp[kt] = wq_mfma(vf[kt], dofi, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) rd += dp[kt][r] * p[kt][r];
      }
      rd += __shfl_xor(rd, 16, 64);
      rd += __shfl_xor(rd, 32, 64);
      if (kg == 0) {
        stat[i] = m;
        stat[64 + i] = inv;
        stat[128 + i] = rd;
      }
      u16x4 dsb[NT];
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float ds = p[kt][r] * (dp[kt][r] - rd);
          dsacc[qt][kt][r] += ds;
          dsb[kt][r] = wq_bf16(ds);
        }
      }
      f32x4 dq[2];
      wq_strip_times<NT>(dsb, lA, lane, dq);
      wm_store_rows(dq0, tab, 3 * C, i, N, kg, dq, scale);
    }
    wq_wave_sync();                           // Kᵀ is done with
    // (the opaque zero keeps these loads from being merged with pass 1's)
    u16x8 qf[NT], dof[NT];
    wm_load_frags<NT>(q0 + wq_opaque(0), tab, 3 * C, N, lane, qf);
    wm_load_frags<NT>(do0 + wq_opaque(0), tab, C, N, lane, dof);
    wq_put_transposed<NT>(lA, qf, lane);
    wq_wave_sync();

    // pass 2: lane = one key, 4 queries per query tile.  A rolled loop:
    // the key tile's K and V fragments come from global memory again (L2
    // hits) so that nothing is indexed by kt.
#pragma unroll 1
    for (int kt = 0; kt < NT; ++kt) {
      const int j = kt * 16 + fr;
      const u16x8 kfj = wm_load_frag(q0 + C, tab, 3 * C, N, j, kg);
      const u16x8 vfj = wm_load_frag(q0 + 2 * C, tab, 3 * C, N, j, kg);
      unsigned lj = 0;
      if (SHIFTED) lj = ((const unsigned char*)(tab + 64))[j];
      u16x4 pb[NT], dsb[NT];
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
        __builtin_amdgcn_sched_barrier(0);    // as in pass 1
        const int i0 = qt * 16 + kg * 4;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 s = wq_mfma(qf[qt], kfj, zero);
        const f32x4 dp = wq_mfma(dof[qt], vfj, zero);
        const f32x4 b = wq_load_col(brow, i0, j, N);
        f32x4 mk = {0.f, 0.f, 0.f, 0.f};
        if (SHIFTED) mk = wm_mask4((unsigned)tab[64 + 4 * qt + kg], lj);
        const f32x4 m4 = *(const f32x4*)(stat + i0);
        const f32x4 inv4 = *(const f32x4*)(stat + 64 + i0);
        const f32x4 rd4 = *(const f32x4*)(stat + 128 + i0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv = s[r] * scale + b[r];
          sv += mk[r];
          sv = (j < N) ? sv : -INFINITY;
          // a query >= N has inv = 0 and a finite max: P = 0
          const float pv = __expf(sv - m4[r]) * inv4[r];
          pb[qt][r] = wq_bf16(pv);
          dsb[qt][r] = wq_bf16(pv * (dp[r] - rd4[r]));
        }
      }
      f32x4 dv[2], dk[2];
      wq_strip_times<NT>(pb, lB, lane, dv);
      wm_store_rows(dq0 + 2 * C, tab, 3 * C, j, N, kg, dv, 1.0f);
      wq_strip_times<NT>(dsb, lA, lane, dk);
      wm_store_rows(dq0 + C, tab, 3 * C, j, N, kg, dk, scale);
    }
  }

  // dbias partial of the run: waves 1, 2, 3 into wave 0, in that order
  f32x4* red = (f32x4*)lds;
  __syncthreads();
#pragma unroll 1
  for (int w = 1; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          red[(qt * NT + kt) * 64 + lane] = dsacc[qt][kt];
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
          dsacc[qt][kt] += red[(qt * NT + kt) * 64 + lane];
        }
      }
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* part = DBP + ((int64_t)blockIdx.x * H + h) * (int64_t)N * N;
#pragma unroll
    for (int qt = 0; qt < NT; ++qt) {
#pragma unroll
      for (int kt = 0; kt < NT; ++kt) {
        wq_store4(part, qt * 16 + fr, kt * 16 + kg * 4, N, vec4,
                  dsacc[qt][kt]);
      }
    }
  }
}

// Checks the geometry and returns it; BW = B·nW through *BW.
WmGeom wm_check(const char* who, int B, int Hi, int Wi, int ws, int shift,
                int H, int64_t* BW, std::initializer_list<const void*> ptrs) {
  const std::string w(who);
  if (ws < 1 || ws > 8) throw std::runtime_error(w + ": needs 1 <= ws <= 8");
  if (B <= 0 || H <= 0 || H > 65535 || Hi <= 0 || Wi <= 0 || Hi % ws ||
      Wi % ws || shift < 0 || shift >= ws) {
    throw std::runtime_error(
        w + ": needs B, H > 0, Hi and Wi multiples of ws, 0 <= shift < ws");
  }
  // a token's byte offset from its image base is a 32-bit int
  if ((int64_t)Hi * Wi * 3 * H * WQ_D * 2 >= ((int64_t)1 << 31)) {
    throw std::runtime_error(w + ": one image of qkv must stay below 2 GiB");
  }
  const int nWx = Wi / ws, nW = (Hi / ws) * nWx;
  *BW = (int64_t)B * nW;
  if (*BW * H > (int64_t)0x7fffffff) {
    throw std::runtime_error(w + ": too many (window, head) pairs");
  }
  for (const void* p : ptrs) {
    if (!p || ((uintptr_t)p & 15)) {
      throw std::runtime_error(w + ": pointers must be 16-byte aligned");
    }
  }
  return WmGeom{Hi, Wi, ws, shift, nWx, nW, ws * ws};
}

}  // namespace

extern "C" void flreid_window_attn_map_fwd(const void* qkv, const float* bias,
                                           void* out, int B, int Hi, int Wi,
                                           int ws, int shift, int H,
                                           float scale, hipStream_t stream) {
  int64_t BW;
  const WmGeom gm = wm_check("window_attn_map_fwd", B, Hi, Wi, ws, shift, H,
                             &BW, {qkv, bias, out});
  const int64_t WH = BW * H;
  dim3 grid((unsigned)((WH + 3) / 4)), block(256);
  switch ((gm.N + 15) / 16) {
#define FLREID_WM_CASE(NT)                                                    \
  case NT:                                                                    \
    if (shift) {                                                              \
      hipLaunchKernelGGL((window_attn_map_fwd_kernel<NT, true>), grid, block, \
                         0, stream, (const __hip_bfloat16*)qkv, bias,         \
                         (__hip_bfloat16*)out, WH, H, gm, scale);             \
    } else {                                                                  \
      hipLaunchKernelGGL((window_attn_map_fwd_kernel<NT, false>), grid,       \
                         block, 0, stream, (const __hip_bfloat16*)qkv, bias,  \
                         (__hip_bfloat16*)out, WH, H, gm, scale);             \
    }                                                                         \
    break;
    FLREID_WM_CASE(1)
    FLREID_WM_CASE(2)
    FLREID_WM_CASE(3)
    FLREID_WM_CASE(4)
#undef FLREID_WM_CASE
  }
  HIP_CHECK(hipGetLastError());
}

extern "C" void flreid_window_attn_map_bwd(const void* qkv, const float* bias,
                                           const void* dout, void* dqkv,
                                           float* dbias_part, int B, int Hi,
                                           int Wi, int ws, int shift, int H,
                                           float scale, hipStream_t stream) {
  int64_t BW;
  const WmGeom gm = wm_check("window_attn_map_bwd", B, Hi, Wi, ws, shift, H,
                             &BW, {qkv, bias, dout, dqkv, dbias_part});
  dim3 grid((unsigned)((BW + WQ_GROUP - 1) / WQ_GROUP), (unsigned)H);
  dim3 block(256);
  switch ((gm.N + 15) / 16) {
#define FLREID_WM_CASE(NT)                                                    \
  case NT:                                                                    \
    if (shift) {                                                              \
      hipLaunchKernelGGL((window_attn_map_bwd_kernel<NT, true>), grid, block, \
                         0, stream, (const __hip_bfloat16*)qkv, bias,         \
                         (const __hip_bfloat16*)dout, (__hip_bfloat16*)dqkv,  \
                         dbias_part, (int)BW, H, gm, scale);                  \
    } else {                                                                  \
      hipLaunchKernelGGL((window_attn_map_bwd_kernel<NT, false>), grid,       \
                         block, 0, stream, (const __hip_bfloat16*)qkv, bias,  \
                         (const __hip_bfloat16*)dout, (__hip_bfloat16*)dqkv,  \
                         dbias_part, (int)BW, H, gm, scale);                  \
    }                                                                         \
    break;
    FLREID_WM_CASE(1)
    FLREID_WM_CASE(2)
    FLREID_WM_CASE(3)
    FLREID_WM_CASE(4)
#undef FLREID_WM_CASE
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

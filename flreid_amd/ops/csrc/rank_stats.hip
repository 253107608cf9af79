// Sort-free CMC / AP rank statistics of one [Qc, G] similarity tile (K8).
//
// For one query, CMC and AP are functions of (a) the order of its good
// gallery entries among themselves and (b) for each good entry the number of
// valid (non-junk) entries ranking ahead of it.  The good entries are few and
// the row is long, so nothing sorts the row: the good similarities are sorted
// (a handful of keys), and one streaming pass over the row counts every other
// entry against them.  Only comparisons of the same fp32 values are involved,
// so the integers are the ones the stable argsort of the row gives.
//
// Ranking: entry a ranks ahead of entry b iff sim_a > sim_b, or sim_a == sim_b
// and index_a > index_b (np.argsort(sim)[::-1]: the higher index wins a tie;
// −0.0 == +0.0 is a tie; inputs are finite).
//
// With the gallery labels sorted once per evaluation (`perm`), a query's
// same-id entries are the segment perm[lo, hi) and the gallery's −1 entries
// another.  Camera mode: a same-id entry is junk when its camera is the
// query's and good otherwise, and the −1 segment is junk; without cameras
// every same-id entry is good and nothing is junk.
//
// Three launches per tile.  This departs from one fused kernel: the row split
// that the large-gallery tile needs would otherwise repeat the candidate
// gather and the key sort in every slice of a row.
//
//  1. rank_keys_kernel, one workgroup per row.  Walks the query's segment,
//     gathers (sims[q, j], j) of the good entries into LDS, bitonic-sorts them
//     into rank order over the next power of two (pads are (−inf, −1) and rank
//     last), and writes the keys to the workspace.  Then the junk entries —
//     enumerable: the −1 segment and the same-camera candidates — binary-search
//     the keys and increment jhist[b], b = number of keys ranking ahead of the
//     entry; entries behind every key (b == n_good) are dropped.
//  2. rank_count_kernel, `splits` workgroups per row, each one contiguous
//     slice of the row: scalar head up to 16-byte alignment of the ADDRESS
//     (rows start misaligned when G % 4 != 0, and the tile may itself start
//     inside an allocation), float4 body with four loads in flight per lane,
//     scalar tail.  An element first takes one compare against the weakest
//     key: what ranks behind every good hit is dropped, since no count needs
//     it and in a trained model it is almost the whole row (it also keeps the
//     last bin from being a hot spot).  The others binary-search the keys in
//     LDS and increment hist[b] there; the slice's histogram goes to the
//     workspace with plain stores — no global atomics, nothing to clear.
//     A good entry finds b == its own position, so it counts itself once.
//  3. rank_finish_kernel, one workgroup per row.  net[p] = Σ_slices hist[p] −
//     jhist[p]; an inclusive block scan gives the junk-free rank r_p =
//     prefix[p] − 1; the AP terms ((p+1)/(r_p+1) + (r_p > 0 ? p/r_p : 1))/2 are
//     formed in double by every lane and reduced once; first_rank = r_0.
//
// Launch shape: splits = min(ceil(G / 8192), max(1, 2048 / Qc)) — about 2048
// workgroups of 256 threads whenever the tile is large enough.  The 256 × 1M
// chunk runs 8 slices of 131k columns per row (2048 workgroups, 8 per CU);
// a 3000 × 20k split runs one workgroup per row.  LDS is 12 bytes per padded
// key (keys, indices, histogram): 768 B at the common ≤ 64 good entries (LDS
// never limits occupancy: 8 workgroups = 32 waves per CU), 48 KB at the cap
// of 4096 keys (3 workgroups per CU of the 160 KB).

#include <cmath>

#include "common.h"
#include "ops.h"

namespace flreid {

namespace {

constexpr int RS_BLOCK = 256;
constexpr int RS_MAX_GOOD = 4096;   // keys one query may hold (48 KB of LDS)
constexpr int RS_MIN_PAD = 64;
constexpr int RS_SLICE_MIN = 8192;  // columns below which a row is not split
constexpr int RS_TARGET_WGS = 2048;

__host__ __device__ inline int rs_pad(int kmax) {
  int kp = RS_MIN_PAD;
  while (kp < kmax) kp <<= 1;
  return kp;
}

inline int rs_splits(int64_t Qc, int64_t G) {
  const int64_t by_len = (G + RS_SLICE_MIN - 1) / RS_SLICE_MIN;
  const int64_t by_fill = RS_TARGET_WGS / Qc > 1 ? RS_TARGET_WGS / Qc : 1;
  return (int)(by_len < by_fill ? by_len : by_fill);
}

__device__ __forceinline__ bool ahead(float sa, int ja, float sb, int jb) {
  return sa > sb || (sa == sb && ja > jb);
}

// number of the n sorted keys that rank ahead of (s, j)
__device__ __forceinline__ int keys_ahead(const float* ks, const int* ki,
                                          int n, float s, int j) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ahead(ks[mid], ki[mid], s, j)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// workspace, in int32 units, Kp = rs_pad(kmax): key sims [Qc][Kp] (fp32
// bits), key indices [Qc][Kp], junk histograms [Qc][Kp], slice histograms
// [Qc][splits][Kp]
struct RsWs {
  float* ksim;
  int* kidx;
  int* jhist;
  int* part;
};

__host__ __device__ inline RsWs rs_ws(int* ws, int64_t Qc, int Kp) {
  const int64_t n = Qc * Kp;
  return {reinterpret_cast<float*>(ws), ws + n, ws + 2 * n, ws + 3 * n};
}

__global__ __launch_bounds__(RS_BLOCK) void rank_keys_kernel(
    const float* __restrict__ sims, const int* __restrict__ perm,
    const int* __restrict__ segs, const int* __restrict__ neg,
    const int* __restrict__ qcam, const int* __restrict__ gcam, int* ws,
    int* __restrict__ n_good, int64_t Qc, int64_t G, int Kp) {
  extern __shared__ int rs_lds[];
  float* ks = reinterpret_cast<float*>(rs_lds);
  int* ki = rs_lds + Kp;
  int* jh = rs_lds + 2 * Kp;
  __shared__ int s_n;

  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const float* row = sims + q * G;
  const int lo = segs[2 * q];
  // the wrapper sizes Kp from the largest segment; the clamp only keeps a
  // wrong table from writing past the key arrays
  const int n_same = min(segs[2 * q + 1] - lo, Kp);
  const bool cams = qcam != nullptr;
  const int cam = cams ? qcam[q] : 0;

  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int i = tid; i < n_same; i += RS_BLOCK) {
    const int j = perm[lo + i];
    if (!cams || gcam[j] != cam) {
      const int at = atomicAdd(&s_n, 1);   // any order: the sort follows
      ks[at] = row[j];
      ki[at] = j;
    }
  }
  __syncthreads();
  const int n = s_n;
  if (tid == 0) n_good[q] = n;
  if (n == 0) return;

  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  for (int i = n + tid; i < n2; i += RS_BLOCK) {
    ks[i] = -INFINITY;
    ki[i] = -1;
  }
  for (int i = tid; i < n; i += RS_BLOCK) jh[i] = 0;
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int d = k >> 1; d > 0; d >>= 1) {
      for (int i = tid; i < n2; i += RS_BLOCK) {
        const int l = i ^ d;
        if (l > i) {
          const float si = ks[i], sl = ks[l];
          const int ji = ki[i], jl = ki[l];
          const bool swap = (i & k) == 0 ? ahead(sl, jl, si, ji)
                                         : ahead(si, ji, sl, jl);
          if (swap) {
            ks[i] = sl; ki[i] = jl;
            ks[l] = si; ki[l] = ji;
          }
        }
      }
      __syncthreads();
    }
  }

  const RsWs w = rs_ws(ws, Qc, Kp);
  for (int i = tid; i < n; i += RS_BLOCK) {
    w.ksim[q * Kp + i] = ks[i];
    w.kidx[q * Kp + i] = ki[i];
  }
  if (cams) {
    const int neg_lo = neg[0], neg_hi = neg[1];
    for (int i = neg_lo + tid; i < neg_hi; i += RS_BLOCK) {
      const int j = perm[i];
      const int b = keys_ahead(ks, ki, n, row[j], j);
      if (b < n) atomicAdd(&jh[b], 1);
    }
    for (int i = tid; i < n_same; i += RS_BLOCK) {
      const int j = perm[lo + i];
      if (gcam[j] == cam) {
        const int b = keys_ahead(ks, ki, n, row[j], j);
        if (b < n) atomicAdd(&jh[b], 1);
      }
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += RS_BLOCK) w.jhist[q * Kp + i] = jh[i];
}

__global__ __launch_bounds__(RS_BLOCK) void rank_count_kernel(
    const float* __restrict__ sims, int* ws, const int* __restrict__ n_good,
    int64_t Qc, int64_t G, int Kp, int splits) {
  extern __shared__ int rs_lds[];
  float* ks = reinterpret_cast<float*>(rs_lds);
  int* ki = rs_lds + Kp;
  int* hist = rs_lds + 2 * Kp;

  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x / splits;
  const int split = blockIdx.x % splits;
  const int n = n_good[q];
  if (n == 0) return;

  const RsWs w = rs_ws(ws, Qc, Kp);
  for (int i = tid; i < n; i += RS_BLOCK) {
    ks[i] = w.ksim[q * Kp + i];
    ki[i] = w.kidx[q * Kp + i];
    hist[i] = 0;
  }
  __syncthreads();
  const float weak_s = ks[n - 1];
  const int weak_j = ki[n - 1];

  auto count = [&](float s, int j) {
    if (ahead(weak_s, weak_j, s, j)) return;
    atomicAdd(&hist[keys_ahead(ks, ki, n, s, j)], 1);
  };

  const float* row = sims + q * G;
  const int slice = (int)((G + splits - 1) / splits);
  const int c0 = (int)min((int64_t)split * slice, G);
  const int c1 = (int)min((int64_t)c0 + slice, G);
  // floats up to the next 16-byte boundary of the address
  const int mis = (int)((reinterpret_cast<uintptr_t>(row + c0) & 15) >> 2);
  const int head = min((4 - mis) & 3, c1 - c0);
  if (tid < head) count(row[c0 + tid], c0 + tid);
  const int b0 = c0 + head;
  const int nvec = (c1 - b0) >> 2;
  const float4* body = reinterpret_cast<const float4*>(row + b0);
  int i = tid;
  for (; i + 3 * RS_BLOCK < nvec; i += 4 * RS_BLOCK) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = body[i + u * RS_BLOCK];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = b0 + 4 * (i + u * RS_BLOCK);
      count(v[u].x, j);
      count(v[u].y, j + 1);
      count(v[u].z, j + 2);
      count(v[u].w, j + 3);
    }
  }
  for (; i < nvec; i += RS_BLOCK) {
    const float4 v = body[i];
    const int j = b0 + 4 * i;
    count(v.x, j);
    count(v.y, j + 1);
    count(v.z, j + 2);
    count(v.w, j + 3);
  }
  const int t0 = b0 + 4 * nvec;
  if (tid < c1 - t0) count(row[t0 + tid], t0 + tid);
  __syncthreads();

  int* out = w.part + (q * splits + split) * Kp;
  for (int p = tid; p < n; p += RS_BLOCK) out[p] = hist[p];
}

__global__ __launch_bounds__(RS_BLOCK) void rank_finish_kernel(
    const int* ws, const int* __restrict__ n_good, int* __restrict__ first_rank,
    double* __restrict__ ap, int64_t Qc, int Kp, int splits) {
  extern __shared__ int rs_lds[];
  int* net = rs_lds;                 // [Kp]
  __shared__ int s_sum[RS_BLOCK];
  __shared__ double s_ap[RS_BLOCK / kWave];

  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x;
  const int n = n_good[q];
  if (n == 0) {
    if (tid == 0) {
      first_rank[q] = -1;
      ap[q] = 0.0;
    }
    return;
  }
  const RsWs w = rs_ws(const_cast<int*>(ws), Qc, Kp);
  for (int p = tid; p < n; p += RS_BLOCK) {
    int v = -w.jhist[q * Kp + p];
    for (int s = 0; s < splits; ++s) v += w.part[(q * splits + s) * Kp + p];
    net[p] = v;
  }
  __syncthreads();

  // thread t owns positions [t·per, (t+1)·per): its total, a scan of the
  // totals, then its own prefix walk
  const int per = (n + RS_BLOCK - 1) / RS_BLOCK;
  const int p0 = min(tid * per, n), p1 = min(p0 + per, n);
  int total = 0;
  for (int p = p0; p < p1; ++p) total += net[p];
  s_sum[tid] = total;
  __syncthreads();
  for (int d = 1; d < RS_BLOCK; d <<= 1) {
    const int add = tid >= d ? s_sum[tid - d] : 0;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  int prefix = s_sum[tid] - total;
  double acc = 0.0;
  for (int p = p0; p < p1; ++p) {
    prefix += net[p];
    const int r = prefix - 1;
    if (p == 0) first_rank[q] = r;
    const double precision = (p + 1.0) / (r + 1.0);
    const double old_precision = r > 0 ? (double)p / (double)r : 1.0;
    acc += (precision + old_precision) * 0.5;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & (kWave - 1)) == 0) s_ap[tid / kWave] = acc;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int wv = 0; wv < RS_BLOCK / kWave; ++wv) sum += s_ap[wv];
    ap[q] = sum / (double)n;
  }
}

}  // namespace

extern "C" int flreid_rank_stats_max_good() { return RS_MAX_GOOD; }

extern "C" int64_t flreid_rank_stats_ws_ints(int64_t Qc, int64_t G, int kmax) {
  if (Qc < 1 || G < 1 || kmax < 0 || kmax > RS_MAX_GOOD)
    throw std::invalid_argument(
        "rank_stats: needs Qc >= 1, G >= 1, kmax in [0, " +
        std::to_string(RS_MAX_GOOD) + "]");
  return Qc * rs_pad(kmax) * (3 + rs_splits(Qc, G));
}

extern "C" void flreid_rank_stats(const float* sims, const int* perm,
                                  const int* segs, const int* neg,
                                  const int* qcam, const int* gcam, int* ws,
                                  int* first_rank, int* n_good, double* ap,
                                  int64_t Qc, int64_t G, int kmax,
                                  hipStream_t stream) {
  if (Qc < 1 || G < 1 || G > INT32_MAX - 4 || Qc > INT32_MAX / RS_TARGET_WGS
      || kmax < 0 || kmax > RS_MAX_GOOD)
    throw std::invalid_argument(
        "rank_stats: needs Qc >= 1, 1 <= G < 2^31, kmax in [0, " +
        std::to_string(RS_MAX_GOOD) + "]");
  if (sims == nullptr || perm == nullptr || segs == nullptr || neg == nullptr
      || ws == nullptr || first_rank == nullptr || n_good == nullptr
      || ap == nullptr || (qcam == nullptr) != (gcam == nullptr))
    throw std::invalid_argument(
        "rank_stats: null pointer, or one camera array without the other");
  const int Kp = rs_pad(kmax);
  const int splits = rs_splits(Qc, G);
  const size_t lds = (size_t)Kp * 3 * sizeof(int);
  hipLaunchKernelGGL(rank_keys_kernel, dim3((unsigned)Qc), dim3(RS_BLOCK), lds,
                     stream, sims, perm, segs, neg, qcam, gcam, ws, n_good, Qc,
                     G, Kp);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)(Qc * splits)),
                     dim3(RS_BLOCK), lds, stream, sims, ws,
                     (const int*)n_good, Qc, G, Kp, splits);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(rank_finish_kernel, dim3((unsigned)Qc), dim3(RS_BLOCK),
                     (size_t)Kp * sizeof(int), stream, (const int*)ws,
                     (const int*)n_good, first_rank, ap, Qc, Kp, splits);
  HIP_CHECK(hipGetLastError());
}

}  // namespace flreid

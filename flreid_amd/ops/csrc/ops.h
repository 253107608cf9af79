// The extension's C interface: the single declaration of every launcher and
// helper the python bindings (module.cpp) call.
//
// Every .hip that defines one of these includes this header, so a definition
// whose parameter list drifts from its declaration is a compile error (two
// extern "C" functions of one name cannot differ in their parameters) instead
// of scrambled arguments at run time.  Pointers are device pointers unless
// noted; `dtype` arguments are the DType tags of common.h; every launcher
// enqueues on `stream` and returns.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace flreid {

// int64 fields per head_step table row: aw, aw0, dw, gw, atten, m, v, theta,
// step (device addresses), numel, L, inner, flags, partial0
constexpr int kHeadStepFields = 14;

extern "C" {

// ---- elementwise.hip ------------------------------------------------------
void flreid_l2norm_rows(const void* x, void* y, int64_t rows, int64_t cols,
                        int dtype, float eps, hipStream_t stream);
void flreid_ce_smooth(const void* score, const int64_t* target,
                      float* row_loss, void* grad, int64_t B, int64_t C,
                      int dtype, float eps, hipStream_t stream);
// atten / aw may be null (no scaling / no addend)
void flreid_compose2(const void* gw, const float* atten, const void* aw,
                     void* out, int64_t numel, int64_t L, int64_t inner,
                     int in_dtype, int out_dtype, hipStream_t stream);
// sq: 1 accumulates scale·g², 0 accumulates scale·|g|
void flreid_importance(float* F, const void* g, int64_t numel, int dtype,
                       int sq, float scale, hipStream_t stream);
void flreid_bn_eval(const void* x, void* y, const float* gamma,
                    const float* beta, const float* mean, const float* var,
                    int64_t numel, int C, int64_t HW, float eps, int nhwc,
                    int relu, int dtype, hipStream_t stream);
// bn_eval with an optional residual (x's shape, layout and dtype; null for
// none): y = relu(bn(x) + res), the BN output rounded to the tensor dtype
// before the add; a residual implies the ReLU.  wide != 0 lets NHWC input
// with C % 8 == 0 and 16-byte-aligned pointers take the 16-byte kernel (same
// bits); wide == 0 keeps the one-element-per-thread kernel.  bn_eval itself
// is this with no residual and wide = 1.
void flreid_bn_eval_res(const void* x, const void* res, void* y,
                        const float* gamma, const float* beta,
                        const float* mean, const float* var, int64_t numel,
                        int C, int64_t HW, float eps, int nhwc, int relu,
                        int wide, int dtype, hipStream_t stream);

// ---- distance.hip ---------------------------------------------------------
void flreid_pairwise(const float* A, const float* B, const float* aa,
                     const float* bb, float* out, int64_t M, int64_t N,
                     int64_t D, int mode, hipStream_t stream);
void flreid_rowsq(const float* x, float* out, int64_t rows, int64_t cols,
                  hipStream_t stream);

// ---- window_attn.hip ------------------------------------------------------
void flreid_window_attn_fwd(const void* q, const void* k, const void* v,
                            const float* bias, const float* mask, void* out,
                            int64_t BW, int H, int N, int D, int nW,
                            float scale, int dtype, hipStream_t stream);
void flreid_window_attn_bwd(const void* q, const void* k, const void* v,
                            const float* bias, const float* mask,
                            const void* dout, void* dq, void* dk, void* dv,
                            float* ds, int64_t BW, int H, int N, int D, int nW,
                            float scale, int dtype, hipStream_t stream);

// ---- window_attn_mfma.hip -------------------------------------------------
// bf16 only, D == 32, 64 < N <= 144; every pointer 16-byte aligned.
// host helper: windows per backward workgroup; dbias_part is
// [ceil(BW / group)][H][N][N] fp32, summed over its first axis by the caller
int flreid_window_attn_mfma_group();
void flreid_window_attn_mfma_fwd(const void* q, const void* k, const void* v,
                                 const float* bias, const float* mask,
                                 void* out, int64_t BW, int H, int N, int D,
                                 int nW, float scale, hipStream_t stream);
void flreid_window_attn_mfma_bwd(const void* q, const void* k, const void* v,
                                 const float* bias, const float* mask,
                                 const void* dout, void* dq, void* dk,
                                 void* dv, float* dbias_part, int64_t BW,
                                 int H, int N, int D, int nW, float scale,
                                 hipStream_t stream);

// ---- window_attn_qkv.hip --------------------------------------------------
// bf16 only, D == 32, 1 <= N <= 64; every pointer 16-byte aligned.  qkv and
// dqkv are [BW][N][3·H·32] with the last axis ordered (q|k|v, head, d); out
// and dout are [BW][N][H·32].
// host helper: windows per backward workgroup; dbias_part is
// [ceil(BW / group)][H][N][N] fp32, summed over its first axis by the caller
int flreid_window_attn_qkv_group();
void flreid_window_attn_qkv_fwd(const void* qkv, const float* bias,
                                const float* mask, void* out, int64_t BW,
                                int H, int N, int nW, float scale,
                                hipStream_t stream);
void flreid_window_attn_qkv_bwd(const void* qkv, const float* bias,
                                const float* mask, const void* dout,
                                void* dqkv, float* dbias_part, int64_t BW,
                                int H, int N, int nW, float scale,
                                hipStream_t stream);

// ---- window_attn_map.hip --------------------------------------------------
// The same attention on the feature map: bf16 only, D == 32, 1 <= ws <= 8,
// Hi and Wi multiples of ws, 0 <= shift < ws, one image of qkv below 2 GiB;
// every pointer 16-byte aligned.  qkv and dqkv are [B][Hi][Wi][3·H·32] with
// the last axis ordered (q|k|v, head, d); out and dout are [B][Hi][Wi][H·32],
// in image order.  The kernels do roll(-shift), the window partition, its
// reverse and roll(+shift) by addressing, and form the standard shift mask
// (0 / -100 by region label) of this geometry themselves when shift > 0:
// there is no mask tensor.  bias is [H][ws²][ws²] fp32.  dbias_part is
// [ceil(B·nW / flreid_window_attn_qkv_group())][H][ws²][ws²] fp32, nW =
// (Hi / ws)·(Wi / ws), summed over its first axis by the caller.
void flreid_window_attn_map_fwd(const void* qkv, const float* bias, void* out,
                                int B, int Hi, int Wi, int ws, int shift,
                                int H, float scale, hipStream_t stream);
void flreid_window_attn_map_bwd(const void* qkv, const float* bias,
                                const void* dout, void* dqkv,
                                float* dbias_part, int B, int Hi, int Wi,
                                int ws, int shift, int H, float scale,
                                hipStream_t stream);

// ---- triplet.hip ----------------------------------------------------------
void flreid_triplet_fwd(const float* F, const float* norms,
                        const int64_t* labels, float* row_loss, int* p_idx,
                        int* n_idx, int N, int D, float margin,
                        hipStream_t stream);
void flreid_triplet_bwd(const float* F, const float* row_loss,
                        const int* p_idx, const int* n_idx, float* grad, int N,
                        int D, float coeff, hipStream_t stream);

// ---- triplet_gram.hip -----------------------------------------------------
// host helper: the largest batch (rows) the Gram-form triplet loss serves
int flreid_triplet_gram_max_n();
// host helper: K slices of the Gram phase; slabs is [slices][N][N] fp32
int flreid_triplet_gram_slices(int N, int D);
// Triplet loss of fp32 F [N][D] (any D >= 1) and int64 labels [N], metric
// cosine (1) or squared euclidean (0), mining batch-hard (hard = 1) or
// softmax-weighted, row loss log1p(exp(ap - an)) (soft = 1) or a hinge at
// margin > 0.  Outputs: row_loss [N] and C [N][N] = d(sum of row losses) /
// d(distance); with soft = 1 also row_fb / C_fb, the same for the 0.3 hinge
// the soft-margin mode falls back to (else unread, may be null); with
// cosine = 1 also G [N][N] and rinv [N] for the backward (else unread).
// slabs is uninitialised scratch.
void flreid_triplet_gram_fwd(const float* F, const int64_t* labels,
                             float* slabs, float* G, float* rinv, float* C,
                             float* C_fb, float* row_loss, float* row_fb,
                             int N, int D, int cosine, int hard, int soft,
                             float margin, hipStream_t stream);
// dF [N][D] = (*gscale / N)·M·F from the forward's outputs, every element
// written once.  use_fb (one int32 on the device, or null with C_fb null)
// != 0 selects C_fb.  gscale: device pointer to the upstream gradient.
void flreid_triplet_gram_bwd(const float* F, const float* C,
                             const float* C_fb, const int* use_fb,
                             const float* G, const float* rinv,
                             const float* gscale, float* dF, int N, int D,
                             int cosine, hipStream_t stream);

// ---- adaptive_gemm.hip ----------------------------------------------------
void flreid_adaptive_linear_fwd(const void* X, const float* GW,
                                const float* AW, const float* ATTEN,
                                const float* BIAS, void* OUT, int M, int N,
                                int K, int split_layout, hipStream_t stream);
void flreid_theta_linear_fwd(const void* x, const void* theta,
                             const float* bias, void* out, int M, int N, int K,
                             hipStream_t stream);

// ---- conv3x3.hip ----------------------------------------------------------
void flreid_conv3x3_fwd(const void* x, const float* w, void* y, int NB, int H,
                        int Wd, int C, int K, hipStream_t stream);

// ---- conv3x3_img.hip ------------------------------------------------------
void flreid_conv3x3_tile(const void* gw, const float* atten, const void* aw,
                         void* out, int C, int K, int in_dtype, int mode,
                         hipStream_t stream);
void flreid_conv3x3_img_fwd(const void* x, const void* w, void* y, int NB,
                            int H, int Wd, int C, int K, hipStream_t stream);
void flreid_transpose_bf16(const void* in, void* out, int64_t M, int64_t N,
                           hipStream_t stream);
void flreid_conv3x3_wgrad(const void* dy, const void* x, float* dw, int NB,
                          int H, int Wd, int C, int K, hipStream_t stream);

// ---- conv3x3_img_ldsw.hip -------------------------------------------------
void flreid_conv3x3_img_fwd_ldsw(const void* x, const void* w, void* y, int NB,
                                 int H, int Wd, int C, int K,
                                 hipStream_t stream);

// ---- bn_train.hip ---------------------------------------------------------
// host helper: row slabs of the reduction; part_a / part_b are [nslab][C]
int flreid_bn_train_nslab(int64_t M, int C);
void flreid_bn_train_fwd(const void* x, void* y, const float* gamma,
                         const float* beta, float* rmean, float* rvar,
                         float* smean, float* sinv, float* part_a,
                         float* part_b, unsigned long long* nbt, int64_t M,
                         int C, float momentum, float eps, float unbiased,
                         int relu, int dtype, hipStream_t stream);
void flreid_bn_train_bwd(const void* x, const void* dy, void* dx,
                         const float* gamma, const float* beta,
                         const float* smean, const float* sinv, float* dgamma,
                         float* dbeta, float* part_a, float* part_b, int64_t M,
                         int C, int relu, int dtype, hipStream_t stream);

// ---- bn_onepass.hip -------------------------------------------------------
// host helper: ≥ 0 when (M, C) is inside the one-launch regime, −1 when the
// shape stays on the two-launch pair above
int flreid_bn_onepass_config(int64_t M, int C);
// bf16 only; same outputs, bit for bit, as flreid_bn_train_fwd / _bwd, with
// no workspace.  variant < 0 takes the launcher's per-shape tile; otherwise
// low byte = instantiation, bit 8 = plain block order (benchmark only).
// Throws when the shape (or the variant) does not fit.
void flreid_bn_onepass_fwd(const void* x, void* y, const float* gamma,
                           const float* beta, float* rmean, float* rvar,
                           float* smean, float* sinv, unsigned long long* nbt,
                           int64_t M, int C, float momentum, float eps,
                           float unbiased, int relu, int variant,
                           hipStream_t stream);
void flreid_bn_onepass_bwd(const void* x, const void* dy, void* dx,
                           const float* gamma, const float* beta,
                           const float* smean, const float* sinv,
                           float* dgamma, float* dbeta, int64_t M, int C,
                           int relu, int variant, hipStream_t stream);
// The same with the residual epilogue, y = relu(bf16(bn(x)) + res): res and z
// (the saved y) have x's shape and layout.  Backward masks dz where z <= 0,
// writes the masked value to dres (the residual's gradient; may be null) and
// runs the plain backward on it.  The BN's own ReLU does not combine.
void flreid_bn_onepass_res_fwd(const void* x, const void* res, void* y,
                               const float* gamma, const float* beta,
                               float* rmean, float* rvar, float* smean,
                               float* sinv, unsigned long long* nbt, int64_t M,
                               int C, float momentum, float eps,
                               float unbiased, int variant,
                               hipStream_t stream);
void flreid_bn_onepass_res_bwd(const void* x, const void* dz, const void* z,
                               void* dres, void* dx, const float* gamma,
                               const float* beta, const float* smean,
                               const float* sinv, float* dgamma, float* dbeta,
                               int64_t M, int C, int variant,
                               hipStream_t stream);

// ---- drift.hip ------------------------------------------------------------
// ptrs: [n][2] int64 (p, anchor); chunks: [n_chunks][4] int32
// (tensor, elem_offset, len, flat_offset); partials: one float per chunk
void flreid_drift_fwd(const int64_t* ptrs, const int* chunks, float* partials,
                      int n_chunks, hipStream_t stream);
// gscale: device pointer to the upstream gradient (one float)
void flreid_drift_bwd(const int64_t* ptrs, const int* chunks,
                      const float* gscale, float* flat_grad, int n_chunks,
                      hipStream_t stream);

// ---- kd.hip ---------------------------------------------------------------
void flreid_kd_fwd(const float* zs, const float* zt, float* row_loss,
                   float* grad, int64_t B, int64_t C, float temperature,
                   hipStream_t stream);
void flreid_icarl_distill(const float* score, const int64_t* target,
                          const float* prev, float* row_loss, float* grad,
                          int64_t B, int64_t C, int64_t P, hipStream_t stream);

// ---- patch_merge.hip ------------------------------------------------------
void flreid_patch_merge_ln_fwd(const void* x, const float* gamma,
                               const float* beta, void* y, float* mean,
                               float* rstd, int64_t rows, int C, int H, int W,
                               float eps, int dtype, hipStream_t stream);
void flreid_patch_merge_ln_bwd(const void* x, const float* gamma,
                               const void* dy, const float* mean,
                               const float* rstd, void* dx, float* dg,
                               float* db, int64_t rows, int C, int H, int W,
                               int dtype, hipStream_t stream);

// ---- add_ln.hip -----------------------------------------------------------
// Residual add + LayerNorm over rows × C contiguous rows, C % 8 == 0,
// 8 <= C <= 1536, every pointer 16-byte aligned; dtype tags are kF32 / kBF16.
// host helper: blocks either launch uses for (rows, C), at most 1024 (0 out
// of regime); dg_part / db_part are [blocks][C] fp32
int flreid_add_ln_blocks(int64_t rows, int C);
// s = a + b rounded to a_dtype and stored (b null: s is a, nothing stored);
// y = LN(s)·gamma + beta in y_dtype, statistics of the stored s in fp32, the
// variance from centred values; mean / rstd [rows] may both be null.
void flreid_add_ln_fwd(const void* a, const void* b, const float* gamma,
                       const float* beta, void* s, void* y, float* mean,
                       float* rstd, int64_t rows, int C, float eps,
                       int a_dtype, int b_dtype, int y_dtype,
                       hipStream_t stream);
// ds = ds_in + LNbwd(dy) in a_dtype; dy (y_dtype) or ds_in (a_dtype) may be
// null, ds_b (may be null) receives the same values in b_dtype.  affine != 0:
// one dgamma / dbeta partial per block, no atomics, summed by the caller;
// affine == 0 leaves dg_part / db_part (may be null) alone.
void flreid_add_ln_bwd(const void* s, const float* gamma, const float* mean,
                       const float* rstd, const void* dy, const void* ds_in,
                       void* ds, void* ds_b, float* dg_part, float* db_part,
                       int64_t rows, int C, int a_dtype, int b_dtype,
                       int y_dtype, int affine, hipStream_t stream);

// ---- decomposed.hip -------------------------------------------------------
// host helper; out-parameters (tasks_per_row, blocks): dmask_part is
// [rows][tasks_per_row], datten_part is [blocks][KB]
void flreid_decomposed_plan(int64_t rows, int64_t C, int64_t S,
                            int channels_last, int64_t* tasks_per_row,
                            int64_t* blocks);
void flreid_decomposed_fwd(const float* sw, const float* mask, const float* aw,
                           const float* aw_kb, const float* atten, void* out,
                           int64_t rows, int64_t C, int64_t S, int64_t KB,
                           int channels_last, int train, float lambda_l1,
                           float lambda_mask, int out_dtype,
                           hipStream_t stream);
void flreid_decomposed_bwd(const void* g, int g_dtype, const float* sw,
                           const float* mask, const float* aw,
                           const float* aw_kb, float* d_aw, float* dmask_part,
                           float* datten_part, int64_t rows, int64_t C,
                           int64_t S, int64_t KB, int channels_last, int train,
                           float lambda_l1, float lambda_mask, int need_aw,
                           int need_mask, int need_atten, hipStream_t stream);

// ---- head_step.hip --------------------------------------------------------
int flreid_head_step_chunk();
// rows: HOST pointer to n_rows × kHeadStepFields int64; the table is
// validated in full before anything is launched
void flreid_head_step(const int64_t* rows, int n_rows, double* partials,
                      int64_t n_partials, double lr, double beta1,
                      double beta2, double weight_decay, double eps,
                      float lambda, hipStream_t stream);

// ---- penalty.hip ----------------------------------------------------------
int flreid_penalty_chunk();
int flreid_penalty_block();
// ptrs: [n][1 + 2·S] int64 (p, then anchor / importance per set, 0 = absent)
void flreid_penalty_fwd(const int64_t* ptrs, const int* chunks, int S,
                        float* partials, int n_chunks, hipStream_t stream);
// gscale: device pointer to the upstream gradient (one float)
void flreid_penalty_bwd(const int64_t* ptrs, const int* chunks, int S,
                        const float* gscale, float* flat_grad, int n_chunks,
                        hipStream_t stream);

// ---- herding.hip ----------------------------------------------------------
// host helper: the largest identity (rows) whose Gram matrix stays in LDS
int flreid_herding_lds_max();
// Herding exemplar selection, m picks per identity.  feats is [N][D] fp32,
// 16-byte aligned, D % 4 == 0; order is [N] int32, the rows sorted by
// identity (stable); offsets is [P + 1] int32 into order; sel is [P][m] int32
// and receives original row indices.  Identities have 1..1024 rows.  n_lds is
// the largest identity of at most flreid_herding_lds_max() rows (0: none).
// Larger identities need gram_ws (n² floats each, at ws_offsets[p] floats;
// [P] int32, unread for the others) and tiles, n_tiles int32 rows of (offset
// into order, n, tile row, tile col, ws offset): every 64×64 tile with tile
// row <= tile col of every such identity.  All tables are device memory.
void flreid_herding_select(const float* feats, const int* order,
                           const int* offsets, int* sel, float* gram_ws,
                           const int* ws_offsets, const int* tiles,
                           int n_tiles, int n_lds, int P, int D, int m,
                           hipStream_t stream);

// ---- rank_stats.hip -------------------------------------------------------
// host helper: the most good entries (same-id group size) one query may have
int flreid_rank_stats_max_good();
// host helper: int32 elements of workspace a [Qc, G] tile needs when no
// query's same-id segment exceeds kmax
int64_t flreid_rank_stats_ws_ints(int64_t Qc, int64_t G, int kmax);
// CMC / AP rank statistics of sims [Qc][G] fp32 (contiguous, any 4-byte
// alignment), without sorting the rows.  perm is [G] int32, the gallery
// sorted by label; segs is [Qc][2] int32, each query's same-id segment
// [lo, hi) of perm, at most kmax long; neg is [2] int32, the segment of the
// label −1.  qcam [Qc] / gcam [G] int32 are both given (camera mode: same-id
// same-camera entries and the −1 segment are junk) or both null (nothing is
// junk, neg unread).  Outputs per row: first_rank, the junk-free 0-based rank
// of the first good hit (−1 without one), n_good and ap.  ws is uninitialised
// scratch of flreid_rank_stats_ws_ints(Qc, G, kmax) int32.
void flreid_rank_stats(const float* sims, const int* perm, const int* segs,
                       const int* neg, const int* qcam, const int* gcam,
                       int* ws, int* first_rank, int* n_good, double* ap,
                       int64_t Qc, int64_t G, int kmax, hipStream_t stream);

}  // extern "C"

}  // namespace flreid

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

// ---- triplet.hip ----------------------------------------------------------
void flreid_triplet_fwd(const float* F, const float* norms,
                        const int64_t* labels, float* row_loss, int* p_idx,
                        int* n_idx, int N, int D, float margin,
                        hipStream_t stream);
void flreid_triplet_bwd(const float* F, const float* row_loss,
                        const int* p_idx, const int* n_idx, float* grad, int N,
                        int D, float coeff, hipStream_t stream);

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

}  // extern "C"

}  // namespace flreid

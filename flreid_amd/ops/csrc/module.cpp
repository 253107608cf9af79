// Python bindings for the flreid MI355X kernels.
//
// Deliberately torch-header-free: tensors cross as raw device pointers plus
// the caller's torch HIP stream (uintptr_t), so the extension compiles with
// plain hipcc for gfx950 — no hipify, no CUDA-compat layer — and launches
// stay ordered with PyTorch work on the same stream.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ops.h"

namespace py = pybind11;
using namespace flreid;

// binder<&fn>::call is fn with every pointer parameter (hipStream_t is one)
// taken as uintptr_t: the binding is generated from the launcher's own type,
// so its parameter list cannot drift from the declaration in ops.h.
template <typename T> struct py_arg {
  using type = T;
  static T to(T v) { return v; }
};
template <typename T> struct py_arg<T*> {
  using type = uintptr_t;
  static T* to(uintptr_t v) { return reinterpret_cast<T*>(v); }
};
template <auto Fn> struct binder;
template <typename R, typename... A, R (*Fn)(A...)> struct binder<Fn> {
  static R call(typename py_arg<A>::type... a) {
    return Fn(py_arg<A>::to(a)...);
  }
};

#define FLREID_DEF(name) m.def(#name, &binder<&flreid_##name>::call)

PYBIND11_MODULE(_flreid_hip, m) {
  m.doc() = "flreid MI355X (gfx950) kernels";

  FLREID_DEF(l2norm_rows);
  FLREID_DEF(ce_smooth);
  FLREID_DEF(compose2);
  FLREID_DEF(bn_eval);
  FLREID_DEF(pairwise);
  FLREID_DEF(rowsq);
  FLREID_DEF(window_attn_fwd);
  FLREID_DEF(window_attn_bwd);
  FLREID_DEF(triplet_fwd);
  FLREID_DEF(triplet_bwd);
  FLREID_DEF(adaptive_linear_fwd);
  FLREID_DEF(theta_linear_fwd);
  FLREID_DEF(conv3x3_fwd);
  FLREID_DEF(conv3x3_tile);
  FLREID_DEF(conv3x3_img_fwd);
  FLREID_DEF(conv3x3_img_fwd_ldsw);
  FLREID_DEF(conv3x3_wgrad);
  FLREID_DEF(transpose_bf16);
  FLREID_DEF(bn_train_nslab);
  FLREID_DEF(bn_train_fwd);
  FLREID_DEF(bn_train_bwd);
  FLREID_DEF(drift_fwd);
  FLREID_DEF(drift_bwd);
  FLREID_DEF(kd_fwd);
  FLREID_DEF(icarl_distill);
  FLREID_DEF(patch_merge_ln_fwd);
  FLREID_DEF(patch_merge_ln_bwd);
  FLREID_DEF(decomposed_fwd);
  FLREID_DEF(decomposed_bwd);
  FLREID_DEF(head_step_chunk);
  FLREID_DEF(penalty_chunk);
  FLREID_DEF(penalty_block);
  FLREID_DEF(penalty_fwd);
  FLREID_DEF(penalty_bwd);

  // The three bindings whose Python signature differs from the C one.

  // sq crosses as a Python bool
  m.def("importance",
        [](uintptr_t F, uintptr_t g, int64_t numel, int dtype, bool sq,
           float scale, uintptr_t stream) {
          flreid_importance((float*)F, (const void*)g, numel, dtype,
                            sq ? 1 : 0, scale, (hipStream_t)stream);
        });

  // (tasks_per_row, blocks): dmask_part is [rows][tasks_per_row],
  // datten_part is [blocks][KB]
  m.def("decomposed_plan",
        [](int64_t rows, int64_t C, int64_t S, int channels_last) {
          int64_t tpr = 0, blocks = 0;
          flreid_decomposed_plan(rows, C, S, channels_last, &tpr, &blocks);
          return py::make_tuple(tpr, blocks);
        });

  // rows: one kHeadStepFields-int64 row per adaptive weight (see
  // head_step.hip); the table is validated in full before anything is
  // launched
  m.def("head_step",
        [](const std::vector<std::vector<int64_t>>& rows, uintptr_t partials,
           int64_t n_partials, double lr, double beta1, double beta2,
           double weight_decay, double eps, float lambda, uintptr_t stream) {
          std::vector<int64_t> flat;
          flat.reserve(rows.size() * kHeadStepFields);
          for (const auto& r : rows) {
            if (r.size() != kHeadStepFields)
              throw std::invalid_argument(
                  "head_step: rows need " + std::to_string(kHeadStepFields) +
                  " fields");
            flat.insert(flat.end(), r.begin(), r.end());
          }
          flreid_head_step(flat.data(), (int)rows.size(), (double*)partials,
                           n_partials, lr, beta1, beta2, weight_decay, eps,
                           lambda, (hipStream_t)stream);
        });
}

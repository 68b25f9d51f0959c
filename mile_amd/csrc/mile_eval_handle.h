// Everything the evaluation layer (mile_eval.hip) may ask of a sampler handle.  mile_hip.hip implements it and stays the only
// file that defines struct mile_sampler: the statistics see neither the slabs, the NUTS buffers nor the gradient kernels.
// No kernel header is included here, and none may be.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/mile_hip.h"

#define MILE_LOCAL __attribute__((visibility("hidden")))   // shared by the library's translation units, not exported

// The one error path: the message mile_last_error returns (thread-local), and `code` back.
MILE_LOCAL int fail(int code, const std::string &msg);
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return fail(MILE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));           \
  } while (0)

// The FCN's parameter row without a handle: bias and kernel offset of each of spec->n_layers layers (in_features >= 1, widths
// >= 1 and 1 <= n_layers <= MILE_MAX_LAYERS are the caller's to check), d back.  The table behind mile_param_offsets.
struct FcnOffsets { int32_t *b_off, *w_off; };       // [n_layers] each, the caller's
MILE_LOCAL long long fcn_param_layout(const mile_model_spec *spec, FcnOffsets ds);

// what the statistics read of a handle: its device and compute units, the task, the row width F, the head width O, d
struct EvalView { int device, n_cu, task, in_features, O, d; };
MILE_LOCAL EvalView eval_view(const mile_sampler *s);
// the handle's model, for the statistic that runs its own kernel on the FCN's layers (mile_predict_sensitivities)
MILE_LOCAL const mile_model_spec *eval_spec(const mile_sampler *s);

// every call that evaluates the likelihood refuses a pretrained-attention sampler whose tables are not set
MILE_LOCAL bool tables_missing(const mile_sampler *s);
MILE_LOCAL extern const char *const kNoTables;

// Stage N evaluation rows (and, y not null, their labels) in the handle.  The handle holds one staged set: staging replaces it.
MILE_LOCAL int stage_rows(mile_sampler *s, const float *X, const void *y, int64_t N, hipStream_t st);
// The one forward of evaluation: the resolved kernel's `loglik` of S samples (rows of theta) on the staged rows, into
// out [S, N] -- or, staged without labels, the raw outputs [S, N, O]: eval_per_sample floats of out per sample.
MILE_LOCAL size_t eval_per_sample(const mile_sampler *s);
MILE_LOCAL int eval_forward(mile_sampler *s, const float *theta, int64_t S, float *out, hipStream_t st);

// The streamed calls' workspace of at least `bytes`, or null.  The sweeps of the last mile_predict_quantiles lie in it: whoever
// reserves it forgets them.
MILE_LOCAL void *reserve_eval_ws(mile_sampler *s, size_t bytes);
// the sweeps per row that mile_predict_quantiles recorded in the workspace, for mile_debug_quantile_sweeps (rows 0: none)
MILE_LOCAL void record_quantile_sweeps(mile_sampler *s, const int32_t *sweeps, int64_t rows);
MILE_LOCAL int64_t recorded_quantile_sweeps(const mile_sampler *s, const int32_t **sweeps);

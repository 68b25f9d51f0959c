// libmile_hip.so -- the evaluation layer of the C ABI declared in include/mile_hip.h: the host drivers of the likelihood and
// prediction calls and of every statistic of the ensemble (argument checks, tile plans, tile loops).  The statistics' kernels
// are in their own translation units behind the launchers of their headers; the forward is the sampler's, reached through
// mile_eval_handle.h and nothing else of the handle.  No kernel is defined or launched from this file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mile_hip.h"
#include "mile_eval_handle.h"
#include "mile_eval_plan.h"
#include "mile_moments.h"
#include "mile_lppd.h"
#include "mile_quantiles.h"
#include "mile_loo.h"
#include "mile_lxp.h"
#include "mile_stack.h"
#include "mile_calib.h"
#include "mile_crps.h"
#include "mile_diag.h"
#include "mile_fdiag.h"
#include "mile_dtail.h"
#include "mile_sens.h"
#include "mile_pdp.h"

// D consecutive draws in passes of `chunk`, each pass at its draw offset of out [D][per sample]: every (draw, row) forward once
static int forward_draws(mile_sampler *s, const float *theta, int64_t D, int64_t chunk, float *out, hipStream_t st) {
  const size_t d = eval_view(s).d;
  for (int64_t s0 = 0; s0 < D; s0 += chunk) {
    const int rc = eval_forward(s, theta + (size_t)s0 * d, std::min<int64_t>(chunk, D - s0), out + (size_t)s0 * eval_per_sample(s), st);
    if (rc != MILE_OK) return rc;
  }
  return MILE_OK;
}
// draws j0 .. j0 + J of each of C chains of S draws (chain c's are rows c * S + j0 .. of theta) into out [C][J][per sample]
static int forward_chains(mile_sampler *s, const float *theta, int C, int64_t S, int64_t j0, int J, float *out, hipStream_t st) {
  const size_t d = eval_view(s).d;
  for (int c = 0; c < C; ++c) {
    const int rc = eval_forward(s, theta + ((size_t)c * S + (size_t)j0) * d, J, out + (size_t)c * J * eval_per_sample(s), st);
    if (rc != MILE_OK) return rc;
  }
  return MILE_OK;
}

// mile_pointwise_loglik and (y == nullptr) mile_predict: stage the evaluation rows, then the forward
static int evaluate_rows(mile_sampler *s, const float *theta, int32_t S, const float *X, const void *y, int64_t N, float *out, void *stream) {
  hipStream_t st = (hipStream_t)stream;
  const int rc = stage_rows(s, X, y, N, st);
  return rc != MILE_OK ? rc : eval_forward(s, theta, S, out, st);
}

// The checks that the evaluation calls share, each a message or null: the range of N, the generic shape of a call (S, then
// N), the signs of the caller's pass and tile caps, the model of the statistics of a Gaussian predictive.
static const char *bad_N(int64_t N) { return N < 1 || N > 0x3fffffff ? "N out of range (1 .. 2^30 - 1)" : nullptr; }
static const char *bad_SN(int64_t S, int64_t N) { return S < 1 || S > 0x7fffffff ? "S out of range (1 .. 2^31 - 1)" : bad_N(N); }
static const char *bad_caps(int64_t max_draws_per_pass, int64_t max_rows_per_tile) {
  if (max_draws_per_pass < 0) return "max_draws_per_pass < 0";
  return max_rows_per_tile < 0 ? "max_rows_per_tile < 0" : nullptr;
}
static const char *not_mu_log_sigma(const mile_sampler *s) {
  return eval_view(s).task != MILE_TASK_REGRESSION || eval_view(s).O != 2 ? "needs a regression model with (mu, log sigma) outputs" : nullptr;
}
// the refusal of an argument of `fn`: MILE_ERR_INVALID with "fn: m"
static int bad(const char *fn, const char *m) { return fail(MILE_ERR_INVALID, std::string(fn) + ": " + m); }

// What every evaluation entry point `fn` on a handle checks before anything else, in this order: null arguments, the shape
// (`shape`: the statistic's own message or null, bad_SN for most), the call's other checks (`more`: a message or null; it may
// read the handle), then the frozen tables.  MILE_OK, or the failure with its message set.
template <class More>
static int eval_args(const char *fn, const mile_sampler *s, bool null_arg, const char *shape, More more) {
  if (!s || null_arg) return bad(fn, "null argument");
  if (shape) return bad(fn, shape);
  if (const char *m = more()) return bad(fn, m);
  if (tables_missing(s)) return fail(MILE_ERR_STATE, kNoTables);
  return MILE_OK;
}
static const char *no_more_checks() { return nullptr; }

// What every streamed call `fn` does once its checks have passed and its plan stands: the handle's device, then the handle's
// workspace of the plan's `bytes` in ws.  No memory is MILE_ERR_NOMEM with "fn: workspace allocation failed (hint)".
static int stream_ws(const char *fn, mile_sampler *s, size_t bytes, const char *hint, char *&ws) {
  HIP_TRY(hipSetDevice(eval_view(s).device));
  ws = (char *)reserve_eval_ws(s, bytes);
  return ws ? MILE_OK : fail(MILE_ERR_NOMEM, std::string(fn) + ": workspace allocation failed (" + hint + ")");
}

// The tensor-input calls' workspace of `bytes` (0: none), this call's own: `run` gets it, and the stream is drained before it is
// freed, whatever run returned.  run's code goes before the synchronise's; no memory is MILE_ERR_NOMEM with `nomem`.
template <class Run>
static int with_call_ws(size_t bytes, const char *nomem, hipStream_t st, Run run) {
  void *ws = nullptr;
  if (bytes && hipMalloc(&ws, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(MILE_ERR_NOMEM, nomem);
  }
  const int rc = run((char *)ws);
  const hipError_t es = hipStreamSynchronize(st);   // the kernels finish before their workspace goes
  if (ws) (void)hipFree(ws);
  if (rc != MILE_OK) return rc;
  HIP_TRY(es);
  return MILE_OK;
}
// the compute units of the current device, for the tensor-input calls that size a grid by them
static int current_cus(int *n_cu) {
  int dev = 0;
  *n_cu = 256;
  HIP_TRY(hipGetDevice(&dev));
  (void)hipDeviceGetAttribute(n_cu, hipDeviceAttributeMultiprocessorCount, dev);
  return MILE_OK;
}

// Where a tile's block of forward outputs lies and how many rows each draw has in it.  A statistic's tile loop asks its source
// for the tile of rows r0 .. r0 + nt: a tensor-input call answers with the caller's array at the tile's first row (ld = N), a
// streamed call stages the rows, forwards every draw into the workspace and answers with that (ld = nt).
struct Tile { const float *at; int64_t ld; };
// the streamed source of the statistics that read raw outputs: the block [D][nt][O] at the start of the workspace ws
static auto stream_tiles(mile_sampler *s, const float *theta, int64_t D, int64_t chunk, const void *X, char *ws, hipStream_t st) {
  return [=](int64_t r0, int nt, Tile &t) -> int {
    const int rc = stage_rows(s, (const float *)X + (size_t)r0 * eval_view(s).in_features, nullptr, nt, st);
    t = {(const float *)ws, nt};
    return rc != MILE_OK ? rc : forward_draws(s, theta, D, chunk, (float *)ws, st);
  };
}

extern "C" int32_t mile_pointwise_loglik(mile_sampler *s, const float *theta, int32_t S, const float *X, const void *y,
                                         int64_t N, float *out, void *stream) {
  const int rc = eval_args("mile_pointwise_loglik", s, !theta || !X || !y || !out, bad_SN(S, N), no_more_checks);
  return rc != MILE_OK ? rc : evaluate_rows(s, theta, S, X, y, N, out, stream);
}

extern "C" int32_t mile_predict(mile_sampler *s, const float *theta, int32_t S, const float *X, int64_t N, float *out, void *stream) {
  const int rc = eval_args("mile_predict", s, !theta || !X || !out, bad_SN(S, N), no_more_checks);
  return rc != MILE_OK ? rc : evaluate_rows(s, theta, S, X, nullptr, N, out, stream);
}

// mile_predict_moments: mile_predict's forward in passes of `chunk` draws into the library's workspace, each folded into the
// per-row accumulators by k_moments_accum; k_moments_finish writes out.  Every check before any launch.
extern "C" int32_t mile_predict_moments_width(const mile_sampler *s) {
  if (!s) return fail(MILE_ERR_INVALID, "mile_predict_moments_width: null handle");
  return eval_view(s).task == MILE_TASK_REGRESSION ? 3 : eval_view(s).O + 2;
}

extern "C" int32_t mile_predict_moments(mile_sampler *s, const float *theta, int64_t S, const void *X, int64_t N, float *out,
                                        int32_t *dropped, int64_t max_draws_per_pass, void *stream) {
  const int rc0 = eval_args("mile_predict_moments", s, !theta || !X || !out, bad_SN(S, N), [&] { return bad_caps(max_draws_per_pass, 0); });
  if (rc0 != MILE_OK) return rc0;
  const EvalView v = eval_view(s);
  const int task = v.task, O = v.O;
  if (task == MILE_TASK_REGRESSION && O != 2) return fail(MILE_ERR_INVALID, "mile_predict_moments: regression needs (mu, log sigma) outputs");
  hipStream_t st = (hipStream_t)stream;
  const int64_t per_draw = N * O * 4;
  const int64_t chunk = pass_draws(EVAL_PASS_TARGET, per_draw, max_draws_per_pass, S);
  // enough one-wave workgroups for about eight waves per CU, at most one slice per draw of a pass
  const int slices = (int)std::min<int64_t>(std::min<int64_t>(MOM_MAX_SLICES, chunk), std::max<int64_t>(1, ((int64_t)v.n_cu * 8 * MOM_NT + N - 1) / N));
  const size_t raw_bytes = r256((size_t)chunk * per_draw), acc_bytes = mom_acc_bytes(task, O, (int)N, slices);
  char *ws;
  const int rc2 = stream_ws("mile_predict_moments", s, raw_bytes + acc_bytes, "lower max_draws_per_pass", ws);
  if (rc2 != MILE_OK) return rc2;
  MomParams p{};
  p.raw = (const float *)ws; p.N = (int)N; p.O = O; p.slices = slices; p.S = S;
  p.acc = (double *)(ws + raw_bytes);
  p.cnt = (int32_t *)(p.acc + (size_t)slices * mom_planes(task, O) * N);
  p.out = out; p.dropped = dropped;
  HIP_TRY(hipMemsetAsync(p.acc, 0, acc_bytes, st));
  const int rc1 = stage_rows(s, (const float *)X, nullptr, N, st);
  if (rc1 != MILE_OK) return rc1;
  for (int64_t s0 = 0; s0 < S; s0 += chunk) {
    p.Sc = (int)std::min<int64_t>(chunk, S - s0);
    const int rc = eval_forward(s, theta + s0 * v.d, p.Sc, (float *)ws, st);
    if (rc != MILE_OK) return rc;
    HIP_TRY(mile_launch_moments_accum(task, p, st));
  }
  HIP_TRY(mile_launch_moments_finish(task, p, st));
  return MILE_OK;
}

// mile_mixture_quantiles / mile_predict_quantiles: every check before any launch; rows in tiles whose raw block and packed
// copy fit the evaluation budget, k_qnt_pack + k_qnt_solve per tile (mile_quantiles.h).
static double host_Phi(double z) { return 0.5 * std::erfc(-z * 0.70710678118654752440); }
// Phi^-1(p), 0 < p < 1, in fp64: bisection on the lower tail (where erfc keeps its relative accuracy), mirrored for p > 1/2
static double host_ndtri(double p) {
  if (p == 0.5) return 0.0;
  const double pl = p < 0.5 ? p : 1.0 - p;
  double lo = -40.0, hi = 0.0;
  for (int i = 0; i < 200 && hi - lo > 0.0; ++i) {
    const double mid = 0.5 * (lo + hi);
    if (mid <= lo || mid >= hi) break;
    if (host_Phi(mid) < pl) lo = mid; else hi = mid;
  }
  double z = 0.5 * (lo + hi);
  for (int i = 0; i < 2; ++i) {   // Newton polish
    const double f = std::exp(-0.5 * z * z) * 0.39894228040143267794;
    if (f > 0.0) z -= (host_Phi(z) - pl) / f;
  }
  return p < 0.5 ? z : -z;
}

// what is wrong with the levels or the outputs asked for, or null
static const char *qnt_bad_args(const double *levels, int32_t Q, const float *y, const float *quant, const float *pit) {
  if (!levels) return "null levels";
  if (Q < 1 || Q > QNT_MAX_Q) return "Q out of range (1 .. 32)";
  for (int i = 0; i < Q; ++i) {
    if (!(levels[i] > 0.0 && levels[i] < 1.0)) return "levels must lie strictly inside (0, 1)";
    if (i > 0 && !(levels[i] > levels[i - 1])) return "levels must be strictly increasing";
  }
  if (!quant && !pit) return "neither quantiles nor PIT asked for";
  if (pit && !y) return "PIT needs y";
  return nullptr;
}

// The plan of one call: rows per tile, draws per pass and the byte offset of every block of its workspace.  own_raw: the
// streamed call, whose workspace begins with the forward's raw block [S][Nt][2] (16 bytes per (draw, row) with the packed copy,
// tiles of whole transpose tiles) and ends with the sweeps [N]; else raw is the caller's and the packed copy comes first.
// C > 0: the chain-weighted form, whose weights [C] come last.
struct QntTilePlan { int64_t Nt, chunk; int slices; size_t pk, part, lev, sweeps, w, total; };
static QntTilePlan qnt_tile_plan(int64_t S, int64_t N, int n_cu, bool own_raw, int64_t max_rows, int64_t max_draws, int32_t C = 0) {
  QntTilePlan t;
  t.Nt = tile_rows(EVAL_PASS_TARGET, S * (own_raw ? 16 : 8), own_raw ? QNT_TILE : 1, max_rows, N);
  t.chunk = pass_draws(EVAL_NO_BUDGET, 1, max_draws, S);
  t.slices = qnt_slices((int)S, (int)t.Nt, n_cu);   // of the full tile, for every tile: the partials of a ragged last tile fit behind it
  t.pk = own_raw ? r256((size_t)S * t.Nt * 8) : 0;
  t.part = t.pk + qnt_pk_bytes(S, t.Nt);
  t.lev = t.part + qnt_part_bytes((int)t.Nt, QNT_MAX_Q, t.slices);
  t.sweeps = t.lev + r256(2 * QNT_MAX_Q * 8);
  t.w = t.sweeps + (own_raw ? r256((size_t)N * 4) : 0);
  t.total = t.w + (C > 0 ? r256((size_t)C * 8) : 0);
  return t;
}

// the chains of a weighted call: S = C * Sc draws, weights [C] on the host
struct QntChains { int32_t C; int64_t Sc; const double *weights; };
// what is wrong with them, or null
static const char *qnt_bad_chains(const QntChains &ch) {
  if (ch.C < 1 || ch.C > QNT_MAX_C) return "C out of range (1 .. 1024)";
  if (ch.Sc < 1 || ch.Sc > 0x7fffffff / ch.C) return "C * S out of range (1 .. 2^31 - 1)";
  return nullptr;
}
static const char *qnt_bad_weights(const QntChains &ch) {
  if (!ch.weights) return "null weights";
  double sum = 0.0;
  for (int c = 0; c < ch.C; ++c) {
    if (!std::isfinite(ch.weights[c]) || ch.weights[c] < 0.0) return "weights must be finite and >= 0";
    sum += ch.weights[c];
  }
  return std::fabs(sum - 1.0) <= 1e-9 ? nullptr : "the weights must sum to 1 (within 1e-9)";
}

// the tiles of one call, each from `source`; sweeps: record them in the workspace; ch: the chain-weighted form, dropped [C][N]
template <class Source>
static int qnt_run(char *ws, const QntTilePlan &t, int64_t S, int64_t N, const double *levels, int32_t Q, const float *y, float *quant,
                   float *pit, int32_t *dropped, bool sweeps, hipStream_t st, Source source, const QntChains *ch = nullptr) {
  double lev[2 * QNT_MAX_Q];
  for (int i = 0; i < Q; ++i) { lev[i] = levels[i]; lev[Q + i] = host_ndtri(levels[i]); }
  QntWParams p{};
  p.S = (int)S; p.Q = Q; p.slices = t.slices;
  p.pk = (float2 *)(ws + t.pk); p.part_brk = (double *)(ws + t.part); p.lev = (const double *)(ws + t.lev);
  HIP_TRY(hipMemcpyAsync(ws + t.lev, lev, (size_t)2 * Q * 8, hipMemcpyHostToDevice, st));
  if (ch) {
    p.C = ch->C; p.Sc = (int)ch->Sc; p.N = N; p.w = (const double *)(ws + t.w);
    HIP_TRY(hipMemcpyAsync(ws + t.w, ch->weights, (size_t)ch->C * 8, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipStreamSynchronize(st));   // lev is on this stack, the weights are the caller's host memory
  for (int64_t r0 = 0; r0 < N; r0 += t.Nt) {
    p.Nt = (int)std::min<int64_t>(t.Nt, N - r0);
    p.part_cnt = (int32_t *)(ws + t.part + r256((size_t)p.slices * p.Nt * Q * 16));
    Tile tile;
    const int rc = source(r0, p.Nt, tile);
    if (rc != MILE_OK) return rc;
    p.raw = tile.at; p.ld = tile.ld;
    p.y = y ? y + r0 : nullptr;
    p.quant = quant ? quant + r0 * Q : nullptr;
    p.pit = pit ? pit + r0 : nullptr;
    (ch ? p.dropped_c : p.dropped) = dropped ? dropped + r0 : nullptr;
    p.sweeps = sweeps ? (int32_t *)(ws + t.sweeps) + r0 : nullptr;
    HIP_TRY(ch ? mile_launch_quantiles_weighted(p, st) : mile_launch_quantiles(p, st));
  }
  return MILE_OK;
}

extern "C" int32_t mile_mixture_quantiles(const float *raw, int64_t S, int64_t N, const double *levels, int32_t Q, const float *y,
                                          float *quant, float *pit, int32_t *dropped, void *stream) {
  if (!raw) return bad("mile_mixture_quantiles", "null raw");
  if (const char *m = bad_SN(S, N)) return bad("mile_mixture_quantiles", m);
  if (const char *m = qnt_bad_args(levels, Q, y, quant, pit)) return bad("mile_mixture_quantiles", m);
  hipStream_t st = (hipStream_t)stream;
  int n_cu;
  const int rc0 = current_cus(&n_cu);
  if (rc0 != MILE_OK) return rc0;
  const QntTilePlan t = qnt_tile_plan(S, N, n_cu, false, 0, 0);
  return with_call_ws(t.total, "mile_mixture_quantiles: workspace allocation failed", st, [&](char *ws) {
    return qnt_run(ws, t, S, N, levels, Q, y, quant, pit, dropped, false, st,
                   [&](int64_t r0, int, Tile &tile) { tile = {raw + 2 * r0, N}; return (int)MILE_OK; });
  });
}

extern "C" int64_t mile_predict_quantiles_workspace(const mile_sampler *s, int64_t S, int64_t N) {
  return !s || bad_SN(S, N) ? -1 : (int64_t)qnt_tile_plan(S, N, eval_view(s).n_cu, true, 0, 0).total;
}

extern "C" int32_t mile_predict_quantiles(mile_sampler *s, const float *theta, int64_t S, const void *X, int64_t N,
                                          const double *levels, int32_t Q, const float *y, float *quant, float *pit, int32_t *dropped,
                                          int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream) {
  const int rc0 = eval_args("mile_predict_quantiles", s, !theta || !X, bad_SN(S, N), [&]() -> const char * {
    if (const char *m = qnt_bad_args(levels, Q, y, quant, pit)) return m;
    if (const char *m = bad_caps(max_draws_per_pass, max_rows_per_tile)) return m;
    return not_mu_log_sigma(s);
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const QntTilePlan t = qnt_tile_plan(S, N, eval_view(s).n_cu, true, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc1 = stream_ws("mile_predict_quantiles", s, t.total, "lower max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  const int rc = qnt_run(ws, t, S, N, levels, Q, y, quant, pit, dropped, quant != nullptr, st, stream_tiles(s, theta, S, t.chunk, X, ws, st));
  if (rc != MILE_OK) return rc;
  record_quantile_sweeps(s, (const int32_t *)(ws + t.sweeps), quant ? N : 0);
  return MILE_OK;
}

// The chain-weighted pair: the same plan, passes and workspace with the draws' C * S for S, and the weights behind them.
extern "C" int32_t mile_mixture_quantiles_weighted(const float *raw, int32_t C, int64_t S, int64_t N, const double *weights,
                                                   const double *levels, int32_t Q, const float *y, float *quant, float *pit,
                                                   int32_t *dropped, void *stream) {
  const char *fn = "mile_mixture_quantiles_weighted";
  const QntChains ch{C, S, weights};
  if (!raw) return bad(fn, "null raw");
  if (const char *m = qnt_bad_chains(ch)) return bad(fn, m);
  if (const char *m = bad_N(N)) return bad(fn, m);
  if (const char *m = qnt_bad_weights(ch)) return bad(fn, m);
  if (const char *m = qnt_bad_args(levels, Q, y, quant, pit)) return bad(fn, m);
  hipStream_t st = (hipStream_t)stream;
  int n_cu;
  const int rc0 = current_cus(&n_cu);
  if (rc0 != MILE_OK) return rc0;
  const int64_t D = (int64_t)C * S;
  const QntTilePlan t = qnt_tile_plan(D, N, n_cu, false, 0, 0, C);
  return with_call_ws(t.total, "mile_mixture_quantiles_weighted: workspace allocation failed", st, [&](char *ws) {
    return qnt_run(ws, t, D, N, levels, Q, y, quant, pit, dropped, false, st,
                   [&](int64_t r0, int, Tile &tile) { tile = {raw + 2 * r0, N}; return (int)MILE_OK; }, &ch);
  });
}

extern "C" int64_t mile_predict_quantiles_weighted_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N) {
  if (!s || qnt_bad_chains({C, S, nullptr}) || bad_N(N)) return -1;
  return (int64_t)qnt_tile_plan((int64_t)C * S, N, eval_view(s).n_cu, true, 0, 0, C).total;
}

extern "C" int32_t mile_predict_quantiles_weighted(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, int64_t N,
                                                   const double *weights, const double *levels, int32_t Q, const float *y, float *quant,
                                                   float *pit, int32_t *dropped, int64_t max_draws_per_pass, int64_t max_rows_per_tile,
                                                   void *stream) {
  const char *fn = "mile_predict_quantiles_weighted";
  const QntChains ch{C, S, weights};
  const char *shape = qnt_bad_chains(ch);
  const int rc0 = eval_args(fn, s, !theta || !X, shape ? shape : bad_N(N), [&]() -> const char * {
    if (const char *m = qnt_bad_weights(ch)) return m;
    if (const char *m = qnt_bad_args(levels, Q, y, quant, pit)) return m;
    if (const char *m = bad_caps(max_draws_per_pass, max_rows_per_tile)) return m;
    return not_mu_log_sigma(s);
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const int64_t D = (int64_t)C * S;
  const QntTilePlan t = qnt_tile_plan(D, N, eval_view(s).n_cu, true, max_rows_per_tile, max_draws_per_pass, C);
  char *ws;
  const int rc1 = stream_ws(fn, s, t.total, "lower max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  return qnt_run(ws, t, D, N, levels, Q, y, quant, pit, dropped, false, st, stream_tiles(s, theta, D, t.chunk, X, ws, st), &ch);
}

/* test and tool hook: sweeps of k_qnt_solve over the rows of the handle's last mile_predict_quantiles that asked for quantiles */
extern "C" int32_t mile_debug_quantile_sweeps(mile_sampler *s, int64_t *rows, int64_t *total, int32_t *most) {
  if (!s || !rows || !total || !most) return fail(MILE_ERR_INVALID, "mile_debug_quantile_sweeps: null argument");
  const int32_t *sweeps;
  *rows = recorded_quantile_sweeps(s, &sweeps); *total = 0; *most = 0;
  if (!*rows) return MILE_OK;
  HIP_TRY(hipSetDevice(eval_view(s).device));
  HIP_TRY(hipDeviceSynchronize());
  std::vector<int32_t> h((size_t)*rows);
  HIP_TRY(hipMemcpy(h.data(), sweeps, h.size() * 4, hipMemcpyDeviceToHost));
  for (int32_t v : h) { *total += v; *most = std::max(*most, v); }
  return MILE_OK;
}

// mile_psis_loo / mile_loo_stream: every check before any launch; rows in tiles whose [S][Nt] block of log-likelihoods and
// packed copy fit the evaluation budget, k_loo_pack + k_loo_row per tile (mile_loo.h).
static const char *loo_bad_SN(int64_t S, int64_t N) { return S < 2 || S > LOO_MAX_S ? "S out of range (2 .. 2^20)" : bad_N(N); }
// what is wrong with r_eff or the outputs asked for (S in range), or null
static const char *loo_bad_args(int64_t S, double r_eff, bool any_output) {
  if (!any_output) return "no output asked for";
  if (!std::isfinite(r_eff) || !(r_eff > 0.0)) return "r_eff must be finite and positive";
  if (loo_tail_host(S, r_eff) > LOO_MAX_TAIL) return "the tail is longer than 4096 draws (S / r_eff too large)";
  return nullptr;
}

struct LooOut {   // [C, N] each, any may be null
  double *lppd, *p_waic, *elpd_loo, *khat;
  int32_t *dropped;
  bool any() const { return lppd || p_waic || elpd_loo || khat || dropped; }
};

// The plan of one call: rows per tile, draws per pass and the byte offset of the packed copy in its workspace.  own_raw: the
// streamed call, whose workspace begins with the forward's block [S][Nt] (8 bytes per (draw, row) with the packed copy, tiles of
// whole transpose tiles); else loglik is the caller's and the packed copy is all there is.
struct LooTilePlan { int64_t Nt, chunk; size_t pk, total; };
static LooTilePlan loo_tile_plan(int64_t S, int64_t N, bool own_raw, int64_t max_rows, int64_t max_draws) {
  LooTilePlan t;
  t.Nt = tile_rows(EVAL_PASS_TARGET, S * (own_raw ? 8 : 4), own_raw ? LOO_TILE : 1, max_rows, N);
  t.chunk = pass_draws(EVAL_NO_BUDGET, 1, max_draws, S);
  t.pk = own_raw ? loo_pk_bytes(S, t.Nt) : 0;   // the forward's block is as large as its packed copy
  t.total = t.pk + loo_pk_bytes(S, t.Nt);
  return t;
}

// the tiles of one call, the C chains inside each: chain c's block [S][..] of the tile from `source`, its outputs at row c
template <class Source>
static int loo_run(char *ws, const LooTilePlan &t, int64_t C, int64_t S, int64_t N, int n_cu, double r_eff, const LooOut &o, hipStream_t st,
                   Source source) {
  LooParams p{};
  p.S = (int)S; p.pk = (float *)(ws + t.pk); p.r_eff = r_eff; p.M_full = loo_tail_host(S, r_eff);
  for (int64_t r0 = 0; r0 < N; r0 += t.Nt) {
    p.Nt = (int)std::min<int64_t>(t.Nt, N - r0);
    p.slices = loo_slices((int)S, p.Nt, n_cu);
    for (int64_t c = 0; c < C; ++c) {
      Tile tile;
      const int rc = source(r0, p.Nt, c, tile);
      if (rc != MILE_OK) return rc;
      p.ll = tile.at; p.ld = tile.ld;
      const size_t at = (size_t)c * N + r0;
      p.lppd = o.lppd ? o.lppd + at : nullptr;
      p.p_waic = o.p_waic ? o.p_waic + at : nullptr;
      p.elpd_loo = o.elpd_loo ? o.elpd_loo + at : nullptr;
      p.khat = o.khat ? o.khat + at : nullptr;
      p.dropped = o.dropped ? o.dropped + at : nullptr;
      HIP_TRY(mile_launch_loo(p, st));
    }
  }
  return MILE_OK;
}

extern "C" int32_t mile_psis_loo(const float *loglik, int64_t S, int64_t N, double r_eff, double *lppd, double *p_waic, double *elpd_loo,
                                 double *khat, int32_t *dropped, void *stream) {
  const LooOut o{lppd, p_waic, elpd_loo, khat, dropped};
  if (!loglik) return bad("mile_psis_loo", "null loglik");
  if (const char *m = loo_bad_SN(S, N)) return bad("mile_psis_loo", m);
  if (const char *m = loo_bad_args(S, r_eff, o.any())) return bad("mile_psis_loo", m);
  hipStream_t st = (hipStream_t)stream;
  int n_cu;
  const int rc0 = current_cus(&n_cu);
  if (rc0 != MILE_OK) return rc0;
  const LooTilePlan t = loo_tile_plan(S, N, false, 0, 0);
  return with_call_ws(t.total, "mile_psis_loo: workspace allocation failed", st, [&](char *ws) {
    return loo_run(ws, t, 1, S, N, n_cu, r_eff, o, st, [&](int64_t r0, int, int64_t, Tile &tile) { tile = {loglik + r0, N}; return (int)MILE_OK; });
  });
}

extern "C" int64_t mile_loo_stream_workspace(const mile_sampler *s, int64_t S, int64_t N) {
  return !s || loo_bad_SN(S, N) ? -1 : (int64_t)loo_tile_plan(S, N, true, 0, 0).total;
}

// mile_loo_stream (C = 1) and mile_chain_loo_stream: theta [C * S, d], chain c's S draws at row c * S, outputs [C, N].  A tile's
// rows are staged once for all chains; each chain's block [S][Nt] is forwarded and goes through k_loo_pack + k_loo_row on its
// own, as a call on that chain alone would send it.
static int loo_stream_chains(const char *fn, mile_sampler *s, const float *theta, int64_t C, int64_t S, const void *X, const void *y, int64_t N,
                             double r_eff, const LooOut &o, int64_t max_draws_per_pass, int64_t max_rows_per_tile, hipStream_t st) {
  const int rc0 = eval_args(fn, s, !theta || !X || !y, loo_bad_SN(S, N), [&]() -> const char * {
    if (C < 1 || C > 1024) return "C out of range (1 .. 1024)";
    if (const char *m = loo_bad_args(S, r_eff, o.any())) return m;
    return bad_caps(max_draws_per_pass, max_rows_per_tile);
  });
  if (rc0 != MILE_OK) return rc0;
  const LooTilePlan t = loo_tile_plan(S, N, true, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc1 = stream_ws(fn, s, t.total, "lower max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  const EvalView v = eval_view(s);
  float *raw = (float *)ws;
  return loo_run(ws, t, C, S, N, v.n_cu, r_eff, o, st, [&](int64_t r0, int nt, int64_t c, Tile &tile) -> int {
    if (c == 0) {   // the tile's rows and labels, staged when its first chain is asked for
      const int rc = stage_rows(s, (const float *)X + (size_t)r0 * v.in_features, (const char *)y + (size_t)r0 * 4, nt, st);
      if (rc != MILE_OK) return rc;
    }
    tile = {raw, nt};
    return forward_draws(s, theta + (size_t)c * S * v.d, S, t.chunk, raw, st);
  });
}

extern "C" int32_t mile_loo_stream(mile_sampler *s, const float *theta, int64_t S, const void *X, const void *y, int64_t N, double r_eff,
                                   double *lppd, double *p_waic, double *elpd_loo, double *khat, int32_t *dropped,
                                   int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream) {
  return loo_stream_chains("mile_loo_stream", s, theta, 1, S, X, y, N, r_eff, {lppd, p_waic, elpd_loo, khat, dropped}, max_draws_per_pass,
                           max_rows_per_tile, (hipStream_t)stream);
}

extern "C" int64_t mile_chain_loo_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N) {
  if (C < 1 || C > 1024) return -1;
  return mile_loo_stream_workspace(s, S, N);   // a chain at a time: the workspace of one
}

extern "C" int32_t mile_chain_loo_stream(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, const void *y, int64_t N,
                                         double r_eff, double *lppd, double *p_waic, double *elpd_loo, double *khat, int32_t *dropped,
                                         int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream) {
  return loo_stream_chains("mile_chain_loo_stream", s, theta, C, S, X, y, N, r_eff, {lppd, p_waic, elpd_loo, khat, dropped}, max_draws_per_pass,
                           max_rows_per_tile, (hipStream_t)stream);
}

// mile_psis_expect / mile_loo_predict_stream: every check before any launch; rows in tiles whose packed log-likelihoods, weights,
// partial sums and (streamed) forward block fit the evaluation budget; k_lxp_pack + k_lxp_row, then k_lxp_apply + k_lxp_finish
// per tile (mile_lxp.h).
struct LxpOut {   // expect, posterior [N, Q]; ess_w, khat, elpd_loo, dropped [N]; weights [N, S]; any may be null
  double *expect, *posterior, *ess_w, *khat, *elpd_loo;
  int32_t *dropped;
  double *weights;
  bool any() const { return expect || posterior || ess_w || khat || elpd_loo || dropped || weights; }
  bool sums() const { return expect || posterior; }
};
static const char *lxp_bad_Q(int32_t Q) { return Q < 1 || Q > LXP_MAX_Q ? "Q out of range (1 .. 64)" : nullptr; }
// what is wrong with the handle's head for the streamed call, or null; Q: the columns it forms
static const char *lxp_bad_head(const mile_sampler *s, int *Q) {
  const EvalView v = eval_view(s);
  if (v.task == MILE_TASK_REGRESSION) { *Q = 4; return not_mu_log_sigma(s); }
  *Q = v.O;
  return v.O > LXP_MAX_Q ? "more than 64 classes are not supported on the device (form the columns and call mile_psis_expect, or use the dense form)" : nullptr;
}

// The plan of one call: rows per tile, draws per pass and the byte offset of every block of its workspace.  O > 0: the streamed
// call, whose workspace begins with the forward's raw block [S][Nt][O] (tiles of whole transpose tiles).  Per (draw, row): the raw
// block O * 4, the packed l 4, the weight 8 where the workspace holds it (own_w); per row: the runs' partial sums where a sum is
// asked for.
struct LxpTilePlan { int64_t Nt, chunk; int runs; size_t pk, w, part, cnt, total; };
static LxpTilePlan lxp_tile_plan(int64_t S, int64_t N, int Q, int O, bool own_w, bool sums, int64_t max_rows, int64_t max_draws) {
  LxpTilePlan t;
  const int64_t per_row = S * (4 + (int64_t)O * 4 + (own_w ? 8 : 0)) + (sums ? (int64_t)lxp_part_row_bytes(S, Q) : 0);
  t.Nt = tile_rows(EVAL_PASS_TARGET, per_row, O > 0 ? LOO_TILE : 1, max_rows, N);
  t.chunk = pass_draws(EVAL_NO_BUDGET, 1, max_draws, S);
  t.runs = lxp_runs(S, Q);
  t.pk = O > 0 ? r256((size_t)S * t.Nt * O * 4) : 0;
  t.w = t.pk + loo_pk_bytes(S, t.Nt);
  t.part = t.w + (own_w ? lxp_w_bytes(S, t.Nt) : 0);
  t.cnt = t.part + (sums ? lxp_part_bytes(S, t.Nt, Q) : 0);
  t.total = t.cnt + (sums ? lxp_cnt_bytes(S, t.Nt, Q) : 0);
  return t;
}

// the tiles of one call, each from `source`: the caller's loglik (src LXP_SRC_VALUES, with the caller's values) or the forward's
// raw outputs, whose head the kernels apply (y: the caller's labels)
template <class Source>
static int lxp_run(char *ws, const LxpTilePlan &t, int64_t S, int64_t N, int n_cu, double r_eff, int src, int Q, int O, int task,
                   const float *values, const void *y, const LxpOut &o, hipStream_t st, Source source) {
  LxpParams p{};
  p.S = (int)S; p.O = O; p.task = task; p.pk = (float *)(ws + t.pk); p.r_eff = r_eff; p.M_full = loo_tail_host(S, r_eff);
  p.src = src; p.Q = Q; p.runs = t.runs;
  p.part = (double *)(ws + t.part); p.part_cnt = (int32_t *)(ws + t.cnt);
  for (int64_t r0 = 0; r0 < N; r0 += t.Nt) {
    p.Nt = (int)std::min<int64_t>(t.Nt, N - r0);
    p.slices = loo_slices((int)S, p.Nt, n_cu);
    Tile tile;
    const int rc = source(r0, p.Nt, tile);
    if (rc != MILE_OK) return rc;
    p.ld = tile.ld;
    if (src == LXP_SRC_VALUES) { p.ll = tile.at; p.values = values ? values + (size_t)r0 * Q : nullptr; }
    else { p.raw = tile.at; p.y = (const char *)y + (size_t)r0 * 4; }
    p.w = o.weights ? o.weights + (size_t)r0 * S : o.sums() ? (double *)(ws + t.w) : nullptr;
    p.ess_w = o.ess_w ? o.ess_w + r0 : nullptr;
    p.khat = o.khat ? o.khat + r0 : nullptr;
    p.elpd_loo = o.elpd_loo ? o.elpd_loo + r0 : nullptr;
    p.dropped = o.dropped ? o.dropped + r0 : nullptr;
    p.expect = o.expect ? o.expect + (size_t)r0 * Q : nullptr;
    p.posterior = o.posterior ? o.posterior + (size_t)r0 * Q : nullptr;
    HIP_TRY(mile_launch_lxp_rows(p, st));
    if (o.sums()) HIP_TRY(mile_launch_lxp_apply(p, st));
  }
  return MILE_OK;
}

extern "C" int32_t mile_psis_expect(const float *loglik, const float *values, int64_t S, int64_t N, int32_t Q, double r_eff, double *expect,
                                    double *posterior, double *ess_w, double *khat, double *elpd_loo, int32_t *dropped, double *weights,
                                    void *stream) {
  const LxpOut o{expect, posterior, ess_w, khat, elpd_loo, dropped, weights};
  if (!loglik) return bad("mile_psis_expect", "null loglik");
  if (const char *m = loo_bad_SN(S, N)) return bad("mile_psis_expect", m);
  if (const char *m = lxp_bad_Q(Q)) return bad("mile_psis_expect", m);
  if (const char *m = loo_bad_args(S, r_eff, o.any())) return bad("mile_psis_expect", m);
  if (!values && o.sums()) return bad("mile_psis_expect", "expect and posterior need values");
  hipStream_t st = (hipStream_t)stream;
  int n_cu;
  const int rc0 = current_cus(&n_cu);
  if (rc0 != MILE_OK) return rc0;
  const LxpTilePlan t = lxp_tile_plan(S, N, Q, 0, !weights && o.sums(), o.sums(), 0, 0);
  return with_call_ws(t.total, "mile_psis_expect: workspace allocation failed", st, [&](char *ws) {
    return lxp_run(ws, t, S, N, n_cu, r_eff, LXP_SRC_VALUES, Q, 0, 0, values, nullptr, o, st,
                   [&](int64_t r0, int, Tile &tile) { tile = {loglik + r0, N}; return (int)MILE_OK; });
  });
}

extern "C" int64_t mile_loo_predict_stream_workspace(const mile_sampler *s, int64_t S, int64_t N) {
  int Q = 0;
  if (!s || loo_bad_SN(S, N) || lxp_bad_head(s, &Q)) return -1;
  return (int64_t)lxp_tile_plan(S, N, Q, eval_view(s).O, true, true, 0, 0).total;
}

extern "C" int32_t mile_loo_predict_stream(mile_sampler *s, const float *theta, int64_t S, const void *X, const void *y, int64_t N, double r_eff,
                                           double *expect, double *posterior, double *ess_w, double *khat, double *elpd_loo, int32_t *dropped,
                                           int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream) {
  const char *fn = "mile_loo_predict_stream";
  const LxpOut o{expect, posterior, ess_w, khat, elpd_loo, dropped, nullptr};
  int Q = 0;
  const int rc0 = eval_args(fn, s, !theta || !X || !y, loo_bad_SN(S, N), [&]() -> const char * {
    if (const char *m = loo_bad_args(S, r_eff, o.any())) return m;
    if (const char *m = bad_caps(max_draws_per_pass, max_rows_per_tile)) return m;
    return lxp_bad_head(s, &Q);
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const EvalView v = eval_view(s);
  const LxpTilePlan t = lxp_tile_plan(S, N, Q, v.O, o.sums(), o.sums(), max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc1 = stream_ws(fn, s, t.total, "lower max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  const int src = v.task == MILE_TASK_REGRESSION ? LXP_SRC_REGR : LXP_SRC_CLASS;
  return lxp_run(ws, t, S, N, v.n_cu, r_eff, src, Q, v.O, v.task, nullptr, y, o, st, stream_tiles(s, theta, S, t.chunk, X, ws, st));
}

// mile_mixture_crps / mile_crps_stream: every check before any launch; rows in tiles that respect the evaluation budget, the
// pairs of one launch (CRPS_MAX_PAIRS_PER_LAUNCH) and the slots' bytes; k_crps_pack + k_crps_pairs + k_crps_finish per tile
// (mile_crps.h).
struct CrpsOut {
  double *crps_chain, *spread_chain, *crps_mix, *spread_mix, *gram;
  int32_t *dropped;
  bool any() const { return crps_chain || spread_chain || crps_mix || spread_mix || gram || dropped; }
  bool pairs() const { return crps_chain || spread_chain || crps_mix || spread_mix || gram; }
};
// what is wrong with the shape, or null; then (the shape in range) with the weights, the outputs asked for or the tile cap
static const char *crps_bad_shape(int32_t C, int64_t S, int64_t N) {
  if (C < 1 || C > CRPS_MAX_C) return "C out of range (1 .. 1024)";
  if (S < 1) return "S < 1";
  if (S > CRPS_MAX_DRAWS || (int64_t)C * S > CRPS_MAX_DRAWS) return "C * S out of range (1 .. 2^20)";
  return bad_N(N);
}
static const char *crps_bad_args(int32_t C, const double *weights, int32_t n_w, const CrpsOut &o, int64_t max_rows) {
  if (!o.any()) return "no output asked for";
  if (n_w < 0 || n_w > CRPS_MAX_W) return "n_w out of range (0 .. 8)";
  if (n_w > 0 && !weights) return "n_w > 0 without weights";
  for (int m = 0; m < n_w; ++m) {
    double sum = 0.0;
    for (int c = 0; c < C; ++c) {
      const double w = weights[(size_t)m * C + c];
      if (!std::isfinite(w) || w < 0.0) return "weights must be finite and >= 0";
      sum += w;
    }
    if (!(std::fabs(sum - 1.0) <= 1e-9)) return "every weight vector must sum to 1 (within 1e-9)";
  }
  return bad_caps(0, max_rows);
}

// The plan of one call: the pairs' units, rows per tile (the budget's, then the caps of one k_crps_pairs launch), draws per pass
// and the byte offset of every block of its workspace.  own_raw: the streamed call, whose workspace begins with the forward's raw
// block [C * S][Nt][2] (16 bytes per (draw, row) with the packed copy); else raw is the caller's and the packed copy comes first.
struct CrpsTilePlan { CrpsPlan pl; int64_t Nt, chunk; size_t pk, cnt, part, w, total; };
static CrpsTilePlan crps_tile_plan(int64_t C, int64_t S, int64_t N, bool own_raw, int64_t max_rows, int64_t max_draws) {
  CrpsTilePlan t;
  const int64_t D = C * S;
  t.pl = crps_plan(C, S, N);
  t.Nt = tile_rows(EVAL_PASS_TARGET, D * (own_raw ? 16 : 8), 1, max_rows, N);
  t.Nt = std::min(t.Nt, std::max<int64_t>(1, CRPS_MAX_PAIRS_PER_LAUNCH / (D * (D + 1) / 2)));
  t.Nt = std::min(t.Nt, std::max<int64_t>(1, CRPS_MAX_SLOT_BYTES / (t.pl.units * 8)));
  t.Nt = std::min(t.Nt, std::max<int64_t>(1, CRPS_MAX_GRID / t.pl.units));
  t.chunk = pass_draws(EVAL_NO_BUDGET, 1, max_draws, D);
  t.pk = own_raw ? r256((size_t)D * t.Nt * 8) : 0;
  t.cnt = t.pk + r256((size_t)D * t.Nt * 8);
  t.part = t.cnt + r256((size_t)t.Nt * C * 4);
  t.w = t.part + r256((size_t)t.Nt * t.pl.units * 8);
  t.total = t.w + r256((size_t)CRPS_MAX_W * C * 8);
  return t;
}

// the tiles of one call, each from `source`
template <class Source>
static int crps_run(char *ws, const CrpsTilePlan &t, int32_t C, int64_t S, int64_t N, const float *y, const double *weights, int32_t n_w,
                    const CrpsOut &o, hipStream_t st, Source source) {
  CrpsParams p{};
  p.C = C; p.S = (int)S; p.pl = t.pl; p.N = N; p.n_w = n_w;
  p.pk = (float2 *)(ws + t.pk); p.cnt = (int32_t *)(ws + t.cnt); p.part = (double *)(ws + t.part);
  if (n_w > 0) {
    HIP_TRY(hipMemcpyAsync(ws + t.w, weights, (size_t)n_w * C * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));   // weights is the caller's host memory
    p.w = (const double *)(ws + t.w);
  }
  p.crps_chain = o.crps_chain; p.spread_chain = o.spread_chain; p.crps_mix = o.crps_mix; p.spread_mix = o.spread_mix;
  p.gram = o.gram; p.dropped = o.dropped;
  for (int64_t r0 = 0; r0 < N; r0 += t.Nt) {
    p.Nt = (int)std::min<int64_t>(t.Nt, N - r0);
    p.r0 = r0;
    Tile tile;
    const int rc = source(r0, p.Nt, tile);
    if (rc != MILE_OK) return rc;
    p.raw = tile.at; p.ld = tile.ld;
    p.y = y + r0;
    HIP_TRY(mile_launch_crps_pack(p, st));
    if (!o.pairs()) continue;
    HIP_TRY(mile_launch_crps_pairs(p, st));
    HIP_TRY(mile_launch_crps_finish(p, st));
  }
  return MILE_OK;
}

extern "C" int32_t mile_mixture_crps(const float *raw, int32_t C, int64_t S, int64_t N, const float *y, const double *weights, int32_t n_w,
                                     double *crps_chain, double *spread_chain, double *crps_mix, double *spread_mix, double *gram,
                                     int32_t *dropped, int64_t max_rows_per_tile, void *stream) {
  if (!raw || !y) return bad("mile_mixture_crps", "null raw or y");
  const CrpsOut o{crps_chain, spread_chain, crps_mix, spread_mix, gram, dropped};
  if (const char *m = crps_bad_shape(C, S, N)) return bad("mile_mixture_crps", m);
  if (const char *m = crps_bad_args(C, weights, n_w, o, max_rows_per_tile)) return bad("mile_mixture_crps", m);
  hipStream_t st = (hipStream_t)stream;
  const CrpsTilePlan t = crps_tile_plan(C, S, N, false, max_rows_per_tile, 0);
  return with_call_ws(t.total, "mile_mixture_crps: workspace allocation failed (lower max_rows_per_tile)", st, [&](char *ws) {
    return crps_run(ws, t, C, S, N, y, weights, n_w, o, st, [&](int64_t r0, int, Tile &tile) { tile = {raw + 2 * r0, N}; return (int)MILE_OK; });
  });
}

extern "C" int64_t mile_crps_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N) {
  return !s || crps_bad_shape(C, S, N) ? -1 : (int64_t)crps_tile_plan(C, S, N, true, 0, 0).total;
}

extern "C" int32_t mile_crps_stream(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, const float *y, int64_t N,
                                    const double *weights, int32_t n_w, double *crps_chain, double *spread_chain, double *crps_mix,
                                    double *spread_mix, double *gram, int32_t *dropped, int64_t max_draws_per_pass,
                                    int64_t max_rows_per_tile, void *stream) {
  const CrpsOut o{crps_chain, spread_chain, crps_mix, spread_mix, gram, dropped};
  const int rc0 = eval_args("mile_crps_stream", s, !theta || !X || !y, crps_bad_shape(C, S, N), [&]() -> const char * {
    if (const char *m = crps_bad_args(C, weights, n_w, o, max_rows_per_tile)) return m;
    if (const char *m = bad_caps(max_draws_per_pass, 0)) return m;
    return not_mu_log_sigma(s);
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const CrpsTilePlan t = crps_tile_plan(C, S, N, true, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc1 = stream_ws("mile_crps_stream", s, t.total, "lower max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  return crps_run(ws, t, C, S, N, y, weights, n_w, o, st, stream_tiles(s, theta, (int64_t)C * S, t.chunk, X, ws, st));
}

// mile_stack_eval: every check before any launch; rows in tiles whose responsibilities fit 256 MiB, k_stk_rows + k_stk_gram per
// tile, k_stk_final at the end (mile_stack.h).  The workspace is this call's.
extern "C" int32_t mile_stack_eval(const double *lpd, const double *w, int32_t C, int64_t N, double *score, double *row_score, double *grad,
                                   double *hess, int64_t *used, int64_t max_rows_per_tile, void *stream) {
  if (!lpd || !w) return bad("mile_stack_eval", "null lpd or w");
  if (const char *m = stk_bad_args(C, N, max_rows_per_tile, score || row_score || grad || hess || used)) return bad("mile_stack_eval", m);
  hipStream_t st = (hipStream_t)stream;
  StkParams p{};
  p.lpd = lpd; p.w = w; p.C = C; p.Cx = C + 2; p.N = N;
  p.B = stk_block_rows(C, N); p.nb = (int)stk_blocks(C, N);
  p.want_grad = grad != nullptr; p.want_hess = hess != nullptr; p.want_sums = score || grad || hess || used;
  p.score = score; p.row_score = row_score; p.grad = grad; p.hess = hess; p.used = (long long *)used;
  const int64_t Nt = stk_tile_rows(C, N, max_rows_per_tile);
  p.ldR = Nt;
  const size_t rx_bytes = stk_rx_bytes(C, Nt);
  return with_call_ws(p.want_sums ? rx_bytes + stk_part_bytes(C, N) : 0, "mile_stack_eval: workspace allocation failed (lower max_rows_per_tile)",
                      st, [&](char *ws) -> int {
    if (ws) { p.Rx = (double *)ws; p.part = (double *)(ws + rx_bytes); }
    for (int64_t r0 = 0; r0 < N; r0 += Nt) {
      p.r0 = r0; p.Nt = (int)std::min<int64_t>(Nt, N - r0);
      HIP_TRY(mile_launch_stack_tile(p, st));
    }
    if (p.want_sums) HIP_TRY(mile_launch_stack_final(p, st));
    return MILE_OK;
  });
}

// mile_calibration / mile_calibration_stream: every check before any launch; rows in tiles whose per-chain sums and per-group
// records fit half the evaluation budget, k_cal_accum per pass of draws, k_cal_rows + k_cal_part per tile, k_cal_final at the
// end (mile_calib.h).
struct CalOut { double *probs; int32_t *kept, *order, *set_size, *rank; double *totals, *bins; };
// what is wrong with the shape, the levels or the outputs asked for, or null (pointers other than y and the outputs checked before)
static const char *cal_bad_args(int32_t C, int64_t S, int64_t N, int32_t K, const double *coverages, int32_t Q, int32_t n_bins, const void *y,
                                const CalOut &o) {
  if (!o.probs && !o.kept && !o.order && !o.set_size && !o.rank && !o.totals && !o.bins) return "no output asked for";
  if (C < 1 || C > 65535) return "C out of range (1 .. 65535)";
  if (const char *m = bad_SN(S, N)) return m;
  if (K < 2 || K > CAL_K_MAX) return "K out of range (2 .. 64)";
  if (Q < 1 || Q > CAL_Q_MAX) return "Q out of range (1 .. 16)";
  for (int i = 0; i < Q; ++i) {
    if (!(coverages[i] > 0.0 && coverages[i] < 1.0)) return "coverages must lie strictly inside (0, 1)";
    if (i > 0 && !(coverages[i] > coverages[i - 1])) return "coverages must be strictly increasing";
  }
  if (n_bins < 1 || n_bins > CAL_BINS_MAX) return "n_bins out of range (1 .. 64)";
  if (!y && (o.rank || o.totals || o.bins)) return "rank, totals and bins need y";
  if ((int64_t)C * S > 0x7fffffff) return "C * S above 2^31 - 1";
  return nullptr;
}

static const int64_t CAL_STATE_TARGET = (int64_t)128 << 20;   // bytes of a tile's sums, counts and records; the pass's logits take as much
// The plan of one call: rows per tile (whole k_cal_accum workgroups), draws per pass and the byte offset of every block of its
// workspace: sums, counts, records, the blocks' partial sums.  own_raw: the streamed call, whose workspace begins with a pass's
// logits [C][J][Nt][K], as many bytes as the tile's state; else raw is the caller's and its S draws are one pass.
struct CalTilePlan { int64_t Nt, J; size_t sum, cnt, rec, part, total; };
static CalTilePlan cal_tile_plan(int C, int K, int64_t S, int64_t N, int Q, int n_bins, bool own_raw, int64_t max_rows, int64_t max_draws) {
  CalTilePlan t;
  t.Nt = tile_rows(CAL_STATE_TARGET, (int64_t)cal_row_bytes(C, K), CAL_NT, max_rows, N);
  t.J = own_raw ? pass_draws(CAL_STATE_TARGET, (int64_t)C * t.Nt * K * 4, max_draws, S) : S;
  t.sum = own_raw ? r256((size_t)C * t.J * t.Nt * K * 4) : 0;
  t.cnt = t.sum + cal_sum_bytes(C, K, t.Nt);
  t.rec = t.cnt + cal_cnt_bytes(C, t.Nt);
  t.part = t.rec + cal_rec_bytes(C, t.Nt);
  t.total = t.part + cal_part_bytes(N, C + 1, cal_cols(Q, n_bins));
  return t;
}

// the tiles of one call: `accum` folds all draws of the tile p describes (r0, Nt) into p.sum / p.cnt, zeroed here
template <class Accum>
static int cal_run(char *ws, const CalTilePlan &t, int C, int64_t N, int K, const void *y, const double *coverages, int Q, int n_bins,
                   const CalOut &o, hipStream_t st, Accum accum) {
  const int W = cal_cols(Q, n_bins);
  const int64_t Nt = t.Nt;
  CalParams p{};
  p.C = C; p.K = K; p.Q = Q; p.n_bins = n_bins; p.N = N; p.y = (const int32_t *)y;
  for (int i = 0; i < Q; ++i) p.cov[i] = coverages[i];
  const bool reduce = y && (o.totals || o.bins);
  p.sum = (double *)(ws + t.sum); p.cnt = (int32_t *)(ws + t.cnt); p.rec = reduce ? (CalRec *)(ws + t.rec) : nullptr; p.part = (double *)(ws + t.part);
  p.B = cal_block_rows(N, C + 1, W); p.nblk = (N + p.B - 1) / p.B;
  p.probs = o.probs; p.kept = o.kept; p.order = o.order; p.set_size = o.set_size; p.rank = o.rank; p.totals = o.totals; p.bins = o.bins;
  if (reduce) HIP_TRY(hipMemsetAsync(p.part, 0, (size_t)(C + 1) * p.nblk * W * 8, st));
  for (int64_t r0 = 0; r0 < N; r0 += Nt) {
    p.r0 = r0; p.Nt = (int)std::min<int64_t>(Nt, N - r0);
    HIP_TRY(hipMemsetAsync(p.sum, 0, (size_t)C * p.Nt * K * 8, st));
    HIP_TRY(hipMemsetAsync(p.cnt, 0, (size_t)C * p.Nt * 4, st));
    const int rc = accum(p);
    if (rc != MILE_OK) return rc;
    HIP_TRY(mile_launch_cal_rows(p, st));
  }
  if (reduce) HIP_TRY(mile_launch_cal_final(p, st));
  return MILE_OK;
}

extern "C" int32_t mile_calibration(const float *raw, int32_t C, int64_t S, int64_t N, int32_t K, const void *y, const double *coverages,
                                    int32_t Q, int32_t n_bins, double *probs, int32_t *kept, int32_t *order, int32_t *set_size, int32_t *rank,
                                    double *totals, double *bins, void *stream) {
  const CalOut o{probs, kept, order, set_size, rank, totals, bins};
  if (!raw || !coverages) return bad("mile_calibration", "null argument");
  if (const char *m = cal_bad_args(C, S, N, K, coverages, Q, n_bins, y, o)) return bad("mile_calibration", m);
  hipStream_t st = (hipStream_t)stream;
  const CalTilePlan t = cal_tile_plan(C, K, S, N, Q, n_bins, false, 0, 0);
  return with_call_ws(t.total, "mile_calibration: workspace allocation failed", st, [&](char *ws) {
    return cal_run(ws, t, C, N, K, y, coverages, Q, n_bins, o, st, [&](CalParams &p) -> int {
      p.raw = raw + (size_t)p.r0 * K; p.cs = S; p.ld = N; p.J = (int)S;   // the caller's tensor, walked in place
      HIP_TRY(mile_launch_cal_accum(p, st));
      return MILE_OK;
    });
  });
}

extern "C" int64_t mile_calibration_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N) {
  if (!s || C < 1 || C > 65535 || bad_SN(S, N)) return -1;
  const int K = eval_view(s).O;
  if (eval_view(s).task != MILE_TASK_CLASSIFICATION || K < 2 || K > CAL_K_MAX) return -1;
  return (int64_t)cal_tile_plan(C, K, S, N, CAL_Q_MAX, CAL_BINS_MAX, true, 0, 0).total;
}

extern "C" int32_t mile_calibration_stream(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, const void *y, int64_t N,
                                           const double *coverages, int32_t Q, int32_t n_bins, double *probs, int32_t *kept, int32_t *order,
                                           int32_t *set_size, int32_t *rank, double *totals, double *bins, int64_t max_draws_per_pass,
                                           int64_t max_rows_per_tile, void *stream) {
  const CalOut o{probs, kept, order, set_size, rank, totals, bins};
  int K = 0;
  const int rc0 = eval_args("mile_calibration_stream", s, !theta || !X || !coverages, bad_SN(S, N), [&]() -> const char * {
    if (eval_view(s).task != MILE_TASK_CLASSIFICATION) return "needs a classification model";
    K = eval_view(s).O;
    if (const char *m = cal_bad_args(C, S, N, K, coverages, Q, n_bins, y, o)) return m;
    return bad_caps(max_draws_per_pass, max_rows_per_tile);
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const CalTilePlan t = cal_tile_plan(C, K, S, N, Q, n_bins, true, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc2 = stream_ws("mile_calibration_stream", s, t.total, "lower max_draws_per_pass or max_rows_per_tile", ws);
  if (rc2 != MILE_OK) return rc2;
  float *raw = (float *)ws;
  return cal_run(ws, t, C, N, K, y, coverages, Q, n_bins, o, st, [&](CalParams &p) -> int {
    const int rc1 = stage_rows(s, (const float *)X + (size_t)p.r0 * eval_view(s).in_features, nullptr, p.Nt, st);
    if (rc1 != MILE_OK) return rc1;
    p.raw = raw; p.ld = p.Nt;
    for (int64_t j0 = 0; j0 < S; j0 += t.J) {   // every (draw, row) forward once
      p.J = (int)std::min<int64_t>(t.J, S - j0); p.cs = p.J;
      const int rc = forward_chains(s, theta, C, S, j0, p.J, raw, st);
      if (rc != MILE_OK) return rc;
      HIP_TRY(mile_launch_cal_accum(p, st));
    }
    return MILE_OK;
  });
}

// mile_lppd_stream: mile_pointwise_loglik's forward on the same draw window of every chain, a pass at a time, into the library's
// workspace; k_lppd_accum folds the pass into the (m, s) state up to the next curve point, k_lppd_emit reduces the state there.
// Every check before any launch (the curve points come to the host for theirs: a copy, no kernel).
static bool lppd_shape_ok(int32_t C, int64_t N) { return C >= 1 && C <= LPPD_C_MAX && !bad_N(N); }

extern "C" int64_t mile_lppd_stream_workspace(const mile_sampler *s, int32_t C, int64_t N) {
  if (!s || !lppd_shape_ok(C, N)) return -1;
  return (int64_t)lppd_state_bytes(C, N);
}

extern "C" int32_t mile_lppd_stream(mile_sampler *s, const float *theta, int32_t C, int32_t S, const void *X, const void *y, int64_t N,
                                    const int32_t *curve_points, int32_t K, double *run_chain, double *run_ens, double *chain_lppd,
                                    double *row_lppd, double *lppd, int64_t *dropped, int64_t max_draws_per_pass, void *stream) {
  const int rc1 = eval_args("mile_lppd_stream", s, !theta || !X || !y, bad_SN(S, N), [&]() -> const char * {
    if (!lppd_shape_ok(C, N)) return "C out of range (1 .. 65535)";
    if (K < 0 || K > S) return "K out of range (0 .. S)";
    if (K == 0 && (run_chain || run_ens)) return "K = 0 with a curve output";
    if (K > 0 && !curve_points) return "null curve_points";
    if (K > 0 && !run_chain && !run_ens) return "curve points without a curve output";
    if (K == 0 && !chain_lppd && !row_lppd && !lppd && !dropped) return "no output asked for";
    return bad_caps(max_draws_per_pass, 0);
  });
  if (rc1 != MILE_OK) return rc1;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(eval_view(s).device));   // the curve points' copy comes before the preamble the other streamed calls share
  std::vector<int32_t> pts((size_t)K);
  if (K > 0) {
    HIP_TRY(hipMemcpyAsync(pts.data(), curve_points, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < K; ++i) {
      if (pts[i] < 1 || pts[i] > S) return fail(MILE_ERR_INVALID, "mile_lppd_stream: curve point outside [1, S]");
      if (i > 0 && pts[i] <= pts[i - 1]) return fail(MILE_ERR_INVALID, "mile_lppd_stream: curve points not strictly increasing");
    }
  }
  const int64_t per_draw = (int64_t)C * N * 4;   // one draw of every chain
  const int64_t J = pass_draws(EVAL_PASS_TARGET, per_draw, max_draws_per_pass, std::min<int64_t>(S, LPPD_J_MAX));
  const size_t raw_bytes = r256((size_t)J * per_draw), st_bytes = lppd_state_bytes(C, N);
  char *ws;
  const int rc2 = stream_ws("mile_lppd_stream", s, raw_bytes + st_bytes, "lower max_draws_per_pass", ws);
  if (rc2 != MILE_OK) return rc2;
  const size_t cn = (size_t)C * (size_t)N;
  LppdParams p{};
  p.ll = (const float *)ws; p.C = C; p.N = (int)N; p.S = S; p.waves = lppd_waves(N);
  p.state = (double2 *)(ws + raw_bytes);
  p.cnt = (int32_t *)(p.state + cn);
  p.part_ens = (double *)((char *)p.cnt + (cn * 4 + 7) / 8 * 8);
  p.part_chain = p.part_ens + p.waves;
  p.part_cnt = (long long *)(p.part_chain + (size_t)p.waves * C);
  p.run_chain = run_chain; p.run_ens = run_ens; p.chain_lppd = chain_lppd; p.row_lppd = row_lppd; p.lppd = lppd;
  p.dropped = (long long *)dropped;
  const bool want_final = chain_lppd || row_lppd || lppd || dropped;
  const int rc0 = stage_rows(s, (const float *)X, y, N, st);
  if (rc0 != MILE_OK) return rc0;
  p.fresh = 1;    // the first launch of k_lppd_accum starts every (chain, row) at (m, s) = (-inf, 0), cnt = 0
  int next = 0;   // next curve point
  for (int64_t j0 = 0; j0 < S; j0 += J) {
    p.J = (int)std::min<int64_t>(J, S - j0);
    const int rc = forward_chains(s, theta, C, S, j0, p.J, (float *)ws, st);
    if (rc != MILE_OK) return rc;
    int ja = 0;
    while (ja < p.J) {   // split the pass at every curve point inside it
      const int jb = next < K && pts[next] <= j0 + p.J ? (int)(pts[next] - j0) : p.J;
      p.ja = ja; p.jb = jb;
      HIP_TRY(mile_launch_lppd_accum(p, st));
      p.fresh = 0;
      if (next < K && pts[next] == j0 + jb) {
        p.point = next++;
        HIP_TRY(mile_launch_lppd_emit(p, want_final && j0 + jb == S, st));
      }
      ja = jb;
    }
  }
  if (want_final && (K == 0 || pts[K - 1] != S)) {
    p.point = -1;
    HIP_TRY(mile_launch_lppd_emit(p, true, st));
  }
  return MILE_OK;
}

// mile_chain_diagnostics: every check before any launch; parameters in chunks that fit the workspace --------------------------
static int diag_shape_ok(int32_t C, int32_t S, int64_t d) {
  return C >= 1 && C <= DIAG_C_MAX && S >= DIAG_S_MIN && S <= DIAG_S_MAX && d >= 1 && d <= ((int64_t)1 << 40);
}
static const int64_t DIAG_WS_TARGET = (int64_t)256 << 20;   // workspace asked for: chunks of as many parameters as fit in it
// an output of `what` whose pointer is null: the message, or null
static const char *diag_null_output(uint32_t what, const float *wcv, const float *bcv, const float *ess, const float *crhat, const float *rhat) {
  if (((what & MILE_DIAG_WCV) && !wcv) || ((what & MILE_DIAG_BCV) && !bcv) || ((what & MILE_DIAG_ESS) && !ess) ||
      ((what & MILE_DIAG_CRHAT) && !crhat) || ((what & MILE_DIAG_RHAT) && !rhat))
    return "null pointer for an output asked for";
  return nullptr;
}

extern "C" int64_t mile_chain_diagnostics_workspace(int32_t C, int32_t S, int64_t d, uint32_t what) {
  if (!diag_shape_ok(C, S, d)) return -1;
  const int64_t per = diag_param_bytes(C, S, what);
  const int64_t chunk = std::max<int64_t>(DIAG_TILE, DIAG_WS_TARGET / per / DIAG_TILE * DIAG_TILE);
  return per * std::min<int64_t>(d, chunk);
}

extern "C" int32_t mile_chain_diagnostics(const float *samples, int32_t C, int32_t S, int64_t d, int32_t n_splits, uint32_t what,
                                          float *wcv, float *bcv, float *ess, float *crhat, float *rhat, void *workspace,
                                          int64_t workspace_bytes, void *stream) {
  const uint32_t outs = MILE_DIAG_WCV | MILE_DIAG_BCV | MILE_DIAG_ESS | MILE_DIAG_CRHAT | MILE_DIAG_RHAT;
  if (!samples) return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: null samples");
  if (!diag_shape_ok(C, S, d)) return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: needs 1 <= C <= 65535, 4 <= S <= 4096, d >= 1");
  if (n_splits < 1 || S % n_splits) return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: n_splits must divide S");
  if (S / n_splits < 2) return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: fewer than 2 draws per split");
  if (!(what & outs) || (what & ~(outs | MILE_DIAG_POOLED_INPUT))) return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: bad `what`");
  if (const char *m = diag_null_output(what, wcv, bcv, ess, crhat, rhat)) return bad("mile_chain_diagnostics", m);
  const bool pooled_in = what & MILE_DIAG_POOLED_INPUT;
  if (pooled_in && (what & (MILE_DIAG_WCV | MILE_DIAG_BCV | MILE_DIAG_CRHAT)))
    return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: wcv, bcv and crhat need the raw draws");
  if (!pooled_in && (what & (MILE_DIAG_ESS | MILE_DIAG_RHAT)) && (int64_t)C * S > DIAG_POOL_MAX)
    return fail(MILE_ERR_INVALID, "mile_chain_diagnostics: unsupported: C * S > 16384 pooled draws (pass pooled scores)");
  const int64_t per = diag_param_bytes(C, S, what);
  if (!workspace || workspace_bytes < per * std::min<int64_t>(d, DIAG_TILE))
    return fail(MILE_ERR_STATE, "mile_chain_diagnostics: workspace too small");
  int64_t chunk = std::min<int64_t>(d, workspace_bytes / per);
  if (chunk < d) chunk = chunk / DIAG_TILE * DIAG_TILE;
  chunk = std::min<int64_t>(chunk, 1 << 20);
  DiagParams p{};
  p.samples = samples; p.C = C; p.S = S; p.n_splits = n_splits; p.d = d; p.what = what;
  p.wcv = wcv; p.bcv = bcv; p.ess = ess; p.crhat = crhat; p.rhat = rhat;
  p.stat = (double *)workspace;                                      // [chunk][C][DIAG_NSTAT], then the fp32 planes
  float *planes = (float *)((char *)workspace + chunk * C * DIAG_NSTAT * 8);
  p.raw = pooled_in ? nullptr : planes;
  p.z = pooled_in ? planes : planes + chunk * C * S;
  for (int64_t p0 = 0; p0 < d; p0 += chunk) {
    p.p0 = p0;
    p.P = (int)std::min<int64_t>(chunk, d - p0);
    HIP_TRY(mile_launch_diag(p, (hipStream_t)stream));
  }
  return MILE_OK;
}

// mile_function_diagnostics: every check before any launch; rows in tiles whose raw block, two [P][C][S] planes and stat block fit
// the evaluation budget; per tile the forward, k_fdiag_pack, k_fdiag_lp and mile_chain_diagnostics' launches on the tile's columns
// (mile_fdiag.h).  The plan of one call: the head's width, rows per tile, draws per pass and the byte offset of every block.
struct FdiagPlan { int O, Q; int64_t D, NQ, M, nt, chunk; size_t plane, z, stat, acc, part, total; };
static FdiagPlan fdiag_plan(int O, int C, int S, int64_t N, bool with_y, int64_t max_rows, int64_t max_draws) {
  FdiagPlan t;
  t.O = O; t.Q = t.O + (with_y ? 1 : 0);
  t.D = (int64_t)C * S; t.NQ = N * t.Q; t.M = t.NQ + (with_y ? 1 : 0);
  const int64_t per_row = t.D * t.O * 4 + t.Q * diag_param_bytes(C, S, 0);
  int64_t cap = FDIAG_P_MAX / t.Q;
  if (max_rows > 0 && max_rows < cap) cap = max_rows;
  t.nt = tile_rows(EVAL_PASS_TARGET, per_row, 1, cap, N);
  t.chunk = pass_draws(EVAL_PASS_TARGET, t.nt * t.O * 4, max_draws, t.D);
  const size_t plane = r256((size_t)t.nt * t.Q * t.D * 4);
  t.plane = r256((size_t)t.D * t.nt * t.O * 4);
  t.z = t.plane + plane;
  t.stat = t.z + plane;
  t.acc = t.stat + r256((size_t)t.nt * t.Q * C * DIAG_NSTAT * 8);
  t.part = t.acc + r256((size_t)t.D * 8);
  t.total = t.part + r256(fdiag_part_bytes(C, t.NQ));
  return t;
}
static const char *fdiag_bad_shape(int32_t C, int32_t S, int64_t N) {
  return !diag_shape_ok(C, S, 1) ? "needs 1 <= C <= 65535 and 4 <= S <= 4096" : bad_N(N);
}

extern "C" int64_t mile_function_diagnostics_workspace(const mile_sampler *s, int32_t C, int32_t S, int64_t N, int32_t with_y) {
  if (!s || fdiag_bad_shape(C, S, N) || eval_view(s).O > FDIAG_O_MAX) return -1;
  return (int64_t)fdiag_plan(eval_view(s).O, C, S, N, with_y != 0, 0, 0).total;
}

extern "C" int32_t mile_function_diagnostics(mile_sampler *s, const float *theta, int32_t C, int32_t S, const void *X, const void *y, int64_t N,
                                             int32_t n_splits, uint32_t what, float *wcv, float *bcv, float *ess, float *crhat, float *rhat,
                                             float *columns, double *loglik_sum, double *summary, double *chain_summary,
                                             int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream) {
  const uint32_t outs = MILE_DIAG_WCV | MILE_DIAG_BCV | MILE_DIAG_ESS | MILE_DIAG_CRHAT | MILE_DIAG_RHAT;
  const uint32_t summed = MILE_DIAG_ESS | MILE_DIAG_CRHAT | MILE_DIAG_RHAT;
  const int rc0 = eval_args("mile_function_diagnostics", s, !theta || !X, fdiag_bad_shape(C, S, N), [&]() -> const char * {
    if (eval_view(s).O > FDIAG_O_MAX) return "more than 64 head outputs";
    if (n_splits < 1 || S % n_splits) return "n_splits must divide S";
    if (S / n_splits < 2) return "fewer than 2 draws per split";
    if (what & MILE_DIAG_POOLED_INPUT) return "MILE_DIAG_POOLED_INPUT: the columns are formed here, there is no input that could hold scores";
    if (what & ~outs) return "bad `what`";
    if (!what && !columns && !loglik_sum) return "no output asked for";
    if (const char *m = diag_null_output(what, wcv, bcv, ess, crhat, rhat)) return m;
    if ((!(what & MILE_DIAG_WCV) && wcv) || (!(what & MILE_DIAG_BCV) && bcv) || (!(what & MILE_DIAG_ESS) && ess) ||
        (!(what & MILE_DIAG_CRHAT) && crhat) || (!(what & MILE_DIAG_RHAT) && rhat))
      return "an output whose statistic is not in `what`";
    if ((summary || chain_summary) && (what & summed) != summed) return "summary and chain_summary need ESS, CRHAT and RHAT in `what`";
    if (loglik_sum && !y) return "loglik_sum needs y";
    if ((what & (MILE_DIAG_ESS | MILE_DIAG_RHAT)) && (int64_t)C * S > DIAG_POOL_MAX)
      return "unsupported: C * S > 16384 pooled draws (take WCV, BCV, CRHAT and `columns`, and rank those outside)";
    return bad_caps(max_draws_per_pass, max_rows_per_tile);
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const FdiagPlan t = fdiag_plan(eval_view(s).O, C, S, N, y != nullptr, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc2 = stream_ws("mile_function_diagnostics", s, t.total, "lower max_rows_per_tile", ws);
  if (rc2 != MILE_OK) return rc2;
  FdiagParams f{};
  f.out = (const float *)ws; f.D = (int)t.D; f.O = t.O; f.Q = t.Q; f.task = eval_view(s).task;
  f.raw = (float *)(ws + t.plane); f.acc = (double *)(ws + t.acc);
  DiagParams p{};
  p.C = C; p.S = S; p.n_splits = n_splits; p.d = t.M; p.what = what;   // samples stays null: k_fdiag_pack fills the raw plane
  p.raw = f.raw; p.z = (float *)(ws + t.z); p.stat = (double *)(ws + t.stat);
  p.wcv = wcv; p.bcv = bcv; p.ess = ess; p.crhat = crhat; p.rhat = rhat;
  if (y) HIP_TRY(hipMemsetAsync(f.acc, 0, (size_t)t.D * 8, st));
  auto source = stream_tiles(s, theta, t.D, t.chunk, X, ws, st);         // the raw block [D][nt][O] at the start of the workspace
  for (int64_t r0 = 0; r0 < N; r0 += t.nt) {
    const int nt = (int)std::min<int64_t>(t.nt, N - r0);
    Tile tile;
    const int rc1 = source(r0, nt, tile);
    if (rc1 != MILE_OK) return rc1;
    f.out = tile.at; f.nt = nt; f.y = y ? (const char *)y + (size_t)r0 * 4 : nullptr; f.lcol = nullptr;
    HIP_TRY(mile_launch_fdiag_pack(f, st));
    if (y) HIP_TRY(mile_launch_fdiag_lp(f, st));
    const size_t m0 = (size_t)r0 * t.Q;
    if (columns) HIP_TRY(hipMemcpyAsync(columns + m0 * t.D, f.raw, (size_t)nt * t.Q * t.D * 4, hipMemcpyDeviceToDevice, st));
    if (what) {
      p.p0 = (long long)m0; p.P = nt * t.Q;
      HIP_TRY(mile_launch_diag(p, st));
    }
  }
  if (y) {                                                              // the L column: one chunk of its own
    f.nt = 0; f.lcol = f.raw;
    HIP_TRY(mile_launch_fdiag_lp(f, st));
    if (columns) HIP_TRY(hipMemcpyAsync(columns + (size_t)t.NQ * t.D, f.raw, (size_t)t.D * 4, hipMemcpyDeviceToDevice, st));
    if (loglik_sum) HIP_TRY(hipMemcpyAsync(loglik_sum, f.acc, (size_t)t.D * 8, hipMemcpyDeviceToDevice, st));
    if (what) {
      p.p0 = t.NQ; p.P = 1;
      HIP_TRY(mile_launch_diag(p, st));
    }
  }
  if (summary || chain_summary) {
    FdiagSumParams q{};
    q.rhat = rhat; q.crhat = crhat; q.ess = ess; q.M = t.M; q.NQ = t.NQ; q.C = C; q.B = fdiag_sum_blocks(C, t.NQ);
    q.part = (FdiagPart *)(ws + t.part); q.summary = summary; q.chain_summary = chain_summary;
    HIP_TRY(mile_launch_fdiag_summary(q, st));
  }
  return MILE_OK;
}

// mile_chain_diagnostics_tail: every check before any launch; parameters in chunks that fit the workspace, each through
// mile_dtail.h's launches and, for rhat_folded, mile_chain_diagnostics' own on the folded score plane ------------------------------
static const char *diag_bad_splits(int32_t S, int32_t n_splits) {
  if (n_splits < 1 || S % n_splits) return "n_splits must divide S";
  return S / n_splits < 2 ? "fewer than 2 draws per split" : nullptr;
}
// workspace bytes of one parameter: the x plane (unless the input is one), z and zf, k_diag_chain's moments, the four ESS and
// the sd, the two thresholds
static int64_t dtail_param_bytes(int C, int S, uint32_t what) {
  const int64_t cs = (int64_t)C * S * 4;
  return ((what & MILE_DTAIL_PLANE_INPUT) ? 2 : 3) * cs + (int64_t)C * DIAG_NSTAT * 8 + DTAIL_NRES * 8 + 2 * 4;
}
static int64_t diag_ws_chunk(int64_t per) { return std::max<int64_t>(DIAG_TILE, DIAG_WS_TARGET / per / DIAG_TILE * DIAG_TILE); }
// the parameters per chunk of a workspace of `bytes`: all of them, or a multiple of the transpose tile
static int64_t diag_chunk_of(int64_t bytes, int64_t per, int64_t d) {
  int64_t chunk = std::min<int64_t>(d, bytes / per);
  if (chunk < d) chunk = chunk / DIAG_TILE * DIAG_TILE;
  return std::min<int64_t>(chunk, 1 << 20);
}

extern "C" int64_t mile_chain_diagnostics_tail_workspace(int32_t C, int32_t S, int64_t d, uint32_t what) {
  if (!diag_shape_ok(C, S, d)) return -1;
  const int64_t per = dtail_param_bytes(C, S, what);
  return per * std::min<int64_t>(d, diag_ws_chunk(per));
}

extern "C" int32_t mile_chain_diagnostics_tail(const float *samples, int32_t C, int32_t S, int64_t d, int32_t n_splits, uint32_t what,
                                               float *ess_bulk, float *ess_tail, float *ess_mean, float *mcse_mean, float *rhat_folded,
                                               float *quantiles, void *workspace, int64_t workspace_bytes, void *stream) {
  const char *fn = "mile_chain_diagnostics_tail";
  const uint32_t outs = MILE_DTAIL_ESS_BULK | MILE_DTAIL_ESS_TAIL | MILE_DTAIL_ESS_MEAN | MILE_DTAIL_RHAT_FOLDED;
  const uint32_t sorted = MILE_DTAIL_ESS_BULK | MILE_DTAIL_ESS_TAIL | MILE_DTAIL_RHAT_FOLDED;
  if (!samples) return bad(fn, "null samples");
  if (!diag_shape_ok(C, S, d)) return bad(fn, "needs 1 <= C <= 65535, 4 <= S <= 4096, d >= 1");
  if (const char *m = diag_bad_splits(S, n_splits)) return bad(fn, m);
  if (!(what & outs) || (what & ~(outs | MILE_DTAIL_PLANE_INPUT))) return bad(fn, "bad `what`");
  if (((what & MILE_DTAIL_ESS_BULK) && !ess_bulk) || ((what & MILE_DTAIL_ESS_TAIL) && !ess_tail) ||
      ((what & MILE_DTAIL_ESS_MEAN) && (!ess_mean || !mcse_mean)) || ((what & MILE_DTAIL_RHAT_FOLDED) && !rhat_folded))
    return bad(fn, "null pointer for an output asked for");
  const bool sort = (what & sorted) || quantiles;
  if (sort && (int64_t)C * S > DIAG_POOL_MAX)
    return bad(fn, "unsupported: C * S > 16384 pooled draws (sort outside, pass the series to mile_multichain_ess)");
  const int64_t per = dtail_param_bytes(C, S, what);
  if (!workspace || workspace_bytes < per * std::min<int64_t>(d, DIAG_TILE)) return fail(MILE_ERR_STATE, std::string(fn) + ": workspace too small");
  const bool plane_in = what & MILE_DTAIL_PLANE_INPUT;
  const int64_t chunk = diag_chunk_of(workspace_bytes, per, d), cs = (int64_t)C * S;
  hipStream_t st = (hipStream_t)stream;
  DiagParams g{};                                   // the transpose, and R-hat of the folded scores
  g.C = C; g.S = S; g.n_splits = n_splits; g.d = d; g.rhat = rhat_folded;
  g.stat = (double *)workspace;                                       // [chunk][C][DIAG_NSTAT], [chunk][DTAIL_NRES], then the fp32 blocks
  DtailParams t{};
  t.C = C; t.S = S; t.n_splits = n_splits; t.d = d; t.quantiles = quantiles;
  t.res = g.stat + chunk * C * DIAG_NSTAT;
  t.z = (float *)(t.res + chunk * DTAIL_NRES);
  t.zf = t.z + chunk * cs;
  float *xplane = plane_in ? nullptr : t.zf + chunk * cs;
  t.thr = t.zf + chunk * cs * (plane_in ? 1 : 2);
  t.want_zf = (what & MILE_DTAIL_RHAT_FOLDED) != 0;
  t.series = ((what & MILE_DTAIL_ESS_BULK) ? 1u : 0u) | ((what & MILE_DTAIL_ESS_TAIL) ? 6u : 0u) | ((what & MILE_DTAIL_ESS_MEAN) ? 8u : 0u);
  if (what & MILE_DTAIL_ESS_BULK) t.ess_bulk = ess_bulk;
  if (what & MILE_DTAIL_ESS_TAIL) t.ess_tail = ess_tail;
  if (what & MILE_DTAIL_ESS_MEAN) { t.ess_mean = ess_mean; t.mcse_mean = mcse_mean; }
  for (int64_t p0 = 0; p0 < d; p0 += chunk) {
    const int P = (int)std::min<int64_t>(chunk, d - p0);
    t.p0 = p0; t.P = P;
    if (plane_in) {
      t.x = samples + p0 * cs;
    } else {
      g.samples = samples; g.what = 0; g.raw = xplane; g.p0 = p0; g.P = P;
      HIP_TRY(mile_launch_diag_transpose(g, st));
      t.x = xplane;
    }
    if (sort) HIP_TRY(mile_launch_dtail_derive(t, st));
    if (t.series) {
      HIP_TRY(mile_launch_dtail_ess(t, st));
      HIP_TRY(mile_launch_dtail_final(t, st));
    }
    if (what & MILE_DTAIL_RHAT_FOLDED) {
      g.samples = nullptr; g.what = MILE_DIAG_RHAT | MILE_DIAG_POOLED_INPUT; g.raw = nullptr; g.z = t.zf; g.p0 = p0; g.P = P;
      HIP_TRY(mile_launch_diag(g, st));
    }
  }
  return MILE_OK;
}

extern "C" int64_t mile_multichain_ess_workspace(int32_t C, int32_t S, int64_t m, int32_t plane_input) {
  if (!diag_shape_ok(C, S, m)) return -1;
  if (plane_input) return 0;
  const int64_t per = (int64_t)C * S * 4;
  return per * std::min<int64_t>(m, diag_ws_chunk(per));
}

extern "C" int32_t mile_multichain_ess(const float *series, int32_t C, int32_t S, int64_t m, int32_t n_splits, int32_t plane_input,
                                       float *ess, void *workspace, int64_t workspace_bytes, void *stream) {
  const char *fn = "mile_multichain_ess";
  if (!series || !ess) return bad(fn, "null series or ess");
  if (!diag_shape_ok(C, S, m)) return bad(fn, "needs 1 <= C <= 65535, 4 <= S <= 4096, m >= 1");
  if (const char *e = diag_bad_splits(S, n_splits)) return bad(fn, e);
  const int64_t cs = (int64_t)C * S, per = cs * 4;
  if (!plane_input && (!workspace || workspace_bytes < per * std::min<int64_t>(m, DIAG_TILE)))
    return fail(MILE_ERR_STATE, std::string(fn) + ": workspace too small");
  const int64_t chunk = plane_input ? std::min<int64_t>(m, 1 << 20) : diag_chunk_of(workspace_bytes, per, m);
  hipStream_t st = (hipStream_t)stream;
  DiagParams g{};
  g.samples = series; g.C = C; g.S = S; g.n_splits = n_splits; g.d = m; g.raw = (float *)workspace;
  DtailParams t{};
  t.C = C; t.S = S; t.n_splits = n_splits; t.d = m; t.series = 8u; t.ess_plain = ess;
  for (int64_t p0 = 0; p0 < m; p0 += chunk) {
    const int P = (int)std::min<int64_t>(chunk, m - p0);
    t.p0 = p0; t.P = P;
    if (plane_input) {
      t.x = series + p0 * cs;
    } else {
      g.p0 = p0; g.P = P;
      HIP_TRY(mile_launch_diag_transpose(g, st));
      t.x = g.raw;
    }
    HIP_TRY(mile_launch_dtail_ess(t, st));
  }
  return MILE_OK;
}

// mile_predict_sensitivities: every check before any launch; rows in tiles and draws in passes whose block [Sc][Nt][P][F] of
// Jacobians fits the evaluation budget; k_sens_jac + k_sens_accum + k_sens_chain per pass, k_sens_finish per tile, k_sens_chain_finish
// after the last (mile_sens.h).
struct SensOut {
  float *mean, *sd, *pos;       // [N, P, F]
  int32_t *dropped;             // [N]
  double *chain_ape, *chain_abs;   // [C, P, F]
  int64_t *chain_kept;          // [C]
  bool any() const { return rows() || chains(); }
  bool rows() const { return mean || sd || pos || dropped; }
  bool chains() const { return chain_ape || chain_abs || chain_kept; }
};
static const char *sens_bad_shape(int32_t C, int64_t S, int64_t N) {
  if (C < 1 || C > 1024) return "C out of range (1 .. 1024)";
  if (S < 1 || S > 0x7fffffff / C) return "C * S out of range (1 .. 2^31 - 1)";
  return bad_N(N);
}
// what keeps the handle's model from k_sens_jac, or null; net: the FCN as the kernel takes it
static const char *sens_bad_model(const mile_sampler *s, SensNet *net) {
  const mile_model_spec *spec = eval_spec(s);
  if (spec->model != MILE_MODEL_FCN) return "needs an FCN (token ids and image pixels have no input sensitivities here)";
  if (spec->task == MILE_TASK_REGRESSION && spec->widths[spec->n_layers - 1] != 2) return "regression needs (mu, log sigma) outputs";
  int32_t b_off[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS];
  const long long d = fcn_param_layout(spec, {b_off, w_off});
  *net = sens_net(spec, b_off, w_off, (int)d);
  return sens_R(*net) < 1 ? "network too wide: one row's activations and sweeps do not fit 160 KiB of LDS" : nullptr;
}

// The plan of one call: rows per tile, draws per pass (of the C * S = D draws, chains one after the other), the slices of
// k_sens_accum and the byte offset of every block of its workspace.  Per (draw, row) P * F floats of jac; per row also the
// accumulators of at most SENS_MAX_SLICES slices.
struct SensTilePlan { int64_t Nt, chunk; int slices; size_t acc, chain, total; };
static SensTilePlan sens_tile_plan(const SensNet &net, int n_cu, int32_t C, int64_t D, int64_t N, int64_t max_rows, int64_t max_draws) {
  SensTilePlan t;
  const int64_t PF = (int64_t)net.widths[net.n_layers - 1] * net.in_features;
  t.Nt = tile_rows(EVAL_PASS_TARGET, PF * 4 + SENS_MAX_SLICES * PF * 24, 1, max_rows, N);
  t.chunk = pass_draws(EVAL_PASS_TARGET, t.Nt * PF * 4, max_draws, D);
  // enough workgroups for about eight waves per CU, at most one slice per draw of a pass
  const int64_t cols = t.Nt * PF;
  t.slices = (int)std::min<int64_t>(std::min<int64_t>(SENS_MAX_SLICES, t.chunk), std::max<int64_t>(1, ((int64_t)n_cu * 8 * 64 + cols - 1) / cols));
  t.acc = r256((size_t)t.chunk * t.Nt * PF * 4);
  t.chain = t.acc + r256(sens_acc_bytes(t.Nt, (int)PF, t.slices));
  t.total = t.chain + r256(sens_chain_bytes(C, (int)PF));
  return t;
}

// the tiles of one call, the passes inside each
static int sens_run(char *ws, const SensTilePlan &t, const SensNet &net, int n_cu, const float *theta, int32_t C, int64_t S, const float *X,
                    int64_t N, const SensOut &o, hipStream_t st) {
  const int F = net.in_features, PF = net.widths[net.n_layers - 1] * F, R = sens_R(net);
  const int64_t D = (int64_t)C * S;
  SensJacParams jp{};
  jp.net = net; jp.jac = (float *)ws; jp.R = R;
  SensAccParams ap{};
  ap.jac = (const float *)ws; ap.PF = PF; ap.slices = t.slices; ap.D = D;
  SensChainParams cp{};
  cp.jac = (const float *)ws; cp.PF = PF; cp.C = C; cp.S = S;
  cp.sum = (double *)(ws + t.chain); cp.abs = cp.sum + (size_t)C * PF; cp.kept = (long long *)(cp.abs + (size_t)C * PF);
  cp.o_ape = o.chain_ape; cp.o_abs = o.chain_abs; cp.o_kept = (long long *)o.chain_kept;
  if (o.chains()) HIP_TRY(hipMemsetAsync(ws + t.chain, 0, sens_chain_bytes(C, PF), st));
  for (int64_t r0 = 0; r0 < N; r0 += t.Nt) {
    const int nt = (int)std::min<int64_t>(t.Nt, N - r0);
    const size_t cols = (size_t)nt * PF;
    jp.Nt = ap.Nt = cp.Nt = nt;
    jp.X = X + (size_t)r0 * F;
    ap.mean = (double *)(ws + t.acc); ap.M2 = ap.mean + (size_t)t.slices * cols;
    ap.pos = (int32_t *)(ap.M2 + (size_t)t.slices * cols); ap.cnt = ap.pos + (size_t)t.slices * cols;
    ap.o_mean = o.mean ? o.mean + (size_t)r0 * PF : nullptr;
    ap.o_sd = o.sd ? o.sd + (size_t)r0 * PF : nullptr;
    ap.o_pos = o.pos ? o.pos + (size_t)r0 * PF : nullptr;
    ap.dropped = o.dropped ? o.dropped + r0 : nullptr;
    if (o.rows()) HIP_TRY(hipMemsetAsync(ws + t.acc, 0, sens_acc_bytes(nt, PF, t.slices), st));
    for (int64_t d0 = 0; d0 < D; d0 += t.chunk) {
      const int Sc = (int)std::min<int64_t>(t.chunk, D - d0);
      jp.theta = theta + (size_t)d0 * net.d;
      jp.SB = (int)std::max<int64_t>(1, std::min<int64_t>((2 * (int64_t)n_cu + Sc - 1) / Sc, (nt + R - 1) / R));
      HIP_TRY(mile_launch_sens_jac(jp, Sc, st));
      ap.Sc = cp.Sc = Sc; cp.d0 = d0;
      if (o.rows()) HIP_TRY(mile_launch_sens_accum(ap, st));
      if (o.chains()) HIP_TRY(mile_launch_sens_chain(cp, st));
    }
    if (o.rows()) HIP_TRY(mile_launch_sens_finish(ap, st));
  }
  if (o.chains()) HIP_TRY(mile_launch_sens_chain_finish(cp, st));
  return MILE_OK;
}

extern "C" int64_t mile_predict_sensitivities_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N) {
  SensNet net;
  if (!s || sens_bad_shape(C, S, N) || sens_bad_model(s, &net)) return -1;
  return (int64_t)sens_tile_plan(net, eval_view(s).n_cu, C, (int64_t)C * S, N, 0, 0).total;
}

extern "C" int32_t mile_predict_sensitivities(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, int64_t N,
                                              int64_t max_draws_per_pass, int64_t max_rows_per_tile, float *mean, float *sd, float *pos,
                                              int32_t *dropped, double *chain_ape, double *chain_abs, int64_t *chain_kept, void *stream) {
  const char *fn = "mile_predict_sensitivities";
  const SensOut o{mean, sd, pos, dropped, chain_ape, chain_abs, chain_kept};
  SensNet net;
  const int rc0 = eval_args(fn, s, !theta || !X, sens_bad_shape(C, S, N), [&]() -> const char * {
    if (!o.any()) return "no output asked for";
    if (const char *m = bad_caps(max_draws_per_pass, max_rows_per_tile)) return m;
    if (const char *m = sens_bad_model(s, &net)) return m;
    // no output may lie over theta [C * S, d] or X [N, F]: both are read until the last tile's last pass
    const size_t PF = (size_t)net.widths[net.n_layers - 1] * net.in_features;
    const uintptr_t in[2][2] = {{(uintptr_t)theta, (size_t)C * S * net.d * 4}, {(uintptr_t)X, (size_t)N * net.in_features * 4}};
    const uintptr_t out[7][2] = {{(uintptr_t)mean, (size_t)N * PF * 4}, {(uintptr_t)sd, (size_t)N * PF * 4}, {(uintptr_t)pos, (size_t)N * PF * 4},
                                 {(uintptr_t)dropped, (size_t)N * 4}, {(uintptr_t)chain_ape, (size_t)C * PF * 8},
                                 {(uintptr_t)chain_abs, (size_t)C * PF * 8}, {(uintptr_t)chain_kept, (size_t)C * 8}};
    for (const auto &b : out)
      for (const auto &a : in)
        if (b[0] && a[0] < b[0] + b[1] && b[0] < a[0] + a[1]) return "an output overlaps theta or X";
    return nullptr;
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const EvalView v = eval_view(s);
  const SensTilePlan t = sens_tile_plan(net, v.n_cu, C, (int64_t)C * S, N, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc1 = stream_ws(fn, s, t.total, "lower max_draws_per_pass or max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  return sens_run(ws, t, net, v.n_cu, theta, C, S, (const float *)X, N, o, st);
}

// mile_predict_partial_dependence: every check before any launch; rows in tiles and draws in passes whose block
// [Sc][Nt][Fs][G][P] of head outputs fits the evaluation budget; k_pdp_fwd + k_pdp_accum + k_pdp_rows per pass, k_pdp_row_finish per
// tile, k_pdp_finish after the last (mile_pdp.h).
struct PdpOut {
  float *ice_mean, *ice_sd;     // [N, Fs, G, P]
  int32_t *dropped;             // [N, Fs]
  float *curves;                // [C S, Fs, G, P]
  double *pd_mean, *pd_sd;      // [Fs, G, P]
  double *chain_pd;             // [C, Fs, G, P]
  int64_t *chain_draws;         // [C, Fs]
  bool any() const { return ice() || pd(); }
  bool ice() const { return ice_mean || ice_sd || dropped; }
  bool pd() const { return curves || pd_mean || pd_sd || chain_pd || chain_draws; }
};
// what keeps the handle's model or the selection's size from k_pdp_fwd, or null; net: the FCN as the kernel takes it
static const char *pdp_bad_model(const mile_sampler *s, int32_t C, int64_t S, int32_t Fs, int32_t G, PdpNet *net) {
  const mile_model_spec *spec = eval_spec(s);
  if (spec->model != MILE_MODEL_FCN) return "needs an FCN (token ids and image pixels have no partial dependence here)";
  if (spec->task == MILE_TASK_REGRESSION && spec->widths[spec->n_layers - 1] != 2) return "regression needs (mu, log sigma) outputs";
  if (Fs < 1 || Fs > spec->in_features) return "Fs out of range (1 .. F)";
  if (G < 1 || G > PDP_G_MAX) return "G out of range (1 .. 256)";
  int32_t b_off[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS];
  const long long d = fcn_param_layout(spec, {b_off, w_off});
  *net = pdp_net(spec, b_off, w_off, (int)d);
  if (pdp_lds(*net, Fs).R < 1) return "network too wide: one row's first layer and one pseudo-row do not fit 160 KiB of LDS";
  // C * S <= 2^31 - 1, Fs * G * P small enough for the product to stay inside int64
  if ((int64_t)Fs * G * spec->widths[spec->n_layers - 1] > PDP_CELL_MAX / 8 / ((int64_t)C * S))
    return "the per-draw sums [C * S, Fs, G, P] fp64 exceed 1 GiB: call it on fewer features (columns of different features are "
           "independent, so the results are the same bits)";
  return nullptr;
}

// The plan of one call.  Rows per tile, draws per pass and the slices of k_pdp_accum are sized as if all F features were
// selected, so that a call on a subset of the features runs the tiles, passes and slices of the full call and returns its bits;
// the blocks of the workspace take what the Fs selected ones need.
struct PdpTilePlan { int64_t Nt, chunk; int slices; size_t feat, acc, sum, kept, chain, total; };
static PdpTilePlan pdp_tile_plan(const PdpNet &net, int n_cu, int32_t C, int64_t D, int64_t N, int32_t Fs, int32_t G, int64_t max_rows,
                                 int64_t max_draws) {
  PdpTilePlan t;
  const int64_t GP = (int64_t)G * net.widths[net.n_layers - 1], QF = GP * net.in_features, Q = GP * Fs;
  t.Nt = tile_rows(EVAL_PASS_TARGET, QF * 4 + PDP_MAX_SLICES * QF * 20, 1, max_rows, N);
  t.chunk = pass_draws(EVAL_PASS_TARGET, t.Nt * QF * 4, max_draws, D);
  const int64_t cols = t.Nt * QF;
  t.slices = (int)std::min<int64_t>(std::min<int64_t>(PDP_MAX_SLICES, t.chunk), std::max<int64_t>(1, ((int64_t)n_cu * 8 * 64 + cols - 1) / cols));
  t.feat = r256((size_t)t.chunk * t.Nt * Q * 4);
  t.acc = t.feat + r256((size_t)Fs * 4);
  t.sum = t.acc + r256(pdp_acc_bytes(t.Nt, Q, t.slices));
  t.kept = t.sum + r256((size_t)D * Q * 8);
  t.chain = t.kept + r256((size_t)D * Fs * 4);
  t.total = t.chain + r256(pdp_chain_bytes(C, Q));
  return t;
}

// the tiles of one call, the passes inside each
static int pdp_run(char *ws, const PdpTilePlan &t, const PdpNet &net, int n_cu, const float *theta, int32_t C, int64_t S, const float *X,
                   int64_t N, const int32_t *features, int32_t Fs, const float *grid, int32_t G, const PdpOut &o, hipStream_t st) {
  const int F = net.in_features, GP = G * net.widths[net.n_layers - 1], Q = Fs * GP;
  const PdpLds lds = pdp_lds(net, Fs);
  const int64_t D = (int64_t)C * S;
  // from the caller's pageable array, which may be gone once the call returns: HIP stages a pageable source before
  // hipMemcpyAsync returns (as for the levels and weights of the quantile calls above)
  HIP_TRY(hipMemcpyAsync(ws + t.feat, features, (size_t)Fs * 4, hipMemcpyHostToDevice, st));
  PdpFwdParams fp{};
  fp.net = net; fp.val = (float *)ws; fp.features = (const int32_t *)(ws + t.feat); fp.grid = grid; fp.Fs = Fs; fp.G = G;
  fp.R = (int)std::min<int64_t>(lds.R, std::max<int64_t>(1, ((int64_t)1 << 30) / Q));   // R * Q stays inside int
  fp.PR = lds.PR;
  PdpAccParams ap{};
  ap.val = (const float *)ws; ap.Q = Q; ap.GP = GP; ap.slices = t.slices; ap.D = D;
  PdpRowsParams rp{};
  rp.val = (const float *)ws; rp.Q = Q; rp.GP = GP; rp.Fs = Fs; rp.C = C; rp.S = S;
  rp.sum = (double *)(ws + t.sum); rp.kept = (int32_t *)(ws + t.kept);
  rp.c_mean = (double *)(ws + t.chain); rp.c_M2 = rp.c_mean + (size_t)C * Q; rp.c_n = (int32_t *)(rp.c_M2 + (size_t)C * Q);
  rp.curves = o.curves; rp.pd_mean = o.pd_mean; rp.pd_sd = o.pd_sd; rp.chain_pd = o.chain_pd; rp.chain_draws = (long long *)o.chain_draws;
  if (o.pd()) HIP_TRY(hipMemsetAsync(ws + t.sum, 0, t.chain - t.sum, st));
  for (int64_t r0 = 0; r0 < N; r0 += t.Nt) {
    const int nt = (int)std::min<int64_t>(t.Nt, N - r0);
    const size_t cols = (size_t)nt * Q;
    fp.Nt = ap.Nt = rp.Nt = nt;
    fp.X = X + (size_t)r0 * F;
    ap.mean = (double *)(ws + t.acc); ap.M2 = ap.mean + (size_t)t.slices * cols; ap.cnt = (int32_t *)(ap.M2 + (size_t)t.slices * cols);
    ap.o_mean = o.ice_mean ? o.ice_mean + (size_t)r0 * Q : nullptr;
    ap.o_sd = o.ice_sd ? o.ice_sd + (size_t)r0 * Q : nullptr;
    ap.dropped = o.dropped ? o.dropped + (size_t)r0 * Fs : nullptr;
    if (o.ice()) HIP_TRY(hipMemsetAsync(ws + t.acc, 0, pdp_acc_bytes(nt, Q, t.slices), st));
    for (int64_t d0 = 0; d0 < D; d0 += t.chunk) {
      const int Sc = (int)std::min<int64_t>(t.chunk, D - d0);
      fp.theta = theta + (size_t)d0 * net.d;
      fp.SB = (int)std::max<int64_t>(1, std::min<int64_t>((2 * (int64_t)n_cu + Sc - 1) / Sc, (nt + fp.R - 1) / fp.R));
      HIP_TRY(mile_launch_pdp_fwd(fp, Sc, st));
      ap.Sc = rp.Sc = Sc; rp.d0 = d0;
      if (o.ice()) HIP_TRY(mile_launch_pdp_accum(ap, st));
      if (o.pd()) HIP_TRY(mile_launch_pdp_rows(rp, st));
    }
    if (o.ice()) HIP_TRY(mile_launch_pdp_row_finish(ap, st));
  }
  if (o.pd()) HIP_TRY(mile_launch_pdp_finish(rp, st));
  return MILE_OK;
}

extern "C" int64_t mile_predict_partial_dependence_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N, int32_t Fs, int32_t G) {
  PdpNet net;
  if (!s || sens_bad_shape(C, S, N) || pdp_bad_model(s, C, S, Fs, G, &net)) return -1;
  return (int64_t)pdp_tile_plan(net, eval_view(s).n_cu, C, (int64_t)C * S, N, Fs, G, 0, 0).total;
}

extern "C" int32_t mile_predict_partial_dependence(mile_sampler *s, const float *theta, int32_t C, int64_t S, const void *X, int64_t N,
                                                   const int32_t *features, int32_t Fs, const float *grid, int32_t G,
                                                   int64_t max_draws_per_pass, int64_t max_rows_per_tile, float *ice_mean, float *ice_sd,
                                                   int32_t *dropped, float *curves, double *pd_mean, double *pd_sd, double *chain_pd,
                                                   int64_t *chain_draws, void *stream) {
  const char *fn = "mile_predict_partial_dependence";
  const PdpOut o{ice_mean, ice_sd, dropped, curves, pd_mean, pd_sd, chain_pd, chain_draws};
  PdpNet net;
  const int rc0 = eval_args(fn, s, !theta || !X || !features || !grid, sens_bad_shape(C, S, N), [&]() -> const char * {
    if (!o.any()) return "no output asked for";
    if (const char *m = bad_caps(max_draws_per_pass, max_rows_per_tile)) return m;
    if (const char *m = pdp_bad_model(s, C, S, Fs, G, &net)) return m;
    std::vector<char> seen((size_t)net.in_features, 0);
    for (int i = 0; i < Fs; ++i) {
      if (features[i] < 0 || features[i] >= net.in_features) return "a feature index is out of range (0 .. F - 1)";
      if (seen[features[i]]++) return "a feature index is repeated";
    }
    // no output may lie over theta [C * S, d], X [N, F] or grid [Fs, G]: all are read until the last tile's last pass
    const size_t Q = (size_t)Fs * G * net.widths[net.n_layers - 1], D = (size_t)C * S;
    const uintptr_t in[3][2] = {{(uintptr_t)theta, D * net.d * 4}, {(uintptr_t)X, (size_t)N * net.in_features * 4}, {(uintptr_t)grid, (size_t)Fs * G * 4}};
    const uintptr_t out[8][2] = {{(uintptr_t)ice_mean, (size_t)N * Q * 4}, {(uintptr_t)ice_sd, (size_t)N * Q * 4}, {(uintptr_t)dropped, (size_t)N * Fs * 4},
                                 {(uintptr_t)curves, D * Q * 4}, {(uintptr_t)pd_mean, Q * 8}, {(uintptr_t)pd_sd, Q * 8},
                                 {(uintptr_t)chain_pd, (size_t)C * Q * 8}, {(uintptr_t)chain_draws, (size_t)C * Fs * 8}};
    for (const auto &b : out)
      for (const auto &a : in)
        if (b[0] && a[0] < b[0] + b[1] && b[0] < a[0] + a[1]) return "an output overlaps theta, X or grid";
    return nullptr;
  });
  if (rc0 != MILE_OK) return rc0;
  hipStream_t st = (hipStream_t)stream;
  const EvalView v = eval_view(s);
  const PdpTilePlan t = pdp_tile_plan(net, v.n_cu, C, (int64_t)C * S, N, Fs, G, max_rows_per_tile, max_draws_per_pass);
  char *ws;
  const int rc1 = stream_ws(fn, s, t.total, "lower max_draws_per_pass or max_rows_per_tile", ws);
  if (rc1 != MILE_OK) return rc1;
  return pdp_run(ws, t, net, v.n_cu, theta, C, S, (const float *)X, N, features, Fs, grid, G, o, st);
}

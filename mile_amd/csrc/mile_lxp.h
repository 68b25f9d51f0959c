// PSIS-LOO expectations of the ensemble (mile_psis_expect, mile_loo_predict_stream): the smoothed, normalised importance weights
// of mile_psis_loo kept per draw, and with them the leave-one-out expectation sum_s w_s h_q(s, n) of Q per-draw columns next to
// their in-sample mean.  include/mile_hip.h states the definition.  Kernels in mile_lxp.hip on the device helpers of
// mile_loo_device.h; the entry points (argument checks, the row tiles and the passes over the draws) in mile_eval.hip.
//
// One tile of Nt rows goes through four launches:
//   k_lxp_pack   k_loo_pack's transpose ll [S][ld] -> pk [Nt][S] (NaN: a draw left out of the row).  <true>: the streamed call,
//                where l is row_loglik (mile_row_head.h) of the forward's raw outputs [S][ld][O], formed on the way in.
//   k_lxp_row    one workgroup of four waves per row: k_loo_row's stages 1 to 6 (the functions of mile_loo_device.h), which leave
//                the smoothed log weights of the tail in LDS, ascending, and log Z = mlw + log s1.  Then
//                a. w_i = exp(lw_i - log Z) in place of lw_i;
//                b. the tie rule inside the tail: the thread that finds the head of a run of equal keys below the cut key T sums
//                   the run serially and leaves its mean in the head's slot (a run's slots are read and written by its head
//                   alone); the draws with key == T share (a workgroup sum of their tail slots' weights + the weights of those
//                   the tail did not take) / their count;
//                c. one pass over the row in draw order: a dropped draw 0, key > T exp(r - log Z), key == T the shared boundary
//                   weight, key < T the head's slot, found by a lower-bound search in the sorted keys -> w [Nt][S] fp64 (the
//                   caller's or the workspace), and ess_w = 1 / sum w^2 by a workgroup sum.
//                dropped, khat and elpd_loo come from the same launch, the latter two by k_loo_row's operations in its order.
//                LDS is k_loo_row's: the row at most 64 KiB (dynamic), the keys 16 KiB, x / lw / w 32 KiB, the rest 3.5 KiB.
//   k_lxp_apply  grid (ceil(Nt / 32), ceil(runs / G)): the weighted and the plain sums of the columns over one run of draws each.
//                The draw axis is cut into `runs` = lxp_runs(S, Q) runs of whole 32-draw tiles, a function of S and Q alone.
//                A workgroup takes 32 rows and G = lxp_groups(Q) runs, 256 / G threads each.  Per step it brings one 32 x 32
//                tile of weights per run through LDS (read along draws, used along rows; -1 marks a dropped draw, a row or a
//                draw outside the tile: nothing of such a (draw, row) is read), then every thread adds draw after draw, in
//                index order, to its up to 8 (row, column) sums in fp64: thread e of a group owns element e, e + 256 / G, ... of
//                the 32 Q columns of the 32 rows, which lie contiguous in a draw's block of values, so a draw is read as one
//                coalesced run.  <LXP_SRC_VALUES>: the caller's fp32 columns.  <LXP_SRC_REGR>, <LXP_SRC_CLASS>: the streamed
//                call's heads on the forward's raw outputs, in fp64: (mu, mu^2, sigma^2, Phi((y - mu) / sigma)), or the softmax
//                probabilities from a per-(draw, row) log-sum-exp formed with the tile.
//   k_lxp_finish one thread per (row, column): the runs' partial sums and kept counts in index order -> expect, posterior.
// fp64 sums, fixed order, no floating-point atomics: a row's result depends on its own S draws alone, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mile_hip.h"
#include "mile_eval_plan.h"
#include "mile_loo.h"

#define LXP_MAX_Q 64              // columns of a call; K of the streamed classification head
#define LXP_MAX_RUNS 64           // runs of the draw axis per group slot: at most LXP_MAX_RUNS * LXP_MAX_GROUPS runs
#define LXP_MAX_GROUPS 4          // runs that one k_lxp_apply workgroup takes side by side
#define LXP_MAX_ELEMS 8           // (row, column) sums of a thread: 32 * LXP_MAX_Q / 256

enum { LXP_SRC_VALUES = 0, LXP_SRC_REGR = 1, LXP_SRC_CLASS = 2 };

struct LxpParams {
  // k_lxp_pack: the tile's log-likelihoods ll [S][ld], or (head) the raw outputs raw [S][ld][O] with the labels y of the tile
  const float *ll;
  const float *raw;
  const void *y;           // at the tile's first row
  long long ld;            // rows per draw in ll / raw / values
  int S, Nt, slices, O, task;
  float *pk;               // [Nt][S]
  // k_lxp_row
  double r_eff;
  int M_full;
  double *w;               // [Nt][S] at the tile's first row: the caller's weights or the workspace; null: not written
  double *ess_w, *khat, *elpd_loo;   // [Nt] at the tile's first row, each may be null
  int32_t *dropped;
  // k_lxp_apply, k_lxp_finish
  int src, Q, runs;
  const float *values;     // [S][ld][Q] at the tile's first row (LXP_SRC_VALUES)
  double *part;            // [2][runs][Nt * Q]: the weighted, then the plain partial sums
  int32_t *part_cnt;       // [runs][Nt]
  double *expect, *posterior;   // [Nt][Q] at the tile's first row, each may be null
};

// runs of one k_lxp_apply workgroup, and runs of the draw axis: functions of Q and S alone
__host__ __device__ static inline int lxp_groups(int Q) {
  const int g = 256 / (LOO_TILE * Q);
  return g < 1 ? 1 : g > LXP_MAX_GROUPS ? LXP_MAX_GROUPS : g;
}
static inline int lxp_runs(int64_t S, int Q) {
  const int64_t s_tiles = (S + LOO_TILE - 1) / LOO_TILE, cap = (int64_t)LXP_MAX_RUNS * lxp_groups(Q);
  return (int)(s_tiles < cap ? s_tiles : cap);
}
static inline size_t lxp_w_bytes(int64_t S, int64_t Nt) { return r256((size_t)S * (size_t)Nt * 8); }
static inline size_t lxp_part_row_bytes(int64_t S, int Q) { return (size_t)lxp_runs(S, Q) * ((size_t)Q * 16 + 4); }   // of one row
static inline size_t lxp_part_bytes(int64_t S, int64_t Nt, int Q) { return r256((size_t)lxp_runs(S, Q) * Nt * Q * 16); }
static inline size_t lxp_cnt_bytes(int64_t S, int64_t Nt, int Q) { return r256((size_t)lxp_runs(S, Q) * Nt * 4); }

hipError_t mile_launch_lxp_rows(const LxpParams &p, hipStream_t st);    // k_lxp_pack + k_lxp_row
hipError_t mile_launch_lxp_apply(const LxpParams &p, hipStream_t st);   // k_lxp_apply + k_lxp_finish

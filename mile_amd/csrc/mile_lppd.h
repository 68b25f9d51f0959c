// Streamed LPPD (mile_lppd_stream): the log posterior predictive density of C chains x S draws on N rows, of each chain, of
// each row, and both as curves over the number of draws, reduced on the device without a [C, S, N] tensor.  Kernels in
// mile_lppd.hip; the entry point (argument checks, the passes over the draws through mile_pointwise_loglik's forward) in
// mile_eval.hip.
//
// State per (chain, row): a streaming log-sum-exp (m, s) -- the running maximum m and s = sum exp(l - m) over the draws
// folded so far -- both fp64, [C][N] pairs of 16 bytes, plus cnt[C][N], the draws folded.  Every figure is written in terms
// of A[c][n] = m + log s; s * exp(m) is never formed.
// The forward writes one pass ll[c][j][n] = log p(y_n | x_n, theta_{c, j0 + j}) of the SAME draw window of every chain; then
//   k_lppd_accum        grid (ceil(N / 64), C): a thread per (chain, row), n the contiguous axis of [C][J][N] so a wave
//                       reads runs of 64 floats, folds draws [ja, jb) of the pass into the state in draw order
//   k_lppd_emit<FINAL>  grid ceil(N / 64), at a curve point or after the last draw: a thread per row walks the chains in index
//                       order; per chain the wave sums A - log cnt over its 64 rows with a fixed shuffle tree (the block
//                       reduction: one wave per workgroup) into part_chain[wave][c]; the row's ensemble term, the
//                       log-sum-exp of A over the chains minus log sum_c cnt, is kept the same streaming way and summed into
//                       part_ens[wave]
//   k_lppd_finish<FINAL>  one workgroup, the second stage: per chain the sum of the waves' partial sums in wave order, then
//                       the chains and the ensemble partial sums through a fixed LDS tree
// The host splits a pass at every curve point, so a point falls exactly on its draw count.  No atomics, every sum in a fixed
// order, and the state carries from pass to pass in fp64 unrounded: the outputs are bitwise the same for every pass size.
//
// NaN rule (that of mile_predict_moments: per draw and per row).  A draw whose log-likelihood on row n is NaN is left out of
// (chain, n) and counted; +inf and -inf take part as values (-inf adds 0 to s).  A (chain, row) with every draw left out
// makes that chain's figures NaN (and with them the chain-averaged curve); the ensemble figures skip that chain on that row,
// and are NaN only where no chain has a draw.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

#define LPPD_NT 64            // one wave per workgroup: its shuffle tree is the block reduction
#define LPPD_FIN_NT 256       // the one workgroup of the second stage
#define LPPD_C_MAX 65535      // chains (gridDim.y of k_lppd_accum)
#define LPPD_J_MAX 65535      // draws of a chain per pass (gridDim.y of the forward kernels)

struct LppdParams {
  const float *ll;     // [C][J][N] pointwise log-likelihoods of this pass
  int C, N, J;         // J: draws per chain the pass holds
  int ja, jb;          // accum: folds draws [ja, jb) of the pass
  int fresh;           // accum: 1 = the call's first launch: start from (m, s) = (-inf, 0), cnt = 0 instead of loading
  long long S;         // draws per chain of the whole call (finish: dropped = S * N - sum cnt)
  double2 *state;      // [C][N] (m, s)
  int32_t *cnt;        // [C][N]
  int waves;           // ceil(N / 64)
  double *part_ens;    // [waves]
  double *part_chain;  // [waves][C]
  long long *part_cnt; // [waves][C] (FINAL only)
  int point;           // index into run_chain / run_ens, -1: no curve point here
  double *run_chain, *run_ens;              // [K] or null
  double *chain_lppd, *row_lppd, *lppd;     // [C], [N], [1] or null (FINAL only)
  long long *dropped;                       // [C] or null (FINAL only)
};

static inline int lppd_waves(long long N) { return (int)((N + LPPD_NT - 1) / LPPD_NT); }
// bytes of the state, the counts and the partial sums: the workspace behind the pass's log-likelihood block
static inline size_t lppd_state_bytes(int C, long long N) {
  const size_t cn = (size_t)C * (size_t)N, w = (size_t)lppd_waves(N);
  return cn * 16 + (cn * 4 + 7) / 8 * 8 + w * 8 + 2 * w * (size_t)C * 8;
}

hipError_t mile_launch_lppd_accum(const LppdParams &p, hipStream_t st);
hipError_t mile_launch_lppd_emit(const LppdParams &p, bool final, hipStream_t st);

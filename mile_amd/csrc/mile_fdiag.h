// Function-space chain diagnostics (mile_function_diagnostics): the statistics of mile_chain_diagnostics, not of the
// parameters but of what each draw PREDICTS on every row -- the head outputs (mu, log sigma, or the softmax probabilities),
// the row's log-likelihood, and the draw's summed log-likelihood L.  Kernels in mile_fdiag.hip; the entry point (argument
// checks, row tiles) in mile_eval.hip.
//
// Columns: with O the width of the last layer and Q = O + (y ? 1 : 0), column m = n * Q + q is quantity q of row n; with y
// there is one last column m = N * Q, the draw's L.  One tile of nt rows goes through
//   forward_draws     every draw on the tile's rows -> the raw block [D][nt][O], D = C * S (mile_predict's launches)
//   k_fdiag_pack      raw block -> plane [p][c][s], p = r * Q + q, through two padded LDS tiles: the read walks whole runs of
//                     the block's rows, the write whole runs of s -- the layout k_diag_pool_rank / k_diag_chain read
//   k_fdiag_lp        one thread per draw: acc[c][s] += the tile's log-likelihoods of the draw, row after row, in fp64
//   k_diag_pool_rank / k_diag_chain / k_diag_final (mile_diag.h) on the tile's P = nt * Q columns, at column offset r0 * Q
// and after the last tile one chunk of P = 1 for L (acc rounded to fp32).  k_fdiag_summary reduces the finished statistic
// arrays in two stages.  No atomics, every sum in a fixed order: the outputs are bitwise reproducible, and since L is summed in
// row order whatever the tiles, they do not depend on the tiling either.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mile_diag.h"

#define FDIAG_O_MAX 64               // head outputs of a row (the softmax runs over them in registers' reach of one thread)
#define FDIAG_DT 32                  // draws per pack tile: one 128-byte run of s
#define FDIAG_IN_MAX 64              // floats of the raw block per draw of a pack tile: ceil(32 / O) rows of O
#define FDIAG_OUT_MAX 80             // columns of a pack tile: ceil(32 / O) * (O + 1) at most
#define FDIAG_P_MAX (1 << 20)        // columns of a tile
#define FDIAG_SUM_NT 256
#define FDIAG_PART_MAX 8192          // stage-1 partials of k_fdiag_summary, over all (series, block)

// layout of `summary` (fp64); indices and counts are whole numbers, -1 where there is no finite cell
enum {
  FDIAG_RHAT_MAX, FDIAG_RHAT_MEAN, FDIAG_RHAT_COLUMN, FDIAG_RHAT_GT_1_01, FDIAG_RHAT_GT_1_05, FDIAG_RHAT_GT_1_1, FDIAG_RHAT_SKIPPED,
  FDIAG_CRHAT_MAX, FDIAG_CRHAT_CHAIN, FDIAG_CRHAT_COLUMN, FDIAG_CRHAT_SKIPPED,
  FDIAG_ESS_MIN, FDIAG_ESS_MEAN, FDIAG_ESS_CHAIN, FDIAG_ESS_COLUMN, FDIAG_ESS_SKIPPED,
  FDIAG_NSUM
};

struct FdiagParams {
  const float *out;       // raw block [D][nt][O]
  const void *y;          // labels of the tile's rows (fp32 / int32 by task), or null
  int D, nt, O, Q, task;
  float *raw;             // plane [nt * Q][D]
  double *acc;            // [D] running L
  float *lcol;            // k_fdiag_lp: where acc goes rounded to fp32 after this launch, or null
};

// what one series (rhat, one chain's crhat, one chain's ess) reduces to over a run of columns
struct FdiagPart {
  double mx, mn, sum;
  long long imx, imn, nfin, nskip, g1, g2, g3;
};

struct FdiagSumParams {
  const float *rhat, *crhat, *ess;   // [M], [C][M], [C][M]
  long long M, NQ;                   // row stride, and the columns the summaries take (the L column is not one)
  int C, B;                          // chains, stage-1 blocks per series
  FdiagPart *part;                   // [2C + 1][B], then [2C + 1] reduced
  double *summary, *chain_summary;   // [FDIAG_NSUM], [C][2] (min ess, max crhat); either may be null
};

static inline int fdiag_pack_rows(int O) { return (FDIAG_DT + O - 1) / O; }
static inline int fdiag_sum_blocks(int C, long long NQ) {
  long long b = (NQ + FDIAG_SUM_NT - 1) / FDIAG_SUM_NT;
  const long long cap = FDIAG_PART_MAX / (2LL * C + 1);
  if (b > cap) b = cap;
  return b < 1 ? 1 : (int)b;
}
static inline size_t fdiag_part_bytes(int C, long long NQ) { return (size_t)(2LL * C + 1) * (fdiag_sum_blocks(C, NQ) + 1) * sizeof(FdiagPart); }

hipError_t mile_launch_fdiag_pack(const FdiagParams &p, hipStream_t st);
hipError_t mile_launch_fdiag_lp(const FdiagParams &p, hipStream_t st);
hipError_t mile_launch_fdiag_summary(const FdiagSumParams &p, hipStream_t st);

// Prediction sets and calibration of the classification ensemble (mile_calibration, mile_calibration_stream): from the logits
// of C chains x S draws on N rows, for every chain and for the ensemble of all chains, the mean class probabilities, the
// classes in descending order of probability, the highest-probability set at each coverage level, the rank of the true
// label, the Brier score, the NLL, the accuracy and the reliability bins.  include/mile_hip.h states the definition.  Kernels
// in mile_calib.hip; the entry points (argument checks, the row tiles and the passes over the draws through mile_predict's
// forward) in mile_eval.hip.
//
// One tile of Nt rows goes through these launches:
//   k_cal_accum   grid (ceil(Nt / 64), C), once per pass of J draws: a thread per (chain, row) along the contiguous row axis
//                 of the pass's logits walks the chain's draws in draw order; per kept draw e_k = exp(z_k - max z), their sum
//                 in class order, p_k = e_k / sum, and p_k is added to the chain's fp64 sums sum [C][Nt][K], which live in
//                 device memory across passes (with the kept counts cnt [C][Nt]).  CAL_KC classes are held in registers at a
//                 time; K > CAL_KC takes further trips over the pass, each with the same sum of e_k in the same order.
//   k_cal_rows    one wave64 per (group, row), a class per lane (K <= 64), after the last pass.  P = sum / kept for a chain,
//                 (the chain sums added in chain order) / (the counts added) for the ensemble.  The position of class k in the
//                 order is the number of classes j with P_j > P_k, or P_j == P_k and j < k, counted over the lanes by shuffles;
//                 P goes to LDS in class order and in that order, lane q then walks the serial cumulative sum for coverage
//                 q, and every lane the serial Brier sum.  Writes probs, kept, (ensemble) order, set_size, rank, and one
//                 record per (group, row) for the reduction: brier, nll, conf, rank, the Q sizes.
//   k_cal_part    a thread per (group, block of B rows, column of the totals-and-bins row): adds the tile's rows of the block
//                 to the block's partial sum in row order, starting from what earlier tiles left there -- so a block cut by
//                 a tile boundary sums exactly as an uncut one.  B depends on (N, G, Q, n_bins) alone.
// and after the last tile
//   k_cal_final   a thread per (group, column): the blocks' partial sums in block order -> totals, bins.
// fp64 throughout, fixed order, no floating-point atomics; counts are sums of 0.0 / 1.0 and exact below 2^53.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mile_hip.h"
#include "mile_eval_plan.h"

#define CAL_NT 64          // k_cal_accum workgroup: one wave
#define CAL_KC 16          // classes whose sums a thread of k_cal_accum holds in registers at a time
#define CAL_K_MAX 64       // a class per lane in k_cal_rows
#define CAL_Q_MAX 16
#define CAL_BINS_MAX 64
#define CAL_ROWS_NW 4      // waves (rows) per workgroup of k_cal_rows
#define CAL_BLOCK 256      // rows per reduction block, doubled while the partial sums exceed CAL_PART_TARGET
#define CAL_PART_TARGET ((size_t)64 << 20)

struct CalRec {            // what the reduction needs of one (group, row)
  double brier, nll, conf;
  int32_t rank;            // -1: not counted (nothing kept); 0: label outside [0, K); else the 1-based rank
  uint8_t size[CAL_Q_MAX];
  int32_t pad;
};

struct CalParams {
  // k_cal_accum: logit k of draw j of chain c on tile row n is raw[((c * cs + j) * ld + n) * K + k]
  const float *raw;
  long long cs, ld;
  int J;                   // draws of this pass
  int C, K, Nt, Q, n_bins;
  long long N, r0;         // rows of the call, first row of the tile
  double *sum;             // [C][Nt][K]
  int32_t *cnt;            // [C][Nt]
  const int32_t *y;        // [N] or null
  double cov[CAL_Q_MAX];
  CalRec *rec;             // [G][Nt] (with y)
  double *part;            // [G][nblk][W], W = 5 + 2 Q + 3 n_bins (with y)
  long long B, nblk;
  // outputs at row 0 of the call, each may be null
  double *probs; int32_t *kept, *order, *set_size, *rank;
  double *totals, *bins;
};

__host__ __device__ static inline int cal_cols(int Q, int n_bins) { return 5 + 2 * Q + 3 * n_bins; }
// rows per reduction block: a function of the call's shape alone, never of its tiling
static inline int64_t cal_block_rows(int64_t N, int G, int W) {
  int64_t B = CAL_BLOCK;
  while (B < N && (size_t)G * (size_t)((N + B - 1) / B) * W * 8 > CAL_PART_TARGET) B *= 2;
  return B;
}
static inline size_t cal_part_bytes(int64_t N, int G, int W) {
  const int64_t B = cal_block_rows(N, G, W);
  return r256((size_t)G * (size_t)((N + B - 1) / B) * W * 8);
}
// per tile row: the chains' sums and counts, and the groups' records
static inline size_t cal_row_bytes(int C, int K) { return (size_t)C * ((size_t)K * 8 + 4) + (size_t)(C + 1) * sizeof(CalRec); }
static inline size_t cal_sum_bytes(int C, int K, int64_t Nt) { return r256((size_t)C * Nt * K * 8); }
static inline size_t cal_cnt_bytes(int C, int64_t Nt) { return r256((size_t)C * Nt * 4); }
static inline size_t cal_rec_bytes(int C, int64_t Nt) { return r256((size_t)(C + 1) * Nt * sizeof(CalRec)); }

hipError_t mile_launch_cal_accum(const CalParams &p, hipStream_t st);
hipError_t mile_launch_cal_rows(const CalParams &p, hipStream_t st);    // k_cal_rows, then (with y) k_cal_part
hipError_t mile_launch_cal_final(const CalParams &p, hipStream_t st);

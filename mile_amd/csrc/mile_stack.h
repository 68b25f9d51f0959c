// Stacking of non-mixing chains (mile_stack_eval): the score of the weighted mixture of the chains' pointwise predictive
// densities, its gradient in the weights and the Gram matrix of the responsibilities (the negative Hessian), from
// lpd [C, N] fp64 and w [C] fp64 (Yao, Vehtari, Simpson & Gelman 2018).  include/mile_hip.h states the definition.  Kernels in
// mile_stack.hip; the entry point (argument checks, the row tiles) in mile_eval.hip.
//
// The responsibilities of a tile of Nt rows are written as Rx [Cx][Nt] fp64, Cx = C + 2: rows 0 .. C-1 hold R_cn, row C holds
// 1 for a used row and row C + 1 its row_score; a row left out holds 0 in all of them.  Every sum over the rows is then an
// entry of Rx Rx^T:  sum_n R_an R_bn = G[a][b],  sum_n R_cn = G[C][c],  sum_n row_score_n = G[C+1][C],  used = G[C][C]
// (a product with 1 is exact, and so is a count below 2^53), and one kernel takes them all.
//   k_stk_rows   a thread per row: the max over the chains, the mixture in chain order, row_score, and the column of Rx.
//   k_stk_gram   grid (lower-triangle pairs of 64 x 64 output tiles, row blocks of the tile): a workgroup of 256 threads, a
//                4 x 4 register block of fp64 accumulators each, walks its block's rows 16 at a time through LDS; every entry
//                is one chain of fma over the rows in row order.  A block that a row tile cuts is carried: the workgroup
//                starts from the block's partial sum where its rows do not begin the block, so the chain of fma is the same
//                for every tile size, bit for bit.  Calls that ask for no Hessian launch only the pairs that hold row C
//                (and without the gradient, the pairs that hold [C][C] and [C+1][C]).
//   k_stk_final  the blocks' partial sums in block order, divided by `used`; the lower triangle is mirrored.
// The Gram product runs on the VALU: gfx950's fp64 matrix and vector peaks are the same, and v_mfma_f64_16x16x4 sums four rows
// inside the instruction, which a tile boundary that is no multiple of four would cut differently.
// B rows per block, a function of C and N alone: the blocks' partials [nb][Cx][Cx] stay within 64 MiB and nb <= 1024.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mile_eval_plan.h"

#define STK_NT 256               // every kernel's workgroup
#define STK_TILE 64              // chains of an output tile's side
#define STK_K 16                 // rows of a step through LDS
#define STK_MAX_C 1024
#define STK_MAX_BLOCKS 1024
#define STK_PART_BYTES ((int64_t)64 << 20)
#define STK_R_BYTES ((int64_t)256 << 20)

struct StkParams {
  const double *lpd;       // [C][N]
  const double *w;         // [C]
  int C, Cx;               // Cx = C + 2
  long long N;
  long long r0;            // the tile's first row
  int Nt;                  // rows of this tile
  long long ldR;           // rows the tile buffer holds per chain (the full tile's Nt)
  long long B;             // rows per block
  int nb;                  // blocks of the call
  double *Rx;              // [Cx][ldR]
  double *part;            // [nb][Cx][Cx]
  int want_grad, want_hess, want_sums;   // want_sums: anything beyond row_score
  double *score, *row_score, *grad, *hess;
  long long *used;
};

// rows per block: at most STK_MAX_BLOCKS blocks whose partials fit STK_PART_BYTES, a multiple of 32 rows
static inline int64_t stk_block_rows(int64_t C, int64_t N) {
  const int64_t Cx = C + 2;
  int64_t nb_max = STK_PART_BYTES / (8 * Cx * Cx);
  if (nb_max > STK_MAX_BLOCKS) nb_max = STK_MAX_BLOCKS;
  if (nb_max < 1) nb_max = 1;
  const int64_t b = (N + nb_max - 1) / nb_max;
  return (b + 31) / 32 * 32;
}
static inline int64_t stk_blocks(int64_t C, int64_t N) {
  const int64_t B = stk_block_rows(C, N);
  return (N + B - 1) / B;
}
// rows per tile: Rx [C + 2][Nt] fp64 within STK_R_BYTES; max_rows > 0 caps it
static inline int64_t stk_tile_rows(int64_t C, int64_t N, int64_t max_rows) {
  int64_t nt = STK_R_BYTES / (8 * (C + 2));
  if (max_rows > 0 && nt > max_rows) nt = max_rows;
  return nt < N ? nt : N;
}
static inline size_t stk_rx_bytes(int64_t C, int64_t Nt) { return r256((size_t)(C + 2) * (size_t)Nt * 8); }
static inline size_t stk_part_bytes(int64_t C, int64_t N) { return r256((size_t)stk_blocks(C, N) * (size_t)(C + 2) * (size_t)(C + 2) * 8); }
// what is wrong with the shape or the outputs asked for, or null
static inline const char *stk_bad_args(int64_t C, int64_t N, int64_t max_rows, bool any_output) {
  if (C < 1 || C > STK_MAX_C) return "C out of range (1 .. 1024)";
  if (N < 1 || N > 0x3fffffff) return "N out of range (1 .. 2^30 - 1)";
  if (max_rows < 0) return "max_rows_per_tile < 0";
  if (!any_output) return "no output asked for";
  return nullptr;
}

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
hipError_t mile_launch_stack_tile(const StkParams &p, hipStream_t st);    // k_stk_rows, then k_stk_gram if want_sums
hipError_t mile_launch_stack_final(const StkParams &p, hipStream_t st);   // k_stk_final (want_sums)
#endif

// Exact predictive quantiles and PIT of the ensemble (mile_mixture_quantiles, mile_predict_quantiles): the equal-weight
// mixture of the S draws' Normals on every row, F_n(t) = mean_s Phi((t - mu_sn) / sigma_sn), inverted at Q levels and
// evaluated at y_n.  Kernels in mile_quantiles.hip; the entry points (argument checks, the row tiles and the passes over the
// draws through mile_predict's forward) in mile_eval.hip.
//
// One tile of Nt rows goes through two launches:
//   k_qnt_pack   grid (ceil(Nt / 32), slices): raw [S][ld][2] -> pk [Nt][S] pairs, contiguous per row, through a 32 x 32 LDS
//                tile (both sides coalesced).  A pair is (mu, log sigma) as it came, fp32, or (NaN, NaN) for a draw left out
//                of the row (weight 0): sigma = clip(exp(log sigma)) is formed in fp64 where it is used, because an fp32
//                sigma would cost up to z_p * 2^-24 * sigma of a quantile, half of what the output's own rounding allows.
//                Each slice of the draw axis also records, per row, its kept count and per level min_s and max_s of
//                mu_s + z_p sigma_s: F <= p at the minimum and F >= p at the maximum, the exact bracket of the root.
//   k_qnt_solve  one workgroup per row.  The slices' counts and brackets merge first (integer sums, min and max: the same for
//                every slicing).  A lane holds ONE level q and one component in 64 / Q: wave w, lane c * Q + q walks
//                components w * (64 / Q) + c, + 4 * (64 / Q), ...  A sweep sums Phi (through fp64 erfc) and the density for
//                every level at once; the lanes of a level add up inside the wave in component order (shuffles), the four
//                waves through LDS in wave order.  Every lane of a level keeps the same (lo, hi, t) and takes the same step:
//                Newton, pushed a quarter of the stopping width past its target so that a converged iterate crosses the root
//                and closes the bracket; bisection when the step leaves the bracket, the density is 0 or the step is more
//                than half the one before.  The loop is uniform: it ends when every level's bracket is below
//                2^-25 max(|mid|, sd_n) or after QNT_MAX_SWEEPS.  PIT is one more sweep at y_n over all lanes.
//                <true>: the row's S pairs are loaded into LDS once (S <= QNT_LDS_MAX_S); <false>: every sweep streams them
//                from global memory.
// fp64 sums, fixed order, no atomics: a row's result depends on its S pairs alone, bit for bit.
//
// The chain-weighted form (mile_mixture_quantiles_weighted, mile_predict_quantiles_weighted; QntWParams and
// mile_launch_quantiles_weighted): the S = C * Sc pairs of a row are C chains of Sc draws, chain c with weight w_c, and
// F_n(t) = sum_c (w_c / K_c) sum_{i in c, kept} Phi((t - mu_i) / sigma_i).  k_qnt_pack runs as above with no level (its counts and
// brackets are not read).  k_qnt_solve<., QntWParams> first counts K_c per chain (whole waves by ballot, integer adds in LDS),
// writes dropped [C][N] and a table omega_c = w_c / K_c in LDS (0 for w_c = 0: such a chain enters no sum, the bracket
// included; w_c > 0 with K_c = 0: the row is NaN), takes the bracket min_i and max_i of mu_i + z_p sigma_i over the components
// with omega > 0 in the sweep's own lane layout, and multiplies omega[chain(i)] into Phi and the density of every sweep, into
// the mean and sd_n of the first iterate and into the PIT sum.  Same summation orders as above; a row's result depends on its
// pairs and the weights alone, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"
#include "mile_eval_plan.h"

#define QNT_MAX_Q 32
#define QNT_NT 256                // solve workgroup: four waves
#define QNT_NW (QNT_NT / 64)
#define QNT_TILE 32               // rows and draws of a transpose tile
#define QNT_MAX_SLICES 64         // slices of the draw axis in k_qnt_pack (gridDim.y)
#define QNT_LDS_MAX_S 16384       // pairs a row keeps in LDS: 128 KiB of the CU's 160 KiB, beside 2.3 KiB of reduction scratch
#define QNT_MAX_SWEEPS 200        // hard cap; bisection alone needs 25 + log2(bracket / sd_n) <= 25 + log2(4 sqrt(S)) sweeps

struct QntParams {
  const float *raw;        // [S][ld][2], at the tile's first row
  long long ld;            // rows per draw in raw
  int S, Nt, Q, slices;
  const double *lev;       // device: [Q] levels, then [Q] z_p = Phi^-1(p)
  float2 *pk;              // [Nt][S]
  double *part_brk;        // [slices][Nt][Q][2]
  int32_t *part_cnt;       // [slices][Nt]
  const float *y;          // [Nt] at the tile's first row, or null
  float *quant;            // [Nt][Q], or null
  float *pit;              // [Nt], or null
  int32_t *dropped;        // [Nt], or null
  int32_t *sweeps;         // [Nt], or null
};

// the chain-weighted form: S = C * Sc, chain c's draws at pairs c * Sc .. of a row
#define QNT_MAX_C 1024
struct QntWParams : QntParams {
  const double *w;         // device: [C] weights, >= 0, summing to 1
  int C, Sc;
  int32_t *dropped_c;      // [C][N] at the tile's first row, or null
  long long N;             // rows per chain in dropped_c
};

static inline int qnt_slices(int S, int Nt, int n_cu) {   // about two workgroups per CU, whole transpose tiles per slice
  const int row_groups = (Nt + QNT_TILE - 1) / QNT_TILE, s_tiles = (S + QNT_TILE - 1) / QNT_TILE;
  int sl = (2 * n_cu + row_groups - 1) / row_groups;
  if (sl > QNT_MAX_SLICES) sl = QNT_MAX_SLICES;
  if (sl > s_tiles) sl = s_tiles;
  return sl < 1 ? 1 : sl;
}
// bytes behind the raw block: the packed copy, the slices' brackets and counts (each rounded up to 256)
static inline size_t qnt_pk_bytes(int64_t S, int64_t Nt) { return r256((size_t)S * (size_t)Nt * 8); }
static inline size_t qnt_part_bytes(int Nt, int Q, int slices) {
  return r256((size_t)slices * Nt * Q * 16) + r256((size_t)slices * Nt * 4);
}

hipError_t mile_launch_quantiles(const QntParams &p, hipStream_t st);
hipError_t mile_launch_quantiles_weighted(const QntWParams &p, hipStream_t st);

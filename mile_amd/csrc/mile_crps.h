// Exact CRPS of the predictive mixture, per chain and chain-weighted (mile_mixture_crps, mile_crps_stream).  On one row the
// draws i of chain c are Normals (mu_i, sigma_i^2); with A(d, v) = E|N(d, v)| = d erf(d / sqrt(2v)) + sqrt(2v / pi) exp(-d^2 / 2v)
//   a_c   = mean_i A(y - mu_i, sigma_i^2)                               G_cc' = mean_{i in c, j in c'} A(mu_i - mu_j, sigma_i^2 + sigma_j^2)
//   crps_chain[c] = a_c - G_cc / 2                                       crps_mix(w) = sum_c w_c a_c - w'Gw / 2
// Kernels in mile_crps.hip; the entry points (argument checks, row tiles, the forward passes) in mile_eval.hip.
//
// One tile of Nt rows goes through three launches:
//   k_crps_pack    grid (ceil(Nt / 32), C): raw [C * S][ld][2] -> pk [Nt][C][S] pairs (mu, sigma^2), a chain's kept draws of a row
//                  contiguous and in draw order (32 x 32 LDS transpose, then a ballot prefix per row); cnt [Nt][C] = K_c and
//                  dropped [C, N] = S - K_c.  sigma = clip(expf(log sigma), 1e-6, 1e6) in fp32 as in mile_pointwise_loglik.
//   k_crps_pairs   the hot path, VALU and transcendental bound.  One workgroup per (row, chain block c <= c', i-tile, j-split):
//                  a thread keeps CRPS_R i-draws of chain c in registers (i-tile: CRPS_TI = 1024 draws), the j-draws of chain
//                  c' pass through LDS in tiles of CRPS_TJ = 256 and are read as broadcasts, one read for CRPS_R pair terms.
//                  A block c = c' visits only j-tiles at or above its i-tile: pairs j > i count twice, j = i once, j < i not;
//                  the mask costs its selects only in the (at most four) j-tiles that overlap the i-tile.  Pair terms are fp32
//                  (A = |d| + s g(|d| / s), g one approximation in place of erff + expf: crps_A); a thread sums runs of at
//                  most CRPS_RUN = 32 terms in fp32 and the runs in fp64, the workgroup's 256 sums meet in a fixed order, and
//                  the result goes to the unit's slot:
//                  no atomics.  The j-tiles of an i-tile are split over n_js workgroups by crps_plan, a function of (C, S, N)
//                  alone -- not of the row tile, the pass size or the device -- so the bits of a row depend on its draws alone.
//   k_crps_finish  one workgroup per row: a_c in fp64, G_cc' = (its slots, in slot order) / (K_c K_c'), written over the block's
//                  first slot and, mirrored, to gram; the chains' own outputs; then the pooled weights K_c / sum K and the
//                  caller's weight vectors contract a and G (a chain of weight 0 is skipped, so an empty chain spoils only
//                  mixtures that use it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"
#include "mile_eval_plan.h"

#define CRPS_NT 256                       // workgroup of every kernel: four waves
#define CRPS_R 4                          // i-draws a thread of k_crps_pairs keeps
#define CRPS_TI (CRPS_NT * CRPS_R)        // draws of an i-tile
#define CRPS_TJ 256                       // draws of a j-tile in LDS
#define CRPS_RUN 32                       // pair terms summed in fp32 before the sum goes to fp64
#define CRPS_TILE 32                      // rows and draws of k_crps_pack's transpose tile
#define CRPS_MAX_W 8                      // caller weight vectors
#define CRPS_MAX_C 1024
#define CRPS_MAX_DRAWS (1 << 20)          // C * S
#define CRPS_TARGET_WG 2048               // workgroups of k_crps_pairs that crps_plan aims at over all N rows: 8 per CU of 256
// Pairs (i <= j over all C * S draws, times rows) one launch of k_crps_pairs may get; the row tile shrinks to respect it, and
// a single row is the least a launch can take.  The largest power of two that the measured 1.08e12 pairs / s (tools/crps_time.py,
// DESIGN 3.2s) finishes within 0.25 s: 2^37 pairs take 0.13 s.
#define CRPS_MAX_PAIRS_PER_LAUNCH (1ll << 37)
#define CRPS_MAX_SLOT_BYTES (256ll << 20) // of the slots of one tile
#define CRPS_MAX_GRID (1ll << 30)         // workgroups of one launch

struct CrpsPlan {
  int n_it, n_jt, n_js;      // i-tiles and j-tiles of a chain, workgroups that share an i-tile's j-tiles
  long long n_blocks;        // C (C + 1) / 2 chain blocks c <= c'
  int upb;                   // units (slots) per chain block: n_it * n_js
  long long units;           // per row
};
static inline CrpsPlan crps_plan(int64_t C, int64_t S, int64_t N) {
  CrpsPlan pl;
  pl.n_it = (int)((S + CRPS_TI - 1) / CRPS_TI);
  pl.n_jt = (int)((S + CRPS_TJ - 1) / CRPS_TJ);
  pl.n_blocks = C * (C + 1) / 2;
  const long long base = pl.n_blocks * pl.n_it * N;
  long long js = (CRPS_TARGET_WG + base - 1) / base;
  if (js > pl.n_jt) js = pl.n_jt;
  pl.n_js = js < 1 ? 1 : (int)js;
  pl.upb = pl.n_it * pl.n_js;
  pl.units = pl.n_blocks * pl.upb;
  return pl;
}

struct CrpsParams {
  const float *raw;          // [C * S][ld][2], at the tile's first row
  long long ld;              // rows per draw in raw
  int C, S, Nt;
  CrpsPlan pl;
  float2 *pk;                // [Nt][C][S]
  int32_t *cnt;              // [Nt][C]
  double *part;              // [Nt][units]
  const float *y;            // [Nt] at the tile's first row
  const double *w;           // device [n_w][C], or null
  int n_w;
  long long N, r0;           // the outputs' row count and the tile's first row in them
  double *crps_chain, *spread_chain;   // [C, N], or null
  double *crps_mix, *spread_mix;       // [1 + n_w, N], or null
  double *gram;                        // [N, C, C], or null
  int32_t *dropped;                    // [C, N], or null
};

hipError_t mile_launch_crps_pack(const CrpsParams &p, hipStream_t st);
hipError_t mile_launch_crps_pairs(const CrpsParams &p, hipStream_t st);
hipError_t mile_launch_crps_finish(const CrpsParams &p, hipStream_t st);

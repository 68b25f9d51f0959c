// PSIS-LOO and WAIC of the ensemble on the rows the sampler conditioned on (mile_psis_loo, mile_loo_stream): per row n, from
// the S pointwise log-likelihoods l_s = log p(y_n | x_n, theta_s), the log pointwise predictive density, the WAIC penalty,
// the Pareto-smoothed importance-sampling leave-one-out density and the Pareto shape khat of its weights (Vehtari, Gelman &
// Gabry 2017; Vehtari et al. 2024; the fit of Zhang & Stephens 2009).  include/mile_hip.h states the definition.  Kernels in
// mile_loo.hip; the entry points (argument checks, the row tiles and the passes over the draws through
// mile_pointwise_loglik's forward) in mile_eval.hip.
//
// One tile of Nt rows goes through two launches:
//   k_loo_pack  grid (ceil(Nt / 32), slices): ll [S][ld] -> pk [Nt][S], contiguous per row, through a 32 x 32 LDS tile (both
//               sides coalesced).  A value is the fp32 log-likelihood as it came, or NaN for a draw left out of the row (NaN
//               and +-inf alike).  The kept count is not taken here: it falls out of k_loo_row's first pass over the row.
//   k_loo_row   one workgroup of four waves per row, everything in fp64 from the fp32 values.
//               1. one pass: kept count, min, Welford mean and M2, streaming log-sum-exp per thread (elements tid, tid + 256,
//                  ...), merged with Chan's formula down the wave by shuffles and over the waves in index order
//                  -> dropped, lppd, p_waic.  Calls that ask for neither elpd_loo nor khat end here.
//               2. the ratios are r = -l - max(-l), so the M largest r are the M smallest l: the (M+1)-th smallest l is found
//                  by a radix select on the order-preserving 32-bit image of the float, 8 bits a pass, four passes, each a
//                  256-bin LDS histogram (integer LDS atomics: counts, the same in any order) scanned by one thread.
//               3. the keys below the selected one are gathered into LDS (slots from an integer LDS counter; the order they
//                  land in does not matter, they are sorted next), copies of the selected key fill the tail up to M (ties at
//                  the boundary all hold the same bits), +max pads to a power of two, and an LDS bitonic network sorts them.
//               4. x_i = exp(r_(i)) - exp(cut) to LDS in fp64; the m = 30 + floor(sqrt(M)) candidate means of log1p(-b_j x)
//                  go a wave per candidate, a lane per 64th of the tail, summed by an xor butterfly.
//               5. the candidates' weights (thread j: sum_i exp(L_i - L_j) in index order), b, then k, sigma and khat by a
//                  workgroup sum; the smoothed tail min(log(sigma expm1(-khat log1p(-p_i)) / khat + exp(cut)), 0) replaces
//                  x in LDS (without a fit: r itself).
//               6. a second pass over the body (keys above the selected one, plus the copies of it the tail did not take) and
//                  the tail from LDS: sum exp(lw - max lw) and sum exp(lw + l - max(lw + l)) -> elpd_loo.
//               <true>: the row's S values stay in LDS (S <= LOO_LDS_MAX_S); <false>: every pass streams them from the
//               packed copy.
// LDS of k_loo_row, of the CU's 160 KiB: the row, at most 64 KiB (dynamic); the tail's keys 16 KiB and its x / lw 32 KiB; the
// histogram, the candidates and the reduction scratch 3.5 KiB.
// fp64 sums, fixed order, no floating-point atomics: a row's result depends on its S values alone, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mile_hip.h"
#include "mile_eval_plan.h"

#define LOO_NT 256                // k_loo_row workgroup: four waves
#define LOO_NW (LOO_NT / 64)
#define LOO_TILE 32               // rows and draws of a transpose tile
#define LOO_MAX_SLICES 64         // slices of the draw axis in k_loo_pack (gridDim.y)
#define LOO_LDS_MAX_S 16384       // values a row keeps in LDS: 64 KiB
#define LOO_MAX_S (1 << 20)
#define LOO_MAX_TAIL 4096         // tail values sorted in LDS; M <= 3072 at r_eff >= 1, and a call whose M(S) is above this is refused
#define LOO_MAX_CAND 96           // m = 30 + floor(sqrt(M)) <= 94

struct LooParams {
  const float *ll;         // [S][ld], at the tile's first row
  long long ld;            // rows per draw in ll
  int S, Nt, slices;
  float *pk;               // [Nt][S]
  double r_eff;
  int M_full;              // the tail length of a row that keeps all S draws, from the host
  double *lppd, *p_waic, *elpd_loo, *khat;   // [Nt] at the tile's first row, each may be null
  int32_t *dropped;        // [Nt], or null
};

// M = ceil(fmin(S_n / 5.0, 3.0 * sqrt(S_n / r_eff))), the same expression on the host and on the device
static inline int loo_tail_host(int64_t Sn, double r_eff) { return (int)ceil(fmin((double)Sn / 5.0, 3.0 * sqrt((double)Sn / r_eff))); }

static inline int loo_slices(int S, int Nt, int n_cu) {   // about two workgroups per CU, whole transpose tiles per slice
  const int row_groups = (Nt + LOO_TILE - 1) / LOO_TILE, s_tiles = (S + LOO_TILE - 1) / LOO_TILE;
  int sl = (2 * n_cu + row_groups - 1) / row_groups;
  if (sl > LOO_MAX_SLICES) sl = LOO_MAX_SLICES;
  if (sl > s_tiles) sl = s_tiles;
  return sl < 1 ? 1 : sl;
}
static inline size_t loo_pk_bytes(int64_t S, int64_t Nt) { return r256((size_t)S * (size_t)Nt * 4); }

hipError_t mile_launch_loo(const LooParams &p, hipStream_t st);

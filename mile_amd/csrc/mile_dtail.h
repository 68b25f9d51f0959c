// Tail diagnostics of the ensemble (mile_chain_diagnostics_tail, mile_multichain_ess): the multi-chain ESS of the pooled
// normal scores (bulk), of the two tail indicators and of the raw draws (with the MCSE of the mean), and the split R-hat of
// the draws folded about their pooled median.  The definitions are stated once, in include/mile_hip.h.  Kernels in
// mile_dtail.hip; the entry points (argument checks, parameter chunks) in mile_eval.hip.
//
// One chunk of P parameters on the [p][c][s] plane:
//   k_diag_transpose  (mile_diag.h) [C][S][d] -> x[p][c][s]                    (skipped with MILE_DTAIL_PLANE_INPUT)
//   k_dtail_derive    one workgroup per parameter, C*S <= DIAG_POOL_MAX: the pooled LDS sort of k_diag_pool_rank once ->
//                     q_lo, q_hi, m32 and the score plane z (k_diag_pool_rank's bits); then the keys of |x - m32| sorted
//                     -> the folded score plane zf
//   k_dtail_ess       one workgroup per (parameter, series): z, (x <= q_lo), (x <= q_hi), x.  Piece means and their
//                     variance in fp64, then lag blocks of 64 by direct summation over all pieces -- a piece at a time
//                     staged centred in LDS -- with Geyer's stop voted after each block, and one lane for the Geyer tail
//   k_diag_chain / k_diag_final (mile_diag.h) on zf as MILE_DIAG_RHAT | MILE_DIAG_POOLED_INPUT -> rhat_folded
//   k_dtail_final     one thread per parameter: the four ESS and the sd -> ess_bulk, ess_tail, ess_mean, mcse_mean
// No atomics, every sum in a fixed order: the outputs are bitwise reproducible and do not depend on the chunks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"
#include "mile_diag.h"

#define DTAIL_ESS_NT 256
#define DTAIL_NSER 4                 // series of k_dtail_ess: 0 z, 1 (x <= q_lo), 2 (x <= q_hi), 3 x
#define DTAIL_NRES 5                 // per parameter, fp64: the four ESS, then the ddof-1 sd of the pooled draws

struct DtailParams {
  const float *x;         // [P][C][S] the chunk's draws
  float *z, *zf;          // [P][C][S] pooled normal scores of x and of |x - m32| (null where k_dtail_derive is not run)
  float *thr;             // [P][2] q_lo, q_hi
  double *res;            // [P][DTAIL_NRES]
  int C, S, n_splits, P;
  long long d, p0;        // the outputs' row length and the chunk's first parameter
  unsigned series;        // bit i: series i runs in k_dtail_ess
  int want_zf;            // k_dtail_derive folds and ranks a second time
  float *quantiles;       // [3][d] q_lo, q_hi, m32 (or null)
  float *ess_bulk, *ess_tail, *ess_mean, *mcse_mean;   // [d], null where not asked for
  float *ess_plain;       // mile_multichain_ess: series 3 alone, its ESS straight to ess_plain[p0 + q]
};

#define DTAIL_STAGE 4096             // draws staged in LDS at a time by k_dtail_ess: whole pieces, at least one
// LDS of k_dtail_ess: the staged pieces and the autocovariances in fp64, 8 + 256 partial sums
static inline size_t dtail_ess_lds(int len) { return ((size_t)DTAIL_STAGE + len + 8 + 256) * 8; }

hipError_t mile_launch_dtail_derive(const DtailParams &p, hipStream_t st);
hipError_t mile_launch_dtail_ess(const DtailParams &p, hipStream_t st);
hipError_t mile_launch_dtail_final(const DtailParams &p, hipStream_t st);

// Chain diagnostics (mile_chain_diagnostics): within / between chain variance, rank-normalised per-chain ESS, per-chain
// split R-hat and the pooled split R-hat of draws [C][S][d].  Kernels in mile_diag.hip; the entry point (argument checks,
// parameter chunks) in mile_eval.hip.
//
// One chunk of P parameters goes through four launches:
//   k_diag_transpose  [C][S][d] -> [p][c][s] through a 32 x 32 LDS tile (both sides coalesced)
//   k_diag_pool_rank  one workgroup per parameter: bitonic sort of the C*S (key, index) pairs in LDS, average ranks,
//                     normal scores -> z[p][c][s]                (skipped when the input already holds pooled scores)
//   k_diag_chain      one workgroup per (parameter, chain): raw moments, within-chain ranks -> crhat, the split moments
//                     of the pooled scores, direct-summation autocovariance with Geyer's stop -> ess
//   k_diag_final      one thread per parameter: wcv, bcv, rhat from the per-chain moments, chains in index order
// No atomics, every sum in a fixed order: the outputs are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

#define DIAG_S_MIN 4
#define DIAG_S_MAX 4096
#define DIAG_C_MAX 65535
#define DIAG_POOL_MAX 16384          // pooled (key, index) pairs sorted in LDS: 8 B each, 128 KB of the CU's 160 KB
#define DIAG_TILE 32                 // parameters per transpose tile
#define DIAG_NSTAT 5                 // per (parameter, chain): raw mean, raw var, and of the pooled scores: sum of the
                                     // split variances, chain mean, sum of squares of the split means about it
#define DIAG_CHAIN_NT 256
#define DIAG_POOL_NT 1024

struct DiagParams {
  const float *samples;   // [C][S][d]; null: raw (z with MILE_DIAG_POOLED_INPUT) already holds the chunk, no k_diag_transpose
  int C, S, n_splits;
  long long d;
  long long p0;           // first parameter of this chunk
  int P;                  // parameters in this chunk
  unsigned what;
  float *raw;             // workspace [P][C][S] raw draws (null with MILE_DIAG_POOLED_INPUT)
  float *z;               // workspace [P][C][S] pooled normal scores
  double *stat;           // workspace [P][C][DIAG_NSTAT]
  float *wcv, *bcv, *ess, *crhat, *rhat;
};

static inline int diag_pow2(int n) { int m = 1; while (m < n) m <<= 1; return m; }
// workspace bytes of one parameter, and the LDS of the two sorting kernels
static inline long long diag_param_bytes(int C, int S, unsigned what) {
  const long long cs = (long long)C * S * 4;
  return ((what & MILE_DIAG_POOLED_INPUT) ? cs : 2 * cs) + (long long)C * DIAG_NSTAT * 8;
}
static inline size_t diag_chain_lds(int S) { return (size_t)((S * 4 + 15) / 16 * 16) + (size_t)diag_pow2(S) * 16 + (8 + 256) * 8; }
static inline size_t diag_pool_lds(int n) { return (size_t)diag_pow2(n) * 8; }

hipError_t mile_launch_diag(const DiagParams &p, hipStream_t st);
// k_diag_transpose alone: the chunk's [C][S][d] columns into p.raw (p.z with MILE_DIAG_POOLED_INPUT), for mile_dtail.h
hipError_t mile_launch_diag_transpose(const DiagParams &p, hipStream_t st);

// Posterior-predictive moments (mile_predict_moments): the Bayesian-model-average prediction of S draws on N rows, reduced
// over the draw axis on the device.  Kernels in mile_moments.hip; the entry point (argument checks, the passes over the
// draws through mile_predict's forward) in mile_eval.hip.
//
// The forward writes one pass of raw outputs [Sc][N][O] into the library's workspace; then
//   k_moments_accum<TASK>   grid (ceil(N / 64), slices): a thread per row n (the contiguous axis of [Sc][N][O], so a wave reads
//                           one run of 64 * O floats per draw) walks its slice of the pass's draws and folds them into the
//                           slice's accumulators, which live in device memory across passes
//   k_moments_finish<TASK>  a thread per row, after the last pass: merges the slices in index order and writes out[n][W]
// Regression keeps Welford's (count, mean, M2) of mu and a running sum of sigma^2; two partial results -- the pass just
// walked and what the slice held before, and in finish the slices -- merge with Chan's formula.  Classification keeps
// sums of the softmax probabilities and of each draw's entropy.  Every accumulator is fp64, no atomics, every sum in a
// fixed order: the outputs are bitwise reproducible for one (S, N, max_draws_per_pass).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

#define MOM_NT 64            // one wave per workgroup: at N = 301 the grid is 5 x slices workgroups, spread over the CUs
#define MOM_KC 16            // classes whose probability sums a thread holds in registers at a time
#define MOM_MAX_SLICES 256   // slices of the draw loop (gridDim.y)

struct MomParams {
  const float *raw;    // [Sc][N][O] raw outputs of this pass
  int Sc, N, O, slices;
  long long S;         // draws of the whole call (finish: dropped = S - kept)
  double *acc;         // [slices][A][N]; regression A = 3: mean, M2, sum sigma^2; classification A = O + 1: sum p_k, sum H
  int32_t *cnt;        // [slices][N] draws kept so far
  float *out;          // [N][W]
  int32_t *dropped;    // [N], or null
};

// accumulator planes per slice, and the workspace bytes behind the raw block
static inline int mom_planes(int task, int O) { return task == MILE_TASK_REGRESSION ? 3 : O + 1; }
static inline size_t mom_acc_bytes(int task, int O, int N, int slices) {
  return (size_t)slices * N * ((size_t)mom_planes(task, O) * 8 + 4);
}

hipError_t mile_launch_moments_accum(int task, const MomParams &p, hipStream_t st);
hipError_t mile_launch_moments_finish(int task, const MomParams &p, hipStream_t st);

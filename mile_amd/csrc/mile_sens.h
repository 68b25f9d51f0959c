// Input sensitivities of the ensemble's predictions (mile_predict_sensitivities): per draw and row the Jacobian of the head
// outputs with respect to the row's inputs, reduced over the draw axis per row and over draws and rows per chain.  Kernels in
// mile_sens.hip; the entry point (argument checks, the tile plan, the tile loop) in mile_eval.hip.
//
// FCN only: a_0 = x, z_l = a_l W_l + b_l, a_{l+1} = phi(z_l) for l < L - 1, raw output r = z_{L-1};
//   Jraw[o][f] = d r_o / d x_f = [W_0 diag phi'(z_0) W_1 ... diag phi'(z_{L-2}) W_{L-1}]_{f,o},  phi' = act_bwd of the activation's
// output (relu'(0) = 0), the convention of the gradient kernels.  The reported columns J[p][f], P = O head outputs:
//   regression      J = Jraw: the sensitivities of mu and of log sigma, unclipped
//   classification  J[k][f] = pi_k (Jraw[k][f] - sum_j pi_j Jraw[j][f]), pi = softmax(r) in the stable form of mile_row_head.h
// A (draw, row) pair is kept iff its raw outputs and all P * F entries are finite; a NaN pre-activation stays NaN in the forward
// here (act_fwd's ReLU would answer 0), so what IEEE arithmetic makes non-finite is dropped.
//
// Per tile of Nt rows and pass of Sc draws:
//   k_sens_jac     grid (row slabs, draws), 256 threads, as k_fwd_generic: the activations of all layers of R rows in LDS (they
//                  give phi'), then the P backward sweeps delta_l = (delta_{l+1} W_l^T) .* phi'(z_l) of all rows at once through two
//                  LDS buffers [R][P][width]; a thread owns (row, output p, input unit i) and reads the contiguous weight row i.  fp32
//                  fmaf on the VALU.  Writes the pass's block jac [Sc][Nt][P][F]; a dropped pair has NaN in entry 0 of its block.
//   k_sens_accum   grid (ceil(Nt P F / 256), slices): a thread per column (n, p, f) -- the contiguous axis of jac, so a wave reads
//                  one run of 64 floats per draw -- walks its slice of the pass's draws and folds them into the slice's fp64
//                  accumulators (Welford's count, mean, M2 and the count of J > 0), which live in the workspace across passes;
//                  the pass and what the slice held before merge with Chan's formula
//   k_sens_chain   grid (column blocks, chains): one workgroup reduces its chain's draws of the pass and the tile's rows for its
//                  columns -- every thread a run of (draw, row) pairs in fp64, then the threads of a column in index order
//                  through LDS -- and adds sum J, sum |J| and the kept pairs to its own cells [C][P][F]: one owner per cell, the
//                  launches in tile-then-pass order
//   k_sens_finish  a thread per column, after the tile's last pass: merges the slices in index order, writes mean, sd, pos, dropped
//   k_sens_chain_finish  after the last tile: chain_ape = sum J / kept, chain_abs = sum |J| / kept, chain_kept
// Every accumulator is fp64, no atomics, every sum in a fixed order: the outputs are bitwise reproducible for one
// (C, S, N, max_draws_per_pass, max_rows_per_tile).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

#define SENS_NT 256              // threads of every workgroup here
#define SENS_MAX_SLICES 16       // slices of the draw loop of k_sens_accum (gridDim.y)
#define SENS_MAX_R 64            // rows of an LDS tile of k_sens_jac at most
#define SENS_LDS_TARGET (56 * 1024)    // LDS of k_sens_jac where more than one row fits it (k_fwd_generic's budget)
#define SENS_LDS_MAX (160 * 1024)      // and the most one row may take

// The FCN as k_sens_jac takes it by value.  act_off / act_stride: the row's activation record in LDS ([0] the input, [l + 1] the
// output of layer l), d_stride: the stride of one sweep's row of deltas; both odd, so that the rows of a tile start on different
// LDS banks.
struct SensNet {
  int32_t n_layers, in_features;
  int32_t widths[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS], b_off[MILE_MAX_LAYERS], act_off[MILE_MAX_LAYERS + 1];
  int32_t act_stride, d_stride, activation, task, d;
};
static inline SensNet sens_net(const mile_model_spec *spec, const int32_t *b_off, const int32_t *w_off, int d) {
  SensNet n{};
  n.n_layers = spec->n_layers; n.in_features = spec->in_features; n.activation = spec->activation; n.task = spec->task; n.d = d;
  int off = spec->in_features, dmax = spec->in_features;
  n.act_off[0] = 0;
  for (int l = 0; l < spec->n_layers; ++l) {
    n.widths[l] = spec->widths[l]; n.w_off[l] = w_off[l]; n.b_off[l] = b_off[l];
    n.act_off[l + 1] = off;
    off += spec->widths[l];
    if (l + 1 < spec->n_layers && spec->widths[l] > dmax) dmax = spec->widths[l];
  }
  n.act_stride = off | 1;
  n.d_stride = dmax | 1;
  return n;
}
// floats of LDS per row of a tile (the record, two delta buffers [P][d_stride], the drop flag), the rows of a tile (0: not even
// one row fits) and the bytes of the launch
static inline size_t sens_row_floats(const SensNet &n) {
  return (size_t)n.act_stride + 2 * (size_t)n.widths[n.n_layers - 1] * n.d_stride + 1;
}
static inline int sens_R(const SensNet &n) {
  const size_t per_row = sens_row_floats(n) * 4;
  if (per_row > SENS_LDS_MAX) return 0;
  const size_t R = SENS_LDS_TARGET / per_row;
  return R < 1 ? 1 : R > SENS_MAX_R ? SENS_MAX_R : (int)R;
}
static inline size_t sens_lds(const SensNet &n) { return sens_row_floats(n) * 4 * sens_R(n); }

struct SensJacParams {
  SensNet net;
  const float *theta;   // [Sc, d]: the pass's draws
  const float *X;       // [Nt, F]: the tile's rows
  float *jac;           // [Sc][Nt][P][F]
  int32_t Nt, SB, R;
};

struct SensAccParams {
  const float *jac;     // [Sc][Nt][PF]
  int Sc, Nt, PF, slices;
  long long D;          // draws of the whole call (finish: dropped = D - kept)
  double *mean, *M2;    // [slices][Nt * PF] each
  int32_t *pos, *cnt;   // [slices][Nt * PF] each: kept draws with J > 0, kept draws
  float *o_mean, *o_sd, *o_pos;   // [Nt][PF] at the tile's first row, any may be null
  int32_t *dropped;     // [Nt] at the tile's first row, or null
};
// bytes of the accumulators of one tile
static inline size_t sens_acc_bytes(int64_t Nt, int PF, int slices) { return (size_t)slices * Nt * PF * 24; }

struct SensChainParams {
  const float *jac;     // [Sc][Nt][PF]
  long long d0;         // the pass's first draw among the C * S of the call
  int Sc, Nt, PF, C;
  long long S;          // draws per chain
  double *sum, *abs;    // [C][PF]
  long long *kept;      // [C]
  double *o_ape, *o_abs;   // [C][PF], either may be null (chain_finish)
  long long *o_kept;       // [C], or null
};
static inline size_t sens_chain_bytes(int C, int PF) { return (size_t)C * ((size_t)PF * 16 + 8); }

hipError_t mile_launch_sens_jac(const SensJacParams &p, int Sc, hipStream_t st);
hipError_t mile_launch_sens_accum(const SensAccParams &p, hipStream_t st);
hipError_t mile_launch_sens_chain(const SensChainParams &p, hipStream_t st);
hipError_t mile_launch_sens_finish(const SensAccParams &p, hipStream_t st);
hipError_t mile_launch_sens_chain_finish(const SensChainParams &p, hipStream_t st);

// Partial dependence and ICE curves of the ensemble's predictions (mile_predict_partial_dependence): per draw, row, selected
// feature f = features[i] and grid value v = grid[i][g] the head outputs of the FCN on the row with x_f replaced by v, reduced
// over the draw axis per row (ICE) and over the rows per draw (PD), then over draws and chains.  Kernels in mile_pdp.hip; the
// entry point (argument checks, the tile plan, the tile loop) in mile_eval.hip.
//
// FCN only: z_0 = x W_0 + b_0 once per (draw, row); per grid point z_0' = z_0 + (v - x_f) W_0[f, :], one fmaf per first-layer unit,
// then a_1 = phi(z_0'), z_l = a_l W_l + b_l, a_{l+1} = phi(z_l) for l < L - 1, raw output r = z_{L-1}.  The reported columns
// h[p], P = O head outputs:
//   regression      h = r: mu and log sigma, unclipped
//   classification  h = softmax(r) in the stable form of mile_row_head.h
// This arithmetic is the definition (in exact arithmetic it is the substitution of v for x_f).  A NaN pre-activation stays NaN,
// as in mile_sens.h.  A (draw, row, feature) triple is kept iff all G * P values of the feature are finite: columns of different
// features are independent, so a call on a subset of the features returns, for those, the bits of the full call.  A row with a
// non-finite input in ANY column, f included, has a non-finite z_0 and is dropped for every feature: (v - inf) W_0[f, :] does not
// take the inf back out of z_0.
//
// Per tile of Nt rows and pass of Sc draws, Q = Fs * G * P columns:
//   k_pdp_fwd      grid (row slabs, draws), 256 threads: z_0 of R rows in LDS, then the (row, feature, grid point) triples as
//                  pseudo-rows of the remaining layers in batches of PR through two LDS buffers [PR][h_stride]; a thread owns one
//                  output unit of PDP_T pseudo-rows, reads the contiguous weight row once for them and the pseudo-rows 16 bytes
//                  at a time.  fp32 fmaf on the VALU, every accumulator in rising order of the input unit.
//                  Writes the pass's block val [Sc][Nt][Fs][G][P]; a dropped triple has NaN in all its G * P entries.
//   k_pdp_accum    grid (ceil(Nt Q / 256), slices): a thread per column (n, i, g, p) walks its slice of the pass's draws (Welford)
//                  and merges with what the slice held before (Chan): k_sens_accum with the NaN of the column itself as the drop mark
//   k_pdp_rows     grid (features x column blocks, draws): the fp64 sum of the tile's kept rows of every (draw, column) -- every
//                  thread a strided run of rows, then the threads of a column in index order through LDS; the split of the rows
//                  depends on G * P alone, not on Fs -- added to the draw's own cell
//                  [C S][Q], and the kept rows to [C S][Fs]: one owner per cell, the launches in tile-then-pass order
//   k_pdp_row_finish  a thread per column, after the tile's last pass: merges the slices in index order, writes ice_mean, ice_sd, dropped
//   k_pdp_finish   after the last tile: curves = sum / kept rows; per chain Welford over its draws in index order (chain_pd,
//                  chain_draws), then the chains in index order by Chan's merge (pd_mean, pd_sd), from the fp64 row means
// Every accumulator is fp64, no atomics, every sum in a fixed order: the outputs are bitwise reproducible for one
// (C, S, N, Fs, G, max_draws_per_pass, max_rows_per_tile).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

#define PDP_NT 256               // threads of every workgroup here
#define PDP_MAX_SLICES 16        // slices of the draw loop of k_pdp_accum (gridDim.y)
#define PDP_MAX_R 64             // rows of an LDS slab of k_pdp_fwd at most
#define PDP_MAX_PR 1024          // pseudo-rows of a batch at most
#define PDP_T 8                  // pseudo-rows of a thread's register tile
#define PDP_G_MAX 256            // grid points per feature at most
#define PDP_LDS_TARGET (56 * 1024)    // LDS of k_pdp_fwd where more than one row fits it (k_sens_jac's budget)
#define PDP_LDS_MAX (160 * 1024)      // and the most one row with one pseudo-row may take
#define PDP_FIN_W 32             // k_pdp_finish: columns of a workgroup; its 256 / 32 = 8 lanes take chains
#define PDP_CELL_MAX ((int64_t)1 << 30)   // bytes of the per-draw cells [C S][Q] fp64 at most

// The FCN as k_pdp_fwd takes it by value.  z_stride: one row's z_0, odd, so that consecutive rows start on different LDS banks;
// h_stride: one pseudo-row's activations of any later layer, a multiple of 4 floats with 4 to spare: the layer loop reads a
// pseudo-row 16 bytes at a time, and the lanes of a wave that share the pseudo-row get it by broadcast.
struct PdpNet {
  int32_t n_layers, in_features;
  int32_t widths[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS], b_off[MILE_MAX_LAYERS];
  int32_t z_stride, h_stride, activation, task, d;
};
static inline PdpNet pdp_net(const mile_model_spec *spec, const int32_t *b_off, const int32_t *w_off, int d) {
  PdpNet n{};
  n.n_layers = spec->n_layers; n.in_features = spec->in_features; n.activation = spec->activation; n.task = spec->task; n.d = d;
  int hmax = 1;
  for (int l = 0; l < spec->n_layers; ++l) {
    n.widths[l] = spec->widths[l]; n.w_off[l] = w_off[l]; n.b_off[l] = b_off[l];
    if (spec->widths[l] > hmax) hmax = spec->widths[l];
  }
  n.z_stride = spec->widths[0] | 1;
  n.h_stride = (hmax + 3) / 4 * 4 + 4;
  return n;
}
// The LDS of a launch with Fs selected features: R rows of (z_0, the Fs selected inputs, the Fs drop flags), rounded up to 16
// bytes, and two buffers of PR pseudo-rows (whole register tiles where more than one fits).  R == 0: not even one row with one
// pseudo-row fits.
struct PdpLds { int R, PR; size_t bytes; };
static inline PdpLds pdp_lds(const PdpNet &n, int Fs) {
  const size_t row = ((size_t)n.z_stride + 2 * (size_t)Fs) * 4, pr = 2 * (size_t)n.h_stride * 4;
  if (row + 16 + pr > PDP_LDS_MAX) return {0, 0, 0};
  size_t R = 1, PR;
  if (row + 16 + pr > PDP_LDS_TARGET) {
    PR = (PDP_LDS_MAX - row - 16) / pr;
    if (PR > 64) PR = 64;
  } else {
    R = PDP_LDS_TARGET / 4 / row;
    if (R > (PDP_LDS_TARGET - 16 - pr) / row) R = (PDP_LDS_TARGET - 16 - pr) / row;
    R = R < 1 ? 1 : R > PDP_MAX_R ? PDP_MAX_R : R;
    PR = (PDP_LDS_TARGET - 16 - R * row) / pr;
    if (PR > PDP_MAX_PR) PR = PDP_MAX_PR;
  }
  if (PR > PDP_T) PR = PR / PDP_T * PDP_T;
  return {(int)R, (int)PR, (R * row + 15) / 16 * 16 + PR * pr};
}

struct PdpFwdParams {
  PdpNet net;
  const float *theta;       // [Sc, d]: the pass's draws
  const float *X;           // [Nt, F]: the tile's rows
  const int32_t *features;  // [Fs], device
  const float *grid;        // [Fs][G]
  float *val;               // [Sc][Nt][Fs][G][P]
  int32_t Nt, SB, R, PR, Fs, G;
};

struct PdpAccParams {
  const float *val;     // [Sc][Nt][Q]
  int Sc, Nt, Q, GP, slices;
  long long D;          // draws of the whole call (row_finish: dropped = D - kept)
  double *mean, *M2;    // [slices][Nt * Q] each
  int32_t *cnt;         // [slices][Nt * Q]: kept draws
  float *o_mean, *o_sd; // [Nt][Q] at the tile's first row, either may be null
  int32_t *dropped;     // [Nt][Fs] at the tile's first row, or null
};
static inline size_t pdp_acc_bytes(int64_t Nt, int64_t Q, int slices) { return (size_t)slices * Nt * Q * 20; }

struct PdpRowsParams {
  const float *val;     // [Sc][Nt][Q]
  long long d0;         // the pass's first draw among the C * S of the call
  int Sc, Nt, Q, GP, Fs, C;
  long long S;          // draws per chain
  double *sum;          // [C S][Q]: sums over the kept rows
  int32_t *kept;        // [C S][Fs]: the kept rows
  double *c_mean, *c_M2;   // [C][Q]: the chains' Welford records (k_pdp_finish)
  int32_t *c_n;            // [C][Q]
  float *curves;           // [C S][Q], or null
  double *pd_mean, *pd_sd; // [Q], either may be null
  double *chain_pd;        // [C][Q], or null
  long long *chain_draws;  // [C][Fs], or null
};
static inline size_t pdp_chain_bytes(int C, int64_t Q) { return (size_t)C * Q * 20; }

hipError_t mile_launch_pdp_fwd(const PdpFwdParams &p, int Sc, hipStream_t st);
hipError_t mile_launch_pdp_accum(const PdpAccParams &p, hipStream_t st);
hipError_t mile_launch_pdp_rows(const PdpRowsParams &p, hipStream_t st);
hipError_t mile_launch_pdp_row_finish(const PdpAccParams &p, hipStream_t st);
hipError_t mile_launch_pdp_finish(const PdpRowsParams &p, hipStream_t st);

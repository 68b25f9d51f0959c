// Canonical hidden-unit ordering of FCN draws (mile_canonicalize_fcn): every draw theta[m] is replaced by the representative
// of its orbit under the hidden-unit permutations (and, for tanh with MILE_CANON_SIGN, the sign flips) of the net.
// Kernels in mile_canon.hip; this header holds the rule, the plan and the launcher.  The entry points (argument checks) are in
// mile_canon.hip too: they need no sampler handle and launch on the current device.
//
// THE RULE (restated in NumPy by tests/canon_ref.py and in torch by mile_amd.metrics.canonicalize_dense).
//   Hidden layers are l = 0 .. n_layers - 2, widths W_l; the output layer and the inputs never move.  H = sum_l W_l, hidden
//   layer l owns [o_l, o_l + W_l) of the H axis.
//   sign  (MILE_CANON_SIGN, tanh only)   s_l[j] = -1 iff bias_l[j] < 0, else +1: -0.0, +0.0 and NaN are not flipped.
//   key   MILE_CANON_KEY_BIAS            s_l[j] * bias_l[j], compared as a number (fp32; held as the fp64 of the same value)
//         MILE_CANON_KEY_NORM            bias^2 + sum_i kernel_l[i][j]^2 in fp64, the terms added one after another, bias first,
//                                        then i ascending.  A square of an fp32 is exact in fp64, so a fused and an unfused
//                                        multiply-add round alike: the key is reproducible bit for bit.  No tree.
//   order ascending key; equal keys (-0.0 == +0.0, duplicated units) keep their index order; NaN keys come after every number,
//         among themselves in index order; +-inf sort as numbers.  p_l[j'] = the original index of the unit at position j'.
//   result  bias_l'[j'] = s_l[p_l[j']] * bias_l[p_l[j']]
//           kernel_l'[i'][j'] = s_{l-1}[p_{l-1}[i']] * s_l[p_l[j']] * kernel_l[p_{l-1}[i']][p_l[j']]
//           (row factors: identity for l = 0; column factors: identity for the output layer).  Every output float is an input
//           float moved, possibly negated; nothing is recomputed.  A draw is handled on its own.
//   perm [M][H] int32: perm[m][o_l + j'] = p_l[j'];  sign [M][H] int8: sign[m][o_l + j'] = s_l[p_l[j']].
//
// LAUNCHES.  A draw whose d floats, H keys and H ranks fit the CU's LDS (canon_fits) takes ONE launch:
//   k_canon_draw   one workgroup per draw (256 threads, 512 from 4096 floats a draw on): the draw into LDS with 16-byte loads; a thread per hidden unit forms its key,
//                  then its rank by a stable count over the keys of its layer (a broadcast read per comparison; for W <= 64 one
//                  wave holds a layer, a unit per lane); then every layer's bias and rows are written in coalesced runs, the
//                  source row and column looked up in LDS.
// Any other draw takes the per-layer, row-tiled form of the same code in two launches:
//   k_canon_rank   one workgroup per draw: keys and ranks as above from global memory (for the norm key the lanes of a wave read
//                  one source row side by side) -> (index | flip bit) words [M][H] in the workspace
//   k_canon_rows   one workgroup per (draw, layer, 16 output rows): a wave takes a row at a time; the source row p_{l-1}[i'] is
//                  one contiguous run of W_l floats, read coalesced into the wave's LDS row and written back with its columns
//                  permuted.
// No atomics, nothing depends on the launch geometry: a draw gives the same bits whatever M is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mile_hip.h"

#define CANON_NT 256               // workgroup of k_canon_rank, k_canon_rows and of k_canon_draw on small draws
#define CANON_NT_BIG 512           // k_canon_draw on draws of CANON_BIG_D floats or more: more loads and stores in flight per phase
#define CANON_BIG_D 4096
#define CANON_LDS_MAX (160 * 1024)
#define CANON_TILE_ROWS 16           // output rows per workgroup of k_canon_rows (the bias counts as row 0)
#define CANON_FLIP 0x80000000u       // a rank word: the unit's original index, and this bit when its sign is flipped

// The FCN's parameter row as the library lays it out (fcn_param_layout of mile_hip.hip: ravel_pytree's order, "layer10" before
// "layer2"), with the hidden spans of the H axis.
struct CanonPlan {
  int n_layers, n_hidden, H, d;
  int fin[MILE_MAX_LAYERS], fout[MILE_MAX_LAYERS], b_off[MILE_MAX_LAYERS], w_off[MILE_MAX_LAYERS];
  int o[MILE_MAX_LAYERS];            // o[l]: first H index of hidden layer l; o[n_hidden] = H
  int max_rows;                      // the most rows (bias + fin) any layer has
};

struct CanonParams {
  CanonPlan pl;
  const float *theta;
  long long M;
  unsigned how;
  float *out;
  int32_t *perm;       // [M][H] or null
  int8_t *sign;        // [M][H] or null
  uint32_t *ranks;     // workspace [M][H] of the tiled form, null in the LDS form
};

// LDS of k_canon_draw: the draw (shifted by up to 3 floats so that 16-byte global loads land on 16-byte LDS slots), H fp64
// keys, H rank words
static inline size_t canon_draw_lds(const CanonPlan &pl) {
  return ((size_t)pl.d + 3 + 3) / 4 * 16 + (size_t)pl.H * 8 + ((size_t)pl.H * 4 + 15) / 16 * 16;
}
static inline bool canon_fits(const CanonPlan &pl) { return canon_draw_lds(pl) <= CANON_LDS_MAX; }
static inline size_t canon_rank_lds(const CanonPlan &pl) { return (size_t)pl.H * 8; }

hipError_t mile_launch_canon(const CanonParams &p, hipStream_t st);

// For other makers of rank words (mile_align.hip): the shape check and the layout of the plan, each returning why not or null,
// and the write phase alone -- k_canon_rows from p.theta and p.ranks [M][H] to p.out (p.how, p.perm and p.sign are not read).
const char *mile_canon_shape(const mile_model_spec *spec);
const char *mile_canon_layout(const mile_model_spec *spec, CanonPlan &pl);
hipError_t mile_launch_canon_rows(const CanonParams &p, hipStream_t st);

// Alignment of FCN draws to a reference draw by hidden-unit assignment (mile_align_fcn): every draw's hidden units are matched,
// layer by layer, to those of one reference row by a linear assignment problem, so that "parameter j" is the same unit in every
// draw and chain.  The rule is stated in include/mile_hip.h and restated in NumPy by tests/align_ref.py.  Kernel, launcher and
// entry points in mile_align.hip; the move of the floats is mile_canon.h's write phase (k_canon_rows), driven by rank words.
//
// LAUNCHES.  Two, whatever the shape:
//   k_align_solve  one workgroup of ONE wave per draw, so no wave idles while the solve runs and S is the wave's own.  Per hidden
//                  layer, in ascending order:
//                    similarity  S [W][W] fp64 in LDS.  A lane owns column j (and j + 64 for 64 < W <= 128) and carries ALIGN_IB
//                                rows i at a time in registers; every element is accumulated in the rule's order by that one lane.
//                                The draw's row kernel_l[p_{l-1}[t]][.] is one coalesced read (p_{l-1}, s_{l-1} looked up in LDS),
//                                the reference terms are the same address in every lane.  Draw and reference are read from global
//                                memory (through the caches), so d is not bounded by the LDS.
//                    assignment  the shortest-augmenting-path Hungarian method with potentials, fp64, in the rule's operation
//                                order.  minv, used, way, v of a column live in its lane's registers, and so do the row assigned
//                                to the column and that row's potential u (a row keeps exactly one column once it is inserted;
//                                both move along the augmenting path).  The row inserted now has its potential in a uniform
//                                register.  The cost row c[i0][.] = -G[i0][.] is read row-contiguous from LDS.  The argmin is a
//                                DPP minimum inside each row of 16 lanes, four readlanes across, then a ballot of the lanes that
//                                hold the minimum: the lowest column among equals (the first 64 columns before the second).
//                    ranks       (index | flip bit) words of the layer into LDS, the score added in ascending i.
//                  Last, the draw's rank words go to the workspace [M][H] and perm, sign, score, dropped to their arrays -- or,
//                  for a draw with a non-finite similarity, the identity, NaN scores and dropped = 1.
//   k_canon_rows   (mile_launch_canon_rows) out from theta and the rank words.
// No atomics; a draw is handled by its own wave from its own floats: the same bits for any M and launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mile_canon.h"

#define ALIGN_NT 64                // one wave
#define ALIGN_IB 4                 // rows of S a lane accumulates side by side
#define ALIGN_LDS_MAX (160 * 1024)

struct AlignParams {
  CanonPlan pl;
  const float *theta;  // [M][d]
  const float *ref;    // [d]
  long long M;
  unsigned how;
  int wmax;            // the widest hidden layer (0 without one)
  uint32_t *ranks;     // workspace [M][H]
  int32_t *perm;       // [M][H] or null
  int8_t *sign;        // [M][H] or null
  double *score;       // [M][n_hidden] or null
  int32_t *dropped;    // [M] or null
};

// LDS of k_align_solve: S [wmax][wmax] fp64, a score per hidden layer, the draw's H rank words, five rows of the plan
// (all of it dynamic: at most 128 KB + 120 + 7680 + 300 bytes, below ALIGN_LDS_MAX)
static inline size_t align_lds(const AlignParams &p) {
  return (size_t)p.wmax * p.wmax * 8 + (size_t)MILE_MAX_LAYERS * 8 + ((size_t)p.pl.H * 4 + 15) / 16 * 16 + 5 * MILE_MAX_LAYERS * 4;
}

hipError_t mile_launch_align(const AlignParams &p, float *out, hipStream_t st);

// The padded geometry of a stack of Dense layers on the layer-wise k_mm3 path, and the format of its weights as bf16 term planes
// [batch][layer][term][in][outp]: what launch_grad_wide, launch_fwd_wide and the Dense half of LeNet agree on.  Plain C++17,
// nothing from HIP: host tests include this file alone.
#pragma once
#include <stddef.h>

#include "../../include/mile_hip.h"

struct LayerPlan {
  int L, terms;                                        // layers; bf16 terms per weight (3: fp32-faithful, 1: bf16-rounded operands)
  int fin[MILE_MAX_LAYERS], fout[MILE_MAX_LAYERS];     // real in and out widths
  int wp[MILE_MAX_LAYERS];                             // out width rounded up to 8: leading dimension of the layer's outputs and planes
  int ldin[MILE_MAX_LAYERS];                           // leading dimension of the layer's input
  int w_off[MILE_MAX_LAYERS], b_off[MILE_MAX_LAYERS];  // kernel and bias in a parameter row
  size_t wt_off[MILE_MAX_LAYERS], wt_elems;            // the layer's term planes in a batch entry's, and all of them, in bf16 elements
  int maxwp;                                           // the widest padded width
  size_t sum_wp;

  size_t plane(int l) const { return (size_t)fin[l] * wp[l]; }     // one term plane of layer l: [in][outp]
  size_t per_row() const { return sum_wp + 2 * (size_t)maxwp; }    // activation floats per row: every layer's outputs, two dZ buffers

  void push(int fin_, int ldin_, int fout_, int w_off_, int b_off_) {
    const int l = L++;
    fin[l] = fin_; ldin[l] = ldin_; fout[l] = fout_; w_off[l] = w_off_; b_off[l] = b_off_;
    wp[l] = (fout_ + 7) / 8 * 8;
    wt_off[l] = wt_elems;
    wt_elems += terms * plane(l);
    sum_wp += wp[l];
    if (wp[l] > maxwp) maxwp = wp[l];
  }
};

// the FCN (DevSpec): in_features -> widths[0] -> .. -> widths[L - 1], on X zero-padded to Fp columns
template <class Spec>
static inline LayerPlan layer_plan_fcn(const Spec &ds, int Fp, int terms) {
  LayerPlan p{0, terms};
  for (int l = 0; l < ds.n_layers; ++l)
    p.push(l ? ds.widths[l - 1] : ds.in_features, l ? p.wp[l - 1] : Fp, ds.widths[l], ds.w_off[l], ds.b_off[l]);
  return p;
}
// the Dense half of LeNet (LeNetGeom), three terms: flat -> 120 -> 84 -> K, on the pooled convolution output [rows][flat]
template <class Geom>
static inline LayerPlan layer_plan_lenet(const Geom &g) {
  LayerPlan p{0, 3};
  p.push(g.flat, g.flat, 120, g.k_f1, g.b_f1);
  p.push(120, p.wp[0], 84, g.k_f2, g.b_f2);
  p.push(84, p.wp[1], g.K, g.k_f3, g.b_f3);
  return p;
}

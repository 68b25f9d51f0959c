// k_grad_narrow<NH, TH, TF, WL, PART = true>: the partition-sampling form of the narrow fused grad kernel (mile_grad_narrow.h),
// one instantiation per shape the ordinary form covers with at least two hidden layers
// (a net with one has no frozen layer and never enters partition mode).  A translation unit of its own so that these instantiations
// compile next to mile_hip.hip instead of lengthening it.
#include <hip/hip_runtime.h>

#include "mile_grad_narrow.h"

template <int NH, int TH, int TF>
static hipError_t launch(const GradParams &gp, int E, int nw, hipStream_t st) {
  constexpr bool WL = TH >= 3;
  using LY = NarrowLayout<NH, TH, TF, WL>;
  if constexpr (WL) {
    hipError_t e = mile_set_max_lds<k_grad_narrow<NH, TH, TF, WL, true>>(LY::BYTES);
    if (e != hipSuccess) return e;
  }
  k_grad_narrow<NH, TH, TF, WL, true><<<dim3(gp.S, E), 64 * nw, LY::BYTES, st>>>(gp);
  return hipGetLastError();
}

// nh hidden layers, th = tiles of 16 of the widest hidden layer, tf = 1 (F <= 16) or 4, nw waves per workgroup
hipError_t mile_launch_narrow_part(int nh, int th, int tf, int nw, const GradParams &gp, int E, hipStream_t st) {
  if (!gp.part_frozen || gp.part_d < 1) return hipErrorInvalidValue;
#define MILE_NRW(NH_, TH_, TF_) if (nh == NH_ && th == TH_ && tf == TF_) return launch<NH_, TH_, TF_>(gp, E, nw, st);
  MILE_NRW(2, 1, 1) MILE_NRW(2, 2, 1) MILE_NRW(2, 1, 4) MILE_NRW(2, 2, 4)
  MILE_NRW(3, 1, 1) MILE_NRW(3, 2, 1) MILE_NRW(3, 1, 4) MILE_NRW(3, 2, 4)
  MILE_NRW(4, 1, 1) MILE_NRW(5, 1, 1) MILE_NRW(6, 1, 1) MILE_NRW(7, 1, 1) MILE_NRW(8, 1, 1) MILE_NRW(9, 1, 1) MILE_NRW(10, 1, 1)
  MILE_NRW(2, 3, 1) MILE_NRW(2, 4, 1) MILE_NRW(2, 3, 4) MILE_NRW(2, 4, 4)      // hidden widths 33..64: weights in LDS
  MILE_NRW(3, 3, 1) MILE_NRW(3, 4, 1) MILE_NRW(3, 3, 4) MILE_NRW(3, 4, 4)
#undef MILE_NRW
  return hipErrorInvalidValue;
}

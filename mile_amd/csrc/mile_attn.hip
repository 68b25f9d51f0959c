// AttentionClassifier kernels (mile_attn.h) in a translation unit of their own.  The dK register tiles per key tile
// (ceil(hd / 16): 1..4) and whether Wq|Wk|Wv fit in LDS next to the sequence are template arguments.
#include <hip/hip_runtime.h>

#include "mile_attn.h"

template <bool WL>
struct AttnKernels {
  template <int NHT> static constexpr auto grad = k_grad_attn<NHT, WL>;
  template <int NHT> static constexpr auto fwd = k_fwd_attn<NHT, WL>;
  template <int NHT> static constexpr auto out = k_out_attn<NHT, WL>;
};

hipError_t mile_launch_attn(const AttnParams &p, int E, MileRun run, hipStream_t st) {
  if (!attn_supported(p.g)) return hipErrorInvalidValue;
  return attn_weights_in_lds(p.g) ? attn_launch<AttnKernels<true>, 4>(p, E, run, attn_lds_bytes(p.g, true), st)
                                  : attn_launch<AttnKernels<false>, 4>(p, E, run, attn_lds_bytes(p.g, false), st);
}

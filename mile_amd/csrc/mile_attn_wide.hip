// Wide AttentionClassifier kernels (mile_attn_wide.h) in a translation unit of their own.  The dq register tiles per query
// tile (ceil(hd / 16): 1..8) are a template argument.
#include <hip/hip_runtime.h>

#include "mile_attn_wide.h"

struct AttnWideKernels {
  template <int NHT> static constexpr auto grad = k_grad_attn_wide<NHT>;
  template <int NHT> static constexpr auto fwd = k_fwd_attn_wide<NHT>;
  template <int NHT> static constexpr auto out = k_out_attn_wide<NHT>;
};

hipError_t mile_launch_attn_wide(const AttnParams &p, int E, MileRun run, hipStream_t st) {
  if (!attn_wide_supported(p.g)) return hipErrorInvalidValue;
  return attn_launch<AttnWideKernels, 8>(p, E, run, attnp_lds_bytes(p.g), st);
}

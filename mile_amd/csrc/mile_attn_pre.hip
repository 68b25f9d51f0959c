// PretrainedAttentionClassifier kernels (mile_attn_pre.h) in a translation unit of their own.  The dq register tiles per
// query tile (ceil(hd / 16): 1..8) are a template argument.
#include <hip/hip_runtime.h>

#include "mile_attn_pre.h"

struct AttnPreKernels {
  template <int NHT> static constexpr auto grad = k_grad_attn_pre<NHT>;
  template <int NHT> static constexpr auto fwd = k_fwd_attn_pre<NHT>;
  template <int NHT> static constexpr auto out = k_out_attn_pre<NHT>;
};

hipError_t mile_launch_attn_pre(const AttnParams &p, int E, MileRun run, hipStream_t st) {
  if (!attnp_supported(p.g) || !p.emb || !p.pos) return hipErrorInvalidValue;
  return attn_launch<AttnPreKernels, 8>(p, E, run, attnp_lds_bytes(p.g), st);
}

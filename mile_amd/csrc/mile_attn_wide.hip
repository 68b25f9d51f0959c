// Wide AttentionClassifier kernels (mile_attn_wide.h) in a translation unit of their own.  The dq register tiles per query
// tile (ceil(hd / 16): 1..8) are a template argument.
#include <hip/hip_runtime.h>

#include "mile_attn_wide.h"

template <int NHT>
static hipError_t launch_t(const AttnPreParams &p, int E, MileRun run, hipStream_t st) {
  const size_t lds = attn_wide_lds_bytes(p.g);
  hipError_t e = run == MILE_RUN_GRAD  ? mile_set_max_lds<k_grad_attn_wide<NHT>>(ATTN_LDS_MAX)
                 : run == MILE_RUN_RAW ? mile_set_max_lds<k_out_attn_wide<NHT>>(ATTN_LDS_MAX)
                                       : mile_set_max_lds<k_fwd_attn_wide<NHT>>(ATTN_LDS_MAX);
  if (e != hipSuccess) return e;
  const dim3 grid(p.S, E);
  if (run == MILE_RUN_GRAD) k_grad_attn_wide<NHT><<<grid, ATTN_NT, lds, st>>>(p);
  else if (run == MILE_RUN_RAW) k_out_attn_wide<NHT><<<grid, ATTN_NT, lds, st>>>(p);
  else k_fwd_attn_wide<NHT><<<grid, ATTN_NT, lds, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_attn_wide(const AttnPreParams &p, int E, MileRun run, hipStream_t st) {
  if (!attn_wide_supported(p.g)) return hipErrorInvalidValue;
  switch ((p.g.hd + 15) / 16) {
    case 1: return launch_t<1>(p, E, run, st);
    case 2: return launch_t<2>(p, E, run, st);
    case 3: return launch_t<3>(p, E, run, st);
    case 4: return launch_t<4>(p, E, run, st);
    case 5: return launch_t<5>(p, E, run, st);
    case 6: return launch_t<6>(p, E, run, st);
    case 7: return launch_t<7>(p, E, run, st);
    case 8: return launch_t<8>(p, E, run, st);
  }
  return hipErrorInvalidValue;
}

// AttentionClassifier kernels (mile_attn.h) in a translation unit of their own.  The dK register tiles per key tile
// (ceil(hd / 16): 1..4) and whether Wq|Wk|Wv fit in LDS next to the sequence are template arguments.
#include <hip/hip_runtime.h>

#include "mile_attn.h"

template <int NHT, bool WL>
static hipError_t launch_t(const AttnParams &p, int E, MileRun run, hipStream_t st) {
  const size_t lds = attn_lds_bytes(p.g, WL);
  hipError_t e = run == MILE_RUN_GRAD  ? mile_set_max_lds<k_grad_attn<NHT, WL>>(ATTN_LDS_MAX)
                 : run == MILE_RUN_RAW ? mile_set_max_lds<k_out_attn<NHT, WL>>(ATTN_LDS_MAX)
                                       : mile_set_max_lds<k_fwd_attn<NHT, WL>>(ATTN_LDS_MAX);
  if (e != hipSuccess) return e;
  const dim3 grid(p.S, E);
  if (run == MILE_RUN_GRAD) k_grad_attn<NHT, WL><<<grid, ATTN_NT, lds, st>>>(p);
  else if (run == MILE_RUN_RAW) k_out_attn<NHT, WL><<<grid, ATTN_NT, lds, st>>>(p);
  else k_fwd_attn<NHT, WL><<<grid, ATTN_NT, lds, st>>>(p);
  return hipGetLastError();
}

template <bool WL>
static hipError_t launch_w(const AttnParams &p, int E, MileRun run, hipStream_t st) {
  switch ((p.g.hd + 15) / 16) {
    case 1: return launch_t<1, WL>(p, E, run, st);
    case 2: return launch_t<2, WL>(p, E, run, st);
    case 3: return launch_t<3, WL>(p, E, run, st);
    case 4: return launch_t<4, WL>(p, E, run, st);
  }
  return hipErrorInvalidValue;
}

hipError_t mile_launch_attn(const AttnParams &p, int E, MileRun run, hipStream_t st) {
  const AttnGeom &g = p.g;
  if (g.T < 1 || g.T > ATTN_MAX_T || g.C < 1 || g.C > ATTN_MAX_C || g.D < 1 || g.D > ATTN_MAX_D || g.H < 1 || g.D % g.H ||
      g.K < 1 || g.K > ATTN_MAX_K || g.NP < 0 || g.NP > ATTN_MAX_NP || g.Tp != (g.T + 15) / 16 * 16 || g.V < 1)
    return hipErrorInvalidValue;
  for (int l = 0; l < g.NP; ++l)
    if (g.P[l] < 1 || g.P[l] > ATTN_MAX_P) return hipErrorInvalidValue;
  if (attn_lds_bytes(g, false) > ATTN_LDS_MAX) return hipErrorInvalidValue;
  return attn_weights_in_lds(g) ? launch_w<true>(p, E, run, st) : launch_w<false>(p, E, run, st);
}

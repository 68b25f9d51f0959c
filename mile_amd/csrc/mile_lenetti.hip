// LeNetti kernels (mile_lenetti.h) in a translation unit of their own: the instantiations compile concurrently with
// mile_hip.hip.  Pixels per thread (1..8) and the channel bound (1 or 4) are template arguments.
#include <hip/hip_runtime.h>

#include "mile_lenetti.h"

template <int PPT, int T, int CM>
static hipError_t launch_t(const LeNettiParams &lp, int E, MileRun run, hipStream_t st) {
  const size_t lds = lenetti_lds_bytes(lp.g, T);
  hipError_t e = run == MILE_RUN_GRAD  ? mile_set_max_lds<k_grad_lenetti<PPT, T, CM>>(150 * 1024)
                 : run == MILE_RUN_RAW ? mile_set_max_lds<k_out_lenetti<PPT, T, CM>>(150 * 1024)
                                       : mile_set_max_lds<k_fwd_lenetti<PPT, T, CM>>(150 * 1024);
  if (e != hipSuccess) return e;
  const dim3 grid(lp.S, E);
  if (run == MILE_RUN_GRAD) k_grad_lenetti<PPT, T, CM><<<grid, LENETTI_NT, lds, st>>>(lp);
  else if (run == MILE_RUN_RAW) k_out_lenetti<PPT, T, CM><<<grid, LENETTI_NT, lds, st>>>(lp);
  else k_fwd_lenetti<PPT, T, CM><<<grid, LENETTI_NT, lds, st>>>(lp);
  return hipGetLastError();
}

template <int CM>
static hipError_t launch_c(const LeNettiParams &lp, int E, MileRun run, hipStream_t st) {
  switch (lenetti_ppt(lp.g)) {
    case 1: return launch_t<1, 4, CM>(lp, E, run, st);
    case 2: return launch_t<2, 4, CM>(lp, E, run, st);
    case 3: return launch_t<3, 4, CM>(lp, E, run, st);
    case 4: return launch_t<4, 4, CM>(lp, E, run, st);
    case 5: return launch_t<5, 2, CM>(lp, E, run, st);
    case 6: return launch_t<6, 2, CM>(lp, E, run, st);
    case 7: return launch_t<7, 2, CM>(lp, E, run, st);
    case 8: return launch_t<8, 2, CM>(lp, E, run, st);
  }
  return hipErrorInvalidValue;
}

hipError_t mile_launch_lenetti(const LeNettiParams &lp, int E, MileRun run, hipStream_t st) {
  if (lp.g.C < 1 || lp.g.C > LENETTI_MAX_C || lp.g.K < 1 || lp.g.K > LENETTI_MAX_K) return hipErrorInvalidValue;
  return lp.g.C == 1 ? launch_c<1>(lp, E, run, st) : launch_c<LENETTI_MAX_C>(lp, E, run, st);
}

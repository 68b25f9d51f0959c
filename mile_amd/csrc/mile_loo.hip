// PSIS-LOO / WAIC kernels (mile_loo.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_device.h"
#include "mile_loo.h"
#include "mile_loo_device.h"

__global__ __launch_bounds__(256) void k_loo_pack(const LooParams p) {
  loo_pack_tile(p.pk, p.S, p.Nt, p.slices, [&](int s, int row) -> float { return p.ll[(size_t)s * (size_t)p.ld + row]; });
}

// One workgroup per row, from the stages of mile_loo_device.h (the one text of them, k_lxp_row's too).  An output that is not
// asked for ends the row early: lppd and p_waic fall out of stage 1, khat out of the fit.
template <bool LDS>
__global__ __launch_bounds__(LOO_NT) void k_loo_row(const LooParams p) {
  extern __shared__ float loo_row[];                  // <true>: the row's S values
  __shared__ uint32_t tkey[LOO_MAX_TAIL];             // the tail's keys, ascending in l after the sort
  __shared__ double tx[LOO_MAX_TAIL];                 // x_i, then lw_i, ascending in r (tx[i] belongs to tkey[M - 1 - i])
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[4];                         // the scan's digit, rank left, keys below, keys in the bin
  __shared__ uint32_t tail_cnt;
  __shared__ double cb[LOO_MAX_CAND], cL[LOO_MAX_CAND], cw[LOO_MAX_CAND];
  __shared__ double red[LOO_NW];
  __shared__ LooStat wst[LOO_NW];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int S = p.S;
  const float *g = p.pk + (size_t)n * S;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  auto val = [&](int i) -> float {
    if constexpr (LDS) return loo_row[i];
    else return g[i];
  };

  const LooStat st = loo_row_stats<LDS>(g, loo_row, S, wst);
  const int kept = st.n;     // (the same in every thread from here on)
  if (tid == 0 && p.dropped) p.dropped[n] = (int32_t)(S - kept);
  const bool want_loo = p.elpd_loo || p.khat;
  if (kept < 2) {
    if (tid == 0) {
      if (p.lppd) p.lppd[n] = qnan;
      if (p.p_waic) p.p_waic[n] = qnan;
      if (p.elpd_loo) p.elpd_loo[n] = qnan;
      if (p.khat) p.khat[n] = qnan;
    }
    return;
  }
  if (tid == 0) {
    if (p.lppd) p.lppd[n] = st.m + log(st.s) - log((double)kept);
    if (p.p_waic) p.p_waic[n] = st.M2 / (double)(kept - 1);
  }
  if (!want_loo) return;
  const int M = loo_row_tail_length(kept, S, p.M_full, p.r_eff);
  if (M < 1 || M > LOO_MAX_TAIL || M + 1 > kept) {     // cannot happen: M(kept) <= M(S) <= LOO_MAX_TAIL is checked on the host
    if (tid == 0) {
      if (p.elpd_loo) p.elpd_loo[n] = qnan;
      if (p.khat) p.khat[n] = qnan;
    }
    return;
  }
  const double lmin = st.lo, mx = -lmin;     // r = -l - max(-l)
  const LooCut c = loo_row_select(val, S, M, hist, sel);
  loo_row_sort_tail(val, S, M, c, tkey, &tail_cnt);
  const double r_T = -(double)f32_unkey(c.T) - mx;
  const double cut = fmax(r_T, LOO_LOG_DBL_MIN), ec = exp(cut);
  const LooFit f = loo_row_fit(M, tkey, tx, mx, ec, cb, cL, cw, red);
  if (tid == 0 && p.khat) p.khat[n] = f.khat;
  if (!p.elpd_loo) return;
  double mlw = r_T, ma = lmin, s1, s2;     // the body: lw = r <= r_T, lw + l = lmin up to rounding
  loo_row_smooth(M, tkey, tx, f, mx, ec, mlw, ma, red);
  loo_row_sums(val, S, M, c, tkey, tx, mx, r_T, mlw, ma, s1, s2, red);
  if (tid == 0) p.elpd_loo[n] = (ma + log(s2)) - (mlw + log(s1));
}

hipError_t mile_launch_loo(const LooParams &p, hipStream_t st) {
  k_loo_pack<<<dim3((p.Nt + LOO_TILE - 1) / LOO_TILE, p.slices), 256, 0, st>>>(p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (p.S <= LOO_LDS_MAX_S) {
    e = mile_set_max_lds<k_loo_row<true>>(LOO_LDS_MAX_S * 4);
    if (e != hipSuccess) return e;
    k_loo_row<true><<<p.Nt, LOO_NT, (size_t)p.S * 4, st>>>(p);
  } else {
    k_loo_row<false><<<p.Nt, LOO_NT, 0, st>>>(p);
  }
  return hipGetLastError();
}

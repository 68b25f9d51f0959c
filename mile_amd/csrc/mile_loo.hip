// PSIS-LOO / WAIC kernels (mile_loo.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_device.h"
#include "mile_loo.h"
#include "mile_loo_device.h"

__global__ __launch_bounds__(256) void k_loo_pack(const LooParams p) {
  __shared__ float tile[LOO_TILE][LOO_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int r0 = blockIdx.x * LOO_TILE, sl = blockIdx.y, row = r0 + tx;
  const int S = p.S, Nt = p.Nt;
  const int s_tiles = (S + LOO_TILE - 1) / LOO_TILE;
  const int t0 = (int)(((long long)sl * s_tiles) / p.slices), t1 = (int)(((long long)(sl + 1) * s_tiles) / p.slices);
  const float qnan = __int_as_float(0x7fc00000);
  for (int t = t0; t < t1; ++t) {
    const int sb = t * LOO_TILE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // row tx of draws ty, ty + 8, ...: a half-wave reads 32 consecutive rows of one draw
      const int j = ty + 8 * k, s = sb + j;
      float v = qnan;
      if (s < S && row < Nt) {
        const float r = p.ll[(size_t)s * (size_t)p.ld + row];
        if (loo_finite(r)) v = r;
      }
      tile[j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // draw sb + tx of rows ty, ty + 8, ...: a half-wave writes 32 consecutive values of one row
      const int rr = ty + 8 * k, s = sb + tx;
      if (s < S && r0 + rr < Nt) p.pk[(size_t)(r0 + rr) * S + s] = tile[tx][rr];
    }
    __syncthreads();
  }
}

// (LooStat, the workgroup sums and maxima and loo_bitonic: mile_loo_device.h.  k_loo_row keeps its own text of the stages that
// header also offers as device functions: its machine code, and with it every bit of its outputs, stays what it was.)
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
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int S = p.S;
  const float *g = p.pk + (size_t)n * S;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  auto val = [&](int i) -> float {
    if constexpr (LDS) return loo_row[i];
    else return g[i];
  };

  // 1. kept count, min, mean and M2, log-sum-exp
  LooStat st{0, 0.0, 0.0, -INFINITY, 0.0, INFINITY};
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = g[i];
    if constexpr (LDS) loo_row[i] = v;
    if (v == v) loo_stat_add(st, (double)v);
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {     // lane l takes lanes l + o's block: elements stay in lane order
    LooStat b;
    b.n = __shfl_down(st.n, o); b.mean = __shfl_down(st.mean, o); b.M2 = __shfl_down(st.M2, o);
    b.m = __shfl_down(st.m, o); b.s = __shfl_down(st.s, o); b.lo = __shfl_down(st.lo, o);
    if ((lane & (2 * o - 1)) == 0) loo_stat_merge(st, b);
  }
  if (lane == 0) wst[wv] = st;
  __syncthreads();     // (also: the row is in LDS)
  st = wst[0];
#pragma unroll
  for (int w = 1; w < LOO_NW; ++w) loo_stat_merge(st, wst[w]);
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
  const int M = kept == S ? p.M_full : (int)ceil(fmin((double)kept / 5.0, 3.0 * sqrt((double)kept / p.r_eff)));
  if (M < 1 || M > LOO_MAX_TAIL || M + 1 > kept) {     // cannot happen: M(kept) <= M(S) <= LOO_MAX_TAIL is checked on the host
    if (tid == 0) {
      if (p.elpd_loo) p.elpd_loo[n] = qnan;
      if (p.khat) p.khat[n] = qnan;
    }
    return;
  }
  const double lmin = st.lo, mx = -lmin;     // r = -l - max(-l)

  // 2. the (M+1)-th smallest key
  uint32_t prefix = 0, mask = 0, rank = (uint32_t)M + 1, below = 0, neq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;     // (LOO_NT == 256 bins)
    __syncthreads();
    for (int i = tid; i < S; i += LOO_NT) {
      const float v = val(i);
      if (v == v) {
        const uint32_t k = loo_key(v);
        if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t c = 0, b = 0, h = hist[0];
      while (c + h < rank && b < 255u) { c += h; h = hist[++b]; }
      sel[0] = b; sel[1] = rank - c; sel[2] = c; sel[3] = h;
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 255u << shift;
    rank = sel[1];
    below += sel[2];
    neq = sel[3];
  }
  const uint32_t T = prefix;                 // `below` keys are smaller, `neq` equal; the tail takes rank - 1 of the equal ones
  const int n_low = (int)below;              // (= M - (rank - 1))
  const double tie_body = (double)(neq - (rank - 1));

  // 3. the tail's keys, sorted
  if (tid == 0) tail_cnt = 0;
  __syncthreads();
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = val(i);
    if (v == v) {
      const uint32_t k = loo_key(v);
      if (k < T) {
        const uint32_t slot = atomicAdd(&tail_cnt, 1u);
        if (slot < (uint32_t)LOO_MAX_TAIL) tkey[slot] = k;
      }
    }
  }
  int P = 1;
  while (P < M) P <<= 1;
  for (int i = n_low + tid; i < P; i += LOO_NT) tkey[i] = i < M ? T : 0xffffffffu;
  __syncthreads();
  loo_bitonic(tkey, P, tid);

  // 4. the exceedances, ascending
  const double r_T = -(double)loo_unkey(T) - mx;
  const double cut = fmax(r_T, LOO_LOG_DBL_MIN), ec = exp(cut);
  for (int i = tid; i < M; i += LOO_NT) tx[i] = exp(-(double)loo_unkey(tkey[M - 1 - i]) - mx) - ec;
  __syncthreads();
  const double fM = (double)M;
  bool fit = false;
  double khat = qnan, sigma = qnan;
  const int q = (M + 2) >> 2;     // floor(M / 4 + 0.5), 1-based; 0 only below the smallest M that is fitted
  const double xq = tx[q > 0 ? q - 1 : 0], xM = tx[M - 1];
  if (M >= 5 && xq > 0.0) {
    int rt = (int)sqrt(fM);
    while (rt * rt > M) --rt;
    while ((rt + 1) * (rt + 1) <= M) ++rt;
    const int m = 30 + rt;
    for (int j = wv; j < m; j += LOO_NW) {
      const double bj = (1.0 - sqrt((double)m / ((double)(j + 1) - 0.5))) / (3.0 * xq) + 1.0 / xM;
      double acc = 0.0;
      for (int i = lane; i < M; i += 64) acc += log1p(-bj * tx[i]);
      const double kj = loo_wave_sum(acc) / fM;
      if (lane == 0) { cb[j] = bj; cL[j] = fM * (log(-bj / kj) - kj - 1.0); }
    }
    __syncthreads();
    // 5. weights, b, k, sigma, khat
    if (tid < m) {
      const double Lj = cL[tid];
      double sum = 0.0;
      for (int i = 0; i < m; ++i) sum += exp(cL[i] - Lj);
      cw[tid] = 1.0 / sum;
    }
    __syncthreads();
    double b = 0.0;
    for (int j = 0; j < m; ++j) b += cb[j] * cw[j];
    double acc = 0.0;
    for (int i = tid; i < M; i += LOO_NT) acc += log1p(-b * tx[i]);
    const double k = loo_block_sum(acc, red) / fM;
    sigma = -k / b;
    khat = (fM * k + 5.0) / (fM + 10.0);
    fit = fabs(khat) <= 1.7976931348623157e308 && fabs(sigma) <= 1.7976931348623157e308;
    if (!fit) khat = qnan;
  }
  if (tid == 0 && p.khat) p.khat[n] = khat;
  if (!p.elpd_loo) return;
  __syncthreads();     // every read of x is done: lw takes its place

  // the smoothed tail, and the maxima the two log-sum-exps are shifted by
  double mlw = r_T, ma = lmin;     // the body: lw = r <= r_T, lw + l = lmin up to rounding
  for (int i = tid; i < M; i += LOO_NT) {
    const double l = (double)loo_unkey(tkey[M - 1 - i]);
    double lw;
    if (fit) {
      const double lp = log1p(-((double)(i + 1) - 0.5) / fM);
      const double q = khat == 0.0 ? -sigma * lp : sigma * expm1(-khat * lp) / khat;
      lw = log(q + ec);
    } else {
      lw = -l - mx;
    }
    lw = lw > 0.0 ? 0.0 : lw;
    tx[i] = lw;
    mlw = fmax(mlw, lw);
    ma = fmax(ma, lw + l);
  }
  mlw = loo_block_max(mlw, red);
  ma = loo_block_max(ma, red);

  // 6. the body from the row, the tail from LDS
  double s1 = 0.0, s2 = 0.0;
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = val(i);
    if (v == v && loo_key(v) > T) {
      const double l = (double)v, r = -l - mx;
      s1 += exp(r - mlw);
      s2 += exp((r + l) - ma);
    }
  }
  for (int i = tid; i < M; i += LOO_NT) {
    const double l = (double)loo_unkey(tkey[M - 1 - i]), lw = tx[i];
    s1 += exp(lw - mlw);
    s2 += exp((lw + l) - ma);
  }
  s1 = loo_block_sum(s1, red);
  s2 = loo_block_sum(s2, red);
  if (tid == 0) {
    const double lT = (double)loo_unkey(T);
    s1 += tie_body * exp(r_T - mlw);
    s2 += tie_body * exp((r_T + lT) - ma);
    p.elpd_loo[n] = (ma + log(s2)) - (mlw + log(s1));
  }
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

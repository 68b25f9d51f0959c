// Device code of the PSIS kernels, shared by mile_loo.hip (k_loo_pack, k_loo_row) and mile_lxp.hip (k_lxp_pack, k_lxp_row): the
// pack's transpose, a row's running statistics and their merge, and the stages of one row (mile_loo.h numbers them) as device
// functions of a workgroup of LOO_NT threads.  Both row kernels are built from these stages: this is their one text, so the two
// write the same bits for the same row.  The workgroup primitives are mile_block.h's.  Every function that holds a barrier is
// called by all threads of the workgroup with the same arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mile_block.h"
#include "mile_loo.h"

#define LOO_LOG_DBL_MIN (-708.39641853226410622)   // log(DBL_MIN)

// The pack of a tile of Nt rows: workgroup (x, y) of 256 threads transposes slice y of the draws of rows 32 x .. 32 x + 31 into
// pk [Nt][S], through LDS in 32 x 32 pieces; load(draw, row) is the value, and one that is not finite is packed as NaN.
template <class Load>
__device__ __forceinline__ void loo_pack_tile(float *pk, int S, int Nt, int slices, Load load) {
  __shared__ float tile[LOO_TILE][LOO_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int r0 = blockIdx.x * LOO_TILE, sl = blockIdx.y, row = r0 + tx;
  const int s_tiles = (S + LOO_TILE - 1) / LOO_TILE;
  const int t0 = (int)(((long long)sl * s_tiles) / slices), t1 = (int)(((long long)(sl + 1) * s_tiles) / slices);
  const float qnan = __int_as_float(0x7fc00000);
  for (int t = t0; t < t1; ++t) {
    const int sb = t * LOO_TILE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // row tx of draws ty, ty + 8, ...: a half-wave reads 32 consecutive rows of one draw
      const int j = ty + 8 * k, s = sb + j;
      float v = qnan;
      if (s < S && row < Nt) {
        const float r = load(s, row);
        if (finite_f32(r)) v = r;
      }
      tile[j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // draw sb + tx of rows ty, ty + 8, ...: a half-wave writes 32 consecutive values of one row
      const int rr = ty + 8 * k, s = sb + tx;
      if (s < S && r0 + rr < Nt) pk[(size_t)(r0 + rr) * S + s] = tile[tx][rr];
    }
    __syncthreads();
  }
}

// a thread's, wave's or row's running statistics of the kept l: count, Welford mean and M2, streaming log-sum-exp (m, s), min
struct LooStat {
  int n;
  double mean, M2, m, s, lo;
};
__device__ __forceinline__ void loo_stat_add(LooStat &a, double x) {
  ++a.n;
  const double d = x - a.mean;
  a.mean += d / (double)a.n;
  a.M2 += d * (x - a.mean);
  if (x > a.m) { a.s = a.s * exp(a.m - x) + 1.0; a.m = x; }
  else a.s += exp(x - a.m);
  a.lo = fmin(a.lo, x);
}
// Chan's merge of b into a (a before b)
__device__ __forceinline__ void loo_stat_merge(LooStat &a, const LooStat &b) {
  if (b.n == 0) return;
  if (a.n == 0) { a = b; return; }
  const double na = (double)a.n, nb = (double)b.n, nn = na + nb, d = b.mean - a.mean;
  a.mean += d * (nb / nn);
  a.M2 += b.M2 + d * d * (na * nb / nn);
  const double mm = fmax(a.m, b.m);
  a.s = a.s * exp(a.m - mm) + b.s * exp(b.m - mm);
  a.m = mm;
  a.lo = fmin(a.lo, b.lo);
  a.n += b.n;
}

// ---- the stages of one row ------------------------------------------------------------------------------------------------------
// 1. kept count, min, mean and M2, log-sum-exp of the row g [S] (NaN: a draw left out); <true> also keeps the row in LDS.  Ends
// on a barrier: the row is in LDS.
template <bool LDS>
__device__ __forceinline__ LooStat loo_row_stats(const float *g, float *row, int S, LooStat *wst) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  LooStat st{0, 0.0, 0.0, -INFINITY, 0.0, INFINITY};
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = g[i];
    if constexpr (LDS) row[i] = v;
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
  __syncthreads();
  st = wst[0];
#pragma unroll
  for (int w = 1; w < LOO_NW; ++w) loo_stat_merge(st, wst[w]);
  return st;     // (the same in every thread)
}

// the tail length of a row that keeps `kept` of its S draws; outside [1, min(LOO_MAX_TAIL, kept - 1)] cannot happen (the host checks M(S))
__device__ __forceinline__ int loo_row_tail_length(int kept, int S, int M_full, double r_eff) {
  return kept == S ? M_full : (int)ceil(fmin((double)kept / 5.0, 3.0 * sqrt((double)kept / r_eff)));
}

// 2. the (M+1)-th smallest key T of the row val(0 .. S): n_low keys are smaller and neq equal, of which the tail takes n_tie
struct LooCut { uint32_t T; int n_low, n_tie, neq; };
template <class Val>
__device__ __forceinline__ LooCut loo_row_select(Val val, int S, int M, uint32_t *hist, uint32_t *sel) {
  const int tid = threadIdx.x;
  uint32_t prefix = 0, mask = 0, rank = (uint32_t)M + 1, below = 0, neq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0;     // (LOO_NT == 256 bins)
    __syncthreads();
    for (int i = tid; i < S; i += LOO_NT) {
      const float v = val(i);
      if (v == v) {
        const uint32_t k = f32_key(v);
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
  return LooCut{prefix, (int)below, (int)(rank - 1), (int)neq};     // (n_low + n_tie == M)
}

// 3. the tail's keys in tkey [0, M), ascending: the n_low keys below T, then n_tie copies of T
template <class Val>
__device__ __forceinline__ void loo_row_sort_tail(Val val, int S, int M, const LooCut &c, uint32_t *tkey, uint32_t *tail_cnt) {
  const int tid = threadIdx.x;
  if (tid == 0) *tail_cnt = 0;
  __syncthreads();
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = val(i);
    if (v == v) {
      const uint32_t k = f32_key(v);
      if (k < c.T) {
        const uint32_t slot = atomicAdd(tail_cnt, 1u);
        if (slot < (uint32_t)LOO_MAX_TAIL) tkey[slot] = k;
      }
    }
  }
  int P = 1;
  while (P < M) P <<= 1;
  for (int i = c.n_low + tid; i < P; i += LOO_NT) tkey[i] = i < M ? c.T : 0xffffffffu;
  __syncthreads();
  bitonic(tkey, P, tid, LOO_NT);
}

// 4. and 5. the exceedances x_i = exp(r_(i)) - ec into tx [0, M), ascending (tx[i] belongs to tkey[M - 1 - i]), and the fit
struct LooFit { bool fit; double khat, sigma; };
__device__ __forceinline__ LooFit loo_row_fit(int M, const uint32_t *tkey, double *tx, double mx, double ec, double *cb, double *cL, double *cw,
                                              double *red) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  for (int i = tid; i < M; i += LOO_NT) tx[i] = exp(-(double)f32_unkey(tkey[M - 1 - i]) - mx) - ec;
  __syncthreads();
  const double fM = (double)M;
  LooFit f{false, qnan, qnan};
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
      const double kj = wave_sum(acc) / fM;
      if (lane == 0) { cb[j] = bj; cL[j] = fM * (log(-bj / kj) - kj - 1.0); }
    }
    __syncthreads();
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
    const double k = block_sum<LOO_NW>(acc, red) / fM;
    f.sigma = -k / b;
    f.khat = (fM * k + 5.0) / (fM + 10.0);
    f.fit = fabs(f.khat) <= 1.7976931348623157e308 && fabs(f.sigma) <= 1.7976931348623157e308;
    if (!f.fit) f.khat = qnan;
  }
  return f;
}

// The smoothed tail lw_i = min(., 0) in place of x_i (behind a barrier: every read of x is done), and the maxima the two
// log-sum-exps are shifted by: mlw of lw (from r_T, the body's largest) and ma of lw + l (from lmin, the body's up to rounding).
__device__ __forceinline__ void loo_row_smooth(int M, const uint32_t *tkey, double *tx, const LooFit &f, double mx, double ec, double &mlw,
                                               double &ma, double *red) {
  const int tid = threadIdx.x;
  const double fM = (double)M;
  __syncthreads();
  for (int i = tid; i < M; i += LOO_NT) {
    const double l = (double)f32_unkey(tkey[M - 1 - i]);
    double lw;
    if (f.fit) {
      const double lp = log1p(-((double)(i + 1) - 0.5) / fM);
      const double q = f.khat == 0.0 ? -f.sigma * lp : f.sigma * expm1(-f.khat * lp) / f.khat;
      lw = log(q + ec);
    } else {
      lw = -l - mx;
    }
    lw = lw > 0.0 ? 0.0 : lw;
    tx[i] = lw;
    mlw = fmax(mlw, lw);
    ma = fmax(ma, lw + l);
  }
  mlw = block_max<LOO_NW>(mlw, red);
  ma = block_max<LOO_NW>(ma, red);
}

// 6. s1 = sum exp(lw - mlw) and s2 = sum exp(lw + l - ma) over the kept draws: the body from the row, the tail from LDS, the copies
// of T that the tail did not take added last; the same bits in every thread
template <class Val>
__device__ __forceinline__ void loo_row_sums(Val val, int S, int M, const LooCut &c, const uint32_t *tkey, const double *tx, double mx, double r_T,
                                             double mlw, double ma, double &s1, double &s2, double *red) {
  const int tid = threadIdx.x;
  s1 = 0.0; s2 = 0.0;
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = val(i);
    if (v == v && f32_key(v) > c.T) {
      const double l = (double)v, r = -l - mx;
      s1 += exp(r - mlw);
      s2 += exp((r + l) - ma);
    }
  }
  for (int i = tid; i < M; i += LOO_NT) {
    const double l = (double)f32_unkey(tkey[M - 1 - i]), lw = tx[i];
    s1 += exp(lw - mlw);
    s2 += exp((lw + l) - ma);
  }
  s1 = block_sum<LOO_NW>(s1, red);
  s2 = block_sum<LOO_NW>(s2, red);
  const double lT = (double)f32_unkey(c.T), tie_body = (double)(c.neq - c.n_tie);
  s1 += tie_body * exp(r_T - mlw);
  s2 += tie_body * exp((r_T + lT) - ma);
}

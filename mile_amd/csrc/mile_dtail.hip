// Tail-diagnostics kernels (mile_dtail.h) in a translation unit of their own.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_device.h"
#include "mile_diag_device.h"
#include "mile_dtail.h"

// ---- k_dtail_derive: one workgroup of DIAG_POOL_NT per parameter ------------------------------------------------------------
// The sort and the scores are k_diag_pool_rank's, statement for statement, so z holds its bits.
__global__ __launch_bounds__(DIAG_POOL_NT) void k_dtail_derive(DtailParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dtail_smem[];
  __shared__ float med;
  uint64_t *a = (uint64_t *)dtail_smem;
  const int tid = threadIdx.x, n = p.C * p.S;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  const long long base = (long long)blockIdx.x * n, col = p.p0 + blockIdx.x;
  const float *src = p.x + base;
  float *z = p.z + base, *zf = p.want_zf ? p.zf + base : nullptr;
  const float qnan = __int_as_float(0x7fc00000);
  int nan = 0;
  for (int i = tid; i < n2; i += DIAG_POOL_NT) {
    if (i < n) {
      const float x = src[i];
      nan |= x != x;
      a[i] = ((uint64_t)diag_key(x) << 32) | (uint32_t)i;
    } else {
      a[i] = ~0ull;
    }
  }
  if (__syncthreads_or(nan)) {      // a NaN draw has no rank: no score, no order statistic
    for (int i = tid; i < n; i += DIAG_POOL_NT) {
      z[i] = qnan;
      if (zf) zf[i] = qnan;
    }
    if (tid == 0) {
      p.thr[2 * blockIdx.x] = p.thr[2 * blockIdx.x + 1] = qnan;
      if (p.quantiles) p.quantiles[col] = p.quantiles[p.d + col] = p.quantiles[2 * p.d + col] = qnan;
    }
    return;
  }
  bitonic(a, n2, tid, DIAG_POOL_NT);
  for (int i = tid; i < n; i += DIAG_POOL_NT) z[(uint32_t)a[i]] = (float)diag_rank_score(a, n, i);
  if (tid == 0) {                   // integer indices only: ceil(n/20) - 1, ceil(19n/20) - 1, and the two middle draws
    const float q_lo = src[(uint32_t)a[(n + 19) / 20 - 1]], q_hi = src[(uint32_t)a[(19 * n + 19) / 20 - 1]];
    const float m32 = (float)(((double)src[(uint32_t)a[(n - 1) / 2]] + (double)src[(uint32_t)a[n / 2]]) / 2.0);
    p.thr[2 * blockIdx.x] = q_lo;
    p.thr[2 * blockIdx.x + 1] = q_hi;
    if (p.quantiles) { p.quantiles[col] = q_lo; p.quantiles[p.d + col] = q_hi; p.quantiles[2 * p.d + col] = m32; }
    med = m32;
  }
  __syncthreads();                  // the median is known, and every read of the sorted draws is done
  if (!zf) return;
  const float m = med;
  nan = 0;
  for (int i = tid; i < n2; i += DIAG_POOL_NT) {
    if (i < n) {
      const float f = fabsf(src[i] - m);           // inf - inf: a folded draw without a rank
      nan |= f != f;
      a[i] = ((uint64_t)diag_key(f) << 32) | (uint32_t)i;
    } else {
      a[i] = ~0ull;
    }
  }
  if (__syncthreads_or(nan)) {
    for (int i = tid; i < n; i += DIAG_POOL_NT) zf[i] = qnan;
    return;
  }
  bitonic(a, n2, tid, DIAG_POOL_NT);
  for (int i = tid; i < n; i += DIAG_POOL_NT) zf[(uint32_t)a[i]] = (float)diag_rank_score(a, n, i);
}

// ---- k_dtail_ess: one workgroup of 256 per (parameter, series) -----------------------------------------------------------------
// Draw i of a series, in fp64: a plane's float, or the 0 / 1 of the raw draw against the series' threshold.
__device__ __forceinline__ double dtail_value(const float *col, bool indicator, float thr, int i) {
  const float x = col[i];
  return indicator ? (x <= thr ? 1.0 : 0.0) : (double)x;
}
// The mean of v[0, len) by one wave: lane-strided sums, then the xor-shuffles.  The one statement of a piece mean, so the
// first pass (from the plane) and every staging of the piece (from LDS) give the same bits.
template <class V>
__device__ __forceinline__ double dtail_piece_mean(V v, int len, int lane) {
  double s = 0.0;
  for (int t = lane; t < len; t += 64) s += v(t);
  return wave_sum(s) / (double)len;
}

__global__ __launch_bounds__(DTAIL_ESS_NT) void k_dtail_ess(DtailParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dtail_smem[];
  const int ser = p.ess_plain ? 3 : (int)blockIdx.y;
  if (!((p.series >> ser) & 1u)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
  const int len = p.S / p.n_splits, n = p.C * p.S, M = p.C * p.n_splits;
  double *xc = (double *)dtail_smem, *ac = xc + DTAIL_STAGE, *red = ac + len, *part = red + 8;
  const bool ind = ser == 1 || ser == 2;
  const float *col = (ser == 0 ? p.z : p.x) + (long long)q * n;
  const float thr = ind ? p.thr[2 * q + (ser - 1)] : 0.0f;
  const double fn = (double)n, fl = (double)len;

  // First pass: the mean of all draws, the ddof-1 variance of the piece means about it (their mean: the pieces are equal in
  // length), and for the raw series the sd of the pooled draws.
  double s = 0.0;
  for (int i = tid; i < n; i += DTAIL_ESS_NT) s += dtail_value(col, ind, thr, i);
  const double G = block_sum<4>(s, red) / fn;
  double as = 0.0;
  for (int m = wave; m < M; m += DTAIL_ESS_NT / 64) {
    const float *pc = col + (long long)m * len;
    const double mk = dtail_piece_mean([&](int t) { return dtail_value(pc, ind, thr, t); }, len, lane);
    as += (mk - G) * (mk - G);
  }
  if (lane == 0) red[wave] = as;
  __syncthreads();
  const double between = M > 1 ? (((red[0] + red[1]) + red[2]) + red[3]) / (double)(M - 1) : 0.0;
  __syncthreads();
  if (ser == 3) {
    double s2 = 0.0;
    for (int i = tid; i < n; i += DTAIL_ESS_NT) { const double e = (double)col[i] - G; s2 += e * e; }
    const double sd = sqrt(block_sum<4>(s2, red) / (fn - 1.0));
    if (tid == 0 && p.res) p.res[(long long)q * DTAIL_NRES + 4] = sd;
  }

  // mean_acov[k] = sum over the pieces of sum_t xc[t] xc[t+k] / (len * M), xc the piece about its own mean, by direct
  // summation, 64 lags (32 Geyer pairs) at a time: whole pieces staged in LDS, a wave centring each, then a wave per quarter of
  // the t range and a lane per lag, pieces in index order.  No further block once one holds a pair sum that is not positive.
  const int len_even = len & ~1, T = len_even >> 1, lag = lane, seg = wave;
  const int per_stage = DTAIL_STAGE / len > 0 ? DTAIL_STAGE / len : 1;
  double wv = 0.0, v0 = 0.0;
  int nlag = 0;
  for (int k0 = 0; k0 < len_even; k0 += 64) {
    const int k = k0 + lag;
    double acc = 0.0;
    for (int m0 = 0; m0 < M; m0 += per_stage) {
      const int g = min(per_stage, M - m0), cnt = g * len;
      const float *pc = col + (long long)m0 * len;
      for (int i = tid; i < cnt; i += DTAIL_ESS_NT) xc[i] = dtail_value(pc, ind, thr, i);
      __syncthreads();
      for (int j = wave; j < g; j += DTAIL_ESS_NT / 64) {
        double *xj = xc + j * len;
        const double mk = dtail_piece_mean([&](int t) { return xj[t]; }, len, lane);
        for (int t = lane; t < len; t += 64) xj[t] -= mk;
      }
      __syncthreads();
      if (k < len_even)
        for (int j = 0; j < g; ++j) {
          const double *xj = xc + j * len;
          for (int t = seg; t < len - k; t += DTAIL_ESS_NT / 64) acc += xj[t] * xj[t + k];
        }
      __syncthreads();
    }
    part[seg * 64 + lag] = acc;
    __syncthreads();
    if (seg == 0 && k < len_even) ac[k] = (((part[lag] + part[64 + lag]) + part[128 + lag]) + part[192 + lag]) / (fl * (double)M);
    __syncthreads();
    if (k0 == 0) { v0 = ac[0] * fl / (fl - 1.0); wv = ac[0] + between; }
    nlag = min(k0 + 64, len_even);
    int stop = !(wv > 0.0 && wv < INFINITY);
    const int t = (k0 >> 1) + lag;
    if (seg == 0 && lag < 32 && t < T) {
      const double re = t == 0 ? 1.0 : 1.0 - (v0 - ac[2 * t]) / wv, ro = 1.0 - (v0 - ac[2 * t + 1]) / wv;
      stop |= !(re + ro > 0.0);
    }
    if (__syncthreads_or(stop)) break;
  }
  // Lane 0 alone walks the pairs kept, as in k_diag_chain.
  if (tid == 0) {
    double ess = __longlong_as_double(0x7ff8000000000000ll);       // weighted_var not a positive finite number: NaN
    if (wv > 0.0 && wv < INFINITY) {
      auto rho = [&](int k) { return k == 0 ? 1.0 : 1.0 - (v0 - ac[k]) / wv; };
      const int Tc = nlag >> 1;                      // pairs computed
      int t_star = T;                                // first pair whose sum is not positive (T: none)
      for (int t = 0; t < Tc; ++t)
        if (!(rho(2 * t) + rho(2 * t + 1) > 0.0)) { t_star = t; break; }
      const int max_t = t_star > 0 ? t_star - 1 : 0;
      const int nxt = min(max_t + 1, T - 1);
      const bool in_range = max_t + 1 <= T - 1;
      double sum = 0.0, prev = 0.0, last = 0.0;
      for (int t = 0; t <= nxt; ++t) {
        const bool m = t < t_star;
        const double re = rho(2 * t);
        const bool me = (t == nxt && in_range) ? re > 0.0 : m;
        const double ev = me ? re : 0.0, od = m ? rho(2 * t + 1) : 0.0, rs = ev + od;
        if (t == 0) prev = rs;
        const bool um = rs > prev;                   // initial monotone sequence
        const double cur = um ? prev : rs;
        const double ef = um ? 0.5 * cur : ev, of = um ? 0.5 * cur : od;
        sum += ef + of;
        if (t == nxt) last = ef;
        prev = cur;
      }
      double tau = -1.0 + 2.0 * sum - last;
      const double floor_ = 1.0 / log10(fn);
      if (tau < floor_) tau = floor_;
      ess = fn / tau;
    }
    if (p.ess_plain) p.ess_plain[p.p0 + q] = (float)ess;
    else p.res[(long long)q * DTAIL_NRES + ser] = ess;
  }
}

// ---- k_dtail_final: one thread per parameter --------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_dtail_final(DtailParams p) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= p.P) return;
  const double *r = p.res + (long long)q * DTAIL_NRES;
  const long long col = p.p0 + q;
  if (p.ess_bulk) p.ess_bulk[col] = (float)r[0];
  if (p.ess_tail) p.ess_tail[col] = (r[1] != r[1] || r[2] != r[2]) ? __int_as_float(0x7fc00000) : (float)fmin(r[1], r[2]);
  if (p.ess_mean) p.ess_mean[col] = (float)r[3];
  if (p.mcse_mean) p.mcse_mean[col] = (float)(r[4] / sqrt(r[3]));
}

hipError_t mile_launch_dtail_derive(const DtailParams &p, hipStream_t st) {
  hipError_t e = mile_set_max_lds<k_dtail_derive>((int)diag_pool_lds(DIAG_POOL_MAX));
  if (e != hipSuccess) return e;
  k_dtail_derive<<<p.P, DIAG_POOL_NT, diag_pool_lds(p.C * p.S), st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_dtail_ess(const DtailParams &p, hipStream_t st) {
  hipError_t e = mile_set_max_lds<k_dtail_ess>((int)dtail_ess_lds(DIAG_S_MAX));
  if (e != hipSuccess) return e;
  k_dtail_ess<<<dim3(p.P, p.ess_plain ? 1 : DTAIL_NSER), DTAIL_ESS_NT, dtail_ess_lds(p.S / p.n_splits), st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_dtail_final(const DtailParams &p, hipStream_t st) {
  k_dtail_final<<<(p.P + 63) / 64, 64, 0, st>>>(p);
  return hipGetLastError();
}

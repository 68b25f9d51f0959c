// Posterior-predictive moment kernels (mile_moments.h) in a translation unit of their own: they compile concurrently with
// mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_block.h"
#include "mile_moments.h"

// p log p with the product rounded on its own (no contraction into the sum that follows): a draw's entropy and the
// entropy of a one-draw mean are then the same arithmetic, and their difference is exactly 0
__device__ __forceinline__ double mom_plogp(double p) { return p > 0.0 ? __dmul_rn(p, log(p)) : 0.0; }

// Chan's merge of (nb, mb, M2b) into (na, ma, M2a); nb > 0
__device__ __forceinline__ void mom_chan(int &na, double &ma, double &M2a, int nb, double mb, double M2b) {
  if (na == 0) { na = nb; ma = mb; M2a = M2b; return; }
  const double nt = (double)na + (double)nb, delta = mb - ma;
  ma += delta * ((double)nb / nt);
  M2a += M2b + delta * delta * ((double)na * (double)nb / nt);
  na += nb;
}

template <int TASK>
__global__ __launch_bounds__(MOM_NT) void k_moments_accum(const MomParams p) {
  const int n = blockIdx.x * MOM_NT + threadIdx.x, sl = blockIdx.y;
  if (n >= p.N) return;
  const int N = p.N;
  const int s0 = (int)(((long long)sl * p.Sc) / p.slices), s1 = (int)(((long long)(sl + 1) * p.Sc) / p.slices);
  if (s1 <= s0) return;
  int32_t *cnt = p.cnt + (size_t)sl * N + n;

  if constexpr (TASK == MILE_TASK_REGRESSION) {
    double *acc = p.acc + (size_t)sl * 3 * N + n;
    const float2 *r = (const float2 *)p.raw + (size_t)s0 * N + n;    // (mu, log sigma) of row n: 8 B per lane, contiguous
    int c = 0;
    double mean = 0.0, M2 = 0.0, sv = 0.0;
#pragma unroll 4
    for (int s = s0; s < s1; ++s, r += N) {
      const float2 v = *r;
      if (finite_f32(v.x) && finite_f32(v.y)) {
        ++c;
        const double x = (double)v.x, d = x - mean;
        mean += d / (double)c;
        M2 += d * (x - mean);
        const double sig = fmin(fmax(exp((double)v.y), 1e-6), 1e6);
        sv += sig * sig;
      }
    }
    if (c == 0) return;
    int ca = *cnt;
    double ma = acc[0], M2a = acc[N];
    mom_chan(ca, ma, M2a, c, mean, M2);
    *cnt = ca; acc[0] = ma; acc[N] = M2a; acc[2 * (size_t)N] += sv;
  } else {
    const int K = p.O;
    double *acc = p.acc + (size_t)sl * (K + 1) * N + n;
    for (int k0 = 0; k0 < K; k0 += MOM_KC) {      // (K <= 16: one trip, one exp per logit)
      double a[MOM_KC];
#pragma unroll
      for (int j = 0; j < MOM_KC; ++j) a[j] = 0.0;
      double hs = 0.0;
      int c = 0;
      for (int s = s0; s < s1; ++s) {
        const float *x = p.raw + ((size_t)s * N + n) * K;
        float m = x[0];
        bool fin = finite_f32(m);
        for (int k = 1; k < K; ++k) { const float v = x[k]; fin = fin && finite_f32(v); m = fmaxf(m, v); }
        if (!fin) continue;
        const double md = (double)m;
        // sum of exp(x - m) over k = 0 .. K-1 in that order in every trip, the trip's own classes kept in registers
        double se = 0.0, e[MOM_KC];
        for (int k = 0; k < k0; ++k) se += exp((double)x[k] - md);
#pragma unroll
        for (int j = 0; j < MOM_KC; ++j) {
          e[j] = 0.0;
          if (k0 + j < K) { e[j] = exp((double)x[k0 + j] - md); se += e[j]; }
        }
        for (int k = k0 + MOM_KC; k < K; ++k) se += exp((double)x[k] - md);
        const double inv = 1.0 / se;
        ++c;
#pragma unroll
        for (int j = 0; j < MOM_KC; ++j) {
          if (k0 + j < K) {
            const double pk = e[j] * inv;
            a[j] += pk;
            if (k0 == 0) hs -= mom_plogp(pk);
          }
        }
        if (k0 == 0)
          for (int k = MOM_KC; k < K; ++k) hs -= mom_plogp(exp((double)x[k] - md) * inv);
      }
#pragma unroll
      for (int j = 0; j < MOM_KC; ++j)
        if (k0 + j < K) acc[(size_t)(k0 + j) * N] += a[j];
      if (k0 == 0) { acc[(size_t)K * N] += hs; *cnt += c; }
    }
  }
}

template <int TASK>
__global__ __launch_bounds__(MOM_NT) void k_moments_finish(const MomParams p) {
  const int n = blockIdx.x * MOM_NT + threadIdx.x;
  if (n >= p.N) return;
  const int N = p.N;
  const float qnan = __int_as_float(0x7fc00000);
  if constexpr (TASK == MILE_TASK_REGRESSION) {
    int c = 0;
    double mean = 0.0, M2 = 0.0, sv = 0.0;
    for (int sl = 0; sl < p.slices; ++sl) {
      const int cb = p.cnt[(size_t)sl * N + n];
      if (cb == 0) continue;
      const double *acc = p.acc + (size_t)sl * 3 * N + n;
      mom_chan(c, mean, M2, cb, acc[0], acc[N]);
      sv += acc[2 * (size_t)N];
    }
    float *o = p.out + (size_t)n * 3;
    o[0] = c ? (float)mean : qnan;
    o[1] = c ? (float)(M2 / (double)c) : qnan;
    o[2] = c ? (float)(sv / (double)c) : qnan;
    if (p.dropped) p.dropped[n] = (int32_t)(p.S - c);
  } else {
    const int K = p.O;
    long long c = 0;
    for (int sl = 0; sl < p.slices; ++sl) c += p.cnt[(size_t)sl * N + n];
    float *o = p.out + (size_t)n * (K + 2);
    if (p.dropped) p.dropped[n] = (int32_t)(p.S - c);
    if (c == 0) {
      for (int k = 0; k < K + 2; ++k) o[k] = qnan;
      return;
    }
    const double fc = (double)c;
    double h = 0.0, hs = 0.0;
    for (int k = 0; k <= K; ++k) {
      double t = 0.0;
      for (int sl = 0; sl < p.slices; ++sl) t += p.acc[((size_t)sl * (K + 1) + k) * N + n];
      if (k < K) {
        const double pk = t / fc;
        o[k] = (float)pk;
        h -= mom_plogp(pk);
      } else {
        hs = t / fc;
      }
    }
    o[K] = (float)h;
    o[K + 1] = (float)fmax(h - hs, 0.0);
  }
}

hipError_t mile_launch_moments_accum(int task, const MomParams &p, hipStream_t st) {
  const dim3 grid((p.N + MOM_NT - 1) / MOM_NT, p.slices);
  if (task == MILE_TASK_REGRESSION) k_moments_accum<MILE_TASK_REGRESSION><<<grid, MOM_NT, 0, st>>>(p);
  else k_moments_accum<MILE_TASK_CLASSIFICATION><<<grid, MOM_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_moments_finish(int task, const MomParams &p, hipStream_t st) {
  const dim3 grid((p.N + MOM_NT - 1) / MOM_NT);
  if (task == MILE_TASK_REGRESSION) k_moments_finish<MILE_TASK_REGRESSION><<<grid, MOM_NT, 0, st>>>(p);
  else k_moments_finish<MILE_TASK_CLASSIFICATION><<<grid, MOM_NT, 0, st>>>(p);
  return hipGetLastError();
}

// Streamed-LPPD kernels (mile_lppd.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_lppd.h"

// fold one value into a streaming log-sum-exp (m, s), s = sum exp(l - m); starts at (-inf, 0).  l is not NaN.
__device__ __forceinline__ void lppd_fold(double &m, double &s, double l) {
  if (l == -INFINITY) return;              // adds 0
  if (l == m) { s += 1.0; return; }        // equal infinities too: l - m would be NaN
  const double e = exp(-fabs(l - m));      // (an infinite distance: 0)
  if (l > m) { s = s * e + 1.0; m = l; }
  else s += e;
}

// sum over the wave's 64 lanes in a fixed tree; the total is in lane 0
__device__ __forceinline__ double lppd_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ long long lppd_wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

__global__ __launch_bounds__(LPPD_NT) void k_lppd_accum(const LppdParams p) {
  const int n = blockIdx.x * LPPD_NT + threadIdx.x, c = blockIdx.y;
  if (n >= p.N) return;
  const size_t i = (size_t)c * p.N + n;
  double2 ms = make_double2(-INFINITY, 0.0);
  int cnt = 0;
  if (!p.fresh) { ms = p.state[i]; cnt = p.cnt[i]; }
  const float *l = p.ll + ((size_t)c * p.J + p.ja) * p.N + n;
#pragma unroll 4
  for (int j = p.ja; j < p.jb; ++j, l += p.N) {
    const float v = *l;
    if (v != v) continue;                  // NaN: left out of this (chain, row); dropped = S - cnt
    ++cnt;
    lppd_fold(ms.x, ms.y, (double)v);
  }
  p.state[i] = ms;
  p.cnt[i] = cnt;
}

template <bool FINAL>
__global__ __launch_bounds__(LPPD_NT) void k_lppd_emit(const LppdParams p) {
  const int w = blockIdx.x, n = w * LPPD_NT + threadIdx.x;
  const bool valid = n < p.N;              // lanes past N add 0 to every sum (no early return: the shuffles need every lane)
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  double M = -INFINITY, T = 0.0;           // the row's log-sum-exp of A over the chains
  long long tot = 0;
  for (int c = 0; c < p.C; ++c) {
    double t = 0.0;
    long long k = 0;
    if (valid) {
      const size_t i = (size_t)c * p.N + n;
      const double2 ms = p.state[i];
      k = p.cnt[i];
      if (k > 0) {
        const double A = ms.x + log(ms.y);
        t = A - log((double)k);
        lppd_fold(M, T, A);
        tot += k;
      } else {
        t = qnan;
      }
    }
    t = lppd_wave_sum(t);
    if (FINAL) k = lppd_wave_sum(k);
    if (threadIdx.x == 0) {
      p.part_chain[(size_t)w * p.C + c] = t;
      if (FINAL) p.part_cnt[(size_t)w * p.C + c] = k;
    }
  }
  const double e = valid ? (tot > 0 ? M + log(T) - log((double)tot) : qnan) : 0.0;
  if (FINAL && valid && p.row_lppd) p.row_lppd[n] = e;
  const double es = lppd_wave_sum(e);
  if (threadIdx.x == 0) p.part_ens[w] = es;
}

// sum over the workgroup in a fixed LDS tree; every thread gets the total
__device__ __forceinline__ double lppd_block_sum(double v, double *red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int o = LPPD_FIN_NT / 2; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

template <bool FINAL>
__global__ __launch_bounds__(LPPD_FIN_NT) void k_lppd_finish(const LppdParams p) {
  __shared__ double red[LPPD_FIN_NT];
  const int t = threadIdx.x;
  const double fN = (double)p.N;
  double cs = 0.0;
  for (int c = t; c < p.C; c += LPPD_FIN_NT) {
    double a = 0.0;
    long long k = 0;
    for (int w = 0; w < p.waves; ++w) {
      a += p.part_chain[(size_t)w * p.C + c];
      if (FINAL) k += p.part_cnt[(size_t)w * p.C + c];
    }
    a /= fN;
    cs += a;
    if (FINAL && p.chain_lppd) p.chain_lppd[c] = a;
    if (FINAL && p.dropped) p.dropped[c] = p.S * (long long)p.N - k;
  }
  cs = lppd_block_sum(cs, red);
  double es = 0.0;
  for (int w = t; w < p.waves; w += LPPD_FIN_NT) es += p.part_ens[w];
  es = lppd_block_sum(es, red);
  if (t == 0) {
    if (p.point >= 0 && p.run_chain) p.run_chain[p.point] = cs / (double)p.C;
    if (p.point >= 0 && p.run_ens) p.run_ens[p.point] = es / fN;
    if (FINAL && p.lppd) p.lppd[0] = es / fN;
  }
}

hipError_t mile_launch_lppd_accum(const LppdParams &p, hipStream_t st) {
  k_lppd_accum<<<dim3(p.waves, p.C), LPPD_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_lppd_emit(const LppdParams &p, bool final, hipStream_t st) {
  if (final) {
    k_lppd_emit<true><<<p.waves, LPPD_NT, 0, st>>>(p);
    k_lppd_finish<true><<<1, LPPD_FIN_NT, 0, st>>>(p);
  } else {
    k_lppd_emit<false><<<p.waves, LPPD_NT, 0, st>>>(p);
    k_lppd_finish<false><<<1, LPPD_FIN_NT, 0, st>>>(p);
  }
  return hipGetLastError();
}

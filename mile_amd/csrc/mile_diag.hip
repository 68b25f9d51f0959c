// Chain-diagnostics kernels (mile_diag.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_device.h"
#include "mile_diag.h"
#include "mile_diag_device.h"

// ---- k_diag_transpose: block (32, 8), grid (ceil(P/32), ceil(S/32), C) ----------------------------------------------------
__global__ __launch_bounds__(256) void k_diag_transpose(DiagParams p) {
  __shared__ float tile[DIAG_TILE][DIAG_TILE + 1];
  const int tx = threadIdx.x, ty = threadIdx.y, c = blockIdx.z;
  const int s0 = blockIdx.y * DIAG_TILE, q0 = blockIdx.x * DIAG_TILE;
  for (int j = ty; j < DIAG_TILE; j += 8) {
    const int s = s0 + j, q = q0 + tx;
    if (s < p.S && q < p.P) tile[j][tx] = p.samples[((long long)c * p.S + s) * p.d + p.p0 + q];
  }
  __syncthreads();
  float *dst = (p.what & MILE_DIAG_POOLED_INPUT) ? p.z : p.raw;
  for (int j = ty; j < DIAG_TILE; j += 8) {
    const int q = q0 + j, s = s0 + tx;
    if (q < p.P && s < p.S) dst[((long long)q * p.C + c) * p.S + s] = tile[tx][j];
  }
}

// ---- k_diag_pool_rank: one workgroup per parameter ---------------------------------------------------------------------------
__global__ __launch_bounds__(DIAG_POOL_NT) void k_diag_pool_rank(DiagParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char diag_smem[];
  uint64_t *a = (uint64_t *)diag_smem;
  const int tid = threadIdx.x, n = p.C * p.S;
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  const float *src = p.raw + (long long)blockIdx.x * n;
  float *dst = p.z + (long long)blockIdx.x * n;
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
  if (__syncthreads_or(nan)) {      // a NaN draw has no rank: every score of the parameter is NaN (scipy's rankdata)
    for (int i = tid; i < n; i += DIAG_POOL_NT) dst[i] = __int_as_float(0x7fc00000);
    return;
  }
  bitonic(a, n2, tid, DIAG_POOL_NT);
  for (int i = tid; i < n; i += DIAG_POOL_NT) dst[(uint32_t)a[i]] = (float)diag_rank_score(a, n, i);
}

// ---- k_diag_chain: one workgroup of 256 per (parameter, chain) ------------------------------------------------------------------
// x[0, S) cut into n_splits pieces of len: the sum of the pieces' ddof-1 variances, the mean M of x, and the sum of squares
// of the piece means about M.  A wave per piece, two passes; waves and pieces are added in index order.
// (n_splits is small in practice -- the reference uses 2 and 4 -- so a wave per piece keeps the lanes busy; with very
// many short pieces most lanes of a wave idle, which costs time, not correctness.)
__device__ static void diag_split_moments(const float *x, int S, int n_splits, double *red, int tid, double &sumvar,
                                          double &M, double &ss) {
  double s = 0.0;
  for (int t = tid; t < S; t += DIAG_CHAIN_NT) s += (double)x[t];
  M = block_sum<4>(s, red) / (double)S;
  const int len = S / n_splits, lane = tid & 63, wave = tid >> 6;
  double av = 0.0, as = 0.0;
  for (int k = wave; k < n_splits; k += DIAG_CHAIN_NT / 64) {
    const float *xk = x + k * len;
    double s1 = 0.0;
    for (int t = lane; t < len; t += 64) s1 += (double)xk[t];
    const double mk = wave_sum(s1) / (double)len;
    double s2 = 0.0;
    for (int t = lane; t < len; t += 64) { const double e = (double)xk[t] - mk; s2 += e * e; }
    av += wave_sum(s2) / (double)(len - 1);
    as += (mk - M) * (mk - M);
  }
  if (lane == 0) { red[wave] = av; red[4 + wave] = as; }
  __syncthreads();
  sumvar = ((red[0] + red[1]) + red[2]) + red[3];
  ss = ((red[4] + red[5]) + red[6]) + red[7];
  __syncthreads();
}

__global__ __launch_bounds__(DIAG_CHAIN_NT) void k_diag_chain(DiagParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char diag_smem[];
  const int S = p.S, tid = threadIdx.x, q = blockIdx.x, c = blockIdx.y;
  int S2 = 1;
  while (S2 < S) S2 <<= 1;
  float *xf = (float *)diag_smem;
  unsigned char *regB = diag_smem + (S * 4 + 15) / 16 * 16;
  uint64_t *a = (uint64_t *)regB;                 // the sort ...
  double *xc = (double *)regB, *ac = xc + S2;     // ... and later the centred scores and their autocovariances
  double *red = (double *)(regB + (size_t)S2 * 16);   // [8] + [256] partial lag sums
  double *part = red + 8;
  const long long row = ((long long)q * p.C + c) * S;
  double *stat = p.stat + ((long long)q * p.C + c) * DIAG_NSTAT;
  const float qnan = __int_as_float(0x7fc00000);

  if (p.what & (MILE_DIAG_WCV | MILE_DIAG_BCV | MILE_DIAG_CRHAT)) {
    int nan = 0;
    for (int t = tid; t < S; t += DIAG_CHAIN_NT) { const float x = p.raw[row + t]; xf[t] = x; nan |= x != x; }
    nan = __syncthreads_or(nan);
    if (p.what & (MILE_DIAG_WCV | MILE_DIAG_BCV)) {
      double var, mean, ss;
      diag_split_moments(xf, S, 1, red, tid, var, mean, ss);
      if (tid == 0) { stat[0] = mean; stat[1] = var; }
    }
    if (p.what & MILE_DIAG_CRHAT) {
      float out = qnan;
      if (!nan) {                                   // (block-uniform)
        for (int i = tid; i < S2; i += DIAG_CHAIN_NT)
          a[i] = i < S ? (((uint64_t)diag_key(xf[i]) << 32) | (uint32_t)i) : ~0ull;
        __syncthreads();
        bitonic(a, S2, tid, DIAG_CHAIN_NT);
        for (int i = tid; i < S; i += DIAG_CHAIN_NT) xf[(uint32_t)a[i]] = (float)diag_rank_score(a, S, i);
        __syncthreads();
        double sumvar, M, ss;
        diag_split_moments(xf, S, p.n_splits, red, tid, sumvar, M, ss);
        const double len = (double)(S / p.n_splits), w = sumvar / (double)p.n_splits, b = ss / (double)(p.n_splits - 1);
        out = (float)sqrt(((len - 1.0) / len * w + b) / w);
      }
      if (tid == 0) p.crhat[(long long)c * p.d + p.p0 + q] = out;
    }
    __syncthreads();
  }
  if (!(p.what & (MILE_DIAG_ESS | MILE_DIAG_RHAT))) return;

  for (int t = tid; t < S; t += DIAG_CHAIN_NT) xf[t] = p.z[row + t];
  __syncthreads();
  double sumvar, M, ss;
  diag_split_moments(xf, S, p.n_splits, red, tid, sumvar, M, ss);
  if (tid == 0) { stat[2] = sumvar; stat[3] = M; stat[4] = ss; }
  if (!(p.what & MILE_DIAG_ESS)) return;

  // Single-chain ESS of mile_amd/diagnostics.py: biased autocovariance ac[k] = sum_t xc[t] xc[t+k] / S by direct summation,
  // 64 lags (32 Geyer pairs) at a time -- a wave per quarter of the t range, a lane per lag, so xc[t] is a broadcast and
  // xc[t+k] a conflict-free row -- and no further block once one holds a pair sum that is not positive.
  for (int t = tid; t < S; t += DIAG_CHAIN_NT) xc[t] = (double)xf[t] - M;
  __syncthreads();
  const int S_even = S & ~1, T = S_even >> 1, lag = tid & 63, seg = tid >> 6;
  const double fS = (double)S;
  int nlag = 0;
  for (int k0 = 0; k0 < S_even; k0 += 64) {
    const int k = k0 + lag;
    double s = 0.0;
    if (k < S_even)
      for (int t = seg; t < S - k; t += DIAG_CHAIN_NT / 64) s += xc[t] * xc[t + k];
    part[seg * 64 + lag] = s;
    __syncthreads();
    if (seg == 0 && k < S_even) ac[k] = (((part[lag] + part[64 + lag]) + part[128 + lag]) + part[192 + lag]) / fS;
    __syncthreads();
    nlag = min(k0 + 64, S_even);
    int stop = 0;
    const int t = (k0 >> 1) + lag;
    if (seg == 0 && lag < 32 && t < T) {
      const double a0 = ac[0], v0 = a0 * fS / (fS - 1.0);
      const double re = t == 0 ? 1.0 : 1.0 - (v0 - ac[2 * t]) / a0, ro = 1.0 - (v0 - ac[2 * t + 1]) / a0;
      stop = !(re + ro > 0.0);
    }
    if (__syncthreads_or(stop)) break;
  }
  // Lane 0 alone walks the pairs kept: a few for a typical chain, up to S/2 when no pair sum ever turns non-positive.
  if (tid == 0) {
    const double a0 = ac[0], v0 = a0 * fS / (fS - 1.0);
    auto rho = [&](int k) { return k == 0 ? 1.0 : 1.0 - (v0 - ac[k]) / a0; };
    const int Tc = nlag >> 1;                      // pairs computed
    int t_star = T;                                // first pair whose sum is not positive (T: none)
    for (int t = 0; t < Tc; ++t)
      if (!(rho(2 * t) + rho(2 * t + 1) > 0.0)) { t_star = t; break; }
    const int max_t = t_star > 0 ? t_star - 1 : 0;
    const int nxt = min(max_t + 1, T - 1);
    const bool in_range = max_t + 1 <= T - 1;
    // pairs past nxt are all zero and the running minimum is >= 0 by then: they add nothing
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
    const double floor_ = 1.0 / log10(fS);
    if (tau < floor_) tau = floor_;
    p.ess[(long long)c * p.d + p.p0 + q] = (float)(fS / tau);
  }
}

// ---- k_diag_final: one thread per parameter, chains in index order ---------------------------------------------------------
__global__ __launch_bounds__(64) void k_diag_final(DiagParams p) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= p.P) return;
  const double *st = p.stat + (long long)q * p.C * DIAG_NSTAT;
  const int C = p.C;
  if (p.what & (MILE_DIAG_WCV | MILE_DIAG_BCV)) {
    double sm = 0.0, sv = 0.0;
    for (int c = 0; c < C; ++c) { sm += st[c * DIAG_NSTAT]; sv += st[c * DIAG_NSTAT + 1]; }
    const double gm = sm / C;
    double sb = 0.0;
    for (int c = 0; c < C; ++c) { const double e = st[c * DIAG_NSTAT] - gm; sb += e * e; }
    if (p.what & MILE_DIAG_WCV) p.wcv[p.p0 + q] = (float)(sv / C);
    if (p.what & MILE_DIAG_BCV) p.bcv[p.p0 + q] = (float)(sb / (double)(C - 1));
  }
  if (p.what & MILE_DIAG_RHAT) {
    double sm = 0.0, sv = 0.0;
    for (int c = 0; c < C; ++c) { sv += st[c * DIAG_NSTAT + 2]; sm += st[c * DIAG_NSTAT + 3]; }
    const double gm = sm / C, ns = (double)p.n_splits, np_ = ns * C, len = (double)(p.S / p.n_splits);
    double sb = 0.0;
    for (int c = 0; c < C; ++c) { const double e = st[c * DIAG_NSTAT + 3] - gm; sb += st[c * DIAG_NSTAT + 4] + ns * e * e; }
    const double w = sv / np_, b = sb / (np_ - 1.0);
    p.rhat[p.p0 + q] = (float)sqrt(((len - 1.0) / len * w + b) / w);
  }
}

hipError_t mile_launch_diag_transpose(const DiagParams &p, hipStream_t st) {
  const dim3 tg((p.P + DIAG_TILE - 1) / DIAG_TILE, (p.S + DIAG_TILE - 1) / DIAG_TILE, p.C);
  k_diag_transpose<<<tg, dim3(DIAG_TILE, 8), 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_diag(const DiagParams &p, hipStream_t st) {
  const bool pooled_in = p.what & MILE_DIAG_POOLED_INPUT, need_z = p.what & (MILE_DIAG_ESS | MILE_DIAG_RHAT);
  const dim3 tg((p.P + DIAG_TILE - 1) / DIAG_TILE, (p.S + DIAG_TILE - 1) / DIAG_TILE, p.C);
  if (p.samples) k_diag_transpose<<<tg, dim3(DIAG_TILE, 8), 0, st>>>(p);   // null: the caller has filled the plane itself
  if (need_z && !pooled_in) {
    hipError_t e = mile_set_max_lds<k_diag_pool_rank>((int)diag_pool_lds(DIAG_POOL_MAX));
    if (e != hipSuccess) return e;
    k_diag_pool_rank<<<p.P, DIAG_POOL_NT, diag_pool_lds(p.C * p.S), st>>>(p);
  }
  hipError_t e = mile_set_max_lds<k_diag_chain>((int)diag_chain_lds(DIAG_S_MAX));
  if (e != hipSuccess) return e;
  k_diag_chain<<<dim3(p.P, p.C), DIAG_CHAIN_NT, diag_chain_lds(p.S), st>>>(p);
  if (p.what & (MILE_DIAG_WCV | MILE_DIAG_BCV | MILE_DIAG_RHAT)) k_diag_final<<<(p.P + 63) / 64, 64, 0, st>>>(p);
  return hipGetLastError();
}

// Calibration kernels (mile_calib.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_block.h"
#include "mile_calib.h"

__global__ __launch_bounds__(CAL_NT) void k_cal_accum(const CalParams p) {
  const int n = blockIdx.x * CAL_NT + threadIdx.x, c = blockIdx.y;
  if (n >= p.Nt) return;
  const int K = p.K;
  double *sum = p.sum + ((size_t)c * p.Nt + n) * K;
  int32_t *cnt = p.cnt + (size_t)c * p.Nt + n;
  const size_t stride = (size_t)p.ld * K;                                 // floats from one draw to the next
  const float *base = p.raw + (size_t)c * (size_t)p.cs * stride + (size_t)n * K;
  for (int k0 = 0; k0 < K; k0 += CAL_KC) {                                // (K <= 16: one trip, one exp per logit)
    double a[CAL_KC];
#pragma unroll
    for (int j = 0; j < CAL_KC; ++j) a[j] = k0 + j < K ? sum[k0 + j] : 0.0;
    int kc = 0;
    const float *x = base;
    for (int s = 0; s < p.J; ++s, x += stride) {
      float m = x[0];
      bool fin = finite_f32(m);
      for (int k = 1; k < K; ++k) { const float v = x[k]; fin = fin && finite_f32(v); m = fmaxf(m, v); }
      if (!fin) continue;
      const double md = (double)m;
      // sum of exp(x - m) over k = 0 .. K-1 in that order in every trip, the trip's own classes kept in registers
      double se = 0.0, e[CAL_KC];
      for (int k = 0; k < k0; ++k) se += exp((double)x[k] - md);
#pragma unroll
      for (int j = 0; j < CAL_KC; ++j) {
        e[j] = 0.0;
        if (k0 + j < K) { e[j] = exp((double)x[k0 + j] - md); se += e[j]; }
      }
      for (int k = k0 + CAL_KC; k < K; ++k) se += exp((double)x[k] - md);
      ++kc;
#pragma unroll
      for (int j = 0; j < CAL_KC; ++j)
        if (k0 + j < K) a[j] += e[j] / se;
    }
#pragma unroll
    for (int j = 0; j < CAL_KC; ++j)
      if (k0 + j < K) sum[k0 + j] = a[j];
    if (k0 == 0) *cnt += kc;
  }
}

__global__ __launch_bounds__(64 * CAL_ROWS_NW) void k_cal_rows(const CalParams p) {
  __shared__ double pc[CAL_ROWS_NW][CAL_K_MAX], ps[CAL_ROWS_NW][CAL_K_MAX], cv[CAL_Q_MAX];
  const int w = threadIdx.x >> 6, k = threadIdx.x & 63;
  const int K = p.K, C = p.C, Q = p.Q, Nt = p.Nt;
  const long long id = (long long)blockIdx.x * CAL_ROWS_NW + w;           // (group, tile row), the row fastest
  const bool act = id < (long long)(C + 1) * Nt;                           // uniform over the wave
  const int g = act ? (int)(id / Nt) : 0, n = act ? (int)(id % Nt) : 0;
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (threadIdx.x < Q) cv[threadIdx.x] = p.cov[threadIdx.x];

  long long kept = 0;
  double t = 0.0;
  if (act) {
    const int kk = k < K ? k : 0;
    if (g < C) {
      kept = p.cnt[(size_t)g * Nt + n];
      t = p.sum[((size_t)g * Nt + n) * K + kk];
    } else {
      for (int c = 0; c < C; ++c) {                                        // the chain sums in chain order
        kept += p.cnt[(size_t)c * Nt + n];
        t += p.sum[((size_t)c * Nt + n) * K + kk];
      }
    }
  }
  const double P = kept > 0 && k < K ? t / (double)kept : qnan;
  int pos = k;                                                             // nothing kept: the classes by index
  if (kept > 0) {
    pos = 0;
    for (int j = 0; j < K; ++j) {
      const double Pj = __shfl(P, j);
      pos += (Pj > P || (Pj == P && j < k)) ? 1 : 0;
    }
  }
  if (k < K) { pc[w][k] = P; ps[w][pos] = P; }
  __syncthreads();

  int sz = 0;
  if (kept > 0 && k < Q) {                                                 // lane q: the serial cumulative sum against coverage q
    const double lev = cv[k];
    double cum = 0.0;
    for (int i = 0; i < K; ++i) {
      cum += ps[w][i];
      if (sz == 0 && cum >= lev) sz = i + 1;
    }
    if (sz == 0) sz = K;
  }
  const int yv = p.y && act ? p.y[p.r0 + n] : -1;
  const bool bad = yv < 0 || yv >= K;
  const int rk = bad ? 0 : __shfl(pos, yv) + 1;
  const double Py = __shfl(P, bad ? 0 : yv);
  if (!act) return;

  const size_t row = (size_t)p.r0 + n;
  if (p.probs && k < K) p.probs[((size_t)g * p.N + row) * K + k] = P;
  if (p.kept && k == 0) p.kept[(size_t)g * p.N + row] = (int32_t)kept;
  if (g == C) {
    if (p.order && k < K) p.order[row * K + pos] = k;
    if (p.set_size && k < Q) p.set_size[row * Q + k] = sz;
    if (p.rank && k == 0) p.rank[row] = kept > 0 ? rk : 0;
  }
  if (p.rec) {
    CalRec *r = p.rec + (size_t)g * Nt + n;
    if (k < CAL_Q_MAX) r->size[k] = (uint8_t)sz;
    if (k == 0) {
      double b = 0.0;
      if (kept > 0 && !bad)
        for (int i = 0; i < K; ++i) { const double d = pc[w][i] - (i == yv ? 1.0 : 0.0); b += d * d; }
      r->brier = b;
      r->nll = kept > 0 && !bad ? -log(Py) : 0.0;
      r->conf = kept > 0 ? ps[w][0] : 0.0;
      r->rank = kept > 0 ? rk : -1;
      r->pad = 0;
    }
  }
}

// column `col` of the totals-and-bins row of one record: totals (rows counted, rows correct, brier, nll, bad labels,
// covered_q .., size_q ..), then bins (count, conf, correct) per bin
__device__ __forceinline__ double cal_column(const CalRec &r, int col, int Q, int n_bins) {
  if (r.rank < 0) return 0.0;
  if (r.rank == 0) return col == 4 ? 1.0 : 0.0;
  if (col < 5) return col == 0 ? 1.0 : col == 1 ? (r.rank == 1 ? 1.0 : 0.0) : col == 2 ? r.brier : col == 3 ? r.nll : 0.0;
  if (col < 5 + Q) return r.rank <= (int)r.size[col - 5] ? 1.0 : 0.0;
  if (col < 5 + 2 * Q) return (double)r.size[col - 5 - Q];
  const int j = col - 5 - 2 * Q, bin = min(n_bins - 1, (int)floor(r.conf * (double)n_bins));
  if (j / 3 != bin) return 0.0;
  return j % 3 == 0 ? 1.0 : j % 3 == 1 ? r.conf : (r.rank == 1 ? 1.0 : 0.0);
}

__global__ __launch_bounds__(256) void k_cal_part(const CalParams p) {
  const int W = cal_cols(p.Q, p.n_bins);
  const long long b0 = p.r0 / p.B, nb = (p.r0 + p.Nt - 1) / p.B - b0 + 1;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)(p.C + 1) * nb * W) return;
  const int col = (int)(t % W);
  const long long b = b0 + (t / W) % nb, g = t / ((long long)W * nb);
  const long long lo = max(b * p.B, p.r0), hi = min((b + 1) * p.B, p.r0 + p.Nt);
  double *dst = p.part + ((size_t)g * p.nblk + b) * W + col;
  double acc = *dst;
  const CalRec *r = p.rec + (size_t)g * p.Nt + (lo - p.r0);
  for (long long i = lo; i < hi; ++i, ++r) acc += cal_column(*r, col, p.Q, p.n_bins);   // the block's rows in row order
  *dst = acc;
}

__global__ __launch_bounds__(256) void k_cal_final(const CalParams p) {
  const int W = cal_cols(p.Q, p.n_bins), T = 5 + 2 * p.Q;
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)(p.C + 1) * W) return;
  const int col = (int)(t % W);
  const long long g = t / W;
  const double *src = p.part + (size_t)g * p.nblk * W + col;
  double acc = 0.0;
  for (long long b = 0; b < p.nblk; ++b) acc += src[(size_t)b * W];                       // the blocks in block order
  if (col < T) { if (p.totals) p.totals[g * T + col] = acc; }
  else if (p.bins) p.bins[g * (W - T) + (col - T)] = acc;
}

hipError_t mile_launch_cal_accum(const CalParams &p, hipStream_t st) {
  const dim3 grid((p.Nt + CAL_NT - 1) / CAL_NT, p.C);
  k_cal_accum<<<grid, CAL_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_cal_rows(const CalParams &p, hipStream_t st) {
  const long long waves = (long long)(p.C + 1) * p.Nt;
  k_cal_rows<<<(unsigned)((waves + CAL_ROWS_NW - 1) / CAL_ROWS_NW), 64 * CAL_ROWS_NW, 0, st>>>(p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !p.rec) return e;
  const long long nb = (p.r0 + p.Nt - 1) / p.B - p.r0 / p.B + 1, threads = (long long)(p.C + 1) * nb * cal_cols(p.Q, p.n_bins);
  k_cal_part<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_cal_final(const CalParams &p, hipStream_t st) {
  const long long threads = (long long)(p.C + 1) * cal_cols(p.Q, p.n_bins);
  k_cal_final<<<(unsigned)((threads + 255) / 256), 256, 0, st>>>(p);
  return hipGetLastError();
}

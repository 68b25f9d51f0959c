// CRPS kernels (mile_crps.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.  No fast-math:
// expf is the accurate one.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_block.h"
#include "mile_device.h"
#include "mile_crps.h"

// first chain block of chain c among the C (C + 1) / 2 blocks c <= c', in row-major order of the upper triangle
__device__ __forceinline__ int crps_block0(int c, int C) { return c * (2 * C - c + 1) / 2; }

__global__ __launch_bounds__(CRPS_NT) void k_crps_pack(const CrpsParams p) {
  __shared__ float2 tile[CRPS_TILE][CRPS_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, half = ty & 1;
  const int r0 = blockIdx.x * CRPS_TILE, c = blockIdx.y;
  const int S = p.S, Nt = p.Nt, C = p.C;
  const float2 *raw = (const float2 *)p.raw + (size_t)c * S * (size_t)p.ld;
  const float qnan = __int_as_float(0x7fc00000);
  int base[4] = {0, 0, 0, 0};     // kept draws so far of rows r0 + ty + 8 k (the same in the 32 lanes of a half-wave)
  for (int sb = 0; sb < S; sb += CRPS_TILE) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // row tx of draws ty, ty + 8, ...: a half-wave reads 32 consecutive rows of one draw
      const int j = ty + 8 * k, s = sb + j;
      float2 v = make_float2(qnan, qnan);
      if (s < S && r0 + tx < Nt) {
        const float2 r = raw[(size_t)s * (size_t)p.ld + r0 + tx];
        if (finite_f32(r.x) && finite_f32(r.y)) {
          const float sg = fminf(fmaxf(expf(r.y), 1e-6f), 1e6f);
          v = make_float2(r.x, sg * sg);
        }
      }
      tile[j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // draw sb + tx of rows ty, ty + 8, ...: a half-wave holds 32 consecutive draws of one row
      const int rr = r0 + ty + 8 * k;
      const float2 v = tile[tx][ty + 8 * k];
      const bool kept = v.x == v.x;     // (out-of-range draws and rows are NaN in the tile)
      const unsigned long long m = __ballot(kept);
      const unsigned mh = (unsigned)(m >> (32 * half));
      if (kept) p.pk[((size_t)rr * C + c) * S + base[k] + __popc(mh & ((1u << tx) - 1u))] = v;
      base[k] += __popc(mh);
    }
    __syncthreads();
  }
  if (tx == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rr = r0 + ty + 8 * k;
      if (rr < Nt) {
        p.cnt[(size_t)rr * C + c] = base[k];
        if (p.dropped) p.dropped[(size_t)c * p.N + p.r0 + rr] = (int32_t)(S - base[k]);
      }
    }
  }
}

// A(d, v) = E|N(d, v)| in fp32.  With s = sqrt(v) and t = |d| / s, A = |d| + s g(t), where
//   g(t) = sqrt(2 / pi) exp(-t^2 / 2) - t erfc(t / sqrt 2) = exp(-t^2 / 2) R(t),  R(t) = sqrt(2 / pi) - t erfcx(t / sqrt 2):
// one approximation of the even function h(t) = A / s = t + g(t) in place of erff and expf of their own.  R falls smoothly from
// sqrt(2 / pi) to 0 like 1 / t^2, and is a degree-8 polynomial in w = t / (4 + t) to 4e-10 of h (least squares on 6000 Chebyshev
// nodes of w, weighted by exp(-t^2 / 2)): w = 0 at t = 0, so the coefficients do not cancel where g matters, and where they do
// (w -> 1) exp(-t^2 / 2) has taken g below an ulp of |d|.  In fp32 with v_rsq_f32, v_rcp_f32 (1 ulp each) and the accurate expf: 3e-7 of A at the most
// over |d| / s from 0 to 1e14 (4e6 random arguments, emulated on the host), 1.5e-8 on average.  t is capped at 64 (exp(-2048) = 0)
// so that an overflowing d * rs leaves A = |d|.
__device__ __forceinline__ float crps_A(float d, float v) {
  const float rs = __builtin_amdgcn_rsqf(v), s = v * rs, ad = fabsf(d), t = fminf(ad * rs, 64.0f);   // v in [2e-12, 2e12]: normal
  const float q = 0.25f * t, w = q * __builtin_amdgcn_rcpf(1.0f + q);
  float p = 1.616507649e-01f;
  p = fmaf(p, w, 5.051566395e-01f);
  p = fmaf(p, w, -1.546404125e+00f);
  p = fmaf(p, w, -5.637862036e-01f);
  p = fmaf(p, w, 6.380986862e+00f);
  p = fmaf(p, w, -1.046742736e+01f);
  p = fmaf(p, w, 8.766143297e+00f);
  p = fmaf(p, w, -3.999999866e+00f);
  p = fmaf(p, w, 7.978845605e-01f);
  return fmaf(s, p * expf(-0.5f * t * t), ad);
}
__device__ __forceinline__ double crps_A64(double d, double v) {
  const double s = sqrt(v), t = d / s;
  return d * erf(t * 0.70710678118654752440) + s * 0.79788456080286535588 * exp(-0.5 * t * t);
}

// the nj draws of one j-tile against this thread's NR i-draws i_first + 256 r: acc[r] += w * (runs of <= CRPS_RUN terms).
// DIAG (a j-tile that overlaps the i-tile of a block c = c'): a pair j > i counts twice, j = i once, j < i not.
template <int NR, bool DIAG>
__device__ __forceinline__ void crps_tile_terms(const float2 *tj, int nj, const float *mu, const float *var, int i_first, int j0,
                                                double w, double *acc) {
  for (int jb = 0; jb < nj; jb += CRPS_RUN) {
    const int je = min(CRPS_RUN, nj - jb);
    float run[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) run[r] = 0.0f;
#pragma unroll 4
    for (int jj = 0; jj < je; ++jj) {
      const float2 q = tj[jb + jj];     // one broadcast read for NR pair terms
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        float a = crps_A(mu[r] - q.x, var[r] + q.y);
        if constexpr (DIAG) {
          const int jg = j0 + jb + jj, ig = i_first + CRPS_NT * r;
          a = jg > ig ? 2.0f * a : (jg == ig ? a : 0.0f);
        }
        run[r] += a;
      }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] += w * (double)run[r];
  }
}

template <bool DIAG>
__device__ __forceinline__ void crps_tile_nr(int nr, const float2 *tj, int nj, const float *mu, const float *var, int i_first, int j0,
                                             double w, double *acc) {
  switch (nr) {     // (the same in every lane of a wave)
    case 1: crps_tile_terms<1, DIAG>(tj, nj, mu, var, i_first, j0, w, acc); break;
    case 2: crps_tile_terms<2, DIAG>(tj, nj, mu, var, i_first, j0, w, acc); break;
    case 3: crps_tile_terms<3, DIAG>(tj, nj, mu, var, i_first, j0, w, acc); break;
    case 4: crps_tile_terms<4, DIAG>(tj, nj, mu, var, i_first, j0, w, acc); break;
    default: break;
  }
}

__global__ __launch_bounds__(CRPS_NT) void k_crps_pairs(const CrpsParams p) {
  __shared__ float2 tj[CRPS_TJ];
  __shared__ double red[CRPS_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int C = p.C, S = p.S;
  const unsigned units = (unsigned)p.pl.units;
  const unsigned n = blockIdx.x / units, u = blockIdx.x - n * units;
  const int b = (int)(u / (unsigned)p.pl.upb), ub = (int)(u - (unsigned)b * (unsigned)p.pl.upb);
  const int ti = ub / p.pl.n_js, js = ub - ti * p.pl.n_js;
  // b -> (c, c2), c <= c2: the root of crps_block0(c) = b in fp32, then exact
  int c = (int)(0.5f * ((float)(2 * C + 1) - sqrtf((float)((2 * C + 1) * (2 * C + 1) - 8 * b))));
  c = min(max(c, 0), C - 1);
  while (c + 1 < C && crps_block0(c + 1, C) <= b) ++c;
  while (c > 0 && crps_block0(c, C) > b) --c;
  const int c2 = c + (b - crps_block0(c, C));
  const bool same = c == c2;
  const int Ki = p.cnt[(size_t)n * C + c], Kj = p.cnt[(size_t)n * C + c2];
  const float2 *gi = p.pk + ((size_t)n * C + c) * S, *gj = p.pk + ((size_t)n * C + c2) * S;
  const int i0 = ti * CRPS_TI, i_first = i0 + tid;
  // i-draws of this wave: rows r of 256 with a draw below Ki in the wave (a prefix of 0 .. CRPS_R - 1)
  const int left = Ki - i0 - wv * 64;
  const int nr = left <= 0 ? 0 : min(CRPS_R, (left + CRPS_NT - 1) / CRPS_NT);
  float mu[CRPS_R], var[CRPS_R];
  double acc[CRPS_R];
#pragma unroll
  for (int r = 0; r < CRPS_R; ++r) {
    const int i = i_first + CRPS_NT * r;
    const float2 v = i < Ki ? gi[i] : make_float2(0.0f, 1.0f);
    mu[r] = v.x; var[r] = v.y; acc[r] = 0.0;
  }
  // the j-tiles of this i-tile (a block c = c' starts at the i-tile's own), an even share of them for split js
  const int t_first = same ? ti * (CRPS_TI / CRPS_TJ) : 0, t_cnt = max(p.pl.n_jt - t_first, 0);
  const int t_lo = t_first + (int)(((long long)js * t_cnt) / p.pl.n_js), t_hi = t_first + (int)(((long long)(js + 1) * t_cnt) / p.pl.n_js);
  for (int t = t_lo; t < t_hi; ++t) {
    const int j0 = t * CRPS_TJ;
    if (j0 >= Kj) break;     // (the same in every thread)
    __syncthreads();
    tj[tid] = j0 + tid < Kj ? gj[j0 + tid] : make_float2(0.0f, 1.0f);
    __syncthreads();
    const int nj = min(CRPS_TJ, Kj - j0);
    if (same && j0 < i0 + CRPS_TI) crps_tile_nr<true>(nr, tj, nj, mu, var, i_first, j0, 1.0, acc);
    else crps_tile_nr<false>(nr, tj, nj, mu, var, i_first, j0, same ? 2.0 : 1.0, acc);
  }
  double tot = 0.0;
#pragma unroll
  for (int r = 0; r < CRPS_R; ++r)
    if (i_first + CRPS_NT * r < Ki) tot += acc[r];     // (a lane past Ki computed on a stand-in draw)
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) tot += __shfl_xor(tot, o);
  if (lane == 0) red[wv] = tot;
  __syncthreads();
  if (tid == 0) p.part[(size_t)n * units + u] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(CRPS_NT) void k_crps_finish(const CrpsParams p) {
  __shared__ double a_s[CRPS_MAX_C], w_s[CRPS_MAX_C];
  __shared__ int K_s[CRPS_MAX_C];
  __shared__ double red[CRPS_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = blockIdx.x, C = p.C, S = p.S, upb = p.pl.upb;
  const size_t row = (size_t)(p.r0 + n);
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  for (int c = tid; c < C; c += CRPS_NT) K_s[c] = p.cnt[(size_t)n * C + c];
  __syncthreads();
  // a_c: a wave per chain, lanes over its kept draws, fp64
  const double yv = (double)p.y[n];
  for (int c = wv; c < C; c += CRPS_NT / 64) {
    const float2 *g = p.pk + ((size_t)n * C + c) * S;
    const int K = K_s[c];
    double sum = 0.0;
    for (int i = lane; i < K; i += 64) { const float2 v = g[i]; sum += crps_A64(yv - (double)v.x, (double)v.y); }
    sum = wave_sum(sum);
    if (lane == 0) a_s[c] = sum / (double)K;     // NaN for an empty chain
  }
  __syncthreads();
  // G_cc' from its slots in slot order, over the block's first slot; the chains' own outputs; gram, both triangles
  double *part = p.part + (size_t)n * (size_t)p.pl.units;
  for (int c = 0; c < C; ++c) {
    double *blk = part + (size_t)crps_block0(c, C) * upb;
    const double Kc = (double)K_s[c];
    for (int c2 = c + tid; c2 < C; c2 += CRPS_NT) {
      double *sl = blk + (size_t)(c2 - c) * upb;
      double sum = 0.0;
      for (int k = 0; k < upb; ++k) sum += sl[k];
      const double g = sum / (Kc * (double)K_s[c2]);
      sl[0] = g;
      if (p.gram) {
        p.gram[(row * C + c) * C + c2] = g;
        p.gram[(row * C + c2) * C + c] = g;
      }
      if (c2 == c) {
        if (p.crps_chain) p.crps_chain[(size_t)c * p.N + row] = a_s[c] - 0.5 * g;
        if (p.spread_chain) p.spread_chain[(size_t)c * p.N + row] = 0.5 * g;
      }
    }
  }
  if (!p.crps_mix && !p.spread_mix) return;
  long long Ktot = 0;
  for (int c = 0; c < C; ++c) Ktot += K_s[c];
  for (int m = 0; m <= p.n_w; ++m) {     // m = 0: the pooled ensemble, w_c = K_c / sum K
    __syncthreads();     // G is written, w_s is free
    for (int c = tid; c < C; c += CRPS_NT)
      w_s[c] = m == 0 ? (Ktot > 0 ? (double)K_s[c] / (double)Ktot : 0.0) : p.w[(size_t)(m - 1) * C + c];
    __syncthreads();
    double t1 = 0.0, t2 = 0.0;
    for (int c = tid; c < C; c += CRPS_NT)
      if (w_s[c] != 0.0) t1 += w_s[c] * a_s[c];
    for (int c = 0; c < C; ++c) {
      const double wc = w_s[c];
      if (wc == 0.0) continue;     // a chain of weight 0 is not read: an empty one spoils only mixtures that use it
      const double *blk = part + (size_t)crps_block0(c, C) * upb;
      for (int c2 = c + tid; c2 < C; c2 += CRPS_NT) {
        const double w2 = w_s[c2];
        if (w2 != 0.0) t2 += (c2 == c ? 1.0 : 2.0) * wc * w2 * blk[(size_t)(c2 - c) * upb];
      }
    }
    t1 = block_sum<CRPS_NT / 64>(t1, red);
    t2 = block_sum<CRPS_NT / 64>(t2, red);
    if (tid == 0) {
      const bool none = m == 0 && Ktot == 0;
      if (p.crps_mix) p.crps_mix[(size_t)m * p.N + row] = none ? qnan : t1 - 0.5 * t2;
      if (p.spread_mix) p.spread_mix[(size_t)m * p.N + row] = none ? qnan : 0.5 * t2;
    }
  }
}

hipError_t mile_launch_crps_pack(const CrpsParams &p, hipStream_t st) {
  k_crps_pack<<<dim3((p.Nt + CRPS_TILE - 1) / CRPS_TILE, p.C), CRPS_NT, 0, st>>>(p);
  return hipGetLastError();
}
hipError_t mile_launch_crps_pairs(const CrpsParams &p, hipStream_t st) {
  k_crps_pairs<<<(unsigned)((long long)p.Nt * p.pl.units), CRPS_NT, 0, st>>>(p);
  return hipGetLastError();
}
hipError_t mile_launch_crps_finish(const CrpsParams &p, hipStream_t st) {
  k_crps_finish<<<p.Nt, CRPS_NT, 0, st>>>(p);
  return hipGetLastError();
}

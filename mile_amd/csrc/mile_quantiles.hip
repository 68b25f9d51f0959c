// Mixture-quantile kernels (mile_quantiles.h) in a translation unit of their own: they compile concurrently with
// mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "mile_block.h"
#include "mile_device.h"
#include "mile_quantiles.h"

__device__ __forceinline__ double qnt_sigma(float log_sigma) { return fmin(fmax(exp((double)log_sigma), 1e-6), 1e6); }
// 1 / sigma: the clip of the reciprocal is the reciprocal of the clip, and an exp costs about what the division would
__device__ __forceinline__ double qnt_rsigma(float log_sigma) { return fmin(fmax(exp(-(double)log_sigma), 1e-6), 1e6); }
__device__ __forceinline__ double qnt_Phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

__global__ __launch_bounds__(256) void k_qnt_pack(const QntParams p) {
  __shared__ float2 tile[QNT_TILE][QNT_TILE + 1];
  __shared__ double red[4][QNT_TILE][2];
  __shared__ int redc[4][QNT_TILE];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5, wv = tid >> 6, lane = tid & 63;
  const int r0 = blockIdx.x * QNT_TILE, sl = blockIdx.y, row = r0 + tx;
  const int S = p.S, Nt = p.Nt, Q = p.Q;
  const int s_tiles = (S + QNT_TILE - 1) / QNT_TILE;
  const int t0 = (int)(((long long)sl * s_tiles) / p.slices), t1 = (int)(((long long)(sl + 1) * s_tiles) / p.slices);
  const float2 *raw = (const float2 *)p.raw;
  const float qnan = __int_as_float(0x7fc00000);
  double lo[QNT_MAX_Q], hi[QNT_MAX_Q];
#pragma unroll
  for (int q = 0; q < QNT_MAX_Q; ++q) { lo[q] = INFINITY; hi[q] = -INFINITY; }
  int cnt = 0;
  for (int t = t0; t < t1; ++t) {
    const int sb = t * QNT_TILE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // row tx of draws ty, ty + 8, ...: a half-wave reads 32 consecutive rows of one draw
      const int j = ty + 8 * k, s = sb + j;
      float2 v = make_float2(qnan, qnan);
      if (s < S && row < Nt) {
        const float2 r = raw[(size_t)s * (size_t)p.ld + row];
        if (finite_f32(r.x) && finite_f32(r.y)) {
          v = r;
          ++cnt;
          const double mu = (double)r.x, sig = qnt_sigma(r.y);
#pragma unroll
          for (int q = 0; q < QNT_MAX_Q; ++q)
            if (q < Q) {
              const double b = fma(p.lev[Q + q], sig, mu);
              lo[q] = fmin(lo[q], b);
              hi[q] = fmax(hi[q], b);
            }
        }
      }
      tile[j][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {     // draw sb + tx of rows ty, ty + 8, ...: a half-wave writes 32 consecutive pairs of one row
      const int rr = ty + 8 * k, s = sb + tx;
      if (s < S && r0 + rr < Nt) p.pk[(size_t)(r0 + rr) * S + s] = tile[tx][rr];
    }
    __syncthreads();
  }
  // the eight partial results of a row: lanes l and l + 32 of a wave by shuffle, the four waves through LDS in wave order
  cnt += __shfl_xor(cnt, 32);
  if (lane < 32) redc[wv][tx] = cnt;
  __syncthreads();
  if (tid < 32 && row < Nt) p.part_cnt[(size_t)sl * Nt + row] = redc[0][tx] + redc[1][tx] + redc[2][tx] + redc[3][tx];
#pragma unroll
  for (int q = 0; q < QNT_MAX_Q; ++q) {
    if (q < Q) {
      const double a = fmin(lo[q], __shfl_xor(lo[q], 32)), b = fmax(hi[q], __shfl_xor(hi[q], 32));
      __syncthreads();
      if (lane < 32) { red[wv][tx][0] = a; red[wv][tx][1] = b; }
      __syncthreads();
      if (tid < 32 && row < Nt) {
        double *o = p.part_brk + (((size_t)sl * Nt + row) * Q + q) * 2;
        o[0] = fmin(fmin(red[0][tx][0], red[1][tx][0]), fmin(red[2][tx][0], red[3][tx][0]));
        o[1] = fmax(fmax(red[0][tx][1], red[1][tx][1]), fmax(red[2][tx][1], red[3][tx][1]));
      }
    }
  }
}

// omega of component i's chain, for a walk of increasing i: the division only where the walk enters another chain
struct QntChainWalk {
  int c = 0, end = 0;
  __device__ __forceinline__ double at(int i, int Sc, const double *om) {
    if (i >= end) { c = i / Sc; end = (c + 1) * Sc; }
    return om[c];
  }
};

// P = QntParams: the equal-weight mixture; P = QntWParams: the chain-weighted one (W below)
template <bool LDS, class P = QntParams>
__global__ __launch_bounds__(QNT_NT) void k_qnt_solve(const P p) {
  constexpr bool W = std::is_same<P, QntWParams>::value;
  extern __shared__ float2 qnt_comp[];
  __shared__ double red[QNT_NW][QNT_MAX_Q][2];
  __shared__ double redb[QNT_NW];
  __shared__ double res[QNT_MAX_Q];
  __shared__ double om[W ? QNT_MAX_C : 1];     // omega_c = w_c / K_c
  __shared__ int kc[W ? QNT_MAX_C : 1];        // K_c
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int S = p.S, Nt = p.Nt, Q = p.Q;
  const float2 *g = p.pk + (size_t)n * S;
  const float qnan = __int_as_float(0x7fc00000);

  int kept = 0;
  if constexpr (!W) {
    for (int sl = 0; sl < p.slices; ++sl) kept += p.part_cnt[(size_t)sl * Nt + n];
    if (tid == 0 && p.dropped) p.dropped[n] = (int32_t)(S - kept);
    if (kept == 0) {     // (the same in every thread)
      if (p.quant && tid < Q) p.quant[(size_t)n * Q + tid] = qnan;
      if (p.pit && tid == 0) p.pit[n] = qnan;
      if (p.sweeps && tid == 0) p.sweeps[n] = 0;
      return;
    }
  }
  if constexpr (LDS) {
    for (int i = tid; i < S; i += QNT_NT) qnt_comp[i] = g[i];
    __syncthreads();
  }
  auto comp = [&](int i) -> float2 {
    if constexpr (LDS) return qnt_comp[i];
    else return g[i];
  };
  int Sc = 1;
  if constexpr (W) {
    Sc = p.Sc;
    const int C = p.C;
    for (int c = tid; c < C; c += QNT_NT) kc[c] = 0;
    __syncthreads();
    // K_c: 64 consecutive components per wave step; a step inside one chain adds its ballot's count once
    for (int b = wv * 64; b < S; b += QNT_NT) {
      const int i = b + lane;
      bool k = false;
      if (lane <= S - 1 - b) { const float mu = comp(i).x; k = mu == mu; }
      const int c0 = b / Sc, c1 = (S - 1 - b < 63 ? S - 1 : b + 63) / Sc;
      if (c0 == c1) {
        const int cnt = __popcll(__ballot(k));
        if (lane == 0 && cnt) atomicAdd(&kc[c0], cnt);
      } else if (k) {
        atomicAdd(&kc[i / Sc], 1);
      }
    }
    __syncthreads();
    int bad = 0;
    for (int c = tid; c < C; c += QNT_NT) {
      const double wc = p.w[c];
      const int K = kc[c];
      if (p.dropped_c) p.dropped_c[(size_t)c * (size_t)p.N + n] = (int32_t)(Sc - K);
      if (wc > 0.0 && K == 0) bad = 1;
      om[c] = wc > 0.0 && K > 0 ? wc / (double)K : 0.0;
    }
    if (__syncthreads_or(bad)) {     // a weighted chain with nothing kept (the same in every thread)
      if (p.quant && tid < Q) p.quant[(size_t)n * Q + tid] = qnan;
      if (p.pit && tid == 0) p.pit[n] = qnan;
      if (p.sweeps && tid == 0) p.sweeps[n] = 0;
      return;
    }
  }
  const double fk = (double)kept;
  int sweeps = 0;

  if (p.quant) {
    // sd_n of the mixture, two passes: the stopping width's scale and, with the mean, the first iterate
    double sm = 0.0, sv = 0.0;
    if constexpr (W) {
      QntChainWalk cw;
      for (int i = tid; i < S; i += QNT_NT) {
        const float2 v = comp(i);
        const double o = cw.at(i, Sc, om);
        if (o > 0.0 && v.x == v.x) { const double sg = qnt_sigma(v.y); sm = fma(o, (double)v.x, sm); sv = fma(o, sg * sg, sv); }
      }
    } else {
      for (int i = tid; i < S; i += QNT_NT) {
        const float2 v = comp(i);
        if (v.x == v.x) { const double sg = qnt_sigma(v.y); sm += (double)v.x; sv += sg * sg; }
      }
    }
    sm = block_sum<QNT_NW>(sm, redb);
    sv = block_sum<QNT_NW>(sv, redb);
    const double mean = W ? sm : sm / fk;
    double sd2 = 0.0;
    if constexpr (W) {
      QntChainWalk cw;
      for (int i = tid; i < S; i += QNT_NT) {
        const float2 v = comp(i);
        const double o = cw.at(i, Sc, om);
        if (o > 0.0 && v.x == v.x) { const double d = (double)v.x - mean; sd2 = fma(o, d * d, sd2); }
      }
    } else {
      for (int i = tid; i < S; i += QNT_NT) {
        const float2 v = comp(i);
        if (v.x == v.x) { const double d = (double)v.x - mean; sd2 += d * d; }
      }
    }
    sd2 = block_sum<QNT_NW>(sd2, redb);
    const double sd = W ? sqrt(sd2 + sv) : sqrt((sd2 + sv) / fk);

    const int nc = 64 / Q, q = lane % Q, cl = lane / Q;     // components a wave takes at a time; this lane's level and slot
    const bool act = lane < nc * Q;
    const double plev = p.lev[q];
    double lo = INFINITY, hi = -INFINITY;
    if constexpr (W) {     // the bracket over the components that carry weight, in the sweep's layout
      if (act) {
        const double zp = p.lev[Q + q];
        QntChainWalk cw;
        for (int i = wv * nc + cl; i < S; i += QNT_NW * nc) {
          const float2 v = comp(i);
          if (cw.at(i, Sc, om) > 0.0 && v.x == v.x) {
            const double b = fma(zp, qnt_sigma(v.y), (double)v.x);
            lo = fmin(lo, b);
            hi = fmax(hi, b);
          }
        }
      }
      double a = INFINITY, b = -INFINITY;
      for (int c = 0; c < nc; ++c) {
        a = fmin(a, __shfl(lo, q + Q * c));
        b = fmax(b, __shfl(hi, q + Q * c));
      }
      if (lane < Q) { red[wv][lane][0] = a; red[wv][lane][1] = b; }
      __syncthreads();
      lo = INFINITY; hi = -INFINITY;
#pragma unroll
      for (int w = 0; w < QNT_NW; ++w) { lo = fmin(lo, red[w][q][0]); hi = fmax(hi, red[w][q][1]); }
      __syncthreads();
    } else {
      for (int sl = 0; sl < p.slices; ++sl) {
        const double *b = p.part_brk + (((size_t)sl * Nt + n) * Q + q) * 2;
        lo = fmin(lo, b[0]);
        hi = fmax(hi, b[1]);
      }
    }
    auto width = [&]() { return 0x1p-25 * fmax(fabs(0.5 * (lo + hi)), sd); };
    double t = fma(p.lev[Q + q], sd, mean);
    if (!(t > lo && t < hi)) t = lo + 0.5 * (hi - lo);
    double dxold = hi - lo;
    bool done = !(hi - lo > width());
    while (sweeps < QNT_MAX_SWEEPS && !__all(done)) {     // every wave holds every level: the same decision in all four
      ++sweeps;
      double F = 0.0, f = 0.0;
      if (act && !done) {
        if constexpr (W) {
          QntChainWalk cw;
          for (int i = wv * nc + cl; i < S; i += QNT_NW * nc) {
            const float2 v = comp(i);
            const double o = cw.at(i, Sc, om);
            if (o > 0.0 && v.x == v.x) {
              const double rs = qnt_rsigma(v.y), z = (t - (double)v.x) * rs;
              F = fma(o, qnt_Phi(z), F);
              f = fma(o, exp(-0.5 * z * z) * rs, f);
            }
          }
        } else {
          for (int i = wv * nc + cl; i < S; i += QNT_NW * nc) {
            const float2 v = comp(i);
            if (v.x == v.x) {
              const double rs = qnt_rsigma(v.y), z = (t - (double)v.x) * rs;
              F += qnt_Phi(z);
              f += exp(-0.5 * z * z) * rs;
            }
          }
        }
      }
      double Fw = 0.0, fw = 0.0;
      for (int c = 0; c < nc; ++c) {     // this level's lanes of the wave, in component order
        Fw += __shfl(F, q + Q * c);
        fw += __shfl(f, q + Q * c);
      }
      if (lane < Q) { red[wv][lane][0] = Fw; red[wv][lane][1] = fw; }
      __syncthreads();
      double Ft = 0.0, ft = 0.0;
#pragma unroll
      for (int w = 0; w < QNT_NW; ++w) { Ft += red[w][q][0]; ft += red[w][q][1]; }
      __syncthreads();
      if (!done) {
        const double e = W ? Ft - plev : Ft / fk - plev;
        ft *= W ? 0.39894228040143267794 : 0.39894228040143267794 / fk;
        if (e < 0.0) lo = t; else hi = t;
        if (e == 0.0) lo = t;     // a root, to the last bit (a flat stretch of F at k / S): the bracket closes on it
        const double wd = hi - lo, tl = width();
        if (!(wd > tl)) {
          done = true;
        } else {
          const double dx = e / ft;
          const double tn = (t - dx) + (e < 0.0 ? 0.25 : -0.25) * tl;     // past the Newton target, towards the far end
          if (ft > 0.0 && tn > lo && tn < hi && fabs(dx) <= 0.5 * dxold) { dxold = fabs(dx); t = tn; }
          else { dxold = 0.5 * wd; t = lo + 0.5 * wd; }
        }
      }
    }
    // non-decreasing in the level whatever the last bits of neighbouring roots say: a running maximum
    if (wv == 0 && lane < Q) res[lane] = lo + 0.5 * (hi - lo);
    __syncthreads();
    if (tid < Q) {
      double m = res[0];
      for (int k = 1; k <= tid; ++k) m = fmax(m, res[k]);
      p.quant[(size_t)n * Q + tid] = (float)m;
    }
  }
  if (p.pit) {
    const double yv = (double)p.y[n];
    double F = 0.0;
    if constexpr (W) {
      QntChainWalk cw;
      for (int i = tid; i < S; i += QNT_NT) {
        const float2 v = comp(i);
        const double o = cw.at(i, Sc, om);
        if (o > 0.0 && v.x == v.x) F = fma(o, qnt_Phi((yv - (double)v.x) * qnt_rsigma(v.y)), F);
      }
    } else {
      for (int i = tid; i < S; i += QNT_NT) {
        const float2 v = comp(i);
        if (v.x == v.x) F += qnt_Phi((yv - (double)v.x) * qnt_rsigma(v.y));
      }
    }
    F = block_sum<QNT_NW>(F, redb);
    if (tid == 0) p.pit[n] = (float)(W ? F : F / fk);
  }
  if (p.sweeps && tid == 0) p.sweeps[n] = sweeps;
}

hipError_t mile_launch_quantiles(const QntParams &p, hipStream_t st) {
  k_qnt_pack<<<dim3((p.Nt + QNT_TILE - 1) / QNT_TILE, p.slices), 256, 0, st>>>(p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (p.S <= QNT_LDS_MAX_S) {
    e = mile_set_max_lds<k_qnt_solve<true>>(QNT_LDS_MAX_S * 8);
    if (e != hipSuccess) return e;
    k_qnt_solve<true><<<p.Nt, QNT_NT, (size_t)p.S * 8, st>>>(p);
  } else {
    k_qnt_solve<false><<<p.Nt, QNT_NT, 0, st>>>(p);
  }
  return hipGetLastError();
}

hipError_t mile_launch_quantiles_weighted(const QntWParams &p, hipStream_t st) {
  QntParams pack = p;     // the transpose alone: with no level k_qnt_pack forms no bracket, and its counts are not read
  pack.Q = 0;
  k_qnt_pack<<<dim3((p.Nt + QNT_TILE - 1) / QNT_TILE, p.slices), 256, 0, st>>>(pack);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (p.S <= QNT_LDS_MAX_S) {
    e = mile_set_max_lds<k_qnt_solve<true, QntWParams>>(QNT_LDS_MAX_S * 8);
    if (e != hipSuccess) return e;
    k_qnt_solve<true, QntWParams><<<p.Nt, QNT_NT, (size_t)p.S * 8, st>>>(p);
  } else {
    k_qnt_solve<false, QntWParams><<<p.Nt, QNT_NT, 0, st>>>(p);
  }
  return hipGetLastError();
}

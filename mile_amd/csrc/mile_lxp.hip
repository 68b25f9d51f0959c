// PSIS-LOO expectation kernels (mile_lxp.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_device.h"
#include "mile_loo_device.h"
#include "mile_lxp.h"
#include "mile_row_head.h"

// k_loo_pack's transpose; HEAD: the value is row_loglik of the forward's raw outputs of the (draw, row)
template <bool HEAD>
__global__ __launch_bounds__(256) void k_lxp_pack(const LxpParams p) {
  loo_pack_tile(p.pk, p.S, p.Nt, p.slices, [&](int s, int row) -> float {
    if constexpr (HEAD) return row_loglik(p.raw + ((size_t)s * (size_t)p.ld + row) * p.O, p.O, p.task, p.y, row);
    else return p.ll[(size_t)s * (size_t)p.ld + row];
  });
}

template <bool LDS>
__global__ __launch_bounds__(LOO_NT) void k_lxp_row(const LxpParams p) {
  extern __shared__ float lxp_row[];                  // <true>: the row's S values
  __shared__ uint32_t tkey[LOO_MAX_TAIL];             // the tail's keys, ascending in l after the sort
  __shared__ double tx[LOO_MAX_TAIL];                 // x_i, then lw_i, then w_i, ascending in r (tx[i] belongs to tkey[M - 1 - i])
  __shared__ uint32_t hist[256];
  __shared__ uint32_t sel[4];
  __shared__ uint32_t tail_cnt;
  __shared__ double cb[LOO_MAX_CAND], cL[LOO_MAX_CAND], cw[LOO_MAX_CAND];
  __shared__ double red[LOO_NW];
  __shared__ LooStat wst[LOO_NW];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int S = p.S;
  const float *g = p.pk + (size_t)n * S;
  double *wout = p.w ? p.w + (size_t)n * S : nullptr;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  auto val = [&](int i) -> float {
    if constexpr (LDS) return lxp_row[i];
    else return g[i];
  };
  auto nan_row = [&]() {     // a row without weights: NaN in every fp64 output
    if (tid == 0) {
      if (p.ess_w) p.ess_w[n] = qnan;
      if (p.khat) p.khat[n] = qnan;
      if (p.elpd_loo) p.elpd_loo[n] = qnan;
    }
    if (wout)
      for (int i = tid; i < S; i += LOO_NT) wout[i] = qnan;
  };

  // 1. to 6. as k_loo_row
  const LooStat st = loo_row_stats<LDS>(g, lxp_row, S, wst);
  const int kept = st.n;     // (the same in every thread from here on)
  if (tid == 0 && p.dropped) p.dropped[n] = (int32_t)(S - kept);
  if (kept < 2) { nan_row(); return; }
  const int M = loo_row_tail_length(kept, S, p.M_full, p.r_eff);
  if (M < 1 || M > LOO_MAX_TAIL || M + 1 > kept) { nan_row(); return; }     // cannot happen: the host checks M(S)
  const double lmin = st.lo, mx = -lmin;     // r = -l - max(-l)
  const LooCut c = loo_row_select(val, S, M, hist, sel);
  loo_row_sort_tail(val, S, M, c, tkey, &tail_cnt);
  const double r_T = -(double)f32_unkey(c.T) - mx;
  const double cut = fmax(r_T, LOO_LOG_DBL_MIN), ec = exp(cut);
  const LooFit f = loo_row_fit(M, tkey, tx, mx, ec, cb, cL, cw, red);
  if (tid == 0 && p.khat) p.khat[n] = f.khat;
  double mlw = r_T, ma = lmin, s1, s2;
  loo_row_smooth(M, tkey, tx, f, mx, ec, mlw, ma, red);
  loo_row_sums(val, S, M, c, tkey, tx, mx, r_T, mlw, ma, s1, s2, red);
  const double logZ = mlw + log(s1);
  if (tid == 0 && p.elpd_loo) p.elpd_loo[n] = (ma + log(s2)) - logZ;
  if (!wout && !p.ess_w) return;

  // a. the tail's normalised weights in place of lw
  for (int i = tid; i < M; i += LOO_NT) tx[i] = exp(tx[i] - logZ);
  __syncthreads();
  // b. the mean over every run of equal keys below T, left in the slot of the run's head (the lowest index in tkey)
  for (int j = tid; j < c.n_low; j += LOO_NT) {
    const uint32_t k = tkey[j];
    if ((j == 0 || tkey[j - 1] != k) && j + 1 < c.n_low && tkey[j + 1] == k) {
      double sum = tx[M - 1 - j];
      int e = j + 1;
      for (; e < c.n_low && tkey[e] == k; ++e) sum += tx[M - 1 - e];
      tx[M - 1 - j] = sum / (double)(e - j);
    }
  }
  // the draws with key == T: n_tie of them in the tail (slots tx[0, n_tie)), the others in the body at lw = r_T
  double tie = 0.0;
  for (int i = tid; i < c.n_tie; i += LOO_NT) tie += tx[i];
  tie = block_sum<LOO_NW>(tie, red);     // (its barriers also publish the heads' slots)
  const double w_T = (tie + (double)(c.neq - c.n_tie) * exp(r_T - logZ)) / (double)c.neq;
  // c. every draw's weight, in draw order
  double sq = 0.0;
  for (int i = tid; i < S; i += LOO_NT) {
    const float v = val(i);
    double w = 0.0;
    if (v == v) {
      const uint32_t k = f32_key(v);
      if (k > c.T) {
        w = exp((-(double)v - mx) - logZ);
      } else if (k == c.T) {
        w = w_T;
      } else {
        int lo = 0, hi = c.n_low;     // the first slot whose key is not below k: the head of k's run
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (tkey[mid] < k) lo = mid + 1; else hi = mid;
        }
        w = tx[M - 1 - lo];
      }
    }
    sq += w * w;
    if (wout) wout[i] = w;
  }
  sq = block_sum<LOO_NW>(sq, red);
  if (tid == 0 && p.ess_w) p.ess_w[n] = 1.0 / sq;
}

// the tiles [lo, hi) of run u of the draw axis; a run past the last is empty
__device__ __forceinline__ int lxp_run_lo(int u, int runs, int s_tiles) { return u >= runs ? s_tiles : (int)(((long long)u * s_tiles) / runs); }

// NEL: the (row, column) sums of a thread, 1 where the 32 Q columns of a row group fit the group's threads (Q <= 8)
template <int SRC, int NEL>
__global__ __launch_bounds__(256) void k_lxp_apply(const LxpParams p) {
  __shared__ double wt[LXP_MAX_GROUPS][LOO_TILE][LOO_TILE + 1];     // [run of the workgroup][row][draw]; -1: nothing to add
  __shared__ double lse[SRC == LXP_SRC_CLASS ? LXP_MAX_GROUPS : 1][LOO_TILE][LOO_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int S = p.S, Nt = p.Nt, Q = p.Q, runs = p.runs;
  const int G = lxp_groups(Q), TPG = 256 / G, grp = tid / TPG, lt = tid - grp * TPG;
  const int rg0 = blockIdx.x * LOO_TILE, u0 = blockIdx.y * G, u = u0 + grp;
  const int s_tiles = (S + LOO_TILE - 1) / LOO_TILE;
  const int NE = LOO_TILE * Q;
  int steps = 0;
  for (int gg = 0; gg < G; ++gg) steps = max(steps, lxp_run_lo(u0 + gg + 1, runs, s_tiles) - lxp_run_lo(u0 + gg, runs, s_tiles));
  const int my_lo = lxp_run_lo(u, runs, s_tiles), my_hi = lxp_run_lo(u + 1, runs, s_tiles);

  int erow[NEL], eq[NEL], cnt[NEL];
  double aE[NEL], aP[NEL];
#pragma unroll
  for (int k = 0; k < NEL; ++k) {
    const int e = lt + TPG * k;
    const bool on = e < NE && u < runs;
    erow[k] = on ? e / Q : -1;
    eq[k] = on ? e - erow[k] * Q : 0;
    if (on && rg0 + erow[k] >= Nt) erow[k] = -1;
    cnt[k] = 0; aE[k] = 0.0; aP[k] = 0.0;
  }

  for (int step = 0; step < steps; ++step) {
    for (int gg = 0; gg < G; ++gg) {
      const int t = lxp_run_lo(u0 + gg, runs, s_tiles) + step;
      const bool in = t < lxp_run_lo(u0 + gg + 1, runs, s_tiles);
#pragma unroll
      for (int k = 0; k < 4; ++k) {     // draw t * 32 + tx of rows ty, ty + 8, ...: a half-wave reads 32 consecutive weights of one row
        const int row = ty + 8 * k, s = t * LOO_TILE + tx;
        double w = -1.0;
        if (in && s < S && rg0 + row < Nt) {
          const size_t at = (size_t)(rg0 + row) * S + s;
          const float l = p.pk[at];
          if (l == l) w = p.w[at];
        }
        wt[gg][row][tx] = w;
        if constexpr (SRC == LXP_SRC_CLASS) {
          double v = 0.0;
          if (!(w < 0.0)) {     // log sum_c exp z_c of the (draw, row), in fp64
            const float *z = p.raw + ((size_t)s * (size_t)p.ld + rg0 + row) * Q;
            double m = (double)z[0];
            for (int cc = 1; cc < Q; ++cc) m = fmax(m, (double)z[cc]);
            double se = 0.0;
            for (int cc = 0; cc < Q; ++cc) se += exp((double)z[cc] - m);
            v = m + log(se);
          }
          lse[gg][row][tx] = v;
        }
      }
    }
    __syncthreads();
    const int t = my_lo + step;
    if (t < my_hi) {
      for (int j = 0; j < LOO_TILE; ++j) {     // draw after draw, in index order
        const size_t s = (size_t)t * LOO_TILE + j;
#pragma unroll
        for (int k = 0; k < NEL; ++k) {
          if (erow[k] < 0) continue;
          const double w = wt[grp][erow[k]][j];
          if (w < 0.0) continue;
          double h;
          if constexpr (SRC == LXP_SRC_VALUES) {
            h = (double)p.values[(s * (size_t)p.ld + rg0) * Q + (lt + TPG * k)];
          } else if constexpr (SRC == LXP_SRC_REGR) {
            const float *z = p.raw + (s * (size_t)p.ld + rg0 + erow[k]) * 2;
            const double mu = (double)z[0];
            if (eq[k] == 0) h = mu;
            else if (eq[k] == 1) h = mu * mu;
            else {
              const double es = exp((double)z[1]);
              const double sig = es != es ? es : fmin(fmax(es, 1e-6), 1e6);     // row_loglik's clip
              if (eq[k] == 2) h = sig * sig;
              else h = 0.5 * erfc(-(((double)((const float *)p.y)[rg0 + erow[k]] - mu) / sig) * 0.70710678118654752440);
            }
          } else {
            h = exp((double)p.raw[(s * (size_t)p.ld + rg0) * Q + (lt + TPG * k)] - lse[grp][erow[k]][j]);
          }
          aE[k] += w * h;
          aP[k] += h;
          ++cnt[k];
        }
      }
    }
    __syncthreads();
  }

  if (u >= runs) return;
  const size_t NQ = (size_t)Nt * Q;
  double *pe = p.part + (size_t)u * NQ, *pp = p.part + ((size_t)runs + u) * NQ;
#pragma unroll
  for (int k = 0; k < NEL; ++k) {
    if (erow[k] < 0) continue;
    const size_t at = (size_t)rg0 * Q + (lt + TPG * k);
    pe[at] = aE[k];
    pp[at] = aP[k];
    if (eq[k] == 0) p.part_cnt[(size_t)u * Nt + rg0 + erow[k]] = cnt[k];
  }
}

__global__ __launch_bounds__(256) void k_lxp_finish(const LxpParams p) {
  const size_t NQ = (size_t)p.Nt * p.Q, at = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (at >= NQ) return;
  const size_t row = at / p.Q;
  double e = 0.0, m = 0.0;
  long long kept = 0;
  for (int u = 0; u < p.runs; ++u) {     // the runs in index order
    e += p.part[(size_t)u * NQ + at];
    m += p.part[((size_t)p.runs + u) * NQ + at];
    kept += p.part_cnt[(size_t)u * p.Nt + row];
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (p.expect) p.expect[at] = kept < 2 ? qnan : e;
  if (p.posterior) p.posterior[at] = kept < 2 ? qnan : m / (double)kept;
}

hipError_t mile_launch_lxp_rows(const LxpParams &p, hipStream_t st) {
  const dim3 grid((p.Nt + LOO_TILE - 1) / LOO_TILE, p.slices);
  if (p.raw) k_lxp_pack<true><<<grid, 256, 0, st>>>(p);
  else k_lxp_pack<false><<<grid, 256, 0, st>>>(p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (p.S <= LOO_LDS_MAX_S) {
    e = mile_set_max_lds<k_lxp_row<true>>(LOO_LDS_MAX_S * 4);
    if (e != hipSuccess) return e;
    k_lxp_row<true><<<p.Nt, LOO_NT, (size_t)p.S * 4, st>>>(p);
  } else {
    k_lxp_row<false><<<p.Nt, LOO_NT, 0, st>>>(p);
  }
  return hipGetLastError();
}

hipError_t mile_launch_lxp_apply(const LxpParams &p, hipStream_t st) {
  const int G = lxp_groups(p.Q);
  const dim3 grid((p.Nt + LOO_TILE - 1) / LOO_TILE, (p.runs + G - 1) / G);
  const bool one = LOO_TILE * p.Q <= 256;
  if (p.src == LXP_SRC_REGR) k_lxp_apply<LXP_SRC_REGR, 1><<<grid, 256, 0, st>>>(p);     // (Q = 4)
  else if (p.src == LXP_SRC_VALUES && one) k_lxp_apply<LXP_SRC_VALUES, 1><<<grid, 256, 0, st>>>(p);
  else if (p.src == LXP_SRC_VALUES) k_lxp_apply<LXP_SRC_VALUES, LXP_MAX_ELEMS><<<grid, 256, 0, st>>>(p);
  else if (one) k_lxp_apply<LXP_SRC_CLASS, 1><<<grid, 256, 0, st>>>(p);
  else k_lxp_apply<LXP_SRC_CLASS, LXP_MAX_ELEMS><<<grid, 256, 0, st>>>(p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t NQ = (size_t)p.Nt * p.Q;
  k_lxp_finish<<<(unsigned)((NQ + 255) / 256), 256, 0, st>>>(p);
  return hipGetLastError();
}

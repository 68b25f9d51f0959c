// Partial-dependence kernels (mile_pdp.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_block.h"
#include "mile_chan.h"
#include "mile_device.h"
#include "mile_pdp.h"

// One (row slab, draw): z_0 of the slab's rows once, then the (row, feature, grid point) triples in batches of PR pseudo-rows
// through the remaining layers and the head, the drop flags per (row, feature), and the slab's block [nr][Fs][G][P] of val.
__global__ __launch_bounds__(PDP_NT) void k_pdp_fwd(const PdpFwdParams p) {
  extern __shared__ __align__(16) float lds[];
  const PdpNet &sp = p.net;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int e = blockIdx.y, s = blockIdx.x;
  const int nl = sp.n_layers, zs = sp.z_stride, hs = sp.h_stride, R = p.R, PR = p.PR, F = sp.in_features;
  const int Fs = p.Fs, G = p.G, FG = Fs * G, P = sp.widths[nl - 1], w0 = sp.widths[0];
  const float *th = p.theta + (size_t)e * sp.d;
  const float *W0 = th + sp.w_off[0];
  float *z0 = lds, *xs = z0 + (size_t)R * zs;
  int *bad = (int *)(xs + (size_t)R * Fs);
  float *bufA = lds + ((size_t)R * (zs + 2 * Fs) + 3) / 4 * 4, *bufB = bufA + (size_t)PR * hs;   // 16-byte aligned
  const float qnan = __int_as_float(0x7fc00000);
  const int rows_per = (p.Nt + p.SB - 1) / p.SB;
  const int r_begin = s * rows_per, r_end = min(p.Nt, r_begin + rows_per);
  for (int t0 = r_begin; t0 < r_end; t0 += R) {
    const int nr = min(R, r_end - t0);
    {
      const float *b = th + sp.b_off[0];
      for (int idx = tid; idx < nr * w0; idx += nt) {
        const int r = idx / w0, o = idx - r * w0;
        const float *x = p.X + (size_t)(t0 + r) * F;
        float z = b[o];
        for (int i = 0; i < F; ++i) z = fmaf(x[i], W0[i * w0 + o], z);
        z0[r * zs + o] = z;
      }
      for (int idx = tid; idx < nr * Fs; idx += nt) {
        const int r = idx / Fs, i = idx - r * Fs;
        xs[idx] = p.X[(size_t)(t0 + r) * F + p.features[i]];
        bad[idx] = 0;
      }
    }
    __syncthreads();
    float *o_blk = p.val + ((size_t)e * p.Nt + t0) * FG * P;
    const int npr = nr * FG;
    for (int c0 = 0; c0 < npr; c0 += PR) {
      const int nc = min(PR, npr - c0);
      // the first layer of pseudo-row j = (r, i, g): one fmaf on the row's z_0
      for (int idx = tid; idx < nc * w0; idx += nt) {
        const int pr = idx / w0, o = idx - pr * w0, j = c0 + pr, r = j / FG, ig = j - r * FG, i = ig / G;
        float z = fmaf(p.grid[ig] - xs[r * Fs + i], W0[(size_t)p.features[i] * w0 + o], z0[r * zs + o]);
        // a NaN pre-activation stays NaN (act_fwd's ReLU, fmaxf, would answer 0), as in k_sens_jac
        if (nl > 1 && z == z) z = act_fwd(sp.activation, z);
        bufA[pr * hs + o] = z;
      }
      __syncthreads();
      float *cur = bufA, *nxt = bufB;
      const int ngrp = (nc + PDP_T - 1) / PDP_T;
      for (int l = 1; l < nl; ++l) {
        const int win = sp.widths[l - 1], wout = sp.widths[l];
        const float *W = th + sp.w_off[l], *b = th + sp.b_off[l];
        // consecutive threads take consecutive output units of PDP_T pseudo-rows: a wave reads runs of the weight row, once for
        // the PDP_T rows; the tail group reads its last row again and does not write it
        for (int idx = tid; idx < ngrp * wout; idx += nt) {
          const int gq = idx / wout, o = idx - gq * wout, p0 = gq * PDP_T;
          int at[PDP_T];
          float z[PDP_T];
#pragma unroll
          for (int t = 0; t < PDP_T; ++t) { at[t] = min(p0 + t, nc - 1) * hs; z[t] = b[o]; }
          int i = 0;
          for (; i + 4 <= win; i += 4) {   // 16 bytes of each pseudo-row per read; every accumulator still adds i in rising order
            const float w0_ = W[i * wout + o], w1_ = W[(i + 1) * wout + o], w2_ = W[(i + 2) * wout + o], w3_ = W[(i + 3) * wout + o];
#pragma unroll
            for (int t = 0; t < PDP_T; ++t) {
              const float4 a = *(const float4 *)(cur + at[t] + i);
              z[t] = fmaf(a.w, w3_, fmaf(a.z, w2_, fmaf(a.y, w1_, fmaf(a.x, w0_, z[t]))));
            }
          }
          for (; i < win; ++i) {
            const float w = W[i * wout + o];
#pragma unroll
            for (int t = 0; t < PDP_T; ++t) z[t] = fmaf(cur[at[t] + i], w, z[t]);
          }
#pragma unroll
          for (int t = 0; t < PDP_T; ++t)
            if (p0 + t < nc) {
              float v = z[t];
              if (l < nl - 1 && v == v) v = act_fwd(sp.activation, v);
              nxt[(p0 + t) * hs + o] = v;
            }
        }
        __syncthreads();
        float *t = cur; cur = nxt; nxt = t;
      }
      if (sp.task == MILE_TASK_CLASSIFICATION) {
        for (int pr = tid; pr < nc; pr += nt) {   // a thread owns its pseudo-row: in place
          float *z = cur + pr * hs;
          float m = z[0];
          for (int k = 1; k < P; ++k) m = fmaxf(m, z[k]);
          float se = 0.0f;
          for (int k = 0; k < P; ++k) { const float ex = expf(z[k] - m); z[k] = ex; se += ex; }
          for (int k = 0; k < P; ++k) z[k] = z[k] / se;
        }
        __syncthreads();
      }
      float *o = o_blk + (size_t)c0 * P;
      for (int idx = tid; idx < nc * P; idx += nt) {
        const int pr = idx / P, k = idx - pr * P;
        const float v = cur[pr * hs + k];
        o[idx] = v;
        if (!finite_f32(v)) { const int j = c0 + pr, r = j / FG; bad[r * Fs + (j - r * FG) / G] = 1; }   // every writer stores the same 1
      }
      __syncthreads();
    }
    const int GP = G * P;
    for (int idx = tid; idx < npr * P; idx += nt)
      if (bad[idx / GP]) o_blk[idx] = qnan;   // idx / GP = r * Fs + i
    __syncthreads();
  }
}

__global__ __launch_bounds__(PDP_NT) void k_pdp_accum(const PdpAccParams p) {
  const size_t cols = (size_t)p.Nt * p.Q;
  const size_t j = (size_t)blockIdx.x * PDP_NT + threadIdx.x;
  const int sl = blockIdx.y;
  if (j >= cols) return;
  const int s0 = (int)(((long long)sl * p.Sc) / p.slices), s1 = (int)(((long long)(sl + 1) * p.Sc) / p.slices);
  if (s1 <= s0) return;
  const float *v = p.val + (size_t)s0 * cols + j;
  int c = 0;
  double mean = 0.0, M2 = 0.0;
#pragma unroll 4
  for (int s = s0; s < s1; ++s, v += cols) {
    const float x32 = *v;
    if (x32 == x32) {                                    // NaN: the triple was dropped
      ++c;
      const double x = (double)x32, d = x - mean;
      mean += d / (double)c;
      M2 += d * (x - mean);
    }
  }
  if (c == 0) return;
  const size_t a = (size_t)sl * cols + j;
  int ca = p.cnt[a];
  double ma = p.mean[a], M2a = p.M2[a];
  chan_merge(ca, ma, M2a, c, mean, M2);
  p.cnt[a] = ca; p.mean[a] = ma; p.M2[a] = M2a;
}

__global__ __launch_bounds__(PDP_NT) void k_pdp_row_finish(const PdpAccParams p) {
  const size_t cols = (size_t)p.Nt * p.Q;
  const size_t j = (size_t)blockIdx.x * PDP_NT + threadIdx.x;
  if (j >= cols) return;
  int c = 0;
  double mean = 0.0, M2 = 0.0;
  for (int sl = 0; sl < p.slices; ++sl) {
    const size_t a = (size_t)sl * cols + j;
    const int cb = p.cnt[a];
    if (cb == 0) continue;
    chan_merge(c, mean, M2, cb, p.mean[a], p.M2[a]);
  }
  const float qnan = __int_as_float(0x7fc00000);
  if (p.o_mean) p.o_mean[j] = c ? (float)mean : qnan;
  if (p.o_sd) p.o_sd[j] = c > 1 ? (float)sqrt(M2 / (double)(c - 1)) : c ? 0.0f : qnan;
  if (p.dropped && j % p.GP == 0) p.dropped[j / p.GP] = (int32_t)(p.D - c);   // j / GP = n * Fs + i
}

// grid (features x column blocks, draws of the pass).  A workgroup takes columns of ONE feature, so that the split of the rows
// depends on G * P alone and a call on fewer features adds every sum in the order of the full call.  G * P <= 256: one column
// block per feature, thread t is column t % (G P) of row group t / (G P), the groups walk the tile's rows with stride
// 256 / (G P); else a thread per column and one group.
__global__ __launch_bounds__(PDP_NT) void k_pdp_rows(const PdpRowsParams p) {
  __shared__ double ps[PDP_NT];
  __shared__ int pk[PDP_NT];
  const int s = blockIdx.y, tid = threadIdx.x, Q = p.Q, GP = p.GP;
  const int W = GP < PDP_NT ? GP : PDP_NT, NG = PDP_NT / W, nb = (GP + W - 1) / W;
  const int i = blockIdx.x / nb, cb = blockIdx.x - i * nb;
  const int g = tid / W, ci = tid - g * W, gc = cb * W + ci, col = i * GP + gc;
  const float *base = p.val + (size_t)s * p.Nt * Q;
  double sv = 0.0;
  int k = 0;
  if (g < NG && gc < GP)
    for (int n = g; n < p.Nt; n += NG) {
      const float v = base[(size_t)n * Q + col];
      if (v == v) { sv += (double)v; ++k; }
    }
  ps[tid] = sv; pk[tid] = k;
  __syncthreads();
  if (g == 0 && gc < GP) {
    double tv = ps[ci];
    int tk = pk[ci];
    for (int gg = 1; gg < NG; ++gg) { tv += ps[gg * W + ci]; tk += pk[gg * W + ci]; }
    const size_t d = (size_t)(p.d0 + s);
    p.sum[d * Q + col] += tv;
    if (gc == 0) p.kept[d * p.Fs + i] += tk;
  }
}

// grid (column blocks of PDP_FIN_W): lane t / PDP_FIN_W takes the chains lane, lane + 8, ..: Welford over the chain's draws in index
// order; then lane 0 merges the chains' records, which the lanes left in the workspace, in index order.
__global__ __launch_bounds__(PDP_NT) void k_pdp_finish(const PdpRowsParams p) {
  const int tid = threadIdx.x, ci = tid % PDP_FIN_W, lane = tid / PDP_FIN_W, Q = p.Q;
  const int col = blockIdx.x * PDP_FIN_W + ci, f = col / p.GP;
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (col < Q)
    for (int c = lane; c < p.C; c += PDP_NT / PDP_FIN_W) {
      int n = 0;
      double mean = 0.0, M2 = 0.0;
      for (long long j = 0; j < p.S; ++j) {
        const size_t d = (size_t)c * p.S + j;
        const int k = p.kept[d * p.Fs + f];
        if (k > 0) {
          const double m = p.sum[d * Q + col] / (double)k, dl = m - mean;
          ++n;
          mean += dl / (double)n;
          M2 += dl * (m - mean);
          if (p.curves) p.curves[d * Q + col] = (float)m;
        } else if (p.curves) {
          p.curves[d * Q + col] = __int_as_float(0x7fc00000);
        }
      }
      const size_t a = (size_t)c * Q + col;
      p.c_n[a] = n; p.c_mean[a] = mean; p.c_M2[a] = M2;
      if (p.chain_pd) p.chain_pd[a] = n ? mean : qnan;
      if (p.chain_draws && col % p.GP == 0) p.chain_draws[(size_t)c * p.Fs + f] = n;
    }
  __syncthreads();
  if (lane == 0 && col < Q) {
    int n = 0;
    double mean = 0.0, M2 = 0.0;
    for (int c = 0; c < p.C; ++c) {
      const size_t a = (size_t)c * Q + col;
      const int nb = p.c_n[a];
      if (nb) chan_merge(n, mean, M2, nb, p.c_mean[a], p.c_M2[a]);
    }
    if (p.pd_mean) p.pd_mean[col] = n ? mean : qnan;
    if (p.pd_sd) p.pd_sd[col] = n > 1 ? sqrt(M2 / (double)(n - 1)) : n ? 0.0 : qnan;
  }
}

#define PDP_GRID_Y_MAX 65535
hipError_t mile_launch_pdp_fwd(const PdpFwdParams &p0, int Sc, hipStream_t st) {
  const size_t lds = pdp_lds(p0.net, p0.Fs).bytes;
  if (lds > 64 * 1024) {
    const hipError_t e = mile_set_max_lds<k_pdp_fwd>((int)PDP_LDS_MAX);
    if (e != hipSuccess) return e;
  }
  const size_t per_draw = (size_t)p0.Nt * p0.Fs * p0.G * p0.net.widths[p0.net.n_layers - 1];
  for (int s0 = 0; s0 < Sc; s0 += PDP_GRID_Y_MAX) {
    PdpFwdParams p = p0;
    p.theta = p0.theta + (size_t)s0 * p0.net.d;
    p.val = p0.val + (size_t)s0 * per_draw;
    const int ns = Sc - s0 < PDP_GRID_Y_MAX ? Sc - s0 : PDP_GRID_Y_MAX;
    k_pdp_fwd<<<dim3(p.SB, ns), PDP_NT, lds, st>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t mile_launch_pdp_accum(const PdpAccParams &p, hipStream_t st) {
  const size_t cols = (size_t)p.Nt * p.Q;
  k_pdp_accum<<<dim3((unsigned)((cols + PDP_NT - 1) / PDP_NT), p.slices), PDP_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_pdp_row_finish(const PdpAccParams &p, hipStream_t st) {
  const size_t cols = (size_t)p.Nt * p.Q;
  k_pdp_row_finish<<<(unsigned)((cols + PDP_NT - 1) / PDP_NT), PDP_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_pdp_rows(const PdpRowsParams &p0, hipStream_t st) {
  const int W = p0.GP < PDP_NT ? p0.GP : PDP_NT, nb = (p0.GP + W - 1) / W;
  for (int s0 = 0; s0 < p0.Sc; s0 += PDP_GRID_Y_MAX) {
    PdpRowsParams p = p0;
    p.val = p0.val + (size_t)s0 * p0.Nt * p0.Q;
    p.d0 = p0.d0 + s0;
    const int ns = p0.Sc - s0 < PDP_GRID_Y_MAX ? p0.Sc - s0 : PDP_GRID_Y_MAX;
    k_pdp_rows<<<dim3(p.Fs * nb, ns), PDP_NT, 0, st>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t mile_launch_pdp_finish(const PdpRowsParams &p, hipStream_t st) {
  k_pdp_finish<<<(p.Q + PDP_FIN_W - 1) / PDP_FIN_W, PDP_NT, 0, st>>>(p);
  return hipGetLastError();
}

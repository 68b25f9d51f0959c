// Input-sensitivity kernels (mile_sens.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_block.h"
#include "mile_chan.h"
#include "mile_device.h"
#include "mile_sens.h"

// One (row slab, draw): the forward of k_fwd_generic with every layer's activations kept, the P backward sweeps through the two
// delta buffers, the head rule, the drop flag, and the tile's block [nr][P][F] of jac as one contiguous run.
__global__ __launch_bounds__(SENS_NT) void k_sens_jac(const SensJacParams p) {
  extern __shared__ float lds[];
  const SensNet &sp = p.net;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int e = blockIdx.y, s = blockIdx.x;
  const int nl = sp.n_layers, as = sp.act_stride, ds = sp.d_stride, R = p.R, F = sp.in_features;
  const int P = sp.widths[nl - 1], PF = P * F;
  const float *th = p.theta + (size_t)e * sp.d;
  float *act = lds, *dA = act + (size_t)R * as, *dB = dA + (size_t)R * P * ds;
  int *drop = (int *)(dB + (size_t)R * P * ds);
  const int rows_per = (p.Nt + p.SB - 1) / p.SB;
  const int r_begin = s * rows_per, r_end = min(p.Nt, r_begin + rows_per);
  for (int t0 = r_begin; t0 < r_end; t0 += R) {
    const int nr = min(R, r_end - t0);
    for (int idx = tid; idx < nr * F; idx += nt) {
      const int r = idx / F, c = idx - r * F;
      act[r * as + c] = p.X[(size_t)(t0 + r) * F + c];
    }
    __syncthreads();
    for (int l = 0; l < nl; ++l) {
      const int win = l == 0 ? F : sp.widths[l - 1], wout = sp.widths[l];
      const float *W = th + sp.w_off[l], *b = th + sp.b_off[l];
      for (int idx = tid; idx < nr * wout; idx += nt) {
        const int r = idx / wout, o = idx - r * wout;
        const float *a = act + r * as + sp.act_off[l];
        float z = b[o];
        for (int i = 0; i < win; ++i) z = fmaf(a[i], W[i * wout + o], z);
        // a NaN pre-activation stays NaN (act_fwd's ReLU, fmaxf, would answer 0): the pair is then dropped by its raw outputs,
        // as IEEE arithmetic and the fp64 restatement have it, and not kept with a Jacobian that ignores the unit
        if (l < nl - 1 && z == z) z = act_fwd(sp.activation, z);
        act[r * as + sp.act_off[l + 1] + o] = z;
      }
      __syncthreads();
    }
    // the sweeps: cur holds d r_p / d z_l [r][p][wout_l], nxt receives d r_p / d z_{l-1} [r][p][win_l]; the last is Jraw [r][p][F]
    float *cur = dA, *nxt = dB;
    for (int l = nl - 1; l >= 0; --l) {
      const int win = l == 0 ? F : sp.widths[l - 1], wout = sp.widths[l];
      const float *W = th + sp.w_off[l];
      // consecutive threads take consecutive (row, p) of one input unit i: a wave reads one weight row (one cache line per
      // load, not 64) and its lanes' deltas lie d_stride apart, on different banks
      const int nrp = nr * P;
      for (int idx = tid; idx < nrp * win; idx += nt) {
        const int i = idx / nrp, rp = idx - i * nrp, r = rp / P;
        const float *w = W + (size_t)i * wout;
        float g;
        if (l == nl - 1) {
          g = w[rp - r * P];           // the seed is the unit vector of output p
        } else {
          const float *dz = cur + (size_t)rp * ds;
          g = 0.0f;
          for (int o = 0; o < wout; ++o) g = fmaf(dz[o], w[o], g);
        }
        if (l > 0) g *= act_bwd(sp.activation, act[r * as + sp.act_off[l] + i]);
        nxt[(size_t)rp * ds + i] = g;
      }
      __syncthreads();
      float *t = cur; cur = nxt; nxt = t;
    }
    if (sp.task == MILE_TASK_CLASSIFICATION) {
      for (int r = tid; r < nr; r += nt) {   // pi of row r into the free buffer
        const float *z = act + r * as + sp.act_off[nl];
        float *pi = nxt + (size_t)r * P * ds;
        float m = z[0];
        for (int k = 1; k < P; ++k) m = fmaxf(m, z[k]);
        float se = 0.0f;
        for (int k = 0; k < P; ++k) { const float ex = expf(z[k] - m); pi[k] = ex; se += ex; }
        for (int k = 0; k < P; ++k) pi[k] = pi[k] / se;
      }
      __syncthreads();
      for (int idx = tid; idx < nr * F; idx += nt) {   // a thread owns column f of row r for every class: in place
        const int r = idx / F, f = idx - r * F;
        const float *pi = nxt + (size_t)r * P * ds;
        float *j = cur + (size_t)r * P * ds + f;
        float t = 0.0f;
        for (int k = 0; k < P; ++k) t = fmaf(pi[k], j[(size_t)k * ds], t);
        for (int k = 0; k < P; ++k) j[(size_t)k * ds] = pi[k] * (j[(size_t)k * ds] - t);
      }
      __syncthreads();
    }
    for (int r = tid; r < nr; r += nt) {
      const float *z = act + r * as + sp.act_off[nl];
      bool fin = true;
      for (int k = 0; k < P; ++k) fin = fin && finite_f32(z[k]);
      for (int k = 0; k < P; ++k) {
        const float *j = cur + ((size_t)r * P + k) * ds;
        for (int f = 0; f < F; ++f) fin = fin && finite_f32(j[f]);
      }
      drop[r] = fin ? 0 : 1;
    }
    __syncthreads();
    float *o = p.jac + ((size_t)e * p.Nt + t0) * PF;
    for (int idx = tid; idx < nr * PF; idx += nt) {
      const int r = idx / PF, q = idx - r * PF, k = q / F, f = q - k * F;
      const float v = cur[((size_t)r * P + k) * ds + f];
      o[idx] = q == 0 && drop[r] ? __int_as_float(0x7fc00000) : v;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(SENS_NT) void k_sens_accum(const SensAccParams p) {
  const size_t cols = (size_t)p.Nt * p.PF;
  const size_t j = (size_t)blockIdx.x * SENS_NT + threadIdx.x;
  const int sl = blockIdx.y;
  if (j >= cols) return;
  const int s0 = (int)(((long long)sl * p.Sc) / p.slices), s1 = (int)(((long long)(sl + 1) * p.Sc) / p.slices);
  if (s1 <= s0) return;
  const size_t row0 = j / p.PF * p.PF;                 // entry 0 of the row's block: NaN marks a dropped pair
  const float *v = p.jac + (size_t)s0 * cols + j, *flag = p.jac + (size_t)s0 * cols + row0;
  int c = 0, pos = 0;
  double mean = 0.0, M2 = 0.0;
#pragma unroll 4
  for (int s = s0; s < s1; ++s, v += cols, flag += cols) {
    const float f0 = *flag, x32 = *v;
    if (f0 == f0) {
      ++c;
      const double x = (double)x32, d = x - mean;
      mean += d / (double)c;
      M2 += d * (x - mean);
      pos += x32 > 0.0f ? 1 : 0;
    }
  }
  if (c == 0) return;
  const size_t a = (size_t)sl * cols + j;
  int ca = p.cnt[a];
  double ma = p.mean[a], M2a = p.M2[a];
  chan_merge(ca, ma, M2a, c, mean, M2);
  p.cnt[a] = ca; p.mean[a] = ma; p.M2[a] = M2a; p.pos[a] += pos;
}

__global__ __launch_bounds__(SENS_NT) void k_sens_finish(const SensAccParams p) {
  const size_t cols = (size_t)p.Nt * p.PF;
  const size_t j = (size_t)blockIdx.x * SENS_NT + threadIdx.x;
  if (j >= cols) return;
  int c = 0;
  long long pos = 0;
  double mean = 0.0, M2 = 0.0;
  for (int sl = 0; sl < p.slices; ++sl) {
    const size_t a = (size_t)sl * cols + j;
    const int cb = p.cnt[a];
    if (cb == 0) continue;
    chan_merge(c, mean, M2, cb, p.mean[a], p.M2[a]);
    pos += p.pos[a];
  }
  const float qnan = __int_as_float(0x7fc00000);
  if (p.o_mean) p.o_mean[j] = c ? (float)mean : qnan;
  if (p.o_sd) p.o_sd[j] = c > 1 ? (float)sqrt(M2 / (double)(c - 1)) : c ? 0.0f : qnan;
  if (p.o_pos) p.o_pos[j] = c ? (float)((double)pos / (double)c) : qnan;
  if (p.dropped && j % p.PF == 0) p.dropped[j / p.PF] = (int32_t)(p.D - c);
}

// grid (column blocks, chains).  PF <= 256: one column block, thread t is column t % PF of pair group t / PF, the groups walk the
// chain's (draw, row) pairs of this pass with stride 256 / PF; else a thread per column and one group.
__global__ __launch_bounds__(SENS_NT) void k_sens_chain(const SensChainParams p) {
  __shared__ double ps[SENS_NT], pa[SENS_NT];
  __shared__ int pk[SENS_NT];
  const int c = blockIdx.y, tid = threadIdx.x, PF = p.PF;
  const int W = PF < SENS_NT ? PF : SENS_NT, G = SENS_NT / W;
  const int g = tid / W, ci = tid - g * W, col = blockIdx.x * W + ci;
  // the chain's draws inside the pass, as draws of the pass
  const long long lo = (long long)c * p.S - p.d0, hi = lo + p.S;
  const long long a = lo > 0 ? lo : 0, b = hi < p.Sc ? hi : p.Sc;
  if (b <= a) return;
  const size_t npairs = (size_t)(b - a) * p.Nt;
  const float *base = p.jac + (size_t)a * p.Nt * PF;
  double sj = 0.0, sa = 0.0;
  int k = 0;
  if (g < G && col < PF)
    for (size_t i = g; i < npairs; i += G) {
      const float *blk = base + i * PF;
      const float f0 = blk[0], v = blk[col];
      if (f0 == f0) { sj += (double)v; sa += fabs((double)v); ++k; }
    }
  ps[tid] = sj; pa[tid] = sa; pk[tid] = k;
  __syncthreads();
  if (g == 0 && col < PF) {
    double tj = ps[ci], ta = pa[ci];
    for (int gg = 1; gg < G; ++gg) { tj += ps[gg * W + ci]; ta += pa[gg * W + ci]; }
    p.sum[(size_t)c * PF + col] += tj;
    p.abs[(size_t)c * PF + col] += ta;
    if (col == 0) {
      long long tk = 0;
      for (int gg = 0; gg < G; ++gg) tk += pk[gg * W];
      p.kept[c] += tk;
    }
  }
}

__global__ __launch_bounds__(SENS_NT) void k_sens_chain_finish(const SensChainParams p) {
  const int i = blockIdx.x * SENS_NT + threadIdx.x;
  if (i >= p.C * p.PF) return;
  const int c = i / p.PF;
  const long long k = p.kept[c];
  const double qnan = __longlong_as_double(0x7ff8000000000000LL);
  if (p.o_ape) p.o_ape[i] = k ? p.sum[i] / (double)k : qnan;
  if (p.o_abs) p.o_abs[i] = k ? p.abs[i] / (double)k : qnan;
  if (p.o_kept && i == c * p.PF) p.o_kept[c] = k;
}

#define SENS_GRID_Y_MAX 65535
hipError_t mile_launch_sens_jac(const SensJacParams &p0, int Sc, hipStream_t st) {
  const size_t lds = sens_lds(p0.net);
  if (lds > 64 * 1024) {
    const hipError_t e = mile_set_max_lds<k_sens_jac>((int)SENS_LDS_MAX);
    if (e != hipSuccess) return e;
  }
  const size_t P = p0.net.widths[p0.net.n_layers - 1], per_draw = (size_t)p0.Nt * P * p0.net.in_features;
  for (int s0 = 0; s0 < Sc; s0 += SENS_GRID_Y_MAX) {
    SensJacParams p = p0;
    p.theta = p0.theta + (size_t)s0 * p0.net.d;
    p.jac = p0.jac + (size_t)s0 * per_draw;
    const int ns = Sc - s0 < SENS_GRID_Y_MAX ? Sc - s0 : SENS_GRID_Y_MAX;
    k_sens_jac<<<dim3(p.SB, ns), SENS_NT, lds, st>>>(p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

hipError_t mile_launch_sens_accum(const SensAccParams &p, hipStream_t st) {
  const size_t cols = (size_t)p.Nt * p.PF;
  k_sens_accum<<<dim3((unsigned)((cols + SENS_NT - 1) / SENS_NT), p.slices), SENS_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_sens_finish(const SensAccParams &p, hipStream_t st) {
  const size_t cols = (size_t)p.Nt * p.PF;
  k_sens_finish<<<(unsigned)((cols + SENS_NT - 1) / SENS_NT), SENS_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_sens_chain(const SensChainParams &p, hipStream_t st) {
  const int W = p.PF < SENS_NT ? p.PF : SENS_NT;
  k_sens_chain<<<dim3((p.PF + W - 1) / W, p.C), SENS_NT, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_sens_chain_finish(const SensChainParams &p, hipStream_t st) {
  k_sens_chain_finish<<<(p.C * p.PF + SENS_NT - 1) / SENS_NT, SENS_NT, 0, st>>>(p);
  return hipGetLastError();
}

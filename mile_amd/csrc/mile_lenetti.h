// LeNetti target (src/models/images/cnns.py:69-121, LeNettiConfig src/config/models/cnns.py), fp32 (MILE_GRAD_LENETTI_F32):
//   x NCHW -> NHWC -> Conv(1, 3x3, stride 1, pad 2) -> act -> flatten (P = (H+2)(W+2) features, index h*(W+2) + w)
//   -> Dense(8) -> act -> Dense(8) -> act -> Dense(8) -> act -> Dense(out)
// One fused forward + backward launch per gradient: k_grad_lenetti, grid (S row ranges, E chains), 256 threads.  Each thread
// owns PPT conv-output pixels p = tid + 256 k and holds their fc1 kernel rows W1[p][0..8) in registers, so the fc1 kernel
// gradient and the 9C conv-weight gradient accumulate in registers over all of the workgroup's images and go to the slab once.
// Images go in tiles of T: staged zero-padded in LDS, conv + activation per (image, pixel) into registers, the fc1 products
// as per-thread partial sums that one butterfly reduce-scatter per wave (T*8 values over 64 lanes: ~1 shuffle per value)
// and a 4-wave LDS combine turn into z1[T][8].  The 8-wide tail (fc2..fc4, the head and its backward pass) runs in wave 0,
// one lane per (image, unit), exchanging through lane shuffles; then every thread forms dz0 = (dz1 W1^T) * act'(a0) for its
// pixels and accumulates the fc1 and conv gradients.  Plain fp32 (fmaf) throughout.
// k_fwd_lenetti is the same body without the backward half: per-row log-likelihoods for mile_pointwise_loglik.
#pragma once
#include "mile_device.h"
#include "mile_grad_generic.h"

#define LENETTI_NT 256
#define LENETTI_MAX_C 4
#define LENETTI_MAX_PPT 8          // P <= 2048 conv-output pixels
#define LENETTI_MAX_K 16           // output width (two slots of the 8 tail lanes of an image)

struct LeNettiGeom {
  int C, H, W, K, Ho, Wo, P;
  // parameter offsets in the raveled vector (ravel_pytree order: conv1, fc1, fc2, fc3, fc4; bias before kernel)
  int b_c, k_c, b_1, k_1, b_2, k_2, b_3, k_3, b_4, k_4, d;
};

struct LeNettiParams {
  LeNettiGeom g;
  int activation, task;
  const float *theta;   // [E, d] (gradient) or [S, d] (evaluation)
  const float *X;       // [N, C*H*W] NCHW rows
  const void *y;        // [N] fp32 (regr) or int32 (classification)
  float *slabs;         // [E, S, dp] likelihood-gradient slabs (gradient)
  float *llpart;        // [E, S] (gradient)
  float *out;           // [S, N] per-row log-likelihoods (evaluation); RAW: [S, N, K] raw outputs, y unread
  int N, S, dp;
};

// LDS floats: image tiles [T][C][H+4][W+4], tail weights, 4 x 64 partial sums, dz1 [T][8], tail gradients [TG_N][64]
__host__ __device__ inline int lenetti_tail_floats(int K) { return 64 + 64 + 8 * K + 24 + K; }
__host__ __device__ inline size_t lenetti_lds_bytes(const LeNettiGeom &g, int T) {
  return ((size_t)T * g.C * (g.H + 4) * (g.W + 4) + (lenetti_tail_floats(g.K) + 3) / 4 * 4 + 4 * 64 + 64 + 64 * (24 + LENETTI_MAX_K)) * 4;
}

// float division of small non-negative ints (n < 2^22, d < 2^16): exact
__device__ __forceinline__ int lenetti_div(int n, float inv) { return (int)(((float)n + 0.5f) * inv); }

// Reduce-scatter over the 64 lanes of a wave: on return lane l holds the wave-wide sum of value index l >> (6 - log2 NV)
// in v[0].  Halving stages while more than one value is left (send one half, keep the other), plain adds after that.
template <int NV, int H, int M>
__device__ __forceinline__ void lenetti_rs_stage(float (&v)[NV], int lane) {
  if constexpr (M >= 1) {
    if constexpr (H >= 1) {
      const bool up = (lane & M) != 0;
#pragma unroll
      for (int q = 0; q < H; ++q) {
        const float send = up ? v[q] : v[q + H];
        const float keep = up ? v[q + H] : v[q];
        v[q] = keep + __shfl_xor(send, M);
      }
      lenetti_rs_stage<NV, H / 2, M / 2>(v, lane);
    } else {
      v[0] += __shfl_xor(v[0], M);
      lenetti_rs_stage<NV, 0, M / 2>(v, lane);
    }
  }
}
template <int NV>
__device__ __forceinline__ void lenetti_reduce_scatter(float (&v)[NV], int lane) {
  static_assert(NV >= 1 && NV <= 64 && (NV & (NV - 1)) == 0, "power of two <= 64");
  lenetti_rs_stage<NV, NV / 2, 32>(v, lane);
}

// tail gradient accumulators of wave 0, lane-private in LDS: entry q of lane l at tg[q * 64 + l]
enum { TG_W2 = 0, TG_W3 = 8, TG_W4 = 16, TG_B1 = 16 + LENETTI_MAX_K, TG_B2, TG_B3, TG_B4, TG_N = TG_B4 + 2 };

template <int PPT, int T, int CM, bool GRAD, bool RAW = false>
__device__ __forceinline__ void lenetti_body(const LeNettiParams &p) {
  static_assert(T == 4 || T == 2, "tile of 4 or 2 images");
  constexpr int NV = T * 8, SHIFT = T == 4 ? 1 : 2;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const LeNettiGeom &g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int e = blockIdx.y, s = blockIdx.x;
  const int C = g.C, H = g.H, W = g.W, K = g.K, Wo = g.Wo, P = g.P, Hp = H + 4, Wp = W + 4, plane = Hp * Wp, img = C * plane;
  const int F = C * H * W, act = p.activation;
  const float *th = p.theta + (size_t)e * g.d;
  float *xt = lds;                                   // [T][C][Hp][Wp], zero border
  float *tw = xt + T * img;                          // W2[64] W3[64] W4[8K] b1[8] b2[8] b3[8] b4[K]
  float *red = tw + (lenetti_tail_floats(K) + 3) / 4 * 4;   // [4][64]
  float *dz1s = red + 4 * 64;                        // [T][8]
  float *tg = dz1s + 64;                             // [TG_N][64]
  float *W2 = tw, *W3 = tw + 64, *W4 = tw + 128, *B1 = W4 + 8 * K, *B2 = B1 + 8, *B3 = B2 + 8, *B4 = B3 + 8;

  for (int i = tid; i < T * img; i += LENETTI_NT) xt[i] = 0.0f;
  for (int i = tid; i < 64; i += LENETTI_NT) { W2[i] = th[g.k_2 + i]; W3[i] = th[g.k_3 + i]; }
  for (int i = tid; i < 8 * K; i += LENETTI_NT) W4[i] = th[g.k_4 + i];
  if (tid < 8) { B1[tid] = th[g.b_1 + tid]; B2[tid] = th[g.b_2 + tid]; B3[tid] = th[g.b_3 + tid]; }
  if (tid < K) B4[tid] = th[g.b_4 + tid];

  // the thread's pixels: tile offset of their top-left tap, fc1 kernel rows
  int poff[PPT];
  bool pval[PPT];
  float w1[PPT][8];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int px = tid + LENETTI_NT * k;
    pval[k] = px < P;
    const int pc = pval[k] ? px : 0, yy = pc / Wo, xx = pc - yy * Wo;
    poff[k] = yy * Wp + xx;
#pragma unroll
    for (int j = 0; j < 8; ++j) w1[k][j] = pval[k] ? th[g.k_1 + (size_t)pc * 8 + j] : 0.0f;
  }
  float kc[9 * CM];                                  // [tap][channel], channel stride CM
#pragma unroll
  for (int q = 0; q < 9 * CM; ++q) {
    const int t = q / CM, c = q % CM;
    kc[q] = c < C ? th[g.k_c + t * C + c] : 0.0f;
  }
  const float cb = th[g.b_c];

  // gradient accumulators: fc1 kernel rows and conv weights (all threads), the tail's (wave 0: lane (i, j) -> unit j)
  float gw1[PPT][8], gk[9 * CM], gcb = 0.0f, ll_acc = 0.0f;
#pragma unroll
  for (int k = 0; k < PPT; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) gw1[k][j] = 0.0f;
#pragma unroll
  for (int q = 0; q < 9 * CM; ++q) gk[q] = 0.0f;
  if (GRAD && tid < 64)
    for (int q = 0; q < TG_N; ++q) tg[q * 64 + tid] = 0.0f;

  // rows of this workgroup: gradient -> row range s of S for chain e; evaluation -> row block s of gridDim.x for sample e
  const int nsplit = GRAD ? p.S : (int)gridDim.x;
  const int rows_per = (p.N + nsplit - 1) / nsplit;
  const int r_begin = min(p.N, s * rows_per), r_end = min(p.N, r_begin + rows_per);
  const float invW = 1.0f / (float)W, invH = 1.0f / (float)H;
  const int ti = lane >> 3, tj = lane & 7;           // tail lane: image, unit

  for (int t0 = r_begin; t0 < r_end; t0 += T) {
    const int nt = min(T, r_end - t0);
    __syncthreads();                                 // previous tile's readers are done
    {   // stage the tile's images (rows are contiguous in X); images past nt are zero.  U loads per thread in flight before
        // the first LDS store: one HBM round trip per tile for MNIST-sized images (4 x 784 floats over 256 threads)
      const float *src = p.X + (size_t)t0 * F;
      const int n = T * F, nv = nt * F;
      constexpr int U = 16;
      for (int i0 = tid; i0 < n; i0 += LENETTI_NT * U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + LENETTI_NT * u;
          v[u] = i < nv ? src[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + LENETTI_NT * u;
          if (i < n) {
            const int row = lenetti_div(i, invW), w = i - row * W;        // row over (image, channel, h)
            const int pl = lenetti_div(row, invH), h = row - pl * H;      // plane = image * C + channel
            xt[pl * plane + (h + 2) * Wp + w + 2] = v[u];
          }
        }
      }
    }
    __syncthreads();
    // ---- forward: conv + activation per (image, pixel), fc1 partial sums
    float a0[T][PPT];
    float part[NV];
#pragma unroll
    for (int i = 0; i < T; ++i) {
      const float *xi = xt + i * img;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        float z = cb;
#pragma unroll
        for (int c = 0; c < CM; ++c) {   // (unrolled: constant register indices)
          if (c >= C) break;
          const float *xc = xi + c * plane + poff[k];
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) z = fmaf(xc[kh * Wp + kw], kc[(kh * 3 + kw) * CM + c], z);
        }
        a0[i][k] = pval[k] ? act_fwd(act, z) : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < PPT; ++k) acc = fmaf(a0[i][k], w1[k][j], acc);
        part[i * 8 + j] = acc;
      }
    }
    lenetti_reduce_scatter<NV>(part, lane);
    if ((lane & ((1 << SHIFT) - 1)) == 0) red[wave * 64 + (lane >> SHIFT)] = part[0];
    __syncthreads();
    // ---- tail: wave 0, lane (image ti, unit tj)
    if (wave == 0) {
      const bool live = ti < nt;
      const int base = lane & ~7;
      float z1 = 0.0f;
      if (ti < T) z1 = B1[tj] + ((red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]));
      const float h1 = act_fwd(act, z1);
      float z2 = B2[tj], z3 = B3[tj];
#pragma unroll
      for (int k = 0; k < 8; ++k) z2 = fmaf(__shfl(h1, base + k), W2[k * 8 + tj], z2);
      const float h2 = act_fwd(act, z2);
#pragma unroll
      for (int k = 0; k < 8; ++k) z3 = fmaf(__shfl(h2, base + k), W3[k * 8 + tj], z3);
      const float h3 = act_fwd(act, z3);
      float o[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int c = tj + 8 * m;
        float z = c < K ? B4[c] : 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float hk = __shfl(h3, base + k);
          if (c < K) z = fmaf(hk, W4[k * K + c], z);
        }
        o[m] = z;
      }
      if constexpr (RAW) {   // lane (ti, tj) holds outputs tj and tj + 8 of image ti: the tile's rows are one contiguous run of out
        if (live) {
          float *dst = p.out + ((size_t)e * p.N + t0 + ti) * K;
          if (tj < K) dst[tj] = o[0];
          if (tj + 8 < K) dst[tj + 8] = o[1];
        }
        continue;           // (the other waves leave the tile below; the barrier is the loop's first statement)
      }
      // head: regression (mu, log sigma) or softmax over K logits, as row_loss_regr / k_grad_generic
      float ll = 0.0f, dout[2] = {0.0f, 0.0f};
      if (p.task == MILE_TASK_REGRESSION) {
        const float mu = __shfl(o[0], base), sr = __shfl(o[0], base + 1);
        const float yv = live ? ((const float *)p.y)[t0 + ti] : 0.0f;
        if (GRAD) {
          float dmu, dsr;
          ll = row_loss_regr(mu, sr, yv, dmu, dsr);
          dout[0] = tj == 0 ? dmu : (tj == 1 ? dsr : 0.0f);
        } else {
          const float es = expf(sr);
          const float sig = isnan(es) ? es : fminf(fmaxf(es, 1e-6f), 1e6f);
          const float r = (yv - mu) / sig;
          ll = -0.5f * r * r - logf(sig) - 0.91893853320467274f;
        }
      } else {
        float mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < 2; ++m)
          if (tj + 8 * m < K) mx = fmaxf(mx, o[m]);
        mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2)); mx = fmaxf(mx, __shfl_xor(mx, 4));
        float se = 0.0f;
#pragma unroll
        for (int m = 0; m < 2; ++m)
          if (tj + 8 * m < K) se += expf(o[m] - mx);
        se += __shfl_xor(se, 1); se += __shfl_xor(se, 2); se += __shfl_xor(se, 4);
        const float lse = mx + logf(se);
        const int yi = live ? ((const int32_t *)p.y)[t0 + ti] : 0;
        const float oy0 = __shfl(o[0], base + (yi & 7)), oy1 = __shfl(o[1], base + (yi & 7));
        ll = (yi < 8 ? oy0 : oy1) - lse;
        const bool bad = isnan(ll);
        if (GRAD) {
#pragma unroll
          for (int m = 0; m < 2; ++m) {
            const int c = tj + 8 * m;
            dout[m] = (bad || c >= K) ? 0.0f : ((c == yi ? 1.0f : 0.0f) - expf(o[m] - lse));
          }
          if (bad) ll = 0.0f;
        }
      }
      if (!GRAD) {
        if (live && tj == 0) p.out[(size_t)e * p.N + t0 + ti] = ll;
      } else {
        if (!live) { dout[0] = 0.0f; dout[1] = 0.0f; }
        if (live && tj == 0) ll_acc += ll;
        // backward through the tail; weight gradients of unit tj's rows, summed over the images later
        float dh3 = 0.0f;
#pragma unroll
        for (int c = 0; c < LENETTI_MAX_K; ++c) {
          const float dc = __shfl(dout[c >> 3], base + (c & 7));
          if (c < K) {
            dh3 = fmaf(dc, W4[tj * K + c], dh3);
            tg[(TG_W4 + c) * 64 + lane] = fmaf(h3, dc, tg[(TG_W4 + c) * 64 + lane]);
          }
        }
        const float dz3 = dh3 * act_bwd(act, h3);
        float dh2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float dk = __shfl(dz3, base + k);
          dh2 = fmaf(dk, W3[tj * 8 + k], dh2);
          tg[(TG_W3 + k) * 64 + lane] = fmaf(h2, dk, tg[(TG_W3 + k) * 64 + lane]);
        }
        const float dz2 = dh2 * act_bwd(act, h2);
        float dh1 = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float dk = __shfl(dz2, base + k);
          dh1 = fmaf(dk, W2[tj * 8 + k], dh1);
          tg[(TG_W2 + k) * 64 + lane] = fmaf(h1, dk, tg[(TG_W2 + k) * 64 + lane]);
        }
        const float dz1 = dh1 * act_bwd(act, h1);
        tg[TG_B4 * 64 + lane] += dout[0]; tg[(TG_B4 + 1) * 64 + lane] += dout[1];
        tg[TG_B3 * 64 + lane] += dz3; tg[TG_B2 * 64 + lane] += dz2; tg[TG_B1 * 64 + lane] += dz1;
        if (ti < T) dz1s[lane] = dz1;
      }
    }
    if (!GRAD) continue;
    __syncthreads();
    // ---- backward over the tile: dz0 = (dz1 W1^T) * act'(a0); fc1 kernel and conv weight gradients
#pragma unroll
    for (int i = 0; i < T; ++i) {
      if (i >= nt) break;
      float dz[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) dz[j] = dz1s[i * 8 + j];
      const float *xi = xt + i * img;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        float da = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          da = fmaf(dz[j], w1[k][j], da);
          gw1[k][j] = fmaf(a0[i][k], dz[j], gw1[k][j]);
        }
        const float dz0 = pval[k] ? da * act_bwd(act, a0[i][k]) : 0.0f;
        gcb += dz0;
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          if (c >= C) break;
          const float *xc = xi + c * plane + poff[k];
#pragma unroll
          for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
              float &acc = gk[(kh * 3 + kw) * CM + c];
              acc = fmaf(xc[kh * Wp + kw], dz0, acc);
            }
        }
      }
    }
  }
  if (!GRAD) return;

  // ---- write the slab row (every entry exactly once)
  float *slab = p.slabs + ((size_t)e * p.S + s) * p.dp;
#pragma unroll
  for (int k = 0; k < PPT; ++k)
    if (pval[k]) {
      float *dst = slab + g.k_1 + (size_t)(tid + LENETTI_NT * k) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = gw1[k][j];
    }
  __syncthreads();                                   // red / dz1s are reused below
  float *cred = red;                                 // [4][9C + 1] (4 * 37 <= 256 + 64 floats)
#pragma unroll
  for (int q = 0; q < 9 * CM; ++q) {
    const int t = q / CM, c = q % CM;   // -> flax order [kh][kw][c]
    if (c < C) {
      const float v = wave_sum(gk[q]);
      if (lane == 0) cred[wave * (9 * C + 1) + t * C + c] = v;
    }
  }
  {
    const float v = wave_sum(gcb);
    if (lane == 0) cred[wave * (9 * C + 1) + 9 * C] = v;
  }
  if (wave == 0) {   // tail gradients: sum the image groups of wave 0 (lanes with the same unit tj), one entry at a time
    for (int q = 0; q < TG_N; ++q) {
      float v = tg[q * 64 + lane];
      v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
      if (lane < 8) {
        if (q < TG_W3) slab[g.k_2 + lane * 8 + q - TG_W2] = v;
        else if (q < TG_W4) slab[g.k_3 + lane * 8 + q - TG_W3] = v;
        else if (q < TG_B1) { if (q - TG_W4 < K) slab[g.k_4 + lane * K + q - TG_W4] = v; }
        else if (q == TG_B1) slab[g.b_1 + lane] = v;
        else if (q == TG_B2) slab[g.b_2 + lane] = v;
        else if (q == TG_B3) slab[g.b_3 + lane] = v;
        else if (q == TG_B4) { if (lane < K) slab[g.b_4 + lane] = v; }
        else if (lane + 8 < K) slab[g.b_4 + lane + 8] = v;
      }
    }
    const float ll = wave_sum(ll_acc);
    if (lane == 0) p.llpart[(size_t)e * p.S + s] = ll;
  }
  __syncthreads();
  if (tid <= 9 * C) {
    const int n = 9 * C + 1;
    const float v = (cred[tid] + cred[n + tid]) + (cred[2 * n + tid] + cred[3 * n + tid]);
    slab[tid < 9 * C ? g.k_c + tid : g.b_c] = v;
  }
}

template <int PPT, int T, int CM>
__global__ __launch_bounds__(LENETTI_NT) void k_grad_lenetti(const LeNettiParams p) { lenetti_body<PPT, T, CM, true>(p); }

template <int PPT, int T, int CM>
__global__ __launch_bounds__(LENETTI_NT) void k_fwd_lenetti(const LeNettiParams p) { lenetti_body<PPT, T, CM, false>(p); }
template <int PPT, int T, int CM>
__global__ __launch_bounds__(LENETTI_NT) void k_out_lenetti(const LeNettiParams p) { lenetti_body<PPT, T, CM, false, true>(p); }

// host: images per tile (registers hold a0 [T][PPT]) and the launch, in mile_lenetti.hip (its own translation unit)
inline int lenetti_ppt(const LeNettiGeom &g) { return (g.P + LENETTI_NT - 1) / LENETTI_NT; }
inline int lenetti_T(const LeNettiGeom &g) { return lenetti_ppt(g) <= 4 ? 4 : 2; }
// MILE_RUN_GRAD: grid (S row ranges, E chains) -> slabs / llpart; _LOGLIK / _RAW: grid (S row blocks, E samples) -> out
hipError_t mile_launch_lenetti(const LeNettiParams &lp, int E, MileRun run, hipStream_t st);

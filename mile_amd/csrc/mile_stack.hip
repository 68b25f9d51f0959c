// Stacking kernels (mile_stack.h) in a translation unit of their own: they compile concurrently with mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_stack.h"

__global__ __launch_bounds__(STK_NT) void k_stk_rows(const StkParams p) {
  const long long n = (long long)blockIdx.x * STK_NT + threadIdx.x;
  if (n >= p.Nt) return;
  const int C = p.C;
  const size_t N = (size_t)p.N, gn = (size_t)(p.r0 + n), ld = (size_t)p.ldR;
  const double *l = p.lpd + gn;
  double *rx = p.want_sums ? p.Rx + n : nullptr;
  double m = -INFINITY;
  bool bad = false;
  for (int c = 0; c < C; ++c) {
    const double v = l[(size_t)c * N];
    bad |= (v != v) || v == INFINITY;
    m = fmax(m, v);
  }
  if (bad || !(m > -INFINITY)) {     // left out: NaN in row_score, nothing in any sum
    if (p.row_score) p.row_score[gn] = __longlong_as_double(0x7ff8000000000000LL);
    if (rx)
      for (int c = 0; c < p.Cx; ++c) rx[(size_t)c * ld] = 0.0;
    return;
  }
  double mix = 0.0;
  for (int c = 0; c < C; ++c) {      // chain order
    const double e = exp(l[(size_t)c * N] - m);
    mix = fma(p.w[c], e, mix);
    if (rx) rx[(size_t)c * ld] = e;
  }
  const double rs = m + log(mix);
  if (p.row_score) p.row_score[gn] = rs;
  if (!rx) return;
  for (int c = 0; c < C; ++c) rx[(size_t)c * ld] = rx[(size_t)c * ld] / mix;
  rx[(size_t)C * ld] = 1.0;
  rx[(size_t)(C + 1) * ld] = rs;
}

// G[a][b] += sum over the block's rows inside the tile of Rx[a][n] Rx[b][n], one fma per row in row order
__global__ __launch_bounds__(STK_NT) void k_stk_gram(const StkParams p, const int b_first) {
  __shared__ double As[STK_K][STK_TILE + 2], Bs[STK_K][STK_TILE + 2];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  int ta = 0;
  while ((ta + 1) * (ta + 2) / 2 <= (int)blockIdx.x) ++ta;
  const int tb = (int)blockIdx.x - ta * (ta + 1) / 2;     // tb <= ta
  const int tC = p.C / STK_TILE, tS = (p.C + 1) / STK_TILE;   // the tiles that hold rows C and C + 1
  if (!p.want_hess) {                // (the same for the whole workgroup)
    const bool sums = (ta == tC || ta == tS) && tb == tC;     // [C][C] and [C+1][C]
    if (!(sums || (p.want_grad && ta == tC))) return;
  }
  const int Cx = p.Cx;
  const long long blk = b_first + (long long)blockIdx.y;
  const long long b_lo = blk * p.B, t_hi = p.r0 + p.Nt;
  const long long n_lo = b_lo > p.r0 ? b_lo : p.r0, n_hi = b_lo + p.B < t_hi ? b_lo + p.B : t_hi;
  if (n_lo >= n_hi) return;
  const int a0 = ta * STK_TILE, b0 = tb * STK_TILE;
  double *pt = p.part + (size_t)blk * Cx * Cx;
  double acc[4][4];
  const bool carry = n_lo > b_lo;    // an earlier tile began this block
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int a = a0 + ty * 4 + i, b = b0 + tx * 4 + j;
      acc[i][j] = (carry && a < Cx && b < Cx) ? pt[(size_t)a * Cx + b] : 0.0;
    }
  const int ci = tid >> 2, kq = (tid & 3) * 4;
  const bool a_in = a0 + ci < Cx, b_in = b0 + ci < Cx;
  const double *ga = p.Rx + (size_t)(a_in ? a0 + ci : 0) * (size_t)p.ldR, *gb = p.Rx + (size_t)(b_in ? b0 + ci : 0) * (size_t)p.ldR;
  for (long long n0 = n_lo; n0 < n_hi; n0 += STK_K) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long n = n0 + kq + q;
      const bool in = n < n_hi;
      As[kq + q][ci] = (in && a_in) ? ga[n - p.r0] : 0.0;
      Bs[kq + q][ci] = (in && b_in) ? gb[n - p.r0] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < STK_K; ++k) {
      double av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { av[i] = As[k][ty * 4 + i]; bv[i] = Bs[k][tx * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int a = a0 + ty * 4 + i, b = b0 + tx * 4 + j;
      if (a < Cx && b < Cx) pt[(size_t)a * Cx + b] = acc[i][j];
    }
}

// entry [a][b] of the blocks' partials, summed in block order
__device__ __forceinline__ double stk_entry(const StkParams &p, int a, int b) {
  const size_t cc = (size_t)p.Cx * p.Cx, at = (size_t)a * p.Cx + b;
  double v = 0.0;
  for (int k = 0; k < p.nb; ++k) v += p.part[(size_t)k * cc + at];
  return v;
}

__global__ __launch_bounds__(STK_NT) void k_stk_final(const StkParams p, const long long base) {
  __shared__ double s_used;
  const int C = p.C;
  if (threadIdx.x == 0) s_used = stk_entry(p, C, C);
  __syncthreads();
  const double used = s_used;
  const long long idx = base + (long long)blockIdx.x * STK_NT + threadIdx.x, cc = (long long)C * C;
  if (idx < cc) {
    const int a = (int)(idx / C), b = (int)(idx % C);
    if (b > a) return;
    const double v = stk_entry(p, a, b) / used;
    p.hess[(size_t)a * C + b] = v;
    p.hess[(size_t)b * C + a] = v;
  } else if (idx < cc + C) {
    const int c = (int)(idx - cc);
    if (p.grad) p.grad[c] = stk_entry(p, C, c) / used;
  } else if (idx == cc + C) {
    if (p.score) p.score[0] = stk_entry(p, C + 1, C) / used;
    if (p.used) p.used[0] = (long long)used;
  }
}

hipError_t mile_launch_stack_tile(const StkParams &p, hipStream_t st) {
  k_stk_rows<<<(unsigned)((p.Nt + STK_NT - 1) / STK_NT), STK_NT, 0, st>>>(p);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !p.want_sums) return e;
  const int T = (p.Cx + STK_TILE - 1) / STK_TILE;
  const long long b_first = p.r0 / p.B, b_last = (p.r0 + p.Nt - 1) / p.B;
  k_stk_gram<<<dim3((unsigned)(T * (T + 1) / 2), (unsigned)(b_last - b_first + 1)), STK_NT, 0, st>>>(p, (int)b_first);
  return hipGetLastError();
}

hipError_t mile_launch_stack_final(const StkParams &p, hipStream_t st) {
  const long long cc = (long long)p.C * p.C, base = p.want_hess ? 0 : cc, n = cc + p.C + 1 - base;
  k_stk_final<<<(unsigned)((n + STK_NT - 1) / STK_NT), STK_NT, 0, st>>>(p, base);
  return hipGetLastError();
}

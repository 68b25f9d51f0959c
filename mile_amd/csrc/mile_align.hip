// Alignment of FCN draws to a reference draw by hidden-unit assignment: the kernel, the launcher and the entry points of
// mile_align.h in a translation unit of their own.  The entry points take no sampler handle: the layout comes from
// mile_canon_layout, the launches go to the current device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>

#include "mile_device.h"
#include "mile_eval_handle.h"
#include "mile_align.h"

#define ALIGN_IDX 0x7fffffffu

// ---- wave helpers --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float align_signed(float v, uint32_t flip) { return __uint_as_float(__float_as_uint(v) ^ (flip & CANON_FLIP)); }

// x of lane `l` (the same l in every lane), in every lane
__device__ __forceinline__ int lane_int(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ double lane_double(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
template <int CTRL>
__device__ __forceinline__ double dpp_min(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const double o = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xF, 0xF, false),
                                    __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xF, 0xF, false));
  return o < v ? o : v;
}
// the smallest v of the wave in every lane (no NaN comes here): a butterfly inside each row of 16 lanes, then the four rows
__device__ __forceinline__ double wave_min(double v) {
  v = dpp_min<0xB1>(v);     // quad_perm [1,0,3,2]
  v = dpp_min<0x4E>(v);     // quad_perm [2,3,0,1]
  v = dpp_min<0x141>(v);    // row_half_mirror
  v = dpp_min<0x140>(v);    // row_mirror: every lane holds its row's minimum
  const double a = lane_double(v, 0), b = lane_double(v, 16), c = lane_double(v, 32), d = lane_double(v, 48);
  const double ab = b < a ? b : a, cd = d < c ? d : c;
  return cd < ab ? cd : ab;
}
// x[c] for a c known only at run time, without indexing the registers
template <int NC, class T>
__device__ __forceinline__ T pick(const T (&x)[NC], int c) {
  T r = x[0];
#pragma unroll
  for (int k = 1; k < NC; ++k) r = c == k ? x[k] : r;
  return r;
}

// ---- k_align_solve: one wave per draw; NC columns per lane ------------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(ALIGN_NT) void k_align_solve(AlignParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char align_smem[];
  const CanonPlan &pl = p.pl;
  const int lane = threadIdx.x, H = pl.H, nh = pl.n_hidden;
  const size_t m = blockIdx.x;
  const float *th = p.theta + m * (size_t)pl.d, *rf = p.ref;
  double *S = (double *)align_smem;
  double *scores = S + (size_t)p.wmax * p.wmax;
  uint32_t *ranks = (uint32_t *)(scores + MILE_MAX_LAYERS);
  const bool sgn = (p.how & MILE_ALIGN_SIGN) != 0;
  const double inf = __builtin_huge_val();
  bool drop = false;

  // the plan's rows into LDS, read back one layer at a time: indexed in the kernel arguments they would all sit in SGPRs at once
  int (*lp)[MILE_MAX_LAYERS] = (int (*)[MILE_MAX_LAYERS])(ranks + (H + 3) / 4 * 4);
  if (lane < MILE_MAX_LAYERS) {
    lp[0][lane] = pl.fin[lane]; lp[1][lane] = pl.fout[lane]; lp[2][lane] = pl.b_off[lane]; lp[3][lane] = pl.w_off[lane]; lp[4][lane] = pl.o[lane];
  }
  __syncthreads();
  const auto plan = [&](int what, int k) { return __builtin_amdgcn_readfirstlane(lp[what][k]); };
  const int w_out = nh < pl.n_layers ? plan(3, nh) : 0, O_out = nh < pl.n_layers ? plan(1, nh) : 0;

  for (int l = 0; l < nh; ++l) {
    const int W = plan(1, l), fin = plan(0, l), o = plan(4, l);
    // ---- similarity: S[i][j] = bias product, then the incoming rows in aligned order and sign, then (last hidden layer) the outgoing row
    {
      const uint32_t *rw = l ? ranks + plan(4, l - 1) : nullptr;
      const int b_off = plan(2, l), w_off = plan(3, l);
      const int O = l == nh - 1 ? O_out : 0;                             // (every offset inside a draw fits an int: d does)
      bool bad = false;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int j = lane + 64 * c, jj = min(j, W - 1);                 // a lane past W computes column W - 1 and stores nothing
        if (64 * c >= W) break;
        const double bj = (double)th[b_off + jj];
        for (int i0 = 0; i0 < W; i0 += ALIGN_IB) {
          double acc[ALIGN_IB];
          int ii[ALIGN_IB];
#pragma unroll
          for (int k = 0; k < ALIGN_IB; ++k) {
            ii[k] = min(i0 + k, W - 1);
            acc[k] = (double)rf[b_off + ii[k]] * bj;
          }
          for (int t = 0; t < fin; ++t) {
            const uint32_t r = rw ? rw[t] : (uint32_t)t;
            const double x = (double)align_signed(th[w_off + (int)(r & ALIGN_IDX) * W + jj], r);
            const float *rr = rf + (w_off + t * W);
#pragma unroll
            for (int k = 0; k < ALIGN_IB; ++k) acc[k] = fma((double)rr[ii[k]], x, acc[k]);
          }
          for (int q = 0; q < O; ++q) {
            const double x = (double)th[w_out + jj * O + q];
#pragma unroll
            for (int k = 0; k < ALIGN_IB; ++k) acc[k] = fma((double)rf[w_out + ii[k] * O + q], x, acc[k]);
          }
#pragma unroll
          for (int k = 0; k < ALIGN_IB; ++k)
            if (i0 + k < W && j < W) {
              S[(i0 + k) * W + j] = acc[k];
              bad |= !(fabs(acc[k]) < inf);
            }
        }
      }
      __syncthreads();
      drop = __any(bad) != 0;
    }
    if (drop) break;

    // ---- assignment: rows inserted in ascending i; column j of slot c is lane + 64 c
    double v[NC], ucol[NC];
    int prow[NC];                                                        // the row assigned to the column, -1 while it is free
#pragma unroll
    for (int c = 0; c < NC; ++c) { v[c] = 0.0; ucol[c] = 0.0; prow[c] = -1; }
    for (int i = 0; i < W; ++i) {
      double minv[NC];
      int way[NC];
      bool used[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) { minv[c] = inf; way[c] = -1; used[c] = lane + 64 * c >= W; }   // no column past W is ever chosen
      double ui = 0.0;                                                   // u of row i, the row of the virtual column -1
      int j0 = -1;
      for (;;) {
        int i0 = i;
        double u0 = ui;
        if (j0 >= 0) {
          const int c0 = j0 >> 6, l0 = j0 & 63;
          i0 = lane_int(pick<NC>(prow, c0), l0);
          u0 = lane_double(pick<NC>(ucol, c0), l0);
#pragma unroll
          for (int c = 0; c < NC; ++c) used[c] |= c == c0 && lane == l0;
        }
        const double *row = S + i0 * W;
        double loc = inf;
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (!used[c]) {
            const double s = row[lane + 64 * c];
            const double cur = ((sgn ? -fabs(s) : -s) - u0) - v[c];
            if (cur < minv[c]) { minv[c] = cur; way[c] = j0; }
            loc = minv[c] < loc ? minv[c] : loc;
          }
        const double delta = wave_min(loc);
        int j1 = -1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const unsigned long long b = __ballot(!used[c] && minv[c] == delta);
          if (j1 < 0 && b) j1 = 64 * c + __ffsll(b) - 1;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (!used[c]) minv[c] -= delta;
          else if (lane + 64 * c < W) { ucol[c] += delta; v[c] -= delta; }
        }
        ui += delta;
        j0 = j1;
        if (j1 < 0) { drop = true; break; }                              // (no free column holds the minimum: cannot happen on finite S)
        if (lane_int(pick<NC>(prow, j0 >> 6), j0 & 63) < 0) break;
      }
      if (drop) break;
      while (j0 >= 0) {                                                  // flip the path back to the virtual column
        const int c0 = j0 >> 6, l0 = j0 & 63;
        const int j1 = lane_int(pick<NC>(way, c0), l0);
        int pr = i;
        double ur = ui;
        if (j1 >= 0) {
          pr = lane_int(pick<NC>(prow, j1 >> 6), j1 & 63);
          ur = lane_double(pick<NC>(ucol, j1 >> 6), j1 & 63);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c == c0 && lane == l0) { prow[c] = pr; ucol[c] = ur; }
        j0 = j1;
      }
    }

    if (drop) break;
    // ---- rank words of the layer, then its score in ascending i
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = lane + 64 * c;
      if (j < W) ranks[o + prow[c]] = (uint32_t)j | ((sgn && S[prow[c] * W + j] < 0.0) ? CANON_FLIP : 0u);
    }
    __syncthreads();
    double sc = 0.0;
    for (int i = 0; i < W; ++i) {
      const double s = S[i * W + (int)(ranks[o + i] & ALIGN_IDX)];
      sc += sgn ? fabs(s) : s;
    }
    if (lane == 0) scores[l] = sc;
    __syncthreads();
  }

  // ---- the draw's outputs: what was found, or for a dropped draw the identity
  for (int l = 0; l < nh; ++l) {
    const int o = plan(4, l), W = plan(1, l);
    for (int j = lane; j < W; j += ALIGN_NT) {
      const uint32_t w = drop ? (uint32_t)j : ranks[o + j];
      p.ranks[m * H + o + j] = w;
      if (p.perm) p.perm[m * H + o + j] = (int32_t)(w & ALIGN_IDX);
      if (p.sign) p.sign[m * H + o + j] = (w & CANON_FLIP) ? (int8_t)-1 : (int8_t)1;
    }
    if (p.score && lane == 0) p.score[m * nh + l] = drop ? __builtin_nan("") : scores[l];
  }
  if (p.dropped && lane == 0) p.dropped[m] = drop ? 1 : 0;
}

hipError_t mile_launch_align(const AlignParams &p, float *out, hipStream_t st) {
  const unsigned M = (unsigned)p.M;
  const size_t lds = align_lds(p);
  if (p.wmax <= 64) {
    const hipError_t e = mile_set_max_lds<k_align_solve<1>>(ALIGN_LDS_MAX);
    if (e != hipSuccess) return e;
    k_align_solve<1><<<M, ALIGN_NT, lds, st>>>(p);
  } else {
    const hipError_t e = mile_set_max_lds<k_align_solve<2>>(ALIGN_LDS_MAX);
    if (e != hipSuccess) return e;
    k_align_solve<2><<<M, ALIGN_NT, lds, st>>>(p);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  CanonParams c{};
  c.pl = p.pl; c.theta = p.theta; c.M = p.M; c.out = out; c.ranks = p.ranks;
  return mile_launch_canon_rows(c, st);
}

// ---- the entry points: every check before any launch, none of them touches a device ------------------------------------------------
// The parameters of `spec` under `how` (pl, how, wmax), or why there are none.
static const char *align_plan(const mile_model_spec *spec, uint32_t how, AlignParams &p) {
  if (const char *m = mile_canon_shape(spec)) return m;
  if (how & ~MILE_ALIGN_SIGN) return "unknown bits in `how`";
  if ((how & MILE_ALIGN_SIGN) && spec->activation != MILE_ACT_TANH) return "MILE_ALIGN_SIGN needs an odd activation: tanh only";
  p.wmax = 0;
  for (int l = 0; l + 1 < spec->n_layers; ++l) {
    if (spec->widths[l] > MILE_ALIGN_WIDTH_MAX) return "unsupported: a hidden width above MILE_ALIGN_WIDTH_MAX (128)";
    p.wmax = std::max(p.wmax, (int)spec->widths[l]);
  }
  p.how = how;
  return mile_canon_layout(spec, p.pl);
}
static int align_bad(const char *fn, const char *m) { return fail(MILE_ERR_INVALID, std::string(fn) + ": " + m); }
static bool overlaps(uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a < b + nb && b < a + na; }

extern "C" int64_t mile_align_fcn_workspace(const mile_model_spec *spec, int64_t M, uint32_t how) {
  AlignParams p{};
  if (const char *m = align_plan(spec, how, p)) { align_bad("mile_align_fcn_workspace", m); return -1; }
  if (M < 1 || M > 0x7fffffffLL) { align_bad("mile_align_fcn_workspace", "M out of range (1 .. 2^31 - 1)"); return -1; }
  return M * p.pl.H * 4;
}

extern "C" int32_t mile_align_fcn(const mile_model_spec *spec, const float *theta, int64_t M, const float *reference, uint32_t how,
                                  float *out, int32_t *perm, int8_t *sign, double *score, int32_t *dropped, void *workspace,
                                  int64_t workspace_bytes, void *stream) {
  const char *fn = "mile_align_fcn";
  if (!spec || !theta || !reference || !out) return align_bad(fn, "null spec, theta, reference or out");
  if (M < 1 || M > 0x7fffffffLL) return align_bad(fn, "M out of range (1 .. 2^31 - 1)");
  AlignParams p{};
  if (const char *m = align_plan(spec, how, p)) return align_bad(fn, m);
  const uintptr_t row = (uintptr_t)p.pl.d * 4, bytes = (uintptr_t)M * row;
  if (overlaps((uintptr_t)theta, bytes, (uintptr_t)out, bytes)) return align_bad(fn, "out overlaps theta");
  if (overlaps((uintptr_t)reference, row, (uintptr_t)out, bytes)) return align_bad(fn, "out overlaps reference");
  if (p.pl.H > 0 && (!workspace || workspace_bytes < M * p.pl.H * 4)) return fail(MILE_ERR_STATE, std::string(fn) + ": workspace too small");
  p.theta = theta; p.ref = reference; p.M = M; p.ranks = (uint32_t *)workspace;
  p.perm = perm; p.sign = sign; p.score = score; p.dropped = dropped;
  HIP_TRY(mile_launch_align(p, out, (hipStream_t)stream));
  return MILE_OK;
}

// Canonical hidden-unit ordering of FCN draws: the kernels, the launcher and the entry points of mile_canon.h in a translation
// unit of their own.  The entry points take no sampler handle: the layout comes from fcn_param_layout, the launches go to the
// current device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "mile_device.h"
#include "mile_eval_handle.h"
#include "mile_canon.h"

#define CANON_IDX 0x7fffffffu

// ---- the rule on one unit ---------------------------------------------------------------------------------------------------------
// hidden layer of H index h (at most 15 spans: a short scan)
__device__ __forceinline__ int canon_layer_of(const CanonPlan &pl, int h) {
  int l = 0;
  while (h >= pl.o[l + 1]) ++l;
  return l;
}
__device__ __forceinline__ bool canon_flip(unsigned how, float bias) { return (how & MILE_CANON_SIGN) && bias < 0.0f; }

// key of unit j of hidden layer l of the draw at th (LDS or global): the bias key is the fp64 of the fp32 number, which
// compares as it does; the norm key adds its terms one after another, bias first, then i ascending
__device__ __forceinline__ double canon_key(const CanonPlan &pl, const float *th, int l, int j, unsigned how) {
  const float b = th[pl.b_off[l] + j];
  if (!(how & MILE_CANON_KEY_NORM)) return canon_flip(how, b) ? -(double)b : (double)b;
  double k = (double)b * (double)b;
  const int W = pl.fout[l], fin = pl.fin[l];
  const float *w = th + pl.w_off[l] + j;
  for (int i = 0; i < fin; ++i) {
    const double x = (double)w[(size_t)i * W];
    k += x * x;
  }
  return k;
}

// position of unit j among keys[0, W): the units with a smaller key, and those with an equal key and a smaller index.  A NaN
// is larger than every number and equal to every NaN.  Every lane reads the same keys[k]: a broadcast.
__device__ __forceinline__ int canon_rank(const double *keys, int W, int j) {
  const double kj = keys[j];
  const bool nj = kj != kj;
  int r = 0;
  for (int k = 0; k < W; ++k) {
    const double kk = keys[k];
    const bool nk = kk != kk;
    const bool less = nj ? !nk : kk < kj, eq = nj ? nk : kk == kj;
    r += (less || (eq && k < j)) ? 1 : 0;
  }
  return r;
}

// keys of every hidden unit of the draw at th into keys [H] (LDS), then, past a barrier, the rank words into ranks [H] (LDS or
// global): ranks[o_l + position] = original index | CANON_FLIP when the unit's sign is flipped.  Ends with a barrier.
__device__ __forceinline__ void canon_rank_draw(const CanonPlan &pl, const float *th, unsigned how, double *keys, uint32_t *ranks,
                                                int tid, int nt) {
  for (int h = tid; h < pl.H; h += nt) {
    const int l = canon_layer_of(pl, h);
    keys[h] = canon_key(pl, th, l, h - pl.o[l], how);
  }
  __syncthreads();
  for (int h = tid; h < pl.H; h += nt) {
    const int l = canon_layer_of(pl, h), o = pl.o[l], j = h - o;
    const int r = canon_rank(keys + o, pl.fout[l], j);
    ranks[o + r] = (uint32_t)j | (canon_flip(how, th[pl.b_off[l] + j]) ? CANON_FLIP : 0u);
  }
  __syncthreads();
}

// perm and sign of draw m from its rank words (either may be null)
__device__ __forceinline__ void canon_write_index(const CanonParams &p, const uint32_t *ranks, size_t m, int tid, int nt) {
  const int H = p.pl.H;
  for (int h = tid; h < H; h += nt) {
    const uint32_t w = ranks[h];
    if (p.perm) p.perm[m * H + h] = (int32_t)(w & CANON_IDX);
    if (p.sign) p.sign[m * H + h] = (w & CANON_FLIP) ? (int8_t)-1 : (int8_t)1;
  }
}

__device__ __forceinline__ float canon_signed(float v, uint32_t flip) { return __uint_as_float(__float_as_uint(v) ^ (flip & CANON_FLIP)); }

// ---- k_canon_draw: one workgroup per draw, the draw in LDS --------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(NT) void k_canon_draw(CanonParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char canon_smem[];
  const CanonPlan &pl = p.pl;
  const int tid = threadIdx.x, d = pl.d, H = pl.H;
  const size_t m = blockIdx.x, base = m * (size_t)d;
  const float *src = p.theta + base;
  const int a = (int)(((uintptr_t)src >> 2) & 3);               // floats past a 16-byte boundary: LDS keeps the same phase
  float *th = (float *)canon_smem + a;
  double *keys = (double *)(canon_smem + ((size_t)d + 6) / 4 * 16);
  uint32_t *ranks = (uint32_t *)(keys + H);

  const int head = min(d, (4 - a) & 3), n4 = (d - head) >> 2, tail0 = head + 4 * n4;
  if (tid < head) th[tid] = src[tid];
  const float4 *s4 = (const float4 *)(src + head);
  float4 *d4 = (float4 *)(th + head);
  for (int i = tid; i < n4; i += NT) d4[i] = s4[i];
  if (tid < d - tail0) th[tail0 + tid] = src[tail0 + tid];
  __syncthreads();

  canon_rank_draw(pl, th, p.how, keys, ranks, tid, NT);
  canon_write_index(p, ranks, m, tid, NT);

  float *out = p.out + base;
  for (int li = 0; li < pl.n_layers; ++li) {
    const int fin = pl.fin[li], fout = pl.fout[li], n = fin * fout;
    const uint32_t *rw = li > 0 ? ranks + pl.o[li - 1] : nullptr;           // the rows follow the layer below
    const uint32_t *cw = li < pl.n_hidden ? ranks + pl.o[li] : nullptr;     // the columns this layer's own units
    const float *B = th + pl.b_off[li], *K = th + pl.w_off[li];
    float *oB = out + pl.b_off[li], *oK = out + pl.w_off[li];
    for (int j = tid; j < fout; j += NT) {
      const uint32_t c = cw ? cw[j] : (uint32_t)j;
      oB[j] = canon_signed(B[c & CANON_IDX], c);
    }
    // (i, j) of flat index idx = tid, tid + NT, ..: stepped, not divided
    const int di = NT / fout, dj = NT - di * fout;
    int i = tid / fout, j = tid - i * fout;
    for (int idx = tid; idx < n; idx += NT) {
      const uint32_t r = rw ? rw[i] : (uint32_t)i, c = cw ? cw[j] : (uint32_t)j;
      oK[idx] = canon_signed(K[(r & CANON_IDX) * fout + (c & CANON_IDX)], r ^ c);
      j += dj; i += di;
      if (j >= fout) { j -= fout; ++i; }
    }
  }
}

// ---- the tiled form: k_canon_rank, one workgroup per draw ---------------------------------------------------------------------------
__global__ __launch_bounds__(CANON_NT) void k_canon_rank(CanonParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char canon_smem[];
  const size_t m = blockIdx.x;
  uint32_t *ranks = p.ranks + m * p.pl.H;
  canon_rank_draw(p.pl, p.theta + m * (size_t)p.pl.d, p.how, (double *)canon_smem, ranks, threadIdx.x, CANON_NT);
  canon_write_index(p, ranks, m, threadIdx.x, CANON_NT);      // (the barrier above orders the workgroup's own global writes)
}

// ---- k_canon_rows: grid (M, row tiles, layers); a wave takes one output row at a time ------------------------------------------------
// Row 0 of a layer is its bias, row 1 + i' its kernel row i'.  The source row is one contiguous run: read side by side into the
// wave's LDS row, written back with the columns permuted.  A layer whose columns stay (the output layer) is copied row by row.
__global__ __launch_bounds__(CANON_NT) void k_canon_rows(CanonParams p) {
  __shared__ float rowbuf[CANON_NT / 64][MILE_CANON_WIDTH_MAX];
  const CanonPlan &pl = p.pl;
  const int li = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const size_t m = blockIdx.x, base = m * (size_t)pl.d;
  const int fin = pl.fin[li], fout = pl.fout[li];
  const uint32_t *ranks = p.ranks + m * pl.H;
  const uint32_t *rw = li > 0 ? ranks + pl.o[li - 1] : nullptr, *cw = li < pl.n_hidden ? ranks + pl.o[li] : nullptr;
  const float *th = p.theta + base;
  float *out = p.out + base;
  // the trip counts are the workgroup's, not the wave's: the barriers inside are reached by every wave
  for (int r0 = blockIdx.y * CANON_TILE_ROWS; r0 <= fin; r0 += gridDim.y * CANON_TILE_ROWS)
    for (int k = 0; k < CANON_TILE_ROWS; k += CANON_NT / 64) {
      const int row = r0 + k + wave;
      const bool live = row <= fin;
      uint32_t r = 0;
      const float *srow = th + pl.b_off[li];
      float *orow = out + pl.b_off[li];
      if (live && row > 0) {
        r = rw ? rw[row - 1] : (uint32_t)(row - 1);
        srow = th + pl.w_off[li] + (size_t)(r & CANON_IDX) * fout;
        orow = out + pl.w_off[li] + (size_t)(row - 1) * fout;
      }
      if (!cw) {
        if (live) for (int j = lane; j < fout; j += 64) orow[j] = canon_signed(srow[j], r);
        continue;                                                // (cw is the workgroup's: no wave reaches the barriers)
      }
      if (live) for (int j = lane; j < fout; j += 64) rowbuf[wave][j] = srow[j];
      __syncthreads();
      if (live)
        for (int j = lane; j < fout; j += 64) {
          const uint32_t c = cw[j];
          orow[j] = canon_signed(rowbuf[wave][c & CANON_IDX], r ^ c);
        }
      __syncthreads();
    }
}

hipError_t mile_launch_canon(const CanonParams &p, hipStream_t st) {
  const unsigned M = (unsigned)p.M;
  if (canon_fits(p.pl)) {
    const bool big = p.pl.d >= CANON_BIG_D;
    const hipError_t e = big ? mile_set_max_lds<k_canon_draw<CANON_NT_BIG>>(CANON_LDS_MAX) : mile_set_max_lds<k_canon_draw<CANON_NT>>(CANON_LDS_MAX);
    if (e != hipSuccess) return e;
    if (big) k_canon_draw<CANON_NT_BIG><<<M, CANON_NT_BIG, canon_draw_lds(p.pl), st>>>(p);
    else k_canon_draw<CANON_NT><<<M, CANON_NT, canon_draw_lds(p.pl), st>>>(p);
    return hipGetLastError();
  }
  const hipError_t e = mile_set_max_lds<k_canon_rank>(CANON_LDS_MAX);
  if (e != hipSuccess) return e;
  k_canon_rank<<<M, CANON_NT, canon_rank_lds(p.pl), st>>>(p);
  return mile_launch_canon_rows(p, st);
}

// The write phase alone: out from theta and the rank words p.ranks [M][H], whoever made them (p.how, p.perm, p.sign are not read).
hipError_t mile_launch_canon_rows(const CanonParams &p, hipStream_t st) {
  const int tiles = (p.pl.max_rows + CANON_TILE_ROWS - 1) / CANON_TILE_ROWS;
  k_canon_rows<<<dim3((unsigned)p.M, (unsigned)std::min(tiles, 65535), (unsigned)p.pl.n_layers), CANON_NT, 0, st>>>(p);
  return hipGetLastError();
}

// ---- the entry points: every check before any launch, none of them touches a device ------------------------------------------------
// The shape of `spec` as an FCN whose hidden units can be moved, or why it is none.
const char *mile_canon_shape(const mile_model_spec *spec) {
  if (!spec) return "null spec";
  if (spec->model != MILE_MODEL_FCN) return "only MILE_MODEL_FCN has a canonical form here";
  if (spec->use_bias != 1) return "use_bias must be 1";
  if (spec->n_layers < 1 || spec->n_layers > MILE_MAX_LAYERS) return "n_layers out of range";
  if (spec->in_features < 1) return "in_features must be >= 1";
  for (int l = 0; l < spec->n_layers; ++l)
    if (spec->widths[l] < 1) return "layer width must be >= 1";
  return nullptr;
}

// The plan of `spec` under `how`, or why there is none.
static const char *canon_plan(const mile_model_spec *spec, uint32_t how, CanonPlan &pl) {
  if (const char *m = mile_canon_shape(spec)) return m;
  if (how & ~(MILE_CANON_KEY_NORM | MILE_CANON_SIGN)) return "unknown bits in `how`";
  if ((how & MILE_CANON_SIGN) && spec->activation != MILE_ACT_TANH) return "MILE_CANON_SIGN needs an odd activation: tanh only";
  for (int l = 0; l + 1 < spec->n_layers; ++l)
    if (spec->widths[l] > MILE_CANON_WIDTH_MAX) return "unsupported: a hidden width above MILE_CANON_WIDTH_MAX (1024)";
  return mile_canon_layout(spec, pl);
}

// The layout of a spec that passed mile_canon_shape: offsets, fans and the hidden spans of the H axis.
const char *mile_canon_layout(const mile_model_spec *spec, CanonPlan &pl) {
  pl = CanonPlan{};
  const long long d = fcn_param_layout(spec, FcnOffsets{pl.b_off, pl.w_off});
  if (d > 0x7fffffffLL) return "parameter count exceeds int32";
  pl.n_layers = spec->n_layers; pl.n_hidden = spec->n_layers - 1; pl.d = (int)d;
  for (int l = 0; l < spec->n_layers; ++l) {
    pl.fin[l] = l ? spec->widths[l - 1] : spec->in_features;
    pl.fout[l] = spec->widths[l];
    pl.max_rows = std::max(pl.max_rows, pl.fin[l] + 1);
    if (l < pl.n_hidden) { pl.o[l] = pl.H; pl.H += spec->widths[l]; }
  }
  pl.o[pl.n_hidden] = pl.H;
  return nullptr;
}
static int canon_bad(const char *fn, const char *m) { return fail(MILE_ERR_INVALID, std::string(fn) + ": " + m); }

extern "C" int64_t mile_canonical_hidden(const mile_model_spec *spec) {
  CanonPlan pl;
  if (const char *m = canon_plan(spec, 0, pl)) { canon_bad("mile_canonical_hidden", m); return -1; }
  return pl.H;
}

extern "C" int64_t mile_canonicalize_fcn_workspace(const mile_model_spec *spec, int64_t M, uint32_t how) {
  CanonPlan pl;
  if (const char *m = canon_plan(spec, how, pl)) { canon_bad("mile_canonicalize_fcn_workspace", m); return -1; }
  if (M < 1 || M > 0x7fffffffLL) { canon_bad("mile_canonicalize_fcn_workspace", "M out of range (1 .. 2^31 - 1)"); return -1; }
  return canon_fits(pl) ? 0 : M * pl.H * 4;
}

extern "C" int32_t mile_canonicalize_fcn(const mile_model_spec *spec, const float *theta, int64_t M, uint32_t how, float *out,
                                         int32_t *perm, int8_t *sign, void *workspace, int64_t workspace_bytes, void *stream) {
  const char *fn = "mile_canonicalize_fcn";
  if (!spec || !theta || !out) return canon_bad(fn, "null spec, theta or out");
  if (M < 1 || M > 0x7fffffffLL) return canon_bad(fn, "M out of range (1 .. 2^31 - 1)");
  CanonParams p{};
  if (const char *m = canon_plan(spec, how, p.pl)) return canon_bad(fn, m);
  const uintptr_t t0 = (uintptr_t)theta, o0 = (uintptr_t)out, bytes = (uintptr_t)M * (uintptr_t)p.pl.d * 4;
  if (t0 < o0 + bytes && o0 < t0 + bytes) return canon_bad(fn, "out overlaps theta");
  const bool tiled = !canon_fits(p.pl);
  if (tiled && p.pl.H > 0 && (!workspace || workspace_bytes < M * p.pl.H * 4)) return fail(MILE_ERR_STATE, std::string(fn) + ": workspace too small");
  p.theta = theta; p.M = M; p.how = how; p.out = out; p.perm = perm; p.sign = sign;
  p.ranks = tiled ? (uint32_t *)workspace : nullptr;
  HIP_TRY(mile_launch_canon(p, (hipStream_t)stream));
  return MILE_OK;
}

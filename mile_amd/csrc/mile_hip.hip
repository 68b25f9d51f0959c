// libmile_hip.so -- host side of the C ABI declared in include/mile_hip.h.
// gfx950 (MI355X) only.  No torch types: plain pointers, sizes and a hipStream_t.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "mile_device.h"
#include "mile_grad_generic.h"
#include "mile_grad_narrow.h"
#include "mile_grad_w64.h"
#include "mile_grad_w128b.h"
#include "mile_grad_gemm.h"
#include "mile_mm3.h"
#include "mile_lenet.h"
#include "mile_lenet_mfma.h"
#include "mile_lenetti.h"
#include "mile_attn.h"
#include "mile_attn_pre.h"
#include "mile_attn_wide.h"
#include "mile_predict.h"
#include "mile_update.h"
#include "mile_nuts.h"
#include "mile_eval_handle.h"
#include "mile_eval_plan.h"
#include "mile_layer_plan.h"

static thread_local std::string g_err;
int fail(int code, const std::string &msg) { g_err = msg; return code; }

// Grow the device buffer p of `cap` elements to `need` of `unit` bytes each (contents are not kept).  On failure p is null, cap
// is 0 and the sticky HIP error is cleared.
template <class P, class N>
static hipError_t grow(P *&p, N &cap, size_t need, size_t unit) {
  if (need <= (size_t)cap) return hipSuccess;
  if (p) (void)hipFree(p);
  p = nullptr; cap = 0;
  const hipError_t e = hipMalloc(&p, need * unit);
  if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return e; }
  cap = (N)need;
  return hipSuccess;
}

static const double MCLACHLAN_B1 = 0.1931833275037836;

struct PartSegs { int n; int begin[4], len[4]; };   // sampled segments of the full row (mile_partition_segments)

struct mile_sampler {
  mile_model_spec spec{};
  DevSpec ds{};
  int device = 0;
  int n_cu = 256;
  // data
  float *X = nullptr, *Xp = nullptr;
  void *Xb = nullptr, *Xt = nullptr;   // bf16 copies for k_grad_w128b
  void *y = nullptr;
  int N = 0, Npad = 0, Fp = 0, Npb = 0;
  int win_begin = 0, win_count = 0;     // mile_set_row_window: rows [begin, begin + count) only (count 0 = all)
  // workspace
  int E_cap = 0;
  size_t ES_cap = 0;   // slab rows (particles x row splits) the workspace holds: fewer particles may split the rows further
  float *slabs = nullptr, *llpart = nullptr, *dK = nullptr, *lold = nullptr;
  float *upart = nullptr;               // segmented update (d beyond the one-workgroup forms): partial sums per segment
  int32_t *arrive = nullptr;            // [E_cap] arrival tickets of the fused integrator epilogue (k_grad_w64 SPLIT)
  float *nzbuf = nullptr;               // [2][nz_E][d] O-step noise a mid-step update launch prefills for the record launch
  int nz_E = 0;                         // particle rows nzbuf holds (allocated by the first mile_step that prefills)
  int64_t nz_launches = 0;              // mid-step launches that prefilled noise (mile_debug_prefill_count)
  void *ev_rows = nullptr; size_t ev_rows_bytes = 0;   // evaluation (test) set staging: X, its padded copy and y (stage_rows)
  PredParams ev_set{};                  // the one staged set, as stage_rows left it: what eval_forward runs on
  // the streamed evaluation calls' one workspace (reserve_eval_ws): a pass's or a tile's forward outputs first, then the call's
  // own state at the offsets of its plan (qnt_ / loo_ / crps_ / cal_tile_plan; moments and LPPD lay theirs out in place)
  void *eval_ws = nullptr; size_t eval_ws_bytes = 0;
  const int32_t *qnt_sweeps = nullptr; int64_t qnt_rows = 0;   // sweeps per row of the last mile_predict_quantiles, in eval_ws
  float *alt_x = nullptr, *alt_u = nullptr, *alt_g = nullptr, *alt_logp = nullptr;   // ping-pong state of mile_tune
  int grad_kernel = MILE_GRAD_AUTO;
  LeNetGeom lg{};                       // MILE_MODEL_LENET geometry and parameter offsets
  LeNettiGeom ng{};                     // MILE_MODEL_LENETTI geometry and parameter offsets
  AttnGeom ag{};                        // MILE_MODEL_ATTN / ATTN_PRETRAINED / ATTN_WIDE geometry and parameter offsets
  float *emb_tab = nullptr, *pos_tab = nullptr;   // ATTN_PRETRAINED: frozen tables [V, C], [T, C] (mile_set_embedding)
  struct ParamLayer { int bias_off, kernel_off; };
  std::vector<ParamLayer> layers;       // mile_param_offsets, in ABI order (bias -1: none)
  // layer-wise GEMM path (MILE_GRAD_GEMM_F32): rocBLAS handle and activation workspace
  void *blas = nullptr;
  float *tune_info = nullptr;           // [E_cap, 3] scratch MCLMCInfo of mile_tune's large-d path
  float *gemm_ws = nullptr, *gemm_ones = nullptr;
  int gemm_ones_n = 0;
  size_t gemm_ws_floats = 0;
  int gemm_R = 0, gemm_E = 0;
  // layer-wise MFMA path (MILE_GRAD_MFMA_WIDE_*): activation workspace (zero-initialised: padding columns stay 0) and
  // the pre-split weight term planes
  float *wide_ws = nullptr; size_t wide_ws_floats = 0; int wide_R = 0, wide_E = 0;
  void *wide_wt = nullptr; size_t wide_wt_bytes = 0;
  float *wide_hb = nullptr; size_t wide_hb_floats = 0;   // k_wide_headblock's per-workgroup partial sums
  // NUTS trajectory buffers (mile_nuts_reserve)
  NutsBufs nb{};
  int nuts_E = 0, nuts_M = 0;
  int32_t *nuts_count_h = nullptr;      // pinned host copy of nb.count
  // partition sampling (mile_set_partition): the first and the last layer are sampled, the others stay at part_rows' values
  bool part = false;
  int part_E = 0, part_d = 0;           // chains of part_rows; d_s = sampled coordinates per chain
  float *part_rows = nullptr;           // [part_E][d] full-layout rows: frozen layers, and what the general path scatters into
  float *part_slabs = nullptr;          // [ES_cap][part_d rounded up] compact slabs: what the update kernels read
  PartSegs part_seg{};                  // the sampled segments of the full row, in full-row order
  int part_b0 = 0, part_w0 = 0, part_bl = 0, part_wl = 0;   // first / last layer's bias and kernel inside the compact row
  // timing of grad launches
  bool timing = false;
  std::vector<hipEvent_t> ev;
  size_t ev_used = 0;
};

// ---- which specs each grad kernel runs: the `supports` of its row in kGrad ------------------------------------------------
static bool is_fcn(const mile_sampler *s) { return s->spec.model == MILE_MODEL_FCN; }
static bool is_lenet(const mile_sampler *s) { return s->spec.model == MILE_MODEL_LENET; }
static bool is_lenetti(const mile_sampler *s) { return s->spec.model == MILE_MODEL_LENETTI; }
static bool is_attn(const mile_sampler *s) { return s->spec.model == MILE_MODEL_ATTN; }
static bool is_attn_pre(const mile_sampler *s) { return s->spec.model == MILE_MODEL_ATTN_PRETRAINED; }
static bool is_attn_wide(const mile_sampler *s) { return s->spec.model == MILE_MODEL_ATTN_WIDE; }
// every call that evaluates the likelihood refuses a pretrained-attention sampler whose tables are not set
bool tables_missing(const mile_sampler *s) { return is_attn_pre(s) && !s->emb_tab; }
const char *const kNoTables = "PretrainedAttentionClassifier: call mile_set_embedding first";
static bool lenet_bf16_supported(const mile_sampler *s) { return is_lenet(s) && s->lg.C <= 4; }   // LENET_BF16 and LENET_BF16X3

// k_grad_w64 / k_grad_w128b: ReLU regression, 1-3 hidden layers of the kernel's width, F <= 16
static bool relu_regression_of_width(const mile_sampler *s, int width) {
  const mile_model_spec &sp = s->spec;
  if (sp.model != MILE_MODEL_FCN) return false;
  if (sp.task != MILE_TASK_REGRESSION || sp.activation != MILE_ACT_RELU) return false;
  const int nh = sp.n_layers - 1;
  if (nh < 1 || nh > 3) return false;
  for (int l = 0; l < nh; ++l)
    if (sp.widths[l] != width) return false;
  if (sp.widths[nh] != 2) return false;
  if (sp.in_features > 16) return false;
  return true;
}
static bool w64_supported(const mile_sampler *s) { return relu_regression_of_width(s, 64); }
static bool w128b_supported(const mile_sampler *s) { return relu_regression_of_width(s, 128); }
// the split-bf16 variant replaces the hidden->hidden products, so it needs at least one
static bool w64x3_supported(const mile_sampler *s) { return w64_supported(s) && s->spec.n_layers - 1 >= 2; }

// k_grad_narrow: 1-3 hidden layers of width <= 64 and F <= 64 (<= 32: weights in registers; 33..64: weights in LDS), or 4-10
// hidden layers of width <= 16 and F <= 16 (the depth ablations of the reference: experiments/**: [16]*4 .. [16]*9 + [2],
// [8]*6 + [2]); <= 16 outputs (regression: exactly mu, log sigma), any activation
static int narrow_tiles_hidden(const mile_model_spec &sp) {
  int mw = 0;
  for (int l = 0; l + 1 < sp.n_layers; ++l) mw = std::max(mw, sp.widths[l]);
  return (mw + 15) / 16;
}
static bool narrow_supported(const mile_sampler *s) {
  const mile_model_spec &sp = s->spec;
  if (sp.model != MILE_MODEL_FCN || !sp.use_bias) return false;
  const int nh = sp.n_layers - 1;
  if (nh < 1 || nh > 10 || sp.in_features > 64) return false;
  for (int l = 0; l < nh; ++l)
    if (sp.widths[l] < 1 || sp.widths[l] > (nh > 3 ? 16 : 64)) return false;
  if (nh > 3 && sp.in_features > 16) return false;
  const int K = sp.widths[nh];
  if (K < 1 || K > 16) return false;
  if (sp.task == MILE_TASK_REGRESSION && K != 2) return false;
  return true;
}

// ---- rocBLAS, resolved at first use: libmile_hip.so has no link-time dependency on it -----------
typedef int (*rb_create_t)(void **);
typedef int (*rb_destroy_t)(void *);
typedef int (*rb_set_stream_t)(void *, hipStream_t);
typedef int (*rb_sgemm_sb_t)(void *, int, int, int, int, int, const float *, const float *, int, long long, const float *, int,
                             long long, const float *, float *, int, long long, int);
static struct {
  void *lib = nullptr;
  rb_create_t create = nullptr;
  rb_destroy_t destroy = nullptr;
  rb_set_stream_t set_stream = nullptr;
  rb_sgemm_sb_t sgemm_sb = nullptr;
  bool tried = false;
} g_rb;
enum { RB_OP_N = 111, RB_OP_T = 112 };   // rocblas_operation_none / _transpose

static bool rocblas_load() {
  if (g_rb.tried) return g_rb.sgemm_sb != nullptr;
  g_rb.tried = true;
  for (const char *name : {"librocblas.so.5", "librocblas.so", "/opt/rocm/lib/librocblas.so"}) {
    g_rb.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (g_rb.lib) break;
  }
  if (!g_rb.lib) return false;
  g_rb.create = (rb_create_t)dlsym(g_rb.lib, "rocblas_create_handle");
  g_rb.destroy = (rb_destroy_t)dlsym(g_rb.lib, "rocblas_destroy_handle");
  g_rb.set_stream = (rb_set_stream_t)dlsym(g_rb.lib, "rocblas_set_stream");
  g_rb.sgemm_sb = (rb_sgemm_sb_t)dlsym(g_rb.lib, "rocblas_sgemm_strided_batched");
  if (!g_rb.create || !g_rb.destroy || !g_rb.set_stream || !g_rb.sgemm_sb) { g_rb.sgemm_sb = nullptr; return false; }
  return true;
}
// what a launcher needs before its first SGEMM: the library, the sampler's handle, the handle on the launcher's stream
static int rocblas_ready(mile_sampler *s, hipStream_t st) {
  if (!rocblas_load()) return fail(MILE_ERR_HIP, "librocblas.so could not be loaded");
  if (!s->blas && g_rb.create(&s->blas) != 0) { s->blas = nullptr; return fail(MILE_ERR_HIP, "rocblas_create_handle failed"); }
  if (g_rb.set_stream(s->blas, st) != 0) return fail(MILE_ERR_HIP, "rocblas_set_stream failed");
  return MILE_OK;
}
// MILE_GEMM_ROWS (test hook): the rows per chunk of the layer-wise and LeNet paths, 1 .. N, in place of the R their own rule gave
static size_t gemm_rows_hook(size_t R, size_t N) {
  if (const char *rv = getenv("MILE_GEMM_ROWS")) R = std::max<size_t>(1, std::min<size_t>((size_t)atoll(rv), N));
  return R;
}

// library GEMMs pay off once the hidden layers are wide; below that the single-launch generic kernel wins
static bool gemm_preferred(const mile_sampler *s) {
  int mw = 0;
  for (int l = 0; l + 1 < s->spec.n_layers; ++l) mw = std::max(mw, s->spec.widths[l]);
  return is_fcn(s) && s->spec.n_layers >= 2 && mw >= 96;
}

// ---- row ranges (slabs) per particle: the `row_splits` of each row in kGrad ----------------------------------------------
// rows per LDS tile of the generic kernel: fit the activation record in ~56 KiB
static int generic_R(const DevSpec &ds) {
  const int per_row = ds.act_stride + 2 * ds.max_width;
  int R = (56 * 1024 / 4 - 16) / per_row;
  R = std::max(1, std::min(R, 64));
  return R;
}
static int generic_S(const mile_sampler *s, int E) {
  int S = std::max(1, (2 * s->n_cu) / std::max(E, 1));
  S = std::min(S, std::max(1, s->N / 64));
  return std::min(S, 64);
}
static int w64_S(const mile_sampler *s, int E) {
  const int NB = s->Npad / 32;
  int S = std::max(1, s->n_cu / std::max(E, 1));
  S = std::min(S, std::max(1, NB / 4));  // keep >= 4 row blocks (one per wave) per workgroup
  return S;
}
static int w128b_S(const mile_sampler *s, int E) {
  const int NBS = s->Npb / 64;              // iterations of two 32-row tiles
  int S = std::max(1, s->n_cu / std::max(E, 1));
  return std::min(S, std::max(1, NBS / 4));  // amortise weight staging over >= 8 row tiles
}
static int one_S(const mile_sampler *, int) { return 1; }   // the layer-wise paths: every launch covers all rows

// k_grad_narrow: 16-row tiles, workgroups of up to 4 waves.  About four waves per SIMD over the whole grid (16 x CUs waves) and
// NO MORE row splits than that needs: every split is one more slab the update kernels sum -- with S = 64 splits of a d = 402
// net the two update launches of a step took 27-31 us each against 6.8 us for the gradient itself (profiles/r03/12_*), the
// slab / llpart loops being 64 dependent global loads long.  E = 12, N = 1052 (66 tiles): 17 splits of 4 waves; E = 128: 8.
static int narrow_S(const mile_sampler *s, int E) {
  const int tiles = (s->N + 15) / 16;
  if (narrow_tiles_hidden(s->spec) >= 3)      // LDS-weight form: ~100 KB of images staged per workgroup -> one workgroup per CU
    return std::max(1, std::min({64, s->n_cu / std::max(E, 1), std::max(1, tiles / NRW_MAXW)}));
  const int waves_per_particle = std::max(1, std::min(tiles, (16 * s->n_cu + std::max(E, 1) - 1) / std::max(E, 1)));
  return std::max(1, std::min(64, (waves_per_particle + NRW_MAXW - 1) / NRW_MAXW));
}
static int narrow_waves(const mile_sampler *s, int S, int N) {
  const int tiles = (N + 15) / 16;
  return std::max(1, std::min(NRW_MAXW, (tiles + S - 1) / S));
}

// k_grad_lenetti: about two workgroups per CU over the grid, at most 64 row ranges (every range is one more slab the update
// kernels sum) and at least 32 images per range
static int lenetti_S(const mile_sampler *s, int E) {
  const int want = (2 * s->n_cu + std::max(E, 1) - 1) / std::max(E, 1);
  return std::max(1, std::min({64, want, std::max(1, s->N / 32)}));
}

// k_grad_attn / k_grad_attn_pre, and the evaluation of all three attention models: one workgroup per CU (its LDS), at most 64
// row ranges and at least 16 sequences per range
static int attn_ranges(int n_cu, int E, int rows) {
  const int want = (n_cu + std::max(E, 1) - 1) / std::max(E, 1);
  return std::max(1, std::min({64, want, std::max(1, rows / 16)}));
}
static int attn_S(const mile_sampler *s, int E) { return attn_ranges(s->n_cu, E, s->N); }

// k_grad_attn_wide: every row range is one more slab row, and a slab row holds a [V][C] table block (7.68 MB at V = 10 000,
// C = 192) that its workgroup zero-fills before the first sequence and the update sums afterwards.  One workgroup per CU is
// still the aim -- a sequence costs ~0.5 ms of one CU, a table block ~2 us of HBM time each way at full width -- so there is
// no cap at 64 ranges: one chain on N = 35 000 rows takes all 256 CUs (2.04 GB of slabs, ~1 ms of fill + sum against >= 60 ms
// of gradient).  But a range must hold enough sequences to pay for a fill that ONE workgroup does alone (7.68 MB from one CU:
// ~0.15 ms, a third of a sequence): at least ATTN_WIDE_MIN_ROWS, so a 256-row warm-start minibatch is cut into 32 ranges, not
// 256.  The rows are the row window's when one is set; mile_reserve sizes for the whole data set, which is never fewer.
#define ATTN_WIDE_MIN_ROWS 8
static int attn_wide_S_rows(const mile_sampler *s, int E, int rows) {
  const int want = (s->n_cu + std::max(E, 1) - 1) / std::max(E, 1);
  return std::max(1, std::min(want, std::max(1, rows / ATTN_WIDE_MIN_ROWS)));
}
static int attn_wide_S(const mile_sampler *s, int E) { return attn_wide_S_rows(s, E, s->win_count ? s->win_count : s->N); }

// ---- partition sampling -------------------------------------------------------------------------------------------------------
// The dimension of everything the integrator and the tuner touch: d_s in partition mode, d otherwise.
static int sample_dim(const mile_sampler *s) { return s->part ? s->part_d : s->ds.d; }
static int sample_dp(const mile_sampler *s) { return (sample_dim(s) + 3) / 4 * 4; }
static float *sample_slabs(const mile_sampler *s) { return s->part ? s->part_slabs : s->slabs; }

// General path, before the grad launch: the compact rows' segments into the library's full-layout rows.
__global__ void k_part_scatter(const float *compact, int ds, float *full, int d, PartSegs sg) {
  const float *c = compact + (size_t)blockIdx.x * ds;
  float *f = full + (size_t)blockIdx.x * d;
  int o = 0;
  for (int k = 0; k < sg.n; ++k) {
    for (int i = threadIdx.x; i < sg.len[k]; i += blockDim.x) f[sg.begin[k] + i] = c[o + i];
    o += sg.len[k];
  }
}
// General path, after it: the sampled segments of every full-layout slab row (E * S of them) into the compact slab rows.
__global__ void k_part_gather(const float *full, long long dp, float *compact, long long dps, PartSegs sg) {
  const float *f = full + (size_t)blockIdx.x * dp;
  float *c = compact + (size_t)blockIdx.x * dps;
  int o = 0;
  for (int k = 0; k < sg.n; ++k) {
    for (int i = threadIdx.x; i < sg.len[k]; i += blockDim.x) c[o + i] = f[sg.begin[k] + i];
    o += sg.len[k];
  }
}

// Everything the library knows about one grad kernel: one row per MILE_GRAD_* id in kGrad, defined below the launchers.
struct LaunchShape { int block, lds; };
struct GradKernel {
  int id;                                             // MILE_GRAD_*
  const char *name;                                   // what mile_grad_launch_info reports
  bool (*supports)(const mile_sampler *);             // the specs it runs: loads, allocates and reads nothing else
  const char *refusal;                                // mile_set_grad_kernel's message for any other spec
  const char *needs_rocblas;                          // non-null: mile_set_grad_kernel loads rocBLAS, and this is why it failed
  int (*row_splits)(const mile_sampler *, int E);     // S: row ranges (slabs) per particle
  bool windowed;                                      // takes a row window (mile_set_row_window)
  bool fuses;                                         // can run the update that follows as its epilogue (W64Fuse)
  int (*grad)(mile_sampler *, const GradParams &, const W64Fuse &, int E, hipStream_t);
  int (*loglik)(mile_sampler *, PredParams pp, int S, hipStream_t);   // mile_pointwise_loglik on the staged evaluation set;
                                                                      // pp.y == nullptr: mile_predict, raw outputs [S, N, O]
  LaunchShape (*shape)(const mile_sampler *, int S);  // block and LDS bytes that mile_grad_launch_info reports
};
static const GradKernel &grad_kernel(int kernel);

// MILE_GRAD_AUTO, as a priority list
static int auto_kernel(const mile_sampler *s) {
  if (w64x3_supported(s)) return MILE_GRAD_MFMA_W64_BF16X3;   // fp32-faithful and never slower than MFMA_W64
  if (w64_supported(s)) return MILE_GRAD_MFMA_W64;
  // wide nets: the hand-written layer-wise MFMA GEMMs (fp32-faithful); rocBLAS (GEMM_F32) is the cross-check, never AUTO
  if (gemm_preferred(s)) return MILE_GRAD_MFMA_WIDE_BF16X3;
  // the reference's own nets (16 / 32 wide, any activation, either head): fused fp32-MFMA kernel
  if (narrow_supported(s) && getenv("MILE_NO_NARROW") == nullptr) return MILE_GRAD_MFMA_NARROW_F32;
  if (is_lenet(s)) return MILE_GRAD_LENET_F32;                // the other models: their own kernel
  if (is_lenetti(s)) return MILE_GRAD_LENETTI_F32;
  if (is_attn(s)) return MILE_GRAD_ATTN_F32;
  if (is_attn_pre(s)) return MILE_GRAD_ATTN_PRE_F32;
  if (is_attn_wide(s)) return MILE_GRAD_ATTN_WIDE_F32;
  return MILE_GRAD_GENERIC;
}
static int resolved_kernel(const mile_sampler *s) { return s->grad_kernel == MILE_GRAD_AUTO ? auto_kernel(s) : s->grad_kernel; }
static int choose_S(const mile_sampler *s, int E, int kernel) { return grad_kernel(kernel).row_splits(s, E); }

// ---- one layout per model family: validates the spec, fills the geometry, ds and the ABI layers of mile_param_offsets -------
// The FCN's parameter row, the one table every user of the layout reads (mile_eval_handle.h): ravel_pytree order, layers sorted
// by NAME ("layer10" < "layer2"), bias before kernel.  Returns d.
long long fcn_param_layout(const mile_model_spec *spec, FcnOffsets ds) {
  std::vector<int> order(spec->n_layers);
  for (int i = 0; i < spec->n_layers; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [](int a, int b) {
    return std::string("layer") + std::to_string(a) < std::string("layer") + std::to_string(b);
  });
  long long off = 0;
  for (int li : order) {
    const int fin = li == 0 ? spec->in_features : spec->widths[li - 1], fout = spec->widths[li];
    ds.b_off[li] = (int)off; off += fout;
    ds.w_off[li] = (int)off; off += (long long)fin * fout;
  }
  return off;
}

static int layout_fcn(mile_sampler *s) {
  const mile_model_spec *spec = &s->spec;
  DevSpec &ds = s->ds;
  const long long off = fcn_param_layout(spec, FcnOffsets{ds.b_off, ds.w_off});
  if (off > 0x7fffffffLL) return fail(MILE_ERR_INVALID, "parameter count exceeds int32");
  if (off < 2) return fail(MILE_ERR_INVALID, "The target distribution must have more than 1 dimension for MCLMC.");
  ds.d = (int)off;
  ds.act_off[0] = 0;
  int a = spec->in_features, mw = spec->in_features;
  for (int l = 0; l < spec->n_layers; ++l) {
    ds.widths[l] = spec->widths[l];
    ds.act_off[l + 1] = a;
    a += spec->widths[l];
    mw = std::max(mw, spec->widths[l]);
    s->layers.push_back({ds.b_off[l], ds.w_off[l]});
  }
  ds.act_stride = a;
  ds.max_width = mw;
  if (generic_R(ds) < 1) return fail(MILE_ERR_INVALID, "network too wide for the generic kernel");
  return MILE_OK;
}

static int layout_lenet(mile_sampler *s) {   // ravel_pytree order of {'core': {conv1, conv2, fc1, fc2, fc3}}: bias, kernel each
  const mile_model_spec *spec = &s->spec;
  if (spec->n_layers != 1) return fail(MILE_ERR_INVALID, "LeNet: n_layers must be 1 (widths[0] = out_dim)");
  if (spec->img_c < 1 || spec->img_h < 1 || spec->img_w < 1 ||
      (long long)spec->img_c * spec->img_h * spec->img_w != spec->in_features)
    return fail(MILE_ERR_INVALID, "LeNet: in_features must equal img_c * img_h * img_w");
  if ((spec->img_h / 2 - 4) / 2 < 1 || (spec->img_w / 2 - 4) / 2 < 1) return fail(MILE_ERR_INVALID, "LeNet: image too small");
  if (!rocblas_load()) return fail(MILE_ERR_HIP, "LeNet needs librocblas.so, which could not be loaded");
  LeNetGeom &g = s->lg;
  g.C = spec->img_c; g.H = spec->img_h; g.W = spec->img_w; g.K = spec->widths[0];
  g.hp1 = g.H / 2; g.wp1 = g.W / 2; g.h2 = g.hp1 - 4; g.w2 = g.wp1 - 4; g.hp2 = g.h2 / 2; g.wp2 = g.w2 / 2;
  g.flat = g.hp2 * g.wp2 * 16;
  long long o = 0;
  g.b_c1 = (int)o; o += 6;   g.k_c1 = (int)o; o += 25LL * g.C * 6;
  g.b_c2 = (int)o; o += 16;  g.k_c2 = (int)o; o += 150LL * 16;
  g.b_f1 = (int)o; o += 120; g.k_f1 = (int)o; o += (long long)g.flat * 120;
  g.b_f2 = (int)o; o += 84;  g.k_f2 = (int)o; o += 120LL * 84;
  g.b_f3 = (int)o; o += g.K; g.k_f3 = (int)o; o += 84LL * g.K;
  if (o > 0x7fffffffLL) return fail(MILE_ERR_INVALID, "parameter count exceeds int32");
  g.d = (int)o;
  s->ds.d = g.d;
  s->ds.widths[0] = g.K;
  s->ds.b_off[0] = g.b_c1; s->ds.w_off[0] = g.k_c1;
  s->ds.max_width = 150; s->ds.act_stride = 0;
  s->layers = {{g.b_c1, g.k_c1}, {g.b_c2, g.k_c2}, {g.b_f1, g.k_f1}, {g.b_f2, g.k_f2}, {g.b_f3, g.k_f3}};
  return MILE_OK;
}

static int layout_lenetti(mile_sampler *s) {   // ravel_pytree order of {'core': {conv1, fc1, fc2, fc3, fc4}}: bias, kernel each
  const mile_model_spec *spec = &s->spec;
  if (spec->n_layers != 1) return fail(MILE_ERR_INVALID, "LeNetti: n_layers must be 1 (widths[0] = out_dim)");
  if (spec->img_c < 1 || spec->img_h < 1 || spec->img_w < 1 ||
      (long long)spec->img_c * spec->img_h * spec->img_w != spec->in_features)
    return fail(MILE_ERR_INVALID, "LeNetti: in_features must equal img_c * img_h * img_w");
  if (spec->img_c > LENETTI_MAX_C) return fail(MILE_ERR_INVALID, "LeNetti: at most 4 image channels");
  if ((long long)(spec->img_h + 2) * (spec->img_w + 2) > LENETTI_NT * LENETTI_MAX_PPT)
    return fail(MILE_ERR_INVALID, "LeNetti: (H+2)*(W+2) must be <= 2048 conv-output pixels");
  if (spec->widths[0] > LENETTI_MAX_K) return fail(MILE_ERR_INVALID, "LeNetti: out_dim must be <= 16");
  LeNettiGeom &g = s->ng;
  g.C = spec->img_c; g.H = spec->img_h; g.W = spec->img_w; g.K = spec->widths[0];
  g.Ho = g.H + 2; g.Wo = g.W + 2; g.P = g.Ho * g.Wo;
  int o = 0;
  g.b_c = o; o += 1;   g.k_c = o; o += 9 * g.C;
  g.b_1 = o; o += 8;   g.k_1 = o; o += 8 * g.P;
  g.b_2 = o; o += 8;   g.k_2 = o; o += 64;
  g.b_3 = o; o += 8;   g.k_3 = o; o += 64;
  g.b_4 = o; o += g.K; g.k_4 = o; o += 8 * g.K;
  g.d = o;
  s->ds.d = g.d;
  s->ds.widths[0] = g.K;
  s->ds.b_off[0] = g.b_c; s->ds.w_off[0] = g.k_c;
  s->ds.max_width = 8; s->ds.act_stride = 0;
  s->layers = {{g.b_c, g.k_c}, {g.b_1, g.k_1}, {g.b_2, g.k_2}, {g.b_3, g.k_3}, {g.b_4, g.k_4}};
  return MILE_OK;
}

// The three attention models.  tables == true (the two AttentionClassifiers): ravel_pytree order (sorted keys) MDPA.{key, out,
// query, value}, TokenEmbedding_0, classifier, projection_*; bias before kernel.  ABI layers: key, out, query, value, Embedding,
// PositionEmbedding (no bias: -1), classifier, projection_*.  tables == false (PretrainedAttentionClassifier): the same without
// the TokenEmbedding_0 leaves and their two ABI layers -- the tables are frozen (mile_set_embedding).
// max_c / max_d / max_p: the kernel's limits on emb_size, qkv_dim and the projection widths; supported: its envelope, LDS
// included; max_v: token ids travel as fp32, so the vocabulary ends at 2^24 (the wide model takes what its spec takes, V < 2^24)
static int layout_attn_model(mile_sampler *s, const std::string &name, int max_c, int max_d, int max_p, bool tables,
                             bool (*supported)(const AttnGeom &), int max_v) {
  const mile_model_spec *spec = &s->spec;
  if (spec->task != MILE_TASK_CLASSIFICATION) return fail(MILE_ERR_INVALID, name + ": classification only");
  if (spec->n_layers < 1 || spec->n_layers > ATTN_MAX_NP + 1)
    return fail(MILE_ERR_INVALID, name + ": widths = projection_dim (at most 2) + [n_classes]");
  if (spec->ctx_len < 1 || spec->ctx_len > ATTN_MAX_T || spec->in_features != spec->ctx_len)
    return fail(MILE_ERR_INVALID, name + ": 1 <= ctx_len <= 128 and in_features == ctx_len");
  if (spec->emb_size < 1 || spec->emb_size > max_c) return fail(MILE_ERR_INVALID, name + ": emb_size <= " + std::to_string(max_c));
  if (spec->qkv_dim < 1 || spec->qkv_dim > max_d || spec->n_heads < 1 || spec->qkv_dim % spec->n_heads)
    return fail(MILE_ERR_INVALID, name + ": qkv_dim <= " + std::to_string(max_d) + " and n_heads dividing it");
  if (spec->vocab_size < 1 || spec->vocab_size > max_v)
    return fail(MILE_ERR_INVALID, name + (max_v < (1 << 24) ? ": 1 <= vocab_size < 2^24" : ": 1 <= vocab_size <= 2^24"));
  for (int l = 0; l + 1 < spec->n_layers; ++l)
    if (spec->widths[l] > max_p) return fail(MILE_ERR_INVALID, name + ": projection widths <= " + std::to_string(max_p));
  if (spec->widths[spec->n_layers - 1] > ATTN_MAX_K) return fail(MILE_ERR_INVALID, name + ": n_classes <= 16");
  AttnGeom &g = s->ag;
  g.V = spec->vocab_size; g.T = spec->ctx_len; g.C = spec->emb_size; g.H = spec->n_heads; g.D = spec->qkv_dim;
  g.hd = g.D / g.H; g.NP = spec->n_layers - 1; g.K = spec->widths[g.NP]; g.bias = spec->use_bias ? 1 : 0;
  g.Tp = (g.T + 15) / 16 * 16;
  for (int l = 0; l < ATTN_MAX_NP; ++l) { g.P[l] = l < g.NP ? spec->widths[l] : 0; g.b_p[l] = g.k_p[l] = -1; }
  g.emb = g.pos = tables ? 0 : -1;                   // (the wide envelope asks for tables; their offsets follow)
  if (!supported(g)) return fail(MILE_ERR_INVALID, name + ": shape needs more than 160 KB of LDS");
  long long o = 0;
  auto put = [&](int &b, int &k, long long nb, long long nk) { b = g.bias && nb ? (int)o : -1; o += g.bias ? nb : 0; k = (int)o; o += nk; };
  int no_bias;
  put(g.b_k, g.k_k, g.D, (long long)g.C * g.D);
  put(g.b_o, g.k_o, g.C, (long long)g.D * g.C);
  put(g.b_q, g.k_q, g.D, (long long)g.C * g.D);
  put(g.b_v, g.k_v, g.D, (long long)g.C * g.D);
  if (tables) {
    put(no_bias, g.emb, 0, (long long)g.V * g.C);
    put(no_bias, g.pos, 0, (long long)g.T * g.C);
  }
  put(g.b_c, g.k_c, g.K, (long long)(g.NP ? g.P[g.NP - 1] : g.C) * g.K);
  for (int l = 0; l < g.NP; ++l) put(g.b_p[l], g.k_p[l], g.P[l], (long long)(l ? g.P[l - 1] : g.C) * g.P[l]);
  if (o > 0x7fffffffLL) return fail(MILE_ERR_INVALID, name + ": too many parameters");
  g.d = (int)o;
  s->ds.d = g.d;
  s->ds.widths[0] = g.K;
  s->ds.b_off[0] = g.b_c; s->ds.w_off[0] = g.k_c;
  s->ds.max_width = 64; s->ds.act_stride = 0;
  s->layers = {{g.b_k, g.k_k}, {g.b_o, g.k_o}, {g.b_q, g.k_q}, {g.b_v, g.k_v}};
  if (tables) { s->layers.push_back({-1, g.emb}); s->layers.push_back({-1, g.pos}); }
  s->layers.push_back({g.b_c, g.k_c});
  for (int l = 0; l < g.NP; ++l) s->layers.push_back({g.b_p[l], g.k_p[l]});
  return MILE_OK;
}
static int layout_attn(mile_sampler *s) {
  return layout_attn_model(s, "AttentionClassifier", ATTN_MAX_C, ATTN_MAX_D, ATTN_MAX_P, true, attn_supported, 1 << 24);
}
static int layout_attn_pre(mile_sampler *s) {
  return layout_attn_model(s, "PretrainedAttentionClassifier", ATTNP_MAX_C, ATTNP_MAX_D, ATTNP_MAX_P, false, attnp_supported, 1 << 24);
}
static int layout_attn_wide(mile_sampler *s) {
  return layout_attn_model(s, "AttentionClassifier (wide)", ATTNP_MAX_C, ATTNP_MAX_D, ATTNP_MAX_P, true, attn_wide_supported, (1 << 24) - 1);
}

extern "C" {

const char *mile_last_error(void) { return g_err.c_str(); }
int32_t mile_abi_version(void) { return MILE_ABI_VERSION; }

int32_t mile_create(const mile_model_spec *spec, int32_t device, mile_sampler **out) {
  if (!spec || !out) return fail(MILE_ERR_INVALID, "mile_create: null argument");
  if (spec->n_layers < 1 || spec->n_layers > MILE_MAX_LAYERS) return fail(MILE_ERR_INVALID, "n_layers out of range");
  if (spec->in_features < 1) return fail(MILE_ERR_INVALID, "in_features must be >= 1");
  const bool attn_family = spec->model == MILE_MODEL_ATTN || spec->model == MILE_MODEL_ATTN_PRETRAINED || spec->model == MILE_MODEL_ATTN_WIDE;
  if (!spec->use_bias && !attn_family) return fail(MILE_ERR_INVALID, "use_bias=false is not supported");
  if (spec->activation < 0 || spec->activation > MILE_ACT_SIGMOID) return fail(MILE_ERR_INVALID, "unknown activation");
  if (spec->task != MILE_TASK_REGRESSION && spec->task != MILE_TASK_CLASSIFICATION) return fail(MILE_ERR_INVALID, "unknown task");
  if (spec->prior != MILE_PRIOR_NORMAL && spec->prior != MILE_PRIOR_LAPLACE) return fail(MILE_ERR_INVALID, "unknown prior");
  if (!(spec->prior_scale > 0.0f)) return fail(MILE_ERR_INVALID, "prior_scale must be > 0");
  for (int l = 0; l < spec->n_layers; ++l)
    if (spec->widths[l] < 1) return fail(MILE_ERR_INVALID, "layer width must be >= 1");
  if (spec->task == MILE_TASK_REGRESSION && spec->widths[spec->n_layers - 1] != 2)
    return fail(MILE_ERR_INVALID, "regression needs an output layer of width 2 (mu, log sigma)");
  static int (*const layout[])(mile_sampler *) = {layout_fcn, layout_lenet, layout_lenetti, layout_attn, layout_attn_pre,
                                                  layout_attn_wide};   // by mile_model
  if (spec->model < MILE_MODEL_FCN || spec->model > MILE_MODEL_ATTN_WIDE) return fail(MILE_ERR_INVALID, "unknown model");

  auto *s = new mile_sampler();
  s->spec = *spec;
  s->device = device;
  DevSpec &ds = s->ds;
  ds.n_layers = spec->n_layers;
  ds.in_features = spec->in_features;
  ds.activation = spec->activation;
  ds.task = spec->task;
  ds.prior = spec->prior;
  ds.prior_loc = spec->prior_loc;
  ds.prior_scale = spec->prior_scale;
  if (const int rc = layout[spec->model](s)) {
    delete s;
    return rc;
  }
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) == hipSuccess && device < cnt) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) s->n_cu = prop.multiProcessorCount;
  }
  *out = s;
  return MILE_OK;
}

static void free_data(mile_sampler *s) {
  if (s->X) (void)hipFree(s->X);
  if (s->Xp) (void)hipFree(s->Xp);
  if (s->y) (void)hipFree(s->y);
  if (s->Xb) (void)hipFree(s->Xb);
  if (s->Xt) (void)hipFree(s->Xt);
  s->X = s->Xp = nullptr; s->y = nullptr; s->Xb = s->Xt = nullptr;
}
static void free_ws(mile_sampler *s) {
  if (s->slabs) (void)hipFree(s->slabs);
  if (s->llpart) (void)hipFree(s->llpart);
  if (s->dK) (void)hipFree(s->dK);
  if (s->upart) (void)hipFree(s->upart);
  s->upart = nullptr;
  if (s->lold) (void)hipFree(s->lold);
  if (s->alt_x) (void)hipFree(s->alt_x);
  if (s->alt_u) (void)hipFree(s->alt_u);
  if (s->alt_g) (void)hipFree(s->alt_g);
  if (s->alt_logp) (void)hipFree(s->alt_logp);
  s->alt_x = s->alt_u = s->alt_g = s->alt_logp = nullptr;
  if (s->tune_info) (void)hipFree(s->tune_info);
  s->tune_info = nullptr;
  if (s->arrive) (void)hipFree(s->arrive);
  s->arrive = nullptr;
  if (s->nzbuf) (void)hipFree(s->nzbuf);
  s->nzbuf = nullptr;
  s->nz_E = 0;
  if (s->part_slabs) (void)hipFree(s->part_slabs);
  s->part_slabs = nullptr;
  s->slabs = s->llpart = s->dK = s->lold = nullptr;
  s->E_cap = 0; s->ES_cap = 0;
}

static void free_nuts(mile_sampler *s) {
  NutsBufs &b = s->nb;
  float **fs[] = {&b.T, &b.Ph, &b.xe[0], &b.xe[1], &b.pe[0], &b.pe[1], &b.ge[0], &b.ge[1], &b.psT, &b.psS, &b.xs, &b.gs,
                  &b.ck_r, &b.ck_rs};
  for (float **f : fs) { if (*f) (void)hipFree(*f); *f = nullptr; }
  if (b.chain) (void)hipFree(b.chain);
  if (b.count) (void)hipFree(b.count);
  b.chain = nullptr; b.count = nullptr;
  s->nuts_E = s->nuts_M = 0;
}

int32_t mile_destroy(mile_sampler *s) {
  if (!s) return MILE_OK;
  if (s->ev_rows) (void)hipFree(s->ev_rows);
  if (s->eval_ws) (void)hipFree(s->eval_ws);
  free_data(s);
  free_ws(s);
  if (s->gemm_ws) (void)hipFree(s->gemm_ws);
  if (s->gemm_ones) (void)hipFree(s->gemm_ones);
  if (s->wide_ws) (void)hipFree(s->wide_ws);
  if (s->wide_wt) (void)hipFree(s->wide_wt);
  if (s->wide_hb) (void)hipFree(s->wide_hb);
  if (s->tune_info) (void)hipFree(s->tune_info);
  if (s->emb_tab) (void)hipFree(s->emb_tab);
  if (s->pos_tab) (void)hipFree(s->pos_tab);
  if (s->part_rows) (void)hipFree(s->part_rows);
  free_nuts(s);
  if (s->nuts_count_h) (void)hipHostFree(s->nuts_count_h);
  if (s->blas && g_rb.destroy) (void)g_rb.destroy(s->blas);
  for (auto ev : s->ev) (void)hipEventDestroy(ev);
  delete s;
  return MILE_OK;
}

int64_t mile_param_count(const mile_sampler *s) { return s ? s->ds.d : -1; }

int32_t mile_param_offsets(const mile_sampler *s, int32_t layer, int64_t *bias_off, int64_t *kernel_off) {
  if (!s || layer < 0 || layer >= (int)s->layers.size()) return fail(MILE_ERR_INVALID, "mile_param_offsets: bad layer");
  if (bias_off) *bias_off = s->layers[layer].bias_off;
  if (kernel_off) *kernel_off = s->layers[layer].kernel_off;
  return MILE_OK;
}

__global__ void k_pad_x(const float *X, float *Xp, int N, int Npad, int F, int Fp) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)Npad * Fp) return;
  const int r = (int)(idx / Fp), c = (int)(idx % Fp);
  Xp[idx] = (r < N && c < F) ? X[(long long)r * F + c] : 0.0f;
}

__global__ void k_prep_bf16(const float *X, bf16 *Xb, bf16 *Xt, int N, int Npad, int F) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)Npad * 32) return;
  const int r = (int)(idx >> 5), c = (int)(idx & 31);
  const bf16 v = (bf16)((r < N && c < F) ? X[(long long)r * F + c] : 0.0f);
  if (c < 16) Xb[(long long)r * 16 + c] = v;
  Xt[(long long)c * Npad + r] = v;
}

int32_t mile_set_data(mile_sampler *s, const float *X, const void *y, int64_t N, void *stream) {
  if (!s || !X || !y) return fail(MILE_ERR_INVALID, "mile_set_data: null argument");
  if (N < 1 || N > 0x3fffffff) return fail(MILE_ERR_INVALID, "mile_set_data: N out of range");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->device));
  const int F = s->spec.in_features;
  // Same number of rows as before (the warm-start stage hands over a reshuffled copy of the training set every epoch,
  // src/dataset/tabular.py:170-212): every buffer and the workspace keep their sizes -- overwrite in place, no
  // free / malloc cycle of ~15 allocations per epoch.
  const bool w128b = grad_kernel(MILE_GRAD_MFMA_W128_BF16).supports(s);   // + the bf16 copies of k_grad_w128b
  const bool same_shape = s->N == (int)N && s->X && s->Xp && s->y && (!w128b || (s->Xb && s->Xt));
  if (!same_shape) {
    free_data(s);
    free_ws(s);
  }
  s->N = (int)N;
  s->Npad = ((int)N + 31) / 32 * 32;
  s->Fp = (F + 7) / 8 * 8;
  if (!same_shape) {
    HIP_TRY(hipMalloc(&s->X, (size_t)N * F * 4));
    // (32 rows of slack: a row window that ends at the last row still reads whole 32-row blocks from its own first row)
    HIP_TRY(hipMalloc(&s->Xp, (size_t)(s->Npad + 32) * s->Fp * 4));
    HIP_TRY(hipMalloc(&s->y, (size_t)(s->Npad + 32) * 4));
  }
  HIP_TRY(hipMemsetAsync(s->Xp, 0, (size_t)(s->Npad + 32) * s->Fp * 4, st));
  HIP_TRY(hipMemcpyAsync(s->X, X, (size_t)N * F * 4, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemsetAsync(s->y, 0, (size_t)(s->Npad + 32) * 4, st));
  s->win_begin = s->win_count = 0;
  HIP_TRY(hipMemcpyAsync(s->y, y, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  const long long tot = (long long)s->Npad * s->Fp;
  k_pad_x<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(s->X, s->Xp, s->N, s->Npad, F, s->Fp);
  HIP_TRY(hipGetLastError());
  if (w128b) {
    s->Npb = ((int)N + 63) / 64 * 64;
    if (!same_shape) {
      HIP_TRY(hipMalloc(&s->Xb, (size_t)s->Npb * 16 * 2));
      HIP_TRY(hipMalloc(&s->Xt, (size_t)s->Npb * 32 * 2));
    }
    const long long tb = (long long)s->Npb * 32;
    k_prep_bf16<<<(unsigned)((tb + 255) / 256), 256, 0, st>>>(s->X, (bf16 *)s->Xb, (bf16 *)s->Xt, s->N, s->Npb, F);
    HIP_TRY(hipGetLastError());
  }
  return MILE_OK;
}

int32_t mile_set_embedding(mile_sampler *s, const float *emb, const float *pos, void *stream) {
  if (!s || !emb || !pos) return fail(MILE_ERR_INVALID, "mile_set_embedding: null argument");
  if (!is_attn_pre(s)) return fail(MILE_ERR_INVALID, "mile_set_embedding: only MILE_MODEL_ATTN_PRETRAINED has frozen tables");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->device));
  const AttnGeom &g = s->ag;
  if (!s->emb_tab) {
    HIP_TRY(hipMalloc(&s->emb_tab, (size_t)g.V * g.C * 4));
    HIP_TRY(hipMalloc(&s->pos_tab, (size_t)g.T * g.C * 4));
  }
  HIP_TRY(hipMemcpyAsync(s->emb_tab, emb, (size_t)g.V * g.C * 4, hipMemcpyDefault, st));
  HIP_TRY(hipMemcpyAsync(s->pos_tab, pos, (size_t)g.T * g.C * 4, hipMemcpyDefault, st));
  return MILE_OK;
}

int32_t mile_set_row_window(mile_sampler *s, int64_t begin, int64_t count) {
  if (!s) return fail(MILE_ERR_INVALID, "null handle");
  if (!s->X) return fail(MILE_ERR_STATE, "mile_set_row_window: call mile_set_data first");
  if (begin < 0 || count < 0 || begin + count > s->N) return fail(MILE_ERR_INVALID, "mile_set_row_window: window outside the data");
  s->win_begin = count ? (int)begin : 0;
  s->win_count = (int)count;
  return MILE_OK;
}

int32_t mile_set_partition(mile_sampler *s, const float *frozen, int32_t E, void *stream) {
  if (!s || !frozen || E < 1) return fail(MILE_ERR_INVALID, "mile_set_partition: bad argument");
  if (!is_fcn(s)) return fail(MILE_ERR_INVALID, "mile_set_partition: partition sampling is built for the FCN only (first and last Dense layer)");
  const int n = s->spec.n_layers;
  if (n <= 2) return MILE_OK;   // no frozen layer: partition sampling of this net is ordinary sampling
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->device));
  // the four sampled leaves in full-row order, adjacent ones merged into one segment
  const DevSpec &ds = s->ds;
  struct Leaf { int off, len, which; } lv[4] = {
      {ds.b_off[0], ds.widths[0], 0}, {ds.w_off[0], ds.in_features * ds.widths[0], 1},
      {ds.b_off[n - 1], ds.widths[n - 1], 2}, {ds.w_off[n - 1], ds.widths[n - 2] * ds.widths[n - 1], 3}};
  std::sort(lv, lv + 4, [](const Leaf &a, const Leaf &b) { return a.off < b.off; });
  PartSegs sg{};
  int o = 0, coff[4];
  for (const Leaf &l : lv) {
    if (sg.n && sg.begin[sg.n - 1] + sg.len[sg.n - 1] == l.off) sg.len[sg.n - 1] += l.len;
    else { sg.begin[sg.n] = l.off; sg.len[sg.n] = l.len; ++sg.n; }
    coff[l.which] = o;
    o += l.len;
  }
  if (s->part_rows && s->part_E != E) { (void)hipFree(s->part_rows); s->part_rows = nullptr; }
  if (!s->part_rows) HIP_TRY(hipMalloc(&s->part_rows, (size_t)E * ds.d * 4));
  HIP_TRY(hipMemcpyAsync(s->part_rows, frozen, (size_t)E * ds.d * 4, hipMemcpyDeviceToDevice, st));
  if (!s->part) free_ws(s);   // the compact slabs are part of the workspace: the next mile_reserve allocates them
  s->part = true; s->part_E = E; s->part_d = o; s->part_seg = sg;
  s->part_b0 = coff[0]; s->part_w0 = coff[1]; s->part_bl = coff[2]; s->part_wl = coff[3];
  return MILE_OK;
}

int64_t mile_partition_dim(const mile_sampler *s) { return s ? sample_dim(s) : -1; }

int32_t mile_partition_segments(const mile_sampler *s, int64_t *begin, int64_t *length, int32_t capacity) {
  if (!s) return fail(MILE_ERR_INVALID, "mile_partition_segments: null handle");
  if (!s->part) return 0;
  if ((begin || length) && capacity < s->part_seg.n) return fail(MILE_ERR_INVALID, "mile_partition_segments: capacity too small");
  for (int k = 0; k < s->part_seg.n; ++k) {
    if (begin) begin[k] = s->part_seg.begin[k];
    if (length) length[k] = s->part_seg.len[k];
  }
  return s->part_seg.n;
}

// floats of one of the two noise-prefill arrays in s->nzbuf (E rows of d, rounded up so the second array is 16-byte aligned)
static size_t nz_stride(int E, int d) { return ((size_t)E * d + 3) / 4 * 4; }

int32_t mile_reserve(mile_sampler *s, int32_t E) {
  if (!s || E < 1) return fail(MILE_ERR_INVALID, "mile_reserve: bad argument");
  if (!s->X) return fail(MILE_ERR_STATE, "mile_reserve: call mile_set_data first");
  HIP_TRY(hipSetDevice(s->device));
  // capacity must cover whichever grad kernel is selected later
  int S = 1;   // (only the kernels that run this model: GENERIC's 64 ranges would double the wide attention's 2 GB)
  for (int k = MILE_GRAD_GENERIC; k <= MILE_GRAD_LENET_BF16X3; ++k)
    if (grad_kernel(k).supports(s)) S = std::max(S, choose_S(s, E, k));
  if (is_attn_wide(s)) S = std::max(S, attn_wide_S_rows(s, E, s->N));   // whatever row window is set now
  // A smaller ensemble splits the rows of a particle over MORE workgroups (S grows as E shrinks): capacity is counted in
  // slab rows E * S, and a later call with fewer particles must neither fail nor shrink what a larger one reserved.
  if (E <= s->E_cap && (size_t)E * S <= s->ES_cap) return MILE_OK;
  const int En = std::max(E, s->E_cap);
  const size_t ESn = std::max((size_t)E * S, s->ES_cap);
  free_ws(s);
  HIP_TRY(hipMalloc(&s->slabs, ESn * ((s->ds.d + 3) / 4 * 4) * 4));
  if (s->part) HIP_TRY(hipMalloc(&s->part_slabs, ESn * sample_dp(s) * 4));
  HIP_TRY(hipMalloc(&s->llpart, ESn * 4));
  HIP_TRY(hipMalloc(&s->dK, (size_t)En * 4));
  HIP_TRY(hipMalloc(&s->lold, (size_t)En * 4));
  HIP_TRY(hipMalloc(&s->upart, ((size_t)En * ((s->ds.d + UPD_SEG - 1) / UPD_SEG) * UPD_NSUM + (size_t)En * 8) * 4));
  HIP_TRY(hipMalloc(&s->alt_x, (size_t)En * s->ds.d * 4));
  HIP_TRY(hipMalloc(&s->alt_u, (size_t)En * s->ds.d * 4));
  HIP_TRY(hipMalloc(&s->alt_g, (size_t)En * s->ds.d * 4));
  HIP_TRY(hipMalloc(&s->alt_logp, (size_t)En * 4));
  HIP_TRY(hipMalloc(&s->arrive, ((size_t)En * 4 + 15) / 16 * 16));
  HIP_TRY(hipMemset(s->arrive, 0, ((size_t)En * 4 + 15) / 16 * 16));
  s->E_cap = En;
  s->ES_cap = ESn;
  return MILE_OK;
}

int32_t mile_set_grad_kernel(mile_sampler *s, int32_t which) {
  if (!s) return fail(MILE_ERR_INVALID, "null handle");
  if (which < MILE_GRAD_AUTO || which > MILE_GRAD_LENET_BF16X3) return fail(MILE_ERR_INVALID, "unknown grad kernel");
  if (which != MILE_GRAD_AUTO) {
    const GradKernel &k = grad_kernel(which);
    if (!k.supports(s)) return fail(MILE_ERR_INVALID, k.refusal);
    if (k.needs_rocblas && !rocblas_load()) return fail(MILE_ERR_HIP, k.needs_rocblas);
  }
  s->grad_kernel = which;
  return MILE_OK;
}
int32_t mile_get_grad_kernel(const mile_sampler *s) { return s ? resolved_kernel(s) : MILE_ERR_INVALID; }
int64_t mile_slab_bytes(const mile_sampler *s) { return s ? (int64_t)(s->ES_cap * ((size_t)(s->ds.d + 3) / 4 * 4) * 4) : -1; }

}  // extern "C"

// ------------------------------------------------------------------------------------
// grad launch
// ------------------------------------------------------------------------------------
static int ptr_align(const void *q) {   // alignment in floats (4, 2 or 1) of a device pointer
  const uintptr_t a = (uintptr_t)q;
  return (a & 15) == 0 ? 4 : ((a & 7) == 0 ? 2 : 1);
}

// Every row base of an update launch is (pointer + e*d): the vector width (4, 2 or 1 floats) allowed by d and by the row
// pointers the update kernels access in vectors.  (bk_* are read element by element; x_acc, when set, equals x_in.)
static int row_align(const UpdParams &u) {
  int al = (u.d % 4 == 0) ? 4 : ((u.d % 2 == 0) ? 2 : 1);
  const void *ptrs[] = {u.x, u.u, u.g, u.slabs, u.sdc, u.zA, u.zB, u.out_sample, u.x_in, u.u_in, u.g_in, u.t_avg, u.u_rec, u.nz_A, u.nz_B};
  for (const void *q : ptrs)
    if (q) al = std::min(al, ptr_align(q));
  return al;
}

// f(AL, SDC) with the launch's vector width and preconditioner as compile-time constants
template <class F>
static auto with_al_sdc(int al, bool sdc, F &&f) {
  using A4 = std::integral_constant<int, 4>;
  using A2 = std::integral_constant<int, 2>;
  using A1 = std::integral_constant<int, 1>;
  if (sdc) return al == 4 ? f(A4{}, std::true_type{}) : (al == 2 ? f(A2{}, std::true_type{}) : f(A1{}, std::true_type{}));
  return al == 4 ? f(A4{}, std::false_type{}) : (al == 2 ? f(A2{}, std::false_type{}) : f(A1{}, std::false_type{}));
}

template <int AL, bool SDC>
static void launch_update_al(const UpdParams &u, int E, int nk, hipStream_t st) {
  // fewest waves that still leave <= nk quads per thread: padded lanes are wasted VALU time in a kernel that only fills
  // half the chip (d = 8834: 2208 quads, nk = 3 -> 768 threads instead of 1024)
  const int nqf = u.d >> 2;
  const int nt = std::min(UPD_NT, ((nqf + nk - 1) / nk + 63) / 64 * 64);
  const int kind = SDC ? -1 : upd_kind(u);
  const int nwg_mid = (u.nz_A || u.nz_B) ? 2 * E : E;   // + E workgroups that prefill the next launch's noise
#define MILE_UPD_CASE(NK_)                                                                       \
  if constexpr (!SDC) {                                                                          \
    if (kind == UPD_KIND_MID) { k_update_fast<NK_, AL, SDC, UPD_KIND_MID><<<nwg_mid, nt, 0, st>>>(u); break; } \
    if (kind == UPD_KIND_REC) { k_update_fast<NK_, AL, SDC, UPD_KIND_REC><<<E, nt, 0, st>>>(u); break; } \
    if (kind == UPD_KIND_TUNE) {                                                                 \
      if (nt <= 768) k_update_fast<NK_, AL, SDC, UPD_KIND_TUNE, 768><<<E, nt, 0, st>>>(u);       \
      else k_update_fast<NK_, AL, SDC, UPD_KIND_TUNE><<<E, nt, 0, st>>>(u);                      \
      break;                                                                                     \
    }                                                                                            \
  }                                                                                              \
  if (nt <= 768) k_update_fast<NK_, AL, SDC, -1, 768><<<E, nt, 0, st>>>(u);                      \
  else k_update_fast<NK_, AL, SDC><<<E, nt, 0, st>>>(u);                                         \
  break;
  switch (nk) {
    case 1: MILE_UPD_CASE(1)
    case 2: MILE_UPD_CASE(2)
    case 3: MILE_UPD_CASE(3)
    default: MILE_UPD_CASE(4)
  }
#undef MILE_UPD_CASE
}

// d beyond the register cache, up to 4 * UPD_NT * UPD_QMAX_BIG: k_update_big (x, u in registers, g in LDS)
template <int NK, int AL, bool SDC>
static bool launch_update_big_nk(const UpdParams &u, int E, int nt, size_t lds, hipStream_t st) {
  if (mile_set_max_lds<k_update_big<NK, AL, SDC, -1>>(UPD_NT * NK * 16) != hipSuccess) return false;
  k_update_big<NK, AL, SDC, -1><<<E, nt, lds, st>>>(u);
  return true;
}
template <int AL, bool SDC>
static bool launch_update_big_al(const UpdParams &u, int E, int nk, hipStream_t st) {
  const int nqf = u.d >> 2;
  const int nt = std::min(UPD_NT, ((nqf + nk - 1) / nk + 63) / 64 * 64);
  const size_t lds = (size_t)nk * nt * 16;
  // no compile-time launch kinds here: with the flag tests folded the unrolled quads become one basic block, the compiler
  // interleaves them and spills 109 registers (NK = 9, record kind) against 7 with the run-time flags
  switch (nk) {
    case 5: return launch_update_big_nk<5, AL, SDC>(u, E, nt, lds, st);
    case 6: return launch_update_big_nk<6, AL, SDC>(u, E, nt, lds, st);
    case 7: return launch_update_big_nk<7, AL, SDC>(u, E, nt, lds, st);
    case 8: return launch_update_big_nk<8, AL, SDC>(u, E, nt, lds, st);
    case 9: return launch_update_big_nk<9, AL, SDC>(u, E, nt, lds, st);
  }
  return false;
}

static bool launch_update_big(const UpdParams &u, int E, hipStream_t st) {
  const int nqf = u.d >> 2;
  const int nk = (nqf + UPD_NT - 1) / UPD_NT;
  if (nk <= UPD_QMAX || nk > UPD_QMAX_BIG || (u.flags & UPD_TUNE) || u.zA || u.zB || getenv("MILE_NO_UPD_BIG")) return false;
  return with_al_sdc(row_align(u), u.sdc, [&](auto al, auto sdc) { return launch_update_big_al<al, sdc>(u, E, nk, st); });
}

// Whether launch_update runs `u` as the k_update_fast mid-step kind, the one launch that can prefill the next launch's noise
// (u.nz_A / u.nz_B); for any other launch those fields are ignored.
static bool update_prefills(const UpdParams &u) {
  return upd_fast_d(u.d) && !u.sdc && upd_kind(u) == UPD_KIND_MID;
}

static void launch_update(const UpdParams &u, int E, hipStream_t st) {
  const int nqf = u.d >> 2;
  if (!upd_fast_d(u.d)) {
    if (nqf >= 1 && launch_update_big(u, E, st)) return;
    if ((u.d + 3) / 4 <= UPD_NT * UPD_QMAX) { k_update<true><<<E, UPD_NT, 0, st>>>(u); return; }
    if (u.upart && getenv("MILE_NO_UPD_SEG") == nullptr) {   // any d, all CUs: segments of UPD_SEG elements, sums -> chain + apply -> scalars
      const int nseg = (u.d + UPD_SEG - 1) / UPD_SEG;
      k_update_seg<1><<<dim3(nseg, E), UPD_NT, 0, st>>>(u, u.upart, nseg);
      k_update_seg<2><<<dim3(nseg, E), UPD_NT, 0, st>>>(u, u.upart, nseg);
      k_update_seg_scalars<<<(E + 255) / 256, 256, 0, st>>>(u, u.upart, nseg, E);
      return;
    }
    k_update<false><<<E, UPD_NT, 0, st>>>(u);
    return;
  }
  const int nk = (nqf + UPD_NT - 1) / UPD_NT;
  with_al_sdc(row_align(u), u.sdc, [&](auto al, auto sdc) { launch_update_al<al, sdc>(u, E, nk, st); });
}

// The F > 8 split kernels live in their own translation unit, built WITHOUT -amdgpu-mfma-vgpr-form: with that option
// hipcc 7.2's 'AMDGPU Rewrite AGPR-Copy-MFMA' pass crashes on the heavily spilling k_grad_w64<3,2,true> (mile_amd/_build.py).
hipError_t mile_launch_w64_split_fq2(int nh, const GradParams &gp, int E, hipStream_t st);
// The partition forms of k_grad_narrow: mile_narrow_part.hip.
hipError_t mile_launch_narrow_part(int nh, int th, int tf, int nw, const GradParams &gp, int E, hipStream_t st);

template <int NH, int FQ, bool SPLIT = false>
static hipError_t launch_w64(const GradParams &gp, const W64Fuse &fz, int E, hipStream_t st) {
  using LY = W64Layout<NH, FQ, SPLIT>;
  hipError_t e = mile_set_max_lds<k_grad_w64<NH, FQ, SPLIT>>(LY::BYTES);
  if (e != hipSuccess) return e;
  if constexpr (W64FuseArg<FQ, SPLIT>::FUSABLE) {
    k_grad_w64<NH, FQ, SPLIT><<<dim3(gp.S, E), 256, LY::BYTES, st>>>(gp, fz);
  } else {
    if (fz.enabled) return hipErrorInvalidValue;
    k_grad_w64<NH, FQ, SPLIT><<<dim3(gp.S, E), 256, LY::BYTES, st>>>(gp, W64NoFuse{0});
  }
  return hipGetLastError();
}

// Can the update that follows this gradient run as the grad launch's epilogue (k_grad_w64 SPLIT, W64Fuse)?
// 8-byte aligned rows everywhere (the epilogue is the AL = 2 form), no preconditioner, d within its register cache.
static bool fuse_ok(const mile_sampler *s, int kernel, const UpdParams &u) {
  if (!MILE_W64_EPILOGUE_ON || !grad_kernel(kernel).fuses || s->part) return false;   // (partition: a gather sits in between)
  if (u.sdc || u.u_rec) return false;   // (the merged warm-up launch exists as a stand-alone kernel only)
  const int nh = s->spec.n_layers - 1, fq = s->Fp / 8;
  if (fq != 1) return false;                       // the F > 8 kernels are built without the epilogue (mile_grad_w64.h)
  const int nk = nh == 2 ? w64_fuse_nk<2, 1>() : w64_fuse_nk<3, 1>();
  return (u.d >> 2) <= 256 * nk && row_align(u) >= 2;
}

template <int NH, int TH, int TF>
static hipError_t launch_narrow_t(const GradParams &gp, int E, int nw, hipStream_t st) {
  constexpr bool WL = TH >= 3;
  using LY = NarrowLayout<NH, TH, TF, WL>;
  if constexpr (WL) {
    hipError_t e = mile_set_max_lds<k_grad_narrow<NH, TH, TF, WL>>(LY::BYTES);
    if (e != hipSuccess) return e;
  }
  k_grad_narrow<NH, TH, TF, WL><<<dim3(gp.S, E), 64 * nw, LY::BYTES, st>>>(gp);
  return hipGetLastError();
}
static hipError_t launch_narrow(const mile_sampler *s, const GradParams &gp, int E, hipStream_t st) {
  const int nh = s->spec.n_layers - 1;
  const int th = narrow_tiles_hidden(s->spec), tf = s->spec.in_features <= 16 ? 1 : 4;
  const int nw = th >= 3 ? NRW_MAXW : narrow_waves(s, gp.S, gp.N);
  if (gp.part_frozen) return mile_launch_narrow_part(nh, th, tf, nw, gp, E, st);
#define MILE_NRW(NH_, TH_, TF_) if (nh == NH_ && th == TH_ && tf == TF_) return launch_narrow_t<NH_, TH_, TF_>(gp, E, nw, st);
  MILE_NRW(1, 1, 1) MILE_NRW(1, 2, 1) MILE_NRW(1, 1, 4) MILE_NRW(1, 2, 4)
  MILE_NRW(2, 1, 1) MILE_NRW(2, 2, 1) MILE_NRW(2, 1, 4) MILE_NRW(2, 2, 4)
  MILE_NRW(3, 1, 1) MILE_NRW(3, 2, 1) MILE_NRW(3, 1, 4) MILE_NRW(3, 2, 4)
  MILE_NRW(4, 1, 1) MILE_NRW(5, 1, 1) MILE_NRW(6, 1, 1) MILE_NRW(7, 1, 1) MILE_NRW(8, 1, 1) MILE_NRW(9, 1, 1) MILE_NRW(10, 1, 1)
  MILE_NRW(1, 3, 1) MILE_NRW(1, 4, 1) MILE_NRW(1, 3, 4) MILE_NRW(1, 4, 4)      // hidden widths 33..64: weights in LDS
  MILE_NRW(2, 3, 1) MILE_NRW(2, 4, 1) MILE_NRW(2, 3, 4) MILE_NRW(2, 4, 4)
  MILE_NRW(3, 3, 1) MILE_NRW(3, 4, 1) MILE_NRW(3, 3, 4) MILE_NRW(3, 4, 4)
#undef MILE_NRW
  return hipErrorInvalidValue;
}

template <int NH>
static hipError_t launch_w128b(const GradParams &gp, int E, hipStream_t st) {
  using LY = W128Layout<NH, 2>;
  hipError_t e = mile_set_max_lds<k_grad_w128b<NH, 2>>(LY::BYTES);
  if (e != hipSuccess) return e;
  k_grad_w128b<NH, 2><<<dim3(gp.S, E), 256, LY::BYTES, st>>>(gp);
  return hipGetLastError();
}

__global__ void k_fill(float *p, float v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// An operand of the layer-wise paths: (pointer, batch stride, leading dimension), in floats
struct MMIn { const float *p; long long s; int ld; };
struct MMOut { float *p; long long s; int ld; operator MMIn() const { return {p, s, ld}; } };
// The row head of the layer-wise evaluations, on the outputs Z [batch][rows][ld] (O per row) of data rows r0 .. of N and samples
// s0 ..: the per-row log-likelihoods against y into out [.., N], or (y == nullptr: mile_predict) the raw outputs into out [.., N, O]
static void launch_rowll(MMIn Z, const void *y, int r0, int rows, int O, int task, float *out, long long N, long long s0, int batch, hipStream_t st) {
  if (y) k_rowll<<<dim3((unsigned)((rows + 255) / 256), batch), 256, 0, st>>>(Z.p, Z.s, Z.ld, y, r0, rows, O, task, out, N, s0);
  else k_rowll<true><<<dim3((unsigned)std::min<long long>(((long long)rows * O + 255) / 256, 65535), batch), 256, 0, st>>>(Z.p, Z.s, Z.ld, y, r0, rows, O, task, out, N, s0);
}

// LeNet: forward (+ backward when slab != nullptr) over image chunks; batch = particles (or samples).
// out_ll != nullptr: evaluation, per-row log-likelihoods out_ll[(s0 + e) * N + r]; otherwise the gradient goes
// to slab[e * dp + offset] and the log-likelihood sums to llacc[e].
// Dense half of LeNet on the hand-written MFMA GEMMs (k_mm3 with fp32-faithful three-term products; defined below the k_mm3
// launchers): LENET_BF16 / LENET_BF16X3 use no library kernel.  lenet_dense_prep once per gradient, lenet_dense_chunk per image chunk.
struct LeNetDenseBufs { const float *p2; float *f1, *f2, *out, *df2, *df1, *dp2; };
static int lenet_dense_prep(mile_sampler *s, const float *theta, int E, hipStream_t st);
static int lenet_dense_chunk(mile_sampler *s, const float *theta, int E, int Rc, int r0, int chunk, const LeNetDenseBufs &b, const void *y,
                             float *slab, long long dp, float *llacc, float *out_ll, long long Ntot, long long s0, hipStream_t st);

// the convolution products: fp32 VALU kernels (mile_lenet.h) / bf16-rounded operands on the matrix pipe / exact three-term
// bf16 splits of both operands and six MFMA products (fp32-faithful), mile_lenet_mfma.h
enum { LENET_CONV_F32 = 0, LENET_CONV_BF16 = 1, LENET_CONV_BF16X3 = 2 };
// images per barrier pair of the MFMA convolution kernels: as many as keep the tiles (all term planes) under ~56 KB, at most 4
static int lenet_ni_for(size_t per_img, int terms) { return std::max(1, std::min(4, (int)(57344 / (terms * per_img)))); }
static int run_lenet(mile_sampler *s, const float *theta, int E, const float *X, const void *y, int N, float *slab, long long dp,
                     float *llacc, float *out_ll, long long s0, hipStream_t st, int mode = LENET_CONV_F32) {
  const bool mfma = mode != LENET_CONV_F32, x3 = mode == LENET_CONV_BF16X3;
  if (const int rc = rocblas_ready(s, st)) return rc;
  const LeNetGeom &g = s->lg;
  const int d = g.d, act = s->ds.activation, task = s->ds.task;
  const bool grad = slab != nullptr;
  const size_t HW = (size_t)g.H * g.W, P1 = (size_t)g.hp1 * g.wp1, HW2 = (size_t)g.h2 * g.w2;
  const size_t n_a1 = 6 * HW, n_p1 = 6 * P1, n_col2 = 150 * HW2, n_a2 = 16 * HW2, n_p2 = g.flat;
  // direct convolution kernels (LDS tiles per image) unless the image is too large for them or the im2col + SGEMM
  // form is asked for (MILE_LENET_GEMM=1: kept as the second implementation / fallback)
  const int ipw = mfma ? 16 : 8;   // images per workgroup (measured: 53.0 / 54.7 ms at 16 / 8 on the MFMA forms)
  const size_t lds_f1 = (size_t)(25 * g.C * 8 + 8 + g.C * (g.H + 4) * (g.W + 4)) * 4;
  const int KT1 = 25 * g.C;
  // k_conv5_dw: pixel groups are reduced 3 at a time through LDS (buffer aliases the tiles)
  const size_t lds_w1 = std::max((size_t)(g.C * (g.H + 4) * (g.W + 4)) + HW * 6, 3 * (size_t)(KT1 * 6 + 6)) * 4;
  const size_t lds_f2 = (size_t)(150 * 16 + 16 + 6 * P1) * 4, lds_x2 = (size_t)(2400 + 1 * (g.h2 + 8) * (g.w2 + 8) * 16) * 4;   // 2 images' dZ per pass: two workgroups per CU
  const size_t lds_w2 = std::max(6 * P1 + HW2 * 16, 3 * (size_t)(2400 + 16)) * 4;
  const size_t lds_max = std::max({lds_f1, lds_w1, lds_f2, lds_x2, lds_w2});
  // compile-time geometry for CIFAR- / MNIST-sized inputs (their LDS needs are below the 64 KiB default limit)
  const int geo = (g.C == 3 && g.H == 32 && g.W == 32) ? 1 : (g.C == 1 && g.H == 28 && g.W == 28) ? 3 : 0;
  const bool direct = getenv("MILE_LENET_GEMM") == nullptr && g.C <= 16 && lds_max <= 150 * 1024;
  // MILE_GRAD_LENET_BF16: the five convolution launches on the bf16 matrix pipe (mile_lenet_mfma.h), everything else as below
  // small images: several per barrier pair (as many as keep the tiles under ~56 KB, at most 4)
  const int terms = x3 ? 3 : 1;   // LENET_BF16X3: every tile once per term plane, so fewer images per barrier pair
  const auto ni_for = [terms](size_t per_img) { return lenet_ni_for(per_img, terms); };
  const int ni2 = ni_for((size_t)(g.hp1 * g.wp1 + 8) * 16 + (size_t)g.h2 * g.w2 * 32);   // input tile + dZ rows of one image
  const int ni_x2 = ni_for((size_t)((g.h2 + 8) * (g.w2 + 8) + 8) * 32), ni_f1 = ni_for((size_t)((g.H + 4) * (g.W + 4) + 8) * 8);
  // the 6-channel sides of the two convolutions in the PAIR forms (two pixels per MFMA row / column)
  const size_t ldm_f1p = cm_lds_fwd(CM_IN4, g.H, g.W, 2, g.C, 6, ni_f1, terms), ldm_f2 = cm_lds_fwd(CM_IN8, g.hp1, g.wp1, 0, 6, 16, ni2, terms);
  const size_t ldm_x2p = cm_lds_dx2x(g.h2, g.w2, 6, 16, ni_x2, terms), ldm_w1p = cm_lds_dw2x(g.H, g.W, 2, terms);
  const size_t ldm_w2 = cm_lds_dw(CM_IN8, g.hp1, g.wp1, 0, ni2, terms);
  // ldm_w1 (conv1's kernel gradient in the pixel form, no longer built) exceeds ldm_w1p: kept in the check so that the same
  // images are refused as when the pixel forms could be selected.  Their other two sizes never exceed ldm_f1p and ldm_x2p.
  const size_t ldm_w1 = cm_lds_dw(CM_IN4, g.H, g.W, 2);
  // ReLU: the full-size conv activations are kept for the backward pass only as two-byte "was it positive" values
  const int a16 = mfma && act == MILE_ACT_RELU;
  if (mfma && (!direct || g.C > 4 || std::max({ldm_f1p, ldm_f2, ldm_x2p, ldm_w1, ldm_w1p, ldm_w2}) > 150 * 1024))
    return fail(MILE_ERR_INVALID, x3 ? "LENET_BF16X3 needs <= 4 image channels and an image whose three term planes fit the LDS tiles"
                                     : "LENET_BF16 needs <= 4 image channels and an image that fits the LDS tiles");
  // Dense activations: exact widths on the rocBLAS path; k_mm3 wants rows of 8 k floats (zero padding columns)
  const size_t w_f2 = mfma ? 88 : 84, w_out = mfma ? (size_t)(g.K + 7) / 8 * 8 : (size_t)g.K;
  size_t per = n_a1 + n_p1 + (direct ? 0 : n_col2) + n_a2 + n_p2 + 120 + w_f2 + w_out;
  if (grad) per += w_f2 + 120 + n_p2 + n_p1 + (direct ? 0 : n_a2 + n_a1);
  const size_t shared = direct ? 0 : 25 * (size_t)g.C * HW;
  size_t R = ((size_t)1 << 30) / ((size_t)E * per + shared);
  R = std::max<size_t>(1, std::min<size_t>(R, (size_t)N));
  R = gemm_rows_hook(R, (size_t)N);
  const size_t nwg_max = (R + ipw - 1) / ipw;
  const size_t n_part1 = direct && grad ? (size_t)E * nwg_max * (25 * g.C * 6 + 6) : 0;
  const size_t n_part2 = direct && grad ? (size_t)E * nwg_max * (2400 + 16) : 0;
  const size_t need = R * ((size_t)E * per + shared) + n_part1 + n_part2 + 128;   // + the arrays' alignment padding
  HIP_TRY(grow(s->gemm_ws, s->gemm_ws_floats, need, 4));
  s->gemm_E = 0;
  const size_t n_ones = R * HW;
  if ((size_t)s->gemm_ones_n < n_ones) {
    HIP_TRY(grow(s->gemm_ones, s->gemm_ones_n, n_ones, 4));
    k_fill<<<(unsigned)((n_ones + 255) / 256), 256, 0, st>>>(s->gemm_ones, 1.0f, (int)n_ones);
  }
  const size_t ER = (size_t)E * R;
  float *q = s->gemm_ws;
  auto take = [&](size_t n) { float *r = q; q += (n + 3) / 4 * 4; return r; };   // every array 16-byte aligned (vector loads in the conv kernels)
  float *col1 = take(R * shared), *a1 = take(ER * n_a1), *p1 = take(ER * n_p1), *col2 = take(direct ? 0 : ER * n_col2), *a2 = take(ER * n_a2);
  float *p2 = take(ER * n_p2), *f1 = take(ER * 120), *f2 = take(ER * w_f2), *out = take(ER * w_out);
  float *df2 = nullptr, *df1 = nullptr, *dp2 = nullptr, *dz2 = nullptr, *dp1 = nullptr, *dz1 = nullptr;
  if (grad) { df2 = take(ER * w_f2); df1 = take(ER * 120); dp2 = take(ER * n_p2); dz2 = take(direct ? 0 : ER * n_a2); dp1 = take(ER * n_p1); dz1 = take(direct ? 0 : ER * n_a1); }
  float *part1 = take(n_part1), *part2 = take(n_part2);
  if (direct) {
    HIP_TRY((mile_set_max_lds<k_conv5_fwd<6, 0>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5_fwd<16, 0>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5_dw<6, 0>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5_dw<16, 0>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5_dx<6, 16, 1, 0, 0>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_fwd<CM_IN8, 16>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_dw<CM_IN8, 16>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_fwd2x<6>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_dx2x<6, 16>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_dw2x<6>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_fwd<CM_IN8, 16, 3>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_dw<CM_IN8, 16, 3>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_fwd2x<6, 3>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_dx2x<6, 16, 3>>(150 * 1024)));
    HIP_TRY((mile_set_max_lds<k_conv5m_dw2x<6, 3>>(150 * 1024)));
  }
  const float one = 1.0f, zero = 0.0f;
  auto blocks = [](long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 65535); };
  // row-major C[rows x fout] = A[rows x fin] W[fin x fout] per batch entry; W from theta (+ offset), batch stride d
  auto fwd = [&](int w_off, int fin, int fout, const float *in, long long sin, long long rows, float *o) {
    return g_rb.sgemm_sb(s->blas, RB_OP_N, RB_OP_N, fout, (int)rows, fin, &one, theta + w_off, fout, d, in, fin, sin, &zero, o, fout,
                         rows * fout, E);
  };
  auto bias_act = [&](float *z, int b_off, int W, long long rows, int apply) {
    k_gemm_bias_act<<<dim3(blocks(rows * W), E), 256, 0, st>>>(z, theta, b_off, d, W, rows * W, act, apply);
  };
  if (mfma) {   // padding columns of the Dense activations are read as operands: zero them (never written afterwards)
    HIP_TRY(hipMemsetAsync(f1, 0, (ER * 120 + 4 + ER * w_f2 + 4 + ER * w_out) * 4, st));
    if (grad) HIP_TRY(hipMemsetAsync(df2, 0, (ER * w_f2 + 4 + ER * 120) * 4, st));
    const int rc = lenet_dense_prep(s, theta, E, st);
    if (rc) return rc;
  }
  for (int r0 = 0, chunk = 0; r0 < N; r0 += (int)R, ++chunk) {
    const long long Rc = std::min<long long>((long long)R, N - r0), B = (long long)E * Rc;
    const long long M1 = Rc * (long long)HW, M2 = Rc * (long long)HW2;
    // ---- forward
    const float *Xc = X + (size_t)r0 * g.C * HW;
    const unsigned nwg = (unsigned)((Rc + ipw - 1) / ipw);
    if (direct) {
#define LAUNCH_FWD1(GEO_) k_conv5_fwd<6, GEO_><<<dim3(nwg, E), 256, lds_f1, st>>>(Xc, 0, (long long)g.C * HW, g.W, 1, (long long)HW, g.C, g.H, g.W, 2, theta, g.k_c1, g.b_c1, d, a1, (int)Rc, ipw, act)
#define LAUNCH_FWD2(GEO_) k_conv5_fwd<16, GEO_><<<dim3(nwg, E), 256, lds_f2, st>>>(p1, Rc * (long long)n_p1, (long long)n_p1, g.wp1 * 6, 6, 1, 6, g.hp1, g.wp1, 0, theta, g.k_c2, g.b_c2, d, a2, (int)Rc, ipw, act)
      // MFMA form: the pooled activations come out of the convolution's own epilogue; evaluation skips the full-size ones
      if (x3) k_conv5m_fwd2x<6, 3><<<dim3(nwg, E), 256, ldm_f1p, st>>>(Xc, 0, (long long)g.C * HW, g.W, 1, (long long)HW, g.C, g.H, g.W, 2, theta, g.k_c1, g.b_c1, d, grad ? a1 : nullptr, p1, (int)Rc, ipw, act, a16, ni_f1);
      else if (mfma) k_conv5m_fwd2x<6><<<dim3(nwg, E), 256, ldm_f1p, st>>>(Xc, 0, (long long)g.C * HW, g.W, 1, (long long)HW, g.C, g.H, g.W, 2, theta, g.k_c1, g.b_c1, d, grad ? a1 : nullptr, p1, (int)Rc, ipw, act, a16, ni_f1);
      else if (geo == 1) LAUNCH_FWD1(1); else if (geo == 3) LAUNCH_FWD1(3); else LAUNCH_FWD1(0);
      if (!mfma) k_avgpool2<<<blocks(B * (long long)n_p1), 256, 0, st>>>(a1, p1, B, g.H, g.W, 6);
      if (x3) k_conv5m_fwd<CM_IN8, 16, 3><<<dim3(nwg, E), 256, ldm_f2, st>>>(p1, Rc * (long long)n_p1, (long long)n_p1, g.wp1 * 6, 6, 1, 6, g.hp1, g.wp1, 0, theta, g.k_c2, g.b_c2, d, grad ? a2 : nullptr, p2, (int)Rc, ipw, act, a16, ni2);
      else if (mfma) k_conv5m_fwd<CM_IN8, 16><<<dim3(nwg, E), 256, ldm_f2, st>>>(p1, Rc * (long long)n_p1, (long long)n_p1, g.wp1 * 6, 6, 1, 6, g.hp1, g.wp1, 0, theta, g.k_c2, g.b_c2, d, grad ? a2 : nullptr, p2, (int)Rc, ipw, act, a16, ni2);
      else if (geo == 1) LAUNCH_FWD2(2); else if (geo == 3) LAUNCH_FWD2(4); else LAUNCH_FWD2(0);
#undef LAUNCH_FWD1
#undef LAUNCH_FWD2
    } else {
      k_im2col5<<<blocks(M1 * 25 * g.C), 256, 0, st>>>(Xc, col1, Rc, g.H, g.W, g.C, g.H, g.W, 2, (long long)g.C * HW, g.W, 1, (long long)HW);
      if (fwd(g.k_c1, 25 * g.C, 6, col1, 0, M1, a1)) return fail(MILE_ERR_HIP, "rocblas sgemm (conv1) failed");
      bias_act(a1, g.b_c1, 6, M1, 1);
      k_avgpool2<<<blocks(B * (long long)n_p1), 256, 0, st>>>(a1, p1, B, g.H, g.W, 6);
      k_im2col5<<<blocks(B * (long long)n_col2), 256, 0, st>>>(p1, col2, B, g.hp1, g.wp1, 6, g.h2, g.w2, 0, (long long)n_p1, g.wp1 * 6, 6, 1);
      if (fwd(g.k_c2, 150, 16, col2, M2 * 150, M2, a2)) return fail(MILE_ERR_HIP, "rocblas sgemm (conv2) failed");
      bias_act(a2, g.b_c2, 16, M2, 1);
    }
    if (!mfma) k_avgpool2<<<blocks(B * (long long)n_p2), 256, 0, st>>>(a2, p2, B, g.h2, g.w2, 16);
    if (mfma) {   // Dense layers, head and their backward pass on k_mm3; leaves dp2 for the convolution backward pass below
      const LeNetDenseBufs db{p2, f1, f2, out, df2, df1, dp2};
      const int rc = lenet_dense_chunk(s, theta, E, (int)Rc, r0, chunk, db, y, slab, dp, llacc, out_ll, N, s0, st);
      if (rc) return rc;
      if (!grad) continue;
    } else {
      if (fwd(g.k_f1, g.flat, 120, p2, Rc * g.flat, Rc, f1)) return fail(MILE_ERR_HIP, "rocblas sgemm (fc1) failed");
      bias_act(f1, g.b_f1, 120, Rc, 1);
      if (fwd(g.k_f2, 120, 84, f1, Rc * 120, Rc, f2)) return fail(MILE_ERR_HIP, "rocblas sgemm (fc2) failed");
      bias_act(f2, g.b_f2, 84, Rc, 1);
      if (fwd(g.k_f3, 84, g.K, f2, Rc * 84, Rc, out)) return fail(MILE_ERR_HIP, "rocblas sgemm (fc3) failed");
      bias_act(out, g.b_f3, g.K, Rc, 0);
      if (!grad) {   // per-row log-likelihoods, or (y == nullptr: mile_predict) the raw outputs [.., N, K]
        launch_rowll({out, Rc * g.K, g.K}, y, r0, (int)Rc, g.K, task, out_ll, N, s0, E, st);
        continue;
      }
      k_gemm_head<<<E, 256, 0, st>>>(out, y, r0, (int)Rc, g.K, task, llacc, chunk == 0);
    }
    // ---- backward
    const float *beta = chunk == 0 ? &zero : &one;
    // dW[fin x fout] (+)= in^T dz into the slab; bias gradient = dz^T 1
    auto dW = [&](int w_off, int b_off, int fin, int fout, const float *in, long long sin, const float *dz, long long rows) -> int {
      if (g_rb.sgemm_sb(s->blas, RB_OP_N, RB_OP_T, fout, fin, (int)rows, &one, dz, fout, rows * fout, in, fin, sin, beta, slab + w_off, fout,
                        dp, E))
        return 1;
      return g_rb.sgemm_sb(s->blas, RB_OP_N, RB_OP_N, fout, 1, (int)rows, &one, dz, fout, rows * fout, s->gemm_ones, (int)rows, 0, beta,
                           slab + b_off, fout, dp, E);
    };
    // dX[rows x fin] = dz[rows x fout] W^T
    auto dX = [&](int w_off, int fin, int fout, const float *dz, long long rows, float *o) {
      return g_rb.sgemm_sb(s->blas, RB_OP_T, RB_OP_N, fin, (int)rows, fout, &one, theta + w_off, fout, d, dz, fout, rows * fout, &zero, o, fin,
                           rows * fin, E);
    };
    auto act_grad = [&](float *dh, const float *h, long long n) {
      k_gemm_act_grad<<<dim3(blocks(n), E), 256, 0, st>>>(dh, h, n, act);
    };
    if (!mfma) {
      if (dW(g.k_f3, g.b_f3, 84, g.K, f2, Rc * 84, out, Rc)) return fail(MILE_ERR_HIP, "rocblas sgemm (d fc3) failed");
      if (dX(g.k_f3, 84, g.K, out, Rc, df2)) return fail(MILE_ERR_HIP, "rocblas sgemm (d fc3 in) failed");
      act_grad(df2, f2, Rc * 84);
      if (dW(g.k_f2, g.b_f2, 120, 84, f1, Rc * 120, df2, Rc)) return fail(MILE_ERR_HIP, "rocblas sgemm (d fc2) failed");
      if (dX(g.k_f2, 120, 84, df2, Rc, df1)) return fail(MILE_ERR_HIP, "rocblas sgemm (d fc2 in) failed");
      act_grad(df1, f1, Rc * 120);
      if (dW(g.k_f1, g.b_f1, g.flat, 120, p2, Rc * g.flat, df1, Rc)) return fail(MILE_ERR_HIP, "rocblas sgemm (d fc1) failed");
      if (dX(g.k_f1, g.flat, 120, df1, Rc, dp2)) return fail(MILE_ERR_HIP, "rocblas sgemm (d fc1 in) failed");
    }
    if (!direct) k_unpool_actgrad<<<blocks(B * (long long)n_a2), 256, 0, st>>>(dp2, a2, dz2, B, g.h2, g.w2, 16, act);
    if (direct) {   // dZ = unpool(dP) * act'(A) is formed inside the kernels' tile loads: no dz2 / dz1 arrays
      const int acc = chunk != 0;
#define LAUNCH_DW2(GEO_) k_conv5_dw<16, GEO_><<<dim3(nwg, E), 256, lds_w2, st>>>(p1, Rc * (long long)n_p1, (long long)n_p1, g.wp1 * 6, 6, 1, 6, g.hp1, g.wp1, 0, dp2, a2, act, part2, (int)Rc, ipw)
#define LAUNCH_DX(HO_, WO_) k_conv5_dx<6, 16, 1, HO_, WO_><<<dim3(nwg, E), 256, lds_x2, st>>>(dp2, a2, act, theta, g.k_c2, d, dp1, (int)Rc, g.h2, g.w2, ipw)
#define LAUNCH_DW1(GEO_) k_conv5_dw<6, GEO_><<<dim3(nwg, E), 256, lds_w1, st>>>(Xc, 0, (long long)g.C * HW, g.W, 1, (long long)HW, g.C, g.H, g.W, 2, dp1, a1, act, part1, (int)Rc, ipw)
      if (x3) k_conv5m_dw<CM_IN8, 16, 3><<<dim3(nwg, E), 256, ldm_w2, st>>>(p1, Rc * (long long)n_p1, (long long)n_p1, g.wp1 * 6, 6, 1, 6, g.hp1, g.wp1, 0, dp2, a2, act, part2, (int)Rc, ipw, a16, ni2);
      else if (mfma) k_conv5m_dw<CM_IN8, 16><<<dim3(nwg, E), 256, ldm_w2, st>>>(p1, Rc * (long long)n_p1, (long long)n_p1, g.wp1 * 6, 6, 1, 6, g.hp1, g.wp1, 0, dp2, a2, act, part2, (int)Rc, ipw, a16, ni2);
      else if (geo == 1) LAUNCH_DW2(2); else if (geo == 3) LAUNCH_DW2(4); else LAUNCH_DW2(0);
      k_conv_reduce<<<dim3(10, E), 256, 0, st>>>(part2, (int)nwg, 2400, 16, slab, dp, g.k_c2, g.b_c2, acc);
      if (x3) k_conv5m_dx2x<6, 16, 3><<<dim3(nwg, E), 256, ldm_x2p, st>>>(dp2, a2, act, theta, g.k_c2, d, dp1, (int)Rc, g.h2, g.w2, ipw, a16, ni_x2);
      else if (mfma) k_conv5m_dx2x<6, 16><<<dim3(nwg, E), 256, ldm_x2p, st>>>(dp2, a2, act, theta, g.k_c2, d, dp1, (int)Rc, g.h2, g.w2, ipw, a16, ni_x2);
      else if (geo == 1) LAUNCH_DX(12, 12); else if (geo == 3) LAUNCH_DX(10, 10); else LAUNCH_DX(0, 0);
      if (x3) k_conv5m_dw2x<6, 3><<<dim3(nwg, E), 256, ldm_w1p, st>>>(Xc, 0, (long long)g.C * HW, g.W, 1, (long long)HW, g.C, g.H, g.W, 2, dp1, a1, act, part1, (int)Rc, ipw, a16);
      else if (mfma) k_conv5m_dw2x<6><<<dim3(nwg, E), 256, ldm_w1p, st>>>(Xc, 0, (long long)g.C * HW, g.W, 1, (long long)HW, g.C, g.H, g.W, 2, dp1, a1, act, part1, (int)Rc, ipw, a16);
      else if (geo == 1) LAUNCH_DW1(1); else if (geo == 3) LAUNCH_DW1(3); else LAUNCH_DW1(0);
#undef LAUNCH_DW2
#undef LAUNCH_DX
#undef LAUNCH_DW1
      k_conv_reduce<<<dim3(2, E), 256, 0, st>>>(part1, (int)nwg, KT1 * 6, 6, slab, dp, g.k_c1, g.b_c1, acc);
    } else {
      if (dW(g.k_c2, g.b_c2, 150, 16, col2, M2 * 150, dz2, M2)) return fail(MILE_ERR_HIP, "rocblas sgemm (d conv2) failed");
      if (dX(g.k_c2, 150, 16, dz2, M2, col2)) return fail(MILE_ERR_HIP, "rocblas sgemm (d conv2 in) failed");   // d(col2) over col2
      k_col2im5<<<blocks(B * (long long)n_p1), 256, 0, st>>>(col2, dp1, B, g.h2, g.w2, 6);
      k_unpool_actgrad<<<blocks(B * (long long)n_a1), 256, 0, st>>>(dp1, a1, dz1, B, g.H, g.W, 6, act);
      if (dW(g.k_c1, g.b_c1, 25 * g.C, 6, col1, 0, dz1, M1)) return fail(MILE_ERR_HIP, "rocblas sgemm (d conv1) failed");
    }
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

// Layer-wise path: per row chunk, forward GEMM + bias/activation per layer, head, then per layer
// dW (accumulated in place in the slab), bias column sums, dH GEMM + activation derivative.
// Row-major products through rocBLAS's column-major interface: C = A B  <=>  C^T = B^T A^T.
static int launch_grad_gemm(mile_sampler *s, const GradParams &gp, int E, hipStream_t st) {
  if (const int rc = rocblas_ready(s, st)) return rc;
  const DevSpec &ds = s->ds;
  const int L = ds.n_layers, F = ds.in_features, d = ds.d, N = s->N;
  size_t per_row = 2 * (size_t)ds.max_width;
  for (int l = 0; l < L; ++l) per_row += ds.widths[l];
  if (E != s->gemm_E || !s->gemm_ws) {   // (re)size the activation workspace: <= ~4 GiB, whole data set if it fits
    const size_t budget = (size_t)1 << 30;   // floats
    size_t R = budget / ((size_t)E * per_row);
    R = std::min<size_t>(R, (size_t)N);
    if (R < (size_t)N) R = std::max<size_t>(256, R / 256 * 256);
    R = std::min<size_t>(R, (size_t)N);
    R = gemm_rows_hook(R, (size_t)N);
    const size_t need = (size_t)E * R * per_row;
    HIP_TRY(grow(s->gemm_ws, s->gemm_ws_floats, need, 4));
    s->gemm_R = (int)R; s->gemm_E = E;
  }
  const int R = s->gemm_R;
  if (s->gemm_ones_n < R) {   // ones[R]: bias gradients are dZ^T 1 (a skinny GEMM, memory bound like the sum it replaces)
    HIP_TRY(grow(s->gemm_ones, s->gemm_ones_n, (size_t)R, 4));
    k_fill<<<(R + 255) / 256, 256, 0, st>>>(s->gemm_ones, 1.0f, R);
  }
  float *H[MILE_MAX_LAYERS], *tmp[2];
  {
    float *q = s->gemm_ws;
    for (int l = 0; l < L; ++l) { H[l] = q; q += (size_t)E * R * ds.widths[l]; }
    tmp[0] = q; q += (size_t)E * R * ds.max_width;
    tmp[1] = q;
  }
  const float one = 1.0f, zero = 0.0f;
  float *slab = gp.slabs;        // S = 1: [E][dp]
  const long long dp = gp.dp;
  auto gemm = [&](int ta, int tb, int m, int n, int k, const float *A, int lda, long long sa, const float *B, int ldb, long long sb,
                  const float *beta, float *C, int ldc, long long sc) -> int {
    return g_rb.sgemm_sb(s->blas, ta, tb, m, n, k, &one, A, lda, sa, B, ldb, sb, beta, C, ldc, sc, E);
  };
  auto blocks = [](long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 4096); };
  for (int r0 = 0, chunk = 0; r0 < N; r0 += R, ++chunk) {
    const int Rc = std::min(R, N - r0);
    // ---- forward
    for (int l = 0; l < L; ++l) {
      const int fin = l == 0 ? F : ds.widths[l - 1], fout = ds.widths[l];
      const float *in = l == 0 ? gp.X + (size_t)r0 * F : H[l - 1];
      const long long sin = l == 0 ? 0 : (long long)Rc * fin;
      if (gemm(RB_OP_N, RB_OP_N, fout, Rc, fin, gp.theta + ds.w_off[l], fout, d, in, fin, sin, &zero, H[l], fout, (long long)Rc * fout))
        return fail(MILE_ERR_HIP, "rocblas sgemm (forward) failed");
      const long long RW = (long long)Rc * fout;
      k_gemm_bias_act<<<dim3(blocks(RW), E), 256, 0, st>>>(H[l], gp.theta, ds.b_off[l], d, fout, RW, ds.activation, l + 1 < L);
    }
    // ---- head: log-likelihood and d(out), in place
    k_gemm_head<<<E, 256, 0, st>>>(H[L - 1], gp.y, r0, Rc, ds.widths[L - 1], ds.task, gp.llpart, chunk == 0);
    // ---- backward
    float *dz = H[L - 1];
    int pp = 0;
    const float *beta = chunk == 0 ? &zero : &one;
    for (int l = L - 1; l >= 0; --l) {
      const int fin = l == 0 ? F : ds.widths[l - 1], fout = ds.widths[l];
      const float *in = l == 0 ? gp.X + (size_t)r0 * F : H[l - 1];
      const long long sin = l == 0 ? 0 : (long long)Rc * fin;
      // dW[in][out] (+)= in^T dz, written straight into the slab at the kernel's offset
      if (gemm(RB_OP_N, RB_OP_T, fout, fin, Rc, dz, fout, (long long)Rc * fout, in, fin, sin, beta, slab + ds.w_off[l], fout, dp))
        return fail(MILE_ERR_HIP, "rocblas sgemm (dW) failed");
      if (gemm(RB_OP_N, RB_OP_N, fout, 1, Rc, dz, fout, (long long)Rc * fout, s->gemm_ones, Rc, 0, beta, slab + ds.b_off[l], fout, dp))
        return fail(MILE_ERR_HIP, "rocblas sgemm (bias gradient) failed");
      if (l > 0) {
        if (gemm(RB_OP_T, RB_OP_N, fin, Rc, fout, gp.theta + ds.w_off[l], fout, d, dz, fout, (long long)Rc * fout, &zero, tmp[pp], fin,
                 (long long)Rc * fin))
          return fail(MILE_ERR_HIP, "rocblas sgemm (dH) failed");
        const long long RW = (long long)Rc * fin;
        k_gemm_act_grad<<<dim3(blocks(RW), E), 256, 0, st>>>(tmp[pp], H[l - 1], RW, ds.activation);
        dz = tmp[pp];
        pp ^= 1;
      }
    }
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

static int launch_grad(mile_sampler *s, const float *theta, int E, hipStream_t st, const UpdParams *fused_update = nullptr,
                       bool full_layout = false);

// ------------------------------------------------------------------------------------
// Layer-wise MFMA path (MILE_GRAD_MFMA_WIDE_BF16X3 / _BF16): mile_mm3.h.  Per row chunk: forward GEMM per layer with bias +
// activation in its epilogue, head, then per layer dW (K = the chunk's rows, accumulated in place in the slab), bias
// column sums, and the dH GEMM with the activation derivative in its epilogue.
// ------------------------------------------------------------------------------------
#ifndef MILE_MM_KC
#define MILE_MM_KC 32     // K chunk of k_mm3: 32 = two workgroups per CU (mile_mm3.h); 64 = one, measured slower
#endif
template <int ALAY, int BSRC, int EPI, int TERMS, int ACT, bool ACCUM, bool COLSUM, bool FULL = false>
static hipError_t launch_mm3_k(const MMParams &p, int batch, hipStream_t st) {
  constexpr int KC = MILE_MM_KC;
  using LY = MMLayout<ALAY, BSRC, TERMS, KC>;
  if constexpr (!FULL) {   // whole tiles everywhere: the predicate-free instantiation
    if (p.M % 128 == 0 && p.N % 128 == 0)
      return launch_mm3_k<ALAY, BSRC, EPI, TERMS, ACT, ACCUM, COLSUM, true>(p, batch, st);
  }
  hipError_t e = mile_set_max_lds<k_mm3<ALAY, BSRC, EPI, TERMS, KC, ACT, ACCUM, COLSUM, FULL>>(LY::BYTES);
  if (e != hipSuccess) return e;
  MMParams q = p;
  const int mtiles = (p.M + 127) / 128;
  const dim3 grid((p.N + 127) / 128, mtiles, batch);
  q.c_vec = (p.ldc % 4 == 0) && (p.sC % 4 == 0) && (((uintptr_t)p.C & 15) == 0);
  q.xcd_remap = 0;
  if (COLSUM && batch % 8 == 0) q.xcd_remap = 2;                     // dW: the few tiles of a particle share both operands
  else if (!COLSUM && grid.x > 1 && grid.y >= 8) q.xcd_remap = 1;
  k_mm3<ALAY, BSRC, EPI, TERMS, KC, ACT, ACCUM, COLSUM, FULL><<<grid, 256, LY::BYTES, st>>>(q);
  return hipGetLastError();
}
// the three products of the layer-wise path, dispatched on the launch constants the kernel takes as template parameters
template <int TERMS>
static hipError_t launch_mm3_fwd(const MMParams &p, int batch, hipStream_t st) {
  const int act = p.apply_act ? p.act : -1;
#define MILE_MM_FWD(A_) launch_mm3_k<MM_A_MK, MM_B_T3_KN, MM_EPI_BIAS_ACT, TERMS, A_, false, false>(p, batch, st)
  return act == MILE_ACT_RELU ? MILE_MM_FWD(MILE_ACT_RELU) : act == MILE_ACT_TANH ? MILE_MM_FWD(MILE_ACT_TANH)
       : act == MILE_ACT_SIGMOID ? MILE_MM_FWD(MILE_ACT_SIGMOID) : MILE_MM_FWD(-1);
#undef MILE_MM_FWD
}
template <int TERMS>
static hipError_t launch_mm3_dh(const MMParams &p, int batch, hipStream_t st) {
#define MILE_MM_DH(A_) launch_mm3_k<MM_A_MK, MM_B_T3_NK, MM_EPI_ACT_GRAD, TERMS, A_, false, false>(p, batch, st)
  return p.act == MILE_ACT_RELU ? MILE_MM_DH(MILE_ACT_RELU) : p.act == MILE_ACT_TANH ? MILE_MM_DH(MILE_ACT_TANH) : MILE_MM_DH(MILE_ACT_SIGMOID);
#undef MILE_MM_DH
}
template <int TERMS>
static hipError_t launch_mm3_dw(const MMParams &p, int batch, hipStream_t st) {
  return p.accumulate ? launch_mm3_k<MM_A_KM, MM_B_F32_KN, MM_EPI_STORE, TERMS, -1, true, true>(p, batch, st)
                      : launch_mm3_k<MM_A_KM, MM_B_F32_KN, MM_EPI_STORE, TERMS, -1, false, true>(p, batch, st);
}

// ---- the MMParams of the three products of layer l of a LayerPlan (mile_layer_plan.h).  The plan owns the weights' term-plane
// format; the callers own their activations, each operand an MMIn / MMOut
struct LayerGemm {                 // what the products of one call share
  const LayerPlan &pl;
  const bf16 *Wt;                  // the batch's term planes, from wide_prep_weights
  const float *theta; int d;       // the batch's parameter rows (the biases) and their stride
  int act;
};
// the kernels of n parameter rows at stride d as zero-padded bf16 term planes Wt [n][layer][term][in][outp]
template <int TERMS>
static void wide_prep_weights(const LayerPlan &pl, const float *theta, int d, int n, bf16 *Wt, hipStream_t st) {
  for (int l = 0; l < pl.L; ++l)
    k_wide_prep_weights<TERMS><<<dim3((unsigned)std::min<long long>(((long long)pl.plane(l) + 255) / 256, 1024), n), 256, 0, st>>>(
        theta, d, pl.w_off[l], pl.fin[l], pl.fout[l], pl.wp[l], Wt + pl.wt_off[l], (long long)pl.wt_elems);
}
static void mm3_weights(const LayerGemm &g, int l, MMParams &p) {   // B = layer l's term planes, [in][outp] each
  p.B = g.Wt + g.pl.wt_off[l]; p.sB = (long long)g.pl.wt_elems; p.ldb = g.pl.wp[l]; p.tB = (long long)g.pl.plane(l);
}
// forward (launch_mm3_fwd): C [rows][fout] = act(A [rows][fin] W_l + b_l), no activation on the last layer
static MMParams layer_fwd(const LayerGemm &g, int l, MMIn A, MMOut C, int rows) {
  MMParams p{};
  p.A = A.p; p.sA = A.s; p.lda = A.ld; p.K = g.pl.fin[l];
  mm3_weights(g, l, p);
  p.C = C.p; p.sC = C.s; p.ldc = C.ld;
  p.M = rows; p.N = g.pl.fout[l];
  p.bias = g.theta + g.pl.b_off[l]; p.sBias = g.d;
  p.act = g.act; p.apply_act = l + 1 < g.pl.L;
  return p;
}
// dW (launch_mm3_dw): dW_l [fin][fout] (+)= A^T dZ over the rows, straight into the slab rows at the kernel's offset (leading
// dimension: the real width); the bias gradient dZ^T 1 from the B tiles of M tile 0
static MMParams layer_dw(const LayerGemm &g, int l, MMIn A, MMIn dZ, int rows, float *slab, long long dp, bool accumulate) {
  MMParams p{};
  p.A = A.p; p.sA = A.s; p.lda = A.ld;
  p.B = dZ.p; p.sB = dZ.s; p.ldb = dZ.ld;
  p.C = slab + g.pl.w_off[l]; p.sC = dp; p.ldc = g.pl.fout[l];
  p.M = g.pl.fin[l]; p.N = g.pl.fout[l]; p.K = rows;
  p.accumulate = accumulate;
  p.colsum = slab + g.pl.b_off[l]; p.sColsum = dp;
  return p;
}
// dH (launch_mm3_dh): C [rows][fin] = (dZ [rows][fout] W_l^T) * act'(Hprev), the forward's planes read as [in][out] rows.  No
// Hprev (the layer's input is no activation's output): the product alone, for the plain store form
static MMParams layer_dh(const LayerGemm &g, int l, MMIn dZ, MMIn Hprev, MMOut C, int rows) {
  MMParams p{};
  p.A = dZ.p; p.sA = dZ.s; p.lda = dZ.ld; p.K = g.pl.fout[l];
  mm3_weights(g, l, p);
  p.C = C.p; p.sC = C.s; p.ldc = C.ld;
  p.M = rows; p.N = g.pl.fin[l];
  if (Hprev.p) { p.Hprev = Hprev.p; p.sH = Hprev.s; p.ldh = Hprev.ld; p.act = g.act; }
  return p;
}

// ---- Dense half of LeNet (flat -> 120 -> 84 -> K) on k_mm3, TERMS = 3: the weights as term planes in s->wide_wt, activations
// [E][Rc][ld] with ld = 120 / 88 / up8(K)
static int lenet_dense_prep(mile_sampler *s, const float *theta, int E, hipStream_t st) {
  const LayerPlan pl = layer_plan_lenet(s->lg);
  HIP_TRY(grow(s->wide_wt, s->wide_wt_bytes, (size_t)E * pl.wt_elems * 2, 1));
  wide_prep_weights<3>(pl, theta, s->lg.d, E, (bf16 *)s->wide_wt, st);
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}
static int lenet_dense_chunk(mile_sampler *s, const float *theta, int E, int Rc, int r0, int chunk, const LeNetDenseBufs &b, const void *y,
                             float *slab, long long dp, float *llacc, float *out_ll, long long Ntot, long long s0, hipStream_t st) {
  const LeNetGeom &g = s->lg;
  const LayerPlan pl = layer_plan_lenet(g);
  const LayerGemm lg{pl, (const bf16 *)s->wide_wt, theta, g.d, s->ds.activation};
  auto of = [&](float *p, int l) { return MMOut{p, (long long)Rc * pl.wp[l], pl.wp[l]}; };   // layer l's outputs, or their dZ
  const MMOut H[3] = {of(b.f1, 0), of(b.f2, 1), of(b.out, 2)};
  const MMOut dz[3] = {of(b.df1, 0), of(b.df2, 1), H[2]};        // the head's d(out) is in place
  const MMIn in[3] = {{b.p2, (long long)Rc * g.flat, g.flat}, H[0], H[1]};
  for (int l = 0; l < 3; ++l) HIP_TRY(launch_mm3_fwd<3>(layer_fwd(lg, l, in[l], H[l], Rc), E, st));
  if (!slab) {   // evaluation
    launch_rowll(H[2], y, r0, Rc, g.K, s->ds.task, out_ll, Ntot, s0, E, st);
    HIP_TRY(hipGetLastError());
    return MILE_OK;
  }
  k_wide_head<<<E, 256, 0, st>>>(H[2].p, H[2].s, H[2].ld, y, r0, Rc, g.K, s->ds.task, llacc, chunk == 0);
  for (int l = 2; l >= 0; --l) {
    HIP_TRY(launch_mm3_dw<3>(layer_dw(lg, l, in[l], dz[l], Rc, slab, dp, chunk != 0), E, st));
    if (l > 0) HIP_TRY(launch_mm3_dh<3>(layer_dh(lg, l, dz[l], in[l], dz[l - 1], Rc), E, st));
    else   // the pooled conv output [E][Rc][flat] takes d(in) as it is
      HIP_TRY((launch_mm3_k<MM_A_MK, MM_B_T3_NK, MM_EPI_STORE, 3, -1, false, false>(layer_dh(lg, 0, dz[0], {}, {b.dp2, in[0].s, in[0].ld}, Rc), E, st)));
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

template <int TERMS>
static int launch_grad_wide(mile_sampler *s, const GradParams &gp, int E, hipStream_t st) {
  const DevSpec &ds = s->ds;
  const int L = ds.n_layers, d = ds.d, N = gp.N, Fp = s->Fp;   // gp.N < s->N under a row window (workspace sized for the whole set)
  const LayerPlan pl = layer_plan_fcn(ds, Fp, TERMS);
  if (E != s->wide_E || !s->wide_ws) {   // activation workspace: MILE_WIDE_WS_GB (default 16 GiB of the 288), whole data set if it fits
    double gb = 16.0;
    if (const char *ev = getenv("MILE_WIDE_WS_GB")) gb = std::max(0.001, atof(ev));
    const size_t budget = (size_t)(gb * (double)(1ull << 30) / 4.0);
    const size_t Nall = (size_t)s->N;   // sized for the whole data set, also when the first call comes under a row window
    size_t R = budget / ((size_t)E * pl.per_row());
    R = std::min<size_t>(std::max<size_t>(R, 128), Nall);
    if (R < Nall) R = std::max<size_t>(128, R / 128 * 128);
    R = gemm_rows_hook(R, Nall);
    const size_t need = (size_t)E * R * pl.per_row();
    HIP_TRY(grow(s->wide_ws, s->wide_ws_floats, need, 4));
    HIP_TRY(hipMemsetAsync(s->wide_ws, 0, s->wide_ws_floats * 4, st));   // padding columns are read as operands: zero, once per layout
    s->wide_R = (int)R; s->wide_E = E;
  }
  HIP_TRY(grow(s->wide_wt, s->wide_wt_bytes, (size_t)E * pl.wt_elems * 2, 1));
  const int R = s->wide_R;
  float *H[MILE_MAX_LAYERS], *tmp[2];
  {
    float *q = s->wide_ws;
    for (int l = 0; l < L; ++l) { H[l] = q; q += (size_t)E * R * pl.wp[l]; }
    tmp[0] = q; q += (size_t)E * R * pl.maxwp;
    tmp[1] = q;
  }
  auto of = [&](float *p, int l) { return MMOut{p, (long long)R * pl.wp[l], pl.wp[l]}; };   // layer l's outputs, or their dZ: [E][R][wp]
  // The two dZ buffers are shared by layers of different padded widths: a layer's padding columns (real width .. wp) are not
  // written by the dH epilogue and would otherwise show what an earlier use with another leading dimension -- possibly an
  // earlier CALL with a diverged, non-finite theta -- left there; k_mm3 reads operands in 4- / 8-element granules, and
  // NaN x 0 is NaN.  Re-zeroed per call whenever the hidden layers pad to different widths (nets of equal hidden
  // widths -- B4 -- keep one layout per buffer, whose padding stays zero from the workspace's own memset).
  {
    bool mixed = false;                                    // dZ of layers 0 .. L-2 lives in tmp with leading dimension wp[l]
    for (int l = 1; l + 1 < L; ++l) mixed = mixed || pl.wp[l] != pl.wp[0];
    if (mixed) HIP_TRY(hipMemsetAsync(tmp[0], 0, (size_t)E * R * pl.maxwp * 2 * 4, st));
  }
  const LayerGemm g{pl, (const bf16 *)s->wide_wt, gp.theta, d, ds.activation};
  wide_prep_weights<TERMS>(pl, gp.theta, d, E, (bf16 *)s->wide_wt, st);   // this gradient's weights
  float *slab = gp.slabs;        // S = 1: [E][dp]
  const long long dp = gp.dp;
  // The last layer (K <= 8 outputs on a hidden width <= 256) as one pass over the last hidden activations -- forward, head, dH and
  // dW of that layer in k_wide_headblock -- instead of four launches on 128-wide MFMA tiles (fp32-faithful form only: the
  // bf16-operand recipe rounds this product's operands)
  const bool headblock = TERMS == 3 && L >= 2 && ds.widths[L - 2] <= 256 && ds.widths[L - 1] <= WH_KMAX;
  constexpr int HB_ROWS = 512;                      // rows per workgroup of k_wide_headblock
  if (headblock) {
    const size_t need = (size_t)E * ((R + HB_ROWS - 1) / HB_ROWS) * ((size_t)ds.widths[L - 2] * ds.widths[L - 1] + ds.widths[L - 1] + 1);
    HIP_TRY(grow(s->wide_hb, s->wide_hb_floats, need, 4));
  }
  for (int r0 = 0, chunk = 0; r0 < N; r0 += R, ++chunk) {
    const int Rc = std::min(R, N - r0);
    auto in = [&](int l) { return l ? MMIn(of(H[l - 1], l - 1)) : MMIn{gp.Xp + (size_t)r0 * Fp, 0, Fp}; };   // X zero-padded to Fp columns, one copy for the batch
    // ---- forward
    for (int l = 0; l < L - (headblock ? 1 : 0); ++l) HIP_TRY(launch_mm3_fwd<TERMS>(layer_fwd(g, l, in(l), of(H[l], l), Rc), E, st));
    // ---- head: log-likelihood and d(out), in place
    float *dz = H[L - 1];
    int pp = 0, ltop = L - 1;
    if (headblock) {
      const int Wl = ds.widths[L - 2], K = ds.widths[L - 1], nblk = (Rc + HB_ROWS - 1) / HB_ROWS;
#define MILE_HB(K_, WF_) k_wide_headblock<K_, WF_><<<dim3(nblk, E), 256, 0, st>>>(H[L - 2], (long long)R * pl.wp[L - 2], pl.wp[L - 2], Wl, gp.theta, d, \
      ds.w_off[L - 1], ds.b_off[L - 1], gp.y, r0, Rc, ds.task, ds.activation, tmp[0], (long long)R * pl.wp[L - 2], pl.wp[L - 2], s->wide_hb, HB_ROWS)
#define MILE_HB_K(K_) case K_: if (Wl == 256) MILE_HB(K_, true); else MILE_HB(K_, false); break;
      switch (K) { MILE_HB_K(1) MILE_HB_K(2) MILE_HB_K(3) MILE_HB_K(4) MILE_HB_K(5) MILE_HB_K(6) MILE_HB_K(7) MILE_HB_K(8) }
#undef MILE_HB_K
#undef MILE_HB
      k_wide_headblock_reduce<<<dim3(8, E), 256, 0, st>>>(s->wide_hb, nblk, Wl * K, K, slab, dp, ds.w_off[L - 1], ds.b_off[L - 1], gp.llpart,
                                                          chunk != 0);
      dz = tmp[0]; pp = 1; ltop = L - 2;
    } else {
      k_wide_head<<<E, 256, 0, st>>>(H[L - 1], (long long)R * pl.wp[L - 1], pl.wp[L - 1], gp.y, r0, Rc, ds.widths[L - 1], ds.task, gp.llpart, chunk == 0);
    }
    // ---- backward
    for (int l = ltop; l >= 0; --l) {
      HIP_TRY(launch_mm3_dw<TERMS>(layer_dw(g, l, in(l), of(dz, l), Rc, slab, dp, chunk != 0), E, st));
      if (l > 0) {   // dZ_{l-1} = (dz W_l^T) * act'(H_{l-1})
        HIP_TRY(launch_mm3_dh<TERMS>(layer_dh(g, l, of(dz, l), in(l), of(tmp[pp], l - 1), Rc), E, st));
        dz = tmp[pp];
        pp ^= 1;
      }
    }
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

// what the fused kernels' launchers below run: the gradient (out_ll == nullptr), the log-likelihoods, or (y == nullptr) raw outputs
static MileRun run_of(const void *y, const float *out_ll) { return !out_ll ? MILE_RUN_GRAD : (y ? MILE_RUN_LOGLIK : MILE_RUN_RAW); }

// ---- LeNetti (mile_lenetti.h; the kernels are instantiated in mile_lenetti.hip).  Gradient (out_ll == nullptr): grid (S row
// ranges, E chains) -> slabs / llpart; evaluation: grid (S row blocks, E samples) -> out_ll[e * N + row], or (y == nullptr) the
// raw outputs out_ll[(e * N + row) * K + c]
static hipError_t launch_lenetti(mile_sampler *s, const float *theta, int E, const float *X, const void *y, int N, int S, int dp,
                                 float *out_ll, hipStream_t st) {
  LeNettiParams lp{};
  lp.g = s->ng; lp.activation = s->ds.activation; lp.task = s->ds.task;
  lp.theta = theta; lp.X = X; lp.y = y; lp.slabs = s->slabs; lp.llpart = s->llpart; lp.out = out_ll;
  lp.N = N; lp.S = S; lp.dp = dp;
  return mile_launch_lenetti(lp, E, run_of(y, out_ll), st);
}

// ---- the three attention models (mile_attn.h, mile_attn_pre.h, mile_attn_wide.h; the kernels are instantiated in the .hip file
// of the same name).  Gradient (out_ll == nullptr): grid (S row ranges, E chains) -> slabs / llpart; evaluation: grid (S row
// blocks, E samples) -> out_ll[e * N + row], or (y == nullptr) the logits out_ll[(e * N + row) * K + c]
static hipError_t launch_attn(mile_sampler *s, const float *theta, int E, const float *X, const void *y, int N, int S, int dp,
                              float *out_ll, hipStream_t st) {
  AttnParams ap{};
  ap.g = s->ag;
  ap.theta = theta; ap.X = X; ap.y = y; ap.emb = s->emb_tab; ap.pos = s->pos_tab;   // the tables: null but for the pretrained model
  ap.slabs = s->slabs; ap.llpart = s->llpart; ap.out = out_ll;
  ap.N = N; ap.S = S; ap.dp = dp;
  const MileRun run = run_of(y, out_ll);
  return is_attn(s) ? mile_launch_attn(ap, E, run, st)
         : is_attn_pre(s) ? mile_launch_attn_pre(ap, E, run, st)
                          : mile_launch_attn_wide(ap, E, run, st);
}

// ---- the gradient of each grad kernel: the `grad` of its row in kGrad.  gp holds the row window and S; fz the update that runs
// as the launch's epilogue (fuses) ----------------------------------------------------------------------------------------------
static int grad_w64(mile_sampler *s, const GradParams &gp, const W64Fuse &fz, int E, hipStream_t st) {
  const int nh = s->spec.n_layers - 1, fq = s->Fp / 8;
  hipError_t e = hipErrorInvalidValue;
  if (nh == 1 && fq == 1) e = launch_w64<1, 1>(gp, fz, E, st);
  else if (nh == 2 && fq == 1) e = launch_w64<2, 1>(gp, fz, E, st);
  else if (nh == 3 && fq == 1) e = launch_w64<3, 1>(gp, fz, E, st);
  else if (nh == 1 && fq == 2) e = launch_w64<1, 2>(gp, fz, E, st);
  else if (nh == 2 && fq == 2) e = launch_w64<2, 2>(gp, fz, E, st);
  else if (nh == 3 && fq == 2) e = launch_w64<3, 2>(gp, fz, E, st);
  HIP_TRY(e);
  return MILE_OK;
}
static int grad_w64x3(mile_sampler *s, const GradParams &gp, const W64Fuse &fz, int E, hipStream_t st) {
  const int nh = s->spec.n_layers - 1, fq = s->Fp / 8;
  hipError_t e = hipErrorInvalidValue;
  if (nh == 2 && fq == 1) e = launch_w64<2, 1, true>(gp, fz, E, st);
  else if (nh == 3 && fq == 1) e = launch_w64<3, 1, true>(gp, fz, E, st);
  else if (fq == 2 && !fz.enabled) e = mile_launch_w64_split_fq2(nh, gp, E, st);   // mile_w64_fq2.hip
  HIP_TRY(e);
  return MILE_OK;
}
static int grad_narrow(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) {
  HIP_TRY(launch_narrow(s, gp, E, st));
  return MILE_OK;
}
static int grad_attn(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) {
  HIP_TRY(launch_attn(s, gp.theta, E, gp.X, gp.y, gp.N, gp.S, gp.dp, nullptr, st));
  return MILE_OK;
}
static int grad_lenetti(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) {
  HIP_TRY(launch_lenetti(s, gp.theta, E, gp.X, gp.y, gp.N, gp.S, gp.dp, nullptr, st));
  return MILE_OK;
}
template <int MODE>
static int grad_lenet(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) {
  return run_lenet(s, gp.theta, E, gp.X, gp.y, gp.N, gp.slabs, gp.dp, gp.llpart, nullptr, 0, st, MODE);
}
static int grad_gemm(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) { return launch_grad_gemm(s, gp, E, st); }
static int grad_wide3(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) { return launch_grad_wide<3>(s, gp, E, st); }
static int grad_wide1(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) { return launch_grad_wide<1>(s, gp, E, st); }
static int grad_w128b(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) {
  if (!s->Xb) return fail(MILE_ERR_STATE, "bf16 data copies missing: call mile_set_data");
  const int nh = s->spec.n_layers - 1;
  hipError_t e = hipErrorInvalidValue;
  if (nh == 1) e = launch_w128b<1>(gp, E, st);
  else if (nh == 2) e = launch_w128b<2>(gp, E, st);
  else if (nh == 3) e = launch_w128b<3>(gp, E, st);
  HIP_TRY(e);
  return MILE_OK;
}
static size_t generic_lds(const DevSpec &ds) { return ((size_t)generic_R(ds) * (ds.act_stride + 2 * ds.max_width) + 16) * 4; }
static int grad_generic(mile_sampler *s, const GradParams &gp, const W64Fuse &, int E, hipStream_t st) {
  k_grad_generic<<<dim3(gp.S, E), 256, generic_lds(s->ds), st>>>(gp);
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

// Partition mode: theta is the compact [E, d_s] array and the gradient lands in the compact slabs (sample_slabs) -- straight
// from the partition form of k_grad_narrow, or, for every other kernel, from the unchanged kernel on the library's full rows
// between k_part_scatter and k_part_gather.  full_layout (mile_warmstart_step): theta is [E, d] whatever the mode.
static int launch_grad(mile_sampler *s, const float *theta, int E, hipStream_t st, const UpdParams *fused_update, bool full_layout) {
  if (!s->X) return fail(MILE_ERR_STATE, "no data: call mile_set_data first");
  const bool part = s->part && !full_layout;
  if (part && E != s->part_E) return fail(MILE_ERR_INVALID, "partition mode: E differs from the frozen rows' (mile_set_partition)");
  if (part && !s->part_slabs) return fail(MILE_ERR_STATE, "workspace too small: call mile_reserve(E) after mile_set_partition");
  if (tables_missing(s)) return fail(MILE_ERR_STATE, kNoTables);
  const GradKernel &k = grad_kernel(resolved_kernel(s));
  const int S = k.row_splits(s, E);
  if (E > s->E_cap || (size_t)E * S > s->ES_cap) return fail(MILE_ERR_STATE, "workspace too small: call mile_reserve(E) first");
  GradParams gp;
  gp.spec = s->ds;
  gp.theta = theta;
  gp.X = s->X; gp.Xp = s->Xp; gp.y = s->y; gp.Xb = s->Xb; gp.Xt = s->Xt;
  gp.slabs = s->slabs; gp.llpart = s->llpart;
  gp.N = s->N; gp.Npad = s->Npad; gp.Npb = s->Npb; gp.Fp = s->Fp; gp.S = S; gp.R = generic_R(s->ds); gp.dp = (s->ds.d + 3) / 4 * 4;
  if (s->win_count) {   // minibatch: the same kernels on a shifted view of the rows
    if (!k.windowed)
      return fail(MILE_ERR_STATE, "a row window needs the generic, the MFMA_NARROW, an MFMA_W64, an MFMA_WIDE, a LENET, the LENETTI or an ATTN grad kernel");
    if (fused_update) return fail(MILE_ERR_STATE, "row windows are for mile_logpost_grad only");
    const int F = s->spec.in_features;
    gp.X = s->X + (size_t)s->win_begin * F;
    gp.Xp = s->Xp + (size_t)s->win_begin * s->Fp;
    gp.y = (const char *)s->y + (size_t)s->win_begin * 4;
    gp.N = s->win_count;
    gp.Npad = (s->win_count + 31) / 32 * 32;
  }
  gp.dbg_buf = nullptr; gp.dbg = 0;   // lab-harness fields
  const bool part_fused = part && k.id == MILE_GRAD_MFMA_NARROW_F32;
  if (part_fused) {
    gp.part_frozen = s->part_rows; gp.part_d = s->part_d;
    gp.part_b0 = s->part_b0; gp.part_w0 = s->part_w0; gp.part_bl = s->part_bl; gp.part_wl = s->part_wl;
    gp.slabs = s->part_slabs; gp.dp = sample_dp(s);
  } else if (part) {
    if (fused_update) return fail(MILE_ERR_STATE, "partition mode: no update epilogue");
    gp.theta = s->part_rows;
  }
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (s->timing) {
    if (s->ev_used + 2 > s->ev.size()) {
      for (int k = 0; k < 2; ++k) {
        hipEvent_t ev;
        HIP_TRY(hipEventCreate(&ev));
        s->ev.push_back(ev);
      }
    }
    e0 = s->ev[s->ev_used]; e1 = s->ev[s->ev_used + 1];
    s->ev_used += 2;
    HIP_TRY(hipEventRecord(e0, st));
  }
  W64Fuse fz{};
  if (fused_update) {
    if (!k.fuses) return fail(MILE_ERR_STATE, "fused update needs the mfma_w64_bf16x3 grad kernel");
    fz.upd = *fused_update; fz.arrive = s->arrive; fz.enabled = 1; fz.kind = upd_kind(*fused_update);
  }
  if (part && !part_fused) {
    k_part_scatter<<<E, 256, 0, st>>>(theta, s->part_d, s->part_rows, s->ds.d, s->part_seg);
    HIP_TRY(hipGetLastError());
  }
  if (const int rc = k.grad(s, gp, fz, E, st)) return rc;
  if (part && !part_fused) {
    k_part_gather<<<E * S, 256, 0, st>>>(s->slabs, gp.dp, s->part_slabs, sample_dp(s), s->part_seg);
    HIP_TRY(hipGetLastError());
  }
  if (s->timing) HIP_TRY(hipEventRecord(e1, st));
  return MILE_OK;
}

// gradient at `theta`, then the update `u` that consumes it: one launch when the update can be the grad kernel's epilogue
static int grad_then_update(mile_sampler *s, const float *theta, int E, const UpdParams &u, bool fused, hipStream_t st) {
  if (fused) return launch_grad(s, theta, E, st, &u);
  const int rc = launch_grad(s, theta, E, st);
  if (rc) return rc;
  launch_update(u, E, st);
  return MILE_OK;
}

// ---- MCLMC (mile_step, mile_tune) ------------------------------------------------------------------------------------
// A step is three update launches around two gradients:
//   start   O(z1) . B(b1) . A(1/2) from the cached gradient: the first step of a call, later chained onto a record launch
//   mid     B(1 - 2 b1) . A(1/2)
//   record  B(b1) . O(z2) . record [. the next step's start]
// The steady-state words must be the kinds k_update_fast specialises (upd_kind); any other word runs the run-time-flag form.
static constexpr int32_t UPD_STEP_START = UPD_B2 | UPD_A;                                   // + UPD_OB under O-step-O
static constexpr int32_t UPD_STEP_RECORD = UPD_FROM_SLABS | UPD_B1 | UPD_OA | UPD_RECORD;
static_assert((UPD_STEP_RECORD | UPD_STEP_START | UPD_OB | UPD_NO_G) == UPD_KIND_REC, "sampling steady state");
static_assert((UPD_STEP_RECORD | UPD_TUNE | UPD_STEP_START | UPD_OB) == UPD_KIND_TUNE, "warm-up steady state");
static const float MC_B1 = (float)MCLACHLAN_B1, MC_B2 = (float)(1.0 - 2.0 * MCLACHLAN_B1);

struct Mclmc {             // one mile_step / mile_tune call
  UpdParams up;            // what every update launch shares: sizes, prior, state, workspace, step size, L, preconditioner, RNG
  int kernel;
  bool oso;                // MILE_REFRESH_O_STEP_O
  const float *noise;      // [n_steps, 2, E, d] or NULL: Philox
  int64_t step_offset;
  float *out_info;         // [n_steps, E, 3] or NULL
  const float *noise_at(int i, int k) const { return noise ? noise + ((size_t)i * 2 + k) * ((size_t)up.E * up.d) : nullptr; }
};

// O(z1) . B(b1) . A(1/2) of step i, added to u (a start launch, or a record launch that chains the next step on)
static void chain_start(UpdParams &u, const Mclmc &m, int i) {
  u.flags |= UPD_STEP_START | (m.oso ? UPD_OB : 0);
  u.zB = m.noise_at(i, 0); u.stepB = (uint32_t)(m.step_offset + i); u.stageB = 0; u.hB = 0.5f;
  u.coef_b2 = MC_B1; u.coef_a = 0.5f;
}
static UpdParams upd_start(const Mclmc &m, int i) {
  UpdParams u = m.up;
  u.flags = UPD_START;
  chain_start(u, m, i);
  return u;
}
static UpdParams upd_mid(const Mclmc &m) {
  UpdParams u = m.up;
  u.flags = UPD_KIND_MID;
  u.coef_b1 = MC_B2; u.coef_a = 0.5f;
  return u;
}
static UpdParams upd_record(const Mclmc &m, int i) {
  UpdParams u = m.up;
  u.flags = UPD_STEP_RECORD;
  u.coef_b1 = MC_B1;
  u.zA = m.noise_at(i, 1); u.stepA = (uint32_t)(m.step_offset + i); u.stageA = 1; u.hA = m.oso ? 0.5f : 1.0f;
  if (m.out_info) u.out_info = m.out_info + (size_t)i * m.up.E * 3;
  return u;
}

// The warm-up tuner's inputs at schedule step sp (UpdParams under UPD_TUNE, TunePostParams)
template <class P>
static void set_tuner(P &p, const mile_tune_args *a, int sp) {
  p.t_eps = a->step_size; p.t_eps_max = a->step_size_max; p.t_time = a->time; p.t_xavg = a->x_average;
  p.t_W = a->stream_weight; p.t_avg = a->stream_average;
  p.t_mask = sp < a->n_mask_steps ? 1.0f : 0.0f;
  const double tot = (double)a->schedule_total, vs = a->desired_energy_var_start, ve = a->desired_energy_var_end;
  if (vs > 2.0) {
    const double tau = tot / 4.0, ex = std::exp(-(double)sp / tau);
    p.t_var = (float)(vs * ex + ve * (1.0 - ex));
  } else {
    p.t_var = (float)(vs - (vs - ve) * std::min((double)sp / tot, 1.0));
  }
  p.t_trust = a->trust_in_estimate; p.t_decay = a->decay_rate;
}

static const char *args_refusal(const mile_sampler *, const mile_step_args *a) {
  if (!a->step_size || !a->L) return "mile_step: step_size and L are required";
  if (a->n_steps < 0) return "mile_step: n_steps < 0";
  return nullptr;
}
static const char *args_refusal(const mile_sampler *s, const mile_tune_args *a) {
  if (!a->step_size || !a->L || !a->step_size_max || !a->time || !a->x_average || !a->stream_weight || !a->stream_average)
    return "mile_tune: null tuner array";
  if (a->n_steps < 0 || a->schedule_total < 1) return "mile_tune: bad step counts";
  if ((sample_dim(s) >> 2) < 1) return "mile_tune: d < 4";
  return nullptr;
}

// The checks of mile_step / mile_tune (`fn`), then the call's Mclmc.  n_steps == 0 passes before the device is touched.
template <class Args>
static int mclmc_begin(mile_sampler *s, mile_state *state, const Args *a, const std::string &fn, Mclmc &m) {
  if (!s || !state || !a) return fail(MILE_ERR_INVALID, fn + ": null argument");
  if (!state->position || !state->momentum || !state->logdensity || !state->logdensity_grad)
    return fail(MILE_ERR_INVALID, fn + ": null state field");
  if (const char *r = args_refusal(s, a)) return fail(MILE_ERR_INVALID, r);
  if (a->refresh != MILE_REFRESH_O_STEP_O && a->refresh != MILE_REFRESH_STEP_O)
    return fail(MILE_ERR_INVALID, fn + ": unknown refresh mode");
  const int E = state->n_particles, d = sample_dim(s);
  if (E < 1) return fail(MILE_ERR_INVALID, fn + ": n_particles must be >= 1");
  if (s->part && E != s->part_E) return fail(MILE_ERR_INVALID, fn + ": partition mode: E differs from the frozen rows' (mile_set_partition)");
  if (a->n_steps == 0) return MILE_OK;
  HIP_TRY(hipSetDevice(s->device));
  if (!s->X) return fail(MILE_ERR_STATE, "no data: call mile_set_data first");
  if (tables_missing(s)) return fail(MILE_ERR_STATE, kNoTables);
  m.kernel = resolved_kernel(s);
  const int S = choose_S(s, E, m.kernel);
  if (E > s->E_cap || (size_t)E * S > s->ES_cap) return fail(MILE_ERR_STATE, "workspace too small: call mile_reserve(E) first");
  m.oso = a->refresh == MILE_REFRESH_O_STEP_O;
  m.noise = a->noise; m.step_offset = a->step_offset; m.out_info = a->out_info;
  UpdParams &up = m.up;
  up.d = d; up.E = E; up.S = S; up.dp = (d + 3) / 4 * 4;
  up.prior = s->ds.prior; up.prior_loc = s->ds.prior_loc; up.prior_scale = s->ds.prior_scale;
  up.x = state->position; up.u = state->momentum; up.g = state->logdensity_grad; up.logp = state->logdensity;
  up.slabs = sample_slabs(s); up.llpart = s->llpart;
  up.eps = a->step_size; up.L = a->L; up.sdc = a->sqrt_diag_cov;
  up.seed = a->seed; up.pids = a->particle_ids;
  up.dK = s->dK; up.lold = s->lold; up.upart = s->upart;
  return MILE_OK;
}

// gridDim.y holds at most 65 535 samples: eval_forward walks S in chunks of that many, so every `loglik` below sees S <= this
#define MILE_GRID_Y_MAX 65535

template <int NH, int FQ>
static hipError_t launch_fwd_w64(const PredParams &pp, int S, hipStream_t st) {
  using LY = W64Layout<NH, FQ>;
  const bool raw = !pp.y;   // mile_predict: (mu, log sigma) per row
  const hipError_t e = raw ? mile_set_max_lds<k_fwd_w64<NH, FQ, true>>(LY::BYTES) : mile_set_max_lds<k_fwd_w64<NH, FQ>>(LY::BYTES);
  if (e != hipSuccess) return e;
  if (raw) k_fwd_w64<NH, FQ, true><<<dim3(pp.SB, S), 256, LY::BYTES, st>>>(pp);
  else k_fwd_w64<NH, FQ><<<dim3(pp.SB, S), 256, LY::BYTES, st>>>(pp);
  return hipGetLastError();
}

// Evaluation forward for wide nets: the same strided-batched SGEMMs, samples as the batch.  y == nullptr (mile_predict): out is
// the raw outputs [S, N, O].
static int launch_fwd_gemm(mile_sampler *s, const float *theta, int S, const float *X, const void *y, int N, float *out, hipStream_t st) {
  if (const int rc = rocblas_ready(s, st)) return rc;
  const DevSpec &ds = s->ds;
  const int L = ds.n_layers, F = ds.in_features, d = ds.d;
  // two ping-pong activation buffers of [Sc][Rc][max_width]; <= 1 GiB of floats
  const size_t budget = (size_t)1 << 28;
  const int Sc = std::min(S, 1024);
  size_t Rr = budget / (2 * (size_t)Sc * ds.max_width);
  Rr = std::max<size_t>(1, std::min<size_t>(Rr, (size_t)N));
  Rr = gemm_rows_hook(Rr, (size_t)N);
  const int R = (int)Rr;
  const size_t need = 2 * (size_t)Sc * R * ds.max_width;
  HIP_TRY(grow(s->gemm_ws, s->gemm_ws_floats, need, 4));
  s->gemm_E = 0;   // the gradient path re-derives its layout on its next call
  float *buf[2] = {s->gemm_ws, s->gemm_ws + (size_t)Sc * R * ds.max_width};
  const float one = 1.0f, zero = 0.0f;
  for (int s0 = 0; s0 < S; s0 += Sc) {
    const int Sn = std::min(Sc, S - s0);
    const float *th = theta + (size_t)s0 * d;
    for (int r0 = 0; r0 < N; r0 += R) {
      const int Rc = std::min(R, N - r0);
      int pp = 0;
      for (int l = 0; l < L; ++l) {
        const int fin = l == 0 ? F : ds.widths[l - 1], fout = ds.widths[l];
        const float *in = l == 0 ? X + (size_t)r0 * F : buf[pp ^ 1];
        const long long sin = l == 0 ? 0 : (long long)Rc * fin;
        if (g_rb.sgemm_sb(s->blas, RB_OP_N, RB_OP_N, fout, Rc, fin, &one, th + ds.w_off[l], fout, d, in, fin, sin, &zero, buf[pp], fout,
                          (long long)Rc * fout, Sn))
          return fail(MILE_ERR_HIP, "rocblas sgemm (evaluation) failed");
        const long long RW = (long long)Rc * fout;
        k_gemm_bias_act<<<dim3((unsigned)std::min<long long>((RW + 255) / 256, 4096), Sn), 256, 0, st>>>(buf[pp], th, ds.b_off[l], d, fout, RW,
                                                                                                   ds.activation, l + 1 < L);
        pp ^= 1;
      }
      const int O = ds.widths[L - 1];
      launch_rowll({buf[pp ^ 1], (long long)Rc * O, O}, y, r0, Rc, O, ds.task, out, N, s0, Sn, st);
    }
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

// Evaluation forward for wide nets on the MFMA GEMMs (fp32-faithful, whatever the sampling kernel was): samples as the batch.
// y == nullptr (mile_predict): out is the raw outputs [S, N, O].
static int launch_fwd_wide(mile_sampler *s, const float *theta, int S, const float *Xp, int Fp, const void *y, int N, float *out,
                           hipStream_t st) {
  const DevSpec &ds = s->ds;
  const int L = ds.n_layers, d = ds.d;
  const LayerPlan pl = layer_plan_fcn(ds, Fp, 3);
  const int Sc = std::min(S, 512);
  size_t Rr = ((size_t)1 << 28) / (2 * (size_t)Sc * pl.maxwp);        // two ping-pong buffers, <= 1 GiB of floats
  Rr = std::max<size_t>(1, std::min<size_t>(Rr, (size_t)N));
  Rr = gemm_rows_hook(Rr, (size_t)N);
  const int R = (int)Rr;
  const size_t need = 2 * (size_t)Sc * R * pl.maxwp;
  HIP_TRY(grow(s->wide_ws, s->wide_ws_floats, need, 4));
  s->wide_E = 0;   // the gradient path re-derives (and re-zeroes) its layout on its next call
  HIP_TRY(grow(s->wide_wt, s->wide_wt_bytes, (size_t)Sc * pl.wt_elems * 2, 1));
  float *buf[2] = {s->wide_ws, s->wide_ws + (size_t)Sc * R * pl.maxwp};
  for (int s0 = 0; s0 < S; s0 += Sc) {
    const int Sn = std::min(Sc, S - s0);
    const float *th = theta + (size_t)s0 * d;
    const LayerGemm g{pl, (const bf16 *)s->wide_wt, th, d, ds.activation};
    wide_prep_weights<3>(pl, th, d, Sn, (bf16 *)s->wide_wt, st);
    for (int r0 = 0; r0 < N; r0 += R) {
      const int Rc = std::min(R, N - r0);
      // layers of different widths share the two buffers: padding columns an operand read may touch must be zero
      HIP_TRY(hipMemsetAsync(s->wide_ws, 0, need * 4, st));
      MMIn in{Xp + (size_t)r0 * Fp, 0, Fp};
      for (int l = 0; l < L; ++l) {
        const MMOut Hl{buf[l & 1], (long long)R * pl.wp[l], pl.wp[l]};
        HIP_TRY(launch_mm3_fwd<3>(layer_fwd(g, l, in, Hl, Rc), Sn, st));
        in = Hl;
      }
      launch_rowll(in, y, r0, Rc, ds.widths[L - 1], ds.task, out, N, s0, Sn, st);
    }
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

// ---- evaluation of each grad kernel's model: the `loglik` of its row in kGrad.  pp holds the staged evaluation set; without
// labels (pp.y == nullptr, mile_predict) every row of the table writes the raw outputs, O floats per (sample, row) -----------------
static int loglik_attn_t(mile_sampler *s, PredParams pp, int S, hipStream_t st) {   // the three attention models
  HIP_TRY(launch_attn(s, pp.theta, S, pp.X, pp.y, pp.N, attn_ranges(s->n_cu, S, pp.N), 0, pp.out, st));
  return MILE_OK;
}
static int loglik_lenetti(mile_sampler *s, PredParams pp, int S, hipStream_t st) {
  const int SB = std::max(1, std::min({64, (2 * s->n_cu + S - 1) / S, std::max(1, pp.N / 32)}));
  HIP_TRY(launch_lenetti(s, pp.theta, S, pp.X, pp.y, pp.N, SB, 0, pp.out, st));
  return MILE_OK;
}
template <int MODE>
static int loglik_lenet(mile_sampler *s, PredParams pp, int S, hipStream_t st) {
  for (int s0 = 0; s0 < S; s0 += 256) {
    const int rc = run_lenet(s, pp.theta + (size_t)s0 * s->ds.d, std::min(256, S - s0), pp.X, pp.y, pp.N, nullptr, 0, nullptr, pp.out, s0, st, MODE);
    if (rc) return rc;
  }
  return MILE_OK;
}
static int loglik_gemm(mile_sampler *s, PredParams pp, int S, hipStream_t st) {
  return launch_fwd_gemm(s, pp.theta, S, pp.X, pp.y, pp.N, pp.out, st);
}
// wide nets: evaluation stays fp32-faithful whatever the sampling kernel was
static int loglik_wide(mile_sampler *s, PredParams pp, int S, hipStream_t st) {
  return launch_fwd_wide(s, pp.theta, S, pp.Xp, pp.Fp, pp.y, pp.N, pp.out, st);
}
static int loglik_w64(mile_sampler *s, PredParams pp, int S, hipStream_t st) {
  const int NB = pp.Npad / 32;
  pp.SB = std::max(1, std::min(std::max(1, (2 * s->n_cu) / S), std::max(1, NB / 4)));
  const int nh = s->spec.n_layers - 1, fq = pp.Fp / 8;
  hipError_t e = hipErrorInvalidValue;
  if (nh == 1 && fq == 1) e = launch_fwd_w64<1, 1>(pp, S, st);
  else if (nh == 2 && fq == 1) e = launch_fwd_w64<2, 1>(pp, S, st);
  else if (nh == 3 && fq == 1) e = launch_fwd_w64<3, 1>(pp, S, st);
  else if (nh == 1 && fq == 2) e = launch_fwd_w64<1, 2>(pp, S, st);
  else if (nh == 2 && fq == 2) e = launch_fwd_w64<2, 2>(pp, S, st);
  else if (nh == 3 && fq == 2) e = launch_fwd_w64<3, 2>(pp, S, st);
  HIP_TRY(e);
  return MILE_OK;
}
static int loglik_generic(mile_sampler *s, PredParams pp, int S, hipStream_t st) {
  pp.SB = std::max(1, std::min(std::max(1, (4 * s->n_cu) / S), std::max(1, pp.N / 64)));
  const size_t lds = ((size_t)pp.R * s->ds.act_stride + 16) * 4;
  if (pp.y) k_fwd_generic<<<dim3(pp.SB, S), 256, lds, st>>>(pp);
  else k_fwd_generic<true><<<dim3(pp.SB, S), 256, lds, st>>>(pp);   // mile_predict
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

// ---- launch shape that mile_grad_launch_info reports: the `shape` of each row in kGrad --------------------------------------
static LaunchShape shape_generic(const mile_sampler *s, int) { return {256, (int)generic_lds(s->ds)}; }
static LaunchShape shape_w64(const mile_sampler *s, int) {
  const int nh = s->spec.n_layers - 1, fq = s->Fp / 8;
  return {256, nh == 1 ? (fq == 1 ? W64Layout<1, 1>::BYTES : W64Layout<1, 2>::BYTES)
             : nh == 2 ? (fq == 1 ? W64Layout<2, 1>::BYTES : W64Layout<2, 2>::BYTES)
                       : (fq == 1 ? W64Layout<3, 1>::BYTES : W64Layout<3, 2>::BYTES)};
}
static LaunchShape shape_w64x3(const mile_sampler *s, int) {
  const int nh = s->spec.n_layers - 1, fq = s->Fp / 8;
  return {256, nh == 2 ? (fq == 1 ? W64Layout<2, 1, true>::BYTES : W64Layout<2, 2, true>::BYTES)
                       : (fq == 1 ? W64Layout<3, 1, true>::BYTES : W64Layout<3, 2, true>::BYTES)};
}
static LaunchShape shape_narrow(const mile_sampler *s, int S) {
  const bool wl = narrow_tiles_hidden(s->spec) >= 3;
  return {64 * (wl ? NRW_MAXW : narrow_waves(s, S, s->N)),
          wl ? NarrowLayout<3, 4, 4, true>::BYTES                                         // upper bounds over the instantiations
             : std::max(NarrowLayout<3, 2, 4>::BYTES, NarrowLayout<10, 1, 1>::BYTES)};
}
static LaunchShape shape_attn(const mile_sampler *s, int) { return {256, (int)attn_lds_bytes(s->ag, attn_weights_in_lds(s->ag))}; }
static LaunchShape shape_attn_streamed(const mile_sampler *s, int) { return {256, (int)attnp_lds_bytes(s->ag)}; }   // _pre and _wide
static LaunchShape shape_lenetti(const mile_sampler *s, int) { return {256, (int)lenetti_lds_bytes(s->ng, lenetti_T(s->ng))}; }
static LaunchShape shape_lenet_bf16(const mile_sampler *s, int) { return {256, (int)cm_lds_dw(CM_IN8, s->lg.hp1, s->lg.wp1, 0)}; }
// the largest of the five launches at three term planes: conv2's kernel gradient, or (large images) conv1's
static LaunchShape shape_lenet_bf16x3(const mile_sampler *s, int) {
  const LeNetGeom &g = s->lg;
  const int ni2 = lenet_ni_for((size_t)(g.hp1 * g.wp1 + 8) * 16 + (size_t)g.h2 * g.w2 * 32, 3);
  return {256, (int)std::max(cm_lds_dw(CM_IN8, g.hp1, g.wp1, 0, ni2, 3), cm_lds_dw2x(g.H, g.W, 2, 3))};
}
static LaunchShape shape_rocblas(const mile_sampler *, int) { return {256, 0}; }
template <int TERMS>
static LaunchShape shape_wide(const mile_sampler *, int) { return {256, MMLayout<MM_A_MK, MM_B_T3_NK, TERMS, MILE_MM_KC>::BYTES}; }
static LaunchShape shape_w128b(const mile_sampler *s, int) {
  const int nh = s->spec.n_layers - 1;
  return {256, nh == 1 ? W128Layout<1, 2>::BYTES : nh == 2 ? W128Layout<2, 2>::BYTES : W128Layout<3, 2>::BYTES};
}

// ---- the grad kernels, one row per MILE_GRAD_* id (in id order) --------------------------------------------------------------
static constexpr GradKernel kGrad[] = {
    {MILE_GRAD_GENERIC, "k_grad_generic", is_fcn, "GENERIC is an FCN kernel", nullptr,
     generic_S, true, false, grad_generic, loglik_generic, shape_generic},
    {MILE_GRAD_MFMA_W64, "k_grad_w64", w64_supported,
     "MFMA_W64 needs ReLU regression with 1-3 hidden layers of width 64 and F <= 16", nullptr,
     w64_S, true, false, grad_w64, loglik_w64, shape_w64},
    {MILE_GRAD_MFMA_W128_BF16, "k_grad_w128b", w128b_supported,
     "MFMA_W128_BF16 needs ReLU regression with 1-3 hidden layers of width 128 and F <= 16", nullptr,
     w128b_S, false, false, grad_w128b, loglik_wide, shape_w128b},
    {MILE_GRAD_GEMM_F32, "rocblas_sgemm_strided_batched+k_gemm_*", is_fcn, "GEMM_F32 is an FCN kernel",
     "GEMM_F32 needs librocblas.so, which could not be loaded",
     one_S, false, false, grad_gemm, loglik_gemm, shape_rocblas},
    {MILE_GRAD_LENET_F32, "rocblas_sgemm_strided_batched+k_im2col5/k_col2im5/k_avgpool2", is_lenet,
     "LENET_F32 / LENET_BF16 / LENET_BF16X3 are the kernels of MILE_MODEL_LENET, and its only ones", nullptr,
     one_S, true, false, grad_lenet<LENET_CONV_F32>, loglik_lenet<LENET_CONV_F32>, shape_rocblas},
    {MILE_GRAD_MFMA_W64_BF16X3, "k_grad_w64", w64x3_supported,
     "MFMA_W64_BF16X3 needs ReLU regression with 2-3 hidden layers of width 64 and F <= 16", nullptr,
     w64_S, true, true, grad_w64x3, loglik_w64, shape_w64x3},
    {MILE_GRAD_MFMA_WIDE_BF16X3, "k_mm3 (layer-wise MFMA GEMMs)", is_fcn, "MFMA_WIDE_* are FCN kernels", nullptr,
     one_S, true, false, grad_wide3, loglik_wide, shape_wide<3>},
    {MILE_GRAD_MFMA_WIDE_BF16, "k_mm3 (layer-wise MFMA GEMMs)", is_fcn, "MFMA_WIDE_* are FCN kernels", nullptr,
     one_S, true, false, grad_wide1, loglik_wide, shape_wide<1>},
    {MILE_GRAD_LENET_BF16, "k_conv5m_fwd/dx/dw (implicit-GEMM bf16 MFMA) + k_mm3 (Dense, fp32-faithful three-term products)",
     lenet_bf16_supported, "LENET_BF16 is a kernel of MILE_MODEL_LENET and needs <= 4 image channels", nullptr,
     one_S, true, false, grad_lenet<LENET_CONV_BF16>, loglik_lenet<LENET_CONV_BF16>, shape_lenet_bf16},
    {MILE_GRAD_MFMA_NARROW_F32, "k_grad_narrow", narrow_supported,
     "MFMA_NARROW_F32 needs an FCN with 1-3 hidden layers of width <= 64 and F <= 64 (or 4-10 of width <= 16 and F <= 16) and <= 16 outputs",
     nullptr, narrow_S, true, false, grad_narrow, loglik_generic, shape_narrow},
    {MILE_GRAD_LENETTI_F32, "k_grad_lenetti", is_lenetti, "LENETTI_F32 is the kernel of MILE_MODEL_LENETTI, and its only one", nullptr,
     lenetti_S, true, false, grad_lenetti, loglik_lenetti, shape_lenetti},
    {MILE_GRAD_ATTN_F32, "k_grad_attn", is_attn, "ATTN_F32 is the kernel of MILE_MODEL_ATTN, and its only one", nullptr,
     attn_S, true, false, grad_attn, loglik_attn_t, shape_attn},
    {MILE_GRAD_ATTN_PRE_F32, "k_grad_attn_pre", is_attn_pre,
     "ATTN_PRE_F32 is the kernel of MILE_MODEL_ATTN_PRETRAINED, and its only one", nullptr,
     attn_S, true, false, grad_attn, loglik_attn_t, shape_attn_streamed},
    {MILE_GRAD_ATTN_WIDE_F32, "k_grad_attn_wide", is_attn_wide,
     "ATTN_WIDE_F32 is the kernel of MILE_MODEL_ATTN_WIDE, and its only one", nullptr,
     attn_wide_S, true, false, grad_attn, loglik_attn_t, shape_attn_streamed},
    {MILE_GRAD_LENET_BF16X3, "k_conv5m_fwd/dx/dw<.., 3> (implicit-GEMM bf16x3 MFMA: six products of three-term splits) + k_mm3 (Dense, the same)",
     lenet_bf16_supported, "LENET_BF16X3 is a kernel of MILE_MODEL_LENET and needs <= 4 image channels", nullptr,
     one_S, true, false, grad_lenet<LENET_CONV_BF16X3>, loglik_lenet<LENET_CONV_BF16X3>, shape_lenet_bf16x3},
};
static constexpr bool rows_in_id_order() {
  for (int k = 0; k < (int)(sizeof(kGrad) / sizeof(kGrad[0])); ++k)
    if (kGrad[k].id != k + 1) return false;
  return sizeof(kGrad) / sizeof(kGrad[0]) == MILE_GRAD_LENET_BF16X3;
}
static_assert(rows_in_id_order(), "kGrad: one row per MILE_GRAD_* id, in id order");
static const GradKernel &grad_kernel(int kernel) { return kGrad[kernel - 1]; }

// ---- the evaluation layer's side of the handle (mile_eval_handle.h) -----------------------------------------------------------
EvalView eval_view(const mile_sampler *s) {
  return {s->device, s->n_cu, s->spec.task, s->spec.in_features, s->spec.widths[s->spec.n_layers - 1], s->ds.d};
}
const mile_model_spec *eval_spec(const mile_sampler *s) { return &s->spec; }

// stage the evaluation rows (and labels) in the handle and describe them in s->ev_set; theta and out are eval_forward's to fill in
int stage_rows(mile_sampler *s, const float *X, const void *y, int64_t N, hipStream_t st) {
  HIP_TRY(hipSetDevice(s->device));
  const int F = s->spec.in_features, Npad = ((int)N + 31) / 32 * 32, Fp = (F + 7) / 8 * 8;
  const size_t x_bytes = r256((size_t)Npad * F * 4), xp_bytes = r256((size_t)Npad * Fp * 4);
  HIP_TRY(grow(s->ev_rows, s->ev_rows_bytes, x_bytes + xp_bytes + (size_t)Npad * 4, 1));   // evaluation is off the stepping path
  float *ev_X = (float *)s->ev_rows, *ev_Xp = (float *)((char *)s->ev_rows + x_bytes);
  void *ev_y = (char *)s->ev_rows + x_bytes + xp_bytes;
  HIP_TRY(hipMemcpyAsync(ev_X, X, (size_t)N * F * 4, hipMemcpyDeviceToDevice, st));
  if (y) {
    HIP_TRY(hipMemsetAsync(ev_y, 0, (size_t)Npad * 4, st));
    HIP_TRY(hipMemcpyAsync(ev_y, y, (size_t)N * 4, hipMemcpyDeviceToDevice, st));
  }
  const long long tot = (long long)Npad * Fp;
  k_pad_x<<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(ev_X, ev_Xp, (int)N, Npad, F, Fp);
  PredParams &pp = s->ev_set;
  pp.spec = s->ds; pp.theta = nullptr; pp.X = ev_X; pp.Xp = ev_Xp; pp.y = y ? ev_y : nullptr; pp.out = nullptr;
  pp.N = (int)N; pp.Npad = Npad; pp.Fp = Fp; pp.R = generic_R(s->ds);
  return MILE_OK;
}

// The one forward of evaluation: the resolved kernel's `loglik` of S samples (rows of theta) on the staged rows s->ev_set, into
// out [S, N] -- or, staged without labels, the raw outputs [S, N, O] -- in launches of at most MILE_GRID_Y_MAX samples.
size_t eval_per_sample(const mile_sampler *s) {   // floats of out per sample
  return (size_t)s->ev_set.N * (s->ev_set.y ? 1 : (size_t)s->spec.widths[s->spec.n_layers - 1]);
}
int eval_forward(mile_sampler *s, const float *theta, int64_t S, float *out, hipStream_t st) {
  const GradKernel &gk = grad_kernel(resolved_kernel(s));
  const size_t per_sample = eval_per_sample(s);
  PredParams pp = s->ev_set;
  for (int64_t s0 = 0; s0 < S; s0 += MILE_GRID_Y_MAX) {
    pp.theta = theta + (size_t)s0 * s->ds.d; pp.out = out + (size_t)s0 * per_sample;
    const int rc = gk.loglik(s, pp, (int)std::min<int64_t>(MILE_GRID_Y_MAX, S - s0), st);
    if (rc != MILE_OK) return rc;
  }
  return MILE_OK;
}

// The streamed calls' workspace.  The sweeps of the last mile_predict_quantiles lie in it: whoever reserves it forgets them.
void *reserve_eval_ws(mile_sampler *s, size_t bytes) {
  s->qnt_rows = 0;
  return grow(s->eval_ws, s->eval_ws_bytes, bytes, 1) == hipSuccess ? s->eval_ws : nullptr;
}
void record_quantile_sweeps(mile_sampler *s, const int32_t *sweeps, int64_t rows) { s->qnt_sweeps = sweeps; s->qnt_rows = rows; }
int64_t recorded_quantile_sweeps(const mile_sampler *s, const int32_t **sweeps) { *sweeps = s->qnt_sweeps; return s->qnt_rows; }

extern "C" {

int32_t mile_grad_launch_info(const mile_sampler *s, int32_t E, int32_t *grid_x, int32_t *grid_y,
                              int32_t *block, int32_t *lds_bytes, char *name, int32_t name_len) {
  if (!s || !s->X) return fail(MILE_ERR_STATE, "mile_grad_launch_info: no data set");
  const GradKernel &k = grad_kernel(resolved_kernel(s));
  const int S = k.row_splits(s, E);
  const LaunchShape sh = k.shape(s, S);
  if (grid_x) *grid_x = S;
  if (grid_y) *grid_y = E;
  if (block) *block = sh.block;
  if (lds_bytes) *lds_bytes = sh.lds;
  const std::string nm = std::string(k.name) + (!s->part ? "" : k.id == MILE_GRAD_MFMA_NARROW_F32 ? "<partition>" : " between k_part_scatter / k_part_gather");
  if (name && name_len > 0) { std::strncpy(name, nm.c_str(), name_len - 1); name[name_len - 1] = 0; }
  return MILE_OK;
}

int32_t mile_grad_timing_begin(mile_sampler *s) {
  if (!s) return fail(MILE_ERR_INVALID, "null handle");
  s->timing = true;
  s->ev_used = 0;
  return MILE_OK;
}

int32_t mile_grad_timing_end(mile_sampler *s, float *total_ms, int32_t *n_launches) {
  if (!s) return fail(MILE_ERR_INVALID, "null handle");
  s->timing = false;
  double tot = 0.0;
  const size_t n = s->ev_used / 2;
  if (n) HIP_TRY(hipEventSynchronize(s->ev[s->ev_used - 1]));
  for (size_t k = 0; k < n; ++k) {
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev[2 * k], s->ev[2 * k + 1]));
    tot += ms;
  }
  if (total_ms) *total_ms = (float)tot;
  if (n_launches) *n_launches = (int32_t)n;
  s->ev_used = 0;
  return MILE_OK;
}

int32_t mile_logpost_grad(mile_sampler *s, const float *theta, int32_t E, float *logp, float *grad, void *stream) {
  if (!s || !theta || !logp || !grad || E < 1) return fail(MILE_ERR_INVALID, "mile_logpost_grad: bad argument");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->device));
  int rc = launch_grad(s, theta, E, st);
  if (rc) return rc;
  const int S = choose_S(s, E, resolved_kernel(s));
  k_finalize<<<E, AUX_NT, 0, st>>>(sample_dim(s), sample_dp(s), S, s->ds.prior, s->ds.prior_loc, s->ds.prior_scale, theta,
                                   sample_slabs(s), s->llpart, grad, logp);
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

int32_t mile_warmstart_step(mile_sampler *s, float *theta, int32_t E, const mile_optim_args *a, void *stream) {
  if (!s || !theta || !a || E < 1) return fail(MILE_ERR_INVALID, "mile_warmstart_step: bad argument");
  if (a->kind < MILE_OPT_SGD || a->kind > MILE_OPT_ADAMW) return fail(MILE_ERR_INVALID, "mile_warmstart_step: unknown optimizer");
  if (a->kind != MILE_OPT_SGD && (!a->m || !a->v)) return fail(MILE_ERR_INVALID, "mile_warmstart_step: adam / adamw need m and v");
  if (a->t < 1) return fail(MILE_ERR_INVALID, "mile_warmstart_step: t counts from 1");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->device));
  const int rc = launch_grad(s, theta, E, st, nullptr, true);   // likelihood gradient of the row window -> slabs, llpart
  if (rc) return rc;
  OptimParams op{};
  op.d = s->ds.d; op.S = choose_S(s, E, resolved_kernel(s)); op.dp = (s->ds.d + 3) / 4 * 4; op.kind = a->kind;
  op.lr = a->learning_rate; op.b1 = a->b1; op.b2 = a->b2; op.eps = a->eps; op.wd = a->weight_decay;
  op.inv_batch = 1.0f / (float)(s->win_count ? s->win_count : s->N);
  op.bc1 = (float)(1.0 - std::pow((double)a->b1, (double)a->t));
  op.bc2 = (float)(1.0 - std::pow((double)a->b2, (double)a->t));
  op.theta = theta; op.m = a->m; op.v = a->v; op.slabs = s->slabs; op.llpart = s->llpart; op.active = a->active; op.out_nll = a->out_nll;
  k_optim_step<<<dim3((op.d + 255) / 256, E), 256, 0, st>>>(op);
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

int32_t mile_init(mile_sampler *s, mile_state *state, const float *noise, uint64_t seed,
                  const int32_t *particle_ids, void *stream) {
  if (!s || !state || !state->position || !state->momentum || !state->logdensity || !state->logdensity_grad)
    return fail(MILE_ERR_INVALID, "mile_init: null state field");
  const int E = state->n_particles;
  if (E < 1) return fail(MILE_ERR_INVALID, "mile_init: n_particles must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  int rc = mile_logpost_grad(s, state->position, E, state->logdensity, state->logdensity_grad, stream);
  if (rc) return rc;
  k_init_momentum<<<E, AUX_NT, 0, st>>>(sample_dim(s), noise, seed, particle_ids, state->momentum);
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

int32_t mile_step(mile_sampler *s, mile_state *state, const mile_step_args *a, void *stream) {
  const char *dv = getenv("MILE_DEBUG");
  const bool no_prefill = dv && (atoi(dv) & 128);   // test hook: every launch draws its own noise, as before the prefill
  Mclmc m{};
  if (const int rc = mclmc_begin(s, state, a, "mile_step", m); rc || a->n_steps == 0) return rc;
  const int E = m.up.E, d = m.up.d;
  hipStream_t st = (hipStream_t)stream;

  // two launches per step when the updates can run as the grad kernel's epilogue (k_grad_w64 SPLIT), else four
  UpdParams probe = m.up;
  probe.zA = a->noise; probe.zB = a->noise; probe.out_sample = a->out_samples;
  const bool fused = fuse_ok(s, m.kernel, probe);
  if (fused) HIP_TRY(hipMemsetAsync(s->arrive, 0, ((size_t)E * 4 + 15) / 16 * 16, st));   // tickets re-zeroed every call
  // noise prefill of the record launches: only Philox calls with the register-cached update can prefill; they allocate the
  // workspace the first time
  const bool prefill = !fused && !a->noise && upd_fast_d(d) && !no_prefill;
  if (prefill && s->nz_E < E) {
    if (s->nzbuf) HIP_TRY(hipFree(s->nzbuf));
    s->nzbuf = nullptr;
    s->nz_E = 0;
    HIP_TRY(hipMalloc(&s->nzbuf, 2 * nz_stride(s->E_cap, d) * 4));
    s->nz_E = s->E_cap;
  }
  int kept = 0;
  for (int i = 0; i < a->n_steps; ++i) {
    if (i == 0) launch_update(upd_start(m, i), E, st);
    UpdParams ur = upd_record(m, i);
    if (i + 1 < a->n_steps) {
      chain_start(ur, m, i + 1);
      ur.flags |= UPD_NO_G;
    }
    const int64_t gstep = a->step_offset + i;
    if (a->out_samples && a->n_thinning > 0 && (gstep % a->n_thinning) == 0) ur.out_sample = a->out_samples + (size_t)kept++ * E * d;
    UpdParams u = upd_mid(m);
    // Philox noise of the record launch: drawn by E extra workgroups of this launch (the update kernel of the record launch
    // fills only E of the chip's CUs) and read back through the record launch's explicit-noise path -- the same numbers.
    if (prefill && update_prefills(u)) {
      ++s->nz_launches;
      if (!ur.zA) {
        u.nz_A = s->nzbuf; u.nz_stepA = ur.stepA; u.nz_stageA = ur.stageA;
        ur.zA = u.nz_A;
      }
      if ((ur.flags & UPD_OB) && !ur.zB) {
        u.nz_B = s->nzbuf + nz_stride(s->nz_E, d); u.nz_stepB = ur.stepB; u.nz_stageB = ur.stageB;
        ur.zB = u.nz_B;
      }
    }
    if (const int rc = grad_then_update(s, state->position, E, u, fused, st)) return rc;
    if (const int rc = grad_then_update(s, state->position, E, ur, fused, st)) return rc;
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

int32_t mile_tune(mile_sampler *s, mile_state *state, const mile_tune_args *a, void *stream) {
  // test hooks: the k_tune_post path at any d; the five-launch form of rounds 1-2; every chain through the merged launch's restart
  const bool post = getenv("MILE_TUNE_POST") != nullptr, no_merge = getenv("MILE_TUNE_NO_MERGE") != nullptr;
  const bool force_restart = getenv("MILE_TUNE_FORCE_RESTART") != nullptr;
  Mclmc m{};
  if (const int rc = mclmc_begin(s, state, a, "mile_tune", m); rc || a->n_steps == 0) return rc;
  const int E = m.up.E, d = m.up.d;
  const size_t Ed = (size_t)E * d;
  hipStream_t st = (hipStream_t)stream;

  struct Buf { float *x, *u, *g, *logp; };
  const Buf A{state->position, state->momentum, state->logdensity_grad, state->logdensity};
  const Buf B{s->alt_x, s->alt_u, s->alt_g, s->alt_logp};
  auto set_state = [](UpdParams &u, const Buf &b) { u.x = b.x; u.u = b.u; u.g = b.g; u.logp = b.logp; };

  if ((d >> 2) > UPD_NT * UPD_QMAX || post) {   // beyond k_update_fast's register cache
    // Large d: an ordinary in-place kernel step (two-pass update kernels), the previous state copied aside first,
    // then k_tune_post applies the predictor, the rejection of non-finite steps and the streaming averages.
    if (!s->tune_info) HIP_TRY(hipMalloc(&s->tune_info, (size_t)s->E_cap * 3 * 4));
    for (int i = 0; i < a->n_steps; ++i) {
      HIP_TRY(hipMemcpyAsync(B.x, A.x, Ed * 4, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(B.u, A.u, Ed * 4, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(B.g, A.g, Ed * 4, hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(B.logp, A.logp, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
      float *info_i = a->out_info ? a->out_info + (size_t)i * E * 3 : s->tune_info;
      launch_update(upd_start(m, i), E, st);
      if (const int rc = launch_grad(s, A.x, E, st)) return rc;
      launch_update(upd_mid(m), E, st);
      if (const int rc = launch_grad(s, A.x, E, st)) return rc;
      UpdParams ur = upd_record(m, i);
      ur.out_info = info_i;
      launch_update(ur, E, st);
      TunePostParams tp{};
      tp.d = d; tp.x = A.x; tp.u = A.u; tp.g = A.g; tp.logp = A.logp;
      tp.bk_x = B.x; tp.bk_u = B.u; tp.bk_g = B.g; tp.bk_logp = B.logp;
      tp.info = info_i;
      set_tuner(tp, a, a->schedule_step0 + i);
      k_tune_post<<<E, AUX_NT, 0, st>>>(tp);
    }
    HIP_TRY(hipGetLastError());
    return MILE_OK;
  }

  UpdParams probe = m.up;
  probe.x_in = B.x; probe.u_in = B.u; probe.g_in = B.g;
  probe.zA = a->noise; probe.t_avg = a->stream_average;
  if (a->n_steps > 1) probe.u_rec = A.u;
  const bool fused = fuse_ok(s, m.kernel, probe);
  if (fused) HIP_TRY(hipMemsetAsync(s->arrive, 0, ((size_t)E * 4 + 15) / 16 * 16, st));
  // Per step: grad . update(B, A) . grad . update(B, O, record + TUNE [. O, B, A of the next step with the NEW step size]) --
  // four launches, as a sampling step (mile_step).  Step i works in buffer W_i and leaves the accepted state there; its last
  // launch writes the next step's working position / momentum into the other buffer, which until then held the state before
  // step i (what handle_nans reverts to): W_{i+1} = K_i, K_{i+1} = W_i, no copies.
  for (int i = 0; i < a->n_steps; ++i) {
    const Buf &cur = (i & 1) ? B : A, &nxt = (i & 1) ? A : B;
    if (i == 0 || no_merge) {  // reads the current state, writes the other buffer (free backup)
      UpdParams u = upd_start(m, i);
      set_state(u, nxt);
      u.x_in = cur.x; u.u_in = cur.u; u.g_in = cur.g; u.logp_in = cur.logp;
      launch_update(u, E, st);
    }
    UpdParams u = upd_mid(m);
    set_state(u, nxt);
    if (const int rc = grad_then_update(s, nxt.x, E, u, fused, st)) return rc;
    // record + tuner (step-size predictor, handle_nans, streaming averages) [+ the next step's start]
    UpdParams ur = upd_record(m, i);
    set_state(ur, nxt);
    ur.flags |= UPD_TUNE;
    ur.bk_x = cur.x; ur.bk_u = cur.u; ur.bk_g = cur.g; ur.bk_logp = cur.logp;
    set_tuner(ur, a, a->schedule_step0 + i);
    if (i + 1 < a->n_steps && !no_merge) {
      chain_start(ur, m, i + 1);
      ur.x_in = nxt.x; ur.u_in = nxt.u;          // the step ran in nxt; its accepted state stays there ...
      ur.x_acc = nxt.x; ur.u_rec = nxt.u;
      ur.x = cur.x; ur.u = cur.u;                // ... and the next step's working state goes to the other buffer
      ur.force_restart = force_restart;
    }
    if (const int rc = grad_then_update(s, nxt.x, E, ur, fused, st)) return rc;
  }
  if (a->n_steps & 1) {   // the final state sits in the library's buffer
    HIP_TRY(hipMemcpyAsync(A.x, B.x, Ed * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(A.u, B.u, Ed * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(A.g, B.g, Ed * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(A.logp, B.logp, (size_t)E * 4, hipMemcpyDeviceToDevice, st));
  }
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

int32_t mile_debug_noise(mile_sampler *s, uint64_t seed, const int32_t *particle_ids, int32_t E,
                         int64_t step, int32_t stage, float *out, void *stream) {
  if (!s || !out || E < 1) return fail(MILE_ERR_INVALID, "mile_debug_noise: bad argument");
  HIP_TRY(hipSetDevice(s->device));
  k_debug_noise<<<E, AUX_NT, 0, (hipStream_t)stream>>>(sample_dim(s), seed, particle_ids, (uint32_t)step, (uint32_t)stage, out);
  HIP_TRY(hipGetLastError());
  return MILE_OK;
}

int64_t mile_debug_prefill_count(const mile_sampler *s) { return s ? s->nz_launches : -1; }

int32_t mile_nuts_reserve(mile_sampler *s, int32_t E, int32_t max_num_doublings) {
  if (!s || E < 1 || max_num_doublings < 1 || max_num_doublings > NUTS_MAX_DOUBLINGS)
    return fail(MILE_ERR_INVALID, "mile_nuts_reserve: E >= 1 and 1 <= max_num_doublings <= 12");
  if (s->part) return fail(MILE_ERR_INVALID, "mile_nuts_reserve: partition sampling with NUTS is not built");
  const int rc = mile_reserve(s, E);
  if (rc) return rc;
  if (E <= s->nuts_E && max_num_doublings <= s->nuts_M) return MILE_OK;
  const int En = std::max(E, s->nuts_E), Mn = std::max(max_num_doublings, s->nuts_M);
  free_nuts(s);
  const size_t Ed = (size_t)En * s->ds.d * 4;
  NutsBufs &b = s->nb;
  float **fs[] = {&b.T, &b.Ph, &b.xe[0], &b.xe[1], &b.pe[0], &b.pe[1], &b.ge[0], &b.ge[1], &b.psT, &b.psS, &b.xs, &b.gs};
  for (float **f : fs) HIP_TRY(hipMalloc(f, Ed));
  HIP_TRY(hipMalloc(&b.ck_r, Ed * Mn));
  HIP_TRY(hipMalloc(&b.ck_rs, Ed * Mn));
  HIP_TRY(hipMalloc(&b.chain, (size_t)En * sizeof(NutsChain)));
  HIP_TRY(hipMalloc(&b.count, 16));
  HIP_TRY(hipMemset(b.T, 0, Ed));   // rows of chains outside a launch are never read uninitialised by the grad kernels
  if (!s->nuts_count_h) HIP_TRY(hipHostMalloc((void **)&s->nuts_count_h, 16, hipHostMallocDefault));
  s->nuts_E = En; s->nuts_M = Mn;
  return MILE_OK;
}

// n_steps NUTS steps (and, with `w`, one window-adaptation update after each), all chains in lockstep.
static int nuts_run(mile_sampler *s, mile_state *state, const mile_nuts_args *a, const mile_nuts_adapt_args *w, void *stream) {
  const char *fn = w ? "mile_nuts_warmup" : "mile_nuts_step";
  if (!s || !state || !a) return fail(MILE_ERR_INVALID, std::string(fn) + ": null argument");
  if (s->part) return fail(MILE_ERR_INVALID, std::string(fn) + ": partition sampling with NUTS is not built");
  if (!state->position || !state->logdensity || !state->logdensity_grad) return fail(MILE_ERR_INVALID, std::string(fn) + ": null state field");
  const int E = state->n_particles, d = s->ds.d, M = a->max_num_doublings;
  if (E < 1 || a->n_steps < 0) return fail(MILE_ERR_INVALID, std::string(fn) + ": n_particles >= 1 and n_steps >= 0");
  if (M < 1 || M > NUTS_MAX_DOUBLINGS) return fail(MILE_ERR_INVALID, std::string(fn) + ": 1 <= max_num_doublings <= 12");
  if (w) {
    if (!w->step_size || !w->inverse_mass_matrix || !w->da || !w->welford || !w->welford_count || !w->schedule)
      return fail(MILE_ERR_INVALID, "mile_nuts_warmup: null adaptation field");
  } else if (!a->step_size || !a->inverse_mass_matrix) {
    return fail(MILE_ERR_INVALID, "mile_nuts_step: step_size and inverse_mass_matrix are required");
  }
  if (!s->X) return fail(MILE_ERR_STATE, "no data: call mile_set_data first");
  if (E > s->nuts_E || M > s->nuts_M) return fail(MILE_ERR_STATE, std::string(fn) + ": call mile_nuts_reserve(E, max_num_doublings) first");
  if (tables_missing(s)) return fail(MILE_ERR_STATE, kNoTables);
  if (a->n_steps == 0) return MILE_OK;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(hipSetDevice(s->device));
  const int kernel = resolved_kernel(s);
  const int S = choose_S(s, E, kernel);
  if (E > s->E_cap || (size_t)E * S > s->ES_cap) return fail(MILE_ERR_STATE, "workspace too small: call mile_reserve(E) first");
  NutsParams p{};
  p.d = d; p.dp = (d + 3) / 4 * 4; p.S = S; p.E = E; p.M = M; p.prior = s->ds.prior;
  p.loc = s->ds.prior_loc; p.scale = s->ds.prior_scale; p.thr = a->divergence_threshold;
  p.slabs = s->slabs; p.llpart = s->llpart;
  p.x = state->position; p.g = state->logdensity_grad; p.logp = state->logdensity;
  p.eps = w ? w->step_size : a->step_size;
  p.m = w ? w->inverse_mass_matrix : a->inverse_mass_matrix;
  p.NU = 2 * M + (1 << M);
  p.seed = a->seed; p.pids = a->particle_ids; p.b = s->nb;
  const size_t Ed = (size_t)E * d;
  int64_t rounds = 0, syncs = 0;
  int kept = 0;
  for (int i = 0; i < a->n_steps; ++i) {
    const int64_t gstep = a->step_offset + i;
    p.gstep = (uint32_t)gstep;
    p.z = a->momentum_noise ? a->momentum_noise + (size_t)i * Ed : nullptr;
    p.unif = a->uniforms ? a->uniforms + (size_t)i * E * p.NU : nullptr;
    p.out_info = a->out_info ? a->out_info + (size_t)i * E * NUTS_INFO : nullptr;
    p.out_sample = nullptr;
    if (a->out_samples && a->n_thinning > 0 && (gstep % a->n_thinning) == 0) p.out_sample = a->out_samples + (size_t)(kept++) * Ed;
    k_nuts_begin<<<E, NUTS_NT, 0, st>>>(p);
    HIP_TRY(hipGetLastError());
    for (int j = 0; j < M; ++j) {
      p.sub_len = 1 << j;
      for (int k = 0; k < p.sub_len; ++k) {   // one round: every chain still in its subtree takes one leapfrog step
        const int rc = launch_grad(s, s->nb.T, E, st);
        if (rc) return rc;
        p.leaf = k;
        k_nuts_leaf<<<E, NUTS_NT, 0, st>>>(p);
        HIP_TRY(hipGetLastError());
        ++rounds;
      }
      HIP_TRY(hipMemsetAsync(s->nb.count, 0, 4, st));
      k_nuts_merge<<<E, NUTS_NT, 0, st>>>(p);
      HIP_TRY(hipGetLastError());
      if (j == M - 1) break;   // every chain has stopped
      HIP_TRY(hipMemcpyAsync(s->nuts_count_h, s->nb.count, 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      ++syncs;
      if (*s->nuts_count_h == 0) break;
    }
    if (w) {
      NutsAdaptParams ap{};
      ap.d = d; ap.stage = w->schedule[2 * i]; ap.window_end = w->schedule[2 * i + 1]; ap.target = w->target_acceptance_rate;
      ap.x = state->position; ap.chain = s->nb.chain; ap.step_size = w->step_size; ap.imm = w->inverse_mass_matrix;
      ap.da = w->da; ap.wf = w->welford; ap.wf_n = w->welford_count;
      k_nuts_adapt<<<E, NUTS_NT, 0, st>>>(ap);
      HIP_TRY(hipGetLastError());
    }
  }
  if (a->out_stats) { a->out_stats[0] += rounds; a->out_stats[1] += syncs; }
  return MILE_OK;
}

int32_t mile_nuts_step(mile_sampler *s, mile_state *state, const mile_nuts_args *a, void *stream) {
  return nuts_run(s, state, a, nullptr, stream);
}

int32_t mile_nuts_warmup(mile_sampler *s, mile_state *state, const mile_nuts_args *a, const mile_nuts_adapt_args *w, void *stream) {
  if (!w) return fail(MILE_ERR_INVALID, "mile_nuts_warmup: null adaptation state");
  return nuts_run(s, state, a, w, stream);
}

}  // extern "C"

// Function-space diagnostics kernels (mile_fdiag.h) in a translation unit of their own: they compile concurrently with
// mile_hip.hip.
#include <hip/hip_runtime.h>

#include <math.h>

#include "mile_row_head.h"
#include "mile_fdiag.h"

// ---- k_fdiag_pack: block (32, 8), grid (ceil(D / 32), ceil(nt / RT)), RT = ceil(32 / O) rows -----------------------------------
// A workgroup takes 32 draws x RT rows.  Each draw's RT * O head outputs are one contiguous run of the raw block: a row of
// `in`.  A thread then forms the Q quantities of one (draw, row) from LDS and puts them into `ot` [column][draw], whose rows go
// out as runs of 32 consecutive s.  Both tiles are padded by one float: within a half-wave (32 draws of one row) the
// per-(draw, row) reads of `in` (stride 65) and the writes of `ot` (stride 33) touch 32 different banks.  The two halves of a
// wave work on neighbouring rows and may meet on a bank; 32-bit LDS accesses are banked per half-wave, so that costs nothing.
// With O >= 33 a workgroup holds one row and only 32 of its 256 threads form quantities, each with a serial softmax.
__global__ __launch_bounds__(256) void k_fdiag_pack(const FdiagParams p) {
  __shared__ float in[FDIAG_DT][FDIAG_IN_MAX + 1];
  __shared__ float ot[FDIAG_OUT_MAX][FDIAG_DT + 1];
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * FDIAG_DT + tx;
  const int O = p.O, Q = p.Q, RT = (FDIAG_DT + O - 1) / O;
  const long long d0 = (long long)blockIdx.x * FDIAG_DT;
  const int r0 = blockIdx.y * RT, nr = min(RT, p.nt - r0), W = nr * O;
  for (int j = ty; j < FDIAG_DT; j += 8) {
    const long long d = d0 + j;
    if (d >= p.D) break;
    const float *src = p.out + ((size_t)d * p.nt + r0) * O;
    for (int i = tx; i < W; i += FDIAG_DT) in[j][i] = src[i];
  }
  __syncthreads();
  for (int w = tid; w < FDIAG_DT * nr; w += 256) {
    const int j = w & (FDIAG_DT - 1), r = w / FDIAG_DT;
    if (d0 + j >= p.D) continue;
    const float *z = &in[j][r * O];
    const int q0 = r * Q;
    if (p.task == MILE_TASK_REGRESSION) {
      for (int k = 0; k < O; ++k) ot[q0 + k][j] = z[k];          // (mu, log sigma) as mile_predict writes them
    } else {
      float m = z[0];                                            // the m and se of row_loglik
      for (int k = 1; k < O; ++k) m = fmaxf(m, z[k]);
      float se = 0.0f;
      for (int k = 0; k < O; ++k) se += expf(z[k] - m);
      const float lse = m + logf(se);
      for (int k = 0; k < O; ++k) ot[q0 + k][j] = expf(z[k] - lse);
    }
    if (p.y) ot[q0 + O][j] = row_loglik(z, O, p.task, p.y, r0 + r);
  }
  __syncthreads();
  const long long d = d0 + tx;
  if (d < p.D)
    for (int q = ty; q < nr * Q; q += 8) p.raw[((size_t)r0 * Q + q) * p.D + d] = ot[q][tx];
}

// ---- k_fdiag_lp: one thread per draw, the tile's rows in order ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fdiag_lp(const FdiagParams p) {
  const long long d = (long long)blockIdx.x * 256 + threadIdx.x;
  if (d >= p.D) return;
  double a = p.acc[d];
  const float *l = p.raw + (size_t)p.O * p.D + d;                // column r * Q + O of row r
  for (int r = 0; r < p.nt; ++r) a += (double)l[(size_t)r * p.Q * p.D];
  p.acc[d] = a;
  if (p.lcol) p.lcol[d] = (float)a;
}

// ---- k_fdiag_summary: stage 1 grid (2C + 1, B), stage 2 one workgroup ------------------------------------------------------------
// Series j: 0 rhat, 1 .. C the chains' crhat, C + 1 .. 2C the chains' ess.  Of equal extremes the lower column wins.
__device__ __forceinline__ void fdiag_merge(FdiagPart &a, const FdiagPart &b) {
  if (b.imx >= 0 && (a.imx < 0 || b.mx > a.mx || (b.mx == a.mx && b.imx < a.imx))) { a.mx = b.mx; a.imx = b.imx; }
  if (b.imn >= 0 && (a.imn < 0 || b.mn < a.mn || (b.mn == a.mn && b.imn < a.imn))) { a.mn = b.mn; a.imn = b.imn; }
  a.sum += b.sum; a.nfin += b.nfin; a.nskip += b.nskip; a.g1 += b.g1; a.g2 += b.g2; a.g3 += b.g3;
}
__device__ __forceinline__ FdiagPart fdiag_empty() {
  FdiagPart e;
  e.mx = e.mn = e.sum = 0.0;
  e.imx = e.imn = -1;
  e.nfin = e.nskip = e.g1 = e.g2 = e.g3 = 0;
  return e;
}
__device__ __forceinline__ const float *fdiag_series(const FdiagSumParams &p, int j) {
  if (j == 0) return p.rhat;
  return j <= p.C ? p.crhat + (size_t)(j - 1) * p.M : p.ess + (size_t)(j - 1 - p.C) * p.M;
}

__global__ __launch_bounds__(FDIAG_SUM_NT) void k_fdiag_summary(const FdiagSumParams p, int stage) {
  __shared__ FdiagPart red[FDIAG_SUM_NT];
  const int tid = threadIdx.x, nser = 2 * p.C + 1;
  if (stage == 1) {
    const int j = blockIdx.x, b = blockIdx.y;
    const float *src = fdiag_series(p, j);
    const long long chunk = (p.NQ + p.B - 1) / p.B, lo = b * chunk, hi = min(p.NQ, lo + chunk);
    FdiagPart a = fdiag_empty();
    for (long long i = lo + tid; i < hi; i += FDIAG_SUM_NT) {
      const double v = (double)src[i];
      if (!(fabs(v) <= 1.79769313486231570e+308)) { a.nskip++; continue; }
      if (a.imx < 0 || v > a.mx) { a.mx = v; a.imx = i; }
      if (a.imn < 0 || v < a.mn) { a.mn = v; a.imn = i; }
      a.sum += v; a.nfin++;
      a.g1 += v > 1.01; a.g2 += v > 1.05; a.g3 += v > 1.1;
    }
    red[tid] = a;
    __syncthreads();
    for (int o = FDIAG_SUM_NT >> 1; o > 0; o >>= 1) {
      if (tid < o) fdiag_merge(red[tid], red[tid + o]);
      __syncthreads();
    }
    if (tid == 0) p.part[(size_t)j * p.B + b] = red[0];
    return;
  }
  FdiagPart *tot = p.part + (size_t)nser * p.B;
  for (int j = tid; j < nser; j += FDIAG_SUM_NT) {
    FdiagPart a = fdiag_empty();
    for (int b = 0; b < p.B; ++b) fdiag_merge(a, p.part[(size_t)j * p.B + b]);
    tot[j] = a;
  }
  __syncthreads();
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  if (p.chain_summary)
    for (int c = tid; c < p.C; c += FDIAG_SUM_NT) {
      const FdiagPart &e = tot[1 + p.C + c], &r = tot[1 + c];
      p.chain_summary[2 * c] = e.imn >= 0 ? e.mn : qnan;
      p.chain_summary[2 * c + 1] = r.imx >= 0 ? r.mx : qnan;
    }
  if (tid != 0 || !p.summary) return;
  double *o = p.summary;
  const FdiagPart &r = tot[0];
  o[FDIAG_RHAT_MAX] = r.imx >= 0 ? r.mx : qnan;
  o[FDIAG_RHAT_MEAN] = r.nfin ? r.sum / (double)r.nfin : qnan;
  o[FDIAG_RHAT_COLUMN] = (double)r.imx;
  o[FDIAG_RHAT_GT_1_01] = (double)r.g1; o[FDIAG_RHAT_GT_1_05] = (double)r.g2; o[FDIAG_RHAT_GT_1_1] = (double)r.g3;
  o[FDIAG_RHAT_SKIPPED] = (double)r.nskip;
  double cmx = qnan, emn = qnan, esum = 0.0;
  long long cc = -1, ci = -1, ec = -1, ei = -1, cskip = 0, eskip = 0, efin = 0;
  for (int c = 0; c < p.C; ++c) {                                 // chains in index order: of equal extremes the lower chain wins
    const FdiagPart &a = tot[1 + c], &e = tot[1 + p.C + c];
    if (a.imx >= 0 && (cc < 0 || a.mx > cmx)) { cmx = a.mx; cc = c; ci = a.imx; }
    if (e.imn >= 0 && (ec < 0 || e.mn < emn)) { emn = e.mn; ec = c; ei = e.imn; }
    cskip += a.nskip; eskip += e.nskip; efin += e.nfin; esum += e.sum;
  }
  o[FDIAG_CRHAT_MAX] = cmx; o[FDIAG_CRHAT_CHAIN] = (double)cc; o[FDIAG_CRHAT_COLUMN] = (double)ci; o[FDIAG_CRHAT_SKIPPED] = (double)cskip;
  o[FDIAG_ESS_MIN] = emn; o[FDIAG_ESS_MEAN] = efin ? esum / (double)efin : qnan;
  o[FDIAG_ESS_CHAIN] = (double)ec; o[FDIAG_ESS_COLUMN] = (double)ei; o[FDIAG_ESS_SKIPPED] = (double)eskip;
}

hipError_t mile_launch_fdiag_pack(const FdiagParams &p, hipStream_t st) {
  const int RT = fdiag_pack_rows(p.O);
  const dim3 grid((unsigned)((p.D + FDIAG_DT - 1) / FDIAG_DT), (unsigned)((p.nt + RT - 1) / RT));
  k_fdiag_pack<<<grid, dim3(FDIAG_DT, 8), 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_fdiag_lp(const FdiagParams &p, hipStream_t st) {
  k_fdiag_lp<<<(unsigned)((p.D + 255) / 256), 256, 0, st>>>(p);
  return hipGetLastError();
}

hipError_t mile_launch_fdiag_summary(const FdiagSumParams &p, hipStream_t st) {
  k_fdiag_summary<<<dim3(2 * p.C + 1, p.B), FDIAG_SUM_NT, 0, st>>>(p, 1);
  k_fdiag_summary<<<1, FDIAG_SUM_NT, 0, st>>>(p, 2);
  return hipGetLastError();
}

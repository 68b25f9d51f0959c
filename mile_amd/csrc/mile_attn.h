// AttentionClassifier target (src/models/text/attention_classifier.py), fp32 (MILE_GRAD_ATTN_F32):
//   x [T] token ids -> e = Embedding[x] + PositionEmbedding[0..T) -> MultiHeadDotProductAttention 'MDPA' (H heads of hd = D / H,
//   q / sqrt(hd), mask = outer(x != 0, x != 0), where(mask, s, finfo.min), softmax over keys) -> out Dense [H, hd] -> C
//   -> mean over all T positions -> (Dense P_i -> gelu (tanh form)) per projection -> Dense K 'classifier'
// One fused forward + backward launch per gradient: k_grad_attn, grid (S row ranges, E chains), 256 threads (4 waves), one
// sequence at a time.  LDS holds the chain's Wq|Wk|Wv [C][3D] (when it fits; WL), the sequence's q|k|v [Tp][3D] (Tp = T rounded
// up to 16; positions T..Tp are no tokens and carry weight 0), and a [64][Tp] scratch: the embedded input e [Tp][C] while the
// projections run, one [16][Tp] dS tile per wave during the attention.  Every product runs on v_mfma_f32_16x16x4_f32 through
// attn_tile (fp32 operands read from LDS with bounds guards, k-ordered fp32 accumulation).
//   - q|k|v = e [Wq|Wk|Wv] (+ b): output tiles round-robin over the waves.
//   - Attention: wave w owns heads w, w + 4, ...  A 16-query-row tile's scores S [16][Tp] live in registers (<= 8 tiles of 4),
//     masked and softmaxed there with 16-lane shuffles.  Mean pooling is linear, so mean_t(o_t) Wo = (mean_t o_t) Wo and
//     mean_t o_t = (1/T) sum_j colsum_j(P) v_j: the forward keeps only the column sums of P.
//   - The Dense tail (Wo, projections, classifier, head) runs on vectors in LDS, one thread per unit.
//   - Backward: the upstream gradient of every o_t is dobar / T, so dP_ij = u_j = (dobar_h / T) . v_j for every query row,
//     dV_j = (dobar_h / T) colsum_j, dS_ij = P_ij (u_j - sum_j' P_ij' u_j') -- zero on pad query rows (where() drops their
//     gradient) and on pad keys (P = 0).  The scores are recomputed per tile; dS goes through the wave's scratch to form
//     dQ (tile rows, written over q) and dK (accumulated in registers over the query tiles, written over k at the end).
//   - dW_qkv = e^T [dq|dk|dv] and dPos = de accumulate in registers over all of the workgroup's sequences (static tile
//     ownership per wave); de = [dq|dk|dv] W^T rows are scatter-added into the slab's [V][C] embedding block with
//     global_atomic_add_f32 (each workgroup zero-fills its own slab's block first).
// k_fwd_attn is the forward half: per-row log-likelihoods for mile_pointwise_loglik.
#pragma once
#include "mile_device.h"

#define ATTN_NT 256
#define ATTN_MAX_T 128       // Tp / 16 <= 8 key tiles in registers
#define ATTN_MAX_C 64        // e [Tp][C] fits the [64][Tp] scratch
#define ATTN_MAX_D 64
#define ATTN_MAX_P 64        // projection widths: one thread per unit, <= 64 x 64 tail matrices
#define ATTN_MAX_NP 2
#define ATTN_MAX_K 16
#define ATTN_LDS_MAX (160 * 1024)

struct AttnGeom {
  int V, T, C, H, D, hd, K, NP, P[ATTN_MAX_NP], bias, Tp;
  // parameter offsets in the raveled vector (ravel_pytree order, see mile_hip.h); bias offsets are -1 without bias
  int b_k, k_k, b_o, k_o, b_q, k_q, b_v, k_v, emb, pos, b_c, k_c, b_p[ATTN_MAX_NP], k_p[ATTN_MAX_NP], d;
};

struct AttnParams {
  AttnGeom g;
  const float *theta;   // [E, d] (gradient) or [S, d] (evaluation)
  const float *X;       // [N, T] token ids as fp32
  const void *y;        // [N] int32 labels
  const float *emb;     // [V, C] frozen token table (mile_attn_pre.h); null where the tables are inside theta (g.emb / g.pos)
  const float *pos;     // [T, C] frozen position rows, likewise
  float *slabs;         // [E, S, dp] likelihood-gradient slabs (gradient)
  float *llpart;        // [E, S] (gradient)
  float *out;           // [S, N] per-row log-likelihoods (evaluation); RAW: [S, N, K] logits, y unread
  int N, S, dp;
};

// LDS floats: [W (C x 3D) if WL] QKV [Tp][3D] | scratch | vectors.  Scratch: e [Tp][C], or per busy wave a dS tile [16][Tp]
// and, for hd > 16 (dK too large for registers), the head's dK [Tp][16 ceil(hd / 16)]
__host__ __device__ inline int attn_vec_floats(int Tp) { return 5 * Tp + 10 * 64 + 16; }
__host__ __device__ inline int attn_scr_wave(const AttnGeom &g) { return 16 * g.Tp + (g.hd > 16 ? g.Tp * ((g.hd + 15) / 16 * 16) : 0); }
__host__ __device__ inline int attn_scr_floats(const AttnGeom &g) {
  const int w = g.H < 4 ? g.H : 4, a = 64 * g.Tp, b = w * attn_scr_wave(g);
  return a > b ? a : b;
}
__host__ __device__ inline size_t attn_lds_bytes(const AttnGeom &g, bool wl) {
  return ((size_t)(wl ? g.C * 3 * g.D : 0) + (size_t)g.Tp * 3 * g.D + attn_scr_floats(g) + attn_vec_floats(g.Tp)) * 4;
}
__host__ __device__ inline bool attn_weights_in_lds(const AttnGeom &g) { return attn_lds_bytes(g, true) <= ATTN_LDS_MAX; }

__device__ __forceinline__ f32x4 attn_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// lane-ordered LDS traffic inside one wave: the wave's own stores are visible to its later loads
__device__ __forceinline__ void attn_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// One 16x16 tile += A[16][Kd] B[Kd][16]; a(m, k) / b(k, n) return the operands (0 where out of range).
// Lane l supplies A[l & 15][k0 + (l >> 4)] and B[k0 + (l >> 4)][l & 15]; the result holds rows 4 (l >> 4) + r, column l & 15.
template <class FA, class FB>
__device__ __forceinline__ f32x4 attn_tile(int Kd, FA a, FB b, f32x4 acc) {
  const int lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
  for (int k0 = 0; k0 < Kd; k0 += 4) {
    const int k = k0 + kq;
    const bool ok = k < Kd;
    acc = attn_mfma(ok ? a(m, k) : 0.0f, ok ? b(k, m) : 0.0f, acc);
  }
  return acc;
}

__device__ __forceinline__ float attn_gelu(float x) {
  const float c = 0.7978845608028654f;   // sqrt(2 / pi)
  return 0.5f * x * (1.0f + tanhf(c * fmaf(0.044715f * x, x * x, x)));
}
__device__ __forceinline__ float attn_gelu_grad(float x) {
  const float c = 0.7978845608028654f;
  const float th = tanhf(c * fmaf(0.044715f * x, x * x, x));
  return 0.5f * (1.0f + th) + 0.5f * x * (1.0f - th * th) * c * fmaf(3.0f * 0.044715f, x * x, 1.0f);
}

// Probabilities of query tile `it` of head h: pr[jt][r] = P[it*16 + 4 (lane >> 4) + r][jt*16 + (lane & 15)].
// Rows past T are 0; pad query rows are uniform 1/T over the T real positions; pad keys of real rows are 0.
template <int NJ>
__device__ __forceinline__ void attn_probs(const float *QKV, int ld, const int *tok, int T, int D, int hd, int it, int h, f32x4 (&pr)[NJ],
                                           int nj) {
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const float *Q = QKV + h * hd, *Kt = QKV + D + h * hd;
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
    pr[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (jt < nj)
      pr[jt] = attn_tile(hd, [&](int m, int k) { return Q[(it * 16 + m) * ld + k]; },
                         [&](int k, int n) { return Kt[(jt * 16 + n) * ld + k]; }, pr[jt]);
  }
  bool kv[NJ];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) {
    const int j = jt * 16 + col;
    kv[jt] = jt < nj && j < T && tok[j] != 0;
  }
  const float invT = 1.0f / (float)T;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = it * 16 + 4 * kq + r;
    const int tq = i < T ? tok[i] : -1;
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
      if (kv[jt]) mx = fmaxf(mx, pr[jt][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 1)); mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4)); mx = fmaxf(mx, __shfl_xor(mx, 8));
    float se = 0.0f;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
      const float ev = kv[jt] ? expf(pr[jt][r] - mx) : 0.0f;
      pr[jt][r] = ev;
      se += ev;
    }
    se += __shfl_xor(se, 1); se += __shfl_xor(se, 2); se += __shfl_xor(se, 4); se += __shfl_xor(se, 8);
    const float inv = tq > 0 ? 1.0f / se : 0.0f;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
      const int j = jt * 16 + col;
      pr[jt][r] = tq > 0 ? pr[jt][r] * inv : (tq == 0 && j < T ? invT : 0.0f);
    }
  }
}

// ---- The blocks that attn_body (below) and attnp_body (mile_attn_pre.h) share: each exists once, here.  The workgroup barriers
// between them stay in the bodies; the in-wave LDS ordering (attn_wave_sync) is inside.  What stays per kernel, because it is
// not the same code: the Dense tail forward and backward (vectors at stride 64 against packed, `#pragma unroll 8`, accumulators
// in registers against the slab row), the q | k | v product (LDS operands through attn_tile against the software-pipelined L2
// form), and dW_qkv, de and the slab write-out.

// tok[t] = the sequence's token ids clamped to [0, V), -1 for t in [T, Tp)
__device__ __forceinline__ void attn_stage_tokens(int *tok, const float *X, int row, int T, int Tp, int V) {
  for (int t = threadIdx.x; t < Tp; t += ATTN_NT) {
    int v = -1;
    if (t < T) v = min(max((int)X[(size_t)row * T + t], 0), V - 1);
    tok[t] = v;
  }
}

// e [Tp][C] = embt[tok] + post (token table [V][C], position rows [T][C]), rows past T zero.  V C < 2^32 (V <= 2^24, C <= 192)
__device__ __forceinline__ void attn_stage_e(float *e, const int *tok, const float *embt, const float *post, int T, int Tp, int C) {
  for (int i = threadIdx.x; i < Tp * C; i += ATTN_NT) {
    const int t = i / C, c = i - t * C;
    e[i] = t < T ? embt[(size_t)tok[t] * C + c] + post[t * C + c] : 0.0f;
  }
}

// Attention forward of head h, by one wave: obar[h hd ..) = invT sum_j colsum_j(P) v_j, invT = 1 / T.  Its scalars are arguments
// and attn_bwd_head reads its own from the geometry: other forms spill in k_grad_attn<1, *> or cost k_out_attn a wave per SIMD
// (profiles/r08/01_attn_shared_blocks.md).  attnp_body<WIDE> keeps this text in place of the call, for speed.
template <int NJ>
__device__ __forceinline__ void attn_fwd_head(const float *QKV, int ld, const int *tok, int T, int D, int hd, int h, int nj, float invT,
                                              float *obar) {
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  float cs[NJ];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) cs[jt] = 0.0f;
  for (int it = 0; it < nj; ++it) {
    f32x4 pr[NJ];
    attn_probs<NJ>(QKV, ld, tok, T, D, hd, it, h, pr, nj);
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) cs[jt] += (pr[jt][0] + pr[jt][1]) + (pr[jt][2] + pr[jt][3]);
  }
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) { cs[jt] += __shfl_xor(cs[jt], 16); cs[jt] += __shfl_xor(cs[jt], 32); }
  for (int d0 = 0; d0 < hd; d0 += 4) {
    const int dd = d0 + kq;
    float a = 0.0f;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
      if (jt < nj && dd < hd) a = fmaf(cs[jt], QKV[(jt * 16 + col) * ld + 2 * D + h * hd + dd], a);
    a += __shfl_xor(a, 1); a += __shfl_xor(a, 2); a += __shfl_xor(a, 4); a += __shfl_xor(a, 8);
    if (col == 0 && dd < hd) obar[h * hd + dd] = a * invT;
  }
}

// The head, by wave 0 (tid < 64): log softmax of the logits lg [K] at the label.  !GRAD: the row's log-likelihood goes to
// *out_ll.  GRAD: lg becomes d(ll) / d(logits), zero for a row whose ll is NaN (`bad`; the caller leaves it out of its sum).
struct AttnHead { float ll; bool bad; };
template <bool GRAD>
__device__ __forceinline__ AttnHead attn_head(float *lg, int K, int yi, float *out_ll) {
  const int tid = threadIdx.x;
  float mx = -INFINITY;
  for (int k = 0; k < K; ++k) mx = fmaxf(mx, lg[k]);
  float se = 0.0f;
  for (int k = 0; k < K; ++k) se += expf(lg[k] - mx);
  const float lse = mx + logf(se);
  const float ll = lg[min(max(yi, 0), K - 1)] - lse;
  const bool bad = isnan(ll);
  const float dl = (bad || tid >= K) ? 0.0f : ((tid == yi ? 1.0f : 0.0f) - expf(lg[min(tid, K - 1)] - lse));
  if (!GRAD && tid == 0) *out_ll = ll;
  if (GRAD) {
    __builtin_amdgcn_wave_barrier();
    if (tid < K) lg[tid] = dl;
  }
  return {ll, bad};
}

// Attention backward of head h, by one wave.  In: q' | k | v of the head in QKV [Tp][3D], dobar [D].
// Out: dq (pre-scale) | dK | dV over them.  The wave's scratch, carved out by the caller: dS [16][Tp], u [Tp], and for NHT > 1
// (dK too large for registers) dKl [Tp][16 NHT].
template <int NJ, int NHT>
__device__ __forceinline__ void attn_bwd_head(const AttnGeom &g, float *QKV, const int *tok, int h, const float *dobar, float *dS, float *u,
                                              float *dKl) {
  constexpr bool DKL = NHT > 1;                      // dK in the wave's scratch, not in registers
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
  const int T = g.T, Tp = g.Tp, D = g.D, hd = g.hd, ld = 3 * D, nj = Tp / 16;
  const float scale = 1.0f / sqrtf((float)hd), invT = 1.0f / (float)T;
  if (DKL) {
    for (int i = lane; i < Tp * 16 * NHT; i += 64) dKl[i] = 0.0f;
  }
  for (int j = lane; j < Tp; j += 64) {
    float a = 0.0f;
    for (int dd = 0; dd < hd; ++dd) a = fmaf(dobar[h * hd + dd], QKV[j * ld + 2 * D + h * hd + dd], a);
    u[j] = a * invT;
  }
  attn_wave_sync();
  float cs[NJ];
  f32x4 dk[NJ];
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) { cs[jt] = 0.0f; dk[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; }
  for (int it = 0; it < nj; ++it) {
    f32x4 pr[NJ];
    attn_probs<NJ>(QKV, ld, tok, T, D, hd, it, h, pr, nj);
    float uj[NJ];
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) uj[jt] = jt < nj ? u[jt * 16 + col] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = it * 16 + 4 * kq + r;
      const bool real = i < T && tok[i] > 0;
      float rs = 0.0f;
#pragma unroll
      for (int jt = 0; jt < NJ; ++jt) rs = fmaf(pr[jt][r], uj[jt], rs);
      rs += __shfl_xor(rs, 1); rs += __shfl_xor(rs, 2); rs += __shfl_xor(rs, 4); rs += __shfl_xor(rs, 8);
#pragma unroll
      for (int jt = 0; jt < NJ; ++jt) {
        cs[jt] += pr[jt][r];
        if (jt < nj) dS[(4 * kq + r) * Tp + jt * 16 + col] = real ? pr[jt][r] * (uj[jt] - rs) : 0.0f;
      }
    }
    attn_wave_sync();
    const float *Qh = QKV + h * hd, *Kh = QKV + D + h * hd;
    // dK[j] += sum_i dS[i][j] q'[i] over this tile's rows
    if (!DKL) {
#pragma unroll
      for (int jt = 0; jt < NJ; ++jt)
        if (jt < nj)
          dk[jt] = attn_tile(16, [&](int m, int k) { return dS[k * Tp + jt * 16 + m]; },
                             [&](int k, int n) { return n < hd ? Qh[(it * 16 + k) * ld + n] : 0.0f; }, dk[jt]);
    } else {
      for (int jt = 0; jt < nj; ++jt)
#pragma unroll
        for (int q = 0; q < NHT; ++q) {
          f32x4 a;
#pragma unroll
          for (int r = 0; r < 4; ++r) a[r] = dKl[(jt * 16 + 4 * kq + r) * 16 * NHT + q * 16 + col];
          a = attn_tile(16, [&](int m, int k) { return dS[k * Tp + jt * 16 + m]; },
                        [&](int k, int n) { return q * 16 + n < hd ? Qh[(it * 16 + k) * ld + q * 16 + n] : 0.0f; }, a);
#pragma unroll
          for (int r = 0; r < 4; ++r) dKl[(jt * 16 + 4 * kq + r) * 16 * NHT + q * 16 + col] = a[r];
        }
    }
    // dq (pre-scale) = dS K / sqrt(hd) for this tile's rows, written over q'
    f32x4 dq[NHT];
#pragma unroll
    for (int q = 0; q < NHT; ++q)
      dq[q] = attn_tile(Tp, [&](int m, int k) { return dS[m * Tp + k]; },
                        [&](int k, int n) { return q * 16 + n < hd ? Kh[k * ld + q * 16 + n] : 0.0f; }, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
    attn_wave_sync();
#pragma unroll
    for (int q = 0; q < NHT; ++q)
      if (q * 16 + col < hd)
#pragma unroll
        for (int r = 0; r < 4; ++r) QKV[(it * 16 + 4 * kq + r) * ld + h * hd + q * 16 + col] = dq[q][r] * scale;
    attn_wave_sync();
  }
#pragma unroll
  for (int jt = 0; jt < NJ; ++jt) { cs[jt] += __shfl_xor(cs[jt], 16); cs[jt] += __shfl_xor(cs[jt], 32); }
  // dV[j] = (dobar_h / T) colsum_j; dK written over k
  for (int d0 = 0; d0 < hd; d0 += 4) {
    const int dd = d0 + kq;
    if (dd < hd) {
      const float gdd = dobar[h * hd + dd] * invT;
#pragma unroll
      for (int jt = 0; jt < NJ; ++jt)
        if (jt < nj) QKV[(jt * 16 + col) * ld + 2 * D + h * hd + dd] = gdd * cs[jt];
    }
  }
  if (!DKL) {
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt)
      if (jt < nj && col < hd)
#pragma unroll
        for (int r = 0; r < 4; ++r) QKV[(jt * 16 + 4 * kq + r) * ld + D + h * hd + col] = dk[jt][r];
  } else {
    attn_wave_sync();
    for (int i = lane; i < Tp * hd; i += 64) {
      const int j = i / hd, dd = i - j * hd;
      QKV[j * ld + D + h * hd + dd] = dKl[j * 16 * NHT + dd];
    }
  }
}

// NHT: ceil(hd / 16) (dK register tiles per key tile); WL: Wq|Wk|Wv staged in LDS
// RAW (evaluation only): the logits go to out[e][row][K] and the head is skipped, y unread (mile_predict)
template <int NHT, bool WL, bool GRAD, bool RAW = false>
__device__ __forceinline__ void attn_body(const AttnParams &p) {
  constexpr int NJ = ATTN_MAX_T / 16, NDW = 12, NDP = 8, NFW = ATTN_MAX_P / 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const AttnGeom &g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the tile bookkeeping stays in SGPRs
  const int q4 = tid >> 6;                                     // tail: thread (q4, lane) owns rows q4 + 4m, column lane
  const int e = blockIdx.y, s = blockIdx.x;
  const int T = g.T, C = g.C, H = g.H, D = g.D, hd = g.hd, K = g.K, NP = g.NP, Tp = g.Tp, V = g.V;
  const int ld = 3 * D, nj = Tp / 16, CT = (C + 15) / 16, ND = (D + 15) / 16;
  const float *th = p.theta + (size_t)e * g.d;
  float *Wl = lds;                                   // [C][3D]: q | k | v columns
  float *QKV = lds + (WL ? C * 3 * D : 0);           // [Tp][3D]
  float *scr = QKV + Tp * 3 * D;                     // [64][Tp]: e [Tp][C], or 4 x dS [16][Tp]
  float *vec = scr + attn_scr_floats(g);
  int *tok = (int *)vec;                             // [Tp], -1 past T
  float *uw = vec + Tp;                              // [4][Tp] per-wave u
  float *obar = uw + 4 * Tp, *dobar = obar + 64;     // [D]
  float *zv = dobar + 64;                            // [NP + 1][64] layer inputs (zv[0] = pooled)
  float *av = zv + 3 * 64;                           // [NP][64] pre-activations
  float *dv0 = av + 2 * 64, *dv1 = dv0 + 64;         // backward vectors (ping-pong)
  float *lg = dv1 + 64;                              // [16] logits, then their gradient
  const int woff[3] = {g.k_q, g.k_k, g.k_v}, boff[3] = {g.b_q, g.b_k, g.b_v};
  const float scale = 1.0f / sqrtf((float)hd), invT = 1.0f / (float)T;

  if (WL)
    for (int i = tid; i < C * 3 * D; i += ATTN_NT) {
      const int c = i / ld, n = i - c * ld, part = n / D;
      Wl[i] = th[woff[part] + c * D + n - part * D];
    }
  auto wget = [&](int c, int n) -> float {   // [Wq|Wk|Wv][c][n], n < 3D
    if (WL) return Wl[c * ld + n];
    const int part = n / D;
    return th[woff[part] + c * D + n - part * D];
  };

  float *slab = GRAD ? p.slabs + ((size_t)e * p.S + s) * p.dp : nullptr;
  if (GRAD) {   // this workgroup's embedding block is reached by atomics: zero it first
    for (int i = tid; i < V * C; i += ATTN_NT) slab[g.emb + i] = 0.0f;
    __threadfence();
  }

  // gradient accumulators: dW_qkv tiles, dPos tiles (static per wave), tail entries (flat, per thread), qkv bias columns
  f32x4 aw[NDW], ap[NDP];
#pragma unroll
  for (int m = 0; m < NDW; ++m) aw[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int m = 0; m < NDP; ++m) ap[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float gwo[NFW], gwp[ATTN_MAX_NP][NFW], gwc[NFW];
#pragma unroll
  for (int m = 0; m < NFW; ++m) { gwo[m] = 0.0f; gwp[0][m] = 0.0f; gwp[1][m] = 0.0f; gwc[m] = 0.0f; }
  float gbqkv = 0.0f, gbo = 0.0f, gbp[ATTN_MAX_NP] = {0.0f, 0.0f}, gbc = 0.0f, ll_acc = 0.0f;
  const int PL = NP > 0 ? g.P[NP - 1] : C;           // classifier input width

  const int nsplit = GRAD ? p.S : (int)gridDim.x;
  const int rows_per = (p.N + nsplit - 1) / nsplit;
  const int r_begin = min(p.N, s * rows_per), r_end = min(p.N, r_begin + rows_per);

  for (int row = r_begin; row < r_end; ++row) {
    __syncthreads();                                 // previous sequence's readers are done
    attn_stage_tokens(tok, p.X, row, T, Tp, V);
    __syncthreads();
    attn_stage_e(scr, tok, th + g.emb, th + g.pos, T, Tp, C);
    __syncthreads();
    // ---- q | k | v = e W (+ b); q scaled by 1/sqrt(hd)
    for (int f = wave; f < nj * 3 * ND; f += 4) {
      const int mt = f / (3 * ND), rest = f - mt * 3 * ND, part = rest / ND, nt = rest - part * ND;
      const int n = nt * 16 + col, cn = part * D + n;
      f32x4 acc = attn_tile(C, [&](int m, int k) { return scr[(mt * 16 + m) * C + k]; },
                            [&](int k, int m) { return nt * 16 + m < D ? wget(k, part * D + nt * 16 + m) : 0.0f; },
                            f32x4{0.0f, 0.0f, 0.0f, 0.0f});
      if (n < D) {
        const float b = g.bias ? th[boff[part] + n] : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = acc[r] + b;
          QKV[(mt * 16 + 4 * kq + r) * ld + cn] = part == 0 ? v * scale : v;
        }
      }
    }
    __syncthreads();
    // ---- attention forward: column sums of P per head -> obar
    for (int h = wave; h < H; h += 4) attn_fwd_head<NJ>(QKV, ld, tok, T, D, hd, h, nj, invT, obar);
    __syncthreads();
    // ---- tail: pooled = obar Wo (+ bo), projections with gelu, classifier (this kernel's own: vectors at stride 64)
    if (tid < C) {
      float a = g.bias ? th[g.b_o + tid] : 0.0f;
      for (int d = 0; d < D; ++d) a = fmaf(obar[d], th[g.k_o + d * C + tid], a);
      zv[tid] = a;
    }
    __syncthreads();
    int I = C;
    for (int l = 0; l < NP; ++l) {
      const int Pn = g.P[l];
      if (tid < Pn) {
        float a = g.bias ? th[g.b_p[l] + tid] : 0.0f;
        for (int i = 0; i < I; ++i) a = fmaf(zv[l * 64 + i], th[g.k_p[l] + i * Pn + tid], a);
        av[l * 64 + tid] = a;
        zv[(l + 1) * 64 + tid] = attn_gelu(a);
      }
      I = Pn;
      __syncthreads();
    }
    const float *zL = zv + NP * 64;
    if (tid < K) {
      float a = g.bias ? th[g.b_c + tid] : 0.0f;
      for (int i = 0; i < PL; ++i) a = fmaf(zL[i], th[g.k_c + i * K + tid], a);
      lg[tid] = a;
      if constexpr (RAW) p.out[((size_t)e * p.N + row) * K + tid] = a;   // K <= 16 lanes: one contiguous run of the row
    }
    if constexpr (RAW) continue;
    __syncthreads();
    if (tid < 64) {   // wave 0: head (log softmax at the label, its gradient)
      const AttnHead hh = attn_head<GRAD>(lg, K, ((const int32_t *)p.y)[row], GRAD ? nullptr : p.out + (size_t)e * p.N + row);
      if (GRAD && tid == 0) ll_acc += hh.bad ? 0.0f : hh.ll;
    }
    if (!GRAD) continue;
    __syncthreads();
    // ---- backward through the tail (this kernel's own: weight gradients in registers)
#pragma unroll
    for (int m = 0; m < NFW; ++m)
      if (q4 + 4 * m < PL && lane < K) gwc[m] = fmaf(zL[q4 + 4 * m], lg[lane], gwc[m]);
    if (tid < K) gbc += lg[tid];
    float *dcur = dv0, *dnxt = dv1;
    if (tid < PL) {   // d(classifier input); through the gelu when a projection feeds it
      float a = 0.0f;
      for (int k = 0; k < K; ++k) a = fmaf(th[g.k_c + tid * K + k], lg[k], a);
      dcur[tid] = NP > 0 ? a * attn_gelu_grad(av[(NP - 1) * 64 + tid]) : a;
    }
    __syncthreads();
    for (int l = NP - 1; l >= 0; --l) {   // dcur = d(pre-activation of projection l)
      const int Pn = g.P[l], In = l > 0 ? g.P[l - 1] : C;
#pragma unroll
      for (int m = 0; m < NFW; ++m)
        if (q4 + 4 * m < In && lane < Pn) {
          const float v = zv[l * 64 + q4 + 4 * m] * dcur[lane];
          if (l == 0) gwp[0][m] += v; else gwp[1][m] += v;
        }
      if (tid < Pn) gbp[l] += dcur[tid];
      if (tid < In) {
        float a = 0.0f;
        for (int j = 0; j < Pn; ++j) a = fmaf(th[g.k_p[l] + tid * Pn + j], dcur[j], a);
        dnxt[tid] = l > 0 ? a * attn_gelu_grad(av[(l - 1) * 64 + tid]) : a;
      }
      __syncthreads();
      float *t_ = dcur; dcur = dnxt; dnxt = t_;
    }
    // dcur = d(pooled) [C]
#pragma unroll
    for (int m = 0; m < NFW; ++m)
      if (q4 + 4 * m < D && lane < C) gwo[m] = fmaf(obar[q4 + 4 * m], dcur[lane], gwo[m]);
    if (tid < C) gbo += dcur[tid];
    if (tid < D) {
      float a = 0.0f;
      for (int c = 0; c < C; ++c) a = fmaf(th[g.k_o + tid * C + c], dcur[c], a);
      dobar[tid] = a;
    }
    __syncthreads();
    // ---- attention backward, head by head (wave-owned columns of q | k | v)
    for (int h = wave; h < H; h += 4) {
      float *dS = scr + wave * attn_scr_wave(g);
      attn_bwd_head<NJ, NHT>(g, QKV, tok, h, dobar, dS, uw + wave * Tp, dS + 16 * Tp);
    }
    __syncthreads();
    // ---- e again (the scratch held dS), then dW_qkv += e^T d(qkv), de = d(qkv) W^T
    attn_stage_e(scr, tok, th + g.emb, th + g.pos, T, Tp, C);
    if (g.bias && tid < ld) {
      float a = 0.0f;
      for (int t = 0; t < T; ++t) a += QKV[t * ld + tid];
      gbqkv += a;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NDW; ++m) {
      const int f = wave + 4 * m;
      if (f < CT * 3 * ND) {
        const int ct = f / (3 * ND), n0 = (f - ct * 3 * ND) * 16;   // n0: 16-column block of [q | k | v], each part padded to ND blocks
        const int part = n0 / (16 * ND), nb = n0 - part * 16 * ND;
        aw[m] = attn_tile(Tp, [&](int mm, int k) { return ct * 16 + mm < C ? scr[k * C + ct * 16 + mm] : 0.0f; },
                          [&](int k, int n) { return nb + n < D ? QKV[k * ld + part * D + nb + n] : 0.0f; }, aw[m]);
      }
    }
#pragma unroll
    for (int m = 0; m < NDP; ++m) {
      const int f = wave + 4 * m;
      if (f < nj * CT) {
        const int mt = f / CT, ct = f - mt * CT;
        const f32x4 de = attn_tile(ld, [&](int mm, int k) { return QKV[(mt * 16 + mm) * ld + k]; },
                                   [&](int k, int n) { return ct * 16 + n < C ? wget(ct * 16 + n, k) : 0.0f; }, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
        ap[m] += de;
        const int c = ct * 16 + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = mt * 16 + 4 * kq + r;
          if (t < T && c < C) unsafeAtomicAdd(slab + g.emb + (size_t)tok[t] * C + c, de[r]);
        }
      }
    }
  }
  if (!GRAD) return;

  // ---- write the slab row (every entry but the atomically summed embedding block exactly once)
#pragma unroll
  for (int m = 0; m < NDW; ++m) {
    const int f = wave + 4 * m;
    if (f < CT * 3 * ND) {
      const int ct = f / (3 * ND), n0 = (f - ct * 3 * ND) * 16;
      const int part = n0 / (16 * ND), nb = n0 - part * 16 * ND, n = nb + col;
      if (n < D)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + 4 * kq + r;
          if (c < C) slab[woff[part] + c * D + n] = aw[m][r];
        }
    }
  }
#pragma unroll
  for (int m = 0; m < NDP; ++m) {
    const int f = wave + 4 * m;
    if (f < nj * CT) {
      const int mt = f / CT, ct = f - mt * CT, c = ct * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = mt * 16 + 4 * kq + r;
        if (t < T && c < C) slab[g.pos + t * C + c] = ap[m][r];
      }
    }
  }
  if (g.bias && tid < ld) {
    const int part = tid / D;
    slab[boff[part] + tid - part * D] = gbqkv;
  }
#pragma unroll
  for (int m = 0; m < NFW; ++m) {
    const int i = q4 + 4 * m;
    if (i < D && lane < C) slab[g.k_o + i * C + lane] = gwo[m];
    for (int l = 0; l < NP; ++l)
      if (i < (l > 0 ? g.P[l - 1] : C) && lane < g.P[l]) slab[g.k_p[l] + i * g.P[l] + lane] = l == 0 ? gwp[0][m] : gwp[1][m];
    if (i < PL && lane < K) slab[g.k_c + i * K + lane] = gwc[m];
  }
  if (g.bias) {
    if (tid < C) slab[g.b_o + tid] = gbo;
    if (tid < K) slab[g.b_c + tid] = gbc;
    for (int l = 0; l < NP; ++l)
      if (tid < g.P[l]) slab[g.b_p[l] + tid] = gbp[l];
  }
  if (tid < p.dp - g.d) slab[g.d + tid] = 0.0f;
  if (tid == 0) p.llpart[(size_t)e * p.S + s] = ll_acc;
}

template <int NHT, bool WL>
static __global__ __launch_bounds__(ATTN_NT) void k_grad_attn(const AttnParams p) { attn_body<NHT, WL, true>(p); }
template <int NHT, bool WL>
static __global__ __launch_bounds__(ATTN_NT) void k_fwd_attn(const AttnParams p) { attn_body<NHT, WL, false>(p); }
template <int NHT, bool WL>
static __global__ __launch_bounds__(ATTN_NT) void k_out_attn(const AttnParams p) { attn_body<NHT, WL, false, true>(p); }

// the envelope k_grad_attn takes (mile_create refuses everything else; spec.py AttentionSpec mirrors it)
__host__ inline bool attn_supported(const AttnGeom &g) {
  if (g.T < 1 || g.T > ATTN_MAX_T || g.C < 1 || g.C > ATTN_MAX_C || g.D < 1 || g.D > ATTN_MAX_D || g.H < 1 || g.D % g.H ||
      g.K < 1 || g.K > ATTN_MAX_K || g.NP < 0 || g.NP > ATTN_MAX_NP || g.Tp != (g.T + 15) / 16 * 16 || g.V < 1)
    return false;
  for (int l = 0; l < g.NP; ++l)
    if (g.P[l] < 1 || g.P[l] > ATTN_MAX_P) return false;
  return attn_lds_bytes(g, false) <= ATTN_LDS_MAX;
}

// The launch of all three attention translation units.  KS names a kernel family by its members grad<NHT>, fwd<NHT>,
// out<NHT>; the instantiation is picked by ceil(hd / 16) in 1..MAX, the kernel by `run`, and it runs on grid (p.S, E) with
// `lds` bytes of dynamic LDS.
template <auto K>
static hipError_t attn_launch_kernel(const AttnParams &p, int E, size_t lds, hipStream_t st) {
  const hipError_t e = mile_set_max_lds<K>(ATTN_LDS_MAX);
  if (e != hipSuccess) return e;
  K<<<dim3(p.S, E), ATTN_NT, lds, st>>>(p);
  return hipGetLastError();
}
template <class KS, int MAX, int NHT = 1>
static hipError_t attn_launch(const AttnParams &p, int E, MileRun run, size_t lds, hipStream_t st) {
  if constexpr (NHT > MAX) {
    return hipErrorInvalidValue;
  } else {
    if ((p.g.hd + 15) / 16 != NHT) return attn_launch<KS, MAX, NHT + 1>(p, E, run, lds, st);
    return run == MILE_RUN_GRAD  ? attn_launch_kernel<KS::template grad<NHT>>(p, E, lds, st)
           : run == MILE_RUN_RAW ? attn_launch_kernel<KS::template out<NHT>>(p, E, lds, st)
                                 : attn_launch_kernel<KS::template fwd<NHT>>(p, E, lds, st);
  }
}

// MILE_RUN_GRAD: grid (S row ranges, E chains) -> slabs / llpart; _LOGLIK / _RAW: grid (S row blocks, E samples) -> out
hipError_t mile_launch_attn(const AttnParams &p, int E, MileRun run, hipStream_t st);

// PretrainedAttentionClassifier target (src/models/text/attention_classifier.py:74-132), fp32 (MILE_GRAD_ATTN_PRE_F32):
//   x [T] token ids -> e = emb[x] + pos[0..T) (frozen tables loaded from .npy, not parameters) -> MDPA as in mile_attn.h ->
//   mean over all T positions -> (Dense P_i -> gelu) per projection -> gelu -> Dense K 'classifier'
// One fused forward + backward launch per gradient: k_grad_attn_pre, grid (S row ranges, E chains), 256 threads (4 waves), one
// sequence at a time.  The products and the masking are those of k_grad_attn (attn_tile, attn_probs), and so are the blocks of
// mile_attn.h that attnp_body calls: token and e staging, the attention forward and backward of one head, the head.
// What differs:
//   - C <= 192 and D <= 128: Wq|Wk|Wv (up to 288 KB) never fit in LDS next to the sequence, so every weight streams from L2.
//     LDS holds q|k|v [Tp][3D], a scratch that is e [Tp][C] while the projections and dW_qkv run and per-wave dS tiles, u and
//     dK during the attention, and the tail vectors.
//   - The tables are shared by all chains and read-only.  e is gathered from them twice per sequence (it is not kept across
//     the attention), from L2 / the Infinity Cache.
//   - No embedding gradient: no de = d(qkv) W^T product, no atomics.
//   - Gradient accumulators live in the workgroup's own slab row, not in registers.  dW_qkv alone is C 3D floats (36 864 at
//     the stock shape, 57 600 at the larger one: 144 / 225 per lane), and the Wo / projection / classifier gradients add
//     another 18 k / 48 k.  Each entry has one owner thread for the whole launch (dW_qkv: a wave's 16x16 MFMA tile, loaded
//     into the accumulator, advanced by e^T d(qkv) over the sequence's Tp rows, stored back; the rank-1 tail gradients: a
//     strided flat index), so the read-modify-write needs no atomics and no barrier.  That is about 0.7 / 1.1 MB of L2 traffic
//     per sequence and workgroup against 19 / 30 MFLOP of MFMA work.  The first sequence of a range writes instead of adding;
//     an empty range writes zeros.
// k_fwd_attn_pre is the forward half: per-row log-likelihoods for mile_pointwise_loglik.
// The same body with WIDE set is the AttentionClassifier at these widths (mile_attn_wide.h): tables inside theta, their
// gradient, no extra gelu.
#pragma once
#include "mile_attn.h"

#define ATTNP_MAX_C 192
#define ATTNP_MAX_D 128        // hd = D / H <= 128: ceil(hd / 16) <= 8 dq register tiles
#define ATTNP_MAX_P 128

// tail vectors (float offsets): tok [Tp] | obar [D] | dobar [D] | z0 [C] z1 [P0] z2 [P1] (layer inputs) | a0 [P0] a1 [P1]
// (pre-activations) | zf [PL] (after the extra gelu) | dv0, dv1 [W] | lg [16]
struct AttnPreVec { int tok, obar, dobar, z0, z1, z2, a0, a1, zf, dv0, dv1, lg, n; };   // scalars: no array to spill
__host__ __device__ inline AttnPreVec attnp_vec(const AttnGeom &g) {
  const int p0 = g.NP > 0 ? g.P[0] : 0, p1 = g.NP > 1 ? g.P[1] : 0;
  const int W = g.C > p0 ? (g.C > p1 ? g.C : p1) : (p0 > p1 ? p0 : p1);
  AttnPreVec v;
  v.tok = 0;
  v.obar = v.tok + g.Tp;
  v.dobar = v.obar + g.D;
  v.z0 = v.dobar + g.D;
  v.z1 = v.z0 + g.C;
  v.z2 = v.z1 + p0;
  v.a0 = v.z2 + p1;
  v.a1 = v.a0 + p0;
  v.zf = v.a1 + p1;
  v.dv0 = v.zf + (g.NP > 1 ? p1 : (g.NP > 0 ? p0 : g.C));
  v.dv1 = v.dv0 + W;
  v.lg = v.dv1 + W;
  v.n = v.lg + 16;
  return v;
}
// per busy wave: dS [16][Tp] | u [Tp] | (hd > 16) dK [Tp][16 ceil(hd / 16)]
__host__ __device__ inline int attnp_scr_wave(const AttnGeom &g) { return 17 * g.Tp + (g.hd > 16 ? g.Tp * ((g.hd + 15) / 16 * 16) : 0); }
__host__ __device__ inline int attnp_scr_floats(const AttnGeom &g) {
  const int w = g.H < 4 ? g.H : 4, a = g.Tp * g.C, b = w * attnp_scr_wave(g);
  return a > b ? a : b;
}
__host__ __device__ inline size_t attnp_lds_bytes(const AttnGeom &g) {
  return ((size_t)g.Tp * 3 * g.D + attnp_scr_floats(g) + attnp_vec(g).n) * 4;
}

// NHT: ceil(hd / 16) (dq register tiles; dK in registers for NHT == 1, in the wave's scratch otherwise)
// WIDE: the AttentionClassifier of mile_attn_wide.h -- the tables are the chain's own parameters (g.emb / g.pos offsets into
// theta, p.emb / p.pos unused), they get a gradient, and the classifier reads the last projection without the extra gelu
// RAW (evaluation only): the logits go to out[e][row][K] and the head is skipped, y unread (mile_predict)
template <int NHT, bool GRAD, bool WIDE = false, bool RAW = false>
__device__ __forceinline__ void attnp_body(const AttnParams &p) {
  constexpr int NJ = ATTN_MAX_T / 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const AttnGeom &g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, col = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e = blockIdx.y, s = blockIdx.x;
  const int T = g.T, C = g.C, H = g.H, D = g.D, hd = g.hd, K = g.K, NP = g.NP, Tp = g.Tp, V = g.V;
  const int ld = 3 * D, nj = Tp / 16, CT = (C + 15) / 16, ND = (D + 15) / 16;
  const float *th = p.theta + (size_t)e * g.d;
  const float *embt = WIDE ? th + g.emb : p.emb, *post = WIDE ? th + g.pos : p.pos;   // token table [V][C], position rows [T][C]
  float *QKV = lds;                                  // [Tp][3D]: q | k | v columns
  float *scr = QKV + Tp * ld;                        // e [Tp][C], or per wave dS | u | dK
  float *vb = scr + attnp_scr_floats(g);
  const AttnPreVec vo = attnp_vec(g);
  int *tok = (int *)(vb + vo.tok);                   // [Tp], -1 past T
  float *obar = vb + vo.obar, *dobar = vb + vo.dobar, *zf = vb + vo.zf, *lg = vb + vo.lg;
  float *dv0 = vb + vo.dv0, *dv1 = vb + vo.dv1;
  // offsets picked by selects, not by indexing small arrays with run-time indices (which would put the arrays in scratch)
  auto woff = [&](int part) { return part == 0 ? g.k_q : (part == 1 ? g.k_k : g.k_v); };
  auto boff = [&](int part) { return part == 0 ? g.b_q : (part == 1 ? g.b_k : g.b_v); };
  const int p0 = NP > 0 ? g.P[0] : 0, p1 = NP > 1 ? g.P[1] : 0;
  auto Pw = [&](int l) { return l == 0 ? p0 : p1; };
  auto kp = [&](int l) { return l == 0 ? g.k_p[0] : g.k_p[1]; };
  auto bp = [&](int l) { return l == 0 ? g.b_p[0] : g.b_p[1]; };
  const int z0 = vo.z0, a0 = vo.a0;
  auto zv = [&](int l) { return vb + z0 + (l > 0 ? C : 0) + (l > 1 ? p0 : 0); };   // input of layer l (z1 = z0 + C, z2 = z1 + P0)
  auto av = [&](int l) { return vb + a0 + (l > 0 ? p0 : 0); };                     // pre-activation of projection l
  const float scale = 1.0f / sqrtf((float)hd), invT = 1.0f / (float)T;
  const int PL = NP > 0 ? Pw(NP - 1) : C;            // classifier input width
  const float *zL = zv(NP);                          // input of the extra gelu
  const float *zc = WIDE ? zL : zf;                  // classifier input

  float *slab = GRAD ? p.slabs + ((size_t)e * p.S + s) * p.dp : nullptr;
  float ll_acc = 0.0f;
  const int nsplit = GRAD ? p.S : (int)gridDim.x;
  const int rows_per = (p.N + nsplit - 1) / nsplit;
  const int r_begin = min(p.N, s * rows_per), r_end = min(p.N, r_begin + rows_per);

  // slab[off + r nb + c] (+)= a[r] b[c] over [na][nb]: thread-owned flat entries
  auto rank1 = [&](int off, const float *a, int na, const float *b, int nb, bool first) {
    const int dr = ATTN_NT / nb, dc = ATTN_NT - dr * nb;
    int r = tid / nb, c = tid - r * nb;
    for (int i = tid; i < na * nb; i += ATTN_NT) {
      const float v = a[r] * b[c];
      slab[off + i] = first ? v : slab[off + i] + v;
      r += dr; c += dc;
      if (c >= nb) { c -= nb; ++r; }
    }
  };

  if (GRAD && WIDE) {   // the table block of this slab row is reached by atomics: zero it first (16-byte stores between the ends)
    float *blk = slab + g.emb;
    const int n = V * C, head = min(n, (4 - (g.emb & 3)) & 3), nq = (n - head) >> 2;
    for (int i = tid; i < nq; i += ATTN_NT) *(f32x4 *)(blk + head + 4 * i) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (tid < head) blk[tid] = 0.0f;
    if (tid < n - head - 4 * nq) blk[head + 4 * nq + tid] = 0.0f;
    __threadfence();
  }

  for (int row = r_begin; row < r_end; ++row) {
    const bool first = row == r_begin;
    __syncthreads();                                 // previous sequence's readers are done
    attn_stage_tokens(tok, p.X, row, T, Tp, V);
    __syncthreads();
    attn_stage_e(scr, tok, embt, post, T, Tp, C);
    __syncthreads();
    // ---- q | k | v = e W (+ b), W from global; q scaled by 1/sqrt(hd).  A wave owns a 16-column block of [Wq|Wk|Wv] and all
    // nj row tiles: each W operand it loads from L2 feeds nj MFMAs, and the next k step's operand is loaded before this one's
    // MFMAs issue (one wave per SIMD: nothing else hides the L2 latency)
    for (int f = wave; f < 3 * ND; f += 4) {
      const int part = f / ND, nt = f - part * ND, n = nt * 16 + col, cn = part * D + n;
      const float *W = th + woff(part) + n;
      const bool nok = n < D;
      f32x4 acc[NJ];
#pragma unroll
      for (int mt = 0; mt < NJ; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      float bnext = nok && kq < C ? W[kq * D] : 0.0f;
      for (int k0 = 0; k0 < C; k0 += 4) {
        const int k = k0 + kq;
        const float b = bnext;
        bnext = nok && k + 4 < C ? W[(k + 4) * D] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < NJ; ++mt)
          if (mt < nj) acc[mt] = attn_mfma(k < C ? scr[(mt * 16 + col) * C + k] : 0.0f, b, acc[mt]);
      }
      if (nok) {
        const float b = g.bias ? th[boff(part) + n] : 0.0f;
#pragma unroll
        for (int mt = 0; mt < NJ; ++mt)
          if (mt < nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float v = acc[mt][r] + b;
              QKV[(mt * 16 + 4 * kq + r) * ld + cn] = part == 0 ? v * scale : v;
            }
      }
    }
    __syncthreads();
    // ---- attention forward: column sums of P per head -> obar
    if constexpr (WIDE) {   // attn_fwd_head's text in place: called as a function, k_grad_attn_wide was 1.2 % slower (profiles/r08)
    for (int h = wave; h < H; h += 4) {
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
    } else {
    for (int h = wave; h < H; h += 4) attn_fwd_head<NJ>(QKV, ld, tok, T, D, hd, h, nj, invT, obar);
    }
    __syncthreads();
    // ---- tail: pooled = obar Wo (+ bo), projections with gelu, the extra gelu, classifier (this kernel's own: packed vectors)
    if (tid < C) {
      float a = g.bias ? th[g.b_o + tid] : 0.0f;
      #pragma unroll 8
      for (int d = 0; d < D; ++d) a = fmaf(obar[d], th[g.k_o + d * C + tid], a);
      zv(0)[tid] = a;
    }
    __syncthreads();
    for (int l = 0; l < NP; ++l) {
      const int Pn = Pw(l), In = l > 0 ? Pw(l - 1) : C;
      const float *zi = zv(l);
      if (tid < Pn) {
        float a = g.bias ? th[bp(l) + tid] : 0.0f;
        #pragma unroll 8
        for (int i = 0; i < In; ++i) a = fmaf(zi[i], th[kp(l) + i * Pn + tid], a);
        av(l)[tid] = a;
        zv(l + 1)[tid] = attn_gelu(a);
      }
      __syncthreads();
    }
    if (!WIDE) {
      if (tid < PL) zf[tid] = attn_gelu(zL[tid]);
      __syncthreads();
    }
    if (tid < K) {
      float a = g.bias ? th[g.b_c + tid] : 0.0f;
      #pragma unroll 8
      for (int i = 0; i < PL; ++i) a = fmaf(zc[i], th[g.k_c + i * K + tid], a);
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
    // ---- backward through the tail (this kernel's own); rank-1 weight gradients into the slab row
    rank1(g.k_c, zc, PL, lg, K, first);
    if (g.bias && tid < K) slab[g.b_c + tid] = first ? lg[tid] : slab[g.b_c + tid] + lg[tid];
    float *dcur = dv0, *dnxt = dv1;
    if (tid < PL) {   // d(classifier input) -> through the extra gelu -> through the last projection's gelu
      float a = 0.0f;
      for (int k = 0; k < K; ++k) a = fmaf(th[g.k_c + tid * K + k], lg[k], a);
      if (!WIDE) a *= attn_gelu_grad(zL[tid]);
      dcur[tid] = NP > 0 ? a * attn_gelu_grad(av(NP - 1)[tid]) : a;
    }
    __syncthreads();
    for (int l = NP - 1; l >= 0; --l) {   // dcur = d(pre-activation of projection l)
      const int Pn = Pw(l), In = l > 0 ? Pw(l - 1) : C;
      rank1(kp(l), zv(l), In, dcur, Pn, first);
      if (g.bias && tid < Pn) slab[bp(l) + tid] = first ? dcur[tid] : slab[bp(l) + tid] + dcur[tid];
      if (tid < In) {
        float a = 0.0f;
        #pragma unroll 8
        for (int j = 0; j < Pn; ++j) a = fmaf(th[kp(l) + tid * Pn + j], dcur[j], a);
        dnxt[tid] = l > 0 ? a * attn_gelu_grad(av(l - 1)[tid]) : a;
      }
      __syncthreads();
      float *t_ = dcur; dcur = dnxt; dnxt = t_;
    }
    // dcur = d(pooled) [C]
    rank1(g.k_o, obar, D, dcur, C, first);
    if (g.bias && tid < C) slab[g.b_o + tid] = first ? dcur[tid] : slab[g.b_o + tid] + dcur[tid];
    if (tid < D) {
      float a = 0.0f;
      #pragma unroll 8
      for (int c = 0; c < C; ++c) a = fmaf(th[g.k_o + tid * C + c], dcur[c], a);
      dobar[tid] = a;
    }
    __syncthreads();
    // ---- attention backward, head by head (wave-owned columns of q | k | v)
    for (int h = wave; h < H; h += 4) {
      float *dS = scr + wave * attnp_scr_wave(g), *u = dS + 16 * Tp;
      attn_bwd_head<NJ, NHT>(g, QKV, tok, h, dobar, dS, u, u + Tp);
    }
    __syncthreads();
    // ---- e again (the scratch held dS), then dW_qkv (+)= e^T d(qkv) into the slab, one 16x16 tile per wave at a time
    attn_stage_e(scr, tok, embt, post, T, Tp, C);
    if (g.bias)
      for (int n = tid; n < ld; n += ATTN_NT) {
        float a = 0.0f;
        for (int t = 0; t < T; ++t) a += QKV[t * ld + n];
        const int part = n / D, o = boff(part) + n - part * D;
        slab[o] = first ? a : slab[o] + a;
      }
    __syncthreads();
    for (int f = wave; f < CT * 3 * ND; f += 4) {
      const int ct = f / (3 * ND), rest = f - ct * 3 * ND, part = rest / ND, nb = (rest - part * ND) * 16, n = nb + col;
      float *dst = slab + woff(part) + n;
      f32x4 a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      if (!first && n < D)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + 4 * kq + r;
          if (c < C) a[r] = dst[c * D];
        }
      a = attn_tile(Tp, [&](int mm, int k) { return ct * 16 + mm < C ? scr[k * C + ct * 16 + mm] : 0.0f; },
                    [&](int k, int nn) { return nb + nn < D ? QKV[k * ld + part * D + nb + nn] : 0.0f; }, a);
      if (n < D)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + 4 * kq + r;
          if (c < C) dst[c * D] = a[r];
        }
    }
    // ---- (WIDE) de = d(qkv) [Wq|Wk|Wv]^T, [Tp][3D] x [3D][C]: a wave owns a 16-column block of C and all nj row tiles, each W operand
    // it loads from L2 feeds nj MFMAs (the form of the q | k | v product).  The tiles leave the accumulators directly:
    // dPos[t] (+)= de[t] is owned by the tile's thread for the whole launch; dEmb[x_t] += de[t] is a scatter (a token may repeat
    // inside a sequence) by fp32 vector atomics into this workgroup's own table block
    for (int ct = wave; WIDE && ct < CT; ct += 4) {
      const int c = ct * 16 + col;
      const bool cok = c < C;
      const float *Wc = th + c * D;
      f32x4 acc[NJ];
#pragma unroll
      for (int mt = 0; mt < NJ; ++mt) acc[mt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
      for (int part = 0; part < 3; ++part) {
        const float *W = Wc + woff(part);
        const float *A = QKV + part * D;
        float bnext = cok && kq < D ? W[kq] : 0.0f;
        for (int k0 = 0; k0 < D; k0 += 4) {
          const int k = k0 + kq;
          const float b = bnext;
          bnext = cok && k + 4 < D ? W[k + 4] : 0.0f;
#pragma unroll
          for (int mt = 0; mt < NJ; ++mt)
            if (mt < nj) acc[mt] = attn_mfma(k < D ? A[(mt * 16 + col) * ld + k] : 0.0f, b, acc[mt]);
        }
      }
      if (cok)
#pragma unroll
        for (int mt = 0; mt < NJ; ++mt)
          if (mt < nj)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int t = mt * 16 + 4 * kq + r;
              if (t < T) {
                float *dp_ = slab + g.pos + t * C + c;
                *dp_ = first ? acc[mt][r] : *dp_ + acc[mt][r];
                unsafeAtomicAdd(slab + g.emb + (size_t)tok[t] * C + c, acc[mt][r]);
              }
            }
    }
  }
  if (!GRAD) return;
  if (r_begin >= r_end) {   // no sequence in this range: its slab row is zero (WIDE: the table block already is)
    const int lo = WIDE ? g.emb : g.d, hi = WIDE ? g.emb + V * C : g.d;
    for (int i = tid; i < lo; i += ATTN_NT) slab[i] = 0.0f;
    for (int i = hi + tid; i < g.d; i += ATTN_NT) slab[i] = 0.0f;
  }
  if (tid < p.dp - g.d) slab[g.d + tid] = 0.0f;
  if (tid == 0) p.llpart[(size_t)e * p.S + s] = ll_acc;
}

template <int NHT>
static __global__ __launch_bounds__(ATTN_NT) void k_grad_attn_pre(const AttnParams p) { attnp_body<NHT, true>(p); }
template <int NHT>
static __global__ __launch_bounds__(ATTN_NT) void k_fwd_attn_pre(const AttnParams p) { attnp_body<NHT, false>(p); }
template <int NHT>
static __global__ __launch_bounds__(ATTN_NT) void k_out_attn_pre(const AttnParams p) { attnp_body<NHT, false, false, true>(p); }

// the envelope k_grad_attn_pre takes (mile_create refuses everything else; spec.py PretrainedAttentionSpec mirrors it)
__host__ inline bool attnp_supported(const AttnGeom &g) {
  if (g.T < 1 || g.T > ATTN_MAX_T || g.C < 1 || g.C > ATTNP_MAX_C || g.D < 1 || g.D > ATTNP_MAX_D || g.H < 1 || g.D % g.H ||
      g.K < 1 || g.K > ATTN_MAX_K || g.NP < 0 || g.NP > ATTN_MAX_NP || g.Tp != (g.T + 15) / 16 * 16 || g.V < 1)
    return false;
  for (int l = 0; l < g.NP; ++l)
    if (g.P[l] < 1 || g.P[l] > ATTNP_MAX_P) return false;
  return attnp_lds_bytes(g) <= ATTN_LDS_MAX;
}

// MILE_RUN_GRAD: grid (S row ranges, E chains) -> slabs / llpart; _LOGLIK / _RAW: grid (S row blocks, E samples) -> out
hipError_t mile_launch_attn_pre(const AttnParams &p, int E, MileRun run, hipStream_t st);

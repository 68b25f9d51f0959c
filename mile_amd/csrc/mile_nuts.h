// mile_nuts.h -- lockstep ensemble NUTS (blackjax 1.2.2 nuts.build_kernel with velocity_verlet and a diagonal metric) and its
// window adaptation (adaptation.window_adaptation.base), restated on the device.  Included from mile_hip.hip after
// mile_update.h.
//
// Lockstep: every chain that is still building its tree takes ONE leapfrog step per round, and a round is one grad launch
// over the ensemble followed by k_nuts_leaf.  Doubling j adds a subtree of exactly 2^j leaves and a chain only leaves a
// subtree early by ending its whole NUTS step, so every chain that is still active sits at the same (doubling j, leaf k):
// the host knows the schedule, the iterative U-turn checkpoint slots depend on k only (uniform across the ensemble), and
// the one device -> host read per doubling is "how many chains go on".
//
// One workgroup per chain; every per-chain reduction over d (kinetic energy, log prior, <= max_num_doublings pairs of
// U-turn dot products) is one block reduction.  Per-chain scalars live in NutsChain [E] (device memory); the d-sized
// trajectory buffers in NutsBufs.  Uniform draws of one NUTS step and chain, by slot (also the layout of explicit draws):
//   [0, M)            direction bit of doubling j (forward when u < 0.5)
//   [M, 2M)           progressive_biased_sampling of doubling j
//   [2M, 2M + 2^M - 1) progressive_uniform_sampling of the leaf with that index in the step (leaf 0 of a subtree draws none)
#pragma once
#include "mile_device.h"

#define NUTS_NT 256
#define NUTS_NW (NUTS_NT / 64)
#define NUTS_MAX_DOUBLINGS 12
#define NUTS_STAGE_MOMENTUM 3u    // Philox stage ids (MCLMC uses 0-2)
#define NUTS_STAGE_UNIFORM 4u
#define NUTS_INFO 6               // num_integration_steps, acceptance_rate, num_trajectory_expansions, is_divergent, energy, is_turning

struct NutsChain {
  float eps;            // step size of this NUTS step
  float e0;             // initial energy (-logp + kinetic energy of the drawn momentum)
  float p_w, p_slpa;    // trajectory proposal: log weight, log sum of acceptance probabilities (Proposal.weight / sum_log_p_accept)
  float p_energy;
  float s_w, s_slpa;    // subtree proposal
  float s_energy, s_logp;
  float acc_rate;       // info of the finished step (read by the adaptation)
  int32_t dir;          // +1 / -1 direction of the current subtree
  int32_t active;       // still expanding the trajectory
  int32_t sub_active;   // still integrating the current subtree
  int32_t depth;        // doublings completed
  int32_t n_states;     // leaves of the trajectory before the current subtree
  int32_t s_n, s_div, s_turn;
  int32_t is_div, is_turn;
};

struct NutsBufs {
  float *T;             // [E, d] position of the next leaf (theta of the next grad launch)
  float *Ph;            // [E, d] momentum of the next leaf after its first half kick
  float *xe[2], *pe[2], *ge[2];   // [E, d] trajectory ends (0 = leftmost, 1 = rightmost): position, momentum, gradient
  float *psT, *psS;     // [E, d] momentum sums of the trajectory and of the current subtree
  float *xs, *gs;       // [E, d] subtree proposal position and gradient
  float *ck_r, *ck_rs;  // [E, M, d] iterative U-turn checkpoints: momenta and momentum sums
  NutsChain *chain;     // [E]
  int32_t *count;       // [1] chains that go on after a doubling
};

struct NutsParams {
  int d, dp, S, E, M, prior;
  float loc, scale, thr;
  const float *slabs, *llpart;
  float *x, *g, *logp;          // the chain state == the trajectory proposal
  const float *eps;             // [E]
  const float *m;               // [E, d] diagonal inverse mass matrix
  const float *z;               // [E, d] explicit momentum normals of this step, or NULL
  const float *unif;            // [E, NU] explicit uniforms of this step, or NULL
  int NU;
  uint64_t seed;
  const int32_t *pids;
  uint32_t gstep;
  int leaf, sub_len;            // k_nuts_leaf: leaf index k in the subtree, 2^j
  float *out_info;              // [E, 6] row of this step or NULL
  float *out_sample;            // [E, d] kept position of this step or NULL
  NutsBufs b;
};

__device__ __forceinline__ float nuts_uniform(const NutsParams &p, int e, uint32_t pid, int slot) {
  if (p.unif) return p.unif[(size_t)e * p.NU + slot];
  uint32_t w[4];
  philox4x32_10((uint32_t)slot, pid, p.gstep, NUTS_STAGE_UNIFORM, (uint32_t)p.seed, (uint32_t)(p.seed >> 32), w);
  return ((float)(w[0] >> 8) + 0.5f) * (1.0f / 16777216.0f);   // (0, 1)
}

// jnp.logaddexp, with logaddexp(-inf, -inf) = -inf
__device__ __forceinline__ float nuts_logaddexp(float a, float b) {
  const float mx = fmaxf(a, b);
  if (mx == -INFINITY) return -INFINITY;
  return mx + log1pf(expf(-fabsf(a - b)));
}

// sum of NR values over the workgroup, result in every thread
template <int NR>
__device__ __forceinline__ void nuts_block_sum(float (&v)[NR], float (*red)[NR]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < NR; ++r) v[r] = wave_sum(v[r]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int r = 0; r < NR; ++r) red[tid >> 6][r] = v[r];
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    float t = 0.0f;
    for (int w = 0; w < NUTS_NW; ++w) t += red[w][r];
    v[r] = t;
  }
  __syncthreads();
}

// First half kick and drift of the leapfrog that starts at trajectory end `side` (integrators.velocity_verlet,
// coefficients (1/2, 1, 1/2), signed step h): Ph = p + h/2 g, T = x + h m Ph.
__device__ __forceinline__ void nuts_start_leaf(const NutsParams &p, size_t base, int tid, int side, float h) {
  for (int i = tid; i < p.d; i += NUTS_NT) {
    const float ph = p.b.pe[side][base + i] + 0.5f * h * p.b.ge[side][base + i];
    p.b.Ph[base + i] = ph;
    p.b.T[base + i] = p.b.xe[side][base + i] + h * p.m[base + i] * ph;
  }
}

// Step start (nuts.build_kernel): momentum p = z / sqrt(m) (metrics.default_metric sample_momentum), initial energy,
// both trajectory ends = the state, p_sum = p, proposal = the state (weight 0, sum_log_p_accept -inf); then the direction
// of doubling 0 and the first half kick + drift.
static __global__ __launch_bounds__(NUTS_NT) void k_nuts_begin(const NutsParams p) {
  __shared__ float red[NUTS_NW][1];
  __shared__ NutsChain c;
  const int tid = threadIdx.x, e = blockIdx.x, d = p.d;
  const size_t base = (size_t)e * d;
  const uint32_t pid = p.pids ? (uint32_t)p.pids[e] : (uint32_t)e;
  float kin[1] = {0.0f};
  const int nq = (d + 3) >> 2;
  for (int q = tid; q < nq; q += NUTS_NT) {
    f32x4 zz = {0, 0, 0, 0};
    if (!p.z) zz = philox_normal4(q, pid, p.gstep, NUTS_STAGE_MOMENTUM, p.seed);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = 4 * q + r;
      if (i < d) {
        const float zi = p.z ? p.z[base + i] : zz[r], mi = p.m[base + i];
        const float pi = zi / sqrtf(mi);
        const float xi = p.x[base + i], gi = p.g[base + i];
        kin[0] += mi * pi * pi;
        p.b.xe[0][base + i] = xi; p.b.xe[1][base + i] = xi;
        p.b.ge[0][base + i] = gi; p.b.ge[1][base + i] = gi;
        p.b.pe[0][base + i] = pi; p.b.pe[1][base + i] = pi;
        p.b.psT[base + i] = pi;
      }
    }
  }
  nuts_block_sum<1>(kin, red);
  if (tid == 0) {
    NutsChain t{};
    t.eps = p.eps[e];
    t.e0 = -p.logp[e] + 0.5f * kin[0];
    t.p_w = 0.0f; t.p_slpa = -INFINITY; t.p_energy = t.e0;
    t.dir = nuts_uniform(p, e, pid, 0) < 0.5f ? 1 : -1;   // dynamic_multiplicative_expansion: bernoulli(0.5) -> +1
    t.active = 1; t.sub_active = 1;
    c = t;
    p.b.chain[e] = t;
  }
  __syncthreads();
  nuts_start_leaf(p, base, tid, c.dir > 0 ? 1 : 0, (float)c.dir * c.eps);
}

// One leaf of the current subtree (trajectory.dynamic_progressive_integration, one iteration of add_one_state): the
// gradient at T from the grad kernel's slabs, the second half kick, the leaf's proposal (proposal.proposal_generator),
// the divergence test, progressive_uniform_sampling into the subtree proposal, the subtree momentum sum and the
// iterative U-turn checkpoints (termination.iterative_uturn_numpyro); then, if the subtree goes on, the first half kick
// and drift of the next leaf.
static __global__ __launch_bounds__(NUTS_NT) void k_nuts_leaf(const NutsParams p) {
  constexpr int NR = 2 + 2 * NUTS_MAX_DOUBLINGS;
  __shared__ float red[NUTS_NW][NR];
  __shared__ NutsChain c;
  __shared__ int go[2];
  const int tid = threadIdx.x, e = blockIdx.x, d = p.d;
  if (tid == 0) c = p.b.chain[e];
  __syncthreads();
  if (!c.sub_active) return;
  const size_t base = (size_t)e * d, ckbase = (size_t)e * p.M * d;
  const int k = p.leaf, side = c.dir > 0 ? 1 : 0;
  const float h = (float)c.dir * c.eps;
  // _leaf_idx_to_ckpt_idxs(k): idx_max = popcount(k >> 1), checks idx_max down to idx_max - (trailing ones of k) + 1
  const int idx_max = __popc((unsigned)k >> 1);
  const int nchk = __builtin_ctz(~(unsigned)k);     // trailing ones (0 for even k)
  const bool store_ck = (k & 1) == 0;
  const float *sl = p.slabs + (size_t)e * p.S * p.dp;
  float v[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) v[r] = 0.0f;   // v[0] = m p^2, v[1] = log prior, v[2 + 2c], v[3 + 2c] = U-turn dots of check c
  for (int i = tid; i < d; i += NUTS_NT) {
    const float xi = p.b.T[base + i];
    const float gi = slab_grad_logprior(sl, p.S, p.dp, i, p.prior, p.loc, p.scale, xi, v[1]);
    const float mi = p.m[base + i];
    const float pi = p.b.Ph[base + i] + 0.5f * h * gi;
    p.b.xe[side][base + i] = xi; p.b.pe[side][base + i] = pi; p.b.ge[side][base + i] = gi;
    v[0] += mi * pi * pi;
    const float ps = (k == 0 ? 0.0f : p.b.psS[base + i]) + pi;   // append_to_trajectory: momentum_sum + momentum
    p.b.psS[base + i] = ps;
    if (store_ck) {   // update_criterion_state: even leaves store (r, r_sum) at idx_max
      p.b.ck_r[ckbase + (size_t)idx_max * d + i] = pi;
      p.b.ck_rs[ckbase + (size_t)idx_max * d + i] = ps;
    }
#pragma unroll
    for (int q = 0; q < NUTS_MAX_DOUBLINGS; ++q) {
      if (q < nchk) {   // _is_iterative_turning: is_turning(r_ckpts[i], r, r_sum - r_sum_ckpts[i] + r_ckpts[i])
        const size_t o = ckbase + (size_t)(idx_max - q) * d + i;
        const float r0 = p.b.ck_r[o];
        const float rho = ps - p.b.ck_rs[o] + r0 - 0.5f * (r0 + pi);   // metrics: rho = m_sum - (m_right + m_left) / 2
        v[2 + 2 * q] += mi * r0 * rho;
        v[3 + 2 * q] += mi * pi * rho;
      }
    }
  }
  nuts_block_sum<NR>(v, red);
  if (tid == 0) {
    const uint32_t pid = p.pids ? (uint32_t)p.pids[e] : (uint32_t)e;
    const float logp = (float)llpart_logprior(p.llpart, p.S, e, d, p.prior, p.scale, (double)v[1]);
    const float energy = -logp + 0.5f * v[0];
    float w = c.e0 - energy;                           // proposal_generator: delta_energy, NaN -> -inf
    if (isnan(w)) w = -INFINITY;
    const bool div = -w > p.thr;                       // is_diverging = -weight > divergence_threshold
    bool turn = false;
    for (int q = 0; q < nchk; ++q) turn = turn || v[2 + 2 * q] <= 0.0f || v[3 + 2 * q] <= 0.0f;
    bool accept;
    if (k == 0) {                                      // the first leaf always becomes the subtree proposal
      accept = true;
      c.s_w = w; c.s_slpa = fminf(w, 0.0f);
    } else {                                           // progressive_uniform_sampling: p = expit(w_new - w)
      const float pa = 1.0f / (1.0f + expf(-(w - c.s_w)));
      accept = nuts_uniform(p, e, pid, 2 * p.M + c.n_states + k) < pa;
      c.s_w = nuts_logaddexp(c.s_w, w);
      c.s_slpa = nuts_logaddexp(c.s_slpa, fminf(w, 0.0f));
    }
    if (accept) { c.s_energy = energy; c.s_logp = logp; }
    c.s_n = k + 1; c.s_div = div; c.s_turn = turn;
    const bool cont = !div && !turn && k + 1 < p.sub_len;
    c.sub_active = cont;
    p.b.chain[e] = c;
    go[0] = accept; go[1] = cont;
  }
  __syncthreads();
  const bool accept = go[0], cont = go[1];
  if (!accept && !cont) return;
  for (int i = tid; i < d; i += NUTS_NT) {   // this thread wrote these elements of the end above
    const float xi = p.b.xe[side][base + i], gi = p.b.ge[side][base + i];
    if (accept) { p.b.xs[base + i] = xi; p.b.gs[base + i] = gi; }
    if (cont) {
      const float ph = p.b.pe[side][base + i] + 0.5f * h * gi;
      p.b.Ph[base + i] = ph;
      p.b.T[base + i] = xi + h * p.m[base + i] * ph;
    }
  }
}

// End of doubling j (trajectory.dynamic_multiplicative_expansion, expand_once after the subtree): progressive_biased_sampling
// of the subtree proposal into the trajectory proposal (skipped for a diverging or turning subtree; sum_log_p_accept is
// accumulated either way), merge_trajectories, the U-turn check of the whole trajectory, and either the step end (state,
// info row, thinned sample) or the direction of doubling j + 1 and its first leapfrog half.
static __global__ __launch_bounds__(NUTS_NT) void k_nuts_merge(const NutsParams p) {
  __shared__ float red[NUTS_NW][2];
  __shared__ NutsChain c;
  __shared__ int take_s;
  const int tid = threadIdx.x, e = blockIdx.x, d = p.d;
  if (tid == 0) c = p.b.chain[e];
  __syncthreads();
  if (!c.active) return;
  const size_t base = (size_t)e * d;
  const uint32_t pid = p.pids ? (uint32_t)p.pids[e] : (uint32_t)e;
  if (tid == 0) {
    bool take = false;
    if (!(c.s_div || c.s_turn)) {
      const float r = expf(c.s_w - c.p_w);
      const float pa = r > 1.0f ? 1.0f : r;            // clip(exp(dw), max=1), NaN stays NaN (never accepts)
      take = nuts_uniform(p, e, pid, p.M + c.depth) < pa;
      c.p_w = nuts_logaddexp(c.p_w, c.s_w);
    }
    c.p_slpa = nuts_logaddexp(c.p_slpa, c.s_slpa);
    if (take) { c.p_energy = c.s_energy; p.logp[e] = c.s_logp; }
    take_s = take;
  }
  __syncthreads();
  const bool take = take_s;
  float v[2] = {0.0f, 0.0f};
  for (int i = tid; i < d; i += NUTS_NT) {
    if (take) { p.x[base + i] = p.b.xs[base + i]; p.g[base + i] = p.b.gs[base + i]; }
    const float ps = p.b.psT[base + i] + p.b.psS[base + i];
    p.b.psT[base + i] = ps;
    const float pl = p.b.pe[0][base + i], pr = p.b.pe[1][base + i], mi = p.m[base + i];
    const float rho = ps - 0.5f * (pr + pl);
    v[0] += mi * pl * rho;
    v[1] += mi * pr * rho;
  }
  nuts_block_sum<2>(v, red);
  if (tid == 0) {
    const bool full_turn = v[0] <= 0.0f || v[1] <= 0.0f;
    c.n_states += c.s_n;
    c.depth += 1;
    c.is_div = c.s_div;
    c.is_turn = c.s_turn || full_turn;
    const bool cont = !c.s_div && !c.is_turn && c.depth < p.M;
    if (!cont) {
      c.active = 0; c.sub_active = 0;
      c.acc_rate = expf(c.p_slpa) / (float)c.n_states;
      if (p.out_info) {
        float *o = p.out_info + (size_t)e * NUTS_INFO;
        o[0] = (float)c.n_states; o[1] = c.acc_rate; o[2] = (float)c.depth;
        o[3] = (float)c.is_div; o[4] = c.p_energy; o[5] = (float)c.is_turn;
      }
    } else {
      c.dir = nuts_uniform(p, e, pid, c.depth) < 0.5f ? 1 : -1;
      c.sub_active = 1;
      atomicAdd(p.b.count, 1);
    }
    p.b.chain[e] = c;
  }
  __syncthreads();
  if (c.active) {
    nuts_start_leaf(p, base, tid, c.dir > 0 ? 1 : 0, (float)c.dir * c.eps);
  } else if (p.out_sample) {
    for (int i = tid; i < d; i += NUTS_NT) p.out_sample[base + i] = p.x[base + i];
  }
}

// Window adaptation, one step (adaptation.window_adaptation.base: update + slow_final), per chain after the NUTS step:
// dual averaging of log(step size) on target - acceptance_rate (optimizers.dual_averaging, t0 = 10, gamma = 0.05,
// kappa = 0.75); in slow windows a Welford update of the position; at a slow window's end the regularised diagonal
// inverse mass matrix (mass_matrix_adaptation final), a Welford reset and a dual-averaging restart from
// exp(log_step_size_avg) (da_init(da_final(state))).
struct NutsAdaptParams {
  int d;
  int stage, window_end;
  float target;
  const float *x;          // [E, d] positions after the step
  const NutsChain *chain;  // acceptance rate of the step
  float *step_size;        // [E]
  float *imm;              // [E, d]
  float *da;               // [E, 5] log_step_size, log_step_size_avg, step, avg_error, mu
  float *wf;               // [E, 2, d] Welford mean, m2
  float *wf_n;             // [E]
};

static __global__ __launch_bounds__(NUTS_NT) void k_nuts_adapt(const NutsAdaptParams p) {
  const int tid = threadIdx.x, e = blockIdx.x, d = p.d;
  const size_t base = (size_t)e * d;
  const float n_old = p.wf_n[e];
  if (p.stage == 1) {
    const float n = n_old + 1.0f;
    float *mean = p.wf + 2 * base, *m2 = p.wf + 2 * base + d;
    for (int i = tid; i < d; i += NUTS_NT) {   // welford_algorithm update (diagonal)
      const float xi = p.x[base + i];
      const float delta = xi - mean[i];
      const float mu = mean[i] + delta / n;
      mean[i] = mu;
      m2[i] += delta * (xi - mu);
    }
    if (p.window_end) {
      __syncthreads();
      for (int i = tid; i < d; i += NUTS_NT) {   // mass_matrix_adaptation final: n/(n+5) var + 1e-3 * 5/(n+5); Welford reset
        const float var = m2[i] / (n - 1.0f);
        p.imm[base + i] = (n / (n + 5.0f)) * var + 1e-3f * (5.0f / (n + 5.0f));
        mean[i] = 0.0f; m2[i] = 0.0f;
      }
    }
  }
  if (tid == 0) {
    float *da = p.da + (size_t)e * 5;
    const float acc = p.chain[e].acc_rate;
    // dual_averaging update with gradient = target - acceptance_rate
    const float t = da[2], reg = t + 10.0f, eta = powf(t, -0.75f);
    const float avg = (1.0f - 1.0f / reg) * da[3] + (p.target - acc) / reg;
    const float lx = da[4] - (sqrtf(t) / 0.05f) * avg;
    da[0] = lx; da[1] = eta * lx + (1.0f - eta) * da[1]; da[2] = t + 1.0f; da[3] = avg;
    float ss = expf(lx);
    if (p.stage == 1) p.wf_n[e] = n_old + 1.0f;
    if (p.stage == 1 && p.window_end) {
      p.wf_n[e] = 0.0f;
      ss = expf(da[1]);                                   // da_init(da_final(ss_state))
      da[0] = logf(ss); da[1] = 0.0f; da[2] = 1.0f; da[3] = 0.0f; da[4] = logf(10.0f * ss);
    }
    p.step_size[e] = ss;
  }
}

// AttentionClassifier at the widths the on-chip k_grad_attn cannot hold (C <= 192, D <= 128, projections <= 128), fp32
// (MILE_GRAD_ATTN_WIDE_F32).  The model is mile_attn.h's: token and position tables are parameters of every chain, no extra
// gelu.  The kernel is mile_attn_pre.h's body with WIDE set: weights streamed from L2, accumulators in the workgroup's own slab
// row, and on top of it
//   - e gathered from the chain's own tables inside theta (AttnGeom emb / pos offsets);
//   - de = d(qkv) [Wq|Wk|Wv]^T straight from the accumulators: dPos[t] (+)= de[t] by the tile's owner thread, dEmb[x_t] += de[t]
//     by fp32 vector atomics into the slab row's own [V][C] block, which the workgroup zero-fills when it starts.
// That block is 4 V C bytes per slab row (7.68 MB at V = 10 000, C = 192): see attn_wide_S in mile_hip.hip for what it means
// for the number of row ranges.  LDS is the pretrained kernel's (attnp_lds_bytes); no [Tp][C] image of de is kept.
#pragma once
#include "mile_attn_pre.h"

template <int NHT>
static __global__ __launch_bounds__(ATTN_NT) void k_grad_attn_wide(const AttnParams p) { attnp_body<NHT, true, true>(p); }
template <int NHT>
static __global__ __launch_bounds__(ATTN_NT) void k_fwd_attn_wide(const AttnParams p) { attnp_body<NHT, false, true>(p); }
template <int NHT>
static __global__ __launch_bounds__(ATTN_NT) void k_out_attn_wide(const AttnParams p) { attnp_body<NHT, false, true, true>(p); }

// the envelope k_grad_attn_wide takes (mile_create refuses everything else; spec.py WideAttentionSpec mirrors it)
__host__ inline bool attn_wide_supported(const AttnGeom &g) { return attnp_supported(g) && g.emb >= 0 && g.pos >= 0; }

// MILE_RUN_GRAD: grid (S row ranges, E chains) -> slabs / llpart; _LOGLIK / _RAW: grid (S row blocks, E samples) -> out
hipError_t mile_launch_attn_wide(const AttnParams &p, int E, MileRun run, hipStream_t st);

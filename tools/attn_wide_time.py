"""AttentionClassifier at emb_size 192 (k_grad_attn_wide): the grad kernel by HIP events, one MCLMC step and one 256-row
warm-start step by wall clock, the FLOP model and its fraction of the fp32 peak, the gradient slabs' size, and a torch fp32
yardstick (the same model through autograd, chains batched as a leading axis, rows in chunks) on the same GPU.

    python tools/attn_wide_time.py [--shape stock larger] [--E 1 8] [--N 35000] [--reps 5]

The shapes of experiments/mclmc_seqmod_pretraining_synthetic.yaml (stock: V = 10 000, T = 70, C = 192, 8 heads, qkv_dim 64,
projection [32]; d = 1 989 218) and ..._larger_synthetic.yaml (10 heads, qkv_dim 100, projections [128, 32]; d = 2 039 630);
2 classes, bias, Normal prior, synthetic token rows.  One JSON line per shape and ensemble size.
FLOP model per sequence and chain: WideAttentionSpec.flops_per_sequence (3 x forward; stock 24.44 MFLOP: 0.855 TFLOP and 5.4 ms
of fp32 peak per gradient of one chain on N = 35 000 rows).
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from mile_amd.dataset import synthetic_text
from mile_amd.engine import Engine
from mile_amd.spec import WideAttentionSpec

PEAK_FP32_TFLOPS = 157.3     # MI355X fp32 (vector and f32 MFMA)
SHAPES = {'stock': dict(n_heads=8, qkv_dim=64, projection_dim=(32,), prior_scale=0.2),
          'larger': dict(n_heads=10, qkv_dim=100, projection_dim=(128, 32), prior_scale=0.4)}


def torch_yardstick(spec, x, y, theta, reps, chunk=8192):
    """Gradient of the summed log-likelihood + Normal prior for all chains at once, fp32, eager torch autograd on the GPU.
    `chunk` counts sequence-chains per backward pass, so that one chain is batched as deeply as eight (1024 rows at E = 8)."""
    leaves = spec.leaves()
    E, T = theta.shape[0], spec.context_len
    chunk = max(1, chunk // E)
    H, D = spec.n_heads, spec.qkv_dim
    hd = D // H
    neg = torch.finfo(torch.float32).min
    gelu = lambda a: torch.nn.functional.gelu(a, approximate='tanh')   # noqa: E731

    def loglik(th, xb, yb):
        P = {n: th[:, o:o + int(np.prod(sh))].reshape((E,) + tuple(sh)) for n, o, sh in leaves}
        e = P['TokenEmbedding_0.Embedding.embedding'][:, xb] + P['TokenEmbedding_0.PositionEmbedding.embedding'][:, None]
        q = (torch.einsum('entc,echd->enhtd', e, P['MDPA.query.kernel']) + P['MDPA.query.bias'][:, None, :, None]) / math.sqrt(hd)
        k = torch.einsum('entc,echd->enhtd', e, P['MDPA.key.kernel']) + P['MDPA.key.bias'][:, None, :, None]
        v = torch.einsum('entc,echd->enhtd', e, P['MDPA.value.kernel']) + P['MDPA.value.bias'][:, None, :, None]
        m = xb != 0
        mask = (m[:, None, :, None] & m[:, None, None, :])[None]
        s = torch.where(mask, q @ k.transpose(-1, -2), neg)
        o = torch.softmax(s, dim=-1) @ v
        z = torch.einsum('enhtd,ehdc->entc', o, P['MDPA.out.kernel']).mean(dim=2) + P['MDPA.out.bias'][:, None]
        for i in range(len(spec.projection_dim)):
            z = gelu(z @ P[f'projection_{i}.kernel'] + P[f'projection_{i}.bias'][:, None])
        lg = z @ P['classifier.kernel'] + P['classifier.bias'][:, None]
        return torch.log_softmax(lg, dim=-1).gather(2, yb[None, :, None].expand(E, -1, 1)).sum()

    def once():
        th = theta.detach().requires_grad_(True)
        for r0 in range(0, x.shape[0], chunk):
            loglik(th, x[r0:r0 + chunk], y[r0:r0 + chunk]).backward()
        return th.grad - th.detach() / spec.prior_scale ** 2

    try:
        once()
        torch.cuda.synchronize()
    except RuntimeError as exc:                     # e.g. out of memory
        return None, f'{type(exc).__name__}: {str(exc)[:120]}'
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, None


def run(shape, E, N, reps):
    spec = WideAttentionSpec(10000, 70, 192, n_classes=2, use_bias=True, prior='Normal', **SHAPES[shape])
    x, y = synthetic_text(np.random.Generator(np.random.PCG64(0)), N, 70, 10000, 2)
    rng = np.random.default_rng(0)
    eng = Engine(spec, torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.int32)), device='cuda:0')
    th = torch.from_numpy((0.1 * rng.standard_normal((E, spec.n_params))).astype(np.float32)).cuda()
    eng.logpost_grad(th)
    torch.cuda.synchronize()
    eng.grad_timing_begin()
    for _ in range(reps):
        eng.logpost_grad(th)
    torch.cuda.synchronize()
    grad_ms, n = eng.grad_timing_end()
    grad_ms /= max(n, 1)
    st = eng.init(th, seed=0)
    eng.step(st, 1e-3, 1.0, n_steps=2, seed=0, inplace=True, want_info=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.step(st, 1e-3, 1.0, n_steps=reps, seed=0, step_offset=2, inplace=True, want_info=False)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / reps
    # one warm-start step on a 256-row minibatch (adamw, the reference's settings)
    thw = th.clone()
    ost = {'name': 'adamw', 'learning_rate': 0.01, 'b1': 0.9, 'b2': 0.999, 'eps': 1e-8, 'weight_decay': 0.001, 't': 0,
           'm': torch.zeros_like(thw), 'v': torch.zeros_like(thw)}
    active = torch.ones(E, dtype=torch.bool, device='cuda')
    eng.set_row_window(0, 256)
    eng.warmstart_step(thw, ost, active)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(reps):
        eng.set_row_window(256 * (k + 1), 256)
        eng.warmstart_step(thw, ost, active)
    torch.cuda.synchronize()
    warm_ms = (time.perf_counter() - t0) * 1e3 / reps
    eng.set_row_window(0, 0)
    fl = spec.flops_per_sequence * N * E
    floor_ms = fl / (PEAK_FP32_TFLOPS * 1e12) * 1e3
    yard_ms, yard_err = torch_yardstick(spec, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), th, max(2, reps // 4))
    rec = dict(shape=shape, E=E, N=N, d=spec.n_params, grad_kernel=eng.grad_kernel, grad_ms=round(grad_ms, 3),
               mclmc_step_ms=round(step_ms, 3), warmstart_step_256_ms=round(warm_ms, 3),
               slab_bytes=eng.slab_bytes, slab_rows=eng.slab_bytes // (4 * ((spec.n_params + 3) // 4 * 4)), tflop_per_grad=round(fl / 1e12, 3), fp32_floor_ms=round(floor_ms, 3),
               fraction_of_fp32_peak=round(floor_ms / grad_ms, 3),
               torch_autograd_ms=None if yard_ms is None else round(yard_ms, 2), torch_error=yard_err,
               speedup_vs_torch=None if yard_ms is None else round(yard_ms / grad_ms, 2), launch=eng.grad_launch_info(E))
    print(json.dumps(rec, default=str), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', nargs='+', choices=sorted(SHAPES), default=['stock', 'larger'])
    ap.add_argument('--E', type=int, nargs='+', default=[1, 8])
    ap.add_argument('--N', type=int, default=35000)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    for shape in a.shape:
        for E in a.E:
            run(shape, E, a.N, a.reps)


if __name__ == '__main__':
    main()

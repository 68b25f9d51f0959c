"""AttentionClassifier timing (k_grad_attn): the grad kernel by HIP events, one MCLMC step, the FLOP model and its fraction of the
fp32 peak, and a torch fp32 yardstick (the same model through autograd, chains batched as a leading axis, rows in chunks) on the
same GPU.

    python tools/attn_time.py [--E 8] [--N 35000] [--reps 10]

The stock shape of experiments/mclmc_seqmod_synthetic.yaml: V = 1000, T = 70, C = 48, 8 heads, qkv_dim 64, projection [32],
2 classes, no bias, Normal(0, 0.2) prior; synthetic token rows.  One JSON line per ensemble size.
FLOP model per sequence and chain: 3 x forward, forward = 2 T C 3D + 4 T^2 D + 2 T D C + sum 2 P_{i-1} P_i (AttentionSpec).
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
from mile_amd.spec import AttentionSpec

PEAK_FP32_TFLOPS = 157.3     # MI355X fp32 (vector and f32 MFMA)


def torch_yardstick(spec, x, y, theta, reps, chunk=2048):
    """Gradient of the summed log-likelihood + Normal prior for all chains at once, fp32, eager torch autograd on the GPU;
    the rows go in chunks so that the [E, chunk, H, T, T] scores fit in memory."""
    leaves = spec.leaves()
    E, T = theta.shape[0], spec.context_len
    C, H, D = spec.emb_size, spec.n_heads, spec.qkv_dim
    hd = D // H
    neg = torch.finfo(torch.float32).min

    def loglik(th, xb, yb):
        P = {n: th[:, o:o + int(np.prod(sh))].reshape((E,) + tuple(sh)) for n, o, sh in leaves}
        e = P['TokenEmbedding_0.Embedding.embedding'][:, xb] + P['TokenEmbedding_0.PositionEmbedding.embedding'][:, None]
        q = torch.einsum('entc,echd->enhtd', e, P['MDPA.query.kernel']) / math.sqrt(hd)
        k = torch.einsum('entc,echd->enhtd', e, P['MDPA.key.kernel'])
        v = torch.einsum('entc,echd->enhtd', e, P['MDPA.value.kernel'])
        m = xb != 0
        mask = (m[:, None, :, None] & m[:, None, None, :])[None]
        s = torch.where(mask, q @ k.transpose(-1, -2), neg)
        o = torch.softmax(s, dim=-1) @ v
        out = torch.einsum('enhtd,ehdc->entc', o, P['MDPA.out.kernel']).mean(dim=2)
        z = out
        for i in range(len(spec.projection_dim)):
            z = torch.nn.functional.gelu(z @ P[f'projection_{i}.kernel'], approximate='tanh')
        lg = z @ P['classifier.kernel']
        return torch.log_softmax(lg, dim=-1).gather(2, yb[None, :, None].expand(E, -1, 1)).sum()

    def once():
        th = theta.detach().requires_grad_(True)
        for r0 in range(0, x.shape[0], chunk):
            loglik(th, x[r0:r0 + chunk], y[r0:r0 + chunk]).backward()
        g = th.grad - th.detach() / 0.04
        return g

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


def run(E, N, reps):
    spec = AttentionSpec(1000, 70, 48, 8, 64, n_classes=2, projection_dim=(32,), use_bias=False, prior='Normal', prior_scale=0.2)
    x, y = synthetic_text(np.random.Generator(np.random.PCG64(0)), N, 70, 1000, 2)
    X = torch.from_numpy(x.astype(np.float32))
    eng = Engine(spec, X, torch.from_numpy(y.astype(np.int32)), device='cuda:0')
    rng = np.random.default_rng(0)
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
    fl = spec.flops_per_sequence * N * E
    floor_ms = fl / (PEAK_FP32_TFLOPS * 1e12) * 1e3
    yard_ms, yard_err = torch_yardstick(spec, torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), th, max(2, reps // 4))
    info = eng.grad_launch_info(E) if hasattr(eng, 'grad_launch_info') else None
    rec = dict(E=E, N=N, d=spec.n_params, grad_kernel=eng.grad_kernel, grad_ms=round(grad_ms, 3), mclmc_step_ms=round(step_ms, 3),
               tflop_per_grad=round(fl / 1e12, 3), fp32_floor_ms=round(floor_ms, 3), fraction_of_fp32_peak=round(floor_ms / grad_ms, 3),
               torch_autograd_ms=None if yard_ms is None else round(yard_ms, 2), torch_error=yard_err,
               speedup_vs_torch=None if yard_ms is None else round(yard_ms / grad_ms, 2), launch=info)
    print(json.dumps(rec, default=str), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--E', type=int, nargs='+', default=[8])
    ap.add_argument('--N', type=int, default=35000)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    for E in a.E:
        run(E, a.N, a.reps)


if __name__ == '__main__':
    main()

"""LeNetti timing (k_grad_lenetti): the grad kernel by HIP events, one MCLMC step, the FLOP model and its fraction of the fp32
peak, and a torch fp32 yardstick (the same net through autograd, chains batched by torch.func.vmap) on the same GPU.

    python tools/lenetti_time.py [--E 10 128] [--N 48000] [--reps 20]

MNIST-shaped images (1 x 28 x 28, 10 classes, relu).  One JSON line per ensemble size.
FLOP model per image and chain: forward conv 2 (9C P), fc1 forward 2 (8P), fc1 weight gradient 2 (8P), fc1 input gradient 2 (8P),
conv weight gradient 2 (9C P): 2 (9C P) 2 + 2 (8P) 3 (the 8-wide tail is ignored).
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from mile_amd import LeNettiSpec
from mile_amd.engine import Engine

PEAK_FP32_TFLOPS = 157.3     # MI355X vector fp32


def flops_per_grad(C, H, W, N, E):
    P = (H + 2) * (W + 2)
    return (2 * (9 * C * P) * 2 + 2 * (8 * P) * 3) * N * E


def torch_yardstick(spec, X, y, theta, reps):
    """value_and_grad of the summed log-likelihood + Normal prior, vmapped over the chains, fp32, eager torch on the GPU."""
    import torch.nn.functional as F
    from torch.func import grad_and_value, vmap
    leaves = spec.leaves()

    def logpost(th):
        p = {n: th[o:o + int(np.prod(sh))].reshape(sh) for n, o, sh in leaves}
        w = p['core.conv1.kernel'].permute(3, 2, 0, 1)
        h = torch.relu(F.conv2d(X, w, p['core.conv1.bias'], padding=2)).reshape(X.shape[0], -1)
        for name in ('fc1', 'fc2', 'fc3'):
            h = torch.relu(h @ p[f'core.{name}.kernel'] + p[f'core.{name}.bias'])
        out = h @ p['core.fc4.kernel'] + p['core.fc4.bias']
        ll = torch.log_softmax(out, dim=-1).gather(1, y[:, None]).sum()
        return ll - 0.5 * (th * th).sum()

    f = vmap(grad_and_value(logpost))
    try:
        f(theta)
        torch.cuda.synchronize()
    except RuntimeError as exc:                     # e.g. out of memory at large E
        return None, f'{type(exc).__name__}: {str(exc)[:120]}'
    t0 = time.perf_counter()
    for _ in range(reps):
        f(theta)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps, None


def run(E, N, reps):
    C, H, W, K = 1, 28, 28, 10
    rng = np.random.default_rng(0)
    X = torch.from_numpy(rng.standard_normal((N, C, H, W)).astype(np.float32))
    y = torch.from_numpy(rng.integers(0, K, N).astype(np.int32))
    spec = LeNettiSpec(C, H, W, K, activation='relu', prior='Normal')
    eng = Engine(spec, X, y, device='cuda:0')
    th = torch.from_numpy((0.03 * rng.standard_normal((E, spec.n_params))).astype(np.float32)).cuda()
    eng.logpost_grad(th)
    torch.cuda.synchronize()
    eng.grad_timing_begin()
    for _ in range(reps):
        eng.logpost_grad(th)
    torch.cuda.synchronize()
    grad_ms, n = eng.grad_timing_end()
    grad_ms /= max(n, 1)
    st = eng.init(th, seed=0)
    eng.step(st, 1e-3, 1.0, n_steps=3, seed=0, inplace=True, want_info=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.step(st, 1e-3, 1.0, n_steps=reps, seed=0, step_offset=3, inplace=True, want_info=False)
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / reps
    fl = flops_per_grad(C, H, W, N, E)
    floor_ms = fl / (PEAK_FP32_TFLOPS * 1e12) * 1e3
    yard_ms, yard_err = torch_yardstick(spec, X.cuda(), y.long().cuda(), th, max(3, reps // 4))
    rec = dict(E=E, N=N, d=spec.n_params, grad_kernel=eng.grad_kernel, grad_ms=round(grad_ms, 4), mclmc_step_ms=round(step_ms, 4),
               gflop_per_grad=round(fl / 1e9, 2), fp32_floor_ms=round(floor_ms, 4), fraction_of_fp32_peak=round(floor_ms / grad_ms, 3),
               torch_vmap_ms=None if yard_ms is None else round(yard_ms, 3), torch_error=yard_err,
               speedup_vs_torch=None if yard_ms is None else round(yard_ms / grad_ms, 1))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--E', type=int, nargs='+', default=[10, 128])
    ap.add_argument('--N', type=int, default=48000)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    for E in a.E:
        run(E, a.N, a.reps)


if __name__ == '__main__':
    main()

"""Lockstep NUTS timing (mile_nuts_step): time per leapfrog round split into the grad launch and the rest of the round,
host syncs per NUTS step, lockstep efficiency, and the MCLMC update cost per gradient on the same shape for comparison.

    python tools/nuts_time.py [--steps 20] [--eps-stock 0.01] [--eps-b2 0.005]

Shapes: the stock airfoil net ([16, 16, 2], 12 chains, N = 1052) and B2 ([5, 64, 64, 64, 2], 128 chains).  The step
size is fixed (no adaptation) so that the tree depth is comparable between runs; one JSON line per shape.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from mile_amd import ModelSpec
from mile_amd.engine import Engine


def run(name, hs, E, N, eps, steps, M=10):
    rng = np.random.default_rng(0)
    X = torch.from_numpy(rng.standard_normal((N, 5)).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
    eng = Engine(ModelSpec(5, hs), X, y, device='cuda:0')
    th = torch.from_numpy((0.1 * rng.standard_normal((E, eng.d))).astype(np.float32))
    s = eng.nuts_init(th)
    eng.nuts_step(s, eps, 1.0, n_steps=3, max_num_doublings=M, seed=1, inplace=True)    # warm caches / burn in a little
    torch.cuda.synchronize()
    stats = (C.c_int64 * 2)(0, 0)
    t0 = time.perf_counter()
    _, info, _ = eng.nuts_step(s, eps, 1.0, n_steps=steps, max_num_doublings=M, seed=2, step_offset=3, inplace=True,
                               stats=stats)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the same steps again with HIP events around the grad launches only
    s2 = eng.nuts_init(th)
    eng.nuts_step(s2, eps, 1.0, n_steps=3, max_num_doublings=M, seed=1, inplace=True)
    torch.cuda.synchronize()
    eng.grad_timing_begin()
    eng.nuts_step(s2, eps, 1.0, n_steps=steps, max_num_doublings=M, seed=2, step_offset=3, inplace=True)
    torch.cuda.synchronize()
    grad_ms, n_grad = eng.grad_timing_end()
    rounds, syncs = int(stats[0]), int(stats[1])
    leapfrogs = info.num_integration_steps.double().mean().item() * steps     # mean per chain over the steps
    # MCLMC on the same shape: (time per step - its two grad launches) / 2 = update cost per gradient
    st = eng.init(th, seed=0)
    eng.step(st, 1e-3, 1.0, n_steps=20, seed=0, inplace=True, want_info=False)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    eng.step(st, 1e-3, 1.0, n_steps=200, seed=0, step_offset=20, inplace=True, want_info=False)
    torch.cuda.synchronize()
    mclmc_ms = (time.perf_counter() - t1) * 1e3 / 200
    eng.grad_timing_begin()
    eng.step(st, 1e-3, 1.0, n_steps=200, seed=0, step_offset=220, inplace=True, want_info=False)
    torch.cuda.synchronize()
    mg_ms, mg_n = eng.grad_timing_end()
    out = {'shape': name, 'E': E, 'd': eng.d, 'grad_kernel': eng.grad_kernel, 'eps': eps, 'nuts_steps': steps,
           'rounds': rounds, 'host_syncs_per_step': syncs / steps,
           'mean_leapfrogs_per_chain_step': leapfrogs / steps, 'lockstep_efficiency': leapfrogs / rounds,
           'mean_expansions': info.num_trajectory_expansions.double().mean().item(),
           'mean_acceptance': info.acceptance_rate.double().mean().item(),
           'us_per_round': wall * 1e6 / rounds, 'grad_us_per_round': grad_ms * 1e3 / n_grad,
           'non_grad_us_per_round': (wall * 1e3 - grad_ms) * 1e3 / rounds,
           'mclmc_us_per_step': mclmc_ms * 1e3, 'mclmc_update_us_per_grad': (mclmc_ms * 1e3 - mg_ms * 1e3 / 200) / 2,
           'mclmc_grad_kernel_us': mg_ms * 1e3 / mg_n}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--eps-stock', type=float, default=0.01)
    ap.add_argument('--eps-b2', type=float, default=0.005)
    a = ap.parse_args()
    run('stock_16x16_e12', (16, 16, 2), 12, 1052, a.eps_stock, a.steps)
    run('b2_64x3_e128', (64, 64, 64, 2), 128, 1052, a.eps_b2, a.steps)


if __name__ == '__main__':
    main()

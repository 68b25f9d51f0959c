"""Stacking timing: Engine.stack_eval (mile_stack_eval: the responsibilities in row tiles, their fp64 Gram product in fixed-order
blocks) against metrics.stack_eval_dense (the torch fp64 form: one [C, N] responsibility tensor and a matmul) on the same
matrix and the same device, and a whole metrics.stacking_weights solve on each:

    python tools/stack_time.py [--reps 3] [--shapes stock b2 large]

Shapes: the stock airfoil run (12 chains x 1052 train rows), the B2 schedule (128 x 1052) and the largest ensemble the kernels
take on a large split (1024 x 36 000).  The matrix is synthetic: Normal log densities of N targets under C predictors of
differing bias, slope and scale.  Host clock around work that ends in a device synchronise; the two paths alternate, `reps`
runs each after one warm-up call of each, the best and all runs reported.  Peak device memory per path: torch's peak allocation
above what was live before (the inputs), plus the workspace the library allocates and frees inside the call.
``round_trips`` of a solve: its evaluations, each of which ends in a copy to the host (1 + Newton steps + line-search
evaluations).  One JSON line per shape.
"""
import argparse
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import ModelSpec
from mile_amd import metrics as M
from mile_amd.engine import Engine

SHAPES = {'stock': (12, 1052), 'b2': (128, 1052), 'large': (1024, 36000)}
OUT = ('score', 'grad', 'hess', 'used')


def once(fn):
    """(result, seconds, peak bytes) of one call of fn: torch's peak allocation above what was live before."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return res, dt, int(torch.cuda.max_memory_allocated() - live)


def workspace_bytes(C_, N):
    """What mile_stack_eval allocates and frees inside a call that asks for a sum (mile_stack.h): the responsibilities of a row
    tile [C + 2][Nt] within 256 MiB and the blocks' partial sums [nb][C + 2][C + 2] within 64 MiB, fp64."""
    cx = C_ + 2
    nt = min(N, (256 << 20) // (8 * cx))
    nb_max = max(1, min(1024, (64 << 20) // (8 * cx * cx)))
    B = (-(-N // nb_max) + 31) // 32 * 32
    r256 = lambda b: (b + 255) // 256 * 256
    return r256(cx * nt * 8) + r256(-(-N // B) * cx * cx * 8)


def matrix(C_, N, g, dev):
    f = torch.randn(N, generator=g, device=dev, dtype=torch.float64)
    y = f + 0.5 * torch.randn(N, generator=g, device=dev, dtype=torch.float64)
    slope = 1.0 + 0.6 * torch.randn(C_, generator=g, device=dev, dtype=torch.float64)
    bias = 0.4 * torch.randn(C_, generator=g, device=dev, dtype=torch.float64)
    scale = 0.7 * torch.exp(0.3 * torch.randn(C_, generator=g, device=dev, dtype=torch.float64))
    mu = slope[:, None] * f[None] + bias[:, None] + 0.3 * torch.randn((C_, N), generator=g, device=dev, dtype=torch.float64)
    return -0.5 * ((y[None] - mu) / scale[:, None]) ** 2 - torch.log(scale)[:, None] - 0.5 * math.log(2 * math.pi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2', 'large'], choices=sorted(SHAPES))
    ap.add_argument('--skip-dense', action='store_true', help='time the kernels only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    eng = Engine(ModelSpec(5, (16, 16, 2)), torch.zeros((64, 5)), torch.zeros(64), device=dev)     # stack_eval needs no handle
    for name in args.shapes:
        C_, N = SHAPES[name]
        lpd = matrix(C_, N, g, dev)
        w = torch.full((C_,), 1.0 / C_, dtype=torch.float64, device=dev)
        kern = lambda: eng.stack_eval(lpd, w, outputs=OUT)
        dense = lambda: M.stack_eval_dense(lpd, w, outputs=OUT)
        score_only = lambda: eng.stack_eval(lpd, w, outputs=('score',))
        once(kern)
        if not args.skip_dense:
            once(dense)
        t_new, t_old, m_new, m_old, t_sc, b = [], [], [], [], [], None
        for _ in range(args.reps):                                              # alternating
            a, t, m = once(kern)
            t_new.append(t)
            m_new.append(m)
            t_sc.append(once(score_only)[1])
            if not args.skip_dense:
                b, t, m = once(dense)
                t_old.append(t)
                m_old.append(m)
        rec = {'shape': name, 'C': C_, 'N': N, 'gram_fma': C_ * C_ * N, 'kernel_s': min(t_new), 'kernel_runs_s': t_new,
               'kernel_peak_bytes': max(m_new) + workspace_bytes(C_, N), 'kernel_workspace_bytes': workspace_bytes(C_, N),
               'kernel_score_only_s': min(t_sc)}
        sol, t_sol, _ = once(lambda: M.stacking_weights(lpd, eval=eng.stack_eval))
        rec.update(solve_kernel_s=t_sol, solve_iterations=sol['iterations'], solve_score_evals=sol['score_evals'],
                   solve_round_trips=1 + sol['iterations'] + sol['score_evals'], solve_gap=sol['gap'], solve_converged=sol['converged'])
        if b is not None:
            rec.update(dense_s=min(t_old), dense_runs_s=t_old, dense_peak_bytes=max(m_old), speedup=min(t_old) / min(t_new))
            for k in ('score', 'grad', 'hess'):
                rec[f'max_diff_{k}'] = float(((a[k] - b[k]).abs() / b[k].abs().clamp(min=1.0)).max())
            assert int(a['used']) == int(b['used'])
            sol_d, t_sol_d, _ = once(lambda: M.stacking_weights(lpd))
            rec.update(solve_dense_s=t_sol_d, solve_dense_iterations=sol_d['iterations'],
                       solve_max_diff_w=float(abs(sol['w'] - sol_d['w']).max()))
        print(json.dumps(rec), flush=True)
        del lpd, w, a, b


if __name__ == '__main__':
    main()

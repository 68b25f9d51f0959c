"""Streamed-LPPD timing: metrics.streamed_lppd (mile_lppd_stream: the forward in passes, reduced on the device in a streaming
log-sum-exp) against Engine.pointwise_loglik followed by metrics.lppd, metrics.running_lppd and the per-chain LPPD on the
dense [C, S, N] tensor.

    python tools/lppd_time.py [--reps 3] [--shapes b2 large] [--points 64] [--draws-per-pass K]

Shapes: the B2 run (128 chains x 1000 draws, 301 rows) and the same draws on 4000 rows (2 GB of pointwise log-likelihoods:
the dense path still fits), both on the B2 net 5 -> [64, 64, 64, 2] with N(0, 0.1^2) draws.
Host clock around work that ends in a device synchronise, best of `reps` after one warm-up call.  Peak device memory per
path: torch's peak allocation over the calls (torch.cuda.max_memory_allocated above what was live before) plus what the
library allocated itself (the drop in free device memory that torch's own reservations do not explain); the library's state
workspace (mile_lppd_stream_workspace) is reported on its own.  One JSON line: a record per shape.
"""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import ModelSpec
from mile_amd import metrics as M
from mile_amd.engine import Engine

SHAPES = {'b2': (128, 1000, 301), 'large': (128, 1000, 4000)}


def best(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def measured(fn, reps):
    """(best seconds, peak bytes) of fn: torch's peak allocation above what was live before, plus the library's own."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    live, free0, res0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    t = best(fn, reps)
    lib = (free0 - torch.cuda.mem_get_info()[0]) - (torch.cuda.memory_reserved() - res0)
    return t, int(torch.cuda.max_memory_allocated() - live + max(lib, 0))


def dense(eng, theta, X, y):
    """What evaluate.py does without --running, plus the whole running curve."""
    pw = eng.pointwise_loglik(theta, X, y)
    return {'lppd': M.lppd(pw), 'run_chain': M.running_lppd(pw),
            'chain_lppd': torch.stack([M.lppd(pw[c:c + 1]) for c in range(pw.shape[0])])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['b2', 'large'], choices=sorted(SHAPES))
    ap.add_argument('--points', type=int, default=64, help='curve points of the streamed call')
    ap.add_argument('--draws-per-pass', type=int, default=0)
    ap.add_argument('--skip-dense', action='store_true', help='time the streamed call only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    spec = ModelSpec(5, (64, 64, 64, 2))
    g = torch.Generator(device=dev).manual_seed(0)
    recs = []
    for name in args.shapes:
        C, S, N = SHAPES[name]
        theta = 0.1 * torch.randn((C, S, spec.n_params), generator=g, device=dev)
        X = torch.randn((N, 5), generator=g, device=dev)
        y = torch.randn(N, generator=g, device=dev)
        eng = Engine(spec, X[:64], y[:64], device=dev)               # a fresh handle: its workspace starts empty
        pts = M.curve_points(S, args.points)
        run = lambda: M.streamed_lppd(eng, theta, X, y, curve_points=pts, max_draws_per_pass=args.draws_per_pass)
        t_new, m_new = measured(run, args.reps)
        rec = {'shape': name, 'C': C, 'S': S, 'N': N, 'kernel': eng.grad_kernel, 'points': len(pts),
               'draws_per_pass': args.draws_per_pass, 'dense_bytes': C * S * N * 4,
               'state_workspace_bytes': eng.lppd_stream_workspace(C, N), 'streamed_s': t_new, 'streamed_peak_bytes': m_new}
        if not args.skip_dense:
            t_fwd, _ = measured(lambda: eng.pointwise_loglik(theta, X, y), args.reps)
            t_old, m_old = measured(lambda: dense(eng, theta, X, y), args.reps)
            a, b = run(), dense(eng, theta, X, y)
            rec.update(pointwise_only_s=t_fwd, dense_s=t_old, dense_peak_bytes=m_old, speedup=t_old / t_new,
                       lppd_diff=float((a['lppd'] - b['lppd'].double()).abs()),
                       chain_lppd_max_diff=float((a['chain_lppd'] - b['chain_lppd'].double()).abs().max()),
                       run_chain_last_diff=float((a['run_chain'][-1] - b['run_chain'][-1].double()).abs()),
                       dense_run_chain_neg_inf=int(torch.isneginf(b['run_chain']).sum()))
        recs.append(rec)
        del eng, theta, X, y
        torch.cuda.empty_cache()
    print(json.dumps({'tool': 'lppd_time', 'reps': args.reps, 'shapes': recs}), flush=True)


if __name__ == '__main__':
    main()

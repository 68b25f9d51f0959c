"""Alignment timing: the library call (mile_align_fcn through mile_amd.metrics) against metrics.align_dense -- fp64 similarities as
one matrix product per layer on the device, then scipy.optimize.linear_sum_assignment per draw on the host -- on the same machine.
There is no torch form of the assignment, so align_dense is the yardstick.

    python tools/align_time.py [--reps 5] [--dense-reps 5] [--rounds 3] [--shapes stock b2] [--noise 0.3] [--sign] [--no-index]
                               [--skip-dense]

Shapes: the stock run's [12, 1000] draws of 5 -> 16 -> 16 -> 2 and B2's [128, 1000] draws of 5 -> 64 -> 64 -> 64 -> 2 (tanh, so
that --sign applies).  The draws are noisy copies (--noise) of one centre drawn from N(0, 0.7^2), generated on the device, each
with its hidden units scrambled by ordering them by their norm (metrics.canonicalize_dense); the reference is the centre.  The two
paths alternate in one process: per round each is timed as best of its reps around a device synchronise (host clock), after a
warm-up of each at that shape; the spread is over the rounds.  Peak memory: torch's allocator high-water mark above the input, per
path.  One JSON line per shape, with the share of draws on which the two paths give the same bits.  --skip-dense runs the library
call alone (for a kernel trace).
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

SHAPES = {'stock': (12, 1000, 5, (16, 16, 2)), 'b2': (128, 1000, 5, (64, 64, 64, 2))}


def best(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts)


def peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--dense-reps', type=int, default=None, help='reps of align_dense (default: --reps)')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--noise', type=float, default=0.3)
    ap.add_argument('--sign', action='store_true')
    ap.add_argument('--no-index', action='store_true', help='the library call without perm, sign and score')
    ap.add_argument('--skip-dense', action='store_true', help='time the library call only (for a profiler run)')
    args = ap.parse_args()
    dense_reps = args.dense_reps or args.reps
    dev = 'cuda:0'
    for name in args.shapes:
        C, S, fin, hs = SHAPES[name]
        spec = ModelSpec(fin, hs, activation='tanh', task='regr')
        Mn, d, H = C * S, spec.n_params, M.canonical_hidden(spec)
        gen = torch.Generator(device=dev).manual_seed(1)
        centre = 0.7 * torch.randn(d, device=dev, generator=gen)
        theta = M.canonicalize_dense(spec, centre[None] + args.noise * torch.randn((Mn, d), device=dev, generator=gen), 'norm', False)[0]
        lib = lambda: M._library_align(spec, theta, centre, args.sign, not args.no_index, not args.no_index)
        dense = lambda: M.align_dense(spec, theta, centre, args.sign)
        rec = {'shape': name, 'M': Mn, 'd': d, 'H': H, 'noise': args.noise, 'sign': args.sign, 'index': not args.no_index}
        lib()                                                        # warm-up of each path at this shape
        if not args.skip_dense:
            got, ref = lib(), dense()
            rec['draws_equal'] = float((got[0] == ref[0]).all(dim=1).float().mean())
            rec['dropped'] = int(got[4].sum())
            del got, ref
        t_lib, t_dense = [], []
        for _ in range(args.rounds):                                 # the two paths alternate
            t_lib.append(best(lib, args.reps))
            if not args.skip_dense:
                t_dense.append(best(dense, dense_reps))
        rec.update(library_s=min(t_lib), library_s_rounds=t_lib, library_draws_per_s=Mn / min(t_lib), library_peak_bytes=peak(lib, dev))
        if not args.skip_dense:
            rec.update(dense_s=min(t_dense), dense_s_rounds=t_dense, dense_peak_bytes=peak(dense, dev), ratio=min(t_dense) / min(t_lib),
                       ratio_rounds=[b / a for a, b in zip(t_lib, t_dense)])
        print(json.dumps(rec), flush=True)
        del theta


if __name__ == '__main__':
    main()

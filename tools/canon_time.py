"""Canonical-ordering timing: the library call (mile_canonicalize_fcn through mile_amd.metrics) against the torch composition
metrics.canonicalize_dense -- a stable sort per hidden layer plus three gathers per layer -- on the same device.

    python tools/canon_time.py [--reps 5] [--rounds 3] [--shapes stock b2] [--key bias] [--sign] [--no-index] [--skip-dense]

Shapes: the stock run's [12, 1000] draws of 5 -> 16 -> 16 -> 2 and B2's [128, 1000] draws of 5 -> 64 -> 64 -> 64 -> 2 (tanh, so
that --sign applies), N(0, 0.7^2) draws generated on the device.  The two paths alternate in one process: per round each is
timed as best of `reps` around a device synchronise (host clock), after a warm-up of each at that shape; the spread is over
the rounds.  Algorithmic bytes: 8 M d (every float read once, written once) plus 5 M H with both index outputs; the rate they
imply is printed for both paths.  Peak memory: torch's allocator high-water mark above the input, per path.  One JSON line per
shape.  --skip-dense runs the library call alone (for a kernel trace).
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
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--shapes', nargs='+', default=['stock', 'b2'], choices=sorted(SHAPES))
    ap.add_argument('--key', default='bias', choices=M.CANON_KEYS)
    ap.add_argument('--sign', action='store_true')
    ap.add_argument('--no-index', action='store_true', help='the library call without perm and sign')
    ap.add_argument('--skip-dense', action='store_true', help='time the library call only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    for name in args.shapes:
        C, S, fin, hs = SHAPES[name]
        spec = ModelSpec(fin, hs, activation='tanh', task='regr')
        Mn, d, H = C * S, spec.n_params, M.canonical_hidden(spec)
        theta = 0.7 * torch.randn((Mn, d), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        lib = lambda: M._library_canonicalize(spec, theta, args.key, args.sign, not args.no_index)
        dense = lambda: M.canonicalize_dense(spec, theta, args.key, args.sign)
        nbytes = 8 * Mn * d + (0 if args.no_index else 5 * Mn * H)
        rec = {'shape': name, 'M': Mn, 'd': d, 'H': H, 'key': args.key, 'sign': args.sign, 'index': not args.no_index,
               'algorithmic_bytes': nbytes}
        lib()                                                        # warm-up of each path at this shape
        if not args.skip_dense:
            got, ref = lib(), dense()
            rec['equal'] = all(bool(torch.equal(g, r)) for g, r in zip(got, ref) if g is not None)
            del got, ref
        t_lib, t_dense = [], []
        for _ in range(args.rounds):                                 # the two paths alternate
            t_lib.append(best(lib, args.reps))
            if not args.skip_dense:
                t_dense.append(best(dense, args.reps))
        rec.update(library_s=min(t_lib), library_s_rounds=t_lib, library_GBps=nbytes / min(t_lib) / 1e9,
                   library_peak_bytes=peak(lib, dev))
        if not args.skip_dense:
            rec.update(dense_s=min(t_dense), dense_s_rounds=t_dense, dense_GBps=nbytes / min(t_dense) / 1e9,
                       dense_peak_bytes=peak(dense, dev), ratio=min(t_dense) / min(t_lib),
                       ratio_rounds=[b / a for a, b in zip(t_lib, t_dense)])
        print(json.dumps(rec), flush=True)
        del theta


if __name__ == '__main__':
    main()

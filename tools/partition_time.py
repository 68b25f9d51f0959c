"""Partition sampling against full-parameter sampling of the same net, ensemble and data: one MCLMC step by wall clock around
a synchronise, and the gradient launch alone by HIP events (in partition mode that includes the scatter / gather launches of
the general path).

    python tools/partition_time.py [--steps 2000] [--repeats 5]

Shapes: the reference's partition net [8 -> 16 x 8 -> 2] (energy: N = 537 training rows) with 12 and 128 chains, where AUTO
runs the partition form of k_grad_narrow, and B2's [5 -> 64 x 3 -> 2] (airfoil: N = 1052) with 128 chains on the general path
(k_grad_w64 split-bf16 between k_part_scatter and k_part_gather; the full run there fuses its updates into the grad launch,
the partition run cannot).  Both modes are warmed up, then timed alternately `repeats` times in the same process; the table
gives the median and the min..max spread of each.  One JSON line per shape.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch

from mile_amd import ModelSpec
from mile_amd.engine import Engine

SHAPES = [('partition net', 8, (16,) * 8 + (2,), 537, 12), ('partition net', 8, (16,) * 8 + (2,), 537, 128),
          ('B2 3x64', 5, (64, 64, 64, 2), 1052, 128)]


def timed(eng, theta, steps):
    st = eng.init(theta, seed=1)
    eng.step(st, 1e-3, 15.0, n_steps=50, seed=1, inplace=True, want_info=False)        # warm-up of this shape
    torch.cuda.synchronize()

    def once():
        t0 = time.perf_counter()
        eng.step(st, 1e-3, 15.0, n_steps=steps, seed=1, step_offset=50, inplace=True, want_info=False)
        torch.cuda.synchronize()
        step_us = (time.perf_counter() - t0) * 1e6 / steps
        eng.grad_timing_begin()
        eng.step(st, 1e-3, 15.0, n_steps=200, seed=1, step_offset=50, inplace=True, want_info=False)
        torch.cuda.synchronize()
        ms, n = eng.grad_timing_end()
        return step_us, ms * 1e3 / max(n, 1)
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('partition_time.py needs the GPU: nothing is measured without one')
    for name, F, hs, N, E in SHAPES:
        rng = np.random.default_rng(0)
        spec = ModelSpec(in_features=F, hidden_structure=hs, prior='Normal')
        X = torch.from_numpy(rng.standard_normal((N, F)).astype(np.float32))
        y = torch.from_numpy(rng.standard_normal(N).astype(np.float32))
        theta = torch.from_numpy((0.1 * rng.standard_normal((E, spec.n_params))).astype(np.float32)).cuda()
        full = Engine(spec, X, y, device='cuda:0')
        part = Engine(spec, X, y, device='cuda:0')
        part.set_partition(theta)
        runs = {'full': timed(full, theta, a.steps), 'partition': timed(part, part.partition(theta), a.steps)}
        res = {k: [] for k in runs}
        for _ in range(a.repeats):                       # alternating: both modes see the same machine state
            for k, fn in runs.items():
                res[k].append(fn())
        rec = dict(shape=name, widths=[F] + list(hs), N=N, E=E, d=full.d, d_s=part.dim, steps=a.steps, repeats=a.repeats)
        for k, eng in (('full', full), ('partition', part)):
            su, gu = [r[0] for r in res[k]], [r[1] for r in res[k]]
            rec[k] = dict(kernel=eng.grad_launch_info(E)['kernel'], step_us=round(statistics.median(su), 2),
                          step_us_min_max=[round(min(su), 2), round(max(su), 2)], grad_us=round(statistics.median(gu), 2),
                          grad_us_min_max=[round(min(gu), 2), round(max(gu), 2)])
        rec['step_ratio_partition_over_full'] = round(rec['partition']['step_us'] / rec['full']['step_us'], 3)
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()

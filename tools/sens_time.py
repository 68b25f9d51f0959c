"""Input-sensitivity timing: Engine.predict_sensitivities (mile_predict_sensitivities: one forward and P backward sweeps per
(draw, row) in k_sens_jac, reduced on the device) against metrics.sensitivities_dense on the device (the closed-form chain of
matrices in torch fp64, 64 draws at a time), against torch.func.vmap(jacrev) of the fp32 forward reduced the same way (where
[C S, N, P, F] and its intermediates fit), and against Engine.predict alone on the same inputs (what the forward costs).

    python tools/sens_time.py [--reps 3] [--nets stock b2] [--chains 12 128] [--draws 100] [--rows 301]

Nets: the stock 5 -> [16, 16, 2] and B2's 5 -> [64, 64, 64, 2], ReLU regression, N(0, 0.3^2) draws; C chains of ``--draws`` draws
on ``--rows`` rows.  Host clock around work that ends in a device synchronise, best of `reps` after one warm-up call.  Peak
device memory per path as in tools/moments_time.py.  One JSON line per (net, chains).
"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch

from mile_amd import ModelSpec
from mile_amd import metrics as M
from mile_amd.engine import Engine
from tools.moments_time import measured

NETS = {'stock': (5, (16, 16, 2)), 'b2': (5, (64, 64, 64, 2))}
VMAP_LIMIT = 1 << 30      # bytes of [C S, N, P, F] fp32 up to which the vmap(jacrev) form is tried


def vmap_jacrev(spec, theta, X, chunk=256):
    """mean, sd (ddof 1) and pos [N, P, F] from the Jacobians of every (draw, row) by torch.func: [C S, N, P, F] held whole."""
    leaves = {n: (o, s) for n, o, s in spec.leaves()}
    nl = len(spec.hidden_structure)

    def f(th, x):
        h = x
        for li in range(nl):
            ko, ks = leaves[f'{spec.root}.layer{li}.kernel']
            bo, bs = leaves[f'{spec.root}.layer{li}.bias']
            h = h @ th[ko:ko + ks[0] * ks[1]].reshape(ks) + th[bo:bo + bs[0]]
            if li < nl - 1:
                h = torch.relu(h)
        return h

    rows = torch.func.vmap(torch.func.jacrev(f, argnums=1), in_dims=(None, 0))
    J = torch.func.vmap(rows, in_dims=(0, None), chunk_size=chunk)(theta, X)
    return J.mean(dim=0), J.std(dim=0), (J > 0).float().mean(dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--nets', nargs='+', default=['stock', 'b2'], choices=sorted(NETS))
    ap.add_argument('--chains', type=int, nargs='+', default=[12, 128])
    ap.add_argument('--draws', type=int, default=100)
    ap.add_argument('--rows', type=int, default=301)
    ap.add_argument('--skip-torch', action='store_true', help='time predict_sensitivities and predict only (for a profiler run)')
    args = ap.parse_args()
    dev = 'cuda:0'
    g = torch.Generator(device=dev).manual_seed(0)
    for name in args.nets:
        F, hs = NETS[name]
        spec = ModelSpec(F, hs)
        for C in args.chains:
            S, N = args.draws, args.rows
            theta = 0.3 * torch.randn((C, S, spec.n_params), generator=g, device=dev)
            X = torch.randn((N, F), generator=g, device=dev)
            eng = Engine(spec, X[:64], torch.zeros(64, device=dev), device=dev)      # a fresh handle: its workspace starts empty
            t_new, m_new = measured(lambda: eng.predict_sensitivities(theta, X), args.reps)
            t_fwd, _ = measured(lambda: eng.predict(theta, X), args.reps)
            rec = {'net': name, 'C': C, 'S': S, 'N': N, 'jacobian_bytes': C * S * N * hs[-1] * F * 4, 'device_s': t_new,
                   'device_peak_bytes': m_new, 'predict_only_s': t_fwd, 'ratio_to_predict': t_new / t_fwd}
            if not args.skip_torch:
                t_dense, m_dense = measured(lambda: M.sensitivities_dense(spec, theta, X), args.reps)
                a, b = eng.predict_sensitivities(theta, X), M.sensitivities_dense(spec, theta, X)
                rec.update(dense_s=t_dense, dense_peak_bytes=m_dense, speedup_over_dense=t_dense / t_new,
                           max_abs_diff={k: float((a[k].double() - b[k].double()).abs().max()) for k in ('mean', 'sd', 'chain_ape', 'chain_abs')})
                if rec['jacobian_bytes'] <= VMAP_LIMIT:
                    try:
                        t_vmap, m_vmap = measured(lambda: vmap_jacrev(spec, theta.reshape(C * S, -1), X), args.reps)
                        rec.update(vmap_s=t_vmap, vmap_peak_bytes=m_vmap, speedup_over_vmap=t_vmap / t_new)
                    except torch.cuda.OutOfMemoryError:
                        rec.update(vmap_s=None, vmap_note='out of memory')
                else:
                    rec.update(vmap_s=None, vmap_note='[C S, N, P, F] beyond 1 GiB: not tried')
            print(json.dumps(rec), flush=True)
            del eng, theta, X
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()

"""The compile-time kinds of k_update_fast against its run-time-flag form, bit for bit (-m gpu).

The mid-step kind forms, reduces and exchanges only the four sums its scalar chain reads (u.u, u.g, g.g and the log-prior); the
record kind keeps the ten dot products and the log-prior.  The run-time-flag form always forms all twelve sums.  For finite states
the two must agree in every bit: a sum that is not formed would have been +0.  (Both forms share the per-element code, lane
mask included, so this comparison sees an error in the list of sums, not one in that shared code; the oracle comparisons of
tests/test_gpu_update_schedule.py cover it.)

Ten steps of one mile_step call with Philox noise, E = 3, kept every step, for

    d = 8834   the benchmark's net [5 -> 64, 64, 64, 2]: 768 threads, three quads per thread, a two-element tail (AL = 2)
    d = 8833   d % 4 = 1: a one-element tail, 4-byte loads (AL = 1)
    d = 259    one wave of 64 threads, one quad each, a three-element tail

run twice from the same start: as the library runs it (start launch, then MID and REC kinds, the record launch's noise
prefilled by the mid-step launch: mile_debug_prefill_count must say so), and with a preconditioner of ones, which
tests/test_gpu_update_schedule.py uses to reach the run-time-flag form (upd_kind is -1 under sqrt_diag_cov; g * 1 and eps * 1
are exact, and that form draws its own noise with the same counters).  Position, momentum, log-density, gradient, the kept
samples and the info of every step must be equal.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
E, N_STEPS, N_ROWS = 3, 10, 48
SEED, STEP_OFFSET = 0x5EED0123456789, 5
# d -> (F, hidden structure, grad kernel)
NETS = {8834: (5, (64, 64, 64, 2), 'mfma_w64_bf16x3'), 8833: (2, (49, 167, 2), 'generic'), 259: (2, (4, 35, 2), 'generic')}


def n_params(F, hidden):
    d, fin = 0, F
    for w in hidden:
        d += w + fin * w
        fin = w
    return d


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('d', list(NETS), ids=[f'd{d}' for d in NETS])
def test_compile_time_kinds_equal_the_run_time_form(d):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    from oracle import mclmc_oracle as O
    F, hidden, kernel = NETS[d]
    assert n_params(F, hidden) == d
    prob = O.synthetic_problem(O.ModelSpec(F, hidden), N_ROWS, E, seed=3)
    eng = Engine(ModelSpec(in_features=F, hidden_structure=hidden), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']),
                 device=DEV, grad_kernel=kernel)
    assert eng.grad_kernel == kernel and eng.d == d
    ids = torch.from_numpy((np.arange(E, dtype=np.int32) * 7919 + 13).astype(np.int32))
    s0 = eng.init(torch.from_numpy(prob['theta0']), seed=SEED, particle_ids=ids)
    eps, Lp = torch.from_numpy(prob['eps']), torch.from_numpy(prob['L'])
    kw = dict(n_steps=N_STEPS, n_thinning=1, seed=SEED, step_offset=STEP_OFFSET, particle_ids=ids, want_info=True)

    def call(**more):
        n0 = eng.debug_prefill_count()
        s1, info, samples = eng.step(s0, eps, Lp, **kw, **more)
        torch.cuda.synchronize()
        out = dict(x=_np(s1.position), u=_np(s1.momentum), logp=_np(s1.logdensity), g=_np(s1.logdensity_grad), samples=_np(samples),
                   info=np.stack([_np(info.logdensity), _np(info.kinetic_change), _np(info.energy_change)], axis=2))
        return out, eng.debug_prefill_count() - n0

    fast, n_fast = call()
    general, n_general = call(sqrt_diag_cov=torch.ones((E, d), dtype=torch.float32))
    # the fast call ran the MID kind with its noise workgroups at every step; the run-time form draws in place
    assert n_fast == N_STEPS and n_general == 0, (d, n_fast, n_general)
    assert fast['samples'].shape == (N_STEPS, E, d)
    for k, v in fast.items():
        assert np.isfinite(v).all(), (d, k)
        same = np.array_equal(v, general[k])
        print(f'\nUPDKIND d{d} {k}: {"equal" if same else "DIFFERS"}', end='')
        assert same, (d, k, np.abs(v.astype(np.float64) - general[k]).max())
    # and the chain moved: ten steps of a sampler, not a fixed point
    assert np.abs(fast['x'] - prob['theta0']).max() > 0 and not np.array_equal(fast['samples'][0], fast['samples'][-1])

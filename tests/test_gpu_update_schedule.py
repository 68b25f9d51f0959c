"""The MCLMC update kernels over every cell of their launch schedule (-m gpu): k_update_fast in its MID, REC, TUNE and run-time
forms, k_update_big, k_update_seg + k_update_seg_scalars and the two-pass k_update<false>, on the cases of
tests/update_schedule.py, against the fp64 oracle (the epilogue form inside k_grad_w64 is not in the library as built: its cells
are listed there as unreachable).  tests/test_update_schedule_host.py proves on the CPU that the table
reaches every cell, derives the bounds below and shows that each of 24 plausible kernel errors misses one of them tenfold on every
case that runs the code it breaks.

A step case is ONE mile_step call of three steps (or one) from eng.init, with n_thinning = 1 and the info of every step: the start
launch, the MID kind, the chained REC kind and the last record launch, compared with the restated call in float64
(update_schedule.simulate, which the host test holds to oracle.mclmc_step) from the device's own float32 start, on the same
explicit noise or on oracle.philox_normal of the same seed, particle ids, step and stage.  Increments are compared, not states:

    quantity         what                                                 of                                               bound
    displacement     x_i - x_(i-1), both differenced in fp64              the particle's largest oracle displacement
                                                                          + 2 fp32 ulps of max |x|                         2e-4
    momentum         final u                                              the particle's largest |u|                       5e-5
    unit norm        | |u| - 1 |                                                                                           2e-6
    logdensity       info.logdensity of every step, final logdensity      |logp|                                           2e-5
    kinetic change   info.kinetic_change of every step                    s_K = eps (b1 |g~0| + b2 |g~1| + b1 |g~2|)       3e-5
    energy change    info.energy_change of every step                     3e-5 s_K + 16 fp32 ulps of max |logp|            1
    gradient         final logdensity_grad                                its largest entry                                2e-5
    stream weight    the tuner's stream_weight                            its largest entry                                1e-5
    stream average   the tuner's stream_average                           its largest entry                                1e-5

One bound per quantity for the whole table, each with 8 r_q <= B_q <= m_q / 10 (r_q: the float32 evaluation's own error, m_q: the
least miss of a mutant; the figures are in the host test's docstring and in DESIGN.md).  A tuner case is one mile_tune call of two
steps -- the merged launch, then the unmerged record -- from step_size_max = 1.25 eps, which clamps the predictor on both sides:
step_size and step_size_max must come back equal to it bit for bit.  An offset case runs the state as contiguous views one or two
floats into a larger buffer (row_align lowers AL although d % 4 == 0) and must equal the aligned call bit for bit: AL only changes
the width of ld4 / st4, no order of summation.

Every test prints what it measured before it asserts (`pytest -s`, lines UPDCASE); the last test prints the worst value per
quantity and its case (UPDWORST).  Measured on an MI355X (8 r_q, the bound, m_q / 10 from the host test; then the device's worst):

    displacement     1.2e-04  2e-04  3.1e-03    1.5e-05  d40962
    momentum         4.4e-06  5e-05  4.2e-04    3.6e-07  d3073
    unit norm        9.3e-07  2e-06  3.1e-06    2.0e-07  d3073
    logdensity       1.3e-05  2e-05  6.2e-04    1.0e-05  d8191-x
    kinetic change   4.2e-06  3e-05  3.4e-05    2.0e-07  t7-2
    energy change    0.92     1      1.01       0.57     t16387-x
    gradient         3.6e-06  2e-05  4.9e-05    6.9e-07  t3072-sdc
    stream weight    0        1e-05  1.0e-02    0
    stream average   1.3e-06  1e-05  5.7e-03    1.9e-07  t4099-0

What the table found: no cell returns a wrong result; every offset case equals its aligned call bit for bit; the slab splits 1,
4 and 5 occur; the prefill count of every call is the restatement's.  Closest to a bound is the log-density at d = 8191 (half of
it): the prior's sum and its constant, both near 1.7e4, cancel to a log-density of 4e2 .. 1e3.

Checked by hand against two mutants of upd_fast_body itself, in scratch builds of the library: the pass-2 tail store without
`has_tail` failed the 70 cases with d % 4 != 0 that run k_update_fast or k_update_big (every step and tuner case with a tail
except the seven whose launches are all k_update_seg or k_update<false>: d16389-nobig, d36869-x, d36869-noseg-x, d40961-x,
d40961-n1-x, d40962, d40963-so-x) and nothing else; `philox_normal4(nqf - 1, ...)` for
the tail's noise failed the 48 cases with a tail and an O-step that draws in place (start launches, MILE_DEBUG bit 128, step-O,
k_update_big, the tuner's unmerged launches) and nothing else.  Both sets are what update_schedule.launches predicts.
"""
import numpy as np
import pytest

from tests import update_schedule as U

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
_WORST = {}                     # quantity -> (error, case name)
_S_CLASSES = set()


def _engine(case):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    pb = U.problem(case)
    o = pb['ospec']
    spec = ModelSpec(in_features=o.in_features, hidden_structure=o.hidden_structure, activation=o.activation, task=o.task,
                     prior=o.prior, prior_loc=o.prior_loc, prior_scale=o.prior_scale)
    eng = Engine(spec, torch.from_numpy(pb['X']), torch.from_numpy(pb['y']), device=DEV, grad_kernel=case.kernel)
    assert eng.grad_kernel == case.kernel and eng.d == U.dim(case)
    return eng


def _setenv(monkeypatch, case):
    for e in case.env:
        k, _, v = e.partition('=')
        monkeypatch.setenv(k, v or '1')


def _init(eng, case):
    pb = U.problem(case)
    if case.noise == 'explicit':
        return eng.init(torch.from_numpy(pb['theta0']), noise=torch.from_numpy(pb['z0']))
    return eng.init(torch.from_numpy(pb['theta0']), seed=U.SEED, particle_ids=torch.from_numpy(pb['ids']))


def _call_kw(case):
    pb = U.problem(case)
    kw = dict(seed=U.SEED, step_offset=U.STEP_OFFSET, particle_ids=torch.from_numpy(pb['ids']), refresh=case.refresh, want_info=True)
    if case.noise == 'explicit':
        kw['noise'] = torch.from_numpy(pb['noise'])
    if case.sdc:
        kw['sqrt_diag_cov'] = torch.from_numpy(pb['sdc'])
    return kw


def _np(t):
    return t.detach().cpu().numpy()


def _step(eng, case, s0, inplace=False, **views):
    pb = U.problem(case)
    s1, info, samples = eng.step(s0, torch.from_numpy(pb['eps']), torch.from_numpy(pb['L']), n_steps=case.n_steps, n_thinning=1,
                                 inplace=inplace, **dict(_call_kw(case), **views))
    torch.cuda.synchronize()
    return dict(samples=_np(samples), x=_np(s1.position), u=_np(s1.momentum), g=_np(s1.logdensity_grad), logp=_np(s1.logdensity),
                info=np.stack([_np(info.logdensity), _np(info.kinetic_change), _np(info.energy_change)], axis=2))


def _check(case, got, ref, capsys):
    err = U.errors(got, ref, case)
    with capsys.disabled():
        print(f'\nUPDCASE {case.name:18s} ' + '  '.join(f'{q} {v:.1e}' for q, v in err.items()), end='')
    for q, v in err.items():
        if v > _WORST.get(q, (-1.0, None))[0]:
            _WORST[q] = (v, case.name)
    for q, v in err.items():
        assert v <= U.BOUNDS[q], (case.name, q, v, U.BOUNDS[q])


@pytest.mark.parametrize('case', [c for c in U.ORACLE_CASES if c.mode == 'step'], ids=lambda c: c.name)
def test_step_call_matches_the_oracle(case, monkeypatch, capsys):
    _setenv(monkeypatch, case)
    eng = _engine(case)
    if case.kernel == 'generic':
        S = eng.grad_launch_info(case.E)['grid'][0]
        assert U.s_class(S) == U.s_class(U.generic_S(case.N, case.E)), (S, case.name)   # the slab-splits cell the table claims
        _S_CLASSES.add(U.s_class(S))
    s0 = _init(eng, case)
    start = tuple(_np(t).copy() for t in s0)
    n0 = eng.debug_prefill_count()
    got = _step(eng, case, s0)
    assert eng.debug_prefill_count() - n0 == sum(1 for ln in U.launches(case) if ln['prefills'])
    assert all(np.array_equal(_np(t), a) for t, a in zip(s0, start))                     # a functional step
    assert np.array_equal(got['x'], got['samples'][-1])                                  # the last record launch's out_sample
    assert np.array_equal(got['logp'], got['info'][-1, :, 0])
    _check(case, got, U.simulate(case, start), capsys)


@pytest.mark.parametrize('case', [c for c in U.ORACLE_CASES if c.mode == 'tune'], ids=lambda c: c.name)
def test_tune_call_matches_the_oracle(case, monkeypatch, capsys):
    _setenv(monkeypatch, case)
    eng = _engine(case)
    assert eng.supports_device_tuner
    pb, E, d = U.problem(case), case.E, U.dim(case)
    st = _init(eng, case)
    start = tuple(_np(t).copy() for t in st)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    tuner = dict(step_size=torch.from_numpy(pb['eps'].copy()).to(DEV), step_size_max=torch.from_numpy(pb['eps_max'].copy()).to(DEV),
                 time=z(E), x_average=z(E), stream_weight=z(E), stream_average=z(E, 2, d))
    kw = _call_kw(case)
    info = eng.tune(st, tuner, torch.from_numpy(pb['L']), case.n_steps, schedule_step0=0, n_mask_steps=case.mask,
                    schedule_total=U.TUNE_TOTAL, **U.TUNE_KW, **kw)
    torch.cuda.synchronize()
    got = dict(x=_np(st.position), u=_np(st.momentum), g=_np(st.logdensity_grad), logp=_np(st.logdensity),
               info=np.stack([_np(info.logdensity), _np(info.kinetic_change), _np(info.energy_change)], axis=2),
               W=_np(tuner['stream_weight']), avg=_np(tuner['stream_average']))
    # the clamp: the predictor wants more than step_size_max on both sides, so the step size is step_size_max bit for bit
    assert np.array_equal(_np(tuner['step_size']), pb['eps_max']) and np.array_equal(_np(tuner['step_size_max']), pb['eps_max'])
    ref = U.simulate(case, start)
    assert np.array_equal(ref['eps'], pb['eps_max'].astype(np.float64))
    if case.mask == case.n_steps:
        assert not got['W'].any() and not got['avg'].any()                               # no averaging under the mask
    _check(case, got, ref, capsys)


@pytest.mark.parametrize('case', U.OFFSET_CASES, ids=lambda c: c.name)
def test_rows_off_the_16_byte_boundary_equal_the_aligned_call(case, capsys):
    """d % 4 == 0 with the state -- and the explicit noise and the preconditioner, where the case has them -- `off` floats into a
    larger buffer: AL 2 or 1 by a pointer.  Bit for bit the aligned call."""
    base = U.aligned_of(case)
    eng = _engine(case)
    s0 = _init(eng, base)
    want = _step(eng, base, s0)
    E, d = case.E, U.dim(case)

    def view(t):
        t = t.to(DEV)
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[case.off:case.off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and (v.data_ptr() // 4) % 4 == case.off
        return v
    from mile_amd.engine import IntegratorState
    s_off = IntegratorState(view(s0.position), view(s0.momentum), s0.logdensity.clone(), view(s0.logdensity_grad))
    pb, views = U.problem(case), {}
    if case.noise == 'explicit':
        views['noise'] = view(torch.from_numpy(pb['noise']))
    if case.sdc:
        views['sqrt_diag_cov'] = view(torch.from_numpy(pb['sdc']))
    got = _step(eng, case, s_off, inplace=True, **views)
    with capsys.disabled():
        print(f'\nUPDCASE {case.name:18s} ' + '  '.join(f'{k} {"equal" if np.array_equal(got[k], want[k]) else "DIFFERS"}' for k in want), end='')
    for k in want:
        assert np.array_equal(got[k], want[k]), (case.name, k, np.abs(got[k].astype(np.float64) - want[k]).max())


def test_report_worst_per_quantity(capsys):
    """Runs last: the worst normalised error per quantity with its case, and the slab-split classes that occurred."""
    with capsys.disabled():
        print()
        for q in U.QUANTITIES:
            if q in _WORST:
                print(f'UPDWORST {q:16s} {_WORST[q][0]:.2e} of a bound of {U.BOUNDS[q]:.0e}  ({_WORST[q][1]})')
        print(f'UPDWORST slab splits seen: {sorted(_S_CLASSES)}')
    if len(_WORST) == len(U.QUANTITIES):                     # the whole module ran
        assert _S_CLASSES == {'1', '2..4', '>= 5'}

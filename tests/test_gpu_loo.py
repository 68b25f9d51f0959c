"""mile_psis_loo / mile_loo_stream (Engine.psis_loo, Engine.loo_stream) against the fp64 restatement of tests/loo_ref.py
(-m gpu): the per-row kernel on crafted log-likelihoods in every regime, the streamed call bit for bit under every pass and
tile size, end to end through the forward kernels, the refusals, and evaluate.py --loo.

Bounds.  On a given fp32 tensor every output is within 1e-9 max(1, |value|) of the restatement of the same tensor, the
project's bound for "the new kernels alone" (tests/test_gpu_lppd.py), with equal NaN patterns and equal ``dropped``.  End to
end the device forward is fp32: lppd is a log-sum-exp minus a log count, 1-Lipschitz in the max norm, so it gets the measured
forward error + 1e-9.  p_waic, elpd_loo and khat are not 1-Lipschitz in l; their bound is measured from the reference
alone: the largest change of its output over four seeded perturbations of its fp64 input, each uniform within +- the case's
measured forward error, times 8 (random perturbations understate the worst case), + 1e-9 -- asserted on the rows whose
reference khat is at most 0.7 (heavier rows are held by the crafted tensors alone), which must be at least 80 % of a case's rows.

Measured on an MI355X: see DESIGN.md section 3.2p."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import lenetti_ref as RL
from tests import loo_ref as LR
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _reload, _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

KEYS = ('lppd', 'p_waic', 'elpd_loo', 'khat')
_ENGINE = {}


def _engine():
    """Any engine: psis_loo needs no handle, only the library and the device."""
    if 'e' not in _ENGINE:
        ospec = O.ModelSpec(5, (16, 16, 2), activation='relu', task='regr')
        _ENGINE['e'] = _fcn_engine(ospec, O.synthetic_problem(ospec, 64, 1, seed=3, theta_scale=0.3), 'mfma_narrow_f32')
    return _ENGINE['e']


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


# ---- a. the kernels on given tensors ---------------------------------------------------------------------------------------
def _regime(name, S, rng):
    """One row of S log-likelihoods.  exp(-l) of 'heavy<k>' is Pareto with shape k: l = -k E, E exponential."""
    if name == 'light':
        return -0.5 * (0.3 * rng.standard_normal(S) + 0.5) ** 2 - 0.9
    if name.startswith('heavy'):
        return -float(name[5:]) * rng.exponential(size=S) + 0.25
    if name == 'constant':
        return np.full(S, -1.75)
    if name == 'eight-levels':
        return -0.7 * np.floor(8.0 * rng.uniform(size=S)) - 0.1
    if name == 'nonfinite':
        l = -0.5 * (0.5 * rng.standard_normal(S) + 0.2) ** 2 - 1.1
        if S >= 20:
            l[[1, S // 2, S - 2]] = [np.nan, np.inf, -np.inf]
        return l
    raise KeyError(name)


SEVEN = ('light', 'heavy0.6', 'heavy1.5', 'heavy3', 'constant', 'eight-levels', 'nonfinite')


def _tensor(S, rows, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([_regime(r, S, rng) for r in rows], axis=1).astype(np.float32))


def _check_given(tag, ll, r_eff=1.0):
    got = _np(_engine().psis_loo(torch.from_numpy(ll), r_eff=r_eff))
    ref = LR.psis_loo(ll, r_eff)
    assert got['dropped'].dtype == np.int32 and got['dropped'].tolist() == ref['dropped'].tolist(), (tag, got['dropped'], ref['dropped'])
    worst = {}
    for k in KEYS:
        g, r = got[k], ref[k]
        assert g.dtype == np.float64 and g.shape == r.shape, (tag, k)
        assert (np.isnan(g) == np.isnan(r)).all(), (tag, k, 'NaN pattern', g, r)
        fin = ~np.isnan(r)
        rel = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        worst[k] = float(rel.max()) if fin.any() else 0.0
    print(f'{tag}: max |out - ref| / max(1, |ref|) = ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items())
          + f'; khat {np.array2string(ref["khat"], precision=2)}')
    for k in KEYS:
        assert worst[k] <= 1e-9, (tag, k, worst[k])
    return got, ref


@pytest.mark.parametrize('S', [2, 20, 21, 26, 70, 1000, 16384, 16385])
def test_every_regime_on_given_tensors(S):
    """S = 2: the smallest call; 20 / 21: M = 4 (no fit) and M = 5 (the smallest fit); 16 384 / 16 385: the row in LDS and
    streamed from the packed copy."""
    got, ref = _check_given(f'S={S}', _tensor(S, SEVEN, 100 + S))
    assert np.isnan(ref['khat'][4])                                # the constant row is never fitted
    assert abs(got['elpd_loo'][4] + 1.75) <= 1e-9 and got['p_waic'][4] == 0.0
    if S >= 20:
        assert ref['dropped'].tolist() == [0] * 6 + [3]
    if S <= 20:
        assert np.isnan(ref['khat']).all()
    if S >= 16384:                                                 # the inputs are what they are called
        k = ref['khat']
        assert k[0] < 0.5 < k[1] < 1.0 < k[2] < 2.2 < k[3], k


def test_rows_with_fewer_than_two_finite_draws():
    ll = _tensor(26, ('light', 'light', 'heavy0.6', 'light'), 7)
    ll[:, 1] = np.nan                                              # nothing kept
    ll[1:, 3] = np.inf                                             # one draw kept
    got, ref = _check_given('too few', ll)
    assert got['dropped'].tolist() == [0, 26, 0, 25]
    assert all(np.isnan(got[k][[1, 3]]).all() and np.isfinite(got[k][[0, 2]]).all() for k in KEYS)


@pytest.mark.parametrize('S', [116508, 116509, 1 << 20])
def test_the_sort_s_padding_boundary_and_the_longest_tail(S):
    """M = 1024 and 1025: a tail that fills its power of two and one that starts the next; S = 2^20: M = 3072."""
    assert LR.tail_length(S) == {116508: 1024, 116509: 1025, 1 << 20: 3072}[S]
    _check_given(f'S={S}', _tensor(S, ('light', 'heavy1.5'), S % 1000))


def test_a_tensor_beyond_the_budget_is_walked_in_tiles_of_its_own_rows():
    """S = 2^20, N = 66: the packed copy of 64 rows fills the budget, so mile_psis_loo walks the caller's tensor (ld = N) in a
    tile of 64 rows and one of 2.  A row's result depends on its own draws only: the call on all rows is, bit for bit, the
    call on each tile's columns alone."""
    S, N, tile = 1 << 20, 66, 64
    assert (256 << 20) // (S * 4) == tile < N
    ll = -torch.rand(S, N, device=DEV, generator=torch.Generator(device=DEV).manual_seed(11)).square_() - 0.5
    eng = _engine()
    whole = _np(eng.psis_loo(ll))
    assert np.isfinite(whole['elpd_loo']).all() and not whole['dropped'].any()
    parts = [_np(eng.psis_loo(ll[:, r0:r0 + tile].contiguous())) for r0 in range(0, N, tile)]
    _same_bits('two tiles', whole, {k: np.concatenate([p[k] for p in parts]) for k in KEYS + ('dropped',)})


def test_r_eff_moves_the_tail_length():
    ll = _tensor(1000, SEVEN, 9)
    assert LR.tail_length(1000, 0.2) == 200 and LR.tail_length(1000, 4.0) == 48 and LR.tail_length(1000) == 95
    a, _ = _check_given('r_eff=0.2', ll, 0.2)
    b, _ = _check_given('r_eff=4', ll, 4.0)
    assert a['khat'][1] != b['khat'][1] and a['lppd'].tobytes() == b['lppd'].tobytes()


# ---- b. and c. the streamed call --------------------------------------------------------------------------------------------
FCN = {
    # F, hidden_structure, activation, task, kernel, jitter of the draws in c.
    'narrow-regr': (5, (16, 16, 2), 'relu', 'regr', 'mfma_narrow_f32', 0.01),
    'generic-class': (7, (24, 12, 5), 'relu', 'classification', 'generic', 0.1),
}
S_FCN, N_FCN = 300, 70


@functools.lru_cache(maxsize=None)
def _fcn_case(name):
    """(ospec, training problem, draws [S, d] fp32, X, y): a base parameter vector plus Gaussian jitter, on test rows."""
    F, hs, act, task, _, jitter = FCN[name]
    ospec = O.ModelSpec(F, hs, activation=act, task=task)
    prob = O.synthetic_problem(ospec, 64, 1, seed=3, theta_scale=0.3)
    test = O.synthetic_problem(ospec, N_FCN, 1, seed=4)
    base = prob['theta0'][0].astype(np.float64)
    theta = (base[None] + jitter * np.random.default_rng(5).standard_normal((S_FCN, base.shape[0]))).astype(np.float32)
    return ospec, prob, theta, np.ascontiguousarray(test['X']), np.ascontiguousarray(test['y'])


def _lenetti_case():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    ospec = RL.LeNettiSpec(1, 1, 1, 3, activation='relu', task='classification')      # the smallest shape of tests/test_gpu_lppd.py
    prob = RL.synthetic_problem(ospec, 4, 6, seed=6)
    test = RL.synthetic_problem(ospec, 5, 1, seed=7)
    eng = Engine(LeNettiSpec(1, 1, 1, 3, activation='relu', task='classification'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    return eng, prob['theta0'], test['X'].reshape(5, -1), test['y']


def _same_bits(tag, a, b):
    for k in KEYS + ('dropped',):
        assert a[k].tobytes() == b[k].tobytes(), (tag, k, a[k], b[k])


@pytest.mark.parametrize('name', list(FCN) + ['lenetti'])
def test_stream_is_psis_loo_of_the_pointwise_tensor_for_every_pass_and_tile(name):
    if name == 'lenetti':
        eng, theta, X, y = _lenetti_case()
    else:
        ospec, prob, theta, X, y = _fcn_case(name)
        eng = _fcn_engine(ospec, prob, FCN[name][4])
    th, Xt, yt = torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y)
    alone = _np(eng.psis_loo(eng.pointwise_loglik(th, Xt, yt)))
    assert np.isfinite(alone['lppd']).all() and not alone['dropped'].any()
    for draws in (1, 7, 0):
        for rows in (32, 0):                                       # 32 at N = 70: two full tiles and a ragged one of 6
            got = _np(eng.loo_stream(th, Xt, yt, max_draws_per_pass=draws, max_rows_per_tile=rows))
            _same_bits(f'{name}: passes of {draws}, tiles of {rows}', got, alone)
    S, N = theta.shape[0], X.shape[0]
    assert eng.loo_stream_workspace(S, N) == 2 * ((S * N * 4 + 255) // 256 * 256)
    # one workspace for every streamed call of the handle: another call in between changes nothing
    eng.predict_moments(th, Xt)
    _same_bits(f'{name}: after predict_moments', _np(eng.loo_stream(th, Xt, yt)), alone)


@pytest.mark.parametrize('name', list(FCN))
def test_stream_end_to_end_against_the_fp64_forward(name):
    ospec, prob, theta, X, y = _fcn_case(name)
    eng = _fcn_engine(ospec, prob, FCN[name][4])
    out64 = O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64))
    pw64 = O.pointwise_lppd(ospec, out64[None], y)[0]                                        # [S, N]
    th, Xt, yt = torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y)
    pw_dev = eng.pointwise_loglik(th, Xt, yt).cpu().numpy().astype(np.float64)
    assert np.isfinite(pw64).all() and np.isfinite(pw_dev).all()
    err = float(np.abs(pw_dev - pw64).max())
    ref = LR.psis_loo(pw64)
    held = ref['khat'] <= 0.7                                      # (NaN: not held)
    share = float(held.mean())
    change = {k: 0.0 for k in KEYS}
    for seed in range(4):
        moved = LR.psis_loo(pw64 + np.random.default_rng(100 + seed).uniform(-err, err, pw64.shape))
        for k in KEYS:
            change[k] = max(change[k], float(np.abs(moved[k] - ref[k])[held].max()))
    bound = {k: 8.0 * change[k] + 1e-9 for k in KEYS}
    bound['lppd'] = err + 1e-9
    got = _np(eng.loo_stream(th, Xt, yt))
    dev = {k: float(np.abs(got[k] - ref[k])[held if k != 'lppd' else slice(None)].max()) for k in KEYS}
    print(f'{name}: max|pointwise_loglik - fp64| = {err:.3e}; rows with khat <= 0.7: {100 * share:.1f} %; khat from '
          f'{np.nanmin(ref["khat"]):.2f} to {np.nanmax(ref["khat"]):.2f}')
    print(f'{name}: device error | bound: ' + ', '.join(f'{k} {dev[k]:.3e} | {bound[k]:.3e}' for k in KEYS))
    assert share >= 0.8, (name, share)
    assert not got['dropped'].any() and (np.isnan(got['khat']) == np.isnan(ref['khat'])).all()
    for k in KEYS:
        assert dev[k] <= bound[k], (name, k, dev[k], bound[k])


# ---- d. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_through_the_engine():
    from mile_amd import _lib
    ospec, prob, theta, X, y = _fcn_case('narrow-regr')
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt, yt = torch.from_numpy(theta).to(DEV), torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    ll = eng.pointwise_loglik(th, Xt, yt)
    for tag, fn in [('S = 1, psis_loo', lambda: eng.psis_loo(ll[:1])), ('S = 1, loo_stream', lambda: eng.loo_stream(th[:1], Xt, yt)),
                    ('r_eff = 0, psis_loo', lambda: eng.psis_loo(ll, r_eff=0.0)),
                    ('r_eff = 0, loo_stream', lambda: eng.loo_stream(th, Xt, yt, r_eff=0.0)),
                    ('r_eff NaN', lambda: eng.loo_stream(th, Xt, yt, r_eff=float('nan')))]:
        with pytest.raises(_lib.MileHipError, match='libmile_hip error -1') as exc:
            fn()
        print(tag, '->', exc.value)
    p = lambda t: C.c_void_p(t.data_ptr())
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_psis_loo: no output'):
        _lib.check(eng.lib.mile_psis_loo(p(ll), S_FCN, N_FCN, 1.0, None, None, None, None, None, None), eng.lib)
    with pytest.raises(_lib.MileHipError, match='libmile_hip error -1: mile_loo_stream: no output'):
        _lib.check(eng.lib.mile_loo_stream(eng._h, p(th), S_FCN, p(Xt), p(yt), N_FCN, 1.0, None, None, None, None, None, 0, 0, None), eng.lib)
    assert eng.loo_stream_workspace(1, 70) == -1
    # one output alone is a call like any other, and the handle is as usable as before
    only = torch.full((N_FCN,), 7.0, dtype=torch.float64, device=DEV)
    _lib.check(eng.lib.mile_loo_stream(eng._h, p(th), S_FCN, p(Xt), p(yt), N_FCN, 1.0, None, None, None, p(only), None, 0, 0, None), eng.lib)
    full = eng.loo_stream(th, Xt, yt)
    assert only.cpu().numpy().tobytes() == full['khat'].cpu().numpy().tobytes()


# ---- e. evaluate.py --loo ---------------------------------------------------------------------------------------------------
def test_evaluate_cli_loo(tmp_path):
    import yaml
    from mile_amd import metrics as M
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=120, n_chains=4)      # thinning 10: 12 draws kept per chain
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp])
    plain = json.loads((exp / 'metrics.json').read_text())
    assert not (exp / 'loo.npz').exists() and not any(k.startswith('loo_') for k in plain)
    _run([ROOT / 'evaluate.py', '-e', exp, '--loo'])                                   # --split stays 'test': LOO takes the train rows
    m = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m.items() if not k.startswith('loo_')} == plain
    eng, samples, x, y = _reload(exp, 'train')
    N = x.shape[0]
    z = np.load(exp / 'loo.npz')
    assert sorted(z.files) == ['dropped', 'elpd_loo', 'khat', 'lppd', 'p_waic'] and all(z[k].shape == (N,) for k in z.files)
    assert N != plain['n_points'] and m['loo_n_points'] == N and m['split'] == 'test'
    summary = M.loo_summary({k: z[k] for k in KEYS})
    assert sorted(k for k in m if k.startswith('loo_')) == sorted(['loo_' + k for k in summary] + ['loo_n_points', 'loo_dropped'])
    assert all(m['loo_' + k] == v or (v != v and m['loo_' + k] != m['loo_' + k]) for k, v in summary.items())
    assert m['loo_dropped'] == 0 and m['loo_elpd_loo'] <= m['loo_lppd_sum'] and m['loo_p_loo'] >= 0.0
    stream = eng.lppd_stream(torch.from_numpy(samples), torch.from_numpy(x), torch.from_numpy(y), curve_points=[])
    lppd = float(stream['lppd'])
    print(f"cli: loo_lppd_sum / N = {m['loo_lppd_sum'] / N!r}, lppd_stream = {lppd!r}; elpd_loo {m['loo_elpd_loo']:.3f}, "
          f"p_loo {m['loo_p_loo']:.3f}, khat > 0.7 on {m['loo_n_khat_above_0.7']} rows of {N}")
    assert abs(m['loo_lppd_sum'] / N - lppd) <= 1e-9 * max(1.0, abs(lppd))            # the same fp32 forward: the reductions alone

"""mile_lppd_stream / Engine.lppd_stream against tests/lppd_ref.py fed with the fp64 forward's pointwise log-likelihoods (-m gpu):
every pass size bit for bit, full and sparse curve grids, underflow, the NaN rule, the refusals, LeNetti and evaluate.py --running.

Bound.  The device forward is fp32, the reduction fp64, and every output is a mean of log-sum-exps minus logs of counts: a
log-sum-exp is 1-Lipschitz in the max norm, so no output can be further from the restatement than the largest error of a
pointwise log-likelihood.  That error is measured per case (Engine.pointwise_loglik against the fp64 values, the quantity
tests/test_gpu_predict.py bounds) and each output gets it + 1e-9.  Fed the device's own pointwise tensor, the restatement must
agree to 1e-9 absolute: the new kernels alone."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import lenetti_ref as RL
from tests.lppd_ref import ref_lppd_stream
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _reload, _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

KEYS = ('run_chain', 'run_ens', 'chain_lppd', 'row_lppd', 'lppd')
CASES = {
    # F, hidden_structure, activation, task, kernel, C, S, N, scale of the draws
    'narrow-regr': (5, (16, 16, 2), 'relu', 'regr', 'mfma_narrow_f32', 3, 7, 70, 0.3),     # N no multiple of 64, S prime
    'tanh-class': (7, (40, 40, 3), 'tanh', 'classification', 'mfma_narrow_f32', 4, 12, 130, 0.3),
    'w64-b2': (5, (64, 64, 64, 2), 'relu', 'regr', 'mfma_w64_bf16x3', 2, 5, 301, 0.1),     # the B2 forward kernel
    'one': (5, (16, 16, 2), 'relu', 'regr', 'mfma_narrow_f32', 1, 1, 1, 0.3),
}
# small weights, sigma near 1: a target moved to 40 puts every draw of every chain between -1400 and -500 on that row
SMALL = {'narrow-small': (5, (16, 16, 2), 'relu', 'regr', 'mfma_narrow_f32', 3, 7, 70, 0.1)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(ospec, training problem, theta [C, S, d], X, y, fp64 pointwise [C, S, N]) of a case, computed once."""
    F, hs, act, task, kernel, C_, S, N, scale = {**CASES, **SMALL}[name]
    ospec = O.ModelSpec(F, hs, activation=act, task=task)
    prob = O.synthetic_problem(ospec, 64, C_ * S, seed=3, theta_scale=scale)
    test = O.synthetic_problem(ospec, max(N, 8), 1, seed=4)      # (the targets are z-scored: not from one row)
    X, y = np.ascontiguousarray(test['X'][:N]), np.ascontiguousarray(test['y'][:N])
    theta = prob['theta0'].reshape(C_, S, -1)
    return ospec, prob, theta, X, y, _pw64(ospec, theta, X, y)


def _pw64(ospec, theta, X, y):
    C_, S, d = theta.shape
    out = O.mlp_forward(ospec, theta.reshape(C_ * S, d).astype(np.float64), X.astype(np.float64))
    with np.errstate(invalid='ignore'):
        return O.pointwise_lppd(ospec, out.reshape(C_, S, X.shape[0], -1), y)


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _stream(eng, theta, X, y, pts, mdp=0):
    return _np(eng.lppd_stream(torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y), curve_points=pts, max_draws_per_pass=mdp))


def _forward_error(eng, theta, X, y, pw64):
    """(device pointwise tensor [C, S, N] as fp64, its largest error against the fp64 values over the entries finite in both)."""
    pw = eng.pointwise_loglik(torch.from_numpy(theta), torch.from_numpy(X), torch.from_numpy(y)).cpu().numpy().astype(np.float64)
    fin = np.isfinite(pw) & np.isfinite(pw64)
    assert (np.isnan(pw) == np.isnan(pw64)).all() and fin.any()
    return pw, float(np.abs(pw[fin] - pw64[fin]).max())


def _assert_within(tag, got, ref, bound):
    worst = 0.0
    for k in KEYS:
        g, r = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        assert g.shape == r.shape, (tag, k, g.shape, r.shape)
        assert (np.isnan(g) == np.isnan(r)).all(), (tag, k, 'NaN pattern')
        fin = ~np.isnan(r)
        err = float(np.abs(g[fin] - r[fin]).max()) if fin.any() else 0.0
        worst = max(worst, err)
        assert err <= bound, (tag, k, err, bound)
    print(f'{tag}: max|out - ref| over the outputs = {worst:.3e}, bound {bound:.3e}')
    assert (got['dropped'] == ref['dropped']).all(), (tag, got['dropped'], ref['dropped'])


def _assert_same_bits(tag, a, b):
    for k in KEYS + ('dropped',):
        assert a[k].tobytes() == b[k].tobytes(), (tag, k, a[k], b[k])


@pytest.mark.parametrize('name', list(CASES))
def test_outputs_match_fp64_and_do_not_depend_on_the_pass_size(name):
    ospec, prob, theta, X, y, pw64 = _case(name)
    C_, S, N = pw64.shape
    eng = _fcn_engine(ospec, prob, CASES[name][4])
    full = list(range(1, S + 1))
    got = {mdp: _stream(eng, theta, X, y, full, mdp) for mdp in (1, 2, 3, 0)}     # 2 and 3: a ragged last pass at S = 7 and 5
    for mdp in (1, 2, 3):
        _assert_same_bits(f'{name}: passes of {mdp} vs the library\'s choice', got[mdp], got[0])
    assert got[0]['curve_points'].tolist() == full and got[0]['run_chain'].dtype == np.float64
    assert got[0]['run_ens'][-1] == got[0]['lppd'] and got[0]['dropped'].dtype == np.int64
    pw_dev, err = _forward_error(eng, theta, X, y, pw64)
    print(f'{name}: max|pointwise_loglik - fp64| = {err:.3e}, max|fp64| = {np.abs(pw64).max():.3e}')
    _assert_within(f'{name} vs the fp64 forward', got[0], ref_lppd_stream(pw64, full), err + 1e-9)
    _assert_within(f'{name} vs the restatement of the device tensor', got[0], ref_lppd_stream(pw_dev, full), 1e-9)
    # a sparse grid: points inside passes and on pass boundaries give the full grid's values at those points
    sparse = sorted({1, min(4, S), S})
    for mdp in (2, 0):
        sp = _stream(eng, theta, X, y, sparse, mdp)
        assert sp['curve_points'].tolist() == sparse
        for k in ('run_chain', 'run_ens'):
            assert sp[k].tobytes() == got[0][k][[p - 1 for p in sparse]].tobytes(), (name, mdp, k)
        for k in ('chain_lppd', 'row_lppd', 'lppd', 'dropped'):
            assert sp[k].tobytes() == got[0][k].tobytes(), (name, mdp, k)
    # a grid that stops before S, and no grid at all: the final figures are the same
    for pts in ([1], []):
        part = _stream(eng, theta, X, y, pts, 2)
        assert part['run_ens'].shape == (len(pts),)
        for k in ('chain_lppd', 'row_lppd', 'lppd', 'dropped'):
            assert part[k].tobytes() == got[0][k].tobytes(), (name, pts, k)
    assert eng.lppd_stream_workspace(C_, N) >= C_ * N * 20


def test_underflow_stays_finite():
    """Targets moved far off on every fifth row: l < -150 there for every draw of every chain, so exp(l) is 0 in fp32."""
    from mile_amd import metrics as M
    ospec, prob, theta, X, y, _ = _case('narrow-small')
    y = y.copy()
    y[::5] = 40.0
    pw64 = _pw64(ospec, theta, X, y)
    assert (pw64[:, :, ::5] < -150.0).all() and pw64.min() > -1e4
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    S = theta.shape[1]
    full = list(range(1, S + 1))
    got = _stream(eng, theta, X, y, full, 3)
    assert all(np.isfinite(got[k]).all() for k in KEYS)
    pw_dev, err = _forward_error(eng, theta, X, y, pw64)
    print(f'underflow: max|pointwise_loglik - fp64| = {err:.3e}, max|fp64| = {np.abs(pw64).max():.3e}')
    _assert_within('underflow vs the fp64 forward', got, ref_lppd_stream(pw64, full), err + 1e-9)
    _assert_within('underflow vs the restatement of the device tensor', got, ref_lppd_stream(pw_dev, full), 1e-9)
    literal = M.running_lppd(torch.from_numpy(pw_dev.astype(np.float32)))
    assert torch.isneginf(literal).any()                         # what the literal form gives: documented, not a failure of it


def test_one_chain_far_below_the_others():
    """Chain 1 predicts 50 off on every row: all its draws are below -500 while the other chains stay near 0, so the log-sum-exp
    over chains spans more than 700 on every row -- exp of the difference is 0 in fp64, and the ensemble must not notice."""
    from mile_amd import metrics as M
    ospec, prob, theta, X, y, _ = _case('narrow-small')
    theta = theta.copy()
    theta[1, :, O.param_slices(ospec)[-1]['bias'][0]] += 50.0
    pw64 = _pw64(ospec, theta, X, y)
    assert (pw64[1] < -150.0).all() and (pw64[[0, 2]].max(axis=(0, 1)) - pw64[1].max(axis=0) > 700.0).any() and pw64.min() > -1e4
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    full = list(range(1, theta.shape[1] + 1))
    got = _stream(eng, theta, X, y, full, 2)
    assert all(np.isfinite(got[k]).all() for k in KEYS) and got['chain_lppd'][1] < -150.0
    pw_dev, err = _forward_error(eng, theta, X, y, pw64)
    print(f'one chain far below: max|pointwise_loglik - fp64| = {err:.3e}, max|fp64| = {np.abs(pw64).max():.3e}')
    _assert_within('one chain far below vs the fp64 forward', got, ref_lppd_stream(pw64, full), err + 1e-9)
    _assert_within('one chain far below vs the restatement of the device tensor', got, ref_lppd_stream(pw_dev, full), 1e-9)
    assert torch.isneginf(M.running_lppd(torch.from_numpy(pw_dev.astype(np.float32)))).all()      # the literal form: one -inf chain


def test_nan_draws_are_left_out_and_counted():
    ospec, prob, theta, X, y, pw64 = _case('narrow-regr')
    C_, S, N = pw64.shape
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    full = list(range(1, S + 1))
    clean = _stream(eng, theta, X, y, full, 3)
    bias = O.param_slices(ospec)[-1]['bias'][0]                  # the output layer's bias of mu: no activation can absorb it
    th = theta.copy()
    th[1, 2, bias] = np.nan
    got = {mdp: _stream(eng, th, X, y, full, mdp) for mdp in (3, 0)}
    _assert_same_bits('one NaN draw: passes of 3 vs the library\'s choice', got[3], got[0])
    assert got[0]['dropped'].tolist() == [0, N, 0]
    pw_nan = pw64.copy()
    pw_nan[1, 2] = np.nan
    pw_dev, err = _forward_error(eng, th, X, y, pw_nan)
    assert np.isnan(pw_dev[1, 2]).all()
    _assert_within('one NaN draw vs the fp64 forward without it', got[0], ref_lppd_stream(pw_nan, full), err + 1e-9)
    _assert_within('one NaN draw vs the restatement of the device tensor', got[0], ref_lppd_stream(pw_dev, full), 1e-9)
    assert all(np.isfinite(got[0][k]).all() for k in KEYS)
    for c in (0, 2):                                             # the other chains are untouched
        assert got[0]['chain_lppd'][c] == clean['chain_lppd'][c]
    assert got[0]['run_chain'][:2].tobytes() == clean['run_chain'][:2].tobytes()      # and so is everything before the draw
    assert got[0]['run_ens'][:2].tobytes() == clean['run_ens'][:2].tobytes()
    # every draw of chain 1: its own figures are NaN, the ensemble goes on without it
    th[1, :, bias] = np.nan
    dead = _stream(eng, th, X, y, full, 2)
    assert dead['dropped'].tolist() == [0, S * N, 0]
    assert np.isnan(dead['chain_lppd'][1]) and np.isfinite(dead['chain_lppd'][[0, 2]]).all() and np.isnan(dead['run_chain']).all()
    assert np.isfinite(dead['run_ens']).all() and np.isfinite(dead['row_lppd']).all() and np.isfinite(dead['lppd'])
    pw_nan[1] = np.nan
    _assert_within('a dead chain vs the fp64 forward', dead, ref_lppd_stream(pw_nan, full), err + 1e-9)
    two = _stream(eng, np.ascontiguousarray(th[[0, 2]]), X, y, full, 2)
    assert two['run_ens'].tobytes() == dead['run_ens'].tobytes() and two['row_lppd'].tobytes() == dead['row_lppd'].tobytes()


def test_refusals_leave_the_handle_usable():
    ospec, prob, theta, X, y, _ = _case('narrow-regr')
    C_, S, N = theta.shape[0], theta.shape[1], X.shape[0]
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt, yt = torch.from_numpy(theta).to(DEV), torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    pts = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    rc_, re_ = torch.full((8,), 7.0, dtype=torch.float64, device=DEV), torch.full((8,), 7.0, dtype=torch.float64, device=DEV)
    lp = torch.full((1,), 7.0, dtype=torch.float64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(theta_=p(th), points=None, K=0, run_chain=None, run_ens=None, mdp=0):
        return eng.lib.mile_lppd_stream(eng._h, theta_, C_, S, p(Xt), p(yt), N, None if points is None else p(points), K,
                                        run_chain, run_ens, None, None, p(lp), None, mdp, None)

    good, back, high = pts([1, 4, S]), pts([1, 4, 4]), pts([1, 4, S + 1])
    for tag, kw, text in [('non-increasing points', dict(points=back, K=3, run_chain=p(rc_)), 'strictly increasing'),
                          ('a point above S', dict(points=high, K=3, run_ens=p(re_)), 'outside [1, S]'),
                          ('a point below 1', dict(points=pts([0, 4, S]), K=3, run_ens=p(re_)), 'outside [1, S]'),
                          ('K = 0 with a curve output', dict(K=0, run_chain=p(rc_)), 'K = 0'),
                          ('null theta', dict(theta_=None, points=good, K=3, run_chain=p(rc_)), 'null'),
                          ('negative pass size', dict(points=good, K=3, run_chain=p(rc_), mdp=-1), 'max_draws_per_pass')]:
        rc = call(**kw)
        msg = eng.lib.mile_last_error().decode()
        print(tag, rc, msg)
        assert rc == -1 and 'mile_lppd_stream' in msg and text in msg, (tag, rc, msg)
    torch.cuda.synchronize()
    assert (rc_ == 7.0).all() and (re_ == 7.0).all() and (lp == 7.0).all()         # nothing was launched
    assert eng.lib.mile_lppd_stream_workspace(eng._h, 0, N) == -1
    assert call(points=good, K=3, run_chain=p(rc_), run_ens=p(re_)) == 0
    after = _stream(eng, theta, X, y, [1, 4, S])
    torch.cuda.synchronize()
    assert rc_[:3].cpu().numpy().tobytes() == after['run_chain'].tobytes() and float(lp) == float(after['lppd'])
    with pytest.raises(ValueError):
        eng.lppd_stream(th[0], Xt, yt)                           # samples must be [C, S, d]


def test_lenetti_goes_through_the_same_call():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    ospec = RL.LeNettiSpec(1, 1, 1, 3, activation='relu', task='classification')      # the smallest shape of tests/test_gpu_lenetti.py
    C_, S, N = 2, 3, 5
    prob = RL.synthetic_problem(ospec, 4, C_ * S, seed=6)
    test = RL.synthetic_problem(ospec, N, 1, seed=7)
    eng = Engine(LeNettiSpec(1, 1, 1, 3, activation='relu', task='classification'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    theta = prob['theta0'].reshape(C_, S, -1)
    out = RL.forward(ospec, prob['theta0'].astype(np.float64), test['X'])
    pw64 = O.pointwise_loglik_raw(ospec, out, test['y'])[0].reshape(C_, S, N)
    Xf = test['X'].reshape(N, -1)
    got = _stream(eng, theta, Xf, test['y'], [1, 2, 3], 2)
    pw_dev, err = _forward_error(eng, theta, Xf, test['y'], pw64)
    print(f'lenetti: max|pointwise_loglik - fp64| = {err:.3e}')
    _assert_within('lenetti vs the fp64 restatement', got, ref_lppd_stream(pw64, [1, 2, 3]), err + 1e-9)
    _assert_within('lenetti vs the restatement of the device tensor', got, ref_lppd_stream(pw_dev, [1, 2, 3]), 1e-9)


def test_evaluate_cli_running(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=120, n_chains=4)      # thinning 10: 12 draws kept per chain
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--running', 8])
    m = json.loads((exp / 'metrics.json').read_text())
    z = np.load(exp / 'running_lppd.npz')
    assert sorted(z.files) == ['chain_lppd', 'curve_points', 'dropped', 'row_lppd', 'run_chain', 'run_ens']
    assert z['curve_points'].shape == z['run_chain'].shape == z['run_ens'].shape == (8,) and m['running_points'] == 8
    assert z['curve_points'][0] == 1 and z['curve_points'][-1] == m['n_samples'] == 12
    assert z['chain_lppd'].shape == z['dropped'].shape == (4,) and z['row_lppd'].shape == (m['n_points'],)
    assert float(z['run_ens'][-1]) == m['running_lppd'] == m['running_ens_last'] and not z['dropped'].any()
    assert m['running_per_chain_lppd'] == [float(v) for v in z['chain_lppd']] and m['running_chain_first'] == float(z['run_chain'][0])
    # against the plain keys of the same run: the same draws through the fp32 tensor
    eng, samples, x, y = _reload(exp, 'test')
    ospec = O.ModelSpec(x.shape[1], tuple(cfg['model']['hidden_structure']), activation=cfg['model']['activation'], task='regr')
    _, err = _forward_error(eng, samples, x, y, _pw64(ospec, samples, x, y))
    print(f"cli: running_lppd = {m['running_lppd']!r}, lppd = {m['lppd']!r}, difference {abs(m['running_lppd'] - m['lppd']):.3e}, "
          f'max|pointwise_loglik - fp64| = {err:.3e}')
    assert abs(m['running_lppd'] - m['lppd']) <= err
    # without the flag nothing of it is written
    (exp / 'running_lppd.npz').unlink()
    _run([ROOT / 'evaluate.py', '-e', exp])
    assert not (exp / 'running_lppd.npz').exists()
    assert not any(k.startswith('running_') and k != 'running_lppd_last' for k in json.loads((exp / 'metrics.json').read_text()))

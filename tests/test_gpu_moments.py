"""mile_predict_moments / Engine.predict_moments against the fp64 forwards of tests/test_gpu_predict.py reduced in fp64 NumPy
(-m gpu): every pass size, the Chan merge, cancellation, the non-finite rule, S = 1, the refusals and the predict.py CLI.

Bounds.  Means and probabilities: test_gpu_predict.py's bound on the raw outputs, max|out - ref| < 1e-4 * max(1, max|ref|)
(a mean of outputs is no worse than its terms).  Variances, entropy and mutual information: the error of the float32
restatement (metrics.predictive_moments on the float32 oracle forward) against fp64 is measured per case and column, and the
device gets 4x that, plus 1e-7 absolute for the two columns that are differences (epistemic variance, mutual information).
A case whose restatement error is above 1e-3 of the column's largest value has badly chosen inputs and fails as such."""
import ctypes as C

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import attn_ref as RA
from tests import lenetti_ref as RL
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _run
from tests.test_moments_host import ref_moments

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _check(tag, got, out64, out32, task):
    """got [N, W] (device) against ref_moments(out64); out32: the same forward in float32, for the restatement's error."""
    from mile_amd import metrics as M
    got = got.cpu().numpy().astype(np.float64)
    ref = ref_moments(out64, task)
    rest = M.predictive_moments(torch.from_numpy(np.ascontiguousarray(out32, dtype=np.float32)), task).numpy().astype(np.float64)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    n_mean = 1 if task == 'regr' else ref.shape[1] - 2
    names = ['mean', 'epistemic_var', 'aleatoric_var'] if task == 'regr' else ['probs', 'entropy', 'mutual_information']
    err = np.abs(got[:, :n_mean] - ref[:, :n_mean]).max()
    bound = 1e-4 * max(1.0, np.abs(ref[:, :n_mean]).max())
    print(f'{tag} {names[0]}: max|out - ref| = {err:.3e}, bound {bound:.3e}')
    assert err < bound, (tag, names[0], err, bound)
    for i, name in enumerate(names[1:]):
        c = n_mean + i
        e32 = np.abs(rest[:, c] - ref[:, c]).max()
        err = np.abs(got[:, c] - ref[:, c]).max()
        bound = 4.0 * e32 + (1e-7 if name in ('epistemic_var', 'mutual_information') else 0.0)
        print(f'{tag} {name}: max|out - ref| = {err:.3e}, float32 restatement {e32:.3e}, bound {bound:.3e}, max|ref| = {np.abs(ref[:, c]).max():.3e}')
        assert e32 <= 1e-3 * np.abs(ref[:, c]).max(), (tag, name, 'badly chosen inputs', e32)
        assert err <= bound, (tag, name, err, bound)


def _agree(tag, a, b, rel=1e-6):
    a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    d = np.abs(a - b).max(axis=0)
    print(f'{tag}: max|a - b| per column = {d}')
    assert (np.abs(a - b) <= rel * np.abs(b)).all(), (tag, d)


def _fcn_problem(F, hs, act, task, N, S):
    ospec = O.ModelSpec(F, hs, activation=act, task=task)
    prob = O.synthetic_problem(ospec, 64, S, seed=3, theta_scale=0.3)
    X = O.synthetic_problem(ospec, N, 1, seed=4)['X']
    return ospec, prob, X


@pytest.mark.parametrize('kernel,hs', [('mfma_narrow_f32', (16, 16, 2)), ('mfma_w64', (64, 64, 64, 2))])
def test_fcn_regression_every_pass_size(kernel, hs):
    ospec, prob, X = _fcn_problem(5, hs, 'relu', 'regr', 70, 7)
    eng = _fcn_engine(ospec, prob, kernel)
    th, Xt = torch.from_numpy(prob['theta0']), torch.from_numpy(X)
    out64 = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), X.astype(np.float64))
    out32 = O.mlp_forward(ospec, prob['theta0'], X)
    got = {}
    for k in (0, 3, 7):                                            # 3: a ragged last pass, merged by Chan's formula
        got[k], dropped = eng.predict_moments(th, Xt, max_draws_per_pass=k, return_dropped=True)
        assert got[k].shape == (70, 3) and dropped.dtype == torch.int32 and not dropped.any()
        _check(f'{kernel} passes of {k}', got[k], out64, out32, 'regr')
    _agree('passes of 3 vs one pass', got[3], got[0])
    _agree('passes of 7 vs one pass', got[7], got[0])


@pytest.mark.parametrize('F,hs,act', [(7, (40, 40, 3), 'tanh'), (11, (32, 7), 'sigmoid')])
def test_fcn_classification(F, hs, act):
    ospec, prob, X = _fcn_problem(F, hs, act, 'classification', 130, 5)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    got = eng.predict_moments(torch.from_numpy(prob['theta0']), torch.from_numpy(X), max_draws_per_pass=2)
    assert got.shape == (130, hs[-1] + 2)
    _check(f'classification {hs}', got, O.mlp_forward(ospec, prob['theta0'].astype(np.float64), X.astype(np.float64)),
           O.mlp_forward(ospec, prob['theta0'], X), 'classification')
    _agree('passes of 2 vs one pass', got, eng.predict_moments(torch.from_numpy(prob['theta0']), torch.from_numpy(X)))


def test_lenetti():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    ospec = RL.LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr')
    prob = RL.synthetic_problem(ospec, 20, 5, seed=6)
    X = RL.synthetic_problem(ospec, 70, 1, seed=7)['X']
    eng = Engine(LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    got = eng.predict_moments(torch.from_numpy(prob['theta0']), torch.from_numpy(X), max_draws_per_pass=2)
    _check('lenetti', got, RL.forward(ospec, prob['theta0'].astype(np.float64), X), RL.forward(ospec, prob['theta0'], X), 'regr')


def test_attention_classifier():
    from mile_amd.engine import Engine
    from mile_amd.spec import AttentionSpec
    spec = AttentionSpec(100, 30, 16, 4, 16, n_classes=3, projection_dim=(8,), use_bias=True, prior='Normal', prior_scale=0.2)
    prob = RA.synthetic_problem(spec, 20, 5, seed=6)
    test = RA.synthetic_problem(spec, 70, 1, seed=7)
    eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'attn_f32'
    got = eng.predict_moments(torch.from_numpy(prob['theta0']), torch.from_numpy(test['X']), max_draws_per_pass=2)
    out64 = np.stack([RA._forward(spec, RA.unpack(spec, t), test['x'])['logits'] for t in prob['theta0']])
    out32 = np.stack([RA._forward(spec, RA.unpack(spec, t, dtype=np.float32), test['x'])['logits'] for t in prob['theta0']])
    _check('attn', got, out64, out32, 'classification')


def test_cancellation_on_the_device():
    """2048 draws that differ only in the output layer's mu-bias, 10 + 1e-3 z: Var(mu) = 1e-6 next to mu^2 = 100.  A sum of
    squares in fp32 keeps nothing of it; Welford and Chan do."""
    ospec = O.ModelSpec(5, (16, 16, 2))
    S, N = 2048, 70
    prob = O.synthetic_problem(ospec, 64, 1, seed=3, theta_scale=0.3)
    X = O.synthetic_problem(ospec, N, 1, seed=4)['X']
    theta = np.repeat(prob['theta0'], S, axis=0)
    theta[:, O.param_slices(ospec)[-1]['bias'][0]] = (10.0 + 1e-3 * np.random.default_rng(0).standard_normal(S)).astype(np.float32)
    ref = ref_moments(O.mlp_forward(ospec, theta.astype(np.float64), X.astype(np.float64)), 'regr')
    assert np.abs(ref[:, 0]).max() > 9.0
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    for k in (0, 300):
        got = eng.predict_moments(torch.from_numpy(theta), torch.from_numpy(X), max_draws_per_pass=k).cpu().numpy().astype(np.float64)
        rows = ref[:, 1] > 1e-8
        rel = np.abs(got[rows, 1] - ref[rows, 1]) / ref[rows, 1]
        print(f'passes of {k}: {rows.sum()} rows, max relative error of the epistemic variance = {rel.max():.3e}, bound 1e-2')
        assert rows.any() and (rel < 1e-2).all()


def test_nonfinite_draw_is_left_out_per_row():
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 7)
    theta = prob['theta0'].copy()
    theta[2, O.param_slices(ospec)[-1]['bias'][0]] = np.inf        # mu = inf on every row of draw 2
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    Xt = torch.from_numpy(X)
    got, dropped = eng.predict_moments(torch.from_numpy(theta), Xt, max_draws_per_pass=3, return_dropped=True)
    assert (dropped == 1).all()
    rest = prob['theta0'][[0, 1, 3, 4, 5, 6]]
    assert torch.isfinite(got).all()
    _agree('without the draw', got, eng.predict_moments(torch.from_numpy(rest), Xt))
    _check('six finite draws', got, O.mlp_forward(ospec, rest.astype(np.float64), X.astype(np.float64)), O.mlp_forward(ospec, rest, X), 'regr')


def test_one_draw_has_no_spread():
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 1)
    got = _fcn_engine(ospec, prob, 'mfma_narrow_f32').predict_moments(torch.from_numpy(prob['theta0']), torch.from_numpy(X))
    assert (got[:, 1] == 0).all() and torch.isfinite(got).all()
    ospec, prob, X = _fcn_problem(7, (40, 40, 3), 'tanh', 'classification', 130, 1)
    got = _fcn_engine(ospec, prob, 'mfma_narrow_f32').predict_moments(torch.from_numpy(prob['theta0']), torch.from_numpy(X))
    assert (got[:, 4] == 0).all() and torch.isfinite(got).all() and (got[:, 3] > 0).all()


def test_refusals_leave_the_handle_usable():
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 3)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt = torch.from_numpy(prob['theta0']).to(DEV), torch.from_numpy(X).to(DEV)
    out = torch.empty((70, 3), dtype=torch.float32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda th_, S, X_, N, out_: eng.lib.mile_predict_moments(eng._h, th_, S, X_, N, out_, None, 0, None)
    assert eng.lib.mile_predict_moments_width(eng._h) == 3
    for tag, args in [('null out', (p(th), 3, p(Xt), 70, None)), ('S = 0', (p(th), 0, p(Xt), 70, p(out))),
                      ('no data', (p(th), 3, None, 70, p(out))), ('N = 0', (p(th), 3, p(Xt), 0, p(out)))]:
        rc = call(*args)
        msg = eng.lib.mile_last_error().decode()
        print(tag, rc, msg)
        assert rc in (-1, -2) and 'mile_predict_moments' in msg, (tag, rc, msg)
    got = eng.predict_moments(th, Xt)
    _agree('after the refusals', got, eng.predict_moments(th, Xt, max_draws_per_pass=1))
    assert torch.isfinite(got).all()


def test_predict_cli(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    norm = np.load(exp / 'normalization.npz')
    F = norm['x_mean'].shape[0]
    assert norm['x_std'].shape == (F,) and norm['y_mean'].shape == norm['y_std'].shape == (1,)
    # a 20-row table in the units of the raw data
    table = (np.random.default_rng(0).standard_normal((20, F)) * norm['x_std'] + norm['x_mean']).astype(np.float32)
    np.savetxt(tmp_path / 'new.csv', table, delimiter=',')
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'new.csv', '-o', tmp_path / 'pred.npz', '--draws-per-pass', 50])
    pred = np.load(tmp_path / 'pred.npz')
    assert sorted(pred.files) == ['aleatoric_var', 'dropped', 'epistemic_var', 'mean']
    assert all(pred[k].shape == (20,) for k in pred.files) and all(np.isfinite(pred[k]).all() for k in pred.files)
    assert (pred['epistemic_var'] >= 0).all() and (pred['aleatoric_var'] > 0).all() and not pred['dropped'].any()
    # the experiment's own test rows: evaluate.py --moments and predict.py reduce the same draws on the same rows
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--moments'])
    mom = np.load(exp / 'moments.npz')
    from mile_amd.config import Config
    from mile_amd.trainer import BDETrainer
    tr = BDETrainer.__new__(BDETrainer)
    tr.build_model(Config.from_file(exp / 'config.yaml').replace(logging=False))
    np.save(tmp_path / 'test_x.npy', np.ascontiguousarray(tr.loader.test_x))
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'test_x.npy', '--normalized'])
    same = np.load(exp / 'predictions.npz')
    for k in ('mean', 'epistemic_var', 'aleatoric_var', 'dropped'):
        assert same[k].shape == mom[k].shape == (len(tr.loader.test_x),)
        np.testing.assert_allclose(same[k], mom[k], rtol=1e-6, atol=0)
    # and through the recorded statistics: raw units in, target units out
    raw = (np.ascontiguousarray(tr.loader.test_x) * norm['x_std'] + norm['x_mean']).astype(np.float32)
    np.save(tmp_path / 'raw_x.npy', raw)
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'raw_x.npy', '-o', tmp_path / 'raw.npz'])
    back = np.load(tmp_path / 'raw.npz')
    ys, ym = float(norm['y_std'][0]), float(norm['y_mean'][0])
    scale = max(1.0, np.abs(mom['mean']).max())
    assert np.abs((back['mean'] - ym) / ys - mom['mean']).max() < 1e-4 * scale      # (the inputs went through x * std + mean and back)
    np.testing.assert_allclose(back['aleatoric_var'], mom['aleatoric_var'] * ys * ys, rtol=1e-4)

"""mile_mixture_quantiles / mile_predict_quantiles (Engine.mixture_quantiles, Engine.predict_quantiles) against the fp64
reference of tests/quantile_ref.py (-m gpu): the solver on crafted outputs, end to end through the forward kernels, every
tiling bit for bit, the consistency of PIT and quantiles, and the two command-line tools.

Bounds.  Solver on given fp32 outputs: each quantile within 2^-22 max(|q*|, sd_n) of the reference (fp32 rounding of the
output, 2^-24, with a factor 4 for the stopping rule) OR |F_ref(q) - p| <= 1e-12 (fp64 rounding of a sum of up to 4e4 terms:
flat stretches of F, where the root is ill-conditioned); PIT within 2^-22.  End to end: test_gpu_predict.py's bound on the raw
outputs, max|q - q*| < 1e-4 max(1, max|q*|), PIT within 1e-4 absolute; the float32 restatement's error (the reference on the
float32 oracle forward) is measured and printed beside the device's, and a case where it exceeds 1e-3 sd_n has badly chosen
inputs and fails as such.

Measured on an MI355X (device | float32 restatement, max over rows and levels of |q - q*| / sd_n, and max |pit - pit*|):
narrow 1.0e-7 | 3.7e-8 and 3.0e-8; w64 (log sigma -26.4 .. 23.6) 1.3e-7 | 6.3e-8 and 2.9e-8; LeNetti 2.9e-7 | 2.4e-7 and
4.3e-8 (DESIGN.md section 3.2o has the table).

Partition mode: tests/test_gpu_moments.py has no case with set_partition, so there is none here either."""
import json

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import lenetti_ref as RL
from tests import quantile_ref as QR
from tests.test_gpu_moments import _fcn_problem
from tests.test_gpu_predict import DEV, ROOT, _fcn_engine, _run

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _levels():
    from mile_amd import metrics as M
    return sorted(set(M.interval_levels([0.5, 0.75, 0.9, 0.95]).tolist()) | {0.5})


_ENGINE = {}


def _engine():
    """Any engine: mixture_quantiles needs no handle, only the library and the device."""
    if 'e' not in _ENGINE:
        ospec, prob, _ = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 8, 1)
        _ENGINE['e'] = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    return _ENGINE['e']


def _random_raw(S, N, seed):
    rng = np.random.default_rng(seed)
    centre, spread = rng.standard_normal(N) * 3.0, np.exp(rng.uniform(-3.0, 1.0, N))
    mu = centre[None] + spread[None] * rng.standard_normal((S, N))
    ls = rng.uniform(-2.0, 1.0, N)[None] + 0.5 * rng.standard_normal((S, N))
    return np.stack([mu, ls], axis=-1).astype(np.float32)


def _bimodal_raw():
    """Rows of two groups 50 sigma apart, the lower one holding 25 %, 40 % and 75 % of the 200 draws in turn: a level equal
    to that share lies on the flat stretch of F between the groups."""
    rng = np.random.default_rng(5)
    S, rows = 200, []
    for share in (0.25, 0.4, 0.75):
        k = int(round(share * S))
        mu = np.concatenate([-25.0 + 0.1 * rng.standard_normal(k), 25.0 + 0.1 * rng.standard_normal(S - k)])
        rows.append(np.stack([mu, np.zeros(S)], axis=-1))
    return np.stack(rows, axis=1).astype(np.float32)


def _clip_raw():
    """log sigma at and beyond both clips of sigma = clip(exp(log sigma), 1e-6, 1e6): the clip values themselves
    (+-13.8155...), -20 and 20, and rows that mix clipped and plain draws."""
    rng = np.random.default_rng(6)
    S = 64
    at = np.float32(np.log(1e6))
    cols = [np.full(S, -20.0), np.full(S, 20.0), np.full(S, -at), np.full(S, at),
            np.where(np.arange(S) % 2 == 0, -20.0, 0.0), np.where(np.arange(S) % 3 == 0, 20.0, -1.0)]
    ls = np.stack(cols, axis=1)
    mu = rng.standard_normal((S, len(cols))) * np.array([1.0, 1.0, 1e-6, 1e5, 1.0, 1.0])
    return np.stack([mu, ls], axis=-1).astype(np.float32)


def _nonfinite_raw():
    raw = _random_raw(50, 6, 7)
    raw[3, 0, 0] = np.nan
    raw[4, 0, 1] = np.inf
    raw[5, 1, 0] = -np.inf
    raw[7, 1, 1] = -np.inf
    raw[9, 1, 1] = np.nan
    raw[:, 2, 0] = np.nan                                           # nothing kept
    raw[1:, 3, 1] = np.inf                                          # one draw kept
    return raw, [2, 3, 50, 49, 0, 0]


SOLVER_CASES = {
    'random_300x70': lambda: _random_raw(300, 70, 1),
    'one_draw': lambda: _random_raw(1, 9, 2),
    'one_past_a_workgroup_257': lambda: _random_raw(257, 5, 3),
    'bimodal': _bimodal_raw,
    'sigma_clips': _clip_raw,
    'streamed_40000x3': lambda: _random_raw(40000, 3, 4),
}


def _check_solver(tag, raw, levels, got_q, got_pit, y):
    got_q, got_pit = got_q.cpu().numpy().astype(np.float64), got_pit.cpu().numpy().astype(np.float64)
    ref = QR.quantiles(raw, levels)
    sd = QR.mixture_sd(raw)
    fin = np.isfinite(ref).all(axis=1)
    assert got_q.shape == ref.shape and np.isnan(got_q[~fin]).all() and np.isnan(got_pit[~fin]).all(), tag
    assert np.isfinite(got_q[fin]).all() and np.isfinite(got_pit[fin]).all(), tag
    err = np.abs(got_q - ref)[fin]
    bound = (2.0 ** -22 * np.maximum(np.abs(ref), sd[:, None]))[fin]
    res = np.abs(QR.cdf(raw, got_q) - np.asarray(levels)[None])[fin]
    print(f'{tag}: max |q - q*| / bound = {(err / bound).max():.3f}, rows x levels by the residual rule = '
          f'{int(((err > bound) & (res <= 1e-12)).sum())}, max residual |F(q) - p| = {res.max():.3e}')
    assert ((err <= bound) | (res <= 1e-12)).all(), (tag, (err / bound).max(), res.max())
    assert (np.diff(got_q[fin], axis=1) >= 0).all(), (tag, 'quantiles must not decrease with the level')
    epit = np.abs(got_pit - QR.pit(raw, y))[fin].max()
    print(f'{tag}: max |pit - pit*| = {epit:.3e}, bound {2.0 ** -22:.3e}')
    assert epit <= 2.0 ** -22, (tag, epit)


@pytest.mark.parametrize('case', list(SOLVER_CASES))
def test_solver_on_given_outputs(case):
    raw = SOLVER_CASES[case]()
    levels = [0.25, 0.4, 0.75] if case == 'bimodal' else _levels()
    rng = np.random.default_rng(11)
    y = (raw[rng.integers(0, raw.shape[0], raw.shape[1]), np.arange(raw.shape[1]), 0]
         + rng.standard_normal(raw.shape[1]).astype(np.float32)).astype(np.float32)
    q, pit, dropped = _engine().mixture_quantiles(torch.from_numpy(raw), levels, y=torch.from_numpy(y), return_dropped=True)
    assert q.shape == (raw.shape[1], len(levels)) and q.dtype == pit.dtype == torch.float32 and dropped.dtype == torch.int32
    assert not dropped.any()
    _check_solver(case, raw, levels, q, pit, y)
    if case == 'one_draw':                                         # S = 1: mu + z_p sigma, the bracket itself
        from scipy.special import ndtri
        exact = raw[0, :, :1].astype(np.float64) + ndtri(np.array(levels))[None] * np.exp(raw[0, :, 1:].astype(np.float64))
        assert np.abs(q.cpu().numpy() - exact).max() <= 2.0 ** -23 * np.abs(exact).max()
    if case == 'random_300x70':                                    # quantiles alone, PIT alone: the same numbers
        only_q = _engine().mixture_quantiles(torch.from_numpy(raw), levels)
        assert torch.equal(only_q, q)


def test_nonfinite_draws_are_left_out_per_row():
    raw, want = _nonfinite_raw()
    levels = _levels()
    y = np.linspace(-1.0, 1.0, raw.shape[1]).astype(np.float32)
    eng = _engine()
    q, pit, dropped = eng.mixture_quantiles(torch.from_numpy(raw), levels, y=torch.from_numpy(y), return_dropped=True)
    assert dropped.tolist() == want
    assert torch.isnan(q[2]).all() and torch.isnan(pit[2])          # the all-NaN row
    _check_solver('nonfinite', raw, levels, q, pit, y)
    # the kept draws alone give the same bits: a left-out draw has weight 0
    keep = np.isfinite(raw[:, 1]).all(axis=-1)
    q1 = eng.mixture_quantiles(torch.from_numpy(np.ascontiguousarray(raw[keep][:, 1:2])), levels)
    q1, q2 = q1.cpu().numpy().astype(np.float64)[0], q.cpu().numpy().astype(np.float64)[1]
    assert (np.abs(q1 - q2) <= 2.0 ** -22 * np.maximum(np.abs(q2), QR.mixture_sd(raw)[1])).all()


def test_outputs_beyond_the_budget_are_walked_in_tiles_of_their_own_rows():
    """S = 2^20, N = 33: the packed copy of 32 rows fills the budget, so mile_mixture_quantiles walks the caller's array
    (ld = N) in a tile of 32 rows and one of 1.  A row's result depends on its own pairs only: the call on all rows is, bit
    for bit, the call on each tile's rows alone."""
    S, N, tile, levels = 1 << 20, 33, 32, [0.05, 0.5, 0.95]
    assert (256 << 20) // (S * 8) == tile < N
    gen = torch.Generator(device=DEV).manual_seed(12)
    raw = torch.randn(S, N, 2, device=DEV, generator=gen)
    raw[..., 0] += torch.linspace(-3.0, 3.0, N, device=DEV)
    raw[..., 1] *= 0.5
    y = torch.linspace(-4.0, 4.0, N, device=DEV)
    eng = _engine()
    whole = eng.mixture_quantiles(raw, levels, y=y, return_dropped=True)
    assert torch.isfinite(whole[0]).all() and not whole[2].any()
    parts = [eng.mixture_quantiles(raw[:, r0:r0 + tile].contiguous(), levels, y=y[r0:r0 + tile], return_dropped=True) for r0 in range(0, N, tile)]
    for k, name in enumerate(('quant', 'pit', 'dropped')):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), name


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _end_to_end(tag, eng, theta, X, out64, out32):
    levels = _levels()
    sd = QR.mixture_sd(out64)
    ref_q = QR.quantiles(out64, levels)
    rng = np.random.default_rng(12)
    y = (ref_q[:, len(levels) // 2] + sd * rng.standard_normal(len(sd))).astype(np.float32)
    ref_pit = QR.pit(out64, y)
    q, pit, dropped = eng.predict_quantiles(torch.from_numpy(theta), torch.from_numpy(X), levels, y=torch.from_numpy(y),
                                            return_dropped=True)
    assert q.shape == ref_q.shape and not dropped.any()
    q, pit = q.cpu().numpy().astype(np.float64), pit.cpu().numpy().astype(np.float64)
    r32 = np.ascontiguousarray(out32, dtype=np.float32)
    e32 = np.abs(QR.quantiles(r32, levels) - ref_q)
    err = np.abs(q - ref_q)
    bound = 1e-4 * max(1.0, np.abs(ref_q).max())
    print(f'{tag} quantiles: max|q - q*| = {err.max():.3e} (bound {bound:.3e}); in units of sd_n: device {(err / sd[:, None]).max():.3e}, '
          f'float32 restatement {(e32 / sd[:, None]).max():.3e}; log sigma from {out64[..., 1].min():.1f} to {out64[..., 1].max():.1f}')
    epit, e32pit = np.abs(pit - ref_pit).max(), np.abs(QR.pit(r32, y) - ref_pit).max()
    print(f'{tag} pit: max|pit - pit*| = {epit:.3e} (bound 1e-4), float32 restatement {e32pit:.3e}')
    assert (e32 <= 1e-3 * sd[:, None]).all(), (tag, 'badly chosen inputs', (e32 / sd[:, None]).max())
    assert err.max() < bound, (tag, err.max(), bound)
    assert epit < 1e-4, (tag, epit)
    assert (np.diff(q, axis=1) >= 0).all()


FCN_E2E = [('mfma_narrow_f32', (16, 16, 2)), ('mfma_w64', (64, 64, 64, 2))]


@pytest.mark.parametrize('kernel,hs', FCN_E2E)
def test_fcn_end_to_end(kernel, hs):
    ospec, prob, X = _fcn_problem(5, hs, 'relu', 'regr', 70, 300)
    eng = _fcn_engine(ospec, prob, kernel)
    _end_to_end(kernel, eng, prob['theta0'], X, O.mlp_forward(ospec, prob['theta0'].astype(np.float64), X.astype(np.float64)),
                O.mlp_forward(ospec, prob['theta0'], X))
    rows, total, most = eng.debug_quantile_sweeps()
    print(f'{kernel}: {total / rows:.2f} sweeps per row, at most {most}')
    assert rows == 70 and 0 < most < 200                           # (the hard cap is never what ends the loop)


def test_lenetti_end_to_end():
    from mile_amd import LeNettiSpec
    from mile_amd.engine import Engine
    ospec = RL.LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr')
    prob = RL.synthetic_problem(ospec, 20, 5, seed=6)
    X = RL.synthetic_problem(ospec, 70, 1, seed=7)['X']
    eng = Engine(LeNettiSpec(3, 9, 11, 2, activation='tanh', task='regr'), torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device=DEV)
    assert eng.grad_kernel == 'lenetti_f32'
    _end_to_end('lenetti', eng, prob['theta0'], X.reshape(len(X), -1), RL.forward(ospec, prob['theta0'].astype(np.float64), X),
                RL.forward(ospec, prob['theta0'], X))


@pytest.mark.parametrize('kernel,hs', FCN_E2E)
def test_every_tiling_gives_the_same_bits(kernel, hs):
    ospec, prob, X = _fcn_problem(5, hs, 'relu', 'regr', 70, 300)
    eng = _fcn_engine(ospec, prob, kernel)
    th, Xt, levels = torch.from_numpy(prob['theta0']), torch.from_numpy(X), _levels()
    y = torch.from_numpy(np.random.default_rng(13).standard_normal(70).astype(np.float32))
    base = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    for draws in (0, 7, 300):
        for rows in (0, 32, 70):                                   # 32: two full tiles and a ragged one of 6
            got = eng.predict_quantiles(th, Xt, levels, y=y, max_draws_per_pass=draws, max_rows_per_tile=rows, return_dropped=True)
            assert all(torch.equal(a, b) for a, b in zip(got, base)), (kernel, draws, rows)
    # and they are the solver on mile_predict's outputs, and PIT and quantiles tell the same coverage
    from mile_amd import metrics as M
    alone = eng.mixture_quantiles(eng.predict(th, Xt), levels, y=y, return_dropped=True)
    assert all(torch.equal(a, b) for a, b in zip(alone, base))
    q, pit = base[0].double().cpu(), base[1].cpu()
    cov = [0.5, 0.75, 0.9, 0.95]
    counted = []
    for c in cov:
        lo, hi = (levels.index(v) for v in M.get_quantiles(c).tolist())
        counted.append(float(((q[:, lo] <= y.double()) & (y.double() <= q[:, hi])).double().mean()))
    from_pit = M.coverage_from_pit(pit, cov).tolist()
    print(f'{kernel}: coverage from PIT {from_pit}, counted from the quantiles {counted}')
    assert from_pit == counted


def test_streamed_calls_share_one_workspace():
    """predict_quantiles, predict_moments and lppd_stream lay their blocks out in the same buffer of the handle: a quantile
    call gives the same bits after the others have used it, and the sweeps of a quantile call are forgotten, not read
    back stale, once another streamed call has reused the buffer."""
    eng = _engine()
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 12)
    th, Xt, levels = torch.from_numpy(prob['theta0']), torch.from_numpy(X), _levels()
    y = torch.from_numpy(np.random.default_rng(13).standard_normal(70).astype(np.float32))
    first = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    assert eng.debug_quantile_sweeps()[0] == 70
    moments = eng.predict_moments(th, Xt)
    assert eng.debug_quantile_sweeps()[0] == 0
    lppd = eng.lppd_stream(th.reshape(3, 4, -1), Xt, y)
    again = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    assert eng.debug_quantile_sweeps()[0] == 70
    assert all(torch.equal(a, b) for a, b in zip(again, first))
    assert torch.isfinite(moments).all() and torch.isfinite(lppd['lppd'])


def test_refusals_leave_the_handle_usable():
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 3)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt = torch.from_numpy(prob['theta0']), torch.from_numpy(X)
    with pytest.raises(ValueError):
        eng.predict_quantiles(th, Xt, [0.5, 0.25])
    with pytest.raises(ValueError):
        eng.predict_quantiles(th, Xt, [0.0, 0.5])
    with pytest.raises(Exception, match='mile_predict_quantiles'):
        eng.predict_quantiles(th, Xt, [0.5], max_rows_per_tile=-1)
    cspec, cprob, cX = _fcn_problem(7, (40, 40, 3), 'tanh', 'classification', 30, 3)
    with pytest.raises(ValueError):
        _fcn_engine(cspec, cprob, 'mfma_narrow_f32').predict_quantiles(torch.from_numpy(cprob['theta0']), torch.from_numpy(cX), [0.5])
    assert eng.predict_quantiles_workspace(3, 70) > 0 and eng.predict_quantiles_workspace(0, 70) == -1
    q = eng.predict_quantiles(th, Xt, [0.1, 0.5, 0.9])
    assert torch.isfinite(q).all() and (q[:, 1:] >= q[:, :-1]).all()


def test_the_tools_on_a_tiny_run(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test'])
    plain = json.loads((exp / 'metrics.json').read_text())
    assert not (exp / 'intervals.npz').exists() and not any(k.startswith('intervals_') for k in plain)
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--intervals'])
    m = json.loads((exp / 'metrics.json').read_text())
    assert {k: v for k, v in m.items() if not k.startswith('intervals_')} == plain          # the seeded keys included
    cov = [0.5, 0.75, 0.9, 0.95]
    assert all(0.0 <= m[f'intervals_coverage_{c}'] <= 1.0 and m[f'intervals_width_{c}'] > 0 for c in cov)
    assert all(m[f'intervals_width_{a}'] < m[f'intervals_width_{b}'] for a, b in zip(cov, cov[1:]))
    obs = np.array([m[f'intervals_coverage_{c}'] for c in cov])
    assert m['intervals_cal_error'] == pytest.approx(float(np.sqrt(np.mean((np.array(cov) - obs) ** 2))), rel=1e-12)
    assert m['intervals_dropped'] == 0
    z = np.load(exp / 'intervals.npz')
    n = plain['n_points']
    assert sorted(z.files) == ['dropped', 'levels', 'pit', 'quantiles']
    assert z['levels'].shape == (8,) and z['quantiles'].shape == (n, 8) and z['pit'].shape == z['dropped'].shape == (n,)
    assert (np.diff(z['quantiles'], axis=1) >= 0).all() and ((z['pit'] >= 0) & (z['pit'] <= 1)).all()
    # predict.py on 20 new rows in the units of the raw data: quantiles in target units around the mean of the same file
    norm = np.load(exp / 'normalization.npz')
    F = norm['x_mean'].shape[0]
    table = (np.random.default_rng(0).standard_normal((20, F)) * norm['x_std'] + norm['x_mean']).astype(np.float32)
    np.savetxt(tmp_path / 'new.csv', table, delimiter=',')
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'new.csv', '-o', tmp_path / 'plain.npz'])
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'new.csv', '-o', tmp_path / 'pred.npz', '--intervals', '0.5', '0.9'])
    old, pred = np.load(tmp_path / 'plain.npz'), np.load(tmp_path / 'pred.npz')
    assert sorted(old.files) == ['aleatoric_var', 'dropped', 'epistemic_var', 'mean']
    assert sorted(pred.files) == sorted(old.files + ['quantile_levels', 'quantiles'])
    assert all(np.array_equal(old[k], pred[k]) for k in old.files)
    np.testing.assert_allclose(pred['quantile_levels'], [0.05, 0.25, 0.5, 0.75, 0.95], rtol=0, atol=1e-15)
    assert pred['quantiles'].shape == (20, 5) and (np.diff(pred['quantiles'], axis=1) > 0).all()
    sd = np.sqrt(pred['epistemic_var'] + pred['aleatoric_var'])
    assert (np.abs(pred['quantiles'][:, 2] - pred['mean']) <= 3.0 * sd).all()
    # target units: the same rows with the outputs left in the training normalisation map onto them
    xn = ((table - norm['x_mean']) / norm['x_std']).astype(np.float32)
    np.save(tmp_path / 'xn.npy', xn)
    _run([ROOT / 'predict.py', '-e', exp, '-i', tmp_path / 'xn.npy', '-o', tmp_path / 'normed.npz', '--normalized', '--intervals', '0.5', '0.9'])
    qn = np.load(tmp_path / 'normed.npz')['quantiles']
    ys, ym = float(norm['y_std'][0]), float(norm['y_mean'][0])
    np.testing.assert_allclose(pred['quantiles'], qn * ys + ym, rtol=1e-5, atol=1e-4 * max(1.0, abs(ym), ys))

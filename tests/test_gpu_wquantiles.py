"""mile_mixture_quantiles_weighted / mile_predict_quantiles_weighted (Engine.mixture_quantiles_weighted,
Engine.predict_quantiles_weighted) against the fp64 reference of tests/wquantile_ref.py (-m gpu): the weighted solver on
crafted outputs in the smallest shapes where it can go wrong, the leave-out rules, its consistency with the equal-weight
entry points, end to end through the forward kernels with every tiling bit for bit, the shared workspace, the refusals and
the two command-line tools.

Bounds: those of tests/test_gpu_quantiles.py.  Solver on given fp32 outputs: each quantile within 2^-22 max(|q*|, sd_n) of the
reference OR |F_ref(q) - p| <= 1e-12, the second rule allowed only on the flat stretch; PIT within 2^-22.  End to end:
max|q - q*| < 1e-4 max(1, max|q*|) and PIT within 1e-4 against the reference fed the fp64 oracle forward.  Two device results
for the same mixture (w = 1 / C against the equal-weight entry, a one-hot w against the chain's slice) are compared within
the solver bound of one, 2^-22 max(|q|, sd_n): each is an fp32 rounding (2^-24 |q|) and half a stopping width
(2^-26 max(|q|, sd_n)) away from the root.

Measured on an MI355X: solver cases at most 0.23 of the quantile bound with no entry by the residual rule, except the flat
stretch, where the three entries at level 0.3 pass by it (residual 2.3e-7 at the other levels' worst, |F - p| <= 1e-12 on the
stretch); PIT at most 2.8e-8.  End to end: narrow 9.8e-7 (bound 8.4e-4), 3.4e-7 sd_n, PIT 3.4e-8; w64 7.0e-3 (bound 4.4),
2.8e-6 sd_n, PIT 5.2e-8.

Partition mode: the unweighted quantile tests have no case with set_partition, so there is none here either."""
import json
import shutil

import numpy as np
import pytest

from oracle import mclmc_oracle as O
from tests import quantile_ref as QR
from tests import wquantile_ref as WR
from tests.test_gpu_moments import _fcn_problem
from tests.test_gpu_predict import ROOT, _fcn_engine, _run
from tests.test_gpu_quantiles import _clip_raw, _levels

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

_ENGINE = {}


def _engine():
    """Any engine: mixture_quantiles_weighted needs no handle, only the library and the device."""
    if 'e' not in _ENGINE:
        ospec, prob, _ = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 8, 1)
        _ENGINE['e'] = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    return _ENGINE['e']


def _random_raw(Cn, S, N, seed):
    """Chains that do not mix: each has its own offset of the order of the spread within it."""
    rng = np.random.default_rng(seed)
    centre, spread = rng.standard_normal(N) * 3.0, np.exp(rng.uniform(-3.0, 1.0, N))
    mu = centre + spread * rng.standard_normal((Cn, S, N)) + 1.5 * spread * rng.standard_normal((Cn, 1, N))
    ls = rng.uniform(-2.0, 1.0, N) + 0.5 * rng.standard_normal((Cn, S, N))
    return np.stack([mu, ls], axis=-1).astype(np.float32)


def _simplex(Cn, seed):
    w = np.random.default_rng(seed).dirichlet(np.ones(Cn))
    return w / w.sum()


def _flat_raw():
    """Two chains 50 sigma apart, w = (0.3, 0.7): the level 0.3 lies on the flat stretch of F between them."""
    rng = np.random.default_rng(5)
    mu = np.stack([-25.0 + 0.1 * rng.standard_normal((7, 3)), 25.0 + 0.1 * rng.standard_normal((7, 3))])
    return np.stack([mu, np.zeros_like(mu)], axis=-1).astype(np.float32)


# name -> (raw [C, S, N, 2], weights [C], levels or None for the interval levels)
SOLVER_CASES = {
    'C1_S1': lambda: (_random_raw(1, 1, 9, 1), [1.0], None),
    'C3_S1_one_draw_per_chain': lambda: (_random_raw(3, 1, 9, 2), [0.2, 0.3, 0.5], None),
    'C5_S7_boundaries_off_every_stride': lambda: (_random_raw(5, 7, 9, 3), _simplex(5, 3), None),
    'C257_S1_one_past_a_workgroup': lambda: (_random_raw(257, 1, 5, 4), _simplex(257, 4), None),
    'C1_S257_one_past_a_workgroup': lambda: (_random_raw(1, 257, 5, 5), [1.0], None),
    'Q1': lambda: (_random_raw(5, 7, 9, 6), _simplex(5, 6), [0.37]),
    'Q5_idle_lanes': lambda: (_random_raw(5, 7, 9, 7), _simplex(5, 7), [0.05, 0.25, 0.5, 0.75, 0.95]),
    'Q32_two_components_per_wave_step': lambda: (_random_raw(5, 7, 9, 8), _simplex(5, 8), [(i + 1) / 33 for i in range(32)]),
    'streamed_C4_S4100': lambda: (_random_raw(4, 4100, 3, 9), _simplex(4, 9), None),
    'C1024_S2_largest_chain_table': lambda: (_random_raw(1024, 2, 2, 10), _simplex(1024, 10), None),
    # (weights off every grid: with sigma = 1e-6 F is a staircase, and weights such as 0.1 .. 0.4 over 16 draws put partial sums
    # of w_c / 16 exactly on the levels -- flat stretches, which are the next case's subject, not this one's)
    'sigma_clips': lambda: (_clip_raw().reshape(4, 16, -1, 2), _simplex(4, 12), None),
    'flat_stretch': lambda: (_flat_raw(), [0.3, 0.7], [0.1, 0.3, 0.6]),
    'exact_zero_weights': lambda: (_random_raw(5, 7, 9, 11), [0.5, 0.0, 0.25, 0.0, 0.25], None),
}


def _check_solver(tag, raw, w, levels, got_q, got_pit, y, residual_rule=False):
    got_q, got_pit = got_q.cpu().numpy().astype(np.float64), got_pit.cpu().numpy().astype(np.float64)
    ref = WR.quantiles(raw, w, levels)
    sd = WR.mixture_sd(raw, w)
    fin = np.isfinite(ref).all(axis=1)
    assert got_q.shape == ref.shape and np.isnan(got_q[~fin]).all() and np.isnan(got_pit[~fin]).all(), tag
    assert np.isfinite(got_q[fin]).all() and np.isfinite(got_pit[fin]).all(), tag
    err = np.abs(got_q - ref)[fin]
    bound = (2.0 ** -22 * np.maximum(np.abs(ref), sd[:, None]))[fin]
    res = np.abs(WR.cdf(raw, w, got_q) - np.asarray(levels)[None])[fin]
    by_residual = int(((err > bound) & (res <= 1e-12)).sum())
    print(f'{tag}: max |q - q*| / bound = {(err / bound).max():.3f}, rows x levels by the residual rule = {by_residual}, '
          f'max residual |F(q) - p| = {res.max():.3e}')
    assert ((err <= bound) | (res <= 1e-12)).all(), (tag, (err / bound).max(), res.max())
    assert residual_rule or by_residual == 0, (tag, 'the residual rule is for the flat stretch only', by_residual)
    assert (np.diff(got_q[fin], axis=1) >= 0).all(), (tag, 'quantiles must not decrease with the level')
    epit = np.abs(got_pit - WR.pit(raw, w, y))[fin].max()
    print(f'{tag}: max |pit - pit*| = {epit:.3e}, bound {2.0 ** -22:.3e}')
    assert epit <= 2.0 ** -22, (tag, epit)


def _some_y(raw, seed=11):
    rng = np.random.default_rng(seed)
    Cn, S, N = raw.shape[:3]
    y = raw[rng.integers(0, Cn, N), rng.integers(0, S, N), np.arange(N), 0] + rng.standard_normal(N).astype(np.float32)
    return np.where(np.isfinite(y), y, 0.0).astype(np.float32)


@pytest.mark.parametrize('case', list(SOLVER_CASES))
def test_solver_on_given_outputs(case):
    raw, w, levels = SOLVER_CASES[case]()
    levels = levels or _levels()
    y = _some_y(raw)
    q, pit, dropped = _engine().mixture_quantiles_weighted(torch.from_numpy(raw), w, levels, y=torch.from_numpy(y), return_dropped=True)
    assert q.shape == (raw.shape[2], len(levels)) and q.dtype == pit.dtype == torch.float32
    assert dropped.dtype == torch.int32 and dropped.shape == raw.shape[:1] + raw.shape[2:3] and not dropped.any()
    _check_solver(case, raw, w, levels, q, pit, y, residual_rule=case == 'flat_stretch')
    if case == 'flat_stretch':                                     # the bracket closed on the stretch: between the two chains
        mid = q.cpu().numpy()[:, 1]
        assert (mid > raw[0, :, :, 0].max(axis=0)).all() and (mid < raw[1, :, :, 0].min(axis=0)).all()
    if case == 'C1_S1':                                            # one component: mu + z_p sigma, the bracket itself
        from scipy.special import ndtri
        exact = raw[0, 0, :, :1].astype(np.float64) + ndtri(np.array(levels))[None] * np.exp(raw[0, 0, :, 1:].astype(np.float64))
        assert np.abs(q.cpu().numpy() - exact).max() <= 2.0 ** -23 * np.abs(exact).max()


def test_leave_out_rules():
    """NaN and +-inf draws of a weighted chain are dropped per row and counted exactly; a zero-weight chain that is all NaN
    leaves every row finite; a weighted chain with nothing kept makes that row alone NaN."""
    raw = _random_raw(3, 9, 11, 12)
    raw[1] = np.nan                                                 # zero weight below
    raw[0, 2, 0, 0] = np.nan
    raw[0, 3, 0, 1] = np.inf
    raw[2, 5, 1, 0] = -np.inf
    raw[2, 7, 1, 1] = -np.inf
    raw[2, :, 4, 1] = np.nan                                        # a weighted chain with nothing kept on row 4
    raw[0, 1:, 6, 0] = np.inf                                       # one draw kept on row 6
    w, levels, y = [0.25, 0.0, 0.75], _levels(), _some_y(raw)
    want = np.zeros((3, 11), dtype=np.int32)
    want[1], want[0, 0], want[2, 1], want[2, 4], want[0, 6] = 9, 2, 2, 9, 8
    eng = _engine()
    q, pit, dropped = eng.mixture_quantiles_weighted(torch.from_numpy(raw), w, levels, y=torch.from_numpy(y), return_dropped=True)
    assert np.array_equal(dropped.cpu().numpy(), want) and np.array_equal(WR.dropped(raw), want)
    nan_rows = torch.isnan(q).any(dim=1).cpu().numpy()
    assert nan_rows.tolist() == [n == 4 for n in range(11)] and torch.isnan(q[4]).all() and torch.isnan(pit[4])
    _check_solver('leave_out', raw, w, levels, q, pit, y)
    # weight on the all-NaN chain: every row NaN, and the counts are the same
    q, pit, dropped = eng.mixture_quantiles_weighted(torch.from_numpy(raw), [0.2, 0.3, 0.5], levels, y=torch.from_numpy(y), return_dropped=True)
    assert torch.isnan(q).all() and torch.isnan(pit).all() and np.array_equal(dropped.cpu().numpy(), want)


def _within_solver_bound(tag, a, b, sd):
    a, b = a.double().cpu().numpy(), b.double().cpu().numpy()
    rel = np.abs(a - b) / (2.0 ** -22 * np.maximum(np.abs(b), sd[:, None]))
    print(f'{tag}: max |q_a - q_b| / bound = {rel.max():.3f}')
    assert rel.max() <= 1.0, (tag, rel.max())


def test_consistency_with_the_equal_weight_entry_points():
    raw = _random_raw(4, 33, 17, 13)
    rt, levels = torch.from_numpy(raw), _levels()
    y = torch.from_numpy(_some_y(raw))
    eng = _engine()
    pooled = raw.reshape(-1, 17, 2)
    # w = 1 / C with nothing dropped: the equal-weight mixture of all draws (not bitwise: the sums differ in their last bits)
    q, pit = eng.mixture_quantiles_weighted(rt, [0.25] * 4, levels, y=y)
    q0, pit0 = eng.mixture_quantiles(rt, levels, y=y)
    _within_solver_bound('w = 1 / C', q, q0, QR.mixture_sd(pooled))
    assert (pit - pit0).abs().max() <= 2.0 ** -22
    # a one-hot w: that chain's slice alone
    q1, pit1 = eng.mixture_quantiles_weighted(rt, [0.0, 0.0, 1.0, 0.0], levels, y=y)
    q2, pit2 = eng.mixture_quantiles(rt[2], levels, y=y)
    _within_solver_bound('one-hot', q1, q2, QR.mixture_sd(raw[2]))
    assert (pit1 - pit2).abs().max() <= 2.0 ** -22
    # quantiles alone are the quantiles asked for together with PIT, bit for bit; and a second call gives the same bits
    w = _simplex(4, 13)
    both = eng.mixture_quantiles_weighted(rt, w, levels, y=y)
    assert torch.equal(eng.mixture_quantiles_weighted(rt, w, levels), both[0])
    again = eng.mixture_quantiles_weighted(rt, w, levels, y=y)
    assert torch.equal(again[0], both[0]) and torch.equal(again[1], both[1])


# ---- end to end ------------------------------------------------------------------------------------------------------------
FCN_E2E = [('mfma_narrow_f32', (16, 16, 2)), ('mfma_w64', (64, 64, 64, 2))]
W_E2E = [0.5, 0.125, 0.375]


@pytest.mark.parametrize('kernel,hs', FCN_E2E)
def test_fcn_end_to_end_in_every_tiling(kernel, hs):
    ospec, prob, X = _fcn_problem(5, hs, 'relu', 'regr', 70, 12)
    eng = _fcn_engine(ospec, prob, kernel)
    levels = _levels()
    out64 = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), X.astype(np.float64)).reshape(3, 4, 70, 2)
    sd, ref_q = WR.mixture_sd(out64, W_E2E), WR.quantiles(out64, W_E2E, levels)
    y = (ref_q[:, len(levels) // 2] + sd * np.random.default_rng(12).standard_normal(70)).astype(np.float32)
    ref_pit = WR.pit(out64, W_E2E, y)
    th, Xt, yt = torch.from_numpy(prob['theta0']).reshape(3, 4, -1), torch.from_numpy(X), torch.from_numpy(y)
    base = eng.predict_quantiles_weighted(th, Xt, W_E2E, levels, y=yt, return_dropped=True)
    q, pit = base[0].double().cpu().numpy(), base[1].double().cpu().numpy()
    assert q.shape == ref_q.shape and base[2].shape == (3, 70) and not base[2].any()
    err, bound, epit = np.abs(q - ref_q), 1e-4 * max(1.0, np.abs(ref_q).max()), np.abs(pit - ref_pit).max()
    print(f'{kernel} quantiles: max|q - q*| = {err.max():.3e} (bound {bound:.3e}), in units of sd_n {(err / sd[:, None]).max():.3e}; '
          f'pit: max|pit - pit*| = {epit:.3e} (bound 1e-4)')
    assert err.max() < bound and epit < 1e-4 and (np.diff(q, axis=1) >= 0).all()
    for draws in (0, 1, 5):
        for rows in (0, 32, 33):                                   # 32: two full tiles and a ragged one; 33: rounded down to 32 or not, the same bits
            got = eng.predict_quantiles_weighted(th, Xt, W_E2E, levels, y=yt, max_draws_per_pass=draws, max_rows_per_tile=rows,
                                                 return_dropped=True)
            assert all(torch.equal(a, b) for a, b in zip(got, base)), (kernel, draws, rows)
    alone = eng.mixture_quantiles_weighted(eng.predict(th, Xt), W_E2E, levels, y=yt, return_dropped=True)
    assert all(torch.equal(a, b) for a, b in zip(alone, base))
    assert eng.predict_quantiles_weighted_workspace(3, 4, 70) > 0


def test_a_weighted_call_shares_the_workspace():
    """The weighted call lays its blocks out in the buffer predict_quantiles uses: a predict_quantiles call gives the same
    bits before and after one, and the sweeps recorded there are forgotten, not read back stale."""
    eng = _engine()
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 12)
    th, Xt, levels = torch.from_numpy(prob['theta0']), torch.from_numpy(X), _levels()
    y = torch.from_numpy(np.random.default_rng(13).standard_normal(70).astype(np.float32))
    first = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    assert eng.debug_quantile_sweeps()[0] == 70
    weighted = eng.predict_quantiles_weighted(th.reshape(3, 4, -1), Xt, W_E2E, levels, y=y)
    assert eng.debug_quantile_sweeps()[0] == 0
    again = eng.predict_quantiles(th, Xt, levels, y=y, return_dropped=True)
    assert all(torch.equal(a, b) for a, b in zip(again, first))
    assert torch.isfinite(weighted[0]).all() and torch.isfinite(weighted[1]).all()


def test_refusals_leave_the_handle_usable():
    import ctypes as C
    from mile_amd.engine import _ptr
    ospec, prob, X = _fcn_problem(5, (16, 16, 2), 'relu', 'regr', 70, 12)
    eng = _fcn_engine(ospec, prob, 'mfma_narrow_f32')
    th, Xt = torch.from_numpy(prob['theta0']).reshape(3, 4, -1), torch.from_numpy(X)
    for w in ([0.5, 0.5], [0.5, 0.75, -0.25], [0.5, float('nan'), 0.5], [0.5, 0.25, 0.25 + 1e-8]):     # the Python layer's checks
        with pytest.raises(ValueError):
            eng.predict_quantiles_weighted(th, Xt, w, [0.5])
    with pytest.raises(ValueError):
        eng.predict_quantiles_weighted(th, Xt, W_E2E, [0.5, 0.25])
    with pytest.raises(ValueError):
        eng.predict_quantiles_weighted(th.reshape(12, -1), Xt, W_E2E, [0.5])
    with pytest.raises(Exception, match='mile_predict_quantiles_weighted'):
        eng.predict_quantiles_weighted(th, Xt, W_E2E, [0.5], max_rows_per_tile=-1)
    # the library's own, behind the Python layer: every MILE_ERR_INVALID of the header
    thd, Xd = th.reshape(12, -1).to(eng.device).contiguous(), Xt.to(eng.device)
    quant = torch.empty((70, 1), dtype=torch.float32, device=eng.device)
    dbl = lambda v: (C.c_double * len(v))(*v)
    ok = dict(theta=_ptr(thd), Cn=3, S=4, X=_ptr(Xd), N=70, w=dbl(W_E2E), lev=dbl([0.5]), Q=1, y=None, quant=_ptr(quant), pit=None, draws=0, rows=0)
    bad = [dict(theta=None), dict(X=None), dict(Cn=0), dict(Cn=1025), dict(S=0), dict(Cn=2, S=1 << 30), dict(N=0), dict(N=1 << 30),
           dict(w=None), dict(w=dbl([0.5, 0.75, -0.25])), dict(w=dbl([0.5, float('nan'), 0.5])), dict(w=dbl([float('inf'), 0.0, 0.0])),
           dict(w=dbl([0.5, 0.25, 0.25 + 1e-8])), dict(lev=None), dict(Q=0), dict(Q=33), dict(lev=dbl([1.0])), dict(pit=_ptr(quant)),
           dict(quant=None), dict(draws=-1), dict(rows=-1)]
    for kw in bad:
        a = {**ok, **kw}
        rc = eng.lib.mile_predict_quantiles_weighted(eng._h, a['theta'], a['Cn'], a['S'], a['X'], a['N'], a['w'], a['lev'], a['Q'], a['y'],
                                                     a['quant'], a['pit'], None, a['draws'], a['rows'], None)
        assert rc == -1 and 'mile_predict_quantiles_weighted' in eng.lib.mile_last_error().decode(), kw
    cspec, cprob, cX = _fcn_problem(7, (40, 40, 3), 'tanh', 'classification', 30, 12)
    with pytest.raises(ValueError):
        _fcn_engine(cspec, cprob, 'mfma_narrow_f32').predict_quantiles_weighted(torch.from_numpy(cprob['theta0']).reshape(3, 4, -1),
                                                                                torch.from_numpy(cX), W_E2E, [0.5])
    assert eng.predict_quantiles_weighted_workspace(0, 4, 70) == -1 and eng.predict_quantiles_weighted_workspace(1025, 4, 70) == -1
    q = eng.predict_quantiles_weighted(th, Xt, W_E2E, [0.1, 0.5, 0.9])
    assert torch.isfinite(q).all() and (q[:, 1:] >= q[:, :-1]).all()


def test_the_tools_on_a_tiny_run(tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / 'experiments' / 'smoke_synthetic.yaml').read_text())
    cfg['saving_dir'] = str(tmp_path)
    cfg['training']['sampler'].update(warmup_steps=50, n_samples=30, n_chains=4)
    (tmp_path / 'cfg.yaml').write_text(yaml.safe_dump(cfg))
    _run([ROOT / 'train.py', '-c', tmp_path / 'cfg.yaml', '-d', '1'])
    exp = tmp_path / 'smoke_synthetic'
    norm = np.load(exp / 'normalization.npz')
    F = norm['x_mean'].shape[0]
    table = (np.random.default_rng(0).standard_normal((20, F)) * norm['x_std'] + norm['x_mean']).astype(np.float32)
    np.savetxt(tmp_path / 'new.csv', table, delimiter=',')
    predict = lambda out, *more, e=exp: _run([ROOT / 'predict.py', '-e', e, '-i', tmp_path / 'new.csv', '-o', tmp_path / out,
                                              '--intervals', '0.5', '0.9', *more])
    # without --weights: the arrays of the equal-weight ensemble, as before
    predict('plain.npz')
    plain = np.load(tmp_path / 'plain.npz')
    assert sorted(plain.files) == ['aleatoric_var', 'dropped', 'epistemic_var', 'mean', 'quantile_levels', 'quantiles']
    assert plain['dropped'].shape == (20,) and plain['quantiles'].shape == (20, 5)
    # w = 1 / C: the same mixture
    np.save(tmp_path / 'equal.npy', np.full(4, 0.25))
    predict('equal.npz', '--weights', tmp_path / 'equal.npy')
    eq = np.load(tmp_path / 'equal.npz')
    assert sorted(eq.files) == sorted(plain.files + ['chain_weights']) and eq['dropped'].shape == (4, 20)
    np.testing.assert_array_equal(eq['chain_weights'], np.full(4, 0.25))
    # 1e-6 relative to the largest mean: the chains' fp32 moments are each rounded at their own size, so a row whose chains
    # cancel to a mean near 0 holds no relative accuracy of its own
    assert np.abs(eq['mean'] - plain['mean']).max() <= 1e-6 * np.abs(plain['mean']).max()
    sd = np.sqrt(plain['epistemic_var'] + plain['aleatoric_var'])
    np.testing.assert_allclose(eq['epistemic_var'] + eq['aleatoric_var'], sd ** 2, rtol=1e-4)
    assert (np.abs(eq['quantiles'] - plain['quantiles']) <= 1e-5 * np.maximum(np.abs(plain['quantiles']), sd[:, None])).all()
    # a one-hot vector: a run on that chain alone
    (tmp_path / 'onehot.txt').write_text('0\n0\n1\n0\n')
    predict('onehot.npz', '--weights', tmp_path / 'onehot.txt')
    solo = tmp_path / 'solo'
    shutil.copytree(exp, solo)
    chains = sorted([d for d in (solo / 'samples').iterdir() if d.is_dir()], key=lambda d: int(d.stem.split('_')[-1]))
    assert len(chains) == 4
    for k, d in enumerate(chains):
        if k != 2:
            shutil.rmtree(d)
    predict('solo.npz', e=solo)
    hot, one = np.load(tmp_path / 'onehot.npz'), np.load(tmp_path / 'solo.npz')
    sd = np.sqrt(one['epistemic_var'] + one['aleatoric_var'])
    assert np.abs(hot['mean'] - one['mean']).max() <= 1e-6 * np.abs(one['mean']).max()
    np.testing.assert_allclose(hot['epistemic_var'], one['epistemic_var'], rtol=1e-4, atol=1e-6 * sd.max() ** 2)
    np.testing.assert_allclose(hot['aleatoric_var'], one['aleatoric_var'], rtol=1e-5)
    assert (np.abs(hot['quantiles'] - one['quantiles']) <= 1e-5 * np.maximum(np.abs(one['quantiles']), sd[:, None])).all()
    # evaluate.py: --stacking next to --intervals adds the stacked keys and arrays and leaves the others as they are
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--intervals', '--moments'])
    before, zb = json.loads((exp / 'metrics.json').read_text()), dict(np.load(exp / 'intervals.npz'))
    _run([ROOT / 'evaluate.py', '-e', exp, '--split', 'test', '--intervals', '--moments', '--stacking'])
    m, z = json.loads((exp / 'metrics.json').read_text()), np.load(exp / 'intervals.npz')
    assert {k: v for k, v in m.items() if 'stack' not in k} == before
    cov = [0.5, 0.75, 0.9, 0.95]
    assert all(0.0 <= m[f'intervals_stacked_coverage_{c}'] <= 1.0 and m[f'intervals_stacked_width_{c}'] > 0 for c in cov)
    assert m['intervals_stacked_cal_error'] >= 0 and m['moments_stacked_rmse'] > 0 and 'intervals_stacked_dropped' not in m
    assert sorted(z.files) == sorted(list(zb) + ['pit_stacked', 'quantiles_stacked'])
    assert all(np.array_equal(z[k], zb[k]) for k in zb)
    assert z['quantiles_stacked'].shape == zb['quantiles'].shape and z['pit_stacked'].shape == zb['pit'].shape
    assert (np.diff(z['quantiles_stacked'], axis=1) >= 0).all() and ((z['pit_stacked'] >= 0) & (z['pit_stacked'] <= 1)).all()

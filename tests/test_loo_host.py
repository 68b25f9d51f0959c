"""The fp64 restatement of PSIS-LOO and WAIC (tests/loo_ref.py) held to facts that do not come from it -- the generalised
Pareto's own quantiles, the exact leave-one-out density of a conjugate model, invariances -- the torch restatement of
mile_amd.metrics against it, and the host side of mile_psis_loo / mile_loo_stream: exports, bindings and every argument
refusal through ctypes on handles created without a GPU.

Measured on the CPU: test 1, worst |khat - (n k + 5) / (n + 10)| = 1.4e-3 and |sigma - 1| = 1.5e-3 (bound 5e-3); test 2,
worst |elpd_loo - exact| = 0.0099 (bound 0.03) and lppd_0 - exact between 0.61 and 0.68 (at least 0.5)."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from mile_amd import metrics as M
from tests import loo_ref as LR
from tests.test_predict_host import _attn_pre_cspec, _fcn_cspec

ROOT = Path(__file__).resolve().parents[1]
KEYS = ('lppd', 'p_waic', 'elpd_loo', 'khat')


# ---------------------------------------------------------------- the reference -----------------
@pytest.mark.parametrize('k', [-0.3, 0.2, 0.5, 0.9])
def test_gpdfit_recovers_a_generalised_pareto(k):
    n = 2000
    p = (np.arange(1, n + 1) - 0.5) / n
    khat, sigma = LR.gpdfit(np.expm1(-k * np.log1p(-p)) / k)
    print(f'k = {k}: khat - (n k + 5) / (n + 10) = {khat - (n * k + 5) / (n + 10):.2e}, sigma - 1 = {sigma - 1:.2e}')
    assert abs(khat - (n * k + 5) / (n + 10)) <= 5e-3 and abs(sigma - 1.0) <= 5e-3


def _conjugate(seed):
    """N = 20 unit-variance Normal observations with a N(0, 100) prior on their mean, one of them an outlier: S = 4000 exact
    posterior draws -> (loglik [S, N], the exact leave-one-out log predictive density of every row)."""
    rng = np.random.default_rng(seed)
    N, S = 20, 4000
    y = rng.standard_normal(N) + 0.3
    y[0] = 4.0
    v = 1.0 / (1.0 / 100.0 + N)
    m = v * y.sum()
    theta = m + math.sqrt(v) * rng.standard_normal(S)
    ll = -0.5 * math.log(2.0 * math.pi) - 0.5 * (y[None] - theta[:, None]) ** 2
    v_out = 1.0 / (1.0 / 100.0 + N - 1)
    m_out = v_out * (y.sum() - y)
    return ll, -0.5 * np.log(2.0 * math.pi * (1.0 + v_out)) - 0.5 * (y - m_out) ** 2 / (1.0 + v_out)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_exact_loo_of_a_conjugate_model(seed):
    ll, exact = _conjugate(seed)
    out = LR.psis_loo(ll)
    err = np.abs(out['elpd_loo'] - exact).max()
    print(f'seed {seed}: max |elpd_loo - exact| = {err:.4f}, lppd_0 - exact_0 = {out["lppd"][0] - exact[0]:.3f}')
    assert err <= 0.03
    assert out['lppd'][0] - exact[0] >= 0.5                       # the outlier: LOO is not LPPD
    assert not out['dropped'].any() and np.isfinite(out['khat']).all()


def _row(seed=3, S=500, scale=1.0):
    rng = np.random.default_rng(seed)
    return -0.5 * (scale * rng.standard_normal(S) + 1.0) ** 2 - 0.3


def _wide_row():
    """One draw 800 nats below the rest: every other ratio underflows, so x_q = 0 - exp(cut) is not positive."""
    l = _row(9)
    l[11] = -800.0
    return l


def _same(a, b, tol=1e-12, keys=KEYS + ('dropped',)):
    for x, y, k in zip(a, b, KEYS + ('dropped',)):
        if k in keys:
            assert (math.isnan(x) and math.isnan(y)) or abs(x - y) <= tol, (k, x, y)


def test_a_shift_moves_lppd_and_elpd_loo_only():
    l = _row()
    base, moved = LR.psis_row(l), LR.psis_row(l + 7.25)
    assert abs(moved[0] - base[0] - 7.25) <= 1e-12 and abs(moved[2] - base[2] - 7.25) <= 1e-12
    _same(base, moved, keys=('p_waic', 'khat', 'dropped'))
    assert math.isfinite(base[3])


def test_the_order_of_the_draws_does_not_matter():
    l = _row(4)
    _same(LR.psis_row(l), LR.psis_row(np.random.default_rng(5).permutation(l)))


def test_nonfinite_draws_are_left_out_and_counted():
    l = _row(6)
    with_bad = np.concatenate([l[:100], [np.nan, np.inf], l[100:], [-np.inf]])
    got = LR.psis_row(with_bad)
    assert got[4] == 3
    _same(got, LR.psis_row(l), keys=KEYS)
    assert all(math.isnan(v) for v in LR.psis_row(np.array([np.nan, 1.0, np.inf]))[:4])      # fewer than two kept
    assert LR.psis_row(np.array([np.nan, 1.0, np.inf]))[4] == 2


def test_a_constant_row():
    lppd, p_waic, elpd, khat, dropped = LR.psis_row(np.full(300, -1.75))
    assert math.isnan(khat) and abs(elpd + 1.75) <= 1e-12 and abs(lppd + 1.75) <= 1e-12 and p_waic == 0.0 and dropped == 0


def test_the_smallest_tail_that_is_fitted():
    assert LR.tail_length(20) == 4 and LR.tail_length(21) == 5
    l = _row(7, S=21)
    assert math.isnan(LR.psis_row(l[:20])[3]) and math.isfinite(LR.psis_row(l)[3])
    assert math.isfinite(LR.psis_row(l[:20])[2])


def test_a_spread_beyond_the_range_of_exp_is_not_fitted():
    l = _wide_row()
    assert l.max() - l.min() > 708.0
    lppd, p_waic, elpd, khat, _ = LR.psis_row(l)
    assert math.isnan(khat) and math.isfinite(elpd) and math.isfinite(lppd) and elpd < lppd


# ---------------------------------------------------------------- the torch restatement -----------------
def _invariance_inputs():
    rows = [_row(), _row() + 7.25, _row(4), np.full(500, -1.75), _wide_row(), _row(8, scale=3.0)]
    ll = np.stack(rows, axis=1)
    ll = np.concatenate([ll, np.full((2, ll.shape[1]), 0.5)])
    ll[500:, :5] = np.nan                                         # different kept counts in one call
    ll[500, 1] = np.inf
    ll[501, 2] = -np.inf
    ll[17, 0] = np.nan
    return ll


@pytest.mark.parametrize('name', ['invariances', 'S=20', 'S=21', 'conjugate', 'float32', 'r_eff'])
def test_torch_restatement_matches_the_reference(name):
    r_eff = 1.0
    if name == 'conjugate':
        ll = _conjugate(1)[0]
    elif name.startswith('S='):
        ll = np.stack([_row(7, S=21), _row(9, S=21)], axis=1)[:int(name[2:])]
    else:
        ll = _invariance_inputs()
    if name == 'float32':
        ll = ll.astype(np.float32)
    if name == 'r_eff':
        r_eff = 0.37
    ref = LR.psis_loo(ll, r_eff)
    got = M.psis_loo(torch.from_numpy(ll), r_eff)
    assert got['dropped'].dtype == torch.int32 and got['dropped'].tolist() == ref['dropped'].tolist()
    for k in KEYS:
        g = got[k].numpy()
        assert got[k].dtype == torch.float64 and (np.isnan(g) == np.isnan(ref[k])).all(), (name, k)
        fin = ~np.isnan(g)
        err = np.abs(g[fin] - ref[k][fin]).max() if fin.any() else 0.0
        assert err <= 1e-10, (name, k, err)
    assert np.isnan(ref['khat']).all() == (name == 'S=20')
    if name == 'invariances':                                      # leading axes are draw axes; fewer than two kept draws
        again = M.psis_loo(torch.from_numpy(ll.reshape(2, 251, -1)))
        assert all(torch.equal(torch.nan_to_num(again[k], nan=-7.0), torch.nan_to_num(got[k], nan=-7.0)) for k in KEYS)
        ll2 = ll.copy()
        ll2[1:, 3] = np.nan
        dead = M.psis_loo(torch.from_numpy(ll2))
        assert all(torch.isnan(dead[k][3]) for k in KEYS) and int(dead['dropped'][3]) == 501
    with pytest.raises(ValueError):
        M.psis_loo(torch.from_numpy(ll), r_eff=0.0)


def test_loo_summary_by_hand():
    rows = {'lppd': np.array([-1.0, -2.0, -0.5, -4.0]), 'p_waic': np.array([0.1, 0.5, 0.05, 0.4]),
            'elpd_loo': np.array([-1.25, -2.75, -0.5, -5.0]), 'khat': np.array([0.2, 0.9, np.nan, 0.7])}
    s = M.loo_summary({k: torch.from_numpy(v) for k, v in rows.items()})
    assert s['elpd_loo'] == -9.5 and s['lppd_sum'] == -7.5 and s['p_loo'] == pytest.approx(2.0, abs=1e-15)
    assert s['p_waic'] == pytest.approx(1.05, abs=1e-15) and s['elpd_waic'] == pytest.approx(-8.55, abs=1e-14)
    # sqrt(N var) with the divisor N - 1: elpd_loo has mean -2.375 and squared deviations 1.265625 + 0.140625 + 3.515625 + 6.890625
    assert s['se_elpd_loo'] == pytest.approx(math.sqrt(4 * 11.8125 / 3), rel=1e-14)
    waic = [-1.1, -2.5, -0.55, -4.4]
    mean = sum(waic) / 4
    assert s['se_elpd_waic'] == pytest.approx(math.sqrt(4 * sum((w - mean) ** 2 for w in waic) / 3), rel=1e-13)
    assert (s['n_khat_above_0.7'], s['n_khat_nofit'], s['n_p_waic_above_0.4']) == (1, 1, 1)
    assert s == M.loo_summary(rows)                                # arrays or tensors


# ---------------------------------------------------------------- C ABI and CLI -----------------
NEW = ('mile_psis_loo', 'mile_loo_stream', 'mile_loo_stream_workspace')


def test_library_exports_the_three_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    p, i64, f64 = C.c_void_p, C.c_int64, C.c_double
    assert _lib.SIGNATURES['mile_psis_loo'] == (C.c_int32, [p, i64, i64, f64, p, p, p, p, p, p])
    assert _lib.SIGNATURES['mile_loo_stream'] == (C.c_int32, [p, p, i64, p, p, i64, f64, p, p, p, p, p, i64, i64, p])
    assert _lib.SIGNATURES['mile_loo_stream_workspace'] == (i64, [p, i64, i64])
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10         # new symbols under the same ABI
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert '#define MILE_ABI_VERSION 10' in header
    assert ('int32_t mile_psis_loo(const float *loglik, int64_t S, int64_t N, double r_eff, double *lppd, double *p_waic, '
            'double *elpd_loo, double *khat, int32_t *dropped, void *stream);') in header
    assert ('int32_t mile_loo_stream(mile_sampler *s, const float *theta, int64_t S, const void *X, const void *y, int64_t N, '
            'double r_eff, double *lppd, double *p_waic, double *elpd_loo, double *khat, int32_t *dropped, '
            'int64_t max_draws_per_pass, int64_t max_rows_per_tile, void *stream);') in header
    assert 'int64_t mile_loo_stream_workspace(const mile_sampler *s, int64_t S, int64_t N);' in header


BAD_R_EFF = [('r_eff = 0', 0.0), ('r_eff < 0', -1.0), ('r_eff NaN', float('nan')), ('r_eff inf', float('inf'))]


def test_psis_loo_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)

    def call(ll=p, S=8, N=4, r_eff=1.0, outs=(p, p, p, p, p)):
        return lib.mile_psis_loo(ll, S, N, r_eff, *outs, None)
    cases = [('null loglik', dict(ll=None), 'null'), ('S = 1', dict(S=1), 'S out of range'), ('S = 0', dict(S=0), 'S out of range'),
             ('S < 0', dict(S=-4), 'S out of range'), ('S = 2^20 + 1', dict(S=(1 << 20) + 1), 'S out of range'),
             ('N = 0', dict(N=0), 'N out of range'), ('N = 2^30', dict(N=1 << 30), 'N out of range'),
             ('no output', dict(outs=(None,) * 5), 'no output'),
             ('a tail beyond the LDS sort', dict(S=1 << 20, r_eff=0.25), 'tail')]
    cases += [(tag, dict(r_eff=v), 'r_eff') for tag, v in BAD_R_EFF]
    for tag, kw, text in cases:
        assert call(**kw) == -1, tag
        msg = lib.mile_last_error().decode()
        assert 'mile_psis_loo' in msg and text in msg, (tag, msg)


def test_loo_stream_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 2))), 0, C.byref(h)) == 0
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)

    def call(hh, theta=p, S=8, X=p, y=p, N=4, r_eff=1.0, outs=(p, p, p, p, p), passes=0, tile=0):
        return lib.mile_loo_stream(hh, theta, S, X, y, N, r_eff, *outs, passes, tile, None)
    try:
        cases = [('null handle', None, {}, 'null'), ('null theta', h, dict(theta=None), 'null'), ('null X', h, dict(X=None), 'null'),
                 ('null y', h, dict(y=None), 'null'), ('S = 1', h, dict(S=1), 'S out of range (2 .. 2^20)'),
                 ('S = 0', h, dict(S=0), 'S out of range (2 .. 2^20)'), ('S = 2^20 + 1', h, dict(S=(1 << 20) + 1), 'S out of range'),
                 ('N = 0', h, dict(N=0), 'N out of range'), ('N = 2^30', h, dict(N=1 << 30), 'N out of range'),
                 ('no output', h, dict(outs=(None,) * 5), 'no output'), ('passes < 0', h, dict(passes=-1), 'max_draws_per_pass'),
                 ('tile < 0', h, dict(tile=-1), 'max_rows_per_tile'),
                 ('a tail beyond the LDS sort', h, dict(S=1 << 20, r_eff=0.25), 'tail')]
        cases += [(tag, h, dict(r_eff=v), 'r_eff') for tag, v in BAD_R_EFF]
        for tag, hh, kw, text in cases:
            assert call(hh, **kw) == -1, tag
            msg = lib.mile_last_error().decode()
            assert 'mile_loo_stream' in msg and text in msg, (tag, msg)
        assert lib.mile_loo_stream_workspace(h, 12000, 1052) >= 2 * 12000 * 1052 * 4
        assert lib.mile_loo_stream_workspace(h, 1 << 20, 1052) <= (256 << 20) + 512       # tiles: within the budget
        for S, N in ((1, 4), (4, 0), ((1 << 20) + 1, 4), (4, 1 << 30)):
            assert lib.mile_loo_stream_workspace(h, S, N) == -1
        assert lib.mile_loo_stream_workspace(None, 4, 4) == -1
    finally:
        lib.mile_destroy(h)
    # frozen tables not set: a state error, after the argument checks
    assert lib.mile_create(C.byref(_attn_pre_cspec()), 0, C.byref(h)) == 0, lib.mile_last_error()
    try:
        assert call(h, r_eff=0.0) == -1 and call(h) == -2
    finally:
        lib.mile_destroy(h)


def test_evaluate_parser_accepts_loo():
    import evaluate as EV
    ap = EV.build_parser()
    assert ap.parse_args(['-e', 'x']).loo is False                 # opt-in
    args = ap.parse_args(['-e', 'x', '--loo', '--split', 'test'])
    assert args.loo is True and args.loo_r_eff == 1.0
    assert 'TRAIN split' in ' '.join(ap.format_help().split())
    ll, _ = _conjugate(0)
    keys, arrays = EV.loo_metrics(M.psis_loo(torch.from_numpy(ll)))
    assert sorted(arrays) == ['dropped', 'elpd_loo', 'khat', 'lppd', 'p_waic'] and arrays['khat'].shape == (20,)
    assert sorted(keys) == sorted(['loo_' + k for k in M.loo_summary(arrays)] + ['loo_n_points', 'loo_dropped'])
    assert keys['loo_n_points'] == 20 and keys['loo_elpd_loo'] < keys['loo_lppd_sum'] and keys['loo_p_loo'] > 0

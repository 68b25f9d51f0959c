"""PSIS-LOO expectations on the host: the NumPy restatement of tests/lxp_ref.py against itself and against tests/loo_ref.py,
metrics.psis_expect_dense against the restatement, the three new symbols and their refusals (which need no GPU),
metrics.loo_predict_summary on hand-made rows, and evaluate.py's --loo-predict flag.

Bounds.  The restatement against itself: sum w = 1 and log sum w e^l = elpd_loo to 1e-12 (a handful of fp64 roundings per
draw, S <= 1000); a permutation of the draws moves expect by the rounding of a sum in another order, 1e-12.
psis_expect_dense and the restatement are the same fp64 formulas in another summation order: 1e-9 max(1, |value|), the
project's bound for fixed-order fp64 sums (tests/test_gpu_loo.py)."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.special import logsumexp

from mile_amd import metrics as M
from tests import loo_ref as LR
from tests import lxp_ref as XR
from tests.test_gpu_loo import SEVEN, _tensor

ROOT = Path(__file__).resolve().parent.parent
SIZES = [2, 20, 21, 26, 70, 1000]


def _values(ll, seed):
    """Q = 3 columns: standard normal, l itself, the constant 1 (a dropped draw's l column is non-finite: never read)."""
    S, N = ll.shape
    v = np.empty((S, N, 3), dtype=np.float32)
    v[..., 0] = np.random.default_rng(seed).standard_normal((S, N))
    v[..., 1] = ll
    v[..., 2] = 1.0
    return v


# ---------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize('S', SIZES)
def test_restatement_weights_sum_to_one_and_give_loo_ref_s_elpd(S):
    ll = _tensor(S, SEVEN, 100 + S)
    for n, name in enumerate(SEVEN):
        w, khat, elpd, dropped = XR.weights_row(ll[:, n])
        ref = LR.psis_row(ll[:, n])
        keep = np.isfinite(ll[:, n])
        assert dropped == ref[4] and (w[~keep] == 0.0).all(), name
        assert abs(w.sum() - 1.0) <= 1e-12, (name, w.sum())
        assert abs(logsumexp(ll[keep, n].astype(np.float64), b=w[keep]) - ref[2]) <= 1e-12 * max(1.0, abs(ref[2])), name
        assert elpd == ref[2] and (khat == ref[3] or (khat != khat and ref[3] != ref[3])), name
        _, first, inv = np.unique(ll[keep, n].view(np.uint32), return_index=True, return_inverse=True)
        assert (w[keep] == w[keep][first][inv.reshape(-1)]).all(), name              # equal l bits, equal weight bits


@pytest.mark.parametrize('S', [26, 70, 1000])
def test_restatement_does_not_see_a_permutation_of_the_draws(S):
    ll = _tensor(S, SEVEN, 100 + S)
    v = _values(ll, S)
    a = XR.expect(ll, v)
    perm = np.random.default_rng(S).permutation(S)
    b = XR.expect(np.ascontiguousarray(ll[perm]), np.ascontiguousarray(v[perm]))
    for k in ('expect', 'posterior'):
        assert np.allclose(a[k], b[k], rtol=0.0, atol=1e-12, equal_nan=True), k
    for k in ('ess_w', 'elpd_loo'):                                                    # (ess_w is of the order of S)
        assert (np.abs(a[k] - b[k]) <= 1e-12 * np.maximum(1.0, np.abs(a[k]))).all(), k
    assert np.allclose(a['weights'][:, perm], b['weights'], rtol=0.0, atol=1e-15)


def test_restatement_on_a_constant_row():
    S = 70
    ll = _tensor(S, ('constant',), 1)
    res = XR.expect(ll, _values(ll, 2))
    assert np.allclose(res['weights'], 1.0 / S, rtol=0.0, atol=1e-15)
    assert np.allclose(res['expect'], res['posterior'], rtol=0.0, atol=1e-12) and abs(res['ess_w'][0] - S) <= 1e-9


# ---------------------------------------------------------------- the torch form against the restatement
KEYS = ('expect', 'posterior', 'ess_w', 'khat', 'elpd_loo', 'weights')


def check_against_ref(tag, got, ref, keys=KEYS, bound=1e-9):
    """got (numpy arrays) against the restatement: equal dropped, equal NaN patterns, |got - ref| <= bound max(1, |ref|)."""
    assert got['dropped'].tolist() == ref['dropped'].tolist(), (tag, got['dropped'], ref['dropped'])
    worst = {}
    for k in keys:
        g, r = np.asarray(got[k], dtype=np.float64), ref[k]
        assert g.shape == r.shape, (tag, k, g.shape, r.shape)
        assert (np.isnan(g) == np.isnan(r)).all(), (tag, k, 'NaN pattern', g, r)
        fin = ~np.isnan(r)
        with np.errstate(invalid='ignore'):
            rel = np.abs(g[fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        worst[k] = float(rel.max()) if fin.any() else 0.0
    print(f'{tag}: max |out - ref| / max(1, |ref|) = ' + ', '.join(f'{k} {v:.2e}' for k, v in worst.items()))
    for k in keys:
        assert worst[k] <= bound, (tag, k, worst[k])


@pytest.mark.parametrize('S', SIZES)
def test_psis_expect_dense_is_the_restatement(S):
    ll = _tensor(S, SEVEN, 100 + S)
    v = _values(ll, S)
    got = M.psis_expect_dense(torch.from_numpy(ll), torch.from_numpy(v), return_weights=True)
    check_against_ref(f'dense S={S}', {k: t.numpy() for k, t in got.items()}, XR.expect(ll, v))


def test_psis_expect_dense_on_rows_with_fewer_than_two_finite_draws():
    ll = _tensor(26, ('light', 'light', 'heavy0.6', 'light'), 7)
    ll[:, 1] = np.nan
    ll[1:, 3] = np.inf
    v = _values(ll, 3)
    got = {k: t.numpy() for k, t in M.psis_expect_dense(torch.from_numpy(ll), torch.from_numpy(v), return_weights=True).items()}
    check_against_ref('too few', got, XR.expect(ll, v))
    assert got['dropped'].tolist() == [0, 26, 0, 25] and np.isnan(got['expect'][[1, 3]]).all() and np.isnan(got['weights'][[1, 3]]).all()


def test_predictive_columns_are_the_restatement_s():
    rng = np.random.default_rng(4)
    raw = rng.standard_normal((9, 5, 2)).astype(np.float32)
    raw[0, 0, 1], raw[1, 1, 1], raw[2, 2, 1] = -40.0, 40.0, np.nan                    # sigma clipped below, above; NaN
    y = rng.standard_normal(5).astype(np.float32)
    a, b = M.loo_predict_columns(torch.from_numpy(raw), torch.from_numpy(y), 'regr').numpy(), XR.columns(raw, y, 'regr')
    assert a.shape == (9, 5, 4) and np.allclose(a, b, rtol=1e-14, atol=0.0, equal_nan=True)
    assert a[0, 0, 2] == 1e-12 and a[1, 1, 2] == 1e12 and np.isnan(a[2, 2, 2:]).all() and ((a[..., 3] >= 0) | np.isnan(a[..., 3])).all()
    z = (5.0 * rng.standard_normal((9, 5, 7))).astype(np.float32)
    a, b = M.loo_predict_columns(torch.from_numpy(z), None, 'classification').numpy(), XR.columns(z, None, 'classification')
    assert np.allclose(a, b, rtol=1e-14, atol=0.0) and np.allclose(a.sum(-1), 1.0, rtol=0.0, atol=1e-14)


# ---------------------------------------------------------------- C ABI
def test_library_exports_the_three_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    want = {'mile_psis_expect': (i32, [p, p, i64, i64, i32, f64, p, p, p, p, p, p, p, p]),
            'mile_loo_predict_stream': (i32, [p, p, i64, p, p, i64, f64, p, p, p, p, p, p, i64, i64, p]),
            'mile_loo_predict_stream_workspace': (i64, [p, i64, i64])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name), name
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_psis_expect(const float *loglik, const float *values, int64_t S, int64_t N, int32_t Q, double r_eff, '
            'double *expect, double *posterior, double *ess_w, double *khat, double *elpd_loo, int32_t *dropped, double *weights, '
            'void *stream);') in header
    assert 'int64_t mile_loo_predict_stream_workspace(const mile_sampler *s, int64_t S, int64_t N);' in header


def test_psis_expect_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)

    def call(ll=p, values=p, S=8, N=4, Q=3, r_eff=1.0, outs=(p,) * 7):
        return lib.mile_psis_expect(ll, values, S, N, Q, r_eff, *outs, None)
    nul = None
    for tag, kw, text in [('null loglik', dict(ll=None), 'null loglik'), ('S = 1', dict(S=1), 'S out of range (2 .. 2^20)'),
                          ('S = 2^20 + 1', dict(S=(1 << 20) + 1), 'S out of range'), ('N = 0', dict(N=0), 'N out of range'),
                          ('Q = 0', dict(Q=0), 'Q out of range (1 .. 64)'), ('Q = 65', dict(Q=65), 'Q out of range (1 .. 64)'),
                          ('no output', dict(outs=(None,) * 7), 'no output'), ('r_eff = 0', dict(r_eff=0.0), 'r_eff'),
                          ('r_eff NaN', dict(r_eff=float('nan')), 'r_eff'), ('the tail', dict(S=1 << 20, r_eff=0.5), 'tail is longer'),
                          ('expect without values', dict(values=None, outs=(p, nul, nul, nul, nul, nul, nul)), 'need values'),
                          ('posterior without values', dict(values=None, outs=(nul, p, nul, nul, nul, nul, nul)), 'need values')]:
        assert call(**kw) == -1, tag
        msg = lib.mile_last_error().decode()
        assert 'mile_psis_expect' in msg and text in msg, (tag, msg)


def test_loo_predict_stream_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    from tests.test_predict_host import _fcn_cspec
    lib = _lib.load_library()
    h, h65 = C.c_void_p(), C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 2))), 0, C.byref(h)) == 0
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 65), task=1)), 0, C.byref(h65)) == 0
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)

    def call(hh, theta=p, S=8, X=p, y=p, N=4, r_eff=1.0, outs=(p,) * 6, passes=0, tile=0):
        return lib.mile_loo_predict_stream(hh, theta, S, X, y, N, r_eff, *outs, passes, tile, None)
    try:
        for tag, hh, kw, text in [('null handle', None, {}, 'null'), ('null theta', h, dict(theta=None), 'null'), ('null X', h, dict(X=None), 'null'),
                                  ('null y', h, dict(y=None), 'null'), ('S = 1', h, dict(S=1), 'S out of range (2 .. 2^20)'),
                                  ('N = 0', h, dict(N=0), 'N out of range'), ('no output', h, dict(outs=(None,) * 6), 'no output'),
                                  ('r_eff = 0', h, dict(r_eff=0.0), 'r_eff'), ('passes < 0', h, dict(passes=-1), 'max_draws_per_pass'),
                                  ('tile < 0', h, dict(tile=-1), 'max_rows_per_tile'), ('K = 65', h65, {}, 'more than 64 classes')]:
            assert call(hh, **kw) == -1, tag
            msg = lib.mile_last_error().decode()
            assert 'mile_loo_predict_stream' in msg and text in msg, (tag, msg)
        # per (draw, row): the forward's 8 bytes, the packed l 4, the weight 8; per row 1000 / 32 -> 32 runs of 4 columns' two sums and a count
        r256 = lambda b: (b + 255) // 256 * 256
        S, N = 1000, 1052
        assert lib.mile_loo_predict_stream_workspace(h, S, N) == r256(S * N * 8) + r256(S * N * 4) + r256(S * N * 8) + r256(32 * N * 4 * 16) + r256(32 * N * 4)
        assert lib.mile_loo_predict_stream_workspace(h, S, N) > lib.mile_loo_stream_workspace(h, S, N)
        for hh, S, N in ((None, 8, 4), (h, 1, 4), (h, 8, 0), (h65, 8, 4)):
            assert lib.mile_loo_predict_stream_workspace(hh, S, N) == -1
    finally:
        for hh in (h, h65):
            lib.mile_destroy(hh)


# ---------------------------------------------------------------- the summary
def test_summary_of_hand_made_regression_rows():
    y = np.array([0.0, 1.0, 2.0, 3.0])
    mean = np.array([0.5, 1.0, 1.5, 3.0])
    expect = np.stack([mean, mean ** 2 + 0.25, np.full(4, 0.5), np.array([0.5, 0.1, 0.9, 0.99])], axis=1)
    post = np.stack([y, y ** 2, np.full(4, 0.25), np.full(4, 0.5)], axis=1)
    rows = {'expect': expect, 'posterior': post, 'khat': np.array([0.1, 0.8, np.nan, 0.2]), 'ess_w': np.array([10.0, 2.0, 4.0, 8.0]),
            'elpd_loo': -np.ones(4), 'dropped': np.array([0, 1, 0, 2], dtype=np.int32)}
    s = M.loo_predict_summary(rows, y, 'regr', coverages=(0.5, 0.9))
    assert abs(s['rmse'] - np.sqrt(0.125)) <= 1e-15 and s['rmse_insample'] == 0.0
    assert abs(s['r2'] - (1.0 - 0.5 / 5.0)) <= 1e-15 and s['r2_insample'] == 1.0
    assert abs(s['var_epistemic'] - 0.25) <= 1e-15 and s['var_aleatoric'] == 0.5 and s['var_epistemic_insample'] == 0.0
    assert s['coverage_0.5'] == 0.25 and s['coverage_0.9'] == 0.75 and s['coverage_0.5_insample'] == 1.0   # |pit - 1/2| <= c / 2
    assert abs(s["cal_error"] - np.sqrt((0.25 ** 2 + 0.15 ** 2) / 2)) <= 1e-12
    assert abs(s['khat_above_0.7_share'] - 1.0 / 3.0) <= 1e-15 and s['khat_nofit'] == 1
    assert s['ess_w_min'] == 2.0 and s['ess_w_median'] in (4.0, 6.0, 8.0) and s['n_rows'] == 4 and s['dropped'] == 3 and s['n_rows_nan'] == 0


def test_summary_of_hand_made_classification_rows():
    y = np.array([0, 1, 2, 1])
    expect = np.array([[0.7, 0.2, 0.1], [0.1, 0.8, 0.1], [0.5, 0.3, 0.2], [0.3, 0.6, 0.1]])
    post = np.eye(3)[y] * 0.9 + 0.1 / 3
    rows = {'expect': expect, 'posterior': post, 'khat': np.array([0.1, 0.2, 0.3, 0.9]), 'ess_w': np.array([5.0, 6.0, 7.0, 8.0]),
            'elpd_loo': np.log(np.array([0.7, 0.8, 0.2, 0.6])), 'dropped': np.zeros(4, dtype=np.int32)}
    s = M.loo_predict_summary(rows, y, 'classification', n_bins=10)
    assert s['accuracy'] == 0.75 and s['accuracy_insample'] == 1.0
    assert abs(s['nll'] + np.log(np.array([0.7, 0.8, 0.2, 0.6])).mean()) <= 1e-15
    brier = ((expect - np.eye(3)[y]) ** 2).sum(axis=1).mean()
    assert abs(s['brier'] - brier) <= 1e-15 and s['brier_insample'] < s['brier']
    assert 0.0 <= s['ece'] <= s['mce'] <= 1.0 and s['khat_above_0.7_share'] == 0.25 and s['ess_w_min'] == 5.0


def test_evaluate_help_lists_the_flag():
    res = subprocess.run([sys.executable, str(ROOT / 'evaluate.py'), '--help'], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr
    assert '--loo-predict' in res.stdout and 'loo_predict.npz' in ' '.join(res.stdout.split())

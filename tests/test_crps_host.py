"""The host side of the CRPS of the predictive mixture (no GPU): metrics.mixture_crps_dense against the NumPy fp64 definitions
of tests/crps_ref.py, the single-Normal closed form, crps_summary's arithmetic, the thinning rule, the weight checks of the
Python layer, the C ABI's refusals (every one is decided before anything touches a device) and evaluate.py's arguments.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from mile_amd import metrics as M
from tests import crps_ref as CR

ROOT = Path(__file__).resolve().parents[1]


def _raw(Cn, S, N, seed):
    rng = np.random.default_rng(seed)
    centre, spread = rng.standard_normal(N) * 3.0, np.exp(rng.uniform(-3.0, 1.0, N))
    mu = centre + spread * rng.standard_normal((Cn, S, N)) + 0.5 * spread * rng.standard_normal((Cn, 1, N))
    ls = rng.uniform(-2.0, 1.0, N) + 0.5 * rng.standard_normal((Cn, S, N))
    raw = np.stack([mu, ls], axis=-1).astype(np.float32)
    y = (raw[rng.integers(0, Cn, N), rng.integers(0, S, N), np.arange(N), 0] + rng.standard_normal(N)).astype(np.float32)
    return raw, y


def _simplex(rng, n_w, Cn):
    w = rng.dirichlet(np.ones(Cn), size=n_w)
    return w / w.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('Cn,S,N', [(1, 1, 9), (3, 5, 7), (2, 257, 5), (5, 40, 11)])
def test_dense_form_is_the_definition(Cn, S, N):
    raw, y = _raw(Cn, S, N, 1)
    W = np.concatenate([_simplex(np.random.default_rng(2), 2, Cn), np.eye(Cn)[:1]])
    ref = CR.crps(raw, y, W)
    got = M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y), W, outputs=M.CRPS_OUTPUTS, budget=1 << 12)
    scale = {'crps_chain': ref['t1_chain'] + 0.5 * ref['t2_chain'], 'spread_chain': ref['t2_chain'], 'crps_mix': ref['t1'] + 0.5 * ref['t2'],
             'spread_mix': ref['t2'], 'gram': np.abs(ref['gram'])}
    for k, s in scale.items():
        assert got[k].dtype == torch.float64 and got[k].shape == ref[k].shape, k
        assert (np.abs(got[k].numpy() - ref[k]) <= 1e-12 * s).all(), k
    assert got['dropped'].dtype == torch.int32 and not got['dropped'].any()
    # a vertex is the chain alone; the pooled ensemble of chains of equal length is the uniform mixture
    np.testing.assert_allclose(got['crps_mix'][3].numpy(), got['crps_chain'][0].numpy(), rtol=1e-12, atol=0)
    assert (got['crps_mix'].numpy() >= 0).all() and torch.equal(got['gram'], got['gram'].transpose(1, 2))


def test_one_draw_is_the_single_normal_closed_form():
    raw, y = _raw(1, 1, 9, 3)
    got = M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y))
    exact = CR.single_normal_crps(raw[0, 0, :, 0].astype(np.float64), np.exp(raw[0, 0, :, 1].astype(np.float64)), y)
    np.testing.assert_allclose(got['crps_mix'][0].numpy(), exact, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got['crps_chain'][0].numpy(), exact, rtol=1e-12, atol=0)


def test_nonfinite_draws_and_empty_chains():
    raw, y = _raw(3, 6, 5, 4)
    raw[0, 2, 0, 0] = np.nan
    raw[1, :, 1, 1] = np.inf                                         # chain 1 wholly dropped on row 1
    raw[:, :, 2, 0] = -np.inf                                        # nothing kept on row 2
    W = np.array([[0.5, 0.0, 0.5], [0.2, 0.3, 0.5]])
    ref = CR.crps(raw, y, W)
    got = {k: v.numpy() for k, v in M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y), W, outputs=M.CRPS_OUTPUTS).items()}
    assert got['dropped'].tolist() == ref['dropped'].tolist() == [[1, 0, 6, 0, 0], [0, 6, 6, 0, 0], [0, 0, 6, 0, 0]]
    for k in ('crps_chain', 'spread_chain', 'crps_mix', 'spread_mix', 'gram'):
        assert (np.isnan(got[k]) == np.isnan(ref[k])).all(), k
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-12, atol=0, equal_nan=True)
    assert np.isnan(got['crps_chain'][1, 1]) and np.isfinite(got['crps_mix'][0, 1])      # the pooled weights skip the empty chain
    assert np.isfinite(got['crps_mix'][1, 1]) and np.isnan(got['crps_mix'][2, 1])        # w_1 = 0 skips it too, w_1 > 0 does not
    assert np.isnan(got['crps_mix'][:, 2]).all() and np.isnan(got['crps_chain'][:, 2]).all()
    np.testing.assert_allclose(ref['pooled'][1], [0.5, 0.0, 0.5])
    np.testing.assert_allclose(ref['pooled'][0], [5 / 17, 6 / 17, 6 / 17])


def test_summary_arithmetic():
    rows = {'crps_mix': np.array([[1.0, 3.0, np.nan], [2.0, 2.0, 2.0]]), 'spread_mix': np.array([[0.5, 0.5, np.nan], [1.0, 3.0, 5.0]]),
            'crps_chain': np.array([[2.0, 4.0, 6.0], [4.0, 4.0, 1.0]]), 'spread_chain': np.array([[1.0, 1.0, 1.0], [0.0, 2.0, 4.0]]),
            'gram': np.array([[[2.0, 5.0], [5.0, 4.0]], [[2.0, 3.0], [3.0, 4.0]], [[np.nan, np.nan], [np.nan, 1.0]]])}
    s = M.crps_summary(rows, weights=[[0.5, 0.5]])
    assert s['crps'] == 2.0 and s['crps_se'] == pytest.approx(np.sqrt(2.0) / np.sqrt(2.0)) and s['rows_nan'] == 1 and s['n_rows'] == 3
    assert s['spread'] == 0.5 and s['spread_se'] == 0.0
    assert s['mix_crps'] == [2.0] and s['mix_crps_se'] == [0.0] and s['mix_spread'] == [3.0]
    assert s['mix_spread_se'] == [pytest.approx(2.0 / np.sqrt(3.0))]
    assert s['chain_crps'] == [4.0, 3.0] and s['chain_spread'] == [1.0, 2.0]
    assert s['chain_crps_se'] == [pytest.approx(2.0 / np.sqrt(3.0)), pytest.approx(np.sqrt(3.0) / np.sqrt(3.0))]
    assert s['mix_pooling_gain'] == [pytest.approx((1.0 + 2.0 + 1.5) / 3.0)]
    assert s['energy_distance'] == [[0.0, 2.0], [2.0, 0.0]]           # rows 0 and 1: 10 - 6 = 4 and 6 - 6 = 0; row 2 is not finite
    assert 'mix_pooling_gain' not in M.crps_summary(rows) and 'energy_distance' not in M.crps_summary({k: rows[k] for k in ('crps_mix',)})


def test_thinning_rule():
    assert M.crps_thin_stride(12, 1000, 131072) == 1 and M.crps_thin_stride(128, 1000, 131072) == 1
    assert M.crps_thin_stride(128, 1024, 131072) == 1 and M.crps_thin_stride(128, 1025, 131072) == 2
    assert M.crps_thin_stride(4, 30, 50) == 3 and M.crps_thin_stride(4, 30, 1) == 120
    S, k = 30, M.crps_thin_stride(4, 30, 50)
    assert list(range(S))[::k] == [j for j in range(S) if j % k == 0] and 4 * len(range(0, S, k)) <= 50
    with pytest.raises(ValueError):
        M.crps_thin_stride(4, 30, 0)


def test_python_layer_refuses_bad_weights():
    assert M.crps_weights(None, 3).shape == (0, 3)
    assert M.crps_weights([0.25, 0.25, 0.5], 3).shape == (1, 3) and M.crps_weights(np.eye(3), 3).dtype == torch.float64
    for tag, w in [('negative', [0.5, 0.75, -0.25]), ('nan', [0.5, float('nan'), 0.5]), ('inf', [float('inf'), 0.0, 0.0]),
                   ('sum', [0.5, 0.25, 0.25 + 1e-8]), ('length', [0.5, 0.5]), ('nine vectors', np.full((9, 3), 1.0 / 3.0)),
                   ('rank', np.full((1, 1, 3), 1.0 / 3.0))]:
        with pytest.raises(ValueError):
            M.crps_weights(w, 3)
        raw, y = _raw(3, 2, 4, 5)
        with pytest.raises(ValueError):
            M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y), w)
    assert M.crps_weights([0.5, 0.25, 0.25 + 5e-10], 3).shape == (1, 3)
    raw, y = _raw(3, 2, 4, 5)
    with pytest.raises(ValueError):
        M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y), outputs=('crps',))
    with pytest.raises(ValueError):
        M.mixture_crps_dense(torch.from_numpy(raw[0]), torch.from_numpy(y))


# ---------------------------------------------------------------- C ABI -------------------------
def test_library_exports_the_crps_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    p, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    want = {'mile_mixture_crps': (i32, [p, i32, i64, i64, p, p, i32, p, p, p, p, p, p, i64, p]),
            'mile_crps_stream': (i32, [p, p, i32, i64, p, p, i64, p, i32, p, p, p, p, p, p, i64, i64, p]),
            'mile_crps_stream_workspace': (i64, [p, i32, i64, i64])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name), name
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_mixture_crps(const float *raw, int32_t C, int64_t S, int64_t N, const float *y, const double *weights, '
            'int32_t n_w, double *crps_chain, double *spread_chain, double *crps_mix, double *spread_mix, double *gram, '
            'int32_t *dropped, int64_t max_rows_per_tile, void *stream);') in header
    assert 'int64_t mile_crps_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);' in header


def _weights(rows):
    flat = [v for r in rows for v in r]
    return (C.c_double * len(flat))(*flat)


BAD_SHARED = [('C = 0', dict(Cn=0), 'C out of range (1 .. 1024)'), ('C = 1025', dict(Cn=1025), 'C out of range'), ('S = 0', dict(S=0), 'S < 1'),
              ('C * S > 2^20', dict(Cn=1024, S=1025), 'C * S out of range'), ('S > 2^20', dict(Cn=1, S=(1 << 20) + 1), 'C * S out of range'),
              ('N = 0', dict(N=0), 'N out of range'), ('N = 2^30', dict(N=1 << 30), 'N out of range'),
              ('no output', dict(outs=(None,) * 6), 'no output'), ('n_w = -1', dict(n_w=-1), 'n_w out of range (0 .. 8)'),
              ('n_w = 9', dict(n_w=9), 'n_w out of range'), ('n_w without weights', dict(n_w=1, w=None), 'without weights'),
              ('negative weight', dict(n_w=1, w=_weights([[0.5, 0.75, -0.25]])), 'finite and >= 0'),
              ('nan weight', dict(n_w=1, w=_weights([[0.5, float('nan'), 0.5]])), 'finite and >= 0'),
              ('inf weight', dict(n_w=2, w=_weights([[0.5, 0.25, 0.25], [float('inf'), 0.0, 0.0]])), 'finite and >= 0'),
              ('sum off by 1e-8', dict(n_w=1, w=_weights([[0.5, 0.25, 0.25 + 1e-8]])), 'sum to 1'),
              ('tile < 0', dict(tile=-1), 'max_rows_per_tile')]


def test_mixture_crps_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(raw=p, Cn=3, S=8, N=4, y=p, w=None, n_w=0, outs=(p,) * 6, tile=0):
        return lib.mile_mixture_crps(raw, Cn, S, N, y, w, n_w, *outs, tile, None)
    for tag, kw, text in [('null raw', dict(raw=None), 'null'), ('null y', dict(y=None), 'null')] + BAD_SHARED:
        assert call(**kw) == -1, tag
        msg = lib.mile_last_error().decode()
        assert 'mile_mixture_crps' in msg and text in msg, (tag, msg)


def test_crps_stream_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    from tests.test_predict_host import _fcn_cspec
    lib = _lib.load_library()
    h, hc = C.c_void_p(), C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 2))), 0, C.byref(h)) == 0
    assert lib.mile_create(C.byref(_fcn_cspec(7, (40, 40, 3), task=1)), 0, C.byref(hc)) == 0
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)

    def call(hh, theta=p, Cn=3, S=8, X=p, y=p, N=4, w=None, n_w=0, outs=(p,) * 6, passes=0, tile=0):
        return lib.mile_crps_stream(hh, theta, Cn, S, X, y, N, w, n_w, *outs, passes, tile, None)
    try:
        cases = [('null handle', None, {}, 'null'), ('null theta', h, dict(theta=None), 'null'), ('null X', h, dict(X=None), 'null'),
                 ('null y', h, dict(y=None), 'null'), ('passes < 0', h, dict(passes=-1), 'max_draws_per_pass'),
                 ('classification', hc, {}, 'regression')] + [(tag, h, kw, text) for tag, kw, text in BAD_SHARED]
        for tag, hh, kw, text in cases:
            assert call(hh, **kw) == -1, tag
            msg = lib.mile_last_error().decode()
            assert 'mile_crps_stream' in msg and text in msg, (tag, msg)
        assert lib.mile_crps_stream_workspace(h, 12, 1000, 301) > 12 * 1000 * 16
        for Cn, S, N in ((0, 8, 4), (1025, 8, 4), (3, 0, 4), (1024, 1025, 4), (3, 8, 0), (3, 8, 1 << 30)):
            assert lib.mile_crps_stream_workspace(h, Cn, S, N) == -1
        assert lib.mile_crps_stream_workspace(None, 3, 8, 4) == -1
    finally:
        lib.mile_destroy(h)
        lib.mile_destroy(hc)


# ---------------------------------------------------------------- CLI ---------------------------
def test_evaluate_parser_accepts_crps():
    import evaluate as EV
    ap = EV.build_parser()
    args = ap.parse_args(['-e', 'x'])
    assert args.crps is False and args.crps_max_draws == 131072      # opt-in
    args = ap.parse_args(['-e', 'x', '--crps', '--crps-max-draws', '5000', '--stacking'])
    assert args.crps is True and args.crps_max_draws == 5000 and args.stacking is True
    assert '--crps' in ap.format_help() and 'mile_crps_stream' in ' '.join(ap.format_help().split())
    assert EV.crps_refusal('regr', 12) is None
    assert EV.crps_refusal('classification', 12).startswith('--crps:') and '--calibration' in EV.crps_refusal('classification', 12)
    assert 'at most 1024 chains' in EV.crps_refusal('regr', 1025)
    assert 'gram' in EV.crps_outputs(301, 128) and 'gram' not in EV.crps_outputs(301, 1024)
    assert 'gram' in EV.crps_outputs(2048, 128) and 'gram' not in EV.crps_outputs(2049, 128)      # 256 MiB exactly, and a row more


def test_crps_metrics_keys_and_arrays():
    import evaluate as EV
    raw, y = _raw(4, 10, 21, 6)
    w = np.array([0.1, 0.2, 0.3, 0.4])
    W = np.stack([np.full(4, 0.25), w])
    rows = M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y), W, outputs=M.CRPS_OUTPUTS)
    keys, arrays = EV.crps_metrics(rows, 3, stacked=w)
    names = ('', '_se', '_spread', '_spread_se', '_uniform', '_uniform_se', '_uniform_pooling_gain', '_per_chain', '_per_chain_median',
             '_per_chain_spread', '_rows_nan', '_thin_stride', '_dropped', '_stacked', '_stacked_se', '_stacked_pooling_gain',
             '_energy_distance_max')
    assert sorted(keys) == sorted('crps' + k for k in names)
    ref = CR.crps(raw, y, W)
    assert keys['crps'] == pytest.approx(ref['crps_mix'][0].mean(), rel=1e-12) and keys['crps_stacked'] == pytest.approx(ref['crps_mix'][2].mean(), rel=1e-12)
    assert keys['crps_uniform'] == pytest.approx(keys['crps'], rel=1e-12)           # nothing dropped: pooled is uniform
    assert keys['crps_uniform_pooling_gain'] >= 0 and keys['crps_stacked_pooling_gain'] >= 0 and keys['crps_energy_distance_max'] >= 0
    assert keys['crps_thin_stride'] == 3 and keys['crps_dropped'] == 0 and len(keys['crps_per_chain']) == 4
    assert sorted(arrays) == sorted(M.CRPS_OUTPUTS + ('energy_distance', 'weights', 'thin_stride'))
    assert arrays['crps_mix'].shape == (3, 21) and arrays['gram'].shape == (21, 4, 4) and arrays['weights'].shape == (2, 4)
    keys2, arrays2 = EV.crps_metrics(M.mixture_crps_dense(torch.from_numpy(raw), torch.from_numpy(y), W[:1], outputs=EV.crps_outputs(21, 4096)), 1)
    assert 'crps_stacked' not in keys2 and 'gram' not in arrays2 and 'crps_energy_distance_max' not in keys2

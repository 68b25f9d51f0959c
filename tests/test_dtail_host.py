"""Tail diagnostics without a GPU: the torch forms of mile_amd.metrics against the fp64 restatement tests/dtail_ref.py, the
block-wise direct summation of k_dtail_ess (emulated in NumPy) against the FFT estimator, the integer quantile positions, the
cases the definitions single out, and evaluate.py's key builder."""
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import diag_ref as R  # noqa: E402
import dtail_ref as T  # noqa: E402

RTOL = 1e-9
SHAPES = [(3, 64, 40, False, 2), (4, 250, 96, True, 2), (2, 100, 70, True, 4), (1, 128, 8, False, 2), (2, 8, 8, False, 1),
          (1, 4, 8, False, 2)]
OUTPUTS = ('ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean', 'rhat_folded')


def _run(x, ns, **kw):
    from mile_amd import metrics as M
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        out = M.tail_diagnostics(torch.from_numpy(x), ns, **kw)
    assert M.LAST_DTAIL_PATH == 'torch'
    return {k: v.numpy() for k, v in out.items()}


def _close(got, ref, rtol=RTOL):
    assert got.shape == ref.shape
    assert (np.isnan(got) == np.isnan(ref)).all()
    m = ~np.isnan(ref)
    np.testing.assert_allclose(got[m], ref[m], rtol=rtol, atol=0)


@pytest.mark.parametrize('C_,S,d,ties,ns', SHAPES)
def test_torch_path_matches_the_restatement(C_, S, d, ties, ns):
    x = R.ar1_draws(C_, S, d, 1, ties)
    ref = T.tail_diagnostics(x, ns)
    got = _run(x, ns)
    assert got['quantiles'].dtype == np.float32 and np.array_equal(got['quantiles'], ref['quantiles'], equal_nan=True)
    for k in OUTPUTS:
        assert got[k].dtype == np.float64, k
        _close(got[k], ref[k])
    # plane input: the same columns, laid out [d][C][S]
    plane = _run(np.ascontiguousarray(x.transpose(2, 0, 1)), ns, plane=True)
    for k in OUTPUTS + ('quantiles',):
        assert np.array_equal(plane[k], got[k], equal_nan=True), k


@pytest.mark.parametrize('C_,S,d,ties,ns', SHAPES + [(3, 1000, 6, False, 2)])
def test_blockwise_direct_summation_with_the_early_stop_matches_the_fft_estimator(C_, S, d, ties, ns):
    x = R.ar1_draws(C_, S, d, 1, ties)
    s = T.series(x)
    for k in T.SERIES:
        got, used = T.blockwise_ess(s[k], ns)
        _close(got, T.ess_mc(s[k], ns), rtol=1e-12)
        if S // ns > 128:
            assert used.min() < (S // ns) // 2, 'the early stop never took effect'


def test_integer_quantile_positions():
    for n in range(4, 201):
        lo, hi, a, b = T.quantile_indices(n)
        assert lo == int(np.ceil(n / 20)) - 1 and hi == int(np.ceil(19 * n / 20)) - 1
        assert (a, b) == ((n - 1) // 2, n // 2) and 0 <= lo <= a <= b <= hi < n
    from mile_amd.metrics import tail_quantile_indices
    assert all(tail_quantile_indices(n) == T.quantile_indices(n) for n in range(4, 201))


def test_chains_that_differ_in_scale_only():
    """Four iid N(0, 1) chains of 400 draws, one multiplied by 3: the rank R-hat sees nothing, the folded one does."""
    from mile_amd import metrics as M
    x = np.random.default_rng(0).standard_normal((4, 400, 6)).astype(np.float32)
    x[3] *= 3
    got = _run(x, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        rhat = M.gelman_split_r_hat(torch.from_numpy(x), 2).numpy()
    assert (rhat < 1.01).all(), rhat
    assert (got['rhat_folded'] > 1.1).all(), got['rhat_folded']
    _close(got['rhat_folded'], T.tail_diagnostics(x, 2)['rhat_folded'])


def test_constant_column_is_nan():
    x = R.ar1_draws(3, 64, 4, 1, False)
    x[:, :, 2] = 1.25
    got, ref = _run(x, 2), T.tail_diagnostics(x, 2)
    for k in OUTPUTS:
        assert np.isnan(got[k][2]) and np.isnan(ref[k][2]), k
        assert np.isfinite(got[k][[0, 1, 3]]).all(), k
    assert (got['quantiles'][:, 2] == 1.25).all()


def test_four_draws_of_one_chain_have_no_upper_tail():
    x = R.ar1_draws(1, 4, 8, 1, False)
    s = T.series(x)
    assert (s['i_hi'] == 1).all()                                   # ceil(19 * 4 / 20) - 1 = 3: q_hi is the largest draw
    got, ref = _run(x, 2), T.tail_diagnostics(x, 2)
    assert np.isnan(got['ess_tail']).all() and np.isnan(ref['ess_tail']).all()
    assert np.isfinite(got['ess_bulk']).all() and np.isfinite(got['ess_mean']).all()


def test_nan_draw_makes_its_column_nan():
    x = R.ar1_draws(3, 64, 4, 1, False)
    x[1, 7, 1] = np.nan
    got, ref = _run(x, 2), T.tail_diagnostics(x, 2)
    for k in OUTPUTS + ('quantiles',):
        assert np.isnan(got[k][..., 1]).all() and np.isnan(ref[k][..., 1]).all(), k
        assert np.isfinite(got[k][..., [0, 2, 3]]).all(), k


def test_evaluate_key_builder():
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import evaluate as E
    d = 5
    res = {'ess_bulk': torch.tensor([100., 400., float('nan'), 200., 300.]), 'ess_tail': torch.tensor([50., 80., float('nan'), 60., 70.]),
           'ess_mean': torch.tensor([400., 100., float('nan'), 1600., 25.]), 'mcse_mean': torch.ones(d),
           'rhat_folded': torch.tensor([1.0, 1.2, float('nan'), 1.05, 1.01]), 'quantiles': torch.zeros(3, d)}
    rhat = torch.tensor([1.3, 1.0, 1.0, 1.0, 1.0])
    keys, arrays = E.tail_keys('dtail', res, 1000, 2, rhat)
    assert keys == {'dtail_n_splits': 2, 'dtail_ess_bulk_min': 100.0, 'dtail_ess_bulk_median': 250.0, 'dtail_ess_tail_min': 50.0,
                    'dtail_ess_tail_median': 65.0, 'dtail_rhat_folded_median': pytest.approx(1.03), 'dtail_rhat_folded_max': pytest.approx(1.2),
                    'dtail_rhat_rank_max': pytest.approx(1.3), 'dtail_mcse_mean_over_sd_max': pytest.approx(0.2),
                    'dtail_ess_bulk_share': 0.25}
    assert set(arrays) == {'ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean', 'rhat_folded', 'quantiles'}
    keys, arrays = E.tail_keys('fdiag_tail', res, 1000, 2, rhat)
    assert set(keys) == {k.replace('dtail_', 'fdiag_tail_') for k in
                         ('dtail_n_splits', 'dtail_ess_bulk_min', 'dtail_ess_bulk_median', 'dtail_ess_tail_min', 'dtail_ess_tail_median',
                          'dtail_rhat_folded_median', 'dtail_rhat_folded_max', 'dtail_rhat_rank_max', 'dtail_mcse_mean_over_sd_max',
                          'dtail_ess_bulk_share')}
    assert set(arrays) == {'fdiag_' + k for k in ('ess_bulk', 'ess_tail', 'ess_mean', 'mcse_mean', 'rhat_folded', 'quantiles')}

"""Function-space chain diagnostics, host side (-m "not gpu"): the torch columns and their statistics against the fp64
restatements tests/fdiag_ref.py and tests/diag_ref.py, the summaries on hand-made arrays, the C ABI surface, the
permutation case in fp64, and the evaluate.py flag."""
import ctypes as C
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import mclmc_oracle as O
from tests import diag_ref as R
from tests import fdiag_ref as F

ROOT = Path(__file__).resolve().parents[1]

PERM_C, PERM_S, PERM_SEED = F.PERM_C, F.PERM_S, F.PERM_SEED


def _outputs(task, seed, C_=3, S=16, N=7):
    hs = (6, 2) if task == 'regr' else (6, 3)
    ospec = O.ModelSpec(4, hs, activation='tanh', task=task)
    prob = O.synthetic_problem(ospec, N, C_ * S, seed=seed, theta_scale=0.5)
    out = O.mlp_forward(ospec, prob['theta0'].astype(np.float64), prob['X'].astype(np.float64)).reshape(C_, S, N, hs[-1])
    return out, prob['y']


@pytest.mark.parametrize('task', ['regr', 'classification'])
@pytest.mark.parametrize('with_y', [True, False])
def test_dense_columns_match_the_restatement(task, with_y):
    from mile_amd import metrics as M
    out, y = _outputs(task, 1)
    if task == 'regr':
        out[0, 3, 2, 1] = 20.0                            # sigma clipped at 1e6
        out[1, 5, 4, 1] = -20.0                           # sigma clipped at 1e-6
    ref, L = F.columns(out, y if with_y else None, task)
    got = M.function_columns_dense(torch.from_numpy(out), torch.from_numpy(y) if with_y else None, task).numpy()
    O_ = out.shape[-1]
    assert got.shape == ref.shape == (3, 16, 7 * (O_ + with_y) + with_y)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    if task != 'regr':                                    # the probabilities of a row sum to one
        p = ref[:, :, :7 * (O_ + with_y)].reshape(3, 16, 7, O_ + with_y)[..., :O_]
        np.testing.assert_allclose(p.sum(axis=-1), 1.0, rtol=1e-14)
    if with_y:
        np.testing.assert_allclose(L, F.row_loglik(out, y, task).sum(axis=-1), rtol=1e-13)


@pytest.mark.parametrize('task', ['regr', 'classification'])
def test_dense_diagnostics_match_the_restatement(task):
    from mile_amd import metrics as M
    out, y = _outputs(task, 2)
    cols, L = F.columns(out, y, task)
    ref = R.chain_diagnostics(cols, 2)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        got = M.function_diagnostics_dense(torch.from_numpy(out), torch.from_numpy(y), task, 2)
    assert M.LAST_DIAG_PATH == 'torch'
    Q = out.shape[-1] + 1
    assert got['Q'] == Q and got['M'] == cols.shape[2] == 7 * Q + 1
    for k in ('wcv', 'bcv', 'ess', 'crhat', 'rhat'):
        np.testing.assert_allclose(got[k].numpy(), ref[k], rtol=1e-9, err_msg=k)
    assert got['ess'].shape == (3, got['M']) and bool(torch.isfinite(got['ess']).all())
    np.testing.assert_allclose(got['columns'].numpy(), np.transpose(cols, (2, 0, 1)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got['loglik_sum'].numpy(), L, rtol=1e-12)
    s, chain = F.summaries(got['rhat'].numpy(), got['crhat'].numpy(), got['ess'].numpy(), 7 * Q)
    for k in F.SUMMARY:
        assert got['summary'][k] == pytest.approx(s[k], rel=1e-12), k
    np.testing.assert_allclose(got['chain_summary'].numpy(), chain, rtol=1e-12)
    keys = M.function_diagnostics_summary(got, 7, Q, task)
    assert keys['fdiag_rhat_max'] == pytest.approx(np.max(ref['rhat'][:7 * Q]), rel=1e-9)
    assert keys['fdiag_n_columns'] == got['M'] and 0.0 < keys['fdiag_r_eff_mean'] and 0.0 <= keys['fdiag_between_share'] <= 1.0
    assert keys['fdiag_loglik_sum_rhat'] == pytest.approx(ref['rhat'][-1], rel=1e-9)
    names = ['mu', 'log_sigma', 'loglik'] if task == 'regr' else ['p0', 'p1', 'p2', 'loglik']
    for q, n in enumerate(names):
        assert keys[f'fdiag_rhat_max_{n}'] == pytest.approx(np.max(ref['rhat'][q:7 * Q:Q]), rel=1e-9), n


def test_summaries_skip_non_finite_cells_and_the_first_of_equal_extremes_wins():
    from mile_amd import _lib
    from mile_amd.metrics import _function_summaries
    assert _lib.FDIAG_SUMMARY == F.SUMMARY
    nan, inf = np.nan, np.inf
    #                 0     1     2     3     4     5    | L
    rhat = np.array([1.02, nan, 1.20, 1.20, 1.06, inf, 9.0], np.float32)
    crhat = np.array([[1.0, 1.5, nan, 1.5, 1.1, 1.0, 9.0],
                      [1.5, 1.0, 1.0, 1.0, 1.0, 1.0, 9.0]], np.float32)
    ess = np.array([[50.0, 7.0, 9.0, nan, 9.0, 8.0, 1.0],
                    [7.0, 30.0, inf, 7.0, 9.0, 8.0, 1.0]], np.float32)
    s, chain = F.summaries(rhat, crhat, ess, 6)
    f32 = lambda v: float(np.float32(v))
    assert s['rhat_max'] == f32(1.2) and s['rhat_column'] == 2 and s['rhat_skipped'] == 2
    assert (s['rhat_gt_1_01'], s['rhat_gt_1_05'], s['rhat_gt_1_1']) == (4, 3, 2)
    assert s['rhat_mean'] == pytest.approx((f32(1.02) + 2 * f32(1.2) + f32(1.06)) / 4, rel=1e-15)
    assert (s['crhat_max'], s['crhat_chain'], s['crhat_column'], s['crhat_skipped']) == (1.5, 0, 1, 1)
    assert (s['ess_min'], s['ess_chain'], s['ess_column'], s['ess_skipped']) == (7.0, 0, 1, 2)
    assert s['ess_mean'] == pytest.approx((50 + 7 + 9 + 9 + 8 + 7 + 30 + 7 + 9 + 8) / 10, rel=1e-15)
    assert chain.tolist() == [[7.0, 1.5], [7.0, 1.5]]
    got, gchain = _function_summaries(torch.from_numpy(rhat), torch.from_numpy(crhat), torch.from_numpy(ess), 6)
    for k in F.SUMMARY:
        assert got[k] == pytest.approx(s[k], rel=1e-15), k
    assert gchain.tolist() == chain.tolist()
    s0, chain0 = F.summaries(np.full(3, nan), np.full((2, 3), nan), np.full((2, 3), inf), 3)       # nothing finite
    got0, gchain0 = _function_summaries(torch.full((3,), nan), torch.full((2, 3), nan), torch.full((2, 3), inf), 3)
    for k in F.SUMMARY:
        assert (np.isnan(s0[k]) and np.isnan(got0[k])) or s0[k] == got0[k], k
    assert s0['rhat_column'] == s0['ess_chain'] == -1 and s0['ess_skipped'] == 6 and np.isnan(chain0).all() and bool(torch.isnan(gchain0).all())


def permutation_case():
    from mile_amd import ModelSpec
    return F.permutation_case(tuple((n, o, tuple(sh)) for n, o, sh in ModelSpec(3, F.PERM_WIDTHS, activation='tanh', task='regr').leaves()))


def test_permuted_chains_agree_in_function_space_and_not_in_parameter_space():
    """Three chains of 64 i.i.d. draws around one mode of a [3 -> 8 -> 8 -> 2] tanh net, chains 1 and 2 with the first hidden
    layer's units permuted.  fp64 reference with seed 0: un-permuting the draws moves the outputs by 1.55e-15; function-space
    max rhat 1.0108 over the 15 per-row columns (1.0026 for the summed log-likelihood); parameter-space max rhat 2.4091, 76 %
    of the parameters above 1.5."""
    theta, X, y, ospec, cols, fn, par = permutation_case()
    d = ospec.n_params
    rng = np.random.default_rng(PERM_SEED)                # the same stream: centre, noise -- the draws before the permutation
    base = 0.7 * rng.standard_normal(d) + 0.05 * rng.standard_normal((PERM_C, PERM_S, d))
    out_b = O.mlp_forward(ospec, base.reshape(-1, d), X.astype(np.float64))
    out_p = O.mlp_forward(ospec, theta.reshape(-1, d), X.astype(np.float64))
    moved = np.abs(out_p - out_b).max()
    share = float((par['rhat'] > 1.5).mean())
    print(f'FDIAG permutation fp64: outputs moved {moved:.2e}  function rhat max {fn["rhat"][:-1].max():.4f} (L {fn["rhat"][-1]:.4f})  '
          f'parameter rhat max {par["rhat"].max():.4f}  share above 1.5 {share:.2f}')
    assert moved < 1e-13 and not np.array_equal(theta[1], base[1])
    assert fn['rhat'].max() < 1.02
    assert par['rhat'].max() > 2.0
    # and the project's own dense path on the same draws: the same two bounds, and the reference's values
    from mile_amd import metrics as M
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        got = M.function_diagnostics_dense(torch.from_numpy(out_p.reshape(PERM_C, PERM_S, F.PERM_N, 2)), torch.from_numpy(np.array(y)), 'regr', 2)
        got_par = M.chain_diagnostics(torch.from_numpy(np.array(theta)), 2)
    np.testing.assert_allclose(got['columns'].numpy(), np.transpose(cols, (2, 0, 1)), rtol=1e-12, atol=1e-12)
    for k in ('wcv', 'bcv', 'ess', 'crhat', 'rhat'):
        np.testing.assert_allclose(got[k].numpy(), fn[k], rtol=1e-9, err_msg=k)
    assert float(got['rhat'].max()) < 1.02 and got['summary']['rhat_max'] == float(got['rhat'][:-1].max())
    assert float(got_par['rhat'].max()) > 2.0
    keys = M.function_diagnostics_summary(got, F.PERM_N, 3, 'regr')
    assert keys['fdiag_rhat_gt_1_05'] == 0 and keys['fdiag_rhat_max'] < 1.02


def test_c_abi_surface():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    p, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    assert _lib.SIGNATURES['mile_function_diagnostics'] == (i32, [p, p, i32, i32, p, p, i64, i32, u32, p, p, p, p, p, p, p, p, p, i64, i64, p])
    assert _lib.SIGNATURES['mile_function_diagnostics_workspace'] == (i64, [p, i32, i32, i64, i32])
    for name in ('mile_function_diagnostics', 'mile_function_diagnostics_workspace'):
        assert hasattr(lib, name) and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_function_diagnostics(mile_sampler *s, const float *theta, int32_t C, int32_t S, const void *X, const void *y, '
            'int64_t N, int32_t n_splits, uint32_t what, float *wcv, float *bcv, float *ess, float *crhat, float *rhat, float *columns, '
            'double *loglik_sum, double *summary, double *chain_summary, int64_t max_draws_per_pass, int64_t max_rows_per_tile, '
            'void *stream);') in header
    assert 'int64_t mile_function_diagnostics_workspace(const mile_sampler *s, int32_t C, int32_t S, int64_t N, int32_t with_y);' in header
    enum = (ROOT / 'mile_amd' / 'csrc' / 'mile_fdiag.h').read_text()
    body = enum[enum.index('enum {'):enum.index('FDIAG_NSUM')]
    names = [n.strip().lower()[len('fdiag_'):] for n in body[body.index('{') + 1:].split(',') if n.strip()]
    assert tuple(names) == _lib.FDIAG_SUMMARY                          # the binding's names are the header's enum, in order
    assert lib.mile_function_diagnostics_workspace(None, 3, 64, 10, 1) == -1      # no GPU needed: refused on the host
    assert lib.mile_function_diagnostics(None, None, 3, 64, None, None, 10, 2, 31, *([None] * 9), 0, 0, None) == -1
    assert b'mile_function_diagnostics: null argument' in lib.mile_last_error()


def test_evaluate_flag_parses():
    sys.path.insert(0, str(ROOT))
    import evaluate as EV
    ap = EV.build_parser()
    assert ap.parse_args(['-e', 'x']).function_diagnostics is None                # opt-in
    assert ap.parse_args(['-e', 'x', '--function-diagnostics']).function_diagnostics == 2
    assert ap.parse_args(['-e', 'x', '--function-diagnostics', '4']).function_diagnostics == 4
    assert ap.parse_args(['-e', 'x', '--function-diagnostics', '--diagnostics']).diagnostics == 2
    assert 'function-diagnostics' in EV.__doc__

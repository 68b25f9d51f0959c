"""Chain diagnostics without a GPU: the torch functions of mile_amd.metrics against the fp64 restatement tests/diag_ref.py,
the argument checks of mile_chain_diagnostics (which come before any launch), and evaluate.py's --diagnostics surface.
Like the other host tests of the C ABI, the library test builds libmile_hip.so if it is stale, so it needs hipcc (no GPU)."""
import ctypes as C
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import diag_ref as R  # noqa: E402

RTOL = 1e-9
SHAPES = [(3, 64, 40, False, 2), (4, 250, 96, True, 2), (2, 100, 70, True, 4), (1, 128, 8, False, 2)]


def _close(got, ref):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == ref.shape
    assert (np.isnan(got) == np.isnan(ref)).all()
    m = ~np.isnan(ref)
    np.testing.assert_allclose(got[m], ref[m], rtol=RTOL, atol=0)


@pytest.mark.parametrize('C_,S,d,ties,ns', SHAPES)
def test_torch_functions_match_the_restatement(C_, S, d, ties, ns):
    from mile_amd import metrics as M
    x = R.ar1_draws(C_, S, d, 1, ties).astype(np.float64)
    xt = torch.from_numpy(x)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', UserWarning)
        _close(M.within_chain_var(xt), R.within_chain_var(x))
        _close(M.between_chain_var(xt), R.between_chain_var(x))
        _close(M.gelman_split_r_hat(xt, ns), R.gelman_split_r_hat(x, ns))
        _close(M.split_chain_r_hat(xt, ns), R.split_chain_r_hat(x, ns))
        _close(M.gelman_split_r_hat(xt, ns, rank_normalize=False), R.gelman_split_r_hat(x, ns, rank_normalize=False))
        got = M.chain_diagnostics(xt, ns)
    assert M.LAST_DIAG_PATH == 'torch' and sorted(got) == ['bcv', 'crhat', 'ess', 'rhat', 'wcv']
    ref = R.chain_diagnostics(x, ns)
    for k in ref:
        _close(got[k], ref[k])
    if C_ == 1:
        assert np.isnan(got['bcv'].numpy()).all()


def test_batched_ranks_average_ties_and_propagate_nan():
    from mile_amd import metrics as M
    x = np.array([[1.0, 0.0, 2.0], [1.0, 0.0, np.nan], [0.5, 0.0, 1.0], [1.0, -0.0, 3.0], [2.0, 0.0, 0.0]])
    z = M.rank_normalize_columns(torch.from_numpy(x)).numpy()
    _close(z[:, :2], R.rank_normalize_columns(x[:, :2]))
    assert np.isnan(z[:, 2]).all()
    assert z[0, 0] == z[1, 0] == z[3, 0] and len(set(z[:, 1])) == 1
    one = M.rank_normalize_array(torch.from_numpy(x[:, 0])).numpy()              # the existing column-by-column function
    np.testing.assert_allclose(z[:, 0], one, rtol=1e-12)


def test_value_error_and_warning():
    from mile_amd import metrics as M
    x = torch.from_numpy(R.ar1_draws(2, 64, 3, 1, False))
    for f in (M.gelman_split_r_hat, M.split_chain_r_hat, M.chain_diagnostics):
        with pytest.raises(ValueError, match='divisible by n_splits'):
            f(x, 3)
        with pytest.warns(UserWarning, match='at least 50x'):
            f(x, 2)
    big = torch.from_numpy(R.ar1_draws(2, 100, 3, 1, False))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        M.gelman_split_r_hat(big, 2)
        M.chain_diagnostics(big, 2)


def test_trailing_shapes():
    from mile_amd import metrics as M
    x = R.ar1_draws(3, 100, 12, 1, True).astype(np.float64)
    flat = M.chain_diagnostics(torch.from_numpy(x), 2)
    shaped = M.chain_diagnostics(torch.from_numpy(x.reshape(3, 100, 3, 4)), 2)
    for k, v in flat.items():
        lead = (3,) if k in ('ess', 'crhat') else ()
        assert shaped[k].shape == (*lead, 3, 4)
        assert torch.equal(shaped[k].reshape(v.shape), v) or (torch.isnan(v) == torch.isnan(shaped[k].reshape(v.shape))).all()
    _close(shaped['rhat'], R.gelman_split_r_hat(x.reshape(3, 100, 3, 4), 2))
    _close(M.split_chain_r_hat(torch.from_numpy(x.reshape(3, 100, 3, 4)), 2), R.split_chain_r_hat(x.reshape(3, 100, 3, 4), 2))


def test_chain_diagnostics_on_cpu_equals_the_pieces():
    from mile_amd import metrics as M
    x = torch.from_numpy(R.ar1_draws(3, 100, 10, 1, True))               # fp32 CPU tensor: the torch path
    got = M.chain_diagnostics(x, 2)
    xd = x.double()
    assert torch.allclose(got['wcv'], M.within_chain_var(xd), rtol=1e-12)
    assert torch.allclose(got['bcv'], M.between_chain_var(xd), rtol=1e-12)
    assert torch.allclose(got['rhat'], M.gelman_split_r_hat(xd, 2), rtol=1e-12)
    assert torch.allclose(got['crhat'], M.split_chain_r_hat(xd, 2), rtol=1e-12)
    assert torch.allclose(got['ess'], M.effective_sample_size(xd), rtol=1e-9)   # (erfinv there, ndtri here)


def test_library_exports_and_refuses_bad_arguments_before_any_launch():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    assert lib.mile_abi_version() == _lib.ABI_VERSION
    B = _lib.DIAG_BITS
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    every = B['wcv'] | B['bcv'] | B['ess'] | B['crhat'] | B['rhat']

    def call(C_=3, S=64, d=4, ns=2, what=every, ws=p, nbytes=1 << 40, src=p, outs=(p,) * 5):
        return lib.mile_chain_diagnostics(src, C_, S, d, ns, what, *outs, ws, nbytes, None)

    INVALID, STATE = -1, -2
    assert call(ns=3) == INVALID and b'divide' in lib.mile_last_error()
    assert call(S=2) == INVALID
    assert call(S=4, ns=4) == INVALID and b'fewer than 2' in lib.mile_last_error()
    assert call(S=5000) == INVALID
    assert call(C_=0) == INVALID and call(d=0) == INVALID and call(src=None) == INVALID
    assert call(what=0) == INVALID and call(what=64) == INVALID
    assert call(outs=(p, p, None, p, p)) == INVALID
    assert call(what=B['wcv'] | B['pooled_input']) == INVALID
    assert call(C_=5, S=3500) == INVALID and b'unsupported' in lib.mile_last_error()
    need = lib.mile_chain_diagnostics_workspace(3, 64, 4, every)
    assert need == 4 * (2 * 3 * 64 * 4 + 3 * 5 * 8)
    assert call(nbytes=need - 1) == STATE and b'workspace' in lib.mile_last_error()
    assert call(ws=None) == STATE
    assert lib.mile_chain_diagnostics_workspace(3, 5000, 4, every) == -1
    # a chunked walk is accepted from one tile of 32 parameters on
    per = 2 * 12 * 1000 * 4 + 12 * 5 * 8
    assert lib.mile_chain_diagnostics_workspace(12, 1000, 10 ** 6, every) == per * ((256 << 20) // per // 32 * 32)
    assert call(C_=12, S=1000, d=10 ** 6, nbytes=32 * per - 1) == STATE


def test_evaluate_accepts_the_flag_and_adds_nothing_without_it():
    sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
    import evaluate
    from mile_amd import ModelSpec
    ap = evaluate.build_parser()
    assert ap.parse_args(['-e', 'x']).diagnostics is None
    assert ap.parse_args(['-e', 'x', '--diagnostics']).diagnostics == 2
    assert ap.parse_args(['-e', 'x', '--diagnostics', '4']).diagnostics == 4
    spec = ModelSpec(5, (4, 2))
    d = spec.n_params
    samples = R.ar1_draws(3, 100, d, 1, False)
    samples[1, 7, 3] = np.nan                                               # chain 1 is left out
    none, arrays = evaluate.diagnostic_metrics(samples, spec, None, 'cpu')
    assert none == {} and arrays is None
    m, arrays = evaluate.diagnostic_metrics(samples, spec, 2, 'cpu')
    assert all(k.startswith('diag_') for k in m) and m['diag_n_splits'] == 2
    for k in ('diag_ess_min', 'diag_ess_median', 'diag_crhat_median', 'diag_crhat_max', 'diag_rhat_median', 'diag_rhat_max',
              'diag_wcv_median', 'diag_bcv_median'):
        assert np.isfinite(m[k]), k
    assert arrays['ess'].shape == arrays['crhat'].shape == (2, d) and arrays['rhat'].shape == arrays['wcv'].shape == (d,)
    names = [n for n, _, _ in spec.leaves()]
    assert sorted(m['diag_ess_layer_mean']) == sorted(names) == sorted(m['diag_crhat_layer_mean'])
    ref = R.chain_diagnostics(samples[[0, 2]], 2)
    np.testing.assert_allclose(arrays['ess'], ref['ess'], rtol=1e-9)
    n0, o0, s0 = next(iter(spec.leaves()))
    np.testing.assert_allclose(m['diag_ess_layer_mean'][n0], ref['ess'][:, o0:o0 + int(np.prod(s0))].mean(), rtol=1e-9)

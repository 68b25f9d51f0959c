"""CPU tests of mile_predict's host side (symbol, binding, argument validation on handles created without a GPU) and of
the metrics built on the raw outputs: sample_from_predictions, accuracy (ties as scipy.stats.mode), coverage and
calibration error (against np.quantile), rmse.  No GPU compute."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from mile_amd import metrics as M


# ---------------------------------------------------------------- C ABI -----------------
def _fcn_cspec(F, widths, task=0):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features, cs.n_layers = F, len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.activation, cs.task, cs.prior, cs.prior_loc, cs.prior_scale, cs.use_bias = 0, task, 0, 0.0, 1.0, 1
    return cs


def _attn_pre_cspec(V=50, T=16, Cc=32, H=2, D=16, proj=(8,), K=2):
    from mile_amd import _lib
    cs = _lib.ModelSpecC()
    cs.in_features = T
    widths = list(proj) + [K]
    cs.n_layers = len(widths)
    for i, w in enumerate(widths):
        cs.widths[i] = w
    cs.task, cs.prior, cs.prior_scale, cs.use_bias = 1, 0, 1.0, 1
    cs.model, cs.vocab_size, cs.ctx_len, cs.emb_size, cs.n_heads, cs.qkv_dim = 4, V, T, Cc, H, D
    return cs


def test_library_exports_and_binds_mile_predict():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    assert 'mile_predict' in _lib.SIGNATURES
    assert hasattr(lib, 'mile_predict')
    res, args = _lib.SIGNATURES['mile_predict']
    assert res is C.c_int32 and len(args) == 7          # handle, theta, S, X, N, out, stream: no labels
    assert lib.mile_predict.argtypes == args
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10     # a new symbol under the same ABI


def test_mile_predict_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 2))), 0, C.byref(h)) == 0
    try:
        buf = (C.c_float * 1024)()
        p = C.cast(buf, C.c_void_p)
        for theta, S, X, N, out in ((None, 1, p, 1, p), (p, 1, None, 1, p), (p, 1, p, 1, None),
                                    (p, 0, p, 1, p), (p, -3, p, 1, p), (p, 1, p, 0, p), (p, 1, p, -1, p),
                                    (p, 1, p, 0x40000000, p)):
            assert lib.mile_predict(h, theta, S, X, N, out, None) == -1, (S, N)
            assert b'mile_predict' in lib.mile_last_error()
        assert lib.mile_predict(None, p, 1, p, 1, p, None) == -1
    finally:
        lib.mile_destroy(h)


def test_mile_predict_needs_the_pretrained_tables():
    from mile_amd import _lib
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.mile_create(C.byref(_attn_pre_cspec()), 0, C.byref(h)) == 0, lib.mile_last_error()
    try:
        buf = (C.c_float * 1024)()
        p = C.cast(buf, C.c_void_p)
        assert lib.mile_predict(h, p, 1, p, 1, p, None) == -2
        assert b'mile_set_embedding' in lib.mile_last_error()
        assert lib.mile_predict(h, None, 1, p, 1, p, None) == -1      # argument checks come first
    finally:
        lib.mile_destroy(h)


# ---------------------------------------------------------------- accuracy -----------------
def _scipy_mode(draws):
    from scipy.stats import mode
    return mode(draws, axis=(0, 1)).mode


def test_accuracy_matches_scipy_mode_with_ties():
    rng = np.random.default_rng(0)
    Cn, S, N, K = 3, 40, 50, 4
    draws = rng.integers(0, K, size=(Cn, S, N))
    # hand-built ties: every class 30 times; two classes 60 times; three classes 40 times (the smallest must win)
    draws[:, :, 0] = (np.arange(Cn * S) % 4).reshape(Cn, S)
    draws[:, :, 1] = np.where(np.arange(Cn * S) % 2 == 0, 3, 1).reshape(Cn, S)
    draws[:, :, 2] = (1 + np.arange(Cn * S) % 3).reshape(Cn, S)[:, ::-1]
    draws[:, :, 3] = np.where(np.arange(Cn * S) < 60, 2, 0).reshape(Cn, S)
    expected_mode = _scipy_mode(draws)
    assert list(expected_mode[:4]) == [0, 1, 1, 0]       # scipy's own tie rule, on the tie rows
    labels = expected_mode.copy()
    labels[::3] = (labels[::3] + 1) % K                   # some rows wrong
    labels[1] = 3                                         # the tie row's larger label is NOT the mode
    expected = np.mean(labels == expected_mode)
    got = M.accuracy(torch.from_numpy(draws), torch.from_numpy(labels), K)
    assert float(got) == pytest.approx(expected, abs=1e-15)
    counts = M.class_counts(torch.from_numpy(draws), K)
    assert counts.shape == (N, K) and int(counts.sum()) == Cn * S * N
    assert torch.equal(torch.argmax(counts * K + (K - 1 - torch.arange(K)), dim=-1), torch.from_numpy(expected_mode))
    # per chain: the mode over the samples of each chain (evaluation.py:487)
    from scipy.stats import mode
    pc = M.accuracy_from_counts(torch.stack([M.class_counts(torch.from_numpy(draws[c]), K) for c in range(Cn)]),
                                torch.from_numpy(labels))
    for c in range(Cn):
        assert float(pc[c]) == pytest.approx(np.mean(labels == mode(draws[c], axis=0).mode), abs=1e-15)


def test_chunked_counts_give_the_same_accuracy():
    rng = np.random.default_rng(1)
    Cn, S, N, K = 3, 40, 50, 4
    draws = torch.from_numpy(rng.integers(0, K, size=(Cn, S, N)))
    labels = torch.from_numpy(rng.integers(0, K, size=N))
    whole = M.class_counts(draws, K)
    acc = torch.zeros_like(whole)
    for c in range(Cn):
        for s0 in range(0, S, 7):                         # 7 does not divide 40
            acc += M.class_counts(draws[c, s0:s0 + 7], K)
    assert torch.equal(acc, whole)
    assert float(M.accuracy_from_counts(acc, labels)) == float(M.accuracy(draws, labels, K))


# ---------------------------------------------------------------- coverage -----------------
def test_coverage_and_calibration_error_match_numpy_quantiles():
    rng = np.random.default_rng(2)
    draws = rng.standard_normal((2, 500, 30)) * rng.uniform(0.5, 2.0, size=30) + rng.standard_normal(30)
    y = rng.standard_normal(30) * 1.5
    nominal = [0.5, 0.75, 0.9, 0.95]
    flat = draws.reshape(-1, 30)
    y[7] = np.quantile(flat[:, 7], 0.05)                  # exactly the lower bound of the 0.9 interval: inside (inclusive)
    y[8] = np.quantile(flat[:, 8], 0.875)                 # exactly the upper bound of the 0.75 interval
    expected = []
    for c in nominal:
        lo, hi = np.quantile(flat, [0.5 - c / 2, 0.5 + c / 2], axis=0)       # linear interpolation
        expected.append(np.mean((lo <= y) & (hi >= y)))
    lo9, hi9 = np.quantile(flat[:, 7], [0.05, 0.95])
    assert lo9 <= y[7] and not lo9 < y[7]
    got = M.calculate_coverage(nominal, torch.from_numpy(y), torch.from_numpy(draws))
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.numpy(), expected, rtol=1e-12)
    # the quantiles themselves
    q = M._quantiles_linear(torch.from_numpy(flat), torch.tensor([0.025, 0.05, 0.125, 0.25, 0.75, 0.875, 0.95, 0.975], dtype=torch.float64))
    np.testing.assert_allclose(q.numpy(), np.quantile(flat, [0.025, 0.05, 0.125, 0.25, 0.75, 0.875, 0.95, 0.975], axis=0), rtol=1e-12)
    np.testing.assert_allclose(M.get_quantiles(0.9).numpy(), [0.05, 0.95], rtol=1e-15)
    ce = M.calibration_error(nominal, got)
    assert float(ce) == pytest.approx(math.sqrt(np.mean((np.array(nominal) - np.array(expected)) ** 2)), rel=1e-12)
    w = M.coverage_weighting(nominal, kappa=2.0)
    np.testing.assert_allclose(w.numpy(), np.array(nominal) ** 2 / np.sum(np.array(nominal) ** 2), rtol=1e-12)
    cew = M.calibration_error(nominal, got, weights=w)
    assert float(cew) == pytest.approx(math.sqrt(np.mean(w.numpy() * (np.array(nominal) - np.array(expected)) ** 2)), rel=1e-12)
    # rmse: the mean over (chain, sample), then over the rows
    assert float(M.rmse(torch.from_numpy(y), torch.from_numpy(draws))) == pytest.approx(
        math.sqrt(np.mean((y - flat.mean(axis=0)) ** 2)), rel=1e-12)
    assert float(M.rmse(torch.from_numpy(y), torch.from_numpy(flat.mean(axis=0)))) == pytest.approx(
        math.sqrt(np.mean((y - flat.mean(axis=0)) ** 2)), rel=1e-12)


# ---------------------------------------------------------------- draws -----------------
def test_sample_from_predictions_regression():
    g = torch.Generator().manual_seed(7)
    preds = torch.randn((2, 5, 11, 2), generator=g, dtype=torch.float64)
    preds[0, 0, 0, 1], preds[0, 0, 1, 1] = 40.0, -40.0
    state = g.get_state()
    draws = M.sample_from_predictions(preds, 'regr', g)
    assert draws.shape == (2, 5, 11)
    g2 = torch.Generator()
    g2.set_state(state)
    z = torch.randn((2, 5, 11), generator=g2, dtype=torch.float64)
    scale = torch.exp(preds[..., 1]).clamp(min=1e-6, max=1e6)
    assert torch.equal(draws, z * scale + preds[..., 0])
    assert scale[0, 0, 0] == 1e6 and scale[0, 0, 1] == 1e-6
    assert draws[0, 0, 0] == z[0, 0, 0] * 1e6 + preds[0, 0, 0, 0]
    assert draws[0, 0, 1] == z[0, 0, 1] * 1e-6 + preds[0, 0, 1, 0]


def test_sample_from_predictions_classification():
    g = torch.Generator().manual_seed(8)
    logits = torch.randn((3, 6, 9, 5), generator=g)
    want = torch.randint(0, 5, (3, 6, 9), generator=g)
    logits.scatter_(-1, want[..., None], (50.0 + logits.max()).expand(3, 6, 9, 1))        # one logit 50 above the rest
    draws = M.sample_from_predictions(logits, 'class', g)
    assert draws.shape == (3, 6, 9) and draws.dtype == torch.int64
    assert torch.equal(draws, want)
    # otherwise the frequencies follow the softmax
    lg = torch.log(torch.tensor([0.1, 0.2, 0.7])).expand(20000, 1, 3)
    f = torch.bincount(M.sample_from_predictions(lg, 'class', g).reshape(-1), minlength=3) / 20000.0
    assert torch.allclose(f, torch.tensor([0.1, 0.2, 0.7]), atol=0.015)

"""The cases of tests/head_cases.py on the CPU: their conditions, what the fp64 oracle gives in the clip, the float32-vs-fp64
table that is the yardstick of tests/test_gpu_head_edges.py's bounds (`pytest -s` prints it), and the C restatement
(oracle/cpu_mclmc.c) against the NumPy oracle on the FCN regression cases, so that the two oracles are known to agree in the clip
before anything is asked of a kernel."""
import shutil

import numpy as np
import pytest

from tests import head_cases as H

ALL = sorted(H.ALL_CASES)
REGR = [n for n in ALL if n.startswith('regr-')]
FCN_REGR = [n for n in REGR if H.ALL_CASES[n][0]().kind == 'fcn']


@pytest.mark.parametrize('name', ALL)
def test_conditions_and_steering(name):
    """build() asserts the conditions of the module docstring for the seed in the table; here also: at most 2 + 17 rows went, the N
    training and 61 evaluation rows are whole, and the steering changed the last layer of the steered chains and nothing else."""
    c = H.case(name)
    model_fn, N, seed, _ = H.ALL_CASES[name]
    assert (c.N, len(c.yt), c.seed) == (N, H.N_TEST, seed)
    assert c.dropped['band'] <= H.MAX_BAND_ROWS and c.dropped['kink'] <= H.MAX_KINK_ROWS
    assert c.dropped['band_test'] <= H.MAX_BAND_ROWS and c.dropped['kink_test'] <= H.MAX_KINK_ROWS
    assert c.theta.dtype == np.float32 and np.isfinite(c.theta).all()
    base = model_fn().synthetic(N + H.EXTRA_ROWS, c.E, seed)['theta0']
    (k0, k1), (b0, b1), fin, fout = c.model.last
    other = np.ones(c.model.d, dtype=bool)
    other[k0:k1] = False
    other[b0:b1] = False
    assert np.array_equal(c.theta[:, other], base[:, other])
    ctl = c.chain('control')
    assert np.array_equal(c.theta[ctl], base[ctl])
    if c.model.task == 'regr':                  # the mu column of the steered chains is untouched as well
        mu = np.concatenate([[b0], k0 + np.arange(fin) * fout])
        assert np.array_equal(c.theta[:, mu], base[:, mu])
        for e in range(c.E):
            assert (e == ctl) == np.array_equal(c.theta[e, c.sigma_columns()], base[e, c.sigma_columns()])
        # on the evaluation rows the steered chains are in the clip too (not asserted to the row: other rows than steered on)
        ft = c.clipped_fraction(c.Xt)
        assert ft[c.chain('hi')] > 0.9 and ft[c.chain('lo')] > 0.9 and 0.1 < ft[c.chain('hi_edge')] < 0.9 and ft[ctl] == 0.0
    else:
        for nm in ('sat_pos', 'sat_neg'):
            assert not np.array_equal(c.theta[c.chain(nm), k0:k1], base[c.chain(nm), k0:k1])


@pytest.mark.parametrize('name', REGR)
def test_oracle_gradient_in_the_clip(name):
    """fp64 oracle: in hi and lo the gradient on the log-sigma bias and kernel column is the prior's, exactly; in hi the
    log-likelihood is -N (T + log sqrt(2 pi)) up to r^2 / 2 = 1e-12; in lo d/dmu is of order 1e12."""
    c = H.case(name)
    lp, g = c.ref64
    lpp, gp = c.prior
    cols = c.sigma_columns()
    for nm in ('hi', 'lo'):
        e = c.chain(nm)
        assert np.array_equal(g[e, cols], gp[e, cols]), nm
    for nm in ('hi_edge', 'lo_edge', 'control'):
        e = c.chain(nm)
        assert np.abs(g[e, cols] - gp[e, cols]).max() > 0, nm
    hi, lo = c.chain('hi'), c.chain('lo')
    want = -c.N * (H.T_CLIP + H.LOG_SQRT_2PI)
    assert abs((lp[hi] - lpp[hi]) / want - 1.0) < 1e-10
    (k0, _), (b0, _), _, _ = c.model.last
    assert 1e10 < abs(g[lo, b0] - gp[lo, b0]) < 1e15         # sum over the rows of (y - mu) * 1e12


def test_float32_oracle_against_fp64_table():
    """The yardstick: per case and chain, max |float32 - fp64| / max |fp64| of the gradient, the log-posterior and the pointwise
    log-likelihood (training rows, evaluation rows) of the NumPy restatements evaluated in float32 throughout.  Finite everywhere
    and, as it turns out, below 1e-5 everywhere: the clip costs float32 nothing that the project's bounds do not already allow,
    so 4 x this error raises only a few per-leaf bounds of the attention models above the 5e-5 of tests/leafcheck.py."""
    print('\nHEADCASES float32 restatement vs fp64 (per chain)')
    print(f'{"case":<22s}{"chain":<9s}{"logp":>10s}{"grad":>10s}{"worst leaf":>12s}{"pointwise":>11s}{"pw (eval)":>11s}')
    for name in ALL:
        c = H.case(name)
        f = H.f32_errors(c)
        for e, nm in enumerate(c.regimes):
            row = (f['logp'][e], f['grad'][e], f['leaf'][e].max(), f['pointwise'][e], f['pointwise_test'][e])
            print(f'{name:<22s}{nm:<9s}' + ''.join(f'{v:>{w}.2e}' for v, w in zip(row, (10, 10, 12, 11, 11))))
            assert np.isfinite(row).all(), (name, nm, row)
            assert max(row[0], row[1], row[3], row[4]) < 1e-5, (name, nm, row)
        b = H.bounds(c)
        assert (b['logp'] == H.LOGP_TOL).all() and (b['grad'] == H.GRAD_TOL.get(c.model.kind, 2e-5)).all(), name
        assert (b['pointwise_test'] == H.PW_TOL).all(), name


@pytest.mark.skipif(shutil.which('gcc') is None, reason='needs gcc')
@pytest.mark.parametrize('name', FCN_REGR)
def test_c_oracle_agrees_in_the_clip(name):
    """oracle/cpu_mclmc.c (float32 C) on the steered ensembles, chain by chain, within the bounds the kernels are held to; and
    the structural facts of the clip: exactly the prior's gradient on the log-sigma column in hi and lo."""
    from oracle.cpu_c import CpuPort
    c = H.case(name)
    lp, g = CpuPort(c.model.ospec, c.X, c.y).logpost_grad(np.array(c.theta))
    lp64, g64 = c.ref64
    b = H.bounds(c)
    el, eg = H.logp_error(lp, lp64), H.chain_error(g, g64)
    print(f'\nHEADCASES C oracle {name}: logp {np.array2string(el, precision=2)} grad {np.array2string(eg, precision=2)}')
    assert (el < b['logp']).all() and (eg < b['grad']).all(), (el, eg)
    gp = c.prior[1]
    cols = c.sigma_columns()
    for nm in ('hi', 'lo'):
        e = c.chain(nm)
        assert np.abs(g[e, cols] - gp[e, cols]).max() <= 1e-6 * np.abs(gp[e, cols]).max(), nm

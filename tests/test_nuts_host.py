"""NUTS and window adaptation without a GPU: the fp64 restatement (tests/nuts_ref.py) against independent forms, the
host-side schedule, and the C ABI's NUTS structs."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import nuts_ref as R

ROOT = Path(__file__).resolve().parents[1]


def _rotating_momenta(rng, n, d):
    """Momenta whose direction drifts, so sub-trees of every size turn somewhere."""
    th = np.cumsum(rng.uniform(0.05, 0.9, n))
    ps = np.zeros((n, d))
    ps[:, 0], ps[:, 1] = np.cos(th), np.sin(th)
    ps[:, 2:] = 0.3 * rng.standard_normal((n, d - 2))
    return ps


def test_iterative_uturn_matches_recursive_tree_doubling():
    rng = np.random.default_rng(0)
    stops = set()
    for trial in range(600):
        depth = int(rng.integers(1, 7))
        d = 4
        m = rng.uniform(0.3, 3.0, d)
        ps = _rotating_momenta(rng, 2 ** depth, d) if trial % 3 else rng.standard_normal((2 ** depth, d)) + 0.5
        it, rec = R.iterative_subtree_turns(m, ps, depth), R.recursive_subtree_turns(m, ps, depth)
        assert it == rec, (trial, depth, it, rec)
        stops.add(rec)
    assert None in stops and len(stops) > 10        # both outcomes, at many different leaves


def test_checkpoint_indices():
    # termination.iterative_uturn_numpyro._leaf_idx_to_ckpt_idxs, the docstring's examples
    assert R.leaf_idx_to_ckpt_idxs(6) == (3, 2)     # even leaf: stores at idx_max 2, checks nothing (min > max)
    assert R.leaf_idx_to_ckpt_idxs(7) == (0, 2)     # three nested subtrees complete at 7
    assert R.leaf_idx_to_ckpt_idxs(13) == (2, 2)


def _gaussian_target(d=10, seed=3):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((d, d))
    Q, _ = np.linalg.qr(A)
    cov = Q @ np.diag(np.linspace(0.5, 2.0, d)) @ Q.T
    mu = rng.standard_normal(d)
    P = np.linalg.inv(cov)

    def f(x):
        r = x - mu
        return -0.5 * float(r @ P @ r), -(P @ r)
    return f, mu, cov


def test_restated_nuts_samples_a_correlated_gaussian():
    d, n = 10, 1500
    f, mu, cov = _gaussian_target(d)
    rng = np.random.default_rng(1)
    x = mu.copy()
    lp, g = f(x)
    st = R.HMCState(x, lp, g)
    M = 10
    xs, acc, steps = [], [], []
    for i in range(n + 100):
        st, info = R.nuts_step(f, st, 0.4, np.ones(d), rng.standard_normal(d), rng.uniform(size=2 * M + 2 ** M), M)
        if i >= 100:
            xs.append(st.position)
            acc.append(info.acceptance_rate)
            steps.append(info.num_integration_steps)
    xs = np.array(xs)
    sd = np.sqrt(np.diag(cov))
    # NUTS draws of a Gaussian are close to independent; allow an effective sample size of n/3: 5 standard errors
    se_mean = sd / math.sqrt(n / 3)
    assert np.all(np.abs(xs.mean(0) - mu) < 5 * se_mean), (xs.mean(0) - mu) / se_mean
    se_var = np.diag(cov) * math.sqrt(2 / (n / 3))
    assert np.all(np.abs(xs.var(0) - np.diag(cov)) < 5 * se_var), (xs.var(0) - np.diag(cov)) / se_var
    assert 0.6 < np.mean(acc) <= 1.0
    assert 3 <= np.mean(steps) < 2 ** M


def test_build_schedule_windows():
    from mile_amd.warmup import build_schedule
    for n in (10, 19, 20, 100, 150, 1000, 1500):
        host = np.array(build_schedule(n), dtype=np.int64).reshape(-1, 2)
        assert (host == R.build_schedule(n)).all() and len(host) == n
    assert build_schedule(10) == [(0, False)] * 10                     # < 20 steps: step size only
    s = np.array(build_schedule(100), dtype=np.int64)
    # 75 + 25 + 50 > 100: buffers of int(0.15 n) = 15 and int(0.1 n) = 10, one slow window of 75
    assert (s[:15, 0] == 0).all() and (s[15:90, 0] == 1).all() and (s[90:, 0] == 0).all()
    assert np.flatnonzero(s[:, 1]).tolist() == [89]
    s = np.array(build_schedule(1000), dtype=np.int64)
    # windows 25, 50, 100, 200 and the remaining 500 between the 75- and 50-step buffers
    assert np.flatnonzero(s[:, 1]).tolist() == [99, 149, 249, 449, 949]
    assert (s[:75, 0] == 0).all() and (s[75:950, 0] == 1).all() and (s[950:, 0] == 0).all()


def test_dual_averaging_reaches_the_target_acceptance_rate():
    # synthetic acceptance curve a(eps) = exp(-eps): the target 0.8 sits at eps* = -log 0.8
    ad = R.WindowAdaptation(3, initial_step_size=1.0, target=0.8)
    for _ in range(3000):
        ad.update(0, False, np.zeros(3), math.exp(-ad.step_size))
    eps, _ = ad.final()
    assert abs(eps + math.log(0.8)) < 0.02 * -math.log(0.8)
    assert abs(math.exp(-eps) - 0.8) < 0.01


def test_slow_window_end_sets_the_regularised_variance():
    rng = np.random.default_rng(0)
    ad = R.WindowAdaptation(4)
    xs = rng.standard_normal((30, 4)) * np.array([0.1, 1.0, 2.0, 5.0])
    for i, x in enumerate(xs):
        ad.update(1, i == len(xs) - 1, x, 0.8)
    n = len(xs)
    want = n / (n + 5) * xs.var(0, ddof=1) + 1e-3 * 5 / (n + 5)
    assert np.allclose(ad.imm, want) and ad.n == 0 and ad.da.step == 1


def test_sampler_config_nuts_resolves_to_a_kernel():
    from mile_amd.config import SamplerConfig
    from mile_amd.kernels import KERNELS, nuts
    assert SamplerConfig(name='nuts').kernel is nuts is KERNELS['nuts']
    assert SamplerConfig().name == 'nuts'                             # the reference's default
    assert 'hmc' not in KERNELS
    with pytest.raises(NotImplementedError):
        SamplerConfig(name='hmc').kernel


def test_nuts_structs_match_the_header():
    from mile_amd import _lib
    header = (ROOT / 'include' / 'mile_hip.h').read_text()
    for cls, name in ((_lib.NutsArgsC, 'mile_nuts_args'), (_lib.NutsAdaptArgsC, 'mile_nuts_adapt_args')):
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1),
                      flags=re.S)
        fields = re.findall(r'(?:const\s+)?\w+\s*\*?\s*(\w+)(?:\[\w+\])?\s*;', body)
        assert fields == [f[0] for f in cls._fields_], (name, fields)
    assert {'mile_nuts_reserve', 'mile_nuts_step', 'mile_nuts_warmup'} <= set(_lib.SIGNATURES)


def test_nuts_info_is_gathered_in_chain_order():
    from mile_amd.sampling import NUTS_INFO_FIELDS, _nuts_info_fields
    a = np.arange(2 * 6 * 5, dtype=np.float32).reshape(2, 6, 5)
    b = 1000 + np.arange(1 * 6 * 5, dtype=np.float32).reshape(1, 6, 5)
    out = _nuts_info_fields([a, np.zeros((0, 6, 0), np.float32), b])
    assert set(out) == set(NUTS_INFO_FIELDS)
    assert out['energy'].shape == (3, 5) and out['energy'][2, 0] == b[0, 4, 0]
    assert out['num_integration_steps'].dtype == np.int32 and out['is_divergent'].dtype == np.bool_

"""The problems of the per-leaf gradient checks, built from the fp64 restatements alone: tests/test_leafcheck_host.py asserts on
the CPU that every leaf of them is seen, tests/test_gpu_leaf_parity.py runs the HIP kernels on the same problems.

Attention models: the shapes of the `CASES` lists of tests/test_gpu_attn.py and tests/test_gpu_attn_pre.py with
`sharp_problem` (sharp attention) under a prior so wide that every leaf's gradient is the likelihood's.  FCN: the depth-ablation
cases of tests/test_gpu_parity.py and the deep third of its random specs, with the standard prior; the size of the parameters
(then the activation, then further draws of the data and parameters) is searched in a fixed order until the likelihood gradient
reaches every layer of every chain.  The search reads the fp64 oracle only, never a kernel's output.
"""
from __future__ import annotations

import numpy as np

from tests import attn_pre_ref as RP
from tests import attn_ref as RA
from tests import leafcheck as L

ATTN_PRIOR_SCALE = 1000.0         # prior gradient = -theta * 1e-6: below every leaf's likelihood gradient (asserted, share >= 0.5)
KEY_BIAS = 'MDPA.key.bias'        # likelihood gradient zero analytically (softmax is shift-invariant per query row) ...
SCALE_OF = {KEY_BIAS: 'MDPA.query.bias'}      # ... so it is compared absolutely, on the scale of the query bias of the same chain
MIN_SHARE = 0.5                   # max |likelihood gradient| / max |gradient| per leaf
SEED = 3


def attn_cases():
    from tests.test_gpu_attn import CASES
    return list(CASES)


def attn_pre_cases():
    from tests.test_gpu_attn_pre import CASES
    return list(CASES)


def attn_spec(kind, V, T, C, H, D, K, proj, bias, prior_scale=ATTN_PRIOR_SCALE):
    from mile_amd.spec import AttentionSpec, PretrainedAttentionSpec
    cls = AttentionSpec if kind == 'attn' else PretrainedAttentionSpec
    return cls(V, T, C, H, D, n_classes=K, projection_dim=proj, use_bias=bias, prior='Normal', prior_scale=prior_scale)


class AttnProblem:
    """One attention problem and its restatement: `ref(dtype)` -> (logp [E], grad [E, d]), `lik()` -> likelihood gradient [E, d]."""

    def __init__(self, kind, spec, prob):
        self.kind, self.spec, self.prob = kind, spec, prob
        self.leaves = L.spec_leaves(spec)
        self.scale_of = SCALE_OF if spec.use_bias else None

    def _args(self, x=None, y=None):
        p = self.prob
        x, y = (p['x'] if x is None else x), (p['y'] if y is None else y)
        return (p['emb'], p['pos'], x, y) if self.kind == 'pre' else (x, y)

    def ref(self, dtype=np.float64, rows=slice(None), mutant=None, theta=None):
        R = RP if self.kind == 'pre' else RA
        th = self.prob['theta0'] if theta is None else theta
        return R.logpost_and_grad(self.spec, th, *self._args(self.prob['x'][rows], self.prob['y'][rows]), dtype=dtype, mutant=mutant)

    def lik(self, rows=slice(None)):
        R = RP if self.kind == 'pre' else RA
        return R.loglik_grad(self.spec, self.prob['theta0'], *self._args(self.prob['x'][rows], self.prob['y'][rows]))

    def stats(self):
        """attention_stats per chain."""
        p = self.prob
        if self.kind == 'pre':
            Ps = [RP.params(self.spec, t, p['emb'], p['pos']) for t in p['theta0']]
        else:
            Ps = [RA.unpack(self.spec, t) for t in p['theta0']]
        return [RA.attention_stats(self.spec, P, p['x']) for P in Ps]

    def bound(self, g_ref, rows=slice(None), theta=None):
        """Per chain and leaf: 5e-5, or 8x the float32 restatement's own error where that is larger (tests/leafcheck.py)."""
        _, g32 = self.ref(np.float32, rows, theta=theta)
        return L.leaf_bounds(self.leaves, g_ref.shape[0], g32, g_ref, self.scale_of)

    def engine(self, X=None, y=None):
        import torch
        from mile_amd.engine import Engine
        p = self.prob
        X, y = (p['X'] if X is None else X), (p['y'] if y is None else y)
        kw = {'tables': (p['emb'], p['pos'])} if self.kind == 'pre' else {}
        eng = Engine(self.spec, torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(np.ascontiguousarray(y)), device='cuda:0', **kw)
        assert eng.grad_kernel == ('attn_pre_f32' if self.kind == 'pre' else 'attn_f32')
        return eng


def attn_problem(kind, V, T, C, H, D, K, proj, bias, N, E, seed=SEED, sharp=True, prior_scale=None):
    """sharp=True: the new problem (sharp attention, wide prior); False: the one tests/test_gpu_attn*.py use (prior_scale 0.2)."""
    spec = attn_spec(kind, V, T, C, H, D, K, proj, bias, (ATTN_PRIOR_SCALE if sharp else 0.2) if prior_scale is None else prior_scale)
    R = RP if kind == 'pre' else RA
    prob = R.sharp_problem(spec, N, E, seed, QK_SCALE.get((V, T, C, H, D))) if sharp else R.synthetic_problem(spec, N, E, seed=seed)
    return AttnProblem(kind, spec, prob)


# the row-split / row-window problem of test_row_splits_and_windows in both attention test files (N = 600: E = 1, 2, 4 give different
# row ranges), and a data set with fewer rows than row ranges
STEP_SHAPES = {'attn': (40, 12, 16, 4, 16, 2, (8,), False), 'pre': (40, 12, 40, 4, 16, 2, (8,), False)}     # test_mclmc_steps_match_oracle's
# sharp_problem's scale on the query and key kernels where its default sqrt(2 C) is not enough: one row of five real keys needs
# larger scores before one weight falls to 1e-6 of its row's largest
QK_SCALE = {(17, 11, 8, 2, 8): 6.0}
SPLIT_SHAPES = {'attn': (300, 24, 32, 4, 32, 2, (16,), True), 'pre': (300, 24, 40, 4, 32, 2, (16,), True)}


# ---- deep FCN ----------------------------------------------------------------------------------------------------------------

DEEP_FCN = [
    # F, hidden, activation, task, N, E: the depth ablations of tests/test_gpu_parity.py's CASES whose first layers the whole-vector
    # criterion does not see
    (6, (12,) * 10 + (4,), 'sigmoid', 'classification', 90, 2),
    (8, (8,) * 6 + (2,), 'relu', 'regr', 203, 2),
    (13, (16,) * 9 + (2,), 'tanh', 'regr', 150, 2),
]
THETA_LADDER = (0.1, 0.2, 0.3, 0.5, 0.7, 1.0, 1.4, 2.0)
ACTIVATIONS = ('relu', 'tanh', 'sigmoid')
SEED_TRIES = 40                  # further draws of the data and parameters (seed + 1000 k), after every activation and scale


def random_deep_specs():
    """The deep third (4-10 hidden layers) of test_narrow_kernel_on_random_specs: the same draws in the same order."""
    rng = np.random.default_rng(2024)
    out = []
    for it in range(30):
        deep = it % 3 == 2
        nh = int(rng.integers(4, 11)) if deep else int(rng.integers(1, 4))
        wmax = 16 if deep else 32
        F = int(rng.integers(1, 17 if deep else 65))
        hidden = tuple(int(rng.integers(1, wmax + 1)) for _ in range(nh))
        task = 'regr' if rng.random() < 0.5 else 'classification'
        K = 2 if task == 'regr' else int(rng.integers(2, 17))
        act = ('relu', 'tanh', 'sigmoid')[int(rng.integers(0, 3))]
        N, E = int(rng.integers(1, 400)), int(rng.integers(1, 8))
        if deep:
            out.append((F, hidden + (K,), act, task, N, E, 100 + it))
    return out


def deep_fcn_cases():
    return [c + (SEED,) for c in DEEP_FCN] + random_deep_specs()


def _fcn_eval(ospec, prob):
    from oracle import mclmc_oracle as M
    th = prob['theta0'].astype(np.float64)
    lp, g = M.logpost_and_grad(ospec, th, prob['X'], prob['y'])
    return lp, g, g - M.log_prior(ospec, th)[1]


def deep_fcn_problem(F, hs, act, task, N, E, seed):
    """(ospec, prob, logp_ref, g_ref, g_lik_ref, (activation, theta_scale, seed)) with the standard prior: the first draw (the
    case's own seed first), activation (the case's own first) and scale (THETA_LADDER in order) for which every leaf of every chain has
    max |likelihood gradient| >= MIN_SHARE * max |gradient|, judged on the fp64 oracle alone.  Rows with a ReLU pre-activation
    within fp32 rounding of the kink are left out, as in tests/test_gpu_parity.py."""
    from oracle import mclmc_oracle as M
    best = None
    for sd, a in [(seed + 1000 * k, a) for k in range(SEED_TRIES) for a in (act,) + tuple(x for x in ACTIVATIONS if x != act)]:
        ospec = M.ModelSpec(F, hs, activation=a, task=task)
        leaves = L.fcn_leaves(ospec)
        for ts in THETA_LADDER:
            prob = M.synthetic_problem(ospec, N, E, seed=sd, theta_scale=ts)
            if a == 'relu':
                _, zs, _ = M.mlp_forward(ospec, prob['theta0'].astype(np.float64), prob['X'], keep=True)
                near = np.zeros(N, dtype=bool)
                for z in zs[:-1]:
                    near |= (np.abs(z) < 3e-7 * max(np.abs(z).max(), 1e-30)).any(axis=(0, 2))
                if near.any() and near.sum() < N:
                    prob = dict(prob, X=np.ascontiguousarray(prob['X'][~near]), y=np.ascontiguousarray(prob['y'][~near]))
            lp, g, gl = _fcn_eval(ospec, prob)
            share = L.likelihood_share(gl, g, leaves).min()
            if best is None or share > best[0]:
                best = (share, a, ts, sd)
            if share >= MIN_SHARE:
                return ospec, prob, lp, g, gl, (a, ts, sd)
    raise AssertionError(f'no (activation, theta_scale) gives every leaf a likelihood share >= {MIN_SHARE}: best {best} for {(F, hs, act, task, N, E, seed)}')

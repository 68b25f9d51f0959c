"""The cases that the host and the device tests of the input sensitivities share, and their inputs.  Inputs as in
tests/test_gpu_moments.py: synthetic_problem(..., seed=3, theta_scale) for theta [C * S, d], seed=4 for X [N, F]."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import mclmc_oracle as O
from tests import sens_ref as R


@dataclass(frozen=True)
class Case:
    id: str
    F: int
    hs: tuple
    act: str
    task: str
    N: int
    C: int
    S: int
    what: str
    theta_scale: float = 0.3
    theta_seed: int = 3
    x_seed: int = 4


CASES = [
    Case('1-stock', 5, (16, 16, 2), 'relu', 'regr', 70, 1, 7, 'the stock net; ragged last pass and last tile'),
    Case('2-softmax', 7, (40, 40, 3), 'tanh', 'classification', 130, 2, 3, 'the softmax head, per-chain outputs'),
    Case('3-k7', 11, (32, 7), 'sigmoid', 'classification', 130, 1, 5, 'one hidden layer, K = 7'),
    Case('4-b2', 5, (64, 64, 64, 2), 'relu', 'regr', 70, 2, 3, "B2's net, smaller row tiles"),
    Case('5-deep', 8, (16,) * 8 + (2,), 'relu', 'regr', 70, 1, 7, 'nine layers of sweeps'),
    Case('6-wide', 9, (128, 128, 2), 'relu', 'regr', 70, 1, 5, 'widths beyond a wave, fewest rows per tile'),
    Case('7-f70', 70, (8, 2), 'tanh', 'regr', 40, 1, 3, 'more than 64 inputs: P * F = 140 columns'),
    Case('8-linear', 5, (2,), 'relu', 'regr', 33, 2, 2, 'no hidden layer: J is W_0 itself'),
]
BY_ID = {c.id: c for c in CASES}
RELU_CASES = [c for c in CASES if c.act == 'relu' and len(c.hs) > 1]


def ospec_of(case):
    return O.ModelSpec(case.F, case.hs, activation=case.act, task=case.task)


@lru_cache(maxsize=None)
def problem(case_id):
    """(ospec, prob, theta [C * S, d] fp32, X [N, F] fp32) of a case; prob is the training problem an Engine is made on.  Cached:
    the arrays are shared, nobody writes to them."""
    case = BY_ID[case_id]
    ospec = ospec_of(case)
    prob = O.synthetic_problem(ospec, 64, case.C * case.S, seed=case.theta_seed, theta_scale=case.theta_scale)
    X = O.synthetic_problem(ospec, case.N, 1, seed=case.x_seed)['X']
    for a in (prob['theta0'], X):
        a.setflags(write=False)
    return ospec, prob, prob['theta0'], X


@lru_cache(maxsize=None)
def reference(case_id):
    """What the tests of a case compare against, computed once: the fp64 Jacobians and statistics, those of the float32
    restatement of the Jacobian chain, and for a ReLU case the rows whose masks rounding may change (else none)."""
    case = BY_ID[case_id]
    ospec, _, theta, X = problem(case_id)
    raw64, J64, _ = R.jacobians(ospec, theta, X)
    raw32, J32, _ = R.jacobians(ospec, theta, X, dtype=np.float32)
    near = R.relu_rows_near_zero(ospec, theta, X) if case in RELU_CASES else np.zeros(case.N, dtype=bool)
    return {'raw64': raw64, 'J64': J64, 'raw32': raw32, 'J32': J32, 'near': near}

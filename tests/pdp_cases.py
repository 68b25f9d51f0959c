"""The cases that the host and the device tests of partial dependence share.  The problems are those of tests/sens_cases.py,
by import: the same nets, seeds, N <= 130 and C * S <= 7 -- the smallest shapes that still exercise a ragged pass, a ragged tile,
widths beyond a wave, F > 64, a deep net and both heads.  Per case Fs = 3 features and G = 5 grid values, metrics.pd_grid at the
5 % - 95 % quantiles of the case's own table."""
from functools import lru_cache

import numpy as np

from tests import pdp_ref as R
from tests import sens_cases as SC

CASES = SC.CASES
BY_ID = SC.BY_ID
problem = SC.problem
G = 5


def features_of(case_id):
    """The first, an inner and the last input; for F = 70 one on each side of a wave's 64."""
    F = BY_ID[case_id].F
    return (0, 33, 69) if case_id == '7-f70' else (0, 2, F - 1)


@lru_cache(maxsize=None)
def grid_of(case_id):
    """[Fs, G] fp32, read-only: shared, nobody writes to it."""
    from mile_amd import metrics as M
    _, _, _, X = problem(case_id)
    g = M.pd_grid(X, features_of(case_id), G).numpy()
    g.setflags(write=False)
    return g


@lru_cache(maxsize=None)
def reference(case_id):
    """What the tests of a case compare against, computed once: h [C * S, N, Fs, G, P] of the update form in fp64 and in float32,
    and of the substitute form in fp64 and in float32."""
    ospec, _, theta, X = problem(case_id)
    f, g = features_of(case_id), grid_of(case_id)
    res = {'h64': R.values(ospec, theta, X, f, g), 'h32': R.values(ospec, theta, X, f, g, dtype=np.float32),
           'sub64': R.values(ospec, theta, X, f, g, form='substitute'),
           'sub32': R.values(ospec, theta, X, f, g, dtype=np.float32, form='substitute')}
    for a in res.values():
        a.setflags(write=False)
    return res

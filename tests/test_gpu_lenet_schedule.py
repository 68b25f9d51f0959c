"""The LeNet gradient paths over every cell of run_lenet's launch schedule (-m gpu): lenet_f32 in its direct and its im2col + SGEMM
form, lenet_bf16 and lenet_bf16x3 on the cases of tests/lenet_schedule.py.  tests/test_lenet_schedule_host.py proves on the CPU
that the table reaches every cell, that every leaf's gradient is at least half the likelihood's (all of it under the wide prior
that most cases have) and that a schedule that is wrong in one of six ways misses the per-leaf bound below by more than 10x.

lenet_f32 (both forms) and lenet_bf16x3 against oracle.lenet_oracle.logpost_and_grad in fp64: logp 2e-5 relative, every leaf of
every chain 5e-5 of its own largest entry, or 8x the float32 oracle's own error where that is larger (tests/leafcheck.py; a leaf
that takes the 8x branch is printed).  lenet_bf16 against logpost_and_grad_bf16: logp 1e-4, the gradient 1e-3 in norm, every leaf
3e-3 of its largest entry, or 8x the error of the same recipe evaluated in float32 where that is larger -- the rounding-boundary
flip test_lenet_mfma_convolutions_match_the_bf16_recipe describes.  Nothing in a bound comes from a kernel.  Every particle beyond
the first two repeats particle 0's or 1's parameters and must repeat its result bit for bit.

Each test prints what it measured before it asserts (`pytest -s`, lines LENETSCHED), and the module prints the worst leaf per back
end at its end (LENETWORST); profiles/r10/01_lenet_schedule.md keeps the figures of an MI355X."""
import re
from contextlib import contextmanager
from functools import lru_cache

import numpy as np
import pytest

from oracle import lenet_oracle as LN
from oracle import mclmc_oracle as O
from tests import leafcheck as L
from tests import lenet_schedule as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
LP_TOL = 2e-5            # relative: tests/test_gpu_lenet.py, tests/test_gpu_lenet_bf16x3.py
BF16_LP_TOL = 1e-4       # test_lenet_mfma_convolutions_match_the_bf16_recipe
BF16_LEAF_TOL = 3e-3
BF16_NORM_TOL = 1e-3
PREDICT_TOL = {S.F32: 1e-4, S.X3: 1e-4, S.BF16: 2e-3}     # tests/test_gpu_predict.py: of max(1, max |ref|)
_WORST = {}              # back end -> [leaf error / bound, leaf error, float32 restatement's, case, leaf]


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    for b, (ratio, err, err32, name, leaf) in sorted(_WORST.items()):
        print(f'\nLENETWORST {b:<12s} worst leaf {err:.2e} ({ratio:.3f} of its bound; float32 restatement {err32:.2e}) in {leaf} of {name}')


@contextmanager
def _env(case):
    """MILE_GEMM_ROWS and MILE_LENET_GEMM of the case, for the engines made and launched inside (run_lenet reads both per call)."""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in (('MILE_GEMM_ROWS', case.chunk_rows), ('MILE_LENET_GEMM', 1 if case.gemm_env else None)):
            if v is None:
                mp.delenv(k, raising=False)
            else:
                mp.setenv(k, str(int(v)))
        yield


def _engine(case, X, y):
    from mile_amd import LeNetSpec
    from mile_amd.engine import Engine
    o = S.ospec_of(case)
    spec = LeNetSpec(o.channels, o.height, o.width, o.out_dim, activation=o.activation, task=o.task, prior=o.prior, prior_loc=o.prior_loc,
                     prior_scale=o.prior_scale)
    assert [(n, a, tuple(s)) for n, a, s in spec.leaves()] == [(n, a, tuple(s)) for n, a, s in o.leaves()]
    eng = Engine(spec, torch.from_numpy(np.ascontiguousarray(X)), torch.from_numpy(np.ascontiguousarray(y)), device=DEV, grad_kernel=case.kernel)
    assert eng.grad_kernel == case.kernel
    return eng


def _launch(eng, theta):
    lp, g = eng.logpost_grad(torch.from_numpy(theta))
    torch.cuda.synchronize()
    return lp.cpu(), g.cpu()


def _differ(lp, g):
    """Particles beyond the first two that do not repeat their chain bit for bit."""
    return [e for e in range(2, lp.shape[0]) if not (torch.equal(lp[e], lp[e % 2]) and torch.equal(g[e], g[e % 2]))]


def _where(case):
    p = S.plan(case)
    w = ' '.join(f"{Rc}/{nwg}wg/{last}{'+' if acc else ''}" for Rc, nwg, last, acc in p['walk'])
    if case.kernel == S.F32:
        form = f"direct geo {p['geo']} G {p['dw1']['G']}" if p['direct'] else f"gemm ({p['reason']})"
    else:
        form = 'ni ' + '/'.join(str(p['ni'][k]) for k in S.KINDS)
    return f'{form}, chunks {w}'


def _check(case, where, lp, g):
    """logp and every leaf of the first min(E, 2) particles against the case's reference, at the case's kernel's bounds."""
    n = min(case.E, 2)
    lp_ref, g_ref, g32 = (a[:n] for a in S.reference_of(case))
    leaves = L.spec_leaves(S.ospec_of(case))
    bf16 = case.kernel == S.BF16
    bound = L.leaf_bounds(leaves, n, g32=g32, g_ref=g_ref, tol=BF16_LEAF_TOL if bf16 else L.LEAF_TOL, margin=L.F32_MARGIN)
    lp, g = np.asarray(lp, np.float64)[:n], np.asarray(g, np.float64)[:n]
    e_lp = np.abs(lp - lp_ref).max() / np.abs(lp_ref).max()
    err, err32 = L.leaf_errors(g, g_ref, leaves), L.leaf_errors(g32, g_ref, leaves)
    nrm = (np.linalg.norm(g - g_ref, axis=1) / np.linalg.norm(g_ref, axis=1)).max()
    c, j = np.unravel_index(int((err / bound).argmax()), err.shape)
    base = BF16_LEAF_TOL if bf16 else L.LEAF_TOL
    wider = sorted({leaves[jj][0] for jj in np.nonzero((bound > base).any(axis=0))[0]})
    print(f'\nLENETSCHED {case.name} [{where}]: logp {e_lp:.2e}  norm {nrm:.2e}  worst leaf {err[c, j]:.2e} in {leaves[j][0]} '
          f'(float32 restatement {err32.max():.2e}, bound {bound.min():.2e}..{bound.max():.2e})'
          + (f'  8x branch: {wider}' if wider else ''))
    b = S.backend_of(case)
    if b not in _WORST or err[c, j] / bound[c, j] > _WORST[b][0]:
        _WORST[b] = [float(err[c, j] / bound[c, j]), float(err[c, j]), float(err32[c, j]), case.name, leaves[j][0]]
    assert np.isfinite(lp).all() and np.isfinite(g).all(), (case.name, where)
    assert e_lp < (BF16_LP_TOL if bf16 else LP_TOL), (case.name, where, e_lp)
    if bf16:
        assert nrm < BF16_NORM_TOL, (case.name, where, nrm)
    L.assert_leaves(g, g_ref, leaves, bound, tag=(case.name, where))


@lru_cache(maxsize=None)
def _run(case):
    _, X, y, theta = S.problem(case)
    with _env(case):
        lp, g = _launch(_engine(case, X, y), theta)
    return lp, g


# ---- the full data set ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', S.FULL_CASES, ids=lambda c: c.name)
def test_every_cell_of_the_schedule(case):
    lp, g = _run(case)
    _check(case, _where(case), lp, g)
    assert not _differ(lp, g), (case.name, 'particles that differ from their chain')


@pytest.mark.parametrize('name', ['f32-walk-20+17', 'gemm-walk-20+17', 'bf16-walk-20+17', 'x3-walk-20+17', 'x3-walk-18+18+1', 'f32-walk-18+18+1'])
def test_chunked_and_unchunked_both_meet_the_oracle(name):
    """The same problem walked in chunks and at once: each against the oracle at the full bound, not against the other; what
    they differ by is printed."""
    case = S.BY_NAME[name]
    whole = case._replace(name=case.name + '-unchunked', chunk_rows=None)
    assert len(S.walk(case)) > 1 and len(S.walk(whole)) == 1
    lp, g = _run(case)
    lp1, g1 = _run(whole)
    _check(whole, _where(whole), lp1, g1)
    _check(case, _where(case), lp, g)
    print(f'LENETSCHED {name}: chunked against unchunked {float((g - g1).abs().max() / g1.abs().max()):.2e} of the largest entry')


# ---- row windows ----------------------------------------------------------------------------------------------------------------

def _window_bases():
    out = []
    for c in S.WINDOW_CASES:
        if S.base_of(c) not in out:
            out.append(S.base_of(c))
    return out


@pytest.mark.parametrize('base', _window_bases(), ids=lambda c: c.name)
def test_row_windows_and_the_full_set_behind_them(base):
    """All windows of one base case in turn on one engine, each against the oracle on its rows; then count = 0: the first full-set
    result bit for bit."""
    _, X, y, theta = S.problem(base)
    with _env(base):
        eng = _engine(base, X, y)
        full = _launch(eng, theta)
        _check(base, 'full set before the windows', *full)
        for case in (c for c in S.WINDOW_CASES if S.base_of(c) == base):
            eng.set_row_window(*case.window)
            lp, g = _launch(eng, theta)
            _check(case, f'rows {case.window[0]}+{case.window[1]}: ' + _where(case), lp, g)
            assert not _differ(lp, g), case.name
        eng.set_row_window(0, 0)
        lp, g = _launch(eng, theta)
    assert torch.equal(lp, full[0]) and torch.equal(g, full[1]), base.name


# ---- evaluation: more samples than one block --------------------------------------------------------------------------------------

@pytest.mark.parametrize('kernel', [S.F32, S.BF16, S.X3])
def test_evaluation_over_two_sample_blocks(kernel):
    """S = 257 samples on three 12 x 12 images: loglik_lenet's second block is one sample at s0 = 256.  pointwise_loglik and
    predict, each block against the oracle (lenet_bf16: the oracle with bf16-rounded convolution operands) at the bounds of
    tests/test_gpu_predict.py: 1e-4 of max(1, max |ref|), 2e-3 for lenet_bf16."""
    n_s = S.EVAL_BLOCK + 1
    case = S._c('eval', 1, 12, 12, K=3, act='tanh', N=3, kernel=kernel)
    ospec = S.ospec_of(case)
    prob = LN.synthetic_problem(ospec, 3, n_s, seed=0)
    th64 = prob['theta0'].astype(np.float64)
    out_ref = LN.forward(ospec, th64, prob['X'], q=O.bf16_round if kernel == S.BF16 else LN._same)
    ll_ref = O.pointwise_loglik(ospec, out_ref, prob['y'])[0]
    eng = _engine(case, prob['X'], prob['y'])
    theta = torch.from_numpy(prob['theta0'])
    pw = eng.pointwise_loglik(theta, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']))
    out = eng.predict(theta, torch.from_numpy(prob['X']))
    torch.cuda.synchronize()
    assert tuple(pw.shape) == (n_s, 3) and tuple(out.shape) == (n_s, 3, 3)
    pw, out = pw.cpu().numpy().astype(np.float64), out.cpu().numpy().astype(np.float64)
    tol = PREDICT_TOL[kernel]
    for tag, got, ref in (('pointwise_loglik', pw, ll_ref), ('predict', out, out_ref)):
        blocks = [np.abs(got[sl] - ref[sl]).max() for sl in (slice(0, S.EVAL_BLOCK), slice(S.EVAL_BLOCK, n_s))]
        print(f'\nLENETSCHED eval {kernel} {tag}: samples 0..255 {blocks[0]:.2e}, sample 256 {blocks[1]:.2e} (bound {tol * max(1.0, np.abs(ref).max()):.2e})')
        assert np.isfinite(got).all()
        for e in blocks:
            assert e < tol * max(1.0, np.abs(ref).max()), (kernel, tag, blocks)


# ---- what the library refuses -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kernel', S.MFMA)
def test_five_channels_are_refused_on_the_mfma_forms(kernel):
    """The cells ('channels', kernel, 5) of tests/lenet_schedule.py: refused when the kernel is chosen, an error and no other
    kernel in its place."""
    from mile_amd._lib import MileHipError
    case = S._c('five', 5, 16, 16, kernel=kernel)
    assert ('channels', kernel, 5) in S.UNREACHABLE and S.mfma_refused(5, 16, 16, 3 if kernel == S.X3 else 1)
    _, X, y, theta = S.problem(case)
    with pytest.raises(MileHipError, match=re.escape(S.MFMA_REFUSAL[kernel])):
        _launch(_engine(case, X, y), theta)

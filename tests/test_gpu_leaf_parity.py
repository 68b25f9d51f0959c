"""HIP gradients against the fp64 restatements leaf by leaf and chain by chain (-m gpu), on problems where every leaf's gradient
is the likelihood's (tests/leaf_cases.py; tests/test_leafcheck_host.py proves that on the CPU).  Every leaf is held to 5e-5 of its
own largest entry; `MDPA.key.bias`, zero analytically, is held to the query bias's scale.  Each test prints what it measured
before it asserts (`pytest -s`), next to the error of the float32 evaluation of the same restatement on the CPU: the device's
worst leaf is 1.7e-5 (the atomically accumulated embedding table at the reference's shape, float32 restatement 2.7e-5), every
other leaf is below 1.2e-5 and no leaf needed the wider 8x-float32 bound that tests/leafcheck.py offers, so it is not used here.
profiles/r05/01_leaf_parity.md records the run."""
import numpy as np
import pytest

from tests import leaf_cases as LC
from tests import leafcheck as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


def _report(tag, leaves, err, err32, bound):
    print(f'\nLEAFPARITY {tag}')
    for j, (n, _, _) in enumerate(leaves):
        print(f'LEAF {n:<48s} device {err[:, j].max():.2e}  float32 restatement {err32[:, j].max():.2e}  bound {bound[:, j].min():.2e}')


def _check_attn(P, lp, g, tag, rows=slice(None), theta=None, reps=1):
    """Log-density 2e-5 relative, gradient per leaf; `reps`: the ensemble is the problem's repeated."""
    lp_ref, g_ref = P.ref(rows=rows, theta=theta)
    _, g32 = P.ref(np.float32, rows, theta=theta)
    lp_ref, g_ref, g32 = np.tile(lp_ref, reps), np.tile(g_ref, (reps, 1)), np.tile(g32, (reps, 1))
    bound = np.full((g_ref.shape[0], len(P.leaves)), L.LEAF_TOL)
    g = g.cpu().numpy().astype(np.float64)
    _report(tag, P.leaves, L.leaf_errors(g, g_ref, P.leaves, P.scale_of), L.leaf_errors(g32, g_ref, P.leaves, P.scale_of), bound)
    if lp is not None:
        lp = lp.cpu().numpy().astype(np.float64)
        assert np.abs(lp - lp_ref).max() < 2e-5 * max(1.0, np.abs(lp_ref).max()), (tag, lp, lp_ref)
    L.assert_leaves(g, g_ref, P.leaves, bound, P.scale_of, tag=tag)


ATTN = [('attn',) + c for c in LC.attn_cases()] + [('pre',) + c for c in LC.attn_pre_cases()]


@pytest.mark.parametrize('kind,V,T,C,H,D,K,proj,bias,N,E', ATTN)
def test_attention_gradient_per_leaf(kind, V, T, C, H, D, K, proj, bias, N, E):
    P = LC.attn_problem(kind, V, T, C, H, D, K, proj, bias, N, E)
    eng = P.engine()
    lp, g = eng.logpost_grad(torch.from_numpy(P.prob['theta0']))
    torch.cuda.synchronize()
    _check_attn(P, lp, g, (kind, V, T, C, H, D, K, proj, bias, N, E))


@pytest.mark.parametrize('kind', ['attn', 'pre'])
def test_attention_row_splits_and_windows_per_leaf(kind):
    """Ensembles of 1, 2 and 4 chains split N = 600 rows into different ranges (the slab reduction and, for the AttentionClassifier,
    the atomically accumulated embedding block are per leaf too); a row window; fewer rows than row ranges."""
    shape = LC.SPLIT_SHAPES[kind]
    P = LC.attn_problem(kind, *shape, 600, 2, seed=4)
    eng = P.engine()
    th = torch.from_numpy(P.prob['theta0'])
    _check_attn(P, *eng.logpost_grad(th), (kind, 'N 600', 'E 2'))
    lp1, g1 = eng.logpost_grad(th[:1])
    P1 = LC.AttnProblem(kind, P.spec, dict(P.prob, theta0=P.prob['theta0'][:1]))
    _check_attn(P1, lp1, g1, (kind, 'N 600', 'E 1'))
    _check_attn(P, *eng.logpost_grad(th.repeat(2, 1)), (kind, 'N 600', 'E 4'), reps=2)
    b, c = 100, 77
    eng.set_row_window(b, c)
    lpw, gw = eng.logpost_grad(th)
    eng.set_row_window(0, 0)
    _check_attn(P, lpw, gw, (kind, 'window', b, c), rows=slice(b, b + c))
    small = LC.attn_problem(kind, *shape, 3, 2, seed=5)
    if kind == 'pre':
        small.prob['emb'], small.prob['pos'] = P.prob['emb'], P.prob['pos']
    eng.set_data(torch.from_numpy(small.prob['X']), torch.from_numpy(small.prob['y']))
    _check_attn(small, *eng.logpost_grad(torch.from_numpy(small.prob['theta0'])), (kind, 'N 3', 'E 2'))
    torch.cuda.synchronize()


@pytest.mark.parametrize('kind', ['attn', 'pre'])
def test_attention_mclmc_step_gradient_per_leaf(oracle, kind):
    """One MCLMC step with explicit noise from the sharp problem: the position against the oracle's step, and the state's
    `logdensity_grad` per leaf against the restatement at the device's own new position (so that the comparison is the kernel's
    gradient inside the step launch, not the fp32 position's rounding carried through the Hessian)."""
    P = LC.attn_problem(kind, *LC.STEP_SHAPES[kind], 48, 3, seed=9)
    prob, d, E = P.prob, P.spec.n_params, 3
    rng = np.random.default_rng(4)
    z0 = rng.standard_normal((E, d)).astype(np.float32)
    noise = rng.standard_normal((1, 2, E, d)).astype(np.float32)
    f = lambda th: P.ref(theta=th)     # noqa: E731
    st = oracle.mclmc_init(f, prob['theta0'].astype(np.float64), z0.astype(np.float64))
    st, _ = oracle.mclmc_step(f, st, prob['eps'].astype(np.float64), prob['L'].astype(np.float64), noise[0, 0].astype(np.float64),
                              noise[0, 1].astype(np.float64))
    eng = P.engine()
    s = eng.init(torch.from_numpy(prob['theta0']), noise=torch.from_numpy(z0))
    _check_attn(P, s.logdensity, s.logdensity_grad, (kind, 'mclmc init'))
    s, _, _ = eng.step(s, torch.from_numpy(prob['eps']), torch.from_numpy(prob['L']), n_steps=1, noise=torch.from_numpy(noise))
    torch.cuda.synchronize()
    pos = s.position.cpu().numpy()
    assert np.abs(pos - st.position).max() < 1e-4 * np.abs(st.position).max()
    assert np.abs(pos - prob['theta0']).max() > 0
    _check_attn(P, s.logdensity, s.logdensity_grad, (kind, 'mclmc step'), theta=pos)


@pytest.mark.parametrize('F,hs,act,task,N,E,seed', LC.deep_fcn_cases())
def test_deep_fcn_gradient_per_leaf(oracle, F, hs, act, task, N, E, seed):
    """k_grad_narrow's depth-ablation templates (4-10 hidden layers) and the generic kernel, standard prior, on parameters for which
    the likelihood gradient reaches layer 0 (tests/leaf_cases.py's search on the fp64 oracle)."""
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    ospec, prob, lp_ref, g_ref, _, chosen = LC.deep_fcn_problem(F, hs, act, task, N, E, seed)
    leaves = L.fcn_leaves(ospec)
    _, g32 = oracle.logpost_and_grad(ospec, prob['theta0'], prob['X'], prob['y'])
    assert g32.dtype == np.float32
    bound = np.full((g_ref.shape[0], len(leaves)), L.LEAF_TOL)
    spec = ModelSpec(in_features=F, hidden_structure=hs, activation=ospec.activation, task=task)
    for k in ('mfma_narrow_f32', 'generic'):
        eng = Engine(spec, torch.from_numpy(prob['X']), torch.from_numpy(prob['y']), device='cuda:0', grad_kernel=k)
        assert eng.grad_kernel == k
        lp, g = eng.logpost_grad(torch.from_numpy(prob['theta0']))
        torch.cuda.synchronize()
        lp, g = lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
        _report((k, F, hs, task, N, E) + chosen, leaves, L.leaf_errors(g, g_ref, leaves), L.leaf_errors(g32, g_ref, leaves), bound)
        assert np.abs(lp - lp_ref).max() < 2e-5 * np.abs(lp_ref).max(), k
        L.assert_leaves(g, g_ref, leaves, bound, tag=(k, F, hs, task, N, E) + chosen)

"""Every likelihood head where sigma clips and softmax saturates (-m gpu): the HIP kernels on the steered ensembles of
tests/head_cases.py against the fp64 restatements, chain by chain (the `lo` chain's gradient of order 1e12 must not hide the
others).  tests/test_head_cases_host.py proves the cases' conditions and prints the float32-vs-fp64 yardstick on the CPU.

Bounds, per chain: max(the project's bound at benign inputs, 4 x the float32 restatement's error): 2e-5 for the log-posterior
and the whole gradient (5e-5 for LeNet, its own figure), 5e-5 per leaf, 1e-4 of max(1, max |ref|) for the pointwise
log-likelihood.  The float32 restatement loses less than 4e-6 anywhere in these cases, so the project's bounds are the ones that
hold, apart from a few leaves of the attention models.  Each test prints what it measured before it asserts (`pytest -s`).

Structural facts, whatever the operand precision (mfma_w128_bf16 included, whose values are not compared): in `hi` and `lo` the
gradient on the log-sigma output bias and kernel column is the prior's (1e-6 relative), in `hi` logp - prior = -N (T + 0.9189385)
to 1e-5.

Measured on an MI355X (worst over the case's kernels; error / bound).  Whole gradient, per chain, of its largest entry:

    case (kernels)                                      hi        lo        hi_edge   lo_edge   control   bound
    narrow_relu (generic, mfma_narrow_f32)              1.1e-12   5.3e-08   1.1e-07   6.8e-07   1.6e-07   2e-5
    narrow_tanh (generic, mfma_narrow_f32)              2.2e-12   1.9e-07   6.1e-08   4.3e-07   2.2e-07   2e-5
    w64 (mfma_w64, mfma_w64_bf16x3)                     4.0e-12   2.4e-07   8.0e-08   2.3e-07   1.8e-06   2e-5
    w64_two_quads (mfma_w64)                            4.0e-12   1.4e-07   7.5e-08   2.6e-07   4.6e-07   2e-5
    wide (gemm_f32, mfma_wide_bf16x3)                   4.1e-11   2.3e-07   1.8e-07   1.1e-06   2.1e-06   2e-5
    lenetti (lenetti_f32)                               2.6e-13   1.0e-07   6.7e-08   1.1e-06   1.2e-07   2e-5
    lenet (lenet_f32)                                   2.8e-13   2.0e-07   1.4e-07   2.6e-07   1.4e-07   5e-5

    case (kernels)                                      sat_pos   sat_neg   control   bound
    covertype_like (generic, narrow, gemm, wide x3)     1.2e-06   1.1e-06   2.1e-07   2e-5
    wide3 (mfma_wide_bf16x3, gemm_f32)                  5.4e-07   9.0e-07   4.0e-07   2e-5
    lenet (lenet_f32)                                   5.8e-06   5.1e-06   2.0e-07   5e-5
    lenetti (lenetti_f32)                               1.2e-06   1.6e-06   1.6e-07   2e-5
    attn / attn_wide / attn_pre                         8.7e-07   9.9e-07   8.6e-08   2e-5

logp: at most 2.0e-06 (gemm_f32, wide, control chain) against 2e-5.  Worst leaf: 1.9e-06 in the regression cases, 1.2e-05
(lenet_f32, sat_pos) and 1.8e-05 (attn_pre_f32, sat_neg) in the softmax cases, against 5e-5 or more.  The log-sigma column in hi
and lo equalled the prior's gradient bit for bit in every kernel, mfma_w128_bf16 included; logp - prior in hi was within 1.2e-06
of -N (T + 0.9189385) (lenet_f32 the largest).  Pointwise log-likelihood: at most 3.2e-06 of max(1, max |ref|) (gemm forward,
control chain; 1.5e-06 in a clipped chain) against 1e-4.  Aleatoric variance: 4.1e-09 off 1e12, 4.0e-09 off 1e-12, against 1e-6.
No head needed more than its project bound, so the 4 x float32 term decided nothing.

With the `unclipped` test of row_loss_regr forced to true, all eleven test_regression_head_gradient_in_the_clip cases fail; with
the clip constants of row_loglik swapped, test_pointwise_loglik_on_the_steered_chains[regr-narrow_relu-generic] and
[regr-w64-mfma_w64] fail; with the `- m` of k_grad_generic's softmax taken out,
test_softmax_head_gradient_when_saturated[cls-covertype_like-generic] fails; each time everything else in this file passes.
"""
import numpy as np
import pytest

from tests import head_cases as H
from tests import leafcheck as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'


def _spec(model):
    from mile_amd import LeNetSpec, LeNettiSpec, ModelSpec
    o = model.ospec
    if model.kind == 'fcn':
        return ModelSpec(in_features=o.in_features, hidden_structure=o.hidden_structure, activation=o.activation, task=o.task)
    if model.kind in ('lenet', 'lenetti'):
        cls = LeNetSpec if model.kind == 'lenet' else LeNettiSpec
        spec = cls(o.channels, o.height, o.width, o.out_dim, activation=o.activation, task=o.task)
        assert [(n, int(b), tuple(s)) for n, b, s in spec.leaves()] == [(n, int(b), tuple(s)) for n, b, s in o.leaves()]
        return spec
    return o


def _engine(case, kernel):
    from mile_amd.engine import Engine
    kw = {'tables': case.model.tables} if case.model.kind == 'attn_pre' else {}
    eng = Engine(_spec(case.model), torch.tensor(case.X), torch.tensor(case.y), device=DEV, grad_kernel=kernel, **kw)
    assert eng.grad_kernel == kernel and eng.d == case.model.d
    return eng


def _logpost_grad(case, kernel):
    eng = _engine(case, kernel)
    lp, g = eng.logpost_grad(torch.tensor(case.theta))
    torch.cuda.synchronize()
    lp, g = lp.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    assert np.isfinite(lp).all() and np.isfinite(g).all(), (case.name, kernel, 'non-finite output')
    return eng, lp, g


def _pairs(cases, prefix, faithful=True):
    return [(f'{prefix}-{n}', k.rstrip('*')) for n, (_, _, _, ks) in cases.items() for k in ks if k.endswith('*') != faithful]


def _check_values(case, kernel, lp, g):
    lp64, g64 = case.ref64
    b = H.bounds(case)
    el, eg = H.logp_error(lp, lp64), H.chain_error(g, g64)
    leaf = L.leaf_errors(g, g64, case.model.leaves, case.model.scale_of)
    print(f'\nHEADEDGE {case.name} {kernel}')
    for e, nm in enumerate(case.regimes):
        print(f'HEADEDGE   {nm:<8s} logp {el[e]:.2e} (bound {b["logp"][e]:.1e})  grad {eg[e]:.2e} (bound {b["grad"][e]:.1e})  '
              f'worst leaf {leaf[e].max():.2e} (smallest leaf bound {b["leaf"][e].min():.1e})')
    assert (el < b['logp']).all(), (case.name, kernel, 'logp', el, b['logp'])
    assert (eg < b['grad']).all(), (case.name, kernel, 'grad', eg, b['grad'])
    L.assert_leaves(g, g64, case.model.leaves, b['leaf'], case.model.scale_of, tag=(case.name, kernel))


def _check_structure(case, kernel, lp, g):
    lpp, gp = case.prior
    cols = case.sigma_columns()
    for nm in ('hi', 'lo'):
        e = case.chain(nm)
        d = np.abs(g[e, cols] - gp[e, cols])
        print(f'HEADEDGE   {case.name} {kernel} {nm}: log-sigma column vs the prior, worst {(d / np.maximum(np.abs(gp[e, cols]), 1e-300)).max():.2e}')
        assert (d <= 1e-6 * np.abs(gp[e, cols])).all(), (case.name, kernel, nm, 'the log-sigma column is not the prior\'s')
    for nm in ('hi_edge', 'lo_edge'):           # ... and there it is not
        e = case.chain(nm)
        assert np.abs(g[e, cols] - gp[e, cols]).max() > 1e-3 * np.abs(gp[e, cols]).max(), (case.name, kernel, nm)
    hi = case.chain('hi')
    want = -case.N * (H.T_CLIP + 0.9189385)
    rel = abs((lp[hi] - lpp[hi]) / want - 1.0)
    print(f'HEADEDGE   {case.name} {kernel} hi: logp - prior vs -N (T + 0.9189385): {rel:.2e}')
    assert rel < 1e-5, (case.name, kernel, lp[hi] - lpp[hi], want)


@pytest.mark.parametrize('name,kernel', _pairs(H.REGR_CASES, 'regr'))
def test_regression_head_gradient_in_the_clip(name, kernel):
    """row_loss_regr at each of its sites (generic, narrow, w64 block, gemm, both k_mm3 sites, lenetti, lenet): logp, the gradient
    and every leaf per chain against fp64, and the structural facts."""
    case = H.case(name)
    _, lp, g = _logpost_grad(case, kernel)
    _check_values(case, kernel, lp, g)
    _check_structure(case, kernel, lp, g)


@pytest.mark.parametrize('name,kernel', _pairs(H.REGR_CASES, 'regr', faithful=False))
def test_bf16_regression_head_structure_in_the_clip(name, kernel):
    """row_loss_regr_fast (mfma_w128_bf16): operands are bf16-rounded, so only the structural facts are checked."""
    case = H.case(name)
    _, lp, g = _logpost_grad(case, kernel)
    _check_structure(case, kernel, lp, g)


@pytest.mark.parametrize('name,kernel', _pairs(H.CLS_CASES, 'cls'))
def test_softmax_head_gradient_when_saturated(name, kernel):
    """The nine softmax heads with logits of +100 +- 200 and -300 +- 200: finite outputs, logp, the gradient and every leaf per chain
    against the model's fp64 restatement."""
    case = H.case(name)
    _, lp, g = _logpost_grad(case, kernel)
    _check_values(case, kernel, lp, g)


# one case per distinct forward kernel: k_fwd_generic, k_fwd_w64, the gemm forward, the mm3 forward, lenetti, and the forward-only
# heads of the other models
FORWARD = [('regr-narrow_relu', 'generic'), ('regr-w64', 'mfma_w64'), ('regr-wide', 'gemm_f32'), ('regr-wide', 'mfma_wide_bf16x3'),
           ('regr-lenetti', 'lenetti_f32'), ('regr-lenet', 'lenet_f32'),
           ('cls-covertype_like', 'generic'), ('cls-covertype_like', 'gemm_f32'), ('cls-covertype_like', 'mfma_wide_bf16x3'),
           ('cls-lenetti', 'lenetti_f32'), ('cls-lenet', 'lenet_f32'), ('cls-attn', 'attn_f32'), ('cls-attn_wide', 'attn_wide_f32'),
           ('cls-attn_pre', 'attn_pre_f32')]


@pytest.mark.parametrize('name,kernel', FORWARD)
def test_pointwise_loglik_on_the_steered_chains(name, kernel):
    """Engine.pointwise_loglik on the 61 evaluation rows against oracle.pointwise_lppd, per chain."""
    case = H.case(name)
    eng = _engine(case, kernel)
    pw = eng.pointwise_loglik(torch.tensor(case.theta), torch.tensor(case.Xt), torch.tensor(case.yt))
    torch.cuda.synchronize()
    pw = pw.cpu().numpy().astype(np.float64)
    assert pw.shape == (case.E, H.N_TEST) and np.isfinite(pw).all(), (name, kernel)
    err, bound = H.pw_error(pw, case.pw64), H.bounds(case)['pointwise_test']
    print(f'\nHEADEDGE pointwise {name} {kernel}: ' + '  '.join(f'{nm} {err[e]:.2e} (bound {bound[e]:.1e}, max |ref| {np.abs(case.pw64[e]).max():.1e})'
                                                               for e, nm in enumerate(case.regimes)))
    assert (err < bound).all(), (name, kernel, err, bound)


@pytest.mark.parametrize('kernel', ['generic', 'mfma_w64'])
@pytest.mark.parametrize('regime,want', [('hi', 1e12), ('lo', 1e-12)])
def test_predict_moments_aleatoric_in_the_clip(kernel, regime, want):
    """All S = 3 draws in one regime: the aleatoric column is clip(sigma)^2 = 1e12 / 1e-12 on every row to 1e-6 (fp64 accumulators); a
    clip applied after squaring, or not at all, gives 4e-18 or 2e17 instead."""
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    model, theta, Xt = H.moments_case(regime)
    o = model.ospec
    eng = Engine(ModelSpec(in_features=o.in_features, hidden_structure=o.hidden_structure), torch.tensor(Xt), torch.zeros(len(Xt)),
                 device=DEV, grad_kernel=kernel)
    assert eng.grad_kernel == kernel
    mom = eng.predict_moments(torch.tensor(theta), torch.tensor(Xt)).cpu().numpy().astype(np.float64)
    torch.cuda.synchronize()
    out = model.outputs(theta, Xt)
    assert mom.shape == (H.N_TEST, 3) and np.isfinite(mom).all()
    rel = np.abs(mom[:, 2] / want - 1.0).max()
    print(f'\nHEADEDGE moments {kernel} {regime}: aleatoric vs {want:.0e}: {rel:.2e}')
    assert rel < 1e-6, (kernel, regime, mom[:3])
    mu = out[..., 0]
    assert np.abs(mom[:, 0] - mu.mean(axis=0)).max() < 1e-4 * max(1.0, np.abs(mu).max())

"""What the per-leaf gradient checks see, proven without a GPU from the fp64 restatements alone: the problems of
tests/leaf_cases.py are likelihood-dominated leaf by leaf and make attention sharp; wrong gradients built from the restatement
itself pass the whole-vector criterion of DESIGN section 1 on the old problems and fail `leafcheck.assert_leaves` on the new."""
import numpy as np
import pytest

from tests import attn_ref as A
from tests import leaf_cases as LC
from tests import leafcheck as L

ATTN = [('attn',) + c for c in LC.attn_cases()] + [('pre',) + c for c in LC.attn_pre_cases()]
# the row-split problems (N = 600 and fewer rows than row ranges) and the MCLMC-step problems of tests/test_gpu_leaf_parity.py
ATTN_EXTRA = [(k,) + LC.SPLIT_SHAPES[k] + (600, 2, 4) for k in ('attn', 'pre')] + \
             [(k,) + LC.SPLIT_SHAPES[k] + (3, 2, 5) for k in ('attn', 'pre')] + \
             [(k,) + LC.STEP_SHAPES[k] + (48, 3, 9) for k in ('attn', 'pre')]


def _visible(P, g, gl, tag):
    share = L.likelihood_share(gl, g, P.leaves)
    blind = L.visibility(gl, g, P.leaves, L.LEAF_TOL)
    for j, (n, b, e) in enumerate(P.leaves):
        if n == LC.KEY_BIAS:
            # zero analytically: the restatement gives rounding, far below the query bias that scales its comparison
            qb = [s for s in P.leaves if s[0] == 'MDPA.query.bias'][0]
            assert (np.abs(gl[:, b:e]).max(axis=1) < 1e-12 * np.abs(gl[:, qb[1]:qb[2]]).max(axis=1)).all(), tag
            continue
        assert share[:, j].min() >= LC.MIN_SHARE, (tag, n, share[:, j])
        assert blind[:, j].max() <= 1e-3, (tag, n, blind[:, j])


@pytest.mark.parametrize('kind,V,T,C,H,D,K,proj,bias,N,E', ATTN)
def test_sharp_attention_problems_are_seen_leaf_by_leaf(kind, V, T, C, H, D, K, proj, bias, N, E):
    P = LC.attn_problem(kind, V, T, C, H, D, K, proj, bias, N, E)
    _, g = P.ref()
    _visible(P, g, P.lik(), (kind, V, T, C, H, D))
    for e, st in enumerate(P.stats()):
        assert st['median_top'] >= 0.2, (e, st)                # attention is sharp ...
        assert st['min_rel'] <= 1e-6, (e, st)                  # the max-subtraction matters
        assert st['max_logit'] < 80.0, (e, st)                 # ... and exp(logit) is finite in fp32 even without the max-subtraction
    lp32, g32 = P.ref(np.float32)
    assert g32.dtype == np.float32 and np.isfinite(g32).all() and np.isfinite(lp32).all()


@pytest.mark.parametrize('kind,V,T,C,H,D,K,proj,bias,N,E,seed', ATTN_EXTRA)
def test_split_and_step_problems_are_seen_leaf_by_leaf(kind, V, T, C, H, D, K, proj, bias, N, E, seed):
    P = LC.attn_problem(kind, V, T, C, H, D, K, proj, bias, N, E, seed=seed)
    _, g = P.ref()
    _visible(P, g, P.lik(), (kind, N))
    if N == 600:
        rows = slice(100, 177)
        _visible(P, P.ref(rows=rows)[1], P.lik(rows), (kind, 'window'))
    assert all(st['median_top'] >= 0.2 for st in P.stats())


def test_old_attention_problems_are_prior_dominated():
    """The finding: at prior_scale 0.2 the whole-vector tolerance exceeds the whole likelihood gradient of the query and key
    kernels, and attention is uniform to within a few per cent."""
    for kind, case in (('attn', LC.attn_cases()[0]), ('pre', LC.attn_pre_cases()[0])):
        P = LC.attn_problem(kind, *case, sharp=False)
        _, g = P.ref()
        blind = dict(zip([n for n, _, _ in P.leaves], L.visibility(P.lik(), g, P.leaves, 2e-5, per_leaf=False)[0]))
        assert blind['MDPA.query.kernel'] > 1.0 and blind['MDPA.key.kernel'] > 1.0, blind
        assert P.stats()[0]['median_top'] < 0.06


@pytest.mark.parametrize('F,hs,act,task,N,E,seed', LC.deep_fcn_cases())
def test_deep_fcn_problems_are_seen_leaf_by_leaf(F, hs, act, task, N, E, seed):
    ospec, prob, lp, g, gl, chosen = LC.deep_fcn_problem(F, hs, act, task, N, E, seed)
    leaves = L.fcn_leaves(ospec)
    assert ospec.prior_scale == 1.0 and ospec.hidden_structure == hs and prob['theta0'].shape[0] == E
    assert L.likelihood_share(gl, g, leaves).min() >= LC.MIN_SHARE, chosen
    assert L.visibility(gl, g, leaves, L.LEAF_TOL).max() <= 1e-3, chosen


# ---- mutants ------------------------------------------------------------------------------------------------------------------

QK = ('MDPA.query.kernel', 'MDPA.key.kernel')
# Does the whole-vector criterion (2e-5 of the chain's largest entry) accept the wrong query / key kernel gradient on the old
# problem of the reference-shaped case?  Measured from the restatement (error / tolerance in brackets): the pretrained model
# accepts all three; the AttentionClassifier accepts the zeroed kernels (0.8) and misses the other two by 1.2x and 1.7x only.
OLD_ACCEPTS = {('attn', 'zero_qk_kernels'): True, ('attn', 'dq_unscaled'): False, ('attn', 'ds_unmasked'): False,
               ('pre', 'zero_qk_kernels'): True, ('pre', 'dq_unscaled'): True, ('pre', 'ds_unmasked'): True}


def _qk_only(P, g, g_mut):
    """The wrong dq / ds reaching the query and key kernels' weight gradient only (the leaves the audit found unseen)."""
    out = g.copy()
    for n, b, e in P.leaves:
        if n in QK:
            out[:, b:e] = g_mut[:, b:e]
    return out


@pytest.mark.parametrize('kind', ['attn', 'pre'])
@pytest.mark.parametrize('mutant', A.MUTANTS)
def test_attention_mutants(kind, mutant):
    """Query and key kernel gradients zeroed, dq without 1/sqrt(hd), ds without the mask, on the reference's shape.  Old problem:
    the whole-vector criterion does what OLD_ACCEPTS records (the wrong gradient in every leaf it reaches -- the embedding table,
    the query bias -- is caught by it: those leaves were seen).  New problem: assert_leaves rejects every form, by orders of
    magnitude."""
    case = (LC.attn_cases() if kind == 'attn' else LC.attn_pre_cases())[0]
    old = LC.attn_problem(kind, *case, sharp=False)
    _, g = old.ref()
    g_mut = _qk_only(old, g, old.ref(mutant=mutant)[1])
    assert np.abs(g_mut - g).max() > 0
    assert L.whole_vector_accepts(g_mut, g) == OLD_ACCEPTS[kind, mutant]
    assert np.abs(g_mut - g).max() < 2 * 2e-5 * np.abs(g).max()          # never far from unseen
    new = LC.attn_problem(kind, *case)
    _, g = new.ref()
    full = new.ref(mutant=mutant)[1]
    bound = new.bound(g)
    for wrong in (_qk_only(new, g, full), full):
        with pytest.raises(AssertionError, match='MDPA.(query|key)'):
            L.assert_leaves(wrong, g, new.leaves, bound, new.scale_of, tag=mutant)
        err = L.leaf_errors(wrong, g, new.leaves, new.scale_of)
        assert (err / bound).max() > 1e3
    L.assert_leaves(new.ref(np.float32)[1], g, new.leaves, bound, new.scale_of)      # the bound admits the float32 restatement


def test_deep_fcn_mutant():
    """Layer 0's likelihood gradient zeroed in (6, (12,) * 10 + (4,)): accepted by the whole-vector criterion on the old problem
    (sigmoid, theta_scale 0.1: the gradient has vanished by layer 0), rejected per leaf on the new one."""
    from oracle import mclmc_oracle as M
    F, hs, act, task, N, E = LC.DEEP_FCN[0]
    ospec = M.ModelSpec(F, hs, activation=act, task=task)
    prob = M.synthetic_problem(ospec, N, E, seed=LC.SEED)
    th = prob['theta0'].astype(np.float64)
    _, g = M.logpost_and_grad(ospec, th, prob['X'], prob['y'])

    def zero_layer0(ospec, g, th):
        out, gp = g.copy(), M.log_prior(ospec, th)[1]
        for n, b, e in L.fcn_leaves(ospec):
            if n.startswith('layer0.'):
                out[:, b:e] = gp[:, b:e]
        return out

    g_mut = zero_layer0(ospec, g, th)
    assert np.abs(g_mut - g).max() > 0 and L.whole_vector_accepts(g_mut, g)
    ospec, prob, _, g, _, _ = LC.deep_fcn_problem(F, hs, act, task, N, E, LC.SEED)
    with pytest.raises(AssertionError, match='layer0'):
        L.assert_leaves(zero_layer0(ospec, g, prob['theta0'].astype(np.float64)), g, L.fcn_leaves(ospec), tag='layer 0 zeroed')


# ---- the helper itself --------------------------------------------------------------------------------------------------------

def test_leafcheck_reports_leaf_chain_and_index():
    leaves = [('a', 0, 3), ('b', 3, 5)]
    g_ref = np.array([[100.0, 1.0, 2.0, 1e-3, 2e-3], [50.0, 1.0, 2.0, 1e-3, 2e-3]])
    g = g_ref.copy()
    g[1, 4] += 1e-6                                   # 5e-4 of leaf b, 2e-8 of the vector
    assert L.whole_vector_accepts(g, g_ref)
    err = L.leaf_errors(g, g_ref, leaves)
    assert err.shape == (2, 2) and err[0].max() == 0 and err[1, 0] == 0 and abs(err[1, 1] - 5e-4) < 1e-9
    with pytest.raises(AssertionError, match=r"leaf 'b' chain 1 index 1 \(flat 4\)"):
        L.assert_leaves(g, g_ref, leaves)
    L.assert_leaves(g, g_ref, leaves, bound=np.array([[5e-5, 5e-5], [5e-5, 1e-3]]))
    # a leaf that is zero analytically takes another leaf's scale
    assert abs(L.leaf_errors(g, g_ref, leaves, {'b': 'a'})[1, 1] - 1e-6 / 50.0) < 1e-15
    # blind: tolerance over the likelihood's largest entry, per leaf and for the whole vector
    lik = np.array([[1.0, 0, 0, 1e-3, 0], [1.0, 0, 0, 1e-6, 0]])
    assert np.allclose(L.visibility(lik, g_ref, leaves, 2e-5, per_leaf=False), [[2e-3, 2.0], [1e-3, 1e3]])
    assert np.allclose(L.visibility(lik, g_ref, leaves, 5e-5), [[5e-3, 1e-4], [2.5e-3, 0.1]])
    with pytest.raises(AssertionError, match='non-finite'):
        L.assert_leaves(np.full_like(g_ref, np.nan), g_ref, leaves)


def test_float32_restatement_has_no_float64_intermediates():
    """`dtype=float32` runs every product, the softmax and the sums in float32 (loglik_and_grad asserts the dtypes of the
    probabilities, the logits and the gradient); its distance to fp64 is fp32-rounding-sized on every leaf."""
    for kind in ('attn', 'pre'):
        P = LC.attn_problem(kind, *LC.SPLIT_SHAPES[kind], 40, 2)
        lp, g = P.ref()
        lp32, g32 = P.ref(np.float32)
        assert lp32.dtype == np.float32 and g32.dtype == np.float32
        err = L.leaf_errors(g32, g, P.leaves, P.scale_of)
        assert 0 < err.max() < 1e-4, err.max(axis=0)

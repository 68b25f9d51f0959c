"""The three attention gradient kernels over every cell of their launch schedule (-m gpu): k_grad_attn, k_grad_attn_pre and
k_grad_attn_wide on the cases of tests/attn_schedule.py.  tests/test_attn_schedule_host.py proves on the CPU that the table reaches
every cell, that every leaf's gradient is at least half the likelihood's and that a schedule that is wrong in one of the listed ways
misses the per-leaf bound below by more than 10x.

Every gradient against tests/attn_ref.py / tests/attn_pre_ref.py in fp64: logp 2e-5 relative, every leaf of every chain 5e-5 of
its own largest entry (leafcheck.LEAF_TOL), or 8x (F32_MARGIN) the float32 restatement's own error where that is larger; a leaf
that takes the 8x branch is printed; MDPA.key.bias on the query bias's scale (tests/leaf_cases.py).  Nothing in a bound comes from
a kernel.  Every particle beyond the first two repeats particle 0's or 1's parameters and must repeat its result bit for bit in
every leaf that is not summed by atomics; the token table is held to the bound instead.

Each test prints what it measured before it asserts (`pytest -s`, lines ATTNSCHED), and the module prints the worst leaf per family
and kernel at its end (ATTNWORST); profiles/r11/01_attn_schedule.md keeps the figures of an MI355X."""
from functools import lru_cache

import numpy as np
import pytest

from tests import attn_pre_ref as RP
from tests import attn_ref as RA
from tests import attn_schedule as S
from tests import leafcheck as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
LP_TOL = 2e-5            # relative: DESIGN section 1, tests/test_gpu_attn*.py
EVAL_TOL = 1e-4          # of max(1, max |ref|): tests/test_gpu_attn*.py::test_pointwise_loglik_matches_restatement, tests/test_gpu_predict.py
TABLE = 'TokenEmbedding_0.Embedding.embedding'
EVAL_KERNEL = {'pointwise_loglik': 'k_fwd', 'predict': 'k_out'}
_WORST = {}              # (family, kernel) -> [leaf error / bound, leaf error, float32 restatement's, case, leaf]


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    for (f, k), (ratio, err, err32, name, leaf) in sorted(_WORST.items()):
        print(f'\nATTNWORST {f:<5s} {k:<22s} worst leaf {err:.2e} ({ratio:.3f} of its bound; float32 restatement {err32:.2e}) in {leaf} of {name}')


def _engine(case, P):
    from mile_amd.engine import Engine
    p = P.prob
    kw = {'tables': (p['emb'], p['pos'])} if case.family == 'pre' else {}
    eng = Engine(P.spec, torch.from_numpy(np.array(p['X'])), torch.from_numpy(np.array(p['y'])), device=DEV, **kw)
    assert eng.grad_kernel == S.GRAD_KERNEL[case.family]
    return eng


def _launch(eng, case, P):
    """One gradient of the case on the engine, after the launch it will take is what the plan says."""
    assert S.supported(case), case.name                            # nothing is launched that the envelope does not take
    eng.set_row_window(*(case.window or (0, 0)))
    theta = torch.from_numpy(P.theta(case.E))
    eng.reserve(case.E)
    info, plan = eng.grad_launch_info(case.E), S.plan(case)
    assert info['kernel'] == S.KERNEL[case.family] and info['grid'] == (plan['S'], case.E) and info['lds_bytes'] == plan['lds'], (case.name, info, plan['S'], plan['lds'])
    lp, g = eng.logpost_grad(theta)
    torch.cuda.synchronize()
    return lp.cpu(), g.cpu()


def _kernel_name(case):
    p = S.plan(case)
    return f"{S.KERNEL[case.family]}<{p['NHT']}" + (f", {str(p['WL']).lower()}>" if case.family == 'attn' else '>')


def _where(case):
    p = S.plan(case)
    return f"{_kernel_name(case)} S {p['S']} rows {'/'.join(str(c) for c in sorted(set(p['counts']), reverse=True))} lds {p['lds']}"


def _check(case, P, lp, g, where=''):
    """logp and every leaf of the first min(E, 2) particles against the case's reference."""
    n = min(case.E, 2)
    lp_ref, g_ref, g32 = (a[:n] for a in S.reference_of(case))
    bound = L.leaf_bounds(P.leaves, n, g32, g_ref, P.scale_of)
    lp, g = np.asarray(lp, np.float64)[:n], np.asarray(g, np.float64)[:n]
    e_lp = np.abs(lp - lp_ref).max() / max(1.0, np.abs(lp_ref).max())
    err, err32 = L.leaf_errors(g, g_ref, P.leaves, P.scale_of), L.leaf_errors(g32, g_ref, P.leaves, P.scale_of)
    c, j = np.unravel_index(int((err / bound).argmax()), err.shape)
    wider = sorted({P.leaves[jj][0] for jj in np.nonzero((bound > L.LEAF_TOL).any(axis=0))[0]})
    print(f'\nATTNSCHED {case.name} [{_where(case)}{where}]: logp {e_lp:.2e}  worst leaf {err[c, j]:.2e} in {P.leaves[j][0]} '
          f'(float32 restatement {err32.max():.2e}, bound {bound.min():.2e}..{bound.max():.2e})' + (f'  8x branch: {wider}' if wider else ''))
    key = (case.family, _kernel_name(case))
    if key not in _WORST or err[c, j] / bound[c, j] > _WORST[key][0]:
        _WORST[key] = [float(err[c, j] / bound[c, j]), float(err[c, j]), float(err32[c, j]), case.name, P.leaves[j][0]]
    assert np.isfinite(lp).all() and np.isfinite(g).all(), case.name
    assert e_lp < LP_TOL, (case.name, e_lp)
    L.assert_leaves(g, g_ref, P.leaves, bound, P.scale_of, tag=(case.name, _where(case) + where))


def _repeats(case, P, lp, g):
    """Particles beyond the first two that do not repeat their chain bit for bit, the token table left out (atomics)."""
    keep = torch.ones(g.shape[1], dtype=torch.bool)
    for n, b, e in P.leaves:
        if n == TABLE:
            keep[b:e] = False
    return [e for e in range(2, lp.shape[0]) if not (torch.equal(lp[e], lp[e % 2]) and torch.equal(g[e][keep], g[e % 2][keep]))]


@lru_cache(maxsize=None)
def _run(case):
    P = S.problem(case)
    return _launch(_engine(case, P), case, P)


# ---- every case ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', S.SINGLE_CASES, ids=lambda c: c.name)
def test_every_cell_of_the_schedule(case):
    P = S.problem(case)
    lp, g = _run(case)
    _check(case, P, lp, g)
    assert not _repeats(case, P, lp, g), (case.name, 'particles that differ from their chain')
    for k in range(1, min(3, (case.E + 1) // 2)):                    # the table of a repeated particle: at the bound, like its chain's
        idx = [2 * k, 2 * k + 1 if 2 * k + 1 < case.E else 1]
        _check(case._replace(E=2), P, lp[idx], g[idx], where=f', particles {idx}')


# ---- stale state: four gradients on one engine --------------------------------------------------------------------------------

@pytest.mark.parametrize('family', S.FAMILIES)
def test_windows_on_one_engine_leave_nothing_behind(family):
    """The full set, a window, a smaller window with fewer distinct tokens, the full set again, on one engine: each against fp64
    on its rows; the last against the first bit for bit off the token table and at the bound on it."""
    cases = [S.BY_NAME[n] for n in S.SEQUENCES[family]]
    P0 = S.problem(cases[0])
    x = P0.prob['x']
    assert len(np.unique(x[slice(*np.cumsum(cases[2].window))])) < len(np.unique(x[slice(*np.cumsum(cases[1].window))]))
    eng = _engine(cases[0], P0)
    got = []
    for case in cases:
        P = S.problem(case)
        lp, g = _launch(eng, case, P)
        _check(case, P, lp, g, where=f", rows {S.rows_of(case)[0]}+{S.rows_of(case)[1]}")
        got.append((lp, g))
    eng.set_row_window(0, 0)
    (lp0, g0), (lp3, g3) = got[0], got[3]
    keep = torch.ones(g0.shape[1], dtype=torch.bool)
    for n, b, e in P0.leaves:
        if n == TABLE:
            keep[b:e] = False
    print(f'ATTNSCHED {family} full set again against the first: table {float((g3 - g0).abs().max()):.2e}')
    assert torch.equal(lp3, lp0) and torch.equal(g3[:, keep], g0[:, keep]), family


# ---- on chip against the wide kernel ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', S.ALSO_WIDE)
def test_on_chip_cases_on_the_wide_kernel(name):
    """A case inside k_grad_attn's envelope on k_grad_attn_wide as well: each against fp64 at the full bound, not against the
    other; what they differ by is printed."""
    case = S.BY_NAME[name]
    wide = case._replace(name=name + '-on-wide', family='wide')
    P = S.problem(wide)
    lp, g = _run(wide)
    _check(wide, P, lp, g)
    assert not _repeats(wide, P, lp, g), wide.name
    lp1, g1 = _run(case)
    print(f'ATTNSCHED {name}: wide against on chip {float((g - g1).abs().max() / g1.abs().max()):.2e} of the largest entry')


# ---- evaluation -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', S.EVAL_CASES, ids=lambda c: c.name)
def test_evaluation_kernels(case):
    """pointwise_loglik (k_fwd_*) and predict (k_out_*) of every reachable (family, NHT, WL) at 5 samples on 37 rows (two row
    blocks of 19 and 18): 1e-4 of max(1, max |ref|)."""
    n_s, n_rows = 5, 37
    assert S.attn_ranges(S.N_CU, n_s, n_rows) == 2 and n_rows % 2
    P = S.problem(case)
    R = RP if case.family == 'pre' else RA
    params = R.synthetic_problem(P.spec, 2, n_s, seed=6)
    test = RA.synthetic_problem(P.spec, n_rows, 1, seed=7)
    th64 = params['theta0'].astype(np.float64)
    if case.family == 'pre':
        fw = [RP.forward(P.spec, RP.params(P.spec, t, P.prob['emb'], P.prob['pos']), test['x']) for t in th64]
        ll_ref = np.stack([RP.pointwise_loglik(P.spec, t, P.prob['emb'], P.prob['pos'], test['x'], test['y']) for t in th64])
    else:
        fw = [RA._forward(P.spec, RA.unpack(P.spec, t), test['x']) for t in th64]
        ll_ref = np.stack([RA.pointwise_loglik(P.spec, t, test['x'], test['y']) for t in th64])
    out_ref = np.stack([f['logits'] for f in fw])
    eng = _engine(case, P)
    theta = torch.from_numpy(params['theta0'])
    pw = eng.pointwise_loglik(theta, torch.from_numpy(test['X']), torch.from_numpy(test['y']))
    out = eng.predict(theta, torch.from_numpy(test['X']))
    torch.cuda.synchronize()
    assert tuple(pw.shape) == (n_s, n_rows) and tuple(out.shape) == (n_s, n_rows, case.K)
    for tag, got, ref in (('pointwise_loglik', pw, ll_ref), ('predict', out, out_ref)):
        got = got.cpu().numpy().astype(np.float64)
        tol = EVAL_TOL * max(1.0, np.abs(ref).max())
        kernel = _kernel_name(case).replace('k_grad', EVAL_KERNEL[tag])
        print(f'\nATTNSCHED eval {case.name} [{kernel}] {tag}: {np.abs(got - ref).max():.2e} (bound {tol:.2e})')
        assert np.isfinite(got).all() and np.abs(got - ref).max() < tol, (case.name, tag)


# ---- what the library refuses -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('family,T,C,H,D,proj,K', S.REFUSED)
def test_the_first_geometry_past_each_bound_is_refused(family, T, C, H, D, proj, K):
    """One 16-step of T beyond the largest supported geometry: the library's error with its string and no handle, the spec's
    NotImplementedError; the step before it is made by both."""
    assert S.UNREACHABLE[('bound', family, 'refused one step of T on')].endswith(S.REFUSAL[family])
    rc, msg, handle = S.library_refuses(family, 60, T, C, H, D, K, proj)
    assert rc != 0 and msg == S.REFUSAL[family] and not handle, (rc, msg)
    assert S.library_refuses(family, 60, T - 16, C, H, D, K, proj)[0] == 0
    with pytest.raises(NotImplementedError, match='LDS'):
        S.spec_of(S._c('refused', family, 60, T, C, H, D, K=K, proj=proj))
    S.spec_of(S._c('ok', family, 60, T - 16, C, H, D, K=K, proj=proj))


def test_two_heads_on_a_wave_with_dk_in_scratch_is_refused_on_chip():
    """The cell ('two heads on one wave', 'attn', 'dK in scratch'): H >= 5 and hd >= 17 is D >= 85, which the on-chip envelope
    refuses; the factory gives the shape to the wide kernel, where it is a case."""
    from mile_amd.spec import AttentionSpec, WideAttentionSpec, attention_spec
    (family, T, C, H, D, proj, K), = S.REFUSED_BY_LIMIT
    assert S.LIMIT_REFUSAL['attn'] in S.UNREACHABLE[('two heads on one wave', 'attn', S.DK[1])]
    rc, msg, handle = S.library_refuses(family, 25, T, C, H, D, K, proj)
    assert rc != 0 and msg == S.LIMIT_REFUSAL['attn'] and not handle, (rc, msg)
    with pytest.raises(NotImplementedError, match='qkv_dim'):
        AttentionSpec(25, T, C, H, D, projection_dim=proj)
    assert type(attention_spec(vocab_size=25, context_len=T, emb_size=C, n_heads=H, qkv_dim=D, projection_dim=proj)) is WideAttentionSpec
    assert any((c.T, c.C, c.H, c.D) == (T, C, H, D) for c in S.CASES if c.family == 'wide')

"""Alignment of FCN draws to a reference draw by hidden-unit assignment, host side (-m "not gpu"): the NumPy restatement
tests/align_ref.py against scipy's assignment, the dense form against the restatement, idempotence, recovery of permuted and
sign-flipped noisy copies bit for bit, the permutation case in parameter space, a NaN draw, the C ABI surface with every refusal
(called on a machine without a GPU: nothing touches a device before the checks), and the evaluate.py flags."""
import ctypes as C
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests import align_ref as A
from tests import canon_ref as CR
from tests import diag_ref as R
from tests import fdiag_ref as F

ROOT = Path(__file__).resolve().parents[1]
CASE_SIGNS = [(n, s) for n in A.CASES for s in A.case_signs(n)]


def _t(a):
    return torch.from_numpy(np.array(a))                  # a copy: the shared cases are read-only


def _identity(spec, M):
    return np.broadcast_to(np.concatenate([np.arange(w) for w in spec.hidden_structure[:-1]] + [np.arange(0)]),
                           (M, sum(spec.hidden_structure[:-1])))


@pytest.mark.parametrize('name,sign', CASE_SIGNS)
def test_the_restatement_reaches_scipys_objective(name, sign):
    """Per (draw, layer) the restated solver's objective equals scipy.optimize.linear_sum_assignment's on the same gain matrix to
    rtol 1e-12 (ties make the permutation itself legal to differ, so only the objective is demanded)."""
    spec = A.case_spec(name)
    centre, _, moved = A.case_data(name)
    gains = []
    out, perm, sgn, score, dropped = A.align(spec, moved, centre, sign, gains=gains)
    for v, r in zip((out, perm, sgn, score, dropped), A.case_aligned(name, sign)):
        assert np.array_equal(v, r)
    nh = len(spec.hidden_structure) - 1
    assert len(gains) == moved.shape[0] * nh and not dropped.any() and score.shape == (moved.shape[0], nh)
    worst = 0.0
    for m, l, G in gains:
        r, c = linear_sum_assignment(G, maximize=True)
        best = G[r, c].sum()
        worst = max(worst, abs(score[m, l] - best) / abs(best))
        assert abs(score[m, l] - best) <= 1e-12 * abs(best), (name, m, l, score[m, l], best)
    print(f'ALIGN {name} sign={sign}: {len(gains)} problems, worst relative objective gap {worst:.1e}')
    # every output float is an input float moved, possibly negated; each span of perm is a permutation of its layer's units
    assert np.array_equal(np.sort(np.abs(out), axis=1), np.sort(np.abs(moved), axis=1))
    if not sign:
        assert (sgn == 1).all() and np.array_equal(np.sort(out, axis=1), np.sort(moved, axis=1))
    o = 0
    for w in spec.hidden_structure[:-1]:
        assert np.array_equal(np.sort(perm[:, o:o + w], axis=1), np.broadcast_to(np.arange(w), (moved.shape[0], w)))
        o += w
    if nh == 0:
        assert np.array_equal(out, moved) and perm.shape == (moved.shape[0], 0)


def test_the_solver_on_ties_and_a_hand_made_problem():
    """Equal gains everywhere: the fixed operation order gives the identity.  A 3 x 3 problem with a known optimum."""
    assert A.hungarian(np.zeros((5, 5))).tolist() == [0, 1, 2, 3, 4]
    c = np.array([[4.0, 1.0, 3.0], [2.0, 0.0, 5.0], [3.0, 2.0, 2.0]])
    p = A.hungarian(c)
    assert p.tolist() == [1, 0, 2] and c[np.arange(3), p].sum() == 5.0


@pytest.mark.parametrize('name,sign', CASE_SIGNS)
def test_dense_is_in_the_orbit_and_reaches_the_objective(name, sign):
    """align_dense: the output is a member of the draw's orbit (per layer leaf the sorted multiset of |values| is the draw's), and
    each layer's objective is the restatement's.  Its similarities come from one fp64 matrix product, whose terms add in another
    order: of at most 128 + 3 products of magnitude O(1) each, so a score -- a sum of at most 128 matched similarities, which on
    these cases are positive and of the size of the sum of their terms' magnitudes -- differs by at most a few thousand roundings
    of 2^-53 relative: rtol 1e-11."""
    from mile_amd import metrics as M
    spec = A.case_spec(name)
    centre, _, moved = A.case_data(name)
    out, perm, sgn, score, dropped = (t.numpy() for t in M.align_dense(spec, _t(moved), _t(centre), sign))
    ref = A.case_aligned(name, sign)
    assert out.dtype == np.float32 and perm.dtype == np.int32 and sgn.dtype == np.int8 and score.dtype == np.float64 and dropped.dtype == np.int32
    assert out.shape == moved.shape and perm.shape == ref[1].shape and score.shape == ref[3].shape and not dropped.any()
    for _, off, shape in spec.leaves():
        n = int(np.prod(shape))
        assert np.array_equal(np.sort(np.abs(out[:, off:off + n]), axis=1), np.sort(np.abs(moved[:, off:off + n]), axis=1))
    np.testing.assert_allclose(score, ref[3], rtol=1e-11, atol=0)


@pytest.mark.parametrize('name,sign', CASE_SIGNS)
def test_idempotent(name, sign):
    """Aligning the aligned draws to the same reference moves nothing."""
    spec = A.case_spec(name)
    centre = A.case_data(name)[0]
    once = A.case_aligned(name, sign)
    out, perm, sgn, score, dropped = A.align(spec, once[0], centre, sign)
    assert np.array_equal(out, once[0]) and np.array_equal(perm, _identity(spec, out.shape[0])) and (sgn == 1).all()
    assert not dropped.any()


@pytest.mark.parametrize('name', A.RECOVERED)
def test_recovery_of_permuted_noisy_copies(name):
    """Noisy copies (scale 0.05) of a centre, permuted (for tanh sign-flipped) per draw: alignment to the centre returns the
    unpermuted draws bit for bit -- what ordering by a key cannot do."""
    from mile_amd import metrics as M
    spec = A.case_spec(name)
    centre, orig, moved = A.case_data(name)
    sign = spec.activation == 'tanh'
    assert not np.array_equal(moved, orig)
    assert np.array_equal(A.case_aligned(name, sign)[0], orig)
    assert np.array_equal(M.align_dense(spec, _t(moved), _t(centre), sign)[0].numpy(), orig)
    res = M.align(spec, _t(moved), _t(centre), sign=sign)
    assert M.LAST_ALIGN_PATH == 'scipy' and np.array_equal(res['theta'].numpy(), orig)
    key_sorted = CR.canonicalize(spec, moved, 'bias', sign)[0]
    assert not np.array_equal(key_sorted, orig)


def test_noise_large_enough_not_to_recover():
    """w16 at noise 0.3: 38 of the 40 draws come back, the other two have a better matching than their own."""
    spec = A.case_spec('w16')
    centre, orig, moved = A.case_data('w16')
    out, _, _, score, _ = A.case_aligned('w16', False)
    back = np.array([np.array_equal(out[m], orig[m]) for m in range(40)])
    assert back.sum() == 38
    own = A.align(spec, orig, centre)[3]                                       # (the scores do not depend on the orbit member)
    assert np.array_equal(own, score)


def test_permutation_case_in_parameter_space():
    """Three chains around one mode of [3 -> 8 -> 8 -> 2] tanh, chains 1 and 2 permuted: fp64 parameter-space max rhat 2.4091 raw,
    1.0370 aligned to draw 0 (two rounds), none of the 122 parameters above 1.1, and no chain ever changes its matching."""
    from mile_amd import metrics as M
    spec, theta = CR.permutation_spec(), CR.permutation_draws()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        raw = R.chain_diagnostics(theta, 2)['rhat']
        assert raw.max() > 2.0
        for sign in (False, True):
            out, perm, sgn, score, dropped, ref = A.permutation_aligned(sign)
            rhat = R.chain_diagnostics(out, 2)['rhat']
            sw = CR.switches(perm, F.PERM_WIDTHS[:-1])
            print(f'ALIGN permutation fp64 sign={sign}: parameter rhat max raw {raw.max():.4f} aligned {rhat.max():.4f}  '
                  f'above 1.1: {int((rhat > 1.1).sum())} of {rhat.size}  switches {sw.tolist()}')
            assert rhat.max() < 1.1 and (sw == 0).all() and not dropped.any()
            got = M.aligned_diagnostics(spec, _t(theta), 2, reference='first', rounds=2, sign=sign)
            assert M.LAST_ALIGN_PATH == 'scipy' and M.LAST_DIAG_PATH == 'torch'
            assert float(got['rhat'].max()) < 1.1 and (got['switches'] == 0).all() and got['dropped'] == 0
            assert got['switches'].shape == (3, 2) and got['scores'].shape == (3, 64, 2) and got['score_mean'].shape == (2,)
            assert np.array_equal(got['theta'].numpy(), out) and np.array_equal(got['reference'].numpy(), ref)
            np.testing.assert_allclose(got['rhat'].numpy(), rhat, rtol=1e-9)
        # ordering by a key switches labels on this case; the assignment does not
        assert CR.switches(CR.permutation_canonical('bias', False)[1], F.PERM_WIDTHS[:-1]).sum() > 0


def test_a_nan_draw_is_dropped_and_copied():
    spec = A.case_spec('sep')
    centre, _, moved = A.case_data('sep')
    from mile_amd import metrics as M
    theta = np.array(moved[:5])
    off = {n.split('.', 1)[1]: o for n, o, _ in spec.leaves()}
    theta[1, off['layer1.kernel'] + 3] = np.nan                # layer 0 solves, layer 1 does not
    theta[3, off['layer0.bias'] + 2] = np.inf
    for sign in (False, True):
        out, perm, sgn, score, dropped = A.align(spec, theta, centre, sign)
        assert dropped.tolist() == [0, 1, 0, 1, 0]
        clean = A.case_aligned('sep', sign)
        for m in (0, 2, 4):                                    # a dropped draw touches no other
            assert all(np.array_equal(v[m], r[m]) for v, r in zip((out, perm, sgn, score), clean))
        for m in (1, 3):
            assert np.array_equal(out[m], theta[m], equal_nan=True) and np.array_equal(perm[m], _identity(spec, 1)[0])
            assert (sgn[m] == 1).all() and np.isnan(score[m]).all()
        d = [t.numpy() for t in M.align_dense(spec, _t(theta), _t(centre), sign)]
        assert np.array_equal(d[0], out, equal_nan=True) and np.array_equal(d[1], perm) and np.array_equal(d[2], sgn)
        assert np.array_equal(d[4], dropped) and np.isnan(d[3][[1, 3]]).all()
    res = M.align(spec, _t(theta), 'first', rounds=2)          # the mean of round 1 leaves the dropped draws out
    assert res['dropped'].tolist() == [0, 1, 0, 1, 0] and bool(torch.isfinite(res['reference']).all())


def test_python_refusals():
    from mile_amd import ModelSpec
    from mile_amd import metrics as M
    from mile_amd.spec import LeNettiSpec
    relu = ModelSpec(3, (4, 2), activation='relu', task='regr')
    th = torch.zeros((2, relu.n_params))
    with pytest.raises(ValueError, match='tanh only'):
        M.align(relu, th, sign=True)
    with pytest.raises(ValueError, match='reference'):
        M.align(relu, th, reference='mean')
    with pytest.raises(ValueError, match='reference must hold'):
        M.align(relu, th, reference=torch.zeros(3))
    with pytest.raises(ValueError, match='rounds'):
        M.align(relu, th, rounds=0)
    with pytest.raises(ValueError, match='theta must be'):
        M.align(relu, th[:, :-1])
    with pytest.raises(ValueError, match='FCN only'):
        M.align(LeNettiSpec.__new__(LeNettiSpec), th)
    with pytest.raises(ValueError, match=r'\[C, S, d\]'):
        M.aligned_diagnostics(relu, th)


def _cspec(fin=3, hs=(8, 8, 2), act='tanh', task='regr'):
    from mile_amd import ModelSpec, _lib
    return _lib.fcn_spec_c(ModelSpec(fin, hs, activation=act, task=task))


def test_c_abi_surface_and_refusals():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    assert lib.mile_abi_version() == 10
    p, i32, i64, u32, sp = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.POINTER(_lib.ModelSpecC)
    assert _lib.SIGNATURES['mile_align_fcn'] == (i32, [sp, p, i64, p, u32, p, p, p, p, p, p, i64, p])
    assert _lib.SIGNATURES['mile_align_fcn_workspace'] == (i64, [sp, i64, u32])
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_align_fcn(const mile_model_spec *spec, const float *theta, int64_t M, const float *reference, uint32_t how, '
            'float *out, int32_t *perm, int8_t *sign, double *score, int32_t *dropped, void *workspace, int64_t workspace_bytes, '
            'void *stream);') in header
    assert 'int64_t mile_align_fcn_workspace(const mile_model_spec *spec, int64_t M, uint32_t how);' in header
    assert '#define MILE_ALIGN_SIGN 1u' in header and '#define MILE_ALIGN_WIDTH_MAX 128' in header
    assert _lib.ALIGN_SIGN == 1 and _lib.ALIGN_WIDTH_MAX == 128

    good = _cspec()
    d = 3 * 8 + 8 + 8 * 8 + 8 + 8 * 2 + 2
    # host memory stands in for the device pointers: every one of these calls is refused before anything reads them
    theta = (C.c_float * (4 * d))()
    out = (C.c_float * (4 * d))()
    ref = (C.c_float * d)()
    work = (C.c_uint32 * (4 * 16))()
    T, Out, Ref, Ws = C.cast(theta, p), C.cast(out, p), C.cast(ref, p), C.cast(work, p)

    def refused(rc, word, code=-1):
        msg = lib.mile_last_error()
        assert rc == code and b'mile_align_fcn: ' in msg and word in msg, (rc, msg)

    call = lambda spec=good, th=T, M=4, r=Ref, how=0, o=Out, ws=Ws, nws=4 * 16 * 4: lib.mile_align_fcn(
        C.byref(spec) if spec is not None else None, th, M, r, how, o, None, None, None, None, ws, nws, None)
    for kw in ({'spec': None}, {'th': None}, {'r': None}, {'o': None}):
        refused(call(**kw), b'null spec, theta, reference or out')
    refused(call(M=0), b'M out of range')
    lenet = _cspec()
    lenet.model = _lib.MODEL_IDS['lenet']
    refused(call(spec=lenet), b'only MILE_MODEL_FCN')
    nobias = _cspec()
    nobias.use_bias = 0
    refused(call(spec=nobias), b'use_bias must be 1')
    refused(call(how=2), b'unknown bits in `how`')
    refused(call(how=3), b'unknown bits in `how`')
    refused(call(spec=_cspec(act='relu'), how=1), b'tanh only')
    refused(call(spec=_cspec(act='sigmoid'), how=1), b'tanh only')
    wide = _cspec(hs=(130, 2))
    refused(call(spec=wide), b'hidden width above MILE_ALIGN_WIDTH_MAX')
    refused(call(spec=_cspec(hs=(8, 129, 2))), b'hidden width above MILE_ALIGN_WIDTH_MAX')
    refused(call(o=T), b'out overlaps theta')
    refused(call(o=C.c_void_p(T.value + 4 * (4 * d - 1))), b'out overlaps theta')
    refused(call(th=C.c_void_p(Out.value + 4 * d)), b'out overlaps theta')
    refused(call(r=Out), b'out overlaps reference')
    refused(call(r=C.c_void_p(Out.value + 4 * (4 * d - 1))), b'out overlaps reference')
    refused(call(o=C.c_void_p(Ref.value + 4 * (d - 1)), th=C.c_void_p(Ref.value + (1 << 40))), b'out overlaps reference')
    need = lib.mile_align_fcn_workspace(C.byref(good), 4, 1)
    assert need == 4 * 16 * 4
    refused(call(ws=None, nws=0), b'workspace too small', code=-2)
    refused(call(nws=need - 1), b'workspace too small', code=-2)
    refused(call(ws=None, nws=need), b'workspace too small', code=-2)

    ws = lambda s, M, how: lib.mile_align_fcn_workspace(C.byref(s) if s is not None else None, M, how)
    assert ws(good, 1000, 1) == 1000 * 16 * 4 and ws(_cspec(hs=(2,)), 7, 0) == 0 and ws(_cspec(hs=(128, 2)), 3, 1) == 3 * 128 * 4
    assert ws(_cspec(fin=4, hs=(3,) * 11 + (2,)), 5, 0) == 5 * 33 * 4
    assert ws(None, 4, 0) == -1 and ws(good, 0, 0) == -1 and ws(good, 4, 2) == -1 and ws(_cspec(act='relu'), 4, 1) == -1 and ws(wide, 4, 0) == -1
    assert b'mile_align_fcn_workspace: ' in lib.mile_last_error()
    assert ws(lenet, 4, 0) == -1 and ws(nobias, 4, 0) == -1
    zero = _cspec()
    zero.widths[1] = 0
    assert ws(zero, 4, 0) == -1 and b'layer width' in lib.mile_last_error()


def test_evaluate_flags_and_refusals(capsys):
    sys.path.insert(0, str(ROOT))
    import evaluate as EV
    ap = EV.build_parser()
    a = ap.parse_args(['-e', 'x'])
    assert a.aligned_diagnostics is None and a.align_reference == 'first' and a.align_rounds == 2 and a.align_sign is False   # opt-in
    a = ap.parse_args(['-e', 'x', '--aligned-diagnostics', '--align-reference', 'r.npy', '--align-rounds', '3', '--align-sign'])
    assert a.aligned_diagnostics == 2 and a.align_reference == 'r.npy' and a.align_rounds == 3 and a.align_sign is True
    assert ap.parse_args(['-e', 'x', '--aligned-diagnostics', '4']).aligned_diagnostics == 4
    with pytest.raises(SystemExit):
        ap.parse_args(['-e', 'x', '--align-rounds', 'two'])
    with pytest.raises(SystemExit):
        ap.parse_args(['--help'])
    text = capsys.readouterr().out
    for flag in ('--aligned-diagnostics', '--align-reference', '--align-rounds', '--align-sign'):
        assert flag in text
    assert 'aligned-diagnostics' in EV.__doc__
    assert EV.aligned_refusal('FCN', 'tanh', True) is None and EV.aligned_refusal('FCN', 'relu', False) is None
    assert 'FCN experiments only' in EV.aligned_refusal('LeNet', None, False)
    assert 'odd activation' in EV.aligned_refusal('FCN', 'relu', True)


@pytest.mark.parametrize('argv,word', [(['--aligned-diagnostics'], 'FCN experiments only'),
                                       (['--aligned-diagnostics', '--align-sign'], 'odd activation'),
                                       (['--aligned-diagnostics', '--align-rounds', '0'], 'at least 1'),
                                       (['--aligned-diagnostics', '--align-reference', 'missing.npy'], 'neither')])
def test_evaluate_refuses_before_any_work(tmp_path, monkeypatch, argv, word):
    """evaluate.py on a LeNetti experiment, with --align-sign on a relu FCN, with no round and with a reference file that is not
    there: SystemExit with the reason, before the model, the samples or a device are touched (the directory holds a config.yaml
    and nothing else)."""
    import yaml
    sys.path.insert(0, str(ROOT))
    import evaluate as EV
    src = 'mclmc_lenetti_mnist.yaml' if word.startswith('FCN') else 'smoke_synthetic.yaml'
    cfg = yaml.safe_load((ROOT / 'experiments' / src).read_text())
    if not word.startswith('FCN'):
        cfg['model']['activation'] = 'relu'
    (tmp_path / 'config.yaml').write_text(yaml.safe_dump(cfg))
    monkeypatch.setattr(sys, 'argv', ['evaluate.py', '-e', str(tmp_path)] + argv)
    with pytest.raises(SystemExit) as e:
        EV.main()
    assert word in str(e.value)

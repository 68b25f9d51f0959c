"""Canonical hidden-unit ordering of FCN draws, host side (-m "not gpu"): the torch form against the NumPy restatement
tests/canon_ref.py bit for bit, idempotence, invariance over the orbit, the function left alone (fp64 oracle), the permutation
case in parameter space, the C ABI surface with every refusal (called on a machine without a GPU: nothing touches a device
before the checks), and the evaluate.py flags."""
import ctypes as C
import sys
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import mclmc_oracle as O
from tests import canon_ref as CR
from tests import diag_ref as R
from tests import fdiag_ref as F

ROOT = Path(__file__).resolve().parents[1]
CASE_COMBOS = [(n, k, s) for n in CR.CASES for k, s in CR.case_combos(n)]


def _dense(spec, theta, key, sign):
    from mile_amd import metrics as M
    return tuple(t.numpy() for t in M.canonicalize_dense(spec, torch.from_numpy(np.array(theta)), key, sign))


def _same(got, ref, what):
    for g, r, name, dt in zip(got, ref, ('out', 'perm', 'sign'), (np.float32, np.int32, np.int8)):
        assert g.dtype == dt and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        assert np.array_equal(g, r, equal_nan=name == 'out'), (what, name)


@pytest.mark.parametrize('name,key,sign', CASE_COMBOS)
def test_dense_equals_the_restatement(name, key, sign):
    spec, theta = CR.case_spec(name), CR.case_draws(name)
    ref = CR.case_canonical(name, key, sign)
    _same(_dense(spec, theta, key, sign), ref, name)
    H = sum(spec.hidden_structure[:-1])
    assert ref[1].shape == (theta.shape[0], H) and ref[0].shape == theta.shape
    if H == 0:
        assert np.array_equal(ref[0], theta)
    # every output float is an input float moved, possibly negated
    assert np.array_equal(np.sort(np.abs(ref[0]), axis=1), np.sort(np.abs(theta), axis=1))
    if not sign:
        assert (ref[2] == 1).all() and np.array_equal(np.sort(ref[0], axis=1), np.sort(theta, axis=1))
    o = 0
    for w in spec.hidden_structure[:-1]:                    # each span of perm is a permutation of its layer's units
        assert np.array_equal(np.sort(ref[1][:, o:o + w], axis=1), np.broadcast_to(np.arange(w), (theta.shape[0], w)))
        o += w


def test_specials_ties_zeros_infinities_and_a_nan_draw():
    spec, theta = CR.specials()
    for key, sign in CR.COMBOS:
        ref = CR.canonicalize(spec, theta, key, sign)
        _same(_dense(spec, theta, key, sign), ref, (key, sign))
        clean = np.delete(theta, 2, axis=0)                 # the NaN draw touches no other draw
        for g, r in zip(CR.canonicalize(spec, clean, key, sign), ref):
            assert np.array_equal(g, np.delete(r, 2, axis=0))
    out, perm, sgn = CR.canonicalize(spec, theta, 'bias', False)
    p0, p1 = perm[:, :8], perm[:, 8:]
    assert list(p0[0]).index(2) + 1 == list(p0[0]).index(5)                    # identical units: index order
    z = [int(u) for u in p1[0] if u in (1, 3, 6)]
    assert z == [1, 3, 6]                                                      # -0.0 == +0.0 == -0.0: index order
    assert p0[1][0] == 1 and p0[1][-1] == 4 and p1[1][-1] == 7                 # -inf first, +inf last
    assert p0[2][-1] == 3 and list(p1[2][-2:]) == [0, 5]                       # NaN after every number, in index order
    out_s, perm_s, sgn_s = CR.canonicalize(spec, theta, 'bias', True)
    assert sgn_s[0][8 + list(perm_s[0, 8:]).index(1)] == 1 and sgn_s[2][list(perm_s[2, :8]).index(3)] == 1   # -0.0, NaN: not flipped
    assert (sgn_s == -1).any() and list(perm_s[1][6:8]) == [1, 4]              # |-inf| = +inf: last with +inf, in index order


@pytest.mark.parametrize('name,key,sign', CASE_COMBOS)
def test_idempotent(name, key, sign):
    spec = CR.case_spec(name)
    once = CR.case_canonical(name, key, sign)
    out, perm, sgn = _dense(spec, once[0], key, sign)
    if key == 'norm' and name != 'nohidden':
        # the norm key's sum runs over the rows in their new order: its last bits may move, so equal order needs distinct keys
        for k, _ in CR.keys_of(spec, once[0], key, sign):
            assert (np.diff(np.sort(k, axis=1), axis=1) > 1e-9 * np.abs(np.sort(k, axis=1)[:, 1:])).all()
    assert np.array_equal(out, once[0])
    assert np.array_equal(perm, np.broadcast_to(np.concatenate([np.arange(w) for w in spec.hidden_structure[:-1]] + [np.arange(0)]),
                                                perm.shape))
    assert (sgn == 1).all()


@pytest.mark.parametrize('name', ['perm', 'w64x3', 'deep12', 'wide'])
def test_the_orbit_has_one_representative(name):
    spec, theta = CR.case_spec(name), CR.case_draws(name)
    tanh = spec.activation == 'tanh'
    for key, sign in CR.case_combos(name):
        for k, _ in CR.keys_of(spec, theta, key, sign):     # the case's keys are pairwise distinct (with room for the norm key's
            ks = np.sort(k, axis=1)                         # last bits) and no bias is 0: the orbit has ONE sorted member
            assert (np.diff(ks, axis=1) > 1e-9 * np.abs(ks[:, 1:])).all(), (name, key, sign)
        for ob, _, _, fout in CR._layers(spec)[:-1]:
            assert (theta[:, ob:ob + fout] != 0).all()
        moved = CR.orbit_member(spec, theta, seed=5, flips=tanh and sign)
        assert not np.array_equal(moved, theta)
        ref = CR.case_canonical(name, key, sign)
        assert np.array_equal(CR.canonicalize(spec, moved, key, sign)[0], ref[0]), (name, key, sign)
        assert np.array_equal(_dense(spec, moved, key, sign)[0], ref[0]), (name, key, sign)


@pytest.mark.parametrize('name', ['perm', 'w64x3', 'deep12', 'width1', 'wide'])
def test_the_function_does_not_move(name):
    spec, theta = CR.case_spec(name), CR.case_draws(name)
    ospec = O.ModelSpec(spec.in_features, spec.hidden_structure, activation=spec.activation, task=spec.task)
    X = np.random.default_rng(3).standard_normal((6, spec.in_features))
    before = O.mlp_forward(ospec, theta.astype(np.float64), X)
    for key, sign in CR.case_combos(name):
        after = O.mlp_forward(ospec, CR.case_canonical(name, key, sign)[0].astype(np.float64), X)
        moved = float(np.abs(after - before).max())
        print(f'CANON {name} {key} sign={sign}: fp64 outputs moved {moved:.2e}')
        assert moved < 1e-12


def test_permutation_case_in_parameter_space():
    """Three chains around one mode of [3 -> 8 -> 8 -> 2] tanh, chains 1 and 2 permuted: fp64 parameter-space max rhat 2.4091 raw,
    1.0370 canonical under all four rule combinations, with none of the 122 parameters above 1.1."""
    from mile_amd import metrics as M
    spec, theta = CR.permutation_spec(), CR.permutation_draws()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        raw = R.chain_diagnostics(theta, 2)['rhat']
        assert raw.max() > 2.0
        for key, sign in CR.COMBOS:
            out, perm, _ = CR.permutation_canonical(key, sign)
            rhat = R.chain_diagnostics(out, 2)['rhat']
            sw = CR.switches(perm, F.PERM_WIDTHS[:-1])
            print(f'CANON permutation fp64 {key} sign={sign}: parameter rhat max raw {raw.max():.4f} canonical {rhat.max():.4f}  '
                  f'above 1.1: {int((rhat > 1.1).sum())} of {rhat.size}  switches {sw.tolist()}')
            assert rhat.max() < 1.1
            got = M.canonical_diagnostics(spec, torch.from_numpy(np.array(theta)), 2, key=key, sign=sign)
            assert M.LAST_CANON_PATH == 'torch' and M.LAST_DIAG_PATH == 'torch'
            np.testing.assert_allclose(got['rhat'].numpy(), rhat, rtol=1e-9)
            assert np.array_equal(got['switches'].numpy(), sw) and float(got['rhat'].max()) < 1.1
            c3 = M.canonicalize(spec, torch.from_numpy(np.array(theta)), key, sign)
            assert c3.shape == theta.shape and np.array_equal(c3.numpy(), out)


def test_permutation_switches_on_a_hand_made_perm():
    from mile_amd import ModelSpec
    from mile_amd import metrics as M
    spec = ModelSpec(2, (3, 2, 2), activation='relu', task='regr')
    perm = np.array([[[0, 1, 2, 0, 1], [0, 1, 2, 1, 0], [0, 2, 1, 1, 0], [0, 2, 1, 1, 0], [1, 2, 0, 0, 1]],
                     [[2, 1, 0, 0, 1], [2, 1, 0, 0, 1], [2, 1, 0, 0, 1], [2, 1, 0, 0, 1], [2, 1, 0, 0, 1]]], np.int32)
    got = M.permutation_switches(torch.from_numpy(perm), spec)
    assert got.dtype == torch.int64 and got.tolist() == [[2, 2], [0, 0]] and CR.switches(perm, (3, 2)).tolist() == got.tolist()
    with pytest.raises(ValueError):
        M.permutation_switches(torch.from_numpy(perm[:, :, :4]), spec)


def test_python_refusals():
    from mile_amd import ModelSpec
    from mile_amd import metrics as M
    from mile_amd.spec import LeNettiSpec
    relu = ModelSpec(3, (4, 2), activation='relu', task='regr')
    th = torch.zeros((2, relu.n_params))
    with pytest.raises(ValueError, match='tanh only'):
        M.canonicalize(relu, th, sign=True)
    with pytest.raises(ValueError, match='key'):
        M.canonicalize(relu, th, key='weight')
    with pytest.raises(ValueError, match='theta must be'):
        M.canonicalize(relu, th[:, :-1])
    with pytest.raises(ValueError, match='FCN only'):
        M.canonicalize(LeNettiSpec.__new__(LeNettiSpec), th)


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
    assert _lib.SIGNATURES['mile_canonicalize_fcn'] == (i32, [sp, p, i64, u32, p, p, p, p, i64, p])
    assert _lib.SIGNATURES['mile_canonicalize_fcn_workspace'] == (i64, [sp, i64, u32])
    assert _lib.SIGNATURES['mile_canonical_hidden'] == (i64, [sp])
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_canonicalize_fcn(const mile_model_spec *spec, const float *theta, int64_t M, uint32_t how, float *out, '
            'int32_t *perm, int8_t *sign, void *workspace, int64_t workspace_bytes, void *stream);') in header
    assert 'int64_t mile_canonicalize_fcn_workspace(const mile_model_spec *spec, int64_t M, uint32_t how);' in header
    assert 'int64_t mile_canonical_hidden(const mile_model_spec *spec);' in header
    for name, v in (('KEY_BIAS 0u', 0), ('KEY_NORM 1u', 1), ('SIGN 2u', 2), ('WIDTH_MAX 1024', 1024)):
        assert f'#define MILE_CANON_{name}' in header
    assert _lib.CANON_BITS == {'bias': 0, 'norm': 1, 'sign': 2} and _lib.CANON_WIDTH_MAX == 1024

    good = _cspec()
    d = 3 * 8 + 8 + 8 * 8 + 8 + 8 * 2 + 2
    # host memory stands in for the device pointers: every one of these calls is refused before anything reads them
    theta = (C.c_float * (4 * d))()
    out = (C.c_float * (4 * d))()
    T, Out = C.cast(theta, p), C.cast(out, p)

    def refused(rc, word, code=-1):
        msg = lib.mile_last_error()
        assert rc == code and b'mile_canonicalize_fcn: ' in msg and word in msg, (rc, msg)

    call = lambda spec=good, th=T, M=4, how=0, o=Out, ws=None, nws=0: lib.mile_canonicalize_fcn(
        C.byref(spec) if spec is not None else None, th, M, how, o, None, None, ws, nws, None)
    refused(call(spec=None), b'null spec, theta or out')
    refused(call(th=None), b'null spec, theta or out')
    refused(call(o=None), b'null spec, theta or out')
    refused(call(M=0), b'M out of range')
    lenet = _cspec()
    lenet.model = _lib.MODEL_IDS['lenet']
    refused(call(spec=lenet), b'only MILE_MODEL_FCN')
    nobias = _cspec()
    nobias.use_bias = 0
    refused(call(spec=nobias), b'use_bias must be 1')
    refused(call(how=4), b'unknown bits in `how`')
    refused(call(spec=_cspec(act='relu'), how=2), b'tanh only')
    refused(call(spec=_cspec(act='sigmoid'), how=3), b'tanh only')
    wide = _cspec(hs=(1025, 2))
    refused(call(spec=wide), b'hidden width above MILE_CANON_WIDTH_MAX')
    refused(call(o=T), b'out overlaps theta')
    refused(call(o=C.c_void_p(T.value + 4 * (4 * d - 1))), b'out overlaps theta')
    refused(call(th=C.c_void_p(Out.value + 4 * d)), b'out overlaps theta')
    # a draw that does not fit the LDS needs the workspace of the tiled form
    big = _cspec(fin=54, hs=(256, 256, 7), act='relu', task='classification')
    need = lib.mile_canonicalize_fcn_workspace(C.byref(big), 2, 1)
    assert need == 2 * 512 * 4
    far = C.c_void_p(T.value + (1 << 40))                                      # (never read: the workspace check comes first)
    refused(call(spec=big, M=2, o=far, how=1), b'workspace too small', code=-2)
    refused(call(spec=big, M=2, o=far, how=1, ws=T, nws=need - 1), b'workspace too small', code=-2)

    hidden = lambda s: lib.mile_canonical_hidden(C.byref(s) if s is not None else None)
    assert hidden(good) == 16 and hidden(big) == 512 and hidden(_cspec(hs=(2,))) == 0
    assert hidden(_cspec(fin=4, hs=(3,) * 11 + (2,))) == 33
    assert hidden(None) == -1 and b'mile_canonical_hidden: null spec' in lib.mile_last_error()
    assert hidden(lenet) == -1 and hidden(nobias) == -1 and hidden(wide) == -1
    zero = _cspec()
    zero.widths[1] = 0
    assert hidden(zero) == -1 and b'layer width' in lib.mile_last_error()
    nl = _cspec()
    nl.n_layers = 17
    assert hidden(nl) == -1 and b'n_layers' in lib.mile_last_error()
    ws = lambda s, M, how: lib.mile_canonicalize_fcn_workspace(C.byref(s) if s is not None else None, M, how)
    assert ws(good, 1000, 3) == 0 and ws(_cspec(fin=9, hs=(256, 130, 7), act='sigmoid', task='classification'), 3, 1) == 0
    assert ws(big, 5, 0) == 5 * 512 * 4
    assert ws(None, 4, 0) == -1 and ws(good, 0, 0) == -1 and ws(good, 4, 8) == -1 and ws(_cspec(act='relu'), 4, 2) == -1 and ws(wide, 4, 0) == -1
    assert b'mile_canonicalize_fcn_workspace: ' in lib.mile_last_error()


def test_evaluate_flags_and_refusals(capsys):
    sys.path.insert(0, str(ROOT))
    import evaluate as EV
    ap = EV.build_parser()
    a = ap.parse_args(['-e', 'x'])
    assert a.canonical_diagnostics is None and a.canonical_key == 'bias' and a.canonical_sign is False      # opt-in
    a = ap.parse_args(['-e', 'x', '--canonical-diagnostics', '--canonical-key', 'norm', '--canonical-sign'])
    assert a.canonical_diagnostics == 2 and a.canonical_key == 'norm' and a.canonical_sign is True
    assert ap.parse_args(['-e', 'x', '--canonical-diagnostics', '4']).canonical_diagnostics == 4
    with pytest.raises(SystemExit):
        ap.parse_args(['-e', 'x', '--canonical-key', 'weight'])
    with pytest.raises(SystemExit):
        ap.parse_args(['--help'])
    text = capsys.readouterr().out
    for flag in ('--canonical-diagnostics', '--canonical-key', '--canonical-sign'):
        assert flag in text
    assert 'canonical-diagnostics' in EV.__doc__
    assert EV.canonical_refusal('FCN', 'tanh', True) is None and EV.canonical_refusal('FCN', 'relu', False) is None
    assert 'FCN experiments only' in EV.canonical_refusal('LeNet', None, False)
    assert 'odd activation' in EV.canonical_refusal('FCN', 'relu', True)


@pytest.mark.parametrize('argv,word', [(['--canonical-diagnostics'], 'FCN experiments only'),
                                       (['--canonical-diagnostics', '--canonical-sign'], 'odd activation')])
def test_evaluate_refuses_before_any_work(tmp_path, monkeypatch, argv, word):
    """evaluate.py on a LeNetti experiment, and with --canonical-sign on a relu FCN: SystemExit with the reason, before the model,
    the samples or a device are touched (the directory holds a config.yaml and nothing else)."""
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

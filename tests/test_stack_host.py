"""Stacking on the host: metrics.stack_eval_dense and metrics.stacking_weights against the NumPy restatement of
tests/stack_ref.py on seeded synthetic [C, N] matrices, the new symbols and their refusals (which need no GPU), the sizing
helpers of mile_stack.h under the address and undefined-behaviour sanitizers in a program of their own, and evaluate.py's
--stacking arguments.

Bounds.  stack_eval_dense and the restatement are the same fp64 formulas in another summation order: 1e-9 max(1, |value|), the
project's bound for fixed-order fp64 sums (tests/test_gpu_loo.py).  The solver's own bounds are the ones its certificate gives:
gap <= 1e-8 within 50 iterations, and the score no lower than any feasible point's minus the gap."""
import ctypes as C
import functools
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from mile_amd import metrics as M
from tests import stack_ref as SR

ROOT = Path(__file__).resolve().parent.parent
CASES = [(f, c, n) for (c, n) in SR.HOST_SHAPES for f in SR.FAMILIES]


@functools.lru_cache(maxsize=None)
def _solved(family, Cn, N):
    lpd = SR.make_case(family, Cn, N)
    return lpd, SR.stacking_weights_ref(lpd), M.stacking_weights(torch.from_numpy(lpd))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


# ---------------------------------------------------------------- the evaluation ----------------
@pytest.mark.parametrize('family,Cn,N', CASES)
def test_dense_evaluation_is_the_definition(family, Cn, N):
    lpd = SR.make_case(family, Cn, N).copy()
    rng = np.random.default_rng(Cn + N)
    if N >= 5:
        lpd[rng.integers(Cn), 1] = np.nan
        lpd[:, 3] = -np.inf
        lpd[rng.integers(Cn), 4] = np.inf
    for tag, w in (('uniform', np.full(Cn, 1.0 / Cn)), ('random', rng.dirichlet(np.ones(Cn)))):
        ref = SR.stack_eval_ref(lpd, w)
        got = M.stack_eval_dense(torch.from_numpy(lpd), torch.from_numpy(w), outputs=('score', 'row_score', 'grad', 'hess', 'used'))
        assert int(got['used']) == ref['used'] == (N - 3 if N >= 5 else N)
        assert (np.isnan(got['row_score'].numpy()) == np.isnan(ref['row_score'])).all()
        fin = ~np.isnan(ref['row_score'])
        worst = {'score': _rel(got['score'], ref['score']), 'row_score': _rel(got['row_score'].numpy()[fin], ref['row_score'][fin]),
                 'grad': _rel(got['grad'], ref['grad']), 'hess': _rel(got['hess'], ref['hess'])}
        assert all(v <= 1e-9 for v in worst.values()), (family, Cn, N, tag, worst)
        h = got['hess'].numpy()
        assert np.array_equal(h, h.T)
        assert abs(float(w @ ref['grad']) - 1.0) <= 1e-12                 # sum_c w_c R_cn = 1 on every used row


def test_rows_left_out_and_counted():
    lpd = SR.make_case('distinct', 3, 7).copy()
    lpd[1, 2] = np.nan
    lpd[:, 5] = -np.inf
    r = M.stack_eval_dense(torch.from_numpy(lpd), np.full(3, 1 / 3), outputs=('score', 'row_score', 'used'))
    assert int(r['used']) == 5 and np.isnan(r['row_score'].numpy()).tolist() == [False, False, True, False, False, True, False]
    assert abs(float(r['score']) - float(np.nanmean(r['row_score'].numpy()))) <= 1e-12
    lpd[0, 0] = -np.inf                                                    # one chain at -inf: the row stays
    assert int(M.stack_eval_dense(torch.from_numpy(lpd), np.full(3, 1 / 3), outputs=('used',))['used']) == 5
    sol = M.stacking_weights(torch.from_numpy(lpd))
    assert sol['converged'] and sol['used'] == 5


def test_a_start_without_mass_on_a_row_is_minus_inf_and_no_exception():
    lpd = SR.make_case('distinct', 3, 7).copy()
    lpd[1:, 2] = -np.inf                                                   # only chain 0 covers row 2
    w0 = np.array([0.0, 0.5, 0.5])
    r = M.stack_eval_dense(torch.from_numpy(lpd), w0, outputs=('score', 'used'))
    assert float(r['score']) == -np.inf and int(r['used']) == 7
    assert SR.stack_eval_ref(lpd, w0)['score'] == -np.inf
    sol = M.stacking_weights(torch.from_numpy(lpd), w0=w0)
    assert sol['converged'] is False and sol['score'] == -np.inf and sol['iterations'] == 0
    assert M.weighted_lppd(torch.from_numpy(lpd), w0) == -np.inf


# ---------------------------------------------------------------- the solver --------------------
@pytest.mark.parametrize('family,Cn,N', CASES)
def test_solver_converges_with_a_certificate(family, Cn, N):
    lpd, ref, got = _solved(family, Cn, N)
    assert ref['converged'] and ref['gap'] <= 1e-8 and ref['iterations'] <= 50, ref      # the restatement itself, on these seeds
    assert got['converged'] and got['gap'] <= 1e-8 and got['iterations'] <= 50, got
    w = got['w']
    assert abs(w.sum() - 1.0) <= 1e-12 and (w >= 0).all()
    equal = SR.stack_eval_ref(lpd, np.full(Cn, 1.0 / Cn))['score']
    assert got['score'] >= equal
    assert abs(M.weighted_lppd(torch.from_numpy(lpd), w) - got['score']) <= 1e-12
    assert got['iterations'] == ref['iterations'] and abs(got['score'] - ref['score']) <= 1e-9
    cond = SR.support_condition(lpd, ref['w'])
    print(f'{family} {Cn}x{N}: {got["iterations"]} Newton steps, {got["score_evals"]} line-search evaluations, gap {got["gap"]:.2e}, '
          f'score - equal {got["score"] - equal:.3e}, support {(w > 1e-10).sum()}, cond {cond:.2e}')
    if cond < 1e8:                                                         # elsewhere the optimum is a face, not a point
        assert np.abs(w - ref['w']).max() <= 1e-6
    if Cn == 1:
        assert w.tolist() == [1.0] and got['iterations'] == 0 and got['score_evals'] == 0


@pytest.mark.parametrize('family,Cn,N', CASES)
def test_solver_is_no_worse_than_two_thousand_multiplicative_updates(family, Cn, N):
    lpd, _, got = _solved(family, Cn, N)
    em = SR.em_lower_bound(lpd, 2000)
    score = SR._eval_fast(lpd, got['w'], need_hess=False)[0]            # both points through one evaluator: equal points, equal bits
    print(f'{family} {Cn}x{N}: score - EM score = {score - em:.3e}, gap {got["gap"]:.2e}')
    assert abs(score - got['score']) <= 1e-12
    assert score >= em - got['gap']


@pytest.mark.parametrize('family,Cn,N', [c for c in CASES if c[1] in (3, 12, 64)])
def test_permuting_the_chains_permutes_the_weights(family, Cn, N):
    lpd, ref, got = _solved(family, Cn, N)
    perm = np.random.default_rng(7).permutation(Cn)
    moved = M.stacking_weights(torch.from_numpy(np.ascontiguousarray(lpd[perm])))
    assert moved['converged'] and abs(moved['score'] - got['score']) <= 1e-9
    if SR.support_condition(lpd, ref['w']) < 1e8:
        assert np.abs(moved['w'] - got['w'][perm]).max() <= 1e-6


def test_max_iter_is_reported_not_raised():
    lpd = SR.make_case('distinct', 12, 1052)
    sol = M.stacking_weights(torch.from_numpy(lpd), max_iter=1)
    assert sol['converged'] is False and sol['iterations'] == 1 and sol['gap'] > 1e-8 and np.isfinite(sol['score'])
    assert abs(sol['w'].sum() - 1.0) <= 1e-12


def test_summary_counts_per_chain():
    rows = {'elpd_loo': np.array([[-1.0, -2.0, np.nan], [-0.5, -0.5, -0.5]]), 'khat': np.array([[0.2, 0.9, np.nan], [0.71, 0.7, 1.5]])}
    s = M.stacking_summary(rows)
    assert s == {'chain_elpd_loo': [-3.0, -1.5], 'chain_rows_nan': [1, 0], 'chain_khat_bad': [1, 2], 'n_rows': 3}


# ---------------------------------------------------------------- C ABI -------------------------
def test_library_exports_the_new_symbols_under_abi_10():
    from mile_amd import _lib
    from mile_amd._build import build_library
    build_library()
    lib = _lib.load_library()
    p, i32, i64, f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    want = {'mile_chain_loo_stream': (i32, [p, p, i32, i64, p, p, i64, f64, p, p, p, p, p, i64, i64, p]),
            'mile_chain_loo_stream_workspace': (i64, [p, i32, i64, i64]),
            'mile_stack_eval': (i32, [p, p, i32, i64, p, p, p, p, p, i64, p])}
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig and hasattr(lib, name), name
    assert lib.mile_abi_version() == _lib.ABI_VERSION == 10
    header = ' '.join((ROOT / 'include' / 'mile_hip.h').read_text().split())
    assert ('int32_t mile_stack_eval(const double *lpd, const double *w, int32_t C, int64_t N, double *score, double *row_score, '
            'double *grad, double *hess, int64_t *used, int64_t max_rows_per_tile, void *stream);') in header
    assert 'int64_t mile_chain_loo_stream_workspace(const mile_sampler *s, int32_t C, int64_t S, int64_t N);' in header


def test_stack_eval_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(lpd=p, w=p, Cn=3, N=4, outs=(p, p, p, p, p), tile=0):
        return lib.mile_stack_eval(lpd, w, Cn, N, *outs, tile, None)
    for tag, kw, text in [('null lpd', dict(lpd=None), 'null'), ('null w', dict(w=None), 'null'), ('C = 0', dict(Cn=0), 'C out of range'),
                          ('C = 1025', dict(Cn=1025), 'C out of range (1 .. 1024)'), ('N = 0', dict(N=0), 'N out of range'),
                          ('N = 2^30', dict(N=1 << 30), 'N out of range'), ('tile < 0', dict(tile=-1), 'max_rows_per_tile'),
                          ('no output', dict(outs=(None,) * 5), 'no output')]:
        assert call(**kw) == -1, tag
        msg = lib.mile_last_error().decode()
        assert 'mile_stack_eval' in msg and text in msg, (tag, msg)


def test_chain_loo_stream_refuses_bad_arguments_without_a_gpu():
    from mile_amd import _lib
    from tests.test_predict_host import _fcn_cspec
    lib = _lib.load_library()
    h = C.c_void_p()
    assert lib.mile_create(C.byref(_fcn_cspec(5, (16, 16, 2))), 0, C.byref(h)) == 0
    buf = (C.c_double * 1024)()
    p = C.cast(buf, C.c_void_p)

    def call(hh, theta=p, Cn=3, S=8, X=p, y=p, N=4, r_eff=1.0, outs=(p, p, p, p, p), passes=0, tile=0):
        return lib.mile_chain_loo_stream(hh, theta, Cn, S, X, y, N, r_eff, *outs, passes, tile, None)
    try:
        for tag, hh, kw, text in [('null handle', None, {}, 'null'), ('null theta', h, dict(theta=None), 'null'), ('null X', h, dict(X=None), 'null'),
                                  ('null y', h, dict(y=None), 'null'), ('C = 0', h, dict(Cn=0), 'C out of range (1 .. 1024)'),
                                  ('C = 1025', h, dict(Cn=1025), 'C out of range'), ('S = 1', h, dict(S=1), 'S out of range (2 .. 2^20)'),
                                  ('N = 0', h, dict(N=0), 'N out of range'), ('no output', h, dict(outs=(None,) * 5), 'no output'),
                                  ('r_eff = 0', h, dict(r_eff=0.0), 'r_eff'), ('passes < 0', h, dict(passes=-1), 'max_draws_per_pass'),
                                  ('tile < 0', h, dict(tile=-1), 'max_rows_per_tile')]:
            assert call(hh, **kw) == -1, tag
            msg = lib.mile_last_error().decode()
            assert 'mile_chain_loo_stream' in msg and text in msg, (tag, msg)
        assert lib.mile_chain_loo_stream_workspace(h, 12, 1000, 1052) == lib.mile_loo_stream_workspace(h, 1000, 1052) > 0
        for Cn, S, N in ((0, 8, 4), (1025, 8, 4), (3, 1, 4), (3, 8, 0)):
            assert lib.mile_chain_loo_stream_workspace(h, Cn, S, N) == -1
    finally:
        lib.mile_destroy(h)


# ---------------------------------------------------------------- sizing under the sanitizers ---
_MAIN = r'''
#include <stdio.h>
#include <stddef.h>
#include "mile_stack.h"
static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails at C=%lld N=%lld cap=%lld\n", __LINE__, #c, (long long)C, (long long)N, (long long)cap); ++bad; } } while (0)
int main() {
  const long long Cs[] = {1, 2, 3, 12, 17, 62, 63, 64, 65, 126, 127, 128, 1000, 1023, 1024};
  const long long Ns[] = {1, 2, 7, 31, 32, 33, 63, 64, 65, 1052, 32703, 32704, 32705, 36000, 1000000, (1LL << 30) - 1};
  const long long caps[] = {0, 1, 32, 33, 1 << 20};
  for (long long C : Cs) for (long long N : Ns) for (long long cap : caps) {
    CHECK(stk_bad_args(C, N, cap, true) == nullptr);
    const long long B = stk_block_rows(C, N), nb = stk_blocks(C, N), Nt = stk_tile_rows(C, N, cap);
    CHECK(B >= 32 && B % 32 == 0);
    CHECK(nb >= 1 && nb <= STK_MAX_BLOCKS && (nb - 1) * B < N && nb * B >= N);
    CHECK(nb == 1 || (long long)stk_part_bytes(C, N) <= STK_PART_BYTES + 256);
    CHECK((long long)stk_part_bytes(C, N) >= nb * (C + 2) * (C + 2) * 8);
    CHECK(Nt >= 1 && Nt <= N && (cap == 0 || Nt <= cap) && Nt <= 0x7fffffff);
    CHECK((long long)stk_rx_bytes(C, Nt) <= STK_R_BYTES + 256 && (long long)stk_rx_bytes(C, Nt) >= (C + 2) * Nt * 8);
    // the blocks a tile touches stay inside the partials, whatever the tile
    for (long long r0 = 0; r0 < N; r0 += (N / 3 > Nt ? N / 3 / Nt * Nt : Nt)) {
      const long long nt = Nt < N - r0 ? Nt : N - r0;
      CHECK(r0 / B >= 0 && (r0 + nt - 1) / B < nb && (r0 + nt - 1) / B - r0 / B + 1 <= 65535);
    }
  }
  long long C = 3, N = 4, cap = 0;
  CHECK(stk_bad_args(0, N, 0, true) && stk_bad_args(1025, N, 0, true) && stk_bad_args(-1, N, 0, true));
  CHECK(stk_bad_args(C, 0, 0, true) && stk_bad_args(C, 1LL << 30, 0, true) && stk_bad_args(C, -5, 0, true));
  CHECK(stk_bad_args(C, N, -1, true) && stk_bad_args(C, N, 0, false));
  CHECK(stk_block_rows(12, 1052) == 32 && stk_blocks(12, 1052) == 33 && stk_tile_rows(1024, 36000, 0) == 32704);
  printf("%s\n", bad ? "FAILED" : "stack sizing ok");
  return bad != 0;
}
'''


def test_sizing_helpers_under_address_and_undefined_sanitizers(tmp_path):
    """mile_stack.h's host side (argument checks, block and tile sizing, workspace bytes) in a program of its own, built with
    -fsanitize=address,undefined: every invariant the kernels' indexing rests on, over the corners of the shape range."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    (tmp_path / 'main.cpp').write_text(_MAIN)
    exe = tmp_path / 'stack_sizing'
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I', str(ROOT / 'mile_amd' / 'csrc'), str(tmp_path / 'main.cpp'), '-o', str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and 'stack sizing ok' in res.stdout and 'runtime error' not in res.stderr, (res.stdout[-2000:], res.stderr[-2000:])


# ---------------------------------------------------------------- CLI ---------------------------
def test_evaluate_parser_accepts_stacking():
    import evaluate as EV
    ap = EV.build_parser()
    assert ap.parse_args(['-e', 'x']).stacking is False                 # opt-in
    args = ap.parse_args(['-e', 'x', '--stacking', '--r-eff', '0.5'])
    assert args.stacking is True and args.loo_r_eff == 0.5 and args.loo is False
    assert ap.parse_args(['-e', 'x', '--stacking', '--loo-r-eff', '2']).loo_r_eff == 2.0
    assert 'TRAIN split' in ' '.join(ap.format_help().split()) and '--stacking' in ap.format_help()
    assert EV.stacking_refusal(4, 12) is None
    assert 'at least 2 draws per chain' in EV.stacking_refusal(4, 1) and EV.stacking_refusal(4, 1).startswith('--stacking:')
    assert 'at most 1024 chains' in EV.stacking_refusal(1025, 12)


def test_stacking_metrics_keys_and_arrays():
    import evaluate as EV
    train = SR.make_case('distinct', 12, 1052)
    test = SR.make_case('distinct', 12, 200, seed=1)
    rows = {'elpd_loo': torch.from_numpy(train), 'khat': torch.from_numpy(np.where(train < -6.0, 0.9, 0.1))}
    keys, arrays = EV.stacking_metrics(rows, torch.from_numpy(test))
    assert sorted(keys) == sorted('stacking_' + k for k in ('lppd', 'lppd_equal', 'gain', 'gap', 'iterations', 'converged',
                                                             'effective_chains', 'khat_bad', 'weights'))
    assert sorted(arrays) == ['chain_elpd_loo', 'chain_khat_bad', 'gap', 'n_eval', 'n_train', 'n_train_used', 'weights']
    assert keys['stacking_converged'] is True and keys['stacking_gap'] <= 1e-8 and abs(sum(keys['stacking_weights']) - 1) <= 1e-12
    eq = float(np.mean(np.log(np.mean(np.exp(test), axis=0))))
    assert abs(keys['stacking_lppd_equal'] - eq) <= 1e-12 and abs(keys['stacking_gain'] - (keys['stacking_lppd'] - eq)) <= 1e-12
    assert 1.0 <= keys['stacking_effective_chains'] <= 12.0 and keys['stacking_khat_bad'] == int((train < -6.0).sum())
    assert arrays['n_train'] == arrays['n_train_used'] == 1052 and arrays['n_eval'] == 200
    assert np.allclose(arrays['chain_elpd_loo'], train.sum(axis=1))

"""The case table of tests/wide_schedule.py has no holes, proven without a GPU: every cell of launch_grad_wide's schedule that the
layers above the library do not refuse gets a launch, every tabulated seed keeps its problem off the ReLU kink without masking a
row, the restatement agrees with the facts the sources and the other tests state, and a schedule that drops the last K chunk of a
dW, counts the bias gradient once per M tile, stores a later chunk instead of accumulating it, drops the last rows of a head block
or reads a window one row late misses the per-leaf bound of tests/test_gpu_wide_schedule.py by more than 10x on a leaf it touches
(measured on the fp64 oracle: 40x at the least, the one row that w200-136-n1153 leaves to its last K chunk; the same case's
dropped head-block row 69x, the late window 2185x, the stored chunk and the bias gradient beyond 1e4)."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import leafcheck as L
from tests import wide_schedule as W

CSRC = Path(__file__).resolve().parents[1] / 'mile_amd' / 'csrc'


# ---- the restatement against the sources ----------------------------------------------------------------------------------------

def _src(name):
    return (CSRC / name).read_text()


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def test_constants_are_the_sources():
    """The tile, K chunk, head block and workspace constants, parsed: a later change of one of them fails here instead of silently
    moving cases out of their cells."""
    hip, mm3 = _src('mile_hip.hip'), _src('mile_mm3.h')
    assert int(_one(r'#define MILE_MM_KC (\d+)', hip)) == W.KC
    assert int(_one(r'#define WH_KMAX (\d+)', mm3)) == W.WH_KMAX
    assert int(_one(r'constexpr int HB_ROWS = (\d+);', hip)) == W.HB_ROWS
    # launch_mm3_k: FULL, the grid
    assert _one(r'if \(p\.M % (\d+) == 0 && p\.N % (\d+) == 0\)', hip) == (str(W.TILE),) * 2
    assert _one(r'const int mtiles = \(p\.M \+ (\d+)\) / (\d+);', hip) == (str(W.TILE - 1), str(W.TILE))
    assert _one(r'const dim3 grid\(\(p\.N \+ (\d+)\) / (\d+), mtiles, batch\);', hip) == (str(W.TILE - 1), str(W.TILE))
    assert 'q.c_vec = (p.ldc % 4 == 0) && (p.sC % 4 == 0) && (((uintptr_t)p.C & 15) == 0);' in hip
    assert 'if (COLSUM && batch % 8 == 0) q.xcd_remap = 2;' in hip and 'else if (!COLSUM && grid.x > 1 && grid.y >= 8) q.xcd_remap = 1;' in hip
    # k_mm3: tile origin, K walk, the remainder of placement 1, who writes the column sums
    assert _one(r'const int n0 = bx \* (\d+);', mm3) == str(W.TILE) and _one(r'const int m0 = by \* (\d+);', mm3) == str(W.TILE)
    assert 'const int nk = (K + KC - 1) / KC;' in mm3
    assert f'const int ksteps = min(KC / {W.KSTEP}, (K - KC * kc + {W.KSTEP - 1}) / {W.KSTEP});' in mm3
    assert 'const int nfull = ny / 8 * 8;' in mm3
    assert re.search(r'if constexpr \(COLSUM\) \{\s*if \(by == 0\)', mm3)
    # the head block: four waves, a row each
    assert '__launch_bounds__(256) void k_wide_headblock(' in mm3
    assert f'for (int r = rbeg + wave; r < rend; r += {W.HB_WAVES})' in mm3
    # launch_grad_wide: the head block's condition, the layout
    assert 'const bool headblock = TERMS == 3 && L >= 2 && ds.widths[L - 2] <= 256 && ds.widths[L - 1] <= WH_KMAX;' in hip
    assert 'if (Wl == 256) MILE_HB(K_, true); else MILE_HB(K_, false);' in hip
    assert float(_one(r'double gb = ([\d.]+);\s*if \(const char \*ev = getenv\("MILE_WIDE_WS_GB"\)\)', hip)) == W.WS_GB
    assert 'R = std::min<size_t>(std::max<size_t>(R, 128), Nall);' in hip and 'if (R < Nall) R = std::max<size_t>(128, R / 128 * 128);' in hip
    assert 'if (E != s->wide_E || !s->wide_ws) {' in hip
    # the padded widths and the floats per row, in the one LayerPlan (tests/test_wide_plan_host.py checks its integers)
    plan = _src('mile_layer_plan.h')
    assert _one(r'wp\[l\] = \(fout_ \+ (\d+)\) / (\d+) \* (\d+);', plan) == ('7', '8', '8') and W.up8(17) == 24
    assert 'size_t per_row() const { return sum_wp + 2 * (size_t)maxwp; }' in plan and 'size_t R = budget / ((size_t)E * pl.per_row());' in hip
    # the parameter layout: bias, then kernel
    assert re.search(r'ds\.b_off\[li\] = \(int\)off; off \+= fout;\s*ds\.w_off\[li\] = \(int\)off; off \+= \(long long\)fin \* fout;', hip)


def test_launch_info_row_of_the_wide_kernels():
    """tests/test_gpu_parity.py::test_grad_launch_info_per_kernel's row: 256 threads, 65536 bytes of LDS (the dH form's two
    row-major-K images), one row split."""
    pytest.importorskip('torch')
    from tests import test_gpu_parity as P
    for k in (W.X3, W.X1):
        name, grid, block, lds = P.LAUNCH_SHAPES[k]
        assert name.startswith('k_mm3') and block == 256 and lds == W.lds_bytes() and grid[0] == 1
    F, hs, task, N, E = (54, (256, 256, 7), 'classification', 300, 4)
    case = W._c('launch-info', F, hs, 'relu', task, N, E=E)
    assert P.LAUNCH_SHAPES[W.X3][1] == (1, case.E)
    ls = W.launches(case)
    assert [ln['kind'] if ln['kind'] != 'mm3' else ln['form'] for ln in ls] == ['fwd', 'fwd', 'headblock', 'reduce', 'dw', 'dh', 'dw']
    assert [ln['grid'] for ln in ls if ln['kind'] == 'mm3'] == [(2, 3, 4), (2, 3, 4), (2, 2, 4), (2, 3, 4), (2, 1, 4)]


def test_restated_schedule_on_known_shapes():
    # B4 itself: 232404 rows of [54 -> 256 x 4 -> 7] at 128 particles walk in chunks of 16 GiB / (128 * 1544 floats) -> 21632 rows
    assert W.layout_rows((256,) * 4 + (7,), 128, 232404) == 21632
    assert W.layout_rows((96, 4), 2, 130) == 130 and W.layout_rows((96, 4), 2, 130, 128) == 128 and W.layout_rows((96, 4), 2, 130, 500) == 130
    assert W.chunks_of(300, 128) == [128, 128, 44] and W.chunks_of(1153, 576) == [576, 576, 1] and W.chunks_of(256, 256) == [256]
    b4 = W._c('b4', 54, (256,) * 4 + (7,), 'relu', 'classification', 232404, E=128)
    ls = [ln for ln in W.launches(b4) if ln['chunk'] == 0]
    mm = [ln for ln in ls if ln['kind'] == 'mm3']
    assert all(ln['FULL'] for ln in mm if ln['layer'] > 0) and not any(ln['FULL'] for ln in mm if ln['form'] == 'dw' and ln['layer'] == 0)
    assert all(ln['c_vec'] for ln in mm) and {ln['xcd'] for ln in mm if ln['form'] == 'dw'} == {2}
    assert {ln['xcd'] for ln in mm if ln['form'] in ('fwd', 'dh')} == {1}
    hb = [ln for ln in ls if ln['kind'] == 'headblock']
    assert len(hb) == 1 and hb[0]['K'] == 7 and hb[0]['WFULL'] and hb[0]['nblk'] == 43 and hb[0]['last_rows'] == 128
    # offsets: bias before kernel
    b_off, w_off, d, dp = W.offsets(W._c('o', 5, (129, 128, 5), 'tanh', 'classification', 10))
    assert (b_off, w_off) == ([0, 774, 17414], [129, 902, 17419]) and d == 18059 and dp == 18060
    # K walk
    k = {K: W.kshape(W.mm3('fwd', 'relu', 10, 10, K, 16, 160, 0, False, False, 2, 3, 0, 0)) for K in (1, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 127, 264)}
    assert k[1] == k[16] == ('nk 1', 'last <= 16') and k[17] == k[31] == ('nk 1', 'last 17..31') and k[32] == ('nk 1', 'last 32')
    assert k[33] == k[48] == ('nk 2', 'last <= 16') and k[49] == ('nk 2', 'last 17..31') and k[64] == ('nk 2', 'last 32')
    assert k[65] == k[264] == ('nk >= 3', 'last <= 16') and k[96] == ('nk >= 3', 'last 32') and k[127] == ('nk >= 3', 'last 17..31')
    assert [W.last_rows_class(n) for n in (1, 3, 4, 5, 129, 512)] == ['< 4', '< 4', '% 4 == 0', '% 4 != 0', '% 4 != 0', '% 4 == 0']
    assert [W.shape(n) for n in (7, 127, 128, 129, 256, 300)] == [W.SHAPES[0], W.SHAPES[0], W.SHAPES[1], W.SHAPES[2], W.SHAPES[1], W.SHAPES[2]]


def test_what_the_issue_names_is_in_the_table():
    has = {(c.F, c.hidden, c.act, c.task, c.N, c.chunk_rows) for c in W.CASES if c.kernel == W.X3 and c.window is None}
    for want in ((54, (256, 256, 7), 'relu', 'classification', 256, None), (54, (256, 256, 7), 'relu', 'classification', 300, None),
                 (54, (256, 256, 7), 'relu', 'classification', 300, 128), (54, (256,) * 4 + (7,), 'relu', 'classification', 256, None),
                 (20, (160, 12), 'relu', 'classification', 200, None), (7, (96, 4), 'relu', 'classification', 130, None),
                 (7, (256, 8), 'relu', 'classification', 130, None), (5, (129, 127, 2), 'relu', 'regr', 300, None),
                 (9, (264, 264, 2), 'tanh', 'regr', 130, None), (130, (128, 3), 'sigmoid', 'classification', 130, None),
                 (13, (200, 136, 3), 'tanh', 'classification', 1153, None), (13, (100, 50, 20, 3), 'tanh', 'classification', 300, None)):
        assert want in has, want
    assert W.chunks_of(300, W.layout_rows((256, 256, 7), 2, 300, 128)) == [128, 128, 44]
    assert any(c.N in (513, 1025) for c in W.CASES) and {c.E for c in W.CASES} == {2, 3, 8}
    assert any(c.prior == 'Laplace' for c in W.CASES) and any(len(c.hidden) == 1 for c in W.CASES)
    assert all(c.N <= 1200 and max(c.hidden) <= 264 and max(c.hidden[-1:]) <= 16 for c in W.CASES)
    assert all(c.act == 'relu' for c in W.X1_CASES) and any(c.chunk_rows for c in W.X1_CASES)
    for c in W.WINDOW_CASES:
        assert W.base_of(c) in W.X3_CASES and 0 < c.window[1] and c.window[0] + c.window[1] <= c.N


# ---- coverage ------------------------------------------------------------------------------------------------------------------------

def test_every_cell_gets_a_launch(capsys):
    hit = {}
    for c in W.CASES:
        for cell in W.cells_of(c):
            hit.setdefault(cell, []).append(c.name)
    assert set(hit) <= set(W.CELLS), sorted(set(hit) - set(W.CELLS), key=str)               # nothing runs outside the enumeration
    assert set(W.UNREACHABLE) <= set(W.CELLS) and not set(W.UNREACHABLE) & set(hit)
    missing = [cell for cell in W.CELLS if cell not in hit and cell not in W.UNREACHABLE]
    assert not missing, missing
    # regression needs exactly two outputs: the refusal UNREACHABLE cites
    from mile_amd.spec import ModelSpec
    with pytest.raises(ValueError, match='mu, log sigma'):
        ModelSpec(7, (96, 12), task='regr')
    ModelSpec(7, (96, 1), task='classification')                                            # a single class is not refused
    with capsys.disabled():
        print(f'\nWIDESCHED {len(W.CELLS)} cells, {len(W.UNREACHABLE)} unreachable, {len(W.CASES)} cases')
        for c in W.CASES:
            only = sorted((cell for cell, names in hit.items() if names == [c.name]), key=str)
            print(f'WIDESCHED {c.name:<28s} alone in {len(only)} cells' + (': ' + '; '.join(' '.join(map(str, o)) for o in only) if only else ''))


def test_no_two_cases_run_the_same_launches():
    """Of the three-term form, windows included."""
    seen = {}
    for c in W.X3_CASES + W.WINDOW_CASES:
        key = (c[1:6], tuple(sorted((k, str(v)) for ln in W.launches(c) for k, v in ln.items())), c.window)
        assert key not in seen, (c.name, seen.get(key))
        seen[key] = c.name


# ---- seeds -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', [c for c in W.CASES if c.act == 'relu' and len(c.hidden) > 1], ids=lambda c: c.name)
def test_tabulated_seed_is_the_first_clean_one(case):
    """No row is masked (the cap on left-out rows is zero): the tabulated seed is the first in 0..9 with no hidden pre-activation
    within 3e-7 of its layer's largest, on the fp64 oracle.  A window's rows are rows of that problem, whose layer maxima bound
    theirs."""
    net, seed = W.net_of(case), W.seed_of(case)
    assert 0 <= seed < W.SEED_TRIES
    assert W.near_kink(net, case.N, seed) == 0, (case.name, seed)
    assert seed == W.first_clean_seed(net, case.N), (case.name, seed)


def test_seed_table_has_no_stale_entry():
    used = {(c.F, c.hidden, c.N) for c in W.CASES if c.act == 'relu' and len(c.hidden) > 1}
    assert set(W.SEEDS) == used


def test_problem_tiles_two_chains():
    case = W.BY_NAME['w256-n300-rows128-e8']
    ospec, X, y, theta = W.problem(case)
    assert X.shape == (300, 54) and y.shape == (300,) and theta.shape == (8, ospec.n_params) and theta.dtype == np.float32
    assert all(np.array_equal(theta[e], theta[e % 2]) for e in range(8)) and not np.array_equal(theta[0], theta[1])
    lp, g, g32 = W.reference_of(case)
    assert lp.shape == (2,) and g.shape == (2, ospec.n_params) and g32.dtype == np.float32 and not g.flags.writeable
    win = W.BY_NAME['w256-n300-win-interior']
    assert np.abs(W.reference_of(win)[1] - W.reference_of(W.base_of(win))[1]).max() > 0
    lap = W.ospec_of(W.net_of(W.BY_NAME['w256-regr']))
    assert lap.prior == 'Laplace' and lap.prior_scale == 0.7


# ---- mutants -----------------------------------------------------------------------------------------------------------------------

MUTANT_KINDS = ('dw-last-k-chunk-dropped', 'bias-once-per-m-tile', 'last-chunk-stored', 'head-block-tail-dropped', 'window-one-row-late')
_SEEN = {}


def _distinct():
    """One case per (net, N, chunks, window): E does not change the oracle's answer."""
    seen, out = set(), []
    for c in W.X3_CASES + W.WINDOW_CASES:
        if c.hidden[-1] == 1:
            continue                                          # a single class: the likelihood's gradient is zero, nothing to drop
        key = (W.net_of(c), c.N, c.chunk_rows, c.window)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize('case', _distinct(), ids=lambda c: c.name)
def test_a_wrong_schedule_misses_the_bound_tenfold(case):
    """Each mutant misses the GPU test's per-leaf bound -- 5e-5 of the leaf's largest entry, or 8x the float32 oracle's own error --
    by 10x or more on a leaf it touches, in both chains, and the float32 oracle itself is inside the bound."""
    ospec = W.ospec_of(W.net_of(case))
    leaves = L.fcn_leaves(ospec)
    names = [n for n, _, _ in leaves]
    _, g, g32 = W.reference_of(case)
    bound = L.leaf_bounds(leaves, 2, g32=g32, g_ref=g, tol=L.LEAF_TOL, margin=L.F32_MARGIN)
    L.assert_leaves(g32, g, leaves, bound, tag=(case.name, 'float32 oracle'))
    for name, (g_mut, touched) in W.schedule_mutants(case).items():
        cols = [names.index(t) for t in touched]
        ratio = (L.leaf_errors(g_mut, g, leaves) / bound)[:, cols].max(axis=1)
        kind = next(k for k in MUTANT_KINDS if name.startswith(k))
        _SEEN[kind] = min(_SEEN.get(kind, np.inf), float(ratio.min()))
        assert ratio.min() >= 10.0, (case.name, name, ratio)
        with pytest.raises(AssertionError, match='leaf'):
            L.assert_leaves(g_mut, g, leaves, bound, tag=name)


def test_every_kind_of_mutant_was_built(capsys):
    kinds = set()
    for c in _distinct():
        ls = W.launches(c)
        ch = W.chunks_of(c.window[1] if c.window else c.N, W.layout_rows(c.hidden, c.E, c.N, c.chunk_rows))
        if ch[-1] % W.KC and ch[-1] > ch[-1] % W.KC:
            kinds.add(MUTANT_KINDS[0])
        if any(ln['kind'] == 'mm3' and ln['form'] == 'dw' and ln['ny'] >= 2 for ln in ls):
            kinds.add(MUTANT_KINDS[1])
        if len(ch) > 1:
            kinds.add(MUTANT_KINDS[2])
        if any(ln['kind'] == 'headblock' and ln['last_rows'] % W.HB_WAVES for ln in ls):
            kinds.add(MUTANT_KINDS[3])
        if c.window and sum(c.window) < c.N:
            kinds.add(MUTANT_KINDS[4])
    assert kinds == set(MUTANT_KINDS)
    if _SEEN:
        with capsys.disabled():
            print('\nWIDESCHED least miss of the bound per mutant: ' + ', '.join(f'{k} {v:.0f}x' for k, v in sorted(_SEEN.items())))

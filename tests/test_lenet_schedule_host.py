"""The case table of tests/lenet_schedule.py has no holes, proven without a GPU: the restatement's constants and formulas are the
sources', it reproduces the figures tests/test_gpu_lenet_bf16x3.py states, every cell of run_lenet's schedule that can be reached
gets a launch, every case keeps every leaf's likelihood share at 0.5 or more and its ReLU units off the kink without masking a
row, and a schedule that is wrong in one of six ways misses the per-leaf bound of tests/test_gpu_lenet_schedule.py by more than
10x on a leaf it touches.

Measured on the fp64 oracle, the least miss over all cases, as a multiple of the bound (5e-5 of the leaf's largest entry or 8x the
float32 oracle's error for lenet_f32 and lenet_bf16x3; for lenet_bf16 3e-3 or 8x the float32 recipe's error, 60 times as much):

    mutant                              lenet_f32 / lenet_bf16x3   lenet_bf16
    last-chunk-stored                   12898x                     215x
    short-group-last-image-dropped      3158x                      53x
    last-short-workgroup-dropped        3158x                      56x
    bias-one-workgroup-too-often        4641x                      107x
    crop-treated-as-present             1281x                      20x
    window-one-image-late               7950x                      132x"""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import leafcheck as L
from tests import lenet_schedule as S

CSRC = Path(__file__).resolve().parents[1] / 'mile_amd' / 'csrc'
BF16_LEAF_TOL = 3e-3      # tests/test_gpu_lenet.py::test_lenet_mfma_convolutions_match_the_bf16_recipe


# ---- the restatement against the sources ----------------------------------------------------------------------------------------

def _src(name):
    return (CSRC / name).read_text()


def _body(text, name):
    """The definition of function `name`: from its name followed by '(' to the brace that closes its body."""
    for m in re.finditer(r'\b' + re.escape(name) + r'\(', text):
        i = text.find('{', m.end())
        semi = text.find(';', m.end())
        if i < 0 or (0 <= semi < i):
            continue                                              # a declaration or a call
        depth, j = 0, i
        while True:
            depth += {'{': 1, '}': -1}.get(text[j], 0)
            if depth == 0:
                return text[m.start():j + 1]
            j += 1
    raise AssertionError(f'no definition of {name}')


def _one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) == 1, (pattern, m)
    return m[0]


def test_constants_are_the_sources():
    """Each constant and formula where its function states it: a later change fails here instead of silently emptying a cell."""
    hip, f32, mfma = _src('mile_hip.hip'), _src('mile_lenet.h'), _src('mile_lenet_mfma.h')
    run = _body(hip, 'run_lenet')
    assert _one(r'const int ipw = mfma \? (\d+) : (\d+);', run) == (str(S.IPW_MFMA), str(S.IPW_F32))
    ni = _body(hip, 'lenet_ni_for')
    assert _one(r'std::max\(1, std::min\((\d+), \(int\)\((\d+) / \(terms \* per_img\)\)\)\)', ni) == (str(S.NI_CAP), str(S.NI_BYTES))
    assert 'const int terms = x3 ? 3 : 1;' in run
    assert 'const int ni2 = ni_for((size_t)(g.hp1 * g.wp1 + 8) * 16 + (size_t)g.h2 * g.w2 * 32);' in run
    assert 'const int ni_x2 = ni_for((size_t)((g.h2 + 8) * (g.w2 + 8) + 8) * 32), ni_f1 = ni_for((size_t)((g.H + 4) * (g.W + 4) + 8) * 8);' in run
    # the direct form: its condition, its LDS sizes, the compile-time geometries
    assert 'const bool direct = getenv("MILE_LENET_GEMM") == nullptr && g.C <= 16 && lds_max <= 150 * 1024;' in run and S.LDS_LIMIT == 150 * 1024
    assert 'const size_t lds_f1 = (size_t)(25 * g.C * 8 + 8 + g.C * (g.H + 4) * (g.W + 4)) * 4;' in run
    assert 'const size_t lds_w1 = std::max((size_t)(g.C * (g.H + 4) * (g.W + 4)) + HW * 6, 3 * (size_t)(KT1 * 6 + 6)) * 4;' in run
    assert 'const size_t lds_f2 = (size_t)(150 * 16 + 16 + 6 * P1) * 4, lds_x2 = (size_t)(2400 + 1 * (g.h2 + 8) * (g.w2 + 8) * 16) * 4;' in run
    assert 'const size_t lds_w2 = std::max(6 * P1 + HW2 * 16, 3 * (size_t)(2400 + 16)) * 4;' in run
    assert 'const size_t lds_max = std::max({lds_f1, lds_w1, lds_f2, lds_x2, lds_w2});' in run
    assert 'const int geo = (g.C == 3 && g.H == 32 && g.W == 32) ? 1 : (g.C == 1 && g.H == 28 && g.W == 28) ? 3 : 0;' in run
    # the MFMA forms: what they refuse, their LDS sizes
    assert 'if (mfma && (!direct || g.C > 4 || std::max({ldm_f1p, ldm_f2, ldm_x2p, ldm_w1, ldm_w1p, ldm_w2}) > 150 * 1024))' in run
    for k in S.MFMA:
        assert S.RUN_LENET_REFUSAL[k] in run and f'lenet_bf16_supported, "{S.MFMA_REFUSAL[k]}"' in hip, k
    assert 'return is_lenet(s) && s->lg.C <= 4;' in _body(hip, 'lenet_bf16_supported')
    assert 'ldm_f1p = cm_lds_fwd(CM_IN4, g.H, g.W, 2, g.C, 6, ni_f1, terms), ldm_f2 = cm_lds_fwd(CM_IN8, g.hp1, g.wp1, 0, 6, 16, ni2, terms);' in run
    assert 'ldm_x2p = cm_lds_dx2x(g.h2, g.w2, 6, 16, ni_x2, terms), ldm_w1p = cm_lds_dw2x(g.H, g.W, 2, terms);' in run
    assert 'ldm_w2 = cm_lds_dw(CM_IN8, g.hp1, g.wp1, 0, ni2, terms);' in run and 'ldm_w1 = cm_lds_dw(CM_IN4, g.H, g.W, 2);' in run
    b = _body(mfma, 'cm_lds_fwd')
    assert 'const int pb = mode == CM_IN4 ? 8 : 16;' in b
    assert 'return std::max((size_t)terms * ni * ((H + 2 * pad) * (W + 2 * pad) + 8) * pb, (size_t)25 * CIN * COUT * 4);' in b
    assert 'return std::max((size_t)terms * ni * ((Ho + 8) * (Wo + 8) + 8) * 32, (size_t)25 * CIN * COUT * 4);' in _body(mfma, 'cm_lds_dx2x')
    b = _body(mfma, 'cm_lds_dw2x')
    assert 'npairs = Ho * ((Wo + 1) / 2);' in b and 'const size_t red = (size_t)4 * (8 + 1) * 64 * 16;' in b
    assert 'terms * (((size_t)((H + 2 * pad) * (W + 2 * pad) + 8) * 8 + 15) / 16 * 16 + (size_t)((npairs + 31) / 32 * 32) * 32);' in b
    b = _body(mfma, 'cm_lds_dw')
    assert 'const int pb = mode == CM_IN4 ? 8 : 16, ns = mode == CM_IN4 ? 30 : 50;' in b and 'const size_t red = (size_t)4 * ((ns + 3) / 4 + 1) * 64 * 16;' in b
    assert ('terms * ((size_t)ni * (((size_t)((H + 2 * pad) * (W + 2 * pad) + 8) * pb + 15) / 16 * 16) + '
            '(size_t)((ni * Ho * Wo + 31) / 32 * 32) * 32);') in b
    # the tiles and groups of the MFMA kernels
    assert 'TX = (Wo + 15) / 16, ntiles = ((Ho + 1) / 2) * TX;' in _body(mfma, 'k_conv5m_fwd2x')
    assert 'TX = (Wo + 7) / 8, ntiles = ((Ho + 1) / 2) * TX;' in _body(mfma, 'k_conv5m_fwd')
    b = _body(mfma, 'k_conv5m_dx2x')
    assert 'W2 = (W + 1) / 2, npairs = H * W2;' in b and 'const int ntiles = (npairs + 15) / 16' in b
    for k in ('k_conv5m_fwd2x', 'k_conv5m_fwd', 'k_conv5m_dx2x', 'k_conv5m_dw'):
        b = _body(mfma, k)
        assert 'for (int b = b0; b < b1; b += ni)' in b and 'const int nimg = min(ni, b1 - b)' in b, k
        assert 'const int b0 = blockIdx.x * ipw, b1 = min(R, b0 + ipw);' in b, k
    b = _body(mfma, 'cm_image_f')
    assert f'const int nt0 = t0 + {S.PAIR_ROUND};' in b and 'min(t0 + 4, ntiles - 1)' in b
    # the walk, the workgroups, the reduction
    assert _one(r'size_t R = \(\(size_t\)1 << (\d+)\) / \(\(size_t\)E \* per \+ shared\);', run) == '30' and S.WS_FLOATS == 1 << 30
    assert 'R = std::max<size_t>(1, std::min<size_t>(R, (size_t)N));' in run and 'R = gemm_rows_hook(R, (size_t)N);' in run
    assert 'if (const char *rv = getenv("MILE_GEMM_ROWS")) R = std::max<size_t>(1, std::min<size_t>((size_t)atoll(rv), N));' in _body(hip, 'gemm_rows_hook')
    assert 'size_t per = n_a1 + n_p1 + (direct ? 0 : n_col2) + n_a2 + n_p2 + 120 + w_f2 + w_out;' in run
    assert 'if (grad) per += w_f2 + 120 + n_p2 + n_p1 + (direct ? 0 : n_a2 + n_a1);' in run
    assert 'const size_t w_f2 = mfma ? 88 : 84, w_out = mfma ? (size_t)(g.K + 7) / 8 * 8 : (size_t)g.K;' in run
    assert 'const unsigned nwg = (unsigned)((Rc + ipw - 1) / ipw);' in run and 'const int acc = chunk != 0;' in run
    assert 'const size_t nwg_max = (R + ipw - 1) / ipw;' in run
    assert _one(r'k_conv_reduce<<<dim3\((\d+), E\), 256, 0, st>>>\(part1, \(int\)nwg, KT1 \* 6, 6,', run) == str(S.REDUCE_GRID[1])
    assert _one(r'k_conv_reduce<<<dim3\((\d+), E\), 256, 0, st>>>\(part2, \(int\)nwg, 2400, 16,', run) == str(S.REDUCE_GRID[2])
    assert 'for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256)' in _body(f32, 'k_conv_reduce')
    b = _body(f32, 'k_conv5_dw')
    assert int(_one(r'constexpr int RG = (\d+);', b)) == S.RG
    assert 'const int K5 = 5 * CIN, G = nt / K5;' in b and 'nt = 256' in b and S.NT == 256
    assert 'for (int base = 1; base < G; base += RG)' in b and 'const int ng = min(RG, G - base);' in b
    assert 'const int b0 = blockIdx.x * ipw, b1 = min(R, b0 + ipw);' in b
    # evaluation: blocks of 256 samples
    b = _body(hip, 'loglik_lenet')
    assert f'for (int s0 = 0; s0 < S; s0 += {S.EVAL_BLOCK})' in b and f'std::min({S.EVAL_BLOCK}, S - s0)' in b


def test_known_shapes():
    """The figures tests/test_gpu_lenet_bf16x3.py states: its ni table, and test_launch_info's 57344."""
    assert S.ni_of(36, 36, 3) == (1, 1, 1) and S.ni_of(22, 22, 3) == (3, 4, 2) and S.ni_of(12, 12, 3) == (4, 4, 4)
    assert S.ni_of(28, 28, 3) == (2, 2, 1) and S.ni_of(32, 32, 3) == (1, 2, 1)
    assert 57344 // (3 * 12864) == 1 and 57344 // (3 * 5472) == 3 and ((36 + 4) ** 2 + 8) * 8 == 12864 and ((22 + 4) ** 2 + 8) * 8 == 5472
    assert max(S.cm_lds_dw(False, 8, 8, 0, 4, 3), S.cm_lds_dw2x(16, 16, 2, 3)) == 57344
    assert S.cm_lds_dw(False, 8, 8, 0, 4, 3) == max(3 * (4 * 72 * 16 + 64 * 32), 4 * 14 * 64 * 16)
    assert S.cm_lds_dw2x(16, 16, 2, 3) == max(3 * (408 * 8 + 128 * 32), 4 * 9 * 64 * 16)
    # terms = 1 keeps ni = 4 up to 38 pixels a side: lenet_bf16's ni < 4 needs the larger images of the table
    assert S.ni_of(38, 38, 1)[0] == 4 and S.ni_of(37, 41, 1) == (3, 4, 3) and S.ni_of(37, 54, 1) == (3, 3, 2)
    assert S.ni_of(37, 60, 1) == (2, 2, 2) and S.ni_of(37, 84, 1) == (1, 1, 1)
    # the thread map of k_conv5_dw: what the suite saw before (C = 1 .. 4) and what it did not
    assert [S.G_OF_C[c] for c in (1, 2, 3, 4)] == [51, 25, 17, 12]
    assert sorted(set(S.G_OF_C.values())) == [3, 4, 5, 6, 7, 8, 10, 12, 17, 25, 51]
    assert [S.dw_threads(c)['idle'] for c in range(1, 17)] == [1, 6, 1, 16, 6, 16, 11, 16, 31, 6, 36, 16, 61, 46, 31, 16]
    assert S.dw_threads(1) == dict(K5=5, G=51, idle=1, rounds=17, last_ng=2) and S.dw_threads(6) == dict(K5=30, G=8, idle=16, rounds=3, last_ng=1)
    assert [S.reduce_passes(1, c) for c in (1, 3, 4, 16)] == [1, 1, 2, 5] and S.reduce_passes(2, 1) == 1
    # the LDS bound of the direct form for one channel: between 73 and 74 pixels a side, from lds_w1
    assert S.backend(1, 73, 73) == (True, 'direct', 0) and S.backend(1, 74, 74) == (False, 'lds_w1', 0)
    assert S.lds_direct(1, 73, 73)['lds_w1'] == 151612 and S.lds_direct(1, 74, 74)['lds_w1'] == 155760
    assert S.backend(17, 12, 13)[:2] == (False, 'C > 16') and S.backend(3, 16, 20, True)[:2] == (False, 'env')
    assert S.backend(3, 32, 32)[2] == 1 and S.backend(1, 28, 28)[2] == 3
    # the walks the issue names
    w = S.walk(S.BY_NAME['f32-walk-20+17'])
    assert w == [(20, 3, 4, 0), (17, 3, 1, 1)]
    assert S.walk(S.BY_NAME['x3-walk-20+17']) == S.walk(S.BY_NAME['bf16-walk-20+17']) == [(20, 2, 4, 0), (17, 2, 1, 1)]
    assert S.walk(S.BY_NAME['x3-walk-4+4+3']) == [(4, 1, 4, 0), (4, 1, 4, 1), (3, 1, 3, 1)]
    assert S.walk(S.BY_NAME['f32-win-5+33-rows20']) == [(20, 3, 4, 0), (13, 2, 5, 1)]
    assert S.groups(16, 3) == [3, 3, 3, 3, 3, 1] and S.groups(5, 4) == [4, 1] and S.groups(12, 4) == [4, 4, 4]
    assert S.plan(S.BY_NAME['x3-k10'])['w_out'] == 16 and S.plan(S.BY_NAME['f32-k10'])['w_out'] == 10


def test_what_the_issue_names_is_in_the_table():
    f32 = [c for c in S.CASES if c.kernel == S.F32 and not c.gemm_env]
    assert {c.C for c in f32 if S.backend(c.C, c.H, c.W)[0]} >= set(range(1, 17))
    assert any((c.C, c.H, c.W) == (1, 73, 73) and c.N <= 2 and c.E == 1 for c in f32)
    assert any((c.C, c.H, c.W) == (1, 74, 74) and c.N <= 2 and c.E == 1 for c in f32) and any(c.C == 17 for c in f32)
    assert any((c.C, c.H, c.W) == (1, 28, 28) for c in f32) and any((c.C, c.H, c.W) == (3, 32, 32) for c in f32)
    for k in (S.F32, S.BF16, S.X3):
        mine = [c for c in S.CASES if c.kernel == k]
        assert any(c.chunk_rows == 20 and c.N == 37 and c.window is None for c in mine), k           # 20 + 17
        assert {c.act for c in mine} == set(S.ACTS) and {c.E for c in mine} >= {1, 2, 3}
        assert {(c.prior, c.wide) for c in mine} >= {('Normal', True), ('Normal', False), ('Laplace', False)}
        assert any(c.window for c in mine)
    for c in S.CASES:
        exception = (c.C, c.H, c.W) in ((1, 73, 73), (1, 74, 74), (1, 28, 28), (3, 32, 32)) or (c.kernel == S.BF16 and c.H == 37 and c.W > 37)
        assert c.N <= 40 and c.E <= 3 and (exception or (12 <= c.H <= 37 and 12 <= c.W <= 37)), c.name
    for c in S.WINDOW_CASES:
        assert S.base_of(c) in S.FULL_CASES and 0 < c.window[1] and c.window[0] + c.window[1] <= c.N


# ---- coverage ------------------------------------------------------------------------------------------------------------------------

def test_every_cell_gets_a_launch(capsys):
    hit = {}
    for c in S.CASES:
        for cell in S.cells_of(c):
            hit.setdefault(cell, []).append(c.name)
    assert set(hit) <= set(S.CELLS), sorted(set(hit) - set(S.CELLS), key=str)               # nothing runs outside the enumeration
    assert set(S.UNREACHABLE) <= set(S.CELLS) and not set(S.UNREACHABLE) & set(hit)
    missing = [cell for cell in S.CELLS if cell not in hit and cell not in S.UNREACHABLE]
    assert not missing, missing
    # the MFMA forms run nothing that they refuse, and refuse five channels by the restatement too
    for c in S.CASES:
        if c.kernel in S.MFMA:
            assert not S.plan(c)['refused'], c.name
    assert S.mfma_refused(5, 16, 16, 1) and S.mfma_refused(5, 16, 16, 3) and S.mfma_refused(1, 96, 96, 3) and not S.mfma_refused(4, 16, 16, 3)
    # k_conv5_dw always has idle threads: 5 C G = 256 has no solution
    assert all(S.dw_threads(c)['idle'] > 0 for c in range(1, 52))
    with capsys.disabled():
        fam = {}
        for cell in S.CELLS:
            fam[cell[0]] = fam.get(cell[0], 0) + 1
        print(f'\nLENETSCHED {len(S.CELLS)} cells, {len(S.UNREACHABLE)} unreachable, {len(S.CASES)} cases; per family: '
              + ', '.join(f'{k} {v}' for k, v in fam.items()))


def test_no_two_cases_are_the_same_launch():
    seen = {}
    for c in S.CASES:
        key = c[1:]
        assert key not in seen, (c.name, seen.get(key))
        seen[key] = c.name


# ---- the problems ------------------------------------------------------------------------------------------------------------------

def _distinct(cases):
    """One case per problem and rows: the kernel, E and the chunk rows do not change the oracle's answer."""
    seen, out = set(), []
    for c in cases:
        key = (S._key(c), c.window)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize('case', _distinct(S.CASES), ids=lambda c: c.name)
def test_every_leaf_sees_the_likelihood_and_no_unit_sits_on_the_kink(case):
    """likelihood_share >= 0.5 on every leaf of both chains (1.000 under the wide prior, 0.70 Normal, 0.56 Laplace), and every
    Dense pre-activation of a ReLU case farther than 5e-6 of its layer's largest from zero, in fp64, with no row masked.  A case
    whose seed is not 0 names the condition that seeds below it miss."""
    sh = S.shares(case)
    assert sh.min() >= S.SHARE, (case.name, sh.min(axis=0))
    if case.wide:
        assert sh.min() > 0.999, (case.name, sh.min())
    assert S.kink_margin(case) > S.KINK, (case.name, S.kink_margin(case))
    if case.seed:                                                 # a window has the seed of the set it is a window of
        assert case.act == 'relu' or not case.wide, case.name
        whole = S.base_of(case) if case.window else case
        assert whole.seed == case.seed
        for s in range(case.seed):
            lower = whole._replace(seed=s)
            assert S.kink_margin(lower) <= S.KINK or S.shares(lower).min() < S.SHARE, (case.name, s)


def test_problem_tiles_two_chains():
    case = S.BY_NAME['x3-walk-4+4+3']
    ospec, X, y, theta = S.problem(case)
    assert X.shape == (11, 2, 16, 20) and y.shape == (11,) and theta.shape == (3, ospec.n_params) and theta.dtype == np.float32
    assert np.array_equal(theta[2], theta[0]) and not np.array_equal(theta[0], theta[1])
    assert ospec.prior_scale == S.WIDE_PRIOR and S.ospec_of(S.BY_NAME['x3-laplace']).prior_scale == 0.7
    lp, g, g32 = S.reference_of(case)
    assert lp.shape == (2,) and g.shape == (2, ospec.n_params) and g32.dtype == np.float32 and not g.flags.writeable
    win = S.BY_NAME['f32-win-10+16']
    assert np.abs(S.reference_of(win)[1] - S.reference_of(S.base_of(win))[1]).max() > 0
    assert np.abs(S.reference_of(S.BY_NAME['bf16-windows'])[1] - S.reference_of(S.BY_NAME['x3-windows'])[1]).max() > 0    # the recipe


# ---- mutants -----------------------------------------------------------------------------------------------------------------------

MUTANT_KINDS = ('last-chunk-stored', 'short-group-last-image-dropped', 'last-short-workgroup-dropped', 'bias-one-workgroup-too-often',
                'crop-treated-as-present', 'window-one-image-late')
_SEEN = {}


def _mutant_cases():
    """One case per (problem, rows, walk, kernel class): E does not change the oracle's answer."""
    seen, out = set(), []
    for c in S.CASES:
        key = (S._key(c), c.window, c.chunk_rows, c.kernel, c.gemm_env)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def bounds_of(case, leaves):
    """The GPU test's per-leaf bound: nothing in it comes from a kernel."""
    _, g, g32 = S.reference_of(case)
    tol = BF16_LEAF_TOL if case.kernel == S.BF16 else L.LEAF_TOL
    return L.leaf_bounds(leaves, 2, g32=g32, g_ref=g, tol=tol, margin=L.F32_MARGIN)


@pytest.mark.parametrize('case', _mutant_cases(), ids=lambda c: c.name)
def test_a_wrong_schedule_misses_the_bound_tenfold(case):
    """Each mutant of the plain fp64 oracle misses the GPU test's per-leaf bound by 10x or more on a leaf it touches, in both
    chains, and the float32 evaluation of the case's own reference is inside the bound."""
    leaves = L.spec_leaves(S.ospec_of(case))
    names = [n for n, _, _ in leaves]
    _, g, g32 = S.reference_of(case)
    _, g64, _ = S.reference_of(case, 'f64')
    bound = bounds_of(case, leaves)
    L.assert_leaves(g32, g, leaves, bound, tag=(case.name, 'float32 restatement'))
    for name, (g_mut, touched) in S.schedule_mutants(case).items():
        cols = [names.index(t) for t in touched]
        ratio = (L.leaf_errors(g_mut, g64, leaves) / bound)[:, cols].max(axis=1)
        kind = next(k for k in MUTANT_KINDS if name.startswith(k))
        key = (kind, case.kernel == S.BF16)
        _SEEN[key] = min(_SEEN.get(key, np.inf), float(ratio.min()))
        assert ratio.min() >= 10.0, (case.name, name, ratio)
        with pytest.raises(AssertionError, match='leaf'):
            L.assert_leaves(g_mut, g64, leaves, bound, tag=name)


def test_every_kind_of_mutant_was_built(capsys):
    kinds = {}
    for c in _mutant_cases():
        if (c.C, c.H, c.W) in ((1, 73, 73), (1, 74, 74)):
            continue
        for name in S.schedule_mutants(c):
            kinds.setdefault(next(k for k in MUTANT_KINDS if name.startswith(k)), set()).add(S.backend_of(c))
    assert set(kinds) == set(MUTANT_KINDS)
    assert kinds['last-chunk-stored'] == set(S.BACKENDS) and kinds['crop-treated-as-present'] == set(S.BACKENDS)
    assert kinds['short-group-last-image-dropped'] == set(S.MFMA)
    for k in ('last-short-workgroup-dropped', 'bias-one-workgroup-too-often', 'window-one-image-late'):
        assert kinds[k] == {'f32-direct', S.BF16, S.X3}, k
    if _SEEN:
        with capsys.disabled():
            print('\nLENETSCHED least miss of the bound per mutant (f32 / x3 bound, bf16 bound): '
                  + ', '.join(f'{k[0]}{" [bf16]" if k[1] else ""} {v:.1f}x' for k, v in sorted(_SEEN.items())))

"""The table of tests/narrow_schedule.py has no holes, proven without a GPU: its 54 nets are the 31 + 23 instantiations the two
launchers list, no supported spec falls through a launcher, the restated schedule gives the launches the project records, every
form gets a workgroup in every cell of the row walk that exists for its class, every tabulated problem is off the ReLU kink with
every leaf's gradient the likelihood's, and a walk, a mask or a head that is wrong misses the per-leaf bound of
tests/test_gpu_narrow_schedule.py by more than 10x.

Smallest miss found, as a multiple of the bound (MUTANT_MISS below prints it per form with `pytest -s`): 11.0x, input row 15 of the
last layer's kernel zeroed on <3,2,1>, N = 130; the walk mutants miss by 200x at the least (the two-row last tile of
<5,1,1,partition>, N = 130), the head mutant by 5568x.
"""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest

from tests import leaf_cases as LC
from tests import leafcheck as L
from tests import narrow_schedule as W
from tests import partition_ref as PR

CSRC = Path(__file__).resolve().parents[1] / 'mile_amd' / 'csrc'
FORM_IDS = [W.form_id(f) for f in W.FORMS]
_MISS = {}


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    if _MISS:
        fid = min(_MISS, key=lambda k: _MISS[k][0])
        print(f'\nMUTANT_MISS smallest {_MISS[fid][0]:.1f}x: {fid} {_MISS[fid][1]}')


# ---- the dispatch, from the sources ---------------------------------------------------------------------------------------------

def _listed(path):
    return [tuple(int(x) for x in m) for m in re.findall(r'MILE_NRW\((\d+), (\d+), (\d+)\)', (CSRC / path).read_text())]


def _layout_constants(nh, th, tf):
    """NarrowLayout's own expressions, evaluated: every `static constexpr int` of the struct but the two with a conditional."""
    src = (CSRC / 'mile_grad_narrow.h').read_text()
    body = src[src.index('struct NarrowLayout {'):]
    body = body[:body.index('};')]
    env = {'NH': nh, 'TH': th, 'TF': tf, 'NRW_MAXW': W.NRW_MAXW, 'NRW_TS': W.NRW_TS}
    for line in body.splitlines():
        line = line.split('//')[0].strip()
        if not line.startswith('static constexpr int') or '?' in line or line.startswith('static constexpr int BYTES'):
            continue
        for decl in line[len('static constexpr int'):].rstrip(';').split(','):
            name, expr = decl.split('=')
            env[name.strip()] = eval(expr, {}, env)      # integer arithmetic on names defined above
    return env


def test_constants_and_both_lists_are_the_sources():
    src = (CSRC / 'mile_grad_narrow.h').read_text()
    assert int(re.search(r'#define NRW_MAXW (\d+)', src).group(1)) == W.NRW_MAXW
    assert int(re.search(r'#define NRW_TS (\d+)', src).group(1)) == W.NRW_TS
    full, part = _listed('mile_hip.hip'), _listed('mile_narrow_part.hip')
    assert len(full) == len(set(full)) == 31 and len(part) == len(set(part)) == 23
    assert sorted(full) == sorted(W.FULL_INSTANTIATIONS) and sorted(part) == sorted(W.PART_INSTANTIATIONS)
    assert [f.inst for f in W.FORMS if not f.part] == W.FULL_INSTANTIATIONS
    assert [f.inst for f in W.FORMS if f.part] == W.PART_INSTANTIATIONS
    assert len(W.FORMS) == len(set(FORM_IDS)) == 54
    # WL = TH >= 3 in both launchers, tf from F, nw = NRW_MAXW for the LDS form
    hip = (CSRC / 'mile_hip.hip').read_text()
    assert hip.count('constexpr bool WL = TH >= 3;') == 1 and (CSRC / 'mile_narrow_part.hip').read_text().count('constexpr bool WL = TH >= 3;') == 1
    assert 'tf = s->spec.in_features <= 16 ? 1 : 4;' in hip and 'const int nw = th >= 3 ? NRW_MAXW : narrow_waves(s, gp.S, gp.N);' in hip


@pytest.mark.parametrize('inst', W.FULL_INSTANTIATIONS, ids=lambda i: '%d.%d.%d' % i)
def test_restated_layout_is_the_struct(inst):
    nh, th, tf = inst
    env = _layout_constants(nh, th, tf)
    assert env['NACC'] == W.nacc(nh, th, tf)
    floats = env['TRANS'] + (max(env['WTOT'], env['RED']) if th >= 3 else env['RED'])
    assert 4 * floats == W.layout_bytes(nh, th, tf) <= 160 * 1024
    if th < 3:
        assert W.layout_bytes(nh, th, tf) <= 64 * 1024          # launched without raising the kernel's LDS limit


def test_every_supported_spec_has_an_instantiation_and_every_instantiation_a_spec():
    reached_full, reached_part = set(), set()
    for nh in range(1, 11):
        widths = (1, 15, 16, 17, 32, 33, 48, 64) if nh <= 3 else (1, 16)
        for hidden in itertools.product(widths, repeat=nh):
            for task, K in (('regr', 2), ('classification', 1), ('classification', 16)):
                ok = [F for F in range(1, 65) if W.supported(F, hidden + (K,), task)]
                assert ok == (list(range(1, 65 if nh <= 3 else 17)) if max(hidden) <= (64 if nh <= 3 else 16) else []), (hidden, task)
                for F in (ok[0], 16, 17, ok[-1]) if ok else ():
                    if F not in ok:
                        continue
                    inst = W.instantiation(F, hidden + (K,))
                    assert inst in W.FULL_INSTANTIATIONS, (F, hidden, inst)
                    reached_full.add(inst)
                    if nh >= 2:                          # (mile_set_partition leaves a net of one hidden layer in ordinary sampling)
                        assert inst in W.PART_INSTANTIATIONS, (F, hidden, inst)
                        reached_part.add(inst)
    assert reached_full == set(W.FULL_INSTANTIATIONS) and reached_part == set(W.PART_INSTANTIATIONS)
    # tf depends on F alone and th on the widest hidden layer alone: F in 1 .. 64 adds nothing to the four values above
    assert {W.instantiation(F, (16, 2))[2] for F in range(1, 17)} == {1} and {W.instantiation(F, (16, 2))[2] for F in range(17, 65)} == {4}
    for F, hs, task in ((65, (16, 2), 'regr'), (5, (65, 2), 'regr'), (5, (16,) * 4 + (17, 2), 'regr'), (17, (16,) * 4 + (2,), 'regr'),
                        (5, (16,) * 11 + (2,), 'regr'), (5, (16, 17), 'classification'), (5, (16, 3), 'regr'), (5, (0, 2), 'regr')):
        assert not W.supported(F, hs, task), (F, hs, task)


@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_form_is_its_instantiation(form):
    assert W.supported(form.F, form.hs, form.task) and W.instantiation(form.F, form.hs) == form.inst
    assert not form.part or len(form.hs) >= 3
    assert form.F in W.F_OF[form.inst[2]]
    assert len(set(form.hs[:-1])) == len(form.hs[:-1]) or len(form.hs) > 4 or len(form.hs) == 2 or form.inst == (3, 1, 4)
    assert form.hs[-1] == 2 if form.task == 'regr' else form.hs[-1] in W.K_OF


def test_forms_exercise_the_masks():
    for tf in (1, 4):
        assert {f.F for f in W.FORMS if f.inst[2] == tf} == set(W.F_OF[tf])
    assert W.F_OF == {1: (1, 5, 15, 16), 4: (17, 33, 60, 64)}
    assert {f.hs[-1] for f in W.FORMS if f.task == 'classification'} == {2, 5, 16}
    hidden = {w for f in W.FORMS for w in f.hs[:-1]}
    assert {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64} <= hidden
    want = {(3, 2, 1): (17, 9, 32), (3, 3, 1): (33, 48, 5), (3, 4, 1): (64, 49, 33)}
    for f in W.FORMS:
        if not f.part and f.inst in want:
            assert f.hs[:-1] == want[f.inst]
    for part in (False, True):
        for cls in ('reg', 'deep', 'lds'):
            mine = [f for f in W.FORMS if f.part == part and W.form_class(f.inst) == cls]
            assert {f.act for f in mine} == set(W.ACTS), (part, cls)
            assert {f.task for f in mine} == {'regr', 'classification'}, (part, cls)


# ---- the restated schedule --------------------------------------------------------------------------------------------------------

def test_restated_schedule_on_known_launches():
    """The launch tests/test_gpu_parity.py records for mfma_narrow_f32 (LAUNCH_SHAPES: (5, (48, 48, 2)) on 1052 rows, 12 particles)
    and the figures in the comment above narrow_S."""
    pytest.importorskip('torch')
    from tests.test_gpu_parity import LAUNCH_SHAPES
    name, grid, block, lds = LAUNCH_SHAPES['mfma_narrow_f32']
    inst = W.instantiation(5, (48, 48, 2))
    lch = W.launch(inst, 1052, 12)
    assert name == 'k_grad_narrow' and grid == (lch.S, 12) == (16, 12) and block == 64 * lch.nw == 256
    assert lds == W.layout_bytes(3, 4, 4) == max(W.layout_bytes(*i) for i in W.FULL_INSTANTIATIONS)
    stock = W.instantiation(5, (16, 16, 2))
    assert (W.launch(stock, 1052, 12).S, W.launch(stock, 1052, 12).nw) == (17, 4) and W.launch(stock, 1052, 128).S == 8
    # the upper bound shape_narrow reports for the register forms
    assert max(W.layout_bytes(*i) for i in W.FULL_INSTANTIATIONS if i[1] < 3) == max(W.layout_bytes(3, 2, 4), W.layout_bytes(10, 1, 1))
    # both branches' floors and caps
    assert W.splits(64, 300, 3) == 1 and W.splits(64, 300, 1) == 1 and W.splits(10 ** 6, 1, 1) == 64 and W.splits(10 ** 6, 1, 4) == 64
    assert W.splits(1052, 12, 1, n_cu=304) == 17 and W.splits(4096, 64, 3, n_cu=304) == 4
    for rows, S, nw in ((1052, 17, 4), (200, 4, 2), (7, 4, 1), (130, 3, 3), (100, 1, 4)):
        wk = W.walk(rows, S, nw)
        tiles = sorted(t for wg in wk for wv in wg for t in wv)
        assert [t[0] for t in tiles] == list(range(0, rows, 16)) and sum(t[1] for t in tiles) == rows      # every row once


def test_tables_state_what_the_schedule_gives():
    for cls, inst in (('reg', (2, 2, 1)), ('lds', (2, 3, 1))):
        for case in W.FULL_CASES[cls]:
            assert W.tile_counts(W.launch(inst, *case)) == W.FULL_TILES[cls][case], (cls, case)
        for win in W.WINDOW_CASES[cls]:
            assert W.tile_counts(W.launch(inst, W.WINDOW_N, W.WINDOW_E, win[1])) == W.WINDOW_TILES[cls][win], (cls, win)
            assert win[0] % 16 and win[1] > 0 and win[0] + win[1] <= W.WINDOW_N
        assert any(b + c == W.WINDOW_N for b, c in W.WINDOW_CASES[cls])
        assert max(N for N, _ in W.FULL_CASES[cls]) <= W.WINDOW_N
    assert W.launch((2, 1, 1), W.WINDOW_N, W.WINDOW_E).S == 4 and W.launch((2, 3, 1), W.WINDOW_N, W.WINDOW_E).S == 3
    # what the issue names, still there
    assert set(W.FULL_CASES['reg']) >= {(N, 2) for N in (1, 16, 31, 33, 64, 80, 130)} | {(200, 512), (150, 2048)}
    assert set(W.FULL_CASES['lds']) >= {(N, 2) for N in (1, 64, 100, 128)} | {(64, 300)}
    for cls in ('reg', 'lds'):
        assert set(W.WINDOW_CASES[cls]) >= {(13, 7), (13, 40), (45, 96), (177, 23)}


@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_form_reaches_every_cell(form):
    """Every cell of the form's class over its full-set cases, each also alone in a one-workgroup launch (but the register forms'
    idle wave, which needs a second workgroup); the workgroup without a tile is the windows' alone."""
    cls = W.walk_class(form)
    reached, alone = set(), set()
    for case in W.full_cases(form):
        lch = W.launch(form.inst, *case)
        assert W.tile_counts(lch) == W.FULL_TILES[cls][case]
        assert ('empty',) not in W.cells(lch)
        reached |= W.cells(lch)
        if lch.S == 1:
            alone |= W.cells(lch)
    assert reached >= set(W.CELLS[cls]) and alone >= set(W.CELLS_ALONE[cls]), (set(W.CELLS[cls]) - reached, set(W.CELLS_ALONE[cls]) - alone)
    if cls == 'reg':        # nw = min(4, tiles) at S = 1: no idle wave
        assert all(min(n) > 0 for N in range(1, 400) for n in W.tile_counts(W.launch(form.inst, N, 4096)))


@pytest.mark.parametrize('cls', ['reg', 'lds'])
def test_window_cases(cls):
    """Every window has a workgroup without a tile or a ragged last tile with the data's own rows behind it -- but (45, 96) at the
    LDS forms' S = 3, which (45, 90) stands in for -- and the class sees both."""
    inst = (2, 2, 1) if cls == 'reg' else (2, 3, 1)
    seen = set()
    for begin, count in W.WINDOW_CASES[cls]:
        lch = W.launch(inst, W.WINDOW_N, W.WINDOW_E, count)
        r0, valid = W.last_tile(lch)
        empty = ('empty',) in W.cells(lch)
        real_rows_behind = valid < 16 and begin + r0 + valid < W.WINDOW_N
        seen |= {'empty'} if empty else set()
        seen |= {'rows behind'} if real_rows_behind else set()
        assert empty or real_rows_behind or (cls, begin, count) == ('lds', 45, 96), (cls, begin, count)
    assert seen == {'empty', 'rows behind'}
    lch = W.launch(inst, W.WINDOW_N, W.WINDOW_E, 90)
    assert cls == 'reg' or (W.last_tile(lch) == (80, 10) and 45 + 90 < W.WINDOW_N)


# ---- the problems -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_restated_gradient_is_the_oracles(form):
    from oracle import mclmc_oracle as M
    N = 80 if W.walk_class(form) == 'reg' else 100
    prob, ospec = W.problem(form, N), W.ospec_of(form)
    assert ospec.prior_scale == LC.ATTN_PRIOR_SCALE
    for dtype in (np.float64, np.float32):
        lp, g, gl, gabs = W.evaluate(form, prob, np.arange(N), dtype)
        assert (gabs >= np.abs(gl) * (1 - 1e-5)).all()
        if form.part:
            lp_ref, g_ref = PR.logdensity_and_grad(ospec, prob['theta'], prob['X'][:N], prob['y'][:N])(prob['compact'].astype(dtype))
        else:
            lp_ref, g_ref = M.logpost_and_grad(ospec, prob['theta'].astype(dtype), prob['X'][:N], prob['y'][:N])
        assert lp.dtype == g.dtype == dtype and g.shape == g_ref.shape == (2, len(PR.index(ospec)) if form.part else ospec.n_params)
        assert np.array_equal(g, g_ref) and np.array_equal(lp, lp_ref)
    lp2, g2, _, g32, bound, _ = W.reference(form, N)
    assert np.array_equal(g2, W.evaluate(form, prob, np.arange(N))[1]) and bound.shape == (2, len(W.leaves_of(form)))
    # the zero rows behind the data add the head's term of a zero input, nothing to the first layer's kernel
    g_pad = W.evaluate(form, prob, np.arange(N + 3))[2]
    j, b, e = next((j, b, e) for j, (n, b, e) in enumerate(W.leaves_of(form)) if n == 'layer0.kernel')
    g_lik = W.evaluate(form, prob, np.arange(N))[2]
    assert np.abs(g_pad[:, b:e] - g_lik[:, b:e]).max() <= 1e-13 * np.abs(g_lik[:, b:e]).max() and np.abs(g_pad - g_lik).max() > 1e-6
    th = W.point(form, prob, 5)
    assert th.dtype == np.float32 and np.array_equal(th[4], th[0]) and np.array_equal(th[3], th[1]) and not np.array_equal(th[0], th[1])


@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_tabulated_problems_are_valid_and_the_check_can_see(form):
    """Per data set of the form, on the fp64 oracle: no hidden pre-activation within 3e-7 of the kink; every leaf of both chains
    has a likelihood share >= MIN_SHARE on the full set and on every window; the float32 oracle is inside the per-leaf bound and
    within 5e-6 of the whole gradient; no leaf's row sum cancels by more than CANCEL_MAX; and every mutant that applies -- a
    split's last tile dropped, the rows behind a ragged tile counted, a wave left out of the reduction, and on the cases of 64
    rows or more a kernel leaf's row or column 16 k - 1 or 16 k zeroed and a lane group's classes dropped from the softmax --
    misses that bound by more than 10x in both chains."""
    names = set()
    for N in W.data_sizes(form):
        kink, share, f32, whole32, cancel, miss, worst = W.audit(form, N)
        assert 0 <= W.seed_of(form, N) < W.SEED_TRIES and W.scale_of(form) in LC.THETA_LADDER
        assert kink == 0, (N, kink)
        assert share >= LC.MIN_SHARE, (N, share)
        assert f32 < 1.0, (N, f32)
        assert whole32 < W.WHOLE_F32, (N, whole32)
        assert cancel < W.CANCEL_MAX, (N, cancel)
        assert miss > W.MUTANT_FACTOR, (N, miss, worst)
        if W.form_id(form) not in _MISS or miss < _MISS[W.form_id(form)][0]:
            _MISS[W.form_id(form)] = (miss, worst)
        names |= {name for _, name in W.mutant_misses(form, N)}
    print(f'\nMUTANT_MISS {W.form_id(form):<18s} {_MISS[W.form_id(form)][0]:10.1f}x  {_MISS[W.form_id(form)][1]}')
    # every kind of mutant met the form somewhere
    assert {'last-tile-of-first-workgroup-dropped', 'last-tile-of-last-workgroup-dropped', 'trailing-rows-counted', 'wave-1-left-out',
            'last-busy-wave-left-out'} <= names
    widest = max(max(n_in, n_out) for _, n_in, n_out in W.kernel_leaves(form))       # (a partition form: the sampled leaves')
    assert any(n.endswith('-row-15-zeroed') or n.endswith('-column-15-zeroed') for n in names) == (widest >= 16)
    assert any('-16-zeroed' in n for n in names) == (widest >= 17)
    assert sum(n.startswith('classes-of-lane-group') for n in names) == (0 if form.task == 'regr' or form.hs[-1] <= 4 else (form.hs[-1] + 3) // 4)
    # labels in every lane group of the head
    if form.task == 'classification':
        y = W.problem(form, W.WINDOW_N)['y'][:W.WINDOW_N]
        assert {int(c) // 4 for c in y} == set(range((form.hs[-1] + 3) // 4))


def test_every_tabulated_entry_is_used():
    sizes = {(W.form_id(f), N) for f in W.FORMS for N in W.data_sizes(f)}
    assert set(W.SEEDS) <= sizes and set(W.SCALES) <= set(FORM_IDS)
    assert any(w == 1 for f in W.FORMS for w in f.hs[:-1])          # a one-unit layer somewhere

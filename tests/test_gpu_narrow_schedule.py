"""k_grad_narrow in every cell of its launch schedule (-m gpu): each of its 31 + 23 template instantiations (the partition forms of
mile_narrow_part.hip included) on one net of tests/narrow_schedule.py and on that table's cases, which put a workgroup into every
cell of the kernel's row walk (1..4 waves; a wave with no, one, several tiles; a last tile that is full, has 1 row or 15; under a row
window a workgroup without any tile and a ragged tile with the data's next rows behind it), against the fp64 oracle.
tests/test_narrow_schedule_host.py proves on the CPU that the table has no holes and that a wrong walk, mask or head misses the
per-leaf bound below by more than 10x.

One test per form, all its cases on one engine.  Every case first asserts that the launch is the tabulated one -- kernel name, grid
(S, E), block 64 nw, LDS at least the form's own -- so a case that has left its cell fails instead of testing another one.  Then,
particles 0 and 1 against the oracle: logp 2e-5 relative, the whole gradient 2e-5 of its largest entry, every leaf 5e-5 of its own
largest entry or 8x the float32 oracle's own error where that is larger (the figures of tests/test_gpu_parity.py and
tests/leafcheck.py; nothing is taken from the kernel).  Every other particle repeats particle 0's or 1's parameters and must repeat
its result bit for bit, a second launch must repeat the first bit for bit, the full set must return bit for bit after the windows,
and a window must equal the same rows installed as a full set: within the whole-gradient bound, and bit for bit where the restated
schedule gives both launches the same tiles per workgroup and wave.

Each test prints what it measured before it asserts (`pytest -s`, lines NRWSCHED) and the module one line per form at its end
(NRWFORM).  Measured on an MI355X, worst over all cases of the form; of the leaf's / the gradient's largest entry:

    form                             worst leaf  (float32 oracle)  whole gradient  logp      where the worst leaf was
    k_grad_narrow<1,1,1>             2.0e-06     2.3e-06           2.6e-07         5.0e-08   rows13+40 as a full set, tiles [[1, 1, 1]]
    k_grad_narrow<1,2,1>             1.1e-06     1.6e-06           2.5e-07         5.3e-08   rows13+40 as a full set, tiles [[1, 1, 1]]
    k_grad_narrow<1,1,4>             5.9e-07     9.1e-07           3.8e-07         4.5e-08   N200-E512 tiles [[2, 2, 2, 1], [2, 2, 1, 1]]
    k_grad_narrow<1,2,4>             4.3e-07     3.7e-07           3.0e-07         5.0e-08   rows45+96 as a full set, tiles [[1, 1, 1], [1, 1, 1]]
    k_grad_narrow<2,1,1>             8.5e-07     8.5e-07           5.2e-07         5.4e-08   N33-E2 tiles [[1, 1, 1]]
    k_grad_narrow<2,2,1>             7.2e-07     6.1e-07           2.0e-07         4.7e-08   N130-E2 tiles [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    k_grad_narrow<2,1,4>             5.1e-07     7.0e-07           4.1e-07         4.0e-08   N130-E2 tiles [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    k_grad_narrow<2,2,4>             9.9e-07     1.2e-06           2.9e-07         3.5e-08   N64-E2 tiles [[1, 1, 1, 1]]
    k_grad_narrow<3,1,1>             2.7e-06     1.7e-06           1.5e-06         3.7e-08   N64-E2 tiles [[1, 1, 1, 1]]
    k_grad_narrow<3,2,1>             8.5e-07     6.6e-07           6.7e-07         4.0e-08   rows13+40 as a full set, tiles [[1, 1, 1]]
    k_grad_narrow<3,1,4>             1.4e-06     6.9e-07           7.7e-07         3.2e-08   rows177+23 as a full set, tiles [[1, 1]]
    k_grad_narrow<3,2,4>             4.6e-07     6.3e-07           2.0e-07         5.7e-08   N64-E2 tiles [[1, 1, 1, 1]]
    k_grad_narrow<4,1,1>             7.4e-07     7.8e-07           6.5e-07         3.2e-08   N80-E2 tiles [[1, 1, 1], [1, 1, 0]]
    k_grad_narrow<5,1,1>             9.1e-06     4.3e-06           3.6e-06         3.6e-08   N130-E2 tiles [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    k_grad_narrow<6,1,1>             5.3e-07     7.8e-07           2.3e-07         5.7e-08   N1-E2 tiles [[1]]
    k_grad_narrow<7,1,1>             1.3e-06     7.3e-07           7.3e-07         4.1e-08   rows13+40 as a full set, tiles [[1, 1, 1]]
    k_grad_narrow<8,1,1>             1.2e-06     1.5e-06           6.1e-07         3.5e-08   rows45+96 as a full set, tiles [[1, 1, 1], [1, 1, 1]]
    k_grad_narrow<9,1,1>             2.3e-06     1.5e-06           2.1e-07         3.0e-08   N150-E2048 tiles [[3, 3, 2, 2]]
    k_grad_narrow<10,1,1>            1.9e-06     2.2e-06           6.9e-07         3.4e-08   N31-E2 tiles [[1, 1]]
    k_grad_narrow<1,3,1>             4.2e-07     4.6e-07           2.5e-07         5.6e-08   N128-E2 tiles [[1, 1, 1, 1], [1, 1, 1, 1]]
    k_grad_narrow<1,4,1>             1.0e-06     1.3e-06           2.3e-07         3.5e-08   rows13+40 as a full set, tiles [[1, 1, 1, 0]]
    k_grad_narrow<1,3,4>             4.7e-07     7.9e-07           4.5e-07         3.1e-08   rows13+40 as a full set, tiles [[1, 1, 1, 0]]
    k_grad_narrow<1,4,4>             3.0e-07     4.4e-07           3.0e-07         5.5e-08   N31-E2 tiles [[1, 1, 0, 0]]
    k_grad_narrow<2,3,1>             3.7e-07     5.9e-07           2.4e-07         5.0e-08   rows177+23 as a full set, tiles [[1, 1, 0, 0]]
    k_grad_narrow<2,4,1>             3.4e-07     5.7e-07           1.8e-07         2.9e-08   N128-E2 tiles [[1, 1, 1, 1], [1, 1, 1, 1]]
    k_grad_narrow<2,3,4>             5.0e-07     5.3e-07           4.2e-07         5.0e-08   rows177+23 as a full set, tiles [[1, 1, 0, 0]]
    k_grad_narrow<2,4,4>             1.4e-06     1.6e-06           3.1e-07         3.8e-08   rows13+40 as a full set, tiles [[1, 1, 1, 0]]
    k_grad_narrow<3,3,1>             1.1e-06     1.2e-06           2.9e-07         5.9e-08   N100-E2 tiles [[2, 2, 2, 1]]
    k_grad_narrow<3,4,1>             5.9e-07     5.8e-07           5.9e-07         3.8e-08   N128-E2 tiles [[1, 1, 1, 1], [1, 1, 1, 1]]
    k_grad_narrow<3,3,4>             1.4e-06     1.4e-06           5.0e-07         5.4e-08   N128-E2 tiles [[1, 1, 1, 1], [1, 1, 1, 1]]
    k_grad_narrow<3,4,4>             5.4e-07     5.3e-07           2.4e-07         4.1e-08   N64-E300 tiles [[1, 1, 1, 1]]
    k_grad_narrow<2,1,1,partition>   6.0e-07     4.0e-07           4.0e-07         4.1e-08   rows13+40 as a full set, tiles [[1, 1, 1]]
    k_grad_narrow<2,2,1,partition>   7.0e-07     1.6e-06           4.8e-07         4.9e-08   N33-E2 tiles [[1, 1, 1]]
    k_grad_narrow<2,1,4,partition>   3.4e-07     4.4e-07           2.7e-07         4.1e-08   N16-E2 tiles [[1]]
    k_grad_narrow<2,2,4,partition>   4.4e-07     6.1e-07           3.6e-07         3.0e-08   N64-E2 tiles [[1, 1, 1, 1]]
    k_grad_narrow<3,1,1,partition>   2.8e-06     3.4e-06           1.9e-06         5.1e-08   N64-E2 tiles [[1, 1, 1, 1]]
    k_grad_narrow<3,2,1,partition>   3.8e-07     8.4e-07           3.8e-07         4.0e-08   rows45+96 as a full set, tiles [[1, 1, 1], [1, 1, 1]]
    k_grad_narrow<3,1,4,partition>   9.5e-07     8.2e-07           7.5e-07         5.4e-08   N150-E2048 tiles [[3, 3, 2, 2]]
    k_grad_narrow<3,2,4,partition>   4.5e-07     6.5e-07           3.6e-07         4.0e-08   N16-E2 tiles [[1]]
    k_grad_narrow<4,1,1,partition>   3.4e-07     5.1e-07           1.7e-07         4.0e-08   N31-E2 tiles [[1, 1]]
    k_grad_narrow<5,1,1,partition>   2.4e-06     2.7e-06           1.2e-06         5.2e-08   N64-E2 tiles [[1, 1, 1, 1]]
    k_grad_narrow<6,1,1,partition>   1.8e-06     7.5e-07           1.1e-06         4.9e-08   N130-E2 tiles [[1, 1, 1], [1, 1, 1], [1, 1, 1]]
    k_grad_narrow<7,1,1,partition>   1.1e-06     2.9e-06           5.0e-07         5.5e-08   N31-E2 tiles [[1, 1]]
    k_grad_narrow<8,1,1,partition>   8.0e-07     3.0e-06           1.8e-07         4.0e-08   rows13+7 as a full set, tiles [[1]]
    k_grad_narrow<9,1,1,partition>   1.2e-06     9.9e-07           3.2e-07         5.1e-08   rows13+7 as a full set, tiles [[1]]
    k_grad_narrow<10,1,1,partition>  5.5e-07     5.1e-07           2.3e-07         5.7e-08   N16-E2 tiles [[1]]
    k_grad_narrow<2,3,1,partition>   6.8e-06     4.2e-06           2.0e-06         4.7e-08   N200-E2 tiles [[2, 1, 1, 1], [2, 1, 1, 1], [1, 1, 1, 0]]
    k_grad_narrow<2,4,1,partition>   6.8e-07     5.6e-07           3.5e-07         3.4e-08   rows177+23 as a full set, tiles [[1, 1, 0, 0]]
    k_grad_narrow<2,3,4,partition>   7.3e-07     4.0e-07           6.2e-07         3.4e-08   rows45+90 as a full set, tiles [[2, 2, 1, 1]]
    k_grad_narrow<2,4,4,partition>   8.4e-07     6.5e-07           7.0e-07         3.1e-08   N100-E2 tiles [[2, 2, 2, 1]]
    k_grad_narrow<3,3,1,partition>   6.7e-07     5.2e-07           2.0e-07         4.7e-08   N100-E2 tiles [[2, 2, 2, 1]]
    k_grad_narrow<3,4,1,partition>   1.4e-06     2.5e-06           9.0e-07         4.3e-08   rows177+23 as a full set, tiles [[1, 1, 0, 0]]
    k_grad_narrow<3,3,4,partition>   1.6e-06     1.5e-06           9.8e-07         5.3e-08   N128-E2 tiles [[1, 1, 1, 1], [1, 1, 1, 1]]
    k_grad_narrow<3,4,4,partition>   4.4e-07     5.2e-07           2.5e-07         4.9e-08   rows13+7 as a full set, tiles [[1, 0, 0, 0]]
    bound                            5e-05 (the 8x float32 term never exceeded it)  2e-05      2e-05

No replica differed from its chain anywhere (E = 300, 512, 2048 included) and no second launch from the first.  A window's result
equalled that of the same rows installed as a full set bit for bit wherever both launches walk the same tiles per workgroup and wave
(rows 13+7 of every form: one tile in workgroup 0, three or two workgroups without any), so a workgroup without a tile adds exactly
nothing; of the other 182 comparisons 106 were bit-identical too, the rest differ by summation order, 2.3e-07 of the largest entry
at most.  The table found no wrong gradient in any of the 54 instantiations and no kernel source changed.

What its first run did find was in the problems: the net with a one-unit first layer (<3,1,1,partition>) had, for two of its
data sets, a first-layer bias gradient that is a sum over the rows cancelling to 1e-4 of its terms; the kernel's 2.2e-4 of that
leaf was rounding of the sum (1.7e-9 absolute) while the float32 oracle happened to land closer.  tests/narrow_schedule.py now
asks of every tabulated problem, on the fp64 oracle, that no leaf cancels by more than 209x and that the float32 oracle stays within
5e-6 of the whole gradient (CANCEL_MAX, WHOLE_F32); no bound here moved.
"""
import numpy as np
import pytest

from tests import leafcheck as L
from tests import narrow_schedule as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
KERNEL = 'mfma_narrow_f32'
LP_TOL = 2e-5            # relative, test_logpost_grad_matches_oracle
WHOLE_TOL = 2e-5         # of the gradient's largest entry, test_logpost_grad_matches_oracle
FORM_IDS = [W.form_id(f) for f in W.FORMS]
_WORST = {}              # form id -> [leaf, float32 oracle's leaf, whole gradient, logp, where the worst leaf was, bit-identical windows]


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    for form in W.FORMS:
        fid = W.form_id(form)
        if fid in _WORST:
            leaf, leaf32, whole, lp, where, same = _WORST[fid]
            print(f'\nNRWFORM {W.form_name(form):<32s} leaf {leaf:.1e} (float32 oracle {leaf32:.1e})  whole {whole:.1e}  logp {lp:.1e}  '
                  f'windows bit-identical to their rows as a full set {same}  worst leaf in {where}')


def _spec(form):
    from mile_amd import ModelSpec
    return ModelSpec(in_features=form.F, hidden_structure=form.hs, activation=form.act, task=form.task, prior='Normal', prior_loc=0.0,
                     prior_scale=W.PRIOR_SCALE)


def _install(eng, form, prob, rows, E):
    """The rows `rows` of the problem as the engine's full data set (a new engine for the first), the frozen rows of E particles."""
    from mile_amd.engine import Engine
    X, y = torch.from_numpy(np.ascontiguousarray(prob['X'][rows])), torch.from_numpy(np.ascontiguousarray(prob['y'][rows]))
    if eng is None:
        eng = Engine(_spec(form), X, y, device=DEV, grad_kernel=KERNEL)
    else:
        eng.set_data(X, y)
    if form.part:
        eng.set_partition(torch.from_numpy(W.frozen(prob, E)))
    assert eng.grad_kernel == KERNEL
    return eng


def _launch(eng, theta):
    lp, g = eng.logpost_grad(torch.from_numpy(theta))
    torch.cuda.synchronize()
    return lp, g


def _assert_cell(eng, form, lch, E, tiles, windowed=False):
    info = eng.grad_launch_info(E)
    assert info['kernel'] == ('k_grad_narrow<partition>' if form.part else 'k_grad_narrow'), info
    assert info['grid'] == (lch.S, E), (W.form_id(form), info, lch.S)
    if not windowed:        # (under a window the launch info still describes the full set: shape_narrow reads s->N)
        assert info['block'] == 64 * lch.nw, (W.form_id(form), info, lch.nw)
    assert info['lds_bytes'] >= W.layout_bytes(*form.inst), info     # an upper bound over the instantiations
    assert W.tile_counts(lch) == tiles, (W.form_id(form), W.tile_counts(lch), tiles)


def _check(form, where, lp, g, ref):
    """The three bounds on particles 0 and 1 (CPU tensors); notes the figures."""
    fid, leaves = W.form_id(form), W.leaves_of(form)
    lp_ref, g_ref, _, g32, bound, _ = ref
    lp, g = lp.numpy().astype(np.float64), g.numpy().astype(np.float64)
    e_lp = np.abs(lp - lp_ref).max() / np.abs(lp_ref).max()
    e_whole = np.abs(g - g_ref).max(axis=1) / np.abs(g_ref).max(axis=1)
    err, err32 = L.leaf_errors(g, g_ref, leaves), L.leaf_errors(g32, g_ref, leaves)
    print(f'\nNRWSCHED {fid} {where}: logp {e_lp:.2e}  whole {e_whole.max():.2e}  worst leaf {err.max():.2e} '
          f'(float32 oracle {err32.max():.2e}, bound {bound.min():.2e}..{bound.max():.2e})')
    w = _WORST.setdefault(fid, [0.0, 0.0, 0.0, 0.0, None, ''])
    if err.max() >= w[0]:
        w[0], w[4] = float(err.max()), where
    w[1], w[2], w[3] = max(w[1], float(err32.max())), max(w[2], float(e_whole.max())), max(w[3], float(e_lp))
    assert np.isfinite(lp).all() and np.isfinite(g).all(), (fid, where)
    assert e_lp < LP_TOL, (fid, where, e_lp)
    assert e_whole.max() < WHOLE_TOL, (fid, where, e_whole)
    L.assert_leaves(g, g_ref, leaves, bound, tag=(fid, where))


def _run(eng, form, where, theta, ref):
    """Two launches: the first against the oracle, every replica against its chain, the second against the first."""
    lp, g = _launch(eng, theta)
    _check(form, where, lp[:2].cpu(), g[:2].cpu(), ref)
    chain = torch.arange(theta.shape[0], device=g.device) % 2
    differ = torch.nonzero((g != g[chain]).any(dim=1) | (lp != lp[chain])).flatten().tolist()
    assert not differ, (W.form_id(form), where, 'particles that differ from their chain', differ[:8])
    lp2, g2 = _launch(eng, theta)
    assert torch.equal(lp2, lp) and torch.equal(g2, g), (W.form_id(form), where, 'a second launch differs')
    return lp[:2].cpu(), g[:2].cpu()


@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_form_in_every_cell(form):
    fid, cls = W.form_id(form), W.walk_class(form)
    eng = None
    # ---- the full data sets ----
    for case in W.full_cases(form):
        N, E = case
        prob = W.problem(form, N)
        eng = _install(eng, form, prob, slice(0, N), E)
        lch = W.launch(form.inst, N, E)
        _assert_cell(eng, form, lch, E, W.FULL_TILES[cls][case])
        _run(eng, form, f'{W.case_id(case)} tiles {W.tile_counts(lch)}', W.point(form, prob, E), W.reference(form, N))
    # ---- row windows on N = 200 ----
    N, E = W.WINDOW_N, W.WINDOW_E
    prob = W.problem(form, N)
    theta = W.point(form, prob, E)
    eng = _install(eng, form, prob, slice(0, N), E)
    lch = W.launch(form.inst, N, E)
    _assert_cell(eng, form, lch, E, W.tile_counts(lch))
    full = _run(eng, form, f'{W.case_id((N, E))} tiles {W.tile_counts(lch)}', theta, W.reference(form, N))
    windowed = {}
    for win in W.window_cases(form):
        begin, count = win
        eng.set_row_window(begin, count)
        lw = W.launch(form.inst, N, E, count)
        _assert_cell(eng, form, lw, E, W.WINDOW_TILES[cls][win], windowed=True)
        windowed[win] = _run(eng, form, f'{W.window_id(win)} tiles {W.tile_counts(lw)}', theta, W.reference(form, N, begin, count))
    eng.set_row_window(0, 0)
    lp, g = _launch(eng, theta)
    assert torch.equal(lp.cpu(), full[0]) and torch.equal(g.cpu(), full[1]), (fid, 'the full set after the windows')
    # ---- the windows' rows as full data sets ----
    same = []
    for win in W.window_cases(form):
        begin, count = win
        eng = _install(eng, form, prob, slice(begin, begin + count), E)
        lw, lf = W.launch(form.inst, N, E, count), W.launch(form.inst, count, E)
        _assert_cell(eng, form, lf, E, W.tile_counts(lf))
        ref = W.reference(form, N, begin, count)
        lp2, g2 = _run(eng, form, f'{W.window_id(win)} as a full set, tiles {W.tile_counts(lf)}', theta, ref)
        lp1, g1 = windowed[win]
        d_lp = np.abs(lp1.numpy().astype(np.float64) - lp2.numpy()).max() / np.abs(ref[0]).max()
        d_g = np.abs(g1.numpy().astype(np.float64) - g2.numpy()).max(axis=1) / np.abs(ref[1]).max(axis=1)
        identical = torch.equal(lp1, lp2) and torch.equal(g1, g2)
        same_walk = lw.nw == lf.nw and [wg for wg in lw.walk if any(wg)] == lf.walk
        print(f'NRWSCHED {fid} {W.window_id(win)}: window against full set of the same rows: logp {d_lp:.2e} whole {d_g.max():.2e} '
              f'bit-identical {identical} (same walk {same_walk})')
        same.append(f'{int(identical)}/{int(same_walk)}')
        assert d_lp < LP_TOL and d_g.max() < WHOLE_TOL, (fid, win, d_lp, d_g)
        if same_walk:       # the workgroups without a tile add exactly nothing
            assert identical, (fid, win, 'same tiles per workgroup and wave, different bits')
    _WORST[fid][5] = ' '.join(same)

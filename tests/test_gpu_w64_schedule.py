"""k_grad_w64 over every row-block schedule (-m gpu): each of its ten template forms on the cases of tests/w64_schedule.py, which
put a workgroup into every cell (main-loop rounds 0 / 1 / 2+, leftover blocks 0..3) of the kernel's row walk, against the fp64
oracle.  tests/test_w64_schedule_host.py proves on the CPU that the table has no holes and that a walk one block off misses the
per-leaf bound below by more than 10x.

Every test first asserts that the launch has the grid, and so the blocks per workgroup, its case is tabulated with: a case that
has left its cell fails instead of testing another one.  Then, particles 0 and 1 against the oracle: logp 2e-5 relative, the whole
gradient 2e-5 of its largest entry, every leaf 5e-5 of its own largest entry or 8x the float32 oracle's own error where that is
larger (the figures of tests/test_gpu_parity.py and tests/test_gpu_leaf_parity.py; nothing is taken from the kernel).  Every
other particle repeats particle 0's or 1's parameters and must repeat its result bit for bit.  A split-bf16 form may be no worse
than twice the fp32 form on the same case, + 1e-7 (test_split_bf16_w64_kernel_is_fp32_faithful's relation).  Row windows put a
workgroup without any block next to one with 1..5 blocks that does not begin at block 0.

Each test prints what it measured before it asserts (`pytest -s`, lines W64SCHED), and the module prints one line per form at its
end (W64FORM).  Measured on an MI355X, worst over all cells of the form; of the leaf's / the gradient's largest entry:

    form            worst leaf  (float32 oracle)  whole gradient  logp      where the worst leaf was
    NH1-F5-fp32     1.2e-06     1.5e-06           1.6e-07         7.1e-08   N416-E128, blocks [6, 7]
    NH1-F12-fp32    3.4e-07     1.4e-06           2.5e-07         7.6e-08   N351-E128, blocks [5, 6]
    NH2-F5-fp32     6.8e-07     9.4e-07           3.1e-07         5.4e-08   window rows 13+96, blocks [1, 2]
    NH2-F5-split    9.9e-07     9.4e-07           4.5e-07         5.4e-08   window rows 13+96, blocks [1, 2]
    NH2-F12-fp32    4.5e-07     1.1e-06           3.0e-07         5.0e-08   N59-E2, blocks [2]
    NH2-F12-split   5.4e-07     1.1e-06           4.6e-07         5.0e-08   N315-E130, blocks [10]
    NH3-F5-fp32     5.0e-07     1.1e-06           4.1e-07         5.4e-08   N123-E2, blocks [4]
    NH3-F5-split    4.4e-07     1.1e-06           3.4e-07         5.4e-08   N59-E2, blocks [2]
    NH3-F16-fp32    2.7e-06     5.4e-06           9.1e-07         5.3e-08   N123-E2, blocks [4]
    NH3-F16-split   1.7e-06     5.4e-06           6.6e-07         5.3e-08   N123-E2, blocks [4]
    bound           5e-05 (the 8x float32 term never exceeded it)  2e-05   2e-05

No replica differed from its chain anywhere.  A window's result equalled that of the same rows installed as a full set bit for bit
wherever both launches walk the same blocks per workgroup ([0, 1] against [1], [4, 5] against [4, 5]: 30 of 60), so the empty
workgroup's slab adds exactly nothing; elsewhere the two differ by summation order, 4.1e-07 of the largest entry at most.  The split
forms sit closest to their relation at NH3-F16, N225-E2: 3.12e-07 against 2 x 1.06e-07 + 1e-7.

What this table found when it first ran: the NH = 3, F 9..16 fp32 form (never run by the suite before) returned a wrong gradient
from every workgroup with three leftover blocks -- whole gradient off by 2e-2 .. 1.9e-1, a leaf by up to 8.5e-1, logp right, all
other cells of that form within 2.8e-06 -- in 11 tests: N = 91, 193, 219, 347, 416, 477, 855, windows [1, 2] (as a full set of
three blocks), [2, 3], [3, 4].  It is the one fp32 form whose registers spill; the three-block round sat behind a branch on the
per-lane wave index.  mile_grad_w64.h now takes that branch on the wave index as a scalar for this form.
"""
from functools import lru_cache

import numpy as np
import pytest

from tests import leafcheck as L
from tests import w64_schedule as W

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

DEV = 'cuda:0'
LP_TOL = 2e-5            # relative, test_logpost_grad_matches_oracle
WHOLE_TOL = 2e-5         # of the gradient's largest entry, test_logpost_grad_matches_oracle
FORM_IDS = [W.form_id(f) for f in W.FORMS]
_WORST = {}              # form id -> [leaf, float32 oracle's leaf, whole gradient, logp, where the worst leaf was]


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    for fid in FORM_IDS:
        if fid in _WORST:
            leaf, leaf32, whole, lp, where = _WORST[fid]
            print(f'\nW64FORM {fid:<14s} leaf {leaf:.1e} (float32 oracle {leaf32:.1e})  whole {whole:.1e}  logp {lp:.1e}  worst leaf in {where}')


def _engine(form, X, y):
    from mile_amd import ModelSpec
    from mile_amd.engine import Engine
    F, hs, kernel = form
    eng = Engine(ModelSpec(in_features=F, hidden_structure=hs), torch.from_numpy(X), torch.from_numpy(y), device=DEV, grad_kernel=kernel)
    assert eng.grad_kernel == kernel
    return eng


def _launch(eng, theta):
    lp, g = eng.logpost_grad(torch.from_numpy(theta))
    torch.cuda.synchronize()
    return lp.cpu(), g.cpu()


def _bound(leaves, g_ref, g32):
    return L.leaf_bounds(leaves, 2, g32=g32, g_ref=g_ref, tol=L.LEAF_TOL, margin=L.F32_MARGIN)


def _measure(lp, g, ref):
    """(logp error, per-particle whole-gradient error [2]) of two particles against the oracle."""
    lp_ref, g_ref, _ = ref
    lp, g = np.asarray(lp, np.float64), np.asarray(g, np.float64)
    e_lp = np.abs(lp - lp_ref).max() / np.abs(lp_ref).max()
    e_whole = np.abs(g - g_ref).max(axis=1) / np.abs(g_ref).max(axis=1)
    return e_lp, e_whole


def _note(fid, where, e_lp, e_whole, err, err32):
    w = _WORST.setdefault(fid, [0.0, 0.0, 0.0, 0.0, None])
    if err.max() > w[0]:
        w[0], w[4] = float(err.max()), where
    w[1], w[2], w[3] = max(w[1], float(err32.max())), max(w[2], float(e_whole.max())), max(w[3], float(e_lp))


def _check(fid, where, lp, g, ref, leaves):
    """The three bounds on two particles; returns the per-particle whole-gradient error."""
    lp_ref, g_ref, g32 = ref
    bound = _bound(leaves, g_ref, g32)
    g = np.asarray(g, np.float64)
    e_lp, e_whole = _measure(lp, g, ref)
    err, err32 = L.leaf_errors(g, g_ref, leaves), L.leaf_errors(g32, g_ref, leaves)
    print(f'\nW64SCHED {fid} {where}: logp {e_lp:.2e}  whole {e_whole.max():.2e}  worst leaf {err.max():.2e} '
          f'(float32 oracle {err32.max():.2e}, bound {bound.min():.2e}..{bound.max():.2e})')
    _note(fid, where, e_lp, e_whole, err, err32)
    assert np.isfinite(np.asarray(lp)).all() and np.isfinite(g).all(), (fid, where)
    assert e_lp < LP_TOL, (fid, where, e_lp)
    assert e_whole.max() < WHOLE_TOL, (fid, where, e_whole)
    L.assert_leaves(g, g_ref, leaves, bound, tag=(fid, where))
    return e_whole


# ---- the full data set ----------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _run(form, case):
    """One launch of `form` on `case`: the launch shape, particles 0 and 1, and which of the other particles do not repeat their
    chain bit for bit.  Kept for the split form's comparison with the fp32 form."""
    N, E = case
    seed = W.seed_of(form, N)
    _, X, y, theta = W.problem(form, N, E, seed)
    eng = _engine(form, X, y)
    info = eng.grad_launch_info(E)
    lp, g = _launch(eng, theta)
    differ = [e for e in range(2, E) if not (torch.equal(lp[e], lp[e % 2]) and torch.equal(g[e], g[e % 2]))]
    return {'kernel': info['kernel'], 'grid': info['grid'], 'lp': lp[:2].numpy().copy(), 'g': g[:2].numpy().copy(), 'differ': differ,
            'seed': seed}


def _where(case, blocks):
    return f'{W.case_id(case)} blocks {blocks} cells {[W.cell(n) for n in blocks]}'


@pytest.mark.parametrize('case', W.FULL_CASES, ids=[W.case_id(c) for c in W.FULL_CASES])
@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_every_cell_of_the_row_walk(form, case):
    N, E = case
    fid, net = W.form_id(form), (form[0], form[1])
    r = _run(form, case)
    # the cell: the launch is the one the table was made for
    assert r['kernel'] == 'k_grad_w64' and r['grid'] == (W.splits(N, E), E), (fid, case, r['kernel'], r['grid'])
    blocks = W.blocks(N, r['grid'][0])
    assert blocks == W.FULL_BLOCKS[case], (fid, case, blocks)
    where = _where(case, blocks)
    # the oracle
    ref = W.reference(net, N, r['seed'])
    leaves = L.fcn_leaves(W.ospec_of(net))
    e_whole = _check(fid, where, r['lp'], r['g'], ref, leaves)
    # replicas: one schedule for all particles of a launch, a fixed reduction order
    assert not r['differ'], (fid, where, 'particles that differ from their chain', r['differ'][:8])
    # the split form against the fp32 form on the same case
    if form[2] == 'mfma_w64_bf16x3':
        r32 = _run(W.fp32_form(form), case)
        assert r32['grid'] == r['grid'] and r32['seed'] == r['seed']
        e32 = _measure(r32['lp'], r32['g'], ref)[1]
        print(f'W64SCHED {fid} {where}: worst particle split {e_whole.max():.2e}  fp32 form {e32.max():.2e}')
        assert e_whole.max() <= 2.0 * e32.max() + 1e-7, (fid, where, e_whole.max(), e32.max())


# ---- row windows ----------------------------------------------------------------------------------------------------------------

def _window_problem(form):
    _, X, y, theta = W.problem(form, W.WINDOW_N, W.WINDOW_E, W.seed_of(form, W.WINDOW_N))
    return X, y, theta


@pytest.mark.parametrize('win', W.WINDOW_CASES, ids=[W.window_id(w) for w in W.WINDOW_CASES])
@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_row_window_cells(form, win):
    """A window keeps the full set's two workgroups: [0, 1] .. [4, 5] blocks, the second workgroup beginning at block 0..4 of rows
    that begin at row 13 or 45 of the data; the ragged block's padding then reads real rows, which only the head's mask removes.
    Against the oracle on those rows, against the same rows as a full data set on a second engine (one workgroup, or [4, 5] again:
    the empty workgroup's slab adds nothing), and the full set's result returns bit for bit."""
    begin, count = win
    fid, net = W.form_id(form), (form[0], form[1])
    N, E = W.WINDOW_N, W.WINDOW_E
    X, y, theta = _window_problem(form)
    eng = _engine(form, X, y)
    S = W.splits(N, E)
    assert eng.grad_launch_info(E)['grid'] == (S, E) and S == 2, fid
    blocks = W.blocks(count, S)
    assert blocks == W.WINDOW_BLOCKS[win]
    where = f'{W.window_id(win)} blocks {blocks} first blocks {W.first_blocks(count, S)}'
    leaves = L.fcn_leaves(W.ospec_of(net))
    seed = W.seed_of(form, N)
    full = _launch(eng, theta)
    _check(fid, f'N{N}-E{E} full set', full[0].numpy(), full[1].numpy(), W.reference(net, N, seed), leaves)
    eng.set_row_window(begin, count)
    assert eng.grad_launch_info(E)['grid'] == (S, E)                 # S is the full set's under a window
    lp, g = _launch(eng, theta)
    ref = W.reference(net, N, seed, begin, count)
    _check(fid, where, lp.numpy(), g.numpy(), ref, leaves)
    # the same rows as a full data set
    rows = slice(begin, begin + count)
    eng2 = _engine(form, np.ascontiguousarray(X[rows]), np.ascontiguousarray(y[rows]))
    assert eng2.grad_launch_info(E)['grid'] == (W.splits(count, E), E)
    lp2, g2 = _launch(eng2, theta)
    _check(fid, where + ' as a full set', lp2.numpy(), g2.numpy(), ref, leaves)
    lp_ref, g_ref, g32 = ref
    d_lp = np.abs(lp.numpy().astype(np.float64) - lp2.numpy()).max() / np.abs(lp_ref).max()
    d_g = np.abs(g.numpy().astype(np.float64) - g2.numpy()).max(axis=1) / np.abs(g_ref).max(axis=1)
    print(f'W64SCHED {fid} {where}: window against full set of the same rows: logp {d_lp:.2e} whole {d_g.max():.2e} '
          f'bit-identical {torch.equal(g, g2) and torch.equal(lp, lp2)}')
    assert d_lp < LP_TOL and d_g.max() < WHOLE_TOL, (fid, where, d_lp, d_g)
    L.assert_leaves(g.numpy(), g2.numpy().astype(np.float64), leaves, _bound(leaves, g_ref, g32), tag=(fid, where, 'window against full set'))
    # and back
    eng.set_row_window(0, 0)
    lp3, g3 = _launch(eng, theta)
    assert torch.equal(lp3, full[0]) and torch.equal(g3, full[1]), (fid, where)


@pytest.mark.parametrize('form', W.FORMS, ids=FORM_IDS)
def test_full_set_returns_after_all_windows(form):
    """All windows in turn on one engine, each still right after the ones before it, then count = 0: the first full-set result
    bit for bit."""
    fid, net = W.form_id(form), (form[0], form[1])
    X, y, theta = _window_problem(form)
    eng = _engine(form, X, y)
    leaves = L.fcn_leaves(W.ospec_of(net))
    seed = W.seed_of(form, W.WINDOW_N)
    full = _launch(eng, theta)
    for begin, count in W.WINDOW_CASES:
        eng.set_row_window(begin, count)
        lp, g = _launch(eng, theta)
        _check(fid, W.window_id((begin, count)) + ' in sequence', lp.numpy(), g.numpy(), W.reference(net, W.WINDOW_N, seed, begin, count), leaves)
    eng.set_row_window(0, 0)
    lp, g = _launch(eng, theta)
    assert torch.equal(lp, full[0]) and torch.equal(g, full[1]), fid
